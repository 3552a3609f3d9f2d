"""CPU checks that pin the natural-gradient step's numpy restatement (tests/natgrad_ref.py) to the oracle, and of what the device
path declares before it touches a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import natgrad_ref as nr
import svgp_oracle as o
from approxgp import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JITTER = 1e-5


def _block_err(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def test_step_is_theta_plus_gamma_times_the_gradient_in_the_expectation_parameters():
    """theta' = theta + gamma dL/d eta, the derivative taken by central differences of the oracle's ELBO as a function of
    eta = (m, S + m m') (M = 5, n = 50, d = 1, Bernoulli-logistic GH-20, num_data = 120, gamma = 0.3).  Measured 1e-8; asserted 1e-6."""
    M, n, gamma, num_data, lik = 5, 50, 0.3, 120.0, o.LIK_BERNOULLI_LOGISTIC
    kernel, z, x, y, _, m0, Lq0 = nr.problem(n, M, 1, lik=lik, seed=3)
    S0 = Lq0 @ Lq0.T
    eta1, eta2 = m0.copy(), S0 + np.outer(m0, m0)

    def L(e1, e2):
        S = e2 - np.outer(e1, e1)
        sva = o.SVA(kernel, z, e1, np.linalg.cholesky(0.5 * (S + S.T)), jitter=JITTER)
        return o.elbo(sva, x, y, lik=lik, num_data=num_data, quadrature_n=20)

    h = 1e-5
    g1 = np.zeros(M)
    for i in range(M):
        e = np.zeros(M)
        e[i] = h
        g1[i] = (L(eta1 + e, eta2) - L(eta1 - e, eta2)) / (2 * h)
    g2 = np.zeros((M, M))   # <g2, d eta2> = dL for symmetric d eta2
    for i in range(M):
        for j in range(i + 1):
            E = np.zeros((M, M))
            E[i, j] = E[j, i] = h
            dL = (L(eta1, eta2 + E) - L(eta1, eta2 - E)) / (2 * h)
            g2[i, j] = g2[j, i] = dL if i == j else 0.5 * dL
    Lam = np.linalg.inv(S0)
    theta1_fd = Lam @ m0 + gamma * g1
    Lam_fd = Lam - 2.0 * gamma * g2      # theta2 = -Lambda / 2
    new = nr.step(o.SVA(kernel, z, m0, Lq0, jitter=JITTER), x, y, lik=lik, num_data=num_data, gamma=gamma, quadrature_n=20)
    Lam_new = np.linalg.inv(new.Lq @ new.Lq.T)
    e_lam, e_th = _block_err(Lam_new, Lam_fd), _block_err(Lam_new @ new.m, theta1_fd)
    print(f"natural-parameter identity: Lambda' {e_lam:.2e}, Lambda' m' {e_th:.2e}")
    assert e_lam < 1e-6 and e_th < 1e-6


@pytest.mark.parametrize("centered", [False, True], ids=["noncentered", "centered_mc0.3"])
def test_full_step_gaussian_full_batch_is_the_titsias_optimum(centered):
    """gamma = 1, Gaussian likelihood, full batch: the step lands on optimal_variational_posterior and its ELBO is titsias_bound, from
    any starting q (n = 777, M = 200, d = 3), to 1e-10."""
    import collapsed_ref as cr

    mc = 0.3 if centered else 0.0
    kernel, z, x, y, s2, m0, Lq0 = nr.problem(777, 200, 3, ard=True, mean_const=mc)
    start = nr.start_sva(kernel, z, JITTER, m0, Lq0, mean_const=mc, centered=centered)
    new = nr.step(start, x, y, lik=o.LIK_GAUSSIAN, sigma2=s2, gamma=1.0)
    bound = o.titsias_bound(kernel, z, JITTER, x, s2, y - mc)
    val = o.elbo(new, x, y, lik=o.LIK_GAUSSIAN, sigma2=s2)
    m_opt, S_opt = o.optimal_variational_posterior(kernel, z, JITTER, x, s2, y - mc)   # u-space, ZeroMean
    if centered:
        m_new, S_new = new.m - mc, new.Lq @ new.Lq.T
    else:
        m_opt, S_opt = o.whiten(kernel, z, JITTER, m_opt, S_opt)
        m_new, S_new = new.m, new.Lq @ new.Lq.T
    ref = cr.collapsed(kernel, z, JITTER, x, s2, y, mean_const=mc)    # the second, M-sized route to the same optimum
    e_b, e_m, e_S = abs(val - bound) / abs(bound), _block_err(m_new, m_opt), _block_err(S_new, S_opt)
    print(f"gamma = 1: bound {e_b:.2e}, m {e_m:.2e}, S {e_S:.2e} against optimal_variational_posterior; "
          f"against the M-sized form m {_block_err(nr.whitened(new)[0], ref.m_w):.2e} S {_block_err(nr.whitened(new)[1], ref.S_w):.2e}")
    assert e_b < 1e-10
    assert _block_err(nr.whitened(new)[0], ref.m_w) < 1e-10 and _block_err(nr.whitened(new)[1], ref.S_w) < 1e-10
    assert e_m < 1e-10 and e_S < 1e-10
    g = o.elbo_grad(new, x, y, lik=o.LIK_GAUSSIAN, sigma2=s2)[1]
    g0 = o.elbo_grad(start, x, y, lik=o.LIK_GAUSSIAN, sigma2=s2)[1]
    assert np.abs(g["m"]).max() < 1e-6 * np.abs(g0["m"]).max() and np.abs(g["Lq"]).max() < 1e-6 * np.abs(g0["Lq"]).max()


@pytest.mark.parametrize("centered", [False, True], ids=["noncentered", "centered"])
@pytest.mark.parametrize("lik,qn", [(o.LIK_BERNOULLI_LOGISTIC, 20), (o.LIK_POISSON_EXP, 0)], ids=["bernoulli_gh20", "poisson"])
def test_elbo_rises_over_eight_half_steps(lik, qn, centered):
    kernel, z, x, y, _, m0, Lq0 = nr.problem(640, 129, 2, lik=lik, seed=1)
    sva = nr.start_sva(kernel, z, JITTER, m0, Lq0, centered=centered)
    vals = [o.elbo(sva, x, y, lik=lik, num_data=2000.0, quadrature_n=qn)]
    for _ in range(8):
        sva = nr.step(sva, x, y, lik=lik, num_data=2000.0, gamma=0.5, quadrature_n=qn)
        vals.append(o.elbo(sva, x, y, lik=lik, num_data=2000.0, quadrature_n=qn))
    print("elbo:", " ".join(f"{v:.6f}" for v in vals))
    assert all(b > a for a, b in zip(vals, vals[1:]))


def test_the_three_symbols_exist_with_the_declared_signatures():
    new = {"svgp_natgrad_step": 12, "svgp_natgrad_step_ext": 15, "svgp_model_update_keep_q": 3}
    header = open(os.path.join(ROOT, "include", "svgp_mi355x.h")).read()
    lib = _ffi.load_library()
    ctype_of = {"double": C.c_double, "int64_t": C.c_int64, "int32_t": C.c_int32}
    for name, nargs in new.items():
        proto = re.search(r"int32_t\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert proto, name
        args = [a.strip() for a in proto.group(1).replace("\n", " ").split(",")]
        res, argtypes = _ffi.SYMBOLS[name]
        assert res is C.c_int32 and len(args) == len(argtypes) == nargs
        for a, t in zip(args, argtypes):
            if "*" in a:
                assert t is C.c_void_p or issubclass(t, C._Pointer), (name, a)
            else:
                assert t is ctype_of[a.split()[0]], (name, a)
        assert hasattr(lib, name)
    # a NULL context is refused before anything else
    assert lib.svgp_natgrad_step(None, None, None, 0, 1, 0.0, 1.0, None, None, None, None, None) == _ffi.INVALID_ARG
    assert lib.svgp_natgrad_step_ext(None, None, None, 0, 1, 0.0, 1.0, 0.0, None, None, None, None, None, None, None) == _ffi.INVALID_ARG
    assert lib.svgp_model_update_keep_q(None, None, None) == _ffi.INVALID_ARG
    src = open(os.path.join(ROOT, "integration", "julia", "src", "SVGPMI355X.jl")).read()
    called = set(re.findall(r"ccall\(\(:(svgp_[a-z_0-9]+), lib\)", src))
    assert set(new) <= called
