"""CPU checks of the float64 restatement tests/collapsed_noise_ref.py (the collapsed bound with per-point noise variances and any prior
mean), and of the Python argument checks that need no GPU."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import approxgp as ag
import collapsed_noise_ref as cn
import collapsed_ref as cr
import svgp_oracle as o
from approxgp import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
JITTER = 1e-6


def _rel(a, b):
    return abs(a - b) / abs(b)


def _small(seed=1, n=40, M=6, d=1, family=o.KERNEL_SE, decades=1.7):
    # (noise spanning a factor of ~50, as the issue's own float64 check)
    return cn.problem(n, M, d, seed=seed, family=family, ard=d > 1, noise_decades=decades)


@pytest.mark.parametrize("family,d", [(o.KERNEL_SE, 1), (o.KERNEL_MATERN32, 3), (o.KERNEL_MATERN52, 2)])
def test_restatement_equals_the_dense_expression(family, d):
    kernel, z, x, y, s2, s, mux, muz = _small(seed=2, n=60, M=7, d=d, family=family, decades=4.0)
    r = cn.collapsed(kernel, z, JITTER, x, s2, s, y, mean_const=0.3, mux=mux, chunk=17)   # (chunked sums: 17 does not divide 60)
    bound, fit, trace = cn.dense_bound(kernel, z, JITTER, x, s2, s, y, mean_const=0.3, mux=mux)
    assert _rel(r.bound, bound) < 1e-12 and _rel(r.fit, fit) < 1e-12 and abs(r.trace - trace) < 1e-12 * abs(bound)


def test_constant_noise_and_zero_mean_is_the_existing_restatement():
    kernel, z, x, y, s2, s, mux, muz = _small(seed=3, n=50, M=8, d=2)
    old = cr.collapsed(kernel, z, JITTER, x, s2 + 0.07, y, mean_const=-0.2)
    new = cn.collapsed(kernel, z, JITTER, x, s2, np.full(50, 0.07), y, mean_const=-0.2)
    assert _rel(new.bound, old.bound) < 1e-13 and _rel(new.fit, old.fit) < 1e-13 and _rel(new.trace, old.trace) < 1e-13
    assert _rel(new.logdet_B, old.logdet_B) < 1e-13
    assert np.abs(new.m_w - old.m_w).max() < 1e-12 * np.abs(old.m_w).max() and np.abs(new.Lq_w - old.Lq_w).max() < 1e-12
    # ... and a mean offset is a shift of y
    a = cn.collapsed(kernel, z, JITTER, x, s2, s, y, mux=mux)
    b = cn.collapsed(kernel, z, JITTER, x, s2, s, y - mux)
    assert _rel(a.bound, b.bound) < 1e-14
    # the envelope gradient of the constant case is the existing one, and lik_sigma2 = sum s_bar keeps its meaning
    _, _, g_old = cr.bound_grad(kernel, z, JITTER, x, s2 + 0.07, y, mean_const=-0.2)
    _, g_new = cn.bound_grad(kernel, z, JITTER, x, s2, np.full(50, 0.07), y, mean_const=-0.2)
    for k in ("variance", "lik_sigma2", "mean_const"):
        assert _rel(g_new[k], g_old[k]) < 1e-10, k
    assert np.abs(g_new["z"] - g_old["z"]).max() < 1e-10 * np.abs(g_old["z"]).max()
    assert np.abs(g_new["m"]).max() < 1e-9 and np.abs(g_new["Lq"]).max() < 1e-9      # d elbo / d q = 0 at the optimal q


def test_z_equal_x_is_exact_gp_regression_with_heteroscedastic_noise():
    rng = np.random.default_rng(5)
    n = 40
    x = np.sort(rng.random(n))[None, :] * 4.0
    kernel = o.Kernel(o.KERNEL_MATERN32, 1.2, [1.5])
    s2, jitter = 0.05, 1e-9
    s = 0.5 * rng.random(n) ** 2
    mean = 0.4 + 0.3 * x[0]
    y = mean + np.sin(2 * x[0]) + np.sqrt(s2 + s) * rng.standard_normal(n)
    r = cn.collapsed(kernel, x, jitter, x, s2, s, y, mean_const=0.4, mux=0.3 * x[0])
    K = o.kernelmatrix(kernel, x) + np.diag(s2 + s)
    L = np.linalg.cholesky(K)
    a = np.linalg.solve(L, y - mean)
    exact = -0.5 * n * math.log(2 * math.pi) - float(np.sum(np.log(np.diag(L)))) - 0.5 * float(a @ a)
    assert _rel(r.bound, exact) < 1e-5     # (O(jitter / sigma^2), as tests/test_collapsed_cpu.py)


def test_every_gradient_block_against_central_differences():
    kernel, z, x, y, s2, s, mux, muz = _small(seed=4, n=40, M=6, d=2, family=o.KERNEL_MATERN52)
    mc = 0.25
    _, g = cn.bound_grad(kernel, z, JITTER, x, s2, s, y, mean_const=mc, mux=mux, want_x=True)

    def f(kernel=kernel, z=z, x=x, s2=s2, s=s, mc=mc, mux=mux):
        return cn.collapsed(kernel, z, JITTER, x, s2, s, y, mean_const=mc, mux=mux).bound

    def cd(fun, h):
        return (fun(h) - fun(-h)) / (2 * h)

    def vec_cd(make, size, h, scale=None):
        out = np.zeros(size)
        for i in range(size):
            e = np.zeros(size)
            e[i] = 1.0
            out[i] = cd(lambda t: make(t * e), h if scale is None else h * scale[i])
        return out

    assert _rel(g["variance"], cd(lambda t: f(kernel=o.Kernel(kernel.family, kernel.variance + t, kernel.inv_lengthscale)), 1e-6)) < 1e-6
    il = vec_cd(lambda e: f(kernel=o.Kernel(kernel.family, kernel.variance, kernel.inv_lengthscale + e)), 2, 1e-6)
    assert np.abs(g["inv_lengthscale"] - il).max() < 1e-6 * np.abs(il).max()
    assert _rel(g["lik_sigma2"], cd(lambda t: f(s2=s2 + t), 1e-7)) < 1e-5
    assert _rel(g["mean_const"], cd(lambda t: f(mc=mc + t), 1e-6)) < 1e-7
    zb = vec_cd(lambda e: f(z=z + e.reshape(z.shape)), z.size, 1e-6).reshape(z.shape)
    assert np.abs(g["z"] - zb).max() < 1e-6 * np.abs(zb).max()
    xb = vec_cd(lambda e: f(x=x + e.reshape(x.shape)), x.size, 1e-6).reshape(x.shape)
    assert np.abs(g["x"] - xb).max() < 1e-6 * np.abs(xb).max()
    mb = vec_cd(lambda e: f(mux=mux + e), 40, 1e-6)
    assert np.abs(g["mean_x"] - mb).max() < 1e-7 * np.abs(mb).max()
    # steps of 1e-3 sigma_j^2: the noise spans a factor of ~50, one absolute step cannot serve every entry; 1e-5 of the largest
    # entry is the differences' own noise
    sb = vec_cd(lambda e: f(s=s + e), 40, 1e-3, scale=s2 + s)
    assert np.abs(g["noise"] - sb).max() < 1e-5 * np.abs(sb).max()
    assert _rel(float(np.sum(g["noise"])), g["lik_sigma2"]) < 1e-14
    assert np.abs(g["m"]).max() < 1e-8 and np.abs(g["Lq"]).max() < 1e-8


def test_bound_is_the_elbo_at_the_written_q():
    """Gaussian expectation with sigma_j^2 minus the KL at the optimal q, Centered with muz, from the oracle's own marginals."""
    kernel, z, x, y, s2, s, mux, muz = _small(seed=6, n=40, M=6, d=1)
    mc = -0.3
    r = cn.collapsed(kernel, z, JITTER, x, s2, s, y, mean_const=mc, mux=mux)
    m, Lq = cn.optimal_q(r, mean_const=mc, muz=muz, centered=True)
    # mean(fz) = mc + muz: the oracle's SVA knows constants only, so shift m by muz and add mux to its marginal means
    sva = o.SVA(kernel, z, m - muz, Lq, jitter=JITTER, mean_const=mc, centered=True)
    mu, sd = o.marginals(o.posterior(sva), x)
    sig = s2 + s
    e = -0.5 * np.log(2 * np.pi * sig) - ((y - mu - mux) ** 2 + sd * sd) / (2 * sig)
    assert _rel(float(np.sum(e)) - o.prior_kl(sva), r.bound) < 1e-12


def test_argument_checks_need_no_gpu():
    f = ag.GP(ag.SqExponentialKernel())
    z, x, y = np.linspace(0, 1, 20), np.linspace(0, 1, 100), np.zeros(100)
    vfe = ag.VFE(f(z, 1e-6))
    bad = np.full(100, 0.1)
    bad[17] = 0.0
    for sy in (bad, -bad, np.where(np.arange(100) == 3, np.nan, 0.1)):
        for call in (ag.elbo, ag.elbo_and_gradient, ag.posterior):
            with pytest.raises(ValueError, match="positive"):
                call(vfe, f(x, ag.Diagonal(sy)), y)
        with pytest.raises(ValueError, match="positive"):
            ag.optimal_variational_posterior(f(z, 1e-6), f(x, ag.Diagonal(sy)), y)
    for sy in (np.full(99, 0.1), np.full((100, 1), 0.1), np.full(101, 0.1)):
        with pytest.raises(ValueError, match="one variance per point"):
            ag.elbo(vfe, f(x, ag.Diagonal(sy)), y)
    # a valid vector passes every check that needs no GPU: the offload rule is the next thing asked
    with pytest.raises(ag.DeclinedError):
        ag.elbo(vfe, f(x, ag.Diagonal(np.full(100, 0.1))), y, small_problems="decline")
    # ... and so does a CustomMean prior
    g = ag.GP(ag.CustomMean(lambda t: np.sin(np.asarray(t)).reshape(-1)), ag.SqExponentialKernel())
    with pytest.raises(ag.DeclinedError):
        ag.elbo(ag.VFE(g(z, 1e-6)), g(x, ag.Diagonal(np.full(100, 0.1))), y, small_problems="decline")
    # the SVGP path keeps the reference's error (SVA:319-327)
    sva = ag.SparseVariationalApproximation(f(z, 1e-6), ag.MvNormal(np.zeros(20), np.eye(20)))
    for sy in (np.full(100, 0.1), ag.Diagonal(np.full(100, 0.1))):
        with pytest.raises(RuntimeError, match="homoscedastic"):
            ag.elbo(sva, f(x, sy), y)
    # a plain vector Σy keeps its refusal in the VFE path too: the non-isotropic noise is asked for by type, Diagonal(v)
    with pytest.raises(RuntimeError, match="homoscedastic"):
        ag.elbo(vfe, f(x, np.full(100, 0.1)), y)
    with pytest.raises(TypeError, match="unexpected keyword"):
        ag.elbo_and_gradient(vfe, f(x, 0.1), y, wrt_sigma=True)
    # host-side argument packing
    pn, keep = _ffi.point_noise(np.arange(5.0), 5, _ffi.F32)
    assert keep.dtype == np.float32 and pn.on_device == 0 and pn.reserved == 0
    with pytest.raises(ValueError, match="one entry per point"):
        _ffi.point_noise(np.arange(5.0), 6, _ffi.F64)


def test_abi_structs_symbols_and_julia_binding():
    for st, first in ((_ffi.PointNoise, "s"), (_ffi.PointNoiseGrad, "s_bar")):
        assert C.sizeof(st) == 16 and st._fields_[0][0] == first and st.on_device.offset == 8 and st.reserved.offset == 12
    new = {"svgp_collapsed_bound_with_noise", "svgp_collapsed_q_with_noise", "svgp_collapsed_grad_with_noise"}
    header = open(os.path.join(ROOT, "include", "svgp_mi355x.h")).read()
    declared = set(re.findall(r"\b(svgp_[a-z_0-9]+)\s*\(", header))
    assert new <= declared and declared == set(_ffi.SYMBOLS)
    assert "svgp_point_noise;" in header and "svgp_point_noise_grad;" in header
    lib = _ffi.load_library()
    assert all(hasattr(lib, n) for n in new) and lib.svgp_version() == 5
    src = open(os.path.join(ROOT, "integration", "julia", "src", "SVGPMI355X.jl")).read()
    called = set(re.findall(r"ccall\(\(:(svgp_[a-z_0-9]+), lib\)", src))
    assert new <= called <= set(_ffi.SYMBOLS)
    # a NULL context is refused before anything else
    assert lib.svgp_collapsed_bound_with_noise(None, None, None, 0, 1, None, None, None, None) == _ffi.INVALID_ARG
    assert lib.svgp_collapsed_q_with_noise(None, None, None, 0, 1, None, None, None, None, None) == _ffi.INVALID_ARG
    assert lib.svgp_collapsed_grad_with_noise(None, None, None, 0, 1, None, None, None, None, None, None, None, None) == _ffi.INVALID_ARG
