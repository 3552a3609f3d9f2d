"""CPU checks of the collapsed (Titsias) bound's reference restatement (tests/collapsed_ref.py) against the oracle, and of what the
device path checks before it touches a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import approxgp as ag
import collapsed_ref as cr
import svgp_oracle as o
from approxgp import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(300, 20, 1), (777, 200, 3), (1500, 130, 8)]
JITTER = 1e-5


def _rel(a, b):
    return abs(a - b) / abs(b)


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: "n%d_M%d_d%d" % s)
def prob(request):
    n, M, d = request.param
    kernel, z, x, y, s2 = cr.problem(n, M, d, ard=(d == 8))
    return kernel, z, x, y, s2, cr.collapsed(kernel, z, JITTER, x, s2, y)


def test_restatement_matches_the_oracles_bound(prob):
    kernel, z, x, y, s2, r = prob
    ref = o.titsias_bound(kernel, z, JITTER, x, s2, y)
    assert _rel(r.bound, ref) < 1e-12, (r.bound, ref)
    assert _rel(r.fit + r.trace, r.bound) < 1e-15
    # chunked accumulation (the M x M form at any n) gives the same numbers
    r2 = cr.collapsed(kernel, z, JITTER, x, s2, y, chunk=97)
    assert _rel(r2.bound, r.bound) < 1e-12


@pytest.mark.parametrize("centered", [False, True])
def test_elbo_at_the_restated_q_is_the_bound(prob, centered):
    kernel, z, x, y, s2, r = prob
    sva, _ = cr.optimal_sva(kernel, z, JITTER, x, s2, y, centered=centered)
    assert np.allclose(sva.Lq, np.tril(sva.Lq)) and np.all(np.diag(sva.Lq) > 0)
    assert _rel(o.elbo(sva, x, y, sigma2=s2), r.bound) < 1e-12


def test_nonzero_mean_const_is_a_shift_of_y():
    kernel, z, x, y, s2 = cr.problem(300, 20, 1, mean_const=0.7)
    a = cr.collapsed(kernel, z, JITTER, x, s2, y, mean_const=0.7)
    b = cr.collapsed(kernel, z, JITTER, x, s2, y - 0.7)
    assert _rel(a.bound, b.bound) < 1e-13
    sva, _ = cr.optimal_sva(kernel, z, JITTER, x, s2, y, mean_const=0.7, centered=True)
    assert _rel(o.elbo(sva, x, y, sigma2=s2), a.bound) < 1e-12


def test_whitened_mean_agrees_with_the_oracles_sigma_route(prob):
    """Not tighter than 1e-6: the oracle's Sigma^-1 route is itself only good to 4e-9 ... 8e-8 at jitter 1e-5."""
    kernel, z, x, y, s2, r = prob
    m, S = o.optimal_variational_posterior(kernel, z, JITTER, x, s2, y)
    me, Se = o.whiten(kernel, z, JITTER, m, S)
    assert np.max(np.abs(me - r.m_w)) < 1e-6 * max(1.0, np.max(np.abs(r.m_w)))
    assert np.max(np.abs(Se - r.S_w)) < 1e-6


def test_envelope_gradient_matches_central_differences(prob):
    kernel, z, x, y, s2, r = prob
    bound, val, g = cr.bound_grad(kernel, z, JITTER, x, s2, y)
    assert _rel(val, bound) < 1e-12
    assert np.max(np.abs(g["m"])) < 1e-8 * max(1.0, abs(bound)) and np.max(np.abs(g["Lq"])) < 1e-8 * max(1.0, abs(bound))

    def cd(f, h):
        return (f(h) - f(-h)) / (2 * h)

    il = kernel.inv_lengthscale
    tb = o.titsias_bound
    fd_var = cd(lambda h: tb(o.Kernel(kernel.family, kernel.variance + h, il), z, JITTER, x, s2, y), 1e-5)
    fd_s2 = cd(lambda h: tb(kernel, z, JITTER, x, s2 + h, y), 1e-6)

    def il_shift(h):
        v = il.copy()
        v[0] += h
        return tb(o.Kernel(kernel.family, kernel.variance, v), z, JITTER, x, s2, y)

    def z_shift(h):
        zz = z.copy()
        zz[0, 3] += h
        return tb(kernel, zz, JITTER, x, s2, y)

    fd_il, fd_z = cd(il_shift, 1e-5), cd(z_shift, 1e-5)
    # an isotropic kernel shares one inverse lengthscale: shifting entry 0 alone is still the partial derivative g[0]
    for name, got, want in (("variance", g["variance"], fd_var), ("lik_sigma2", g["lik_sigma2"], fd_s2),
                            ("inv_lengthscale[0]", g["inv_lengthscale"][0], fd_il), ("z[0, 3]", g["z"][0, 3], fd_z)):
        assert abs(got - want) <= 1e-5 * abs(want), (name, got, want)


def test_z_equal_x_is_exact_gp_regression():
    """test/SparseVariationalApproximationModule.jl:99-134: with z = x the bound is logpdf(fx, y), the posterior is exact GPR's."""
    rng = np.random.default_rng(5)
    x = np.sort(rng.random(40))[None, :] * 4.0
    # z = x reproduces exact GPR up to O(jitter / sigma^2) (Qff = K (K + jitter I)^-1 K): a Matern-3/2 Kuu is well enough conditioned
    # for a jitter of 1e-9, which keeps that difference two orders below the 1e-6 asked for
    kernel = o.Kernel(o.KERNEL_MATERN32, 1.2, [1.5])
    s2, jitter = 0.1, 1e-9
    y = np.sin(2 * x[0]) + np.sqrt(s2) * rng.standard_normal(40)
    r = cr.collapsed(kernel, x, jitter, x, s2, y)
    assert _rel(r.bound, o.exact_gp_logpdf(kernel, x, s2, y)) < 1e-5
    xs = np.linspace(-0.5, 4.5, 25)[None, :]
    mean, cov = cr.posterior_at(kernel, x, jitter, x, s2, y, xs)
    em, ec = o.exact_gp_posterior(kernel, x, s2, y, xs)
    assert np.max(np.abs(mean - em)) < 1e-6 and np.max(np.abs(cov - ec)) < 1e-6


def test_argument_checks_happen_before_the_gpu():
    f, g = ag.GP(ag.SqExponentialKernel()), ag.GP(ag.SqExponentialKernel())
    z, x, y = np.linspace(0, 1, 20), np.linspace(0, 1, 100), np.zeros(100)
    vfe = ag.VFE(f(z, 1e-6))
    with pytest.raises(RuntimeError, match="homoscedastic"):                       # SVA:319-327, the SVGP path's text
        ag.elbo(vfe, f(x, np.full(100, 0.1)), y)
    with pytest.raises(RuntimeError, match="homoscedastic"):
        ag.optimal_variational_posterior(f(z, 1e-6), f(x, np.full(100, 0.1)), y)
    with pytest.raises(ValueError, match="Gaussian"):
        ag.elbo(vfe, ag.LatentFiniteGP(f(x, 1e-6), ag.BernoulliLikelihood()), y)
    with pytest.raises(ValueError, match="not consistent"):                        # SVA:347-351
        ag.elbo(vfe, g(x, 0.1), y)
    for call in (ag.elbo, ag.approx_lml, ag.elbo_and_gradient, ag.posterior):      # declined exactly as sva.elbo declines
        with pytest.raises(ag.DeclinedError):
            call(vfe, f(x, 0.1), y, small_problems="decline")
    sva = ag.SparseVariationalApproximation(f(z, 1e-6), ag.MvNormal(np.zeros(20), np.eye(20)))
    with pytest.raises(ag.DeclinedError):
        ag.elbo(sva, f(x, 0.1), y, small_problems="decline")                       # the dispatch passes the SVGP call on unchanged
    with pytest.raises(TypeError):
        ag.VFE(z)
    with pytest.raises(TypeError, match="unexpected keyword"):
        ag.elbo(vfe, f(x, 0.1), y, num_data=10)


def test_abi_struct_and_julia_binding_cover_the_new_calls():
    assert C.sizeof(_ffi.CollapsedTerms) == 64 and _ffi.CollapsedTerms.n_points.offset == 40
    assert _ffi.CollapsedTerms.chol_info.offset == 48 and _ffi.CollapsedTerms.chol_info_b.offset == 52
    new = {"svgp_collapsed_bound", "svgp_collapsed_q", "svgp_collapsed_grad"}
    header = open(os.path.join(ROOT, "include", "svgp_mi355x.h")).read()
    declared = set(re.findall(r"\b(svgp_[a-z_0-9]+)\s*\(", header))
    assert new <= declared and declared == set(_ffi.SYMBOLS)
    lib = _ffi.load_library()
    assert all(hasattr(lib, n) for n in new)
    src = open(os.path.join(ROOT, "integration", "julia", "src", "SVGPMI355X.jl")).read()
    called = set(re.findall(r"ccall\(\(:(svgp_[a-z_0-9]+), lib\)", src))
    assert new <= called <= set(_ffi.SYMBOLS)
    jl = re.findall(r"(\w+)::(?:Int32|Int64|Float64)", src[src.index("struct CollapsedTerms"):src.index("end", src.index("struct CollapsedTerms"))])
    assert jl == [f[0] for f in _ffi.CollapsedTerms._fields_]
    # a NULL context is refused before anything else
    assert lib.svgp_collapsed_bound(None, None, None, 0, 1, None, None) == _ffi.INVALID_ARG
