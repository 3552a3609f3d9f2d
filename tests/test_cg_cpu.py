"""CPU checks (no GPU) of the exact GP by conjugate gradients: the float64 restatement tests/cg_ref.py against the oracle's dense exact
GP, the host-only svgp_lanczos_logdet against numpy.linalg.eigh, and the Python layer's argument checks and dispatch."""
import ctypes as C

import numpy as np
import pytest

import approxgp
import cg_ref as cr
import svgp_oracle as o
from approxgp import _ffi

FAMILIES = [o.KERNEL_SE, o.KERNEL_MATERN32, o.KERNEL_MATERN52]


def _problem(N, d, family, seed=0):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-3, 3, size=(d, N))
    kernel = o.Kernel(family, 1.3, np.full(d, 1 / 0.7))
    y = np.sin(x.sum(0)) + 0.1 * rng.standard_normal(N)
    return kernel, x, y


@pytest.fixture(scope="module")
def solved():
    """one restatement run per family on the (300, 2, 0.1) problem with 16 Rademacher probes, shared"""
    out = {}
    for fam in FAMILIES:
        kernel, x, y = _problem(300, 2, fam)
        z = approxgp.draw_probes(300, 16, 1)
        out[fam] = (kernel, x, y, z, cr.estimate(kernel, x, 0.1, y, z, 1e-10, 2000, grad=True))
    return out


@pytest.mark.parametrize("family", FAMILIES)
def test_unit_probes_give_the_exact_lml(family):
    kernel, x, y = _problem(48, 1, family)
    r = cr.estimate(kernel, x, 0.1, y, cr.unit_probes(48), 1e-12, 2000)
    ref = o.exact_gp_logpdf(kernel, x, 0.1, y)
    assert abs(r["lml"] - ref) <= 1e-10 * abs(ref)
    assert r["iters"].max() <= 48


@pytest.mark.parametrize("family", FAMILIES)
def test_predictions_equal_the_exact_posterior(family):
    kernel, x, y = _problem(300, 2, family)
    xs = np.random.default_rng(5).uniform(-3, 3, size=(2, 65))
    m, v = cr.predict(kernel, x, 0.1, y, xs)
    mr, cov = o.exact_gp_posterior(kernel, x, 0.1, y, xs)
    np.testing.assert_allclose(m, mr, atol=1e-10 * np.abs(mr).max())
    np.testing.assert_allclose(v, np.diag(cov), atol=1e-10 * kernel.variance)
    # and alpha from the iteration reproduces the mean
    alpha = cr.mbcg(lambda P: cr.khat(kernel, x, 0.1) @ P, y, 1e-12, 2000)[0][:, 0]
    np.testing.assert_allclose(o.kernelmatrix(kernel, x, xs).T @ alpha, mr, atol=1e-9 * np.abs(mr).max())


@pytest.mark.parametrize("family", FAMILIES)
def test_unit_probe_gradient_equals_central_differences(family):
    kernel, x, y = _problem(48, 2, family)
    g = cr.estimate(kernel, x, 0.1, y, cr.unit_probes(48), 1e-12, 2000, grad=True)["grad"]
    h = 1e-6

    def f(var, il, diag, mc=0.0):
        return o.exact_gp_logpdf(o.Kernel(family, var, il), x, diag, y - mc)

    il = kernel.inv_lengthscale
    fd = {"variance": (f(1.3 + h, il, 0.1) - f(1.3 - h, il, 0.1)) / (2 * h), "diag": (f(1.3, il, 0.1 + h) - f(1.3, il, 0.1 - h)) / (2 * h),
          "mean_const": (f(1.3, il, 0.1, h) - f(1.3, il, 0.1, -h)) / (2 * h)}
    fil = np.zeros(2)
    for c in range(2):
        e = np.zeros(2)
        e[c] = h
        fil[c] = (f(1.3, il + e, 0.1) - f(1.3, il - e, 0.1)) / (2 * h)
    for k in ("variance", "diag", "mean_const"):
        assert abs(g[k] - fd[k]) <= 1e-6 * max(abs(fd[k]), 1.0), (k, g[k], fd[k])
    np.testing.assert_allclose(g["inv_lengthscale"], fil, atol=1e-6 * np.abs(fil).max())


def test_iteration_converges_to_the_dense_estimator(solved):
    for fam, (kernel, x, y, z, r) in solved.items():
        dn = cr.dense_estimate(kernel, x, 0.1, y, z)
        assert abs(r["lml"] - dn["lml"]) <= 1e-8 * abs(dn["lml"])
        for k in ("variance", "diag", "mean_const"):
            assert abs(r["grad"][k] - dn["grad"][k]) <= 1e-7 * max(abs(dn["grad"][k]), 1.0), (fam, k)
        np.testing.assert_allclose(r["grad"]["inv_lengthscale"], dn["grad"]["inv_lengthscale"],
                                   atol=1e-7 * np.abs(dn["grad"]["inv_lengthscale"]).max())
        assert r["iters"].max() <= 349 and r["rel"].max() <= 1e-10


def test_float32_kmv_chain_is_the_float64_product_to_float32_accuracy():
    kernel, x, y = _problem(257, 9, o.KERNEL_MATERN52)
    x32 = x.astype(np.float32).astype(np.float64)
    V = np.random.default_rng(2).standard_normal((257, 3)).astype(np.float32)
    ref = cr.khat(o.Kernel(kernel.family, 1.3, kernel.inv_lengthscale.astype(np.float32).astype(np.float64)), x32, 0.1) @ V.astype(np.float64)
    err = np.abs(cr.kmv_f32(kernel, x32, V, 0.1) - ref).max()
    assert err <= 1e-4 * np.abs(ref).max()


@pytest.mark.parametrize("iters", [1, 2, 44, 349])
def test_lanczos_logdet_matches_eigh(solved, iters):
    lib = _ffi.load_library()
    dp = C.POINTER(C.c_double)
    found = 0
    for fam, (kernel, x, y, z, r) in solved.items():
        ca, cb = r["coef"]
        for t in range(len(ca)):
            if len(ca[t]) < iters:
                continue
            a, b = np.array(ca[t][:iters]), np.array(cb[t][:iters])
            out = C.c_double()
            assert lib.svgp_lanczos_logdet(a.ctypes.data_as(dp), b.ctypes.data_as(dp), iters, C.byref(out)) == _ffi.OK
            ref = cr.lanczos_quad(a, b)
            assert abs(out.value - ref) <= 1e-12 * max(abs(ref), 1e-300), (fam, t, out.value, ref)
            found += 1
    if iters < 349:
        assert found
    else:   # the (300, 2, 0.01) problem, stopped by maxiter = 349 before it reaches the tolerance: sets of exactly 349 steps
        kernel, x, y = _problem(300, 2, o.KERNEL_MATERN32)
        ca, cb = cr.estimate(kernel, x, 0.01, y, approxgp.draw_probes(300, 2, 3), 1e-15, 349)["coef"]
        for t in range(3):
            a, b = np.array(ca[t]), np.array(cb[t])
            assert len(a) == 349
            out = C.c_double()
            assert lib.svgp_lanczos_logdet(a.ctypes.data_as(dp), b.ctypes.data_as(dp), 349, C.byref(out)) == _ffi.OK
            ref = cr.lanczos_quad(a, b)
            assert abs(out.value - ref) <= 1e-12 * abs(ref), (t, out.value, ref)
    bad = C.c_double()
    one = np.ones(1)
    assert lib.svgp_lanczos_logdet(None, one.ctypes.data_as(dp), 1, C.byref(bad)) == _ffi.INVALID_ARG
    assert lib.svgp_lanczos_logdet(one.ctypes.data_as(dp), one.ctypes.data_as(dp), 0, C.byref(bad)) == _ffi.INVALID_ARG
    neg = -np.ones(1)
    assert lib.svgp_lanczos_logdet(neg.ctypes.data_as(dp), one.ctypes.data_as(dp), 1, C.byref(bad)) == _ffi.NOT_POSDEF and np.isnan(bad.value)


def test_struct_layouts():
    assert C.sizeof(_ffi.CGDesc) == 64 and _ffi.CGDesc.tol.offset == 48 and _ffi.CGDesc.inv_lengthscale.offset == 24
    assert C.sizeof(_ffi.CGInfo) == 64 and _ffi.CGInfo.max_rel_residual.offset == 16 and _ffi.CGInfo.ms_vector.offset == 56


def test_python_argument_errors_need_no_context(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the GPU was touched")

    monkeypatch.setattr(_ffi, "default_context", boom)
    f = approxgp.GP(approxgp.SqExponentialKernel())
    x, y = np.linspace(0, 1, 9), np.zeros(9)
    cg = approxgp.ConjugateGradients()
    for bad in (dict(tol=0.0), dict(tol=-1.0), dict(maxiter=0), dict(n_probes=-1), dict(probes=np.zeros(3))):
        with pytest.raises(ValueError):
            approxgp.ConjugateGradients(**bad)
    with pytest.raises(_ffi.UnsupportedError):
        approxgp.approx_lml(cg, f(x, np.full(9, 0.1)), y)
    with pytest.raises(_ffi.UnsupportedError):
        approxgp.posterior(cg, f(x, approxgp.Diagonal(np.full(9, 0.1))), y)
    with pytest.raises(ValueError, match="lengths differ"):
        approxgp.approx_lml_and_gradient(cg, f(x, 0.1), np.zeros(8))
    with pytest.raises(ValueError, match="one row per data point"):
        approxgp.approx_lml(approxgp.ConjugateGradients(probes=np.ones((8, 2))), f(x, 0.1), y)
    with pytest.raises(TypeError, match="unexpected keyword"):
        approxgp.approx_lml(cg, f(x, 0.1), y, small_problems="run")
    assert cg.tol_for(np.float32) == 1e-4 and cg.tol_for(np.float64) == 1e-8 and approxgp.ConjugateGradients(tol=1e-3).tol_for(np.float32) == 1e-3
    z = approxgp.draw_probes(7, 3, 0)
    assert z.shape == (7, 3) and set(np.unique(z)) <= {-1.0, 1.0} and z.flags.f_contiguous
    np.testing.assert_array_equal(z, cg.__class__(n_probes=3).probes_for(7))


def test_other_approximations_pass_through_untouched(monkeypatch):
    from approxgp import iterative, nearest_neighbors, vfe

    seen = []
    monkeypatch.setattr(vfe, "approx_lml", lambda *a, **k: seen.append(("lml", a, k)) or 1.0)
    monkeypatch.setattr(vfe, "posterior", lambda *a, **k: seen.append(("post", a, k)) or 2.0)
    monkeypatch.setattr(nearest_neighbors, "approx_lml_and_gradient", lambda *a, **k: seen.append(("grad", a, k)) or 3.0)
    other, fx, y = object(), object(), object()
    assert iterative.approx_lml(other, fx, y, ctx=5, small_problems="decline") == 1.0
    assert iterative.posterior(other, fx, y, dtype=np.float32) == 2.0
    assert iterative.posterior(other) == 2.0
    assert iterative.approx_lml_and_gradient(other, fx, y, anything=7) == 3.0
    assert seen == [("lml", (other, fx, y), dict(ctx=5, small_problems="decline")), ("post", (other, fx, y), dict(dtype=np.float32)),
                    ("post", (other,), {}), ("grad", (other, fx, y), dict(anything=7))]
    assert approxgp.approx_lml is iterative.approx_lml and approxgp.posterior is iterative.posterior
    assert approxgp.approx_lml_and_gradient is iterative.approx_lml_and_gradient
