"""CPU checks (no GPU) of the exact GP by conjugate gradients with per-point noise variances: the restatement tests/cg_noise_ref.py
against dense closed forms, its Woodbury preconditioner with a diagonal D against numpy.linalg, and the Python layer's argument checks.
Inputs: test_gpu_cg.py's x, y, variance 1.3, lengthscale 0.7; s = exp(U[log 0.02, log 0.5]) from default_rng(11), diag 0.05,
mean_const 0.25.  cond(Khat) is 2.3e2 to 4.6e2 on them.

Bounds (the restatement's own error on these inputs, N = 48 d = 1 and N = 300 d = 2, every family): lml with unit probes against the
dense exact GP 1e-14 (float64, tol 1e-12, at most 170 iterations) and 1.2e-6 (float32, tol 1e-5, at most 100 iterations); s_bar with
16 Rademacher probes (draw_probes(N, 16, 4), the GPU suite's) against the dense-solve estimator of the same probes, relative to its
largest entry, 3.8e-12 (float64) and 3.7e-5 (float32).  With unit probes the estimator is the exact gradient 1/2 (alpha^2 - diag Khat^-1),
which is asserted on the dense forms.  Every figure is printed."""
import numpy as np
import pytest

import approxgp
import cg_noise_ref as nr
import cg_ref as cr
import svgp_oracle as o
from approxgp import _ffi

F64, F32 = np.float64, np.float32
FAMILIES = [o.KERNEL_SE, o.KERNEL_MATERN32, o.KERNEL_MATERN52]
VAR, LS, MC = 1.3, 0.7, 0.25


def _problem(N, d, family, dtype):
    x, y = nr.xy(N, d)
    x = x.astype(dtype).astype(F64)
    kernel = o.Kernel(family, float(dtype(VAR)), np.full(d, 1 / LS).astype(dtype).astype(F64))
    s = nr.noise_vector(N)
    return kernel, x, (y - MC).astype(dtype).astype(F64), s, nr.sigma2(nr.DIAG, s, dtype)


@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("N,d", [(48, 1), (300, 2)])
def test_restatement_against_the_dense_exact_gp(N, d, family, dtype):
    kernel, x, delta, s, sig2 = _problem(N, d, family, dtype)
    cond = float(np.linalg.cond(nr.khat(kernel, x, sig2)))
    tol = 1e-12 if dtype == F64 else 1e-5
    z = cr.unit_probes(N)
    r = nr.estimate(kernel, x, nr.DIAG, s, delta, z, tol, 2000, dtype, grad=True)
    ref = nr.dense_lml(kernel, x, sig2, delta)
    de = nr.dense_estimate(kernel, x, sig2, delta, z)
    sb = de["grad"]["noise"]
    e_lml = abs(r["lml"] - ref) / abs(ref)
    zr = approxgp.draw_probes(N, 16, 4)
    sr = nr.estimate(kernel, x, nr.DIAG, s, delta, zr, tol, 2000, dtype, grad=True)["grad"]["noise"]
    sd = nr.dense_estimate(kernel, x, sig2, delta, zr)["grad"]["noise"]
    e_sb = float(np.abs(sr.astype(F64) - sd).max() / np.abs(sd).max())
    e_unit = float(np.abs(r["grad"]["noise"].astype(F64) - sb).max() / np.abs(sb).max())
    e_exact = float(np.abs(nr.dense_noise_gradient(kernel, x, sig2, delta) - sb).max() / np.abs(sb).max())
    print(f"N{N} d{d} k{family} {np.dtype(dtype).name}: cond {cond:.2e}, iterations {r['iters'].max()}, lml {e_lml:.2e}, s_bar {e_sb:.2e} (Rademacher), {e_unit:.2e} (unit), "
          f"unit-probe estimator against 1/2 (alpha^2 - diag Khat^-1) {e_exact:.1e}")
    assert 2.3e2 <= cond <= 4.6e2
    assert r["iters"].max() <= (170 if dtype == F64 else 100)
    assert e_lml <= (1e-14 if dtype == F64 else 1.2e-6)
    assert e_sb <= (3.8e-12 if dtype == F64 else 3.7e-5)
    assert e_exact <= 1e-12   # with unit probes the estimator is the exact gradient
    g, gd = r["grad"], de["grad"]
    c = 1e-8 if dtype == F64 else 1e-4
    assert abs(g["diag"] - g["noise"].astype(F64).sum()) <= (1e-12 if dtype == F64 else 1e-5) * np.abs(g["noise"]).astype(F64).sum()
    for n in ("variance", "diag", "mean_const"):
        assert abs(g[n] - gd[n]) <= c * max(abs(gd[n]), 1.0), (n, g[n], gd[n])
    assert np.abs(g["inv_lengthscale"] - gd["inv_lengthscale"]).max() <= c * np.abs(gd["inv_lengthscale"]).max()


@pytest.mark.parametrize("family", FAMILIES)
def test_noise_gradient_equals_central_differences(family):
    """d lml / d sigma_i^2 of the dense logpdf by central differences: step 1e-5, truncation h^2 f''' / 6 far below 1e-6 relative"""
    kernel, x, delta, s, sig2 = _problem(48, 1, family, F64)
    g = nr.dense_noise_gradient(kernel, x, sig2, delta)
    h = 1e-5
    for i in np.random.default_rng(3).choice(48, size=8, replace=False):
        e = np.zeros(48)
        e[i] = h
        fd = (nr.dense_lml(kernel, x, sig2 + e, delta) - nr.dense_lml(kernel, x, sig2 - e, delta)) / (2 * h)
        assert abs(fd - g[i]) <= 1e-6 * np.abs(g).max(), (i, fd, g[i])


def test_without_a_vector_the_restatement_is_cg_ref():
    kernel, x, delta, s, sig2 = _problem(48, 1, o.KERNEL_MATERN32, F64)
    z = approxgp.draw_probes(48, 4, 1)
    a = nr.estimate(kernel, x, 0.1, None, delta, z, 1e-10, 2000, grad=True)
    b = cr.estimate(kernel, x, 0.1, delta, z, 1e-10, 2000, grad=True)
    assert a["lml"] == b["lml"] and a["quad"] == b["quad"] and np.array_equal(a["alpha"], b["alpha"])
    assert a["grad"]["diag"] == b["grad"]["diag"] and np.array_equal(a["grad"]["inv_lengthscale"], b["grad"]["inv_lengthscale"])
    assert abs(a["grad"]["variance"] - b["grad"]["variance"]) <= 1e-12 * abs(b["grad"]["variance"])
    assert abs(a["grad"]["noise"].sum() - a["grad"]["diag"]) <= 1e-12 * np.abs(a["grad"]["noise"]).sum()


@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("k", [17, 129])
def test_woodbury_with_a_diagonal_against_numpy(k, dtype):
    kernel, x, delta, s, sig2 = _problem(300, 2, o.KERNEL_MATERN32, dtype)
    zp = np.ascontiguousarray(x[:, np.random.default_rng(5).choice(300, size=k, replace=False)])
    ny = nr.Nystrom(kernel, x, zp, sig2, 1e-4, dtype)
    P = ny.dense()
    R = np.random.default_rng(7).standard_normal((300, 3)).astype(dtype)
    ref = np.linalg.solve(P, R.astype(F64))
    err = float(np.abs(ny.apply(R).astype(F64) - ref).max() / np.abs(ref).max())
    eld = abs(ny.logdet - np.linalg.slogdet(P)[1]) / abs(np.linalg.slogdet(P)[1])
    print(f"Woodbury k{k} {np.dtype(dtype).name}: P^-1 R {err:.2e} relative, log det P {eld:.2e}")
    assert err <= (1e-8 if dtype == F64 else 1e-4) and eld <= 1e-10
    # the probes' covariance is P: with the exact probes (1 / T) sum_t z_t z_t' = P
    if dtype == F64 and k == 17:
        import cg_precond_ref as pr
        eps, xi = pr.exact_probes(300, k)
        Zt = ny.probes(eps, xi)
        assert np.abs(Zt @ Zt.T / (300 + k) - P).max() <= 1e-10 * np.abs(P).max()


def test_preconditioned_restatement_with_exact_probes_is_the_exact_gp():
    import cg_precond_ref as pr
    kernel, x, delta, s, sig2 = _problem(48, 1, o.KERNEL_MATERN52, F64)
    zp = np.ascontiguousarray(x[:, :8])
    eps, xi = pr.exact_probes(48, 8)
    r = nr.estimate_precond(kernel, x, zp, nr.DIAG, s, delta, eps, xi, 1e-12, 2000, grad=True)
    ref = nr.dense_lml(kernel, x, sig2, delta)
    assert abs(r["lml"] - ref) <= 1e-10 * abs(ref)
    g = nr.dense_noise_gradient(kernel, x, sig2, delta)
    assert np.abs(r["grad"]["noise"] - g).max() <= 1e-8 * np.abs(g).max()
    plain = nr.estimate(kernel, x, nr.DIAG, s, delta, cr.unit_probes(48), 1e-12, 2000, grad=True)
    assert abs(r["grad"]["variance"] - plain["grad"]["variance"]) <= 1e-8 * abs(plain["grad"]["variance"])


def test_python_argument_errors_need_no_context(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the GPU was touched")

    monkeypatch.setattr(_ffi, "default_context", boom)
    f = approxgp.GP(approxgp.SqExponentialKernel())
    x, y = np.linspace(0, 1, 9), np.zeros(9)
    cg = approxgp.ConjugateGradients()
    D = approxgp.Diagonal
    post = lambda cg_, fx_, y_: approxgp.CGPosteriorGP(cg_, fx_, y_)
    for call in (approxgp.approx_lml, approxgp.approx_lml_and_gradient, post):
        with pytest.raises(ValueError, match="one variance per point"):
            call(cg, f(x, D(np.full(8, 0.1))), y)
        with pytest.raises(ValueError, match="one variance per point"):
            call(cg, f(x, D(np.full((9, 1), 0.1))), y)
        for bad in (0.0, -0.1, float("nan")):
            v = np.full(9, 0.1)
            v[4] = bad
            with pytest.raises(ValueError, match="must be > 0"):
                call(cg, f(x, D(v)), y)
        with pytest.raises(_ffi.UnsupportedError, match="Diagonal"):   # a plain vector is still asked for by type
            call(cg, f(x, np.full(9, 0.1)), y)
    with pytest.raises(AssertionError, match="the GPU was touched"):   # a good Diagonal passes every check
        approxgp.approx_lml(cg, f(x, D(np.full(9, 0.1))), y)
    with pytest.raises(AssertionError, match="the GPU was touched"):
        approxgp.CGPosteriorGP(cg, f(x, D(np.full(9, 0.1))), y)
    with pytest.raises(_ffi.UnsupportedError, match="CGPosteriorGP"):   # the dispatch keeps refusing a Diagonal, as it always has
        approxgp.posterior(cg, f(x, D(np.full(9, 0.1))), y)
    with pytest.raises(ValueError, match="wrt_noise is True or False"):
        approxgp.approx_lml_and_gradient(cg, f(x, 0.1), y, wrt_noise=1)
    # the handle's own checks come before its library call
    dev = object.__new__(approxgp.DeviceConjugateGradients)
    dev.n, dev.d, dev.dtype, dev.precond_k, dev.ctx, dev.h, dev.data = 9, 1, _ffi.F64, 0, None, None, None
    with pytest.raises(ValueError, match="noise_grad_out needs wrt_noise=True"):
        dev.lml_grad(None, None, noise_grad_out=np.zeros(9))
    with pytest.raises(ValueError, match="wrt_noise is True or False"):
        dev.lml_grad(None, None, wrt_noise="yes")
    with pytest.raises(ValueError, match="one entry per point"):
        dev.set_noise(np.zeros(8))
    # predictions of y on a per-point-noise posterior need the test points' noise
    post = object.__new__(approxgp.iterative.CGPosteriorGP)
    post.noise, post.dev = None, dev
    with pytest.raises(ValueError, match="pass noise="):
        post.predict_y(np.zeros(3))
    with pytest.raises(ValueError, match="pass noise="):
        post.log_predictive_density(np.zeros(3), np.zeros(3))
    with pytest.raises(ValueError, match="one variance per test point"):
        post.predict_y(np.zeros(3), noise=np.full(4, 0.1))
    with pytest.raises(ValueError, match="noise > 0"):
        post.predict_y(np.zeros(3), noise=0.0)


def test_other_approximations_pass_through_untouched(monkeypatch):
    from approxgp import iterative, nearest_neighbors, vfe

    seen = []
    monkeypatch.setattr(vfe, "approx_lml", lambda *a, **k: seen.append(("lml", a, k)) or 1.0)
    monkeypatch.setattr(vfe, "posterior", lambda *a, **k: seen.append(("post", a, k)) or 2.0)
    monkeypatch.setattr(nearest_neighbors, "approx_lml_and_gradient", lambda *a, **k: seen.append(("grad", a, k)) or 3.0)
    other, y = object(), object()
    fx = approxgp.GP(approxgp.SqExponentialKernel())(np.zeros(3), approxgp.Diagonal(np.full(3, 0.1)))
    assert iterative.approx_lml(other, fx, y, wrt_noise=True) == 1.0
    assert iterative.posterior(other, fx, y, noise=3) == 2.0
    assert iterative.approx_lml_and_gradient(other, fx, y, wrt_noise=True) == 3.0
    assert seen == [("lml", (other, fx, y), dict(wrt_noise=True)), ("post", (other, fx, y), dict(noise=3)),
                    ("grad", (other, fx, y), dict(wrt_noise=True))]


def test_abi_and_header():
    import ctypes as C
    assert C.sizeof(_ffi.PointNoise) == 16 and C.sizeof(_ffi.PointNoiseGrad) == 16
    lib = approxgp.load_library()
    assert hasattr(lib, "svgp_cg_set_noise") and hasattr(lib, "svgp_cg_lml_grad_noise")
    assert lib.svgp_cg_set_noise(None, None, None) == _ffi.INVALID_ARG   # a NULL context, before anything else
