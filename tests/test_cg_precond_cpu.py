"""CPU checks (no GPU) of the Nystrom preconditioner of the conjugate gradients: the numpy restatement tests/cg_precond_ref.py against the
oracle's dense exact GP, the dense gradient and central differences, and the Python layer's new arguments."""
import numpy as np
import pytest

import approxgp
import cg_precond_ref as pr
import cg_ref as cr
import svgp_oracle as o
from approxgp import _ffi

FAMILIES = [o.KERNEL_SE, o.KERNEL_MATERN32, o.KERNEL_MATERN52]


def _problem(N, d, family, k, seed=0):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-3, 3, size=(d, N))
    kernel = o.Kernel(family, 1.3, np.full(d, 1 / 0.7))
    y = np.sin(x.sum(0)) + 0.1 * rng.standard_normal(N)
    zp = x[:, np.random.default_rng(5).choice(N, size=k, replace=False)]
    return kernel, x, y, zp


@pytest.mark.parametrize("family", FAMILIES)
def test_apply_and_logdet_equal_the_dense_preconditioner(family):
    kernel, x, y, zp = _problem(120, 2, family, 24)
    ny = pr.Nystrom(kernel, x, zp, 0.05)
    P = ny.dense()
    R = np.random.default_rng(1).standard_normal((120, 3))
    ref = np.linalg.solve(P, R)
    assert np.abs(ny.apply(R) - ref).max() <= 1e-9 * np.abs(ref).max()
    assert abs(ny.logdet - np.linalg.slogdet(P)[1]) <= 1e-9 * abs(ny.logdet)
    np.testing.assert_allclose(ny.cross(R), o.kernelmatrix(kernel, x, zp).T @ R, rtol=0, atol=1e-12 * 120)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("N,d,k", [(48, 1, 8), (150, 2, 32)])
def test_exact_probes_give_the_exact_lml(N, d, k, family):
    kernel, x, y, zp = _problem(N, d, family, k)
    eps, xi = pr.exact_probes(N, k)
    r = pr.estimate(kernel, x, zp, 0.1, y, eps, xi, 1e-12, 2000)
    ref = o.exact_gp_logpdf(kernel, x, 0.1, y)
    assert abs(r["lml"] - ref) <= 1e-8 * abs(ref), (r["lml"], ref)
    assert r["rel"].max() <= 1e-12


@pytest.mark.parametrize("family", FAMILIES)
def test_exact_probe_gradient_equals_the_dense_gradient_and_central_differences(family):
    N, d, k = 48, 2, 8
    kernel, x, y, zp = _problem(N, d, family, k)
    eps, xi = pr.exact_probes(N, k)
    g = pr.estimate(kernel, x, zp, 0.1, y, eps, xi, 1e-12, 2000, grad=True)["grad"]
    dn = cr.dense_estimate(kernel, x, 0.1, y, cr.unit_probes(N))["grad"]   # the exact gradient
    h = 1e-6
    il = kernel.inv_lengthscale

    def f(var, il_, diag, mc=0.0):
        return o.exact_gp_logpdf(o.Kernel(family, var, il_), x, diag, y - mc)

    fd = {"variance": (f(1.3 + h, il, 0.1) - f(1.3 - h, il, 0.1)) / (2 * h), "diag": (f(1.3, il, 0.1 + h) - f(1.3, il, 0.1 - h)) / (2 * h),
          "mean_const": (f(1.3, il, 0.1, h) - f(1.3, il, 0.1, -h)) / (2 * h)}
    for name in ("variance", "diag", "mean_const"):
        assert abs(g[name] - dn[name]) <= 1e-7 * max(abs(dn[name]), 1.0), (name, g[name], dn[name])
        assert abs(g[name] - fd[name]) <= 1e-6 * max(abs(fd[name]), 1.0), (name, g[name], fd[name])
    fil = np.array([(f(1.3, il + h * np.eye(d)[c], 0.1) - f(1.3, il - h * np.eye(d)[c], 0.1)) / (2 * h) for c in range(d)])
    np.testing.assert_allclose(g["inv_lengthscale"], dn["inv_lengthscale"], atol=1e-7 * np.abs(dn["inv_lengthscale"]).max())
    np.testing.assert_allclose(g["inv_lengthscale"], fil, atol=1e-6 * np.abs(fil).max())


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("family", FAMILIES)
def test_preconditioned_iteration_converges_to_the_dense_solve_in_fewer_steps(family, dtype):
    N, d, k, diag = 300, 2, 64, 0.01
    kernel, x, y, zp = _problem(N, d, family, k)
    x = x.astype(dtype).astype(np.float64)
    zp = zp.astype(dtype).astype(np.float64)
    tol = 1e-10 if dtype == np.float64 else 1e-5
    Kh = cr.khat(kernel, x, float(dtype(diag)))
    B = np.column_stack([y, np.random.default_rng(3).standard_normal((N, 2))])
    ny = pr.Nystrom(kernel, x, zp, diag, 1e-4, dtype)
    mv = (lambda P: Kh @ P) if dtype == np.float64 else (lambda P: cr.kmv_f32(kernel, x, P, diag))
    X, it, rel, _, _, _ = pr.pmbcg(mv, ny.apply, B, tol, 2000, dtype)
    X0, it0, rel0, _, _, _ = cr.mbcg(mv, B, tol, 2000, dtype)
    ref = np.linalg.solve(Kh, B.astype(dtype).astype(np.float64))
    err = np.linalg.norm(X - ref, axis=0) / np.linalg.norm(ref, axis=0)
    assert rel.max() <= tol and err.max() <= np.linalg.cond(Kh) * tol
    assert 2 * it.max() <= it0.max(), (it, it0)


def test_python_argument_errors_need_no_context(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the GPU was touched")

    monkeypatch.setattr(_ffi, "default_context", boom)
    for bad in (dict(precond_size=-1), dict(precond_size=1.5), dict(precond_size=4096), dict(precond_jitter=-1e-3),
                dict(precond_jitter=float("nan")), dict(precond_points=np.zeros((2, 0))), dict(precond_points=np.zeros((2, 3, 1))),
                dict(precond_points=np.zeros((2, 3)), precond_size=4), dict(precond_points=np.zeros((1, 4096)))):
        with pytest.raises(ValueError):
            approxgp.ConjugateGradients(**bad)
    f = approxgp.GP(approxgp.SqExponentialKernel())
    x, y = np.linspace(0, 1, 9), np.zeros(9)
    with pytest.raises(ValueError, match="dimension"):
        approxgp.approx_lml(approxgp.ConjugateGradients(precond_points=np.zeros((2, 3))), f(x, 0.1), y)
    with pytest.raises(ValueError, match="noise"):
        approxgp.approx_lml(approxgp.ConjugateGradients(precond_size=4), f(x, 0.0), y)
    with pytest.raises(ValueError, match="seed"):
        approxgp.approx_lml(approxgp.ConjugateGradients(precond_size=4, seed=None), f(x, 0.1), y)


def test_probes_and_points_of_a_seed():
    plain = approxgp.ConjugateGradients(n_probes=5, seed=3)
    pc = approxgp.ConjugateGradients(n_probes=5, seed=3, precond_size=4, precond_jitter=1e-3)
    np.testing.assert_array_equal(plain.probes_for(11), approxgp.draw_probes(11, 5, 3))   # what the seed gave before the new arguments
    np.testing.assert_array_equal(pc.probes_for(11), plain.probes_for(11))
    xi = pc.probes_k_for(4, 5)
    np.testing.assert_array_equal(xi, approxgp.draw_probes(4, 5, np.random.default_rng([3, 1])))
    assert xi.shape == (4, 5) and set(np.unique(xi)) <= {-1.0, 1.0}
    x = np.random.default_rng(0).standard_normal((2, 11))
    pts = pc.precond_points_for(x)
    idx = np.random.default_rng([3, 2]).choice(11, size=4, replace=False)
    np.testing.assert_array_equal(pts, x[:, idx])
    assert plain.precond_points_for(x) is None
    assert approxgp.ConjugateGradients(precond_size=50).precond_points_for(x).shape == (2, 11)   # clipped to N
    own = np.ones((2, 3))
    assert approxgp.ConjugateGradients(precond_points=own).precond_points_for(x) is not None
    assert approxgp.ConjugateGradients(precond_points=np.arange(3.0)).precond_points.shape == (1, 3)   # a plain vector, d = 1


def test_other_approximations_pass_through_untouched(monkeypatch):
    from approxgp import iterative, nearest_neighbors, vfe

    seen = []
    monkeypatch.setattr(vfe, "approx_lml", lambda *a, **k: seen.append(("lml", a, k)) or 1.0)
    monkeypatch.setattr(vfe, "posterior", lambda *a, **k: seen.append(("post", a, k)) or 2.0)
    monkeypatch.setattr(nearest_neighbors, "approx_lml_and_gradient", lambda *a, **k: seen.append(("grad", a, k)) or 3.0)
    other, fx, y = object(), object(), object()
    assert iterative.approx_lml(other, fx, y, precond_size=5) == 1.0
    assert iterative.posterior(other, fx, y) == 2.0
    assert iterative.approx_lml_and_gradient(other, fx, y, precond_points=7) == 3.0
    assert seen == [("lml", (other, fx, y), dict(precond_size=5)), ("post", (other, fx, y), {}), ("grad", (other, fx, y), dict(precond_points=7))]
