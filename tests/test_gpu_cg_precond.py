"""GPU checks of the Nystrom preconditioner of the conjugate gradients (svgp_cg_set_preconditioner, svgp_cg_precond_cross / _apply,
svgp_cg_fit_precond / _lml_grad_precond; csrc/cg.hip, cg_api.hip).  A wrong preconditioner still lets CG reach the right solution, so the
cross product, P^-1 and log det P are pinned directly against dense float64; the solver, the log det estimate, the gradient and the
predictions are then checked as tests/test_gpu_cg.py checks the unpreconditioned ones, with the same data, variance and lengthscale.

Bounds.  precond_cross: test_matvec_against_dense's (fp64 1e-12 max_i sum_j |K_ij V_js|; fp32 4 x the float32 chain's own error).
precond_apply: fp64 1e-8 relative to the largest entry; fp32 4 x the error of the float32 restatement (cg_precond_ref) on the same
inputs; log det P 1e-8 relative in both dtypes, because the k-sized stage is fp64 for both.  lml / gradient / predictions: the project's
parity contracts, 1e-8 relative in fp64 and 1e-4 in fp32 (the float32 restatement's own lml error with the exact probes is <= 2.1e-6
on both shapes, inside the contract).  test_report_observed_errors prints every measured figure (profiles/cg/accuracy_precond.md
records a run on an MI355X)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import cg_precond_ref as pr
import cg_ref as cr
import svgp_oracle as o
from approxgp import GP, ConjugateGradients, _ffi, approx_lml, approx_lml_and_gradient, draw_probes, posterior
from test_gpu_cg import FAMILIES, LS, M32, SE, SOLVE_CASES, VAR, _dev, _grad_err, _kernel, _okernel, _xy

pytestmark = pytest.mark.gpu

F64, F32 = np.float64, np.float32
OBSERVED = {}


@pytest.fixture(scope="module")
def ctx():
    c = _ffi.Context(0)
    yield c
    c.close()


def _points(x, k, seed=5):
    """k of the data points, default_rng(seed).choice without replacement"""
    return np.ascontiguousarray(x[:, np.random.default_rng(seed).choice(x.shape[1], size=k, replace=False)])


def _name(dtype):
    return np.dtype(dtype).name


# ---- 1. the cross product K(z_p, X) V ------------------------------------------------------------------------------------------------
CROSS = [(1, 1, 1, 1), (31, 15, 16, 8), (33, 17, 17, 9), (1000, 64, 65, 33), (2049, 65, 1, 1), (2049, 257, 17, 8), (1000, 257, 16, 9),
         (33, 1, 65, 33), (31, 64, 17, 1), (2049, 15, 65, 9), (1, 17, 16, 33), (1000, 65, 1, 8)]


@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("i", range(len(CROSS)))
def test_precond_cross_against_dense(ctx, i, dtype):
    N, k, S, d = CROSS[i]
    family = FAMILIES[i % 3]
    x, y = _xy(N, d)
    x = x.astype(dtype)
    rng = np.random.default_rng(N + k + S + d)
    zp = rng.uniform(-3, 3, size=(d, k)).astype(dtype)
    V = np.asfortranarray(rng.standard_normal((N, S)).astype(dtype))
    dev = _dev(ctx, x, None, dtype)
    try:
        desc, keep = dev.desc(_kernel(family, d), 0.1, tol=1e-8, maxiter=10)
        dev.set_preconditioner(zp[0] if d == 1 else zp)
        out = dev.precond_cross(desc, V)
        again = dev.precond_cross(desc, V)
        c = S // 2
        alone = dev.precond_cross(desc, V[:, c])
        Vt = torch.from_numpy(np.ascontiguousarray(V.T)).cuda()
        ot = torch.empty((S, k), dtype=Vt.dtype, device="cuda")
        torch.cuda.synchronize()
        dev.precond_cross(desc, Vt, out=ot)
        on_dev = ot.cpu().numpy().T
        mv = dev.matvec(desc, V)   # the handle's own product is untouched by a preconditioner
    finally:
        dev.free()
    plain = _dev(ctx, x, None, dtype)
    try:
        mv0 = plain.matvec(desc, V)
    finally:
        plain.free()
    assert np.array_equal(mv, mv0)
    assert out.shape == (k, S) and out.dtype == dtype and np.array_equal(out, again), "two calls differ"
    assert np.array_equal(out, on_dev), "host and device-memory outputs differ"
    assert np.array_equal(out[:, c], alone[:, 0]), "a column depends on its neighbours"
    ok = _okernel(family, d, dtype)
    Kc = o.kernelmatrix(ok, x.astype(F64), zp.astype(F64)).T   # k x N
    ref = Kc @ V.astype(F64)
    err = float(np.abs(out.astype(F64) - ref).max())
    scale = float((np.abs(Kc) @ np.abs(V.astype(F64))).max())
    name = f"cross N{N} k{k} S{S} d{d} k{family} {_name(dtype)}"
    if dtype == F64:
        OBSERVED[name] = f"error {err:.2e}, bound {1e-12 * scale:.2e}"
        print(name, OBSERVED[name])
        assert err <= 1e-12 * scale, (err, scale)
    else:
        chain = cr.kernel_chain(ok, x, F32, xt=zp)[0] @ V
        e_ref = float(np.abs(chain.astype(F64) - ref).max())
        OBSERVED[name] = f"error {err:.2e}, float32 chain {e_ref:.2e}, ratio {err / max(e_ref, 1e-300):.2f}"
        print(name, OBSERVED[name])
        assert err <= 4.0 * e_ref, (err, e_ref)


# ---- 2. P^-1 R and log det P ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _apply_reference(family, k, s2, dtype):
    """dense float64 P^-1 R and log det P from the dtype-rounded inputs, and the float32 restatement's own error (shared by the cases)"""
    N, d = 300, 2
    x, y = _xy(N, d)
    x = x.astype(dtype).astype(F64)
    zp = _points(x, k)
    R = np.random.default_rng(7).standard_normal((N, 3)).astype(dtype)
    ok = _okernel(family, d, dtype)
    ny = pr.Nystrom(ok, x, zp, float(dtype(s2)))
    P = ny.dense()
    ref = np.linalg.solve(P, R.astype(F64))
    logdet = float(np.linalg.slogdet(P)[1])
    e32 = float(np.abs(pr.Nystrom(ok, x, zp, s2, dtype=F32).apply(R).astype(F64) - ref).max()) if dtype == F32 else 0.0
    for a in (x, zp, R, ref):
        a.setflags(write=False)
    return x, zp, R, ref, logdet, e32


@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("s2", [0.1, 0.01])
@pytest.mark.parametrize("k", [17, 64])
def test_precond_apply_against_dense(ctx, k, s2, family, dtype):
    x, zp, R, ref, logdet, e32 = _apply_reference(family, k, s2, dtype)
    dev = _dev(ctx, x.astype(dtype), None, dtype)
    try:
        desc, keep = dev.desc(_kernel(family, 2), s2, tol=1e-8, maxiter=10)
        dev.set_preconditioner(zp, 1e-4)
        out, ld = dev.precond_apply(desc, R)
        again, ld2 = dev.precond_apply(desc, R)
        Rt = torch.from_numpy(np.ascontiguousarray(R.T)).cuda()
        ot = torch.empty_like(Rt)
        torch.cuda.synchronize()
        _, ld3 = dev.precond_apply(desc, Rt, out=ot)
        on_dev = ot.cpu().numpy().T
    finally:
        dev.free()
    assert np.array_equal(out, again) and ld == ld2 == ld3 and np.array_equal(out, on_dev)
    err = float(np.abs(out.astype(F64) - ref).max())
    eld = abs(ld - logdet) / abs(logdet)
    name = f"apply k{k} s2 {s2} k{family} {_name(dtype)}"
    if dtype == F64:
        OBSERVED[name] = f"error {err / np.abs(ref).max():.2e} relative, log det P {eld:.2e}"
        print(name, OBSERVED[name])
        assert err <= 1e-8 * np.abs(ref).max(), (err, np.abs(ref).max())
    else:
        OBSERVED[name] = f"error {err:.2e}, float32 restatement {e32:.2e}, ratio {err / max(e32, 1e-300):.2f}, log det P {eld:.2e}"
        print(name, OBSERVED[name])
        assert err <= 4.0 * e32, (err, e32)
    assert eld <= 1e-8, (ld, logdet)


@pytest.mark.parametrize("k", [129, 257])
def test_precond_apply_beyond_one_tile(ctx, k):
    """k > 128: two and three 128-tiles in the k-sized factorisations and products (fp64, Matern-3/2, the suite's 1e-8 contract; the
    float64 restatement is within 4e-11 of the dense solve on these inputs)"""
    x, zp, R, ref, logdet, _ = _apply_reference(M32, k, 0.1, F64)
    dev = _dev(ctx, x, None, F64)
    try:
        desc, keep = dev.desc(_kernel(M32, 2), 0.1, tol=1e-8, maxiter=10)
        dev.set_preconditioner(zp, 1e-4)
        out, ld = dev.precond_apply(desc, R)
    finally:
        dev.free()
    err = float(np.abs(out - ref).max() / np.abs(ref).max())
    OBSERVED[f"apply k{k} s2 0.1 k{M32} float64"] = f"error {err:.2e} relative, log det P {abs(ld - logdet) / abs(logdet):.2e}"
    assert err <= 1e-8 and abs(ld - logdet) <= 1e-8 * abs(logdet), (err, ld, logdet)


@pytest.mark.parametrize("family", [SE, M32])
def test_precond_apply_at_eight_tiles(ctx, family):
    """k = 1024 (eight 128-tiles in every factorisation and product of the k-sized stage) on N = 2049, fp64, against dense.  W is built
    from explicit inverses, Lu^-T B^-1 Lu^-1, so its error grows like cond(Kuu) cond(B) eps: that product, computed here, is the bound
    (about 2e-7 on these inputs; the float64 restatement itself is within 5.5e-9 (SE) and 5.2e-10 (Matern-3/2) of the dense solve)."""
    N, d, k, s2 = 2049, 2, 1024, 0.1
    x, y = _xy(N, d)
    zp = _points(x, k)
    R = np.random.default_rng(7).standard_normal((N, 3))
    ny = pr.Nystrom(_okernel(family, d), x, zp, s2)
    P = ny.dense()
    ref = np.linalg.solve(P, R)
    logdet = float(np.linalg.slogdet(P)[1])
    bound = np.linalg.cond(ny.Lu) ** 2 * np.linalg.cond(ny.B) * np.finfo(F64).eps
    dev = _dev(ctx, x, None, F64)
    try:
        desc, keep = dev.desc(_kernel(family, d), s2, tol=1e-8, maxiter=10)
        dev.set_preconditioner(zp, 1e-4)
        out, ld = dev.precond_apply(desc, R)
    finally:
        dev.free()
    err = float(np.abs(out - ref).max() / np.abs(ref).max())
    e_ref = float(np.abs(ny.apply(R) - ref).max() / np.abs(ref).max())
    OBSERVED[f"apply N2049 k1024 s2 0.1 k{family} float64"] = (
        f"error {err:.2e} relative, float64 restatement {e_ref:.2e}, bound {bound:.2e}, log det P {abs(ld - logdet) / abs(logdet):.2e}")
    print(OBSERVED[f"apply N2049 k1024 s2 0.1 k{family} float64"])
    assert err <= bound and abs(ld - logdet) <= 1e-8 * abs(logdet), (err, bound, ld, logdet)


# ---- 3. solve ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("N,d,diag", SOLVE_CASES)
def test_preconditioned_solve_against_dense(ctx, N, d, diag, family, dtype):
    x, y = _xy(N, d)
    x = x.astype(dtype)
    B = np.asfortranarray(np.column_stack([y, np.random.default_rng(3).standard_normal((N, 2))]).astype(dtype))
    tol = 1e-10 if dtype == F64 else 1e-5
    dev = _dev(ctx, x, None, dtype)
    try:
        desc, keep = dev.desc(_kernel(family, d), diag, tol=tol, maxiter=2000)
        dev.set_preconditioner(_points(x, 32)[0] if d == 1 else _points(x, 32))
        X, iters, rel, info = dev.solve(desc, B)
    finally:
        dev.free()
    Kh = cr.khat(_okernel(family, d, dtype), x.astype(F64), float(dtype(diag)))
    ref = np.linalg.solve(Kh, B.astype(F64))
    cond = np.linalg.cond(Kh)
    err = np.linalg.norm(X.astype(F64) - ref, axis=0) / np.linalg.norm(ref, axis=0)
    name = f"solve N{N} d{d} diag{diag} k{family} {_name(dtype)}"
    OBSERVED[name] = f"iterations {iters.max()}, residual {rel.max():.2e}, error {err.max():.2e}, cond tol {cond * tol:.2e}"
    print(name, OBSERVED[name])
    assert info.converged == 1 and info.n_unconverged == 0 and info.iterations == iters.max()
    assert rel.max() <= tol and info.max_rel_residual == rel.max()
    assert err.max() <= cond * tol, (err, cond)


@pytest.mark.parametrize("dtype", [F64, F32])
def test_preconditioned_columns_do_not_depend_on_their_neighbours(ctx, dtype):
    N, d = 300, 2
    x, y = _xy(N, d)
    B = np.asfortranarray(np.random.default_rng(9).standard_normal((N, 70)).astype(dtype))
    B[:, 5] = 0
    dev = _dev(ctx, x.astype(dtype), None, dtype)
    try:
        desc, keep = dev.desc(_kernel(M32, d), 0.1, tol=1e-10 if dtype == F64 else 1e-5, maxiter=2000)
        dev.set_preconditioner(_points(x.astype(dtype), 32))
        X, iters, rel, info = dev.solve(desc, B)
        X2, iters2, rel2, _ = dev.solve(desc, B)
        X0, it0, rel0, _ = dev.solve(desc, B[:, :1])
        X66, it66, rel66, _ = dev.solve(desc, B[:, 66:67])
    finally:
        dev.free()
    assert np.array_equal(X, X2) and np.array_equal(iters, iters2) and np.array_equal(rel, rel2)
    assert np.array_equal(X[:, 0], X0[:, 0]) and iters[0] == it0[0] and rel[0] == rel0[0]
    assert np.array_equal(X[:, 66], X66[:, 0]) and iters[66] == it66[0] and rel[66] == rel66[0]
    assert iters[5] == 0 and not X[:, 5].any() and rel[5] == 0 and info.converged == 1


# ---- 4. fewer iterations -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("family", FAMILIES)
def test_the_preconditioner_halves_the_iterations(ctx, family, dtype):
    N, d, diag = 300, 2, 0.01
    x, y = _xy(N, d)
    x = x.astype(dtype)
    B = np.asfortranarray(np.column_stack([y, np.random.default_rng(3).standard_normal((N, 2))]).astype(dtype))
    dev = _dev(ctx, x, None, dtype)
    try:
        desc, keep = dev.desc(_kernel(family, d), diag, tol=1e-10 if dtype == F64 else 1e-5, maxiter=2000)
        _, it0, _, info0 = dev.solve(desc, B)
        dev.set_preconditioner(_points(x, 64))
        _, it1, _, info1 = dev.solve(desc, B)
    finally:
        dev.free()
    OBSERVED[f"iterations N300 diag0.01 k64 k{family} {_name(dtype)}"] = f"{it0.max()} unpreconditioned, {it1.max()} preconditioned"
    print(family, _name(dtype), it0, it1)
    assert info0.converged == 1 and info1.converged == 1
    assert 2 * it1.max() <= it0.max(), (it1, it0)


# ---- 5. exact probes -----------------------------------------------------------------------------------------------------------------
EXACT = [(48, 1, 8), (150, 2, 32)]


@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("N,d,k", EXACT)
def test_lml_with_exact_probes_is_the_exact_gp(ctx, N, d, k, family, dtype):
    x, y = _xy(N, d)
    x, y = x.astype(dtype), y.astype(dtype)
    eps, xi = pr.exact_probes(N, k)
    dev = _dev(ctx, x, y, dtype)
    try:
        desc, keep = dev.desc(_kernel(family, d), 0.1, tol=1e-12 if dtype == F64 else 1e-5, maxiter=2000)
        dev.set_preconditioner(_points(x, k), 1e-4)
        lml, info = dev.fit(desc, eps, probes_k=xi)
    finally:
        dev.free()
    ref = o.exact_gp_logpdf(_okernel(family, d, dtype), x.astype(F64), float(dtype(0.1)), y.astype(F64))
    err = abs(lml - ref) / abs(ref)
    OBSERVED[f"lml exact probes N{N} d{d} k{k} k{family} {_name(dtype)}"] = f"relative error {err:.2e}, iterations {info.iterations}"
    if dtype == F32:   # the float32 restatement's own error on the same inputs, for the record (the 1e-4 contract holds if it is inside it)
        r32 = pr.estimate(_okernel(family, d, dtype), x.astype(F64), _points(x, k).astype(F64), 0.1, y.astype(F64), eps, xi, 1e-5, 2000, dtype=F32)
        OBSERVED[f"lml exact probes N{N} d{d} k{k} k{family} {_name(dtype)}"] += f", float32 restatement {abs(r32['lml'] - ref) / abs(ref):.2e}"
    print(N, d, k, family, _name(dtype), err, info.iterations)
    assert lml == info.lml and info.converged == 1
    assert err <= (1e-8 if dtype == F64 else 1e-4), (lml, ref)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("N,d,k", EXACT)
def test_exact_probe_gradient_against_dense_and_central_differences(ctx, N, d, k, family):
    x, y = _xy(N, d)
    eps, xi = pr.exact_probes(N, k)
    il = np.full(d, 1.0 / LS)
    dev = _dev(ctx, x, y, F64)

    def device_lml(var, il_, dg, mc=0.0):
        ds = _ffi.CGDesc(dtype=dev.dtype, kernel=family, d=d, maxiter=2000, variance=var, inv_lengthscale=il_.ctypes.data_as(C.POINTER(C.c_double)),
                         diag=dg, mean_const=mc, tol=1e-12, reserved=0)
        return dev.fit(ds, eps, probes_k=xi)[0]

    try:
        desc, keep = dev.desc(_kernel(family, d), 0.1, tol=1e-12, maxiter=2000)
        dev.set_preconditioner(_points(x, k), 1e-4)
        lml, g, info = dev.lml_grad(desc, eps, probes_k=xi)
        # central differences of the device's own lml.  Two fits at nearby parameters differ by iteration noise of up to about
        # cond tol |lml| ~ 1e-9, which a quotient with h ~ 1e-5 would turn into 1e-4: so the five-point stencil (truncation h^4 f^(5) / 30)
        # with h = 2e-3, whose noise is 18 / (12 h) = 750 times the lml's; lml is exactly quadratic in mean_const, where h = 0.1 is exact
        def diff(f, h):
            return (-f(2 * h) + 8 * f(h) - 8 * f(-h) + f(-2 * h)) / (12 * h)

        h = 2e-3
        e = np.eye(d)
        fd = {"variance": diff(lambda t: device_lml(VAR + t, il, 0.1), h), "diag": diff(lambda t: device_lml(VAR, il, 0.1 + t), h),
              "mean_const": diff(lambda t: device_lml(VAR, il, 0.1, t), 0.1),
              "inv_lengthscale": np.array([diff(lambda t, c=c: device_lml(VAR, il + t * e[c], 0.1), h) for c in range(d)])}
    finally:
        dev.free()
    dn = cr.dense_estimate(_okernel(family, d), x, 0.1, y, cr.unit_probes(N))["grad"]   # unit probes: the exact gradient
    for what, ref in (("dense", dn), ("central differences", fd)):
        ge = _grad_err(g, ref)
        OBSERVED[f"exact-probe gradient vs {what} N{N} d{d} k{k} k{family}"] = ", ".join(f"{n} {v:.2e}" for n, v in ge.items())
        print(what, N, family, ge)
        for n, v in ge.items():
            assert v <= 1e-6 or (n == "mean_const" and abs(g[n] - ref[n]) <= 1e-7), (what, n, v, g[n], ref[n])


# ---- 6. Rademacher probes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("family", FAMILIES)
def test_lml_and_gradient_with_rademacher_probes(ctx, family, dtype):
    N, d, diag, k = 300, 2, 0.1, 32
    x, y = _xy(N, d)
    x, y = x.astype(dtype), y.astype(dtype)
    eps, xi = draw_probes(N, 16, 4), draw_probes(k, 16, np.random.default_rng([4, 1]))
    zp = _points(x, k)
    tol = 1e-12 if dtype == F64 else 1e-5
    dev = _dev(ctx, x, y, dtype)
    try:
        desc, keep = dev.desc(_kernel(family, d), diag, mean_const=0.25, tol=tol, maxiter=2000)
        dev.set_preconditioner(zp, 1e-4)
        lml, g, info = dev.lml_grad(desc, eps, probes_k=xi)
        lml2, info2 = dev.fit(desc, eps, probes_k=xi)
    finally:
        dev.free()
    ok = _okernel(family, d, dtype)
    r = pr.estimate(ok, x.astype(F64), zp.astype(F64), float(dtype(diag)), y.astype(F64) - 0.25, eps, xi, tol, 2000, grad=True)
    c = 1e-8 if dtype == F64 else 1e-4
    ge = _grad_err(g, r["grad"])
    OBSERVED[f"lml rademacher k{family} {_name(dtype)}"] = (
        f"lml {abs(lml - r['lml']) / abs(r['lml']):.2e}, gradient " + ", ".join(f"{n} {v:.2e}" for n, v in ge.items()))
    print(family, _name(dtype), OBSERVED[f"lml rademacher k{family} {_name(dtype)}"])
    assert lml == lml2 and info.converged == 1 and info.quad == info2.quad   # bitwise
    assert abs(lml - r["lml"]) <= c * abs(r["lml"]) and abs(info.quad - r["quad"]) <= c * abs(r["quad"])
    assert abs(info.logdet - r["logdet"]) <= c * max(abs(r["logdet"]), abs(r["lml"]))
    for n, v in ge.items():
        assert v <= c, (n, v, g, r["grad"])


# ---- 7. predictions ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F64, F32])
def test_predict_against_the_exact_posterior(ctx, dtype):
    N, d, diag, ns = 300, 2, 0.1, 65
    family = FAMILIES[ns % 3]
    x, y = _xy(N, d)
    x, y = x.astype(dtype), y.astype(dtype)
    xs = np.random.default_rng(ns).uniform(-3, 3, size=(d, ns)).astype(dtype)
    tol = 1e-10 if dtype == F64 else 1e-5
    dev = _dev(ctx, x, y, dtype)
    try:
        desc, keep = dev.desc(_kernel(family, d), diag, tol=tol, maxiter=2000)
        dev.set_preconditioner(_points(x, 32))
        dev.fit(desc, None)
        m, v, info = dev.predict(xs)
    finally:
        dev.free()
    ok = _okernel(family, d, dtype)
    mr, cov = o.exact_gp_posterior(ok, x.astype(F64), float(dtype(diag)), y.astype(F64), xs.astype(F64))
    cond = np.linalg.cond(cr.khat(ok, x.astype(F64), float(dtype(diag))))
    em, ev = np.abs(m - mr).max(), np.abs(v - np.diag(cov)).max()
    OBSERVED[f"predict n{ns} k{family} {_name(dtype)}"] = f"mean {em:.2e}, var {ev:.2e}, cond tol {cond * tol:.2e}, iterations {info.iterations}"
    assert info.converged == 1
    assert em <= cond * tol * np.abs(mr).max() and ev <= cond * tol * ok.variance, (em, ev, cond * tol)


def test_the_python_layer_picks_the_preconditioner_up(ctx):
    N, d = 300, 2
    x, y = _xy(N, d)
    f = GP(_kernel(SE, d))
    plain = ConjugateGradients(tol=1e-10, maxiter=2000, n_probes=8, seed=1)
    cg = ConjugateGradients(tol=1e-10, maxiter=2000, n_probes=8, seed=1, precond_size=32)
    own = ConjugateGradients(tol=1e-10, maxiter=2000, n_probes=8, seed=1, precond_points=_points(x, 32, seed=11))
    a = approx_lml(cg, f(x, 0.1), y, ctx=ctx)
    b, g = approx_lml_and_gradient(cg, f(x, 0.1), y, ctx=ctx)
    c = approx_lml(own, f(x, 0.1), y, ctx=ctx)
    p0 = approx_lml(plain, f(x, 0.1), y, ctx=ctx)
    assert a == b and set(g) == {"variance", "inv_lengthscale", "diag", "mean_const"}
    assert a != p0 and a != c   # another estimator, other points
    # what the dispatcher must have done: the data subset of default_rng([seed, 2]), xi from default_rng([seed, 1]), the seed's own probes
    dev = _dev(ctx, x, y, F64)
    try:
        desc, keep = dev.desc(_kernel(SE, d), 0.1, tol=1e-10, maxiter=2000)
        dev.set_preconditioner(x[:, np.random.default_rng([1, 2]).choice(N, size=32, replace=False)], 1e-4)
        by_hand, _ = dev.fit(desc, draw_probes(N, 8, 1), probes_k=draw_probes(32, 8, np.random.default_rng([1, 1])))
        dev.set_preconditioner(_points(x, 32, seed=11), 1e-4)
        by_hand_own, _ = dev.fit(desc, draw_probes(N, 8, 1), probes_k=draw_probes(32, 8, np.random.default_rng([1, 1])))
    finally:
        dev.free()
    assert a == by_hand and c == by_hand_own   # bitwise
    post = posterior(cg, f(x, 0.1), y, ctx=ctx)
    try:
        xs = np.random.default_rng(2).uniform(-3, 3, size=(d, 17))
        m, v = post.mean_and_var(xs)
        assert post.lml == a
    finally:
        post.dev.free()
    mr, cov = o.exact_gp_posterior(_okernel(SE, d), x, 0.1, y, xs)
    np.testing.assert_allclose(m, mr, atol=1e-6 * np.abs(mr).max())
    np.testing.assert_allclose(v, np.diag(cov), atol=1e-6 * VAR)


# ---- 8. state and statuses -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F64, F32])
def test_set_then_clear_is_bitwise_a_handle_without_preconditioner(ctx, dtype):
    N, d = 300, 2
    x, y = _xy(N, d)
    x, y = x.astype(dtype), y.astype(dtype)
    B = np.asfortranarray(np.random.default_rng(3).standard_normal((N, 3)).astype(dtype))
    z = draw_probes(N, 4, 0)
    tol = 1e-10 if dtype == F64 else 1e-5
    never, dev = _dev(ctx, x, y, dtype), _dev(ctx, x, y, dtype)
    try:
        desc, keep = dev.desc(_kernel(M32, d), 0.1, tol=tol, maxiter=2000)
        X0, it0, rel0, _ = never.solve(desc, B)
        lml0, info0 = never.fit(desc, z)
        dev.set_preconditioner(_points(x, 32))
        Xp, itp, _, _ = dev.solve(desc, B)
        a1, ld1 = dev.precond_apply(desc, B)
        dev.set_preconditioner(_points(x, 48, seed=6))   # replacing the points takes effect
        a2, ld2 = dev.precond_apply(desc, B)
        dev.set_preconditioner(None)
        X1, it1, rel1, _ = dev.solve(desc, B)
        lml1, info1 = dev.fit(desc, z)
        with pytest.raises(ValueError, match="preconditioner"):
            dev.precond_apply(desc, B)
    finally:
        never.free()
        dev.free()
    assert itp.max() < it0.max() and not np.array_equal(Xp, X0)
    assert np.array_equal(X0, X1) and np.array_equal(it0, it1) and np.array_equal(rel0, rel1)
    assert lml0 == lml1 and info0.quad == info1.quad and info0.logdet == info1.logdet
    ok = _okernel(M32, d, dtype)
    ny = pr.Nystrom(ok, x.astype(F64), _points(x, 48, seed=6).astype(F64), float(dtype(0.1)))
    assert ld1 != ld2 and abs(ld2 - ny.logdet) <= 1e-8 * abs(ny.logdet) and not np.array_equal(a1, a2)
    ref = np.linalg.solve(ny.dense(), B.astype(F64))
    e32 = np.abs(pr.Nystrom(ok, x.astype(F64), _points(x, 48, seed=6).astype(F64), 0.1, dtype=F32).apply(B).astype(F64) - ref).max()
    assert np.abs(a2 - ref).max() <= (1e-8 * np.abs(ref).max() if dtype == F64 else 4.0 * e32)   # test_precond_apply_against_dense's bounds


def test_statuses_leave_the_context_healthy(ctx):
    N, d = 300, 2
    x, y = _xy(N, d)
    lib, h = ctx.lib, ctx.h
    dev = _dev(ctx, x, y, F64)
    k = _kernel(M32, d)
    desc, keep = dev.desc(k, 0.01, tol=1e-10, maxiter=2000)
    zero, keep0 = dev.desc(k, 0.0, tol=1e-10, maxiter=2000)
    B = np.asfortranarray(y[:, None].copy())
    X = np.zeros_like(B)
    zp = np.asfortranarray(_points(x, 16))
    out, info, ld = C.c_double(), _ffi.CGInfo(), C.c_double()
    dp = C.POINTER(C.c_double)
    z, zk = draw_probes(N, 2, 0), draw_probes(16, 2, 1)
    INV = _ffi.INVALID_ARG
    setp = lambda layout, kk, pts, jit: lib.svgp_cg_set_preconditioner(h, dev.h, layout, kk, _ffi._ptr(pts) if pts is not None else None, jit)
    try:
        lml_plain, _ = dev.fit(desc, z)
        # the new calls without a preconditioner
        assert lib.svgp_cg_precond_cross(h, dev.h, C.byref(desc), 1, _ffi._ptr(B), N, _ffi._ptr(X), N, 0) == INV
        assert lib.svgp_cg_precond_apply(h, dev.h, C.byref(desc), 1, _ffi._ptr(B), N, _ffi._ptr(X), N, 0, C.byref(ld)) == INV
        assert lib.svgp_cg_fit_precond(h, dev.h, C.byref(desc), None, 2, z.ctypes.data_as(dp), zk.ctypes.data_as(dp), C.byref(out), C.byref(info)) == INV
        assert lib.svgp_cg_lml_grad_precond(h, dev.h, C.byref(desc), None, 0, None, None, C.byref(out), C.byref(info), C.byref(ld),
                                            np.zeros(d).ctypes.data_as(dp), None, None) == INV
        # set_preconditioner's arguments
        assert setp(_ffi.COLVECS, -1, zp, 1e-4) == INV and setp(_ffi.COLVECS, 2049, zp, 1e-4) == INV and setp(_ffi.COLVECS, 16, None, 1e-4) == INV
        assert setp(7, 16, zp, 1e-4) == INV and setp(_ffi.VEC, 16, zp, 1e-4) == INV
        assert setp(_ffi.COLVECS, 16, zp, -1e-4) == INV and setp(_ffi.COLVECS, 16, zp, float("nan")) == INV
        assert setp(_ffi.COLVECS, 16, zp, 1e-4) == _ffi.OK
        dev.set_preconditioner(zp, 1e-4)   # (the same points through the Python layer, which keeps their number)
        # with a preconditioner set: T > 0 through the plain calls, NULL probes_k, diag == 0
        assert lib.svgp_cg_fit(h, dev.h, C.byref(desc), None, 2, z.ctypes.data_as(dp), C.byref(out), C.byref(info)) == INV
        assert lib.svgp_cg_lml_grad(h, dev.h, C.byref(desc), None, 2, z.ctypes.data_as(dp), C.byref(out), C.byref(info), C.byref(ld),
                                    np.zeros(d).ctypes.data_as(dp), None, None) == INV
        assert lib.svgp_cg_fit_precond(h, dev.h, C.byref(desc), None, 2, z.ctypes.data_as(dp), None, C.byref(out), C.byref(info)) == INV
        assert lib.svgp_cg_solve(h, dev.h, C.byref(zero), 1, _ffi._ptr(B), N, _ffi._ptr(X), N, 0, None, None, C.byref(info)) == INV
        assert lib.svgp_cg_precond_apply(h, dev.h, C.byref(zero), 1, _ffi._ptr(B), N, _ffi._ptr(X), N, 0, C.byref(ld)) == INV
        assert lib.svgp_cg_fit(h, dev.h, C.byref(zero), None, 0, None, C.byref(out), C.byref(info)) == INV
        assert lib.svgp_cg_precond_cross(h, dev.h, C.byref(desc), 1, _ffi._ptr(B), N - 1, _ffi._ptr(X), N, 0) == INV
        assert lib.svgp_cg_precond_cross(h, dev.h, C.byref(desc), 1, _ffi._ptr(B), N, _ffi._ptr(X), 15, 0) == INV
        assert lib.svgp_cg_precond_apply(h, dev.h, C.byref(desc), 0, _ffi._ptr(B), N, _ffi._ptr(X), N, 0, C.byref(ld)) == INV
        # T = 0 through the plain call uses the preconditioner
        assert lib.svgp_cg_fit(h, dev.h, C.byref(desc), None, 0, None, C.byref(out), C.byref(info)) == _ffi.OK and info.converged == 1
        # Kuu + jitter that does not factor: two coincident points and no jitter.  NaN outputs, SVGP_NOT_POSDEF
        twice = np.asfortranarray(np.column_stack([zp[:, :1]] * 2 + [zp[:, 1:15]]))
        assert setp(_ffi.COLVECS, 16, twice, 0.0) == _ffi.OK
        Xn = np.zeros_like(B)
        rc = lib.svgp_cg_solve(h, dev.h, C.byref(desc), 1, _ffi._ptr(B), N, _ffi._ptr(Xn), N, 0, None, None, C.byref(info))
        assert rc == _ffi.NOT_POSDEF and np.isnan(Xn).all() and np.isnan(info.max_rel_residual)
        An = np.zeros_like(B)
        assert lib.svgp_cg_precond_apply(h, dev.h, C.byref(desc), 1, _ffi._ptr(B), N, _ffi._ptr(An), N, 0, C.byref(ld)) == _ffi.NOT_POSDEF
        assert np.isnan(An).all() and np.isnan(ld.value)
        with pytest.raises(_ffi.PosDefException):
            dev.fit(desc, z, probes_k=zk)
        # and healthy calls afterwards: the preconditioned solve, then a plain fit equal to the first one
        assert setp(_ffi.COLVECS, 16, zp, 1e-4) == _ffi.OK
        Xh, iters, rel, inf = dev.solve(desc, B)
        assert inf.converged == 1 and np.abs(cr.khat(_okernel(M32, d), x, 0.01) @ Xh[:, 0] - y).max() <= 1e-8 * np.abs(y).max()
        dev.set_preconditioner(None)
        assert dev.fit(desc, z)[0] == lml_plain
    finally:
        dev.free()


def test_report_observed_errors():
    """Prints the table profiles/cg/accuracy_precond.md records (run the module with -s); SVGP_CG_PRECOND_ACCURACY_MD=path also writes it."""
    lines = ["| check | measured |", "|---|---|"] + [f"| {name} | {text} |" for name, text in OBSERVED.items()]
    print("\n".join(lines))
    path = os.environ.get("SVGP_CG_PRECOND_ACCURACY_MD")
    if path:
        with open(path, "w") as fh:
            fh.write("\n".join(lines) + "\n")
