"""GPU checks of the exact GP by conjugate gradients with per-point noise variances (svgp_cg_set_noise, svgp_cg_lml_grad_noise; csrc/cg.hip,
cg_api.hip) against dense numpy and the restatement tests/cg_noise_ref.py (itself pinned to dense closed forms in
tests/test_cg_noise_cpu.py).  Inputs: test_gpu_cg.py's _xy, variance 1.3, lengthscale 0.7 and the three families;
s = exp(U[log 0.02, log 0.5]) from default_rng(11), diag 0.05, so sigma_i^2 = T(0.05) + T(s_i) and cond(Khat) is 2.3e2 to 4.6e2.

Bounds: the sibling suites' contracts, no new numbers.  matvec fp64: 1e-12 max_i sum_j |Khat_ij V_js|; fp32: 4 x the float32 chain's own
error.  lml, quad, logdet and the gradient blocks: 1e-8 relative in fp64, 1e-4 in fp32.  s_bar, relative to its largest entry: 1e-8 in
fp64; in fp32 the larger of 1e-4 and 4 x the float32 restatement's own error on the same inputs (precond_apply's rule).  P^-1 R and
log det P: test_gpu_cg_precond.py's bounds against dense float64.  The central differences of the dense logpdf (step 1e-5) are held to
1e-6 relative, the step's own truncation and rounding.  Every observed figure is printed (profiles/cg/accuracy_noise.md records a run
on an MI355X)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import cg_noise_ref as nr
import cg_precond_ref as pr
import cg_ref as cr
import svgp_oracle as o
from approxgp import GP, CGPosteriorGP, ConjugateGradients, Diagonal, _ffi, approx_lml, approx_lml_and_gradient, draw_probes, posterior
from test_gpu_cg import FAMILIES, VAR, _dev, _kernel, _okernel, _xy

pytestmark = pytest.mark.gpu

F64, F32 = np.float64, np.float32
SE, M32, M52 = FAMILIES
DIAG, MC = nr.DIAG, 0.25
OBSERVED = {}


@pytest.fixture(scope="module")
def ctx():
    c = _ffi.Context(0)
    yield c
    c.close()


def _name(dtype):
    return np.dtype(dtype).name


def _note(name, text):
    OBSERVED[name] = text
    print(name, text)


def _noise(N, dtype):
    """(s in the data dtype, sigma^2 as the device forms it, float64 values)"""
    s = nr.noise_vector(N).astype(dtype)
    return s, nr.sigma2(DIAG, s, dtype)


def test_the_inputs_are_the_sibling_suites():
    x, y = _xy(48, 1)
    x2, y2 = nr.xy(48, 1)
    assert np.array_equal(x, x2) and np.array_equal(y, y2)


# ---- 1. matvec against dense ----------------------------------------------------------------------------------------------------------
MATVEC = [(1, 1, 1), (17, 16, 8), (65, 17, 9), (257, 65, 33), (1000, 130, 1), (1000, 1, 64)]


@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("i", range(len(MATVEC)))
def test_matvec_against_dense(ctx, i, dtype):
    N, S, d = MATVEC[i]
    family = FAMILIES[i % 3]
    x, y = _xy(N, d)
    x = x.astype(dtype)
    s, sig2 = _noise(N, dtype)
    V = np.asfortranarray(np.random.default_rng(N + S + d).standard_normal((N, S)).astype(dtype))
    dev, fresh = _dev(ctx, x, None, dtype), _dev(ctx, x, None, dtype)
    try:
        desc, keep = dev.desc(_kernel(family, d), DIAG, tol=1e-8, maxiter=10)
        plain = fresh.matvec(desc, V)
        dev.set_noise(s)
        out = dev.matvec(desc, V)
        again = dev.matvec(desc, V)
        c = S // 2
        alone = dev.matvec(desc, V[:, c])
        Vt = torch.from_numpy(np.ascontiguousarray(V.T)).cuda()
        ot = torch.empty_like(Vt)
        torch.cuda.synchronize()
        dev.matvec(desc, Vt, out=ot)
        on_dev = ot.cpu().numpy().T
        dev.set_noise(torch.from_numpy(s).cuda())   # a device vector is the same snapshot
        from_dev = dev.matvec(desc, V)
        dev.set_noise(None)
        cleared = dev.matvec(desc, V)
    finally:
        dev.free()
        fresh.free()
    assert out.dtype == dtype and np.array_equal(out, again), "two calls differ"
    assert np.array_equal(out, on_dev), "host and device-memory panels differ"
    assert np.array_equal(out, from_dev), "a host and a device noise vector differ"
    assert np.array_equal(out[:, c], alone[:, 0]), "a column depends on its neighbours"
    assert np.array_equal(cleared, plain), "set_noise(None) is not a fresh handle"
    ok = _okernel(family, d, dtype)
    Kh = nr.khat(ok, x.astype(F64), sig2)
    ref = Kh @ V.astype(F64)
    err = float(np.abs(out.astype(F64) - ref).max())
    scale = float((np.abs(Kh) @ np.abs(V.astype(F64))).max())
    name = f"matvec N{N} S{S} d{d} k{family} {_name(dtype)}"
    if dtype == F64:
        _note(name, f"error {err:.2e}, bound {1e-12 * scale:.2e}")
        assert err <= 1e-12 * scale, (err, scale)
    else:
        e_ref = float(np.abs(nr.kmv_f32(ok, x, V, sig2).astype(F64) - ref).max())
        _note(name, f"error {err:.2e}, float32 chain {e_ref:.2e}, ratio {err / max(e_ref, 1e-300):.2f}")
        assert err <= 4.0 * e_ref, (err, e_ref)


# ---- 2. solve, fit and the gradient ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("family", FAMILIES)
def test_solve_and_unit_probe_lml_against_the_dense_exact_gp(ctx, family, dtype):
    N, d = 48, 1
    x, y = _xy(N, d)
    x, y = x.astype(dtype), y.astype(dtype)
    s, sig2 = _noise(N, dtype)
    tol = 1e-12 if dtype == F64 else 1e-5
    B = np.asfortranarray(np.column_stack([y, np.random.default_rng(3).standard_normal((N, 2))]).astype(dtype))
    dev = _dev(ctx, x, y, dtype)
    try:
        dev.set_noise(s)
        desc, keep = dev.desc(_kernel(family, d), DIAG, mean_const=MC, tol=tol, maxiter=2000)
        X, iters, rel, info = dev.solve(desc, B)
        lml, g, finfo = dev.lml_grad(desc, cr.unit_probes(N), wrt_noise=True)
    finally:
        dev.free()
    ok = _okernel(family, d, dtype)
    Kh = nr.khat(ok, x.astype(F64), sig2)
    cond = float(np.linalg.cond(Kh))
    ref = np.linalg.solve(Kh, B.astype(F64))
    err = np.linalg.norm(X.astype(F64) - ref, axis=0) / np.linalg.norm(ref, axis=0)
    delta = y.astype(F64) - MC
    lref = nr.dense_lml(ok, x.astype(F64), sig2, delta)
    c = 1e-8 if dtype == F64 else 1e-4
    e_lml = abs(lml - lref) / abs(lref)
    sb = nr.dense_noise_gradient(ok, x.astype(F64), sig2, delta)
    e_sb = float(np.abs(g["noise"].astype(F64) - sb).max() / np.abs(sb).max())
    name = f"solve / unit-probe lml N48 k{family} {_name(dtype)}"
    text = f"cond {cond:.2e}, iterations {iters.max()}, solve {err.max():.2e} (bound {cond * tol:.2e}), lml {e_lml:.2e}, s_bar against the exact gradient {e_sb:.2e}"
    assert info.converged == 1 and rel.max() <= tol and finfo.converged == 1
    assert err.max() <= cond * tol, (err, cond)
    assert e_lml <= c, (lml, lref)
    if dtype == F64:
        # central differences of the dense logpdf on 8 sampled indices
        h, worst = 1e-5, 0.0
        for i in np.random.default_rng(3).choice(N, size=8, replace=False):
            e = np.zeros(N)
            e[i] = h
            fd = (nr.dense_lml(ok, x, sig2 + e, delta) - nr.dense_lml(ok, x, sig2 - e, delta)) / (2 * h)
            worst = max(worst, abs(fd - g["noise"][i]) / np.abs(sb).max())
        text += f", central differences {worst:.2e}"
        _note(name, text)
        assert worst <= 1e-6
        assert e_sb <= 1e-8
        assert abs(g["diag"] - g["noise"].sum()) <= 1e-12 * np.abs(g["noise"]).sum()
    else:
        r32 = nr.estimate(ok, x.astype(F64), float(dtype(DIAG)), s.astype(F64), delta, cr.unit_probes(N), tol, 2000, dtype=F32, grad=True)
        e32 = float(np.abs(r32["grad"]["noise"].astype(F64) - sb).max() / np.abs(sb).max())
        _note(name, text + f" (float32 restatement {e32:.2e})")
        assert e_sb <= max(1e-4, 4.0 * e32), (e_sb, e32)


@functools.lru_cache(maxsize=None)
def _rademacher_reference(family, dtype, with_noise=True):
    """the float64 restatement and the dense-solve estimator on the dtype-rounded inputs, and the float32 restatement's own s_bar error"""
    N, d = 300, 2
    x, y = _xy(N, d)
    x, y = x.astype(dtype), y.astype(dtype)
    s, sig2 = _noise(N, dtype)
    if not with_noise:
        s, sig2 = None, np.full(N, float(dtype(DIAG)))
    z = draw_probes(N, 16, 4)
    tol = 1e-12 if dtype == F64 else 1e-5
    ok = _okernel(family, d, dtype)
    delta = y.astype(F64) - MC
    s64 = None if s is None else s.astype(F64)
    r = nr.estimate(ok, x.astype(F64), float(dtype(DIAG)), s64, delta, z, tol, 2000, grad=True)
    de = nr.dense_estimate(ok, x.astype(F64), sig2, delta, z)["grad"]["noise"]
    e32 = 0.0
    if dtype == F32:
        r32 = nr.estimate(ok, x.astype(F64), float(dtype(DIAG)), s64, delta, z, tol, 2000, dtype=F32, grad=True)
        e32 = float(np.abs(r32["grad"]["noise"].astype(F64) - de).max() / np.abs(de).max())
    return x, y, s, z, tol, r, de, e32


def _grad_err(g, ref):
    out = {}
    for k in ("variance", "diag", "mean_const"):
        out[k] = abs(g[k] - ref[k]) / max(abs(ref[k]), 1e-300)
    out["inv_lengthscale"] = float(np.abs(g["inv_lengthscale"] - ref["inv_lengthscale"]).max() / np.abs(ref["inv_lengthscale"]).max())
    return out


@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("family", FAMILIES)
def test_lml_grad_noise_with_rademacher_probes(ctx, family, dtype):
    x, y, s, z, tol, r, de, e32 = _rademacher_reference(family, dtype)
    N, d = 300, 2
    dev = _dev(ctx, x, y, dtype)
    try:
        dev.set_noise(s)
        desc, keep = dev.desc(_kernel(family, d), DIAG, mean_const=MC, tol=tol, maxiter=2000)
        lml, g, info = dev.lml_grad(desc, z, wrt_noise=True)
        lml2, g2, info2 = dev.lml_grad(desc, z, wrt_noise=True)
        st = torch.zeros(N, dtype=torch.float64 if dtype == F64 else torch.float32, device="cuda")
        torch.cuda.synchronize()
        lml3, g3, _ = dev.lml_grad(desc, z, wrt_noise=True, noise_grad_out=st)
        lml4, g4, info4 = dev.lml_grad(desc, z)   # the plain call on a handle with a vector
        lml5, info5 = dev.fit(desc, z)
    finally:
        dev.free()
    assert lml == lml2 == lml3 == lml4 == lml5 and np.array_equal(g["noise"], g2["noise"]), "repeated calls differ"
    assert g3["noise"] is st and np.array_equal(st.cpu().numpy(), g["noise"]), "host and device output differ"
    for k in ("variance", "diag", "mean_const"):
        assert g[k] == g4[k] == g3[k]
    assert np.array_equal(g["inv_lengthscale"], g4["inv_lengthscale"]) and info.quad == info4.quad == info5.quad
    c = 1e-8 if dtype == F64 else 1e-4
    ge = _grad_err(g, r["grad"])
    e_sb = float(np.abs(g["noise"].astype(F64) - de).max() / np.abs(de).max())
    e_sum = abs(g["diag"] - g["noise"].astype(F64).sum()) / np.abs(g["noise"]).astype(F64).sum()
    _note(f"lml_grad_noise rademacher k{family} {_name(dtype)}",
          f"iterations {info.iterations}, lml {abs(lml - r['lml']) / abs(r['lml']):.2e}, quad {abs(info.quad - r['quad']) / abs(r['quad']):.2e}, "
          f"logdet {abs(info.logdet - r['logdet']) / abs(r['logdet']):.2e}, " + ", ".join(f"{k} {v:.2e}" for k, v in ge.items())
          + f", s_bar {e_sb:.2e} (float32 restatement {e32:.2e}), d_diag - sum s_bar {e_sum:.2e}")
    assert info.converged == 1
    assert abs(lml - r["lml"]) <= c * abs(r["lml"]) and abs(info.quad - r["quad"]) <= c * abs(r["quad"])
    assert abs(info.logdet - r["logdet"]) <= c * max(abs(r["logdet"]), abs(r["lml"]))
    for k, v in ge.items():
        assert v <= c, (k, v, g, r["grad"])
    if dtype == F64:
        assert e_sb <= 1e-8 and e_sum <= 1e-12
    else:
        assert e_sb <= max(1e-4, 4.0 * e32), (e_sb, e32)


@pytest.mark.parametrize("dtype", [F64, F32])
def test_s_bar_on_a_handle_without_a_vector(ctx, dtype):
    family = M32
    x, y, _, z, tol, r, de, e32 = _rademacher_reference(family, dtype, False)
    dev = _dev(ctx, x, y, dtype)
    try:
        desc, keep = dev.desc(_kernel(family, 2), DIAG, mean_const=MC, tol=tol, maxiter=2000)
        lml0, g0, info0 = dev.lml_grad(desc, z)
        lml, g, info = dev.lml_grad(desc, z, wrt_noise=True)
    finally:
        dev.free()
    assert lml == lml0 and info.quad == info0.quad and info.logdet == info0.logdet
    for k in ("variance", "diag", "mean_const"):
        assert g[k] == g0[k]   # bitwise the plain call
    assert np.array_equal(g["inv_lengthscale"], g0["inv_lengthscale"])
    e_sb = float(np.abs(g["noise"].astype(F64) - de).max() / np.abs(de).max())
    e_sum = abs(g0["diag"] - g["noise"].astype(F64).sum()) / np.abs(g["noise"]).astype(F64).sum()
    _note(f"s_bar without a vector {_name(dtype)}", f"s_bar {e_sb:.2e} (float32 restatement {e32:.2e}), plain d_diag - sum s_bar {e_sum:.2e}")
    if dtype == F64:
        assert e_sb <= 1e-8 and e_sum <= 1e-12
    else:
        assert e_sb <= max(1e-4, 4.0 * e32) and e_sum <= 1e-5


# ---- 3. the preconditioner -------------------------------------------------------------------------------------------------------------
def _points(x, k, seed=5):
    return np.ascontiguousarray(x[:, np.random.default_rng(seed).choice(x.shape[1], size=k, replace=False)])


@functools.lru_cache(maxsize=None)
def _apply_reference(N, k, family, dtype):
    d = 2
    x, y = _xy(N, d)
    x = x.astype(dtype).astype(F64)
    zp = _points(x, k)
    s, sig2 = _noise(N, dtype)
    R = np.random.default_rng(7).standard_normal((N, 3)).astype(dtype)
    ok = _okernel(family, d, dtype)
    ny = nr.Nystrom(ok, x, zp, sig2)
    P = ny.dense()
    ref = np.linalg.solve(P, R.astype(F64))
    # log det P comes from the k-sized fp64 stage, which takes the descriptor's variance as the double it is (the data stage rounds it to
    # the data dtype): its reference is the dense P of that variance.  Rounding 1.3 to float32 moves log det P by about k 4e-8.
    ok64 = o.Kernel(family, VAR, ok.inv_lengthscale)
    logdet = float(np.linalg.slogdet(nr.Nystrom(ok64, x, zp, sig2).dense())[1])
    e32 = float(np.abs(nr.Nystrom(ok, x, zp, sig2, dtype=F32).apply(R).astype(F64) - ref).max()) if dtype == F32 else 0.0
    return x, zp, s, R, ref, logdet, e32


@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("N,k,family", [(300, 17, SE), (300, 129, M32), (2049, 257, M52)])
def test_precond_apply_against_dense(ctx, N, k, family, dtype):
    x, zp, s, R, ref, logdet, e32 = _apply_reference(N, k, family, dtype)
    dev = _dev(ctx, x.astype(dtype), None, dtype)
    try:
        desc, keep = dev.desc(_kernel(family, 2), DIAG, tol=1e-8, maxiter=10)
        dev.set_preconditioner(zp, 1e-4)
        dev.set_noise(s)
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
    name = f"apply N{N} k{k} k{family} {_name(dtype)}"
    if dtype == F64:
        _note(name, f"error {err / np.abs(ref).max():.2e} relative, log det P {eld:.2e}")
        assert err <= 1e-8 * np.abs(ref).max(), (err, np.abs(ref).max())
    else:
        _note(name, f"error {err:.2e}, float32 restatement {e32:.2e}, ratio {err / max(e32, 1e-300):.2f}, log det P {eld:.2e}")
        assert err <= 4.0 * e32, (err, e32)
    assert eld <= 1e-8, (ld, logdet)


@pytest.mark.parametrize("dtype", [F64, F32])
def test_exact_probes_with_a_preconditioner(ctx, dtype):
    """T = N + k exact probes: fit_precond is the exact lml, and the preconditioned lml_grad_noise is the unpreconditioned unit-probe gradient"""
    N, d, k, family = 48, 1, 8, M52
    x, y = _xy(N, d)
    x, y = x.astype(dtype), y.astype(dtype)
    s, sig2 = _noise(N, dtype)
    zp = _points(x, k)
    eps, xi = pr.exact_probes(N, k)
    tol = 1e-12 if dtype == F64 else 1e-5
    dev = _dev(ctx, x, y, dtype)
    try:
        dev.set_noise(s)
        desc, keep = dev.desc(_kernel(family, d), DIAG, mean_const=MC, tol=tol, maxiter=2000)
        lml0, g0, info0 = dev.lml_grad(desc, cr.unit_probes(N), wrt_noise=True)
        dev.set_preconditioner(zp, 1e-4)
        lmlf, infof = dev.fit(desc, eps, probes_k=xi)
        lml, g, info = dev.lml_grad(desc, eps, probes_k=xi, wrt_noise=True)
    finally:
        dev.free()
    ok = _okernel(family, d, dtype)
    lref = nr.dense_lml(ok, x.astype(F64), sig2, y.astype(F64) - MC)
    c = 1e-8 if dtype == F64 else 1e-4
    ge = _grad_err(g, g0)
    e_sb = float(np.abs(g["noise"].astype(F64) - g0["noise"].astype(F64)).max() / np.abs(g0["noise"]).max())
    _note(f"exact probes with a preconditioner {_name(dtype)}",
          f"lml {abs(lml - lref) / abs(lref):.2e}, against the unpreconditioned gradient: " + ", ".join(f"{k_} {v:.2e}" for k_, v in ge.items())
          + f", s_bar {e_sb:.2e}")
    assert lml == lmlf and info.converged == 1
    assert abs(lml - lref) <= c * abs(lref)
    for k_, v in ge.items():
        assert v <= c, (k_, v)
    if dtype == F64:
        assert e_sb <= c
    else:
        sb = nr.dense_noise_gradient(ok, x.astype(F64), sig2, y.astype(F64) - MC)
        r32 = nr.estimate(ok, x.astype(F64), float(dtype(DIAG)), s.astype(F64), y.astype(F64) - MC, cr.unit_probes(N), tol, 2000, dtype=F32, grad=True)
        e32 = float(np.abs(r32["grad"]["noise"].astype(F64) - sb).max() / np.abs(sb).max())
        assert e_sb <= max(c, 4.0 * e32), (e_sb, e32)


@pytest.mark.parametrize("dtype", [F64, F32])
def test_the_preconditioner_cuts_the_iterations(ctx, dtype):
    N, d, family = 300, 2, M32
    x, y = _xy(N, d)
    x, y = x.astype(dtype), y.astype(dtype)
    s, sig2 = _noise(N, dtype)
    tol = 1e-10 if dtype == F64 else 1e-5
    B = np.asfortranarray(y[:, None].astype(dtype))
    dev = _dev(ctx, x, None, dtype)
    try:
        dev.set_noise(s)
        desc, keep = dev.desc(_kernel(family, d), DIAG, tol=tol, maxiter=2000)
        X0, it0, rel0, info0 = dev.solve(desc, B)
        dev.set_preconditioner(_points(x, 129), 1e-4)
        X1, it1, rel1, info1 = dev.solve(desc, B)
    finally:
        dev.free()
    Kh = nr.khat(_okernel(family, d, dtype), x.astype(F64), sig2)
    ref = np.linalg.solve(Kh, B.astype(F64))
    cond = float(np.linalg.cond(Kh))
    e1 = float(np.linalg.norm(X1.astype(F64) - ref) / np.linalg.norm(ref))
    _note(f"preconditioned solve N300 k129 {_name(dtype)}", f"iterations {it1.max()} against {it0.max()}, error {e1:.2e} (bound {cond * tol:.2e})")
    assert info0.converged == 1 and info1.converged == 1
    assert it1.max() < it0.max(), (it1, it0)
    assert e1 <= cond * tol


# ---- 4. prediction and sampling -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F64, F32])
def test_predict_and_sampler_against_dense(ctx, dtype):
    N, d, family, S = 300, 2, M52, 3
    x, y = _xy(N, d)
    x, y = x.astype(dtype), y.astype(dtype)
    s, sig2 = _noise(N, dtype)
    xs = np.random.default_rng(5).uniform(-3, 3, size=(d, 65)).astype(dtype)
    eps = np.random.default_rng(9).standard_normal((S, N)).astype(dtype)
    tol = 1e-10 if dtype == F64 else 1e-5
    dev = _dev(ctx, x, y, dtype)
    try:
        dev.set_noise(s)
        desc, keep = dev.desc(_kernel(family, d), DIAG, mean_const=MC, tol=tol, maxiter=2000)
        dev.fit(desc)
        m, v, info = dev.predict(xs)
        smp = dev.sampler(desc, (None, None, None, eps))
        try:
            dev.set_noise(None)   # the sampler is a snapshot
            V, iters, rel = smp.state()
            F1, F2 = smp.eval(xs), smp.eval(xs)
        finally:
            smp.free()
    finally:
        dev.free()
    ok = _okernel(family, d, dtype)
    Kh = nr.khat(ok, x.astype(F64), sig2)
    cond = float(np.linalg.cond(Kh))
    delta = y.astype(F64) - MC
    mr, vr = nr.predict(ok, x.astype(F64), sig2, delta, xs.astype(F64), MC)
    em, ev = float(np.abs(m - mr).max()), float(np.abs(v - vr).max())
    Bref = nr.sample_rhs(delta, None, eps, sig2, dtype)
    Vref = np.linalg.solve(Kh, Bref.astype(F64))
    eV = np.linalg.norm(V.astype(F64) - Vref, axis=0) / np.linalg.norm(Vref, axis=0)
    _note(f"predict / sampler N300 {_name(dtype)}", f"mean {em:.2e}, variance {ev:.2e} (bounds {cond * tol * np.abs(mr).max():.2e}, "
          f"{cond * tol * ok.variance:.2e}), sampler V {eV.max():.2e} (bound {cond * tol:.2e})")
    assert info.converged == 1 and rel.max() <= tol
    assert em <= cond * tol * np.abs(mr).max() and ev <= cond * tol * ok.variance, (em, ev, cond * tol)
    assert eV.max() <= cond * tol, (eV, cond * tol)
    assert np.array_equal(F1, F2), "eval is not repeatable"
    assert np.isfinite(F1).all()


# ---- 5. parent-bitwise ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F64, F32])
@pytest.mark.parametrize("precond", [False, True])
def test_bitwise_the_existing_calls(ctx, dtype, precond):
    N, d, family = 257, 2, SE
    x, y = _xy(N, d)
    x, y = x.astype(dtype), y.astype(dtype)
    s, _ = _noise(N, dtype)
    z = draw_probes(N, 5, 4)
    zk = draw_probes(17, 5, 6) if precond else None
    V = np.asfortranarray(np.random.default_rng(1).standard_normal((N, 3)).astype(dtype))
    xs = np.random.default_rng(5).uniform(-3, 3, size=(d, 33)).astype(dtype)
    eps = np.random.default_rng(9).standard_normal((2, N)).astype(dtype)
    tol = 1e-10 if dtype == F64 else 1e-5

    def every_call(dev, desc):
        out = [dev.matvec(desc, V)]
        out += list(dev.solve(desc, V)[:3])
        lml, g, info = dev.lml_grad(desc, z, probes_k=zk, wrt_inputs=True)
        out += [lml, g["variance"], g["inv_lengthscale"], g["diag"], g["mean_const"], g["x"], info.quad, info.logdet, dev.alpha()]
        out += list(dev.predict(xs)[:2])
        if precond:
            out += list(dev.precond_apply(desc, V))
        smp = dev.sampler(desc, (None, None, None, eps))
        out += [smp.state()[0], smp.eval(xs)]
        smp.free()
        return out

    dev = _dev(ctx, x, y, dtype)
    try:
        if precond:
            dev.set_preconditioner(_points(x, 17), 1e-4)
        desc, keep = dev.desc(_kernel(family, d), DIAG, mean_const=MC, tol=tol, maxiter=2000)
        before = every_call(dev, desc)
        # the superset call hands back what lml_grad_inputs does
        lml, g, info = dev.lml_grad(desc, z, probes_k=zk, wrt_inputs=True, wrt_noise=True)
        dev.set_noise(s)
        with_vector = dev.matvec(desc, V)
        dev.set_noise(None)
        after = every_call(dev, desc)
    finally:
        dev.free()
    sup = [lml, g["variance"], g["inv_lengthscale"], g["diag"], g["mean_const"], g["x"], info.quad, info.logdet]
    for a, b in zip(before[4:12], sup):
        assert np.array_equal(np.asarray(a), np.asarray(b)), "lml_grad_noise(gx, gpn) differs from lml_grad_inputs"
    assert not np.array_equal(with_vector, before[0])
    assert len(before) == len(after)
    for i, (a, b) in enumerate(zip(before, after)):
        assert np.array_equal(np.asarray(a), np.asarray(b)), f"output {i} differs after set_noise / set_noise(None)"


# ---- 6. statuses ------------------------------------------------------------------------------------------------------------------------
def test_statuses_leave_the_context_healthy(ctx):
    N, d = 65, 2
    x, y = _xy(N, d)
    s, _ = _noise(N, F64)
    lib, h = ctx.lib, ctx.h
    INV, NPD, OK = _ffi.INVALID_ARG, _ffi.NOT_POSDEF, _ffi.OK
    dp = C.POINTER(C.c_double)
    z = draw_probes(N, 2, 0)
    dev = _dev(ctx, x, y, F64)
    try:
        desc, keep = dev.desc(_kernel(M32, d), DIAG, tol=1e-10, maxiter=500)
        B = np.asfortranarray(y[:, None].copy())
        X = np.zeros((N, 1), order="F")
        info, out, dv, dd, dm, dil = _ffi.CGInfo(), C.c_double(), C.c_double(), C.c_double(), C.c_double(), np.zeros(d)
        sb = np.zeros(N)

        def setn(vec, on_device=0, reserved=0):
            return lib.svgp_cg_set_noise(h, dev.h, C.byref(_ffi.PointNoise(_ffi._ptr(vec) if vec is not None else None, on_device, reserved)))

        def gradn(gpn, T=2):
            return lib.svgp_cg_lml_grad_noise(h, dev.h, C.byref(desc), None, T, z.ctypes.data_as(dp), None, C.byref(out), C.byref(info), C.byref(dv),
                                              dil.ctypes.data_as(dp), C.byref(dd), C.byref(dm), None, gpn)

        def healthy():
            assert lib.svgp_cg_fit(h, dev.h, C.byref(desc), None, 0, None, C.byref(out), C.byref(info)) == OK and info.converged == 1

        # bad arguments
        assert setn(None) == INV and setn(s, on_device=2) == INV and setn(s, reserved=1) == INV
        assert gradn(None) == INV
        assert gradn(C.byref(_ffi.PointNoiseGrad(None, 0, 0))) == INV
        assert gradn(C.byref(_ffi.PointNoiseGrad(_ffi._ptr(sb), 2, 0))) == INV
        assert gradn(C.byref(_ffi.PointNoiseGrad(_ffi._ptr(sb), 0, 1))) == INV
        healthy()
        # predict and alpha need a fit made after set_noise
        assert setn(s) == OK
        m = np.zeros(3)
        xs = np.asfortranarray(x[:, :3])
        assert lib.svgp_cg_predict(h, dev.h, _ffi.COLVECS, 3, _ffi._ptr(xs), _ffi._ptr(m), None, C.byref(info)) == INV
        assert lib.svgp_cg_alpha(h, dev.h, _ffi._ptr(sb)) == INV
        healthy()
        assert lib.svgp_cg_predict(h, dev.h, _ffi.COLVECS, 3, _ffi._ptr(xs), _ffi._ptr(m), None, C.byref(info)) == OK
        assert lib.svgp_cg_set_noise(h, dev.h, None) == OK
        assert lib.svgp_cg_alpha(h, dev.h, _ffi._ptr(sb)) == INV   # removing the vector drops the fit as well
        # a negative variance: diag + min s < 0
        neg = s.copy()
        neg[7] = -DIAG - 1e-3
        assert setn(neg) == OK
        X[:] = 0.0
        assert lib.svgp_cg_matvec(h, dev.h, C.byref(desc), 1, _ffi._ptr(B), N, _ffi._ptr(X), N, 0) == NPD and np.isnan(X).all()
        X[:] = 0.0
        assert lib.svgp_cg_solve(h, dev.h, C.byref(desc), 1, _ffi._ptr(B), N, _ffi._ptr(X), N, 0, None, None, C.byref(info)) == NPD
        assert np.isnan(X).all() and np.isnan(info.max_rel_residual)
        sb[:] = 0.0
        assert gradn(C.byref(_ffi.PointNoiseGrad(_ffi._ptr(sb), 0, 0))) == NPD and np.isnan(sb).all() and np.isnan(out.value)
        assert b"negative" in lib.svgp_last_error(h)
        # a zero variance is a semi-definite Khat without a preconditioner, and SVGP_NOT_POSDEF with one
        zero = s.copy()
        zero[7] = -DIAG
        assert setn(zero) == OK
        assert lib.svgp_cg_matvec(h, dev.h, C.byref(desc), 1, _ffi._ptr(B), N, _ffi._ptr(X), N, 0) == OK and np.isfinite(X).all()
        dev.set_preconditioner(_points(x, 16), 1e-4)
        assert lib.svgp_cg_solve(h, dev.h, C.byref(desc), 1, _ffi._ptr(B), N, _ffi._ptr(X), N, 0, None, None, C.byref(info)) == NPD and np.isnan(X).all()
        ld = C.c_double()
        assert lib.svgp_cg_precond_apply(h, dev.h, C.byref(desc), 1, _ffi._ptr(B), N, _ffi._ptr(X), N, 0, C.byref(ld)) == NPD and np.isnan(ld.value)
        dev.set_preconditioner(None)
        # a NaN in s
        nan = s.copy()
        nan[N - 1] = np.nan
        assert setn(nan) == OK
        X[:] = 0.0
        assert lib.svgp_cg_matvec(h, dev.h, C.byref(desc), 1, _ffi._ptr(B), N, _ffi._ptr(X), N, 0) == NPD and np.isnan(X).all()
        assert lib.svgp_cg_fit(h, dev.h, C.byref(desc), None, 0, None, C.byref(out), C.byref(info)) == NPD and np.isnan(out.value)
        # a good vector afterwards: a healthy fit on the same context
        assert setn(s) == OK
        healthy()
        assert gradn(C.byref(_ffi.PointNoiseGrad(_ffi._ptr(sb), 0, 0)), T=0) == OK and np.isnan(sb).all()   # T = 0: NaN like the other trace blocks
        # a handle on another device than the context cannot be made here; the check is the first in svgp_cg_set_noise
    finally:
        dev.free()


# ---- 7. the Python layer --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F64, F32])
def test_python_layer_with_a_diagonal(ctx, dtype):
    N, d = 48, 1
    x, y = _xy(N, d)
    x, y = x.astype(dtype), y.astype(dtype)
    v = (nr.noise_vector(N) + DIAG)
    f = GP(MC, _kernel(M32, d))
    fx = f(x[0], Diagonal(v))
    cg = ConjugateGradients(tol=1e-12 if dtype == F64 else 1e-5, maxiter=2000, probes=cr.unit_probes(N))
    lml = approx_lml(cg, fx, y, ctx=ctx, dtype=dtype)   # UnsupportedError before svgp_cg_set_noise
    lml2, g = approx_lml_and_gradient(cg, fx, y, ctx=ctx, dtype=dtype, wrt_noise=True)
    with pytest.raises(_ffi.UnsupportedError):   # the dispatch keeps refusing a Diagonal (tests/test_cg_cpu.py): the class is asked for by name
        posterior(cg, fx, y, ctx=ctx, dtype=dtype)
    post = CGPosteriorGP(cg, fx, y, ctx=ctx, dtype=dtype)
    xs = np.linspace(-3, 3, 17).astype(dtype)
    try:
        m, var = post.mean_and_var(xs)
        ym, yv = post.predict_y(xs, noise=0.1)
        lpd = post.log_predictive_density(xs, np.zeros(17), noise=np.full(17, 0.2))
        with pytest.raises(ValueError, match="pass noise="):
            post.predict_y(xs)
        fs = post.function_samples(2, 64, np.random.default_rng(0))
        F = fs(xs)
        fs.free()
    finally:
        post.dev.free()
    # the device forms sigma^2 = T(min v) + T(v - min v)
    sig2 = nr.sigma2(float(v.min()), v - v.min(), dtype)
    ok = _okernel(M32, d, dtype)
    delta = y.astype(F64) - MC
    ref = nr.dense_lml(ok, x.astype(F64), sig2, delta)
    sb = nr.dense_noise_gradient(ok, x.astype(F64), sig2, delta)
    mr, vr = nr.predict(ok, x.astype(F64), sig2, delta, xs.astype(F64)[None, :], MC)
    c = 1e-8 if dtype == F64 else 1e-4
    e_sb = float(np.abs(g["Sigma_y"].astype(F64) - sb).max() / np.abs(sb).max())
    _note(f"python Diagonal {_name(dtype)}", f"lml {abs(lml - ref) / abs(ref):.2e}, Sigma_y {e_sb:.2e}, mean {np.abs(m - mr).max():.2e}, var {np.abs(var - vr).max():.2e}")
    assert lml == lml2 == post.lml and abs(lml - ref) <= c * abs(ref)
    e32 = 0.0
    if dtype == F32:
        r32 = nr.estimate(ok, x.astype(F64), float(dtype(v.min())), (v - v.min()).astype(dtype).astype(F64), delta, cr.unit_probes(N),
                          cg.tol_for(dtype), 2000, dtype=F32, grad=True)
        e32 = float(np.abs(r32["grad"]["noise"].astype(F64) - sb).max() / np.abs(sb).max())
    assert g["Sigma_y"].shape == (N,) and e_sb <= (1e-8 if dtype == F64 else max(1e-4, 4.0 * e32)), (e_sb, e32)
    assert abs(g["diag"] - g["Sigma_y"].astype(F64).sum()) <= (1e-12 if dtype == F64 else 1e-5) * np.abs(g["Sigma_y"]).astype(F64).sum()
    cond = float(np.linalg.cond(nr.khat(ok, x.astype(F64), sig2)))
    tol = cg.tol_for(dtype)
    assert np.abs(m - mr).max() <= max(c, cond * tol) * np.abs(mr).max() and np.abs(var - vr).max() <= max(c, cond * tol) * ok.variance
    np.testing.assert_allclose(ym, m, rtol=1e-6)
    np.testing.assert_allclose(yv, var.astype(F64) + 0.1, rtol=1e-5)
    yv2 = var.astype(F64) + 0.2
    np.testing.assert_allclose(lpd, -0.5 * (np.log(2 * np.pi * yv2) + m.astype(F64) ** 2 / yv2), rtol=1e-12)
    assert F.shape == (17, 2) and np.isfinite(F).all()


def test_report_observed_errors():
    print("\n".join(f"{k}: {v}" for k, v in OBSERVED.items()))
