"""GPU checks of the pathwise function samples of the exact GP (csrc/cg_sample.hip, cg_api.hip; svgp_cg_sampler_*) against the float64
restatement tests/cg_sample_ref.py (itself pinned to central differences, to cg_ref's posterior mean and to the exact posterior's
moments in tests/test_cg_sample_cpu.py).  Inputs are seeded as in test_gpu_cg.py: x ~ U[-3, 3]^d, lengthscale 0.7, variance 1.3.

Bounds.  Data stage (given the V the device holds after ONE CG iteration, read with state), fp64: error <= 1e-12 x the largest per-point
sum of the absolute values of the terms of the case, the suite's matvec bound (test_gpu_cg.py); the gradient uses its own terms' sum.
fp32: at most 4 x the error of the restatement's float32 chain on the same case, both measured against the float64 restatement of the
float32-rounded inputs (the suite's existing rule).  The bitwise contracts are compared with array_equal.  The solve: converged,
|f_s(X) + sigma eps_s + sigma^2 V_s - y|_2 <= tol |b_s|_2 + sqrt(N) 1e-12 scale (scale: the largest sum of absolute terms at X), V within
cond(Khat) tol of the dense solve with cond computed here; fp32 at the project's 1e-4 contract.  Moments: five standard errors.
test_report_observed_errors prints every measured figure (profiles/cg/accuracy_sample.md records a run on an MI355X)."""
import ctypes as C
import functools
import warnings

import numpy as np
import pytest
import torch

import cg_ref as cr
import cg_sample_ref as sr
import svgp_oracle as o
from approxgp import (GP, ConjugateGradients, DeviceConjugateGradients, SEKernel, _ffi, cg_sample_plan, posterior)
from approxgp.kernels import ARDTransform, Matern32Kernel, Matern52Kernel, ScaledKernel, TransformedKernel
from approxgp.pathwise import draw_basis

pytestmark = pytest.mark.gpu

F64, F32 = np.float64, np.float32
SE, M32, M52 = o.KERNEL_SE, o.KERNEL_MATERN32, o.KERNEL_MATERN52
FAMILIES = [SE, M32, M52]
BASES = {SE: SEKernel, M32: Matern32Kernel, M52: Matern52Kernel}
VAR, LS, DIAG, MEAN = 1.3, 0.7, 0.1, 0.3
OBSERVED = {}   # name -> text of the measured figures (printed by the last test)


def _kernel(family, d):
    return ScaledKernel(TransformedKernel(BASES[family](), ARDTransform(np.full(d, 1.0 / LS))), VAR)


def _okernel(family, d, dtype=F64):
    il = np.full(d, 1.0 / LS).astype(dtype).astype(F64)
    return o.Kernel(family, float(dtype(VAR)), il)


@pytest.fixture(scope="module")
def ctx():
    c = _ffi.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def _xy(N, d, seed=0):
    rng = np.random.default_rng(1000 + 7 * N + 13 * d + seed)
    x = rng.uniform(-3, 3, size=(d, N))
    y = np.sin(x.sum(0)) + 0.1 * rng.standard_normal(N)
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y


def _points(n, d, seed=0):
    return np.random.default_rng(5000 + 3 * n + 11 * d + seed).uniform(-3.2, 3.2, size=(d, n))


def _dev(ctx, x, y, dtype, layout=_ffi.COLVECS):
    if x.shape[0] == 1 and layout == _ffi.VEC:
        return DeviceConjugateGradients(ctx, x[0], y, dtype)
    if layout == _ffi.ROWVECS:
        return DeviceConjugateGradients(ctx, np.ascontiguousarray(x.T), y, dtype, layout=_ffi.ROWVECS)
    return DeviceConjugateGradients(ctx, x, y, dtype)


def _data(ctx, xs, dtype, layout):
    if xs.shape[0] == 1 and layout == _ffi.VEC:
        return _ffi.DeviceData(ctx, xs[0], None, dtype)
    if layout == _ffi.ROWVECS:
        return _ffi.DeviceData(ctx, np.ascontiguousarray(xs.T), None, dtype, _ffi.ROWVECS)
    return _ffi.DeviceData(ctx, xs, None, dtype)


# ---- 1. the data stage, every edge --------------------------------------------------------------------------------------------------
N3 = 2 * 512 + 100   # three row segments of 512 rows, the last one partial
ROUND = cg_sample_plan(N3)[2]
NS = [1, 31, 33, 65, 257, N3]
PS = [1, 15, 17, 64, 65, 257, ROUND + 17]
SS = [1, 16, 17, 64, 65, 130]
DS = [1, 8, 9, 17, 33, 64]
LL = [0, 1, 31, 33, 256]


def _stage_cases():
    """36 cases, a Latin square over (N, S, d) as test_gpu_cg's matvec cases: every (N, S), (N, d) and (S, d) pair occurs; L, n, the
    families, dtypes and layouts rotate.  n steps down its list while n S d exceeds 3e6 (the float64 reference of the gradient is an
    (S, d, n) array per term): the round + 17 points meet the narrow shapes.  L = 0 meets d <= 9 only, so the square is not Latin in L
    (every listed L still occurs): with these inputs (U[-3, 3]^d, lengthscale 0.7) every kernel entry is below 1e-30 from d = 17 on, a
    sample without features is then ONE entry near 1e-35, and the fp32 rule would compare two single float32 roundings of that entry,
    the device's and the chain's, whose ratio says nothing about either."""
    cases = []
    for i in range(6):
        for j in range(6):
            N, S, d = NS[i], SS[j], DS[(i + j) % 6]
            L = LL[(i + 2 * j) % 5]
            if L == 0 and d > 9:   # see the docstring
                L = LL[1 + (i + j) % 4]
            k = (5 * i + j) % 7
            while PS[k] * S * d > 3e6:
                k = (k - 1) % 7
            n = PS[k]
            family = FAMILIES[(i + 2 * j) % 3]
            dtype = [F64, F32][(i + j // 2) % 2]
            layout = _ffi.VEC if d == 1 and (i % 2) else [_ffi.COLVECS, _ffi.ROWVECS][(i + j) % 2]
            cases.append(pytest.param(N, n, S, d, L, family, dtype, layout,
                                      id=f"N{N}_n{n}_S{S}_d{d}_L{L}_k{family}_{np.dtype(dtype).name}_l{layout}"))
    return cases


def test_the_cases_cover_every_listed_size():
    got = [c.values for c in _stage_cases()]
    assert cg_sample_plan(N3)[:2] == (512, 3) and N3 % 512 != 0
    for col, want in ((0, NS), (1, PS), (2, SS), (3, DS), (4, LL)):
        assert {g[col] for g in got} == set(want), (col, want)
    assert {g[6] for g in got} == {F64, F32} and {g[5] for g in got} == set(FAMILIES) and len({g[7] for g in got}) == 3


@pytest.mark.parametrize("N,n,S,d,L,family,dtype,layout", _stage_cases())
def test_data_stage_against_the_restatement(ctx, N, n, S, d, L, family, dtype, layout):
    x, y = _xy(N, d)
    x, xs = x.astype(dtype), _points(n, d).astype(dtype)
    basis = draw_basis(family, N, L, S, np.random.default_rng(N + n + S + d + L), dtype, d=d)
    dev = _dev(ctx, x, y, dtype, layout)
    dat = _data(ctx, xs, dtype, layout)
    try:
        desc, keep = dev.desc(_kernel(family, d), DIAG, MEAN, tol=1e-8, maxiter=1)
        smp = dev.sampler(desc, basis)
        V, iters, rel = smp.state()
        F = smp.eval(dat)
        F2, G = smp.eval_grad(dat)
        smp.free()
    finally:
        dat.free()
        dev.free()
    assert V.shape == (N, S) and V.dtype == dtype and F.shape == (S, n) and G.shape == (S, d, n) and F.dtype == dtype and G.dtype == dtype
    assert iters.max() <= 1 and np.isfinite(V).all()
    assert np.array_equal(F, F2), "the gradient call's values differ from eval's"
    ok = _okernel(family, d, dtype)
    omega, tau, w, _ = basis
    Fr, A = sr.evaluate(ok, x.astype(F64), V.astype(F64), xs.astype(F64), omega.astype(F64), tau.astype(F64), w, MEAN)
    Gr, Ag = sr.gradient(ok, x.astype(F64), V.astype(F64), xs.astype(F64), omega.astype(F64), tau.astype(F64), w)
    ef, eg = float(np.abs(F - Fr).max()), float(np.abs(G - Gr).max())
    name = f"data stage N{N} n{n} S{S} d{d} L{L} k{family} {np.dtype(dtype).name}"
    if dtype == F64:
        OBSERVED[name] = (f"value error {ef:.2e} (bound {1e-12 * A.max():.2e}), gradient error {eg:.2e} (bound {1e-12 * Ag.max():.2e}), "
                          f"largest per-entry ratio {np.max(np.abs(F - Fr) / A):.1e} / {np.max(np.abs(G - Gr) / np.maximum(Ag, 1e-300)):.1e}")
        print(name, OBSERVED[name])
        assert ef <= 1e-12 * A.max(), (ef, A.max())
        assert eg <= 1e-12 * Ag.max(), (eg, Ag.max())
    else:
        F32r, _ = sr.evaluate(ok, x, V, xs, omega, tau, w, MEAN, f32=True)
        G32r, _ = sr.gradient(ok, x, V, xs, omega, tau, w, f32=True)
        rf, rg = float(np.abs(F32r - Fr).max()), float(np.abs(G32r - Gr).max())
        OBSERVED[name] = (f"value error {ef:.2e}, float32 chain {rf:.2e}, ratio {ef / max(rf, 1e-300):.2f}; gradient error {eg:.2e}, "
                          f"float32 chain {rg:.2e}, ratio {eg / max(rg, 1e-300):.2f}")
        print(name, OBSERVED[name])
        assert ef <= 4.0 * rf, (ef, rf)
        assert eg <= 4.0 * rg, (eg, rg)


# ---- 2. the bitwise contracts -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,d", [(F64, 9), (F32, 8), (F32, 17)])
def test_bitwise_contracts(ctx, dtype, d):
    N, S, L, n = N3, 65, 33, 300
    x, y = _xy(N, d)
    x, xs = x.astype(dtype), _points(n, d, 1).astype(dtype)
    omega, tau, w, eps = draw_basis(M52, N, L, S, np.random.default_rng(77), dtype, d=d)
    tdt = torch.float64 if dtype == F64 else torch.float32
    dev = _dev(ctx, x, y, dtype)
    dat = _ffi.DeviceData(ctx, xs, None, dtype)
    try:
        desc, keep = dev.desc(_kernel(M52, d), DIAG, MEAN, tol=1e-8, maxiter=5)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            smp = dev.sampler(desc, (omega, tau, w, eps))
        F = smp.eval(dat)
        Fv, G = smp.eval_grad(dat)
        assert np.array_equal(F, smp.eval(dat)) and np.array_equal(G, smp.eval_grad(dat)[1]), "repeated calls differ"
        assert np.array_equal(F, Fv), "the gradient call's values differ from eval's"
        assert np.array_equal(G, smp.eval_grad(dat, values=False)[1]), "the gradient depends on whether the values were asked for"
        # a point alone, in a window, in a call of another length
        for j in (0, 7, 299):
            assert np.array_equal(smp.eval(dat, off=j, length=1)[:, 0], F[:, j])
            assert np.array_equal(smp.eval_grad(dat, off=j, length=1)[1][:, :, 0], G[:, :, j])
            assert np.array_equal(smp.eval(xs[:, j:j + 1])[:, 0], F[:, j])
        assert np.array_equal(smp.eval(dat, off=5, length=200), F[:, 5:205])
        Fw, Gw = smp.eval_grad(dat, off=33, length=97)
        assert np.array_equal(Fw, F[:, 33:130]) and np.array_equal(Gw, G[:, :, 33:130])
        assert np.array_equal(smp.eval(xs[:, 100:117]), F[:, 100:117])
        # host against device output
        ft = torch.empty((S, n), dtype=tdt, device="cuda")
        gt = torch.empty((S, d, n), dtype=tdt, device="cuda")
        ft2 = torch.empty_like(ft)
        torch.cuda.synchronize()
        smp.eval(dat, out=ft)
        smp.eval_grad(dat, out=ft2, grad_out=gt)
        assert np.array_equal(ft.cpu().numpy(), F) and np.array_equal(ft2.cpu().numpy(), F) and np.array_equal(gt.cpu().numpy(), G)
        V = smp.state()[0]
        # column s of the S = 65 sampler against the S = 1 sampler of the same draws
        for s in (0, 16, 64):
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                one = dev.sampler(desc, (omega, tau, w[s:s + 1], eps[s:s + 1]))
            assert np.array_equal(one.state()[0][:, 0], V[:, s]), "V of a column depends on the other columns"
            F1, G1 = one.eval_grad(dat)
            assert np.array_equal(F1[0], F[s]) and np.array_equal(G1[0], G[s]), "a column's values depend on the other columns"
            one.free()
        smp.free()
        # L = 0 and eps = 0: V is alpha of a fit with the same descriptor
        desc2, keep2 = dev.desc(_kernel(M52, d), DIAG, MEAN, tol=1e-6 if dtype == F64 else 1e-4, maxiter=400)
        zero = dev.sampler(desc2, (None, None, None, np.zeros((1, N), dtype=dtype)))
        dev.fit(desc2)
        assert np.array_equal(zero.state()[0][:, 0], dev.alpha()), "V differs from svgp_cg_alpha"
        zero.free()
    finally:
        dat.free()
        dev.free()


# ---- 3. the solve -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precond", [0, 32])
@pytest.mark.parametrize("L", [0, 64])
def test_solve_fp64(ctx, L, precond):
    N, d, S, tol = 300, 2, 5, 1e-10
    x, y = _xy(N, d)
    ok = _okernel(SE, d)
    omega, tau, w, eps = draw_basis(SE, N, L, S, np.random.default_rng(9), F64, d=d)
    dev = _dev(ctx, x, y, F64)
    try:
        if precond:
            dev.set_preconditioner(x[:, np.random.default_rng(2).choice(N, precond, replace=False)], 1e-4)
        desc, keep = dev.desc(_kernel(SE, d), DIAG, MEAN, tol=tol, maxiter=2000)
        smp = dev.sampler(desc, (omega, tau, w, eps))
        V, iters, rel = smp.state()
        FX = smp.eval(x)
        info = smp.info
        smp.free()
    finally:
        dev.free()
    assert info.converged == 1 and info.n_unconverged == 0 and rel.max() <= tol and iters.max() == info.iterations
    B = sr.rhs(ok, x, DIAG, y - MEAN, omega, tau, w, eps)
    Vd, Kh = sr.solve(ok, x, DIAG, B)
    scale = sr.evaluate(ok, x, V, x, omega, tau, w, MEAN)[1].max()
    res = np.linalg.norm(FX.T + np.sqrt(DIAG) * eps.T + DIAG * V - y[:, None], axis=0)
    bound = tol * np.linalg.norm(B, axis=0) + np.sqrt(N) * 1e-12 * scale
    cond = float(np.linalg.cond(Kh))
    ev = np.linalg.norm(V - Vd, axis=0) / np.linalg.norm(Vd, axis=0)
    name = f"solve fp64 L{L} precond{precond}"
    OBSERVED[name] = (f"iterations {info.iterations}, |f(X) + sigma eps + sigma^2 V - y| / bound {np.max(res / bound):.2e}, "
                      f"|V - V*| / |V*| {ev.max():.2e} (cond tol {cond * tol:.2e})")
    print(name, OBSERVED[name])
    assert np.all(res <= bound), (res, bound)
    assert ev.max() <= cond * tol, (ev.max(), cond * tol)


def test_solve_fp32(ctx):
    N, d, S, L = 300, 2, 5, 64
    x, y = _xy(N, d)
    x32, xs = x.astype(F32), _points(65, d, 2).astype(F32)
    ok = _okernel(SE, d, F32)
    omega, tau, w, eps = draw_basis(SE, N, L, S, np.random.default_rng(9), F32, d=d)
    dev = _dev(ctx, x32, y, F32)
    try:
        desc, keep = dev.desc(_kernel(SE, d), DIAG, MEAN, tol=1e-5, maxiter=2000)
        smp = dev.sampler(desc, (omega, tau, w, eps))
        F, G = smp.eval_grad(xs)
        info = smp.info
        smp.free()
    finally:
        dev.free()
    Fr, Gr, _ = sr.sample(ok, x32.astype(F64), float(F32(DIAG)), y.astype(F32).astype(F64) - float(F32(MEAN)), xs.astype(F64),
                          omega.astype(F64), tau.astype(F64), w, eps, float(F32(MEAN)))
    ef, eg = np.abs(F - Fr).max() / np.abs(Fr).max(), np.abs(G - Gr).max() / np.abs(Gr).max()
    OBSERVED["solve fp32"] = f"iterations {info.iterations}, converged {info.converged}, value {ef:.2e}, gradient {eg:.2e} (contract 1e-4)"
    print(OBSERVED["solve fp32"])
    assert info.converged == 1
    assert ef <= 1e-4 and eg <= 1e-4, (ef, eg)


# ---- 4. moments ---------------------------------------------------------------------------------------------------------------------
MOMENT_SEED = 0


def test_moments_against_the_predictive_distribution(ctx):
    N, S, L, d = 40, 512, 4096, 1
    x, y = _xy(N, d)
    xs = np.array([-3.4, -1.0, 0.3, 1.9, 3.6])
    f = GP(MEAN, _kernel(SE, d))
    post = posterior(ConjugateGradients(tol=1e-10, maxiter=500, n_probes=0), f(x[0], DIAG), y, ctx=ctx)
    try:
        m, v = post.mean_and_var(xs)
        fs = post.function_samples(S, L, rng=np.random.default_rng(MOMENT_SEED))
        F = fs(xs)
        assert F.shape == (5, S)
        assert np.array_equal(F, fs.value_and_grad(xs)[0]) and fs.grad(xs).shape == (5, S, 1)
        fs.free()
        zm = np.abs(F.mean(1) - m) / np.sqrt(v / S)
        zv = np.abs(F.var(1, ddof=1) - v) / (v * np.sqrt(2.0 / (S - 1)))
        OBSERVED["moments"] = f"largest z of the mean {zm.max():.2f}, of the variance {zv.max():.2f} (five standard errors allowed)"
        print(OBSERVED["moments"])
        assert zm.max() <= 5.0 and zv.max() <= 5.0
        # no features and no noise draw: the posterior mean, within the data stage's bound for each of the two kernels
        zero = post.dev.sampler(post._desc, (None, None, None, np.zeros((2, N))))
        F0 = zero.eval(xs)
        V = zero.state()[0]
        zero.free()
        A = sr.evaluate(_okernel(SE, d), x, V, xs[None, :], None, None, np.zeros((2, 0)), MEAN)[1]
        e0 = np.abs(F0 - post.mean(xs)[None, :]).max()
        OBSERVED["mean"] = f"|fs - mean| {e0:.2e} (bound {1e-12 * A.max():.2e})"
        print(OBSERVED["mean"])
        assert e0 <= 1e-12 * A.max()
    finally:
        post.dev.free()


# ---- 5. snapshot and errors ---------------------------------------------------------------------------------------------------------
def test_the_sampler_is_a_snapshot(ctx):
    N, d, S, L = 257, 3, 17, 31
    x, y = _xy(N, d)
    xs = _points(65, d, 3)
    basis = draw_basis(M32, N, L, S, np.random.default_rng(4), F64, d=d)
    dev = _dev(ctx, x, y, F64)
    desc, keep = dev.desc(_kernel(M32, d), DIAG, MEAN, tol=1e-8, maxiter=300)
    smp = dev.sampler(desc, basis)
    F, G = smp.eval_grad(xs)
    V = smp.state()[0]
    other, keep2 = dev.desc(ScaledKernel(TransformedKernel(SEKernel(), ARDTransform(np.full(d, 2.0))), 0.4), 0.5, -1.0, tol=1e-6, maxiter=50)
    dev.fit(other)
    F2, G2 = smp.eval_grad(xs)
    assert np.array_equal(F, F2) and np.array_equal(G, G2), "a later fit on the handle changed the sampler"
    dev.free()
    F3, G3 = smp.eval_grad(xs)
    assert np.array_equal(F, F3) and np.array_equal(G, G3) and np.array_equal(V, smp.state()[0]), "freeing the handle changed the sampler"
    smp.free()


def test_invalid_arguments_then_a_healthy_call(ctx):
    N, d, S, L = 65, 2, 3, 8
    x, y = _xy(N, d)
    omega, tau, w, eps = draw_basis(SE, N, L, S, np.random.default_rng(0), F64, d=d)
    lib = ctx.lib
    dev = _dev(ctx, x, y, F64)
    nod = _dev(ctx, x, None, F64)
    dat = _ffi.DeviceData(ctx, _points(33, d), None, F64)
    d3 = _ffi.DeviceData(ctx, _points(33, 3), None, F64)
    d32 = _ffi.DeviceData(ctx, _points(33, d), None, F32)
    try:
        good, keep = dev.desc(_kernel(SE, d), DIAG, MEAN, tol=1e-8, maxiter=200)
        P = _ffi._ptr

        def create(handle=dev, desc=good, delta=None, **kw):
            b = dict(L=L, S=S, omega=P(omega), tau=P(tau), w=P(w), eps=P(eps))
            b.update(kw)
            basis = _ffi.SampleBasis(b["L"], b["S"], b["omega"], b["tau"], b["w"], b["eps"])
            h, info = C.c_void_p(), _ffi.CGInfo()
            rc = lib.svgp_cg_sampler_create(ctx.h, handle.h, C.byref(desc) if desc is not None else None, delta, C.byref(basis), C.byref(h),
                                            C.byref(info))
            return rc, h

        def variant(**kw):
            ds, k = dev.desc(_kernel(SE, d), kw.pop("diag", DIAG), MEAN, tol=kw.pop("tol", 1e-8), maxiter=kw.pop("maxiter", 200))
            for name, val in kw.items():
                setattr(ds, name, val)
            return ds, k

        bad_descs = [variant(maxiter=0), variant(tol=0.0), variant(tol=float("nan")), variant(diag=-1.0), variant(variance=0.0),
                     variant(reserved=1), variant(kernel=7), variant(dtype=_ffi.F32), variant(d=3)]
        for ds, k in bad_descs:
            assert create(desc=ds)[0] == _ffi.INVALID_ARG
        assert create(desc=None)[0] == _ffi.INVALID_ARG
        for kw in (dict(S=0), dict(L=-1), dict(eps=None), dict(omega=None), dict(tau=None), dict(w=None)):
            assert create(**kw)[0] == _ffi.INVALID_ARG, kw
        assert create(handle=nod)[0] == _ffi.INVALID_ARG, "data without y and no delta"
        dev.set_preconditioner(x[:, :16], 1e-4)
        assert create(desc=variant(diag=0.0)[0])[0] == _ffi.INVALID_ARG, "diag == 0 with a preconditioner"
        dev.set_preconditioner(None)
        rc, h = create()
        assert rc == _ffi.OK and h.value
        out = np.zeros((S, 40))
        g = np.zeros((S, d, 40))
        ev = lambda data, off, n, o_, ldo, dv=0: lib.svgp_cg_sampler_eval(ctx.h, h, data.h, off, n, o_, ldo, dv)
        eg = lambda data, off, n, o_, ldo, g_, ldg, dv=0: lib.svgp_cg_sampler_eval_grad(ctx.h, h, data.h, off, n, o_, ldo, g_, ldg, dv)
        for rc in (ev(d3, 0, 33, P(out), 40), ev(d32, 0, 33, P(out), 40), ev(dat, -1, 5, P(out), 40), ev(dat, 30, 4, P(out), 40),
                   ev(dat, 0, 0, P(out), 40), ev(dat, 0, 33, P(out), 32), ev(dat, 0, 33, None, 40), ev(dat, 0, 33, P(out), 40, 2),
                   eg(d3, 0, 33, P(out), 40, P(g), 40), eg(d32, 0, 33, P(out), 40, P(g), 40), eg(dat, 30, 4, P(out), 40, P(g), 40),
                   eg(dat, 0, 33, P(out), 32, P(g), 40), eg(dat, 0, 33, P(out), 40, P(g), 32), eg(dat, 0, 33, P(out), 40, None, 40),
                   lib.svgp_cg_sampler_state(ctx.h, None, None, None, None)):
            assert rc == _ffi.INVALID_ARG
        # a healthy call on the same context, the values nullable in the gradient call
        assert ev(dat, 0, 33, P(out), 40) == _ffi.OK and eg(dat, 0, 33, None, 0, P(g), 40) == _ffi.OK
        assert np.isfinite(out[:, :33]).all() and np.isfinite(g[:, :, :33]).all() and np.abs(g[:, :, :33]).max() > 0
        assert lib.svgp_cg_sampler_state(ctx.h, h, None, None, None) == _ffi.OK
        assert lib.svgp_cg_sampler_free(ctx.h, h) == _ffi.OK and lib.svgp_cg_sampler_free(ctx.h, None) == _ffi.OK
    finally:
        for t in (dat, d3, d32, dev, nod):
            t.free()


def test_non_finite_inputs_and_one_iteration(ctx):
    N, d, S, L = 65, 2, 3, 8
    x, y = _xy(N, d)
    xs = _points(17, d)
    omega, tau, w, eps = draw_basis(SE, N, L, S, np.random.default_rng(0), F64, d=d)
    dev = _dev(ctx, x, y, F64)
    try:
        desc, keep = dev.desc(_kernel(SE, d), DIAG, MEAN, tol=1e-8, maxiter=200)
        bad = eps.copy()
        bad[1, 5] = np.nan
        smp = dev.sampler(desc, (omega, tau, w, bad))   # SVGP_OK
        F, G = smp.eval_grad(xs)
        assert smp.info.converged == 0 and not np.isfinite(F).any() and not np.isfinite(G).any() and np.isnan(smp.state()[0]).all()
        smp.free()
        one, keep1 = dev.desc(_kernel(SE, d), DIAG, MEAN, tol=1e-8, maxiter=1)
        with pytest.warns(RuntimeWarning):
            f = GP(MEAN, _kernel(SE, d))
            post = posterior(ConjugateGradients(tol=1e-8, maxiter=1, n_probes=0), f(x, DIAG), y, ctx=ctx)
        with pytest.warns(RuntimeWarning):
            fs = post.function_samples(2, 8, rng=np.random.default_rng(1))
        assert fs.sampler.info.converged == 0 and fs.sampler.info.iterations == 1 and fs.state()[1].max() == 1
        fs.free()
        post.dev.free()
        smp = dev.sampler(one, (omega, tau, w, eps))
        assert smp.info.converged == 0 and smp.info.n_unconverged == S
        smp.free()
        # the context is healthy
        smp = dev.sampler(desc, (omega, tau, w, eps))
        assert smp.info.converged == 1 and np.isfinite(smp.eval(xs)).all()
        smp.free()
    finally:
        dev.free()


# ---- 6. report ----------------------------------------------------------------------------------------------------------------------
def test_report_observed_errors():
    print()
    for k in sorted(OBSERVED):
        print(f"{k}: {OBSERVED[k]}")
    assert OBSERVED or True
