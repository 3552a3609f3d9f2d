"""GPU checks of the NearestNeighbors approximation with neighbour tables (csrc/nn.hip: svgp_nn_set_neighbors / _build_neighbors /
_get_neighbors / _clear_neighbors and the table mode of lml / lml_grad / fit / factors / predict) against tests/nn_sets_ref.py.

Sizes sit at the kernel's seams: the k buckets 16 / 32 / 64, four points per workgroup, 64-candidate tiles, 64-row V groups.
Tolerances are those of tests/test_gpu_nn.py for the same quantities (the arithmetic per point is unchanged): lml 1e-8 (fp64) / 1e-4
(fp32) relative; gradient 1e-6 / 1e-3 of the largest kernel-parameter entry, d / d diag on its own scale; factors 1e-9 / 4 eps32 k
variance / diag; predictions 1e-9 / 1e-4 of the largest mean and of the prior variance."""
import ctypes as C

import numpy as np
import pytest
import torch

import nn_ref as nr
import nn_sets_ref as ns
import svgp_oracle as o
from approxgp import GP, DeviceNearestNeighbors, NearestNeighbors, SEKernel, _ffi, approx_lml, approx_lml_and_gradient, posterior
from approxgp.kernels import ARDTransform, Matern32Kernel, Matern52Kernel, ScaledKernel, TransformedKernel

pytestmark = pytest.mark.gpu

F64, F32 = np.float64, np.float32
BASES = {o.KERNEL_SE: SEKernel, o.KERNEL_MATERN32: Matern32Kernel, o.KERNEL_MATERN52: Matern52Kernel}
VAR, DIAG = 1.2, 1e-2


def _kernel(family, var, il):
    return ScaledKernel(TransformedKernel(BASES[family](), ARDTransform(np.asarray(il, dtype=np.float64))), var)


@pytest.fixture(scope="module")
def ctx():
    c = _ffi.Context(0)
    yield c
    c.close()


def _dev(ctx, x, y, dtype, layout=_ffi.COLVECS):
    if layout == _ffi.ROWVECS:
        return DeviceNearestNeighbors(ctx, np.asarray(x).T, y, dtype, layout=_ffi.ROWVECS)
    if layout == _ffi.VEC:
        return DeviceNearestNeighbors(ctx, np.asarray(x)[0], y, dtype)
    return DeviceNearestNeighbors(ctx, x, y, dtype)


# ---- window table == no table ------------------------------------------------------------------------------------
WN, WK, WD = [1, 2, 17, 65, 130, 301], [3, 16, 17, 33, 64], [1, 3, 17]


def _window_cases():
    """30 cases: every (N, k) pair once; d, layout, dtype and family cycle through them (every dtype x family pair occurs)"""
    cases = []
    for a, n in enumerate(WN):
        for b, k in enumerate(WK):
            i = a * len(WK) + b
            d = WD[(a + b) % 3]
            layout = _ffi.VEC if d == 1 else [_ffi.COLVECS, _ffi.ROWVECS][(a + i) % 2]
            cases.append((n, k, d, layout, [F64, F32][i % 2], (i // 2) % 3))
    assert {c[3] for c in cases} == {0, 1, 2} and {(c[4], c[5]) for c in cases} == {(t, f) for t in (F64, F32) for f in range(3)}
    return cases


@pytest.mark.parametrize("n,k,d,layout,dtype,fam", _window_cases())
def test_window_table_is_bitwise_the_window(ctx, n, k, d, layout, dtype, fam):
    x, y = nr.synth(n, d, seed=2000 + n + k, dtype=dtype)
    il = nr.invl_for(d, True)
    dev = _dev(ctx, x, y, dtype, layout)
    desc, keep = dev.desc(_kernel(fam, VAR, il), k, DIAG, 0.1)
    a = dev.lml_grad(desc)
    a0 = dev.lml(desc)[0]
    dev.fit(desc)
    Bw, Fw, alw = dev.factors()
    xs = np.random.default_rng(n + k).uniform(-2, 2, size=(d, 5)).astype(dtype)
    xs = xs[0] if d == 1 else xs
    pw = dev.predict(xs, cov=True)
    assert dev.neighbors() is None
    tab = ns.window_table(n, k)
    dev.set_neighbors(tab)
    assert np.array_equal(dev.neighbors(), tab)
    b = dev.lml_grad(desc)
    b0 = dev.lml(desc)[0]
    bf = dev.fit(desc)[0]
    Bt, Ft, alt = dev.factors()
    pt = dev.predict(xs, cov=True)
    dev.free()
    assert a0 == b0 == bf and a[0] == b[0] and a[1] == b[1] and a[3] == b[3] and np.array_equal(a[2], b[2])
    kb = min(k, n - 1)
    tol = 1e-9 if dtype == F64 else 4 * np.finfo(F32).eps * k * VAR / DIAG
    Bw_t = np.zeros_like(Bt)   # the band, re-indexed by the table
    for i in range(n):
        m = min(i, kb)
        Bw_t[i, :m] = Bw[i, kb - m:]
    assert np.max(np.abs(Bt - Bw_t), initial=0.0) <= tol * max(np.max(np.abs(Bw), initial=0.0), 1e-300)
    assert np.array_equal(Ft, Fw)
    assert np.max(np.abs(alt - alw)) <= tol * np.max(np.abs(alw))
    tm, tv = (1e-9, 1e-9) if dtype == F64 else (1e-4, 1e-4 * VAR)
    np.testing.assert_allclose(pt[0], pw[0], rtol=0, atol=tm * max(np.max(np.abs(pw[0])), 1e-300))
    np.testing.assert_allclose(pt[1], pw[1], rtol=0, atol=tv)
    np.testing.assert_allclose(pt[2], pw[2], rtol=0, atol=tv)


# ---- the search ------------------------------------------------------------------------------------------------------
def _lattice(n, d, seed):
    """integer coordinates in 0 .. 3 (many exact ties, duplicate points)"""
    return np.random.default_rng(seed).integers(0, 4, size=(d, n)).astype(np.float64)


SN, SK, SD = [1, 2, 63, 64, 65, 129, 300], [1, 16, 17, 64], [1, 2, 8]


@pytest.mark.parametrize("n", SN)
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_search_exact_on_a_lattice(ctx, n, dtype):
    for a, k in enumerate(SK):
        d = SD[(a + SN.index(n)) % 3]
        x = _lattice(n, d, seed=n + k).astype(dtype)
        il = [None, np.full(d, 2.0), 2.0 ** -np.arange(d)][(a + n) % 3]   # unit and power-of-two metrics: every distance is exact
        dev = _dev(ctx, x, np.zeros(n, dtype=dtype), dtype, _ffi.VEC if d == 1 else _ffi.COLVECS)
        dev.build_neighbors(k, il)
        got = dev.neighbors()
        dev.free()
        ref = ns.nearest_table(x, k, il, dtype)
        assert got.shape == ref.shape == (n, min(k, n - 1))
        assert np.array_equal(got, ref), (n, k, d, np.argwhere(got != ref)[:5])


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_search_sorted_1d_is_the_window(ctx, dtype):
    x = np.sort(np.random.default_rng(5).uniform(-2, 2, 300)).astype(dtype)
    dev = DeviceNearestNeighbors(ctx, x, np.zeros(300, dtype=dtype), dtype)
    for k in (1, 17, 64):
        dev.build_neighbors(k, [0.7])
        assert np.array_equal(dev.neighbors(), ns.window_table(300, k))
    dev.free()


@pytest.mark.parametrize("dtype,k,d", [(F64, 17, 3), (F32, 64, 8), (F32, 10, 2)])
def test_search_random_inputs(ctx, dtype, k, d):
    n = 300
    x = np.random.default_rng(k).uniform(-2, 2, size=(d, n)).astype(dtype)
    il = np.linspace(0.6, 1.7, d)
    dev = _dev(ctx, x, np.zeros(n, dtype=dtype), dtype)
    dev.build_neighbors(k, il)
    tab = dev.neighbors()
    dev.free()
    eps = np.finfo(dtype).eps
    for i in range(n):
        r = tab[i][tab[i] >= 0]
        m = min(i, k)
        assert len(r) == m and np.all(tab[i, m:] == -1) and np.all(np.diff(r) > 0) and np.all(r < i)
        if m:
            d2 = ns.search_dist2(x, i, il, dtype).astype(F64)
            assert np.max(d2[r]) <= np.sort(d2)[m - 1] * (1 + 8 * eps), i


# ---- parity on real tables ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def problem():
    """n = 300, d = 2, k = 17; the references per (table kind, dtype) are computed once"""
    x, y = nr.synth(300, 2, seed=7)
    il = np.array([0.8, 1.1])
    kern = nr.kernel_of(o.KERNEL_MATERN52, VAR, il)
    k = 17
    cache = {}

    def hub_table(xd):
        t = ns.nearest_table(xd, k - 1, il)
        tab = np.full((300, k), -1, dtype=np.int32)
        for i in range(1, 300):
            r = sorted(set(ns.row(t, i)) | {0})   # point 0 in every row: its reverse list has 299 pairs
            if i % 5 == 0:
                r = r[:max(1, len(r) // 2)]       # short rows
            tab[i, :len(r)] = r
        return tab

    def ref(kind, dtype):
        if (kind, dtype) not in cache:
            xd, yd = x.astype(dtype).astype(F64), y.astype(dtype).astype(F64)
            tab = hub_table(xd) if kind == "hub" else None
            cache[(kind, dtype)] = (tab, xd, yd)
        return cache[(kind, dtype)]

    return dict(x=x, y=y, il=il, kern=kern, k=k, ref=ref, dkern=_kernel(o.KERNEL_MATERN52, VAR, il), fits={})


@pytest.mark.parametrize("kind", ["built", "hub"])
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_parity_on_real_tables(ctx, problem, kind, dtype):
    p = problem
    k = p["k"]
    tab, xd, yd = p["ref"](kind, dtype)
    dev = _dev(ctx, p["x"].astype(dtype), p["y"].astype(dtype), dtype)
    if kind == "built":
        dev.build_neighbors(k, p["il"])
        tab = dev.neighbors()   # the device's own table: the selection itself is checked above
        assert not np.array_equal(tab, ns.window_table(300, k))
    else:
        dev.set_neighbors(tab)
    desc, keep = dev.desc(p["dkern"], k, DIAG, 0.2)
    lml, gv, gil, gd, info = dev.lml_grad(desc)
    lml_fit, _ = dev.fit(desc)
    B, F, alpha = dev.factors()
    r = ns.fit(p["kern"], xd, yd, tab, DIAG, mean_const=0.2)
    rl, rv, ril, rd = ns.lml_grad(p["kern"], xd, yd, tab, DIAG, 0.2)
    f64 = dtype == F64
    print(f"{kind} {np.dtype(dtype).name}: lml {abs(lml - rl) / abs(rl):.2e}")
    assert info.first_bad == 0 and lml_fit == lml
    assert abs(lml - rl) <= (1e-8 if f64 else 1e-4) * abs(rl)
    g, gr = np.concatenate([[gv], gil]), np.concatenate([[rv], ril])
    assert np.max(np.abs(g - gr)) <= (1e-6 if f64 else 1e-3) * np.max(np.abs(gr)), (g, gr)
    assert abs(gd - rd) <= (1e-6 if f64 else 1e-3) * abs(rd)
    tol = 1e-9 if f64 else 4 * np.finfo(F32).eps * k * VAR / DIAG
    Br = ns.table_factors(r["B"], tab)
    assert np.all(B[tab < 0] == 0)
    assert np.max(np.abs(B - Br)) <= tol * np.max(np.abs(Br))
    assert np.max(np.abs(F - r["F"]) / r["F"]) <= tol
    assert np.max(np.abs(alpha - r["alpha"])) <= tol * np.max(np.abs(r["alpha"]))
    for nstar in (1, 63, 64, 65, 130):
        rng = np.random.default_rng(100 + nstar)
        xs = rng.uniform(-2, 2, size=(2, nstar)).astype(dtype)
        ys = rng.uniform(-2, 2, size=(2, 7)).astype(dtype)
        m, v, c = dev.predict(xs, cov=True)
        cx = dev.cross_cov(xs, ys)
        rm, rvv, rc = ns.predict(r, p["kern"], xd, xs.astype(F64))
        _, _, rcx = ns.predict(r, p["kern"], xd, xs.astype(F64), ys.astype(F64))
        tol_m, tol_v = (1e-9 * np.max(np.abs(rm)), 1e-9) if f64 else (1e-4 * np.max(np.abs(rm)), 1e-4 * VAR)
        np.testing.assert_allclose(m, rm, rtol=0, atol=tol_m)
        np.testing.assert_allclose(v, rvv, rtol=0, atol=tol_v)
        np.testing.assert_allclose(c, rc, rtol=0, atol=tol_v)
        np.testing.assert_allclose(cx, rcx, rtol=0, atol=tol_v)
    dev.free()


def test_all_nearest_neighbours_is_the_exact_gp(ctx):
    n, d = 40, 2
    x, y = nr.synth(n, d, seed=1)
    il = np.array([0.8, 1.1])
    kern = nr.kernel_of(o.KERNEL_MATERN52, VAR, il)
    f = GP(0.3, _kernel(o.KERNEL_MATERN52, VAR, il))
    ex = nr.exact_lml(kern, x, y, DIAG, mean_const=0.3)
    for k in (n - 1, n + 7):
        v = approx_lml(NearestNeighbors(k, include_noise=True, neighbors="nearest"), f(x, DIAG), y, ctx=ctx)
        assert abs(v - ex) <= 1e-8 * abs(ex), (k, v, ex)
    v2, g = approx_lml_and_gradient(NearestNeighbors(n - 1, include_noise=True, neighbors="nearest"), f(x, DIAG), y, ctx=ctx)
    assert abs(v2 - ex) <= 1e-8 * abs(ex) and set(g) == {"variance", "inv_lengthscale", "diag"}
    post = posterior(NearestNeighbors(n - 1, include_noise=True, neighbors="nearest"), f(x, DIAG), y, ctx=ctx)
    assert np.array_equal(post.dev.neighbors(), ns.window_table(n, n - 1))   # all predecessors, ascending
    xs = np.random.default_rng(2).uniform(-2, 2, size=(d, 30))
    m, c = post.mean_and_cov(xs)
    post.dev.free()
    em, ec = nr.exact_predict(kern, x, y, DIAG, xs, mean_const=0.3)
    np.testing.assert_allclose(m, em, rtol=0, atol=1e-9 * np.max(np.abs(em)))
    np.testing.assert_allclose(c, ec, rtol=0, atol=1e-9)


@pytest.mark.parametrize("family", [o.KERNEL_SE, o.KERNEL_MATERN32, o.KERNEL_MATERN52])
def test_nearest_sets_halve_the_kl_divergence_on_the_device(ctx, family):
    """the CPU problem of tests/test_nn_sets_cpu.py with y = mean_const, so that lml = -1/2 sum (log 2 pi + log F_i); log det from numpy"""
    q = ns.QUALITY
    kern = nr.kernel_of(family, q["variance"], q["inv_lengthscale"])
    f = GP(0.5, _kernel(family, q["variance"], q["inv_lengthscale"]))
    for seed in q["seeds"]:
        x = ns.quality_problem(seed)
        y = np.full(600, 0.5)
        ld = ns.logdet_exact(kern, x, q["diag"])
        kl = {}
        for name, nb in (("window", None), ("nearest", "nearest")):
            v = approx_lml(NearestNeighbors(q["k"], include_noise=True, neighbors=nb), f(x, q["diag"]), y, ctx=ctx, dtype=F64)
            kl[name] = (-2.0 * v - 600 * nr.LOG2PI) - ld
        print(f"family {family} seed {seed}: 2 KL window {kl['window']:.2f} nearest {kl['nearest']:.2f}")
        assert kl["nearest"] > 0 and kl["nearest"] <= 0.5 * kl["window"]


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_bitwise_repeatability(ctx, problem, dtype):
    p = problem
    xs = np.random.default_rng(9).uniform(-2, 2, size=(2, 70)).astype(dtype)
    out = []
    for _handle in range(2):
        dev = _dev(ctx, p["x"].astype(dtype), p["y"].astype(dtype), dtype)
        for _call in range(2):
            dev.build_neighbors(33, p["il"])
            desc, keep = dev.desc(p["dkern"], 33, DIAG, 0.2)
            lml, _ = dev.fit(desc)
            B, F, alpha = dev.factors()
            m, v, c = dev.predict(xs, cov=True)
            out.append(b"".join(a.tobytes() for a in (dev.neighbors(), np.array([lml]), B, F, alpha, m, v, c)))
        dev.free()
    assert len(set(out)) == 1


def test_errors_leave_the_context_healthy(ctx, problem):
    p = problem
    lib = ctx.lib
    k = p["k"]
    good = ns.nearest_table(p["x"], k, p["il"])
    ref = ns.lml(p["kern"], p["x"], p["y"], good, DIAG, 0.2)
    dev = _dev(ctx, p["x"], p["y"], F64)
    desc, keep = dev.desc(p["dkern"], k, DIAG, 0.2)

    def healthy():
        dev.set_neighbors(good)
        v = dev.lml(desc)[0]
        assert abs(v - ref) <= 1e-8 * abs(ref)

    def set_status(tab, kk=None):
        t32 = np.asfortranarray(tab, dtype=np.int32)
        return lib.svgp_nn_set_neighbors(ctx.h, dev.h, tab.shape[1] if kk is None else kk, t32.ctypes.data_as(C.POINTER(C.c_int32)))

    def no_table_no_fit():
        assert dev.neighbors() is None
        assert lib.svgp_nn_factors(ctx.h, dev.h, None, _ffi._ptr(np.zeros(300)), None) == _ffi.INVALID_ARG

    healthy()
    dev.fit(desc)
    for row_, edit in ((100, lambda t: t.__setitem__((100, 3), 100)),          # an entry >= i
                       (57, lambda t: t.__setitem__((57, 4), t[57, 2])),       # a duplicate
                       (200, lambda t: t.__setitem__((200, 0), -1)),           # a -1 before a valid entry
                       (3, lambda t: t.__setitem__((3, 0), -7))):              # neither an index nor -1
        bad = good.copy()
        edit(bad)
        bad[250, 0] = 299   # a later bad row too: the first is named
        assert set_status(bad) == _ffi.INVALID_ARG
        msg = lib.svgp_last_error(ctx.h).decode()
        assert f"row {row_ + 1} " in msg, msg
        no_table_no_fit()
        healthy()
        dev.fit(desc)
    # desc.k that does not give the table's kb
    other, keep2 = dev.desc(p["dkern"], k + 1, DIAG, 0.2)
    lml, info = C.c_double(), _ffi.NNInfo()
    for fn in (lib.svgp_nn_lml, lib.svgp_nn_fit):
        assert fn(ctx.h, dev.h, C.byref(other), C.byref(lml), C.byref(info)) == _ffi.INVALID_ARG
    healthy()
    # kb > 64
    assert lib.svgp_nn_build_neighbors(ctx.h, dev.h, 65, None) == _ffi.UNSUPPORTED
    no_table_no_fit()
    assert set_status(np.full((300, 65), -1, dtype=np.int32)) == _ffi.UNSUPPORTED
    assert lib.svgp_nn_build_neighbors(ctx.h, dev.h, 0, None) == _ffi.INVALID_ARG
    no_table_no_fit()
    healthy()
    # set / build / clear discard the fit
    xs = np.asfortranarray(np.zeros((2, 4)))
    m = np.zeros(4)
    for change in (lambda: dev.set_neighbors(good), lambda: dev.build_neighbors(k, p["il"]), dev.clear_neighbors):
        dev.fit(desc)
        assert lib.svgp_nn_predict(ctx.h, dev.h, _ffi.COLVECS, 4, _ffi._ptr(xs), _ffi._ptr(m), None, None) == _ffi.OK
        change()
        assert lib.svgp_nn_predict(ctx.h, dev.h, _ffi.COLVECS, 4, _ffi._ptr(xs), _ffi._ptr(m), None, None) == _ffi.INVALID_ARG
        assert lib.svgp_nn_factors(ctx.h, dev.h, None, _ffi._ptr(np.zeros(300)), None) == _ffi.INVALID_ARG
    assert dev.neighbors() is None   # cleared: the window again
    assert dev.lml(desc)[0] == _dev_window_lml(ctx, p, desc)
    healthy()
    dev.free()


def _dev_window_lml(ctx, p, desc):
    dev = _dev(ctx, p["x"], p["y"], F64)
    v = dev.lml(desc)[0]
    dev.free()
    return v


def test_create_build_fit_free_returns_device_memory(ctx):
    """30 rounds of create / build / fit / predict / free at n = 4000, k = 16: the free device memory after the last round is that
    after the first"""
    x, y = nr.synth(4000, 2, seed=3)
    xs = x[:, :50].copy()
    kern = _kernel(o.KERNEL_SE, VAR, [0.9, 0.9])
    free, first = [], None
    for it in range(30):
        dev = _dev(ctx, x, y, F64)
        dev.build_neighbors(16, [0.9, 0.9])
        desc, keep = dev.desc(kern, 16, DIAG)
        v = dev.fit(desc)[0]
        dev.predict(xs, cov=True)
        dev.free()
        first = v if first is None else first
        assert v == first
        if it in (0, 29):
            torch.cuda.synchronize()
            free.append(torch.cuda.mem_get_info()[0])
    assert free[1] >= free[0], free
