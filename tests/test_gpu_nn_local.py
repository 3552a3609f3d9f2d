"""GPU checks of the local (nearest-neighbour kriging) predictions of the NearestNeighbors approximation (csrc/nn.hip:
svgp_nn_predict_local - the query search and the gathered predict kernel) against tests/nn_local_ref.py.

Sizes sit at the kernels' seams: the 64-candidate tiles of the search (N = 63 / 64 / 65 / 129), its 16 queries per workgroup (n* = 1,
3, 5 are partial workgroups, 257 = 16 full ones and one query), the four queries per workgroup of the predict kernel, the k buckets
16 / 32 / 64, and the 32768 test points of one round of the host loop.
Tolerances are those of tests/test_gpu_nn.py for predictions: 1e-9 (fp64) of the largest |mean| and of the prior variance; fp32: see
TOL32."""
import numpy as np
import pytest

import nn_local_ref as nl
import nn_ref as nr
import nn_sets_ref as ns
import svgp_oracle as o
from approxgp import GP, DeviceNearestNeighbors, NearestNeighbors, SEKernel, _ffi, posterior
from approxgp.kernels import ARDTransform, Matern32Kernel, Matern52Kernel, ScaledKernel, TransformedKernel

pytestmark = pytest.mark.gpu

F64, F32 = np.float64, np.float32
BASES = {o.KERNEL_SE: SEKernel, o.KERNEL_MATERN32: Matern32Kernel, o.KERNEL_MATERN52: Matern52Kernel}
VAR, DIAG, MC = 1.2, 1e-2, 0.1
CHUNK = 32768   # test points of one round (include/svgp_mi355x.h)
# fp32 predictions against the float64 restatement on the fp32-rounded inputs with the device's own table, as a fraction of the
# largest |mean| / of the prior variance: the project's 1e-4 (tests/test_gpu_nn.py).  At diag = 1e-2 the block has cond(C) up to
# k variance / diag = 7.7e3 at k = 64, where a solve may lose cond(C) eps32 = 4.6e-4; should a case miss 1e-4 for that reason (the
# fp64 device result on the same inputs is the yardstick), the practice of tests/test_gpu_collapsed.py applies: the worst measured
# error goes here and 4 x it is asserted.
TOL32 = (1e-4, 1e-4)


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


def _local(dev, xs, k, layout, neighbors=True):
    """xs (d, n*) -> predict_local in the given layout of the test points"""
    if layout == _ffi.ROWVECS:
        return dev.predict_local(np.asarray(xs).T, k, neighbors=neighbors, layout=_ffi.ROWVECS)
    return dev.predict_local(xs[0] if layout == _ffi.VEC else xs, k, neighbors=neighbors)


def _lattice(n, d, seed):
    """integer coordinates in 0 .. 3 (many exact ties, duplicate points)"""
    return np.random.default_rng(seed).integers(0, 4, size=(d, n)).astype(np.float64)


# ---- the search ------------------------------------------------------------------------------------------------------
SN, SK, SD, SQ = [1, 2, 63, 64, 65, 129, 300], [1, 16, 17, 64], [1, 2, 8, 17], [1, 3, 5, 257]


def _metric(d, which):
    """unit and power-of-two metrics: every distance is exact in both dtypes"""
    return [np.ones(d), np.full(d, 2.0), 2.0 ** -(np.arange(d) % 4)][which % 3]


@pytest.mark.parametrize("n", SN)
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_search_exact_on_a_lattice(ctx, n, dtype):
    layouts = set()
    for a, k in enumerate(SK):
        b = a + SN.index(n)
        d, nq = SD[b % 4], SQ[(b + (dtype == F32)) % 4]
        layout = _ffi.VEC if d == 1 else [_ffi.COLVECS, _ffi.ROWVECS][b % 2]
        layouts.add(layout)
        x = _lattice(n, d, seed=n + k).astype(dtype)
        xs = _lattice(nq, d, seed=1000 + n + k).astype(dtype)
        il = _metric(d, b)
        dev = _dev(ctx, x, np.zeros(n, dtype=dtype), dtype, layout)
        dev.fit(dev.desc(_kernel(o.KERNEL_MATERN32, VAR, il), 1, 1.0, MC)[0])   # the search metric is the fit's; diag 1: duplicates are fine
        m, v, got = _local(dev, xs, k, layout)
        dev.free()
        ref = nl.query_table(x, xs, k, il, dtype)
        assert got.shape == ref.shape == (nq, min(k, n))
        assert np.array_equal(got, ref), (n, k, d, nq, np.argwhere(got != ref)[:5])
        assert np.all(np.isfinite(m)) and np.all(np.isfinite(v))


def test_search_covers_the_three_layouts():
    seen = set()
    for n in SN:
        for a in range(len(SK)):
            b = a + SN.index(n)
            seen.add(_ffi.VEC if SD[b % 4] == 1 else [_ffi.COLVECS, _ffi.ROWVECS][b % 2])
    assert seen == {_ffi.COLVECS, _ffi.ROWVECS, _ffi.VEC}


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_points_that_are_not_finite(ctx, dtype):
    n, d, k = 65, 2, 16
    x = _lattice(n, d, seed=3).astype(dtype)
    x[1, 7] = np.nan            # a training point with a NaN coordinate is never chosen
    xs = _lattice(6, d, seed=4).astype(dtype)
    xs[0, 2] = np.nan           # a test point with one: NaN out, not the prior, and no error
    xs[1, 4] = np.inf
    y = np.random.default_rng(5).standard_normal(n).astype(dtype)
    dev = _dev(ctx, x, y, dtype)
    dev.set_neighbors(np.full((n, 1), -1, dtype=np.int32))   # nobody is conditioned on the NaN point: the fit succeeds
    dev.fit(dev.desc(_kernel(o.KERNEL_SE, VAR, np.ones(d)), 1, 1.0, MC)[0])
    m, v, tab = dev.predict_local(xs, k, neighbors=True)     # returns: SVGP_OK
    dev.free()
    dev = _dev(ctx, x[:, :64], y[:64], dtype)                # k = N = 64, the most there may be, and 63 candidates that are finite
    dev.set_neighbors(np.full((64, 1), -1, dtype=np.int32))
    dev.fit(dev.desc(_kernel(o.KERNEL_SE, VAR, np.ones(d)), 1, 1.0, MC)[0])
    m64, v64, tab64 = dev.predict_local(xs, 64, neighbors=True)
    dev.free()
    assert np.array_equal(tab, nl.query_table(x, xs, k, np.ones(d), dtype)) and not np.any(tab == 7)
    assert np.array_equal(tab64[0], np.r_[np.arange(7), np.arange(8, 64), -1])   # a short row: -1 follows the valid entries
    assert np.array_equal(tab64, nl.query_table(x[:, :64], xs, 64, np.ones(d), dtype))
    bad = np.array([False, False, True, False, True, False])
    for mm, vv, tt in ((m, v, tab), (m64, v64, tab64)):
        assert np.all(np.isnan(mm[bad])) and np.all(np.isnan(vv[bad])) and np.all(tt[bad] == -1)
        assert np.all(np.isfinite(mm[~bad])) and np.all(np.isfinite(vv[~bad]))


# ---- predictions against the restatement --------------------------------------------------------------------------------
PD = [1, 3, 17]


def _predict_cases():
    """28 cases: every (N, k) pair of the search grid once; d, dtype, family and the layout cycle through them.  diag = 0 where the
    block is well conditioned without it (d = 17: random points are far apart; k = 1), else 1e-2"""
    cases = []
    for a, n in enumerate(SN):
        for b, k in enumerate(SK):
            i = a * len(SK) + b
            d = PD[(a + b) % 3]
            layout = _ffi.VEC if d == 1 else [_ffi.COLVECS, _ffi.ROWVECS][(a + i) % 2]
            diag = 0.0 if (d == 17 or k == 1) else DIAG
            cases.append((n, k, d, layout, [F64, F32][(a + b) % 2], (i // 2) % 3, diag))
    assert {(c[4], c[5]) for c in cases} == {(t, f) for t in (F64, F32) for f in range(3)}
    for t in (F64, F32):   # every k bucket in both dtypes
        assert {(min(c[1], c[0]) + 15) // 16 for c in cases if c[4] == t} >= {1, 2, 4}
    assert {c[6] for c in cases} == {0.0, DIAG}
    return cases


def _assert_close(m, v, rm, rv, dtype, what=""):
    tm, tv = (1e-9, 1e-9) if dtype == F64 else TOL32
    em = np.max(np.abs(m - rm)) / max(np.max(np.abs(rm)), 1e-300)
    ev = np.max(np.abs(v - rv)) / VAR
    print(f"{what} {np.dtype(dtype).name}: mean err {em:.3e} (tol {tm:.1e}) var err {ev:.3e} (tol {tv:.1e})")
    assert em <= tm and ev <= tv, (what, em, ev)


@pytest.mark.parametrize("n,k,d,layout,dtype,fam,diag", _predict_cases())
def test_predictions_match_the_restatement(ctx, n, k, d, layout, dtype, fam, diag):
    x, y = nr.synth(n, d, seed=3000 + n + k, dtype=dtype)
    xs = np.random.default_rng(n + k).uniform(-2, 2, size=(d, 7)).astype(dtype)
    il = nr.invl_for(d, True)
    dev = _dev(ctx, x, y, dtype, layout)
    dev.fit(dev.desc(_kernel(fam, VAR, il), 1, diag, MC)[0])
    m, v, tab = _local(dev, xs, k, layout)
    dev.free()
    kq = min(k, n)
    assert tab.shape == (7, kq) and np.all(tab >= 0) and np.all(np.diff(tab, axis=1) > 0)
    eps = np.finfo(dtype).eps
    for q in range(7):   # the device's own table is the kq nearest (up to the rounding of the distances)
        d2 = nl.query_dist2(x, xs, q, il, dtype).astype(F64)
        assert np.max(d2[tab[q]]) <= np.sort(d2)[kq - 1] * (1 + 8 * eps)
    rm, rv = nl.predict_local(nr.kernel_of(fam, VAR, il), x.astype(F64), y.astype(F64), xs.astype(F64), tab, diag, MC)
    _assert_close(m, v, rm, rv, dtype, f"n {n} k {k} d {d} fam {fam} diag {diag}")


# ---- the exact GP ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [17, 64])
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_every_point_in_the_set_is_the_exact_gp(ctx, n, dtype):
    d = 3
    x, y = nr.synth(n, d, seed=40 + n, dtype=dtype)
    xs = np.random.default_rng(n).uniform(-2, 2, size=(d, 9)).astype(dtype)
    il = nr.invl_for(d, True)
    dev = _dev(ctx, x, y, dtype)
    dev.fit(dev.desc(_kernel(o.KERNEL_MATERN52, VAR, il), 63, DIAG, MC)[0])   # N <= 64, k = 63: the window is everything before a point, the exact GP
    gm, gv, _ = dev.predict(xs)
    m, v = dev.predict_local(xs, 64)
    dev.free()
    em, ec = nr.exact_predict(nr.kernel_of(o.KERNEL_MATERN52, VAR, il), x.astype(F64), y.astype(F64), DIAG, xs.astype(F64), MC)
    _assert_close(m, v, em, np.diag(ec), dtype, f"exact n {n}")
    if n == 64:
        _assert_close(m, v, gm.astype(F64), gv.astype(F64), dtype, "svgp_nn_predict at k = 63")


# ---- independence and repeatability -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_independent_repeatable_and_chunked(ctx, dtype):
    n, d, k = 65, 2, 16
    x, y = nr.synth(n, d, seed=9, dtype=dtype)
    dev = _dev(ctx, x, y, dtype)
    dev.fit(dev.desc(_kernel(o.KERNEL_SE, VAR, nr.invl_for(d, True)), 5, DIAG, MC)[0])
    xs = np.random.default_rng(10).uniform(-2, 2, size=(d, CHUNK + 1)).astype(dtype)
    a = dev.predict_local(xs, k, neighbors=True)
    b = dev.predict_local(xs, k, neighbors=True)
    for u, w in zip(a, b):   # two identical calls
        assert np.array_equal(u, w)
    lo, hi = dev.predict_local(xs[:, :CHUNK], k, neighbors=True), dev.predict_local(xs[:, CHUNK:], k, neighbors=True)
    for u, l, h in zip(a, lo, hi):   # across the seam of the rounds
        assert np.array_equal(u, np.concatenate([l, h]))
    for q in (0, 1, 4, 15, 16, CHUNK - 1, CHUNK):   # each alone
        one = dev.predict_local(xs[:, q:q + 1], k, neighbors=True)
        assert one[0][0] == a[0][q] and one[1][0] == a[1][q] and np.array_equal(one[2][0], a[2][q])
    five = dev.predict_local(xs[:, 3:8], k, neighbors=True)
    for u, w in zip(a, five):
        assert np.array_equal(u[3:8], w)
    dev.free()


# ---- statuses ---------------------------------------------------------------------------------------------------------
def test_statuses(ctx):
    n, d = 70, 2
    x, y = nr.synth(n, d, seed=11)
    x[:, 40] = x[:, 12]   # an exactly repeated point
    xs = np.random.default_rng(12).uniform(-2, 2, size=(d, 6))
    xs[:, 3] = x[:, 12] + 1e-3   # its two copies are the nearest two of test point 4 (1-based)
    kern = _kernel(o.KERNEL_MATERN52, VAR, np.array([0.8, 1.1]))
    dev = _dev(ctx, x, y, F64)
    with pytest.raises(ValueError):          # before a fit: SVGP_INVALID_ARG
        dev.predict_local(xs, 5)
    dev.fit(dev.desc(kern, 3, DIAG, MC)[0])
    with pytest.raises(ValueError):          # k = 0
        dev.predict_local(xs, 0)
    with pytest.raises(_ffi.UnsupportedError):   # min(k, N) = 65
        dev.predict_local(xs, 65)
    assert dev.predict_local(xs, 64)[0].shape == (6,)
    dev.build_neighbors(3, np.array([0.8, 1.1]))
    dev.fit(dev.desc(kern, 3, DIAG, MC)[0])
    dev.predict_local(xs, 5)
    dev.clear_neighbors()
    with pytest.raises(ValueError):          # clearing the table discards the fit
        dev.predict_local(xs, 5)
    dev.free()
    # diag = 0 and both copies in a conditioning set: the block is not positive
    tab = ns.window_table(n, 1)
    tab[40, 0] = 39   # (already the window: point 40 is conditioned on 39, not on its copy, so the fit itself is healthy)
    dev = _dev(ctx, x, y, F64)
    dev.fit(dev.desc(kern, 1, 0.0, MC)[0])
    with pytest.raises(_ffi.PosDefException) as ei:
        dev.predict_local(xs, 5)
    e = ei.value
    assert e.info == 4 and "test point 4 " in str(e)
    bad = np.arange(6) == 3
    assert np.all(np.isnan(e.mean[bad])) and np.all(np.isnan(e.var[bad]))
    assert np.all(np.isfinite(e.mean[~bad])) and np.all(np.isfinite(e.var[~bad]))
    t = nl.query_table(x, xs, 5, [0.8, 1.1])
    assert {12, 40} <= set(t[3]) and not any({12, 40} <= set(r) for r in t[~bad])
    rm, rv = nl.predict_local(nr.kernel_of(o.KERNEL_MATERN52, VAR, [0.8, 1.1]), x, y, xs[:, ~bad], t[~bad], 0.0, MC)
    _assert_close(e.mean[~bad], e.var[~bad], rm, rv, F64, "beside a bad test point")
    m, v = dev.predict_local(xs[:, ~bad], 5)   # afterwards a healthy call on the same context and handle
    assert np.array_equal(m, e.mean[~bad]) and np.array_equal(v, e.var[~bad])
    dev.free()


# ---- the handle's cached state -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("table", [False, True], ids=["window", "table"])
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_existing_results_are_undisturbed(ctx, table, dtype):
    n, d, k = 130, 3, 17
    x, y = nr.synth(n, d, seed=13, dtype=dtype)
    il = nr.invl_for(d, True)
    xs = np.random.default_rng(14).uniform(-2, 2, size=(d, 9)).astype(dtype)
    dev = _dev(ctx, x, y, dtype)
    if table:
        dev.build_neighbors(k, il)
    desc, keep = dev.desc(_kernel(o.KERNEL_MATERN32, VAR, il), k, DIAG, MC)

    def state():
        fitted = dev.fit(desc)[0]
        return [dev.lml(desc)[0], *dev.lml_grad(desc)[:4], fitted, *dev.factors(), *dev.predict(xs, cov=True)]

    before = state()
    dev.predict_local(xs, 64, neighbors=True)
    mid = [*dev.factors(), *dev.predict(xs, cov=True)]   # the fit of before the call still serves
    dev.predict_local(xs, 5)
    after = state()
    dev.free()
    for u, w in zip(before, after):
        assert np.array_equal(np.asarray(u), np.asarray(w))
    for u, w in zip(before[6:], mid):
        assert np.array_equal(np.asarray(u), np.asarray(w))


def test_posterior_methods(ctx):
    x, y = nr.synth(200, 2, seed=15)
    xs = np.random.default_rng(16).uniform(-2, 2, size=(2, 11))
    il = np.array([0.8, 1.1])
    f = GP(MC, _kernel(o.KERNEL_SE, VAR, il))
    post = posterior(NearestNeighbors(10, include_noise=True, neighbors="nearest"), f(x, DIAG), y, ctx=ctx)
    m, v = post.local_mean_and_var(xs)
    assert np.array_equal(m, post.local_mean(xs)) and np.array_equal(v, post.local_var(xs))
    m20, v20 = post.local_mean_and_var(xs, k=20)
    assert np.all(v20 <= v + 1e-9 * VAR) and not np.array_equal(m20, m)
    tab = nl.query_table(x, xs, 10, il)
    rm, rv = nl.predict_local(nr.kernel_of(o.KERNEL_SE, VAR, il), x, y, xs, tab, DIAG, MC)
    _assert_close(m, v, rm, rv, F64, "posterior")
    post.dev.free()
