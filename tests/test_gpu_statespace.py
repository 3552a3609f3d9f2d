"""GPU tests of the exact one-dimensional Matern GP in O(N) (svgp_ss_*, approxgp.StateSpace): the parallel-scan Kalman filter and RTS
smoother against the dense float64 exact GP of tests/statespace_ref.py.  Tolerances (profiles/statespace/accuracy.md), all below the fp64
contract of 1e-8: regular / long - 10 x the larger of the device's and the sequential float64 reference's measured distance to the
dense GP; every later group - 10 x the sequential float64 reference's distance to its better reference alone (the dense GP; for the
4-level fit the same filter in long double), never below the regular group's values."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import approxgp
import statespace_ref as R
from approxgp import _ffi
from approxgp.statespace import DeviceStateSpace

pytestmark = pytest.mark.gpu

# (relative for the lml, in units of the prior variance for the moments) per group of cases; float32 handles round the moments once more.
# edges: unions and layouts around the tile and block boundaries; regime: quiet / loud; deep: 3 full and 4 levels in predict - its lml
# is that of the 129-point fit and keeps the regular value; deep_fit: its moments are checked against the sequential smoother itself (no
# better reference exists at that size, so nothing is derived: the regular floor)
LML_RTOL = {"regular": 5.6e-14, "long": 1.4e-12, "edges": 1.9e-13, "regime": 1.5e-10, "deep": 5.6e-14, "deep_fit": 1.9e-13}
MEAN_ATOL = {"regular": 7.6e-13, "long": 2.8e-12, "edges": 7.6e-13, "regime": 1.8e-9, "deep": 7.5e-12, "deep_fit": 7.6e-13}
VAR_ATOL = {"regular": 1.7e-13, "long": 4.2e-14, "edges": 2.5e-13, "regime": 2.4e-12, "deep": 2.0e-11, "deep_fit": 1.7e-13}
F32_EPS = 2.0 ** -24
GROUP = {"long": "long", "quiet": "regime", "loud": "regime"}

BLOCK_N = (256, 257)                                        # the lml kernel's 256-thread workgroups: one, two
CASES = [(N, "plain") for N in R.SIZES + BLOCK_N + (R.RECURSIVE_N,)] + [(2 * R.TILE + 1, k) for k in R.KINDS[1:]]
BOTH = [np.float64, np.float32]


@pytest.fixture(scope="module")
def ctx():
    c = _ffi.Context(0)
    yield c
    c.close()


def dense_of(family, p, ts=None, dtype=np.float64):
    out = R.dense(family, p["variance"], p["inv_lengthscale"], p["t"], p["y"] - p["mean_const"], p["sig2"], p["ts"] if ts is None else ts, dtype)
    return tuple(np.asarray(a, dtype=np.float64) for a in out)


@functools.lru_cache(maxsize=None)
def reference(family, N, kind):
    p = R.problem(N, kind)
    return p, dense_of(family, p, dtype=R.DENSE_DTYPE.get(kind, np.float64))


@functools.lru_cache(maxsize=None)
def named_reference(family, maker, arg):
    """(problem, dense GP) of R.union_problem(U) / R.layout_problem(name)"""
    p = getattr(R, maker)(arg)
    return p, dense_of(family, p)


@functools.lru_cache(maxsize=None)
def deep_fit_reference(family):
    """-> (problem, lml by the sequential float64 filter, (mean, var) at the test times by the sequential smoother over the union)"""
    p = R.deep_problem()
    v, il, dl = p["variance"], p["inv_lengthscale"], p["y"] - p["mean_const"]
    lml = R.filter_lml(family, v, il, p["t"], dl, np.broadcast_to(p["sig2"], p["t"].shape))
    tm, dm, rm, pos = R.merged(p["t"], dl, p["sig2"], p["ts"])
    _, mean, var = R.kalman(family, v, il, tm, dm, rm)
    return p, float(lml), mean[pos], var[pos]


def kernel_of(family, p):
    base = approxgp.Matern32Kernel() if family == 1 else approxgp.Matern52Kernel()
    return p["variance"] * approxgp.with_lengthscale(base, 1.0 / p["inv_lengthscale"])


def desc_of(dev, family, p):
    return dev.desc(kernel_of(family, p), p["diag"], p["mean_const"])


def run(ctx, family, dtype, p):
    dev = DeviceStateSpace(ctx, p["t"], p["y"], dtype)
    try:
        if np.ndim(p["sig2"]):
            dev.set_noise(p["sig2"] - p["diag"])
        desc = desc_of(dev, family, p)
        out = []
        for _ in range(2):
            lml, info = dev.fit(desc)
            out.append((lml,) + dev.predict(p["ts"]))
        return out, info
    finally:
        dev.free()


def check(label, p, ref, got, dtype, group):
    """Prints and bounds the distance of got = (lml, mean, var) to ref (the latent mean without the prior mean)"""
    (lml_d, mean_d, var_d), (lml, mean, var), v = ref, got, p["variance"]
    e_lml = abs(lml - lml_d) / abs(lml_d)
    e_mean = np.abs(mean - p["mean_const"] - mean_d).max() / v
    e_var = np.abs(var - var_d).max() / v
    print(f"ss accuracy {label} {np.dtype(dtype).name}: lml {e_lml:.2e} mean {e_mean:.2e} var {e_var:.2e}")
    r32 = F32_EPS * (np.abs(mean_d).max() + abs(p["mean_const"]) + v) / v if dtype == np.float32 else 0.0
    assert e_lml <= LML_RTOL[group]
    assert e_mean <= MEAN_ATOL[group] + r32 and e_var <= VAR_ATOL[group] + r32
    assert mean.dtype == dtype and var.dtype == dtype and mean.shape == var.shape == mean_d.shape


def same_bits(a, b):
    return all((x is None and y is None) or np.array_equal(x, y) for x, y in zip(a, b))


def fresh(ctx, family, dtype, p, noise=None, delta=None, with_y=True):
    """(lml, mean, var) of one fit and one predict on a handle that has seen nothing else: what a used handle must return bit for bit"""
    dev = DeviceStateSpace(ctx, p["t"], p["y"] if with_y else None, dtype)
    try:
        if noise is not None:
            dev.set_noise(noise)
        return (dev.fit(desc_of(dev, family, p), delta=delta)[0],) + dev.predict(p["ts"])
    finally:
        dev.free()


@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("family", [1, 2])
@pytest.mark.parametrize("N,kind", CASES)
def test_lml_and_marginals_match_the_dense_gp(ctx, family, dtype, N, kind):
    p, ref = reference(family, N, kind)
    (first, second), info = run(ctx, family, dtype, p)
    assert info.state_dim == family + 1 and info.n_tiles == -(-N // R.TILE) and info.levels == R.scan_levels(N)
    check(f"family={family} N={N} {kind}", p, ref, first, dtype, GROUP.get(kind, "regular"))
    # a repeated call returns the same bits
    assert second[0] == first[0] and same_bits(second[1:], first[1:])


@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("family", [1, 2])
@pytest.mark.parametrize("U", [R.TILE, R.TILE + 1, 2 * R.TILE, R.TILE ** 2, R.TILE ** 2 + 1])
def test_union_sizes_at_the_tile_edges(ctx, family, dtype, U):
    """The union of data and test points fills its last tile exactly / starts a new one with a single point, at levels 1 and 2 (the
    smoother runs from the last point: its partial tile holds the first points)"""
    p, ref = named_reference(family, "union_problem", U)
    assert p["t"].shape[0] + p["ts"].shape[0] == U
    (first, second), _ = run(ctx, family, dtype, p)
    check(f"family={family} U={U}", p, ref, first, dtype, "edges")
    assert second[0] == first[0] and same_bits(second[1:], first[1:])


@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("family", [1, 2])
@pytest.mark.parametrize("layout", R.LAYOUTS)
def test_test_time_layouts(ctx, family, dtype, layout):
    p, ref = named_reference(family, "layout_problem", layout)
    (first, second), _ = run(ctx, family, dtype, p)
    check(f"family={family} {layout}", p, ref, first, dtype, "edges")
    assert second[0] == first[0] and same_bits(second[1:], first[1:])
    if layout == "run":
        # 70 unobserved points at one time stamp, over a tile boundary: one result, 70 times.  Not bit for bit: the smoother's gain
        # P (A P A' + Q)^-1 at dt = 0 is the identity only up to the rounding of its solve, in the sequential float64 smoother too,
        # whose 70 variances spread over 3.83e-16 of the prior variance (R.run_spread, pinned by the CPU test at R.RUN_SPREAD; means:
        # 0).  10 x that, plus an ulp for a float32 handle
        v = p["variance"]
        spread = max(np.ptp(first[1].astype(np.float64)), np.ptp(first[2].astype(np.float64))) / v
        print(f"ss run of {p['ts'].shape[0]} equal times family={family} {np.dtype(dtype).name}: spread {spread:.2e}")
        r32 = 2.0 * F32_EPS * (np.abs(ref[1]).max() + abs(p["mean_const"]) + v) / v if dtype == np.float32 else 0.0
        assert p["ts"].shape[0] > R.TILE and spread <= 10.0 * R.RUN_SPREAD + r32


@pytest.mark.parametrize("U,levels,dtype", [(R.DEEP_U, 3, np.float64), (R.DEEP_U + 1, 4, np.float64), (R.DEEP_U + 1, 4, np.float32)])
@pytest.mark.parametrize("family", [1, 2])
def test_four_level_predict_matches_the_dense_gp(ctx, family, U, levels, dtype):
    """129 data points and test times (a uniform grid and every data time) that fill 3 levels exactly / need a 4th: unobserved points
    change no marginal, so the dense GP of the 129 points checks every one of the 64^3 - 129 (+ 1) results"""
    assert R.scan_levels(U) == levels and R.scan_levels(U - 1) == 3
    p, ref = named_reference(family, "union_problem", U)
    N, n = p["t"].shape[0], p["ts"].shape[0]
    assert N + n == U and np.isin(p["t"], p["ts"]).all()
    dev = DeviceStateSpace(ctx, p["t"], p["y"], dtype)
    try:
        lml, info = dev.fit(desc_of(dev, family, p))
        assert info.n_tiles == -(-N // R.TILE) and info.levels == R.scan_levels(N)   # the library's tile is the helper's
        mean, var = dev.predict(p["ts"])
    finally:
        dev.free()
    check(f"family={family} U={U} deep", p, ref, (lml, mean, var), dtype, "deep")


@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("family", [1, 2])
def test_four_level_fit_matches_the_sequential_filter(ctx, family, dtype):
    """64^3 + 64 + 1 observed points: the aggregates' scan recurses, and the lml kernel's workgroups stride over the points a second
    time.  No dense GP at this size: the lml against the sequential float64 filter (its long double run differs by 1.8e-14), the
    marginals at ~100 test times against the sequential smoother over the union."""
    p, lml_s, mean_s, var_s = deep_fit_reference(family)
    N = p["t"].shape[0]
    assert N == R.DEEP_N and R.scan_levels(N + p["ts"].shape[0]) == 4
    dev = DeviceStateSpace(ctx, p["t"], p["y"], dtype)
    try:
        lml, info = dev.fit(desc_of(dev, family, p))
        assert info.levels == 4 and info.n_tiles == 4098
        mean, var = dev.predict(p["ts"])
    finally:
        dev.free()
    check(f"family={family} N={N} deep fit", p, (lml_s, mean_s, var_s), (lml, mean, var), dtype, "deep_fit")


def c_fit(ctx, dev, desc, delta=None):
    lml = C.c_double(0.0)
    rc = ctx.lib.svgp_ss_fit(ctx.h, dev.h, C.byref(desc), None if delta is None else delta.ctypes.data_as(C.POINTER(C.c_double)), C.byref(lml), None)
    return rc, lml.value


def c_predict(ctx, dev, dtype):
    ts, m = np.array([0.25, 0.5], dtype=dtype), np.zeros(2, dtype=dtype)
    return ctx.lib.svgp_ss_predict(ctx.h, dev.h, 2, _ffi._ptr(ts), _ffi._ptr(m), None)


@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("family", [1, 2])
@pytest.mark.parametrize("s_bad", [-0.125, -0.5])
def test_a_noise_variance_that_is_not_positive(ctx, family, dtype, s_bad):
    p, ref = reference(family, 2 * R.TILE + 1, "plain")
    dev = DeviceStateSpace(ctx, p["t"], p["y"], dtype)
    try:
        desc = desc_of(dev, family, p)
        dev.fit(desc)
        s = np.zeros(p["t"].shape[0])
        s[100] = s_bad                                        # diag + s_i = 0 / < 0 at one point of the second tile
        dev.set_noise(s)
        rc, lml = c_fit(ctx, dev, desc)
        assert rc == _ffi.NOT_POSDEF and math.isnan(lml)
        with pytest.raises(_ffi.PosDefException):
            dev.fit(desc)
        assert c_predict(ctx, dev, dtype) == _ffi.INVALID_ARG
        dev.set_noise(None)
        got = (dev.fit(desc)[0],) + dev.predict(p["ts"])
    finally:
        dev.free()
    check(f"family={family} after s_i={s_bad}", p, ref, got, dtype, "regular")
    assert same_bits(got, fresh(ctx, family, dtype, p))      # nothing of the failed fit or of its noise is left


@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("family", [1, 2])
def test_set_noise_invalidates_the_fit(ctx, family, dtype):
    p, ref = reference(family, 2 * R.TILE + 1, "noise")
    plain = dict(p, sig2=p["diag"])
    dev = DeviceStateSpace(ctx, p["t"], p["y"], dtype)
    try:
        desc = desc_of(dev, family, p)
        dev.fit(desc)
        assert c_predict(ctx, dev, dtype) == _ffi.OK
        dev.set_noise(p["sig2"] - p["diag"])
        assert c_predict(ctx, dev, dtype) == _ffi.INVALID_ARG
        noisy = (dev.fit(desc)[0],) + dev.predict(p["ts"])
        dev.set_noise(None)
        assert c_predict(ctx, dev, dtype) == _ffi.INVALID_ARG
        removed = (dev.fit(desc)[0],) + dev.predict(p["ts"])
    finally:
        dev.free()
    check(f"family={family} noise set", p, ref, noisy, dtype, "regular")
    check(f"family={family} noise removed", plain, dense_of(family, plain), removed, dtype, "regular")
    assert same_bits(noisy, fresh(ctx, family, dtype, p, noise=p["sig2"] - p["diag"])) and same_bits(removed, fresh(ctx, family, dtype, plain))


@pytest.mark.parametrize("dtype", BOTH)
@pytest.mark.parametrize("family", [1, 2])
def test_data_without_y_need_a_delta(ctx, family, dtype):
    p, ref = reference(family, 2 * R.TILE + 1, "plain")
    dev = DeviceStateSpace(ctx, p["t"], None, dtype)
    try:
        desc = desc_of(dev, family, p)
        assert c_fit(ctx, dev, desc)[0] == _ffi.INVALID_ARG
        assert c_predict(ctx, dev, dtype) == _ffi.INVALID_ARG
        delta = p["y"] - p["mean_const"]
        got = (dev.fit(desc, delta=delta)[0],) + dev.predict(p["ts"])
    finally:
        dev.free()
    check(f"family={family} delta", p, ref, got, dtype, "regular")
    assert same_bits(got, fresh(ctx, family, dtype, p, delta=delta, with_y=False))
    assert same_bits(got, fresh(ctx, family, dtype, p))          # y exact in the data dtype: y - mean_const on the device is delta


SEQ_N, SEQ_BIG = 2 * R.TILE + 1, 5000
OTHER = dict(variance=2.0, inv_lengthscale=2.0, mean_const=-0.25, sig2=0.25, diag=0.25)


@functools.lru_cache(maxsize=None)
def sequence_reference(family):
    """-> (problem, its dense GP) of the handle test's two parameter sets: family 2 at SEQ_BIG grid times, family 1 (OTHER) at 3"""
    p = R.problem(SEQ_N)
    p = dict(p, ts=R.grid_times(SEQ_BIG)) if family == 2 else dict(p, **OTHER, ts=np.array([-1.0, p["t"][64], 11.0]))
    return p, dense_of(family, p)


@pytest.mark.parametrize("dtype", BOTH)
def test_one_handle_through_changing_sizes_and_families(ctx, dtype):
    """fm, work, out and slot are reused with another leading dimension and another element size (12 / 27 doubles in the filter, 8 / 18
    in the smoother): every result is the dense GP's, and bit for bit that of the same call on a fresh handle"""
    (pa, ref_a), (pb, ref_b) = sequence_reference(2), sequence_reference(1)
    assert SEQ_N + SEQ_BIG > R.TILE ** 2

    dev = DeviceStateSpace(ctx, pa["t"], pa["y"], dtype)
    try:
        a1 = (dev.fit(desc_of(dev, 2, pa))[0],) + dev.predict(pa["ts"])
        b = (dev.fit(desc_of(dev, 1, pb))[0],) + dev.predict(pb["ts"])
        mean_only, var_only = dev.predict(pb["ts"], var=False), dev.predict(pb["ts"], mean=False)
        a2 = (dev.fit(desc_of(dev, 2, pa))[0],) + dev.predict(pa["ts"])
    finally:
        dev.free()
    check("handle: family=2 n=5000", pa, ref_a, a1, dtype, "regular")
    check("handle: family=1 n=3", pb, ref_b, b, dtype, "regular")
    assert mean_only[1] is None and var_only[0] is None
    assert np.array_equal(mean_only[0], b[1]) and np.array_equal(var_only[1], b[2])
    assert same_bits(a2, a1) and same_bits(a1, fresh(ctx, 2, dtype, pa)) and same_bits(b, fresh(ctx, 1, dtype, pb))


def test_unsorted_inputs_come_back_in_the_callers_order(ctx):
    p, (lml_d, mean_d, var_d) = reference(2, 2 * R.TILE + 1, "noise")
    rng = np.random.default_rng(1)
    pd, pt = rng.permutation(p["t"].shape[0]), rng.permutation(p["ts"].shape[0])
    f = approxgp.GP(p["mean_const"], kernel_of(2, p))
    fx = f(p["t"][pd], approxgp.Diagonal(p["sig2"][pd]))
    assert abs(approxgp.approx_lml(approxgp.StateSpace(), fx, p["y"][pd], ctx=ctx) - lml_d) <= LML_RTOL["regular"] * abs(lml_d)
    post = approxgp.posterior(approxgp.StateSpace(), fx, p["y"][pd], ctx=ctx)
    try:
        m, v = post.mean_and_var(p["ts"][pt])
        np.testing.assert_allclose(m - p["mean_const"], mean_d[pt], rtol=0, atol=MEAN_ATOL["regular"] * p["variance"])
        np.testing.assert_allclose(v, var_d[pt], rtol=0, atol=VAR_ATOL["regular"] * p["variance"])
        ym, yv = post.predict_y(p["ts"][pt], noise=0.25)
        np.testing.assert_allclose(yv, v + 0.25, rtol=1e-14)
        lpd = post.log_predictive_density(p["ts"][pt], np.zeros(pt.shape[0]), noise=0.25)
        np.testing.assert_allclose(lpd, -0.5 * (np.log(2 * np.pi * yv) + ym ** 2 / yv), rtol=1e-12)
    finally:
        post.free()
    # any other prior mean, as offsets: the same lml as the dense GP of y - offsets
    off = 0.1 * p["t"]
    lml_o = approxgp.approx_lml(approxgp.StateSpace(), fx, p["y"][pd], ctx=ctx, mean_offsets=off[pd])
    ref_o = R.dense(2, p["variance"], p["inv_lengthscale"], p["t"], p["y"] - p["mean_const"] - off, p["sig2"], p["ts"][:1])[0]
    assert abs(lml_o - ref_o) <= LML_RTOL["regular"] * abs(ref_o)


def test_status_codes(ctx):
    lib, t = ctx.lib, np.linspace(0.0, 1.0, 9)
    h = C.c_void_p()
    d2 = _ffi.DeviceData(ctx, np.zeros((2, 9)), np.zeros(9), np.float64)
    assert lib.svgp_ss_create(ctx.h, d2.h, C.byref(h)) == _ffi.UNSUPPORTED          # d = 2
    d2.free()
    du = _ffi.DeviceData(ctx, t[::-1].copy(), np.zeros(9), np.float64, _ffi.VEC)
    assert lib.svgp_ss_create(ctx.h, du.h, C.byref(h)) == _ffi.INVALID_ARG           # unsorted at the C level
    du.free()
    dev = DeviceStateSpace(ctx, t, np.zeros(9), np.float64)
    try:
        lml = C.c_double()
        fit = lambda ds: lib.svgp_ss_fit(ctx.h, dev.h, C.byref(ds), None, C.byref(lml), None)
        assert fit(dev.desc(approxgp.SqExponentialKernel(), 0.1)) == _ffi.UNSUPPORTED   # SE has no finite state
        assert fit(dev.desc(approxgp.Matern32Kernel(), 0.0)) == _ffi.INVALID_ARG        # diag = 0
        m = np.zeros(2)
        assert lib.svgp_ss_predict(ctx.h, dev.h, 2, _ffi._ptr(np.array([0.1, 0.2])), _ffi._ptr(m), None) == _ffi.INVALID_ARG   # no fit yet
        assert fit(dev.desc(approxgp.Matern32Kernel(), 0.1)) == _ffi.OK
        assert lib.svgp_ss_predict(ctx.h, dev.h, 2, _ffi._ptr(np.array([0.2, 0.1])), _ffi._ptr(m), None) == _ffi.INVALID_ARG   # unsorted test times
    finally:
        dev.free()
