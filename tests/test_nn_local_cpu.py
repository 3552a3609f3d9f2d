"""CPU pins of tests/nn_local_ref.py, the float64 restatement of the local (nearest-neighbour kriging) predictions that
tests/test_gpu_nn_local.py compares the device against (no GPU): with every training point in the conditioning set it is the exact GP;
its variance is bounded below by the exact GP's and does not grow with k; the search obeys the tie, order and not-finite rules; the
quality record of DESIGN 5.6; and the call's surface (header, ctypes table, Julia binding)."""
import os
import re

import numpy as np
import pytest

import nn_local_ref as nl
import nn_ref as nr
import nn_sets_ref as ns
import svgp_oracle as o
from approxgp import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = [o.KERNEL_SE, o.KERNEL_MATERN32, o.KERNEL_MATERN52]


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("diag", [0.0, 1e-2])
@pytest.mark.parametrize("n,k,d", [(1, 1, 1), (17, 64, 3), (64, 64, 8), (40, 100, 5)])
def test_every_point_in_the_set_is_the_exact_gp(family, diag, n, k, d):
    x, y = nr.synth(n, d, seed=31 * n + d)
    var = 1.2
    kern = nr.kernel_of(family, var, nr.invl_for(d, True))
    xs = np.random.default_rng(n).uniform(-2, 2, size=(d, 9))
    tab = nl.query_table(x, xs, k, kern.inv_lengthscale)
    assert tab.shape == (9, n) and np.array_equal(tab, np.tile(np.arange(n, dtype=np.int32), (9, 1)))
    mean, v = nl.predict_local(kern, x, y, xs, tab, diag, mean_const=0.3)
    em, ec = nr.exact_predict(kern, x, y, diag, xs, mean_const=0.3)
    # both sides solve with K + diag I (the same points in the same order) and contract in another order, so they differ by what a
    # solve loses, cond(K) eps: the sizes are chosen with cond(K) <= 1e5 at diag = 0 (d = 8 at N = 64: d = 2 there has cond 1e10 for
    # the SE kernel), where 1e-10 has a factor of four to spare
    cond = np.linalg.cond(o.kernelmatrix(kern, x) + diag * np.eye(n))
    assert cond <= 1e5
    tol = 1e-10
    print(f"family {family} diag {diag} n {n}: cond {cond:.1e} mean err {np.max(np.abs(mean - em)):.1e} var err {np.max(np.abs(v - np.diag(ec))):.1e}")
    assert np.max(np.abs(mean - em)) <= tol * max(np.max(np.abs(em)), 1e-300)
    assert np.max(np.abs(v - np.diag(ec))) <= tol * var


@pytest.fixture(scope="module")
def quality():
    """the 600-point problem of the quality claim (nn_sets_ref.quality_problem, seed 0) with 200 uniform test points; the exact GP's
    predictions per family are computed once"""
    q = ns.QUALITY
    x = ns.quality_problem(0)
    rng = np.random.default_rng(100)
    y = np.sin(x.sum(axis=0)) + np.sqrt(q["diag"]) * rng.standard_normal(600)
    xs = rng.uniform(-3.0, 3.0, size=(2, 200))
    exact = {}
    for fam in FAMILIES:
        kern = nr.kernel_of(fam, q["variance"], q["inv_lengthscale"])
        em, ec = nr.exact_predict(kern, x, y, q["diag"], xs, 0.1)
        exact[fam] = (kern, em, np.diag(ec))
    return dict(x=x, y=y, xs=xs, exact=exact, q=q)


@pytest.mark.parametrize("family", FAMILIES)
def test_variance_ordering(quality, family):
    """conditioning on a subset cannot give less variance than conditioning on everything, and with the deterministic tie rule the
    k nearest are among the k + 1 nearest: var_local does not grow with k"""
    p, q = quality, quality["q"]
    kern, em, ev = p["exact"][family]
    prev = None
    for k in (1, 2, 5, 10, 20, 40):
        tab = nl.query_table(p["x"], p["xs"], k, q["inv_lengthscale"])
        if prev is not None:
            assert all(set(a[a >= 0]) <= set(b) for a, b in zip(prev[0], tab))
        _, v = nl.predict_local(kern, p["x"], p["y"], p["xs"], tab, q["diag"], 0.1)
        assert np.all(v >= ev - 1e-10 * q["variance"]), k
        if prev is not None:
            assert np.all(v <= prev[1] + 1e-10 * q["variance"]), k
        prev = (tab, v)


# RMS difference from the exact GP's (mean, var) over the 200 test points, k = 10, measured on the CPU (float64):
#   family     local               global, window      global, nearest predecessors
#   SE         (0.0644, 0.00610)   (3.13, 4.35)        (2.16, 1.74)
#   Matern-3/2 (0.0346, 0.00415)   (1.98, 2.81)        (0.773, 0.558)
#   Matern-5/2 (0.0459, 0.00465)   (2.27, 3.24)        (1.03, 0.820)
# Local is the closest of the three in every family, by a factor of 20 and more: the global posterior inherits the error of the
# approximate precision U U' through k(x*, x) (K + diag I is ill-conditioned at diag = 0.05), the local one never forms it.
QUALITY_RECORD = {o.KERNEL_SE: (0.0644, 0.00610), o.KERNEL_MATERN32: (0.0346, 0.00415), o.KERNEL_MATERN52: (0.0459, 0.00465)}


@pytest.mark.parametrize("family", FAMILIES)
def test_quality_record(quality, family):
    p, q = quality, quality["q"]
    kern, em, ev = p["exact"][family]
    rms = lambda a, b: float(np.sqrt(np.mean((a - b) ** 2)))
    tab = nl.query_table(p["x"], p["xs"], q["k"], q["inv_lengthscale"])
    m, v = nl.predict_local(kern, p["x"], p["y"], p["xs"], tab, q["diag"], 0.1)
    res = {"local": (rms(m, em), rms(v, ev))}
    for name, t in (("window", ns.window_table(600, q["k"])), ("nearest", ns.nearest_table(p["x"], q["k"], q["inv_lengthscale"]))):
        c = ns.fit(kern, p["x"], p["y"], t, q["diag"], 0.1)
        gm, gv, _ = nr.predict(c, kern, p["x"], p["xs"])
        res[name] = (rms(gm, em), rms(gv, ev))
    print(f"family {family}: " + ", ".join(f"{n_} mean {a:.3g} var {b:.3g}" for n_, (a, b) in res.items()))
    rm, rv = QUALITY_RECORD[family]
    assert res["local"][0] <= 2 * rm and res["local"][1] <= 2 * rv
    for name in ("window", "nearest"):   # measured: local is the closest of the three
        assert res["local"][0] < res[name][0] and res["local"][1] < res[name][1]


def test_search_rules():
    # distances of x* = 2 to [0, 1, 1, 3, 2, 4, 3] are [4, 1, 1, 1, 0, 4, 1]
    x = np.array([0.0, 1.0, 1.0, 3.0, 2.0, 4.0, 3.0])
    assert list(nl.query_table(x, np.array([2.0]), 3)[0]) == [1, 2, 4]       # 0 first, the tie at 1 to the lower indices; ascending
    assert list(nl.query_table(x, np.array([2.0]), 1)[0]) == [4]
    assert list(nl.query_table(x, np.array([2.0]), 9)[0]) == list(range(7))  # k > n is n
    x2 = np.array([[0.0, 5.0, 1.0], [9.0, 0.0, 0.0]])                        # the metric
    assert nl.query_table(x2, np.array([[1.0], [8.0]]), 1, [1.0, 0.0])[0, 0] == 2
    assert nl.query_table(x2, np.array([[1.0], [8.0]]), 1, [0.0, 1.0])[0, 0] == 0
    xn = x.copy()
    xn[4] = np.nan                                                            # a training point that is not finite is never chosen
    assert list(nl.query_table(xn, np.array([2.0]), 7)[0]) == [0, 1, 2, 3, 5, 6, -1]
    t = nl.query_table(x, np.array([2.0, np.nan]), 3)                         # a test point that is not finite: an empty row, NaN out
    assert list(t[1]) == [-1, -1, -1]
    kern = nr.kernel_of(o.KERNEL_SE, 1.0, [1.0])
    m, v = nl.predict_local(kern, x, np.arange(7.0), np.array([2.0, np.nan]), t, 1e-2)
    assert np.isfinite(m[0]) and np.isfinite(v[0]) and np.isnan(m[1]) and np.isnan(v[1])
    for dtype in (np.float64, np.float32):
        xr, xsr = nr.synth(50, 3, seed=2, dtype=dtype)[0], nr.synth(9, 3, seed=3, dtype=dtype)[0]
        tr = nl.query_table(xr, xsr, 7, [0.8, 1.0, 1.3], dtype)
        assert tr.shape == (9, 7) and np.all(np.diff(tr, axis=1) > 0) and tr.min() >= 0 and tr.max() < 50


def _classes(argtypes):
    import ctypes as C
    cmap = {C.c_int32: "i32", C.c_int64: "i64", C.c_double: "f64"}
    return [cmap.get(t, "ptr") for t in argtypes]


def test_surface():
    """the header, the ctypes table and the Julia binding declare svgp_nn_predict_local alike (the lint of tests/test_abi_cpu.py, for
    this one symbol), the library exports it, and the mirror has its methods"""
    import test_abi_cpu as abi
    from approxgp import DeviceNearestNeighbors
    from approxgp.nearest_neighbors import NNPosteriorGP

    protos = abi._header_prototypes()
    want = ("i32", ["ptr", "ptr", "i32", "i64", "ptr", "i32", "ptr", "ptr", "ptr"])
    assert protos["svgp_nn_predict_local"] == want
    res, args = _ffi.SYMBOLS["svgp_nn_predict_local"]
    assert (_classes([res])[0], _classes(args)) == want
    assert hasattr(_ffi.load_library(), "svgp_nn_predict_local") and _ffi.load_library().svgp_version() == 5
    src = open(os.path.join(ROOT, "integration", "julia", "src", "SVGPMI355X.jl")).read()
    calls = [c for c in abi._julia_ccalls(src) if c[0] == "svgp_nn_predict_local"]
    assert len(calls) == 1 and re.search(r"^function predict_local\(", src, flags=re.M)
    _, _, ret, argt, nvals = calls[0]
    assert (abi._jl_class(ret), [abi._jl_class(a) for a in argt]) == want and nvals == len(argt)
    assert callable(DeviceNearestNeighbors.predict_local)
    for name in ("local_mean_and_var", "local_mean", "local_var"):
        assert callable(getattr(NNPosteriorGP, name))
