"""CPU-side check (no GPU): the sequential Kalman filter / RTS smoother of tests/statespace_ref.py - the conventions of svgp_ss_* (model
matrices, the first update from (0, Pinf), unobserved test points merged behind equal data times) - equals the dense exact GP, and so
do the references the deeper GPU cases lean on: the filter-only lml in float64 and long double, the long double dense factor, the
scan-depth helper and the problems built for a given union size."""
import numpy as np
import pytest

import statespace_ref as R

REGULAR = [(N, "plain") for N in R.SIZES] + [(2 * R.TILE + 1, k) for k in R.KINDS[1:] if k not in R.NOISE]


def seq_and_dense(family, p, dtype=np.float64):
    v, il, dl = p["variance"], p["inv_lengthscale"], p["y"] - p["mean_const"]
    lml_d, mean_d, var_d = (np.asarray(a, dtype=np.float64) for a in R.dense(family, v, il, p["t"], dl, p["sig2"], p["ts"], dtype))
    tm, dm, rm, pos = R.merged(p["t"], dl, p["sig2"], p["ts"])
    assert np.all(np.diff(tm) >= 0) and np.array_equal(tm[pos], p["ts"]) and (rm >= 0).sum() == p["t"].shape[0]
    lml_s, mean_s, var_s = R.kalman(family, v, il, tm, dm, rm)
    return (lml_s, mean_s[pos], var_s[pos]), (lml_d, mean_d, var_d)


@pytest.mark.parametrize("family", [1, 2])
@pytest.mark.parametrize("N,kind", REGULAR)
def test_sequential_filter_equals_the_dense_gp(family, N, kind):
    p = R.problem(N, kind)
    v, il, dl = p["variance"], p["inv_lengthscale"], p["y"] - p["mean_const"]
    (lml_s, mean_s, var_s), (lml_d, mean_d, var_d) = seq_and_dense(family, p)
    # fp64 round-off of two different algorithms over <= 129 points: measured <= 4e-13 (profiles/statespace/accuracy.md)
    assert abs(lml_s - lml_d) <= 1e-11 * abs(lml_d)
    np.testing.assert_allclose(mean_s, mean_d, rtol=0, atol=1e-11 * v)
    np.testing.assert_allclose(var_s, var_d, rtol=0, atol=1e-11 * v)
    # the lml does not depend on the unobserved points
    assert abs(R.kalman(family, v, il, p["t"], dl, np.broadcast_to(p["sig2"], p["t"].shape))[0] - lml_s) <= 1e-11 * abs(lml_d)


@pytest.mark.parametrize("family", [1, 2])
@pytest.mark.parametrize("kind", sorted(R.NOISE))
def test_noise_regimes_against_the_long_double_dense_gp(family, kind):
    """quiet: K + 2^-20 I has a condition number up to 129 * 1.25 * 2^20 = 1.7e8, and a float64 Cholesky factor is itself 1.2e-8 off in
    the mean (measured); the long double factor is the reference, and the sequential float64 filter stays inside the fp64 contract."""
    p = R.problem(2 * R.TILE + 1, kind)
    seq, ref = seq_and_dense(family, p, R.DENSE_DTYPE[kind])
    # quiet: 10 x the measured 1.42e-11 (lml), 1.77e-10 (mean), 2.36e-13 (var) - the GPU tests' values for this group; loud: as regular
    bounds = (1.5e-10, 1.8e-9, 2.4e-12) if kind == "quiet" else (1e-11, 1e-11, 1e-11)
    errs = (abs(seq[0] - ref[0]) / abs(ref[0]),) + tuple(np.abs(a - b).max() / p["variance"] for a, b in zip(seq[1:], ref[1:]))
    print(f"sequential vs long double dense, {kind} family={family}: lml {errs[0]:.2e} mean {errs[1]:.2e} var {errs[2]:.2e}")
    assert all(e <= b for e, b in zip(errs, bounds))


@pytest.mark.parametrize("family", [1, 2])
def test_spread_of_the_sequential_smoother_over_equal_test_times(family):
    """What the GPU test's bound on the 70 equal test times (10 x R.RUN_SPREAD) is derived from"""
    mean, var = R.run_spread(family)
    print(f"sequential spread over 70 equal test times, family={family}: mean {mean:.2e} var {var:.2e}")
    assert 0.0 <= mean <= R.RUN_SPREAD and 0.0 <= var <= R.RUN_SPREAD


@pytest.mark.parametrize("family", [1, 2])
def test_long_double_dense_gp_equals_the_float64_one(family):
    p = R.problem(2 * R.TILE + 1)
    a = seq_and_dense(family, p)[1]
    b = seq_and_dense(family, p, np.longdouble)[1]
    assert abs(a[0] - b[0]) <= 1e-13 * abs(b[0])
    for x, y in zip(a[1:], b[1:]):
        np.testing.assert_allclose(x, y, rtol=0, atol=1e-13 * p["variance"])   # measured 4e-15: cond(K + I / 8) ~ 1e3


@pytest.mark.parametrize("family", [1, 2])
def test_filter_lml_equals_the_dense_gp(family):
    p = R.problem(R.RECURSIVE_N)
    v, il, dl = p["variance"], p["inv_lengthscale"], p["y"] - p["mean_const"]
    lml_d = R.dense(family, v, il, p["t"], dl, p["sig2"], p["ts"][:1])[0]
    r = np.broadcast_to(p["sig2"], p["t"].shape)
    l64, l80 = R.filter_lml(family, v, il, p["t"], dl, r), R.filter_lml(family, v, il, p["t"], dl, r, dtype=np.longdouble)
    assert l64.dtype == np.float64 and l80.dtype == np.longdouble
    print(f"filter_lml family={family} N={R.RECURSIVE_N}: float64 {abs(l64 - lml_d) / abs(lml_d):.2e} long double {float(abs(l80 - lml_d) / abs(lml_d)):.2e}")
    # the regular group's lml tolerance is 10 x the sequential filter's distance to the dense GP at this N (5.57e-15)
    assert abs(l64 - lml_d) <= 5.6e-14 * abs(lml_d) and abs(l80 - lml_d) <= 5.6e-14 * abs(lml_d)
    assert l64 == R.kalman(family, v, il, p["t"], dl, r)[0]              # the same operations as kalman()'s filter
    # unobserved points are skipped
    tm, dm, rm, _ = R.merged(p["t"], dl, p["sig2"], p["ts"])
    assert abs(R.filter_lml(family, v, il, tm, dm, rm) - l64) <= 1e-13 * abs(l64)


def test_scan_levels():
    T = R.TILE
    sizes = {1: 1, T: 1, T + 1: 2, T * T: 2, T * T + 1: 3, R.RECURSIVE_N: 3, T ** 3: 3, T ** 3 + 1: 4, R.DEEP_N: 4, T ** 4: 4, T ** 4 + 1: 5}
    assert {n: R.scan_levels(n) for n in sizes} == sizes
    assert R.DEEP_U == T ** 3 and -(-R.DEEP_N // T) == T * T + 2


def test_problem_builders():
    f32_exact = lambda a: np.array_equal(np.asarray(a, dtype=np.float32).astype(np.float64), a)
    for U in (R.TILE, R.TILE + 1, 2 * R.TILE, R.TILE ** 2, R.TILE ** 2 + 1, R.DEEP_U, R.DEEP_U + 1):
        p = R.union_problem(U)
        assert p["t"].shape[0] + p["ts"].shape[0] == U and f32_exact(p["ts"]) and np.all(np.diff(p["ts"]) >= 0)
        assert p["ts"][0] == -2.0 and (p["ts"] > p["t"][-1]).any()
    assert np.isin(R.union_problem(R.DEEP_U)["t"], R.union_problem(R.DEEP_U)["ts"]).all()
    for name in R.LAYOUTS:
        p = R.layout_problem(name)
        assert f32_exact(p["ts"]) and np.all(np.diff(p["ts"]) >= 0)
    p = R.deep_problem()
    assert p["t"].shape[0] == R.DEEP_N and f32_exact(p["t"]) and f32_exact(p["ts"]) and f32_exact(p["y"]) and 90 <= p["ts"].shape[0] <= 110
    assert abs(np.diff(p["t"]).mean() * 64.0 - 1.0) < 1e-2       # 64 points per lengthscale: the regular regime, not `long`
    q = R.problem(2 * R.TILE + 1, "quiet")
    assert q["sig2"] == q["diag"] == 2.0 ** -20 and R.problem(2 * R.TILE + 1, "loud")["sig2"] == 2.0 ** 10
