"""CPU-side check (no GPU): the sequential Kalman filter / RTS smoother of tests/statespace_ref.py - the conventions of svgp_ss_* (model
matrices, the first update from (0, Pinf), unobserved test points merged behind equal data times) - equals the dense exact GP."""
import numpy as np
import pytest

import statespace_ref as R


@pytest.mark.parametrize("family", [1, 2])
@pytest.mark.parametrize("N,kind", [(N, "plain") for N in R.SIZES] + [(2 * R.TILE + 1, k) for k in R.KINDS[1:]])
def test_sequential_filter_equals_the_dense_gp(family, N, kind):
    p = R.problem(N, kind)
    v, il, dl = p["variance"], p["inv_lengthscale"], p["y"] - p["mean_const"]
    lml_d, mean_d, var_d = R.dense(family, v, il, p["t"], dl, p["sig2"], p["ts"])
    tm, dm, rm, pos = R.merged(p["t"], dl, p["sig2"], p["ts"])
    assert np.all(np.diff(tm) >= 0) and np.array_equal(tm[pos], p["ts"]) and (rm >= 0).sum() == N
    lml_s, mean_s, var_s = R.kalman(family, v, il, tm, dm, rm)
    # fp64 round-off of two different algorithms over <= 129 points: measured <= 4e-13 (profiles/statespace/accuracy.md)
    assert abs(lml_s - lml_d) <= 1e-11 * abs(lml_d)
    np.testing.assert_allclose(mean_s[pos], mean_d, rtol=0, atol=1e-11 * v)
    np.testing.assert_allclose(var_s[pos], var_d, rtol=0, atol=1e-11 * v)
    # the lml does not depend on the unobserved points
    assert abs(R.kalman(family, v, il, p["t"], dl, np.broadcast_to(p["sig2"], p["t"].shape))[0] - lml_s) <= 1e-11 * abs(lml_d)
