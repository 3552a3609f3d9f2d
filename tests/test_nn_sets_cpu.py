"""CPU pins of tests/nn_sets_ref.py, the float64 restatement of the NearestNeighbors approximation with the conditioning sets given as
a table that tests/test_gpu_nn_sets.py compares the device against (no GPU): with the window written out as a table it is
tests/nn_ref.py; its gradient at a fixed table matches central differences; the brute-force search obeys the tie and order rules;
and the quality claim the table form exists for."""
import numpy as np
import pytest

import nn_ref as nr
import nn_sets_ref as ns
import svgp_oracle as o
from approxgp import NearestNeighbors

FAMILIES = [o.KERNEL_SE, o.KERNEL_MATERN32, o.KERNEL_MATERN52]


@pytest.mark.parametrize("n,k,d", [(1, 3, 1), (2, 3, 2), (40, 7, 3), (40, 64, 2)])
def test_window_table_is_nn_ref(n, k, d):
    x, y = nr.synth(n, d, seed=n + k)
    kern = nr.kernel_of(o.KERNEL_MATERN52, 1.2, nr.invl_for(d, True))
    tab = ns.window_table(n, k)
    assert tab.shape == (n, min(k, n - 1))
    a, b = nr.fit(kern, x, y, k, 1e-2, mean_const=0.2), ns.fit(kern, x, y, tab, 1e-2, mean_const=0.2)
    for key in ("B", "F", "alpha"):
        assert np.array_equal(a[key], b[key]), key
    assert a["lml"] == b["lml"]
    assert np.array_equal(ns.table_factors(b["B"], tab)[min(k, n - 1):], nr.banded(a["B"], k)[min(k, n - 1):])   # past the ramp-up the two layouts coincide
    ga, gb = nr.lml_grad(kern, x, y, k, 1e-2, 0.2), ns.lml_grad(kern, x, y, tab, 1e-2, 0.2)
    for u, v in zip(ga, gb):   # the same float64 formulas over a gathered copy of the points: einsum may add in another order
        np.testing.assert_allclose(u, v, rtol=1e-12, atol=0)
    xs = np.random.default_rng(1).uniform(-2, 2, size=(d, 9))
    for u, v in zip(nr.predict(a, kern, x, xs, xs[:, :4]), ns.predict(b, kern, x, xs, xs[:, :4])):
        assert np.array_equal(u, v)


@pytest.mark.parametrize("family", FAMILIES)
def test_gradient_against_central_differences_at_a_fixed_table(family):
    n, d, k = 60, 3, 7
    x, y = nr.synth(n, d, seed=5 + family)
    var, il, diag, mc = 1.2, np.array([0.8, 0.95, 1.1]), 1e-2, 0.2
    tab = ns.nearest_table(x, k, il)
    tab[20, 3:] = -1   # a short row
    assert not np.array_equal(tab, ns.window_table(n, k))
    val, gv, gil, gd = ns.lml_grad(nr.kernel_of(family, var, il), x, y, tab, diag, mc)
    assert abs(val - ns.lml(nr.kernel_of(family, var, il), x, y, tab, diag, mc)) <= 1e-12 * abs(val)
    f = lambda v, l, dg: ns.lml(nr.kernel_of(family, v, l), x, y, tab, dg, mc)
    h = 1e-6
    fd = [(f(var + h, il, diag) - f(var - h, il, diag)) / (2 * h)]
    fd += [(f(var, il + h * e, diag) - f(var, il - h * e, diag)) / (2 * h) for e in np.eye(d)]
    fd += [(f(var, il, diag + h * 1e-2) - f(var, il, diag - h * 1e-2)) / (2 * h * 1e-2)]
    g = np.concatenate([[gv], gil, [gd]])
    np.testing.assert_allclose(g, np.array(fd), rtol=2e-6, atol=1e-6 * np.max(np.abs(g[:-1])))


def test_search_ties_and_order():
    # 1-D lattice with duplicates: distances to x_6 = 2 from [0, 1, 1, 3, 2, 4] are [4, 1, 1, 1, 0, 4]
    x = np.array([0.0, 1.0, 1.0, 3.0, 2.0, 4.0, 2.0])
    tab = ns.nearest_table(x, 3)
    assert list(tab[6]) == [1, 2, 4]            # 0 first, then the tie at 1 goes to the lower indices 1, 2 (not 3); ascending index
    assert list(tab[0]) == [-1, -1, -1] and list(tab[1]) == [0, -1, -1] and list(tab[2]) == [0, 1, -1]
    tab1 = ns.nearest_table(x, 1)
    assert list(tab1[:, 0]) == [-1, 0, 1, 1, 1, 3, 4]   # x_3 = 3: ties between x_1 and x_2 -> 1; x_4 = 2: x_1, x_2, x_3 tie -> 1
    # the metric: with il = (1, 0) only the first coordinate counts
    x2 = np.array([[0.0, 5.0, 1.0], [9.0, 0.0, 0.0]])
    assert ns.nearest_table(x2, 1, [1.0, 0.0])[2, 0] == 0 and ns.nearest_table(x2, 1, [0.0, 1.0])[2, 0] == 1
    for t in (tab, ns.nearest_table(nr.synth(50, 3, seed=2)[0], 7, [0.8, 1.0, 1.3])):
        for i in range(t.shape[0]):
            r = ns.row(t, i)
            assert len(r) == min(i, t.shape[1]) and np.all(np.diff(r) > 0) and np.all(r < i) and np.all(t[i, len(r):] == -1)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_sorted_1d_inputs_give_the_window(dtype):
    x = np.sort(np.random.default_rng(3).uniform(-2, 2, 80)).astype(dtype)
    for k in (1, 5, 64, 100):
        assert np.array_equal(ns.nearest_table(x, k, [0.7], dtype), ns.window_table(80, k))


@pytest.mark.parametrize("family", FAMILIES)
def test_nearest_sets_halve_the_kl_divergence(family):
    """N = 600 uniform points in [-3, 3]^2 in Morton order, k = 10: 2 KL(exact GP || Vecchia) = sum log F_i - log det(K + diag I) of the
    k nearest predecessors is at most half that of the window of the previous k"""
    q = ns.QUALITY
    kern = nr.kernel_of(family, q["variance"], q["inv_lengthscale"])
    for seed in q["seeds"]:
        x = ns.quality_problem(seed)
        ld = ns.logdet_exact(kern, x, q["diag"])
        win = ns.sum_log_f(kern, x, ns.window_table(600, q["k"]), q["diag"]) - ld
        near = ns.sum_log_f(kern, x, ns.nearest_table(x, q["k"], q["inv_lengthscale"]), q["diag"]) - ld
        print(f"family {family} seed {seed}: 2 KL window {win:.2f} nearest {near:.2f} ratio {win / near:.2f}")
        assert near > 0 and win > 0
        assert near <= 0.5 * win


def test_mirror_takes_the_three_forms_of_neighbors():
    assert NearestNeighbors(3).neighbors is None and NearestNeighbors(3, neighbors="nearest").neighbors == "nearest"
    assert NearestNeighbors(3, neighbors=ns.window_table(6, 3)).neighbors.shape == (6, 3)
    for bad in ("window", np.zeros(4, dtype=np.int32), np.zeros((4, 2))):
        with pytest.raises(ValueError):
            NearestNeighbors(3, neighbors=bad)
