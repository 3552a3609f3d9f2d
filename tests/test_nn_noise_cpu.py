"""CPU checks (no GPU) of the NearestNeighbors approximation with per-point noise variances and prior-mean offsets: the restatement
tests/nn_noise_ref.py against the dense exact GP and against central differences, the two sum identities, and the Python layer's
argument checks.  Inputs: nn_ref.synth data, s = exp(U[log 0.02, log 0.5]), diag = 1e-2, mu a smooth function of x, mean_const 0.1.

Measured on these inputs (N = 40, d = 2, k = 6, a random predecessor table, every family): s_bar against central differences of step
1e-6 at most 2.9e-9 of the largest entry, mean_bar at most 3.8e-9 (what is left is the differences' own rounding, eps |lml| / h ~
1e-8 absolute; the formulas' first check, on other inputs, reached 3.5e-10 and 9.6e-10); the bound below is 1e-8 for both."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import approxgp
import nn_noise_ref as nn
import nn_ref as nr
import nn_sets_ref as ns
import svgp_oracle as o
from approxgp import GP, CustomMean, Diagonal, NearestNeighbors, SEKernel, _ffi, approx_lml, approx_lml_and_gradient, posterior
from approxgp.nearest_neighbors import DeviceNearestNeighbors, NNPosteriorGP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = [o.KERNEL_SE, o.KERNEL_MATERN32, o.KERNEL_MATERN52]
VAR, DIAG, MC = 1.2, 1e-2, 0.1


def _problem(n, d, family, seed=3):
    x, y = nr.synth(n, d, seed=seed)
    kern = nr.kernel_of(family, VAR, nr.invl_for(d, True))
    return kern, x, y, nn.noise_vector(n, seed + 1), nn.mean_vector(x)


@pytest.mark.parametrize("family", FAMILIES)
def test_all_predecessors_is_the_dense_exact_gp(family):
    n = 40
    kern, x, y, s, mu = _problem(n, 2, family)
    ex = nn.exact_lml(kern, x, y, DIAG, s, mu, MC)
    tab = ns.window_table(n, n - 1)
    a = nn.lml(kern, x, y, tab, DIAG, s, mu, MC)
    b = nn.fit(kern, x, y, tab, DIAG, s, mu, MC)["lml"]
    assert abs(a - ex) <= 1e-10 * abs(ex) and abs(b - ex) <= 1e-10 * abs(ex), (a, b, ex)


def test_without_vectors_the_restatement_is_nn_sets_ref():
    kern, x, y, s, mu = _problem(30, 2, o.KERNEL_MATERN32)
    tab = nn.random_table(30, 5, 1)
    a = nn.fit(kern, x, y, tab, DIAG, None, None, MC)
    b = ns.fit(kern, x, y, tab, DIAG, MC)
    assert np.array_equal(a["B"], b["B"]) and np.array_equal(a["F"], b["F"]) and np.array_equal(a["alpha"], b["alpha"])
    ga, gb = nn.lml_grad(kern, x, y, tab, DIAG, None, None, MC), ns.lml_grad(kern, x, y, tab, DIAG, MC)
    assert abs(ga[0] - gb[0]) <= 1e-13 * abs(gb[0]) and abs(ga[1] - gb[1]) <= 1e-11 * abs(gb[1])
    assert np.max(np.abs(ga[2] - gb[2])) <= 1e-11 * np.max(np.abs(gb[2])) and abs(ga[3] - gb[3]) <= 1e-11 * abs(gb[3])
    # s = c with diag = a is diag = a + c
    c = nn.lml(kern, x, y, tab, DIAG, np.full(30, 0.07), None, MC)
    assert abs(c - ns.lml(kern, x, y, tab, DIAG + 0.07, MC)) <= 1e-13 * abs(c)


@pytest.mark.parametrize("family", FAMILIES)
def test_point_gradients_equal_central_differences(family):
    """s_bar and mean_bar against central differences of the restatement's lml, step 1e-6: see the module docstring for the figures"""
    n, k = 40, 6
    kern, x, y, s, mu = _problem(n, 2, family)
    tab = nn.random_table(n, k, 2)
    val, s_bar, mean_bar = nn.point_grads(kern, x, y, tab, DIAG, s, mu, MC)
    assert abs(val - nn.lml(kern, x, y, tab, DIAG, s, mu, MC)) <= 1e-13 * abs(val)
    h = 1e-6
    fs, fm = np.zeros(n), np.zeros(n)
    for j in range(n):
        e = np.zeros(n)
        e[j] = h
        fs[j] = (nn.lml(kern, x, y, tab, DIAG, s + e, mu, MC) - nn.lml(kern, x, y, tab, DIAG, s - e, mu, MC)) / (2 * h)
        fm[j] = (nn.lml(kern, x, y, tab, DIAG, s, mu + e, MC) - nn.lml(kern, x, y, tab, DIAG, s, mu - e, MC)) / (2 * h)
    es, em = np.max(np.abs(s_bar - fs)) / np.max(np.abs(fs)), np.max(np.abs(mean_bar - fm)) / np.max(np.abs(fm))
    print(f"family {family}: s_bar {es:.2e}, mean_bar {em:.2e} of the largest entry")
    assert es <= 1e-8 and em <= 1e-8
    # the scalar blocks with the vectors in place, by the same differences
    _, gv, gil, gd, gm = nn.lml_grad(kern, x, y, tab, DIAG, s, mu, MC)
    f = lambda var, il, diag, mc: nn.lml(nr.kernel_of(family, var, il), x, y, tab, diag, s, mu, mc)
    il = kern.inv_lengthscale
    fd = [(f(VAR + h, il, DIAG, MC) - f(VAR - h, il, DIAG, MC)) / (2 * h)]
    fd += [(f(VAR, il + h * e, DIAG, MC) - f(VAR, il - h * e, DIAG, MC)) / (2 * h) for e in np.eye(2)]
    g = np.concatenate([[gv], gil])
    assert np.max(np.abs(g - np.array(fd))) <= 1e-6 * np.max(np.abs(g))
    fdd = (f(VAR, il, DIAG + h * 1e-2, MC) - f(VAR, il, DIAG - h * 1e-2, MC)) / (2 * h * 1e-2)
    fdm = (f(VAR, il, DIAG, MC + h) - f(VAR, il, DIAG, MC - h)) / (2 * h)
    assert abs(gd - fdd) <= 2e-6 * abs(gd) and abs(gm - fdm) <= 1e-6 * max(abs(gm), np.max(np.abs(mean_bar)))


@pytest.mark.parametrize("table", ["window", "random", "hub"])
def test_sum_identities(table):
    """sum_j s_bar_j = d / d diag (nn_sets_ref's own closed form gF + tr C_bar) and sum_j mean_bar_j = d / d mean_const = sum alpha"""
    n, k = 60, 7
    kern, x, y, s, mu = _problem(n, 3, o.KERNEL_MATERN52)
    tab = {"window": ns.window_table(n, k), "random": nn.random_table(n, k, 4), "hub": nn.hub_table(n, k, (0, 9), 4)}[table]
    _, s_bar, mean_bar = nn.point_grads(kern, x, y, tab, DIAG, s, mu, MC)
    gd = 0.0
    for p in nn.points(kern, x, y, tab, DIAG, s, mu, MC):
        gF = -0.5 / p["F"] + 0.5 * p["r"] ** 2 / p["F"] ** 2
        gd += gF + gF * (p["b"] @ p["b"]) - (p["r"] / p["F"]) * (p["w"] @ p["b"])
    assert abs(np.sum(s_bar) - gd) <= 1e-12 * np.sum(np.abs(s_bar))
    alpha = nn.fit(kern, x, y, tab, DIAG, s, mu, MC)["alpha"]
    assert np.max(np.abs(mean_bar - alpha)) <= 1e-12 * np.max(np.abs(alpha))
    assert abs(np.sum(mean_bar) - np.sum(alpha)) <= 1e-12 * np.sum(np.abs(alpha))
    if table == "hub":
        assert np.sum(tab == 0) == n - 1 and np.sum(tab == 9) == n - 10   # the hubs' reverse lists


def test_python_argument_errors_need_no_context(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the GPU was touched")

    monkeypatch.setattr(_ffi, "default_context", boom)
    f = GP(SEKernel())
    x, y = np.linspace(0, 1, 9), np.zeros(9)
    noisy = NearestNeighbors(3, include_noise=True)
    post = lambda a, fx_, y_, **kw: NNPosteriorGP(a, fx_, y_, **kw)
    for call in (approx_lml, approx_lml_and_gradient, post, posterior):
        with pytest.raises(AssertionError, match="the GPU was touched"):   # a good Diagonal passes every check
            call(noisy, f(x, Diagonal(np.full(9, 0.1))), y)
        with pytest.raises(_ffi.UnsupportedError):                         # a plain vector is still refused
            call(noisy, f(x, np.full(9, 0.1)), y)
        with pytest.raises(ValueError, match="one variance per point"):
            call(noisy, f(x, Diagonal(np.full(8, 0.1))), y)
        for bad in (0.0, -0.1, float("nan"), float("inf")):
            v = np.full(9, 0.1)
            v[4] = bad
            with pytest.raises(ValueError, match="must be > 0"):
                call(noisy, f(x, Diagonal(v)), y)
        g = GP(CustomMean(lambda t: np.zeros(len(t))), SEKernel())
        with pytest.raises(_ffi.UnsupportedError, match="mean_offsets="):   # a CustomMean is still refused, and names the keyword
            call(NearestNeighbors(3), g(x), y)
        with pytest.raises(ValueError, match="mean_offsets: one value per point"):
            call(NearestNeighbors(3), f(x), y, mean_offsets=np.zeros(8))
        with pytest.raises(AssertionError, match="the GPU was touched"):
            call(NearestNeighbors(3), f(x), y, mean_offsets=np.zeros(9))
    # include_noise=False ignores Σy as it always has: a Diagonal never reaches the noise checks
    with pytest.raises(AssertionError, match="the GPU was touched"):
        approx_lml(NearestNeighbors(3), f(x, Diagonal(np.full(9, -1.0))), y)
    with pytest.raises(ValueError, match="noise_grad_out needs wrt_noise=True"):
        approx_lml_and_gradient(noisy, f(x, Diagonal(np.full(9, 0.1))), y, noise_grad_out=np.zeros(9))
    with pytest.raises(ValueError, match="mean_grad_out needs wrt_mean=True"):
        approx_lml_and_gradient(noisy, f(x, 0.1), y, wrt_noise=True, mean_grad_out=np.zeros(9))
    with pytest.raises(ValueError, match="wrt_noise is True or False"):
        approx_lml_and_gradient(noisy, f(x, 0.1), y, wrt_noise=1)
    with pytest.raises(TypeError):
        approx_lml(noisy, f(x, 0.1), y, wrt_noise=True)
    # the handle's own checks come before its library call
    dev = object.__new__(DeviceNearestNeighbors)
    dev.n, dev.d, dev.dtype, dev.ctx, dev.h, dev.data, dev.kb = 9, 1, _ffi.F64, None, None, None, None
    with pytest.raises(ValueError, match="one entry per point"):
        dev.set_noise(np.zeros(8))
    with pytest.raises(ValueError, match="one entry per point"):
        dev.set_mean(np.zeros((9, 2)))
    with pytest.raises(ValueError, match="noise_grad_out: a contiguous device tensor"):
        dev.lml_grad_points(None, noise_grad_out=np.zeros(9))
    # predictions of y on a per-point-noise posterior need the test points' noise
    p = object.__new__(NNPosteriorGP)
    p.noise, p.dev = None, dev
    with pytest.raises(ValueError, match="pass noise="):
        p.predict_y(np.zeros(3))
    with pytest.raises(ValueError, match="pass noise="):
        p.log_predictive_density(np.zeros(3), np.zeros(3))
    with pytest.raises(ValueError, match="one variance per test point"):
        p.predict_y(np.zeros(3), noise=np.full(4, 0.1))
    with pytest.raises(ValueError, match="noise > 0"):
        p.predict_y(np.zeros(3), noise=0.0)
    with pytest.raises(ValueError, match="one value per test point"):
        NNPosteriorGP._offset(np.zeros(3), np.zeros(4))


def test_abi_and_header():
    assert C.sizeof(_ffi.PointNoise) == 16 and C.sizeof(_ffi.PointNoiseGrad) == 16
    assert C.sizeof(_ffi.PointMean) == 16 and C.sizeof(_ffi.PointMeanGrad) == 16
    lib = approxgp.load_library()
    for name, nargs in (("svgp_nn_set_noise", 3), ("svgp_nn_set_mean", 3), ("svgp_nn_lml_grad_points", 11)):
        assert hasattr(lib, name) and len(_ffi.SYMBOLS[name][1]) == nargs
        assert getattr(lib, name)(*([None] * nargs)) == _ffi.INVALID_ARG   # a NULL context, before anything else
    hdr = open(os.path.join(ROOT, "include", "svgp_mi355x.h")).read()
    flat = re.sub(r"\s+", " ", hdr)
    assert "int32_t svgp_nn_set_noise(svgp_ctx* ctx, svgp_nn* nn, const struct svgp_point_noise* pn);" in flat
    assert "int32_t svgp_nn_set_mean(svgp_ctx* ctx, svgp_nn* nn, const svgp_point_mean* pm);" in flat
    assert re.search(r"svgp_nn_lml_grad_points\(svgp_ctx\* ctx, svgp_nn\* nn, const svgp_nn_desc\* desc, double\* lml_out, svgp_nn_info\* info, "
                     r"double\* d_variance, double\* d_inv_lengthscale, double\* d_diag, double\* d_mean_const, "
                     r"svgp_point_mean_grad\* gpm, struct svgp_point_noise_grad\* gpn\);", flat)
