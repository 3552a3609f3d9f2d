"""CPU checks (no GPU) behind the input gradient of the pathwise function samples (svgp_sampler_eval_grad):

* tests/pathwise_grad_ref.py - the float64 restatement the GPU tests compare the device with - is pinned here against central
  differences of pathwise_ref.evaluate at the steps 2e-3 / invl_c and 1e-3 / invl_c: a correct gradient leaves the O(h^2) truncation of
  the differences alone, so halving the step divides the error by 4 (asserted: [3.8, 4.2]; it was 4.00 in all twelve cases) and the
  smaller error stays <= 2e-5 of max|G_c| (largest observed 1.1e-5);
* L = 0, eps = 0: it is the gradient of the exact posterior mean (pathwise_ref.posterior_moments), by the same ratio test;
* x = z_i exactly: both Matern families are finite there and equal the sum without term i (no division by r);
* svgp_sampler_eval_grad is declared in the ctypes table and in the header."""
import os
import re

import numpy as np
import pytest

import pathwise_grad_ref as pg
import pathwise_ref as pw
import svgp_oracle as o
from approxgp import _ffi
from approxgp.pathwise import draw_basis

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = {"se": o.KERNEL_SE, "matern32": o.KERNEL_MATERN32, "matern52": o.KERNEL_MATERN52}
SHAPES = [(37, 1, 1), (37, 2, 100), (130, 3, 100), (64, 8, 64)]   # (M, d, L)
STEPS = (2e-3, 1e-3)                                               # times 1 / invl_c


def _problem(family, M, d, L, S=3, n=20, zero_eps=False):
    seed = 500 + 7 * M + 13 * d + L + family
    sva, _ = pw.recipe(M, d, family, seed, centered=(family == o.KERNEL_MATERN32), mean_const=0.3)
    rng = np.random.default_rng(seed + 1)
    x = rng.uniform(-3.0, 3.0, size=(d, n))
    omega, tau, w, eps = draw_basis(family, M, L, S, rng, np.float64, d=d)
    if zero_eps:
        eps = np.zeros_like(eps)
    st = pw.setup(sva, omega, tau, w, eps)
    return sva, st, x, (omega, tau, w)


def _ratio_test(G, f, x, invl, label):
    """G (S, d, n) against central differences of f: (d, n) -> (S, n) at the two steps, per coordinate."""
    for c in range(x.shape[0]):
        scale = np.abs(G[:, c]).max()
        errs = [np.abs(pg.central_differences(f, x, c, h / invl[c]) - G[:, c]).max() / scale for h in STEPS]
        print(f"{label} c={c}: error {errs[0]:.2e} -> {errs[1]:.2e} of max|G_c|, ratio {errs[0] / errs[1]:.3f}")
        assert 3.8 <= errs[0] / errs[1] <= 4.2, (label, c, errs)
        assert errs[1] <= 2e-5, (label, c, errs)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "M%d_d%d_L%d" % s)
@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_restatement_converges_against_central_differences(name, shape):
    M, d, L = shape
    sva, st, x, (omega, tau, w) = _problem(FAMILIES[name], M, d, L)
    G = pg.gradient(sva, st, x, omega, tau, w)
    assert G.shape == (3, d, x.shape[1]) and G.dtype == np.float64
    _ratio_test(G, lambda xx: pw.evaluate(sva, st, xx, omega, tau, w), x, sva.kernel.inv_lengthscale, f"{name} {shape}")


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_no_features_and_no_noise_is_the_gradient_of_the_posterior_mean(name):
    M, d = 37, 2
    sva, st, x, (omega, tau, w) = _problem(FAMILIES[name], M, d, 0, S=2, zero_eps=True)
    G = pg.gradient(sva, st, x, omega, tau, w)
    assert np.array_equal(G[0], G[1])
    _ratio_test(G[:1], lambda xx: pw.posterior_moments(sva, xx)[0][None, :], x, sva.kernel.inv_lengthscale, f"{name} posterior mean")


@pytest.mark.parametrize("name", ["matern32", "matern52"])
@pytest.mark.parametrize("f32", [False, True])
def test_at_an_inducing_point_the_term_vanishes(name, f32):
    M, d, L = 37, 2, 100
    sva, st, x, (omega, tau, w) = _problem(FAMILIES[name], M, d, L)
    i = 5
    x = x.copy()
    x[:, 3] = sva.z[:, i]
    G = pg.gradient(sva, st, x, omega, tau, w, f32=f32)
    assert np.all(np.isfinite(G))
    without = pg.gradient(sva, st, x, omega, tau, w, f32=f32, skip=i)
    assert np.array_equal(G[:, :, 3], without[:, :, 3])
    assert not np.array_equal(G[:, :, 4], without[:, :, 4])   # elsewhere the term counts


def test_float32_chain_stays_close():
    """The float32 data stage (V rounded once) against float64 on the worst case met: SE, M = 37, d = 1, L = 1 (2.6e-5 of max|G_c|)."""
    sva, st, x, (omega, tau, w) = _problem(o.KERNEL_SE, 37, 1, 1)
    G = pg.gradient(sva, st, x, omega, tau, w)
    G32 = pg.gradient(sva, st, x, omega, tau, w, f32=True)
    assert G32.dtype == np.float32
    err = np.abs(G32.astype(np.float64) - G).max() / np.abs(G).max()
    print(f"float32 chain: {err:.2e} of max|G|")
    assert err <= 1e-4   # the project's fp32 contract


def test_symbol_is_declared():
    assert "svgp_sampler_eval_grad" in _ffi.SYMBOLS
    restype, argtypes = _ffi.SYMBOLS["svgp_sampler_eval_grad"]
    assert len(argtypes) == 11
    header = open(os.path.join(ROOT, "include", "svgp_mi355x.h")).read()
    proto = re.search(r"int32_t svgp_sampler_eval_grad\((.*?)\);", header, flags=re.S)
    assert proto and len(proto.group(1).split(",")) == 11
    assert re.search(r"gradient of f_s - mean", header)   # the header says whose the prior mean's Jacobian is
