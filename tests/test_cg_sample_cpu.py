"""CPU checks (no GPU) of the pathwise function samples of the exact GP: the float64 restatement tests/cg_sample_ref.py against central
differences, against cg_ref's posterior mean and, by a seeded moment check, against the exact posterior; the declared prototypes, the
shapes of the random numbers and the Python layer's argument checks, which happen before a context exists."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import approxgp
import cg_ref as cr
import cg_sample_ref as sr
import svgp_oracle as o
from approxgp import _ffi, iterative
from approxgp.pathwise import draw_basis

FAMILIES = [o.KERNEL_SE, o.KERNEL_MATERN32, o.KERNEL_MATERN52]
NEW = ["svgp_cg_sampler_create", "svgp_cg_sampler_eval", "svgp_cg_sampler_eval_grad", "svgp_cg_sampler_state", "svgp_cg_sampler_free",
       "svgp_cg_sampler_plan"]


def _problem(N, d, family, seed=0):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-3, 3, size=(d, N))
    kernel = o.Kernel(family, 1.3, np.full(d, 1 / 0.7))
    y = np.sin(x.sum(0)) + 0.1 * rng.standard_normal(N)
    return kernel, x, y


@pytest.mark.parametrize("family", FAMILIES)
def test_gradient_equals_central_differences(family):
    d, N, S, L = 3, 40, 3, 33
    kernel, x, y = _problem(N, d, family, 1)
    omega, tau, w, eps = draw_basis(family, N, L, S, np.random.default_rng(2), np.float64, d=d)
    xs = np.random.default_rng(3).uniform(-3, 3, size=(d, 7))
    F, G, V = sr.sample(kernel, x, 0.1, y - 0.3, xs, omega, tau, w, eps, 0.3)
    h = 1e-6
    for c in range(d):
        e = np.zeros((d, 1))
        e[c] = h
        fd = (sr.evaluate(kernel, x, V, xs + e, omega, tau, w, 0.3)[0] - sr.evaluate(kernel, x, V, xs - e, omega, tau, w, 0.3)[0]) / (2 * h)
        np.testing.assert_allclose(G[:, c, :], fd, atol=2e-8 * max(1.0, np.abs(G).max()))
    # the float32 chain is the same function to float32 accuracy
    F32, _ = sr.evaluate(kernel, x, V, xs, omega, tau, w, 0.3, f32=True)
    G32, _ = sr.gradient(kernel, x, V, xs, omega, tau, w, f32=True)
    assert F32.dtype == np.float32 and G32.dtype == np.float32
    assert np.abs(F32 - F).max() <= 1e-3 * np.abs(F).max() and np.abs(G32 - G).max() <= 1e-3 * np.abs(G).max()


@pytest.mark.parametrize("family", FAMILIES)
def test_no_features_and_no_noise_draw_give_the_posterior_mean(family):
    d, N = 2, 60
    kernel, x, y = _problem(N, d, family, 4)
    xs = np.random.default_rng(5).uniform(-3, 3, size=(d, 17))
    F, G, V = sr.sample(kernel, x, 0.1, y - 0.2, xs, np.zeros((0, d)), np.zeros(0), np.zeros((2, 0)), np.zeros((2, N)), 0.2)
    m, _ = cr.predict(kernel, x, 0.1, y - 0.2, xs, 0.2)
    np.testing.assert_allclose(F, np.broadcast_to(m, (2, 17)), atol=1e-12 * np.abs(m).max())
    alpha = np.linalg.solve(cr.khat(kernel, x, 0.1), y - 0.2)
    np.testing.assert_allclose(V[:, 0], alpha, rtol=0, atol=1e-12 * np.abs(alpha).max())   # (LAPACK's order differs with the column count)


def test_interpolation_identity_holds_whatever_L():
    kernel, x, y = _problem(30, 1, o.KERNEL_MATERN52, 6)
    for L in (0, 5, 300):
        omega, tau, w, eps = draw_basis(o.KERNEL_MATERN52, 30, L, 4, np.random.default_rng(7), np.float64, d=1)
        F, _, V = sr.sample(kernel, x, 0.1, y, x, omega, tau, w, eps)
        res = F.T + np.sqrt(0.1) * eps.T + 0.1 * V - y[:, None]      # f_s(X) + sigma eps_s + sigma^2 V_s = y
        assert np.abs(res).max() <= 1e-10 * np.abs(y).max()


MOMENT_SEED = 0


def test_sample_moments_match_the_exact_posterior():
    """N = 30, S = 4000, L = 4096, five test points: the sample mean and every covariance entry within five standard errors of the exact
    posterior's (mean: sqrt(C_ii / S); covariance entry: sqrt((C_ii C_jj + C_ij^2) / S), the Gaussian value).  Seeded: deterministic."""
    N, S, L, d = 30, 4000, 4096, 1
    kernel, x, y = _problem(N, d, o.KERNEL_SE, 8)
    xs = np.array([[-3.4, -1.0, 0.3, 1.9, 3.6]])
    omega, tau, w, eps = draw_basis(o.KERNEL_SE, N, L, S, np.random.default_rng(MOMENT_SEED), np.float64, d=d)
    F, _, _ = sr.sample(kernel, x, 0.1, y, xs, omega, tau, w, eps)
    mean, cov = sr.posterior_moments(kernel, x, 0.1, y, xs)
    sm, sc = F.mean(0), np.cov(F.T)
    dv = np.diag(cov)
    z_mean = np.abs(sm - mean) / np.sqrt(dv / S)
    z_cov = np.abs(sc - cov) / np.sqrt((np.outer(dv, dv) + cov ** 2) / S)
    print("moments: largest z of the mean", z_mean.max(), "of the covariance", z_cov.max())
    assert z_mean.max() <= 5.0 and z_cov.max() <= 5.0


def test_new_prototypes_are_declared():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "svgp_mi355x.h")).read()
    for name in NEW:
        assert name in _ffi.SYMBOLS, name
        m = re.search(r"int32_t\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
        assert m, f"{name} is not declared in the header"
        assert len(m.group(1).split(",")) == len(_ffi.SYMBOLS[name][1]), name
    assert "pathwise samples, multi-GPU" not in header, "the CG section still lists pathwise samples as out of scope"
    for n in ("DeviceCGSampler", "CGFunctionSamples", "cg_sample_plan", "pack_cg_basis"):
        assert hasattr(approxgp, n)
    assert hasattr(approxgp.CGPosteriorGP, "function_samples") and hasattr(approxgp.DeviceConjugateGradients, "sampler")


def test_plan_is_a_function_of_N_alone_and_matches_the_library():
    lib = _ffi.load_library()
    # the rule, worked by hand: segments of 512 rows (ceil(N / 32 / 1024) chunks beyond 1024 segments), rounds of 2^20 / segments
    # rounded down to 256 and clamped to [256, 4096]
    want = {0: (512, 1, 4096), 1: (512, 1, 4096), 512: (512, 1, 4096), 513: (512, 2, 4096), 1124: (512, 3, 4096), 100_000: (512, 196, 4096),
            200_000: (512, 391, 2560), 524_288: (512, 1024, 1024), 1_000_000: (992, 1009, 1024), 5_000_000: (4896, 1022, 1024)}
    for N, plan in want.items():
        sr_, ns, rd = C.c_int64(), C.c_int32(), C.c_int64()
        assert lib.svgp_cg_sampler_plan(N, C.byref(sr_), C.byref(ns), C.byref(rd)) == _ffi.OK
        assert (sr_.value, ns.value, rd.value) == plan == iterative.cg_sample_plan(N), (N, sr_.value, ns.value, rd.value)
        assert sr_.value % 32 == 0 and ns.value * sr_.value >= N and ns.value <= 1024
    assert lib.svgp_cg_sampler_plan(-1, C.byref(sr_), C.byref(ns), C.byref(rd)) == _ffi.INVALID_ARG
    assert lib.svgp_cg_sampler_plan(5, None, C.byref(ns), C.byref(rd)) == _ffi.INVALID_ARG


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_draw_basis_shapes_for_the_exact_gp(family, dtype):
    N, L, S, d = 37, 12, 5, 3
    omega, tau, w, eps = draw_basis(family, N, L, S, np.random.default_rng(0), dtype, d=d)
    assert omega.shape == (L, d) and tau.shape == (L,) and w.shape == (S, L) and eps.shape == (S, N)
    assert all(a.dtype == dtype for a in (omega, tau, w, eps))
    Lp, Sp, om, ta, ww, ee = iterative.pack_cg_basis(N, d, _ffi.dtype_code(dtype), (omega, tau, w, eps))
    assert (Lp, Sp) == (L, S) and ee.flags.c_contiguous and ee.shape == (S, N) and ee.dtype == dtype
    L0 = iterative.pack_cg_basis(N, d, _ffi.dtype_code(dtype), draw_basis(family, N, 0, S, np.random.default_rng(0), dtype, d=d))
    assert L0[0] == 0 and L0[2].shape == (0, d)


def test_argument_checks_raise_without_a_context():
    N, d = 20, 2
    omega, tau, w, eps = draw_basis(o.KERNEL_SE, N, 8, 3, np.random.default_rng(0), np.float64, d=d)
    bad = [(omega, tau, w, eps[:, :-1]), (omega, tau, w, eps[0]), (omega, tau, w[:2], eps), (omega[:, :1], tau, w, eps),
           (omega, tau[:-1], w, eps), (omega, tau, w, np.zeros((0, N))), (omega, tau, w)]
    for b in bad:
        with pytest.raises(ValueError):
            iterative.pack_cg_basis(N, d, _ffi.F64, b)
    # the handle's method runs them first: an object that never saw a context raises the same errors
    dev = object.__new__(approxgp.DeviceConjugateGradients)
    dev.n, dev.d, dev.dtype = N, d, _ffi.F64
    with pytest.raises(ValueError):
        dev.sampler(None, (omega, tau, w, eps[:, :-1]))
    with pytest.raises(ValueError):
        dev.sampler(None, (omega, tau, w, eps), delta=np.zeros(N + 1))
    dev.h = dev.data = None
    for ns, nf in ((0, 8), (-1, 8), (1.5, 8), (2, -1), (2, 0.5)):
        with pytest.raises(ValueError):
            iterative._check_sample_counts(ns, nf)
    post = object.__new__(approxgp.CGPosteriorGP)
    with pytest.raises(ValueError):
        post.function_samples(0)
    for x in (np.zeros((3, 4)), np.zeros(4), np.zeros((2, 0)), np.zeros((2, 3, 1))):
        with pytest.raises(ValueError):
            iterative.check_points(x, 2)
    assert iterative.check_points(np.zeros(4), 1).shape == (4,)
    with pytest.raises(ValueError):
        iterative.cg_sample_plan(-1)
