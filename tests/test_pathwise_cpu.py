"""CPU checks (no GPU) behind pathwise posterior function samples (svgp_sampler_*, approxgp/pathwise.py):

* tests/pathwise_ref.py - the float64 restatement the GPU tests compare the device with - is pinned here INDEPENDENTLY: the moments of
  4000 of its samples against the exact posterior moments, and the identity f(z) + jitter V = u, which holds whatever the features are;
* draw_basis draws what the header documents (shapes, dtypes, the Student-t degrees of freedom of the Matern frequencies);
* the ctypes struct is the header's, the new symbols exist and reject bad arguments before the GPU is touched.

Bounds of the statistics: the sample mean of S draws has standard error sqrt(var / S) and must lie within 6 of them; the sample
covariance carries the Fourier error O(variance / sqrt(L)) = 0.029 at L = 2048 (averaged over the 40 feature draws) plus its own
sampling error of about variance sqrt(2 / S) = 0.029, and must lie within 0.1 variance = 0.13.  Measured on the CPU with the seeds
below (printed by the test): mean error 1.05 / 1.68 / 1.85 standard errors and covariance error 0.034 / 0.028 / 0.027 for
Matern-3/2 / Matern-5/2 / SE - the restatement alone stays well inside the bounds."""
import ctypes as C
import os
import re

import numpy as np
import pytest
from scipy import stats

import pathwise_ref as pw
import svgp_oracle as o
from approxgp import _ffi
from approxgp.pathwise import draw_basis

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = {"se": o.KERNEL_SE, "matern32": o.KERNEL_MATERN32, "matern52": o.KERNEL_MATERN52}
VARIANCE = 1.3


def _model(family, centered, seed):
    sva, _ = pw.recipe(40, 2, family, seed, centered=centered, mean_const=0.3 if centered else 0.0, variance=VARIANCE)
    return sva


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_sample_moments_match_the_posterior(name):
    family = FAMILIES[name]
    sva = _model(family, centered=(name == "matern32"), seed=11)
    M, d, L, S = 40, 2, 2048, 4000
    rng = np.random.default_rng(2024)
    x = rng.uniform(-3.0, 3.0, size=(d, 6))
    # 40 independent draws of the features, 100 functions on each (as 40 samplers of 100 samples would be used)
    F = []
    for _ in range(S // 100):
        omega, tau, w, eps = draw_basis(family, M, L, 100, rng, np.float64, d=d)
        st = pw.setup(sva, omega, tau, w, eps)
        F.append(pw.evaluate(sva, st, x, omega, tau, w))
    F = np.concatenate(F)                     # (S, 6)
    mean, cov = pw.posterior_moments(sva, x)
    se = np.sqrt(np.diag(cov) / S)
    zscore = np.abs(F.mean(axis=0) - mean) / se
    cerr = np.abs(np.cov(F.T) - cov).max()
    print(f"{name}: mean error / s.e. {zscore.max():.2f}, covariance error {cerr:.3f} (variance {VARIANCE})")
    assert zscore.max() < 6.0
    assert cerr < 0.1 * VARIANCE


@pytest.mark.parametrize("centered", [False, True])
@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_identity_at_the_inducing_points(name, centered):
    """f(z) + jitter V = u: the update term is exact, whatever L and the features are."""
    family = FAMILIES[name]
    sva, muz = pw.recipe(40, 2, family, 5, centered=centered, mean_const=-0.4, with_muz=True)
    for L in (0, 7, 300):
        omega, tau, w, eps = draw_basis(family, 40, L, 5, np.random.default_rng(L), np.float64, d=2)
        st = pw.setup(sva, omega, tau, w, eps, muz=muz)
        F = pw.evaluate(sva, st, sva.z, omega, tau, w, mux=muz)
        assert np.abs(F.T + sva.jitter * st["V"] - st["u"]).max() < 1e-10


def test_draw_basis_shapes_dtypes_and_degrees_of_freedom():
    import approxgp as ag

    for dt in (np.float32, np.float64):
        omega, tau, w, eps = draw_basis(o.KERNEL_SE, 9, 33, 4, np.random.default_rng(0), dt, d=3)
        assert (omega.shape, tau.shape, w.shape, eps.shape) == ((33, 3), (33,), (4, 33), (4, 9))
        assert {a.dtype for a in (omega, tau, w, eps)} == {np.dtype(dt)}
        assert tau.min() >= 0.0 and tau.max() < 2 * np.pi + 1e-6
    omega, tau, w, eps = draw_basis(o.KERNEL_SE, 5, 0, 2, np.random.default_rng(0), np.float64, d=2)
    assert omega.shape == (0, 2) and tau.shape == (0,) and w.shape == (2, 0) and eps.shape == (2, 5)
    # kernel objects carry the family (and an ARD transform the dimension)
    k = 0.7 * (ag.Matern52Kernel() @ ag.ARDTransform([1.0, 2.0, 4.0]))
    assert draw_basis(k, 5, 8, 1, np.random.default_rng(0))[0].shape == (8, 3)
    assert draw_basis(ag.SqExponentialKernel(), 5, 8, 1, np.random.default_rng(0), d=2)[0].shape == (8, 2)
    with pytest.raises(ValueError):
        draw_basis(o.KERNEL_SE, 5, 8, 0)
    # the marginal of a frequency coordinate: N(0, 1) for SE, Student-t with 2 nu degrees of freedom for Matern-nu - and not the others'
    n = 40000
    dists = {o.KERNEL_SE: stats.norm(), o.KERNEL_MATERN32: stats.t(3), o.KERNEL_MATERN52: stats.t(5)}
    for family, dist in dists.items():
        col = draw_basis(family, 1, n, 1, np.random.default_rng(77), np.float64, d=2)[0][:, 1]
        assert stats.kstest(col, dist.cdf).pvalue > 1e-3, family
        for other, wrong in dists.items():
            if other != family:
                assert stats.kstest(col, wrong.cdf).pvalue < 1e-6, (family, other)
    # one chi-square draw per FEATURE: the coordinates of a Matern frequency share their scale (|omega_1| and |omega_2| correlate)
    om = draw_basis(o.KERNEL_MATERN32, 1, n, 1, np.random.default_rng(78), np.float64, d=2)[0]
    assert stats.spearmanr(np.abs(om[:, 0]), np.abs(om[:, 1]))[0] > 0.1
    se = draw_basis(o.KERNEL_SE, 1, n, 1, np.random.default_rng(78), np.float64, d=2)[0]
    assert abs(stats.spearmanr(np.abs(se[:, 0]), np.abs(se[:, 1]))[0]) < 0.03


def test_features_reproduce_the_prior_covariance():
    """Phi(z) Phi(z)' -> k(z, z) at rate O(variance / sqrt(L)) for the three spectral densities (the convention of oracle/CONVENTIONS.md's kappa)."""
    for family in FAMILIES.values():
        sva = _model(family, False, 3)
        L = 2048
        omega, tau, _, _ = draw_basis(family, 40, L, 1, np.random.default_rng(9), np.float64, d=2)
        Phi = pw.amplitude(sva.kernel, L) * pw.features(sva.kernel, sva.z, omega, tau)
        err = np.abs(Phi @ Phi.T - o.kernelmatrix(sva.kernel, sva.z)).max()
        assert err < 5 * VARIANCE / np.sqrt(L), (family, err)


def test_struct_layout_matches_the_header():
    hdr = open(os.path.join(ROOT, "include", "svgp_mi355x.h")).read()
    body = re.search(r"typedef struct svgp_sample_basis \{(.*?)\} svgp_sample_basis;", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", " ", body, flags=re.S)
    fields = re.findall(r"(int64_t|const void\*)\s+(\w+);", body)
    assert [f[1] for f in fields] == [f[0] for f in _ffi.SampleBasis._fields_]
    for (ctype, name), (_, pytype) in zip(fields, _ffi.SampleBasis._fields_):
        assert pytype is (C.c_int64 if ctype == "int64_t" else C.c_void_p), name
    assert C.sizeof(_ffi.SampleBasis) == 48 and _ffi.SampleBasis.omega.offset == 16 and _ffi.SampleBasis.eps.offset == 40


def test_symbols_exist_and_reject_null_arguments_without_a_gpu():
    lib = _ffi.load_library()
    h = C.c_void_p()
    basis = _ffi.SampleBasis(0, 1, None, None, None, None)
    assert lib.svgp_sampler_create(None, None, C.byref(basis), C.byref(h)) == _ffi.INVALID_ARG
    assert lib.svgp_sampler_eval(None, None, None, 0, 1, None, None, 1, 0) == _ffi.INVALID_ARG
    assert lib.svgp_sampler_state(None, None, None, None) == _ffi.INVALID_ARG
    assert lib.svgp_sampler_free(None, None) == _ffi.OK
