"""Round-6 GPU tests: a 48-panel fp32 Kuu.  The kernel-gradient reductions on the MFMA (grad.hip: kgrad_mfma_kernel) are covered by every gradient test
of tests/test_gpu_grad.py / test_gpu_round4.py / test_gpu_round5.py (d = 1 ... 64, both dtypes, every kernel family), which now run on it."""
import numpy as np
import pytest

import svgp_oracle as o
from approxgp import _ffi
from helpers import device_model, rel

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = _ffi.Context(0)
    yield c
    c.close()


def _factor_against_lapack(c, M, N, d, seed):
    x, y, sva, s2 = o.synth_problem(seed, N, M, d, dtype=np.float32)
    model = device_model(c, sva, dtype=np.float32, sigma2=s2)
    data = _ffi.DeviceData(c, x, y, np.float32)
    vals = {model.elbo(data, 0, N, float(N))[0] for _ in range(3)}
    assert len(vals) == 1, vals                      # run-to-run identical bits: no missing dependency between the launches
    Lk, _, _ = model.posterior()
    K = o.kuu(sva)
    L = np.tril(np.asarray(Lk, dtype=np.float64))
    back = np.linalg.norm(L @ L.T - K) / np.linalg.norm(K)
    Lref = np.linalg.cholesky(K)
    err = np.abs(L - Lref).max() / np.abs(Lref).max()
    val = vals.pop()
    ref = o.elbo(sva, x, y, sigma2=s2, num_data=float(N))
    model.free()
    data.free()
    return back, err, rel(val, ref)


def test_large_fp32_kuu_at_48_panels(ctx):
    """M = 6144 fp32 (48 panels): the factor must be LAPACK's to fp32 rounding and the ELBO the oracle's."""
    back, err, erel = _factor_against_lapack(ctx, 6144, 6200, 3, 8800)
    assert back < 2e-6, back
    assert err < 2e-3, err
    assert erel < 1e-4, erel


# (points, inducing points, d, family, likelihood, seed): cases a randomised sweep (tests/fuzz_grad.py, seed 6) found, where the fp32
# lengthscale gradient of the first MFMA form of the kernel-gradient reductions was 5e-3 ... 7e-2 away from the oracle against 1.5e-4 ... 1.5e-3
# for the entry-by-entry VALU sums of rounds 2-5: many inducing points per lengthscale, so |z - centre|^2 / lengthscale^2 multiplied the
# fp32 rounding of the accumulated sums in IL = sum z^2 R - 2 z Q + sum x^2 W.  With 8 / d centres per feature in the spare slots of the
# feature tile (grad.hip) they are 2e-4 ... 4e-3 (profiles/round6/fuzz_grad.md).
DENSE_INDUCING_FP32 = [
    (127, 129, 1, o.KERNEL_MATERN52, o.LIK_GAUSSIAN, 927227814, 2e-3),
    (33, 200, 1, o.KERNEL_MATERN52, o.LIK_GAUSSIAN, 536005819, 3e-3),
    (65, 640, 1, o.KERNEL_MATERN32, o.LIK_GAUSSIAN, 191970586, 4e-3),
    (2049, 511, 1, o.KERNEL_MATERN32, o.LIK_GAUSSIAN, 827967779, 3e-3),
]


@pytest.mark.parametrize("N,M,d,family,lik,seed,tol", DENSE_INDUCING_FP32)
def test_fp32_lengthscale_gradient_with_many_inducing_points_per_lengthscale(ctx, N, M, d, family, lik, seed, tol):
    x, y, sva, s2 = o.synth_problem(seed, N, M, d, family=family, lik=lik, dtype=np.float32)
    sva.mean_const = 0.1
    _, g_ref = o.elbo_grad(sva, x, y, lik=lik, sigma2=s2, num_data=2.5 * N)
    model = device_model(ctx, sva, dtype=np.float32, lik=lik, sigma2=s2)
    data = _ffi.DeviceData(ctx, x, y, np.float32)
    _, _, g = model.elbo_grad(data, 0, N, 2.5 * N)
    model.free()
    data.free()
    assert abs(g["inv_lengthscale"][0] - g_ref["inv_lengthscale"][0]) <= tol * abs(g_ref["inv_lengthscale"][0])


@pytest.mark.parametrize("d", [1, 2, 3, 4, 5, 8])
@pytest.mark.parametrize("dtype,tol", [(np.float64, 1e-9), (np.float32, 5e-3)])
def test_every_centre_count_of_the_feature_slots(ctx, d, dtype, tol):
    """8 / d centres per feature (8, 4, 2, 2, 1, 1 at d = 1, 2, 3, 4, 5, 8), several row blocks, a ragged last block of inducing rows and a
    batch that is not a multiple of the 128-point stage: every gradient block against the oracle."""
    N, M = 1301, 200
    x, y, sva, s2 = o.synth_problem(4000 + d, N, M, d, family=o.KERNEL_SE, dtype=dtype)
    _, g_ref = o.elbo_grad(sva, x, y, sigma2=s2, num_data=float(N))
    model = device_model(ctx, sva, dtype=dtype, sigma2=s2)
    data = _ffi.DeviceData(ctx, x, y, dtype)
    _, _, g = model.elbo_grad(data, 0, N, float(N))
    model.free()
    data.free()
    gz = g["z"].reshape(g_ref["z"].shape, order="F") if d > 1 else g["z"]
    zr = g_ref["z"] if d > 1 else g_ref["z"][0]
    for a, b in ((gz, zr), (g["inv_lengthscale"], g_ref["inv_lengthscale"]), ([g["variance"]], [g_ref["variance"]]), (g["m"], g_ref["m"])):
        a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
        assert np.abs(a - b).max() <= tol * np.abs(b).max(), (d, np.abs(a - b).max(), np.abs(b).max())


@pytest.mark.parametrize("family", [o.KERNEL_SE, o.KERNEL_MATERN32, o.KERNEL_MATERN52])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_a_nan_coordinate_reaches_the_results(ctx, dtype, family):
    """x with one NaN coordinate: the reference's arithmetic gives NaN marginals for that point and a NaN ELBO.  The clamps of the
    MFMA distance tiles (min(v, c0) for SE, max(r2, 0) for Matern) used to return the clamp value for a NaN - a FINITE value for hostile
    data (found by tests/fuzz_errors.py); they now let it through.  The other points are untouched, bit for bit."""
    N, M, d, bad = 700, 90, 3, 333
    x, y, sva, s2 = o.synth_problem(6100 + family, N, M, d, family=family, dtype=dtype)
    xb = x.copy()
    xb[1, bad] = np.nan
    model = device_model(ctx, sva, dtype=dtype, sigma2=s2)
    clean, dirty = _ffi.DeviceData(ctx, x, y, dtype), _ffi.DeviceData(ctx, xb, y, dtype)
    mu0, v0 = model.marginals(clean)
    mu1, v1 = model.marginals(dirty)
    assert np.isnan(mu1[bad]) and np.isnan(v1[bad])
    keep = np.arange(N) != bad
    assert np.array_equal(mu0[keep], mu1[keep]) and np.array_equal(v0[keep], v1[keep])
    assert not np.isfinite(model.elbo(dirty, 0, N, float(N))[0])
    val, _, g = model.elbo_grad(dirty, 0, N, float(N))
    assert not np.isfinite(val) and not np.isfinite(g["inv_lengthscale"]).any() and not np.isfinite(np.asarray(g["m"])).any()
    K = model.kuf(dirty)
    assert np.isnan(K[:, bad]).all() and np.isfinite(K[:, keep]).all()
    # a window without the point is the clean result
    assert model.elbo(dirty, 0, bad, float(N))[0] == model.elbo(clean, 0, bad, float(N))[0]
    for h in (model, clean, dirty):
        h.free()
