"""GPU tests of svgp_ss_sample (DeviceStateSpace.sample, SSPosteriorGP.rand): mu and G G' from unit draws against the dense long double
posterior, paths from random draws against the sequential NumPy reference of tests/test_statespace_sample_cpu.py.  Bounds: 10 x the
float64 reference's own measured distance (that module), the margin test_gpu_statespace.py gives another summation order."""
import numpy as np
import pytest

import approxgp
import statespace_ref as R
import test_statespace_sample_cpu as T
from approxgp import _ffi
from approxgp.statespace import DeviceStateSpace

pytestmark = pytest.mark.gpu
F32_EPS = 2.0 ** -24


@pytest.fixture(scope="module")
def ctx():
    c = _ffi.Context(0)
    yield c
    c.close()


def kernel_of(family, p):
    base = approxgp.Matern32Kernel() if family == 1 else approxgp.Matern52Kernel()
    return p["variance"] * approxgp.with_lengthscale(base, 1.0 / p["inv_lengthscale"])


def fitted(ctx, family, dtype, p):
    dev = DeviceStateSpace(ctx, p["t"], p["y"], dtype)
    if np.ndim(p["sig2"]):
        dev.set_noise(p["sig2"] - p["diag"])
    dev.fit(dev.desc(kernel_of(family, p), p["diag"], p["mean_const"]))
    return dev


@pytest.mark.parametrize("family", [1, 2])
@pytest.mark.parametrize("kind", T.DIST_KINDS)
def test_unit_draws_give_the_dense_posterior(ctx, family, kind):
    """repeat: equal time stamps, Q = 0 and its factor 0; short: A ~ 0, Q = Pinf to round-off; noise: per-point variances"""
    p, mean, cov = T.dense_posterior(family, kind)
    z, eps = T.unit_draws(40, 25, family + 1)
    dev = fitted(ctx, family, np.float64, p)
    try:
        paths = dev.sample(p["ts"], z, eps)
    finally:
        dev.free()
    assert paths.shape == (25, z.shape[0]) and paths.dtype == np.float64
    e_mu, e_cov = T.distribution_errors(p, mean, cov, paths)
    print(f"ss sample family={family} {kind}: mu {e_mu:.2e} G G' {e_cov:.2e}")
    assert e_mu <= 10.0 * T.MU_TOL and e_cov <= 10.0 * T.COV_TOL


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("S", [1, 4, 5])   # 4 = SC, the samples of one chunk (statespace.hip: kSampleChunk): a part, one, one and a part
@pytest.mark.parametrize("family", [1, 2])
@pytest.mark.parametrize("U", T.PATH_U)
def test_paths_match_the_sequential_reference(ctx, family, U, S, dtype):
    # regular steps only (T.path_problem): for `short` the factor of a Q at round-off level is no stable function of its input
    p, z, eps, ref = T.path_case(family, U)
    dev = fitted(ctx, family, dtype, p)
    try:
        first, second = (dev.sample(p["ts"], z[:S], eps[:S]) for _ in range(2))
    finally:
        dev.free()
    assert first.shape == (p["ts"].shape[0], S) and first.dtype == dtype and np.array_equal(first, second)   # bit for bit
    err = np.abs(first.T - ref[:S]).max() / p["variance"]
    print(f"ss sample family={family} U={U} S={S} {np.dtype(dtype).name}: paths {err:.2e}")
    r32 = F32_EPS * np.abs(ref).max() / p["variance"] if dtype == np.float32 else 0.0
    assert err <= 10.0 * T.PATH_TOL[family] + r32


def test_unsorted_inputs_take_draws_in_the_callers_order(ctx):
    p, z, eps, ref = T.path_case(2, R.TILE + 1)
    N, n = p["t"].shape[0], p["ts"].shape[0]
    rng = np.random.default_rng(1)
    pd, pt = rng.permutation(N), rng.permutation(n)
    fx = approxgp.GP(p["mean_const"], kernel_of(2, p))(p["t"][pd], p["sig2"])
    post = approxgp.posterior(approxgp.StateSpace(), fx, p["y"][pd], ctx=ctx)
    try:
        got = post.dev.sample(p["ts"][pt], z[:, np.concatenate([pd, N + pt])], eps[:, pd])
        drawn, g = post.rand(p["ts"][pt], 3, rng=5), np.random.default_rng(5)
        again = post.dev.sample(p["ts"][pt], g.standard_normal((3, N + n, 3)), g.standard_normal((3, N)))
    finally:
        post.free()
    assert np.abs(got.T - ref[:, pt]).max() <= 10.0 * T.PATH_TOL[2] * p["variance"]
    assert drawn.shape == (n, 3) and np.array_equal(drawn, again)


def test_status_codes(ctx):
    p, z, eps, ref = T.path_case(1, R.TILE)
    N, n, lib = p["t"].shape[0], p["ts"].shape[0], ctx.lib
    out = np.zeros((5, n))
    call = lambda dev, ts=p["ts"], S=5, zz=z, ee=eps: lib.svgp_ss_sample(ctx.h, dev.h, n, _ffi._ptr(ts), S, _ffi._ptr(zz), _ffi._ptr(ee), _ffi._ptr(out))
    dev = DeviceStateSpace(ctx, p["t"], p["y"], np.float64)
    try:
        desc = dev.desc(kernel_of(1, p), p["diag"], p["mean_const"])
        assert call(dev) == _ffi.INVALID_ARG                                  # no fit yet
        dev.fit(desc)
        assert call(dev) == _ffi.OK
        dev.set_noise(None)
        assert call(dev) == _ffi.INVALID_ARG                                  # set_noise cleared the fit
        dev.fit(desc)
        bad = [call(dev, S=0), call(dev, zz=None), call(dev, ee=None), call(dev, ts=np.ascontiguousarray(p["ts"][::-1]))]
        assert bad == [_ffi.INVALID_ARG] * 4                                  # n_samples = 0, NULL draws, unsorted times
        with pytest.raises(ValueError):
            dev.sample(p["ts"], z[:, :-1], eps)                               # a shape check, before the device
        got = dev.sample(p["ts"], z, eps)                                     # and the handle still samples
    finally:
        dev.free()
    assert np.abs(got.T - ref).max() <= 10.0 * T.PATH_TOL[1] * p["variance"]
