"""GPU checks of the predictive distribution of the observation (svgp_predictive, svgp_lik_predictive; csrc/predictive.hip, lik.hpp)
against the float64 restatement tests/predictive_ref.py (itself pinned by tests/test_predictive_cpu.py).

Shapes: the smallest that cross every boundary - M below, one past and between 128-row panels (64, 129, 130, 200); a partial last block of
256 points; a window offset; d = 1, 17 (the MFMA-distance path); more points than one 65 536-point chunk (70 001: grid-stride and the
block-partial reduce); every likelihood, the closed forms and the log-domain quadrature, prior-mean offsets.  fp32: measured against the
fp64 restatement on fp32-rounded inputs, asserted at 4x the worst measured value (see F32_MEASURED)."""
import functools

import numpy as np
import pytest

import laplace_ref as lr
import natgrad_ref as nr
import predictive_ref as pr
import svgp_oracle as o
from approxgp import _ffi
from helpers import device_model

pytestmark = pytest.mark.gpu
JITTER = 1e-5
JITTER_F32 = 1e-3     # the project's fp32 problems carry the larger jitter (approxgp/synthetic.py): an fp32 cholesky(Kuu) needs it
TOL = 1e-8            # the suite's fp64 contract: relative to the largest entry, and to |sum|

# (data points N, M, d, likelihood, quadrature_n, family, ard, layout, centered, mean_const, batch_off, batch_len, prior-mean offsets)
CASES = {
    "normcdf_n513_M64_d1": (513, 64, 1, o.LIK_BERNOULLI_NORMCDF, 0, o.KERNEL_SE, False, _ffi.VEC, False, 0.0, 0, 513, False),
    "gauss_n777_M200_d3": (777, 200, 3, o.LIK_GAUSSIAN, 0, o.KERNEL_SE, True, _ffi.COLVECS, False, 0.0, 0, 777, False),
    "gauss_gh7_n777_M200_d3": (777, 200, 3, o.LIK_GAUSSIAN, 7, o.KERNEL_SE, True, _ffi.COLVECS, False, 0.0, 0, 777, False),
    "logistic_win640_M129_d17": (688, 129, 17, o.LIK_BERNOULLI_LOGISTIC, 20, o.KERNEL_MATERN32, False, _ffi.COLVECS, True, 0.0, 37, 640, False),
    "poisson_n1000_M130_d8": (1000, 130, 8, o.LIK_POISSON_EXP, 0, o.KERNEL_SE, True, _ffi.ROWVECS, False, -0.4, 0, 1000, True),
    "gamma_n600_M64_d2": (600, 64, 2, o.LIK_GAMMA_EXP, 0, o.KERNEL_MATERN52, False, _ffi.COLVECS, False, 0.0, 0, 600, False),
    "exponential_n600_M64_d2": (600, 64, 2, o.LIK_EXPONENTIAL_EXP, 0, o.KERNEL_MATERN52, False, _ffi.COLVECS, False, 0.0, 0, 600, False),
    "gauss_n70001_M64_d2": (70001, 64, 2, o.LIK_GAUSSIAN, 0, o.KERNEL_SE, True, _ffi.COLVECS, False, 0.0, 0, 70001, False),
}
F32_CASES = {
    "f32_gauss_n777_M200_d3": CASES["gauss_n777_M200_d3"],
    "f32_logistic_win640_M129_d17": CASES["logistic_win640_M129_d17"],
}
GAMMA_ALPHA = 2.5
Y_HUGE = 400.0        # one Poisson count far in the tail: a plain log(sum w exp(.)) underflows there
# fp32 models against the fp64 restatement on fp32-rounded inputs: the worst error over F32_CASES as measured on an MI355X, per-point
# outputs relative to their largest entry, sum_lpd relative to |sum_lpd|.  The asserts take 4x these (box-to-box reduction-order
# differences); sum_lpd must in any case stay inside the project's fp32 contract of 1e-4.  Per case (lpd, ymean, yvar, sum_lpd):
# Gaussian n = 777 M = 200: 8.5e-6, 3.0e-5, 1.4e-5, 3.5e-7; Centered logistic window n = 640 M = 129: 1.2e-6, 1.0e-6, 4.8e-7, 3.2e-8.
F32_MEASURED = {"lpd": 8.48e-06, "ymean": 3.01e-05, "yvar": 1.42e-05, "sum_lpd": 3.48e-07}


@pytest.fixture(scope="module")
def ctx():
    c = _ffi.Context(0)
    yield c
    c.close()


def _dtype(name):
    return np.float32 if name.startswith("f32") else np.float64


@functools.lru_cache(maxsize=None)
def _problem(name):
    """(spec, x, y, s2, SVA, mux, reference outputs of the window) - the reference is computed once and shared, read-only."""
    spec = {**CASES, **F32_CASES}[name]
    N, M, d, lik, qn, family, ard, layout, centered, mc, off, n, with_mux = spec
    dtype = _dtype(name)
    rd = lambda a: np.asarray(a, dtype=dtype).astype(np.float64)
    kernel, z, x, y, s2, m0, Lq0 = nr.problem(N, M, d, lik=lik, family=family, ard=ard, dtype=dtype, mean_const=mc)
    rng = np.random.default_rng(4000 + N + M)
    if lik == o.LIK_GAMMA_EXP:
        s2 = GAMMA_ALPHA
        y = rd(rng.gamma(GAMMA_ALPHA, np.exp(np.clip(y, -3.0, 3.0)) / GAMMA_ALPHA) + 1e-3)
    elif lik == o.LIK_EXPONENTIAL_EXP:
        y = rd(rng.exponential(np.exp(np.clip(y, -3.0, 3.0))) + 1e-3)
    elif lik == o.LIK_POISSON_EXP:
        y = y.copy()
        y[5] = Y_HUGE
    sva = nr.start_sva(kernel, z, JITTER_F32 if dtype == np.float32 else JITTER, m0, Lq0, mean_const=mc, centered=centered)
    if dtype == np.float32:   # the device holds q in fp32: the reference starts from the same rounded values
        sva = o.SVA(kernel, z, rd(sva.m), rd(sva.Lq), jitter=sva.jitter, mean_const=mc, centered=centered)
    mux = rd(0.3 * np.sin(1.3 * x[0]) + 0.05 * rng.standard_normal(N)) if with_mux else None
    sl = slice(off, off + n)
    ref = pr.predictive(sva, x[:, sl], y[sl], lik, s2, qn, mux=None if mux is None else mux[sl])
    for a in [x, y, sva.m, sva.Lq] + [v for v in ref.values() if isinstance(v, np.ndarray)] + ([mux] if mux is not None else []):
        a.setflags(write=False)
    return spec, x, y, s2, sva, mux, ref


def _data(ctx, name, with_y=True):
    spec, x, y, _, _, _, _ = _problem(name)
    d, layout = spec[2], spec[7]
    xd = x[0] if d == 1 else (x if layout == _ffi.COLVECS else np.ascontiguousarray(x.T))
    return _ffi.DeviceData(ctx, xd, y if with_y else None, _dtype(name), layout=layout if d > 1 else _ffi.VEC)


def _model(ctx, name, **kw):
    spec, _, _, s2, sva, _, _ = _problem(name)
    return device_model(ctx, sva, dtype=_dtype(name), lik=spec[3], sigma2=s2, quadrature_n=spec[4], **kw)


def _window(name):
    spec, _, _, _, _, mux, _ = _problem(name)
    off, n = spec[10], spec[11]
    return off, n, (None if mux is None else mux[off:off + n])


def _err(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def _errors(got, ref):
    s = got["summary"]
    return {"lpd": _err(got["lpd"], ref["lpd"]), "ymean": _err(got["ymean"], ref["ymean"]), "yvar": _err(got["yvar"], ref["yvar"]),
            "sum_lpd": abs(s.sum_lpd - ref["sum_lpd"]) / abs(ref["sum_lpd"]),
            "sum_sq_err": abs(s.sum_sq_err - ref["sum_sq_err"]) / abs(ref["sum_sq_err"])}


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("lpd", "ymean", "yvar")) and all(
        getattr(a["summary"], f) == getattr(b["summary"], f) for f in ("sum_lpd", "sum_sq_err", "n_points", "n_neg_var"))


@pytest.mark.parametrize("name", list(CASES))
def test_matches_the_restatement(ctx, name):
    """Per-point lpd / ymean / yvar and both sums against predictive_ref; the call twice is bitwise equal; svgp_elbo before and after is
    bitwise unchanged; the array form fed svgp_marginals' output returns the same per-point values, also without y."""
    spec, x, y, s2, sva, _, ref = _problem(name)
    lik, qn = spec[3], spec[4]
    off, n, pm = _window(name)
    model, data = _model(ctx, name), _data(ctx, name)
    try:
        before = model.elbo(data, off, n, 0.0, prior_mean=pm)[0]
        got = model.predictive(data, off, n, prior_mean=pm)
        again = model.predictive(data, off, n, prior_mean=pm)
        after = model.elbo(data, off, n, 0.0, prior_mean=pm)[0]
        mu, var = model.marginals(data, off, n, prior_mean=pm)
        only_sum = model.predictive(data, off, n, prior_mean=pm, want=("summary",))
        timing = ctx.timing()
    finally:
        model.free()
        data.free()
    err = _errors(got, ref)
    print(f"{name}: " + " ".join(f"{k} {v:.2e}" for k, v in err.items()))
    assert all(np.isfinite(got[k]).all() for k in ("lpd", "ymean", "yvar"))
    assert all(v < TOL for v in err.values()), err
    s = got["summary"]
    assert (s.n_points, s.n_neg_var) == (n, 0) == (ref["n_points"], ref["n_neg_var"])
    assert _same(got, again)
    assert before == after                                                  # the new call leaves no state behind
    assert only_sum["summary"].sum_lpd == s.sum_lpd and only_sum["summary"].sum_sq_err == s.sum_sq_err and list(only_sum) == ["summary"]
    if timing.ms_total > 0:                                                 # (a context created with SVGP_TIMING=0 reports zeros)
        assert timing.ms_strip > 0 and timing.ms_expect > 0 and timing.strip_launches >= 1
    # the array form on the same marginals
    yw = y[off:off + n]
    arr = _ffi.lik_predictive(ctx, lik, s2, qn, mu, var, yw)
    for k in ("lpd", "ymean", "yvar"):
        assert _err(arr[k], got[k]) <= 1e-13, (k, _err(arr[k], got[k]))
    assert abs(arr["summary"].sum_lpd - s.sum_lpd) <= 1e-13 * abs(s.sum_lpd) and arr["summary"].n_points == n
    mom = _ffi.lik_predictive(ctx, lik, s2, qn, mu, var)                    # y = NULL: the moments alone
    assert sorted(mom) == ["ymean", "yvar"]
    assert np.array_equal(mom["ymean"], arr["ymean"]) and np.array_equal(mom["yvar"], arr["yvar"])


def test_poisson_tail_count_is_finite(ctx):
    """y = 400 at a point whose rate is a few: the log-domain quadrature with its running maximum stays finite."""
    name = "poisson_n1000_M130_d8"
    _, _, y, _, _, _, ref = _problem(name)
    off, n, pm = _window(name)
    assert y[5] == Y_HUGE and np.isfinite(ref["lpd"][5])
    model, data = _model(ctx, name), _data(ctx, name)
    try:
        lpd = model.predictive(data, off, n, prior_mean=pm, want=("lpd",))["lpd"]
    finally:
        model.free()
        data.free()
    assert np.isfinite(lpd[5]) and abs(lpd[5] - ref["lpd"][5]) <= TOL * abs(ref["lpd"][5])
    # the same count where the rate stays below e^0.71 at every node: every term of the sum is below exp(-745)
    edge = _ffi.lik_predictive(ctx, o.LIK_POISSON_EXP, 1.0, 0, [-1.0], [0.05], [Y_HUGE], want=("lpd",))["lpd"][0]
    want = float(pr.lpd(o.LIK_POISSON_EXP, [-1.0], [0.05], [Y_HUGE])[0])
    assert want < -745.0 and np.isfinite(edge) and abs(edge - want) <= TOL * abs(want)


def test_data_without_observations(ctx):
    """A data object without y: ymean / yvar still work and equal the values with y; summary / lpd are SVGP_INVALID_ARG from the
    library itself (the Python layer's own check is bypassed here), before anything is enqueued."""
    import ctypes as C
    name = "gamma_n600_M64_d2"
    _, _, _, _, _, _, ref = _problem(name)
    off, n, _ = _window(name)
    model, data = _model(ctx, name), _data(ctx, name, with_y=False)
    try:
        got = model.predictive(data, off, n, want=("ymean", "yvar"))
        with pytest.raises(ValueError):
            model.predictive(data, off, n)
        buf, summ = np.zeros(n), _ffi.PredSummary()
        lib = ctx.lib
        assert lib.svgp_predictive(ctx.h, model.h, data.h, off, n, None, C.byref(summ), None, None, None) == _ffi.INVALID_ARG
        assert lib.svgp_predictive(ctx.h, model.h, data.h, off, n, None, None, _ffi._ptr(buf), None, None) == _ffi.INVALID_ARG
        assert lib.svgp_predictive(ctx.h, model.h, data.h, off, n, None, None, None, None, None) == _ffi.INVALID_ARG
        assert lib.svgp_predictive(ctx.h, model.h, data.h, off, n + 1, None, None, None, _ffi._ptr(buf), None) == _ffi.INVALID_ARG
        bad_pm = _ffi.PointMean(None, 0, 0)
        assert lib.svgp_predictive(ctx.h, model.h, data.h, off, n, C.byref(bad_pm), None, None, _ffi._ptr(buf), None) == _ffi.INVALID_ARG
        bad_pm = _ffi.PointMean(_ffi._ptr(buf), 2, 0)
        assert lib.svgp_predictive(ctx.h, model.h, data.h, off, n, C.byref(bad_pm), None, None, _ffi._ptr(buf), None) == _ffi.INVALID_ARG
        one = np.ones(3)
        p = _ffi._ptr(one)
        assert lib.svgp_lik_predictive(ctx.h, 0, 1.0, 0, 3, p, p, None, C.byref(summ), None, None, None) == _ffi.INVALID_ARG
        assert lib.svgp_lik_predictive(ctx.h, 0, 1.0, 0, 3, p, p, None, None, p, None, None) == _ffi.INVALID_ARG
        assert lib.svgp_lik_predictive(ctx.h, 6, 1.0, 0, 3, p, p, p, None, p, None, None) == _ffi.UNSUPPORTED
        assert lib.svgp_lik_predictive(ctx.h, 0, 1.0, 0, 0, p, p, p, None, p, None, None) == _ffi.INVALID_ARG
        assert lib.svgp_lik_predictive(ctx.h, 0, 0.0, 0, 3, p, p, p, None, p, None, None) == _ffi.INVALID_ARG
        assert lib.svgp_lik_predictive(ctx.h, 2, 1.0, 513, 3, p, p, p, None, p, None, None) == _ffi.INVALID_ARG
    finally:
        model.free()
        data.free()
    assert _err(got["ymean"], ref["ymean"]) < TOL and _err(got["yvar"], ref["yvar"]) < TOL


def test_negative_variance_policies(ctx):
    """A model pushed into negative predictive variances the way test_gpu_parity.py::test_error_statuses does it (a negative jitter on a
    nearly diagonal Kuu), with a Poisson likelihood.  ERROR: SVGP_NEG_VARIANCE, n_neg_var > 0, NaN at those points only, the rest and
    both sums the restatement's.  CLAMP: finite everywhere; the clamped points (v = 0) have the zero-spread value log p(y | mu)."""
    z = np.linspace(-2, 2, 8)[None, :]
    k = o.Kernel(o.KERNEL_SE, 1.0, [5.0])
    neg = o.SVA(k, z, 0.2 * np.cos(np.arange(8.0)), 1e-3 * np.eye(8), jitter=-1e-3)
    x = np.concatenate([z[0], 0.5 * (z[0, 1:] + z[0, :-1]), [-3.3, 2.9, 3.7]])[None, :]     # at z: v < 0; between and outside: v > 0
    n = x.shape[1]
    y = np.random.default_rng(5).poisson(1.5, size=n).astype(np.float64)
    mu, v = pr.latent_marginals(neg, x)
    bad = v < 0
    assert 0 < bad.sum() < n and np.abs(v).min() > 1e-6                                    # the signs are not a matter of rounding
    ref_e = pr.from_marginals(o.LIK_POISSON_EXP, mu, v, y)
    ref_c = pr.from_marginals(o.LIK_POISSON_EXP, mu, v, y, clamp=True)
    data = _ffi.DeviceData(ctx, x, y, np.float64)
    strict = device_model(ctx, neg, lik=o.LIK_POISSON_EXP)
    clamp = device_model(ctx, neg, lik=o.LIK_POISSON_EXP, neg_var_policy=_ffi.NEGVAR_CLAMP)
    try:
        with pytest.raises(_ffi.DomainError) as e:
            strict.predictive(data)
        got_e = e.value.outputs
        got_c = clamp.predictive(data)
        mu_c, var_c = clamp.marginals(data)
        arr = _ffi.lik_predictive(ctx, o.LIK_POISSON_EXP, 1.0, 0, mu_c, var_c, y)           # v = 0 through the array form: not negative
        with pytest.raises(_ffi.DomainError) as e2:                                         # var[i] < 0 there: the error policy
            _ffi.lik_predictive(ctx, o.LIK_POISSON_EXP, 1.0, 0, mu, v, y)
    finally:
        strict.free()
        clamp.free()
        data.free()
    s = got_e["summary"]
    assert s.n_neg_var == int(bad.sum()) > 0 and s.n_points == n - int(bad.sum())
    for kk in ("lpd", "ymean", "yvar"):
        assert np.array_equal(np.isnan(got_e[kk]), bad), kk                                  # NaN at those points only
        assert _err(got_e[kk][~bad], ref_e[kk][~bad]) < TOL
        assert np.isfinite(got_c[kk]).all() and _err(got_c[kk], ref_c[kk]) < TOL
        assert np.array_equal(np.isnan(e2.value.outputs[kk]), bad) and _err(e2.value.outputs[kk][~bad], ref_e[kk][~bad]) < TOL
    assert abs(s.sum_lpd - ref_e["sum_lpd"]) <= TOL * abs(ref_e["sum_lpd"]) and abs(s.sum_sq_err - ref_e["sum_sq_err"]) <= TOL * ref_e["sum_sq_err"]
    sc = got_c["summary"]
    assert sc.n_neg_var == int(bad.sum()) and sc.n_points == n
    assert abs(sc.sum_lpd - ref_c["sum_lpd"]) <= TOL * abs(ref_c["sum_lpd"])
    i = int(np.flatnonzero(bad)[0])                                                          # the zero-spread edge: log p(y | mu)
    assert abs(got_c["lpd"][i] - float(o.loglik(o.LIK_POISSON_EXP, mu[i], y[i]))) <= 1e-12 * max(1.0, abs(got_c["lpd"][i]))
    assert _err(arr["lpd"], got_c["lpd"]) <= 1e-13 and arr["summary"].n_neg_var == 0
    assert e2.value.outputs["summary"].n_neg_var == int(bad.sum())


def test_non_finite_inputs_give_non_finite_outputs(ctx):
    mu, var, y = np.array([0.1, np.nan, 0.3]), np.array([0.2, 0.2, np.inf]), np.array([1.0, 2.0, 0.0])
    got = _ffi.lik_predictive(ctx, o.LIK_POISSON_EXP, 1.0, 0, mu, var, y)                    # SVGP_OK: nothing raised
    assert np.isfinite(got["lpd"][0]) and not np.isfinite(got["lpd"][1]) and not np.isfinite(got["ymean"][1])
    assert not np.isfinite(got["summary"].sum_lpd) and got["summary"].n_neg_var == 0


def test_high_order_rule_skips_vanished_weights(ctx):
    """quadrature_n = 512: the outer weights of the rule are 0 in fp64 and are skipped, not turned into -inf - -inf."""
    rng = np.random.default_rng(8)
    mu, var = rng.standard_normal(300), 0.05 + rng.random(300)
    y = (rng.random(300) < 0.5).astype(np.float64)
    got = _ffi.lik_predictive(ctx, o.LIK_BERNOULLI_LOGISTIC, 1.0, 512, mu, var, y)
    ref = pr.from_marginals(o.LIK_BERNOULLI_LOGISTIC, mu, var, y, 1.0, 512)
    assert np.isfinite(got["lpd"]).all()
    assert _err(got["lpd"], ref["lpd"]) < TOL and _err(got["ymean"], ref["ymean"]) < TOL


def test_laplace_posterior(ctx):
    """The Laplace posterior's predict_y / log_predictive_density on the n = 200, d = 2 Bernoulli problem of test_gpu_laplace.py equal
    predictive_ref applied to laplace_ref's latent predictions."""
    from approxgp import GP, BernoulliLikelihood, LaplaceApproximation, LatentGP, posterior
    from approxgp.kernels import ARDTransform, ScaledKernel, SEKernel, TransformedKernel
    x, y = lr.synth(1, 200, 2, seed=3)
    rng = np.random.default_rng(12)
    xs = rng.uniform(-2, 2, size=(2, 150))
    ys = (rng.random(150) < 0.5).astype(np.float64)
    il = np.array([0.8, 0.8])
    lf = LatentGP(GP(ScaledKernel(TransformedKernel(SEKernel(), ARDTransform(il)), 1.5)), BernoulliLikelihood(), 1e-6)
    post = posterior(LaplaceApproximation(), lf(x), y, ctx=ctx)
    try:
        ym, yv = post.predict_y(xs)
        lpd = post.log_predictive_density(xs, ys)
    finally:
        post.dev.free()
    _, cache, _, _ = lr.fit(lr.kernel_of(0, 1.5, il), x, y, 1, jitter=1e-6)
    rm, rv, _ = lr.predict(cache, lr.kernel_of(0, 1.5, il), x, xs)
    ref = pr.from_marginals(o.LIK_BERNOULLI_LOGISTIC, rm, rv, ys)
    assert _err(ym, ref["ymean"]) < TOL and _err(yv, ref["yvar"]) < TOL and _err(lpd, ref["lpd"]) < TOL
    assert np.all((ym > 0) & (ym < 1))


def test_python_top_layer(ctx):
    """posterior(sva, lfx, y).predict_y / log_predictive_density through the package's own types (a Poisson model with a constant prior
    mean), and the NearestNeighbors posterior's Gaussian case through the same array form."""
    import approxgp as ag
    from approxgp.kernels import ARDTransform, ScaledKernel, SEKernel, TransformedKernel
    name = "poisson_n1000_M130_d8"
    spec, x, y, s2, sva, _, _ = _problem(name)
    ref = pr.predictive(sva, x, y, o.LIK_POISSON_EXP)
    kern = ScaledKernel(TransformedKernel(SEKernel(), ARDTransform(np.asarray(sva.kernel.inv_lengthscale))), sva.kernel.variance)
    f = ag.GP(sva.mean_const, kern)
    approx = ag.SparseVariationalApproximation(f(sva.z, sva.jitter), ag.MvNormal.from_cholesky(sva.m, sva.Lq))
    lfx = ag.LatentGP(f, ag.PoissonLikelihood(), 1e-6)(x)
    post = ag.posterior(approx, lfx, y, ctx=ctx)
    ym, yv = post.predict_y(x)
    lpd = post.log_predictive_density(x, y)
    assert _err(ym, ref["ymean"]) < TOL and _err(yv, ref["yvar"]) < TOL and _err(lpd, ref["lpd"]) < TOL
    with pytest.raises(ValueError, match="likelihood"):
        ag.posterior(approx, ctx=ctx).predict_y(x)
    # NearestNeighbors regression: (mean, var + noise) and log N(y; mean, var + noise)
    rng = np.random.default_rng(21)
    xn = rng.uniform(-2, 2, size=(2, 60))                                   # 59 neighbours of 60 points: the exact GP, v > 0
    yn = np.sin(2 * xn[0]) + 0.1 * rng.standard_normal(60)
    xt, yt = rng.uniform(-2, 2, size=(2, 70)), rng.standard_normal(70)
    g = ag.GP(ag.SEKernel())
    pn = ag.posterior(ag.NearestNeighbors(59, include_noise=True), g(xn, 0.04), yn, ctx=ctx)
    try:
        m, v = pn.mean_and_var(xt)
        ymn, yvn = pn.predict_y(xt)
        ln = pn.log_predictive_density(xt, yt)
    finally:
        pn.dev.free()
    m, v = np.asarray(m, dtype=np.float64), np.asarray(v, dtype=np.float64)
    assert np.array_equal(ymn, m) and _err(yvn, v + 0.04) <= 1e-15
    assert _err(ln, pr.lpd(o.LIK_GAUSSIAN, m, v, yt, 0.04)) < 1e-12


def _f32_errors(ctx, name):
    _, _, _, _, _, _, ref = _problem(name)
    off, n, pm = _window(name)
    model, data = _model(ctx, name), _data(ctx, name)
    try:
        got = model.predictive(data, off, n, prior_mean=pm)
    finally:
        model.free()
        data.free()
    err = _errors(got, ref)
    return {k: err[k] for k in F32_MEASURED}


def test_fp32_accuracy(ctx):
    worst = {k: 0.0 for k in F32_MEASURED}
    for name in F32_CASES:
        err = _f32_errors(ctx, name)
        print(f"{name}: " + " ".join(f"{k} {v:.2e}" for k, v in err.items()))
        worst = {k: max(worst[k], err[k]) for k in worst}
    print("fp32 worst:", {k: f"{v:.2e}" for k, v in worst.items()})
    assert worst["sum_lpd"] <= 1e-4                                          # the project's fp32 contract
    for k, v in worst.items():
        assert v <= 4 * F32_MEASURED[k], (k, v)
