"""CPU checks (no GPU) behind the predictive distribution of the observation (svgp_predictive / svgp_lik_predictive):

* tests/predictive_ref.py - the float64 restatement the GPU tests compare the device with - is pinned here INDEPENDENTLY: against
  adaptive quadrature of p(y | f) N(f; mu, v), against Monte Carlo, by normalisation over y and by Jensen's inequality against the
  ELBO's term, so that device-equals-restatement means something;
* the new symbols exist and their argument checks happen before the GPU is touched.

GH-20 and the grid (measured on the CPU with this file's own reference, see GH20_MEASURED): Gauss-Hermite with 20 nodes
resolves the integral when the likelihood is flat on the scale of sqrt(v) - every v = 1e-6 cell to rounding, v = 0.3 to 1e-6 or better
except where y sits far in the likelihood's tail - and does NOT resolve a Poisson count far above e^mu at v >= 0.3 (y = 300, v = 0.3,
mu = -2: the integrand's mass lies 14 prior standard deviations out, beyond the rule's last node at 7.6; the error in the log density is
7e2).  That is a property of the rule the library documents (quadrature_n is the caller's to raise), not of the arithmetic, and it is
recorded here rather than excluded.  No cell is excluded: the adaptive reference reports a relative error below 1e-13 in every cell."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest
from scipy import integrate, optimize

import predictive_ref as pr
import svgp_oracle as o
from approxgp import _ffi

MUS, VS = (-2.0, 0.0, 1.5), (1e-6, 0.3, 2.0)
YS = {o.LIK_GAUSSIAN: (-3.0, 0.4, 2.5), o.LIK_BERNOULLI_LOGISTIC: (0.0, 1.0), o.LIK_BERNOULLI_NORMCDF: (0.0, 1.0),
      o.LIK_POISSON_EXP: (0.0, 3.0, 40.0, 300.0), o.LIK_EXPONENTIAL_EXP: (0.01, 1.0, 25.0), o.LIK_GAMMA_EXP: (0.01, 1.0, 25.0)}
PARAM = {o.LIK_GAUSSIAN: 0.25, o.LIK_GAMMA_EXP: 2.5}

# What the reference itself may be off by, in log p: scipy.integrate.quad's own estimate is < 1e-13 relative in the integral in every
# cell (asserted below), i.e. 1e-13 absolute in its logarithm; |log p| reaches 2.0e3 (Poisson y = 300 at v = 1e-6), where one ulp is
# 2.3e-13, and reference and restatement each carry a few of them.
REF_TOL = 5e-12
# Worst |GH-20 - adaptive| of log p over mu in MUS (and over y, except for the Poisson, whose cells differ by orders of magnitude with
# y), measured on the CPU (x86-64, glibc libm, scipy quad).  Keys: (likelihood, v) or (LIK_POISSON_EXP, v, y).  The assertion is 10 x these (+ REF_TOL).
GH20_MEASURED = {
    (o.LIK_GAUSSIAN, 1e-6): 7.82e-14, (o.LIK_GAUSSIAN, 0.3): 6.76e-07, (o.LIK_GAUSSIAN, 2.0): 3.24e-02,   # sigma2 = 0.25: narrow against v = 2
    (o.LIK_BERNOULLI_LOGISTIC, 1e-6): 7.73e-14, (o.LIK_BERNOULLI_LOGISTIC, 0.3): 5.00e-16, (o.LIK_BERNOULLI_LOGISTIC, 2.0): 1.55e-07,
    (o.LIK_BERNOULLI_NORMCDF, 1e-6): 7.70e-14, (o.LIK_BERNOULLI_NORMCDF, 0.3): 8.88e-16, (o.LIK_BERNOULLI_NORMCDF, 2.0): 1.78e-07,
    (o.LIK_EXPONENTIAL_EXP, 1e-6): 7.82e-14, (o.LIK_EXPONENTIAL_EXP, 0.3): 2.18e-03, (o.LIK_EXPONENTIAL_EXP, 2.0): 1.99e-02,
    (o.LIK_GAMMA_EXP, 1e-6): 8.08e-14, (o.LIK_GAMMA_EXP, 0.3): 1.13e-03, (o.LIK_GAMMA_EXP, 2.0): 2.95e-02,
    (o.LIK_POISSON_EXP, 1e-6, 0.0): 7.11e-14, (o.LIK_POISSON_EXP, 1e-6, 3.0): 9.33e-15, (o.LIK_POISSON_EXP, 1e-6, 40.0): 7.82e-14,
    (o.LIK_POISSON_EXP, 1e-6, 300.0): 0.0,
    (o.LIK_POISSON_EXP, 0.3, 0.0): 8.31e-10, (o.LIK_POISSON_EXP, 0.3, 3.0): 1.11e-07,
    (o.LIK_POISSON_EXP, 0.3, 40.0): 9.00e+00, (o.LIK_POISSON_EXP, 0.3, 300.0): 6.98e+02,                 # NOT resolved (see above)
    (o.LIK_POISSON_EXP, 2.0, 0.0): 1.34e-04, (o.LIK_POISSON_EXP, 2.0, 3.0): 1.23e-02,
    (o.LIK_POISSON_EXP, 2.0, 40.0): 1.14e+00, (o.LIK_POISSON_EXP, 2.0, 300.0): 1.43e+01,                 # NOT resolved
}


def _ref_lpd(lik, mu, v, y, param):
    """log int p(y | f) N(f; mu, v) df by adaptive quadrature around the integrand's mode (every likelihood here is log-concave in f),
    in the log domain: the integrand is scaled by its maximum.  -> (log p, quad's relative error estimate)."""
    def g(f):
        return float(o.loglik(lik, np.float64(f), np.float64(y), param)) - 0.5 * (f - mu) ** 2 / v - 0.5 * math.log(2 * math.pi * v)

    sd = math.sqrt(v)
    fs = optimize.minimize_scalar(lambda f: -g(f), bracket=(mu - sd, mu + sd), tol=1e-14).x
    c, h = g(fs), 1e-3 * sd
    w = 1.0 / math.sqrt(max(-(g(fs + h) - 2 * c + g(fs - h)) / h ** 2, 1e-300))   # the mode's width from its curvature
    val, err = integrate.quad(lambda f: math.exp(g(f) - c), fs - 40 * w, fs + 40 * w, points=[fs - 4 * w, fs, fs + 4 * w], epsabs=0,
                              epsrel=1e-13, limit=500)
    return c + math.log(val), err / val


@pytest.fixture(scope="module")
def grid():
    """{(lik, mu, v, y): (reference log p, its relative error estimate)}: computed once, shared, never changed."""
    out = {}
    for lik in pr.LIKS:
        for mu, v, y in itertools.product(MUS, VS, YS[lik]):
            out[(lik, mu, v, y)] = _ref_lpd(lik, mu, v, y, PARAM.get(lik, 1.0))
    return out


def _key(lik, v, y):
    return (lik, v, y) if lik == o.LIK_POISSON_EXP else (lik, v)


def test_gh20_log_density_against_adaptive_quadrature(grid):
    worst = {}
    for (lik, mu, v, y), (ref, rerr) in grid.items():
        assert rerr < 1e-13, ("the adaptive reference is not converged", lik, mu, v, y, rerr)   # no cell is excluded
        got = float(pr.lpd(lik, [mu], [v], [y], PARAM.get(lik, 1.0), 20)[0])
        assert np.isfinite(got), (lik, mu, v, y)
        k = _key(lik, v, y)
        worst[k] = max(worst.get(k, 0.0), abs(got - ref))
    for k in sorted(worst):
        print(f"GH-20 {k}: worst |error| {worst[k]:.2e} (recorded {GH20_MEASURED[k]:.2e})")
    assert set(worst) == set(GH20_MEASURED)
    for k, e in worst.items():
        assert e <= 10 * GH20_MEASURED[k] + REF_TOL, (k, e, GH20_MEASURED[k])


def test_closed_forms_against_adaptive_quadrature(grid):
    """quadrature_n = 0: log N(y; mu, v + sigma2) and log Phi(+-mu / sqrt(1 + v)) are the integral itself."""
    for (lik, mu, v, y), (ref, _) in grid.items():
        if lik in (o.LIK_GAUSSIAN, o.LIK_BERNOULLI_NORMCDF):
            assert pr.predictive_gh(lik, 0) == 0
            got = float(pr.lpd(lik, [mu], [v], [y], PARAM.get(lik, 1.0), 0)[0])
            assert abs(got - ref) <= REF_TOL, (lik, mu, v, y, got - ref)
        else:
            assert pr.predictive_gh(lik, 0) == 20   # Poisson / Exponential / Gamma: closed ELBO term, no closed predictive density


def _sample_y(rng, lik, f, param):
    if lik == o.LIK_GAUSSIAN:
        return f + math.sqrt(param) * rng.standard_normal(f.shape)
    if lik == o.LIK_BERNOULLI_LOGISTIC:
        return (rng.random(f.shape) < 1.0 / (1.0 + np.exp(-f))).astype(np.float64)
    if lik == o.LIK_BERNOULLI_NORMCDF:
        return (rng.standard_normal(f.shape) < f).astype(np.float64)          # P(xi < f) = Phi(f)
    if lik == o.LIK_POISSON_EXP:
        return rng.poisson(np.exp(f)).astype(np.float64)
    if lik == o.LIK_EXPONENTIAL_EXP:
        return rng.exponential(np.exp(f))
    return rng.gamma(param, np.exp(f))


@pytest.mark.parametrize("lik", pr.LIKS)
def test_moments_against_monte_carlo(lik):
    """(E[y], Var[y]) - the five closed forms, and the logistic Bernoulli's quadrature - against 2e6 samples of f ~ N(mu, v),
    y ~ p(y | f), fixed seed, at 5 standard errors (of the sample mean; of the sample variance, from the sample's fourth moment)."""
    n, param = 2_000_000, PARAM.get(lik, 1.0)
    for j, (mu, v) in enumerate(((0.3, 0.2), (-1.0, 0.5))):
        rng = np.random.default_rng(1000 + 10 * lik + j)
        ys = _sample_y(rng, lik, mu + math.sqrt(v) * rng.standard_normal(n), param)
        ym, yv = (float(a[0]) for a in pr.moments(lik, [mu], [v], param))
        m, c = ys.mean(), ys - ys.mean()
        s2 = float((c * c).mean())
        se_m, se_v = math.sqrt(s2 / n), math.sqrt(max(float((c ** 4).mean()) - s2 * s2, 0.0) / n)
        print(f"lik {lik} (mu, v) = ({mu}, {v}): mean {ym:.6f} vs {m:.6f} ({abs(ym - m) / se_m:.2f} se), var {yv:.6f} vs {s2:.6f} "
              f"({abs(yv - s2) / se_v:.2f} se)")
        assert abs(ym - m) <= 5 * se_m, (lik, mu, v)
        assert abs(yv - s2) <= 5 * se_v, (lik, mu, v)


def test_log_density_is_normalised_over_y():
    mu, v = np.array([-2.0, 0.0, 1.5, 0.4]), np.array([1e-6, 0.3, 2.0, 0.0])
    for lik, qn in ((o.LIK_BERNOULLI_LOGISTIC, 0), (o.LIK_BERNOULLI_NORMCDF, 0), (o.LIK_BERNOULLI_LOGISTIC, 7), (o.LIK_BERNOULLI_NORMCDF, 7)):
        p0, p1 = (np.exp(pr.lpd(lik, mu, v, np.full(4, yy), 1.0, qn)) for yy in (0.0, 1.0))
        assert np.max(np.abs(p0 + p1 - 1.0)) <= 1e-12, (lik, qn)
        if not (lik == o.LIK_BERNOULLI_NORMCDF and qn > 0):   # (there lpd takes GH-n while the moments keep their closed form)
            np.testing.assert_allclose(p1, pr.moments(lik, mu, v, 1.0, qn)[0], rtol=0, atol=1e-12)   # E[y] is the class-1 probability
    ys = np.arange(201.0)
    total = np.exp(pr.lpd(o.LIK_POISSON_EXP, np.full(201, 1.0), np.full(201, 0.3), ys)).sum()
    # the mass beyond y = 200 is below 1e-60 at these moments; the sum over y of a quadrature with weights summing to 1 is exact
    assert abs(total - 1.0) <= 1e-12, total


def test_log_density_edges_are_finite():
    """The log-sum-exp and zero-spread edges the GPU tests visit: a Poisson count of 400 (a plain log(sum w exp(.)) underflows: every
    term is below exp(-745)) and v = 0, where the quadrature collapses to log p(y | mu); the 512-node rule, whose outer weights are 0."""
    a = float(pr.lpd(o.LIK_POISSON_EXP, [-1.0], [0.05], [400.0])[0])    # the rate stays below e^0.71 at every node
    assert np.isfinite(a) and a < -745.0
    b = float(pr.lpd(o.LIK_POISSON_EXP, [0.5], [0.0], [3.0])[0])
    assert abs(b - float(o.loglik(o.LIK_POISSON_EXP, np.float64(0.5), np.float64(3.0)))) <= 1e-14
    assert (np.asarray(o.gausshermite(512)[1]) == 0.0).any()
    c = float(pr.lpd(o.LIK_BERNOULLI_LOGISTIC, [0.3], [0.4], [1.0], 1.0, 512)[0])
    ref, _ = _ref_lpd(o.LIK_BERNOULLI_LOGISTIC, 0.3, 0.4, 1.0, 1.0)
    assert abs(c - ref) <= REF_TOL


@pytest.mark.parametrize("lik", pr.LIKS)
def test_jensen_log_density_is_above_the_elbo_term(lik):
    """log p(y_i | D) >= E_q[log p(y_i | f_i)] pointwise: the statement that makes the predictive density a different quantity from the
    ELBO's expectation.  With the SAME rule on both sides (GH-20) it holds exactly - the weights are positive and sum to 1 - so the only
    slack is rounding; at the library's defaults (closed forms where they exist) it holds up to GH-20's own error, which is below 1e-6 at
    this problem's variances."""
    x, y, sva, s2 = o.synth_problem(31, 80, 12, 2, lik=lik)
    mu, v = pr.latent_marginals(sva, x)
    assert v.min() > 0
    lp, el = pr.lpd(lik, mu, v, y, s2, 20), pr.expected_loglik_points(lik, mu, v, y, s2, 20)
    assert np.all(lp >= el - 1e-12 * np.maximum(1.0, np.abs(el))), float((lp - el).min())
    assert np.all(lp > el) or lik == o.LIK_GAUSSIAN and np.all(lp >= el)     # strictly, wherever the likelihood is not flat
    assert np.median(lp - el) > 1e-6                                          # ... and by far more than rounding: not the same quantity
    lp0, el0 = pr.lpd(lik, mu, v, y, s2, 0), pr.expected_loglik_points(lik, mu, v, y, s2, 0)
    assert np.all(lp0 >= el0 - 1e-6)


# ---- the library side: symbols, struct layout, argument checks before the GPU ------------------------------------------------------
class _NoGpu:
    """Stands where a Context goes: any use of the library through it is an error."""

    def __getattr__(self, name):
        raise AssertionError(f"the GPU context was touched ({name}) before the arguments were checked")


def test_symbols_and_struct_layout():
    lib = _ffi.load_library()
    assert hasattr(lib, "svgp_predictive") and hasattr(lib, "svgp_lik_predictive")
    assert C.sizeof(_ffi.PredSummary) == 32 and _ffi.PredSummary.n_points.offset == 16 and _ffi.PredSummary.n_neg_var.offset == 24
    # a NULL context is refused by the library itself, without a device
    one = np.zeros(1)
    assert lib.svgp_lik_predictive(None, 0, 1.0, 0, 1, _ffi._ptr(one), _ffi._ptr(one), None, None, None, _ffi._ptr(one), None) == _ffi.INVALID_ARG
    assert lib.svgp_predictive(None, None, None, 0, 1, None, None, None, _ffi._ptr(one), None) == _ffi.INVALID_ARG


def test_argument_checks_happen_before_the_gpu():
    ctx, mu, var, y = _NoGpu(), np.zeros(5), np.ones(5), np.zeros(5)
    with pytest.raises(ValueError, match="need y"):            # outputs that require y, without y
        _ffi.lik_predictive(ctx, _ffi.LIK_GAUSSIAN, 0.1, 0, mu, var, None, want=("summary",))
    with pytest.raises(ValueError, match="need y"):
        _ffi.lik_predictive(ctx, _ffi.LIK_GAUSSIAN, 0.1, 0, mu, var, None, want=("ymean", "lpd"))
    for bad in (-1, 6, 99, 1.0, True):                         # bad likelihood code
        with pytest.raises(ValueError, match="likelihood"):
            _ffi.lik_predictive(ctx, bad, 1.0, 0, mu, var, y)
    with pytest.raises(ValueError, match="n must be"):         # n < 1
        _ffi.lik_predictive(ctx, _ffi.LIK_POISSON_EXP, 1.0, 0, np.zeros(0), np.zeros(0), np.zeros(0))
    with pytest.raises(ValueError, match="one entry per point"):
        _ffi.lik_predictive(ctx, _ffi.LIK_POISSON_EXP, 1.0, 0, mu, var[:4], y)
    with pytest.raises(ValueError, match="quadrature_n"):
        _ffi.lik_predictive(ctx, _ffi.LIK_POISSON_EXP, 1.0, 513, mu, var, y)
    with pytest.raises(ValueError, match="sigma2 > 0"):
        _ffi.lik_predictive(ctx, _ffi.LIK_GAUSSIAN, 0.0, 0, mu, var, y)
    with pytest.raises(ValueError, match="want"):
        _ffi.lik_predictive(ctx, _ffi.LIK_GAUSSIAN, 1.0, 0, mu, var, y, want=("nlpd",))

    class _Data:   # what DeviceModel.predictive reads of a DeviceData before it calls the library
        n, h = 9, None

    model = _ffi.DeviceModel.__new__(_ffi.DeviceModel)
    model.ctx, model.dtype, model.h = ctx, _ffi.F64, None
    try:
        no_y, with_y = _Data(), _Data()
        no_y.has_y, with_y.has_y = False, True
        with pytest.raises(ValueError, match="need y"):
            model.predictive(no_y)                                                    # default want includes summary and lpd
        with pytest.raises(ValueError, match="need y"):
            model.predictive(no_y, want=("lpd", "yvar"))
        with pytest.raises(ValueError, match="batch range"):
            model.predictive(with_y, 4, 6)
        with pytest.raises(ValueError, match="batch range"):
            model.predictive(with_y, 0, 0)
        with pytest.raises(ValueError, match="prior_mean"):                           # bad svgp_point_mean: wrong length
            model.predictive(with_y, 0, 9, prior_mean=np.zeros(4))
        with pytest.raises(ValueError, match="want"):
            model.predictive(with_y, want=())
    finally:
        model.h = None   # nothing to free
