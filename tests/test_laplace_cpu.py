"""CPU checks of the Laplace approximation's reference (tests/laplace_ref.py) and of the host-side pieces of approxgp.laplace.
The reference reaches the reference package's own Laplace optimum driven by its closed-form gradient, and that gradient is the
derivative of its own lml."""
import numpy as np
import pytest
from scipy.optimize import minimize

import laplace_ref as lr
import svgp_oracle as o
from test_reference_literal_pin import LBFGS, NELDER_MEAD, X, Y


def _neg_lml_and_grad(theta):
    """-approx_lml(build_latent_gp(theta)) and its theta gradient, softplus chained by hand (variance = softplus(t0),
    lengthscale = softplus(t1), inv_lengthscale = 1 / lengthscale)."""
    v, l = o.softplus(theta[0]), o.softplus(theta[1])
    k = lr.kernel_of(o.KERNEL_SE, v, [1.0 / l])
    lml, dv, dil = lr.lml_grad(k, X, Y, o.LIK_BERNOULLI_LOGISTIC, jitter=1e-8)
    sig = 1.0 / (1.0 + np.exp(-np.asarray(theta)))   # d softplus / dt
    return -lml, -np.array([dv * sig[0], float(np.sum(dil)) * (-1.0 / l ** 2) * sig[1]])


def test_reference_reaches_the_pinned_optimum_with_its_own_gradient():
    res = minimize(_neg_lml_and_grad, np.array([5.0, 1.0]), jac=True, method="L-BFGS-B",
                   options={"ftol": 1e-15, "gtol": 1e-10, "maxiter": 500})
    np.testing.assert_allclose(res.x, LBFGS, rtol=1e-6)
    np.testing.assert_allclose(res.x, NELDER_MEAD, rtol=1e-4)


@pytest.mark.parametrize("lik", [0, 1, 2, 3, 4, 5])
@pytest.mark.parametrize("family", [o.KERNEL_SE, o.KERNEL_MATERN32, o.KERNEL_MATERN52])
def test_closed_form_gradient_matches_central_differences(lik, family):
    x, y = lr.synth(lik, 40, 2, seed=10 * lik + family)
    s2 = 0.3 if lik == o.LIK_GAUSSIAN else (2.0 if lik == o.LIK_GAMMA_EXP else 1.0)
    var, il = 1.3, np.array([0.9, 1.4])
    _, dv, dil = lr.lml_grad(lr.kernel_of(family, var, il), x, y, lik, s2, jitter=1e-6)

    def lml(v, l):
        return lr.fit(lr.kernel_of(family, v, l), x, y, lik, s2, jitter=1e-6, maxiter=200)[0]

    h = 1e-5
    fd_v = (lml(var + h, il) - lml(var - h, il)) / (2 * h)
    fd_l = np.array([(lml(var, il + h * e) - lml(var, il - h * e)) / (2 * h) for e in np.eye(2)])
    scale = max(abs(fd_v), np.max(np.abs(fd_l)))
    assert abs(dv - fd_v) <= 1e-5 * scale, (dv, fd_v)
    np.testing.assert_allclose(dil, fd_l, rtol=0, atol=1e-5 * scale)


def test_derivatives_match_differences_of_the_oracle_loglik():
    f = np.linspace(-3.0, 3.0, 13)
    for lik, y, s2 in ((0, 0.4, 0.5), (1, 1.0, 1.0), (1, 0.0, 1.0), (2, 3.0, 1.0), (3, 0.7, 1.0), (4, 1.3, 2.5), (5, 1.0, 1.0),
                       (5, 0.0, 1.0)):
        yy = np.full_like(f, y)
        d2, d3 = lr.d2d3(lik, f, yy, s2)
        h = 1e-4
        g = lambda t: np.asarray(o._dloglik(lik, t, yy, s2), dtype=np.float64)
        np.testing.assert_allclose(d2, (g(f + h) - g(f - h)) / (2 * h), rtol=1e-6, atol=1e-8)
        d2f = lambda t: lr.d2d3(lik, t, yy, s2)[0]
        np.testing.assert_allclose(d3, (d2f(f + h) - d2f(f - h)) / (2 * h), rtol=1e-6, atol=1e-8)
        assert np.all(d2 <= 0.0)   # log-concave: W >= 0


def test_host_argument_checks():
    from approxgp import GP, BernoulliLikelihood, LaplaceApproximation, LatentGP, SEKernel, approx_lml
    with pytest.raises(ValueError):
        LaplaceApproximation(maxiter=0)
    lf = LatentGP(GP(0.5, SEKernel()), BernoulliLikelihood(), 1e-8)   # nonzero prior mean: the reference asserts
    with pytest.raises(AssertionError):
        approx_lml(LaplaceApproximation(), lf(X), Y)


def test_svgp_dispatch_passes_every_keyword_through(monkeypatch):
    """approx_lml / posterior of the package dispatch on the approximation type: any other approximation reaches the SVGP method
    with exactly the positional and keyword arguments it was given (ctx and dtype included)."""
    import approxgp
    from approxgp import laplace as lp
    seen = []
    monkeypatch.setattr(lp._sva, "approx_lml", lambda *a, **k: seen.append(("approx_lml", a, k)) or 1.5)
    monkeypatch.setattr(lp._sva, "posterior", lambda *a, **k: seen.append(("posterior", a, k)) or "post")
    kw = dict(num_data=5, ctx="MYCTX", dtype="float32", quadrature="Q", return_terms=True)
    assert approxgp.approx_lml("SVA", "LFX", "Y", **kw) == 1.5
    assert approxgp.posterior("SVA", "FX", "Y", ctx="C2", dtype="float64") == "post"
    assert approxgp.posterior("SVA") == "post"
    assert seen == [("approx_lml", ("SVA", "LFX", "Y"), kw), ("posterior", ("SVA", "FX", "Y"), {"ctx": "C2", "dtype": "float64"}),
                    ("posterior", ("SVA",), {})]


def test_laplace_branch_rejects_unknown_keywords():
    from approxgp import GP, BernoulliLikelihood, LaplaceApproximation, LatentGP, SEKernel, approx_lml, posterior
    lf = LatentGP(GP(SEKernel()), BernoulliLikelihood(), 1e-8)
    with pytest.raises(TypeError):
        approx_lml(LaplaceApproximation(), lf(X), Y, num_dat=5)
    with pytest.raises(TypeError):
        posterior(LaplaceApproximation(), lf(X), Y, dtyp="float32")
