"""CPU checks behind the predictive gradients (svgp_predictor_*): the float64 closed form the GPU tests compare against
(test_gpu_predict_grad.reference) is the derivative of the oracle's own mean / var, and ApproxPosteriorGP.mean_and_var_with_grad
returns gradients shaped like its input."""
import numpy as np
import pytest

import pathwise_ref as pw
import svgp_oracle as o
from approxgp import _ffi, sva as sva_mod
from test_gpu_predict_grad import reference

FAMILIES = (o.KERNEL_SE, o.KERNEL_MATERN32, o.KERNEL_MATERN52)


@pytest.mark.parametrize("centered", [False, True])
@pytest.mark.parametrize("d", [1, 3, 9])
def test_closed_form_is_the_derivative_of_the_oracle(d, centered):
    """Central differences of svgp_oracle.mean / var at two steps: their truncation error alone is left, so halving the step divides
    the error by 4 (between 3.5 and 4.5), and the smaller step is within 1e-5 of the closed form."""
    family = FAMILIES[(d + centered) % 3]
    sva, _ = pw.recipe(23, d, family, 40 + d, centered=centered, mean_const=0.4, jitter=1e-3)
    post = o.posterior(sva)
    x = np.random.default_rng(d).uniform(-3.0, 3.0, size=(d, 31))
    mean, var, dmean, dvar = reference(sva, None, x)
    assert np.abs(mean - o.mean(post, x)).max() <= 1e-12 and np.abs(var - o.var(post, x)).max() <= 1e-12
    for c in range(d):
        errs = []
        for h in (2e-3, 1e-3):
            xp, xm = x.copy(), x.copy()
            xp[c] += h / sva.kernel.inv_lengthscale[c]
            xm[c] -= h / sva.kernel.inv_lengthscale[c]
            step = 2 * h / sva.kernel.inv_lengthscale[c]
            fd = ((o.mean(post, xp) - o.mean(post, xm)) / step, (o.var(post, xp) - o.var(post, xm)) / step)
            errs.append([np.abs(f - g[c]).max() / np.abs(g[c]).max() for f, g in zip(fd, (dmean, dvar))])
        ratios = np.array(errs[0]) / np.array(errs[1])
        assert np.all((3.5 <= ratios) & (ratios <= 4.5)) and max(errs[1]) <= 1e-5, (c, errs)


class _StubPredictor:
    def __init__(self, d):
        self.d = d

    def eval(self, data, prior_mean=None):
        n = data.n
        g = np.arange(self.d * n, dtype=np.float64).reshape(self.d, n)
        return np.zeros(n) + (0 if prior_mean is None else prior_mean), np.ones(n), g, -g

    def free(self):
        pass


class _StubData:
    def __init__(self, ctx, x, y, dtype, layout=_ffi.COLVECS):
        x = np.asarray(x)
        self.n, self.d = (x.shape[0], 1) if x.ndim == 1 else (x.shape if layout == _ffi.ROWVECS else x.shape[::-1])

    def free(self):
        pass


@pytest.mark.parametrize("shape, layout, want", [((7,), None, (7,)), ((3, 7), None, (3, 7)), ((3, 7), _ffi.COLVECS, (3, 7)),
                                                 ((7, 3), _ffi.ROWVECS, (7, 3))])
def test_wrapper_shapes_the_gradients_like_x(monkeypatch, shape, layout, want):
    d = 1 if len(shape) == 1 else 3
    post = sva_mod.ApproxPosteriorGP.__new__(sva_mod.ApproxPosteriorGP)
    post.ctx = None
    post.prior = type("P", (), {"mean_offsets": staticmethod(lambda x: np.full(7, 2.0))})()
    post._model = type("M", (), {"dtype": _ffi.F64, "predictor": staticmethod(lambda: _StubPredictor(d))})()
    monkeypatch.setattr(_ffi, "DeviceData", _StubData)
    mean, var, dmean, dvar = post.mean_and_var_with_grad(np.zeros(shape), layout=layout)
    assert mean.shape == (7,) and np.all(mean == 2.0) and var.shape == (7,)
    assert dmean.shape == want and dvar.shape == want
    g = np.arange(d * 7, dtype=np.float64).reshape(d, 7)
    expect = g[0] if len(shape) == 1 else (g.T if layout == _ffi.ROWVECS else g)
    assert np.array_equal(dmean, expect) and np.array_equal(dvar, -expect)
    with pytest.raises(ValueError):
        post.mean_and_var_with_grad(np.zeros(shape), layout=7)
