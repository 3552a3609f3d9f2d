"""The exact one-dimensional Matern GP in O(N) over the C-ABI of libsvgp_mi355x.so (include/svgp_mi355x.h, svgp_ss_*): a Matern-3/2 or
-5/2 GP over scalar inputs is a linear Gaussian state-space model, and a Kalman filter and a Rauch-Tung-Striebel smoother, run on the
device as parallel scans, give its log marginal likelihood and its posterior marginals exactly (TemporalGPs.jl's regime); joint posterior
sample paths over any grid of times (SSPosteriorGP.rand, DeviceStateSpace.sample) come from the same union of points by Matheron's rule
in state-space form, three scans of affine maps, from the caller's standard-normal draws.  This file sorts the inputs, packs parameters,
maps draws given in the caller's order to the library's and returns results in the caller's order.  Out of scope: the gradient of the
lml, sums and products of kernels, periodic kernels, non-Gaussian likelihoods, d > 1, multi-GPU."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _ffi
from . import iterative as _it
from . import nearest_neighbors as _nn
from .gp import Diagonal, FiniteGP
from .kernels import unpack_kernel


class StateSpace:
    """StateSpace(): approx_lml(StateSpace(), fx, y) and posterior(StateSpace(), fx, y) of a GP with a Matern-3/2 or Matern-5/2 kernel
    over one-dimensional inputs, exact, in O(N).  fx.Σy: a scalar > 0 or Diagonal(v); the prior mean: zero, a constant, or any other
    mean as mean_offsets= (its values at x, subtracted from y; predictions then exclude it)."""


class DeviceStateSpace:
    """A resident svgp_ss handle over the times x (any order: they are argsorted here) and y."""

    def __init__(self, ctx: _ffi.Context, x, y, dtype):
        x = np.asarray(x)
        if x.ndim == 2 and x.shape[0] == 1:
            x = x[0]
        if x.ndim != 1:
            raise _ffi.UnsupportedError("StateSpace needs one-dimensional inputs: a plain vector of times")
        dt = np.dtype(dtype)
        x = x.astype(dt)
        if not np.all(np.isfinite(x)):
            raise ValueError("the times must be finite")
        self.ctx, self.dtype, self.n = ctx, _ffi.dtype_code(dt), x.shape[0]
        self.state_dim = None   # D of the last successful fit: the width of sample()'s draws
        self.order = np.argsort(x, kind="stable")
        y = None if y is None else np.asarray(y, dtype=dt).reshape(-1)[self.order]
        self.data = _ffi.DeviceData(ctx, np.ascontiguousarray(x[self.order]), y, dt, _ffi.VEC)
        h = C.c_void_p()
        try:
            ctx.check(ctx.lib.svgp_ss_create(ctx.h, self.data.h, C.byref(h)))
        except Exception:
            self.data.free()
            raise
        self.h = h

    def desc(self, kernel, diag, mean_const=0.0):
        family, variance, il = unpack_kernel(kernel, 1)
        return _ffi.SSDesc(dtype=self.dtype, kernel=family, variance=float(variance), inv_lengthscale=float(il[0]), diag=float(diag),
                           mean_const=float(mean_const), reserved=0)

    def _check(self, rc):
        if rc == _ffi.NOT_POSDEF:
            raise _ffi.PosDefException(-1, (self.ctx.lib.svgp_last_error(self.ctx.h) or b"").decode())
        self.ctx.check(rc)

    def set_noise(self, s=None):
        """Per-point noise variances sigma_k^2 = diag + s_k, s in the caller's order; None removes them."""
        self.state_dim = None   # the library drops the cached fit
        if s is None:
            self.ctx.check(self.ctx.lib.svgp_ss_set_noise(self.ctx.h, self.h, None))
            return
        s = np.asarray(s, dtype=np.float64).reshape(-1)
        if s.shape != (self.n,):
            raise ValueError("noise: one entry per point")
        pn, keep = _ffi.point_noise(s[self.order], self.n, self.dtype)
        self.ctx.check(self.ctx.lib.svgp_ss_set_noise(self.ctx.h, self.h, C.byref(pn)))

    def fit(self, desc, delta=None):
        """-> (lml, SSInfo); delta: y - mean(x) in the caller's order, or None for y - mean_const"""
        dl = None
        if delta is not None:
            dl = np.asarray(delta, dtype=np.float64).reshape(-1)
            if dl.shape != (self.n,):
                raise ValueError("delta: an (N,) array")
            dl = np.ascontiguousarray(dl[self.order])
        lml, info = C.c_double(), _ffi.SSInfo()
        self.state_dim = None
        self._check(self.ctx.lib.svgp_ss_fit(self.ctx.h, self.h, C.byref(desc), None if dl is None else dl.ctypes.data_as(C.POINTER(C.c_double)),
                                             C.byref(lml), C.byref(info)))
        self.state_dim = int(info.state_dim)
        return lml.value, info

    def predict(self, t, mean=True, var=True):
        """-> (latent mean, latent variance) at the times t, in t's order"""
        dt = _ffi.np_dtype(self.dtype)
        t = np.asarray(t, dtype=dt).reshape(-1)
        if t.shape[0] < 1:
            raise ValueError("no test points")
        order = np.argsort(t, kind="stable")
        ts = np.ascontiguousarray(t[order])
        m = np.zeros(t.shape[0], dtype=dt) if mean else None
        v = np.zeros(t.shape[0], dtype=dt) if var else None
        self._check(self.ctx.lib.svgp_ss_predict(self.ctx.h, self.h, t.shape[0], _ffi._ptr(ts), _ffi._ptr(m), _ffi._ptr(v)))
        back = np.empty_like(order)
        back[order] = np.arange(order.shape[0])
        return (None if m is None else m[back]), (None if v is None else v[back])

    def sample(self, t, z, eps):
        """-> (n, S) joint posterior sample paths at the times t, in t's order: a deterministic, affine function of the caller's
        standard-normal draws z (S, N + n, D) and eps (S, N).  Draws are addressed in the CALLER's order: z[:, i] belongs to the
        i-th point of x as given, z[:, N + j] to t[j], eps[:, i] to the noise of y[i].  D: the state dimension of the last fit."""
        dt = _ffi.np_dtype(self.dtype)
        t = np.asarray(t, dtype=dt).reshape(-1)
        n = t.shape[0]
        if n < 1:
            raise ValueError("no test points")
        if self.state_dim is None:
            raise ValueError("sample needs a successful fit on this handle")
        z, eps = np.asarray(z, dtype=np.float64), np.asarray(eps, dtype=np.float64)
        if z.ndim != 3 or z.shape[0] < 1 or z.shape[1:] != (self.n + n, self.state_dim):
            raise ValueError(f"z: an (S, N + n, D) = (S, {self.n + n}, {self.state_dim}) array of standard-normal draws, S >= 1")
        S = z.shape[0]
        if eps.shape != (S, self.n):
            raise ValueError(f"eps: an (S, N) = ({S}, {self.n}) array of standard-normal draws")
        order = np.argsort(t, kind="stable")
        ts = np.ascontiguousarray(t[order])
        zc = np.ascontiguousarray(z[:, np.concatenate([self.order, self.n + order])])
        ec = np.ascontiguousarray(eps[:, self.order])
        out = np.zeros((S, n), dtype=dt)
        self._check(self.ctx.lib.svgp_ss_sample(self.ctx.h, self.h, n, _ffi._ptr(ts), S, _ffi._ptr(zc), _ffi._ptr(ec), _ffi._ptr(out)))
        back = np.empty_like(order)
        back[order] = np.arange(n)
        return np.ascontiguousarray(out[:, back].T)

    def free(self):
        if getattr(self, "h", None):
            self.ctx.lib.svgp_ss_free(self.ctx.h, self.h)
            self.h = None
        if getattr(self, "data", None) is not None:
            self.data.free()
            self.data = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _kwargs(fn, kwargs):
    extra = set(kwargs) - {"ctx", "dtype", "mean_offsets"}
    if extra:
        raise TypeError(f"{fn}() with StateSpace got unexpected keyword arguments {sorted(extra)}")
    return kwargs.get("ctx"), kwargs.get("dtype"), kwargs.get("mean_offsets")


def _device(fx: FiniteGP, y, ctx, dtype, mean_offsets):
    """-> (DeviceStateSpace, desc, delta or None), every check before the GPU is touched"""
    if not isinstance(fx, FiniteGP):
        raise TypeError("StateSpace takes fx = f(x, Σy)")
    if fx.f.mean_fn is not None:
        raise _ffi.UnsupportedError("StateSpace takes a zero or constant prior mean; pass any other mean's values at x as mean_offsets=")
    family, _, _ = unpack_kernel(fx.f.kernel, 1)
    if family not in (_ffi.KERNEL_MATERN32, _ffi.KERNEL_MATERN52):
        raise _ffi.UnsupportedError("StateSpace needs a Matern32Kernel or Matern52Kernel (the squared exponential has no finite state)")
    s = None
    if isinstance(fx.Sigma_y, Diagonal):
        sy = np.asarray(fx.Sigma_y.diag, dtype=np.float64)
        if sy.shape != (fx.n,) or not np.all(sy > 0.0):
            raise ValueError("fx.Σy = Diagonal(v) needs one variance > 0 per point")
        diag = float(sy.min())
        s = sy - diag
    elif not fx.is_isotropic():
        raise _ffi.UnsupportedError("StateSpace needs an isotropic fx.Σy or fx = f(x, Diagonal(v))")
    else:
        diag = float(fx.Sigma_y)
        if not diag > 0:
            raise ValueError("StateSpace needs observation noise fx.Σy > 0")
    if np.shape(y)[0] != fx.n:
        raise ValueError("x and y lengths differ")
    delta = None
    if mean_offsets is not None:
        mo = np.asarray(mean_offsets, dtype=np.float64).reshape(-1)
        if mo.shape != (fx.n,):
            raise ValueError("mean_offsets: one value per point")
        delta = np.asarray(y, dtype=np.float64).reshape(-1) - float(fx.f.mean_const) - mo
    dev = DeviceStateSpace(ctx or _ffi.default_context(), fx.x, y, _nn._dtype_of(fx, dtype))
    try:
        if s is not None:
            dev.set_noise(s)
        return dev, dev.desc(fx.f.kernel, diag, fx.f.mean_const), delta
    except Exception:
        dev.free()
        raise


def approx_lml(approx, fx, y, **kwargs):
    """approx_lml(StateSpace(), fx, y; ctx, dtype, mean_offsets): logpdf(fx, y), exact (approxgp.approx_lml dispatches here); any other
    approximation: the existing methods."""
    if not isinstance(approx, StateSpace):
        return _it.approx_lml(approx, fx, y, **kwargs)
    dev, desc, delta = _device(fx, y, *_kwargs("approx_lml", kwargs))
    try:
        return dev.fit(desc, delta)[0]
    finally:
        dev.free()


class SSPosteriorGP:
    """posterior(StateSpace(), fx, y): the exact posterior's marginals and joint sample paths at any times, each call one filter pass
    and one smoother pass (rand: three scans of sample chunks) over the union of the data and the test times on the device."""

    def __init__(self, fx: FiniteGP, y, ctx=None, dtype=None, mean_offsets=None):
        self.prior = fx.f
        self.dev, self._desc, delta = _device(fx, y, ctx, dtype, mean_offsets)
        self.noise = None if isinstance(fx.Sigma_y, Diagonal) else float(fx.Sigma_y)
        try:
            self.lml, self.info = self.dev.fit(self._desc, delta)
        except Exception:
            self.dev.free()
            raise

    def mean(self, x):
        return self.dev.predict(x, mean=True, var=False)[0]

    def var(self, x):
        return self.dev.predict(x, mean=False, var=True)[1]

    def mean_and_var(self, x):
        return self.dev.predict(x)

    def rand(self, x, n_samples, rng=None):
        """-> (n, n_samples): joint draws of the latent function at the times x (any order), exact in distribution and O((N + n) S);
        rng: a seed or a numpy Generator (np.random.default_rng(rng) draws z, then eps)"""
        n = np.asarray(x).reshape(-1).shape[0]
        if int(n_samples) != n_samples or n_samples < 1:
            raise ValueError("n_samples: an integer >= 1")
        if n < 1:
            raise ValueError("no test points")
        g = np.random.default_rng(rng)
        z = g.standard_normal((int(n_samples), self.dev.n + n, self.info.state_dim))
        return self.dev.sample(x, z, g.standard_normal((int(n_samples), self.dev.n)))

    def _lik_predictive(self, x, y, want, noise):
        if noise is None:
            if self.noise is None:
                raise ValueError("the posterior has per-point noise fx.Σy = Diagonal(v): pass noise=, the test points' noise variance")
            noise = self.noise
        if np.ndim(noise) != 0 or not float(noise) > 0:
            raise ValueError("noise: one variance > 0")
        m, v = self.mean_and_var(x)
        return _ffi.lik_predictive(self.dev.ctx, _ffi.LIK_GAUSSIAN, float(noise), 0, m, v, y, want=want)

    def predict_y(self, x, noise=None):
        """(E[y*], Var[y*]) = (mean, var + noise); noise: the posterior's own fx.Σy by default"""
        r = self._lik_predictive(x, None, ("ymean", "yvar"), noise)
        return r["ymean"], r["yvar"]

    def log_predictive_density(self, x, y, noise=None):
        """log N(y*_i; mean_i, var_i + noise) per point"""
        return self._lik_predictive(x, y, ("lpd",), noise)["lpd"]

    def free(self):
        self.dev.free()


def posterior(approx, *args, **kwargs):
    """posterior(StateSpace(), fx, y; ctx, dtype, mean_offsets) -> SSPosteriorGP; any other approximation: the existing methods."""
    if not isinstance(approx, StateSpace):
        return _it.posterior(approx, *args, **kwargs)
    fx, y = args
    ctx, dtype, mo = _kwargs("posterior", kwargs)
    return SSPosteriorGP(fx, y, ctx=ctx, dtype=dtype, mean_offsets=mo)
