"""Python host mirror of ApproximateGPs.jl's LaplaceApproximation (/root/reference/src/LaplaceApproximationModule.jl, LA) over the
C-ABI of libsvgp_mi355x.so: Newton mode finding, approx_lml, its gradient with respect to the kernel parameters and the posterior's
predictions all run on the device (include/svgp_mi355x.h, svgp_laplace_*).  This file only packs parameters."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _ffi
from . import sva as _sva
from .gp import (BernoulliLikelihood, GammaLikelihood, GaussianLikelihood, LatentFiniteGP, LogisticLink, NormalCDFLink, _as_dn)
from .kernels import unpack_kernel


class LaplaceApproximation:
    """LaplaceApproximation(; f_init=nothing, maxiter=100)  (LA:26-29: the Newton keyword arguments)."""

    def __init__(self, f_init=None, maxiter: int = 100):
        if int(maxiter) < 1:
            raise ValueError("maxiter must be >= 1")   # LA:257 @assert maxiter >= 1
        self.f_init = None if f_init is None else np.asarray(f_init, dtype=np.float64).reshape(-1)
        self.maxiter = int(maxiter)


def _lik_code(lik):
    if type(lik) not in _sva._LIK:
        raise _ffi.UnsupportedError(f"unsupported likelihood {lik!r}")
    code, s2 = _sva._LIK[type(lik)], 1.0
    if isinstance(lik, BernoulliLikelihood):
        if isinstance(lik.invlink, NormalCDFLink):
            code = _ffi.LIK_BERNOULLI_NORMCDF
        elif not isinstance(lik.invlink, LogisticLink):
            raise _ffi.UnsupportedError(f"unsupported link {lik.invlink!r}")
    if isinstance(lik, GaussianLikelihood):
        s2 = float(lik.sigma2)
    elif isinstance(lik, GammaLikelihood):
        s2 = float(lik.alpha)
    return code, s2


def _check_inputs(lfx: LatentFiniteGP, ys):
    """_check_laplace_inputs (LA:167-178): zero prior mean, one latent function per observation."""
    fx = lfx.fx
    assert fx.f.mean_const == 0.0 and fx.f.mean_fn is None, "LaplaceApproximation needs a zero prior mean"
    if not fx.is_isotropic():
        raise _ffi.UnsupportedError("fx.Σy must be isotropic jitter")
    assert np.shape(ys)[0] == fx.n, "LaplaceApproximation does not support multi-latent likelihoods"


class DeviceLaplace:
    """A resident svgp_laplace handle over (x, y): x as lfx.fx.x - a plain vector (d = 1) or a (d, n) ColVecs array; with
    layout = ROWVECS an (n, d) RowVecs array."""

    def __init__(self, ctx: _ffi.Context, x, y, dtype, layout=None):
        self.ctx = ctx
        x = np.asarray(x)
        if layout is None:
            layout = _ffi.VEC if x.ndim == 1 else _ffi.COLVECS
        self.data = _ffi.DeviceData(ctx, x, y, dtype, layout)
        self.dtype, self.d, self.n = self.data.dtype, self.data.d, self.data.n
        h = C.c_void_p()
        ctx.check(ctx.lib.svgp_laplace_create(ctx.h, self.data.h, C.byref(h)))
        self.h = h

    def desc(self, kernel, lik, jitter, maxiter=100, warm_start=False):
        family, variance, il = unpack_kernel(kernel, self.d)
        code, s2 = _lik_code(lik)
        il = np.ascontiguousarray(il, dtype=np.float64)
        ds = _ffi.LaplaceDesc(dtype=self.dtype, kernel=family, likelihood=code, d=self.d, maxiter=int(maxiter),
                              warm_start=1 if warm_start else 0, variance=float(variance),
                              inv_lengthscale=il.ctypes.data_as(C.POINTER(C.c_double)), jitter=float(jitter), lik_sigma2=s2,
                              reserved=0)
        return ds, il

    def _finit(self, f_init):
        if f_init is None:
            return None, None
        buf = np.ascontiguousarray(np.asarray(f_init, dtype=_ffi.np_dtype(self.dtype)).reshape(-1))
        if buf.shape[0] != self.n:
            raise ValueError("f_init must have one value per observation")
        return buf, buf.ctypes.data_as(C.c_void_p)

    def fit(self, desc, f_init=None):
        """-> (lml, LaplaceInfo)"""
        keep, p = self._finit(f_init)
        lml, info = C.c_double(), _ffi.LaplaceInfo()
        self.ctx.check(self.ctx.lib.svgp_laplace_fit(self.ctx.h, self.h, C.byref(desc), p, C.byref(lml), C.byref(info)))
        return lml.value, info

    def lml_grad(self, desc, f_init=None):
        """-> (lml, d lml / d variance, d lml / d inv_lengthscale (d,), LaplaceInfo)"""
        keep, p = self._finit(f_init)
        lml, info, dv = C.c_double(), _ffi.LaplaceInfo(), C.c_double()
        dil = np.zeros(self.d)
        self.ctx.check(self.ctx.lib.svgp_laplace_lml_grad(self.ctx.h, self.h, C.byref(desc), p, C.byref(lml), C.byref(info),
                                                          C.byref(dv), dil.ctypes.data_as(C.POINTER(C.c_double))))
        return lml.value, dv.value, dil, info

    def mode(self):
        """-> (f_opt, d log p / df, W) at the last fit's mode"""
        dt = _ffi.np_dtype(self.dtype)
        f, g, w = (np.zeros(self.n, dtype=dt) for _ in range(3))
        self.ctx.check(self.ctx.lib.svgp_laplace_mode(self.ctx.h, self.h, _ffi._ptr(f), _ffi._ptr(g), _ffi._ptr(w)))
        return f, g, w

    def _x(self, x):
        dt = _ffi.np_dtype(self.dtype)
        x = np.asarray(x, dtype=dt)
        if x.ndim == 1:
            if self.d != 1:
                raise ValueError("test inputs have a different dimension than the data")
            return _ffi.VEC, x.shape[0], np.ascontiguousarray(x)
        if x.shape[0] != self.d:
            raise ValueError("test inputs have a different dimension than the data")
        return _ffi.COLVECS, x.shape[1], np.asfortranarray(x)

    def predict(self, x, mean=True, var=True, cov=False):
        layout, n, xb = self._x(x)
        dt = _ffi.np_dtype(self.dtype)
        m = np.zeros(n, dtype=dt) if mean else None
        v = np.zeros(n, dtype=dt) if var else None
        c = np.zeros((n, n), dtype=dt, order="F") if cov else None
        self.ctx.check(self.ctx.lib.svgp_laplace_predict(self.ctx.h, self.h, layout, n, _ffi._ptr(xb), _ffi._ptr(m), _ffi._ptr(v),
                                                         _ffi._ptr(c)))
        return m, v, c

    def cross_cov(self, x, y):
        lx, nx, xb = self._x(x)
        ly, ny, yb = self._x(y)
        if lx != ly:
            raise ValueError("x and y must have the same layout")
        c = np.zeros((nx, ny), dtype=_ffi.np_dtype(self.dtype), order="F")
        self.ctx.check(self.ctx.lib.svgp_laplace_predict_cross_cov(self.ctx.h, self.h, lx, nx, _ffi._ptr(xb), ny, _ffi._ptr(yb),
                                                                   _ffi._ptr(c)))
        return c

    def free(self):
        if getattr(self, "h", None):
            self.ctx.lib.svgp_laplace_free(self.ctx.h, self.h)
            self.h = None
        if getattr(self, "data", None) is not None:
            self.data.free()
            self.data = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _dtype_of(lfx, dtype):
    if dtype is not None:
        return np.dtype(dtype)
    return np.dtype(np.float32 if np.asarray(lfx.fx.x).dtype == np.float32 else np.float64)


def _fit(la: LaplaceApproximation, lfx: LatentFiniteGP, ys, ctx, dtype, grad):
    _check_inputs(lfx, ys)
    dev = DeviceLaplace(ctx or _ffi.default_context(), lfx.fx.x, ys, _dtype_of(lfx, dtype))
    desc, keep = dev.desc(lfx.fx.f.kernel, lfx.lik, float(lfx.fx.Sigma_y), la.maxiter)
    out = dev.lml_grad(desc, la.f_init) if grad else dev.fit(desc, la.f_init)
    return dev, out


def _laplace_kwargs(fn, kwargs):
    """ctx / dtype of a Laplace call; any other keyword is an error, as in the SVGP methods"""
    extra = set(kwargs) - {"ctx", "dtype"}
    if extra:
        raise TypeError(f"{fn}() with LaplaceApproximation got unexpected keyword arguments {sorted(extra)}")
    return kwargs.get("ctx"), kwargs.get("dtype")


def approx_lml(approx, lfx, ys, **kwargs):
    """approx_lml(la::LaplaceApproximation, lfx, ys; ctx, dtype) (LA:50-52 -> laplace_lml :157-165); any other approximation:
    the SVGP method (sva.approx_lml) with every keyword passed on exactly as given."""
    if not isinstance(approx, LaplaceApproximation):
        return _sva.approx_lml(approx, lfx, ys, **kwargs)
    ctx, dtype = _laplace_kwargs("approx_lml", kwargs)
    dev, (lml, _info) = _fit(approx, lfx, ys, ctx, dtype, grad=False)
    dev.free()
    return lml


def approx_lml_and_gradient(la: LaplaceApproximation, lfx: LatentFiniteGP, ys, *, ctx=None, dtype=None):
    """approx_lml and its gradient with respect to the kernel parameters, what Zygote gives the reference through the rrule of
    newton_inner_loop (LA:330-369): -> (lml, {"variance": d lml / d variance, "inv_lengthscale": d lml / d inv_lengthscale (d,)}).
    An isotropic kernel's d lml / d (1 / lengthscale) is the sum of the d entries."""
    dev, (lml, dv, dil, _info) = _fit(la, lfx, ys, ctx, dtype, grad=True)
    dev.free()
    return lml, {"variance": dv, "inv_lengthscale": dil}


class LaplacePosteriorGP:
    """ApproxPosteriorGP{<:LaplaceApproximation} (LA:39-49) with the Newton intermediates resident on the device; predictions
    RW 3.21 / 3.29 (LA:425-463).  Test inputs: a plain vector (d = 1) or a (d, n) ColVecs array."""

    def __init__(self, la: LaplaceApproximation, lfx: LatentFiniteGP, ys, ctx=None, dtype=None):
        self.approx, self.prior, self.lik = la, lfx.fx.f, lfx.lik
        self.dev, (self.lml, self.info) = _fit(la, lfx, ys, ctx, dtype, grad=False)

    def mean(self, x):
        return self.dev.predict(x, mean=True, var=False)[0]

    def var(self, x):
        return self.dev.predict(x, mean=False, var=True)[1]

    def mean_and_var(self, x):
        m, v, _ = self.dev.predict(x, mean=True, var=True)
        return m, v

    def cov(self, x, y=None):
        if y is None:
            return self.dev.predict(x, mean=False, var=False, cov=True)[2]
        return self.dev.cross_cov(x, y)

    def mean_and_cov(self, x):
        m, _, c = self.dev.predict(x, mean=True, var=False, cov=True)
        return m, c

    def mode(self):
        """(f_opt, d log p / df, W) of the cached intermediates"""
        return self.dev.mode()

    def _lik_predictive(self, x, y, quadrature, want):
        code, s2 = _lik_code(self.lik)
        m, v = self.mean_and_var(x)
        return _ffi.lik_predictive(self.dev.ctx, code, s2, _sva._quadrature_n(quadrature), m, v, y, want=want)

    def predict_y(self, x, quadrature=None):
        """(E[y*], Var[y*]) through the likelihood the approximation was fitted with: svgp_laplace_predict, then svgp_lik_predictive."""
        r = self._lik_predictive(x, None, quadrature, ("ymean", "yvar"))
        return r["ymean"], r["yvar"]

    def log_predictive_density(self, x, y, quadrature=None):
        """log p(y*_i | D) per point under the Gaussian (Laplace) latent marginals; NLPD = -mean of it."""
        return self._lik_predictive(x, y, quadrature, ("lpd",))["lpd"]


def posterior(approx, *args, **kwargs):
    """posterior(la::LaplaceApproximation, lfx, ys) (LA:39-49); any other approximation: the SVGP method (sva.posterior)."""
    if isinstance(approx, LaplaceApproximation):
        lfx, ys = args
        ctx, dtype = _laplace_kwargs("posterior", kwargs)
        return LaplacePosteriorGP(approx, lfx, ys, ctx=ctx, dtype=dtype)
    return _sva.posterior(approx, *args, **kwargs)


class LaplaceObjective:
    """build_laplace_objective(build_latent_gp, xs, ys; newton_warmstart=true, newton_maxiter=100) (LA:84-132):
    objective(*args) = -approx_lml of build_latent_gp(*args)(xs).  With newton_warmstart each Newton loop starts from the mode of
    the previous call (the reference's LaplaceObjectiveCache); the first call, and every call without it, starts from mean(fx) = 0.
    value_and_gradient(*args) -> (-lml, {"variance": -d lml / d variance, "inv_lengthscale": -d lml / d inv_lengthscale}): the
    caller chains it through its own parametrisation (build_latent_gp) by hand."""

    def __init__(self, build_latent_gp, xs, ys, newton_warmstart=True, newton_maxiter=100, ctx=None, dtype=None):
        if int(newton_maxiter) < 1:
            raise ValueError("newton_maxiter must be >= 1")
        self.build_latent_gp, self.xs, self.ys = build_latent_gp, np.asarray(xs), np.asarray(ys)
        self.warm, self.maxiter = bool(newton_warmstart), int(newton_maxiter)
        self.ctx, self.dtype = ctx, dtype
        self.dev = None
        self.last_info = None

    def _prepare(self, args):
        lfx = self.build_latent_gp(*args)(self.xs)
        _check_inputs(lfx, self.ys)
        if self.dev is None:
            self.dev = DeviceLaplace(self.ctx or _ffi.default_context(), self.xs, self.ys, _dtype_of(lfx, self.dtype))
        return self.dev.desc(lfx.fx.f.kernel, lfx.lik, float(lfx.fx.Sigma_y), self.maxiter, warm_start=self.warm)

    def __call__(self, *args):
        desc, keep = self._prepare(args)
        lml, self.last_info = self.dev.fit(desc)
        return -lml

    def value_and_gradient(self, *args):
        desc, keep = self._prepare(args)
        lml, dv, dil, self.last_info = self.dev.lml_grad(desc)
        return -lml, {"variance": -dv, "inv_lengthscale": -dil}

    def mode(self):
        """f_opt of the last call (the start of the next one under newton_warmstart): f_init of a warm-started posterior"""
        return self.dev.mode()[0]

    def free(self):
        if self.dev is not None:
            self.dev.free()
            self.dev = None


def build_laplace_objective(build_latent_gp, xs, ys, newton_warmstart=True, newton_maxiter=100, **kwargs):
    return LaplaceObjective(build_latent_gp, xs, ys, newton_warmstart=newton_warmstart, newton_maxiter=newton_maxiter, **kwargs)
