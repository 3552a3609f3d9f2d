"""Python host mirror of ApproximateGPs.jl's NearestNeighbors (Vecchia) approximation (src/NearestNeighborsModule.jl of the reference,
NN) over the C-ABI of libsvgp_mi355x.so: the per-point factorisations, approx_lml, its gradient and the posterior's predictions all
run on the device (include/svgp_mi355x.h, svgp_nn_*).  This file only packs parameters."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _ffi
from . import laplace as _laplace
from .gp import Diagonal, FiniteGP
from .kernels import unpack_kernel


class NearestNeighbors:
    """NearestNeighbors(k) (NN:73-75): every point is conditioned on the k points before it in the given order.
    include_noise=False is the reference, which builds U from the kernel alone and ignores fx.Σy (NN:100-101); with
    include_noise=True the isotropic fx.Σy joins every diagonal entry: the Vecchia approximation of logpdf(fx, y) itself; per-point
    noise variances v are fx = f(x, Diagonal(v)) (every v > 0: diag = min(v) and s = v - min(v) on the device).
    neighbors: None is the reference's window of the previous k points; "nearest" conditions every point on its k nearest
    predecessors, found on the device with the kernel's inverse lengthscales as the metric; an (n, min(k, n - 1)) integer array is
    the caller's own table (row i: distinct indices below i, the valid ones first, -1 after them).  Gradients are taken at the
    fixed table."""

    def __init__(self, k: int, include_noise: bool = False, neighbors=None):
        if int(k) != k or int(k) < 1:
            raise ValueError("NearestNeighbors needs k >= 1")
        self.k = int(k)
        self.include_noise = bool(include_noise)
        if isinstance(neighbors, str):
            if neighbors != "nearest":
                raise ValueError('neighbors is None, "nearest" or an integer array')
        elif neighbors is not None:
            neighbors = np.asarray(neighbors)
            if neighbors.ndim != 2 or not np.issubdtype(neighbors.dtype, np.integer):
                raise ValueError('neighbors is None, "nearest" or an (n, min(k, n - 1)) integer array')
        self.neighbors = neighbors


def _check_inputs(nn: NearestNeighbors, fx: FiniteGP, y, mean_offsets=None):
    """-> (diag, mean_const, s or None, mu or None), before the GPU is touched.  A CustomMean prior is not supported: the values of a
    mean function at x enter as mean_offsets= ((n,), added to the constant).  With include_noise Σy is isotropic or Diagonal(v):
    diag = min(v) and the per-point variances s = v - min(v) above it (vfe.py's mapping)."""
    if fx.f.mean_fn is not None:
        raise _ffi.UnsupportedError("NearestNeighbors takes a zero or constant prior mean, not a CustomMean: pass the mean's values "
                                    "at x as mean_offsets= (an (n,) array, added to the constant)")
    diag, s = 0.0, None
    if nn.include_noise:
        if isinstance(fx.Sigma_y, Diagonal):
            sy = np.asarray(fx.Sigma_y.diag, dtype=np.float64)
            if sy.ndim != 1 or sy.shape[0] != fx.n:
                raise ValueError(f"fx.Σy = Diagonal(v) needs a vector with one variance per point ({fx.n}); got shape {sy.shape}")
            if not np.all((sy > 0.0) & np.isfinite(sy)):   # (NaN included)
                raise ValueError("fx.Σy must be positive: every per-point noise variance must be > 0 and finite")
            diag = float(sy.min())
            s = sy - diag
        elif not fx.is_isotropic():
            raise _ffi.UnsupportedError("include_noise needs an isotropic fx.Σy, or per-point noise variances v as "
                                        "fx = f(x, Diagonal(v))")
        else:
            diag = float(fx.Sigma_y)
    if np.shape(y)[0] != fx.n:
        raise ValueError("x and y lengths differ")
    mu = None
    if mean_offsets is not None:
        mu = np.asarray(mean_offsets, dtype=np.float64)
        if mu.shape != (fx.n,):
            raise ValueError(f"mean_offsets: one value per point ({fx.n}); got shape {mu.shape}")
    return diag, float(fx.f.mean_const), s, mu


def _flag(name, v):
    if not isinstance(v, (bool, np.bool_)):
        raise ValueError(f"{name} is True or False")
    return bool(v)


class DeviceNearestNeighbors:
    """A resident svgp_nn handle over (x, y): x a plain vector (d = 1) or a (d, n) ColVecs array; with layout = ROWVECS an (n, d)
    RowVecs array.  The neighbours of a point are the points before it in this order."""

    def __init__(self, ctx: _ffi.Context, x, y, dtype, layout=None):
        self.ctx = ctx
        x = np.asarray(x)
        if layout is None:
            layout = _ffi.VEC if x.ndim == 1 else _ffi.COLVECS
        self.data = _ffi.DeviceData(ctx, x, y, dtype, layout)
        self.dtype, self.d, self.n = self.data.dtype, self.data.d, self.data.n
        h = C.c_void_p()
        ctx.check(ctx.lib.svgp_nn_create(ctx.h, self.data.h, C.byref(h)))
        self.h = h
        self.kb = None   # columns of B after a fit

    def desc(self, kernel, k, diag=0.0, mean_const=0.0):
        family, variance, il = unpack_kernel(kernel, self.d)
        il = np.ascontiguousarray(il, dtype=np.float64)
        ds = _ffi.NNDesc(dtype=self.dtype, kernel=family, d=self.d, k=int(k), variance=float(variance),
                         inv_lengthscale=il.ctypes.data_as(C.POINTER(C.c_double)), diag=float(diag), mean_const=float(mean_const),
                         reserved=0)
        return ds, il

    def _check(self, rc, info):
        if rc == _ffi.NOT_POSDEF:
            msg = (self.ctx.lib.svgp_last_error(self.ctx.h) or b"").decode()
            raise _ffi.PosDefException(int(info.first_bad), msg)
        self.ctx.check(rc)

    def lml(self, desc):
        """-> (lml, NNInfo)"""
        lml, info = C.c_double(), _ffi.NNInfo()
        self._check(self.ctx.lib.svgp_nn_lml(self.ctx.h, self.h, C.byref(desc), C.byref(lml), C.byref(info)), info)
        return lml.value, info

    def lml_grad(self, desc):
        """-> (lml, d / d variance, d / d inv_lengthscale (d,), d / d diag, NNInfo)"""
        lml, info, dv, dd = C.c_double(), _ffi.NNInfo(), C.c_double(), C.c_double()
        dil = np.zeros(self.d)
        self._check(self.ctx.lib.svgp_nn_lml_grad(self.ctx.h, self.h, C.byref(desc), C.byref(lml), C.byref(info), C.byref(dv),
                                                  dil.ctypes.data_as(C.POINTER(C.c_double)), C.byref(dd)), info)
        return lml.value, dv.value, dil, dd.value, info

    def fit(self, desc):
        """-> (lml, NNInfo); caches B, F and alpha on the device for predict / cross_cov / factors"""
        lml, info = C.c_double(), _ffi.NNInfo()
        self._check(self.ctx.lib.svgp_nn_fit(self.ctx.h, self.h, C.byref(desc), C.byref(lml), C.byref(info)), info)
        self.kb = min(int(desc.k), self.n - 1)
        return lml.value, info

    def set_noise(self, s):
        """per-point noise variances above the descriptor's diag (sigma_j^2 = diag + s_j): an (n,) numpy array or a contiguous device
        tensor of the data dtype, copied into the handle; None removes them.  Discards the fit."""
        self.kb = None
        if s is None:
            self.ctx.check(self.ctx.lib.svgp_nn_set_noise(self.ctx.h, self.h, None))
            return
        pn, _keep = _ffi.point_noise(s, self.n, self.dtype)
        self.ctx.check(self.ctx.lib.svgp_nn_set_noise(self.ctx.h, self.h, C.byref(pn)))

    def set_mean(self, mu):
        """per-point prior-mean offsets (delta_j = y_j - mean_const - mu_j), as set_noise"""
        self.kb = None
        if mu is None:
            self.ctx.check(self.ctx.lib.svgp_nn_set_mean(self.ctx.h, self.h, None))
            return
        pm, _keep = _ffi.point_mean(mu, self.n, self.dtype)
        self.ctx.check(self.ctx.lib.svgp_nn_set_mean(self.ctx.h, self.h, C.byref(pm)))

    def lml_grad_points(self, desc, mean_grad_out=None, noise_grad_out=None):
        """-> (lml, {"variance", "inv_lengthscale" (d,), "diag", "mean_const", "mean" (n,), "noise" (n,)}, NNInfo): lml_grad's blocks,
        d / d mean_const, d lml / d mu_j and d lml / d sigma_j^2.  mean_grad_out / noise_grad_out: contiguous device tensors of
        the data dtype that receive the two vectors in place of host arrays.  Leaves the handle fitted at desc, as fit does."""
        dt = _ffi.np_dtype(self.dtype)
        outs, structs = {}, {}
        for name, dst, cls in (("mean", mean_grad_out, _ffi.PointMeanGrad), ("noise", noise_grad_out, _ffi.PointNoiseGrad)):
            if dst is None:
                outs[name] = np.zeros(self.n, dtype=dt)
                structs[name] = cls(_ffi._ptr(outs[name]), 0, 0)
            else:
                if not hasattr(dst, "data_ptr"):
                    raise ValueError(f"{name}_grad_out: a contiguous device tensor of the data dtype with one entry per point")
                outs[name] = dst
                structs[name] = cls(C.c_void_p(_ffi.point_mean_grad_ptr(dst, self.n, self.dtype)), 1, 0)
        lml, info, dv, dd, dm = C.c_double(), _ffi.NNInfo(), C.c_double(), C.c_double(), C.c_double()
        dil = np.zeros(self.d)
        self.kb = None
        self._check(self.ctx.lib.svgp_nn_lml_grad_points(self.ctx.h, self.h, C.byref(desc), C.byref(lml), C.byref(info), C.byref(dv),
                                                         dil.ctypes.data_as(C.POINTER(C.c_double)), C.byref(dd), C.byref(dm),
                                                         C.byref(structs["mean"]), C.byref(structs["noise"])), info)
        self.kb = min(int(desc.k), self.n - 1)
        return lml.value, {"variance": dv.value, "inv_lengthscale": dil, "diag": dd.value, "mean_const": dm.value,
                           "mean": outs["mean"], "noise": outs["noise"]}, info

    def set_neighbors(self, table):
        """condition point i on the points table[i, :] ((n, kb) integers: distinct indices below i, the valid ones first, -1 after
        them); k of the descriptors that follow must give kb = min(k, n - 1)"""
        table = np.asarray(table)
        if table.ndim != 2 or table.shape[0] != self.n or not np.issubdtype(table.dtype, np.integer):
            raise ValueError("the neighbour table is an (n, kb) integer array")
        kb = table.shape[1]
        if kb != min(max(kb, 1), self.n - 1):
            raise ValueError("the neighbour table has min(k, n - 1) columns, k >= 1")
        t32 = np.asfortranarray(table, dtype=np.int32)
        self.kb = None
        self.ctx.check(self.ctx.lib.svgp_nn_set_neighbors(self.ctx.h, self.h, max(kb, 1), t32.ctypes.data_as(C.POINTER(C.c_int32))))

    def build_neighbors(self, k, inv_lengthscale=None):
        """the k nearest predecessors of every point under the metric inv_lengthscale ((d,), None: ones), found on the device"""
        il = None
        if inv_lengthscale is not None:
            il = np.ascontiguousarray(np.broadcast_to(np.asarray(inv_lengthscale, dtype=np.float64), (self.d,)))
        self.kb = None
        self.ctx.check(self.ctx.lib.svgp_nn_build_neighbors(self.ctx.h, self.h, int(k),
                                                            il.ctypes.data_as(C.POINTER(C.c_double)) if il is not None else None))

    def neighbors(self):
        """-> the handle's (n, kb) int32 table, None when it conditions on the window"""
        kb = C.c_int32(-1)
        self.ctx.check(self.ctx.lib.svgp_nn_get_neighbors(self.ctx.h, self.h, C.byref(kb), None))
        if kb.value < 0:
            return None
        table = np.zeros((self.n, kb.value), dtype=np.int32, order="F")
        if kb.value:
            self.ctx.check(self.ctx.lib.svgp_nn_get_neighbors(self.ctx.h, self.h, C.byref(kb), table.ctypes.data_as(C.POINTER(C.c_int32))))
        return table

    def clear_neighbors(self):
        self.kb = None
        self.ctx.check(self.ctx.lib.svgp_nn_clear_neighbors(self.ctx.h, self.h))

    def factors(self):
        """-> (B (n, kb) with B[i, t] the coefficient of point i on point i - kb + t (with a neighbour table: on point table[i, t]),
        F (n,), alpha (n,)) of the last fit"""
        dt = _ffi.np_dtype(self.dtype)
        kb = self.kb or 0
        B = np.zeros((self.n, kb), dtype=dt, order="F")
        F, alpha = np.zeros(self.n, dtype=dt), np.zeros(self.n, dtype=dt)
        self.ctx.check(self.ctx.lib.svgp_nn_factors(self.ctx.h, self.h, _ffi._ptr(B) if kb else None, _ffi._ptr(F), _ffi._ptr(alpha)))
        return B, F, alpha

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
        self.ctx.check(self.ctx.lib.svgp_nn_predict(self.ctx.h, self.h, layout, n, _ffi._ptr(xb), _ffi._ptr(m), _ffi._ptr(v),
                                                    _ffi._ptr(c)))
        return m, v, c

    def predict_local(self, x, k, neighbors=False, layout=None):
        """nearest-neighbour kriging: every test point conditioned on its min(k, n) nearest training points under the fit's inverse
        lengthscales -> (mean, var), with neighbors=True (mean, var, table): the (n*, min(k, n)) int32 table of those points, a
        short row ending in -1.  x as for predict; with layout = ROWVECS an (n*, d) RowVecs array.  A test point whose block is not
        positive raises PosDefException(its 1-based index) carrying .mean and .var: NaN there, every other point as computed."""
        dt = _ffi.np_dtype(self.dtype)
        if layout == _ffi.ROWVECS:
            xb = np.asfortranarray(np.asarray(x, dtype=dt))
            if xb.ndim != 2 or xb.shape[1] != self.d:
                raise ValueError("test inputs have a different dimension than the data")
            n, finite = xb.shape[0], np.isfinite(xb).all(axis=1)
        else:
            layout, n, xb = self._x(x)
            finite = np.isfinite(xb) if xb.ndim == 1 else np.isfinite(xb).all(axis=0)
        m, v = np.zeros(n, dtype=dt), np.zeros(n, dtype=dt)
        table = np.zeros((n, min(int(k), self.n)), dtype=np.int32, order="F") if neighbors and int(k) >= 1 else None
        rc = self.ctx.lib.svgp_nn_predict_local(self.ctx.h, self.h, layout, n, _ffi._ptr(xb), int(k), _ffi._ptr(m), _ffi._ptr(v),
                                                table.ctypes.data_as(C.POINTER(C.c_int32)) if table is not None else None)
        if rc == _ffi.NOT_POSDEF:
            msg = (self.ctx.lib.svgp_last_error(self.ctx.h) or b"").decode()
            bad = np.flatnonzero(np.isnan(m) & finite)   # a test point that is not finite is NaN too, and no error
            err = _ffi.PosDefException(int(bad[0]) + 1 if len(bad) else 0, msg)
            err.mean, err.var = m, v
            raise err
        self.ctx.check(rc)
        return (m, v, table) if neighbors else (m, v)

    def cross_cov(self, x, y):
        lx, nx, xb = self._x(x)
        ly, ny, yb = self._x(y)
        if lx != ly:
            raise ValueError("x and y must have the same layout")
        c = np.zeros((nx, ny), dtype=_ffi.np_dtype(self.dtype), order="F")
        self.ctx.check(self.ctx.lib.svgp_nn_predict_cross_cov(self.ctx.h, self.h, lx, nx, _ffi._ptr(xb), ny, _ffi._ptr(yb),
                                                              _ffi._ptr(c)))
        return c

    def free(self):
        if getattr(self, "h", None):
            self.ctx.lib.svgp_nn_free(self.ctx.h, self.h)
            self.h = None
        if getattr(self, "data", None) is not None:
            self.data.free()
            self.data = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _dtype_of(fx, dtype):
    if dtype is not None:
        return np.dtype(dtype)
    return np.dtype(np.float32 if np.asarray(fx.x).dtype == np.float32 else np.float64)


def _nn_kwargs(fn, kwargs, more=()):
    extra = set(kwargs) - {"ctx", "dtype"} - set(more)
    if extra:
        raise TypeError(f"{fn}() with NearestNeighbors got unexpected keyword arguments {sorted(extra)}")
    return kwargs.get("ctx"), kwargs.get("dtype")


def _device(nn: NearestNeighbors, fx: FiniteGP, y, ctx, dtype, mean_offsets=None):
    diag, mean_const, s, mu = _check_inputs(nn, fx, y, mean_offsets)   # before the GPU is touched
    dev = DeviceNearestNeighbors(ctx or _ffi.default_context(), fx.x, y, _dtype_of(fx, dtype))
    desc, keep = dev.desc(fx.f.kernel, nn.k, diag, mean_const)
    try:
        if isinstance(nn.neighbors, str):
            dev.build_neighbors(nn.k, keep)
        elif nn.neighbors is not None:
            dev.set_neighbors(nn.neighbors)
        if s is not None:
            dev.set_noise(s)
        if mu is not None:
            dev.set_mean(mu)
    except Exception:
        dev.free()
        raise
    return dev, desc, keep


def approx_lml(approx, fx, y, **kwargs):
    """approx_lml(nn::NearestNeighbors, fx, y; ctx, dtype, mean_offsets) (NN:108-113); any other approximation: the Laplace / SVGP
    methods with every keyword passed on exactly as given.  mean_offsets: the values of a prior mean function at x, (n,)."""
    if not isinstance(approx, NearestNeighbors):
        return _laplace.approx_lml(approx, fx, y, **kwargs)
    ctx, dtype = _nn_kwargs("approx_lml", kwargs, ("mean_offsets",))
    dev, desc, keep = _device(approx, fx, y, ctx, dtype, kwargs.get("mean_offsets"))
    try:
        return dev.lml(desc)[0]
    finally:
        dev.free()


def approx_lml_and_gradient(approx, fx, y, **kwargs):
    """NearestNeighbors: -> (lml, {"variance", "inv_lengthscale" (d,), "diag"}), the gradient with respect to the kernel parameters
    and to the diagonal term (the noise variance under include_noise).  wrt_noise=True adds "Sigma_y" (n,), d lml / d of every
    point's noise variance ("diag" is its sum); wrt_mean=True adds "mean" (n,), d lml / d of the prior mean's value at every point,
    and "mean_const", their sum.  noise_grad_out / mean_grad_out: contiguous device tensors of the data dtype that receive the two
    vectors in place of host arrays.  mean_offsets as in approx_lml.  LaplaceApproximation: the Laplace method, unchanged."""
    if not isinstance(approx, NearestNeighbors):
        return _laplace.approx_lml_and_gradient(approx, fx, y, **kwargs)
    ctx, dtype = _nn_kwargs("approx_lml_and_gradient", kwargs, ("mean_offsets", "wrt_noise", "wrt_mean", "noise_grad_out", "mean_grad_out"))
    wrt_noise, wrt_mean = _flag("wrt_noise", kwargs.get("wrt_noise", False)), _flag("wrt_mean", kwargs.get("wrt_mean", False))
    ngo, mgo = kwargs.get("noise_grad_out"), kwargs.get("mean_grad_out")
    if ngo is not None and not wrt_noise:
        raise ValueError("noise_grad_out needs wrt_noise=True")
    if mgo is not None and not wrt_mean:
        raise ValueError("mean_grad_out needs wrt_mean=True")
    dev, desc, keep = _device(approx, fx, y, ctx, dtype, kwargs.get("mean_offsets"))
    try:
        if not (wrt_noise or wrt_mean):
            lml, dv, dil, dd, _info = dev.lml_grad(desc)
            return lml, {"variance": dv, "inv_lengthscale": dil, "diag": dd}
        lml, g, _info = dev.lml_grad_points(desc, mean_grad_out=mgo, noise_grad_out=ngo)
    finally:
        dev.free()
    grads = {"variance": g["variance"], "inv_lengthscale": g["inv_lengthscale"], "diag": g["diag"]}
    if wrt_noise:
        grads["Sigma_y"] = g["noise"]
    if wrt_mean:
        grads["mean"], grads["mean_const"] = g["mean"], g["mean_const"]
    return lml, grads


class NNPosteriorGP:
    """PosteriorGP(fx.f, (α, C = InvRoot(U), x, δ)) (NN:97-106) with B, F and α resident on the device.  Test inputs: a plain
    vector (d = 1) or a (d, n) ColVecs array."""

    def __init__(self, nn: NearestNeighbors, fx: FiniteGP, y, ctx=None, dtype=None, mean_offsets=None):
        self.approx, self.prior = nn, fx.f
        if nn.include_noise and isinstance(fx.Sigma_y, Diagonal):
            self.noise = None   # per-point noise: no single value for y*
        elif not fx.is_isotropic():
            raise _ffi.UnsupportedError("fx.Σy must be isotropic noise, or with include_noise=True per-point variances Diagonal(v)")
        else:
            self.noise = float(fx.Sigma_y)
        self.dev, desc, keep = _device(nn, fx, y, ctx, dtype, mean_offsets)
        self.lml, self.info = self.dev.fit(desc)

    @staticmethod
    def _offset(m, mean_offsets):
        """a mean function's values at the test points, added on the host"""
        if mean_offsets is None:
            return m
        mo = np.asarray(mean_offsets, dtype=m.dtype)
        if mo.shape != m.shape:
            raise ValueError(f"mean_offsets: one value per test point ({m.shape[0]}); got shape {mo.shape}")
        return m + mo

    def mean(self, x, mean_offsets=None):
        return self._offset(self.dev.predict(x, mean=True, var=False)[0], mean_offsets)

    def var(self, x):
        return self.dev.predict(x, mean=False, var=True)[1]

    def mean_and_var(self, x, mean_offsets=None):
        m, v, _ = self.dev.predict(x, mean=True, var=True)
        return self._offset(m, mean_offsets), v

    def cov(self, x, y=None):
        if y is None:
            return self.dev.predict(x, mean=False, var=False, cov=True)[2]
        return self.dev.cross_cov(x, y)

    def mean_and_cov(self, x):
        m, _, c = self.dev.predict(x, mean=True, var=False, cov=True)
        return m, c

    def factors(self):
        return self.dev.factors()

    def _lik_predictive(self, x, y, want, noise=None):
        """the Gaussian observation model y = f + N(0, noise) on the latent predictions, through the array form the SVGP and Laplace
        posteriors share (svgp_lik_predictive): one definition of the three.  noise: the test points' observation noise variance, a
        scalar or (n,); the posterior's own fx.Σy by default, which a per-point-noise posterior does not have."""
        if noise is None:
            if self.noise is None:
                raise ValueError("the posterior has per-point noise fx.Σy = Diagonal(v): pass noise=, the observation noise variance of "
                                 "the test points (a scalar or an (n,) array)")
            if not self.noise > 0:
                raise ValueError("predictions of y need observation noise fx.Σy > 0")
            m, v = self.mean_and_var(x)
            return _ffi.lik_predictive(self.dev.ctx, _ffi.LIK_GAUSSIAN, self.noise, 0, m, v, y, want=want)
        nv = np.asarray(noise, dtype=np.float64)
        xa = np.asarray(x)
        n = xa.shape[0] if xa.ndim == 1 else xa.shape[-1]
        if nv.ndim > 1 or (nv.ndim == 1 and nv.shape[0] != n):
            raise ValueError("noise: a scalar or one variance per test point")
        if not np.all(nv > 0):
            raise ValueError("predictions of y need observation noise > 0")
        m, v = self.mean_and_var(x)
        if nv.ndim == 0:
            return _ffi.lik_predictive(self.dev.ctx, _ffi.LIK_GAUSSIAN, float(nv), 0, m, v, y, want=want)
        # one variance per test point: the Gaussian closed forms, O(n) on the host in fp64
        m64, yv = np.asarray(m, dtype=np.float64), np.asarray(v, dtype=np.float64) + nv
        out = {"ymean": m64, "yvar": yv}
        if y is not None:
            yy = np.asarray(y, dtype=np.float64).reshape(-1)
            if yy.shape != (n,):
                raise ValueError("y: one observation per test point")
            out["lpd"] = -0.5 * (np.log(2.0 * np.pi * yv) + (yy - m64) ** 2 / yv)
        return {k: out[k] for k in want}

    def predict_y(self, x, noise=None):
        """(E[y*], Var[y*]) = (mean, var + noise)"""
        r = self._lik_predictive(x, None, ("ymean", "yvar"), noise)
        return r["ymean"], r["yvar"]

    def log_predictive_density(self, x, y, noise=None):
        """log N(y*_i; mean_i, var_i + noise_i) per point"""
        return self._lik_predictive(x, y, ("lpd",), noise)["lpd"]

    def local_mean_and_var(self, x, k=None, mean_offsets=None):
        """nearest-neighbour kriging (GpGp `predictions`): every test point conditioned on its k nearest observed points, k
        defaulting to the approximation's; the latent mean and variance, test points independent of each other.  The blocks carry
        the posterior's per-point noise variances and mean offsets."""
        m, v = self.dev.predict_local(x, self.approx.k if k is None else k)
        return self._offset(m, mean_offsets), v

    def local_mean(self, x, k=None, mean_offsets=None):
        return self.local_mean_and_var(x, k, mean_offsets)[0]

    def local_var(self, x, k=None):
        return self.local_mean_and_var(x, k)[1]


def posterior(approx, *args, **kwargs):
    """posterior(nn::NearestNeighbors, fx, y) (NN:97-106); any other approximation: the Laplace / SVGP methods."""
    if isinstance(approx, NearestNeighbors):
        fx, y = args
        ctx, dtype = _nn_kwargs("posterior", kwargs, ("mean_offsets",))
        return NNPosteriorGP(approx, fx, y, ctx=ctx, dtype=dtype, mean_offsets=kwargs.get("mean_offsets"))
    return _laplace.posterior(approx, *args, **kwargs)
