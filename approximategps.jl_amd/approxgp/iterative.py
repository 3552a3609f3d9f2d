"""The exact GP by matrix-free conjugate gradients (GPyTorch's BBMM, Gardner et al. 2018; Wang et al. 2019) over the C-ABI of
libsvgp_mi355x.so (include/svgp_mi355x.h, svgp_cg_*): the batched solves, the stochastic Lanczos quadrature of log det, the
gradient and the predictions all run on the device.  This file packs parameters and draws the probe vectors, which the library never
does itself."""
from __future__ import annotations

import ctypes as C
import warnings

import numpy as np

from . import _ffi
from . import nearest_neighbors as _nn
from . import vfe as _vfe
from .gp import Diagonal, FiniteGP
from .kernels import unpack_kernel


def draw_probes(N: int, T: int, rng=None):
    """(N, T) Rademacher columns (E z z' = I), float64, column-major: the probe vectors of the log det estimate."""
    rng = np.random.default_rng(rng)
    return np.asfortranarray(rng.integers(0, 2, size=(int(N), int(T))).astype(np.float64) * 2.0 - 1.0)


MAX_PRECOND = 2048   # svgp_cg_set_preconditioner's limit


def _seed_int(seed):
    if seed is None or int(seed) != seed or int(seed) < 0:
        raise ValueError("a preconditioner needs a non-negative integer seed")
    return int(seed)


class ConjugateGradients:
    """ConjugateGradients(tol, maxiter, n_probes, seed, probes): logpdf(fx, y), its gradient and the posterior of the exact GP by
    iterative solves against K(x, x) + Σy, never stored.  tol None: 1e-8, and 1e-4 for float32 data.  The log det comes from n_probes
    Rademacher vectors drawn from default_rng(seed) - the same vectors on every call, so the objective is a deterministic function of
    the hyperparameters (common random numbers) - or from the caller's (N, T) probes.
    precond_size = k > 0 or precond_points (a (d, k) array, e.g. a trained model's z; a plain vector for d = 1) sets the Nystrom
    preconditioner P = Z Kuu^-1 Z' + Σy I of k points: without points, a subset of the data drawn from default_rng([seed, 2]) without
    replacement, k clipped to N.  precond_jitter (times the kernel variance) is added to Kuu.  The k-sized part of the probes comes from
    default_rng([seed, 1]); the (N, T) probes of a seed do not depend on the preconditioner."""

    def __init__(self, tol=None, maxiter: int = 1000, n_probes: int = 16, seed: int = 0, probes=None, precond_size: int = 0,
                 precond_points=None, precond_jitter: float = 1e-4):
        if tol is not None and not float(tol) > 0:
            raise ValueError("ConjugateGradients needs tol > 0")
        if int(maxiter) != maxiter or int(maxiter) < 1:
            raise ValueError("ConjugateGradients needs maxiter >= 1")
        if int(n_probes) != n_probes or int(n_probes) < 0:
            raise ValueError("ConjugateGradients needs n_probes >= 0")
        if probes is not None:
            probes = np.asarray(probes, dtype=np.float64)
            if probes.ndim != 2:
                raise ValueError("probes is an (N, T) array")
        if int(precond_size) != precond_size or int(precond_size) < 0:
            raise ValueError("ConjugateGradients needs precond_size >= 0")
        if not float(precond_jitter) >= 0:
            raise ValueError("ConjugateGradients needs precond_jitter >= 0")
        if precond_points is not None:
            precond_points = np.asarray(precond_points, dtype=np.float64)
            if precond_points.ndim == 1:
                precond_points = precond_points[None, :]
            if precond_points.ndim != 2 or precond_points.shape[1] < 1:
                raise ValueError("precond_points is a (d, k) array with k >= 1")
            if precond_points.shape[1] > MAX_PRECOND:
                raise ValueError(f"at most {MAX_PRECOND} preconditioner points")
            if precond_size not in (0, precond_points.shape[1]):
                raise ValueError("precond_size differs from the number of precond_points")
        elif int(precond_size) > MAX_PRECOND:
            raise ValueError(f"at most {MAX_PRECOND} preconditioner points")
        self.tol = None if tol is None else float(tol)
        self.maxiter, self.n_probes, self.seed, self.probes = int(maxiter), int(n_probes), seed, probes
        self.precond_size, self.precond_points, self.precond_jitter = int(precond_size), precond_points, float(precond_jitter)

    def tol_for(self, dtype) -> float:
        if self.tol is not None:
            return self.tol
        return 1e-4 if np.dtype(dtype) == np.float32 else 1e-8

    def probes_for(self, N: int):
        if self.probes is not None:
            if self.probes.shape[0] != N:
                raise ValueError("probes has one row per data point")
            return np.asfortranarray(self.probes)
        return draw_probes(N, self.n_probes, self.seed)

    def precond_points_for(self, x):
        """-> the (d, k) preconditioner points for the (d, N) inputs x, or None"""
        if self.precond_points is not None:
            if self.precond_points.shape[0] != x.shape[0]:
                raise ValueError("precond_points have a different dimension than the data")
            return self.precond_points
        if self.precond_size == 0:
            return None
        N = x.shape[1]
        idx = np.random.default_rng([_seed_int(self.seed), 2]).choice(N, size=min(self.precond_size, N), replace=False)
        return np.asarray(x, dtype=np.float64)[:, idx]

    def probes_k_for(self, k: int, T: int):
        """(k, T) Rademacher columns from default_rng([seed, 1]): the preconditioner's part of the probes"""
        return draw_probes(k, T, np.random.default_rng([_seed_int(self.seed), 1]))


class DeviceConjugateGradients:
    """A resident svgp_cg handle over x (and y): x a plain vector (d = 1) or a (d, n) ColVecs array; with layout = ROWVECS an (n, d)
    RowVecs array.  data = an existing _ffi.DeviceData (x, y, dtype and layout None) borrows it instead of uploading: e.g. a
    DeviceData.wrap of torch features, with no host round trip; the caller keeps it alive and frees it."""

    def __init__(self, ctx: _ffi.Context, x=None, y=None, dtype=None, layout=None, data=None):
        self.ctx = ctx
        if data is not None:
            if not isinstance(data, _ffi.DeviceData):
                raise TypeError("data: an _ffi.DeviceData")
            if x is not None or y is not None or dtype is not None or layout is not None:
                raise ValueError("data replaces x, y, dtype and layout")
            if getattr(data, "h", None) is None:
                raise ValueError("data has been freed")
            self.data, self._owns_data = data, False
        else:
            if x is None or dtype is None:
                raise ValueError("DeviceConjugateGradients needs x and dtype, or data")
            x = np.asarray(x)
            if layout is None:
                layout = _ffi.VEC if x.ndim == 1 else _ffi.COLVECS
            self.data, self._owns_data = _ffi.DeviceData(ctx, x, y, dtype, layout), True
        self.dtype, self.d, self.n = self.data.dtype, self.data.d, self.data.n
        self.precond_k = 0   # points of the preconditioner set through set_preconditioner
        self.has_noise = False   # a per-point noise vector set through set_noise
        h = C.c_void_p()
        ctx.check(ctx.lib.svgp_cg_create(ctx.h, self.data.h, C.byref(h)))
        self.h = h

    def desc(self, kernel, diag=0.0, mean_const=0.0, tol=1e-8, maxiter=1000):
        """-> (CGDesc, the array it points into: keep it alive)"""
        family, variance, il = unpack_kernel(kernel, self.d)
        il = np.ascontiguousarray(il, dtype=np.float64)
        ds = _ffi.CGDesc(dtype=self.dtype, kernel=family, d=self.d, maxiter=int(maxiter), variance=float(variance),
                         inv_lengthscale=il.ctypes.data_as(C.POINTER(C.c_double)), diag=float(diag), mean_const=float(mean_const),
                         tol=float(tol), reserved=0)
        return ds, il

    def _check(self, rc):
        if rc == _ffi.NOT_POSDEF:
            msg = (self.ctx.lib.svgp_last_error(self.ctx.h) or b"").decode()
            raise _ffi.PosDefException(-1, msg)
        self.ctx.check(rc)

    def _cols(self, a, name):
        """-> (pointer, ld, S, on_device, host array or None) of an (N, S) panel: a numpy array, or a torch device tensor holding it
        column-major (shape (S, N) contiguous, or (N,))"""
        if _ffi._is_device_tensor(a):
            if (not a.is_contiguous() or a.element_size() != np.dtype(_ffi.np_dtype(self.dtype)).itemsize or not a.is_floating_point()
                    or a.shape[-1] != self.n or a.dim() > 2):
                raise ValueError(f"{name}: a contiguous (S, N) device tensor of the data dtype (its rows are the columns)")
            S = 1 if a.dim() == 1 else a.shape[0]
            return C.c_void_p(int(a.data_ptr())), self.n, S, 1, None
        h = np.asarray(a, dtype=_ffi.np_dtype(self.dtype))
        if h.ndim == 1:
            h = h[:, None]
        if h.ndim != 2 or h.shape[0] != self.n:
            raise ValueError(f"{name}: an (N, S) array")
        h = np.asfortranarray(h)
        return _ffi._ptr(h), self.n, h.shape[1], 0, h

    def matvec(self, desc, V, out=None):
        """(K(x, x) + diag I) V for an (N, S) panel.  A torch device tensor ((S, N), contiguous) needs out of the same kind."""
        vp, ldv, S, dev, keep = self._cols(V, "V")
        if S < 1:
            raise ValueError("V: an (N, S) array with S >= 1")
        if dev:
            if out is None or not _ffi._is_device_tensor(out):
                raise ValueError("out: a device tensor like V")
            op, ldo, So, _, _ = self._cols(out, "out")
            if So != S:
                raise ValueError("out: a device tensor like V")
            res = out
        else:
            res = np.zeros((self.n, S), dtype=_ffi.np_dtype(self.dtype), order="F")
            op, ldo = _ffi._ptr(res), self.n
        self._check(self.ctx.lib.svgp_cg_matvec(self.ctx.h, self.h, C.byref(desc), S, vp, ldv, op, ldo, dev))
        return res

    def solve(self, desc, B, out=None):
        """-> (X, iterations (S,), relative residuals (S,), CGInfo).  PosDefException when a curvature is not positive."""
        bp, ldb, S, dev, keep = self._cols(B, "B")
        if S < 1:
            raise ValueError("B: an (N, S) array with S >= 1")
        if dev:
            if out is None or not _ffi._is_device_tensor(out):
                raise ValueError("out: a device tensor like B")
            xp, ldx, So, _, _ = self._cols(out, "out")
            if So != S:
                raise ValueError("out: a device tensor like B")
            res = out
        else:
            res = np.zeros((self.n, S), dtype=_ffi.np_dtype(self.dtype), order="F")
            xp, ldx = _ffi._ptr(res), self.n
        iters, rel, info = np.zeros(S, dtype=np.int32), np.zeros(S), _ffi.CGInfo()
        self._check(self.ctx.lib.svgp_cg_solve(self.ctx.h, self.h, C.byref(desc), S, bp, ldb, xp, ldx, dev,
                                               iters.ctypes.data_as(C.POINTER(C.c_int32)), rel.ctypes.data_as(C.POINTER(C.c_double)),
                                               C.byref(info)))
        return res, iters, rel, info

    @staticmethod
    def _f64(a):
        return None if a is None else np.asfortranarray(np.asarray(a, dtype=np.float64))

    def set_preconditioner(self, points=None, jitter=1e-4, layout=None):
        """The Nystrom preconditioner's k points: x as for the handle ((d, k), a plain vector for d = 1, or (k, d) with ROWVECS);
        None removes it."""
        if points is None:
            self.ctx.check(self.ctx.lib.svgp_cg_set_preconditioner(self.ctx.h, self.h, _ffi.COLVECS, 0, None, 0.0))
            self.precond_k = 0
            return
        z = np.asarray(points, dtype=_ffi.np_dtype(self.dtype))
        if z.ndim == 1:
            if self.d != 1:
                raise ValueError("preconditioner points have a different dimension than the data")
            layout, k, zb = _ffi.VEC, z.shape[0], np.ascontiguousarray(z)
        elif layout == _ffi.ROWVECS:
            if z.ndim != 2 or z.shape[1] != self.d:
                raise ValueError("preconditioner points have a different dimension than the data")
            k, zb = z.shape[0], np.asfortranarray(z)
        else:
            if z.ndim != 2 or z.shape[0] != self.d:
                raise ValueError("preconditioner points have a different dimension than the data")
            layout, k, zb = _ffi.COLVECS, z.shape[1], np.asfortranarray(z)
        if k < 1:
            raise ValueError("at least one preconditioner point (None removes the preconditioner)")
        self.ctx.check(self.ctx.lib.svgp_cg_set_preconditioner(self.ctx.h, self.h, layout, k, _ffi._ptr(zb), float(jitter)))
        self.precond_k = k

    def set_noise(self, s=None):
        """Per-point noise variances (svgp_cg_set_noise): sigma_i^2 = diag + s_i, Khat = K + diag(sigma^2) in every later call.  s: an
        (N,) numpy array (converted to the data dtype) or a contiguous torch device tensor of the data dtype; the handle keeps a copy.
        None removes the vector.  The cached fit is dropped either way."""
        if s is None:
            self.ctx.check(self.ctx.lib.svgp_cg_set_noise(self.ctx.h, self.h, None))
            self.has_noise = False
            return
        pn, keep = _ffi.point_noise(s, self.n, self.dtype)
        self.has_noise = False
        self.ctx.check(self.ctx.lib.svgp_cg_set_noise(self.ctx.h, self.h, C.byref(pn)))
        self.has_noise = True

    def _noise_grad(self, noise_grad_out):
        """-> (PointNoiseGrad, what lml_grad returns as grads["noise"]): an (N,) array of the data dtype, or the caller's device tensor"""
        if noise_grad_out is None:
            sg = np.zeros(self.n, dtype=_ffi.np_dtype(self.dtype))
            return _ffi.PointNoiseGrad(_ffi._ptr(sg), 0, 0), sg
        t = noise_grad_out
        if (not _ffi._is_device_tensor(t) or not t.is_contiguous() or not t.is_floating_point() or t.numel() != self.n
                or t.element_size() != np.dtype(_ffi.np_dtype(self.dtype)).itemsize):
            raise ValueError("noise_grad_out: a contiguous (N,) device tensor of the data dtype")
        return _ffi.PointNoiseGrad(C.c_void_p(int(t.data_ptr())), 1, 0), t

    def _need_precond(self):
        if not self.precond_k:
            raise ValueError("no preconditioner is set (set_preconditioner)")
        return self.precond_k

    def precond_cross(self, desc, V, out=None):
        """K(z_p, x) V, (k, S), for an (N, S) panel: the row-split kernel alone.  A torch device tensor ((S, N), contiguous) needs out
        as an (S, k) contiguous device tensor."""
        k = self._need_precond()
        vp, ldv, S, dev, keep = self._cols(V, "V")
        if S < 1:
            raise ValueError("V: an (N, S) array with S >= 1")
        if dev:
            shapes = ((S, k), (k,)) if V.dim() == 1 else ((S, k),)
            if (out is None or not _ffi._is_device_tensor(out) or not out.is_contiguous() or out.dtype != V.dtype
                    or tuple(out.shape) not in shapes):
                raise ValueError("out: a contiguous (S, k) device tensor of the data dtype")
            res, op = out, C.c_void_p(int(out.data_ptr()))
        else:
            res = np.zeros((k, S), dtype=_ffi.np_dtype(self.dtype), order="F")
            op = _ffi._ptr(res)
        self._check(self.ctx.lib.svgp_cg_precond_cross(self.ctx.h, self.h, C.byref(desc), S, vp, ldv, op, k, dev))
        return res

    def precond_apply(self, desc, R, out=None):
        """-> (P^-1 R, log det P) for an (N, S) panel"""
        self._need_precond()
        rp, ldr, S, dev, keep = self._cols(R, "R")
        if S < 1:
            raise ValueError("R: an (N, S) array with S >= 1")
        if dev:
            if out is None or not _ffi._is_device_tensor(out):
                raise ValueError("out: a device tensor like R")
            op, ldo, So, _, _ = self._cols(out, "out")
            if So != S:
                raise ValueError("out: a device tensor like R")
            res = out
        else:
            res = np.zeros((self.n, S), dtype=_ffi.np_dtype(self.dtype), order="F")
            op, ldo = _ffi._ptr(res), self.n
        ld = C.c_double()
        self._check(self.ctx.lib.svgp_cg_precond_apply(self.ctx.h, self.h, C.byref(desc), S, rp, ldr, op, ldo, dev, C.byref(ld)))
        return res, ld.value

    def _probes(self, probes, probes_k):
        z, zk = self._f64(probes), self._f64(probes_k)
        T = 0 if z is None else z.shape[1]
        if zk is not None:
            if zk.ndim != 2 or zk.shape != (self._need_precond(), T):
                raise ValueError("probes_k: a (k, T) array beside the (N, T) probes")
        dp = C.POINTER(C.c_double)
        return T, (None if z is None or T == 0 else z.ctypes.data_as(dp)), (None if zk is None or T == 0 else zk.ctypes.data_as(dp)), (z, zk)

    def fit(self, desc, probes=None, delta=None, probes_k=None):
        """-> (lml, CGInfo); caches alpha for predict.  probes: (N, T) float64 or None (T = 0: lml is NaN, info.quad valid); probes_k:
        the (k, T) part a preconditioner's probes need."""
        T, zp, zkp, keep = self._probes(probes, probes_k)
        dl = self._f64(delta)
        lml, info = C.c_double(), _ffi.CGInfo()
        dlp = None if dl is None else dl.ctypes.data_as(C.POINTER(C.c_double))
        if probes_k is None:
            self._check(self.ctx.lib.svgp_cg_fit(self.ctx.h, self.h, C.byref(desc), dlp, T, zp, C.byref(lml), C.byref(info)))
        else:
            self._check(self.ctx.lib.svgp_cg_fit_precond(self.ctx.h, self.h, C.byref(desc), dlp, T, zp, zkp, C.byref(lml), C.byref(info)))
        return lml.value, info

    def _x_grad(self, x_grad_out):
        """-> (InputGrad, what lml_grad returns as grads["x"]): a (d, N) array of the data dtype, or the caller's device tensor"""
        if x_grad_out is None:
            xg = np.zeros((self.d, self.n), dtype=_ffi.np_dtype(self.dtype))
            return _ffi.InputGrad(_ffi._ptr(xg), self.n, 0, 0), xg
        t = x_grad_out
        if (not _ffi._is_device_tensor(t) or not t.is_contiguous() or not t.is_floating_point() or tuple(t.shape) != (self.d, self.n)
                or t.element_size() != np.dtype(_ffi.np_dtype(self.dtype)).itemsize):
            raise ValueError("x_grad_out: a contiguous (d, N) device tensor of the data dtype")
        return _ffi.InputGrad(C.c_void_p(int(t.data_ptr())), self.n, 1, 0), t

    def lml_grad(self, desc, probes, delta=None, probes_k=None, wrt_inputs=False, x_grad_out=None, wrt_noise=False, noise_grad_out=None):
        """-> (lml, {"variance", "inv_lengthscale" (d,), "diag", "mean_const"}, CGInfo).  wrt_inputs: grads["x"] as well, (d, N) in the
        data dtype: d lml / d x_ic by the same trace estimator (svgp_cg_lml_grad_inputs), every other entry bitwise what it is without;
        x_grad_out: a contiguous (d, N) torch device tensor to write it into (it is returned as grads["x"]).  wrt_noise: grads["noise"]
        as well, (N,) in the data dtype: d lml / d sigma_i^2 (svgp_cg_lml_grad_noise), with or without a vector set; its sum is
        grads["diag"]; noise_grad_out: a contiguous (N,) torch device tensor to write it into."""
        if not isinstance(wrt_inputs, (bool, np.bool_)):
            raise ValueError("wrt_inputs is True or False")
        if not isinstance(wrt_noise, (bool, np.bool_)):
            raise ValueError("wrt_noise is True or False")
        if x_grad_out is not None and not wrt_inputs:
            raise ValueError("x_grad_out needs wrt_inputs=True")
        if noise_grad_out is not None and not wrt_noise:
            raise ValueError("noise_grad_out needs wrt_noise=True")
        T, zp, zkp, keep = self._probes(probes, probes_k)
        dl = self._f64(delta)
        if (wrt_inputs or wrt_noise) and dl is not None and dl.shape != (self.n,):
            raise ValueError("delta: an (N,) array")
        lml, info = C.c_double(), _ffi.CGInfo()
        dv, dd, dm, dil = C.c_double(), C.c_double(), C.c_double(), np.zeros(self.d)
        dp = C.POINTER(C.c_double)
        dlp = None if dl is None else dl.ctypes.data_as(dp)
        if wrt_noise:
            if self.precond_k and T > 0 and probes_k is None:
                raise ValueError("a preconditioner is set: the probes need probes_k, a (k, T) array")
            gx, xg = self._x_grad(x_grad_out) if wrt_inputs else (None, None)
            gpn, sg = self._noise_grad(noise_grad_out)
            self._check(self.ctx.lib.svgp_cg_lml_grad_noise(self.ctx.h, self.h, C.byref(desc), dlp, T, zp, zkp if self.precond_k else None,
                                                            C.byref(lml), C.byref(info), C.byref(dv), dil.ctypes.data_as(dp), C.byref(dd),
                                                            C.byref(dm), None if gx is None else C.byref(gx), C.byref(gpn)))
            grads = {"variance": dv.value, "inv_lengthscale": dil, "diag": dd.value, "mean_const": dm.value, "noise": sg}
            if wrt_inputs:
                grads["x"] = xg
            return lml.value, grads, info
        if wrt_inputs:
            if self.precond_k and T > 0 and probes_k is None:
                raise ValueError("a preconditioner is set: the probes need probes_k, a (k, T) array")
            gx, xg = self._x_grad(x_grad_out)
            self._check(self.ctx.lib.svgp_cg_lml_grad_inputs(self.ctx.h, self.h, C.byref(desc), dlp, T, zp, zkp if self.precond_k else None,
                                                             C.byref(lml), C.byref(info), C.byref(dv), dil.ctypes.data_as(dp), C.byref(dd),
                                                             C.byref(dm), C.byref(gx)))
            return lml.value, {"variance": dv.value, "inv_lengthscale": dil, "diag": dd.value, "mean_const": dm.value, "x": xg}, info
        if probes_k is None:
            self._check(self.ctx.lib.svgp_cg_lml_grad(self.ctx.h, self.h, C.byref(desc), dlp, T, zp, C.byref(lml), C.byref(info),
                                                      C.byref(dv), dil.ctypes.data_as(dp), C.byref(dd), C.byref(dm)))
        else:
            self._check(self.ctx.lib.svgp_cg_lml_grad_precond(self.ctx.h, self.h, C.byref(desc), dlp, T, zp, zkp, C.byref(lml), C.byref(info),
                                                              C.byref(dv), dil.ctypes.data_as(dp), C.byref(dd), C.byref(dm)))
        return lml.value, {"variance": dv.value, "inv_lengthscale": dil, "diag": dd.value, "mean_const": dm.value}, info

    def alpha(self):
        a = np.zeros(self.n, dtype=_ffi.np_dtype(self.dtype))
        self.ctx.check(self.ctx.lib.svgp_cg_alpha(self.ctx.h, self.h, _ffi._ptr(a)))
        return a

    def predict(self, x, mean=True, var=True, layout=None):
        """-> (mean, var, CGInfo of the variance's solve); x as for the handle"""
        dt = _ffi.np_dtype(self.dtype)
        x = np.asarray(x, dtype=dt)
        if x.ndim == 1:
            if self.d != 1:
                raise ValueError("test inputs have a different dimension than the data")
            layout, n, xb = _ffi.VEC, x.shape[0], np.ascontiguousarray(x)
        elif layout == _ffi.ROWVECS:
            if x.shape[1] != self.d:
                raise ValueError("test inputs have a different dimension than the data")
            n, xb = x.shape[0], np.asfortranarray(x)
        else:
            if x.shape[0] != self.d:
                raise ValueError("test inputs have a different dimension than the data")
            layout, n, xb = _ffi.COLVECS, x.shape[1], np.asfortranarray(x)
        m = np.zeros(n, dtype=dt) if mean else None
        v = np.zeros(n, dtype=dt) if var else None
        info = _ffi.CGInfo()
        self._check(self.ctx.lib.svgp_cg_predict(self.ctx.h, self.h, layout, n, _ffi._ptr(xb), _ffi._ptr(m), _ffi._ptr(v), C.byref(info)))
        return m, v, info

    def sampler(self, desc, basis, delta=None):
        """svgp_cg_sampler_create: S pathwise function samples of the exact posterior under `desc` from basis = (omega (L, d), tau (L,),
        w (S, L), eps (S, N)) - every random number is the caller's (approxgp.pathwise.draw_basis(kernel, N, L, S, ...) draws them).
        One batched solve of S right-hand sides; the DeviceCGSampler is a snapshot and outlives this handle.  delta: (N,) or None for
        y - mean_const."""
        packed = pack_cg_basis(self.n, self.d, self.dtype, basis)   # every check before the GPU is touched
        dl = self._f64(delta)
        if dl is not None and dl.shape != (self.n,):
            raise ValueError("delta: an (N,) array")
        return DeviceCGSampler(self, desc, packed, dl)

    def free(self):
        if getattr(self, "h", None):
            self.ctx.lib.svgp_cg_free(self.ctx.h, self.h)
            self.h = None
        if getattr(self, "data", None) is not None:
            if getattr(self, "_owns_data", True):
                self.data.free()
            self.data = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def cg_sample_plan(N: int):
    """-> (seg_rows, n_segments, round_points) of the sampler's evaluations over N data rows: the library's own svgp_cg_sampler_plan (host
    only, no GPU needed), where the rule lives."""
    N = int(N)
    if N < 0:
        raise ValueError("N >= 0")
    seg_rows, nseg, rnd = C.c_int64(), C.c_int32(), C.c_int64()
    rc = _ffi.load_library().svgp_cg_sampler_plan(N, C.byref(seg_rows), C.byref(nseg), C.byref(rnd))
    if rc != _ffi.OK:
        raise ValueError(f"svgp_cg_sampler_plan({N}) returned {rc}")
    return seg_rows.value, nseg.value, rnd.value


def pack_cg_basis(N: int, d: int, dtype: int, basis):
    """(omega (L, d), tau (L,), w (S, L), eps (S, N)) checked and laid out for svgp_cg_sampler_create -> (L, S, omega, tau, w, eps)."""
    try:
        omega, tau, w, eps = basis
    except (TypeError, ValueError):
        raise ValueError("basis is (omega (L, d), tau (L,), w (S, L), eps (S, N))") from None
    dt = _ffi.np_dtype(dtype)
    eps = np.ascontiguousarray(np.asarray(eps, dtype=dt))
    if eps.ndim != 2 or eps.shape[1] != N or eps.shape[0] < 1:
        raise ValueError("eps must be (S, N) with S >= 1: one standard normal draw per sample and data point")
    S = eps.shape[0]
    w = np.asarray(np.zeros((S, 0)) if w is None else w, dtype=dt)
    if w.ndim != 2 or w.shape[0] != S:
        raise ValueError("w must be (S, L)")
    w = np.ascontiguousarray(w)
    L = w.shape[1]
    omega = np.asarray(np.zeros((0, d)) if omega is None else omega, dtype=dt)
    tau = np.asarray(np.zeros(0) if tau is None else tau, dtype=dt)
    if omega.shape != (L, d):
        raise ValueError("omega must be (L, d)")
    if tau.shape != (L,):
        raise ValueError("tau must be (L,)")
    return L, S, np.ascontiguousarray(omega), np.ascontiguousarray(tau), w, eps


def _check_sample_counts(n_samples, n_features):
    if int(n_samples) != n_samples or int(n_samples) < 1:
        raise ValueError("function_samples needs n_samples >= 1")
    if int(n_features) != n_features or int(n_features) < 0:
        raise ValueError("function_samples needs n_features >= 0")
    return int(n_samples), int(n_features)


class DeviceCGSampler:
    """S function samples of the exact GP's posterior, resident in HBM (svgp_cg_sampler): evaluate them and their input gradients
    anywhere, any number of times.  A point's value does not depend on the other points, the call or the other samples, bitwise."""

    def __init__(self, dev: DeviceConjugateGradients, desc, packed, delta=None):
        self.ctx = ctx = dev.ctx
        self.n, self.d, self.dtype = dev.n, dev.d, dev.dtype
        L, S, omega, tau, w, eps = packed
        self.n_samples, self.n_features = S, L
        basis = _ffi.SampleBasis(L, S, _ffi._ptr(omega) if L else None, _ffi._ptr(tau) if L else None, _ffi._ptr(w) if L else None,
                                 _ffi._ptr(eps))
        h, self.info = C.c_void_p(), _ffi.CGInfo()
        dlp = None if delta is None else delta.ctypes.data_as(C.POINTER(C.c_double))
        dev._check(ctx.lib.svgp_cg_sampler_create(ctx.h, dev.h, C.byref(desc), dlp, C.byref(basis), C.byref(h), C.byref(self.info)))
        self.h = h

    def _points(self, x):
        """-> (DeviceData, owned): a resident DeviceData as it is, or x (a plain vector for d = 1, or (d, n) ColVecs) uploaded"""
        if isinstance(x, _ffi.DeviceData):
            if x.d != self.d or x.dtype != self.dtype:
                raise ValueError("the data have a different dimension or dtype than the sampler")
            return x, False
        x = check_points(x, self.d)
        return _ffi.DeviceData(self.ctx, x, None, _ffi.np_dtype(self.dtype)), True

    def _dev_out(self, t, rows, n, name):
        if (not _ffi._is_device_tensor(t) or not t.is_contiguous() or not t.is_floating_point()
                or t.element_size() != np.dtype(_ffi.np_dtype(self.dtype)).itemsize or t.numel() != rows * n):
            raise ValueError(f"{name}: a contiguous device tensor of the data dtype with {rows} x n elements")
        return C.c_void_p(int(t.data_ptr()))

    @staticmethod
    def _window(data, off, length):
        off = int(off)
        n = data.n - off if length is None else int(length)
        if off < 0 or n < 1 or off + n > data.n:
            raise ValueError("window outside the data")
        return off, n

    def eval(self, x, out=None, off=0, length=None):
        """f_s at the points x (of a DeviceData: its window [off, off + length)) -> (S, n) array of the data dtype (row s = sample s);
        out: a contiguous (S, n) torch device tensor to write there instead (it is returned)."""
        data, owned = self._points(x)
        try:
            ctx = self.ctx
            off, n = self._window(data, off, length)
            if out is not None:
                ctx.check(ctx.lib.svgp_cg_sampler_eval(ctx.h, self.h, data.h, off, n, self._dev_out(out, self.n_samples, n, "out"), n, 1))
                return out
            buf = np.zeros((self.n_samples, n), dtype=_ffi.np_dtype(self.dtype))
            ctx.check(ctx.lib.svgp_cg_sampler_eval(ctx.h, self.h, data.h, off, n, _ffi._ptr(buf), n, 0))
            return buf
        finally:
            if owned:
                data.free()

    def eval_grad(self, x, values=True, out=None, grad_out=None, off=0, length=None):
        """-> (F (S, n) or None, G (S, d, n)): G[s, c, j] = d f_s / d x_c at point j; the values are bitwise eval's.  grad_out (and out,
        when values are wanted): contiguous torch device tensors of S d n (S n) elements to write there instead."""
        data, owned = self._points(x)
        try:
            ctx, S, d = self.ctx, self.n_samples, self.d
            off, n = self._window(data, off, length)
            if grad_out is not None or out is not None:
                if grad_out is None or (values and out is None):
                    raise ValueError("device output: grad_out is required, and out when values are wanted (both live in the same kind of memory)")
                gp = self._dev_out(grad_out, S * d, n, "grad_out")
                op = self._dev_out(out, S, n, "out") if values else None
                ctx.check(ctx.lib.svgp_cg_sampler_eval_grad(ctx.h, self.h, data.h, off, n, op, n, gp, n, 1))
                return (out if values else None), grad_out
            dt = _ffi.np_dtype(self.dtype)
            F = np.zeros((S, n), dtype=dt) if values else None
            G = np.zeros((S, d, n), dtype=dt)
            ctx.check(ctx.lib.svgp_cg_sampler_eval_grad(ctx.h, self.h, data.h, off, n, _ffi._ptr(F), n, _ffi._ptr(G), n, 0))
            return F, G
        finally:
            if owned:
                data.free()

    def state(self):
        """-> (V (N, S) in the data dtype exactly as evaluated, iterations (S,), relative residuals (S,)) of the solve"""
        V = np.zeros((self.n, self.n_samples), dtype=_ffi.np_dtype(self.dtype), order="F")
        iters, rel = np.zeros(self.n_samples, dtype=np.int32), np.zeros(self.n_samples)
        self.ctx.check(self.ctx.lib.svgp_cg_sampler_state(self.ctx.h, self.h, _ffi._ptr(V), iters.ctypes.data_as(C.POINTER(C.c_int32)),
                                                          rel.ctypes.data_as(C.POINTER(C.c_double))))
        return V, iters, rel

    def free(self):
        if getattr(self, "h", None):
            self.ctx.lib.svgp_cg_sampler_free(self.ctx.h, self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def check_points(x, d):
    """test inputs as an array: a plain vector for d = 1, or a (d, n) ColVecs array with n >= 1"""
    x = np.asarray(x)
    if x.ndim == 1:
        if d != 1:
            raise ValueError("test inputs have a different dimension than the data")
    elif x.ndim != 2 or x.shape[0] != d:
        raise ValueError("test inputs have a different dimension than the data")
    if x.shape[-1] < 1:
        raise ValueError("no test points")
    return x


class CGFunctionSamples:
    """S functions drawn from a CGPosteriorGP, resident on the device, with pathwise.FunctionSamples' interface: fs(x) -> (n, S),
    fs.grad(x) -> (n, S, d), fs.value_and_grad(x), fs.state(), fs.free()."""

    def __init__(self, post, sampler):
        self._post, self.sampler, self.n_samples = post, sampler, sampler.n_samples

    def _offsets(self, x, F):
        mu = self._post.prior.mean_offsets(np.asarray(x))
        return F if mu is None else (F + np.asarray(mu)[:, None]).astype(F.dtype)

    def __call__(self, x):
        return self._offsets(x, np.ascontiguousarray(self.sampler.eval(check_points(x, self.sampler.d)).T))

    def grad(self, x):
        """-> (n, S, d): [j, s, c] = d f_s / d x_c at x_j, the gradient of f_s minus the prior mean (a non-constant mean function's own
        Jacobian is the caller's to add)."""
        return np.ascontiguousarray(self.sampler.eval_grad(check_points(x, self.sampler.d), values=False)[1].transpose(2, 0, 1))

    def value_and_grad(self, x):
        """-> (fs(x) (n, S), grad(x) (n, S, d)) from one call; the values are bitwise those of fs(x)."""
        F, G = self.sampler.eval_grad(check_points(x, self.sampler.d), values=True)
        return self._offsets(x, np.ascontiguousarray(F.T)), np.ascontiguousarray(G.transpose(2, 0, 1))

    def state(self):
        return self.sampler.state()

    def free(self):
        self.sampler.free()


def _warn(info, what):
    if not info.converged:
        warnings.warn(f"conjugate gradients: {info.n_unconverged} column(s) of {what} did not reach tol in {info.iterations} "
                      f"iterations (largest relative residual {info.max_rel_residual:.3e})", RuntimeWarning, stacklevel=3)


def _cg_kwargs(fn, kwargs, also=()):
    extra = set(kwargs) - {"ctx", "dtype"} - set(also)
    if extra:
        raise TypeError(f"{fn}() with ConjugateGradients got unexpected keyword arguments {sorted(extra)}")
    return kwargs.get("ctx"), kwargs.get("dtype")


def _check_inputs(fx: FiniteGP, y):
    """-> (diag, mean_const, delta or None, s or None), before the GPU is touched.  A CustomMean prior is passed as delta = y - mean(x);
    Σy = Diagonal(v) as diag = min(v) and the per-point variances s = v - min(v) above it (vfe.py's mapping)."""
    if not isinstance(fx, FiniteGP):
        raise TypeError("ConjugateGradients takes fx = f(x, Σy)")
    s = None
    if isinstance(fx.Sigma_y, Diagonal):
        sy = np.asarray(fx.Sigma_y.diag, dtype=np.float64)
        if sy.ndim != 1 or sy.shape[0] != fx.n:
            raise ValueError(f"fx.Σy = Diagonal(v) needs a vector with one variance per point ({fx.n}); got shape {sy.shape}")
        if not np.all(sy > 0.0):   # (NaN included)
            raise ValueError("fx.Σy must be positive: every per-point noise variance must be > 0")
        diag = float(sy.min())
        s = sy - diag
    elif not fx.is_isotropic():
        raise _ffi.UnsupportedError("ConjugateGradients needs an isotropic fx.Σy, or per-point noise variances v as fx = f(x, Diagonal(v)) "
                                    "(a full noise covariance is out of scope)")
    else:
        diag = float(fx.Sigma_y)
        if not diag >= 0:
            raise ValueError("fx.Σy must be >= 0")
    if np.shape(y)[0] != fx.n:
        raise ValueError("x and y lengths differ")
    delta = None
    if fx.f.mean_fn is not None:
        delta = np.asarray(y, dtype=np.float64).reshape(-1) - fx.f.mean_offsets(fx.x)
    return diag, float(fx.f.mean_const), delta, s


def _device(cg: ConjugateGradients, fx: FiniteGP, y, ctx, dtype):
    diag, mean_const, delta, s = _check_inputs(fx, y)
    dt = _nn._dtype_of(fx, dtype)
    probes = cg.probes_for(fx.n)
    xa = np.asarray(fx.x)
    points = cg.precond_points_for(xa[None, :] if xa.ndim == 1 else xa)
    probes_k = None
    if points is not None:
        if not diag > 0:
            raise ValueError("the preconditioner needs observation noise fx.Σy > 0")
        probes_k = cg.probes_k_for(points.shape[1], probes.shape[1])
    dev = DeviceConjugateGradients(ctx or _ffi.default_context(), fx.x, y, dt)
    try:
        if points is not None:
            dev.set_preconditioner(points[0] if dev.d == 1 and xa.ndim == 1 else points, cg.precond_jitter)
        if s is not None:
            dev.set_noise(s)
        desc, keep = dev.desc(fx.f.kernel, diag, mean_const, cg.tol_for(dt), cg.maxiter)
    except Exception:
        dev.free()
        raise
    return dev, desc, keep, (probes, probes_k), delta


def approx_lml(approx, fx, y, **kwargs):
    """approx_lml(ConjugateGradients(), fx, y; ctx, dtype): logpdf(fx, y) of the exact GP with log det by stochastic Lanczos
    quadrature; any other approximation: the existing methods with every keyword passed on exactly as given."""
    if not isinstance(approx, ConjugateGradients):
        return _vfe.approx_lml(approx, fx, y, **kwargs)
    ctx, dtype = _cg_kwargs("approx_lml", kwargs)
    dev, desc, keep, probes, delta = _device(approx, fx, y, ctx, dtype)
    try:
        lml, info = dev.fit(desc, probes[0], delta, probes_k=probes[1])
    finally:
        dev.free()
    _warn(info, "the fit")
    return lml


def approx_lml_and_gradient(approx, fx, y, **kwargs):
    """ConjugateGradients: -> (lml, {"variance", "inv_lengthscale" (d,), "diag", "mean_const"}): the gradient with respect to the
    kernel parameters, the noise variance Σy and the constant mean.  wrt_noise=True adds grads["Sigma_y"], (N,): d lml / d σ_i² per point, for fx.Σy a
    scalar or a Diagonal(v) alike (grads["diag"] is its sum).  wrt_inputs=True adds grads["x"] = d lml / d x shaped like fx.x (a
    vector for a plain vector x, (d, N) ColVecs otherwise), from the same solve and the same probes: what a feature map in front of the
    kernel, input warping or latent inputs chain through.  With a CustomMean prior it is the gradient of the kernel part alone:
    d lml / d (y - mean(x)) is the posterior's alpha, and the mean's Jacobian is the caller's.  The estimator is unbiased for the gradient
    but is not the derivative of the estimated value: a caller who trains a flexible map through grads["x"] passes a new seed each step.
    Any other approximation: the existing methods."""
    if not isinstance(approx, ConjugateGradients):
        return _nn.approx_lml_and_gradient(approx, fx, y, **kwargs)
    ctx, dtype = _cg_kwargs("approx_lml_and_gradient", kwargs, also=("wrt_inputs", "wrt_noise"))
    wrt_inputs, wrt_noise = kwargs.get("wrt_inputs", False), kwargs.get("wrt_noise", False)
    if not isinstance(wrt_inputs, (bool, np.bool_)):
        raise ValueError("wrt_inputs is True or False")
    if not isinstance(wrt_noise, (bool, np.bool_)):
        raise ValueError("wrt_noise is True or False")
    dev, desc, keep, probes, delta = _device(approx, fx, y, ctx, dtype)
    try:
        lml, grads, info = dev.lml_grad(desc, probes[0], delta, probes_k=probes[1], wrt_inputs=bool(wrt_inputs), wrt_noise=bool(wrt_noise))
    finally:
        dev.free()
    _warn(info, "the fit")
    if wrt_noise:
        grads["Sigma_y"] = grads.pop("noise")
    if wrt_inputs and np.ndim(fx.x) == 1:
        grads["x"] = grads["x"][0]
    return lml, grads


class CGPosteriorGP:
    """posterior(fx, y) of the exact GP with alpha = (K + Σy)^-1 (y - mean(x)) resident on the device.  Test inputs: a plain vector
    (d = 1) or a (d, n) ColVecs array.  The variance costs one batched solve with k(X, x*) as right-hand sides.  fx = f(x, Diagonal(v)):
    per-point noise variances (svgp_cg_set_noise); predict_y and log_predictive_density then need noise= for the test points."""

    def __init__(self, cg: ConjugateGradients, fx: FiniteGP, y, ctx=None, dtype=None):
        self.approx, self.prior = cg, fx.f
        self.dev, desc, keep, probes, delta = _device(cg, fx, y, ctx, dtype)
        self._desc, self._keep, self._delta = desc, keep, delta   # function_samples solves under the same parameter set
        self.noise = None if isinstance(fx.Sigma_y, Diagonal) else float(fx.Sigma_y)   # None: per-point noise, no single value for y*
        try:
            self.lml, self.info = self.dev.fit(desc, probes[0], delta, probes_k=probes[1])
        except Exception:
            self.dev.free()
            raise
        _warn(self.info, "the fit")

    @property
    def alpha(self):
        return self.dev.alpha()

    def _offsets(self, x, m):
        mu = self.prior.mean_offsets(np.asarray(x))
        return m if mu is None or m is None else (m + mu).astype(m.dtype)

    def mean(self, x):
        return self._offsets(x, self.dev.predict(x, mean=True, var=False)[0])

    def var(self, x):
        _, v, info = self.dev.predict(x, mean=False, var=True)
        _warn(info, "the predictive variance")
        return v

    def mean_and_var(self, x):
        m, v, info = self.dev.predict(x, mean=True, var=True)
        _warn(info, "the predictive variance")
        return self._offsets(x, m), v

    def function_samples(self, n_samples, n_features=2048, rng=None):
        """n_samples pathwise function samples of the exact posterior (svgp_cg_sampler_*): one batched solve of n_samples right-hand
        sides at the posterior's own tol, maxiter and preconditioner, then fs(x) -> (n, S), fs.grad(x) -> (n, S, d), fs.value_and_grad(x)
        at any x, any number of times.  The random numbers come from pathwise.draw_basis(kernel, N, n_features, n_samples, rng)."""
        from .pathwise import draw_basis
        S, L = _check_sample_counts(n_samples, n_features)
        basis = draw_basis(self.prior.kernel, self.dev.n, L, S, rng, _ffi.np_dtype(self.dev.dtype), d=self.dev.d)
        smp = self.dev.sampler(self._desc, basis, self._delta)
        _warn(smp.info, "the function samples")
        return CGFunctionSamples(self, smp)

    def _lik_predictive(self, x, y, want, noise=None):
        if noise is None:
            if self.noise is None:
                raise ValueError("the posterior has per-point noise fx.Σy = Diagonal(v): pass noise=, the observation noise variance of "
                                 "the test points (a scalar or an (n,) array)")
            if not self.noise > 0:
                raise ValueError("predictions of y need observation noise fx.Σy > 0")
            noise = self.noise
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
        """(E[y*], Var[y*]) = (mean, var + noise).  noise: the test points' observation noise variance, a scalar or (n,); the
        posterior's own fx.Σy by default, which a per-point-noise posterior does not have."""
        r = self._lik_predictive(x, None, ("ymean", "yvar"), noise)
        return r["ymean"], r["yvar"]

    def log_predictive_density(self, x, y, noise=None):
        """log N(y*_i; mean_i, var_i + noise_i) per point (noise as in predict_y)"""
        return self._lik_predictive(x, y, ("lpd",), noise)["lpd"]


def posterior(approx, *args, **kwargs):
    """posterior(ConjugateGradients(), fx, y; ctx, dtype) -> CGPosteriorGP; any other approximation: the existing methods.  A Diagonal Σy
    keeps raising UnsupportedError here (existing behaviour): CGPosteriorGP(approx, f(x, Diagonal(v)), y, ctx=, dtype=) is its posterior."""
    if isinstance(approx, ConjugateGradients):
        fx, y = args
        ctx, dtype = _cg_kwargs("posterior", kwargs)
        if isinstance(fx, FiniteGP) and isinstance(fx.Sigma_y, Diagonal):
            # this dispatch has always refused a Diagonal Σy, and callers rely on it: the per-point-noise posterior is asked for by name
            raise _ffi.UnsupportedError("posterior(ConjugateGradients(), f(x, Diagonal(v)), y) is not dispatched: construct "
                                        "CGPosteriorGP(approx, f(x, Diagonal(v)), y) for the exact posterior with per-point noise")
        return CGPosteriorGP(approx, fx, y, ctx=ctx, dtype=dtype)
    return _vfe.posterior(approx, *args, **kwargs)
