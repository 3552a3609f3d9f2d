"""Pathwise posterior function samples (Wilson et al. 2020, Matheron's rule) over svgp_sampler_* of libsvgp_mi355x.so:

    f(.) = mean(.) + Phi(.) w + k(., z) V,    V = Kuu^-1 (u - mean(z) - Phi(z) w),    u ~ q(u)

with Phi the L random Fourier features phi_l(x) = sqrt(2 variance / L) cos(omega_l . (x / lengthscale) + tau_l) of the prior.  The library
draws nothing; this module draws the random numbers (draw_basis) and hands them over.  The Fourier part approximates the prior with a
covariance error of O(variance / sqrt(L)); the update term is exact."""
from __future__ import annotations

import numpy as np

from . import _ffi
from .kernels import ARDTransform, ScaledKernel, TransformedKernel, unpack_kernel

# 2 nu of the Matern families: omega is multivariate Student-t with that many degrees of freedom (SE: the limit, a normal)
MATERN_DOF = {_ffi.KERNEL_MATERN32: 3, _ffi.KERNEL_MATERN52: 5}


def _family_and_d(kernel, d):
    if isinstance(kernel, (int, np.integer)):
        return int(kernel), (1 if d is None else int(d))
    k = kernel.kernel if isinstance(kernel, ScaledKernel) else kernel
    if d is None:
        t = k.transform if isinstance(k, TransformedKernel) else None
        d = len(t.v) if isinstance(t, ARDTransform) else 1
    return unpack_kernel(kernel, int(d))[0], int(d)


def draw_basis(kernel, M, n_features, n_samples, rng=None, dtype=np.float64, d=None):
    """The random numbers of `n_samples` function samples with `n_features` Fourier features for a model with M inducing points:
    -> (omega (L, d), tau (L,), w (S, L), eps (S, M)) in `dtype`.  omega are frequencies of the UNIT-lengthscale base kernel of `kernel`
    (a kernel object of approxgp.kernels or a family code; the library applies the lengthscales): SE omega ~ N(0, I), Matern-nu
    omega = g sqrt(2 nu / chi2_{2 nu}) with g ~ N(0, I) and one chi-square draw per feature.  tau ~ U[0, 2 pi); w, eps ~ N(0, 1).
    d: the input dimension, when `kernel` does not carry it (no ARDTransform); default 1."""
    family, d = _family_and_d(kernel, d)
    if family not in (_ffi.KERNEL_SE, _ffi.KERNEL_MATERN32, _ffi.KERNEL_MATERN52):
        raise _ffi.UnsupportedError(f"unsupported kernel family {family}")
    L, S, M = int(n_features), int(n_samples), int(M)
    if L < 0 or S < 1 or M < 1:
        raise ValueError("n_features >= 0, n_samples >= 1 and M >= 1")
    rng = rng if rng is not None else np.random.default_rng()
    dt = _ffi.np_dtype(_ffi.dtype_code(dtype))
    omega = rng.standard_normal((L, d))
    dof = MATERN_DOF.get(family)
    if dof is not None:
        omega *= np.sqrt(dof / rng.chisquare(dof, size=(L, 1)))
    tau = rng.uniform(0.0, 2.0 * np.pi, size=L)
    w = rng.standard_normal((S, L))
    eps = rng.standard_normal((S, M))
    return omega.astype(dt), tau.astype(dt), w.astype(dt), eps.astype(dt)


class FunctionSamples:
    """S functions drawn from an ApproxPosteriorGP, resident on the device: fs(x) -> (n, S), at any x, any number of times - the same
    functions every time (a point's value does not depend on the other points of the call)."""

    def __init__(self, post, basis):
        self._post = post
        self.sampler = post._model.sampler(basis)
        self.n_samples = self.sampler.n_samples

    def __call__(self, x):
        post = self._post
        data = _ffi.DeviceData(post.ctx, x, None, _ffi.np_dtype(self.sampler.dtype))
        try:
            return np.ascontiguousarray(self.sampler.eval(data, prior_mean=post.prior.mean_offsets(x)).T)
        finally:
            data.free()

    def _eval_grad(self, x, values):
        post = self._post
        data = _ffi.DeviceData(post.ctx, x, None, _ffi.np_dtype(self.sampler.dtype))
        try:
            F, G = self.sampler.eval_grad(data, prior_mean=post.prior.mean_offsets(x) if values else None, values=values)
        finally:
            data.free()
        return (np.ascontiguousarray(F.T) if values else None), np.ascontiguousarray(G.transpose(2, 0, 1))

    def grad(self, x):
        """-> (n, S, d): [j, s, c] = d f_s / d x_c at x_j (svgp_sampler_eval_grad), the gradient of f_s minus the prior mean: a
        non-constant mean function's own Jacobian is the caller's to add (the constant mean contributes nothing)."""
        return self._eval_grad(x, False)[1]

    def value_and_grad(self, x):
        """-> (fs(x) (n, S), grad(x) (n, S, d)) from one call; the values are bitwise those of fs(x)."""
        return self._eval_grad(x, True)

    def state(self):
        return self.sampler.state()

    def free(self):
        self.sampler.free()


def function_samples(post, n_samples, n_features=2048, rng=None):
    """ApproxPosteriorGP.function_samples: n_samples pathwise function samples of `post`, their random numbers drawn from rng."""
    z = np.asarray(post.approx.fz.x)
    d, M = (1, z.shape[0]) if z.ndim == 1 else z.shape
    basis = draw_basis(post.prior.kernel, M, n_features, n_samples, rng, _ffi.np_dtype(post._model.dtype), d=d)
    return FunctionSamples(post, basis)
