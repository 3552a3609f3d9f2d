"""CPU checks of d elbo / d x (svgp_elbo_grad_inputs / svgp_elbo_grad_ext_inputs), no GPU needed: the ABI surface
(symbols, the 24-byte svgp_input_grad, the Julia struct) and the float64 reference the GPU tests compare against
(tests/input_grad_ref.py), pinned by central finite differences of the oracle's elbo()."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import svgp_oracle as o
from approxgp import _ffi
from input_grad_ref import input_grad

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("svgp_elbo_grad_inputs", "svgp_elbo_grad_ext_inputs")


def test_symbols_exported_and_declared():
    header = open(os.path.join(ROOT, "include", "svgp_mi355x.h")).read()
    declared = set(re.findall(r"\b(svgp_[a-z_0-9]+)\s*\(", header))
    lib = _ffi.load_library()
    for name in NEW:
        assert name in declared and name in _ffi.SYMBOLS
        assert hasattr(lib, name)
    assert "typedef struct svgp_input_grad" in header
    assert lib.svgp_version() == 5   # found by symbol: no version step


def test_input_grad_struct_layout():
    assert C.sizeof(_ffi.InputGrad) == 24
    assert [getattr(_ffi.InputGrad, f).offset for f in ("x", "ld", "on_device", "reserved")] == [0, 8, 16, 20]
    src = open(os.path.join(ROOT, "integration", "julia", "src", "SVGPMI355X.jl")).read()
    body = re.search(r"struct InputGrad\b[^\n]*\n(.*?)\nend", src, re.S).group(1)
    fields = re.findall(r"(\w+)::(Int32|Int64|Ptr\{\w+\})", body)
    assert [f for f, _ in fields] == [f[0] for f in _ffi.InputGrad._fields_]
    assert [t for _, t in fields] == ["Ptr{Cvoid}", "Int64", "Int32", "Int32"]


def test_null_context_is_an_argument_error():
    lib = _ffi.load_library()
    out, terms, g = C.c_double(), _ffi.Terms(), _ffi.Grads()
    buf = np.zeros(8)
    gx = _ffi.InputGrad(buf.ctypes.data_as(C.c_void_p), 8, 0, 0)
    assert lib.svgp_elbo_grad_inputs(None, None, None, 0, 8, 0.0, C.byref(out), C.byref(terms), C.byref(g), C.byref(gx)) == _ffi.INVALID_ARG
    gmu = np.zeros(8)
    assert lib.svgp_elbo_grad_ext_inputs(None, None, None, 0, 8, 0.0, 0.0, gmu.ctypes.data_as(C.c_void_p), gmu.ctypes.data_as(C.c_void_p),
                                         C.byref(out), C.byref(terms), C.byref(g), C.byref(gx)) == _ffi.INVALID_ARG


def _fd_x(sva, x, y, kw, h=1e-5):
    g = np.zeros_like(x)
    for idx in np.ndindex(*x.shape):
        xp, xm = x.copy(), x.copy()
        xp[idx] += h
        xm[idx] -= h
        g[idx] = (o.elbo(sva, xp, y, **kw) - o.elbo(sva, xm, y, **kw)) / (2 * h)
    return g


LIKS = [(o.LIK_GAUSSIAN, 0), (o.LIK_BERNOULLI_LOGISTIC, 0), (o.LIK_BERNOULLI_NORMCDF, 0), (o.LIK_POISSON_EXP, 0),
        (o.LIK_EXPONENTIAL_EXP, 0), (o.LIK_GAMMA_EXP, 0)]


@pytest.mark.parametrize("family", [o.KERNEL_SE, o.KERNEL_MATERN32, o.KERNEL_MATERN52])
@pytest.mark.parametrize("lik,qn", LIKS)
@pytest.mark.parametrize("centered", [False, True])
@pytest.mark.parametrize("d", [1, 3, 8])
def test_reference_matches_finite_differences(family, lik, qn, centered, d):
    x, y, nc, s2 = o.synth_problem(60 + 7 * family + d, 23, 6, d, family=family, lik=lik)
    ils = np.linspace(0.7, 1.6, d) * np.asarray(nc.kernel.inv_lengthscale, dtype=np.float64)   # ARD
    k = o.Kernel(family, nc.kernel.variance, ils)
    if centered:
        sva = o.SVA(k, nc.z, nc.m + 0.3, 0.7 * nc.Lq, jitter=1e-4, mean_const=0.25, centered=True)
    else:
        sva = o.SVA(k, nc.z, nc.m, nc.Lq, jitter=nc.jitter, mean_const=0.25)
    kw = dict(lik=lik, sigma2=s2, num_data=61.0, quadrature_n=qn)
    ref = input_grad(sva, x, y, **kw)
    fd = _fd_x(sva, np.asarray(x, dtype=np.float64).reshape(d, -1), y, kw)
    scale = np.abs(fd).max()
    assert scale > 0
    assert np.abs(ref - fd).max() <= 1e-6 * scale, (np.abs(ref - fd).max(), scale)


@pytest.mark.parametrize("family", [o.KERNEL_SE, o.KERNEL_MATERN52])
@pytest.mark.parametrize("centered", [False, True])
def test_translation_identity(family, centered):
    """A stationary ELBO does not change when x and z shift together: sum_j x_bar_j + sum_i z_bar_i = 0."""
    x, y, nc, s2 = o.synth_problem(91 + family, 50, 9, 3, family=family, lik=o.LIK_POISSON_EXP)
    sva = o.SVA(nc.kernel, nc.z, nc.m + 0.1, nc.Lq, jitter=1e-4 if centered else nc.jitter, mean_const=-0.2, centered=centered)
    kw = dict(lik=o.LIK_POISSON_EXP, sigma2=s2, num_data=120.0)
    xb = input_grad(sva, x, y, **kw)
    _, g = o.elbo_grad(sva, x, y, **kw)
    total = xb.sum(1) + g["z"].sum(1)
    assert np.abs(total).max() <= 1e-10 * max(np.abs(xb).sum(1).max(), np.abs(g["z"]).sum(1).max())


def test_elbo_grad_inputs_rejects_shard_form():
    """inputs= and shard= together: the shard form has no x gradient (checked before the library is called)."""
    model = _ffi.DeviceModel.__new__(_ffi.DeviceModel)
    model.M, model.d, model.dtype = 4, 1, _ffi.F64

    class _Data:
        n, d, layout = 8, 1, _ffi.VEC

    with pytest.raises(ValueError):
        model.elbo_grad(_Data(), 0, 8, 0.0, shard=(1.0, 1.0), inputs=True)
