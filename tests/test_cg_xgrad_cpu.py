"""CPU checks (no GPU) of the input gradient of the exact GP by conjugate gradients: the float64 restatement tests/cg_xgrad_ref.py
against central differences of the oracle's dense exact GP, the estimator's two identities, and the Python layer's argument checks."""
import ctypes as C

import numpy as np
import pytest

import approxgp
import cg_ref as cr
import cg_xgrad_ref as xr
import svgp_oracle as o
from approxgp import _ffi

FAMILIES = [o.KERNEL_SE, o.KERNEL_MATERN32, o.KERNEL_MATERN52]


def _problem(N, d, family, seed=0):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-3, 3, size=(d, N))
    kernel = o.Kernel(family, 1.3, np.array([1 / 0.7, 1 / 0.9, 1 / 1.1, 1 / 0.8][:d]))
    y = np.sin(x.sum(0)) + 0.1 * rng.standard_normal(N)
    return kernel, x, y


@pytest.mark.parametrize("family", FAMILIES)
def test_unit_probe_input_gradient_equals_central_differences(family):
    N, d = 37, 3
    kernel, x, y = _problem(N, d, family)
    g = xr.estimate(kernel, x, 0.1, y, cr.unit_probes(N), 1e-12, 2000)["grad"]["x"]
    fd = xr.central_differences(kernel, x, 0.1, y)
    err = np.abs(g - fd).max() / np.abs(fd).max()
    print(f"family {family}: unit-probe x_bar against central differences {err:.2e}")
    assert g.shape == (d, N) and err <= 1e-6, err


@pytest.mark.parametrize("family", FAMILIES)
def test_translation_and_scaling_identities_for_any_probes(family):
    N, d = 65, 3
    kernel, x, y = _problem(N, d, family, seed=2)
    x = x + 5.0   # the identities do not care where the data sit
    r = xr.estimate(kernel, x, 0.1, y, approxgp.draw_probes(N, 5, 3), 1e-12, 2000)
    g = r["grad"]["x"]
    scale = np.abs(g).sum(1)
    assert np.all(np.abs(g.sum(1)) <= 1e-12 * scale), (g.sum(1), scale)
    lhs, rhs = (x * g).sum(1), kernel.inv_lengthscale * r["grad"]["inv_lengthscale"]
    assert np.all(np.abs(lhs - rhs) <= 1e-12 * (np.abs(x) * np.abs(g)).sum(1)), (lhs, rhs)


def test_preconditioned_restatement_keeps_the_identities_and_the_exact_gradient():
    N, d, k = 37, 2, 8
    kernel, x, y = _problem(N, d, o.KERNEL_MATERN52, seed=4)
    zp = x[:, np.random.default_rng(5).choice(N, size=k, replace=False)]
    import cg_precond_ref as pr
    eps, xi = pr.exact_probes(N, k)
    r = xr.estimate_precond(kernel, x, zp, 0.1, y, eps, xi, 1e-13, 2000)
    fd = xr.central_differences(kernel, x, 0.1, y)
    assert np.abs(r["x"] - fd).max() <= 1e-6 * np.abs(fd).max()
    r = xr.estimate_precond(kernel, x, zp, 0.1, y, approxgp.draw_probes(N, 4, 1), approxgp.draw_probes(k, 4, 2), 1e-13, 2000)
    assert np.all(np.abs(r["x"].sum(1)) <= 1e-12 * np.abs(r["x"]).sum(1))
    lhs, rhs = (x * r["x"]).sum(1), kernel.inv_lengthscale * r["inv_lengthscale"]
    assert np.all(np.abs(lhs - rhs) <= 1e-12 * (np.abs(x) * np.abs(r["x"])).sum(1)), (lhs, rhs)


def test_float32_restatement_is_the_float64_one_to_float32_accuracy():
    kernel, x, y = _problem(65, 3, o.KERNEL_MATERN32, seed=6)
    x = x.astype(np.float32).astype(np.float64)
    z = approxgp.draw_probes(65, 4, 1)
    r = cr.estimate(kernel, x, 0.1, y, z, 1e-10, 2000)
    g64 = xr.x_bar(kernel, x, r["alpha"], r["W"], z)
    g32 = xr.x_bar(kernel, x, r["alpha"], r["W"], z, np.float32)
    assert np.abs(g32 - g64).max() <= 1e-5 * np.abs(g64).max()


def test_ffi_declares_the_entry_point():
    res, args = _ffi.SYMBOLS["svgp_cg_lml_grad_inputs"]
    pre = _ffi.SYMBOLS["svgp_cg_lml_grad_precond"][1]
    assert res is C.c_int32 and list(args[:-1]) == list(pre) and args[-1]._type_ is _ffi.InputGrad   # _precond's list plus gx
    assert C.sizeof(_ffi.InputGrad) == 24


class _NoGpu:
    """stands in for a context: any use of the library is an error"""

    def __getattr__(self, name):
        raise AssertionError("the GPU was touched")


def _handle(n=9, d=2, precond_k=0):
    dev = approxgp.DeviceConjugateGradients.__new__(approxgp.DeviceConjugateGradients)
    dev.ctx, dev.h, dev.data = _NoGpu(), None, None
    dev.n, dev.d, dev.dtype, dev.precond_k = n, d, _ffi.dtype_code(np.float64), precond_k
    return dev


def test_python_argument_errors_need_no_context(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the GPU was touched")

    monkeypatch.setattr(_ffi, "default_context", boom)
    f = approxgp.GP(approxgp.SqExponentialKernel())
    x, y = np.linspace(0, 1, 9), np.zeros(9)
    cg = approxgp.ConjugateGradients()
    # wrt_inputs is a keyword of the ConjugateGradients method now: the first complaint is about the data
    with pytest.raises(ValueError, match="lengths differ"):
        approxgp.approx_lml_and_gradient(cg, f(x, 0.1), np.zeros(8), wrt_inputs=True)
    with pytest.raises(ValueError, match="wrt_inputs"):
        approxgp.approx_lml_and_gradient(cg, f(x, 0.1), y, wrt_inputs="yes")
    with pytest.raises(_ffi.UnsupportedError):
        approxgp.approx_lml_and_gradient(cg, f(x, np.full(9, 0.1)), y, wrt_inputs=True)
    with pytest.raises(TypeError, match="unexpected keyword"):
        approxgp.approx_lml_and_gradient(cg, f(x, 0.1), y, wrt_inputs=True, wrt_outputs=True)
    with pytest.raises(TypeError, match="unexpected keyword"):
        approxgp.approx_lml(cg, f(x, 0.1), y, wrt_inputs=True)   # the value alone has no gradient to extend
    dev, desc, z = _handle(), _ffi.CGDesc(), np.ones((9, 2))
    with pytest.raises(ValueError, match="wrt_inputs"):
        dev.lml_grad(desc, z, wrt_inputs=1)
    with pytest.raises(ValueError, match="x_grad_out needs"):
        dev.lml_grad(desc, z, x_grad_out=np.zeros((2, 9)))
    with pytest.raises(ValueError, match="x_grad_out: a contiguous"):
        dev.lml_grad(desc, z, wrt_inputs=True, x_grad_out=np.zeros((2, 9)))   # a host array is not a device tensor
    with pytest.raises(ValueError, match="delta"):
        dev.lml_grad(desc, z, delta=np.zeros(8), wrt_inputs=True)
    with pytest.raises(ValueError, match="no preconditioner"):
        dev.lml_grad(desc, z, probes_k=np.ones((4, 2)), wrt_inputs=True)
    with pytest.raises(ValueError, match="probes need probes_k"):
        _handle(precond_k=4).lml_grad(desc, z, wrt_inputs=True)
    with pytest.raises(TypeError, match="DeviceData"):
        approxgp.DeviceConjugateGradients(_NoGpu(), data=np.zeros((2, 9)))
    with pytest.raises(ValueError, match="needs x and dtype"):
        approxgp.DeviceConjugateGradients(_NoGpu())
    held = _ffi.DeviceData.__new__(_ffi.DeviceData)
    held.h = None
    with pytest.raises(ValueError, match="freed"):
        approxgp.DeviceConjugateGradients(_NoGpu(), data=held)
    held.h = C.c_void_p(1)
    with pytest.raises(ValueError, match="replaces"):
        approxgp.DeviceConjugateGradients(_NoGpu(), x=np.zeros((2, 9)), data=held)
    held.h = None
