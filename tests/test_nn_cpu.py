"""CPU pins of tests/nn_ref.py, the float64 restatement of the reference's NearestNeighbors approximation that tests/test_gpu_nn.py
compares the device against, and the argument checks of the Python mirror (no GPU)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import nn_ref as nr
import svgp_oracle as o
from approxgp import GP, CustomMean, NearestNeighbors, SEKernel, _ffi, approx_lml, approx_lml_and_gradient, posterior

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# test/NearestNeighborsModule.jl:2-6
XR = np.array([1.0, 2.0, 3.5, 4.2, 5.9, 8.0])
YR = np.sin(XR)
UNIT = nr.kernel_of(o.KERNEL_SE, 1.0, [1.0])


def test_reference_data_values():
    v3 = nr.lml(UNIT, XR, YR, 3)
    assert abs(v3 - (-6.070853690320693)) <= 1e-12
    assert abs(nr.lml_joint(UNIT, XR, YR, 3) - v3) <= 1e-13
    v5 = nr.lml(UNIT, XR, YR, 5)
    assert abs(v5 - (-6.073251508326499)) <= 1e-11
    assert abs(nr.exact_lml(UNIT, XR, YR, 0.0) - v5) <= 1e-11


def test_reference_assertions():
    """test/NearestNeighborsModule.jl: mean_and_cov at 1.0:0.1:8 against the exact GP (atol 1e-4 for k = 5, 1e-1 for k = 3), lml atol 1e-2"""
    xs = np.arange(1.0, 8.0 + 1e-9, 0.1)
    em, ec = nr.exact_predict(UNIT, XR, YR, 0.0, xs)
    for k, atol in ((5, 1e-4), (3, 1e-1)):
        cache = nr.fit(UNIT, XR, YR, k)
        m, v, c = nr.predict(cache, UNIT, XR, xs)
        np.testing.assert_allclose(m, em, rtol=0, atol=atol)
        np.testing.assert_allclose(c, ec, rtol=0, atol=atol)
        np.testing.assert_allclose(v, np.diag(c), rtol=0, atol=1e-13)
    assert abs(nr.lml(UNIT, XR, YR, 3) - nr.exact_lml(UNIT, XR, YR, 0.0)) <= 1e-2


def test_all_neighbours_is_the_exact_gp_with_noise():
    n, d, diag = 40, 2, 1e-2
    x, y = nr.synth(n, d, seed=1)
    kern = nr.kernel_of(o.KERNEL_MATERN52, 1.2, [0.8, 1.1])
    cache = nr.fit(kern, x, y, n - 1, diag, mean_const=0.3)
    ex = nr.exact_lml(kern, x, y, diag, mean_const=0.3)
    assert abs(cache["lml"] - ex) <= 1e-12 * abs(ex)
    assert abs(nr.lml(kern, x, y, n + 5, diag, mean_const=0.3) - ex) <= 1e-12 * abs(ex)   # k >= n is k = n - 1
    xs = np.random.default_rng(2).uniform(-2, 2, size=(d, 30))
    m, v, c = nr.predict(cache, kern, x, xs)
    em, ec = nr.exact_predict(kern, x, y, diag, xs, mean_const=0.3)
    np.testing.assert_allclose(m, em, rtol=0, atol=1e-11)
    np.testing.assert_allclose(c, ec, rtol=0, atol=1e-11)
    ys = xs[:, :7] + 0.1
    _, _, cx = nr.predict(cache, kern, x, xs, ys)
    K = o.kernelmatrix(kern, x) + diag * np.eye(n)
    ecx = o.kernelmatrix(kern, xs, ys) - o.kernelmatrix(kern, x, xs).T @ np.linalg.solve(K, o.kernelmatrix(kern, x, ys))
    np.testing.assert_allclose(cx, ecx, rtol=0, atol=1e-11)


@pytest.mark.parametrize("family", [o.KERNEL_SE, o.KERNEL_MATERN32, o.KERNEL_MATERN52])
def test_two_formulations_and_float32(family):
    """the figures the GPU tolerances rest on: per-point solve vs joint Cholesky <= 5e-14 relative, float32 within 1e-5 of float64"""
    for k, d in ((16, 1), (33, 3), (64, 8)):
        x, y = nr.synth(300, d, seed=10 + k)
        kern = nr.kernel_of(family, 1.2, nr.invl_for(d, True))
        a, b = nr.lml(kern, x, y, k, 1e-2), nr.lml_joint(kern, x, y, k, 1e-2)
        assert abs(a - b) <= 5e-14 * abs(a)
        x32, y32 = x.astype(np.float32), y.astype(np.float32)
        c = nr.lml(kern, x32, y32, k, 1e-2, dtype=np.float32)
        assert abs(c - nr.lml(kern, x32, y32, k, 1e-2)) <= 1e-5 * abs(a)


@pytest.mark.parametrize("family", [o.KERNEL_SE, o.KERNEL_MATERN32, o.KERNEL_MATERN52])
def test_gradient_against_central_differences(family):
    n, d, k = 60, 3, 7
    x, y = nr.synth(n, d, seed=5 + family)
    var, il, diag, mc = 1.2, np.array([0.8, 0.95, 1.1]), 1e-2, 0.2
    val, gv, gil, gd = nr.lml_grad(nr.kernel_of(family, var, il), x, y, k, diag, mc)
    assert abs(val - nr.lml(nr.kernel_of(family, var, il), x, y, k, diag, mc)) <= 1e-12 * abs(val)
    f = lambda v, l, dg: nr.lml(nr.kernel_of(family, v, l), x, y, k, dg, mc)
    h = 1e-6
    fd = [(f(var + h, il, diag) - f(var - h, il, diag)) / (2 * h)]
    fd += [(f(var, il + h * e, diag) - f(var, il - h * e, diag)) / (2 * h) for e in np.eye(d)]
    fd += [(f(var, il, diag + h * 1e-2) - f(var, il, diag - h * 1e-2)) / (2 * h * 1e-2)]
    g = np.concatenate([[gv], gil, [gd]])
    np.testing.assert_allclose(g, np.array(fd), rtol=2e-6, atol=1e-6 * np.max(np.abs(g[:-1])))


def test_banded_layout():
    B, F = nr.factors(UNIT, XR, 3)
    band = nr.banded(B, 3)
    assert band.shape == (6, 3)
    assert np.all(band[0] == 0) and band[1, 0] == 0 and band[1, 1] == 0 and band[1, 2] == B[1, 0]
    assert np.array_equal(band[4], B[4, 1:4])
    assert F[0] == 1.0


def test_mirror_argument_checks_happen_before_the_gpu():
    with pytest.raises(ValueError):
        NearestNeighbors(0)
    f = GP(SEKernel())
    with pytest.raises(_ffi.UnsupportedError):
        approx_lml(NearestNeighbors(3, include_noise=True), f(XR, np.full(6, 0.1)), YR)
    g = GP(CustomMean(lambda x: np.zeros(len(x))), SEKernel())
    for fn in (approx_lml, approx_lml_and_gradient, posterior):
        with pytest.raises(_ffi.UnsupportedError):
            fn(NearestNeighbors(3), g(XR), YR)
    with pytest.raises(TypeError):
        approx_lml(NearestNeighbors(3), f(XR), YR, num_data=3)
    with pytest.raises(ValueError):
        approx_lml(NearestNeighbors(3), f(XR), YR[:5])


def test_struct_sizes_match_the_header_and_the_julia_binding():
    assert C.sizeof(_ffi.NNDesc) == 56 and _ffi.NNDesc.variance.offset == 16 and _ffi.NNDesc.reserved.offset == 48
    assert C.sizeof(_ffi.NNInfo) == 24 and _ffi.NNInfo.lml.offset == 16
    hdr = open(os.path.join(ROOT, "include", "svgp_mi355x.h")).read()
    assert re.search(r"\} svgp_nn_desc;\s*/\* 56 bytes \*/", hdr) and re.search(r"\} svgp_nn_info;\s*/\* 24 bytes \*/", hdr)
    body = hdr[hdr.index("typedef struct svgp_nn_desc {"):hdr.index("} svgp_nn_desc;")]
    names = re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert names == [f[0] for f in _ffi.NNDesc._fields_]
    jl = open(os.path.join(ROOT, "integration", "julia", "src", "SVGPMI355X.jl")).read()
    jl_fields = re.findall(r"(\w+)::(?:Int32|Int64|Float64|Ptr\{\w+\})", jl[jl.index("struct NNDesc"):jl.index("struct NNInfo")])
    assert jl_fields == [f[0] for f in _ffi.NNDesc._fields_]
    tests_jl = open(os.path.join(ROOT, "integration", "julia", "test", "runtests.jl")).read()
    assert "sizeof(MI.NNDesc) == 56" in tests_jl and "sizeof(MI.NNInfo) == 24" in tests_jl
