"""CPU checks of prior mean offsets (svgp_model_set_mean_z, svgp_elbo_with_mean, svgp_marginals_with_mean, svgp_elbo_grad_with_mean),
no GPU needed: the ABI surface and the float64 reference the GPU tests compare against (tests/prior_mean_ref.py), pinned three ways -
against the unchanged oracle for constant offsets, by the Gaussian shift identity, and by central finite differences of every block."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import prior_mean_ref as pmr
import svgp_oracle as o
from approxgp import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("svgp_model_set_mean_z", "svgp_elbo_with_mean", "svgp_marginals_with_mean", "svgp_elbo_grad_with_mean")
LIKS = [(o.LIK_GAUSSIAN, 0), (o.LIK_BERNOULLI_LOGISTIC, 0), (o.LIK_BERNOULLI_NORMCDF, 0), (o.LIK_POISSON_EXP, 0),
        (o.LIK_EXPONENTIAL_EXP, 0), (o.LIK_GAMMA_EXP, 0), (o.LIK_GAUSSIAN, 9), (o.LIK_POISSON_EXP, 7)]
BLOCKS = ("variance", "inv_lengthscale", "z", "m", "Lq", "lik_sigma2", "mean_const")


def test_symbols_exported_and_declared():
    header = open(os.path.join(ROOT, "include", "svgp_mi355x.h")).read()
    declared = set(re.findall(r"\b(svgp_[a-z_0-9]+)\s*\(", header))
    lib = _ffi.load_library()
    for name in NEW:
        assert name in declared and name in _ffi.SYMBOLS
        assert hasattr(lib, name)
    assert "typedef struct svgp_point_mean" in header and "typedef struct svgp_point_mean_grad" in header
    assert lib.svgp_version() == 5   # found by symbol: no version step


def test_ctypes_signatures_match_the_header():
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "svgp_mi355x.h")).read(), flags=re.S)
    for name in NEW:
        args = re.search(name + r"\s*\(([^;]*?)\)\s*;", hdr, re.S).group(1)
        params = [" ".join(p.split()) for p in args.split(",")]
        _, argt = _ffi.SYMBOLS[name]
        assert len(params) == len(argt), name
        for p, t in zip(params, argt):
            if "*" in p:
                assert t is C.c_void_p or t is C.c_char_p or hasattr(t, "_type_") and not isinstance(t._type_, str), (name, p, t)
            else:
                want = {"int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double}[p.replace("const ", "").split()[0]]
                assert t is want, (name, p, t)


def test_struct_layouts():
    assert C.sizeof(_ffi.PointMean) == 16 and C.sizeof(_ffi.PointMeanGrad) == 16
    assert [getattr(_ffi.PointMean, f).offset for f in ("mu", "on_device", "reserved")] == [0, 8, 12]
    assert [getattr(_ffi.PointMeanGrad, f).offset for f in ("mu_bar", "on_device", "reserved")] == [0, 8, 12]
    src = open(os.path.join(ROOT, "integration", "julia", "src", "SVGPMI355X.jl")).read()
    for jl, py in (("PointMean", _ffi.PointMean), ("PointMeanGrad", _ffi.PointMeanGrad)):
        body = re.search(r"struct " + jl + r"\b[^\n]*\n(.*?)\nend", src, re.S).group(1)
        fields = re.findall(r"(\w+)::(Int32|Int64|Ptr\{\w+\})", body)
        assert [f for f, _ in fields] == [f[0] for f in py._fields_]
        assert [t for _, t in fields] == ["Ptr{Cvoid}", "Int32", "Int32"]


def test_null_context_is_an_argument_error():
    lib = _ffi.load_library()
    buf = np.zeros(8)
    pm = _ffi.PointMean(buf.ctypes.data_as(C.c_void_p), 0, 0)
    out, terms, g = C.c_double(), _ffi.Terms(), _ffi.Grads()
    assert lib.svgp_model_set_mean_z(None, None, None) == _ffi.INVALID_ARG
    assert lib.svgp_elbo_with_mean(None, None, None, 0, 8, 0.0, C.byref(pm), C.byref(out), C.byref(terms)) == _ffi.INVALID_ARG
    assert lib.svgp_marginals_with_mean(None, None, None, 0, 8, C.byref(pm), None, None) == _ffi.INVALID_ARG
    assert lib.svgp_elbo_grad_with_mean(None, None, None, 0, 8, 0.0, C.byref(pm), 0.0, None, None, C.byref(out), C.byref(terms),
                                        C.byref(g), None, None) == _ffi.INVALID_ARG


def _problem(seed, n, M, d, family=o.KERNEL_SE, lik=o.LIK_GAUSSIAN, centered=False):
    x, y, nc, s2 = o.synth_problem(seed, n, M, d, family=family, lik=lik)
    ils = np.linspace(0.7, 1.6, d) * np.asarray(nc.kernel.inv_lengthscale, dtype=np.float64)
    k = o.Kernel(family, nc.kernel.variance, ils)
    if centered:
        sva = o.SVA(k, nc.z, nc.m + 0.3, 0.7 * nc.Lq, jitter=1e-4, mean_const=0.25, centered=True)
    else:
        sva = o.SVA(k, nc.z, nc.m, nc.Lq, jitter=nc.jitter, mean_const=0.25)
    rng = np.random.default_rng(seed)
    mux = 0.3 * rng.standard_normal(n)
    muz = 0.4 * rng.standard_normal(M)
    if lik in (o.LIK_POISSON_EXP, o.LIK_EXPONENTIAL_EXP, o.LIK_GAMMA_EXP):   # keep exp(mu) tame for the differences
        mux *= 0.5
    return np.asarray(x, dtype=np.float64).reshape(d, -1), y, sva, s2, mux, muz


def _with(sva, **kw):
    f = dict(kernel=sva.kernel, z=sva.z, m=sva.m, Lq=sva.Lq, jitter=sva.jitter, mean_const=sva.mean_const, centered=sva.centered)
    f.update(kw)
    return o.SVA(f["kernel"], f["z"], f["m"], f["Lq"], jitter=f["jitter"], mean_const=f["mean_const"], centered=f["centered"])


@pytest.mark.parametrize("lik,qn", LIKS)
@pytest.mark.parametrize("centered", [False, True])
def test_constant_offsets_equal_the_oracle(lik, qn, centered):
    """mux = muz = delta (constant vectors): the oracle with mean_const = c + delta, value and every gradient block."""
    x, y, sva, s2, _, _ = _problem(11 + 3 * LIKS.index((lik, qn)), 40, 7, 2, lik=lik, centered=centered)
    delta = -0.35
    kw = dict(lik=lik, sigma2=s2, num_data=97.0, quadrature_n=qn)
    v, g = pmr.elbo_grad(sva, x, y, np.full(40, delta), np.full(7, delta), **kw)
    vo, go = o.elbo_grad(_with(sva, mean_const=sva.mean_const + delta), x, y, **kw)
    assert abs(v - vo) <= 1e-12 * abs(vo)
    for b in BLOCKS:
        np.testing.assert_allclose(g[b], go[b], rtol=1e-10, atol=1e-12 * max(np.abs(go[b]).max(), 1.0), err_msg=b)
    assert abs(g["mean_const"] - (g["mean_x"].sum() + g["mean_z"].sum())) <= 1e-12 * max(abs(g["mean_const"]), 1.0)


@pytest.mark.parametrize("centered", [False, True])
@pytest.mark.parametrize("family", [o.KERNEL_SE, o.KERNEL_MATERN32, o.KERNEL_MATERN52])
def test_gaussian_shift_identity(centered, family):
    """Gaussian likelihood: the ELBO at (mux, muz, m, y) is the oracle's at zero offsets, y - mux and (Centered) m - muz.  NonCentered
    muz has no effect (alpha = Lk' \\ m), so there the oracle keeps m."""
    x, y, sva, s2, mux, muz = _problem(31 + family, 45, 8, 3, family=family, centered=centered)
    v = pmr.elbo(sva, x, y, mux, muz, sigma2=s2, num_data=150.0)
    shifted = _with(sva, m=sva.m - muz) if centered else sva
    vo = o.elbo(shifted, x, y - mux, sigma2=s2, num_data=150.0)
    assert abs(v - vo) <= 1e-12 * abs(vo)
    mu, var = pmr.marginals(sva, x, mux, muz)
    post = o.posterior(shifted)
    mo, vo2 = o.mean_and_var(post, x)
    np.testing.assert_allclose(mu - mux, mo, rtol=0, atol=1e-12 * np.abs(mo).max())
    np.testing.assert_allclose(var, vo2 + o.DEFAULT_SIGMA2, rtol=1e-12)


def _fd(fun, a, h):
    g = np.zeros(np.shape(a))
    for idx in np.ndindex(*np.shape(a)):
        ap, am = np.array(a, dtype=np.float64), np.array(a, dtype=np.float64)
        ap[idx] += h
        am[idx] -= h
        g[idx] = (fun(ap) - fun(am)) / (2 * h)
    return g


@pytest.mark.parametrize("lik,qn", LIKS)
@pytest.mark.parametrize("centered", [False, True])
def test_reference_matches_finite_differences(lik, qn, centered):
    i = LIKS.index((lik, qn))
    family = (o.KERNEL_SE, o.KERNEL_MATERN32, o.KERNEL_MATERN52)[i % 3]
    n, M, d = 19, 5, 2
    x, y, sva, s2, mux, muz = _problem(50 + i + 10 * centered, n, M, d, family=family, lik=lik, centered=centered)
    kw = dict(lik=lik, sigma2=s2, num_data=61.0, quadrature_n=qn)
    _, g = pmr.elbo_grad(sva, x, y, mux, muz, **kw)
    k = sva.kernel
    h = 1e-6
    fds = {
        "mean_x": _fd(lambda a: pmr.elbo(sva, x, y, a, muz, **kw), mux, h),
        "mean_z": _fd(lambda a: pmr.elbo(sva, x, y, mux, a, **kw), muz, h),
        "mean_const": _fd(lambda a: pmr.elbo(_with(sva, mean_const=float(a[0])), x, y, mux, muz, **kw), [sva.mean_const], h)[0],
        "m": _fd(lambda a: pmr.elbo(_with(sva, m=a), x, y, mux, muz, **kw), sva.m, h),
        "z": _fd(lambda a: pmr.elbo(_with(sva, z=a), x, y, mux, muz, **kw), sva.z, h),
        "variance": _fd(lambda a: pmr.elbo(_with(sva, kernel=o.Kernel(k.family, float(a[0]), k.inv_lengthscale)), x, y, mux, muz, **kw),
                        [k.variance], h)[0],
        "inv_lengthscale": _fd(lambda a: pmr.elbo(_with(sva, kernel=o.Kernel(k.family, k.variance, a)), x, y, mux, muz, **kw),
                               k.inv_lengthscale, h),
    }
    if lik in (o.LIK_GAUSSIAN, o.LIK_GAMMA_EXP):
        fds["lik_sigma2"] = _fd(lambda a: pmr.elbo(sva, x, y, mux, muz, **dict(kw, sigma2=float(a[0]))), [s2], h)[0]
    Lq0 = np.tril(sva.Lq).astype(np.float64)
    fdL = np.zeros_like(Lq0)
    for r, c in zip(*np.tril_indices(M)):
        Lp, Lm = Lq0.copy(), Lq0.copy()
        Lp[r, c] += h
        Lm[r, c] -= h
        fdL[r, c] = (pmr.elbo(_with(sva, Lq=Lp), x, y, mux, muz, **kw) - pmr.elbo(_with(sva, Lq=Lm), x, y, mux, muz, **kw)) / (2 * h)
    fds["Lq"] = fdL
    for b, fd in fds.items():
        scale = max(np.abs(fd).max(), 1e-3)
        err = np.abs(np.asarray(g[b]) - fd).max()
        assert err <= 2e-6 * scale, (b, err, scale)
    if not centered:
        assert np.all(g["mean_z"] == 0.0)
    else:
        np.testing.assert_array_equal(g["mean_z"], -g["m"])
    assert abs(g["mean_const"] - (g["mean_x"].sum() + g["mean_z"].sum())) <= 1e-12 * max(abs(g["mean_const"]), 1.0)


def test_caller_point_gradients_route():
    """point_grads = the built-in likelihood's own (sum_e, g_mu, g_v) at the shifted marginals: the same gradient."""
    x, y, sva, s2, mux, muz = _problem(71, 30, 6, 2, lik=o.LIK_POISSON_EXP, centered=True)
    v, g = pmr.elbo_grad(sva, x, y, mux, muz, lik=o.LIK_POISSON_EXP, num_data=90.0)
    mu, var = pmr.marginals(sva, x, mux, muz)
    e = o.expected_loglik(o.LIK_POISSON_EXP, mu, np.sqrt(var), y, 1.0)
    gmu, gv, _ = o.expected_loglik_grads(o.LIK_POISSON_EXP, mu, var, y, 1.0)
    ve, ge = pmr.elbo_grad(sva, x, None, mux, muz, num_data=90.0, point_grads=(e, gmu, gv))
    assert abs(v - ve) <= 1e-13 * abs(v)
    for b in ("variance", "inv_lengthscale", "z", "m", "Lq", "mean_const", "mean_x", "mean_z"):
        np.testing.assert_allclose(ge[b], g[b], rtol=1e-12, atol=1e-14, err_msg=b)


def test_with_mean_rejects_shard_form():
    model = _ffi.DeviceModel.__new__(_ffi.DeviceModel)
    model.M, model.d, model.dtype = 4, 1, _ffi.F64

    class _Data:
        n, d, layout = 8, 1, _ffi.VEC

    with pytest.raises(ValueError):
        model.elbo_grad(_Data(), 0, 8, 0.0, shard=(1.0, 1.0), prior_mean=np.zeros(8))


def test_mean_grad_destination_is_checked():
    """A tensor given as the d elbo / d mux destination must be a contiguous device tensor of the data dtype with at least batch_len
    elements (the library writes batch_len of them); checked before anything reaches the library."""
    import torch
    with pytest.raises(ValueError):
        _ffi.point_mean_grad_ptr(torch.zeros(8, dtype=torch.float64), 8, _ffi.F64)   # host tensor
    with pytest.raises(ValueError):
        _ffi.point_mean_grad_ptr(1.5, 8, _ffi.F64)
    with pytest.raises(ValueError):
        _ffi.point_mean_grad_ptr(True, 8, _ffi.F64)
    assert _ffi.point_mean_grad_ptr(4096, 8, _ffi.F64) == 4096                       # a raw device pointer: the caller's to size
