"""GPU checks of the collapsed bound with per-point noise variances and any prior mean (svgp_collapsed_bound_with_noise / _q_ / _grad_)
against the float64 restatement tests/collapsed_noise_ref.py.

Shapes: M = 1, 127, 129, 300 (padding to Mp, more than two 128-panels); n = 1, 17, 1000 and 70 001 (two chunks of the data pass);
d = 1, 4, 17 (the wide-input twin); windows that start off a multiple of 16; the three kernel families, ARD, both parametrisations,
both dtypes.  Noise spans four orders of magnitude inside a batch, the prior mean offsets are of the size of y.
f64: the tolerances of tests/test_gpu_collapsed.py (bound 1e-8, gradient blocks 1e-6 of the block's largest entry), also for the new
per-point blocks.  fp32: measured against the fp64 restatement on fp32-rounded inputs, asserted at 4x the worst measured value."""
import ctypes as C
import functools

import numpy as np
import pytest

import collapsed_noise_ref as cn
import svgp_oracle as o
from approxgp import _ffi
from helpers import device_model

pytestmark = pytest.mark.gpu
JITTER = 1e-5
JITTER_F32 = 1e-3

# (n, M, d, family, ard, layout, centered, mean_const, batch_off)
CASES = {
    "n1_M1_d1": (1, 1, 1, o.KERNEL_SE, False, _ffi.VEC, False, 0.2, 0),
    "n17_M127_d4": (17, 127, 4, o.KERNEL_MATERN32, True, _ffi.ROWVECS, True, -0.4, 5),
    "n1000_M129_d17": (1000, 129, 17, o.KERNEL_SE, False, _ffi.COLVECS, False, 0.3, 37),
    "n1000_M300_d4": (1000, 300, 4, o.KERNEL_MATERN52, True, _ffi.COLVECS, True, 0.7, 0),
    "n70001_M128_d2": (70001, 128, 2, o.KERNEL_SE, True, _ffi.COLVECS, False, 0.0, 0),
}
F32_CASES = {
    "f32_n1000_M129_d17": (1000, 129, 17, o.KERNEL_MATERN32, False, _ffi.COLVECS, True, 0.3, 37),
    "f32_n1000_M300_d4": (1000, 300, 4, o.KERNEL_SE, True, _ffi.ROWVECS, False, 0.0, 0),
    "f32_n70001_M128_d2": (70001, 128, 2, o.KERNEL_SE, True, _ffi.COLVECS, False, 0.0, 0),
}
# fp32 against the fp64 restatement on fp32-rounded inputs: worst value over F32_CASES as measured on an MI355X, relative to the bound /
# to each gradient block's largest entry (profiles/collapsed/accuracy_noise.md); asserted at 4x
F32_MEASURED = {"bound": 9.5e-7, "variance": 2.0e-4, "lik_sigma2": 5.7e-5, "mean_const": 2.2e-2, "inv_lengthscale": 7.9e-5, "z": 3.0e-3,
                "noise": 2.0e-4, "mean_x": 2.5e-4, "m": 1.2e-2, "Lq": 1.5e-3}


@pytest.fixture(scope="module")
def ctx():
    c = _ffi.Context(0)
    yield c
    c.close()


def _is32(name):
    return name.startswith("f32")


def _jitter(name):
    return JITTER_F32 if _is32(name) else JITTER


@functools.lru_cache(maxsize=None)
def _problem(name):
    """(kernel, z, x, y, s2, s, mux, muz, spec, window slices, reference + gradient reference over the window) - computed once."""
    spec = {**CASES, **F32_CASES}[name]
    n, M, d, family, ard, layout, centered, mc, off = spec
    dtype = np.float32 if _is32(name) else np.float64
    kernel, z, x, y, s2, s, mux, muz = cn.problem(n + off + (11 if off else 0), M, d, family=family, ard=ard, dtype=dtype, mean_const=mc)
    w = slice(off, off + n)
    ref, g = cn.bound_grad(kernel, z, _jitter(name), x[:, w], s2, s[w], y[w], mean_const=mc, mux=mux[w], want_x=n <= 1000)
    for a in (z, x, y, s, mux, muz):
        a.setflags(write=False)
    return kernel, z, x, y, s2, s, mux, muz, spec, w, ref, g


def _device(ctx, name, with_muz=True):
    kernel, z, x, y, s2, s, mux, muz, spec, w, ref, g = _problem(name)
    n, M, d, family, ard, layout, centered, mc, off = spec
    dtype = np.float32 if _is32(name) else np.float64
    q = o.SVA(kernel, z, np.zeros(M), np.eye(M), jitter=_jitter(name), mean_const=mc, centered=centered)
    xd = x[0] if d == 1 else (x if layout == _ffi.COLVECS else np.ascontiguousarray(x.T))
    data = _ffi.DeviceData(ctx, xd, y, dtype, layout=layout if d > 1 else _ffi.VEC)
    model = device_model(ctx, q, dtype=dtype, sigma2=s2)
    if with_muz:
        model.set_mean_z(muz)
    return model, data


def _rel(a, b):
    return abs(a - b) / abs(b)


def _block_err(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-12)


def _errors(name, val, m, Lq, g):
    """relative error of the bound and of every block against the restatement (q in the case's parametrisation, muz included)."""
    kernel, z, x, y, s2, s, mux, muz, spec, w, ref, g_ref = _problem(name)
    d, centered, mc = spec[2], spec[6], spec[7]
    m_ref, Lq_ref = cn.optimal_q(ref, mean_const=mc, muz=muz, centered=centered)
    e = {"bound": _rel(val, ref.bound), "m": _block_err(m, m_ref), "Lq": _block_err(Lq, Lq_ref)}
    for k in ("variance", "lik_sigma2", "mean_const"):
        e[k] = _block_err([g[k]], [g_ref[k]])
    for k in ("inv_lengthscale", "noise", "mean_x"):
        e[k] = _block_err(g[k], g_ref[k])
    zr = g_ref["z"] if d > 1 else g_ref["z"][0]
    e["z"] = _block_err(g["z"].reshape(zr.shape, order="F") if d > 1 else g["z"], zr)
    if "x" in g and "x" in g_ref:
        gx = np.asarray(g["x"], dtype=np.float64)
        e["x"] = _block_err(gx if gx.shape == g_ref["x"].shape else gx.T.reshape(g_ref["x"].shape) if gx.ndim == 2 else gx[None, :], g_ref["x"])
    return e


@pytest.mark.parametrize("name", list(CASES))
def test_bound_q_and_every_gradient_block_match_the_restatement(ctx, name):
    kernel, z, x, y, s2, s, mux, muz, spec, w, ref, g_ref = _problem(name)
    n, off = spec[0], spec[8]
    model, data = _device(ctx, name)
    try:
        kw = dict(prior_mean=mux[w], noise=s[w], mean_z=True)
        val, t = model.collapsed_bound(data, off, n, **kw)
        assert _rel(val, ref.bound) < 1e-8
        assert t.bound == val and t.n_points == n and t.chol_info == 0 and t.chol_info_b == 0 and t.reserved == 0
        assert _rel(t.fit, ref.fit) < 1e-8 and abs(t.trace - ref.trace) < 1e-8 * abs(ref.bound)
        assert _rel(t.logdet_B, ref.logdet_B) < 1e-8 and abs(t.logdet_kuu - ref.logdet_kuu) < 1e-8 * abs(ref.logdet_kuu)
        vq, m, Lq = model.collapsed_q(data, off, n, **kw)
        assert vq == val and np.all(np.triu(Lq, 1) == 0) and np.all(np.diag(Lq) > 0)
        vg, tg, g = model.collapsed_grad(data, off, n, inputs=True if n <= 1000 else None, want_mean_grad=True, want_noise_grad=True, **kw)
        assert vg == val and tg.bound == val and tg.fit == t.fit and tg.trace == t.trace
        e = _errors(name, val, m, Lq, g)
        print(name, {k: f"{v:.2e}" for k, v in e.items()})
        assert e.pop("bound") < 1e-8
        assert e.pop("m") < 1e-8 and e.pop("Lq") < 1e-8
        for k, v in e.items():
            assert v <= 1e-6, (k, v)
        # repeated calls: bitwise
        v2, t2, g2 = model.collapsed_grad(data, off, n, want_mean_grad=True, want_noise_grad=True, **kw)
        assert v2 == val and t2.fit == t.fit and all(np.array_equal(g2[k], g[k]) for k in ("z", "inv_lengthscale", "noise", "mean_x"))
        assert g2["variance"] == g["variance"] and g2["lik_sigma2"] == g["lik_sigma2"] and g2["mean_const"] == g["mean_const"]
        _, m2, Lq2 = model.collapsed_q(data, off, n, **kw)
        assert np.array_equal(m2, m) and np.array_equal(Lq2, Lq)
    finally:
        model.free()
        data.free()


def test_fp32_accuracy(ctx):
    """fp32 models (data pass in fp32, M-sized tail in fp64) against the fp64 restatement on fp32-rounded inputs, jitter 1e-3.  Measured on
    an MI355X, relative to the bound / to each block's largest entry (bound, m, Lq, variance, lik_sigma2, mean_const, inv_lengthscale,
    s_bar, mux_bar, z):
        f32_n1000_M129_d17   2.4e-7  1.8e-5  2.0e-5  2.8e-6  5.9e-7  7.3e-5  6.9e-6  7.8e-6  7.9e-6  2.9e-5     (Centered, wide inputs)
        f32_n1000_M300_d4    5.1e-7  4.9e-4  2.3e-4  3.2e-5  8.6e-6  4.5e-4  2.6e-5  6.7e-5  7.0e-5  2.9e-3
        f32_n70001_M128_d2   9.4e-7  1.2e-2  1.5e-3  2.0e-4  5.6e-5  2.1e-2  7.8e-5  2.0e-4  2.4e-4  5.9e-5     (two chunks)
    With weights up to 1 / sigma^2 = 100 over 70 001 points the whitened mean and the mean_const gradient (sum_j mux_bar_j, which all but
    cancels at the optimal q) lose the most.  F32_MEASURED holds the worst of each column (profiles/collapsed/accuracy_noise.md);
    asserted at 4x.  The bound must also stay inside the project's fp32 contract of 1e-4."""
    worst = {k: 0.0 for k in F32_MEASURED}
    for name in F32_CASES:
        kernel, z, x, y, s2, s, mux, muz, spec, w, ref, g_ref = _problem(name)
        n, off = spec[0], spec[8]
        model, data = _device(ctx, name)
        try:
            kw = dict(prior_mean=mux[w], noise=s[w], mean_z=True)
            _, m, Lq = model.collapsed_q(data, off, n, **kw)
            val, _, g = model.collapsed_grad(data, off, n, want_mean_grad=True, want_noise_grad=True, **kw)
        finally:
            model.free()
            data.free()
        e = _errors(name, val, m, Lq, g)
        print(name, {k: f"{v:.2e}" for k, v in e.items()})
        for k, v in e.items():
            worst[k] = max(worst[k], v)
    print("fp32 worst", {k: f"{v:.2e}" for k, v in worst.items()})
    assert worst["bound"] < 1e-4
    for k, v in worst.items():
        assert F32_MEASURED[k] is not None, "fp32 figures have not been recorded"
        assert v <= 4 * F32_MEASURED[k], (k, v, F32_MEASURED[k])


def _raw(ctx, model, data, off, n, pm, pn, which, M=None, want=()):
    """the three C calls with explicit (possibly NULL) structs -> (rc, bound, terms, extras)."""
    lib, out, t = ctx.lib, C.c_double(), _ffi.CollapsedTerms()
    ref = lambda p: C.byref(p) if p is not None else None
    if which == "bound":
        return lib.svgp_collapsed_bound_with_noise(ctx.h, model.h, data.h, off, n, ref(pm), ref(pn), C.byref(out), C.byref(t)), out.value, t, None
    dt = _ffi.np_dtype(model.dtype)
    if which == "q":
        m, Lq = np.zeros(model.M, dtype=dt), np.zeros((model.M, model.M), dtype=dt, order="F")
        rc = lib.svgp_collapsed_q_with_noise(ctx.h, model.h, data.h, off, n, ref(pm), ref(pn), _ffi._ptr(m), _ffi._ptr(Lq), C.byref(out))
        return rc, out.value, None, (m, Lq)
    il, zb = np.zeros(model.d), np.zeros((model.d, model.M), dtype=dt, order="F")
    g = _ffi.Grads(0.0, 0.0, 0.0, il.ctypes.data_as(C.POINTER(C.c_double)), _ffi._ptr(zb), None, None)
    rc = lib.svgp_collapsed_grad_with_noise(ctx.h, model.h, data.h, off, n, ref(pm), ref(pn), C.byref(out), C.byref(t), C.byref(g), None, None, None)
    return rc, out.value, t, (g.variance, g.lik_sigma2, g.mean_const, il, zb)


@pytest.mark.parametrize("name", ["n1000_M129_d17", "f32_n1000_M300_d4"])
def test_null_arguments_are_the_plain_calls_bitwise(ctx, name):
    spec = _problem(name)[8]
    n, off = spec[0], spec[8]
    model, data = _device(ctx, name, with_muz=False)
    try:
        b0, t0 = model.collapsed_bound(data, off, n)
        rc, b1, t1, _ = _raw(ctx, model, data, off, n, None, None, "bound")
        assert rc == 0 and b1 == b0 and (t1.fit, t1.trace, t1.logdet_B, t1.logdet_kuu) == (t0.fit, t0.trace, t0.logdet_B, t0.logdet_kuu)
        bq0, m0, Lq0 = model.collapsed_q(data, off, n)
        rc, bq1, _, (m1, Lq1) = _raw(ctx, model, data, off, n, None, None, "q")
        assert rc == 0 and bq1 == bq0 and np.array_equal(m1, m0) and np.array_equal(Lq1, Lq0)
        bg0, _, g0 = model.collapsed_grad(data, off, n)
        rc, bg1, _, (var, ls2, mcb, il, zb) = _raw(ctx, model, data, off, n, None, None, "grad")
        assert rc == 0 and bg1 == bg0 and var == g0["variance"] and ls2 == g0["lik_sigma2"] and mcb == g0["mean_const"]
        assert np.array_equal(il, g0["inv_lengthscale"]) and np.array_equal(zb.ravel(order="F"), np.asarray(g0["z"]).ravel(order="F"))
    finally:
        model.free()
        data.free()


@pytest.mark.parametrize("name", ["n1000_M129_d17", "f32_n1000_M129_d17"])
def test_windows_sentinels_and_host_against_device_memory(ctx, name):
    """Element j of s / mux / s_bar / mux_bar belongs to point batch_off + j (the window starts at 37), nothing past batch_len is read or
    written, and host and device memory give the same bits for every input and output."""
    import torch
    kernel, z, x, y, s2, s, mux, muz, spec, w, ref, g_ref = _problem(name)
    n, d, off = spec[0], spec[2], spec[8]
    dt = np.float32 if _is32(name) else np.float64
    tdt = torch.float32 if _is32(name) else torch.float64
    model, data = _device(ctx, name)
    try:
        kw = dict(mean_z=True, want_mean_grad=True, want_noise_grad=True)
        vh, _, gh = model.collapsed_grad(data, off, n, prior_mean=mux[w], noise=s[w], inputs=True, **kw)
        # a shifted window reads other elements: the restatement's s_bar of THIS window matched above (test_bound_q_...), and a window
        # moved by one point with the vectors moved along gives the matching entries of ITS gradient, not these
        w1 = slice(off + 1, off + 1 + n)
        _, _, g1 = model.collapsed_grad(data, off + 1, n, prior_mean=mux[w1], noise=s[w1], **kw)
        assert not np.array_equal(g1["noise"][:-1], gh["noise"][1:]) and _block_err(g1["noise"][:5], gh["noise"][1:6]) < 0.5
        # host inputs with NaN past batch_len: only batch_len elements are read
        pad = lambda v: np.concatenate([np.asarray(v, dtype=dt), np.full(9, np.nan, dtype=dt)])
        sp, mp = pad(s[w]), pad(mux[w])
        pn, pm = _ffi.PointNoise(_ffi._ptr(sp), 0, 0), _ffi.PointMean(_ffi._ptr(mp), 0, 0)
        rc, vb, _, _ = _raw(ctx, model, data, off, n, pm, pn, "bound")
        assert rc == 0 and vb == vh
        # device inputs (NaN past batch_len as well) and device outputs with sentinels past batch_len
        st, mt = torch.tensor(sp, device="cuda"), torch.tensor(mp, device="cuda")
        sb = torch.full((n + 16,), -7.25, dtype=tdt, device="cuda")
        mb = torch.full((n + 16,), -3.5, dtype=tdt, device="cuda")
        xg = torch.full((d, n + 16), 9.75, dtype=tdt, device="cuda")
        torch.cuda.synchronize()
        vd, _, gd = model.collapsed_grad(data, off, n, prior_mean=mt[:n], noise=st[:n], mean_z=True, want_mean_grad=mb, want_noise_grad=sb,
                                         inputs=(xg.data_ptr(), n + 16))
        torch.cuda.synchronize()
        assert vd == vh and "noise" not in gd and "mean_x" not in gd
        assert np.array_equal(sb[:n].cpu().numpy(), gh["noise"]) and np.array_equal(mb[:n].cpu().numpy(), gh["mean_x"])
        assert torch.all(sb[n:] == -7.25) and torch.all(mb[n:] == -3.5) and torch.all(xg[:, n:] == 9.75)
        assert np.array_equal(xg[:, :n].cpu().numpy(), np.asarray(gh["x"]).reshape(d, n))
        for k in ("z", "inv_lengthscale", "variance", "lik_sigma2", "mean_const"):
            assert np.array_equal(gd[k], gh[k]), k
        bq_h, m_h, Lq_h = model.collapsed_q(data, off, n, prior_mean=mux[w], noise=s[w], mean_z=True)
        bq_d, m_d, Lq_d = model.collapsed_q(data, off, n, prior_mean=mt[:n], noise=st[:n], mean_z=True)
        assert bq_d == bq_h == vh and np.array_equal(m_d, m_h) and np.array_equal(Lq_d, Lq_h)
        # bad structs are refused before anything is enqueued
        for bad in (_ffi.PointNoise(None, 0, 0), _ffi.PointNoise(_ffi._ptr(sp), 2, 0), _ffi.PointNoise(_ffi._ptr(sp), 0, 1)):
            for which in ("bound", "q", "grad"):
                assert _raw(ctx, model, data, off, n, None, bad, which)[0] == _ffi.INVALID_ARG
        assert _raw(ctx, model, data, off, n, _ffi.PointMean(None, 0, 0), pn, "bound")[0] == _ffi.INVALID_ARG
        # the plain calls keep their SVGP_UNSUPPORTED for a model carrying muz
        with pytest.raises(_ffi.UnsupportedError):
            model.collapsed_bound(data, off, n)
    finally:
        model.free()
        data.free()


@pytest.mark.parametrize("name", ["n1000_M300_d4", "n1000_M129_d17"])
def test_bound_is_the_elbo_at_the_written_q(ctx, name):
    """Without trusting the new code: svgp_marginals_with_mean at the q that svgp_collapsed_q_with_noise wrote, the Gaussian expectation
    with sigma_j^2 on the host, minus svgp_prior_kl.  Centered with muz (M300) and NonCentered with muz (M129)."""
    kernel, z, x, y, s2, s, mux, muz, spec, w, ref, g_ref = _problem(name)
    n, off = spec[0], spec[8]
    model, data = _device(ctx, name)
    try:
        bound, _, _ = model.collapsed_q(data, off, n, fetch=False, prior_mean=mux[w], noise=s[w], mean_z=True)
        mu, v = model.marginals(data, off, n, prior_mean=mux[w])
        sig = s2 + s[w]
        e = float(np.sum(-0.5 * np.log(2 * np.pi * sig) - ((y[w] - mu) ** 2 + v) / (2 * sig)))
        kl = model.prior_kl()[0]
        print(f"{name}: elbo at q {e - kl:.12g} bound {bound:.12g}")
        assert _rel(e - kl, bound) < 1e-9
    finally:
        model.free()
        data.free()


def test_downweighted_points_leave_only_their_normalisation(ctx):
    """Points given s_j = 1e12 contribute -1/2 log(2 pi sigma_j^2) and nothing else: the bound minus those terms is the bound of the
    remaining points (a wrong weight on the SYRK's padding would show here)."""
    name = "n1000_M129_d17"
    kernel, z, x, y, s2, s, mux, muz, spec, w, ref, g_ref = _problem(name)
    n, M, d, off = spec[0], spec[1], spec[2], spec[8]
    xw, yw, sw, mw = x[:, w], y[w], s[w].copy(), mux[w]
    down = np.arange(n) % 3 == 1
    down[-130:] = True                      # (the last chunk's tail and its padding weights)
    sw[down] = 1e12
    q = o.SVA(kernel, z, np.zeros(M), np.eye(M), jitter=JITTER, mean_const=spec[7], centered=False)
    model = device_model(ctx, q, dtype=np.float64, sigma2=s2)
    full = _ffi.DeviceData(ctx, xw, yw, np.float64)
    rest = _ffi.DeviceData(ctx, np.ascontiguousarray(xw[:, ~down]), yw[~down], np.float64)
    try:
        b_all, _ = model.collapsed_bound(full, 0, n, prior_mean=mw, noise=sw)
        b_rest, _ = model.collapsed_bound(rest, 0, int((~down).sum()), prior_mean=mw[~down], noise=sw[~down])
        norm = float(np.sum(-0.5 * np.log(2 * np.pi * (s2 + sw[down]))))
        print(f"down-weighted: {b_all - norm:.12g} remaining {b_rest:.12g}")
        assert _rel(b_all - norm, b_rest) < 1e-8
    finally:
        model.free()
        full.free()
        rest.free()


def test_failure_rules(ctx):
    name = "n1000_M129_d17"
    kernel, z, x, y, s2, s, mux, muz, spec, w, ref, g_ref = _problem(name)
    n, off = spec[0], spec[8]
    model, data = _device(ctx, name)
    try:
        kw = dict(prior_mean=mux[w], mean_z=True)
        good, m_good, Lq_good = model.collapsed_q(data, off, n, noise=s[w], **kw)
        before = model.posterior()
        for badval in (-s2, -2.0 * s2):                       # sigma_j^2 = 0 and < 0
            sb = s[w].copy()
            sb[n // 2] = badval
            with pytest.raises(_ffi.PosDefException):
                model.collapsed_bound(data, off, n, noise=sb, **kw)
            pn, keep = _ffi.point_noise(sb, n, model.dtype)
            assert _raw(ctx, model, data, off, n, None, pn, "q")[0] == _ffi.NOT_POSDEF
            assert _raw(ctx, model, data, off, n, None, pn, "grad")[0] == _ffi.NOT_POSDEF
            after = model.posterior()
            assert all(np.array_equal(a, b) for a, b in zip(before, after))           # q untouched
        sn = s[w].copy()
        sn[3] = np.nan
        val, t = model.collapsed_bound(data, off, n, noise=sn, **kw)
        assert np.isnan(val) and np.isnan(t.bound)                                    # NaN with SVGP_OK
        mn = mux[w].copy()
        mn[n - 1] = np.nan
        assert np.isnan(model.collapsed_bound(data, off, n, prior_mean=mn, noise=s[w], mean_z=True)[0])
        # a healthy call afterwards is what a fresh context gives, bitwise
        again, m_a, Lq_a = model.collapsed_q(data, off, n, noise=s[w], **kw)
        assert again == good and np.array_equal(m_a, m_good) and np.array_equal(Lq_a, Lq_good)
        c2 = _ffi.Context(0)
        try:
            model2, data2 = _device(c2, name)
            try:
                fresh, m_f, Lq_f = model2.collapsed_q(data2, off, n, noise=s[w], **kw)
            finally:
                model2.free()
                data2.free()
        finally:
            c2.close()
        assert fresh == good and np.array_equal(m_f, m_good) and np.array_equal(Lq_f, Lq_good)
    finally:
        model.free()
        data.free()


def test_call_order_on_one_context_matches_fresh_contexts(ctx):
    """collapsed_q_with_noise, svgp_elbo_grad, svgp_collapsed_bound, collapsed_grad_with_noise on two models of different M sharing one
    context (the workspace cached by Mp, the staging buffers): each result is bitwise what a fresh context gives."""
    names = ("n1000_M300_d4", "n17_M127_d4")

    def steps(c, only=None):
        out = []
        devs = {nm: _device(c, nm, with_muz=False) for nm in names}
        try:
            plan = [(0, "q"), (1, "elbo_grad"), (0, "bound"), (1, "grad"), (1, "q"), (0, "grad")]
            for i, (which, what) in enumerate(plan):
                if only is not None and i != only:
                    out.append(None)
                    continue
                nm = names[which]
                kernel, z, x, y, s2, s, mux, muz, spec, w, ref, g_ref = _problem(nm)
                n, off = spec[0], spec[8]
                model, data = devs[nm]
                if what == "q":
                    b, m, Lq = model.collapsed_q(data, off, n, prior_mean=mux[w], noise=s[w])
                    out.append((b, m.tobytes(), Lq.tobytes()))
                elif what == "elbo_grad":
                    v, _, g = model.elbo_grad(data, off, n, float(n))
                    out.append((v, g["variance"], g["z"].tobytes(), g["Lq"].tobytes()))
                elif what == "bound":
                    out.append((model.collapsed_bound(data, off, n)[0],))
                else:
                    b, _, g = model.collapsed_grad(data, off, n, prior_mean=mux[w], noise=s[w], want_mean_grad=True, want_noise_grad=True)
                    out.append((b, g["variance"], g["lik_sigma2"], g["z"].tobytes(), g["noise"].tobytes(), g["mean_x"].tobytes()))
        finally:
            for model, data in devs.values():
                model.free()
                data.free()
        return out

    shared = steps(ctx)
    for i in range(len(shared)):
        c2 = _ffi.Context(0)
        try:
            alone = steps(c2, only=i)[i]
        finally:
            c2.close()
        assert alone == shared[i], i


def test_python_mirror_accepts_vector_noise_and_a_custom_mean(ctx):
    """elbo / elbo_and_gradient / optimal_variational_posterior with f(x, Diagonal(v)) and GP(CustomMean(g), k): min(v) goes to lik_sigma2,
    the rest to s; mean_offsets(x) -> pm, mean_offsets(z) -> muz."""
    import approxgp as ag
    name = "n1000_M129_d17"
    kernel, z, x, y, s2, s, mux, muz, spec, w, ref, g_ref = _problem(name)
    n, M, d, mc = spec[0], spec[1], spec[2], spec[7]
    xw, yw = np.ascontiguousarray(x[:, w]), y[w]
    lut = {xw[:, j].tobytes(): mux[w][j] for j in range(n)}
    lut.update({z[:, i].tobytes(): muz[i] for i in range(M)})
    fn = lambda a: np.array([lut[np.ascontiguousarray(np.asarray(a, dtype=np.float64)[:, j]).tobytes()] + mc for j in range(np.asarray(a).shape[1])])
    from approxgp import kernels as K
    k = kernel.variance * K.TransformedKernel(K.SqExponentialKernel(), K.ARDTransform(kernel.inv_lengthscale))
    f = ag.GP(ag.CustomMean(fn), k)
    sy = ag.Diagonal(s2 + s[w])
    vfe = ag.VFE(f(z, JITTER))
    val = ag.elbo(vfe, f(xw, sy), yw, ctx=ctx)
    assert _rel(val, ref.bound) < 1e-8
    val2, g = ag.elbo_and_gradient(vfe, f(xw, sy), yw, ctx=ctx, wrt_noise=True, wrt_mean=True)
    assert val2 == val and _block_err(g["Sigma_y"], g_ref["noise"]) < 1e-6 and _block_err(g["mean_x"], g_ref["mean_x"]) < 1e-6
    assert _rel(g["lik_sigma2"], g_ref["lik_sigma2"]) < 1e-6
    sva = ag.optimal_variational_posterior(f(z, JITTER), f(xw, sy), yw, ag.Centered, ctx=ctx)
    m_ref, Lq_ref = cn.optimal_q(ref, mean_const=mc, muz=muz, centered=True)
    assert _block_err(sva.q.m, m_ref) < 1e-8
