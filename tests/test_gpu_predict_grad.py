"""GPU checks of the predictive mean and variance with their input gradients (svgp_predictor_*; csrc/predict_grad.hip,
predict_grad_api.hip) through the C ABI, against a float64 closed form in numpy on the SAME numbers (pathwise_ref.recipe).

The reference uses the two-solve form a = Lk^-1 k (never the explicit G) from the oracle's Kuu and its Cholesky factor:
    mu = mean + a' w,   v = k(x, x) - a'a + |B'a|^2 + 1e-18,   w = m, B = Lq (NonCentered);  w = Lk^-1 (m - mean(z)), B = Lk^-1 Lq (Centered)
and differentiates analytically, d k_i / d x_c = invl_c 2 g(r_i^2) (xs_c - zs_ic), with the kappa and g of the oracle.

Shapes: M = 1, 37, 128, 130, 257, 300 (one row block, padding, the row-block boundary, three row blocks); d = 1, 3, 8, 9, 17, 33, 64
(every DREG bucket, the fp32 by-differences boundary, the second and the 4-wide coordinate blocks); n* = 1, 17, 65, 129, 1000 (ragged
groups and workgroups).  Every case in both dtypes, the families rotating; Centered and NonCentered, with and without muz + pm,
ColVecs and RowVecs, host and device output.

Tolerances, per output and relative to that output's largest entry: fp64 1e-8; fp32 max(1e-4, 8 e32), e32 the error of the same
reference with its data stage in float32 (the convention and the factor of test_gpu_pathwise_grad.py).  The observed multiples are
printed by the last test (profiles/predict_grad/accuracy.md)."""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.linalg as sla

import pathwise_ref as pw
import svgp_oracle as o
from approxgp import _ffi
from pathwise_grad_ref import dkappa_dr2

pytestmark = pytest.mark.gpu
JITTER = 1e-3
TOL64 = 1e-8
F32_FACTOR = 8.0
FAMILIES = (o.KERNEL_SE, o.KERNEL_MATERN32, o.KERNEL_MATERN52)
COL, ROW = _ffi.COLVECS, _ffi.ROWVECS

# (M, d, n*, centered, layout, mean_const, muz + pm, device output)
SHAPES = [
    (1, 1, 17, False, COL, 0.0, False, False),
    (37, 3, 129, True, COL, 0.7, True, False),
    (128, 8, 65, False, ROW, 0.0, False, True),
    (130, 9, 1000, True, COL, -0.4, True, True),
    (257, 17, 65, False, ROW, 0.3, False, False),
    (300, 33, 17, True, COL, 0.2, False, True),
    (37, 64, 1, False, COL, 0.0, False, False),
]
CASES = {}
for _i, _s in enumerate(SHAPES):
    _tag = "M%d_d%d_n%d" % _s[:3]
    CASES[_tag] = _s + (FAMILIES[_i % 3],)
    CASES["f32_" + _tag] = _s + (FAMILIES[(_i + 1) % 3],)
assert {(n.startswith("f32"), c[-1]) for n, c in CASES.items()} == {(f, k) for f in (False, True) for k in FAMILIES}
OBSERVED = {}


def reference(sva, muz, x, mux=None, f32=False):
    """(mean (n,), var (n,), dmean (d, n), dvar (d, n)): the M-sized stage in float64, the data-sized stage in float32 with f32 (every
    array of it rounded once, every operation in float32)."""
    dt = np.float32 if f32 else np.float64
    Lk = np.linalg.cholesky(o.kuu(o.SVA(sva.kernel, sva.z.astype(np.float64), sva.m, sva.Lq, jitter=sva.jitter)))
    mean_z = sva.mean_const + (0.0 if muz is None else np.asarray(muz, dtype=np.float64))
    m, Lq = sva.m.astype(np.float64), np.tril(sva.Lq.astype(np.float64))
    w, B = (sla.solve_triangular(Lk, m - mean_z, lower=True), sla.solve_triangular(Lk, Lq, lower=True)) if sva.centered else (m, Lq)
    x, z = o._as_dn(np.asarray(x)).astype(dt), sva.z.astype(dt)
    Lk, w, B, il = Lk.astype(dt), w.astype(dt), B.astype(dt), sva.kernel.inv_lengthscale.astype(dt)
    diff = (x[:, :, None] - z[:, None, :]) * il[:, None, None]           # (d, n, M)
    r2 = np.zeros(diff.shape[1:], dtype=dt)
    for c in range(diff.shape[0]):
        r2 += diff[c] * diff[c]
    A = sla.solve_triangular(Lk, o._kappa(sva.kernel, r2).T.astype(dt), lower=True)   # (M, n)
    Cm = B.T @ A
    mean = dt(sva.mean_const) + (0 if mux is None else np.asarray(mux, dtype=dt)) + A.T @ w
    var = dt(sva.kernel.variance) - np.sum(A * A, axis=0) + np.sum(Cm * Cm, axis=0) + dt(1e-18)
    g2 = dt(2) * dkappa_dr2(sva.kernel, r2)
    dmean, dvar = np.zeros(x.shape, dtype=dt), np.zeros(x.shape, dtype=dt)
    for c in range(x.shape[0]):
        dA = sla.solve_triangular(Lk, (g2 * diff[c]).T * il[c], lower=True)
        dmean[c] = dA.T @ w
        dvar[c] = dt(2) * (np.sum(Cm * (B.T @ dA), axis=0) - np.sum(A * dA, axis=0))
    return mean.astype(dt), var, dmean, dvar


def dense_state(sva, muz):
    """(beta, G) in float64 by dense solves."""
    Kuu = o.kuu(sva)
    Lk = np.linalg.cholesky(Kuu)
    mean_z = sva.mean_const + (0.0 if muz is None else muz)
    Lq = np.tril(sva.Lq)
    if sva.centered:
        return sla.cho_solve((Lk, True), sva.m - mean_z), sla.cho_solve((Lk, True), sla.cho_solve((Lk, True), Lq @ Lq.T - Kuu).T)
    Li = sla.solve_triangular(Lk, np.eye(sva.M), lower=True)
    return Li.T @ sva.m, Li.T @ (Lq @ Lq.T - np.eye(sva.M)) @ Li


def _dtype(name):
    return np.float32 if name.startswith("f32") else np.float64


@pytest.fixture(scope="module")
def ctx():
    c = _ffi.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def _problem(name):
    """Everything of a case, computed once and shared read-only."""
    M, d, n, centered, layout, mc, with_mean, dev, family = CASES[name]
    dt = _dtype(name)
    rd = lambda a: np.asarray(a, dtype=dt).astype(np.float64)
    seed = 5000 + 7 * M + 13 * d + n
    sva, muz = pw.recipe(M, d, family, seed, centered=centered, mean_const=mc, with_muz=with_mean, jitter=JITTER, dtype=dt)
    x = rd(np.random.default_rng(seed + 1).uniform(-3.0, 3.0, size=(d, n)))
    mux = rd(0.3 * np.cos(x[0])) if with_mean else None
    ref = reference(sva, muz, x, mux)
    e32 = None
    if dt == np.float32:
        e32 = _errors(reference(sva, muz, x, mux, f32=True), ref)
    for a in (x,) + ref + ((muz, mux) if with_mean else ()):
        a.setflags(write=False)
    return dict(sva=sva, muz=muz, x=x, mux=mux, ref=ref, e32=e32)


def _errors(got, ref):
    return np.array([np.abs(np.asarray(g, dtype=np.float64) - r).max() / max(np.abs(r).max(), 1e-300) for g, r in zip(got, ref)])


def _tolerances(e32):
    return np.full(4, TOL64) if e32 is None else np.maximum(1e-4, F32_FACTOR * e32)


def _model(ctx, name, sva=None):
    M, d, layout = CASES[name][0], CASES[name][1], CASES[name][4]
    p = _problem(name)
    sva = p["sva"] if sva is None else sva
    z = sva.z[0] if d == 1 else (sva.z if layout == COL else np.ascontiguousarray(sva.z.T))
    desc, keep = _ffi.make_desc(_dtype(name), sva.kernel.family, sva.kernel.variance, sva.kernel.inv_lengthscale, z, sva.m, sva.Lq,
                                sva.jitter, parametrization=_ffi.CENTERED if sva.centered else _ffi.NONCENTERED, lik_sigma2=0.1,
                                mean_const=sva.mean_const, layout_z=layout)
    model = _ffi.DeviceModel(ctx, desc, keep)
    if p["muz"] is not None:
        model.set_mean_z(p["muz"])
    return model


def _data(ctx, name, x=None, y=None):
    d, layout = CASES[name][1], CASES[name][4]
    x = _problem(name)["x"] if x is None else x
    return _ffi.DeviceData(ctx, x[0] if d == 1 else (x if layout == COL else np.ascontiguousarray(x.T)), y, _dtype(name), layout=layout)


def _eval(pred, data, off=0, length=None, prior_mean=None, device=False):
    """The four outputs on the host, through host or device memory."""
    if not device:
        return pred.eval(data, off, length, prior_mean=prior_mean)
    import torch

    length = data.n - off if length is None else length
    tdt = torch.float32 if pred.dtype == _ffi.F32 else torch.float64
    bufs = [torch.full(s, -777.0, dtype=tdt, device="cuda") for s in ((length,), (length,), (pred.d, length), (pred.d, length))]
    torch.cuda.synchronize()
    pred.eval(data, off, length, prior_mean=prior_mean, out=bufs)
    return tuple(b.cpu().numpy() for b in bufs)


class _Session:
    """A case's model, data and predictor on the device."""

    def __init__(self, ctx, name, x=None, y=None, sva=None):
        self.model, self.data, self.pred = _model(ctx, name, sva), _data(ctx, name, x=x, y=y), None
        try:
            self.pred = self.model.predictor()
        except Exception:
            self.close()
            raise

    def close(self):
        for h in (self.pred, self.model, self.data):
            if h is not None:
                h.free()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


@pytest.mark.parametrize("name", list(CASES))
def test_device_matches_closed_form(ctx, name):
    M, d, n = CASES[name][:3]
    p = _problem(name)
    with _Session(ctx, name) as s:
        out = _eval(s.pred, s.data, prior_mean=p["mux"], device=CASES[name][7])
        mu, var = s.model.marginals(s.data, prior_mean=p["mux"])
    assert [a.shape for a in out] == [(n,), (n,), (d, n), (d, n)] and all(a.dtype == _dtype(name) for a in out)
    assert all(np.all(np.isfinite(a)) for a in out)
    err, tol = _errors(out, p["ref"]), _tolerances(p["e32"])
    OBSERVED[name] = (err, tol, p["e32"])
    print(f"{name}: errors {err} tolerances {tol} e32 {p['e32']}")
    assert np.all(err <= tol), (err, tol)
    # the same tolerance against svgp_marginals on the same window
    em = _errors(out[:2], (mu, var))
    print(f"{name}: against svgp_marginals {em}")
    assert np.all(em <= tol[:2]), (em, tol[:2])


@pytest.mark.parametrize("name", ["M37_d3_n129", "f32_M130_d9_n1000", "M128_d8_n65", "f32_M257_d17_n65"])
def test_q_equal_to_the_prior(ctx, name):
    """G = 0 and beta = 0: var = variance + 1e-18 to rounding, no gradient."""
    p = _problem(name)
    sva, eps = p["sva"], np.finfo(_dtype(name)).eps
    M = sva.M
    mean_z = sva.mean_const + (0.0 if p["muz"] is None else p["muz"])
    m, Lq = (mean_z + np.zeros(M), np.linalg.cholesky(o.kuu(sva))) if sva.centered else (np.zeros(M), np.eye(M))
    prior = o.SVA(sva.kernel, sva.z, m, Lq, jitter=sva.jitter, mean_const=sva.mean_const, centered=sva.centered)
    with _Session(ctx, name, sva=prior) as s:
        mean, var, dmean, dvar = s.pred.eval(s.data)
        beta, G = s.pred.state()
    # NonCentered: P = Lk^-1 exactly, so G = P'P - W and beta vanish exactly.  Centered: Lq = Lk and m = mean(z) are rounded to the model
    # dtype on their way in: E = Lq Lq' - Kuu has |E_ij| <= 2 eps |Lk_i.| |Lk_j.| <= 2 eps (variance + jitter), so
    # max|G| <= |Kuu^-1|_inf^2 max|E|, and max|beta| <= |Kuu^-1|_inf eps max|mean(z)|; a factor 2 for the M-sized stage's own rounding.
    # Downstream |k_i| <= variance and |D_ic| <= variance (r kappa'-type maxima: 0.61, 0.64, 0.63 variance), M terms a sum.
    v, il = sva.kernel.variance, np.abs(sva.kernel.inv_lengthscale).max()
    ninf = np.abs(np.linalg.inv(o.kuu(sva))).sum(axis=1).max()
    gb = 4 * eps * (v + JITTER) * ninf ** 2 if sva.centered else 0.0
    bb = 2 * eps * np.abs(mean_z).max() * ninf if sva.centered else 0.0
    print(f"{name}: max|G| {np.abs(G).max():.2e} (bound {gb:.2e}) max|beta| {np.abs(beta).max():.2e} (bound {bb:.2e}) "
          f"max|var - variance| {np.abs(var - v).max():.2e} max|dvar| {np.abs(dvar).max():.2e} max|dmean| {np.abs(dmean).max():.2e}")
    assert np.abs(G).max() <= gb and np.abs(beta).max() <= bb
    assert np.abs(var - v).max() <= 2 * gb * (M * v) ** 2 + 4 * eps * v
    assert np.abs(dvar).max() <= 4 * il * gb * (M * v) ** 2
    assert np.abs(dmean).max() <= 2 * il * M * v * bb
    assert np.abs(mean - sva.mean_const).max() <= 2 * M * v * bb + 4 * eps * abs(sva.mean_const)


@pytest.mark.parametrize("name", [n for n in CASES if CASES[n][-1] != o.KERNEL_SE and CASES[n][0] in (37, 128, 130)])
def test_at_the_inducing_points(ctx, name):
    """x equal to inducing points: r = 0 in one term of every point.  Finite, and inside the case's band."""
    p = _problem(name)
    x = np.array(p["sva"].z)
    ref = reference(p["sva"], p["muz"], x)
    tol = _tolerances(None if p["e32"] is None else _errors(reference(p["sva"], p["muz"], x, f32=True), ref))
    with _Session(ctx, name, x=x) as s:
        out = s.pred.eval(s.data)
    assert all(np.all(np.isfinite(a)) for a in out)
    err = _errors(out, ref)
    print(f"{name} at x = z: errors {err} tolerances {tol}")
    assert np.all(err <= tol), (err, tol)


@pytest.mark.parametrize("name", ["M130_d9_n1000", "f32_M130_d9_n1000", "f32_M128_d8_n65", "M257_d17_n65", "f32_M300_d33_n17", "M37_d64_n1"])
def test_contracts_are_bitwise(ctx, name):
    """A point's four outputs do not depend on the window, the call or the kind of output memory; svgp_elbo is unchanged."""
    n = CASES[name][2]
    p = _problem(name)
    mux = p["mux"]
    cut = lambda off, ln: None if mux is None else mux[off:off + ln]
    model, data = _model(ctx, name), _data(ctx, name, y=np.sin(p["x"][0]))
    try:
        e0 = model.elbo(data)[0]
        pred = model.predictor()
        full = pred.eval(data, prior_mean=mux)
        for other in (pred.eval(data, prior_mean=mux), _eval(pred, data, prior_mean=mux, device=True)):
            assert all(np.array_equal(a, b) for a, b in zip(full, other))
        for off in (0, 1, 63):
            if off >= n:
                continue
            for ln in sorted({1, min(17, n - off), n - off}):
                for device in (False, True):
                    win = _eval(pred, data, off, ln, prior_mean=cut(off, ln), device=device)
                    assert all(np.array_equal(a[..., off:off + ln], b) for a, b in zip(full, win)), (off, ln, device)
        values = pred.eval(data, prior_mean=mux, want_grad=False)
        assert np.array_equal(values[0], full[0]) and np.array_equal(values[1], full[1]) and values[2] is None
        pred.free()
        assert model.elbo(data)[0] == e0
        pred = model.predictor()
        model.free()   # the predictor is a snapshot
        assert all(np.array_equal(a, b) for a, b in zip(full, pred.eval(data, prior_mean=mux)))
        pred.free()
    finally:
        model.free()
        data.free()


@pytest.mark.parametrize("name", ["M37_d3_n129", "M130_d9_n1000", "f32_M257_d17_n65", "M300_d33_n17", "f32_M1_d1_n17"])
def test_state_matches_dense_solves(ctx, name):
    p = _problem(name)
    beta_ref, G_ref = dense_state(p["sva"], p["muz"])
    with _Session(ctx, name) as s:
        beta, G = s.pred.state()
        alpha = s.model.posterior()[1]
    assert np.array_equal(G, G.T)
    err = np.abs(G - G_ref).max() / np.abs(G_ref).max()
    print(f"{name}: G error {err:.2e} of max|G| {np.abs(G_ref).max():.2e}")
    assert err <= 1e-10
    np.testing.assert_allclose(beta, beta_ref, rtol=1e-6, atol=1e-7)   # svgp_posterior's tolerance for alpha
    if _dtype(name) == np.float64:
        np.testing.assert_allclose(beta, alpha, rtol=1e-6, atol=1e-7)


def test_statuses_then_a_healthy_call(ctx):
    name = "M37_d3_n129"
    p = _problem(name)
    lib, ptr = ctx.lib, _ffi._ptr
    other_d = _ffi.DeviceData(ctx, np.zeros((2, 5)), None, np.float64)
    other_t = _ffi.DeviceData(ctx, np.zeros((3, 5)), None, np.float32)
    try:
        with _Session(ctx, name) as s:
            out0 = s.pred.eval(s.data, prior_mean=p["mux"])
            mean, var, dm, dv = np.zeros(129), np.zeros(129), np.zeros((3, 129)), np.zeros((3, 129))
            call = lambda d_, off, n, ldg, pm=None, dev=0, outs=(mean, var, dm, dv): lib.svgp_predictor_eval(
                ctx.h, s.pred.h, d_.h, off, n, pm, *(ptr(a) for a in outs), ldg, dev)
            assert call(other_d, 0, 5, 5) == _ffi.INVALID_ARG            # d mismatch
            assert call(other_t, 0, 5, 5) == _ffi.INVALID_ARG            # dtype mismatch
            assert call(s.data, 0, 0, 129) == _ffi.INVALID_ARG           # empty window
            assert call(s.data, 100, 30, 129) == _ffi.INVALID_ARG        # window past the data
            assert call(s.data, 0, 129, 128) == _ffi.INVALID_ARG         # ldg < len
            assert call(s.data, 0, 129, 129, outs=(None,) * 4) == _ffi.INVALID_ARG
            assert call(s.data, 0, 129, 129, dev=2) == _ffi.INVALID_ARG
            assert call(s.data, 0, 129, 129, pm=C.byref(_ffi.PointMean())) == _ffi.INVALID_ARG   # NULL offsets
            assert call(s.data, 0, 129, 129, pm=C.byref(_ffi.PointMean(ptr(np.zeros(129)), 2, 0))) == _ffi.INVALID_ARG
            assert all(np.all(a == 0.0) for a in (mean, var, dm, dv))
            # one output alone is no error
            assert call(s.data, 0, 129, 129, outs=(None, None, None, dv)) == _ffi.OK
            assert np.array_equal(dv, out0[3])
            # non-finite inputs: non-finite outputs for that point only, SVGP_OK
            xn = p["x"].copy()
            xn[1, 3] = np.nan
            dn = _data(ctx, name, x=xn)
            bad = s.pred.eval(dn, prior_mean=p["mux"])
            dn.free()
            for a, b in zip(bad, out0):
                assert np.all(np.isnan(a[..., 3])) and np.array_equal(np.delete(a, 3, axis=-1), np.delete(b, 3, axis=-1))
            out = s.pred.eval(s.data, prior_mean=p["mux"])
    finally:
        other_d.free()
        other_t.free()
    assert all(np.array_equal(a, b) for a, b in zip(out, out0))
    assert np.all(_errors(out, p["ref"]) <= TOL64)


def test_report_observed_errors():
    """Prints the table profiles/predict_grad/accuracy.md records (run the module with -s)."""
    for name, (err, tol, e32) in OBSERVED.items():
        cells = " | ".join(f"{e:.2e} ({'-' if e32 is None else format(e / max(q, 1e-300), '.2f')})" for e, q in zip(err, np.ones(4) if e32 is None else e32))
        print(f"| {name} | {cells} | {' '.join(format(t, '.1e') for t in tol)} |")
