"""GPU checks of the NearestNeighbors approximation with per-point noise variances and prior-mean offsets (csrc/nn.hip, nn_points.hip:
svgp_nn_set_noise / _set_mean / _lml_grad_points and the vector forms of lml / lml_grad / fit / factors / predict / predict_local)
against tests/nn_noise_ref.py.

Shapes are the seams of tests/test_gpu_nn_sets.py: N in {1, 2, 17, 65, 130, 301}, k in {3, 16, 17, 33, 64}, d in {1, 3, 17}: the k
buckets 16 / 32 / 64, four points per workgroup, the ramp-up rows i < k; every (N, k) pair once, d, layout, dtype and family cycle.
Inputs: nn_ref.synth data, s = exp(U[log 0.02, log 0.5]), diag = 1e-2, mu a smooth function of x, mean_const = 0.1.

Tolerances are the existing suite's for the same quantities: lml 1e-8 (fp64) / 1e-4 (fp32) relative; gradient 1e-6 / 1e-3 of the
largest kernel-parameter entry, d / d diag on its own scale, d / d mean_const = sum_j alpha_j on the scale sum_j |alpha_j| (a sum's
rounding error scales with the magnitudes summed, and E[alpha] = 0 under the model: the sum cancels); factors 1e-9 / 4 eps32 k
variance / diag; predictions 1e-9 / 1e-4 of the largest mean and of the prior variance; s_bar and mean_bar in fp64 1e-6 of the largest
entry.

s_bar and mean_bar in fp32 have no bound fixed ahead: the restatement run in float32 (numpy's LU solves, the per-pair terms rounded to
float32) against itself in float64, on the fp32-rounded inputs of the fp32 cases below (window and random table), is measured on the
CPU when the module starts, and 4 x its worst case over those cases is allowed: the device factorises in registers in another, fixed,
order of summation.  Measured: s_bar 1.90e-5 and mean_bar 1.06e-5 of the largest entry (the worst case is N = 301, k = 64, d = 1,
window), so 7.58e-5 and 4.23e-5 are allowed; the device's worst on an MI355X was 2.13e-5 and 1.18e-5 (the same shape, nearest
table).  profiles/nn/accuracy_noise.md has the table."""
import ctypes as C

import numpy as np
import pytest
import torch

import nn_local_ref as nl
import nn_noise_ref as nn
import nn_ref as nr
import nn_sets_ref as ns
import svgp_oracle as o
from approxgp import GP, DeviceNearestNeighbors, Diagonal, NearestNeighbors, SEKernel, _ffi, approx_lml, approx_lml_and_gradient
from approxgp.kernels import ARDTransform, Matern32Kernel, Matern52Kernel, ScaledKernel, TransformedKernel
from approxgp.nearest_neighbors import NNPosteriorGP

pytestmark = pytest.mark.gpu

F64, F32 = np.float64, np.float32
BASES = {o.KERNEL_SE: SEKernel, o.KERNEL_MATERN32: Matern32Kernel, o.KERNEL_MATERN52: Matern52Kernel}
VAR, DIAG, MC = 1.2, 1e-2, 0.1
WN, WK, WD = [1, 2, 17, 65, 130, 301], [3, 16, 17, 33, 64], [1, 3, 17]


def _kernel(family, var, il):
    return ScaledKernel(TransformedKernel(BASES[family](), ARDTransform(np.asarray(il, dtype=np.float64))), var)


@pytest.fixture(scope="module")
def ctx():
    c = _ffi.Context(0)
    yield c
    c.close()


def _dev(ctx, x, y, dtype, layout=_ffi.COLVECS):
    if layout == _ffi.ROWVECS:
        return DeviceNearestNeighbors(ctx, np.asarray(x).T, y, dtype, layout=_ffi.ROWVECS)
    if layout == _ffi.VEC:
        return DeviceNearestNeighbors(ctx, np.asarray(x)[0], y, dtype)
    return DeviceNearestNeighbors(ctx, x, y, dtype)


def cases():
    """30 cases: every (N, k) pair once; d, layout, dtype and family cycle through them (test_gpu_nn_sets._window_cases)"""
    out = []
    for a, n in enumerate(WN):
        for b, k in enumerate(WK):
            i = a * len(WK) + b
            d = WD[(a + b) % 3]
            layout = _ffi.VEC if d == 1 else [_ffi.COLVECS, _ffi.ROWVECS][(a + i) % 2]
            out.append((n, k, d, layout, [F64, F32][i % 2], (i // 2) % 3))
    assert {c[3] for c in out} == {0, 1, 2} and {(c[4], c[5]) for c in out} == {(t, f) for t in (F64, F32) for f in range(3)}
    return out


def inputs(n, k, d, dtype):
    """(x, y, s, mu) in `dtype`, and the same values in float64 for the restatement"""
    x, y = nr.synth(n, d, seed=4000 + n + k, dtype=dtype)
    s = nn.noise_vector(n, 100 + n + k).astype(dtype)
    mu = nn.mean_vector(x.astype(F64)).astype(dtype)
    return (x, y, s, mu), tuple(a.astype(F64) for a in (x, y, s, mu))


def emulation_error(n, k, d, fam, table):
    """the restatement in float32 against itself in float64 on the fp32-rounded inputs -> (s_bar, mean_bar) errors of the largest entry"""
    _, (x, y, s, mu) = inputs(n, k, d, F32)
    kern = nr.kernel_of(fam, VAR, nr.invl_for(d, True))
    _, sa, ma = nn.point_grads(kern, x, y, table, DIAG, s, mu, MC, dtype=F32)
    _, sb, mb = nn.point_grads(kern, x, y, table, DIAG, s, mu, MC)
    return (float(np.max(np.abs(sa - sb)) / np.max(np.abs(sb))), float(np.max(np.abs(ma - mb)) / np.max(np.abs(mb))))


def emulation_table():
    rows = []
    for n, k, d, layout, dtype, fam in cases():
        if dtype == F32:
            for form, tab in (("window", ns.window_table(n, k)), ("random", nn.random_table(n, k, n + k))):
                rows.append((n, k, d, fam, form) + emulation_error(n, k, d, fam, tab))
    return rows


@pytest.fixture(scope="module")
def bound32():
    """4 x the worst float32-emulation error of s_bar and of mean_bar over the fp32 cases"""
    rows = emulation_table()
    es, em = max(r[5] for r in rows), max(r[6] for r in rows)
    print(f"float32 emulation against float64: s_bar {es:.2e}, mean_bar {em:.2e}; allowed {4 * es:.2e}, {4 * em:.2e}")
    return 4 * es, 4 * em


def _grad_points(dev, desc):
    lml, g, info = dev.lml_grad_points(desc)
    return lml, g


@pytest.mark.parametrize("n,k,d,layout,dtype,fam", cases())
def test_window_and_table_forms_match_the_restatement(ctx, bound32, n, k, d, layout, dtype, fam):
    (x, y, s, mu), (x64, y64, s64, mu64) = inputs(n, k, d, dtype)
    il = nr.invl_for(d, True)
    kern = nr.kernel_of(fam, VAR, il)
    f64 = dtype == F64
    dev = _dev(ctx, x, y, dtype, layout)
    desc, keep = dev.desc(_kernel(fam, VAR, il), k, DIAG, MC)
    dev.set_noise(s)
    dev.set_mean(mu)
    kb = min(k, n - 1)
    xs = np.random.default_rng(n + k).uniform(-2, 2, size=(d, 5)).astype(dtype)
    xs_arg = xs[0] if d == 1 else xs
    for form in ("window", "nearest", "random"):
        if form == "window":
            tab = ns.window_table(n, k)
        elif form == "nearest":
            dev.build_neighbors(k, il)
            tab = dev.neighbors()
        else:
            tab = nn.random_table(n, k, n + k)
            dev.set_neighbors(tab)
        what = f"n {n} k {k} d {d} fam {fam} {np.dtype(dtype).name} {form}"
        lml0, info = dev.lml(desc)
        lml, gv, gil, gd, _ = dev.lml_grad(desc)
        lml_fit, _ = dev.fit(desc)
        B, F, alpha = dev.factors()
        pm, pv, pc = dev.predict(xs_arg, cov=True)
        lml_p, g = _grad_points(dev, desc)
        B2, F2, alpha2 = dev.factors()   # lml_grad_points leaves the handle fitted
        r = nn.fit(kern, x64, y64, tab, DIAG, s64, mu64, MC)
        rl, rv, ril, rd, rm = nn.lml_grad(kern, x64, y64, tab, DIAG, s64, mu64, MC)
        _, rs_bar, rmean_bar = nn.point_grads(kern, x64, y64, tab, DIAG, s64, mu64, MC)
        assert info.first_bad == 0 and lml0 == lml == lml_fit == lml_p
        assert np.array_equal(B, B2) and np.array_equal(F, F2) and np.array_equal(alpha, alpha2)
        assert abs(lml - rl) <= (1e-8 if f64 else 1e-4) * abs(rl), (what, lml, rl)
        gtol = 1e-6 if f64 else 1e-3
        gg, gr = np.concatenate([[gv], gil]), np.concatenate([[rv], ril])
        assert np.max(np.abs(gg - gr)) <= gtol * np.max(np.abs(gr)), (what, gg, gr)
        assert abs(gd - rd) <= gtol * abs(rd), (what, gd, rd)
        assert abs(g["mean_const"] - rm) <= gtol * np.sum(np.abs(rmean_bar)), (what, g["mean_const"], rm)
        tol = 1e-9 if f64 else 4 * np.finfo(F32).eps * k * VAR / DIAG
        Br = ns.table_factors(r["B"], tab)
        if form == "window":   # the band: B[i, t] is the coefficient on point i - kb + t
            Br = nr.banded(r["B"], k)
        else:
            assert np.all(B[tab < 0] == 0)
        assert np.max(np.abs(B - Br), initial=0.0) <= tol * max(np.max(np.abs(Br), initial=0.0), 1e-300), what
        assert np.max(np.abs(F - r["F"]) / r["F"]) <= tol, what
        assert np.max(np.abs(alpha - r["alpha"])) <= tol * np.max(np.abs(r["alpha"])), what
        qm, qv, qc = nr.predict(r, kern, x64, xs.astype(F64))
        tol_m, tol_v = (1e-9 * np.max(np.abs(qm)), 1e-9) if f64 else (1e-4 * np.max(np.abs(qm)), 1e-4 * VAR)
        np.testing.assert_allclose(pm, qm, rtol=0, atol=tol_m, err_msg=what)
        np.testing.assert_allclose(pv, qv, rtol=0, atol=tol_v, err_msg=what)
        np.testing.assert_allclose(pc, qc, rtol=0, atol=tol_v, err_msg=what)
        es = np.max(np.abs(g["noise"] - rs_bar)) / np.max(np.abs(rs_bar))
        em = np.max(np.abs(g["mean"] - rmean_bar)) / np.max(np.abs(rmean_bar))
        bs, bm = (1e-6, 1e-6) if f64 else bound32
        print(f"{what}: s_bar {es:.2e} (allowed {bs:.1e}) mean_bar {em:.2e} (allowed {bm:.1e})")
        assert es <= bs and em <= bm, what
        if f64:   # the sums take other orders: not bitwise
            assert abs(np.sum(g["noise"]) - g["diag"]) <= 1e-12 * abs(g["diag"]), (what, np.sum(g["noise"]), g["diag"])
            assert abs(np.sum(g["mean"]) - g["mean_const"]) <= 1e-12 * abs(g["mean_const"]), (what, np.sum(g["mean"]), g["mean_const"])
        if form == "window":   # a window table with the vectors is no table with the vectors, bitwise in lml and F
            dev.set_neighbors(tab)
            assert dev.fit(desc)[0] == lml and np.array_equal(dev.factors()[1], F), what
    dev.free()


def _hub_problem(dtype):
    n, k, d = 130, 17, 3
    (x, y, s, mu), r64 = inputs(n, k, d, dtype)
    return n, k, d, (x, y, s, mu), r64, nn.hub_table(n, k, (0, 41), 9)


@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_hub_table_strides_the_reverse_lists(ctx, bound32, dtype):
    """point 0 sits in every row (its reverse list has 129 > 64 pairs: the lanes stride it), point 41 in every row after it"""
    n, k, d, (x, y, s, mu), (x64, y64, s64, mu64), tab = _hub_problem(dtype)
    assert np.sum(tab == 0) == 129 and np.sum(tab == 41) == 88
    il = nr.invl_for(d, True)
    kern = nr.kernel_of(o.KERNEL_MATERN52, VAR, il)
    dev = _dev(ctx, x, y, dtype)
    desc, keep = dev.desc(_kernel(o.KERNEL_MATERN52, VAR, il), k, DIAG, MC)
    dev.set_neighbors(tab)
    dev.set_noise(s)
    dev.set_mean(mu)
    lml, g = _grad_points(dev, desc)
    dev.free()
    rl, rs_bar, rmean_bar = nn.point_grads(kern, x64, y64, tab, DIAG, s64, mu64, MC)
    f64 = dtype == F64
    assert abs(lml - rl) <= (1e-8 if f64 else 1e-4) * abs(rl)
    bs, bm = (1e-6, 1e-6) if f64 else bound32
    es = np.max(np.abs(g["noise"] - rs_bar)) / np.max(np.abs(rs_bar))
    em = np.max(np.abs(g["mean"] - rmean_bar)) / np.max(np.abs(rmean_bar))
    print(f"hub {np.dtype(dtype).name}: s_bar {es:.2e} mean_bar {em:.2e}; at the hubs {abs(g['noise'][0] - rs_bar[0]):.2e} {abs(g['noise'][41] - rs_bar[41]):.2e}")
    assert es <= bs and em <= bm
    for j in (0, 41):
        assert abs(g["noise"][j] - rs_bar[j]) <= bs * np.max(np.abs(rs_bar)) and abs(g["mean"][j] - rmean_bar[j]) <= bm * np.max(np.abs(rmean_bar))
    if f64:
        assert abs(np.sum(g["noise"]) - g["diag"]) <= 1e-12 * abs(g["diag"])
        assert abs(np.sum(g["mean"]) - g["mean_const"]) <= 1e-12 * abs(g["mean_const"])


def _state(dev, desc, xs, klocal):
    """everything the plain calls return on this handle state"""
    a = dev.lml_grad(desc)
    l0 = dev.lml(desc)[0]
    lf = dev.fit(desc)[0]
    B, F, alpha = dev.factors()
    p = dev.predict(xs, cov=True)
    loc = dev.predict_local(xs, klocal)
    return [l0, lf, a[0], a[1], a[2], a[3], B, F, alpha, *p, *loc]


def _same(a, b):
    return all(np.array_equal(np.asarray(u), np.asarray(v)) for u, v in zip(a, b))


@pytest.mark.parametrize("n,k,d,dtype,table", [(65, 16, 3, F64, False), (130, 33, 1, F32, True), (301, 64, 3, F32, False),
                                               (17, 17, 17, F64, True)])
def test_consistency_with_the_plain_calls(ctx, n, k, d, dtype, table):
    (x, y, s, mu), _ = inputs(n, k, d, dtype)
    il = nr.invl_for(d, True)
    dev = _dev(ctx, x, y, dtype, _ffi.VEC if d == 1 else _ffi.COLVECS)
    if table:
        dev.set_neighbors(nn.random_table(n, k, 3))
    kern = _kernel(o.KERNEL_MATERN32, VAR, il)
    desc, keep = dev.desc(kern, k, DIAG, MC)
    xs = np.random.default_rng(n).uniform(-2, 2, size=(d, 6)).astype(dtype)
    xs = xs[0] if d == 1 else xs
    never = _state(dev, desc, xs, 5)
    dev.set_noise(s)
    dev.set_mean(mu)
    with_vectors = _state(dev, desc, xs, 5)
    assert with_vectors[0] != never[0]
    dev.set_noise(None)
    dev.set_mean(None)
    assert _same(_state(dev, desc, xs, 5), never)   # set and removed: bitwise the handle that never had them
    # s = c with diag = a is the plain call with diag = a + c
    c = 0.0625
    desc2, keep2 = dev.desc(kern, k, DIAG + c, MC)
    plain = dev.lml_grad(desc2)
    dev.set_noise(np.full(n, c, dtype=dtype))
    got = dev.lml_grad(desc)
    dev.free()
    f64 = dtype == F64
    assert abs(got[0] - plain[0]) <= (1e-8 if f64 else 1e-4) * abs(plain[0])
    gtol = 1e-6 if f64 else 1e-3
    gg, gr = np.concatenate([[got[1]], got[2]]), np.concatenate([[plain[1]], plain[2]])
    assert np.max(np.abs(gg - gr)) <= gtol * np.max(np.abs(gr)) and abs(got[3] - plain[3]) <= gtol * abs(plain[3])


@pytest.mark.parametrize("n,k,d,dtype,table,vectors", [(65, 3, 3, F64, False, False), (65, 16, 3, F32, True, False), (130, 17, 1, F64, True, True),
                                                       (130, 33, 17, F32, False, True), (301, 64, 3, F64, False, False),
                                                       (301, 64, 3, F32, True, True), (17, 33, 3, F32, False, False), (2, 3, 1, F64, False, True)])
def test_bitwise_equalities(ctx, n, k, d, dtype, table, vectors):
    """the scalars of lml_grad_points are lml_grad's, host and device outputs are equal, two calls are equal: bit for bit"""
    (x, y, s, mu), _ = inputs(n, k, d, dtype)
    il = nr.invl_for(d, True)
    dev = _dev(ctx, x, y, dtype, _ffi.VEC if d == 1 else _ffi.COLVECS)
    if table:
        dev.set_neighbors(nn.random_table(n, k, 3))
    if vectors:
        dev.set_noise(torch.as_tensor(s, device="cuda"))   # the device form of the two setters
        dev.set_mean(torch.as_tensor(mu, device="cuda"))
    desc, keep = dev.desc(_kernel(o.KERNEL_SE, VAR, il), k, DIAG, MC)
    a = dev.lml_grad(desc)
    lml, g, info = dev.lml_grad_points(desc)
    assert lml == a[0] and g["variance"] == a[1] and np.array_equal(g["inv_lengthscale"], a[2]) and g["diag"] == a[3]
    lml2, g2, _ = dev.lml_grad_points(desc)
    tdt = torch.float64 if dtype == F64 else torch.float32
    tm, tn = torch.full((n,), 7.0, dtype=tdt, device="cuda"), torch.full((n,), 7.0, dtype=tdt, device="cuda")
    lml3, g3, _ = dev.lml_grad_points(desc, mean_grad_out=tm, noise_grad_out=tn)
    torch.cuda.synchronize()
    assert g3["mean"] is tm and g3["noise"] is tn
    for other, gm, gn in ((g2, g2["mean"], g2["noise"]), (g3, tm.cpu().numpy(), tn.cpu().numpy())):
        assert np.array_equal(gm, g["mean"]) and np.array_equal(gn, g["noise"])
        assert other["mean_const"] == g["mean_const"] and other["diag"] == g["diag"] and other["variance"] == g["variance"]
    assert lml2 == lml == lml3
    if vectors:   # the host form of the setters gives the same bits
        dev.set_noise(s)
        dev.set_mean(mu)
        lml4, g4, _ = dev.lml_grad_points(desc)
        assert lml4 == lml and np.array_equal(g4["noise"], g["noise"]) and np.array_equal(g4["mean"], g["mean"])
    dev.free()


@pytest.mark.parametrize("nstar", [1, 5, 65])
@pytest.mark.parametrize("dtype", [F64, F32], ids=["f64", "f32"])
def test_predict_local_with_vectors(ctx, nstar, dtype):
    n, d = 130, 3
    (x, y, s, mu), (x64, y64, s64, mu64) = inputs(n, 16, d, dtype)
    il = nr.invl_for(d, True)
    kern = nr.kernel_of(o.KERNEL_MATERN52, VAR, il)
    dev = _dev(ctx, x, y, dtype)
    dev.set_noise(s)
    dev.set_mean(mu)
    dev.fit(dev.desc(_kernel(o.KERNEL_MATERN52, VAR, il), 8, DIAG, MC)[0])
    xs = np.random.default_rng(nstar).uniform(-2, 2, size=(d, nstar)).astype(dtype)
    for k in (1, 16, 17, 64):
        m, v, tab = dev.predict_local(xs, k, neighbors=True)
        rm, rv = nn.predict_local(kern, x64, y64, xs.astype(F64), tab, DIAG, s64, mu64, MC)
        tm, tv = (1e-9, 1e-9) if dtype == F64 else (1e-4, 1e-4)
        em, ev = np.max(np.abs(m - rm)) / np.max(np.abs(rm)), np.max(np.abs(v - rv)) / VAR
        print(f"n* {nstar} k {k} {np.dtype(dtype).name}: mean {em:.2e} var {ev:.2e}")
        assert tab.shape == (nstar, k) and em <= tm and ev <= tv
        plain = nl.predict_local(kern, x64, y64, xs.astype(F64), tab, DIAG, MC)
        assert np.max(np.abs(rm - plain[0])) > 1e-3   # the vectors matter on these inputs
    dev.free()


def test_posterior_with_per_point_noise(ctx):
    n, d, k = 65, 3, 64   # 64 neighbours of 65 points: the exact GP, whose latent variances are positive (predict_y needs them so)
    (x, y, s, mu), _ = inputs(n, k, d, F64)
    il = nr.invl_for(d, True)
    kern = nr.kernel_of(o.KERNEL_SE, VAR, il)
    v = DIAG + s
    f = GP(MC, _kernel(o.KERNEL_SE, VAR, il))
    app = NearestNeighbors(k, include_noise=True, neighbors="nearest")
    post = NNPosteriorGP(app, f(x, Diagonal(v)), y, ctx=ctx, mean_offsets=mu)
    tab = post.dev.neighbors()
    r = nn.fit(kern, x, y, tab, DIAG, s, mu, MC)   # diag = min(v), s = v - min(v): the same variances
    assert abs(post.lml - r["lml"]) <= 1e-8 * abs(r["lml"])
    xs = np.random.default_rng(4).uniform(-2, 2, size=(d, 9))
    off = nn.mean_vector(xs)
    qm, qv, _ = nr.predict(r, kern, x, xs)
    m, var = post.mean_and_var(xs, mean_offsets=off)
    np.testing.assert_allclose(m, qm + off, rtol=0, atol=1e-9 * np.max(np.abs(qm)))
    np.testing.assert_allclose(var, qv, rtol=0, atol=1e-9)
    with pytest.raises(ValueError, match="pass noise="):
        post.predict_y(xs)
    ym, yv = post.predict_y(xs, noise=0.2)
    np.testing.assert_allclose(yv, var + 0.2, rtol=1e-12)
    nv = np.linspace(0.05, 0.3, 9)
    ym, yv = post.predict_y(xs, noise=nv)
    np.testing.assert_allclose(yv, var + nv, rtol=1e-12)
    lpd = post.log_predictive_density(xs, np.zeros(9), noise=nv)
    np.testing.assert_allclose(lpd, -0.5 * (np.log(2 * np.pi * yv) + ym ** 2 / yv), rtol=1e-12)
    lm, lv = post.local_mean_and_var(xs, mean_offsets=off)
    qt = nn.query_table(x, xs, k, il)
    rm, rv = nn.predict_local(kern, x, y, xs, qt, float(v.min()), v - v.min(), mu, MC)
    np.testing.assert_allclose(lm, rm + off, rtol=0, atol=1e-9 * np.max(np.abs(rm)))
    np.testing.assert_allclose(lv, rv, rtol=0, atol=1e-9)
    post.dev.free()
    # the three dispatches, and the gradient's new keys
    fx = f(x, Diagonal(v))
    val = approx_lml(app, fx, y, ctx=ctx, mean_offsets=mu)
    assert abs(val - r["lml"]) <= 1e-8 * abs(r["lml"])
    val2, g = approx_lml_and_gradient(app, fx, y, ctx=ctx, mean_offsets=mu)
    assert val2 == val and set(g) == {"variance", "inv_lengthscale", "diag"}
    val3, g3 = approx_lml_and_gradient(app, fx, y, ctx=ctx, mean_offsets=mu, wrt_noise=True, wrt_mean=True)
    assert val3 == val and set(g3) == {"variance", "inv_lengthscale", "diag", "Sigma_y", "mean", "mean_const"}
    assert g3["variance"] == g["variance"] and g3["diag"] == g["diag"]
    _, rs_bar, rmean_bar = nn.point_grads(kern, x, y, tab, float(v.min()), v - v.min(), mu, MC)
    assert np.max(np.abs(g3["Sigma_y"] - rs_bar)) <= 1e-6 * np.max(np.abs(rs_bar))
    assert np.max(np.abs(g3["mean"] - rmean_bar)) <= 1e-6 * np.max(np.abs(rmean_bar))


def test_statuses(ctx):
    n, k, d = 65, 16, 3
    (x, y, s, mu), _ = inputs(n, k, d, F64)
    il = nr.invl_for(d, True)
    dev = _dev(ctx, x, y, F64)
    desc, keep = dev.desc(_kernel(o.KERNEL_SE, VAR, il), k, DIAG, MC)
    healthy = dev.fit(desc)[0]
    xs = np.zeros((d, 3))
    dev.predict(xs)
    lib, h = ctx.lib, ctx.h
    # a variance below zero, and a NaN: SVGP_NOT_POSDEF before any launch, first_bad 0
    for bad in (-2 * DIAG, float("nan")):
        sb = s.copy()
        sb[7] = bad
        dev.set_noise(sb)
        for call in (dev.lml, dev.lml_grad, dev.fit, dev.lml_grad_points):
            with pytest.raises(_ffi.PosDefException) as e:
                call(desc)
            assert e.value.info == 0
        lml, info = C.c_double(1.0), _ffi.NNInfo(first_bad=9)
        assert lib.svgp_nn_lml(h, dev.h, C.byref(desc), C.byref(lml), C.byref(info)) == _ffi.NOT_POSDEF
        assert np.isnan(lml.value) and info.first_bad == 0 and np.isnan(info.lml)
    sz = s.copy()
    sz[7] = -DIAG   # diag + s = 0 exactly: allowed, as diag = 0 is
    dev.set_noise(sz)
    assert np.isfinite(dev.lml(desc)[0])
    dev.set_noise(None)
    assert dev.fit(desc)[0] == healthy   # a healthy call on the same handle afterwards
    # NaN in mu: NaN lml, SVGP_OK
    mb = mu.copy()
    mb[3] = float("nan")
    dev.set_mean(mb)
    lml, info = dev.lml(desc)
    assert np.isnan(lml) and info.first_bad == 0
    dev.set_mean(None)
    # argument checks
    buf = np.ascontiguousarray(s)
    for pn in (_ffi.PointNoise(_ffi._ptr(buf), 2, 0), _ffi.PointNoise(_ffi._ptr(buf), 0, 1), _ffi.PointNoise(None, 0, 0)):
        assert lib.svgp_nn_set_noise(h, dev.h, C.byref(pn)) == _ffi.INVALID_ARG
    for pm in (_ffi.PointMean(_ffi._ptr(buf), -1, 0), _ffi.PointMean(_ffi._ptr(buf), 1, 5), _ffi.PointMean(None, 0, 0)):
        assert lib.svgp_nn_set_mean(h, dev.h, C.byref(pm)) == _ffi.INVALID_ARG
    out = np.zeros(n)
    lml, info, dv, dil = C.c_double(), _ffi.NNInfo(), C.c_double(), np.zeros(d)
    for gpm, gpn in ((_ffi.PointMeanGrad(_ffi._ptr(out), 2, 0), None), (None, _ffi.PointNoiseGrad(_ffi._ptr(out), 0, 3)),
                     (_ffi.PointMeanGrad(None, 0, 0), None)):
        rc = lib.svgp_nn_lml_grad_points(h, dev.h, C.byref(desc), C.byref(lml), C.byref(info), C.byref(dv),
                                         dil.ctypes.data_as(C.POINTER(C.c_double)), None, None,
                                         C.byref(gpm) if gpm is not None else None, C.byref(gpn) if gpn is not None else None)
        assert rc == _ffi.INVALID_ARG
    # every output of lml_grad_points may be NULL but the kernel blocks
    rc = lib.svgp_nn_lml_grad_points(h, dev.h, C.byref(desc), C.byref(lml), C.byref(info), C.byref(dv),
                                     dil.ctypes.data_as(C.POINTER(C.c_double)), None, None, None, None)
    assert rc == _ffi.OK and lml.value == healthy
    # setting a vector discards the fit
    dev.fit(desc)
    dev.predict(xs)
    for setter, vec in ((dev.set_noise, s), (dev.set_mean, mu), (dev.set_noise, None), (dev.set_mean, None)):
        dev.fit(desc)
        setter(vec)
        m = np.zeros(3)
        assert lib.svgp_nn_predict(h, dev.h, _ffi.COLVECS, 3, _ffi._ptr(np.asfortranarray(xs)), _ffi._ptr(m), None, None) == _ffi.INVALID_ARG
        with pytest.raises(Exception):
            dev.predict_local(xs, 4)
    dev.fit(desc)
    dev.predict(xs)
    dev.free()
