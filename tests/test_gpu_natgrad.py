"""GPU checks of the natural-gradient step on q(u) (svgp_natgrad_step / _ext, svgp_model_update_keep_q) against the float64
restatement tests/natgrad_ref.py.

Shapes: the smallest that cross every boundary - M below, one past and between 128-row panels (64, 129, 130, 200), one 65 536-point
chunk boundary (70 001 points: two chunks, the non-overlapped SYRK), a window offset, d = 1, 17 and 64; both parametrisations, the
uniform-weight and the weighted SYRK, gamma = 1 (Lambda never formed) and gamma < 1.  fp32: measured against the fp64 restatement on
fp32-rounded inputs, asserted at 4x the worst measured value (see F32_MEASURED)."""
import ctypes as C
import functools

import numpy as np
import pytest

import natgrad_ref as nr
import svgp_oracle as o
from approxgp import _ffi
from helpers import desc_from_oracle, device_model

pytestmark = pytest.mark.gpu
JITTER = 1e-5
JITTER_F32 = 1e-3     # the project's fp32 problems carry the larger jitter (approxgp/synthetic.py): an fp32 cholesky(Kuu) needs it

# (n, M, d, likelihood, quadrature_n, family, ard, layout, centered, mean_const, batch_off, gamma, num_data (None: n))
CASES = {
    "gauss_n777_M200_d3": (777, 200, 3, o.LIK_GAUSSIAN, 0, o.KERNEL_SE, True, _ffi.COLVECS, False, 0.0, 0, 0.5, None),
    "poisson_n1000_M130_d8": (1000, 130, 8, o.LIK_POISSON_EXP, 0, o.KERNEL_MATERN32, True, _ffi.ROWVECS, True, -0.4, 0, 1.0, None),
    "bernoulli_n640_M129_d17": (640, 129, 17, o.LIK_BERNOULLI_LOGISTIC, 20, o.KERNEL_SE, False, _ffi.COLVECS, True, 0.0, 37, 0.3, 5000.0),
    "gauss_gh7_n513_M64_d64": (513, 64, 64, o.LIK_GAUSSIAN, 7, o.KERNEL_MATERN52, False, _ffi.COLVECS, False, 0.0, 0, 0.7, None),
    "normcdf_n513_M64_d1": (513, 64, 1, o.LIK_BERNOULLI_NORMCDF, 0, o.KERNEL_SE, False, _ffi.VEC, False, 0.0, 0, 1.0, None),
    "gauss_n70001_M64_d2": (70001, 64, 2, o.LIK_GAUSSIAN, 0, o.KERNEL_SE, True, _ffi.COLVECS, False, 0.0, 0, 0.5, None),
}
F32_CASES = {
    "f32_gauss_n1000_M256_d4": (1000, 256, 4, o.LIK_GAUSSIAN, 0, o.KERNEL_SE, True, _ffi.COLVECS, False, 0.0, 0, 0.5, None),
    "f32_bernoulli_n640_M129_d17": (640, 129, 17, o.LIK_BERNOULLI_LOGISTIC, 20, o.KERNEL_SE, False, _ffi.COLVECS, True, 0.0, 37, 0.3, 5000.0),
    "f32_gauss_n70001_M64_d2": (70001, 64, 2, o.LIK_GAUSSIAN, 0, o.KERNEL_SE, True, _ffi.COLVECS, False, 0.0, 0, 0.5, None),
}
# fp32 against the fp64 restatement on fp32-rounded inputs, worst value over F32_CASES as measured on an MI355X (relative to each
# block's largest entry and to |elbo|); the asserts below take 4x these (box-to-box reduction-order differences).  Per case (m, S, elbo):
# n = 1000 M = 256: 3.7e-3, 4.0e-5, 5.1e-6; Centered Bernoulli n = 640 M = 129: 9.1e-6, 9.7e-6, 9.0e-8; n = 70 001 M = 64: 5.1e-1, 1.2e-4,
# 1.8e-5.  m is loose where a Gaussian likelihood with many points dominates the step: a = scale A g_mu and W m_w are each ~ n / sigma^2
# times their sum b / sigma^2, and a carries the fp32 rounding of the data pass's posterior means, so m moves by eps_fp32 n / sigma^2 in the
# directions the data hardly determine.  The ELBO at the new q and S stay inside the fp32 contract (1e-4); fp64 has 1e-9 there.
F32_MEASURED = {"m": 5.07e-1, "S": 1.24e-4, "elbo": 1.82e-5}


@pytest.fixture(scope="module")
def ctx():
    c = _ffi.Context(0)
    yield c
    c.close()


def _jitter(name):
    return JITTER_F32 if name.startswith("f32") else JITTER


def _dtype(name):
    return np.float32 if name.startswith("f32") else np.float64


@functools.lru_cache(maxsize=None)
def _problem(name):
    """(spec, kernel, x, y, s2, window, starting SVA, SVA after the step, ELBO at the new q) - the reference, computed once."""
    spec = {**CASES, **F32_CASES}[name]
    n, M, d, lik, qn, family, ard, layout, centered, mc, off, gamma, num_data = spec
    dtype = _dtype(name)
    kernel, z, x, y, s2, m0, Lq0 = nr.problem(n + off + (11 if off else 0), M, d, lik=lik, family=family, ard=ard, dtype=dtype, mean_const=mc)
    start = nr.start_sva(kernel, z, _jitter(name), m0, Lq0, mean_const=mc, centered=centered)
    if dtype == np.float32:   # the device holds q in fp32: the reference starts from the same rounded values
        start = o.SVA(kernel, z, start.m.astype(np.float32).astype(np.float64), start.Lq.astype(np.float32).astype(np.float64),
                      jitter=start.jitter, mean_const=mc, centered=centered)
    xw, yw = x[:, off:off + n], y[off:off + n]
    new = nr.step(start, xw, yw, lik=lik, sigma2=s2, num_data=num_data, gamma=gamma, quadrature_n=qn)
    elbo_new = o.elbo(new, xw, yw, lik=lik, sigma2=s2, num_data=num_data, quadrature_n=qn)
    for a in (x, y, xw, yw, start.m, start.Lq, new.m, new.Lq):
        a.setflags(write=False)
    return spec, kernel, x, y, s2, (xw, yw), start, new, elbo_new


def _data(ctx, name):
    spec, kernel, x, y, s2, _, start, _, _ = _problem(name)
    d, layout = spec[2], spec[7]
    xd = x[0] if d == 1 else (x if layout == _ffi.COLVECS else np.ascontiguousarray(x.T))
    return _ffi.DeviceData(ctx, xd, y, _dtype(name), layout=layout if d > 1 else _ffi.VEC)


def _model(ctx, name, sva=None, **kw):
    spec, kernel, x, y, s2, _, start, _, _ = _problem(name)
    return device_model(ctx, sva if sva is not None else start, dtype=_dtype(name), lik=spec[3], sigma2=s2, quadrature_n=spec[4], **kw)


def _nd(spec):
    return 0.0 if spec[12] is None else spec[12]


def _block_err(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _cov(Lq):
    Lq = np.asarray(Lq, dtype=np.float64)
    return Lq @ Lq.T


def _with_q(sva, m, Lq):
    return o.SVA(sva.kernel, sva.z, np.asarray(m, dtype=np.float64), np.asarray(Lq, dtype=np.float64), jitter=sva.jitter,
                 mean_const=sva.mean_const, centered=sva.centered)


def _errors_of_a_step(ctx, name):
    """One step on the device -> the errors of m, S = Lq Lq' and of svgp_elbo on the updated model against the restatement."""
    spec, kernel, x, y, s2, _, start, new, elbo_new = _problem(name)
    n, off, gamma = spec[0], spec[10], spec[11]
    model, data = _model(ctx, name), _data(ctx, name)
    try:
        _, _, _, m, Lq = model.natgrad_step(data, off, n, _nd(spec), gamma=gamma)
        assert np.array_equal(np.triu(Lq, 1), np.zeros_like(Lq)) and np.all(np.diag(Lq) > 0)
        val, _ = model.elbo(data, off, n, _nd(spec))
    finally:
        model.free()
        data.free()
    return {"m": _block_err(m, new.m), "S": _block_err(_cov(Lq), _cov(new.Lq)), "elbo": abs(val - elbo_new) / abs(elbo_new)}


@pytest.mark.parametrize("name", list(CASES))
def test_step_matches_the_restatement(ctx, name):
    err = _errors_of_a_step(ctx, name)
    print(f"{name}: m {err['m']:.2e} S {err['S']:.2e} elbo {err['elbo']:.2e}")
    assert err["m"] < 1e-8 and err["S"] < 1e-8 and err["elbo"] < 1e-8      # the project's fp64 contract


@pytest.mark.parametrize("name", list(CASES))
def test_values_at_the_old_q_are_bitwise_those_of_elbo_grad(ctx, name):
    spec = _problem(name)[0]
    n, off, gamma = spec[0], spec[10], spec[11]
    twin, model, data = _model(ctx, name), _model(ctx, name), _data(ctx, name)
    try:
        v0, t0, g0 = twin.elbo_grad(data, off, n, _nd(spec))
        v1, t1, g1, _, _ = model.natgrad_step(data, off, n, _nd(spec), gamma=gamma, want_grads=True, fetch=False)
        assert v0 == v1
        for f, _ in _ffi.Terms._fields_:
            assert getattr(t0, f) == getattr(t1, f), f
        for k in ("variance", "lik_sigma2", "mean_const"):
            assert g0[k] == g1[k], k
        for k in ("inv_lengthscale", "z", "m", "Lq"):
            assert np.array_equal(g0[k], g1[k]), k
    finally:
        twin.free()
        model.free()
        data.free()


@pytest.mark.parametrize("centered", [False, True], ids=["noncentered", "centered"])
def test_full_step_gaussian_full_batch_is_collapsed_q(ctx, centered):
    """gamma = 1, Gaussian likelihood, num_data = n: the q after the step is the q after svgp_collapsed_q on a twin, from any start."""
    kernel, z, x, y, s2, m0, Lq0 = nr.problem(777, 200, 3, ard=True, mean_const=0.3 if centered else 0.0)
    start = nr.start_sva(kernel, z, JITTER, m0, Lq0, mean_const=0.3 if centered else 0.0, centered=centered)
    data = _ffi.DeviceData(ctx, x, y, np.float64)
    model, twin = device_model(ctx, start, sigma2=s2), device_model(ctx, start, sigma2=s2)
    try:
        _, _, _, m, Lq = model.natgrad_step(data, 0, 777, gamma=1.0)
        bound, mc, Lqc = twin.collapsed_q(data, 0, 777)
        val, _ = model.elbo(data, 0, 777)
        e_m, e_S, e_b = _block_err(m, mc), _block_err(_cov(Lq), _cov(Lqc)), abs(val - bound) / abs(bound)
        print(f"centered={centered}: m {e_m:.2e} S {e_S:.2e} elbo after the step against collapsed_bound {e_b:.2e}")
        assert e_m < 1e-9 and e_S < 1e-9 and e_b < 1e-9
    finally:
        model.free()
        twin.free()
        data.free()


def test_eight_half_steps_reach_a_fixed_point(ctx):
    """NonCentered, Bernoulli-logistic GH-20, n = 640, M = 129, num_data = 2000: every step's ELBO exceeds the previous one and the
    Euclidean gradients in q fall below 2 % of their starting values (the restatement reaches 0.4 % and 0.1 %)."""
    lik = o.LIK_BERNOULLI_LOGISTIC
    kernel, z, x, y, _, m0, Lq0 = nr.problem(640, 129, 2, lik=lik, seed=1)
    data = _ffi.DeviceData(ctx, x, y, np.float64)
    model = device_model(ctx, nr.start_sva(kernel, z, JITTER, m0, Lq0), lik=lik, quadrature_n=20)
    try:
        vals, g_first = [], None
        for _ in range(8):
            v, _, g, _, _ = model.natgrad_step(data, 0, 640, 2000.0, gamma=0.5, want_grads=True, fetch=False)
            vals.append(v)
            g_first = g_first or g
        v, _, g = model.elbo_grad(data, 0, 640, 2000.0)
        vals.append(v)
        r_m, r_L = np.abs(g["m"]).max() / np.abs(g_first["m"]).max(), np.abs(g["Lq"]).max() / np.abs(g_first["Lq"]).max()
        print("elbo:", " ".join(f"{v:.6f}" for v in vals), f"| m_bar ratio {r_m:.2e} Lq_bar ratio {r_L:.2e}")
        assert all(b > a for a, b in zip(vals, vals[1:]))
        assert r_m < 0.02 and r_L < 0.02
    finally:
        model.free()
        data.free()


@pytest.mark.parametrize("name", ["gauss_n777_M200_d3", "bernoulli_n640_M129_d17"])
def test_bitwise_repeatable(ctx, name):
    spec, kernel, x, y, s2, _, start, _, _ = _problem(name)
    n, off, gamma = spec[0], spec[10], spec[11]
    a, b, data = _model(ctx, name), _model(ctx, name), _data(ctx, name)
    try:
        _, _, _, ma, La = a.natgrad_step(data, off, n, _nd(spec), gamma=gamma)
        _, _, _, mb, Lb = b.natgrad_step(data, off, n, _nd(spec), gamma=gamma)
        assert np.array_equal(ma, mb) and np.array_equal(La, Lb)
        fresh = _model(ctx, name, _with_q(start, ma, La))
        try:
            assert fresh.elbo(data, off, n, _nd(spec))[0] == a.elbo(data, off, n, _nd(spec))[0]
        finally:
            fresh.free()
    finally:
        a.free()
        b.free()
        data.free()


def test_ext_agrees_with_the_built_in_step(ctx):
    """svgp_natgrad_step_ext with g_mu / g_v from svgp_marginals and the oracle's expected_loglik_grads: the Bernoulli case."""
    name = "bernoulli_n640_M129_d17"
    spec, kernel, x, y, s2, (xw, yw), start, new, _ = _problem(name)
    n, off, gamma, lik, qn = spec[0], spec[10], spec[11], spec[3], spec[4]
    builtin, model, data = _model(ctx, name), _model(ctx, name), _data(ctx, name)
    try:
        v0, _, _, m0, L0 = builtin.natgrad_step(data, off, n, _nd(spec), gamma=gamma)
        mu, var = model.marginals(data, off, n)
        gmu, gv, _ = o.expected_loglik_grads(lik, mu, var, yw, 1.0, qn)
        sum_e = o.expected_loglik(lik, mu, np.sqrt(var), yw, 1.0, qn)
        v1, _, _, m1, L1 = model.natgrad_step(data, off, n, _nd(spec), gamma=gamma, ext=(sum_e, gmu, gv))
        e_m, e_S = _block_err(m1, m0), _block_err(_cov(L1), _cov(L0))
        print(f"_ext against the built-in step: m {e_m:.2e} S {e_S:.2e} elbo {abs(v1 - v0) / abs(v0):.2e}")
        assert e_m < 1e-9 and e_S < 1e-9 and abs(v1 - v0) < 1e-9 * abs(v0)
    finally:
        builtin.free()
        model.free()
        data.free()


def test_update_keep_q_keeps_the_device_resident_q(ctx):
    name = "gauss_n777_M200_d3"
    spec, kernel, x, y, s2, _, start, _, _ = _problem(name)
    n, gamma = spec[0], spec[11]
    rng = np.random.default_rng(5)
    kernel2 = o.Kernel(kernel.family, 1.2 * kernel.variance, kernel.inv_lengthscale * (0.8 + 0.3 * rng.random(kernel.d)))
    z2 = start.z + 0.02 * rng.standard_normal(start.z.shape)
    changed = o.SVA(kernel2, z2, start.m, start.Lq, jitter=JITTER)   # new hyperparameters, the STALE starting q
    model, twin, data = _model(ctx, name), _model(ctx, name), _data(ctx, name)
    try:
        _, _, _, m, Lq = model.natgrad_step(data, 0, n, gamma=gamma)
        twin.natgrad_step(data, 0, n, gamma=gamma, fetch=False)
        desc, keep = desc_from_oracle(changed, sigma2=1.1 * s2)
        twin.update(desc, keep)                                       # plain svgp_model_update still overwrites q
        desc.m, desc.Lq = None, None
        model.update_keep_q(desc, keep)
        kept = device_model(ctx, _with_q(changed, m, Lq), sigma2=1.1 * s2)
        stale = device_model(ctx, changed, sigma2=1.1 * s2)
        try:
            v_keep, v_twin = model.elbo(data, 0, n)[0], twin.elbo(data, 0, n)[0]
            v_kept_ref, v_stale_ref = kept.elbo(data, 0, n)[0], stale.elbo(data, 0, n)[0]
        finally:
            kept.free()
            stale.free()
        print(f"update_keep_q {v_keep:.12g} fresh model with the fetched q {v_kept_ref:.12g}; model_update {v_twin:.12g} stale q {v_stale_ref:.12g}")
        assert abs(v_keep - v_kept_ref) <= 1e-12 * abs(v_kept_ref)
        assert abs(v_twin - v_stale_ref) <= 1e-12 * abs(v_stale_ref) and abs(v_twin - v_keep) > 1e-6 * abs(v_keep)
    finally:
        model.free()
        twin.free()
        data.free()


def test_errors_leave_q_and_the_context_usable(ctx):
    name = "bernoulli_n640_M129_d17"
    spec, kernel, x, y, s2, _, start, new, _ = _problem(name)
    n, M, off, gamma = spec[0], spec[1], spec[10], spec[11]
    model, data = _model(ctx, name), _data(ctx, name)

    def healthy():
        probe = _model(ctx, name)
        try:
            _, _, _, m, _ = probe.natgrad_step(data, off, n, _nd(spec), gamma=gamma)
            assert _block_err(m, new.m) < 1e-8
        finally:
            probe.free()

    try:
        before = model.elbo(data, off, n, _nd(spec))[0]
        for bad in (0.0, -0.1, 1.5, float("nan")):
            with pytest.raises(ValueError, match="gamma"):
                model.natgrad_step(data, off, n, _nd(spec), gamma=bad)
            healthy()
        with pytest.raises(ValueError, match="batch range"):             # what svgp_elbo_grad rejects
            model.natgrad_step(data, data.n - 5, n, gamma=gamma)
        healthy()
        model.set_mean_z(np.zeros(M))                                    # a model with muz: SVGP_UNSUPPORTED
        with pytest.raises(_ffi.UnsupportedError):
            model.natgrad_step(data, off, n, _nd(spec), gamma=gamma)
        model.set_mean_z(None)
        healthy()
        with pytest.raises(_ffi.PosDefException, match="order"):         # a caller's g_v > 0: Lambda' is not positive definite
            model.natgrad_step(data, off, n, _nd(spec), gamma=gamma, ext=(0.0, np.zeros(n), np.full(n, 10.0)))
        assert model.elbo(data, off, n, _nd(spec))[0] == before          # q exactly as it was
        healthy()
        assert model.elbo(data, off, n, _nd(spec))[0] == before
    finally:
        model.free()
        data.free()


def test_nan_coordinate_gives_nan_not_an_error(ctx):
    name = "gauss_n777_M200_d3"
    spec, kernel, x, y, s2, _, start, _, _ = _problem(name)
    xn = x.copy()
    xn[1, 500] = np.nan
    data = _ffi.DeviceData(ctx, xn, y, np.float64)
    model = _model(ctx, name)
    try:
        val, _, _, m, Lq = model.natgrad_step(data, 0, 777, gamma=0.5)
        assert np.isnan(val) and np.all(np.isnan(m)) and np.all(np.isnan(Lq[np.tril_indices(200)])) and not np.triu(Lq, 1).any()
    finally:
        model.free()
    model = _model(ctx, name)
    try:   # the window that leaves the point out is healthy
        val, _, _, m, _ = model.natgrad_step(data, 0, 500, gamma=0.5)
        assert np.isfinite(val) and np.all(np.isfinite(m))
    finally:
        model.free()
        data.free()


def test_fp32_accuracy(ctx):
    worst = {k: 0.0 for k in F32_MEASURED}
    for name in F32_CASES:
        err = _errors_of_a_step(ctx, name)
        print(f"{name}: m {err['m']:.2e} S {err['S']:.2e} elbo {err['elbo']:.2e}")
        worst = {k: max(worst[k], err[k]) for k in worst}
    print("fp32 worst:", {k: f"{v:.2e}" for k, v in worst.items()})
    for k, v in worst.items():
        assert v <= 4 * F32_MEASURED[k], (k, v)


def test_python_top_layer(ctx):
    """approxgp.natural_gradient_step: the round trip through the package's own types, both ways of giving the likelihood."""
    import approxgp as ag
    name = "gauss_n777_M200_d3"
    spec, kernel, x, y, s2, _, start, new, elbo_new = _problem(name)
    f = ag.GP(kernel.variance * (ag.SqExponentialKernel() @ ag.ARDTransform(list(kernel.inv_lengthscale))))
    fz, fx = f(start.z, JITTER), f(x, s2)
    sva = ag.SparseVariationalApproximation(fz, ag.MvNormal.from_cholesky(start.m, start.Lq))
    stepped, old = ag.natural_gradient_step(sva, fx, y, step=spec[11], ctx=ctx)
    assert isinstance(stepped, ag.SparseVariationalApproximation) and not stepped.is_centered and stepped.fz is fz
    assert abs(old - ag.elbo(sva, fx, y, ctx=ctx)) <= 1e-12 * abs(old)
    assert _block_err(stepped.q.m, new.m) < 1e-8 and _block_err(_cov(stepped.q.chol_lower), _cov(new.Lq)) < 1e-8
    assert abs(ag.elbo(stepped, fx, y, ctx=ctx) - elbo_new) < 1e-8 * abs(elbo_new)
    lfx = ag.LatentFiniteGP(f(x, 1e-18), ag.GaussianLikelihood(s2))
    again, _ = ag.natural_gradient_step(sva, lfx, y, step=spec[11], ctx=ctx)
    assert _block_err(again.q.m, new.m) < 1e-8
    with pytest.raises(ValueError, match="step"):
        ag.natural_gradient_step(sva, fx, y, step=0.0, ctx=ctx)
