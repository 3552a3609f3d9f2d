"""Seeded slices of tests/fuzz_families.py (the stateful sweep over the natgrad, collapsed, predictive and prior-mean calls interleaved
with the older ones on one context) and five short hand-written sequences, one per place where the host layer keeps something between
calls, plus the sequences the long run flagged.  Every op is checked against its family's float64 restatement AND, bitwise, against the
same op on a context that is opened for that one op and closed after it.

500 ops and four slots per slice; SLICE_TIMES: the wall time of each as measured on an MI355X with the twin check on every op (the float64
restatements on the host are most of it)."""
import pytest

import fuzz_families as ff
import svgp_oracle as o
from approxgp import _ffi

pytestmark = pytest.mark.gpu
SLICE_TIMES = {"f64": 9.2, "f32": 8.4, "mixed": 9.3}   # seconds for fuzz_families.SLICE_OPS = 500 ops


@pytest.fixture(scope="module")
def ctx():
    c = _ffi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def twin_ctx():
    """Not a context but the recipe for one: every twin op opens a new context and closes it afterwards, so that the twin's workspaces,
    buffers, cached rule and staging have seen that one op only."""
    return ff.fresh_context


def _run(ctx, twin_ctx, plan):
    results = ff.execute(ctx, plan, twin_ctx)
    for key, v in sorted(ff.worst(results).items()):
        print("worst", key, f"{v:.2e}")
    assert all("twin" in errs for rec, errs in results if rec["kind"] not in ("create", "update"))
    bad = ff.failures(results)
    assert not bad, bad


@pytest.mark.parametrize("name", list(ff.SLICES))
def test_random_sequence_over_the_call_families(ctx, twin_ctx, name):
    _run(ctx, twin_ctx, ff.slice_plan(name))


def test_collapsed_workspace_shared_by_models_of_one_padding(ctx, twin_ctx):
    """(a) CollapsedWs is cached by Mp alone and zeroed at creation only: M = 129 and M = 200 (both Mp 256) alternate between a
    gamma < 1 step, which factors into TB three times, and the collapsed calls; M = 64 rebuilds the workspace in between."""
    specs = {0: ff.spec_of(129, 500, 3, seed=11), 1: ff.spec_of(200, 1025, 8, seed=12, centered=True), 2: ff.spec_of(64, 127, 2, seed=13)}
    _run(ctx, twin_ctx, ff.script(specs, [
        ("natgrad", 0, dict(gamma=0.3)), ("collapsed_bound", 1, {}), ("collapsed_q", 1, {}), ("natgrad", 0, dict(gamma=1.0)),
        ("collapsed_q", 2, {}), ("natgrad", 1, dict(gamma=0.7, want_grads=True))]))


def test_chunking_does_not_come_from_an_older_call(ctx, twin_ctx):
    """(b) the gradient workspace built for 3000 points serves a collapsed bound on 33 of them, then the collapsed gradient on all."""
    specs = {0: ff.spec_of(128, 3000, 3, seed=21)}
    _run(ctx, twin_ctx, ff.script(specs, [
        ("grad", 0, {}), ("collapsed_bound", 0, dict(off=1400, nb=33)), ("collapsed_grad", 0, dict(inputs=True))]))


def test_every_reader_prepares_after_a_device_side_q(ctx, twin_ctx):
    """(c) q written device to device and not fetched: the prep is left to svgp_predictive, svgp_predict, svgp_elbo_grad behind a
    keep_q, svgp_marginals behind a keep_q."""
    logit = dict(lik=o.LIK_BERNOULLI_LOGISTIC, quadrature_n=20)
    specs = {0: ff.spec_of(129, 500, 2, seed=31, **logit), 1: ff.spec_of(100, 500, 17, seed=32, lik=o.LIK_POISSON_EXP, centered=True),
             2: ff.spec_of(200, 1025, 3, seed=33), 3: ff.spec_of(64, 127, 1, seed=34, **logit)}
    _run(ctx, twin_ctx, ff.script(specs, [
        ("natgrad", 0, dict(gamma=0.7, fetch=False)), ("predictive", 0, {}),
        ("natgrad", 1, dict(gamma=0.3, fetch=False, num_data=1500.0)), ("predict", 1, {}),
        ("collapsed_q", 2, dict(fetch=False)), ("keep_q", 2, {}), ("grad", 2, {}),
        ("natgrad", 3, dict(gamma=0.7)), ("keep_q", 3, {}), ("marginals", 3, {})]))


def test_predictive_rule_cache_and_buffers(ctx, twin_ctx):
    """(d) ctx->pred_gh is keyed by its order and a closed-form call leaves it in place: GH-20, closed form, GH-7, GH-20 across models;
    the array form with 3, 3000 and 3 points (pred_in / pred_out grow and are reused)."""
    specs = {0: ff.spec_of(100, 3000, 2, seed=41, lik=o.LIK_BERNOULLI_LOGISTIC, quadrature_n=20),
             1: ff.spec_of(64, 500, 3, seed=42, lik=o.LIK_BERNOULLI_NORMCDF), 2: ff.spec_of(129, 500, 8, seed=43, quadrature_n=7)}
    _run(ctx, twin_ctx, ff.script(specs, [
        ("predictive", 0, dict(off=100, nb=500)), ("predictive", 1, {}), ("predictive", 2, {}), ("predictive", 0, dict(off=100, nb=500)),
        ("lik_predictive", 0, dict(n=3)), ("lik_predictive", 0, {}), ("lik_predictive", 0, dict(n=3))]))


def test_moment_buffer_growth_and_shared_offset_staging(ctx, twin_ctx):
    """(e) mom_var() is mom + mom.cap / 16: marginals on 33 points, predictive on 3000, predictive on 33 with offsets; then an fp32 model
    stages offsets for 1025 points in the buffer the fp64 model used, and the fp64 model again."""
    specs = {0: ff.spec_of(128, 3000, 3, seed=51, lik=o.LIK_POISSON_EXP), 1: ff.spec_of(129, 1025, 8, seed=52, f32=True)}
    _run(ctx, twin_ctx, ff.script(specs, [
        ("marginals", 0, dict(off=7, nb=33)), ("predictive", 0, {}), ("predictive", 0, dict(off=7, nb=33, offsets=True)),
        ("mean", 1, dict(variant="grad")), ("mean", 0, dict(variant="grad", off=7, nb=500)), ("mean", 1, dict(variant="marginals")),
        ("mean", 0, dict(variant="elbo"))]))


def test_z_gradient_of_many_inducing_points_on_a_line_behind_a_full_step_on_one_point(ctx, twin_ctx):
    """Found by the long run (profiles/fuzz_families/summary.md, op 3092): 256 inducing points in one dimension, ONE data point, a
    natgrad_ext step, marginals, a full unfetched natgrad step, then svgp_elbo_grad.  The z gradient there is a residue of 1e-8 of
    cancelling terms; device and oracle differ by 1.6e-5 of it and the oracle itself moves by 1e-4 of it under one-ulp inputs, so the
    block is held to its condition (Executor._settle), the value, the q and every other block to the plain fp64 tolerances, and all
    of it bitwise to the fresh context."""
    specs = {0: ff.spec_of(256, 1, 1, lik=o.LIK_BERNOULLI_NORMCDF, quadrature_n=7, seed=863933224)}
    _run(ctx, twin_ctx, ff.script(specs, [
        ("natgrad_ext", 0, dict(gamma=0.3, want_grads=True)), ("marginals", 0, dict(num_data=3.0)),
        ("natgrad", 0, dict(gamma=1.0, num_data=3.0, want_grads=True, fetch=False)), ("grad", 0, {})]))


def test_q_gradient_read_later_while_the_optimal_q_is_still_in_place(ctx, twin_ctx):
    """Found by the long run: the m / Lq gradient blocks vanish not only directly behind svgp_collapsed_q or a full natural-gradient
    step but for as long as that q stays on the model - here with marginals / predict in between, on one inducing point and one data
    point and on 200 inducing points on a line.  They are measured against the KL term's gradient (Executor._settle)."""
    specs = {0: ff.spec_of(1, 1, 1, seed=61, centered=True, family=o.KERNEL_MATERN52), 1: ff.spec_of(200, 127, 1, seed=62, family=o.KERNEL_MATERN52),
             2: ff.spec_of(1, 1, 33, seed=63, z_rows=True)}
    _run(ctx, twin_ctx, ff.script(specs, [
        ("natgrad", 0, dict(gamma=1.0)), ("marginals", 0, {}), ("grad", 0, {}), ("grad_inputs", 0, {}),
        ("collapsed_q", 1, {}), ("predict", 1, {}), ("ext", 1, {}),
        ("collapsed_q", 2, dict(fetch=False)), ("elbo", 2, {}), ("grad", 2, {}), ("grad_inputs", 2, {})]))


def test_fp32_gradients_on_windows_of_one_or_two_points(ctx, twin_ctx):
    """Found by the long run: fp32 models, windows of one or two points, the inv_lengthscale and z gradients of svgp_elbo_grad, its shard
    form, natgrad_ext and svgp_collapsed_grad off by up to 5.6e-2 where the bounds are 2e-2 and below (256 inducing points in two
    dimensions at jitter 1e-2, one data point; a window of two points of 500; of one point of 33).  Replayed on the host, fp32 rounding
    of the kernel parameters and of the jitter moves the float64 oracle's block by 4e-4 only; rounding the ENTRIES of Kuu and Kuf by one
    ulp moves it by 3.1e-11, a condition of 1.4e5 - 6.7e-2 at 4 kappa u for fp32.  Executor._settle probes those entries, and the
    blocks are held to that."""
    f32 = dict(f32=True)
    specs = {0: ff.spec_of(256, 1, 2, seed=1057369858, centered=True, family=o.KERNEL_MATERN52, z_rows=True, **f32),
             1: ff.spec_of(64, 500, 1, seed=1026526221, quadrature_n=20, **f32),
             2: ff.spec_of(300, 1, 2, seed=518604996, centered=True, family=o.KERNEL_MATERN52, quadrature_n=20, z_rows=True, x_rows=True, **f32),
             3: ff.spec_of(17, 33, 8, seed=743169158, family=o.KERNEL_MATERN32, x_rows=True, **f32)}
    _run(ctx, twin_ctx, ff.script(specs, [
        ("update", 0, {}), ("collapsed_grad", 0, {}), ("natgrad_ext", 0, dict(gamma=0.7, want_grads=True)), ("grad", 0, dict(num_data=3.0)),
        ("grad", 0, {}), ("shard", 0, {}), ("collapsed_grad", 0, {}),
        ("collapsed_grad", 1, dict(off=230, nb=2, inputs=True)), ("collapsed_grad", 2, dict(inputs=True)),
        ("collapsed_grad", 3, dict(off=3, nb=1, num_data=99.0, inputs=True))]))
