"""Randomised STATEFUL sweep over the call families that keep or change state on the context or on the model and that
tests/fuzz_stateful.py (round 6) does not know: svgp_natgrad_step / _ext, svgp_collapsed_bound / _q / _grad, svgp_model_update_keep_q,
svgp_predictive / svgp_lik_predictive, the *_with_mean calls, svgp_model_set_mean_z and svgp_elbo_grad_inputs - interleaved with the old
six (elbo, grad, shard, ext, marginals, predict) over several live models of different shapes and dtypes on ONE context.  What it is
after is the ORDER of calls: the collapsed / natgrad workspace cached by Mp alone, chunking drawn from an older call's workspace, the
prep left to whatever reads next after a device-side write of q, the cached predictive rule and buffers, the staging of offsets.

Two halves, so that the first needs no device:
    plan(rng, n_ops, slots=4)          -> the list of op records (dicts): everything random is in there
    execute(ctx, plan, twin_ctx=None)  -> per record, the dict of errors against the float64 restatements (tests/*_ref.py, the oracle)
With ctx = None `execute` runs the reference side alone (the device's outputs replaced by the restatements' own): the slot bookkeeping -
adopting q, mu_z, keep_q, the barred calls - without a GPU.

Adopting the device's q: after natgrad, natgrad_ext, collapsed_q and collapsed_grad the q is fetched, checked against the restatement and
the FETCHED values go into the slot's oracle SVA, so errors do not compound along a sequence.  On one op in four (`fetch` False) the busy
model is left with its unfetched, unprepared q for the next reader; what that q is, is read by repeating the call with its fetch on on
a second model (Executor._read_unfetched_q), so the next reader is checked at the device's own q and at the unchanged bounds.

The twin check: the same op on a context opened for that op alone (fresh_context) and closed after it, on a model and data created for
it from what the slot's device model holds (the last exactly known q, then the unfetched q-writing calls and keep_q updates since,
replayed).  Every array and scalar
the op returns must be BITWISE equal on the two contexts - the library states fixed splits and fixed orders for each of these calls.

    python tests/fuzz_families.py [--seconds 300] [--seed 40] [--slots 4]

A script for the GPU box (exit code 1 when a result is outside its tolerance) and the module behind tests/test_gpu_fuzz_families.py /
tests/test_fuzz_families_cpu.py."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("oracle", "approximategps.jl_amd", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))

import svgp_oracle as o  # noqa: E402
from approxgp import _ffi  # noqa: E402
from fuzz_stateful import FAMS, Slot, block_err, check_grads  # noqa: E402
from helpers import rel  # noqa: E402

import collapsed_ref as cr  # noqa: E402
import input_grad_ref  # noqa: E402
import natgrad_ref as nr  # noqa: E402
import predictive_ref as pr  # noqa: E402
import prior_mean_ref as pmr  # noqa: E402

MS = [1, 17, 64, 100, 128, 129, 200, 256, 300]
NS = [1, 33, 127, 500, 1025, 3000]
DS = [1, 2, 3, 8, 17, 33]
LIKS = [o.LIK_GAUSSIAN, o.LIK_GAUSSIAN, o.LIK_BERNOULLI_LOGISTIC, o.LIK_BERNOULLI_NORMCDF, o.LIK_POISSON_EXP]
QNS = [0, 7, 20]
GAMMAS = [1.0, 0.7, 0.3]

OLD_OPS = ["elbo", "grad", "shard", "ext", "marginals", "predict"]
NEW_OPS = ["natgrad", "natgrad_ext", "collapsed_bound", "collapsed_q", "collapsed_grad", "keep_q", "predictive", "lik_predictive", "mean",
           "mean_z", "grad_inputs"]
Q_WRITERS = ("natgrad", "natgrad_ext", "collapsed_q", "collapsed_grad")
# the classes of the op that follows a q-writing op on the same slot (tests/test_fuzz_families_cpu.py asks for every pair)
FOLLOWERS = ("elbo", "grad", "predictive", "predict", "marginals", "keep_q", "natgrad", "collapsed")
WEIGHTS = {"elbo": 1.0, "grad": 1.5, "shard": 0.7, "ext": 0.7, "marginals": 1.0, "predict": 1.0, "natgrad": 3.0, "natgrad_ext": 1.5,
           "collapsed_bound": 1.5, "collapsed_q": 2.0, "collapsed_grad": 2.0, "keep_q": 1.5, "predictive": 2.0, "lik_predictive": 1.2,
           "mean": 1.5, "mean_z": 1.5, "grad_inputs": 1.2}

# fp32 against the float64 restatements on fp32-rounded inputs.  FAMILY_F32: the bound each family's own test file asserts (4 x its
# F32_MEASURED, or its TOL32 / TOL table).  F32_MEASURED: the worst value of the long run (profiles/fuzz_families/summary.md: 300 s on an
# MI355X, seed 40, 16 153 operations; its table holds every number here) per (new op, output), asserted at 4 x (the project's convention
# for box-to-box reduction order) - for every output that exceeded its family's bound there WITHOUT a difference between the busy and
# the fresh context, and for every output that no family file bounds.  Blocks enter as Executor._settle leaves them (an ill-conditioned
# slot is held to its condition, not to these numbers); a value measured below one fp32 ulp is entered as 1.2e-7.
FAMILY_F32 = {
    ("natgrad", "S_q"): 4 * 1.24e-4, ("natgrad", "elbo_q"): 4 * 1.82e-5,
    ("collapsed", "bound"): 4 * 7.4e-6, ("collapsed", "variance"): 4 * 2.1e-4, ("collapsed", "lik_sigma2"): 4 * 5.7e-5,
    ("collapsed", "mean_const"): 4 * 6.3e-4, ("collapsed", "inv_lengthscale"): 4 * 1.0e-5, ("collapsed", "z"): 4 * 1.1e-3,
    ("collapsed", "x"): 5e-4, ("collapsed", "S_q"): 4 * 1.24e-4, ("collapsed", "elbo_q"): 4 * 1.82e-5,
    ("predictive", "lpd"): 4 * 8.48e-6, ("predictive", "ymean"): 4 * 3.01e-5, ("predictive", "yvar"): 4 * 1.42e-5,
    ("predictive", "sum_lpd"): 4 * 3.48e-7,
    ("mean", "value"): 1e-5, ("mean", "mean"): 1e-4, ("mean", "var"): 1e-5, ("mean", "m"): 1e-4, ("mean", "Lq"): 1e-4, ("mean", "mean_x"): 5e-5,
    ("mean", "z"): 5e-4, ("mean", "inv_lengthscale"): 2e-3, ("mean", "variance"): 1e-3,
    ("grad_inputs", "x"): 5e-4,
}
F32_MEASURED = {
    ("collapsed_bound", "fit"): 8.99e-07, ("collapsed_bound", "logdet_B"): 4.45e-06, ("collapsed_bound", "trace"): 8.61e-07,
    ("collapsed_grad", "S_q"): 5.54e-04, ("collapsed_grad", "lik_sigma2"): 3.24e-04, ("grad_inputs", "Lq"): 9.84e-03,
    ("grad_inputs", "inv_lengthscale"): 1.12e-02, ("grad_inputs", "m"): 5.05e-03, ("grad_inputs", "value"): 7.84e-06,
    ("grad_inputs", "variance"): 8.54e-03, ("grad_inputs", "z"): 5.63e-03, ("keep_q", "probe"): 1.00e-05, ("mean", "value"): 1.03e-05,
    ("mean", "var"): 2.36e-04, ("mean_z", "elbo_after"): 1.60e-05, ("natgrad", "Lq"): 5.24e-03, ("natgrad", "S_q"): 5.81e-04,
    ("natgrad", "inv_lengthscale"): 6.88e-03, ("natgrad", "m"): 2.04e-02, ("natgrad", "value"): 2.26e-05,
    ("natgrad", "variance"): 4.40e-03, ("natgrad", "z"): 1.06e-02, ("natgrad_ext", "Lq"): 8.87e-03,
    ("natgrad_ext", "inv_lengthscale"): 4.07e-02, ("natgrad_ext", "m"): 1.57e-02, ("natgrad_ext", "value"): 2.34e-05,
    ("natgrad_ext", "variance"): 2.01e-03, ("natgrad_ext", "z"): 1.61e-02, ("predictive", "lpd"): 5.72e-05,
    ("predictive", "sum_lpd"): 4.09e-05, ("predictive", "sum_sq_err"): 4.50e-05, ("predictive", "ymean"): 1.62e-04,
    ("predictive", "yvar"): 1.06e-04,
}
F32_CONTRACT = 1e-4          # scalar values of the new ops (ELBO, bound, sum_lpd) in fp32, whatever was measured
SCALARS_F32 = ("value", "bound", "sum_lpd", "elbo_q", "probe", "elbo_after")
OLD_F32 = {"value": 2e-4, "variance": 0.1}   # tests/test_gpu_fuzz.py's seeded slice of fuzz_stateful; every other block 2e-2
# keys that are values (1e-8 in fp64); the other keys are blocks of gradients / marginals / predictions (1e-6, as fuzz_stateful)
VALUE_KEYS = ("value", "bound", "fit", "trace", "logdet_B", "sum_lpd", "sum_sq_err", "elbo_q", "m_q", "S_q", "probe", "elbo_after", "lpd",
              "ymean", "yvar")
# a result that is bitwise different on the busy and the fresh context by the code's own design: op kind -> (file:line, why); compared at
# 1e-13 relative instead (none so far)
TWIN_DELIBERATE = {}


def family_of(op):
    return "natgrad" if op.startswith("natgrad") else "collapsed" if op.startswith("collapsed") else op


def tolerance(op, key, f64):
    if key == "twin":
        return 0.0
    if key in ("structure", "raised", "n_points", "n_neg_var"):
        return 0.0
    if key.startswith("arr_"):
        return 1e-13                      # svgp_lik_predictive against svgp_predictive (test_gpu_predictive.py), fp64 point stage in both
    if op == "lik_predictive":
        return 1e-8                       # fp64 arrays in, fp64 out, whatever the model's dtype
    if f64:
        return 1e-8 if key in VALUE_KEYS else 1e-6
    if op in OLD_OPS:
        return OLD_F32.get(key, 2e-2)
    fam = family_of(op)
    if (op, key) in F32_MEASURED:
        t = 4.0 * F32_MEASURED[(op, key)]
    elif (fam, key) in FAMILY_F32:
        t = FAMILY_F32[(fam, key)]
    else:                                 # the value and gradient blocks of an evaluation: the old sweep's bounds
        t = OLD_F32.get(key, 2e-2)
    return min(t, F32_CONTRACT) if key in SCALARS_F32 else t


def round_through(a, dtype):
    return np.asarray(a, dtype=dtype).astype(np.float64)


def with_q(sva, m, Lq):
    return o.SVA(sva.kernel, sva.z, np.asarray(m, dtype=np.float64), np.tril(np.asarray(Lq, dtype=np.float64)), jitter=sva.jitter,
                 mean_const=sva.mean_const, centered=sva.centered)


def padded(M):
    return (M + 127) // 128 * 128


class FamSlot(Slot):
    """fuzz_stateful.Slot built from a drawn spec instead of an rng (so that `plan` owns every random number), with the model's
    quadrature order, the prior mean offsets at z, and what the twin needs: the last exactly known q and the calls since."""

    def __init__(self, ctx, spec):
        self.spec = spec
        self.d, self.M, self.N = spec["d"], spec["M"], spec["N"]
        self.family, self.lik, self.qn = spec["family"], spec["lik"], spec["quadrature_n"]
        self.dtype = np.float32 if spec["f32"] else np.float64
        self.x, self.y, self.sva, self.s2 = o.synth_problem(spec["seed"], self.N, self.M, self.d, family=self.family, lik=self.lik, dtype=self.dtype)
        self.sva.mean_const = 0.05
        if spec["centered"]:
            nc = self.sva
            tame = 0.1 if self.lik == o.LIK_POISSON_EXP else 1.0
            self.sva = o.SVA(nc.kernel, nc.z, tame * (nc.m + 0.3), 0.7 * tame * nc.Lq, jitter=1e-4 if self.dtype == np.float64 else 1e-2,
                             mean_const=0.15, centered=True)
        self.sva = with_q(self.sva, round_through(self.sva.m, self.dtype), round_through(self.sva.Lq, self.dtype))
        self.z_rows, self.x_rows = spec["z_rows"], spec["x_rows"]
        self.muz = None
        self.base, self.pending = self.sva, []
        self.ctx = ctx
        self.model = self.data = None
        if ctx is not None:
            self.model, self.data = self.device_pair(ctx, self.sva)

    def desc(self, sva=None):
        s = sva if sva is not None else self.sva
        return _ffi.make_desc(self.dtype, s.kernel.family, s.kernel.variance, s.kernel.inv_lengthscale, s.z.T if self.z_rows else s.z, s.m, s.Lq,
                              s.jitter, parametrization=_ffi.CENTERED if s.centered else _ffi.NONCENTERED, likelihood=self.lik,
                              lik_sigma2=self.s2, quadrature_n=self.qn, mean_const=s.mean_const,
                              layout_z=_ffi.ROWVECS if self.z_rows else _ffi.COLVECS)

    def device_pair(self, ctx, sva):
        model = _ffi.DeviceModel(ctx, *self.desc(sva))
        data = (_ffi.DeviceData(ctx, self.x.T, self.y, self.dtype, layout=_ffi.ROWVECS) if self.x_rows
                else _ffi.DeviceData(ctx, self.x, self.y, self.dtype))
        return model, data

    def tag(self):
        return Slot.tag(self) + f"[gh={self.qn}{' muz' if self.muz is not None else ''}{' pending=%d' % len(self.pending) if self.pending else ''}]"

    def twin_pair(self, twin_ctx):
        """A model and data on the fresh context holding what the busy context's model holds."""
        model, data = self.device_pair(twin_ctx, self.base)
        for replay in self.pending:
            replay(model, data)
        if self.muz is not None:
            model.set_mean_z(self.muz)
        return model, data

    def exact(self, sva):
        """The oracle SVA `sva` is exactly what the device model holds."""
        self.sva = self.base = sva
        self.pending = []

    def moved(self, sva, replay):
        """The device model changed by `replay` (a call whose result was not fetched, or keep_q); `sva` describes it to rounding."""
        self.sva = sva
        if self.pending or replay.inexact:
            self.pending.append(replay)
        else:
            self.base = sva

    def free(self):
        if self.model is not None:
            Slot.free(self)


class Replay:
    """A call that changed the device model and whose result was not fetched: fn(model, data, fetch) repeats it on another model and
    returns (m, Lq) of the q it wrote when fetch is set (None for a call that writes no q)."""

    def __init__(self, fn, inexact):
        self.fn, self.inexact = fn, inexact

    def __call__(self, model, data, fetch=False):
        return self.fn(model, data, fetch)


# ---- the plan: every random number of a run ----------------------------------------------------------------------------------------
def draw_spec(rng):
    d, M, N = int(rng.choice(DS)), int(rng.choice(MS)), int(rng.choice(NS))
    if M >= 200 and N > 1025:
        N = 1025
    spec = dict(d=d, M=M, N=N, family=int(rng.choice(FAMS)), lik=int(rng.choice(LIKS)), quadrature_n=int(rng.choice(QNS)),
                f32=bool(rng.random() < 0.35), seed=int(rng.integers(1, 1 << 30)), centered=bool(rng.random() < 0.25))
    spec["z_rows"] = bool(d > 1 and rng.random() < 0.3)
    spec["x_rows"] = bool(d > 1 and rng.random() < 0.3)
    return spec


def applicable(spec, muz_set):
    gauss = spec["lik"] == o.LIK_GAUSSIAN
    ops = ["elbo", "grad", "ext", "marginals", "predict", "keep_q", "predictive", "lik_predictive", "mean"]
    ops.append("grad_inputs")
    if not muz_set:   # natgrad / collapsed take no offsets at z; the shard form's restatement (the oracle's kl_weight) has none either
        ops += ["shard", "natgrad", "natgrad_ext"] + (["collapsed_bound", "collapsed_q", "collapsed_grad"] if gauss else [])
    if spec["centered"]:
        ops.append("mean_z")
    return ops


def follower_class(kind):
    return "natgrad" if kind.startswith("natgrad") else "collapsed" if kind.startswith("collapsed") else kind


class Planner:
    """Draws op records one at a time.  Shapes, windows, arguments and the order of slots are random; WHICH op comes next is steered so
    that a short plan already covers what the sweep is for: it knows of a slot what decides applicability (likelihood, parametrisation,
    whether mu_z is set), walks the list of pairs (q-writing op, class of the op that follows on the same slot) round robin, starting at
    `pair_offset`, and otherwise prefers the op kinds it has drawn fewer than three times."""

    def __init__(self, rng, slots=4, dtypes="mixed", pair_offset=0):
        self.rng, self.n_slots, self.dtypes = rng, slots, dtypes
        self.slots, self.n, self.counts = [], 0, {}
        todo = [(w, f) for f in FOLLOWERS for w in Q_WRITERS]
        self.todo = todo[pair_offset % len(todo):] + todo[:pair_offset % len(todo)]

    def state(self):
        return [dict(st) for st in self.slots], self.n, dict(self.counts), list(self.todo)

    def restore(self, saved):
        self.slots, self.n, self.counts, self.todo = saved

    def _spec(self):
        spec = draw_spec(self.rng)
        if self.dtypes != "mixed":
            spec["f32"] = self.dtypes == "f32"
        live = [st["spec"] for st in self.slots]
        if sum(sp["lik"] == o.LIK_GAUSSIAN and not sp["centered"] for sp in live) < 1 and len(live) >= 1:
            spec["lik"], spec["centered"] = o.LIK_GAUSSIAN, False        # the collapsed calls need one
        elif sum(sp["centered"] for sp in live) < 1 and len(live) >= 2:
            spec["centered"] = True                                      # svgp_model_set_mean_z needs one
        return spec

    def _window(self, N):
        rng = self.rng
        if rng.random() < 0.5 or N < 4:
            return 0, N
        off = int(rng.integers(0, N // 2))
        return off, int(rng.integers(1, N - off + 1))

    def _aim(self, st, ops, writer=None):
        """The next pair of the walk that this slot can serve (its writer `writer` if given) -> the pair, moved to the end of the walk."""
        classes = {follower_class(a) for a in ops}
        for pair in self.todo:
            if (pair[0] == writer if writer else pair[0] in ops) and pair[1] in classes:
                self.todo.remove(pair)
                self.todo.append(pair)
                return pair
        return None

    def next(self):
        rng = self.rng
        r = rng.random()
        rec = dict(i=self.n)
        self.n += 1
        hot = [i for i, st in enumerate(self.slots) if st["target"]]
        if len(self.slots) < self.n_slots or r < 0.06:
            at = len(self.slots)
            if len(self.slots) >= self.n_slots:
                cold = [i for i in range(len(self.slots)) if i not in hot] or list(range(len(self.slots)))
                at = cold[int(rng.integers(len(cold)))]
            replaced = self.slots[at]["spec"]["M"] if at < len(self.slots) else None
            if at < len(self.slots):
                self.slots[at] = None
                self.slots = [st for st in self.slots if st is not None]
                spec = self._spec()
                self.slots.insert(at, dict(spec=spec, muz=False, target=None))
            else:
                spec = self._spec()
                self.slots.append(dict(spec=spec, muz=False, target=None))
            rec.update(kind="create", slot=at, spec=spec, f32=spec["f32"], Mp=padded(spec["M"]), replaced_Mp=None if replaced is None else padded(replaced))
            return rec
        # mostly the slot of the last q-writing op goes on, so that the lazy prep meets every kind of reader
        k = hot[int(rng.integers(len(hot)))] if hot and rng.random() < 0.85 else int(rng.integers(len(self.slots)))
        if not self.slots[k]["target"]:   # a slot that can serve the op kind drawn least so far, while one is short
            least = min(OLD_OPS + NEW_OPS, key=lambda a: self.counts.get(a, 0))
            able = [i for i, st in enumerate(self.slots) if not st["target"] and least in applicable(st["spec"], st["muz"])]
            if self.counts.get(least, 0) < 3 and able:
                k = able[int(rng.integers(len(able)))]
        st = self.slots[k]
        spec = st["spec"]
        rec.update(slot=k, quadrature_n=spec["quadrature_n"], f32=spec["f32"], Mp=padded(spec["M"]))
        if r < 0.12 and not st["target"]:
            rec.update(kind="update", seed=int(rng.integers(1, 1 << 30)))
            return rec
        ops = applicable(spec, st["muz"])
        steer = rng.random()
        if st["target"]:
            ops = [a for a in ops if follower_class(a) == st["target"]]
        elif steer < 0.5:
            pair = self._aim(st, ops)
            if pair:
                ops = [pair[0]]
        fewest = min(self.counts.get(a, 0) for a in ops)
        if fewest < 3:
            ops = [a for a in ops if self.counts.get(a, 0) == fewest]
        w = np.array([WEIGHTS[a] for a in ops])
        kind = ops[int(rng.choice(len(ops), p=w / w.sum()))]
        self.counts[kind] = self.counts.get(kind, 0) + 1
        st["target"] = None
        off, nb = self._window(spec["N"])
        nd = float(rng.choice([0.0, 3.0 * spec["N"]]))
        rec.update(kind=kind, off=off, nb=nb, num_data=nd, gamma=None, offsets=False, seed=int(rng.integers(1, 1 << 30)))
        if kind in ("natgrad", "natgrad_ext"):
            rec.update(gamma=float(rng.choice(GAMMAS)), want_grads=bool(rng.random() < 0.5), fetch=bool(rng.random() >= 0.25))
        elif kind in ("collapsed_q", "collapsed_grad"):
            rec.update(fetch=bool(rng.random() >= 0.25), inputs=bool(rng.random() < 0.5))
        elif kind == "keep_q":
            rec.update(probe=bool(rng.random() < 0.5))
        elif kind == "predictive":
            want = [w_ for w_ in _ffi.PRED_WANTS if rng.random() < 0.5] or [str(rng.choice(_ffi.PRED_WANTS))]
            rec.update(offsets=bool(rng.random() < 1.0 / 3.0), want=want)
        elif kind == "lik_predictive":
            rec.update(n=int(rng.choice([3, nb])))
        elif kind == "mean":
            rec.update(offsets=True, variant=str(rng.choice(["elbo", "marginals", "grad"])))
        elif kind == "mean_z":
            clear = st["muz"] and rng.random() < 0.6
            barred = None
            if not clear and rng.random() < 0.6:
                barred = str(rng.choice(["natgrad", "collapsed_bound"] if spec["lik"] == o.LIK_GAUSSIAN else ["natgrad"]))
            rec.update(clear=bool(clear), barred=barred, gamma=0.7 if barred == "natgrad" else None)
            st["muz"] = not clear
        if kind in Q_WRITERS:
            pair = self._aim(st, applicable(spec, st["muz"]), writer=kind)
            st["target"] = pair[1] if pair else None
        return rec


class Plan(list):
    redrawn = 0


def plan(rng, n_ops, slots=4, dtypes="mixed", simulate=False, pair_offset=0):
    """-> Plan (a list of op records; .redrawn: how many draws the reference could not evaluate).  simulate=True walks the records
    through the reference side as they are drawn (execute's device calls replaced by the restatements' outputs) and redraws an op whose
    restatement is not finite; fewer than 2 % of the ops may need that."""
    planner = Planner(rng, slots, dtypes, pair_offset)
    ex = Executor(None) if simulate else None
    out = Plan()
    while len(out) < n_ops:
        saved = planner.state()
        rec = planner.next()
        if ex is not None:
            try:
                ex.run(rec)
            except ReferenceFailure:
                planner.restore(saved)
                out.redrawn += 1
                continue
        out.append(rec)
    if ex is not None:
        ex.close()
    assert out.redrawn < 0.02 * n_ops, f"{out.redrawn} of {n_ops} ops redrawn: the reference cannot evaluate them"
    return out


def coverage(plans):
    """What a set of plans exercises -> (count per op kind, count per (q-writing op, class of the op that follows it on the same slot),
    number of slot replacements that change Mp between a natgrad op before and a natgrad / collapsed op on the new slot after)."""
    kinds, pairs, mp_changes = {}, {}, 0
    for p in plans:
        last, seen_natgrad, fresh = {}, False, {}
        for rec in p:
            k, sl = rec["kind"], rec["slot"]
            kinds[k] = kinds.get(k, 0) + 1
            if k == "create":
                last.pop(sl, None)
                fresh[sl] = seen_natgrad and rec["replaced_Mp"] is not None and rec["replaced_Mp"] != rec["Mp"]
                continue
            if last.get(sl) in Q_WRITERS and follower_class(k) in FOLLOWERS:
                key = (last[sl], follower_class(k))
                pairs[key] = pairs.get(key, 0) + 1
            last[sl] = k
            if follower_class(k) in ("natgrad", "collapsed"):
                seen_natgrad = seen_natgrad or k.startswith("natgrad")
                if fresh.get(sl):
                    mp_changes += 1
                    fresh[sl] = False
    return kinds, pairs, mp_changes


# ---- execution ---------------------------------------------------------------------------------------------------------------------
class ReferenceFailure(Exception):
    pass


def _finite(ref):
    for v in ref.values():
        if isinstance(v, dict):
            if not _finite(v):
                return False
        elif v is not None and not callable(v) and not isinstance(v, (str, o.SVA)) and not np.all(np.isfinite(np.asarray(v, dtype=np.float64))):
            return False
    return True


def _same(a, b):
    """Bitwise equality of two raw results (dicts of scalars / arrays / None) -> the first key that differs, or None."""
    for k in a:
        u, v = a[k], b[k]
        if u is None or v is None:
            if u is not v:
                return k
        elif not np.array_equal(np.asarray(u), np.asarray(v), equal_nan=True):
            return k
    return None


def _close13(a, b):
    for k in a:
        if a[k] is not None and block_err(a[k], b[k]) > 1e-13:
            return k
    return None


def _grads_raw(g, keys=("variance", "inv_lengthscale", "z", "m", "Lq", "lik_sigma2", "mean_const", "x", "mean_x")):
    return {"g_" + k: g[k] for k in keys if k in g}


def _x_canon(s, gx):
    return np.asarray(gx).T if s.x_rows else np.asarray(gx)


def _summary_raw(res):
    out = {k: res[k] for k in ("lpd", "ymean", "yvar") if k in res}
    if "summary" in res:
        su = res["summary"]
        out.update(sum_lpd=su.sum_lpd, sum_sq_err=su.sum_sq_err, n_points=su.n_points, n_neg_var=su.n_neg_var)
    return out


def _pred_errs(raw, ref):
    e = {k: block_err(raw[k], ref[k]) for k in ("lpd", "ymean", "yvar") if k in raw}
    if "sum_lpd" in raw:
        e["sum_lpd"] = rel(raw["sum_lpd"], ref["sum_lpd"])
        e["sum_sq_err"] = abs(raw["sum_sq_err"] - ref["sum_sq_err"]) / max(abs(ref["sum_sq_err"]), 1e-300)
        e["n_points"] = float(raw["n_points"] != ref["n_points"])
        e["n_neg_var"] = float(raw["n_neg_var"] != ref["n_neg_var"])
    return e


def fresh_context(ctx):
    """A context on the busy context's device that has run nothing: what `execute` and `Executor` take as twin_ctx to open one per
    twin op and close it afterwards."""
    return _ffi.Context(ctx.device)


EPS = {np.float64: float(np.finfo(np.float64).eps), np.float32: float(np.finfo(np.float32).eps)}


class Executor:
    """Runs op records over live slots: on `ctx` (None: the reference side alone), with the twin check where asked.  twin_ctx is a
    callable (fresh_context): a NEW context is opened for every twin op and closed after it, so that its workspaces, moment buffers,
    cached rule and staging have seen this one op only.  (A context object is accepted too and then reused; it gathers a history of its
    own, the same ops as the busy one in the same order, and sees model-level state only.)"""

    def __init__(self, ctx, twin_ctx=None):
        self.ctx, self.twin_ctx, self.slots = ctx, twin_ctx, {}

    def close(self):
        for s in self.slots.values():
            s.free()
        self.slots = {}

    # -- the reference of an evaluation under the slot's offsets at z
    @staticmethod
    def _kw(s, nd):
        return dict(lik=s.lik, sigma2=s.s2, num_data=nd if nd else None, quadrature_n=s.qn)

    def _elbo_ref(self, s, sva, xs, ys, nd, mux=None):
        if mux is None and s.muz is None:
            return o.elbo(sva, xs, ys, **self._kw(s, nd))
        return pmr.elbo(sva, xs, ys, mux, s.muz, **self._kw(s, nd))

    def _grad_ref(self, s, xs, ys, nd, mux=None, sva=None):
        sva = s.sva if sva is None else sva
        if mux is None and s.muz is None:
            return o.elbo_grad(sva, xs, ys, **self._kw(s, nd))
        return pmr.elbo_grad(sva, xs, ys, mux, s.muz, **self._kw(s, nd))

    def _settle(self, s, rec, errs, ref, xs, after_write):
        """Re-measures the gradient blocks (and the marginal means / variances of svgp_marginals) that lie outside their tolerance where
        the REFERENCE cannot resolve them; nothing is computed
        for an op whose blocks are all inside.  ref["_blocks"](sva, xs) restates the op's reference blocks for another model / window.

        1. Blocks in q while the model holds the OPTIMAL q of this very window: written by svgp_collapsed_q / _grad or by a full
           (gamma = 1) natural-gradient step under the Gaussian likelihood, no update, keep_q or set_mean_z since.  m_bar and Lq_bar are the data term's gradient MINUS the KL
           term's; right after svgp_collapsed_q or a full natural-gradient step on that window the two cancel to rounding (that is what
           the optimal q means) and the reference block is noise of 1e-16 times its terms.  Such a block is measured relative to the
           larger of itself and the KL term's own gradient: the terms it is the difference of.
        2. Any block, by its condition.  The restatement is evaluated twice more with z, x and every entry of the kernel matrices it
           forms (Kuu symmetrically, Kuf) moved by one unit in the last place of float64 (random signs) - the rounding that any
           implementation commits when it stores those matrices in its working precision; delta is how far the block moves, relative to its largest entry, so kappa = delta / eps64 is the
           block's condition number as the reference sees it.  A computation in working precision u (eps of the model's dtype) does
           not commit ONE rounding per entry: the factorisation of the M x M Kuu alone has a backward error that grows with M - M u in
           the worst case, about sqrt(M) u for rounding errors of random sign (Higham, Accuracy and Stability of Numerical Algorithms,
           Theorem 10.3; Higham and Mary 2019) - so no implementation, the float64 oracle included, resolves such a block below
           sqrt(M) kappa u.  The block is held to max(its tolerance, max(4, sqrt(M)) kappa u), 4 being the project's factor for
           reduction order, and the error is reported scaled by tolerance / that bound.  On a well-conditioned slot kappa u is far
           below every tolerance and nothing changes; on 256 inducing points on a line behind a full step on ONE data point the z
           gradient is a residue of 1e-8 and kappa is 1e12; on 256 points in a plane at the fp32 jitter with one data point the
           inv_lengthscale gradient has kappa 1.4e5 to 3e5 (profiles/fuzz_families/summary.md)."""
        fn = ref.get("_blocks")
        f64 = s.dtype == np.float64
        over = [k for k, v in errs.items() if not v <= tolerance(rec["kind"], k, f64)] if fn is not None else []
        if not over:
            return errs
        with np.errstate(all="ignore"):
            base = fn(s.sva, xs)
        over = [k for k in over if k in base]
        scale = {k: max(float(np.abs(np.asarray(base[k], dtype=np.float64)).max()), 1e-12) for k in over}
        if after_write == (rec["off"], rec["nb"]) and any(k in ("m", "Lq") for k in over):
            x1, y1 = s.x[:, :1], s.y[:1]
            kw = dict(lik=s.lik, sigma2=s.s2, num_data=1e-200, quadrature_n=s.qn)      # scale 1e-200: the KL term alone
            g_kl = (o.elbo_grad(s.sva, x1, y1, **kw) if s.muz is None else pmr.elbo_grad(s.sva, x1, y1, None, s.muz, **kw))[1]
            for k in ("m", "Lq"):
                floor = float(np.abs(g_kl[k]).max())
                if k in over and floor > scale[k]:
                    print(f"SETTLED op {rec['i']} {rec['kind']} {k}: {errs[k]:.2e} of a block that cancels to {scale[k]:.1e}; KL term {floor:.1e}")
                    errs[k] *= scale[k] / floor
        over = [k for k in over if not errs[k] <= tolerance(rec["kind"], k, f64)]
        if over:
            rng = np.random.default_rng(rec["seed"] + 2)
            delta = {k: 0.0 for k in over}
            jig = lambda a: a * (1.0 + EPS[np.float64] * rng.choice([-1.0, 1.0], size=np.shape(a)))  # noqa: E731
            kappa_fn = o._kappa

            def rounded_kernel(kernel, r2):
                K = kappa_fn(kernel, r2)
                S = rng.choice([-1.0, 1.0], size=K.shape)
                if K.ndim == 2 and K.shape[0] == K.shape[1]:
                    S = np.triu(S) + np.triu(S, 1).T
                return K * (1.0 + EPS[np.float64] * S)
            for _ in range(2):
                v = s.sva
                try:
                    o._kappa = rounded_kernel
                    with np.errstate(all="ignore"):
                        moved = fn(o.SVA(v.kernel, jig(v.z), v.m, v.Lq, jitter=v.jitter, mean_const=v.mean_const, centered=v.centered), jig(xs))
                except (o.PosDefException, np.linalg.LinAlgError):
                    continue
                finally:
                    o._kappa = kappa_fn
                for k in over:
                    delta[k] = max(delta[k], float(np.abs(np.asarray(moved[k], dtype=np.float64) - base[k]).max()) / scale[k])
            for k in over:
                tol, bound = tolerance(rec["kind"], k, f64), max(4.0, np.sqrt(s.M)) * delta[k] / EPS[np.float64] * EPS[s.dtype]
                if bound > tol:
                    print(f"SETTLED op {rec['i']} {rec['kind']} {k}: {errs[k]:.2e}; the reference moves by {delta[k]:.1e} under one-ulp "
                          f"inputs, bound {bound:.1e} in place of {tol:.1e}")
                    errs[k] *= tol / bound
        return errs

    def _q_errs(self, s, m, Lq, new, xs, ys, nd, elbo_new):
        """The q check: m (fp64 only), S = Lq Lq' and the oracle's ELBO at the device's q against the restatement's."""
        Lq64 = np.asarray(Lq, dtype=np.float64)
        e = {"structure": float(np.triu(Lq64, 1).any() or not np.all(np.diag(Lq64) > 0)),
             "S_q": block_err(Lq64 @ Lq64.T, new.Lq @ new.Lq.T),
             "elbo_q": rel(self._elbo_ref(s, with_q(s.sva, m, Lq), xs, ys, nd), elbo_new)}
        if s.dtype == np.float64:
            e["m_q"] = block_err(m, new.m)
        return e

    def run(self, rec, twin=False):
        """One record -> (label, dict of errors).  Raises ReferenceFailure when the restatement is not finite (before any state moved)."""
        kind = rec["kind"]
        if kind == "create":
            if rec["slot"] in self.slots:
                self.slots.pop(rec["slot"]).free()
            self.slots[rec["slot"]] = FamSlot(self.ctx, rec["spec"])
            return kind, {}
        s = self.slots[rec["slot"]]
        after_write = getattr(s, "after_write", None)      # the window of the q-writing call whose q the model still holds, or None
        if kind in ("update", "keep_q", "mean_z"):
            s.after_write = None
        if kind == "update":
            self._update(s, rec)
            return kind, {}
        off, nb = rec["off"], rec["nb"]
        xs, ys = s.x[:, off:off + nb], s.y[off:off + nb]
        try:
            with np.errstate(all="ignore"):
                ref, dev, errs_of, adopt = getattr(self, "_op_" + kind)(s, rec, xs, ys)
        except (o.PosDefException, np.linalg.LinAlgError, FloatingPointError) as e:
            raise ReferenceFailure(f"{kind}: {e!r}")
        if not _finite(ref):
            raise ReferenceFailure(f"{kind}: non-finite restatement")
        if self.ctx is None:
            adopt(None)
            if self._writes_optimal_q(s, rec):
                s.after_write = (off, nb)
            return kind, {}
        raw = dev(s.model, s.data, self.ctx)
        errs = self._settle(s, rec, errs_of(raw), ref, xs, after_write)
        if twin and self.twin_ctx is not None:
            fresh = callable(self.twin_ctx)
            tctx = self.twin_ctx(self.ctx) if fresh else self.twin_ctx
            tm = td = None
            try:
                tm, td = s.twin_pair(tctx)
                raw2 = dev(tm, td, tctx)
            finally:
                for h in (tm, td):
                    if h is not None:
                        h.free()
                if fresh:
                    tctx.close()
            diff = _close13(raw, raw2) if kind in TWIN_DELIBERATE else _same(raw, raw2)
            errs["twin"] = 0.0 if diff is None else 1.0
            if diff is not None:
                print(f"TWIN op {rec['i']} {kind} {s.tag()}: '{diff}' differs between the busy and the fresh context by "
                      f"{block_err(raw[diff], raw2[diff]):.2e} (relative to its largest entry)", flush=True)
        adopt(raw)
        if s.pending and s.pending[-1].inexact:
            self._read_unfetched_q(s)
        if self._writes_optimal_q(s, rec):
            s.after_write = (off, nb)
        return kind, errs

    @staticmethod
    def _writes_optimal_q(s, rec):
        """The calls after which d elbo / d q vanishes on their window: svgp_collapsed_q / _grad, and a full natural-gradient step under
        the Gaussian likelihood (which lands on the same q)."""
        kind = rec["kind"]
        return kind in ("collapsed_q", "collapsed_grad") or (kind in ("natgrad", "natgrad_ext") and rec["gamma"] == 1.0
                                                              and s.lik == o.LIK_GAUSSIAN)

    def _read_unfetched_q(self, s):
        """The q that an unfetched call left on the busy model, without touching that model: the library's calls are bitwise repeatable
        (the twin check holds them to it), so the same calls on a second model built from the last exactly known q, the last of them
        with its fetch on, return exactly that q.  It goes into the slot's oracle; the busy model keeps its unprepared q for the next
        reader, whose reference is then the ELBO / marginals / gradient at the device's own q, at the unchanged bounds."""
        model = _ffi.DeviceModel(self.ctx, *s.desc(s.base))
        try:
            q = None
            for n, replay in enumerate(s.pending):
                got = replay(model, s.data, n == len(s.pending) - 1)
                q = got if got is not None else q
        finally:
            model.free()
        s.exact(with_q(s.sva, *q))

    # -- state changes that return nothing
    def _update(self, s, rec):
        """New parameter values of the same shape, q included (fuzz_stateful.Slot.update with the record's own rng)."""
        rng = np.random.default_rng(rec["seed"])
        k, v = s.sva.kernel, s.sva
        f = lambda a, e: round_through(a * (1.0 + e * rng.standard_normal(np.shape(a))), s.dtype)  # noqa: E731
        kern = o.Kernel(k.family, float(k.variance * (1.0 + 0.1 * rng.random())), f(k.inv_lengthscale, 0.05))
        Lq = np.tril(f(v.Lq, 0.02))
        np.fill_diagonal(Lq, np.abs(np.diag(Lq)) + 1e-3)
        Lq = round_through(Lq, s.dtype)
        z = round_through(v.z + 0.01 * rng.standard_normal(v.z.shape), s.dtype)
        m = round_through(f(v.m, 0.05) + 0.01, s.dtype)
        s.exact(o.SVA(kern, z, m, Lq, jitter=v.jitter, mean_const=float(v.mean_const + 0.01), centered=v.centered))
        if s.model is not None:
            s.model.update(*s.desc())

    @staticmethod
    def _new_hypers(s, rec):
        rng = np.random.default_rng(rec["seed"])
        k, v = s.sva.kernel, s.sva
        kern = o.Kernel(k.family, float(k.variance * (1.0 + 0.1 * rng.random())), k.inv_lengthscale * (1.0 + 0.05 * rng.standard_normal(k.inv_lengthscale.shape)))
        z = round_through(v.z + 0.01 * rng.standard_normal(v.z.shape), s.dtype)
        return o.SVA(kern, z, v.m, v.Lq, jitter=v.jitter, mean_const=float(v.mean_const + 0.01), centered=v.centered)

    def _mux(self, s, rec, off, nb):
        rng = np.random.default_rng(rec["seed"] + 1)
        return round_through(0.3 * np.sin(1.3 * s.x[0, off:off + nb]) + 0.05 * rng.standard_normal(nb), s.dtype)

    # -- the old six (fuzz_stateful.step restated as reference / device halves; they know of mu_z and of the quadrature order)
    def _op_elbo(self, s, rec, xs, ys):
        off, nb, nd = rec["off"], rec["nb"], rec["num_data"]
        ref = {"value": self._elbo_ref(s, s.sva, xs, ys, nd)}
        dev = lambda model, data, ctx: {"value": model.elbo(data, off, nb, nd)[0]}  # noqa: E731
        return ref, dev, lambda raw: {"value": rel(raw["value"], ref["value"])}, lambda raw: None

    def _grad_like(self, s, rec, xs, ys, call, v_ref, g_ref, extra=lambda raw: {}, blocks=None):
        def dev(model, data, ctx):
            v, _, g = call(model, data, ctx)
            return {"value": v, **_grads_raw(g)}

        def errs_of(raw):
            g = {k[2:]: v for k, v in raw.items() if k.startswith("g_")}
            return {"value": rel(raw["value"], v_ref), **check_grads(s, g, g_ref), **extra(raw)}
        return {"value": v_ref, "g": g_ref, "_blocks": blocks}, dev, errs_of, lambda raw: None

    def _op_grad(self, s, rec, xs, ys):
        off, nb, nd = rec["off"], rec["nb"], rec["num_data"]
        v_ref, g_ref = self._grad_ref(s, xs, ys, nd)
        return self._grad_like(s, rec, xs, ys, lambda model, data, ctx: model.elbo_grad(data, off, nb, nd, z_shape=s.zshape()), v_ref, g_ref,
                               blocks=lambda sva, x: self._grad_ref(s, x, ys, nd, sva=sva)[1])

    def _op_shard(self, s, rec, xs, ys):
        off, nb = rec["off"], rec["nb"]
        scale, klw = 1.7, 0.25
        ref_at = lambda sva, x: o.elbo_grad(sva, x, ys, lik=s.lik, sigma2=s.s2, num_data=scale * nb, kl_weight=klw, quadrature_n=s.qn)  # noqa: E731
        v_ref, g_ref = ref_at(s.sva, xs)
        return self._grad_like(s, rec, xs, ys, lambda model, data, ctx: model.elbo_grad(data, off, nb, shard=(scale, klw), z_shape=s.zshape()),
                               v_ref, g_ref, blocks=lambda sva, x: ref_at(sva, x)[1])

    def _host_lik(self, s, model, data, off, nb, ys):
        mu, var = model.marginals(data, off, nb)
        gmu, gv, _ = o.expected_loglik_grads(s.lik, mu, var, ys, s.s2, s.qn)
        return o.expected_loglik(s.lik, mu, np.sqrt(var), ys, s.s2, s.qn), gmu, gv

    def _op_ext(self, s, rec, xs, ys):
        off, nb, nd = rec["off"], rec["nb"], rec["num_data"]
        v_ref, g_ref = self._grad_ref(s, xs, ys, nd)

        def call(model, data, ctx):
            return model.elbo_grad(data, off, nb, nd, ext=self._host_lik(s, model, data, off, nb, ys), z_shape=s.zshape())
        return self._grad_like(s, rec, xs, ys, call, v_ref, g_ref, blocks=lambda sva, x: self._grad_ref(s, x, ys, nd, sva=sva)[1])

    def _marg_ref(self, s, sva, x, mux=None):
        if mux is None and s.muz is None:
            mr, vr = o.mean_and_var(o.posterior(sva), x)
            return mr, vr + 1e-18
        return pmr.marginals(sva, x, mux, s.muz)

    def _op_marginals(self, s, rec, xs, ys):
        off, nb = rec["off"], rec["nb"]
        mr, vr = self._marg_ref(s, s.sva, xs)
        ref = {"mean": mr, "var": vr, "_blocks": lambda sva, x: dict(zip(("mean", "var"), self._marg_ref(s, sva, x)))}
        dev = lambda model, data, ctx: dict(zip(("mean", "var"), model.marginals(data, off, nb)))  # noqa: E731
        return ref, dev, lambda raw: {k: block_err(raw[k], ref[k]) for k in ("mean", "var")}, lambda raw: None

    def _op_predict(self, s, rec, xs, ys):
        xp = xs[:, :min(rec["nb"], 80)]
        mr, vr = self._marg_ref(s, s.sva, xp)
        ref = {"mean": mr, "var": vr - 1e-18, "cov": o.cov(o.posterior(s.sva), xp)}
        dev = lambda model, data, ctx: dict(zip(("mean", "var", "cov"), model.predict(xp, True, True, True)))  # noqa: E731
        return ref, dev, lambda raw: {k: block_err(raw[k], ref[k]) for k in ref}, lambda raw: None

    # -- natural-gradient steps
    def _op_natgrad(self, s, rec, xs, ys, ext=False):
        off, nb, nd, gamma, fetch, want = rec["off"], rec["nb"], rec["num_data"], rec["gamma"], rec["fetch"], rec["want_grads"]
        new = nr.step(s.sva, xs, ys, lik=s.lik, sigma2=s.s2, num_data=nd if nd else None, gamma=gamma, quadrature_n=s.qn)
        v_ref, g_ref = self._grad_ref(s, xs, ys, nd)
        elbo_new = self._elbo_ref(s, new, xs, ys, nd)
        ref = {"value": v_ref, "g": g_ref, "m": new.m, "Lq": new.Lq, "elbo_new": elbo_new,
               "_blocks": lambda sva, x: self._grad_ref(s, x, ys, nd, sva=sva)[1]}

        def step(model, data, ctx, fetch=fetch):
            e = self._host_lik(s, model, data, off, nb, ys) if ext else None
            return model.natgrad_step(data, off, nb, nd, gamma=gamma, ext=e, want_grads=want, fetch=fetch, z_shape=s.zshape())

        def dev(model, data, ctx):
            v, _, g, m, Lq = step(model, data, ctx)
            return {"value": v, "m": m, "Lq": Lq, **(_grads_raw(g) if g is not None else {})}

        def errs_of(raw):
            e = {"value": rel(raw["value"], v_ref)}
            if want:
                e.update(check_grads(s, {k[2:]: v for k, v in raw.items() if k.startswith("g_")}, g_ref))
            if fetch:
                e.update(self._q_errs(s, raw["m"], raw["Lq"], new, xs, ys, nd, elbo_new))
            return e

        def adopt(raw):
            if raw is not None and fetch:
                s.exact(with_q(s.sva, raw["m"], raw["Lq"]))
            else:
                s.moved(new, Replay(lambda model, data, f: step(model, data, None, fetch=f)[3:], True))
        return ref, dev, errs_of, adopt

    def _op_natgrad_ext(self, s, rec, xs, ys):
        return self._op_natgrad(s, rec, xs, ys, ext=True)

    # -- the collapsed bound and the optimal q
    def _collapsed_ref(self, s, xs, ys):
        v = s.sva
        return cr.optimal_sva(v.kernel, v.z, v.jitter, xs, s.s2, ys, mean_const=v.mean_const, centered=v.centered)

    def _op_collapsed_bound(self, s, rec, xs, ys):
        off, nb = rec["off"], rec["nb"]
        _, r = self._collapsed_ref(s, xs, ys)
        ref = {"bound": r.bound, "fit": r.fit, "trace": r.trace, "logdet_B": r.logdet_B}

        def dev(model, data, ctx):
            v, t = model.collapsed_bound(data, off, nb)
            return {"bound": v, "fit": t.fit, "trace": t.trace, "logdet_B": t.logdet_B, "t_bound": t.bound, "n_points": t.n_points}

        def errs_of(raw):
            return {"bound": rel(raw["bound"], r.bound), "fit": rel(raw["fit"], r.fit), "trace": abs(raw["trace"] - r.trace) / abs(r.bound),
                    "logdet_B": abs(raw["logdet_B"] - r.logdet_B) / max(abs(r.logdet_B), 1e-8 * abs(r.bound), 1e-300),
                    "structure": float(raw["t_bound"] != raw["bound"] or raw["n_points"] != nb)}
        return ref, dev, errs_of, lambda raw: None

    def _op_collapsed_q(self, s, rec, xs, ys):
        off, nb, fetch = rec["off"], rec["nb"], rec["fetch"]
        new, r = self._collapsed_ref(s, xs, ys)
        elbo_new = o.elbo(new, xs, ys, lik=s.lik, sigma2=s.s2, quadrature_n=s.qn)
        ref = {"bound": r.bound, "m": new.m, "Lq": new.Lq, "elbo_new": elbo_new}

        def dev(model, data, ctx):
            v, m, Lq = model.collapsed_q(data, off, nb, fetch=fetch)
            return {"bound": v, "m": m, "Lq": Lq}

        def errs_of(raw):
            e = {"bound": rel(raw["bound"], r.bound)}
            if fetch:
                e.update(self._q_errs(s, raw["m"], raw["Lq"], new, xs, ys, 0.0, elbo_new))
            return e

        def adopt(raw):
            if raw is not None and fetch:
                s.exact(with_q(s.sva, raw["m"], raw["Lq"]))
            else:
                s.moved(new, Replay(lambda model, data, f: model.collapsed_q(data, off, nb, fetch=f)[1:], True))
        return ref, dev, errs_of, adopt

    def _op_collapsed_grad(self, s, rec, xs, ys):
        """svgp_collapsed_grad returns no q: with `fetch` a svgp_collapsed_q on the same window follows (it rewrites the same q - bitwise,
        the bound included - and fetches it); without, the restatement's q is adopted and the next reader preps."""
        off, nb, fetch, inputs = rec["off"], rec["nb"], rec["fetch"], rec["inputs"]
        new, r = self._collapsed_ref(s, xs, ys)
        g_ref = o.elbo_grad(new, xs, ys, lik=o.LIK_GAUSSIAN, sigma2=s.s2)[1]
        x_ref = input_grad_ref.input_grad(new, xs, ys, sigma2=s.s2) if inputs else None
        elbo_new = o.elbo(new, xs, ys, lik=s.lik, sigma2=s.s2, quadrature_n=s.qn)
        ref = {"bound": r.bound, "g": {k: g_ref[k] for k in ("variance", "inv_lengthscale", "z", "lik_sigma2", "mean_const")}, "x": x_ref,
               "m": new.m, "Lq": new.Lq}

        def blocks(sva, x):
            opt = cr.optimal_sva(sva.kernel, sva.z, sva.jitter, x, s.s2, ys, mean_const=sva.mean_const, centered=sva.centered)[0]
            g = dict(o.elbo_grad(opt, x, ys, lik=o.LIK_GAUSSIAN, sigma2=s.s2)[1])
            if inputs:
                g["x"] = input_grad_ref.input_grad(opt, x, ys, sigma2=s.s2)
            return g
        ref["_blocks"] = blocks

        def dev(model, data, ctx):
            v, t, g = model.collapsed_grad(data, off, nb, z_shape=s.zshape(), inputs=True if inputs else None)
            raw = {"bound": v, "t_bound": t.bound, **_grads_raw(g)}
            if fetch:
                raw["bound_q"], raw["m"], raw["Lq"] = model.collapsed_q(data, off, nb)
            return raw

        def errs_of(raw):
            g = {k[2:]: v for k, v in raw.items() if k.startswith("g_")}
            g.update(m=np.zeros(s.M), Lq=np.zeros((s.M, s.M)))
            cg = check_grads(s, g, {**g_ref, "m": np.zeros(s.M), "Lq": np.zeros((s.M, s.M))})
            e = {"bound": rel(raw["bound"], r.bound), **{k: cg[k] for k in ("z", "inv_lengthscale", "variance")},
                 "lik_sigma2": block_err([g["lik_sigma2"]], [g_ref["lik_sigma2"]]), "mean_const": block_err([g["mean_const"]], [g_ref["mean_const"]]),
                 "structure": float(raw["t_bound"] != raw["bound"])}
            if inputs:
                e["x"] = block_err(_x_canon(s, g["x"]), x_ref)
            if fetch:
                e.update(self._q_errs(s, raw["m"], raw["Lq"], new, xs, ys, 0.0, elbo_new))
                e["structure"] = max(e["structure"], float(raw["bound_q"] != raw["bound"]))
            return e

        def adopt(raw):
            if raw is not None and fetch:
                s.exact(with_q(s.sva, raw["m"], raw["Lq"]))
            else:
                def again(model, data, f):
                    model.collapsed_grad(data, off, nb, z_shape=s.zshape())
                    return model.collapsed_q(data, off, nb)[1:] if f else None
                s.moved(new, Replay(again, True))
        return ref, dev, errs_of, adopt

    # -- new hyperparameters under the device-resident q
    def _op_keep_q(self, s, rec, xs, ys):
        off, nb, nd, probe = rec["off"], rec["nb"], rec["num_data"], rec["probe"]
        new = self._new_hypers(s, rec)
        ref = {"probe": self._elbo_ref(s, new, xs, ys, nd)}

        def upload(model, data, fetch=False):
            desc, keep = s.desc(new)
            desc.m, desc.Lq = None, None
            model.update_keep_q(desc, keep)

        def dev(model, data, ctx):
            upload(model, data)
            return {"probe": model.elbo(data, off, nb, nd)[0]} if probe else {}
        return ref, dev, lambda raw: ({"probe": rel(raw["probe"], ref["probe"])} if probe else {}), lambda raw: s.moved(new, Replay(upload, False))

    # -- the predictive distribution of the observation
    def _op_predictive(self, s, rec, xs, ys):
        off, nb, want = rec["off"], rec["nb"], tuple(rec["want"])
        mux = self._mux(s, rec, off, nb) if rec["offsets"] else None
        ref = pr.from_marginals(s.lik, *self._marg_ref(s, s.sva, xs, mux), ys, s.s2, s.qn)
        dev = lambda model, data, ctx: _summary_raw(model.predictive(data, off, nb, prior_mean=mux, want=want))  # noqa: E731
        return ref, dev, lambda raw: _pred_errs(raw, ref), lambda raw: None

    def _op_lik_predictive(self, s, rec, xs, ys):
        """svgp_lik_predictive on svgp_marginals' output, on n of the window's points: against predictive_ref.from_marginals at those
        marginals, and (arr_*) against svgp_predictive on the same points at 1e-13."""
        off, nb = rec["off"], rec["nb"]
        n = min(rec["n"], nb)
        mr, vr = self._marg_ref(s, s.sva, xs[:, :n])
        ref = pr.from_marginals(s.lik, mr, vr, ys[:n], s.s2, s.qn)

        def dev(model, data, ctx):
            mu, var = model.marginals(data, off, nb)
            arr = _summary_raw(_ffi.lik_predictive(ctx, s.lik, s.s2, s.qn, mu[:n], var[:n], ys[:n]))
            whole = model.predictive(data, off, n, want=("lpd", "ymean", "yvar"))
            return {**arr, "mu": mu, "var": var, **{"p_" + k: whole[k] for k in whole}}

        def errs_of(raw):
            at = pr.from_marginals(s.lik, raw["mu"][:n], raw["var"][:n], ys[:n], s.s2, s.qn)
            e = _pred_errs({k: raw[k] for k in raw if k not in ("mu", "var") and not k.startswith("p_")}, at)
            e.update({"arr_" + k: block_err(raw[k], raw["p_" + k]) for k in ("lpd", "ymean", "yvar")})
            return e
        return ref, dev, errs_of, lambda raw: None

    # -- prior mean offsets
    def _op_mean(self, s, rec, xs, ys):
        off, nb, nd, variant = rec["off"], rec["nb"], rec["num_data"], rec["variant"]
        mux = self._mux(s, rec, off, nb)
        if variant == "elbo":
            ref = {"value": self._elbo_ref(s, s.sva, xs, ys, nd, mux)}
            dev = lambda model, data, ctx: {"value": model.elbo(data, off, nb, nd, prior_mean=mux)[0]}  # noqa: E731
            return ref, dev, lambda raw: {"value": rel(raw["value"], ref["value"])}, lambda raw: None
        if variant == "marginals":
            ref = dict(zip(("mean", "var"), self._marg_ref(s, s.sva, xs, mux)))
            ref["_blocks"] = lambda sva, x: dict(zip(("mean", "var"), self._marg_ref(s, sva, x, mux)))
            dev = lambda model, data, ctx: dict(zip(("mean", "var"), model.marginals(data, off, nb, prior_mean=mux)))  # noqa: E731
            return ref, dev, lambda raw: {k: block_err(raw[k], ref[k]) for k in ("mean", "var")}, lambda raw: None
        v_ref, g_ref = pmr.elbo_grad(s.sva, xs, ys, mux, s.muz, **self._kw(s, nd))
        return self._grad_like(s, rec, xs, ys,
                               lambda model, data, ctx: model.elbo_grad(data, off, nb, nd, z_shape=s.zshape(), prior_mean=mux, mean_grad=True),
                               v_ref, g_ref, extra=lambda raw: {"mean_x": block_err(raw["g_mean_x"], g_ref["mean_x"])},
                               blocks=lambda sva, x: pmr.elbo_grad(sva, x, ys, mux, s.muz, **self._kw(s, nd))[1])

    def _op_mean_z(self, s, rec, xs, ys):
        """set_mean_z(values) / set_mean_z(None) on a Centered slot; with `barred`, a natgrad / collapsed call that must be refused with
        UnsupportedError; svgp_posterior's three arrays before and after it are bitwise equal (the q is unchanged) and the ELBO afterwards
        is the one of that q under the offsets."""
        off, nb, nd, barred = rec["off"], rec["nb"], rec["num_data"], rec["barred"]
        rng = np.random.default_rng(rec["seed"])
        muz = None if rec["clear"] else round_through(0.2 * rng.standard_normal(s.M), s.dtype)
        old, s.muz = s.muz, muz
        try:
            ref = {"elbo_after": self._elbo_ref(s, s.sva, xs, ys, nd)} if barred else {}
        finally:
            s.muz = old

        def dev(model, data, ctx):
            model.set_mean_z(muz)
            if not barred:
                return {}
            before = model.posterior()          # (Lk, alpha, B): a function of the device-resident q, bit for bit
            try:
                if barred == "natgrad":
                    model.natgrad_step(data, off, nb, nd, gamma=rec["gamma"])
                else:
                    model.collapsed_bound(data, off, nb)
                raised = False
            except _ffi.UnsupportedError:
                raised = True
            same = all(np.array_equal(a, b) for a, b in zip(before, model.posterior()))
            return {"raised": raised, "q_same": same, "elbo_after": model.elbo(data, off, nb, nd)[0]}

        def errs_of(raw):
            return {"raised": float(not raw["raised"]), "structure": float(not raw["q_same"]),
                    "elbo_after": rel(raw["elbo_after"], ref["elbo_after"])} if barred else {}

        def adopt(raw):
            s.muz = muz
        return ref, dev, errs_of, adopt

    def _op_grad_inputs(self, s, rec, xs, ys):
        off, nb, nd = rec["off"], rec["nb"], rec["num_data"]
        v_ref, g_ref = self._grad_ref(s, xs, ys, nd)

        def x_bar(sva, x):
            # offsets at z enter a Centered model through m - mean_const - mu_z alone: the restatement takes them folded into m
            at = sva if s.muz is None else with_q(sva, sva.m - s.muz, sva.Lq)
            return input_grad_ref.input_grad(at, x, ys, lik=s.lik, sigma2=s.s2, num_data=nd if nd else None, quadrature_n=s.qn)
        x_ref = x_bar(s.sva, xs)
        ref, dev, errs_of, adopt = self._grad_like(
            s, rec, xs, ys, lambda model, data, ctx: model.elbo_grad(data, off, nb, nd, z_shape=s.zshape(), inputs=True), v_ref, g_ref,
            extra=lambda raw: {"x": block_err(_x_canon(s, raw["g_x"]), x_ref)},
            blocks=lambda sva, x: {**self._grad_ref(s, x, ys, nd, sva=sva)[1], "x": x_bar(sva, x)})
        return {**ref, "x": x_ref}, dev, errs_of, adopt


def execute(ctx, plan_, twin_ctx=None, twin_every=1, log=None):
    """Runs the records of a plan over live slots on `ctx` -> list of (record, dict of errors), one per record.  twin_ctx: the twin check
    on every twin_every-th op.  ctx = None: the reference side alone (no errors; the bookkeeping)."""
    ex = Executor(ctx, twin_ctx)
    out = []
    try:
        for n, rec in enumerate(plan_):
            kind, errs = ex.run(rec, twin=twin_ctx is not None and n % twin_every == 0)
            out.append((rec, errs))
            if log is not None and kind not in ("create",):
                log(rec, ex.slots[rec["slot"]], errs)
    finally:
        ex.close()
    return out


def failures(results):
    """-> [(op index, kind, key, error, tolerance)] of what lies outside its tolerance."""
    bad = []
    for rec, errs in results:
        f64 = not rec["f32"]
        for k, v in errs.items():
            t = tolerance(rec["kind"], k, f64)
            if not v <= t:
                bad.append((rec["i"], rec["kind"], k, v, t))
    return bad


def worst(results, into=None):
    """-> {(kind, key, dtype): the largest error} over the results of `execute`."""
    into = {} if into is None else into
    for rec, errs in results:
        for k, v in errs.items():
            key = (rec["kind"], k, "f32" if rec["f32"] else "f64")
            into[key] = max(into.get(key, 0.0), v)
    return into


# the seeded slices of tests/test_gpu_fuzz_families.py: name -> (seed, dtypes, where its walk over the (writer, follower) pairs starts);
# tests/test_fuzz_families_cpu.py asserts what they cover
SLICE_OPS = 500
SLICES = {"f64": (900, "f64", 0), "f32": (910, "f32", 11), "mixed": (920, "mixed", 22)}


def slice_plan(name, simulate=False):
    seed, dtypes, pair_offset = SLICES[name]
    return plan(np.random.default_rng(seed), SLICE_OPS, 4, dtypes, simulate, pair_offset)


# ---- hand-written sequences ----------------------------------------------------------------------------------------------------------
def spec_of(M, N, d, lik=o.LIK_GAUSSIAN, f32=False, centered=False, quadrature_n=0, family=o.KERNEL_SE, seed=7, z_rows=False, x_rows=False):
    return dict(d=d, M=M, N=N, family=family, lik=lik, quadrature_n=quadrature_n, f32=f32, seed=seed, centered=centered, z_rows=z_rows,
                x_rows=x_rows)


DEFAULTS = {"natgrad": dict(gamma=1.0, want_grads=False, fetch=True), "natgrad_ext": dict(gamma=1.0, want_grads=False, fetch=True),
            "collapsed_q": dict(fetch=True, inputs=False), "collapsed_grad": dict(fetch=True, inputs=False), "keep_q": dict(probe=False),
            "predictive": dict(want=list(_ffi.PRED_WANTS)), "mean": dict(offsets=True, variant="elbo"), "mean_z": dict(clear=False, barred=None)}


def script(specs, steps):
    """specs: {slot: spec}; steps: [(kind, slot, {overrides})] -> a plan: the slots created first, then one record per step with the
    whole data as its window unless overridden."""
    out = Plan()
    for slot, spec in specs.items():
        out.append(dict(i=len(out), kind="create", slot=slot, spec=spec, f32=spec["f32"], Mp=padded(spec["M"]), replaced_Mp=None))
    for kind, slot, kw in steps:
        spec = specs[slot]
        rec = dict(i=len(out), kind=kind, slot=slot, quadrature_n=spec["quadrature_n"], f32=spec["f32"], Mp=padded(spec["M"]), off=0,
                   nb=spec["N"], num_data=0.0, gamma=None, offsets=False, seed=1000 + len(out))
        rec.update(DEFAULTS.get(kind, {}))
        rec.update(kw)
        if kind == "lik_predictive":
            rec.setdefault("n", rec["nb"])
        out.append(rec)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=300.0)
    ap.add_argument("--seed", type=int, default=40)
    ap.add_argument("--slots", type=int, default=4)
    ap.add_argument("--twin-every", type=int, default=5)
    args = ap.parse_args()
    rng = np.random.default_rng(args.seed)
    ctx, twin_ctx = _ffi.Context(0), fresh_context
    planner, ex = Planner(rng, args.slots), Executor(ctx, twin_ctx)
    t0, n, bad, worst, redrawn, f32 = time.time(), 0, [], {}, 0, {}
    while time.time() - t0 < args.seconds:
        saved = planner.state()
        rec = planner.next()
        try:
            kind, errs = ex.run(rec, twin=n % args.twin_every == 0)
        except ReferenceFailure as e:
            planner.restore(saved)
            redrawn += 1
            print("OP", n, "REDRAWN", repr(e), flush=True)
            continue
        except Exception as e:
            bad.append((n, rec["kind"], ex.slots[rec["slot"]].tag(), repr(e)))
            print("OP", n, "EXCEPTION", rec, repr(e), flush=True)
            n += 1
            continue
        s = ex.slots[rec["slot"]]
        is64 = s.dtype == np.float64
        fails = {k: v for k, v in errs.items() if not v <= tolerance(kind, k, is64)}
        for k, v in errs.items():
            key = (kind, k, "f64" if is64 else "f32")
            worst[key] = max(worst.get(key, 0.0), v)
        extra = {k: rec[k] for k in ("off", "nb", "num_data", "gamma", "fetch", "want_grads", "want", "n", "variant", "inputs", "probe", "clear",
                                     "barred", "offsets") if rec.get(k) is not None}
        print("OP", n, kind, s.tag(), extra, "FAIL" if fails else "ok", {k: f"{v:.1e}" for k, v in (fails or errs).items()}, flush=True)
        if fails:
            bad.append((n, kind, s.tag(), extra, fails))
        n += 1
    ex.close()
    ctx.close()
    print(f"SUMMARY {n} operations in {time.time() - t0:.0f} s, {redrawn} redrawn, {len(bad)} outside tolerance")
    for k in sorted(worst):
        print("  worst", k, f"{worst[k]:.2e}")
    for b in bad:
        print("  BAD", b)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
