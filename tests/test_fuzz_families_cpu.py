"""The device-free half of tests/fuzz_families.py: what the seeded slices of tests/test_gpu_fuzz_families.py cover, that a plan is a
function of its seed, that the reference can evaluate what is drawn, and the slot bookkeeping (adopting q, mu_z, keep_q, the barred
calls) with the device's outputs replaced by the restatements' own."""
import functools

import numpy as np

import fuzz_families as ff
import natgrad_ref as nr
import svgp_oracle as o


@functools.lru_cache(maxsize=None)
def _plan(name):
    return ff.slice_plan(name)


def test_every_op_kind_at_least_three_times_in_each_slice():
    for name in ff.SLICES:
        kinds = ff.coverage([_plan(name)])[0]
        short = {k: kinds.get(k, 0) for k in ff.OLD_OPS + ff.NEW_OPS if kinds.get(k, 0) < 3}
        assert not short, (name, short)
        assert len(_plan(name)) == ff.SLICE_OPS


def test_every_reader_follows_every_q_writer_across_the_slices():
    _, pairs, mp_changes = ff.coverage([_plan(name) for name in ff.SLICES])
    missing = [(w, f) for w in ff.Q_WRITERS for f in ff.FOLLOWERS if pairs.get((w, f), 0) < 1]
    assert not missing, missing
    assert mp_changes >= 1          # a slot replaced by one of another Mp between a natgrad op and a natgrad / collapsed op on the new slot


def test_slices_are_the_dtypes_they_say():
    f32 = {name: {rec["spec"]["f32"] for rec in _plan(name) if rec["kind"] == "create"} for name in ff.SLICES}
    assert f32 == {"f64": {False}, "f32": {True}, "mixed": {False, True}}


def test_shapes_and_arguments_stay_in_the_issue_s_lists():
    for name in ff.SLICES:
        for rec in _plan(name):
            if rec["kind"] == "create":
                sp = rec["spec"]
                assert sp["M"] in ff.MS and sp["N"] in ff.NS and sp["d"] in ff.DS and sp["quadrature_n"] in ff.QNS and sp["lik"] in ff.LIKS
                assert not (sp["M"] >= 200 and sp["N"] > 1025)
            elif rec["kind"] in ("natgrad", "natgrad_ext"):
                assert rec["gamma"] in ff.GAMMAS


def test_same_seed_same_plan():
    for name in ff.SLICES:
        assert list(ff.slice_plan(name)) == list(_plan(name))
    a = ff.plan(np.random.default_rng(5), 40)
    assert list(a) == list(ff.plan(np.random.default_rng(5), 40)) and list(a) != list(ff.plan(np.random.default_rng(6), 40))


def test_reference_evaluates_the_slices_with_few_redraws():
    """plan(simulate=True) walks the reference side and redraws what the restatement cannot evaluate; it asserts a share under 2 % itself.
    The committed slices need none, so the plan the GPU test executes is the simulated one."""
    for name in ff.SLICES:
        p = ff.slice_plan(name, simulate=True)
        assert p.redrawn < 0.02 * len(p)
        assert list(p) == list(_plan(name)) or p.redrawn > 0


def test_random_plan_runs_through_the_reference_side():
    p = ff.plan(np.random.default_rng(9), 25)
    results = ff.execute(None, p)
    assert len(results) == 25 and all(errs == {} for _, errs in results)


def test_slot_bookkeeping_without_a_device():
    specs = {0: ff.spec_of(17, 33, 2, seed=3, centered=True), 1: ff.spec_of(17, 33, 2, seed=4, lik=o.LIK_POISSON_EXP)}
    steps = [("natgrad", 0, dict(gamma=0.7)),                    # 2: adopts the restatement's q (no device): one call since the exact q
             ("keep_q", 0, {}),                                  # 3: new hyperparameters, the old q
             ("mean_z", 0, dict(barred="natgrad", gamma=0.7)),   # 4: offsets at z persist; the barred call changes nothing
             ("elbo", 0, {}),                                    # 5
             ("mean_z", 0, dict(clear=True)),                    # 6
             ("collapsed_q", 0, {}),                             # 7
             ("update", 0, {}),                                  # 8: a full upload: exactly known again
             ("natgrad_ext", 1, dict(gamma=1.0, fetch=False))]   # 9
    p = ff.script(specs, steps)
    ex = ff.Executor(None)
    for rec in p[:2]:
        ex.run(rec)
    s = ex.slots[0]
    start = s.sva
    xs, ys = s.x, s.y
    ex.run(p[2])
    want = nr.step(start, xs, ys, lik=s.lik, sigma2=s.s2, gamma=0.7)
    assert np.array_equal(s.sva.m, want.m) and np.array_equal(s.sva.Lq, want.Lq) and s.base is start and len(s.pending) == 1
    q = (s.sva.m, s.sva.Lq)
    ex.run(p[3])
    assert np.array_equal(s.sva.m, q[0]) and np.array_equal(s.sva.Lq, q[1]) and s.sva.kernel.variance != start.kernel.variance and len(s.pending) == 2
    assert s.sva.mean_const != start.mean_const and not np.array_equal(s.sva.z, start.z) and s.base is start
    ex.run(p[4])
    assert s.muz is not None and s.muz.shape == (17,) and np.array_equal(s.sva.m, q[0]) and len(s.pending) == 2
    muz = s.muz
    ex.run(p[5])
    assert s.muz is muz
    ex.run(p[6])
    assert s.muz is None
    ex.run(p[7])
    assert len(s.pending) == 3 and not np.array_equal(s.sva.m, q[0])
    ex.run(p[8])
    assert s.pending == [] and s.base is s.sva
    t = ex.slots[1]
    before = t.sva
    ex.run(p[9])
    assert len(t.pending) == 1 and t.base is before and t.sva is not before
    assert ex.slots[0].pending == []
    ex.close()


def test_planner_bars_what_the_library_bars():
    """While mu_z is set on a slot no natgrad / collapsed / shard op is drawn for it, and mean_z is drawn for Centered
    slots only; the collapsed calls for Gaussian slots only."""
    for name in ff.SLICES:
        spec, muz = {}, {}
        for rec in _plan(name):
            k, sl = rec["kind"], rec["slot"]
            if k == "create":
                spec[sl], muz[sl] = rec["spec"], False
                continue
            if k == "mean_z":
                assert spec[sl]["centered"]
                muz[sl] = not rec["clear"]
            elif ff.follower_class(k) in ("natgrad", "collapsed") or k == "shard":
                assert not muz[sl], rec
            if k.startswith("collapsed"):
                assert spec[sl]["lik"] == o.LIK_GAUSSIAN


def test_twin_comparison_is_bitwise():
    a = {"v": 1.0, "arr": np.array([1.0, 2.0]), "none": None, "nan": np.array([np.nan])}
    assert ff._same(a, {"v": 1.0, "arr": np.array([1.0, 2.0]), "none": None, "nan": np.array([np.nan])}) is None
    assert ff._same(a, {**a, "arr": np.array([1.0, np.nextafter(2.0, 3.0)])}) == "arr"
    assert ff._same(a, {**a, "v": np.nextafter(1.0, 2.0)}) == "v"
    assert ff._same(a, {**a, "none": np.zeros(1)}) == "none"
    assert ff.tolerance("natgrad", "twin", True) == 0.0 and ff.tolerance("predictive", "twin", False) == 0.0
