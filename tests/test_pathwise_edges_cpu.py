"""The device-free half of the pathwise sampler's edge tests (tests/pathwise_cases.py, fuzz_pathwise.py, test_gpu_pathwise_edges.py):

* the case table launches every one of the 20 kernels sample_eval_kernel<T, DREG, NSB> according to the mirror of the dispatch, holds the
  boundary values of d, S, L, M and n*, an NSB = 4 launch at s0 > 0 and a case of three or more launches;
* every table case meets the stated conditions (cond(Kuu) <= 1e4, max|V| <= 64) on the float64 restatement;
* the seeded slice of the sweep covers the 20 kernels too and skips at most 5 % of its cases;
* the mirror agrees with the sources: the thresholds are parsed out of csrc/sample.hip, sample_api.hip and api.hip."""
import os
import re

import numpy as np
import pytest

import fuzz_pathwise as fp
import pathwise_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "approximategps.jl_amd", "csrc")
CASES = list(pc.TABLE.values())


def _src(name):
    return open(os.path.join(CSRC, name)).read()


def test_the_table_launches_every_kernel_variant():
    assert len(pc.ALL_VARIANTS) == 20
    missing = pc.ALL_VARIANTS - pc.variants_of(CASES)
    assert not missing, sorted(missing)
    # PG and DIFF are functions of the variant; the table meets each of their values, and the widest by-differences path
    launches = [(np.dtype(c.dtype).name,) + v for c in CASES for v in pc.variant(c.dtype, c.d, c.S)]
    assert {v[3] for v in launches} == {1, 2, 4}
    assert ("float32", 8, 1, 4, True, 0) in launches and ("float32", 8, 4, 2, True, 0) in launches
    assert any(v[1] == 16 and not v[4] for v in launches if v[0] == "float32")   # the fp32 expansion form at d = 9..16


def test_the_table_holds_the_specified_cases_and_every_edge_value():
    spec = CASES[:pc.N_SPECIFIED]
    assert [(np.dtype(c.dtype).name, c.M, c.d, c.n, c.S, c.L, c.family, c.centered) for c in spec] == [
        ("float64", 127, 4, 65, 16, 31, pc.SE, False), ("float64", 128, 5, 257, 3, 32, pc.M32, True),
        ("float64", 129, 8, 63, 33, 33, pc.M52, False), ("float64", 37, 9, 17, 16, 256, pc.SE, True),
        ("float64", 130, 16, 64, 17, 257, pc.M32, False), ("float64", 37, 32, 129, 1, 31, pc.M52, False),
        ("float64", 130, 33, 257, 16, 33, pc.SE, True), ("float64", 37, 2, 65, 64, 0, pc.M32, False),
        ("float64", 37, 2, 65, 65, 32, pc.M52, False), ("float64", 37, 3, 17, 81, 33, pc.SE, True),
        ("float64", 17, 2, 15, 129, 31, pc.M32, False), ("float64", 17, 1, 16, 300, 257, pc.SE, False),
        ("float32", 127, 4, 257, 16, 31, pc.M52, True), ("float32", 128, 5, 65, 17, 32, pc.SE, False),
        ("float32", 129, 8, 257, 1, 33, pc.M32, False), ("float32", 37, 9, 64, 16, 256, pc.M52, False),
        ("float32", 130, 16, 63, 33, 257, pc.SE, True), ("float32", 130, 32, 129, 3, 31, pc.M32, False),
        ("float32", 37, 33, 65, 81, 33, pc.M52, True), ("float32", 17, 2, 17, 129, 0, pc.SE, False),
        ("float32", 17, 7, 15, 300, 257, pc.M52, False), ("float32", 256, 6, 129, 65, 100, pc.SE, False)]
    have = lambda k: {getattr(c, k) for c in CASES}
    assert {4, 5, 8, 9, 16, 32, 33} <= have("d")
    assert {16, 64, 65, 81, 129, 300} <= have("S")
    assert {31, 32, 33, 256, 257} <= have("L")
    assert {127, 128, 129} <= have("M")
    assert {15, 16, 17, 63, 64, 65, 257} <= have("n")
    per_case = [pc.variant(c.dtype, c.d, c.S) for c in CASES]
    assert any(NSB == 4 and s0 > 0 for v in per_case for (_, NSB, _, _, s0) in v)
    assert any(len(v) >= 3 for v in per_case)
    # NSB = 4 at s0 = 64 with a PARTIAL block: fewer than 64 padded columns left, and the last 16-block ragged (S = 81: Sp = 96)
    assert any(NSB == 4 and s0 > 0 and pc.padding(1, 0, c.S)[2] - s0 < 64 and c.S % 16 for c, v in zip(CASES, per_case) for (_, NSB, _, _, s0) in v)
    # what is spread over the cases
    assert sum(c.layout_z != c.layout_x and c.d > 1 for c in CASES) >= 2
    assert sum(c.out == "dev_ld" and c.off > 0 for c in CASES) >= 2
    assert {c.out for c in CASES} == {"host", "host_ld", "dev_ld"} and {c.layout_z for c in CASES} == {pc.COL, pc.ROW}
    assert any(c.with_mean and c.centered for c in CASES) and any(c.with_mean and not c.centered for c in CASES)
    for c in CASES:
        assert 0 <= c.off < c.n


def test_paddings():
    assert pc.padding(127, 31, 16) == (128, 32, 16) and pc.padding(128, 32, 17) == (128, 32, 32) and pc.padding(129, 33, 300) == (256, 64, 304)
    assert pc.padding(1, 0, 1) == (128, 0, 16) and pc.padding(300, 256, 64) == (384, 256, 64) and pc.padding(17, 257, 65) == (128, 288, 80)


@pytest.mark.parametrize("name", list(pc.TABLE))
def test_table_case_meets_the_stated_conditions(name):
    p = pc.problem(pc.TABLE[name])
    print(f"{name}: cond {p['st']['cond']:.2e}, max|V| {p['vmax']:.1f}, e32 {p['e32']}")
    assert pc.meets_conditions(p), (p["st"]["cond"], p["vmax"])
    assert np.all(np.isfinite(p["F"])) and p["F"].shape == (pc.TABLE[name].S, pc.TABLE[name].n)


def test_the_seeded_slice_covers_every_variant_and_skips_little():
    plan_ = fp.slice_plan()
    assert len(plan_) == fp.SLICE_CASES == 60
    assert plan_ == fp.slice_plan()   # a plan is a function of its seed
    missing = pc.ALL_VARIANTS - pc.variants_of([r["case"] for r in plan_])
    assert not missing, sorted(missing)
    for r in plan_:
        off, length = r["window"]
        assert 0 <= off and 1 <= length and off + length <= r["case"].n
        for k in ("M", "d", "S", "L", "n"):
            assert getattr(r["case"], k) in pc.SWEEP[k]
    results = fp.execute(None, plan_)   # the reference side alone
    assert not fp.failures(results)
    print(f"skipped {sum(r['skipped'] for r in results)} of {len(results)}")
    fp.check_skips(results)


def test_check_skips_fails_above_five_percent():
    ok = [dict(name="a", skipped=False, cond=1.0, vmax=1.0)] * 19 + [dict(name="b", skipped=True, cond=2e4, vmax=70.0)]
    fp.check_skips(ok)   # 5 %
    with pytest.raises(AssertionError):
        fp.check_skips(ok[1:])


def test_the_mirror_agrees_with_the_sources():
    hip = _src("sample.hip")
    # launch_eval_t: the chain of d <= R, each launching DREG = R, and the else branch
    body = re.search(r"void launch_eval_t\(.*?\{(.*?)\n\}", hip, flags=re.S).group(1)
    chain = [(int(a), int(b)) for a, b in re.findall(r"if \(a\.d <= (\d+)\) launch_eval_d<T, (\d+)>", body)]
    last = int(re.search(r"\n\s*else launch_eval_d<T, (\d+)>", body).group(1))
    assert all(a == b for a, b in chain)
    assert tuple(a for a, _ in chain) + (last,) == pc.DREGS
    for d in range(1, 65):
        assert pc.dreg(d) == next((r for r in pc.DREGS if d <= r))
    # launch_eval_d: the 64-column loop, NSB = 1 at <= 16 padded columns left and 4 otherwise
    body = re.search(r"void launch_eval_d\(.*?\{(.*?)\n\}", hip, flags=re.S).group(1)
    assert int(re.search(r"for \(int64_t s0 = 0; s0 < a\.Sp; s0 \+= (\d+)\)", body).group(1)) == pc.COLUMN_BLOCK
    assert int(re.search(r"const bool one = a\.Sp - s0 <= (\d+);", body).group(1)) == pc.ONE_BLOCK
    assert re.search(r"if \(one\) hipLaunchKernelGGL\(\(sample_eval_kernel<T, DREG, 1>\)", body)
    assert re.search(r"else hipLaunchKernelGGL\(\(sample_eval_kernel<T, DREG, 4>\)", body)
    # sample_point_groups: the expression itself, evaluated over every variant
    expr = re.search(r"constexpr int sample_point_groups\(\) \{\s*return (.*?);\s*\}", hip, flags=re.S).group(1)
    assert re.fullmatch(r"[\w\s()<>=&|?:]+", expr)

    def c_ternary(e, env):
        e = e.strip()
        depth = 0
        for i, ch in enumerate(e):   # the first top-level '?' splits condition from the branches; ':' at the same depth of ternaries
            depth += ch == "("
            depth -= ch == ")"
            if ch == "?" and depth == 0:
                cond, rest = e[:i], e[i + 1:]
                nest = par = 0
                for j, cj in enumerate(rest):
                    par += cj == "("
                    par -= cj == ")"
                    if par == 0 and cj == "?":
                        nest += 1
                    if par == 0 and cj == ":":
                        if nest == 0:
                            return c_ternary(rest[:j], env) if c_ternary(cond, env) else c_ternary(rest[j + 1:], env)
                        nest -= 1
        return eval(e.replace("&&", " and ").replace("||", " or ").replace("sizeof(T)", "SIZEOF_T"), {"__builtins__": {}}, env)

    for dt in (pc.F64, pc.F32):
        for R in pc.DREGS:
            for NSB in (1, 4):
                assert c_ternary(expr, dict(SIZEOF_T=np.dtype(dt).itemsize, DREG=R, NSB=NSB)) == pc.point_groups(dt, R, NSB), (dt, R, NSB)
    # a workgroup's points: 4 waves x 16 points x PG
    assert re.search(r"const int64_t per = 4 \* 16 \* \(one \? sample_point_groups<T, DREG, 1>\(\) : sample_point_groups<T, DREG, 4>\(\)\);", hip)
    # DIFF
    m = re.search(r"constexpr bool DIFF = sizeof\(T\) == 4 && DREG <= (\d+);", hip)
    assert int(m.group(1)) == pc.DIFF_MAX_DREG
    # ... and the host side that lays out the inducing rows for those kernels (raw z) draws the same line
    m = re.search(r"const int raw = \(dtype != 0 && d <= (\d+)\) \? 1 : 0;", hip)
    assert int(m.group(1)) == pc.DIFF_MAX_DREG
    # the paddings
    api = _src("sample_api.hip")
    m = re.search(r"sp->Lp = \(L \+ (\d+)\) / (\d+) \* (\d+);", api)
    assert (int(m.group(1)) + 1, int(m.group(2)), int(m.group(3))) == (pc.PAD_L,) * 3
    assert int(re.search(r"constexpr int kSampleKC = (\d+);", hip).group(1)) == pc.PAD_L   # Lp and Mp are multiples of the chunk
    m = re.search(r"sp->Sp = \(S \+ (\d+)\) / (\d+) \* (\d+);", api)
    assert (int(m.group(1)) + 1, int(m.group(2)), int(m.group(3))) == (pc.PAD_S,) * 3
    m = re.search(r"m->Mp = \(desc->M \+ (\d+)\) / (\d+) \* (\d+);", _src("api.hip"))
    assert (int(m.group(1)) + 1, int(m.group(2)), int(m.group(3))) == (pc.PAD_M,) * 3
    assert pc.PAD_M % pc.PAD_L == 0


def test_the_cited_lines_hold_the_rules():
    """pathwise_cases.py cites file:line next to each rule; the lines still hold what it says."""
    hip, api, main = (_src(f).splitlines() for f in ("sample.hip", "sample_api.hip", "api.hip"))
    assert "DREG > 32 && NSB > 1" in hip[30 - 1]
    assert "constexpr bool DIFF" in hip[51 - 1]
    assert "s0 += 64" in hip[192 - 1] and "a.Sp - s0 <= 16" in hip[194 - 1]
    assert "a.d <= 4" in hip[204 - 1] and "launch_eval_d<T, 64>" in hip[208 - 1]
    assert "sp->Lp" in api[58 - 1] and "sp->Sp" in api[60 - 1] and "m->Mp" in main[364 - 1]
