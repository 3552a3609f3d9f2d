"""What the edge tests of the pathwise sampler share (tests/test_gpu_pathwise_edges.py, test_pathwise_edges_cpu.py, fuzz_pathwise.py):

* a Python mirror of the dispatch of sample_eval_kernel<T, DREG, NSB> (`variant`) and of the sampler's paddings (`padding`), written from
  approximategps.jl_amd/csrc/sample.hip, sample_api.hip and api.hip with the line of every rule next to it;
  tests/test_pathwise_edges_cpu.py parses the same thresholds out of the sources, so the mirror cannot drift silently;
* the case table of the edge tests (TABLE) and the value lists of the seeded sweep (SWEEP);
* `problem` / `model` / `data` / `check`: one case -> inputs rounded to its dtype, the float64 restatement (tests/pathwise_ref.py) of it,
  the device objects, and the comparison at the bands of tests/test_gpu_pathwise.py (nothing new: fp64 1e-8 of max|F|, fp32
  max(1e-4, 4 e32) with e32 computed per case, u <= 1e-10, V <= 1e-8; stated conditions cond(Kuu) <= 1e4, max|V| <= 64).

No device is needed to import this module or to build a problem."""
import collections

import numpy as np

import pathwise_ref as pw
import svgp_oracle as o
from approxgp import _ffi
from approxgp.pathwise import draw_basis

JITTER = 1e-3
MEAN_CONST = 0.3
TOL64 = 1e-8          # tests/test_gpu_pathwise.py: the project's fp64 contract
F32_FACTOR = 4.0      # tests/test_gpu_pathwise.py: max(1e-4, 4 e32)
TOL_U, TOL_V = 1e-10, 1e-8
COND_MAX, V_MAX = 1e4, 64.0
SE, M32, M52 = o.KERNEL_SE, o.KERNEL_MATERN32, o.KERNEL_MATERN52
COL, ROW = _ffi.COLVECS, _ffi.ROWVECS
F64, F32 = np.float64, np.float32
SENTINEL = -777.0

# ---- the dispatch -------------------------------------------------------------------------------------------------------------------

DREGS = (4, 8, 16, 32, 64)            # sample.hip:204-208 (launch_eval_t): d <= 4, <= 8, <= 16, <= 32, else 64
COLUMN_BLOCK = 64                     # sample.hip:192 (launch_eval_d): one launch per 64 padded columns
ONE_BLOCK = 16                        # sample.hip:194: `a.Sp - s0 <= 16` -> NSB = 1, else NSB = 4
DIFF_MAX_DREG = 8                     # sample.hip:51: DIFF = sizeof(T) == 4 && DREG <= 8
PAD_M, PAD_L, PAD_S = 128, 32, 16     # api.hip:364 (Mp), sample_api.hip:58 (Lp), sample_api.hip:60 (Sp)


def dreg(d):
    """sample.hip:204-208."""
    for r in DREGS[:-1]:
        if d <= r:
            return r
    return DREGS[-1]


def point_groups(dtype, DREG, NSB):
    """sample.hip:30 (sample_point_groups): (sizeof(T) == 8 && DREG > 32 && NSB > 1) ? 1 : (DREG > 16 || NSB > 1) ? 2 : 4."""
    return 1 if (np.dtype(dtype).itemsize == 8 and DREG > 32 and NSB > 1) else 2 if (DREG > 16 or NSB > 1) else 4


def padding(M, L, S):
    """-> (Mp, Lp, Sp): api.hip:364, sample_api.hip:58, sample_api.hip:60."""
    up = lambda v, p: (v + p - 1) // p * p
    return up(M, PAD_M), up(L, PAD_L), up(S, PAD_S)


def variant(dtype, d, S):
    """The launches of one svgp_sampler_eval -> [(DREG, NSB, PG, DIFF, s0)], in launch order (sample.hip:190-209, :30, :51)."""
    Sp = padding(1, 0, S)[2]
    R = dreg(d)
    out = []
    for s0 in range(0, Sp, COLUMN_BLOCK):
        NSB = 1 if Sp - s0 <= ONE_BLOCK else 4
        out.append((R, NSB, point_groups(dtype, R, NSB), np.dtype(dtype).itemsize == 4 and R <= DIFF_MAX_DREG, s0))
    return out


ALL_VARIANTS = frozenset((np.dtype(dt).name, R, NSB) for dt in (F64, F32) for R in DREGS for NSB in (1, 4))


def variants_of(cases):
    """The (dtype name, DREG, NSB) kernels that a collection of cases launches."""
    return {(np.dtype(c.dtype).name, R, NSB) for c in cases for (R, NSB, _, _, _) in variant(c.dtype, c.d, c.S)}


# ---- the cases ----------------------------------------------------------------------------------------------------------------------

# layout_z / layout_x: of the model's z and of the data (d = 1 is a Vec whatever they say); with_mean: svgp_model_set_mean_z plus a
# prior_mean at the points; out: "host" | "host_ld" (ldo = len + 3) | "dev_ld" (device memory, ldo = len + 5); off: the window of the
# main evaluation is [off, n)
Case = collections.namedtuple("Case", "dtype M d n S L family centered layout_z layout_x with_mean out off")


def case_name(c):
    return f"{'f32' if c.dtype == F32 else 'f64'}_M{c.M}_d{c.d}_n{c.n}_S{c.S}_L{c.L}"


def case_seed(c):
    return 1000 + 7 * c.M + 13 * c.d + c.n + c.S + c.L   # as tests/test_gpu_pathwise.py::_problem


_T = [
    # dtype M    d   n*   S    L   family centered  z    x   mean   out      off
    (F64, 127, 4, 65, 16, 31, SE, False, COL, COL, False, "host", 0),
    (F64, 128, 5, 257, 3, 32, M32, True, COL, ROW, True, "dev_ld", 0),
    (F64, 129, 8, 63, 33, 33, M52, False, ROW, ROW, False, "host_ld", 0),
    (F64, 37, 9, 17, 16, 256, SE, True, COL, COL, False, "host", 0),
    (F64, 130, 16, 64, 17, 257, M32, False, ROW, COL, False, "dev_ld", 21),
    (F64, 37, 32, 129, 1, 31, M52, False, COL, COL, True, "host", 0),
    (F64, 130, 33, 257, 16, 33, SE, True, ROW, ROW, False, "host", 0),
    (F64, 37, 2, 65, 64, 0, M32, False, COL, COL, False, "dev_ld", 0),
    (F64, 37, 2, 65, 65, 32, M52, False, COL, ROW, False, "host_ld", 0),
    (F64, 37, 3, 17, 81, 33, SE, True, ROW, ROW, True, "host", 0),
    (F64, 17, 2, 15, 129, 31, M32, False, COL, COL, False, "host", 0),
    (F64, 17, 1, 16, 300, 257, SE, False, COL, COL, False, "host_ld", 0),
    (F32, 127, 4, 257, 16, 31, M52, True, COL, COL, False, "dev_ld", 0),
    (F32, 128, 5, 65, 17, 32, SE, False, ROW, ROW, False, "host", 0),
    (F32, 129, 8, 257, 1, 33, M32, False, COL, ROW, True, "dev_ld", 67),
    (F32, 37, 9, 64, 16, 256, M52, False, COL, COL, False, "host_ld", 0),
    (F32, 130, 16, 63, 33, 257, SE, True, ROW, COL, True, "host", 0),
    (F32, 130, 32, 129, 3, 31, M32, False, COL, COL, False, "host", 0),
    (F32, 37, 33, 65, 81, 33, M52, True, ROW, ROW, False, "dev_ld", 0),
    (F32, 17, 2, 17, 129, 0, SE, False, COL, COL, False, "host", 0),
    (F32, 17, 7, 15, 300, 257, M52, False, COL, COL, False, "host_ld", 0),
    (F32, 256, 6, 129, 65, 100, SE, False, COL, COL, False, "host", 0),
    # Four more than the table this work was specified with: read against `variant`, its 22 rows leave f64 and fp32 DREG = 32 with
    # NSB = 4, f64 DREG = 64 with NSB = 4 and fp32 DREG = 64 with NSB = 1 to tests/test_gpu_pathwise.py alone.  These rows launch them at
    # edges too (d = 17 one feature past DREG = 16; a second NSB = 4 launch at s0 = 64; 15 / 63 / 64 points), so that this table by itself
    # covers the 20 kernels (tests/test_pathwise_edges_cpu.py).
    (F64, 37, 17, 63, 81, 32, SE, False, COL, COL, False, "host", 0),
    (F64, 129, 64, 15, 17, 31, M32, True, COL, ROW, False, "dev_ld", 0),
    (F32, 127, 17, 64, 65, 33, M52, False, ROW, COL, False, "host", 0),
    (F32, 37, 64, 17, 16, 1, SE, False, COL, COL, True, "host_ld", 0),
]
TABLE = {case_name(c): c for c in (Case(*t) for t in _T)}
assert len(TABLE) == len(_T)
N_SPECIFIED = 22   # the first 22 rows are the specified table, in its order

# the value lists of the seeded sweep (tests/fuzz_pathwise.py)
SWEEP = dict(M=[1, 17, 37, 127, 128, 129, 257, 300], d=[1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64], S=[1, 3, 16, 17, 64, 65, 81, 129],
             L=[0, 1, 31, 32, 33, 100, 256, 257], n=[1, 15, 16, 17, 63, 64, 65, 129, 257, 1000], family=[SE, M32, M52],
             out=["host", "host_ld", "dev_ld"])


# ---- one case: inputs, restatement, device objects, comparison ----------------------------------------------------------------------

def problem(c, seed=None):
    """Everything of a case, read-only: the model, the points, the basis (rounded to the case's dtype, so that the restatement and the
    device start from the same numbers) and the restatement's results.  e32: the error of the restatement's own float32 data stage
    against its float64 one (None for an fp64 case)."""
    dt = c.dtype
    rd = lambda a: np.asarray(a, dtype=dt).astype(np.float64)
    seed = case_seed(c) if seed is None else seed
    sva, muz = pw.recipe(c.M, c.d, c.family, seed, centered=c.centered, mean_const=MEAN_CONST, with_muz=c.with_mean, jitter=JITTER, dtype=dt)
    rng = np.random.default_rng(seed + 1)
    x = rd(rng.uniform(-3.0, 3.0, size=(c.d, c.n)))
    mux = rd(0.3 * np.cos(x[0])) if c.with_mean else None
    basis = draw_basis(c.family, c.M, c.L, c.S, rng, dt, d=c.d)
    omega, tau, w, eps = (a.astype(np.float64) for a in basis)
    st = pw.setup(sva, omega, tau, w, eps, muz=muz)
    F = pw.evaluate(sva, st, x, omega, tau, w, mux=mux)
    e32 = None
    if dt == F32:
        e32 = float(np.abs(pw.evaluate(sva, st, x, omega, tau, w, mux=mux, f32=True).astype(np.float64) - F).max() / np.abs(F).max())
    for a in (x, F, st["u"], st["V"]) + tuple(basis) + ((muz, mux) if c.with_mean else ()):
        a.setflags(write=False)
    return dict(case=c, sva=sva, muz=muz, x=x, mux=mux, basis=basis, st=st, F=F, e32=e32, vmax=float(np.abs(st["V"]).max()))


def meets_conditions(p):
    return p["st"]["cond"] <= COND_MAX and p["vmax"] <= V_MAX


def tolerance(p):
    return TOL64 if p["e32"] is None else max(1e-4, F32_FACTOR * p["e32"])


def rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def _laid_out(a, d, layout):
    """A (d, n) array as the library takes it in `layout`."""
    return a[0] if d == 1 else (a if layout == COL else np.ascontiguousarray(a.T))


def model(ctx, p, sva=None):
    c = p["case"]
    sva = sva if sva is not None else p["sva"]
    desc, keep = _ffi.make_desc(c.dtype, sva.kernel.family, sva.kernel.variance, sva.kernel.inv_lengthscale, _laid_out(sva.z, c.d, c.layout_z),
                                sva.m, sva.Lq, sva.jitter, parametrization=_ffi.CENTERED if sva.centered else _ffi.NONCENTERED, lik_sigma2=0.1,
                                mean_const=sva.mean_const, layout_z=c.layout_z)
    mdl = _ffi.DeviceModel(ctx, desc, keep)
    if p["muz"] is not None:
        mdl.set_mean_z(p["muz"])
    return mdl


def data(ctx, p, x=None, y=None):
    c = p["case"]
    return _ffi.DeviceData(ctx, _laid_out(p["x"] if x is None else x, c.d, c.layout_x), y, c.dtype, layout=c.layout_x)


def window_mean(p, off, length):
    return None if p["mux"] is None else p["mux"][off:off + length]


def eval_device_memory(smp, dat, off, length, ldo, prior_mean=None):
    """eval into device memory, rows ldo apart -> the whole (S, ldo) buffer on the host (columns >= length keep the sentinel)."""
    import torch

    tdt = torch.float32 if smp.dtype == _ffi.F32 else torch.float64
    buf = torch.full((smp.n_samples, ldo), SENTINEL, dtype=tdt, device="cuda")
    torch.cuda.synchronize()
    smp.eval(dat, off, length, prior_mean=prior_mean, out=buf, ldo=ldo)
    return buf.cpu().numpy()


def eval_as_the_case_says(smp, dat, p, off, length):
    """The window [off, off + length) through the case's output kind -> (S, length); the columns beyond `length` are checked."""
    c = p["case"]
    pm = window_mean(p, off, length)
    if c.out == "dev_ld":
        full = eval_device_memory(smp, dat, off, length, length + 5, prior_mean=pm)
        assert full.shape == (c.S, length + 5)
        assert np.all(full[:, length:] == SENTINEL), "columns beyond len were written (device output, ldo > len)"
        return full[:, :length]
    if c.out == "host_ld":
        full = smp.eval(dat, off, length, prior_mean=pm, ldo=length + 3)
        assert full.shape == (c.S, length + 3)
        assert np.all(full[:, length:] == 0.0), "columns beyond len were written (host output, ldo > len)"
        return full[:, :length]
    return smp.eval(dat, off, length, prior_mean=pm)


def window_cuts(n):
    """(cut, point) of the window contract: a cut that is odd (so no multiple of 16) and away from the middle, one interior point."""
    return (n // 3) | 1, n // 2


def check_windows(smp, dat, p, whole):
    """`whole` = the host evaluation of all n points.  Two windows cut at an odd position and a single interior point are bitwise equal
    to it (include/svgp_mi355x.h: a point's value does not depend on the window or the call).  n* < 3: the repeat alone."""
    n = p["case"].n
    assert np.array_equal(whole, smp.eval(dat, prior_mean=p["mux"])), "a repeated evaluation differs"
    if n < 3:
        return
    cut, pt = window_cuts(n)
    assert 0 < cut < n and cut % 16 != 0
    a = smp.eval(dat, 0, cut, prior_mean=window_mean(p, 0, cut))
    b = smp.eval(dat, cut, n - cut, prior_mean=window_mean(p, cut, n - cut))
    one = smp.eval(dat, pt, 1, prior_mean=window_mean(p, pt, 1))
    got = np.concatenate([a, b], axis=1)
    bad = np.argwhere(got != whole)
    assert bad.size == 0, f"windows [0, {cut}) + [{cut}, {n}) differ from the whole at (s, j) = {bad[:4].tolist()} ({len(bad)} entries)"
    assert np.array_equal(whole[:, pt:pt + 1], one), f"the single point {pt} differs from the whole"


def check_columns(F, ref, tol, scale=None):
    """For every sample s: max_j |F[s, j] - ref[s, j]| <= tol max|ref|.  The max-norm implies it; a wrong column block names itself."""
    F, ref = np.asarray(F, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    scale = max(np.abs(ref).max(), 1e-300) if scale is None else scale
    per = np.abs(F - ref).max(axis=1) / scale
    worst = int(np.argmax(per))
    assert np.all(np.isfinite(F)), f"non-finite values in samples {np.unique(np.argwhere(~np.isfinite(F))[:, 0])[:8].tolist()}"
    assert per[worst] <= tol, (f"sample {worst} (column block s0 = {worst // COLUMN_BLOCK * COLUMN_BLOCK}, 16-block {worst // 16}) is off by "
                               f"{per[worst]:.2e} > {tol:.2e}; samples outside: {np.flatnonzero(per > tol)[:16].tolist()}")
    return float(per[worst])


def run_case(ctx, p, windows=True, window=None):
    """The case on the device against its restatement -> dict(F, u, V errors ...).  Asserts the bands.  window = (off, len): the window
    of the evaluation through the case's output kind, instead of [case.off, n)."""
    c = p["case"]
    off, length = (c.off, c.n - c.off) if window is None else window
    assert meets_conditions(p), (p["st"]["cond"], p["vmax"])   # the stated conditions, before the device is touched
    mdl, dat = model(ctx, p), data(ctx, p)
    try:
        smp = mdl.sampler(p["basis"])
        try:
            F = eval_as_the_case_says(smp, dat, p, off, length)
            u, V = smp.state()
            whole = smp.eval(dat, prior_mean=p["mux"])
            assert whole.shape == (c.S, c.n) and whole.dtype == c.dtype and F.dtype == c.dtype
            if windows:
                check_windows(smp, dat, p, whole)
        finally:
            smp.free()
    finally:
        mdl.free()
        dat.free()
    tol = tolerance(p)
    scale = float(np.abs(p["F"]).max())
    res = dict(u=rel(u, p["st"]["u"]), V=rel(V, p["st"]["V"]), tol=tol, e32=p["e32"], cond=p["st"]["cond"], vmax=p["vmax"])
    assert res["u"] <= TOL_U and res["V"] <= TOL_V, (res["u"], res["V"])
    # the case's own output kind and window, then the whole range through host output
    assert np.array_equal(F, whole[:, off:off + length]), (
        f"the window [{off}, {off + length}) through output kind {c.out!r} differs bitwise from the host evaluation of the whole")
    res["F"] = check_columns(whole, p["F"], tol, scale)
    check_columns(F, p["F"][:, off:off + length], tol, scale)
    return res


def report_line(name, r):
    return (f"| {name} | {r['F']:.2e} | {r['tol']:.2e} | {'-' if r['e32'] is None else format(r['e32'], '.2e')} | {r['u']:.1e} | {r['V']:.1e} | "
            f"{r['cond']:.1e} | {r['vmax']:.1f} |")
