"""Two ranks sharing the one GPU of the test box (gloo for the collective, the HIP library for every partial):
the data-parallel ELBO and value-and-gradient of approxgp/distributed.py against a single-process evaluation.
The 8-GPU RCCL launch itself is the driver's; this covers everything but the transport."""
import os
import socket
import sys

import numpy as np
import pytest
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rank(rank, world, port, out, centered):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    for p in (os.path.join(ROOT, "approximategps.jl_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)
    import torch.distributed as dist

    import svgp_oracle as o
    from approxgp import _ffi
    from approxgp.distributed import ShardedELBO, shard_range
    from helpers import device_model

    dist.init_process_group("gloo", rank=rank, world_size=world)
    N, M, d, batch = 4001, 96, 3, 700
    x, y, nc, s2 = o.synth_problem(71, N, M, d, family=o.KERNEL_MATERN52)
    sva = o.SVA(nc.kernel, nc.z, nc.m + 0.2, 0.8 * nc.Lq, jitter=1e-4, mean_const=0.1, centered=True) if centered else nc
    lo, hi = shard_range(N, rank, world)
    ctx = _ffi.Context(0)
    model = device_model(ctx, sva, sigma2=s2)
    data = _ffi.DeviceData(ctx, x[:, lo:hi], y[lo:hi], np.float64)        # this rank's shard only
    sh = ShardedELBO(model, data, num_data=float(N))
    full = sh.step(0, hi - lo)                                             # whole data set, sharded
    val, g = sh.step_grad(100, batch, n_global=world * batch, world=world)  # a minibatch window per rank
    if rank == 0:
        ref_full = o.elbo(sva, x, y, sigma2=s2)
        idx = np.concatenate([np.arange(shard_range(N, r, world)[0] + 100, shard_range(N, r, world)[0] + 100 + batch)
                              for r in range(world)])
        ref_val, ref_g = o.elbo_grad(sva, x[:, idx], y[idx], sigma2=s2, num_data=float(N))
        errs = [abs(full - ref_full) / abs(ref_full), abs(val - ref_val) / abs(ref_val)]
        errs += [float(np.abs(np.asarray(g[k], dtype=np.float64).reshape(np.shape(ref_g[k]), order="F") - np.asarray(ref_g[k])).max()
                       / max(np.abs(np.asarray(ref_g[k])).max(), 1e-12)) for k in ("variance", "inv_lengthscale", "z", "m", "Lq", "mean_const")]
        np.save(out, np.array(errs))
    model.free()
    data.free()
    dist.destroy_process_group()


@pytest.mark.parametrize("centered", [False, True])
def test_two_ranks_on_one_gpu_match_single_process(tmp_path, centered):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    out = str(tmp_path / "res.npy")
    mp.spawn(_rank, args=(2, port, out, centered), nprocs=2, join=True)
    errs = np.load(out)
    assert errs[0] < 1e-8 and errs[1] < 1e-8, errs      # fp64 ELBO contract
    assert errs[2:].max() < 1e-6, errs                  # gradient blocks, relative to their max-norm


# ---- the collective INSIDE the library (csrc/comm.hip) -----------------------------------------------------------
# The test box has one GPU and RCCL refuses the same device twice in one communicator, so what runs here is a world of
# one rank: the full code path (dlopen of librccl, ncclCommInitRank / ncclCommInitAll, ncclAllReduce of the
# device-resident vectors on the context's stream, grouped gradient all-reduce, status flags), with a sum over one rank.
def _problem(centered, dtype=np.float64):
    import svgp_oracle as o

    N, M, d = 3001, 96, 3
    x, y, nc, s2 = o.synth_problem(72, N, M, d, family=o.KERNEL_MATERN52, dtype=dtype)
    sva = o.SVA(nc.kernel, nc.z, nc.m + 0.2, 0.8 * nc.Lq, jitter=nc.jitter, mean_const=0.1, centered=True) if centered else nc
    return x, y, sva, s2


@pytest.mark.parametrize("centered", [False, True])
def test_library_collective_world_of_one(centered):
    for p in (os.path.join(ROOT, "approximategps.jl_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import svgp_oracle as o
    from approxgp import _ffi
    from helpers import device_model

    x, y, sva, s2 = _problem(centered)
    ctx = _ffi.Context(0)
    model = device_model(ctx, sva, sigma2=s2)
    data = _ffi.DeviceData(ctx, x, y, np.float64)
    local = model.elbo(data, 100, 1500, 9000.0)
    lv, _, lg = model.elbo_grad(data, 100, 1500, 9000.0)
    ctx.attach_comm(_ffi.comm_unique_id(), 1, 0)
    assert ctx.comm_info() == (1, 0)
    val, t = model.elbo(data, 100, 1500, 9000.0)            # collective path: ncclAllReduce on d_res
    assert val == local[0] and t.n_points == 1500 and t.scale == 6.0
    gv, gt, gg = model.elbo_grad(data, 100, 1500, 9000.0)   # n_global all-reduced on the device, grouped gradient all-reduce
    assert abs(gv - lv) <= 1e-12 * abs(lv) and gt.n_points == 1500
    for k in ("variance", "lik_sigma2", "mean_const", "inv_lengthscale", "z", "m", "Lq"):
        np.testing.assert_allclose(np.asarray(gg[k]), np.asarray(lg[k]), rtol=1e-12, atol=1e-13)
    assert abs(val - o.elbo(sva, x[:, 100:1600], y[100:1600], sigma2=s2, num_data=9000.0)) <= 1e-8 * abs(val)
    # the host-evaluated-likelihood form takes the same collective route (handshake, device-side sum E, grouped all-reduce)
    mu, var = model.marginals(data, 100, 1500)
    yb = y[100:1600]
    e_host = o.expected_loglik(o.LIK_GAUSSIAN, mu, np.sqrt(var), yb, s2)
    gmu_h, gv_h, _ = o.expected_loglik_grads(o.LIK_GAUSSIAN, mu, var, yb, s2)
    ev, et, eg = model.elbo_grad(data, 100, 1500, 9000.0, ext=(e_host, gmu_h, gv_h))
    assert abs(ev - gv) <= 1e-12 * abs(gv) and et.n_points == 1500
    for k in ("variance", "mean_const", "inv_lengthscale", "z", "m", "Lq"):
        np.testing.assert_allclose(np.asarray(eg[k]), np.asarray(gg[k]), rtol=1e-9, atol=1e-11)
    # a local argument error still goes through the collective and comes back as the argument error
    with pytest.raises(ValueError):
        model.elbo(data, 2900, 500, 0.0)
    assert model.elbo(data, 100, 1500, 9000.0)[0] == val      # and the communicator is still usable
    with pytest.raises(ValueError):                           # the gradient call: argument errors go through its opening handshake
        model.elbo_grad(data, 2900, 500, 0.0)
    g2 = model.elbo_grad(data, 100, 1500, 9000.0)
    assert abs(g2[0] - lv) <= 1e-12 * abs(lv)
    # (round 6) a rank handed NO model: it cannot size the gradient all-reduce, so it takes part in the opening
    # fixed-size all-reduce only (with the failure flag) and returns its own error; rounds 2-5 aborted the communicator here
    import ctypes as C
    out_, terms_, grads_ = C.c_double(), _ffi.Terms(), _ffi.Grads()
    rc_null = ctx.lib.svgp_elbo_grad(ctx.h, None, data.h, 100, 1500, 9000.0, C.byref(out_), C.byref(terms_), C.byref(grads_))
    assert rc_null == _ffi.INVALID_ARG
    g3 = model.elbo_grad(data, 100, 1500, 9000.0)              # ... and the communicator is still usable
    assert abs(g3[0] - lv) <= 1e-12 * abs(lv)
    assert model.elbo(data, 100, 1500, 9000.0)[0] == val
    # status travels in the reduced vector: a non-PD Kuu is reported collectively
    bad = device_model(ctx, o.SVA(sva.kernel, sva.z, sva.m, sva.Lq, jitter=-1.0, centered=sva.centered, mean_const=sva.mean_const))
    with pytest.raises(_ffi.PosDefException):
        bad.elbo(data, 0, 500, 0.0)
    ctx.detach_comm()
    assert ctx.comm_info() == (1, 0)
    assert model.elbo(data, 100, 1500, 9000.0)[0] == val
    for h in (bad, model, data):
        h.free()
    ctx.close()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_group_of_one_device_matches_plain_context(dtype):
    """svgp_group_* (one process driving the GPUs, ncclCommInitAll): upload sharding, replicated model, group elbo and
    value-and-gradient against the plain single-context calls on the same data."""
    for p in (os.path.join(ROOT, "approximategps.jl_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    from approxgp import _ffi
    from helpers import desc_from_oracle, device_model

    x, y, sva, s2 = _problem(False, dtype)
    ctx = _ffi.Context(0)
    model = device_model(ctx, sva, dtype=dtype, sigma2=s2)
    data = _ffi.DeviceData(ctx, x, y, dtype)
    ref, rt = model.elbo(data, 0, None, 12000.0)
    rv, _, rg = model.elbo_grad(data, 200, 2048, 12000.0)
    grp = _ffi.Group([0])
    grp.upload(x, y, dtype)
    desc, keep = desc_from_oracle(sva, dtype=dtype, sigma2=s2)
    grp.create_model(desc, keep)
    val, t = grp.elbo(num_data=12000.0)
    assert val == ref and t.n_points == x.shape[1] and t.kl == rt.kl
    gv, gt, gg = grp.elbo_grad(offs=[200], lens=[2048], num_data=12000.0)
    tol = 1e-12 if dtype == np.float64 else 1e-5
    assert abs(gv - rv) <= tol * abs(rv)
    for k in ("variance", "inv_lengthscale", "z", "m", "Lq"):
        np.testing.assert_allclose(np.asarray(gg[k], dtype=np.float64), np.asarray(rg[k], dtype=np.float64), rtol=tol, atol=tol)
    # RowVecs upload goes through the strided gather
    grp2 = _ffi.Group([0])
    grp2.upload(np.ascontiguousarray(x.T), y, dtype, layout=_ffi.ROWVECS)
    desc, keep = desc_from_oracle(sva, dtype=dtype, sigma2=s2)
    grp2.create_model(desc, keep)
    assert grp2.elbo(num_data=12000.0)[0] == ref
    for h in (grp2, grp, model, data):
        (h.close if hasattr(h, "close") else h.free)()
    ctx.close()


def test_group_member_with_a_bad_window_fails_before_any_collective():
    """one member of a one-process group failing its local checks used to leave the others' all-reduces waiting
    inside the same ncclGroup.  Now every member is validated first: the error comes back, nothing was enqueued, and the
    group is still usable."""
    for p in (os.path.join(ROOT, "approximategps.jl_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    from approxgp import _ffi
    from helpers import desc_from_oracle

    x, y, sva, s2 = _problem(False)
    grp = _ffi.Group([0])
    grp.upload(x, y, np.float64)
    desc, keep = desc_from_oracle(sva, sigma2=s2)
    grp.create_model(desc, keep)
    ref = grp.elbo(num_data=12000.0)[0]
    gref = grp.elbo_grad(offs=[0], lens=[2000], num_data=12000.0)[0]
    with pytest.raises((ValueError, _ffi.SvgpError)):
        grp.elbo(offs=[2900], lens=[500], num_data=12000.0)          # window past the shard
    with pytest.raises((ValueError, _ffi.SvgpError)):
        grp.elbo_grad(offs=[2900], lens=[500], num_data=12000.0)
    with pytest.raises((ValueError, _ffi.SvgpError)):
        grp.elbo_grad(offs=[0], lens=[0], num_data=12000.0)          # empty batch
    assert grp.elbo(num_data=12000.0)[0] == ref
    assert grp.elbo_grad(offs=[0], lens=[2000], num_data=12000.0)[0] == gref
    grp.close()


def test_one_shot_host_entry_keeps_the_collective_matched():
    """svgp_elbo_host on a context with a communicator returned straight away when the model or the upload failed,
    leaving its peers in ncclAllReduce.  It now joins the all-reduce with the failure flag; with a world of one the call
    returns its own error and the communicator stays usable."""
    for p in (os.path.join(ROOT, "approximategps.jl_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import ctypes as C

    import svgp_oracle as o
    from approxgp import _ffi
    from helpers import desc_from_oracle, device_model

    x, y, sva, s2 = _problem(False)
    ctx = _ffi.Context(0)
    ctx.attach_comm(_ffi.comm_unique_id(), 1, 0)
    desc, keep = desc_from_oracle(sva, sigma2=s2)
    lib = ctx.lib
    out, terms = C.c_double(), _ffi.Terms()
    xs, ys = np.ascontiguousarray(x.T.ravel()), np.ascontiguousarray(y)   # ColVecs: point-contiguous
    good = lib.svgp_elbo_host(ctx.h, C.byref(desc), _ffi.COLVECS, x.shape[1], xs.ctypes.data, ys.ctypes.data, 0.0, C.byref(out), C.byref(terms))
    assert good == _ffi.OK
    assert abs(out.value - o.elbo(sva, x, y, sigma2=s2)) <= 1e-8 * abs(out.value)
    desc.kernel = 17                                                      # unsupported family: model creation fails
    rc = lib.svgp_elbo_host(ctx.h, C.byref(desc), _ffi.COLVECS, x.shape[1], xs.ctypes.data, ys.ctypes.data, 0.0, C.byref(out), C.byref(terms))
    assert rc == _ffi.UNSUPPORTED
    desc.kernel = sva.kernel.family
    again = C.c_double()
    assert lib.svgp_elbo_host(ctx.h, C.byref(desc), _ffi.COLVECS, x.shape[1], xs.ctypes.data, ys.ctypes.data, 0.0, C.byref(again), C.byref(terms)) == _ffi.OK
    assert again.value == out.value
    model = device_model(ctx, sva, sigma2=s2)                             # and the collective calls still work
    data = _ffi.DeviceData(ctx, x, y, np.float64)
    assert abs(model.elbo(data, 0, None, 0.0)[0] - out.value) <= 1e-12 * abs(out.value)
    model.free()
    data.free()
    ctx.close()


def _device_count():
    import torch
    return torch.cuda.device_count()   # counting devices does not initialise the GPU in this process


@pytest.mark.skipif(_device_count() < 2, reason="needs two GPUs (the round's test boxes have one): the real RCCL launch, bench.py --gpus 2")
def test_bench_two_gpu_launch_runs_two_rccl_ranks():
    """bench.py --gpus 2 started plainly launches its own two ranks (one per GPU); the line must prove it: rccl_world = 2 from the
    library's communicator, twice the points from the all-reduced terms, and the library's all-reduce agreeing with a
    torch.distributed all-reduce of the ranks' local partial sums.  A small config keeps it short."""
    import json
    import subprocess
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1",
                        "--config", "C2", "--full", "--no-grad", "--no-c5"], capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["n_gpus"] == 2 and line["rccl_world"] == 2
    assert line["n_points_global"] == 2 * 100000
    assert line["value"] is not None and line["value"] > 0
    assert line["collective_check"]["rel_err"] < 1e-12
    # round 4: the N > 1 line is self-contained - rank 0's baseline, parity of its shard and the Kuf figure
    assert line["cpu_baseline"]["value"] > 0 and "rank 0's shard" in line["cpu_baseline"]["scope"]
    assert line["parity"]["ok"] and "svgp_elbo_partial" in line["parity"]["via"]
    assert line["kuf_roofline"]["achieved"] > 0


# ---- two real GPUs: skipped on the one-GPU boxes of this build; the transport-level checks a reader with a
# multi-GPU node can run.  One process per GPU (gloo carries the 128-byte communicator id, the library's own RCCL communicator does
# the arithmetic), and one process driving both GPUs (svgp_group_*, ncclCommInitAll).
def _two_gpu_rank(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      HSA_ENABLE_IPC_MODE_LEGACY="0")
    for p in (os.path.join(ROOT, "approximategps.jl_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)
    import torch.distributed as dist

    import svgp_oracle as o
    from approxgp import _ffi
    from approxgp.distributed import attach_comm_via_torch, shard_range
    from helpers import device_model

    dist.init_process_group("gloo", rank=rank, world_size=world)
    x, y, sva, s2 = _problem(False)
    N = x.shape[1]
    lo, hi = shard_range(N, rank, world)
    ctx = _ffi.Context(rank)                                    # one GPU per rank
    attach_comm_via_torch(ctx)
    assert ctx.comm_info() == (world, rank)
    model = device_model(ctx, sva, sigma2=s2)
    data = _ffi.DeviceData(ctx, x[:, lo:hi], y[lo:hi], np.float64)
    res = {}
    val, t = model.elbo(data, 0, hi - lo, float(N))             # whole data set: one in-library all-reduce
    res["full"] = (val, t.n_points)
    gv, gt, gg = model.elbo_grad(data, 10, 1000, float(N))       # a 1000-point window per rank
    res["grad"] = (gv, gt.n_points, {k: np.asarray(v, dtype=np.float64) for k, v in gg.items() if np.ndim(v)})
    # a bad window on rank 1 only: BOTH ranks get an error back (the failure flag travels in the all-reduce), nobody hangs
    errs = 0
    try:
        model.elbo(data, (hi - lo) - 10 if rank == 1 else 0, 500, float(N))
    except (ValueError, _ffi.SvgpError):
        errs += 1
    try:
        model.elbo_grad(data, (hi - lo) - 10 if rank == 1 else 0, 500, float(N))
    except (ValueError, _ffi.SvgpError):
        errs += 1
    res["errors"] = errs
    res["after"] = model.elbo(data, 0, hi - lo, float(N))[0]     # the communicator is still usable
    # a non-positive-definite Kuu is the same on every rank and is reported collectively
    bad = device_model(ctx, o.SVA(sva.kernel, sva.z, sva.m, sva.Lq, jitter=-1.0))
    try:
        bad.elbo(data, 0, 500, float(N))
        res["posdef"] = False
    except _ffi.PosDefException:
        res["posdef"] = True
    if rank == 0:
        idx = np.concatenate([np.arange(shard_range(N, r, world)[0] + 10, shard_range(N, r, world)[0] + 1010) for r in range(world)])
        ref_full = o.elbo(sva, x, y, sigma2=s2)
        ref_val, ref_g = o.elbo_grad(sva, x[:, idx], y[idx], sigma2=s2, num_data=float(N))
        res["ref"] = (ref_full, ref_val, {k: np.asarray(ref_g[k], dtype=np.float64) for k in ("z", "m", "Lq", "inv_lengthscale")})
    import pickle
    with open(f"{out}.{rank}", "wb") as f:
        pickle.dump(res, f)
    for h in (bad, model, data):
        h.free()
    ctx.close()
    dist.destroy_process_group()


@pytest.mark.skipif(_device_count() < 2, reason="needs two GPUs")
def test_two_processes_two_gpus_library_collective(tmp_path):
    import pickle
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    out = str(tmp_path / "res")
    mp.spawn(_two_gpu_rank, args=(2, port, out), nprocs=2, join=True)
    r = [pickle.load(open(f"{out}.{k}", "rb")) for k in range(2)]
    ref_full, ref_val, ref_g = r[0]["ref"]
    for k in range(2):
        assert r[k]["full"][1] == 3001 and abs(r[k]["full"][0] - ref_full) <= 1e-8 * abs(ref_full)
        assert r[k]["grad"][1] == 2000 and abs(r[k]["grad"][0] - ref_val) <= 1e-8 * abs(ref_val)
        assert r[k]["errors"] == 2 and r[k]["posdef"] and r[k]["after"] == r[k]["full"][0]
        for name in ("m", "Lq", "inv_lengthscale"):
            a = r[k]["grad"][2][name].reshape(ref_g[name].shape, order="F")
            assert np.abs(a - ref_g[name]).max() <= 1e-6 * np.abs(ref_g[name]).max(), name
    # both ranks hold the SAME all-reduced gradient, bit for bit
    for name in r[0]["grad"][2]:
        assert np.array_equal(r[0]["grad"][2][name], r[1]["grad"][2][name]), name


@pytest.mark.skipif(_device_count() < 2, reason="needs two GPUs")
def test_group_of_two_devices_matches_one_context():
    for p in (os.path.join(ROOT, "approximategps.jl_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    from approxgp import _ffi
    from approxgp.distributed import shard_range
    from helpers import desc_from_oracle, device_model

    x, y, sva, s2 = _problem(False)
    N = x.shape[1]
    ctx = _ffi.Context(0)
    model = device_model(ctx, sva, sigma2=s2)
    data = _ffi.DeviceData(ctx, x, y, np.float64)
    ref = model.elbo(data, 0, None, float(N))[0]
    grp = _ffi.Group([0, 1])
    grp.upload(x, y, np.float64)                                # contiguous shards, one per device
    desc, keep = desc_from_oracle(sva, sigma2=s2)
    grp.create_model(desc, keep)
    val, t = grp.elbo(num_data=float(N))
    assert t.n_points == N and abs(val - ref) <= 1e-10 * abs(ref)
    # value and gradient of a window per shard against the same points on one context (two calls summed by hand is not
    # possible for the gradient of a scaled sum: compare with the oracle instead)
    import svgp_oracle as o
    offs, lens = [10, 10], [1000, 1000]
    gv, gt, gg = grp.elbo_grad(offs=offs, lens=lens, num_data=float(N))
    idx = np.concatenate([np.arange(shard_range(N, r, 2)[0] + 10, shard_range(N, r, 2)[0] + 1010) for r in range(2)])
    ref_val, ref_g = o.elbo_grad(sva, x[:, idx], y[idx], sigma2=s2, num_data=float(N))
    assert gt.n_points == 2000 and abs(gv - ref_val) <= 1e-8 * abs(ref_val)
    for name in ("m", "Lq", "inv_lengthscale"):
        a = np.asarray(gg[name], dtype=np.float64).reshape(np.shape(ref_g[name]), order="F")
        assert np.abs(a - np.asarray(ref_g[name])).max() <= 1e-6 * np.abs(np.asarray(ref_g[name])).max(), name
    # one member with a window past its shard: the error comes back before anything is enqueued, the group stays usable
    with pytest.raises((ValueError, _ffi.SvgpError)):
        grp.elbo(offs=[0, 1400], lens=[500, 500], num_data=float(N))
    assert grp.elbo(num_data=float(N))[0] == val
    for h in (grp, model, data):
        (h.close if hasattr(h, "close") else h.free)()
    ctx.close()
