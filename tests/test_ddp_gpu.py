"""Data-parallel training step on the real GPU path with 2 processes (both on cuda:0, gloo transport -- RCCL
refuses two ranks on one device; the 8-GPU RCCL run is the driver's).  Exercises what changes at world size > 1:
bucket hooks fired by autograd AND by the direct gradient sinks of the HIP backward kernels, the side stream,
the 1/world scale folded into the fused SGD kernel.  Checks: both ranks end with identical parameters, and the
synchronised gradient equals the mean of the two local gradients."""
import os
import sys

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(seed=0):
    sys.path.insert(0, ROOT)
    from mrfp_amd.config import cfg
    from mrfp_amd.network import Resnet
    cfg.MODEL.ACT_DTYPE = torch.float32
    torch.manual_seed(seed)
    net = Resnet.resnet18(pretrained=False, wt_layer=[0, 0, 4, 4, 0, 0, 0])
    del net.fc, net.avgpool
    return net.to("cuda:0").train()


class _Wrap(torch.nn.Module):
    def __init__(self, net):
        super().__init__()
        self.net = net

    def forward(self, x, y, training=True):
        return self.net(x).float().pow(2).mean()


def _worker(rank, world, port, outdir):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sys.path.insert(0, ROOT)
    from mrfp_amd.harness import Trainer
    model = _Wrap(_build(rank))             # DIFFERENT initial weights per rank: Trainer must broadcast rank 0's
    tr = Trainer(model, lr=1e-3, bucket_mb=4.0)
    assert tr.sync.enabled and len(tr.sync.buckets) >= 3
    g = torch.Generator().manual_seed(100 + rank)
    x = (torch.rand(2, 3, 64, 64, generator=g) * 255).cuda()
    # step 1 by hand to look at the synchronised gradient
    tr.opt.zero_grad()
    tr.sync.begin()
    model(x, None).backward()
    scale = tr.sync.finish()
    torch.cuda.synchronize()
    torch.save((tr.opt.flat_g.cpu() * scale, x.cpu()), os.path.join(outdir, "g%d.pt" % rank))
    tr.opt.step(scale)
    loss = tr.step(x, None)            # a full second step through Trainer
    torch.cuda.synchronize()
    torch.save((tr.opt.flat_p.cpu(), float(loss)), os.path.join(outdir, "p%d.pt" % rank))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_gradient_sync_on_gpu(tmp_path):
    world, port = 2, 29733
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_worker, args=(r, world, port, str(tmp_path))) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=600)
        assert p.exitcode == 0
    g = [torch.load(os.path.join(str(tmp_path), "g%d.pt" % r)) for r in range(world)]
    p = [torch.load(os.path.join(str(tmp_path), "p%d.pt" % r)) for r in range(world)]
    assert torch.equal(g[0][0], g[1][0])                       # same averaged gradient on both ranks
    assert torch.equal(p[0][0], p[1][0])                       # replicas stay bit-identical
    # the averaged gradient == mean of the two local gradients (recomputed here, single process)
    sys.path.insert(0, ROOT)
    from mrfp_amd.harness import FlatArena
    model = _Wrap(_build(0))
    arena = FlatArena(model)
    ref = torch.zeros_like(arena.flat_g)
    for r in range(world):
        arena.zero_grad()
        model(g[r][1].cuda(), None).backward()
        ref += arena.flat_g / world
    torch.cuda.synchronize()
    torch.testing.assert_close(g[0][0], ref.cpu(), rtol=1e-4, atol=1e-6)


# ---------------------------------------------------------------------------------------------------------------------
# RCCL itself: one rank, backend nccl, MRFP_FORCE_SYNC=1 -> buckets, side stream, wgrad stream join and the RCCL
# all-reduce kernels all run; the result must equal the plain single-process step bit for bit (a 1-rank sum is x).
# ---------------------------------------------------------------------------------------------------------------------
def _worker_nccl(outdir, force):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT="29741", HSA_ENABLE_IPC_MODE_LEGACY="0")
    if force:
        os.environ["MRFP_FORCE_SYNC"] = "1"
        torch.cuda.set_device(0)
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    sys.path.insert(0, ROOT)
    from mrfp_amd.harness import Trainer
    model = _Wrap(_build(0))
    if force:
        os.environ["MRFP_SEED"] = "1234"            # sync_replicas seeds the torch generators base + rank (rank 0: the base)
    tr = Trainer(model, lr=1e-3, bucket_mb=4.0)       # force: sync_replicas runs its broadcasts over RCCL (world size 1)
    assert tr.sync.enabled == bool(force)
    if force:
        assert torch.initial_seed() == 1234
        ones = torch.ones(1, device="cuda")
        dist.all_reduce(ones)                         # bench.py's `ranks_seen`
        assert int(ones.item()) == 1
    g = torch.Generator().manual_seed(100)
    x = (torch.rand(2, 3, 64, 64, generator=g) * 255).cuda()
    losses = [float(tr.step(x, None)) for _ in range(3)]
    torch.cuda.synchronize()
    torch.save((tr.opt.flat_p.cpu(), losses, len(tr.sync.buckets)), os.path.join(outdir, "n%d.pt" % int(force)))
    if force:
        dist.barrier()
        dist.destroy_process_group()


def test_rccl_single_rank_forced_sync_equals_plain_step(tmp_path):
    ctx = mp.get_context("spawn")
    for force in (0, 1):
        p = ctx.Process(target=_worker_nccl, args=(str(tmp_path), force))
        p.start()
        p.join(timeout=600)
        assert p.exitcode == 0, force
    plain = torch.load(os.path.join(str(tmp_path), "n0.pt"))
    rccl = torch.load(os.path.join(str(tmp_path), "n1.pt"))
    assert rccl[2] >= 3                                        # several buckets went through RCCL
    assert plain[1] == rccl[1] and torch.equal(plain[0], rccl[0])


# ---------------------------------------------------------------------------------------------------------------------
# cross-rank switchable whitening (iw = 5) against the reference's SyncSwitchWhiten2d run by two gloo processes
# (tests/golden/syncsw.npz, tests/golden/make_golden_syncsw.py)
# ---------------------------------------------------------------------------------------------------------------------
def _worker_syncsw(rank, world, port, outdir):
    import numpy as np
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_golden_syncsw as gen                      # seeds / parameter values only (no reference import at module level)
    from mrfp_amd.network.sync_switchwhiten import SyncSwitchWhiten2d
    sw = SyncSwitchWhiten2d(gen.C, num_pergroup=16, sw_type=2, T=5, tie_weight=False, eps=1e-5, momentum=0.99, affine=True).cuda()
    with torch.no_grad():
        for k, v in gen.params().items():
            getattr(sw, k).copy_(v)
    sw.train()
    x, gy = gen.case(rank)
    x = x.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(True)
    y = sw(x)
    y.backward(gy.cuda().contiguous(memory_format=torch.channels_last))
    out = {"y": y, "gx": x.grad, "g_weight": sw.weight.grad, "g_bias": sw.bias.grad, "g_mean_w": sw.sw_mean_weight.grad,
           "g_var_w": sw.sw_var_weight.grad, "running_mean": sw.running_mean, "running_cov": sw.running_cov}
    sw.eval()
    with torch.no_grad():
        out["y_eval"] = sw(x.detach())
    np.savez(os.path.join(outdir, "s%d.npz" % rank), **{k: v.detach().float().cpu().numpy() for k, v in out.items()})
    dist.barrier()
    dist.destroy_process_group()


def test_sync_switch_whiten_two_ranks_vs_reference(tmp_path):
    import numpy as np
    G = np.load(os.path.join(ROOT, "tests", "golden", "syncsw.npz"))
    world, port = 2, 29747
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_worker_syncsw, args=(r, world, port, str(tmp_path))) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=600)
        assert p.exitcode == 0

    def rel(a, b):
        return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))
    tol = {"y": 2e-4, "y_eval": 2e-4, "gx": 2e-3, "g_weight": 2e-3, "g_bias": 2e-4, "g_mean_w": 5e-3, "g_var_w": 5e-3,
           "running_mean": 1e-4, "running_cov": 1e-4}
    for r in range(world):
        z = np.load(os.path.join(str(tmp_path), "s%d.npz" % r))
        for k, t in tol.items():
            assert rel(z[k], G["r%d_%s" % (r, k)]) < t, (r, k, rel(z[k], G["r%d_%s" % (r, k)]))


# ---------------------------------------------------------------------------------------------------------------------
# bench.py --full end to end at world size 2 (the roofline leg used to run on rank 0 only and would have left
# the other ranks' collectives unmatched).  Both ranks share the one GPU, gloo transport.
# ---------------------------------------------------------------------------------------------------------------------
def test_bench_two_ranks_end_to_end():
    import json
    import subprocess
    env = dict(os.environ, MRFP_BENCH_SHARE_GPU="1", MRFP_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29753", os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
           "--trunk", "resnet-50", "--size", "128", "--batch", "2", "--dtype", "bf16", "--full"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1                                      # ONE JSON line, from rank 0
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["config"]["global_batch"] == 4 and out["scaling"] == "weak"
    assert out["value"] > 0 and out["roofline"]["achieved"] > 0 and out["cpu_baseline"] is None
    assert out["ranks_seen"] == 2


def test_bench_gpus_flag_launches_the_ranks_itself():
    """`python bench.py --gpus 2` with no launcher environment (the driver's form of the command): bench.py starts the two
    ranks as a child torch.distributed.run BEFORE touching the GPU and relays rank 0's single JSON line; `ranks_seen` is an
    all-reduce of ones over the data-path group."""
    import json
    import subprocess
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(MRFP_BENCH_SHARE_GPU="1", MRFP_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
           "--trunk", "resnet-50", "--size", "128", "--batch", "2", "--dtype", "bf16"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["ranks_seen"] == 2 and out["config"]["global_batch"] == 4
    assert out["value"] > 0 and out["cpu_baseline"] is None


def test_four_rank_rehearsal_on_the_one_gpu():
    """The widest rehearsal this pool allows on the card: at most six processes may hold the GPU at once, and the test runner,
    the launcher and the rendezvous agent count (a six-rank attempt was killed by the box's process guard with 8 holders), so
    four ranks.  The eight-rank launch itself is rehearsed on the CPU (tests/test_ddp_cpu.py::
    test_eight_rank_launch_rehearsal_on_cpu).  `python bench.py --gpus 4` in the driver's form -- bench.py starts the ranks
    itself -- with every rank on cuda:0 over gloo: shows what two ranks cannot -- the rendezvous of more than two processes, port
    handling, OMP_NUM_THREADS under oversubscription, four HIP contexts with eight hardware queues each on one device."""
    import json
    import subprocess
    import time
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(MRFP_BENCH_SHARE_GPU="1", MRFP_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4", "--steps", "2", "--warmup", "1",
           "--trunk", "resnet-50", "--size", "64", "--batch", "2", "--dtype", "bf16"]
    t0 = time.time()
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    wall = time.time() - t0
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["n_gpus"] == 4 and out["ranks_seen"] == 4 and out["config"]["global_batch"] == 8
    assert out["value"] > 0 and wall < 300, wall


# ---------------------------------------------------------------------------------------------------------------------
# cfg.MODEL.SYNC_BN (reference config.py:105-107: torch.nn.SyncBatchNorm when args.syncbn): BatchNorm statistics over the
# batches of all ranks.  Two ranks with two images each against ONE process with the four images: forward output, running
# statistics, input gradient; the weight / bias gradients are each rank's LOCAL sums (the data-parallel exchange averages
# them), so they add up to the single-process gradient.  Also through a residual tail (sign-mask path) and a conv epilogue
# that produced the statistics.
# ---------------------------------------------------------------------------------------------------------------------
def _syncbn_case(device, dtype=torch.float32):
    g = torch.Generator().manual_seed(5)
    x = torch.randn(4, 64, 10, 12, generator=g)
    res = torch.randn(4, 64, 10, 12, generator=g)
    gy = torch.randn(4, 64, 10, 12, generator=g)
    w, b = torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g) * 0.1
    cw = torch.randn(64, 64, 1, 1, generator=g) * 0.1
    to = lambda t: t.to(device, dtype).contiguous(memory_format=torch.channels_last)
    return to(x), to(res), to(gy), w.to(device), b.to(device), cw.to(device)


def _syncbn_run(sl, sync):
    sys.path.insert(0, ROOT)
    from mrfp_amd import conv, ops
    from mrfp_amd.config import cfg
    cfg.MODEL.SYNC_BN = sync
    x, res, gy, w, b, cw = _syncbn_case("cuda:0")
    out = {}
    for name, use_res, through_conv in (("plain", False, False), ("res", True, False), ("conv", False, True)):
        xs = x[sl].detach().clone().requires_grad_(True)
        ws, bs = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
        rm, rv = torch.zeros(64, device="cuda:0"), torch.ones(64, device="cuda:0")
        h = conv.conv2d(xs, cw, None, 1, 0, 1) if through_conv else xs       # (1x1 conv: its epilogue carries the statistics)
        y = ops.batch_norm_act(h, ws, bs, rm, rv, training=True, relu=True, res=res[sl] if use_res else None)
        y.backward(gy[sl])
        out[name] = {k: v.detach().float().cpu() for k, v in (("y", y), ("dx", xs.grad), ("dw", ws.grad), ("db", bs.grad), ("rm", rm), ("rv", rv))}
    cfg.MODEL.SYNC_BN = False
    return out


def _worker_syncbn(rank, world, port, outdir):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sys.path.insert(0, ROOT)
    from mrfp_amd import ops
    before = ops.SYNC_BN_CALLS[0]
    out = _syncbn_run(slice(2 * rank, 2 * rank + 2), True)
    assert ops.SYNC_BN_CALLS[0] - before == 6          # forward + backward of the three layers
    torch.save(out, os.path.join(outdir, "sbn%d.pt" % rank))
    dist.barrier()
    dist.destroy_process_group()


def test_sync_batchnorm_two_ranks_equal_one_process_on_the_whole_batch(tmp_path):
    world, port = 2, 29761
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_worker_syncbn, args=(r, world, port, str(tmp_path))) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=600)
        assert p.exitcode == 0
    full = _syncbn_run(slice(0, 4), False)              # one process, all four images, no process group
    parts = [torch.load(os.path.join(str(tmp_path), "sbn%d.pt" % r)) for r in range(world)]

    def rel(a, b):
        return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))
    for name in ("plain", "res", "conv"):
        f = full[name]
        for r in range(world):
            sl = slice(2 * r, 2 * r + 2)
            assert rel(parts[r][name]["y"], f["y"][sl]) < 2e-5, (name, r, "y")
            assert rel(parts[r][name]["dx"], f["dx"][sl]) < 5e-5, (name, r, "dx")
            assert rel(parts[r][name]["rm"], f["rm"]) < 1e-5 and rel(parts[r][name]["rv"], f["rv"]) < 1e-5, (name, r, "running")
        assert rel(parts[0][name]["dw"] + parts[1][name]["dw"], f["dw"]) < 5e-5, (name, "dw")
        assert rel(parts[0][name]["db"] + parts[1][name]["db"], f["db"]) < 5e-5, (name, "db")
        # and per-replica statistics (the default) do NOT give the whole-batch result: the option changes something
    sys.path.insert(0, ROOT)
    local = _syncbn_run(slice(0, 2), False)
    assert rel(local["plain"]["y"], full["plain"]["y"][0:2]) > 1e-3


def _worker_syncbn_uneven(rank, world, port, outdir):
    """a rank whose batch shrinks for one step (a partial last batch) while this one's does not leaves this rank's cached
    global count stale.  Every synchronised layer compares the all-reduced count with the cached one ON THE DEVICE; sync_bn_poll()
    reports it (here: blocking) -- on the rank whose cache went stale, every time, not on one use in 512."""
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sys.path.insert(0, ROOT)
    from mrfp_amd import _lib, ops
    _syncbn_run(slice(2 * rank, 2 * rank + 2), True)                 # even step: counts cached (2 images per rank)
    ops.sync_bn_poll(block=True)                                      # nothing to report
    _syncbn_run(slice(0, 2) if rank == 0 else slice(2, 3), True)      # rank 1 runs ONE image
    raised = False
    try:
        ops.sync_bn_poll(block=True)
    except _lib.MrfpHipError as e:
        raised = "uneven per-rank batches" in str(e)
    # rank 0's key (2 images) was cached with the even total: stale now -> reported; rank 1's key (1 image) is new -> read back fresh
    assert raised == (rank == 0), (rank, raised)
    # the non-blocking form: first call starts the read-back, a later one reports
    _syncbn_run(slice(0, 2) if rank == 0 else slice(2, 3), True)
    late = False
    try:
        ops.sync_bn_poll()
        torch.cuda.synchronize()
        ops.sync_bn_poll()
    except _lib.MrfpHipError:
        late = True
    assert late == (rank == 0), (rank, late)
    open(os.path.join(outdir, "uneven%d.ok" % rank), "w").write("ok")
    dist.barrier()
    dist.destroy_process_group()


def test_sync_batchnorm_reports_an_uneven_step_from_the_device_side_check(tmp_path):
    world, port = 2, 29773
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_worker_syncbn_uneven, args=(r, world, port, str(tmp_path))) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=600)
        assert p.exitcode == 0
    assert all(os.path.exists(os.path.join(str(tmp_path), "uneven%d.ok" % r)) for r in range(world))


def _worker_syncbn_rccl(outdir):
    """cfg.MODEL.SYNC_BN over RCCL itself (backend "nccl", world size 1 forced with MRFP_FORCE_SYNC=1 -- RCCL refuses two ranks on
    one device): the statistics' own communicator (dist.new_group), its float64 all-reduce on the device, the cached global
    count (no host synchronisation after the first call of a shape)."""
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT="29767", HSA_ENABLE_IPC_MODE_LEGACY="0", MRFP_FORCE_SYNC="1")
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    sys.path.insert(0, ROOT)
    from mrfp_amd import ops
    before = ops.SYNC_BN_CALLS[0]
    out = _syncbn_run(slice(0, 4), True)
    again = _syncbn_run(slice(0, 4), True)
    assert ops.SYNC_BN_CALLS[0] - before == 12 and ops._SYNC_BN_GROUP[0] is not None and ops._SYNC_BN_GROUP[0] is not dist.group.WORLD
    assert list(ops._SYNC_BN_COUNTS.values()) == [4 * 10 * 12]          # one cached count: read back once
    for name in out:
        for k in out[name]:
            assert torch.equal(out[name][k], again[name][k]), (name, k)
    torch.save(out, os.path.join(outdir, "sbn_rccl.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_sync_batchnorm_over_rccl_at_world_size_one(tmp_path):
    ctx = mp.get_context("spawn")
    p = ctx.Process(target=_worker_syncbn_rccl, args=(str(tmp_path),))
    p.start()
    p.join(timeout=600)
    assert p.exitcode == 0
    full = _syncbn_run(slice(0, 4), False)
    got = torch.load(os.path.join(str(tmp_path), "sbn_rccl.pt"))
    for name in ("plain", "res", "conv"):
        for k in ("y", "dx", "dw", "db", "rm", "rv"):
            a, b = got[name][k], full[name][k]
            assert float((a - b).abs().max() / b.abs().max().clamp_min(1e-30)) < 5e-5, (name, k)


def _worker_local_bn_never_syncs(outdir):
    """Set up as _worker_syncbn_rccl: the process group is up and cfg.MODEL.SYNC_BN is on.  ops.local_batch_norm_act (the plain
    nn.BatchNorm2d of MobileNetV2) exchanges nothing in forward or backward; the same layer through ops.batch_norm_act does."""
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT="29779", HSA_ENABLE_IPC_MODE_LEGACY="0", MRFP_FORCE_SYNC="1")
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    sys.path.insert(0, ROOT)
    from mrfp_amd import ops
    from mrfp_amd.config import cfg
    cfg.MODEL.SYNC_BN = True
    x, _, gy, w, b, _ = _syncbn_case("cuda:0")
    for fn, expect in ((ops.local_batch_norm_act, 0), (ops.batch_norm_act, 2)):
        xs = x.detach().clone().requires_grad_(True)
        ws, bs = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
        rm, rv = torch.zeros(64, device="cuda:0"), torch.ones(64, device="cuda:0")
        before = ops.SYNC_BN_CALLS[0]
        fn(xs, ws, bs, rm, rv, training=True).backward(gy)
        torch.cuda.synchronize()
        assert ops.SYNC_BN_CALLS[0] - before == expect, (fn.__name__, ops.SYNC_BN_CALLS[0] - before)
        if expect == 0:
            assert ops._SYNC_BN_GROUP[0] is None          # the statistics' communicator was not even created
    cfg.MODEL.SYNC_BN = False
    open(os.path.join(outdir, "local_bn.ok"), "w").write("ok")
    dist.barrier()
    dist.destroy_process_group()


def test_local_batch_norm_never_synchronises_with_sync_bn_on(tmp_path):
    ctx = mp.get_context("spawn")
    p = ctx.Process(target=_worker_local_bn_never_syncs, args=(str(tmp_path),))
    p.start()
    p.join(timeout=600)
    assert p.exitcode == 0
    assert os.path.exists(os.path.join(str(tmp_path), "local_bn.ok"))
