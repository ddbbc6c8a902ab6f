"""No-GPU checks of gradient accumulation over micro-batches: the C entry point mrfp_grad_accumulate (declared, exported, refuses bad
arguments before any launch), the Trainer's argument checks, and the data-parallel window on two gloo processes with CPU arenas --
no collective during the inner micro-batch, one per bucket during the last, every rank left with the sum over ranks and window."""
import ctypes
import os
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from mrfp_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cdll():
    build.build()
    return _lib.lib()


def test_grad_accumulate_is_declared_and_exported(cdll):
    protos = _lib.parse_header()
    assert "mrfp_grad_accumulate" in protos and hasattr(cdll, "mrfp_grad_accumulate")
    restype, argtypes = protos["mrfp_grad_accumulate"]
    assert restype is ctypes.c_int
    assert _lib.ARG_NAMES["mrfp_grad_accumulate"] == ["acc", "g", "n", "first", "stream"]
    assert len(argtypes) == len(_lib.ARG_NAMES["mrfp_grad_accumulate"]) == 5
    assert argtypes == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p]


def test_grad_accumulate_refuses_bad_arguments(cdll):
    """Through the loaded library, with pointers into a host buffer: every refusal happens before a launch (this machine has no GPU:
    a launch would show as a different error text and code)."""
    buf = ctypes.create_string_buffer(1 << 12)
    p = (ctypes.addressof(buf) + 255) & ~255
    acc, g = p, p + 1024
    good = dict(acc=acc, g=g, n=8, first=0, stream=None)
    names = _lib.ARG_NAMES["mrfp_grad_accumulate"]
    assert names == list(good), names
    for change in (dict(acc=None), dict(g=None), dict(n=0), dict(n=6), dict(acc=acc + 4), dict(g=g + 4), dict(n=-4),
                   dict(acc=None, first=1), dict(n=6, first=1)):
        args = dict(good, **change)
        rc = cdll.mrfp_grad_accumulate(*[args[k] for k in names])
        assert rc == -1 and cdll.mrfp_last_error().startswith(b"grad_accumulate:"), (change, rc, cdll.mrfp_last_error())


def test_trainer_refuses_bad_accumulation_arguments_before_touching_a_device():
    from mrfp_amd.harness import Trainer

    class Untouchable:
        def parameters(self):
            raise AssertionError("the model was touched before the arguments were checked")

    for bad in (0, -1, 1.5, True, "2"):
        with pytest.raises(ValueError):
            Trainer(Untouchable(), accum_steps=bad)
    for bad in ((), (1.0, float("nan")), "x"):
        with pytest.raises(ValueError):
            Trainer(Untouchable(), loss_weights=bad)
    for bad in ((1.0, float("inf")), [1.0, None], 0.4, (True,)):
        with pytest.raises(ValueError):
            Trainer(Untouchable(), loss_weights=bad)
    # good values pass the checks and reach the model
    with pytest.raises(AssertionError):
        Trainer(Untouchable(), accum_steps=4, loss_weights=(1.0, 0.4))


def test_arena_accumulate_on_cpu_arenas_and_lazy_allocation():
    """The host side of FlatArena.accumulate (the gloo path): flat_a appears with the first call, ranges stay ranges, the roles swap."""
    from mrfp_amd.harness import FlatArena
    torch.manual_seed(0)
    arena = FlatArena(torch.nn.Linear(7, 5))
    assert arena.flat_a is None
    g1, g2 = torch.randn(arena.n), torch.randn(arena.n)
    arena.flat_g.copy_(g1)
    arena.accumulate(first=True)
    assert arena.flat_a.shape == arena.flat_g.shape and torch.equal(arena.flat_a, g1)
    arena.flat_g.copy_(g2)
    arena.accumulate(4, 12)
    want = g1.clone()
    want[4:12] += g2[4:12]
    assert torch.equal(arena.flat_a, want)
    arena.accumulate(8, 16, into_grad=True)
    want_g = g2.clone()
    want_g[8:16] += want[8:16]
    assert torch.equal(arena.flat_g, want_g) and torch.equal(arena.flat_a, want)


class TinyNet(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.a = torch.nn.Linear(7, 33)
        self.b = torch.nn.Linear(33, 65)
        self.c = torch.nn.Linear(65, 3)

    def forward(self, x):
        return self.c(torch.relu(self.b(torch.relu(self.a(x))))).pow(2).sum()


def _worker(rank, world, port, outdir):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from mrfp_amd.harness import FlatArena, GradSync
    torch.manual_seed(0)
    net = TinyNet()
    arena = FlatArena(net)
    sync = GradSync(arena, bucket_mb=150 * 4 / (1 << 20))          # 150 floats per bucket: {c.*}, {b.*}, {a.*}
    launched = []
    real = sync._launch
    sync._launch = lambda b: (launched.append(b), real(b))[1]
    torch.manual_seed(100 + rank)
    xs = [torch.randn(5, 7), torch.randn(5, 7)]
    # micro-batch 1 of 2: joins the window, exchanges nothing
    arena.zero_grad()
    sync.begin(reduce=False)
    net(xs[0]).backward()
    scale1 = sync.finish()
    during_first = (list(launched), len(sync.works))
    g1 = arena.flat_g.clone()
    arena.accumulate(first=True)
    # micro-batch 2 of 2: every bucket takes the partial sum, then is reduced once
    arena.zero_grad()
    sync.begin(accum=True)
    net(xs[1]).backward()
    scale2 = sync.finish()
    torch.save({"first": during_first, "launched": launched, "works": len(sync.works), "buckets": len(sync.buckets),
                "scales": (scale1, scale2), "g1": g1, "g": arena.flat_g.clone(), "xs": xs},
               os.path.join(outdir, "a%d.pt" % rank))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_window_one_collective_per_bucket(tmp_path):
    world, port = 2, 29623
    ctx = mp.get_context("spawn")
    procs = [ctx.Process(target=_worker, args=(r, world, port, str(tmp_path))) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    out = [torch.load(os.path.join(str(tmp_path), "a%d.pt" % r)) for r in range(world)]
    for o in out:
        assert o["buckets"] >= 3
        assert o["first"] == ([], 0)                                   # no collective during the first micro-batch
        assert o["launched"] == list(range(o["buckets"])) and o["works"] == o["buckets"]      # exactly one per bucket in the second
        assert o["scales"] == (0.5, 0.5)
    assert torch.equal(out[0]["g"], out[1]["g"])
    # the yardstick, single process: (g1_r0 + g2_r0) + (g1_r1 + g2_r1)
    sys.path.insert(0, ROOT)
    from mrfp_amd.harness import FlatArena
    torch.manual_seed(0)
    net = TinyNet()
    arena = FlatArena(net)
    sums = []
    for r in range(world):
        gs = []
        for x in out[r]["xs"]:
            arena.zero_grad()
            net(x).backward()
            gs.append(arena.flat_g.clone())
        assert torch.equal(gs[0], out[r]["g1"])
        sums.append(gs[0] + gs[1])
    ref = sums[0] + sums[1]
    # to 1 ulp: rtol = 2^-23 (one unit in the last place of a normal fp32), atol = the smallest normal for sums that cancel
    torch.testing.assert_close(out[0]["g"], ref, rtol=2.0 ** -23, atol=2.0 ** -126)
