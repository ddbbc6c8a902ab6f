"""Gradient accumulation over micro-batches on the flat arenas: mrfp_grad_accumulate bit for bit against torch's add, FlatSGD
against torch.optim.SGD with stock accumulation, and Trainer(accum_steps=k) against a bitwise yardstick -- a second model from the
same state that runs the passes one by one, clones the gradient arena after each, writes the sum back and makes one step with
gscale = 1 / k.  Eager, checked (dynamic loss scale + clipping), skipped windows, graph mode, list-valued losses (DeepLabV3+
factories) and the bucket path over RCCL at world size 1."""
import contextlib
import io
import os
import re
import sys

import pytest
import torch
import torch.multiprocessing as mp

from mrfp_amd import _lib, synth
from mrfp_amd._lib import call, ptr, stream

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


# ---------------------------------------------------------------------------------------------------------------------
# the kernel
# ---------------------------------------------------------------------------------------------------------------------
def _grid_cap():
    src = open(os.path.join(ROOT, "mrfp_amd", "csrc", "sgd.hip")).read()
    cap = int(re.search(r"constexpr int kArenaCap = (\d+);", src).group(1))
    assert "blocks > mrfp::kArenaCap" in src.split('extern "C" int mrfp_grad_accumulate')[1].split('extern "C"')[0]
    return cap


_SPECIAL = None


def _special_pairs():
    """(acc, g) operand pairs: signed zeros, denormals, infinities, NaN on either side, inf + (-inf), overflow to inf."""
    global _SPECIAL
    if _SPECIAL is None:
        inf, nan, den, big = float("inf"), float("nan"), 1e-41, 3e38
        pairs = [(0.0, -0.0), (-0.0, -0.0), (-0.0, 0.0), (0.0, 0.0), (den, den), (den, -den), (-den, 3e-45), (den, 1.0),
                 (1.17549435e-38, -1.1754942e-38), (inf, 1.0), (-inf, -inf), (1.0, -inf), (inf, -inf), (-inf, inf),
                 (nan, 1.0), (1.0, nan), (nan, inf), (big, big), (-big, -big), (1.0, -1.0)]
        _SPECIAL = (torch.tensor([p[0] for p in pairs], dtype=torch.float32), torch.tensor([p[1] for p in pairs], dtype=torch.float32))
    return _SPECIAL


def _operands(n, seed):
    g = torch.Generator().manual_seed(seed)
    a, b = torch.randn(n, generator=g), torch.randn(n, generator=g) * 3.0
    sa, sb = _special_pairs()
    m = min(n, sa.numel())
    a[:m], b[:m] = sa[:m], sb[:m]                       # at the front ...
    if n >= 2 * sa.numel():
        a[-sa.numel():], b[-sa.numel():] = sa, sb        # ... and in the ragged tail of the last trip
    return a.to(DEV), b.to(DEV)


def _accumulate(acc, g, n, first, off=0):
    call("mrfp_grad_accumulate", ptr(acc) + 4 * off, ptr(g) + 4 * off, n, int(first), stream())


@pytest.mark.parametrize("n", [4, 1028, "cap"])
def test_kernel_adds_bit_for_bit(n):
    cap = _grid_cap()
    if n == "cap":
        n = cap * 256 * 4 + 4 * 1027            # more than one trip of the capped grid, ragged tail
    a, b = _operands(n, seed=n % 1000)
    want = a + b                                 # torch's add on the same device
    acc = a.clone()
    _accumulate(acc, b, n, first=0)
    assert _same_bits(acc, want)
    assert _same_bits(b, _operands(n, seed=n % 1000)[1])         # g is only read
    if n >= 40:
        assert torch.isnan(want).sum() >= 5 and torch.isinf(want).sum() >= 5 and (want == 0).sum() >= 5     # the specials are in
    # first: a bit copy of g -- NaN payloads included -- that does not read acc
    g = b.clone()
    _bits(g)[n // 2] = 0x7FC12345
    _bits(g)[n - 1] = -0x3EDCBB                 # 0xFFC12345: a negative NaN with a payload
    acc = torch.full((n,), float("nan"), device=DEV)
    _accumulate(acc, g, n, first=1)
    assert _same_bits(acc, g)


def test_kernel_on_a_range_leaves_both_sides_untouched():
    off, n, total = 4 * 333, 1028, 4 * 333 + 1028 + 4 * 50
    g = torch.Generator().manual_seed(7)
    a, b = torch.randn(total, generator=g).to(DEV), torch.randn(total, generator=g).to(DEV)
    for first in (0, 1):
        acc = a.clone()
        _accumulate(acc, b, n, first, off=off)
        want = a.clone()
        want[off:off + n] = b[off:off + n] if first else a[off:off + n] + b[off:off + n]
        assert _same_bits(acc, want), first
        assert _same_bits(acc[:off], a[:off]) and _same_bits(acc[off + n:], a[off + n:])      # the sentinels on both sides


def test_device_pointers_are_refused_like_host_ones():
    t = torch.zeros(64, device=DEV)
    for args in ((ptr(t) + 4, ptr(t) + 128, 8, 0), (ptr(t), ptr(t) + 128, 6, 0), (ptr(t), None, 8, 1)):
        with pytest.raises(_lib.MrfpHipError, match="grad_accumulate"):
            call("mrfp_grad_accumulate", *args, stream())


# ---------------------------------------------------------------------------------------------------------------------
# FlatSGD against stock accumulation
# ---------------------------------------------------------------------------------------------------------------------
def test_flat_sgd_windows_match_torch_optim_with_stock_accumulation():
    """The two-Linear toy and tolerance of test_fused_sgd_matches_torch_optim; k = 3, three windows: backward() three times into
    .grad, the gradient divided by 3, torch.optim.SGD + LambdaLR."""
    from mrfp_amd.harness import FlatSGD
    k = 3
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Linear(37, 19), torch.nn.Linear(19, 5))
    ref = torch.nn.Sequential(torch.nn.Linear(37, 19), torch.nn.Linear(19, 5))
    ref.load_state_dict(net.state_dict())
    net = net.to(DEV)
    opt = FlatSGD(net, lr=1e-2, max_iter=10)
    ropt = torch.optim.SGD(ref.parameters(), lr=1e-2, momentum=0.9, weight_decay=5e-4)
    sched = torch.optim.lr_scheduler.LambdaLR(ropt, lr_lambda=lambda it: (1 - it / 10) ** 0.9)
    assert opt.flat_a is None
    for window in range(3):
        ropt.zero_grad()
        for micro in range(k):
            x = torch.randn(11, 37)
            opt.zero_grad()
            net(x.to(DEV)).pow(2).sum().backward()
            if micro < k - 1:
                opt.accumulate(first=micro == 0)
            else:
                opt.accumulate(into_grad=True)
            ref(x).pow(2).sum().backward()              # stock accumulation into .grad
        opt.step(gscale=1.0 / k)
        for q in ref.parameters():
            q.grad.div_(k)
        ropt.step()
        sched.step()
        for p, q in zip(net.parameters(), ref.parameters()):
            torch.testing.assert_close(p.detach().cpu(), q.detach(), rtol=2e-5, atol=1e-6)
    assert opt.it == 3 and opt.flat_a is not None


# ---------------------------------------------------------------------------------------------------------------------
# Trainer against the bitwise yardstick
# ---------------------------------------------------------------------------------------------------------------------
def _mrfp():
    from mrfp_amd import deepv3
    from mrfp_amd.config import cfg
    import json
    spec = json.load(open(os.path.join(HERE, "golden", "state_dict_spec.json")))
    cfg.MODEL.ACT_DTYPE = torch.float32
    m = deepv3.MRFPPlus(19, criterion=torch.nn.CrossEntropyLoss(ignore_index=255))
    m.load_state_dict(synth.synth_state_dict([(k, tuple(s)) for k, s in spec["MRFPPlus"]], seed=0))
    return m.to(DEV).train()


_TOGGLES = [(True, True, True), (False, True, False)]


def _mrfp_batches(size, k=2):
    out = []
    for i in range(k):
        x, y = synth.synth_batch(2, size, size, seed=10 + i)
        noise = {key: v.to(DEV) for key, v in synth.synth_noise(2, seed=20 + i).items()}
        out.append((x.to(DEV), y.to(DEV), _TOGGLES[i % 2], noise))
    return out


def _yardstick_window(tr, passes, k):
    """`tr`: a Trainer with accum_steps = 1 whose arenas are driven by hand.  passes: k callables that run zero_grad + forward +
    backward on tr's model and return the loss.  The gradient arena is cloned after each pass, the sum written back in the order
    ((g1 + g2) + ...) + gk, and ONE step made with gscale = 1 / k."""
    from mrfp_amd import conv
    losses, total = [], None
    for run in passes:
        losses.append(float(run().detach()))
        tr.sync.finish()
        conv.join_wgrad_stream()
        g = tr.opt.flat_g.clone()
        total = g if total is None else total + g
    tr.opt.flat_g.copy_(total)
    tr._opt_step(1.0 / k)
    return losses


@pytest.mark.parametrize("checked", [False, True])
def test_trainer_window_equals_separate_passes_summed(checked):
    from mrfp_amd.deepv3 import InjectedRandom
    from mrfp_amd.harness import Trainer
    kw = dict(loss_scale="dynamic", max_grad_norm=1.0) if checked else {}
    batches = _mrfp_batches(256)
    model = _mrfp()
    tr = Trainer(model, lr=1e-2, accum_steps=2, **kw)
    losses = []
    for i, (x, y, tog, noise) in enumerate(batches):
        assert tr.micro == i
        model.rng = InjectedRandom(tog, noise)
        losses.append(float(tr.step(x, y).detach()))
        if i == 0:                                   # the inner micro-batch stepped nothing
            assert tr.opt.it == 0 and not tr.opt.has_momentum and float(tr.opt.flat_m.abs().max()) == 0.0
    assert tr.micro == 0 and tr.opt.it == 1

    ref = _mrfp()
    tr2 = Trainer(ref, lr=1e-2, **kw)

    def one(x, y, tog, noise):
        def run():
            ref.rng = InjectedRandom(tog, noise)
            return tr2._fwd_bwd(x, y)
        return run
    ref_losses = _yardstick_window(tr2, [one(*b) for b in batches], 2)
    torch.cuda.synchronize()
    assert losses == ref_losses
    assert _same_bits(tr.opt.flat_p, tr2.opt.flat_p) and _same_bits(tr.opt.flat_m, tr2.opt.flat_m)
    assert float(tr.opt.flat_m.abs().max()) > 0.0 and tr2.opt.it == 1
    assert int(model.state_dict()["layer1.0.bn1.num_batches_tracked"]) == 2
    assert torch.equal(model.state_dict()["layer1.0.bn1.running_mean"], ref.state_dict()["layer1.0.bn1.running_mean"])
    if checked:
        assert torch.equal(tr.scaler.state, tr2.scaler.state)            # all eight words of the step state
        info = tr.step_info()
        assert info["taken"] == 1 and info["skipped"] == 0 and info["found_inf"] == 0 and 0.0 < info["grad_norm"] < float("inf")
        assert info["gmul"] <= 0.5 / info["scale"]                       # the mean over the window, clipped to norm 1


def test_a_non_finite_micro_batch_skips_the_whole_window():
    from mrfp_amd.deepv3 import InjectedRandom
    from mrfp_amd.harness import Trainer
    batches = _mrfp_batches(128)
    model = _mrfp()
    tr = Trainer(model, lr=1e-2, accum_steps=2, loss_scale="dynamic")
    p0, m0 = tr.opt.flat_p.clone(), tr.opt.flat_m.clone()
    x, y, tog, noise = batches[0]
    model.rng = InjectedRandom(tog, noise)
    tr.step(x, y)
    tr.opt.flat_a[tr.opt.n // 2 + 1] = float("inf")        # a data value in the partial sum: what an overflowed micro-batch leaves
    x, y, tog, noise = batches[1]
    model.rng = InjectedRandom(tog, noise)
    tr.step(x, y)
    info = tr.step_info()
    assert _same_bits(tr.opt.flat_p, p0) and _same_bits(tr.opt.flat_m, m0)
    assert info["scale"] == 32768.0 and info["skipped"] == 1 and info["taken"] == 0 and info["found_inf"] == 1
    assert tr.opt.it == 1 and tr.micro == 0                  # the schedule advances on a skipped window too


def test_graph_mode_window_matches_eager():
    """The comparison of test_graph_mode_matches_eager with k = 2: four calls on each of two toggle combinations, each of them
    met at both positions of a window, as the warm-up call of its graph and as a replay."""
    from mrfp_amd.deepv3 import InjectedRandom
    from mrfp_amd.harness import Trainer
    a, b = _TOGGLES
    order = [a, a, b, b, a, b, b, a]
    x, y = synth.synth_batch(2, 128, 128, seed=3)
    x, y = x.to(DEV), y.to(DEV)
    noise = {k: v.to(DEV) for k, v in synth.synth_noise(2, seed=4).items()}
    out = []
    for graph in (False, True):
        model = _mrfp()
        tr = Trainer(model, lr=1e-3, accum_steps=2)
        if graph:
            tr.enable_graph()
        losses = []
        for i, tog in enumerate(order):
            assert tr.micro == i % 2
            model.rng = InjectedRandom(tog, noise)
            losses.append(float(tr.step(x, y).detach()))
        sd = model.state_dict()
        out.append((losses, sd["final2.0.weight"].clone(), sd["layer1.0.conv1.weight"].clone(),
                    int(sd["layer1.0.bn1.num_batches_tracked"]), sd["layer1.0.bn1.running_mean"].clone(), tr.opt.it))
    assert out[0][0] == out[1][0], (out[0][0], out[1][0])
    assert torch.equal(out[0][1], out[1][1]) and torch.equal(out[0][2], out[1][2])
    assert out[0][3] == out[1][3] == 8 and torch.equal(out[0][4], out[1][4])
    assert out[0][5] == out[1][5] == 4 and len(tr._graphs) == 2


class _DeepWrap(torch.nn.Module):
    """A network/deepv3.py factory behind the call Trainer makes: returns the factory's [main_loss, aux_loss]."""

    def __init__(self, net):
        super().__init__()
        self.net = net

    def forward(self, img, label, training=True):
        return self.net(img, gts=label, aux_gts=label)


def test_list_valued_losses_deep_mobilenet_window():
    import deepv3_common as dc
    from mrfp_amd import conv
    from mrfp_amd.config import cfg
    from mrfp_amd.harness import Trainer
    from mrfp_amd.network import deepv3, wider_resnet
    name = "DeepMobileNetV3PlusD"
    sd, x, y, keep = dc.case_inputs(name)
    x, y = x.to(DEV), y.to(DEV)
    batches = [(x, y), (x.flip(3).contiguous(), y.flip(2).contiguous())]

    def build():
        crit = torch.nn.CrossEntropyLoss(ignore_index=255)
        with contextlib.redirect_stdout(io.StringIO()):
            m = getattr(deepv3, name)(None, dc.NC, crit, crit)
        m.load_state_dict(sd)
        return _DeepWrap(m.to(DEV)).train()

    cfg.MODEL.ACT_DTYPE = torch.float32
    wider_resnet.DROP_MASKS.injected = {"dsn": keep.reshape(dc.B, -1)}
    try:
        model = build()
        tr = Trainer(model, lr=1e-2, accum_steps=2, loss_weights=(1.0, 0.4))
        losses = [tr.step(bx, by) for bx, by in batches]
        assert all(l.dim() == 0 for l in losses)
        losses = [float(l.detach()) for l in losses]

        ref = build()
        tr2 = Trainer(ref, lr=1e-2)

        def one(bx, by):
            def run():                                # the weighted sum by hand, as tests/test_deepv3_gpu.py adds the two terms
                tr2.opt.zero_grad()
                l1, l2 = ref(bx, by)
                total = l1 + 0.4 * l2
                total.backward()
                return total
            return run
        ref_losses = _yardstick_window(tr2, [one(*b) for b in batches], 2)
        torch.cuda.synchronize()
    finally:
        wider_resnet.DROP_MASKS.injected = None
        conv.backward_failed()
    assert losses == ref_losses                       # l1 + 0.4 * l2 of the same forward pass
    assert _same_bits(tr.opt.flat_p, tr2.opt.flat_p) and _same_bits(tr.opt.flat_m, tr2.opt.flat_m)
    assert float(tr.opt.flat_m.abs().max()) > 0.0 and tr.opt.it == tr2.opt.it == 1
    nbt = [v for k_, v in model.state_dict().items() if k_.endswith("num_batches_tracked")]
    assert nbt and all(int(v) == 2 for v in nbt)


class _Toy(torch.nn.Module):
    def __init__(self, nloss):
        super().__init__()
        self.lin = torch.nn.Linear(6, 4)
        self.nloss = nloss

    def forward(self, img, label, training=True):
        out = self.lin(img)
        terms = [out.pow(2).mean(), out.abs().mean(), out.sum()][:max(1, self.nloss)]
        return terms if self.nloss else terms[0]


def test_loss_weights_must_fit_what_the_model_returns():
    from mrfp_amd.harness import Trainer
    x = torch.randn(3, 6, device=DEV)
    torch.manual_seed(0)
    with pytest.raises(ValueError):
        Trainer(_Toy(0).to(DEV), loss_weights=(1.0,)).step(x, None)          # weights for a scalar loss
    with pytest.raises(ValueError):
        Trainer(_Toy(2).to(DEV), loss_weights=(1.0, 0.4, 0.1)).step(x, None)   # wrong length
    with pytest.raises(ValueError):
        Trainer(_Toy(3).to(DEV), loss_weights=(1.0, 0.4)).step(x, None)
    # the fitting cases: None = all ones, the plain sum; weights applied on the device
    toy = _Toy(2).to(DEV)
    l1, l2 = toy(x, None)
    l1, l2 = l1.detach(), l2.detach()
    assert float(Trainer(toy, lr=0.0, weight_decay=0.0).step(x, None).detach()) == float(l1 + l2)
    assert float(Trainer(toy, lr=0.0, weight_decay=0.0, loss_weights=(1.0, 0.4)).step(x, None).detach()) == float(l1 + 0.4 * l2)
    tr = Trainer(toy, lr=0.0, weight_decay=0.0, loss_weights=[2, 0.5])
    tr.step(x, None)
    t1, t2 = toy(x, None)
    want = torch.autograd.grad(2.0 * t1 + 0.5 * t2, toy.lin.weight)[0]
    torch.testing.assert_close(toy.lin.weight.grad, want, rtol=1e-6, atol=1e-7)


def test_without_accumulation_no_accumulator_is_allocated():
    from mrfp_amd.harness import Trainer
    torch.manual_seed(0)
    tr = Trainer(_Toy(0).to(DEV), lr=1e-2)
    x = torch.randn(3, 6, device=DEV)
    for i in range(3):
        tr.step(x, None)
        assert tr.micro == 0 and tr.opt.it == i + 1
    assert tr.opt.flat_a is None and tr.accum_steps == 1


# ---------------------------------------------------------------------------------------------------------------------
# the bucket path over RCCL, world size 1 (MRFP_FORCE_SYNC=1), in one child process
# ---------------------------------------------------------------------------------------------------------------------
class _Wrap(torch.nn.Module):
    def __init__(self, net):
        super().__init__()
        self.net = net

    def forward(self, x, y, training=True):
        return self.net(x).float().pow(2).mean()


def _resnet18():
    from mrfp_amd.config import cfg
    from mrfp_amd.network import Resnet
    cfg.MODEL.ACT_DTYPE = torch.float32
    torch.manual_seed(0)
    net = Resnet.resnet18(pretrained=False, wt_layer=[0, 0, 4, 4, 0, 0, 0])
    del net.fc, net.avgpool
    return _Wrap(net.to("cuda:0").train())


def _worker_rccl(outdir):
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    from mrfp_amd.harness import Trainer
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT="29787", HSA_ENABLE_IPC_MODE_LEGACY="0")
    torch.cuda.set_device(0)
    g = torch.Generator().manual_seed(100)
    xs = [(torch.rand(2, 3, 64, 64, generator=g) * 255).cuda() for _ in range(2)]
    res = []
    for force in (0, 1):
        if force:
            os.environ["MRFP_FORCE_SYNC"] = "1"
            os.environ["MRFP_SEED"] = "1234"
            dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
        tr = Trainer(_resnet18(), lr=1e-3, bucket_mb=4.0, accum_steps=2)
        assert tr.sync.enabled == bool(force)
        launched = []
        if force:
            real = tr.sync._launch
            tr.sync._launch = lambda b, real=real: (launched.append(b), real(b))[1]
        losses, counts = [], []
        for i in range(4):
            losses.append(float(tr.step(xs[i % 2], None).detach()))
            counts.append(len(launched))
        torch.cuda.synchronize()
        res.append((tr.opt.flat_p.cpu(), tr.opt.flat_m.cpu(), losses, counts, len(tr.sync.buckets), tr.opt.it))
    torch.save(res, os.path.join(outdir, "rccl.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_rccl_single_rank_bucket_path_equals_the_plain_window(tmp_path):
    ctx = mp.get_context("spawn")
    p = ctx.Process(target=_worker_rccl, args=(str(tmp_path),))
    p.start()
    p.join(timeout=600)
    if p.is_alive():
        p.kill()
        p.join()
    assert p.exitcode == 0
    plain, rccl = torch.load(os.path.join(str(tmp_path), "rccl.pt"))
    nb = rccl[4]
    assert nb >= 3 and rccl[3] == [0, nb, nb, 2 * nb]         # no launch in an inner micro-batch, one per bucket at the window's end
    assert plain[5] == rccl[5] == 2 and plain[2] == rccl[2]
    assert _same_bits(plain[0], rccl[0]) and _same_bits(plain[1], rccl[1])
