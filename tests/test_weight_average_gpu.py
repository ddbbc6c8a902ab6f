"""Weight averaging inside the fused SGD step: mrfp_sgd_step_avg / mrfp_sgd_step_checked_avg bit for bit against the plain step
kernels (p, m) and against torch's `e + c * (p - e)` on the same device (e), the device's coefficient against
harness.average_coefficient, mrfp_arena_swap, and Trainer(average=...) -- eager, accumulation windows, skipped windows, graph mode,
averaged() on the small MRFP model, resume from a checkpoint -- and harness.update_bn against per-batch statistics in float64."""
import contextlib
import io
import json
import os
import re

import pytest
import torch

from mrfp_amd import _lib, synth
from mrfp_amd._lib import call, ptr, stream
from mrfp_amd.harness import (Trainer, WeightAverage, average_coefficient, average_index, evaluate, load_checkpoint, save_checkpoint,
                              update_bn)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
KIND = {"ema": 0, "swa": 1}
LR, MU, WD, GS = 0.05, 0.9, 5e-4, 0.5


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _grid_cap():
    src = open(os.path.join(ROOT, "mrfp_amd", "csrc", "sgd.hip")).read()
    cap = int(re.search(r"constexpr int kArenaCap = (\d+);", src).group(1))
    assert "blocks > kArenaCap ? kArenaCap" in src and src.count("mrfp::arena_blocks(n)") == 3      # the three new launches are capped
    return cap


# signed zeros and denormals (no inf / NaN: p, g, m stay finite), in the four roles p, g, m, e
_SPECIAL = torch.tensor([[0.0, -0.0, 0.0, -0.0], [-0.0, 0.0, -0.0, 0.0], [-0.0, -0.0, -0.0, -0.0], [1e-41, -1e-41, 3e-45, 1e-41],
                         [1e-41, 1e-41, -1e-41, -3e-45], [-3e-45, 1e-41, 1e-41, 1.0], [1.17549435e-38, -1.1754942e-38, 1e-39, 1e-41],
                         [1.0, -0.0, 1e-41, 1.0], [-2.5, 1e-41, -0.0, -2.5], [0.0, 0.0, 0.0, 1e-41]], dtype=torch.float32).t().contiguous()


def _operands(n, seed):
    """p, g, m, e on the device with the specials at the front and, when they fit twice, in the ragged tail of the last trip."""
    gen = torch.Generator().manual_seed(seed)
    ts = [torch.randn(n, generator=gen) * s for s in (1.0, 3.0, 0.5, 1.0)]
    k = _SPECIAL.shape[1]
    for t, sp in zip(ts, _SPECIAL):
        t[:min(n, k)] = sp[:min(n, k)]
        if n >= 2 * k:
            t[-k:] = sp
    return [t.to(DEV) for t in ts]


def _rule(kind="ema", decay=0.999, warmup=True, start=1, every=1):
    return (KIND[kind], float(decay), int(warmup), start, every)


def _step_avg(p, g, m, e, n, first, rule, t, off=0, lr=LR, wd=WD, gs=GS):
    call("mrfp_sgd_step_avg", ptr(p) + 4 * off, ptr(g) + 4 * off, ptr(m) + 4 * off, ptr(e) + 4 * off, n, lr, MU, wd, gs, int(first),
         *rule, t, stream())


def _step(p, g, m, n, first, off=0):
    call("mrfp_sgd_step", ptr(p) + 4 * off, ptr(g) + 4 * off, ptr(m) + 4 * off, n, LR, MU, WD, GS, int(first), stream())


def _state(found_inf, gmul, taken):
    w = torch.zeros(8, dtype=torch.int32)
    w.view(torch.float32)[0] = 1.0
    w.view(torch.float32)[4] = gmul
    w[2], w[5] = found_inf, taken
    return w.to(DEV)


def _lerp(e, p, c):
    return e + c * (p - e)                      # torch on the same device: three rounded operations


# (name, rule, t, n): the step count t lands on update n of the rule (None: off the period)
_CASES = [("copy", _rule("ema", 0.999, True, 5, 2), 5, 0),
          ("ema3_warmup", _rule("ema", 0.999, True, 1, 1), 4, 3),
          ("ema20000", _rule("ema", 0.999, True, 1, 1), 20001, 20000),
          ("swa7", _rule("swa", 0.999, True, 2, 3), 23, 7),
          ("off_period", _rule("swa", 0.999, True, 2, 3), 24, None),
          ("before_start", _rule("ema", 0.9, False, 7, 1), 6, None)]
_KINDNAME = {0: "ema", 1: "swa"}


# ---------------------------------------------------------------------------------------------------------------------
# 1. the unchecked kernel
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4, 1028, "cap"])
def test_step_avg_matches_the_plain_step_and_torch_bit_for_bit(n):
    cap = _grid_cap()
    if n == "cap":
        n = cap * 256 * 4 + 4 * 1027             # more than one trip of the capped grid, ragged tail
    p0, g0, m0, e0 = _operands(n, seed=n % 1000)
    nan = torch.full((n,), float("nan"), device=DEV)
    _bits(nan)[n // 2] = 0x7FC12345              # a payload: "untouched" means these bits
    for first in (0, 1):
        pr, mr = p0.clone(), m0.clone()
        _step(pr, g0, mr, n, first)              # the yardstick for p and m, once per `first`
        if n >= 40:
            assert (pr == 0).sum() >= 2 and ((pr != 0) & (pr.abs() < 1.1754944e-38)).sum() >= 2        # the specials are in
        for name, rule, t, idx in _CASES:
            assert average_index(t, rule[3], rule[4]) == idx, name
            p, g, m = p0.clone(), g0.clone(), m0.clone()
            e = e0.clone() if idx else nan.clone()        # copy / no update: e is pre-filled with NaN
            _step_avg(p, g, m, e, n, first, rule, t)
            assert _same_bits(p, pr) and _same_bits(m, mr), (name, first)
            assert _same_bits(g, g0), (name, first)
            if idx is None:
                assert _same_bits(e, nan), (name, first)          # neither read nor written
            elif idx == 0:
                assert _same_bits(e, pr), (name, first)           # a bit copy of the new parameters
            else:
                c = average_coefficient(_KINDNAME[rule[0]], idx, rule[1], bool(rule[2]))
                assert _same_bits(e, _lerp(e0, pr, c)), (name, first, c)
                assert not _same_bits(e, e0)


# ---------------------------------------------------------------------------------------------------------------------
# 2. the coefficient on the device
# ---------------------------------------------------------------------------------------------------------------------
def test_device_coefficient_equals_average_coefficient():
    """lr = wd = 0, g = 0, p = 1, e = 0: p stays 1 and e comes out as 0 + c * (1 - 0) = c itself."""
    one, zero = torch.ones(4, device=DEV), torch.zeros(4, device=DEV)
    got, want = [], []
    for kind in ("ema", "swa"):
        for warmup in (True, False):
            for n in (1, 2, 3, 8, 9, 10, 100, 8989, 8990, 8991, 10 ** 6):
                p, g, m, e = one.clone(), zero.clone(), zero.clone(), zero.clone()
                _step_avg(p, g, m, e, 4, 0, _rule(kind, 0.999, warmup), n + 1, lr=0.0, wd=0.0, gs=1.0)
                assert _same_bits(p, one)
                got.append(e)
                want.append(average_coefficient(kind, n, 0.999, warmup))
    got = torch.stack(got).cpu()
    want = torch.tensor(want, dtype=torch.float64)
    assert torch.equal(got.double(), want[:, None].expand(-1, 4)), (got[:, 0].tolist(), want.tolist())
    assert len(set(want.tolist())) >= 11          # (the eleven swa values alone are distinct: the cases do not collapse into one)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the checked kernel
# ---------------------------------------------------------------------------------------------------------------------
def _step_checked_avg(p, g, m, e, n, st, base, rule, off=0):
    call("mrfp_sgd_step_checked_avg", ptr(p) + 4 * off, ptr(g) + 4 * off, ptr(m) + 4 * off, ptr(e) + 4 * off, n, LR, MU, WD, ptr(st),
         base, *rule, stream())


def test_checked_step_avg_obeys_the_step_state():
    n = 4 * 1027
    p0, g0, m0, e0 = _operands(n, seed=5)
    rule = _rule("ema", 0.9, False, 1, 1)
    # found_inf: nothing at all is written (t = 3 would update)
    st = _state(1, 0.25, 5)
    p, m, e = p0.clone(), m0.clone(), e0.clone()
    _step_checked_avg(p, g0, m, e, n, st, -2, rule)
    assert _same_bits(p, p0) and _same_bits(m, m0) and _same_bits(e, e0)
    # taken = 5, taken_base = -2: t = 3 on the device
    st = _state(0, 0.25, 5)
    pr, mr = p0.clone(), m0.clone()
    call("mrfp_sgd_step_checked", ptr(pr), ptr(g0), ptr(mr), n, LR, MU, WD, ptr(st), stream())
    assert not _same_bits(pr, p0)
    for rule, idx in ((_rule("ema", 0.9, False, 1, 1), 2), (_rule("swa", 0.9, False, 1, 2), 1), (_rule("ema", 0.9, True, 3, 4), 0),
                      (_rule("ema", 0.9, False, 2, 2), None), (_rule("swa", 0.9, False, 4, 1), None)):
        assert average_index(3, rule[3], rule[4]) == idx
        p, g, m, e = p0.clone(), g0.clone(), m0.clone(), e0.clone()
        _step_checked_avg(p, g, m, e, n, st, -2, rule)
        assert _same_bits(p, pr) and _same_bits(m, mr) and _same_bits(g, g0), rule
        if idx is None:
            assert _same_bits(e, e0), rule
        elif idx == 0:
            assert _same_bits(e, pr), rule
        else:
            assert _same_bits(e, _lerp(e0, pr, average_coefficient(_KINDNAME[rule[0]], idx, rule[1], bool(rule[2])))), rule
    assert torch.equal(st.cpu(), _state(0, 0.25, 5).cpu())            # the state is only read


# ---------------------------------------------------------------------------------------------------------------------
# 4. ranges
# ---------------------------------------------------------------------------------------------------------------------
def test_kernels_on_a_range_leave_both_sides_untouched():
    off, n, total = 4 * 333, 1028, 4 * 333 + 1028 + 4 * 50
    p0, g0, m0, e0 = _operands(total, seed=7)
    rule = _rule("ema", 0.9, False, 1, 1)
    pr, mr = p0.clone(), m0.clone()
    _step(pr, g0, mr, n, 0, off=off)
    want_e = e0.clone()
    want_e[off:off + n] = _lerp(e0, pr, average_coefficient("ema", 3, 0.9, False))[off:off + n]

    def check(p, m, e):
        for got, want, orig in ((p, pr, p0), (m, mr, m0), (e, want_e, e0)):
            assert _same_bits(got, want)
            assert _same_bits(got[:off], orig[:off]) and _same_bits(got[off + n:], orig[off + n:])      # the sentinels on both sides
    p, m, e = p0.clone(), m0.clone(), e0.clone()
    _step_avg(p, g0, m, e, n, 0, rule, 4, off=off)
    check(p, m, e)
    p, m, e = p0.clone(), m0.clone(), e0.clone()
    _step_checked_avg(p, g0, m, e, n, _state(0, GS, 7), -3, rule, off=off)         # gmul = the unchecked call's gscale, t = 4
    check(p, m, e)
    a, b = p0.clone(), e0.clone()
    call("mrfp_arena_swap", ptr(a) + 4 * off, ptr(b) + 4 * off, n, stream())
    wa, wb = p0.clone(), e0.clone()
    wa[off:off + n], wb[off:off + n] = e0[off:off + n], p0[off:off + n]
    assert _same_bits(a, wa) and _same_bits(b, wb)


# ---------------------------------------------------------------------------------------------------------------------
# 5. refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_every_refusal_names_its_entry_point_and_leaves_the_arenas_alone():
    n = 64
    p, g, m, e = _operands(n, seed=9)
    st = _state(0, 1.0, 1)
    keep = [t.clone() for t in (p, g, m, e, st)]
    good = dict(p=ptr(p), g=ptr(g), m=ptr(m), e=ptr(e), n=n, lr=LR, momentum=MU, weight_decay=WD, gscale=1.0, first=0, state=ptr(st),
                taken_base=0, kind=0, decay=0.999, warmup=1, start=1, every=1, t=1, stream=None)
    bad = [dict(p=None), dict(g=None), dict(m=None), dict(e=None), dict(p=ptr(p) + 4), dict(g=ptr(g) + 8), dict(m=ptr(m) + 4),
           dict(e=ptr(e) + 4), dict(n=6), dict(n=0), dict(decay=0.0), dict(decay=1.0), dict(decay=float("nan")), dict(start=0),
           dict(every=0), dict(kind=2), dict(kind=-1)]
    for name in ("mrfp_sgd_step_avg", "mrfp_sgd_step_checked_avg"):
        names = _lib.ARG_NAMES[name]
        extra = [dict(state=None), dict(state=ptr(st) + 4)] if "state" in names else []
        for change in bad + extra:
            args = dict(good, stream=stream(), **change)
            with pytest.raises(_lib.MrfpHipError, match=name[len("mrfp_"):] + ":"):
                call(name, *[args[k] for k in names])
    torch.cuda.synchronize()
    for t, k in zip((p, g, m, e, st), keep):
        assert _same_bits(t, k)


# ---------------------------------------------------------------------------------------------------------------------
# 6. mrfp_arena_swap
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4, 1028, "cap"])
def test_arena_swap_exchanges_bits(n):
    if n == "cap":
        n = _grid_cap() * 256 * 4 + 4 * 1027
    a0, b0, _, _ = _operands(n, seed=3)
    _bits(a0)[0] = 0x7FC12345                    # NaN payloads on both sides, one of them negative
    _bits(b0)[n - 1] = -0x3EDCBB
    _bits(b0)[1] = 0x7F800001                    # a signalling NaN
    a, b = a0.clone(), b0.clone()
    call("mrfp_arena_swap", ptr(a), ptr(b), n, stream())
    assert _same_bits(a, b0) and _same_bits(b, a0)
    call("mrfp_arena_swap", ptr(a), ptr(b), n, stream())
    assert _same_bits(a, a0) and _same_bits(b, b0)          # twice is the identity


def test_arena_swap_refuses_overlap_and_bad_arguments():
    t = torch.arange(256, dtype=torch.float32, device=DEV)
    keep = t.clone()
    for a, b, n in ((ptr(t), ptr(t), 64), (ptr(t), ptr(t) + 16, 64), (ptr(t) + 128, ptr(t), 64), (ptr(t), ptr(t) + 4 * 63 + 4, 128),
                    (None, ptr(t), 8), (ptr(t), None, 8), (ptr(t) + 4, ptr(t) + 512, 8), (ptr(t), ptr(t) + 512, 6)):
        with pytest.raises(_lib.MrfpHipError, match="arena_swap:"):
            call("mrfp_arena_swap", a, b, n, stream())
    with pytest.raises(_lib.MrfpHipError, match="overlap"):
        call("mrfp_arena_swap", ptr(t), ptr(t) + 16, 64, stream())
    call("mrfp_arena_swap", ptr(t), ptr(t) + 4 * 64, 64, stream())          # adjacent ranges are fine
    assert torch.equal(t[:64], keep[64:128]) and torch.equal(t[64:128], keep[:64]) and torch.equal(t[128:], keep[128:])


# ---------------------------------------------------------------------------------------------------------------------
# 7.-9., 12., 14. Trainer on the two-Linear toy
# ---------------------------------------------------------------------------------------------------------------------
class _Toy(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.net = torch.nn.Sequential(torch.nn.Linear(37, 19), torch.nn.Linear(19, 5))

    def forward(self, img, label, training=True):
        return self.net(img).pow(2).mean()


def _toy():
    torch.manual_seed(0)
    return _Toy().to(DEV)


def _toy_inputs(k):
    gen = torch.Generator().manual_seed(11)
    return [torch.randn(11, 37, generator=gen).to(DEV) for _ in range(k)]


def test_default_trainer_is_untouched():
    tr = Trainer(_toy(), lr=1e-2)
    tr.step(_toy_inputs(1)[0], None)
    assert tr.opt.flat_e is None and tr.opt.average is None and tr.opt.taken_base == 0


def test_trainer_ema_equals_the_host_model_and_does_not_perturb_training():
    avg = WeightAverage("ema", decay=0.9, warmup=False, start=2, every=2)
    tr, ref = Trainer(_toy(), lr=1e-2, max_iter=10, average=avg), Trainer(_toy(), lr=1e-2, max_iter=10)
    assert _same_bits(tr.opt.flat_p, ref.opt.flat_p) and float(tr.opt.flat_e.abs().max()) == 0.0
    with pytest.raises(_lib.MrfpHipError):
        with tr.averaged():                      # before any update has happened
            pass
    e = torch.zeros_like(ref.opt.flat_p)
    for t, x in enumerate(_toy_inputs(6), start=1):
        la, lb = tr.step(x, None), ref.step(x, None)
        assert float(la.detach()) == float(lb.detach())
        assert _same_bits(tr.opt.flat_p, ref.opt.flat_p) and _same_bits(tr.opt.flat_m, ref.opt.flat_m), t
        idx = average_index(t, 2, 2)
        if idx == 0:
            e = ref.opt.flat_p.clone()
        elif idx:
            e = _lerp(e, ref.opt.flat_p, average_coefficient("ema", idx, 0.9, False))
        assert _same_bits(tr.opt.flat_e, e), t
        assert tr.average_info()["t"] == t
    info = tr.average_info()
    assert info["n_averaged"] == 3 and info["kind"] == "ema" and info["start"] == 2 and info["every"] == 2
    assert float(tr.opt.flat_e.abs().max()) > 0.0 and not _same_bits(tr.opt.flat_e, tr.opt.flat_p)


def test_swa_is_the_mean_of_the_iterates():
    """|flat_e - mean64(p_1 .. p_5)| <= 16 * 2^-24 * max|p|: three roundings per update, five updates, each at most half an ulp of a
    value no larger than max|p| -- derived, not measured."""
    tr = Trainer(_toy(), lr=5e-2, max_iter=10, average="swa")
    snaps = []
    for x in _toy_inputs(5):
        tr.step(x, None)
        snaps.append(tr.opt.flat_p.double())
    mean = torch.stack(snaps).mean(0)
    bound = 16 * 2.0 ** -24 * float(torch.stack(snaps).abs().max())
    err = float((tr.opt.flat_e.double() - mean).abs().max())
    print("swa: max |e - mean| = %.3e, bound %.3e" % (err, bound))
    assert err <= bound
    assert float((snaps[0] - snaps[4]).abs().max()) > 100 * bound          # the iterates differ by far more than the bound
    assert tr.average_info()["n_averaged"] == 5


def test_accumulation_windows_make_one_update_each():
    tr = Trainer(_toy(), lr=1e-2, max_iter=10, accum_steps=2, average="swa")
    xs = _toy_inputs(4)
    ps = []
    for i, x in enumerate(xs):
        tr.step(x, None)
        assert tr.average_info()["n_averaged"] == (i + 1) // 2
        if i % 2:
            ps.append(tr.opt.flat_p.clone())
    assert tr.average_info() == {"t": 2, "n_averaged": 2, **WeightAverage("swa").config()}
    assert _same_bits(tr.opt.flat_e, _lerp(ps[0], ps[1], average_coefficient("swa", 1)))


def test_a_skipped_window_makes_no_update_and_is_not_counted():
    avg = WeightAverage("ema", decay=0.9, warmup=False)
    tr = Trainer(_toy(), lr=1e-2, max_iter=10, accum_steps=2, loss_scale="dynamic", average=avg)
    xs = _toy_inputs(6)
    tr.step(xs[0], None)
    tr.step(xs[1], None)                          # window 1, clean: t = 1, the copy
    assert tr.average_info()["n_averaged"] == 1 and _same_bits(tr.opt.flat_e, tr.opt.flat_p)
    p1, m1, e1 = tr.opt.flat_p.clone(), tr.opt.flat_m.clone(), tr.opt.flat_e.clone()
    tr.step(xs[2], None)
    tr.opt.flat_a[tr.opt.n // 2 + 1] = float("inf")          # what an overflowed micro-batch leaves in the partial sum
    tr.step(xs[3], None)                          # window 2: skipped as a whole
    info = tr.step_info()
    assert info["skipped"] == 1 and info["taken"] == 1 and info["found_inf"] == 1
    assert _same_bits(tr.opt.flat_p, p1) and _same_bits(tr.opt.flat_m, m1) and _same_bits(tr.opt.flat_e, e1)
    assert tr.average_info()["n_averaged"] == 1 and tr.average_info()["t"] == 1 and tr.opt.it == 2
    tr.step(xs[4], None)
    tr.step(xs[5], None)                          # window 3, clean: t = 2, update 1 -- the index ignores the skipped window
    info = tr.step_info()
    assert info["taken"] == 2 and info["skipped"] == 1
    assert tr.average_info()["n_averaged"] == 2 and not _same_bits(tr.opt.flat_p, p1)
    assert _same_bits(tr.opt.flat_e, _lerp(e1, tr.opt.flat_p, average_coefficient("ema", 1, 0.9, False)))


@pytest.mark.parametrize("loss_scale", [None, "dynamic"])
def test_resume_from_a_checkpoint_continues_the_average(tmp_path, loss_scale):
    """3 steps, save, a fresh model and trainer, load, 2 steps == 5 straight steps.  With a scaler the fresh `taken` word starts at
    0 and taken_base carries the three applied steps."""
    avg = WeightAverage("ema", decay=0.9, warmup=True, start=2, every=1)
    kw = dict(lr=1e-2, max_iter=10, loss_scale=loss_scale, average=avg)
    xs = _toy_inputs(5)
    straight = Trainer(_toy(), **kw)
    for x in xs:
        straight.step(x, None)
    first = Trainer(_toy(), **kw)
    for x in xs[:3]:
        first.step(x, None)
    path = str(tmp_path / "ck.pth")
    save_checkpoint(path, first.model, 0, optimizer=first)
    model = _toy()
    with torch.no_grad():
        for q in model.parameters():
            q.add_(1.0)                           # a fresh model with other weights
    second = Trainer(model, **kw)
    load_checkpoint(path, model, optimizer=second)
    assert second.opt.taken_base == 3 and second.average_info() == first.average_info()
    assert _same_bits(second.opt.flat_e, first.opt.flat_e) and _same_bits(second.opt.flat_p, first.opt.flat_p)
    for x in xs[3:]:
        second.step(x, None)
    for name in ("flat_p", "flat_m", "flat_e"):
        assert _same_bits(getattr(second.opt, name), getattr(straight.opt, name)), name
    assert second.average_info() == straight.average_info() and straight.average_info()["n_averaged"] == 4
    if loss_scale:
        assert second.step_info()["taken"] == 2 and straight.step_info()["taken"] == 5


# ---------------------------------------------------------------------------------------------------------------------
# 10., 11. the small MRFP model
# ---------------------------------------------------------------------------------------------------------------------
def _mrfp():
    from mrfp_amd import deepv3
    from mrfp_amd.config import cfg
    spec = json.load(open(os.path.join(HERE, "golden", "state_dict_spec.json")))
    cfg.MODEL.ACT_DTYPE = torch.float32
    m = deepv3.MRFPPlus(19, criterion=torch.nn.CrossEntropyLoss(ignore_index=255))
    m.load_state_dict(synth.synth_state_dict([(k, tuple(s)) for k, s in spec["MRFPPlus"]], seed=0))
    return m.to(DEV).train()


_TOG = (True, True, True)


def _mrfp_inputs():
    x, y = synth.synth_batch(2, 128, 128, seed=3)
    noise = {k: v.to(DEV) for k, v in synth.synth_noise(2, seed=4).items()}
    return x.to(DEV), y.to(DEV), noise


def test_averaged_swaps_the_weights_in_and_back():
    from mrfp_amd import conv
    from mrfp_amd.deepv3 import InjectedRandom
    x, y, noise = _mrfp_inputs()
    avg = WeightAverage("ema", decay=0.5, warmup=False)

    def run(steps, model, tr):
        for _ in range(steps):
            model.train()
            model.rng = InjectedRandom(_TOG, noise)
            tr.step(x, y)

    model = _mrfp()
    tr = Trainer(model, lr=1e-2, average=avg)
    run(2, model, tr)
    p0, e0, m0 = tr.opt.flat_p.clone(), tr.opt.flat_e.clone(), tr.opt.flat_m.clone()
    assert not _same_bits(p0, e0)
    buf = io.BytesIO()
    save_checkpoint(buf, model, 0, optimizer=tr)
    buf.seek(0)
    ck = torch.load(buf, map_location="cpu", weights_only=True)
    fresh = _mrfp()
    fresh.load_state_dict({k[len("module."):]: v for k, v in ck["average"]["state_dict"].items()})
    conv.invalidate_packs()
    fresh.eval()
    with torch.no_grad():
        want_logits = fresh(x, training=False)
        live_logits = model.eval()(x, training=False)
    want_hist = evaluate(fresh, [(x, y)], fold=True)[0]
    with tr.averaged() as inside:
        assert inside is tr
        assert _same_bits(tr.opt.flat_p, e0) and _same_bits(tr.opt.flat_e, p0)
        with torch.no_grad():
            logits = model.eval()(x, training=False)
        assert _same_bits(logits, want_logits)                   # the packs were rebuilt from the averaged arena
        assert not _same_bits(logits, live_logits)
        assert (evaluate(model, [(x, y)], fold=True)[0] == want_hist).all()
        assert torch.equal(model.state_dict()["final2.0.weight"].cpu(), ck["average"]["state_dict"]["module.final2.0.weight"])
        with pytest.raises(_lib.MrfpHipError, match="averaged"):
            tr.step(x, y)
        with pytest.raises(_lib.MrfpHipError, match="averaged"):
            save_checkpoint(io.BytesIO(), model, 0, optimizer=tr)
    assert _same_bits(tr.opt.flat_p, p0) and _same_bits(tr.opt.flat_e, e0) and _same_bits(tr.opt.flat_m, m0)
    with torch.no_grad():
        assert _same_bits(model.eval()(x, training=False), live_logits)         # ... and rebuilt again on the way out
    with pytest.raises(RuntimeError, match="boom"):
        with tr.averaged():
            raise RuntimeError("boom")
    assert _same_bits(tr.opt.flat_p, p0) and _same_bits(tr.opt.flat_e, e0) and not tr._in_average
    run(1, model, tr)                                            # the next step equals that of a trainer that never entered
    model2 = _mrfp()
    tr2 = Trainer(model2, lr=1e-2, average=avg)
    run(3, model2, tr2)
    for name in ("flat_p", "flat_m", "flat_e"):
        assert _same_bits(getattr(tr.opt, name), getattr(tr2.opt, name)), name
    assert tr.average_info() == tr2.average_info() and tr.average_info()["n_averaged"] == 3


def test_graph_mode_average_matches_eager():
    from mrfp_amd.deepv3 import InjectedRandom
    x, y, noise = _mrfp_inputs()
    out = []
    for graph in (False, True):
        model = _mrfp()
        tr = Trainer(model, lr=1e-3, average=WeightAverage("ema", decay=0.9, warmup=True, start=2))
        if graph:
            tr.enable_graph()
        for _ in range(4):                        # the warm-up call of the graph, then three replays
            model.rng = InjectedRandom(_TOG, noise)
            tr.step(x, y)
        out.append((tr.opt.flat_p.clone(), tr.opt.flat_e.clone(), tr.average_info()))
    assert len(tr._graphs) == 1
    assert _same_bits(out[0][0], out[1][0]) and _same_bits(out[0][1], out[1][1])
    assert out[0][2] == out[1][2] and out[0][2]["n_averaged"] == 3 and float(out[0][1].abs().max()) > 0.0


# ---------------------------------------------------------------------------------------------------------------------
# 13. update_bn
# ---------------------------------------------------------------------------------------------------------------------
class _DeepWrap(torch.nn.Module):
    """A network/deepv3.py factory behind the call Trainer and update_bn make."""

    def __init__(self, net):
        super().__init__()
        self.net = net

    def forward(self, img, label, training=True):
        return self.net(img, gts=label, aux_gts=label)


def test_update_bn_is_the_cumulative_mean_of_the_batch_statistics():
    """Yardstick, per channel and statistic: the float64 mean of the running values each batch leaves when it runs alone from a
    reset with momentum = 1.  Bound 32 * 2^-24 * max_j |b_j|: three roundings per update, four updates, the rounded factor
    1 / (j + 1), and 2x slack -- derived, not measured."""
    import deepv3_common as dc
    from mrfp_amd import conv
    from mrfp_amd.config import cfg
    from mrfp_amd.network import deepv3, wider_resnet
    from mrfp_amd.network.mynn import HipBatchNorm2d
    name = "DeepMobileNetV3PlusD"
    sd, x, y, keep = dc.case_inputs(name)
    x, y = x.to(DEV), y.to(DEV)
    batches = [(x, y), (x.flip(3).contiguous(), y.flip(2).contiguous()), (x.flip(2).contiguous(), y.flip(1).contiguous()),
               ((x * 0.5 + 0.1).contiguous(), y)]
    cfg.MODEL.ACT_DTYPE = torch.float32
    crit = torch.nn.CrossEntropyLoss(ignore_index=255)
    with contextlib.redirect_stdout(io.StringIO()):
        net = getattr(deepv3, name)(None, dc.NC, crit, crit)
    net.load_state_dict(sd)
    model = _DeepWrap(net.to(DEV)).train()
    bns = [(n, m) for n, m in model.named_modules() if isinstance(m, HipBatchNorm2d) and m.running_mean is not None]
    assert len(bns) > 20
    bns[3][1].eval()                              # a flag that differs from the rest: it has to come back
    bns[5][1].momentum = 0.03
    flags = [m.training for m in model.modules()]
    momenta = [m.momentum for _, m in bns]
    wider_resnet.DROP_MASKS.injected = {"dsn": keep.reshape(dc.B, -1)}
    try:
        alone = []
        with torch.no_grad():
            for bx, by in batches:
                for _, m in bns:
                    m.running_mean.zero_()
                    m.running_var.fill_(1.0)
                    m.momentum = 1.0
                    m.training = True
                model(bx, by, training=True)
                alone.append([(m.running_mean.double().clone(), m.running_var.double().clone()) for _, m in bns])
        for (_, m), mom in zip(bns, momenta):
            m.momentum = mom
        for m, f in zip(model.modules(), flags):
            m.training = f
        assert update_bn(model, batches) == len(bns)
        torch.cuda.synchronize()
    finally:
        wider_resnet.DROP_MASKS.injected = None
        conv.backward_failed()
    assert [m.training for m in model.modules()] == flags and [m.momentum for _, m in bns] == momenta
    worst = 0.0
    for i, (n, m) in enumerate(bns):
        for s, got in enumerate((m.running_mean, m.running_var)):
            b = torch.stack([alone[j][i][s] for j in range(4)])
            bound = 32 * 2.0 ** -24 * b.abs().max(0).values
            err = (got.double() - b.mean(0)).abs()
            worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
            assert bool((err <= bound).all()), (n, s, float(err.max()), float(bound.min()))
    print("update_bn: worst error / bound = %.3f" % worst)
    assert float(torch.stack([alone[0][1][0], alone[3][1][0]]).std(0).max()) > 0.0          # the batches' statistics differ
    nbt = [v for k, v in model.state_dict().items() if k.endswith("num_batches_tracked")]
    assert nbt and all(int(v) == 4 for v in nbt)
