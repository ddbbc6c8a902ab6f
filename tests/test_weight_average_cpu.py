"""No-GPU checks of weight averaging inside the fused step: the coefficient and the schedule of the averaging rule as Python states
them (harness.average_coefficient / average_index; tests/test_weight_average_gpu.py compares the device with them), the argument
checks of WeightAverage and Trainer(average=...), the three C entry points (declared, exported, refuse bad arguments before any
launch) and the checkpoint entry built on CPU arenas."""
import ctypes
import os

import numpy as np
import pytest
import torch

from mrfp_amd import _lib, build
from mrfp_amd.harness import (Trainer, WeightAverage, average_coefficient, average_index, averages_made, load_checkpoint,
                              save_checkpoint)


@pytest.fixture(scope="module")
def cdll():
    build.build()
    return _lib.lib()


def _f32(v):
    return float(np.float32(v))


# ---------------------------------------------------------------------------------------------------------------------
# the rule
# ---------------------------------------------------------------------------------------------------------------------
def test_swa_coefficient_is_the_running_mean():
    for n in (1, 2, 3, 7, 100, 8990, 10 ** 6):
        assert average_coefficient("swa", n) == _f32(1.0 / (n + 1))
        assert average_coefficient("swa", n, decay=0.5, warmup=False) == _f32(1.0 / (n + 1))       # decay / warmup unused


def test_ema_coefficient_follows_the_warm_up_to_the_crossover_then_the_decay():
    decay = 0.999
    for n in (1, 2, 3, 8, 9, 10, 100, 5000, 8989):
        assert (1 + n) / (10 + n) < decay
        assert average_coefficient("ema", n, decay, True) == _f32(1.0 - (1 + n) / (10 + n)), n
    for n in (8990, 8991, 20000, 10 ** 6):                     # (1 + 8990) / (10 + 8990) == 0.999: the crossover
        assert (1 + n) / (10 + n) >= decay
        assert average_coefficient("ema", n, decay, True) == _f32(1.0 - decay), n
    assert average_coefficient("ema", 8989, decay, True) > average_coefficient("ema", 8990, decay, True)
    assert average_coefficient("ema", 8990, decay, True) == average_coefficient("ema", 8991, decay, True)
    for n in (1, 9, 8989, 8990):                               # without warm-up: the decay from the first update on
        assert average_coefficient("ema", n, decay, False) == _f32(1.0 - decay)
    assert average_coefficient("ema", 1, 0.9, True) == _f32(1.0 - 2.0 / 11.0)
    assert average_coefficient("ema", 200, 0.9, True) == _f32(1.0 - 0.9)
    # rounded through float32: the value is exactly representable
    for args in (("ema", 3, 0.999, True), ("ema", 9000, 0.999, True), ("swa", 6)):
        c = average_coefficient(*args)
        assert c == _f32(c) and 0.0 < c < 1.0
    with pytest.raises(ValueError):
        average_coefficient("ema", 0)
    with pytest.raises(ValueError):
        average_coefficient("mean", 1)


@pytest.mark.parametrize("start", [1, 2, 3])
@pytest.mark.parametrize("every", [1, 2, 3])
def test_schedule(start, every):
    updates = [(t, average_index(t, start, every)) for t in range(-1, 14) if average_index(t, start, every) is not None]
    want_t = list(range(start, 14, every))
    assert [t for t, _ in updates] == want_t
    assert [n for _, n in updates] == list(range(len(want_t)))          # 0, 1, 2, ...: the first update is the copy
    for t in range(0, 14):
        assert averages_made(t, start, every) == sum(1 for u in want_t if u <= t)


# ---------------------------------------------------------------------------------------------------------------------
# argument checks
# ---------------------------------------------------------------------------------------------------------------------
def test_weight_average_refuses_what_the_c_side_refuses():
    for bad in (dict(kind="mean"), dict(kind=0), dict(kind=None), dict(decay=0.0), dict(decay=1.0), dict(decay=-0.1), dict(decay=1.5),
                dict(decay=float("nan")), dict(decay="0.9"), dict(decay=True), dict(start=0), dict(start=-3), dict(start=1.0),
                dict(start=True), dict(start=2 ** 31), dict(every=0), dict(every=-1), dict(every=2.0), dict(every=False),
                dict(kind="swa", decay=0.0), dict(kind="swa", every=0)):
        with pytest.raises(ValueError):
            WeightAverage(**bad)
    w = WeightAverage()
    assert w.config() == {"kind": "ema", "decay": 0.999, "warmup": True, "start": 1, "every": 1}
    assert w.c_args() == (0, 0.999, 1, 1, 1)
    assert WeightAverage("swa", start=5, every=2, warmup=0).c_args() == (1, 0.999, 0, 5, 2)


def test_trainer_refuses_a_bad_average_before_touching_the_model():
    class Untouchable:
        def parameters(self):
            raise AssertionError("the model was touched before the arguments were checked")

    for bad in ("mean", "EMA", 0.999, 1, True, ("ema",), {"kind": "ema"}):
        with pytest.raises(ValueError):
            Trainer(Untouchable(), average=bad)
    for good in ("ema", "swa", WeightAverage("swa", start=3)):
        with pytest.raises(AssertionError):
            Trainer(Untouchable(), average=good)


def test_default_trainer_allocates_no_average():
    torch.manual_seed(0)
    tr = Trainer(torch.nn.Linear(5, 3))
    assert tr.opt.flat_e is None and tr.opt.average is None
    with pytest.raises(_lib.MrfpHipError):
        tr.average_info()
    with pytest.raises(_lib.MrfpHipError):
        with tr.averaged():
            pass
    tr = Trainer(torch.nn.Linear(5, 3), average="swa")
    assert tr.opt.flat_e.shape == tr.opt.flat_p.shape and float(tr.opt.flat_e.abs().max()) == 0.0
    assert tr.opt.average.kind == "swa" and tr.average_info()["n_averaged"] == 0 and tr.average_info()["t"] == 0
    with pytest.raises(_lib.MrfpHipError):              # CPU arenas: no fallback
        with tr.averaged():
            pass


# ---------------------------------------------------------------------------------------------------------------------
# the C boundary
# ---------------------------------------------------------------------------------------------------------------------
_V, _I, _L, _F, _D = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_double


def test_entry_points_are_declared_and_exported(cdll):
    protos = _lib.parse_header()
    want = {
        "mrfp_sgd_step_avg": (["p", "g", "m", "e", "n", "lr", "momentum", "weight_decay", "gscale", "first", "kind", "decay", "warmup",
                               "start", "every", "t", "stream"],
                              [_V, _V, _V, _V, _L, _F, _F, _F, _F, _I, _I, _D, _I, _I, _I, _I, _V]),
        "mrfp_sgd_step_checked_avg": (["p", "g", "m", "e", "n", "lr", "momentum", "weight_decay", "state", "taken_base", "kind", "decay",
                                       "warmup", "start", "every", "stream"],
                                      [_V, _V, _V, _V, _L, _F, _F, _F, _V, _I, _I, _D, _I, _I, _I, _V]),
        "mrfp_arena_swap": (["a", "b", "n", "stream"], [_V, _V, _L, _V]),
    }
    for name, (names, types) in want.items():
        assert name in protos and hasattr(cdll, name), name
        assert protos[name] == (ctypes.c_int, types), name
        assert _lib.ARG_NAMES[name] == names, name


def _host_arenas():
    buf = ctypes.create_string_buffer(1 << 13)
    base = (ctypes.addressof(buf) + 255) & ~255
    return buf, base


def test_averaged_steps_refuse_bad_arguments(cdll):
    """Pointers into a host buffer: every refusal happens before a launch (this needs no GPU: a launch would show as another
    error text and code), and names its entry point."""
    buf, b = _host_arenas()
    common = dict(p=b, g=b + 1024, m=b + 2048, e=b + 3072, n=8, lr=0.1, momentum=0.9, weight_decay=0.0)
    rule = dict(kind=0, decay=0.999, warmup=1, start=1, every=1)
    good = {"mrfp_sgd_step_avg": dict(common, gscale=1.0, first=0, **rule, t=1, stream=None),
            "mrfp_sgd_step_checked_avg": dict(common, state=b + 4096, taken_base=0, **rule, stream=None)}
    changes = [dict(p=None), dict(g=None), dict(m=None), dict(e=None), dict(n=0), dict(n=6), dict(n=-4), dict(p=b + 4), dict(g=b + 1028),
               dict(m=b + 2052), dict(e=b + 3076), dict(e=b + 3080), dict(kind=2), dict(kind=-1), dict(decay=0.0), dict(decay=1.0),
               dict(decay=-0.5), dict(decay=float("nan")), dict(kind=1, decay=1.5), dict(start=0), dict(start=-1), dict(every=0),
               dict(every=-2)]
    for name, base in good.items():
        names = _lib.ARG_NAMES[name]
        assert sorted(names) == sorted(base), name
        extra = [dict(state=None), dict(state=b + 4100)] if "state" in base else []
        for change in changes + extra:
            args = dict(base, **change)
            rc = getattr(cdll, name)(*[args[k] for k in names])
            msg = cdll.mrfp_last_error()
            assert rc == -1 and msg.startswith(name[len("mrfp_"):].encode() + b":"), (name, change, rc, msg)


def test_arena_swap_refuses_bad_arguments(cdll):
    buf, b = _host_arenas()
    for a, c, n in ((None, b, 8), (b, None, 8), (b, b + 1024, 0), (b, b + 1024, 6), (b, b + 1024, -8), (b + 4, b + 1024, 8),
                    (b, b + 1028, 8), (b, b, 8), (b, b + 16, 8), (b + 16, b, 8), (b, b + 16, 1024)):
        rc = cdll.mrfp_arena_swap(a, c, n, None)
        assert rc == -1 and cdll.mrfp_last_error().startswith(b"arena_swap:"), (a, c, n, cdll.mrfp_last_error())
    rc = cdll.mrfp_arena_swap(b, b + 16, 8, None)
    assert b"overlap" in cdll.mrfp_last_error()


# ---------------------------------------------------------------------------------------------------------------------
# the checkpoint entry, on CPU arenas
# ---------------------------------------------------------------------------------------------------------------------
class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.a = torch.nn.Linear(7, 5)
        self.bn = torch.nn.BatchNorm1d(5)                   # buffers: not averaged
        self.frozen = torch.nn.Linear(5, 3).requires_grad_(False)
        self.b = torch.nn.Linear(3, 2)


def test_checkpoint_entry_layout_and_round_trip(tmp_path):
    torch.manual_seed(0)
    net = _Net()
    net.bn.running_mean.copy_(torch.randn(5))
    tr = Trainer(net, average=WeightAverage("ema", decay=0.9, warmup=False, start=2, every=2))
    opt = tr.opt
    for p, o in zip(opt.params, opt.offsets):               # what six applied steps would have left there (the padding between
        opt.flat_e[o:o + p.numel()] = torch.randn(p.numel())  # tensors stays zero, as the kernels leave it: p, g, m are zero there)
    opt.taken_base = 6
    assert tr.average_info() == {"t": 6, "n_averaged": 3, "kind": "ema", "decay": 0.9, "warmup": False, "start": 2, "every": 2}
    path = str(tmp_path / "ck.pth")
    save_checkpoint(path, net, 4, optimizer=tr)
    ck = torch.load(path, map_location="cpu", weights_only=True)          # the safe unpickler takes the file
    assert set(ck) == {"epoch", "state_dict", "optimizer", "average"}
    avg = ck["average"]
    assert set(avg) == {"kind", "decay", "warmup", "start", "every", "t", "n_averaged", "state_dict"}
    assert {k: v for k, v in avg.items() if k != "state_dict"} == tr.average_info()
    msd = net.state_dict()
    assert list(avg["state_dict"]) == ["module." + k for k in msd] == list(ck["state_dict"])
    trainable = {n for n, p in net.named_parameters() if p.requires_grad}
    assert trainable == {"a.weight", "a.bias", "bn.weight", "bn.bias", "b.weight", "b.bias"}
    by_name = dict(net.named_parameters())
    for k, v in msd.items():
        got = avg["state_dict"]["module." + k]
        assert got.shape == v.shape and got.dtype == v.dtype
        if k in trainable:                                   # cut from the averaged arena
            o = opt.offsets[[id(p) for p in opt.params].index(id(by_name[k]))]
            assert torch.equal(got.reshape(-1), opt.flat_e[o:o + v.numel()])
            assert not torch.equal(got, v)
        else:                                                # buffers and frozen parameters: the live model's
            assert torch.equal(got, v)
    # ... and loads straight into a model
    fresh = _Net()
    fresh.load_state_dict({k[len("module."):]: v for k, v in avg["state_dict"].items()})
    assert torch.equal(fresh.a.weight, avg["state_dict"]["module.a.weight"])

    # round trip into a second trainer: the arena and the count come back; a trainer without an average ignores the entry
    torch.manual_seed(1)
    net2 = _Net()
    tr2 = Trainer(net2, average=WeightAverage("ema", decay=0.9, warmup=False, start=2, every=2))
    epoch, _ = load_checkpoint(path, net2, optimizer=tr2)
    assert epoch == 4 and torch.equal(tr2.opt.flat_e, opt.flat_e) and torch.equal(tr2.opt.flat_p, opt.flat_p)
    assert tr2.average_info() == tr.average_info() and tr2.opt.taken_base == 6
    net3 = _Net()
    tr3 = Trainer(net3)
    load_checkpoint(path, net3, optimizer=tr3)
    assert tr3.opt.flat_e is None and torch.equal(tr3.opt.flat_p, opt.flat_p)


def test_checkpoint_without_the_entry_loads_as_before(tmp_path):
    torch.manual_seed(0)
    net = _Net()
    path = str(tmp_path / "plain.pth")
    save_checkpoint(path, net, 1, optimizer=Trainer(net))
    assert "average" not in torch.load(path, map_location="cpu", weights_only=True)
    net2 = _Net()
    tr2 = Trainer(net2, average="swa")
    tr2.opt.flat_e.fill_(3.0)
    tr2.opt.taken_base = 2
    epoch, _ = load_checkpoint(path, net2, optimizer=tr2)
    assert epoch == 1 and float(tr2.opt.flat_e.min()) == 3.0 and tr2.opt.taken_base == 2          # untouched
