"""No-GPU checks of the checked optimiser step (dynamic loss scale, overflow skip, gradient-norm clipping): argument refusals
of LossScaler / Trainer / the two C entry points before anything touches a device, the grid query, and the state-dict layout
shared with torch.amp.GradScaler."""
import ctypes
import math

import pytest
import torch

from mrfp_amd import _lib, build


@pytest.fixture(scope="module")
def cdll():
    build.build()
    return _lib.lib()


def test_loss_scaler_refuses_bad_arguments():
    from mrfp_amd.harness import LossScaler
    for kw in (dict(init_scale=0.0), dict(init_scale=-1.0), dict(init_scale=math.inf), dict(init_scale=math.nan),
               dict(growth_factor=1.0), dict(growth_factor=0.5), dict(backoff_factor=1.0), dict(backoff_factor=0.0),
               dict(backoff_factor=1.5), dict(growth_interval=0), dict(growth_interval=-3), dict(growth_interval=1.5)):
        with pytest.raises(ValueError):
            LossScaler(device="cpu", **kw)
    s = LossScaler(device="cpu")
    assert s.info() == {"scale": 65536.0, "growth_tracker": 0, "found_inf": 0, "grad_norm": 0.0, "gmul": 0.0, "taken": 0,
                        "skipped": 0}
    assert s.scale_tensor.dim() == 0 and s.scale_tensor.dtype == torch.float32 and float(s.scale_tensor) == 65536.0
    assert s.scale_tensor.data_ptr() == s.state.data_ptr() and s.state.data_ptr() % 16 == 0
    assert s.dynamic and not LossScaler(device="cpu", dynamic=False).dynamic
    for bad in (dict(scale=0.0), dict(growth_factor=1.0), dict(backoff_factor=1.0), dict(growth_interval=0), dict(_growth_tracker=-1)):
        with pytest.raises(ValueError):
            s.load_state_dict(dict(s.state_dict(), **bad))
    assert s.info()["scale"] == 65536.0                    # a refused dict changed nothing


def test_trainer_refuses_bad_arguments_before_touching_a_device():
    """The checks come first: the model is never looked at (a model without parameters would raise 'no trainable parameters',
    a CPU model would build CPU arenas)."""
    from mrfp_amd.harness import FlatSGD, LossScaler, Trainer

    class Untouchable:
        def parameters(self):
            raise AssertionError("the model was touched before the arguments were checked")

    for kw in (dict(loss_scale="static"), dict(loss_scale=0.0), dict(loss_scale=-2.0), dict(loss_scale=math.inf),
               dict(loss_scale=math.nan), dict(loss_scale=[1.0]), dict(loss_scale=True), dict(max_grad_norm=0.0),
               dict(max_grad_norm=-1.0), dict(max_grad_norm=math.nan), dict(loss_scale="dynamic", max_grad_norm=0.0)):
        with pytest.raises(ValueError):
            Trainer(Untouchable(), **kw)
    # FlatSGD.step: no CPU fallback for the checked step either
    opt = FlatSGD(torch.nn.Linear(3, 2))
    with pytest.raises(_lib.MrfpHipError):
        opt.step(scaler=LossScaler(device="cpu"))


def _buf():
    buf = ctypes.create_string_buffer(1 << 12)
    return buf, (ctypes.addressof(buf) + 255) & ~255


def test_grad_check_refuses_bad_arguments(cdll):
    """Through the loaded library, with pointers into a host buffer: every refusal happens before a launch."""
    buf, p = _buf()
    g, ws, st = p, p + 1024, p + 2048
    good = dict(g=g, n=8, gscale=1.0, ws=ws, state=st, dynamic=1, growth=2.0, backoff=0.5, growth_interval=2000,
                max_norm=math.inf, stream=None)
    names = _lib.ARG_NAMES["mrfp_grad_check"]
    assert names == list(good), names
    bad = [dict(g=None), dict(ws=None), dict(state=None), dict(n=6), dict(n=0), dict(g=g + 4), dict(ws=ws + 4), dict(state=st + 4),
           dict(backoff=1.0), dict(backoff=0.0), dict(growth=1.0), dict(growth_interval=0), dict(max_norm=0.0), dict(max_norm=-1.0),
           dict(max_norm=math.nan), dict(growth=math.nan), dict(backoff=math.nan)]
    for change in bad:
        args = dict(good, **change)
        rc = cdll.mrfp_grad_check(*[args[k] for k in names])
        assert rc == -1 and cdll.mrfp_last_error().startswith(b"grad_check:"), (change, rc, cdll.mrfp_last_error())


def test_sgd_step_checked_refuses_bad_arguments(cdll):
    buf, p = _buf()
    pp, g, m, st = p, p + 512, p + 1024, p + 2048
    good = dict(p=pp, g=g, m=m, n=8, lr=0.01, momentum=0.9, weight_decay=5e-4, state=st, stream=None)
    names = _lib.ARG_NAMES["mrfp_sgd_step_checked"]
    assert names == list(good), names
    bad = [dict(p=None), dict(g=None), dict(m=None), dict(state=None), dict(n=6), dict(n=0), dict(p=pp + 4), dict(g=g + 4),
           dict(m=m + 4), dict(state=st + 4)]
    for change in bad:
        args = dict(good, **change)
        rc = cdll.mrfp_sgd_step_checked(*[args[k] for k in names])
        assert rc == -1 and cdll.mrfp_last_error().startswith(b"sgd_step_checked:"), (change, rc, cdll.mrfp_last_error())


def test_grad_check_nblocks(cdll):
    """One workgroup per 256 16-byte vectors, capped by one constant (csrc/sgd.hip: kGradCheckCap)."""
    import os
    import re
    nb = cdll.mrfp_grad_check_nblocks
    src = open(os.path.join(os.path.dirname(_lib.HEADER), "..", "mrfp_amd", "csrc", "sgd.hip")).read()
    cap = int(re.search(r"constexpr int kGradCheckCap = (\d+);", src).group(1))
    assert nb(4) == 1 and nb(8) == 1 and nb(1024) == 1 and nb(1028) == 2
    assert nb(1 << 30) == cap and nb(cap * 1024) == cap and nb(cap * 1024 - 1024) == cap - 1
    last = 0
    for n in [4 * k for k in (1, 2, 255, 256, 257, 1000, 4096, 65536, 1 << 19, (1 << 19) + 1, 1 << 22, 1 << 26, 1 << 28)]:
        v = int(nb(n))
        assert last <= v <= cap, (n, v)
        last = v


def test_state_dict_round_trip_with_torch_grad_scaler():
    from mrfp_amd.harness import LossScaler
    ours = LossScaler(init_scale=1024.0, growth_factor=3.0, backoff_factor=0.25, growth_interval=7, device="cpu")
    sd = ours.state_dict()
    assert sd == {"scale": 1024.0, "growth_factor": 3.0, "backoff_factor": 0.25, "growth_interval": 7, "_growth_tracker": 0}
    stock = torch.amp.GradScaler("cpu")
    assert set(stock.state_dict()) == set(sd)
    stock.load_state_dict(sd)                                   # a stock scaler loads ours
    assert stock.state_dict() == sd
    # ... and we load a stock scaler's, tracker included
    stock2 = torch.amp.GradScaler("cpu", init_scale=4.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=3)
    sd2 = dict(stock2.state_dict(), _growth_tracker=2)
    ours.load_state_dict(sd2)
    assert ours.state_dict() == sd2
    i = ours.info()
    assert i["scale"] == 4.0 and i["growth_tracker"] == 2 and ours.growth_interval == 3 and ours.backoff_factor == 0.5
    assert float(ours.scale_tensor) == 4.0                      # loaded in place: the view still reads the live state


def test_expected_scale_sequence_of_the_stock_scaler():
    """What the GPU test compares with, pinned on the CPU: GradScaler(init_scale=4, growth_interval=2) over five finite steps
    goes 4 -> 4, 8, 8, 16, 16 (value after each update)."""
    s = torch.amp.GradScaler("cpu", init_scale=4.0, growth_interval=2)
    w = torch.nn.Parameter(torch.ones(3))
    opt = torch.optim.SGD([w], lr=0.1)
    seq = []
    for _ in range(5):
        opt.zero_grad()
        s.scale(w.sum()).backward()
        s.step(opt)
        s.update()
        seq.append(s.get_scale())
    assert seq == [4.0, 8.0, 8.0, 16.0, 16.0]


def test_checkpoint_with_scaler_entry_loads_under_the_safe_unpickler(tmp_path):
    from mrfp_amd import harness

    class FakeTrainer:                    # what save_checkpoint reads of a Trainer
        def __init__(self, model):
            self.opt = harness.FlatSGD(model)
            self.scaler = harness.LossScaler(init_scale=512.0, device="cpu")

    model = torch.nn.Linear(5, 3)
    tr = FakeTrainer(model)
    path = str(tmp_path / "ck.pth")
    harness.save_checkpoint(path, model, epoch=2, optimizer=tr)
    ck = torch.load(path, weights_only=True)
    assert set(ck) == {"epoch", "state_dict", "optimizer", "scaler"}
    assert ck["scaler"] == {"scale": 512.0, "growth_factor": 2.0, "backoff_factor": 0.5, "growth_interval": 2000, "_growth_tracker": 0}
    # restored when both sides have one; a file without the key, or a target without a scaler, loads as before
    model2 = torch.nn.Linear(5, 3)
    tr2 = FakeTrainer(model2)
    tr2.scaler = harness.LossScaler(init_scale=2.0, device="cpu")
    epoch, _ = harness.load_checkpoint(path, model2, optimizer=tr2)
    assert epoch == 2 and tr2.scaler.info()["scale"] == 512.0
    harness.load_checkpoint(path, model2, optimizer=tr2.opt)
    path0 = str(tmp_path / "ck0.pth")
    harness.save_checkpoint(path0, model, epoch=1, optimizer=tr.opt)
    assert "scaler" not in torch.load(path0, weights_only=True)
    tr2.scaler = harness.LossScaler(init_scale=2.0, device="cpu")
    harness.load_checkpoint(path0, model2, optimizer=tr2)
    assert tr2.scaler.info()["scale"] == 2.0
