"""The checked optimiser step (mrfp_grad_check + mrfp_sgd_step_checked, harness.LossScaler) against stock PyTorch on the same
device: torch.amp.GradScaler + torch.nn.utils.clip_grad_norm_ + torch.optim.SGD(momentum .9, wd 5e-4) + LambdaLR(poly .9).
Arena level: a FlatSGD over an nn.ParameterList, scaled gradients written straight into flat_g.  Model level: float16 ResNet-50."""
import json
import math
import os

import pytest
import torch

from mrfp_amd import _lib, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
SPEC = json.load(open(os.path.join(HERE, "golden", "state_dict_spec.json")))
RTOL, ATOL = 2e-5, 1e-6              # test_harness_gpu.py::test_fused_sgd_matches_torch_optim: the project's bar for this kernel


def _cap():
    return int(_lib.lib().mrfp_grad_check_nblocks(1 << 30))


def _sizes():
    """The smallest arenas that reach each code path: one workgroup with most lanes idle; a ragged tail across workgroups;
    every thread of the capped grid loops more than once, plus a tail."""
    return [8, 4 * (256 * 3 + 5), _cap() * 256 * 4 * 2 + 4 * 37]


class Pair:
    """Our FlatSGD + LossScaler and the stock recipe over the same start values; step(G) feeds both the same RAW (scaled)
    gradient."""

    def __init__(self, n, seed=0, max_norm=None, **scaler_kw):
        from mrfp_amd.harness import FlatSGD, LossScaler
        g = torch.Generator().manual_seed(seed)
        w0 = torch.randn(n, generator=g)
        self.n, self.max_norm = n, max_norm
        self.net = torch.nn.ParameterList([torch.nn.Parameter(w0.clone())]).to(DEV)
        self.opt = FlatSGD(self.net, lr=1e-2, max_iter=40)
        self.scaler = LossScaler(device=DEV, **scaler_kw)
        self.ref = torch.nn.Parameter(w0.clone().to(DEV))
        self.ropt = torch.optim.SGD([self.ref], lr=1e-2, momentum=0.9, weight_decay=5e-4)
        self.sched = torch.optim.lr_scheduler.LambdaLR(self.ropt, lr_lambda=lambda it: (1 - it / 40) ** 0.9)
        self.stock = torch.amp.GradScaler(torch.device(DEV).type, **{k: v for k, v in scaler_kw.items() if k != "dynamic"})
        self.stock.scale(torch.zeros((), device=DEV))            # (creates the stock scaler's device scale)
        self.dynamic = scaler_kw.get("dynamic", True)

    def grad(self, seed, amp=1.0):
        g = torch.Generator().manual_seed(1000 + seed)
        return (torch.randn(self.n, generator=g) * amp).to(DEV)

    def step(self, G, gscale=1.0):
        self.opt.flat_g.copy_(G)
        self.opt.step(gscale, scaler=self.scaler, max_grad_norm=self.max_norm)
        self.ref.grad = (G * gscale).clone()
        self.stock.unscale_(self.ropt)
        if self.max_norm is not None:
            torch.nn.utils.clip_grad_norm_([self.ref], self.max_norm)
        self.stock.step(self.ropt)
        if self.dynamic:
            self.stock.update()
        else:
            self.stock.update(self.stock.get_scale())           # a fixed scale (update still closes the stock scaler's step)
        self.sched.step()

    def check_params(self):
        torch.testing.assert_close(self.opt.flat_p, self.ref.detach(), rtol=RTOL, atol=ATOL)

    def check_scale(self):
        i = self.scaler.info()
        assert i["scale"] == self.stock.get_scale(), (i, self.stock.get_scale())
        if self.dynamic:
            assert i["growth_tracker"] == self.stock._get_growth_tracker(), (i, self.stock._get_growth_tracker())
        return i


@pytest.mark.parametrize("size", range(3))
def test_finite_gradients_dynamic_scale_matches_grad_scaler(size):
    """Case 1: five finite steps against GradScaler(init_scale=4, growth_interval=2): parameters at the fused kernel's own
    tolerance, scale and growth tracker EXACTLY, after every step (4 -> 4, 8, 8, 16, 16)."""
    pr = Pair(_sizes()[size], seed=size, init_scale=4.0, growth_interval=2)
    scales = []
    for k in range(5):
        S = pr.scaler.info()["scale"]
        pr.step(pr.grad(k) * S)
        pr.check_params()
        i = pr.check_scale()
        scales.append(i["scale"])
        assert i["found_inf"] == 0 and i["taken"] == k + 1 and i["skipped"] == 0 and i["gmul"] == 1.0 / S, i
    assert scales == [4.0, 8.0, 8.0, 16.0, 16.0]
    assert pr.opt.it == 5
    sd = pr.opt.state_dict()                      # `taken` tells state_dict that momentum exists
    assert torch.equal(sd["state"][0]["momentum_buffer"], pr.opt.flat_m.cpu())


@pytest.mark.parametrize("size", range(3))
def test_overflow_anywhere_skips_the_step_bit_for_bit(size):
    """Case 2: one inf / -inf / nan at element 0, at the last element, inside the ragged tail and (largest arena) beyond
    cap*256*4, where a thread arrives only on its second loop.  The step writes nothing, found_inf = 1, skipped += 1, the scale
    halves, the tracker resets; the next finite step equals stock torch's next step -- also when the skipped step was the very
    first one (the first case of each chain: momentum starts from the zero arena)."""
    n, cap = _sizes()[size], _cap()
    pos = {0: [0, n - 1], 1: [0, n - 1, 4 * 256 * 3 + 2], 2: [0, n - 1, cap * 2048 + 5, cap * 1024 + 17]}[size]
    pr = Pair(n, seed=10 + size, init_scale=2.0 ** 16, growth_interval=1000)
    k = 0
    for val in (math.inf, -math.inf, math.nan):
        for at in pos:
            before = pr.scaler.info()
            p0, m0, it0 = pr.opt.flat_p.clone(), pr.opt.flat_m.clone(), pr.opt.it
            G = pr.grad(k) * before["scale"]
            G[at] = val
            pr.step(G)
            i = pr.check_scale()
            assert torch.equal(pr.opt.flat_p, p0) and torch.equal(pr.opt.flat_m, m0), (val, at)
            assert i["found_inf"] == 1 and i["skipped"] == before["skipped"] + 1 and i["taken"] == before["taken"], (val, at, i)
            assert i["scale"] == before["scale"] * 0.5 and i["growth_tracker"] == 0, (val, at, i)
            assert pr.opt.it == it0 + 1                          # the schedule advances on a skipped step too
            pr.check_params()
            pr.step(pr.grad(k + 500) * i["scale"])               # the next finite step
            j = pr.check_scale()
            assert j["found_inf"] == 0 and j["taken"] == before["taken"] + 1 and j["growth_tracker"] == 1, (val, at, j)
            pr.check_params()
            k += 1


def test_a_large_finite_gradient_is_taken():
    """Case 2, last item: 1e30 in one slot (its square overflows float32), scale 1, no clipping: not an overflow."""
    n = _sizes()[1]
    pr = Pair(n, seed=3, init_scale=1.0)
    G = pr.grad(0)
    G[n // 2 + 1] = 1e30
    p0 = pr.opt.flat_p.clone()
    pr.step(G)
    i = pr.check_scale()
    assert i["found_inf"] == 0 and i["taken"] == 1 and i["skipped"] == 0 and i["gmul"] == 1.0, i
    assert math.isfinite(i["grad_norm"]) and abs(i["grad_norm"] / 1e30 - 1) < 1e-5, i
    assert not torch.equal(pr.opt.flat_p, p0) and bool(torch.isfinite(pr.opt.flat_p).all())
    pr.check_params()


@pytest.mark.parametrize("max_norm", [1.0, 1e9])
@pytest.mark.parametrize("size", range(3))
def test_clipping_matches_clip_grad_norm(size, max_norm):
    """Case 3: clip_grad_norm_ after unscale_.  grad_norm within rtol 1e-5 of the float64 norm of the same data (a float32 square
    carries 2^-24, a per-thread float32 chain of L terms at most L * 2^-24: 1e-5 covers 160 terms; the kernel accumulates in
    double from the first term on, so it has room to spare at every size); 1e9 must not clip."""
    n = _sizes()[size]
    pr = Pair(n, seed=20 + size, max_norm=max_norm, init_scale=64.0, growth_interval=1000)
    for k in range(2):
        G = pr.grad(k, amp=3.0) * 64.0
        pr.step(G)
        i = pr.check_scale()
        want = float(torch.linalg.vector_norm(G.double() / 64.0))
        assert abs(i["grad_norm"] - want) <= 1e-5 * want, (i, want)
        c = min(1.0, max_norm / (want + 1e-6))
        assert (c == 1.0) == (max_norm == 1e9)
        assert abs(i["gmul"] - c / 64.0) <= 1e-6 * c / 64.0, (i, c)
        if max_norm == 1e9:
            assert i["gmul"] == 1.0 / 64.0
        assert i["found_inf"] == 0 and i["taken"] == k + 1
        pr.check_params()


def test_the_check_is_deterministic():
    """Case 4: the same arena checked twice gives bit-identical grad_norm and gmul (fixed summation order, no atomics)."""
    n = _sizes()[2]
    pr = Pair(n, seed=5, max_norm=1.0, init_scale=8.0, dynamic=False)
    G = pr.grad(0) * 8.0
    words = []
    for _ in range(2):
        pr.opt.flat_g.copy_(G)
        pr.opt.step(1.0, scaler=pr.scaler, max_grad_norm=1.0)
        words.append(pr.scaler.state.cpu()[3:5].clone())
    assert torch.equal(words[0], words[1]), words
    i = pr.scaler.info()
    assert i["taken"] == 2 and 0.0 < i["gmul"] < 1.0 / 8.0 and i["grad_norm"] > 1.0


def test_static_scaler_skips_and_keeps_its_scale():
    """Case 5: dynamic=False: an overflow skips the step and leaves the scale alone; clean steps never grow it."""
    n = _sizes()[1]
    pr = Pair(n, seed=6, init_scale=128.0, growth_interval=1, dynamic=False)
    pr.step(pr.grad(0) * 128.0)
    pr.check_params()
    p0, m0 = pr.opt.flat_p.clone(), pr.opt.flat_m.clone()
    G = pr.grad(1) * 128.0
    G[n - 3] = math.inf
    pr.step(G)
    i = pr.scaler.info()
    assert torch.equal(pr.opt.flat_p, p0) and torch.equal(pr.opt.flat_m, m0)
    assert i["found_inf"] == 1 and i["skipped"] == 1 and i["taken"] == 1 and i["scale"] == 128.0 and i["growth_tracker"] == 0, i
    pr.step(pr.grad(2) * 128.0)
    i = pr.scaler.info()
    assert i["found_inf"] == 0 and i["taken"] == 2 and i["scale"] == 128.0 and i["growth_tracker"] == 0, i
    pr.check_params()


def test_gscale_and_scale_fold_into_one_factor():
    """Case 6: gscale = 0.25 (four ranks) with scale 8: the applied factor is 0.25 / 8, and the update is the closed form
    test_fused_sgd_matches_torch_optim ends with."""
    from mrfp_amd.harness import FlatSGD, LossScaler
    n = _sizes()[1]
    net = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(n, generator=torch.Generator().manual_seed(7)))]).to(DEV)
    opt = FlatSGD(net, lr=1e-2, max_iter=10)
    sc = LossScaler(init_scale=8.0, device=DEV)
    gen = torch.Generator().manual_seed(8)
    for k in range(2):                                            # the second step starts from a non-zero momentum
        opt.flat_g.copy_(torch.randn(n, generator=gen).to(DEV) * 8.0)
        before, g, m, lr = opt.flat_p.clone(), opt.flat_g.clone(), opt.flat_m.clone(), opt.lr
        opt.step(gscale=0.25, scaler=sc)
        i = sc.info()
        assert i["gmul"] == 0.25 / 8.0 and i["found_inf"] == 0 and i["taken"] == k + 1, i
        exp_m = 0.9 * m + (0.25 / 8.0 * g + 5e-4 * before)
        torch.testing.assert_close(opt.flat_p, before - lr * exp_m, rtol=1e-5, atol=1e-7)
        torch.testing.assert_close(opt.flat_m, exp_m, rtol=1e-5, atol=1e-7)


# ---- model level ---------------------------------------------------------------------------------------------------------------
def _model(dtype):
    from mrfp_amd import deepv3
    from mrfp_amd.config import cfg
    cfg.MODEL.ACT_DTYPE = dtype
    m = deepv3.MRFPPlus(19, criterion=torch.nn.CrossEntropyLoss(ignore_index=255))
    m.load_state_dict(synth.synth_state_dict([(k, tuple(s)) for k, s in SPEC["MRFPPlus"]], seed=0))
    return m.to(DEV).train()


@pytest.mark.parametrize("graph", [False, True])
def test_float16_resnet50_backs_off_from_an_absurd_scale(graph):
    """Case 7: float16 ResNet-50 MRFPPlus at 2 x 256 x 256 with LossScaler(init_scale=2**32): the first step must overflow -- it is
    skipped (every parameter and momentum value bit-unchanged, scale 2**31).  Eager: stepping on, the scale halves until a step is
    taken, after at most 33 more steps (at scale 1 nothing can overflow); the parameters are then finite and have moved.  Graph
    mode: warm-up + capture, then one replay -- the replayed backward reads the scale its own step finds in the device state, so
    the reported scale is 2**32 * 0.5**skipped.  inf / NaN are ordinary float values to these kernels: nothing faults."""
    from mrfp_amd.config import cfg
    from mrfp_amd.deepv3 import InjectedRandom
    from mrfp_amd.harness import LossScaler, Trainer
    try:
        model = _model(torch.float16)
        tr = Trainer(model, lr=1e-2, loss_scale=LossScaler(init_scale=2.0 ** 32))
        if graph:
            tr.enable_graph()
        x, y = synth.synth_batch(2, 256, 256, seed=3)
        x, y = x.to(DEV), y.to(DEV)
        noise = {k: v.to(DEV) for k, v in synth.synth_noise(2, seed=4).items()}
        model.rng = InjectedRandom((True, True, True), noise)
        p0, m0 = tr.opt.flat_p.clone(), tr.opt.flat_m.clone()
        tr.step(x, y)
        i = tr.step_info()
        print("first step:", i)
        assert i["skipped"] == 1 and i["taken"] == 0 and i["found_inf"] == 1 and i["scale"] == 2.0 ** 31, i
        assert torch.equal(tr.opt.flat_p, p0) and torch.equal(tr.opt.flat_m, m0)
        if graph:
            tr.step(x, y)                                        # the first replay
            i = tr.step_info()
            print("after one replay:", i)
            assert i["skipped"] + i["taken"] == 2 and i["scale"] == 2.0 ** 32 * 0.5 ** i["skipped"], i
            assert len(tr._graphs) == 1
            return
        for _ in range(33):
            tr.step(x, y)
            i = tr.step_info()
            if i["taken"] == 1:
                break
        print("first taken step:", i)
        assert i["taken"] == 1 and i["scale"] == 2.0 ** 32 * 0.5 ** i["skipped"] and i["scale"] >= 1.0, i
        assert bool(torch.isfinite(tr.opt.flat_p).all()) and bool(torch.isfinite(tr.opt.flat_m).all())
        assert not torch.equal(tr.opt.flat_p, p0)
        assert all(bool(torch.isfinite(p).all()) for p in model.parameters())
    finally:
        cfg.MODEL.ACT_DTYPE = torch.float32


def test_resume_restores_the_scaler_bit_for_bit(tmp_path):
    """Case 8: 2 steps -> save_checkpoint -> fresh model + Trainer('dynamic') -> load_checkpoint: scale, growth tracker and the
    next step's parameters equal the uninterrupted run bit for bit (pattern of test_resume_from_checkpoint_reproduces_step_4)."""
    from mrfp_amd import harness
    from mrfp_amd.deepv3 import InjectedRandom
    toggles = [(True, True, True), (False, True, False), (True, False, True)]
    data = [synth.synth_batch(2, 128, 128, seed=30 + i) for i in range(3)]
    noise = [synth.synth_noise(2, seed=40 + i) for i in range(3)]

    def run(tr, model, i):
        model.rng = InjectedRandom(toggles[i], noise[i])
        return float(tr.step(data[i][0].to(DEV), data[i][1].to(DEV)))

    model = _model(torch.float32)
    # (a growth interval of 3 and a start away from the default: the scale and the tracker both move within the two steps)
    tr = harness.Trainer(model, lr=1e-2, max_iter=10, loss_scale=harness.LossScaler(init_scale=1024.0, growth_interval=3))
    for i in range(2):
        run(tr, model, i)
    path = str(tmp_path / "ck2.pth")
    harness.save_checkpoint(path, model, epoch=0, optimizer=tr)
    ck = torch.load(path, weights_only=True)
    assert set(ck) == {"epoch", "state_dict", "optimizer", "scaler"}
    assert ck["scaler"]["scale"] == 1024.0 and ck["scaler"]["_growth_tracker"] == 2 and ck["scaler"]["growth_interval"] == 3
    loss3 = run(tr, model, 2)
    want = {k: v.clone() for k, v in model.state_dict().items()}
    want_m, want_i = tr.opt.flat_m.clone(), tr.step_info()
    assert want_i["scale"] == 2048.0 and want_i["growth_tracker"] == 0 and want_i["taken"] == 3      # the third step grew it

    model2 = _model(torch.float32)
    tr2 = harness.Trainer(model2, lr=123.0, max_iter=10, loss_scale="dynamic")
    assert tr2.step_info()["scale"] == 65536.0
    epoch, _ = harness.load_checkpoint(path, model2, optimizer=tr2)
    i2 = tr2.step_info()
    assert epoch == 0 and tr2.opt.it == 2 and i2["scale"] == 1024.0 and i2["growth_tracker"] == 2
    assert tr2.scaler.growth_interval == 3
    assert run(tr2, model2, 2) == loss3
    got = model2.state_dict()
    for k, v in want.items():
        assert torch.equal(got[k], v), k
    assert torch.equal(tr2.opt.flat_m, want_m)
    i2 = tr2.step_info()
    assert i2["scale"] == want_i["scale"] and i2["growth_tracker"] == want_i["growth_tracker"]
    assert i2["grad_norm"] == want_i["grad_norm"] and i2["gmul"] == want_i["gmul"]
