"""Train-step and eval harness against numbers captured from the reference's
optimiser loop (torch.optim.SGD + LambdaLR poly 0.9 on the reference module, tests/golden/make_golden.py)."""
import json
import os

import numpy as np
import pytest
import torch

from mrfp_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT_DIR = os.path.dirname(HERE)
G = np.load(os.path.join(HERE, "golden", "mrfp_c1.npz"))
SPEC = json.load(open(os.path.join(HERE, "golden", "state_dict_spec.json")))


def _model():
    from mrfp_amd import deepv3
    from mrfp_amd.config import cfg
    cfg.MODEL.ACT_DTYPE = torch.float32
    m = deepv3.MRFPPlus(19, criterion=torch.nn.CrossEntropyLoss(ignore_index=255))
    sd = synth.synth_state_dict([(k, tuple(s)) for k, s in SPEC["MRFPPlus"]], seed=0)
    m.load_state_dict(sd)
    return m.to(DEV), sd


def _check_trajectory(losses, tag):
    """Each loss must be as close to the fp64 evaluation of the reference's loop as the reference's own fp32 run is
    (x3 slack, + 1e-3 relative floor).  Measured (make_golden.py): at lr 1e-4 the reference's third fp32 loss is
    2.6e-3 off the fp64 one, at lr 1e-2 the trajectory is chaotic (a 1-ulp change of the update moves it 3e-3)."""
    ref32, ref64 = G[f"{tag}_losses"], G[f"{tag}_losses64"]
    for i, l in enumerate(losses):
        band = 3 * abs(ref32[i] - ref64[i]) + 1e-3 * abs(ref64[i])
        assert abs(l - ref64[i]) <= band, (tag, i, l, ref32[i], ref64[i])
    assert abs(losses[0] - ref32[0]) / ref32[0] < 1e-4      # the first step has no accumulated history


def test_three_train_steps_low_lr_match_reference_sgd():
    """lr 1e-4 (the well-conditioned pin, see make_golden.py): losses and parameter heads after 3 iterations of
    zero_grad -> backward -> fused SGD(momentum .9, wd 5e-4) -> poly LR."""
    from mrfp_amd.deepv3 import InjectedRandom
    from mrfp_amd.harness import Trainer
    model, sd0 = _model()
    model.train()
    tr = Trainer(model, lr=1e-4)
    toggles = [(True, True, True), (False, True, False), (True, False, True)]
    losses = []
    for i in range(3):
        x, y = synth.synth_batch(2, 256, 256, seed=10 + i)
        model.rng = InjectedRandom(toggles[i], synth.synth_noise(2, seed=20 + i))
        losses.append(tr.step(x.to(DEV), y.to(DEV)).item())
    _check_trajectory(losses, "train3lo")
    msd = model.state_dict()
    # parameter updates: checked element-wise on the well-conditioned head of the network (the stem-side updates
    # inherit the 2.5e-2 gradient noise of fp32 and then feed a chaotic trajectory; the optimiser arithmetic itself
    # is pinned exactly by test_fused_sgd_matches_torch_optim below)
    for k in ("final2.0.weight", "final2.0.bias", "final1.4.weight"):
        ref_head = G[f"train3lo_param_head/{k}"]
        delta = float(G[f"train3lo_param_delta_l2/{k}"])
        got = msd[k].flatten()[:8].cpu().numpy()
        # the update itself (not just the parameter) must agree: compare the deltas against the tensor's delta RMS
        d_got, d_ref = got - sd0[k].flatten()[:8].numpy(), ref_head - sd0[k].flatten()[:8].numpy()
        rms = delta / np.sqrt(msd[k].numel())
        np.testing.assert_allclose(d_got, d_ref, rtol=0.05, atol=0.15 * rms + 1e-9, err_msg=k)
    assert int(msd["layer1.0.bn1.num_batches_tracked"]) == int(G["train3lo_nbt"])
    assert tr.opt.it == 3 and abs(tr.opt.lr - 1e-4 * (1 - 3 / 40000) ** 0.9) < 1e-12


def test_fused_sgd_matches_torch_optim():
    """mrfp_sgd_step over the flat arena == torch.optim.SGD(momentum .9, wd 5e-4) + LambdaLR(poly .9), 3 steps."""
    from mrfp_amd.harness import FlatSGD
    torch.manual_seed(0)
    net = torch.nn.Sequential(torch.nn.Linear(37, 19), torch.nn.Linear(19, 5))
    ref = torch.nn.Sequential(torch.nn.Linear(37, 19), torch.nn.Linear(19, 5))
    ref.load_state_dict(net.state_dict())
    net = net.to(DEV)
    opt = FlatSGD(net, lr=1e-2, max_iter=10)
    ropt = torch.optim.SGD(ref.parameters(), lr=1e-2, momentum=0.9, weight_decay=5e-4)
    sched = torch.optim.lr_scheduler.LambdaLR(ropt, lr_lambda=lambda it: (1 - it / 10) ** 0.9)
    for step in range(3):
        x = torch.randn(11, 37)
        opt.zero_grad()
        net(x.to(DEV)).pow(2).sum().backward()
        opt.step(gscale=1.0)
        ropt.zero_grad()
        ref(x).pow(2).sum().backward()
        ropt.step()
        sched.step()
        for p, q in zip(net.parameters(), ref.parameters()):
            torch.testing.assert_close(p.detach().cpu(), q.detach(), rtol=2e-5, atol=1e-6)
    # gscale folds the data-parallel 1/world averaging into the update
    opt.zero_grad()
    net(torch.ones(3, 37, device=DEV)).sum().backward()
    before = opt.flat_p.clone()
    g = opt.flat_g.clone()
    m = opt.flat_m.clone()
    lr = opt.lr
    opt.step(gscale=0.25)
    exp_m = 0.9 * m + (0.25 * g + 5e-4 * before)
    torch.testing.assert_close(opt.flat_p, before - lr * exp_m, rtol=1e-5, atol=1e-7)


def test_reference_recipe_lr_runs_and_tracks_reference():
    """lr 1e-2 (the reference's recipe): the trajectory is chaotic with synthetic weights (a 1-ulp change of the
    update moves loss 3 by 3e-3, measured in make_golden.py) -> loose, stated tolerance 2e-2."""
    from mrfp_amd.deepv3 import InjectedRandom
    from mrfp_amd.harness import Trainer
    model, _ = _model()
    model.train()
    tr = Trainer(model, lr=1e-2)
    toggles = [(True, True, True), (False, True, False), (True, False, True)]
    losses = []
    for i in range(3):
        x, y = synth.synth_batch(2, 256, 256, seed=10 + i)
        model.rng = InjectedRandom(toggles[i], synth.synth_noise(2, seed=20 + i))
        losses.append(tr.step(x.to(DEV), y.to(DEV)).item())
    _check_trajectory(losses, "train3")


def test_eval_harness_hist_miou_and_checkpoint_roundtrip(tmp_path):
    from mrfp_amd import harness
    model, sd = _model()
    x, y = synth.synth_batch(2, 256, 256, seed=1)
    # one image per eval iteration like the reference loop (bs 1), one with a mismatching label size (dropped)
    batches = [(x[i:i + 1].to(DEV), y[i:i + 1].to(DEV)) for i in range(2)]
    batches.append((x[:1].to(DEV), y[:1, :128].to(DEV)))
    hist, miou, dropped = harness.evaluate(model, batches)
    assert dropped == 1
    assert np.abs(hist - G["eval_hist"]).sum() <= 0.002 * hist.sum()
    assert abs(100 * miou - 100 * float(G["eval_miou"])) < 0.1
    path = str(tmp_path / "ck.pth")
    harness.save_checkpoint(path, model, epoch=3)
    ck = torch.load(path, weights_only=False)
    assert set(ck) == {"epoch", "state_dict"} and all(k.startswith("module.") for k in ck["state_dict"])
    assert len(ck["state_dict"]) == 431
    from mrfp_amd import deepv3
    m2 = deepv3.MRFPPlus(19).to(DEV)
    epoch, _ = harness.load_checkpoint(path, m2)
    assert epoch == 3
    with torch.no_grad():
        m2.eval()
        l1 = m2(x.to(DEV), training=False)
        model.eval()
        l0 = model(x.to(DEV), training=False)
    assert torch.equal(l0, l1)


def test_graph_mode_matches_eager():
    """Trainer.enable_graph(): zero_grad + forward + backward captured into a hipGraph per toggle combination and
    replayed; with fixed noise and no HRFP re-draw the captured kernels are the eager ones, so losses and parameters
    after 5 steps (two toggle combinations, each seen before and after its capture) must be bitwise identical."""
    from mrfp_amd.deepv3 import InjectedRandom
    from mrfp_amd.harness import Trainer
    toggles = [(True, True, True), (False, True, False), (True, True, True), (False, True, False), (True, True, True)]
    x, y = synth.synth_batch(2, 128, 128, seed=3)
    x, y = x.to(DEV), y.to(DEV)
    noise = {k: v.to(DEV) for k, v in synth.synth_noise(2, seed=4).items()}
    out = []
    for graph in (False, True):
        model, _ = _model()
        model.train()
        tr = Trainer(model, lr=1e-3)
        if graph:
            tr.enable_graph()
        losses = []
        for i in range(5):
            model.rng = InjectedRandom(toggles[i], noise)
            losses.append(float(tr.step(x, y)))
        sd = model.state_dict()
        out.append((losses, sd["final2.0.weight"].clone(), sd["layer1.0.conv1.weight"].clone(),
                    int(sd["layer1.0.bn1.num_batches_tracked"]), sd["layer1.0.bn1.running_mean"].clone()))
    assert out[0][0] == out[1][0], (out[0][0], out[1][0])
    assert torch.equal(out[0][1], out[1][1]) and torch.equal(out[0][2], out[1][2])
    assert out[0][3] == out[1][3] == 5 and torch.equal(out[0][4], out[1][4])
    # the captured graphs are CHAINS: no fork / join pair (= no cross-stream dependency a replay would have to honour across
    # hardware queues; the round-2 capture had one pair per parameter and crashed in hipGraphLaunch with one queue: DESIGN.md section 5)
    from mrfp_amd.harness import graph_topology
    assert len(tr._graphs) == 2
    for entry in tr._graphs.values():
        topo = graph_topology(entry[0])
        assert topo["nodes"] > 500 and topo["forks"] == 0 and topo["joins"] == 0 and topo["roots"] == 1, topo


def test_graph_mode_with_hrfp_redraw_inside_the_graph():
    """The bench's configuration of graph mode: the HRFP weights are re-drawn at the start of every forward (reference
    deepv3.py:290-306) INSIDE the captured graph (graph-safe Philox), followed by the batched re-pack of their convolution packs --
    whose job table is built the first time the packs exist when the re-initialisation runs, i.e. during the capture pass (pinned
    staging + asynchronous copy: a legal memcpy node).  Replays must re-draw (the weights change from step to step) and train."""
    from mrfp_amd.deepv3 import InjectedRandom
    from mrfp_amd.harness import Trainer
    x, y = synth.synth_batch(2, 128, 128, seed=3)
    x, y = x.to(DEV), y.to(DEV)
    model, _ = _model()
    model.train()
    tr = Trainer(model, lr=1e-3).enable_graph()
    model.rng = InjectedRandom((True, True, True), None, reinit=True)
    losses, ws = [], []
    for _ in range(4):
        losses.append(float(tr.step(x, y)))
        ws.append(model.OClayer1.weight.detach().clone())
    assert all(np.isfinite(losses)), losses
    assert len(tr._graphs) == 1
    assert not torch.equal(ws[1], ws[2]) and not torch.equal(ws[2], ws[3])          # replays re-draw


def test_graph_mode_with_one_hardware_queue_in_subprocess():
    """GPU_MAX_HW_QUEUES=1 (read by the HIP runtime at start-up: a child process): capture + three replays of the ResNet-50 step
    must run and reproduce the eager losses bit for bit -- with the round-2 capture this configuration crashed inside
    hipGraphLaunch."""
    import subprocess
    import sys
    code = (
        "import os, sys, json, torch\n"
        "sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import test_harness_gpu as t\n"
        "from mrfp_amd import synth\n"
        "from mrfp_amd.deepv3 import InjectedRandom\n"
        "from mrfp_amd.harness import Trainer\n"
        "x, y = synth.synth_batch(2, 128, 128, seed=3); x, y = x.cuda(), y.cuda()\n"
        "noise = {k: v.cuda() for k, v in synth.synth_noise(2, seed=4).items()}\n"
        "res = []\n"
        "for graph in (False, True):\n"
        "    model, _ = t._model(); model.train(); tr = Trainer(model, lr=1e-3)\n"
        "    if graph: tr.enable_graph()\n"
        "    model.rng = InjectedRandom((True, True, True), noise)\n"
        "    res.append([float(tr.step(x, y)) for _ in range(4)])\n"
        "torch.cuda.synchronize()\n"
        "assert res[0] == res[1], res\n"
        "print('ok', os.environ.get('GPU_MAX_HW_QUEUES'))\n") % (ROOT_DIR, HERE)
    env = dict(os.environ, GPU_MAX_HW_QUEUES="1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "ok 1" in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-2000:])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_training_reduces_the_loss(dtype):
    """End-to-end sanity of the whole loop (forward, backward, fused SGD, weight repack, loss scaling for float16): 30
    steps on one fixed synthetic batch with the reference's random toggles, HRFP re-draws and NP+ noise must bring the
    loss well below its starting value."""
    import random
    from mrfp_amd import deepv3
    from mrfp_amd.config import cfg
    from mrfp_amd.harness import Trainer
    cfg.MODEL.ACT_DTYPE = dtype
    try:
        torch.manual_seed(0)
        random.seed(0)
        m = deepv3.MRFPPlus(19, criterion=torch.nn.CrossEntropyLoss(ignore_index=255)).to(DEV).train()
        tr = Trainer(m, lr=1e-2)
        x, y = synth.synth_batch(4, 128, 128, seed=3)
        y = (y.clamp(max=18) // 6).clamp(max=2)          # 3 classes in large blobs are learnable in a few steps
        x, y = x.to(DEV), y.to(DEV)
        losses = [float(tr.step(x, y).detach()) for _ in range(30)]
    finally:
        cfg.MODEL.ACT_DTYPE = torch.float32
    assert all(np.isfinite(losses)), losses
    assert min(losses[-5:]) < 0.6 * losses[0], losses


def test_resume_from_checkpoint_reproduces_step_4_bit_for_bit(tmp_path):
    """reference main.py:867-869 / 884-886: {'epoch', 'state_dict', 'optimizer'}.  3 steps -> save -> fresh process
    state (new model, new Trainer) -> load -> step 4 must equal step 4 of the uninterrupted run BIT FOR BIT (weights,
    BN running statistics, momentum arena, schedule position); and the 'optimizer' entry must be loadable by a stock
    torch.optim.SGD over model.parameters()."""
    from mrfp_amd import harness
    from mrfp_amd.deepv3 import InjectedRandom
    toggles = [(True, True, True), (False, True, False), (True, False, True), (True, True, False)]
    data = [synth.synth_batch(2, 128, 128, seed=30 + i) for i in range(4)]
    noise = [synth.synth_noise(2, seed=40 + i) for i in range(4)]

    def run(tr, model, i):
        model.rng = InjectedRandom(toggles[i], noise[i])
        return float(tr.step(data[i][0].to(DEV), data[i][1].to(DEV)))

    model, _ = _model()
    model.train()
    tr = harness.Trainer(model, lr=1e-2, max_iter=10)          # a short schedule: the LR factor moves visibly per step
    for i in range(3):
        run(tr, model, i)
    path = str(tmp_path / "ck3.pth")
    harness.save_checkpoint(path, model, epoch=0, optimizer=tr)
    loss4 = run(tr, model, 3)
    want = {k: v.clone() for k, v in model.state_dict().items()}
    want_m = tr.opt.flat_m.clone()

    ck = torch.load(path, weights_only=False)
    assert set(ck) == {"epoch", "state_dict", "optimizer"}
    osd = ck["optimizer"]
    assert len(osd["state"]) == 192 and osd["mrfp_iteration"] == 3
    assert abs(osd["param_groups"][0]["lr"] - 1e-2 * harness.poly_lr_factor(3, 10)) < 1e-15

    model2, _ = _model()
    model2.train()
    tr2 = harness.Trainer(model2, lr=123.0, max_iter=10)       # wrong on purpose: everything must come from the checkpoint
    epoch, _ = harness.load_checkpoint(path, model2, optimizer=tr2)
    assert epoch == 0 and tr2.opt.it == 3 and tr2.opt.base_lr == 1e-2
    loss4b = run(tr2, model2, 3)
    assert loss4b == loss4
    got = model2.state_dict()
    for k, v in want.items():
        assert torch.equal(got[k], v), k
    assert torch.equal(tr2.opt.flat_m, want_m)

    stock = torch.optim.SGD(model2.parameters(), lr=1e-2, momentum=0.9, weight_decay=5e-4)
    stock.load_state_dict({k: v for k, v in osd.items() if k != "mrfp_iteration"})
    bufs = [st["momentum_buffer"] for st in stock.state_dict()["state"].values()]
    assert len(bufs) == 192


def test_grouped_deferred_weight_gradients_equal_the_per_layer_launches():
    """conv.GROUP_WGRAD: with a gradient arena present backward only queues its weight gradients; a stage's repeated blocks
    (reference network/Resnet.py:579-585) leave as ONE mrfp_conv_wgrad_grouped launch per conv position when backward crosses the
    stage boundary.  Against the per-layer launches: every dgrad / normalisation gradient bit-identical (they do not depend on
    it), every weight gradient equal up to the fp32 association of its K' splits, two grouped runs bit-identical."""
    from mrfp_amd import conv
    from mrfp_amd.deepv3 import InjectedRandom
    from mrfp_amd.harness import Trainer
    x, y = synth.synth_batch(2, 128, 128, seed=3)
    x, y = x.to(DEV), y.to(DEV)
    noise = {k: v.to(DEV) for k, v in synth.synth_noise(2, seed=4).items()}
    model, _ = _model()
    model.train()
    tr = Trainer(model, lr=1e-3)
    model.rng = InjectedRandom((True, True, True), noise)
    was = conv.GROUP_WGRAD[0]
    grads, groups = [], []
    try:
        for on in (False, True, True):
            conv.GROUP_WGRAD[0] = on
            conv.WGRAD_GROUP_LAUNCHES.clear()
            loss = tr._fwd_bwd(x, y)
            torch.cuda.synchronize()
            assert not conv._WGRADS.queues and not conv.GRAD_DEFERRED
            grads.append((float(loss), tr.opt.flat_g.clone()))
            groups.append(list(conv.WGRAD_GROUP_LAUNCHES))
    finally:
        conv.GROUP_WGRAD[0] = was
    # ResNet-50 layer3: conv3 of all six blocks, conv1 / conv2 of blocks 1..5 share a geometry; the second grouped pass knows the
    # counts from the first (singletons leave at once, full groups as soon as they are complete): same launches, same bits
    assert groups[0] == [] and max(groups[1]) == 6 and sorted(groups[1]) == sorted(groups[2])
    assert sum(groups[1]) == sum(1 for p in tr.opt.params if p.dim() == 4) - 1      # every conv weight but the shared final2 pair
    assert grads[0][0] == grads[1][0] == grads[2][0]
    assert torch.equal(grads[1][1], grads[2][1])
    off, on = grads[0][1], grads[1][1]
    for p, o in zip(tr.opt.params, tr.opt.offsets):
        a, b = off[o:o + p.numel()], on[o:o + p.numel()]
        if p.dim() == 4:
            assert ((a - b).abs().max() / a.abs().max().clamp_min(1e-30)).item() < 2e-5
        else:
            assert torch.equal(a, b)


def test_two_trainers_and_two_input_shapes_interleaved_with_grouping_on():
    """the deferred weight-gradient queues learn how many problems of a geometry a backward pass produces from
    the previous pass OF THE SAME KIND (conv._WGRADS.expect_all, keyed by the pass's first weight-gradient geometry).  Two Trainers
    (two models) and two input shapes alternating in one process: every pass must reproduce, bit for bit, the gradients the same
    model / shape gives when it runs alone, leave no queue behind, and -- from its second occurrence on -- issue the same grouped
    launches as when it runs alone (no late or early flush on the other pass's counts)."""
    from mrfp_amd import conv
    from mrfp_amd.deepv3 import InjectedRandom
    from mrfp_amd.harness import Trainer
    assert conv.GROUP_WGRAD[0]
    shapes = [(2, 128, 128), (2, 96, 160)]
    data = []
    for i, (b, h, w) in enumerate(shapes):
        x, y = synth.synth_batch(b, h, w, seed=5 + i)
        data.append((x.to(DEV), y.to(DEV), {k: v.to(DEV) for k, v in synth.synth_noise(b, seed=7 + i).items()}))
    trainers = []
    for _ in range(2):
        model, _sd = _model()
        model.train()
        trainers.append((model, Trainer(model, lr=1e-3)))

    def one(ti, si):
        model, tr = trainers[ti]
        x, y, noise = data[si]
        model.rng = InjectedRandom((True, True, True), noise)
        conv.WGRAD_GROUP_LAUNCHES.clear()
        loss = tr._fwd_bwd(x, y)
        torch.cuda.synchronize()
        assert not conv._WGRADS.queues and not conv.GRAD_DEFERRED and not conv._WGRADS.callback_queued
        return float(loss), tr.opt.flat_g.clone(), sorted(conv.WGRAD_GROUP_LAUNCHES)

    # alone: each (trainer, shape) twice in a row -- the second pass is the steady state of that kind
    alone = {}
    for ti in range(2):
        for si in range(2):
            one(ti, si)
            alone[(ti, si)] = one(ti, si)
    # interleaved: every switch changes model and / or shape
    order = [(0, 0), (1, 1), (0, 1), (1, 0), (0, 0), (1, 1), (0, 1), (1, 0)]
    for ti, si in order:
        loss, g, groups = one(ti, si)
        ref = alone[(ti, si)]
        assert loss == ref[0] and torch.equal(g, ref[1]), (ti, si)
        assert groups == ref[2], (ti, si, groups, ref[2])       # the expectation of this kind of pass was learnt in the `alone` phase
    assert len(conv._WGRADS.expect_all) <= 64


def test_a_backward_pass_that_raises_leaves_no_deferred_state_behind():
    """a backward that dies must not leave queued weight gradients for the next forward convolution to find (and a
    forward convolution issued INSIDE a backward pass -- recomputation -- must not be taken for the sign of a dead one)."""
    import warnings
    from mrfp_amd import conv
    from mrfp_amd.deepv3 import InjectedRandom
    from mrfp_amd.harness import Trainer
    x, y = synth.synth_batch(2, 128, 128, seed=3)
    x, y = x.to(DEV), y.to(DEV)
    noise = {k: v.to(DEV) for k, v in synth.synth_noise(2, seed=4).items()}
    model, _ = _model()
    model.train()
    tr = Trainer(model, lr=1e-3)
    model.rng = InjectedRandom((True, True, True), noise)
    loss0 = float(tr._fwd_bwd(x, y))
    g0 = tr.opt.flat_g.clone()

    class Boom(RuntimeError):
        pass

    fired = []

    def hook(_g):
        # a legitimate forward convolution from inside backward (activation recomputation) ...
        assert conv._in_backward()
        q = sum(len(v) for v in conv._WGRADS.queues.values())
        with torch.no_grad():
            conv.conv2d(torch.zeros(1, 64, 8, 8, device=DEV).contiguous(memory_format=torch.channels_last),
                        torch.zeros(64, 64, 1, 1, device=DEV), None, 1, 0, 1)
        assert sum(len(v) for v in conv._WGRADS.queues.values()) == q        # ... did not drop the queues
        fired.append(q)
        raise Boom("injected")

    # the hook sits on layer3's input: by then the head, ASPP, layer4 and layer3 have queued their weight gradients
    h = model.layer3[0].conv1.weight.register_hook(lambda g: g)       # (keeps the parameter's node alive; no-op)
    handle = []
    orig = model.layer2.forward

    def fwd(*a, **k):
        out = orig(*a, **k)
        t = out[0] if isinstance(out, (list, tuple)) else out
        handle.append(t.register_hook(hook))
        return out
    model.layer2.forward = fwd
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            with pytest.raises(Boom):
                tr._fwd_bwd(x, y)
        assert fired and not conv._WGRADS.queues and not conv.GRAD_DEFERRED and not conv._WGRADS.callback_queued
        if fired[0]:
            assert any("queued weight gradients" in str(i.message) for i in w)
    finally:
        model.layer2.forward = orig
        for hd in handle:
            hd.remove()
        h.remove()
    # the next pass is a clean one
    assert float(tr._fwd_bwd(x, y)) == loss0 and torch.equal(tr.opt.flat_g, g0)
