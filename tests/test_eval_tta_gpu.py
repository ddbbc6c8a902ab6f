"""Multi-scale / flipped / sliding-window evaluation on the GPU: ops.prob_accum and ops.acc_argmax_hist against the plain-torch
fp64 restatement (tests/eval_tta_common.py), and harness.evaluate_tta end to end.

Tolerances.
  * exact part (no resize, no flip, weight 1, fp32 scores): 2 ulp of fp32 per element (one exp, one divide) against the fp32
    softmax -- exp(fl32(z - max)) / sum, the exp and the divide evaluated exactly.  torch's own fp32 softmax is 4.2 ulp away from
    that value on the host for these inputs, so it is printed, not used as the 2-ulp reference.  Measured: profiles/eval_tta.md.
  * resized / flipped / weighted / accumulated: |acc - fp64 restatement of the same rounded inputs| <= k * 2^-23 * (sum of the
    weights accumulated into that pixel).  k = 4 x the noise floor of the arithmetic: the largest error, in the same unit, of an
    fp32 torch run of the restatement against the fp64 one over ALL the cases below for that input format -- a property of the
    inputs, not of the kernel.  Floors and the kernel's own figures: profiles/eval_tta.md.
  * end to end: predictions are compared pixel for pixel where the restatement's top-two averaged-probability gap exceeds 1e-5 (a
    margin above the fp32 accumulation error); at most 0.5 % of the pixels may be excluded that way.
"""
import contextlib
import io
import json
import os

import numpy as np
import pytest
import torch

from mrfp_amd import synth

import eval_tta_common as etc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
GAP, CAP = 1e-5, 0.005


def _dev_logits(z):
    """host NHWC-storage scores -> the same storage on the device"""
    return z.to(DEV).contiguous(memory_format=torch.channels_last)


# ------------------------------------------------------------------------------------------------------------------------
# 1. exact part
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ld", [19, 32])
def test_prob_accum_exact_part(ld):
    from mrfp_amd import ops
    B, NC, H, W = 2, 19, 41, 67
    y0, x0, hd, wd = 5, 9, 30, 50
    z = etc.nhwc_logits(B, ld, hd, wd, torch.float32, seed=100 + ld)
    g = torch.Generator().manual_seed(7)
    acc0 = torch.randn(B, H, W, NC, generator=g)
    cnt0 = torch.rand(B, H, W, generator=g)
    acc0[:, y0:y0 + hd, x0:x0 + wd] = 0
    cnt0[:, y0:y0 + hd, x0:x0 + wd] = 0
    acc, cnt = acc0.to(DEV), cnt0.to(DEV)
    zd = _dev_logits(z)
    ops.prob_accum(zd, acc, cnt, (y0, x0, hd, wd))
    # the fp32 softmax the kernel is specified to evaluate -- max-subtracted in fp32 -- with its one exp and its one divide taken
    # exactly (fp64): 2 ulp is the budget of those two operations against THIS value.  torch's own fp32 softmax is printed next
    # to it; it cannot carry a 2-ulp bound itself (on the host it sits 4.2 ulp from the exact value on these very inputs).
    zz = z[:, :NC].permute(0, 2, 3, 1).contiguous()
    t = (zz - zz.amax(-1, keepdim=True)).double()                    # fl32(z - max), then exact
    want = torch.exp(t) / torch.exp(t).sum(-1, keepdim=True)
    got = acc.cpu()[:, y0:y0 + hd, x0:x0 + wd]
    spacing = torch.from_numpy(np.spacing(want.float().numpy())).double()
    ulp = (got.double() - want).abs() / spacing
    dev32 = torch.softmax(zd[:, :NC].permute(0, 2, 3, 1).contiguous(), dim=-1).cpu().double()
    host32 = torch.softmax(zz, dim=-1).double()
    print("exact part ld=%d: max ulp vs exact fp32-softmax %.2f | vs torch fp32 on the device %.2f, on the host %.2f | torch "
          "device vs exact %.2f, torch host vs exact %.2f"
          % (ld, ulp.max().item(), ((got.double() - dev32).abs() / spacing).max().item(),
             ((got.double() - host32).abs() / spacing).max().item(), ((dev32 - want).abs() / spacing).max().item(),
             ((host32 - want).abs() / spacing).max().item()))
    assert ulp.max().item() <= 2.0
    inside = torch.zeros(B, H, W, dtype=torch.bool)
    inside[:, y0:y0 + hd, x0:x0 + wd] = True
    assert torch.equal(cnt.cpu()[inside], torch.ones(int(inside.sum())))
    assert torch.equal(cnt.cpu()[~inside], cnt0[~inside])                                     # untouched outside
    assert torch.equal(acc.cpu()[~inside].view(torch.int32), acc0[~inside].view(torch.int32))      # bit-identical outside


# ------------------------------------------------------------------------------------------------------------------------
# 2. resized / flipped / weighted / accumulated
# ------------------------------------------------------------------------------------------------------------------------
def _case_inputs(case, dtype):
    name, B, NC, ld, hs, ws, H, W, steps = case
    return [etc.nhwc_logits(B, ld, hs, ws, dtype, seed=1000 * i + len(name) + ld) for i in range(len(steps))]


def _restate_case(case, zs, dtype):
    name, B, NC, ld, hs, ws, H, W, steps = case
    acc, cnt = torch.zeros(B, H, W, NC, dtype=dtype), torch.zeros(B, H, W, dtype=dtype)
    for z, (rect, flip, w) in zip(zs, steps):
        etc.accum_restated(z.float(), NC, acc, cnt, rect, flip, w, dtype=dtype)
    return acc, cnt


_FLOOR = {}


def _noise_floor(dtype):
    """largest |fp32 restatement - fp64 restatement| / (2^-23 * cnt) over all cases for this input format"""
    if dtype not in _FLOOR:
        worst = 0.0
        for case in etc.ACCUM_CASES:
            zs = _case_inputs(case, dtype)
            a64, c64 = _restate_case(case, zs, torch.float64)
            a32, _ = _restate_case(case, zs, torch.float32)
            m = c64 > 0
            err = (a32.double() - a64).abs().amax(-1)
            worst = max(worst, (err[m] / (etc.U * c64[m])).max().item())
        _FLOOR[dtype] = worst
    return _FLOOR[dtype]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("case", etc.ACCUM_CASES, ids=[c[0] for c in etc.ACCUM_CASES])
def test_prob_accum_vs_restatement(case, dtype):
    from mrfp_amd import ops
    name, B, NC, ld, hs, ws, H, W, steps = case
    floor = _noise_floor(dtype)
    k = 4.0 * floor
    zs = _case_inputs(case, dtype)
    a64, c64 = _restate_case(case, zs, torch.float64)
    acc = torch.zeros(B, H, W, NC, dtype=torch.float32, device=DEV)
    cnt = torch.zeros(B, H, W, dtype=torch.float32, device=DEV)
    for z, (rect, flip, w) in zip(zs, steps):
        ops.prob_accum(_dev_logits(z), acc, cnt, rect, flip=flip, weight=w)
    got, gotc = acc.cpu().double(), cnt.cpu().double()
    assert torch.equal(gotc, c64)                              # the weights are dyadic: their sums are exact in fp32
    m = c64 > 0
    assert torch.equal(got[~m], torch.zeros_like(got[~m]))     # never-covered pixels stay zero
    err = (got - a64).abs().amax(-1)
    ratio = (err[m] / (etc.U * c64[m])).max().item()
    print("prob_accum %s %s: max err %.3f x 2^-23 x cnt (fp32-torch floor %.3f, gate %.3f)" % (name, dtype, ratio, floor, k))
    assert ratio <= k, (name, dtype, ratio, k)


# ------------------------------------------------------------------------------------------------------------------------
# 3. arg-max / histogram
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("NC,B,H,W", [(19, 2, 37, 53), (2, 1, 5, 301), (32, 3, 16, 16), (19, 1, 1, 1)])
def test_acc_argmax_hist_matches_numpy(NC, B, H, W):
    from mrfp_amd import ops
    g = torch.Generator().manual_seed(NC + H)
    acc = torch.rand(B, H, W, NC, generator=g)
    flat = acc.view(-1, NC)
    n = flat.shape[0]
    for p in range(0, n, 3):                    # exact ties: the maximum is duplicated at a second (sometimes third) class
        mx = flat[p].max()
        flat[p, int(torch.randint(0, NC, (1,), generator=g))] = mx
        if p % 2 == 0:
            flat[p, NC - 1] = mx
    if n > 4:
        flat[4] = 0.25                            # all classes equal: class 0 wins
    label = torch.randint(0, NC, (B, H, W), generator=g)
    r = torch.rand(B, H, W, generator=g)
    label[r < 0.1] = 255                          # ignore label
    label[(r >= 0.1) & (r < 0.2)] = NC            # first label outside the class range
    label[(r >= 0.2) & (r < 0.25)] = -1
    cnt = torch.ones(B, H, W)
    if n > 8:
        cnt.view(-1)[5] = 0
        cnt.view(-1)[8] = 0
    accd, cntd = acc.to(DEV), cnt.to(DEV)
    unc = torch.zeros(1, dtype=torch.int64, device=DEV)
    hist0 = torch.arange(NC * NC, dtype=torch.int64).reshape(NC, NC)
    hist, pred = ops.acc_argmax_hist(accd, cntd, label.to(DEV), hist0.to(DEV), want_pred=True, uncovered=unc)
    want_hist, want_pred = etc.hist_from_acc(accd, label, NC)          # the device's own acc copied to the host
    assert np.array_equal(pred.cpu().numpy().astype(np.int64), want_pred)
    assert np.array_equal(hist.cpu().numpy(), want_hist + hist0.numpy())      # added to
    assert int(unc.item()) == (2 if n > 8 else 0)
    hist2, none = ops.acc_argmax_hist(accd, cntd, label.to(DEV))
    assert none is None and np.array_equal(hist2.cpu().numpy(), want_hist)


# ------------------------------------------------------------------------------------------------------------------------
# 4. / 5. end to end
# ------------------------------------------------------------------------------------------------------------------------
def _mrfp_r50(residual_gain=1.0):
    from mrfp_amd import deepv3
    from mrfp_amd.config import cfg
    cfg.MODEL.ACT_DTYPE = torch.float32
    spec = json.load(open(os.path.join(HERE, "golden", "state_dict_spec.json")))["MRFPPlus"]
    m = deepv3.MRFPPlus(19, criterion=torch.nn.CrossEntropyLoss(ignore_index=255))
    m.load_state_dict(synth.synth_state_dict([(k, tuple(s)) for k, s in spec], seed=0, residual_gain=residual_gain))
    return m.to(DEV)


def _mobilenet():
    import deepv3_common as dc
    from mrfp_amd.config import cfg
    from mrfp_amd.network import deepv3
    cfg.MODEL.ACT_DTYPE = torch.float32
    crit = torch.nn.CrossEntropyLoss(ignore_index=255)
    with contextlib.redirect_stdout(io.StringIO()):
        m = deepv3.DeepMobileNetV3PlusD(None, 19, crit, crit)
    m.load_state_dict(synth.synth_state_dict(dc.spec("DeepMobileNetV3PlusD"), seed=0))
    return m.to(DEV)


MODELS = {"MRFPPlus_r50": _mrfp_r50, "DeepMobileNetV3PlusD": _mobilenet}
HEAD_STRIDE = {"MRFPPlus_r50": 4, "DeepMobileNetV3PlusD": 8}          # resolution of the class scores the head is fed with


def _batches(with_small_label):
    x, y = synth.synth_batch(2, 160, 224, seed=31)
    out = [(x[i:i + 1].to(DEV), y[i:i + 1].to(DEV)) for i in range(2)]
    if with_small_label:
        x2, y2 = synth.synth_batch(1, 160, 224, seed=32)
        out.append((x2.to(DEV), y2[:, :128, :192].contiguous().to(DEV)))
    return out


def _replay(batches, kept, captured, NC=19):
    """Per kept image: the device accumulator rebuilt from the captured low-resolution scores (the launches evaluate_tta issued) and
    the fp64 restatement driven by the SAME scores -> (device hist, device preds, restated preds, gaps, labels)."""
    from mrfp_amd import ops
    hist, out = None, []
    for idx in kept:
        label = batches[idx][1]
        B, Hd, Wd = label.shape
        acc = torch.zeros(B, Hd, Wd, NC, dtype=torch.float32, device=DEV)
        cnt = torch.zeros(B, Hd, Wd, dtype=torch.float32, device=DEV)
        a64, c64 = torch.zeros(B, Hd, Wd, NC, dtype=torch.float64), torch.zeros(B, Hd, Wd, dtype=torch.float64)
        for (s, size, f, win, rect), low in captured[idx]:
            ops.prob_accum(low, acc, cnt, rect, flip=f)
            etc.accum_restated(low.float(), NC, a64, c64, rect, f, 1.0)
        hist, pred = ops.acc_argmax_hist(acc, cnt, label, hist, want_pred=True)
        assert torch.equal(cnt.cpu().double(), c64) and float(c64.min()) >= 1.0
        out.append((pred.cpu().numpy().astype(np.int64), np.argmax(a64.numpy(), -1), etc.top2_gap(a64, c64).numpy(),
                    label.cpu().numpy()))
    return hist.cpu().numpy(), out


def _capture():
    captured = {}

    def hook(idx, var, low):
        captured.setdefault(idx, []).append((var, low))
    return captured, hook


@pytest.mark.parametrize("which", list(MODELS))
def test_evaluate_tta_defaults_equal_evaluate(which):
    """all defaults = one whole-image forward at scale 1: the existing path, up to near-ties of the two best classes"""
    from mrfp_amd import harness, ops
    model = MODELS[which]()
    batches = _batches(True)
    hist_e, miou_e, dropped_e = harness.evaluate(model, batches)
    captured, hook = _capture()
    hist_t, miou_t, dropped_t = harness.evaluate_tta(model, batches, on_variant=hook)
    assert dropped_e == dropped_t == 1 and sorted(captured) == [0, 1]
    st = HEAD_STRIDE[which]
    assert all(len(v) == 1 and v[0][1].shape[2:] == (160 // st, 224 // st) for v in captured.values())      # low-resolution scores, one variant
    hist_r, per = _replay(batches, [0, 1], captured)
    assert np.array_equal(hist_r, hist_t)                       # the replay IS what evaluate_tta ran (bitwise reproducible)
    excluded = total = moved = 0
    for idx, (pred_d, pred_r, gap, label) in zip([0, 1], per):
        with torch.no_grad():
            _, pred_e = ops.argmax_hist(model(batches[idx][0], training=False), batches[idx][1], want_pred=True)
        pred_e = pred_e.cpu().numpy().astype(np.int64)
        clear = gap > GAP
        assert np.array_equal(pred_d[clear], pred_e[clear]) and np.array_equal(pred_d[clear], pred_r[clear])
        excluded += int((~clear).sum())
        total += clear.size
        moved += int(((~clear) & (label >= 0) & (label < 19)).sum())
    print("%s defaults: %d of %d pixels under the %.0e gap (%.4f %%)" % (which, excluded, total, GAP, 100.0 * excluded / total))
    assert excluded <= CAP * total
    assert int(np.abs(hist_t - hist_e).sum()) <= 2 * moved and hist_t.sum() == hist_e.sum()
    if excluded == 0:
        assert np.array_equal(hist_t, hist_e) and miou_t == miou_e


# Models of the full-feature test.  The ResNet-50 MRFP+ takes its synthetic weights at residual_gain 0.3, the regime of a trained
# network that the well-conditioned fixtures use (synth.synth_state_dict).  At gain 1.0 its class scores are saturated (measured on
# an MI355X: |score| up to 156, standard deviation 43), every variant's softmax is one-hot, and the 48-variant average becomes a
# vote count with EXACT ties between two classes: 0.77 % of the pixels sit under the 1e-5 gap (0.35 % even under 1e-6), which trips
# the 0.5 % cap -- a property of those inputs, computed from the fp64 restatement alone (the device and the restatement agreed on
# every pixel above the gap there too).  At gain 0.3: 0 of 96256 pixels under 1e-5; MobileNetV2: 6 of 96256.
FULL_MODELS = {"MRFPPlus_r50_gain0.3": (lambda: _mrfp_r50(0.3), 4), "DeepMobileNetV3PlusD": (_mobilenet, 8)}


@pytest.mark.parametrize("resize_to_label", [False, True])
@pytest.mark.parametrize("which", list(FULL_MODELS))
def test_evaluate_tta_full_feature(which, resize_to_label):
    from mrfp_amd import harness
    make, st = FULL_MODELS[which]
    model = make()
    batches = _batches(True)
    captured, hook = _capture()
    kw = dict(scales=(0.75, 1.0, 1.25), flip=True, window=(96, 96), resize_to_label=resize_to_label)
    hist_t, miou_t, dropped = harness.evaluate_tta(model, batches, on_variant=hook, **kw)
    kept = [0, 1, 2] if resize_to_label else [0, 1]
    assert dropped == 3 - len(kept) and sorted(captured) == kept
    for idx in kept:
        Hd, Wd = batches[idx][1].shape[1:]
        want = harness.tta_variants(160, 224, (Hd, Wd), kw["scales"], True, (96, 96), None)
        assert [v for v, _ in captured[idx]] == want and len(want) == 2 * (6 + 6 + 12)
        assert all(low.shape[2:] == (96 // st, 96 // st) for _, low in captured[idx])
    hist_r, per = _replay(batches, kept, captured)
    assert np.array_equal(hist_r, hist_t)
    excluded = total = 0
    want_hist = np.zeros((19, 19), dtype=np.int64)
    from mrfp_amd import metrics
    for pred_d, pred_r, gap, label in per:
        clear = gap > GAP
        assert np.array_equal(pred_d[clear], pred_r[clear])
        excluded += int((~clear).sum())
        total += clear.size
        pred_w = np.where(clear, pred_r, pred_d)            # the restatement's prediction wherever it is not a near-tie
        want_hist += metrics.fast_hist(pred_w.reshape(-1), label.reshape(-1), 19)
    print("full feature %s (resize_to_label=%s): %d of %d pixels under the %.0e gap (%.4f %%)"
          % (which, resize_to_label, excluded, total, GAP, 100.0 * excluded / total))
    assert excluded <= CAP * total
    assert np.array_equal(hist_t, want_hist)
    assert miou_t == metrics.miou_from_hist(want_hist)


# ------------------------------------------------------------------------------------------------------------------------
# 6. / 7. reproducible, capturable
# ------------------------------------------------------------------------------------------------------------------------
def _accumulate_all(zs, label, steps, B, H, W, NC):
    from mrfp_amd import ops
    acc = torch.zeros(B, H, W, NC, dtype=torch.float32, device=DEV)
    cnt = torch.zeros(B, H, W, dtype=torch.float32, device=DEV)
    for z, (rect, flip, w) in zip(zs, steps):
        ops.prob_accum(z, acc, cnt, rect, flip=flip, weight=w)
    hist, _ = ops.acc_argmax_hist(acc, cnt, label)
    return acc, cnt, hist


def test_bitwise_reproducible():
    name, B, NC, ld, hs, ws, H, W, steps = etc.ACCUM_CASES[2]
    zs = [_dev_logits(z) for z in _case_inputs(etc.ACCUM_CASES[2], torch.bfloat16)]
    label = synth.synth_batch(B, H, W, seed=5)[1].to(DEV)
    a1, c1, h1 = _accumulate_all(zs, label, steps, B, H, W, NC)
    a2, c2, h2 = _accumulate_all(zs, label, steps, B, H, W, NC)
    assert torch.equal(a1.view(torch.int32), a2.view(torch.int32)) and torch.equal(c1, c2) and torch.equal(h1, h2)


def test_graph_capture_replays_to_the_same_result():
    """no allocation, no synchronisation inside the two entry points: they capture on one stream and replay"""
    from mrfp_amd import ops
    name, B, NC, ld, hs, ws, H, W, steps = etc.ACCUM_CASES[0]
    zs = [_dev_logits(z) for z in _case_inputs(etc.ACCUM_CASES[0], torch.float32)]
    label = synth.synth_batch(B, H, W, seed=6)[1].to(DEV)
    a_ref, c_ref, h_ref = _accumulate_all(zs, label, steps, B, H, W, NC)
    acc = torch.zeros(B, H, W, NC, dtype=torch.float32, device=DEV)
    cnt = torch.zeros(B, H, W, dtype=torch.float32, device=DEV)
    hist = torch.zeros(NC, NC, dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                  # one capture stream: a chain, no parallel branches
        for z, (rect, flip, w) in zip(zs, steps):
            ops.prob_accum(z, acc, cnt, rect, flip=flip, weight=w)
        ops.acc_argmax_hist(acc, cnt, label, hist)
    for _ in range(2):                                         # the second replay starts from cleared buffers again
        acc.zero_()
        cnt.zero_()
        hist.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(acc.view(torch.int32), a_ref.view(torch.int32)) and torch.equal(cnt, c_ref)
        assert torch.equal(hist, h_ref)
