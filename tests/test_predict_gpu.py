"""The prediction path on the GPU: ops.upsample_argmax (mrfp_upsample_argmax) against the chain it replaces -- exactly -- and
against fp64 on the pixels tests/test_predict_cpu.py found decidable; ties, labels, the loss and the confidence; ops.colorize byte for
byte; harness.predict / harness.validate against harness.evaluate on two models.

Bounds.
  * predictions and histograms: equality (the kernel rounds its fp32 interpolation to the storage type, as mrfp_bilinear_fwd does).
  * loss: relative error against an fp64 cross entropy of the materialised logits within predict_common.LOSS_TOL, the bounds of the
    training kernels with the same arithmetic (1e-5 fp32, 2e-3 16-bit).
  * confidence: 2 ulp of fp32 against 1 / sum exp(z - max z) in fp64 on the kernel's own z (the fp32 restatement, rounded to the
    storage type): the bound tests/test_eval_tta_gpu.py holds prob_accum's soft-max to.  Measured: profiles/predict.md.
"""
import contextlib
import io
import json
import math
import os
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from mrfp_amd import synth

import predict_common as pc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
IDS = [c[0] for c in pc.CASES]


def _ops():
    from mrfp_amd import ops
    return ops


def _inputs(case, dtype):
    name, B, Hi, Wi, H, W, C, _ = case
    return pc.to_device(pc.scores(name, dtype), DEV), pc.labels(name, B, H, W, C)


def _chain(P, size, C, target):
    ops = _ops()
    return ops.argmax_hist(ops.upsample_bilinear(P, size, channels=C).float(), target, want_pred=True)


# ------------------------------------------------------------------------------------------------------------------------
# 1. equality with the existing chain; 2. against fp64
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", pc.DTYPES, ids=pc.dname)
@pytest.mark.parametrize("case", pc.CASES, ids=IDS)
def test_equals_the_chain_and_fp64(case, dtype):
    name, B, Hi, Wi, H, W, C, _ = case
    P, y = _inputs(case, dtype)
    yd = y.to(DEV)
    r = _ops().upsample_argmax(P, (H, W), C, yd)
    hist_c, pred_c = _chain(P, (H, W), C, yd)
    assert r.pred.dtype == torch.uint8 and tuple(r.pred.shape) == (B, H, W) and r.conf is None and r.loss_acc is None
    assert torch.equal(r.pred, pred_c) and torch.equal(r.hist, hist_c)
    pred = r.pred.cpu().numpy().astype(np.int64)
    assert int(pred.max()) < C                                     # the pad channels (1e30 / 65504) never show
    z32, am64, decidable = pc.reference(name, dtype)
    assert np.array_equal(pred, np.argmax(z32, axis=-1))           # the restatement is the kernel
    assert np.array_equal(pred[decidable], am64[decidable])
    assert 1.0 - decidable.mean() <= pc.GAP_CAP[dtype]
    assert np.array_equal(r.hist.cpu().numpy(), pc.np_hist(pred, y.numpy(), C))


# ------------------------------------------------------------------------------------------------------------------------
# 3. ties and labels
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", pc.DTYPES, ids=pc.dname)
def test_ties_take_the_first_index(dtype):
    C, ld = 19, 32
    z = torch.full((1, 6, 6, ld), -3.0)
    z[..., C:] = 1000.0                                            # pad channels above every class
    z[0, :3, :, 3] = 5.0
    z[0, :3, :, 7] = 5.0                                           # rows 0..2: classes 3 and 7 tie -> 3
    z[0, 3, :, 18] = -3.0                                          # row 3: every class equal -> 0
    z[0, 4:, :, 18] = 2.0
    z[0, 4:, :, 9] = 2.0                                           # rows 4, 5: 9 and 18 tie -> 9
    P = pc.to_device(z.to(dtype), DEV)
    want = np.repeat(np.array([3, 3, 3, 0, 9, 9])[:, None], 6, axis=1)[None]
    r = _ops().upsample_argmax(P, (6, 6), C)                       # the identity: z is the input
    assert np.array_equal(r.pred.cpu().numpy(), want) and r.hist is None
    # upsampled, with maps that are constant per class: equal classes stay equal through the interpolation
    zc = torch.zeros(2, 3, 5, ld)
    zc[..., C:] = 1000.0
    zc[0, ..., 4] = 6.0
    zc[0, ..., 11] = 6.0                                           # image 0: 4 and 11 tie -> 4; image 1: all equal -> 0
    r = _ops().upsample_argmax(pc.to_device(zc.to(dtype), DEV), (11, 23), C)
    p = r.pred.cpu().numpy()
    assert (p[0] == 4).all() and (p[1] == 0).all()
    assert torch.equal(r.pred, _chain(pc.to_device(zc.to(dtype), DEV), (11, 23), C, None)[1])


def test_labels_outside_the_classes_are_ignored_and_hist_is_added_to():
    ops = _ops()
    case = pc.CASES[0]
    name, B, Hi, Wi, H, W, C, _ = case
    P, y = _inputs(case, pc.F32)
    assert all(int((y == v).sum()) > 0 for v in (255, -1, C, 200))
    hist0 = torch.arange(C * C, dtype=torch.int64).reshape(C, C)
    r = ops.upsample_argmax(P, (H, W), C, y.to(DEV), hist=hist0.to(DEV), loss_acc=True)
    pred = r.pred.cpu().numpy()
    assert np.array_equal(r.hist.cpu().numpy(), hist0.numpy() + pc.np_hist(pred, y.numpy(), C))       # added to, invalid labels nowhere
    valid = (y >= 0) & (y < C)
    assert r.loss_acc.dtype == torch.float64 and float(r.loss_acc[1]) == float(valid.sum())          # 255 is outside 0..C-1 here
    # an ignore_index inside the class range leaves the histogram alone and takes its pixels out of the loss
    r3 = ops.upsample_argmax(P, (H, W), C, y.to(DEV), ignore_index=3, loss_acc=True)
    assert np.array_equal(r3.hist.cpu().numpy(), pc.np_hist(pred, y.numpy(), C))
    assert float(r3.loss_acc[1]) == float((valid & (y != 3)).sum()) < float(valid.sum())
    # all ignored: hist unchanged, no valid pixel, a zero sum
    bad = torch.tensor([255, -1, C, 200])[torch.arange(B * H * W) % 4].reshape(B, H, W)
    ra = ops.upsample_argmax(P, (H, W), C, bad.to(DEV), hist=hist0.to(DEV), loss_acc=True)
    assert torch.equal(ra.hist.cpu(), hist0) and ra.loss_acc.cpu().tolist() == [0.0, 0.0]
    assert torch.equal(ra.pred, r.pred)


@pytest.mark.parametrize("case", [pc.CASES[0], pc.CASES[2], pc.CAPPED_CASES[1]], ids=lambda c: c[0])
def test_per_image_histograms(case):
    ops = _ops()
    name, B, Hi, Wi, H, W, C, _ = case
    P, y = _inputs(case, pc.BF16)
    yd = y.to(DEV)
    pooled = ops.upsample_argmax(P, (H, W), C, yd, want_pred=False)
    per = ops.upsample_argmax(P, (H, W), C, yd, per_image=True, want_pred=False)
    assert pooled.pred is None and tuple(per.hist.shape) == (B, C, C) and tuple(pooled.hist.shape) == (C, C)
    assert torch.equal(per.hist.sum(0), pooled.hist)
    for b in range(B):
        one = ops.upsample_argmax(P[b:b + 1], (H, W), C, yd[b:b + 1], want_pred=False)
        assert torch.equal(one.hist, per.hist[b]), b
    again = ops.upsample_argmax(P, (H, W), C, yd, hist=per.hist, per_image=True, want_pred=False)      # added to
    assert again.hist is per.hist and torch.equal(per.hist.sum(0), 2 * pooled.hist)


# ------------------------------------------------------------------------------------------------------------------------
# 4. loss
# ------------------------------------------------------------------------------------------------------------------------
def _materialised(P, size, C):
    return _ops().upsample_bilinear(P, size, channels=C).float().permute(0, 2, 3, 1).cpu().numpy()


@pytest.mark.parametrize("dtype", pc.DTYPES, ids=pc.dname)
@pytest.mark.parametrize("case", [pc.CASES[0], pc.CASES[2], pc.CASES[3], pc.CAPPED_CASES[1]], ids=lambda c: c[0])
def test_loss_against_fp64_of_the_materialised_logits(case, dtype):
    name, B, Hi, Wi, H, W, C, _ = case
    P, y = _inputs(case, dtype)
    r = _ops().upsample_argmax(P, (H, W), C, y.to(DEV), want_pred=False, loss_acc=True)
    nll, n = pc.fp64_loss_sums(_materialised(P, (H, W), C), y.numpy(), C)
    got_nll, got_n = r.loss_acc.cpu().tolist()
    assert got_n == n and n > 0                                    # pixels: exact
    err = abs(got_nll / got_n - nll / n) / abs(nll / n)
    print("loss %s %s: %.9g vs fp64 %.9g, relative error %.3g (bound %.0e)" % (name, pc.dname(dtype), got_nll / got_n, nll / n, err,
                                                                                pc.LOSS_TOL[dtype]))
    assert err < pc.LOSS_TOL[dtype]


@pytest.mark.parametrize("dtype", pc.DTYPES, ids=pc.dname)
def test_loss_accumulates_over_calls(dtype):
    ops = _ops()
    a, b = pc.CASES[0], pc.CASES[4]                                # both 19 classes
    acc, nll, n = True, 0.0, 0
    for case in (a, b):
        name, B, Hi, Wi, H, W, C, _ = case
        P, y = _inputs(case, dtype)
        acc = ops.upsample_argmax(P, (H, W), C, y.to(DEV), want_pred=False, loss_acc=acc).loss_acc
        s, k = pc.fp64_loss_sums(_materialised(P, (H, W), C), y.numpy(), C)
        nll, n = nll + s, n + k
    got_nll, got_n = acc.cpu().tolist()
    assert got_n == n
    assert abs(got_nll / got_n - nll / n) / abs(nll / n) < pc.LOSS_TOL[dtype]


# ------------------------------------------------------------------------------------------------------------------------
# 5. confidence
# ------------------------------------------------------------------------------------------------------------------------
CONF_ULP = 2.0


@pytest.mark.parametrize("dtype", pc.DTYPES, ids=pc.dname)
@pytest.mark.parametrize("case", [pc.CASES[0], pc.CASES[1], pc.CASES[3], pc.CAPPED_CASES[0]], ids=lambda c: c[0])
def test_confidence_within_two_ulp(case, dtype):
    name, B, Hi, Wi, H, W, C, _ = case
    P, _ = _inputs(case, dtype)
    r = _ops().upsample_argmax(P, (H, W), C, want_conf=True)
    assert r.conf.dtype == torch.float32 and tuple(r.conf.shape) == (B, H, W)
    z = pc.reference(name, dtype)[0].astype(np.float64)
    want = 1.0 / np.exp(z - z.max(-1, keepdims=True)).sum(-1)
    got = r.conf.cpu().numpy()
    ulp = np.abs(got.astype(np.float64) - want) / np.spacing(want.astype(np.float32)).astype(np.float64)
    print("conf %s %s: max %.3f ulp, mean %.3f" % (name, pc.dname(dtype), ulp.max(), ulp.mean()))
    assert ulp.max() <= CONF_ULP
    assert (got > 0).all() and (got <= 1.0).all()


# ------------------------------------------------------------------------------------------------------------------------
# 6. reproducibility and options
# ------------------------------------------------------------------------------------------------------------------------
def test_two_runs_are_bit_identical():
    case = pc.CAPPED_CASES[1]
    name, B, Hi, Wi, H, W, C, _ = case
    P, y = _inputs(case, pc.BF16)
    yd = y.to(DEV)
    runs = [_ops().upsample_argmax(P, (H, W), C, yd, want_conf=True, loss_acc=True) for _ in range(2)]
    assert torch.equal(runs[0].conf.view(torch.int32), runs[1].conf.view(torch.int32))
    assert torch.equal(runs[0].loss_acc.view(torch.int64), runs[1].loss_acc.view(torch.int64))
    assert torch.equal(runs[0].pred, runs[1].pred) and torch.equal(runs[0].hist, runs[1].hist)


@pytest.mark.parametrize("dtype", [pc.F32, pc.BF16], ids=pc.dname)
def test_every_combination_of_outputs(dtype):
    ops = _ops()
    case = pc.CASES[2]
    name, B, Hi, Wi, H, W, C, _ = case
    P, y = _inputs(case, dtype)
    yd = y.to(DEV)
    full = ops.upsample_argmax(P, (H, W), C, yd, want_conf=True, loss_acc=True)
    for want_pred in (False, True):
        for want_conf in (False, True):
            for with_target in (False, True):
                for loss in ((False, True) if with_target else (False,)):
                    if not (want_pred or want_conf or with_target):
                        with pytest.raises(Exception, match="no output requested"):
                            ops.upsample_argmax(P, (H, W), C, want_pred=False)
                        continue
                    r = ops.upsample_argmax(P, (H, W), C, yd if with_target else None, want_pred=want_pred, want_conf=want_conf,
                                            loss_acc=loss)
                    assert (r.pred is not None) == want_pred and (r.conf is not None) == want_conf
                    assert (r.hist is not None) == with_target and (r.loss_acc is not None) == loss
                    if want_pred:
                        assert torch.equal(r.pred, full.pred)
                    if want_conf:
                        assert torch.equal(r.conf.view(torch.int32), full.conf.view(torch.int32))
                    if with_target:
                        assert torch.equal(r.hist, full.hist)
                    if loss:
                        assert torch.equal(r.loss_acc.view(torch.int64), full.loss_acc.view(torch.int64))
    with pytest.raises(Exception, match="target"):
        ops.upsample_argmax(P, (H, W), C, loss_acc=True)
    with pytest.raises(Exception, match="target"):
        ops.upsample_argmax(P, (H, W), C, hist=torch.zeros(C, C, dtype=torch.int64, device=DEV))
    with pytest.raises(Exception, match="NHWC"):
        ops.upsample_argmax(P.contiguous(), (H, W), C)                        # NCHW storage is refused, not converted


def test_c_abi_loss_only_and_refusals_on_the_device():
    """what has no ops spelling: the loss alone (no pred, no hist, no conf); ws missing"""
    from mrfp_amd import _lib
    case = pc.CASES[0]
    name, B, Hi, Wi, H, W, C, _ = case
    P, y = _inputs(case, pc.F16)
    yd = y.to(DEV)
    nb = int(_lib.lib().mrfp_upsample_argmax_nblocks(B, H, W))
    ws = torch.empty(2 * nb, dtype=torch.float32, device=DEV)
    acc = torch.zeros(2, dtype=torch.float64, device=DEV)
    _lib.call("mrfp_upsample_argmax", P.data_ptr(), P.shape[1], yd.data_ptr(), _lib.dt(P), B, Hi, Wi, H, W, C, 255, None, None, None, 0,
              ws.data_ptr(), acc.data_ptr(), _lib.stream())
    want = _ops().upsample_argmax(P, (H, W), C, yd, loss_acc=True).loss_acc
    assert torch.equal(acc.view(torch.int64), want.view(torch.int64))
    with pytest.raises(_lib.MrfpHipError, match="without ws"):
        _lib.call("mrfp_upsample_argmax", P.data_ptr(), P.shape[1], yd.data_ptr(), _lib.dt(P), B, Hi, Wi, H, W, C, 255, None, None, None,
                  0, None, acc.data_ptr(), _lib.stream())


# ------------------------------------------------------------------------------------------------------------------------
# 7. colorize
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("npix", [1, 442, 768 * 768])
def test_colorize_byte_exact(npix):
    from mrfp_amd import predict
    ops = _ops()
    g = torch.Generator().manual_seed(npix)
    pred = torch.randint(0, 256, (npix,), generator=g, dtype=torch.uint8)
    pred[::3] = pred[::3] % 19
    img = torch.randint(0, 256, (npix, 3), generator=g, dtype=torch.uint8)
    pal = predict.Palette(torch.randint(0, 256, (256, 3), generator=g).numpy())
    pd, imd, tab = pred.to(DEV), img.to(DEV), pal.device_table(DEV)
    assert pal.device_table(DEV) is tab                                        # cached
    assert np.array_equal(ops.colorize(pd, tab).cpu().numpy(), pc.np_colorize(pred.numpy(), pal.table))
    assert np.array_equal(pal(pd).cpu().numpy(), pc.np_colorize(pred.numpy(), pal.table))
    for alpha, a in ((0.0, 0), (0.5, 128), (1.0, 256), (0.3, 77)):
        got = ops.colorize(pd, tab, imd, alpha).cpu().numpy()
        assert np.array_equal(got, pc.np_colorize(pred.numpy(), pal.table, img.numpy(), a)), alpha
    assert np.array_equal(ops.colorize(pd, tab, imd, 0.0).cpu().numpy(), img.numpy())
    assert np.array_equal(ops.colorize(pd, tab, imd, 1.0).cpu().numpy(), pc.np_colorize(pred.numpy(), pal.table))
    # misaligned views (byte path) and a given out
    buf = torch.full((3 * npix + 8,), 7, dtype=torch.uint8, device=DEV)
    out = buf[1:1 + 3 * npix].view(npix, 3)
    assert ops.colorize(pd, tab, imd, 0.5, out=out) is out
    assert np.array_equal(out.cpu().numpy(), pc.np_colorize(pred.numpy(), pal.table, img.numpy(), 128))
    assert int(buf[0]) == 7 and (buf[1 + 3 * npix:] == 7).all()                # nothing written outside the view
    pbuf = torch.zeros(npix + 3, dtype=torch.uint8, device=DEV)
    pbuf[3:] = pd
    assert np.array_equal(ops.colorize(pbuf[3:], tab).cpu().numpy(), pc.np_colorize(pred.numpy(), pal.table))
    with pytest.raises(Exception, match="overlaps"):
        ops.colorize(pd, tab, imd, 0.5, out=imd)
    with pytest.raises(ValueError):
        ops.colorize(pd, tab, imd, 1.5)


def test_colorize_image_shape_and_decode_segmap_golden():
    from mrfp_amd import predict
    gold = np.load(pc.FIXTURE)
    mask = torch.from_numpy(gold["mask"]).to(DEV)
    got = predict.decode_segmap(mask, "cityscapes")
    assert got.dtype == np.float64 and np.array_equal(got, gold["rgb"])
    pal = predict.Palette.cityscapes()
    lab = torch.from_numpy(np.tile(gold["mask"], (3, 5))).to(DEV)              # [18,40]
    col = pal(lab)
    assert tuple(col.shape) == (18, 40, 3) and np.array_equal(col.cpu().numpy(), pal.table[lab.cpu().numpy().astype(np.int64)])


def test_label_encoder_inverse_round_trip_on_the_device():
    from mrfp_amd import input_pipeline as ip
    enc = ip.label_encoder("CityscapesSegmentation")
    inv = enc.inverse()
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(0, 34, (37, 53), generator=g, dtype=torch.uint8)
    train = enc(ids.to(DEV))
    back = inv(train).cpu().numpy()
    t = train.cpu().numpy()
    valid = t != 255
    assert valid.any() and (~valid).any()
    assert np.array_equal(back[valid], ids.numpy()[valid]) and (back[~valid] == 0).all()


# ------------------------------------------------------------------------------------------------------------------------
# 8. model level
# ------------------------------------------------------------------------------------------------------------------------
def _mrfp_r50(dtype):
    from mrfp_amd import deepv3
    from mrfp_amd.config import cfg
    cfg.MODEL.ACT_DTYPE = dtype
    spec = json.load(open(os.path.join(HERE, "golden", "state_dict_spec.json")))["MRFPPlus"]
    with contextlib.redirect_stdout(io.StringIO()):
        m = deepv3.MRFPPlus(19, criterion=torch.nn.CrossEntropyLoss(ignore_index=255))
    m.load_state_dict(synth.synth_state_dict([(k, tuple(s)) for k, s in spec], seed=0))
    return m.to(DEV)


def _mobilenet(dtype):
    import deepv3_common as dc
    from mrfp_amd.config import cfg
    from mrfp_amd.network import deepv3
    cfg.MODEL.ACT_DTYPE = dtype
    crit = torch.nn.CrossEntropyLoss(ignore_index=255)
    with contextlib.redirect_stdout(io.StringIO()):
        m = deepv3.DeepMobileNetV3PlusD(None, 19, crit, crit)
    m.load_state_dict(synth.synth_state_dict(dc.spec("DeepMobileNetV3PlusD"), seed=0))
    return m.to(DEV)


MODELS = {"MRFPPlus_r50": (_mrfp_r50, 1, 128, 160), "DeepMobileNetV3PlusD": (_mobilenet, 2, 96, 128)}


@pytest.fixture
def _restore_dtype():
    from mrfp_amd.config import cfg
    yield
    cfg.MODEL.ACT_DTYPE = torch.float32


@pytest.mark.parametrize("dtype", [pc.F32, pc.BF16], ids=pc.dname)
@pytest.mark.parametrize("which", list(MODELS))
def test_validate_and_predict_equal_evaluate(which, dtype, _restore_dtype):
    from mrfp_amd import harness, ops
    from mrfp_amd.inference import fold_norms
    make, B, H, W = MODELS[which]
    model = make(dtype)
    batches = []
    for seed in (41, 42):
        x, y = synth.synth_batch(B, H, W, seed=seed)
        batches.append((x.to(DEV), y.to(DEV)))
    x, y = synth.synth_batch(B, H, W, seed=43)
    batches.append((x.to(DEV), y[:, :H - 32, :W - 32].contiguous().to(DEV)))      # label size differs: dropped
    model.train()
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    for fold in (False, True):
        hist_e, miou_e, dropped_e = harness.evaluate(model, batches, fold=fold)
        model.train()
        v = harness.validate(model, batches, fold=fold)
        assert model.training and all(m.training for m in model.modules())
        assert dropped_e == v["dropped"] == 1
        assert np.array_equal(v["hist"], hist_e) and v["mean_iu"] == miou_e
        assert "image_hists" not in v
        # the loss, pooled over the kept batches, against torch on the full-size logits of the stock path
        nll, n = 0.0, 0
        preds_e = []
        model.eval()
        with torch.no_grad(), (fold_norms(model) if fold else contextlib.nullcontext()):
            for img, label in batches[:2]:
                logits = model(img, training=False)
                assert logits.dtype == torch.float32
                nll += float(F.cross_entropy(logits.double(), label, ignore_index=255, reduction="sum"))
                n += int((label != 255).sum())
                preds_e.append(ops.argmax_hist(logits, None, want_pred=True)[1])
        model.train()
        assert v["pixels"] == n
        err = abs(v["val_loss"] - nll / n) / abs(nll / n)
        print("%s %s fold=%s: val_loss %.9g vs torch %.9g (relative %.3g), mIoU %.6f" % (which, pc.dname(dtype), fold, v["val_loss"],
                                                                                           nll / n, err, v["mean_iu"]))
        assert err < pc.LOSS_TOL[dtype]
        got = list(harness.predict(model, (b[0] for b in batches[:2]), fold=fold, want_conf=(not fold)))
        assert model.training and len(got) == 2
        for (pred, conf), want in zip(got, preds_e):
            assert torch.equal(pred, want) and (conf is None) == fold
            if conf is not None:
                assert conf.dtype == torch.float32 and tuple(conf.shape) == tuple(pred.shape) and float(conf.min()) > 0 and float(conf.max()) <= 1
    vp = harness.validate(model, batches, per_image=True)
    assert tuple(vp["image_hists"].shape) == (2 * B, 19, 19) and np.array_equal(vp["image_hists"].sum(0), vp["hist"])
    assert np.array_equal(vp["hist"], harness.validate(model, batches)["hist"])
    if which == "DeepMobileNetV3PlusD" and dtype == pc.F32:
        dead = [(batches[0][0], torch.full_like(batches[0][1], 255))]
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)                      # the mean IoU of an empty histogram (metrics.py)
            vd = harness.validate(model, dead)
        assert vd["pixels"] == 0 and math.isnan(vd["val_loss"]) and int(vd["hist"].sum()) == 0 and vd["dropped"] == 0
        none = harness.validate(model, batches[2:])
        assert none["hist"] is None and none["mean_iu"] == 0.0 and none["dropped"] == 1 and math.isnan(none["val_loss"])
    after = model.state_dict()
    assert all(torch.equal(before[k], after[k]) for k in before)                 # parameters and buffers untouched
