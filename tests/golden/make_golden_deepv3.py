#!/usr/bin/env python3
"""Golden vectors for the DeepLabV3+ baseline (reference network/deepv3.py DeepV3Plus, network/Mobilenet.py) -- runs ONLY in
the build container (needs /root/reference).

Imports the reference's `network/deepv3.py` and `network/Mobilenet.py` with four run-time shims (nothing of the reference is
copied): an inert `torchvision` (imported at module level, used only by the resnext / wide-resnet trunks), an inert `kmeans1d`
(imported by network/cov_settings.py; the ISW layer that would call it is never built), `pretrained=False` bound on the trunk
factories (and every checkpoint download replaced by an error), and `Tensor.cuda` as the identity while the script runs (the
training branch calls `.cuda()` on the auxiliary labels).

For DeepMobileNetV3PlusD, DeepMobileNetV3PlusD_OS8 and DeepR50V3PlusD at 2 x 128^2 fp32: per-key synthetic weights
(mrfp_amd.synth), an injected Dropout2d keep-mask for the dsn head, one train forward + backward of loss1 + loss2, the running
statistics after it, and one eval forward.  Asserts that the restatement tests/deepv3_common.py reproduces the reference exactly
(rel 0), then writes tests/golden/deepv3.npz (losses, logit crops and statistics, per-parameter gradient L2, running statistics,
eval logit statistics) and tests/golden/deepv3_spec.json (the key / shape spec of each model).
"""
from __future__ import annotations

import contextlib
import functools
import io
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

from mrfp_amd import synth  # noqa: E402


def _no_download(*a, **k):
    raise RuntimeError("make_golden_deepv3: checkpoint downloads are disabled (pretrained=False is bound)")


def import_reference():
    for name in ("torchvision", "torchvision.models", "kmeans1d"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["torchvision"].models = sys.modules["torchvision.models"]
    import torch.hub
    import torch.utils.model_zoo
    torch.hub.load_state_dict_from_url = _no_download
    torch.utils.model_zoo.load_url = _no_download
    sys.path.insert(0, REF)
    from network import Mobilenet as ref_mnet
    from network import Resnet as ref_resnet
    ref_mnet.load_state_dict_from_url = _no_download
    for mod, fn in ((ref_mnet, "mobilenet_v2"), (ref_resnet, "resnet50"), (ref_resnet, "resnet101")):
        orig = getattr(mod, fn)

        @functools.wraps(orig)
        def bound(*a, _orig=orig, **k):
            k["pretrained"] = False
            return _orig(*a, **k)
        setattr(mod, fn, bound)
    from network import deepv3 as ref_deepv3
    sys.path.remove(REF)
    return ref_deepv3


class _Args:
    use_wtloss = False


def l2(t):
    return t.detach().double().pow(2).sum().sqrt().item()


def rel(a, b):
    return ((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30)).item()


def main():
    import deepv3_common as dc
    ref = import_reference()
    torch.Tensor.cuda = lambda self, *a, **k: self
    crit = torch.nn.CrossEntropyLoss(ignore_index=255)
    specs, fx = {}, {}
    for name, (trunk, variant) in dc.CASES.items():
        torch.manual_seed(0)
        with contextlib.redirect_stdout(io.StringIO()):
            model = getattr(ref, name)(_Args(), dc.NC, crit, crit)
        spec = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
        specs[name] = [[k, list(s)] for k, s in spec]
        json.dump(specs, open(dc.SPEC_PATH, "w"))          # (case_inputs reads it)
        sd, x, y, keep = dc.case_inputs(name)
        model.load_state_dict(sd)
        model.train()
        orig = F.dropout2d
        F.dropout2d = lambda inp, p=0.5, training=True, inplace=False: inp * keep if training else inp
        try:
            loss1, loss2 = model(x, gts=y, aux_gts=y)
        finally:
            F.dropout2d = orig
        (loss1 + loss2).backward()
        grads = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
        running = {k: v.detach().clone() for k, v in model.state_dict().items() if "running" in k}
        model.load_state_dict(sd)
        model.eval()
        with torch.no_grad():
            logits = model(x)

        # the restatement on the same numbers: exact
        leaf = {k: v.clone().requires_grad_(True) for k, v in sd.items() if v.is_floating_point() and "running" not in k}
        work = {k: v.clone() for k, v in sd.items()}
        work.update(leaf)
        ns, taps = {}, {}
        l1, l2_ = dc.deepv3_forward(work, x, trunk, variant, True, gts=y, drop_mask=keep, new_stats=ns, taps=taps)
        (l1 + l2_).backward()
        assert l1.item() == loss1.item() and l2_.item() == loss2.item(), (name, l1.item(), loss1.item(), l2_.item(), loss2.item())
        for k, g in grads.items():
            assert torch.equal(leaf[k].grad, g), (name, k, rel(leaf[k].grad, g))
        assert set(grads) == {k for k, v in leaf.items() if v.grad is not None}, name
        for k, v in running.items():
            assert torch.equal(ns[k], v), (name, k)
        with torch.no_grad():
            lo = dc.deepv3_forward({k: v.clone() for k, v in sd.items()}, x, trunk, variant, False)
        assert torch.equal(lo, logits), (name, rel(lo, logits))
        print("[%s] loss1 %.6f loss2 %.6f  restatement == reference (rel 0)" % (name, loss1.item(), loss2.item()))

        p = name + "/"
        fx[p + "loss1"] = np.float64(loss1.item())
        fx[p + "loss2"] = np.float64(loss2.item())
        fx[p + "train_logits_stats"] = dc.stats(taps["logits"])
        fx[p + "train_logits_crop"] = taps["logits"][:, :4, 60:64, 60:64].detach().numpy()
        fx[p + "aux_logits_stats"] = dc.stats(taps["aux_logits"])
        fx[p + "eval_logits_stats"] = dc.stats(logits)
        fx[p + "eval_logits_crop"] = logits[:, :4, 60:64, 60:64].numpy()
        for k, g in grads.items():
            fx[p + "grad_l2/" + k] = np.float64(l2(g))
        for k in [k for k in running if k.endswith("running_mean")][::7] + [k for k in running if k.endswith("running_var")][::11]:
            fx[p + "running/" + k] = running[k][:8].numpy()
    np.savez_compressed(dc.GOLDEN, **fx)
    print("wrote", dc.GOLDEN, "and", dc.SPEC_PATH)


if __name__ == "__main__":
    main()
