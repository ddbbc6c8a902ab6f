"""DeepLabV3+ with the MRFP+ perturbations (HRFP + NP+), same nn.Module surface, constructor and
forward signatures, attribute names and state_dict keys as the reference's top-level deepv3.py
(reference deepv3.py:64-126 ASPP, 152-367 MRFPPlus, 370-490 simpleDeepV3Plus), running on the
hand-written gfx950 kernels of mrfp_amd/csrc through mrfp_amd/ops.py.

Differences from the reference that a caller can observe (all documented in DESIGN.md):
  * randomness is drawn through `self.rng` (default: python `random` for the three toggles exactly
    as the reference, the torch *device* generator for the HRFP re-initialisation and the NP+
    normals); tests replace it to inject numbers;
  * `trunk='resnet-101'` is accepted as a build-defined extension (BASELINE.json configs 3-4); the
    reference raises ValueError for anything but 'resnet-50' and so does this class for other names;
  * activations are NHWC and may be bf16 (cfg.MODEL.ACT_DTYPE); logits are returned as fp32.
"""
from __future__ import annotations

import math
import random

import torch
from torch import nn

from . import ops
from .config import cfg
from .conv import wgrad_boundary
from .loss import ScoreMap, fused_ce_kwargs, fused_loss, refuse_two_view_criterion
from .network import Resnet
from .network.mynn import (HipBatchNorm2d, HipConv2d, HipInstanceNorm2d, Norm2d, Upsample, conv_norm, initialize_weights,
                           initialize_weights_kaimingnormal_forOC)

__all__ = ["_AtrousSpatialPyramidPoolingModule", "MRFPPlus", "simpleDeepV3Plus", "ReferenceRandom", "InjectedRandom"]


class ReferenceRandom:
    """The reference's three RNG uses inside forward (deepv3.py:281-283, 290-306, 274-275)."""

    _py = random        # python's global stream, as the reference; harness.sync_replicas() installs a shared private one

    def toggles(self):
        return self._py.random(), self._py.random(), self._py.random()

    def seed_toggles(self, seed):
        """Private toggle stream (same seed on every rank of a data-parallel job: all ranks take the same branches)."""
        self._py = random.Random(seed)

    def reinit_hrfp(self, model):
        flat = _hrfp_arena(model)
        if flat is not None:
            # the reference's re-initialiser (mynn.py:57-74: kaiming_normal_ on the eight convolutions, N(0, 0.5) on the BatchNorm
            # weights, zero biases; deepv3.py:291-306) as TWO kernels over one flat arena the 32 tensors are views of -- one normal
            # draw, one multiply by the per-element standard deviation (0 for the biases) -- instead of ~40 launches of ~5 us
            flat[0].normal_()
            flat[0].mul_(flat[1])
        else:
            for conv, bn in model.hrfp_layers():
                initialize_weights_kaimingnormal_forOC(conv)
                initialize_weights_kaimingnormal_forOC(bn)
        from . import conv as conv_mod
        conv_mod.repack_weights([c.weight for c, _ in model.hrfp_layers()], tag="hrfp",
                                biases=[c.bias for c, _ in model.hrfp_layers()])            # one pack launch instead of one per layer

    def np_noise(self, which, B, C, device):
        # torch.normal(mean_tensor, std_tensor) as the reference calls it (deepv3.py:274-275) is, inside ATen,
        # normal_(0, 1).mul_(std).add_(mean) preceded by a host-synchronising check std.min() >= 0; the same draws
        # (same generator consumption) without the two device->host round trips per call:
        # (one draw for both: three launches per call instead of five)
        z = torch.randn(2, B, C, 1, 1, device=device).mul_(0.75)
        alpha, beta_noise = z[0], z[1]
        alpha.add_(1.0)
        return alpha, beta_noise


_HRFP_ARENA = __import__("os").environ.get("MRFP_HRFP_ARENA", "1") != "0"      # (0: the per-module initialiser calls, for A/B runs)


def _hrfp_arena(model):
    """(flat fp32 arena, per-element standard deviation) with the HRFP convolutions' and BatchNorms' parameters as views of the
    arena, or None on the CPU.  Built at the first re-initialisation on the device and rebuilt when ANY parameter's storage was
    replaced (`model.to(...)`, an assignment to one `.data`); in-place updates of the parameters (load_state_dict, broadcasts)
    keep the views.
    RNG-STREAM DEVIATION (stated): the reference draws tensor by tensor in module order (mynn.py:57-74: sixteen
    kaiming_normal_ / normal_ calls); one normal_() over the arena draws the same DISTRIBUTION per tensor but consumes the
    generator differently (bias and padding slots are drawn and multiplied by 0), so a SEEDED run does not reproduce the
    reference's HRFP weights -- nor the NP+ draws behind them -- value for value.  MRFP_HRFP_ARENA=0 keeps the per-module calls
    for seeded parity runs (tests/test_model_gpu.py compares the two initialisers' statistics)."""
    layers = model.hrfp_layers()
    first = layers[0][0].weight
    if not first.is_cuda or not _HRFP_ARENA:
        return None
    params, stds = [], []
    for conv, bn in layers:
        fan_in = conv.weight.shape[1] * conv.weight.shape[2] * conv.weight.shape[3]
        params += [conv.weight, conv.bias, bn.weight, bn.bias]
        stds += [math.sqrt(2.0 / fan_in), 0.0, 0.5, 0.0]           # kaiming_normal_(nonlinearity="relu", mode="fan_in"); N(0, 0.5); zeros
    if any(p is None or p.dtype != torch.float32 for p in params):
        return None
    st = getattr(model, "_hrfp_arena_state", None)
    if st is not None and st[0].device == first.device and st[2] == tuple(p.data_ptr() for p in params):
        return st
    offs, n = [], 0
    for p in params:
        offs.append(n)
        n += (p.numel() + 3) // 4 * 4
    flat = torch.zeros(n, dtype=torch.float32, device=first.device)
    std = torch.zeros(n, dtype=torch.float32, device=first.device)
    with torch.no_grad():
        for p, o, sd in zip(params, offs, stds):
            v = flat[o:o + p.numel()].view(p.shape)
            v.copy_(p.data)
            p.data = v
            std[o:o + p.numel()] = sd
    st = model._hrfp_arena_state = (flat, std, tuple(p.data_ptr() for p in params))
    from . import conv as conv_mod
    conv_mod.invalidate_packs()
    return st


class InjectedRandom(ReferenceRandom):
    """Fixed toggles / NP+ draws (and no HRFP re-draw) -- for parity tests and benchmarks."""

    def __init__(self, toggles=(True, True, True), noise=None, reinit=False):
        self._t, self._noise, self._reinit = toggles, noise, reinit

    def toggles(self):
        return tuple(0.25 if t else 0.75 for t in self._t)

    def reinit_hrfp(self, model):
        if self._reinit:
            super().reinit_hrfp(model)

    def np_noise(self, which, B, C, device):
        if self._noise is None:
            return super().np_noise(which, B, C, device)
        return self._noise[which + "_alpha"].to(device), self._noise[which + "_beta"].to(device)


class _ConvBnRelu(nn.Sequential):
    """Sequential(conv, Norm2d, ReLU) with the BN statistics/apply + ReLU fused (keys .0 / .1)."""

    def __init__(self, cin, cout, k, padding=0, dilation=1):
        super().__init__(HipConv2d(cin, cout, kernel_size=k, padding=padding, dilation=dilation, bias=False),
                         Norm2d(cout), nn.ReLU(inplace=True))

    def forward(self, x):
        return conv_norm(self[0], self[1], x, relu=True)

    def forward_skip(self, x):
        """(module(x), alias of x): gradients arriving on the alias are added by this conv's dgrad epilogue, so a
        tensor with several consumers is chained through them instead of being summed by separate passes."""
        return conv_norm(self[0], self[1], x, want_skip=True, relu=True)


class _AtrousSpatialPyramidPoolingModule(nn.Module):
    """reference deepv3.py:64-126: image pooling + 1x1 + three dilated 3x3 branches, concatenated
    (channel order: img, 1x1, r0, r1, r2)."""

    def __init__(self, in_dim, reduction_dim=256, output_stride=16, rates=(6, 12, 18)):
        super().__init__()
        print("output_stride = ", output_stride)
        if output_stride == 8:
            rates = [2 * r for r in rates]
        elif output_stride == 4:
            rates = [4 * r for r in rates]
        elif output_stride == 16:
            pass
        elif output_stride == 32:
            rates = [r // 2 for r in rates]
        else:
            raise TypeError("output stride of {} not supported".format(output_stride))   # reference raises a str
        feats = [_ConvBnRelu(in_dim, reduction_dim, 1)]
        feats += [_ConvBnRelu(in_dim, reduction_dim, 3, padding=r, dilation=r) for r in rates]
        self.features = nn.ModuleList(feats)
        self.img_pooling = nn.AdaptiveAvgPool2d(1)
        self.img_conv = _ConvBnRelu(in_dim, 256, 1)

    def forward(self, x):
        outs, cur = [], x
        for f in self.features:          # x is chained through its five consumers (see _ConvBnRelu.forward_skip)
            y, cur = f.forward_skip(cur)
            outs.append(y)
        img = self.img_conv(ops.global_avg_pool(cur))
        return ops.concat_channels([Upsample(img, x.shape[2:])] + outs)


class _DeepLabBase(nn.Module):
    # keep_scores = True: a training forward leaves self.last_scores = loss.ScoreMap(dec2, size, classes), the autograd-attached
    # low-resolution class scores the fused loss read, for a second criterion over them (loss.ConsistencyLoss2d through
    # harness.ConsistencyStep).  False, the default: nothing is retained.
    keep_scores = False
    last_scores = None

    def __setattr__(self, name, value):
        if name in ("criterion", "criterion_aux"):
            refuse_two_view_criterion("%s(%s=)" % (type(self).__name__, name), value)
        super().__setattr__(name, value)

    def _keep(self, dec2, size, nc, training):
        if self.keep_scores and training:
            self.last_scores = ScoreMap(dec2, size, nc)

    def _build_trunk_and_head(self, num_classes, trunk, wt_layer):
        if trunk == "wider_resnet38_a2" and self._allow_101:
            return self._build_wrn_trunk_and_head(num_classes)
        if trunk == "resnet-50":
            resnet = Resnet.resnet50(wt_layer=wt_layer)
        elif trunk == "resnet-101" and self._allow_101:
            resnet = Resnet.resnet101(wt_layer=wt_layer)
        else:
            raise ValueError("Not a valid network arch")
        if isinstance(resnet, Resnet.ResNet3X3):
            resnet.layer0 = nn.Sequential(resnet.conv1, resnet.bn1, resnet.relu1, resnet.conv2, resnet.bn2,
                                          resnet.relu2, resnet.conv3, resnet.bn3, resnet.relu3, resnet.maxpool)
        else:
            resnet.layer0 = nn.Sequential(resnet.conv1, resnet.bn1, resnet.relu, resnet.maxpool)
        self._trunk = [resnet]            # kept out of the module tree (the reference drops it too)
        self.layer0 = resnet.layer0
        self.layer1, self.layer2, self.layer3, self.layer4 = resnet.layer1, resnet.layer2, resnet.layer3, resnet.layer4
        if self.variant == "D16":         # reference deepv3.py:184-189
            for n, m in self.layer4.named_modules():
                if "conv2" in n:
                    m.dilation, m.padding, m.stride = (2, 2), (2, 2), (1, 1)
                elif "downsample.0" in n:
                    m.stride = (1, 1)
        else:
            print("Not using Dilation ")
        self.output_stride = 16
        self._build_head(num_classes, 2048)

    def _build_wrn_trunk_and_head(self, num_classes):
        """BUILD-DEFINED composition (BASELINE.json configs[4]; the reference's MRFPPlus only takes resnet-50 and its
        WiderResNet is not wired into any of its DeepLab variants): WiderResNet-38-A2, dilated (output stride 8).
        The trunk is cut where the ResNet trunks are cut: `stem` = mod1 -> pool2 -> mod2 -> pool3 (128 ch, 1/4
        resolution) is what HRFP and the first NP+ see, `mod3` (256 ch, 1/4) plays layer1 (second NP+, low-level
        skip), mod4..mod7 + bn_out (4096 ch, 1/8) feed an output-stride-8 ASPP."""
        from .network import wider_resnet
        wrn = wider_resnet.wider_resnet38_a2(classes=0, dilation=True)
        self._trunk = [wrn]
        for name in ("mod1", "pool2", "mod2", "pool3", "mod3", "mod4", "mod5", "mod6", "mod7", "bn_out"):
            setattr(self, name, getattr(wrn, name))
        self.output_stride = 8
        self._build_head(num_classes, 4096)

    def _build_head(self, num_classes, trunk_channels):
        self.aspp = _AtrousSpatialPyramidPoolingModule(trunk_channels, 256, output_stride=self.output_stride)
        self.bot_fine = _ConvBnRelu(256, 48, 1)
        self.bot_aspp = _ConvBnRelu(1280, 256, 1)
        self.final1 = nn.Sequential(HipConv2d(304, 256, kernel_size=3, padding=1, bias=False), Norm2d(256),
                                    nn.ReLU(inplace=True),
                                    HipConv2d(256, 256, kernel_size=3, padding=1, bias=False), Norm2d(256),
                                    nn.ReLU(inplace=True))
        self.final2 = nn.Sequential(HipConv2d(256, num_classes, kernel_size=1, bias=True))

    def _init_head(self):
        initialize_weights(self.aspp)
        initialize_weights(self.bot_aspp)
        initialize_weights(self.bot_fine)
        initialize_weights(self.final1)
        initialize_weights(self.final2)
        self.eps = 1e-5
        self.whitening = False
        self.three_input_layer = False

    _taps = None        # tests set this to a dict: per-stage activations are recorded there (names as the oracle's taps)

    def _tap(self, name, t):
        if self._taps is not None:
            self._taps[name] = t.detach()

    def _stem(self, x):
        """layer0: conv(s) -> norm -> ReLU -> maxpool (reference deepv3.py:309-315)."""
        trunk = self._trunk[0]
        w_arr = []
        if not isinstance(trunk, (Resnet.ResNet, Resnet.ResNet3X3)):
            return trunk.stem(x), w_arr                # WiderResNet: mod1 -> pool2 -> mod2 -> pool3
        if isinstance(trunk, Resnet.ResNet3X3):
            return trunk.stem(x, w_arr), w_arr
        return Resnet._conv_norm_relu_pool(self.layer0[0], self.layer0[1], trunk.wt_layer[2], ops.as_activation(x), w_arr), w_arr

    def _low(self, t, w_arr):
        """stem output -> low-level features (256 ch, 1/4): layer1 (reference deepv3.py:331-333) / mod3."""
        # (conv.wgrad_boundary: when backward reaches this activation, the stage behind it has queued all its weight gradients and
        #  they are issued as grouped launches -- mrfp_amd/conv.py)
        if hasattr(self, "layer1"):
            return self.layer1([wgrad_boundary(t), w_arr])[0]
        return self.mod3(wgrad_boundary(t))

    def _high(self, t, w_arr, fourier=None):
        """low-level features -> ASPP input: layer2..layer4 (reference deepv3.py:338-344) / mod4..mod7 + bn_out."""
        if hasattr(self, "layer1"):
            t = self.layer2([wgrad_boundary(t), w_arr])
            if fourier is not None:
                t[0] = fourier.at("layer2", t[0])
            self._tap("layer2", t[0])
            t[0] = wgrad_boundary(t[0])
            t = self.layer3(t)
            self._tap("layer3", t[0])
            t[0] = wgrad_boundary(t[0])
            return wgrad_boundary(self.layer4(t)[0])
        t = self.mod7(self.mod6(self.mod5(wgrad_boundary(self.mod4(wgrad_boundary(t))))))
        return wgrad_boundary(self.bn_out[0].fused(t, relu=True))

    def _final1(self, d):
        d = conv_norm(self.final1[0], self.final1[1], d, relu=True)
        return conv_norm(self.final1[3], self.final1[4], d, relu=True)

    def _head(self, dec1, size, gts, training, low_res=False):
        """final2 (1x1 conv + bias) -> bilinear upsample to the input size -> loss or logits (reference
        deepv3.py:360-367).  The low-resolution class scores live in a 32-channel padded buffer so the conv stays
        chunk-aligned; in training with a criterion the fused kernels compute (loss.fused_loss) the upsample and the loss are
        one kernel and the full-resolution logits are never written.  low_res (eval only): return that padded low-resolution buffer
        [B,32,h/4,w/4] itself, in the activation dtype -- harness.evaluate_tta resizes it inside ops.prob_accum."""
        f2 = self.final2[0]
        nc = f2.out_channels
        pitch = (nc + 31) // 32 * 32
        dec2 = ops.conv2d(dec1, f2.weight, f2.bias, f2.stride, f2.padding, f2.dilation, phys_out=pitch)
        if low_res:
            if training:
                raise ValueError("low_res is an eval-path option (training=False)")
            return dec2
        self._keep(dec2, size, nc, training)
        if training and cfg.MODEL.FUSE_UPSAMPLE_CE and fused_ce_kwargs(self.criterion) is not None:
            return fused_loss(self.criterion, dec2, gts, size, nc)
        main_out = ops.upsample_bilinear(dec2, size, channels=nc)
        if training:
            return self._loss(main_out, gts)
        return main_out.float()

    def _head_o2(self, dec1, oc_dec, size, gts, training):
        """final2(Upsample(dec1) + OCout_dec) (reference deepv3.py:355-361) evaluated as
        Upsample(final2_nobias(dec1)) + final2(OCout_dec): the 1x1 convolution commutes with the bilinear
        interpolation, so the 2x upsample and its backward run on the 19 (padded 32) class-score planes instead of on 256
        channels.  Same arithmetic up to fp32 summation order (inside the 1e-3 parity bound, tests/test_model_gpu.py)."""
        from . import conv
        f2 = self.final2[0]
        nc = f2.out_channels
        pitch = (nc + 31) // 32 * 32
        p_low, p_half = conv.shared_conv1x1_pair(dec1, oc_dec, f2.weight, f2.bias, pitch)
        dec2 = ops.upsample_bilinear(p_low, (oc_dec.shape[2], oc_dec.shape[3]), addend=p_half)
        self._keep(dec2, size, nc, training)
        if training and cfg.MODEL.FUSE_UPSAMPLE_CE and fused_ce_kwargs(self.criterion) is not None:
            return fused_loss(self.criterion, dec2, gts, size, nc)
        main_out = ops.upsample_bilinear(dec2, size, channels=nc)
        if training:
            return self._loss(main_out, gts)
        return main_out.float()

    def _loss(self, main_out, gts):
        loss = fused_loss(self.criterion, main_out, gts)
        if loss is None:          # reduction='none', a foreign module: the one stock path, on the full-resolution fp32 logits
            loss = self.criterion(main_out.float(), gts)
        return loss


class MRFPPlus(_DeepLabBase):
    """reference deepv3.py:152-367."""
    _allow_101 = True

    def __init__(self, num_classes, trunk="resnet-50", criterion=None, criterion_aux=None,
                 variant="D16", wt_layer=[0, 0, 4, 4, 4, 0, 0], use_wtloss=False):
        super().__init__()
        self.criterion = criterion
        self.criterion_aux = criterion_aux
        self.variant = variant
        self.wt_layer = wt_layer
        self.use_wtloss = use_wtloss
        self.trunk = trunk
        self._build_trunk_and_head(num_classes, trunk, wt_layer)

        # HRFP: frozen random over-complete auto-encoder (reference deepv3.py:221-237)
        stem_c = 64 if trunk == "resnet-50" else 128
        enc = [(stem_c, 64, 1), (64, 64, 1), (64, 128, 2), (128, 256, 2)]
        dec = [(256, 128, 1), (128, 64, 1), (64, 64, 2), (64, stem_c, 2)]
        for i, (ci, co, d) in enumerate(enc, 1):
            setattr(self, "OClayer%d" % i, HipConv2d(ci, co, kernel_size=3, stride=1, padding=d, dilation=d).requires_grad_(False))
            setattr(self, "OC%d_bn" % i, HipBatchNorm2d(co).requires_grad_(False))
        for i, (ci, co, d) in enumerate(dec, 1):
            setattr(self, "OCdeclayer%d" % i, HipConv2d(ci, co, kernel_size=3, stride=1, padding=d, dilation=d).requires_grad_(False))
            setattr(self, "OC%d_decbn" % i, HipBatchNorm2d(co).requires_grad_(False))
        for conv, bn in self.hrfp_layers():
            initialize_weights_kaimingnormal_forOC(conv)
            initialize_weights_kaimingnormal_forOC(bn)
        self._init_head()
        self.rng = ReferenceRandom()
        self.fourier_perturb = None      # optional build-defined extension (mrfp_amd/perturb.py); off = reference path

    def _fold_skips_hrfp(self):
        return (getattr(self, "_mrfp_fold", False) and not self.training and not torch.is_grad_enabled())

    def hrfp_layers(self):
        """(conv, bn) pairs in the reference's re-initialisation order (deepv3.py:291-306)."""
        enc = [(getattr(self, "OClayer%d" % i), getattr(self, "OC%d_bn" % i)) for i in range(1, 5)]
        dec = [(getattr(self, "OCdeclayer%d" % i), getattr(self, "OC%d_decbn" % i)) for i in range(1, 5)]
        return enc + dec

    def Normalization_Perturbation_Plus(self, feat, which="np1", res=None):
        """reference deepv3.py:268-277 (res: added to the result in the same pass)."""
        B, C = feat.shape[0], feat.shape[1]
        alpha, beta_noise = self.rng.np_noise(which, B, C, feat.device)
        return ops.np_plus(feat, alpha, beta_noise, res)

    def _hrfp(self, xp, h, w, need_out=True, need_dec=True):
        """reference deepv3.py:320-327: conv -> nearest resize -> BN(train stats) -> ReLU, x8.  The resize
        is never materialised on its own: BN statistics and apply read the conv output through the
        nearest index tables.  need_out / need_dec (cfg.MODEL.HRFP_LAZY only): whether OCout / OCout_dec are read."""
        # (folded inference, inference.fold_norms: at training=False nothing reads the branch -- need_out / need_dec are False -- and in
        #  eval() its BatchNorms update no running statistics, so skipping it changes no output and no state)
        lazy = (cfg.MODEL.HRFP_LAZY or self._fold_skips_hrfp()) and self._taps is None
        if lazy and not (need_out or need_dec):
            return None, None, xp
        resize = [dict(scale=1.205), dict(scale=1.2), dict(scale=1.2), dict(size=(int(h / 2), int(w / 2))),
                  dict(size=(int(h / 2), int(w / 2))), dict(scale=0.838), dict(scale=0.798),
                  dict(size=(math.ceil(h / 4), math.ceil(w / 4)))]
        t, dec, xp_alias = xp, None, xp
        for i, ((conv, bn), rs) in enumerate(zip(self.hrfp_layers(), resize)):
            if i == 4 and lazy and not need_out:
                return t, None, xp_alias
            # (the 3x3 convolutions keep the size: the plan of the resize behind this one is known before it runs, and its epilogue
            #  sums its output with the resize's pixel multiplicities -- the BatchNorm then has its statistics: stat_resize)
            plan = ops.nearest_plan(t.shape[2], t.shape[3], device=t.device, **rs)
            stat_resize = plan if bn.training else None
            if i == 0:            # xp also feeds the trunk: the trunk-side gradient rides in this conv's dgrad epilogue
                t, xp_alias = conv.forward_skip(t, stat_resize=stat_resize)
            elif i == 4:          # OCout_dec also feeds the O2 add: same chaining
                t, dec = conv.forward_skip(t, stat_resize=stat_resize)
            else:
                t = conv(t, stat_resize=stat_resize)
            if (plan.Hs, plan.Ws) != tuple(t.shape[2:]):
                plan = ops.nearest_plan(t.shape[2], t.shape[3], device=t.device, **rs)
            t = bn.fused(t, relu=True, plan=plan)
            self._tap("hrfp%d" % i, t)
        return dec, t, xp_alias

    def forward(self, x, gts=None, training=True, low_res=False):
        if low_res and training:
            raise ValueError("low_res is an eval-path option (training=False)")
        p, p2, p3 = self.rng.toggles()
        h, w = x.shape[2], x.shape[3]
        o1, npp, o2 = (training == True and p < 0.5), (training == True and p2 < 0.5), (training == True and p3 < 0.5)  # noqa: E712
        if o1:
            self.rng.reinit_hrfp(self)

        xp, w_arr = self._stem(x)
        fourier = None
        if training == True and self.fourier_perturb is not None:      # noqa: E712  (build-defined extension, default off)
            fp = self.fourier_perturb
            if hasattr(fp, "begin"):            # perturb.MultiResolutionFourier: stem, layer1 and layer2 resolutions
                fp.begin(x.shape[0], True)
                xp = fp.at("stem", xp)
                fourier = fp
            else:                               # a single perturb.FourierAmplitudeMix at the stem
                xp = fp(xp)
        self._tap("stem", xp)
        OCout_dec, OCout, xp = self._hrfp(xp, h, w, o1, o2)   # always computed, as the reference does (no RNG inside), unless HRFP_LAZY
        t = xp
        if npp and o1 and self._taps is None:
            # NP+(xp) + OCout in ONE pass (the per-stage taps of the parity tests want the intermediate: they take the two-pass form)
            t = self.Normalization_Perturbation_Plus(xp, "np1", res=OCout)
        else:
            if npp:
                t = self.Normalization_Perturbation_Plus(xp, "np1")
                self._tap("np1", t)
            if o1:
                t = ops.add(OCout, t)
        tap = getattr(self.layer1[-1], "instance_norm_layer", None) if hasattr(self, "layer1") else None
        if isinstance(tap, HipInstanceNorm2d):
            tap._emit_plane_stats = bool(npp) and fourier is None      # NP+ reads layer1's output next: its apply pass sums it
        t = self._low(t, w_arr)
        if fourier is not None:
            t = fourier.at("layer1", t)
        if npp:
            t = self.Normalization_Perturbation_Plus(t, "np2")
        self._tap("layer1", t)
        dec0_fine, low_level = self.bot_fine.forward_skip(t)      # low-level features: decoder + layer2
        t = self._high(low_level, w_arr, fourier)
        if self.use_wtloss:
            # the reference stores use_wtloss and never reads it (deepv3.py:167); here it keeps the whitened feature maps of
            # the last forward so that a training script can add network.cov_settings.whitening_loss(model.w_arr, layers)
            self.w_arr = w_arr
        self._tap("layer4", t)
        t = self.aspp(t)
        self._tap("aspp", t)
        dec0_up = self.bot_aspp(t)
        dec1 = self._final1(ops.concat_upsample(dec0_fine, dec0_up, low_level.shape[2:], cfg.MODEL.DECODER_PAD))   # cat([dec0_fine, Upsample(dec0_up)], 1)
        self._tap("dec1", dec1)
        if o2:                                         # "+" of MRFP+: deepv3.py:355-357
            if cfg.MODEL.COMMUTE_O2:
                return self._head_o2(dec1, OCout_dec, (h, w), gts, training)
            dec1 = ops.upsample_bilinear(dec1, (int(h / 2), int(w / 2)), addend=OCout_dec)   # one fused pass
        return self._head(dec1, (h, w), gts, training, low_res)


class simpleDeepV3Plus(_DeepLabBase):
    """reference deepv3.py:370-490: the same network without HRFP / NP+."""
    _allow_101 = False

    def __init__(self, num_classes, trunk="resnet-50", criterion=None, criterion_aux=None,
                 variant="D16", wt_layer=[0, 0, 0, 0, 0, 0, 0], use_wtloss=False):
        super().__init__()
        self.criterion = criterion
        self.criterion_aux = criterion_aux
        self.variant = variant
        self.wt_layer = wt_layer
        self.use_wtloss = use_wtloss
        self.trunk = trunk
        self._build_trunk_and_head(num_classes, trunk, wt_layer)
        self._init_head()

    def forward(self, x, gts=None, training=False, low_res=False):
        h, w = x.shape[2], x.shape[3]
        t, w_arr = self._stem(x)
        x_tuple = self.layer1([t, w_arr])
        low_level = x_tuple[0]
        x_tuple = self.layer4(self.layer3(self.layer2(x_tuple)))
        dec0_up = self.bot_aspp(self.aspp(x_tuple[0]))
        dec0_fine = self.bot_fine(low_level)
        dec1 = self._final1(ops.concat_upsample(dec0_fine, dec0_up, low_level.shape[2:], cfg.MODEL.DECODER_PAD))    # cat([dec0_fine, Upsample(dec0_up)], 1)
        return self._head(dec1, (h, w), gts, training, low_res)
