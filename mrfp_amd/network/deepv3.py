"""RobustNet's DeepLabV3+ "Baseline" behind the reference's `network.deepv3` surface (reference network/deepv3.py:
DeepV3Plus and its factory functions), executing on the HIP kernels of mrfp_amd/csrc.

Same constructor and forward signatures, module tree and state_dict keys as the reference for the trunks built here:
`mobilenetv2` (network/Mobilenet.py, depthwise convolutions on csrc/conv_dw.hip), `resnet-50` and `resnet-101` (the three-conv
stem), variants `D` (output stride 8) and `D16` (output stride 16).  Any other trunk raises ValueError naming it.

Reference behaviour mirrored on purpose (DESIGN.md section 8 lists the same):
  * `self.wt_layer` is forced to [0]*7 whatever the caller passes (reference deepv3.py:119), so no trunk layer returns a whitened
    map: `w_arr` is always empty and the ISW / IRW covariance layers are never built;
  * hence `cal_covstat=True` runs the trunk on the concatenated list of images and returns 0;
  * `args.use_wtloss` divides a zero loss by len(w_arr) == 0: the returned `wt_loss` is tensor([nan]), as the reference's is;
  * `visualize` returns an empty covariance list.
Extensions beyond the reference: `aux_gts=None` means "use gts" (the reference requires a tensor and substitutes gts only for a
1-D one), and `args=None` means use_wtloss=False.
"""
from __future__ import annotations

import torch
from torch import nn

from .. import ops
from ..config import cfg
from ..conv import wgrad_boundary
from ..deepv3 import _AtrousSpatialPyramidPoolingModule, _ConvBnRelu, _DeepLabBase
from ..loss import ImgWtLossSoftNLL, fused_loss
from . import Mobilenet, Resnet
from .mynn import HipConv2d, Norm2d, freeze_weights, initialize_weights, unfreeze_weights  # noqa: F401
from .wider_resnet import HipDropout2d

__all__ = ["DeepV3Plus", "DeepR50V3PlusD", "DeepR50V3PlusD_OS8", "DeepR101V3PlusD", "DeepR101V3PlusD_OS8",
           "DeepMobileNetV3PlusD", "DeepMobileNetV3PlusD_OS8", "get_final_layer"]


def _dilate_strided(layer, dil):
    """reference deepv3.py:280-292: every stride-2 convolution of `layer` (MobileNetV2: the depthwise one of the first block)
    becomes stride 1 with dilation = padding = dil."""
    for _, m in layer.named_modules():
        if isinstance(m, nn.Conv2d) and m.stride == (2, 2):
            m.dilation, m.padding, m.stride = (dil, dil), (dil, dil), (1, 1)


def _dilate_bottlenecks(layer, dil):
    """reference deepv3.py:340-360: conv2 of every Bottleneck dilated, the downsample convolution at stride 1."""
    for n, m in layer.named_modules():
        if "conv2" in n:
            m.dilation, m.padding, m.stride = (dil, dil), (dil, dil), (1, 1)
        elif "downsample.0" in n:
            m.stride = (1, 1)


class DeepV3Plus(_DeepLabBase):
    """reference network/deepv3.py DeepV3Plus (A: stride 8, B: stride 16, with skip connections)."""

    def __init__(self, num_classes, trunk='resnet-101', criterion=None, criterion_aux=None,
                 variant='D', skip='m1', skip_num=48, wt_layer=[0, 0, 0, 0, 0, 0, 0], args=None):
        super().__init__()
        self.criterion = criterion
        self.criterion_aux = criterion_aux
        self.variant = variant
        self.args = args
        self.trunk = trunk
        self.wt_layer = [0, 0, 0, 0, 0, 0, 0]          # the reference ignores the argument (deepv3.py:119)

        if trunk == 'mobilenetv2':
            channel_3rd = 32
            prev_final_channel = 320
            final_channel = 1280
            mnet = Mobilenet.mobilenet_v2(pretrained=True, iw=self.wt_layer)
            f = mnet.features
            self.layer0 = nn.Sequential(f[0], f[1])
            self.layer1 = nn.Sequential(f[2], f[3], f[4], f[5], f[6])
            self.layer2 = nn.Sequential(f[7], f[8], f[9], f[10])
            self.layer3 = nn.Sequential(f[11], f[12], f[13], f[14], f[15], f[16], f[17])
            self.layer4 = nn.Sequential(f[18])
            self._trunk = [mnet]
            if self.variant == 'D':
                _dilate_strided(self.layer2, 2)
                _dilate_strided(self.layer3, 4)
            elif self.variant == 'D16':
                _dilate_strided(self.layer3, 2)
            else:
                print("Not using Dilation ")
        elif trunk in ('resnet-50', 'resnet-101'):
            channel_3rd = 256
            prev_final_channel = 1024
            final_channel = 2048
            if trunk == 'resnet-50':
                resnet = Resnet.resnet50(wt_layer=self.wt_layer)
                resnet.layer0 = nn.Sequential(resnet.conv1, resnet.bn1, resnet.relu, resnet.maxpool)
            else:
                resnet = Resnet.resnet101(pretrained=True, wt_layer=self.wt_layer)
                resnet.layer0 = nn.Sequential(resnet.conv1, resnet.bn1, resnet.relu1, resnet.conv2, resnet.bn2, resnet.relu2,
                                              resnet.conv3, resnet.bn3, resnet.relu3, resnet.maxpool)
            self._trunk = [resnet]            # kept out of the module tree (the reference drops it too)
            self.layer0 = resnet.layer0
            self.layer1, self.layer2, self.layer3, self.layer4 = resnet.layer1, resnet.layer2, resnet.layer3, resnet.layer4
            if self.variant == 'D':
                _dilate_bottlenecks(self.layer3, 2)
                _dilate_bottlenecks(self.layer4, 4)
            elif self.variant == 'D16':
                _dilate_bottlenecks(self.layer4, 2)
            else:
                print("Not using Dilation ")
        else:
            raise ValueError("Not a valid network arch: %r (built here: 'mobilenetv2', 'resnet-50', 'resnet-101')" % (trunk,))

        os_ = {'D': 8, 'D4': 4, 'D16': 16}.get(self.variant, 32)
        self.output_stride = os_
        self.aspp = _AtrousSpatialPyramidPoolingModule(final_channel, 256, output_stride=os_)
        self.bot_fine = _ConvBnRelu(channel_3rd, 48, 1)
        self.bot_aspp = _ConvBnRelu(1280, 256, 1)
        self.final1 = nn.Sequential(HipConv2d(304, 256, kernel_size=3, padding=1, bias=False), Norm2d(256), nn.ReLU(inplace=True),
                                    HipConv2d(256, 256, kernel_size=3, padding=1, bias=False), Norm2d(256), nn.ReLU(inplace=True))
        self.final2 = nn.Sequential(HipConv2d(256, num_classes, kernel_size=1, bias=True))
        self.dsn = nn.Sequential(
            HipConv2d(prev_final_channel, 512, kernel_size=3, stride=1, padding=1),
            Norm2d(512),
            nn.ReLU(inplace=True),
            HipDropout2d(0.1),
            HipConv2d(512, num_classes, kernel_size=1, stride=1, padding=0, bias=True))
        self.dsn[3].mask_name = "dsn"
        initialize_weights(self.dsn)
        initialize_weights(self.aspp)
        initialize_weights(self.bot_aspp)
        initialize_weights(self.bot_fine)
        initialize_weights(self.final1)
        initialize_weights(self.final2)
        self.eps = 1e-5
        self.whitening = False
        self.three_input_layer = trunk == 'resnet-101'
        self.cov_matrix_layer = []        # wt_layer is all zeros: no ISW / IRW covariance layer is ever built
        self.cov_type = []

    def set_mask_matrix(self):
        for layer in self.cov_matrix_layer:
            layer.set_mask_matrix()

    def reset_mask_matrix(self):
        for layer in self.cov_matrix_layer:
            layer.reset_mask_matrix()

    def _trunk_forward(self, x):
        """layer0..layer4 -> (low-level features, layer3 output for the aux head, layer4 output, w_arr)."""
        if self.trunk == 'mobilenetv2':
            w_arr = []
            t = self.layer0([ops.as_activation(x), w_arr])[0]
        else:
            t, w_arr = self._stem(x)
        # (conv.wgrad_boundary: when backward reaches these activations the stage behind them has queued its deferred weight
        #  gradients, which are then issued as grouped launches)
        x_tuple = self.layer1([wgrad_boundary(t), w_arr])
        low_level = x_tuple[0]
        x_tuple = self.layer2([wgrad_boundary(low_level), w_arr])
        x_tuple = self.layer3([wgrad_boundary(x_tuple[0]), w_arr])
        aux_in = x_tuple[0]
        x_tuple = self.layer4([wgrad_boundary(aux_in), w_arr])
        return low_level, aux_in, wgrad_boundary(x_tuple[0]), x_tuple[1]

    def _aux_loss(self, aux_in, gts, aux_gts):
        """dsn head (3x3 conv + bias -> Norm2d -> ReLU -> Dropout2d(0.1) -> 1x1 conv + bias) and its loss against the labels
        nearest-downsampled to its resolution (reference deepv3.py:430-438)."""
        t = self.dsn[1].fused(self.dsn[0](aux_in), relu=True)
        t = self.dsn[3](t)
        aux_out = self.dsn[4](t)
        if aux_gts is None or aux_gts.dim() == 1:
            aux_gts = gts
        h, w = aux_out.shape[2], aux_out.shape[3]
        Hs, Ws = aux_gts.shape[-2], aux_gts.shape[-1]
        # F.interpolate(mode='nearest') of the label map: ATen's float32 source-index rule, as the activations' nearest resizes use
        th = torch.as_tensor(ops._nearest_table(Hs, h, None), dtype=torch.long, device=aux_gts.device)
        tw = torch.as_tensor(ops._nearest_table(Ws, w, None), dtype=torch.long, device=aux_gts.device)
        if not (isinstance(self.criterion_aux, ImgWtLossSoftNLL) and aux_gts.dtype in (torch.int32, torch.uint8)):
            aux_gts = aux_gts.long()          # a label map; relaxed words [B,H,W] and multi-hot planes [B,C+1,H,W] keep their type
        aux_gts = aux_gts.index_select(-2, th).index_select(-1, tw).contiguous()
        loss = fused_loss(self.criterion_aux, aux_out, aux_gts)
        if loss is None:
            loss = self.criterion_aux(aux_out.float(), aux_gts)
        return loss

    def forward(self, x, gts=None, aux_gts=None, img_gt=None, visualize=False, cal_covstat=False, apply_wtloss=True,
                training=None, low_res=False):
        """training / low_res: the keywords harness.evaluate / harness.evaluate_tta call every model with.  The mode is the
        module's own (self.training, as in the reference); `training`, when given, has to agree with it.  low_res (eval only):
        the head's padded low-resolution class scores instead of the full-size logits (deepv3._DeepLabBase._head)."""
        if training is not None and bool(training) != self.training:
            raise ValueError("training=%r contradicts the module's mode (call .train() / .eval())" % (training,))
        if low_res and self.training:
            raise ValueError("low_res is an eval-path option")
        if cal_covstat:
            x = torch.cat(x, dim=0)
        h, w = x.shape[2], x.shape[3]
        low_level, aux_in, t, w_arr = self._trunk_forward(x)
        if cal_covstat:
            return 0                      # w_arr is empty: no covariance layer to update (reference deepv3.py:395-405)
        t = self.aspp(t)
        dec0_up = self.bot_aspp(t)
        dec0_fine = self.bot_fine(low_level)
        dec1 = self._final1(ops.concat_upsample(dec0_fine, dec0_up, low_level.shape[2:], cfg.MODEL.DECODER_PAD))  # cat([fine, Up(up)], 1)
        use_wtloss = self.args is not None and bool(getattr(self.args, "use_wtloss", False))
        if self.training:
            loss1 = self._head(dec1, (h, w), gts, True)
            loss2 = self._aux_loss(aux_in, gts, aux_gts)
            return_loss = [loss1, loss2]
            if use_wtloss:
                # zero loss over len(w_arr) == 0 whitened maps: the reference's 0 / 0 (deepv3.py:420-428)
                wt_loss = torch.zeros(1, device=loss1.device) / len(w_arr)
                return_loss.append(wt_loss)
                if visualize:
                    return_loss.append([])
            return return_loss
        main_out = self._head(dec1, (h, w), None, False, low_res)
        if visualize:
            return main_out, []
        return main_out


def get_final_layer(model):
    unfreeze_weights(model.final)
    return model.final


def DeepR50V3PlusD_OS8(args, num_classes, criterion, criterion_aux):
    """ResNet-50, output stride 8."""
    print("Model : DeepLabv3+, Backbone : ResNet-50")
    return DeepV3Plus(num_classes, trunk='resnet-50', criterion=criterion, criterion_aux=criterion_aux,
                      variant='D', skip='m1', args=args)


def DeepR50V3PlusD(args, num_classes, criterion, criterion_aux):
    """ResNet-50, output stride 16."""
    print("Model : DeepLabv3+, Backbone : ResNet-50")
    return DeepV3Plus(num_classes, trunk='resnet-50', criterion=criterion, criterion_aux=criterion_aux,
                      variant='D16', skip='m1', args=args)


def DeepR101V3PlusD(args, num_classes, criterion, criterion_aux):
    """ResNet-101 (three-conv stem), output stride 16."""
    print("Model : DeepLabv3+, Backbone : ResNet-101")
    return DeepV3Plus(num_classes, trunk='resnet-101', criterion=criterion, criterion_aux=criterion_aux,
                      variant='D16', skip='m1', args=args)


def DeepR101V3PlusD_OS8(args, num_classes, criterion, criterion_aux):
    """ResNet-101 (three-conv stem), output stride 8."""
    print("Model : DeepLabv3+, Backbone : ResNet-101")
    return DeepV3Plus(num_classes, trunk='resnet-101', criterion=criterion, criterion_aux=criterion_aux,
                      variant='D', skip='m1', args=args)


def DeepMobileNetV3PlusD(args, num_classes, criterion, criterion_aux):
    """MobileNetV2, output stride 16."""
    print("Model : DeepLabv3+, Backbone : mobilenetv2")
    return DeepV3Plus(num_classes, trunk='mobilenetv2', criterion=criterion, criterion_aux=criterion_aux,
                      variant='D16', skip='m1', args=args)


def DeepMobileNetV3PlusD_OS8(args, num_classes, criterion, criterion_aux):
    """MobileNetV2, output stride 8."""
    print("Model : DeepLabv3+, Backbone : mobilenetv2")
    return DeepV3Plus(num_classes, trunk='mobilenetv2', criterion=criterion, criterion_aux=criterion_aux,
                      variant='D', skip='m1', args=args)
