"""Host-side operator layer: torch.autograd.Functions over the C ABI of libmrfp_hip.so.

Activations are torch tensors of logical shape [B,C,H,W] in channels_last memory format, i.e.
physically NHWC -- the layout every kernel in mrfp_amd/csrc assumes.  PyTorch is used here for
device memory (caching allocator), streams and the autograd tape only; every arithmetic op on
an activation goes through a hand-written HIP kernel, and a missing library raises
(mrfp_amd/_lib.py) -- there is no eager / CPU fallback.
"""
from __future__ import annotations

import collections
import math
import os
import weakref
from functools import lru_cache
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import call, dt, ptr, stream
from .skipgrad import ALIAS, GATE, AliasCell, gateable, mask_possible, ungate

CL = torch.channels_last

# Direct gradient sinks: when the harness has placed a parameter's .grad inside its flat fp32 arena
# (harness.FlatArena sets `_mrfp_direct`), backward kernels write the parameter gradient straight into that view
# (no temporary, no autograd accumulate kernel) and report it through GRAD_NOTIFY (data-parallel bucket counting).
GRAD_NOTIFY = [None]
GRAD_DEFERRED = set()      # id(param) of weights whose gradient launch is queued (conv._WGRADS.submit): not written yet -- autograd's
                           # post-accumulate hook fires for them all the same and must not count them as arrived (harness.GradSync)


def wgrad_workspace(M, N, Q, device, n=1):
    """Scratch of one mrfp_conv_wgrad (n = 1) / mrfp_conv_wgrad_grouped launch: n problems of M pixels, N output channels, Q = R*S*C."""
    return torch.empty(int(_lib.lib().mrfp_conv_wgrad_grouped_ws_bytes(M, N, Q, n)), dtype=torch.uint8, device=device)


def grad_sink(param):
    """The tensor a backward kernel should write d(param) into, or None for the ordinary autograd return path."""
    if param is not None and getattr(param, "_mrfp_direct", False) and param.grad is not None \
            and param.grad.dtype == torch.float32 and param.grad.is_contiguous():
        return param.grad
    return None


def notify_grad(param):
    if GRAD_NOTIFY[0] is not None:
        GRAD_NOTIFY[0](param)


# ------------------------------------------------------------------------------------------
# layout helpers
# ------------------------------------------------------------------------------------------
def to_cl(x: torch.Tensor) -> torch.Tensor:
    """Dense NHWC storage for a logical NCHW tensor (no copy if already so)."""
    if x.dim() != 4:
        raise ValueError("expected a 4-D activation, got %s" % (tuple(x.shape),))
    return x.contiguous(memory_format=CL)


def empty_cl(B, C, H, W, dtype, device) -> torch.Tensor:
    return torch.empty((B, C, H, W), dtype=dtype, device=device, memory_format=CL)


def zeros_cl(B, C, H, W, dtype, device) -> torch.Tensor:
    return torch.zeros((B, H, W, C), dtype=dtype, device=device).permute(0, 3, 1, 2)


def _chk(x: torch.Tensor, name="x") -> torch.Tensor:
    if not x.is_cuda:
        raise _lib.MrfpHipError("%s must live on the GPU (got %s): the HIP path has no CPU fallback" % (name, x.device))
    cell = getattr(x, ALIAS, None)
    if cell is not None:          # a convolution's skip alias (conv.conv2d(..., want_skip=True)): count the operators that consume it
        cell.use()
    if x.dim() != 4 or not x.is_contiguous(memory_format=CL):
        x = to_cl(x)
    return x


def _f32(t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    if t is None:
        return None
    return t.detach().float().contiguous()


# ------------------------------------------------------------------------------------------
# nearest-neighbour resize plans (HRFP, reference deepv3.py:320-327)
# ------------------------------------------------------------------------------------------
def nearest_out_size(in_size: int, scale: float) -> int:
    """ATen: floor(in * scale_factor) in double."""
    return int(math.floor(float(in_size) * scale))


def _nearest_table(in_size: int, out_size: int, scale: Optional[float]) -> np.ndarray:
    """ATen nearest rule in float32: src = min(floor(dst * s), in-1), s = 1/scale_factor if a scale
    factor was given else in/out."""
    s = np.float32(1.0 / scale) if scale is not None else np.float32(in_size) / np.float32(out_size)
    src = np.floor(np.arange(out_size, dtype=np.float32) * s).astype(np.int64)
    return np.minimum(src, in_size - 1).astype(np.int32)


def _inverse_table(tab: np.ndarray, in_size: int) -> np.ndarray:
    """[2*in]: half-open destination range reading each source index (tab is non-decreasing)."""
    lo = np.searchsorted(tab, np.arange(in_size), side="left")
    hi = np.searchsorted(tab, np.arange(in_size), side="right")
    return np.stack([lo, hi], 1).astype(np.int32).reshape(-1)


class NearestPlan:
    """Index tables of one F.interpolate(mode='nearest') call, resident on the device."""

    def __init__(self, Hs, Ws, Ho, Wo, scale, device):
        self.Hs, self.Ws, self.Ho, self.Wo = Hs, Ws, Ho, Wo
        th, tw = _nearest_table(Hs, Ho, scale), _nearest_table(Ws, Wo, scale)
        self.tabH = torch.from_numpy(th).to(device)
        self.tabW = torch.from_numpy(tw).to(device)
        self.invH = torch.from_numpy(_inverse_table(th, Hs)).to(device)
        self.invW = torch.from_numpy(_inverse_table(tw, Ws)).to(device)
        mh, mw = np.bincount(th, minlength=Hs), np.bincount(tw, minlength=Ws)
        self._mult = np.outer(mh, mw)          # how many destination pixels read each source pixel
        self._mult_dev = {}

    def multiplicity(self, B):
        """uint8 [B*Hs*Ws + 256] on the device (zero padding: mrfp_conv_fwd_wstats reads whole tiles), or None when a pixel
        is read more than 255 times: the weights with which statistics over the SOURCE equal statistics over the resized tensor."""
        if B not in self._mult_dev:
            if self._mult.max() > 255:
                self._mult_dev[B] = None
            else:
                flat = np.zeros(B * self.Hs * self.Ws + 256, dtype=np.uint8)
                flat[:B * self.Hs * self.Ws] = np.tile(self._mult.astype(np.uint8).reshape(-1), B)
                self._mult_dev[B] = torch.from_numpy(flat).to(self.tabH.device)
        return self._mult_dev[B]


@lru_cache(maxsize=256)
def _plan_cached(Hs, Ws, Ho, Wo, scale, device_str):
    return NearestPlan(Hs, Ws, Ho, Wo, scale, torch.device(device_str))


def nearest_plan(Hs: int, Ws: int, *, scale: Optional[float] = None, size: Optional[Tuple[int, int]] = None,
                 device="cuda") -> NearestPlan:
    if scale is not None:
        Ho, Wo = nearest_out_size(Hs, scale), nearest_out_size(Ws, scale)
    else:
        Ho, Wo = int(size[0]), int(size[1])
    return _plan_cached(Hs, Ws, Ho, Wo, scale, str(device))


# ------------------------------------------------------------------------------------------
# statistics plumbing
# ------------------------------------------------------------------------------------------
def _geom(x, plan: Optional[NearestPlan]):
    B, C, Hs, Ws = x.shape
    if plan is None:
        return B, Hs, Ws, C, Hs, Ws, None, None, None, None
    if (plan.Hs, plan.Ws) != (Hs, Ws):
        raise _lib.MrfpHipError("resize plan %dx%d does not match input %dx%d" % (plan.Hs, plan.Ws, Hs, Ws))
    return B, plan.Ho, plan.Wo, C, Hs, Ws, plan.tabH, plan.tabW, plan.invH, plan.invW


def _stats_ws(B, Ho, C, device):
    nslab = int(_lib.lib().mrfp_stats_nslab(B, Ho))
    return nslab, torch.empty(B * nslab * 2 * C, dtype=torch.float32, device=device)


def _stats_fwd(x, plan):
    B, Ho, Wo, C, Hs, Ws, tH, tW, _, _ = _geom(x, plan)
    nslab, ws = _stats_ws(B, Ho, C, x.device)
    call("mrfp_stats_fwd", ptr(x), dt(x), B, Ho, Wo, C, Hs, Ws, ptr(tH), ptr(tW), ptr(ws), stream())
    return nslab, ws


def _stats_bwd(dy, x, y, mean, per_image, plan, fA=None, fS=None):
    B, Ho, Wo, C, Hs, Ws, tH, tW, _, _ = _geom(x, plan)
    nslab, ws = _stats_ws(B, Ho, C, x.device)
    call("mrfp_stats_bwd", ptr(dy), ptr(x), ptr(y), ptr(mean), ptr(fA), ptr(fS), int(per_image), dt(x), B, Ho, Wo, C,
         Hs, Ws, ptr(tH), ptr(tW), ptr(ws), stream())
    return nslab, ws


PLANE_STATS = [os.environ.get("MRFP_PLANE_STATS", "1") != "0"]
PLANE_STATS_HITS = [0]        # statistics passes replaced by the producing apply pass's sums (tests)


def _take_planestats(x):
    """(nslab, ws) for x when the apply pass that produced it also wrote the partial sums of its stored output
    (mrfp_affine_fwd_stats: bit for bit the rows of mrfp_stats_fwd(x)), else None."""
    ps = getattr(x, "_mrfp_planestats", None)
    if ps is None or not PLANE_STATS[0] or ps[2] != x._version:
        return None
    PLANE_STATS_HITS[0] += 1
    return ps[0], ps[1]


def _planestats_rows(x, want):
    """(nslab, ws) for the plane sums of an apply pass over x's geometry (the wrapper allocates them, hands ws to its Function,
    which fills it, and tags the tensor it gets back: autograd re-wraps the output, so forward cannot tag it), or None."""
    if not (want and PLANE_STATS[0]):
        return None
    B, C, H, W = x.shape
    return _stats_ws(B, H, C, x.device)


def _tag_planestats(y, ps):
    if ps is not None:
        y._mrfp_planestats = (ps[0], ps[1], y._version)
    return y


def _serving_colstats(x, C, elements, plan, per_image):
    """The statistics the producing convolution's epilogue wrote (x._mrfp_colstats, a conv.ConvStats) if they serve this consumer,
    else None: x as the convolution returned it (version stamp), summed over `elements` values per channel, weighted for exactly
    the resize this consumer applies (`plan`; statistics weighted for a resize serve that one layer only), with whole rows of C
    channels.  per_image: the consumer needs the raw per-row-block rows (InstanceNorm), else the rows for a BatchNorm finalize."""
    cs = getattr(x, "_mrfp_colstats", None)
    if cs is None or cs.version != x._version or cs.resize_plan is not plan or cs.elements != elements:
        return None
    if not per_image:
        return cs if cs.final.numel() == cs.final_count * 2 * C else None
    # (16-bit activations only: behind the stem convolutions a channel's mean is tens of its standard deviations -- inputs are
    #  0..255 -- and the fp32 parity criteria of the ill-conditioned fixture resolve the SUMMATION ORDER of its statistics:
    #  with the epilogue's sums the stem weight gradient of mrfp_c1 moved 0.37 from fp64 where 3x the reference's own fp32
    #  distance allows 0.19; bf16 storage rounds 10^4 times coarser than that)
    return cs if IN_FUSED_STATS[0] and x.element_size() == 2 and cs.rows.numel() >= cs.row_blocks * 2 * C else None


def channel_sums(dy, n):
    """fp32 [n]: the sums of dy's first n channels over batch and pixels -- the bias gradient of a convolution.  The statistics pass
    and a BatchNorm finalize without weights give the column means; times the count."""
    B, C, H, W = dy.shape
    nslab, ws = _stats_fwd(dy, None)
    out = torch.empty(4 * C, dtype=torch.float32, device=dy.device)
    call("mrfp_bn_finalize", ptr(ws), B, nslab, B * H * W, C, None, None, 0.0, 0.0, None, None,
         ptr(out[:C]), ptr(out[C:2 * C]), ptr(out[2 * C:3 * C]), ptr(out[3 * C:]), stream())
    return out[:n] * float(B * H * W)


def _grad_dest(param, wanted, tmp):
    """Where a backward kernel writes d(param): the parameter's slot in the flat gradient arena (grad_sink) or the temporary."""
    sink = grad_sink(param) if wanted else None
    return sink if sink is not None else tmp


def _grad_result(param, dest):
    """After the launches that wrote `dest` (_grad_dest): what backward returns for d(param) -- None for a gradient that went to the
    arena, which is reported (notify_grad) instead."""
    if param is None:
        return None
    if getattr(param, "_mrfp_direct", False) and dest is param.grad:
        notify_grad(param)
        return None
    return dest


def _affine_fwd(x, res, A, S, per_image, relu, plan, like=None, stats=None):
    """stats: rows (_planestats_rows) that also receive the partial plane sums of the stored output."""
    src = x if x is not None else like
    B, Ho, Wo, C, Hs, Ws, tH, tW, _, _ = _geom(src, plan)
    y = empty_cl(B, C, Ho, Wo, src.dtype, src.device)
    if stats is not None:
        call("mrfp_affine_fwd_stats", ptr(x), ptr(res), ptr(y), dt(src), B, Ho, Wo, C, ptr(A), ptr(S), int(per_image), int(relu),
             ptr(stats), stream())
        return y
    call("mrfp_affine_fwd", ptr(x), ptr(res), ptr(y), dt(src), B, Ho, Wo, C, Hs, Ws, ptr(tH), ptr(tW),
         ptr(A), ptr(S), int(per_image), int(relu), stream())
    return y


def _affine_bwd(dy, x, y, P, Q, R, per_image, plan, want_dres, like, fA=None, fS=None):
    B, Ho, Wo, C, Hs, Ws, _, _, iH, iW = _geom(like, plan)
    dx = empty_cl(B, C, Hs, Ws, dy.dtype, dy.device)
    dres = empty_cl(B, C, Ho, Wo, dy.dtype, dy.device) if want_dres else None
    call("mrfp_affine_bwd", ptr(dy), ptr(x), ptr(y), ptr(dx), ptr(dres), dt(dy), B, Ho, Wo, C, Hs, Ws,
         ptr(iH), ptr(iW), ptr(P), ptr(Q), ptr(R), ptr(fA), ptr(fS), int(per_image), stream())
    return dx, dres


# ------------------------------------------------------------------------------------------
# BatchNorm (+ nearest resize in front) (+ residual) (+ ReLU)
# ------------------------------------------------------------------------------------------
SIGN_MASK = [os.environ.get("MRFP_SIGN_MASK", "1") != "0"]     # residual BatchNorm+ReLU: 1-bit sign mask instead of y in backward
GATED_SKIP = [os.environ.get("MRFP_GATED_SKIP", "1") != "0"]   # ... and the skip gradient gated by the consuming dgrad epilogue


SYNC_BN_CALLS = [0]       # BatchNorm layers that exchanged their statistics across ranks (tests)


_SYNC_BN_GROUP = [None]     # the statistics' own communicator (created once, collectively, at the first synchronised layer)
_SYNC_BN_COUNTS = {}        # (local element count, world) -> element count over all ranks
_SYNC_BN_FLAG = {}          # device -> int32[1]: number of layers whose all-reduced count differed from the cached one (device side)
_SYNC_BN_POLL = {}          # device -> (pinned int32[1], event) of the asynchronous read-back in flight


def sync_bn_poll(block=False):
    """Raise if a SYNC_BN layer has seen an all-reduced element count that differs from the one cached for its shape (a rank with a
    partial last batch).  The comparison runs ON THE DEVICE in every synchronised layer; this function looks at its result without a
    host synchronisation of its own: it checks the asynchronous read-back started by the previous call if that has landed, and starts
    the next one (harness.Trainer.step calls it once per step, so a mismatch raises one or two steps after it happened);
    block=True waits for the flag as it stands now (tests, the end of a run)."""
    for dev, flag in list(_SYNC_BN_FLAG.items()):
        pend = _SYNC_BN_POLL.get(dev)
        if block:
            bad = int(flag.item())
            _SYNC_BN_POLL.pop(dev, None)
        else:
            bad = 0
            if pend is not None and pend[1].query():
                bad = int(pend[0].item())
                pend = None
            if pend is None:
                host = torch.empty(1, dtype=torch.int32, pin_memory=True)
                host.copy_(flag, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(torch.cuda.current_stream(dev))
                _SYNC_BN_POLL[dev] = (host, ev)
        if bad:
            flag.zero_()
            raise _lib.MrfpHipError("SYNC_BN: the element count over all ranks differed from the cached one in %d layer call(s) -- a rank "
                                    "ran a batch of another size; uneven per-rank batches are not supported (use a drop_last loader)" % bad)


def _sync_bn_group():
    """The process group BatchNorm statistics are summed over, or None: cfg.MODEL.SYNC_BN (the reference's syncbn switch,
    config.py:92-93: torch.nn.SyncBatchNorm) with more than one rank.  Off by default: 16 images per GPU is the reference's
    own statistical population; it matters for per-GPU batches below that (configs[4]: 2 images).
    The statistics travel on their OWN communicator, never on the one harness.GradSync issues its hook-driven bucket all-reduces
    on: a bucket whose gradients arrive in a rank-dependent order (a tensor without gradient on one rank) is launched at a
    rank-dependent point between two BatchNorm collectives, and on one communicator that would mis-pair them."""
    import torch.distributed as dist
    from .config import cfg
    if not cfg.MODEL.SYNC_BN or not dist.is_available() or not dist.is_initialized():
        return None
    if dist.get_world_size() < 2 and os.environ.get("MRFP_FORCE_SYNC") != "1":     # (forced: the one-rank rehearsal over RCCL)
        return None
    if _SYNC_BN_GROUP[0] is None:
        _SYNC_BN_GROUP[0] = dist.new_group()        # collective: every rank reaches its first synchronised layer in the same forward
    return _SYNC_BN_GROUP[0]


def _allreduce_stats(ws, rows, C, count, group):
    """Per-channel (sum, second sum) partial rows of THIS rank -> the same two sums over all ranks, as a 2-row workspace (fp32
    high part + remainder of the fp64 totals, which the finalize kernels add in fp64) and the global element count.  A few KB:
    torch ops + one all-reduce of 2 C + 1 doubles (torch.nn.SyncBatchNorm exchanges the same quantities).  The global count is
    read back from the device ONCE per local count (one host synchronisation per layer shape, in the first step) and cached:
    per-rank batch sizes are fixed over a run (drop_last loaders, as the reference's, main.py:424-430)."""
    import torch.distributed as dist
    tot = torch.zeros(2 * C + 1, dtype=torch.float64, device=ws.device)
    tot[:2 * C] = ws.view(rows, 2 * C).sum(0, dtype=torch.float64)
    tot[2 * C] = float(count)
    dist.all_reduce(tot, group=group)
    hi = tot[:2 * C].float()
    lo = (tot[:2 * C] - hi.double()).float()
    SYNC_BN_CALLS[0] += 1
    total = 0
    if count:
        # UNEVEN PER-RANK BATCHES ARE NOT SUPPORTED under SYNC_BN: the cached total is keyed by this rank's count alone, so a rank
        # whose batch shrinks while this one's does not (a partial last batch of a non-drop_last loader) would leave it stale.
        # The first use of a key reads the all-reduced count back (one host synchronisation per layer shape, in the first step);
        # EVERY later use compares the all-reduced count with the cached one on the device and adds a mismatch to a flag that
        # sync_bn_poll() reads without a host synchronisation of its own (harness.Trainer.step: once per step) -- a step that
        # normalised with a stale N is reported one or two steps later, every time, not on one use in 512.
        key = (int(count), dist.get_world_size(group))
        total = _SYNC_BN_COUNTS.get(key)
        if total is None:
            total = _SYNC_BN_COUNTS[key] = int(round(tot[2 * C].item()))
        else:
            flag = _SYNC_BN_FLAG.get(ws.device)
            if flag is None:
                flag = _SYNC_BN_FLAG[ws.device] = torch.zeros(1, dtype=torch.int32, device=ws.device)
            flag.add_((tot[2 * C:2 * C + 1] != float(total)).to(torch.int32))
    return torch.stack([hi, lo]).contiguous(), total


ACT_NONE, ACT_RELU, ACT_RELU6 = 0, 1, 2      # the activation of a normalisation's apply pass (as conv.conv2d_folded numbers them)
GATED_BN_HITS = [0]        # BatchNorm backward passes that applied a residual tail's gate to their incoming gradient (tests)
GATED_BN = [os.environ.get("MRFP_GATED_BN", "1") != "0"]      # (A/B switch for this form alone)
RELU6_GATE_HITS = [0]      # ReLU6 backward passes that gated with mrfp_mask_gate (fp32 / channel counts off the 8-chunk; tests)


def _keeps_sign_mask(x, relu, res, plan):
    """Residual BatchNorm+ReLU on 16-bit activations: the apply pass writes the sign of its output as one bit per element."""
    return bool(relu and res is not None and plan is None and SIGN_MASK[0] and mask_possible(x))


class _BatchNormAct(torch.autograd.Function):
    """y = act(BN(resize(x)) + res), act one of ACT_NONE / ACT_RELU / ACT_RELU6.  reference: Norm2d/SyncBatchNorm on one process =
    F.batch_norm (mynn.py:19-25), Bottleneck tail (Resnet.py:202-225), HRFP stage (deepv3.py:320-327); with may_sync false the
    plain nn.BatchNorm2d of the reference's MobileNetV2 (network/Mobilenet.py: never Norm2d / SyncBatchNorm), whose statistics
    stay on this process -- it does not even ask for the statistics' communicator, which is created collectively.
    ReLU6 (nn.ReLU6 = hardtanh(0, 6)): the apply pass writes a 1-bit pass mask of the fp32 PRE-activation, 0 < x*A + S < 6 -- the
    gate torch applies -- and backward gates dy with it (a rounded 16-bit output cannot tell 5.99 from 6).
    stats: rows that receive the plane sums of the output (batch_norm_act(emit_stats=True)), or None."""

    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, res, training, momentum, eps, act, plan, may_sync, stats):
        relu, relu6 = act == ACT_RELU, act == ACT_RELU6
        if relu6 and (res is not None or plan is not None):
            raise _lib.MrfpHipError("BatchNorm + ReLU6 takes no residual and no resize plan")
        x = _chk(x)
        res = _chk(res, "res") if res is not None else None
        B, Ho, Wo, C, Hs, Ws, *_ = _geom(x, plan)
        dev = x.device
        w32, b32 = _f32(weight), _f32(bias)
        coef = torch.empty(4 * C, dtype=torch.float32, device=dev)
        mean, invstd, A, S = coef[0:C], coef[C:2 * C], coef[2 * C:3 * C], coef[3 * C:4 * C]
        if training:
            fused = _serving_colstats(x, C, B * Ho * Wo, plan, False)
            if fused is not None:
                # the producing convolution already summed its output per channel in its epilogue
                ws, nb_, nslab = fused.final, 1, fused.final_count
            else:
                nslab, ws = _stats_fwd(x, plan)
                nb_ = B
            count = B * Ho * Wo
            ctx.sync = _sync_bn_group() if may_sync else None
            if ctx.sync is not None:        # statistics over the batches of ALL ranks (one host synchronisation: the count)
                ws, count = _allreduce_stats(ws, nb_ * nslab, C, count, ctx.sync)
                nb_, nslab = 1, 2
            ctx.count = count
            call("mrfp_bn_finalize", ptr(ws), nb_, nslab, count, C, ptr(w32), ptr(b32), float(eps),
                 float(momentum), ptr(running_mean), ptr(running_var), ptr(mean), ptr(invstd), ptr(A), ptr(S), stream())
        else:
            ctx.sync, ctx.count = None, B * Ho * Wo
            call("mrfp_bn_eval_coef", C, ptr(w32), ptr(b32), ptr(running_mean), ptr(running_var), float(eps),
                 ptr(A), ptr(S), stream())
            if x.requires_grad or (weight is not None and weight.requires_grad):
                mean.copy_(running_mean)                          # what the backward's x-hat is built from
                torch.rsqrt(running_var.float() + eps, out=invstd)
        ctx.plan, ctx.act, ctx.training, ctx.has_res = plan, act, training, res is not None
        # ReLU mask for backward: without a residual it is recomputed from x and the apply coefficients
        # ((x*A+S) > 0, bit-identical to the forward expression), so y is not read again; with a residual the
        # stored output is the only place the sign lives -- and the two backward passes need nothing else of y, so
        # the apply pass also writes its sign as ONE BIT per element (16-bit activations): they then read 1/16 of y's
        # bytes (3.7 GB of y per step of the bench workload, read twice).  (ReLU6 never recomputes: its gate is on the fp32
        # pre-activation, and its pass mask is written for every dtype and channel count.)
        ctx.keep_y = relu and res is not None
        ctx.remask = relu and res is None
        ctx.ymask = _keeps_sign_mask(x, relu, res, plan)
        # res is the skip alias of a convolution (conv.conv2d(..., want_skip=True)): its gradient is consumed by that
        # convolution's dgrad epilogue only, which can apply the gate itself -- backward then hands it the incoming
        # gradient as it is, with the mask attached, instead of writing dy * [y > 0] -- provided this tail stays the alias's ONLY
        # consumer (skipgrad: the cell's use count is read in backward, when the whole forward has run)
        ctx.res_alias = getattr(res, ALIAS, None) if ctx.ymask and GATED_SKIP[0] else None
        # this layer itself can take a gated gradient: plain BatchNorm (no activation, no residual, no resize), 16-bit, whole mask bytes
        ctx.gate_ok = bool(act == ACT_NONE and res is None and plan is None and training and mask_possible(x))
        keep = None
        if relu6:
            y = empty_cl(B, C, Ho, Wo, x.dtype, dev)
            keep = torch.empty((B * Ho * Wo * C + 7) // 8, dtype=torch.uint8, device=dev)
            call("mrfp_affine_fwd_relu6_mask", ptr(x), ptr(y), ptr(keep), dt(x), B * Ho * Wo, C, ptr(A), ptr(S), stream())
        elif ctx.ymask:
            y = empty_cl(B, C, Ho, Wo, x.dtype, dev)
            keep = torch.empty(B * Ho * Wo * C // 8, dtype=torch.uint8, device=dev)
            call("mrfp_affine_fwd_relu_mask", ptr(x), ptr(res), ptr(y), ptr(keep), dt(x), B, Ho, Wo, C, ptr(A), ptr(S), 0, stream())
        else:
            y = _affine_fwd(x, res, A, S, False, relu, plan, stats=stats)
            if ctx.keep_y:
                keep = y
        ctx.wparam, ctx.bparam = weight, bias
        ctx.save_for_backward(x, keep, w32, mean, invstd, A, S)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, keep, w32, mean, invstd, A, S = ctx.saved_tensors      # keep: the sign / pass mask, or y itself (residual tail without one)
        # A residual tail may hand this layer its incoming gradient UNMASKED with its sign mask attached (this layer is the
        # BatchNorm of a downsample branch: reference Resnet.py:209-212 `residual = self.downsample(x)`; batch_norm_act() marked
        # its output as able to take that): the two passes below then gate dy while they read it, and dy * [out > 0] of the tail
        # is never written.  As in conv._Conv2d.backward: if the gate was promised and something else arrives, fail loudly.
        gate = None
        cell = getattr(ctx, ALIAS, None)
        if cell is not None:
            cell.redeem(dy, bn=True)
        g = GATE.fetch(dy)
        if g is not None:
            if ctx.gate_ok and gateable(dy, x):
                gate = g.mask
            else:
                dy = ungate(dy)
        dy = _chk(dy, "dy")
        plan = ctx.plan
        B, Ho, Wo, C, *_ = _geom(x, plan)
        fA, fS = (A, S) if ctx.remask else (None, None)
        # the 1-bit mask the masked kernel pair gates dy with while it reads it: the tail's sign mask behind a gated gradient, this
        # layer's own sign mask, or its ReLU6 pass mask (16-bit, whole mask bytes; otherwise dy is gated in a pass of its own first)
        mask = y = None
        if gate is not None:
            mask = gate
            GATED_BN_HITS[0] += 1
        elif ctx.ymask:
            mask = keep
        elif ctx.act == ACT_RELU6:
            if mask_possible(x) and dy.dtype == x.dtype:
                mask = keep
            else:
                gated = torch.empty_like(dy, memory_format=CL)
                call("mrfp_mask_gate", ptr(dy), ptr(keep), ptr(gated), dt(dy), dy.numel(), stream())
                dy = gated
                RELU6_GATE_HITS[0] += 1
        else:
            y = keep
        if mask is not None:
            nslab, ws = _stats_ws(B, Ho, C, x.device)
            call("mrfp_stats_bwd_mask", ptr(dy), ptr(x), ptr(mask), ptr(mean), 0, dt(x), B, Ho, Wo, C, ptr(ws), stream())
        else:
            nslab, ws = _stats_bwd(dy, x, y, mean, False, plan, fA, fS)
        out = torch.empty(5 * C, dtype=torch.float32, device=dy.device)
        dw, db, P, Q, R = (out[i * C:(i + 1) * C] for i in range(5))
        dw = _grad_dest(ctx.wparam, ctx.needs_input_grad[1], dw)
        db = _grad_dest(ctx.bparam, ctx.needs_input_grad[2], db)
        call("mrfp_bn_bwd_finalize", ptr(ws), B, nslab, B * Ho * Wo, C, ptr(w32), ptr(mean), ptr(invstd),
             ptr(dw), ptr(db), ptr(P), ptr(Q), ptr(R), stream())
        if ctx.sync is not None:
            # cross-rank statistics: dweight / dbias above are this rank's LOCAL sums (the data-parallel exchange averages
            # them, as with torch.nn.SyncBatchNorm); the input-gradient coefficients use the sums over ALL ranks
            gws, _ = _allreduce_stats(ws, B * nslab, C, 0, ctx.sync)
            call("mrfp_bn_bwd_finalize", ptr(gws), 1, 2, ctx.count, C, ptr(w32), ptr(mean), ptr(invstd), None, None,
                 ptr(P), ptr(Q), ptr(R), stream())
        if not ctx.training:
            # module in eval mode (running statistics are constants): the same dweight / dbias sums, but the input
            # gradient is just dy' * weight * invstd -- the batch-statistics terms Q, R vanish
            Q.zero_()
            R.zero_()
        if mask is not None:
            dx = empty_cl(B, C, Ho, Wo, dy.dtype, dy.device)
            dres = dres_out = None
            if ctx.ymask:
                if ctx.res_alias is not None and ctx.needs_input_grad[5] and ctx.res_alias.sole_consumer():
                    dres = dy.view_as(dy)                  # unmasked; the consumer applies the mask (conv._Conv2d.backward / ungate)
                    GATE.attach(dres, mask)
                    # told to the node that owns the alias: if what reaches it is not this tagged tensor (a consumer of the
                    # alias that bypassed _chk made autograd sum it into a fresh one), it raises instead of using it as if it were masked
                    ctx.res_alias.promise_gate()
                else:
                    dres = dres_out = empty_cl(B, C, Ho, Wo, dy.dtype, dy.device)
            call("mrfp_affine_bwd_mask", ptr(dy), ptr(x), ptr(mask), ptr(dx), ptr(dres_out), dt(dy), B, Ho, Wo, C, ptr(P), ptr(Q),
                 ptr(R), 0, stream())
        else:
            dx, dres = _affine_bwd(dy, x, y, P, Q, R, False, plan, ctx.has_res, x, fA, fS)
        return (dx, _grad_result(ctx.wparam, dw), _grad_result(ctx.bparam, db), None, None, dres) + (None,) * 7


# bumped by every training-mode BatchNorm forward: its kernel updates the running statistics in place through raw pointers, which no
# autograd version counter sees -- the folded inference packs built from those statistics (conv.get_folded_pack) key on this
RUNNING_STATS_EPOCH = [0]


def batch_norm_act(x, weight, bias, running_mean, running_var, *, training, momentum=0.1, eps=1e-5,
                   relu=False, res=None, plan=None, emit_stats=False):
    """emit_stats: the caller normalises the result per image next (an InstanceNorm `iw` tap behind this residual tail, reference
    Resnet.py:218-225): the apply pass also writes the partial plane sums of its output and that statistics pass is skipped."""
    if training and running_mean is not None:
        RUNNING_STATS_EPOCH[0] += 1
    ps = _planestats_rows(x, emit_stats and plan is None and not _keeps_sign_mask(x, relu, res, plan))
    y = _BatchNormAct.apply(x, weight, bias, running_mean, running_var, res, training, momentum, eps,
                            ACT_RELU if relu else ACT_NONE, plan, True, ps[1] if ps is not None else None)
    _tag_planestats(y, ps)
    if (GATED_BN[0] and GATED_SKIP[0] and SIGN_MASK[0] and not relu and res is None and plan is None and training and y.grad_fn is not None
            and mask_possible(y)):
        # the plain BatchNorm of a downsample branch: a residual tail that consumes this output (and nothing else does: the use
        # count) may send its gradient gated -- see _BatchNormAct.backward.  Same protocol as a convolution's skip alias.
        AliasCell(y, y.grad_fn)
    return y


def local_batch_norm_act(x, weight, bias, running_mean, running_var, *, training, momentum=0.1, eps=1e-5, act=None):
    """BatchNorm over this process's batch (never synchronised across ranks) followed by `act`: None or 'relu6'."""
    if act not in (None, "relu6"):
        raise _lib.MrfpHipError("local_batch_norm_act: act must be None or 'relu6' (got %r)" % (act,))
    if training and running_mean is not None:
        RUNNING_STATS_EPOCH[0] += 1
    return _BatchNormAct.apply(x, weight, bias, running_mean, running_var, None, bool(training), momentum, eps,
                               ACT_RELU6 if act == "relu6" else ACT_NONE, None, False, None)


def batch_norm_relu6(x, weight, bias, running_mean, running_var, *, training, momentum=0.1, eps=1e-5):
    """clamp(BN(x), 0, 6): nn.BatchNorm2d -> nn.ReLU6 (reference network/Mobilenet.py ConvBNReLU)."""
    return local_batch_norm_act(x, weight, bias, running_mean, running_var, training=training, momentum=momentum, eps=eps,
                                act="relu6")


# ------------------------------------------------------------------------------------------
# InstanceNorm (+ReLU)
# ------------------------------------------------------------------------------------------
IN_FUSED_STATS = [os.environ.get("MRFP_IN_FUSED_STATS", "1") != "0"]     # InstanceNorm statistics from the producing convolution's epilogue
IN_FUSED_HITS = [0]


def _in_plane_sums(x):
    """-> (x checked, nslab, ws): the [B][nslab][2][C] partial (sum, sum of squares) rows of x's planes for mrfp_in_finalize, from
    whoever already has them -- the producing convolution's epilogue, the producing apply pass -- or a statistics pass."""
    ps = _take_planestats(x)
    x = _chk(x)
    B, C, H, W = x.shape
    fused = _serving_colstats(x, C, B * H * W, None, True)
    rb = fused.block_rows if fused is not None else 0
    if rb < 0 and B * (-rb) == fused.row_blocks:
        # the weight-stationary 3x3 kernel (csrc/conv_c64.hip) writes its statistics rows per IMAGE: -rb rows each
        IN_FUSED_HITS[0] += 1
        return x, -rb, fused.rows
    if rb > 0 and (H * W) % rb == 0 and B * ((H * W) // rb) <= fused.row_blocks:
        # the producing convolution summed its output per row block in its epilogue, and no row block straddles an image
        # (H*W is a multiple of the block height): its rows ARE the [B][blocks per image][2][C] partials of the plane sums --
        # the statistics pass over the convolution output disappears
        IN_FUSED_HITS[0] += 1
        return x, (H * W) // rb, fused.rows
    if ps is not None:
        return x, ps[0], ps[1]
    nslab, ws = _stats_fwd(x, None)
    return x, nslab, ws


def _in_finalize(x, nslab, ws, weight, bias, eps):
    """-> (w32, mean, invstd, A, S): per-(image, channel) statistics and apply coefficients from the plane sums (_in_plane_sums)."""
    B, C, H, W = x.shape
    w32, b32 = _f32(weight), _f32(bias)
    n = B * C
    coef = torch.empty(4 * n, dtype=torch.float32, device=x.device)
    mean, invstd, A, S = coef[0:n], coef[n:2 * n], coef[2 * n:3 * n], coef[3 * n:4 * n]
    call("mrfp_in_finalize", ptr(ws), B, nslab, H * W, C, ptr(w32), ptr(b32), float(eps), ptr(mean),
         ptr(invstd), ptr(A), ptr(S), stream())
    return w32, mean, invstd, A, S


def _in_bwd_finalize(ctx, x, nslab, ws, w32, mean, invstd):
    """-> (P, Q, R, dw, db): the input-gradient coefficients from the backward plane sums; dweight / dbias are written where
    _grad_dest says (the caller returns _grad_result of them after its apply launch)."""
    B, C, H, W = x.shape
    n = B * C
    pqr = torch.empty(3 * n, dtype=torch.float32, device=x.device)
    P, Q, R = pqr[0:n], pqr[n:2 * n], pqr[2 * n:3 * n]
    dwb = torch.empty(2 * C, dtype=torch.float32, device=x.device)
    dw = _grad_dest(ctx.wparam, ctx.wparam is not None, dwb[:C])
    db = _grad_dest(ctx.bparam, ctx.bparam is not None, dwb[C:])
    call("mrfp_in_bwd_finalize", ptr(ws), B, nslab, H * W, C, ptr(w32), ptr(mean), ptr(invstd), ptr(dw), ptr(db),
         ptr(P), ptr(Q), ptr(R), stream())
    return P, Q, R, dw, db


class _InstanceNormAct(torch.autograd.Function):
    """nn.InstanceNorm2d(affine) (+ReLU): reference Resnet.py:176-178, 218-225, 534-536.
    stats: rows that receive the plane sums of the output (instance_norm_act(emit_stats=True)), or None."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps, relu, stats):
        x, nslab, ws = _in_plane_sums(x)
        w32, mean, invstd, A, S = _in_finalize(x, nslab, ws, weight, bias, eps)
        y = _affine_fwd(x, None, A, S, True, relu, None, stats=stats)
        ctx.relu = relu
        ctx.wparam, ctx.bparam = weight, bias
        ctx.save_for_backward(x, w32, mean, invstd, A, S)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w32, mean, invstd, A, S = ctx.saved_tensors
        dy = _chk(dy, "dy")
        fA, fS = (A, S) if ctx.relu else (None, None)      # ReLU mask recomputed from x (see _BatchNormAct)
        nslab, ws = _stats_bwd(dy, x, None, mean, True, None, fA, fS)
        P, Q, R, dw, db = _in_bwd_finalize(ctx, x, nslab, ws, w32, mean, invstd)
        dx, _ = _affine_bwd(dy, x, None, P, Q, R, True, None, False, x, fA, fS)
        return dx, _grad_result(ctx.wparam, dw), _grad_result(ctx.bparam, db), None, None, None


def instance_norm_act(x, weight, bias, *, eps=1e-5, relu=False, emit_stats=False):
    """emit_stats: NP+ follows (reference deepv3.py:333-335): the apply pass also writes the partial plane sums of its output."""
    ps = _planestats_rows(x, emit_stats)
    return _tag_planestats(_InstanceNormAct.apply(x, weight, bias, eps, relu, ps[1] if ps is not None else None), ps)


# ------------------------------------------------------------------------------------------
# NP+
# ------------------------------------------------------------------------------------------
class _NPPlus(torch.autograd.Function):
    """Normalization_Perturbation_Plus, reference deepv3.py:268-277; alpha / beta_noise are the two
    normal draws ([B,C,1,1])."""

    @staticmethod
    def forward(ctx, x, alpha, beta_noise, res=None):
        ps = _take_planestats(x)
        x = _chk(x)
        res = _chk(res, "res") if res is not None else None
        B, C, H, W = x.shape
        a32 = alpha.detach().float().reshape(B, C).contiguous()
        n32 = beta_noise.detach().float().reshape(B, C).contiguous()
        buf = torch.empty(3 * B * C + C, dtype=torch.float32, device=x.device)
        n = B * C
        mu, A, S, sigma = buf[0:n], buf[n:2 * n], buf[2 * n:3 * n], buf[3 * n:3 * n + C]
        nslab, ws = ps if ps is not None else _stats_fwd(x, None)      # (ps: the producing apply pass summed its output already)
        call("mrfp_np_finalize", ptr(ws), B, nslab, H * W, C, ptr(a32), ptr(n32), ptr(mu), ptr(sigma), ptr(A),
             ptr(S), stream())
        y = _affine_fwd(x, res, A, S, True, False, None)      # (+ res: the HRFP output added in the same pass, deepv3.py:333-334)
        ctx.save_for_backward(a32, n32, mu, sigma)
        ctx.shape = (B, C, H, W)
        ctx.has_res = res is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        a32, n32, mu, sigma = ctx.saved_tensors
        dy = _chk(dy, "dy")
        B, C, H, W = ctx.shape
        nslab, ws = _stats_bwd(dy, dy, None, None, True, None)       # G[b,c] = sum_hw dy
        tmp = torch.empty(2 * B * C, dtype=torch.float32, device=dy.device)
        G, K = tmp[:B * C], tmp[B * C:]
        call("mrfp_np_bwd_finalize", ptr(ws), B, nslab, H * W, C, ptr(a32), ptr(n32), ptr(mu), ptr(sigma),
             ptr(G), ptr(K), stream())
        dx = empty_cl(B, C, H, W, dy.dtype, dy.device)               # dx = alpha*dy + K
        call("mrfp_affine_fwd", ptr(dy), None, ptr(dx), dt(dy), B, H, W, C, H, W, None, None, ptr(a32), ptr(K), 1, 0,
             stream())
        return dx, None, None, (dy if ctx.has_res else None)


def np_plus(x, alpha, beta_noise, res=None):
    """res: a tensor added to the perturbed features in the same pass (y = NP+(x) + res)."""
    return _NPPlus.apply(x, alpha, beta_noise, res)


# ------------------------------------------------------------------------------------------
# bilinear align_corners resize (+ add)
# ------------------------------------------------------------------------------------------
class _Bilinear(torch.autograd.Function):
    """Upsample(): reference mynn.py:114-119; with addend: torch.add(OCout_dec, Upsample(dec1)) of
    deepv3.py:356-357 fused into one pass."""

    @staticmethod
    def forward(ctx, x, addend, Ho, Wo, channels):
        x = _chk(x)
        addend = _chk(addend, "addend") if addend is not None else None
        B, ld, Hi, Wi = x.shape
        C = ld if channels is None else int(channels)
        y = empty_cl(B, C, Ho, Wo, x.dtype, x.device)
        call("mrfp_bilinear_fwd", ptr(x), ptr(addend), ptr(y), dt(x), B, Hi, Wi, Ho, Wo, C, ld, stream())
        ctx.dims = (B, C, ld, Hi, Wi, Ho, Wo)
        ctx.has_add = addend is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        dy = _chk(dy, "dy")
        B, C, ld, Hi, Wi, Ho, Wo = ctx.dims
        if ld == C:
            dx = empty_cl(B, ld, Hi, Wi, dy.dtype, dy.device)
        else:       # pad channels of the low-resolution gradient stay zero
            dx = zeros_cl(B, ld, Hi, Wi, dy.dtype, dy.device)
        call("mrfp_bilinear_bwd", ptr(dy), ptr(dx), dt(dy), B, Hi, Wi, Ho, Wo, C, ld, stream())
        return dx, (dy if ctx.has_add else None), None, None, None


class _Broadcast(torch.autograd.Function):
    """Upsample() of a 1x1 map (the ASPP image-pooling branch, reference deepv3.py:117-121): every output pixel is
    the source value, so forward is a broadcast store and backward a plane sum (the statistics kernel) instead of
    one thread gathering a whole plane."""

    @staticmethod
    def forward(ctx, x, Ho, Wo):
        x = _chk(x)
        B, C = x.shape[0], x.shape[1]
        S = x.detach().float().reshape(B, C).contiguous()
        y = empty_cl(B, C, Ho, Wo, x.dtype, x.device)
        call("mrfp_affine_fwd", None, None, ptr(y), dt(x), B, Ho, Wo, C, Ho, Wo, None, None, None, ptr(S), 1, 0, stream())
        ctx.dims = (B, C, Ho, Wo)
        return y

    @staticmethod
    def backward(ctx, dy):
        dy = _chk(dy, "dy")
        B, C, Ho, Wo = ctx.dims
        nslab, ws = _stats_fwd(dy, None)
        dx = empty_cl(B, C, 1, 1, dy.dtype, dy.device)
        tmp = torch.empty(B * C, dtype=torch.float32, device=dy.device)
        call("mrfp_mean_finalize", ptr(ws), B, nslab, 1, C, ptr(tmp), ptr(dx), dt(dy), stream())     # count 1: the sum
        return dx, None, None


def upsample_bilinear(x, size, addend=None, channels=None):
    """channels: use only the first `channels` channels of x (x is a channel-padded buffer)."""
    if x.shape[2] == 1 and x.shape[3] == 1 and addend is None and channels is None:
        return _Broadcast.apply(x, int(size[0]), int(size[1]))
    return _Bilinear.apply(x, addend, int(size[0]), int(size[1]), channels)


# ------------------------------------------------------------------------------------------
# max pool 3x3 / stride 2 / pad 1
# ------------------------------------------------------------------------------------------
class _MaxPool(torch.autograd.Function):
    """nn.MaxPool2d(3, 2, 1): reference Resnet.py:551, deepv3.py:315."""

    @staticmethod
    def forward(ctx, x):
        x = _chk(x)
        B, C, H, W = x.shape
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        y = empty_cl(B, C, Ho, Wo, x.dtype, x.device)
        idx = torch.empty(B * Ho * Wo * C, dtype=torch.uint8, device=x.device)
        call("mrfp_maxpool_fwd", ptr(x), ptr(y), ptr(idx), dt(x), B, H, W, C, stream())
        ctx.save_for_backward(idx)
        ctx.dims = (B, C, H, W)
        return y

    @staticmethod
    def backward(ctx, dy):
        (idx,) = ctx.saved_tensors
        dy = _chk(dy, "dy")
        B, C, H, W = ctx.dims
        dx = empty_cl(B, C, H, W, dy.dtype, dy.device)
        call("mrfp_maxpool_bwd", ptr(dy), ptr(idx), ptr(dx), dt(dy), B, H, W, C, stream())
        return dx


def max_pool_3x3_s2(x):
    return _MaxPool.apply(x)


POOL_FUSED = [os.environ.get("MRFP_POOL_FUSED", "1") != "0"]
POOL_FUSED_HITS = [0]


class _InstanceNormReluPool(torch.autograd.Function):
    """InstanceNorm2d -> ReLU -> MaxPool2d(3, 2, 1) as ONE operator: the stem of the trunks whose wt_layer selects an
    instance norm there (reference Resnet.py:176-178, 549-551; deepv3.py:309-315).  The normalised tensor is never stored: the
    pool applies x*A + S and the ReLU to its window values (mrfp_maxpool_affine_fwd), and the two backward passes of the
    normalisation rebuild the gradient of the pool's input from the pooled gradient and the arg-max positions
    (mrfp_pool_norm_bwd_stats / _apply) -- per step one write and three reads of the largest activation of the network less.
    Results are those of instance_norm_act(relu=True) + max_pool_3x3_s2 (statistics: same kernels; maxima / positions: same values,
    rounded before the comparison; backward sums in a different order)."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps):
        x, nslab, ws = _in_plane_sums(x)
        B, C, H, W = x.shape
        w32, mean, invstd, A, S = _in_finalize(x, nslab, ws, weight, bias, eps)
        Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        y = empty_cl(B, C, Ho, Wo, x.dtype, x.device)
        idx = torch.empty(B * Ho * Wo * C, dtype=torch.uint8, device=x.device)
        call("mrfp_maxpool_affine_fwd", ptr(x), ptr(A), ptr(S), 1, 1, ptr(y), ptr(idx), dt(x), B, H, W, C, stream())
        ctx.wparam, ctx.bparam = weight, bias
        ctx.save_for_backward(x, idx, w32, mean, invstd, A, S)
        POOL_FUSED_HITS[0] += 1
        return y

    @staticmethod
    def backward(ctx, dy):
        x, idx, w32, mean, invstd, A, S = ctx.saved_tensors
        dy = _chk(dy, "dy")
        B, C, H, W = x.shape
        nslab, ws = _stats_ws(B, H, C, x.device)
        call("mrfp_pool_norm_bwd_stats", ptr(dy), ptr(idx), ptr(x), ptr(mean), ptr(A), ptr(S), 1, 1, ptr(ws), dt(x), B, H, W, C,
             stream())
        P, Q, R, dw, db = _in_bwd_finalize(ctx, x, nslab, ws, w32, mean, invstd)
        dx = empty_cl(B, C, H, W, dy.dtype, dy.device)
        call("mrfp_pool_norm_bwd_apply", ptr(dy), ptr(idx), ptr(x), ptr(P), ptr(Q), ptr(R), ptr(A), ptr(S), 1, 1, ptr(dx), dt(x),
             B, H, W, C, stream())
        return dx, _grad_result(ctx.wparam, dw), _grad_result(ctx.bparam, db), None


def instance_norm_relu_pool(x, weight, bias, *, eps=1e-5):
    """instance_norm_act(relu=True) followed by max_pool_3x3_s2, fused (MRFP_POOL_FUSED=0: the two operators)."""
    if not POOL_FUSED[0]:
        return max_pool_3x3_s2(instance_norm_act(x, weight, bias, eps=eps, relu=True))
    return _InstanceNormReluPool.apply(x, weight, bias, eps)


# ------------------------------------------------------------------------------------------
# global average pool
# ------------------------------------------------------------------------------------------
class _GlobalAvgPool(torch.autograd.Function):
    """nn.AdaptiveAvgPool2d(1): reference deepv3.py:109, 117."""

    @staticmethod
    def forward(ctx, x):
        x = _chk(x)
        B, C, H, W = x.shape
        nslab, ws = _stats_fwd(x, None)
        out = empty_cl(B, C, 1, 1, x.dtype, x.device)
        tmp = torch.empty(B * C, dtype=torch.float32, device=x.device)
        call("mrfp_mean_finalize", ptr(ws), B, nslab, H * W, C, ptr(tmp), ptr(out), dt(x), stream())
        ctx.dims = (B, C, H, W)
        return out

    @staticmethod
    def backward(ctx, g):
        B, C, H, W = ctx.dims
        S = (g.detach().float().reshape(B, C) / float(H * W)).contiguous()
        dx = empty_cl(B, C, H, W, g.dtype, g.device)
        call("mrfp_affine_fwd", None, None, ptr(dx), dt(g), B, H, W, C, H, W, None, None, None, ptr(S), 1, 0, stream())
        return dx


def global_avg_pool(x):
    return _GlobalAvgPool.apply(x)


# ------------------------------------------------------------------------------------------
# per-(image, channel) scale: Dropout2d
# ------------------------------------------------------------------------------------------
class _ChannelScale(torch.autograd.Function):
    """y[b,c,:,:] = x[b,c,:,:] * m[b,c] (nn.Dropout2d with its keep-mask / (1-p) given explicitly; reference
    network/wider_resnet.py:302, 333-338): one apply pass forward, one backward."""

    @staticmethod
    def forward(ctx, x, m):
        x = _chk(x)
        B, C = x.shape[0], x.shape[1]
        m = m.detach().to(device=x.device, dtype=torch.float32).reshape(B * C).contiguous()
        y = _affine_fwd(x, None, m, None, True, False, None)
        ctx.save_for_backward(m)
        return y

    @staticmethod
    def backward(ctx, dy):
        (m,) = ctx.saved_tensors
        dy = _chk(dy, "dy")
        dx, _ = _affine_bwd(dy, None, None, m, None, None, True, None, False, dy)
        return dx, None


def channel_scale(x, m):
    return _ChannelScale.apply(x, m)


# ------------------------------------------------------------------------------------------
# elementwise add
# ------------------------------------------------------------------------------------------
class _Add(torch.autograd.Function):
    """torch.add(OCout, x): reference deepv3.py:330."""

    @staticmethod
    def forward(ctx, a, b):
        a, b = _chk(a, "a"), _chk(b, "b")
        if a.shape != b.shape or a.dtype != b.dtype:
            raise _lib.MrfpHipError("add: shape/dtype mismatch %s %s" % (tuple(a.shape), tuple(b.shape)))
        y = torch.empty_like(a, memory_format=CL)
        call("mrfp_add", ptr(a), ptr(b), ptr(y), dt(a), a.numel(), stream())
        return y

    @staticmethod
    def backward(ctx, g):
        return g, g


def add(a, b):
    return _Add.apply(a, b)


# ------------------------------------------------------------------------------------------
# cross entropy (ignore_index) -- scalar fp32 loss
# ------------------------------------------------------------------------------------------
# The loss operators have the two axes of the kernels under them (csrc/loss_common.hpp): where a pixel's class vector comes from
# (_Scores: dense logits, or low-resolution scores the kernel upsamples) and which criterion reads it (_PlainCe, _WeightedCe,
# _SoftNll, _Focal).  One autograd function, _PixelLoss, serves every pair (the region and Lovasz losses have a sibling, _RegionLoss); the entry is mrfp_[upsample_]<stem>_{fwd,bwd}, and its arguments
# are looked up by the names include/mrfp_hip.h gives them, never placed by position.
def _call_named(entry, env):
    """Calls `entry` with its positional arguments taken from env, a dictionary of named values to which the stream is added here; a
    name the header asks for and env lacks is a KeyError, before anything is launched."""
    env["stream"] = stream()
    call(entry, *[env[n] for n in _lib.ARG_NAMES[entry]])


def _chk_target(who, t, dtype, dims, shape=None):
    """A label-like operand, contiguous: a GPU tensor of `dims` dimensions, or with `shape` a loss's target of exactly that shape."""
    if shape is not None:
        t = t.contiguous()
        if t.dtype != dtype or tuple(t.shape) != shape:
            raise _lib.MrfpHipError("%s: target must be int64 [B,H,W]" % who)
        return t
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _lib.MrfpHipError("%s: the target must be a GPU tensor: the HIP path has no CPU fallback" % who)
    if t.dtype != dtype or t.dim() != dims:
        raise _lib.MrfpHipError("%s: expected a %d-dimensional %s tensor (got %s %s)" % (who, dims, dtype, t.dtype, tuple(t.shape)))
    return t.contiguous()


class _Scores:
    """Where the class vector of a pixel comes from: dense logits [B,C,H,W] (size None), or channel-padded low-resolution scores
    P [B,ld,Hi,Wi] (ld a multiple of the 16-byte chunk) that the kernel upsamples to `size`, the first `channels` of them classes.
    x: the tensor as _chk returned it."""

    def __init__(self, x, size=None, channels=None):
        self.x, self.fused, self.B = x, size is not None, x.shape[0]
        if self.fused:
            self.ld, self.Hi, self.Wi = x.shape[1:]
            self.H, self.W, self.C = int(size[0]), int(size[1]), int(channels)
        else:
            self.C, self.H, self.W = x.shape[1:]
        self.prefix = "mrfp_upsample_" if self.fused else "mrfp_"

    def env(self):
        """Head and geometry arguments under the header's names: logits and P are the one pointer; an entry takes the geometry it
        names (npix, or B and HW, or B, Hi, Wi, H, W)."""
        x = self.x
        env = dict(logits=ptr(x), P=ptr(x), dtype=dt(x), B=self.B, H=self.H, W=self.W, HW=self.H * self.W, C=self.C,
                   npix=self.B * self.H * self.W)
        if self.fused:
            env.update(ld=self.ld, Hi=self.Hi, Wi=self.Wi)
        return env

    def grad(self, entry, env, tag=""):
        """d(loss)/d(scores) by the backward `entry`.  Dense: the entry writes it.  Fused: the entry writes d(loss)/d(logits) at full
        resolution once, channel-padded to Cd, and the gather-form bilinear backward takes it to dP.
        tag: a two-view entry (mrfp_[upsample_]consist_bwd) names this view's rows dlogits<tag>; it is launched once for both views,
        by the caller: with entry None this only places the row buffer in env and returns finish() -> the gradient, to be called
        after that launch."""
        x = self.x
        if not self.fused:
            d = torch.empty_like(x, memory_format=CL)
            env["dlogits" + tag] = ptr(d)
            if entry is None:
                return lambda: d
            _call_named(entry, env)
            return d
        B, ld, Hi, Wi, H, W = self.B, self.ld, self.Hi, self.Wi, self.H, self.W
        epc = 16 // x.element_size()
        Cd = (self.C + epc - 1) // epc * epc
        dP = empty_cl(B, ld, Hi, Wi, x.dtype, x.device)
        dlog = empty_cl(B, Cd, H, W, x.dtype, x.device)
        env.update({"dlogits" + tag: ptr(dlog), "Cd": Cd})

        def down():
            if ld != Cd:
                dP.zero_()
            call("mrfp_bilinear_bwd", ptr(dlog), ptr(dP), dt(x), B, Hi, Wi, H, W, Cd, ld, stream())
            return dP
        if entry is None:
            return down
        _call_named(entry, env)
        return down()

    def view_env(self, tag):
        """This view's own arguments of a two-view entry under the header's names: logits<tag> / P<tag> and, fused, ld / Hi / Wi<tag>."""
        env = {"logits" + tag: ptr(self.x), "P" + tag: ptr(self.x)}
        if self.fused:
            env.update({"ld" + tag: self.ld, "Hi" + tag: self.Hi, "Wi" + tag: self.Wi})
        return env


class _PlainCe:
    """nn.CrossEntropyLoss(ignore_index=255): reference main.py:822, deepv3.py:363 (mrfp_[upsample_]ce_*).  A criterion record: its
    entry stem, check() -> the validated (target, weight), extra() -> its own C arguments, sizes() -> (workgroups, loss floats)."""
    stem = "ce"

    def __init__(self, who, ignore_index):
        self.who, self.ignore_index = who, ignore_index

    def check(self, src, target, weight):
        return _chk_target(self.who, target, torch.int64, 3, (src.B, src.H, src.W)), None

    def extra(self, weight):
        return dict(ignore_index=int(self.ignore_index))

    def sizes(self, L, src):
        return L.mrfp_ce_nblocks(src.B * src.H * src.W), 2


def _ce_options(who, weight, label_smoothing, reduction, per_image, B, C, device):
    """-> (weight fp32 [C] / [B,C] or None, wstride, eps, mode), validated without touching the device."""
    if reduction not in ("mean", "sum"):
        raise _lib.MrfpHipError("%s: reduction must be 'mean' or 'sum' (got %r; 'none' stays the caller's business)" % (who, reduction))
    if per_image and reduction != "mean":
        raise _lib.MrfpHipError("%s: per_image sums the per-image weighted means: reduction must be 'mean'" % who)
    eps = float(label_smoothing)
    if not 0.0 <= eps < 1.0:
        raise _lib.MrfpHipError("%s: label_smoothing must be in [0, 1) (got %r)" % (who, label_smoothing))
    wstride = 0
    if weight is not None:
        if not isinstance(weight, torch.Tensor) or weight.dtype != torch.float32 or weight.device != device \
                or tuple(weight.shape) not in ((C,), (B, C)):
            raise _lib.MrfpHipError("%s: weight must be a float32 tensor of shape [C] or [B, C] on %s (C=%d, B=%d; got %s)" % (
                who, device, C, B, (weight.dtype, tuple(weight.shape), weight.device) if isinstance(weight, torch.Tensor) else type(weight)))
        weight = weight.detach().contiguous()
        wstride = C if weight.dim() == 2 else 0
    mode = 2 if per_image else (0 if reduction == "mean" else 1)      # mrfp_ce_mode: MRFP_CE_IMAGE_MEAN, MRFP_CE_MEAN, MRFP_CE_SUM
    return weight, wstride, eps, mode


class _WeightedCe(_PlainCe):
    """nn.CrossEntropyLoss(weight, ignore_index, label_smoothing, reduction 'mean' / 'sum') and the per-image weighted mean: the
    criteria a caller hands to the reference's DeepV3Plus (network/deepv3.py:111 `criterion`, `criterion_aux`) instead of the plain
    one of main.py:822 -- csrc/loss.hip, mrfp_[upsample_]ce_w_*."""
    stem = "ce_w"

    def __init__(self, who, ignore_index, *options):
        self.who, self.ignore_index, self.options = who, ignore_index, options

    def check(self, src, target, weight):
        target, _ = _PlainCe.check(self, src, target, weight)
        weight, self.wstride, self.eps, self.mode = _ce_options(self.who, weight, *self.options, src.B, src.C, src.x.device)
        return target, weight

    def extra(self, weight):
        return dict(ignore_index=int(self.ignore_index), weight=ptr(weight), wstride=self.wstride, smoothing=self.eps, mode=self.mode)

    def sizes(self, L, src):
        return L.mrfp_ce_w_nblocks(src.B, src.H * src.W), L.mrfp_ce_w_loss_floats(src.B, self.mode)


def _loss_env(src, crit, target, weight, loss):
    """The named values a loss entry of (src, crit) can ask for, its own buffers and the stream apart: target and words are the one
    pointer."""
    env = src.env()
    env.update(crit.extra(weight))
    env["target"] = env["words"] = ptr(target)
    env["loss"] = ptr(loss)
    return env


class _PixelLoss(torch.autograd.Function):
    """loss = crit(the class scores of (x, size, channels) at full resolution, target): every loss operator of this section.  The
    fused source never materialises the full-resolution logits (reference deepv3.py:361-365 in training mode)."""

    @staticmethod
    def forward(ctx, x, target, weight, size, channels, crit):
        src = _Scores(_chk(x, "logits" if size is None else "P"), size, channels)
        target, weight = crit.check(src, target, weight)
        nblk, nloss = crit.sizes(_lib.lib(), src)
        ws = torch.empty(2 * int(nblk), dtype=torch.float32, device=src.x.device)
        loss = torch.empty(int(nloss), dtype=torch.float32, device=src.x.device)
        env = _loss_env(src, crit, target, weight, loss)
        env["ws"] = ptr(ws)
        _call_named(src.prefix + crit.stem + "_fwd", env)
        ctx.save_for_backward(src.x, target, loss, weight)
        ctx.size, ctx.channels, ctx.crit = size, channels, crit
        return loss[0].clone()

    @staticmethod
    def backward(ctx, g):
        x, target, loss, weight = ctx.saved_tensors
        src, crit = _Scores(x, ctx.size, ctx.channels), ctx.crit
        gs = g.detach().float().reshape(1).contiguous()
        env = _loss_env(src, crit, target, weight, loss)
        env["gscale"] = ptr(gs)
        return src.grad(src.prefix + crit.stem + "_bwd", env), None, None, None, None, None


def _cross_entropy(who, x, target, size, channels, ignore_index, weight, label_smoothing, reduction, per_image, _general):
    """With the four keywords at their defaults the plain kernels run untouched; `_general` forces the weighted entries."""
    if _general or weight is not None or float(label_smoothing) != 0.0 or reduction != "mean" or bool(per_image):
        crit = _WeightedCe(who, ignore_index, label_smoothing, reduction, per_image)
    else:
        crit = _PlainCe(who, ignore_index)
    return _PixelLoss.apply(x, target, weight, size, channels, crit)


def cross_entropy(logits, target, ignore_index=255, *, weight=None, label_smoothing=0.0, reduction="mean", per_image=False,
                  _general=False):
    """weight: float32 [C] (shared) or [B, C] (one row per image) on the device; reduction 'mean' (sum of weighted losses over the
    sum of the target weights, as torch) or 'sum'; per_image: the sum over images of each image's weighted mean."""
    return _cross_entropy("cross_entropy", logits, target, None, None, ignore_index, weight, label_smoothing, reduction, per_image,
                          _general)


def upsample_cross_entropy(P, target, size, channels, ignore_index=255, *, weight=None, label_smoothing=0.0, reduction="mean",
                           per_image=False, _general=False):
    """P: channel-padded low-resolution class scores [B,ld,Hi,Wi] (ld a multiple of the 16-byte chunk).  Keywords as cross_entropy."""
    return _cross_entropy("upsample_cross_entropy", P, target, (int(size[0]), int(size[1])), int(channels), ignore_index, weight,
                          label_smoothing, reduction, per_image, _general)


def label_class_weights(target, num_classes, upper_bound=1.0, norm=False, batch=False):
    """Per-image class weights from the label map, on the device (csrc/loss.hip, mrfp_label_class_weights):
    with n_c the count of label c in [0, num_classes) and f_c = n_c / sum n_c, w_c = 1 + upper_bound * (1 - f_c) (norm: 1 +
    upper_bound / f_c) where n_c > 0, else 1.  -> float32 [B, C], or [1, C] from the pooled counts of all images (batch)."""
    if not isinstance(target, torch.Tensor) or not target.is_cuda:
        raise _lib.MrfpHipError("label_class_weights: target must be a GPU tensor: the HIP path has no CPU fallback")
    if target.dtype != torch.int64 or target.dim() != 3:
        raise _lib.MrfpHipError("label_class_weights: target must be int64 [B,H,W] (got %s %s)" % (target.dtype, tuple(target.shape)))
    target = target.contiguous()
    B, H, W = target.shape
    C, rows = int(num_classes), (1 if batch else B)
    counts = torch.empty(rows * C, dtype=torch.int64, device=target.device)
    out = torch.empty(rows, C, dtype=torch.float32, device=target.device)
    call("mrfp_label_class_weights", ptr(target), B, H * W, C, float(upper_bound), int(bool(norm)), int(bool(batch)), ptr(counts),
         ptr(out), stream())
    return out


# ---- boundary label relaxation and the joint-weighted soft-NLL loss (csrc/relax.hip; include/mrfp_hip.h and DESIGN.md section 8
# hold the definitions): the relaxed target of a pixel is one int32 word, bit c = class c occurs in its window, bit C = ignore ----
RELAX_MAX_CLASSES, RELAX_MAX_BORDER = 31, 8


def strict_class_mask(strict_classes, num_classes):
    """STRICTBORDERCLASS (None or a list of class ids, reference config.py:64) as the bit mask the kernel takes."""
    mask = 0
    for c in strict_classes or ():
        c = int(c)
        if not 0 <= c < num_classes:
            raise _lib.MrfpHipError("strict_classes: %d is not a class of 0..%d" % (c, num_classes - 1))
        mask |= 1 << c
    return mask


def _relax_args(who, num_classes, border=0):
    C, r = int(num_classes), int(border)
    if not 1 <= C <= RELAX_MAX_CLASSES:
        raise _lib.MrfpHipError("%s: 1 <= num_classes <= %d: the classes and the ignore bit share one 32-bit word (got %d)" % (
            who, RELAX_MAX_CLASSES, C))
    if not 0 <= r <= RELAX_MAX_BORDER:
        raise _lib.MrfpHipError("%s: 0 <= border <= %d (got %d)" % (who, RELAX_MAX_BORDER, r))
    return C, r


def relax_labels(target, num_classes, border=1, strict_classes=None, want_counts=False):
    """int64 [B,H,W] label map -> int32 [B,H,W] relaxed words (reference transforms/transforms.py:91-118), and with want_counts the
    int64 [B, C+1] number of pixels per image that carry each bit."""
    C, r = _relax_args("relax_labels", num_classes, border)
    mask = strict_class_mask(strict_classes, C)
    target = _chk_target("relax_labels", target, torch.int64, 3)
    B, H, W = target.shape
    words = torch.empty(B, H, W, dtype=torch.int32, device=target.device)
    counts = torch.empty(B, C + 1, dtype=torch.int64, device=target.device) if want_counts else None
    call("mrfp_relax_labels", ptr(target), B, H, W, C, r, mask, ptr(words), ptr(counts), stream())
    return (words, counts) if want_counts else words


def pack_multihot(onehot_u8, want_counts=False):
    """uint8 [B, C+1, H, W] multi-hot (what the reference's transform emits; any non-zero byte is set) -> int32 [B,H,W] words."""
    m = _chk_target("pack_multihot", onehot_u8, torch.uint8, 4)
    B, C1, H, W = m.shape
    C, _ = _relax_args("pack_multihot", C1 - 1)
    words = torch.empty(B, H, W, dtype=torch.int32, device=m.device)
    counts = torch.empty(B, C + 1, dtype=torch.int64, device=m.device) if want_counts else None
    call("mrfp_multihot_pack", ptr(m), B, H * W, C, ptr(words), ptr(counts), stream())
    return (words, counts) if want_counts else words


def relaxed_counts(words, num_classes):
    """int32 [B,H,W] words -> int64 [B, C+1] pixels per image with each bit set."""
    C, _ = _relax_args("relaxed_counts", num_classes)
    words = _chk_target("relaxed_counts", words, torch.int32, 3)
    B, H, W = words.shape
    counts = torch.empty(B, C + 1, dtype=torch.int64, device=words.device)
    call("mrfp_relax_word_counts", ptr(words), B, H * W, C, ptr(counts), stream())
    return counts


def relaxed_class_weights(counts, upper_bound=1.0, norm=False, batch=False):
    """int64 [B, C+1] counts -> float32 [B, C] class weights, or [C] from the pooled counts of all images (batch): with
    f_c = n_c / sum_{c=0..C} n_c, w_c = 1 + upper_bound * (1 - f_c) (norm: 1 + upper_bound / f_c) where n_c > 0, else 1."""
    counts = _chk_target("relaxed_class_weights", counts, torch.int64, 2)
    B, C1 = counts.shape
    C, _ = _relax_args("relaxed_class_weights", C1 - 1)
    out = torch.empty((C,) if batch else (B, C), dtype=torch.float32, device=counts.device)
    call("mrfp_relax_class_weights", ptr(counts), B, C, float(upper_bound), int(bool(norm)), int(bool(batch)), ptr(out), stream())
    return out


def _soft_nll_options(who, relaxed, weight, B, H, W, C, device):
    if not isinstance(relaxed, torch.Tensor) or relaxed.dtype != torch.int32 or tuple(relaxed.shape) != (B, H, W) \
            or relaxed.device != device:
        raise _lib.MrfpHipError("%s: the relaxed target must be int32 [B,H,W] words on %s (ops.relax_labels / ops.pack_multihot)" % (
            who, device))
    _relax_args(who, C)
    weight, wstride, _, _ = _ce_options(who, weight, 0.0, "mean", False, B, C, device)
    return relaxed.contiguous(), weight, wstride


class _SoftNll:
    """The joint-weighted soft-NLL loss of relaxed targets (mrfp_[upsample_]soft_nll_*): a criterion record, as _PlainCe."""
    stem = "soft_nll"

    def __init__(self, who, num_classes):
        self.who, self.C = who, num_classes

    def check(self, src, relaxed, weight):
        if src.C != self.C:
            raise _lib.MrfpHipError("%s: logits have %d channels, num_classes is %d" % (self.who, src.C, self.C))
        relaxed, weight, self.wstride = _soft_nll_options(self.who, relaxed, weight, src.B, src.H, src.W, src.C, src.x.device)
        return relaxed, weight

    def extra(self, weight):
        return dict(weight=ptr(weight), wstride=self.wstride)

    def sizes(self, L, src):
        return L.mrfp_soft_nll_nblocks(src.B, src.H * src.W), L.mrfp_soft_nll_loss_floats(src.B)


def soft_nll(logits, relaxed, num_classes, weight=None):
    """logits [B,C,H,W]; relaxed: int32 [B,H,W] words; weight: float32 [C] (shared) or [B, C] (one row per image) on the device, None =
    ones.  -> the sum over the images of sum_valid (W_i / k_i) (lse_all - lse_set) / (valid_b + 1), fp32 scalar."""
    return _PixelLoss.apply(logits, relaxed, weight, None, None, _SoftNll("soft_nll", int(num_classes)))


def upsample_soft_nll(P, relaxed, size, channels, weight=None):
    """P: channel-padded low-resolution class scores [B,ld,Hi,Wi] (ld a multiple of the 16-byte chunk); the rest as soft_nll."""
    return _PixelLoss.apply(P, relaxed, weight, (int(size[0]), int(size[1])), int(channels), _SoftNll("upsample_soft_nll", int(channels)))


# ---- online hard example mining for the cross entropy (csrc/ohem.hip; include/mrfp_hip.h and DESIGN.md section 8 hold the
# definition): the kept set is chosen on the device -- probability plane, exact radix select, masked target -- with no host wait,
# and the loss and its gradient are the cross-entropy operators above on the masked target ----
OHEM_SENTINEL = 2.0                       # the probability plane's value at an invalid pixel
OHEM_KEEP_ALL, OHEM_THRESH, OHEM_KTH = 0, 1, 2          # the state's mode word


def _ohem_ws(B, HW, device):
    n = int(_lib.lib().mrfp_ohem_ws_bytes(B, HW))
    if n < 0:
        raise _lib.MrfpHipError("ohem: unsupported size (B=%d, H*W=%d): 1 <= B <= 65535, H*W < 2^30, B*H*W < 2^31" % (B, HW))
    return torch.empty(n // 4, dtype=torch.int32, device=device)


def select_kth(x_f32, k):
    """The k-th smallest (from 1) element of a float32 tensor, exactly, as a 0-d float32 tensor on the device (mrfp_select_kth: a
    three-level radix select on the bit patterns, no sort and no host wait).  x holds non-negative values; NaN sorts last, as in
    torch.sort; elements equal to OHEM_SENTINEL are skipped and k counts the others."""
    if not isinstance(x_f32, torch.Tensor) or not x_f32.is_cuda or x_f32.dtype != torch.float32:
        raise _lib.MrfpHipError("select_kth: x must be a float32 GPU tensor: the HIP path has no CPU fallback")
    x = x_f32.detach().contiguous()
    n, k = x.numel(), int(k)
    if n < 1 or not 1 <= k <= n:
        raise _lib.MrfpHipError("select_kth: 1 <= k <= numel (k=%d, numel=%d)" % (k, n))
    ws = _ohem_ws(1, 1, x.device)
    out = torch.empty((), dtype=torch.float32, device=x.device)
    call("mrfp_select_kth", ptr(x), n, k, ptr(ws), ptr(out), stream())
    return out


def _ohem_args(who, thresh, min_kept):
    thresh, min_kept = float(thresh), int(min_kept)
    if not 0.0 <= thresh <= 1.0:              # also false for a NaN
        raise _lib.MrfpHipError("%s: thresh must be in [0, 1] (got %r)" % (who, thresh))
    if min_kept < 0:
        raise _lib.MrfpHipError("%s: min_kept must not be negative (got %d)" % (who, min_kept))
    return thresh, min_kept


def ohem_target(logits, target, ignore_index=255, thresh=0.7, min_kept=100000, *, size=None, channels=None, want_prob=False,
                want_state=False):
    """The masked int64 target [B,H,W] of the OHEM rule (include/mrfp_hip.h): `target` where the pixel is kept, ignore_index
    elsewhere.  logits: [B,C,H,W]; with `size` the channel-padded low-resolution class scores [B,ld,Hi,Wi] and `channels` classes,
    as for upsample_cross_entropy.  want_prob: also the float32 plane [B,H,W] of p = softmax(z)[t] (OHEM_SENTINEL where the pixel is
    invalid); want_state: also int32 [4] on the device, (valid pixels, kept pixels, bits of theta, mode).  No autograd through it:
    the selection is a constant."""
    who = "ohem_target"
    thresh, min_kept = _ohem_args(who, thresh, min_kept)
    src = _Scores(_chk(logits.detach(), "logits"), size, channels)
    B, H, W, dev = src.B, src.H, src.W, src.x.device
    target = _chk_target(who, target, torch.int64, 3, (B, H, W))
    ws = _ohem_ws(B, H * W, dev)
    prob = torch.empty(B, H, W, dtype=torch.float32, device=dev)
    masked = torch.empty(B, H, W, dtype=torch.int64, device=dev)
    env = src.env()
    env.update(target=ptr(target), ignore_index=int(ignore_index), thresh=thresh, min_kept=min_kept, prob=ptr(prob), masked=ptr(masked),
               ws=ptr(ws))
    _call_named(src.prefix + "ohem_target", env)
    if not (want_prob or want_state):
        return masked
    return (masked,) + ((prob,) if want_prob else ()) + ((ws[:4],) if want_state else ())


def ohem_cross_entropy(logits, target, ignore_index=255, *, thresh=0.7, min_kept=100000, weight=None):
    """nn.CrossEntropyLoss(weight, ignore_index) of the pixels the OHEM rule keeps: cross_entropy on ohem_target's masked target."""
    masked = ohem_target(logits, target, ignore_index, thresh, min_kept)
    return cross_entropy(logits, masked, ignore_index, weight=weight)


def upsample_ohem_cross_entropy(P, target, size, channels, ignore_index=255, *, thresh=0.7, min_kept=100000, weight=None):
    """ohem_cross_entropy of Upsample(P[:, :channels], size) without materialising the full-resolution logits: upsample_cross_entropy
    on the masked target ohem_target computes from the same low-resolution scores."""
    masked = ohem_target(P, target, ignore_index, thresh, min_kept, size=size, channels=channels)
    return upsample_cross_entropy(P, masked, size, channels, ignore_index, weight=weight)


# ---- focal loss and the soft Dice / Jaccard region loss (csrc/loss.hip: Focal; csrc/region.hip; include/mrfp_hip.h and DESIGN.md
# section 8 hold the definitions).  Focal is one more criterion record of _PixelLoss.  The region loss needs per-class sums over its
# scope before any pixel has a gradient, so its workspace and saved tensors differ: a sibling function, _RegionLoss, again one
# for both sources ----
LOSS_MAX_CLASSES = 64                     # kMaxClasses: the class vector of a pixel lives in registers
REGION_KINDS = {"dice": 0, "jaccard": 1}  # mrfp_region_kind


def _class_limit(who, C):
    if not 1 <= int(C) <= LOSS_MAX_CLASSES:
        raise _lib.MrfpHipError("%s: 1 <= C <= %d: the class vector of a pixel lives in registers (C=%d)" % (who, LOSS_MAX_CLASSES, C))


def _focal_options(who, gamma):
    """-> gamma as a float, validated without touching the device."""
    try:
        g = float(gamma)
    except (TypeError, ValueError):
        g = float("nan")
    if not 0.0 <= g < float("inf"):           # also false for a NaN
        raise _lib.MrfpHipError("%s: gamma must be a finite number >= 0 (got %r)" % (who, gamma))
    return g


class _Focal(_WeightedCe):
    """-w[t] (1 - p_t)^gamma log p_t with the reductions of the weighted cross entropy (mrfp_[upsample_]focal_*): a criterion record,
    as _PlainCe.  gamma == 0 is the weighted cross entropy."""
    stem = "focal"

    def __init__(self, who, ignore_index, gamma, reduction, per_image):
        _WeightedCe.__init__(self, who, ignore_index, 0.0, reduction, per_image)
        self.gamma = _focal_options(who, gamma)

    def check(self, src, target, weight):
        _class_limit(self.who, src.C)
        return _WeightedCe.check(self, src, target, weight)

    def extra(self, weight):
        return dict(ignore_index=int(self.ignore_index), weight=ptr(weight), wstride=self.wstride, gamma=self.gamma, mode=self.mode)


def focal_loss(logits, target, ignore_index=255, *, gamma=2.0, weight=None, reduction="mean", per_image=False):
    """logits [B,C,H,W], C <= 64; target int64 [B,H,W].  sum_i -w[t_i] (1 - p_{i,t_i})^gamma log p_{i,t_i} over the valid pixels, reduced
    as cross_entropy reduces ('mean': over the sum of the target weights; 'sum'; per_image: the sum of the per-image means).  weight:
    float32 [C] or [B, C] on the device.  -> fp32 scalar."""
    return _PixelLoss.apply(logits, target, weight, None, None, _Focal("focal_loss", ignore_index, gamma, reduction, per_image))


def upsample_focal_loss(P, target, size, channels, ignore_index=255, *, gamma=2.0, weight=None, reduction="mean", per_image=False):
    """focal_loss of Upsample(P[:, :channels], size) without materialising the full-resolution logits.  P: channel-padded
    low-resolution class scores [B,ld,Hi,Wi] (ld a multiple of the 16-byte chunk)."""
    return _PixelLoss.apply(P, target, weight, (int(size[0]), int(size[1])), int(channels),
                            _Focal("upsample_focal_loss", ignore_index, gamma, reduction, per_image))


def _region_options(who, kind, smooth, present_only, weight, C, device):
    """-> (kind id, smooth, present_only, weight fp32 [C] or None), validated without touching the device."""
    if kind not in REGION_KINDS:
        raise _lib.MrfpHipError("%s: kind must be 'dice' or 'jaccard' (got %r)" % (who, kind))
    try:
        s = float(smooth)
    except (TypeError, ValueError):
        s = float("nan")
    if not 0.0 <= s < float("inf"):
        raise _lib.MrfpHipError("%s: smooth must be a finite number >= 0 (got %r)" % (who, smooth))
    present_only = bool(present_only)
    if not present_only and s <= 0.0:
        raise _lib.MrfpHipError("%s: present_only=False needs smooth > 0: an absent class has an empty denominator (got %r)" % (who, smooth))
    if C is not None:
        _class_limit(who, C)
    if weight is not None and C is not None:
        if not isinstance(weight, torch.Tensor) or weight.dtype != torch.float32 or weight.device != device or tuple(weight.shape) != (C,):
            raise _lib.MrfpHipError("%s: weight must be a float32 tensor of shape [C] on %s (C=%d; got %s)" % (
                who, device, C, (weight.dtype, tuple(weight.shape), weight.device) if isinstance(weight, torch.Tensor) else type(weight)))
        weight = weight.detach().contiguous()
    return REGION_KINDS[kind], s, present_only, weight


class _Region:
    """The soft Dice / Jaccard loss over per-class sums (mrfp_[upsample_]region_*): a criterion record, as _PlainCe, of _RegionLoss."""
    stem = "region"

    def __init__(self, who, ignore_index, kind="dice", smooth=1.0, present_only=True, per_image=False):
        self.who, self.ignore_index, self.per_image = who, ignore_index, bool(per_image)
        self.options = (kind, smooth, present_only)
        _region_options(who, kind, smooth, present_only, None, None, None)         # what does not depend on the tensors: at once

    def check(self, src, target, weight):
        self.kind, self.smooth, self.present_only, weight = _region_options(self.who, *self.options, weight, src.C, src.x.device)
        return _chk_target(self.who, target, torch.int64, 3, (src.B, src.H, src.W)), weight

    def extra(self, weight):
        return dict(ignore_index=int(self.ignore_index), weight=ptr(weight), kind=self.kind, smooth=self.smooth,
                    present_only=int(self.present_only), per_image=int(self.per_image))

    def rows(self, src):
        return src.B if self.per_image else 1

    def sizes(self, L, src):
        """(workspace floats, out floats)"""
        return L.mrfp_region_ws_floats(src.B, src.H * src.W, src.C), L.mrfp_region_out_floats(src.B, src.C, int(self.per_image))


def _region_forward(src, crit, target, weight):
    """The forward entry of a criterion over a scope (_Region: sums pass and finalize; _Lovasz: keys, sort, scan, coefficients per class
    group and finalize) -> (validated target, out): out[0] the loss, out[1] the factor of the backward, then what the backward of the
    criterion reads (include/mrfp_hip.h)."""
    target, weight = crit.check(src, target, weight)
    L, dev = _lib.lib(), src.x.device
    nws, nout = crit.sizes(L, src)
    ws = torch.empty(int(nws), dtype=torch.float32, device=dev)
    out = torch.empty(int(nout), dtype=torch.float32, device=dev)
    env = _loss_env(src, crit, target, weight, out)
    env.update(ws=ptr(ws), out=ptr(out))
    _call_named(src.prefix + crit.stem + "_fwd", env)
    return target, out


class _RegionLoss(torch.autograd.Function):
    """loss = the region criterion of the class scores of (x, size, channels) at full resolution: two launches forward (sums,
    finalize; neither waits for the host), one backward plus the bilinear backward of the fused source."""

    @staticmethod
    def forward(ctx, x, target, weight, size, channels, crit):
        src = _Scores(_chk(x, "logits" if size is None else "P"), size, channels)
        target, out = _region_forward(src, crit, target, weight)
        ctx.save_for_backward(src.x, target, out)
        ctx.size, ctx.channels, ctx.crit = size, channels, crit
        return out[0].clone()

    @staticmethod
    def backward(ctx, g):
        x, target, out = ctx.saved_tensors
        src, crit = _Scores(x, ctx.size, ctx.channels), ctx.crit
        gs = g.detach().float().reshape(1).contiguous()
        env = _loss_env(src, crit, target, None, out)
        env.update(out=ptr(out), gscale=ptr(gs))
        return src.grad(src.prefix + crit.stem + "_bwd", env), None, None, None, None, None


def region_loss(logits, target, ignore_index=255, *, kind="dice", smooth=1.0, present_only=True, weight=None, per_image=False):
    """The soft Dice (kind 'dice') or Jaccard ('jaccard') loss of softmax(logits) against the one-hot target over the valid pixels:
    with I_c = sum p_c [t = c], P_c = sum p_c, T_c = #{t = c}, S_c = (2 I_c + s) / (P_c + T_c + s) (dice) or (I_c + s) / (P_c + T_c - I_c +
    s) (jaccard), the weighted mean of 1 - S_c over the classes present in the scope (present_only) or over all (needs smooth > 0).
    The scope is the whole batch OF THIS RANK -- under data parallelism the sums are per rank, like the OHEM selection -- or with
    per_image each image, averaged over the images that have a class.  Nothing valid: 0, and a zero gradient.  logits [B,C,H,W], C <= 64;
    weight: float32 [C] on the device.  -> fp32 scalar."""
    return _RegionLoss.apply(logits, target, weight, None, None, _Region("region_loss", ignore_index, kind, smooth, present_only, per_image))


def upsample_region_loss(P, target, size, channels, ignore_index=255, *, kind="dice", smooth=1.0, present_only=True, weight=None,
                         per_image=False):
    """region_loss of Upsample(P[:, :channels], size) without materialising the full-resolution logits (per-rank sums, as
    region_loss).  P: channel-padded low-resolution class scores [B,ld,Hi,Wi] (ld a multiple of the 16-byte chunk)."""
    return _RegionLoss.apply(P, target, weight, (int(size[0]), int(size[1])), int(channels),
                             _Region("upsample_region_loss", ignore_index, kind, smooth, present_only, per_image))


def region_sums(logits, target, ignore_index=255, *, size=None, channels=None, per_image=False):
    """The sums the region loss is made of, float64 [rows, 3, C] on the device (rows = B with per_image, else 1; I_c, P_c, T_c), of
    this rank's batch.  With `size`, logits are the channel-padded low-resolution scores.  No autograd through it."""
    crit = _Region("region_sums", ignore_index, per_image=per_image)
    fused = size is not None
    src = _Scores(_chk(logits.detach(), "P" if fused else "logits"), (int(size[0]), int(size[1])) if fused else None,
                  int(channels) if fused else None)
    _, out = _region_forward(src, crit, target, None)
    rows, CP = crit.rows(src), (src.C + 7) // 8 * 8
    return out[2 + rows * 2 * CP:].view(torch.float64).view(rows, 3, src.C).clone()


# ---- the Lovasz-Softmax loss and the stable segmented radix sort under it (csrc/lovasz.hip, csrc/sort.hip; include/mrfp_hip.h and
# DESIGN.md section 8 hold the definition).  The gradient of a pixel depends on the rank of its error among the pixels of the scope:
# the loss is an operator of its own, not a kind of region_loss; its criterion record runs on _RegionLoss, whose forward asks the
# record for the workspace and the saved `out` (here: loss, factor table, coefficient plane) ----
LOVASZ_CLASSES = {"present": 0, "all": 1}   # all_classes
LOVASZ_SENTINEL = 2.0                       # lovasz_errors at an invalid pixel
LOVASZ_MAX_PIXELS = 2 ** 31                 # B * H * W below this: the payload holds 2 * flat index + the foreground bit


def _lovasz_options(who, classes):
    if not isinstance(classes, str) or classes not in LOVASZ_CLASSES:
        raise _lib.MrfpHipError("%s: classes must be 'present' or 'all' (got %r; an explicit class list is not built)" % (who, classes))
    return LOVASZ_CLASSES[classes]


def _lovasz_limits(who, src):
    _class_limit(who, src.C)
    if not 0 < src.B * src.H * src.W < LOVASZ_MAX_PIXELS or src.B > 65535:
        raise _lib.MrfpHipError("%s: 1 <= B <= 65535 and B * H * W < 2^31: a pixel's rank and index are 31-bit (B=%d, H=%d, W=%d)" % (
            who, src.B, src.H, src.W))


class _Lovasz:
    """The Lovasz-Softmax loss (mrfp_[upsample_]lovasz_*): a criterion record, as _Region, of _RegionLoss."""
    stem = "lovasz"

    def __init__(self, who, ignore_index, classes="present", per_image=False):
        self.who, self.ignore_index, self.per_image = who, ignore_index, bool(per_image)
        self.all_classes = _lovasz_options(who, classes)           # what does not depend on the tensors: at once

    def check(self, src, target, weight):
        _lovasz_limits(self.who, src)
        return _chk_target(self.who, target, torch.int64, 3, (src.B, src.H, src.W)), None

    def extra(self, weight):
        return dict(ignore_index=int(self.ignore_index), all_classes=self.all_classes, per_image=int(self.per_image))

    def sizes(self, L, src):
        B, HW, C, per = src.B, src.H * src.W, src.C, int(self.per_image)
        return (int(L.mrfp_lovasz_ws_bytes(B, HW, C, per)) + 3) // 4, L.mrfp_lovasz_out_floats(B, HW, C, per)


def lovasz_softmax(logits, target, ignore_index=255, *, classes="present", per_image=False):
    """The Lovasz-Softmax loss (Berman et al., CVPR 2018) of softmax(logits) against the target over the valid pixels.  Per scope and class
    c: e_i = |[t_i == c] - p_i[c]|; the scope's pixels ordered by e descending, ties by ascending flat pixel index (a stable sort: the
    tie rule is part of the definition); loss_c = sum_i e_i g_i with g the Lovasz gradient of the Jaccard loss along that order, a
    constant for the backward.  classes 'present': the mean over the classes that occur in the scope; 'all': over all C.  The scope
    is the whole batch OF THIS RANK -- under data parallelism the order is per rank, like the OHEM selection -- or with per_image each
    image, averaged over the images that have a counted class.  Nothing valid: 0, and a zero gradient.  logits [B,C,H,W], C <= 64,
    B * H * W < 2^31.  -> fp32 scalar."""
    return _RegionLoss.apply(logits, target, None, None, None, _Lovasz("lovasz_softmax", ignore_index, classes, per_image))


def upsample_lovasz_softmax(P, target, size, channels, ignore_index=255, *, classes="present", per_image=False):
    """lovasz_softmax of Upsample(P[:, :channels], size) without materialising the full-resolution logits (what is kept per pixel and
    class is the fp32 coefficient plane the backward reads).  P: channel-padded low-resolution class scores [B,ld,Hi,Wi] (ld a multiple
    of the 16-byte chunk)."""
    return _RegionLoss.apply(P, target, None, (int(size[0]), int(size[1])), int(channels),
                             _Lovasz("upsample_lovasz_softmax", ignore_index, classes, per_image))


def lovasz_errors(logits, target, ignore_index=255, *, size=None, channels=None):
    """The error planes e = |[t == c] - softmax(z)[c]| exactly as the loss's keys pass computes them: float32 [C,B,H,W] on the device,
    LOVASZ_SENTINEL at an invalid pixel.  With `size`, logits are the channel-padded low-resolution scores.  A stable sort of a plane by
    (-e, flat index) is the device's own order.  No autograd through it."""
    who = "lovasz_errors"
    fused = size is not None
    src = _Scores(_chk(logits.detach(), "P" if fused else "logits"), (int(size[0]), int(size[1])) if fused else None,
                  int(channels) if fused else None)
    _lovasz_limits(who, src)
    target = _chk_target(who, target, torch.int64, 3, (src.B, src.H, src.W))
    # (filled, not torch.empty: tests/test_poison_gpu.py holds the table of functions that obtain uninitialised memory, and this
    # one is a diagnostic off the training path)
    err = torch.full((src.C, src.B, src.H, src.W), LOVASZ_SENTINEL, dtype=torch.float32, device=src.x.device)
    call("mrfp_lovasz_errors", ptr(src.x), src.ld if fused else 0, ptr(target), dt(src.x), src.B, src.Hi if fused else 0,
         src.Wi if fused else 0, src.H, src.W, src.C, int(ignore_index), ptr(err), stream())
    return err


# ---- two-view consistency losses (csrc/consist.hip; include/mrfp_hip.h and DESIGN.md section 8 hold the definitions).  The "target" of a
# pixel is the class vector of a second forward pass, so this is no criterion record of _PixelLoss: one autograd function over TWO
# _Scores, both dense or both fused, launched once forward and once backward for both views ----
CONSIST_KINDS = {"kl": 0, "js": 1, "hard": 2}        # mrfp_consist_kind
CONSIST_NORMALIZE = {"kept": 0, "valid": 1}          # mrfp_consist_normalize
CONSIST_MAX_CLASSES = 64                             # mrfp_consist_max_classes(): the student's class vector lives in registers


def _consist_options(who, kind, temperature, threshold, normalize):
    """-> (kind id, T, threshold, normalize id), validated without touching the device or the library."""
    if not isinstance(kind, str) or kind not in CONSIST_KINDS:
        raise _lib.MrfpHipError("%s: kind must be 'kl', 'js' or 'hard' (got %r)" % (who, kind))
    try:
        T, thr = float(temperature), float(threshold)
    except (TypeError, ValueError):
        T = thr = float("nan")
    if not 0.0 < T < float("inf"):              # also false for a NaN
        raise _lib.MrfpHipError("%s: temperature must be a finite number > 0 (got %r)" % (who, temperature))
    if not 0.0 <= thr <= 1.0:
        raise _lib.MrfpHipError("%s: threshold must be in [0, 1] (got %r)" % (who, threshold))
    if not isinstance(normalize, str) or normalize not in CONSIST_NORMALIZE:
        raise _lib.MrfpHipError("%s: normalize must be 'kept' or 'valid' (got %r)" % (who, normalize))
    return CONSIST_KINDS[kind], T, thr, CONSIST_NORMALIZE[normalize]


def _consist_views(who, student, teacher, valid, size, channels):
    """The two views and the validity map against each other, before the library is touched: types, dtypes, shapes, the class limit,
    and last the devices.  -> (C, H, W)."""
    for name, t in (("student", student), ("teacher", teacher)):
        if not isinstance(t, torch.Tensor) or t.dim() != 4:
            raise _lib.MrfpHipError("%s: %s must be a 4-D tensor, dense logits [B,C,H,W] or fused scores [B,ld,Hi,Wi] (got %s)" % (
                who, name, tuple(t.shape) if isinstance(t, torch.Tensor) else type(t)))
    if student.dtype != teacher.dtype or student.dtype not in _lib._DT:
        raise _lib.MrfpHipError("%s: both views have one dtype, float32 / bfloat16 / float16 (got %s and %s)" % (
            who, student.dtype, teacher.dtype))
    if size is None:
        if tuple(student.shape) != tuple(teacher.shape):
            raise _lib.MrfpHipError("%s: dense views have one shape [B,C,H,W] (got %s and %s)" % (
                who, tuple(student.shape), tuple(teacher.shape)))
        C, H, W = student.shape[1:]
    else:
        H, W, C = int(size[0]), int(size[1]), int(channels)
        epc = 16 // student.element_size()
        if student.shape[0] != teacher.shape[0] or H < 1 or W < 1:
            raise _lib.MrfpHipError("%s: the views have one batch size and one output size (got %s and %s -> %s)" % (
                who, tuple(student.shape), tuple(teacher.shape), (H, W)))
        for name, t in (("student", student), ("teacher", teacher)):
            if t.shape[1] % epc or t.shape[1] < C or C < 1:
                raise _lib.MrfpHipError("%s: the %s's scores must be channel-padded to 16-byte chunks and hold %d classes (ld=%d)" % (
                    who, name, C, t.shape[1]))
    if not 1 <= int(C) <= CONSIST_MAX_CLASSES:
        raise _lib.MrfpHipError("%s: 1 <= C <= %d: the student's class vector lives in registers (C=%d)" % (who, CONSIST_MAX_CLASSES, C))
    if valid is not None and (not isinstance(valid, torch.Tensor) or valid.dtype != torch.int64
                              or tuple(valid.shape) != (student.shape[0], H, W)):
        raise _lib.MrfpHipError("%s: valid must be None or an int64 [B,H,W] label map (got %s)" % (
            who, (valid.dtype, tuple(valid.shape)) if isinstance(valid, torch.Tensor) else type(valid)))
    for name, t in (("student", student), ("teacher", teacher), ("valid", valid)):
        if t is not None and (not t.is_cuda or t.device != student.device):
            raise _lib.MrfpHipError("%s: %s must live on the student's GPU (got %s): the HIP path has no CPU fallback" % (who, name, t.device))
    return int(C), int(H), int(W)


def _consist_env(ss, st, valid, out, opts):
    kind, T, thr, norm = opts
    env = ss.env()
    env.update(ss.view_env("_s"))
    env.update(st.view_env("_t"))
    env.update(valid=ptr(valid), loss=ptr(out), kind=kind, temperature=T, threshold=thr, normalize=norm)
    return env


class _Consistency(torch.autograd.Function):
    """(loss, counts) = the consistency criterion of two views at full resolution: two launches forward (pixel loop, finalize;
    neither waits for the host), one backward for both views plus the bilinear backward of each fused view that takes a gradient.
    counts: int64 [2] on the device, (N_counted, N_kept)."""

    @staticmethod
    def forward(ctx, xs, xt, valid, size, channels, opts):
        ss = _Scores(_chk(xs, "student"), size, channels)
        st = _Scores(_chk(xt, "teacher"), size, channels)
        valid = None if valid is None else valid.contiguous()
        L, dev = _lib.lib(), ss.x.device
        nloss = int(L.mrfp_consist_loss_floats())
        nws = int(L.mrfp_consist_ws_floats(ss.B, ss.H * ss.W))
        # (one zero-filled buffer, not torch.empty: tests/test_poison_gpu.py holds the table of the functions that obtain uninitialised
        #  memory; 8 + 4 * workgroups floats.  The loss words come first: 8-byte aligned)
        buf = torch.zeros(8 + nws, dtype=torch.float32, device=dev)
        out, ws = buf[:nloss], buf[8:]
        env = _consist_env(ss, st, valid, out, opts)
        env["ws"] = ptr(ws)
        _call_named(ss.prefix + "consist_fwd", env)
        ctx.save_for_backward(ss.x, st.x, valid, buf)
        ctx.size, ctx.channels, ctx.opts = size, channels, opts
        counts = out[2:6].view(torch.int64).clone()
        ctx.mark_non_differentiable(counts)
        return out[0].clone(), counts

    @staticmethod
    def backward(ctx, g, _gcounts):
        xs, xt, valid, buf = ctx.saved_tensors
        ss, st = _Scores(xs, ctx.size, ctx.channels), _Scores(xt, ctx.size, ctx.channels)
        gs = g.detach().float().reshape(1).contiguous()
        env = _consist_env(ss, st, valid, buf, ctx.opts)
        env.update(gscale=ptr(gs), dlogits_s=None, dlogits_t=None, Cd=0)
        js = ctx.opts[0] == CONSIST_KINDS["js"]
        fin_s = ss.grad(None, env, "_s") if ctx.needs_input_grad[0] else None
        fin_t = st.grad(None, env, "_t") if js and ctx.needs_input_grad[1] else None
        _call_named(ss.prefix + "consist_bwd", env)
        return (None if fin_s is None else fin_s()), (None if fin_t is None else fin_t()), None, None, None, None


def _consistency(who, student, teacher, valid, size, channels, kind, temperature, threshold, normalize, want_counts):
    opts = _consist_options(who, kind, temperature, threshold, normalize)
    _consist_views(who, student, teacher, valid, size, channels)
    if kind != "js":
        teacher = teacher.detach()           # the teacher is a constant of kl and hard
    loss, counts = _Consistency.apply(student, teacher, valid, size, channels, opts)
    return (loss, counts) if want_counts else loss


def consistency_loss(student, teacher, valid=None, *, kind="kl", temperature=1.0, threshold=0.0, normalize="kept", want_counts=False):
    """The consistency of two views' class scores, dense logits [B,C,H,W] of one shape and dtype, C <= 64.  With p = softmax(student / T),
    q = softmax(teacher / T), m = (p + q) / 2, over the counted pixels (valid: an int64 [B,H,W] label map, counted iff 0 <= valid < C --
    the ground truth as it is -- or None: every pixel):
      kind 'kl':   T^2 KL(q || p), the mean over the counted pixels; the teacher is a constant.
      kind 'js':   T^2 (KL(p || m) + KL(q || m)) / 2, the same mean; the gradient goes to every view that requires one.
      kind 'hard': the cross entropy of the student against the teacher's arg-max (the first maximum) over the pixels whose teacher
                   confidence softmax(teacher)_k (at T = 1: temperature does not enter this kind) reaches `threshold`; divided by the
                   kept pixels (normalize 'kept') or by the counted ones ('valid': weighted by the confident share).  The teacher is a
                   constant.
    An empty denominator gives 0 and a zero gradient.  -> fp32 scalar; with want_counts (loss, int64 [2] on the device: N_counted, N_kept)."""
    return _consistency("consistency_loss", student, teacher, valid, None, None, kind, temperature, threshold, normalize, want_counts)


def upsample_consistency_loss(Ps, Pt, size, channels, valid=None, *, kind="kl", temperature=1.0, threshold=0.0, normalize="kept",
                              want_counts=False):
    """consistency_loss of Upsample(Ps[:, :channels], size) and Upsample(Pt[:, :channels], size) without materialising either at full
    resolution.  Ps, Pt: channel-padded low-resolution class scores [B,ld,Hi,Wi] (ld a multiple of the 16-byte chunk), which may
    differ in ld, Hi and Wi -- a teacher with another output stride."""
    return _consistency("upsample_consistency_loss", Ps, Pt, valid, (int(size[0]), int(size[1])), int(channels), kind, temperature,
                        threshold, normalize, want_counts)


def _chk_u32(who, name, t, n=None):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _lib.MrfpHipError("%s: %s must be a GPU tensor: the HIP path has no CPU fallback" % (who, name))
    if t.dtype != torch.int32 or t.dim() != 1 or (n is not None and t.numel() != n):
        raise _lib.MrfpHipError("%s: %s must be a 1-dimensional int32 tensor%s (got %s %s)" % (
            who, name, "" if n is None else " of %d elements" % n, t.dtype, tuple(t.shape)))
    return t.detach().contiguous()


def sort_pairs(keys, payload, offsets=None, bits=32):
    """(keys, payload) sorted by key, ascending and STABLE (equal keys keep their order), on the device (mrfp_sort_pairs: a
    least-significant-digit radix sort, three launches per 8 key bits, no host wait).  keys, payload: int32 GPU tensors [n] whose bits
    are read as unsigned; bits: how many low key bits take part (the rest travels along).  offsets: int64 GPU tensor [S + 1],
    non-decreasing from 0 to n: the pairs are sorted inside each segment [offsets[s], offsets[s + 1]) independently.  -> new tensors."""
    who = "sort_pairs"
    bits = int(bits)
    if not 1 <= bits <= 32:
        raise _lib.MrfpHipError("%s: 1 <= bits <= 32 (got %d)" % (who, bits))
    keys = _chk_u32(who, "keys", keys)
    n = keys.numel()
    payload = _chk_u32(who, "payload", payload, n)
    if n >= 2 ** 31:
        raise _lib.MrfpHipError("%s: n < 2^31 (n=%d)" % (who, n))
    S = 1
    if offsets is not None:
        if not isinstance(offsets, torch.Tensor) or not offsets.is_cuda or offsets.dtype != torch.int64 or offsets.dim() != 1 \
                or offsets.numel() < 2:
            raise _lib.MrfpHipError("%s: offsets must be a 1-dimensional int64 GPU tensor of S + 1 >= 2 elements" % who)
        offsets = offsets.contiguous()
        S = offsets.numel() - 1
    # the outputs start as copies and the workspace filled (see lovasz_errors): with an odd number of passes the entry reads the copies
    # and writes them last; with an even number it sorts them in place
    ko, po = keys.clone(), payload.clone()
    if n == 0:
        return ko, po
    nws = int(_lib.lib().mrfp_sort_pairs_ws_bytes(n, S))
    if nws < 0:
        raise _lib.MrfpHipError("%s: unsupported size (n=%d, S=%d)" % (who, n, S))
    ws = torch.zeros((nws + 3) // 4, dtype=torch.int32, device=keys.device)
    even = ((bits + 7) // 8) % 2 == 0
    call("mrfp_sort_pairs", ptr(ko if even else keys), ptr(po if even else payload), ptr(ko), ptr(po), n, ptr(offsets), S, bits, ptr(ws),
         stream())
    return ko, po


# ------------------------------------------------------------------------------------------
# eval: arg-max + confusion histogram on the device
# ------------------------------------------------------------------------------------------
def argmax_hist(logits, target, hist: Optional[torch.Tensor] = None, want_pred=False):
    """reference main.py:898-909 + metrics.fast_hist (metrics.py:122-126), without the two full-logit
    D2H copies: returns (hist int64 [C,C] on device, pred uint8 [B,H,W] or None)."""
    logits = _chk(logits.detach(), "logits")
    B, C, H, W = logits.shape
    if hist is None:
        hist = torch.zeros(C, C, dtype=torch.int64, device=logits.device)
    pred = torch.empty(B, H, W, dtype=torch.uint8, device=logits.device) if want_pred else None
    tg = target.contiguous() if target is not None else None
    call("mrfp_argmax_hist", ptr(logits), ptr(tg), dt(logits), B * H * W, C, ptr(hist), ptr(pred), stream())
    return hist, pred


# ------------------------------------------------------------------------------------------
# eval: test-time-augmentation accumulator (one launch per scale / flip / window variant) and its closing pass
# ------------------------------------------------------------------------------------------
def _chk_acc(acc, cnt, who):
    for t, name, nd in ((acc, "acc", 4), (cnt, "cnt", 3)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise _lib.MrfpHipError("%s: %s must be a GPU tensor: the HIP path has no CPU fallback" % (who, name))
        if t.dtype != torch.float32 or t.dim() != nd or not t.is_contiguous():
            raise _lib.MrfpHipError("%s: %s must be a contiguous float32 %d-D tensor (got %s %s)"
                                    % (who, name, nd, t.dtype, tuple(t.shape)))
    if tuple(cnt.shape) != tuple(acc.shape[:3]) or cnt.device != acc.device:
        raise _lib.MrfpHipError("%s: cnt %s does not match acc %s" % (who, tuple(cnt.shape), tuple(acc.shape)))
    if not 1 <= acc.shape[3] <= 32:
        raise _lib.MrfpHipError("%s: 1 <= classes <= 32 (acc %s)" % (who, tuple(acc.shape)))


def prob_accum(logits, acc, cnt, rect=None, flip=False, weight=1.0):
    """acc[:, y0:y0+hd, x0:x0+wd, :] += weight * softmax(bilinear_align_corners(flip(logits), (hd, wd))) and
    cnt[:, y0:y0+hd, x0:x0+wd] += weight, in one pass over the rectangle (mrfp_prob_accum).

    logits: class scores [B,ld,hs,ws] in NHWC storage (as the head produces them; ld >= classes, pad channels ignored), float32 /
    bfloat16 / float16.  acc: float32 [B,H,W,classes] dense (class-minor), cnt: float32 [B,H,W]; both updated in place.
    rect = (y0, x0, hd, wd), default the whole accumulator plane.  flip: the scores come from a horizontally mirrored input."""
    _chk_acc(acc, cnt, "prob_accum")
    if not isinstance(logits, torch.Tensor) or not logits.is_cuda or logits.device != acc.device:
        raise _lib.MrfpHipError("prob_accum: logits must live on the accumulator's GPU: the HIP path has no CPU fallback")
    if logits.dim() != 4 or not logits.is_contiguous(memory_format=CL):
        raise _lib.MrfpHipError("prob_accum: logits must be a 4-D tensor in channels_last (NHWC) storage, got %s strides %s"
                                % (tuple(logits.shape), tuple(logits.stride())))
    B, ld, hs, ws = logits.shape
    Ba, H, W, NC = acc.shape
    if B != Ba or ld < NC:
        raise _lib.MrfpHipError("prob_accum: logits %s do not fit acc %s" % (tuple(logits.shape), tuple(acc.shape)))
    y0, x0, hd, wd = (0, 0, H, W) if rect is None else (int(v) for v in rect)
    if y0 < 0 or x0 < 0 or hd < 1 or wd < 1 or y0 + hd > H or x0 + wd > W:
        raise _lib.MrfpHipError("prob_accum: rectangle %s leaves the %d x %d accumulator" % ((y0, x0, hd, wd), H, W))
    call("mrfp_prob_accum", ptr(logits), dt(logits), B, hs, ws, ld, ptr(acc), ptr(cnt), H, W, NC, y0, x0, hd, wd,
         1 if flip else 0, float(weight), stream())


def acc_argmax_hist(acc, cnt, target, hist: Optional[torch.Tensor] = None, want_pred=False, uncovered=None):
    """arg-max over the classes of a prob_accum accumulator + confusion histogram (mrfp_acc_argmax_hist): returns (hist int64
    [classes,classes] on the device, added to when given; pred uint8 [B,H,W] or None), as argmax_hist.  A pixel with cnt == 0 is
    the caller's error; `uncovered` (int64 [1] on the device, added to) receives their number so that it can be checked once,
    without a synchronisation per image."""
    _chk_acc(acc, cnt, "acc_argmax_hist")
    B, H, W, NC = acc.shape
    if target is not None:
        if not target.is_cuda or target.device != acc.device or target.dtype != torch.int64 or tuple(target.shape) != (B, H, W):
            raise _lib.MrfpHipError("acc_argmax_hist: target must be int64 %s on the accumulator's GPU" % ((B, H, W),))
        target = target.contiguous()
    if hist is None:
        hist = torch.zeros(NC, NC, dtype=torch.int64, device=acc.device)
    elif hist.dtype != torch.int64 or tuple(hist.shape) != (NC, NC) or not hist.is_contiguous() or hist.device != acc.device:
        raise _lib.MrfpHipError("acc_argmax_hist: hist must be a contiguous int64 %s on the accumulator's GPU" % ((NC, NC),))
    if uncovered is not None and (uncovered.dtype != torch.int64 or uncovered.numel() != 1 or uncovered.device != acc.device):
        raise _lib.MrfpHipError("acc_argmax_hist: uncovered must be int64 [1] on the accumulator's GPU")
    pred = torch.empty(B, H, W, dtype=torch.uint8, device=acc.device) if want_pred else None
    call("mrfp_acc_argmax_hist", ptr(acc), ptr(cnt), ptr(target), B * H * W, NC, ptr(hist), ptr(pred), ptr(uncovered), stream())
    return hist, pred


# ------------------------------------------------------------------------------------------
# prediction path: upsample + arg-max (+ histogram, confidence, validation loss) in one launch; colour coding
# ------------------------------------------------------------------------------------------
Prediction = collections.namedtuple("Prediction", ("pred", "conf", "hist", "loss_acc"))


def upsample_argmax(P, size, channels, target=None, ignore_index=255, hist=None, per_image=False, want_pred=True, want_conf=False,
                    loss_acc=None):
    """arg-max over the classes of Upsample(P[:, :channels], size) without the full-resolution logits (mrfp_upsample_argmax,
    include/mrfp_hip.h): the label map ops.argmax_hist(ops.upsample_bilinear(P, size, channels=channels).float(), ...) gives, pixel
    for pixel.  P: channel-padded low-resolution class scores [B,ld,Hi,Wi] in NHWC storage (ld a multiple of the 16-byte chunk), as
    model(x, training=False, low_res=True) returns them.  -> Prediction(pred, conf, hist, loss_acc); members not asked for are None.
      pred      uint8 [B,H,W] (want_pred)
      conf      float32 [B,H,W], the largest soft-max probability (want_conf)
      hist      with `target` (int64 [B,H,W]): the confusion histogram int64 [C,C], or [B,C,C] with per_image; `hist` given: added to
      loss_acc  float64 [2] on the device, (sum nll, valid pixels) of the plain cross entropy with ignore_index, ADDED to: pass
                True for a fresh accumulator or the tensor of an earlier call; the validation loss is loss_acc[0] / loss_acc[1]."""
    who = "upsample_argmax"
    if not isinstance(P, torch.Tensor) or not P.is_cuda:
        raise _lib.MrfpHipError("%s: P must be a GPU tensor: the HIP path has no CPU fallback" % who)
    if P.dim() != 4 or not P.is_contiguous(memory_format=CL):
        raise _lib.MrfpHipError("%s: P must be a 4-D tensor in channels_last (NHWC) storage, got %s strides %s"
                                % (who, tuple(P.shape), tuple(P.stride())))
    P = P.detach()
    B, ld, Hi, Wi = P.shape
    H, W, C = int(size[0]), int(size[1]), int(channels)
    if H < 1 or W < 1 or not 1 <= C <= min(64, ld):
        raise _lib.MrfpHipError("%s: size %s / channels %d do not fit P %s (1 <= channels <= 64)" % (who, (H, W), C, tuple(P.shape)))
    if target is not None:
        if (not isinstance(target, torch.Tensor) or target.device != P.device or target.dtype != torch.int64
                or tuple(target.shape) != (B, H, W)):
            raise _lib.MrfpHipError("%s: target must be int64 %s on P's GPU" % (who, (B, H, W)))
        target = target.contiguous()
    elif hist is not None or (loss_acc is not None and loss_acc is not False):
        raise _lib.MrfpHipError("%s: hist / loss_acc need a target" % who)
    hshape = (B, C, C) if per_image else (C, C)
    if target is None:
        hist = None
    elif hist is None:
        hist = torch.zeros(hshape, dtype=torch.int64, device=P.device)
    elif (not isinstance(hist, torch.Tensor) or hist.dtype != torch.int64 or tuple(hist.shape) != hshape or not hist.is_contiguous()
          or hist.device != P.device):
        raise _lib.MrfpHipError("%s: hist must be a contiguous int64 %s on P's GPU" % (who, hshape))
    ws = None
    if loss_acc is None or loss_acc is False:
        loss_acc = None
    else:
        if loss_acc is True:
            loss_acc = torch.zeros(2, dtype=torch.float64, device=P.device)
        elif (not isinstance(loss_acc, torch.Tensor) or loss_acc.dtype != torch.float64 or tuple(loss_acc.shape) != (2,)
              or not loss_acc.is_contiguous() or loss_acc.device != P.device):
            raise _lib.MrfpHipError("%s: loss_acc must be True or a contiguous float64 [2] on P's GPU" % who)
        ws = torch.empty(2 * int(_lib.lib().mrfp_upsample_argmax_nblocks(B, H, W)), dtype=torch.float32, device=P.device)
    if not (want_pred or want_conf or hist is not None or loss_acc is not None):
        raise _lib.MrfpHipError("%s: no output requested" % who)
    pred = torch.empty(B, H, W, dtype=torch.uint8, device=P.device) if want_pred else None
    conf = torch.empty(B, H, W, dtype=torch.float32, device=P.device) if want_conf else None
    call("mrfp_upsample_argmax", ptr(P), ld, ptr(target), dt(P), B, Hi, Wi, H, W, C, int(ignore_index), ptr(pred), ptr(conf),
         ptr(hist), 1 if per_image else 0, ptr(ws), ptr(loss_acc), stream())
    return Prediction(pred, conf, hist, loss_acc)


def _chk_u8(who, name, t, dev=None):
    if not isinstance(t, torch.Tensor) or not t.is_cuda or (dev is not None and t.device != dev):
        raise _lib.MrfpHipError("%s: %s must be a uint8 tensor on the GPU%s: the HIP path has no CPU fallback"
                                % (who, name, "" if dev is None else " of pred"))
    if t.dtype != torch.uint8 or not t.is_contiguous():
        raise _lib.MrfpHipError("%s: %s must be a contiguous uint8 tensor (got %s, strides %s)" % (who, name, t.dtype, tuple(t.stride())))


def colorize(pred_u8, palette, image_u8=None, alpha=0.5, out=None):
    """pred_u8 uint8 [...] -> uint8 [..., 3]: palette[pred] (mrfp_colorize_u8), or with image_u8 (uint8 [..., 3]) the blend
    (a * palette[pred] + (256 - a) * image + 128) >> 8 with a = round(alpha * 256), 0 <= alpha <= 1.  palette: uint8 [256,3] on the
    device (predict.Palette.device_table).  out: a contiguous uint8 [..., 3] to write into (any byte alignment)."""
    who = "colorize"
    _chk_u8(who, "pred_u8", pred_u8)
    dev = pred_u8.device
    _chk_u8(who, "palette", palette, dev)
    if tuple(palette.shape) != (256, 3):
        raise _lib.MrfpHipError("%s: palette must be uint8 [256,3], got %s" % (who, tuple(palette.shape)))
    shape = tuple(pred_u8.shape) + (3,)
    a = 256
    if image_u8 is not None:
        _chk_u8(who, "image_u8", image_u8, dev)
        if tuple(image_u8.shape) != shape:
            raise _lib.MrfpHipError("%s: image_u8 must be uint8 %s, got %s" % (who, shape, tuple(image_u8.shape)))
        if not 0.0 <= float(alpha) <= 1.0:
            raise ValueError("%s: alpha must be in [0, 1], got %r" % (who, alpha))
        a = int(round(float(alpha) * 256))
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=dev)
    else:
        _chk_u8(who, "out", out, dev)
        if tuple(out.shape) != shape:
            raise _lib.MrfpHipError("%s: out must be uint8 %s, got %s" % (who, shape, tuple(out.shape)))
        lo, hi = out.data_ptr(), out.data_ptr() + out.numel()
        for t in (pred_u8, image_u8):
            if t is not None and t.data_ptr() < hi and lo < t.data_ptr() + t.numel():
                raise _lib.MrfpHipError("%s: out overlaps an input" % who)
    if pred_u8.numel():
        call("mrfp_colorize_u8", ptr(pred_u8), ptr(palette), ptr(image_u8), ptr(out), pred_u8.numel(), a, stream())
    return out


# ------------------------------------------------------------------------------------------
# ReLU, input staging, convolution
# ------------------------------------------------------------------------------------------
class _ReLU(torch.autograd.Function):
    """Stand-alone ReLU (only the iw=1/2/5 paths need it; BN/IN fold theirs into the apply pass)."""

    @staticmethod
    def forward(ctx, x):
        x = _chk(x)
        y = _affine_fwd(x, None, None, None, False, True, None)
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        dy = _chk(dy, "dy")
        dx, _ = _affine_bwd(dy, None, y, None, None, None, False, None, False, y)
        return dx


def relu(x):
    return _ReLU.apply(x)


def as_activation(x: torch.Tensor) -> torch.Tensor:
    """Network input -> NHWC storage in the configured activation dtype (cfg.MODEL.ACT_DTYPE)."""
    from .config import cfg
    if not x.is_cuda:
        raise _lib.MrfpHipError("input must live on the GPU (got %s): the HIP path has no CPU fallback" % x.device)
    from . import conv                      # one kernel: NCHW fp32 -> NHWC act dtype, channels padded to a chunk
    return conv.pad_input_channels(x, cfg.MODEL.ACT_DTYPE)


def conv2d_skip(x, weight, bias, stride, padding, dilation, stat_resize=None):
    """(conv(x), alias of x for a skip connection): the gradient arriving on the alias is accumulated in this conv's
    dgrad epilogue."""
    from . import conv
    return conv.conv2d(_chk(x), weight, bias, stride, padding, dilation, None, True, stat_resize=stat_resize)


def conv2d(x, weight, bias, stride, padding, dilation, phys_out=None, stat_resize=None):
    """nn.Conv2d forward/backward on the MFMA implicit-GEMM kernels (mrfp_amd/conv.py).  phys_out: return the
    channel-padded output buffer.  stat_resize: the NearestPlan of the resize the output goes through into a training-mode
    BatchNorm (see conv.conv2d).  There is no other backend: a stock-ROCm (MIOpen) comparison of BASELINE.json
    configs[1] was measured once in round 1 and does not live in the product."""
    from . import conv
    return conv.conv2d(_chk(x), weight, bias, stride, padding, dilation, phys_out, stat_resize=stat_resize)


class _ConcatChannels(torch.autograd.Function):
    """torch.cat(dim=1) of NHWC activations (reference deepv3.py:125, 353): one strided channel-block copy per input
    straight into the wide buffer, and one per slice on the way back."""

    @staticmethod
    def forward(ctx, *tensors):
        ts = [_chk(t) for t in tensors]
        B, _, H, W = ts[0].shape
        Cs = [int(t.shape[1]) for t in ts]
        Ct = sum(Cs)
        y = empty_cl(B, Ct, H, W, ts[0].dtype, ts[0].device)
        c0 = 0
        for t, C in zip(ts, Cs):
            if tuple(t.shape) != (B, C, H, W) or t.dtype != y.dtype:
                raise _lib.MrfpHipError("concat_channels: shape / dtype mismatch")
            call("mrfp_copy_channels", ptr(t), ptr(y), dt(t), B * H * W, C, C, 0, Ct, c0, stream())
            c0 += C
        ctx.Cs = Cs
        return y

    @staticmethod
    def backward(ctx, dy):
        dy = _chk(dy, "dy")
        B, Ct, H, W = dy.shape
        out, c0 = [], 0
        for i, C in enumerate(ctx.Cs):
            if ctx.needs_input_grad[i]:
                g = empty_cl(B, C, H, W, dy.dtype, dy.device)
                call("mrfp_copy_channels", ptr(dy), ptr(g), dt(dy), B * H * W, C, Ct, c0, C, 0, stream())
                out.append(g)
            else:
                out.append(None)
            c0 += C
        return tuple(out)


class _ConcatUpsample(torch.autograd.Function):
    """torch.cat([a, Upsample(b, size)], 1) (the decoder input, reference deepv3.py:349-353) with the bilinear kernel writing
    straight into the concatenation buffer and, backward, reading its channel block of the buffer's gradient: the 256-channel
    upsampled map (302 MB at 16 x 192 x 192) is never copied in either direction."""

    @staticmethod
    def forward(ctx, a, b, Ho, Wo, pad_to):
        a, b = _chk(a), _chk(b)
        B, Ca, H, W = a.shape
        _, Cb, Hi, Wi = b.shape
        if (H, W) != (Ho, Wo) or b.shape[0] != B or a.dtype != b.dtype:
            raise _lib.MrfpHipError("concat_upsample: shape / dtype mismatch")
        Ct = (Ca + Cb + pad_to - 1) // pad_to * pad_to          # physical channels: [a | Upsample(b) | zeros]
        y = empty_cl(B, Ct, H, W, a.dtype, a.device)
        esz = a.element_size()
        if Ct != Ca + Cb:
            y[:, Ca + Cb:].zero_()
        call("mrfp_copy_channels", ptr(a), ptr(y), dt(a), B * H * W, Ca, Ca, 0, Ct, 0, stream())
        call("mrfp_bilinear_fwd_into", ptr(b), y.data_ptr() + Ca * esz, dt(b), B, Hi, Wi, Ho, Wo, Cb, Cb, Ct, stream())
        ctx.dims = (B, Ca, Cb, Hi, Wi, Ho, Wo, Ct)
        return y

    @staticmethod
    def backward(ctx, dy):
        dy = _chk(dy, "dy")
        B, Ca, Cb, Hi, Wi, Ho, Wo, Ct = ctx.dims
        esz = dy.element_size()
        da = db = None
        if ctx.needs_input_grad[0]:
            da = empty_cl(B, Ca, Ho, Wo, dy.dtype, dy.device)
            call("mrfp_copy_channels", ptr(dy), ptr(da), dt(dy), B * Ho * Wo, Ca, Ct, 0, Ca, 0, stream())
        if ctx.needs_input_grad[1]:
            db = empty_cl(B, Cb, Hi, Wi, dy.dtype, dy.device)
            call("mrfp_bilinear_bwd_from", dy.data_ptr() + Ca * esz, ptr(db), dt(dy), B, Hi, Wi, Ho, Wo, Cb, Cb, Ct, stream())
        return da, db, None, None, None


def concat_upsample(a, b, size, pad_to=1):
    """concat_channels([a, upsample_bilinear(b, size)]) without materialising the upsampled map on its own.  Needs both
    channel counts to be whole 16-byte chunks (else the plain composition runs).  pad_to > 1: the result carries zero
    channels up to the next multiple of pad_to (the consuming convolution takes a channel-padded input: its weight pack is
    zero-padded to match) -- the decoder's 48 + 256 = 304 channels become 320 = whole 128-byte K tiles, which puts its 3x3
    convolution, dgrad and wgrad on the aligned / row-reuse kernels."""
    epc = 16 // a.element_size()
    if a.shape[1] % epc or b.shape[1] % epc or (b.shape[2] == 1 and b.shape[3] == 1):
        return concat_channels([a, upsample_bilinear(b, size)])
    return _ConcatUpsample.apply(a, b, int(size[0]), int(size[1]), int(pad_to))


def concat_channels(tensors):
    """torch.cat(dim=1) of NHWC activations (reference deepv3.py:125, 353): pure data movement, done by
    mrfp_copy_channels (a strided channel-block copy) in both directions."""
    return _ConcatChannels.apply(*tensors)


# ------------------------------------------------------------------------------------------
# second-moment statistics for the whitening options (iw = 1, 2, 5)
# ------------------------------------------------------------------------------------------
class _PlaneMean(torch.autograd.Function):
    """mean over H*W per (b, c) in fp32 -- in_data.mean(-1) of reference sync_switchwhiten.py:20, 161."""

    @staticmethod
    def forward(ctx, x):
        x = _chk(x)
        B, C, H, W = x.shape
        nslab, ws = _stats_fwd(x, None)
        out = torch.empty(B, C, dtype=torch.float32, device=x.device)
        call("mrfp_mean_finalize", ptr(ws), B, nslab, H * W, C, ptr(out), ptr(out), _lib.F32, stream())
        ctx.dims, ctx.dtype = (B, C, H, W), x.dtype
        return out

    @staticmethod
    def backward(ctx, g):
        B, C, H, W = ctx.dims
        S = (g.detach().float() / float(H * W)).contiguous()
        dx = empty_cl(B, C, H, W, ctx.dtype, g.device)
        call("mrfp_affine_fwd", None, None, ptr(dx), _lib._DT[ctx.dtype], B, H, W, C, H, W, None, None, None, ptr(S), 1, 0,
             stream())
        return dx


def plane_mean(x):
    return _PlaneMean.apply(x)


class _CrossGram(torch.autograd.Function):
    """G[b] = sum over pixels of a[b,:,p] b[b,:,p]^T  ([B,Ca,Cb], fp32): the bmm(f, f^T) of reference
    instance_whitening.py:36 and sync_switchwhiten.py:23, 165.  Runs on the MFMA weight-gradient kernel
    (the same "reduce over pixels" GEMM), its backward on the 1x1 implicit-GEMM kernel."""

    @staticmethod
    def forward(ctx, a, b):
        a, b = _chk(a, "a"), _chk(b, "b")
        B, Ca, H, W = a.shape
        Cb = b.shape[1]
        esz = a.element_size()
        if (Ca * esz) % 16 or (Cb * esz) % 16 or a.dtype != b.dtype or b.shape[0] != B or b.shape[2:] != a.shape[2:]:
            raise _lib.MrfpHipError("cross_gram: channel counts must make 16-byte chunks and shapes must match")
        G = torch.empty(B, Ca, Cb, dtype=torch.float32, device=a.device)
        ws = wgrad_workspace(H * W, Ca, Cb, a.device)
        abytes, bbytes = H * W * Ca * esz, H * W * Cb * esz
        for i in range(B):
            call("mrfp_conv_wgrad", b.data_ptr() + i * bbytes, a.data_ptr() + i * abytes, G.data_ptr() + i * Ca * Cb * 4,
                 ptr(ws), dt(a), 1, H, W, Cb, Cb, Ca, Ca, 1, 1, H, W, 1, 0, 0, 1, stream())
        ctx.save_for_backward(a, b)
        ctx.same = a.data_ptr() == b.data_ptr()
        return G

    @staticmethod
    def backward(ctx, dG):
        from . import conv
        a, b = ctx.saved_tensors
        B = a.shape[0]
        dG = dG.float()
        da = db = None
        if ctx.same:          # d(x x^T): x (dG + dG^T), returned once (both inputs are the same tensor)
            sym = dG + dG.transpose(1, 2)
            parts = [conv.conv2d(a[i:i + 1].detach(), sym[i].reshape(*sym.shape[1:], 1, 1).contiguous(), None, 1, 0, 1)
                     for i in range(B)]
            return torch.cat(parts, 0), None
        if ctx.needs_input_grad[0]:
            da = torch.cat([conv.conv2d(b[i:i + 1].detach(), dG[i].reshape(*dG.shape[1:], 1, 1).contiguous(), None, 1, 0, 1)
                            for i in range(B)], 0)
        if ctx.needs_input_grad[1]:
            dGt = dG.transpose(1, 2).contiguous()
            db = torch.cat([conv.conv2d(a[i:i + 1].detach(), dGt[i].reshape(*dGt.shape[1:], 1, 1).contiguous(), None, 1, 0, 1)
                            for i in range(B)], 0)
        return da, db


def cross_gram(a, b):
    return _CrossGram.apply(a, b)


def channel_gram(x):
    """sum over pixels of x x^T per image: [B,C,C] fp32 (divide by HW-1 / HW for a covariance)."""
    x = _chk(x)
    return _CrossGram.apply(x, x)


def per_image_matmul(x, Wm, bias=None):
    """y[b,:,p] = Wm[b] @ x[b,:,p] (+ bias[b]): torch.bmm(wm, in_data) of reference sync_switchwhiten.py:217 as one
    1x1 implicit-GEMM convolution per image (weights differ per image); autograd flows into Wm and bias."""
    from . import conv
    x = _chk(x)
    outs = []
    for i in range(x.shape[0]):
        w = Wm[i].reshape(Wm.shape[1], Wm.shape[2], 1, 1)
        outs.append(conv.conv2d(x[i:i + 1], w, None if bias is None else bias[i], 1, 0, 1))
    return torch.cat(outs, 0)


# ------------------------------------------------------------------------------------------
# group whitening passes (csrc/whiten.hip): groups of 16 channels, one read per statistics pass
# ------------------------------------------------------------------------------------------
def _gm_call(a, b, want_sum=True):
    B, C, H, W = a.shape
    dev = a.device
    M = torch.empty(B, C // 16, 16, 16, dtype=torch.float32, device=dev)
    s = torch.empty(B, C, dtype=torch.float32, device=dev) if want_sum else None
    nbytes = int(_lib.lib().mrfp_group_moments_ws_bytes(B, H * W, C))
    if nbytes <= 0:
        raise _lib.MrfpHipError("group_moments: unsupported shape %s (C %% 16 == 0, C <= 1024)" % (tuple(a.shape),))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    call("mrfp_group_moments", ptr(a), ptr(b), ptr(M), ptr(s), ptr(ws), dt(a), B, H * W, C, stream())
    return s, M


def _ga_call(x, Wm, z=None, Vm=None, shift=None):
    B, C, H, W = x.shape
    y = empty_cl(B, C, H, W, x.dtype, x.device)
    call("mrfp_group_apply", ptr(x), ptr(Wm), ptr(z), ptr(Vm), ptr(shift), ptr(y), dt(x), B, H * W, C, stream())
    return y


class _GroupMoments(torch.autograd.Function):
    """s[b,c] = sum_p x, M[b,g] = sum_p x_g x_g^T (16x16 per group): in_data.mean / bmm(x, x^T) of reference
    sync_switchwhiten.py:20-23, 161-165 in one read of x."""

    @staticmethod
    def forward(ctx, x):
        x = _chk(x)
        ctx.save_for_backward(x)
        return _gm_call(x, x)

    @staticmethod
    def backward(ctx, ds, dM):
        (x,) = ctx.saved_tensors
        dM = dM.float()
        sym = (dM + dM.transpose(-1, -2)).contiguous()
        return _ga_call(x, sym, shift=ds.float().contiguous())


def group_moments(x):
    return _GroupMoments.apply(x)


class _GroupApply(torch.autograd.Function):
    """y_g(p) = Wm[b,g] x_g(p) + shift[b]: bmm(wm, in_data) of reference sync_switchwhiten.py:217 with the mean and the
    affine folded in; backward = one transposed apply + one cross-moments pass (dWm = sum_p dy_g x_g^T, dshift = sum_p dy)."""

    @staticmethod
    def forward(ctx, x, Wm, shift):
        x = _chk(x)
        Wm, shift = Wm.float().contiguous(), shift.float().contiguous()
        ctx.save_for_backward(x, Wm)
        return _ga_call(x, Wm, shift=shift)

    @staticmethod
    def backward(ctx, dy):
        x, Wm = ctx.saved_tensors
        dy = _chk(dy, "dy")
        dshift, dWm = _gm_call(dy, x)
        dx = _ga_call(dy, Wm.transpose(-1, -2).contiguous())
        return dx, dWm, dshift


def group_apply(x, Wm, shift):
    return _GroupApply.apply(x, Wm, shift)


class _GroupISqrt(torch.autograd.Function):
    """cov^{-1/2} of [..., 16, 16] covariance matrices by T Newton-Schulz steps (reference sync_switchwhiten.py:206-215),
    forward and backward as one launch each (the backward recomputes the iteration)."""

    @staticmethod
    def forward(ctx, cov, T):
        c = cov.detach().float().contiguous()
        if c.shape[-1] != 16 or c.shape[-2] != 16 or not c.is_cuda:
            raise _lib.MrfpHipError("group_isqrt: [...,16,16] matrices on the GPU expected, got %s" % (tuple(cov.shape),))
        wm = torch.empty_like(c)
        call("mrfp_group_isqrt_fwd", ptr(c), ptr(wm), c.numel() // 256, int(T), stream())
        ctx.save_for_backward(c)
        ctx.T = int(T)
        return wm

    @staticmethod
    def backward(ctx, dwm):
        (c,) = ctx.saved_tensors
        g = dwm.float().contiguous()
        dcov = torch.empty_like(c)
        call("mrfp_group_isqrt_bwd", ptr(c), ptr(g), ptr(dcov), c.numel() // 256, ctx.T, stream())
        return dcov, None


def group_isqrt(cov, T=5):
    return _GroupISqrt.apply(cov, T)


class _AlgebraGraph:
    """The 16x16 algebra between the two activation passes of a whitening layer -- ~100 few-microsecond torch kernels forward, as many
    backward, launch-bound: 1.4 of the 1.6 ms a SwitchWhiten2d layer takes at 16 x 256 x 96 x 96 -- captured ONCE per (module, shape) as two
    hipGraphs: the forward algebra over static (s, M) inputs, and torch.autograd.grad of its outputs over static output gradients (the
    scheme of torch.cuda.make_graphed_callables, written out because the algebra is a closure inside an autograd Function and its
    running-statistics buffers must survive the warm-up runs).  Same kernels in the same order as the eager path: bit-identical results
    (tests/test_whitening_gpu.py).  A replay overwrites the static tensors the backward graph reads, so a second forward of the same layer
    before its backward falls back to the eager algebra: the graph is `busy` while the token of the forward that replayed it is alive
    and not yet consumed by its backward -- the token lives on that forward's autograd node, so a forward whose backward never comes
    (an exception, a dropped loss, a statistics-only pass) frees the graph when its node is collected instead of leaving the layer on
    the eager algebra for the rest of the process."""

    def __init__(self, algebra, s, M, params, buffers):
        self.params = tuple(p for p in params if p.requires_grad)
        saved = [b.detach().clone() for b in buffers]
        self.s = s.detach().clone().requires_grad_(True)
        self.M = M.detach().clone().requires_grad_(True)
        self.inputs = (self.s, self.M) + self.params
        cur = torch.cuda.current_stream()
        side = torch.cuda.Stream()
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            for _ in range(3):                       # warm-up: allocator, lazy kernel attributes -- nothing of that may happen in a capture
                with torch.enable_grad():
                    Wm, shift = algebra(self.s, self.M)
                torch.autograd.grad((Wm, shift), self.inputs, (torch.ones_like(Wm), torch.ones_like(shift)), allow_unused=True)
        cur.wait_stream(side)
        with torch.no_grad():
            for b, v in zip(buffers, saved):         # the warm-up runs updated the running statistics three times: undo
                b.copy_(v)
        pool = torch.cuda.graph_pool_handle()
        self.fwd = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.fwd, pool=pool):
            with torch.enable_grad():
                self.Wm, self.shift = algebra(self.s, self.M)
        self.dWm, self.dshift = torch.zeros_like(self.Wm), torch.zeros_like(self.shift)
        self.bwd = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.bwd, pool=pool):
            self.grads = torch.autograd.grad((self.Wm, self.shift), self.inputs, (self.dWm, self.dshift), allow_unused=True)
        self._owner = None          # weakref to the token of the forward whose backward has not replayed `bwd` yet

    @property
    def busy(self):
        return self._owner is not None and self._owner() is not None

    def acquire(self):
        tok = _GraphToken()
        self._owner = weakref.ref(tok)
        return tok

    def release(self, tok):
        if self._owner is not None and self._owner() is tok:
            self._owner = None


class _GraphToken:
    """Held by the autograd node of the forward that replayed an _AlgebraGraph (weak-referenced by the graph)."""
    __slots__ = ("__weakref__",)


_ALG_GRAPH_CAP = 4           # graphs (each with its private pool) kept per module: one per input shape / mode, least recently used out


_ALG_GRAPHS = weakref.WeakKeyDictionary()      # module -> {(shape, mode, parameter / buffer addresses): _AlgebraGraph}


def whiten_graph_enabled():
    """MRFP_WHITEN_GRAPH=0: the whitening algebra stays eager torch ops (A/B runs, the bit-identity test)."""
    return os.environ.get("MRFP_WHITEN_GRAPH", "1") != "0"


class _GroupWhiten(torch.autograd.Function):
    """moments -> (small algebra, torch autograd) -> apply as ONE node, so that the backward pass touches the activation
    only twice: cross moments of (dy, x), then dx = Wm^T dy + (dM + dM^T) x + ds in a single pass."""

    @staticmethod
    def forward(ctx, x, algebra, graph, *params):
        x = _chk(x)
        s, M = _gm_call(x, x)
        g = graph if (graph is not None and not graph.busy) else None
        ctx.tok = None
        if g is not None:
            g.s.detach().copy_(s)
            g.M.detach().copy_(M)
            g.fwd.replay()
            ctx.tok = g.acquire()
            s_l, M_l, Wm, shift = g.s, g.M, g.Wm, g.shift
            Wm_c, shift_c = Wm.detach().float().clone(), shift.detach().float().contiguous()     # (Wm_c is saved for backward: its own copy)
        else:
            with torch.enable_grad():
                s_l, M_l = s.requires_grad_(True), M.requires_grad_(True)
                Wm, shift = algebra(s_l, M_l)
            Wm_c, shift_c = Wm.detach().float().contiguous(), shift.detach().float().contiguous()
        y = _ga_call(x, Wm_c, shift=shift_c)
        ctx.save_for_backward(x, Wm_c)
        ctx.graph = (s_l, M_l, Wm, shift)
        ctx.alg = g
        ctx.params = params
        return y

    @staticmethod
    def backward(ctx, dy):
        x, Wm_c = ctx.saved_tensors
        s_l, M_l, Wm, shift = ctx.graph
        ctx.graph = None
        dy = _chk(dy, "dy")
        dshift, dWm = _gm_call(dy, x)
        g = ctx.alg
        if g is not None:
            g.dWm.copy_(dWm)
            g.dshift.copy_(dshift.view_as(g.dshift))
            g.bwd.replay()
            grads = tuple(t.detach().clone() if t is not None else None for t in g.grads)
            g.release(ctx.tok)
            ctx.tok = None
            wrt = g.params
        else:
            wrt = tuple(p for p in ctx.params if p.requires_grad)
            grads = torch.autograd.grad((Wm, shift), (s_l, M_l) + wrt, (dWm.to(Wm.dtype), dshift.view_as(shift).to(shift.dtype)),
                                        allow_unused=True)
        ds = grads[0] if grads[0] is not None else torch.zeros_like(s_l)
        dM = grads[1] if grads[1] is not None else torch.zeros_like(M_l)
        sym = (dM + dM.transpose(-1, -2)).float().contiguous()
        dx = _ga_call(dy, Wm_c.transpose(-1, -2).contiguous(), z=x, Vm=sym, shift=ds.float().contiguous())
        # parameter gradients BY IDENTITY of the tensors they were taken with respect to (a captured graph fixed that set at capture
        # time; weight / bias and the two blend weights have equal shapes, so a positional hand-out after a requires_grad_ flip
        # would give one parameter the other's gradient)
        by_param = {id(p): gp for p, gp in zip(wrt, grads[2:])}
        return (dx, None, None) + tuple(by_param.get(id(p)) if p.requires_grad else None for p in ctx.params)


def group_whiten(x, algebra, params, graph=None):
    """y = apply(x, *algebra(sum_p x, sum_p x x^T per group)); `algebra(s [B,C], M [B,C/16,16,16]) -> (Wm [B,C/16,16,16],
    shift [B,C])` is differentiable torch code over a few KB that may use the parameters `params`.  `graph` = (owner module, hashable key of
    everything the algebra bakes in besides `params` -- shape, mode --, the buffers it updates in place) lets the algebra run as two
    captured hipGraphs (_AlgebraGraph); None: eager."""
    g = None
    # (no graph under saved-tensor hooks -- torch.utils.checkpoint(use_reentrant=False), activation offloading: they compare / replay
    #  what the forward SAVES, and the replayed algebra saves different tensors than the eager one the recomputation may fall back to)
    if graph is not None and x.is_cuda and not torch.cuda.is_current_stream_capturing() and not _saved_tensor_hooks_active():
        owner, key, buffers = graph
        cache = _ALG_GRAPHS.setdefault(owner, {})
        # (the requires_grad flags are part of the key: the captured backward graph differentiates with respect to the parameters
        #  that required a gradient AT CAPTURE TIME -- freezing or unfreezing one later must not reuse that graph)
        key = key + tuple(t.data_ptr() for t in params) + tuple(bool(t.requires_grad) for t in params) \
            + tuple(t.data_ptr() for t in buffers)
        g = cache.get(key)
        if g is not None:
            cache[key] = cache.pop(key)              # most recently used last
        elif torch.is_grad_enabled() and not _inside_autograd_engine():
            # Captured HERE, in the caller's plain Python frame, never from inside the autograd machinery: a capture begun inside
            # autograd.Function.forward ends in a segmentation fault in hipStreamEndCapture on this stack (a process abort, not an
            # exception), and a forward issued from inside a backward pass (activation checkpointing, a custom backward that
            # recomputes) would run this build -- a side-stream warm-up, two captures, a re-entrant autograd.grad -- on the engine's
            # thread in that same kind of context.  There the layer simply runs the eager algebra (and uses the graph once a plain
            # forward has built it).  Stand-in inputs: zero sums, identity covariance (well conditioned).
            B, C, H, W = x.shape
            s0 = torch.zeros(B, C, dtype=torch.float32, device=x.device)
            M0 = (torch.eye(16, dtype=torch.float32, device=x.device) * float(H * W)).expand(B, C // 16, 16, 16).contiguous()
            g = cache[key] = _AlgebraGraph(algebra, s0, M0, params, buffers)
            while len(cache) > _ALG_GRAPH_CAP:       # variable input shapes: a bounded number of graphs / private pools per module
                cache.pop(next(iter(cache)))
    return _GroupWhiten.apply(x, algebra, g, *params)


def _saved_tensor_hooks_active():
    f = getattr(torch._C._autograd, "_top_saved_tensors_default_hooks", None)
    try:
        return f is not None and f(False) is not None
    except Exception:       # an interpreter without the query: assume hooks may be active (eager algebra, always correct)
        return True


def _inside_autograd_engine():
    """True while the autograd engine is executing a graph task on this thread (conv._in_backward is this function: a forward
    convolution issued from inside a backward pass -- activation checkpointing, recomputation in a custom backward -- is legitimate
    and must not be taken for the sign of a dead pass)."""
    f = getattr(torch._C, "_current_graph_task_id", None)
    return f is not None and f() != -1


# ------------------------------------------------------------------------------------------
# Fourier amplitude perturbation (build-defined extension)
# ------------------------------------------------------------------------------------------
@lru_cache(maxsize=32)
def _twiddles(n: int, device_str: str) -> torch.Tensor:
    t = np.arange(n, dtype=np.float64)
    tab = np.stack([np.cos(2 * np.pi * t / n), -np.sin(2 * np.pi * t / n)], 1).astype(np.float32)
    return torch.from_numpy(tab).to(device_str)


class _FourierMix(torch.autograd.Function):
    """y = irfft2(rfft2(x) * ratio), ratio = band ? ((1-lam)|F| + lam|F[perm]|)/|F| : 1 (detached).
    The backward applies the same (saved) ratio to the gradient: the operator is real-symmetric."""

    @staticmethod
    def forward(ctx, x, perm, radius, lam, high):
        x = _chk(x)
        B, C, H, W = x.shape
        dev = x.device
        # bins along W the spectra / ratio hold: W/2+1, or floor(radius)+1 on the band-limited (low band) path
        ws = int(_lib.lib().mrfp_fourier_stored_bins(H, W, float(radius), int(bool(high))))
        S = torch.empty(B * H * ws * C * 8, dtype=torch.uint8, device=dev)
        S3 = torch.empty(B * H * ws * C * 8, dtype=torch.uint8, device=dev)
        ratio = torch.empty(B * H * ws * C, dtype=torch.float32, device=dev)
        y = empty_cl(B, C, H, W, x.dtype, dev)
        perm = perm.to(device=dev, dtype=torch.int64).contiguous()
        twH, twW = _twiddles(H, str(dev)), _twiddles(W, str(dev))
        call("mrfp_fourier_mix", ptr(x), ptr(y), ptr(perm), ptr(S), ptr(S3), ptr(ratio), 0, ptr(twH), ptr(twW), dt(x),
             B, H, W, C, float(radius), float(lam), int(bool(high)), stream())
        ctx.save_for_backward(ratio)
        ctx.dims = (B, C, H, W, ws, float(radius), int(bool(high)))
        return y

    @staticmethod
    def backward(ctx, dy):
        (ratio,) = ctx.saved_tensors
        dy = _chk(dy, "dy")
        B, C, H, W, ws, radius, high = ctx.dims
        dev = dy.device
        S = torch.empty(B * H * ws * C * 8, dtype=torch.uint8, device=dev)
        S3 = torch.empty(B * H * ws * C * 8, dtype=torch.uint8, device=dev)
        dx = empty_cl(B, C, H, W, dy.dtype, dev)
        twH, twW = _twiddles(H, str(dev)), _twiddles(W, str(dev))
        # same radius / band as the forward call: they fix the layout of the saved ratio
        call("mrfp_fourier_mix", ptr(dy), ptr(dx), None, ptr(S), ptr(S3), ptr(ratio), 1, ptr(twH), ptr(twW), dt(dy),
             B, H, W, C, radius, 0.0, high, stream())
        return dx, None, None, None, None


def fourier_amplitude_mix(x, perm, radius, lam=1.0, high=False):
    """Per-(b,c) plane: swap/blend the spectral amplitude inside (low band) or outside (high band) `radius`
    with the partner sample perm[b], keep the phase."""
    return _FourierMix.apply(x, perm, radius, lam, high)


# ------------------------------------------------------------------------------------------
# MobileNetV2 layers: depthwise 3x3 convolution, BatchNorm (+ReLU6) that is never synchronised
# ------------------------------------------------------------------------------------------
class _DepthwiseConv2d(torch.autograd.Function):
    """nn.Conv2d(C, C, 3, stride, padding=dilation, dilation, groups=C) (reference network/Mobilenet.py ConvBNReLU with
    groups = hidden_dim) on csrc/conv_dw.hip.  x: [B,Cp,H,W] channels-last, Cp = C rounded up to a 16-byte chunk.  The weight
    gradient runs inline in backward (slabs + a fixed-order sum: bitwise reproducible); it does not join the deferred wgrad
    stream of the MFMA convolutions."""

    @staticmethod
    def forward(ctx, x, weight, bias, stride, dil, stats):
        B, Cp, H, W = x.shape
        C = weight.shape[0]
        Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
        w32 = weight.detach().float().contiguous()
        b32 = _f32(bias)
        y = empty_cl(B, Cp, Ho, Wo, x.dtype, x.device)
        call("mrfp_dwconv_fwd", ptr(x), ptr(w32), ptr(b32), ptr(y), dt(x), B, H, W, Cp, C, Ho, Wo, stride, dil, ptr(stats), stream())
        ctx.save_for_backward(x, w32)
        ctx.geom = (B, Cp, C, H, W, Ho, Wo, stride, dil)
        ctx.wparam, ctx.has_bias = weight, bias is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w32 = ctx.saved_tensors
        B, Cp, C, H, W, Ho, Wo, stride, dil = ctx.geom
        dy = _chk(dy, "dy")
        if dy.shape[1] != Cp:            # the caller saw the logical C channels of a padded output: back to the channel pitch
            dp = zeros_cl(B, Cp, Ho, Wo, dy.dtype, dy.device)
            dp[:, :dy.shape[1]] = dy
            dy = dp
        if dy.dtype != x.dtype:
            raise _lib.MrfpHipError("depthwise_conv2d: gradient dtype %s differs from the activation dtype %s" % (dy.dtype, x.dtype))
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = empty_cl(B, Cp, H, W, dy.dtype, dy.device)
            call("mrfp_dwconv_dgrad", ptr(dy), ptr(w32), ptr(dx), dt(dy), B, H, W, Cp, C, Ho, Wo, stride, dil, stream())
        if ctx.needs_input_grad[1]:
            nbytes = int(_lib.lib().mrfp_dwconv_wgrad_ws_bytes(dt(x), B, Ho, Cp))
            ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
            sink = grad_sink(ctx.wparam)
            out = sink if sink is not None else torch.empty((C, 1, 3, 3), dtype=torch.float32, device=x.device)
            call("mrfp_dwconv_wgrad", ptr(x), ptr(dy), ptr(out), ptr(ws), dt(x), B, H, W, Cp, C, Ho, Wo, stride, dil, stream())
            if sink is not None:
                notify_grad(ctx.wparam)
            else:
                dw = out.to(ctx.wparam.dtype)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            db = channel_sums(dy, C)
        return dx, dw, db, None, None, None


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (int(v), int(v))


def depthwise_conv2d(x, weight, bias, stride, padding, dilation):
    """F.conv2d(x, weight, bias, stride, padding, dilation, groups=C) for weight [C,1,3,3], padding == dilation, stride 1 or 2.
    Returns [B,C,Ho,Wo] channels-last; a bias-free convolution tags its output with the BatchNorm partial statistics its kernel
    wrote (y._mrfp_colstats, as the MFMA convolutions do), so the BatchNorm behind it skips its statistics pass."""
    from . import conv
    st, dl, pd = _pair(stride), _pair(dilation), _pair(padding)
    C = weight.shape[0]
    if weight.dim() != 4 or tuple(weight.shape[1:]) != (1, 3, 3) or st[0] != st[1] or st[0] not in (1, 2) \
            or dl[0] != dl[1] or dl[0] < 1 or pd != dl:
        raise _lib.MrfpHipError("depthwise_conv2d: weight %s stride %s padding %s dilation %s is not a depthwise 3x3 with padding = "
                                "dilation and stride 1 or 2" % (tuple(weight.shape), st, pd, dl))
    x = _chk(x)
    epc = conv._epc(x.dtype)
    Cp = conv._round_up(C, epc)
    if x.shape[1] != Cp:
        if x.shape[1] != C:
            raise _lib.MrfpHipError("depthwise_conv2d: input has %d channels, weight %s expects %d" % (x.shape[1], tuple(weight.shape), C))
        xp = zeros_cl(x.shape[0], Cp, x.shape[2], x.shape[3], x.dtype, x.device)     # chunk-pad the channels (copy)
        xp[:, :C] = x
        x = xp
    ws = None
    if bias is None and conv.FUSE_STATS[0] and Cp == C:
        B, Ho = x.shape[0], (x.shape[2] - 1) // st[0] + 1
        rows = B * int(_lib.lib().mrfp_dwconv_nslab(dt(x), B, Ho, Cp))
        ws = torch.empty(rows * 2 * Cp, dtype=torch.float32, device=x.device)
    y = _DepthwiseConv2d.apply(x, weight, bias, st[0], dl[0], ws)
    if ws is not None:                    # consumed by the BatchNorm behind it (statistics pass skipped)
        y._mrfp_colstats = conv.ConvStats(ws, rows, y.numel() // Cp, ws, rows, 0, None, y._version)
    if Cp != C:
        y = y[:, :C].contiguous(memory_format=CL)
    return y
