"""nn.Conv2d forward / backward on the MFMA implicit-GEMM kernels (mrfp_amd/csrc/conv.hip).

The OIHW fp32 Parameter stays the master copy (checkpoint ABI, optimiser state); the kernels read
two derived packs in the activation dtype -- forward [N][R][S][C] and dgrad [C][R][S][N] with flipped
taps -- rebuilt by one small kernel whenever the Parameter's version counter moves (optimizer
step, HRFP re-initialisation, load_state_dict).
"""
from __future__ import annotations

import collections
import ctypes
import os as _os
import warnings
import weakref
from typing import Any, NamedTuple, Optional

import torch

from . import _lib, ops
from ._lib import call, dt, ptr, stream
from .ops import CL, GRAD_DEFERRED, _chk, channel_sums, empty_cl, grad_sink, notify_grad, wgrad_workspace, zeros_cl
from .ops import _inside_autograd_engine as _in_backward
from .skipgrad import ALIAS, GATE, LOWRANK, AliasCell, alias_cell, gateable, mask_possible, ungate, unlowrank

FUSE_STATS = [_os.environ.get("MRFP_FUSE_STATS", "1") != "0"]   # conv epilogues emit BatchNorm partial statistics for bias-free convolutions


class ConvStats(NamedTuple):
    """The statistics a convolution's epilogue wrote (y._mrfp_colstats; layout: mrfp_conv_stats_layout)."""
    final: torch.Tensor        # the rows to hand to a BatchNorm finalize (compacted for large launches)
    final_count: int           # ... their count
    elements: int              # the element count per channel they sum over
    rows: torch.Tensor         # the RAW per-row-block rows (an InstanceNorm consumer needs them per image: ops._in_plane_sums)
    row_blocks: int            # ... their count
    block_rows: int            # output rows of one row block; < 0: -(rows per image); 0: resize-weighted, no per-image use
    resize_plan: Any           # the ops.NearestPlan the statistics are weighted for (conv2d(stat_resize=): its one consumer), or None
    version: int               # the tagged tensor's _version when it was tagged: modified in place since, the tag is ignored


WSTATS = [_os.environ.get("MRFP_WSTATS", "1") != "0"]
WSTATS_HITS = [0]


def _epc(dtype) -> int:
    """elements per 16-byte chunk"""
    return 4 if dtype == torch.float32 else 8


def _round_up(n, m):
    return (n + m - 1) // m * m


def _pad_to_chunk(x):
    """x with its channel count padded to a 16-byte chunk, by copy (e.g. a raw 3-channel image)"""
    C, Cp = x.shape[1], _round_up(x.shape[1], _epc(x.dtype))
    if Cp == C:
        return x
    xp = zeros_cl(x.shape[0], Cp, x.shape[2], x.shape[3], x.dtype, x.device)
    xp[:, :C] = x
    return xp


# ---- weight packs ---------------------------------------------------------------------------------------------------------------
# A pack is fresh while its version stamp equals the one that _plain_version / _fold_version build now.
_PACKS = {}      # id(weight Parameter) -> _WeightPacks; entry dropped when the Parameter dies
_EPOCH = [0]     # bumped by writers that bypass autograd's version counters (the fused SGD kernel)
_BATCH = {}      # (tag, dtype) -> the cached job table of a batched re-pack (_batched_repack)
_REPACK_LISTS = {}       # tag -> the (weights, biases) of the last repack_weights() call
_new_key = tuple.__new__         # (a named key built at the cost of a bare tuple: get_pack's hit path runs ~250 times per step)
_PlainKey = collections.namedtuple("_PlainKey", "dtype Cphys Nphys weight bias")          # weight, bias: data pointers (no bias: 0)
_FoldKey = collections.namedtuple("_FoldKey", "dtype Cphys Nphys depthwise tensors")     # tensors: the pointers of _fold_tensors (or 0)
# the packs of one weight: plain {_PlainKey: _Pack} (get_pack: forward + dgrad) and folded {_FoldKey: _Pack} (get_folded_pack), apart
_WeightPacks = collections.namedtuple("_WeightPacks", "plain folded")
_NO_PACKS = _WeightPacks({}, {})         # of a weight without a cache entry: read, never written
_PACK_JOB = ([("w", "<u8"), ("wf", "<u8"), ("wd", "<u8"), ("dims", "<i4", (6,))], 48)           # PackJob of csrc/conv_pack.hip
_FOLD_JOB = ([("ptrs", "<u8", (8,)), ("eps", "<f4"), ("dims", "<i4", (7,))], 96)                # FoldJob


class _Pack:
    __slots__ = ("key", "wref", "version", "wf", "wd", "bias")

    def __init__(self, key, weight):
        self.key, self.wref = key, weakref.ref(weight)
        self.version = self.wf = self.wd = self.bias = None          # (the buffers: get_pack / _fold_slot, right away)


def _packs_of(weight, create=False):
    """The packs of this weight: made on first use (create), dropped when the Parameter dies."""
    rec = _PACKS.get(id(weight), _NO_PACKS)
    if rec is _NO_PACKS and create:
        rec = _PACKS[id(weight)] = _WeightPacks({}, {})
        weakref.finalize(weight, _PACKS.pop, id(weight), None)
    return rec


def invalidate_packs():
    _EPOCH[0] += 1


def _plain_version(weight, bias):
    return (weight._version, bias._version if bias is not None else 0, _EPOCH[0])


def _capturing(device) -> bool:
    """Under hipGraph capture (harness.Trainer.enable_graph) a pack kernel is only recorded, not run: a pack written under capture
    must stay "stale" for eager code, and the recorded kernel re-packs on every replay.  So who packs stamps only when this is false."""
    return device.type == "cuda" and torch.cuda.is_current_stream_capturing()


def get_pack(weight: torch.Tensor, bias: Optional[torch.Tensor], dtype, Cphys: int, Nphys: int) -> _Pack:
    key = _new_key(_PlainKey, (dtype, Cphys, Nphys, weight.data_ptr(), bias.data_ptr() if bias is not None else 0))
    ver = _plain_version(weight, bias)
    packs = _packs_of(weight, True).plain
    pk = packs.get(key)
    if pk is not None and pk.version == ver:
        return pk
    N, C, R, S = weight.shape
    dev = weight.device
    w32 = weight.detach()
    if w32.dtype != torch.float32 or not w32.is_contiguous():
        w32 = w32.float().contiguous()
    if pk is None:
        pk = _Pack(key, weight)
        pk.wf = torch.empty(Nphys * R * S * Cphys, dtype=dtype, device=dev)
        # dgrad pack [Cphys][R][S][Nphys]: the rows of pad input channels (c >= C) stay zero, so a dgrad launch over a
        # channel-padded input writes exact zeros into the pad channels of dx
        pk.wd = (torch.zeros(Cphys * R * S * Nphys, dtype=dtype, device=dev) if Cphys != C
                 else torch.empty(C * R * S * Nphys, dtype=dtype, device=dev))
    call("mrfp_pack_weight", ptr(w32), ptr(pk.wf), ptr(pk.wd), _lib._DT[dtype], N, C, R, S, Nphys, Cphys, stream())
    if bias is not None:
        if pk.bias is None:                      # allocated once (pad entries stay zero), refreshed in place
            pk.bias = torch.zeros(Nphys, dtype=torch.float32, device=dev)
        pk.bias[:N].copy_(bias.detach())
    if not _capturing(dev):
        pk.version = ver
    packs[key] = pk
    return pk


def _job_table(rows, record):
    """rows = [(the fields of one job record, its work items)], record = (numpy fields, bytes per record) -> the records as a host
    byte tensor, the int64 prefix table of the work items as a host tensor, and their total: the operands of a batched launch."""
    import numpy as np
    rec = np.zeros(len(rows), dtype=np.dtype(record[0]))
    assert rec.itemsize == record[1]
    prefix = np.zeros(len(rows) + 1, dtype=np.int64)
    for i, (fields, work) in enumerate(rows):
        rec[i] = fields
        prefix[i + 1] = prefix[i] + work
    return torch.from_numpy(rec.view(np.uint8).copy()), torch.from_numpy(prefix), int(prefix[-1])


def _packable(pk, w, with_bias=False):
    return ((with_bias or pk.bias is None) and w.dtype == torch.float32 and w.is_contiguous()
            and w.shape[2] * w.shape[3] <= 9)        # the brick kernel holds up to 3x3 taps; the 7x7 stem packs lazily


def _batched_repack(todo, tag, biases=None, launch=True):
    """ONE mrfp_pack_weights_batched launch per dtype for the (plain pack, weight) pairs in `todo`; the job table is cached
    per (tag, dtype) and rebuilt only when the set of packs changes."""
    by_dtype = {}
    for pk, w in todo:
        by_dtype.setdefault(pk.key.dtype, []).append((pk, w))
    for dtype, items in by_dtype.items():
        sig = tuple((id(pk), w.data_ptr(), pk.wf.data_ptr(), pk.wd.data_ptr()) for pk, w in items)
        dev = items[0][1].device
        st = _BATCH.get((tag, dtype))
        if st is None or st["sig"] != sig:
            rows = []
            for pk, w in items:
                N, C, R, S = w.shape
                Nphys, Cphys = pk.key.Nphys, pk.key.Cphys
                bc = 64 if R * S == 1 else 8                                           # input channels per brick (conv.hip)
                rows.append(((w.data_ptr(), pk.wf.data_ptr(), pk.wd.data_ptr(), (N, C, R, S, Nphys, Cphys)),
                             ((Nphys + 63) // 64) * ((Cphys + bc - 1) // bc)))
            # (pinned staging + asynchronous copies: legal while a hipGraph is being captured too -- the first capture pass of
            #  Trainer.enable_graph() is the first time the HRFP packs exist when the re-initialisation runs; the host copies stay
            #  alive in the table entry for the graph's memcpy nodes)
            hj, hp, total = _job_table(rows, _PACK_JOB)
            if dev.type == "cuda":
                hj, hp = hj.pin_memory(), hp.pin_memory()
            st = _BATCH[(tag, dtype)] = {"sig": sig, "host": (hj, hp), "jobs": hj.to(dev, non_blocking=True),
                                         "prefix": hp.to(dev, non_blocking=True), "total": total, "n": len(items)}
        if not launch:
            continue
        call("mrfp_pack_weights_batched", ptr(st["jobs"]), ptr(st["prefix"]), st["n"], st["total"], _lib._DT[dtype], stream())
        capturing = _capturing(dev)
        for pk, w in items:
            b = biases.get(id(w)) if biases else None
            if b is not None and pk.bias is not None:           # packs with a bias (the HRFP convolutions): refresh the fp32 copy
                pk.bias[:w.shape[0]].copy_(b.detach())
            if not capturing:
                pk.version = _plain_version(w, b)


def repack_all():
    """Re-packs, in ONE launch, every cached bias-free pack whose fp32 master changed (called by the harness right after
    the fused SGD kernel rewrote the parameter arena; 124 launches of ~7 us per step otherwise).  Packs with a bias
    (final2) keep the lazy per-layer path; the frozen HRFP weights, re-drawn at the start of a forward, go through
    repack_weights(); folded inference packs are rebuilt lazily (get_folded_pack)."""
    todo = []
    for rec in _PACKS.values():
        for pk in rec.plain.values():
            w = pk.wref()
            if w is not None and w.requires_grad and _packable(pk, w):
                todo.append((pk, w))
    _batched_repack(todo, "trainable")


def _repack_selection(weights, biases):
    """-> the plain packs of `weights` that a batched launch refreshes, as (pack, weight) pairs, and id(weight) -> its bias"""
    todo = []
    bmap = {id(w): b for w, b in zip(weights, biases)} if biases is not None else {}
    for w in weights:
        b = bmap.get(id(w))
        for pk in _packs_of(w).plain.values():
            if _packable(pk, w, with_bias=b is not None) and (pk.bias is None) == (b is None) \
                    and pk.key.bias == (b.data_ptr() if b is not None else 0):
                todo.append((pk, w))
    return todo, bmap


def repack_weights(weights, tag="list", biases=None):
    """The same for an explicit list of weights that were just rewritten (the HRFP branch's convolutions after their
    re-initialisation: reference deepv3.py:290-299 re-draws them at the start of a forward; 28 pack launches per step
    otherwise).  `biases`: the bias Parameter of each weight (or None) -- a pack with a bias gets its fp32 copy refreshed here too.
    Weights without a cached pack yet are left to the lazy path."""
    _REPACK_LISTS[tag] = ([weakref.ref(w) for w in weights], [weakref.ref(b) if b is not None else None for b in biases]
                          if biases is not None else None)
    todo, bmap = _repack_selection(weights, biases)
    # the masters were just rewritten -- possibly through a flat arena they are views of (deepv3._hrfp_arena), which does not bump
    # the parameters' own version counters: every cached pack of these weights that the batched launch does NOT refresh (another
    # padding, a 7x7 filter, a bias mismatch, a folded pack) is marked stale here and rebuilt lazily at its next use
    sel = {id(pk) for pk, _ in todo}
    for w in weights:
        for pk in (*_packs_of(w).plain.values(), *_packs_of(w).folded.values()):
            if id(pk) not in sel:
                pk.version = None
    _batched_repack(todo, tag, bmap)


def prebuild_repack_tables():
    """Builds (without launching) the job tables of every repack_weights() list seen so far, for the packs that exist NOW: called
    by harness.Trainer between the eager warm-up pass of a hipGraph capture and the capture itself -- in the very first step the
    packs of the HRFP convolutions come into being AFTER the re-initialisation ran, so the capture pass would be the first to
    need the table, and a host -> device copy cannot be captured."""
    for tag, (wrefs, brefs) in list(_REPACK_LISTS.items()):
        weights = [r() for r in wrefs]
        if any(w is None for w in weights):          # the model is gone
            del _REPACK_LISTS[tag]
            continue
        biases = [r() if r is not None else None for r in brefs] if brefs is not None else None
        todo, bmap = _repack_selection(weights, biases)
        _batched_repack(todo, tag, bmap, launch=False)


# ---- folded inference packs (mrfp_amd/inference.py) -----------------------------------------------------------------
# conv -> eval-mode BatchNorm as ONE convolution: forward pack round(w * A[n]) from the fp32 master, fp32 bias S (mrfp_pack_weight_folded).
# The packs live in the folded dictionary of their weight's cache entry.  They are stale when the weight, the convolution's
# bias or any of the four BatchNorm tensors changed: their autograd version counters (optimizer.step of torch, load_state_dict,
# any in-place torch operator), _EPOCH (invalidate_packs(): the fused SGD kernel, checkpoint loads, broadcasts) and
# ops.RUNNING_STATS_EPOCH -- bumped by every training-mode BatchNorm forward, whose kernel updates the running statistics through raw
# pointers that no version counter sees.  Nothing is read back to the host to decide.
FOLD_PACK_LAUNCHES = [0]      # fold-pack launches so far (tests)
_FOLD_SETS = []               # weak references to the pair lists of models with the fold enabled: a stale pack refolds its whole set


def _fold_tensors(weight, conv_bias, norm):
    return (weight, conv_bias, norm.weight, norm.bias, norm.running_mean, norm.running_var)


def _fold_key(weight, conv_bias, norm, dtype, Cphys, Nphys, depthwise):
    return _FoldKey(dtype, Cphys, Nphys, bool(depthwise), tuple(t.data_ptr() if t is not None else 0 for t in _fold_tensors(weight, conv_bias, norm)))


def _fold_version(weight, conv_bias, norm):
    return tuple(t._version if t is not None else 0 for t in _fold_tensors(weight, conv_bias, norm)) + \
        (float(norm.eps), _EPOCH[0], ops.RUNNING_STATS_EPOCH[0])


def _fold_slot(weight, key):
    packs = _packs_of(weight, True).folded
    pk = packs.get(key)
    if pk is None:
        N, _, R, S = weight.shape
        pk = packs[key] = _Pack(key, weight)
        pk.wf = torch.empty(key.Nphys * R * S * key.Cphys, dtype=torch.float32 if key.depthwise else key.dtype, device=weight.device)
        pk.bias = torch.empty(key.Nphys, dtype=torch.float32, device=weight.device)
    return pk


# One fold job: eight pointers in the order of the FoldJob record of csrc/conv_pack.hip (None: no such tensor), eps, and the dims
# (N, C, R, S, Nphys, Cphys, depthwise), of which the first six are the single entry point's
_FoldJob = collections.namedtuple("_FoldJob", "weight wf conv_bias gamma beta mean var shift eps dims")


def _fold_job(weight, conv_bias, norm, pk) -> _FoldJob:
    N, C, R, S = weight.shape
    for t, what in zip(_fold_tensors(weight, conv_bias, norm), ("weight", "conv bias", "norm weight", "norm bias", "running_mean", "running_var")):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous()):
            raise _lib.MrfpHipError("folded inference: %s must be a contiguous fp32 tensor (got %s)" % (what, t.dtype))
    if norm.running_mean is None or norm.running_var is None:
        raise _lib.MrfpHipError("folded inference: the BatchNorm has no running statistics")
    dims = (N, 1, R, S, pk.key.Nphys, 1, 1) if pk.key.depthwise else (N, C, R, S, pk.key.Nphys, pk.key.Cphys, 0)
    return _FoldJob(ptr(weight), ptr(pk.wf), ptr(conv_bias), ptr(norm.weight), ptr(norm.bias), ptr(norm.running_mean),
                    ptr(norm.running_var), ptr(pk.bias), float(norm.eps), dims)


def fold_packs_batched(items):
    """ONE mrfp_pack_weights_folded_batched launch per pack dtype for `items` = [(weight, conv_bias, norm, key)]."""
    by_dtype = {}
    for it in items:
        by_dtype.setdefault(it[3].dtype, []).append(it)
    for dtype, its in by_dtype.items():
        rows, pks = [], []
        for w, cb, norm, key in its:
            pk = _fold_slot(w, key)
            job = _fold_job(w, cb, norm, pk)
            N, C, R, S, Nphys, Cphys, _ = job.dims
            rows.append(((tuple(p or 0 for p in job[:8]), job.eps, job.dims), Nphys * R * S * Cphys + Nphys))
            pks.append(pk)
        hj, hp, total = _job_table(rows, _FOLD_JOB)
        dev = its[0][0].device
        jobs, pre = hj.to(dev), hp.to(dev)
        call("mrfp_pack_weights_folded_batched", ptr(jobs), ptr(pre), len(its), total, _lib._DT[dtype], stream())
        FOLD_PACK_LAUNCHES[0] += 1
        for (w, cb, norm, key), pk in zip(its, pks):
            pk.version = _fold_version(w, cb, norm)


def register_fold_set(pairs):
    """pairs: [(conv module, norm module)] of a model whose fold was enabled (inference.fold_norms): when one of their packs is
    found stale, every stale pack of the set is rebuilt in the same launch."""
    _FOLD_SETS[:] = [r for r in _FOLD_SETS if r() is not None]
    _FOLD_SETS.append(weakref.ref(pairs))


def _refold_set(weight, dtype):
    """Rebuilds, in one launch, the stale packs of the registered set `weight` belongs to (packs that exist, plus this dtype's
    standard geometry for pairs that have none yet).  False: the weight is in no set."""
    for r in _FOLD_SETS:
        pairs = r()
        if pairs is None or not any(c.weight is weight for c, _ in pairs):
            continue
        items = []
        epc = _epc(dtype)
        for c, n in pairs:
            w, cb = c.weight, c.bias
            if not w.is_cuda:
                continue
            depthwise = c.groups != 1
            N, C = w.shape[0], w.shape[1]
            packs = _packs_of(w).folded
            std = _fold_key(w, cb, n, dtype, 1 if depthwise else _round_up(C, epc), N if depthwise else _round_up(N, epc), depthwise)
            ver = _fold_version(w, cb, n)
            for k in list(packs) if std in packs else [*packs, std]:
                pk = packs.get(k)
                if k.tensors == std.tensors and (pk is None or pk.version != ver):
                    items.append((w, cb, n, k))
        fold_packs_batched(items)
        return True
    return False


def get_folded_pack(weight, conv_bias, norm, dtype, Cphys, Nphys, depthwise=False) -> _Pack:
    key = _fold_key(weight, conv_bias, norm, dtype, Cphys, Nphys, depthwise)
    ver = _fold_version(weight, conv_bias, norm)
    pk = _packs_of(weight).folded.get(key)
    if pk is not None and pk.version == ver:
        return pk
    capturing = _capturing(weight.device)
    if not capturing and _refold_set(weight, dtype):
        pk = _packs_of(weight).folded.get(key)
        if pk is not None and pk.version == ver:
            return pk
    pk = _fold_slot(weight, key)
    job = _fold_job(weight, conv_bias, norm, pk)
    # (the single entry writes the pack in the dtype it is given: a depthwise fp32 [C][9] pack is an fp32 job)
    call("mrfp_pack_weight_folded", job.weight, job.wf, job.conv_bias, job.gamma, job.beta, job.mean, job.var, job.eps, job.shift,
         _lib.F32 if depthwise else _lib._DT[dtype], *job.dims[:6], stream())
    FOLD_PACK_LAUNCHES[0] += 1
    if not capturing:
        pk.version = ver
    return pk


def conv2d_folded(x, conv, norm, act=0, res=None):
    """act(BN_eval(conv(x)) (+ res)) as ONE mrfp_conv_fwd_act launch (no normalisation launch).  No autograd: the caller
    (network.mynn.conv_norm) only comes here with gradients disabled.  act: 0 none, 1 ReLU, 2 ReLU6."""
    if torch.is_grad_enabled():
        raise _lib.MrfpHipError("conv2d_folded: the folded form has no backward (call it under torch.no_grad())")
    weight, bias = conv.weight, conv.bias
    x = _pad_to_chunk(_chk(x))
    st = conv.stride[0]
    ph, pw = conv.padding
    dl = conv.dilation[0]
    N, C, R, S = weight.shape
    if x.shape[1] < C:
        raise _lib.MrfpHipError("conv2d_folded: input has %d channels, weight expects %d" % (x.shape[1], C))
    B, Cphys, H, W = x.shape
    Nphys = _round_up(N, _epc(x.dtype))
    Ho, Wo = _out_size(H, R, st, ph, dl), _out_size(W, S, st, pw, dl)
    if res is not None:
        res = _chk(res, "res")
        if tuple(res.shape) != (B, Nphys, Ho, Wo) or res.dtype != x.dtype:
            raise _lib.MrfpHipError("conv2d_folded: the residual %s / %s does not match the output (%d, %d, %d, %d) / %s"
                                    % (tuple(res.shape), res.dtype, B, Nphys, Ho, Wo, x.dtype))
    pk = get_folded_pack(weight, bias, norm, x.dtype, Cphys, Nphys)
    y = empty_cl(B, Nphys, Ho, Wo, x.dtype, x.device)
    _lib.NOTE[0] = (C, N)
    call("mrfp_conv_fwd_act", ptr(x), ptr(pk.wf), ptr(pk.bias), ptr(y), dt(x), B, H, W, Cphys, Nphys, Nphys, R, S, Ho, Wo,
         st, ph, pw, dl, 1, ptr(res), int(act), stream())
    if Nphys != N:
        y = y[:, :N].contiguous(memory_format=CL)
    return y


def depthwise_conv2d_folded(x, conv, norm, act=0):
    """The depthwise 3x3 form of conv2d_folded (mrfp_dwconv_fwd_act over the scaled fp32 taps)."""
    if torch.is_grad_enabled():
        raise _lib.MrfpHipError("depthwise_conv2d_folded: the folded form has no backward")
    weight = conv.weight
    st, dl, pd = conv.stride, conv.dilation, conv.padding
    C = weight.shape[0]
    if tuple(weight.shape[1:]) != (1, 3, 3) or st[0] != st[1] or st[0] not in (1, 2) or dl[0] != dl[1] or tuple(pd) != tuple(dl):
        raise _lib.MrfpHipError("depthwise_conv2d_folded: weight %s stride %s padding %s dilation %s is not a depthwise 3x3 with "
                                "padding = dilation and stride 1 or 2" % (tuple(weight.shape), st, pd, dl))
    x = _chk(x)
    Cp = _round_up(C, _epc(x.dtype))
    if x.shape[1] == C:
        x = _pad_to_chunk(x)
    if x.shape[1] != Cp:
        raise _lib.MrfpHipError("depthwise_conv2d_folded: input has %d channels, weight expects %d" % (x.shape[1], C))
    B, _, H, W = x.shape
    Ho, Wo = (H - 1) // st[0] + 1, (W - 1) // st[0] + 1
    pk = get_folded_pack(weight, conv.bias, norm, x.dtype, 1, C, depthwise=True)
    y = empty_cl(B, Cp, Ho, Wo, x.dtype, x.device)
    call("mrfp_dwconv_fwd_act", ptr(x), ptr(pk.wf), ptr(pk.bias), ptr(y), dt(x), B, H, W, Cp, C, Ho, Wo, st[0], dl[0], int(act), stream())
    if Cp != C:
        y = y[:, :C].contiguous(memory_format=CL)
    return y


def _out_size(H, R, stride, pad, dil):
    return (H + 2 * pad - dil * (R - 1) - 1) // stride + 1


# ---- weight gradients: one launcher, one scheduler --------------------------------------------------------------------------------
# The weight gradient feeds nothing but the optimizer, so it may run beside the dgrad chain and it may wait.
# Second stream (MRFP_WGRAD_STREAM): with a gradient arena present (harness.FlatArena) the launches go to a side stream, concurrently
# with the dgrad chain of the main stream (their workgroups fill the tails / small-kernel gaps of that chain).  Ordering: the side
# stream waits for dy (an event on the main stream); the consumers of the arena (optimizer step, gradient all-reduce) wait for the
# side stream (harness.Trainer / GradSync, join_wgrad_stream()).
# Grouped, deferred launches (MRFP_WGRAD_GROUP): a ResNet stage is `blocks` Bottlenecks of ONE geometry (reference
# network/Resnet.py:579-585 _make_layer; autograd of Resnet.py:202-216 yields their weight gradients one launch at a time).  At
# M = 16*48*48 a single launch has 16-72 output tiles and needs 21-32 K' splits to fill 256 CUs -- 12 K' tiles per workgroup behind a
# prologue, and fp32 slabs of 20-30x the size of dW written and read again.  So backward only QUEUES (x, dy, sink) per launch geometry
# and a whole queue runs as one grouped launch + one slab reduction -- when a queue is full or complete, when backward leaves a stage
# (wgrad_boundary), and when backward ends.  _WgradScheduler decides all of that; _launch_wgrads is the only launcher.
USE_WGRAD_STREAM = [_os.environ.get("MRFP_WGRAD_STREAM", "1") != "0"]
GROUP_WGRAD = [_os.environ.get("MRFP_WGRAD_GROUP", "1") != "0"]
WGRAD_GROUP_LAUNCHES = collections.deque(maxlen=4096)   # sizes of the last launches the scheduler issued (tests / diagnostics; bounded)
_DEBUG_SKIP_WGRAD = _os.environ.get("MRFP_DEBUG_SKIP_WGRAD") == "1"     # timing diagnostics only: weight gradients are NOT computed


def _launch_wgrads(sig, items, side):
    """ONE launch for `items` = [(x, dy, out)] of launch geometry `sig`: mrfp_conv_wgrad for one problem, mrfp_conv_wgrad_grouped for
    several.  side: None = on the current stream; else on that stream, behind everything the current one holds so far (the operands
    are recorded on it, the scheduler is told that a join is due).  Who is notified, and when this is called, is the caller's
    matter; no autograd callback is registered here (flush_wgrads() also runs outside a backward pass: harness.GradSync.finish)."""
    (dtype, B, H, W, Cphys, C, N, Nphys, R, S, Ho, Wo, stride, pad_h, pad_w, dil) = sig
    n = len(items)

    def run():
        ws = wgrad_workspace(B * Ho * Wo, N, R * S * Cphys, items[0][0].device, n)
        if n == 1:
            x, dy, out = items[0]
            call("mrfp_conv_wgrad", ptr(x), ptr(dy), ptr(out), ptr(ws), _lib._DT[dtype], B, H, W, Cphys, C, N, Nphys, R, S,
                 Ho, Wo, stride, pad_h, pad_w, dil, stream())
            return
        arr = ctypes.c_void_p * n
        xs, dys, dws = arr(*[ptr(i[0]) for i in items]), arr(*[ptr(i[1]) for i in items]), arr(*[ptr(i[2]) for i in items])
        call("mrfp_conv_wgrad_grouped", xs, dys, dws, n, ptr(ws), _lib._DT[dtype], B, H, W, Cphys, C, N, Nphys, R, S,
             Ho, Wo, stride, pad_h, pad_w, dil, stream())

    if side is None:
        run()
        return
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    for x, dy, _ in items:
        dy.record_stream(side)
        x.record_stream(side)
    _WGRADS.stream_pending = True


class _WgradScheduler:
    """When a weight gradient is launched, on which stream, and who is told (one instance: _WGRADS).
    How many problems of a geometry one backward pass produces is learnt from the previous pass of the same kind: a geometry that
    came ONCE is launched at once from then on (nothing to group with -- and the last layers of backward, the stem, would otherwise
    leave as an exposed tail behind the end of the dgrad chain), a repeated one leaves as soon as its expected count is complete.
    Passes are told apart by the geometry of their first weight gradient (the head's convolution: input shape, batch, dtype and
    class count are in it), so two models / two input shapes alternating in one process each keep their own expectation instead of
    flushing late or early on the other one's counts.  (Grouping is a speed matter only: every flush is a correct launch.)"""

    def __init__(self):
        self.queues = {}            # launch geometry -> [(x, dy, sink, weight)], in first-queued order
        # Activations (x, dy) the queues keep alive beyond the point where an immediate launch would have released them, and their
        # cap.  MRFP_WGRAD_GROUP_GB fixes it; by default it is a quarter of the device memory that is free when the first gradient
        # is queued, at most 24 GB (the bench step on a 288 GB part: 24; a large-activation configuration -- configs[4] -- on a
        # fuller device gets less and flushes earlier instead of raising the peak).
        self.pending_bytes = 0
        self.max_bytes = int(float(_os.environ["MRFP_WGRAD_GROUP_GB"]) * (1 << 30)) if "MRFP_WGRAD_GROUP_GB" in _os.environ else None
        self.group_max = None       # problems per launch: min(mrfp_conv_wgrad_group_max(), MRFP_WGRAD_GROUP_MAX), taken at the first submit
        self.expect_all = {}        # pass key -> {launch geometry -> problems} of the last complete pass that started with it (64 kinds)
        self._reset_pass()
        self.callback_queued = False    # end_of_backward is queued on the autograd engine for the running pass
        self.streams = {}           # device index -> side stream
        self.stream_pending = False     # a side stream holds launches that the current stream has not waited for

    def _reset_pass(self, key=None):
        """The running pass: its key (the geometry of its first weight gradient; None: no pass is running), the problems seen per
        geometry so far, and those the last complete pass of this kind produced."""
        self.pass_key, self.seen, self.expect = key, {}, dict(self.expect_all.get(key, ()))

    def stream(self, device):
        """The side stream weight gradients are computed on (None when disabled or while a hipGraph is being captured)."""
        if not USE_WGRAD_STREAM[0] or device.type != "cuda" or torch.cuda.is_current_stream_capturing():
            return None
        key = device.index if device.index is not None else torch.cuda.current_device()
        st = self.streams.get(key)
        if st is None:
            st = self.streams[key] = torch.cuda.Stream(device=device)
        return st

    def ensure_callback(self):
        """From inside a backward node: when this backward pass ends, every queue is flushed, then the caller's stream waits for
        the side stream."""
        if not self.callback_queued:
            self.callback_queued = True
            torch.autograd.Variable._execution_engine.queue_callback(self.end_of_backward)

    def submit(self, sig, x, dy, sink, weight):
        """Queues one weight gradient (from inside a backward node); launches what the rules above say is due."""
        if self.group_max is None:
            self.group_max = min(int(_lib.lib().mrfp_conv_wgrad_group_max()), int(_os.environ.get("MRFP_WGRAD_GROUP_MAX", "32")))
        self.ensure_callback()
        if self.pass_key is None:     # first weight gradient of this pass: pick up the expectation of the passes that started like it
            self._reset_pass(sig)
        if self.max_bytes is None:
            free, _total = torch.cuda.mem_get_info(x.device)
            self.max_bytes = min(24 << 30, max(1 << 30, free // 4))
        seen = self.seen[sig] = self.seen.get(sig, 0) + 1
        expect = self.expect.get(sig, 0)
        if expect == 1 and seen == 1 and sig not in self.queues:
            self.issue(sig, [(x, dy, sink, weight)])       # a geometry of its own: nothing to wait for
            return
        q = self.queues.setdefault(sig, [])
        q.append((x, dy, sink, weight))
        GRAD_DEFERRED.add(id(weight))
        self.pending_bytes += x.numel() * x.element_size() + dy.numel() * dy.element_size()
        if len(q) >= self.group_max or (expect > 1 and seen % expect == 0):
            self.flush(sig)
        elif self.pending_bytes > self.max_bytes:
            self.flush()

    def flush(self, sig=None):
        """Issues the queued weight gradients (of one launch geometry, or all of them in first-queued order)."""
        for k in [sig] if sig is not None else list(self.queues):
            items = self.queues.pop(k, None)
            if items:
                self.pending_bytes -= sum(x.numel() * x.element_size() + dy.numel() * dy.element_size() for x, dy, _, _ in items)
                self.issue(k, items)

    def issue(self, sig, items):
        """One launch for `items` (same geometry) on the side stream (or the current one); their weights are reported written."""
        if not _DEBUG_SKIP_WGRAD:
            _launch_wgrads(sig, [i[:3] for i in items], self.stream(items[0][0].device))
            WGRAD_GROUP_LAUNCHES.append(len(items))
        for _, _, _, weight in items:
            GRAD_DEFERRED.discard(id(weight))
            notify_grad(weight)

    def end_of_backward(self):
        self.callback_queued = False
        self.flush()
        # what this pass produced is what the next pass OF THE SAME KIND is expected to produce
        if self.pass_key is not None:
            if len(self.expect_all) >= 64 and self.pass_key not in self.expect_all:
                self.expect_all.pop(next(iter(self.expect_all)))
            self.expect_all[self.pass_key] = self.seen
        self._reset_pass()
        self.join()

    def drop_stale(self, reason="a forward convolution found the end-of-backward callback of an earlier pass still pending"):
        """The last backward pass died with an exception before the engine ran its callbacks (the harness calls this from the
        `finally` of its forward/backward, conv2d() when it is called OUTSIDE any backward pass with the callback still marked as
        queued).  Its queued weight gradients are forgotten -- their step is lost anyway -- so that the next backward registers its
        own callback; dropping a non-empty queue is reported, never silent."""
        dropped = sum(len(v) for v in self.queues.values())
        self.callback_queued = False
        self.queues.clear()
        self.pending_bytes = 0
        self._reset_pass()
        GRAD_DEFERRED.clear()
        if dropped:
            warnings.warn("mrfp_amd.conv: %d queued weight gradients of a backward pass that did not finish were dropped (%s)"
                          % (dropped, reason), RuntimeWarning, stacklevel=3)

    def join(self, stream=None):
        """Makes `stream` (default: the current one) wait for every weight gradient issued so far."""
        if not self.stream_pending:
            return
        tgt = stream if stream is not None else torch.cuda.current_stream()
        for st in self.streams.values():
            tgt.wait_stream(st)
        if stream is None:
            self.stream_pending = False


_WGRADS = _WgradScheduler()
wgrad_stream, flush_wgrads, join_wgrad_stream = _WGRADS.stream, _WGRADS.flush, _WGRADS.join


def backward_failed():
    """To be called when a backward pass raised (harness.Trainer does, from its `finally`): clears the deferred weight-gradient
    state at once instead of leaving it for the next forward convolution to find."""
    if _WGRADS.callback_queued or _WGRADS.queues:
        _WGRADS.drop_stale("the backward pass raised")


def wgrad_boundary(t):
    """Marks a stage boundary on activation `t` (the input of a ResNet stage / of the head): when backward has produced t's
    gradient, everything behind it has queued its weight gradients, and the queues are issued -- the stage's gradient buckets
    complete there (harness.GradSync launches buckets in index order, so later arrival is tolerated) instead of at the very end
    of backward.  Returns t."""
    if GROUP_WGRAD[0] and t.requires_grad and torch.is_grad_enabled():
        t.register_hook(_boundary_hook)
    return t


def _boundary_hook(_grad):
    flush_wgrads()
    return None


GATED_SKIP_HITS = [0]       # dgrad launches that applied a residual tail's gate to their addend (tests)
# (the hand-off itself -- the alias's cell, the GATE / LOWRANK tags, ungate / unlowrank -- is skipgrad.py)
# The input gradient of a shared pointwise classifier on a convolution's skip alias (_SharedConv1x1Pair: `final2` of the MRFP+ head on
# the 256-channel half-resolution HRFP map) has rank <= 32 per pixel: dskip = dP . Wf.  Instead of writing it (1.2 GB at the bench
# shape) and reading it back as the dgrad's addend, the pair returns a storage-less stand-in tagged with its two factors and the
# dgrad multiplies them in registers, rounds the product as the written tensor was and adds it (mrfp_conv_fwd_lowrank): same bits.  MRFP_LOWRANK_SKIP=0: the materialised gradient (A/B runs, tests)
LOWRANK_SKIP = [_os.environ.get("MRFP_LOWRANK_SKIP", "1") != "0"]
LOWRANK_SKIP_HITS = [0]     # dgrad launches that took a skip gradient as its two low-rank factors (tests)
_LOWRANK_K = 32             # the K of mrfp_conv_fwd_lowrank: the classifier's padded score planes


def _dgrad_lowrank_ok(dtype, B, H, W, Cphys, Nphys, R, S, Ho, Wo, stride, pad_h, pad_w, dil):
    """whether the dgrad launch of this convolution can take its skip gradient as low-rank factors (the launch plan's answer)"""
    if dtype not in (torch.bfloat16, torch.float16) or stride != 1:
        return False
    return bool(_lib.lib().mrfp_conv_lowrank_ok(_lib._DT[dtype], B, Ho, Wo, Nphys, Cphys, Cphys, R, S, H, W, 1, dil * (R - 1) - pad_h,
                                                dil * (S - 1) - pad_w, dil))


def L_single(B, H, W, Cphys, Ho, Wo, Nphys, esz):
    """both operands of a weight-gradient problem fit one 3.75 GB buffer-descriptor range (a grouped launch needs that)"""
    return max(B * H * W * Cphys, B * Ho * Wo * Nphys) * esz < 0xF0000000


class _Conv2d(torch.autograd.Function):
    """want_skip: also return an alias of x for a skip connection; the gradient arriving on that alias is added by
    the dgrad kernel's epilogue (no separate accumulation pass over the activation); it may arrive behind a GATE or LOWRANK tag, and
    conv2d() hangs the alias's skipgrad.AliasCell (uses, gate_issued, lowrank_issued, lowrank_ok) on the alias and on this node.
    stats: the rows the epilogue writes its output statistics into (sized by conv2d(), which tags the output with them), or None;
    wtab: the pixel multiplicities that weight them (conv2d(stat_resize=))."""

    @staticmethod
    def forward(ctx, x, weight, bias, stride, pad_h, pad_w, dil, Nphys, want_skip, stats, wtab):
        B, Cphys, H, W = x.shape
        N, C, R, S = weight.shape
        Ho, Wo = _out_size(H, R, stride, pad_h, dil), _out_size(W, S, stride, pad_w, dil)
        pk = get_pack(weight, bias, x.dtype, Cphys, Nphys)
        y = empty_cl(B, Nphys, Ho, Wo, x.dtype, x.device)
        _lib.NOTE[0] = (C, N)
        if wtab is not None:
            call("mrfp_conv_fwd_wstats", ptr(x), ptr(pk.wf), ptr(pk.bias), ptr(y), dt(x), B, H, W, Cphys, Nphys, Nphys, R, S,
                 Ho, Wo, stride, pad_h, pad_w, dil, ptr(wtab), ptr(stats), stream())
            WSTATS_HITS[0] += 1
        else:
            call("mrfp_conv_fwd", ptr(x), ptr(pk.wf), ptr(pk.bias), ptr(y), dt(x), B, H, W, Cphys, Nphys, Nphys, R, S,
                 Ho, Wo, stride, pad_h, pad_w, dil, 1, None, ptr(stats), stream())
        ctx.save_for_backward(x, weight, bias)
        ctx.cfg = (stride, pad_h, pad_w, dil, Nphys, Ho, Wo)
        ctx.set_materialize_grads(False)
        if want_skip:
            return y, x.view_as(x)
        return y

    @staticmethod
    def backward(ctx, dy, dskip=None):
        x, weight, bias = ctx.saved_tensors
        cell = getattr(ctx, ALIAS, None)
        if cell is not None:
            # a residual tail sent its UNMASKED incoming gradient to this alias (ops._BatchNormAct.backward), or the shared classifier
            # a stand-in without storage (_SharedConv1x1Pair.backward): only that tagged tensor may arrive here, anything else raises
            cell.redeem(dskip)
        if dy is None:            # only the skip alias was used downstream
            return (unlowrank(ungate(dskip)),) + (None,) * 10
        stride, pad_h, pad_w, dil, Nphys, Ho, Wo = ctx.cfg
        dy = _chk(dy, "dy")
        B, Cphys, H, W = x.shape
        N, C, R, S = weight.shape
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            pk = get_pack(weight, bias, x.dtype, Cphys, Nphys)
            dx = empty_cl(B, Cphys, H, W, x.dtype, x.device)
            gate = None
            lr = LOWRANK.fetch(dskip) if dskip is not None else None
            if lr is not None:
                # the factors go to the dgrad kernel as one more k step; a launch that cannot take them gets the plain gradient
                if (lr.K == _LOWRANK_K and lr.dp.dtype == dy.dtype == x.dtype and dskip.shape == dx.shape
                        and _dgrad_lowrank_ok(x.dtype, B, H, W, Cphys, Nphys, R, S, Ho, Wo, stride, pad_h, pad_w, dil)):
                    dskip = None
                else:
                    dskip, lr = unlowrank(dskip), None
            if dskip is not None:
                g = GATE.fetch(dskip)
                if g is not None:
                    # the skip-connection gradient of a residual tail arrives UNMASKED with that tail's sign mask attached
                    # (ops._BatchNormAct.backward): the dgrad epilogue applies the gate while it adds -- dy * [y > 0] is never
                    # written or re-read.  Anything this launch cannot do that way gets the plain gradient.
                    if mask_possible(x) and gateable(dskip, x):
                        gate = g.mask
                    else:
                        dskip = ungate(dskip)
                dskip = _chk(dskip, "dskip")
                if dskip.dtype != x.dtype:
                    dskip = dskip.to(x.dtype)
            _lib.NOTE[0] = (N, C)
            if lr is not None:
                call("mrfp_conv_fwd_lowrank", ptr(dy), ptr(pk.wd), None, ptr(dx), dt(dy), B, Ho, Wo, Nphys, Cphys, Cphys, R, S, H, W,
                     1, dil * (R - 1) - pad_h, dil * (S - 1) - pad_w, dil, stride, None, None, ptr(lr.dp), ptr(lr.wd), lr.K, stream())
                LOWRANK_SKIP_HITS[0] += 1
            elif gate is not None:
                call("mrfp_conv_fwd_gated", ptr(dy), ptr(pk.wd), None, ptr(dx), dt(dy), B, Ho, Wo, Nphys, Cphys, Cphys, R, S, H, W,
                     1, dil * (R - 1) - pad_h, dil * (S - 1) - pad_w, dil, stride, ptr(dskip), ptr(gate), stream())
                GATED_SKIP_HITS[0] += 1
            else:
                call("mrfp_conv_fwd", ptr(dy), ptr(pk.wd), None, ptr(dx), dt(dy), B, Ho, Wo, Nphys, Cphys, Cphys, R, S, H, W,
                     1, dil * (R - 1) - pad_h, dil * (S - 1) - pad_w, dil, stride, ptr(dskip), None, stream())
        if ctx.needs_input_grad[1]:
            sig = (x.dtype, B, H, W, Cphys, C, N, Nphys, R, S, Ho, Wo, stride, pad_h, pad_w, dil)
            sink = grad_sink(weight)      # the parameter's slot in the flat gradient arena, when the harness owns it
            side = _WGRADS.stream(x.device) if sink is not None else None
            # one of three routes: queue it with the scheduler / launch it now on the side stream / ... on the current stream
            if sink is not None and GROUP_WGRAD[0] and L_single(B, H, W, Cphys, Ho, Wo, Nphys, x.element_size()):
                _WGRADS.submit(sig, x, dy, sink, weight)
            elif side is not None:
                _WGRADS.ensure_callback()
                _launch_wgrads(sig, [(x, dy, sink)], side)
                notify_grad(weight)
            else:
                dw = sink if sink is not None else torch.empty((N, C, R, S), dtype=torch.float32, device=x.device)
                _launch_wgrads(sig, [(x, dy, dw)], None)
                if sink is not None:
                    notify_grad(weight)
                    dw = None
                elif dw.dtype != weight.dtype:
                    dw = dw.to(weight.dtype)
        if bias is not None and ctx.needs_input_grad[2]:
            db = channel_sums(dy, N).to(bias.dtype)
        return (dx, dw, db) + (None,) * 8


class _SharedConv1x1Pair(torch.autograd.Function):
    """(conv1x1(x1, W), conv1x1(x2, W) + b): ONE weight applied to two activations of different resolution.  Used by the
    MRFP+ head, where final2(Upsample(dec1) + OCout_dec) is evaluated as Upsample(final2(dec1)) + final2(OCout_dec) (a 1x1
    convolution commutes with bilinear interpolation), so the 2x upsample runs on the class scores instead of on 256
    channels.  One Function for both uses keeps the shared weight gradient a single sink write + a single ready
    notification (the gradient-arena protocol of _Conv2d assumes one use per weight)."""

    @staticmethod
    def forward(ctx, x1, x2, weight, bias, Nphys):
        N, C, R, S = weight.shape
        if R != 1 or S != 1 or x1.shape[1] != C or x2.shape[1] != C:
            raise _lib.MrfpHipError("shared conv pair: 1x1 weight and unpadded inputs expected")
        pk = get_pack(weight, bias, x1.dtype, C, Nphys)
        ys = []
        for x, b in ((x1, None), (x2, pk.bias)):
            B, _, H, W = x.shape
            y = empty_cl(B, Nphys, H, W, x.dtype, x.device)
            call("mrfp_conv_fwd", ptr(x), ptr(pk.wf), ptr(b), ptr(y), dt(x), B, H, W, C, Nphys, Nphys, 1, 1, H, W, 1, 0, 0, 1, 1,
                 None, None, stream())
            ys.append(y)
        ctx.save_for_backward(x1, x2, weight, bias)
        ctx.Nphys = Nphys
        # x2 is a convolution's skip alias whose dgrad can take this operator's input gradient as its two factors (conv2d marked it):
        # the alias's cell (skipgrad.AliasCell) is read in backward
        cell = alias_cell(x2)
        ctx.x2_alias = cell if cell is not None and cell.lowrank_ok else None
        ctx.set_materialize_grads(False)
        return ys[0], ys[1]

    @staticmethod
    def backward(ctx, dy1, dy2):
        x1, x2, weight, bias = ctx.saved_tensors
        N, C, _, _ = weight.shape
        Nphys = ctx.Nphys
        pk = get_pack(weight, bias, x1.dtype, C, Nphys)
        dxs, dws = [], []
        db = None
        for x, dy, need_dx, cell in ((x1, dy1, ctx.needs_input_grad[0], None), (x2, dy2, ctx.needs_input_grad[1], ctx.x2_alias)):
            if dy is None:
                dxs.append(None)
                continue
            dy = _chk(dy, "dy")
            B, _, H, W = x.shape
            dx = None
            if (need_dx and cell is not None and LOWRANK_SKIP[0] and cell.sole_consumer() and Nphys == _LOWRANK_K and dy.dtype == x.dtype
                    and x.element_size() == 2):
                # this operator is the alias's only consumer: nothing behind dx but the producing convolution's dgrad, which
                # multiplies dy . Wd itself -- dx is a stand-in without storage (an expanded scalar) that carries the factors
                # (never read: torch.empty, not zeros -- no fill launch)
                dx = torch.empty((), dtype=x.dtype, device=x.device).expand(B, C, H, W)
                LOWRANK.attach(dx, dy, pk.wd, Nphys)
                cell.promise_lowrank()  # told to that convolution: anything but this tagged tensor arriving there raises
            elif need_dx:
                dx = empty_cl(B, C, H, W, x.dtype, x.device)
                call("mrfp_conv_fwd", ptr(dy), ptr(pk.wd), None, ptr(dx), dt(dy), B, H, W, Nphys, C, C, 1, 1, H, W, 1, 0, 0, 1, 1,
                     None, None, stream())
            dxs.append(dx)
            if ctx.needs_input_grad[2]:
                dw = torch.empty((N, C, 1, 1), dtype=torch.float32, device=x.device)
                _launch_wgrads((x.dtype, B, H, W, C, C, N, Nphys, 1, 1, H, W, 1, 0, 0, 1), [(x, dy, dw)], None)
                dws.append(dw)
        if bias is not None and ctx.needs_input_grad[3] and dy2 is not None:
            db = channel_sums(_chk(dy2, "dy"), N).to(bias.dtype)
        dw = None
        if dws:
            total = dws[0] if len(dws) == 1 else dws[0].add_(dws[1])
            sink = grad_sink(weight)
            if sink is not None:
                sink.copy_(total)
                notify_grad(weight)
            else:
                dw = total.to(weight.dtype)
        return dxs[0], dxs[1], dw, db, None


def shared_conv1x1_pair(x1, x2, weight, bias, phys_out):
    return _SharedConv1x1Pair.apply(_chk(x1), _chk(x2), weight, bias, int(phys_out))


def pad_input_channels(x: torch.Tensor, dtype) -> torch.Tensor:
    """Network input NCHW fp32 -> NHWC `dtype` with the channel count padded to a 16-byte chunk."""
    if not x.is_cuda:
        raise _lib.MrfpHipError("input must live on the GPU (got %s): the HIP path has no CPU fallback" % x.device)
    B, C, H, W = x.shape
    Cpad = _round_up(C, _epc(dtype))
    xs = x.detach()
    if xs.dtype != torch.float32 or not xs.is_contiguous():
        xs = xs.float().contiguous()
    y = empty_cl(B, Cpad, H, W, dtype, x.device)
    call("mrfp_nchw_to_nhwc_pad", ptr(xs), ptr(y), _lib._DT[dtype], B, C, H, W, Cpad, stream())
    return y


def conv2d(x, weight, bias, stride, padding, dilation, phys_out: Optional[int] = None, want_skip: bool = False,
           groups: int = 1, stat_resize=None):
    """x: [B,Cphys,H,W] channels-last (Cphys >= weight.shape[1], extra channels must be zero);
    returns [B,N,Ho,Wo], or the channel-padded [B,phys_out,Ho,Wo] buffer when phys_out is given.
    want_skip: returns (y, x_skip) -- see _Conv2d.
    A bias-free convolution feeds a normalisation layer: its epilogue also writes the per-channel partial sums of its output, and
    the output is tagged with them (y._mrfp_colstats, a ConvStats) for that layer to take instead of a statistics pass.
    stat_resize: the ops.NearestPlan of a nearest-neighbour resize the output goes through into a training-mode BatchNorm
    (deepv3.MRFPPlus._hrfp).  The epilogue statistics then count every output pixel as often as the resize reads it
    (mrfp_conv_fwd_wstats), and the BatchNorm skips its statistics pass over the resized tensor."""
    st = stride[0] if isinstance(stride, (tuple, list)) else int(stride)
    ph, pw = (padding if isinstance(padding, (tuple, list)) else (int(padding), int(padding)))
    dl = dilation[0] if isinstance(dilation, (tuple, list)) else int(dilation)
    N, C = weight.shape[0], weight.shape[1]
    epc = _epc(x.dtype)
    x = _pad_to_chunk(x)
    if x.shape[1] < C:
        raise _lib.MrfpHipError("conv2d: input has %d channels, weight expects %d" % (x.shape[1], C))
    if groups != 1 or (C == 1 and x.shape[1] > epc):
        # a grouped weight ([N, C/groups, R, S]; depthwise: [C, 1, 3, 3]) would run here as a dense convolution over the first
        # input channels only: refuse it (depthwise 3x3 runs on ops.depthwise_conv2d)
        raise _lib.MrfpHipError("conv2d: weight %s over an input of %d channels (groups=%d) is a grouped convolution; the implicit-GEMM "
                                "path is dense only" % (tuple(weight.shape), x.shape[1], groups))
    Nphys = phys_out if phys_out is not None else _round_up(N, epc)
    B, Cphys, H, W = x.shape
    R, S = weight.shape[2], weight.shape[3]
    Ho, Wo = _out_size(H, R, st, ph, dl), _out_size(W, S, st, pw, dl)
    L = _lib.lib()
    single = bool(L.mrfp_conv_single_launch(B, H * W * Cphys * x.element_size()))
    plan, wtab, stats = stat_resize, None, None
    if plan is not None and WSTATS[0] and FUSE_STATS[0] and single and (plan.Hs, plan.Ws) == (Ho, Wo) and R * S > 1:
        wtab = plan.multiplicity(B)
    if wtab is not None or (bias is None and FUSE_STATS[0] and single):
        lay = (ctypes.c_int64 * 5)()
        rc = L.mrfp_conv_stats_layout(dt(x), B, H, W, Cphys, Nphys, Nphys, R, S, Ho, Wo, st, ph, pw, dl, 1, int(wtab is not None), lay)
        if rc != 0:
            raise _lib.MrfpHipError("mrfp_conv_stats_layout failed (%d): %s" % (rc, L.mrfp_last_error().decode()))
        nblk, rb, rows, first, cnt = lay
        stats = torch.empty(rows * 2 * Nphys, dtype=torch.float32, device=x.device)
    if _WGRADS.callback_queued and not _in_backward():
        _WGRADS.drop_stale()
    out = _Conv2d.apply(x, weight, bias, st, ph, pw, dl, Nphys, want_skip, stats, wtab)
    y, skip = out if want_skip else (out, None)
    if skip is not None:
        # an alias (skipgrad): its gradient goes to this convolution's dgrad epilogue and nowhere else -- which can take it as
        # low-rank factors where the launch plan says so
        AliasCell(skip, y.grad_fn, bool(LOWRANK_SKIP[0] and y.grad_fn is not None and x.requires_grad
                                         and _dgrad_lowrank_ok(x.dtype, B, H, W, Cphys, Nphys, R, S, Ho, Wo, st, ph, pw, dl)))
    if stats is not None and (phys_out is not None or Nphys == N):
        # consumed by ops.batch_norm_act (statistics pass skipped).  final: the rows a BatchNorm finalize should read (compacted for
        # large launches); weighted statistics count the elements of the RESIZED tensor, have no per-image use, and the plan
        # identifies the one consumer they serve.  (The channel slice below returns a new tensor, without the tag.)
        final = stats[first * 2 * Nphys:(first + cnt) * 2 * Nphys]
        if wtab is not None:
            y._mrfp_colstats = ConvStats(final, cnt, B * plan.Ho * plan.Wo, stats, nblk, 0, plan, y._version)
        else:
            y._mrfp_colstats = ConvStats(final, cnt, B * Ho * Wo, stats, nblk, rb, None, y._version)
    if phys_out is None and Nphys != N:
        y = y[:, :N].contiguous(memory_format=CL)
    return (y, skip) if want_skip else y
