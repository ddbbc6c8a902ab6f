"""The skip-gradient hand-off between conv._Conv2d, ops._BatchNormAct and conv._SharedConv1x1Pair ("Skip-gradient
hand-off").  An ALIAS is a tensor whose gradient goes to the backward of one autograd node, its owner, and nowhere else: the skip output
of a convolution (conv.conv2d(want_skip=True)), the output of a plain BatchNorm (ops.batch_norm_act).  Its only consumer may send that
gradient unfinished -- unmasked behind a GATE tag, or as a stand-in without storage behind a LOWRANK tag -- and the owner's kernels
finish it while they read it.  The rules (sole consumer, promise and redeem, tag freshness) are written here once."""
import collections

import torch

from . import _lib
from ._lib import call, dt, ptr, stream

ALIAS = "_mrfp_alias"       # where an AliasCell hangs, on the alias and on its owner (the autograd node IS the ctx of its backward);
                            # hot paths read it in line, getattr(t, ALIAS, None), everything else through alias_cell()
_NO_GATE = ("a gated skip gradient reached its convolution without its gate: the skip alias was also consumed by an operator outside "
            "mrfp_amd.ops (set MRFP_GATED_SKIP=0)")
_NO_GATE_BN = ("a gated gradient reached its BatchNorm without its gate: the layer's output was also consumed by an operator outside "
               "mrfp_amd.ops (set MRFP_GATED_SKIP=0)")
_NO_FACTORS = ("a low-rank skip gradient reached its convolution without its factors: the skip alias was also consumed by an operator "
               "outside mrfp_amd.ops (set MRFP_LOWRANK_SKIP=0)")
Gate = collections.namedtuple("Gate", "mask version")               # one bit per element, NHWC order: the gradient is t * [bit set]
LowRank = collections.namedtuple("LowRank", "dp wd K version")      # the gradient is the pointwise dgrad dp[B,K,H,W] . wd (a dgrad pack)


class _Tag:
    """A payload on a tensor, valid at the tensor `_version` it was attached at."""
    __slots__ = ("attr", "payload", "kind")

    def __init__(self, attr, payload, kind):
        self.attr, self.payload, self.kind = attr, payload, kind

    def attach(self, t, *fields):
        setattr(t, self.attr, self.payload(*fields, t._version))

    def fetch(self, t, promised=None):
        """The payload of t's tag, or None without one (t may be None); a stale tag raises.  promised: the owner was told that only
        a tensor with this tag would arrive (the message to raise): anything else raises that, a stale tag included."""
        p = getattr(t, self.attr, None)
        if p is None and promised is None:
            return None
        if p is None or p.version != t._version:
            raise _lib.MrfpHipError(promised or "a %s skip gradient was modified in place before it reached its consumer" % self.kind)
        return p


GATE = _Tag("_mrfp_gate", Gate, "gated")
LOWRANK = _Tag("_mrfp_lowrank", LowRank, "low-rank")


class AliasCell:
    """The state of one alias, hung on the alias (for its consumers) and on the owning node (for its backward; None: no graph).
    uses: the operators of mrfp_amd.ops that consumed the alias so far (ops._chk); read in backward, when the whole forward has run.
    gate_issued / lowrank_issued: the promises -- the gradient was sent behind a GATE / LOWRANK tag, nothing else may reach the owner.
    lowrank_ok: the owner's dgrad launch can take low-rank factors (conv._dgrad_lowrank_ok)."""
    __slots__ = ("uses", "gate_issued", "lowrank_issued", "lowrank_ok")

    def __init__(self, alias, node, lowrank_ok=False):
        self.uses, self.gate_issued, self.lowrank_issued, self.lowrank_ok = 0, False, False, lowrank_ok
        alias._mrfp_alias = self
        if node is not None:
            node._mrfp_alias = self

    def use(self):
        self.uses += 1

    def sole_consumer(self):
        """With a second consumer autograd sums the gradients into a fresh tensor, which has no tag."""
        return self.uses == 1

    def promise_gate(self):
        self.gate_issued = True

    def promise_lowrank(self):
        self.lowrank_issued = True

    def redeem(self, arrived, bn=False):
        """The owner's backward (bn: a BatchNorm), on the gradient that arrived for the alias.  A promise that something else arrives
        on means a consumer no count saw (a raw torch op on the alias): raise, the sum would be silently wrong."""
        if self.gate_issued:
            GATE.fetch(arrived, _NO_GATE_BN if bn else _NO_GATE)
            self.gate_issued = False
        if self.lowrank_issued:
            LOWRANK.fetch(arrived, _NO_FACTORS)
            self.lowrank_issued = False


def alias_cell(t):
    return getattr(t, ALIAS, None)


def mask_possible(t):
    """A 1-bit mask per element of t: 16-bit storage, whole mask bytes per pixel."""
    return t.element_size() == 2 and t.shape[1] % 8 == 0


def gateable(t, like):
    """t can be gated in flight by a kernel that walks `like`."""
    return t.dtype == like.dtype and t.shape == like.shape and t.is_contiguous(memory_format=torch.channels_last)


def ungate(t):
    """The plain gradient for a tensor that carries a GATE tag: t * [mask bit set].  Tensors without the tag (and None) pass through."""
    g = GATE.fetch(t)
    if g is None:
        return t
    B, C, H, W = t.shape
    out = torch.empty((B, C, H, W), dtype=t.dtype, device=t.device, memory_format=torch.channels_last)
    call("mrfp_affine_bwd_mask", ptr(t), None, ptr(g.mask), ptr(out), None, dt(t), B, H, W, C, None, None, None, 0, stream())
    return out


def unlowrank(t):
    """The plain gradient for a tensor that carries a LOWRANK tag: the pointwise dgrad launch dp . wd the tag stands for.  Tensors
    without the tag (and None) pass through."""
    lr = LOWRANK.fetch(t)
    if lr is None:
        return t
    B, C, H, W = t.shape
    out = torch.empty((B, C, H, W), dtype=lr.dp.dtype, device=lr.dp.device, memory_format=torch.channels_last)
    call("mrfp_conv_fwd", ptr(lr.dp), ptr(lr.wd), None, ptr(out), dt(lr.dp), B, H, W, lr.K, C, C, 1, 1, H, W, 1, 0, 0, 1, 1, None, None,
         stream())
    return out
