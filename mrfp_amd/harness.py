"""Train-step and eval harness: the semantics of the reference's driver loops (reference
main.py:822-839 optimiser + poly LR, 857-864 train step, 887-913 eval loop) re-designed for one
process per MI355X:

  * all trainable parameters, their gradients and the momentum live in three flat fp32 arenas
    (parameters keep their names / shapes / state_dict ABI as views), so the optimiser is ONE fused
    HIP kernel and the data-parallel exchange works on contiguous buckets without packing copies;
  * gradient buckets (contiguous arena ranges, filled in reverse forward order) are all-reduced by
    RCCL over xGMI on a side HIP stream as soon as autograd has finished the last tensor of a bucket,
    overlapping the exchange with the rest of backward; no other collective exists on the data path;
  * BatchNorm / NP+ statistics stay per replica: with 16 images per GPU that is exactly the
    statistical population the reference's single-GPU run sees.
"""
from __future__ import annotations

import contextlib
import math
import os
import random
from typing import List, Optional

import numpy as np
import torch
import torch.distributed as dist

from . import _lib
from ._lib import call, ptr, stream


def poly_lr_factor(it: int, max_iter: int = 40000, power: float = 0.9) -> float:
    """reference main.py:832-839 (LRPolicy)."""
    return math.pow(1 - it / max_iter, power)


class LossScaler:
    """The loss scale of a half-precision run as DEVICE state: torch.amp.GradScaler's rule (scale *= backoff_factor after a step
    whose gradient held an inf / NaN, scale *= growth_factor after growth_interval clean steps in a row) applied by
    mrfp_grad_check's finalize kernel, so no step waits for the host.  dynamic=False keeps the scale fixed and still skips a step
    with a non-finite gradient.  The state is the eight 32-bit words of include/mrfp_hip.h (scale, growth_tracker, found_inf,
    grad_norm, gmul, taken, skipped, reserved); `scale_tensor` is the 0-dim fp32 view of word 0 that backward is seeded with.
    Build-defined: the reference trains in fp32."""

    FIELDS = ("scale", "growth_tracker", "found_inf", "grad_norm", "gmul", "taken", "skipped")
    _FLOAT = (0, 3, 4)            # words that hold a float

    def __init__(self, init_scale=65536.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000, dynamic=True,
                 device=None):
        init_scale, growth_factor, backoff_factor = float(init_scale), float(growth_factor), float(backoff_factor)
        if not (init_scale > 0.0) or math.isinf(init_scale):
            raise ValueError("init_scale must be positive and finite, got %r" % (init_scale,))
        if not (growth_factor > 1.0) or math.isinf(growth_factor):
            raise ValueError("growth_factor must be > 1, got %r" % (growth_factor,))
        if not (0.0 < backoff_factor < 1.0):
            raise ValueError("backoff_factor must be in (0, 1), got %r" % (backoff_factor,))
        if int(growth_interval) != growth_interval or int(growth_interval) < 1:
            raise ValueError("growth_interval must be an integer >= 1, got %r" % (growth_interval,))
        self.growth_factor, self.backoff_factor = growth_factor, backoff_factor
        self.growth_interval, self.dynamic = int(growth_interval), bool(dynamic)
        if device is None:
            device = "cuda" if torch.cuda.is_available() else "cpu"      # (on the CPU: state_dict / info only)
        self._set_state(torch.device(device), init_scale, 0)

    def _set_state(self, device, scale, tracker, taken=0, skipped=0):
        words = torch.zeros(8, dtype=torch.int32)
        words.view(torch.float32)[0] = scale
        words[1], words[5], words[6] = int(tracker), int(taken), int(skipped)
        self.state = words.to(device)
        self.scale_tensor = self.state.view(torch.float32)[0]            # 0-dim view: the CE backward kernels read this address

    def to(self, device):
        if self.state.device != torch.device(device):
            i = self.info()
            self._set_state(torch.device(device), i["scale"], i["growth_tracker"], i["taken"], i["skipped"])
        return self

    def info(self):
        """The seven fields of the device state as python numbers.  This is the one host wait of the feature, and it happens only
        when somebody asks."""
        w = self.state.cpu()
        f = w.view(torch.float32)
        return {k: (float(f[i]) if i in self._FLOAT else int(w[i])) for i, k in enumerate(self.FIELDS)}

    # the key layout of torch.amp.GradScaler.state_dict(): either side loads the other's dict
    def state_dict(self):
        i = self.info()
        return {"scale": i["scale"], "growth_factor": self.growth_factor, "backoff_factor": self.backoff_factor,
                "growth_interval": self.growth_interval, "_growth_tracker": i["growth_tracker"]}

    def load_state_dict(self, sd):
        new = LossScaler(sd["scale"], sd["growth_factor"], sd["backoff_factor"], sd["growth_interval"], self.dynamic, "cpu")
        tracker = int(sd["_growth_tracker"])
        if tracker < 0:
            raise ValueError("_growth_tracker must be >= 0, got %r" % (tracker,))
        self.growth_factor, self.backoff_factor, self.growth_interval = new.growth_factor, new.backoff_factor, new.growth_interval
        i = self.info()
        words = new.state.clone()
        words[1], words[5], words[6] = tracker, i["taken"], i["skipped"]
        self.state.copy_(words)                  # in place: captured graphs and scale_tensor keep pointing at this block


def _check_max_grad_norm(max_grad_norm):
    if max_grad_norm is None:
        return None
    max_grad_norm = float(max_grad_norm)
    if not (max_grad_norm > 0.0):
        raise ValueError("max_grad_norm must be > 0, got %r" % (max_grad_norm,))
    return max_grad_norm


def _check_accum_steps(accum_steps):
    if isinstance(accum_steps, bool) or not isinstance(accum_steps, int) or accum_steps < 1:
        raise ValueError("accum_steps must be an int >= 1, got %r" % (accum_steps,))
    return accum_steps


def _check_loss_weights(loss_weights):
    if loss_weights is None:
        return None
    if not isinstance(loss_weights, (list, tuple)) or len(loss_weights) == 0:
        raise ValueError("loss_weights must be None or a non-empty sequence of finite numbers, got %r" % (loss_weights,))
    for w in loss_weights:
        if isinstance(w, bool) or not isinstance(w, (int, float)) or not math.isfinite(w):
            raise ValueError("loss_weights must be None or a non-empty sequence of finite numbers, got %r" % (loss_weights,))
    return tuple(float(w) for w in loss_weights)


# ------------------------------------------------------------------------------------------
# weight averaging (EMA / SWA) inside the fused step: the rule of include/mrfp_hip.h, once more in Python
# ------------------------------------------------------------------------------------------
AVERAGE_KINDS = {"ema": 0, "swa": 1}          # the `kind` argument of mrfp_sgd_step_avg / mrfp_sgd_step_checked_avg


def _f32(v: float) -> float:
    return float(torch.tensor(v, dtype=torch.float64).to(torch.float32))


def average_coefficient(kind, n, decay=0.999, warmup=True) -> float:
    """The coefficient c of the averaging update with index n >= 1, e = e + c * (p - e): formed in double, rounded through float32
    once -- the value average_rule() in csrc/sgd.hip hands its loop.  swa: 1 / (n + 1), the running arithmetic mean.  ema:
    1 - min(decay, (1 + n) / (10 + n)) with warm-up, 1 - decay without."""
    if kind not in AVERAGE_KINDS:
        raise ValueError("kind must be 'ema' or 'swa', got %r" % (kind,))
    n = int(n)
    if n < 1:
        raise ValueError("the update with index 0 is a copy and has no coefficient; n must be >= 1, got %r" % (n,))
    if kind == "swa":
        c = 1.0 / (float(n) + 1.0)
    else:
        d = float(decay)
        if warmup:
            d = min(d, (1.0 + float(n)) / (10.0 + float(n)))
        c = 1.0 - d
    return _f32(c)


def average_index(t, start=1, every=1):
    """The index n of the averaging update after applied step t (1-based), None when step t makes none: an update happens iff
    t >= start and (t - start) % every == 0, and then n = (t - start) // every."""
    if t < start or (t - start) % every != 0:
        return None
    return (t - start) // every


def averages_made(t, start=1, every=1) -> int:
    """How many averaging updates the applied steps 1 .. t have made."""
    return 0 if t < start else (t - start) // every + 1


class WeightAverage:
    """A validated, plain description of an averaged copy of the weights, kept by the fused step:
      kind    "ema": exponential moving average, e += (1 - d) * (p - e) with d = decay, or min(decay, (1 + n) / (10 + n)) while
              `warmup` (the early average follows the run instead of its initial weights);  "swa": the equal-weight mean of the
              parameters after the updating steps (SWA / SWAD), `decay` and `warmup` unused.
      start   the first applied optimiser step (1-based) that enters the average: a bit copy of the parameters.
      every   an update every that many applied steps from `start` on.
    ValueError on what the C side refuses: an unknown kind, decay outside (0, 1), start < 1, every < 1."""

    def __init__(self, kind="ema", decay=0.999, warmup=True, start=1, every=1):
        if not isinstance(kind, str) or kind not in AVERAGE_KINDS:
            raise ValueError("kind must be 'ema' or 'swa', got %r" % (kind,))
        if isinstance(decay, bool) or not isinstance(decay, (int, float)) or not (0.0 < float(decay) < 1.0):
            raise ValueError("decay must be a number in (0, 1), got %r" % (decay,))
        for name, v in (("start", start), ("every", every)):
            if isinstance(v, bool) or not isinstance(v, int) or not (1 <= v < 2 ** 31):
                raise ValueError("%s must be an int >= 1, got %r" % (name, v))
        self.kind, self.decay, self.warmup, self.start, self.every = kind, float(decay), bool(warmup), start, every

    def config(self):
        return {"kind": self.kind, "decay": self.decay, "warmup": self.warmup, "start": self.start, "every": self.every}

    def c_args(self):
        """(kind, decay, warmup, start, every) as the entry points take them."""
        return AVERAGE_KINDS[self.kind], self.decay, int(self.warmup), self.start, self.every

    def __repr__(self):
        return "WeightAverage(kind=%r, decay=%r, warmup=%r, start=%r, every=%r)" % (
            self.kind, self.decay, self.warmup, self.start, self.every)


def _check_average(average):
    if average is None or isinstance(average, WeightAverage):
        return average
    if isinstance(average, str):
        return WeightAverage(kind=average)           # ValueError on an unknown name
    raise ValueError("average must be None, 'ema', 'swa' or a WeightAverage, got %r" % (average,))


class FlatArena:
    """Trainable parameters and their gradients as views into two flat fp32 buffers (every tensor starts
    16-byte aligned).  Device-agnostic host logic: the data-parallel buckets are ranges of `flat_g`.
    `flat_a`, the sum of a gradient-accumulation window, exists from the first accumulate() on (None until then)."""

    def __init__(self, model: torch.nn.Module):
        every = list(model.parameters())
        self.params = [p for p in every if p.requires_grad]
        if not self.params:
            raise ValueError("no trainable parameters")
        # the reference hands model.parameters() -- frozen HRFP tensors included -- to torch.optim.SGD (main.py:826), so
        # its optimizer.state_dict() numbers parameters by their position in THAT list
        self.n_all = len(every)
        self.all_index = [i for i, p in enumerate(every) if p.requires_grad]
        dev = self.params[0].device
        self.offsets, n = [], 0
        for p in self.params:
            self.offsets.append(n)
            n += (p.numel() + 3) // 4 * 4
        self.n = n
        self.flat_p = torch.zeros(n, dtype=torch.float32, device=dev)
        self.flat_g = torch.zeros(n, dtype=torch.float32, device=dev)
        self.flat_a = None
        for p, o in zip(self.params, self.offsets):
            self.flat_p[o:o + p.numel()].copy_(p.data.reshape(-1))
            p.data = self.flat_p[o:o + p.numel()].view(p.shape)
            p.grad = self.flat_g[o:o + p.numel()].view(p.shape)
            p._mrfp_direct = True          # backward kernels may write this gradient slot directly (ops.grad_sink)

    def zero_grad(self):
        self.flat_g.zero_()
        for p, o in zip(self.params, self.offsets):   # keep .grad pointing into the arena
            if p.grad is None or p.grad.data_ptr() != self.flat_g.data_ptr() + 4 * o:
                p.grad = self.flat_g[o:o + p.numel()].view(p.shape)

    def accumulate(self, lo=0, hi=None, first=False, into_grad=False):
        """mrfp_grad_accumulate over the arena range [lo, hi) on the current stream: flat_a = flat_g (first) | flat_a += flat_g, or,
        with into_grad, flat_g += flat_a -- the same entry point with the arenas in the other roles (a + b is commutative bit for
        bit), which closes a window with the sum where the optimiser and the all-reduce read it.  lo and hi are arena offsets of
        tensors (multiples of 4: 16-byte aligned).  CPU arenas (the gloo tests of the bucket logic) take the plain torch add."""
        hi = self.n if hi is None else hi
        if self.flat_a is None:
            self.flat_a = torch.empty_like(self.flat_g)
        acc, g = (self.flat_g, self.flat_a) if into_grad else (self.flat_a, self.flat_g)
        if not acc.is_cuda:
            if first:
                acc[lo:hi].copy_(g[lo:hi])
            else:
                acc[lo:hi].add_(g[lo:hi])
            return
        call("mrfp_grad_accumulate", ptr(acc) + 4 * lo, ptr(g) + 4 * lo, hi - lo, int(first), stream())


class FlatSGD(FlatArena):
    """torch.optim.SGD(lr, momentum=0.9, weight_decay=5e-4) + LambdaLR(poly 0.9) as ONE fused HIP kernel
    over the flat arenas (reference main.py:826-839, 863-864).
    average: None | WeightAverage | "ema" | "swa".  With one, `flat_e` -- a fourth arena, zeroed here, because in the checked path
    the host does not know when the first update lands -- holds the averaged weights and every step goes through
    mrfp_sgd_step_avg / mrfp_sgd_step_checked_avg; without one flat_e is None and the step is the plain one."""

    def __init__(self, model: torch.nn.Module, lr=1e-2, momentum=0.9, weight_decay=5e-4, max_iter=40000, power=0.9,
                 average=None):
        average = _check_average(average)
        super().__init__(model)
        self.flat_m = torch.zeros_like(self.flat_p)
        self.average = average
        self.flat_e = torch.zeros_like(self.flat_p) if average is not None else None
        # applied steps the scaler's `taken` word has not counted (unchecked steps, steps before a resume): the averaging rule's
        # t is taken + taken_base, formed on the device in the checked path
        self.taken_base = 0
        self.base_lr, self.momentum, self.weight_decay = lr, momentum, weight_decay
        self.max_iter, self.power = max_iter, power
        self.it = 0
        self.has_momentum = False        # torch.optim.SGD: the first step copies the gradient into the momentum buffer
        self._scaler = None              # the LossScaler of the checked steps so far: its `taken` count says whether one was applied
        self._check_ws = None

    @property
    def lr(self):
        return self.base_lr * poly_lr_factor(self.it, self.max_iter, self.power)

    # ---- checkpoint ABI: the layout of torch.optim.SGD.state_dict() (reference main.py:867 stores it as 'optimizer') ----
    def state_dict(self):
        """torch.optim.SGD.state_dict() of the reference's optimizer after the same number of steps: one param group
        over ALL model parameters (frozen ones have no state entry), per-parameter `momentum_buffer` cut from the
        momentum arena, `lr` = current scheduled rate, `initial_lr` = base rate (LambdaLR adds it).  The extra key
        `mrfp_iteration` carries the scheduler position, which the reference does not save (its resume restarts the
        poly schedule); loading a plain torch state dict recovers it from lr / initial_lr."""
        state = {}
        if not self.has_momentum and self._scaler is not None:       # checked steps decide on the device: ask (a host copy, like the rest)
            self.has_momentum = self._scaler.info()["taken"] > 0
        if self.has_momentum:
            for i, p, o in zip(self.all_index, self.params, self.offsets):
                state[i] = {"momentum_buffer": self.flat_m[o:o + p.numel()].view(p.shape).detach().clone().cpu()}
        group = {"lr": self.lr, "momentum": self.momentum, "dampening": 0, "weight_decay": self.weight_decay,
                 "nesterov": False, "maximize": False, "foreach": None, "differentiable": False, "fused": None,
                 "initial_lr": self.base_lr, "params": list(range(self.n_all))}
        return {"state": state, "param_groups": [group], "mrfp_iteration": self.it}

    def load_state_dict(self, sd):
        group = sd["param_groups"][0]
        self.momentum, self.weight_decay = float(group["momentum"]), float(group["weight_decay"])
        self.base_lr = float(group.get("initial_lr", group["lr"]))
        if "mrfp_iteration" in sd:
            self.it = int(sd["mrfp_iteration"])
        else:                                   # a checkpoint written by torch.optim.SGD + LambdaLR: invert the poly factor
            f = float(group["lr"]) / self.base_lr if self.base_lr > 0 else 1.0
            self.it = int(round(self.max_iter * (1.0 - min(max(f, 0.0), 1.0) ** (1.0 / self.power))))
        state = sd.get("state", {})
        # torch numbers the saved parameters 0..P-1 in param_groups[0]["params"] order = model.parameters() order
        slot = {j: t for t, j in enumerate(self.all_index)}          # position in model.parameters() -> arena slot
        self.flat_m.zero_()
        n = 0
        for key, st in state.items():
            t = slot.get(group["params"].index(int(key)) if int(key) in group["params"] else -1)
            buf = st.get("momentum_buffer")
            if t is None or buf is None:
                continue
            p, o = self.params[t], self.offsets[t]
            if buf.numel() != p.numel():
                raise _lib.MrfpHipError("optimizer state %s: momentum_buffer has %d values, the parameter %d"
                                        % (key, buf.numel(), p.numel()))
            self.flat_m[o:o + p.numel()].copy_(buf.reshape(-1).to(self.flat_m.device, torch.float32))
            n += 1
        # torch.optim.SGD keeps no state for a parameter that never received a gradient: its momentum stays zero here
        # (what torch's first step on it would start from, up to the dampening-free first-step copy)
        self.missing_state = len(self.params) - n if n else 0
        self.has_momentum = n > 0

    def applied_steps(self, scaler: Optional[LossScaler] = None) -> int:
        """t of the averaging rule: optimiser steps applied so far.  Unchecked steps are counted here on the host; checked ones by
        the `taken` word of the scaler (the one given, else that of the checked steps so far) on the device, so with a scaler
        this is one device -> host copy."""
        scaler = scaler if scaler is not None else self._scaler
        return self.taken_base + (scaler.info()["taken"] if scaler is not None else 0)

    def step(self, gscale: float = 1.0, scaler: Optional[LossScaler] = None, max_grad_norm: Optional[float] = None):
        """One optimiser step + scheduler step.  Without `scaler`: mrfp_sgd_step with the host-side factor `gscale`.
        With a LossScaler: mrfp_grad_check (partial sums, finalize) and mrfp_sgd_step_checked on the current stream -- the device
        decides whether the step is applied (no inf / NaN in the arena), by which factor (gscale / scale, times the
        clip_grad_norm_ coefficient of `max_grad_norm`), and what the next loss scale is; nothing waits for the host.  The
        schedule position `it` advances on a skipped step too, as the reference's unconditional scheduler.step() does
        (main.py:864)."""
        if self.flat_p.device.type != "cuda":
            raise _lib.MrfpHipError("FlatSGD.step needs the arenas on the GPU: the HIP path has no CPU fallback")
        max_grad_norm = _check_max_grad_norm(max_grad_norm)
        if scaler is None:
            if max_grad_norm is not None:
                raise ValueError("max_grad_norm needs a LossScaler (LossScaler(init_scale=1.0, dynamic=False) for a plain run)")
            # (after a checked step the momentum arena obeys "zero where no momentum exists": mu*0 + g' is the first-step copy)
            first = not self.has_momentum and self._scaler is None
            if self.average is None:
                call("mrfp_sgd_step", ptr(self.flat_p), ptr(self.flat_g), ptr(self.flat_m), self.n, float(self.lr),
                     float(self.momentum), float(self.weight_decay), float(gscale), int(first), stream())
            else:
                self.taken_base += 1                 # an unchecked step is always applied
                call("mrfp_sgd_step_avg", ptr(self.flat_p), ptr(self.flat_g), ptr(self.flat_m), ptr(self.flat_e), self.n,
                     float(self.lr), float(self.momentum), float(self.weight_decay), float(gscale), int(first),
                     *self.average.c_args(), self.applied_steps(), stream())
            self.has_momentum = True
        else:
            if scaler.state.device != self.flat_p.device:
                raise _lib.MrfpHipError("LossScaler state on %s, arenas on %s: scaler.to(device) first"
                                        % (scaler.state.device, self.flat_p.device))
            if self._check_ws is None:
                nblk = int(_lib.lib().mrfp_grad_check_nblocks(self.n))
                self._check_ws = torch.empty(4 * nblk, dtype=torch.float32, device=self.flat_p.device)
            call("mrfp_grad_check", ptr(self.flat_g), self.n, float(gscale), ptr(self._check_ws), ptr(scaler.state),
                 int(scaler.dynamic), scaler.growth_factor, scaler.backoff_factor, scaler.growth_interval,
                 math.inf if max_grad_norm is None else max_grad_norm, stream())
            if self.average is None:
                call("mrfp_sgd_step_checked", ptr(self.flat_p), ptr(self.flat_g), ptr(self.flat_m), self.n, float(self.lr),
                     float(self.momentum), float(self.weight_decay), ptr(scaler.state), stream())
            else:
                call("mrfp_sgd_step_checked_avg", ptr(self.flat_p), ptr(self.flat_g), ptr(self.flat_m), ptr(self.flat_e), self.n,
                     float(self.lr), float(self.momentum), float(self.weight_decay), ptr(scaler.state), self.taken_base,
                     *self.average.c_args(), stream())
            self._scaler = scaler
        # the fused kernel wrote the arena behind autograd's version counters: invalidate the derived
        # weight packs explicitly (mrfp_amd/conv.py rebuilds them on next use)
        from . import conv
        conv.invalidate_packs()
        conv.repack_all()                             # one launch for every bias-free trainable pack
        self.it += 1                                  # scheduler.step()


class GradSync:
    """Bucketed RCCL all-reduce of the flat gradient arena, overlapped with backward."""

    def __init__(self, opt: FlatArena, bucket_mb: float = 32.0, group=None):
        self.opt, self.group = opt, group
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        # MRFP_FORCE_SYNC=1: run the bucket / side-stream / collective machinery even with one rank (rehearsal of the
        # multi-GPU path on a single-GPU box)
        self.enabled = self.world > 1 or (dist.is_initialized() and os.environ.get("MRFP_FORCE_SYNC") == "1")
        self.buckets: List[tuple] = []
        if not self.enabled:
            return
        cap = int(bucket_mb * (1 << 20) / 4)
        # buckets are contiguous arena ranges, cut from the END (gradients arrive in reverse forward order)
        end = opt.n
        members: List[int] = []
        self.bucket_of = [0] * len(opt.params)
        for i in range(len(opt.params) - 1, -1, -1):
            members.append(i)
            if end - opt.offsets[i] >= cap or i == 0:
                self.buckets.append((opt.offsets[i], end, list(members)))
                end, members = opt.offsets[i], []
        for b, (_, _, mem) in enumerate(self.buckets):
            for i in mem:
                self.bucket_of[i] = b
        self.pending = [0] * len(self.buckets)
        self.seen = [False] * len(opt.params)
        self.next = 0                    # buckets are launched strictly in index order on every rank
        self.works = []
        self.reduce, self.accum = True, False        # this pass: exchange the buckets? add the window's flat_a to each one first?
        self.on_gpu = opt.flat_g.is_cuda
        self.side = torch.cuda.Stream() if self.on_gpu else None
        self._index = {id(p): i for i, p in enumerate(opt.params)}
        from . import ops
        for i, p in enumerate(opt.params):
            p.register_post_accumulate_grad_hook(self._make_autograd_hook(i, ops.GRAD_DEFERRED))
        ops.GRAD_NOTIFY[0] = self._notify     # gradients written straight into the arena by the HIP backward kernels

    def _notify(self, param):
        i = self._index.get(id(param))
        if i is not None:
            self._make_hook(i)(param)

    def _make_autograd_hook(self, i, deferred):
        """autograd's post-accumulate hook: fires when the parameter's backward node has RUN -- also when that node returned None
        because its kernel writes the arena directly, and also when it only QUEUED the weight-gradient launch (conv._WGRADS.submit:
        grouped, deferred weight gradients).  A queued gradient has not been written: it is reported by ops.notify_grad when its
        launch has been issued, and ignored here."""
        inner = self._make_hook(i)

        def hook(param):
            if id(param) in deferred:
                return
            inner(param)
        return hook

    def _make_hook(self, i):
        def hook(_param):
            # A parameter can be reported twice in one step: by the HIP backward kernel that wrote its gradient
            # straight into the arena (ops.notify_grad) and by autograd's post-accumulate hook (this PyTorch fires
            # it even when the backward returned None for the parameter).  Count each parameter once.
            if not self.reduce or self.seen[i]:     # (an inner micro-batch of an accumulation window launches nothing)
                return
            self.seen[i] = True
            self.pending[self.bucket_of[i]] -= 1
            self._launch_ready()
        return hook

    def _launch_ready(self):
        """Collectives must be issued in the same order on every rank, whatever order the gradients arrive in (ranks
        may draw different perturbation toggles, a tensor may get no gradient on one rank): a bucket is launched only
        when every bucket before it has been launched -- bucket 0 holds the LAST parameters, whose gradients arrive
        first, so in the common case this is still "as soon as the bucket is complete"."""
        while self.next < len(self.buckets) and self.pending[self.next] == 0:
            self._launch(self.next)
            self.next += 1

    def _launch(self, b):
        lo, hi, _ = self.buckets[b]
        if not self.on_gpu:                      # gloo / CPU arenas (tests): no streams involved
            if self.accum:
                self.opt.accumulate(lo, hi, into_grad=True)
            self.works.append(dist.all_reduce(self.opt.flat_g[lo:hi], group=self.group, async_op=True))
            return
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream())
        from . import conv
        with torch.cuda.stream(self.side):
            self.side.wait_event(ev)
            conv.join_wgrad_stream(self.side)        # the bucket's weight gradients are written on the wgrad stream
            if self.accum:                           # last micro-batch of a window: the range's sum over the earlier ones, behind
                self.opt.accumulate(lo, hi, into_grad=True)      # both waits and in front of the collective, on the side stream
            self.works.append(dist.all_reduce(self.opt.flat_g[lo:hi], group=self.group, async_op=True))

    def begin(self, reduce=True, accum=False):
        """reduce=False: a pass whose gradient only joins an accumulation window -- the hooks launch nothing and finish() only joins
        the weight-gradient stream.  accum=True (the window's last pass): each bucket's range of flat_g gets += flat_a before its
        all-reduce, so one collective per bucket carries the whole window."""
        if self.enabled:
            self.reduce, self.accum = bool(reduce), bool(accum)
            self.pending = [len(m) for _, _, m in self.buckets]
            self.seen = [False] * len(self.opt.params)
            self.next = 0
            self.works = []

    def finish(self):
        """Blocks the compute stream until every bucket has been reduced; returns the 1/world scale."""
        from . import conv
        conv.flush_wgrads()                          # (queued grouped weight gradients: backward's end callback has issued them already)
        conv.join_wgrad_stream()                     # weight gradients are computed on a second stream (mrfp_amd/conv.py)
        if not self.enabled:
            return 1.0
        if not self.reduce:
            return 1.0 / self.world
        for b in range(self.next, len(self.buckets)):   # buckets with tensors that got no gradient this step: same order
            self.pending[b] = 0
        self._launch_ready()
        for w in self.works:
            w.wait()
        if self.on_gpu:
            torch.cuda.current_stream().wait_stream(self.side)
        return 1.0 / self.world


def sync_replicas(model, arena: Optional[FlatArena] = None, group=None, src: int = 0):
    """What DistributedDataParallel does at construction: every rank starts from rank `src`'s parameters and buffers
    (MRFPPlus.__init__ draws its initial weights from the unseeded global RNG, and a missing pretrained checkpoint keeps
    them: without this, replicas would differ for ever because only gradients are averaged).  Also makes the three
    perturbation toggles of MRFPPlus.forward agree across ranks for the whole run: the reference seeds python's
    `random` identically everywhere (main.py:38); here rank `src` draws one seed and every rank gets a private
    `random.Random(seed)` for the toggles -- no per-step collective, no host synchronisation.
    The perturbation DRAWS, by contrast, differ per rank (reference deepv3.py:272-275, 291-306: NP+
    normals and the HRFP re-initialisation come from the torch generators): every torch generator of this process is
    seeded `base + rank` with one base broadcast from `src`, so N replicas apply N different perturbations."""
    if arena is not None:
        dist.broadcast(arena.flat_p, src, group=group)
    with torch.no_grad():
        for p in model.parameters():
            if arena is None or not p.requires_grad:
                dist.broadcast(p.data, src, group=group)
        for b in model.buffers():
            dist.broadcast(b.data, src, group=group)
    from . import conv
    conv.invalidate_packs()
    rng = getattr(model, "rng", None)
    if rng is not None and hasattr(rng, "seed_toggles"):
        import random
        seed = [random.getrandbits(62) if dist.get_rank(group) == src else 0]
        dist.broadcast_object_list(seed, src, group=group)
        rng.seed_toggles(seed[0])
    base = [random_base_seed() if dist.get_rank(group) == src else 0]
    dist.broadcast_object_list(base, src, group=group)
    torch.manual_seed(base[0] + dist.get_rank(group))          # CPU + every device generator of this process
    return base[0]


def random_base_seed() -> int:
    """Base of the per-rank torch seeds: MRFP_SEED when set (reproducible runs), else drawn from the OS."""
    import random
    v = os.environ.get("MRFP_SEED")
    return int(v) if v is not None else random.SystemRandom().getrandbits(48)


class Trainer:
    """zero_grad -> forward -> backward (+ overlapped all-reduce) -> fused SGD step -> LR step; with accum_steps = k the
    optimiser step, the all-reduce and the LR step happen once per window of k calls, on the sum of the k gradients."""

    def __init__(self, model, lr=1e-2, momentum=0.9, weight_decay=5e-4, max_iter=40000, bucket_mb=32.0,
                 loss_scale=None, max_grad_norm=None, accum_steps=1, loss_weights=None, average=None, loss_fn=None):
        """loss_scale: scale of the backward pass for float16 activations (the per-pixel CE gradient is 1/#pixels ~ 1e-7, below
        float16's normal range).
          None / a float, no max_grad_norm: a STATIC host-side scale, default 65536 when cfg.MODEL.ACT_DTYPE is float16, else 1.
            It enters through the gradient of the loss (the CE backward kernel multiplies by it) and leaves in the fused SGD
            kernel's gradient scale, so parameters see exactly the unscaled step.  Nothing looks at the gradient: an overflow
            reaches the parameters.
          "dynamic": a default LossScaler -- the scale lives on the device, a step whose gradient arena holds an inf / NaN is
            skipped (parameters and momentum untouched, scale halved), 2000 clean steps in a row double the scale.
          a LossScaler: that one (LossScaler(init_scale=s, dynamic=False): fixed scale, still skips non-finite steps -- what a
            float together with max_grad_norm builds; use it for bf16 / fp32 runs).
        max_grad_norm: clip_grad_norm_(parameters, max_grad_norm) of the unscaled, averaged gradient, folded into the step.
        With a scaler no host value enters backward (it is seeded with scaler.scale_tensor) and no step waits for the host;
        step_info() reads the device state back on request.  The poly schedule advances on skipped steps too, and the BatchNorm
        running statistics of a skipped step are kept, as with stock AMP.
        accum_steps = k: gradient accumulation over k micro-batches.  Every step() call runs one forward and
        backward pass and returns that micro-batch's loss; calls 1 .. k-1 of a window add their gradient arena to `flat_a`
        (mrfp_grad_accumulate) and do nothing else -- no optimiser step, no repack, no schedule advance, no collective; call k adds
        the partial sum back, ((g1 + g2) + ...) + gk in this fixed order, all-reduces once per bucket and makes ONE optimiser step
        with the mean over the window (1 / (world * k) folded into the kernel's gradient factor).  The loss scale is constant
        inside a window and the check looks at the summed arena, so a window is applied or skipped as a whole; taken / skipped
        and the schedule count windows, max_grad_norm clips the averaged gradient, BatchNorm running statistics advance per
        micro-batch.  `micro` is the position inside the window (0 .. k-1); save checkpoints at micro == 0, the partial sum is
        not part of one.
        loss_weights: for a model that returns a list / tuple of losses (the network/deepv3.py factories: [main, aux(, wt)]) the
        pass backpropagates sum_i w_i * loss_i, formed on the device, and step() returns that scalar; None: all ones.  A length
        that differs from the returned list, or weights for a model that returns one loss, is a ValueError.
        average: None | a WeightAverage | "ema" | "swa" (= WeightAverage(kind) with its defaults): an averaged copy of the trainable
        parameters in a fourth arena `opt.flat_e`, updated INSIDE the fused step kernel after every applied optimiser step the
        description selects -- one update per accumulation window, none for a step or window the scaler
        skipped (that decision stays on the device), no extra launch, no collective (every rank steps from the same all-reduced
        bits).  averaged() evaluates with it, average_info() counts, save_checkpoint / load_checkpoint carry it.  None, the
        default: nothing is allocated and the step launches what it launched before.
        loss_fn: None | a callable (model, img, label) -> loss | list of losses that the pass runs in place of
        model(img, label, training=True) -- a step with more than one forward (ConsistencyStep: the supervised forward, a teacher's
        forward, a consistency term).  loss_weights applies to what it returns.  Eager only: enable_graph() refuses it."""
        from .config import cfg
        if loss_fn is not None and not callable(loss_fn):
            raise ValueError("loss_fn must be None or a callable (model, img, label) -> loss | list, got %r" % (loss_fn,))
        self.loss_fn = loss_fn
        max_grad_norm = _check_max_grad_norm(max_grad_norm)
        average = _check_average(average)
        self.accum_steps, self.micro = _check_accum_steps(accum_steps), 0
        self.loss_weights = _check_loss_weights(loss_weights)
        if isinstance(loss_scale, str):
            if loss_scale != "dynamic":
                raise ValueError("loss_scale must be None, a number, 'dynamic' or a LossScaler, got %r" % (loss_scale,))
        elif loss_scale is not None and not isinstance(loss_scale, LossScaler):
            if isinstance(loss_scale, bool) or not isinstance(loss_scale, (int, float)):
                raise ValueError("loss_scale must be None, a number, 'dynamic' or a LossScaler, got %r" % (loss_scale,))
            if not (float(loss_scale) > 0.0) or math.isinf(float(loss_scale)):
                raise ValueError("loss_scale must be positive and finite, got %r" % (loss_scale,))
        self.model = model
        self.opt = FlatSGD(model, lr, momentum, weight_decay, max_iter, average=average)
        self._in_average = False
        self.sync = GradSync(self.opt, bucket_mb)
        # (MRFP_FORCE_SYNC=1: the replica synchronisation -- parameter / buffer broadcasts, the shared toggle seed, the per-rank
        #  torch seeds -- also runs at world size 1: the rehearsal of every collective of the multi-GPU path on one GPU over RCCL)
        if dist.is_initialized() and (dist.get_world_size() > 1 or os.environ.get("MRFP_FORCE_SYNC") == "1"):
            sync_replicas(model, self.opt)
        self.scaler, self.max_grad_norm = None, max_grad_norm
        dev = self.opt.flat_p.device
        if isinstance(loss_scale, LossScaler):
            self.scaler = loss_scale.to(dev)
        elif loss_scale == "dynamic":
            self.scaler = LossScaler(device=dev)
        if loss_scale is None or self.scaler is not None:
            static = 65536.0 if cfg.MODEL.ACT_DTYPE == torch.float16 else 1.0
        else:
            static = float(loss_scale)
        if self.scaler is None and max_grad_norm is not None:
            self.scaler = LossScaler(init_scale=static, dynamic=False, device=dev)
        self.loss_scale = static if self.scaler is None else None        # the host-side scale of the unchecked path
        self.graph = False

    def _fwd_bwd(self, img, label):
        from . import conv
        self.opt.zero_grad()
        last = self.micro == self.accum_steps - 1          # only the window's last pass exchanges gradients
        self.sync.begin(reduce=last, accum=last and self.accum_steps > 1)
        ok = False
        try:
            if self.loss_fn is not None:
                loss = self._total_loss(self.loss_fn(self.model, img, label))
            else:
                loss = self._total_loss(self.model(img, label, training=True))
            if self.scaler is not None:
                loss.backward(self.scaler.scale_tensor)      # a device address: a replayed graph reads the scale of its own step
            elif self.loss_scale != 1.0:
                loss.backward(torch.full_like(loss, self.loss_scale))
            else:
                loss.backward()
            ok = True
        finally:
            if not ok:          # a pass that raised leaves queued weight gradients and a pending end-of-backward callback behind
                conv.backward_failed()
        return loss

    def _total_loss(self, loss):
        """A list / tuple of losses -> sum_i w_i * loss_i on the device (a unit weight multiplies nothing: with all ones this is the
        plain sum a hand-written loop forms)."""
        if not isinstance(loss, (list, tuple)):
            if self.loss_weights is not None:
                raise ValueError("loss_weights given, but the model returned one loss")
            return loss
        weights = self.loss_weights if self.loss_weights is not None else (1.0,) * len(loss)
        if len(weights) != len(loss):
            raise ValueError("%d loss_weights for the %d losses the model returned" % (len(weights), len(loss)))
        total = None
        for w, term in zip(weights, loss):
            term = term if w == 1.0 else w * term
            total = term if total is None else total + term
        return total

    def _end_pass(self, gscale):
        """After a pass whose gradients are complete on the current stream (GradSync.finish(), weight-gradient stream joined): an
        inner micro-batch of a window joins the partial sum; the last one (every pass with accum_steps = 1) takes the partial sum
        back -- the bucket path has done that range by range before its collectives -- and makes the optimiser step."""
        k = self.accum_steps
        if self.micro < k - 1:
            self.opt.accumulate(first=self.micro == 0)
            self.micro += 1
            return
        if k > 1 and not self.sync.enabled:
            self.opt.accumulate(into_grad=True)
        self.micro = 0
        self._opt_step(gscale / k)

    def _opt_step(self, gscale):
        """After GradSync.finish(): every rank holds the same all-reduced arena, so with a scaler every rank's check decides from
        identical bits and the loss scales stay in lockstep without a collective."""
        if self.scaler is None:
            self.opt.step(gscale / self.loss_scale)
        else:
            self.opt.step(gscale, scaler=self.scaler, max_grad_norm=self.max_grad_norm)

    def step_info(self):
        """LossScaler.info() of this trainer's scaler (scale, growth_tracker, found_inf, grad_norm, gmul, taken, skipped): one
        device -> host copy, on request only."""
        if self.scaler is None:
            raise _lib.MrfpHipError("step_info: this Trainer has no LossScaler (loss_scale='dynamic' or a LossScaler)")
        return self.scaler.info()

    # ---- the averaged weights ---------------------------------------------------------------------------------------
    def average_info(self):
        """{"t": applied optimiser steps (windows) so far, "n_averaged": averaging updates they made} + the WeightAverage's fields.
        One device -> host copy, and only when a scaler exists (its `taken` word holds the count); none otherwise."""
        avg = self.opt.average
        if avg is None:
            raise _lib.MrfpHipError("average_info: this Trainer keeps no average (average='ema', 'swa' or a WeightAverage)")
        t = self.opt.applied_steps(self.scaler)
        return {"t": t, "n_averaged": averages_made(t, avg.start, avg.every), **avg.config()}

    def _swap_average(self):
        from . import conv
        call("mrfp_arena_swap", ptr(self.opt.flat_p), ptr(self.opt.flat_e), self.opt.n, stream())
        conv.invalidate_packs()                        # the arena changed behind autograd's version counters, as in FlatSGD.step
        conv.repack_all()

    @contextlib.contextmanager
    def averaged(self):
        """`with trainer.averaged():` -- the model runs on the averaged weights.  On entry ONE mrfp_arena_swap exchanges flat_p with
        flat_e and the weight packs are rebuilt; on exit, also when the body raised, the same again, so the parameters come back
        bit for bit.  No pointer changes: parameters stay views of flat_p and captured graphs stay valid.  Inside, evaluate,
        evaluate_tta, validate, predict (with or without fold=True) and model.state_dict() see the averaged weights;
        trainer.step raises.  Only the trainable parameters are averaged: buffers (the BatchNorm running statistics) and frozen
        parameters (the HRFP branch) are the live model's -- after SWA, run update_bn() inside the block before evaluating.
        Raises before any update has happened (the arena would be zeros) and on the CPU."""
        if self.opt.average is None:
            raise _lib.MrfpHipError("averaged: this Trainer keeps no average (average='ema', 'swa' or a WeightAverage)")
        if self._in_average:
            raise _lib.MrfpHipError("averaged: already inside averaged()")
        if self.opt.flat_p.device.type != "cuda":
            raise _lib.MrfpHipError("averaged needs the arenas on the GPU: the HIP path has no CPU fallback")
        if self.average_info()["n_averaged"] == 0:
            raise _lib.MrfpHipError("averaged: no averaging update has happened yet (applied steps %d, start %d)"
                                    % (self.opt.applied_steps(self.scaler), self.opt.average.start))
        self._swap_average()
        self._in_average = True
        try:
            yield self
        finally:
            self._swap_average()
            self._in_average = False

    def step(self, img, label):
        if self._in_average:
            raise _lib.MrfpHipError("Trainer.step inside averaged(): the parameter arena holds the averaged weights")
        if self.graph:
            return self._graph_step(img, label)
        loss = self._fwd_bwd(img, label)
        gscale = self.sync.finish()
        from . import conv, ops
        conv.join_wgrad_stream()                       # weight gradients are computed on a second stream
        self._end_pass(gscale)
        if ops._SYNC_BN_FLAG:                          # cfg.MODEL.SYNC_BN over several ranks: the device-side count check (no host wait)
            ops.sync_bn_poll()
        return loss

    # ---- hipGraph mode --------------------------------------------------------------------------------------------
    # zero_grad + forward + backward (~2900 kernel launches, ~28 ms of Python + ctypes per ResNet-101 step) are captured
    # once per (perturbation toggle combination, input shape) and replayed with one hipGraphLaunch; the optimizer step
    # (learning rate and first-step flag are by-value kernel arguments), the batched weight repack and, with accum_steps > 1, the
    # accumulate launch and the decision whether to step stay eager.
    # Single-process only: the overlapped all-reduce of GradSync is driven by Python hooks.
    def enable_graph(self):
        if self.loss_fn is not None:
            # (the capture fixes ONE toggle draw per step and one forward; a second forward inside it is out of scope)
            raise _lib.MrfpHipError("Trainer graph mode captures model(img, label, training=True): a Trainer with a loss_fn runs eagerly")
        if self.sync.enabled:
            raise _lib.MrfpHipError("Trainer graph mode is single-process (the overlapped all-reduce is hook-driven)")
        self.graph = True
        self._graphs = {}
        self._bns = [m for m in self.model.modules() if hasattr(m, "_nbt_pending")]
        return self

    def _graph_step(self, img, label):
        rng = self.model.rng
        tog = tuple(rng.toggles())
        key = (tuple(t < 0.5 for t in tog), tuple(img.shape), img.dtype, tuple(label.shape))
        entry = self._graphs.get(key)

        class _Fixed:                       # the toggles drawn above, everything else from the model's own rng
            def __init__(self, base, t):
                self._b, self._t = base, t

            def toggles(self):
                return self._t

            def __getattr__(self, name):
                return getattr(self._b, name)

        if entry is None:
            static_img, static_lab = img.clone(), label.clone()
            self.model.rng = _Fixed(rng, tog)
            try:
                # ONE capture stream for every key: autograd's gradient accumulators remember the stream they first ran on, and a
                # capture on another stream is forked / joined once per parameter (a cross-queue barrier each at replay)
                if getattr(self, "_graph_stream", None) is None:
                    self._graph_stream = torch.cuda.Stream()
                side = self._graph_stream
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):           # eager warm-up on a side stream (lazy tables, attributes, packs)
                    loss = self._fwd_bwd(static_img, static_lab).detach()
                torch.cuda.current_stream().wait_stream(side)
                from . import conv
                conv.join_wgrad_stream()
                self._end_pass(1.0)                      # (the window logic of an eager step: the warm-up call is one)
                if self.micro != 0:
                    # an inner micro-batch made no optimiser step: leave the weight packs as a step leaves them, so that the
                    # capture records the lazy re-pack of the packs repack_all() does not cover (a pack with a bias: final2) --
                    # every replay has to rebuild them from the parameters of ITS step
                    conv.invalidate_packs()
                    conv.repack_all()
                conv.prebuild_repack_tables()            # (job tables of the batched re-packs: no host -> device copy inside the capture)
                # capture on the warm-up's stream, with the warm-up's autograd graph gone (.detach() above): a gradient
                # accumulator that remembers another stream makes autograd fork / join the capture once per parameter, and
                # the replay of such a graph pays a cross-queue barrier per fork (35 vs 15 ms on ResNet-50 8x512^2)
                g = torch.cuda.CUDAGraph(keep_graph=True)       # (the hipGraph_t stays readable: graph_topology())
                if getattr(self, "_debug_capture_on_fresh_stream", False):      # tools/graph_dbg.py only: the round-2 capture, for evidence
                    side = torch.cuda.Stream()
                    side.wait_stream(self._graph_stream)
                with torch.cuda.graph(g, stream=side):
                    static_loss = self._fwd_bwd(static_img, static_lab).detach()    # only the value is read at replay: no autograd graph
                                                                                      # (and its accumulator nodes) kept alive per key
            finally:
                self.model.rng = rng
            for m in self._bns:                           # the capture pass ran the Python side of every layer once more
                if m.training and m.num_batches_tracked is not None:
                    m._nbt_pending -= 1
            entry = (g, static_img, static_lab, static_loss)
            self._graphs[key] = entry
            return loss                                   # this call was the eager warm-up step
        g, static_img, static_lab, static_loss = entry
        static_img.copy_(img)
        static_lab.copy_(label)
        g.replay()
        for m in self._bns:
            if m.training and m.num_batches_tracked is not None:
                m._nbt_pending += 1
        self._end_pass(1.0)                               # eager, after the replay: accumulate, or close the window and step
        return static_loss


class ConsistencyStep:
    """A Trainer loss_fn: the supervised step plus a consistency term between the model's scores and a teacher's.
        step = ConsistencyStep(loss.ConsistencyLoss2d("kl", temperature=2.0), weight=0.5, teacher=teacher_model)
        Trainer(model, loss_fn=step, ...)
    Per call: (1) model(img, label, training=True) with keep_scores, so the head leaves model.last_scores, the autograd-attached
    low-resolution scores its fused loss read; (2) under no_grad, teacher(img, training=False, low_res=True), the teacher's padded
    low-resolution scores (another output stride or pitch is fine); (3) criterion(student scores, teacher scores, valid) on the fused
    kernels, valid = the labels (valid_from_labels: ignored pixels do not count) or None.  Returns [*supervised, weight * consistency]:
    Trainer(loss_weights=) still applies, with one more entry.
    teacher=None: the model's OWN unperturbed view, model(img, training=False, low_res=True) -- MRFPPlus only, whose perturbations
    are switched by the `training` argument while the module stays in train() mode.  Its BatchNorm layers therefore normalise that
    view with batch statistics and update their running statistics from it too: every step feeds them one perturbed and one
    unperturbed batch.  A separate teacher module should be in eval() mode (network/deepv3.py factories require it for low_res);
    it is never written: no parameter, no buffer.  `model` may be a wrapper: the first submodule with keep_scores is used."""

    def __init__(self, criterion, weight=1.0, teacher=None, valid_from_labels=True):
        from .loss import ConsistencyLoss2d
        if not isinstance(criterion, ConsistencyLoss2d):
            raise TypeError("ConsistencyStep: criterion must be a loss.ConsistencyLoss2d, got %r" % (type(criterion),))
        if isinstance(weight, bool) or not isinstance(weight, (int, float)) or not math.isfinite(float(weight)):
            raise ValueError("ConsistencyStep: weight must be a finite number, got %r" % (weight,))
        self.criterion, self.weight, self.teacher, self.valid_from_labels = criterion, float(weight), teacher, bool(valid_from_labels)

    @staticmethod
    def _scored(model):
        for m in model.modules():
            if hasattr(m, "keep_scores") and hasattr(m, "_head"):
                return m
        raise TypeError("ConsistencyStep: the model has no head that keeps its scores (deepv3._DeepLabBase.keep_scores)")

    def __call__(self, model, img, label):
        from .deepv3 import MRFPPlus
        net = self._scored(model)
        if self.teacher is None and not isinstance(net, MRFPPlus):
            raise TypeError("ConsistencyStep(teacher=None) takes the model's own unperturbed view, which only MRFPPlus has "
                            "(its perturbations follow the `training` argument): give %s a teacher module" % type(net).__name__)
        was = net.keep_scores
        net.keep_scores = True
        try:
            sup = model(img, label, training=True)
        finally:
            net.keep_scores = was
        student, net.last_scores = net.last_scores, None
        with torch.no_grad():
            P = (net if self.teacher is None else self.teacher)(img, training=False, low_res=True)
        from .loss import ScoreMap
        cons = self.criterion(student, ScoreMap(P, student.size, student.channels), label if self.valid_from_labels else None)
        sup = list(sup) if isinstance(sup, (list, tuple)) else [sup]
        return sup + [cons if self.weight == 1.0 else self.weight * cons]


def graph_topology(g):
    """Nodes / dependency edges of a captured torch.cuda.CUDAGraph(keep_graph=True) read back through the HIP runtime
    (hipGraphGetNodes / hipGraphGetEdges): {"nodes", "edges", "forks" (nodes with more than one successor), "joins" (more than
    one predecessor), "roots"}.  A capture that stayed on ONE stream is a chain: forks == joins == 0, one root.  Every stream the
    capture forked to shows up as a fork / join pair -- and each pair becomes a cross-queue dependency at replay (the round-2
    capture had one pair per parameter: see DESIGN.md section 5)."""
    import ctypes
    hip = ctypes.CDLL("libamdhip64.so.7")
    graph = ctypes.c_void_p(int(g.raw_cuda_graph()))
    n = ctypes.c_size_t(0)
    hip.hipGraphGetNodes.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t)]
    hip.hipGraphGetEdges.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t)]
    if hip.hipGraphGetNodes(graph, None, ctypes.byref(n)) != 0:
        raise _lib.MrfpHipError("hipGraphGetNodes failed")
    e = ctypes.c_size_t(0)
    if hip.hipGraphGetEdges(graph, None, None, ctypes.byref(e)) != 0:
        raise _lib.MrfpHipError("hipGraphGetEdges failed")
    src, dst = (ctypes.c_void_p * max(1, e.value))(), (ctypes.c_void_p * max(1, e.value))()
    if e.value and hip.hipGraphGetEdges(graph, src, dst, ctypes.byref(e)) != 0:
        raise _lib.MrfpHipError("hipGraphGetEdges failed")
    out_deg, in_deg = {}, {}
    for i in range(e.value):
        out_deg[src[i]] = out_deg.get(src[i], 0) + 1
        in_deg[dst[i]] = in_deg.get(dst[i], 0) + 1
    return {"nodes": int(n.value), "edges": int(e.value), "forks": sum(1 for v in out_deg.values() if v > 1),
            "joins": sum(1 for v in in_deg.values() if v > 1), "roots": int(n.value) - len(in_deg)}


@torch.no_grad()
def evaluate(model, batches, num_classes=19, fold=False):
    """reference main.py:887-913: model.eval(), per-image arg-max + confusion histogram (on the device,
    one 19x19 int64 D2H at the end instead of two full-logit copies per image), mIoU as metrics.py:60-85.
    fold=True: the forwards run inside inference.fold_norms(model) (eval-mode BatchNorms folded into their convolutions)."""
    from . import metrics, ops
    if fold:
        from .inference import fold_norms
        with fold_norms(model):
            return evaluate(model, batches, num_classes)
    model.eval()
    hist, dropped = None, 0
    for img, label in batches:
        if img.shape[2:] != label.shape[1:]:        # reference main.py:894, 910-912
            dropped += 1
            continue
        logits = model(img, training=False)
        hist, _ = ops.argmax_hist(logits, label, hist)
    if dist.is_initialized() and dist.get_world_size() > 1:
        if hist is None:                              # this rank dropped all of its batches: still take part
            dev = next(model.parameters()).device
            hist = torch.zeros(num_classes, num_classes, dtype=torch.int64, device=dev)
        dist.all_reduce(hist)
    h = hist.cpu().numpy() if hist is not None else None
    return h, (metrics.miou_from_hist(h) if h is not None else 0.0), dropped


@contextlib.contextmanager
def _eval_mode(model, fold):
    """model.eval() for the length of a `with`, inside inference.fold_norms(model) when `fold`; the training flags of every module
    are put back on the way out."""
    flags = [(m, m.training) for m in model.modules()]
    try:
        with contextlib.ExitStack() as stack:
            if fold:
                from .inference import fold_norms
                stack.enter_context(fold_norms(model))
            model.eval()
            yield
    finally:
        for m, f in flags:
            m.training = f


def update_bn(model, batches):
    """What torch.optim.swa_utils.update_bn does, for this project's calling convention: the BatchNorm running statistics of
    averaged weights belong to no set of weights that ever ran, so they are re-estimated before evaluation.  For every
    HipBatchNorm2d (subclasses included) with running statistics: running_mean <- 0, running_var <- 1, num_batches_tracked and the
    host-side pending count <- 0; then `model(img, label, training=True)` under torch.no_grad() for each (img, label) of `batches`
    with the module's momentum set to 1 / (j + 1) for batch j (0-based) -- the cumulative mean of the batch statistics, as
    momentum=None gives in torch.  `momentum` and the training flags of every module are put back on the way out, also when a
    forward raises; num_batches_tracked ends at the number of batches.  The forwards are training forwards in every other respect:
    perturbations and the HRFP re-initialisation are drawn from model.rng as in training, and dropout is live.  Typical use:
    `with trainer.averaged(): update_bn(model, loader); evaluate(model, val)` -- note that the re-estimated buffers stay in the
    model after the block (buffers are not averaged and not swapped).  -> the number of modules updated."""
    from .network.mynn import HipBatchNorm2d
    bns = [m for m in model.modules()
           if isinstance(m, HipBatchNorm2d) and m.track_running_stats and m.running_mean is not None]
    if not bns:
        return 0
    momenta = [m.momentum for m in bns]
    flags = [(m, m.training) for m in model.modules()]
    try:
        with torch.no_grad():
            for m in bns:
                m.running_mean.zero_()
                m.running_var.fill_(1.0)
                if m.num_batches_tracked is not None:
                    m.num_batches_tracked.zero_()
                m._nbt_pending = 0
            model.train()
            for j, (img, label) in enumerate(batches):
                for m in bns:
                    m.momentum = 1.0 / (j + 1)
                model(img, label, training=True)
    finally:
        for m, mom in zip(bns, momenta):
            m.momentum = mom
        for m, f in flags:
            m.training = f
    return len(bns)


@torch.no_grad()
def predict(model, images, fold=False, want_conf=False):
    """Label maps of a trained model, a generator: per float32 [B,3,H,W] batch of `images` (as the evaluation transforms produce
    them) ONE forward with low_res=True and ONE ops.upsample_argmax at the image's own size -> (pred uint8 [B,H,W], conf float32
    [B,H,W] or None).  The prediction is np.argmax of model(img, training=False), pixel for pixel (reference main.py:896-900); the
    full-resolution logits are never written.  conf: the largest soft-max probability.  Runs under torch.no_grad (the caller's grad
    mode is untouched between two batches) with model.eval(); fold=True: inside inference.fold_norms(model).  The model stays in
    eval() while the generator is being consumed; its training flags are restored when the generator ends or is closed."""
    from . import ops
    with _eval_mode(model, fold):
        for img in images:
            low = model(img, training=False, low_res=True)
            r = ops.upsample_argmax(low, img.shape[2:], _num_classes(model, low), want_pred=True, want_conf=want_conf)
            yield r.pred, r.conf


def _num_classes(model, low):
    nc = getattr(model, "num_classes", None)
    if nc is None:
        final2 = getattr(model, "final2", None)
        nc = final2[0].out_channels if final2 is not None else None
    if nc is None:
        raise _lib.MrfpHipError("predict: cannot tell the class count of %s (no num_classes, no final2)" % type(model).__name__)
    return int(nc)


@torch.no_grad()
def validate(model, batches, num_classes=19, fold=False, ignore_index=255, per_image=False):
    """evaluate()'s loop on the fused kernel (ops.upsample_argmax): one forward with low_res=True per batch, then arg-max, confusion
    histogram and the plain cross entropy in one launch -- the full-resolution logits are never written -- and ONE device -> host
    copy at the end.  Same drop rule for size mismatches (reference main.py:894, 910-912), histograms (and the two loss
    accumulators) summed over the data-parallel ranks as in evaluate(); `dropped` stays per rank.  -> dict:
      hist, mean_iu, dropped   what evaluate() returns (hist None / mean_iu 0.0 when every batch was dropped)
      val_loss                 sum nll / valid pixels over ALL batches, pixel-weighted (build-defined: the reference's evaluation
                               bookkeeping, utils/misc.py:139-156, tracks a val_loss its eval loop never computes); NaN without a
                               valid pixel
      pixels                   the valid pixels (labels in 0..num_classes-1 other than ignore_index)
      image_hists              int64 [N,C,C], one matrix per kept image in order (per_image only; per rank)"""
    import numpy as np
    from . import metrics, ops
    C = int(num_classes)
    dev = next(model.parameters()).device
    hist = torch.zeros(C, C, dtype=torch.int64, device=dev)
    loss_acc = torch.zeros(2, dtype=torch.float64, device=dev)
    per, dropped, kept = [], 0, 0
    with _eval_mode(model, fold):
        for img, label in batches:
            if img.shape[2:] != label.shape[1:]:        # reference main.py:894, 910-912
                dropped += 1
                continue
            low = model(img, training=False, low_res=True)
            if per_image:
                r = ops.upsample_argmax(low, img.shape[2:], C, label, ignore_index, per_image=True, want_pred=False, loss_acc=loss_acc)
                per.append(r.hist)
            else:
                ops.upsample_argmax(low, img.shape[2:], C, label, ignore_index, hist=hist, want_pred=False, loss_acc=loss_acc)
            kept += 1
    image_hists = None
    if per_image:
        image_hists = torch.cat(per) if per else torch.zeros(0, C, C, dtype=torch.int64, device=dev)
        hist = image_hists.sum(0)
    distributed = dist.is_initialized() and dist.get_world_size() > 1
    if distributed:
        dist.all_reduce(hist)                         # (a rank that dropped all of its batches still takes part, as in evaluate)
        dist.all_reduce(loss_acc)
    # one device -> host copy: the histogram, the two accumulators (their bits) and the per-image matrices in one int64 buffer
    parts = [hist.reshape(-1), loss_acc.view(torch.int64)] + ([image_hists.reshape(-1)] if per_image else [])
    host = torch.cat(parts).cpu().numpy()
    h = host[:C * C].reshape(C, C).copy() if (kept or distributed) else None
    nll, pixels = (float(v) for v in host[C * C:C * C + 2].view(np.float64))
    out = {"hist": h, "mean_iu": metrics.miou_from_hist(h) if h is not None else 0.0, "dropped": dropped,
           "val_loss": nll / pixels if pixels > 0 else float("nan"), "pixels": int(pixels)}
    if per_image:
        out["image_hists"] = host[C * C + 2:].reshape(-1, C, C).copy()
    return out


def eval_batches(samples, transform, encoder=None):
    """(uint8 [H,W,3] image, uint8 [H,W] label map) device pairs -> the (img [1,3,h,w] float32, label [1,h,w] int64) batches that
    evaluate / evaluate_tta consume, one sample at a time as the reference's batch-1 loop (main.py:887-913) sees them.
    transform: input_pipeline.EvalTransform() or ResizeHeightCenterCropPad(eval_size); encoder: a LabelEncoder or None.
    evaluate(model, eval_batches(samples, EvalTransform(), label_encoder("CityscapesSegmentation"))) is that loop."""
    for img_u8, lab_u8 in samples:
        img, lab = transform(img_u8, lab_u8, encoder)
        yield img.unsqueeze(0), lab.unsqueeze(0)


def train_batches(samples, transform, batch_size, items=None, encoder=None, rng=random, np_rng=np.random, drop_last=True):
    """The training sibling of eval_batches: samples[i] -> (uint8 [H,W,3] image, uint8 [H,W] label map) on the device; yields
    (img [B,3,T,T] float32, label [B,T,T] int64), T = transform.crop_size (a transform with square crops: TrainTransform,
    ScaleCropTransform), every sample written by `transform` into its slot of the batch (out_img / out_lab).  items: the epoch of input_pipeline.ClassUniformSampler, [(index, centroid | None, class_id | None)],
    or None for samples 0 .. len - 1 in order; an item with a centroid is drawn with transform.draw(..., centroid=) (TrainTransform),
    one without exactly as before.  encoder: a LabelEncoder, applied to the label map first (mrfp_label_lut_u8), as the reference's
    __getitem__ encodes before it transforms.  rng / np_rng: the streams the draws consume.  drop_last: a trailing batch of fewer
    than batch_size samples is dropped, else yielded short."""
    from .input_pipeline import _out_slot
    batch_size, T = int(batch_size), int(transform.crop_size)
    if batch_size < 1:
        raise ValueError("train_batches: batch_size must be >= 1, got %r" % (batch_size,))
    if items is None:
        items = [(i, None, None) for i in range(len(samples))]
    for lo in range(0, len(items), batch_size):
        chunk = items[lo:lo + batch_size]
        if len(chunk) < batch_size and drop_last:
            return
        img = lab = None
        for j, (index, centroid, _cls) in enumerate(chunk):
            img_u8, lab_u8 = samples[index]
            if img is None:
                img = _out_slot(None, (len(chunk), 3, T, T), torch.float32, img_u8.device, "img")
                lab = _out_slot(None, (len(chunk), T, T), torch.int64, img_u8.device, "label")
            if encoder is not None:
                lab_u8 = encoder(lab_u8)
            h, w = lab_u8.shape
            d = transform.draw(w, h, rng, np_rng) if centroid is None else transform.draw(w, h, rng, np_rng, centroid=centroid)
            transform(img_u8, lab_u8, d, out_img=img[j], out_lab=lab[j])
        yield img, lab


# ------------------------------------------------------------------------------------------
# multi-scale / flipped / sliding-window evaluation (build-defined: the reference scores one forward per image)
# ------------------------------------------------------------------------------------------
def _window_starts(size: int, win: int, stride: int):
    if size <= win:
        return [0]
    starts = list(range(0, size - win, stride))
    starts.append(size - win)                 # the last window is shifted back so that it ends at the border
    return starts


def window_grid(height: int, width: int, window=None, stride=None):
    """Sliding-window rectangles (y, x, h, w) over a height x width image, rows outer.  Windows start on a grid of `stride`
    (default: two thirds of the window, rounded up); the last row / column of windows is shifted back so that it ends at the image
    border: every pixel is covered, no window leaves the image, nothing is padded.  A dimension not larger than the window is one
    window of the image's own size.  window=None: the whole image."""
    height, width = int(height), int(width)
    if height < 1 or width < 1:
        raise ValueError("empty image %d x %d" % (height, width))
    if window is None:
        return [(0, 0, height, width)]
    wh, ww = int(window[0]), int(window[1])
    if wh < 1 or ww < 1:
        raise ValueError("window must be positive, got %r" % (window,))
    sy, sx = (-(-2 * wh // 3), -(-2 * ww // 3)) if stride is None else (int(stride[0]), int(stride[1]))
    if sy < 1 or sx < 1:
        raise ValueError("stride must be positive, got %r" % (stride,))
    if sy > wh or sx > ww:
        raise ValueError("stride %r larger than the window %r would leave pixels uncovered" % ((sy, sx), (wh, ww)))
    hh, hw = min(wh, height), min(ww, width)
    return [(y, x, hh, hw) for y in _window_starts(height, wh, sy) for x in _window_starts(width, ww, sx)]


def window_dest_rect(win, src_size, dst_size):
    """The rectangle (y0, x0, hd, wd) a window (y, x, h, w) of a src_size = (Hs, Ws) image has in the dst_size = (Hd, Wd)
    accumulator.  Rounding rule, in integer arithmetic: the start is rounded DOWN, y0 = floor(y * Hd / Hs), and the end UP,
    y0 + hd = ceil((y + h) * Hd / Hs) (columns alike).  Windows that cover the source therefore cover the destination without a
    gap (overlaps are allowed and weighted by cnt), and for Hs == Hd the rectangle is the window itself."""
    y, x, h, w = win
    (Hs, Ws), (Hd, Wd) = src_size, dst_size
    y0, y1 = (y * Hd) // Hs, -(-((y + h) * Hd) // Hs)
    x0, x1 = (x * Wd) // Ws, -(-((x + w) * Wd) // Ws)
    return y0, x0, y1 - y0, x1 - x0


def _check_tta_args(scales, window, stride):
    scales = tuple(float(s) for s in scales)
    if not scales:
        raise ValueError("scales must not be empty")
    if any(not (s > 0.0) or math.isinf(s) for s in scales):
        raise ValueError("scales must be positive and finite, got %r" % (scales,))
    if stride is not None and window is None:
        raise ValueError("stride given without window")
    if window is not None:
        window_grid(max(1, int(window[0])), max(1, int(window[1])), window, stride)      # raises on a bad window / stride
    return scales


def tta_variants(height, width, dst_size, scales, flip, window, stride):
    """The (scale, scaled size, flipped, window, destination rectangle) list of one image, in issue order: what evaluate_tta runs
    and what a restatement has to replay.  Scaled size = (round(height * s), round(width * s)), at least 1."""
    out = []
    for s in scales:
        hs, ws = (height, width) if s == 1.0 else (max(1, int(round(height * s))), max(1, int(round(width * s))))
        for win in window_grid(hs, ws, window, stride):
            rect = window_dest_rect(win, (hs, ws), dst_size)
            for f in ((False, True) if flip else (False,)):
                out.append((s, (hs, ws), f, win, rect))
    return out


@torch.no_grad()
def evaluate_tta(model, batches, num_classes=19, scales=(1.0,), flip=False, window=None, stride=None, resize_to_label=False,
                 on_variant=None, fold=False):
    """evaluate() with test-time augmentation: class PROBABILITIES averaged over image scales, a horizontal flip and overlapping
    windows, then arg-max + confusion histogram -> (hist, mIoU, dropped), the triple evaluate() returns.

    Per image and per scale s the input is resized to round(H*s) x round(W*s) with the bilinear align_corners operator (s == 1.0: used
    as it is), cut into window_grid(...) windows (window=None: one forward of the whole scaled image), and every window is forwarded
    once, and once more horizontally mirrored with flip=True.  The model returns its LOW-resolution class scores
    (model(x, training=False, low_res=True)); ops.prob_accum resizes them (the bilinear align_corners resize the head itself ends
    with) straight into the window's rectangle of a full-size fp32 accumulator, soft-maxes and adds: the full-size logits are never
    written.  For s != 1 the rectangle is the window mapped back through the scale with window_dest_rect's rule (start rounded
    down, end rounded up).  ops.acc_argmax_hist closes each image.  Every variant has weight 1.

    resize_to_label=False drops an image whose size differs from its label's, as evaluate() and the reference do (main.py:894,
    910-912); True scores it at the label's size instead.  Histograms are summed over the data-parallel ranks as in evaluate();
    `dropped` stays per rank.  on_variant(image index, variant, low-resolution scores): measurement / test hook.
    fold=True: the forwards run inside inference.fold_norms(model)."""
    from . import metrics, ops
    if fold:
        from .inference import fold_norms
        with fold_norms(model):
            return evaluate_tta(model, batches, num_classes, scales, flip, window, stride, resize_to_label, on_variant)
    scales = _check_tta_args(scales, window, stride)
    model.eval()
    dev = next(model.parameters()).device
    hist, dropped = None, 0
    uncovered = torch.zeros(1, dtype=torch.int64, device=dev)
    for idx, (img, label) in enumerate(batches):
        H, W = int(img.shape[2]), int(img.shape[3])
        Hd, Wd = int(label.shape[1]), int(label.shape[2])
        if (H, W) != (Hd, Wd) and not resize_to_label:
            dropped += 1
            continue
        B = int(img.shape[0])
        acc = torch.zeros(B, Hd, Wd, num_classes, dtype=torch.float32, device=img.device)
        cnt = torch.zeros(B, Hd, Wd, dtype=torch.float32, device=img.device)
        scaled = {}
        for var in tta_variants(H, W, (Hd, Wd), scales, flip, window, stride):
            s, size, f, (y, x, h, w), rect = var
            if size not in scaled:
                scaled = {size: img if size == (H, W) else ops.upsample_bilinear(img, size)}     # one scaled copy alive at a time
            crop = scaled[size][:, :, y:y + h, x:x + w]
            if f:
                crop = torch.flip(crop, dims=(3,))
            low = model(crop, training=False, low_res=True)
            if on_variant is not None:
                on_variant(idx, var, low)
            ops.prob_accum(low, acc, cnt, rect, flip=f)
        hist, _ = ops.acc_argmax_hist(acc, cnt, label, hist, uncovered=uncovered)
    if dist.is_initialized() and dist.get_world_size() > 1:
        if hist is None:                              # this rank dropped all of its batches: still take part
            hist = torch.zeros(num_classes, num_classes, dtype=torch.int64, device=dev)
        dist.all_reduce(hist)
    if int(uncovered.item()) != 0:
        raise _lib.MrfpHipError("evaluate_tta: %d pixels were covered by no window" % int(uncovered.item()))
    h = hist.cpu().numpy() if hist is not None else None
    return h, (metrics.miou_from_hist(h) if h is not None else 0.0), dropped


# ------------------------------------------------------------------------------------------
# checkpoints in the reference's format (reference main.py:867-869, 884-886)
# ------------------------------------------------------------------------------------------
def save_checkpoint(path, model, epoch, optimizer=None):
    """{'epoch', 'state_dict', 'optimizer'} as reference main.py:867-869 writes it, with the `module.` prefix
    nn.DataParallel gives the keys.  `optimizer`: a FlatSGD / Trainer (its torch.optim.SGD-layout state_dict() is
    stored), a torch optimizer, or an already-built state dict.  A Trainer that keeps a weight average adds an 'average' entry of
    plain numbers, strings and tensors: kind, decay, warmup, start, every, t (applied optimiser steps), n_averaged, and
    `state_dict` -- the model's full state dict, `module.`-prefixed like the main one, with the trainable tensors cut from the
    averaged arena (no swap; buffers and frozen parameters are the live model's), which loads straight into a model for
    deployment.  With n_averaged == 0 those tensors are the zeros the arena was created with."""
    msd = model.state_dict()
    sd = {"module." + k: v.detach().cpu() for k, v in msd.items()}
    ck = {"epoch": epoch, "state_dict": sd}
    if optimizer is not None:
        opt = getattr(optimizer, "opt", optimizer)                  # Trainer -> its FlatSGD
        ck["optimizer"] = opt.state_dict() if hasattr(opt, "state_dict") else opt
        if getattr(optimizer, "scaler", None) is not None:          # a Trainer with a LossScaler: GradScaler's dict of plain numbers
            ck["scaler"] = optimizer.scaler.state_dict()
        if getattr(opt, "average", None) is not None and isinstance(optimizer, Trainer):
            ck["average"] = _average_entry(optimizer, model, msd)
    torch.save(ck, path)


def _average_entry(trainer, model, msd):
    opt = trainer.opt
    if trainer._in_average:
        raise _lib.MrfpHipError("save_checkpoint inside averaged(): the arenas are exchanged; save outside the block")
    slot = {id(p): (o, p.numel()) for p, o in zip(opt.params, opt.offsets)}
    cut = {name: slot[id(p)] for name, p in model.named_parameters(remove_duplicate=False) if id(p) in slot}
    sd = {}
    for k, v in msd.items():
        if k in cut:
            o, numel = cut[k]
            v = opt.flat_e[o:o + numel].view(v.shape)
        sd["module." + k] = v.detach().clone().cpu()
    return {**trainer.average_info(), "state_dict": sd}


def _load_average(trainer, entry):
    """The averaged arena and the step count t of a checkpoint's 'average' entry into a Trainer that keeps an average (its own
    description stays: kind / decay / start / every of the file are informative).  The scaler's `taken` word is not part of its
    state dict, so taken_base takes up the difference: t = taken + taken_base holds again, on every rank alike."""
    opt = trainer.opt
    sd = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in entry["state_dict"].items()}
    slot = {id(p): (o, p.numel()) for p, o in zip(opt.params, opt.offsets)}
    opt.flat_e.zero_()
    for name, p in trainer.model.named_parameters():
        if id(p) not in slot:
            continue
        if name not in sd:
            raise _lib.MrfpHipError("checkpoint 'average' entry has no tensor for %s" % name)
        o, numel = slot[id(p)]
        if sd[name].numel() != numel:
            raise _lib.MrfpHipError("checkpoint 'average' entry: %s has %d values, the parameter %d" % (name, sd[name].numel(), numel))
        opt.flat_e[o:o + numel].copy_(sd[name].reshape(-1).to(opt.flat_e.device, torch.float32))
    taken = trainer.scaler.info()["taken"] if trainer.scaler is not None else 0
    opt.taken_base = int(entry["t"]) - taken


def load_checkpoint(path_or_dict, model, strict=True, optimizer=None, trust_pickle=False):
    """Loads a reference checkpoint (keys with or without the `module.` prefix) into the HIP model and, when
    `optimizer` (FlatSGD / Trainer) is given and the checkpoint has an 'optimizer' entry, the momentum buffers and the
    schedule position (reference main.py:884-886 + the 'optimizer' entry of main.py:867); a 'scaler' entry is restored when
    `optimizer` is a Trainer with a LossScaler, and an 'average' entry (the averaged arena and its step count) when it is a
    Trainer that keeps a weight average; files without them load as before.  The reference's format
    ({'epoch', 'state_dict', 'optimizer'} of tensors, numbers, lists and dicts) loads under torch's safe unpickler;
    `trust_pickle=True` opts into arbitrary pickles for files of known origin only."""
    ck = (torch.load(path_or_dict, map_location="cpu", weights_only=not trust_pickle)
          if isinstance(path_or_dict, str) else path_or_dict)
    sd = ck["state_dict"] if "state_dict" in ck else ck
    sd = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in sd.items()}
    with torch.no_grad():
        missing = model.load_state_dict(sd, strict=strict)
    from . import conv
    conv.invalidate_packs()
    if optimizer is not None and isinstance(ck, dict) and ck.get("optimizer") is not None:
        getattr(optimizer, "opt", optimizer).load_state_dict(ck["optimizer"])
    if getattr(optimizer, "scaler", None) is not None and isinstance(ck, dict) and ck.get("scaler") is not None:
        optimizer.scaler.load_state_dict(ck["scaler"])
    if (isinstance(optimizer, Trainer) and optimizer.opt.average is not None and isinstance(ck, dict)
            and ck.get("average") is not None):
        _load_average(optimizer, ck["average"])
    return ck.get("epoch", None) if isinstance(ck, dict) else None, missing
