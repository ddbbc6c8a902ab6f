"""The weight-gradient scheduling policy of mrfp_amd/conv.py, recorded on the CPU: which queued weight gradients leave in which
launch, after which event, and who is told.  No GPU and no kernel runs: the name `call` as conv sees it, `wgrad_workspace` and the
stream query are replaced by stubs that log (entry point, problem count, geometry), the byte cap is set directly, the operands are
CPU tensors of a few elements (only numel * element_size matters to the policy), and the gradients are submitted from inside the
backward of a small CPU autograd Function, where queueing the end-of-backward callback is legal.

    python tools/record_wgrad_schedule.py        rewrites tests/golden/wgrad_schedule.json

tests/test_wgrad_schedule_cpu.py replays record() and compares with the file.  The file was written ONCE, by this script, from the
commit before the scheduler became one object (module-level functions and one-element lists: the second half of Adapter); it is the
yardstick for the object and is not to be regenerated from it.
"""
import json
import os
import sys
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from mrfp_amd import conv, ops  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "wgrad_schedule.json")
NO_CAP = 1 << 50
ITEM_BYTES = 2 * 4 * 4          # x and dy of one problem: four fp32 elements each


class Adapter:
    """submit / flush / drop / backward_failed and the scheduler's state, on the scheduler object (conv._WGRADS) or on the free
    functions and module cells it replaced."""

    def __init__(self):
        self.obj = getattr(conv, "_WGRADS", None)
        self.flush = conv.flush_wgrads
        self.backward_failed = conv.backward_failed
        if self.obj is not None:
            self.submit, self.drop = self.obj.submit, self.obj.drop_stale
            self.saved = dict(vars(self.obj))
        else:
            self.submit, self.drop = conv._queue_wgrad, conv._drop_stale_backward_state

    def reset(self, cap):
        """a scheduler that has seen nothing, with the byte cap set (torch.cuda.mem_get_info is never asked)"""
        if self.obj is not None:
            self.obj.__init__()
            self.obj.max_bytes = cap
        else:
            for d in (conv._WG_QUEUE, conv._WG_SEEN, conv._WG_EXPECT, conv._WG_EXPECT_ALL):
                d.clear()
            conv._WG_PASS_KEY[0], conv._WG_PENDING_BYTES[0], conv._JOIN_QUEUED[0] = None, 0, False
            conv._WG_MAX_BYTES[0] = cap
        ops.GRAD_DEFERRED.clear()
        conv.WGRAD_GROUP_LAUNCHES.clear()

    def restore(self):
        if self.obj is not None:
            vars(self.obj).clear()
            vars(self.obj).update(self.saved)

    def queues(self):
        return self.obj.queues if self.obj is not None else conv._WG_QUEUE

    def callback_queued(self):
        return self.obj.callback_queued if self.obj is not None else conv._JOIN_QUEUED[0]

    def kinds(self):
        return self.obj.expect_all if self.obj is not None else conv._WG_EXPECT_ALL

    def group_max(self):
        return self.obj.group_max if self.obj is not None else conv._GROUP_MAX[0]


def sig(g):
    """launch geometry number g: (dtype, B, H, W, Cphys, C, N, Nphys, R, S, Ho, Wo, stride, pad_h, pad_w, dil) with N = 1000 + g"""
    return (torch.float32, 1, 2, 2, 4, 4, 1000 + g, 1000 + g, 1, 1, 2, 2, 1, 0, 0, 1)


class _Pass(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t, body):
        ctx.body = body
        return t.clone()

    @staticmethod
    def backward(ctx, g):
        ctx.body()
        return g, None


class Boom(RuntimeError):
    pass


class Recorder:
    def __init__(self, adapter):
        self.a = adapter
        self.weights = []            # problem number -> (x, dy, sink, weight), kept alive so that ids and addresses stay unique
        self.begin(NO_CAP)

    def begin(self, cap):
        self.a.reset(cap)
        self.event = -1
        self.launches, self.workspaces, self.notified, self.deferred, self.warnings = [], [], [], [], []
        self.by_sink, self.by_id = {}, {}
        self.weights.clear()

    # ---- the stubs ---------------------------------------------------------------------------------------------------------------
    def call(self, name, *args):
        if name == "mrfp_conv_wgrad":
            n, geometry, sinks = 1, args[10], [args[2]]
        elif name == "mrfp_conv_wgrad_grouped":
            n, geometry, sinks = args[3], args[11], list(args[2])
        else:
            raise AssertionError("unexpected entry point %s" % name)
        assert len(sinks) == n
        self.launches.append([self.event, geometry - 1000, n, name, [self.by_sink[s] for s in sinks]])

    def workspace(self, M, N, Q, device, n=1):
        self.workspaces.append([self.event, N - 1000, n])
        return None

    def notify(self, weight):
        self.notified.append(self.by_id[id(weight)])

    # ---- the driver --------------------------------------------------------------------------------------------------------------
    def _state(self):
        self.deferred.append(sorted(self.by_id[i] for i in ops.GRAD_DEFERRED))

    def _step(self, action):
        self.event += 1
        if action == "flush":                # a stage boundary (conv.wgrad_boundary's hook)
            self.a.flush()
        elif action == "raise":
            self._state()
            raise Boom("injected")
        else:
            x, dy, sink, weight = torch.zeros(4), torch.zeros(4), torch.zeros(1), torch.zeros(1)
            k = len(self.weights)
            self.weights.append((x, dy, sink, weight))
            self.by_sink[sink.data_ptr()], self.by_id[id(weight)] = k, k
            self.a.submit(sig(action), x, dy, sink, weight)
        self._state()

    def run_pass(self, actions):
        """one backward pass: the actions (a geometry number = submit one weight gradient of it, "flush", "raise"), then the
        end-of-backward callback as an event of its own"""
        def body():
            for action in actions:
                self._step(action)
            self.event += 1                  # what the engine's callback launches belongs to this event

        t = torch.zeros(1, requires_grad=True)
        try:
            _Pass.apply(t, body).sum().backward()
        except Boom:
            return False
        self._state()
        return True

    def outside(self, what):
        """an event outside any backward pass; the warning it raises, if any, is recorded"""
        self.event += 1
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            what()
        self.warnings += [[self.event, i.category.__name__, str(i.message)] for i in w]
        self._state()

    def end(self):
        return {"events": self.event + 1, "launches": self.launches, "workspaces": self.workspaces, "notified": self.notified,
                "deferred": self.deferred, "warnings": self.warnings,
                "end": {"queued": sum(len(v) for v in self.a.queues().values()), "callback_queued": bool(self.a.callback_queued()),
                        "kinds": [k[6] - 1000 for k in self.a.kinds()], "group_launches": list(conv.WGRAD_GROUP_LAUNCHES)}}


def stage_pattern(r):
    """one singleton head geometry, a stage of six blocks whose three conv positions repeat 6, 5 and 5 times, the stage boundary,
    a singleton tail"""
    actions = [0]
    for block in range(6):
        actions += [1] if block == 0 else [1, 2, 3]
    actions += ["flush", 4]
    assert [actions.count(g) for g in (0, 1, 2, 3, 4)] == [1, 6, 5, 5, 1]
    for _ in range(3):
        r.run_pass(actions)


def group_maximum(r):
    for _ in range(3):
        r.run_pass([0] * (2 * r.group_max + 3))


def byte_cap(r):
    for _ in range(3):
        r.run_pass([1, 2, 3, 1, 2, 3, 1])


def changing_expectation(r):
    for n in (3, 2, 2, 3, 3):
        r.run_pass([0] + [1] * n)


def alternating_kinds(r):
    for i in range(8):
        r.run_pass([0, 2, 2, 2] if i % 2 == 0 else [1, 2, 2])
    for k in range(66):
        r.run_pass([10 + k])


def dead_pass(r):
    full = [0, 1, 1, 2, 1, 2]
    r.run_pass(full)
    r.run_pass(full[:4] + ["raise"])
    r.outside(r.a.backward_failed)
    r.run_pass(full)
    r.run_pass(full[:4] + ["raise"])

    def next_forward_convolution():          # conv2d(), called outside any backward pass, finds the callback flag still set
        if r.a.callback_queued() and not conv._in_backward():
            r.a.drop()
    r.outside(next_forward_convolution)
    r.run_pass(full)


SCENARIOS = [("stage_pattern", NO_CAP, stage_pattern), ("group_maximum", NO_CAP, group_maximum),
             ("byte_cap", int(2.5 * ITEM_BYTES), byte_cap), ("changing_expectation", NO_CAP, changing_expectation),
             ("alternating_kinds", NO_CAP, alternating_kinds), ("dead_pass", NO_CAP, dead_pass)]


def record():
    """{scenario: what it launched, notified and left behind}; conv and ops are left as they were found"""
    a = Adapter()
    r = Recorder(a)
    saved = (conv.call, conv.wgrad_workspace, conv.stream, ops.GRAD_NOTIFY[0], set(ops.GRAD_DEFERRED), list(conv.WGRAD_GROUP_LAUNCHES))
    conv.call, conv.wgrad_workspace, conv.stream, ops.GRAD_NOTIFY[0] = r.call, r.workspace, (lambda: 0), r.notify
    out = {}
    try:
        r.begin(NO_CAP)
        r.run_pass([0])                      # (takes the group maximum from the library, as the first queued gradient does)
        out["group_max"] = r.group_max = a.group_max()
        for name, cap, scenario in SCENARIOS:
            r.begin(cap)
            scenario(r)
            out[name] = r.end()
        r.begin(NO_CAP)
    finally:
        conv.call, conv.wgrad_workspace, conv.stream, ops.GRAD_NOTIFY[0] = saved[:4]
        a.restore()
        ops.GRAD_DEFERRED.update(saved[4])
        conv.WGRAD_GROUP_LAUNCHES.extend(saved[5])
    return out


def main():
    got = record()
    with open(OUT, "w") as f:
        f.write("{" + ",\n ".join("%s: %s" % (json.dumps(k), json.dumps(v, separators=(",", ":"))) for k, v in got.items()) + "}\n")
    print("%s: %s" % (OUT, ", ".join("%s %d launches" % (k, len(v["launches"])) for k, v in got.items() if k != "group_max")))


if __name__ == "__main__":
    main()
