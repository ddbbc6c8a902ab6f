"""What the loss operators of mrfp_amd/ops.py hand to the library, recorded on the GPU: for a fixed seeded case list, every entry
point each public call reaches (forward and backward), with every non-pointer argument by value and every pointer argument as
"null" or "ptr", and the shape, dtype and strides of the returned loss and of the gradient.  Only the public operators and
_lib.HOOK are used, so the script runs unchanged on any commit that has them.

    python tools/record_loss_launches.py                   rewrites tests/golden/loss_launches.json
    python tools/record_loss_launches.py --save PATH       also stores every loss and gradient of the case list (torch.save)
    python tools/record_loss_launches.py --compare A B     two such files, tensor by tensor, as bytes

tests/test_loss_gpu.py replays record() and compares with the file.  The file was written ONCE, by this script, from the commit
before the six autograd classes of the loss operators became one over (score source, criterion); it is the yardstick for that
operator layer and is not to be regenerated from it.

The cases, the smallest at which each path can go wrong: B = 2, scores 3 x 2 upsampled to 9 x 7 (dense logits 2 x C x 9 x 7), C in
{5, 19, 31} (class pads 8, 24, 32), bf16 and fp32, score pitch 32 (fp32 C = 19: pitch != gradient pad, the score gradient is zeroed
first) and one bf16 case at pitch 24 with C = 19 (pitch == pad: not zeroed); cross entropy plain, with `_general=True`, and weights
{none, [C], [B, C]} x smoothing {0, 0.1} x {mean, sum, per-image mean}; soft-NLL on relax_labels(border=1) words with the three
weight forms; ohem_target with min_kept 0 and 20; each dense and fused; at C = 19 once more with image 1 entirely ignored.  The
incoming gradient is 0.7."""
import ctypes
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from mrfp_amd import _lib, ops  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "loss_launches.json")
DEV = "cuda:0"
B, LOW, SIZE = 2, (3, 2), (9, 7)
CLASSES = (5, 19, 31)
DTYPES = (torch.bfloat16, torch.float32)
IGNORE = 255
GSCALE = 0.7
REDUCTIONS = {"mean": dict(), "sum": dict(reduction="sum"), "image_mean": dict(per_image=True)}


def _scores(C, dtype, pitch, seed):
    """-> (dense logits [B,C,9,7], channel-padded scores [B,pitch,3,2]), channels_last on the device, leaves that require grad"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, *SIZE, generator=g) * 3
    P = torch.zeros(B, pitch, *LOW)
    P[:, :C] = torch.randn(B, C, *LOW, generator=g) * 2
    return [t.to(DEV, dtype).contiguous(memory_format=torch.channels_last).requires_grad_(True) for t in (x, P)]


def _labels(C, seed, dead_image):
    g = torch.Generator().manual_seed(seed)
    y = torch.randint(0, C, (B, *SIZE), generator=g)
    y[torch.rand(B, *SIZE, generator=g) < 0.1] = IGNORE
    if dead_image:
        y[1] = IGNORE
    return y.to(DEV)


def _weights(C, seed):
    g = torch.Generator().manual_seed(seed)
    return {"none": None, "shared": (torch.rand(C, generator=g) + 0.5).to(DEV), "rows": (torch.rand(B, C, generator=g) + 0.5).to(DEV)}


def _variant(out, C, dtype, pitch, dead):
    """the cases of one (class count, dtype, score pitch, image 1 ignored or not), appended to out"""
    seed = 1000 * C + 10 * pitch + int(dead)
    x, P = _scores(C, dtype, pitch, seed)
    y, w = _labels(C, seed + 1, dead), _weights(C, seed + 2)
    words = ops.relax_labels(y, C, 1)
    tag = "C%d %s pitch%d%s" % (C, str(dtype)[6:], pitch, " image1_ignored" if dead else "")
    for kind, s in (("dense", x), ("fused", P)):
        if kind == "dense" and pitch != 32:
            continue                      # the pitch belongs to the fused source alone
        up = dict(size=SIZE, channels=C) if kind == "fused" else {}

        def ce(s=s, up=up, **kw):
            if up:
                return ops.upsample_cross_entropy(s, y, SIZE, C, IGNORE, **kw)
            return ops.cross_entropy(s, y, IGNORE, **kw)

        def nll(s=s, up=up, **kw):
            if up:
                return ops.upsample_soft_nll(s, words, SIZE, C, **kw)
            return ops.soft_nll(s, words, C, **kw)

        def add(what, fn, scores):
            out.append(("%s %s %s" % (tag, kind, what), scores, fn))

        add("ce plain", ce, s)
        add("ce general", lambda ce=ce: ce(_general=True), s)
        for wname, wt in w.items():
            for eps in (0.0, 0.1):
                for rname, rkw in REDUCTIONS.items():
                    if (wname, eps, rname) != ("none", 0.0, "mean"):
                        add("ce w=%s eps=%g %s" % (wname, eps, rname),
                            lambda ce=ce, wt=wt, eps=eps, rkw=rkw: ce(weight=wt, label_smoothing=eps, **rkw), s)
            add("soft_nll w=%s" % wname, lambda nll=nll, wt=wt: nll(weight=wt), s)
        for k in (0, 20):
            add("ohem_target min_kept=%d" % k,
                lambda s=s, up=up, k=k: ops.ohem_target(s, y, IGNORE, 0.7, k, want_prob=True, want_state=True, **up), None)


def cases():
    """-> [(name, scores, run)]: run() calls one public operator; scores is the leaf whose gradient belongs to the record (None for
    ohem_target, which has none)"""
    out = []
    for C in CLASSES:
        for dtype in DTYPES:
            _variant(out, C, dtype, 32, False)
            if C == 19:
                _variant(out, C, dtype, 32, True)
                if dtype == torch.bfloat16:
                    _variant(out, C, dtype, 24, False)
    return out


def _meta(t):
    return [list(t.shape), str(t.dtype), list(t.stride())]


def record(save=None):
    """{case: {"calls": [[entry, [argument values, "null" or "ptr" for a pointer]]], "loss": ..., "grad": ...}}; with `save` (a
    dictionary) every returned tensor and gradient is put there on the CPU"""
    pointer = {name: [t is ctypes.c_void_p for t in types] for name, (_, types) in _lib.parse_header().items()}
    calls = []

    def hook(name, args):
        assert len(args) == len(pointer[name]), (name, len(args))
        calls.append([name, [("null" if a is None or a == 0 else "ptr") if p else a for a, p in zip(args, pointer[name])]])

    got = {}
    todo = cases()                       # (relax_labels launches here, before the hook is set)
    saved, _lib.HOOK[0] = _lib.HOOK[0], hook
    try:
        for name, scores, run in todo:
            del calls[:]
            res = run()
            if scores is None:
                tensors = dict(zip(("masked", "prob", "state"), res))
                got[name] = {"calls": list(calls), **{k: _meta(v) for k, v in tensors.items()}}
            else:
                scores.grad = None
                (res * GSCALE).backward()
                tensors = {"loss": res.detach(), "grad": scores.grad}
                got[name] = {"calls": list(calls), "loss": _meta(res), "grad": _meta(scores.grad)}
            if save is not None:
                save.update({"%s: %s" % (name, k): v.detach().cpu() for k, v in tensors.items()})
    finally:
        _lib.HOOK[0] = saved
    return got


def _bytes(t):
    return t.contiguous().reshape(-1).view(torch.uint8)


def compare(path_a, path_b):
    a, b = torch.load(path_a), torch.load(path_b)
    assert list(a) == list(b), "the two files hold different cases"
    equal = [k for k in a if a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and torch.equal(_bytes(a[k]), _bytes(b[k]))]
    nan = sum(1 for k in equal if a[k].is_floating_point() and bool(torch.isnan(a[k]).any()))
    print("%d tensors compared, %d equal as bytes (%d of them hold a NaN)" % (len(a), len(equal), nan))
    for k in a:
        if k not in equal:
            print("DIFFERENT: %s" % k)
    return len(equal) == len(a)


def main():
    argv = sys.argv[1:]
    if argv[:1] == ["--compare"]:
        sys.exit(0 if compare(argv[1], argv[2]) else 1)
    if not torch.cuda.is_available():
        raise _lib.MrfpHipError("record_loss_launches records on the GPU: no device found")
    out, save = OUT, None
    if "--out" in argv:
        out = argv[argv.index("--out") + 1]
    if "--save" in argv:
        save = {}
    got = record(save)
    with open(out, "w") as f:
        f.write("{" + ",\n ".join("%s: %s" % (json.dumps(k), json.dumps(v, separators=(",", ":"))) for k, v in got.items()) + "}\n")
    if save is not None:
        torch.save(save, argv[argv.index("--save") + 1])
    print("%s: %d cases, %d launches%s" % (out, len(got), sum(len(v["calls"]) for v in got.values()),
                                         "" if save is None else ", %d tensors saved" % len(save)))


if __name__ == "__main__":
    main()
