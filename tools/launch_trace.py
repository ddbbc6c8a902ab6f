"""The C-ABI calls of one seeded training step (after two warm-up steps) and of one training=False forward, one line per call:
the entry point, then every argument -- pointers reduced to null / non-null, integers and floats printed exactly.  Two builds
of the operator layer that issue the same launches write the same file (`diff` prints nothing); pointing both at one library
build with MRFP_HIP_LIB compares the Python layer alone.  The file ends with the losses and a checksum of every gradient.

    python tools/launch_trace.py CASE OUT        CASE one of: r101 r50_f32 wrn38 mbv2 mbv2_f32 r101_fold
"""
import contextlib
import ctypes
import io
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mrfp_amd import _lib, deepv3, synth  # noqa: E402
from mrfp_amd.config import cfg  # noqa: E402

#        case: (model, trunk, dtype, batch, size)
CASES = {"r101": ("mrfp", "resnet-101", torch.bfloat16, 16, 768),
         "r50_f32": ("mrfp", "resnet-50", torch.float32, 4, 192),
         "wrn38": ("mrfp", "wider_resnet38_a2", torch.bfloat16, 2, 128),
         "mbv2": ("mbv2", None, torch.bfloat16, 16, 768),
         "mbv2_f32": ("mbv2", None, torch.float32, 2, 128),
         "r101_fold": ("mrfp", "resnet-101", torch.bfloat16, 16, 768)}


def tracer(out):
    protos = _lib.parse_header()

    def fmt(v, ctype):
        if ctype is ctypes.c_void_p:
            if isinstance(v, ctypes.Array):
                return "array[%d]" % len(v)
            return "ptr" if v else "null"
        return repr(float(v)) if ctype is ctypes.c_float else str(int(v))

    def hook(name, args):
        out.write(name + " " + " ".join(fmt(v, t) for v, t in zip(args, protos[name][1])) + "\n")
    return hook


def checksum(t):
    t = t.detach().double()
    return "%.17g %.17g" % (t.sum().item(), t.abs().sum().item())


def main():
    case, path = sys.argv[1], sys.argv[2]
    kind, trunk, dtype, B, S = CASES[case]
    cfg.MODEL.ACT_DTYPE = dtype
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    crit = torch.nn.CrossEntropyLoss(ignore_index=255)
    with contextlib.redirect_stdout(io.StringIO()):
        if kind == "mrfp":
            model = deepv3.MRFPPlus(19, trunk=trunk, criterion=crit)
        else:
            from mrfp_amd.network import deepv3 as zoo
            model = zoo.DeepMobileNetV3PlusD(None, 19, crit, crit)
    model.load_state_dict(synth.synth_state_dict(synth.spec_of(model.state_dict()), seed=0))
    model = model.to(dev).train()
    x, y = synth.synth_batch(B, S, S, seed=1)
    x, y = x.to(dev), y.to(dev)
    if kind == "mrfp":
        from mrfp_amd.harness import Trainer
        model.rng = deepv3.InjectedRandom((True, True, True), None, reinit=True)      # NP+ and HRFP on, HRFP re-drawn
        trainer = Trainer(model)

        def step():
            return [trainer.step(x, y)]

        def evaluate():
            return model(x, training=False)
    else:
        def step():
            model.zero_grad(set_to_none=True)
            l1, l2 = model(x, gts=y)
            (l1 + l2).backward()
            return [l1, l2]

        def evaluate():
            return model(x)
    _lib.lib()
    with open(path, "w") as out:
        hook = tracer(out)
        if case != "r101_fold":
            for _ in range(2):
                step()
            torch.cuda.synchronize()
            out.write("# training step\n")
            _lib.HOOK[0] = hook
            try:
                losses = step()
            finally:
                _lib.HOOK[0] = None
            torch.cuda.synchronize()
            out.write("# results\n")
            for i, l in enumerate(losses):
                out.write("loss%d %.17g\n" % (i, float(l.detach())))
            for k, p in model.named_parameters():
                if p.grad is not None:
                    out.write("grad %s %s\n" % (k, checksum(p.grad)))
        model.eval()
        fold = contextlib.nullcontext()
        if case == "r101_fold":
            from mrfp_amd import inference
            fold = inference.fold_norms(model)
        out.write("# training=False forward\n")
        with torch.no_grad(), fold:
            _lib.HOOK[0] = hook
            try:
                logits = evaluate()
            finally:
                _lib.HOOK[0] = None
        torch.cuda.synchronize()
        out.write("# results\nlogits %s\n" % checksum(logits[0] if isinstance(logits, (tuple, list)) else logits))


if __name__ == "__main__":
    main()
