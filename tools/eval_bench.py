"""Eval-forward throughput, unfolded against folded (mrfp_amd/inference.py), bf16:
    ResNet-101 MRFPPlus at 16 x 768 x 768 and at 1 x 1024 x 2048, DeepMobileNetV3PlusD at 16 x 768 x 768.
One JSON line per (case, mode): images/s (median over --steps forwards timed with device events, after --warmup), the entry-point
launches of one forward, and -- folded -- the activation bytes the removed apply passes would have moved, from the shapes:
2 x elements x element size per folded norm (one read and one write of the convolution's output).

    python tools/eval_bench.py [--steps 10] [--warmup 3] [--cases r101_768,r101_1024x2048,mnv2_768] [--out out/eval_bench.json]
"""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = {"r101_768": ("mrfp-r101", 16, 768, 768), "r101_1024x2048": ("mrfp-r101", 1, 1024, 2048), "mnv2_768": ("mnv2", 16, 768, 768)}


def build(kind):
    from mrfp_amd import deepv3, synth
    from mrfp_amd.network import deepv3 as ndv3
    with contextlib.redirect_stdout(io.StringIO()):
        m = deepv3.MRFPPlus(19, trunk="resnet-101") if kind == "mrfp-r101" else ndv3.DeepMobileNetV3PlusD(None, 19, None, None)
    m.load_state_dict(synth.synth_state_dict(synth.spec_of(m.state_dict()), seed=0))
    return m.cuda().eval()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--out", default=os.path.join(os.environ.get("MRFP_OUT", "out"), "eval_bench.json"))
    a = ap.parse_args()
    from mrfp_amd import _lib, synth
    from mrfp_amd.config import cfg
    from mrfp_amd.inference import fold_norms, foldable_pairs
    cfg.MODEL.ACT_DTYPE = torch.bfloat16
    rows = []
    for case in a.cases.split(","):
        kind, B, H, W = CASES[case]
        m = build(kind)
        x = synth.synth_batch(B, H, W, seed=1)[0].cuda()
        folded_norms = {id(n) for _, n, _, _ in foldable_pairs(m)}
        for mode in ("unfolded", "folded", "unfolded", "folded"):          # interleaved: each mode twice
            ctx = fold_norms(m) if mode == "folded" else contextlib.nullcontext()
            with torch.no_grad(), ctx:
                for _ in range(a.warmup):
                    m(x, training=False)
                calls, removed, x_esz = [], [0], 2          # bf16 activations
                # launches and removed bytes of ONE forward: every folded norm's convolution output, read + written by the apply pass
                arg = _lib.ARG_NAMES["mrfp_conv_fwd_act"]
                ia = {k: arg.index(k) for k in ("B", "Ho", "Wo", "ldy")}
                darg = _lib.ARG_NAMES["mrfp_dwconv_fwd_act"]
                da = {k: darg.index(k) for k in ("B", "Ho", "Wo", "Cp")}

                def hook(name, args):
                    calls.append(name)
                    if name == "mrfp_conv_fwd_act":
                        removed[0] += 2 * args[ia["B"]] * args[ia["Ho"]] * args[ia["Wo"]] * args[ia["ldy"]] * x_esz
                    elif name == "mrfp_dwconv_fwd_act":
                        removed[0] += 2 * args[da["B"]] * args[da["Ho"]] * args[da["Wo"]] * args[da["Cp"]] * x_esz
                _lib.HOOK[0] = hook
                try:
                    m(x, training=False)
                finally:
                    _lib.HOOK[0] = None
                times = []
                for _ in range(a.steps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    m(x, training=False)
                    e1.record()
                    e1.synchronize()
                    times.append(e0.elapsed_time(e1))
            med = statistics.median(times)
            r = {"case": case, "mode": mode, "batch": B, "size": [H, W], "dtype": "bf16", "ms_median": round(med, 3),
                 "ms_min": round(min(times), 3), "ms_max": round(max(times), 3), "images_per_s": round(B / med * 1e3, 2),
                 "launches": len(calls), "norm_launches": sum(1 for c in calls if c in ("mrfp_bn_eval_coef",) or c.startswith("mrfp_affine_fwd")),
                 "folded_norms": len(folded_norms) if mode == "folded" else 0,
                 "removed_activation_bytes": int(removed[0]) if mode == "folded" else 0}
            rows.append(r)
            print(json.dumps(r), flush=True)
        del m, x
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(rows, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
