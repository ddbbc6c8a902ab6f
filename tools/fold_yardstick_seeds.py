"""The yardstick of the folded bf16 fidelity bar (tests/test_fold_gpu.py, profiles/fold_eval.md): over several seeds -- weights AND
batch re-drawn per seed -- the distance of the UNFOLDED bf16 eval logits to the unfolded fp32 logits (e_plain) and of the FOLDED bf16
logits to the same fp32 logits (e_fold), relative L2, MRFPPlus('resnet-50') at 2 x 256 x 256.  Prints one JSON line per seed and a
summary: the worst e_fold / e_plain ratio, the seed-to-seed spread of e_plain, (max - min) / mean, and their sum -- the k of
`e_fold <= k * e_plain`.

    python tools/fold_yardstick_seeds.py [--seeds 8] [--out out/fold_yardstick.json]
"""
import argparse
import contextlib
import io
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=8)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(os.environ.get("MRFP_OUT", "out"), "fold_yardstick.json"))
    a = ap.parse_args()
    from mrfp_amd import deepv3, synth
    from mrfp_amd.config import cfg
    from mrfp_amd.inference import fold_norms

    def model(dtype, seed):
        cfg.MODEL.ACT_DTYPE = dtype
        with contextlib.redirect_stdout(io.StringIO()):
            m = deepv3.MRFPPlus(19)
        m.load_state_dict(synth.synth_state_dict(synth.spec_of(m.state_dict()), seed=seed))
        return m.cuda().eval()

    def l2(p, q):
        p, q = p.double(), q.double()
        return ((p - q).pow(2).sum().sqrt() / q.pow(2).sum().sqrt()).item()

    rows = []
    with torch.no_grad():
        for seed in range(a.seeds):
            x = synth.synth_batch(2, a.size, a.size, seed=100 + seed)[0].cuda()
            ref = model(torch.float32, seed)(x, training=False)
            m = model(torch.bfloat16, seed)
            plain = m(x, training=False)
            with fold_norms(m):
                folded = m(x, training=False)
            r = {"seed": seed, "e_plain": l2(plain, ref), "e_fold": l2(folded, ref),
                 "argmax_agree": (plain.argmax(1) == folded.argmax(1)).float().mean().item()}
            r["ratio"] = r["e_fold"] / r["e_plain"]
            rows.append(r)
            print(json.dumps(r), flush=True)
    cfg.MODEL.ACT_DTYPE = torch.float32
    ep = [r["e_plain"] for r in rows]
    summary = {"worst_ratio": max(r["ratio"] for r in rows), "e_plain_spread": (max(ep) - min(ep)) / (sum(ep) / len(ep)),
               "e_plain_mean": sum(ep) / len(ep), "seeds": a.seeds}
    summary["k"] = summary["worst_ratio"] + summary["e_plain_spread"]
    print(json.dumps({"summary": summary}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump({"rows": rows, "summary": summary}, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
