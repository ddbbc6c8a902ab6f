"""Regenerates tests/golden/conv_plan.json: the statistics layout of every forward / dgrad convolution shape the bench workload and
tests/test_conv_gpu.py launch, under every kernel-selection switch setting the GPU tests use.

The fixture pins the launch plan of mrfp_conv_fwd / mrfp_conv_fwd_wstats (which kernel, and with it how many statistics row blocks
of how many output rows the epilogue writes).  It was recorded with the five separate queries the C ABI had before
mrfp_conv_stats_layout replaced them (mrfp_conv_stats_blocks, _stats_block_rows, _stats_rows, _stats_final_first,
_stats_final_count); tests/test_conv_plan_cpu.py checks that the one query reproduces every number.  Run it against a library
that still exports those five (MRFP_HIP_LIB=<path> python tests/golden/make_golden_conv_plan.py).  No GPU is needed: the
queries are host-only.  The switches are read once per process, so every setting runs in a child process of its own.
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "conv_plan.json")
F32, BF16 = 0, 1

# the switch settings of tests/test_conv_gpu.py (default; its child processes)
SETTINGS = [
    {},
    {"MRFP_CONV_PW": "0", "MRFP_WGRAD_DENSE": "0"},
    {"MRFP_CONV_T96": "2", "MRFP_CONV_C64": "0"},
    {"MRFP_CONV_T192": "2", "MRFP_CONV_RR": "0", "MRFP_CONV_C64": "0"},
    {"MRFP_CONV_PW32": "1"},
    {"MRFP_CONV_RR": "3", "MRFP_CONV_C64": "0"},
    {"MRFP_CONV_C128": "2"},
]


def _up(n, m):
    return (n + m - 1) // m * m


def _fwd_and_dgrad(B, Cin, H, W, Cout, k, stride, pad, dil, epc):
    """mrfp_conv_fwd geometry [B, H, W, C, N, ldy, R, S, Ho, Wo, stride, pad_h, pad_w, dil, sstride] of conv.py's forward launch and
    of its dgrad launch (the same kernel on dy with the flipped pack; sstride = the forward stride)"""
    C, N = _up(Cin, epc), _up(Cout, epc)
    Ho, Wo = (H + 2 * pad - dil * (k - 1) - 1) // stride + 1, (W + 2 * pad - dil * (k - 1) - 1) // stride + 1
    q = dil * (k - 1) - pad
    return [[B, H, W, C, N, N, k, k, Ho, Wo, stride, pad, pad, dil, 1], [B, Ho, Wo, N, C, C, k, k, H, W, 1, q, q, dil, stride]]


def _test_cases():
    """(B, Cin, H, W, Cout, k, stride, pad, dil) of the convolutions tests/test_conv_gpu.py runs"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_conv_gpu as t
    cases = [c[:9] for c in t.CASES]
    cases += [(B, Cin, H, W, Cout, k, 1, k // 2, 1) for (B, Cin, H, W, Cout, k) in
              [(2, 64, 20, 18, 128, 3), (3, 128, 33, 31, 64, 1), (2, 128, 240, 240, 256, 3), (2, 128, 48, 40, 256, 1), (4, 256, 48, 48, 1024, 1)]]
    cases += [(B, Cin, H, W, Cout, k, st, pad, dil) for (B, Cin, H, W, Cout, k, pad, dil, st) in
              [(2, 128, 240, 240, 256, 3, 1, 1, 1), (2, 304, 120, 120, 256, 3, 1, 1, 1), (3, 64, 33, 31, 64, 3, 1, 1, 1),
               (2, 256, 48, 40, 512, 1, 0, 1, 1), (4, 128, 32, 32, 128, 3, 1, 1, 2), (4, 256, 32, 32, 512, 1, 0, 1, 2),
               (2, 32, 20, 18, 256, 1, 0, 1, 1), (3, 32, 33, 31, 136, 1, 0, 1, 1), (2, 32, 96, 96, 256, 1, 0, 1, 1)]]
    cases += [(B, C, H, W, N, k, 1, pad, pad if k == 3 else 1) for (B, C, H, W, N, k, pad) in
              [(4, 256, 192, 192, 128, 1, 0), (4, 256, 48, 48, 1024, 1, 0), (3, 128, 96, 96, 512, 1, 0), (4, 256, 48, 48, 256, 3, 1),
               (2, 512, 48, 48, 512, 3, 2)]]
    cases += [(B, Cin, H, W, Cout, 3, 1, pad, pad) for (B, Cin, H, W, Cout, pad) in
              [(2, 128, 192, 192, 256, 1), (2, 64, 96, 96, 128, 1), (3, 256, 48, 48, 256, 1), (2, 128, 48, 48, 128, 2), (1, 64, 384, 384, 128, 1),
               (2, 64, 192, 384, 192, 1), (4, 64, 48, 16, 128, 1), (2, 192, 96, 192, 320, 1), (1, 64, 24, 32, 128, 2),
               (1, 128, 384, 384, 64, 1), (2, 64, 192, 192, 64, 1), (3, 64, 96, 96, 64, 2), (2, 64, 48, 48, 64, 1), (2, 128, 192, 192, 48, 1),
               (1, 64, 384, 384, 64, 2)]]
    cases += [(B, C, H, W, N, 3, 1, dil, dil) for (B, C, H, W, N, dil, _) in t.C64_CASES + t.C128_CASES]
    cases += [(B, C, H, W, N, 1, 1, 0, 1) for (B, C, H, W, N) in t.PWK_CASES]
    return cases


def entries():
    """[dtype, geometry (15 values), wstats]"""
    out = []
    for name, a in json.load(open(os.path.join(ROOT, "tools", "bench_conv_shapes.json"))):
        if name == "mrfp_conv_fwd":
            out.append([BF16, a, 0])
            # the HRFP 3x3 layers run with resize-weighted statistics (mrfp_conv_fwd_wstats: stride 1, no sstride argument)
            if a[6] * a[7] > 1 and a[10] == 1 and a[14] == 1 and a[1] >= 192:
                out.append([BF16, a, 1])
    for c in sorted(set(_test_cases())):
        for dtype, epc in ((BF16, 8), (F32, 4)):
            for g in _fwd_and_dgrad(*c, epc):
                out.append([dtype, g, 0])
    uniq = []
    for e in out:
        if e not in uniq:
            uniq.append(e)
    return uniq


def _child(path):
    import ctypes
    from mrfp_amd import _lib
    L = _lib.lib()
    for f in ("mrfp_conv_stats_blocks", "mrfp_conv_stats_block_rows", "mrfp_conv_stats_rows", "mrfp_conv_stats_final_first",
              "mrfp_conv_stats_final_count"):
        getattr(L, f).restype = ctypes.c_int64
    res = []
    for dtype, g, wstats in json.load(open(path)):
        B, H, W, C, N, ldy, R, S, Ho, Wo, stride, pad_h, pad_w, dil, sstride = g
        q = (dtype, B, H, W, C, N, R, S, Ho, Wo, stride, pad_h, pad_w, dil, sstride)
        nblk = int(L.mrfp_conv_stats_blocks(*q))
        res.append([nblk, int(L.mrfp_conv_stats_block_rows(*q)), int(L.mrfp_conv_stats_rows(nblk)),
                    int(L.mrfp_conv_stats_final_first(nblk)), int(L.mrfp_conv_stats_final_count(nblk))])
    print(json.dumps(res))


def main():
    ents = entries()
    tmp = OUT + ".entries.tmp"
    json.dump(ents, open(tmp, "w"))
    layouts = []
    try:
        for s in SETTINGS:
            env = dict(os.environ, PYTHONPATH=ROOT, **s)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", tmp], env=env, capture_output=True, text=True,
                               check=True)
            layouts.append(json.loads(r.stdout.strip().splitlines()[-1]))
    finally:
        os.remove(tmp)
    # one line per entry: [dtype, geometry, wstats, [layout under setting 0, 1, ...]] with layout = [row_blocks, block_rows,
    # alloc_rows, final_first, final_count]
    rows = [json.dumps([d, g, w, [lay[i] for lay in layouts]]) for i, (d, g, w) in enumerate(ents)]
    with open(OUT, "w") as f:
        f.write('{"settings": %s,\n "entries": [\n%s\n]}\n' % (json.dumps(SETTINGS), ",\n".join(rows)))
    print("%s: %d entries x %d settings" % (OUT, len(ents), len(SETTINGS)))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        _child(sys.argv[2])
    else:
        main()
