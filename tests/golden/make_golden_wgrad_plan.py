"""Regenerates tests/golden/wgrad_plan.json: the launch plan of every weight-gradient call of the bench step (mrfp_conv_wgrad and
mrfp_conv_wgrad_grouped with their group counts, the Gram call of the whitening path included) and of the weight-gradient tests of
tests/test_conv_gpu.py, in bf16, f16 and fp32, under every weight-gradient switch setting.

The fixture pins what a weight-gradient launch runs -- {kernel, variant, splits, klen, grid} as mrfp_conv_wgrad_plan reports them --
and the bytes the two workspace queries return.  It was recorded from the library as it was BEFORE the launch had one plan
(conv_wgrad.hip's wgrad_run deriving the choice through wgrad_plan / wg3_applicable / wg1_applicable / launch_wgrad): that library
has no plan query, so a print-only export that walks wgrad_run's own calls in wgrad_run's own order -- with launch_wgrad_v recording
the instance, tiles and grid it is about to launch instead of launching -- was added to a scratch build of it (the diff is quoted in
profiles/wgrad_plan.md).  Run against such a build:

    MRFP_HIP_LIB=<scratch .so> python tests/golden/make_golden_wgrad_plan.py [--fn mrfp_dbg_wgrad_choice] [--trace <launch trace>]

--trace: a tools/launch_trace.py file of the bench step (case r101) to take the bench calls from; without it the calls already in
the fixture (taken from such a trace) are kept.  No GPU is needed: the queries are host-only.  The switches are read once per
process, so every setting runs in a child process of its own.  The generator refuses to write a fixture in which a plan needs more slab slots than the workspace
queries grant (splits * count * N * Q * 4 <= bytes): the recorded library satisfied that for every entry and setting.
"""
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "wgrad_plan.json")
F32, BF16, F16 = 0, 1, 2

SETTINGS = [{}, {"MRFP_WGRAD3": "2"}, {"MRFP_WGRAD3": "0"}, {"MRFP_WGRAD1": "2"}, {"MRFP_WGRAD1": "0"}, {"MRFP_WGRAD_BIG": "2"},
            {"MRFP_WGRAD_BIG": "0"}, {"MRFP_WGRAD_DENSE": "0"}, {"MRFP_WGRAD_DMA": "0"}]


def _up(n, m):
    return (n + m - 1) // m * m


def _out(n, k, stride, pad, dil):
    return (n + 2 * pad - dil * (k - 1) - 1) // stride + 1


def bench_calls(trace):
    """[dtype, [B, H, W, C, N, ldn, R, S, Ho, Wo, stride, pad_h, pad_w, dil, count]] of the training step of a launch trace"""
    out = []
    for line in open(trace):
        f = line.split()
        if line.startswith("# training=False"):
            break
        if not f or f[0] not in ("mrfp_conv_wgrad", "mrfp_conv_wgrad_grouped"):
            continue
        if f[0] == "mrfp_conv_wgrad":      # x dy dw ws dtype B H W C Ctrue N ldn R S Ho Wo stride pad_h pad_w dil stream
            count, a = 1, [int(v) for v in f[5:21]]
        else:                              # xs dys dws count ws dtype B ...
            count, a = int(f[4]), [int(v) for v in f[6:22]]
        dtype, B, H, W, C, _ctrue, N, ldn, R, S, Ho, Wo, stride, pad_h, pad_w, dil = a
        out.append([dtype, [B, H, W, C, N, ldn, R, S, Ho, Wo, stride, pad_h, pad_w, dil, count]])
    return out


def test_calls():
    """(B, Cin, H, W, Cout, k, stride, pad, dil, count) of the weight gradients tests/test_conv_gpu.py launches"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_conv_gpu as t
    cases = [c[:9] + (1,) for c in t.CASES]
    for c in t.GROUP_CASES:                                # test_grouped_wgrad_equals_the_single_launches: grouped and single
        c = (c[0], 320 if c[1] == 304 else c[1]) + c[2:]   # (it pads the 304-channel operand to 320)
        cases += [c, c[:9] + (1,)]
    # test_alternative_tile_variants_in_subprocess
    cases += [(B, Cin, H, W, Cout, k, st, pad, dil, 1) for (B, Cin, H, W, Cout, k, pad, dil, st) in
              [(2, 128, 240, 240, 256, 3, 1, 1, 1), (2, 304, 120, 120, 256, 3, 1, 1, 1), (3, 64, 33, 31, 64, 3, 1, 1, 1),
               (2, 256, 48, 40, 512, 1, 0, 1, 1), (4, 128, 32, 32, 128, 3, 1, 1, 2), (4, 256, 32, 32, 512, 1, 0, 1, 2),
               (2, 32, 20, 18, 256, 1, 0, 1, 1), (3, 32, 33, 31, 136, 1, 0, 1, 1), (2, 32, 96, 96, 256, 1, 0, 1, 1)]]
    cases += [(6, 64, 2432, 2432, 64, 1, 1, 0, 1, 1)]      # test_activation_above_the_buffer_descriptor_range (walked in batch ranges)
    # test_accumulator_stationary_3x3_wgrad_in_subprocess (C: the physical channel count there)
    cases += [(B, C, H, W, N, 3, 1, dil, dil, n) for (B, C, H, W, N, dil, n) in
              [(2, 64, 16, 64, 64, 1, 1), (1, 64, 24, 128, 128, 1, 1), (2, 128, 12, 96, 128, 1, 3), (2, 64, 8, 48, 64, 1, 1), (2, 128, 16, 48, 256, 2, 2),
               (2, 64, 20, 64, 128, 2, 1), (2, 320, 12, 64, 256, 1, 1), (3, 64, 40, 192, 64, 1, 1), (5, 128, 40, 64, 128, 1, 7), (4, 256, 48, 48, 256, 1, 22),
               (2, 128, 24, 96, 64, 2, 2), (1, 64, 4, 144, 64, 1, 1), (2, 64, 8, 144, 128, 2, 1), (1, 128, 2, 64, 64, 1, 32), (4, 128, 48, 192, 128, 1, 5),
               (16, 64, 96, 192, 64, 1, 3)]]
    # test_accumulator_stationary_pointwise_wgrad_in_subprocess
    cases += [(B, C, H, W, N, 1, 1, 0, 1, n) for (B, C, H, W, N, n) in
              [(2, 256, 8, 16, 256, 1), (1, 512, 16, 16, 256, 3), (2, 256, 12, 16, 1024, 5), (4, 1024, 48, 48, 256, 22), (2, 256, 10, 16, 256, 1),
               (1, 2048, 8, 8, 512, 2), (1, 256, 4, 8, 256, 1), (4, 256, 48, 48, 1024, 23), (2, 512, 24, 24, 2048, 3)]]
    # test_wgrad_256x128_tile_in_subprocess
    cases += [(4, 256, 48, 48, 1024, 1, 1, 0, 1, 5), (4, 1024, 48, 48, 256, 1, 1, 0, 1, 3), (4, 256, 48, 48, 256, 3, 1, 1, 1, 4), (3, 128, 33, 31, 256, 3, 2, 1, 1, 2),
              (2, 512, 24, 24, 512, 3, 1, 2, 2, 1), (2, 256, 40, 36, 256, 1, 1, 0, 1, 1), (2, 64, 96, 96, 256, 1, 1, 0, 1, 1)]
    # the operator-layer backward of test_long_k_pointwise_kernel and the 3x3 shapes of the weight-stationary forward tests
    cases += [(B, C, H, W, N, 1, 1, 0, 1, 1) for (B, C, H, W, N) in t.PWK_CASES]
    cases += [(B, C, H, W, N, 3, 1, dil, dil, 1) for (B, C, H, W, N, dil, _) in t.C64_CASES + t.C128_CASES]
    return cases


def gram_calls():
    """ops.cross_gram (the Gram matrix of the whitening path: instance_whitening.py, sync_switchwhiten.py): one image per call, the
    activation on both sides -- (H, W, C) of the whitened trunk stages at the bench size and of tests/test_whitening_gpu.py"""
    return [[1, H, W, C, C, C, 1, 1, H, W, 1, 0, 0, 1, 1] for (H, W, C) in
            [(384, 384, 64), (192, 192, 256), (96, 96, 512), (48, 48, 1024), (14, 10, 64), (12, 10, 64), (16, 8, 64), (24, 24, 32)]]


def entries(bench):
    out = [[d, g] for g in gram_calls() for d in (BF16, F16, F32)]
    for dtype, g in bench:                                 # the bench calls as they are, and in the other two activation types
        for d in (dtype, BF16, F16, F32):
            out.append([d, g])
    for (B, Cin, H, W, Cout, k, stride, pad, dil, n) in test_calls():
        for dtype, epc in ((BF16, 8), (F16, 8), (F32, 4)):
            C, ldn = _up(Cin, epc), _up(Cout, epc)
            out.append([dtype, [B, H, W, C, Cout, ldn, k, k, _out(H, k, stride, pad, dil), _out(W, k, stride, pad, dil), stride, pad, pad, dil, n]])
    uniq = []
    for e in out:
        if e not in uniq:
            uniq.append(e)
    return uniq


def _child(path, fn):
    from mrfp_amd import _lib
    L = ctypes.CDLL(_lib.LIBPATH)
    plan = getattr(L, fn)
    plan.restype, plan.argtypes = ctypes.c_int, [ctypes.c_int] + [ctypes.c_int64] * 15 + [ctypes.c_void_p]
    one, grp = L.mrfp_conv_wgrad_ws_bytes, L.mrfp_conv_wgrad_grouped_ws_bytes
    one.restype = grp.restype = ctypes.c_int64
    one.argtypes, grp.argtypes = [ctypes.c_int64] * 3, [ctypes.c_int64] * 4
    res = []
    for dtype, g in json.load(open(path)):
        B, H, W, C, N, ldn, R, S, Ho, Wo, stride, pad_h, pad_w, dil, count = g
        out = (ctypes.c_int64 * 5)()
        if plan(dtype, *g, out) != 0:
            raise SystemExit("plan query failed for %r" % ((dtype, g),))
        M, Q = B * Ho * Wo, R * S * C
        res.append(list(out) + [int(one(M, N, Q)), int(grp(M, N, Q, count))])
    print(json.dumps(res))


def main():
    argv = sys.argv[1:]
    fn = argv[argv.index("--fn") + 1] if "--fn" in argv else "mrfp_conv_wgrad_plan"
    bench = bench_calls(argv[argv.index("--trace") + 1]) if "--trace" in argv else json.load(open(OUT))["bench_calls"]
    distinct = []
    for c in bench:
        if c not in distinct:
            distinct.append(c)
    ents = entries(distinct)
    tmp = OUT + ".entries.tmp"
    json.dump(ents, open(tmp, "w"))
    plans = []
    try:
        for s in SETTINGS:
            env = dict(os.environ, PYTHONPATH=ROOT, **s)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", tmp, fn], env=env, capture_output=True, text=True, check=True)
            plans.append(json.loads(r.stdout.strip().splitlines()[-1]))
    finally:
        os.remove(tmp)
    for s, plan in zip(SETTINGS, plans):
        for (dtype, g), p in zip(ents, plan):
            need = p[2] * g[14] * g[4] * (g[6] * g[7] * g[3]) * 4      # splits * count * N * Q * 4
            if need > p[6] or (g[14] == 1 and need > p[5]):
                raise SystemExit("the workspace does not cover the plan: %r %r %r" % (s, (dtype, g), p))
    # one line per entry: [dtype, geometry + count, [[kernel, variant, splits, klen, grid, ws_bytes, grouped_ws_bytes] under setting 0, 1, ...]]
    rows = [json.dumps([d, g, [p[i] for p in plans]]) for i, (d, g) in enumerate(ents)]
    with open(OUT, "w") as f:
        f.write('{"settings": %s,\n "bench_calls": %s,\n "entries": [\n%s\n]}\n' % (json.dumps(SETTINGS), json.dumps(distinct), ",\n".join(rows)))
    print("%s: %d bench calls (%d distinct geometries), %d entries x %d settings" % (
        OUT, len(distinct), len({tuple(g[:14]) for _, g in distinct}), len(ents), len(SETTINGS)))


if __name__ == "__main__":
    if len(sys.argv) > 3 and sys.argv[1] == "--child":
        _child(sys.argv[2], sys.argv[3])
    else:
        main()
