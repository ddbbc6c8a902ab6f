"""No-GPU check of the weight-gradient launch plan: mrfp_conv_wgrad_plan and the two workspace queries reproduce, for every
weight-gradient call of the bench step (single and grouped, the Gram call of the whitening path), and for every weight-gradient shape
of tests/test_conv_gpu.py, in bf16, f16 and fp32 under every weight-gradient switch, what the library chose before the launch had one
plan (tests/golden/wgrad_plan.json, tests/golden/make_golden_wgrad_plan.py).  A changed number means a launch moved to another kernel,
split or grid -- or that a launch would write slab slots past the workspace its caller sized."""
import json
import os
import subprocess
import sys

import pytest

from mrfp_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "wgrad_plan.json")
SETTINGS = json.load(open(GOLDEN))["settings"]

# The training step of a `tools/launch_trace.py r101` run (the bench step) issues 36 distinct weight-gradient calls of 36 distinct
# geometries: 24 mrfp_conv_wgrad and 12 mrfp_conv_wgrad_grouped with the group counts below.  The fixture has 414 entries.
BENCH_CALLS, BENCH_GEOMETRIES, ENTRIES = 36, 36, 414
BENCH_GROUP_COUNTS = [2, 2, 3, 3, 3, 3, 3, 3, 4, 22, 22, 23]

# (the switches are read once per process: one child per setting)
_CHILD = r"""
import ctypes, json, sys
from mrfp_amd import _lib
L = _lib.lib()
out = []
for dtype, g in json.load(open(sys.argv[1])):
    B, H, W, C, N, ldn, R, S, Ho, Wo, stride, pad_h, pad_w, dil, count = g
    plan = (ctypes.c_int64 * 5)()
    rc = L.mrfp_conv_wgrad_plan(dtype, *g, plan)
    M, Q = B * Ho * Wo, R * S * C
    out.append((list(plan) if rc == 0 else [L.mrfp_last_error().decode()])
               + [int(L.mrfp_conv_wgrad_ws_bytes(M, N, Q)), int(L.mrfp_conv_wgrad_grouped_ws_bytes(M, N, Q, count))])
print(json.dumps(out))
"""


@pytest.fixture(scope="module")
def golden(tmp_path_factory):
    build.build()
    gold = json.load(open(GOLDEN))
    path = tmp_path_factory.mktemp("wgrad_plan") / "entries.json"
    path.write_text(json.dumps([e[:2] for e in gold["entries"]]))
    return gold, str(path)


def test_fixture_covers_the_bench_step(golden):
    """Every weight-gradient call of the traced bench step, single or grouped with its group count, is an entry, in all three
    activation types; the fixture's call list has the counts of the trace it was taken from."""
    gold, _ = golden
    calls = gold["bench_calls"]
    assert len(calls) == BENCH_CALLS and len({tuple(g[:14]) for _, g in calls}) == BENCH_GEOMETRIES
    assert sorted(g[14] for _, g in calls if g[14] > 1) == BENCH_GROUP_COUNTS and sum(1 for _, g in calls if g[14] == 1) == 24
    have = {(d, tuple(g)) for d, g, _ in gold["entries"]}
    for _, g in calls:
        for d in (0, 1, 2):
            assert (d, tuple(g)) in have, (d, g)
    assert len(gold["entries"]) == ENTRIES >= BENCH_GEOMETRIES


@pytest.mark.parametrize("setting", range(len(SETTINGS)), ids=[",".join("%s=%s" % kv for kv in s.items()) or "default" for s in SETTINGS])
def test_plan_and_workspace_match_the_pinned_choice(golden, setting):
    gold, path = golden
    extra = gold["settings"][setting]
    env = dict(os.environ, PYTHONPATH=ROOT, **extra)
    r = subprocess.run([sys.executable, "-c", _CHILD, path], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert len(got) == len(gold["entries"]) == ENTRIES
    # {kernel, variant, splits, klen, grid} and both byte counts: exact
    bad = [(d, g, e[setting], mine) for (d, g, e), mine in zip(gold["entries"], got) if e[setting] != mine]
    assert not bad, (extra, len(bad), bad[:5])
    # the workspace covers the plan: splits * count * N * Q * 4 <= bytes (the single query too where the call is a single one)
    for (d, g, _), (kernel, variant, splits, klen, grid, ws_one, ws_grouped) in zip(gold["entries"], got):
        B, H, W, C, N, ldn, R, S, Ho, Wo, stride, pad_h, pad_w, dil, count = g
        need = splits * count * N * R * S * C * 4
        assert splits >= 1 and need <= ws_grouped and (count > 1 or need <= ws_one), (extra, d, g, splits, ws_one, ws_grouped)


def test_single_workspace_is_the_grouped_one_of_one_problem(golden):
    import ctypes
    from mrfp_amd import _lib
    L = _lib.lib()
    for M, N, Q in [(36864, 256, 2304), (16 * 384 * 384, 64, 576), (36864, 19, 256), (36864, 2048, 1024), (100, 8, 8)]:
        assert L.mrfp_conv_wgrad_ws_bytes(M, N, Q) == L.mrfp_conv_wgrad_grouped_ws_bytes(M, N, Q, 1) > 0
    assert L.mrfp_conv_wgrad_plan.argtypes[-1] is ctypes.c_void_p


def test_plan_query_refuses_what_the_launch_refuses(golden):
    import ctypes
    from mrfp_amd import _lib
    L = _lib.lib()
    out = (ctypes.c_int64 * 5)()
    ok = (_lib.BF16, 2, 8, 8, 64, 64, 64, 3, 3, 8, 8, 1, 1, 1, 1)
    assert L.mrfp_conv_wgrad_plan(*ok, 1, out) == 0 and out[2] >= 1
    assert L.mrfp_conv_wgrad_plan(_lib.BF16, 2, 8, 8, 20, 64, 64, 3, 3, 8, 8, 1, 1, 1, 1, 1, out) != 0      # 20 bf16 != 16-byte chunks
    assert b"conv_wgrad" in L.mrfp_last_error()
    assert L.mrfp_conv_wgrad_plan(*ok, 33, out) != 0 and L.mrfp_conv_wgrad_plan(*ok, 0, out) != 0          # group limit
    assert L.mrfp_conv_wgrad_plan(7, *ok[1:], 1, out) != 0 and b"dtype" in L.mrfp_last_error()
    assert L.mrfp_conv_wgrad_plan(*ok, 1, None) != 0
    # an activation above one buffer range may not be grouped (the launch walks a single one in batch ranges)
    big = (_lib.BF16, 6, 2432, 2432, 64, 64, 64, 1, 1, 2432, 2432, 1, 0, 0, 1)
    assert L.mrfp_conv_wgrad_plan(*big, 1, out) == 0 and L.mrfp_conv_wgrad_plan(*big, 2, out) != 0
