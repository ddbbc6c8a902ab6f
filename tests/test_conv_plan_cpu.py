"""No-GPU check of the convolution launch plan: mrfp_conv_stats_layout reproduces, for every forward / dgrad shape of the bench
workload and of tests/test_conv_gpu.py under every switch setting the GPU tests use, the statistics layout the library reported
before the plan had one source (tests/golden/conv_plan.json, tests/golden/make_golden_conv_plan.py).  The layout follows from the
kernel choice, so a changed number means a launch moved to another kernel or writes rows past the buffer its caller sized."""
import json
import os
import subprocess
import sys

import pytest

from mrfp_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "conv_plan.json")
SETTINGS = json.load(open(GOLDEN))["settings"]

# (the switches are read once per process: one child per setting)
_CHILD = r"""
import ctypes, json, sys
from mrfp_amd import _lib
L = _lib.lib()
out = []
for dtype, g, wstats in json.load(open(sys.argv[1])):
    lay = (ctypes.c_int64 * 5)()
    rc = L.mrfp_conv_stats_layout(dtype, *g, wstats, lay)
    out.append(list(lay) if rc == 0 else L.mrfp_last_error().decode())
    if not wstats:      # (the block-height query: a dense, unweighted launch -- every entry here has ldy = N)
        out[-1].append(int(L.mrfp_conv_stats_block_rows(dtype, *g[:5], *g[6:])))
print(json.dumps(out))
"""


@pytest.fixture(scope="module")
def golden(tmp_path_factory):
    build.build()
    gold = json.load(open(GOLDEN))
    path = tmp_path_factory.mktemp("conv_plan") / "entries.json"
    path.write_text(json.dumps([e[:3] for e in gold["entries"]]))
    return gold, str(path)


@pytest.mark.parametrize("setting", range(len(SETTINGS)), ids=[",".join("%s=%s" % kv for kv in s.items()) or "default" for s in SETTINGS])
def test_stats_layout_matches_the_pinned_plan(golden, setting):
    gold, path = golden
    extra = gold["settings"][setting]
    env = dict(os.environ, PYTHONPATH=ROOT, **extra)
    r = subprocess.run([sys.executable, "-c", _CHILD, path], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = json.loads(r.stdout.strip().splitlines()[-1])
    assert len(got) == len(gold["entries"]) >= 300
    want = [e[setting] + ([] if w else [e[setting][1]]) for (d, g, w, e) in gold["entries"]]
    bad = [(d, g, w, x, mine) for (d, g, w, e), x, mine in zip(gold["entries"], want, got) if x != mine]
    assert not bad, (extra, len(bad), bad[:5])


def test_stats_layout_refuses_bad_geometry(golden):
    import ctypes
    from mrfp_amd import _lib
    L = _lib.lib()
    lay = (ctypes.c_int64 * 5)()
    assert L.mrfp_conv_stats_layout(_lib.BF16, 2, 8, 8, 20, 64, 64, 3, 3, 8, 8, 1, 1, 1, 1, 1, 0, lay) != 0      # 20 bf16 != 16-byte chunks
    assert b"conv_fwd" in L.mrfp_last_error()
    assert L.mrfp_conv_stats_layout(_lib.BF16, 2, 8, 8, 64, 64, 64, 3, 3, 8, 8, 1, 1, 1, 1, 1, 0, None) != 0
