"""No-GPU check of the weight-pack cache policy of mrfp_amd/conv.py (get_pack, repack_all, repack_weights, prebuild_repack_tables,
get_folded_pack, fold_packs_batched, invalidate_packs, the death of a Parameter): the driver of tools/record_pack_cache.py is replayed
on CPU Parameters with the launches stubbed out, and every scenario must equal tests/golden/pack_cache.json event by event -- recorded
once, with the same driver, from commit 28e6e78, before the cache got per-weight records, named keys and one stamp function per pack
kind.  A difference is a pack that was wrongly judged fresh (a step that silently runs on last step's weights), one that is packed
twice, a buffer or a job table that was reallocated (captured graphs hold their addresses), or a launch with other arguments.

What the CPU cannot show: with CPU tensors get_pack never asks about graph capture (tests/test_harness_gpu.py holds that rule), and
the whole-set refold skips weights that are not on a GPU (tests/test_fold_gpu.py)."""
import json
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "pack_cache.json")
SCENARIOS = ["lazy", "epoch_and_batched", "job_table", "explicit_list", "folded", "lifetime"]
BF16, F32 = 1, 0                             # _lib.BF16, _lib.F32 as the launches carry them


def _module_state():
    from mrfp_amd import conv, ops
    return (conv.call, conv.stream, torch.cuda.is_current_stream_capturing, torch.empty, dict(conv._PACKS), dict(conv._BATCH),
            dict(conv._REPACK_LISTS), list(conv._FOLD_SETS), list(conv.FOLD_PACK_LAUNCHES), list(conv._EPOCH), list(ops.RUNNING_STATS_EPOCH))


@pytest.fixture(scope="module")
def recorded():
    from tools import record_pack_cache as rec
    before = _module_state()
    got = json.loads(json.dumps(rec.record()))
    assert _module_state() == before         # the recorder leaves the modules as it found them
    return json.load(open(GOLDEN)), got


def _launches(events, name):
    return [c for e in events for c in e["calls"] if c[0] == name]


def test_the_fixture_holds_every_scenario(recorded):
    gold, got = recorded
    assert list(gold) == list(got) == SCENARIOS
    # (facts read off the policy, not measurements)
    lazy = gold["lazy"]
    assert [len(e["calls"]) for e in lazy[:3]] == [1, 0, 1]
    assert {k: v["wd_zero"] for k, v in lazy[-1]["packs"].items()} == {"w3.bf16": False, "w3.f32": False, "w3.bf16.c16": True,
                                                                       "w1+b.bf16": False, "w1.bf16": False, "whalf.bf16": False}
    assert all(e["packs"]["w1+b.bf16"]["bias_current"] == (e["event"] != "in-place update of b1: only the pack with the bias is stale")
               for e in lazy if "w1+b.bf16" in e["packs"])
    explicit = gold["explicit_list"]
    marked = [e for e in explicit if e["event"].startswith("repack_weights():")][0]["packs"]
    assert {k for k, v in marked.items() if not v["fresh"]} == {"w7.bf16", "w1.bf16", "w3.fold"}      # 7x7, bias mismatch, folded
    assert marked["w1+b.bf16"]["bias_current"]
    assert explicit[-1]["lists"] == ["hrfp"] and explicit[-2]["lists"] == ["gone", "hrfp"]
    folded = gold["folded"]
    assert sum(1 for e in folded if e["event"] == "... refolds") == 9 and all(len(e["calls"]) == 1 for e in folded if e["event"] == "... refolds")
    assert folded[-1]["packs"]["wdw.fold"]["wf_dtype"] == "torch.float32"
    assert [e["note"] for e in folded[-3:]] == [
        "MrfpHipError: folded inference: norm weight must be a contiguous fp32 tensor (got torch.float16)",
        "MrfpHipError: folded inference: weight must be a contiguous fp32 tensor (got torch.float32)",
        "MrfpHipError: folded inference: the BatchNorm has no running statistics"]
    assert [e["weights"] for e in gold["lifetime"]] == [3, 2, 1, 0]


@pytest.mark.parametrize("scenario", SCENARIOS)
def test_pack_cache_equals_the_recorded_one(recorded, scenario):
    gold, got = recorded
    want, mine = gold[scenario], got[scenario]
    assert [e["event"] for e in mine] == [e["event"] for e in want]
    for a, b in zip(mine, want):
        for what in ("calls", "packs", "tables", "lists", "fold_launches", "weights", "note"):
            assert a.get(what) == b.get(what), (scenario, a["event"], what)
    # no buffer of a pack that already existed is ever reallocated: every ordinal stays 0
    for e in mine:
        for name, st in e["packs"].items():
            for field in ("wf", "wd", "bias"):
                assert st[field] in (None, "%s.%s#0" % (name, field)), (scenario, e["event"], name, field)


def test_repack_all_is_one_batched_launch_per_dtype(recorded):
    _, got = recorded
    ev = [e for e in got["epoch_and_batched"] if e["event"].startswith("repack_all()")]
    assert len(ev) == 1
    launches = _launches(ev, "mrfp_pack_weights_batched")
    assert len(launches) == len(ev[0]["calls"]) == 2 and sorted(c[5] for c in launches) == [F32, BF16]
    assert len(_launches(got["epoch_and_batched"], "mrfp_pack_weights_batched")) == 2
    jobs = sorted(j["ptrs"][1] for c in launches for j in c[1])
    assert jobs == ["w3.bf16.wf#0", "w3.f32.wf#0", "wdw.bf16.wf#0"]          # trainable, bias-free, fp32-contiguous, at most 3x3 taps
    fold = [e for e in got["folded"] if e["event"].startswith("fold_packs_batched()")][0]["calls"]
    assert [c[0] for c in fold] == ["mrfp_pack_weights_folded_batched"] * 2 and sorted(c[5] for c in fold) == [F32, BF16]


def test_the_lazy_and_the_batched_path_stamp_alike():
    """A pack stamped by get_pack and the same pack stamped by the batched re-pack carry equal stamps when nothing changed in
    between (else every pack that repack_all() refreshed would be packed again at its next use, or never again); the same for
    get_folded_pack and fold_packs_batched."""
    from mrfp_amd import conv
    from tools import record_pack_cache as rec
    with rec.stubbed() as r:
        rec._weights(r)
        n3 = r.norm("n3", 16)
        w, b = r.tensors["w3"], r.tensors["b1"]
        pk = conv.get_pack(w, None, torch.bfloat16, 8, 16)
        pkb = conv.get_pack(r.tensors["w1"], b, torch.bfloat16, 8, 16)
        lazy, lazy_b = pk.version, pkb.version
        assert lazy is not None and lazy == r.a.plain_stamp(w, None) and lazy_b == r.a.plain_stamp(r.tensors["w1"], b)
        pk.version = pkb.version = None
        conv.repack_all()
        assert pk.version == lazy and pkb.version is None
        conv.repack_weights([r.tensors["w1"]], "t", [b])
        assert pkb.version == lazy_b
        conv.get_pack(w, None, torch.bfloat16, 8, 16)
        conv.get_pack(r.tensors["w1"], b, torch.bfloat16, 8, 16)
        assert [c[0] for c in r.calls] == ["mrfp_pack_weight"] * 2 + ["mrfp_pack_weights_batched"] * 2        # the last two hit
        fk = conv.get_folded_pack(w, None, n3, torch.bfloat16, 8, 16)
        single = fk.version
        assert single is not None and single == r.a.fold_stamp(w, None, n3)
        fk.version = None
        conv.fold_packs_batched([(w, None, n3, r.a.fold_key(w, None, n3, torch.bfloat16, 8, 16))])
        assert fk.version == single and conv.get_folded_pack(w, None, n3, torch.bfloat16, 8, 16) is fk
        assert [c[0] for c in r.calls[4:]] == ["mrfp_pack_weight_folded", "mrfp_pack_weights_folded_batched"]
