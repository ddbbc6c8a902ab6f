"""The weight-pack cache policy of mrfp_amd/conv.py, recorded on the CPU: which pack is (re)built by which entry point after which
event, which packs are judged fresh, which buffers and job tables are reused.  No GPU and no kernel runs: the name `call` as conv sees
it, `stream` and torch's capture query are replaced by stubs, the weights are CPU Parameters of a few hundred elements, and
torch.empty fills what it hands out with 0x7B bytes, so that a zero-filled buffer can be told from an uninitialised one.

    python tools/record_pack_cache.py        rewrites tests/golden/pack_cache.json

tests/test_pack_cache_cpu.py replays record() and compares with the file.  The file was written ONCE, by this script, from commit
28e6e78 -- the last one whose cache was one dictionary of bare tuples (the second half of Adapter); it is the yardstick for the
per-weight records and named keys and is not to be regenerated from them.

After every driver event: each C-ABI call (entry point, integers and floats exactly, pointers as "which tensor / which pack, which
buffer"; the two batched launches with their job count, prefix table and decoded job records), the state of every named pack (in
the cache?  stamp equal to the current one?  the ordinal identity of wf, wd and bias -- "#0" until a buffer is reallocated -- the
dtype of wf, whether wd is all zero, whether the fp32 bias copy equals the bias), the identity of every cached job table, the tags of
the remembered repack_weights() lists, FOLD_PACK_LAUNCHES and the number of weights the cache holds.
"""
import contextlib
import ctypes
import gc
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from mrfp_amd import _lib, conv, ops  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "pack_cache.json")
F32, BF16 = torch.float32, torch.bfloat16
JOB_T = np.dtype([("w", "<u8"), ("wf", "<u8"), ("wd", "<u8"), ("dims", "<i4", (6,))])             # PackJob of csrc/conv_pack.hip
FOLD_JOB_T = np.dtype([("ptrs", "<u8", (8,)), ("eps", "<f4"), ("dims", "<i4", (7,))])             # FoldJob
BATCHED = {"mrfp_pack_weights_batched": JOB_T, "mrfp_pack_weights_folded_batched": FOLD_JOB_T}


class Adapter:
    """The private names of the cache: per-weight records with a plain and a folded dictionary under named keys (_packs_of), or
    the one dictionary of bare tuples per weight that they replaced."""

    def __init__(self):
        self.new = hasattr(conv, "_packs_of")
        self.cells = [conv._PACKS, conv._BATCH, conv._REPACK_LISTS]
        self.lists = [conv._FOLD_SETS, conv.FOLD_PACK_LAUNCHES, conv._EPOCH, ops.RUNNING_STATS_EPOCH]

    def save(self):
        return [dict(c) for c in self.cells] + [list(c) for c in self.lists]

    def restore(self, saved):
        for c, s in zip(self.cells + self.lists, saved):
            c.clear()
            (c.update if isinstance(c, dict) else c.extend)(s)

    def reset(self):
        for c in self.cells:
            c.clear()
        conv._FOLD_SETS[:] = []
        conv.FOLD_PACK_LAUNCHES[0] = 0

    def packs_of(self, weight):
        """every pack of `weight` in the cache, plain ones first"""
        if self.new:
            rec = conv._packs_of(weight)
            return list(rec.plain.values()) + list(rec.folded.values())
        return list(conv._PACKS.get(id(weight), {}).values())

    def fold_key(self, weight, conv_bias, norm, dtype, Cphys, Nphys, depthwise=False):
        return conv._fold_key(weight, conv_bias, norm, dtype, Cphys, Nphys, depthwise)

    def folded_pack(self, weight, key):
        if self.new:
            return conv._packs_of(weight).folded.get(key)
        return conv._PACKS.get(id(weight), {}).get(key)

    def plain_stamp(self, weight, bias):
        if self.new:
            return conv._plain_version(weight, bias)
        return (weight._version, bias._version if bias is not None else 0, conv._EPOCH[0])

    def fold_stamp(self, weight, conv_bias, norm):
        return conv._fold_version(weight, conv_bias, norm)

    def weights_held(self):
        return len(conv._PACKS)

    def tables(self):
        return conv._BATCH

    def list_tags(self):
        return sorted(conv._REPACK_LISTS)


def _poisoned_empty(real):
    def empty(*a, **k):
        t = real(*a, **k)
        if t.device.type == "cpu" and t.numel() and t.is_contiguous():
            t.view(torch.uint8).fill_(0x7B)
        return t
    return empty


class Recorder:
    def __init__(self, adapter):
        self.a = adapter
        self.protos = _lib.parse_header()
        self.begin()

    def begin(self):
        self.a.reset()
        self.events, self.calls = [], []
        self.tensors = {}            # name -> tensor (driver operands: their addresses get the name)
        self.packs = {}              # name -> (pack, weight name, its current stamp as a function of no arguments, bias name)
        self.slots = {}              # (pack name, field) -> addresses seen, in order
        self.tables = []             # the job tables seen, in order (kept alive: their position is their identity)

    # ---- the stub ------------------------------------------------------------------------------------------------------------------
    def call(self, name, *args):
        types = self.protos[name][1]
        assert len(types) == len(args), (name, len(types), len(args))
        if name in BATCHED:
            n = int(args[2])
            rec = np.frombuffer(ctypes.string_at(args[0], n * BATCHED[name].itemsize), dtype=BATCHED[name]).copy()
            prefix = np.frombuffer(ctypes.string_at(args[1], (n + 1) * 8), dtype=np.int64).tolist()
            self.calls.append((name, ("jobs", rec), ("prefix", prefix), *zip(types[2:], args[2:])))
        else:
            self.calls.append((name, *zip(types, args)))

    # ---- pointers -> names -----------------------------------------------------------------------------------------------------------
    def _names(self):
        tab = {t.data_ptr(): n for n, t in self.tensors.items() if t is not None}
        for pname, (pk, _, _, _) in self.packs.items():
            for field in ("wf", "wd", "bias"):
                t = getattr(pk, field)
                if t is None:
                    continue
                seen = self.slots.setdefault((pname, field), [])
                if t.data_ptr() not in seen:
                    seen.append(t.data_ptr())
                tab[t.data_ptr()] = "%s.%s#%d" % (pname, field, seen.index(t.data_ptr()))
        return tab

    def _arg(self, tab, ctype, v):
        if isinstance(ctype, str):                   # the decoded operands of a batched launch
            if ctype == "prefix":
                return v
            out = []
            for job in v:
                if "ptrs" in v.dtype.names:
                    out.append({"ptrs": [tab.get(int(p), "other") if p else "null" for p in job["ptrs"]], "eps": float(job["eps"]),
                                "dims": job["dims"].tolist()})
                else:
                    out.append({"ptrs": [tab.get(int(job[f]), "other") if job[f] else "null" for f in ("w", "wf", "wd")],
                                "dims": job["dims"].tolist()})
            return out
        if ctype is ctypes.c_void_p:
            return tab.get(int(v), "other") if v else "null"
        return float(v) if ctype in (ctypes.c_float, ctypes.c_double) else int(v)

    # ---- the driver's vocabulary -----------------------------------------------------------------------------------------------------
    def tensor(self, name, t):
        self.tensors[name] = t
        return t

    def norm(self, name, n, **kw):
        m = torch.nn.BatchNorm2d(n, **kw)
        for f in ("weight", "bias", "running_mean", "running_var"):
            self.tensor("%s.%s" % (name, f), getattr(m, f))
        return m

    def plain(self, name, wname, bname, dtype, Cphys, Nphys):
        """get_pack under a name of the driver's"""
        w, b = self.tensors[wname], self.tensors[bname] if bname else None
        pk = conv.get_pack(w, b, dtype, Cphys, Nphys)
        held = self.packs.get(name)
        assert held is None or held[0] is pk, "%s: get_pack returned another pack object" % name
        self.packs[name] = (pk, wname, lambda: self.a.plain_stamp(self.tensors[wname], self.tensors[bname] if bname else None), bname)
        return pk

    def folded(self, name, wname, bname, norm, dtype, Cphys, Nphys, depthwise=False, get=True):
        """get_folded_pack under a name of the driver's (get=False: only name the pack that a batched launch made)"""
        w, b = self.tensors[wname], self.tensors[bname] if bname else None
        if get:
            pk = conv.get_folded_pack(w, b, norm, dtype, Cphys, Nphys, depthwise)
        else:
            pk = self.a.folded_pack(w, self.a.fold_key(w, b, norm, dtype, Cphys, Nphys, depthwise))
        held = self.packs.get(name)
        assert pk is not None and (held is None or held[0] is pk), "%s: another pack object" % name
        self.packs[name] = (pk, wname, lambda: self.a.fold_stamp(self.tensors[wname], self.tensors[bname] if bname else None, norm), None)
        return pk

    def refused(self, what):
        try:
            what()
        except _lib.MrfpHipError as e:
            return "MrfpHipError: %s" % e
        return None

    def drop(self, *names):
        """the driver's last reference to these tensors goes"""
        for n in names:
            del self.tensors[n]
        gc.collect()

    def event(self, label, note=None):
        """closes one driver event: what was called since the last one, and the state it left"""
        tab = self._names()
        calls = [[c[0]] + [self._arg(tab, t, v) for t, v in c[1:]] for c in self.calls]
        self.calls = []
        packs = {}
        for pname, (pk, wname, stamp, bname) in self.packs.items():
            w = self.tensors.get(wname)
            here = w is not None and any(p is pk for p in self.a.packs_of(w))
            st = {"cached": here, "fresh": bool(here and pk.version is not None and pk.version == stamp()),
                  "wf": tab.get(pk.wf.data_ptr()) if pk.wf is not None else None,
                  "wd": tab.get(pk.wd.data_ptr()) if pk.wd is not None else None,
                  "bias": tab.get(pk.bias.data_ptr()) if pk.bias is not None else None,
                  "wf_dtype": str(pk.wf.dtype) if pk.wf is not None else None,
                  "wd_zero": bool((pk.wd.view(torch.uint8) == 0).all()) if pk.wd is not None else None}
            if bname and here and pk.bias is not None:
                b = self.tensors[bname].detach().float()
                st["bias_current"] = bool(torch.equal(pk.bias[:b.numel()], b) and (pk.bias[b.numel():] == 0).all())
            packs[pname] = st
        tables = {}
        for (tag, dtype), st in self.a.tables().items():
            if not any(st is t for t in self.tables):
                self.tables.append(st)
            tables["%s/%s" % (tag, dtype)] = [i for i, t in enumerate(self.tables) if t is st][0]
        ev = {"event": label, "calls": calls, "packs": packs, "tables": tables, "lists": self.a.list_tags(),
              "fold_launches": conv.FOLD_PACK_LAUNCHES[0], "weights": self.a.weights_held()}
        if note is not None:
            ev["note"] = note
        self.events.append(ev)

    def end(self):
        return self.events


def _param(*shape, requires_grad=True, seed=0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return torch.nn.Parameter(torch.randn(*shape, generator=g), requires_grad=requires_grad)


def _bump(t):
    """an in-place update that autograd's version counter sees (optimizer.step of torch, load_state_dict)"""
    with torch.no_grad():
        t.add_(1.0)


def _weights(r):
    r.tensor("w3", _param(16, 8, 3, 3))
    r.tensor("w7", _param(8, 8, 7, 7))
    r.tensor("w1", _param(16, 8, 1, 1))
    r.tensor("b1", _param(16))
    r.tensor("wdw", _param(16, 1, 3, 3))
    r.tensor("wfrozen", _param(16, 8, 3, 3, requires_grad=False, seed=1))
    r.tensor("whalf", torch.nn.Parameter(torch.randn(8, 8, 1, 1, generator=torch.Generator().manual_seed(5)).half()))


# ---- scenarios ---------------------------------------------------------------------------------------------------------------------
def lazy(r):
    _weights(r)
    r.plain("w3.bf16", "w3", None, BF16, 8, 16)
    r.event("first use packs")
    r.plain("w3.bf16", "w3", None, BF16, 8, 16)
    r.event("second use hits")
    r.plain("w3.f32", "w3", None, F32, 8, 16)
    r.event("another dtype is another pack")
    r.plain("w3.bf16.c16", "w3", None, BF16, 16, 16)
    r.event("another padding is another pack; its wd is zero-filled")
    r.plain("w1+b.bf16", "w1", "b1", BF16, 8, 24)
    r.event("a pack with a bias")
    r.plain("w1.bf16", "w1", None, BF16, 8, 24)
    r.event("the same weight without the bias is another pack")
    r.plain("whalf.bf16", "whalf", None, BF16, 8, 8)
    r.event("a weight that is not fp32 is packed from a temporary copy")
    _bump(r.tensors["w3"])
    r.event("in-place update of w3: its packs are stale, the others are not")
    for name, dtype, Cphys in (("w3.bf16", BF16, 8), ("w3.f32", F32, 8), ("w3.bf16.c16", BF16, 16)):
        r.plain(name, "w3", None, dtype, Cphys, 16)
        r.event("re-pack of %s at its next use" % name)
    for name, dtype, Cphys in (("w3.bf16", BF16, 8), ("w3.f32", F32, 8), ("w3.bf16.c16", BF16, 16)):
        r.plain(name, "w3", None, dtype, Cphys, 16)
    r.event("all three hit")
    _bump(r.tensors["b1"])
    r.event("in-place update of b1: only the pack with the bias is stale")
    r.plain("w1+b.bf16", "w1", "b1", BF16, 8, 24)
    r.event("re-pack, the bias buffer refreshed in place")
    r.plain("w1+b.bf16", "w1", "b1", BF16, 8, 24)
    r.plain("w1.bf16", "w1", None, BF16, 8, 24)
    r.event("both hit")


def _model_packs(r):
    _weights(r)
    r.plain("w3.bf16", "w3", None, BF16, 8, 16)
    r.plain("w3.f32", "w3", None, F32, 8, 16)
    r.plain("w7.bf16", "w7", None, BF16, 8, 8)
    r.plain("w1+b.bf16", "w1", "b1", BF16, 8, 16)
    r.plain("wdw.bf16", "wdw", None, BF16, 8, 16)
    r.plain("wfrozen.bf16", "wfrozen", None, BF16, 8, 16)
    r.plain("whalf.bf16", "whalf", None, BF16, 8, 8)
    r.event("packs of a small model")


def _use_all(r):
    for name, (pk, wname, _, bname) in list(r.packs.items()):
        if "fold" in name:
            continue
        dtype = F32 if name.endswith("f32") else BF16
        Cphys = 16 if name.endswith("c16") else 8
        Nphys = 8 if wname in ("w7", "whalf") else 16
        r.plain(name, wname, bname, dtype, Cphys, Nphys)
        r.event("next use of %s" % name)


def epoch_and_batched(r):
    _model_packs(r)
    conv.invalidate_packs()
    r.event("invalidate_packs(): everything is stale")
    conv.repack_all()
    r.event("repack_all(): one launch per dtype over the trainable, bias-free, fp32-contiguous packs of at most 3x3 taps")
    _use_all(r)
    _use_all(r)


def job_table(r):
    _model_packs(r)
    conv.repack_all()
    r.event("repack_all() builds the tables")
    conv.repack_all()
    r.event("the same set: the tables are reused")
    r.plain("w1.f32", "w1", None, F32, 8, 16)
    r.event("a pack created in between")
    conv.repack_all()
    r.event("the fp32 table is rebuilt, the bf16 one reused")
    conv.invalidate_packs()
    conv.repack_all()
    r.event("an epoch bump alone rebuilds nothing")


def explicit_list(r):
    _model_packs(r)
    n3 = r.norm("n3", 16)
    r.plain("w1.bf16", "w1", None, BF16, 8, 16)
    r.folded("w3.fold", "w3", None, n3, BF16, 8, 16)
    r.event("a pack of w1 without its bias, and a folded pack of w3")
    ws = [r.tensors[n] for n in ("w3", "w7", "w1")]
    bs = [None, None, r.tensors["b1"]]
    for t in ws + [bs[2]]:
        t.data.add_(1.0)                     # rewritten behind autograd's back (a flat arena the parameters are views of)
    r.event("the masters were rewritten through .data: every pack still looks fresh", note=[t._version for t in ws])
    conv.repack_weights(ws, "hrfp", bs)
    r.event("repack_weights(): matching packs and their bias copies refreshed, every other pack of these weights marked stale")
    _use_all(r)
    r.folded("w3.fold", "w3", None, n3, BF16, 8, 16)
    r.event("next use of the folded pack")
    _use_all(r)
    r.plain("w3.bf16.c16", "w3", None, BF16, 16, 16)
    r.event("a pack created after the list was remembered")
    conv.prebuild_repack_tables()
    r.event("prebuild_repack_tables(): the bf16 table rebuilt, no launch")
    conv.repack_weights(ws, "hrfp", bs)
    r.event("repack_weights() again: the prebuilt tables are used")
    r.tensor("wtmp", _param(8, 8, 3, 3, seed=2))
    r.plain("wtmp.bf16", "wtmp", None, BF16, 8, 8)
    conv.repack_weights([r.tensors["wtmp"]], "gone")
    r.event("a second list")
    r.drop("wtmp")
    r.event("its weight died")
    conv.prebuild_repack_tables()
    r.event("prebuild_repack_tables() forgets the list whose weights have died")


def folded(r):
    _weights(r)
    n3 = r.norm("n3", 16)
    r.tensor("cb3", _param(16, seed=3))
    get = lambda: r.folded("w3.fold", "w3", "cb3", n3, BF16, 8, 16)      # noqa: E731
    get()
    r.event("first use folds")
    get()
    r.event("second use hits")
    for name in ("w3", "cb3", "n3.weight", "n3.bias", "n3.running_mean", "n3.running_var"):
        _bump(r.tensors[name])
        r.event("in-place change of %s" % name)
        get()
        r.event("... refolds")
    n3.eps = 1e-3
    r.event("a changed eps")
    get()
    r.event("... refolds")
    conv.invalidate_packs()
    r.event("invalidate_packs()")
    get()
    r.event("... refolds")
    ops.RUNNING_STATS_EPOCH[0] += 1
    r.event("a bump of ops.RUNNING_STATS_EPOCH")
    get()
    r.event("... refolds")
    get()
    r.event("and hits")
    ndw = r.norm("ndw", 16)
    r.folded("wdw.fold", "wdw", None, ndw, BF16, 1, 16, depthwise=True)
    r.event("a depthwise pack: fp32 taps for bf16 activations")
    r.folded("wdw.fold", "wdw", None, ndw, BF16, 1, 16, depthwise=True)
    r.event("... hits")
    # the batched launch: two bf16 jobs (one depthwise), one fp32 job, packs that exist and packs that do not
    n1 = r.norm("n1", 16)
    conv.invalidate_packs()
    a = r.a
    items = [(r.tensors["w3"], r.tensors["cb3"], n3, a.fold_key(r.tensors["w3"], r.tensors["cb3"], n3, BF16, 8, 16)),
             (r.tensors["w1"], r.tensors["b1"], n1, a.fold_key(r.tensors["w1"], r.tensors["b1"], n1, F32, 8, 16)),
             (r.tensors["wdw"], None, ndw, a.fold_key(r.tensors["wdw"], None, ndw, BF16, 1, 16, True)),
             (r.tensors["w1"], r.tensors["b1"], n1, a.fold_key(r.tensors["w1"], r.tensors["b1"], n1, BF16, 8, 16))]
    conv.fold_packs_batched(items)
    r.folded("w1.fold.f32", "w1", "b1", n1, F32, 8, 16, get=False)
    r.folded("w1.fold.bf16", "w1", "b1", n1, BF16, 8, 16, get=False)
    r.event("fold_packs_batched(): one launch per dtype, and what it wrote is stamped")
    get()
    r.folded("w1.fold.f32", "w1", "b1", n1, F32, 8, 16)
    r.folded("w1.fold.bf16", "w1", "b1", n1, BF16, 8, 16)
    r.folded("wdw.fold", "wdw", None, ndw, BF16, 1, 16, depthwise=True)
    r.event("all four hit")
    # a registered set: on tensors that are not on a GPU the whole-set refold finds nothing to do and the single launch follows
    c3 = torch.nn.Conv2d(8, 16, 3, bias=True)
    c3.weight, c3.bias = r.tensors["w3"], r.tensors["cb3"]
    from mrfp_amd.inference import _FoldSet
    pairs = _FoldSet([(c3, n3)])
    conv.register_fold_set(pairs)
    ops.RUNNING_STATS_EPOCH[0] += 1
    get()
    r.event("a member of a registered set, not on a GPU: one single launch")
    del pairs, c3
    # refusals
    nhalf = r.norm("nhalf", 16)
    nhalf.weight.data = nhalf.weight.data.half()
    r.tensor("nhalf.weight", nhalf.weight)
    msg = r.refused(lambda: conv.get_folded_pack(r.tensors["w3"], None, nhalf, BF16, 8, 16))
    r.event("a norm weight that is not fp32 is refused", note=msg)
    r.tensor("wnc", torch.nn.Parameter(torch.randn(16, 8, 3, 3, generator=torch.Generator().manual_seed(7)).permute(0, 1, 3, 2)))
    msg = r.refused(lambda: conv.get_folded_pack(r.tensors["wnc"], None, n3, BF16, 8, 16))
    r.event("a weight that is not contiguous is refused", note=msg)
    nostats = torch.nn.BatchNorm2d(16, track_running_stats=False)
    msg = r.refused(lambda: conv.get_folded_pack(r.tensors["w3"], None, nostats, BF16, 8, 16))
    r.event("a norm without running statistics is refused", note=msg)


def lifetime(r):
    _weights(r)
    n3 = r.norm("n3", 16)
    r.plain("w3.bf16", "w3", None, BF16, 8, 16)
    r.plain("w3.f32", "w3", None, F32, 8, 16)
    r.folded("w3.fold", "w3", None, n3, BF16, 8, 16)
    r.plain("w7.bf16", "w7", None, BF16, 8, 8)
    r.folded("wdw.fold", "wdw", None, r.norm("ndw", 16), BF16, 1, 16, depthwise=True)
    r.event("three weights hold packs")
    r.drop("w3")
    r.event("w3 died: its entry is gone")
    r.drop("wdw")
    r.event("a weight with a folded pack only")
    r.drop("w7", "w1", "b1", "wfrozen", "whalf")
    r.event("nothing is left")


SCENARIOS = [("lazy", lazy), ("epoch_and_batched", epoch_and_batched), ("job_table", job_table), ("explicit_list", explicit_list),
             ("folded", folded), ("lifetime", lifetime)]


@contextlib.contextmanager
def stubbed():
    """-> Recorder, over an empty cache with the launches stubbed out; conv, ops and torch are left as they were found"""
    a = Adapter()
    saved = (conv.call, conv.stream, torch.cuda.is_current_stream_capturing, torch.empty, a.save())
    r = Recorder(a)
    conv.call, conv.stream = r.call, (lambda: 0)
    torch.cuda.is_current_stream_capturing = lambda: False
    torch.empty = _poisoned_empty(saved[3])
    try:
        yield r
    finally:
        r.begin()                            # (drops the driver's tensors: their finalizers run on the cache they were made in)
        gc.collect()
        conv.call, conv.stream, torch.cuda.is_current_stream_capturing, torch.empty = saved[:4]
        a.restore(saved[4])


def record():
    """{scenario: its events}"""
    out = {}
    with stubbed() as r:
        for name, scenario in SCENARIOS:
            r.begin()
            gc.collect()
            scenario(r)
            out[name] = r.end()
    return out


def main():
    got = record()
    with open(OUT, "w") as f:
        f.write("{" + ",\n ".join("%s: [\n  %s]" % (json.dumps(k), ",\n  ".join(json.dumps(e, separators=(",", ":")) for e in v))
                                   for k, v in got.items()) + "}\n")
    print("%s: %s" % (OUT, ", ".join("%s %d events, %d calls" % (k, len(v), sum(len(e["calls"]) for e in v)) for k, v in got.items())))


if __name__ == "__main__":
    main()
