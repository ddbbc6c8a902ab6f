"""The allocation poisoner on CPU tensors, and the inventory that ties every allocating function of mrfp_amd to a poison case.

No GPU: poison_common works on whatever device torch.empty is asked for, and the inventory is an AST walk."""
import pytest
import torch

import poison_common as pc

CL = torch.channels_last


@pytest.fixture(autouse=True)
def _clean():
    pc.reset()
    yield
    pc.reset()


@pytest.mark.parametrize("byte,f32,bf16,f16,i64,i32,u8", [
    (0x00, 0.0, 0.0, 0.0, 0, 0, 0),
    (0xFF, float("nan"), float("nan"), float("nan"), -1, -1, 255),
    (0x7B, 1.3057709929374801e+36, 1.3032665114922417e+36, 61280.0, 0x7B7B7B7B7B7B7B7B, 0x7B7B7B7B, 123),
])
def test_each_fill_gives_the_stated_values_per_dtype(byte, f32, bf16, f16, i64, i32, u8):
    with pc.poisoned(byte, host=True):
        got = {d: torch.empty(5, dtype=d) for d in (torch.float32, torch.bfloat16, torch.float16, torch.int64, torch.int32, torch.uint8)}
        like = torch.empty_like(torch.zeros(3, 2))
        strided = torch.empty_strided((2, 3), (3, 1), dtype=torch.float16)
        new = torch.zeros(2, dtype=torch.int32).new_empty((4,))
    want = {torch.float32: f32, torch.bfloat16: bf16, torch.float16: f16, torch.int64: i64, torch.int32: i32, torch.uint8: u8}
    for d, t in got.items():
        for v in t.tolist():
            assert (v != v) if want[d] != want[d] else (v == want[d]), (d, v, want[d])
        assert t.data_ptr() % 16 == 0          # G keeps whatever alignment the allocator gives (64 bytes on the host, 256+ on the device)
    for t, w in ((like, f32), (strided, f16), (new, i32)):
        for v in t.reshape(-1).tolist():
            assert (v != v) if w != w else (v == w)
    if byte == 0x7B:
        assert 1e36 < f32 < 3.4e38 and 1e36 < bf16 < 3.4e38 and 6e4 < f16 < 65504         # finite and huge in every float type
    assert len(pc.REGISTRY) == 9


def test_channels_last_and_zero_dim_requests_keep_shape_and_strides():
    with pc.poisoned(0x7B, host=True):
        a = torch.empty((2, 8, 3, 5), dtype=torch.bfloat16, memory_format=CL)
        b = torch.empty_like(a, memory_format=CL)
        s = torch.empty((), dtype=torch.float16).expand(2, 3, 4, 5)         # conv.py's stand-in for an unread dx
        z = torch.empty(0, dtype=torch.float32)
    ref = torch.zeros((2, 8, 3, 5), dtype=torch.bfloat16).contiguous(memory_format=CL)
    for t in (a, b):
        assert t.shape == ref.shape and t.stride() == ref.stride() and t.is_contiguous(memory_format=CL)
        assert t.data_ptr() % 16 == 0 and t.dtype == torch.bfloat16
    assert s.shape == (2, 3, 4, 5) and s.stride() == (0, 0, 0, 0) and s[1, 2, 3, 4].item() == 61280.0
    assert z.numel() == 0
    assert pc.guards_intact()


def test_zeros_randn_and_autograd_do_not_go_through_the_patched_names():
    with pc.poisoned(0xFF, host=True):
        z = torch.zeros(3)
        r = torch.randn(3, requires_grad=True)
        (r * 2).sum().backward()
    assert z.tolist() == [0.0] * 3 and r.grad.tolist() == [2.0] * 3 and not pc.REGISTRY


def test_host_requests_pass_through_by_default():
    with pc.poisoned(0xFF):
        t = torch.empty(4, dtype=torch.int32)
        u = torch.empty_like(t)
    assert not pc.REGISTRY and t.shape == u.shape == (4,)


def test_pinned_requests_pass_through():
    def ask():
        return torch.empty(1, dtype=torch.int32, pin_memory=True)
    try:
        ask()
        can_pin = True
    except RuntimeError:                     # a torch that cannot pin memory without a device: the patched call must fail alike
        can_pin = False
    with pc.poisoned(0xFF, host=True):
        if can_pin:
            assert ask().shape == (1,)
        else:
            with pytest.raises(RuntimeError):
                ask()
    assert not pc.REGISTRY


def test_patched_names_are_restored_after_an_exception():
    before = (torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty)
    with pytest.raises(KeyError):
        with pc.poisoned(0x7B, host=True):
            assert torch.empty is not before[0] and torch.Tensor.new_empty is not before[3]
            raise KeyError("inside")
    assert (torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty) == before
    assert torch.empty(2).shape == (2,) and not pc.REGISTRY
    with pc.poisoned(0x00, host=True):                  # and the block can be opened again
        pass


def test_nesting_is_refused():
    with pc.poisoned(0x00, host=True):
        with pytest.raises(RuntimeError, match="does not nest"):
            with pc.poisoned(0xFF):
                pass
        assert torch.empty is not pc._REAL["empty"]         # the outer block is still open
    assert torch.empty is pc._REAL["empty"]


@pytest.mark.parametrize("dtype", [torch.uint8, torch.bfloat16, torch.float32, torch.int64])
def test_one_element_past_either_end_breaks_the_guards_and_a_full_overwrite_does_not(dtype):
    es = torch.empty((), dtype=dtype).element_size()
    with pc.poisoned(0x7B, host=True):
        t = torch.empty(7, dtype=dtype)
    t.fill_(1)
    assert pc.guards_intact() and pc.guard_report() == []
    off = t.storage_offset()
    t.as_strided((1,), (1,), off + 7).fill_(1)              # one element behind the end
    rep = pc.guard_report()
    assert len(rep) == 1 and "back guard" in rep[0] and "offset +0 " in rep[0] and not pc.guards_intact()
    pc.reset()
    with pc.poisoned(0xFF, host=True):
        t = torch.empty((2, 8, 3, 3), dtype=dtype, memory_format=CL)
    t.zero_()
    assert pc.guards_intact()
    t.as_strided((1,), (1,), t.storage_offset() - 1).fill_(1)           # one element before the start
    rep = pc.guard_report()
    assert len(rep) == 1 and "front guard" in rep[0] and ("offset %+d " % (-t.numel() * es - es)) in rep[0]


def test_the_call_site_is_the_first_frame_inside_the_package_and_helpers_name_their_caller():
    from mrfp_amd import ops
    with pc.poisoned(0x7B, host=True):
        y = ops.empty_cl(1, 8, 2, 2, torch.float32, "cpu")
        z = ops.zeros_cl(1, 8, 2, 2, torch.float32, "cpu")
        torch.empty(3)
    assert y.is_contiguous(memory_format=CL) and float(z.abs().sum()) == 0.0
    assert [r[3] for r in pc.REGISTRY] == ["ops.empty_cl", None]      # called from a test: the helper is the only package frame
    assert pc.SITES == {"ops.empty_cl"}
    names = pc._qualnames(ops.__file__)
    assert "_BatchNormAct.forward" in names.values() and "empty_cl" in names.values()


def test_bits_tells_zero_signs_apart_and_compares_nan():
    a = torch.tensor([0.0, float("nan")])
    b = torch.tensor([-0.0, float("nan")])
    assert torch.equal(pc.bits(a), pc.bits(a.clone())) and not torch.equal(pc.bits(a), pc.bits(b))
    x = torch.randn(2, 8, 3, 3).contiguous(memory_format=CL).to(torch.bfloat16)
    assert pc.bits(x).shape == x.shape and torch.equal(pc.bits(x), pc.bits(x.clone()))
    msg = pc.describe_mismatch("y", x, x + 1, 0x00, 0xFF)
    assert "(b, y, x, c) = (0, 0, 0, 0)" in msg and "y = H - 3" in msg
    # position in the line: C = 8 in bf16 is one 16-byte vector per pixel, 256 row threads of four pixels each
    assert pc.row_trip(8, torch.bfloat16) == 1024 and pc.row_trip(64, torch.bfloat16) == 128 and pc.row_trip(19, torch.float32) == 52
    wide = torch.zeros(1, 64, 1, 150, dtype=torch.bfloat16).contiguous(memory_format=CL)
    other = wide.clone()
    other[0, 5, 0, 131] = 1.0
    assert "trip 1 of 128 pixels, pixel 3 of it" in pc.describe_mismatch("y", wide, other, 0x00, 0x7B)


def test_named_results_carry_their_names_into_the_report():
    r = pc.named(("loss", torch.zeros(())), y=torch.ones(2), dx=None)
    assert isinstance(r, tuple) and len(r) == 3 and r.names == ("loss", "y", "dx") and r[2] is None

    def counts():
        return pc.named(hist=torch.empty(3, dtype=torch.int64).add_(1), pred=torch.zeros(2))
    with pytest.raises(AssertionError, match="hist: fill 0x00 and fill 0xFF differ"):
        pc.run_three(counts, host=True)


def test_run_three_passes_what_writes_all_it_reads_and_names_what_does_not():
    def good():
        t = torch.empty((2, 8, 3, 3), dtype=torch.bfloat16, memory_format=CL)
        t.fill_(1.5)
        return t, None, torch.empty(4, dtype=torch.int64).zero_()
    assert pc.run_three(good, host=True) == set()           # (no frame of the package on the stack)

    def short():                                             # forgets the last line
        t = torch.empty((2, 8, 3, 3), dtype=torch.float32, memory_format=CL)
        t[:, :, :2].fill_(1.0)
        return (t.clamp(max=3.0e38).nan_to_num(7.0),)
    with pytest.raises(AssertionError, match=r"depends on what fresh memory held(.|\n)*y = H - 1"):
        pc.run_three(short, ["y"], host=True)

    def counts():                                            # an accumulator nobody cleared
        return (torch.empty(3, dtype=torch.int64).add_(1),)
    with pytest.raises(AssertionError, match="fill 0x00 and fill 0xFF differ in 3 of 3"):
        pc.run_three(counts, host=True)

    def unwritten():
        return (torch.empty(3),)
    with pytest.raises(AssertionError, match="non-finite values under fill 0xFF"):
        pc.run_three(unwritten, host=True)

    def past_the_end():
        t = torch.empty(5, dtype=torch.float16)
        t.as_strided((8,), (1,)).fill_(1.0009765625)        # a 16-byte store over a 10-byte body (0x3C01: no byte equals a fill)
        return (t,)
    with pytest.raises(AssertionError, match=r"a store left its buffer(.|\n)*back guard(.|\n)*offset \+0 "):
        pc.run_three(past_the_end, host=True)
    assert torch.empty is pc._REAL["empty"]


# ---- the inventory -------------------------------------------------------------------------------------------------------------------
ADMISSIBLE = ("host memory", "more than one rank")


def _table():
    import test_poison_gpu as g
    return g.CASES, g.EXEMPT


def test_inventory_lists_the_allocating_functions():
    inv = pc.inventory()
    # (when this was written: 80 functions, 127 sites -- ops 55 / 90, conv 11 / 16, input_pipeline 10 / 17, harness 2 / 2, skipgrad 2 / 2)
    print("%d allocating functions, %d sites" % (len(inv), sum(len(v) for v in inv.values())))
    assert len(pc.MODULES) >= 30 and "network.mynn" in pc.MODULES and "inference" in pc.MODULES        # the whole package is walked
    for m in ("ops", "conv", "input_pipeline", "harness", "skipgrad"):
        assert any(k.startswith(m + ".") for k in inv), "no allocating function found in %s.py: did the walk break?" % m
    for name in ("ops._BatchNormAct.forward", "conv._launch_wgrads.run", "ops.sync_bn_poll", "harness.FlatSGD.step", "skipgrad.ungate"):
        assert name in inv, name
    assert [s for s in inv["ops.sync_bn_poll"] if s[2]], "sync_bn_poll's word is pinned"


def claimed(cases):
    out = {}
    for c in cases:
        for s in c.sites:
            out.setdefault(s, []).append(c.name)
    return out


def unclaimed(inv, cases, exempt):
    by = claimed(cases)
    return sorted(f for f in inv if f not in by and f not in exempt)


def test_every_allocating_function_is_claimed_by_a_case_or_exempt():
    cases, exempt = _table()
    inv = pc.inventory()
    missing = unclaimed(inv, cases, exempt)
    assert not missing, "allocating functions without a poison case (add one to tests/test_poison_gpu.py): %s" % missing
    unknown = sorted(s for s in claimed(cases) if s not in inv)
    assert not unknown, "cases claim functions that allocate nothing (renamed?): %s" % unknown
    assert len(exempt) <= 4, exempt
    for name, reason in exempt.items():
        assert name in inv, "EXEMPT names %s, which the walk no longer finds" % name
        assert any(a in reason for a in ADMISSIBLE), "%s: %r is neither of %s" % (name, reason, ADMISSIBLE)
        assert name not in claimed(cases), "%s is both exempt and claimed" % name
    assert "ops.sync_bn_poll" in exempt
    for name in ("harness.FlatArena.accumulate", "harness.FlatSGD.step", "skipgrad.ungate", "skipgrad.unlowrank"):
        assert name not in exempt


def test_dropping_the_only_claim_on_a_function_is_noticed():
    cases, exempt = _table()
    inv = pc.inventory()
    by = claimed(cases)
    singles = sorted(f for f, cs in by.items() if len(cs) == 1)
    assert singles, "every function is claimed twice?"
    for f in singles:
        owner = by[f][0]

        class Without:
            def __init__(self, c):
                self.name, self.sites = c.name, tuple(s for s in c.sites if not (c.name == owner and s == f))
        assert unclaimed(inv, [Without(c) for c in cases], exempt) == [f]


def test_a_stale_exemption_is_noticed():
    cases, exempt = _table()
    inv = dict(pc.inventory())
    inv.pop("ops.sync_bn_poll")
    assert [n for n in exempt if n not in inv] == ["ops.sync_bn_poll"]


def test_case_names_are_unique_and_every_case_declares_a_tuple_of_sites():
    cases, _ = _table()
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    for c in cases:
        assert isinstance(c.sites, tuple) and callable(c.build)


def test_launch_plan_routes_the_chosen_cases_to_their_families():
    """Host-only queries: the premises of the family names of the convolution cases in tests/test_poison_gpu.py."""
    import ctypes
    F32, BF16 = torch.float32, torch.bfloat16
    import conv_exact_common as cx
    from mrfp_amd import _lib
    L = _lib.lib()

    def q(T, c):
        B, C, H, W, N, k, st, pad, dil = c[:9]
        t, epc = (0, 4) if T == F32 else (1, 8)
        Cp, Np = (C + epc - 1) // epc * epc, (N + epc - 1) // epc * epc
        Ho, Wo = cx.out_size(H, k, st, pad, dil), cx.out_size(W, k, st, pad, dil)
        qq = dil * (k - 1) - pad
        out = (ctypes.c_int64 * 5)()
        L.mrfp_conv_wgrad_plan(t, B, H, W, Cp, Np, Np, k, k, Ho, Wo, st, pad, pad, dil, 1, out)
        return (L.mrfp_conv_stats_block_rows(t, B, H, W, Cp, Np, k, k, Ho, Wo, st, pad, pad, dil, 1),
                L.mrfp_conv_stats_block_rows(t, B, Ho, Wo, Np, Cp, k, k, H, W, 1, qq, qq, dil, st), out[0], out[2])

    c64 = (3, 64, 33, 31, 64, 3, 1, 1, 1)
    assert q(BF16, c64)[0] < 0 and q(BF16, c64)[1] < 0                                       # weight-stationary 3x3, both directions
    assert q(BF16, cx.c64_as_dense(cx.C128_CASES[0]))[1] < 0                                 # ... its 128-channel form, as a dgrad
    assert q(BF16, (2, 64, 20, 18, 256, 1, 1, 0, 1))[0] == 128                               # pointwise
    assert q(BF16, cx.pwk_as_dense(cx.PWK_CASES[2]))[0] == 240                               # long-K pointwise
    assert q(BF16, cx.CASES[0])[0] == 64 and q(F32, (2, 128, 16, 16, 128, 3, 2, 1, 1))[0] == 96        # generic tiles
    assert q(BF16, cx.pwk_as_dense(cx.PWK_CASES[4]))[2] == 1 and q(BF16, (8, 128, 192, 192, 128, 3, 1, 1, 1))[2] == 0      # wg1, wg3
    assert q(BF16, (2, 304, 240, 240, 256, 3, 1, 1, 1))[2] == 4 and q(F32, cx.CASES[0])[2] == 2
    assert q(F32, (2, 128, 16, 16, 128, 3, 2, 1, 1))[2] == 3
    assert q(BF16, c64)[3] > 1 and q(F32, cx.pwk_as_dense(cx.PWK_CASES[2]))[3] > 1           # split weight gradients
