"""No-GPU check of the skip-gradient hand-off (mrfp_amd/skipgrad.py): the alias cell, the version-stamped GATE / LOWRANK tags and
the two predicates, on CPU tensors of a few elements -- no kernel is launched.  The rules checked here are the ones the GPU tests
see end to end (tests/test_ops_gpu.py::test_gated_skip_gradient_equals_the_materialised_one, tests/test_lowrank_skip_gpu.py): a broken
promise must raise, because the alternative is a gradient that is silently wrong."""
import itertools

import pytest
import torch

from mrfp_amd import skipgrad as sg
from mrfp_amd._lib import MrfpHipError

CL = torch.channels_last
NO_GATE, NO_FACTORS, STALE = "without its gate", "without its factors", "modified in place before it reached its consumer"


def act(C=8, dtype=torch.bfloat16, shape=None):
    return torch.zeros(shape or (1, C, 2, 3), dtype=dtype).contiguous(memory_format=CL)


def new_cell(lowrank_ok=False):
    return sg.AliasCell(act(), None, lowrank_ok)


def tagged(kind, stale=False):
    t = act()
    if kind == "gate":
        sg.GATE.attach(t, torch.zeros(t.numel() // 8, dtype=torch.uint8))
    else:
        sg.LOWRANK.attach(t, act(32), torch.zeros(8, 32), 32)
    if stale:
        t.add_(0)
    return t


def test_a_tag_is_fetched_by_field_names_only_at_the_version_it_was_attached_at():
    t, mask = act(), torch.zeros(6, dtype=torch.uint8)
    assert sg.GATE.fetch(t) is None and sg.LOWRANK.fetch(t) is None and sg.GATE.fetch(None) is None and sg.LOWRANK.fetch(None) is None
    sg.GATE.attach(t, mask)
    g = sg.GATE.fetch(t)
    assert g.mask is mask and g.version == t._version and sg.LOWRANK.fetch(t) is None
    dp, wd = act(32), torch.zeros(8, 32)
    u = act()
    sg.LOWRANK.attach(u, dp, wd, 32)
    lr = sg.LOWRANK.fetch(u)
    assert lr.dp is dp and lr.wd is wd and lr.K == 32 and lr.version == u._version and sg.GATE.fetch(u) is None
    for tag, x, msg in ((sg.GATE, t, "a gated skip gradient was " + STALE), (sg.LOWRANK, u, "a low-rank skip gradient was " + STALE)):
        v = x._version
        x.add_(0)
        assert x._version != v
        with pytest.raises(MrfpHipError, match=msg):
            tag.fetch(x)
    # the stand-alone forms: untagged tensors and None pass through (no launch), a stale tag raises before any launch
    w = act()
    assert sg.ungate(w) is w and sg.unlowrank(w) is w and sg.ungate(None) is None and sg.unlowrank(None) is None
    with pytest.raises(MrfpHipError, match=STALE):
        sg.ungate(t)
    with pytest.raises(MrfpHipError, match=STALE):
        sg.unlowrank(u)


def test_the_cell_counts_uses_and_is_shared_by_the_alias_and_its_node():
    cell = new_cell()
    assert (cell.uses, cell.gate_issued, cell.lowrank_issued, cell.lowrank_ok) == (0, False, False, False)
    assert new_cell(True).lowrank_ok is True and not hasattr(cell, "__dict__")
    seen = [cell.sole_consumer()]
    for n in (1, 2, 3):
        cell.use()
        assert cell.uses == n
        seen.append(cell.sole_consumer())
    assert seen == [False, True, False, False]   # sole consumer: exactly one use

    class Twice(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            return x * 2

        @staticmethod
        def backward(ctx, dy):
            found.append(sg.alias_cell(ctx))
            return dy * 2

    found = []
    y = Twice.apply(torch.ones(3, requires_grad=True))
    assert sg.alias_cell(y) is None and sg.alias_cell(None) is None
    sg.AliasCell(y, y.grad_fn, True)
    cell = sg.alias_cell(y)
    assert isinstance(cell, sg.AliasCell) and cell.lowrank_ok and sg.alias_cell(y.grad_fn) is cell and getattr(y, sg.ALIAS) is cell
    y.sum().backward()
    assert found == [cell]                       # the autograd node IS the ctx of backward
    z = torch.ones(3)
    sg.AliasCell(z, None)                        # no graph: the tensor alone
    assert sg.alias_cell(z).uses == 0 and not sg.alias_cell(z).lowrank_ok


@pytest.mark.parametrize("bn", [False, True])
def test_a_kept_promise_is_cleared(bn):
    cell = new_cell()
    cell.redeem(act(), bn)                       # nothing promised: anything may arrive
    cell.redeem(None, bn)
    cell.promise_gate()
    assert cell.gate_issued and not cell.lowrank_issued
    cell.redeem(tagged("gate"), bn)
    assert not cell.gate_issued
    cell.promise_lowrank()
    assert cell.lowrank_issued and not cell.gate_issued
    cell.redeem(tagged("lowrank"), bn)
    assert not cell.lowrank_issued


@pytest.mark.parametrize("arrived", ["untagged", "stale", "none", "other tag"])
def test_a_broken_promise_raises_and_the_promise_message_wins_over_the_stale_one(arrived):
    def what(kind):
        other = "lowrank" if kind == "gate" else "gate"
        return {"untagged": act(), "stale": tagged(kind, stale=True), "none": None, "other tag": tagged(other)}[arrived]
    for bn, owner in ((False, "a gated skip gradient reached its convolution "), (True, "a gated gradient reached its BatchNorm ")):
        cell = new_cell()
        cell.promise_gate()
        with pytest.raises(MrfpHipError, match=owner + NO_GATE + r".*outside mrfp_amd\.ops \(set MRFP_GATED_SKIP=0\)") as e:
            cell.redeem(what("gate"), bn)
        assert STALE not in str(e.value) and cell.gate_issued
    cell = new_cell(True)
    cell.promise_lowrank()
    with pytest.raises(MrfpHipError, match="a low-rank skip gradient reached its convolution " + NO_FACTORS
                       + r".*outside mrfp_amd\.ops \(set MRFP_LOWRANK_SKIP=0\)") as e:
        cell.redeem(what("lowrank"))
    assert STALE not in str(e.value) and cell.lowrank_issued
    # both promised: one tensor cannot carry both, and the gate's message comes first
    cell.promise_gate()
    with pytest.raises(MrfpHipError, match=NO_GATE):
        cell.redeem(tagged("lowrank"))


def test_the_predicates_answer_as_the_expressions_they_replaced():
    rows = 0
    for dtype, C, layout, variant in itertools.product((torch.float32, torch.bfloat16, torch.float16), (8, 12, 64),
                                                       ("channels-last", "contiguous"), ("same", "shape", "dtype")):
        x = act(C, dtype)
        t = torch.zeros((1, C, 3, 2) if variant == "shape" else (1, C, 2, 3),
                        dtype=(torch.float16 if dtype != torch.float16 else torch.bfloat16) if variant == "dtype" else dtype)
        if layout == "channels-last":
            t = t.contiguous(memory_format=CL)
        # ops._keeps_sign_mask, ctx.gate_ok, the tail of ops.batch_norm_act as they were spelled (x.shape[1] is _geom's C and conv's Cphys)
        want_mask = x.element_size() == 2 and x.shape[1] % 8 == 0
        assert want_mask == (dtype != torch.float32 and C in (8, 64))
        assert sg.mask_possible(x) is want_mask
        # ops._BatchNormAct.backward as it was spelled
        want_gate = t.dtype == x.dtype and t.shape == x.shape and t.is_contiguous(memory_format=CL)
        assert want_gate == (layout == "channels-last" and variant == "same")
        assert sg.gateable(t, x) is want_gate
        # conv._Conv2d.backward as it was spelled (dskip = t, dx an empty of x's shape)
        dx, Cphys = torch.empty_like(x), x.shape[1]
        want_dgrad = (t.dtype == x.dtype and x.element_size() == 2 and Cphys % 8 == 0 and t.shape == dx.shape
                      and t.is_contiguous(memory_format=CL))
        assert (sg.mask_possible(x) and sg.gateable(t, x)) is want_dgrad
        rows += 1
    assert rows == 54
