"""The rounding model of tests/rounding_model_common.py, proved on the host: no GPU, no HIP library.

  * the honest fp32 emulation of every case passes scaled < C_F32[op] on every output, for bf16 and f16; the designed gradients
    put at least a quarter of dx into the statistic terms; settle() stays under its cap (the case builders raise otherwise);
  * every planted defect is caught by the metric, for both types.  Which output catches which defect (first case that does):

        defect          what the emulation does wrong                                       caught by
        qr0             Q = R = 0: the backward ignores both statistics                     dx
        k0              K = 0 (NP+)                                                         dx
        roll            the finalize reads the sums of the neighbouring channel             y, rm, rv, dx, dw, db
        lastline        the last line missing from the backward reductions                  dw, db, dx
        lastvec         the last channel vector of a line not written                       y, dx, dres
        gate_left       the ReLU gate read one pixel to the left                            dx, dres, dw, db
        double_round    the residual added after a rounding to T                            y
        mult1           the multiplicity n taken as 1 behind a resize                       dx

    so every output the GPU tests assert (y, dx, dres, dweight, dbias, running mean / variance) catches at least one defect;
  * the same defects under the old measure (largest difference over the tensor's largest value, 10 x tol(bf16) = 0.25, an i.i.d.
    upstream gradient) PASS for Q = R = 0 and K = 0: why the old bar was not enough.
"""
from functools import lru_cache

import pytest
import torch

import rounding_model_common as rm

TIDS = [rm.dname(t) for t in rm.TYPES]

EXPECTED_CATCHERS = {
    "qr0": {"dx"}, "k0": {"dx"}, "roll": {"y", "rm", "rv", "dx", "dw", "db"}, "lastline": {"dw", "db", "dx"},
    "lastvec": {"y", "dx", "dres"}, "gate_left": {"dx", "dres", "dw", "db"}, "double_round": {"y"}, "mult1": {"dx"},
}


@lru_cache(maxsize=None)
def cases(T):
    return list(rm.all_cases(T))


def test_constants_are_bounded_and_cover_every_operator():
    assert all(16 <= c <= 4096 for c in rm.C_F32.values())
    for T in rm.TYPES:
        assert {op for op, *_ in cases(T)} == set(rm.C_F32)


@pytest.mark.parametrize("T", rm.TYPES, ids=TIDS)
def test_honest_emulation_passes_and_the_table_is_current(T):
    """scaled < C_F32[op] on every output of every case; the largest value per operator, printed next to the one MEASURED records,
    has not outgrown the record (within a factor of 2: the last digits follow the order in which the host's torch build sums in
    fp32; the constants keep a factor of 16 above the record)."""
    seen = {}
    for op, cid, ref, emu, _ in cases(T):
        w = rm.worst(emu(), ref, T)
        assert set(w) == set(ref["mag"]), (cid, set(w), set(ref["mag"]))
        for k, v in w.items():
            assert v < rm.C_F32[op], (cid, k, v)
        seen[op] = max(seen.get(op, 0.0), max(w.values()))
    for op, v in sorted(seen.items()):
        print("%-26s %-9s largest scaled value of the emulation %8.3f   recorded %8.3f   C_F32 %d"
              % (op, rm.dname(T), v, rm.MEASURED[op][rm.TYPES.index(T)], rm.C_F32[op]))
        assert v <= 2.0 * max(rm.MEASURED[op][rm.TYPES.index(T)], 1.0), (op, v)


@pytest.mark.parametrize("T", rm.TYPES, ids=TIDS)
def test_designed_gradients_put_a_quarter_of_dx_into_the_statistic_terms(T):
    n = 0
    for op, cid, ref, _, _ in cases(T):
        if op in ("batch_norm", "batch_norm_relu6", "batch_norm_resize", "instance_norm", "instance_norm_relu_pool", "np_plus"):
            assert rm.stat_share(ref) >= 0.25, (cid, rm.stat_share(ref))
            n += 1
    assert n > 50


@pytest.mark.parametrize("T", rm.TYPES, ids=TIDS)
def test_pool_inputs_keep_their_arg_max_through_a_rounding(T):
    for shape, affine, _ in rm.IN_POOL_CASES:
        c = rm.in_case(shape, T, affine, True, pool=True)
        z = rm.norm_model("in", c["x"], c["w"], c["b"], torch.zeros_like(c["x"]), act="relu")["y"]
        assert rm.window_gap_ok(z, T), shape


@pytest.mark.parametrize("T", rm.TYPES, ids=TIDS)
def test_settle_leaves_no_pre_activation_in_the_band_and_moves_almost_nothing(T):
    for shape in rm.BN_SHAPES:
        for act, gates in (("relu", (0.0,)), ("relu6", (0.0, 6.0))):
            c = rm.bn_case(shape, T, True, act == "relu", act=act)
            for z, mag in rm.norm_pre(c["w"], c["b"], c["res"], (0, 2, 3), gates=gates)(c["x"].double()):
                assert not bool((z.abs() <= rm.BAND * mag).any())
    # the cap itself: a draw that needs more than 1e-4 of its elements moved is refused
    w, b = torch.ones(8), torch.zeros(8)
    lattice = lambda k: torch.arange(-8.0, 9.0).repeat(2, 8, 4, 1)            # symmetric integers: the mean, 0, is an input value
    with pytest.raises(AssertionError):
        rm.settled(lattice, T, rm.norm_pre(w, b, None, (0, 2, 3)))


@pytest.mark.parametrize("T", rm.TYPES, ids=TIDS)
def test_every_planted_defect_is_caught(T):
    caught = {}
    for op, cid, ref, emu, defects in cases(T):
        for d in defects:
            w = rm.worst(emu(d), ref, T)
            for k, v in w.items():
                if not v < rm.C_F32[op]:
                    caught.setdefault(d, {}).setdefault(k, (cid, v))
    for d, want in EXPECTED_CATCHERS.items():
        got = caught.get(d, {})
        print(d, {k: "%s %.3g" % v for k, v in got.items()})
        assert got, "defect %s passes the metric" % d
        assert want <= set(got), (d, want, set(got))
    catchers = set().union(*[set(v) for v in caught.values()])
    assert {"y", "dx", "dres", "dw", "db", "rm", "rv"} <= catchers


def test_the_f16_subnormal_term_is_the_reference_own_rounding():
    """Without h_T the correctly rounded float64 result fails: P*dy = 3.0e-5 stored in f16 is up to 2^-25 = 3.0e-8 off, u_T |r| is 1.5e-8."""
    r = torch.tensor([503.49 * 2.0 ** -24], dtype=torch.float64)
    d = r.to(rm.F16).double()
    assert rm.scaled(d, r, r.abs(), rm.F16) == 0.0
    literal = float(((d - r).abs() - rm.U[rm.F16] * r.abs()) / (rm.U32 * r.abs()))
    assert literal > 4096.0


OLD_SHAPES = [(2, 64, 17, 23), (3, 48, 9, 31), (2, 256, 12, 12)]                   # tests/test_ops_gpu.py SHAPES
OLD_NP_SHAPES = [(2, 64, 16, 16), (4, 256, 9, 13), (16, 64, 6, 5)]


def test_old_measure_passes_a_backward_that_ignores_the_statistics():
    """The old bar: relerr (over the tensor's maximum) below 10 x tol(bf16) = 0.25 under an i.i.d. zero-mean gy.  A BatchNorm /
    InstanceNorm backward with Q = R = 0 and an NP+ backward with K = 0 pass it on the shapes of tests/test_ops_gpu.py -- and fail
    the per-element metric by orders of magnitude on the same inputs."""
    T, bar = rm.BF16, 10 * 2.5e-2
    for kind, shapes in (("bn", OLD_SHAPES), ("in", OLD_SHAPES)):
        for shape in shapes:
            C = shape[1]
            w, b, _, _ = rm.bn_params(C)
            x = rm.rnd(*shape, seed=1, scale=3.0, shift=1.5, dtype=T)
            gy = rm.rnd(*shape, seed=3, dtype=T)
            ref = rm.norm_reference(kind, x, w, b, gy)
            bad = rm.norm_model(kind, x, w, b, gy, fd=rm.F32, T=T, defect="qr0")
            old = rm.relerr(bad["dx"], ref["dx"])
            new = rm.scaled(bad["dx"], ref["dx"], ref["mag"]["dx"], T)
            print(kind, shape, "Q = R = 0: old measure %.3f (bar %.2f), scaled %.3g" % (old, bar, new))
            assert old < bar and new > 4096
    for shape in OLD_NP_SHAPES:
        B, C, H, W = shape
        c = rm.np_case(shape, T, False)
        c["gy"] = rm.rnd(*shape, seed=10, dtype=T)
        ref = rm.np_reference(**c)
        bad = rm.np_model(fd=rm.F32, T=T, defect="k0", **c)
        old = rm.relerr(bad["dx"], ref["dx"])
        new = rm.scaled(bad["dx"], ref["dx"], ref["mag"]["dx"], T)
        print("np_plus", shape, "K = 0: old measure %.3f (bar %.2f), scaled %.3g" % (old, bar, new))
        assert old < bar and new > 4096
