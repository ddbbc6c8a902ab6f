"""The model of tests/fourier_model_common.py, proved on the host: no GPU.

The metric must discriminate.  The honest emulations of both arithmetic classes pass every case of the table; every planted defect,
applied to the emulation, fails EVERY case it applies to by at least twice the bound; the one defect the old norm-relative measure of
tests/test_fourier_gpu.py cannot see (the lo parts of the split-bf16 factors dropped) is shown to pass that measure and to fail this
one.  The routes the table writes down are checked against mrfp_fourier_route here too (a host function: the library loads without
a GPU), with the enumeration that proves the table complete; tests/test_fourier_exact_gpu.py repeats both before it runs a kernel."""
import ctypes

import pytest
import torch

import fourier_model_common as fm
from fourier_model_common import BF16, F16, F32

OLD_TOL = {F32: 2e-5, BF16: 1.5e-2, F16: 1.5e-2}          # tests/test_fourier_gpu.py::test_fourier_amplitude_mix


@pytest.fixture(scope="module")
def survey():
    """One walk over the table: the honest emulations of every (case, type), every defect on one type per case."""
    emu, bad = {}, {}
    for c in fm.TABLE:
        for i, T in enumerate(c.expect):
            ref = fm.reference_of(c.name, T)
            fm.check_conditioning(ref, c.lam)
            emu[c.name, T, "fp32"] = fm.worst(fm.emulate_case(c.name, T), ref, T)
            split = T == BF16 and fm.split_applies(c)
            if split:
                emu[c.name, T, "split"] = fm.worst(fm.emulate_case(c.name, T, "split"), ref, T)
            if split and fm.applies("lo_dropped", c):
                out = fm.emulate_case(c.name, T, "split", "lo_dropped")
                bad["lo_dropped", c.name, T] = (fm.worst(out, ref, T), {k: fm.relerr(out[k], ref[k]) for k in ("y", "dx")})
            if i == 0:
                for d in fm.DEFECTS:
                    if fm.applies(d, c):
                        bad[d, c.name, T] = (fm.worst(fm.emulate_case(c.name, T, "fp32", d), ref, T), None)
    return emu, bad


@pytest.mark.parametrize("T", [BF16, F16, F32], ids=fm.dname)
@pytest.mark.parametrize("shape", [(32, 512), (512, 32), (96, 192), (48, 64)], ids=lambda s: "%dx%d" % s)
def test_designed_inputs_stay_well_conditioned_after_rounding(shape, T):
    H, W = shape
    x = fm.designed_input(2, 4, H, W, T, seed=H + W)
    assert torch.equal(x.to(T).double(), x)
    ref = fm.reference(x, fm.noise_input(2, 4, H, W, T, 1), (1, 0), 5.0, 0.8, False)
    fm.check_conditioning(ref, 0.8)
    assert ref["amp_min"] >= 0.99, ref["amp_min"]                        # rounding to T moves no amplitude by 1 % of the design minimum
    ref = fm.reference(x, fm.noise_input(2, 4, H, W, T, 1), (1, 0), 5.0, 0.8, True)
    assert 0.55 <= float(ref["ratio"].min()) and float(ref["ratio"].max()) <= 1.85


def test_random_data_would_not_be_held_by_this_metric():
    """Why the inputs are designed: on plain noise the ratio is unbounded, and check_conditioning says so."""
    x = fm.noise_input(2, 4, 48, 64, F32, 3)
    ref = fm.reference(x, x, (1, 0), 5.0, 0.8, True)
    with pytest.raises(AssertionError):
        fm.check_conditioning(ref, 0.8)


def test_honest_emulations_pass_every_case(survey):
    emu, _ = survey
    assert {(n, T) for n, T, cls in emu if cls == "fp32"} == set(fm.RUNS)
    for (name, T, cls), w in emu.items():
        assert max(w.values()) < fm.BOUND[T, cls], (name, fm.dname(T), cls, w)


def test_emulation_table_is_current(survey):
    """fm.MEASURED is the record of this walk (the last digits depend on the host's FFT: 25 % of slack), and the bounds are 2 x it."""
    emu, _ = survey
    seen = {}
    for (name, T, cls), w in emu.items():
        seen[T, cls] = max(seen.get((T, cls), 0.0), *w.values())
    print({(fm.dname(k[0]), k[1]): round(v, 3) for k, v in seen.items()})
    assert set(seen) == set(fm.MEASURED)
    for k, v in seen.items():
        assert v <= 1.25 * fm.MEASURED[k] and v >= fm.MEASURED[k] / 1.25, (k, v, fm.MEASURED[k])
        assert fm.BOUND[k] == fm.bound_for(fm.MEASURED[k])
    assert all(b <= 4 for b in fm.BOUND.values()), fm.BOUND               # a few roundings: the weakest defect scores in the hundreds


@pytest.mark.parametrize("defect", fm.DEFECTS)
def test_planted_defect_fails_every_case_it_applies_to(survey, defect):
    _, bad = survey
    hits = {k: v for k, v in bad.items() if k[0] == defect}
    assert len(hits) >= 10, (defect, len(hits))
    weakest = None
    for (_, name, T), (w, _) in hits.items():
        v = max(w[k] for k in fm.DEFECT_OUTPUT.get(defect, ("y",)))
        assert v >= 2.0 * fm.BOUND[T, "fp32"], (defect, name, fm.dname(T), w)
        weakest = v if weakest is None else min(weakest, v)
    print(defect, "cases", len(hits), "weakest scaled value", weakest)
    if defect == "bwd_recompute":                                        # the forward is untouched by it
        assert all(w["y"] < fm.BOUND[T, "fp32"] for (_, _, T), (w, _) in hits.items())


def test_dropped_lo_parts_fail_this_metric_and_pass_the_old_one(survey):
    """The split-bf16 row passes with the lo parts of the trigonometric matrices and of the column results left out: 8 instead of 16
    mantissa bits per factor.  The norm-relative measure of test_fourier_gpu.py (1.5e-2 for bf16) does not see it; held per element it
    fails every case by at least twice the bound.  This is the defect the per-element bound exists for."""
    _, bad = survey
    hits = {k: v for k, v in bad.items() if k[0] == "lo_dropped"}
    assert len(hits) >= 40
    for (_, name, T), (w, old) in hits.items():
        assert max(w.values()) >= 2.0 * fm.BOUND[BF16, "split"], (name, w)
        assert max(old.values()) < OLD_TOL[BF16], (name, old)
    print("lo_dropped: weakest scaled %.1f, largest old-metric value %.2e" % (min(max(w.values()) for w, _ in hits.values()),
                                                                              max(max(o.values()) for _, o in hits.values())))


def test_failure_report_names_the_bin_that_carries_the_error():
    name, T = "bl16-W96", F32
    c, ref = fm.CASES[name], fm.reference_of(name, T)
    out = fm.emulate_case(name, T, "fp32", "unmixed")
    sel = torch.nonzero(fm.band(c.H, c.W, c.radius, c.high))
    kh, kw = (int(i) for i in sel[sel[:, 1] > 0][0])
    assert "bin (kh=%d, kw=%d)" % (kh, kw) in fm.explain(out["y"], ref["y"], ref["A1y"], T)
    out = fm.emulate_case(name, T, "fp32", "nyq_col_drop")
    assert "kw=%d)" % (c.W // 2) in fm.explain(out["y"], ref["y"], ref["A1y"], T)


# ---------------------------------------------------------------------------------------------------------------------------------
# routes (host only)
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cdll():
    from mrfp_amd import _lib, build
    build.build()
    return _lib.lib()


def test_table_routes_are_what_the_library_reports(cdll):
    if fm.active_switch() is not None:
        pytest.skip("an A/B switch is set: the table states the default routes")
    for name, T in fm.RUNS:
        c = fm.CASES[name]
        assert fm.routes_of(cdll, c, T) == c.expect[T], (name, fm.dname(T), fm.routes_of(cdll, c, T), c.expect[T])
    for c, T, exp in fm.SWITCH_TABLE:
        assert fm.routes_of(cdll, c, T) == exp[None], (c.name, fm.routes_of(cdll, c, T))


def test_table_is_complete(cdll):
    if fm.active_switch() is not None:
        pytest.skip("an A/B switch is set: the table states the default routes")
    fm.check_completeness(cdll)


def test_route_query_refuses_what_the_launch_refuses(cdll):
    q = lambda *a: cdll.mrfp_fourier_route(*a, None, None, None)
    assert q(99, 32, 32, 16, 3.0, 0, 0) < 0                    # dtype
    assert q(0, 32, 32, 24, 3.0, 0, 0) < 0                     # C % 16
    assert q(0, 10, 14, 16, 3.0, 0, 0) < 0 and q(0, 32, 14, 16, 3.0, 0, 0) < 0      # 14 = 2 * 7
    assert q(0, 32, 27, 16, 3.0, 0, 0) < 0                     # odd W
    assert q(0, 1024, 32, 16, 3.0, 0, 0) < 0
    assert q(0, 32, 32, 16, 3.0, 0, 3) < 0 and q(0, 32, 32, 16, 3.0, 0, 4) < 0     # three passes on the register path
    assert q(0, 32, 24, 16, 3.0, 0, 3) == fm.GENERIC
    kb, tu, nh = ctypes.c_int(-1), ctypes.c_int(-1), ctypes.c_int(-1)
    assert cdll.mrfp_fourier_route(1, 192, 192, 128, 16.0, 0, 2, ctypes.byref(kb), ctypes.byref(tu), ctypes.byref(nh)) == fm.MFMA
    assert (kb.value, tu.value, nh.value) == (3, 6, 2)          # the flagship plane: 17 stored bins, 12 tiles in items of 6
