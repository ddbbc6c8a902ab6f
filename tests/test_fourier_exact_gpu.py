"""Every kernel route of mrfp_fourier_mix (csrc/fft.hip), forward and backward through ops.fourier_amplitude_mix, held per element
against the float64 definition: inputs, reference, metric, bounds and the case table are those of tests/fourier_model_common.py
(proved on the host by tests/test_fourier_model_cpu.py).  Every case first asserts, through mrfp_fourier_route, that its three
passes take the kernels the table says, then runs; test_table_is_complete proves from the same query that the table reaches every
instance a call can reach.  The A/B switches (read once per process) run a short sub-table in fresh child processes, one after
another.

Largest scaled values the device produced over the table, per route of the two row passes and type (test_zz_report prints them
with -s; the bound is fourier_model_common.BOUND of the arithmetic class):

    rows forward / inverse              type          y       dx   bound
    generic                             float32     0.718    0.840     2
    generic                             bfloat16    0.995    0.995     2
    generic                             float16     0.993    0.997     2
    two-step, whole spectrum            float32     0.451    0.574     2
    two-step, whole spectrum            bfloat16    0.995    0.995     2
    two-step, whole spectrum            float16     0.994    0.996     2
    two-step / two-step, band-limited   float32     0.117    0.118     2
    two-step / two-step, band-limited   bfloat16    0.995    0.995     2
    two-step / two-step, band-limited   float16     0.993    0.995     2
    pair / pair, band-limited           float32     0.163    0.207     2
    pair / pair, band-limited           bfloat16    0.995    0.995     2
    pair / pair, band-limited           float16     0.997    0.994     2
    pair / direct, band-limited         float32     0.184    0.210     2
    pair / direct, band-limited         bfloat16    0.995    0.996     2
    pair / direct, band-limited         float16     0.995    0.996     2
    mfma / mfma, band-limited           bfloat16    1.248    1.394     3

(16-bit values just below 1 are the one rounding to T.)  Under the A/B switches the sub-table reached at most 0.995 (16-bit) and 0.493
(fp32, MRFP_FFT_GENERIC=1).
"""
import os
import subprocess
import sys

import pytest
import torch

import fourier_model_common as fm
from fourier_model_common import BF16, F16, F32  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_LIMIT = 300            # seconds per child process (a cold start of the interpreter and the runtime is most of it)

SEEN = {}                    # (label of the row routes, type) -> [largest scaled y, largest scaled dx, bound]


@pytest.fixture(scope="module")
def cdll():
    from mrfp_amd import _lib
    return _lib.lib()


def label(lib, c, routes):
    full = int(lib.mrfp_fourier_stored_bins(c.H, c.W, c.radius, int(c.high))) == c.W // 2 + 1
    if routes[0][0] == fm.GENERIC:
        return "generic"
    if full:
        return "two-step, whole spectrum"
    return "%s / %s, band-limited" % (fm.ROUTE_NAMES[routes[0][0]], fm.ROUTE_NAMES[routes[2][0]])


def device_run(c, T, x, gy):
    from mrfp_amd import ops
    xd = x.to(T).to(DEV).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    y = ops.fourier_amplitude_mix(xd, torch.tensor(c.perm), c.radius, c.lam, c.high)
    y.backward(gy.to(T).to(DEV).contiguous(memory_format=torch.channels_last))
    return y.detach().cpu(), xd.grad.cpu()


def hold(lib, c, T, routes):
    """Runs the case on the device and holds y and dx to the bound of its arithmetic class."""
    ref = fm.reference_of(c.name, T)
    fm.check_conditioning(ref, c.lam)
    x, gy = fm.inputs(c.name, T)
    y, dx = device_run(c, T, x, gy)
    assert y.dtype == T and dx.dtype == T
    bound = fm.BOUND[T, fm.route_class(routes)]
    got = dict(y=fm.scaled(y, ref["y"], ref["A1y"], T), dx=fm.scaled(dx, ref["dx"], ref["A1dx"], T))
    rec = SEEN.setdefault((label(lib, c, routes), fm.dname(T)), [0.0, 0.0, bound])
    rec[0], rec[1] = max(rec[0], got["y"]), max(rec[1], got["dx"])
    print("%s %s scaled y %.3f dx %.3f (bound %d)" % (c.name, fm.dname(T), got["y"], got["dx"], bound))
    assert got["y"] < bound, fm.explain(y, ref["y"], ref["A1y"], T)
    assert got["dx"] < bound, fm.explain(dx, ref["dx"], ref["A1dx"], T)
    return y, dx


def test_table_routes_are_what_the_library_reports(cdll):
    if fm.active_switch() is not None:
        pytest.skip("an A/B switch is set: the table states the default routes")
    for name, T in fm.RUNS:
        c = fm.CASES[name]
        assert fm.routes_of(cdll, c, T) == c.expect[T], (name, fm.dname(T), fm.routes_of(cdll, c, T), c.expect[T])


def test_table_is_complete(cdll):
    """reachable instance set == tested instance set, by enumeration through mrfp_fourier_route (fourier_model_common.check_completeness)."""
    if fm.active_switch() is not None:
        pytest.skip("an A/B switch is set: the table states the default routes")
    fm.check_completeness(cdll)


@pytest.mark.parametrize("run", fm.RUNS, ids=fm.run_id)
def test_fourier_mix_exact(cdll, run):
    name, T = run
    c = fm.CASES[name]
    routes = fm.routes_of(cdll, c, T)
    if fm.active_switch() is None:
        assert routes == c.expect[T], (routes, c.expect[T])
    y, dx = hold(cdll, c, T, routes)
    if name in ("edge-identity", "edge-lam0") and fm.active_switch() is None:
        # band-limited routes write y = x + irfft2(F (ratio - 1)): the ratio of an identity mix is ((1 - lam) a + lam a') / a with a' = a
        # or lam = 0, exactly 1 in fp32, so the correction is exactly zero and the output is the input bit for bit (the backward
        # loads the same ratio).  (edge-identity-full takes the whole-spectrum route: the input within the bound, above.)
        x, gy = fm.inputs(name, T)
        assert torch.equal(y.double(), x) and torch.equal(dx.double(), gy)


@pytest.mark.parametrize("entry", fm.SWITCH_TABLE, ids=lambda e: "%s-%s" % (e[0].name, fm.dname(e[1])))
def test_switch_subtable(cdll, entry):
    """The sub-table the A/B switches are held on.  Its expected routes depend on the switch this process runs under (none: the default
    routes), so the same test proves, in a child process of test_ab_switches, that the switch took effect -- and holds the kernels
    the switch selects to the same bounds."""
    c, T, expect = entry
    routes = fm.routes_of(cdll, c, T)
    assert routes == expect[fm.active_switch()], (fm.active_switch(), routes, expect[fm.active_switch()])
    if fm.active_switch() == "MRFP_FFT_GENERIC":
        assert fm.routes_of(cdll, c, T, (3,)) == (fm._G,)
    hold(cdll, c, T, routes)


def test_ab_switches_select_live_kernels_that_hold_the_same_bounds():
    """MRFP_FFT_GENERIC / _FULL / _NOPAIR / _NODIRECT = 1 and MRFP_FFT_MFMA = 0 are what the tools compare a fast route with.  The
    library reads them once, so each runs test_switch_subtable in a fresh child process: one child at a time, each with its one
    switch and under its own time limit; after a child that does not end cleanly no further child is started."""
    if fm.active_switch() is not None:
        pytest.skip("already running under an A/B switch")
    for name, value in fm.SWITCHES:
        env = dict(os.environ)
        env[name] = value
        cmd = [sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-s", "-p", "no:cacheprovider", "-k", "test_switch_subtable"]
        try:
            r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=CHILD_LIMIT)
        except subprocess.TimeoutExpired as e:
            pytest.fail("%s=%s: the child ran into its time limit; no further child started\n%s" % (name, value, str(e.stdout or "")[-2000:]))
        tail = (r.stdout + r.stderr)[-4000:]
        assert r.returncode == 0, "%s=%s: the child ended with status %d; no further child started\n%s" % (name, value, r.returncode, tail)
        assert "%d passed" % len(fm.SWITCH_TABLE) in r.stdout, tail
        assert any(e[name] != e[None] for _, _, e in fm.SWITCH_TABLE), name     # (the child asserted these routes: the switch took effect)
        print("%s=%s: %s" % (name, value, r.stdout.strip().splitlines()[-1]))
        print("\n".join("    " + line for line in r.stdout.splitlines() if " scaled y " in line))


def test_zz_report():
    """The largest scaled value per route and type of this session (run with -s to see it)."""
    print("\n%-34s %-9s %8s %8s %6s" % ("rows forward / inverse", "type", "y", "dx", "bound"))
    for (lab, t), (vy, vdx, b) in sorted(SEEN.items()):
        print("%-34s %-9s %8.3f %8.3f %6d" % (lab, t, vy, vdx, b))
        assert vy < b and vdx < b
