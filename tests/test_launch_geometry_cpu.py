"""No-GPU premises of tests/test_launch_geometry_gpu.py: every shape of tests/launch_geometry_common.py takes the launch path it
was chosen for, as the library's own host-only queries answer (mrfp_stats_nslab, mrfp_dwconv_nslab, mrfp_dwconv_wgrad_ws_bytes,
mrfp_ce_nblocks).  If a cap changes, this file fails; the GPU file would otherwise stay green while testing one line per workgroup
again."""
import pytest

import launch_geometry_common as lg
from mrfp_amd import _lib, build, ops

pytestmark = pytest.mark.skipif(lg.row_blocks_overridden(), reason=lg.SKIP_REASON)


@pytest.fixture(scope="module")
def cdll():
    build.build()
    return _lib.lib()


def nslab(cdll, B, rows):
    return int(cdll.mrfp_stats_nslab(B, rows))


def walk(rows, ly):
    """(lines of the busiest workgroup, lines of the idlest) when workgroup j walks lines j, j + ly, ..."""
    return lg.ceil_div(rows, ly), rows // ly


@pytest.mark.parametrize("name", sorted(lg.ROW_SHAPES))
def test_row_shapes_take_their_path(cdll, name):
    c = lg.ROW_SHAPES[name]
    B, C, H, W = c["shape"]
    ly = nslab(cdll, B, H)
    assert ly == c["ly"], (name, ly)
    most, least = walk(H, ly)
    if c["lines"] == "multi":
        assert B * H > lg.ROW_CAP and ly < H and most >= 2
    else:
        assert ly == H and most == 1                      # one line per workgroup: separates the finalize body from the line loop
    assert (H % ly != 0) == c["uneven"] and (most != least) == c["uneven"]
    assert (B * ly > 3 * lg.KFL) == c["bn_body"]          # reduce_partials over B * ly rows: unrolled body
    assert (ly > 3 * lg.KFL) == c["in_body"]              # ... over the ly rows of one image
    if c["in_body"]:
        assert ly > 3 * lg.KIL                            # in_bwd_finalize_kernel: its own 4 x kIL body
    for dtype in c["dtypes"]:
        vec, lpr, col, rowt = lg.lanes(C, dtype)
        assert (lpr > 256) == c["lpr_over_256"], (name, dtype, lpr)
    # image by image (the bit-identity checks): one line per workgroup
    assert nslab(cdll, 1, H) == H


def test_row_shapes_cover_what_the_issue_lists(cdll):
    s = lg.ROW_SHAPES
    # (16, 8, 161, 5): workgroups 0..79 walk two lines, workgroup 80 one; 1296 partial rows = the unrolled body twice and a tail
    B, C, H, W = s["two_lines_uneven"]["shape"]
    ly = nslab(cdll, B, H)
    assert ly == 81 and [len(range(j, H, ly)) for j in range(ly)] == [2] * 80 + [1]
    n, p, body = B * ly, 0, 0
    while p + 3 * lg.KFL < n:
        p, body = p + 4 * lg.KFL, body + 1
    assert n == 1296 and body == 2 and p < n                  # lane 0: two trips of the body, then the tail
    # (24, 64, 130, 3): cap 85, 2 lines each
    assert lg.ROW_CAP // 24 == 85 and walk(130, nslab(cdll, 24, 130)) == (2, 2)
    # (2, 19, 1100, 3): the scalar (VEC = 1) kernels
    for dtype in s["scalar_c19"]["dtypes"]:
        assert lg.lanes(19, dtype)[0] == 1
    assert lg.lanes(2048, lg.F32)[1] == 512                   # the cv0 loop runs twice
    assert any(c["lines"] == "single" and c["in_body"] for c in s.values())
    assert any(c["lines"] == "multi" and c["in_body"] for c in s.values())


@pytest.mark.parametrize("name", sorted(lg.RESIZE_CASES))
def test_resize_cases_walk_several_output_lines(cdll, name):
    c = lg.RESIZE_CASES[name]
    B, C, H, W = c["shape"]
    Ho = ops.nearest_out_size(H, c["rs"]["scale"])
    assert Ho == c["Ho"] and B * Ho > lg.ROW_CAP
    assert nslab(cdll, B, Ho) == c["ly_out"] < Ho             # statistics / apply: output lines
    assert nslab(cdll, B, H) == c["ly_in"]                    # backward apply: input lines
    assert any(nslab(cdll, v["shape"][0], v["shape"][2]) < v["shape"][2] for v in lg.RESIZE_CASES.values())


@pytest.mark.parametrize("name", sorted(lg.BILINEAR_CASES))
def test_bilinear_cases(cdll, name):
    c = lg.BILINEAR_CASES[name]
    B, C, Hi, Wi = c["shape"]
    Ho, Wo = c["size"]
    assert nslab(cdll, B, Ho) == c["ly_fwd"] and nslab(cdll, B, Hi) == c["ly_bwd"]
    assert (c["ly_fwd"] < Ho) == (name == "up") and (c["ly_bwd"] < Hi) == (name == "down")


@pytest.mark.parametrize("name", sorted(lg.POOL_SHAPES))
def test_pool_shapes(cdll, name):
    c = lg.POOL_SHAPES[name]
    B, C, H, W = c["shape"]
    Ho = (H - 1) // 2 + 1
    assert nslab(cdll, B, Ho) == c["ly_fwd"] < Ho and Ho % c["ly_fwd"] != 0
    assert nslab(cdll, B, H) == c["ly_bwd"] < H and walk(H, c["ly_bwd"])[0] >= 3


def test_trip_cases():
    idle = False
    for name, c in lg.TRIP_CASES.items():
        B, C, H, W = c["shape"]
        vec, lpr, col, rowt = lg.lanes(C, c["dtype"])
        assert 4 * rowt == c["trip"], name
        assert W // c["trip"] == c["full"] >= 1 and W % c["trip"] == c["rest"] > 0, name
        assert (c["rest"] < rowt) == c["idle_threads"], name
        idle = idle or c["idle_threads"]
    assert idle                                               # some row threads get no pixel in the last trip


def _strips(rows, n):
    per = lg.ceil_div(rows, n)
    return (n, per, rows - (n - 1) * per)


@pytest.mark.parametrize("name", sorted(lg.DW_CASES))
def test_depthwise_cases_run_multi_row_strips(cdll, name):
    c = lg.DW_CASES[name]
    B, C, H = c["B"], c["C"], c["H"]
    for dtype in c["dtypes"]:
        code, Cp = _lib._DT[dtype], lg.dw_pitch(C, dtype)
        assert lg.ceil_div(Cp // (16 // (4 if dtype == lg.F32 else 2)), 32) == c["nchunk"]
        for stride in (1, 2):
            want = c["s%d" % stride]
            Ho = (H - 1) // stride + 1
            fwd = int(cdll.mrfp_dwconv_nslab(code, B, Ho, Cp))
            dg = int(cdll.mrfp_dwconv_nslab(code, B, H, Cp))         # the dgrad launch strips the H input rows by the same rule
            nbytes = int(cdll.mrfp_dwconv_wgrad_ws_bytes(code, B, Ho, Cp))
            assert nbytes % (B * 9 * Cp * 4) == 0
            wg = nbytes // (B * 9 * Cp * 4)
            assert _strips(Ho, fwd) == want["fwd"], (name, dtype, stride, _strips(Ho, fwd))
            assert _strips(Ho, wg) == want["wg"], (name, dtype, stride, _strips(Ho, wg))
            assert _strips(H, dg) == want["dg"], (name, dtype, stride, _strips(H, dg))
            assert wg < Ho and dg < H                                # several rows per strip
    if name != "c960_f32":
        assert all(c["s%d" % s]["fwd"][1] >= 2 for s in (1, 2))
    assert c["s1"]["fwd"][1] >= 2


def test_depthwise_table_as_a_whole(cdll):
    d = lg.DW_CASES
    assert d["c960_f32"]["s1"]["fwd"] == (21, 2, 1) and d["c960_f32"]["s1"]["wg"] == (14, 3, 2)      # shorter last strip
    assert any(c["s2"]["fwd"][1] >= 2 for c in d.values() if lg.F32 in c["dtypes"])                  # strided forward, fp32
    assert any(c["s2"]["fwd"][1] >= 2 for c in d.values() if lg.BF16 in c["dtypes"])
    assert lg.dw_pitch(12, lg.BF16) == 16
    name, stride = lg.DW_STATS_CASE
    c = d[name]
    Ho = (c["H"] - 1) // stride + 1
    n = int(cdll.mrfp_dwconv_nslab(_lib.BF16, c["B"], Ho, c["C"]))
    assert n < Ho and c["B"] * n > 3 * lg.KFL                 # statistics rows [B][nslab < Ho]; bn_finalize's unrolled body


def test_loss_cases_are_above_the_grid_cap(cdll):
    for c in (lg.CE_CASE, lg.UPCE_CASE):
        npix = c["B"] * c["H"] * c["W"]
        assert int(cdll.mrfp_ce_nblocks(npix)) == lg.CE_CAP
        assert npix > lg.CE_CAP * lg.CE_THREADS and npix % lg.CE_THREADS != 0
        assert npix < 2 * lg.CE_CAP * lg.CE_THREADS           # just above: some threads take two pixels, most one
    assert int(cdll.mrfp_ce_nblocks(lg.CE_CAP * lg.CE_THREADS)) == lg.CE_CAP
    assert int(cdll.mrfp_ce_nblocks(lg.CE_CAP * lg.CE_THREADS - 256)) == lg.CE_CAP - 1
