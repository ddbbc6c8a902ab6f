"""No-GPU checks of the multi-scale / flipped / sliding-window evaluation: the window grid and the destination rectangles (host
arithmetic shared by harness.evaluate_tta and the restatement), the two new prototypes of the C ABI, argument errors, and the
restatement against a hand-computed case."""
import ctypes

import pytest
import torch

from mrfp_amd import _lib, build, harness

import eval_tta_common as etc


def _covered(H, W, rects):
    c = torch.zeros(H, W, dtype=torch.int32)
    for y, x, h, w in rects:
        assert 0 <= y and 0 <= x and h >= 1 and w >= 1 and y + h <= H and x + w <= W, (H, W, (y, x, h, w))
        c[y:y + h, x:x + w] += 1
    return c


def test_window_grid_hand_written_cases():
    g = harness.window_grid
    # window larger than the image: one window of the image's own size
    assert g(50, 70, (96, 96)) == [(0, 0, 50, 70)]
    # larger in one dimension only
    assert g(50, 200, (96, 96), (64, 64)) == [(0, 0, 50, 96), (0, 64, 50, 96), (0, 104, 50, 96)]
    # exact fit
    assert g(96, 96, (96, 96)) == [(0, 0, 96, 96)]
    assert g(96, 192, (96, 96), (96, 96)) == [(0, 0, 96, 96), (0, 96, 96, 96)]
    # one-pixel remainder: the last window is shifted back by stride - 1
    assert g(96, 97, (96, 96), (64, 64)) == [(0, 0, 96, 96), (0, 1, 96, 96)]
    assert g(193, 96, (96, 96), (96, 96)) == [(0, 0, 96, 96), (96, 0, 96, 96), (97, 0, 96, 96)]
    # stride == window, no remainder: a partition
    assert g(4, 6, (2, 3), (2, 3)) == [(0, 0, 2, 3), (0, 3, 2, 3), (2, 0, 2, 3), (2, 3, 2, 3)]
    assert int(_covered(4, 6, g(4, 6, (2, 3), (2, 3))).max()) == 1
    # default stride: two thirds of the window, rounded up
    assert g(96, 224, (96, 96)) == [(0, 0, 96, 96), (0, 64, 96, 96), (0, 128, 96, 96)]
    assert g(100, 100, (10, 10)) == g(100, 100, (10, 10), (7, 7))
    # no window: the whole image
    assert g(33, 44) == [(0, 0, 33, 44)]


def test_window_grid_covers_every_pixel_and_stays_inside():
    for H, W in ((1, 1), (5, 300), (96, 96), (97, 95), (120, 168), (160, 224), (200, 280), (333, 257)):
        for win in ((96, 96), (64, 128), (7, 5), (1, 1)):
            for stride in (None, win, (1, 1), (max(1, win[0] // 2), max(1, 2 * win[1] // 3))):
                rects = harness.window_grid(H, W, win, stride)
                assert int(_covered(H, W, rects).min()) >= 1, (H, W, win, stride)
                assert all(h == min(win[0], H) and w == min(win[1], W) for _, _, h, w in rects)
                if H <= win[0] and W <= win[1]:
                    assert rects == [(0, 0, H, W)]


def test_dest_rectangles_tile_the_destination():
    """start rounded down, end rounded up: no gap in the accumulator whatever the scale; identity at equal sizes."""
    assert harness.window_dest_rect((3, 5, 7, 9), (20, 30), (20, 30)) == (3, 5, 7, 9)
    assert harness.window_dest_rect((0, 0, 120, 168), (120, 168), (160, 224)) == (0, 0, 160, 224)
    assert harness.window_dest_rect((24, 72, 96, 96), (120, 168), (160, 224)) == (32, 96, 128, 128)
    assert harness.window_dest_rect((1, 1, 3, 3), (10, 10), (7, 7)) == (0, 0, 3, 3)      # floor(.7) = 0, ceil(2.8) = 3
    for (H, W), (Hd, Wd) in (((160, 224), (160, 224)), ((160, 224), (128, 192)), ((97, 131), (160, 224))):
        for s in (0.5, 0.75, 1.0, 1.25, 1.75, 2.0):
            vs = harness.tta_variants(H, W, (Hd, Wd), (s,), True, (96, 96), None)
            assert all(v[1] == (max(1, round(H * s)), max(1, round(W * s))) for v in vs)
            assert [v[2] for v in vs[:2]] == [False, True]
            assert int(_covered(Hd, Wd, [v[4] for v in vs]).min()) >= 2


def test_new_prototypes_declared_and_exported():
    build.build()
    protos = _lib.parse_header()
    cdll = _lib.lib()
    assert protos["mrfp_prob_accum"][0] is ctypes.c_int and len(protos["mrfp_prob_accum"][1]) == 18
    assert protos["mrfp_prob_accum"][1][16] is ctypes.c_float and protos["mrfp_prob_accum"][1][-1] is ctypes.c_void_p
    assert _lib.ARG_NAMES["mrfp_prob_accum"][-3:] == ["flip", "weight", "stream"]
    assert protos["mrfp_acc_argmax_hist"][0] is ctypes.c_int and len(protos["mrfp_acc_argmax_hist"][1]) == 9
    for name in ("mrfp_prob_accum", "mrfp_acc_argmax_hist"):
        assert hasattr(cdll, name), name
    # argument validation happens on the host before any launch
    assert cdll.mrfp_prob_accum(None, 0, 1, 1, 1, 19, None, None, 1, 1, 19, 0, 0, 1, 1, 0, 1.0, None) != 0
    assert b"prob_accum" in cdll.mrfp_last_error()
    assert cdll.mrfp_acc_argmax_hist(None, None, None, 0, 19, None, None, None, None) != 0
    assert b"acc_argmax_hist" in cdll.mrfp_last_error()


def test_ops_refuse_host_tensors():
    from mrfp_amd import ops
    acc, cnt = torch.zeros(1, 4, 4, 19), torch.zeros(1, 4, 4)
    z = etc.nhwc_logits(1, 19, 2, 2, torch.float32, 0)
    with pytest.raises(_lib.MrfpHipError):
        ops.prob_accum(z, acc, cnt)
    with pytest.raises(_lib.MrfpHipError):
        ops.acc_argmax_hist(acc, cnt, torch.zeros(1, 4, 4, dtype=torch.int64))


@pytest.mark.parametrize("kw", [dict(scales=()), dict(scales=(1.0, 0.0)), dict(scales=(-0.5,)),
                                dict(window=(96, 96), stride=(97, 96)), dict(window=(96, 96), stride=(64, 128)),
                                dict(window=(0, 96)), dict(window=(96, 96), stride=(0, 1)), dict(stride=(64, 64))])
def test_evaluate_tta_argument_errors(kw):
    model = torch.nn.Conv2d(3, 19, 1)          # never called: the arguments are checked first
    with pytest.raises(ValueError):
        harness.evaluate_tta(model, [], **kw)


def test_restatement_by_hand():
    """2 classes, a 1 x 2 map resized to 1 x 3 with a flip: columns (b, (a+b)/2, a)."""
    z = torch.tensor([[[[0.0, 2.0]], [[0.0, 0.0]]]])                 # class 0: (0, 2), class 1: (0, 0)
    acc, cnt = torch.zeros(1, 1, 4, 2, dtype=torch.float64), torch.zeros(1, 1, 4, dtype=torch.float64)
    etc.accum_restated(z, 2, acc, cnt, rect=(0, 1, 1, 3), flip=True, weight=0.5)
    sig = lambda v: 1.0 / (1.0 + torch.exp(torch.tensor(-v, dtype=torch.float64)))      # noqa: E731
    want = torch.stack([torch.tensor(0.0, dtype=torch.float64), 0.5 * sig(2.0), 0.5 * sig(1.0), 0.5 * sig(0.0)])
    assert torch.allclose(acc[0, 0, :, 0], want, atol=1e-15, rtol=0)
    assert torch.equal(cnt[0, 0], torch.tensor([0.0, 0.5, 0.5, 0.5], dtype=torch.float64))
    assert torch.allclose(acc.sum(-1), cnt, atol=1e-15, rtol=0)
