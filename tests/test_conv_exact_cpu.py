"""No-GPU proof of the exact-data design of tests/conv_exact_common.py: a pass of tests/test_conv_exact_gpu.py means something.

For every case of every list the GPU file runs (the dense CASES, the weight-stationary and long-K lists, every problem of the grouped
weight gradients, the low-rank shapes, the depthwise list, the shape lists of the switch-forced kernels):
  * the conditions hold on the float64 reference (integer-valued, max|ref| inside the bf16 limit for outputs stored in the activation
    type and 2^24 for the fp32 weight gradients, sum of |terms| below 2^24 -- as the same convolution of |x| with |w| --, per-channel
    sum of ref^2 below 2^24 where statistics are taken);
  * an fp32 host evaluation in a scrambled summation order (taps and channel chunks in a random order, channels permuted, the weight
    gradient in split-K slabs) EQUALS the float64 reference;
  * every planted defect that exists for the case changes at least one element:
      product   one product dropped from one output element
      tap       one tap read from the horizontally adjacent pixel in one tile corner (16 channels x 2 output rows of image 0)
      ktile     the last K tile's remainder dropped: with K = taps x channels in [r][s][c] order, the entries past the last multiple
                of 32 below K (of the last tap that reads inside the image at all)
      pixel     one pixel lost from the weight gradient
      rowblock  one 64-row block missing from the statistics
      padding   a padding pixel read as its in-image neighbour (left edge, one filter row)            -- cases with padding
      parity    stride-2 dgrad with the parity classes (even row, even column) / (even row, odd column) exchanged  -- stride 2
"""
import pytest
import torch
import torch.nn.functional as F

import conv_exact_common as cx
from conv_exact_common import sid

BF16 = torch.bfloat16
SEEN = set()          # defects exercised by the last dense_checks calls (test_every_defect_is_exercised)


def differs(a, b):
    return not torch.equal(a.double(), b.double())


def first_product(x, w, stride, pad, dil, groups=1):
    """-> (b, n, oh, ow, product) of the first nonzero in-image product x * w of the forward sum, scanning outputs from the middle"""
    B, C, H, W = x.shape
    N, Cg, R, S = w.shape
    Ho, Wo = cx.out_size(H, R, stride, pad, dil), cx.out_size(W, S, stride, pad, dil)
    for oh in list(range(Ho // 2, Ho)) + list(range(Ho // 2)):
        for ow in list(range(Wo // 2, Wo)) + list(range(Wo // 2)):
            for r in range(R):
                for s in range(S):
                    ih, iw = oh * stride - pad + r * dil, ow * stride - pad + s * dil
                    if not (0 <= ih < H and 0 <= iw < W):
                        continue
                    for bi, n in [(bi, n) for bi in range(B if groups != 1 else 1) for n in range(N if groups != 1 else min(N, 4))]:
                        for c in ([n] if groups != 1 else range(Cg)):
                            p = float(x[bi, c, ih, iw]) * float(w[n, 0 if groups != 1 else c, r, s])
                            if p != 0.0:
                                return bi, n, oh, ow, p
    raise AssertionError("no nonzero product")


def dense_checks(label, d, stats, addend=None):
    """conditions, scrambled order, defects for one dense convolution (forward, dgrad unless it is the stem, wgrad)"""
    x, w, b, gy = d["x"], d["w"], d["b"], d["gy"]
    st, pad, dil = d["geom"]
    B, C, H, W = x.shape
    N, _, R, S = w.shape
    Ho, Wo = gy.shape[2], gy.shape[3]
    y = cx.ref_forward(x, w, b, st, pad, dil, addend=addend)
    cx.check_output(label + " y", y, cx.mag_forward(x, w, b, st, pad, dil, addend=addend), BF16)
    if stats:
        cx.check_stats(label + " stats", y)
    dw = cx.ref_wgrad(x, w.shape, gy, st, pad, dil)
    cx.check_output(label + " dw", dw, cx.mag_wgrad(x, w.shape, gy, st, pad, dil), torch.float32)
    if b is not None:
        cx.check_output(label + " db", cx.ref_dbias(gy), gy.abs().sum((0, 2, 3)), torch.float32)
    ya = y - addend.double() if addend is not None else y
    assert torch.equal(cx.scrambled_forward(x, w, b, st, pad, dil, seed=1).double(), ya), label
    assert torch.equal(cx.scrambled_wgrad(x, w.shape, gy, st, pad, dil, seed=2).double(), dw), label
    dx = None
    if C != 3:
        dx = cx.ref_dgrad(x.shape, w, gy, st, pad, dil)
        cx.check_output(label + " dx", dx, cx.mag_dgrad(x.shape, w, gy, st, pad, dil), BF16)
        assert torch.equal(cx.scrambled_dgrad(x.shape, w, gy, st, pad, dil, seed=3).double(), dx), label

    # ---- planted defects ----
    bb, n, oh, ow, p = first_product(x, w, st, pad, dil)
    bad = y.clone()
    bad[bb, n, oh, ow] -= p
    assert differs(bad, y)
    SEEN.add("product")

    xp = F.pad(x.double(), (pad, pad + 1, pad, pad))           # (one more column on the right: the neighbour of the last pixel)
    taps = [(r, s) for r in range(R) for s in range(S)
            if any(0 <= o * st - pad + r * dil < H for o in range(Ho)) and any(0 <= o * st - pad + s * dil < W for o in range(Wo))]
    r, s = taps[len(taps) // 2]
    nn, rows = min(16, N), min(2, Ho)
    good = torch.einsum("chw,nc->nhw", cx._tap_view(xp, r, s, dil, st, Ho, Wo)[0, :, :rows], w.double()[:nn, :, r, s])
    shifted = torch.einsum("chw,nc->nhw", cx._tap_view(xp[..., 1:], r, s, dil, st, Ho, Wo)[0, :, :rows], w.double()[:nn, :, r, s])
    bad = y.clone()
    bad[0, :nn, :rows] += shifted - good
    assert differs(bad, y), (label, "tap")
    SEEN.add("tap")

    K = R * S * C
    tail = K - (K - 1) // 32 * 32                              # entries past the last multiple of 32 below K (a whole tile when 32 | K)
    r, s = taps[-1]
    if tail <= C:
        delta = torch.einsum("bchw,nc->bnhw", cx._tap_view(xp, r, s, dil, st, Ho, Wo)[:, C - tail:], w.double()[:, C - tail:, r, s])
    else:                                                      # fewer than 32 channels (the stem): the tail spans several taps
        wt = w.double().permute(0, 2, 3, 1).reshape(N, K).clone()
        wt[:, :K - tail] = 0
        delta = F.conv2d(x.double(), wt.view(N, R, S, C).permute(0, 3, 1, 2), None, st, pad, dil)
    assert bool((delta != 0).any()), (label, "ktile")
    SEEN.add("ktile")

    lost = None
    for m in range(B * Ho * Wo - 1, -1, -1):
        bi, oh, ow = m // (Ho * Wo), m // Wo % Ho, m % Wo
        win = torch.zeros(C, R, S, dtype=torch.float64)
        for r in range(R):
            for s in range(S):
                ih, iw = oh * st - pad + r * dil, ow * st - pad + s * dil
                if 0 <= ih < H and 0 <= iw < W:
                    win[:, r, s] = x[bi, :, ih, iw].double()
        lost = gy[bi, :, oh, ow].double().view(N, 1, 1, 1) * win[None]
        if bool((lost != 0).any()):
            break
    assert lost is not None and differs(dw - lost, dw), (label, "pixel")
    SEEN.add("pixel")

    if stats:
        s0, q0 = cx.ref_stats(y)
        flat = y.permute(0, 2, 3, 1).reshape(B * Ho * Wo, N)
        blk = flat[-64:] if flat.shape[0] > 64 else flat[-1:]   # the last (partial) block: the one an epilogue's tail handling loses
        assert differs(q0.sum(0) - (blk * blk).sum(0), q0.sum(0)), (label, "rowblock")
        SEEN.add("rowblock")

    if pad > 0 and S > 1 and min(pad, W) >= 1:
        r = taps[len(taps) // 2][0]
        xrep = F.pad(F.pad(x.double(), (pad, 0, 0, 0), mode="replicate"), (0, pad + 1, pad, pad))
        cols = min(Wo, (pad + st - 1) // st)                   # the output columns whose tap s = 0 reads left of the image
        d0 = torch.einsum("bchw,nc->bnhw", cx._tap_view(xrep - xp, r, 0, dil, st, Ho, Wo)[..., :cols], w.double()[:, :, r, 0])
        assert bool((d0 != 0).any()), (label, "padding")
        SEEN.add("padding")

    if st == 2 and dx is not None:
        assert H % 2 == 0 and W % 2 == 0
        bad = dx.clone()
        bad[:, :, 0::2, 0::2], bad[:, :, 0::2, 1::2] = dx[:, :, 0::2, 1::2], dx[:, :, 0::2, 0::2]
        assert differs(bad, dx), (label, "parity")
        SEEN.add("parity")


@pytest.mark.parametrize("case", cx.CASES, ids=sid)
def test_dense_cases(case):
    d = cx.dense_data(case)
    dense_checks(sid(case), d, stats=not case[9])


@pytest.mark.parametrize("case", cx.C64_CASES + cx.C128_CASES, ids=sid)
def test_weight_stationary_cases(case):
    d = cx.c64_data(case)
    dense_checks(sid(case), d, stats=not case[6])
    st, pad, dil = d["geom"]
    ya = cx.ref_forward(d["x"], d["w"], None, st, pad, dil, addend=d["addend"])
    cx.check_output(sid(case) + " addend form", ya, cx.mag_forward(d["x"], d["w"], None, st, pad, dil, addend=d["addend"]), BF16)


@pytest.mark.parametrize("case", cx.PWK_CASES, ids=sid)
def test_long_k_cases(case):
    B, C, H, W, N = case
    d = cx.pwk_data(case)
    dense_checks(sid(case), d, stats=True)
    gate = cx.unpack_gate(d["gate_bits"], B, N, H, W)
    for g in (None, gate):
        ya = cx.ref_forward(d["x"], d["w"], None, addend=d["addend"], gate=g)
        cx.check_output(sid(case) + " addend form", ya, cx.mag_forward(d["x"], d["w"], None, addend=d["addend"]), BF16)
    assert differs(cx.ref_forward(d["x"], d["w"], None, addend=d["addend"], gate=gate), cx.ref_forward(d["x"], d["w"], None, addend=d["addend"]))


@pytest.mark.parametrize("case", cx.GROUP_CASES, ids=sid)
def test_grouped_weight_gradient_cases(case):
    """every problem of every group: conditions and the scrambled split-K sum; problems differ from one another (a grouped launch
    that wrote problem i's result into slot j would be seen)"""
    B, C, H, W, N, k, st, pad, dil, n = case
    refs = []
    for i in range(n):
        x, gy = cx.group_data(case, i)
        dw = cx.ref_wgrad(x, (N, C, k, k), gy, st, pad, dil)
        cx.check_output("%s problem %d dw" % (sid(case), i), dw, cx.mag_wgrad(x, (N, C, k, k), gy, st, pad, dil), torch.float32)
        if i in (0, n - 1):
            assert torch.equal(cx.scrambled_wgrad(x, (N, C, k, k), gy, st, pad, dil, seed=i).double(), dw)
        refs.append(dw)
    assert all(differs(refs[0], r) for r in refs[1:])


@pytest.mark.parametrize("case", cx.LOWRANK_CASES, ids=sid)
def test_low_rank_cases(case):
    B, C, H, W, N, dil = case
    d = cx.lowrank_data(case)
    prod = torch.einsum("bkhw,nk->bnhw", d["dp"].double(), d["wf"].double())
    cx.check_output(sid(case) + " product", prod, None, BF16)            # (rounded to the activation type before it is added: exact)
    cx.check_terms(sid(case), 32)
    y = cx.ref_forward(d["x"], d["w"], None, 1, dil, dil, addend=prod)
    cx.check_output(sid(case) + " y", y, cx.mag_forward(d["x"], d["w"], None, 1, dil, dil) + 32, BF16)
    assert differs(y, y - prod)


@pytest.mark.parametrize("case", cx.DW_CASES, ids=sid)
def test_depthwise_cases(case):
    B, C, H, W, s, dil = case
    d = cx.dw_data(case)
    x, w, b, gy = d["x"], d["w"], d["b"], d["gy"]
    label = sid(case)
    y = cx.ref_forward(x, w, None, s, dil, dil, groups=C)
    cx.check_output(label + " y", y, cx.mag_forward(x, w, None, s, dil, dil, groups=C), BF16)
    cx.check_output(label + " y + bias", cx.ref_forward(x, w, b, s, dil, dil, groups=C), None, BF16)
    cx.check_stats(label, y)
    dx = cx.ref_dgrad(x.shape, w, gy, s, dil, dil, groups=C)
    cx.check_output(label + " dx", dx, cx.mag_dgrad(x.shape, w, gy, s, dil, dil, groups=C), BF16)
    dw = cx.ref_wgrad(x, w.shape, gy, s, dil, dil, groups=C)
    cx.check_output(label + " dw", dw, cx.mag_wgrad(x, w.shape, gy, s, dil, dil, groups=C), torch.float32)
    sy, sdx, sdw = cx.scrambled_dw(x, w, gy, s, dil, seed=4)
    assert torch.equal(sy.double(), y) and torch.equal(sdx.double(), dx) and torch.equal(sdw.double(), dw), label
    # ReLU6 on integers: exact, and it gates something
    y6 = cx.ref_forward(x, w, b, s, dil, dil, groups=C, relu6=True)
    assert bool((y6 == y6.round()).all()) and float(y6.max()) <= 6 and float(y6.min()) >= 0
    # defects: a product, a lost pixel, a lost row of the statistics, a padding pixel read as its neighbour
    bb, n, oh, ow, p = first_product(x, w, s, dil, dil, groups=C)
    bad = y.clone()
    bad[bb, n, oh, ow] -= p
    assert differs(bad, y)
    xp = F.pad(x.double(), (dil, dil, dil, dil))
    Ho, Wo = gy.shape[2], gy.shape[3]
    views = [cx._tap_view(xp, t // 3, t % 3, dil, s, Ho, Wo) for t in range(9)]
    lost = [torch.stack([gy[bi, :, oh, ow].double() * v[bi, :, oh, ow] for v in views], 1).view(C, 1, 3, 3)
            for bi in range(B) for oh in range(Ho) for ow in range(Wo)]
    assert any(differs(dw - l, dw) for l in lost[::-1][:64]), (label, "pixel")
    if H * W > 1:
        xr = F.pad(F.pad(x.double(), (dil, 0, 0, 0), mode="replicate"), (0, dil, dil, dil))
        assert differs(F.conv2d(xr, w.double(), None, s, 0, dil, C), y), (label, "padding")
    q = cx.ref_stats(y)[1].sum(0)
    # (a row of a one-pixel image can be all zero over 8 channels: the row of SOME image must count)
    assert any(differs(q - (y[bi, :, -1] ** 2).sum(-1), q) for bi in range(B)), (label, "rowblock")


# (one entry per distinct shape list: the four tile switch sets share one; the 128-channel weight-stationary list is checked above)
_LISTS = {id(v[2]): k for k, v in sorted(cx.SWITCH_SETS.items(), reverse=True) if v[0] != "c64"}


@pytest.mark.parametrize("name", sorted(_LISTS.values()), ids=str)
def test_switch_forced_shape_lists(name):
    """the shape lists of the child processes: conditions on every case (their kernels differ, their arithmetic does not)"""
    kind, _env, shapes = cx.SWITCH_SETS[name]
    for sh in shapes:
        if kind == "dense":
            d = cx.dense_data(sh)
            st, pad, dil = d["geom"]
            y = cx.ref_forward(d["x"], d["w"], None, st, pad, dil)
            cx.check_output(sid(sh) + " y", y, cx.mag_forward(d["x"], d["w"], None, st, pad, dil), BF16)
            cx.check_stats(sid(sh), y)
            cx.check_output(sid(sh) + " dx", cx.ref_dgrad(d["x"].shape, d["w"], d["gy"], st, pad, dil),
                            cx.mag_dgrad(d["x"].shape, d["w"], d["gy"], st, pad, dil), BF16)
            cx.check_output(sid(sh) + " dw", cx.ref_wgrad(d["x"], d["w"].shape, d["gy"], st, pad, dil),
                            cx.mag_wgrad(d["x"], d["w"].shape, d["gy"], st, pad, dil), torch.float32)
        else:
            case, Ct, _T = cx.wgrad_child_case(kind, sh)
            B, C, H, W, N, k, st, pad, dil, n = case
            for i in (0, n - 1):
                x, gy = cx.group_data(case, i)
                x[:, Ct:] = 0
                dw = cx.ref_wgrad(x[:, :Ct], (N, Ct, k, k), gy, st, pad, dil)
                cx.check_output("%s problem %d" % (sid(sh[:6]), i), dw, cx.mag_wgrad(x[:, :Ct], (N, Ct, k, k), gy, st, pad, dil), torch.float32)


def test_every_defect_is_exercised():
    """a padded stride-2 bias-free case has all seven"""
    SEEN.clear()
    case = cx.CASES[5]
    assert case[6] == 2 and case[7] > 0 and not case[9]
    dense_checks(sid(case), cx.dense_data(case), stats=True)
    assert SEEN == {"product", "tap", "ktile", "pixel", "rowblock", "padding", "parity"}, SEEN


def test_mismatch_reporter_names_the_element():
    a = torch.zeros(2, 4, 5, 6)
    b = a.clone()
    b[1, 2, 3, 4] = 7
    msg = cx.mismatch("y", b, a)
    assert "1 of 240" in msg and "(b 1, ch 2, h 3, w 4) got 7 want 0" in msg and "row m = 52" in msg
    assert cx.mismatch("y", a, a.clone()) == ""


def test_bias_gradient_expression():
    """cx.ref_dbias_as_computed (mean times count, as ops.channel_sums forms it): the plain sum where the count is a power of two, and
    never further from it than the two fp32 roundings it states"""
    gy = cx.ternary((2, 8, 16, 16), 32, 5)
    assert torch.equal(cx.ref_dbias_as_computed(gy).double(), cx.ref_dbias(gy))
    gy = cx.ternary((2, 64, 20, 18), 32, 5)
    a, s = cx.ref_dbias_as_computed(gy).double(), cx.ref_dbias(gy)
    assert bool(((a - s).abs() <= 2.0 ** -22 * s.abs()).all())
