"""Per-kernel parity: every HIP kernel (through the C-ABI) against the CPU oracle (oracle/kernels_ref.py,
torch CPU fp32) on seeded inputs.  fp32 mode must hold 1e-4 (exact-fp32 MFMA, summation order only);
bf16 mode is checked against the oracle fed the SAME bf16-rounded inputs (tolerance = bf16 output rounding)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import kernels_ref as R  # noqa: E402
import _f64 as B  # noqa: E402
from kernel_routes import ROUTES  # noqa: E402


def _k():
    from ssl_cr_histo_amd import kernels as K
    return K


DEV = "cuda:0"
TOL = {0: 2e-4, 1: 1.2e-2}


def rnd(seed, shape, scale=1.0):
    return torch.from_numpy(np.random.RandomState(seed).standard_normal(shape).astype(np.float32) * scale)


def to_dev(t, dtype):
    K = _k()
    return t.to(DEV).to(K.tdtype(dtype)).contiguous()


def q(t, dtype):
    """round-trip through the engine storage dtype (so the oracle sees the same operand values)."""
    return t.to(torch.bfloat16).float() if dtype == 1 else t.float()


def close(got, want, tol, what=""):
    got = got.detach().float().cpu()
    want = want.detach().float().cpu()
    err = (got - want).abs().max().item()
    scale = want.abs().max().item() + 1e-20
    assert err <= tol * scale, f"{what}: max err {err:.3e} vs scale {scale:.3e} (rel {err / scale:.2e} > {tol})"


def test_probe_tr16():
    """ds_read_b64_tr_b16: out lane i elem j <- in lane (4j + i/4) elem (i%4), per 16-lane group."""
    from ssl_cr_histo_amd import _lib as L
    img = torch.arange(1024, dtype=torch.int16, device=DEV)
    # canonical: group g reads the [4][16] block at rows 4g..4g+3 of a [16][64]-element image; lane i' -> row i'>>2, cols 4*(i'&3)
    lane = torch.arange(64)
    g, i = lane // 16, lane % 16
    addr = (((4 * g + (i >> 2)) * 64 + (i & 3) * 4) * 2).to(torch.int32).to(DEV)
    out = torch.zeros((64, 4), dtype=torch.int16, device=DEV)
    L.check(L.lib().sslcr_probe_tr16(L.ptr(img), L.ptr(addr), L.ptr(out), L.stream_ptr()))
    torch.cuda.synchronize()
    want = torch.zeros((64, 4), dtype=torch.int16)
    for l in range(64):
        for j in range(4):
            want[l, j] = (4 * (l // 16) + j) * 64 + (l % 16)      # row j of the group's block, column i
    assert torch.equal(out.cpu(), want), out.cpu()[:20]


CONV_CASES = [
    # N, H, W, C, K, R, stride, pad
    (2, 16, 16, 64, 64, 3, 1, 1),
    (3, 9, 11, 64, 128, 3, 2, 1),      # ragged M, stride 2
    (2, 8, 8, 128, 256, 1, 2, 0),      # 1x1 downsample
    (1, 8, 8, 256, 256, 3, 1, 1),
    (40, 32, 32, 64, 64, 3, 1, 1),     # M = 40960 < 65536 -> 64-pixel tiles ; many tiles
    (72, 32, 32, 64, 128, 3, 1, 1),    # M = 73728 -> 128-pixel tiles, K=128 config
    (70, 32, 32, 64, 64, 3, 1, 1),     # 128x64 config
    (2, 8, 8, 512, 512, 3, 1, 1),      # halo kernel, 8-wide rows (2 images per tile), 8 channel slabs, BKO 128
    (4, 8, 8, 64, 64, 3, 1, 1),        # halo kernel, 8-wide, single slab
    (320, 8, 8, 64, 512, 3, 1, 1),     # 80 tiles x 4 kout blocks = 320 items on 256 CUs: the last 64 run as 64-kout half-items (a second launch)
    (2, 16, 32, 128, 128, 3, 1, 1),    # halo kernel, 16-wide, 2 slabs
    (3, 24, 48, 64, 128, 3, 1, 1),     # halo kernel, several tiles per image
    (4, 8, 8, 512, 512, 3, 1, 1),      # 256-pixel halo kernel, 4 images x 8x8, 8 slabs
    (2, 32, 32, 128, 256, 3, 1, 1),    # 256-pixel halo kernel, 16x16 tiles, 2 slabs
    (33, 32, 32, 64, 256, 3, 1, 1),    # persistent h16: 264 items > 256 workgroups, a workgroup walks into the next kout block
    (10, 30, 34, 64, 128, 3, 2, 1),    # all-DMA gather conv: stride 2, ragged M = 2550, 128x128 tiles
    (10, 30, 34, 128, 64, 3, 2, 1),    # all-DMA gather conv: 256x64 tiles, 2 channel slabs
    (9, 32, 32, 64, 128, 1, 2, 0),     # all-DMA gather conv: 1x1/2 projection
    (6, 64, 64, 64, 128, 3, 2, 1),     # plane-gather stride-2 conv (bf16; fp32 stays on the gather kernel): 4 tiles per image, one slab
    (9, 32, 32, 128, 256, 3, 2, 1),    # ... one tile per image, 2 slabs, 2 kout blocks on 18 workgroups (kout-block-fastest walk)
    (70, 64, 64, 64, 128, 3, 2, 1),    # ... 280 items on 256 workgroups: a workgroup walks into a second item
    (6, 32, 64, 256, 384, 3, 2, 1),    # ... 4 slabs, 3 kout blocks (kout-block-major walk), 2 tiles per image side by side
]


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("case", CONV_CASES)
def test_conv_fwd_raw_stats(case, dtype):
    K = _k()
    N, H, W, C, Ko, Rr, stride, pad = case
    x = q(rnd(1, (N, H, W, C)), dtype)
    w = q(rnd(2, (Ko, Rr, Rr, C), 0.05), dtype)
    y, stats = K.conv2d(to_dev(x, dtype), to_dev(w, dtype), stride, pad, want_stats=True)
    # the shapes added for a specific kernel must actually be served by it
    expect = {(33, 32, 32, 64, 256, 3, 1, 1): "conv3x3_h16_kernel", (10, 30, 34, 64, 128, 3, 2, 1): "conv_dma_kernel",
              (10, 30, 34, 128, 64, 3, 2, 1): "conv_dma_kernel", (9, 32, 32, 64, 128, 1, 2, 0): "conv_dma_kernel",
              (4, 8, 8, 512, 512, 3, 1, 1): ", 8>", (320, 8, 8, 64, 512, 3, 1, 1): ", 8>"}.get(case)   # conv3x3_h16<..., 8>: four-image tiles
    if expect:
        assert expect in K.last_conv_kernel, K.last_conv_kernel
    if case[1] % 32 == 0 and case[2] % 32 == 0 and Rr == 3 and stride == 2 and Ko % 128 == 0:
        assert ("conv_s2_kernel<false, false>" if dtype == 1 else "conv_dma_kernel<float") in K.last_conv_kernel, K.last_conv_kernel
    if case == (70, 32, 32, 64, 64, 3, 1, 1) and dtype == 1:      # 280 tiles on 256 workgroups: the resident-filter walk
        assert "conv3x3_pp64_kernel<false, 0>" in K.last_conv_kernel, K.last_conv_kernel
    want = R.conv_fwd(x, w, stride, pad)
    close(y, want, TOL[dtype], "conv raw")
    s, ss = R.channel_stats(want)
    st = stats.double().sum(0).cpu()
    close(st[0], s, 2e-4 if dtype == 0 else 2e-3, "sum")
    close(st[1], ss, 2e-4 if dtype == 0 else 2e-3, "sumsq")


@pytest.mark.parametrize("mode", ["train", "eval"])
@pytest.mark.parametrize("shape", [(6, 64, 64, 64, 128), (9, 32, 32, 128, 256), (70, 64, 64, 64, 128), (6, 32, 64, 256, 384), (130, 32, 32, 128, 256)])
def test_conv_s2_pair(shape, mode):
    """a downsampling block's conv1 (3x3 / 2) and 1x1 / 2 projection of one input in ONE launch (sslcr_conv2d_s2_pair, bf16): raw
    outputs + BatchNorm partial rows (train forward) and bias (+ ReLU on conv1) with the BatchNorm folded (eval forward)"""
    K = _k()
    N, H, W, C, Ko = shape
    x = q(rnd(41, (N, H, W, C)), 1)
    w3 = q(rnd(42, (Ko, 3, 3, C), 0.05), 1)
    w1 = q(rnd(43, (Ko, 1, 1, C), 0.1), 1)
    if mode == "train":
        # (routing: sslcr_conv2d_s2_pair has no other kernel behind it -- kernels.conv2d_s2_pair raises where sslcr_conv2d_s2_pair_ok
        #  says no; the single-conv train instance through the ordinary entry point is asserted by name below)
        y3, yd, s3, sd = K.conv2d_s2_pair(to_dev(x, 1), to_dev(w3, 1), to_dev(w1, 1), want_stats=True)
        y3s, s3s = K.conv2d(to_dev(x, 1), to_dev(w3, 1), 2, 1, want_stats=True)
        assert "conv_s2_kernel<false, false>" in K.last_conv_kernel, K.last_conv_kernel
        assert torch.equal(y3s, y3) and torch.equal(s3s, s3)
        for y, st, w, (r, pad) in ((y3, s3, w3, (3, 1)), (yd, sd, w1, (1, 0))):
            want = R.conv_fwd(x, w, 2, pad)
            close(y, want, TOL[1], f"raw {r}x{r}")
            s, ss = R.channel_stats(want)
            tot = st.double().sum(0).cpu()
            close(tot[0], s, 2e-3, "sum")
            close(tot[1], ss, 2e-3, "sumsq")
    else:
        b3, b1 = rnd(44, (Ko,)), rnd(45, (Ko,))
        y3, yd = K.conv2d_s2_pair(to_dev(x, 1), to_dev(w3, 1), to_dev(w1, 1), bias3=b3.to(DEV), bias1=b1.to(DEV), relu3=True)
        close(y3, R.conv_fwd(x, w3, 2, 1, bias=b3, relu=True), TOL[1], "eval 3x3")
        close(yd, R.conv_fwd(x, w1, 2, 0, bias=b1), TOL[1], "eval 1x1")
    # the single-conv instance through the ordinary entry point gives the same bits as the pair's first accumulator set
    if mode == "eval":
        y3s = K.conv2d(to_dev(x, 1), to_dev(w3, 1), 2, 1, bias=b3.to(DEV), relu=True)
        assert "conv_s2_kernel<false, true>" in K.last_conv_kernel, K.last_conv_kernel
        assert torch.equal(y3s, y3)


def test_conv_s2_relu_without_bias():
    """ReLU asked for WITHOUT a bias on a 3x3 / 2 shape the plane-gather kernel tiles: its output clamp lives in the EVAL
    instance, which the bias selects -- so the descriptor must go to the gather kernel, which honours relu on its own"""
    K = _k()
    N, H, W, C, Ko = 6, 64, 64, 64, 128
    x = q(rnd(46, (N, H, W, C)), 1)
    w3 = q(rnd(47, (Ko, 3, 3, C), 0.05), 1)
    y = K.conv2d(to_dev(x, 1), to_dev(w3, 1), 2, 1, relu=True)
    assert "conv_dma_kernel" in K.last_conv_kernel, K.last_conv_kernel
    close(y, R.conv_fwd(x, w3, 2, 1, relu=True), TOL[1], "relu without bias")
    assert float(y.float().min()) >= 0.0


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("shape", [(2, 12, 12, 128, 128), (2, 16, 16, 128, 128), (2, 8, 8, 256, 64), (4, 8, 8, 256, 128),
                                   (1, 24, 16, 64, 64), (320, 8, 8, 64, 512)])   # generic / h16 / halo128-8 / h16 four-image tiles / halo128-16 / four-image tiles in two launches
def test_conv_fwd_fused_prologue_epilogue(shape, dtype):
    K = _k()
    N, H, W, C, Ko = shape
    x = q(rnd(3, (N, H, W, C)), dtype)
    w = q(rnd(4, (Ko, 3, 3, C), 0.05), dtype)
    sc, sh = rnd(5, (C,)).abs() + 0.5, rnd(6, (C,))
    bias = rnd(7, (Ko,))
    res = q(rnd(8, (N, H, W, Ko)), dtype)
    y = K.conv2d(to_dev(x, dtype), to_dev(w, dtype), 1, 1, in_scale=sc.to(DEV), in_shift=sh.to(DEV), in_relu=True,
                 bias=bias.to(DEV), residual=to_dev(res, dtype), relu=True)
    # the engine rounds the transformed operand to the storage dtype before the MFMA
    xt = q(F.relu(x * sc + sh), dtype)
    want = R.conv_fwd(xt, w, 1, 1, bias=bias, residual=res, relu=True)
    close(y, want, TOL[dtype], "fused conv")


OSC_CASES = [
    # N, H, W, C, K, R, stride, pad, residual, kernel the bf16 launch must land on (None: whatever serves it)
    (2, 32, 32, 128, 128, 3, 1, 1, True, "conv3x3_h16s_kernel"),      # 16x16 tiles, the teacher's conv2 form (the output-scale instance)
    (33, 32, 32, 64, 256, 3, 1, 1, False, "conv3x3_h16s_kernel"),     # a workgroup walks into a second kout block
    (4, 8, 8, 256, 512, 3, 1, 1, True, ", 8>"),                        # four-image tiles
    (320, 8, 8, 64, 512, 3, 1, 1, False, ", 8>"),                      # ... head + 64-kout tail launches
    (40, 32, 32, 64, 64, 3, 1, 1, True, "conv3x3_pp64_kernel"),        # layer1 ping-pong form, residual instance
    (40, 32, 32, 64, 64, 3, 1, 1, False, "conv3x3_pp64_kernel"),
    (6, 64, 64, 64, 128, 3, 2, 1, False, "conv_s2_kernel<false, true>"),
    (6, 32, 64, 256, 384, 3, 2, 1, False, "conv_s2_kernel<false, true>"),   # kout-block-major walk: the block's bias / scale are reloaded
    (10, 30, 34, 64, 128, 3, 2, 1, False, "conv_dma_kernel"),
    (9, 32, 32, 64, 128, 1, 2, 0, False, "conv_dma_kernel"),
    (3, 9, 11, 64, 128, 3, 2, 1, False, None),                         # ragged: generic gather kernel
    (1, 24, 16, 64, 64, 3, 1, 1, True, None),                          # 128-pixel halo kernel
    (2, 8, 8, 256, 64, 3, 1, 1, True, None),
]


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("case", OSC_CASES)
def test_conv_out_scale(case, dtype):
    """sslcr_conv_desc.out_scale (round 6): eval-mode BatchNorm with its scale kept OUT of the filters -- y = relu(acc * scale + bias
    [+ residual]) -- in every kernel that serves a bias epilogue, against the plain conv times the scale; and the scale of ones gives the
    bits of the launch without it"""
    K = _k()
    N, H, W, C, Ko, Rr, stride, pad, with_res, expect = case
    x = q(rnd(81, (N, H, W, C)), dtype)
    w = q(rnd(82, (Ko, Rr, Rr, C), 0.05), dtype)
    bias, sc = rnd(83, (Ko,)), rnd(84, (Ko,)).abs() + 0.25
    sc[::3] *= -1.0                                          # gamma may be negative
    OH, OW = (H + 2 * pad - Rr) // stride + 1, (W + 2 * pad - Rr) // stride + 1
    res = q(rnd(85, (N, OH, OW, Ko)), dtype) if with_res else None
    kw = dict(bias=bias.to(DEV), residual=to_dev(res, dtype) if with_res else None, relu=True)
    y = K.conv2d(to_dev(x, dtype), to_dev(w, dtype), stride, pad, out_scale=sc.to(DEV), **kw)
    if expect and dtype == 1:
        assert expect in K.last_conv_kernel, K.last_conv_kernel
    close(y, R.conv_fwd(x, w, stride, pad, bias=bias, residual=res, relu=True, out_scale=sc), TOL[dtype], "conv with output scale")
    y1 = K.conv2d(to_dev(x, dtype), to_dev(w, dtype), stride, pad, out_scale=torch.ones(Ko, device=DEV), **kw)
    y0 = K.conv2d(to_dev(x, dtype), to_dev(w, dtype), stride, pad, **kw)
    assert torch.equal(y1, y0)


@pytest.mark.parametrize("shape", [(6, 64, 64, 64, 128), (9, 32, 32, 128, 256), (6, 32, 64, 256, 384)])
def test_conv_s2_pair_out_scale(shape):
    """the eval pair (conv1 3x3 / 2 + 1x1 / 2 projection in one launch) with both BatchNorm scales in the epilogue"""
    K = _k()
    N, H, W, C, Ko = shape
    x = q(rnd(91, (N, H, W, C)), 1)
    w3, w1 = q(rnd(92, (Ko, 3, 3, C), 0.05), 1), q(rnd(93, (Ko, 1, 1, C), 0.1), 1)
    b3, b1, s3, s1 = rnd(94, (Ko,)), rnd(95, (Ko,)), rnd(96, (Ko,)).abs() + 0.25, -(rnd(97, (Ko,)).abs() + 0.25)
    y3, yd = K.conv2d_s2_pair(to_dev(x, 1), to_dev(w3, 1), to_dev(w1, 1), bias3=b3.to(DEV), bias1=b1.to(DEV), relu3=True,
                              scale3=s3.to(DEV), scale1=s1.to(DEV))
    close(y3, R.conv_fwd(x, w3, 2, 1, bias=b3, relu=True, out_scale=s3), TOL[1], "eval 3x3 with scale")
    close(yd, R.conv_fwd(x, w1, 2, 0, bias=b1, out_scale=s1), TOL[1], "eval 1x1 with scale")


@pytest.mark.parametrize("dtype", [0, 1])
def test_pack_unfolded_and_stem_out_scale(dtype):
    """sslcr_pack_desc.scale_out: the eval pack keeps the plain filter and hands out gamma / sqrt(var + eps); the stem kernels (conv, and
    conv + max-pool in one launch) apply it in their epilogues.  Against torch's eval-mode conv1 -> bn1 -> relu (-> maxpool)."""
    K = _k()
    N, H = 3, 64
    xu = torch.from_numpy(np.random.RandomState(71).randint(0, 256, (N, 3, H, H), dtype=np.uint8))
    w = rnd(72, (64, 3, 7, 7), 0.03)
    g, b, rm, rv = rnd(73, (64,)).abs() + 0.5, rnd(74, (64,)), rnd(75, (64,)), rnd(76, (64,)).abs() + 0.5
    g[::4] *= -1.0
    bn = tuple(t.to(DEV) for t in (g, b, rm, rv))
    wp, bias, scale = K.pack_stem(w.to(DEV), dtype, bn=bn, unfold=True)
    wp0, _ = K.pack_stem(w.to(DEV), dtype)
    f = g / torch.sqrt(rv + 1e-5)
    assert torch.equal(wp, wp0)                                  # the plain filter
    close(scale, f, 1e-6, "scale_out")
    close(bias, b - rm * f, 1e-5, "bias_out")
    want = F.relu(R.nhwc(F.conv2d(xu.float(), q(w, dtype), None, 2, 3)) * f + (b - rm * f))
    # the two-kernel stem has no output scale (its registers: launch_stem) -- it fails loudly, the engine gives it the folded pack
    from ssl_cr_histo_amd import _lib as L
    with pytest.raises(L.SslcrError):
        K.stem_conv(xu.to(DEV), wp, bias=bias, relu=True, out_scale=scale)
    if dtype == 1:
        yp = K.stem_conv_pool(xu.to(DEV), wp, bias, out_scale=scale)
        wantp = R.nhwc(F.max_pool2d(R.nchw(q(want, 1)), 3, 2, 1))
        close(yp, wantp, TOL[1], "stem + pool with output scale")
    # a 3x3 filter bank
    w3 = rnd(77, (128, 64, 3, 3), 0.05)
    g3, b3, rm3, rv3 = rnd(78, (128,)).abs() + 0.5, rnd(79, (128,)), rnd(80, (128,)), rnd(81, (128,)).abs() + 0.5
    wf, _, bias3, scale3 = K.pack_conv(w3.to(DEV), dtype, bn=tuple(t.to(DEV) for t in (g3, b3, rm3, rv3)), unfold=True)
    wf0, _, _ = K.pack_conv(w3.to(DEV), dtype)
    f3 = g3 / torch.sqrt(rv3 + 1e-5)
    assert torch.equal(wf, wf0)
    close(scale3, f3, 1e-6, "scale_out 3x3")
    close(bias3, b3 - rm3 * f3, 1e-5, "bias_out 3x3")


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("shape", [(4, 8, 8, 512, 512), (320, 8, 8, 64, 512), (12, 8, 8, 128, 128), (2, 32, 32, 128, 128)])
def test_conv_eval_fused_epilogue_four_image_tiles(shape, dtype):
    """bias + residual + ReLU with no prologue (the teacher's conv2 with the BatchNorm folded) on the four-image-tile form of
    conv3x3_h16 -- one launch, and the 128-kout head + 64-kout tail pair of launches -- beside the 16x16-tile form"""
    K = _k()
    N, H, W, C, Ko = shape
    x = q(rnd(31, (N, H, W, C)), dtype)
    w = q(rnd(32, (Ko, 3, 3, C), 0.05), dtype)
    bias = rnd(33, (Ko,))
    res = q(rnd(34, (N, H, W, Ko)), dtype)
    y = K.conv2d(to_dev(x, dtype), to_dev(w, dtype), 1, 1, bias=bias.to(DEV), residual=to_dev(res, dtype), relu=True)
    assert "conv3x3_h16_kernel" in K.last_conv_kernel and K.last_conv_kernel.endswith(", 8>" if H == 8 else ", 16>"), K.last_conv_kernel
    want = R.conv_fwd(x, w, 1, 1, bias=bias, residual=res, relu=True)
    close(y, want, TOL[dtype], "eval-fused conv")
    # plain + statistics through the same shapes (the rows of a two-launch shape follow each other)
    y2, stats = K.conv2d(to_dev(x, dtype), to_dev(w, dtype), 1, 1, want_stats=True)
    want2 = R.conv_fwd(x, w, 1, 1)
    close(y2, want2, TOL[dtype], "conv raw")
    s1, s2 = R.channel_stats(want2)
    st = stats.double().sum(0).cpu()
    close(st[0], s1, 2e-4 if dtype == 0 else 2e-3, "sum")
    close(st[1], s2, 2e-4 if dtype == 0 else 2e-3, "sumsq")


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("case", [(2, 16, 16, 64, 64, 3, 1, 1), (3, 9, 11, 64, 128, 3, 2, 1), (2, 8, 8, 128, 256, 1, 2, 0),
                                  (2, 10, 10, 256, 256, 3, 1, 1),
                                  (10, 30, 34, 64, 128, 3, 2, 1),     # all-DMA gather conv: transposed + parity-class forms
                                  (10, 32, 32, 128, 256, 1, 2, 0)])   # all-DMA gather conv: 1x1 scatter-accumulate
def test_conv_dgrad(case, dtype):
    K = _k()
    N, H, W, C, Ko, Rr, stride, pad = case
    OH, OW = (H + 2 * pad - Rr) // stride + 1, (W + 2 * pad - Rr) // stride + 1
    dy = q(rnd(11, (N, OH, OW, Ko)), dtype)
    w = q(rnd(12, (Ko, Rr, Rr, C), 0.05), dtype)
    wd = w.permute(3, 1, 2, 0).contiguous()               # [C][R][S][K]
    want = R.conv_dgrad(dy, w, stride, pad, (H, W))
    if Rr == 1:
        # 1x1/2 downsample dgrad: scatter-accumulate into an existing gradient (identity-path add)
        base = q(rnd(13, (N, H, W, C)), dtype)
        out = to_dev(base, dtype)
        K.conv2d(to_dev(dy, dtype), to_dev(wd, dtype), 1, 0, out=out, out_hw=(H, W), osh=2, accumulate=True)
        close(out, want + base, TOL[dtype], "dgrad 1x1 scatter")
    else:
        res = q(rnd(14, (N, H, W, C)), dtype)
        dx = K.conv2d(to_dev(dy, dtype), to_dev(wd, dtype), stride, pad, transposed=True, pixel_hw=(H, W),
                      residual=to_dev(res, dtype))
        close(dx, want + res, TOL[dtype], "dgrad")
        if stride == 2:
            # the engine's form: one launch per input-pixel parity class, visiting only that class's taps
            dx3 = torch.zeros((N, H, W, C), dtype=K.tdtype(dtype), device=DEV)
            for par in range(4):
                ph_, pw_ = par >> 1, par & 1
                m = 0
                for r in range(3):
                    for s2 in range(3):
                        if (ph_ + 1 - r) % 2 == 0 and (pw_ + 1 - s2) % 2 == 0:
                            m |= 1 << (r * 3 + s2)
                K.conv2d(to_dev(dy, dtype), to_dev(wd, dtype), stride, pad, transposed=True, out=dx3, out_hw=(H, W),
                         pixel_hw=((H - ph_ + 1) // 2, (W - pw_ + 1) // 2), residual=to_dev(res, dtype), pix_mul=2,
                         pix_off=(ph_, pw_), tap_mask=m)
                if N * H * W >= 4 * 2048:
                    assert "conv_dma_kernel" in K.last_conv_kernel, K.last_conv_kernel
            close(dx3, want + res, TOL[dtype], "dgrad by parity classes")
            if H % 2 == 0 and W % 2 == 0 and N * H * W >= 4 * 2048:
                # ... and all four classes in one launch (class on grid z): bit-identical to the four launches
                dx4 = torch.zeros((N, H, W, C), dtype=K.tdtype(dtype), device=DEV)
                K.conv2d(to_dev(dy, dtype), to_dev(wd, dtype), stride, pad, transposed=True, out=dx4, out_hw=(H, W),
                         pixel_hw=(H // 2, W // 2), residual=to_dev(res, dtype), pix_mul=2, par4=True)
                assert "conv_dma_kernel" in K.last_conv_kernel, K.last_conv_kernel
                assert torch.equal(dx4, dx3)
        if stride == 1:
            # the engine's form: tap-flipped [C][R][S][K] pack => the dgrad is a plain 3x3 conv of dY (halo kernel when it tiles)
            w_kcrs = w.permute(0, 3, 1, 2).contiguous()
            _, wdf, _ = K.pack_conv(w_kcrs.to(DEV), dtype, fwd=False, dgrad=True, dgrad_flip=True)
            dx2 = K.conv2d(to_dev(dy, dtype), wdf, 1, 1, residual=to_dev(res, dtype))
            close(dx2, want + res, TOL[dtype], "dgrad via flipped pack")


@pytest.mark.parametrize("shape", [(6, 64, 64, 64, 128), (9, 32, 32, 128, 256), (70, 64, 64, 64, 128), (3, 8, 32, 192, 384), (130, 32, 32, 128, 256),
                                   (40, 16, 16, 256, 512), (3, 32, 16, 64, 128)])      # last two: 8-wide maps (whole 8x8 images / two tiles per image)
def test_conv_s2_wgrad(shape):
    """weight gradient of the 3x3 / 2 conv in parity-plane halo form (wgrad_s2_kernel, bf16, no producer transform -- what the engine
    launches for layer{2,3}.0.conv1): image-edge tiles (zero row / column), 1-3 cin blocks, 1-3 kout blocks, several pixel splits
    through the ordered fold, accumulation into a non-zero dW"""
    K = _k()
    N, H, W, C, Ko = shape
    OH, OW = H // 2, W // 2
    x = q(rnd(61, (N, H, W, C)), 1)
    dy = q(rnd(62, (N, OH, OW, Ko)), 1)
    base = rnd(63, (Ko, 3, 3, C))
    dw = base.clone().to(DEV)
    K.conv2d_wgrad(to_dev(x, 1), to_dev(dy, 1), dw, 3, 3, 2, 1)
    # routing: were wgrad_s2_ok() to start rejecting these shapes the gather kernel would serve them and pass the numbers below
    assert K.last_wgrad_kernel == f"sslcr::wgrad_s2_kernel<{16 if OW % 16 == 0 else 8}>", K.last_wgrad_kernel
    want = R.conv_wgrad(x, dy, (Ko, 3, 3, C), 2, 1)
    close(dw.cpu() - base, want, 3e-3, "stride-2 wgrad")


@pytest.mark.parametrize("xform", [False, True])
@pytest.mark.parametrize("shape", [(5, 32, 32, 128, 128), (3, 16, 48, 64, 256), (40, 16, 16, 256, 256), (70, 8, 8, 128, 384), (34, 8, 16, 192, 128), (36, 16, 8, 64, 128)])
def test_conv_wgrad_dma(shape, xform):
    """3x3 / 1 weight gradient with the operands staged by LDS DMA (wgrad3x3_dma_kernel, bf16, 128-kout blocks, several pixel splits;
    what the engine launches for layers 2-4): 16-wide and 8-wide tiles (whole 8x8 images, two tiles per image row), image-border
    tiles whose halo is padding from the buffer range check, 1-4 cin blocks x 1-3 kout blocks, the halo by DMA (no producer
    transform) and register-staged with the producer's BatchNorm + ReLU; accumulation into a non-zero dW."""
    K = _k()
    N, H, W, C, Ko = shape
    x = q(rnd(71, (N, H, W, C)), 1)
    dy = q(rnd(72, (N, H, W, Ko)), 1)
    sc, sh = rnd(73, (C,)).abs() + 0.5, rnd(74, (C,))
    base = rnd(75, (Ko, 3, 3, C))
    dw = base.clone().to(DEV)
    kw = dict(in_scale=sc.to(DEV), in_shift=sh.to(DEV), in_relu=True) if xform else {}
    K.conv2d_wgrad(to_dev(x, 1), to_dev(dy, 1), dw, 3, 3, 1, 1, **kw)
    tw = 16 if W % 16 == 0 else 8
    assert K.last_wgrad_kernel == f"sslcr::wgrad3x3_dma_kernel<{tw}, {'true' if xform else 'false'}>", K.last_wgrad_kernel
    xt = q(F.relu(x * sc + sh), 1) if xform else x
    close(dw.cpu() - base, R.conv_wgrad(xt, dy, (Ko, 3, 3, C), 1, 1), 3e-3, "DMA-form wgrad")


@pytest.mark.parametrize("shape", [(6, 64, 64, 64, 128), (9, 32, 32, 128, 256), (70, 64, 64, 64, 128), (3, 32, 64, 256, 384), (130, 32, 32, 128, 256)])
def test_conv_s2_dgrad(shape):
    """input gradient of the 3x3 / 2 conv, the four output-parity classes in one pass over dY (conv_s2d_kernel, bf16; the par4
    descriptor without a residual -- what the engine launches for layer{2,3}.0.conv1): edge tiles (zero halo beyond the bottom /
    right), 2-6 channel slabs, 1-4 channel blocks, more items than workgroups"""
    K = _k()
    N, H, W, C, Ko = shape
    OH, OW = H // 2, W // 2
    dy = q(rnd(51, (N, OH, OW, Ko)), 1)
    w = q(rnd(52, (Ko, 3, 3, C), 0.05), 1)
    wd = w.permute(3, 1, 2, 0).contiguous()               # [C][R][S][K]
    dx = torch.full((N, H, W, C), float("nan"), dtype=torch.bfloat16, device=DEV)
    K.conv2d(to_dev(dy, 1), to_dev(wd, 1), 2, 1, transposed=True, out=dx, out_hw=(H, W), pixel_hw=(OH, OW), pix_mul=2, par4=True)
    assert "conv_s2d_kernel" in K.last_conv_kernel, K.last_conv_kernel
    close(dx, R.conv_dgrad(dy, w, 2, 1, (H, W)), TOL[1], "stride-2 dgrad")


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("case", [(2, 16, 16, 64, 64, 3, 1, 1), (3, 9, 11, 64, 128, 3, 2, 1), (2, 8, 8, 128, 256, 1, 2, 0),
                                  (5, 12, 12, 128, 64, 3, 1, 1), (4, 8, 8, 128, 128, 3, 1, 1), (3, 24, 32, 64, 128, 3, 1, 1),
                                  (6, 8, 8, 512, 64, 3, 1, 1)])    # last three: halo wgrad, 8-wide / 16-wide tiles
def test_conv_wgrad(case, dtype):
    K = _k()
    N, H, W, C, Ko, Rr, stride, pad = case
    OH, OW = (H + 2 * pad - Rr) // stride + 1, (W + 2 * pad - Rr) // stride + 1
    x = q(rnd(21, (N, H, W, C)), dtype)
    dy = q(rnd(22, (N, OH, OW, Ko)), dtype)
    sc, sh = rnd(23, (C,)).abs() + 0.5, rnd(24, (C,))
    dw = torch.zeros((Ko, Rr, Rr, C), dtype=torch.float32, device=DEV)
    K.conv2d_wgrad(to_dev(x, dtype), to_dev(dy, dtype), dw, Rr, Rr, stride, pad, in_scale=sc.to(DEV), in_shift=sh.to(DEV),
                   in_relu=True)
    xt = q(F.relu(x * sc + sh), dtype)
    want = R.conv_wgrad(xt, dy, (Ko, Rr, Rr, C), stride, pad)
    close(dw, want, 2e-4 if dtype == 0 else 3e-3, "wgrad")
    # accumulate semantics: a second call doubles it
    K.conv2d_wgrad(to_dev(x, dtype), to_dev(dy, dtype), dw, Rr, Rr, stride, pad, in_scale=sc.to(DEV), in_shift=sh.to(DEV),
                   in_relu=True)
    close(dw, 2 * want, 2e-4 if dtype == 0 else 3e-3, "wgrad x2")


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("case", [(6, 16, 16, 64, 64, 2), (12, 16, 32, 128, 128, 4), (6, 8, 8, 256, 256, 2), (9, 32, 32, 64, 128, 3)])
def test_conv_wgrad_segments(case, dtype):
    """sslcr_wgrad_desc.seg_images: one launch over several segments (TripletNet branches) with their own producer BatchNorm
    == the sum of the per-segment weight gradients."""
    K = _k()
    N, H, W, C, Ko, seg = case
    nseg = N // seg
    x = q(rnd(25, (N, H, W, C)), dtype)
    dy = q(rnd(26, (N, H, W, Ko)), dtype)
    sc, sh = rnd(27, (nseg, C)).abs() + 0.5, rnd(28, (nseg, C))
    dw = torch.zeros((Ko, 3, 3, C), dtype=torch.float32, device=DEV)
    K.conv2d_wgrad(to_dev(x, dtype), to_dev(dy, dtype), dw, 3, 3, 1, 1, in_scale=sc.to(DEV), in_shift=sh.to(DEV), in_relu=True,
                   seg_images=seg)
    want = torch.zeros((Ko, 3, 3, C))
    for s in range(nseg):
        xs = q(F.relu(x[s * seg:(s + 1) * seg] * sc[s] + sh[s]), dtype)
        want += R.conv_wgrad(xs, dy[s * seg:(s + 1) * seg], (Ko, 3, 3, C), 1, 1)
    close(dw, want, 2e-4 if dtype == 0 else 3e-3, "segmented wgrad")


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("in_u8", [True, False])
@pytest.mark.parametrize("shape", [(2, 64, 64), (3, 56, 40), (1, 256, 256), (2, 30, 34)])   # W % 4 != 0: byte-staged fallback
def test_stem(shape, in_u8, dtype):
    K = _k()
    N, H, W = shape
    xu = torch.from_numpy(np.random.RandomState(31).randint(0, 256, (N, 3, H, W), dtype=np.uint8))
    w = rnd(32, (64, 3, 7, 7), 0.03)
    xin = xu if in_u8 else xu.float()
    wp, _ = K.pack_stem(w.to(DEV), dtype)
    y, stats = K.stem_conv(xin.to(DEV), wp, want_stats=True)
    want = R.nhwc(F.conv2d(xu.float(), q(w, dtype), None, 2, 3))
    close(y, want, TOL[dtype], "stem conv")
    s, ss = R.channel_stats(want)
    st = stats.double().sum(0).cpu()
    close(st[0], s, 2e-4 if dtype == 0 else 3e-3, "stem sum")
    close(st[1], ss, 2e-4 if dtype == 0 else 3e-3, "stem sumsq")
    # folded-BN eval form: bias + relu
    g, b, rm, rv = rnd(33, (64,)).abs() + 0.5, rnd(34, (64,)), rnd(35, (64,)), rnd(36, (64,)).abs() + 0.5
    wp2, bias = K.pack_stem(w.to(DEV), dtype, bn=tuple(t.to(DEV) for t in (g, b, rm, rv)))
    y2 = K.stem_conv(xin.to(DEV), wp2, bias=bias, relu=True)
    f = g / torch.sqrt(rv + 1e-5)
    want2 = F.relu(R.nhwc(F.conv2d(xu.float(), q(w * f.view(-1, 1, 1, 1), dtype), None, 2, 3)) + (b - rm * f))
    close(y2, want2, TOL[dtype], "stem folded")
    # wgrad
    OH, OW = want.shape[1:3]
    dy = q(rnd(37, (N, OH, OW, 64)), dtype)
    dw = torch.zeros((64, 3, 7, 7), dtype=torch.float32, device=DEV)
    K.stem_wgrad(xin.to(DEV), to_dev(dy, dtype), dw)
    wantw = torch.nn.grad.conv2d_weight(xu.float(), (64, 3, 7, 7), R.nchw(dy), 2, 3)
    close(dw, wantw, 2e-4 if dtype == 0 else 3e-3, "stem wgrad")


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("case", [(2, 16, 16, 64, 64), (5, 32, 32, 128, 128), (3, 16, 32, 128, 256), (70, 32, 32, 64, 64)])
def test_conv_bn_backward_front_end(case, dtype):
    """sslcr_conv_desc.mask_x: a 3x3/1 dgrad that also applies the ReLU mask of the BatchNorm it feeds and leaves that
    BatchNorm's two backward sums in its stats rows -- against conv + mask + sums of the reference ops."""
    K = _k()
    N, H, W, C, Ko = case
    x = q(rnd(81, (N, H, W, C)), dtype)
    w = q(rnd(82, (Ko, 3, 3, C), 0.05), dtype)
    xbn = q(rnd(83, (N, H, W, Ko), 2.0) + 0.3, dtype)
    sc, sh, mu = rnd(84, (Ko,)), rnd(85, (Ko,)), rnd(86, (Ko,))
    y, stats = K.conv2d(to_dev(x, dtype), to_dev(w, dtype), 1, 1, want_stats=True,
                        mask=(to_dev(xbn, dtype), sc.to(DEV), sh.to(DEV), mu.to(DEV)))
    assert ("conv3x3_pp64_kernel<false, 2>" if (C == 64 and Ko == 64 and dtype == 1) else "conv3x3_h16_kernel") in K.last_conv_kernel, K.last_conv_kernel
    want = R.conv_fwd(x, w, 1, 1)
    keep = (xbn * sc + sh) > 0
    g = want * keep
    # elements within rounding of the mask threshold may legitimately flip: exclude |scale*x+shift| < 1e-6 from the comparison
    edge = (xbn * sc + sh).abs() < 1e-6
    close(torch.where(edge.to(DEV), torch.zeros_like(y), y), torch.where(edge, torch.zeros_like(g), g), TOL[dtype], "masked dgrad")
    st = stats.double().sum(0).cpu()
    close(st[0], g.double().sum((0, 1, 2)), 2e-4 if dtype == 0 else 3e-3, "sum g")
    ref2 = (g.double() * (xbn.double() - mu.double())).sum((0, 1, 2))
    close(st[1], ref2, 2e-4 if dtype == 0 else 3e-3, "sum g (x - mean)")
    # a shape the 16x16-tile kernel does not serve must be refused, not silently served without the mask
    with pytest.raises(Exception):
        K.conv2d(to_dev(x[:, :15, :13].contiguous(), dtype), to_dev(w, dtype), 1, 1, want_stats=True,
                 mask=(to_dev(xbn[:, :15, :13].contiguous(), dtype), sc.to(DEV), sh.to(DEV), mu.to(DEV)))


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("in_u8", [True, False])
@pytest.mark.parametrize("shape,split", [((5, 64, 64), 2), ((3, 30, 34), 1), ((4, 32, 32), 4)])
def test_stem_two_segment_input(shape, split, in_u8, dtype):
    """torch.cat((inputs_x, inputs_u_s)) (eval_BreastPathQ_SSL_CR.py:82) as an address select in the stem kernels:
    forward and statistics on (x[:split], x2) must be BIT-identical to the same kernel on the concatenated batch,
    wgrad equal up to the order of its fp32 atomics."""
    K = _k()
    N, H, W = shape
    xu = torch.from_numpy(np.random.RandomState(41).randint(0, 256, (N, 3, H, W), dtype=np.uint8))
    xin = (xu if in_u8 else xu.float()).to(DEV)
    a, b = xin[:split].contiguous(), xin[split:].contiguous()
    wp, _ = K.pack_stem(rnd(42, (64, 3, 7, 7), 0.03).to(DEV), dtype)
    y0, s0 = K.stem_conv(xin, wp, want_stats=True)
    y1, s1 = K.stem_conv(a, wp, want_stats=True, x2=b)
    assert torch.equal(y0, y1) and torch.equal(s0, s1)
    dy = to_dev(q(rnd(43, tuple(y0.shape)), dtype), dtype)
    dw0 = torch.zeros((64, 3, 7, 7), dtype=torch.float32, device=DEV)
    dw1 = torch.zeros_like(dw0)
    K.stem_wgrad(xin, dy, dw0)
    K.stem_wgrad(a, dy, dw1, x2=b)
    close(dw1, dw0.cpu(), 1e-5, "stem wgrad two-segment")


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("in_u8", [True, False])
@pytest.mark.parametrize("shape,split", [((3, 64, 64), 0), ((2, 56, 40), 0), ((5, 30, 34), 2), ((1, 256, 256), 0), ((40, 64, 64), 16)])
def test_stem_wgrad_from_pooled_gradient(shape, split, in_u8, dtype):
    """sslcr_stem_wgrad_pool: conv1's weight gradient straight from the pooled gradient (max-pool + ReLU + bn0 backward apply on
    the tile in LDS) -- the same bits as sslcr_bn_bwd_apply -> sslcr_stem_wgrad, whose pieces are pinned against torch above, and
    against autograd of conv1 -> bn1 -> relu -> maxpool (models/net.py:32,77) directly.  Ragged tiles (OH, OW not multiples of
    8, 16; odd pooled sizes), the two-segment input, more tiles than workgroups ((40, 64, 64): 1280 tiles over 768)."""
    K = _k()
    N, H, W = shape
    xu = torch.from_numpy(np.random.RandomState(51).randint(0, 256, (N, 3, H, W), dtype=np.uint8))
    xin = (xu if in_u8 else xu.float()).to(DEV)
    w = rnd(52, (64, 3, 7, 7), 0.03)
    gamma, beta = rnd(53, (64,)).abs() + 0.5, rnd(54, (64,))
    wp, _ = K.pack_stem(w.to(DEV), dtype)
    raw, stats = K.stem_conv(xin, wp, want_stats=True)
    OH, OW = raw.shape[1:3]
    sc, sh, mean, invstd = K.bn_finalize(stats, N * OH * OW, gamma.to(DEV), beta.to(DEV))
    pooled, am = K.bn_relu_maxpool(raw, sc, sh)
    dyp = to_dev(q(rnd(55, tuple(pooled.shape)), dtype), dtype)
    # two launches: apply pass writes dY, wgrad reads it
    dx, sums_a, _ = K.bn_bwd(None, raw, sc, sh, mean, invstd, relu_from_x=True, pool=(dyp, am, pooled))
    dw_a = torch.zeros((64, 3, 7, 7), dtype=torch.float32, device=DEV)
    K.stem_wgrad(xin, dx, dw_a)
    dg_a, db_a = torch.zeros(64, device=DEV), torch.zeros(64, device=DEV)
    K.bn_param_grads(sums_a, invstd, dg_a, db_a)
    # one launch
    dw_b = torch.zeros_like(dw_a)
    dg_b, db_b = torch.zeros(64, device=DEV), torch.zeros(64, device=DEV)
    a, b = (xin[:split].contiguous(), xin[split:].contiguous()) if split else (xin, None)
    sums_b = K.stem_wgrad_pool(a, dw_b, raw, sc, sh, mean, invstd, (dyp, am, pooled), x2=b, dgamma=dg_b, dbeta=db_b)
    assert torch.equal(sums_a, sums_b)
    # same tile -> workgroup assignment and MFMA order; the only freedom is the order of the fold's fp32 atomics
    close(dw_b, dw_a.cpu(), 2e-6, "fused stem wgrad vs apply + wgrad")
    assert torch.equal(dg_b, dg_a) and torch.equal(db_b, db_a)       # one arithmetic: bn_bwd_affine_grads
    # and against autograd of bn1 -> relu -> maxpool on the conv output the kernels saw (in bf16 mode the rounded one: the
    # argmax / ReLU pattern of a separately computed fp32 convolution differs in a few per cent of the windows), then conv1's wgrad
    leaf = R.nchw(raw.float().cpu()).requires_grad_(True)
    gr, br = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    out = F.max_pool2d(F.relu(F.batch_norm(leaf, None, None, gr, br, True, 0.1, 1e-5)), 3, 2, 1)
    out.backward(R.nchw(dyp.float().cpu()))
    wantw = torch.nn.grad.conv2d_weight(xu.float(), (64, 3, 7, 7), leaf.grad, 2, 3)
    t = 3e-4 if dtype == 0 else 5e-2       # bf16: dY is rounded to bf16 ahead of the wgrad MFMAs (2.8e-2 measured at N = 40)
    close(dw_b, wantw, t, "fused stem wgrad vs autograd")
    close(dg_b, gr.grad, t, "dgamma vs autograd")
    close(db_b, br.grad, t, "dbeta vs autograd")


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("shape", [(2, 32, 32), (2, 30, 26)])     # conv1 map 16x16 -> pooled 8x8; 15x13 -> 8x7 (ragged)
def test_bn_param_grads_one_arithmetic(shape, dtype):
    """dgamma / dbeta are float += (float)(double product) wherever they are formed (bn_bwd_affine_grads, csrc/bn_bwd.hpp): the same
    bits from sslcr_bn_param_grads, from workgroup 0 of the pool-form and of the plain-form apply pass, and from the fused stem
    weight-gradient kernel (fp32: stem_wgrad_kernel<POOL>, bf16: stem_wgrad_pool2_kernel).  The buffers start at 0.25: the += counts."""
    K = _k()
    N, H, W = shape
    xin = torch.from_numpy(np.random.RandomState(61).randint(0, 256, (N, 3, H, W), dtype=np.uint8)).to(DEV)
    w = rnd(62, (64, 3, 7, 7), 0.03)
    gamma, beta = rnd(63, (64,)).abs() + 0.5, rnd(64, (64,))
    wp, _ = K.pack_stem(w.to(DEV), dtype)
    raw, stats = K.stem_conv(xin, wp, want_stats=True)
    OH, OW = raw.shape[1:3]
    sc, sh, mean, invstd = K.bn_finalize(stats, N * OH * OW, gamma.to(DEV), beta.to(DEV))
    pooled, am = K.bn_relu_maxpool(raw, sc, sh)
    assert tuple(pooled.shape[1:3]) == ((OH + 1) // 2, (OW + 1) // 2)
    dyp = to_dev(q(rnd(65, tuple(pooled.shape)), dtype), dtype)
    grads = {}

    def bufs(name):
        grads[name] = (torch.full((64,), 0.25, device=DEV), torch.full((64,), 0.25, device=DEV))
        return grads[name]
    dg, db = bufs("pool-form apply")
    dx, sums, _ = K.bn_bwd(None, raw, sc, sh, mean, invstd, relu_from_x=True, pool=(dyp, am, pooled), dgamma=dg, dbeta=db)
    dg, db = bufs("bn_param_grads")
    K.bn_param_grads(sums, invstd, dg, db)
    dg, db = bufs("stem_wgrad_pool")
    dw = torch.zeros((64, 3, 7, 7), dtype=torch.float32, device=DEV)
    sums_w = K.stem_wgrad_pool(xin, dw, raw, sc, sh, mean, invstd, (dyp, am, pooled), dgamma=dg, dbeta=db)
    assert torch.equal(sums_w, sums)
    dg, db = bufs("plain-form apply")
    K.bn_bwd(dx, raw, sc, sh, mean, invstd, sums=sums, dgamma=dg, dbeta=db)       # a dense gradient, the same statistics and sums
    want_g, want_b = grads["bn_param_grads"]
    assert not torch.equal(want_g, torch.full_like(want_g, 0.25)) and not torch.equal(want_b, torch.full_like(want_b, 0.25))
    for name, (dg, db) in grads.items():
        assert torch.equal(dg, want_g), f"dgamma: {name} vs bn_param_grads, max diff {(dg - want_g).abs().max().item():.3e}"
        assert torch.equal(db, want_b), f"dbeta: {name} vs bn_param_grads, max diff {(db - want_b).abs().max().item():.3e}"


def test_stem_wgrad_pool_rejects_foreign_descriptors():
    """sslcr_stem_wgrad_pool fails loudly (error code + message, nothing launched) on a BatchNorm descriptor that is not this
    stem's: wrong channel count, map size, missing pooled gradient, or one that asks for the masked gradient as an output."""
    K = _k()
    from ssl_cr_histo_amd import _lib as L
    N, H = 2, 64
    x = torch.zeros((N, 3, H, H), dtype=torch.uint8, device=DEV)
    raw = torch.zeros((N, H // 2, H // 2, 64), dtype=torch.float32, device=DEV)
    pdy = torch.zeros((N, H // 4, H // 4, 64), dtype=torch.float32, device=DEV)
    am = torch.zeros((N, H // 4, H // 4, 64), dtype=torch.uint8, device=DEV)
    v = torch.ones(64, device=DEV)
    sums = torch.zeros((2, 64), dtype=torch.float64, device=DEV)
    dw = torch.zeros((64, 3, 7, 7), device=DEV)

    def call(**over):
        b = L.BnBwdDesc(None, L.ptr(raw), None, L.ptr(v), L.ptr(v), L.ptr(v), L.ptr(v), L.ptr(sums), None, None, raw.numel() // 64, 64, 1,
                        float(raw.numel() // 64), L.ptr(pdy), L.ptr(am), H // 2, H // 2, H // 4, H // 4, None, 0)
        for k, val in over.items():
            setattr(b, k, val)
        w = L.StemWgradDesc(L.ptr(x), None, L.ptr(dw), N, H, H, H // 2, H // 2, 0, None, 0)
        return L.lib().sslcr_stem_wgrad_pool(0, w, b, L.stream_ptr())
    assert call() == 0
    for over in ({"C": 128}, {"pH": H // 2 - 1}, {"pool_dy": None}, {"pool_argmax": None}, {"gout": L.ptr(raw)}, {"pixels": 17}):
        assert call(**over) != 0, over
        assert b"stem_wgrad_pool" in L.lib().sslcr_last_error()
    torch.cuda.synchronize()


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("hw", [(16, 16), (15, 13)])          # odd sizes: ragged 2x2 blocks / pooling windows at the border
def test_bn_forward_chain(hw, dtype):
    """conv stats -> finalize (x3 replay) -> bn_act / pool, against F.batch_norm train mode."""
    K = _k()
    N, (H, W), C = 4, hw, 64
    x = q(rnd(41, (N, H, W, C), 3.0) + 1.5, dtype)
    w = q(rnd(42, (C, 3, 3, C), 0.05), dtype)
    gamma, beta = rnd(43, (C,)).abs() + 0.5, rnd(44, (C,))
    rm, rv = rnd(45, (C,)), rnd(46, (C,)).abs() + 0.5
    raw, stats = K.conv2d(to_dev(x, dtype), to_dev(w, dtype), 1, 1, want_stats=True)
    rm_d, rv_d = rm.to(DEV).clone(), rv.to(DEV).clone()
    nbt = torch.zeros((), dtype=torch.int64, device=DEV)
    sc, sh, mean, invstd = K.bn_finalize(stats, N * H * W, gamma.to(DEV), beta.to(DEV), running_mean=rm_d, running_var=rv_d,
                                         nbt=nbt, replay=3)
    raw_ref = R.conv_fwd(x, w, 1, 1)
    rm_r, rv_r = rm.clone(), rv.clone()
    for _ in range(3):
        bn_ref = F.batch_norm(R.nchw(raw_ref), rm_r, rv_r, gamma, beta, True, 0.1, 1e-5)
    t = 3e-4 if dtype == 0 else 5e-3
    close(rm_d, rm_r, t, "running_mean x3")
    close(rv_d, rv_r, t, "running_var x3")
    assert int(nbt.item()) == 3
    res = q(rnd(47, (N, H, W, C)), dtype)
    y = K.bn_act(raw, sc, sh, res=to_dev(res, dtype), relu=True)
    close(y, F.relu(R.nhwc(bn_ref) + res), 3e-4 if dtype == 0 else 1.5e-2, "bn+res+relu")
    rsc, rsh = rnd(48, (C,)).abs() + 0.5, rnd(49, (C,))
    y2 = K.bn_act(raw, sc, sh, res=to_dev(res, dtype), rscale=rsc.to(DEV), rshift=rsh.to(DEV), relu=True)
    close(y2, F.relu(R.nhwc(bn_ref) + res * rsc + rsh), 3e-4 if dtype == 0 else 1.5e-2, "bn+bn(res)+relu")
    # maxpool of relu(bn) and its backward
    pooled, am = K.bn_relu_maxpool(raw, sc, sh)
    act = F.relu(bn_ref).detach().requires_grad_(True)
    pool_ref = F.max_pool2d(act, 3, 2, 1)
    close(pooled, R.nhwc(pool_ref), 3e-4 if dtype == 0 else 1.5e-2, "maxpool")
    ap = K.avgpool_fwd(pooled)
    close(ap, pooled.float().mean((1, 2)), 1e-5, "avgpool")
    if dtype == 0:
        dyp = rnd(50, tuple(pool_ref.shape))
        pool_ref.backward(dyp)
        gact = act.grad * (act > 0)
        dx = K.maxpool_relu_bwd(to_dev(R.nhwc(dyp), dtype), am, raw, sc, sh)
        close(dx, R.nhwc(gact), 3e-4, "maxpool+relu bwd")
        # the engine's stem form: max-pool + ReLU backward folded into the BatchNorm backward passes
        dx_a, sums_a, _ = K.bn_bwd(dx, raw, sc, sh, mean, invstd)
        dx_b, sums_b, _ = K.bn_bwd(None, raw, sc, sh, mean, invstd, relu_from_x=True, pool=(to_dev(R.nhwc(dyp), dtype), am))
        close(dx_b, dx_a, 1e-5, "bn bwd through pool")
        close(sums_b, sums_a, 1e-6, "bn bwd sums through pool")
        # with the saved pool OUTPUT the reduce pass works on pooled tensors only ((x - mean) recovered from y where y > 0)
        dx_c, sums_c, _ = K.bn_bwd(None, raw, sc, sh, mean, invstd, relu_from_x=True,
                                   pool=(to_dev(R.nhwc(dyp), dtype), am, pooled))
        close(sums_c, sums_a, 1e-5, "bn bwd sums from pooled tensors")
        close(dx_c, dx_a, 1e-5, "bn bwd through pool (pooled reduce)")
        # a channel with gamma == 0 cannot be inverted: those lanes fetch x at the argmax position
        sc0, sh0 = sc.clone(), sh.clone()
        sc0[3] = 0.0; sh0[3] = 0.25; sc0[5] = 0.0; sh0[5] = -0.5
        pooled0, am0 = K.bn_relu_maxpool(raw, sc0, sh0)
        dxp0 = K.maxpool_relu_bwd(to_dev(R.nhwc(dyp), dtype), am0, raw, sc0, sh0)
        dx_r, sums_r, _ = K.bn_bwd(dxp0, raw, sc0, sh0, mean, invstd)
        dx_z, sums_z, _ = K.bn_bwd(None, raw, sc0, sh0, mean, invstd, relu_from_x=True,
                                   pool=(to_dev(R.nhwc(dyp), dtype), am0, pooled0))
        close(sums_z, sums_r, 1e-5, "bn bwd sums from pooled tensors, gamma == 0 channels")
        close(dx_z, dx_r, 1e-5, "bn bwd through pool, gamma == 0 channels")
    else:
        # bf16: pooled-tensor reduce vs the gather form (same kernels as the engine's stem backward)
        dyp = q(rnd(50, tuple(pooled.shape)), dtype)
        dx_b, sums_b, _ = K.bn_bwd(None, raw, sc, sh, mean, invstd, relu_from_x=True, pool=(to_dev(dyp, dtype), am))
        dx_c, sums_c, _ = K.bn_bwd(None, raw, sc, sh, mean, invstd, relu_from_x=True, pool=(to_dev(dyp, dtype), am, pooled))
        close(sums_c, sums_b, 1e-2, "bn bwd sums from pooled tensors (bf16)")
        close(dx_c, dx_b, 2e-2, "bn bwd through pool (pooled reduce, bf16)")
    dap = K.avgpool_bwd(ap, tuple(pooled.shape), dtype)
    close(dap, (ap / (pooled.shape[1] * pooled.shape[2]))[:, None, None, :].expand(pooled.shape), 1e-2 if dtype else 1e-6, "avgpool bwd")


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("C", [64, 24, 512])      # 24: a width whose chunk count does not divide 256 (generic kernel, not the row form)
@pytest.mark.parametrize("hw", [(16, 16), (9, 7), (2, 2)])
def test_bn_relu_maxpool_shapes(hw, C, dtype):
    """maxpool3x3/2 pad 1 of relu(scale*x+shift) with argmax codes: values against torch, codes through the backward."""
    K = _k()
    N, (H, W) = 3, hw
    x = q(rnd(61, (N, H, W, C), 2.0), dtype)
    sc, sh = rnd(62, (C,)), rnd(63, (C,))
    sc[1] = 0.0                                      # a gamma == 0 channel: every window element ties, the first one wins
    pooled, am = K.bn_relu_maxpool(to_dev(x, dtype), sc.to(DEV), sh.to(DEV))
    act = F.relu(R.nchw(x) * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)).requires_grad_(True)
    ref = F.max_pool2d(act, 3, 2, 1)
    close(pooled, R.nhwc(ref), 1e-6 if dtype == 0 else 1e-2, "maxpool values")
    if dtype == 0:
        dyp = rnd(64, tuple(ref.shape))
        ref.backward(dyp)
        dx = K.maxpool_relu_bwd(to_dev(R.nhwc(dyp), dtype), am, to_dev(x, dtype), sc.to(DEV), sh.to(DEV))
        close(dx, R.nhwc(act.grad * (act > 0)), 1e-6, "maxpool+relu backward through the recorded argmax")


@pytest.mark.parametrize("dtype", [0, 1])
def test_bn_relu_maxpool_many_rows(dtype):
    """4160 output rows (more than the row form's 4096-workgroup grid, so workgroups walk several rows); argmax codes against torch."""
    K = _k()
    N, H, W, C = 130, 64, 64, 64
    x = q(rnd(65, (N, H, W, C), 2.0), dtype)
    sc, sh = rnd(66, (C,)), rnd(67, (C,))
    pooled, am = K.bn_relu_maxpool(to_dev(x, dtype), sc.to(DEV), sh.to(DEV))
    act = F.relu(R.nchw(x) * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1))
    ref, idx = F.max_pool2d(act, 3, 2, 1, return_indices=True)
    close(pooled, R.nhwc(ref), 1e-6 if dtype == 0 else 1e-2, "maxpool values")
    # plain form (the eval path: no affine, no ReLU, no argmax), negative values included: bit-exact, a maximum is one of its inputs
    plain, none = K.bn_relu_maxpool(to_dev(x, dtype), None, None)
    assert none is None and torch.equal(plain.float().cpu(), R.nhwc(F.max_pool2d(R.nchw(x), 3, 2, 1)))
    if dtype == 0:
        # the argmax codes (window position r*3+s) point at the element torch picked wherever the maximum is unique
        am = am.cpu().to(torch.int64).reshape(N, H // 2, W // 2, C)
        oh = torch.arange(H // 2).view(1, -1, 1, 1); ow = torch.arange(W // 2).view(1, 1, -1, 1)
        flat = (2 * oh - 1 + am // 3) * W + (2 * ow - 1 + am % 3)
        pos = R.nhwc(ref) > 0
        assert torch.equal(flat[pos], R.nhwc(idx)[pos])
        # ... and a window whose maximum is not positive carries code 9: the ReLU passes no gradient into it
        assert bool((am[~pos] == 9).all()) and bool((am[pos] < 9).all())


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("mode", ["yact", "from_x", "none"])
def test_bn_backward(mode, dtype):
    K = _k()
    N, H, W, C = 3, 10, 10, 128
    x = q(rnd(51, (N, H, W, C), 2.0) + 0.7, dtype)
    dy = q(rnd(52, (N, H, W, C)), dtype)
    gamma, beta = rnd(53, (C,)).abs() + 0.5, rnd(54, (C,))
    xr = R.nchw(x).clone().requires_grad_(True)
    gr, br = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    bn = F.batch_norm(xr, None, None, gr, br, True, 0.1, 1e-5)
    out = F.relu(bn) if mode != "none" else bn
    out.backward(R.nchw(dy))
    xf = x.reshape(-1, C).double()
    mean = xf.mean(0)
    var = xf.var(0, unbiased=False)
    invstd = 1.0 / torch.sqrt(var + 1e-5)
    scale = (gamma.double() * invstd).float()
    shift = (beta.double() - mean * gamma.double() * invstd).float()
    yact = to_dev(q(R.nhwc(out.detach()), dtype), dtype) if mode == "yact" else None
    dx, sums, g = K.bn_bwd(to_dev(dy, dtype), to_dev(x, dtype), scale.to(DEV), shift.to(DEV), mean.float().to(DEV),
                           invstd.float().to(DEV), yact=yact, relu_from_x=(mode == "from_x"), want_g=True)
    t = 5e-4 if dtype == 0 else 2e-2
    close(dx, R.nhwc(xr.grad), t, "bn dx")
    dg, db = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
    K.bn_param_grads(sums, invstd.float().to(DEV), dg, db)
    close(dg, gr.grad, t, "dgamma")
    close(db, br.grad, t, "dbeta")
    mask = (out.detach() > 0).float() if mode != "none" else torch.ones_like(out)
    close(g, dy * R.nhwc(mask), 1e-6, "g")
    if mode == "yact":
        # the engine's form for a block's second BatchNorm: the reduce pass writes g, the apply pass reads it back -- same bits
        dx2, sums2, g2 = K.bn_bwd(to_dev(dy, dtype), to_dev(x, dtype), scale.to(DEV), shift.to(DEV), mean.float().to(DEV),
                                  invstd.float().to(DEV), yact=yact, want_g=True, g_in_reduce=True)
        assert torch.equal(g2, g) and torch.equal(dx2, dx)
        close(sums2, sums, 1e-12, "sums with g written by the reduce pass")


@pytest.mark.parametrize("nseg", [1, 3])
def test_relu_mask_as_bits_through_bn_act_and_bn_backward(nseg):
    """sslcr_bn_act_desc.ybits / sslcr_bn_bwd_desc.yact_bits (bf16): the block output's sign mask as one bit per element -- written by the
    forward's bn_act from the STORED values, read by bn2's backward reduce pass instead of the tensor: the same g, sums and dx, bit for bit,
    plain and as segments."""
    K = _k()
    n, H, W, C = 4, 6, 10, 128
    N = nseg * n
    x = to_dev(rnd(301, (N, H, W, C)), 1)
    res = to_dev(rnd(302, (N, H, W, C)), 1)
    shp = (nseg, C) if nseg > 1 else (C,)
    sc, sh = (rnd(303, shp).abs() * 0.5 + 0.25).to(DEV), rnd(304, shp, 0.3).to(DEV)
    # tiny positive values too: a float below half the smallest bf16 is stored as 0 and its bit must be 0
    sh.view(-1)[:8] = 1e-41
    sc.view(-1)[:8] = 0.0
    res[..., :8] = 0
    y, bits = K.bn_act(x, sc, sh, res=res, relu=True, nseg=nseg, want_bits=True)
    y_plain = K.bn_act(x, sc, sh, res=res, relu=True, nseg=nseg)
    assert torch.equal(y.view(torch.int16), y_plain.view(torch.int16))
    want = (y.float().flatten() > 0).view(-1, 8).to(torch.int32)
    got = ((bits.to(torch.int32).view(-1, 1) >> torch.arange(8, device=DEV, dtype=torch.int32).view(1, 8)) & 1)
    assert torch.equal(got, want)
    dy = to_dev(rnd(305, (N, H, W, C)), 1)
    mean, invstd = rnd(306, shp, 0.2).to(DEV), (rnd(307, shp).abs() + 0.5).to(DEV)
    for gir in (False, True):
        a = K.bn_bwd(dy, x, sc, sh, mean, invstd, yact=y, want_g=True, g_in_reduce=gir, nseg=nseg)
        b = K.bn_bwd(dy, x, sc, sh, mean, invstd, yact=y, want_g=True, g_in_reduce=gir, nseg=nseg, yact_bits=bits)
        assert torch.equal(a[0].view(torch.int16), b[0].view(torch.int16)) and torch.equal(a[1], b[1])
        assert torch.equal(a[2].view(torch.int16), b[2].view(torch.int16))
    assert float((a[2].float() != 0).float().mean()) > 0.2           # (the mask is not trivially empty)


@pytest.mark.parametrize("shape", [(96, 1024, 512), (64, 512, 256), (160, 768, 128), (32, 64, 32)])
def test_linear_lds_form(shape):
    """the LDS-staged fp32 GEMM (gemm_f32_lds_kernel: M, N multiples of 32, K of 64 -- the fc.0 / fc.2 / FinetuneResNet shapes of a
    step) in its four operand forms: forward (both k-contiguous), dx (B k-strided), dw (both k-strided, accumulating into a
    non-zero buffer), with bias + ReLU and the ReLU mask"""
    K = _k()
    M, Kd, Nn = shape
    x, w, b = rnd(161, (M, Kd)), rnd(162, (Nn, Kd), 0.03), rnd(163, (Nn,))
    xr, wr, br = (t.clone().requires_grad_(True) for t in (x, w, b))
    yr = F.relu(F.linear(xr, wr, br))
    y = K.linear_fwd(x.to(DEV), w.to(DEV), b.to(DEV), relu=True)
    close(y, yr, 2e-5, "linear fwd")
    y0 = K.linear_fwd(x.to(DEV), w.to(DEV), None, relu=False)
    close(y0, F.linear(x, w), 2e-5, "linear fwd, no bias")
    dy = rnd(164, (M, Nn))
    yr.backward(dy)
    base = rnd(165, (Nn, Kd))
    dw = base.clone().to(DEV)
    db = torch.zeros(Nn, device=DEV)
    dx = K.linear_bwd(x.to(DEV), w.to(DEV), dy.to(DEV), yact=y, dw=dw, db=db)
    close(dx, xr.grad, 5e-5, "linear dx")
    close(dw.cpu() - base, wr.grad, 5e-5, "linear dw")
    close(db, br.grad, 5e-5, "linear db")


def test_linear_and_loss():
    K = _k()
    M, Kd, Nn = 37, 1024, 512
    x, w, b = rnd(61, (M, Kd)), rnd(62, (Nn, Kd), 0.03), rnd(63, (Nn,))
    xr, wr, br = (t.clone().requires_grad_(True) for t in (x, w, b))
    yr = F.relu(F.linear(xr, wr, br))
    y = K.linear_fwd(x.to(DEV), w.to(DEV), b.to(DEV), relu=True)
    close(y, yr, 2e-5, "linear fwd")
    dy = rnd(64, (M, Nn))
    yr.backward(dy)
    dw = torch.zeros((Nn, Kd), device=DEV)
    db = torch.zeros(Nn, device=DEV)
    dx = K.linear_bwd(x.to(DEV), w.to(DEV), dy.to(DEV), yact=y, dw=dw, db=db)
    close(dx, xr.grad, 5e-5, "linear dx")
    close(dw, wr.grad, 5e-5, "linear dw")
    close(db, br.grad, 5e-5, "linear db")
    # losses
    for kind, Cn in ((0, 1), (1, 2), (1, 9), (2, 6), (3, 1)):
        nx, nu = 6, 14 if kind in (0, 1) else 0
        lg = rnd(65 + Cn, (nx + nu, Cn), 2.0).requires_grad_(True)
        lt = rnd(66 + Cn, (max(nu, 1), Cn), 2.0)
        lam = 0.7
        if kind in (0, 3):
            tgt = rnd(67, (nx,)).abs()
            lx = F.mse_loss(lg[:nx], tgt.view(-1, 1).expand(nx, Cn))
            lu = F.mse_loss(lt, lg[nx:]) if kind == 0 else torch.zeros(())
            out, dl = K.loss(kind, lg.detach().to(DEV), logits_t=lt.to(DEV) if kind == 0 else None, target_f=tgt.to(DEV), nx=nx, lambda_u=lam)
            correct = None
        else:
            tgt = torch.from_numpy(np.random.RandomState(68).randint(0, Cn, (nx,)).astype(np.int64))
            lx = F.cross_entropy(lg[:nx], tgt)
            lu = F.cross_entropy(lg[nx:], torch.softmax(lt, -1).max(-1)[1]) if kind == 1 else torch.zeros(())
            out, dl = K.loss(kind, lg.detach().to(DEV), logits_t=lt.to(DEV) if kind == 1 else None, target_i=tgt.to(DEV), nx=nx, lambda_u=lam)
            correct = (lg[:nx].argmax(1) == tgt).sum().item()
        total = lx + lam * lu
        total.backward()
        o = out.cpu()
        assert abs(o[0] - total.item()) < 1e-5 * max(1, abs(total.item())), (kind, o, total)
        assert abs(o[1] - lx.item()) < 1e-5 * max(1, abs(lx.item()))
        assert abs(o[2] - float(lu)) < 1e-5 * max(1, abs(float(lu)))
        if correct is not None:
            assert int(o[3]) == correct
        close(dl, lg.grad, 1e-5, f"dlogits kind {kind}")


@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_optimizer_and_pack(kind):
    from ssl_cr_histo_amd import _lib as L
    K = _k()
    shapes = [(64, 3, 7, 7), (128, 64, 3, 3), (128,), (10, 768), (256, 128, 1, 1)]
    ps = [rnd(70 + i, s, 0.1) for i, s in enumerate(shapes)]
    ref = [p.clone().requires_grad_(True) for p in ps]
    opt = (torch.optim.Adam(ref, lr=1e-2, betas=(0.9, 0.999), weight_decay=1e-4) if kind == "adam"
           else torch.optim.SGD(ref, lr=1e-2, momentum=0.9, weight_decay=1e-4, nesterov=True))
    dev_p = [p.to(DEV).contiguous() for p in ps]
    s1 = [torch.zeros_like(p) for p in dev_p]
    s2 = [torch.zeros_like(p) for p in dev_p]
    sh_f = torch.zeros((128, 3, 3, 64), dtype=torch.bfloat16, device=DEV)
    sh_d = torch.zeros((64, 3, 3, 128), dtype=torch.bfloat16, device=DEV)
    for step in range(1, 4):
        grads = [rnd(100 * step + i, s) for i, s in enumerate(shapes)]
        dev_g = []
        descs = (L.TensorDesc * len(shapes))()
        for i, (p, g) in enumerate(zip(dev_p, grads)):
            if g.dim() == 4 and i != 0:                       # engine grad layout KRSC; stem keeps PyTorch layout
                gd = g.permute(0, 2, 3, 1).contiguous().to(DEV)
                Kk, Cc, RS = g.shape[0], g.shape[1], g.shape[2] * g.shape[3]
            else:
                gd = g.to(DEV)
                Kk, Cc, RS = 0, 0, 0
            dev_g.append(gd)
            descs[i] = L.TensorDesc(L.ptr(p), L.ptr(gd), L.ptr(s1[i]), L.ptr(s2[i]), p.numel(), Kk, Cc, RS)
            if i == 1:            # the update also writes this conv's shadow weights (bf16 forward pack, flipped dgrad pack)
                descs[i].w_fwd, descs[i].w_dgrad, descs[i].pack_dtype, descs[i].dgrad_flip = L.ptr(sh_f), L.ptr(sh_d), 1, 1
        dd = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).to(DEV)
        o = L.OptDesc(0 if kind == "adam" else 1, 1e-2, 0.9, 0.999, 1e-8, 1e-4, 0.9, 1 - 0.9 ** step, 1 - 0.999 ** step,
                      int(step == 1), 1.0)
        L.check(L.lib().sslcr_optimizer_step(L.ptr(dd), len(shapes), max(p.numel() for p in dev_p), o, L.stream_ptr()))
        for r, g in zip(ref, grads):
            r.grad = g.clone()
        opt.step()
    for p, r in zip(dev_p, ref):
        close(p, r, 2e-5, f"{kind} param")
    wf1, wd1, _ = K.pack_conv(dev_p[1], 1, fwd=True, dgrad=True, dgrad_flip=True)
    assert torch.equal(sh_f, wf1) and torch.equal(sh_d, wd1), "shadow weights written by the update != pack of the updated parameter"
    # pack: layouts and folding
    w = rnd(90, (128, 64, 3, 3), 0.05)
    wf, wd, _ = K.pack_conv(w.to(DEV), 0, fwd=True, dgrad=True)
    assert torch.equal(wf.cpu(), w.permute(0, 2, 3, 1).contiguous())
    assert torch.equal(wd.cpu(), w.permute(1, 2, 3, 0).contiguous())
    a, b2 = rnd(91, (64,)).to(DEV), rnd(92, (64,)).to(DEV)
    ref_a = 0.3 * a + 0.7 * b2
    L.check(L.lib().sslcr_axpby(L.ptr(a), L.ptr(b2), 64, 0.3, 1, L.stream_ptr()))
    close(a, ref_a, 1e-6, "axpby")
    assert torch.equal(a, b2)


@pytest.mark.parametrize("hwc", [False, True])
@pytest.mark.parametrize("shape", [(5, 300, 300, 256), (3, 40, 52, 30), (4, 64, 64, 64)])   # incl. OW % 4 != 0 and no-crop
def test_weak_augment(shape, hwc):
    """'next' row f1: device-side TransformFix.weak vs the oracle's flip-then-crop on the same host-drawn parameters."""
    from oracle import augment_ref as AR
    from ssl_cr_histo_amd import augment as A
    N, SH, SW, S = shape
    src = torch.from_numpy(np.random.RandomState(77).randint(0, 256, (N, 3, SH, SW), dtype=np.uint8))
    g1, g2 = torch.Generator().manual_seed(5), torch.Generator().manual_seed(5)
    prm = A.weak_params(N, (SH, SW), S, g1)
    assert torch.equal(prm, AR.draw_params(N, (SH, SW), S, g2))
    # extreme offsets too
    prm[0] = torch.tensor([1, SH - S, SW - S], dtype=torch.int32)
    prm[1] = torch.tensor([0, 0, SW - S], dtype=torch.int32)
    want = AR.weak_batch(src, prm, S)
    dev_src = (src.permute(0, 2, 3, 1).contiguous() if hwc else src).to(DEV)
    got = A.weak_augment(dev_src, prm, S, src_hwc=hwc)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (N, 3, S, S)
    assert torch.equal(got.cpu(), want)


def test_transform_fix_geometric_both_branches():
    """row f4, deterministic half: both branches of TransformFix (dataset.py:663-677) -- flip + crop of the weak branch, then flip +
    crop of the strong branch, drawn per sample in that order from ONE torch generator -- on the device, bit-exact against the
    CPU restatement."""
    from oracle import augment_ref as A
    from ssl_cr_histo_amd import augment
    n, sh, sw, size = 7, 300, 280, 256
    src = torch.from_numpy(np.random.RandomState(77).randint(0, 256, (n, 3, sh, sw), dtype=np.uint8))
    pw, ps = A.draw_fix_params(n, (sh, sw), size, torch.Generator().manual_seed(5))
    weak, strong = augment.TransformFixGeometric(size, torch.Generator().manual_seed(5))(src.to(DEV))
    assert torch.equal(weak.cpu(), A.weak_batch(src, pw, size))
    assert torch.equal(strong.cpu(), A.weak_batch(src, ps, size))
    assert not torch.equal(pw, ps)                           # the two branches really see different draws
    g = torch.Generator().manual_seed(5)
    mine = augment.fix_params(n, (sh, sw), size, g)
    assert torch.equal(mine[0], pw) and torch.equal(mine[1], ps)


@pytest.mark.parametrize("hwc", [False, True])
def test_hed_colour_augmentation(hwc):
    """row f4: colour_augmentation (models/randaugment.py:17-48) on the device against the numpy restatement of the same lines on
    top of scikit-image 0.15.0's published rgb2hed / hed2rgb (oracle/augment_ref.py).  Both sides are float64; the kernel's log / exp
    are the ROCm device library's, so a value whose x*255 lands within an ulp of an integer could truncate differently: bytes are
    required equal up to one LSB (modulo the reference's own uint8 wrap-around), and in fact all but a handful must be identical."""
    import random
    from oracle import augment_ref as AR
    from ssl_cr_histo_amd import augment as A
    N, H, W = 6, 96, 80
    rs = np.random.RandomState(123)
    src = rs.randint(0, 256, (N, H, W, 3), dtype=np.uint8)
    src[0, :8, :8] = 0
    src[0, 8:16, :8] = 255                                     # saturated corners: the wrap-around of (x * 255).astype(uint8)
    rng_a, rng_b = random.Random(11), random.Random(11)
    shifts = [A.colour_shifts(rng_a) for _ in range(N)]
    assert shifts == [AR.draw_colour_shifts(rng_b) for _ in range(N)]
    shifts[1] = (0.12, -0.09, 0.11)                            # far outside the usual draw: drives values below 0 and above 1
    apply = [True, True, True, False, True, True]
    want = np.stack([AR.colour_augmentation(src[i], *shifts[i]) if apply[i] else src[i] for i in range(N)])
    t = torch.from_numpy(src)
    dev = (t if hwc else t.permute(0, 3, 1, 2)).contiguous().to(DEV)
    got = A.hed_colour_augment(dev, shifts, apply, hwc=hwc)
    got = (got if hwc else got.permute(0, 2, 3, 1)).cpu().numpy()
    assert np.array_equal(got[3], src[3])
    diff = (got.astype(np.int16) - want.astype(np.int16)) % 256
    diff = np.minimum(diff, 256 - diff)
    assert diff.max() <= 1, diff.max()
    assert (diff != 0).sum() <= 8, (diff != 0).sum()
    assert (want != src).mean() > 0.5                          # the op really changed the images


def test_brightness_contrast_and_the_randaugment_colour_subset():
    """row f4: Brightness / Contrast (models/randaugment.py:93-103 -> albumentations 0.1.8 brightness_contrast_adjust) bit-exact
    against the float32 restatement, and RandAugmentDevice drawing like RandAugment.__call__ (:130-144) for the device-served ops."""
    import random
    from oracle import augment_ref as AR
    from ssl_cr_histo_amd import augment as A
    N, H, W = 5, 64, 48
    rs = np.random.RandomState(5)
    src = rs.randint(0, 256, (N, H, W, 3), dtype=np.uint8)
    src[2] = rs.randint(0, 180, (H, W, 3), dtype=np.uint8)     # max(img) < 255: the @clipped bound is the image's own maximum
    ab = [(1.15, 0.1), (0.85, -0.2), (1.2, 0.2), (1.0, 0.0), (0.8, 0.15)]
    apply = [True, True, True, True, False]
    want = np.stack([AR.brightness_contrast_adjust(src[i], *ab[i]) if apply[i] else src[i] for i in range(N)])
    dev = torch.from_numpy(src).permute(0, 3, 1, 2).contiguous().to(DEV)
    got = A.brightness_contrast(dev, ab, apply).permute(0, 2, 3, 1).cpu().numpy()
    assert np.array_equal(got, want)
    assert want[2].max() <= src[2].max()
    # draw order of the parameter helpers == the oracle's restatement of the library's
    ra, rb = random.Random(9), random.Random(9)
    assert [A.brightness_contrast_params(ra, brightness_limit=0.1) for _ in range(6)] == \
           [AR.draw_brightness_contrast(rb, brightness_limit=0.1) for _ in range(6)]
    # RandAugment(n=2, m=10) restricted to the colour ops: per image choices(k=2), randint(1, m), then the op's own draws
    class ColourOnly(A.RandAugmentDevice):
        POOL = tuple(p for p in A.RandAugmentDevice.POOL if p[0] in ("Color", "Brightness", "Contrast"))
    aug = ColourOnly(2, 10, random.Random(21), np.random.RandomState(22))
    out = aug(dev).permute(0, 2, 3, 1).cpu().numpy()
    rng, nrng = random.Random(21), np.random.RandomState(22)
    ref = []
    for i in range(N):
        img = src[i]
        for name, lo, hi in rng.choices(ColourOnly.POOL, k=2):
            v = nrng.randint(1, 10)
            val = (float(v) / 30) * float(hi - lo) + lo
            if name == "Color":
                img = AR.colour_augmentation(img, *AR.draw_colour_shifts(rng))
            else:
                kw = {"brightness_limit": val} if name == "Brightness" else {"contrast_limit": val}
                on, alpha, beta = AR.draw_brightness_contrast(rng, **kw)
                if on:
                    img = AR.brightness_contrast_adjust(img, alpha, beta)
        ref.append(img)
    d = (out.astype(np.int16) - np.stack(ref).astype(np.int16)) % 256
    d = np.minimum(d, 256 - d)
    assert d.max() <= 2 and (d != 0).mean() < 1e-3, (d.max(), (d != 0).mean())


@pytest.mark.parametrize("case", [(1, 16, 16), (1, 16, 32), (3, 16, 16), (5, 48, 32), (33, 32, 32), (140, 32, 32), (641, 16, 16), (20, 64, 64)])
@pytest.mark.parametrize("op", ["plain_stats", "residual_relu_bias", "prologue_stats", "mask"])
def test_conv_pingpong_64(case, op):
    """conv_pp64.hip, the two-group ping-pong form of the bf16 64 -> 64 3x3 conv (layer1 forward / eval-fused forward / both
    dgrads): every operand combination it serves, on tile counts that exercise its walk -- one tile (group 1 never live), two,
    odd counts (group 1 one live stage short), fewer pairs than workgroups, more than one round (513+ tiles), and a 64x64 map."""
    K = _k()
    N, H, W = case
    dtype = 1
    x = q(rnd(91, (N, H, W, 64)), dtype)
    w = q(rnd(92, (64, 3, 3, 64), 0.05), dtype)
    kw, ref_kw = {}, {}
    if op == "residual_relu_bias":
        res, bias = q(rnd(93, (N, H, W, 64)), dtype), rnd(94, (64,))
        kw = dict(residual=to_dev(res, dtype), bias=bias.to(DEV), relu=True)
        ref_kw = dict(residual=res, bias=bias, relu=True)
    if op == "prologue_stats":
        sc, sh = rnd(95, (64,)).abs() + 0.5, rnd(96, (64,))
        kw = dict(in_scale=sc.to(DEV), in_shift=sh.to(DEV), in_relu=True, want_stats=True)
        ref_kw = dict(in_scale=sc, in_shift=sh, in_relu=True)
    if op == "plain_stats":
        kw = dict(want_stats=True)
    if op == "mask":
        xbn = q(rnd(97, (N, H, W, 64), 2.0) + 0.3, dtype)
        sc, sh, mu = rnd(98, (64,)), rnd(99, (64,)), rnd(100, (64,))
        y, stats = K.conv2d(to_dev(x, dtype), to_dev(w, dtype), 1, 1, want_stats=True, mask=(to_dev(xbn, dtype), sc.to(DEV), sh.to(DEV), mu.to(DEV)))
        assert "conv3x3_pp64_kernel<false, 2>" in K.last_conv_kernel, K.last_conv_kernel
        want = R.conv_fwd(x, w, 1, 1)
        g = want * ((xbn * sc + sh) > 0)
        edge = (xbn * sc + sh).abs() < 1e-6
        close(torch.where(edge.to(DEV), torch.zeros_like(y), y), torch.where(edge, torch.zeros_like(g), g), TOL[dtype], "masked dgrad")
        st = stats.double().sum(0).cpu()
        close(st[0], g.double().sum((0, 1, 2)), 3e-3, "sum g")
        close(st[1], (g.double() * (xbn.double() - mu.double())).sum((0, 1, 2)), 3e-3, "sum g (x - mean)")
        return
    out = K.conv2d(to_dev(x, dtype), to_dev(w, dtype), 1, 1, **kw)
    assert "conv3x3_pp64_kernel" in K.last_conv_kernel, K.last_conv_kernel
    want = R.conv_fwd(x, w, 1, 1, **ref_kw)
    if kw.get("want_stats"):
        y, stats = out
        s, ss = R.channel_stats(want)
        st = stats.double().sum(0).cpu()
        close(st[0], s, 2e-3, "sum")
        close(st[1], ss, 2e-3, "sumsq")
    else:
        y = out
    close(y, want, TOL[dtype], f"pp64 {op}")


@pytest.mark.parametrize("in_u8", [True, False])
@pytest.mark.parametrize("shape,split", [((2, 64, 64), 0), ((3, 256, 256), 0), ((5, 224, 224), 2), ((260, 64, 96), 0), ((3, 96, 64), 1)])
def test_stem_conv_pool_fused(shape, split, in_u8):
    """sslcr_stem_conv_pool (eval-mode conv1 + folded BatchNorm + ReLU + maxpool 3x3/2 in one launch, the conv output never in HBM)
    against (a) the oracle ops and (b) the two-kernel path it replaces, bit for bit: several bands and tile columns, more images than
    workgroups (260 > 256: a workgroup walks into its second image), non-square maps, a two-segment input, uint8 and fp32 input."""
    K = _k()
    N, H, W = shape
    dtype = 1
    xu = torch.from_numpy(np.random.RandomState(131).randint(0, 256, (N, 3, H, W), dtype=np.uint8))
    w = rnd(132, (64, 3, 7, 7), 0.03)
    g, b, rm, rv = rnd(133, (64,)).abs() + 0.5, rnd(134, (64,)), rnd(135, (64,)), rnd(136, (64,)).abs() + 0.5
    wp, bias = K.pack_stem(w.to(DEV), dtype, bn=tuple(t.to(DEV) for t in (g, b, rm, rv)))
    xin = (xu if in_u8 else xu.float()).to(DEV)
    if split:
        got = K.stem_conv_pool(xin[:split].contiguous(), wp, bias, x2=xin[split:].contiguous())
    else:
        got = K.stem_conv_pool(xin, wp, bias)
    conv = K.stem_conv(xin, wp, bias=bias, relu=True)
    two, _ = K.bn_relu_maxpool(conv, None, None)
    assert got.shape == two.shape
    assert torch.equal(got.view(torch.int16), two.view(torch.int16)), float((got.float() - two.float()).abs().max())
    if N <= 5:
        f = g / torch.sqrt(rv + 1e-5)
        ref = F.relu(F.conv2d(xu.float(), q(w * f.view(-1, 1, 1, 1), dtype), None, 2, 3) + (b - rm * f).view(1, -1, 1, 1))
        want = R.nhwc(F.max_pool2d(ref, 3, 2, 1))
        close(got, want, TOL[dtype], "fused stem + pool")


def test_stem_conv_pool_rejects_unserved_shapes():
    K = _k()
    from ssl_cr_histo_amd import _lib as L
    w = rnd(132, (64, 3, 7, 7), 0.03)
    wp, bias = K.pack_stem(w.to(DEV), 1, bn=tuple(torch.ones(64, device=DEV) for _ in range(4)))
    for shape in [(2, 3, 56, 40), (1, 3, 32, 32), (2, 3, 30, 34)]:       # conv output not 16-tileable / a single tile column
        with pytest.raises(L.SslcrError):
            K.stem_conv_pool(torch.zeros(shape, dtype=torch.uint8, device=DEV), wp, bias)
    wp32, bias32 = K.pack_stem(w.to(DEV), 0, bn=tuple(torch.ones(64, device=DEV) for _ in range(4)))
    with pytest.raises(L.SslcrError):
        K.stem_conv_pool(torch.zeros((2, 3, 64, 64), dtype=torch.uint8, device=DEV), wp32, bias32)


# ---------------------------------------------------------------- segments: three TripletNet branches in one launch per layer
SEG_CASES = [
    # images per segment, H, W, C, K, R, stride, pad, prologue       (kernel the shape reaches)
    (2, 32, 32, 64, 64, 3, 1, 1, False),      # conv3x3_pp64, few tiles per segment (grid < CUs)
    (2, 32, 32, 64, 64, 3, 1, 1, True),
    (24, 64, 64, 64, 64, 3, 1, 1, True),      # conv3x3_pp64, 85 workgroups per segment walk 384 tiles each
    (3, 32, 32, 128, 128, 3, 1, 1, True),     # conv3x3_h16 ring form
    (44, 32, 32, 128, 128, 3, 1, 1, False),   # conv3x3_h16, more items than workgroups
    (2, 16, 16, 256, 256, 3, 1, 1, True),     # conv3x3_h16, two kout blocks
    (8, 8, 8, 512, 512, 3, 1, 1, True),       # conv3x3_h16, four images per tile
    (128, 8, 8, 512, 512, 3, 1, 1, True),     # ... 32 tiles x 4 kout blocks on 85 workgroups per segment: a kout-block-major walk skips blocks
    (128, 8, 8, 512, 512, 3, 1, 1, False),
    (4, 64, 64, 64, 128, 3, 2, 1, False),     # conv_dma 3x3 / 2
    (8, 32, 32, 128, 256, 1, 2, 0, False),    # conv_dma 1x1 / 2
]


@pytest.mark.parametrize("case", SEG_CASES)
def test_conv_segments_equal_separate_launches(case):
    """sslcr_conv_desc.seg_images: one launch over three segments writes what three launches write (bit for bit), and the statistics
    rows of segment s -- rows [s, s + 1) * rows / 3 -- add up to the rows of the separate launch."""
    K = _k()
    n, H, W, C, Ko, Rr, stride, pad, pro = case
    dtype, nseg = 1, 3
    x = to_dev(rnd(201, (nseg * n, H, W, C)), dtype)
    w = to_dev(rnd(202, (Ko, Rr, Rr, C), 0.05), dtype)
    sc = (rnd(203, (nseg, C)).abs() + 0.5).to(DEV) if pro else None
    sh = rnd(204, (nseg, C), 0.3).to(DEV) if pro else None
    y, st = K.conv2d(x, w, stride, pad, in_scale=sc, in_shift=sh, in_relu=pro, want_stats=True, seg_images=n)
    name = K.last_conv_kernel
    rows = st.shape[0]
    assert rows % nseg == 0
    for s in range(nseg):
        ys, sts = K.conv2d(x[s * n:(s + 1) * n].contiguous(), w, stride, pad, in_scale=sc[s].contiguous() if pro else None,
                           in_shift=sh[s].contiguous() if pro else None, in_relu=pro, want_stats=True)
        assert K.last_conv_kernel == name
        assert torch.equal(y[s * n:(s + 1) * n].view(torch.int16), ys.view(torch.int16)), (s, name)
        got = st[s * rows // nseg:(s + 1) * rows // nseg].double().sum(0)
        want = sts.double().sum(0)
        assert torch.allclose(got, want, rtol=1e-5, atol=1e-3 * float(want.abs().max())), (s, name, float((got - want).abs().max()))


@pytest.mark.parametrize("case", [(2, 32, 32, 64), (24, 64, 64, 64), (3, 32, 32, 128), (2, 16, 16, 256)])
def test_conv_mask_front_end_segments_equal_separate_launches(case):
    """the BatchNorm-backward front end (sslcr_conv_desc.mask_x) over three segments, each with its own BatchNorm: gradients
    bit-equal to three launches, the rows of (sum g, sum g (x - mean)) per segment add up to theirs."""
    K = _k()
    n, H, W, Cn = case
    nseg = 3
    dy = to_dev(rnd(221, (nseg * n, H, W, Cn)), 1)
    w = to_dev(rnd(222, (Cn, 3, 3, Cn), 0.05), 1)
    xbn = to_dev(rnd(223, (nseg * n, H, W, Cn)), 1)
    sc, sh, mu = (rnd(224, (nseg, Cn)).abs() + 0.5).to(DEV), rnd(225, (nseg, Cn), 0.3).to(DEV), rnd(226, (nseg, Cn), 0.2).to(DEV)
    from ssl_cr_histo_amd import _lib as L

    def run(x_, m_, seg):
        # (K.conv2d takes seg_stride from in_scale; with a mask the stride is the mask arrays')
        N_ = x_.shape[0]
        y = torch.empty((N_, H, W, Cn), dtype=x_.dtype, device=x_.device)
        d = L.ConvDesc(L.ptr(x_), L.ptr(w), L.ptr(y), None, None, None, None, None, N_, H, W, Cn, Cn, 3, 3, 1, 1, H, W, H, W, 1, 0, 0, 0, 0, 0, 0, 0, 0)
        d.mask_x, d.mask_scale, d.mask_shift, d.mask_mean = (L.ptr(t) for t in m_)
        d.seg_images, d.seg_stride = (seg, Cn) if seg else (0, 0)
        rows = L.lib().sslcr_conv2d_partial_rows(d)
        st = torch.full((rows, 2, Cn), float("nan"), dtype=torch.float32, device=x_.device)
        d.stats = L.ptr(st)
        L.check(L.lib().sslcr_conv2d(1, d, L.stream_ptr()))
        return y, st

    y, st = run(dy, (xbn, sc, sh, mu), n)
    rows = st.shape[0]
    assert rows % nseg == 0
    for s in range(nseg):
        sl = slice(s * n, (s + 1) * n)
        ys, sts = run(dy[sl].contiguous(), (xbn[sl].contiguous(), sc[s].contiguous(), sh[s].contiguous(), mu[s].contiguous()), 0)
        assert torch.equal(y[sl].view(torch.int16), ys.view(torch.int16)), s
        got, want = st[s * rows // nseg:(s + 1) * rows // nseg].double().sum(0), sts.double().sum(0)
        assert torch.allclose(got, want, rtol=1e-5, atol=1e-3 * float(want.abs().max())), (s, float((got - want).abs().max()))


def test_conv_segments_rejected_where_no_kernel_has_the_form():
    K = _k()
    from ssl_cr_histo_amd import _lib as L
    x32 = torch.zeros((6, 32, 32, 64), dtype=torch.float32, device=DEV)
    w32 = torch.zeros((64, 3, 3, 64), dtype=torch.float32, device=DEV)
    with pytest.raises(L.SslcrError):
        K.conv2d(x32, w32, 1, 1, want_stats=True, seg_images=2)                       # fp32: segments are a bf16 form
    xb = torch.zeros((6, 9, 11, 64), dtype=torch.bfloat16, device=DEV)
    wb = torch.zeros((64, 3, 3, 64), dtype=torch.bfloat16, device=DEV)
    with pytest.raises(L.SslcrError):
        K.conv2d(xb, wb, 1, 1, want_stats=True, seg_images=2)                         # not 16x16-tileable: the 64-pixel-tile kernel
    with pytest.raises(L.SslcrError):
        K.conv2d(torch.zeros((7, 32, 32, 64), dtype=torch.bfloat16, device=DEV), wb, 1, 1, seg_images=2)      # 7 images, segments of 2


def test_bn_finalize_and_bn_act_segments():
    """three BatchNorm batches in one finalize: outputs per segment and the running statistics after the three updates in order,
    against three calls; bn_act over three segments against three calls."""
    K = _k()
    nseg, rows, Cn, count = 3, 96, 128, 4096.0
    part = torch.from_numpy(np.random.RandomState(211).standard_normal((nseg * rows, 2, Cn)).astype(np.float32)).to(DEV)
    part[:, 1] = part[:, 1].abs() * 40 + 50      # sum of squares large enough for a positive variance
    gamma, beta = (rnd(212, (Cn,)).abs() + 0.5).to(DEV), rnd(213, (Cn,)).to(DEV)
    rm0, rv0 = rnd(214, (Cn,)).to(DEV), (rnd(215, (Cn,)).abs() + 0.5).to(DEV)
    rm, rv, nbt = rm0.clone(), rv0.clone(), torch.zeros(1, dtype=torch.int64, device=DEV)
    outs = K.bn_finalize(part, count * rows, gamma, beta, running_mean=rm, running_var=rv, nbt=nbt, nseg=nseg)
    rm1, rv1, nbt1 = rm0.clone(), rv0.clone(), torch.zeros(1, dtype=torch.int64, device=DEV)
    for s in range(nseg):
        one = K.bn_finalize(part[s * rows:(s + 1) * rows].contiguous(), count * rows, gamma, beta, running_mean=rm1, running_var=rv1, nbt=nbt1)
        for a, b in zip(outs, one):
            assert torch.equal(a[s], b), s
    assert torch.equal(rm, rm1) and torch.equal(rv, rv1) and int(nbt) == int(nbt1) == nseg
    x = to_dev(rnd(216, (nseg * 4, 16, 16, Cn)), 1)
    res = to_dev(rnd(217, (nseg * 4, 16, 16, Cn)), 1)
    sc, sh = outs[0], outs[1]
    rsc, rsh = (rnd(218, (nseg, Cn)).abs() + 0.5).to(DEV), rnd(219, (nseg, Cn)).to(DEV)
    for kw in ({}, {"res": res}, {"res": res, "rscale": rsc, "rshift": rsh}):
        y = K.bn_act(x, sc, sh, nseg=nseg, **kw)
        for s in range(nseg):
            kws = {k: (v[s * 4:(s + 1) * 4].contiguous() if k == "res" else v[s].contiguous()) for k, v in kw.items()}
            ys = K.bn_act(x[s * 4:(s + 1) * 4].contiguous(), sc[s].contiguous(), sh[s].contiguous(), **kws)
            assert torch.equal(y[s * 4:(s + 1) * 4].view(torch.int16), ys.view(torch.int16)), (s, list(kw))


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("mode", ["yact_g_in_reduce", "relu_from_x", "plain"])
def test_bn_bwd_segments_equal_separate_launches(mode, dtype):
    """sslcr_bn_bwd_desc.nseg: reduce + apply over three segments against three pairs of launches -- dx, the masked gradient g
    (bit for bit), the sums per segment, dgamma / dbeta after the three contributions in order."""
    K = _k()
    nseg, n, H, W, Cn = 3, 4, 16, 16, 128
    dy = to_dev(rnd(231, (nseg * n, H, W, Cn)), dtype)
    x = to_dev(rnd(232, (nseg * n, H, W, Cn)), dtype)
    ya = to_dev(rnd(233, (nseg * n, H, W, Cn)), dtype) if mode == "yact_g_in_reduce" else None
    sc, sh = (rnd(234, (nseg, Cn)).abs() + 0.5).to(DEV), rnd(235, (nseg, Cn), 0.3).to(DEV)
    mu, inv = rnd(236, (nseg, Cn), 0.2).to(DEV), (rnd(237, (nseg, Cn)).abs() + 0.5).to(DEV)
    kw = dict(yact=ya, relu_from_x=mode == "relu_from_x", want_g=mode == "yact_g_in_reduce", g_in_reduce=mode == "yact_g_in_reduce")
    dg, db = torch.full((Cn,), 0.25, device=DEV), torch.full((Cn,), -0.5, device=DEV)
    dx, sums, g = K.bn_bwd(dy, x, sc, sh, mu, inv, nseg=nseg, dgamma=dg, dbeta=db, **kw)
    dg1, db1 = torch.full((Cn,), 0.25, device=DEV), torch.full((Cn,), -0.5, device=DEV)
    for s in range(nseg):
        sl = slice(s * n, (s + 1) * n)
        kws = dict(kw, yact=ya[sl].contiguous() if ya is not None else None)
        dxs, sums_s, gs = K.bn_bwd(dy[sl].contiguous(), x[sl].contiguous(), sc[s].contiguous(), sh[s].contiguous(), mu[s].contiguous(),
                                   inv[s].contiguous(), dgamma=dg1, dbeta=db1, **kws)
        # (the sums end in fp64 atomics whose order is not fixed, so a coefficient may round differently: not a bit comparison)
        assert torch.allclose(dx[sl].float(), dxs.float(), rtol=1e-2 if dtype == 1 else 1e-5, atol=1e-2 if dtype == 1 else 1e-5), s
        if g is not None:
            assert torch.equal(g[sl].view(torch.uint8), gs.view(torch.uint8)), s
        assert torch.allclose(sums[s], sums_s, rtol=1e-9, atol=1e-9 * float(sums_s.abs().max())), s      # fp64 atomics: order only
    assert torch.allclose(dg, dg1, rtol=1e-6, atol=1e-6) and torch.allclose(db, db1, rtol=1e-6, atol=1e-6)


# ---------------------------------------------------------------- float64 per-element bounds over the route table
def _route_flags(spec):
    f = {}
    for t in spec.split():
        k, _, v = t.partition("=")
        f[k] = int(v) if v else True
    return f


def _channel_scale(seed, n):
    """a per-channel scale with both signs, and channel 0 scaled by 1e3 next to channel 1 scaled by 1e-3: a per-channel epilogue or
    prologue mix-up moves an element by orders of magnitude"""
    s = rnd(seed, (n,)).abs() + 0.25
    s[::3] *= -1.0
    s[0] *= 1e3
    s[1] *= 1e-3
    return s


@pytest.mark.parametrize("row", ROUTES, ids=[f"{r[0]}-{r[1]}-{'x'.join(map(str, r[2]))}-{r[3].replace(' ', '+')}" for r in ROUTES])
def test_conv_route_f64(row):
    """every row of tests/kernel_routes.py through the kernels wrappers: the launch is EXACTLY the row's instance, and y, the
    BatchNorm partial statistics and dW hold the float64 per-element bounds of tests/_f64.py (operands as the kernel sees them).
    The input-gradient ops beside par4: dgrad_t (transposed, with a residual), dgrad_parity (four launches into one NaN-filled
    buffer, each writing its class only, each class bounded with its own taps * K) and scatter (the 1x1 / 2 gradient accumulated
    into a non-zero base: the positions it does not reach stay bit-equal)"""
    K = _k()
    op, dt, shape, spec, name, _ = row
    print(f"\n[row] {op} {'bf16' if dt else 'fp32'} {'x'.join(map(str, shape))} [{spec}]")     # (with -s: heads the row's [f64] lines)
    f = _route_flags(spec)
    N, H, W, C, Ko, Rr, stride, pad = shape
    OH, OW = (H + 2 * pad - Rr) // stride + 1, (W + 2 * pad - Rr) // stride + 1
    seg = f.get("seg", 0)
    nseg, n_img = (N // seg, seg) if seg else (1, N)
    f32 = dt == 0
    x = q(rnd(501, (N, H, W, C)), dt)
    xt, kw = x, {}
    if f.get("in_scale"):
        sc = torch.stack([_channel_scale(502 + s, C) for s in range(nseg)])
        sh = rnd(510, (nseg, C))
        xt = torch.cat([B.xform(x[s * n_img:(s + 1) * n_img], sc[s], sh[s], True, dt) for s in range(nseg)])
        kw = dict(in_scale=(sc if seg else sc[0]).contiguous().to(DEV), in_shift=(sh if seg else sh[0]).contiguous().to(DEV), in_relu=True)
    if seg:
        kw["seg_images"] = seg
    if op == "wgrad":
        dy = q(rnd(511, (N, OH, OW, Ko)), dt)
        base = rnd(512, (Ko, Rr, Rr, C))
        dw = base.clone().to(DEV)
        K.conv2d_wgrad(to_dev(x, dt), to_dev(dy, dt), dw, Rr, Rr, stride, pad, **kw)
        assert K.last_wgrad_kernel == name, K.last_wgrad_kernel
        want, mag = B.conv_wgrad(xt, dy, (Ko, Rr, Rr, C), stride, pad, base=base)
        B.check(dw, want, B.bound(want, mag, N * OH * OW, 0, f32), "wgrad", name, dims="krsc")
        return
    w = q(rnd(513, (Ko, Rr, Rr, C), 0.05), dt)
    if op == "dgrad":
        dy = q(rnd(514, (N, OH, OW, Ko)), dt)
        dx = torch.full((N, H, W, C), float("nan"), dtype=K.tdtype(dt), device=DEV)
        K.conv2d(to_dev(dy, dt), to_dev(w.permute(3, 1, 2, 0).contiguous(), dt), stride, pad, transposed=True, out=dx, out_hw=(H, W),
                 pixel_hw=(OH, OW), pix_mul=2, par4=True)
        assert K.last_conv_kernel == name, K.last_conv_kernel
        want, mag = B.conv_dgrad(dy, w, stride, pad, (H, W))
        B.check(dx, want, B.bound(want, mag, Rr * Rr * Ko, dt, f32), "dgrad", name)
        return
    if op in ("dgrad_t", "dgrad_parity"):
        dy = q(rnd(514, (N, OH, OW, Ko)), dt)
        res = q(rnd(525, (N, H, W, C)), dt)
        wd = to_dev(w.permute(3, 1, 2, 0).contiguous(), dt)
        want, mag = B.conv_dgrad(dy, w, stride, pad, (H, W), residual=res)
        if op == "dgrad_t":
            dx = torch.full((N, H, W, C), float("nan"), dtype=K.tdtype(dt), device=DEV)
            K.conv2d(to_dev(dy, dt), wd, stride, pad, transposed=True, out=dx, pixel_hw=(H, W), residual=to_dev(res, dt))
            assert K.last_conv_kernel == name, K.last_conv_kernel
            B.check(dx, want, B.bound(want, mag, Rr * Rr * Ko, dt, f32), f"dgrad transposed / {stride}", name)
            return
        # one launch per input-pixel parity class into one NaN-filled buffer; each writes its class and nothing else
        dx = torch.full((N, H, W, C), float("nan"), dtype=K.tdtype(dt), device=DEV)
        for ph, pw, tap_mask, _ in B.parity_classes():
            before = dx.clone()
            K.conv2d(to_dev(dy, dt), wd, stride, pad, transposed=True, out=dx, out_hw=(H, W), pixel_hw=((H - ph + 1) // 2, (W - pw + 1) // 2),
                     residual=to_dev(res, dt), pix_mul=2, pix_off=(ph, pw), tap_mask=tap_mask)
            assert K.last_conv_kernel == name, (ph, pw, K.last_conv_kernel)
            B.check_parity_launch(before, dx, ph, pw, "dgrad by parity classes")
        B.check(dx, want, B.parity_bound(want, mag, Ko, dt, f32), "dgrad by parity classes", name)
        return
    if op == "scatter":
        dy = q(rnd(514, (N, OH, OW, Ko)), dt)
        base = q(rnd(526, (N, H, W, C)), dt)
        dx = to_dev(base, dt)
        K.conv2d(to_dev(dy, dt), to_dev(w.permute(3, 1, 2, 0).contiguous(), dt), 1, 0, out=dx, out_hw=(H, W), osh=2, accumulate=True)
        assert K.last_conv_kernel == name, K.last_conv_kernel
        want, mag = B.conv_dgrad(dy, w, stride, pad, (H, W), residual=base)
        B.check_scatter(dx, base, want, B.bound(want, mag, Ko, dt, f32), "1x1 / 2 scatter-accumulate", name)
        return
    bias =rnd(515, (Ko,)) if f.get("bias") else None
    res = q(rnd(516, (N, OH, OW, Ko)), dt) if f.get("residual") else None
    osc = _channel_scale(517, Ko) if f.get("out_scale") else None
    relu = bool(f.get("relu"))
    n = Rr * Rr * C
    if op == "s2pair":
        w1 = q(rnd(518, (Ko, 1, 1, C), 0.1), dt)
        b1 = rnd(519, (Ko,)) if bias is not None else None
        s1 = _channel_scale(520, Ko) if osc is not None else None
        dev = lambda t: t.to(DEV) if t is not None else None      # noqa: E731
        out = K.conv2d_s2_pair(to_dev(x, dt), to_dev(w, dt), to_dev(w1, dt), bias3=dev(bias), bias1=dev(b1), relu3=relu,
                               want_stats=bool(f.get("stats")), scale3=dev(osc), scale1=dev(s1))
        # the pair launches the single conv's instance with PAIR = true (conv_s2_name); the single launch gives the same bits
        ys = K.conv2d(to_dev(x, dt), to_dev(w, dt), stride, pad, bias=dev(bias), relu=relu, out_scale=dev(osc), want_stats=bool(f.get("stats")))
        assert K.last_conv_kernel.replace("<false, ", "<true, ") == name, K.last_conv_kernel
        assert torch.equal((ys[0] if f.get("stats") else ys).view(torch.int16), out[0].view(torch.int16))
        for y, st, ww, bb, ss, r, p, rl, what in ((out[0], out[2] if f.get("stats") else None, w, bias, osc, 3, 1, relu, "3x3 / 2"),
                                                  (out[1], out[3] if f.get("stats") else None, w1, b1, s1, 1, 0, False, "1x1 / 2")):
            want, mag, acc, amag = B.conv_fwd(x, ww, 2, p, out_scale=ss, bias=bb, relu=rl)
            B.check(y, want, B.bound(want, mag, r * r * C, dt, f32), f"pair {what}", name)
            if st is not None:
                B.check_stats(st, acc, amag, r * r * C, f"pair {what} statistics", name, f32)
        return
    if f.get("mask"):
        xbn = q(rnd(521, (N, OH, OW, Ko), 2.0) + 0.3, dt)
        msc, msh, mmu = _channel_scale(522, Ko), rnd(523, (Ko,)), rnd(524, (Ko,))
        y, stats = K.conv2d(to_dev(x, dt), to_dev(w, dt), stride, pad, want_stats=True,
                            mask=(to_dev(xbn, dt), msc.to(DEV), msh.to(DEV), mmu.to(DEV)))
        assert K.last_conv_kernel == name, K.last_conv_kernel
        _, _, acc, amag = B.conv_fwd(x, w, stride, pad)
        # the kernel's mask: fmaf(x, scale, shift) > 0 in fp32; its second sum takes (x - mean) rounded to fp32
        keep = ((xbn.double() * msc.double() + msh.double()).float() > 0).double()
        g, gmag = acc * keep, amag * keep
        B.check(y, g, B.bound(g, gmag, n, dt, f32), "masked dgrad", name)
        d = (xbn.float() - mmu).double().reshape(-1, Ko)
        e = B.bound(g, gmag, n, 0, f32).reshape(-1, Ko)
        g = g.reshape(-1, Ko)
        lam = B.LAM * (g.shape[0] ** 0.5) * B.U
        st = stats.double().sum(0).cpu()
        B.check(st[0], g.sum(0), e.sum(0) + lam * g.abs().sum(0), "sum g", name, dims="k")
        B.check(st[1], (g * d).sum(0), (e * d.abs()).sum(0) + lam * (g * d).abs().sum(0), "sum g (x - mean)", name, dims="k")
        return
    out = K.conv2d(to_dev(x, dt), to_dev(w, dt), stride, pad, bias=bias.to(DEV) if bias is not None else None,
                   residual=to_dev(res, dt) if res is not None else None, relu=relu, out_scale=osc.to(DEV) if osc is not None else None,
                   want_stats=bool(f.get("stats")), **kw)
    assert K.last_conv_kernel == name, K.last_conv_kernel
    y, stats = out if f.get("stats") else (out, None)
    want, mag, acc, amag = B.conv_fwd(xt, w, stride, pad, out_scale=osc, bias=bias, residual=res, relu=relu)
    B.check(y, want, B.bound(want, mag, n, dt, f32), "forward", name)
    if stats is not None:
        if seg:     # segment s owns rows [s, s + 1) * rows / nseg
            rows = stats.shape[0] // nseg
            for s in range(nseg):
                sl = slice(s * n_img, (s + 1) * n_img)
                B.check_stats(stats[s * rows:(s + 1) * rows], acc[sl], amag[sl], n, f"statistics of segment {s}", name, f32)
        else:
            B.check_stats(stats, acc, amag, n, "statistics", name, f32)


# ---------------------------------------------------------------- the one-launch BatchNorm finalize (bn_reduce_finalize_kernel)
def _bn_finalize_outputs():
    """every output of sslcr_bn_finalize on seeded partial rows: plain, segments, C not a multiple of 32, and the sums_out form
    (with its ticket words); the caller's SSLCR_BN_ONE_LAUNCH picks the form"""
    from ssl_cr_histo_amd import _lib as L
    K = _k()
    out = {}
    for nseg, rows, Cn in ((1, 200, 128), (3, 120, 80), (1, 64, 40)):
        g = np.random.RandomState(600 + Cn)
        part = torch.from_numpy(g.standard_normal((rows, 2, Cn)).astype(np.float32))
        part[:, 1] = part[:, 1].abs() * 30 + 40
        part = part.to(DEV)
        gamma, beta = (rnd(601, (Cn,)).abs() + 0.5).to(DEV), rnd(602, (Cn,)).to(DEV)
        rm, rv, nbt = rnd(603, (Cn,)).to(DEV), (rnd(604, (Cn,)).abs() + 0.5).to(DEV), torch.zeros(1, dtype=torch.int64, device=DEV)
        res = K.bn_finalize(part, 4096.0 * rows / nseg, gamma, beta, running_mean=rm, running_var=rv, nbt=nbt, replay=3, nseg=nseg)
        for k, t in zip(("scale", "shift", "mean", "invstd", "rm", "rv", "nbt"), res + (rm, rv, nbt)):
            out[f"{nseg}/{Cn}/{k}"] = t.cpu()
        # sums_out: rows -> per-segment sums only
        sums = torch.full((nseg, 2, Cn), float("nan"), dtype=torch.float64, device=DEV)
        stage = torch.empty((nseg, 32, 2, Cn), dtype=torch.float64, device=DEV)
        tickets = torch.zeros((Cn + 31) // 32, dtype=torch.int32, device=DEV)
        d = L.BnFinalizeDesc(L.ptr(part), rows, Cn, 0.0, None, None, None, None, None, None, None, None, None, 0.1, 1e-5, 1,
                             L.ptr(sums), None, L.ptr(stage), nseg if nseg > 1 else 0, 2 * Cn if nseg > 1 else 0, L.ptr(tickets))
        L.check(L.lib().sslcr_bn_finalize(d, L.stream_ptr()))
        out[f"{nseg}/{Cn}/sums"] = sums.cpu()
        out[f"{nseg}/{Cn}/tickets"] = tickets.cpu()
    torch.cuda.synchronize()
    return out


def test_bn_finalize_one_launch_same_bits(tmp_path):
    """SSLCR_BN_ONE_LAUNCH=1 (read once into a static, so in a child process of its own): the ticketed one-launch finalize gives the
    two-launch form's bits -- segments, C not a multiple of 32, sums_out -- and leaves every ticket word at zero"""
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    path = tmp_path / "one_launch.pt"
    code = (f"import sys; sys.path[:0] = [{os.path.dirname(here)!r}, {here!r}]\n"
            "import torch, test_kernels_gpu as T\n"
            f"torch.save(T._bn_finalize_outputs(), {str(path)!r})\n")
    env = dict(os.environ, SSLCR_BN_ONE_LAUNCH="1")
    r = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    one = torch.load(path)
    assert "SSLCR_BN_ONE_LAUNCH" not in os.environ
    two = _bn_finalize_outputs()
    assert one.keys() == two.keys()
    for k in two:
        assert torch.equal(one[k], two[k]), k
        if k.endswith("tickets"):
            assert int(one[k].abs().sum()) == 0, k
    assert bool(torch.isfinite(two["3/80/sums"]).all())


# ---------------------------------------------------------------- the non-conv kernels against float64 (tests/nonconv_cases.py, tests/_f64.py)
import nonconv_cases as NC  # noqa: E402


def _nc_id(row):
    op, dt, shape, flags, _ = row
    d = {None: "", 0: "-f32", 1: "-bf16"}[dt]
    return f"{op}{d}-{'x'.join('N' if v is None else str(v) for v in shape)}" + ("-" + flags.replace(" ", "+") if flags else "")


def _nc(table):
    return pytest.mark.parametrize("row", table, ids=[_nc_id(r) for r in table])


def _ew_cap():
    """workgroups ew_grid() caps an elementwise launch at: three per CU of the device"""
    return 3 * torch.cuda.get_device_properties(0).multi_processor_count


def _over_cap(shape, dt, C=None):
    """N = None -> the smallest batch whose 16-byte chunks exceed the capped grid's stride by 4 %"""
    N, H, W, Cn = shape
    if N is None:
        cols = Cn // (8 if dt == 1 else 4)
        N = -(-int(1.04 * _ew_cap() * 256) // (H * W * cols))
        assert N * H * W * cols > _ew_cap() * 256
    return N, H, W, Cn


def _consts(seed, C, nseg=1):
    sc = torch.stack([_channel_scale(seed + 7 * s, C) for s in range(nseg)])
    sh = rnd(seed + 1, (nseg, C))
    return (sc, sh) if nseg > 1 else (sc[0], sh[0])


def _bits(t):
    """the sign mask sslcr_bn_act writes: bit (e & 7) of byte e >> 3 = (t.flatten()[e] > 0)"""
    m = (t.flatten() > 0).view(-1, 8).to(torch.int32)
    return (m << torch.arange(8, dtype=torch.int32, device=t.device).view(1, 8)).sum(1).to(torch.uint8)


def _run_bn_act(K, dt, shape, f, seed=700):
    N, H, W, C = shape
    nseg = 3 if f.get("nseg3") else 1
    x = q(rnd(seed, (N, H, W, C), 2.0), dt)
    sc, sh = _consts(seed + 1, C, nseg)
    res = q(rnd(seed + 3, (N, H, W, C)), dt) if (f.get("res") or f.get("bnres")) else None
    rsc, rsh = _consts(seed + 4, C, nseg) if f.get("bnres") else (None, None)
    dev = lambda t: t.contiguous().to(DEV) if t is not None else None      # noqa: E731
    out = K.bn_act(to_dev(x, dt), dev(sc), dev(sh), res=to_dev(res, dt) if res is not None else None, rscale=dev(rsc), rshift=dev(rsh),
                   relu=bool(f.get("relu")), nseg=nseg, want_bits=bool(f.get("bits")))
    y, bits = out if f.get("bits") else (out, None)
    want, mag = B.bn_act_ref(x, sc, sh, res, rsc, rsh, relu=bool(f.get("relu")))
    return y, bits, want, mag


@_nc(NC.BN_ACT + [r for r in NC.STRIDE if r[0] == "bn_act"])
def test_bn_act_f64(row):
    """relu(fma(x, sc, sh) + fma(r, rsc, rsh)) per element against float64; ybits = the sign of the STORED value, bit for bit.  The rows
    with N = None lie above the grid cap: every thread takes a second trip with the constants it cached before the loop"""
    K = _k()
    _, dt, shape, spec, _ = row
    f = _route_flags(spec)
    shape = _over_cap(shape, dt)
    y, bits, want, mag = _run_bn_act(K, dt, shape, f)
    B.check(y, want, B.bound(want, mag, 0, dt), "bn_act " + spec, "bn_act_kernel")
    if bits is not None:
        assert torch.equal(bits, _bits(y.float())), "ybits != sign of the stored y"


def _pool_inputs(dt, shape, seed=720):
    N, H, W, C = shape
    x = q(rnd(seed, (N, H, W, C), 2.0), dt)
    sc, sh = rnd(seed + 1, (C,)), rnd(seed + 2, (C,))
    sc[1], sh[1] = 0.0, 0.25          # scale == 0: every window element ties at 0.25 -- the first one inside the map wins
    if C > 9:
        sc[9], sh[9] = 0.0, -0.5      # ... and ties at a non-positive value: code 9
    sc[0], sc[2] = sc[0] * 1e3, sc[2] * 1e-3
    return x, sc, sh


def _check_pool_fwd(K, dt, x, sc, sh, what):
    pooled, am = K.bn_relu_maxpool(to_dev(x, dt), sc.to(DEV), sh.to(DEV))
    r = B.maxpool_ref(x, sc, sh, dt)
    B.check(pooled, r["y"], r["bnd"], what + " values", "bn_relu_maxpool")
    B.capped(r["unsure"], what + " near-ties")
    got = am.cpu().long()
    ok = (got == r["code"]) | r["unsure"]
    assert bool(ok.all()), f"{what}: {int((~ok).sum())} argmax codes differ from the float64 window, first at {tuple(int(v) for v in (~ok).nonzero()[0])}"
    return pooled, am, r


@_nc([r for r in NC.STRIDE if r[0] == "bn_relu_maxpool"])
def test_maxpool_generic_above_the_cap_f64(row):
    """the generic pooling form (chunks per pixel do not divide 256) on an output above the grid cap: values and codes"""
    K = _k()
    _, dt, shape, _, _ = row
    N, OH, OW, C = _over_cap(shape, dt)
    x, sc, sh = _pool_inputs(dt, (N, 2 * OH, 2 * OW, C))
    sc, sh = _channel_scale(731, C), rnd(732, (C,))          # constants a foreign chunk cannot stand in for
    _check_pool_fwd(K, dt, x, sc, sh, f"generic max-pool C={C}")


@_nc(NC.POOL)
def test_pool_f64(row):
    """max-pool forward (values, argmax codes against the float64 window), its backward through the codes, avg-pool forward / backward"""
    K = _k()
    _, dt, shape, spec, _ = row
    f = _route_flags(spec)
    shape = _over_cap(shape, dt)
    N, H, W, C = shape
    x, sc, sh = _pool_inputs(dt, shape)
    if f.get("bwd_only"):
        r = B.maxpool_ref(x, sc, sh, dt)
        pooled, am = to_dev(q(r["y"].float(), dt), dt), r["code"].to(torch.uint8).to(DEV)
    else:
        pooled, am, r = _check_pool_fwd(K, dt, x, sc, sh, "max-pool")
    OH, OW = pooled.shape[1:3]
    dyp = q(rnd(725, (N, OH, OW, C)), dt)
    dx = K.maxpool_relu_bwd(to_dev(dyp, dt), am, to_dev(x, dt), sc.to(DEV), sh.to(DEV))
    want, mag = B.maxpool_bwd_ref(dyp, am.cpu(), r["pre"], (H, W))
    unsure = B.mask_unsure(r["pre"], r["premag"])
    B.capped(unsure, "pre-activations at the ReLU threshold")
    bnd = torch.where(unsure, torch.full_like(mag, math.inf), B.bound(want, mag, 0, dt))
    B.check(dx, want, bnd, "max-pool backward", "maxpool_relu_bwd_kernel")
    ps = pooled.float().cpu()
    ap = K.avgpool_fwd(pooled)
    a64, amag, hw = B.avgpool_ref(ps)
    B.check(ap, a64, B.bound(a64, amag, hw, 0), "avg-pool", "avgpool_fwd_kernel", dims="nc")
    dyv = rnd(726, (N, C))
    full = (N, H, W, C) if f.get("bwd_only") else tuple(pooled.shape)          # above the cap: the un-pooled map
    dap = K.avgpool_bwd(dyv.to(DEV), full, dt)
    w64 = (dyv.double() / (full[1] * full[2]))[:, None, None, :].expand(full)
    B.check(dap, w64, B.bound(w64, w64.abs(), 0, dt), "avg-pool backward", "avgpool_bwd_kernel")


def _bn_bwd_inputs(dt, shape, nseg, seed=740):
    """x with a channel of mean / std = 30, and the fp32 constants a forward would have left: per segment"""
    N, H, W, C = shape
    x = rnd(seed, (N, H, W, C), 2.0) + 0.7
    x[..., 2] = rnd(seed + 1, (N, H, W)) + 30.0
    x = q(x, dt)
    gamma, beta = _channel_scale(seed + 2, C), rnd(seed + 3, (C,))
    xs = x.double().reshape(nseg, -1, C)
    mean, var = xs.mean(1), xs.var(1, unbiased=False)
    invstd = 1.0 / torch.sqrt(var + 1e-5)
    sc = (gamma.double() * invstd).float()
    sh = (beta.double() - mean * gamma.double() * invstd).float()
    sq = (lambda t: t.contiguous()) if nseg > 1 else (lambda t: t[0].contiguous())
    return x, sq(sc), sq(sh), sq(mean.float()), sq(invstd.float())


@_nc(NC.BN_BWD)
def test_bn_bwd_f64(row):
    """both sums of the reduce pass, g, dx = cA g + cB x + cC from the kernel's own sums, and the affine gradients, against float64 --
    g formed as each mode forms it"""
    K = _k()
    _, dt, shape, spec, _ = row
    f = _route_flags(spec)
    N, H, W, C = shape
    nseg = 3 if f.get("nseg3") else 1
    x, sc, sh, mean, invstd = _bn_bwd_inputs(dt, shape, nseg)
    count = N * H * W // nseg
    dev = lambda t: t.to(DEV) if t is not None else None      # noqa: E731
    dy = q(rnd(745, (N, H, W, C)), dt)
    kw, g_err, gather = {}, None, 0
    yact = None
    base_g, base_b = rnd(746, (C,)), rnd(747, (C,))
    dg, db = base_g.to(DEV), base_b.to(DEV)
    pooled_form = f.get("pool") or f.get("pool_y")
    if pooled_form:
        sc = sc.clone()
        sc[5] = 0.0                                  # (pool_y: a channel that cannot be inverted fetches x at the argmax position)
        sh = sh.clone()
        sh[5] = 0.25
        pooled, am = K.bn_relu_maxpool(to_dev(x, dt), dev(sc), dev(sh))
        dyp = q(rnd(748, tuple(pooled.shape)), dt)
        kw = dict(relu_from_x=True, pool=(to_dev(dyp, dt), am) + ((pooled,) if f.get("pool_y") else ()))
        g64, gmag = B.bn_bwd_g(None, x, sc, sh, relu_from_x=True, pool=(dyp, am.cpu()))
        g_err, gather = 3 * B.U * gmag, 3
        dx, sums, g = K.bn_bwd(None, to_dev(x, dt), dev(sc), dev(sh), dev(mean), dev(invstd), want_g=True, dgamma=dg, dbeta=db, **kw)
    else:
        if f.get("yact") or f.get("yact_gir") or f.get("yact_bits"):
            ya, _ = B.bn_act_ref(x, sc, sh, relu=True)
            yact = q(ya.float(), dt)
            kw = dict(yact=to_dev(yact, dt), g_in_reduce=bool(f.get("yact_gir")))
            if f.get("yact_bits"):
                kw["yact_bits"] = _bits(kw["yact"].float())
        elif f.get("from_x"):
            kw = dict(relu_from_x=True)
        g64, gmag = B.bn_bwd_g(dy, x, sc, sh, yact=yact, relu_from_x=bool(f.get("from_x")))
        dx, sums, g = K.bn_bwd(to_dev(dy, dt), to_dev(x, dt), dev(sc), dev(sh), dev(mean), dev(invstd), want_g=True, nseg=nseg,
                               dgamma=dg, dbeta=db, **kw)
    name = "bn_bwd " + spec
    if f.get("pool_y"):
        s64, sb = B.bn_bwd_pool_sums_ref(dyp, pooled.float().cpu(), am.cpu(), x, sc, sh, mean)
        B.check(sums.cpu(), s64, sb, name + " sums", "bn_bwd_reduce_pool_kernel", dims="sc")
    else:
        s64, sb = B.bn_bwd_sums_ref(g64, gmag, x, mean, gather)
        B.check(sums.cpu().view(nseg, 2, C), s64, sb, name + " sums", "bn_bwd_reduce_kernel", dims="zsc")
    if gather:
        B.check(g, g64, B.bound(g64, gmag, 0, dt), name + " g", "bn_bwd_g")
    else:
        assert torch.equal(g.float().cpu().double(), g64), "g is dy under the mask, bit for bit"
    want, bnd = B.bn_bwd_apply_ref(g64, x, sc, invstd, mean, sums, count, dt, g_err)
    B.check(dx, want, bnd, name + " dx", "bn_bwd_apply")
    wg, bg, wb, bb = B.bn_param_grads_ref(sums, invstd, base_g, base_b)
    B.check(dg, wg, bg, name + " dgamma", "bn_bwd_param_grads", dims="c")
    B.check(db, wb, bb, name + " dbeta", "bn_bwd_param_grads", dims="c")
    # sslcr_bn_param_grads, the stand-alone launch: the same two roundings onto the same values
    if nseg == 1:
        dg2, db2 = base_g.to(DEV), base_b.to(DEV)
        K.bn_param_grads(sums, dev(invstd), dg2, db2)
        B.check(dg2, wg, bg, name + " dgamma (bn_param_grads)", "bn_param_grads_kernel", dims="c")
        B.check(db2, wb, bb, name + " dbeta (bn_param_grads)", "bn_param_grads_kernel", dims="c")


@_nc([r for r in NC.STRIDE if r[0] == "bn_bwd_apply"])
def test_bn_bwd_apply_odd_width_above_the_cap_f64(row):
    """sslcr_bn_bwd_apply alone (the reduce pass rejects these widths) from sums the test provides, above the grid cap"""
    K = _k()
    _, dt, shape, spec, _ = row
    f = _route_flags(spec)
    shape = _over_cap(shape, dt)
    N, H, W, C = shape
    x, sc, sh, mean, invstd = _bn_bwd_inputs(dt, shape, 1)
    dy = q(rnd(745, shape), dt)
    yact = None
    if f.get("yact"):
        yact = q(B.bn_act_ref(x, sc, sh, relu=True)[0].float(), dt)
    g64, gmag = B.bn_bwd_g(dy, x, sc, sh, yact=yact, relu_from_x=bool(f.get("relu_from_x")))
    xm = x.double() - mean.double()
    sums = torch.stack([g64.reshape(-1, C).sum(0), (g64 * xm).reshape(-1, C).sum(0)]).to(DEV)
    dx, _, g = K.bn_bwd(to_dev(dy, dt), to_dev(x, dt), sc.to(DEV), sh.to(DEV), mean.to(DEV), invstd.to(DEV), want_g=True, sums=sums,
                        yact=to_dev(yact, dt) if yact is not None else None, relu_from_x=bool(f.get("relu_from_x")))
    assert torch.equal(g.float().cpu().double(), g64), "g is dy under the mask, bit for bit"
    want, bnd = B.bn_bwd_apply_ref(g64, x, sc, invstd, mean, sums, N * H * W, dt)
    B.check(dx, want, bnd, f"bn_bwd_apply C={C} " + spec, "bn_bwd_apply_kernel")


def test_cases_above_the_cap_would_meet_the_cached_constant_defect():
    """the stride rows are only worth their time if a grid capped WITHOUT the rounding would hand their threads foreign constants"""
    cap = _ew_cap()
    for _, dt, shape, _, _ in NC.STRIDE:
        N, H, W, C = _over_cap(shape, dt)
        cols = C // (8 if dt == 1 else 4)
        items = N * H * W * cols
        col = torch.arange(items) % cols
        assert int((B.cached_column(items, cols, B.capped_grid(items, cap)) != col).sum()) > 0, (shape, dt)
        assert int((B.cached_column(items, cols, B.rounded_grid(items, cols, cap)) != col).sum()) == 0, (shape, dt)


def _finalize_partials(rows, C, count1, seed=760):
    """fp32 partial rows of a tensor with channel 0 at mean / std = 1e3 and a constant channel 1; k elements per row"""
    k = 1 if count1 else 16
    g = np.random.RandomState(seed)
    mu, sd = g.standard_normal(C) * 2.0, np.abs(g.standard_normal(C)) + 0.5
    mu[0], sd[0] = 1e3, 1.0
    sd[1], mu[1] = 0.0, 2.5
    v = mu[None, None, :] + sd[None, None, :] * g.standard_normal((rows, k, C))
    part = np.stack([v.sum(1), (v * v).sum(1)], 1).astype(np.float32)
    return torch.from_numpy(part), float(rows * k)


@_nc(NC.BN_FINALIZE)
def test_bn_finalize_f64(row):
    """scale, shift, mean, invstd and the running statistics after three replayed updates, from fp32 partial rows, against an
    extended-precision reference: the final fp32 rounding plus the double roundoff through the variance's condition number"""
    K = _k()
    _, _, (rows, C, nseg), spec, _ = row
    f = _route_flags(spec)
    part, total = _finalize_partials(rows, C, f.get("count1"))
    count = total / nseg
    gamma, beta = _channel_scale(761, C), rnd(762, (C,))
    rm, rv = rnd(763, (C,)), rnd(764, (C,)).abs() + 0.5
    rm_d, rv_d = rm.to(DEV), rv.to(DEV)
    nbt = torch.zeros((), dtype=torch.int64, device=DEV)
    got = K.bn_finalize(part.to(DEV), count, gamma.to(DEV), beta.to(DEV), running_mean=rm_d, running_var=rv_d, nbt=nbt, replay=3, nseg=nseg)
    ref = B.bn_finalize_ref(part, count, gamma, beta, rm, rv, replay=3, nseg=nseg)
    for name, t in zip(("scale", "shift", "mean", "invstd"), got):
        B.check(t.view(nseg, C), ref[name][0], ref[name][1], f"bn_finalize {rows}x{C}/{nseg} {name}", "bn_finalize_kernel", dims="zc")
    B.check(rm_d, *ref["running_mean"], f"bn_finalize {rows}x{C}/{nseg} running_mean", "bn_finalize_kernel", dims="c")
    B.check(rv_d, *ref["running_var"], f"bn_finalize {rows}x{C}/{nseg} running_var", "bn_finalize_kernel", dims="c")
    assert int(nbt.item()) == 3 * nseg
    assert float(got[3].view(nseg, C)[0, 1]) == pytest.approx(1.0 / math.sqrt(float(np.float32(1e-5))), rel=1e-6)      # the constant channel


@_nc(NC.GEMM)
def test_linear_f64(row):
    """forward (bias + ReLU, and plain), dx, dw and db into non-zero buffers, with and without the ReLU mask, against float64"""
    K = _k()
    _, _, (M, Kd, Nn), _, _ = row
    x, w, b = rnd(781, (M, Kd)), rnd(782, (Nn, Kd), 0.03), rnd(783, (Nn,))
    xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
    y = K.linear_fwd(xd, wd, bd, relu=True)
    want, mag = B.linear_ref(x, w, bias=b, relu=True)
    B.check(y, want, B.bound(want, mag, Kd, 0, True), "linear forward", "gemm_f32", dims="mn")
    want, mag = B.linear_ref(x, w)
    B.check(K.linear_fwd(xd, wd, None, relu=False), want, B.bound(want, mag, Kd, 0, True), "linear forward, plain", "gemm_f32", dims="mn")
    dy = rnd(784, (M, Nn))
    for masked in (True, False):
        g = torch.where(y.cpu() > 0, dy, torch.zeros_like(dy)) if masked else dy
        base_w, base_b, base_x = rnd(785, (Nn, Kd)), rnd(786, (Nn,)), rnd(787, (M, Kd))
        dw, db, dxb = base_w.to(DEV), base_b.to(DEV), base_x.to(DEV)
        dx = K.linear_bwd(xd, wd, dy.to(DEV), yact=y if masked else None, dw=dw, db=db)
        tag = " (masked)" if masked else ""
        want, mag = B.linear_ref(g, w.t())
        B.check(dx, want, B.bound(want, mag, Nn, 0, True), "linear dx" + tag, "gemm_f32", dims="mk")
        want, mag = B.linear_ref(g.t(), x.t(), base=base_w)
        B.check(dw, want, B.bound(want, mag, M, 0, True), "linear dw" + tag, "gemm_f32", dims="nk")
        want, mag = B.colsum_ref(g, base_b)
        B.check(db, want, B.bound(want, mag, M, 0), "linear db" + tag, "relu_mask_colsum_kernel", dims="n")
        K.linear_bwd(xd, wd, dy.to(DEV), yact=y if masked else None, dx=dxb, dx_accumulate=True)
        want, mag = B.linear_ref(g, w.t(), base=base_x)
        B.check(dxb, want, B.bound(want, mag, Nn, 0, True), "linear dx accumulated" + tag, "gemm_f32", dims="mk")


def _logits(seed, shape, shift=False):
    t = rnd(seed, shape)
    t = t * (80.0 / float(t.abs().max()))
    if shift:
        t[0] += 100.0
        t[1] -= 100.0
    return t


def test_device_expf_error_measured():
    """the one constant of tests/_f64.py that cannot be derived: the device expf (and the add and divide around it) through softmax_col on
    two-column logits (0, t), t in [-87, 0], against float64.  The recorded worst value must still hold"""
    K = _k()
    t = torch.from_numpy(-87.0 * np.random.RandomState(790).random_sample(200000).astype(np.float32))
    lg = torch.stack([torch.zeros_like(t), t], 1).contiguous()
    got = K.softmax_col(lg.to(DEV), 1).cpu().double()
    e = torch.exp(t.double())
    p = e / (1.0 + e)
    worst = float(((got - p).abs() / (B.U * p)).max())
    print(f"[f64] device expf through softmax_col | softmax_col_kernel | worst error {worst:.4f} u (recorded {B.EXPLOG_MEASURED_ULP})")
    assert worst <= B.EXPLOG_MEASURED_ULP, f"measured {worst:.4f} u > the recorded {B.EXPLOG_MEASURED_ULP} u: re-derive EXPLOG_ULP"


@_nc(NC.LOSS)
def test_loss_f64(row):
    """the three losses and dlogits against float64 with nx = 300 / nu = 700 rows (every thread's row loop takes a second trip) and
    logits up to +-80; 'shift': rows offset by +-100, where softmax without the max subtraction overflows"""
    K = _k()
    _, _, (kind, Cn, nx, nu), spec, _ = row
    shift = "shift" in spec
    lg = _logits(800 + Cn, (nx + nu, Cn), shift)
    lt = _logits(801 + Cn, (max(nu, 1), Cn))
    lam = float(np.float32(0.7))
    inx, inu = float(np.float32(1.0 / nx)), float(np.float32(1.0 / max(1, nu)))
    ce = kind in (1, 2)
    if ce:
        tgt = torch.from_numpy(np.random.RandomState(802).randint(0, Cn, (nx,)).astype(np.int64))
        out, dl = K.loss(kind, lg.to(DEV), logits_t=lt.to(DEV) if kind == 1 else None, target_i=tgt.to(DEV), nx=nx, lambda_u=0.7)
        rows, e_rows, dlx, e_dlx = B.ce_rows(lg[:nx], tgt, inx)
        lx, ex = B.loss_total(rows, e_rows, inx, 0)
        correct = int((lg[:nx].argmax(1) == tgt).sum())
    else:
        tf = rnd(803, (nx,)).abs() * 40.0
        out, dl = K.loss(kind, lg.to(DEV), logits_t=lt.to(DEV) if kind == 0 else None, target_f=tf.to(DEV), nx=nx, lambda_u=0.7)
        sq, dlx, e_dlx = B.mse_rows(lg[:nx], tf.view(-1, 1).expand(nx, Cn), inx)
        lx, ex = B.loss_total(sq, torch.zeros(()), inx / Cn, 3)
        correct = None
    lu, eu = 0.0, 0.0
    dlu = e_dlu = torch.zeros((nu, Cn), dtype=torch.float64)
    if kind == 1:
        rows, e_rows, dlu, e_dlu = B.ce_rows(lg[nx:], lt.argmax(1), lam * inu)
        lu, eu = B.loss_total(rows, e_rows, inu, 0)
    elif kind == 0:
        sq, dlu, e_dlu = B.mse_rows(lg[nx:], lt, lam * inu, ops=5)
        lu, eu = B.loss_total(sq, torch.zeros(()), inu / Cn, 3)
    total = lx + lam * lu
    et = ex + lam * eu + 2 * B.U * (abs(lx) + lam * abs(lu))
    o = out.cpu()
    B.check(o[:3], torch.tensor([total, lx, lu], dtype=torch.float64), torch.tensor([et, ex, eu], dtype=torch.float64),
            f"loss kind {kind} C={Cn} {spec}", "loss_kernel", dims="i")
    if correct is not None:
        assert int(o[3]) == correct
    B.check(dl, torch.cat([dlx, dlu]), torch.cat([e_dlx, e_dlu]), f"dlogits kind {kind} C={Cn} {spec}", "loss_kernel", dims="nc")


@_nc(NC.SOFTMAX)
def test_softmax_col_f64(row):
    K = _k()
    _, _, (n, Cn), _, _ = row
    lg = _logits(810 + Cn, (n, Cn))
    for col in (0, Cn - 1):
        want, bnd = B.softmax_col_ref(lg, col)
        B.check(K.softmax_col(lg.to(DEV), col), want, bnd, f"softmax_col C={Cn} col={col}", "softmax_col_kernel", dims="n")


def _stem_operands(K, shape, in_u8, dtype, seed):
    N, H, W = shape
    xu = torch.from_numpy(np.random.RandomState(seed).randint(0, 256, (N, 3, H, W), dtype=np.uint8))
    w = rnd(seed + 1, (64, 3, 7, 7), 0.03)
    bn = (_channel_scale(seed + 2, 64), rnd(seed + 3, (64,)), rnd(seed + 4, (64,)), rnd(seed + 5, (64,)).abs() + 0.5)
    xin = (xu if in_u8 else xu.float()).to(DEV)
    return xu, xu.permute(0, 2, 3, 1).double(), w, bn, xin


def _check_folded_pack(w, bn, wk2, bias, dtype):
    g, b, rm, rv = (t.double() for t in bn)
    f = g / torch.sqrt(rv + float(np.float32(1e-5)))
    w64 = w.double().permute(0, 2, 3, 1) * f.view(-1, 1, 1, 1)
    B.check(wk2, w64, B.bound(w64, w64.abs(), 0, dtype), "folded stem filter", "pack_stem_kernel", dims="krsc")
    B.check(bias, b - rm * f, 6 * B.U * (b.abs() + (rm * f).abs()), "folded stem bias", "pack_stem_kernel", dims="k")


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("in_u8", [True, False])
@pytest.mark.parametrize("shape", [(2, 64, 64), (3, 56, 40), (1, 256, 256), (2, 30, 34)])
def test_stem_f64(shape, in_u8, dtype):
    """the shapes of test_stem against float64: forward + partial statistics, the folded form, both weight gradients (into a non-zero
    buffer; the pooled form from the dY its own apply pass stores) -- reduction lengths 147 and N * OH * OW"""
    K = _k()
    f32 = dtype == 0
    xu, x, w, bn, xin = _stem_operands(K, shape, in_u8, dtype, 831)
    N = shape[0]
    wp, _ = K.pack_stem(w.to(DEV), dtype)
    wk = B.stem_unpack(wp)
    assert torch.equal(wk, q(w, dtype).permute(0, 2, 3, 1)), "the plain pack is the filter rounded to the storage dtype"
    y, stats = K.stem_conv(xin, wp, want_stats=True)
    want, mag, acc, amag = B.conv_fwd(x, wk, 2, 3)
    B.check(y, want, B.bound(want, mag, 147, dtype, f32), "stem forward", "stem_fwd_kernel")
    B.check_stats(stats, acc, amag, 147, "stem statistics", "stem_fwd_kernel", f32)
    wp2, bias = K.pack_stem(w.to(DEV), dtype, bn=tuple(t.to(DEV) for t in bn))
    wk2 = B.stem_unpack(wp2)
    _check_folded_pack(w, bn, wk2, bias, dtype)
    y2 = K.stem_conv(xin, wp2, bias=bias, relu=True)
    want2, mag2, _, _ = B.conv_fwd(x, wk2, 2, 3, bias=bias.cpu(), relu=True)
    B.check(y2, want2, B.bound(want2, mag2, 147, dtype, f32), "stem folded", "stem_fwd_kernel")
    OH, OW = want.shape[1:3]
    dy = q(rnd(837, (N, OH, OW, 64)), dtype)
    base = rnd(838, (64, 3, 7, 7))
    dw = base.clone().to(DEV)
    K.stem_wgrad(xin, to_dev(dy, dtype), dw)
    wantw, magw = B.conv_wgrad(x, dy, (64, 7, 7, 3), 2, 3, base=base.permute(0, 2, 3, 1))
    B.check(dw.permute(0, 2, 3, 1), wantw, B.bound(wantw, magw, N * OH * OW, 0, f32), "stem wgrad", "stem_wgrad", dims="krsc")
    # the pooled form: bn0's backward apply on the tile in LDS -- dY is what sslcr_bn_bwd_apply stores (checked in test_bn_bwd_f64)
    gamma, beta = bn[0].abs() * 0.01 + 0.5, bn[1]
    sc, sh, mean, invstd = K.bn_finalize(stats, N * OH * OW, gamma.to(DEV), beta.to(DEV))
    pooled, am = K.bn_relu_maxpool(y, sc, sh)
    dyp = to_dev(q(rnd(839, tuple(pooled.shape)), dtype), dtype)
    dx, _, _ = K.bn_bwd(None, y, sc, sh, mean, invstd, relu_from_x=True, pool=(dyp, am, pooled))
    dw2 = base.clone().to(DEV)
    K.stem_wgrad_pool(xin, dw2, y, sc, sh, mean, invstd, (dyp, am, pooled))
    wantp, magp = B.conv_wgrad(x, dx.float().cpu(), (64, 7, 7, 3), 2, 3, base=base.permute(0, 2, 3, 1))
    B.check(dw2.permute(0, 2, 3, 1), wantp, B.bound(wantp, magp, N * OH * OW, 0, f32), "stem wgrad from the pooled gradient", "stem_wgrad_pool", dims="krsc")


@pytest.mark.parametrize("in_u8", [True, False])
@pytest.mark.parametrize("shape,split", [((2, 64, 64), 0), ((3, 256, 256), 0), ((5, 224, 224), 2), ((260, 64, 96), 0), ((3, 96, 64), 1)])
def test_stem_conv_pool_f64(shape, split, in_u8):
    """the shapes of test_stem_conv_pool_fused against float64, in the folded form and with the scale in the epilogue (out_scale)"""
    K = _k()
    xu, x, w, bn, xin = _stem_operands(K, shape, in_u8, 1, 841)
    a, b = (xin[:split].contiguous(), xin[split:].contiguous()) if split else (xin, None)
    wp2, bias = K.pack_stem(w.to(DEV), 1, bn=tuple(t.to(DEV) for t in bn))
    wk2 = B.stem_unpack(wp2)
    _check_folded_pack(w, bn, wk2, bias, 1)
    y64, mag, _, _ = B.conv_fwd(x, wk2, 2, 3, bias=bias.cpu(), relu=True)
    want, bnd = B.maxpool_plain_ref(y64, B.bound(y64, mag, 147, 1))
    B.check(K.stem_conv_pool(a, wp2, bias, x2=b), want, bnd, "stem + pool, folded", "stem_conv_pool")
    if shape[0] > 5:          # (the 260-image case is about workgroups walking into a second image: one form is enough)
        return
    wpu, bias_u, scale_u = K.pack_stem(w.to(DEV), 1, bn=tuple(t.to(DEV) for t in bn), unfold=True)
    y64, mag, _, _ = B.conv_fwd(x, B.stem_unpack(wpu), 2, 3, out_scale=scale_u.cpu(), bias=bias_u.cpu(), relu=True)
    want, bnd = B.maxpool_plain_ref(y64, B.bound(y64, mag, 147, 1))
    B.check(K.stem_conv_pool(a, wpu, bias_u, x2=b, out_scale=scale_u), want, bnd, "stem + pool, out_scale", "stem_conv_pool")


@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_optimizer_step_f64(kind):
    """one step of Adam / Nesterov SGD from a non-zero fp32 state against float64: p, s1, s2 per element; the shadow-weight packs the
    update writes are the packs of the updated p, bit for bit"""
    from ssl_cr_histo_amd import _lib as L
    K = _k()
    shapes = [(64, 3, 7, 7), (128, 64, 3, 3), (130,), (10, 768)]
    ps = [rnd(850 + i, s, 0.1) for i, s in enumerate(shapes)]
    gs = [rnd(860 + i, s) for i, s in enumerate(shapes)]
    m0 = [rnd(870 + i, s, 0.3) for i, s in enumerate(shapes)]
    v0 = [rnd(880 + i, s).abs() * 0.5 + 0.01 for i, s in enumerate(shapes)]
    dev_p, s1, s2 = ([t.to(DEV).contiguous() for t in ts] for ts in (ps, m0, v0))
    sh_f = torch.zeros((128, 3, 3, 64), dtype=torch.bfloat16, device=DEV)
    sh_d = torch.zeros((64, 3, 3, 128), dtype=torch.bfloat16, device=DEV)
    descs = (L.TensorDesc * len(shapes))()
    keep, g_param_layout = [], []
    for i, (p, g) in enumerate(zip(dev_p, gs)):
        if g.dim() == 4 and i != 0:                           # engine grad layout KRSC against the parameter's KCRS
            gd, (Kk, Cc, RS) = g.permute(0, 2, 3, 1).contiguous().to(DEV), (g.shape[0], g.shape[1], g.shape[2] * g.shape[3])
        else:
            gd, (Kk, Cc, RS) = g.to(DEV), (0, 0, 0)
        keep.append(gd)
        descs[i] = L.TensorDesc(L.ptr(p), L.ptr(gd), L.ptr(s1[i]), L.ptr(s2[i]), p.numel(), Kk, Cc, RS)
        if i == 1:
            descs[i].w_fwd, descs[i].w_dgrad, descs[i].pack_dtype, descs[i].dgrad_flip = L.ptr(sh_f), L.ptr(sh_d), 1, 1
    dd = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).to(DEV)
    step = 4
    hp = dict(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, wd=1e-4, momentum=0.9, bc1=1 - 0.9 ** step, bc2=1 - 0.999 ** step, first_step=0)
    o = L.OptDesc(0 if kind == "adam" else 1, hp["lr"], hp["beta1"], hp["beta2"], hp["eps"], hp["wd"], hp["momentum"], hp["bc1"], hp["bc2"], 0, 1.0)
    L.check(L.lib().sslcr_optimizer_step(L.ptr(dd), len(shapes), max(p.numel() for p in dev_p), o, L.stream_ptr()))
    torch.cuda.synchronize()
    for i in range(len(shapes)):
        ref = B.optimizer_ref(0 if kind == "adam" else 1, ps[i], gs[i], m0[i], v0[i], **hp)
        for name, got in (("p", dev_p[i]), ("s1", s1[i])) + ((("s2", s2[i]),) if kind == "adam" else ()):
            B.check(got.flatten(), ref[name][0].flatten(), ref[name][1].flatten(), f"{kind} tensor {i} {name}", "optimizer_kernel", dims="i")
        if kind == "sgd":
            assert torch.equal(s2[i].cpu(), v0[i]), "SGD leaves s2 alone"
    wf1, wd1, _ = K.pack_conv(dev_p[1], 1, fwd=True, dgrad=True, dgrad_flip=True)
    assert torch.equal(sh_f, wf1) and torch.equal(sh_d, wd1), "shadow weights written by the update != pack of the updated parameter"
