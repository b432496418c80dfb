"""CPU self-test of the float64 per-element bounds (tests/_f64.py) that the per-kernel GPU tests apply.

A torch emulation of what a bf16 conv kernel computes -- bf16 operands, fp32 accumulation, the fp32 epilogue
y = relu(fmaf(acc, out_scale, bias) + residual), RNE to bf16 -- must pass the bound, and every fault below must fail it.  The five
precision faults are ones the per-kernel suite's close() (max|got - want| <= tol * max|want| against the fp32 oracle) accepts: the
written reason close() alone is not enough.  The indexing faults fail both checks."""
import pytest
import torch
import torch.nn.functional as F

import _f64 as B
from oracle import kernels_ref as R
from test_kernels_gpu import TOL, close, q, rnd

PRECISION = ["trunc", "bias_bf16", "scale_bf16", "acc_bf16", "channel"]
INDEXING = ["halo_row", "chunk", "neighbour"]
SHAPES = [(2, 16, 16, 64, 64, True), (2, 8, 8, 512, 128, False)]        # N, H, W, C, K, residual: one channel slab / eight


def _conv32(x, w):
    return F.conv2d(x.permute(0, 3, 1, 2), w.permute(0, 3, 1, 2), None, 1, 1).permute(0, 2, 3, 1).contiguous()


def _rne(t):
    return t.float().to(torch.bfloat16).float()


def _trunc(t):
    return (t.float().contiguous().view(torch.int32) & -65536).view(torch.float32)


def _fmaf(a, b, c):
    # one rounding of a * b + c to fp32 (a * b is exact in float64; the float64 sum is rounded once more only below 2^-53)
    return (a.double() * b.double() + c.double()).float()


def emulate(x, w, scale, bias, res, fault=None):
    """the kernel's arithmetic, or the arithmetic with one fault"""
    wf = w.clone()
    if fault == "chunk":
        wf[:, 1, 1, 16:32] = 0.0                 # the centre tap loses one 16-channel chunk
    acc = _conv32(x, wf)
    if fault == "halo_row":
        h = x.shape[1] // 2
        xl = x.clone()
        xl[:, h] = 0.0                           # output row h - 1 (a tile's last) without input row h (its halo row)
        acc[:, h - 1] = _conv32(xl, wf)[:, h - 1]
    if fault == "acc_bf16":
        acc = _rne(acc)                          # double rounding: the accumulator to bf16 ahead of the epilogue
    s = _rne(scale) if fault == "scale_bf16" else scale
    b = _rne(bias) if fault == "bias_bf16" else bias
    v = _fmaf(acc, s, b)
    if res is not None:
        v = v + res
    v = v.clamp_min(0.0)
    if fault == "channel":
        v[..., 5] *= 1.0 + 2.0 ** -7             # one output channel off by a factor
    y = _trunc(v) if fault == "trunc" else _rne(v)
    if fault == "neighbour":
        y[:, 3, 4] = y[:, 3, 5]                  # one pixel written from its right-hand neighbour
    return y, acc


def operands(shape, seed=11):
    N, H, W, C, K, with_res = shape
    x = q(rnd(seed, (N, H, W, C)), 1)
    w = q(rnd(seed + 1, (K, 3, 3, C), 0.05), 1)
    scale = rnd(seed + 2, (K,)).abs() + 0.25
    scale[::3] *= -1.0
    bias = rnd(seed + 3, (K,))
    res = q(rnd(seed + 4, (N, H, W, K)), 1) if with_res else None
    return x, w, scale, bias, res


def reference(x, w, scale, bias, res):
    y64, mag, acc64, amag = B.conv_fwd(x, w, 1, 1, out_scale=scale, bias=bias, residual=res, relu=True)
    n = 9 * x.shape[-1]
    return y64, B.bound(y64, mag, n, 1), acc64, amag, n


@pytest.mark.parametrize("shape", SHAPES)
def test_correct_result_passes(shape):
    x, w, scale, bias, res = operands(shape)
    y64, bnd, acc64, amag, n = reference(x, w, scale, bias, res)
    y, acc = emulate(x, w, scale, bias, res)
    B.check(y, y64, bnd, "emulated bf16 conv")
    # statistics of the fp32 accumulator: fp32 partial sums of 64 pixels each (a wave's rows), summed in double by the check
    K = acc.shape[-1]
    rows = acc.reshape(-1, 64, K)
    B.check_stats(torch.stack([rows.sum(1), (rows * rows).sum(1)], 1), acc64, amag, n, "emulated statistics")


@pytest.mark.parametrize("fault", PRECISION + INDEXING)
@pytest.mark.parametrize("shape", SHAPES)
def test_fault_fails_the_bound(shape, fault):
    x, w, scale, bias, res = operands(shape)
    y64, bnd, _, _, _ = reference(x, w, scale, bias, res)
    y, _ = emulate(x, w, scale, bias, res, fault)
    with pytest.raises(AssertionError, match="worst err/bound"):
        B.check(y, y64, bnd, fault)


@pytest.mark.parametrize("fault", PRECISION)
@pytest.mark.parametrize("shape", SHAPES)
def test_close_accepts_the_precision_faults(shape, fault):
    x, w, scale, bias, res = operands(shape)
    y, _ = emulate(x, w, scale, bias, res, fault)
    close(y, R.conv_fwd(x, w, 1, 1, bias=bias, residual=res, relu=True, out_scale=scale), TOL[1], fault)


@pytest.mark.parametrize("fault", INDEXING)
@pytest.mark.parametrize("shape", SHAPES)
def test_close_rejects_the_indexing_faults(shape, fault):
    x, w, scale, bias, res = operands(shape)
    y, _ = emulate(x, w, scale, bias, res, fault)
    with pytest.raises(AssertionError):
        close(y, R.conv_fwd(x, w, 1, 1, bias=bias, residual=res, relu=True, out_scale=scale), TOL[1], fault)


def test_wgrad_partial_slab_rounded_to_bf16_fails():
    """a weight gradient folded from fp32 partial slabs (one per pixel split) into a non-zero dW passes; the same fold with one
    slab rounded to bf16 fails"""
    N, H, W, C, K = 4, 16, 16, 64, 128
    x, dy = q(rnd(31, (N, H, W, C)), 1), q(rnd(32, (N, H, W, K)), 1)
    base = rnd(33, (K, 3, 3, C))
    want, mag = B.conv_wgrad(x, dy, (K, 3, 3, C), 1, 1, base=base)
    bnd = B.bound(want, mag, N * H * W, 0)
    slabs = [torch.nn.grad.conv2d_weight(x[i:i + 1].permute(0, 3, 1, 2), (K, C, 3, 3), dy[i:i + 1].permute(0, 3, 1, 2), 1, 1)
             .permute(0, 2, 3, 1) for i in range(N)]

    def fold(parts):
        out = base.clone()
        for p in parts:
            out = out + p
        return out
    B.check(fold(slabs), want, bnd, "wgrad from fp32 slabs", dims="krsc")
    slabs[2] = _rne(slabs[2])
    with pytest.raises(AssertionError, match="worst err/bound"):
        B.check(fold(slabs), want, bnd, "wgrad with a slab rounded to bf16", dims="krsc")
