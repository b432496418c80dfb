"""Operands and float64 reference of the fp8 conv tests (tests/fp8_cases.py), shared by the GPU tests and the CPU self-test.

The inputs are the same for every row, built to make an indexing or quantisation slip visible element by element:
  activations  bf16, rnd * 1.5 + 0.3; the image-corner pixel (0, 0, 0) holds 1000 on channels 0 .. 7 (saturates at 448); the interior
               pixel (N - 1, H / 2, W / 2) is all zeros; channel SUB is scaled by 2^-9 (e4m3 subnormals at x_scale = 1).
  weights      output channel k multiplied by 2^((5 k mod 13) - 6): neighbouring channels differ in w_dequant (13 values over 2^12);
               channel 3 is an all-zero filter (the scale = 1 arm of pack_fp8_kernel).
  in_scale     _channel_scale: both signs, x 1e3 on channel 0 and x 1e-3 on channel 1; in_shift random; bias _channel_scale; residual bf16.
"""
import math

import torch

import _f64 as B
from test_kernels_gpu import _channel_scale, rnd

SUB = 9         # the activation channel in the e4m3 subnormal range


def flags_of(spec):
    return set(spec.split())


def batch(shape, cus):
    """the row's shape with N resolved for a part with `cus` compute units (fp8_cases.WALK_N)"""
    from fp8_cases import WALK_N
    if shape[0] is not None:
        return tuple(shape)
    div, add, mul = WALK_N[tuple(shape[1:])]
    return (mul * (-(-cus // div) + add),) + tuple(shape[1:])


def tiles(shape):
    N, H, W, _, _ = shape
    return N * (H // 16) * (W // 16) if H % 16 == 0 else N // 4


def walkers(shape, cus):
    return max(1, cus // (shape[4] // 128))


def _bf(t):
    return t.to(torch.bfloat16).float()


def inputs(shape):
    """-> dict of CPU fp32 tensors: x (bf16 values), w [K, C, 3, 3], in_scale, in_shift, bias, residual (bf16 values)"""
    N, H, W, C, K = shape
    x = rnd(901, (N, H, W, C), 1.5) + 0.3
    x[..., SUB] *= 2.0 ** -9
    x[0, 0, 0, :8] = 1000.0
    x[N - 1, H // 2, W // 2, :] = 0.0
    w = rnd(902, (K, C, 3, 3), 0.04)
    k = torch.arange(K)
    w *= torch.pow(2.0, ((5 * k) % 13 - 6).float()).view(-1, 1, 1, 1)
    w[3] = 0.0
    return dict(x=_bf(x), w=w, in_scale=_channel_scale(903, C), in_shift=rnd(904, (C,)), bias=_channel_scale(905, K),
                residual=_bf(rnd(906, (N, H, W, K))))


_CACHE = {}     # (shape, transform, in_relu, xs) -> the dequantised accumulator; the entries of ONE shape at a time


def reference(shape, flags, xs, t=None):
    """-> dict: y / mag / bnd (the stored output, its magnitude and its per-element bound), acc / amag / pmax (what the statistics sum,
    with the alignment companion), n, amax = (hi, lo)"""
    f = flags_of(flags)
    t = inputs(shape) if t is None else t
    key = (tuple(shape), "in_scale" in f, "relu_in" in f, float(xs))
    if key not in _CACHE:
        for k in [k for k in _CACHE if k[0] != key[0]]:
            del _CACHE[k]
        xf = dict(in_scale=t["in_scale"], in_shift=t["in_shift"], in_relu="relu_in" in f) if "in_scale" in f else {}
        xq, amax = B.fp8_activations(t["x"], xs, **xf)
        wq, dq, _ = B.fp8_pack_ref(t["w"])
        _CACHE[key] = B.fp8_conv_ref(xq, wq, dq, xs) + (amax,)
    acc, amag, pmax, amax = _CACHE[key]
    y, mag = B.epilogue(acc, amag, bias=t["bias"] if "bias" in f else None, residual=t["residual"] if "residual" in f else None,
                        relu="relu" in f)
    n = 9 * shape[3]
    return dict(y=y, mag=mag, bnd=B.fp8_bound(y, mag, pmax, n), acc=acc, amag=amag, pmax=pmax, n=n, amax=amax)


# ---- CPU emulation of the kernel in fp32 torch (another summation order), with one fault at a time
def _q8(v, fault=None):
    """fp32 -> e4m3 values through torch's own conversion, or a faulty quantiser"""
    v = v.float().clamp(-448.0, 448.0)
    if fault in ("trunc", "ties_away"):
        a = v.double().abs()
        _, ex = torch.frexp(a)
        step = torch.ldexp(torch.ones_like(a), (ex - 1).clamp_min(-6) - 3)
        r = torch.floor(a / step) if fault == "trunc" else torch.floor(a / step + 0.5)
        return torch.copysign(r * step, v.double()).float()
    out = v.to(torch.float8_e4m3fn).float()
    if fault == "flush":
        out = torch.where(v.abs() < 2.0 ** -6, torch.zeros_like(out), out)
    return out


def emulate(shape, flags, xs, t, fault=None):
    """the fp8 conv in fp32 torch -> (y as bf16 values, stats rows [rows, 2, K] of the dequantised accumulator)"""
    import torch.nn.functional as F
    f = flags_of(flags)
    xs32 = torch.tensor(xs, dtype=torch.float32)
    x = t["x"]
    if "in_scale" in f:
        s = t["in_scale"] * (1.0 if fault == "scale_without_xs" else xs32)
        v = (x.double() * s.double() + (t["in_shift"] * xs32).double()).float()
    else:
        v = x * xs32
    v = v.clamp(0.0 if "relu_in" in f else -448.0, 448.0)
    xq = _q8(v, fault)
    wq, dq, _ = B.fp8_pack_ref(t["w"])
    wq = wq.float()

    def conv(a):
        return F.conv2d(a.permute(0, 3, 1, 2), wq.permute(0, 3, 1, 2), None, 1, 1).permute(0, 2, 3, 1).contiguous()
    acc = conv(xq)
    if fault == "halo_pixel":          # tile 0 staged without ONE pixel of its 18 x 18 halo: the nine outputs around it lose a tap
        xl = xq[:1].clone()
        xl[0, 1, 5] = 0.0
        acc[0, :16, :16] = conv(xl)[0, :16, :16]
    d = dq.float() / xs32
    if fault == "dequant_next":
        d = torch.roll(d, -1)
    acc = acc * d
    y = acc
    if "bias" in f:
        y = y + t["bias"]
    if "residual" in f:
        y = y + t["residual"]
    if "relu" in f:
        y = y.clamp_min(0.0)
    K = shape[4]
    rows = acc.reshape(-1, 64, K)
    return _bf(y), torch.stack([rows.sum(1), (rows * rows).sum(1)], 1)


def ulp32(v):
    """one fp32 ulp at |v| (float64)"""
    return math.ldexp(1.0, max(math.frexp(abs(v))[1] - 1, -126) - 23)
