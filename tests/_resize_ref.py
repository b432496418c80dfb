"""NumPy restatement of Pillow's 8-bit resample (Resample.c: precompute_coeffs, normalize_coeffs_8bpc, the horizontal and vertical
passes) -- the definition include/sslcr.h states for sslcr_resample_coeffs and csrc/resample.hip.  Python floats are C doubles and
``math`` calls the libm Pillow calls, so the coefficient arithmetic is Pillow's operation for operation; the passes are exact integers.
tests/test_resize_cpu.py holds this file EQUAL to the live Pillow, and the library's tables and kernels EQUAL to this file."""
import math

import numpy as np

PRECISION_BITS = 22
_C054, _C046 = float(np.float32(0.54)), float(np.float32(0.46))      # Resample.c spells 0.54f / 0.46f


def _box(x):
    return 1.0 if -0.5 < x <= 0.5 else 0.0


def _bilinear(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def _hamming(x):
    x = abs(x)
    if x == 0.0:
        return 1.0
    if x >= 1.0:
        return 0.0
    x = x * math.pi
    return math.sin(x) / x * (_C054 + _C046 * math.cos(x))


def _bicubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x):
    return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


FILTERS = {"box": (_box, 0.5), "bilinear": (_bilinear, 1.0), "hamming": (_hamming, 1.0), "bicubic": (_bicubic, 2.0),
           "lanczos": (_lanczos, 3.0)}


def coeffs(in_size, in0, in1, out_size, name):
    """-> (k int64 [out_size, ksize], bounds int64 [out_size, 2], sum|w| of the worst row) of one axis"""
    f, s = FILTERS[name]
    scale = filterscale = (in1 - in0) / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = s * filterscale
    ksize = 2 * int(math.ceil(support)) + 1
    ss = 1.0 / filterscale
    k = np.zeros((out_size, ksize), dtype=np.int64)
    bounds = np.zeros((out_size, 2), dtype=np.int64)
    worst = 0.0
    for xx in range(out_size):
        center = in0 + (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [f((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        worst = max(worst, sum(abs(v) for v in w))
        for x, v in enumerate(w):
            k[xx, x] = int(0.5 + v * (1 << PRECISION_BITS)) if v >= 0 else int(-0.5 + v * (1 << PRECISION_BITS))
        bounds[xx] = (xmin, xmax)
    return k, bounds, worst


def nearest_index(in_size, in0, in1, out_size):
    """Pillow's ImagingScaleAffine: the source position is walked, ``xo += scale``, and truncated"""
    scale = (in1 - in0) / out_size
    xo, idx = in0 + scale * 0.5, []
    for _ in range(out_size):
        idx.append(min(in_size - 1, int(xo)))
        xo += scale
    return np.array(idx, dtype=np.int64)


def nearest_index_closed_form(in_size, in0, in1, out_size):
    """``min(inSize - 1, floor(in0 + (xx + 0.5) * scale))``: what the walk is often taken for.  It is NOT Pillow's (512 -> 257)."""
    scale = (in1 - in0) / out_size
    return np.array([min(in_size - 1, int(math.floor(in0 + (xx + 0.5) * scale))) for xx in range(out_size)], dtype=np.int64)


def _pass(img, k, bounds, axis):
    """img int64 [H, W, C]; one pass along axis 1 (horizontal) or 0 (vertical) -> int64, rounded and clipped to 0..255"""
    if axis == 0:
        return _pass(img.transpose(1, 0, 2), k, bounds, 1).transpose(1, 0, 2)
    out = np.empty((img.shape[0], len(k), img.shape[2]), dtype=np.int64)
    for xx, (xmin, xmax) in enumerate(bounds):
        acc = np.tensordot(img[:, xmin:xmin + xmax, :], k[xx, :xmax], axes=([1], [0])) + (1 << (PRECISION_BITS - 1))
        out[:, xx, :] = np.clip(acc >> PRECISION_BITS, 0, 255)            # >> of a negative int64 is arithmetic
    return out


def needs_pass(in_size, in0, in1, out_size):
    return not (out_size == in_size and in0 == 0 and in1 == out_size)


def resize(img, size, name, box=None):
    """``PIL.Image.fromarray(img).resize(size, name, box)`` for a uint8 [H, W] or [H, W, 3] array; size = (ow, oh)"""
    a = np.asarray(img)
    assert a.dtype == np.uint8 and a.ndim in (2, 3)
    x = a.astype(np.int64).reshape(a.shape[0], a.shape[1], -1)
    H, W = x.shape[:2]
    ow, oh = size
    x0, y0, x1, y1 = (0.0, 0.0, float(W), float(H)) if box is None else [float(np.float32(v)) for v in box]
    if name == "nearest":
        assert box is None, "NEAREST with a box is Pillow's fixed-point walk: not restated"
        x = x[nearest_index(H, y0, y1, oh)][:, nearest_index(W, x0, x1, ow)]
    else:
        if needs_pass(W, x0, x1, ow):                                       # horizontal FIRST, rounded to bytes
            k, b, _ = coeffs(W, x0, x1, ow, name)
            x = _pass(x, k, b, 1)
        if needs_pass(H, y0, y1, oh):
            k, b, _ = coeffs(H, y0, y1, oh, name)
            x = _pass(x, k, b, 0)
    return x.astype(np.uint8).reshape((oh, ow) + a.shape[2:])
