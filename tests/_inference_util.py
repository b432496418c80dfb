"""Shared by tests/golden/make_test_golden.py (which drives the REFERENCE's test() functions) and the inference tests: the seeded
loaders of the ``*_test`` cases, a host restatement of the WSI tile cut, and the float64 bound of a softmax row."""
import numpy as np
import torch

from oracle import cases as C

from _f64 import EXPLOG_ULP, TINY, U

# b = 4, three batches, the last one ragged.  Kather at 96x96 (24/12/6/3 maps: the engine's fallback conv shapes), BreastPathQ at 64x64.
TEST_CASES = {"kather": dict(hw=96, sizes=(4, 4, 3), classes=9, head_scale=0.05, seed0=7100),
              "bpq": dict(hw=64, sizes=(4, 4, 3), classes=1, head_scale=1.0, seed0=7200)}
MARGIN = 2e-3          # reference top-2 score margin above which a prediction must be the reference's
MARGIN_SHARE = 0.5     # ... and the share of rows that must have it (the generator refuses a golden below it)


def kather_test_batches(seed0=None):
    """eval_Kather_SSL(_CR).test loader: (input u8 [n, 3, H, W], target int64 [n])"""
    c = TEST_CASES["kather"]
    seed0 = c["seed0"] if seed0 is None else seed0
    return [(C.u8(seed0 + i, (n, 3, c["hw"], c["hw"])), C.ints(seed0 + 50 + i, (n,), c["classes"])) for i, n in enumerate(c["sizes"])]


def bpq_test_batches(seed0=None):
    """eval_BreastPathQ_SSL(_CR).test loader: (input u8 [n, 3, H, W], targetA f32 [n], targetB f32 [n])"""
    c = TEST_CASES["bpq"]
    seed0 = c["seed0"] if seed0 is None else seed0
    return [(C.u8(seed0 + i, (n, 3, c["hw"], c["hw"])), C.f32(seed0 + 50 + i, (n,)), C.f32(seed0 + 80 + i, (n,))) for i, n in enumerate(c["sizes"])]


def scale_head(cls, scale):
    """the seeded random head saturates a softmax; shrink it so that the scores spread (as the cam_wsi_large case does)"""
    if scale != 1.0:
        with torch.no_grad():
            cls.classifier[0].weight.mul_(scale)
            cls.classifier[0].bias.mul_(scale)


def cut_tiles(region, xy, size, origin=(0, 0), fill=0):
    """numpy slicing of a `fill`-padded region: uint8 [N, 3, size, size] with tile n = region[top - oy :, left - ox :] (HWC -> CHW)"""
    RH, RW, _ = region.shape
    xy = np.asarray(xy, dtype=np.int64)
    left, top = xy[:, 0] - origin[0], xy[:, 1] - origin[1]
    # pad so that every tile that touches the region lies inside the padded array; tiles wholly outside are all `fill`
    out = np.full((len(xy), 3, size, size), fill, dtype=np.uint8)
    for n in range(len(xy)):
        y0, y1 = max(top[n], 0), min(top[n] + size, RH)
        x0, x1 = max(left[n], 0), min(left[n] + size, RW)
        if y0 < y1 and x0 < x1:
            out[n, :, y0 - top[n]:y1 - top[n], x0 - left[n]:x1 - left[n]] = region[y0:y1, x0:x1].transpose(2, 0, 1)
    return out


def softmax_rows_ref(l):
    """softmax(l, dim=1) -> (p64 [n, C], bound [n, C]): every column as tests/_f64.py:softmax_col_ref bounds its one -- expf(l_c - m) / s:
    the subtraction [rel. |d_c| u in the exponent], expf [X u], the sum of C terms [(C - 1) u plus the terms' own errors], the division [1]"""
    ld = l.double()
    d = ld - ld.amax(1, keepdim=True)
    ex = torch.exp(d)
    s = ex.sum(1, keepdim=True)
    p = ex / s
    rel_s = ((p * (d.abs() + EXPLOG_ULP)).sum(1, keepdim=True) + (ld.shape[1] - 1)) * U
    return p, p * ((d.abs() + EXPLOG_ULP + 1) * U + rel_s) + TINY
