"""NumPy restatement of the twelve Pillow ops of the RSP v2 RandAugment pool (Pretraining_v2/models/randaugment.py:38-190) and of
the draw order of ``RandAugment.__call__`` (:195-213).  Test infrastructure: it imports neither the reference nor Pillow.

Every function takes an [H, W, 3] uint8 array and returns one.  The arithmetic is Pillow's, operation for operation (float32 blend
and 3x3 filter, float64 LUTs and bicubic, integer fixed-point walk); tests/test_randaug_v2_cpu.py holds it to the goldens and to
the live Pillow byte for byte, tests/test_randaug_v2_gpu.py holds the HIP kernels to it.
"""
import math

import numpy as np

POOL = ("identity", "contrast", "brightness", "sharpness", "rotate", "translate_x", "translate_y", "shear_x", "shear_y",
        "hed", "hsv", "autocontrast", "color", "equalize")          # augment_pool() order (:176-190); random.sample depends on it
SIGNED = ("rotate", "translate_x", "translate_y", "shear_x", "shear_y")     # ops that call _randomly_negate_tensor (:24-34)
HOST = ("hed", "hsv")


# ------------------------------------------------------------------------------------------------ draws
def plan_image(rng, np_rng, n, m):
    """the draws of ONE ``RandAugment(n, m)(img)`` call: -> [(name, val, sign)], sign 1 keeps the level, 0 negates, None = no draw.
    Valid as long as no host op (hed / hsv, which draw from numpy while they run) is sampled."""
    out = []
    for name in rng.sample(POOL, k=n):
        val = float(np_rng.uniform(1, m))
        out.append((name, val, rng.choice([1, 0]) if name in SIGNED else None))
    return out


def enhance_factor(val):
    return np.float32(val / 10 * 1.8 + 0.1)


def signed_level(name, val, sign):
    lv = {"rotate": val / 10 * 30., "translate_x": val / 10 * float(10), "translate_y": val / 10 * float(10),
          "shear_x": val / 10 * 0.3, "shear_y": val / 10 * 0.3}[name]
    return lv if sign == 1 else -lv


# ------------------------------------------------------------------------------------------------ point ops
def luma(img):
    """Image.convert("L"): ITU-R 601-2 in 16.16 fixed point"""
    r, g, b = (img[..., c].astype(np.int64) for c in range(3))
    return ((19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16).astype(np.uint8)


def blend(deg, img, f):
    """Image.blend(deg, img, f): float32 product, then float32 sum, clipped and truncated"""
    f = np.float32(f)
    d32 = deg.astype(np.float32)
    t = d32 + f * (img.astype(np.int32) - deg.astype(np.int32)).astype(np.float32)
    assert t.dtype == np.float32
    return np.where(t <= 0, 0, np.where(t >= 255, 255, np.trunc(t))).astype(np.uint8)


def brightness(img, f):
    return blend(np.zeros_like(img), img, f)


def color(img, f):
    return blend(np.repeat(luma(img)[..., None], 3, axis=2), img, f)


def contrast_mean(img):
    return int(int(luma(img).astype(np.int64).sum()) / (img.shape[0] * img.shape[1]) + 0.5)


def contrast(img, f):
    return blend(np.full_like(img, contrast_mean(img)), img, f)


def smooth(img):
    """ImageFilter.SMOOTH: 3x3 float32 kernel, one-pixel border copied"""
    k = np.array([1, 1, 1, 1, 5, 1, 1, 1, 1], dtype=np.float32) / np.float32(13)
    H, W = img.shape[:2]
    out = img.copy()
    if H < 3 or W < 3:
        return out
    v = img.astype(np.float32)
    acc = np.full((H - 2, W - 2, 3), 0.5, dtype=np.float32)
    for j, rows in enumerate((slice(2, H), slice(1, H - 1), slice(0, H - 2))):      # row y+1, then y, then y-1
        r = v[rows]
        acc = acc + ((r[:, 0:W - 2] * k[3 * j] + r[:, 1:W - 1] * k[3 * j + 1]) + r[:, 2:W] * k[3 * j + 2])
    assert acc.dtype == np.float32
    out[1:H - 1, 1:W - 1] = np.where(acc <= 0, 0, np.where(acc >= 255, 255, np.trunc(acc))).astype(np.uint8)
    return out


def sharpness(img, f):
    return blend(smooth(img), img, f)


def autocontrast_lut(h):
    """ImageOps.autocontrast, cutoff 0, for one channel's 256-bin histogram"""
    nz = np.nonzero(h)[0]
    lut = np.arange(256)
    if len(nz) == 0 or nz[-1] <= nz[0]:
        return lut.astype(np.uint8)
    lo, hi = int(nz[0]), int(nz[-1])
    scale = 255.0 / (hi - lo)
    offset = -lo * scale
    return np.array([min(max(int(i * scale + offset), 0), 255) for i in range(256)], dtype=np.uint8)


def equalize_lut(h):
    """ImageOps.equalize for one channel's 256-bin histogram"""
    histo = [int(x) for x in h if x]
    ident = np.arange(256, dtype=np.uint8)
    if len(histo) <= 1:
        return ident
    step = (sum(histo) - histo[-1]) // 255
    if not step:
        return ident
    lut, n = [], step // 2
    for i in range(256):
        lut.append(min(n // step, 255))
        n += int(h[i])
    return np.array(lut, dtype=np.uint8)


def _per_channel_lut(img, fn):
    out = np.empty_like(img)
    for c in range(3):
        out[..., c] = fn(np.bincount(img[..., c].reshape(-1), minlength=256))[img[..., c]]
    return out


def autocontrast(img):
    return _per_channel_lut(img, autocontrast_lut)


def equalize(img):
    return _per_channel_lut(img, equalize_lut)


# ------------------------------------------------------------------------------------------------ geometry
def rotate_matrix(deg, W, H):
    """Image.rotate(deg) -> the six floats handed to the affine transform"""
    a = -math.radians(deg % 360.0)
    m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]
    cx, cy = W / 2, H / 2
    m[2] = m[0] * (-cx) + m[1] * (-cy) + m[2] + cx
    m[5] = m[3] * (-cx) + m[4] * (-cy) + m[5] + cy
    return m


def fixed_coefficients(m):
    """Pillow's affine_fixed: 16.16 integers of the six floats, the half-pixel centre folded into a2 / a5"""
    def fix(v):
        return int(math.floor(v * 65536.0 + 0.5))
    return [fix(m[0]), fix(m[1]), fix(m[2] + m[0] * 0.5 + m[1] * 0.5), fix(m[3]), fix(m[4]), fix(m[5] + m[3] * 0.5 + m[4] * 0.5)]


def fixed_ok(m, W, H):
    """Pillow takes the fixed-point walk only when both corners stay inside 16 bits"""
    def ok(x, y):
        return abs(x * m[0] + y * m[1] + m[2]) < 32768.0 and abs(x * m[3] + y * m[4] + m[5]) < 32768.0
    return ok(0, 0) and ok(W, H)


def rotate(img, deg):
    H, W = img.shape[:2]
    a0, a1, a2, a3, a4, a5 = fixed_coefficients(rotate_matrix(deg, W, H))
    x, y = np.meshgrid(np.arange(W, dtype=np.int64), np.arange(H, dtype=np.int64))
    xin, yin = (a2 + a0 * x + a1 * y) >> 16, (a5 + a3 * x + a4 * y) >> 16
    ok = (xin >= 0) & (xin < W) & (yin >= 0) & (yin < H)
    out = np.zeros_like(img)
    out[ok] = img[yin[ok], xin[ok]]
    return out


def translate_table(p, n):
    """Pillow's scale path: the source index per output index, -1 = outside; the coordinate grows by repeated addition"""
    o = np.add.accumulate(np.concatenate(([p + 0.5], np.ones(n - 1))))
    idx = np.where(o < 0, -1, np.trunc(o)).astype(np.int64)
    return np.where(idx >= n, -1, idx)


def translate(img, px, py):
    H, W = img.shape[:2]
    xt, yt = translate_table(px, W), translate_table(py, H)
    out = np.zeros_like(img)
    ok = (yt >= 0)[:, None] & (xt >= 0)[None, :]
    src = img[np.maximum(yt, 0)[:, None], np.maximum(xt, 0)[None, :]]
    out[ok] = src[ok]
    return out


def _cubic(v1, v2, v3, v4, d):
    p1 = v2
    p2 = -v1 + v3
    p3 = 2 * (v1 - v2) + v3 - v4
    p4 = -v1 + v2 - v3 + v4
    return p1 + d * (p2 + d * (p3 + d * p4))


def affine_bicubic(img, a):
    """Image.transform(size, AFFINE, a, BICUBIC) in float64"""
    H, W = img.shape[:2]
    x, y = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    xin = a[0] * (x + 0.5) + a[1] * (y + 0.5) + a[2]
    yin = a[3] * (x + 0.5) + a[4] * (y + 0.5) + a[5]
    inside = ~((xin < 0) | (xin >= W) | (yin < 0) | (yin >= H))
    xin, yin = xin - 0.5, yin - 0.5
    x0, y0 = np.floor(xin), np.floor(yin)
    dx, dy = xin - x0, yin - y0
    xs = [np.clip(x0.astype(np.int64) + k, 0, W - 1) for k in (-1, 0, 1, 2)]
    ys = [np.clip(y0.astype(np.int64) + k, 0, H - 1) for k in (-1, 0, 1, 2)]
    v = img.astype(np.float64)
    rows = [_cubic(*(v[yk, xk] for xk in xs), dx[..., None]) for yk in ys]
    r = _cubic(*rows, dy[..., None])
    out = np.where(r <= 0, 0, np.where(r >= 255, 255, np.trunc(r))).astype(np.uint8)
    out[~inside] = 0
    return out


def shear_x(img, lv):
    return affine_bicubic(img, (1, lv, 0, 0, 1, 0))


def shear_y(img, lv):
    return affine_bicubic(img, (1, 0, 0, lv, 1, 0))


# ------------------------------------------------------------------------------------------------ the pool
def apply_op(img, name, val, sign=None):
    """what the reference's op function ``name(img, val)`` returns when its _randomly_negate_tensor draw is ``sign``"""
    if name == "identity":
        return img
    if name in ("contrast", "brightness", "sharpness", "color"):
        return {"contrast": contrast, "brightness": brightness, "sharpness": sharpness, "color": color}[name](img, enhance_factor(val))
    if name == "autocontrast":
        return autocontrast(img)
    if name == "equalize":
        return equalize(img)
    lv = signed_level(name, val, sign)
    if name == "rotate":
        return rotate(img, lv)
    if name == "translate_x":
        return translate(img, lv, 0.0)
    if name == "translate_y":
        return translate(img, 0.0, lv)
    if name == "shear_x":
        return shear_x(img, lv)
    if name == "shear_y":
        return shear_y(img, lv)
    raise NotImplementedError(name)


def randaugment(img, rng, np_rng, n, m):
    """one ``RandAugment(n, m)(img)`` call"""
    for name, val, sign in plan_image(rng, np_rng, n, m):
        img = apply_op(img, name, val, sign)
    return img
