"""Device-side weak augmentation ("next" row f1): the reference's ``TransformFix.weak`` -- ``RandomHorizontalFlip()`` then
``RandomCrop(size=image_size)`` (dataset.py:663-677) -- applied to a uint8 batch that already sits in HBM.

The random draws are made on the host in the order torchvision makes them for ONE sample (``torch.rand(1) < p`` for the
flip, then ``torch.randint(0, h - th + 1)`` and ``torch.randint(0, w - tw + 1)`` for the crop), sample after sample, so a
seeded run reproduces what the CPU transform would have produced sample by sample; the HIP kernel is the deterministic gather.
The output is the NCHW uint8 batch the stem kernel ingests directly.
"""
import torch

from . import _lib as L


def weak_params(n, src_hw, size, generator=None, p=0.5):
    """-> int32 [n, 3] (flip, top, left), drawn like n successive calls of TransformFix.weak."""
    sh, sw = src_hw
    th, tw = (size, size) if isinstance(size, int) else size
    if th > sh or tw > sw:
        raise ValueError(f"Required crop size {(th, tw)} is larger than input image size {(sh, sw)}")
    out = torch.empty((n, 3), dtype=torch.int32)
    for k in range(n):
        flip = bool(torch.rand(1, generator=generator) < p)                         # RandomHorizontalFlip.forward
        if sh == th and sw == tw:                                                   # RandomCrop.get_params
            top = left = 0
        else:
            top = int(torch.randint(0, sh - th + 1, size=(1,), generator=generator).item())
            left = int(torch.randint(0, sw - tw + 1, size=(1,), generator=generator).item())
        out[k, 0], out[k, 1], out[k, 2] = int(flip), top, left
    return out


def weak_augment(src_u8, params, size, *, src_hwc=False, out=None):
    """src uint8 [N,3,SH,SW] (or [N,SH,SW,3] with src_hwc) on the GPU, params int32 [N,3] -> uint8 [N,3,size,size]."""
    if not src_u8.is_cuda or src_u8.dtype != torch.uint8 or not src_u8.is_contiguous():
        raise ValueError("weak_augment: contiguous uint8 CUDA tensor expected")
    n = src_u8.shape[0]
    sh, sw = (src_u8.shape[1], src_u8.shape[2]) if src_hwc else (src_u8.shape[2], src_u8.shape[3])
    th, tw = (size, size) if isinstance(size, int) else size
    prm = params.to(device=src_u8.device, dtype=torch.int32).contiguous()
    if prm.shape != (n, 3):
        raise ValueError("params must be [N, 3]")
    dst = out if out is not None else torch.empty((n, 3, th, tw), dtype=torch.uint8, device=src_u8.device)
    d = L.WeakAugDesc(L.ptr(src_u8), L.ptr(dst), L.ptr(prm), n, sh, sw, th, tw, int(src_hwc))
    L.check(L.lib().sslcr_weak_augment(d, L.stream_ptr()))
    return dst


class TransformFixWeak:
    """Batched, device-side counterpart of ``TransformFix(image_size, N).weak`` (dataset.py:669)."""

    def __init__(self, image_size, generator=None):
        self.image_size, self.generator = image_size, generator

    def __call__(self, batch_u8, src_hwc=False):
        n = batch_u8.shape[0]
        hw = (batch_u8.shape[1], batch_u8.shape[2]) if src_hwc else (batch_u8.shape[2], batch_u8.shape[3])
        return weak_augment(batch_u8, weak_params(n, hw, self.image_size, self.generator), self.image_size, src_hwc=src_hwc)


def fix_params(n, src_hw, size, generator=None, p=0.5):
    """The torch-RNG draws of n successive ``TransformFix.__call__`` (dataset.py:663-677): per sample the weak branch's
    (flip, top, left) and then the strong branch's (flip, top, left) -- ``RandAugment`` draws from Python's ``random`` and numpy
    (models/randaugment.py:53,133-135), so it does not move the torch stream.  -> (weak int32 [n,3], strong int32 [n,3])."""
    weak = torch.empty((n, 3), dtype=torch.int32)
    strong = torch.empty((n, 3), dtype=torch.int32)
    for k in range(n):
        weak[k] = weak_params(1, src_hw, size, generator, p)[0]
        strong[k] = weak_params(1, src_hw, size, generator, p)[0]
    return weak, strong


class TransformFixGeometric:
    """Batched, device-side counterpart of the DETERMINISTIC part of ``TransformFix(image_size, N)`` (row f4, first half): both
    branches' ``RandomHorizontalFlip`` + ``RandomCrop`` with the reference's per-sample draw order, as two launches of the
    gather kernel over the source batch in HBM.  -> (weak uint8 [N,3,S,S], strong_geometric uint8 [N,3,S,S]); the histology
    ``RandAugment`` ops of the strong branch (models/randaugment.py:51-144) remain a host-side stage on the second output."""

    def __init__(self, image_size, generator=None):
        self.image_size, self.generator = image_size, generator

    def __call__(self, batch_u8, src_hwc=False):
        n = batch_u8.shape[0]
        hw = (batch_u8.shape[1], batch_u8.shape[2]) if src_hwc else (batch_u8.shape[2], batch_u8.shape[3])
        pw, ps = fix_params(n, hw, self.image_size, self.generator)
        return (weak_augment(batch_u8, pw, self.image_size, src_hwc=src_hwc),
                weak_augment(batch_u8, ps, self.image_size, src_hwc=src_hwc))


# ------------------------------------------------------------------------------------------------ strong branch, colour ops (row f4)
# skimage.color's stain matrices (scikit-image 0.15.0, requirements.txt:369): Ruifrok & Johnston's rgb_from_hed and its inverse
_RGB_FROM_HED = ((0.65, 0.70, 0.29), (0.07, 0.99, 0.11), (0.27, 0.57, 0.78))


def _hed_matrices():
    import numpy as np
    m = np.array(_RGB_FROM_HED, dtype=np.float64)
    return np.linalg.inv(m).reshape(-1).tolist(), m.reshape(-1).tolist()      # hed_from_rgb = linalg.inv(rgb_from_hed), as skimage builds it


def colour_shifts(rng):
    """the draws of ONE ``Color(img, v)`` call (models/randaugment.py:81-84 -> :30-32) from a ``random.Random``-like ``rng``: three
    ``uniform(-0.035, 0.035)`` standard deviations, then ``normalvariate(0, std)`` for h, d, e.  -> (hmod, dmod, emod)"""
    hs, ds, es = rng.uniform(-0.035, 0.035), rng.uniform(-0.035, 0.035), rng.uniform(-0.035, 0.035)
    return rng.normalvariate(0, hs), rng.normalvariate(0, ds), rng.normalvariate(0, es)


def _apply_mask(apply, n, device):
    if apply is None:
        return None
    a = torch.as_tensor(apply).to(device=device, dtype=torch.uint8).contiguous()
    if a.shape != (n,):
        raise ValueError("apply must be [N]")
    return a


def hed_colour_augment(batch_u8, shifts, apply=None, *, hwc=False, out=None):
    """``colour_augmentation`` (models/randaugment.py:17-48) on a uint8 batch in HBM: [N,3,H,W] (or [N,H,W,3] with hwc);
    shifts [N,3] = (hmod, dmod, emod) per image; apply [N] bool or None.  float64 arithmetic, skimage 0.15.0 order."""
    if not batch_u8.is_cuda or batch_u8.dtype != torch.uint8 or not batch_u8.is_contiguous() or batch_u8.dim() != 4:
        raise ValueError("hed_colour_augment: contiguous uint8 CUDA batch [N,3,H,W] or [N,H,W,3] expected")
    n = batch_u8.shape[0]
    h, w = (batch_u8.shape[1], batch_u8.shape[2]) if hwc else (batch_u8.shape[2], batch_u8.shape[3])
    if (batch_u8.shape[3] if hwc else batch_u8.shape[1]) != 3:
        raise ValueError("three colour channels expected")
    sh = torch.as_tensor(shifts, dtype=torch.float64).to(batch_u8.device).contiguous()
    if sh.shape != (n, 3):
        raise ValueError("shifts must be [N, 3]")
    ap = _apply_mask(apply, n, batch_u8.device)
    dst = out if out is not None else torch.empty_like(batch_u8)
    inv, fwd = _hed_matrices()
    d = L.ColourAugDesc(L.ptr(batch_u8), L.ptr(dst), L.ptr(sh), L.ptr(ap), (L.f64 * 9)(*inv), (L.f64 * 9)(*fwd), n, h, w, int(hwc))
    L.check(L.lib().sslcr_hed_colour_augment(d, L.stream_ptr()))
    return dst


def brightness_contrast_params(rng, brightness_limit=0.2, contrast_limit=0.2, p=0.5):
    """the draws of ONE ``Compose([RandomBrightnessContrast(...)])(image=img)`` call of albumentations 0.1.8 (what ``Brightness`` /
    ``Contrast`` of models/randaugment.py:93-103 build): Compose's ``random.random() < 1``, the transform's ``random.random() < p``,
    and only then alpha = 1 + uniform(contrast), beta = uniform(brightness).  -> (applied, alpha, beta)"""
    rng.random()
    if not rng.random() < p:
        return False, 1.0, 0.0
    # to_tuple(limit) of 0.1.8 is (-limit, limit) UNSORTED and get_params draws random.uniform(limit[0], limit[1]) = a + (b - a) r:
    # RandAugment's val = v / 30 * 0.4 - 0.2 is negative for v < 15, and the draw is then |val| (1 - 2 r), not |val| (2 r - 1)
    alpha = 1.0 + rng.uniform(-contrast_limit, contrast_limit)
    beta = 0.0 + rng.uniform(-brightness_limit, brightness_limit)
    return True, alpha, beta


def brightness_contrast(batch_u8, alpha_beta, apply=None, *, out=None):
    """albumentations 0.1.8 ``brightness_contrast_adjust`` on a uint8 batch in HBM ([N,3,H,W] or [N,H,W,3]; the map does not care):
    clip(float32(img) * alpha + beta * mean(img), 0, max(img)).astype(uint8) with per-image mean / max.  alpha_beta [N,2]."""
    if not batch_u8.is_cuda or batch_u8.dtype != torch.uint8 or not batch_u8.is_contiguous() or batch_u8.dim() != 4:
        raise ValueError("brightness_contrast: contiguous uint8 CUDA batch expected")
    n = batch_u8.shape[0]
    ab = torch.as_tensor(alpha_beta, dtype=torch.float64).to(batch_u8.device).contiguous()
    if ab.shape != (n, 2):
        raise ValueError("alpha_beta must be [N, 2]")
    ap = _apply_mask(apply, n, batch_u8.device)
    dst = out if out is not None else torch.empty_like(batch_u8)
    stats = torch.empty((n, 2), dtype=torch.int64, device=batch_u8.device)
    pix = batch_u8.numel() // (3 * n)
    d = L.BrightnessContrastDesc(L.ptr(batch_u8), L.ptr(dst), L.ptr(ab), L.ptr(ap), L.ptr(stats), n, pix, 1)
    L.check(L.lib().sslcr_brightness_contrast(d, L.stream_ptr()))
    return dst


# The six OpenCV-style ops of the pool (models/randaugment.py:51-110): csrc/augment_v1.hip runs the arithmetic include/sslcr.h DEFINES
# for them, one op SLOT of a whole batch per call.  The host side below makes the draws and turns them into the integers and matrices
# the kernels read.  PARITY UNPINNED against OpenCV 3.4.2 / albumentations 0.1.8 / imgaug 0.4.0 (none is installed): the header is the
# definition, tests/_cv_ref.py restates it, and the draw order is the reference's.
V1_COPY, V1_BLUR, V1_HSV, V1_WARP, V1_RESIZE, V1_NOISE = range(6)
SRC_MARGIN = 20                          # Scale_Resize_Crop: Resize(S + 20), RandomCrop(S)
_WARP_TABLES = {}


def cv_warp_table():
    """the 1024 x 16 int16 weight table of the bicubic warp, as ``sslcr_cv_warp_table`` builds it (numpy, host)"""
    import numpy as np
    tab = np.empty((1024, 16), dtype=np.int16)
    L.check(L.lib().sslcr_cv_warp_table(tab.ctypes.data))
    return tab


def _warp_table_on(device):
    key = (device.type, device.index)
    if key not in _WARP_TABLES:
        _WARP_TABLES[key] = torch.from_numpy(cv_warp_table()).to(device)
    return _WARP_TABLES[key]


def rotation_matrix(hw, angle, scale=1.0, dx=0.0, dy=0.0):
    """``cv2.getRotationMatrix2D((W / 2, H / 2), angle, scale)`` with albumentations' shift added to the translations (dx, dy are
    fractions of W, H) -> the six floats of the FORWARD matrix"""
    import math
    h, w = hw
    cx, cy = w / 2, h / 2
    a = angle * math.pi / 180
    al, be = math.cos(a) * scale, math.sin(a) * scale
    return [al, be, (1 - al) * cx - be * cy + dx * w, -be, al, be * cx + (1 - al) * cy + dy * h]


def invert_affine(m):
    """the inverse ``cv2.warpAffine`` takes of its matrix, in its order of operations"""
    m = [float(v) for v in m]
    D = m[0] * m[4] - m[1] * m[3]
    D = 1.0 / D if D != 0 else 0.0
    a11, a22 = m[4] * D, m[0] * D
    m[0], m[1], m[3], m[4] = a11, m[1] * -D, m[3] * -D, a22
    b1 = -m[0] * m[2] - m[1] * m[5]
    b2 = -m[3] * m[2] - m[4] * m[5]
    m[2], m[5] = b1, b2
    return m


def v1_workspace(n, s, smax, device):
    """scratch of the RESIZE code for N images of S x S whose intermediate sizes stay <= smax -> (uint8 tensor, smax)"""
    nbytes = L.lib().sslcr_augv1_workspace_bytes(n, s, (smax + 0.5) / s)
    if not nbytes:
        raise ValueError(f"Scale_Resize_Crop: no workspace for {n} images of {s} with intermediate size {smax}")
    return torch.empty((nbytes,), dtype=torch.uint8, device=device), smax


def randaug_v1_slot(batch_u8, codes, *, iparam=None, dparam=None, apply=None, hwc=False, out_hwc=None, out=None, workspace=None):
    """One op slot on a uint8 batch in HBM: image n takes ``codes[n]`` (V1_*) with row n of iparam [N,4] ints and dparam [N,6] doubles
    (include/sslcr.h says what each code reads); apply [N] bool or None.  Everything is checked here, at plan time: a bad kernel size,
    a matrix that leaves OpenCV's 16-bit map range, a non-square Scale_Resize_Crop or an intermediate size < 1 is a ValueError.
    -> a new batch in the layout ``out_hwc`` asks for (default: the input's)."""
    import numpy as np
    h, w = _v2_batch(batch_u8, hwc, "randaug_v1_slot")
    n, dev = batch_u8.shape[0], batch_u8.device
    out_hwc = hwc if out_hwc is None else out_hwc
    codes = np.asarray(codes, dtype=np.int32)
    if codes.shape != (n,) or codes.min() < V1_COPY or codes.max() > V1_NOISE:
        raise ValueError("codes must be [N] op codes")
    ap = np.ones(n, bool) if apply is None else np.asarray([bool(a) for a in apply])
    if ap.shape != (n,):
        raise ValueError("apply must be [N]")
    codes = np.where(ap, codes, V1_COPY).astype(np.int32)
    ip = np.zeros((n, 4), np.int64) if iparam is None else np.asarray(iparam, dtype=np.int64).copy()
    dp = np.zeros((n, 6), np.float64) if dparam is None else np.asarray(dparam, dtype=np.float64).copy()
    if ip.shape != (n, 4) or dp.shape != (n, 6):
        raise ValueError("iparam must be [N, 4] and dparam [N, 6]")
    mask, smax = 0, 0
    for i, c in enumerate(codes.tolist()):
        mask |= 1 << c
        if c == V1_BLUR and ip[i, 0] not in (3, 5, 7):
            raise ValueError(f"blur: kernel size {ip[i, 0]} is not 3, 5 or 7")
        if c == V1_HSV and np.abs(ip[i, :3]).max() > 255:
            raise ValueError("hsv: shifts beyond +-255")
        if c == V1_WARP:
            m = dp[i]
            if not np.isfinite(m).all() or max(abs(m[0]) * (w - 1) + abs(m[1]) * (h - 1) + abs(m[2]),
                                               abs(m[3]) * (w - 1) + abs(m[4]) * (h - 1) + abs(m[5])) >= 32000:
                raise ValueError("warp: the matrix leaves OpenCV's 16-bit map range")
        if c == V1_RESIZE:
            if h != w:
                raise ValueError(f"Scale_Resize_Crop needs a square image, got {h}x{w}")
            if ip[i, 0] < 1 or not (0 <= ip[i, 1] <= SRC_MARGIN and 0 <= ip[i, 2] <= SRC_MARGIN):
                raise ValueError(f"Scale_Resize_Crop: intermediate size {ip[i, 0]} / origin ({ip[i, 1]}, {ip[i, 2]}) out of range")
            smax = max(smax, int(ip[i, 0]))
        if c == V1_NOISE and not (np.isfinite(dp[i, 0]) and dp[i, 0] >= 0):
            raise ValueError("noise: sigma must be finite and >= 0")
    work, wsmax = None, 0
    if smax:
        work, wsmax = workspace if workspace is not None else v1_workspace(n, h, smax, dev)
        if wsmax < smax or work.dtype != torch.uint8 or work.device != dev or work.numel() < L.lib().sslcr_augv1_workspace_bytes(n, h, (wsmax + 0.5) / h):
            raise ValueError("workspace: too small for this slot (v1_workspace)")
    shape = (n, h, w, 3) if out_hwc else (n, 3, h, w)
    dst = out if out is not None else torch.empty(shape, dtype=torch.uint8, device=dev)
    if tuple(dst.shape) != shape or dst.dtype != torch.uint8 or not dst.is_contiguous() or dst.device != dev:
        raise ValueError("out: contiguous uint8 batch of the output layout expected")
    t_op = torch.from_numpy(codes).to(dev)
    t_ip = torch.from_numpy((ip & 0xFFFFFFFF).astype(np.uint32).view(np.int32)).to(dev) if mask & ~1 else None
    t_dp = torch.from_numpy(dp).to(dev) if mask & (1 << V1_WARP | 1 << V1_NOISE) else None
    t_w = _warp_table_on(dev) if mask & (1 << V1_WARP) else None
    d = L.AugV1Desc(L.ptr(batch_u8), L.ptr(dst), L.ptr(t_op), None, L.ptr(t_ip), L.ptr(t_dp), L.ptr(t_w), L.ptr(work), wsmax, mask,
                    n, h, w, int(hwc), int(out_hwc))
    L.check(L.lib().sslcr_randaug_v1_slot(d, L.stream_ptr()))
    return dst


def _v1_rows(n, rows, width, name):
    import numpy as np
    a = np.asarray(rows, dtype=np.float64)
    if a.shape != ((n, width) if width else (n,)) or not np.isfinite(a).all():
        raise ValueError(f"{name} must be {[n, width] if width else [n]} finite numbers")
    return a


def cv_blur(batch_u8, ksize, apply=None, **kw):
    """``cv2.blur(img, (k, k))`` with k = ksize[n] in {3, 5, 7} where apply[n] (BORDER_REFLECT_101)."""
    import numpy as np
    n = batch_u8.shape[0]
    ip = np.zeros((n, 4), np.int64)
    ip[:, 0] = _v1_rows(n, ksize, 0, "ksize")
    return randaug_v1_slot(batch_u8, [V1_BLUR] * n, iparam=ip, apply=apply, **kw)


def cv_shift_hsv(batch_u8, shifts, apply=None, **kw):
    """albumentations' ``shift_hsv`` with shifts[n] = (hue, sat, val) draws where apply[n]: the planes move by rint(draw)."""
    import numpy as np
    n = batch_u8.shape[0]
    ip = np.zeros((n, 4), np.int64)
    ip[:, :3] = np.rint(_v1_rows(n, shifts, 3, "shifts"))
    return randaug_v1_slot(batch_u8, [V1_HSV] * n, iparam=ip, apply=apply, **kw)


def cv_warp_affine(batch_u8, matrices, flips=None, apply=None, **kw):
    """``cv2.warpAffine(img, M, (W, H), flags=INTER_CUBIC, borderMode=BORDER_REFLECT_101)`` with the FORWARD matrix M = matrices[n]
    (six floats, ``rotation_matrix``) where apply[n]; flips[n] = (horizontal, vertical) mirrors the source first."""
    import numpy as np
    n = batch_u8.shape[0]
    m = _v1_rows(n, matrices, 6, "matrices")
    ip = np.zeros((n, 4), np.int64)
    if flips is not None:
        ip[:, :2] = _v1_rows(n, flips, 2, "flips") != 0
    dp = np.array([invert_affine(row) for row in m.tolist()], dtype=np.float64)
    return randaug_v1_slot(batch_u8, [V1_WARP] * n, iparam=ip, dparam=dp, apply=apply, **kw)


def cv_scale_resize_crop(batch_u8, scales, origins, apply=None, **kw):
    """``Scale_Resize_Crop``: cv2.resize(INTER_CUBIC) S -> int(S scales[n]) (None: the scale gate did not fire, S stays), resize to
    S + 20, crop S at origins[n] = (y1, x1) pixels, where apply[n].  Square images only."""
    import numpy as np
    n = batch_u8.shape[0]
    s = batch_u8.shape[2]
    ip = np.zeros((n, 4), np.int64)
    ip[:, 0] = [s if sc is None else int(s * float(sc)) for sc in scales]
    ip[:, 1:3] = _v1_rows(n, origins, 2, "origins")
    return randaug_v1_slot(batch_u8, [V1_RESIZE] * n, iparam=ip, apply=apply, **kw)


def gaussian_noise(batch_u8, sigmas, seeds, apply=None, **kw):
    """Additive Gaussian noise, one normal per pixel shared by the channels: out = clip(x + rint(sigmas[n] z)); z from Philox4x32-10
    keyed by the 64-bit seeds[n] (include/sslcr.h states the stream; it is this project's, not imgaug's)."""
    import numpy as np
    n = batch_u8.shape[0]
    ip, dp = np.zeros((n, 4), np.int64), np.zeros((n, 6), np.float64)
    dp[:, 0] = _v1_rows(n, sigmas, 0, "sigmas")
    if len(seeds) != n:
        raise ValueError("seeds must be [N]")
    for i, sd in enumerate(seeds):
        sd = int(sd)
        if not 0 <= sd < 1 << 64:
            raise ValueError("seeds must be 64-bit unsigned integers")
        ip[i, 0], ip[i, 1] = sd & 0xFFFFFFFF, sd >> 32
    return randaug_v1_slot(batch_u8, [V1_NOISE] * n, iparam=ip, dparam=dp, apply=apply, **kw)


def philox_words(seed, count, device, first=0):
    """the integer stream of ``gaussian_noise``: Philox4x32-10 words at counters first .. first + count - 1 -> uint32-valued int64 [count, 4]"""
    out = torch.empty((count, 4), dtype=torch.int32, device=device)
    L.check(L.lib().sslcr_augv1_philox(int(seed), int(first), count, L.ptr(out), L.stream_ptr()))
    return out.to(torch.int64) & 0xFFFFFFFF


def _uniform(rng, a, b):
    """``random.uniform(a, b)`` = a + (b - a) r, with albumentations 0.1.8's UNSORTED ``to_tuple`` limits"""
    return a + (b - a) * rng.random()


class RandAugmentDevice:
    """Batched counterpart of ``RandAugment(n, m)`` (models/randaugment.py:119-144) for a uint8 NCHW batch that sits in HBM.

    Per image the reference draws ``ops = random.choices(augment_pool, k=n)`` and, per op, ``v = np.random.randint(1, m)``; the op
    then makes its own draws from ``random``.  Here the same draws are made on the host, image after image and op after op, from
    the generators passed in; the ops with restatable arithmetic -- Color, Brightness, Contrast -- run on the device, batched per op
    slot with an apply mask.  The six geometric / blur / noise / HSV ops are albumentations 0.1.8 + OpenCV code that is not
    installed here and cannot be pinned; they depend on ``cv_ops``:

    ``"host"`` (default): they go through ``host_ops[name](img_hwc_uint8_numpy, val) -> numpy`` if given (the image makes a round
    trip through host memory for that slot), else NotImplementedError names the op.  A host op draws from the module-level generators
    when it RUNS (after the whole batch has been planned), so a batch that mixes host ops in does not consume the ``random`` stream in
    the reference's image-by-image order; batches served by the device ops alone do.

    ``"device"``: ``plan`` makes the op's own draws in the reference's order -- the sign flip, ``Compose``'s ``random()``, every
    transform's gate (the p = 1 ones included), then the parameters; ``np_rng`` serves ``Blur``'s kernel choice and, as this project's
    own order, Noise's sigma and 64-bit seed -- and ``run`` applies them with ``randaug_v1_slot``: the arithmetic include/sslcr.h
    defines (PARITY UNPINNED against the libraries), no host transfer of pixels, no synchronisation.  Square images only for the
    three ops that crop.  A name present in ``host_ops`` still goes to the host."""

    POOL = (("HSV", -1, 1), ("Noise", 0, 0.15), ("Scale_Resize_Crop", 0.8, 1.2), ("Shift_Scale_Rotate", 0.01, 0.1),
            ("Color", -0.035, 0.035), ("Blur_img", 0, 2), ("Brightness", -0.2, 0.2), ("Contrast", -0.2, 0.2), ("Rotate_Crop", -90, 90))
    CV = ("HSV", "Noise", "Scale_Resize_Crop", "Shift_Scale_Rotate", "Blur_img", "Rotate_Crop")

    def __init__(self, n, m, rng, np_rng, host_ops=None, cv_ops="host"):
        if cv_ops not in ("host", "device"):
            raise ValueError('cv_ops must be "host" or "device"')
        self.n, self.m, self.rng, self.np_rng, self.host_ops, self.cv_ops = n, m, rng, np_rng, host_ops or {}, cv_ops

    def _on_device(self, name):
        return self.cv_ops == "device" and name in self.CV and name not in self.host_ops

    def _cv_draws(self, name, v):
        """the draws of ONE call of the op ``name`` with level v, in the reference's order -> the row's payload"""
        rng = self.rng
        if name in ("HSV", "Shift_Scale_Rotate", "Rotate_Crop") and rng.random() < 0.5:
            v = -v
        rng.random()                                                     # Compose: random() < 1
        if name == "HSV":                                                # HueSaturationValue(p=0.5): hue, sat, val
            if not rng.random() < 0.5:
                return (False, 0.0, 0.0, 0.0)
            return (True, _uniform(rng, -v, v), _uniform(rng, -v, v), _uniform(rng, -v, v))
        if name == "Shift_Scale_Rotate":                                 # ShiftScaleRotate(p=0.5): angle, scale, dx, dy; RandomCrop(p=1)
            row = (False, 0.0, 1.0, 0.0, 0.0)
            if rng.random() < 0.5:
                lim = v + 0.5
                row = (True, _uniform(rng, -90, 90), _uniform(rng, 1 + -lim, 1 + lim), _uniform(rng, -v, v), _uniform(rng, -v, v))
            rng.random(); rng.random(); rng.random()                     # RandomCrop: gate, h_start, w_start (the crop is the identity)
            return row
        if name == "Rotate_Crop":                                        # Flip(p=0.5): randint(-1, 1); Rotate(p=0.5); CenterCrop(p=1)
            flip = rng.randint(-1, 1) if rng.random() < 0.5 else None
            angle = _uniform(rng, -v, v) if rng.random() < 0.5 else None
            rng.random()
            return (flip, angle)
        if name == "Scale_Resize_Crop":                                  # RandomScale(p=0.5); Resize(p=1); RandomCrop(p=1): h_start, w_start
            scale = _uniform(rng, 1 + -v, 1 + v) if rng.random() < 0.5 else None
            rng.random()
            rng.random()
            return (scale, rng.random(), rng.random())
        if name == "Blur_img":                                           # Blur(p=0.5): np.random.choice of the odd sizes up to the limit
            import numpy as np
            if not rng.random() < 0.5:
                return (False, 0)
            return (True, int(self.np_rng.choice(np.arange(3, int(v + 5) + 1, 2))))
        # Noise: IAAAdditiveGaussianNoise(p=0.5); sigma and the seed from np_rng (this project's order: imgaug seeds its own generator)
        import numpy as np
        if not rng.random() < 0.5:
            return (False, 0.0, 0)
        return (True, float(self.np_rng.uniform(0, v * 255)), int(self.np_rng.randint(0, 1 << 64, dtype=np.uint64)))

    def plan(self, count):
        """the draws of ``count`` successive RandAugment calls -> [[(name, payload)] * n] * count.  Color: (hmod, dmod, emod);
        Brightness / Contrast: (applied, alpha, beta); a host op: its level; a device-side cv op: what ``_cv_draws`` returns"""
        plan = []
        # the reference finishes one image (all its ops, in order) before it draws for the next
        for _ in range(count):
            ops = self.rng.choices(self.POOL, k=self.n)
            row = []
            for name, lo, hi in ops:
                v = int(self.np_rng.randint(1, self.m))
                val = (float(v) / 30) * float(hi - lo) + lo
                if name == "Color":
                    row.append((name, colour_shifts(self.rng)))
                elif name == "Brightness":
                    row.append((name, brightness_contrast_params(self.rng, brightness_limit=val)))
                elif name == "Contrast":
                    row.append((name, brightness_contrast_params(self.rng, contrast_limit=val)))
                elif self._on_device(name):
                    row.append((name, self._cv_draws(name, val)))
                else:
                    if name not in self.host_ops:
                        raise NotImplementedError(f"RandAugment op {name} (albumentations 0.1.8) has no device kernel; pass host_ops[{name!r}]")
                    row.append((name, val))      # the host op makes its own draws from the module-level generators when it runs
            plan.append(row)
        return plan

    @staticmethod
    def cv_slot_row(name, payload, hw):
        """one image's (code, iparam row, dparam row) for ``randaug_v1_slot`` from its plan payload"""
        h, w = hw
        ip, dp = [0, 0, 0, 0], [0.0] * 6
        if name == "HSV":
            if not payload[0]:
                return V1_COPY, ip, dp
            return V1_HSV, [int(round(payload[1])), int(round(payload[2])), int(round(payload[3])), 0], dp
        if name == "Shift_Scale_Rotate":
            if not payload[0]:
                return V1_COPY, ip, dp
            return V1_WARP, ip, invert_affine(rotation_matrix(hw, payload[1], payload[2], payload[3], payload[4]))
        if name == "Rotate_Crop":
            flip, angle = payload
            if flip is None and angle is None:
                return V1_COPY, ip, dp
            ip[0], ip[1] = int(flip in (1, -1)), int(flip in (0, -1))      # cv2.flip: 0 vertical, 1 horizontal, -1 both
            return V1_WARP, ip, invert_affine(rotation_matrix(hw, angle or 0.0))
        if name == "Scale_Resize_Crop":
            scale, hs, ws = payload
            return V1_RESIZE, [h if scale is None else int(h * scale), int(SRC_MARGIN * hs), int(SRC_MARGIN * ws), 0], dp
        if name == "Blur_img":
            return (V1_BLUR, [payload[1], 0, 0, 0], dp) if payload[0] else (V1_COPY, ip, dp)
        if name == "Noise":
            if not payload[0]:
                return V1_COPY, ip, dp
            return V1_NOISE, [payload[2] & 0xFFFFFFFF, payload[2] >> 32, 0, 0], [payload[1]] + [0.0] * 5
        raise ValueError(f"no device op {name!r}")

    def run(self, batch_u8, plan):
        """apply a plan (one row per image) to an NCHW batch"""
        N = batch_u8.shape[0]
        if len(plan) != N:
            raise ValueError("one plan row per image expected")
        hw = (batch_u8.shape[2], batch_u8.shape[3])
        cur = batch_u8
        for slot in range(self.n):
            names = [plan[i][slot][0] for i in range(N)]
            if "Color" in names:
                sh = [plan[i][slot][1] if names[i] == "Color" else (0.0, 0.0, 0.0) for i in range(N)]
                cur = hed_colour_augment(cur, sh, [nm == "Color" for nm in names])
            if "Brightness" in names or "Contrast" in names:
                bc = [nm in ("Brightness", "Contrast") and plan[i][slot][1][0] for i, nm in enumerate(names)]
                ab = [plan[i][slot][1][1:] if bc[i] else (1.0, 0.0) for i in range(N)]
                if any(bc):
                    cur = brightness_contrast(cur, ab, bc)
            if any(self._on_device(nm) for nm in names):
                if hw[0] != hw[1] and any(nm in ("Scale_Resize_Crop", "Shift_Scale_Rotate", "Rotate_Crop") and self._on_device(nm) for nm in names):
                    raise ValueError(f"the crops of the pool take a square image, got {hw[0]}x{hw[1]}")
                rows = [self.cv_slot_row(nm, plan[i][slot][1], hw) if self._on_device(nm) else (V1_COPY, [0] * 4, [0.0] * 6)
                        for i, nm in enumerate(names)]
                if any(r[0] != V1_COPY for r in rows):
                    cur = randaug_v1_slot(cur, [r[0] for r in rows], iparam=[r[1] for r in rows], dparam=[r[2] for r in rows])
            host = [i for i, nm in enumerate(names) if nm not in ("Color", "Brightness", "Contrast") and not self._on_device(nm)]
            if host:
                if cur is batch_u8:
                    cur = batch_u8.clone()
                for i in host:
                    img = cur[i].permute(1, 2, 0).contiguous().cpu().numpy()
                    res = self.host_ops[names[i]](img, plan[i][slot][1])
                    if isinstance(res, dict):
                        res = res["image"]
                    cur[i] = torch.from_numpy(res).permute(2, 0, 1).to(cur.device)
        return cur

    def __call__(self, batch_u8):
        return self.run(batch_u8, self.plan(batch_u8.shape[0]))


class TransformFixDevice:
    """Batched, device-side counterpart of the WHOLE ``TransformFix(image_size, N)`` (dataset.py:663-677): ``TransformFixGeometric``'s
    two flip + crop gathers, then ``RandAugment(n=N, m=10)`` on the strong branch with every op of the pool on the device
    (``cv_ops="device"``).  -> (weak uint8 [B,3,S,S], strong uint8 [B,3,S,S]); no pixel makes a host round trip."""

    def __init__(self, image_size, N, generator=None, rng=None, np_rng=None):
        import random
        import numpy as np
        self.geometric = TransformFixGeometric(image_size, generator)
        self.randaugment = RandAugmentDevice(N, 10, rng if rng is not None else random, np_rng if np_rng is not None else np.random,
                                             cv_ops="device")

    def __call__(self, batch_u8, src_hwc=False):
        weak, strong = self.geometric(batch_u8, src_hwc)
        return weak, self.randaugment(strong)


# ------------------------------------------------------------------------------------------------ RSP v2: the Pillow RandAugment pool
# Pretraining_v2/models/randaugment.py:38-190.  Twelve of the fourteen ops are plain Pillow calls; csrc/augment_v2.hip restates them
# byte for byte, one op SLOT of a whole batch per call.  The host side below makes the draws and turns each op's level into the
# numbers Pillow itself would derive from it (enhance factor, 16.16 rotation coefficients, translate index tables, shear matrix).
V2_COPY, V2_BRIGHTNESS, V2_CONTRAST, V2_COLOR, V2_AUTOCONTRAST, V2_EQUALIZE, V2_SHARPNESS, V2_NEAREST_FIXED, V2_NEAREST_TABLE, V2_BICUBIC = range(10)
_V2_STATS = (1 << V2_CONTRAST) | (1 << V2_AUTOCONTRAST) | (1 << V2_EQUALIZE)
_V2_ENHANCE = {"brightness": V2_BRIGHTNESS, "contrast": V2_CONTRAST, "color": V2_COLOR, "sharpness": V2_SHARPNESS}
_V2_POINT = dict(_V2_ENHANCE, identity=V2_COPY, autocontrast=V2_AUTOCONTRAST, equalize=V2_EQUALIZE)
del _V2_POINT["sharpness"]


def _v2_batch(batch_u8, hwc, who):
    if not batch_u8.is_cuda or batch_u8.dtype != torch.uint8 or not batch_u8.is_contiguous() or batch_u8.dim() != 4:
        raise ValueError(f"{who}: contiguous uint8 CUDA batch [N,3,H,W] or [N,H,W,3] expected")
    if (batch_u8.shape[3] if hwc else batch_u8.shape[1]) != 3:
        raise ValueError("three colour channels expected")
    return (batch_u8.shape[1], batch_u8.shape[2]) if hwc else (batch_u8.shape[2], batch_u8.shape[3])


def enhance_factor(val):
    """``(factor / MAX_LEVEL) * 1.8 + 0.1`` (models/randaugment.py:45) as the float32 Image.blend receives"""
    import numpy as np
    return float(np.float32(val / 10 * 1.8 + 0.1))


def rotate_coefficients(degrees, hw):
    """``Image.rotate(degrees)`` for an H x W image -> Pillow's six 16.16 integers (Image.rotate's matrix about the centre, then
    affine_fixed's FIX(), the half-pixel centre folded into a2 / a5)."""
    import math
    h, w = hw
    a = -math.radians(degrees % 360.0)
    m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]
    cx, cy = w / 2, h / 2
    m[2] = m[0] * (-cx) + m[1] * (-cy) + m[2] + cx
    m[5] = m[3] * (-cx) + m[4] * (-cy) + m[5] + cy
    for x, y in ((0, 0), (w, h)):      # Pillow walks in fixed point only while both corners stay inside 16 bits
        if not (abs(x * m[0] + y * m[1] + m[2]) < 32768.0 and abs(x * m[3] + y * m[4] + m[5]) < 32768.0):
            raise ValueError(f"rotate: a {h}x{w} image leaves Pillow's fixed-point range")

    def fix(v):
        return int(math.floor(v * 65536.0 + 0.5))
    return [fix(m[0]), fix(m[1]), fix(m[2] + m[0] * 0.5 + m[1] * 0.5), fix(m[3]), fix(m[4]), fix(m[5] + m[3] * 0.5 + m[4] * 0.5)]


def randaug_v2_slot(batch_u8, codes, *, factor=None, fixed=None, shift=None, affine=None, hwc=False, out_hwc=None, out=None,
                    workspace=None):
    """One op slot on a uint8 batch in HBM: image n takes ``codes[n]`` (V2_*) with row n of the tables its code reads -- factor [N]
    (the ImageEnhance ops), fixed [N,6] (NEAREST_FIXED), shift [N,2] = (px, py) (NEAREST_TABLE), affine [N,6] (BICUBIC).  -> a new
    batch in the layout ``out_hwc`` asks for (default: the input's).  ``workspace``: what ``v2_workspace`` returns, to reuse it."""
    import numpy as np
    h, w = _v2_batch(batch_u8, hwc, "randaug_v2_slot")
    n, dev = batch_u8.shape[0], batch_u8.device
    out_hwc = hwc if out_hwc is None else out_hwc
    codes = np.asarray(codes, dtype=np.int32)
    if codes.shape != (n,) or codes.min() < V2_COPY or codes.max() > V2_BICUBIC:
        raise ValueError("codes must be [N] op codes")
    mask = 0
    for c in np.unique(codes):
        mask |= 1 << int(c)

    def table(t, dtype, shape, needed, name):
        if not needed:
            return None
        if t is None:
            raise ValueError(f"randaug_v2_slot: {name} is needed by the ops of this slot")
        t = np.ascontiguousarray(np.asarray(t, dtype=dtype))
        if t.shape != shape or not np.isfinite(t).all():
            raise ValueError(f"{name} must be {list(shape)} finite numbers")
        return torch.from_numpy(t).to(dev)
    t_op = torch.from_numpy(codes).to(dev)
    t_f = table(factor, np.float32, (n,), mask & sum(1 << c for c in _V2_ENHANCE.values()), "factor")
    t_fx = table(fixed, np.int32, (n, 6), mask & (1 << V2_NEAREST_FIXED), "fixed")
    t_s = table(shift, np.float64, (n, 2), mask & (1 << V2_NEAREST_TABLE), "shift")
    t_a = table(affine, np.float64, (n, 6), mask & (1 << V2_BICUBIC), "affine")
    hist = lsum = lut = tab = None
    if mask & (_V2_STATS | (1 << V2_BRIGHTNESS) | (1 << V2_NEAREST_TABLE)):
        hist, lsum, lut, tab = workspace if workspace is not None else v2_workspace(n, h, w, dev)
    shape = (n, h, w, 3) if out_hwc else (n, 3, h, w)
    dst = out if out is not None else torch.empty(shape, dtype=torch.uint8, device=dev)
    if tuple(dst.shape) != shape or dst.dtype != torch.uint8 or not dst.is_contiguous() or dst.device != dev:
        raise ValueError("out: contiguous uint8 batch of the output layout expected")
    d = L.AugV2Desc(L.ptr(batch_u8), L.ptr(dst), L.ptr(t_op), L.ptr(t_f), L.ptr(t_fx), L.ptr(t_s), L.ptr(t_a),
                    L.ptr(hist), L.ptr(lsum), L.ptr(lut), L.ptr(tab), mask, n, h, w, int(hwc), int(out_hwc))
    L.check(L.lib().sslcr_randaug_v2_slot(d, L.stream_ptr()))
    return dst


def v2_workspace(n, h, w, device):
    """scratch of ``randaug_v2_slot`` for N images of H x W: histograms, luma sums, LUTs, translate index tables"""
    return (torch.empty((n, 768), dtype=torch.int32, device=device), torch.empty((n,), dtype=torch.int64, device=device),
            torch.empty((n, 768), dtype=torch.uint8, device=device), torch.empty((n, w + h), dtype=torch.int32, device=device))


def _v2_apply(apply, n):
    return [True] * n if apply is None else [bool(a) for a in apply]


def pil_point_ops(batch_u8, names, factors=None, **kw):
    """The point-wise family: per image one of identity / brightness / contrast / color (ImageEnhance, ``factors[n]`` the enhance
    factor) / autocontrast / equalize (ImageOps), or None = unchanged."""
    codes = [_V2_POINT[nm or "identity"] for nm in names]
    return randaug_v2_slot(batch_u8, codes, factor=factors, **kw)


def pil_sharpness(batch_u8, factors, apply=None, **kw):
    """``ImageEnhance.Sharpness(img).enhance(factors[n])`` where apply[n]."""
    ap = _v2_apply(apply, batch_u8.shape[0])
    return randaug_v2_slot(batch_u8, [V2_SHARPNESS if a else V2_COPY for a in ap], factor=factors, **kw)


def pil_rotate(batch_u8, degrees, apply=None, *, hwc=False, **kw):
    """``img.rotate(degrees[n])`` (nearest, fill 0) where apply[n]."""
    hw = _v2_batch(batch_u8, hwc, "pil_rotate")
    ap = _v2_apply(apply, batch_u8.shape[0])
    fixed = [rotate_coefficients(dg, hw) if a else [0] * 6 for dg, a in zip(degrees, ap)]
    return randaug_v2_slot(batch_u8, [V2_NEAREST_FIXED if a else V2_COPY for a in ap], fixed=fixed, hwc=hwc, **kw)


def pil_translate(batch_u8, pixels_xy, apply=None, *, hwc=False, **kw):
    """``img.transform(size, AFFINE, (1, 0, px, 0, 1, py))`` (nearest, fill 0) with pixels_xy[n] = (px, py) where apply[n]."""
    ap = _v2_apply(apply, batch_u8.shape[0])
    return randaug_v2_slot(batch_u8, [V2_NEAREST_TABLE if a else V2_COPY for a in ap], shift=[tuple(p) for p in pixels_xy], hwc=hwc, **kw)


def pil_affine_bicubic(batch_u8, coefficients, apply=None, **kw):
    """``img.transform(size, AFFINE, coefficients[n], BICUBIC)`` (fill 0) where apply[n]; shear_x is (1, lv, 0, 0, 1, 0), shear_y
    (1, 0, 0, lv, 1, 0)."""
    ap = _v2_apply(apply, batch_u8.shape[0])
    return randaug_v2_slot(batch_u8, [V2_BICUBIC if a else V2_COPY for a in ap], affine=coefficients, **kw)


# The two histopathology ops of the pool (hed :135-144, hsv :125-132) run in place on the slot's output: csrc/augment_v2.hip restates
# HedColorAugmenter / HsbColorAugmenter.transform and the scikit-image 0.15.0 conversions under them.  The host side makes the draws of
# augmentor.randomize() and turns them into the numbers the in-place numpy ops of the reference use.
V2C_COPY, V2C_HED, V2C_HSV = range(3)
_V2_COLOUR = {"hed": V2C_HED, "hsv": V2C_HSV}
HED_CUTOFF = (0.15, 0.85)                # cutoff_range of models/randaugment.py:141


_V2_HED_MATRICES = None


def v2_hed_matrices():
    """-> (hed_from_rgb, rgb_from_hed) as float32 [3,3], built like custom_hed_transform.py:8-11: the float32 stain matrix and the
    float32 of its inverse (numpy's inverse here, scipy's there)"""
    global _V2_HED_MATRICES
    if _V2_HED_MATRICES is None:
        import numpy as np
        m = np.array(_RGB_FROM_HED).astype(np.float32)
        _V2_HED_MATRICES = (np.linalg.inv(m).astype(np.float32), m)
    return _V2_HED_MATRICES


def colour_param_row(name, draws):
    """the six doubles of one image's ``param`` row from the draws of ``randomize()``: hed (s_h, s_e, s_d, b_h, b_e, b_d) ->
    float32(1 + s_j) and float32(b_j), what ``patch_hed[:, :, j] *= (1.0 + s_j)`` / ``+= b_j`` use on a float32 array; hsv
    (s_hue, s_sat[, s_brightness]) -> (s_hue % 1.0, s_sat), the brightness sigma of the pool's range (0, 0) being 0"""
    import numpy as np
    d = [float(v) for v in draws]
    if name == "hed":
        if len(d) != 6:
            raise ValueError("hed: three sigmas and three biases expected")
        return [float(np.float32(1.0 + v)) for v in d[:3]] + [float(np.float32(v)) for v in d[3:]]
    if name == "hsv":
        if len(d) not in (2, 3):
            raise ValueError("hsv: hue and saturation sigma (and the unused brightness sigma) expected")
        if len(d) == 3 and d[2] != 0.0:
            raise ValueError("hsv: a brightness sigma other than 0 has no kernel (the pool's range is (0, 0))")
        return [d[0] % 1.0 if d[0] != 0.0 else 0.0, d[1], 0.0, 0.0, 0.0, 0.0]
    raise ValueError(f"no colour op {name!r}")


def pil_colour_ops(batch_u8, names, params, *, hwc=False, out=None, workspace=None):
    """The colour family: per image ``"hed"`` / ``"hsv"`` (``params[n]`` the draws of its ``randomize()``, see ``colour_param_row``)
    or None = unchanged.  The kernels work in place: ``out=batch_u8`` modifies the batch itself, any other ``out`` (default: a new
    batch) receives a copy first.  ``workspace``: an int64 [N] device tensor to reuse for the byte sums of the hed cutoff."""
    import numpy as np
    h, w = _v2_batch(batch_u8, hwc, "pil_colour_ops")
    n, dev = batch_u8.shape[0], batch_u8.device
    if len(names) != n or len(params) != n:
        raise ValueError("one name and one parameter row per image expected")
    codes, rows = np.zeros(n, np.int32), np.zeros((n, 6), np.float64)
    for i, nm in enumerate(names):
        if nm is not None:
            if nm not in _V2_COLOUR:
                raise ValueError(f"no colour op {nm!r}")
            codes[i], rows[i] = _V2_COLOUR[nm], colour_param_row(nm, params[i])
    if not np.isfinite(rows).all():
        raise ValueError("params must be finite numbers")
    dst = batch_u8 if out is batch_u8 else out if out is not None else torch.empty_like(batch_u8)
    if dst is not batch_u8:
        if dst.shape != batch_u8.shape or dst.dtype != torch.uint8 or not dst.is_contiguous() or dst.device != dev:
            raise ValueError("out: contiguous uint8 batch of the input's shape expected")
        dst.copy_(batch_u8)
    mask = 0
    for c in np.unique(codes):
        mask |= 1 << int(c)
    if not mask & ~(1 << V2C_COPY):
        return dst
    bsum = None
    if mask & (1 << V2C_HED):
        bsum = workspace if workspace is not None else torch.empty((n,), dtype=torch.int64, device=dev)
        if bsum.dtype != torch.int64 or bsum.dim() != 1 or bsum.shape[0] < n or not bsum.is_contiguous() or bsum.device != dev:
            raise ValueError("workspace: contiguous int64 [>= N] tensor on the batch's device expected")
    t_op, t_p = torch.from_numpy(codes).to(dev), torch.from_numpy(rows).to(dev)
    inv, fwd = v2_hed_matrices()
    d = L.AugV2ColourDesc(L.ptr(dst), L.ptr(t_op), L.ptr(t_p), L.ptr(bsum), HED_CUTOFF[0], HED_CUTOFF[1],
                          (L.f32 * 9)(*inv.reshape(-1).tolist()), (L.f32 * 9)(*fwd.reshape(-1).tolist()), mask, n, h, w, int(hwc))
    L.check(L.lib().sslcr_randaug_v2_colour(d, L.stream_ptr()))
    return dst


class RandAugmentV2Device:
    """Batched counterpart of the RSP v2 ``RandAugment(n, m)`` (Pretraining_v2/models/randaugment.py:195-213) for a uint8 batch in HBM,
    [N,H,W,3] as the v2 dataset holds it or [N,3,H,W]; -> [N,3,H,W] uint8, what the stem ingests.

    Per image the reference draws ``ops = random.sample(augment_pool, k=n)`` and per op ``val = np.random.uniform(1, m)``; rotate,
    translate and shear then draw ``random.choice([1, 0])``, 0 negating the level.  The same draws are made here on the host, image
    after image, from ``rng`` (a ``random.Random`` or the ``random`` module) and ``np_rng`` (a ``RandomState`` or ``numpy.random``);
    the twelve Pillow ops then run on the device, one launch per op slot.  ``hed`` / ``hsv`` (scikit-image arithmetic) depend on
    ``colour_ops``:

    ``"host"`` (default): they go through ``host_ops[name](img_hwc_uint8_numpy, val) -> numpy`` if given (a round trip through host
    memory for that image and slot), else NotImplementedError names the op.  A host op draws from numpy's global generator when it
    RUNS, after the whole batch has been planned, so only batches served by the device ops alone consume the streams in the
    reference's image-by-image order.

    ``"device"``: ``plan`` makes the op's own draws -- what ``augmentor.randomize()`` draws inside the op (:131, :143), from the same
    numpy stream as ``val`` and right after it -- so the whole pool consumes both streams image by image as the reference does; they
    ride in the row's third slot.  ``run`` passes those images through the slot call as COPY and then applies ``pil_colour_ops`` in
    place to the slot's output: no host transfer, no synchronisation.  A name present in ``host_ops`` still goes to the host."""

    POOL = ("identity", "contrast", "brightness", "sharpness", "rotate", "translate_x", "translate_y", "shear_x", "shear_y",
            "hed", "hsv", "autocontrast", "color", "equalize")         # augment_pool() order: random.sample depends on it
    SIGNED = ("rotate", "translate_x", "translate_y", "shear_x", "shear_y")
    HOST = ("hed", "hsv")

    def __init__(self, n, m, rng, np_rng, host_ops=None, colour_ops="host"):
        if colour_ops not in ("host", "device"):
            raise ValueError('colour_ops must be "host" or "device"')
        self.n, self.m, self.rng, self.np_rng, self.host_ops, self.colour_ops = n, m, rng, np_rng, host_ops or {}, colour_ops

    def _on_device(self, name):
        return self.colour_ops == "device" and name in self.HOST and name not in self.host_ops

    def plan(self, count):
        """the draws of ``count`` successive RandAugment calls -> [[(name, val, sign)] * n] * count; sign is None where none is drawn.
        For a device-side hed / hsv the third slot holds the op's own draws: (s_h, s_e, s_d, b_h, b_e, b_d) / (s_hue, s_sat, s_brightness)"""
        plan = []
        for _ in range(count):
            row = []
            for name in self.rng.sample(self.POOL, k=self.n):
                val = float(self.np_rng.uniform(1, self.m))
                if self._on_device(name):
                    f = val * 0.03                   # hed() / hsv(): factor * 0.03, every range (-factor, factor)
                    if name == "hed":                # HedColorAugmenter.randomize: the three sigmas, then the three biases
                        extra = tuple(float(self.np_rng.uniform(-f, f)) for _ in range(6))
                    else:                            # HsbColorAugmenter.randomize: the brightness range is (0, 0), not None: drawn, unused
                        extra = (float(self.np_rng.uniform(-f, f)), float(self.np_rng.uniform(-f, f)), float(self.np_rng.uniform(0, 0)))
                    row.append((name, val, extra))
                    continue
                if name in self.HOST and name not in self.host_ops:
                    raise NotImplementedError(f"RandAugment v2 op {name} (scikit-image) has no device kernel; pass host_ops[{name!r}]")
                row.append((name, val, self.rng.choice([1, 0]) if name in self.SIGNED else None))
            plan.append(row)
        return plan

    @staticmethod
    def _layout(batch_u8, hwc):
        if hwc is not None:
            return bool(hwc)
        last, first = batch_u8.shape[3] == 3, batch_u8.shape[1] == 3
        if last == first:
            raise ValueError("RandAugmentV2Device: pass hwc= for a batch whose layout the shape does not tell")
        return last

    def run(self, batch_u8, plan, hwc=None):
        """apply a plan (one row per image) -> [N,3,H,W]"""
        hwc = self._layout(batch_u8, hwc)
        h, w = _v2_batch(batch_u8, hwc, "RandAugmentV2Device")
        N = batch_u8.shape[0]
        if len(plan) != N:
            raise ValueError("one plan row per image expected")
        import numpy as np
        ws = v2_workspace(N, h, w, batch_u8.device)
        bsum = torch.empty((N,), dtype=torch.int64, device=batch_u8.device) if self.colour_ops == "device" else None
        cur = batch_u8
        for slot in range(max(self.n, 1)):            # n = 0 still converts the layout
            codes, factor = np.zeros(N, np.int32), np.zeros(N, np.float32)
            fixed, affine, shift = np.zeros((N, 6), np.int32), np.zeros((N, 6), np.float64), np.zeros((N, 2), np.float64)
            host, colour, cparams = [], [None] * N, [None] * N
            for i in range(N if self.n else 0):
                name, val, sign = plan[i][slot]
                if self._on_device(name):
                    if not isinstance(sign, tuple):
                        raise ValueError(f"the plan row of a device-side {name} must carry its draws (plan() with colour_ops=\"device\")")
                    colour[i], cparams[i] = name, sign          # COPY in the slot call, then in place on its output
                elif name in _V2_ENHANCE:
                    codes[i], factor[i] = _V2_ENHANCE[name], enhance_factor(val)
                elif name in _V2_POINT:
                    codes[i] = _V2_POINT[name]
                elif name in self.HOST:
                    host.append(i)
                else:
                    lv = val / 10 * {"rotate": 30., "translate_x": float(10), "translate_y": float(10), "shear_x": 0.3, "shear_y": 0.3}[name]
                    lv = lv if sign == 1 else -lv
                    if name == "rotate":
                        codes[i], fixed[i] = V2_NEAREST_FIXED, rotate_coefficients(lv, (h, w))
                    elif name == "translate_x":
                        codes[i], shift[i, 0] = V2_NEAREST_TABLE, lv
                    elif name == "translate_y":
                        codes[i], shift[i, 1] = V2_NEAREST_TABLE, lv
                    else:
                        codes[i], affine[i] = V2_BICUBIC, (1, lv, 0, 0, 1, 0) if name == "shear_x" else (1, 0, 0, lv, 1, 0)
            nxt = randaug_v2_slot(cur, codes, factor=factor, fixed=fixed, shift=shift, affine=affine, hwc=hwc if slot == 0 else False,
                                  out_hwc=False, workspace=ws)
            if any(colour):
                pil_colour_ops(nxt, colour, cparams, out=nxt, workspace=bsum)
            for i in host:
                name, val, _ = plan[i][slot]
                img = nxt[i].permute(1, 2, 0).contiguous().cpu().numpy()
                nxt[i] = torch.from_numpy(self.host_ops[name](img, val)).permute(2, 0, 1).to(nxt.device)
            cur = nxt
        return cur

    def __call__(self, batch_u8, hwc=None):
        return self.run(batch_u8, self.plan(batch_u8.shape[0]), hwc)


class TripletRandAugmentV2:
    """``TensorDataset_Transform.__getitem__`` (Pretraining_v2/dataset.py:85-95) for a whole RSP batch that sits in HBM: the transform
    on the three tile batches D1, D2, D3, the draws made triplet by triplet in the order D1, D2, D3 as the dataset makes them sample
    by sample.  -> three [N,3,H,W] uint8 batches."""

    def __init__(self, n, m, rng, np_rng, host_ops=None, colour_ops="host"):
        self.aug = RandAugmentV2Device(n, m, rng, np_rng, host_ops, colour_ops)

    def __call__(self, d1, d2, d3, hwc=None):
        N = d1.shape[0]
        if d2.shape[0] != N or d3.shape[0] != N:
            raise ValueError("three batches of one length expected")
        plan = self.aug.plan(3 * N)
        return tuple(self.aug.run(d, plan[k::3], hwc) for k, d in enumerate((d1, d2, d3)))
