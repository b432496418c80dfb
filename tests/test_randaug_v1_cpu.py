"""CPU-only checks of the v1 RandAugment pool's OpenCV-style ops (sslcr_randaug_v1_slot): the NumPy restatement of the arithmetic
include/sslcr.h defines (tests/_cv_ref.py) against yardsticks that ARE installed -- scipy, colorsys, torch -- and the host side of
ssl_cr_histo_amd/augment.py: the draw order against literal transcriptions of the reference's calls, the weight table, the plan-time
refusals and the ABI.  PARITY UNPINNED against OpenCV / albumentations / imgaug: none of them is installed."""
import colorsys
import ctypes
import os
import random

import numpy as np
import pytest
import torch

import _cv_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _img(seed, h, w):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def _smooth(seed, h, w):
    """a low-frequency image: interpolation errors of a yardstick show on it without the clipping noise of white noise"""
    rs = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    planes = [127 + 100 * np.sin(yy * rs.uniform(0.1, 0.5) + rs.uniform(0, 6)) * np.cos(xx * rs.uniform(0.1, 0.5) + rs.uniform(0, 6)) for _ in range(3)]
    return np.clip(np.rint(np.stack(planes, -1)), 0, 255).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ restatement vs installed yardsticks
@pytest.mark.parametrize("k", [3, 5, 7])
@pytest.mark.parametrize("hw", [(8, 8), (24, 40), (27, 33)])
def test_blur_equals_scipy_uniform_filter(k, hw):
    from scipy.ndimage import uniform_filter
    img = _img(k, *hw)
    want = np.stack([np.rint(uniform_filter(img[..., c].astype(np.float64), k, mode="mirror")) for c in range(3)], -1)
    # a mean whose float64 value sits within rounding noise of x.5 cannot occur: k*k is odd
    assert np.array_equal(R.blur(img, k), want.astype(np.uint8))


def test_rgb_to_hsv_within_one_of_colorsys():
    rs = np.random.RandomState(0)
    img = rs.randint(0, 256, (64, 64, 3)).astype(np.uint8)
    img[0, :32] = np.arange(32)[:, None] * 8                      # greys (diff = 0), black included
    h, s, v = R.rgb_to_hsv8(img)
    worst = [0.0, 0.0, 0.0]
    for y in range(64):
        for x in range(64):
            r, g, b = (int(c) for c in img[y, x])
            fh, fs, fv = colorsys.rgb_to_hsv(r / 255, g / 255, b / 255)
            dh = abs(int(h[y, x]) - fh * 180)
            dh = min(dh, 180 - dh)                                # half-degrees modulo 180
            worst = [max(worst[0], dh), max(worst[1], abs(int(s[y, x]) - fs * 255)), max(worst[2], abs(int(v[y, x]) - fv * 255))]
    print("rgb->hsv8 max |restatement - colorsys| (h, s, v):", worst)
    assert worst[0] <= 1 and worst[1] <= 1 and worst[2] == 0, worst
    assert h.min() >= 0 and h.max() <= 179


def test_hsv_zero_shift_round_trip_is_recorded():
    """a measurement, no fixed bound (the 8-bit HSV planes lose information); the figure is kept in profiles/augv1_ratios.txt"""
    img = _img(1, 128, 128)
    back = R.shift_hsv(img, 0, 0, 0)
    err = np.abs(back.astype(int) - img.astype(int))
    print("hsv zero-shift round trip: max error", int(err.max()), "mean", float(err.mean()))
    text = open(os.path.join(ROOT, "profiles", "augv1_ratios.txt")).read()
    assert f"hsv_round_trip_max_error {int(err.max())}" in text
    grey = np.repeat(np.arange(256, dtype=np.uint8)[:, None, None], 3, 2).reshape(16, 16, 3)
    assert np.array_equal(R.shift_hsv(grey, 0, 0, 0), grey)       # diff = 0: exact


@pytest.mark.parametrize("src,dst", [(32, 61), (32, 13), (24, 44), (33, 32), (8, 28)])
def test_resize_within_one_of_torch_bicubic(src, dst):
    import torch.nn.functional as F
    img = _smooth(src, src, src)
    t = torch.from_numpy(img).permute(2, 0, 1)[None].double()
    want = np.rint(F.interpolate(t, size=(dst, dst), mode="bicubic", align_corners=False, antialias=False)[0].permute(1, 2, 0).numpy())
    got = R.resize(img, dst, dst).astype(np.float64)
    err = np.abs(got - np.clip(want, 0, 255))
    print(f"resize {src}->{dst}: max |restatement - torch|", err.max())
    assert err.max() <= 1


@pytest.mark.parametrize("angle,scale", [(0.3, 1.0), (45.0, 1.0), (-90.0, 1.0), (17.0, 1.6), (30.0, 0.7)])
def test_warp_within_one_of_torch_grid_sample(angle, scale):
    import torch.nn.functional as F
    h, w = 40, 48
    img = _smooth(7, h, w)
    M = R.invert_affine(R.rotation_matrix(w / 2, h / 2, angle, scale))
    got = R.warp_affine(img, M).astype(np.float64)
    X, Y = R.warp_coords(M, h, w)
    sx, sy = X >> 5, Y >> 5
    inside = (sx - 1 >= 0) & (sx + 2 <= w - 1) & (sy - 1 >= 0) & (sy + 2 <= h - 1)
    assert inside.sum() > 200
    px, py = sx + (X & 31) / 32.0, sy + (Y & 31) / 32.0              # the QUANTISED coordinates, in pixels
    grid = torch.from_numpy(np.stack([(2 * px + 1) / w - 1, (2 * py + 1) / h - 1], -1))[None]
    t = torch.from_numpy(img).permute(2, 0, 1)[None].double()
    want = np.rint(np.clip(F.grid_sample(t, grid, mode="bicubic", padding_mode="zeros", align_corners=False)[0].permute(1, 2, 0).numpy(), 0, 255))
    err = np.abs(got - want)[inside]
    print(f"warp {angle} deg x{scale}: max |restatement - torch| on {int(inside.sum())} inner pixels", err.max())
    assert err.max() <= 1


def test_warp_table_rows_and_unit_tap():
    tab = R.warp_table()
    assert tab.dtype == np.int16 and tab.shape == (1024, 16)
    w = R.warp_weights(tab)
    assert (w.sum(1) == 32768).all()
    unit = np.zeros(16, np.int64)
    unit[5] = 32768
    assert np.array_equal(w[0], unit)
    assert (w[:, 5] >= 0).all() and (np.delete(w, 5, 1) < 32768).all()


def test_warp_and_resize_identities():
    for hw in ((8, 8), (27, 33)):
        img = _img(3, *hw)
        assert np.array_equal(R.warp_affine(img, [1, 0, 0, 0, 1, 0]), img)
        assert np.array_equal(R.warp_affine(img, [1, 0, 0, 0, 1, 0], fx=1), img[:, ::-1])
        assert np.array_equal(R.warp_affine(img, [1, 0, 0, 0, 1, 0], fy=1), img[::-1])
    sq = _img(4, 24, 24)
    assert np.array_equal(R.resize(sq, 24, 24), sq)
    # an integer translation reads through the border: REFLECT_101
    sh = R.warp_affine(sq, [1, 0, -30, 0, 1, 55])
    assert np.array_equal(sh, sq[R.reflect101(np.arange(24) + 55, 24)][:, R.reflect101(np.arange(24) - 30, 24)])


@pytest.mark.parametrize("n", [1, 2, 3, 8, 27])
def test_reflect101_equals_numpy_pad(n):
    if n == 1:
        assert (R.reflect101(np.arange(-5, 6), 1) == 0).all()
        return
    pad = 3 * n
    want = np.pad(np.arange(n), pad, mode="reflect")      # numpy reflects repeatedly past n - 1, as borderInterpolate's loop does
    assert np.array_equal(R.reflect101(np.arange(-pad, n + pad), n), want)


def test_philox_known_answer_and_noise_moments():
    w = R.philox4x32(np.array([0]), 0)[0]
    # Random123's known-answer vector for philox4x32-10, counter 0, key 0
    assert [int(v) for v in w] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    from scipy import stats
    z, _ = R.noise_normals(1 << 16, 0x0123456789ABCDEF)
    z = z.astype(np.float64)
    mean, var, p = z.mean(), z.var(), stats.kstest(z, "norm").pvalue
    print(f"noise over 2^16 normals: mean {mean:.5f} var {var:.5f} KS p {p:.4f}")
    assert np.isfinite(z).all()
    assert abs(mean) < 0.02 and abs(var - 1) < 0.03 and p > 1e-3


def test_noise_half_integer_band_is_thin():
    """the GPU test compares exactly outside |frac(sigma z) - 0.5| < 1e-3: the restatement alone keeps its inputs under the 0.5 % cap"""
    for seed, sigma in ((5, 3.7), (6, 25.0), (7, 38.25)):
        _, sz = R.gaussian_noise(_img(seed, 32, 32), sigma, seed)
        band = np.abs(np.abs(sz - np.floor(sz)) - 0.5) < 1e-3
        assert band.mean() <= 0.005, (sigma, band.mean())


# ------------------------------------------------------------------------------------------------ the host side
def test_c_warp_table_equals_numpy():
    from ssl_cr_histo_amd import augment as A
    assert np.array_equal(A.cv_warp_table(), R.warp_table())


def test_matrices_equal_the_restatement():
    from ssl_cr_histo_amd import augment as A
    for hw, angle, scale, dx, dy in (((32, 32), 33.0, 0.7, 0.1, -0.05), ((24, 40), -90.0, 1.0, 0.0, 0.0)):
        m = R.rotation_matrix(hw[1] / 2, hw[0] / 2, angle, scale)
        m[2] += dx * hw[1]
        m[5] += dy * hw[0]
        assert A.rotation_matrix(hw, angle, scale, dx, dy) == m
        assert A.invert_affine(m) == R.invert_affine(m)


def _transcription(name, v, rnd, nprs):
    """ONE call of the reference's op (models/randaugment.py:51-110) on albumentations 0.1.8, draw by draw: Compose.__call__ draws
    random.random() < p (p = 1), every BasicTransform.__call__ draws random.random() < p before get_params(); to_tuple(v) = (-v, v)"""
    uni = lambda a, b: a + (b - a) * rnd.random()      # random.uniform
    if name == "HSV":
        if rnd.random() < 0.5:
            v = -v
        rnd.random()                                   # Compose
        if rnd.random() < 0.5:                         # HueSaturationValue.get_params
            return (True, uni(-v, v), uni(-v, v), uni(-v, v))
        return (False, 0.0, 0.0, 0.0)
    if name == "Noise":
        rnd.random()
        if rnd.random() < 0.5:
            sigma = float(nprs.uniform(0, v * 255))
            return (True, sigma, int(nprs.randint(0, 1 << 64, dtype=np.uint64)))
        return (False, 0.0, 0)
    if name == "Scale_Resize_Crop":
        rnd.random()
        scale = None
        if rnd.random() < 0.5:                         # RandomScale
            scale = uni(1 + -v, 1 + v)
        assert rnd.random() < 1                        # Resize
        assert rnd.random() < 1                        # RandomCrop
        hs = rnd.random()
        ws = rnd.random()
        return (scale, hs, ws)
    if name == "Shift_Scale_Rotate":
        if rnd.random() < 0.5:
            v = -v
        rnd.random()
        row = (False, 0.0, 1.0, 0.0, 0.0)
        if rnd.random() < 0.5:                         # ShiftScaleRotate(shift_limit=v, scale_limit=v + 0.5, rotate_limit=90)
            angle = uni(-90, 90)
            scale = uni(1 + -(v + 0.5), 1 + (v + 0.5))
            dx = uni(-v, v)
            dy = uni(-v, v)
            row = (True, angle, scale, dx, dy)
        assert rnd.random() < 1                        # RandomCrop
        rnd.random()
        rnd.random()
        return row
    if name == "Blur_img":
        rnd.random()
        if rnd.random() < 0.5:
            return (True, int(nprs.choice(np.arange(3, int(v + 5) + 1, 2))))
        return (False, 0)
    if name == "Rotate_Crop":
        if rnd.random() < 0.5:
            v = -v
        rnd.random()
        flip = angle = None
        if rnd.random() < 0.5:                         # Flip
            flip = rnd.randint(-1, 1)
        if rnd.random() < 0.5:                         # Rotate(limit=v)
            angle = uni(-v, v)
        assert rnd.random() < 1                        # CenterCrop
        return (flip, angle)
    raise AssertionError(name)


def test_draw_order_against_literal_transcriptions():
    from ssl_cr_histo_amd import augment as A
    seen = {}
    for seed in range(40):
        aug = A.RandAugmentDevice(3, 10, random.Random(seed), np.random.RandomState(seed), cv_ops="device")
        plan = aug.plan(6)
        rnd, nprs = random.Random(seed), np.random.RandomState(seed)
        for row in plan:
            ops = rnd.choices(A.RandAugmentDevice.POOL, k=3)
            assert [r[0] for r in row] == [o[0] for o in ops]
            for (name, payload), (_, lo, hi) in zip(row, ops):
                v = int(nprs.randint(1, 10))
                val = (float(v) / 30) * float(hi - lo) + lo
                if name == "Color":
                    want = A.colour_shifts(rnd)
                elif name == "Brightness":
                    want = A.brightness_contrast_params(rnd, brightness_limit=val)
                elif name == "Contrast":
                    want = A.brightness_contrast_params(rnd, contrast_limit=val)
                else:
                    state = rnd.getstate()
                    flipped = name in ("HSV", "Shift_Scale_Rotate", "Rotate_Crop") and _peek(state) < 0.5
                    want = _transcription(name, val, rnd, nprs)
                    fired = want[0] is not None if name in ("Rotate_Crop", "Scale_Resize_Crop") else bool(want[0])
                    seen.setdefault(name, set()).add((flipped, fired))
                assert payload == want, (seed, name)
        # both generators end where the transcription's end: nothing more, nothing less was drawn
        assert aug.rng.random() == rnd.random() and aug.np_rng.randint(1 << 30) == nprs.randint(1 << 30)
    for name in A.RandAugmentDevice.CV:                 # every op: gates fired and not, and both sign-flip branches where there is one
        fired = {f for _, f in seen[name]}
        assert fired == {True, False}, (name, seen[name])
        if name in ("HSV", "Shift_Scale_Rotate", "Rotate_Crop"):
            assert {s for s, _ in seen[name]} == {True, False}, (name, seen[name])


def _peek(state):
    r = random.Random()
    r.setstate(state)
    return r.random()


def test_sign_flip_negates_the_level():
    """with the flip, uniform(-v, v) runs from +|v| down: the draw is v (1 - 2 r) for the flipped level, as to_tuple leaves it unsorted"""
    from ssl_cr_histo_amd import augment as A

    class Fixed:
        def __init__(self, seq):
            self.seq = list(seq)

        def random(self):
            return self.seq.pop(0)
    for first, sign in ((0.4, -1.0), (0.6, 1.0)):
        aug = A.RandAugmentDevice(1, 10, Fixed([first, 0.9, 0.1, 0.25, 0.5, 0.75]), None, cv_ops="device")
        got = aug._cv_draws("HSV", 0.8)
        v = sign * 0.8
        assert got == (True, -v + 2 * v * 0.25, -v + 2 * v * 0.5, -v + 2 * v * 0.75)


def test_cv_ops_host_still_raises_by_name_and_host_ops_win():
    from ssl_cr_histo_amd import augment as A
    with pytest.raises(ValueError):
        A.RandAugmentDevice(1, 10, random.Random(0), np.random.RandomState(0), cv_ops="gpu")
    hit = set()
    for seed in range(60):
        aug = A.RandAugmentDevice(2, 10, random.Random(seed), np.random.RandomState(seed))
        try:
            aug.plan(1)
        except NotImplementedError as e:
            name = [nm for nm in A.RandAugmentDevice.CV if f"op {nm} " in str(e)]
            assert len(name) == 1 and f"host_ops[{name[0]!r}]" in str(e)
            hit.add(name[0])
    assert hit == set(A.RandAugmentDevice.CV)
    # a name in host_ops goes to the host even with cv_ops="device": its row carries the level, not device draws
    aug = A.RandAugmentDevice(3, 10, random.Random(1), np.random.RandomState(1), host_ops={"HSV": lambda img, v: img}, cv_ops="device")
    rows = [r for row in aug.plan(40) for r in row if r[0] == "HSV"]
    assert rows and all(isinstance(r[1], float) for r in rows)
    assert not aug._on_device("HSV") and aug._on_device("Noise")


def test_cv_slot_rows():
    from ssl_cr_histo_amd import augment as A
    row = A.RandAugmentDevice.cv_slot_row
    assert row("HSV", (True, 0.5, -0.5, 0.51), (32, 32))[:2] == (A.V1_HSV, [0, 0, 1, 0])          # rint: half to even
    assert row("HSV", (False, 0.0, 0.0, 0.0), (32, 32))[0] == A.V1_COPY
    assert row("Scale_Resize_Crop", (None, 0.999, 0.0), (32, 32))[:2] == (A.V1_RESIZE, [32, 19, 0, 0])
    assert row("Scale_Resize_Crop", (1.07, 0.5, 0.26), (32, 32))[:2] == (A.V1_RESIZE, [34, 10, 5, 0])
    assert row("Rotate_Crop", (None, None), (32, 32))[0] == A.V1_COPY
    for d, want in ((0, [0, 1]), (1, [1, 0]), (-1, [1, 1])):                                      # cv2.flip codes
        code, ip, dp = row("Rotate_Crop", (d, None), (32, 32))
        assert code == A.V1_WARP and ip[:2] == want and dp == [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]
    code, ip, dp = row("Shift_Scale_Rotate", (True, 30.0, 0.8, 0.05, -0.02), (32, 32))
    m = R.rotation_matrix(16.0, 16.0, 30.0, 0.8)
    m[2] += 0.05 * 32
    m[5] += -0.02 * 32
    assert code == A.V1_WARP and dp == R.invert_affine(m)
    assert row("Noise", (True, 3.5, (7 << 32) | 9), (32, 32)) == (A.V1_NOISE, [9, 7, 0, 0], [3.5, 0, 0, 0, 0, 0])
    assert row("Blur_img", (True, 5), (32, 32))[:2] == (A.V1_BLUR, [5, 0, 0, 0])


class _FakeCuda:
    """what the plan-time checks read of a batch: they run before anything touches the device"""
    is_cuda, dtype = True, torch.uint8

    def __init__(self, shape):
        self.shape, self.device = shape, torch.device("cpu")

    def is_contiguous(self):
        return True

    def dim(self):
        return len(self.shape)


def test_plan_time_refusals():
    from ssl_cr_histo_amd import augment as A
    with pytest.raises(ValueError, match="square"):
        A.cv_scale_resize_crop(_FakeCuda((2, 3, 24, 40)), [1.0, 1.0], [(0, 0), (0, 0)])
    with pytest.raises(ValueError, match="intermediate size 0"):
        A.cv_scale_resize_crop(_FakeCuda((1, 3, 8, 8)), [0.1], [(0, 0)])
    with pytest.raises(ValueError, match="origin"):
        A.cv_scale_resize_crop(_FakeCuda((1, 3, 8, 8)), [1.0], [(21, 0)])
    with pytest.raises(ValueError, match="kernel size"):
        A.cv_blur(_FakeCuda((1, 3, 8, 8)), [4])
    with pytest.raises(ValueError, match="16-bit"):
        A.cv_warp_affine(_FakeCuda((1, 3, 8, 8)), [[1e-6, 0, 0, 0, 1e-6, 0]])
    with pytest.raises(ValueError, match="sigma"):
        A.gaussian_noise(_FakeCuda((1, 3, 8, 8)), [-1.0], [0])
    with pytest.raises(ValueError):
        A.gaussian_noise(_FakeCuda((1, 3, 8, 8)), [1.0], [1 << 64])
    with pytest.raises(ValueError, match="uint8"):
        A.cv_blur(torch.zeros(1, 3, 8, 8, dtype=torch.uint8), [3])


def test_abi_symbols_and_null_descriptors():
    from ssl_cr_histo_amd import _lib as L
    from ssl_cr_histo_amd import build
    lib = L.lib()
    new = ["sslcr_randaug_v1_slot", "sslcr_cv_warp_table", "sslcr_augv1_workspace_bytes", "sslcr_augv1_philox"]
    for name in new:
        assert name in build.header_symbols() and name in L.SIGNATURES and hasattr(lib, name)
    assert lib.sslcr_version() == 16
    assert lib.sslcr_randaug_v1_slot(None, None) == -1
    assert lib.sslcr_randaug_v1_slot(L.AugV1Desc(), None) == -1 and b"null" in lib.sslcr_last_error()
    F = 0x7F0000010000
    d = L.AugV1Desc(src=F, dst=F + 4096, op=F, N=1, H=8, W=8)
    for mask, field in ((1 << 1, b"iparam"), (1 << 6, b"unknown op")):
        d.ops_mask = mask
        assert lib.sslcr_randaug_v1_slot(d, None) == -1 and field in lib.sslcr_last_error()
    d.ops_mask, d.iparam = 1 << 3, F
    assert lib.sslcr_randaug_v1_slot(d, None) == -1 and b"dparam" in lib.sslcr_last_error()
    d.dparam = F
    assert lib.sslcr_randaug_v1_slot(d, None) == -1 and b"wtab" in lib.sslcr_last_error()
    d.ops_mask = 1 << 4
    assert lib.sslcr_randaug_v1_slot(d, None) == -1 and b"workspace" in lib.sslcr_last_error()
    d.dst = F
    assert lib.sslcr_randaug_v1_slot(d, None) == -1 and b"aliases" in lib.sslcr_last_error()
    assert lib.sslcr_cv_warp_table(None) == -1
    assert lib.sslcr_augv1_philox(0, 0, 4, None, None) == -1
    assert lib.sslcr_augv1_workspace_bytes(0, 32, 1.2) == 0 and lib.sslcr_augv1_workspace_bytes(2, 32, 0.0) == 0
    assert lib.sslcr_augv1_workspace_bytes(2, 32, 1.2) == 2 * ((3 * 38 * 38 + 15) // 16 * 16)
    assert ctypes.sizeof(L.AugV1Desc) % 8 == 0
    for k, name in enumerate(L.AUGV1_OPS):
        assert build.header_defines()["SSLCR_AUGV1_" + name.upper()] == k
