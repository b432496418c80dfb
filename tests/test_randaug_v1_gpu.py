"""The six OpenCV-style ops of the v1 RandAugment pool on the device (sslcr_randaug_v1_slot, csrc/augment_v1.hip) against the NumPy
restatement of the arithmetic include/sslcr.h defines (tests/_cv_ref.py): EQUALITY -- the ops are integer, or float32 with + - x in
a fixed order -- except the Gaussian noise, whose log / cos / sin are the device's: equal wherever the float64 sigma z lies farther
than 1e-3 from a half-integer, within one inside that band.  Every shape runs with HWC and CHW on both sides."""
import itertools
import random

import numpy as np
import pytest
import torch

import _cv_ref as R

pytestmark = pytest.mark.gpu

SHAPES = [(1, 8, 8), (3, 24, 40), (2, 27, 33), (5, 32, 32)]
LAYOUTS = [(False, False), (True, True), (True, False), (False, True)]
DEV = "cuda"


def _batch(seed, n, h, w):
    """uint8 [N, H, W, 3]: noise, with a strip of the colours the HSV arithmetic branches on"""
    x = np.random.RandomState(seed).randint(0, 256, (n, h, w, 3)).astype(np.uint8)
    special = [(0, 0, 0), (255, 255, 255), (128, 128, 128), (7, 7, 7),                                   # v = 0 and greys: diff = 0
               (255, 0, 0), (255, 255, 0), (0, 255, 0), (0, 255, 255), (0, 0, 255), (255, 0, 255),      # the sector corners
               (200, 90, 30), (120, 200, 30), (30, 200, 120), (30, 90, 200), (120, 30, 200), (200, 30, 120),      # one per sector
               (255, 0, 4), (255, 0, 1), (255, 1, 0), (250, 3, 0), (9, 9, 8), (1, 0, 0)]               # h at 179 / 0 and the wrap
    for i, c in enumerate(special):
        x[:, (i // w) % h, i % w] = c
    return x


def _to_dev(x, hwc):
    t = torch.from_numpy(x).to(DEV)
    return t.contiguous() if hwc else t.permute(0, 3, 1, 2).contiguous()


def _to_np(t, hwc):
    return (t if hwc else t.permute(0, 2, 3, 1)).cpu().numpy()


def _chunks(cases, n):
    """the cases in calls of n images (the last call is filled from the front)"""
    out = []
    for i in range(0, len(cases), n):
        c = cases[i:i + n]
        out.append(c + cases[:n - len(c)])
    return out


@pytest.mark.parametrize("shape", SHAPES)
def test_blur(shape):
    from ssl_cr_histo_amd import augment as A
    n, h, w = shape
    x = _batch(1, n, h, w)
    cases = [(k, ap) for k in (3, 5, 7) for ap in (True, False)]       # on 8x8 the 7-tap window reflects past the far border
    for j, call in enumerate(_chunks(cases, n)):
        for src_hwc, dst_hwc in LAYOUTS if j == 0 else [LAYOUTS[j % 4]]:
            got = _to_np(A.cv_blur(_to_dev(x, src_hwc), [k for k, _ in call], [ap for _, ap in call], hwc=src_hwc, out_hwc=dst_hwc), dst_hwc)
            for i, (k, ap) in enumerate(call):
                assert np.array_equal(got[i], R.blur(x[i], k) if ap else x[i]), (shape, k, ap, src_hwc, dst_hwc)


@pytest.mark.parametrize("shape", SHAPES)
def test_shift_hsv(shape):
    from ssl_cr_histo_amd import augment as A
    n, h, w = shape
    x = _batch(2, n, h, w)
    cases = list(itertools.product((-1, 0, 1), repeat=3))
    for j, call in enumerate(_chunks(cases, n)):
        src_hwc, dst_hwc = LAYOUTS[j % 4]
        apply = [(j + i) % 5 != 0 for i in range(n)]
        # the draws are floats: +-0.6 rounds to +-1, +-0.4 to 0
        draws = [[0.6 * s + 0.4 * (1 - abs(s)) * (1 if i % 2 else -1) for s in c] for i, c in enumerate(call)]
        got = _to_np(A.cv_shift_hsv(_to_dev(x, src_hwc), draws, apply, hwc=src_hwc, out_hwc=dst_hwc), dst_hwc)
        for i, c in enumerate(call):
            assert np.array_equal(got[i], R.shift_hsv(x[i], *c) if apply[i] else x[i]), (shape, c, src_hwc, dst_hwc)


def _warp_cases(h, w):
    from ssl_cr_histo_amd import augment as A
    hw = (h, w)
    forward = [[1.0, 0.0, 0.0, 0.0, 1.0, 0.0]] + [A.rotation_matrix(hw, a) for a in (90.0, -90.0, 45.0, 0.3)] + \
              [A.rotation_matrix(hw, 30.0, 0.4), A.rotation_matrix(hw, -20.0, 1.6),
               A.rotation_matrix(hw, 10.0, 1.0, 0.1, -0.1), A.rotation_matrix(hw, 0.0, 0.9, -0.1, 0.1)]
    return [(m, f) for m in forward for f in ((0, 0), (1, 0), (0, 1), (1, 1))]


@pytest.mark.parametrize("shape", SHAPES)
def test_warp_affine(shape):
    from ssl_cr_histo_amd import augment as A
    n, h, w = shape
    x = _batch(3, n, h, w)
    tab = R.warp_table()
    for j, call in enumerate(_chunks(_warp_cases(h, w), n)):
        src_hwc, dst_hwc = LAYOUTS[j % 4]
        apply = [(j + i) % 7 != 3 for i in range(n)]
        got = _to_np(A.cv_warp_affine(_to_dev(x, src_hwc), [m for m, _ in call], [f for _, f in call], apply, hwc=src_hwc, out_hwc=dst_hwc), dst_hwc)
        for i, (m, f) in enumerate(call):
            want = R.warp_affine(x[i], R.invert_affine(m), f[0], f[1], tab) if apply[i] else x[i]
            assert np.array_equal(got[i], want), (shape, j, i, m, f, src_hwc, dst_hwc)
    if h == w == 8:      # scale 0.4 on the small image reads 10 pixels past the border: more than one reflection
        X, _ = R.warp_coords(R.invert_affine(A.rotation_matrix((8, 8), 30.0, 0.4)), 8, 8)
        assert (X >> 5).min() - 1 < -7 or (X >> 5).max() + 2 > 14


@pytest.mark.parametrize("shape", [(1, 8, 8), (5, 32, 32)])
def test_scale_resize_crop(shape):
    from ssl_cr_histo_amd import augment as A
    n, s, _ = shape
    x = _batch(4, n, s, s)
    # S' in {1, S, int(1.92 S)}, the scale gate not fired (None), origins (0, 0) and (20, 20)
    cases = [(sc, o) for sc in (1.0 / s + 1e-9, 1.0, 1.92, None) for o in ((0, 0), (20, 20), (7, 13))]
    for j, call in enumerate(_chunks(cases, n)):
        src_hwc, dst_hwc = LAYOUTS[j % 4]
        apply = [(j + i) % 6 != 5 for i in range(n)]
        got = _to_np(A.cv_scale_resize_crop(_to_dev(x, src_hwc), [sc for sc, _ in call], [o for _, o in call], apply, hwc=src_hwc, out_hwc=dst_hwc), dst_hwc)
        for i, (sc, o) in enumerate(call):
            s1 = s if sc is None else int(s * sc)
            assert s1 in (1, s, int(1.92 * s))
            want = R.scale_resize_crop(x[i], s1, o[0], o[1]) if apply[i] else x[i]
            assert np.array_equal(got[i], want), (shape, sc, o, src_hwc, dst_hwc)


def _noise_band(x, sigma, seed):
    want, sz = R.gaussian_noise(x, sigma, seed)
    return want, np.abs((sz - np.floor(sz)) - 0.5) < 1e-3


def _check_noise(got, x, sigma, seed, tally):
    """tally: [pixels in the band, pixels] over the test; the caller holds it to the 0.5 % cap"""
    want, band = _noise_band(x, sigma, seed)
    tally[0] += int(band.sum())
    tally[1] += band.size
    diff = np.abs(got.astype(int) - want.astype(int)).max(-1)
    assert (diff[~band] == 0).all(), (sigma, seed, int((diff[~band] != 0).sum()))
    assert (diff[band] <= 1).all()


def test_philox_words():
    from ssl_cr_histo_amd import augment as A
    for seed, first, count in ((0, 0, 1), (0x0123456789ABCDEF, 0, 300), ((1 << 64) - 1, 0xFFFFFFF0, 32)):
        got = A.philox_words(seed, count, torch.device(DEV), first).cpu().numpy()
        want = R.philox4x32((np.arange(count, dtype=np.uint64) + np.uint64(first)) & np.uint64(0xFFFFFFFF), seed)
        assert np.array_equal(got, want.astype(np.int64)), seed
    assert [int(v) for v in A.philox_words(0, 1, torch.device(DEV))[0]] == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]


@pytest.mark.parametrize("shape", SHAPES)
def test_gaussian_noise(shape):
    from ssl_cr_histo_amd import augment as A
    n, h, w = shape
    x = _batch(5, n, h, w)
    tally = [0, 0]
    for j, (src_hwc, dst_hwc) in enumerate(LAYOUTS):
        sigmas = [0.0, 3.7, 25.0, 38.25, 11.5][j % 2:][:n] if n < 4 else [0.0, 3.7, 25.0, 38.25, 11.5]
        seeds = [(0x9E3779B97F4A7C15 * (i + 1 + 10 * j)) & ((1 << 64) - 1) for i in range(n)]
        apply = [(i + j) % 4 != 3 for i in range(n)]
        got = _to_np(A.gaussian_noise(_to_dev(x, src_hwc), sigmas, seeds, apply, hwc=src_hwc, out_hwc=dst_hwc), dst_hwc)
        for i in range(n):
            if apply[i]:
                _check_noise(got[i], x[i], sigmas[i], seeds[i], tally)
            else:
                assert np.array_equal(got[i], x[i])
    assert tally[1] and tally[0] <= 0.005 * tally[1], tally      # the restatement alone keeps its inputs off the band (checked on the CPU too)


def test_mixed_codes_in_one_slot_and_black_for_a_bad_code():
    from ssl_cr_histo_amd import _lib as L
    from ssl_cr_histo_amd import augment as A
    n, s = 5, 32
    x = _batch(6, n, s, s)
    m = R.invert_affine(A.rotation_matrix((s, s), 33.0, 0.8, 0.05, -0.02))
    seed = 0xDEADBEEFCAFEF00D
    tally = [0, 0]
    for codes, apply in (([A.V1_BLUR, A.V1_HSV, A.V1_WARP, A.V1_RESIZE, A.V1_NOISE], [True] * 5),
                         ([A.V1_NOISE, A.V1_COPY, A.V1_RESIZE, A.V1_WARP, A.V1_BLUR], [True, True, False, True, False])):
        ip, dp = np.zeros((n, 4), np.int64), np.zeros((n, 6))
        for i, c in enumerate(codes):
            ip[i] = {A.V1_BLUR: [5, 0, 0, 0], A.V1_HSV: [1, -1, 1, 0], A.V1_WARP: [1, 0, 0, 0], A.V1_RESIZE: [27, 3, 20, 0],
                     A.V1_NOISE: [seed & 0xFFFFFFFF, seed >> 32, 0, 0], A.V1_COPY: [0, 0, 0, 0]}[c]
            dp[i] = m if c == A.V1_WARP else [9.25, 0, 0, 0, 0, 0]
        for src_hwc, dst_hwc in LAYOUTS:
            got = _to_np(A.randaug_v1_slot(_to_dev(x, src_hwc), codes, iparam=ip, dparam=dp, apply=apply, hwc=src_hwc, out_hwc=dst_hwc), dst_hwc)
            for i, c in enumerate(codes):
                if not apply[i] or c == A.V1_COPY:
                    assert np.array_equal(got[i], x[i])
                elif c == A.V1_NOISE:
                    _check_noise(got[i], x[i], 9.25, seed, tally)
                else:
                    want = {A.V1_BLUR: lambda a: R.blur(a, 5), A.V1_HSV: lambda a: R.shift_hsv(a, 1, -1, 1),
                            A.V1_WARP: lambda a: R.warp_affine(a, m, 1, 0), A.V1_RESIZE: lambda a: R.scale_resize_crop(a, 27, 3, 20)}[c](x[i])
                    assert np.array_equal(got[i], want), (c, src_hwc, dst_hwc)
    assert tally[0] <= 0.005 * tally[1], tally
    # an op[] entry whose bit ops_mask lacks (its tables are NULL) is written black; its neighbour is still served
    src, dst = _to_dev(x[:2], False), torch.full((2, 3, s, s), 77, dtype=torch.uint8, device=DEV)
    t_op = torch.tensor([A.V1_WARP, A.V1_BLUR], dtype=torch.int32, device=DEV)
    t_ip = torch.tensor([[0, 0, 0, 0], [3, 0, 0, 0]], dtype=torch.int32, device=DEV)
    d = L.AugV1Desc(L.ptr(src), L.ptr(dst), L.ptr(t_op), None, L.ptr(t_ip), None, None, None, 0, 1 << A.V1_BLUR, 2, s, s, 0, 0)
    L.check(L.lib().sslcr_randaug_v1_slot(d, L.stream_ptr()))
    got = _to_np(dst, False)
    assert (got[0] == 0).all() and np.array_equal(got[1], R.blur(x[1], 3))


def _band_free(payload, npix):
    z, _ = R.noise_normals(npix, payload[2])
    sz = np.float64(payload[1]) * z.astype(np.float64)
    return not (np.abs((sz - np.floor(sz)) - 0.5) < 1e-3).any()


def _pick_seed(n_img, n_ops, s):
    """the first seed whose plan holds all nine ops and, among the cv ops, every device code (COPY, a gate that did not fire, included),
    and whose Noise rows keep sigma z off the half-integer band (their device result then equals the restatement everywhere)"""
    from ssl_cr_histo_amd import augment as A
    for seed in range(2000):
        plan = A.RandAugmentDevice(n_ops, 10, random.Random(seed), np.random.RandomState(seed), cv_ops="device").plan(n_img)
        rows = [r for row in plan for r in row]
        names = {r[0] for r in rows}
        codes = {A.RandAugmentDevice.cv_slot_row(r[0], r[1], (s, s))[0] for r in rows if r[0] in A.RandAugmentDevice.CV}
        if len(names) == 9 and codes == set(range(6)) and all(_band_free(r[1], s * s) for r in rows if r[0] == "Noise" and r[1][0]):
            return seed
    raise AssertionError("no seed found")


def test_randaugment_device_equals_the_restatement_driven_by_its_plan():
    from ssl_cr_histo_amd import augment as A
    n_img, n_ops, s = 7, 3, 32
    seed = _pick_seed(n_img, n_ops, s)
    x = _batch(7, n_img, s, s)
    aug = A.RandAugmentDevice(n_ops, 10, random.Random(seed), np.random.RandomState(seed), cv_ops="device")
    plan = aug.plan(n_img)
    got = _to_np(aug.run(_to_dev(x, False), plan), False)
    tab = R.warp_table()
    for i in range(n_img):
        img = x[i]
        for name, payload in plan[i]:
            if name in A.RandAugmentDevice.CV:
                code, ip, dp = A.RandAugmentDevice.cv_slot_row(name, payload, (s, s))
                if code == A.V1_BLUR:
                    img = R.blur(img, ip[0])
                elif code == A.V1_HSV:
                    img = R.shift_hsv(img, *ip[:3])
                elif code == A.V1_WARP:
                    img = R.warp_affine(img, dp, ip[0], ip[1], tab)
                elif code == A.V1_RESIZE:
                    img = R.scale_resize_crop(img, ip[0], ip[1], ip[2])
                elif code == A.V1_NOISE:
                    img = R.gaussian_noise(img, dp[0], ip[0] | ip[1] << 32)[0]
            else:      # the three colour ops have their own tests: the device op itself, on this image alone
                t = _to_dev(img[None], False)
                if name == "Color":
                    t = A.hed_colour_augment(t, [payload])
                elif payload[0]:
                    t = A.brightness_contrast(t, [payload[1:]], [True])
                img = _to_np(t, False)[0]
        assert np.array_equal(got[i], img), (seed, i, plan[i])
    # equal seeds, equal bits
    runs = [A.RandAugmentDevice(n_ops, 10, random.Random(seed), np.random.RandomState(seed), cv_ops="device")(_to_dev(x, False)) for _ in range(2)]
    assert torch.equal(runs[0], runs[1]) and np.array_equal(_to_np(runs[0], False), got)


def test_transform_fix_device():
    from ssl_cr_histo_amd import augment as A
    x = _to_dev(_batch(8, 5, 40, 40), False)
    for n in (1, 5):
        tf = A.TransformFixDevice(32, 2, torch.Generator().manual_seed(11), random.Random(3), np.random.RandomState(3))
        weak, strong = tf(x[:n])
        assert weak.shape == strong.shape == (n, 3, 32, 32) and strong.dtype == torch.uint8
        pw, ps = A.fix_params(n, (40, 40), 32, torch.Generator().manual_seed(11))
        assert torch.equal(weak, A.weak_augment(x[:n], pw, 32))
        want = A.RandAugmentDevice(2, 10, random.Random(3), np.random.RandomState(3), cv_ops="device")(A.weak_augment(x[:n], ps, 32))
        assert torch.equal(strong, want)
    # one sample: the weak branch makes the first draws of the stream, as TransformFixWeak does
    weak, _ = A.TransformFixDevice(32, 2, torch.Generator().manual_seed(5), random.Random(0), np.random.RandomState(0))(x[:1])
    assert torch.equal(weak, A.TransformFixWeak(32, torch.Generator().manual_seed(5))(x[:1]))
