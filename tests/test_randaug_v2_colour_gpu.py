"""GPU: the hed / hsv kernels of the RSP v2 device RandAugment (csrc/augment_v2.hip, sslcr_randaug_v2_colour) against the NumPy
restatement of tests/_colour_ref.py.  hsv is float64 with correctly rounded operations only: the bound is EQUALITY.  hed goes
through logf / expf in float32: every byte must lie inside its own admissible set (tests/_colour_ref.py derives it), no element excused."""
import random

import numpy as np
import pytest
import torch

import _colour_ref as CR
import _pil_ref as R

pytestmark = pytest.mark.gpu

SMALL, LARGE = (33, 37), (256, 256)          # 1221 pixels: a multiple of neither 4 nor 16 (byte path, ragged last unit); 64 workgroups


def to_dev(imgs_hwc, hwc):
    t = torch.from_numpy(np.stack(imgs_hwc)).cuda()
    return t.contiguous() if hwc else t.permute(0, 3, 1, 2).contiguous()


def to_np(t, hwc):
    return (t if hwc else t.permute(0, 2, 3, 1)).contiguous().cpu().numpy()


def patched(h, w, seed):
    """a tissue-like tile with a black patch, a grey patch and patches in which two channels tie (as maximum, as minimum)"""
    im = CR.tissue(h, w, seed)
    im[1:5, 2:9] = 0
    im[6:9, 3:12] = im[6:9, 3:12, :1]
    im[10:14, 1:8, 1] = im[10:14, 1:8, 0] = np.maximum(im[10:14, 1:8, 0], im[10:14, 1:8, 2])
    im[15:19, 4:11, 2] = im[15:19, 4:11, 1] = np.minimum(im[15:19, 4:11, 1], im[15:19, 4:11, 0])
    im[20:23, 0:6] = (255, 255, 0)
    return im


_HSV, _HED = {}, {}


def hsv_case(shape):
    """-> (images, names, params, expected), computed once and shared by the two layouts"""
    if shape not in _HSV:
        h, w = shape
        if shape == SMALL:
            rs = np.random.RandomState(3)
            grey = np.repeat(rs.randint(0, 256, (h, w, 1)), 3, axis=2).astype(np.uint8)
            imgs = [patched(h, w, 1), patched(h, w, 2), CR.tissue(h, w, 3), rs.randint(0, 256, (h, w, 3)).astype(np.uint8), grey, patched(h, w, 4)]
            names = ["hsv", "hsv", None, "hsv", "hsv", "hsv"]
            params = [(0.21, 0.17, 0.0), (-0.13, -0.22, 0.0), None, (0.0, 0.3, 0.0), (0.3, -0.3, 0.0), (-0.29, 0.0, 0.0)]
        else:
            imgs, names, params = [patched(h, w, 9)], ["hsv"], [(-0.077, 0.26, 0.0)]
        want = [CR.hsv(im, *p) if nm else im for im, nm, p in zip(imgs, names, params)]
        _HSV[shape] = (imgs, names, params, want)
    return _HSV[shape]


@pytest.mark.parametrize("hwc", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("shape", [SMALL, LARGE], ids=lambda s: f"{s[0]}x{s[1]}")
def test_hsv_equals_restatement(shape, hwc):
    from ssl_cr_histo_amd import augment as A
    imgs, names, params, want = hsv_case(shape)
    src = to_dev(imgs, hwc)
    got = to_np(A.pil_colour_ops(src, names, params, hwc=hwc), hwc)
    for k in range(len(imgs)):
        assert np.array_equal(got[k], want[k]), (shape, k, params[k], int((got[k] != want[k]).sum()))
    assert np.array_equal(to_np(src, hwc), np.stack(imgs))             # out=None works on a copy
    again = A.pil_colour_ops(src, names, params, hwc=hwc, out=src)     # out=batch: in place
    assert again is src and np.array_equal(to_np(src, hwc), np.stack(want))


def with_sum(h, w, total, seed):
    """an image whose 3 h w bytes sum to ``total``"""
    n = 3 * h * w
    base, rest = divmod(int(total), n)
    flat = np.full(n, base, np.int64)
    flat[np.random.RandomState(seed).permutation(n)[:rest]] += 1
    assert flat.sum() == total and flat.max() <= 255
    return flat.reshape(h, w, 3).astype(np.uint8)


def hed_case(shape):
    """-> (images, names, params, lo, hi, (two-valued fraction, unsaturated fraction) over the images the op applies to)"""
    if shape not in _HED:
        h, w = shape
        if shape == SMALL:
            rs = np.random.RandomState(21)
            dark = np.clip(rs.normal(30, 6, (h, w, 3)), 0, 255).astype(np.uint8)
            bright = np.clip(rs.normal(235, 6, (h, w, 3)), 0, 255).astype(np.uint8)
            imgs = [CR.tissue(h, w, 11), dark, bright, CR.tissue(h, w, 12), patched(h, w, 13), CR.tissue(h, w, 14)]
            names = ["hed", "hed", "hed", None, "hed", "hed"]
            params = [tuple(rs.uniform(-f, f, 6)) for f in (0.1, 0.2, 0.2, 0.1, 0.3, 0.03)]
            assert dark.mean() < 0.15 * 255 and bright.mean() > 0.85 * 255
        else:
            imgs, names, params = [CR.tissue(h, w, 15)], ["hed"], [tuple(np.random.RandomState(22).uniform(-0.15, 0.15, 6))]
        lo, hi, two, unsat, cnt = [], [], 0.0, 0.0, 0
        for im, nm, p in zip(imgs, names, params):
            if nm is None:
                lo.append(im), hi.append(im)
                continue
            l, u, Y, _ = CR.hed_bound(im, p)
            lo.append(l), hi.append(u)
            if CR.hed_applies(im):
                t, s = CR.bound_stats(l, u, Y)
                two, unsat, cnt = two + t * im.size, unsat + s * im.size, cnt + im.size
        _HED[shape] = (imgs, names, params, lo, hi, (two / cnt, unsat / cnt))
    return _HED[shape]


def inside(got, lo, hi):
    return int(((got < lo) | (got > hi)).sum())


@pytest.mark.parametrize("hwc", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("shape", [SMALL, LARGE], ids=lambda s: f"{s[0]}x{s[1]}")
def test_hed_inside_its_bound(shape, hwc):
    """every byte admissible; the dark and the bright image (outside the cutoff) and the COPY image bit-identical.  The sets are tight
    (<= 1 % of the bytes two-valued) and the inputs exercise them (>= half unsaturated) on the images the op applies to."""
    from ssl_cr_histo_amd import augment as A
    imgs, names, params, lo, hi, (two, unsat) = hed_case(shape)
    print(f"hed {shape}: {100 * two:.3f} % two-valued, {100 * unsat:.1f} % unsaturated")
    assert two <= 0.01 and unsat >= 0.5
    got = to_np(A.pil_colour_ops(to_dev(imgs, hwc), names, params, hwc=hwc), hwc)
    for k in range(len(imgs)):
        assert inside(got[k], lo[k], hi[k]) == 0, (shape, k, inside(got[k], lo[k], hi[k]))
        if names[k] is None or not CR.hed_applies(imgs[k]):
            assert np.array_equal(got[k], imgs[k]), k
        else:
            assert not np.array_equal(got[k], imgs[k]), k


@pytest.mark.parametrize("hwc", [False, True], ids=["nchw", "nhwc"])
def test_hed_cutoff_at_the_thresholds(hwc):
    """images whose byte sum lies a few counts either side of 0.15 * 255 * (3 H W) and of 0.85 * 255 * (3 H W): the integer sum and the
    float64 compare decide as np.mean(patch) / 255.0 does"""
    from ssl_cr_histo_amd import augment as A
    h, w = SMALL
    n = 3 * h * w
    imgs, expect = [], []
    for thr in CR.CUTOFF:
        edge = int(np.floor(thr * 255.0 * n))
        for k, off in enumerate((-3, -1, 0, 1, 2, 4)):
            imgs.append(with_sum(h, w, edge + off, 30 + k))
            expect.append(CR.hed_applies(imgs[-1]))
    assert expect[0] != expect[5] and expect[6] != expect[11]            # both thresholds are crossed
    p = (0.11, -0.07, 0.05, 0.04, -0.06, 0.02)
    got = to_np(A.pil_colour_ops(to_dev(imgs, hwc), ["hed"] * len(imgs), [p] * len(imgs), hwc=hwc), hwc)
    for k, im in enumerate(imgs):
        if expect[k]:
            lo, hi, _, _ = CR.hed_bound(im, p)
            assert inside(got[k], lo, hi) == 0 and not np.array_equal(got[k], im), k
        else:
            assert np.array_equal(got[k], im), k


def test_hed_without_edits_is_the_identity_round_trip():
    """all sigmas and biases 0: inside the bound, whose Y is the input byte up to rounding -- so every byte is the input or one below"""
    from ssl_cr_histo_amd import augment as A
    imgs = [CR.tissue(*SMALL, 17), patched(*SMALL, 18)]
    got = to_np(A.pil_colour_ops(to_dev(imgs, True), ["hed"] * 2, [(0.0,) * 6] * 2, hwc=True), True)
    for k, im in enumerate(imgs):
        lo, hi, Y, _ = CR.hed_bound(im, (0.0,) * 6)
        assert inside(got[k], lo, hi) == 0, k
        d = im.astype(np.int64) - got[k]
        assert d.min() >= 0 and d.max() <= 1, (k, d.min(), d.max())


# ------------------------------------------------------------------------------------------------ through the class
def check_chain(imgs, rows, final, prefix, host=None):
    """slot by slot: tests/_pil_ref.apply_op for the Pillow ops, the restatement for hsv -- byte-exact -- and for a hed slot the device's
    own output of that slot against the bound, the chain restarting from it (a byte step does not propagate exactly).
    prefix(k) -> the device's batch after the first k slots."""
    for i, (im, row) in enumerate(zip(imgs, rows)):
        cur = im
        for s, (name, val, third) in enumerate(row):
            if host and name in host:
                cur = host[name](cur, val)
            elif name == "hed":
                if s:
                    assert np.array_equal(prefix(s)[i], cur), (i, s, "before hed")
                dev = prefix(s + 1)[i]
                lo, hi, _, _ = CR.hed_bound(cur, third)
                assert inside(dev, lo, hi) == 0, (i, s, inside(dev, lo, hi))
                cur = dev
            elif name == "hsv":
                cur = CR.hsv(cur, *third)
            else:
                cur = R.apply_op(cur, name, val, third)
        assert np.array_equal(final[i], cur), (i, [nm for nm, _, _ in row])


def prefix_runner(src, rows, hwc, host_ops=None):
    from ssl_cr_histo_amd import augment as A
    cache = {}

    def prefix(k):
        if k not in cache:
            aug = A.RandAugmentV2Device(k, 10, None, None, host_ops=host_ops, colour_ops="device")
            cache[k] = to_np(aug.run(src, [row[:k] for row in rows], hwc), False)
        return cache[k]
    return prefix


def no_transfer(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("run() must not leave the device")
    monkeypatch.setattr(torch.Tensor, "cpu", boom)
    monkeypatch.setattr(torch.cuda, "synchronize", boom)


def run_twice(src, n, seed, hwc, monkeypatch):
    """two seeded runs of the class, run() under a Tensor.cpu / synchronize that raise -> (plan rows, result as numpy)"""
    from ssl_cr_histo_amd import augment as A
    outs = []
    for _ in range(2):
        aug = A.RandAugmentV2Device(n, 10, random.Random(seed), np.random.RandomState(seed), colour_ops="device")
        plan = aug.plan(src.shape[0])
        with monkeypatch.context() as mp:
            no_transfer(mp)
            outs.append(aug.run(src, plan, hwc))
    assert torch.equal(outs[0], outs[1])
    assert outs[0].shape[1] == 3 and outs[0].dtype == torch.uint8
    return plan, to_np(outs[0], False)


def test_whole_pool_through_the_class(monkeypatch):
    """n = 14 on a 24 x 32 pair: every image meets both ops, at the slots its sample puts them"""
    imgs = [CR.tissue(24, 32, 51), patched(24, 32, 52)]
    src = to_dev(imgs, False)
    seed = 5
    plan, got = run_twice(src, 14, seed, False, monkeypatch)
    rng, np_rng = random.Random(seed), np.random.RandomState(seed)
    assert plan == [CR.plan_image(rng, np_rng, 14, 10) for _ in imgs]
    check_chain(imgs, plan, got, prefix_runner(src, plan, False))


def colour_seed(n, count, start):
    """the first seed from ``start`` whose ``count`` samples hold at least two hed and two hsv (pure host search)"""
    seed = start
    while True:
        rng, np_rng = random.Random(seed), np.random.RandomState(seed)
        names = [nm for _ in range(count) for nm, _, _ in CR.plan_image(rng, np_rng, n, 10)]
        if names.count("hed") >= 2 and names.count("hsv") >= 2:
            return seed
        seed += 1


def test_mixed_batch_through_the_class(monkeypatch):
    """ten 96 x 80 images, n = 3, NHWC in and NCHW out: in one slot the images take Pillow ops of every family, hed, hsv"""
    imgs = [CR.tissue(96, 80, 60 + k) if k % 2 else patched(96, 80, 60 + k) for k in range(10)]
    src = to_dev(imgs, True)
    seed = colour_seed(3, 10, 0)
    plan, got = run_twice(src, 3, seed, None, monkeypatch)
    check_chain(imgs, plan, got, prefix_runner(src, plan, True))


def test_host_ops_take_precedence():
    from ssl_cr_histo_amd import augment as A
    imgs = [CR.tissue(24, 32, 71), patched(24, 32, 72)]
    src = to_dev(imgs, False)
    seen = []

    def host(im, val):
        seen.append((im.shape, im.dtype))
        return 255 - im
    seed = 3
    aug = A.RandAugmentV2Device(14, 10, random.Random(seed), np.random.RandomState(seed), host_ops={"hed": host}, colour_ops="device")
    plan = aug.plan(2)
    got = to_np(aug.run(src, plan), False)
    assert seen == [((24, 32, 3), np.uint8)] * 2
    assert all(t is None for row in plan for nm, _, t in row if nm == "hed")
    check_chain(imgs, plan, got, None, host={"hed": lambda im, val: 255 - im})      # no hed on the device: the whole chain is byte-exact


def test_triplet_wrapper_equals_sequential_tiles():
    from ssl_cr_histo_amd import augment as A
    N, shape = 4, (32, 40)
    tiles = [[CR.tissue(*shape, 80 + 10 * k + i) for i in range(N)] for k in range(3)]
    seed = colour_seed(2, 3 * N, 0)
    t = A.TripletRandAugmentV2(2, 10, random.Random(seed), np.random.RandomState(seed), colour_ops="device")
    srcs = [to_dev(d, True) for d in tiles]
    got = [to_np(o, False) for o in t(*srcs)]
    rng, np_rng = random.Random(seed), np.random.RandomState(seed)
    plan = [CR.plan_image(rng, np_rng, 2, 10) for _ in range(3 * N)]      # the dataset's order: D1, D2, D3 of one triplet, then the next
    for k in range(3):
        check_chain(tiles[k], plan[k::3], got[k], prefix_runner(srcs[k], plan[k::3], True))


def test_code_without_its_mask_bit_is_a_copy():
    """the raw entry with op[n] = HED / HSV but an ops_mask that lacks the bit, and no bsum: nothing is read through NULL, nothing changes"""
    from ssl_cr_histo_amd import _lib as L
    from ssl_cr_histo_amd import augment as A
    imgs = [CR.tissue(*SMALL, 91), CR.tissue(*SMALL, 92), CR.tissue(*SMALL, 93)]
    src = to_dev(imgs, False)
    t_op = torch.tensor([A.V2C_HED, A.V2C_HSV, A.V2C_HSV], dtype=torch.int32, device="cuda")
    rows = [A.colour_param_row("hed", (0.1,) * 6), A.colour_param_row("hsv", (0.2, 0.2, 0.0)), A.colour_param_row("hsv", (0.2, 0.2, 0.0))]
    t_p = torch.tensor(rows, dtype=torch.float64, device="cuda")
    inv, fwd = A.v2_hed_matrices()
    for mask, changed in ((1 << A.V2C_COPY, ()), (1 << A.V2C_HSV, (1, 2))):
        work = src.clone()
        d = L.AugV2ColourDesc(L.ptr(work), L.ptr(t_op), L.ptr(t_p), None, 0.15, 0.85, (L.f32 * 9)(*inv.reshape(-1).tolist()),
                              (L.f32 * 9)(*fwd.reshape(-1).tolist()), mask, 3, SMALL[0], SMALL[1], 0)
        L.check(L.lib().sslcr_randaug_v2_colour(d, L.stream_ptr()))
        got = to_np(work, False)
        for k, im in enumerate(imgs):
            want = CR.hsv(im, 0.2, 0.2) if k in changed else im
            assert np.array_equal(got[k], want), (mask, k)


def test_wrapper_rejects_bad_arguments():
    from ssl_cr_histo_amd import augment as A
    src = to_dev([CR.tissue(8, 8, 1), CR.tissue(8, 8, 2)], False)
    with pytest.raises(ValueError):
        A.pil_colour_ops(src, ["hed"], [(0.0,) * 6])                       # one name per image
    with pytest.raises(ValueError):
        A.pil_colour_ops(src, ["hed", "color"], [(0.0,) * 6, None])        # not a colour op
    with pytest.raises(ValueError):
        A.pil_colour_ops(src, ["hed", None], [(0.0,) * 5, None])           # six draws
    with pytest.raises(ValueError):
        A.pil_colour_ops(src.float(), [None, None], [None, None])
    for ws in (torch.empty(2, dtype=torch.int32, device="cuda"), torch.empty(1, dtype=torch.int64, device="cuda"), torch.empty(2, dtype=torch.int64)):
        with pytest.raises(ValueError, match="workspace"):
            A.pil_colour_ops(src, ["hed", None], [(0.0,) * 6, None], workspace=ws)
    out = A.pil_colour_ops(src, [None, None], [None, None])                # nothing to do: a copy, no launch
    assert out is not src and torch.equal(out, src)
