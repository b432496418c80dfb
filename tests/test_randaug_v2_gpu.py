"""GPU: the HIP kernels of the RSP v2 device RandAugment (csrc/augment_v2.hip) against the goldens recorded from the reference's own
Pillow op functions and against the NumPy restatement (tests/_pil_ref.py).  The bound is EQUALITY: host and device do the same IEEE
float32 / float64 / integer operations in the same order, so one differing byte is a contraction, a wrong order or a wrong branch."""
import random

import numpy as np
import pytest
import torch

import _pil_ref as R
from _randaug_v2_golden import golden

pytestmark = pytest.mark.gpu

DEVICE_OPS = [nm for nm in R.POOL if nm not in R.HOST]


def to_dev(imgs_hwc, hwc):
    t = torch.from_numpy(np.stack(imgs_hwc)).cuda()
    return t.contiguous() if hwc else t.permute(0, 3, 1, 2).contiguous()


def to_np(t, hwc):
    return (t if hwc else t.permute(0, 2, 3, 1)).contiguous().cpu().numpy()


def run_family(batch, name, vals, signs, apply, hwc):
    """one op for a whole batch through the wrapper of its kernel family; (val, sign) per image, apply[n] False = unchanged"""
    from ssl_cr_histo_amd import augment as A
    if name in ("identity", "contrast", "brightness", "color", "autocontrast", "equalize"):
        return A.pil_point_ops(batch, [name if a else None for a in apply], [A.enhance_factor(v) for v in vals], hwc=hwc)
    if name == "sharpness":
        return A.pil_sharpness(batch, [A.enhance_factor(v) for v in vals], apply, hwc=hwc)
    lv = [R.signed_level(name, v, s) for v, s in zip(vals, signs)]
    if name == "rotate":
        return A.pil_rotate(batch, lv, apply, hwc=hwc)
    if name == "translate_x":
        return A.pil_translate(batch, [(p, 0.0) for p in lv], apply, hwc=hwc)
    if name == "translate_y":
        return A.pil_translate(batch, [(0.0, p) for p in lv], apply, hwc=hwc)
    coef = [(1, p, 0, 0, 1, 0) if name == "shear_x" else (1, 0, 0, p, 1, 0) for p in lv]
    return A.pil_affine_bicubic(batch, coef, apply, hwc=hwc)


@pytest.mark.parametrize("hwc", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("name", DEVICE_OPS)
def test_op_equals_golden(name, hwc):
    """per op and golden image one batch: that image once per recorded (val, sign), and masked-off copies in front, in the middle and
    behind, which come back unchanged"""
    g = golden()
    for j, img in enumerate(g.images):
        cases = [c for c in g.op_cases if c[0] == name and c[1] == j]
        assert cases
        slots = [None] + cases[:1] + [None] + cases[1:] + [None]
        vals = [c[2] if c else 1.0 for c in slots]
        signs = [(c[4] if c[4] is not None else 1) if c else 1 for c in slots]
        apply = [c is not None for c in slots]
        src = to_dev([img] * len(slots), hwc)
        got = to_np(run_family(src, name, vals, signs, apply, hwc), hwc)
        for k, c in enumerate(slots):
            want = c[5] if c else img
            assert np.array_equal(got[k], want), (name, j, k, c and c[2:5], int((got[k] != want).sum()))
        assert np.array_equal(to_np(src, hwc)[0], img)          # the source batch is left alone


def fresh_images(h, w, seed):
    """five different images of one shape: noise, a narrow range, a flat channel, ramps, and one all-equal image"""
    rs = np.random.RandomState(seed)
    a = rs.randint(0, 256, (h, w, 3))
    b = rs.randint(90, 131, (h, w, 3))
    c = rs.randint(0, 256, (h, w, 3))
    c[..., 2] = 201
    d = np.add.outer(np.arange(h) * 3, np.arange(w) * 2)[..., None] + np.array([0, 70, 150])
    e = np.full((h, w, 3), 37)
    return [x.astype(np.uint8) for x in (a, b, c, d, e)]


# (23, 37): odd, H*W no multiple of 16 (byte path, ragged last unit).  (96, 80): 7680 pixels = 480 units of 16, two workgroups per image
# in the statistics pass and the apply pass.  (160, 128): 20480 pixels, five workgroups per image.  All but the first take the 16-byte path.
SHAPES = [(23, 37), (96, 80), (160, 128)]
_REF = {}


def restated(name, shape):
    """-> (images, vals, signs, apply, expected); computed once per (op, shape) and shared by the two layouts"""
    key = (name, shape)
    if key not in _REF:
        imgs = fresh_images(*shape, seed=100 + SHAPES.index(shape))
        rs = np.random.RandomState(7 + DEVICE_OPS.index(name))
        vals = [1.0, float(rs.uniform(1, 10)), 5.0, float(rs.uniform(5, 10)), float(rs.uniform(1, 10))]
        signs = [1, 0, 1, 0, 1]
        apply = [True, True, True, False, True]
        want = [R.apply_op(im, name, v, s) if a else im for im, v, s, a in zip(imgs, vals, signs, apply)]
        _REF[key] = (imgs, vals, signs, apply, want)
    return _REF[key]


@pytest.mark.parametrize("hwc", [False, True], ids=["nchw", "nhwc"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", DEVICE_OPS)
def test_op_equals_restatement(name, shape, hwc):
    imgs, vals, signs, apply, want = restated(name, shape)
    got = to_np(run_family(to_dev(imgs, hwc), name, vals, signs, apply, hwc), hwc)
    for k in range(len(imgs)):
        assert np.array_equal(got[k], want[k]), (name, shape, k, vals[k], signs[k], int((got[k] != want[k]).sum()))


def test_general_affine_and_two_axis_translate():
    """what the pool never asks for but the entry serves: a translate in both axes, a full 6-coefficient bicubic map, large angles"""
    from ssl_cr_histo_amd import augment as A
    imgs = fresh_images(40, 56, seed=9)[:4]
    for hwc in (False, True):
        src = to_dev(imgs, hwc)
        pix = [(3.25, -7.5), (-60.0, 1.0), (0.49999, 0.5), (-0.5, 39.6)]
        got = to_np(A.pil_translate(src, pix, hwc=hwc), hwc)
        for k, (px, py) in enumerate(pix):
            assert np.array_equal(got[k], R.translate(imgs[k], px, py)), ("translate", k)
        coef = [(0.9, 0.2, -3.0, -0.15, 1.1, 2.5), (1.3, 0, 0, 0.4, 0.8, -6), (1, -0.27, 0, 0, 1, 0), (0.5, 0.5, 10, -0.5, 0.5, 20)]
        got = to_np(A.pil_affine_bicubic(src, coef, hwc=hwc), hwc)
        for k, c in enumerate(coef):
            assert np.array_equal(got[k], R.affine_bicubic(imgs[k], c)), ("bicubic", k)
        deg = [45.0, -133.7, 29.999, 271.3]
        got = to_np(A.pil_rotate(src, deg, hwc=hwc), hwc)
        for k, dg in enumerate(deg):
            assert np.array_equal(got[k], R.rotate(imgs[k], dg)), ("rotate", k)


@pytest.mark.parametrize("hwc", [False, True], ids=["nchw", "nhwc"])
def test_pipeline_goldens_through_the_class(hwc):
    from ssl_cr_histo_amd import augment as A
    g = golden()
    for n, m, j, seed, want in g.pipe_cases:
        aug = A.RandAugmentV2Device(n, m, random.Random(seed), np.random.RandomState(seed))
        out = aug(to_dev([g.images[j]], hwc), hwc=hwc)
        assert out.shape == (1, 3) + g.images[j].shape[:2] and out.dtype == torch.uint8
        assert np.array_equal(to_np(out, False)[0], want), (n, m, j, seed)


def host_free_seed(n, m, count, start):
    """the first seed from ``start`` whose ``count`` successive samples avoid hed / hsv (pure host search)"""
    seed = start
    while True:
        rng, np_rng = random.Random(seed), np.random.RandomState(seed)
        plan = [R.plan_image(rng, np_rng, n, m) for _ in range(count)]
        if not any(nm in R.HOST for row in plan for nm, _, _ in row):
            return seed
        seed += 1


def test_mixed_batch_through_the_class_and_determinism():
    """a batch in which the images of one slot take different ops of every family, NHWC in and NCHW out; one 256 x 256 image rides along
    in a batch of its own (16 workgroups per image).  Two runs of the same seeded batch are bit-identical."""
    from ssl_cr_histo_amd import augment as A
    for shape, count, start in (((96, 80), 10, 0), ((256, 256), 1, 50)):
        rs = np.random.RandomState(shape[0])
        imgs = [rs.randint(0, 256, shape + (3,)).astype(np.uint8) for _ in range(count)]
        seed = host_free_seed(3, 10, count, start)
        src = to_dev(imgs, True)
        outs = []
        for _ in range(2):
            aug = A.RandAugmentV2Device(3, 10, random.Random(seed), np.random.RandomState(seed))
            outs.append(aug(src))
        assert torch.equal(outs[0], outs[1])
        rng, np_rng = random.Random(seed), np.random.RandomState(seed)
        got = to_np(outs[0], False)
        for k, im in enumerate(imgs):
            assert np.array_equal(got[k], R.randaugment(im, rng, np_rng, 3, 10)), (shape, k)


def test_triplet_wrapper_equals_sequential_tiles():
    from ssl_cr_histo_amd import augment as A
    N, shape = 4, (32, 40)
    rs = np.random.RandomState(11)
    tiles = [[rs.randint(0, 256, shape + (3,)).astype(np.uint8) for _ in range(N)] for _ in range(3)]
    seed = host_free_seed(2, 10, 3 * N, 0)
    t = A.TripletRandAugmentV2(2, 10, random.Random(seed), np.random.RandomState(seed))
    got = [to_np(o, False) for o in t(*(to_dev(d, True) for d in tiles))]
    rng, np_rng = random.Random(seed), np.random.RandomState(seed)
    for i in range(N):                      # TensorDataset_Transform.__getitem__: D1, D2, D3 of one triplet, then the next triplet
        for k in range(3):
            assert np.array_equal(got[k][i], R.randaugment(tiles[k][i], rng, np_rng, 2, 10)), (i, k)


def test_host_ops_and_their_absence():
    from ssl_cr_histo_amd import augment as A
    img = fresh_images(24, 32, seed=1)[0]
    src = to_dev([img, img], False)
    with pytest.raises(NotImplementedError, match="hed|hsv"):
        A.RandAugmentV2Device(14, 10, random.Random(0), np.random.RandomState(0))(src)
    # with host ops the two images make the round trip through host memory for those slots; everything else stays on the device
    seen = []

    def host(im, val):
        seen.append((im.shape, im.dtype))
        return 255 - im
    seed = 3
    aug = A.RandAugmentV2Device(14, 10, random.Random(seed), np.random.RandomState(seed), host_ops={"hed": host, "hsv": host})
    got = to_np(aug(src), False)
    assert seen == [((24, 32, 3), np.uint8)] * 4
    rng, np_rng = random.Random(seed), np.random.RandomState(seed)
    for k in range(2):
        want = img
        for name, val, sign in R.plan_image(rng, np_rng, 14, 10):
            want = 255 - want if name in R.HOST else R.apply_op(want, name, val, sign)
        assert np.array_equal(got[k], want), k


def test_wrapper_rejects_bad_arguments():
    from ssl_cr_histo_amd import augment as A
    src = to_dev(fresh_images(8, 8, seed=2)[:2], False)
    with pytest.raises(ValueError):
        A.randaug_v2_slot(src, [A.V2_BICUBIC, A.V2_COPY])                 # no coefficient table
    with pytest.raises(ValueError):
        A.randaug_v2_slot(src, [A.V2_COPY])                               # one code per image
    with pytest.raises(ValueError):
        A.randaug_v2_slot(src.float(), [A.V2_COPY, A.V2_COPY])
    from ssl_cr_histo_amd import _lib as L
    with pytest.raises(L.SslcrError, match="aliases"):
        A.randaug_v2_slot(src, [A.V2_COPY, A.V2_COPY], out=src)
