"""CPU-only checks of the RSP v2 device RandAugment: the NumPy restatement of the twelve Pillow ops (tests/_pil_ref.py) against the
goldens recorded from the reference's own op functions and against the live Pillow, the host-side planning of
``RandAugmentV2Device`` against the recorded pipeline cases, and the new C-ABI descriptor against the header."""
import os
import random

import numpy as np
import pytest

import _pil_ref as R
from _randaug_v2_golden import golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_golden_reaches_every_branch():
    g = golden()
    assert g.pool == list(R.POOL)
    assert g.pillow_version.startswith("12.2")
    names = {c[0] for c in g.op_cases}
    assert names == set(R.POOL) - set(R.HOST)
    shapes = {im.shape[:2] for im in g.images}
    assert (17, 33) in shapes and (16, 15) in shapes and all(h <= 48 and w <= 48 for h, w in shapes)
    assert any((im[..., 1] == im[0, 0, 1]).all() for im in g.images)                     # a constant channel
    assert any(im.min() >= 60 and im.max() <= 123 for im in g.images)                    # a narrow range
    for nm in R.SIGNED:
        assert {c[4] for c in g.op_cases if c[0] == nm} == {0, 1}
    f = sorted({float(R.enhance_factor(c[2])) for c in g.op_cases if c[0] == "contrast"})
    assert f[0] < 1 and 1.0 in f and f[-1] > 1
    # equalize's step is 0 on the 240-pixel image (identity LUT) and not on the others
    eq = {c[1]: (c[5] == g.images[c[1]]).all() for c in g.op_cases if c[0] == "equalize"}
    assert [j for j, same in eq.items() if same] == [j for j, im in enumerate(g.images) if im.shape[:2] == (16, 15)]


def test_restatement_equals_every_golden_op():
    g = golden()
    for name, j, val, seed, sign, want in g.op_cases:
        if sign is not None:
            assert random.Random(seed).choice([1, 0]) == sign
        got = R.apply_op(g.images[j], name, val, sign)
        assert got.dtype == np.uint8 and np.array_equal(got, want), (name, j, val, sign, int((got != want).sum()))


def test_restatement_equals_every_golden_pipeline():
    g = golden()
    for n, m, j, seed, want in g.pipe_cases:
        got = R.randaugment(g.images[j], random.Random(seed), np.random.RandomState(seed), n, m)
        assert np.array_equal(got, want), (n, m, j, seed)


def test_restatement_equals_live_pillow():
    pytest.importorskip("PIL")
    from PIL import Image, ImageEnhance, ImageOps

    def pil(img, name, val, sign):
        im = Image.fromarray(img)
        enh = {"contrast": ImageEnhance.Contrast, "brightness": ImageEnhance.Brightness, "sharpness": ImageEnhance.Sharpness,
               "color": ImageEnhance.Color}
        if name in enh:
            return np.asarray(enh[name](im).enhance(val / 10 * 1.8 + 0.1))
        if name == "autocontrast":
            return np.asarray(ImageOps.autocontrast(im))
        if name == "equalize":
            return np.asarray(ImageOps.equalize(im))
        lv = R.signed_level(name, val, sign)
        if name == "rotate":
            return np.asarray(im.rotate(angle=lv))
        a = {"translate_x": (1, 0, lv, 0, 1, 0), "translate_y": (1, 0, 0, 0, 1, lv), "shear_x": (1, lv, 0, 0, 1, 0), "shear_y": (1, 0, 0, lv, 1, 0)}[name]
        return np.asarray(im.transform(im.size, Image.AFFINE, a, Image.BICUBIC) if name.startswith("shear") else im.transform(im.size, Image.AFFINE, a))
    rs = np.random.RandomState(77)
    for h, w in ((21, 30), (40, 23), (64, 48)):
        imgs = [rs.randint(0, 256, (h, w, 3)).astype(np.uint8), rs.randint(100, 140, (h, w, 3)).astype(np.uint8)]
        for img in imgs:
            for name in R.POOL:
                if name in R.HOST or name == "identity":
                    continue
                for val in (1.0, 5.0, float(rs.uniform(1, 10)), float(rs.uniform(1, 3))):
                    for sign in ((1, 0) if name in R.SIGNED else (None,)):
                        assert np.array_equal(R.apply_op(img, name, val, sign), pil(img, name, val, sign)), (h, w, name, val, sign)


def test_device_class_plans_like_the_recorded_pipelines():
    """RandAugmentV2Device.plan consumes ``rng`` / ``np_rng`` draw for draw like the reference's RandAugment.__call__: the plan of every
    recorded whole call, executed op by op with the restatement, gives the recorded output, and both generators end in the state the
    reference's call left them in."""
    from ssl_cr_histo_amd import augment as A
    g = golden()
    for n, m, j, seed, want in g.pipe_cases:
        rng, np_rng = random.Random(seed), np.random.RandomState(seed)
        (row,) = A.RandAugmentV2Device(n, m, rng, np_rng).plan(1)
        img = g.images[j]
        for name, val, sign in row:
            img = R.apply_op(img, name, val, sign)
        assert np.array_equal(img, want), (n, m, j, seed)
        r2, n2 = random.Random(seed), np.random.RandomState(seed)
        assert R.plan_image(r2, n2, n, m) == row
        assert rng.random() == r2.random() and np_rng.uniform() == n2.uniform()
    # several images: one draw sequence, image after image
    rng, np_rng = random.Random(5), np.random.RandomState(5)
    r2, n2 = random.Random(5), np.random.RandomState(5)
    plan = A.RandAugmentV2Device(2, 10, rng, np_rng, host_ops={"hed": None, "hsv": None}).plan(7)
    assert plan == [R.plan_image(r2, n2, 2, 10) for _ in range(7)]


def test_host_side_parameters_equal_the_restatement():
    from ssl_cr_histo_amd import augment as A
    assert A.RandAugmentV2Device.POOL == R.POOL and A.RandAugmentV2Device.SIGNED == R.SIGNED
    rs = np.random.RandomState(3)
    for _ in range(50):
        v, h, w = float(rs.uniform(1, 10)), int(rs.randint(3, 300)), int(rs.randint(3, 300))
        for s in (1.0, -1.0):
            assert A.rotate_coefficients(s * v * 3, (h, w)) == R.fixed_coefficients(R.rotate_matrix(s * v * 3, w, h))
        assert np.float32(A.enhance_factor(v)) == R.enhance_factor(v)
    with pytest.raises(ValueError):
        A.rotate_coefficients(10.0, (40000, 40000))


def test_missing_host_op_is_named():
    from ssl_cr_histo_amd import augment as A
    aug = A.RandAugmentV2Device(14, 10, random.Random(0), np.random.RandomState(0))       # n = 14 samples the whole pool
    with pytest.raises(NotImplementedError, match="hed|hsv"):
        aug.plan(1)


def test_augv2_descriptor_matches_the_header_layout():
    """(size and offsets of sslcr_augv2_desc: tests/test_abi_cpu.py, for every mirror)  The op codes at the two ends of the header's list"""
    from ssl_cr_histo_amd import _lib as L
    from ssl_cr_histo_amd import augment as A
    from ssl_cr_histo_amd import build
    defs = build.header_defines()
    assert "sslcr_augv2_desc" in L.MIRRORS
    assert [defs["SSLCR_AUGV2_COPY"], defs["SSLCR_AUGV2_BICUBIC"]] == [A.V2_COPY, A.V2_BICUBIC]


def test_slot_entry_checks_arguments_without_gpu():
    from ssl_cr_histo_amd import _lib as L
    from ssl_cr_histo_amd import build
    if not os.path.exists(L.LIB_PATH):
        build.build()
    from ssl_cr_histo_amd import engine  # noqa: F401  registers engine signatures
    lib = L.lib()
    assert lib.sslcr_version() >= 7
    d = L.AugV2Desc()
    assert lib.sslcr_randaug_v2_slot(d, None) == -1 and b"null" in lib.sslcr_last_error()
    d.src, d.dst, d.op, d.N, d.H, d.W = 16, 32, 48, 1, 8, 8          # never dereferenced: the checks come first
    d.ops_mask = 1 << 4
    assert lib.sslcr_randaug_v2_slot(d, None) == -1 and b"workspace" in lib.sslcr_last_error()
    d.ops_mask = 1 << 9
    assert lib.sslcr_randaug_v2_slot(d, None) == -1 and b"affine" in lib.sslcr_last_error()
    d.ops_mask = 1 << 12
    assert lib.sslcr_randaug_v2_slot(d, None) == -1 and b"unknown op" in lib.sslcr_last_error()
    d.ops_mask, d.dst = 1, 16
    assert lib.sslcr_randaug_v2_slot(d, None) == -1 and b"aliases" in lib.sslcr_last_error()
