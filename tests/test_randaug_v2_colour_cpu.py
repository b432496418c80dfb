"""CPU-only: the hed / hsv ops of the RSP v2 device RandAugment -- the draw order of ``colour_ops="device"``, the hsv restatement
against Python's ``colorsys``, the hed error bound against numpy's own float32 evaluation, and the C entry's argument checks."""
import colorsys
import ctypes as C
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

import _colour_ref as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ draw order
@pytest.mark.parametrize("n", [2, 14])
@pytest.mark.parametrize("seed", [0, 1, 7, 123, 2024])
def test_device_colour_plan_draws_like_the_reference(n, seed):
    """plan() with colour_ops="device" against the restated per-image planner: same rows, and both generators left in the same
    state.  n = 14 puts hed and hsv into every image."""
    from ssl_cr_histo_amd import augment as A
    k = 9
    rng, np_rng = random.Random(seed), np.random.RandomState(seed)
    got = A.RandAugmentV2Device(n, 10, rng, np_rng, colour_ops="device").plan(k)
    r_rng, r_np = random.Random(seed), np.random.RandomState(seed)
    want = [CR.plan_image(r_rng, r_np, n, 10) for _ in range(k)]
    assert got == want
    if n == 14:
        assert all({"hed", "hsv"} <= {nm for nm, _, _ in row} for row in got)
    for row in got:
        for nm, val, third in row:
            if nm == "hed":
                assert len(third) == 6 and all(abs(v) <= val * 0.03 for v in third)
            elif nm == "hsv":
                assert len(third) == 3 and third[2] == 0.0 and all(abs(v) <= val * 0.03 for v in third)
    assert rng.random() == r_rng.random() and np_rng.uniform() == r_np.uniform()


@pytest.mark.parametrize("seed", [3, 11])
def test_triplet_wrapper_plans_in_dataset_order(seed):
    """TripletRandAugmentV2 hands D1, D2, D3 the rows 3 i + k of ONE plan: the draws of triplet i's three tiles, then triplet i + 1's"""
    from ssl_cr_histo_amd import augment as A
    N = 5
    t = A.TripletRandAugmentV2(3, 10, random.Random(seed), np.random.RandomState(seed), colour_ops="device")
    assert t.aug.colour_ops == "device"
    plan = t.aug.plan(3 * N)
    r_rng, r_np = random.Random(seed), np.random.RandomState(seed)
    for i in range(N):
        for k in range(3):
            assert plan[k::3][i] == CR.plan_image(r_rng, r_np, 3, 10), (i, k)
    assert t.aug.rng.random() == r_rng.random() and t.aug.np_rng.uniform() == r_np.uniform()


def test_default_keyword_keeps_the_host_behaviour():
    from ssl_cr_histo_amd import augment as A
    with pytest.raises(NotImplementedError, match="hed|hsv"):
        A.RandAugmentV2Device(14, 10, random.Random(0), np.random.RandomState(0)).plan(1)
    with pytest.raises(NotImplementedError, match="hed|hsv"):
        A.TripletRandAugmentV2(14, 10, random.Random(0), np.random.RandomState(0)).aug.plan(1)
    with pytest.raises(ValueError):
        A.RandAugmentV2Device(2, 10, random.Random(0), np.random.RandomState(0), colour_ops="gpu")
    # a name in host_ops goes to the host in either mode: no draws at plan time, the row's third slot stays None
    a = A.RandAugmentV2Device(14, 10, random.Random(0), np.random.RandomState(0), host_ops={"hed": lambda im, v: im}, colour_ops="device")
    (row,) = a.plan(1)
    third = {nm: t for nm, _, t in row}
    assert third["hed"] is None and len(third["hsv"]) == 3


def test_param_rows_are_what_the_in_place_numpy_ops_use():
    from ssl_cr_histo_amd import augment as A
    d = (0.1234567891, -0.2, 0.0, 0.05, 0.0, -0.29999)
    row = A.colour_param_row("hed", d)
    assert row == [float(np.float32(1.0 + v)) for v in d[:3]] + [float(np.float32(v)) for v in d[3:]]
    assert A.colour_param_row("hsv", (-0.25, 0.1, 0.0))[:2] == [0.75, 0.1]
    assert A.colour_param_row("hsv", (0.0, -0.1, 0.0))[:2] == [0.0, -0.1]
    assert A.colour_param_row("hsv", (0.3, 0.0))[:2] == [0.3 % 1.0, 0.0]
    with pytest.raises(ValueError):
        A.colour_param_row("hsv", (0.1, 0.1, 0.2))
    inv, fwd = A.v2_hed_matrices()
    r_inv, r_fwd = CR.hed_matrices()
    assert inv.dtype == np.float32 and fwd.dtype == np.float32 and np.array_equal(inv, r_inv) and np.array_equal(fwd, r_fwd)


# ------------------------------------------------------------------------------------------------ hsv: the spec against colorsys
def _circ(a, b):
    d = abs(a - b)
    return min(d, 1.0 - d)


def test_hsv_restatement_agrees_with_colorsys():
    """rgb2hsv / hsv2rgb as restated from scikit-image against an independent implementation, on greys (delta == 0), black, white,
    every kind of channel tie and a random lot; then the whole op with hue shifts of both signs and saturation sigmas of both signs"""
    px = CR.colorsys_check_pixels()
    f = CR.as_float(px[None])                                     # [1, K, 3]
    hsv = CR.rgb2hsv(f)[0]
    back = CR.hsv2rgb(hsv[None])[0]
    for k, (r, g, b) in enumerate(f[0]):
        h, s, v = colorsys.rgb_to_hsv(r, g, b)
        assert _circ(hsv[k, 0], h) <= 1e-12 and abs(hsv[k, 1] - s) <= 1e-12 and abs(hsv[k, 2] - v) <= 1e-12, (px[k], hsv[k], (h, s, v))
        assert np.abs(back[k] - np.array(colorsys.hsv_to_rgb(*hsv[k]))).max() <= 1e-12, px[k]
        assert np.abs(back[k] - f[0, k]).max() <= 1e-12, px[k]         # and the round trip is the identity
    grey = px[:, 0] == px[:, 1]
    grey &= px[:, 1] == px[:, 2]
    assert grey.sum() >= 4 and not hsv[grey, :2].any()                 # h = s = 0 where delta == 0, black included
    for sh, ss in ((0.21, 0.13), (-0.21, -0.13), (0.0, 0.3), (-0.07, 0.0), (0.3, -0.3)):
        got = CR.hsv_float(px[None], sh, ss)[0]
        for k, (r, g, b) in enumerate(f[0]):
            h, s, v = colorsys.rgb_to_hsv(r, g, b)
            if sh != 0.0:
                h = (h + sh % 1.0) % 1.0
            if ss < 0.0:
                s *= 1.0 + ss
            elif ss > 0.0:
                s *= 1.0 + (1.0 - s) * ss
            assert np.abs(got[k] - np.array(colorsys.hsv_to_rgb(h, s, v))).max() <= 1e-12, (px[k], sh, ss)
        out = CR.hsv(px[None], sh, ss)[0]
        assert out.dtype == np.uint8 and np.array_equal(out[grey], px[grey])      # a grey pixel has no hue and no saturation to edit


# ------------------------------------------------------------------------------------------------ hed: the bound
def test_hed_bound_holds_numpys_float32_evaluation():
    """numpy's float32 evaluation of the chain -- the reference's arithmetic, np.dot included -- inside the admissible set of every
    byte; the set is tight (at most 1 % of the bytes have two admissible values) and the inputs exercise it (at least half of the
    bytes unsaturated).  The all-zero draw is kept out of these inputs and checked in test_hed_cutoff_and_identity: its Y is the input
    byte up to rounding, an integer, so there EVERY byte has the two admissible values b - 1 and b by construction."""
    two, unsat, worst, dmax, count = 0.0, 0.0, 0.0, 0.0, 0
    for k in range(12):
        rs = np.random.RandomState(40 + k)
        img = CR.tissue(48, 40, k)
        f = (0.03, 0.1, 0.2, 0.3)[k % 4]
        draws = tuple(rs.uniform(-f, f, 6))
        assert CR.hed_applies(img)
        lo, hi, Y, delta = CR.hed_bound(img, draws)
        got = CR.hed_f32(img, draws)
        bad = (got < lo) | (got > hi)
        assert not bad.any(), (k, int(bad.sum()))
        y32 = _hed_f32_before_truncation(img, draws)
        inner = (Y > 0.0) & (Y < 255.0)
        worst = max(worst, float((np.abs(y32 - np.clip(Y, 0, 255)) / delta)[inner].max()))
        t, u = CR.bound_stats(lo, hi, Y)
        two, unsat, dmax, count = two + t, unsat + u, max(dmax, float(delta.max())), count + 1
    print(f"hed bound: delta <= {dmax:.2e} byte steps, numpy-f32 worst {worst:.3f} of the bound, "
          f"{100 * two / count:.3f} % two-valued, {100 * unsat / count:.1f} % unsaturated")
    assert dmax < 0.05 and worst <= 1.0
    assert two / count <= 0.01 and unsat / count >= 0.5


def _hed_f32_before_truncation(img, draws):
    """hed_f32 without the final astype: float32 value in [0, 255]"""
    mi, m = CR.hed_matrices()
    sig, bias = CR.hed_scalars(draws)
    x = CR.hed_input(img)
    st = np.reshape(np.dot(np.reshape(-np.log(x), (-1, 3)), mi), x.shape)
    for j in range(3):
        st[..., j] *= sig[j]
        st[..., j] += bias[j]
    im = np.reshape(np.exp(np.dot(-np.reshape(st, (-1, 3)), m)) - 2, st.shape)
    im = np.clip(im, -1, 1)
    im = (im - np.float32(-1)) / np.float32(2.0) * np.float32(2) + np.float32(-1)
    return (np.clip(im, 0.0, 1.0) * np.float32(255.0)).astype(np.float64)


def test_hed_cutoff_and_identity():
    dark, bright = np.full((8, 8, 3), 30, np.uint8), np.full((8, 8, 3), 230, np.uint8)
    d = (0.1, -0.1, 0.05, 0.02, -0.02, 0.01)
    for im in (dark, bright):
        assert not CR.hed_applies(im) and CR.hed_f32(im, d) is im
        lo, hi, _, _ = CR.hed_bound(im, d)
        assert np.array_equal(lo, im) and np.array_equal(hi, im)
    img = CR.tissue(16, 16, 3)
    lo, hi, Y, _ = CR.hed_bound(img, (0.0,) * 6)
    assert np.abs(Y - img).max() < 0.01            # no edit: the round trip is the identity up to its rounding ...
    assert ((lo <= img) & (img <= hi) | (hi == img - 1) | (lo == img)).all()      # ... which truncation may turn into one byte step down


# ------------------------------------------------------------------------------------------------ ABI
@pytest.fixture(scope="module")
def lib():
    from ssl_cr_histo_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    return _lib.lib()


def test_colour_entry_is_declared_exported_and_bound(lib):
    from ssl_cr_histo_amd import _lib, build
    assert "sslcr_randaug_v2_colour" in build.header_symbols()
    assert "sslcr_randaug_v2_colour" in _lib.SIGNATURES and hasattr(lib, "sslcr_randaug_v2_colour")
    assert lib.sslcr_version() >= 11
    nm = shutil.which("nm")
    if nm:
        out = subprocess.run([nm, "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
        assert " T sslcr_randaug_v2_colour" in out


def test_colour_entry_refuses_bad_descriptors_without_a_device(lib):
    from ssl_cr_histo_amd import _lib as L
    one = C.c_void_p(4096)
    d = L.AugV2ColourDesc()
    assert lib.sslcr_randaug_v2_colour(None, None) == -1
    assert lib.sslcr_randaug_v2_colour(d, None) == -1 and b"null" in lib.sslcr_last_error()
    d.img, d.op, d.N, d.H, d.W = one, one, 2, 8, 8
    d.cutoff_lo, d.cutoff_hi = 0.15, 0.85
    assert lib.sslcr_randaug_v2_colour(d, None) == -1 and b"param" in lib.sslcr_last_error()
    d.param = one
    d.ops_mask = 1 << 3
    assert lib.sslcr_randaug_v2_colour(d, None) == -1 and b"unknown op" in lib.sslcr_last_error()
    d.ops_mask = (1 << L_HED()) | 1
    assert lib.sslcr_randaug_v2_colour(d, None) == -1 and b"bsum" in lib.sslcr_last_error()
    d.ops_mask, d.N = 1 << 2, 0
    assert lib.sslcr_randaug_v2_colour(d, None) == -1 and b"batch shape" in lib.sslcr_last_error()
    d.N, d.cutoff_lo = 2, 0.9
    assert lib.sslcr_randaug_v2_colour(d, None) == -1 and b"cutoff" in lib.sslcr_last_error()


def L_HED():
    from ssl_cr_histo_amd import augment as A
    assert (A.V2C_COPY, A.V2C_HED, A.V2C_HSV) == (0, 1, 2)
    return A.V2C_HED


def test_colour_descriptor_matches_the_header_layout():
    """(size and offsets of sslcr_augv2_colour_desc: tests/test_abi_cpu.py, for every mirror)  The three op codes of the header"""
    from ssl_cr_histo_amd import _lib as L
    from ssl_cr_histo_amd import build
    defs = build.header_defines()
    assert "sslcr_augv2_colour_desc" in L.MIRRORS
    assert [defs["SSLCR_AUGV2C_COPY"], defs["SSLCR_AUGV2C_HED"], defs["SSLCR_AUGV2C_HSV"]] == [0, 1, 2]
