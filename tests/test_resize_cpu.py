"""CPU-only: the Pillow-exact resize without a device.  The NumPy restatement (tests/_resize_ref.py) EQUALS the live Pillow; the library's
coefficient entry (sslcr_resample_coeffs) EQUALS the restatement; the int32 bound holds for the five filters and a table that breaks
it is refused; the plan (sslcr_resample_plan) stays within the launcher's LDS and picks the forms it should; torchvision's output-size
rule against literal values; the host logic of PatchDeviceLoader; and the recorded golden against the Pillow that is installed."""
import os

import numpy as np
import pytest
import torch

import _resize_cases as RC
import _resize_ref as R


@pytest.fixture(scope="module")
def lib():
    from ssl_cr_histo_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    return _lib.lib()


# ---- the grid the definition was verified on: 5 sources x 6 targets x 5 filters x {no box, a fractional box} = 300 cases
def _grid_sources():
    rs = np.random.RandomState(0)
    srcs = [rs.randint(0, 256, size=(h, w, 3), dtype=np.uint8) for h, w in ((512, 512), (37, 53), (256, 300), (9, 7))]
    srcs.append((rs.randint(0, 2, size=(64, 64, 3)) * 255).astype(np.uint8))
    return srcs


def _targets(h, w):
    return [(256, 256), (h, w // 2 + 1), (2 * h + 1, w), (5, 3), (h + 20, w + 20), (1, 1)]


GRID = [(i, t, f, b) for i in range(5) for t in range(6) for f in RC.FILTERS for b in (False, True)]
needs_pillow = pytest.mark.skipif(RC.pillow() is None, reason="Pillow is not installed: the pin restatement == live Pillow cannot run; "
                                  "test_golden_is_the_installed_pillows still holds the restatement equal to the recorded Pillow 12.2.0 outputs")


@pytest.fixture(scope="module")
def grid_sources():
    return _grid_sources()


@needs_pillow
@pytest.mark.parametrize("i", range(5))
def test_restatement_equals_pillow_on_the_grid(grid_sources, i):
    assert len(GRID) == 300
    a = grid_sources[i]
    h, w = a.shape[:2]
    n = 0
    for oh, ow in _targets(h, w):
        for f in RC.FILTERS:
            for box in (None, RC.frac_box(h, w)):
                want = RC.pil_resize(a, (oh, ow), f, box)
                got = R.resize(a, (ow, oh), f, box)
                assert np.array_equal(want, got), (a.shape, (oh, ow), f, box)
                n += 1
    assert n == 60


@needs_pillow
def test_restatement_equals_pillow_in_mode_l_and_per_channel(grid_sources):
    a = grid_sources[1]
    for f in RC.FILTERS:
        rgb = RC.pil_resize(a, (19, 27), f)
        l = RC.pil_resize(np.ascontiguousarray(a[..., 0]), (19, 27), f)
        assert np.array_equal(l, rgb[..., 0]) and np.array_equal(l, R.resize(a[..., 0], (27, 19), f))


@needs_pillow
def test_nearest_restatement_equals_pillow_without_a_box(grid_sources):
    """21 cases and more: every source of the grid but the binary one x the six targets (24).  Pillow's NEAREST walks the source
    position (``xo += scale``); the closed form floor(in0 + (xx + 0.5) * scale) is NOT equal to it -- 512 -> 257 is in this grid."""
    n = closed_form_differs = 0
    for a in grid_sources[:4]:
        h, w = a.shape[:2]
        for oh, ow in _targets(h, w):
            want = RC.pil_resize(a, (oh, ow), "nearest")
            assert np.array_equal(want, R.resize(a, (ow, oh), "nearest")), (a.shape, oh, ow)
            cf = a[R.nearest_index_closed_form(h, 0.0, float(h), oh)][:, R.nearest_index_closed_form(w, 0.0, float(w), ow)]
            closed_form_differs += not np.array_equal(want, cf)
            n += 1
    assert n == 24 >= 21
    assert closed_form_differs >= 1          # the finding the walk exists for


def _axes_of_grid():
    axes = set()
    for h, w in ((512, 512), (37, 53), (256, 300), (9, 7), (64, 64)):
        for oh, ow in _targets(h, w):
            for box in (None, RC.frac_box(h, w)):
                x0, y0, x1, y1 = (0.0, 0.0, float(w), float(h)) if box is None else box
                axes.add((w, x0, x1, ow))
                axes.add((h, y0, y1, oh))
    return sorted(axes)


@pytest.mark.parametrize("name", RC.FILTERS)
def test_coefficient_entry_equals_the_restatement(lib, name):
    from ssl_cr_histo_amd import kernels as K
    axes = _axes_of_grid()
    assert len(axes) > 60
    for isz, a0, a1, osz in axes:
        k, b = K.resample_axis(isz, a0, a1, osz, name)
        rk, rb, _ = R.coeffs(isz, a0, a1, osz, name)
        assert k.dtype == np.int32 and k.shape == rk.shape and np.array_equal(k, rk), (name, isz, a0, a1, osz)
        assert np.array_equal(b, rb), (name, isz, a0, a1, osz)
    # a wider stride pads with zeros, and NEAREST writes the gather table of the walk
    k, b = K.resample_axis(53, 1.25, 52.25, 27, name, k_stride=40)
    rk, rb, _ = R.coeffs(53, 1.25, 52.25, 27, name)
    assert np.array_equal(k[:, :rk.shape[1]], rk) and not k[:, rk.shape[1]:].any() and np.array_equal(b, rb)


def test_nearest_table_is_the_walk(lib):
    from ssl_cr_histo_amd import kernels as K
    for isz, osz in ((512, 257), (512, 532), (37, 19), (9, 19), (53, 1), (3, 1800)):
        k, b = K.resample_axis(isz, 0.0, float(isz), osz, "nearest")
        assert k.shape == (osz, 1) and (k == 1 << 22).all() and (b[:, 1] == 1).all()
        assert np.array_equal(b[:, 0], R.nearest_index(isz, 0.0, float(isz), osz))


SWEEP = [(512, o) for o in (1, 2, 3, 4, 5, 7, 8, 9, 16, 31, 100, 255, 256, 257, 511, 513, 1000)] + \
        [(3, o) for o in (1, 2, 3, 4, 5, 7, 100, 1800)] + [(600, 1), (1, 600), (2, 1200), (7, 9), (9, 7)]
LIMIT = ((1 << 31) - (1 << 21)) / 255 / (1 << 22)        # sum|w| below which 255 * sum|k| + 2^21 < 2^31 (up to the rounding of k)


@pytest.mark.parametrize("name", RC.FILTERS)
def test_int32_bound_holds_for_the_five_filters(lib, name):
    """scales 1/600 .. 600 (512 -> 1 .. 3 -> 1800), the whole axis and a fractional box: the entry accepts every table (it refuses
    one that breaks the bound), every row has 255 * sum|k| + 2^21 < 2^31 and every |k| < 2^23"""
    from ssl_cr_histo_amd import kernels as K
    worst = 0.0
    for isz, osz in SWEEP:
        for a0, a1 in ((0.0, float(isz)),) + (((0.25, isz - 0.5),) if isz > 1 else ()):
            k, _ = K.resample_axis(isz, a0, a1, osz, name)
            k64 = np.abs(k.astype(np.int64))
            assert (255 * k64.sum(1) + (1 << 21) < 1 << 31).all() and (k64 < 1 << 23).all(), (name, isz, osz)
            assert lib.sslcr_resample_table_ok(k.ctypes.data, osz, k.shape[1]) == 1
            worst = max(worst, R.coeffs(isz, a0, a1, osz, name)[2])
    print(f"{name}: worst sum|w| = {worst:.4f} (limit {LIMIT:.4f})")
    assert worst < {"box": 1.001, "bilinear": 1.001, "hamming": 1.001, "bicubic": 1.5, "lanczos": 1.75}[name] < LIMIT


def test_a_table_that_breaks_the_bound_is_refused(lib):
    from ssl_cr_histo_amd import _lib as L
    from ssl_cr_histo_amd import kernels as K
    k, _ = K.resample_axis(53, 0.0, 53.0, 27, "lanczos")
    assert lib.sslcr_resample_table_ok(k.ctypes.data, 27, k.shape[1]) == 1
    bad = k.copy()
    bad[13, 0], bad[13, 1] = 5_000_000, -5_000_000              # sum|k| = 1e7 + ...: 255 * sum >= 2^31
    assert lib.sslcr_resample_table_ok(bad.ctypes.data, 27, k.shape[1]) == 0
    bad = k.copy()
    bad[3, 2] = 1 << 23                                          # one |k| outside the 24-bit multiply
    assert lib.sslcr_resample_table_ok(bad.ctypes.data, 27, k.shape[1]) == 0
    # the coefficient entry refuses with NOTHING written: a stride below ksize, a box outside the axis, an unknown filter
    for args in ((53, 0.0, 53.0, 27, 1, k.shape[1] - 1), (53, 0.0, 54.0, 27, 1, k.shape[1]), (53, -1.0, 53.0, 27, 1, k.shape[1]),
                 (53, 0.0, 53.0, 27, 9, k.shape[1])):
        kk = np.full((27, k.shape[1]), -7, dtype=np.int32)
        bb = np.full((27, 2), -7, dtype=np.int32)
        isz, a0, a1, osz, code, stride = args
        assert lib.sslcr_resample_coeffs(isz, a0, a1, osz, code, kk.ctypes.data, stride, bb.ctypes.data) == -1
        assert lib.sslcr_last_error() and (kk == -7).all() and (bb == -7).all()
    with pytest.raises(L.SslcrError):
        K.resample_axis(53, 10.0, 5.0, 27, "bilinear")


def test_resize_output_size_is_torchvisions_rule():
    from ssl_cr_histo_amd import kernels as K
    assert K.resize_output_size(512, 512, 256) == (256, 256)
    assert K.resize_output_size(300, 400, 256) == (256, 341)          # int(256 * 400 / 300) = 341
    assert K.resize_output_size(400, 300, 256) == (341, 256)
    assert K.resize_output_size(400, 300, (5, 6)) == (5, 6)           # a pair is (h, w)
    assert K.resize_output_size(37, 53, [19]) == (19, 27)             # int(19 * 53 / 37) = 27
    assert "PARITY UNPINNED" in K.resize_output_size.__doc__
    with pytest.raises(ValueError):
        K.resize_output_size(0, 5, 3)


def test_plan_stays_within_the_launchers_lds(lib):
    from ssl_cr_histo_amd import _lib as L
    from ssl_cr_histo_amd import kernels as K
    forms = set()
    for name in RC.FILTERS:
        for (h, w), (oh, ow) in (((64, 64), (32, 32)), ((512, 512), (256, 256)), ((512, 512), (64, 64)), ((512, 512), (16, 16)),
                                 ((37, 53), (19, 27)), ((9, 7), (19, 27)), ((33, 65), (1, 1)), ((2048, 2048), (24, 24)),
                                 ((2048, 300), (8, 290)), ((100, 4096), (90, 5)), ((256, 256), (1024, 1024))):
            for layout in ("hwc", "chw"):
                for ch in (1, 3):
                    p = K.resample_plan((h, w), (ow, oh), name, n=3, channels=ch, layout=layout)
                    assert p["form"] in ("fused", "two_pass")
                    assert p["lds_bytes"] <= L.RESAMPLE_LDS_CAP
                    assert (p["form"] == "fused") == p["fused_ok"]          # the default is fused wherever it fits
                    if p["form"] == "fused":
                        assert p["lds_bytes"] > 0 and p["tile"][0] % 4 == 0 and p["grid"][0] == 3 * -(-ow // p["tile"][0]) * -(-oh // p["tile"][1])
                        assert p["window"][0] <= h and p["window"][1] <= w and p["workspace_bytes"] == 0
                        assert K.resample_plan((h, w), (ow, oh), name, n=3, channels=ch, layout=layout, form="two_pass")["form"] == "two_pass"
                    else:
                        assert p["workspace_bytes"] == 3 * ch * h * ow and p["grid"][0] > 0 and p["grid"][1] > 0
                    forms.add(p["form"])
    assert forms == {"fused", "two_pass"}


def test_plan_picks_the_forms_it_should(lib):
    from ssl_cr_histo_amd import _lib as L
    from ssl_cr_histo_amd import kernels as K
    assert K.resample_plan((64, 64), (32, 32), "bilinear")["form"] == "fused"
    # 8192 x 8 -> 8 x 8 LANCZOS: an axis of 8 -> 8 without a box is SKIPPED (Pillow's rule), so this descriptor needs one pass and
    # takes its single launch -- in neither reading (8192 the width or the height) can it be the two-launch form ...
    assert K.resample_plan((8, 8192), (8, 8), "lanczos")["form"] == "horizontal"
    assert K.resample_plan((8192, 8), (8, 8), "lanczos")["form"] == "vertical"
    # ... which a large down-scale takes as soon as both axes need a pass: the fused tile would stage 8192 columns
    for hw in ((9, 8192), (8192, 9)):
        p = K.resample_plan(hw, (8, 8), "lanczos")
        assert p["form"] == "two_pass" and not p["fused_ok"] and p["lds_bytes"] == 0
        with pytest.raises(L.SslcrError, match="fused"):
            K.resample_plan(hw, (8, 8), "lanczos", form="fused")
    # a fractional box on the 8-pixel axis makes the literal case a two-pass one as well
    assert K.resample_plan((8, 8192), (8, 8), "lanczos", box=(0.0, 0.5, 8192.0, 7.5))["form"] == "two_pass"
    # forcing a form is for descriptors with both passes
    for kw in (dict(form="fused"), dict(form="two_pass")):
        with pytest.raises(L.SslcrError):
            K.resample_plan((37, 53), (27, 37), "bilinear", **kw)         # (ow, oh) = (27, 37): the horizontal pass only
    assert K.resample_plan((37, 53), (27, 37), "bilinear")["form"] == "horizontal"
    assert K.resample_plan((37, 53), (53, 19), "bilinear")["form"] == "vertical"
    assert K.resample_plan((37, 53), (53, 37), "bilinear")["form"] == "gather"            # nothing to do: the copy
    assert K.resample_plan((37, 53), (27, 19), "nearest")["form"] == "gather"
    assert K.resample_plan((33, 65), (65, 33), "bilinear", box=RC.frac_box(33, 65))["form"] == "fused"
    # per-image boxes: the distinct boxes are the table sets
    assert K.resample_plan((37, 53), (27, 19), "bicubic", box=np.array(RC.BOXES5), n=5)["form"] == "fused"
    with pytest.raises(ValueError):
        K.resample_plan((37, 53), (27, 19), "nearest", box=(0, 0, 5, 5))
    with pytest.raises(ValueError):
        K.resample_plan((37, 53), (27, 19), "bilinear", box=(0, 0, 54, 5))
    with pytest.raises(ValueError):
        K.resample_plan((37, 53), (27, 19), "sinc")


def test_entries_are_declared_bound_and_exported(lib):
    from ssl_cr_histo_amd import _lib as L
    from ssl_cr_histo_amd import build
    names = {"sslcr_resample", "sslcr_resample_plan", "sslcr_resample_coeffs", "sslcr_resample_ksize", "sslcr_resample_table_ok"}
    assert names <= set(build.header_symbols()) and names <= set(L.SIGNATURES)
    for n in names:
        assert hasattr(lib, n)
    assert "resample.hip" in build.SOURCES
    assert lib.sslcr_version() == 16                  # told by their symbols, not by a number (16 is the switch listing's)
    # N == 0 is a no-op that succeeds, without a device
    d = L.ResampleDesc(None, None, None, None, None, None, None, None, None, None, 0, 3, 8, 8, 8, 8, 1, 1, 1, 0, 1, 0, 0)
    assert lib.sslcr_resample(d, None) == 0
    d.C = 4
    assert lib.sslcr_resample(d, None) == -1 and b"C outside" in lib.sslcr_last_error()


def test_patch_loader_host_logic():
    from ssl_cr_histo_amd.inference import PatchDeviceLoader
    patches = RC.loader_patches()
    ta, tb = np.arange(10, dtype=np.float32), np.arange(10, 20, dtype=np.float32)
    ld = PatchDeviceLoader(patches, ta, tb, image_size=32, batch_size=4)
    assert len(ld) == 3 and len(ld.dataset) == 10 and ld.ranges() == [(0, 4), (4, 8), (8, 10)] and ld.out_hw == (32, 32)
    assert torch.equal(ld.targets[1][8:10], torch.tensor([18.0, 19.0]))
    assert PatchDeviceLoader(patches, image_size=(20, 30), batch_size=10).out_hw == (20, 30)
    assert len(PatchDeviceLoader(patches, image_size=32, batch_size=10)) == 1
    assert len(PatchDeviceLoader(patches[:0], image_size=32, batch_size=4)) == 0
    chw = PatchDeviceLoader(np.zeros((5, 3, 40, 60), np.uint8), image_size=20, batch_size=2, layout="chw")
    assert chw.out_hw == (20, 30) and len(chw) == 3
    for bad in (dict(patches=patches.astype(np.float32)), dict(patches=patches[0]), dict(patches=patches[..., :2]), dict(batch_size=0),
                dict(layout="nhwc"), dict(layout="chw"), dict(resample="sinc"), dict(image_size=0), dict(targets=(ta[:9],))):
        kw = dict(patches=patches, targets=(), image_size=32, batch_size=4)
        kw.update(bad)
        p, t = kw.pop("patches"), kw.pop("targets")
        with pytest.raises(ValueError):
            PatchDeviceLoader(p, *t, **kw)


def test_golden_is_the_installed_pillows(lib):
    """the recorded outputs: written by tests/golden/make_resize_golden.py, equal to the restatement, and -- where Pillow is installed
    in the recorded version -- to the live Pillow"""
    g = RC.golden()
    assert str(g["pillow_version"]) == "12.2.0"
    assert os.path.getsize(RC.GOLDEN) < 64 * 1024                        # tens of kilobytes
    for name in RC.RECORDED_INPUTS:
        assert np.array_equal(g["in_" + name], RC.source(name))          # the seeds still give the recorded inputs
    live = RC.pillow() is not None and __import__("PIL").__version__ == "12.2.0"
    for src, hw, f, box in RC.RECORDED:
        want = g[RC.key(src, hw, f, box)]
        assert np.array_equal(want, R.resize(RC.source(src), (hw[1], hw[0]), f, box)), (src, hw, f, box)
        if live:
            assert np.array_equal(want, RC.pil_resize(RC.source(src), hw, f, box))
    for (h, w), hw in RC.BIG_CASES:
        assert np.array_equal(g[RC.key(f"big{h}x{w}", hw, "lanczos", None)], R.resize(RC.big_source(h, w), (hw[1], hw[0]), "lanczos"))
    assert len(RC.RECORDED) == 5 * 3 + 2 + 6 and len(g) == 1 + len(RC.RECORDED_INPUTS) + len(RC.RECORDED) + len(RC.BIG_CASES)
