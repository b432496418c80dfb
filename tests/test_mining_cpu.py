"""CPU-only: the host side of device-resident RSP tile mining (ssl_cr_histo_amd/mining.py) against the reference's expressions as
tests/_mining_ref.py transcribes them, the CIELAB anchors of the restatement, the keep comparison, and the four C-ABI entries of
library version 14: exported, bound, laid out as the header says, and refusing bad arguments before any launch."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import _mining_ref as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("sslcr_tissue_bits", "sslcr_lab_a_sum", "sslcr_tile_popcount", "sslcr_rsp_gather")


@pytest.fixture(scope="module")
def lib():
    from ssl_cr_histo_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    from ssl_cr_histo_amd import engine  # noqa: F401  registers engine signatures
    return _lib.lib()


# ------------------------------------------------------------------------------------------------ grid, origins, orderings
@pytest.mark.parametrize("iw,ih,tile,stride", [(134, 90, 16, 8), (134, 90, 20, 7), (200, 131, 64, 64), (40, 40, 5, 3), (30, 18, 16, 8),
                                               (134, 90, (20, 16), (7, 8))])
def test_candidate_grid_is_the_reference_loop(iw, ih, tile, stride):
    from ssl_cr_histo_amd import mining
    ph, pw = (tile, tile) if np.isscalar(tile) else tile
    sh, sw = (stride, stride) if np.isscalar(stride) else stride
    want = [(xpos, ypos) for ypos in range(sh, ih - 1 - ph, sh) for xpos in range(sw, iw - 1 - pw, sw)]      # dataset.py:424-425
    xs, ys = mining.candidate_grid(iw, ih, tile, stride)
    assert [(x, y) for y in ys for x in xs] == want
    if (iw, ih) == (30, 18):
        assert ys == [] and xs == [8]                               # range(8, 1, 8): no row fits


@pytest.mark.parametrize("variant", ["v1", "v2"])
@pytest.mark.parametrize("downsamples", [(1.0, 4.0, 16.0), (1.0, 4.0003, 16.0012), (1.0, 2.0, 4.0)])
@pytest.mark.parametrize("tile", [16, 21])
def test_triplet_origins_against_the_literal_expressions(variant, downsamples, tile):
    from ssl_cr_histo_amd import mining
    scan = MR.Pyramid([np.zeros((4, 4, 3), np.uint8)] * 3, downsamples)
    xs, ys = mining.candidate_grid(300, 200, tile, 7)
    xpos, ypos = [x for y in ys for x in xs], [y for y in ys for x in xs]
    hr, lr1, lr2 = mining.triplet_origins(xpos, ypos, downsamples, tile, variant)
    assert hr.dtype == lr1.dtype == lr2.dtype == np.int32 and hr.shape == (len(xpos), 2)
    getitem = MR.getitem_v1 if variant == "v1" else MR.getitem_v2
    for k, (x, y) in enumerate(zip(xpos, ypos)):
        loc2, loc1, loc0 = getitem(scan, x, y, tile, tile)
        assert tuple(lr2[k]) == scan.level_origin(loc2, 2), (k, x, y)
        assert tuple(lr1[k]) == scan.level_origin(loc1, 1), (k, x, y)
        assert tuple(hr[k]) == scan.level_origin(loc0, 0), (k, x, y)
    if downsamples == (1.0, 4.0, 16.0) and tile == 16:
        k = 3                                                       # a hand check: x = 28, y = 7
        assert (xpos[k], ypos[k]) == (28, 7)
        if variant == "v1":                                         # hr and lr1 START at the lr2 tile's centre (36, 15) of level 2
            assert tuple(lr2[k]) == (28, 7) and tuple(lr1[k]) == (36 * 4, 15 * 4) and tuple(hr[k]) == (36 * 16, 15 * 16)
        else:                                                       # concentric: the centre minus half a tile in the level's pixels
            assert tuple(lr2[k]) == (28, 7) and tuple(lr1[k]) == (36 * 4 - 8, 15 * 4 - 8) and tuple(hr[k]) == (36 * 16 - 8, 15 * 16 - 8)
    with pytest.raises(ValueError):
        mining.triplet_origins(xpos, ypos, downsamples, tile, "v3")


def test_non_integer_downsample_moves_an_origin():
    """int(int(4.0003 * x) / 4.0003) is not always x: the case the 4.0003 rows above are there for"""
    from ssl_cr_histo_amd import mining
    xs = list(range(1, 400))
    _, _, lr2 = mining.triplet_origins(xs, xs, (1.0, 2.0, 4.0003), 16, "v1")
    assert any(int(lr2[k, 0]) != x for k, x in enumerate(xs))
    _, _, lr2 = mining.triplet_origins(xs, xs, (1.0, 2.0, 4.0), 16, "v1")
    assert all(int(lr2[k, 0]) == x for k, x in enumerate(xs))


def test_ordering_table_against_the_literal_loop():
    from ssl_cr_histo_amd import mining
    T = 3
    tiles = [np.full((T, 2, 2, 3), 10 * lvl, np.uint8) + np.arange(T, dtype=np.uint8).reshape(T, 1, 1, 1) for lvl in range(3)]
    d1, d2, d3, lab = MR.sorted_sequence(*tiles)
    assert lab.shape == (6 * T, 1, 1) and d1.shape == (6 * T, 2, 2, 3)
    for k in range(6 * T):
        order = mining.ORDERINGS[k % 6]
        assert int(lab[k, 0, 0]) == k % 6
        for slot, d in enumerate((d1, d2, d3)):
            assert int(d[k, 0, 0, 0]) == 10 * order[slot] + k // 6, (k, slot)
    assert [list(o) for o in mining.ORDERINGS] == MR.SORTING_ORDERS


# ------------------------------------------------------------------------------------------------ CIELAB
def test_lab_a_anchors():
    px = np.array([[[255, 0, 0], [0, 255, 0], [0, 0, 255]]], np.uint8)
    for f in (MR.lab_a, MR.lab_a_rows):
        a = f(px)[0]
        assert abs(a[0] - 80.0923) < 1e-3 and abs(a[1] + 86.1830) < 1e-3 and abs(a[2] - 79.1856) < 1e-3, a
    greys = np.repeat(np.arange(256, dtype=np.uint8)[None, :, None], 3, axis=2)
    assert np.abs(MR.lab_a_rows(greys)).max() < 3e-3
    assert np.abs(MR.lab_a(greys)).max() < 3e-3


def test_lab_a_forms_agree_to_rounding():
    """NumPy's matmul against the row-by-column loop, t ** (1/3) against cbrt: a few roundings of magnitudes <= 500"""
    img = MR.synthetic_pyramid(0).levels[2]
    a = MR.lab_a_rows(img)
    assert np.abs(MR.lab_a(img) - a).max() <= 1e-12
    xyz = MR.rgb2xyz(img) / np.array(MR.D65_2)
    assert (xyz[..., :2] > 0.008856).all()
    assert np.abs(500.0 * (np.cbrt(xyz[..., 0]) - np.cbrt(xyz[..., 1])) - a).max() <= 1e-12


def test_linear_table_is_the_restatements_linearisation():
    from ssl_cr_histo_amd import mining
    lin = mining.srgb_linear_table()
    assert lin.dtype == np.float64 and lin.shape == (256,)
    ramp = np.zeros((1, 256, 3), np.uint8)
    ramp[0, :, 0] = np.arange(256)                                  # a red ramp: X = lin * 0.412453 + 0 + 0, exact in any order
    assert np.array_equal(MR.rgb2xyz(ramp)[0, :, 0], lin * 0.412453)
    assert lin[0] == 0.0 and lin[255] == 1.0 and lin[10] == (10 * (1.0 / 255)) / 12.92 and (np.diff(lin) > 0).all()


# ------------------------------------------------------------------------------------------------ the keep comparison
def test_keep_comparison_is_the_reference_division():
    assert 380 / 400 >= 0.95 and not 379 / 400 >= 0.95              # util.py:23 at tile 20
    assert 192 / 256 >= 0.75 and not 191 / 256 >= 0.75              # Pretraining_v2/util.py:13 at tile 16
    pink, white = (180, 110, 160), (255, 255, 255)
    tile = np.empty((20, 20, 3), np.uint8)
    for n, want in ((380, True), (379, False)):
        tile.reshape(-1, 3)[:n] = pink
        tile.reshape(-1, 3)[n:] = white
        assert MR.isforeground_v1(tile, mu=10.0) is want
    tile = np.empty((16, 16, 3), np.uint8)
    for n, want in ((192, True), (191, False)):
        tile.reshape(-1, 3)[:n] = pink
        tile.reshape(-1, 3)[n:] = white
        assert bool(MR.isforeground_v2(tile)) is want


def test_synthetic_pyramid_meets_the_conditions_the_gpu_tests_rely_on():
    for seed in range(4):
        P = MR.synthetic_pyramid(seed)
        assert P.level_dimensions == ((536, 360), (268, 180), (134, 90)) and P.overview.shape == (45, 67, 3)
        thr = 1.15 * MR.mean_a(P.overview)
        assert int((np.abs(MR.lab_a_rows(P.levels[2]) - thr) < 1e-9).sum()) == 0
        for tile, stride in ((16, 8), (20, 7)):
            for variant in ("v1", "v2"):
                kept = MR.get_wsi_patches(P, tile, stride, variant)[3]
                assert (len(kept) == 0) if seed == 1 else (20 <= len(kept) <= 60), (seed, tile, stride, variant, len(kept))


# ------------------------------------------------------------------------------------------------ the C ABI
def test_exports_bindings_and_version(lib):
    from ssl_cr_histo_amd import _lib as L
    from ssl_cr_histo_amd import build, kernels, mining
    assert lib.sslcr_version() >= 14
    declared = build.header_symbols()
    for name in ENTRIES:
        assert name in declared and name in L.SIGNATURES and hasattr(lib, name), name
    for name in ("tissue_bits", "lab_a_sum", "tile_popcount", "rsp_gather"):
        assert callable(getattr(kernels, name))
    for name in ("candidate_grid", "triplet_origins", "mine_tiles", "RspDeviceLoader", "ORDERINGS", "srgb_linear_table"):
        assert hasattr(mining, name)
    flags = build.PER_FILE_FLAGS.get("mining.hip", [])
    assert "mining.hip" in build.SOURCES and "-ffp-contract=off" in flags


def _err(lib):
    return lib.sslcr_last_error().decode()


def test_argument_errors_are_decided_before_the_launch(lib):
    """every call below must fail in the argument checks: none reaches a launch (there is no device here)"""
    from ssl_cr_histo_amd import _lib as L
    p = C.c_void_p(0x1000)                                          # a non-NULL, aligned address that is never dereferenced
    for name in ENTRIES:
        assert getattr(lib, name)(None, None) == -1 and "null descriptor" in _err(lib), name
    # tissue_bits
    ok = dict(img=p, bits=p, lin=p, thr_sum=None, threshold=0.1, factor=1.0, count=0.0, H=4, W=70, pitch=3, mode=0)
    for change, msg in ((dict(H=0), "empty image"), (dict(pitch=2), "pitch"), (dict(mode=2), "mode"), (dict(img=None), "null tensor"),
                        (dict(bits=C.c_void_p(0x1002)), "alignment"), (dict(mode=1, lin=None), "lin"),
                        (dict(thr_sum=p, count=0.0), "count"), (dict(lin=C.c_void_p(0x1004)), "alignment")):
        assert lib.sslcr_tissue_bits(L.TissueBitsDesc(**{**ok, **change}), None) == -1, change
        assert msg in _err(lib), (change, _err(lib))
    # lab_a_sum
    ok = dict(img=p, lin=p, partials=p, sum=p, H=4, W=4)
    for change, msg in ((dict(W=0), "empty image"), (dict(lin=None), "null tensor"), (dict(sum=C.c_void_p(0x1004)), "alignment")):
        assert lib.sslcr_lab_a_sum(L.LabASumDesc(**{**ok, **change}), None) == -1, change
        assert msg in _err(lib), (change, _err(lib))
    # tile_popcount: H = 90, W = 134, tile 20 / stride 7 -> 9 x 16
    ok = dict(bits=p, count=p, keep=p, thresh=0.95, H=90, W=134, pitch=5, ph=20, pw=20, sh=7, sw=7, ny=9, nx=16)
    for change, msg in ((dict(ph=0), "tile and stride"), (dict(pitch=4), "pitch"), (dict(ny=10), "ranges"), (dict(nx=15), "ranges"),
                        (dict(keep=None), "null tensor"), (dict(count=C.c_void_p(0x1002)), "alignment")):
        assert lib.sslcr_tile_popcount(L.TilePopcountDesc(**{**ok, **change}), None) == -1, change
        assert msg in _err(lib), (change, _err(lib))
    assert lib.sslcr_tile_popcount(L.TilePopcountDesc(**{**ok, **dict(H=21, ny=0, bits=None, count=None, keep=None)}), None) == 0
    # rsp_gather
    vp3, i3 = C.c_void_p * 3, C.c_int * 3

    def gd(**kw):
        d = dict(src=vp3(0x1000, 0x1000, 0x1000), xy=vp3(0x1000, 0x1000, 0x1000), idx=p, dst=vp3(0x1000, 0x1000, 0x1000), label=p,
                 RH=i3(8, 8, 8), RW=i3(8, 8, 8), T=1, N=2, S=4, fill=0)
        d.update(kw)
        return L.RspGatherDesc(**d)
    for change, msg in ((dict(S=0), "S >= 1"), (dict(T=0), "T >= 1"), (dict(RW=i3(8, 0, 8)), "empty level"), (dict(fill=256), "fill"),
                        (dict(idx=None), "null tensor"), (dict(src=vp3(0x1000, 0, 0x1000)), "null tensor"),
                        (dict(xy=vp3(0x1000, 0x1000, 0x1002)), "xy alignment"), (dict(label=C.c_void_p(0x1004)), "alignment")):
        assert lib.sslcr_rsp_gather(gd(**change), None) == -1, change
        assert msg in _err(lib), (change, _err(lib))
    assert lib.sslcr_rsp_gather(gd(N=0, idx=None, label=None), None) == 0      # N == 0 is a no-op


def test_wrappers_refuse_host_tensors_and_bad_arguments():
    from ssl_cr_histo_amd import _lib as L
    from ssl_cr_histo_amd import kernels, mining
    img = torch.zeros(8, 8, 3, dtype=torch.uint8)
    with pytest.raises(L.SslcrError):
        kernels.tissue_bits(img, "hsv_s", 0.1)
    with pytest.raises(L.SslcrError):
        kernels.lab_a_sum(img, torch.zeros(256, dtype=torch.float64))
    with pytest.raises(L.SslcrError):
        kernels.tile_popcount(torch.zeros(8, 1, dtype=torch.int32), 8, (2, 2), (1, 1), 0.5)
    with pytest.raises(L.SslcrError):
        kernels.rsp_gather((img, img, img), (torch.zeros(1, 2, dtype=torch.int32),) * 3, torch.zeros(1, dtype=torch.int64), 4)
    with pytest.raises(L.SslcrError):
        kernels.rsp_gather((img, img), (), torch.zeros(1, dtype=torch.int64), 4)
    with pytest.raises(ValueError):
        mining.candidate_grid(10, 10, 0, 1)
    with pytest.raises(ValueError):
        mining.mine_tiles((img, img), (1.0, 2.0), 4, 2)
    with pytest.raises(ValueError):
        mining.mine_tiles((img, img, img), (1.0, 2.0, 4.0), 4, 2, variant="v1", criterion=("cmyk", 0.1, 0.5))
    with pytest.raises(ValueError):
        mining.RspDeviceLoader((img, img, img), (1.0, 2.0, 4.0), 4, 2, 0)
