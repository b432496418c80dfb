"""Device-resident RSP tile mining on the MI355X (include/sslcr.h, library version 14) against tests/_mining_ref.py: the tissue bit
plane (hsv_s: equality; lab_a: equality outside a 1e-9 band around the threshold that the inputs are asserted to leave EMPTY), the
deterministic sum of a*, the window popcounts, the triplet gather with sorted_sequence's orderings, and RspDeviceLoader against the
host pipeline batch for batch and through one rsp_train epoch.

Why 1e-9: a* is about 12 float64 operations on magnitudes <= 500 with two ``pow`` within a few ulp, an error <= 1e-12; the device's
threshold, when it takes the mean from sslcr_lab_a_sum, differs from NumPy's by the sum's bound / n <= 2e-11 on these images.  A pixel
whose a* is 1e-9 away from the threshold is decided alike by both."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _mining_ref as MR  # noqa: E402

DEV = "cuda:0"
BAND = 1e-9


def unpack(bits, pitch_check=None):
    """device int32 [H, pitch] -> bool [H, 32 * pitch]: bit x & 31 of dword x >> 5"""
    w = bits.cpu().numpy().view(np.uint32)
    if pitch_check is not None:
        assert w.shape[1] == pitch_check
    return ((w[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).astype(bool).reshape(w.shape[0], -1)


def pack(mask, pitch=None, pad=0):
    """bool [H, W] -> int32 [H, pitch] with the pad bits and pad dwords all ``pad``"""
    H, W = mask.shape
    words = (W + 31) // 32
    pitch = words if pitch is None else pitch
    full = np.full((H, 32 * pitch), bool(pad))
    full[:, :W] = mask
    w = (full.reshape(H, pitch, 32).astype(np.uint32) << np.arange(32, dtype=np.uint32)).sum(axis=2, dtype=np.uint64).astype(np.uint32)
    return torch.from_numpy(w.view(np.int32).copy())


_PYR = {}


def pyramid(seed, *size):
    if (seed,) + size not in _PYR:
        _PYR[(seed,) + size] = MR.synthetic_pyramid(seed, *size)
    return _PYR[(seed,) + size]


def dev(a):
    return torch.as_tensor(a).to(DEV)


def lin_dev():
    from ssl_cr_histo_amd import mining
    return dev(mining.srgb_linear_table())


# ------------------------------------------------------------------------------------------------ 1. bits
S01 = [(250, 240, 225), (10, 9, 9), (200, 180, 190), (100, 95, 90), (20, 18, 19), (255, 250, 229), (30, 27, 28), (40, 36, 36),
       (90, 81, 85), (110, 99, 100)]                                # s = 0.1 in the reals: delta / max = 1 / 10


def special_image(W, H=6):
    """the s = 0.1 pixels in every channel rotation, black, white, greys, near-threshold neighbours, and a random lot"""
    px = []
    for p in S01:
        px += [p, (p[1], p[2], p[0]), (p[2], p[0], p[1]), (p[0], p[1] - 1, p[2]), (p[0], min(p[1] + 1, 255), p[2])]
    px += [(0, 0, 0), (255, 255, 255), (1, 1, 1), (1, 0, 0), (0, 0, 1), (128, 128, 128), (255, 229, 255), (255, 230, 255), (255, 229, 229)]
    rs = np.random.RandomState(40 + W)
    px = np.concatenate([np.array(px, np.uint8), rs.randint(0, 256, (H * W, 3)).astype(np.uint8)])[:H * W]
    return px[rs.permutation(H * W)].reshape(H, W, 3)


@pytest.mark.parametrize("W", [70, 64, 33])
@pytest.mark.parametrize("extra_pitch", [0, 1])
def test_hsv_s_bits_equal_the_restatement(W, extra_pitch):
    from ssl_cr_histo_amd import kernels as K
    img = special_image(W)
    words = (W + 31) // 32
    out = torch.full((img.shape[0], words + extra_pitch), -1, dtype=torch.int32, device=DEV)      # every dword must be overwritten
    got = unpack(K.tissue_bits(dev(img), "hsv_s", 0.1, pitch=words + extra_pitch, out=out), words + extra_pitch)
    want = MR.foreground_pixels_v2(img, 0.1)
    assert 0 < want.sum() < want.size
    assert np.array_equal(got[:, :W], want), np.argwhere(got[:, :W] != want)[:5]
    assert not got[:, W:].any(), "pad bits must be zero"


def test_hsv_s_bits_on_a_slide_and_other_thresholds():
    from ssl_cr_histo_amd import kernels as K
    img = pyramid(0).levels[2]
    d = dev(img)
    for thr in (0.1, 0.0, 0.39, 1.0):
        got = unpack(K.tissue_bits(d, "hsv_s", thr))
        assert np.array_equal(got[:, :img.shape[1]], MR.foreground_pixels_v2(img, thr)), thr
        assert not got[:, img.shape[1]:].any()


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_lab_a_bits_equal_outside_an_empty_band(seed):
    """the threshold as a host double, then read on the device from sslcr_lab_a_sum (no sync between the launches)"""
    from ssl_cr_histo_amd import kernels as K
    P = pyramid(seed)
    img = P.levels[2]
    W = img.shape[1]
    mu = MR.mean_a(P.overview)
    thr = (1 + 0.15) * mu
    a = MR.lab_a_rows(img)
    assert int((np.abs(a - thr) < BAND).sum()) == 0, "the inputs must leave the band empty"
    want = a > thr
    lin = lin_dev()
    got = unpack(K.tissue_bits(dev(img), "lab_a", thr, lin=lin))
    assert np.array_equal(got[:, :W], want) and not got[:, W:].any()
    ov = dev(P.overview)
    total = K.lab_a_sum(ov, lin)
    got = unpack(K.tissue_bits(dev(img), "lab_a", lin=lin, thr_sum=total, factor=1 + 0.15, count=float(P.overview.shape[0] * P.overview.shape[1])))
    assert np.array_equal(got[:, :W], want) and not got[:, W:].any()
    if seed != 1:
        assert 0.1 < want.mean() < 0.9


def test_lab_a_bits_widths():
    from ssl_cr_histo_amd import kernels as K
    lin = lin_dev()
    for W in (70, 64, 33):
        img = special_image(W)
        a = MR.lab_a_rows(img)
        thr = 5.0
        assert int((np.abs(a - thr) < BAND).sum()) == 0
        got = unpack(K.tissue_bits(dev(img), "lab_a", thr, lin=lin))
        assert np.array_equal(got[:, :W], a > thr) and not got[:, W:].any()


def test_lab_a_bits_with_thresholds_next_to_pixels():
    """thresholds 1e-6 above and below the a* of pixels of the image: closer than any float32 evaluation can resolve (the kernel's
    float32 screen must hand these pixels to its float64 chain), 1000 times the band the test keeps empty"""
    from ssl_cr_histo_amd import kernels as K
    img = pyramid(2).levels[2]
    W = img.shape[1]
    a = MR.lab_a_rows(img)
    lin, d = lin_dev(), dev(img)
    flat = a.reshape(-1)
    picks = flat[np.random.RandomState(9).permutation(flat.size)[:6]]
    for thr in [v + s * 1e-6 for v in picks for s in (1, -1)]:
        assert int((np.abs(a - thr) < BAND).sum()) == 0
        assert int((np.abs(a - thr) < 2e-6).sum()) >= 1
        got = unpack(K.tissue_bits(d, "lab_a", float(thr), lin=lin))
        assert np.array_equal(got[:, :W], a > thr), (thr, np.argwhere(got[:, :W] != (a > thr))[:5])


# ------------------------------------------------------------------------------------------------ 2. sum
@pytest.mark.parametrize("which", ["overview", "level1", "random"])
def test_lab_a_sum(which):
    from ssl_cr_histo_amd import kernels as K
    if which == "random":                                           # 300 000 pixels: more than one pixel per thread of a slice
        img = np.random.RandomState(77).randint(0, 256, (500, 600, 3)).astype(np.uint8)
    else:
        img = pyramid(0).overview if which == "overview" else pyramid(0).levels[1]
    a = MR.lab_a_rows(img)
    n = a.size
    lin, d = lin_dev(), dev(img)
    s1, s2 = K.lab_a_sum(d, lin), K.lab_a_sum(d, lin)
    got = s1.item()
    bound = 1e-12 * n + n * 2.0 ** -53 * np.abs(a).sum()
    print(f"lab_a_sum[{which}]: n = {n}, got {got!r}, numpy {a.sum()!r}, |diff| = {abs(got - a.sum()):.3e}, bound {bound:.3e}")
    assert abs(got - a.sum()) <= bound
    assert s1.cpu().numpy().tobytes() == s2.cpu().numpy().tobytes(), "two runs must be bit-equal"


# ------------------------------------------------------------------------------------------------ 3. popcount
def window_counts(mask, tile, stride):
    (ph, pw), (sh, sw) = tile, stride
    H, W = mask.shape
    ys, xs = range(sh, H - 1 - ph, sh), range(sw, W - 1 - pw, sw)
    return np.array([[mask[y:y + ph, x:x + pw].sum() for x in xs] for y in ys], dtype=np.int32).reshape(len(ys), len(xs))


def check_popcount(mask, tile, stride, thresh, pitch=None, pad=0):
    from ssl_cr_histo_amd import kernels as K
    tile, stride = (tile, tile) if np.isscalar(tile) else tile, (stride, stride) if np.isscalar(stride) else stride
    count, keep = K.tile_popcount(pack(mask, pitch, pad).to(DEV), mask.shape[1], tile, stride, thresh)
    want = window_counts(mask, tile, stride)
    assert count.dtype == torch.int32 and keep.dtype == torch.uint8 and tuple(count.shape) == tuple(keep.shape) == want.shape
    assert np.array_equal(count.cpu().numpy(), want)
    want_keep = np.array([[c / (tile[0] * tile[1]) >= thresh for c in row] for row in want.tolist()], dtype=bool).reshape(want.shape)
    assert np.array_equal(keep.cpu().numpy().astype(bool), want_keep)
    return want, want_keep


@pytest.mark.parametrize("tile,stride", [(20, 7), (16, 8), (32, 16), (5, 3), (40, 9), ((20, 16), (7, 8))])
def test_tile_popcount_equals_numpy(tile, stride):
    tissue = MR.foreground_pixels_v2(pyramid(0).levels[2])                       # 134 x 90: windows at every bit offset
    _, keep = check_popcount(tissue, tile, stride, 0.75)
    if tile in (20, 16, 5):
        assert keep.any() and not keep.all()
    rnd = np.random.RandomState(5).random_sample((90, 134)) < 0.5
    check_popcount(rnd, tile, stride, 0.5)
    check_popcount(rnd, tile, stride, 0.5, pitch=6, pad=1)                        # set pad bits and a pad dword: never counted


def test_tile_popcount_aligned_64_at_width_200():
    rnd = np.random.RandomState(6).random_sample((140, 200)) < 0.7
    want, _ = check_popcount(rnd, 64, 64, 0.7)
    assert want.shape == (1, 2)


@pytest.mark.parametrize("nset,kept", [(380, True), (379, False)])
def test_tile_popcount_at_the_threshold(nset, kept):
    """380 / 400 >= 0.95 is kept, 379 / 400 is not: the reference's own division and comparison"""
    mask = np.zeros((45, 60), bool)
    win = np.zeros(400, bool)
    win[np.random.RandomState(nset).permutation(400)[:nset]] = True
    mask[7:27, 7:27] = win.reshape(20, 20)
    want, keep = check_popcount(mask, 20, 7, 0.95)
    assert want[0, 0] == nset and bool(keep[0, 0]) is kept
    mask16 = np.zeros((40, 40), bool)                               # 192 / 256 >= 0.75 at tile 16
    flat = np.zeros(256, bool)
    flat[:192 if kept else 191] = True
    mask16[8:24, 8:24] = flat.reshape(16, 16)
    want, keep = check_popcount(mask16, 16, 8, 0.75)
    assert bool(keep[0, 0]) is kept


def test_tile_popcount_empty_grid_and_a_slide_without_tissue():
    from ssl_cr_histo_amd import kernels as K
    count, keep = K.tile_popcount(pack(np.ones((18, 134), bool)).to(DEV), 134, (16, 16), (8, 8), 0.5)
    assert tuple(count.shape) == (0, 14) and tuple(keep.shape) == (0, 14)
    count, keep = K.tile_popcount(pack(np.ones((90, 20), bool)).to(DEV), 20, (20, 20), (7, 7), 0.5)
    assert tuple(count.shape) == (9, 0)
    P = pyramid(1)
    lr2 = dev(P.levels[2])
    for tile, stride in ((16, 8), (20, 7)):
        bits = K.tissue_bits(lr2, "hsv_s", 0.1)
        count, keep = K.tile_popcount(bits, 134, (tile, tile), (stride, stride), 0.75)
        assert np.array_equal(count.cpu().numpy(), window_counts(MR.foreground_pixels_v2(P.levels[2]), (tile, tile), (stride, stride)))
        assert not keep.cpu().numpy().any()


# ------------------------------------------------------------------------------------------------ 4. gather
LEVEL_HW = ((40, 52), (30, 37), (23, 29))
T_GATHER = 7


def gather_case(S, fill, src_off=(0, 0, 0)):
    """three random levels (each a view ``src_off`` bytes into its buffer), xy tables with tiles inside, across every edge and wholly
    outside, and what slicing + sorted_sequence give: Data_1..3 as uint8 [6 T, 3, S, S], labels [6 T]"""
    rs = np.random.RandomState(100 + S)
    levels = [rs.randint(0, 256, (h, w, 3)).astype(np.uint8) for h, w in LEVEL_HW]
    xy = []
    for h, w in LEVEL_HW:
        t = np.stack([rs.randint(0, w - S, T_GATHER), rs.randint(0, h - S, T_GATHER)], axis=1)
        t[1] = (-3, 2)
        t[2] = (w - S + 2, h - S + 1)
        t[3] = (5, -S + 1)
        t[4] = (-S - 4, 3)                                          # wholly outside
        t[5] = (w - 1, h - 1)
        xy.append(t.astype(np.int32))
    P = MR.Pyramid(levels, (1.0, 1.0, 1.0))
    tiles = [np.stack([P.read_region((int(x), int(y)), l, (S, S), fill) for x, y in xy[l]]) for l in range(3)]
    d1, d2, d3, lab = MR.sorted_sequence(*tiles)
    want = [np.ascontiguousarray(d.transpose(0, 3, 1, 2)) for d in (d1, d2, d3)]
    dl = []
    for lv, off in zip(levels, src_off):
        buf = torch.zeros(lv.size + 8, dtype=torch.uint8, device=DEV)
        buf[off:off + lv.size] = dev(lv.reshape(-1))
        dl.append(buf[off:off + lv.size].view(lv.shape))
    return dl, [dev(t) for t in xy], want, lab.reshape(-1).astype(np.int64)


@pytest.mark.parametrize("S", [8, 6])
@pytest.mark.parametrize("src_off", [(0, 0, 0), (1, 2, 3)])
def test_rsp_gather_equals_slicing_and_sorted_sequence(S, src_off):
    from ssl_cr_histo_amd import kernels as K
    levels, xy, want, lab = gather_case(S, 9, src_off)
    n = 6 * T_GATHER
    for idx in (np.arange(n), np.random.RandomState(S).permutation(n), np.array([41, 0, 0, 17, 41, 6])):
        d1, d2, d3, label = K.rsp_gather(levels, xy, dev(idx.astype(np.int64)), S, fill=9)
        for slot, (got, w) in enumerate(zip((d1, d2, d3), want)):
            assert got.dtype == torch.uint8 and tuple(got.shape) == (len(idx), 3, S, S)
            assert np.array_equal(got.cpu().numpy(), w[idx]), (slot, S, src_off)
        assert label.dtype == torch.int64 and np.array_equal(label.cpu().numpy(), lab[idx]) and np.array_equal(lab[idx], idx % 6)


@pytest.mark.parametrize("S", [8, 6])
def test_rsp_gather_into_odd_output_bases_and_guards(S):
    """outputs 1, 2 and 3 bytes past a dword boundary take the per-byte path; the bytes on either side of every output stay"""
    from ssl_cr_histo_amd import kernels as K
    levels, xy, want, lab = gather_case(S, 0)
    idx = np.random.RandomState(3).permutation(6 * T_GATHER)[:11]
    sz = 11 * 3 * S * S
    bufs = [torch.full((sz + 16,), 0xA5, dtype=torch.uint8, device=DEV) for _ in range(3)]
    outs = tuple(b[4 + o:4 + o + sz].view(11, 3, S, S) for b, o in zip(bufs, (1, 2, 3)))
    lbuf = torch.full((13,), -7, dtype=torch.int64, device=DEV)
    K.rsp_gather(levels, xy, dev(idx.astype(np.int64)), S, fill=0, out=outs + (lbuf[1:12],))
    for b, o, w in zip(bufs, (1, 2, 3), want):
        h = b.cpu().numpy()
        assert np.array_equal(h[4 + o:4 + o + sz].reshape(11, 3, S, S), w[idx])
        assert (h[:4 + o] == 0xA5).all() and (h[4 + o + sz:] == 0xA5).all()
    assert lbuf.cpu().tolist() == [-7] + list(lab[idx]) + [-7]


def test_rsp_gather_index_outside_the_dataset_reads_nothing():
    from ssl_cr_histo_amd import kernels as K
    levels, xy, want, lab = gather_case(8, 9)
    idx = np.array([3, 6 * T_GATHER, -1, 5], dtype=np.int64)
    d1, d2, d3, label = K.rsp_gather(levels, xy, dev(idx), 8, fill=9)
    assert label.cpu().tolist() == [3, -1, -1, 5]
    for got, w in zip((d1, d2, d3), want):
        g = got.cpu().numpy()
        assert np.array_equal(g[0], w[3]) and np.array_equal(g[3], w[5]) and (g[1:3] == 9).all()


# ------------------------------------------------------------------------------------------------ 5. loader
TILE, STRIDE, SIZE = 64, 32, (200, 170)     # the RSP tests' smallest tile; level 2 of 200 x 170: 12 candidates, 3 (v1) / 5 (v2) kept


def host_pipeline(P, variant, fill=0):
    hr, lr1, lr2, kept = MR.get_wsi_patches(P, TILE, STRIDE, variant, fill)
    d1, d2, d3, lab = MR.sorted_sequence(hr, lr1, lr2)
    return [np.ascontiguousarray(d.transpose(0, 3, 1, 2)) for d in (d1, d2, d3)], lab.reshape(-1).astype(np.int64), kept


def make_loader(P, variant, batch_size, **kw):
    from ssl_cr_histo_amd import mining
    return mining.RspDeviceLoader(P.levels, P.level_downsamples, TILE, STRIDE, batch_size, variant=variant, overview=P.overview,
                                  device=DEV, **kw)


@pytest.mark.parametrize("variant", ["v1", "v2"])
def test_loader_equals_the_host_pipeline_batch_for_batch(variant):
    P = pyramid(0, *SIZE)
    if variant == "v1":
        thr = 1.15 * MR.mean_a(P.overview)
        assert int((np.abs(MR.lab_a_rows(P.levels[2]) - thr) < BAND).sum()) == 0
    want, lab, kept = host_pipeline(P, variant, fill=3)
    n = 6 * len(kept)
    assert len(kept) >= 2
    loader = make_loader(P, variant, 4, fill=3)
    assert loader.triplets == len(kept) and list(zip(loader.xpos, loader.ypos)) == kept
    assert len(loader) == (n + 3) // 4
    batches = list(loader)
    assert len(batches) == len(loader)
    for b, (d1, d2, d3, label) in enumerate(batches):
        lo, hi = 4 * b, min(4 * b + 4, n)
        for got, w in zip((d1, d2, d3), want):
            assert got.is_cuda and got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), w[lo:hi]), (variant, b)
        assert np.array_equal(label.cpu().numpy(), lab[lo:hi])
    # drop_last and a shuffled epoch: the permutation torch.randperm draws from the generator, applied to the same virtual dataset
    assert len(make_loader(P, variant, 4, drop_last=True)) == n // 4
    g = torch.Generator().manual_seed(11)
    shuffled = make_loader(P, variant, 5, fill=3, shuffle=True, generator=g)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(11)).numpy()
    epoch = list(shuffled)                                          # ONE epoch: every iteration draws a new permutation
    assert len(epoch) == len(shuffled) == (n + 4) // 5
    got = [torch.cat([b[k] for b in epoch]).cpu().numpy() for k in range(4)]
    for k in range(3):
        assert np.array_equal(got[k], want[k][perm])
    assert np.array_equal(got[3], lab[perm])


def test_loader_on_a_slide_without_tissue():
    P = pyramid(1)
    from ssl_cr_histo_amd import mining
    loader = mining.RspDeviceLoader(P.levels, P.level_downsamples, 16, 8, 4, variant="v2", device=DEV)
    assert loader.triplets == 0 and len(loader) == 0 and list(loader) == []
    assert loader.keep.shape == (9, 14) and not loader.keep.any()


def test_rsp_train_epoch_fed_by_the_loader_has_the_bits_of_host_batches():
    """one rsp_train epoch of two batches: the loader's device batches against the same uint8 batches built on the host"""
    from ssl_cr_histo_amd import steps
    from test_engine_gpu import _engine, build, ns, state_of
    _engine("fp32")
    P = pyramid(0, *SIZE)
    want, lab, kept = host_pipeline(P, "v1")
    n = 6 * len(kept)
    bs = n // 2
    assert n % 2 == 0 and bs >= 2
    host = [tuple(torch.from_numpy(w[lo:lo + bs]) for w in want) + (torch.from_numpy(lab[lo:lo + bs].astype(np.uint8)).view(-1, 1),)
            for lo in (0, bs)]
    loader = make_loader(P, "v1", bs)
    assert len(loader) == 2

    def run(batches):
        model, cls = build("triplet", "mlp", 6, False)
        opt = torch.optim.SGD(list(model.parameters()) + list(cls.parameters()), lr=0.01, momentum=0.9, weight_decay=1e-4, nesterov=True)
        ret = steps.rsp_train(ns(tile_h=TILE, tile_w=TILE), model, cls, batches, torch.nn.CrossEntropyLoss(), opt, 1)
        return ret, state_of(model, cls)
    (l1, a1, f1, t1), s1 = run(loader)
    (l0, a0, f0, t0), s0 = run(host)
    assert l1 == l0 and a1 == a0
    assert torch.equal(f1.cpu(), f0.cpu()) and torch.equal(t1.cpu(), t0.cpu())
    assert np.array_equal(t1.cpu().numpy(), lab)
    for key, v in s0.items():
        assert torch.equal(v, s1[key]), key
