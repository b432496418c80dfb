"""Test-time augmentation over D4 on the MI355X.  The bound everywhere is equality: the two byte kernels against
``inference.d4_apply`` (NumPy), the ensemble reduce against the float32 left-to-right mean of what ``sslcr_predict`` itself returns
for every member, and ``test()`` with ``args.tta`` against an oracle built from the existing code only -- today's ``test()`` on
host-oriented copies of the same tiles, one run per orientation, averaged in float32 in the order listed."""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import cases as C  # noqa: E402
from oracle import model as OM  # noqa: E402

from _inference_util import cut_tiles, scale_head  # noqa: E402

DEV = "cuda:0"


def _engine(dtype):
    from ssl_cr_histo_amd import engine as E
    idx = torch.device(DEV).index
    cur = E._engines.get(idx)
    if cur is None or cur.dtype != E._DTYPES[dtype]:
        E._engines.pop(idx, None)
        E.set_engine(E.Engine(DEV, dtype))
    return E.get_engine(DEV)


def build(classes, head_scale=1.0):
    from ssl_cr_histo_amd import net
    model, cls = net.TripletNet_Finetune("resnet18"), net.FinetuneResNet(classes)
    model.load_state_dict(OM.init_state(C.PARAM_SEED, OM.net_param_specs(), random_running_stats=True))
    cls.load_state_dict(OM.init_state(C.PARAM_SEED + 1, OM.classifier_param_specs("finetune", classes)))
    scale_head(cls, head_scale)
    return model.to(DEV), cls.to(DEV)


def ns(**kw):
    return types.SimpleNamespace(print_freq=0, **kw)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8 if a.dtype == np.uint8 else np.uint32)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _ordered_mean(members):
    """the float32 left-to-right sum of the members divided by float32(G)"""
    acc = np.asarray(members[0], dtype=np.float32).copy()
    for m in members[1:]:
        acc = acc + np.asarray(m, dtype=np.float32)
    assert acc.dtype == np.float32
    return acc / np.float32(len(members))


# ---------------------------------------------------------------------------------------------------------------- d4_transform
ORIENT11 = np.array([0, 1, 2, 3, 4, 5, 6, 7, 5, 3, 6], dtype=np.int32)      # every code present, mixed


@pytest.mark.parametrize("dtype", ["uint8", "float32"])
@pytest.mark.parametrize("Cn", [1, 3])
@pytest.mark.parametrize("S", [1, 4, 5, 31, 32, 33, 64, 96, 128])
def test_d4_transform_equals_d4_apply(S, Cn, dtype):
    """random bytes (a symmetric input would let a wrong orientation pass); sides on both sides of a staging block (32 dwords for
    float32, 64 pixels for uint8), the per-element path (sides that are no multiple of four; an output base offset by one element)"""
    from ssl_cr_histo_amd import kernels as K
    from ssl_cr_histo_amd.inference import d4_apply
    rs = np.random.RandomState(1000 * S + 10 * Cn + len(dtype))
    N = len(ORIENT11)
    if dtype == "uint8":
        host = rs.randint(0, 256, size=(N, Cn, S, S), dtype=np.uint8)
    else:
        host = rs.randint(0, 1 << 32, size=(N, Cn, S, S), dtype=np.uint64).astype(np.uint32).view(np.float32)     # any bit pattern
    want = np.stack([d4_apply(host[n], int(ORIENT11[n])) for n in range(N)])
    x = torch.from_numpy(host).to(DEV)
    orient = torch.from_numpy(ORIENT11).to(DEV)
    got = K.d4_transform(x, orient)
    assert got.shape == x.shape and got.dtype == x.dtype and got.data_ptr() != x.data_ptr()
    assert np.array_equal(_bits(got.cpu().numpy()), _bits(want))
    assert np.array_equal(_bits(x.cpu().numpy()), _bits(host))                      # out of place: the source is untouched
    # an output (and then a source) base offset by one element
    flat = torch.zeros(x.numel() + 1, dtype=x.dtype, device=DEV)
    out = flat[1:].view(x.shape)
    assert K.d4_transform(x, orient, out=out) is out
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(want))
    flat2 = torch.zeros(x.numel() + 1, dtype=x.dtype, device=DEV)
    flat2[1:].copy_(x.view(-1))
    assert np.array_equal(_bits(K.d4_transform(flat2[1:].view(x.shape), orient).cpu().numpy()), _bits(want))
    # one code for the whole batch, every code in turn; N = 0 is a no-op
    for g in range(8):
        table = torch.full((N,), g, dtype=torch.int32, device=DEV)
        assert np.array_equal(_bits(K.d4_transform(x, table).cpu().numpy()), _bits(d4_apply(host, g))), g
    assert K.d4_transform(x[:0], orient[:0]).shape == (0, Cn, S, S)


def test_d4_transform_refuses_overlap_and_non_square():
    from ssl_cr_histo_amd import _lib as L
    from ssl_cr_histo_amd import kernels as K
    x = torch.zeros((2, 3, 8, 8), dtype=torch.uint8, device=DEV)
    o = torch.zeros(2, dtype=torch.int32, device=DEV)
    with pytest.raises(L.SslcrError, match="overlap"):
        K.d4_transform(x, o, out=x)
    with pytest.raises(L.SslcrError, match="square"):
        K.d4_transform(torch.zeros((2, 3, 8, 12), dtype=torch.uint8, device=DEV), o)


# ---------------------------------------------------------------------------------------------------------------- wsi_gather_d4
RH, RW = 40, 52
ORIGIN = (1000, 2000)


def _tile_table(S):
    """region coordinates: fully inside at all four residues of the left edge mod 4 (where S allows), across each of the four edges,
    across two corners, wholly outside on either side"""
    return np.array([(8, 4), (9, 4), (10, 4), (11, 4), (0, 0), (RW - S, RH - S), (-3, 10), (RW - S + 3, 10), (10, -2), (12, RH - S + 1),
                     (-1, -1), (RW - S + 1, RH - S + 2), (RW + 5, RH + 7), (-2 * S, -2 * S), (RW - 1, RH - 1)])


@pytest.mark.parametrize("fill", [0, 255])
@pytest.mark.parametrize("S", [5, 8, 12, 64])
def test_wsi_gather_d4_equals_d4_apply_of_numpy_slicing(S, fill):
    from ssl_cr_histo_amd import kernels as K
    from ssl_cr_histo_amd.inference import d4_apply
    tiles = _tile_table(S)
    T = len(tiles)
    xy = np.repeat(tiles, 8, axis=0) + np.array(ORIGIN)                        # every tile under all eight codes
    codes = np.tile(np.arange(8, dtype=np.int32), T)
    xy_d = torch.from_numpy(xy.astype(np.int32)).to(DEV)
    for off in (1, 2, 3, 0):                                                   # the source base: every alignment
        host = np.random.RandomState(77 + off).randint(0, 256, size=(RH, RW, 3), dtype=np.uint8)
        flat = torch.zeros(RH * RW * 3 + 4, dtype=torch.uint8, device=DEV)
        region = flat[off:off + RH * RW * 3].view(RH, RW, 3)
        region.copy_(torch.from_numpy(host))
        assert region.data_ptr() % 4 == off and region.is_contiguous()
        plain = cut_tiles(host, xy, S, origin=ORIGIN, fill=fill)
        want = np.stack([d4_apply(plain[n], int(codes[n])) for n in range(len(xy))])
        got = K.wsi_gather(region, xy_d, S, origin=ORIGIN, fill=fill, orient=torch.from_numpy(codes).to(DEV))
        assert got.shape == (8 * T, 3, S, S) and got.dtype == torch.uint8
        assert np.array_equal(got.cpu().numpy(), want), off
        if S <= 12:                                                            # the table has what its docstring says
            assert all((plain[8 * t] != fill).any() for t in range(6))
        assert (plain[8 * 12] == fill).all() and (plain[8 * 13] == fill).all()
        # orient = None and an all-zero table: the bytes of sslcr_wsi_gather
        ref = K.wsi_gather(region, xy_d, S, origin=ORIGIN, fill=fill).cpu().numpy()
        assert np.array_equal(ref, plain)
        zero = K.wsi_gather(region, xy_d, S, origin=ORIGIN, fill=fill, orient=torch.zeros(8 * T, dtype=torch.int32, device=DEV))
        assert np.array_equal(zero.cpu().numpy(), ref)
        # an output base offset by one byte: the per-byte path of the oriented gather
        buf = torch.zeros(8 * T * 3 * S * S + 1, dtype=torch.uint8, device=DEV)
        out = buf[1:].view(8 * T, 3, S, S)
        K.wsi_gather(region, xy_d, S, origin=ORIGIN, fill=fill, out=out, orient=torch.from_numpy(codes).to(DEV))
        assert np.array_equal(out.cpu().numpy(), want)
        assert int(buf[0]) == 0


def test_wsi_gather_d4_on_tiles_of_several_blocks():
    """256-pixel tiles (4 x 4 staging blocks) from a region they cross: every code, through the loader's one-code-per-range form"""
    from ssl_cr_histo_amd.inference import WsiDeviceLoader, d4_apply, tile_origins
    rs = np.random.RandomState(9)
    slide = rs.randint(0, 256, size=(384, 512, 3), dtype=np.uint8)
    mask = np.ones((4, 3), bool)
    loader = WsiDeviceLoader(slide, mask, 256, 5, resolution=128)
    _, _, xy = tile_origins(mask, 128, 256)
    plain = cut_tiles(slide, xy, 256)
    assert np.array_equal(loader.tiles(0, 12).cpu().numpy(), plain)
    for g in range(8):
        assert np.array_equal(loader.tiles(2, 7, orient=g).cpu().numpy(), d4_apply(plain[2:7], g)), g
    with pytest.raises(ValueError):
        loader.tiles(0, 4, orient=8)


# ---------------------------------------------------------------------------------------------------------------- predict_tta
def _lowest_max(s):
    """lowest index of the row maximum; a NaN counts as the maximum"""
    out = np.empty(len(s), np.int64)
    for i, row in enumerate(s):
        nan = np.isnan(row)
        out[i] = int(np.argmax(nan)) if nan.any() else int(np.argmax(row))
    return out


def _confusion(y, pred, Cn):
    cm = np.zeros((Cn, Cn), np.int64)
    for t, p in zip(y, pred):
        if 0 <= t < Cn:
            cm[t, p] += 1
    return cm


@pytest.mark.parametrize("Cn", [1, 2, 9, 64])
@pytest.mark.parametrize("n", [1, 7, 300])
@pytest.mark.parametrize("G", [1, 2, 3, 8])
def test_predict_tta_is_the_ordered_mean_of_predict(G, n, Cn):
    from ssl_cr_histo_amd import kernels as K
    rs = np.random.RandomState(10000 * G + 100 * n + Cn)
    l = (rs.standard_normal((G, n, Cn)) * 2.5).astype(np.float32)
    if n > 1:
        l[G - 1, 3, rs.permutation(Cn)[:max(1, Cn // 2)]] = np.nan            # one member's row 3 holds NaNs
        l[:, 5] = l[0, 5]                                                     # every member agrees on row 5
    y = rs.randint(0, Cn, n).astype(np.int64)
    y[::5] = -100                                                             # rows the confusion matrix skips
    if n > 2:
        y[2::11] = Cn
    valid = int(((y >= 0) & (y < Cn)).sum())
    ld, yd = torch.from_numpy(l).to(DEV), torch.from_numpy(y).to(DEV)
    members = [K.predict(ld[g], scores=True, pred=False)["scores"].cpu().numpy() for g in range(G)]
    want = _ordered_mean(members)
    perm = torch.from_numpy(rs.permutation(n + 13)[:n].astype(np.int64))

    cm = torch.zeros((Cn, Cn), dtype=torch.int64, device=DEV)
    m = torch.zeros(n + 13, dtype=torch.float32, device=DEV)
    out = K.predict_tta(ld, yd, scores=True, pred=True, confusion=cm, col=-1, map=m, map_index=perm.to(DEV))
    sc, pred = out["scores"].cpu().numpy(), out["pred"].cpu().numpy()
    assert sc.dtype == np.float32 and pred.dtype == np.int64
    finite = ~np.isnan(want)
    assert np.array_equal(np.isnan(sc), np.isnan(want))
    assert np.array_equal(_bits(sc)[finite], _bits(want)[finite])
    if n > 1:
        assert np.isnan(sc[3]).all()                                          # a NaN logit makes its member's row NaN, and the mean's
        if G <= 2:                                                            # (p + p) / 2 is exact
            assert np.array_equal(_bits(sc[5]), _bits(members[0][5]))
    if G == 1:                                                                # (the scores above ARE sslcr_predict's: want = members[0] / 1)
        assert np.array_equal(pred, K.predict(ld[0])["pred"].cpu().numpy())
    else:
        assert np.array_equal(pred, _lowest_max(want))
        if n > 1:
            assert pred[3] == 0                                               # the whole row is NaN: its lowest index wins
    assert np.array_equal(cm.cpu().numpy(), _confusion(y, pred, Cn))
    assert int(cm.sum()) == valid                                             # once per row, not once per member
    K.predict_tta(ld, yd, pred=False, confusion=cm)                           # accumulates across calls
    assert int(cm.sum()) == 2 * valid
    want_map = np.zeros(n + 13, np.float32)
    want_map[perm.numpy()] = sc[:, -1]
    got_map = m.cpu().numpy()
    assert np.array_equal(np.isnan(got_map), np.isnan(want_map))
    assert np.array_equal(_bits(got_map)[~np.isnan(want_map)], _bits(want_map)[~np.isnan(want_map)])
    if G == 1:                                                                # every output has sslcr_predict's bits
        cm1 = torch.zeros((Cn, Cn), dtype=torch.int64, device=DEV)
        m1 = torch.zeros(n + 13, dtype=torch.float32, device=DEV)
        K.predict(ld[0], yd, pred=False, confusion=cm1, col=-1, map=m1, map_index=perm.to(DEV))
        assert torch.equal(2 * cm1, cm)
        keep = ~torch.isnan(m1)
        assert torch.equal(torch.isnan(m), torch.isnan(m1)) and torch.equal(m[keep].view(torch.int32), m1[keep].view(torch.int32))
    # mode 1: the ordered mean of the raw rows
    raw = K.predict_tta(ld, mode=1, scores=True, pred=False)["scores"].cpu().numpy()
    want_raw = _ordered_mean(list(l))
    fin = ~np.isnan(want_raw)
    assert np.array_equal(np.isnan(raw), ~fin) and np.array_equal(_bits(raw)[fin], _bits(want_raw)[fin])
    assert K.predict_tta(ld[:, :0], pred=True)["pred"].shape == (0,)          # n = 0: a no-op


def test_predict_tta_tie_nan_and_g1_rules():
    from ssl_cr_histo_amd import _lib as L
    from ssl_cr_histo_amd import kernels as K
    # an exact tie: the second member is the first with its columns swapped -> both means are p + q; index 0 wins
    a = np.random.RandomState(3).standard_normal((50, 2)).astype(np.float32) * 3
    l = torch.from_numpy(np.stack([a, a[:, ::-1].copy()])).to(DEV)
    out = K.predict_tta(l, scores=True)
    sc = out["scores"].cpu().numpy()
    assert np.array_equal(_bits(sc[:, 0]), _bits(sc[:, 1])) and (np.abs(a[:, 0] - a[:, 1]) > 0.1).any()
    assert out["pred"].cpu().tolist() == [0] * 50
    # NaN: mode 1 keeps a NaN where it stands, and the lowest NaN index wins over any number
    r = torch.tensor([[[1.0, 5.0, 2.0, 0.0]], [[1.0, float("nan"), float("inf"), float("nan")]]], device=DEV)
    raw = K.predict_tta(r, mode=1, scores=True, pred=False)["scores"].cpu().numpy()
    assert np.isnan(raw[0]).tolist() == [False, True, False, True] and raw[0, 0] == 1.0 and raw[0, 2] == np.inf
    # G = 1: the argmax is sslcr_predict's, over the logits -- two different logits whose probabilities round to one value
    t = torch.tensor([[[0.1, np.nextafter(np.float32(0.1), np.float32(1.0))]]], dtype=torch.float32, device=DEV)
    assert K.predict(t[0])["pred"].cpu().tolist() == [1] and K.predict_tta(t)["pred"].cpu().tolist() == [1]
    for bad in (dict(mode=1), dict(mode=1, pred=False, map=torch.zeros(4, device=DEV), map_index=torch.zeros(1, dtype=torch.int64, device=DEV)),
                dict(mode=2)):
        with pytest.raises(L.SslcrError):
            K.predict_tta(r, **bad)
    with pytest.raises(L.SslcrError, match="G = 9"):
        K.predict_tta(torch.zeros((9, 2, 3), device=DEV))


# ---------------------------------------------------------------------------------------------------------------- end to end: WSI
S_WSI, B_WSI = 64, 4


def _wsi_case():
    rs = np.random.RandomState(41)
    slide = rs.randint(0, 256, size=(160, 200, 3), dtype=np.uint8)                # [RH, RW, 3]
    mask = np.ones((3, 3), bool)                                                   # indexed [x, y]; resolution 64: 9 tiles, the last batch short
    return slide, mask


def _host_loader(slide, mask, g):
    """today's host-fed loader of the tiles in orientation g, cut and turned on the host"""
    from ssl_cr_histo_amd.inference import d4_apply, tile_origins
    x_idcs, y_idcs, xy = tile_origins(mask, 64, S_WSI)
    tiles = d4_apply(cut_tiles(slide, xy, S_WSI), g)
    n = len(x_idcs)
    return C.WsiLoader(mask, [(torch.from_numpy(tiles[i:i + B_WSI]), torch.from_numpy(x_idcs[i:i + B_WSI].copy()),
                               torch.from_numpy(y_idcs[i:i + B_WSI].copy())) for i in range(0, n, B_WSI)])


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_wsi_tta_map_equals_the_ordered_mean_of_todays_maps(dtype):
    from ssl_cr_histo_amd import steps
    from ssl_cr_histo_amd.inference import WsiDeviceLoader
    _engine(dtype)
    slide, mask = _wsi_case()
    model, cls = build(2, head_scale=0.05)
    loader = WsiDeviceLoader(slide, mask, S_WSI, B_WSI, resolution=64)
    assert 6 <= len(loader.dataset) <= 12 and len(loader.dataset) % B_WSI != 0
    # the oracle, from the existing code only: one plain run per orientation on host-oriented tiles
    maps = [steps.camelyon16_test(ns(), model, cls, _host_loader(slide, mask, g)).astype(np.float32) for g in range(8)]
    assert all(not np.array_equal(maps[0], maps[g]) for g in range(1, 8))          # the orientations do score differently
    assert np.array_equal(maps[0].astype(np.float64), steps.camelyon16_test(ns(), model, cls, loader))
    for spec, codes in (("d4", range(8)), ((3, 5), (3, 5)), ("flips", (0, 4, 6))):
        want = _ordered_mean([maps[g] for g in codes]).astype(np.float64)
        got = steps.camelyon16_test(ns(tta=spec), model, cls, loader)
        assert got.dtype == np.float64 and got.shape == mask.shape
        assert np.array_equal(got, want), (spec, float(np.abs(got - want).max()))
        if spec == "d4":
            assert np.array_equal(got, steps.camelyon16_test(ns(tta=spec), model, cls, loader))     # twice: the same bits
            assert got.std() > 1e-5                                                                   # a map that says something
        # a host-fed loader with args.tta: uploaded once, oriented on the device -- the same ensemble
        assert np.array_equal(steps.camelyon16_test(ns(tta=spec), model, cls, _host_loader(slide, mask, 0)), want), spec


# ---------------------------------------------------------------------------------------------------------------- end to end: test() drop-ins
def _kather_batches(g=0):
    from ssl_cr_histo_amd.inference import d4_apply
    return [(torch.from_numpy(d4_apply(C.u8(8100 + i, (n, 3, 64, 64)).numpy(), g)), C.ints(8150 + i, (n,), 9)) for i, n in enumerate((5, 5, 2))]


def _bpq_batches(g=0):
    from ssl_cr_histo_amd.inference import d4_apply
    return [(torch.from_numpy(d4_apply(C.u8(8200 + i, (n, 3, 64, 64)).numpy(), g)), C.f32(8250 + i, (n,)), C.f32(8280 + i, (n,)))
            for i, n in enumerate((4, 4, 3))]


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_kather_tests_with_rot90(dtype):
    from ssl_cr_histo_amd import steps
    _engine(dtype)
    model, cls = build(9, 0.05)
    plain = [steps.kather_cr_test(ns(), model, cls, _kather_batches(g)) for g in range(4)]
    want = _ordered_mean([p[2].numpy() for p in plain])
    pred, target, score = steps.kather_cr_test(ns(tta="rot90"), model, cls, _kather_batches())
    cm = steps.last_test_confusion()
    assert pred.shape == (12,) and pred.dtype == torch.int64 and not pred.is_cuda and not score.is_cuda
    assert _same_bits(score.numpy(), want)
    assert not _same_bits(score.numpy(), plain[0][2].numpy())                       # the ensemble is not the plain score
    assert np.array_equal(pred.numpy(), _lowest_max(want)) and torch.equal(pred, torch.argmax(score, 1))
    assert torch.equal(target, plain[0][1])
    assert cm.dtype == torch.int64 and np.array_equal(cm.numpy(), _confusion(target.numpy(), pred.numpy(), 9)) and int(cm.sum()) == 12
    pred2, target2 = steps.kather_sup_test(ns(tta="rot90"), model, cls, _kather_batches(), torch.nn.CrossEntropyLoss())
    assert torch.equal(pred2, pred) and torch.equal(target2, target)
    assert np.array_equal(steps.last_test_confusion().numpy(), cm.numpy())
    # tta = (0,) is the plain path's result through the ensemble kernels (G = 1)
    pred1, _, score1 = steps.kather_cr_test(ns(tta=(0,)), model, cls, _kather_batches())
    assert _same_bits(score1.numpy(), plain[0][2].numpy()) and torch.equal(pred1, plain[0][0])
    with pytest.raises(ValueError, match="square"):
        steps.kather_cr_test(ns(tta="rot90"), model, cls, [(torch.zeros((2, 3, 64, 96), dtype=torch.uint8), torch.zeros(2, dtype=torch.int64))])


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_bpq_tests_with_flips(dtype):
    from ssl_cr_histo_amd import steps
    _engine(dtype)
    model, cls = build(1)
    codes = (0, 4, 6)
    plain = [steps.bpq_test(ns(), model, cls, _bpq_batches(g)) for g in codes]
    want = _ordered_mean([p[0].numpy() for p in plain])
    out, feats, ta, tb = steps.bpq_test(ns(tta="flips"), model, cls, _bpq_batches())
    assert out.shape == (11,) and not out.is_cuda and _same_bits(out.numpy(), want)
    assert not _same_bits(out.numpy(), plain[0][0].numpy())
    assert _same_bits(feats.numpy(), plain[0][1].numpy())                          # features: the first listed orientation's
    assert torch.equal(ta, plain[0][2]) and torch.equal(tb, plain[0][3])
    assert steps.last_test_confusion() is None
    out2, feats2, _, _ = steps.bpq_sup_test(ns(tta=(6, 0)), model, cls, torch.nn.MSELoss(), _bpq_batches())
    assert _same_bits(out2.numpy(), _ordered_mean([plain[2][0].numpy(), plain[0][0].numpy()]))
    assert _same_bits(feats2.numpy(), plain[2][1].numpy())
