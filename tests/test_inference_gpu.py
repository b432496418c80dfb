"""Device-resident inference on the MI355X: the tile gather and the prediction kernel against host references, the device WSI loader
against the host-fed path of the same ``camelyon16_test`` (bit for bit), and the four ``test()`` drop-ins against the engine's own
forward (bit for bit) and against what the REFERENCE's test() functions returned (tests/golden/make_test_golden.py)."""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import cases as C  # noqa: E402
from oracle import model as OM  # noqa: E402

from _inference_util import (MARGIN, MARGIN_SHARE, TEST_CASES, bpq_test_batches, cut_tiles, kather_test_batches, scale_head,  # noqa: E402
                             softmax_rows_ref)
from _util import load_golden  # noqa: E402

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


# ---------------------------------------------------------------------------------------------------------------- kernels: gather
RH, RW = 300, 333                  # 999-byte rows: every row starts at another alignment
ORIGIN = (1000, 2000)


@pytest.fixture(scope="module")
def region():
    host = np.random.RandomState(21).randint(0, 256, size=(RH, RW, 3), dtype=np.uint8)
    return host, torch.from_numpy(host).to(DEV)


def _tile_table(S):
    """37 tiles in region coordinates: one crossing each edge, each corner, one wholly outside on either side, lefts of all four
    residues mod 4 fully inside, the rest seeded around the region"""
    rs = np.random.RandomState(100 + S)
    xy = np.stack([rs.randint(-S // 2, RW - S // 2 + 1, 37), rs.randint(-S // 2, RH - S // 2 + 1, 37)], 1)
    fixed = [(-3, 10), (RW - S + 3, 10), (10, -2), (12, RH - S + 1), (-1, -1), (RW - S + 1, RH - S + 2), (RW + 5, RH + 7), (-2 * S, -2 * S),
             (RW - 1, RH - 1), (8, 4), (9, 4), (10, 4), (11, 4)]
    xy[:len(fixed)] = fixed
    assert {int(v) % 4 for v in xy[9:13, 0]} == {0, 1, 2, 3}
    return xy


@pytest.mark.parametrize("fill", [0, 255])
@pytest.mark.parametrize("S", [5, 64, 224, 256])
def test_wsi_gather_equals_numpy_slicing(region, S, fill):
    from ssl_cr_histo_amd import inference as I
    host, dev = region
    xy = _tile_table(S) + np.array(ORIGIN)                       # level-0 coordinates
    got = I.gather_tiles(dev, torch.from_numpy(xy.astype(np.int32)).to(DEV), S, origin=ORIGIN, fill=fill)
    want = cut_tiles(host, xy, S, origin=ORIGIN, fill=fill)
    assert got.shape == (37, 3, S, S) and got.dtype == torch.uint8
    assert np.array_equal(got.cpu().numpy(), want)
    inside = [n for n in range(37) if 0 <= xy[n, 0] - ORIGIN[0] <= RW - S and 0 <= xy[n, 1] - ORIGIN[1] <= RH - S]
    assert len(inside) >= 4 and (want[6] == fill).all() and (want[7] == fill).all()         # the table has what its docstring says
    # an `out` buffer is written in place; N = 0 is a no-op
    buf = torch.full((37, 3, S, S), 7, dtype=torch.uint8, device=DEV)
    assert I.gather_tiles(dev, torch.from_numpy(xy.astype(np.int32)).to(DEV), S, origin=ORIGIN, fill=fill, out=buf) is buf
    assert np.array_equal(buf.cpu().numpy(), want)
    assert I.gather_tiles(dev, torch.empty((0, 2), dtype=torch.int32, device=DEV), S).shape == (0, 3, S, S)


def test_wsi_gather_source_offsets_beyond_32_bits():
    """a region of 4.32e9 bytes: rows from 39769 on start past byte 2^32"""
    from ssl_cr_histo_amd import inference as I
    H, W, S = 40000, 36000, 64
    big = torch.empty((H, W, 3), dtype=torch.uint8, device=DEV)
    gen = torch.Generator(device=DEV).manual_seed(5)
    for r0 in range(0, H, 4000):                                                   # filled in slabs: every call stays below 2^31 elements
        big[r0:r0 + 4000].copy_(torch.randint(0, 256, (4000, W, 3), dtype=torch.uint8, device=DEV, generator=gen))
    xy = np.array([(0, 39800), (1, 39801), (35936, 39930), (17002, 39899), (12345, 39936), (35999 - 70, 39850), (7, 39777), (35940, 39970)])
    assert ((xy[:, 1].astype(np.int64) * W + xy[:, 0]) * 3 > 1 << 32).all()
    got = I.gather_tiles(big, torch.from_numpy(xy.astype(np.int32)).to(DEV), S).cpu()
    for n, (x, y) in enumerate(xy):
        want = torch.zeros((3, S, S), dtype=torch.uint8)
        sl = big[y:y + S, x:x + S].permute(2, 0, 1).cpu()                          # the last tile crosses the bottom edge
        want[:, :sl.shape[1], :sl.shape[2]] = sl
        assert torch.equal(got[n], want), n
    assert got.float().std() > 50                                                  # the slices were not all fill
    del big


# ---------------------------------------------------------------------------------------------------------------- kernels: predict
def _predict_case(n, Cn, seed, nan_row, bad_targets):
    rs = np.random.RandomState(seed)
    l = rs.uniform(-30.0, 30.0, size=(n, Cn)).astype(np.float32)
    for r in range(0, n, 7):                                   # constructed ties: the row maximum twice (three times where C allows)
        cols = rs.permutation(Cn)[:min(Cn, 3)]
        l[r, cols] = l[r].max() + 1.0
    if nan_row is not None:
        l[nan_row, rs.permutation(Cn)[:max(1, Cn // 2)]] = np.nan
    y = rs.randint(0, Cn, n).astype(np.int64)
    if bad_targets:
        y[::5] = -100
        y[2::11] = Cn
    return torch.from_numpy(l), torch.from_numpy(y)


def _check_predict(l, y, nan_row):
    from sklearn.metrics import confusion_matrix
    from ssl_cr_histo_amd import kernels as K
    n, Cn = l.shape
    ld, yd = l.to(DEV), y.to(DEV)
    cm = torch.zeros((Cn, Cn), dtype=torch.int64, device=DEV)
    out = K.predict(ld, yd, scores=True, pred=True, confusion=cm)
    want_pred = torch.argmax(l, dim=1)
    pred = out["pred"].cpu()
    assert pred.dtype == torch.int64 and torch.equal(pred, want_pred)
    kept = ((y >= 0) & (y < Cn)).numpy()
    want_cm = confusion_matrix(y.numpy()[kept], want_pred.numpy()[kept], labels=list(range(Cn))) if kept.any() else np.zeros((Cn, Cn), np.int64)
    assert np.array_equal(cm.cpu().numpy(), want_cm)
    K.predict(ld, yd, pred=False, confusion=cm)                                    # accumulates across calls
    assert np.array_equal(cm.cpu().numpy(), 2 * want_cm)
    # scores: per-element float64 bounds (tests/_f64.py's softmax bound, every column); a row with a NaN is all NaN, as torch's
    rows = np.ones(n, bool)
    sc = out["scores"].cpu()
    if nan_row is not None:
        rows[nan_row] = False
        assert torch.isnan(sc[nan_row]).all() and torch.isnan(torch.softmax(l[nan_row], 0)).all()
    if rows.any():
        p64, bnd = softmax_rows_ref(l[rows])
        ratio = ((sc[rows].double() - p64).abs() / bnd).max()
        print(f"predict scores n={n} C={Cn}: worst |err| / bound = {float(ratio):.3f}")
        assert ratio <= 1.0, float(ratio)
    # map: the bits of softmax_col, scattered; untouched cells stay exactly 0
    perm = torch.from_numpy(np.random.RandomState(n + Cn).permutation(n + 13)[:n].astype(np.int64))
    for col in (-1, 0):
        m = torch.zeros(n + 13, dtype=torch.float32, device=DEV)
        assert K.predict(ld, pred=False, col=col, map=m, map_index=perm.to(DEV)) == {}
        want = torch.zeros(n + 13, dtype=torch.float32)
        want[perm] = K.softmax_col(ld, col).cpu()
        assert torch.equal(m.cpu().view(torch.int32), want.view(torch.int32)), col
        untouched = torch.ones(n + 13, dtype=torch.bool)
        untouched[perm] = False
        assert (m.cpu()[untouched].view(torch.int32) == 0).all()


@pytest.mark.parametrize("n", [1, 1000, 4097])
@pytest.mark.parametrize("Cn", [2, 6, 9])
def test_predict_against_torch_and_sklearn(n, Cn):
    if n == 1:                                                 # the one row is, in turn: the tie row, the NaN row, a skipped target
        for nan_row, bad in ((None, False), (0, False), (None, True)):
            _check_predict(*_predict_case(n, Cn, 40 + Cn, nan_row, bad), nan_row)
    else:
        nan_row = 3
        _check_predict(*_predict_case(n, Cn, 40 + n + Cn, nan_row, True), nan_row)


def test_argmax_tie_and_nan_rule_is_torch_s():
    from ssl_cr_histo_amd import kernels as K
    l = torch.tensor([[1, 3, 3, 2], [float("nan"), 5, float("nan"), 1], [2, float("nan"), 9, 9]], dtype=torch.float32)
    assert torch.argmax(l, 1).tolist() == [1, 0, 1]
    assert K.predict(l.to(DEV))["pred"].cpu().tolist() == [1, 0, 1]


# ---------------------------------------------------------------------------------------------------------------- engine: WSI loader
def _slide_and_mask():
    rs = np.random.RandomState(31)
    slide = rs.randint(0, 256, size=(1024, 1280, 3), dtype=np.uint8)              # [RH, RW, 3]: X_slide = 1280, Y_slide = 1024
    mask = rs.rand(20, 16) < 0.45                                                  # indexed [x, y]; resolution 64
    mask[0, 0] = mask[19, 15] = True                                               # tiles that cross the edges
    return slide, mask


class _SyncCounter:
    """counts the calls that wait for the device or copy from it while a block runs"""

    def __init__(self, monkeypatch):
        self.calls = []
        for owner, name in ((torch.Tensor, "cpu"), (torch.Tensor, "item"), (torch.Tensor, "tolist"), (torch.Tensor, "numpy"),
                            (torch.cuda, "synchronize"), (torch.cuda.Stream, "synchronize"), (torch.cuda.Event, "synchronize")):
            orig = getattr(owner, name)

            def wrapped(*a, _orig=orig, _name=name, **k):
                if not (a and torch.is_tensor(a[0]) and not a[0].is_cuda):     # host tensors do not touch the device
                    self.calls.append(_name)
                return _orig(*a, **k)
            monkeypatch.setattr(owner, name, wrapped)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_device_wsi_loader_gives_the_host_loaders_map_bit_for_bit(dtype, monkeypatch):
    from ssl_cr_histo_amd import steps
    from ssl_cr_histo_amd.inference import WsiDeviceLoader, tile_origins
    _engine(dtype)
    slide, mask = _slide_and_mask()
    S, B = 256, 24
    model, cls = build(2, head_scale=0.05)
    # path A: the same tiles cut on the host (numpy, zero padding), fed as uint8 NCHW batches through the unchanged branch
    x_idcs, y_idcs, xy = tile_origins(mask, 64, S)
    n = len(x_idcs)
    assert n % B != 0 and n > 3 * B
    tiles = cut_tiles(slide, xy, S)
    batches = [(torch.from_numpy(tiles[i:i + B]), torch.from_numpy(x_idcs[i:i + B].copy()), torch.from_numpy(y_idcs[i:i + B].copy()))
               for i in range(0, n, B)]
    map_a = steps.camelyon16_test(ns(), model, cls, C.WsiLoader(mask, batches))
    # path B: the slide in HBM
    loader = WsiDeviceLoader(slide, mask, S, B)
    assert loader.dataset.resolution == 64 and len(loader) == len(batches) and loader.dataset.mask is not None
    torch.cuda.synchronize()
    counter = _SyncCounter(monkeypatch)
    map_b = steps.camelyon16_test(ns(), model, cls, loader)
    monkeypatch.undo()
    assert counter.calls == ["cpu"], counter.calls                                 # the one copy of the finished map, after the loop
    assert map_b.dtype == np.float64 and map_b.shape == mask.shape == map_a.shape
    assert np.array_equal(map_b == 0, ~mask)
    assert np.array_equal(map_a, map_b)
    assert map_b[mask].std() > 1e-4                                                # a map that says something
    # iterating the loader yields the host loader's batches
    t0, xm, ym = next(iter(loader))
    assert np.array_equal(t0.cpu().numpy(), tiles[:B]) and torch.equal(xm, batches[0][1]) and torch.equal(ym, batches[0][2])


# ---------------------------------------------------------------------------------------------------------------- engine: test() drop-ins
def _manual(net, batches, want_scores):
    from ssl_cr_histo_amd import kernels as K
    feats, logits = [], []
    for b in batches:
        f, l = net.forward((b[0].to(DEV),), train=False)
        feats.append(f.clone())
        logits.append(l.clone())
    out = dict(feats=torch.cat(feats).cpu(), logits=torch.cat(logits).cpu())
    if want_scores:
        p = [K.predict(l, scores=True) for l in logits]
        out["scores"] = torch.cat([q["scores"] for q in p]).cpu()
        out["pred"] = torch.cat([q["pred"] for q in p]).cpu()
    return out


def _bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("which", ["kather_cr", "kather_sup"])
def test_kather_test_dropins_are_the_engine_forward_and_predict(which, dtype):
    from sklearn.metrics import confusion_matrix
    from ssl_cr_histo_amd import steps
    from ssl_cr_histo_amd.scripts import eval_Kather_SSL, eval_Kather_SSL_CR
    eng = _engine(dtype)
    c = TEST_CASES["kather"]
    model, cls = build(c["classes"], c["head_scale"])
    batches = kather_test_batches()
    if which == "kather_cr":
        pred, target, score = eval_Kather_SSL_CR.test(ns(), model, cls, batches)
    else:
        pred, target = eval_Kather_SSL.test(ns(), model, cls, batches, torch.nn.CrossEntropyLoss())
    cm = steps.last_test_confusion()
    m = _manual(eng.bind(model, cls), batches, True)
    assert pred.dtype == torch.int64 and target.dtype == torch.int64 and not pred.is_cuda and not target.is_cuda
    assert torch.equal(target, torch.cat([b[1] for b in batches]))
    assert torch.equal(pred, m["pred"]) and torch.equal(pred, torch.argmax(m["logits"], 1))
    if which == "kather_cr":
        assert not score.is_cuda and _bits(score, m["scores"])
        assert torch.equal(pred, torch.argmax(score, 1))
    assert cm.dtype == torch.int64 and not cm.is_cuda
    assert np.array_equal(cm.numpy(), confusion_matrix(target.numpy(), pred.numpy(), labels=list(range(c["classes"]))))
    with pytest.raises(NotImplementedError):
        eval_Kather_SSL.test(ns(), model, cls, batches, torch.nn.CrossEntropyLoss(label_smoothing=0.1))


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("which", ["bpq_cr", "bpq_sup"])
def test_bpq_test_dropins_are_the_engine_forward(which, dtype):
    from ssl_cr_histo_amd import steps
    from ssl_cr_histo_amd.scripts import eval_BreastPathQ_SSL, eval_BreastPathQ_SSL_CR
    eng = _engine(dtype)
    model, cls = build(1)
    batches = bpq_test_batches()
    if which == "bpq_cr":
        out, feats, ta, tb = eval_BreastPathQ_SSL_CR.test(ns(), model, cls, batches)
    else:
        out, feats, ta, tb = eval_BreastPathQ_SSL.test(ns(), model, cls, torch.nn.MSELoss(), batches)
    m = _manual(eng.bind(model, cls), batches, False)
    assert not any(t.is_cuda for t in (out, feats, ta, tb))
    assert out.shape == (11,) and feats.shape == (11, 768)
    assert _bits(out, m["logits"].reshape(-1)) and _bits(feats, m["feats"])
    assert torch.equal(ta, torch.cat([b[1] for b in batches])) and torch.equal(tb, torch.cat([b[2] for b in batches])) and ta.dtype == torch.float32
    assert steps.last_test_confusion() is None
    with pytest.raises(NotImplementedError):
        eval_BreastPathQ_SSL.test(ns(), model, cls, torch.nn.L1Loss(), batches)


def test_kather_test_against_the_reference():
    """fp32 mode against eval_Kather_SSL_CR.test / eval_Kather_SSL.test themselves: scores to 1e-3 absolute (the tolerance of the fp32
    validate and WSI tests); predictions equal on every row whose reference top-2 margin exceeds 2e-3, at least half of the rows."""
    from ssl_cr_histo_amd.scripts import eval_Kather_SSL, eval_Kather_SSL_CR
    _engine("fp32")
    c = TEST_CASES["kather"]
    g = load_golden("kather_test")
    model, cls = build(c["classes"], c["head_scale"])
    pred, target, score = eval_Kather_SSL_CR.test(ns(), model, cls, kather_test_batches())
    want = g["kather_test/score"]
    err = float(np.abs(score.numpy().astype(np.float64) - want).max())
    print(f"kather test(): max abs score error {err:.2e} (scores {want.min():.3f}..{want.max():.3f})")
    assert score.shape == want.shape and err <= 1e-3, err
    assert np.array_equal(target.numpy(), g["kather_test/target"])
    top2 = np.sort(want.astype(np.float64), 1)[:, -2:]
    sure = (top2[:, 1] - top2[:, 0]) > MARGIN
    assert sure.mean() >= MARGIN_SHARE and np.array_equal(sure, g["kather_test/margin"] > MARGIN)
    assert np.array_equal(pred.numpy()[sure], g["kather_test/pred"][sure])
    pred2, target2 = eval_Kather_SSL.test(ns(), model, cls, kather_test_batches(), torch.nn.CrossEntropyLoss())
    assert np.array_equal(pred2.numpy()[sure], g["kather_test/sup_pred"][sure]) and np.array_equal(target2.numpy(), g["kather_test/sup_target"])


def test_bpq_test_against_the_reference():
    """fp32 mode against eval_BreastPathQ_SSL_CR.test / eval_BreastPathQ_SSL.test themselves: outputs and features to 1e-3 relative"""
    from ssl_cr_histo_amd.scripts import eval_BreastPathQ_SSL, eval_BreastPathQ_SSL_CR
    _engine("fp32")
    g = load_golden("bpq_test")
    model, cls = build(1)
    for tag, ret in (("", eval_BreastPathQ_SSL_CR.test(ns(), model, cls, bpq_test_batches())),
                     ("sup_", eval_BreastPathQ_SSL.test(ns(), model, cls, torch.nn.MSELoss(), bpq_test_batches()))):
        out, feats, ta, tb = ret
        for got, want in ((out, g[f"bpq_test/{tag}outputs"]), (feats, g[f"bpq_test/{tag}feats"])):
            err = float(np.abs(got.numpy().astype(np.float64) - want).max() / np.abs(want).max())
            print(f"bpq {tag}test(): max error {err:.2e} of the largest value, shape {tuple(got.shape)}")
            assert got.shape == want.shape and err <= 1e-3, err
        assert np.array_equal(ta.numpy(), g["bpq_test/targetsA"]) and np.array_equal(tb.numpy(), g["bpq_test/targetsB"])
