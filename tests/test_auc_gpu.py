"""The ranking metrics on the MI355X.  Every device result is held by EQUALITY: ``sort_pairs`` against NumPy's stable argsort,
``auc_counts`` against the integer restatement of tests/_auc_ref.py, ``roc_auc`` / ``map_auc`` / ``AucMeter`` against the restatement's
float64 (and within n 2^-53 of sklearn, whose trapezoid is a float64 sum of at most n terms with a total of at most 1)."""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _auc_ref as R  # noqa: E402
from _inference_util import TEST_CASES, bpq_test_batches, kather_test_batches, scale_head  # noqa: E402

from ssl_cr_histo_amd.kernels import RANK_SCAN_TRIP as TRIP, SORT_TILE as T  # noqa: E402  (SSLCR_RANK_SCAN_TRIP, SSLCR_SORT_TILE)

DEV = "cuda:0"
# below a wave, a wave, above it; around one tile; three tiles; and the smallest row whose partial scans (the sort's tiles of one digit,
# the AUC's blocks of one column: TRIP of them a trip) take a second trip
LENGTHS = [1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1, TRIP * T + 1]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def test_exported_geometry():
    """the lengths above are derived from the exported constants; the header's values are what the kernels were compiled with"""
    from ssl_cr_histo_amd import _lib as L
    assert (T, TRIP) == (L.SORT_TILE, L.RANK_SCAN_TRIP) == (4096, 64)
    assert (LENGTHS[-1] + T - 1) // T == TRIP + 1                   # a second trip, by one tile
    assert L.lib().sslcr_sort_workspace_bytes(1, LENGTHS[-1]) == 256 * (TRIP + 1 + 1) * 4


# ---------------------------------------------------------------------------------------------------------------- sort_pairs
def key_sets(B, n, seed):
    rs = np.random.RandomState(seed)
    u32 = lambda a: np.asarray(a).astype(np.uint32)                 # noqa: E731
    extremes = u32(rs.randint(0, 1 << 32, (B, n), dtype=np.int64))
    extremes[:, ::7] = 0
    extremes[:, 3::11] = 0xFFFFFFFF
    distinct = np.stack([u32((rs.permutation(n).astype(np.uint64) * 2654435761 + 12345) & 0xFFFFFFFF) for _ in range(B)])   # odd multiplier: a bijection
    return {"equal": np.full((B, n), 0xDEADBEEF, dtype=np.uint32), "distinct": distinct,
            "top byte": u32(rs.randint(0, 256, (B, n)).astype(np.int64) << 24 | 0x00ABCDEF),
            "low byte": u32(rs.randint(0, 256, (B, n)) | 0x12345600), "extremes": extremes,
            "sixteen": u32(rs.randint(0, 1 << 32, 16, dtype=np.int64))[rs.randint(0, 16, (B, n))]}


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n", LENGTHS)
def test_sort_pairs_equals_numpys_stable_argsort(n, B):
    from ssl_cr_histo_amd import kernels as K
    for name, keys in key_sets(B, n, 1000 * B + n % 997).items():
        order = np.argsort(keys, axis=1, kind="stable")
        d = _dev(keys)
        k, v = K.sort_pairs(d)
        assert k.dtype == torch.uint32 and v.dtype == torch.uint32 and k.shape == (B, n) and v.shape == (B, n)
        assert np.array_equal(k.cpu().numpy(), np.take_along_axis(keys, order, 1)), name
        assert np.array_equal(v.cpu().numpy(), order.astype(np.uint32)), name
        assert np.array_equal(d.cpu().numpy(), keys), name         # the input is left alone
        k2, v2 = K.sort_pairs(d)
        assert torch.equal(k.view(torch.int32), k2.view(torch.int32)) and torch.equal(v.view(torch.int32), v2.view(torch.int32)), name
    if B == 1:                                                      # a 1-D row in, 1-D rows out
        k, v = K.sort_pairs(d[0])
        assert k.shape == (n,) and np.array_equal(v.cpu().numpy(), order[0].astype(np.uint32))


@pytest.mark.parametrize("bits", [(8, 24), (0, 0), (5, 8), (4, 17), (31, 32)])
@pytest.mark.parametrize("n", [65, T + 1, 2 * T + 1])
def test_sort_pairs_over_a_bit_range_is_the_sort_of_the_masked_keys(n, bits):
    """keys equal inside [lo, hi) keep their input order whatever their other bits; (5, 8) and (4, 17) end on a digit narrower than 8
    bits, (0, 0) is no pass at all; explicit values travel with their keys"""
    from ssl_cr_histo_amd import kernels as K
    lo, hi = bits
    rs = np.random.RandomState(n + 100 * lo + hi)
    keys = rs.randint(0, 1 << 32, (3, n), dtype=np.int64).astype(np.uint32)
    values = rs.randint(0, 1 << 32, (3, n), dtype=np.int64).astype(np.uint32)
    masked = (keys.astype(np.uint64) >> lo) & ((1 << (hi - lo)) - 1)
    order = np.argsort(masked, axis=1, kind="stable")
    k, v = K.sort_pairs(_dev(keys), _dev(values), bits=bits, workspace=K.sort_workspace(3, n, DEV))
    assert np.array_equal(k.cpu().numpy(), np.take_along_axis(keys, order, 1))
    assert np.array_equal(v.cpu().numpy(), np.take_along_axis(values, order, 1))


def test_sort_pairs_refuses_what_it_cannot_sort():
    from ssl_cr_histo_amd import _lib as L
    from ssl_cr_histo_amd import kernels as K
    keys = torch.zeros(8, dtype=torch.int32, device=DEV)
    with pytest.raises(L.SslcrError):
        K.sort_pairs(keys.cpu())
    with pytest.raises(L.SslcrError):
        K.sort_pairs(keys, bits=(8, 40))
    with pytest.raises(L.SslcrError):
        K.sort_pairs(keys, torch.zeros(9, dtype=torch.int32, device=DEV))
    with pytest.raises(L.SslcrError):
        K.sort_pairs(keys, workspace=torch.zeros(4, dtype=torch.int32, device=DEV))


# ---------------------------------------------------------------------------------------------------------------- auc_counts
def _cases(n, Cn, seed):
    """name -> (scores float32 [n, Cn], target int64 [n], valid bool [n] or None)"""
    rs = np.random.RandomState(seed)
    classes = max(Cn, 2)
    cyc = np.arange(n) % classes                                    # every class next to every other one, on both sides of any border
    rnd = rs.randint(0, classes, n)
    out = {"random": (rs.rand(n, Cn).astype(np.float32), rnd, None),
           "two values": (rs.choice(np.array([0.25, 0.75], dtype=np.float32), (n, Cn)), rnd, None),
           "zeros": (rs.choice(np.array([0.0, -0.0, 0.5, -0.5], dtype=np.float32), (n, Cn)), rnd, None)}
    # one run of ties: everything 0.5 but an eighth below and a few above -- at n > 2 T + n / 8 the run outgrows two tiles, and
    # the stable sort keeps the cycling classes in order inside it
    tie = np.full((n, Cn), 0.5, dtype=np.float32)
    tie[:n // 8] = 0.25
    tie[rs.rand(n) < 0.01] = 0.75
    out["one long run"] = (tie, cyc, None)
    valid = np.ones(n, dtype=bool)
    valid[T:2 * T] = False                                          # a whole tile of the input
    valid[rs.rand(n) < 0.05] = False                                # single cells
    if n > 1:
        valid[n - 1] = True
    out["masked"] = (rs.choice(np.linspace(0, 1, 33).astype(np.float32), (n, Cn)), rnd, valid)
    return out


@pytest.mark.parametrize("Cn", [1, 9])
@pytest.mark.parametrize("n", LENGTHS)
def test_auc_counts_equal_the_restatement(n, Cn):
    from ssl_cr_histo_amd import kernels as K
    positive = [1] if Cn == 1 else None
    for name, (scores, target, valid) in _cases(n, Cn, 31 * n + Cn).items():
        want = R.counts(scores, target, positive, valid)
        args = (_dev(scores), _dev(target.astype(np.int64)))
        kw = dict(positive=positive, valid=None if valid is None else _dev(valid))
        got = K.auc_counts(*args, **kw)
        assert got.dtype == torch.int64 and got.shape == (Cn, 4) and got.is_cuda
        assert np.array_equal(got.cpu().numpy(), want), name
        assert torch.equal(got, K.auc_counts(*args, **kw)), name     # two calls, equal bits
    if Cn == 1:                                                     # a vector is one column
        assert np.array_equal(K.auc_counts(args[0].reshape(-1), args[1], **kw).cpu().numpy(), want)


@pytest.mark.parametrize("n", [65, 2 * T + 1])
def test_a_nan_is_counted_in_its_column_and_nowhere_else(n):
    from ssl_cr_histo_amd import kernels as K
    rs = np.random.RandomState(n)
    scores = rs.rand(n, 9).astype(np.float32)
    target = rs.randint(0, 9, n)
    valid = rs.rand(n) < 0.9
    valid[7] = False
    clean = R.counts(scores, target, None, valid)
    where = np.flatnonzero(valid)[[0, len(np.flatnonzero(valid)) // 2, -1]]
    scores[where, 4] = np.array([np.nan, -np.nan, np.float32(np.nan)], dtype=np.float32)
    scores[np.flatnonzero(~valid)[0], 6] = np.nan                   # on an element left out: not counted
    got = K.auc_counts(_dev(scores), _dev(target), valid=_dev(valid)).cpu().numpy()
    want = R.counts(scores, target, None, valid)
    assert np.array_equal(got, want)
    assert got[4, 3] == 3 and got[:, 3].sum() == 3
    others = [c for c in range(9) if c != 4]
    assert np.array_equal(got[others], clean[others])               # every other column is what it was
    assert got[4, 1] + got[4, 2] == clean[4, 1] + clean[4, 2] - 3   # column 4 counts the other elements only


@pytest.mark.parametrize("n", [64, T + 1])
def test_a_column_without_positives_or_without_negatives(n):
    from ssl_cr_histo_amd import kernels as K
    rs = np.random.RandomState(n)
    scores = rs.rand(n, 9).astype(np.float32)
    target = rs.randint(0, 8, n)
    target[target == 4] = 8                                         # class 4 never occurs: column 4 has P = 0, the others have both
    got = K.auc_counts(_dev(scores), _dev(target)).cpu().numpy()
    assert np.array_equal(got, R.counts(scores, target))
    assert got[4].tolist() == [0, 0, n, 0] and np.all(got[[0, 1, 2, 3, 5, 6, 7, 8], 1] > 0) and np.all(got[:, 2] > 0)
    ones = np.ones(n, dtype=np.int64)                               # a vector whose every element is positive: N = 0
    got = K.auc_counts(_dev(scores[:, 0].copy()), _dev(ones), positive=[1]).cpu().numpy()
    assert got.tolist() == [[0, n, 0, 0]]


# ---------------------------------------------------------------------------------------------------------------- roc_auc, map_auc, AucMeter
def _softmax32(rs, n, Cn):
    l = rs.randn(n, Cn) * 2
    e = np.exp(l - l.max(1, keepdims=True))
    return (e / e.sum(1, keepdims=True)).astype(np.float32)


def test_roc_auc_equals_the_restatement_and_sklearn_within_its_rounding():
    from sklearn.metrics import roc_auc_score
    from ssl_cr_histo_amd import inference as I
    rs = np.random.RandomState(77)
    n = 2 * T + 77
    bound = n * 2.0 ** -53
    for name, s in R.score_sets(n, 5).items():                      # binary: a vector scores class 1
        t = rs.randint(0, 2, n)
        got = I.roc_auc(_dev(s), _dev(t))
        assert isinstance(got, float) and got == R.auc_from_counts(R.counts(s, t, [1])), name
        assert abs(got - roc_auc_score(t, s)) <= bound, name
        assert I.roc_auc(s, t) == got and I.roc_auc(s.reshape(-1, 1), torch.from_numpy(t)) == got      # host inputs are uploaded
    p, t = _softmax32(rs, n, 9), rs.randint(0, 9, n)
    c = R.counts(p, t)
    for average in ("macro", "weighted"):
        got = I.roc_auc(_dev(p), _dev(t), multi_class="ovr", average=average)
        assert got == R.auc_from_counts(c, average)
        assert abs(got - roc_auc_score(t, p.astype(np.float64), multi_class="ovr", average=average)) <= bound
    per_class = I.roc_auc(_dev(p), _dev(t), multi_class="ovr", average=None)
    assert per_class.dtype == np.float64 and np.array_equal(per_class, R.auc_from_counts(c, None))
    valid = rs.rand(n) < 0.5
    assert I.roc_auc(_dev(p), _dev(t), multi_class="ovr", valid=_dev(valid)) == R.auc_from_counts(R.counts(p, t, None, valid))
    # sklearn's errors, from device counts
    with pytest.raises(ValueError, match="multi_class must be in"):
        I.roc_auc(_dev(p), _dev(t))
    bad = p.copy()
    bad[5, 2] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        I.roc_auc(_dev(bad), _dev(t), multi_class="ovr")
    with pytest.raises(ValueError, match="Only one class present"):
        I.roc_auc(_dev(p[:, 0].copy()), _dev(np.zeros(n, dtype=np.int64)))
    with pytest.raises(ValueError, match="Number of classes in y_true not equal"):
        I.roc_auc(_dev(p), _dev(np.where(t == 3, 0, t)), multi_class="ovr")


def test_map_auc_is_the_area_over_the_tissue_cells():
    from sklearn.metrics import roc_auc_score
    from ssl_cr_histo_amd import inference as I
    rs = np.random.RandomState(8)
    X, Y = 130, 67
    pm = rs.rand(X, Y).astype(np.float32)
    pm[rs.rand(X, Y) < 0.6] = np.float32(1.0)                        # a plateau: one run of ties over several blocks
    truth = rs.rand(X, Y) < np.where(pm > 0.8, 0.7, 0.2)
    tissue = rs.rand(X, Y) < 0.8
    want = R.auc_from_counts(R.counts(pm.reshape(-1), truth.reshape(-1).astype(np.int64), [1], tissue.reshape(-1)))
    got = I.map_auc(_dev(pm), _dev(truth), _dev(tissue))
    assert got == want
    assert I.map_auc(pm.astype(np.float64), truth.astype(np.uint8) * 255, tissue) == want             # host inputs, as map_scores takes
    assert abs(got - roc_auc_score(truth[tissue], pm[tissue])) <= tissue.sum() * 2.0 ** -53
    with pytest.raises(ValueError, match="Only one class present"):
        I.map_auc(_dev(pm), _dev(np.zeros((X, Y), dtype=bool)), _dev(tissue))


def test_auc_meter_in_three_uneven_batches_equals_one_call():
    from ssl_cr_histo_amd import inference as I
    rs = np.random.RandomState(4)
    n = T + 300
    p, t = _softmax32(rs, n, 9), rs.randint(0, 9, n)
    dp, dt = _dev(p), _dev(t)
    meter = I.AucMeter(9, DEV)
    for lo, hi in ((0, 5), (5, T + 1), (T + 1, n)):
        meter.update(dp[lo:hi], dt[lo:hi])
    for kw in (dict(multi_class="ovr"), dict(multi_class="ovr", average="weighted")):
        assert meter.compute(**kw) == I.roc_auc(dp, dt, **kw) == R.auc_from_counts(R.counts(p, t), kw.get("average", "macro"))
    binary = I.AucMeter(1, DEV).update(dp[:100, 0], dt[:100] == 1).update(dp[100:, 0], dt[100:] == 1)
    assert binary.compute() == I.roc_auc(dp[:, 0], (dt == 1))


# ---------------------------------------------------------------------------------------------------------------- last_test_auc
def _engine(dtype):
    from ssl_cr_histo_amd import engine as E
    idx = torch.device(DEV).index
    cur = E._engines.get(idx)
    if cur is None or cur.dtype != E._DTYPES[dtype]:
        E._engines.pop(idx, None)
        E.set_engine(E.Engine(DEV, dtype))
    return E.get_engine(DEV)


def _build(classes, head_scale=1.0):
    from oracle import cases as C
    from oracle import model as OM
    from ssl_cr_histo_amd import net
    model, cls = net.TripletNet_Finetune("resnet18"), net.FinetuneResNet(classes)
    model.load_state_dict(OM.init_state(C.PARAM_SEED, OM.net_param_specs(), random_running_stats=True))
    cls.load_state_dict(OM.init_state(C.PARAM_SEED + 1, OM.classifier_param_specs("finetune", classes)))
    scale_head(cls, head_scale)
    return model.to(DEV), cls.to(DEV)


def test_last_test_auc_after_the_kather_test():
    """the fixture loader of tests/test_inference_gpu.py at three seeds (33 images: every one of the nine classes occurs); the returned
    tuple and the confusion matrix are what the engine forward and sslcr_predict give on their own, as before"""
    from sklearn.metrics import confusion_matrix
    from ssl_cr_histo_amd import inference as I
    from ssl_cr_histo_amd import kernels as K
    from ssl_cr_histo_amd import steps
    eng = _engine("fp32")
    c = TEST_CASES["kather"]
    model, cls = _build(c["classes"], c["head_scale"])
    batches = [b for seed in (7100, 7300, 7500) for b in kather_test_batches(seed)]
    args = types.SimpleNamespace(print_freq=0)
    pred, target, score = steps.kather_cr_test(args, model, cls, batches)
    cm = steps.last_test_confusion()
    # what the parent returns: the eval forward and sslcr_predict per batch, concatenated, on the CPU
    net = eng.bind(model, cls)
    manual = [K.predict(net.forward((b[0].to(DEV),), train=False)[1].clone(), scores=True) for b in batches]
    assert not score.is_cuda and score.dtype == torch.float32 and score.shape == (33, 9)
    assert torch.equal(score.view(torch.int32), torch.cat([m["scores"] for m in manual]).cpu().view(torch.int32))
    assert torch.equal(pred, torch.cat([m["pred"] for m in manual]).cpu()) and torch.equal(target, torch.cat([b[1] for b in batches]))
    assert np.array_equal(cm.numpy(), confusion_matrix(target.numpy(), pred.numpy(), labels=list(range(9))))
    for average in ("macro", "weighted", None):
        got = steps.last_test_auc(average)
        assert np.array_equal(got, I.roc_auc(score, target, multi_class="ovr", average=average))
        assert np.array_equal(got, R.auc_from_counts(R.counts(score.numpy(), target.numpy()), average))
        assert steps.last_test_auc(average) is got                  # cached
    assert steps.last_test_auc() == steps.last_test_auc("macro")
    # a test without class scores leaves nothing to rank
    steps.kather_sup_test(args, model, cls, batches[:1], torch.nn.CrossEntropyLoss())
    assert steps.last_test_auc() is None and steps.last_test_confusion() is not None
    steps.kather_cr_test(args, model, cls, batches[:3])
    assert len(set(torch.cat([b[1] for b in batches[:3]]).tolist())) < 9              # these 11 images miss a class
    with pytest.raises(ValueError, match="Number of classes in y_true not equal"):
        steps.last_test_auc()
    model1, cls1 = _build(1)
    steps.bpq_test(args, model1, cls1, bpq_test_batches())
    assert steps.last_test_auc() is None and steps.last_test_confusion() is None
