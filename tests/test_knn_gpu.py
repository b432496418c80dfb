"""The k-NN feature probe on the MI355X (csrc/knn.hip, include/sslcr.h) against tests/_knn_ref.py.

Integer-valued features (entries in {-3 .. 3}: |dot| <= 9 D < 2^24, so every fp32 chain is exact and ties are everywhere) must give
scores and indices EQUAL to the restatement; random floats must give equal bits under every plan, the bits of the fmaf chain in
rising d, and neighbours inside the float64 bounds derived below with nothing left out; normalisation is EQUAL to the restatement on
inputs asserted to stand clear of a float32 rounding boundary; the votes are equal (uniform) or within their derived bounds."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import _knn_ref as R  # noqa: E402

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATIOS = os.path.join(ROOT, "profiles", "knn_ratios.txt")


def dev(a):
    return torch.as_tensor(a).to(DEV)


def record(name, value):
    """profiles/knn_ratios.txt: one ``name value`` line per measured worst ratio (observed / bound), rewritten in name order"""
    lines = {}
    if os.path.exists(RATIOS):
        with open(RATIOS) as f:
            lines = dict(ln.split(None, 1) for ln in f.read().splitlines() if ln.strip() and not ln.startswith("#"))
    lines[name] = f"{value:.4f}"
    with open(RATIOS, "w") as f:
        f.write("# worst observed / bound of the k-NN probe's float comparisons on the MI355X (tests/test_knn_gpu.py)\n")
        f.write("".join(f"{k} {v}\n" for k, v in sorted(lines.items())))


def ints(seed, *shape):
    return np.random.RandomState(seed).randint(-3, 4, shape).astype(np.float32)


def topk(q, b, k, **kw):
    from ssl_cr_histo_amd import kernels as K
    s, i = K.knn_topk(dev(q), dev(b), k, **kw)
    assert s.dtype == torch.float32 and i.dtype == torch.int32 and s.shape == i.shape == (len(q), k)
    return s.cpu().numpy(), i.cpu().numpy()


def same(got, want):
    (gs, gi), (ws, wi) = got, want
    assert np.array_equal(gi, wi), np.argwhere(gi != wi)[:5]
    assert np.array_equal(gs, ws, equal_nan=True), np.argwhere(gs != ws)[:5]
    assert not np.signbit(gs[gs == 0]).any()


# ------------------------------------------------------------------------------------------------ 1. equality on integer features
@pytest.mark.parametrize("nq,nb,D,k", [(1, 1, 4, 1), (65, 129, 68, 20), (64, 4097, 768, 64), (3, 10, 4, 64)])
def test_integer_features_equal_the_restatement(nq, nb, D, k):
    q, b = ints(nq + 1, nq, D), ints(nb + 2, nb, D)
    want = R.topk(R.similarity(q, b), k)
    same(topk(q, b, k), want)
    if nb < k:
        assert (want[1][:, nb:] == -1).all() and np.isneginf(want[0][:, nb:]).all()


def test_a_bank_of_one_repeated_row_returns_the_lowest_indices():
    q = ints(1, 5, 8)
    b = np.repeat(ints(2, 1, 8), 200, 0)
    s, i = topk(q, b, 20)
    assert (i == np.arange(20)[None, :]).all()
    assert np.array_equal(s, np.repeat(R.similarity(q, b[:1]).astype(np.float32), 20, 1))


@pytest.mark.parametrize("slices", [None, 1, 7])
def test_duplicates_on_both_sides_of_every_tile_and_slice_border(slices):
    """the best row of the bank sits at the last row of every bank tile and at the first of the next, so the equal scores meet across
    every tile border and every slice border the plan reports; the k lowest of those indices must come back"""
    from ssl_cr_histo_amd import kernels as K
    nq, nb, D, k = 3, 4097, 12, 64
    p = K.knn_plan(nq, nb, D, k, slices)
    if slices:
        assert p["slices"] == slices
    q = np.full((nq, D), 3, np.float32)
    b = ints(5, nb, D)
    b[(b == 3).all(1)] = 0                                          # no accidental copy of the best row
    borders = np.arange(p["tile_b"], nb, p["tile_b"])
    assert all(s * p["tiles_per_slice"] * p["tile_b"] in borders for s in range(1, p["slices"]) if s * p["tiles_per_slice"] * p["tile_b"] < nb)
    hot = np.sort(np.concatenate([borders - 1, borders]))
    b[hot] = 3
    want = R.topk(R.similarity(q, b), k)
    assert (want[1] == hot[:k][None, :]).all() and (want[0] == 9 * D).all()
    same(topk(q, b, k, slices=slices), want)


def test_exclude_self_with_the_queries_taken_from_the_bank():
    b = ints(7, 130, 12)
    b[64] = b[63]                                                   # a duplicate of a row: each is the other's best neighbour
    s = R.similarity(b, b)
    same(topk(b, b, 5, exclude_self=True), R.topk(s, 5, self_offset=0))
    got = topk(b, b, 5, exclude_self=True)[1]
    assert not (got == np.arange(130)[:, None]).any()
    same(topk(b[10:40], b, 5, exclude_self=10), R.topk(s[10:40], 5, self_offset=10))
    same(topk(b, b, 5), R.topk(s, 5))


@pytest.mark.parametrize("nb_valid", [0, 1, 63, 64, 100])
def test_nb_valid_restricts_the_search_to_a_prefix(nb_valid):
    q, b = ints(8, 9, 8), ints(9, 129, 8)
    got = topk(q, b, 20, nb_valid=nb_valid)
    same(got, R.topk(R.similarity(q, b), 20, nb_valid=nb_valid))
    assert (got[1] < nb_valid).all() and ((got[1] >= 0).sum(1) == min(20, nb_valid)).all()


def test_nan_inf_and_negative_zero():
    q, b = ints(10, 6, 8), ints(11, 60, 8)
    q[q == 0] = 1                                                   # no 0 * inf except where a row asks for it
    q[:, 0:3] = np.abs(q[:, 0:3])                                   # row 5 scores +inf, row 7 -inf and row 30 inf - inf for every query
    b[3, 0] = np.nan
    b[5, 1] = np.inf
    b[7, 2] = -np.inf
    b[30] = [np.inf, -np.inf, 0, 0, 0, 0, 0, 0]                     # inf - inf (or the reverse): NaN for every query
    b[9] = -0.0
    b[11] = 0.0
    b[50, 7] = np.nan
    q[4, 3] = 0.0
    b[20, 3] = np.inf                                               # 0 * inf for query 4 only
    q[5] = np.nan                                                   # every score of query 5 is a NaN: ordered by index
    s = R.similarity(q, b)
    k = 64                                                          # > nb: every row comes back, then four empty slots
    want = R.topk(s, k)
    # the NaNs rank below every number, among themselves by index; the empty slots follow
    assert (want[1][:4, 57:60] == [3, 30, 50]).all() and np.isnan(want[0][:4, 57:60]).all() and (want[1][:, 60:] == -1).all()
    assert (want[1][4, 56:60] == [3, 20, 30, 50]).all() and (want[1][5, :60] == np.arange(60)).all() and np.isnan(want[0][5, :60]).all()
    assert np.isposinf(want[0][:4, 0]).all() and np.isneginf(want[0][:4, 56]).all()
    assert (want[0][0][np.isin(want[1][0], [9, 11])] == 0).all() and list(want[1][0]).index(9) + 1 == list(want[1][0]).index(11)
    same(topk(q, b, k), want)
    same(topk(q, b, 7), R.topk(s, 7))


# ------------------------------------------------------------------------------------------------ 2. random floats
def floats(seed, *shape):
    return np.random.RandomState(seed).randn(*shape).astype(np.float32)


def test_route_independence_and_the_bits_of_the_chain():
    """slices forced to 1, 2 and 7, and the plan's own choice: equal bits; and the scores are the fmaf chain over rising d"""
    q, b = floats(20, 65, 132), floats(21, 4097, 132)
    runs = [topk(q, b, 20, slices=s) for s in (1, 2, 7, None)]
    for s, i in runs[1:]:
        assert np.array_equal(s.view(np.int32), runs[0][0].view(np.int32)) and np.array_equal(i, runs[0][1])
    chain = R.fma_chain(q, b[:300])                                 # a prefix of the bank is enough for the bits
    s, i = topk(q, b, 20, nb_valid=300)
    assert np.array_equal(s.view(np.int32), np.take_along_axis(chain, i.astype(np.int64), 1).view(np.int32))
    same((s, i), R.topk(chain, 20))


def test_random_floats_against_float64_with_nothing_left_out():
    """eps_ij = gamma_D sum_d |q_d b_d|, gamma_D = D 2^-24 / (1 - D 2^-24): the standard bound of a length-D chain.  Every returned score
    is within eps of float64; every returned neighbour's float64 score is at least the true k-th score minus 2 eps; every bank row whose
    float64 score exceeds the true k-th score plus 2 eps is returned (eps: the larger of the two rows involved)."""
    nq, nb, D, k = 65, 1500, 260, 20
    q, b = floats(30, nq, D), floats(31, nb, D)
    b[1000:1200] = b[:200] * np.float32(1 + 2.0 ** -20)             # near ties inside the bound, which it must survive
    s64 = R.similarity(q, b)
    gamma = D * 2.0 ** -24 / (1 - D * 2.0 ** -24)
    eps = gamma * (np.abs(q).astype(np.float64) @ np.abs(b).astype(np.float64).T)
    s, i = topk(q, b, k)
    i = i.astype(np.int64)
    assert (i >= 0).all() and all(len(set(r)) == k for r in i)
    err = np.abs(s.astype(np.float64) - np.take_along_axis(s64, i, 1))
    e_ret = np.take_along_axis(eps, i, 1)
    print("score error / eps", (err / e_ret).max())
    record("topk_score_error", (err / e_ret).max())
    assert (err <= e_ret).all()
    order = np.argsort(-s64, 1, kind="stable")
    jk = order[:, k - 1]
    kth, e_kth = s64[np.arange(nq), jk], eps[np.arange(nq), jk]
    slack = 2 * np.maximum(e_ret, e_kth[:, None])
    worst = ((kth[:, None] - np.take_along_axis(s64, i, 1)) / slack).max()
    print("k-th score deficit / 2 eps", worst)
    record("topk_kth_deficit", max(worst, 0.0))
    assert (np.take_along_axis(s64, i, 1) >= kth[:, None] - slack).all()
    must = s64 > kth[:, None] + 2 * np.maximum(eps, e_kth[:, None])
    returned = np.zeros_like(must)
    np.put_along_axis(returned, i, True, 1)
    assert (returned | ~must).all()
    assert must.sum() >= nq * (k - 3)                               # the test has teeth: nearly every true neighbour is that clear


# ------------------------------------------------------------------------------------------------ 3. normalisation
@pytest.mark.parametrize("n,D", [(37, 768), (5, 4), (3, 2048), (9, 65)])
def test_l2_normalize(n, D):
    from ssl_cr_histo_amd import kernels as K
    x = floats(40 + D, n, D) * np.float32(3.0)
    x[0] *= np.float32(1e-3)
    assert (R.norm_clearance(x) > 2.0 ** -40).all()                 # the band the inputs must leave empty
    xd = dev(x)
    y = K.l2_normalize(xd)
    assert np.array_equal(y.cpu().numpy().view(np.int32), R.l2_normalize(x).view(np.int32))
    ref = F.normalize(xd, dim=1)
    ulp = np.abs(y.cpu().numpy().view(np.int32).astype(np.int64) - ref.cpu().numpy().view(np.int32).astype(np.int64))
    assert ulp.max() <= 2
    z = np.zeros((2, 8), np.float32)
    assert np.array_equal(K.l2_normalize(dev(z)).cpu().numpy(), z)   # 0 / eps
    assert K.l2_normalize(xd, out=xd) is xd and np.array_equal(xd.cpu().numpy(), y.cpu().numpy())


# ------------------------------------------------------------------------------------------------ 4. votes
_VOTE = {}


def vote_case():
    """clustered features, their device neighbours (cosine), computed once and left unchanged"""
    if not _VOTE:
        from ssl_cr_histo_amd import kernels as K
        rs = np.random.RandomState(50)
        C, D, nb, nq, k = 9, 64, 1000, 300, 20
        centres = rs.randn(C, D)
        yb, yq = rs.randint(0, C, nb), rs.randint(0, C, nq)
        bank = (centres[yb] * 0.5 + rs.randn(nb, D)).astype(np.float32)
        qs = (centres[yq] * 0.5 + rs.randn(nq, D)).astype(np.float32)
        s, i = K.knn_topk(K.l2_normalize(dev(qs)), K.l2_normalize(dev(bank)), k)
        s2, i2 = K.knn_topk(K.l2_normalize(dev(qs)), K.l2_normalize(dev(bank)), k, nb_valid=7)     # rows with empty slots
        _VOTE.update(C=C, k=k, yb=yb, yq=yq, tb=rs.rand(nb).astype(np.float32) * 3 - 1,
                     s=torch.cat([s, s2]), i=torch.cat([i, i2]), yq2=np.concatenate([yq, yq]))
    return _VOTE


def test_uniform_votes_equal_the_restatement():
    from ssl_cr_histo_amd import kernels as K
    v = vote_case()
    r = K.knn_vote(v["i"], None, labels=dev(v["yb"]), n_classes=v["C"], query_labels=dev(v["yq2"]))
    pred, counts = R.vote_uniform(v["i"].cpu().numpy(), v["yb"], v["C"])
    assert r["pred"].dtype == torch.int64 and np.array_equal(r["pred"].cpu().numpy(), pred)
    assert np.array_equal(r["votes"].cpu().numpy(), counts.astype(np.float32))
    assert np.array_equal(r["confusion"].cpu().numpy(), R.confusion(v["yq2"], pred, v["C"]))
    srt = np.sort(counts, 1)
    assert (srt[:, -1] == srt[:, -2]).any()                         # ties occur: the lowest class took them
    again = K.knn_vote(v["i"], None, labels=dev(v["yb"]), n_classes=v["C"], query_labels=dev(v["yq2"]), confusion=r["confusion"])
    assert again["confusion"] is r["confusion"] and np.array_equal(r["confusion"].cpu().numpy(), 2 * R.confusion(v["yq2"], pred, v["C"]))


def test_softmax_votes_within_the_derived_bound():
    """1e-5 relative: a 1-2 ulp expf, an argument error of (|s| / T) 2^-23 <= 1.7e-6 at T = 0.07 and |s| <= 1, 64 additions at 2^-24"""
    from ssl_cr_histo_amd import kernels as K
    v = vote_case()
    T = 0.07
    r = K.knn_vote(v["i"], v["s"], labels=dev(v["yb"]), n_classes=v["C"], weights="softmax", temperature=T)
    pred, votes = R.vote_softmax(v["i"].cpu().numpy(), v["s"].cpu().numpy(), v["yb"], v["C"], float(np.float32(T)))
    got = r["votes"].cpu().numpy().astype(np.float64)
    assert ((votes == 0) == (got == 0)).all()
    rel = np.abs(got - votes)[votes > 0] / votes[votes > 0]
    print("softmax vote error / 1e-5", rel.max() / 1e-5)
    record("softmax_vote_error", rel.max() / 1e-5)
    assert rel.max() <= 1e-5
    srt = np.sort(votes, 1)
    clear = (srt[:, -1] - srt[:, -2]) > 2e-5 * srt[:, -1]
    assert clear.mean() > 0.9
    assert np.array_equal(r["pred"].cpu().numpy()[clear], pred[clear])


def test_regression_within_the_derived_bound():
    """the fp32 sum of k terms in rank order, (k - 1) 2^-24 sum|t|, divided by k and rounded once more: k 2^-24 mean|t| over the neighbours"""
    from ssl_cr_histo_amd import kernels as K
    v = vote_case()
    r = K.knn_vote(v["i"], v["s"], targets=dev(v["tb"]))
    idx = v["i"].cpu().numpy()
    want = R.vote_regress(idx, v["tb"])
    ok = idx >= 0
    mean_abs = np.where(ok, np.abs(v["tb"].astype(np.float64))[np.maximum(idx, 0)], 0).sum(1) / ok.sum(1)
    got = r["pred"].cpu().numpy().astype(np.float64)
    assert r["pred"].dtype == torch.float32 and (np.abs(got - want) <= v["k"] * 2.0 ** -24 * mean_abs).all()


# ------------------------------------------------------------------------------------------------ 5. end to end
def _probe_ref(feats, targets, k, C, q=None, qt=None):
    """the restatement of inference.knn_probe on given features: cosine, the fp32 chain's similarities, uniform votes"""
    fn = R.l2_normalize(feats)
    qn = fn if q is None else R.l2_normalize(q)
    _, idx = R.topk(R.fma_chain(qn, fn), k, self_offset=0 if q is None else None)
    pred, _ = R.vote_uniform(idx, targets, C)
    cm = R.confusion(targets if qt is None else qt, pred, C)
    return pred, cm


def test_steps_knn_probe_through_a_real_net():
    """48 labelled tiles of 64 x 64 in two classes through a BoundNet in fp32 mode: leave-one-out, and bank -> queries"""
    from oracle import cases as C
    from ssl_cr_histo_amd import steps
    from test_engine_gpu import _engine, build, ns
    eng = _engine("fp32")
    model, cls = build("finetune", "finetune", 2, True)
    batches = [(C.u8(600 + n, (16, 3, 64, 64)), C.ints(650 + n, (16,), 2)) for n in range(3)]
    net = eng.bind(model, cls)
    feats = torch.cat([net.forward((x.to(DEV),), train=False)[0].clone() for x, _ in batches]).cpu().numpy()
    y = torch.cat([t for _, t in batches]).numpy()
    assert (R.norm_clearance(feats) > 2.0 ** -40).all()
    r = steps.knn_probe(ns(), model, cls, batches, k=5)
    pred, cm = _probe_ref(feats, y, 5, 2)
    assert np.array_equal(r["pred"], pred) and np.array_equal(r["confusion"], cm)
    assert r["accuracy"] == np.trace(cm) / 48
    r2 = steps.knn_probe(ns(), model, cls, batches[:2], batches[2:], k=3)
    pred2, cm2 = _probe_ref(feats[:32], y[:32], 3, 2, feats[32:], y[32:])
    assert np.array_equal(r2["pred"], pred2) and np.array_equal(r2["confusion"], cm2) and r2["accuracy"] == np.trace(cm2) / 16


def test_inference_knn_probe_on_what_rsp_train_returns():
    from oracle import cases as C
    from ssl_cr_histo_amd import inference as I
    from ssl_cr_histo_amd import steps
    from test_engine_gpu import _engine, build, ns
    _engine("fp32")
    model, cls = build("triplet", "mlp", 6, False)
    opt = torch.optim.SGD(list(model.parameters()) + list(cls.parameters()), lr=0.01, momentum=0.9, weight_decay=1e-4, nesterov=True)
    batch = tuple(C.u8(700 + j, (12, 3, 64, 64)) for j in range(3)) + (C.ints(710, (12,), 6).view(-1, 1),)
    _, _, final_feats, final_targets = steps.rsp_train(ns(tile_h=64, tile_w=64), model, cls, [batch], torch.nn.CrossEntropyLoss(), opt, 1)
    assert final_feats.is_cuda and final_feats.shape == (12, 768)
    r = I.knn_probe(final_feats, final_targets, k=3, n_classes=6)
    feats = final_feats.cpu().numpy()
    assert (R.norm_clearance(feats) > 2.0 ** -40).all()
    pred, cm = _probe_ref(feats, final_targets.cpu().numpy(), 3, 6)
    assert np.array_equal(r["pred"], pred) and np.array_equal(r["confusion"], cm) and r["accuracy"] == np.trace(cm) / 12
    assert set(r) >= {"accuracy", "confusion", "pred", "weighted_f1"}


# ------------------------------------------------------------------------------------------------ 6. empty slices, the C-ABI's nb_valid, the probe's arguments
@pytest.mark.parametrize("slices", [40, 65])
def test_a_hint_that_leaves_trailing_slices_empty(slices):
    """65 bank tiles on 40 slices are 2 tiles a slice: slices 33 .. 39 walk nothing and must write EMPTY lists (they store list rows
    that other waves zeroed: a barrier stands between).  Run after a call that left large keys in LDS."""
    from ssl_cr_histo_amd import kernels as K
    nq, nb, D, k = 65, 4097, 12, 64
    p = K.knn_plan(nq, nb, D, k, slices)
    assert p["slices"] == slices and (slices - 1) * p["tiles_per_slice"] >= 65 or slices == 65
    q, b = ints(60, nq, D), ints(61, nb, D)
    want = R.topk(R.similarity(q, b), k)
    topk(np.full((nq, D), 3, np.float32), np.full((nb, D), 3, np.float32), k)      # every list slot of every workgroup holds a big key
    for _ in range(3):
        same(topk(q, b, k, slices=slices), want)


@pytest.mark.parametrize("nb_valid", [0, 1, 64, 65, 700])
def test_nb_valid_through_the_c_abi(nb_valid):
    """kernels.knn_topk hands the library the prefix as the bank; the descriptor's own nb_valid < nb (bank tiles past it are not walked,
    their slices write empty lists) is reached here"""
    from ssl_cr_histo_amd import _lib as L
    nq, nb, D, k = 9, 1300, 8, 20
    q, b = ints(62, nq, D), ints(63, nb, D)
    qd, bd = dev(q), dev(b)
    for slices in (0, 1, 5):
        plan = L.KnnPlan()
        L.check(L.lib().sslcr_knn_plan(nq, nb, D, k, slices, plan))
        s = torch.empty((nq, k), dtype=torch.float32, device=DEV)
        i = torch.empty((nq, k), dtype=torch.int32, device=DEV)
        ws = torch.empty(max(1, plan.workspace_bytes // 8), dtype=torch.int64, device=DEV)
        d = L.KnnDesc(L.ptr(qd), L.ptr(bd), L.ptr(s), L.ptr(i), L.ptr(ws), nq, nb, D, k, nb_valid, -1, slices)
        L.check(L.lib().sslcr_knn_topk(d, L.stream_ptr()))
        same((s.cpu().numpy(), i.cpu().numpy()), R.topk(R.similarity(q, b), k, nb_valid=nb_valid))


def test_probe_class_count_and_targets_out_of_range():
    from ssl_cr_histo_amd import inference as I
    feats = dev(floats(70, 40, 16))
    y = np.random.RandomState(71).randint(0, 3, 40)
    y[0] = 2
    yd = dev(y)
    a = I.knn_probe(feats, yd, k=3, n_classes=3)
    b = I.knn_probe(feats, yd, k=3)                                  # the count read off the labels
    assert a["confusion"].shape == (3, 3) and np.array_equal(a["confusion"], b["confusion"]) and np.array_equal(a["pred"], b["pred"])
    assert a["confusion"].sum() == 40
    wide = I.knn_probe(feats, yd, k=3, n_classes=5)
    assert wide["confusion"].shape == (5, 5) and np.array_equal(wide["confusion"][:3, :3], a["confusion"]) and wide["accuracy"] == a["accuracy"]
    with pytest.raises(ValueError, match="outside"):
        I.knn_probe(feats, yd, k=3, n_classes=2)                     # targets 2 cannot be counted: not averaged over fewer rows
    # bank -> queries with a query label the bank never saw: the count covers it
    r = I.knn_probe(feats[:30], dev(np.minimum(y[:30], 1)), k=3, leave_one_out=False, queries=feats[30:], query_targets=dev(np.full(10, 2)))
    assert r["confusion"].shape == (3, 3) and r["confusion"][2].sum() == 10 and r["accuracy"] == 0.0
    bank = I.FeatureBank(16, n_classes=3).add(feats, yd).finalize()
    assert bank.class_count() == 3 and I.FeatureBank(16).add(feats, yd).class_count() == 3


def test_steps_knn_probe_regression_and_its_keywords():
    """float targets (the BreastPathQ head): the k-NN regressor, leave-one-out; keywords that do not apply raise"""
    from oracle import cases as C
    from ssl_cr_histo_amd import steps
    from test_engine_gpu import _engine, build, ns
    eng = _engine("fp32")
    model, cls = build("finetune", "finetune", 1, True)
    batches = [(C.u8(800 + n, (8, 3, 64, 64)), C.f32(850 + n, (8,))) for n in range(2)]
    net = eng.bind(model, cls)
    feats = torch.cat([net.forward((x.to(DEV),), train=False)[0].clone() for x, _ in batches]).cpu().numpy()
    t = torch.cat([v for _, v in batches]).numpy()
    r = steps.knn_probe(ns(), model, cls, batches, k=3)
    fn = R.l2_normalize(feats)
    _, idx = R.topk(R.fma_chain(fn, fn), 3, self_offset=0)
    want = R.vote_regress(idx, t)
    mean_abs = np.abs(t.astype(np.float64))[idx].mean(1)
    assert (np.abs(r["pred"].astype(np.float64) - want) <= 3 * 2.0 ** -24 * mean_abs).all()
    assert abs(r["mse"] - ((want - t) ** 2).mean()) <= 1e-5 * max(1.0, r["mse"])
    with pytest.raises(TypeError, match="weights"):
        steps.knn_probe(ns(), model, cls, batches, k=3, weights="softmax")
    with pytest.raises(TypeError):
        steps.knn_probe(ns(), model, cls, batches, k=3, temperture=0.1)
