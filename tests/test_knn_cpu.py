"""CPU-only: the k-NN probe's plan and argument validation (host side of the C-ABI, no device), and the NumPy restatement the device
is held to (tests/_knn_ref.py) against sklearn 1.7.2's brute-force neighbours, classifier and regressor."""
import numpy as np
import pytest

import _knn_ref as R


@pytest.fixture(scope="module")
def lib():
    from ssl_cr_histo_amd import _lib
    return _lib.lib()


# ---------------------------------------------------------------------------------------------------------------- plan
@pytest.mark.parametrize("nq", [1, 63, 64, 65, 7180])
@pytest.mark.parametrize("nb", [1, 64, 129, 4097, 100000])
@pytest.mark.parametrize("D,k", [(4, 1), (68, 20), (768, 64), (2048, 5)])
def test_plan_workspace_holds_every_partial_list(lib, nq, nb, D, k):
    from ssl_cr_histo_amd import _lib as L
    from ssl_cr_histo_amd import kernels as K
    p = K.knn_plan(nq, nb, D, k)
    S, b_tiles = p["slices"], -(-nb // p["tile_b"])
    assert (p["tile_q"], p["tile_b"], p["chunk"]) == (L.KNN_TILE, L.KNN_TILE, L.KNN_CHUNK)
    assert 1 <= S <= min(b_tiles, L.KNN_MAX_SLICES)
    assert p["workspace_bytes"] == S * nq * k * 8                       # S lists of k 8-byte keys per query
    assert S * p["tiles_per_slice"] >= b_tiles                          # the slices cover the bank
    assert (S - 1) * p["tiles_per_slice"] < b_tiles or S == 1           # the plan's own choice leaves no slice empty
    assert p["grid"] == (-(-nq // p["tile_q"]) * S, -(-nq // 4))
    assert p["form"] == ("sliced" if S > 1 else "direct")               # the form word names the route
    assert 0 < p["lds_bytes"] <= 80 * 1024                              # two workgroups a CU


def test_plan_fills_the_chip_for_few_queries(lib):
    from ssl_cr_histo_amd import kernels as K
    p = K.knn_plan(64, 100000, 768, 20)
    assert p["form"] == "sliced" and p["grid"][0] >= 256                # one query tile: the slices are the grid
    assert p["tiles_per_slice"] >= 4
    assert K.knn_plan(7180, 100000, 768, 20)["grid"][0] >= 512


@pytest.mark.parametrize("hint", [1, 2, 7, 65, 5000])
def test_plan_honours_the_slices_hint(lib, hint):
    from ssl_cr_histo_amd import _lib as L
    from ssl_cr_histo_amd import kernels as K
    nb = 4097                                                           # 65 bank tiles
    p = K.knn_plan(64, nb, 768, 64, slices=hint)
    assert p["slices"] == min(hint, 65, L.KNN_MAX_SLICES)
    assert p["slices"] * p["tiles_per_slice"] >= 65
    assert p["form"] == ("sliced" if p["slices"] > 1 else "direct")
    assert p["workspace_bytes"] == p["slices"] * 64 * 64 * 8


# ---------------------------------------------------------------------------------------------------------------- validation
def test_argument_validation_without_a_device(lib):
    from ssl_cr_histo_amd import _lib as L
    plan = L.KnnPlan()
    for args, word in (((1, 1, 6, 1, 0), b"D % 4"), ((1, 1, 0, 1, 0), b"D % 4"), ((1, 1, 2052, 1, 0), b"D % 4"), ((1, 1, 4, 0, 0), b"k outside"),
                       ((1, 1, 4, 65, 0), b"k outside"), ((1, 0, 4, 1, 0), b"nb outside"), ((-1, 1, 4, 1, 0), b"nq < 0"),
                       ((1, 1, 4, 1, -1), b"slices < 0")):
        assert lib.sslcr_knn_plan(*args, plan) == -1, args
        assert word in lib.sslcr_last_error(), (args, lib.sslcr_last_error())
    assert lib.sslcr_knn_plan(1, 1, 4, 1, 0, None) == -1
    assert lib.sslcr_knn_plan(2 ** 31 - 1, 100000, 4, 1, 1024, plan) == -1 and b"2^31" in lib.sslcr_last_error()   # the grid would not fit an int
    assert lib.sslcr_knn_plan(2 ** 31 - 1, 100000, 4, 1, 1, plan) == 0 and plan.grid[0] == 2 ** 25
    assert lib.sslcr_knn_topk(None, None) == -1 and b"null descriptor" in lib.sslcr_last_error()
    ok = dict(queries=256, bank=512, scores=1024, indices=2048, workspace=4096, nq=3, nb=10, D=8, k=4, nb_valid=10, self_offset=-1, slices=0)
    for change, word in ((dict(queries=None), b"null tensor"), (dict(workspace=None), b"null tensor"), (dict(queries=264), b"16-byte"),
                         (dict(bank=516), b"16-byte"), (dict(workspace=4100), b"alignment"), (dict(indices=2050), b"alignment"),
                         (dict(nb_valid=11), b"nb_valid"), (dict(nb_valid=-1), b"nb_valid"), (dict(self_offset=-2), b"self_offset"),
                         (dict(D=10), b"D % 4"), (dict(k=65), b"k outside")):
        d = L.KnnDesc(**{**ok, **change})
        assert lib.sslcr_knn_topk(d, None) == -1, change
        assert word in lib.sslcr_last_error(), (change, lib.sslcr_last_error())
    assert lib.sslcr_knn_topk(L.KnnDesc(**{**ok, "nq": 0}), None) == 0   # nothing to do: nothing is launched
    # normalisation
    assert lib.sslcr_l2_normalize(None, None, 0, 8, 1e-12, None) == 0
    assert lib.sslcr_l2_normalize(None, 256, 2, 8, 1e-12, None) == -1 and b"null tensor" in lib.sslcr_last_error()
    assert lib.sslcr_l2_normalize(256, 256, 2, 0, 1e-12, None) == -1
    assert lib.sslcr_l2_normalize(256, 256, 2, 8, -1.0, None) == -1 and b"eps" in lib.sslcr_last_error()
    assert lib.sslcr_l2_normalize(258, 256, 2, 8, 0.0, None) == -1 and b"alignment" in lib.sslcr_last_error()
    # votes
    vok = dict(indices=256, scores=512, labels=1024, pred=2048, votes=4096, nq=3, k=4, nb=10, C=9, mode=0, temperature=0.07)
    for change, word in ((dict(indices=None), b"null indices"), (dict(labels=None), b"classification needs"), (dict(C=65), b"C outside"),
                         (dict(C=0), b"C outside"), (dict(k=0), b"k outside"), (dict(mode=3), b"mode"), (dict(mode=1, temperature=0.0), b"temperature"),
                         (dict(mode=1, scores=None), b"needs scores"), (dict(confusion=8192), b"query_labels"), (dict(labels=1028), b"alignment"),
                         (dict(mode=2), b"regression mode needs"), (dict(mode=2, targets=64, pred_value=128, confusion=8192), b"no confusion")):
        d = L.KnnVoteDesc(**{**vok, **change})
        assert lib.sslcr_knn_vote(d, None) == -1, change
        assert word in lib.sslcr_last_error(), (change, lib.sslcr_last_error())
    assert lib.sslcr_knn_vote(L.KnnVoteDesc(**{**vok, "nq": 0}), None) == 0


def test_python_layer_refuses_host_tensors(lib):
    import torch
    from ssl_cr_histo_amd import _lib as L
    from ssl_cr_histo_amd import inference as I
    from ssl_cr_histo_amd import kernels as K
    x = torch.zeros(4, 8)
    with pytest.raises(L.SslcrError):
        K.knn_topk(x, x, 2)
    with pytest.raises(L.SslcrError):
        K.l2_normalize(x)
    with pytest.raises(L.SslcrError):
        K.knn_vote(torch.zeros(4, 2, dtype=torch.int32), None, labels=torch.zeros(4, dtype=torch.int64), n_classes=2)
    with pytest.raises(ValueError):
        I.FeatureBank(8, metric="euclid")


# ---------------------------------------------------------------------------------------------------------------- restatement
def test_key_order_is_the_float_order():
    s = np.array([-np.inf, -3.5, -1e-40, -0.0, 0.0, 1e-40, 2.0, np.inf], np.float32)
    k = R.score_keys(s)
    assert k[3] == k[4] and (np.diff(k.astype(np.int64))[[0, 1, 2, 4, 5, 6]] > 0).all()
    assert k[0] == 0x007FFFFF and k[-1] == 0xFF800000
    assert (R.score_keys(np.array([np.nan, -np.nan], np.float32)) == R.NAN_KEY).all()
    sc, ix = R.topk(np.array([[1.0, np.nan, 1.0, -np.inf, 0.0, -0.0]]), 8)
    assert ix.tolist() == [[0, 2, 4, 5, 3, 1, -1, -1]]
    assert np.isnan(sc[0, 5]) and sc[0, 6] == -np.inf and not np.signbit(sc[0, 3])


SEED = 20                        # chosen so that the reference alone stays inside both caps below (checked by the test itself)


def _clustered(seed, nb=2000, nq=300, D=64, C=9):
    """seeded Gaussian features around one Gaussian centre per class"""
    rs = np.random.RandomState(seed)
    centres = rs.randn(C, D)
    yb, yq = rs.randint(0, C, nb), rs.randint(0, C, nq)
    return (centres[yb] * 0.5 + rs.randn(nb, D)).astype(np.float32), yb, (centres[yq] * 0.5 + rs.randn(nq, D)).astype(np.float32), yq


@pytest.mark.parametrize("k", [1, 5, 20])
def test_restatement_against_sklearn(k):
    from sklearn.neighbors import KNeighborsClassifier, KNeighborsRegressor, NearestNeighbors
    C = 9
    bank, yb, q, yq = _clustered(SEED)
    tb = np.random.RandomState(SEED + 1).rand(len(bank))
    bn, qn = R.l2_normalize(bank).astype(np.float64), R.l2_normalize(q).astype(np.float64)
    s64 = qn @ bn.T
    top_s, top_i = R.topk_f64(s64, k + 1)
    idx = np.stack([i[:k] for i in top_i])
    gap = np.array([s[k - 1] - s[k] for s in top_s])
    keep = gap >= 1e-9
    assert (~keep).mean() <= 0.01
    # neighbours
    nn = NearestNeighbors(n_neighbors=k, algorithm="brute", metric="cosine").fit(bn)
    _, want = nn.kneighbors(qn)
    assert np.array_equal(idx[keep], want[keep])
    # the key form of the order gives the float64 order wherever float32 keeps the scores apart
    exact = np.round(s64 * 1024).astype(np.float64)                     # integers: exact in float32, ties everywhere
    ks, ki = R.topk(exact, k)
    fs, fi = R.topk_f64(exact, k)
    assert np.array_equal(ki, np.stack(fi)) and np.array_equal(ks.astype(np.float64), np.stack(fs))
    # classifier: uniform votes, ties to the lowest class
    pred, counts = R.vote_uniform(idx, yb, C)
    srt = np.sort(counts, 1)
    tied = srt[:, -1] == srt[:, -2]
    assert tied.mean() <= 0.10
    clf = KNeighborsClassifier(n_neighbors=k, algorithm="brute", metric="cosine", weights="uniform").fit(bn, yb)
    want_pred = clf.predict(qn)
    assert np.array_equal(pred[keep & ~tied], want_pred[keep & ~tied])
    assert np.array_equal(pred[keep & tied], want_pred[keep & tied])     # sklearn is the authority for the tie rule: the lowest class
    assert counts.sum(1).tolist() == [k] * len(q)
    assert np.array_equal(R.confusion(yq, pred, C).sum(1), np.bincount(yq, minlength=C))
    # regressor: the mean of the neighbours' targets
    reg = KNeighborsRegressor(n_neighbors=k, algorithm="brute", metric="cosine").fit(bn, tb)
    assert np.allclose(R.vote_regress(idx, tb)[keep], reg.predict(qn)[keep], rtol=0, atol=k * 2.0 ** -52)
    # the softmax vote with a huge temperature is the uniform one
    _, votes = R.vote_softmax(idx, np.stack([s[:k] for s in top_s]), yb, C, 1e12)
    assert np.allclose(votes, counts, rtol=0, atol=1e-9)
