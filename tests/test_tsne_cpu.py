"""CPU-only: the NumPy restatement of the t-SNE embedding (tests/_tsne_ref.py, the definition the device is held to) against sklearn
1.7.2 -- ``_utils._binary_search_perplexity``, ``_t_sne._joint_probabilities_nn``, ``_kl_divergence``, ``_gradient_descent``, ``TSNE`` and
``trustworthiness`` -- and the host side of the C-ABI: plan answers, argument refusals, symbols."""
import numpy as np
import pytest

import _tsne_ref as R


@pytest.fixture(scope="module")
def lib():
    from ssl_cr_histo_amd import _lib
    return _lib.lib()


def _features(seed, n, D=16):
    rs = np.random.RandomState(seed)
    return (rs.randn(4, D)[np.arange(n) % 4] * 2.0 + rs.randn(n, D)).astype(np.float32)


@pytest.fixture(scope="module")
def graph():
    """n = 200, perplexity 12, k = 37: neighbours, float32 distances, conditional and joint affinities of the restatement"""
    x = R.center(_features(1, 200))
    k = R.neighbour_k(200, 12.0)
    idx, d2 = R.euclidean_topk(x, k)
    P, beta, steps = R.binary_search_perplexity(d2, 12.0)
    return dict(x=x, k=k, idx=idx, d2=d2, P=P, beta=beta, steps=steps, csr=R.joint_csr(idx, P), perplexity=12.0)


# ---------------------------------------------------------------------------------------------------------------- restatement against sklearn
def test_neighbours_are_the_true_nearest(graph):
    d = R.dist2_f64(graph["x"])
    np.fill_diagonal(d, np.inf)
    want = np.sort(d, 1)[:, :graph["k"]]
    got = np.take_along_axis(d, graph["idx"].astype(np.int64), 1)
    assert (got <= want[:, -1:] + R.topk_slack(graph["x"])[:, None]).all()
    assert np.array_equal(graph["d2"], got.astype(np.float32)) or np.abs(graph["d2"] - got).max() <= 2 ** -22 * got.max()
    assert (np.diff(graph["d2"].astype(np.float64), axis=1) >= -R.topk_slack(graph["x"])[:, None]).all()      # nearest first


def test_affinities_equal_sklearn(graph):
    from sklearn.manifold import _utils
    want = _utils._binary_search_perplexity(graph["d2"], graph["perplexity"], 0)
    assert graph["steps"].max() <= 100
    assert np.array_equal(graph["P"], want.astype(np.float32))
    P64, H = R.affinities_at(graph["d2"], graph["beta"])
    assert np.abs(H - np.log(graph["perplexity"])).max() <= 1e-5 + 1e-12
    assert np.abs(P64 - want).max() <= 1e-15


def test_affinities_degenerate_rows_equal_sklearn():
    from sklearn.manifold import _utils
    d = np.random.RandomState(6).rand(20, 16).astype(np.float32) * 8     # more rows than columns: sklearn then skips no column
    d[0] = 2.0                                       # all equal
    d[1, 3:] = 4.0                                   # duplicates at distance 0, fewer than the perplexity
    d[2, 9:] = 4.0                                   # ... more than the perplexity: beta runs to 2^100
    d[2, :9] = 0.0
    d[1, :3] = 0.0
    d[3] = np.arange(16)
    d[4] = 1e30
    d[5] = 0.0
    for perp in (5.0, 2.5):
        got, _, _ = R.binary_search_perplexity(d, perp)
        assert np.array_equal(got, _utils._binary_search_perplexity(d, perp, 0).astype(np.float32))
    one = np.array([[3.0], [0.0], [1e-3]], np.float32)                   # k = 1
    assert np.array_equal(R.binary_search_perplexity(one, 0.5)[0], _utils._binary_search_perplexity(one, 0.5, 0).astype(np.float32))


def test_joint_csr_against_sklearn(graph):
    from scipy.sparse import csr_matrix
    from sklearn.manifold import _t_sne
    n, k = graph["idx"].shape
    dist = csr_matrix((graph["d2"].reshape(-1).astype(np.float64), graph["idx"].reshape(-1), np.arange(0, n * k + 1, k)), shape=(n, n))
    want = _t_sne._joint_probabilities_nn(dist, graph["perplexity"], 0).toarray()
    rowptr, col, val = graph["csr"]
    got = R.densify(rowptr, col, val)
    assert np.array_equal(got != 0, want != 0)
    nz = want != 0
    assert np.abs(got[nz] / want[nz] - 1).max() <= 1e-5
    assert np.array_equal(got, got.T) and (np.diff(rowptr) >= k).all()
    for i in (0, 17, n - 1):
        assert (np.diff(col[rowptr[i]:rowptr[i + 1]]) > 0).all()                          # columns rise within a row
    assert abs(got.sum() - 1) <= 1e-5


def _sk_kl(y, P, n):
    from scipy.spatial.distance import squareform
    from sklearn.manifold import _t_sne
    kl, g = _t_sne._kl_divergence(y.ravel().copy(), squareform(P, checks=False), 1.0, n, 2)
    return kl, g.reshape(n, 2)


@pytest.mark.parametrize("scale", [1e-4, 1.0, 30.0])
def test_gradient_and_kl_against_sklearn(graph, scale):
    n = len(graph["x"])
    P = R.densify(*graph["csr"])
    y = np.random.RandomState(3).randn(n, 2) * scale
    got = R.gradient(y, P, 1.0)
    kl, g = _sk_kl(y, P, n)
    assert np.abs(got["grad"] - g).max() <= 1e-9 * np.abs(g).max()
    assert abs(got["kl"] - kl) <= 1e-9 * abs(kl)
    e = R.gradient(y, P, 12.0)                       # exaggeration multiplies P
    kl12, g12 = _sk_kl(y, 12.0 * P, n)
    assert np.abs(e["grad"] - g12).max() <= 1e-9 * np.abs(g12).max()


def test_complete_graph_is_sklearns_exact_method():
    """n = 60, k = 59: every pair is a neighbour, so the sparse definition IS ``method="exact"``: the float64 conditional affinities
    against ``_joint_probabilities`` on the same float32 distances, then gradient and KL"""
    from scipy.spatial.distance import squareform
    from sklearn.manifold import _t_sne
    n = 60
    x = R.center(_features(2, n))
    k = R.neighbour_k(n, 20.0)
    assert k == n - 1
    idx, d2 = R.euclidean_topk(x, k)
    dense = np.zeros((n, n), np.float32)
    np.put_along_axis(dense, idx.astype(np.int64), d2, 1)
    want = squareform(_t_sne._joint_probabilities(dense, 20.0, 0))
    P32, beta, _ = R.binary_search_perplexity(d2, 20.0)
    P64, _ = R.affinities_at(d2, beta)
    cond = np.zeros((n, n))
    np.put_along_axis(cond, idx.astype(np.int64), P64, 1)
    joint = (cond + cond.T) / (2.0 * n)
    assert np.abs(joint - want).max() <= 2e-16
    # the float32 storage of the conditional affinities is the one difference: 2^-24 relative
    got = R.densify(*R.joint_csr(idx, P32))
    off = ~np.eye(n, dtype=bool)
    assert np.abs(got[off] / want[off] - 1).max() <= 2.0 ** -23
    y = np.random.RandomState(4).randn(n, 2)
    mine, (kl, g) = R.gradient(y, joint, 1.0), _sk_kl(y, want, n)
    assert np.abs(mine["grad"] - g).max() <= 1e-12 and abs(mine["kl"] - kl) <= 1e-11


@pytest.mark.parametrize("exaggeration,momentum,lr", [(12.0, 0.5, 4.0), (1.0, 0.8, 50.0)])
def test_update_against_sklearn_gradient_descent(graph, exaggeration, momentum, lr):
    """fifty iterations of the restated update against sklearn's driver on the same objective, in both stages' settings.  (The
    exaggerated stage runs at lr 4 here: at the floor of 50 its 200 points are chaotic, a difference in the last bit grows tenfold
    every 2.5 iterations and reaches 1e-3 after 40, in sklearn against itself as much as here -- nothing a rule could be held to.)"""
    from scipy.spatial.distance import squareform
    from sklearn.manifold import _t_sne
    n = len(graph["x"])
    P = R.densify(*graph["csr"])
    y0 = R.pca_init(graph["x"])
    want, _, it = _t_sne._gradient_descent(_t_sne._kl_divergence, y0.ravel().copy(), 0, 50, n_iter_check=50, momentum=momentum, learning_rate=lr,
                                           args=[squareform(exaggeration * P, checks=False), 1.0, n, 2], kwargs={})
    assert it == 49
    y, update, gains = y0.copy(), np.zeros_like(y0), np.ones_like(y0)
    for _ in range(50):
        y, update, gains = R.update_step(y, update, gains, R.gradient(y, P, exaggeration)["grad"], momentum, lr)
    assert np.abs(y - want.reshape(n, 2)).max() <= 1e-10 * np.abs(want).max()
    assert gains.min() < 1.0 < gains.max()           # both branches of the gain rule ran
    assert R.schedule(249) == (12.0, 0.5) and R.schedule(250) == (1.0, 0.8)
    assert R.learning_rate(240) == 50.0 and R.learning_rate(7180) == 7180 / 48.0


def test_trustworthiness_equals_sklearn():
    from sklearn.manifold import trustworthiness
    rs = np.random.RandomState(5)
    x = rs.randn(150, 12)
    y = x[:, :2] + 0.5 * rs.randn(150, 2)
    for k in (1, 5, 12):
        assert R.trustworthiness(x, y, k) == trustworthiness(x, y, n_neighbors=k)


def test_quality_beside_sklearn():
    """n = 240, four clusters, perplexity 30 (k = 64, sklearn: 91), 500 iterations: the restatement is no worse than the worse of
    sklearn's exact and Barnes-Hut runs by more than the distance between those two"""
    from sklearn.manifold import TSNE, trustworthiness
    x, _ = R.four_clusters()
    n = len(x)
    assert R.neighbour_k(n, 30.0) == 64
    P = R.densify(*R.affinities(x, 30.0))
    y, kl = R.fit(P, R.pca_init(R.center(x)), 500)
    mine = (R.trustworthiness(x, y), kl)
    sk = {}
    for method in ("exact", "barnes_hut"):
        t = TSNE(perplexity=30.0, max_iter=500, init="pca", method=method, random_state=0, n_jobs=1)
        emb = t.fit_transform(x)
        sk[method] = (trustworthiness(x, emb), t.kl_divergence_)
    print(f"trustworthiness / KL: restatement {mine[0]:.4f} / {mine[1]:.4f}, exact {sk['exact'][0]:.4f} / {sk['exact'][1]:.4f}, "
          f"barnes_hut {sk['barnes_hut'][0]:.4f} / {sk['barnes_hut'][1]:.4f}")
    tw, kls = [v[0] for v in sk.values()], [v[1] for v in sk.values()]
    assert mine[0] >= min(tw) - abs(tw[0] - tw[1])
    assert mine[1] <= max(kls) + abs(kls[0] - kls[1])


def test_refuses_a_perplexity_the_neighbours_cannot_carry():
    with pytest.raises(ValueError):
        R.neighbour_k(10, 9.0)
    with pytest.raises(ValueError):
        R.neighbour_k(10000, 64.0)                   # the cap at 64 neighbours
    assert R.neighbour_k(10000, 30.0) == 64 and R.neighbour_k(20, 5.0) == 16 and R.neighbour_k(3, 1.5) == 2


# ---------------------------------------------------------------------------------------------------------------- host side of the library
@pytest.mark.parametrize("n", [2, 3, 255, 256, 257, 1025, 2049, 7180, 20000, 1 << 20])
@pytest.mark.parametrize("hint", [0, 1, 2, 7, 1000])
def test_plan(lib, n, hint):
    from ssl_cr_histo_amd import _lib as L
    from ssl_cr_histo_amd import kernels as K
    p = K.tsne_plan(n, hint)
    T, C, S = p["tile"], p["chunk"], p["slices"]
    chunks = -(-n // C)
    assert (T, C) == (L.TSNE_TILE, L.TSNE_CHUNK)
    assert 1 <= S <= min(chunks, L.TSNE_MAX_SLICES)
    if hint:
        assert S == min(hint, chunks, L.TSNE_MAX_SLICES)
    else:
        assert (S - 1) * p["chunks_per_slice"] < chunks                                  # the plan's own choice leaves no slice empty
        assert S == chunks or -(-n // T) * S >= 1024 or S == L.TSNE_MAX_SLICES or -(-chunks // p["chunks_per_slice"]) == S
    assert S * p["chunks_per_slice"] >= chunks                                           # the slices cover every column
    assert p["grid"] == (-(-n // T) * S, 1, -(-n // 4))
    assert p["workspace_bytes"] == n * S * 16 and p["lds_bytes"] == 8 * C


def test_argument_validation_without_a_device(lib):
    from ssl_cr_histo_amd import _lib as L
    plan = L.TsnePlan()
    for args, word in (((1, 0), b"n outside"), (((1 << 20) + 1, 0), b"n outside"), ((10, -1), b"slices < 0")):
        assert lib.sslcr_tsne_plan(*args, plan) == -1 and word in lib.sslcr_last_error(), args
    assert lib.sslcr_tsne_plan(10, 0, None) == -1
    assert lib.sslcr_tsne_pair_dist2(256, 512, 1024, 1, 8, 4, None) == -1 and b"n outside" in lib.sslcr_last_error()
    assert lib.sslcr_tsne_pair_dist2(256, 512, 1024, 9, 8, 65, None) == -1 and b"k outside" in lib.sslcr_last_error()
    assert lib.sslcr_tsne_pair_dist2(256, None, 1024, 9, 8, 4, None) == -1 and b"null tensor" in lib.sslcr_last_error()
    assert lib.sslcr_tsne_pair_dist2(256, 514, 1024, 9, 8, 4, None) == -1 and b"alignment" in lib.sslcr_last_error()
    assert lib.sslcr_tsne_affinities(256, 512, 1024, 9, 0, 5.0, None) == -1 and b"k outside" in lib.sslcr_last_error()
    assert lib.sslcr_tsne_affinities(256, 512, 1024, 9, 4, 0.0, None) == -1 and b"perplexity" in lib.sslcr_last_error()
    assert lib.sslcr_tsne_affinities(256, 512, 1028, 9, 4, 2.0, None) == -1 and b"alignment" in lib.sslcr_last_error()
    assert lib.sslcr_tsne_repulsion(None, None) == -1 and b"null descriptor" in lib.sslcr_last_error()
    ok = dict(y=256, y_out=512, update=1024, gains=2048, grad=4096, rowptr=8192, col=16384, val=32768, workspace=65536, Z=131072, n=10, slices=0,
              nnz=40, exaggeration=1.0, momentum=0.5, lr=50.0, min_gain=0.01)
    for change, word in ((dict(y=None), b"null tensor"), (dict(Z=None), b"null tensor"), (dict(n=1), b"n outside"), (dict(slices=-1), b"slices < 0"),
                         (dict(workspace=65544), b"alignment"), (dict(y=260), b"alignment")):
        d = L.TsneGradDesc(**{**ok, **change})
        assert lib.sslcr_tsne_repulsion(d, None) == -1 and word in lib.sslcr_last_error(), change
    for change, word in ((dict(y_out=256), b"y_out == y"), (dict(col=None), b"null tensor"), (dict(update=None), b"null tensor"), (dict(nnz=-1), b"nnz"),
                         (dict(kl_rows=12), b"alignment"), (dict(gains=2052), b"alignment")):
        d = L.TsneGradDesc(**{**ok, **change})
        assert lib.sslcr_tsne_update(d, None) == -1 and word in lib.sslcr_last_error(), change
    assert lib.sslcr_tsne_kl(None, 256, 512, 1024, 10, 0, None) == -1 and b"null tensor" in lib.sslcr_last_error()
    assert lib.sslcr_version() == 16                 # the t-SNE entries are told by their symbols (16 is the switch listing's)


def test_symbols_and_python_layer(lib):
    import torch
    from ssl_cr_histo_amd import _lib as L
    from ssl_cr_histo_amd import build
    from ssl_cr_histo_amd import inference as I
    from ssl_cr_histo_amd import kernels as K
    names = [s for s in build.header_symbols() if s.startswith("sslcr_tsne_")]
    assert names == sorted(["sslcr_tsne_plan", "sslcr_tsne_pair_dist2", "sslcr_tsne_affinities", "sslcr_tsne_repulsion", "sslcr_tsne_update",
                            "sslcr_tsne_kl"])
    for s in names:
        assert s in L.SIGNATURES and getattr(lib, s)
    x = torch.zeros(8, 4)
    for call in (lambda: K.euclidean_topk(x, 2), lambda: K.tsne_affinities(x, 2.0), lambda: K.tsne_gradient(x[:, :2].contiguous(), (x, x, x)),
                 lambda: I.Tsne(max_iter=1).fit(x)):
        with pytest.raises(L.SslcrError):
            call()
    with pytest.raises(ValueError):
        I.Tsne(init="spectral")
    with pytest.raises(ValueError):
        I.Tsne.neighbours(10, 9.0)
    assert I.Tsne.neighbours(7180, 30.0) == 64
