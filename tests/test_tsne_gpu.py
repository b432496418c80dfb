"""The t-SNE embedding on the MI355X (csrc/tsne.hip, include/sslcr.h) against tests/_tsne_ref.py, the float64 restatement that
tests/test_tsne_cpu.py pins to sklearn 1.7.2.

Shapes come from the plan's row tile T and chunk C: n in {2, 3, 65, T - 1, T, T + 1, C + 1, 2 C + 1}, slice hints 1, 2, 7 and the
plan's own.  Neighbours on integer features, degenerate affinity rows and the joint CSR are EQUAL to the restatement; the affinities,
the gradient, Z and the update hold per-element float64 bounds derived in _tsne_ref.py from the operation count, nothing left out;
the end-to-end figures lie beside five restatement runs that differ by float32-sized roundings only."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _tsne_ref as R  # noqa: E402

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATIOS = os.path.join(ROOT, "profiles", "tsne_ratios.txt")
T, C = 256, 1024                 # asserted against the plan below
SIZES = sorted({2, 3, 65, T - 1, T, T + 1, C + 1, 2 * C + 1})
HINTS = (1, 2, 7, None)


def dev(a):
    return torch.as_tensor(a).to(DEV)


FRESH = set()                    # the names this run has written: a worst ratio is the worst of THIS run's cases


def record(name, value, worst=False):
    """profiles/tsne_ratios.txt: one ``name value`` line per measured figure, rewritten in name order; worst: keep the greater of
    this run's values under the name (the cases of a parametrised test share it)"""
    lines = {}
    if os.path.exists(RATIOS):
        with open(RATIOS) as f:
            lines = dict(ln.split(None, 1) for ln in f.read().splitlines() if ln.strip() and not ln.startswith("#"))
    if worst and name in FRESH:
        value = max(value, float(lines.get(name, value)))
    FRESH.add(name)
    lines[name] = f"{value:.4f}"
    with open(RATIOS, "w") as f:
        f.write("# t-SNE on the MI355X (tests/test_tsne_gpu.py): worst observed / bound of the float comparisons, and the end-to-end figures\n")
        f.write("".join(f"{k} {v}\n" for k, v in sorted(lines.items())))


def test_sizes_are_the_plans():
    from ssl_cr_histo_amd import kernels as K
    p = K.tsne_plan(2 * C + 1)
    assert (p["tile"], p["chunk"]) == (T, C) and SIZES == [2, 3, 65, 255, 256, 257, 1025, 2049]
    assert K.tsne_plan(2 * C + 1, 7)["slices"] == 3 and K.tsne_plan(2 * C + 1, 2)["chunks_per_slice"] == 2


# ------------------------------------------------------------------------------------------------ 1. neighbours
@pytest.mark.parametrize("n", SIZES)
def test_euclidean_topk_equals_the_restatement_on_integer_features(n):
    """entries in {-3 .. 3}: every product, norm and chain is exact (|x|^2 / 2 is a half-integer), ties are everywhere; k = 64 also
    where n - 1 < k: the trailing slots are index -1 and distance +inf"""
    from ssl_cr_histo_amd import kernels as K
    x = np.random.RandomState(n).randint(-3, 4, (n, 8)).astype(np.float32)
    idx, d2 = K.euclidean_topk(dev(x), 64)
    assert idx.dtype == torch.int32 and d2.dtype == torch.float32 and idx.shape == d2.shape == (n, 64)
    widx, wd2 = R.euclidean_topk(x, 64)
    assert np.array_equal(idx.cpu().numpy(), widx)
    assert np.array_equal(d2.cpu().numpy(), wd2)


def test_euclidean_topk_on_floats_holds_the_chain_bound():
    """every returned neighbour's float64 distance against the k-th true one, within the fma chain's derived slack; the recomputed
    distances are EQUAL to the restatement's on the device's own indices; any D (the width is padded)"""
    from ssl_cr_histo_amd import kernels as K
    worst = 0.0
    for n, D, k in ((1025, 36, 64), (257, 2, 5), (65, 7, 20)):
        rs = np.random.RandomState(D)
        x = (rs.randn(n, D) + 3.0 * rs.randn(4, D)[np.arange(n) % 4]).astype(np.float32)
        idx, d2 = (t.cpu().numpy() for t in K.euclidean_topk(dev(x), k))
        assert (idx >= 0).all() and (idx != np.arange(n)[:, None]).all()
        assert all(len(set(r)) == k for r in idx)
        full = R.dist2_f64(x)
        np.fill_diagonal(full, np.inf)
        kth = np.sort(full, 1)[:, k - 1]
        got = np.take_along_axis(full, idx.astype(np.int64), 1)
        slack = R.topk_slack(x)
        assert (got <= kth[:, None] + slack[:, None]).all()
        worst = max(worst, float(((got - kth[:, None]) / slack[:, None]).max()))
        assert np.array_equal(d2, R.pair_dist2(x, idx))
    record("topk_kth_excess", worst)


# ------------------------------------------------------------------------------------------------ 2. conditional affinities
@pytest.mark.parametrize("n,D,perplexity", [(1025, 16, 30.0), (65, 8, 6.0), (257, 4, 2.5)])
def test_affinities_hold_the_float64_formula_at_their_own_beta(n, D, perplexity):
    """beta itself is not compared: a last-bit difference may end the bisection one step apart.  P at the device's beta against the
    float64 formula: exp's argument d beta carries one rounding (relative 2^-53, so d beta 2^-53 in the exponential), the sums k
    roundings, the division and the library functions a few more, then ONE float32 rounding: relative 2^-24 + (2 d beta + k + 16) 2^-52,
    plus half a float32 denormal.  The entropy at the device's beta is within 1e-5 of log(perplexity), plus the float64 roundings of
    the entropy's own terms, (k + d beta + 16) 2^-52 (|log s| + beta sum d P), taken twice (the device's evaluation and this one)."""
    from ssl_cr_histo_amd import kernels as K
    rs = np.random.RandomState(n)
    x = R.center((rs.randn(n, D) + 2.0 * rs.randn(4, D)[np.arange(n) % 4]).astype(np.float32))
    k = R.neighbour_k(n, perplexity)
    _, d2 = R.euclidean_topk(x, k)
    _, _, steps = R.binary_search_perplexity(d2, perplexity)
    assert steps.max() <= 100                        # the restatement exhausts its steps on no row
    P, beta = (t.cpu().numpy() for t in K.tsne_affinities(dev(d2), perplexity))
    assert P.dtype == np.float32 and beta.dtype == np.float64 and P.shape == (n, k)
    want, H = R.affinities_at(d2, beta)
    db = d2.astype(np.float64) * beta[:, None]
    bound = want * (R.U + (2 * db + k + 16) * 2.0 ** -52) + 2.0 ** -150
    err = np.abs(P.astype(np.float64) - want)
    assert (err <= bound).all()
    s = np.exp(-db).sum(1)
    slack = 2 * (k + db.max(1) + 16) * 2.0 ** -52 * (np.abs(np.log(s)) + (db * want).sum(1))
    assert (np.abs(H - np.log(perplexity)) <= 1e-5 + slack).all()
    record("affinities_error", float((err / bound).max()), worst=True)


def test_degenerate_affinity_rows_equal_the_restatement():
    from ssl_cr_histo_amd import kernels as K
    d = np.random.RandomState(6).rand(20, 16).astype(np.float32) * 8
    d[0] = 2.0                                       # all distances equal
    d[1, :3], d[1, 3:] = 0.0, 4.0                    # duplicates at distance 0, fewer than the perplexity
    d[2, :9], d[2, 9:] = 0.0, 4.0                    # ... more: beta doubles a hundred times
    d[3] = np.arange(16)
    d[4] = 1e30
    d[5] = 0.0
    for perplexity in (5.0, 2.5):
        P, _ = K.tsne_affinities(dev(d), perplexity)
        want, _, _ = R.binary_search_perplexity(d, perplexity)
        assert np.array_equal(P.cpu().numpy()[:6], want[:6])
    one = np.array([[3.0], [0.0], [1e-3]], np.float32)                   # k = 1
    assert np.array_equal(K.tsne_affinities(dev(one), 0.5)[0].cpu().numpy(), R.binary_search_perplexity(one, 0.5)[0])


# ------------------------------------------------------------------------------------------------ 3. joint CSR
def _lists(kind, n, k, seed):
    rs = np.random.RandomState(seed)
    if kind == "hub":                                # point 0 is in every list: its row has n - 1 entries
        idx = np.stack([np.concatenate([[0], rs.permutation(np.setdiff1d(np.arange(1, n), [i]))[:k - 1]]) for i in range(n)]).astype(np.int32)
        idx[0] = rs.permutation(np.arange(1, n))[:k]
    elif kind == "random":
        idx = np.stack([rs.permutation(np.setdiff1d(np.arange(n), [i]))[:k] for i in range(n)]).astype(np.int32)
    if kind == "short":                              # fewer other points than slots: what euclidean_topk returns for n - 1 < k
        idx = np.full((n, k), -1, np.int32)
        idx[:, :n - 1] = np.stack([np.setdiff1d(np.arange(n), [i]) for i in range(n)])
    P = rs.rand(n, k).astype(np.float32)
    return idx, (P / P.sum(1, keepdims=True)).astype(np.float32)


@pytest.mark.parametrize("kind,n,k", [("random", 257, 20), ("hub", 300, 8), ("short", 3, 64), ("random", 2049, 64), ("random", 2, 1)])
def test_joint_csr_equals_the_restatement(kind, n, k):
    from ssl_cr_histo_amd import kernels as K
    idx, P = _lists(kind, n, k, n + k)
    got = [t.cpu().numpy() for t in K.tsne_joint(dev(idx), dev(P))]
    again = [t.cpu().numpy() for t in K.tsne_joint(dev(idx), dev(P))]
    rowptr, col, val = R.joint_csr(idx, P)
    nnz = rowptr[-1]
    assert got[0].dtype == np.int32 and got[1].dtype == np.int32 and got[2].dtype == np.float32
    assert np.array_equal(got[0], rowptr)
    assert np.array_equal(got[1][:nnz], col) and np.array_equal(got[2][:nnz], val)
    for a, b in zip(got, again):
        assert np.array_equal(a[:nnz] if a.size > n + 1 else a, b[:nnz] if b.size > n + 1 else b)
    if kind == "hub":
        assert rowptr[1] - rowptr[0] == n - 1


# ------------------------------------------------------------------------------------------------ 4. gradient
def _graph(n, seed=0):
    """a joint CSR on n points: neighbours of random 4-d features, random conditional affinities"""
    rs = np.random.RandomState(seed + n)
    k = min(n - 1, 10)
    idx, _ = R.euclidean_topk(rs.randn(n, 4).astype(np.float32), k)
    P = rs.rand(n, k).astype(np.float32)
    return R.joint_csr(idx, (P / P.sum(1, keepdims=True)).astype(np.float32))


def _embedding(kind, n):
    rs = np.random.RandomState(n)
    y = rs.randn(n, 2)
    if kind == "initial":                            # the state a fit starts from
        y *= 1e-4
    elif kind == "wide":                             # 1 + d^2 reaches 1e8 and beyond
        y *= 3e3
        y[n // 2] = 1e4
    else:                                            # unit scale, coincident points, one row at the initial scale
        y[n // 3] = y[0]
        y[n - 1] = y[0]
        y[1] *= 1e-4
    return y.astype(np.float32)


@pytest.mark.parametrize("kind", ["mixed", "initial", "wide"])
@pytest.mark.parametrize("n", SIZES)
def test_gradient_holds_its_bound_under_every_plan(n, kind):
    from ssl_cr_histo_amd import kernels as K
    csr = _graph(n)
    Pd = R.densify(*csr)
    y = _embedding(kind, n)
    if kind == "wide" and n > 3:
        assert 1.0 + R.dist2_f64(y).max() >= 1e8
    Pt = tuple(dev(a) for a in csr)
    worst_g = worst_z = 0.0
    pieces = R.field(y, Pd)                          # the float64 reference, computed once
    for hint in HINTS:
        plan = K.tsne_plan(n, hint)
        for e in (1.0, 12.0):
            want = R.gradient(y, Pd, e, plan, pieces)
            g, Z = K.tsne_gradient(dev(y), Pt, e, slices=hint)
            g2, Z2 = K.tsne_gradient(dev(y), Pt, e, slices=hint)
            g, Z, g2, Z2 = g.cpu().numpy(), Z.cpu().numpy(), g2.cpu().numpy(), Z2.cpu().numpy()
            assert np.array_equal(g, g2) and np.array_equal(Z, Z2)           # two calls: equal bits
            eg = np.abs(g.astype(np.float64) - want["grad"])
            assert (eg <= want["grad_bound"]).all(), (hint, e, np.argwhere(eg > want["grad_bound"])[:5])
            assert abs(Z[0] - want["Z"]) <= want["Z_bound"]
            worst_g = max(worst_g, float((eg / want["grad_bound"]).max()))
            worst_z = max(worst_z, float(abs(Z[0] - want["Z"]) / want["Z_bound"]))
    record(f"gradient_error_{kind}", worst_g, worst=True)
    record(f"Z_error_{kind}", worst_z, worst=True)


def test_kl_rows_and_log_row():
    from ssl_cr_histo_amd import kernels as K
    n = 257
    csr = _graph(n)
    y = _embedding("mixed", n)
    want = R.gradient(y, R.densify(*csr), 1.0)
    kl_rows = torch.empty(n, dtype=torch.float64, device=DEV)
    g, Z = K.tsne_gradient(dev(y), tuple(dev(a) for a in csr), 1.0, kl_rows=kl_rows)
    row = K.tsne_kl(kl_rows, g, Z, torch.zeros(4, dtype=torch.float64, device=DEV), 77).cpu().numpy()
    # KL is float64 but for Z (float32 partial sums): d KL / d log Z = sum p = 1
    z_rel = abs(Z.item() - want["Z"]) / want["Z"]
    assert abs(row[0] - want["kl"]) <= 2 * z_rel + 1e-12 * abs(want["kl"])
    assert abs(row[1] - np.sqrt((g.cpu().numpy().astype(np.float64) ** 2).sum())) <= 1e-12 * row[1]
    assert row[2] == Z.item() and row[3] == 77.0


# ------------------------------------------------------------------------------------------------ 5. step replay
def test_twelve_steps_replayed_in_float64_across_the_switch():
    """n = 257, iterations 245 .. 256.  Each iteration is replayed in float64 from the state the device fed it.  The gradient the
    update consumes is within ``raw_bound`` B of the float64 one.  gains: where |grad| > B (or update == 0) the sign test is decided
    and gains is EQUAL to the one float32 rounding of the float64 rule; elsewhere either outcome is admissible.  update: momentum *
    update - lr * gains * grad with the device's gains: lr gains B, and one float32 rounding.  y: EQUAL to the one rounding of y +
    update.  The undecided share is capped at 1 % and is 0 under float64's own bound."""
    from ssl_cr_histo_amd import inference as I
    from ssl_cr_histo_amd import kernels as K
    n = 257
    rs = np.random.RandomState(9)
    x = (rs.randn(n, 16) + 2.0 * rs.randn(4, 16)[np.arange(n) % 4]).astype(np.float32)
    t = I.Tsne(perplexity=10.0, init=dev((rs.randn(n, 2) * 1e-4).astype(np.float32)), check_every=5).prepare(dev(x))
    rowptr, col, val = (a.cpu().numpy() for a in t.P)
    Pd = R.densify(rowptr, col[:rowptr[-1]], val[:rowptr[-1]])
    plan = K.tsne_plan(n)
    t.iteration = 245
    undecided = total = 0
    worst = 0.0
    for it in range(245, 257):
        s = t.state
        assert int(s["iteration"].item()) == it
        y, up, ga = (s[k].cpu().numpy().astype(np.float64) for k in ("y", "update", "gains"))
        t.step()
        s = t.state
        y1, up1, ga1, g1 = (s[k].cpu().numpy() for k in ("y", "update", "gains", "grad"))
        e, mom = R.schedule(it)
        assert (e, mom) == ((12.0, 0.5) if it < 250 else (1.0, 0.8))
        want = R.gradient(y, Pd, e, plan)
        g, B = want["grad"], want["raw_bound"]
        assert (np.abs(g1.astype(np.float64) - g) <= want["grad_bound"]).all()
        open_ = (up != 0) & (np.abs(g) <= B)
        assert not ((up != 0) & (np.abs(g) <= want["f64_bound"])).any()
        inc = up * g < 0
        g_inc = np.maximum(ga + 0.2, 0.01).astype(np.float32)
        g_dec = np.maximum(ga * 0.8, 0.01).astype(np.float32)
        assert np.array_equal(ga1[~open_], np.where(inc, g_inc, g_dec)[~open_])
        assert ((ga1 == g_inc) | (ga1 == g_dec)).all()
        nu = mom * up - t.lr * ga1.astype(np.float64) * g
        nb = t.lr * ga1 * B * (1 + R.U) + R.U * np.abs(nu) + 2.0 ** -149
        eu = np.abs(up1.astype(np.float64) - nu)
        assert (eu <= nb).all()
        assert np.array_equal(y1, (y + up1.astype(np.float64)).astype(np.float32))
        worst = max(worst, float((eu / nb).max()))
        undecided += int(open_.sum())
        total += open_.size
    assert undecided <= 0.01 * total
    record("step_update_error", worst)
    record("step_undecided_share", undecided / total)


# ------------------------------------------------------------------------------------------------ 6. end to end
def test_end_to_end_beside_five_restatement_runs():
    """the 240-point set, 500 iterations: final KL and trustworthiness against five runs of the restatement that differ only by
    float32-sized roundings -- float64 state, float32-rounded state, three with the init perturbed by 2^-24 relative -- the error
    class the device adds.  The device must lie within [min - spread, max + spread] of the five, for both figures."""
    from ssl_cr_histo_amd import inference as I
    x, labels = R.four_clusters()
    out = I.tsne(dev(x), dev(labels), perplexity=30.0, max_iter=500)
    emb = out["embedding"]
    assert emb.is_cuda and emb.dtype == torch.float32 and emb.shape == (240, 2) and out["n_iter"] == 500 and out["targets"].shape == (240,)
    got = (out["kl_divergence"], R.trustworthiness(x, emb.cpu().numpy().astype(np.float64)))
    P = R.densify(*R.affinities(x, 30.0))
    y0 = R.pca_init(R.center(x))
    assert np.abs(I.Tsne.pca_init(dev(R.center(x))).cpu().numpy() - y0).max() <= 1e-3 * 1e-4      # unpinned against sklearn; close to NumPy's eigh
    rs = np.random.RandomState(7)
    runs = [R.fit(P, y0, 500), R.fit(P, y0, 500, f32=True)] + [R.fit(P, y0 * (1 + 2.0 ** -24 * rs.choice([-1.0, 1.0], y0.shape)), 500) for _ in range(3)]
    kls = [kl for _, kl in runs]
    tws = [R.trustworthiness(x, y) for y, _ in runs]
    print(f"KL: device {got[0]:.4f}, restatement {min(kls):.4f} .. {max(kls):.4f}; trustworthiness: device {got[1]:.4f}, "
          f"restatement {min(tws):.4f} .. {max(tws):.4f}")
    record("end_to_end_kl_device", got[0])
    record("end_to_end_kl_restatement_min", min(kls))
    record("end_to_end_kl_restatement_max", max(kls))
    record("end_to_end_trustworthiness_device", got[1])
    record("end_to_end_trustworthiness_restatement_min", min(tws))
    record("end_to_end_trustworthiness_restatement_max", max(tws))
    for v, runs_ in ((got[0], kls), (got[1], tws)):
        spread = max(runs_) - min(runs_)
        assert min(runs_) - spread <= v <= max(runs_) + spread
    pres = I.neighbour_preservation(dev(x), emb, 10)
    assert abs(pres - R.neighbour_preservation(x, emb.cpu().numpy(), 10)) <= 2.0 / 2400      # a float32 tie may swap a neighbour
    assert 0.2 < pres <= 1.0


def test_neighbour_preservation_equals_the_restatement_on_integers():
    from ssl_cr_histo_amd import inference as I
    rs = np.random.RandomState(11)
    x = rs.randint(-3, 4, (130, 8)).astype(np.float32)
    y = rs.randint(-6, 7, (130, 2)).astype(np.float32)
    assert I.neighbour_preservation(dev(x), dev(y), 7) == R.neighbour_preservation(x, y, 7)


# ------------------------------------------------------------------------------------------------ 7. host reads
def test_default_path_reads_once_and_early_stop_once_per_check():
    from ssl_cr_histo_amd import inference as I
    x, _ = R.four_clusters()
    y0 = dev(R.pca_init(R.center(x)).astype(np.float32))
    t = I.Tsne(max_iter=120, check_every=50, init=y0).fit(dev(x))
    assert t.reads == 1                              # the final copy of the log, nothing before it
    assert t.log.shape == (3, 4) and t.log[:, 3].tolist() == [49.0, 99.0, 120.0] and t.n_iter_ == 120
    assert t.kl_divergence_ == t.log[-1, 0] and np.isfinite(t.log).all()
    assert t.log[0, 0] > t.log[2, 0]                 # the exaggerated KL lies above the final one
    s = I.Tsne(max_iter=120, check_every=50, init=y0, early_stop=True).fit(dev(x))
    assert s.reads == 2 + 1                          # one per check, and the final copy
    assert np.array_equal(s.embedding_.cpu().numpy(), t.embedding_.cpu().numpy())         # no rule fired: the same launches, the same bits
    r = I.Tsne(max_iter=3, init="random", generator=torch.Generator(device=DEV).manual_seed(3)).fit(dev(x))
    assert r.reads == 1 and float(r.embedding_.abs().max()) < 1.0
