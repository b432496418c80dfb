"""NumPy float64 restatement of the t-SNE embedding (csrc/tsne.hip, include/sslcr.h).  THIS FILE IS THE DEFINITION: tests/test_tsne_cpu.py
pins it against sklearn 1.7.2 (sklearn/manifold/_utils.pyx and _t_sne.py), tests/test_tsne_gpu.py holds the device to it.  Two
components, one degree of freedom, squared Euclidean distances, k <= 64 neighbours, an exact repulsive sum."""
import math

import numpy as np

import _knn_ref as KR

U = 2.0 ** -24                   # float32 unit roundoff
U64 = 2.0 ** -53
EPS = np.finfo(np.float64).eps   # sklearn's MACHINE_EPSILON
MAX_K = 64
EXAGGERATION, STOP_LYING = 12.0, 250


def gamma(k, u=U):
    """Higham's gamma_k = k u / (1 - k u): the relative error of k roundings compounded"""
    return k * u / (1.0 - k * u)


# ---------------------------------------------------------------------------------------------------------------- 1. neighbours
def neighbour_k(n, perplexity):
    k = min(n - 1, int(3.0 * perplexity + 1), MAX_K)
    if not perplexity < k:
        raise ValueError(f"perplexity = {perplexity} must be below k = {k}")
    return k


def center(x):
    """x minus the float32 rounding of its float64 column mean, one float32 subtraction per element"""
    x = np.asarray(x, np.float32)
    return (x - x.astype(np.float64).mean(0).astype(np.float32)[None, :]).astype(np.float32)


def augment(x):
    """-> (queries [x, 1, 0..], bank [x, -|x|^2 / 2, 0..]) float32, the width padded to a multiple of 4: maximising their dot
    product minimises the distance.  The norm is summed in float64 and rounded once."""
    x = np.asarray(x, np.float32)
    n, D = x.shape
    W = (D + 1 + 3) // 4 * 4
    q, b = np.zeros((n, W), np.float32), np.zeros((n, W), np.float32)
    q[:, :D] = x
    b[:, :D] = x
    q[:, D] = 1.0
    b[:, D] = (-0.5 * (x.astype(np.float64) ** 2).sum(1)).astype(np.float32)
    return q, b


def pair_dist2(x, idx):
    """float32 [n, k]: sum_d (x_id - x_jd)^2, float64, one rounding per square and per addition in rising d, rounded to float32 once;
    index -1 -> +inf"""
    x64 = np.asarray(x, np.float32).astype(np.float64)
    idx = np.asarray(idx)
    s = np.zeros(idx.shape, np.float64)
    j = np.maximum(idx, 0)
    for d in range(x64.shape[1]):
        t = x64[:, d, None] - x64[j, d]
        s = s + t * t
    s[idx < 0] = np.inf
    return s.astype(np.float32)


def euclidean_topk(x, k):
    """-> (indices int32 [n, k], dist2 float32 [n, k]): the neighbour set is knn_topk's on the augmented rows, in its total order (the
    fp32 fma chain, then the lower index); the distances are recomputed directly"""
    q, b = augment(x)
    _, idx = KR.topk(KR.fma_chain(q, b), k, self_offset=0)
    return idx, pair_dist2(x, idx)


def dist2_f64(x):
    x = np.asarray(x, np.float64)
    return ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1)


def topk_slack(x):
    """per row: by how much the float64 distance of a returned neighbour may exceed the k-th true one.  A score is an fma chain of
    W <= D + 1 terms and the norm's own rounding: |error| <= gamma_{D + 2} (|x_i| |x_j| + |x_j|^2 / 2) (Cauchy-Schwarz).  A returned j
    beat a true neighbour j* in computed score, so d2(j) - d2(j*) <= 2 (E_j + E_j*) <= 4 E_max."""
    x64 = np.asarray(x, np.float32).astype(np.float64)
    nrm = np.sqrt((x64 ** 2).sum(1))
    E = gamma(x64.shape[1] + 2) * (nrm * nrm.max() + 0.5 * nrm.max() ** 2)
    return 4.0 * E


# ---------------------------------------------------------------------------------------------------------------- 2. conditional affinities
def binary_search_perplexity(d32, perplexity, exp=np.exp):
    """sklearn/manifold/_utils.pyx, _binary_search_perplexity, statement by statement (rows in parallel, sums sequential in j):
    -> (P float32 [n, k], beta float64 [n], steps [n])"""
    d = np.asarray(d32, np.float32).astype(np.float64)
    n, k = d.shape
    desired = math.log(perplexity)
    beta, lo, hi = np.ones(n), np.full(n, -np.inf), np.full(n, np.inf)
    P = np.zeros((n, k))
    steps = np.zeros(n, np.int64)
    live = np.arange(n)
    for _ in range(100):
        if live.size == 0:
            break
        dl, bl = d[live], beta[live]
        with np.errstate(all="ignore"):
            e = exp(-dl * bl[:, None])
        s = np.zeros(live.size)
        for j in range(k):
            s = s + e[:, j]
        s[s == 0.0] = 1e-8
        p = e / s[:, None]
        sdp = np.zeros(live.size)
        for j in range(k):
            sdp = sdp + dl[:, j] * p[:, j]
        P[live] = p
        steps[live] += 1
        diff = np.log(s) + bl * sdp - desired
        done = np.abs(diff) <= 1e-5
        up = diff > 0.0
        with np.errstate(all="ignore"):
            nb_up = np.where(hi[live] == np.inf, bl * 2.0, (bl + hi[live]) / 2.0)
            nb_dn = np.where(lo[live] == -np.inf, bl / 2.0, (bl + lo[live]) / 2.0)
        go = ~done
        lo[live[go & up]] = bl[go & up]
        hi[live[go & ~up]] = bl[go & ~up]
        beta[live[go]] = np.where(up, nb_up, nb_dn)[go]
        live = live[go]
    steps[live] = 101                                # never met the tolerance
    return P.astype(np.float32), beta, steps


def affinities_at(d32, beta):
    """the float64 formula at a given beta: -> (P [n, k], H [n])"""
    d = np.asarray(d32, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        e = np.exp(-d * beta[:, None])
    s = e.sum(1)
    s[s == 0.0] = 1e-8
    P = e / s[:, None]
    return P, np.log(s) + beta * (d * P).sum(1)


# ---------------------------------------------------------------------------------------------------------------- 3. joint affinities
def joint_csr(idx, P32):
    """p_ij = (p_j|i + p_i|j) / (2 n) as CSR (rowptr int32 [n + 1], col int32, val float32), columns rising within a row: the 2 n k
    directed entries sorted by (row, column), adjacent equal pairs summed (at most two meet: the float64 sum is exact), one float64
    division by 2 n, rounded to float32"""
    idx, P32 = np.asarray(idx), np.asarray(P32, np.float32)
    n, k = idx.shape
    i = np.repeat(np.arange(n), k)
    j = idx.reshape(-1).astype(np.int64)
    v = P32.reshape(-1).astype(np.float64)
    ok = j >= 0
    i, j, v = i[ok], j[ok], v[ok]
    r, c, v = np.concatenate([i, j]), np.concatenate([j, i]), np.concatenate([v, v])
    key = r * n + c
    o = np.argsort(key, kind="stable")
    key, v = key[o], v[o]
    first = np.concatenate([[True], key[1:] != key[:-1]])
    seg = np.cumsum(first) - 1
    val = np.zeros(int(first.sum()))
    np.add.at(val, seg, v)
    ukey = key[first]
    rows, col = ukey // n, ukey % n
    rowptr = np.zeros(n + 1, np.int32)
    rowptr[1:] = np.cumsum(np.bincount(rows, minlength=n))
    return rowptr, col.astype(np.int32), (val / (2.0 * n)).astype(np.float32)


def densify(rowptr, col, val):
    n = len(rowptr) - 1
    P = np.zeros((n, n))
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    P[rows, col[:rowptr[-1]]] = np.asarray(val, np.float64)[:rowptr[-1]]
    return P


# ---------------------------------------------------------------------------------------------------------------- 4. gradient
def field(y, P):
    """the exaggeration-free pieces of the gradient of a dense float64 P (zeros where the CSR has no entry) at y, float64: the
    attractive and repulsive sums, their sums of magnitudes (for the bounds), Z, KL and the longest row"""
    y = np.asarray(y, np.float64)
    n = y.shape[0]
    with np.errstate(all="ignore"):
        d = [y[:, c, None] - y[None, :, c] for c in range(2)]
        q = 1.0 / (1.0 + (d[0] * d[0] + d[1] * d[1]))
        q[np.arange(n), np.arange(n)] = 0.0          # the self pair, by index: coincident points keep q = 1
        Z = q.sum()
        pq, qq = P * q, q * q
        out = dict(n=n, Z=Z, attr=np.stack([(pq * c).sum(1) for c in d], 1), rep=np.stack([(qq * c).sum(1) for c in d], 1),
                   attr_abs=np.stack([(pq * np.abs(c)).sum(1) for c in d], 1), rep_abs=np.stack([(qq * np.abs(c)).sum(1) for c in d], 1))
        nz = P > 0
        out["kl"] = float((P[nz] * np.log(P[nz] / np.maximum(q[nz] / Z, EPS))).sum())
        out["entries"] = int(nz.sum(1).max())
    return out


def gradient(y, P, exaggeration=1.0, plan=None, pieces=None):
    """sklearn/manifold/_t_sne.py, _kl_divergence, on a dense float64 P: -> dict with ``grad`` [n, 2], ``Z``, ``kl`` and, with ``plan``
    (``kernels.tsne_plan``'s dict), the device's per-element bounds ``grad_bound``, ``Z_bound`` and ``raw_bound`` (the gradient before
    its float32 rounding, what the update consumes), and ``f64_bound``, float64's own.  pieces: ``field(y, P)`` where it is at hand.

    The bounds, from the operation count of tsne_repulsion_kernel (u = 2^-24): dx, dy: one rounding each; d2 = fma(dy, dy, dx dx):
    relative 4 u; 1 + d2: 5 u; v_rcp_f32 is accurate to 1 ulp = 2 u: q to 7 u; q q: 15 u; its product with dx inside the fma: 16 u.
    A lane adds at most m = min(n, chunks_per_slice * chunk) terms in sequence: gamma_m of the sum of their magnitudes.  So
    |rep error| <= gamma_{m + 20} sum_j q^2 |d| and |Z error| <= (gamma_{m + 8} + (n S + 1024) 2^-53) Z, the slices' float64 fold
    included.  The attractive sum is float64: (entries + 16) 2^-53 of its magnitudes.  grad = 4 (e attr - rep / Z) adds rep's
    error over Z, |rep| / Z times Z's relative error, and one float32 rounding."""
    f = pieces or field(y, P)
    n, Z, attr, rep, attr_abs, rep_abs = f["n"], f["Z"], f["attr"], f["rep"], f["attr_abs"], f["rep_abs"]
    grad = 4.0 * (exaggeration * attr - rep / Z)
    out = dict(grad=grad, Z=Z, kl=f["kl"])
    if plan is not None:
        m = min(n, plan["chunks_per_slice"] * plan["chunk"])
        S = plan["slices"]
        z_rel = gamma(m + 8) + (n * S + 1024) * U64
        rep_err = gamma(m + 20) * rep_abs + m * 2.0 ** -149
        raw = 4.0 * ((rep_err + np.abs(rep) * z_rel) / (Z * (1.0 - z_rel)) + exaggeration * (f["entries"] + 16) * U64 * attr_abs) + 8 * U64 * np.abs(grad)
        out.update(Z_bound=z_rel * Z, raw_bound=raw, f64_bound=4.0 * (n + 16) * U64 * (exaggeration * attr_abs + rep_abs / Z),
                   grad_bound=raw + U * (np.abs(grad) + raw) + 2.0 ** -149)
    return out


# ---------------------------------------------------------------------------------------------------------------- 5. update
def update_step(y, update, gains, grad, momentum, lr, min_gain=0.01, f32=False):
    """sklearn/manifold/_t_sne.py, _gradient_descent, one iteration; f32: every stored value rounded to float32 once"""
    inc = update * grad < 0.0
    gains = np.maximum(np.where(inc, gains + 0.2, gains * 0.8), min_gain)
    if f32:
        gains = gains.astype(np.float32).astype(np.float64)
    update = momentum * update - lr * gains * grad
    if f32:
        update = update.astype(np.float32).astype(np.float64)
    y = y + update
    if f32:
        y = y.astype(np.float32).astype(np.float64)
    return y, update, gains


def schedule(it, early_exaggeration=EXAGGERATION):
    """(exaggeration, momentum) of iteration ``it``"""
    return (early_exaggeration, 0.5) if it < STOP_LYING else (1.0, 0.8)


def learning_rate(n, early_exaggeration=EXAGGERATION):
    return max(n / early_exaggeration / 4.0, 50.0)


def pca_init(x):
    """the two leading principal axes of the centred features (float64 covariance, eigh), each signed so that its largest-magnitude
    loading is positive, scaled to std(y[:, 0]) = 1e-4"""
    x = np.asarray(x, np.float64)
    x = x - x.mean(0)
    w, v = np.linalg.eigh(x.T @ x / (x.shape[0] - 1))
    v = v[:, ::-1][:, :2]
    v = v * np.sign(v[np.abs(v).argmax(0), np.arange(2)])[None, :]
    y = x @ v
    return y / y[:, 0].std() * 1e-4


def affinities(x, perplexity):
    """items 1 - 3 on features x: -> (rowptr, col, val)"""
    xc = center(x)
    k = neighbour_k(xc.shape[0], perplexity)
    idx, d2 = euclidean_topk(xc, k)
    P, _, _ = binary_search_perplexity(d2, perplexity)
    return joint_csr(idx, P)


def fit(P, y0, n_iter=1000, early_exaggeration=EXAGGERATION, lr=None, f32=False, start=0):
    """-> (y, kl): ``n_iter`` iterations from y0 on a dense P, then the KL at the final y"""
    n = P.shape[0]
    lr = learning_rate(n, early_exaggeration) if lr is None else lr
    y = np.asarray(y0, np.float64).copy()
    if f32:
        y = y.astype(np.float32).astype(np.float64)
    update, gains = np.zeros_like(y), np.ones_like(y)
    for it in range(start, start + n_iter):
        e, mom = schedule(it, early_exaggeration)
        g = gradient(y, P, e)["grad"]
        y, update, gains = update_step(y, update, gains, g, mom, lr, f32=f32)
    return y, gradient(y, P, 1.0)["kl"]


# ---------------------------------------------------------------------------------------------------------------- quality
def trustworthiness(x, y, k=5):
    """sklearn.manifold.trustworthiness (Euclidean) in NumPy"""
    n = len(x)
    dx = dist2_f64(x)
    np.fill_diagonal(dx, np.inf)
    ind_x = np.argsort(dx, axis=1, kind="stable")
    dy = dist2_f64(y)
    np.fill_diagonal(dy, np.inf)
    ind_y = np.argsort(dy, axis=1, kind="stable")[:, :k]
    inv = np.zeros((n, n), np.int64)
    inv[np.arange(n)[:, None], ind_x] = np.arange(1, n + 1)[None, :]
    ranks = inv[np.arange(n)[:, None], ind_y] - k
    t = float(ranks[ranks > 0].sum())
    return 1.0 - t * (2.0 / (n * k * (2.0 * n - 3.0 * k - 1.0)))


def neighbour_preservation(x, y, k):
    ix, _ = euclidean_topk(x, k)
    iy, _ = euclidean_topk(y, k)
    return sum(len(set(a[a >= 0]) & set(b[b >= 0])) for a, b in zip(ix, iy)) / (len(ix) * k)


def four_clusters(seed=0, n=240, D=32, scale=5.0):
    """the quality set: n points, four Gaussian clusters in D dimensions, centres scaled by ``scale``"""
    rs = np.random.RandomState(seed)
    labels = np.arange(n) % 4
    centres = rs.randn(4, D) * scale
    return (centres[labels] + rs.randn(n, D)).astype(np.float32), labels
