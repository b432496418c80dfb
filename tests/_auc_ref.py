"""NumPy restatements for the ranking metrics (csrc/rank.hip, inference.roc_auc / icc): the key map, the exact pair count U2 by a
stable argsort, run heads and integer cumulative sums, and the ICC mean squares written out literally.  Nothing here imports the
package under test."""
import numpy as np


def key_map(scores):
    """float32 scores -> uint32 keys whose unsigned order is the scores' order under float compares, -0 tied with +0"""
    b = np.ascontiguousarray(scores, dtype=np.float32).view(np.uint32).copy()
    b[(b << np.uint32(1)) == 0] = 0
    flip = np.where((b >> np.uint32(31)) != 0, np.uint32(0xFFFFFFFF), np.uint32(0x80000000))
    return b ^ flip


def is_nan_bits(scores):
    b = np.ascontiguousarray(scores, dtype=np.float32).view(np.uint32)
    return (b & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)


def counts_1d(scores, positive_flags, valid=None):
    """-> (U2, P, N, nan) as Python ints for one column: scores float32 [n], positive_flags bool [n], valid bool [n] or None.
    U2 = sum over valid non-NaN (positive i, negative j) of 2 [s_i > s_j] + [s_i == s_j]: the keys sorted by a stable argsort, the
    runs of equal keys from their heads, the negatives before each run and within it by integer cumsum."""
    s = np.ascontiguousarray(scores, dtype=np.float32).reshape(-1)
    pos = np.asarray(positive_flags, dtype=bool).reshape(-1)
    ok = np.ones(len(s), dtype=bool) if valid is None else np.asarray(valid).reshape(-1) != 0
    nanf = is_nan_bits(s) & ok
    ok = ok & ~nanf
    k, pos = key_map(s)[ok], pos[ok]
    order = np.argsort(k, kind="stable")
    k, pos = k[order], pos[order]
    neg = (~pos).astype(np.int64)
    P, N = int(pos.sum()), int(neg.sum())
    if len(k) == 0:
        return 0, 0, 0, int(nanf.sum())
    head = np.ones(len(k), dtype=bool)
    head[1:] = k[1:] != k[:-1]
    run = np.cumsum(head) - 1                                       # the run every element belongs to
    before = np.cumsum(neg) - neg                                   # negatives before the element
    run_before = before[head]                                       # ... before each run's head
    run_neg = np.add.reduceat(neg, np.flatnonzero(head))           # ... within each run
    u2 = int((2 * run_before[run[pos]] + run_neg[run[pos]]).sum())
    return u2, P, N, int(nanf.sum())


def counts(scores, target, positive=None, valid=None):
    """int64 [C, 4] for scores [n, C] (or [n]): column c against ``target == positive[c]`` (None: arange(C))"""
    s = np.asarray(scores, dtype=np.float32)
    s = s.reshape(len(s), -1)
    t = np.asarray(target).reshape(-1)
    positive = np.arange(s.shape[1]) if positive is None else np.asarray(positive).reshape(-1)
    return np.array([counts_1d(s[:, c], t == positive[c], valid) for c in range(s.shape[1])], dtype=np.int64)


def auc_from_counts(c, average="macro"):
    """float64: every column U2 / (2 P N) as a Python integer division; the vector (None), its mean, or its P-weighted average"""
    rows = np.asarray(c).reshape(-1, 4).tolist()
    a = np.array([int(u2) / (2 * int(p) * int(n)) for u2, p, n, _ in rows], dtype=np.float64)
    if average is None:
        return a
    if average == "macro":
        return float(np.mean(a))
    return float(np.average(a, weights=np.array([float(r[1]) for r in rows])))


def u2_brute(scores, positive_flags):
    """the definition itself, O(P N): for small inputs"""
    s = np.asarray(scores, dtype=np.float32).reshape(-1)
    pos = np.asarray(positive_flags, dtype=bool).reshape(-1)
    a, b = s[pos][:, None], s[~pos][None, :]
    return int(2 * (a > b).sum() + (a == b).sum())


def icc_literal(x):
    """the six Shrout-Fleiss forms with every sum written out as loops over the table; -> (values [6], mean squares dict)"""
    x = [[float(v) for v in row] for row in np.asarray(x, dtype=np.float64).tolist()]
    n, k = len(x), len(x[0])
    grand = sum(sum(row) for row in x) / (n * k)
    rmean = [sum(row) / k for row in x]
    cmean = [sum(x[i][j] for i in range(n)) / n for j in range(k)]
    ssr = k * sum((m - grand) ** 2 for m in rmean)
    ssc = n * sum((m - grand) ** 2 for m in cmean)
    ssw = sum((x[i][j] - rmean[i]) ** 2 for i in range(n) for j in range(k))
    sse = sum((x[i][j] - rmean[i] - cmean[j] + grand) ** 2 for i in range(n) for j in range(k))
    MSR, MSW, MSC, MSE = ssr / (n - 1), ssw / (n * (k - 1)), ssc / (k - 1), sse / ((n - 1) * (k - 1))
    values = [(MSR - MSW) / (MSR + (k - 1) * MSW), (MSR - MSE) / (MSR + (k - 1) * MSE + k * (MSC - MSE) / n),
              (MSR - MSE) / (MSR + (k - 1) * MSE), (MSR - MSW) / MSR, (MSR - MSE) / (MSR + (MSC - MSE) / n), (MSR - MSE) / MSR]
    return np.array(values, dtype=np.float64), dict(n=n, k=k, MSR=MSR, MSW=MSW, MSC=MSC, MSE=MSE)


# ---- shared inputs
def score_sets(n, seed):
    """name -> float32 [n]: random; four-valued; a plateau over 90 % of the elements; mixed +0 / -0 among a few values"""
    rs = np.random.RandomState(seed)
    plateau = rs.rand(n).astype(np.float32)
    plateau[rs.rand(n) < 0.9] = np.float32(1.0)
    zeros = rs.choice(np.array([0.0, -0.0, 0.25, -0.25], dtype=np.float32), n)
    return {"random": rs.rand(n).astype(np.float32), "four": rs.choice(np.array([0.1, 0.4, 0.4000001, 0.9], dtype=np.float32), n),
            "plateau": plateau, "zeros": zeros}
