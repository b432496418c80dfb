"""NumPy restatement of the k-NN feature probe (csrc/knn.hip, include/sslcr.h): similarities in float64, the total order as integer
keys, the votes and the row normalisation.  Shared by tests/test_knn_cpu.py (against sklearn) and tests/test_knn_gpu.py (against
the device)."""
import numpy as np

NAN_KEY = 1                      # the score key of a NaN: below that of -inf (0x007FFFFF), above the empty slot (0)


def similarity(q, b):
    """[nq, nb] dot products in float64"""
    with np.errstate(all="ignore"):
        return np.asarray(q, np.float64) @ np.asarray(b, np.float64).T


def score_keys(s32):
    """the order-preserving uint32 key of float32 scores, as sslcr_rank_keys defines it (-0 tied to +0), NaN -> NAN_KEY"""
    b = np.ascontiguousarray(s32, dtype=np.float32).view(np.uint32).copy()
    nan = (b & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    b[(b << np.uint32(1)) == 0] = 0
    key = np.where(b >> np.uint32(31) != 0, ~b, b ^ np.uint32(0x80000000)).astype(np.uint32)
    key[nan] = NAN_KEY
    return key


def admissible(nq, nb, nb_valid=None, self_offset=None):
    ok = np.ones((nq, nb), bool)
    if nb_valid is not None:
        ok[:, nb_valid:] = False
    if self_offset is not None:
        i = np.arange(nq)
        j = i + self_offset
        ok[i[j < nb], j[j < nb]] = False
    return ok


def topk(s, k, nb_valid=None, self_offset=None):
    """-> (scores float32 [nq, k], indices int32 [nq, k]) of a similarity matrix whose values are float32-representable (cast exactly):
    descending by the 64-bit key (score key << 32) | ~index -- the greater score, then the LOWER index; NaN below every number;
    inadmissible rows have key 0; missing neighbours are index -1, score -inf."""
    with np.errstate(all="ignore"):
        s32 = np.asarray(s).astype(np.float32)
    nq, nb = s32.shape
    j = np.arange(nb, dtype=np.uint64)
    key = (score_keys(s32).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - j)[None, :]
    key[~admissible(nq, nb, nb_valid, self_offset)] = 0
    order = np.argsort(key, axis=1, kind="stable")[:, ::-1][:, :k]          # keys are distinct except the 0s
    got = np.take_along_axis(key, order, 1)
    scores = np.take_along_axis(s32, order, 1)
    scores[np.isnan(scores)] = np.float32(np.nan)
    idx = order.astype(np.int32)
    idx[got == 0] = -1
    scores[got == 0] = -np.inf
    scores[scores == 0] = 0.0                                               # -0 comes back as +0
    if k > nb:
        scores = np.concatenate([scores, np.full((nq, k - nb), -np.inf, np.float32)], 1)
        idx = np.concatenate([idx, np.full((nq, k - nb), -1, np.int32)], 1)
    return scores, idx


def topk_f64(s64, k, nb_valid=None, self_offset=None):
    """the same order on float64 similarities (finite): -> (scores float64 [nq, k'], indices [nq, k']), k' = min(k, admissible)"""
    nq, nb = s64.shape
    ok = admissible(nq, nb, nb_valid, self_offset)
    out_s, out_i = [], []
    for i in range(nq):
        j = np.flatnonzero(ok[i])
        o = np.lexsort((j, -s64[i, j]))[:k]
        out_s.append(s64[i, j[o]])
        out_i.append(j[o])
    return out_s, out_i


def l2_normalize(x, eps=1e-12):
    """x / max(||x||, eps): the squares summed in float64, the root in float64 rounded to float32 once, one float32 division"""
    x = np.asarray(x, np.float32)
    n64 = np.sqrt((x.astype(np.float64) ** 2).sum(1))
    den = np.maximum(n64.astype(np.float32), np.float32(eps))
    return (x / den[:, None]).astype(np.float32)


def norm_clearance(x):
    """per row: the distance of the float64 norm from the nearest float32 rounding boundary (the midpoint of two neighbouring
    float32 values), relative to the norm"""
    n64 = np.sqrt((np.asarray(x, np.float32).astype(np.float64) ** 2).sum(1))
    f = n64.astype(np.float32)
    up = np.nextafter(f, np.float32(np.inf)).astype(np.float64)
    dn = np.nextafter(f, np.float32(-np.inf)).astype(np.float64)
    f = f.astype(np.float64)
    return np.minimum(np.abs(n64 - (f + up) / 2), np.abs(n64 - (f + dn) / 2)) / n64


def vote_uniform(indices, labels, C):
    """-> (pred, counts [nq, C]): the most votes, a tie to the lowest class"""
    indices, labels = np.asarray(indices), np.asarray(labels)
    counts = np.zeros((indices.shape[0], C), np.int64)
    for r in range(indices.shape[1]):
        j = indices[:, r]
        rows = np.flatnonzero(j >= 0)
        np.add.at(counts, (rows, labels[j[rows]]), 1)
    return counts.argmax(1), counts


def vote_softmax(indices, scores, labels, C, temperature):
    """-> (pred, votes float64 [nq, C]): weights exp((s - s_0) / T) in float64"""
    indices, labels = np.asarray(indices), np.asarray(labels)
    s = np.asarray(scores, np.float64)
    votes = np.zeros((indices.shape[0], C), np.float64)
    for r in range(indices.shape[1]):
        j = indices[:, r]
        rows = np.flatnonzero(j >= 0)
        np.add.at(votes, (rows, labels[j[rows]]), np.exp((s[rows, r] - s[rows, 0]) / temperature))
    return votes.argmax(1), votes


def vote_regress(indices, targets):
    """-> the float64 mean of the neighbours' targets"""
    indices = np.asarray(indices)
    t = np.asarray(targets, np.float64)
    ok = indices >= 0
    with np.errstate(all="ignore"):
        return np.where(ok, t[np.maximum(indices, 0)], 0.0).sum(1) / ok.sum(1)


def confusion(query_labels, pred, C):
    cm = np.zeros((C, C), np.int64)
    np.add.at(cm, (np.asarray(query_labels), np.asarray(pred)), 1)
    return cm


def fma_chain(q, b):
    """[nq, nb] float32 similarities as the device forms them: acc = fmaf(q_d, b_d, acc) over d in RISING order from +0.  The product
    of two float32 values is exact in float64; its sum with the accumulator is rounded to 53 bits and then to 24, which differs from
    the single rounding of fmaf only where the 53-bit sum lands on a float32 tie (about 2^-29 of the steps)."""
    q, b = np.asarray(q, np.float32), np.asarray(b, np.float32)
    acc = np.zeros((q.shape[0], b.shape[0]), np.float32)
    with np.errstate(all="ignore"):
        for d in range(q.shape[1]):
            acc = (q[:, d, None].astype(np.float64) * b[None, :, d].astype(np.float64) + acc.astype(np.float64)).astype(np.float32)
    return acc
