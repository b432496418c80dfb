"""NumPy restatements of the lesion-scoring definitions of include/sslcr.h (the Camelyon16 lesion-level FROC chain): the component
labeller, the float32 smoothing chain, the sequential NMS loop and its round-based form, the hit test, and a literal transcription
of the FROC arithmetic.  Test infrastructure: nothing here imports the package."""
import numpy as np

_NEIGHBOURS = {1: ((-1, 0), (0, -1), (0, 1), (1, 0)),
               2: ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))}


def label(mask, connectivity=2):
    """flood fill, components numbered 1..L by the order (linear index) of each component's first cell -> (labels int32, L)"""
    mask = np.asarray(mask) != 0
    X, Y = mask.shape
    W = Y + 2                                                      # a padded frame: no bounds tests in the inner loop
    pad = np.zeros((X + 2, W), dtype=bool)
    pad[1:-1, 1:-1] = mask
    todo = pad.ravel().tolist()
    out = [0] * len(todo)
    steps = [dx * W + dy for dx, dy in _NEIGHBOURS[connectivity]]
    count = 0
    for start in np.flatnonzero(pad.ravel()).tolist():             # increasing padded index = increasing linear index
        if not todo[start]:
            continue
        count += 1
        todo[start] = False
        out[start] = count
        stack = [start]
        while stack:
            c = stack.pop()
            for s in steps:
                q = c + s
                if todo[q]:
                    todo[q] = False
                    out[q] = count
                    stack.append(q)
    return np.asarray(out, dtype=np.int32).reshape(X + 2, W)[1:-1, 1:-1].copy(), count


def gaussian_weights(sigma):
    R = int(4.0 * sigma + 0.5)
    k = np.arange(-R, R + 1, dtype=np.float64)
    w = np.exp(-(k * k) / (2.0 * sigma * sigma))
    return (w / w.sum()).astype(np.float32)


def smooth_pass(a, w, axis):
    """one pass in float32: acc = 0; per tap, from -R to +R, acc = acc + w * a[clamped], a float32 product then a float32 sum"""
    a = np.asarray(a, dtype=np.float32)
    R = (len(w) - 1) // 2
    n = a.shape[axis]
    acc = np.zeros(a.shape, dtype=np.float32)
    for k in range(-R, R + 1):
        idx = np.clip(np.arange(n) + k, 0, n - 1)
        prod = (np.float32(w[k + R]) * np.take(a, idx, axis=axis)).astype(np.float32)
        acc = (acc + prod).astype(np.float32)
    return acc


def smooth(a, sigma):
    """axis 0 first, then axis 1; sigma == 0 returns the map as given"""
    if sigma == 0:
        return np.asarray(a, dtype=np.float32)
    w = gaussian_weights(sigma)
    return smooth_pass(smooth_pass(a, w, 0), w, 1)


def nms(a, threshold, r):
    """the sequential loop: take the first maximum in order, record it, remove its window [x - r, x + r) x [y - r, y + r), repeat while
    max > threshold -> [(x, y, prob)].  (A removed cell and a NaN can never be a maximum again: both become -inf.)"""
    a = np.asarray(a, dtype=np.float32)
    thr = np.float32(threshold)
    with np.errstate(invalid="ignore"):
        work = np.where(a > thr, a, -np.inf).astype(np.float32)
    out = []
    while True:
        i = int(np.argmax(work))                                   # the first maximum in linear order
        x, y = divmod(i, a.shape[1])
        if not work[x, y] > thr:
            return out
        out.append((x, y, float(work[x, y])))
        work[max(x - r, 0):x + r, max(y - r, 0):y + r] = -np.inf


def nms_rounds(a, threshold, r):
    """the round-based form of the definition: per round, from the states at the round's start, a candidate becomes suppressed once a
    selected predecessor's window holds it, selected once every predecessor whose window holds it is decided non-selected
    -> ([(x, y, prob)] in "precedes" order, rounds)"""
    a = np.asarray(a, dtype=np.float32)
    X, Y = a.shape
    with np.errstate(invalid="ignore"):
        cand = [(int(x), int(y)) for x, y in zip(*np.nonzero(a > np.float32(threshold)))]
    state = {p: 1 for p in cand}                                   # 1 undecided, 2 selected, 3 suppressed

    def precedes(q, p):
        return a[q] > a[p] or (a[q] == a[p] and q[0] * Y + q[1] < p[0] * Y + p[1])
    rounds = 0
    while any(s == 1 for s in state.values()):
        rounds += 1
        assert rounds <= len(cand) + 1
        new = dict(state)
        for p in cand:
            if state[p] != 1:
                continue
            waits = suppressed = False
            for qx in range(max(p[0] - r + 1, 0), min(p[0] + r, X - 1) + 1):
                for qy in range(max(p[1] - r + 1, 0), min(p[1] + r, Y - 1) + 1):
                    q = (qx, qy)
                    if q == p or q not in state or not precedes(q, p):
                        continue
                    suppressed |= state[q] == 2
                    waits |= state[q] == 1
            new[p] = 3 if suppressed else 1 if waits else 2
        state = new
    sel = [p for p in cand if state[p] == 2]
    sel.sort(key=lambda p: (-a[p], p[0] * Y + p[1]))
    return [(x, y, float(a[x, y])) for x, y in sel], rounds


def hits(labels, n_lesions, detections, ignore=()):
    """-> (hit int32 [K], tp_prob float32 [L], fp_prob list): hit = the label under each detection; a hit on an ignored label counts
    nowhere; otherwise the lesion keeps its best probability; a lesion nothing hits keeps 0"""
    hit = np.zeros(len(detections), dtype=np.int32)
    tp = np.zeros(n_lesions, dtype=np.float32)
    fp = []
    for k, (x, y, p) in enumerate(detections):
        hit[k] = labels[x, y]
        if hit[k] == 0:
            fp.append(p)
        elif hit[k] not in ignore:
            tp[hit[k] - 1] = max(tp[hit[k] - 1], np.float32(p))
    return hit, tp, fp


def froc(fp_probs, tp_probs, n_slides, n_lesions, fps=(0.25, 0.5, 1, 2, 4, 8)):
    """a literal transcription: all = sorted(set(FP | TP)); for t in all[1:] record (#FP >= t, #TP >= t); append (0, 0);
    avg_fp = FPs / n_slides; sens = TPs / n_lesions (0 on a division by zero); score = mean(interp(fps, avg_fp[::-1], sens[::-1]))"""
    fp_probs = [float(v) for v in fp_probs]
    tp_probs = [float(v) for v in tp_probs]
    every = sorted(set(fp_probs) | set(tp_probs))
    fps_at, tps_at = [], []
    for t in every[1:]:
        fps_at.append(sum(1 for v in fp_probs if v >= t))
        tps_at.append(sum(1 for v in tp_probs if v >= t))
    fps_at.append(0)
    tps_at.append(0)
    avg_fp = np.asarray([v / float(n_slides) if n_slides else 0.0 for v in fps_at], dtype=np.float64)
    sens = np.asarray([v / float(n_lesions) if n_lesions else 0.0 for v in tps_at], dtype=np.float64)
    score = float(np.mean(np.interp(np.asarray(fps, dtype=np.float64), avg_fp[::-1], sens[::-1])))
    return avg_fp, sens, score


# ---------------------------------------------------------------------------------------------------------------- mask patterns
def spiral(X, Y):
    """a one-cell-wide path that spirals inwards from (0, 0) with one-cell gaps between its turns: ONE component at either
    connectivity, and the longest chain a shape holds"""
    m = np.zeros((X, Y), dtype=np.uint8)
    x, y, dx, dy = 0, 0, 0, 1
    m[0, 0] = 1

    def free(u, v):
        return not (0 <= u < X and 0 <= v < Y) or not m[u, v]
    while True:
        moved = False
        while 0 <= x + dx < X and 0 <= y + dy < Y and not m[x + dx, y + dy] and free(x + 2 * dx, y + 2 * dy):
            x, y = x + dx, y + dy
            m[x, y] = 1
            moved = True
        if not moved:
            return m
        dx, dy = dy, -dx                                           # right -> down -> left -> up


def checkerboard(X, Y):
    return ((np.add.outer(np.arange(X), np.arange(Y)) & 1) == 0).astype(np.uint8)


def comb(X, Y):
    """teeth in every other column that join in the LAST row only: the arms merge late"""
    m = np.zeros((X, Y), dtype=np.uint8)
    m[:, ::2] = 1
    m[-1, :] = 1
    return m


def u_shape(X, Y):
    m = np.zeros((X, Y), dtype=np.uint8)
    m[:, 0] = 1
    m[:, -1] = 1
    m[-1, :] = 1
    return m


def corner_blobs(X, Y, cx=16, cy=64):
    """two blobs that touch only diagonally across the tile corner at (cx, cy), and two more across it the other way round, kept
    apart from the first pair: one component each pair at connectivity 2, four components at connectivity 1"""
    m = np.zeros((X, Y), dtype=np.uint8)
    if X > cx and Y > cy:
        m[max(cx - 3, 0):cx, max(cy - 3, 0):cy] = 1                # ends in (cx - 1, cy - 1)
        m[cx:cx + 3, cy:cy + 3] = 1                                # starts in (cx, cy)
    if X > 2 * cx and Y > cy:
        m[2 * cx - 3:2 * cx, cy:cy + 3] = 1                        # ends in (2 cx - 1, cy)
        m[2 * cx:2 * cx + 3, max(cy - 3, 0):cy] = 1                # starts in (2 cx, cy - 1)
    return m
