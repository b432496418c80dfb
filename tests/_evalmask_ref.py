"""NumPy restatements of the evaluation-mask definitions of include/sslcr.h: the exact squared distance transform (separable and brute
force), hole filling, the components' raw moments, a literal float64 transcription of the central-moment chain behind
``regionprops.major_axis_length``, the same quantity in exact rationals, and the challenge's steps chained on the host.  The masks the
tests share are made here too.  Test infrastructure: nothing here imports the package."""
import json
import os
from decimal import Decimal, getcontext
from fractions import Fraction

import numpy as np

import _froc_ref as FR

INT32_MAX = (1 << 31) - 1
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "annotation_small.json")
CELL_UM = 0.243 * 64                                               # microns per cell of a resolution-64 truth mask at level 0


# ---------------------------------------------------------------------------------------------------------------- distance transform
def d2_brute(mask, limit=None, invert=False):
    """by the definition: every cell against every zero cell, int64"""
    zero = (np.asarray(mask) != 0) if invert else (np.asarray(mask) == 0)
    limit = INT32_MAX if limit is None else int(limit)
    X, Y = zero.shape
    zx, zy = np.nonzero(zero)
    out = np.full((X, Y), limit, dtype=np.int64)
    if len(zx):
        xs, ys = np.arange(X, dtype=np.int64), np.arange(Y, dtype=np.int64)
        for x in range(X):
            d = (zx[:, None] - xs[x]) ** 2 + (zy[:, None] - ys[None, :]) ** 2
            out[x] = np.minimum(d.min(0), limit)
    return out.astype(np.int32)


def d2(mask, limit=None, invert=False):
    """min(limit, the exact squared distance to the nearest zero cell), int32; `limit` everywhere when there is no zero cell.  The
    separable form in int64: g = the distance to the nearest zero within the row, then min over x' of g(x', y)^2 + (x - x')^2."""
    zero = (np.asarray(mask) != 0) if invert else (np.asarray(mask) == 0)
    limit = INT32_MAX if limit is None else int(limit)
    X, Y = zero.shape
    far = np.int64(1) << 40
    ys = np.arange(Y, dtype=np.int64)
    last = np.maximum.accumulate(np.where(zero, ys[None, :], -far), axis=1)                 # the last zero at or before y
    first = np.minimum.accumulate(np.where(zero, ys[None, :], far)[:, ::-1], axis=1)[:, ::-1]
    g = np.minimum(ys[None, :] - last, first - ys[None, :])
    g2 = np.where(g >= far // 2, far, g * g)
    xs = np.arange(X, dtype=np.int64)
    out = np.empty((X, Y), dtype=np.int64)
    for x in range(X):
        out[x] = (g2 + ((xs - x) ** 2)[:, None]).min(0)
    return np.minimum(out, limit).astype(np.int32)


# ---------------------------------------------------------------------------------------------------------------- hole filling
def fill(mask):
    """mask != 0, or a background cell whose connectivity-1 background component holds no cell of the array's border -> uint8 0 / 1"""
    b = np.asarray(mask) != 0
    labels, n = FR.label(~b, 1)
    border = np.zeros(n + 1, dtype=bool)
    for edge in (labels[0, :], labels[-1, :], labels[:, 0], labels[:, -1]):
        border[edge] = True
    border[0] = True                                               # label 0 = the set cells: not a hole
    return (b | ~border[labels]).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------- moments
def moments(labels, n):
    """int64 [n, 6] per label l + 1: area, sum x, sum y, sum x^2, sum y^2, sum x y (Python-int sums: no overflow to think about)"""
    labels = np.asarray(labels)
    out = np.zeros((n, 6), dtype=np.int64)
    xs, ys = np.nonzero((labels >= 1) & (labels <= n))
    for x, y, l in zip(xs.tolist(), ys.tolist(), labels[xs, ys].tolist()):
        out[l - 1] += (1, x, y, x * x, y * y, x * y)
    return out


def major_axis_central(xs, ys):
    """a literal float64 transcription of the chain regionprops runs: moments_central about the centroid, divided by the area, the
    inertia tensor's larger eigenvalue, 4 sqrt of it"""
    xs, ys = np.asarray(xs, dtype=np.float64), np.asarray(ys, dtype=np.float64)
    area = float(len(xs))
    cx, cy = xs.sum() / area, ys.sum() / area
    mu20, mu02, mu11 = ((xs - cx) ** 2).sum() / area, ((ys - cy) ** 2).sum() / area, ((xs - cx) * (ys - cy)).sum() / area
    l1 = (mu20 + mu02) / 2.0 + np.sqrt(((mu20 - mu02) / 2.0) ** 2 + mu11 ** 2)
    return 4.0 * np.sqrt(max(l1, 0.0))


def major_axes_central(labels, n):
    labels = np.asarray(labels)
    return np.asarray([major_axis_central(*np.nonzero(labels == l)) for l in range(1, n + 1)], dtype=np.float64).reshape(n)


def major_axis_exact(row, digits=60):
    """the same quantity from raw moments in exact rationals, the two square roots in `digits`-digit decimals -> Decimal"""
    getcontext().prec = digits
    A, sx, sy, sxx, syy, sxy = (int(v) for v in row)
    a, c, b = Fraction(A * sxx - sx * sx, A * A), Fraction(A * syy - sy * sy, A * A), Fraction(A * sxy - sx * sy, A * A)

    def dec(f):
        return Decimal(f.numerator) / Decimal(f.denominator)
    root = dec(((a - c) / 2) ** 2 + b * b).sqrt()
    return 4 * (dec((a + c) / 2) + root).sqrt()


# ---------------------------------------------------------------------------------------------------------------- the chain
def limit_of(T):
    """the smallest k >= 0 with sqrt(float64(k)) >= T, by counting up"""
    k = 0
    while np.sqrt(np.float64(k)) < T:
        k += 1
    return k


def evaluation(truth, cell_um, dilate_um=75.0, itc_um=275.0, connectivity=2):
    """the restatements chained: d2 to the nearest truth cell, d2 < limit, fill, label, moments, the float64 central-moment axis
    lengths -> dict like inference.evaluation_mask's, all on the host"""
    limit = limit_of(dilate_um / (cell_um * 2.0))
    binary = d2(truth, limit, invert=True) < limit
    mask = fill(binary)
    labels, n = FR.label(mask, connectivity)
    major = major_axes_central(labels, n)
    itc = np.flatnonzero(major < itc_um / cell_um).astype(np.int64) + 1
    return dict(mask=mask, labels=labels, n_lesions=n, moments=moments(labels, n), major_axis=major, itc=itc, limit=limit)


def band_is_empty(major, threshold, rel=1e-9):
    """the ITC decision is a float comparison: no component may sit within rel * threshold of it"""
    return bool(np.all(np.abs(np.asarray(major) - threshold) > rel * threshold))


# ---------------------------------------------------------------------------------------------------------------- masks
def ring(X, Y, x0, y0, side, leak=None):
    """a one-cell-wide square ring; leak = "diagonal": the ring's corner is cut, so the hole meets the outside diagonally only"""
    m = np.zeros((X, Y), np.uint8)
    m[x0:x0 + side, y0:y0 + side] = 1
    m[x0 + 1:x0 + side - 1, y0 + 1:y0 + side - 1] = 0
    if leak == "diagonal":
        m[x0, y0] = 0                                              # hole cell (x0 + 1, y0 + 1) now touches the outside at a corner only
    return m


def hole_patterns(X, Y):
    """(name, mask) pairs for fill_holes; the shapes they need are skipped on arrays too small for them"""
    rs = np.random.RandomState(7 * X + Y)
    yield "zero", np.zeros((X, Y), np.uint8)
    yield "one", np.ones((X, Y), np.uint8)
    for density in (0.55, 0.7):
        yield f"random{density}", (rs.rand(X, Y) < density).astype(np.uint8) * rs.randint(1, 256, (X, Y)).astype(np.uint8)
    if X >= 12 and Y >= 12:
        yield "ring", ring(X, Y, 2, 3, 7)
        yield "ring with a diagonal leak", ring(X, Y, 2, 3, 7, leak="diagonal")
        m = ring(X, Y, 0, 2, 8)
        m[0, 3:9] = 0                                              # the top side lies on row 0 and is open: the hole touches the border
        yield "ring whose hole touches the border", m
        n = np.zeros((X, Y), np.uint8)
        s = min(X, Y)
        for k in range(0, s // 2 - 1, 2):                          # nested rings, two cells apart, down to the centre
            n[k:s - k, k:s - k] = 1
            n[k + 1:s - k - 1, k + 1:s - k - 1] = 0
        yield "nested rings", n
        f = np.ones((X, Y), np.uint8)
        f[1:-1, 1:-1] = 0                                          # a frame on the border: everything inside is one hole
        yield "frame", f
    if X >= 40 and Y >= 90:
        both = ring(X, Y, 10, 58, 12) | ring(X, Y, 20, 30, 9, leak="diagonal")   # across the labeller's 16 x 64 tile borders
        yield "rings across tiles", both


def edt_patterns(X, Y):
    """(name, mask) pairs for the distance transform"""
    rs = np.random.RandomState(31 * X + Y)
    yield "all zero", np.zeros((X, Y), np.uint8)
    yield "all one", np.ones((X, Y), np.uint8)
    for name, (x, y) in (("corner 00", (0, 0)), ("corner 0Y", (0, Y - 1)), ("corner X0", (X - 1, 0)), ("corner XY", (X - 1, Y - 1)),
                         ("centre", (X // 2, Y // 2))):
        m = np.ones((X, Y), np.uint8)
        m[x, y] = 0
        yield f"lone zero {name}", m
    m = np.full((X, Y), 255, np.uint8)
    m[0, 0] = m[X - 1, Y - 1] = 0
    yield "two zeros at opposite corners", m
    yield "checkerboard", FR.checkerboard(X, Y)
    for density in (0.5, 0.97, 0.999):
        yield f"random{density}", (rs.rand(X, Y) < density).astype(np.uint8) * rs.randint(1, 256, (X, Y)).astype(np.uint8)


def fixture_truth(shape=(100, 100), resolution=4, positive=True):
    """the truth mask of tests/golden/annotation_small.json, by the annotation restatement (what Annotation.mask gives on the device)"""
    import _annotation_ref as AR
    with open(FIXTURE) as f:
        doc = json.load(f)
    polys = [np.asarray(e["vertices"], dtype=np.float64) for e in doc["positive" if positive else "negative"]]
    X, Y = shape
    pts = np.stack([np.repeat(np.arange(X) * resolution, Y), np.tile(np.arange(Y) * resolution, X)], 1)
    return AR.inside_first(pts, polys)[0].reshape(X, Y)


def blob_truth():
    """one-cell, line, disc and ring lesions on 120 x 150: after the 75 um dilation at CELL_UM some are ITCs (major axis below
    275 um = 17.7 cells) and some are not; two discs close enough to merge under the dilation; a ring whose hole is filled"""
    m = np.zeros((120, 150), np.uint8)
    m[5, 5] = 1                                                    # one cell: ITC
    m[0, 140] = 1                                                  # one cell at the border: ITC
    m[20, 10:40] = 1                                               # a line of 30: not an ITC
    m[30:36, 60] = 1                                               # a line of 6: ITC
    xx, yy = np.mgrid[0:120, 0:150]
    m[(xx - 60) ** 2 + (yy - 40) ** 2 <= 64] = 1                   # a disc of radius 8: not an ITC
    m[(xx - 60) ** 2 + (yy - 100) ** 2 <= 9] = 1                   # a disc of radius 3: ITC
    m[(xx - 95) ** 2 + (yy - 30) ** 2 <= 16] = 1                   # two discs of radius 4, 3 cells apart: one lesion after the dilation
    m[(xx - 95) ** 2 + (yy - 41) ** 2 <= 16] = 1
    m |= ring(120, 150, 85, 90, 14)                                # a ring: its hole is filled
    m[110:113, 120:149:2] = 1                                      # a comb of single columns two cells apart: merged by the dilation
    return m
