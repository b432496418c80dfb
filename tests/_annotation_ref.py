"""Shared by the annotation tests: the restatement of skimage 0.15 ``points_in_poly`` the issue fixes (a literal per-point loop and its
vectorised form), the exact integer form in Python ints, an exact boundary test, seeded polygon generators and the packing the
kernel reads.  Nothing here imports the package under test."""
import numpy as np


# ---------------------------------------------------------------------------------------------------------------- the definition
def pip_loop(x, y, xp, yp):
    """the restatement, literally: one point, Python floats (IEEE float64, one rounding per operation)"""
    x, y = float(x), float(y)
    xp, yp = [float(v) for v in xp], [float(v) for v in yp]
    n = len(xp)
    c = False
    j = n - 1
    for i in range(n):
        if ((yp[i] <= y and y < yp[j]) or (yp[j] <= y and y < yp[i])) and (x < (xp[j] - xp[i]) * (y - yp[i]) / (yp[j] - yp[i]) + xp[i]):
            c = not c
        j = i
    return c


def pip_vec(points, verts):
    """the same chain for points [N, 2] at once: a loop over the edges, NumPy float64 (the same IEEE operations in the same order)"""
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    v = np.asarray(verts, dtype=np.float64).reshape(-1, 2)
    x, y = pts[:, 0], pts[:, 1]
    c = np.zeros(len(pts), dtype=bool)
    n = len(v)
    j = n - 1
    for i in range(n):
        xi, yi, xj, yj = v[i, 0], v[i, 1], v[j, 0], v[j, 1]
        span = ((yi <= y) & (y < yj)) | ((yj <= y) & (y < yi))
        if span.any():                                           # the division is reached only where the y-test holds
            k = np.nonzero(span)[0]
            hit = x[k] < (xj - xi) * (y[k] - yi) / (yj - yi) + xi
            c[k[hit]] ^= True
        j = i
    return c


def pip_int(points, verts):
    """the exact integer form in Python ints: (x - xi) d < (xj - xi) (y - yi) for d = yj - yi > 0, reversed for d < 0"""
    pts = [(int(a), int(b)) for a, b in np.asarray(points).reshape(-1, 2).tolist()]
    v = [(int(a), int(b)) for a, b in np.asarray(verts).reshape(-1, 2).tolist()]
    out = np.zeros(len(pts), dtype=bool)
    n = len(v)
    for k, (x, y) in enumerate(pts):
        c = False
        j = n - 1
        for i in range(n):
            (xi, yi), (xj, yj) = v[i], v[j]
            if (yi <= y < yj) or (yj <= y < yi):
                d = yj - yi
                lhs, rhs = (x - xi) * d, (xj - xi) * (y - yi)
                if (lhs < rhs) if d > 0 else (lhs > rhs):
                    c = not c
            j = i
        out[k] = c
    return out


def on_boundary(points, verts):
    """exact, for integer data: the point is collinear with an edge and within its span (vertices included)"""
    pts = np.asarray(points, dtype=np.int64).reshape(-1, 2)
    v = np.asarray(verts, dtype=np.int64).reshape(-1, 2)
    x, y = pts[:, 0], pts[:, 1]
    out = np.zeros(len(pts), dtype=bool)
    n = len(v)
    for i in range(n):
        (xi, yi), (xj, yj) = v[i], v[i - 1]
        cross = (xj - xi) * (y - yi) - (yj - yi) * (x - xi)        # |terms| <= 2^52 at the magnitudes the tests use it with
        out |= (cross == 0) & (x >= min(xi, xj)) & (x <= max(xi, xj)) & (y >= min(yi, yj)) & (y <= max(yi, yj))
    return out


def inside_first(points, polys):
    """Annotation.inside_polygons over a polygon list -> (inside uint8 [N], first int32 [N]): the lowest index of a polygon that
    contains the point, -1 for none; a polygon of fewer than 3 vertices contains nothing"""
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    first = np.full(len(pts), -1, dtype=np.int32)
    for p, v in enumerate(polys):
        v = np.asarray(v, dtype=np.float64).reshape(-1, 2)
        if len(v) < 3:
            continue
        hit = pip_vec(pts, v) & (first < 0)
        first[hit] = p
    return (first >= 0).astype(np.uint8), first


# ---------------------------------------------------------------------------------------------------------------- inputs
def star_polygon(rs, n, centre, radius, integer=True):
    """n vertices at increasing angles and random radii around ``centre``: simple (star-shaped), usually not convex"""
    ang = np.sort(rs.uniform(0, 2 * np.pi, n))
    r = rs.uniform(0.3, 1.0, n) * radius
    v = np.stack([centre[0] + r * np.cos(ang), centre[1] + r * np.sin(ang)], 1)
    return np.round(v) if integer else v


def tangled_polygon(rs, n, lo, hi, integer=True):
    """n uniformly random vertices in [lo, hi)^2, joined in the order drawn: self-intersecting"""
    v = rs.uniform(lo, hi, (n, 2))
    return np.floor(v) if integer else v


def pack(polys):
    """-> (vertices float64 [V, 2], offsets int32 [P + 1], bounds float64 [P, 4] = the plain extremes)"""
    vs = [np.asarray(v, dtype=np.float64).reshape(-1, 2) for v in polys]
    offsets = np.zeros(len(vs) + 1, dtype=np.int32)
    for k, v in enumerate(vs):
        offsets[k + 1] = offsets[k] + len(v)
    vertices = np.concatenate(vs) if vs else np.zeros((0, 2))
    bounds = np.array([(v[:, 0].min(), v[:, 1].min(), v[:, 0].max(), v[:, 1].max()) if len(v) else (0, 0, -1, -1) for v in vs],
                      dtype=np.float64).reshape(len(vs), 4)
    return np.ascontiguousarray(vertices, dtype=np.float64), offsets, bounds
