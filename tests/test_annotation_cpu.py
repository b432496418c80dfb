"""Camelyon16 annotations, the part that needs no device: the restatement of skimage 0.15 ``points_in_poly`` against itself (loop and
vectorised form), against the exact integer form and against matplotlib away from polygon boundaries; the host ``Annotation``
drop-in; the layout of the two new descriptors; and which of its two paths the kernel wrapper picks."""
import json
import os

import numpy as np
import pytest
import torch

from _annotation_ref import inside_first, on_boundary, pack, pip_int, pip_loop, pip_vec, star_polygon, tangled_polygon

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "annotation_small.json")
BIG = 1 << 24


def _random_polygons(rs, count, lo, hi, nmin=3, nmax=59):
    """alternately star-shaped and self-intersecting, integer vertices in [lo, hi)"""
    out = []
    for k in range(count):
        n = int(rs.randint(nmin, nmax + 1))
        if k % 2:
            out.append(tangled_polygon(rs, n, lo, hi))
        else:
            half = (hi - lo) / 2
            out.append(np.clip(star_polygon(rs, n, (lo + half, lo + half), half * rs.uniform(0.3, 1.0)), lo, hi - 1))
    return out


# ---------------------------------------------------------------------------------------------------------------- the definition
def test_loop_equals_vectorised_form():
    rs = np.random.RandomState(11)
    for k, poly in enumerate(_random_polygons(rs, 6, 0, 64, 3, 17) + [star_polygon(rs, 9, (3.3, -2.1), 7.7, integer=False),
                                                                      tangled_polygon(rs, 11, -5.5, 5.5, integer=False)]):
        integer = k < 6
        pts = rs.randint(-2, 66, (150, 2)).astype(np.float64) if integer else rs.uniform(-6, 12, (150, 2))
        pts = np.concatenate([pts, poly[:5], (poly[:5] + np.roll(poly, 1, 0)[:5]) / 2])       # vertices and edge midpoints too
        want = np.array([pip_loop(x, y, poly[:, 0], poly[:, 1]) for x, y in pts])
        assert np.array_equal(pip_vec(pts, poly), want), k
        assert 0 < want.sum() < len(want)


def _integer_cases():
    """(polygon, points) pairs of integer data: random polygons; a polygon of horizontal and vertical edges with a repeated vertex;
    query points on vertices, on edges and around them; magnitudes up to 2^24, negatives included"""
    rs = np.random.RandomState(12)
    cases = []
    for poly in _random_polygons(rs, 8, 0, 48, 3, 23):
        pts = np.stack(np.meshgrid(np.arange(-1, 50), np.arange(-1, 50), indexing="ij"), -1).reshape(-1, 2)
        cases.append((poly, pts))
    steps = np.array([[2, 2], [10, 2], [10, 6], [10, 6], [6, 6], [6, 10], [14, 10], [14, 14], [2, 14], [2, 2]])     # rectilinear, repeats
    cases.append((steps, np.stack(np.meshgrid(np.arange(0, 17), np.arange(0, 17), indexing="ij"), -1).reshape(-1, 2)))
    for sign in (1, -1):
        for poly in (np.array([[BIG, BIG], [BIG - 7, BIG], [BIG - 3, BIG - 9], [-BIG, -BIG + 5], [BIG - 1, -BIG]]),
                     np.array([[BIG, -BIG], [BIG, BIG], [-BIG, BIG], [-BIG, -BIG]]),
                     tangled_polygon(rs, 13, -BIG, BIG + 1)):
            poly = sign * poly
            around = np.concatenate([poly + d for d in ((0, 0), (1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, -1))])
            mids = (poly + np.roll(poly, 1, 0)) // 2
            far = rs.randint(-BIG, BIG + 1, (300, 2))
            pts = np.clip(np.concatenate([around, mids, far]), -BIG, BIG)
            cases.append((poly, pts))
    return cases


def test_float64_chain_equals_the_exact_integer_form_on_integer_inputs():
    total = 0
    for k, (poly, pts) in enumerate(_integer_cases()):
        assert np.abs(poly).max() <= BIG and np.abs(pts).max() <= BIG
        got, want = pip_vec(pts, poly), pip_int(pts, poly)
        assert np.array_equal(got, want), (k, int((got != want).sum()))
        total += len(pts)
    assert total > 20000


def test_restatement_equals_matplotlib_off_the_boundary():
    Path = pytest.importorskip("matplotlib.path").Path
    rs = np.random.RandomState(13)
    pts = np.stack(np.meshgrid(np.arange(256), np.arange(256), indexing="ij"), -1).reshape(-1, 2)
    polys = _random_polygons(rs, 40, 0, 256)
    edge = compared = 0
    for k, poly in enumerate(polys):
        mine = pip_vec(pts, poly)
        theirs = Path(poly).contains_points(pts.astype(np.float64))
        b = on_boundary(pts, poly)
        assert np.array_equal(mine[~b], theirs[~b]), (k, int((mine[~b] != theirs[~b]).sum()))
        edge += int(b.sum())
        compared += int((~b).sum())
    share = edge / (edge + compared)
    print(f"boundary points: {edge} of {edge + compared} = {100 * share:.3f} %")
    assert share <= 0.01


# ---------------------------------------------------------------------------------------------------------------- Annotation
def test_annotation_from_json_round_trip_and_lists(tmp_path):
    from ssl_cr_histo_amd.annotation import Annotation
    doc = json.load(open(FIXTURE))
    a = Annotation()
    assert str(a) == ""
    a.from_json(FIXTURE)
    assert str(a) == FIXTURE
    for key, flag in (("positive", True), ("negative", False)):
        got = a.polygon_vertices(flag)
        assert len(got) == len(doc[key])
        for g, entry in zip(got, doc[key]):
            assert isinstance(g, np.ndarray) and np.array_equal(g, np.array(entry["vertices"]))
    # written back in the reference's layout and read again: the same polygons
    out = {key: [{"name": str(p), "vertices": p.vertices().tolist()} for p in a._polygons(flag)] for key, flag in (("positive", True), ("negative", False))}
    assert out == doc
    path = tmp_path / "again.json"
    path.write_text(json.dumps(out))
    b = Annotation()
    b.from_json(str(path))
    grid = [(x, y) for x in range(0, 400, 7) for y in range(0, 400, 9)]
    for flag in (True, False):
        polys = [np.array(e["vertices"]) for e in doc["positive" if flag else "negative"]]
        want = inside_first(np.array(grid), polys)[0].astype(bool)
        got = [a.inside_polygons(c, flag) for c in grid]              # a tuple of ints, as the datasets call it
        assert all(isinstance(g, bool) for g in got)
        assert got == want.tolist() and got == [b.inside_polygons(c, flag) for c in grid]
        assert 0 < want.sum() < len(want)
    # the two lists differ: a point of the first tumour polygon that no normal polygon holds, and the other way round
    assert a.inside_polygons((150, 40), True) and not a.inside_polygons((150, 40), False)
    assert a.inside_polygons((350, 305), False) and not a.inside_polygons((350, 305), True)


def test_annotation_first_hit_order_and_degenerate_polygons():
    from ssl_cr_histo_amd.annotation import Annotation
    square = [[0, 0], [10, 0], [10, 10], [0, 10]]
    polys = [[], [[5, 5]], [[0, 0], [10, 10]], square, [[2, 2], [8, 2], [8, 8], [2, 8]]]
    a = Annotation().from_vertices(polys, [square])
    assert [len(v) for v in a.polygon_vertices(True)] == [0, 1, 2, 4, 4] and len(a.polygon_vertices(False)) == 1
    assert a.inside_polygons((5, 5), True) and a.inside_polygons((1, 1), True) and not a.inside_polygons((11, 5), True)
    # a polygon of 0, 1 or 2 vertices contains nothing, not even its own vertices
    empty = Annotation().from_vertices(polys[:3])
    assert not any(empty.inside_polygons(c, True) for c in ((5, 5), (0, 0), (10, 10), (3, 3)))
    assert not Annotation().inside_polygons((0, 0), True) and not Annotation().inside_polygons((0, 0), False)
    # the loop returns at the FIRST polygon that holds the point: the packed order is the list's order
    vertices, offsets, bounds, exact = a.packed(True)
    assert offsets.tolist() == [0, 0, 1, 3, 7, 11] and offsets.dtype == np.int32 and vertices.shape == (11, 2) and exact
    assert bounds.shape == (5, 4) and bounds[3].tolist() == [0, 0, 10, 10] and bounds[0, 0] > bounds[0, 2]
    _, first = inside_first([(5, 5), (1, 1), (11, 5)], polys)
    assert first.tolist() == [3, 3, -1]
    calls = []
    for k, p in enumerate(a._polygons(True)):
        inner = p.inside
        p.inside = lambda coord, k=k, inner=inner: calls.append(k) or inner(coord)
    assert a.inside_polygons((5, 5), True) and calls == [0, 1, 2, 3]


# ---------------------------------------------------------------------------------------------------------------- descriptors
def test_version_is_16_and_the_entries_are_exported():
    from ssl_cr_histo_amd import _lib as L
    from ssl_cr_histo_amd import build
    if not os.path.exists(L.LIB_PATH):
        build.build()
    from ssl_cr_histo_amd import engine  # noqa: F401  registers engine signatures
    lib = L.lib()
    assert lib.sslcr_version() == 16      # (15 brought these entries; 16 the switch listing)
    assert {"sslcr_points_in_polygons", "sslcr_map_confusion"} <= set(build.header_symbols())
    # argument checks run before any device work
    assert lib.sslcr_points_in_polygons(None, None) == -1
    d = L.PipDesc()
    d.N, d.nx, d.ny = 6, 2, 2
    assert lib.sslcr_points_in_polygons(d, None) == -1 and b"nx * ny" in lib.sslcr_last_error()
    d.N = 0
    assert lib.sslcr_points_in_polygons(L.PipDesc(), None) == 0            # N = 0: a no-op
    m = L.MapConfusionDesc()
    m.X, m.Y, m.T = 4, 4, 65
    assert lib.sslcr_map_confusion(m, None) == -1 and b"T outside" in lib.sslcr_last_error()


# ---------------------------------------------------------------------------------------------------------------- path choice
class _Recorder:
    """stands in for libsslcr.so: keeps the descriptor of every sslcr_points_in_polygons call"""

    def __init__(self):
        self.exact = []

    def sslcr_points_in_polygons(self, d, stream):
        self.exact.append(int(d.exact))
        return 0


@pytest.fixture
def recorder(monkeypatch):
    from ssl_cr_histo_amd import _lib as L
    from ssl_cr_histo_amd import kernels as K
    rec = _Recorder()
    monkeypatch.setattr(L, "lib", lambda: rec)
    monkeypatch.setattr(L, "stream_ptr", lambda: None)
    monkeypatch.setattr(K, "_chk", lambda *ts: None)
    return rec


def test_wrapper_picks_the_integer_path_only_under_its_precondition(recorder):
    from ssl_cr_histo_amd import kernels as K
    assert K.PIP_EXACT_MAX == BIG
    ints = np.array([[0, 0], [BIG, 0], [-BIG, BIG], [5, -BIG]], dtype=np.float64)
    half, over = ints.copy(), ints.copy()
    half[2, 1] = 0.5
    over[1, 0] = BIG + 1
    assert K.pip_exact_ok(ints) and K.pip_exact_ok(torch.from_numpy(ints)) and K.pip_exact_ok(np.zeros((0, 2)))
    for bad in (half, over, -over, np.array([[np.nan, 0.0]]), np.array([[np.inf, 0.0]])):
        assert not K.pip_exact_ok(bad) and not K.pip_exact_ok(torch.from_numpy(bad))
    off = torch.tensor([0, 4], dtype=torch.int32)
    t = torch.from_numpy
    for verts, pts, want in ((ints, ints, 1), (half, ints, 0), (ints, half, 0), (over, ints, 0), (ints, over, 0)):
        K.points_in_polygons(t(pts), t(verts), off)
        assert recorder.exact[-1] == want
    for grid, want in (((0, 0), 1), ((-BIG, 64), 1), ((BIG - 64 * 3, 64), 1), ((BIG - 64 * 3 + 1, 64), 0), ((0, BIG), 0)):
        K.points_in_polygons(None, t(ints), off, grid=(grid[0], 0, grid[1], 4, 2))
        assert recorder.exact[-1] == want, grid
    K.points_in_polygons(None, t(half), off, grid=(0, 0, 64, 4, 2))
    assert recorder.exact[-1] == 0
    # forced either way, whatever the data
    K.points_in_polygons(t(half), t(half), off, exact=True)
    K.points_in_polygons(t(ints), t(ints), off, exact=False)
    assert recorder.exact[-2:] == [1, 0]
    from ssl_cr_histo_amd import _lib as L
    with pytest.raises(L.SslcrError):
        K.points_in_polygons(t(ints), t(ints), off, grid=(0, 0, 1, 1, 1))
    with pytest.raises(L.SslcrError):
        K.points_in_polygons(None, t(ints), off)


def test_annotation_checks_each_source_once(recorder):
    """the vertices' check is the annotation's (``packed``), the points' check the call's: Annotation passes ``exact`` itself"""
    from ssl_cr_histo_amd.annotation import Annotation, polygon_bounds
    a = Annotation().from_json(FIXTURE).to_device("cpu")
    assert a.packed(True)[3] and a.packed(False)[3]
    a.inside([(3, 4), (5, 6)])
    a.inside([(3.5, 4), (5, 6)])
    a.inside([(BIG + 1, 4)])
    a.mask((6, 5), 64)
    a.mask((6, 5), 64.5)                                                 # the explicit source: int(x_mask * 64.5) are integers
    a.mask((6, 5), 1 << 23)                                              # centres up to 5 * 2^23 > 2^24
    assert recorder.exact == [1, 0, 0, 1, 1, 0]
    b = Annotation().from_vertices([[[0, 0], [10.5, 0], [3, 9]]]).to_device("cpu")
    assert not b.packed(True)[3]
    b.inside([(3, 4)])
    assert recorder.exact[-1] == 0
    # the cull's bounds: the extremes on integer data, widened in x where the chain can round
    assert polygon_bounds(np.array([[0.0, 0], [10, 0], [3, 9]])) == (0.0, 0.0, 10.0, 9.0)
    xmin, ymin, xmax, ymax = polygon_bounds(np.array([[0.25, 0], [10.5, 0], [3, 9]]))
    assert xmin < 0.25 and xmax > 10.5 and (ymin, ymax) == (0.0, 9.0) and xmax - 10.5 < 1e-13
