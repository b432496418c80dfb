"""Camelyon16 annotations on the MI355X.  Every bound is equality: the polygon kernel (both paths, with and without the cull, both
point sources) against the restatement of tests/_annotation_ref.py, the confusion counts against NumPy on the same float32 values,
the loaders against NumPy slicing plus restated labels, and ``camelyon16_test`` / ``cam_cr_validate`` against the same calls without
the new pieces."""
import functools
import os
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import cases as C  # noqa: E402
from oracle import model as OM  # noqa: E402

from _annotation_ref import inside_first, pack, pip_int, star_polygon, tangled_polygon  # noqa: E402
from _inference_util import cut_tiles, scale_head  # noqa: E402

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "annotation_small.json")
BIG = 1 << 24


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _run(points, polys, *, grid=None, bounds="own", **kw):
    """kernels.points_in_polygons on host arrays -> (inside, first) as NumPy.  bounds: "own" = the polygons' extremes, None, or an array"""
    from ssl_cr_histo_amd import kernels as K
    vertices, offsets, own = pack(polys)
    b = own if isinstance(bounds, str) else bounds
    inside, first = K.points_in_polygons(None if points is None else _dev(np.asarray(points, dtype=np.float64).reshape(-1, 2)),
                                         _dev(vertices), _dev(offsets), grid=grid, bounds=None if b is None else _dev(b), first=True, **kw)
    assert inside.dtype == torch.uint8 and first.dtype == torch.int32
    return inside.cpu().numpy(), first.cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------- the polygon sets
@functools.lru_cache(maxsize=None)
def _polygon_set(P):
    """P polygons with integer vertices in [0, 512): overlapping and nested stars and self-intersecting ones, whose vertex counts walk
    through 1, 2, 3, PIP_CHUNK - 1, PIP_CHUNK, PIP_CHUNK + 1 and 3 PIP_CHUNK + 5 -- a polygon that spans chunks, chunks that span polygons"""
    from ssl_cr_histo_amd import kernels as K
    ch = K.PIP_CHUNK
    sizes = {0: [], 1: [3 * ch + 5], 3: [ch + 1, 2, ch - 1],
             17: [3, 1, ch - 1, 5, 2, ch, 7, ch + 1, 3, 3 * ch + 5, 0, 4, 31, 3, ch, 1, 9]}[P]
    rs = np.random.RandomState(100 + P)
    polys = []
    for k, n in enumerate(sizes):
        if k % 3 == 2:
            polys.append(tangled_polygon(rs, n, 100, 400))
        else:                                                      # centres close to one another, radii from small to large: nested
            polys.append(np.clip(star_polygon(rs, n, (256 + 20 * (k % 5), 256 - 15 * (k % 4)), 40 + 25 * (k % 7)), 0, 511))
    return tuple(polys)


@functools.lru_cache(maxsize=None)
def _points_and_truth(N, P):
    """N integer points over the polygons' frame, some of them ON vertices; their restated (inside, first): computed once"""
    polys = _polygon_set(P)
    rs = np.random.RandomState(7 * N + P)
    pts = rs.randint(90, 430, (N, 2)).astype(np.float64)
    verts = pack(polys)[0]
    if len(verts) and N > 4:
        k = rs.randint(0, len(verts), N // 4)
        pts[:len(k)] = verts[k]
    return pts, inside_first(pts, polys)


@pytest.mark.parametrize("P", [0, 1, 3, 17])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 257, 1000])
def test_points_in_polygons_equals_the_restatement(N, P):
    polys = _polygon_set(P)
    pts, (inside, first) = _points_and_truth(N, P)
    if P and N >= 257:
        assert 0 < inside.sum() < N
    if P == 17 and N == 1000:
        assert len(np.unique(first)) >= 6                          # overlapping polygons: the first hit is not always the same one
    for kw in (dict(exact=True), dict(exact=False), dict(), dict(exact=True, bounds=None), dict(exact=False, bounds=None)):
        got_inside, got_first = _run(pts, polys, **kw)
        assert got_inside.shape == (N,) and np.array_equal(got_first, first), (kw, int((got_first != first).sum()))
        assert np.array_equal(got_inside, inside), kw


def test_inside_alone_and_out_tensors():
    from ssl_cr_histo_amd import kernels as K
    polys = _polygon_set(3)
    pts, (inside, first) = _points_and_truth(257, 3)
    vertices, offsets, bounds = (_dev(a) for a in pack(polys))
    got = K.points_in_polygons(_dev(pts), vertices, offsets, bounds=bounds)
    assert torch.is_tensor(got) and np.array_equal(got.cpu().numpy(), inside)
    out = (torch.full((257,), 9, dtype=torch.uint8, device=DEV), torch.full((257,), 9, dtype=torch.int32, device=DEV))
    ret = K.points_in_polygons(_dev(pts), vertices, offsets, first=True, out=out)
    assert ret[0] is out[0] and ret[1] is out[1]
    assert np.array_equal(out[0].cpu().numpy(), inside) and np.array_equal(out[1].cpu().numpy(), first)
    none = K.points_in_polygons(torch.zeros((0, 2), dtype=torch.float64, device=DEV), vertices, offsets, first=True)
    assert none[0].shape == (0,) and none[1].shape == (0,)


# ---------------------------------------------------------------------------------------------------------------- placements
RECT = np.array([[2, 2], [10, 2], [10, 6], [10, 6], [6, 6], [6, 10], [14, 10], [14, 14], [2, 14], [2, 2]], dtype=np.float64)


@pytest.mark.parametrize("shift, scale", [((0, 0), 1), ((-20, -9), 1), ((BIG - 15, -BIG), 1), ((-BIG, BIG - 15), 1), ((0, 0), 1 << 20)])
def test_points_on_vertices_edges_and_half_open_ends(shift, scale):
    """every integer point of the frame of a rectilinear polygon with a repeated vertex (points on vertices, on horizontal and on
    vertical edges, on both ends of every y-span) and of a slanted one; moved to negative coordinates and to both corners of the
    integer path's range, and scaled up to it"""
    slanted = np.array([[1, 1], [15, 3], [9, 8], [13, 15], [3, 12], [6, 7]], dtype=np.float64)
    pts = np.stack(np.meshgrid(np.arange(0, 17), np.arange(0, 17), indexing="ij"), -1).reshape(-1, 2).astype(np.float64)
    if scale > 1:
        pts = np.concatenate([pts * scale, pts * scale + 1, pts * scale - 1])
    polys = [(RECT * scale + shift), (slanted * scale + shift)]
    pts = np.clip(pts + shift, -BIG, BIG)
    assert max(np.abs(p).max() for p in polys) <= BIG
    inside, first = inside_first(pts, polys)
    # the integer form in Python ints says the same
    assert np.array_equal(pip_int(pts, polys[0]) | pip_int(pts, polys[1]), inside.astype(bool))
    assert 0 < inside.sum() < len(pts) and set(np.unique(first)) == {-1, 0, 1}
    for kw in (dict(exact=True), dict(exact=False), dict(exact=True, bounds=None), dict(exact=False, bounds=None)):
        got_inside, got_first = _run(pts, polys, **kw)
        assert np.array_equal(got_first, first) and np.array_equal(got_inside, inside), kw


def test_float64_path_on_non_integer_data():
    """non-integer vertices and points, negative coordinates, a polygon that spans chunks; the cull's bounds are the package's
    (``polygon_bounds``: x widened by what the chain can round)"""
    from ssl_cr_histo_amd import kernels as K
    from ssl_cr_histo_amd.annotation import polygon_bounds
    rs = np.random.RandomState(5)
    polys = [star_polygon(rs, 5, (10.1, -12.7), 22.0, integer=False) / 3.0, star_polygon(rs, K.PIP_CHUNK + 9, (-3.25, 4.5), 30.0, integer=False),
             tangled_polygon(rs, 23, -40.0, 40.0, integer=False)]
    pts = rs.uniform(-45, 45, (1000, 2))
    pts[:200] = np.round(pts[:200] * 4) / 4
    pts[200:230] = polys[1][:30]                                   # on vertices
    pts[230:253, 1] = polys[2][:, 1]                               # on the y of every vertex of the tangled one: the half-open ends
    inside, first = inside_first(pts, polys)
    assert 0 < inside.sum() < len(pts) and len(np.unique(first)) == 4
    assert not K.pip_exact_ok(pack(polys)[0])
    bounds = np.array([polygon_bounds(v) for v in polys])
    for kw in (dict(exact=False, bounds=None), dict(exact=False, bounds=bounds), dict(bounds=bounds)):
        got_inside, got_first = _run(pts, polys, **kw)
        assert np.array_equal(got_first, first) and np.array_equal(got_inside, inside), kw.keys()


def test_bounds_that_exclude_every_point():
    polys = _polygon_set(17)
    pts, (inside, first) = _points_and_truth(257, 17)
    far = pts + 1000.0                                             # the true bounds exclude every point: nothing is staged, all zeros
    for kw in (dict(exact=True), dict(exact=False)):
        got_inside, got_first = _run(far, polys, **kw)
        assert not got_inside.any() and (got_first == -1).all()
        assert np.array_equal(got_inside, inside_first(far, polys)[0])
    # the cull is the caller's statement: bounds that hold no point switch every polygon off
    nothing = np.tile(np.array([5000.0, 5000.0, 6000.0, 6000.0]), (17, 1))
    got_inside, got_first = _run(pts, polys, bounds=nothing, exact=True)
    assert inside.any() and not got_inside.any() and (got_first == -1).all()
    # ... and bounds that hold everything change nothing
    everything = np.tile(np.array([-1e9, -1e9, 1e9, 1e9]), (17, 1))
    got_inside, got_first = _run(pts, polys, bounds=everything, exact=False)
    assert np.array_equal(got_first, first)


# ---------------------------------------------------------------------------------------------------------------- the grid source
@pytest.mark.parametrize("nx, ny", [(1, 1), (5, 7), (65, 33)])
def test_grid_source_equals_the_explicit_source(nx, ny):
    x0, y0, step = -192, 128, 64
    rs = np.random.RandomState(nx)
    polys = [star_polygon(rs, 40, (x0 + 32 * nx, y0 + 32 * ny), 24.0 * max(nx, ny) + 40), tangled_polygon(rs, 300, x0, x0 + 64 * nx + 64),
             np.array([[x0, y0], [x0 + 64, y0], [x0 + 64, y0 + 64], [x0, y0 + 64]], dtype=np.float64)]
    ii, jj = np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij")
    pts = np.stack([x0 + ii * step, y0 + jj * step], -1).reshape(-1, 2).astype(np.float64)
    inside, first = inside_first(pts, polys)
    assert inside[0] == 1                                          # (x0, y0) is a vertex of the square whose y-span starts there
    for kw in (dict(exact=True), dict(exact=False), dict(), dict(exact=True, bounds=None)):
        e_inside, e_first = _run(pts, polys, **kw)
        g_inside, g_first = _run(None, polys, grid=(x0, y0, step, nx, ny), **kw)
        assert g_inside.shape == (nx, ny) and g_first.shape == (nx, ny)
        assert np.array_equal(g_inside.reshape(-1), e_inside) and np.array_equal(g_first.reshape(-1), e_first), kw
        assert np.array_equal(e_inside, inside) and np.array_equal(e_first, first), kw
    if nx > 1:
        assert 0 < inside.sum() < len(pts)


@pytest.mark.parametrize("resolution", [64, 48.5])
def test_annotation_mask_equals_the_per_cell_expression(resolution):
    from ssl_cr_histo_amd.annotation import Annotation
    a = Annotation().from_json(FIXTURE).to_device(DEV)
    X, Y = 9, 9
    for flag in (True, False):
        polys = a.polygon_vertices(flag)
        centres = [(int(x * resolution), int(y * resolution)) for x in range(X) for y in range(Y)]     # dataset.py:985-988
        want = inside_first(np.array(centres), polys)[0].reshape(X, Y)
        got = a.mask((X, Y), resolution, flag)
        assert got.is_cuda and got.dtype == torch.uint8 and got.shape == (X, Y)
        assert np.array_equal(got.cpu().numpy(), want)
        assert want.tolist() == [[int(a.inside_polygons(centres[x * Y + y], flag)) for y in range(Y)] for x in range(X)]
        assert 0 < want.sum() < X * Y
        inside, first = a.inside(centres, flag, first=True)
        assert np.array_equal(first.cpu().numpy(), inside_first(np.array(centres), polys)[1])
        assert np.array_equal(inside.cpu().numpy(), want.reshape(-1))
    labels = a.labels(np.array(centres))
    assert labels.dtype == torch.int64 and labels.is_cuda
    assert np.array_equal(labels.cpu().numpy(), inside_first(np.array(centres), a.polygon_vertices(True))[0].astype(np.int64))


# ---------------------------------------------------------------------------------------------------------------- map_confusion
def _confusion_ref(pm, truth, tissue, thr):
    out = np.zeros((len(thr), 2, 2), dtype=np.int64)
    sel = tissue != 0
    for t, v in enumerate(thr):
        pred = pm[sel] >= v                                        # float32 against float32
        tr = truth[sel] != 0
        for a in (0, 1):
            for b in (0, 1):
                out[t, a, b] = np.count_nonzero((tr == a) & (pred == b))
    return out


@pytest.mark.parametrize("T", [1, 5, 64])
@pytest.mark.parametrize("X, Y", [(1, 1), (7, 5), (130, 67)])
def test_map_confusion_equals_numpy(X, Y, T):
    from ssl_cr_histo_amd import kernels as K
    rs = np.random.RandomState(X * 100 + T)
    thr = np.sort(rs.rand(T)).astype(np.float32)
    pm = rs.rand(X, Y).astype(np.float32)
    flat = pm.reshape(-1)
    flat[::3] = thr[rs.randint(0, T, len(flat[::3]))]              # values EQUAL to a threshold: >= counts them
    if flat.size > 4:
        flat[4] = np.nan                                           # below every threshold
    truth = (rs.rand(X, Y) < 0.4).astype(np.uint8) * 255           # nonzero = set
    tissue = (rs.rand(X, Y) < 0.7).astype(np.uint8)
    if X * Y == 1:
        tissue[:] = 1
    want = _confusion_ref(pm, truth, tissue, thr)
    got = K.map_confusion(_dev(pm), _dev(truth), _dev(tissue), thr)
    assert got.dtype == torch.int64 and got.shape == (T, 2, 2) and got.is_cuda
    assert np.array_equal(got.cpu().numpy(), want)
    assert (want.sum((1, 2)) == np.count_nonzero(tissue)).all()
    # bool masks, thresholds already on the device; an empty tissue mask counts nothing
    again = K.map_confusion(_dev(pm), _dev(truth != 0), _dev(tissue != 0), _dev(thr))
    assert np.array_equal(again.cpu().numpy(), want)
    empty = K.map_confusion(_dev(pm), _dev(truth), _dev(np.zeros_like(tissue)), thr)
    assert not empty.cpu().numpy().any()


def test_map_scores_figures():
    from ssl_cr_histo_amd.inference import map_scores
    rs = np.random.RandomState(3)
    pm = rs.rand(26, 19)
    truth = rs.rand(26, 19) < 0.3
    tissue = rs.rand(26, 19) < 0.8
    thr = [0.0, 0.25, 0.5, 0.9, 2.0]
    s = map_scores(pm, _dev(truth.astype(np.uint8)), tissue, thr)
    want = _confusion_ref(pm.astype(np.float32), truth, tissue, np.asarray(thr, dtype=np.float32))
    assert np.array_equal(s["confusion"], want) and s["confusion"].dtype == np.int64
    tn, fp, fn, tp = (want[:, a, b].astype(np.float64) for a, b in ((0, 0), (0, 1), (1, 0), (1, 1)))
    assert np.array_equal(s["sensitivity"], tp / (tp + fn)) and np.array_equal(s["specificity"], tn / (tn + fp))
    assert np.array_equal(s["dice"][:4], (2 * tp / (2 * tp + fp + fn))[:4]) and s["dice"][4] == 0.0
    assert s["sensitivity"][0] == 1.0 and s["specificity"][4] == 1.0


# ---------------------------------------------------------------------------------------------------------------- end to end
def _engine(dtype):
    from ssl_cr_histo_amd import engine as E
    idx = torch.device(DEV).index
    cur = E._engines.get(idx)
    if cur is None or cur.dtype != E._DTYPES[dtype]:
        E._engines.pop(idx, None)
        E.set_engine(E.Engine(DEV, dtype))
    return E.get_engine(DEV)


def _build(classes, head_scale=1.0):
    from ssl_cr_histo_amd import net
    model, cls = net.TripletNet_Finetune("resnet18"), net.FinetuneResNet(classes)
    model.load_state_dict(OM.init_state(C.PARAM_SEED, OM.net_param_specs(), random_running_stats=True))
    cls.load_state_dict(OM.init_state(C.PARAM_SEED + 1, OM.classifier_param_specs("finetune", classes)))
    scale_head(cls, head_scale)
    return model.to(DEV), cls.to(DEV)


def ns(**kw):
    return types.SimpleNamespace(print_freq=0, **kw)


def _cam_wsi():
    """the cam_wsi case: 64-pixel tiles in batches of 4 over the seeded 6 x 5 mask, on a 384 x 320 slide (resolution 64)"""
    c = C.CASES["cam_wsi"]
    mask = C.wsi_loader("cam_wsi").dataset.mask
    assert mask.shape == (6, 5) and c["hw"] == 64 and c["b"] == 4
    slide = np.random.RandomState(77).randint(0, 256, size=(5 * 64, 6 * 64, 3), dtype=np.uint8)
    return slide, mask, c["hw"], c["b"]


def _host_confusion(target, pred):
    cm = np.zeros((2, 2), dtype=np.int64)
    np.add.at(cm, (target, pred), 1)
    return cm


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_wsi_loader_with_annotation(dtype):
    from ssl_cr_histo_amd import steps
    from ssl_cr_histo_amd.annotation import Annotation
    from ssl_cr_histo_amd.inference import WsiDeviceLoader, map_scores
    _engine(dtype)
    slide, mask, S, B = _cam_wsi()
    ann = Annotation().from_json(FIXTURE)
    polys = ann.polygon_vertices(True)
    plain = WsiDeviceLoader(slide, mask, S, B)
    loader = WsiDeviceLoader(slide, mask, S, B, annotation=ann)
    assert plain.targets is None and plain.truth is None and loader.dataset.resolution == 64
    # .targets and .truth against the restatement
    xs, ys = np.where(mask)
    labels = inside_first(np.stack([xs * 64, ys * 64], 1), polys)[0].astype(np.int64)
    cells = np.array([(int(x * 64), int(y * 64)) for x in range(6) for y in range(5)])
    truth = inside_first(cells, polys)[0].reshape(6, 5)
    assert loader.targets.is_cuda and loader.targets.dtype == torch.int64 and np.array_equal(loader.targets.cpu().numpy(), labels)
    assert loader.truth.is_cuda and loader.truth.dtype == torch.uint8 and np.array_equal(loader.truth.cpu().numpy(), truth)
    assert 0 < labels.sum() < len(labels) and 0 < truth.sum() < truth.size      # the polygons cut through the mask
    model, cls = _build(2, head_scale=0.05)
    steps._last_test["confusion"] = None
    want_map = steps.camelyon16_test(ns(), model, cls, plain)
    assert steps.last_test_confusion() is None                     # without an annotation: the path of every earlier version
    got_map = steps.camelyon16_test(ns(), model, cls, loader)
    assert got_map.dtype == np.float64 and np.array_equal(got_map, want_map)   # bit for bit
    p = got_map[xs, ys]
    print("map values at the tissue cells:", p)
    assert np.abs(p - 0.5).min() > 1e-6
    cm = steps.last_test_confusion()
    assert cm.dtype == torch.int64 and not cm.is_cuda and cm.shape == (2, 2)
    assert np.array_equal(cm.numpy(), _host_confusion(labels, (p > 0.5).astype(np.int64))) and int(cm.sum()) == len(xs)
    # test-time augmentation: the ensemble's map, every tile counted once
    want_tta = steps.camelyon16_test(ns(tta="flips"), model, cls, plain)
    got_tta = steps.camelyon16_test(ns(tta="flips"), model, cls, loader)
    assert np.array_equal(got_tta, want_tta) and not np.array_equal(got_tta, got_map)
    q = got_tta[xs, ys]
    assert np.abs(q - 0.5).min() > 1e-6
    cm = steps.last_test_confusion()
    assert np.array_equal(cm.numpy(), _host_confusion(labels, (q > 0.5).astype(np.int64))) and int(cm.sum()) == len(xs)
    # the finished map against the truth mask, over the tissue cells
    s = map_scores(got_map, loader.truth, mask, [0.5])
    sel = mask != 0
    assert np.array_equal(s["confusion"][0], _host_confusion(truth[sel].astype(np.int64), (got_map[sel].astype(np.float32) >= np.float32(0.5)).astype(np.int64)))


def _centres():
    """centres over a 384 x 320 slide, some with tiles that leave it on every side, some far outside"""
    rs = np.random.RandomState(9)
    inner = np.stack([rs.randint(40, 340, 8), rs.randint(40, 280, 8)], 1)
    edge = np.array([[0, 0], [383, 319], [10, 300], [380, 5], [-40, 100], [500, 500]])
    return np.concatenate([inner, edge]).astype(np.int64)


@pytest.mark.parametrize("S, fill", [(64, 0), (33, 255)])
def test_centre_list_loader_batches(S, fill):
    from ssl_cr_histo_amd.annotation import Annotation, CentreListLoader
    slide = np.random.RandomState(78).randint(0, 256, size=(320, 384, 3), dtype=np.uint8)
    ann = Annotation().from_json(FIXTURE)
    centres = _centres()
    origin = (16, -8)
    loader = CentreListLoader(slide, centres, ann, S, 4, origin=origin, fill=fill)
    assert len(loader) == 4 and loader.samples() == 14
    xy = np.array([(int(x - S / 2), int(y - S / 2)) for x, y in centres.tolist()])
    tiles = cut_tiles(slide, xy, S, origin=origin, fill=fill)
    labels = inside_first(centres, ann.polygon_vertices(True))[0].astype(np.int64)
    assert labels.tolist() == [int(ann.inside_polygons((int(x), int(y)), True)) for x, y in centres] and 0 < labels.sum() < 14
    got = list(loader)
    assert [len(b[0]) for b in got] == [4, 4, 4, 2]
    for k, (x, y) in enumerate(got):
        assert x.is_cuda and x.dtype == torch.uint8 and x.shape[1:] == (3, S, S) and y.is_cuda and y.dtype == torch.int64
        assert np.array_equal(x.cpu().numpy(), tiles[4 * k:4 * k + 4]) and np.array_equal(y.cpu().numpy(), labels[4 * k:4 * k + 4])
    assert (tiles[-1] == fill).all() and not (tiles[0] == fill).all()


def test_cam_cr_validate_fed_by_centre_list_loaders():
    from ssl_cr_histo_amd import steps
    from ssl_cr_histo_amd.annotation import Annotation, CentreListLoader
    _engine("fp32")
    slide = np.random.RandomState(79).randint(0, 256, size=(320, 384, 3), dtype=np.uint8)
    ann = Annotation().from_json(FIXTURE)
    S, B = 64, 4
    model, cls = _build(2, head_scale=0.05)
    cs = _centres()
    lists = (cs[:6], cs[6:12])

    def host(centres):
        xy = np.array([(int(x - S / 2), int(y - S / 2)) for x, y in centres.tolist()])
        tiles = torch.from_numpy(cut_tiles(slide, xy, S))
        labels = torch.from_numpy(inside_first(centres, ann.polygon_vertices(True))[0].astype(np.int64))
        return [(tiles[i:i + B], labels[i:i + B]) for i in range(0, len(centres), B)]

    torch.manual_seed(5)
    want = steps.cam_cr_validate(ns(), model, cls, host(lists[0]), host(lists[1]), 1)
    torch.manual_seed(5)
    got = steps.cam_cr_validate(ns(), model, cls, CentreListLoader(slide, lists[0], ann, S, B), CentreListLoader(slide, lists[1], ann, S, B), 1)
    assert got == want and np.isfinite(got[0])
