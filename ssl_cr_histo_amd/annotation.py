"""Camelyon16 annotations: the polygon test behind every Camelyon label, on the host as the reference has it and on the device.

The reference's ``Annotation`` (util.py:212-279) holds the tumour ("positive") and normal ("negative") polygons of one slide;
``inside_polygons((x_center, y_center), True)`` is the label of a patch in all four Camelyon datasets (dataset.py:740-743, 834-837,
922-925) and the truth a probability map is scored against at the centre of every mask cell (dataset.py:985-988).  ``Polygon.inside``
is ``skimage.measure.points_in_poly([coord], vertices)[0]``; the version the reference pins (0.15.0) evaluates, in float64,

    c = 0; j = n - 1
    for i in 0 .. n-1:
        if ((yp[i] <= y and y < yp[j]) or (yp[j] <= y and y < yp[i])) and (x < (xp[j] - xp[i]) * (y - yp[i]) / (yp[j] - yp[i]) + xp[i]):
            c = not c
        j = i

and this restatement is the definition here -- unpinned against scikit-image itself.

``Annotation`` is a drop-in for the reference's class and evaluates on the host in NumPy: no device, no scikit-image.  ``to_device``
uploads the two polygon lists once (vertices, offsets, bounds); ``inside`` / ``labels`` / ``mask`` then run one launch of
``kernels.points_in_polygons`` per call and return device tensors.  The kernel's integer path is taken where the host has checked its
precondition -- integer coordinates of magnitude <= 2^24 -- once per annotation and once per point source.

``CentreListLoader`` is the ``DatasetCamelyon16_eval`` contract (dataset.py:871-939) from a slide region in HBM: tiles by
``inference.gather_tiles``, labels by ``Annotation.labels``.
"""
import json

import numpy as np
import torch

from . import kernels as K


def _as_xy(vertices):
    """anything ``np.array`` takes -> float64 [n, 2] (an empty list is a polygon of no vertices)"""
    v = np.asarray(vertices, dtype=np.float64)
    if v.size == 0:
        return np.zeros((0, 2), dtype=np.float64)
    if v.ndim != 2 or v.shape[1] != 2:
        raise ValueError(f"a polygon is an [n, 2] array of (x, y) vertices, got shape {v.shape}")
    return v


def point_in_polygon(coord, vertices):
    """the restatement above for ONE point, vectorised over the edges: the parity of the number of edges that pass both tests.  The
    quotient of an edge that fails the y-test (a horizontal edge divides by zero) is computed and discarded."""
    v = _as_xy(vertices)
    if len(v) < 3:
        return False
    x, y = float(coord[0]), float(coord[1])
    xi, yi = v[:, 0], v[:, 1]
    xj, yj = np.roll(xi, 1), np.roll(yi, 1)
    span = ((yi <= y) & (y < yj)) | ((yj <= y) & (y < yi))
    with np.errstate(divide="ignore", invalid="ignore"):
        cross = span & (x < (xj - xi) * (y - yi) / (yj - yi) + xi)
    return bool(np.count_nonzero(cross) & 1)


class Polygon:
    """a named polygon, [n, 2] vertices (util.py:180-209)"""

    def __init__(self, name, vertices):
        self._name = name
        self._vertices = vertices

    def __str__(self):
        return self._name

    def inside(self, coord):
        return point_in_polygon(coord, self._vertices)

    def vertices(self):
        return np.array(self._vertices)


def polygon_bounds(v):
    """(xmin, ymin, xmax, ymax) of float64 vertices [n, 2] for the kernel's cull.  The y-test is a plain comparison, so ymin / ymax are
    the extremes.  The chain's right-hand side is a rounded convex combination of xp[i] and xp[j]: it can leave [xmin, xmax] by the
    rounding of a product, a quotient and a sum, each at most one ulp of a value no larger than the polygon's x-extent or magnitude.
    2^-50 of that is > 4 ulp; a wider box only culls less."""
    if len(v) == 0:
        return (0.0, 0.0, -1.0, -1.0)                              # nothing lies inside
    xmin, ymin = v.min(0)
    xmax, ymax = v.max(0)
    pad = 0.0 if K.pip_exact_ok(v) else max(abs(xmin), abs(xmax), xmax - xmin) * 2.0 ** -50
    return (xmin - pad, ymin, xmax + pad, ymax)


class Annotation:
    """The polygons of one slide (util.py:212-279): ``from_json`` / ``inside_polygons`` / ``polygon_vertices`` / ``__str__`` as the
    reference's, on the host.  ``from_vertices`` builds one from two lists of [n, 2] arrays.  ``to_device`` and the three device
    queries are this package's."""

    def __init__(self):
        self._json_path = ''
        self._polygons_positive = []
        self._polygons_negative = []
        self._changed()

    def __str__(self):
        return self._json_path

    def _changed(self):
        self._packed, self._device, self._current = {}, {}, None

    def from_json(self, json_path):
        """the reference's JSON layout: {"positive": [{"name": ..., "vertices": [[x, y], ...]}, ...], "negative": [...]}"""
        self._json_path = json_path
        with open(json_path) as f:
            doc = json.load(f)
        for key, polygons in (("positive", self._polygons_positive), ("negative", self._polygons_negative)):
            for entry in doc[key]:
                polygons.append(Polygon(entry["name"], np.array(entry["vertices"])))
        self._changed()
        return self

    def from_vertices(self, positive, negative=()):
        """two sequences of [n, 2] vertex arrays; the polygons are named by their position"""
        for key, arrays, polygons in (("positive", positive, self._polygons_positive), ("negative", negative, self._polygons_negative)):
            for v in arrays:
                polygons.append(Polygon(f"{key}_{len(polygons)}", np.array(v)))
        self._changed()
        return self

    def _polygons(self, is_positive):
        return self._polygons_positive if is_positive else self._polygons_negative

    def inside_polygons(self, coord, is_positive):
        """True at the first polygon of the chosen list that contains ``coord`` = (x, y), else False"""
        for polygon in self._polygons(is_positive):
            if polygon.inside(coord):
                return True
        return False

    def polygon_vertices(self, is_positive):
        return [p.vertices() for p in self._polygons(is_positive)]

    # ---- the device side
    def packed(self, is_positive=True):
        """-> (vertices float64 [V, 2], offsets int32 [P + 1], bounds float64 [P, 4], exact): one list as the kernel reads it, and
        whether every vertex meets the integer path's precondition.  Computed once."""
        key = bool(is_positive)
        if key not in self._packed:
            vs = [_as_xy(p._vertices) for p in self._polygons(key)]
            offsets = np.zeros(len(vs) + 1, dtype=np.int64)
            offsets[1:] = np.cumsum([len(v) for v in vs])
            if offsets[-1] >= 1 << 31:
                raise ValueError("Annotation: the vertex count does not fit int32")
            vertices = np.concatenate(vs) if vs else np.zeros((0, 2), dtype=np.float64)
            bounds = np.array([polygon_bounds(v) for v in vs], dtype=np.float64).reshape(len(vs), 4)
            self._packed[key] = (np.ascontiguousarray(vertices), offsets.astype(np.int32), bounds, K.pip_exact_ok(vertices))
        return self._packed[key]

    def to_device(self, device=None):
        """uploads vertices, offsets and bounds of both lists, once per device -> self"""
        dev = torch.device(device if device is not None else "cuda")
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        if dev not in self._device:
            self._device[dev] = {key: tuple(torch.from_numpy(a).to(dev) for a in self.packed(key)[:3]) + (self.packed(key)[3],)
                                 for key in (True, False)}
        self._current = dev
        return self

    def _on_device(self, is_positive):
        if not self._device:
            self.to_device()
        return self._device[self._current][bool(is_positive)]

    def inside(self, points, is_positive=True, first=False):
        """points: [n, 2] (x, y), host (anything ``np.asarray`` takes) or a device tensor -> device uint8 [n], 1 where a polygon of the
        list contains the point; first=True: ``(inside, first)`` with the int32 index of the first containing polygon, or -1.  Host
        points are checked for the integer path here and uploaded; a device tensor is checked on the device (one sync)."""
        vertices, offsets, bounds, vexact = self._on_device(is_positive)
        if torch.is_tensor(points) and points.is_cuda:
            pts = points.to(vertices.device, torch.float64).contiguous()
            exact = vexact and K.pip_exact_ok(pts)
        else:
            host = np.ascontiguousarray(np.asarray(points.cpu() if torch.is_tensor(points) else points, dtype=np.float64).reshape(-1, 2))
            exact = vexact and K.pip_exact_ok(host)
            pts = torch.from_numpy(host).to(vertices.device)
        return K.points_in_polygons(pts, vertices, offsets, bounds=bounds, first=first, exact=exact)

    def labels(self, centres):
        """-> device int64 [n]: ``1 if inside_polygons((x_center, y_center), True) else 0`` for every centre"""
        return self.inside(centres, True).to(torch.int64)

    def mask(self, mask_shape, resolution, is_positive=True):
        """-> device uint8 [X_mask, Y_mask]: cell [x_mask, y_mask] is ``inside_polygons((int(x_mask * resolution), int(y_mask *
        resolution)), is_positive)`` (dataset.py:985-988).  An integer resolution is the kernel's grid source: no coordinate is
        uploaded.  Any other resolution evaluates the two expressions on the host per row and column and uploads the centres."""
        X, Y = (int(v) for v in mask_shape)
        vertices, offsets, bounds, vexact = self._on_device(is_positive)
        if float(resolution) == int(resolution) and int(resolution) >= 0:
            grid = (0, 0, int(resolution), X, Y)
            exact = vexact and K.pip_exact_ok(K._grid_extremes(grid))
            return K.points_in_polygons(None, vertices, offsets, grid=grid, bounds=bounds, exact=exact)
        xs = np.trunc(np.arange(X) * float(resolution))             # int(x_mask * resolution)
        ys = np.trunc(np.arange(Y) * float(resolution))
        centres = np.stack([np.repeat(xs, Y), np.tile(ys, X)], 1)
        return self.inside(centres, is_positive).view(X, Y)


class CentreListLoader:
    """``DataLoader(DatasetCamelyon16_eval(...))`` (dataset.py:871-939) over ONE slide whose region sits in HBM: batches ``(uint8
    [b, 3, S, S], int64 [b])`` in the order of ``centres``, the last one short.  region_u8_hwc: host or device uint8 [RH, RW, 3],
    uploaded once; centres: [n, 2] level-0 (x_center, y_center) integers; annotation: the slide's ``Annotation``; origin: level-0 (x, y)
    of ``region[0, 0]``; fill: what a tile holds outside the region.  A tile's corner is ``int(centre - image_size / 2)``, the
    expression ``inference.tile_origins`` uses; the labels are ``annotation.labels(centres)``, computed once.  No new kernel: one
    ``inference.gather_tiles`` launch per batch."""

    def __init__(self, region_u8_hwc, centres, annotation, image_size, batch_size, *, origin=(0, 0), fill=0, device=None):
        region = torch.as_tensor(region_u8_hwc)
        if region.dtype != torch.uint8 or region.dim() != 3 or region.shape[2] != 3:
            raise ValueError("CentreListLoader: a uint8 region [RH, RW, 3] expected")
        if int(batch_size) < 1 or int(image_size) < 1:
            raise ValueError("CentreListLoader: batch_size and image_size must be positive")
        centres = np.asarray(centres)
        if centres.size == 0:
            centres = centres.reshape(0, 2)
        if centres.ndim != 2 or centres.shape[1] != 2 or not np.issubdtype(centres.dtype, np.integer):
            raise ValueError("CentreListLoader: centres must be an integer array [n, 2] of (x_center, y_center)")
        xy = np.trunc(centres.astype(np.float64) - int(image_size) / 2).astype(np.int64)
        if len(xy) and (xy.min() < -(1 << 31) or xy.max() >= 1 << 31):
            raise ValueError("CentreListLoader: a tile coordinate does not fit int32")
        if not region.is_cuda:
            region = region.to(torch.device(device if device is not None else "cuda"), non_blocking=True)
        self.region = region.contiguous()
        self.image_size, self.batch_size = int(image_size), int(batch_size)
        self.origin, self.fill = (int(origin[0]), int(origin[1])), int(fill)
        self.centres = centres
        self.xy = torch.from_numpy(xy.astype(np.int32)).to(self.region.device)
        self.targets = annotation.to_device(self.region.device).labels(centres)

    def samples(self):
        return len(self.centres)

    def __len__(self):
        return (self.samples() + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        from .inference import gather_tiles
        n = self.samples()
        for lo in range(0, n, self.batch_size):
            hi = min(lo + self.batch_size, n)
            yield gather_tiles(self.region, self.xy[lo:hi], self.image_size, origin=self.origin, fill=self.fill), self.targets[lo:hi]
