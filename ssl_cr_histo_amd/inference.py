"""Device-resident test-time inference: WSI tiling from a slide region held in HBM, and classification metrics from an integer
confusion matrix counted on the device.

WSI (row f3).  The reference's ``DatasetCamelyon16_test`` (dataset.py:943-996) makes one ``read_region`` per tissue pixel of the mask and
hands a float32 tile to the loader; neighbouring tiles overlap by (1 - resolution / image_size) of their area.  ``WsiDeviceLoader``
uploads the region's uint8 bytes once, computes the tile coordinates with the reference's own expressions (``tile_origins``) and cuts
every batch on the device (``gather_tiles`` -> sslcr_wsi_gather); ``steps.camelyon16_test`` recognises it and keeps the probability map
on the device until one copy at the end.  openslide / h5 I/O is not part of this package: the caller reads the region (for instance
``np.asarray(slide.read_region((ox, oy), 0, (w, h)).convert('RGB'))``) and passes ``origin=(ox, oy)``.  What a tile that leaves the
region holds is the caller's statement (``fill``): openslide returns transparent pixels there, ``.convert('RGB')`` makes them black, which
is the default 0 -- unpinned against openslide itself.

Test-time augmentation.  ``d4_codes`` / ``d4_apply`` define the eight flips and quarter turns of a square tile (the dihedral group
D4) as orientation codes 0..7; ``WsiDeviceLoader.tiles(lo, hi, orient=g)`` cuts a batch already oriented (sslcr_wsi_gather_d4), and
``args.tta`` on the ``steps.*_test`` functions averages the scores of the listed orientations on the device (sslcr_predict_tta).

Ground truth.  ``WsiDeviceLoader(..., annotation=)`` takes the slide's ``annotation.Annotation``: the tiles' labels (``.targets``) and
the truth mask (``.truth``) are two launches of sslcr_points_in_polygons at construction, ``camelyon16_test`` counts the tile-level
confusion matrix in the predict launch it already makes, and ``map_scores`` counts a finished map against the truth mask at up to 64
thresholds in one pass (sslcr_map_confusion).

Lesion-level FROC.  ``lesion_scores`` takes the map and the truth mask to what the Camelyon16 metric counts -- the truth's connected
lesions, the map's non-maximum suppression into detections, the lesion under each detection (csrc/froc.hip) -- and ``froc`` /
``FrocMeter`` turn the slides' false-positive and per-lesion probabilities into the curve and the score in host float64.
``evaluation_mask`` makes the challenge's evaluation mask from the truth mask on the device -- the 75 um dilation by an exact squared
distance transform, the hole filling, the lesions' labels and moments (csrc/evalmask.hip) -- and the isolated-tumour-cell list from
the major axis lengths; ``lesion_scores(..., evaluation=)`` scores against it.

Patch loaders.  The BreastPathQ validation and test loops resize every patch with Pillow on the host (``transforms.Resize``);
``PatchDeviceLoader`` holds the patches in HBM and resizes each batch on the device with Pillow's own bytes (``kernels.pil_resize``,
csrc/resample.hip), yielding the host loader's batches.

Ranking metrics.  The Kather main also prints ``roc_auc_score(targets, scores, multi_class='ovr')`` (eval_Kather_SSL_CR.py:658).
``roc_auc`` counts every column's correctly ordered (positive, negative) pairs exactly on the device -- one radix sort per column, all
columns in one call, ties resolved over runs of equal scores (csrc/rank.hip) -- and divides once on the host; ``map_auc`` is the same
over the tissue cells of a probability map, ``AucMeter`` the batch-by-batch form.  ``icc`` / ``bpq_icc`` are the intraclass correlation
tables the BreastPathQ mains print (eval_BreastPathQ_SSL_CR.py:570-599), in host float64: their input is already on the host.

Metrics.  The Kather mains build sklearn's confusion matrix and a weighted F1 from what ``test()`` returns
(eval_Kather_SSL_CR.py:646-658, eval_Kather_SSL.py:519-530).  ``ConfusionMeter`` counts the same matrix on the device, batch by batch,
with integer atomics; ``metrics_from_confusion`` derives the figures from it in host float64.
"""
import numpy as np
import torch

from . import kernels as K


def tile_origins(mask, resolution, image_size):
    """-> (x_idcs, y_idcs, xy int32 [n, 2]): the tissue pixels of ``mask`` in ``np.where(mask)`` order (dataset.py:978) and the level-0
    (left, top) of their tiles, ``int(int(x_mask * resolution) - image_size / 2)`` (dataset.py:987-991).  ``int()`` truncates toward
    zero: ``int(0 * 64 - 224 / 2) == -112``, ``int(0 * 64 - 255 / 2) == -127``."""
    x_idcs, y_idcs = np.where(np.asarray(mask))
    half = image_size / 2
    xy = np.empty((len(x_idcs), 2), dtype=np.int64)
    for k, idcs in enumerate((x_idcs, y_idcs)):
        centre = np.trunc(idcs * resolution)                       # int(x_mask * resolution); exact in float64 at slide magnitudes
        xy[:, k] = np.trunc(centre - half).astype(np.int64)        # int(x_center - image_size / 2)
    if len(xy) and (xy.min() < -(1 << 31) or xy.max() >= 1 << 31):
        raise ValueError("tile_origins: a tile coordinate does not fit int32")
    return x_idcs, y_idcs, xy.astype(np.int32)


def gather_tiles(region_u8_hwc, xy, size, *, origin=(0, 0), fill=0, out=None):
    """uint8 NCHW tiles [N, 3, size, size] from a device-resident uint8 region [RH, RW, 3]: ``kernels.wsi_gather``.  xy: device int32
    [N, 2] level-0 (left, top); origin: level-0 coordinates of ``region[0, 0]``; fill: the value of pixels outside the region."""
    return K.wsi_gather(region_u8_hwc, xy, size, origin=origin, fill=fill, out=out)


# ---- test-time augmentation over D4: the orientation codes of include/sslcr.h
D4_SETS = {"d4": (0, 1, 2, 3, 4, 5, 6, 7),       # every flip and quarter turn
           "rot90": (0, 1, 2, 3),                # the four quarter turns
           "flips": (0, 4, 6)}                   # identity, horizontal flip, vertical flip (h-flip then a half turn)


def d4_codes(spec):
    """a name of ``D4_SETS`` or a sequence of codes -> the validated tuple of DISTINCT codes in 0..7, in the order given (the order
    the ensemble is summed in).  ValueError for an unknown name, an empty sequence, a duplicate or a code outside 0..7."""
    if isinstance(spec, str):
        if spec not in D4_SETS:
            raise ValueError(f"d4_codes: unknown set {spec!r} (known: {sorted(D4_SETS)})")
        return D4_SETS[spec]
    try:
        raw = list(spec)
    except TypeError:
        raise ValueError(f"d4_codes: a set name or a sequence of codes expected, got {spec!r}") from None
    codes = []
    for g in raw:
        if isinstance(g, bool) or not isinstance(g, (int, np.integer)) or not 0 <= int(g) <= 7:
            raise ValueError(f"d4_codes: {g!r} is not an orientation code in 0..7")
        codes.append(int(g))
    if not codes:
        raise ValueError("d4_codes: no orientation given")
    if len(set(codes)) != len(codes):
        raise ValueError(f"d4_codes: duplicate codes in {tuple(codes)}")
    return tuple(codes)


def d4_apply(array, g):
    """orientation ``g`` of square tiles ``array[..., S, S]`` (numpy, or anything ``np.asarray`` takes): a horizontal flip if
    ``g >> 2``, THEN ``g & 3`` counter-clockwise quarter turns -- the host restatement of sslcr_d4_transform / sslcr_wsi_gather_d4."""
    t = np.asarray(array)
    if not 0 <= int(g) <= 7:
        raise ValueError(f"d4_apply: {g!r} is not an orientation code in 0..7")
    if t.ndim < 2 or t.shape[-1] != t.shape[-2]:
        raise ValueError(f"d4_apply: square tiles [..., S, S] expected, got {t.shape}")
    return np.ascontiguousarray(np.rot90(t[..., ::-1] if int(g) >> 2 else t, int(g) & 3, axes=(-2, -1)))


def default_resolution(slide_wh, mask_shape):
    """the reference's ``round(X_slide / X_mask)`` with its two checks (dataset.py:963-975); the mask is indexed [x, y]"""
    X_slide, Y_slide = slide_wh
    X_mask, Y_mask = mask_shape
    if round(X_slide / X_mask) != round(Y_slide / Y_mask):
        raise Exception('Slide/Mask dimension does not match , X_slide / X_mask : {} / {}, Y_slide / Y_mask : {} / {}'
                        .format(X_slide, X_mask, Y_slide, Y_mask))
    resolution = round(X_slide * 1.0 / X_mask)
    if not np.log2(resolution).is_integer():
        raise Exception('Resolution (X_slide / X_mask) is not power of 2 : {}'.format(resolution))
    return resolution


class _WsiDataset:
    def __init__(self, mask, x_idcs, y_idcs, resolution, image_size):
        self.mask, self.X_idcs, self.Y_idcs, self.resolution, self.image_size = mask, x_idcs, y_idcs, resolution, image_size

    def __len__(self):
        return len(self.X_idcs)


class WsiDeviceLoader:
    """The loader of ``test_Camelyon16.test`` with the slide region in HBM.  region_u8_hwc: host (numpy / torch) or device uint8
    [RH, RW, 3], uploaded once; mask: the tissue mask, indexed [x, y] as the reference's (transposed against the image); resolution:
    level-0 pixels per mask pixel, default ``round(RW / mask.shape[0])`` under the reference's two checks; origin: level-0 (x, y) of
    ``region[0, 0]``; fill: what a tile holds outside the region.  ``.dataset.mask`` and ``len()`` (batches) as the reference loader.
    The coordinate table and the flat map indices are computed and uploaded once; iterating yields the reference's
    ``(tiles, x_mask, y_mask)`` batches with the tiles as device uint8, so any consumer of the host loader can read it too."""

    def __init__(self, region_u8_hwc, mask, image_size, batch_size, *, resolution=None, origin=(0, 0), fill=0, device=None,
                 annotation=None):
        mask = np.asarray(mask)
        if mask.ndim != 2:
            raise ValueError("WsiDeviceLoader: a 2-D tissue mask expected")
        region = torch.as_tensor(region_u8_hwc)
        if region.dtype != torch.uint8 or region.dim() != 3 or region.shape[2] != 3:
            raise ValueError("WsiDeviceLoader: a uint8 region [RH, RW, 3] expected")
        if int(batch_size) < 1 or int(image_size) < 1:
            raise ValueError("WsiDeviceLoader: batch_size and image_size must be positive")
        if resolution is None:
            resolution = default_resolution((region.shape[1], region.shape[0]), mask.shape)
        x_idcs, y_idcs, xy = tile_origins(mask, resolution, image_size)
        if not region.is_cuda:
            region = region.to(torch.device(device if device is not None else "cuda"), non_blocking=True)
        self.region = region.contiguous()
        self.image_size, self.batch_size, self.origin, self.fill = int(image_size), int(batch_size), (int(origin[0]), int(origin[1])), int(fill)
        self.dataset = _WsiDataset(mask, x_idcs, y_idcs, resolution, self.image_size)
        self.x_mask, self.y_mask = torch.from_numpy(x_idcs.copy()), torch.from_numpy(y_idcs.copy())
        dev = self.region.device
        self._orient = None
        self.xy = torch.from_numpy(xy).to(dev)
        self.map_index = torch.from_numpy(x_idcs.astype(np.int64) * mask.shape[1] + y_idcs).to(dev)     # probs_map[x, y], row-major
        self.annotation, self.targets, self.truth = annotation, None, None
        if annotation is not None:                                 # two launches, no host loop: the tiles' labels and the truth mask
            annotation.to_device(dev)
            centres = np.stack([np.trunc(x_idcs * resolution), np.trunc(y_idcs * resolution)], 1)      # tile_origins' centres
            self.targets = annotation.labels(centres)
            self.truth = annotation.mask(mask.shape, resolution)

    def __len__(self):
        return (len(self.dataset) + self.batch_size - 1) // self.batch_size

    def ranges(self):
        n = len(self.dataset)
        return [(lo, min(lo + self.batch_size, n)) for lo in range(0, n, self.batch_size)]

    def tiles(self, lo, hi, out=None, orient=None):
        """tiles lo..hi of the table; orient: None (the plain gather), or ONE D4 code for the whole range (``d4_apply``)"""
        if orient is None:
            return gather_tiles(self.region, self.xy[lo:hi], self.image_size, origin=self.origin, fill=self.fill, out=out)
        (g,) = d4_codes((orient,))
        if self._orient is None:                                   # [8, batch_size] int32, row g = g: uploaded once
            self._orient = torch.arange(8, dtype=torch.int32).repeat_interleave(self.batch_size).view(8, -1).to(self.region.device)
        table = self._orient[g, :hi - lo] if hi - lo <= self.batch_size else torch.full((hi - lo,), g, dtype=torch.int32,
                                                                                      device=self.region.device)
        return K.wsi_gather(self.region, self.xy[lo:hi], self.image_size, origin=self.origin, fill=self.fill, out=out, orient=table)

    def __iter__(self):
        for lo, hi in self.ranges():
            yield self.tiles(lo, hi), self.x_mask[lo:hi], self.y_mask[lo:hi]


class _PatchDataset:
    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n


class PatchDeviceLoader:
    """The evaluation loader of the patch datasets with the patches in HBM: ``DataLoader(DatasetBreastPathQ_eval(...,
    transforms.Resize(size=image_size)), shuffle=False)`` (eval_BreastPathQ_SSL_CR.py:325,365, eval_BreastPathQ_SSL.py:290,319,
    dataset.py:575-599) without the host's one-image-at-a-time Pillow resize.  patches_u8: ONE uint8 array [M, H, W, 3]
    (layout='hwc', what the datasets hold) or [M, 3, H, W] ('chw'), host or device; it is uploaded once, at the first batch.
    targets: any number of arrays of M rows, handed through in slices (host tensors, as a DataLoader collates them).  image_size: an
    int or (h, w), ``kernels.resize_output_size``'s rule.  Iterating yields ``(tiles, *target slices)`` with tiles a device uint8
    [n, 3, oh, ow] -- ``PIL.Image.resize((ow, oh), resample)`` of every patch (``kernels.pil_resize``), channels first -- in order,
    the last batch short: the batch contract of the host loader, so ``steps.bpq_test``, ``bpq_sup_test``, ``bpq_cr_validate``,
    ``kather_cr_test`` and the other loops take it unchanged (they pass device uint8 batches through ``Engine.as_input``).  Patches
    of unequal shape are out of scope."""

    def __init__(self, patches_u8, *targets, image_size, batch_size, resample="bilinear", layout="hwc", device=None):
        patches = torch.as_tensor(patches_u8)
        if layout not in ("hwc", "chw"):
            raise ValueError(f"PatchDeviceLoader: layout = {layout!r} ('hwc' or 'chw')")
        if patches.dtype != torch.uint8 or patches.dim() != 4 or patches.shape[3 if layout == "hwc" else 1] != 3:
            raise ValueError("PatchDeviceLoader: a uint8 array [M, H, W, 3] (layout='hwc') or [M, 3, H, W] ('chw') expected")
        if isinstance(batch_size, bool) or int(batch_size) < 1:
            raise ValueError("PatchDeviceLoader: batch_size must be positive")
        M = patches.shape[0]
        H, W = (patches.shape[1], patches.shape[2]) if layout == "hwc" else (patches.shape[2], patches.shape[3])
        self.targets = [torch.as_tensor(t) for t in targets]
        for t in self.targets:
            if t.dim() < 1 or t.shape[0] != M:
                raise ValueError(f"PatchDeviceLoader: every target needs {M} rows, one per patch")
        K.resample_filter_code(resample)                                   # ValueError for an unknown filter, here and not at the first batch
        self.out_hw = K.resize_output_size(H, W, image_size)
        self.patches, self.layout, self.resample, self.batch_size = patches, layout, resample, int(batch_size)
        self.device = torch.device(device if device is not None else (patches.device if patches.is_cuda else "cuda"))
        self.dataset = _PatchDataset(M)

    def __len__(self):
        return (len(self.dataset) + self.batch_size - 1) // self.batch_size

    def ranges(self):
        n = len(self.dataset)
        return [(lo, min(lo + self.batch_size, n)) for lo in range(0, n, self.batch_size)]

    def tiles(self, lo, hi, out=None):
        """patches lo..hi resized: device uint8 [hi - lo, 3, oh, ow]"""
        if not self.patches.is_cuda or not self.patches.is_contiguous():      # the one upload
            self.patches = self.patches.to(self.device).contiguous()
        oh, ow = self.out_hw
        return K.pil_resize(self.patches[lo:hi], (ow, oh), self.resample, layout=self.layout, out_layout="chw", out=out)

    def __iter__(self):
        for lo, hi in self.ranges():
            yield (self.tiles(lo, hi),) + tuple(t[lo:hi] for t in self.targets)


class ConfusionMeter:
    """int64 [C, C] confusion matrix on the device, rows = targets, columns = predictions (sklearn's ``confusion_matrix`` layout);
    ``update(logits, target)`` adds one batch (argmax of fp32 logits [n, C]; rows with a target outside [0, C) are skipped) without a
    sync; ``cpu()`` is the one copy."""

    def __init__(self, C, device):
        if not 1 <= int(C) <= 64:
            raise ValueError(f"ConfusionMeter: C = {C} outside [1, 64]")
        self.C = int(C)
        self.matrix = torch.zeros((self.C, self.C), dtype=torch.int64, device=device)

    def update(self, logits, target):
        K.predict(logits, target, pred=False, confusion=self.matrix)
        return self

    def reset(self):
        self.matrix.zero_()

    def cpu(self):
        return self.matrix.cpu()


def map_scores(probs_map, truth, tissue, thresholds):
    """A probability map against the truth mask over the tissue cells, at every threshold: one device pass for the counts
    (``kernels.map_confusion``), one copy, host float64 for the figures.  probs_map: [X, Y], a device float32 tensor or what
    ``camelyon16_test`` returns (uploaded as float32, the precision it was computed in); truth / tissue: [X, Y] masks, device uint8 or
    host (``WsiDeviceLoader.truth`` / ``.dataset.mask``); thresholds: 1 <= T <= 64 values, compared as float32.
    -> dict: ``thresholds`` (float32 [T]), ``confusion`` int64 [T, 2, 2] = [t, truth, map >= threshold] ([[tn, fp], [fn, tp]]),
    ``sensitivity`` = tp / (tp + fn), ``specificity`` = tn / (tn + fp), ``dice`` = 2 tp / (2 tp + fp + fn); a division by zero gives 0."""
    dev = next((t.device for t in (probs_map, truth, tissue) if torch.is_tensor(t) and t.is_cuda), None)
    dev = dev if dev is not None else torch.device("cuda")
    pm = torch.as_tensor(probs_map).to(dev, torch.float32).contiguous()
    masks = [torch.as_tensor(np.asarray(m) != 0 if not torch.is_tensor(m) else m).to(dev).contiguous() for m in (truth, tissue)]
    thr = np.asarray(torch.as_tensor(thresholds).cpu(), dtype=np.float32).reshape(-1)
    cm = K.map_confusion(pm, masks[0], masks[1], torch.from_numpy(thr)).cpu().numpy()
    tn, fp, fn, tp = cm[:, 0, 0], cm[:, 0, 1], cm[:, 1, 0], cm[:, 1, 1]
    return dict(thresholds=thr, confusion=cm, sensitivity=_div(tp, tp + fn), specificity=_div(tn, tn + fp),
                dice=_div(2 * tp, 2 * tp + fp + fn))


def _div(a, b):
    """a / b with 0 where b == 0 (sklearn's zero_division default value)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.divide(a, b, out=np.zeros(np.broadcast(a, b).shape, dtype=np.float64), where=b != 0)


def major_axis_lengths(moments):
    """``regionprops``' ``major_axis_length`` of every component, in cells, from its raw moments, in host float64.  moments: [L, 6]
    integers (area A, sum x, sum y, sum x^2, sum y^2, sum x y), what ``kernels.region_moments`` returns.  The central second moments
    over the area, a = (A sum x^2 - (sum x)^2) / A^2, c = (A sum y^2 - (sum y)^2) / A^2, b = (A sum x y - sum x sum y) / A^2, have
    exact Python-int numerators and are rounded once each; l1 = (a + c) / 2 + sqrt(((a - c) / 2)^2 + b^2) is the larger eigenvalue
    of the inertia tensor and the result is 4 sqrt(l1).  A row with A == 0 gives nan.  -> float64 [L]."""
    import math
    rows = np.asarray(torch.as_tensor(moments).cpu()).reshape(-1, 6).tolist()
    out = np.full(len(rows), np.nan, dtype=np.float64)
    for i, (A, sx, sy, sxx, syy, sxy) in enumerate(rows):
        A, sx, sy, sxx, syy, sxy = int(A), int(sx), int(sy), int(sxx), int(syy), int(sxy)
        if A <= 0:
            continue
        a, c, b = (A * sxx - sx * sx) / (A * A), (A * syy - sy * sy) / (A * A), (A * sxy - sx * sy) / (A * A)
        half = (a - c) / 2.0
        out[i] = 4.0 * math.sqrt((a + c) / 2.0 + math.sqrt(half * half + b * b))
    return out


def evaluation_mask(truth, *, cell_um, dilate_um=75.0, itc_um=275.0, connectivity=2, device=None):
    """The Camelyon16 challenge's evaluation mask and ITC list from a truth mask, on the device (include/sslcr.h has the definitions;
    parity with the challenge's script is unpinned, the integer steps are pinned against scipy):
    ``kernels.distance_transform_sq`` to the nearest truth cell, the cells with distance < ``dilate_um / (2 cell_um)`` (as an integer
    limit on the squared distance, ``kernels.distance_limit``), ``kernels.fill_holes``, ``kernels.label_components(connectivity)``,
    ``kernels.region_moments``; then ``major_axis_lengths`` on the host.  truth: [X, Y], a device uint8 / bool tensor or a host array
    (``WsiDeviceLoader.truth``); cell_um: microns per map cell, e.g. 0.243 * 64; device: where to work (default: truth's, else cuda).
    Host traffic: one read of L, one copy of the moments.
    -> dict: ``mask`` device uint8 [X, Y] (the filled dilation), ``labels`` device int32 [X, Y], ``n_lesions`` = L, ``moments`` int64
    [L, 6], ``major_axis`` float64 [L] in cells, ``itc`` = the sorted 1-based labels with ``major_axis < itc_um / cell_um``, ``limit``."""
    cell_um = float(cell_um)
    if not cell_um > 0:
        raise ValueError(f"evaluation_mask: cell_um = {cell_um}")
    if device is None:
        device = truth.device if torch.is_tensor(truth) and truth.is_cuda else torch.device("cuda")
    tr = torch.as_tensor(np.asarray(truth) != 0 if not torch.is_tensor(truth) else truth).to(device).contiguous()
    if tr.dtype != torch.bool and tr.dtype != torch.uint8:
        tr = tr != 0
    limit = K.distance_limit(float(dilate_um) / (cell_um * 2.0))
    _, binary = K.distance_transform_sq(tr, limit, invert=True, below=True)
    mask = K.fill_holes(binary)
    labels, count = K.label_components(mask, connectivity)
    n_lesions = int(count.item())
    moments = K.region_moments(labels, n_lesions).cpu().numpy().astype(np.int64).reshape(n_lesions, 6)
    major = major_axis_lengths(moments)
    itc = np.flatnonzero(major < float(itc_um) / cell_um).astype(np.int64) + 1
    return dict(mask=mask, labels=labels, n_lesions=n_lesions, moments=moments, major_axis=major, itc=itc, limit=limit)


def lesion_scores(probs_map, truth, *, threshold=0.5, radius=12, sigma=0.0, connectivity=2, ignore=None, max_detections=4096,
                  evaluation=None):
    """A probability map against the LESIONS of the truth mask, what lesion-level FROC counts (include/sslcr.h has the definitions):
    the connected components of ``truth`` (``kernels.label_components``), the optional float32 Gaussian of the map
    (``kernels.gaussian_smooth``), its greedy non-maximum suppression into a detection list (``kernels.nms``) and the hit test
    (``kernels.lesion_hits``), all on the device.  probs_map / truth: as for ``map_scores``; ignore: lesion labels (1-based) whose hits
    are neither false nor true positives (the challenge treats isolated tumour cells so; ``areas`` of a first call tells the sizes).
    Host traffic: one read of L, the reads ``kernels.nms`` documents, one copy of the small results.
    -> dict: ``detections`` float64 [K, 3] (x, y, prob) in NMS order, ``hit`` int32 [K] (the label under each, 0 = none), ``fp_prob``
    float64 = the probabilities of the detections with hit 0, ``tp_prob`` float64 [L] = the best probability on each lesion (0 where
    nothing hit it or it is ignored), ``areas`` int64 [L], ``n_lesions`` = L, ``ignore`` = the sorted labels ignored.
    evaluation: the dict ``evaluation_mask`` returns.  The map is then scored against ITS ``labels`` / ``n_lesions`` (the challenge's
    dilated, hole-filled lesions) without labelling anything again, ``ignore`` defaults to its ``itc`` list, and ``truth`` /
    ``connectivity`` are not used (``truth`` may be None)."""
    if evaluation is not None:
        labels, n_lesions = evaluation["labels"], int(evaluation["n_lesions"])
        pm = torch.as_tensor(probs_map).to(labels.device, torch.float32).contiguous()
        if labels.shape != pm.shape:
            raise ValueError(f"lesion_scores: map {tuple(pm.shape)} and evaluation labels {tuple(labels.shape)} differ in shape")
        ign = np.unique(np.asarray(list(ignore if ignore is not None else evaluation["itc"]), dtype=np.int64))
        det_xy, det_prob, k = K.nms(K.gaussian_smooth(pm, float(sigma)), threshold, radius, max_detections)
    else:
        dev = next((t.device for t in (probs_map, truth) if torch.is_tensor(t) and t.is_cuda), None)
        dev = dev if dev is not None else torch.device("cuda")
        pm = torch.as_tensor(probs_map).to(dev, torch.float32).contiguous()
        tr = torch.as_tensor(np.asarray(truth) != 0 if not torch.is_tensor(truth) else truth).to(dev).contiguous()
        if tr.dtype != torch.bool and tr.dtype != torch.uint8:
            tr = tr != 0
        if tr.shape != pm.shape:
            raise ValueError(f"lesion_scores: map {tuple(pm.shape)} and truth {tuple(tr.shape)} differ in shape")
        ign = np.unique(np.asarray(list(ignore) if ignore is not None else [], dtype=np.int64))
        labels, count = K.label_components(tr, connectivity)
        det_xy, det_prob, k = K.nms(K.gaussian_smooth(pm, float(sigma)), threshold, radius, max_detections)
        n_lesions = int(count.item())
    hit, tp, areas = K.lesion_hits(labels, n_lesions, det_xy, det_prob, k, ignore=ign)
    small = torch.cat([det_xy[:k].reshape(-1).double(), det_prob[:k].double(), hit[:k].double(), tp.double(), areas.double()]).cpu().numpy()
    xy, prob, hit, tp, areas = np.split(small, np.cumsum([2 * k, k, k, n_lesions]))      # every value is exact in float64 (areas < 2^31)
    hit = hit.astype(np.int32)
    return dict(detections=np.concatenate([xy.reshape(k, 2), prob[:, None]], 1), hit=hit, fp_prob=prob[hit == 0], tp_prob=tp,
                areas=areas.astype(np.int64), n_lesions=n_lesions, ignore=ign)


def froc(fp_probs, tp_probs, n_slides, n_lesions, fps=(0.25, 0.5, 1, 2, 4, 8)):
    """Lesion-level FROC in host float64, after the Camelyon16 challenge's evaluation.  fp_probs: the false positives' probabilities
    over all scored slides; tp_probs: the best probability on every non-ignored lesion, zeros included; n_lesions: their number.
    Thresholds are ``sorted(set(fp) | set(tp))[1:]``; at each, the false positives and the lesions at or above it are counted, then
    (0, 0) is appended.  -> dict: ``thresholds``, ``avg_fp`` = FPs / n_slides, ``sensitivity`` = TPs / n_lesions (a division by zero
    gives 0), ``fps`` and ``score`` = the mean sensitivity at ``fps`` false positives per slide, linearly interpolated."""
    fp = np.asarray(fp_probs, dtype=np.float64).reshape(-1)
    tp = np.asarray(tp_probs, dtype=np.float64).reshape(-1)
    thr = np.unique(np.concatenate([fp, tp]))[1:]
    n_fp = np.append((fp[None, :] >= thr[:, None]).sum(1), 0)
    n_tp = np.append((tp[None, :] >= thr[:, None]).sum(1), 0)
    avg_fp, sens = _div(n_fp, float(n_slides)), _div(n_tp, float(n_lesions))
    fps = np.asarray(fps, dtype=np.float64)
    return dict(thresholds=thr, avg_fp=avg_fp, sensitivity=sens, fps=fps, score=float(np.mean(np.interp(fps, avg_fp[::-1], sens[::-1]))))


class FrocMeter:
    """``update(lesion_scores(...))`` slide by slide, ``result()`` = ``froc`` over what was collected (ignored lesions left out)."""

    def __init__(self, fps=(0.25, 0.5, 1, 2, 4, 8)):
        self.fps, self.fp, self.tp, self.n_slides = fps, [], [], 0

    def update(self, scores):
        keep = ~np.isin(np.arange(1, scores["n_lesions"] + 1), scores["ignore"])
        self.fp.append(np.asarray(scores["fp_prob"], dtype=np.float64))
        self.tp.append(np.asarray(scores["tp_prob"], dtype=np.float64)[keep])
        self.n_slides += 1

    def result(self):
        fp = np.concatenate(self.fp) if self.fp else np.zeros(0)
        tp = np.concatenate(self.tp) if self.tp else np.zeros(0)
        return froc(fp, tp, self.n_slides, len(tp), self.fps)


def metrics_from_confusion(cm):
    """host float64 figures of an integer confusion matrix [C, C] (rows = targets): dict with ``accuracy``, per-class ``precision`` /
    ``recall`` / ``f1`` / ``support`` (int64), ``weighted_f1`` (sklearn's ``f1_score(average='weighted')``) and ``multilabel`` [C, 2, 2]
    int64 = ``multilabel_confusion_matrix`` ([[tn, fp], [fn, tp]] per class).  A division by zero gives 0."""
    cm = np.asarray(cm.cpu() if torch.is_tensor(cm) else cm)
    if cm.ndim != 2 or cm.shape[0] != cm.shape[1] or not np.issubdtype(cm.dtype, np.integer):
        raise ValueError("metrics_from_confusion: a square integer matrix expected")
    cm = cm.astype(np.int64)
    total = cm.sum()
    tp = np.diag(cm)
    support = cm.sum(1)
    predicted = cm.sum(0)
    fp, fn = predicted - tp, support - tp
    tn = total - tp - fp - fn
    precision, recall = _div(tp, predicted), _div(tp, support)
    f1 = _div(2 * tp, 2 * tp + fp + fn)                           # = 2 p r / (p + r)
    return dict(accuracy=float(_div(tp.sum(), total)), precision=precision, recall=recall, f1=f1, support=support,
                weighted_f1=float(_div((f1 * support).sum(), support.sum())),
                multilabel=np.stack([np.stack([tn, fp], 1), np.stack([fn, tp], 1)], 1))


# ---- ranking metrics: exact ROC-AUC from device counts, intraclass correlation on the host
_ONE_CLASS = "Only one class present in y_true. ROC AUC score is not defined in that case."
_CLASS_COUNT = "Number of classes in y_true not equal to the number of columns in 'y_score'"


def auc_from_counts(counts, multi=False, average="macro"):
    """the host half of ``roc_auc``: integer counts [C, 4] = (U2, P, N, nan), what ``kernels.auc_counts`` returns, -> the figure, or
    sklearn's ValueError.  multi: the one-vs-rest reading of C columns (False: one binary column)."""
    rows = [[int(v) for v in r] for r in np.asarray(counts).reshape(-1, 4).tolist()]
    if any(r[3] for r in rows):
        raise ValueError("Input contains NaN.")
    if multi:
        # under one-vs-rest every valid element is a positive of exactly one column iff its target lies in range(C)
        if any(r[1] == 0 or r[2] == 0 for r in rows) or sum(r[1] for r in rows) != rows[0][1] + rows[0][2]:
            raise ValueError(_CLASS_COUNT)
    elif rows[0][1] == 0 or rows[0][2] == 0:
        raise ValueError(_ONE_CLASS)
    auc = np.array([u2 / (2 * p * n) for u2, p, n, _ in rows], dtype=np.float64)      # Python integers: one correctly rounded division
    if not multi:
        return float(auc[0])
    if average is None:
        return auc
    if average == "macro":
        return float(np.mean(auc))
    return float(np.average(auc, weights=np.array([r[1] for r in rows], dtype=np.float64)))


def _auc_device(*ts):
    dev = next((t.device for t in ts if torch.is_tensor(t) and t.is_cuda), None)
    return dev if dev is not None else torch.device("cuda")


def roc_auc(scores, target, *, multi_class="raise", average="macro", valid=None):
    """sklearn's ``roc_auc_score(target, scores, multi_class=, average=)`` from exact device counts: ``kernels.auc_counts`` (keys, one
    radix sort of all columns, the pair counts), ONE copy of the int64 [C, 4] counts, then per column ``U2 / (2 P N)`` as a Python
    integer true division -- the correctly rounded value of the exact area, where sklearn sums a trapezoid in float64 (the two differ
    by at most n 2^-53).  scores: [n] (or [n, 1]) scores class 1 against the rest, as sklearn's binary case does; [n, C], C >= 2, is
    multi-class and needs ``multi_class='ovr'``: column c scores class c, and ``average`` is 'macro' (``np.mean``), 'weighted'
    (``np.average`` with the class counts as weights) or None (the per-class float64 vector).  The rows are NOT checked to sum to 1
    (sklearn refuses such scores): they are sslcr_predict's softmax.  target: [n] integers; valid: [n] flags, zero = leave the element
    out (None = all in).  Device or host inputs: host ones are uploaded (scores as float32).
    ValueError, with sklearn's wording: a NaN score; a column without a positive or without a negative ('Only one class present': sklearn raised it up to 1.5 and
    warns and returns nan since; here it stays an error);
    multi-class scores without ``multi_class='ovr'``; under 'ovr', a class of range(C) absent from the targets or a target outside it."""
    dev = _auc_device(scores, target, valid)
    sc = torch.as_tensor(scores)
    if sc.dim() == 2 and sc.shape[1] == 1:
        sc = sc.reshape(-1)
    if sc.dim() not in (1, 2) or sc.numel() < 1:
        raise ValueError(f"roc_auc: scores [n] or [n, C] expected, got {tuple(sc.shape)}")
    multi = sc.dim() == 2
    if multi and multi_class != "ovr":
        if multi_class == "raise":
            raise ValueError("multi_class must be in ('ovo', 'ovr')")
        raise ValueError(f"roc_auc: multi_class = {multi_class!r}: only one-vs-rest ('ovr') is counted")
    if average not in ("macro", "weighted", None):
        raise ValueError(f"roc_auc: average = {average!r} outside ('macro', 'weighted', None)")
    sc = sc.to(dev, torch.float32)
    tg = torch.as_tensor(target)
    if tg.is_floating_point() or tg.dtype == torch.bool:
        tg = tg.to(torch.int64)
    tg = tg.reshape(-1).to(dev)
    if tg.numel() != sc.shape[0]:
        raise ValueError(f"roc_auc: {sc.shape[0]} scores and {tg.numel()} targets")
    if valid is not None:
        valid = torch.as_tensor(np.asarray(valid) != 0 if not torch.is_tensor(valid) else valid).reshape(-1).to(dev).contiguous()
        if valid.dtype not in (torch.bool, torch.uint8):
            valid = valid != 0
    counts = K.auc_counts(sc.contiguous(), tg.contiguous(), positive=None if multi else [1], valid=valid)
    return auc_from_counts(counts.cpu().numpy(), multi, average)


def map_auc(probs_map, truth, tissue):
    """The ROC-AUC of a probability map against the truth mask over the tissue cells, the sibling of ``map_scores``: every cell with
    ``tissue != 0`` is one sample, its score the map's float32 value, its class ``truth != 0``.  Inputs as for ``map_scores`` (device
    tensors, or host arrays that are uploaded; the map as float32).  One copy of four integers; ``roc_auc``'s errors."""
    dev = _auc_device(probs_map, truth, tissue)
    pm = torch.as_tensor(probs_map).to(dev, torch.float32).contiguous()
    masks = [torch.as_tensor(np.asarray(m) != 0 if not torch.is_tensor(m) else m).to(dev).contiguous() for m in (truth, tissue)]
    if masks[0].shape != pm.shape or masks[1].shape != pm.shape:
        raise ValueError(f"map_auc: map {tuple(pm.shape)}, truth {tuple(masks[0].shape)} and tissue {tuple(masks[1].shape)} differ in shape")
    return roc_auc(pm.reshape(-1), (masks[0].reshape(-1) != 0).to(torch.int64), valid=masks[1].reshape(-1) != 0)


class AucMeter:
    """The counterpart of ``ConfusionMeter`` for the ROC-AUC: ``update(scores, target)`` keeps one batch on the device (scores float32
    [n, C], or [n] for C = 1; the tensors are kept, not copied: hand it tensors nobody overwrites, as sslcr_predict's outputs are) without
    a sync; ``compute(**kw)`` is ``roc_auc`` over everything kept -- the area is not a sum over batches, so the sort happens here."""

    def __init__(self, C, device):
        if not 1 <= int(C) <= 65535:
            raise ValueError(f"AucMeter: C = {C} outside [1, 65535]")
        self.C, self.device = int(C), torch.device(device)
        self.reset()

    def update(self, scores, target):
        sc = torch.as_tensor(scores).to(self.device, torch.float32)
        sc = sc.reshape(-1) if self.C == 1 else sc
        if self.C > 1 and (sc.dim() != 2 or sc.shape[1] != self.C):
            raise ValueError(f"AucMeter: scores [n, {self.C}] expected, got {tuple(sc.shape)}")
        tg = torch.as_tensor(target).reshape(-1).to(self.device)
        if tg.numel() != sc.shape[0]:
            raise ValueError(f"AucMeter: {sc.shape[0]} scores and {tg.numel()} targets")
        self.scores.append(sc)
        self.targets.append(tg)
        return self

    def reset(self):
        self.scores, self.targets = [], []

    def compute(self, **kw):
        if not self.scores:
            raise ValueError("AucMeter: nothing to compute")
        return roc_auc(torch.cat(self.scores), torch.cat(self.targets), **kw)


ICC_TYPES = ("ICC1", "ICC2", "ICC3", "ICC1k", "ICC2k", "ICC3k")
ICC_DESCRIPTIONS = ("Single raters absolute", "Single random raters", "Single fixed raters", "Average raters absolute",
                    "Average random raters", "Average fixed raters")


def icc_mean_squares(ratings):
    """the mean squares of the two-way layout of ``ratings`` [n targets, k raters], float64, two-pass (sums of squared deviations from
    the means, never of raw squares) -> dict: ``n``, ``k``, ``MSR`` (between targets, n - 1), ``MSW`` (within targets, n (k - 1)),
    ``MSC`` (between raters, k - 1), ``MSE`` (residual, (n - 1)(k - 1))."""
    x = np.asarray(torch.as_tensor(ratings).cpu() if torch.is_tensor(ratings) else ratings, dtype=np.float64)
    if x.ndim != 2 or x.shape[0] < 2 or x.shape[1] < 2 or not np.isfinite(x).all():
        raise ValueError(f"icc: finite ratings [n >= 2 targets, k >= 2 raters] expected, got shape {x.shape}")
    n, k = x.shape
    grand, rows, cols = x.mean(), x.mean(1, keepdims=True), x.mean(0, keepdims=True)
    return dict(n=n, k=k, MSR=float(k * ((rows - grand) ** 2).sum() / (n - 1)), MSW=float(((x - rows) ** 2).sum() / (n * (k - 1))),
                MSC=float(n * ((cols - grand) ** 2).sum() / (k - 1)), MSE=float(((x - rows - cols + grand) ** 2).sum() / ((n - 1) * (k - 1))))


def icc(ratings):
    """The six intraclass correlations of Shrout & Fleiss (1979) for ``ratings`` [n targets, k raters] in host float64, no device code:
    from the two-way mean squares (``icc_mean_squares``),
        ICC1 = (MSR - MSW) / (MSR + (k - 1) MSW)                           ICC1k = (MSR - MSW) / MSR
        ICC2 = (MSR - MSE) / (MSR + (k - 1) MSE + k (MSC - MSE) / n)       ICC2k = (MSR - MSE) / (MSR + (MSC - MSE) / n)
        ICC3 = (MSR - MSE) / (MSR + (k - 1) MSE)                           ICC3k = (MSR - MSE) / MSR
    -> dict of arrays in the row order of ``pingouin.intraclass_corr``: ``Type``, ``Description``, ``ICC``, ``F`` (MSR / MSW for the
    two ICC1 rows, MSR / MSE for the others), ``df1`` = n - 1, ``df2`` (n (k - 1), resp. (n - 1)(k - 1)), ``pval`` (the F test's upper
    tail) and ``CI95`` [6, 2].  ``pval`` and ``CI95`` need ``scipy.stats``, imported here when it is there; NaN otherwise.
    PARITY UNPINNED against pingouin, which this project never had to compare against: pinned are the mean squares and the six
    values against a literal restatement and against Shrout & Fleiss's own table (tests/test_auc_cpu.py); ``CI95`` follows the
    confidence limits of Shrout & Fleiss / McGraw & Wong as pingouin states them, from memory of its source, and is pinned by nothing."""
    m = icc_mean_squares(ratings)
    n, k, MSR, MSW, MSC, MSE = m["n"], m["k"], m["MSR"], m["MSW"], m["MSC"], m["MSE"]
    with np.errstate(divide="ignore", invalid="ignore"):
        MSR_, MSW_, MSC_, MSE_ = (np.float64(v) for v in (MSR, MSW, MSC, MSE))
        values = np.array([(MSR_ - MSW_) / (MSR_ + (k - 1) * MSW_), (MSR_ - MSE_) / (MSR_ + (k - 1) * MSE_ + k * (MSC_ - MSE_) / n),
                           (MSR_ - MSE_) / (MSR_ + (k - 1) * MSE_), (MSR_ - MSW_) / MSR_, (MSR_ - MSE_) / (MSR_ + (MSC_ - MSE_) / n),
                           (MSR_ - MSE_) / MSR_], dtype=np.float64)
        f1, f3 = MSR_ / MSW_, MSR_ / MSE_
        F = np.array([f1, f3, f3, f1, f3, f3], dtype=np.float64)
        df1 = np.full(6, n - 1, dtype=np.int64)
        dfw, dfe = n * (k - 1), (n - 1) * (k - 1)
        df2 = np.array([dfw, dfe, dfe, dfw, dfe, dfe], dtype=np.int64)
        pval, ci = np.full(6, np.nan), np.full((6, 2), np.nan)
        try:
            from scipy.stats import f as fdist
        except ImportError:
            fdist = None
        if fdist is not None:
            pval = fdist.sf(F, df1, df2)
            q = 0.975
            f1l, f1u = f1 / fdist.ppf(q, n - 1, dfw), f1 * fdist.ppf(q, dfw, n - 1)
            f3l, f3u = f3 / fdist.ppf(q, n - 1, dfe), f3 * fdist.ppf(q, dfe, n - 1)
            icc2, fc = values[1], MSC_ / MSE_
            vn = dfe * (k * icc2 * fc + n * (1 + (k - 1) * icc2) - k * icc2) ** 2
            vd = (n - 1) * k ** 2 * icc2 ** 2 * fc ** 2 + (n * (1 + (k - 1) * icc2) - k * icc2) ** 2
            v = vn / vd
            f2u, f2l = fdist.ppf(q, n - 1, v), fdist.ppf(q, v, n - 1)
            l2 = n * (MSR_ - f2u * MSE_) / (f2u * (k * MSC_ + (k * n - k - n) * MSE_) + n * MSR_)
            u2 = n * (f2l * MSR_ - MSE_) / (k * MSC_ + (k * n - k - n) * MSE_ + n * f2l * MSR_)
            ci = np.array([[(f1l - 1) / (f1l + k - 1), (f1u - 1) / (f1u + k - 1)], [l2, u2],
                           [(f3l - 1) / (f3l + k - 1), (f3u - 1) / (f3u + k - 1)], [1 - 1 / f1l, 1 - 1 / f1u],
                           [l2 * k / (1 + l2 * (k - 1)), u2 * k / (1 + u2 * (k - 1))], [1 - 1 / f3l, 1 - 1 / f3u]], dtype=np.float64)
    return dict(Type=np.array(ICC_TYPES), Description=np.array(ICC_DESCRIPTIONS), ICC=values, F=F, df1=df1, df2=df2, pval=pval, CI95=ci)


def bpq_icc(outputs, targetsA, targetsB):
    """The three tables the BreastPathQ mains print after ``test()`` (eval_BreastPathQ_SSL_CR.py:570-599, eval_BreastPathQ_SSL.py):
    the model against pathologist A, against pathologist B, and A against B, every image one target and the pair its two raters --
    ``icc`` of the [n, 2] stacks.  outputs / targetsA / targetsB: [n], what ``steps.bpq_test`` returns (CPU tensors or arrays).
    -> dict ``{"MA": ..., "MB": ..., "AB": ...}`` of ``icc`` dicts.  PARITY UNPINNED against pingouin (see ``icc``)."""
    cols = [np.asarray(torch.as_tensor(v).cpu() if torch.is_tensor(v) else v, dtype=np.float64).reshape(-1) for v in (outputs, targetsA, targetsB)]
    if len({len(c) for c in cols}) != 1:
        raise ValueError(f"bpq_icc: {[len(c) for c in cols]} values in outputs / targetsA / targetsB")
    m, a, b = cols
    return dict(MA=icc(np.stack([m, a], 1)), MB=icc(np.stack([m, b], 1)), AB=icc(np.stack([a, b], 1)))


# ---- k-nearest-neighbour feature probe: the quantitative form of the reference's t-SNE plot of final_feats / final_targets
class FeatureBank:
    """Embeddings and their targets held on the device for ``knn_classify`` / ``knn_regress`` / ``knn_probe``.  ``add(feats, targets)``
    appends a device batch (float32 [n, dim]; integer labels or float targets [n]) without a copy to the host -- into a buffer of
    ``capacity`` rows when one was stated, else into a list ``finalize()`` concatenates.  ``finalize()`` normalises the rows once
    for ``metric="cosine"`` (``kernels.l2_normalize``; "dot" keeps them) and never synchronises.  ``n_classes``: the class count of
    integer labels; a label outside ``[0, n_classes)`` takes no part in a vote.  Without it ``class_count()`` reads the largest label
    off the device -- ONE scalar copy, a synchronisation -- when a classification first needs the count.  dim % 4 == 0,
    4 <= dim <= 2048."""

    def __init__(self, dim, capacity=None, metric="cosine", n_classes=None):
        if metric not in ("cosine", "dot"):
            raise ValueError(f"FeatureBank: metric = {metric!r} outside ('cosine', 'dot')")
        if dim % 4 or not 4 <= dim <= K.KNN_MAX_D:
            raise ValueError(f"FeatureBank: dim = {dim} must be a multiple of 4 in [4, {K.KNN_MAX_D}]")
        self.dim, self.capacity, self.metric, self.n_classes = int(dim), capacity, metric, n_classes
        self.n = 0
        self._feats, self._targets = [], []
        self._buf = self._tbuf = None
        self.feats = self.targets = None

    def add(self, feats, targets):
        if self.feats is not None:
            raise RuntimeError("FeatureBank: add() after finalize()")
        if not feats.is_cuda or feats.dtype != torch.float32 or feats.dim() != 2 or feats.shape[1] != self.dim:
            raise K.L.SslcrError(f"FeatureBank.add: device float32 [n, {self.dim}] expected (no CPU fallback)")
        targets = targets.reshape(-1).to(feats.device)
        if targets.numel() != feats.shape[0]:
            raise ValueError(f"FeatureBank.add: {targets.numel()} targets for {feats.shape[0]} rows")
        targets = targets.float() if targets.is_floating_point() else targets.long()
        n = feats.shape[0]
        if self.capacity is not None:
            if self.n + n > self.capacity:
                raise ValueError(f"FeatureBank.add: {self.n + n} rows exceed the capacity {self.capacity}")
            if self._buf is None:
                self._buf = torch.empty((self.capacity, self.dim), dtype=torch.float32, device=feats.device)
                self._tbuf = torch.empty(self.capacity, dtype=targets.dtype, device=feats.device)
            self._buf[self.n:self.n + n].copy_(feats)
            self._tbuf[self.n:self.n + n].copy_(targets)
        else:
            self._feats.append(feats.detach())
            self._targets.append(targets)
        self.n += n
        return self

    def finalize(self):
        if self.feats is None:
            if self.n == 0:
                raise ValueError("FeatureBank.finalize: the bank is empty")
            feats = self._buf[:self.n] if self.capacity is not None else torch.cat(self._feats)
            self.targets = self._tbuf[:self.n] if self.capacity is not None else torch.cat(self._targets)
            self.feats = K.l2_normalize(feats) if self.metric == "cosine" else feats.contiguous()
            self._feats, self._targets, self._buf, self._tbuf = [], [], None, None
        return self

    def class_count(self, query_labels=None):
        """``n_classes`` as stated; else 1 + the largest label of the bank and of ``query_labels`` (one scalar copy: a sync)"""
        if self.n_classes is not None:
            return int(self.n_classes)
        self.finalize()
        top = self.targets.max()
        if query_labels is not None and query_labels.numel():
            top = torch.maximum(top, query_labels.max().to(top.dtype))
        return int(top.item()) + 1

    def queries(self, feats):
        """query rows in the bank's metric: normalised for cosine"""
        return K.l2_normalize(feats) if self.metric == "cosine" else feats.contiguous()


def _bank_topk(bank, queries, k, exclude_self):
    bank.finalize()
    q = bank.feats if queries is None else bank.queries(queries)
    return K.knn_topk(q, bank.feats, k, exclude_self=exclude_self)


def knn_classify(bank, queries, k=20, weights="uniform", temperature=0.07, *, query_labels=None, exclude_self=None):
    """k-NN classification of device float32 ``queries`` [nq, dim] (None: the bank's own rows) from a ``FeatureBank`` of integer
    labels: ``kernels.knn_topk`` then ``kernels.knn_vote``, everything on the device; no sync when the bank states ``n_classes`` (else
    the one scalar copy of ``FeatureBank.class_count``, over the bank's and the query labels).  -> dict with ``pred`` int64 [nq],
    ``votes`` float32 [nq, C], ``scores`` / ``indices`` [nq, k] and, with ``query_labels``, ``confusion`` int64 [C, C].  weights:
    "uniform" (sklearn's ``KNeighborsClassifier``) or "softmax" (``exp((s - s_0) / temperature)``, the DINO / InstDisc vote).
    exclude_self: query i ignores bank row i + exclude_self (leave-one-out)."""
    scores, indices = _bank_topk(bank, queries, k, exclude_self)
    if bank.targets.is_floating_point():
        raise ValueError("knn_classify: the bank holds float targets (knn_regress)")
    Cn = bank.class_count(query_labels)
    out = K.knn_vote(indices, scores, labels=bank.targets, n_classes=Cn, weights=weights, temperature=temperature,
                     query_labels=query_labels)
    out.update(scores=scores, indices=indices, n_classes=Cn)
    return out


def knn_regress(bank, queries, k=5, *, exclude_self=None):
    """k-NN regression from a ``FeatureBank`` of float targets (the BreastPathQ cellularity scores): -> dict with ``pred`` float32
    [nq], the mean of the k neighbours' targets (sklearn's ``KNeighborsRegressor``), and ``scores`` / ``indices``.  No sync."""
    scores, indices = _bank_topk(bank, queries, k, exclude_self)
    if not bank.targets.is_floating_point():
        raise ValueError("knn_regress: the bank holds integer labels (knn_classify)")
    out = K.knn_vote(indices, scores, targets=bank.targets)
    out.update(scores=scores, indices=indices)
    return out


def knn_probe(feats, targets, k=20, leave_one_out=True, *, queries=None, query_targets=None, metric="cosine", weights="uniform",
              temperature=0.07, n_classes=None):
    """How good are these embeddings: the accuracy of a k-NN classifier on them.  feats / targets: device float32 [n, dim] and integer
    [n] -- what ``steps.rsp_train`` returns as ``final_feats, final_targets`` feeds it as it is.  leave_one_out: every row is classified
    from the others (``exclude_self``); otherwise ``queries`` / ``query_targets`` are classified from the bank.  -> dict with
    ``accuracy`` and the other figures of ``metrics_from_confusion``, ``confusion`` (int64 [C, C] array, rows = targets) and ``pred``
    (int64 array).  With ``n_classes`` stated there is ONE copy to the host, of the final numbers; without it the class count is
    read off the labels first (one more scalar copy, ``FeatureBank.class_count``).  A target outside ``[0, n_classes)`` cannot be
    counted: the confusion matrix then holds fewer rows than there are queries, and this raises instead of averaging over fewer."""
    bank = FeatureBank(feats.shape[1], metric=metric, n_classes=n_classes).add(feats, targets).finalize()
    if leave_one_out:
        r = knn_classify(bank, None, k, weights, temperature, query_labels=bank.targets, exclude_self=0)
    else:
        if queries is None or query_targets is None:
            raise ValueError("knn_probe: leave_one_out=False needs queries and query_targets")
        r = knn_classify(bank, queries, k, weights, temperature, query_labels=query_targets.reshape(-1).to(feats.device))
    Cn = r["n_classes"]
    flat = torch.cat([r["confusion"].reshape(-1), r["pred"]]).cpu().numpy()             # the one copy
    cm = flat[:Cn * Cn].reshape(Cn, Cn)
    if int(cm.sum()) != r["pred"].numel():
        raise ValueError(f"knn_probe: {r['pred'].numel() - int(cm.sum())} query targets lie outside [0, {Cn}): state n_classes to cover them")
    out = metrics_from_confusion(cm)
    out.update(confusion=cm, pred=flat[Cn * Cn:])
    return out


# ---- t-SNE embedding: what the reference's mains do with final_feats after the best epoch (TSNE().fit_transform), without the plot
class Tsne:
    """t-SNE of device features into two components, every launch on the caller's stream (csrc/tsne.hip; the arithmetic is sklearn
    1.7.2's ``TSNE(method="exact")`` on k-nearest-neighbour affinities, restated and pinned in tests/_tsne_ref.py):
    ``kernels.euclidean_topk`` (k = min(n - 1, int(3 perplexity + 1), 64); sklearn has no cap at 64), ``tsne_affinities``,
    ``tsne_joint``, then ``max_iter`` times ``tsne_step`` -- the EXACT repulsive sum over all pairs, no tree and no grid --
    with early exaggeration and momentum 0.5 for the first 250 iterations, then 1 and 0.8.  learning_rate "auto" =
    max(n / early_exaggeration / 4, 50).

    init: "pca" (float64 covariance and ``torch.linalg.eigh`` on the device, each axis signed so that its largest-magnitude loading
    is positive, scaled to std(y[:, 0]) = 1e-4 -- PARITY UNPINNED against sklearn's randomized PCA, whose axes differ in sign and in
    the last bits), "random" (1e-4 randn, ``generator``) or a device tensor [n, 2].

    ``fit(feats)`` (device float32 [n, D], 2 <= n <= 2^20, D % 4 == 0, 4 <= D <= 2044) queues everything and makes ONE copy at the
    end, of the log; KL and |grad| go to a device log every ``check_every`` iterations and once at the end.  ``early_stop=True``
    applies sklearn's two stopping rules (no progress for 250 / 300 iterations, |grad| <= 1e-7 -- of the plain gradient, where
    sklearn measures it after the gains) and pays one host read per check; the default never reads inside the loop.  ``reads`` counts
    the calls of the one read site.  After a fit: ``embedding_`` (device [n, 2]), ``kl_divergence_``, ``log`` (array [checks, 4]:
    KL, |grad|, Z, iteration), ``n_iter_``.  ``step()`` runs one iteration; ``state`` holds y, update, gains, grad and iteration."""
    STOP_LYING, MIN_GRAD_NORM = 250, 1e-7

    def __init__(self, perplexity=30.0, early_exaggeration=12.0, learning_rate="auto", max_iter=1000, init="pca", generator=None,
                 check_every=50, early_stop=False, slices=None):
        if not (isinstance(init, torch.Tensor) or init in ("pca", "random")):
            raise ValueError(f"Tsne: init = {init!r} outside ('pca', 'random', tensor [n, 2])")
        if learning_rate != "auto" and not float(learning_rate) > 0:
            raise ValueError(f"Tsne: learning_rate = {learning_rate!r} must be 'auto' or > 0")
        if max_iter < 0 or check_every < 1 or not perplexity > 0:
            raise ValueError("Tsne: max_iter >= 0, check_every >= 1 and perplexity > 0 expected")
        self.perplexity, self.early_exaggeration, self.learning_rate = float(perplexity), float(early_exaggeration), learning_rate
        self.max_iter, self.init, self.generator, self.check_every, self.early_stop, self.slices = int(max_iter), init, generator, int(check_every), early_stop, slices
        self.reads = 0
        self.iteration = 0
        self.P = None

    # the one read site
    def _read(self, t):
        self.reads += 1
        return t.cpu().numpy()

    @staticmethod
    def neighbours(n, perplexity):
        k = min(n - 1, int(3.0 * perplexity + 1), K.KNN_MAX_K)
        if not perplexity < k:
            raise ValueError(f"Tsne: perplexity = {perplexity} must be below the neighbour count k = {k} (n = {n}; k is capped at {K.KNN_MAX_K})")
        return k

    @staticmethod
    def center(x):
        """x minus the float32 rounding of its float64 column mean"""
        return x - x.double().mean(0).float()[None, :]

    @staticmethod
    def pca_init(xc):
        x = xc.double()
        x = x - x.mean(0)
        _, v = torch.linalg.eigh(x.T @ x / (x.shape[0] - 1))
        v = v.flip(1)[:, :2]
        top = v.gather(0, v.abs().argmax(0, keepdim=True))
        y = x @ (v * torch.sign(top))
        return (y / y[:, 0].std(unbiased=False) * 1e-4).float()

    def prepare(self, feats):
        """everything before the first iteration: neighbours, affinities, the joint CSR, the initial state"""
        if not isinstance(feats, torch.Tensor) or not feats.is_cuda or feats.dtype != torch.float32 or feats.dim() != 2:
            raise K.L.SslcrError("Tsne.fit: device float32 [n, D] expected (no CPU fallback)")
        n, D = feats.shape
        if not 2 <= n <= K.TSNE_MAX_N or D % 4 or not 4 <= D <= K.KNN_MAX_D - 4:
            raise K.L.SslcrError(f"Tsne.fit: n = {n} outside [2, 2^20] or D = {D} not a multiple of 4 in [4, {K.KNN_MAX_D - 4}]")
        k = self.neighbours(n, self.perplexity)
        dev = feats.device
        xc = self.center(feats.detach()).contiguous()
        idx, d2 = K.euclidean_topk(xc, k)
        cond, self.beta = K.tsne_affinities(d2, self.perplexity)
        self.P = K.tsne_joint(idx, cond)
        if isinstance(self.init, torch.Tensor):
            if tuple(self.init.shape) != (n, 2):
                raise ValueError(f"Tsne.fit: init must be [{n}, 2]")
            y = self.init.to(dev, torch.float32).contiguous().clone()
        elif self.init == "pca":
            y = self.pca_init(xc).contiguous()
        else:
            y = (1e-4 * torch.randn((n, 2), generator=self.generator, device=dev if self.generator is None else self.generator.device)).to(dev, torch.float32)
        self.n = n
        self.lr = max(n / self.early_exaggeration / 4.0, 50.0) if self.learning_rate == "auto" else float(self.learning_rate)
        self._y = [y, torch.empty_like(y)]
        self._cur = 0
        self._update, self._gains, self._grad = torch.zeros_like(y), torch.ones_like(y), torch.zeros_like(y)
        self._w = K.tsne_workspace(n, dev, self.slices)
        self._kl_rows = torch.empty(n, dtype=torch.float64, device=dev)
        rows = self.max_iter // self.check_every + 2
        self._log = torch.zeros((rows, K.TSNE_LOG_COLS), dtype=torch.float64, device=dev)
        self._log_rows = 0
        self.iteration = 0
        return self

    @property
    def state(self):
        return dict(y=self._y[self._cur], update=self._update, gains=self._gains, grad=self._grad,
                    iteration=torch.tensor(self.iteration, device=self._grad.device))

    def schedule(self, it):
        return (self.early_exaggeration, 0.5) if it < self.STOP_LYING else (1.0, 0.8)

    def _log_kl(self, it):
        if self._log_rows >= self._log.shape[0]:                                         # step() called past max_iter: a longer log
            self._log = torch.cat([self._log, torch.zeros_like(self._log)])
        K.tsne_kl(self._kl_rows, self._grad, self._w["Z"], self._log[self._log_rows], it)
        self._log_rows += 1
        return self._log[self._log_rows - 1]

    def step(self):
        """one iteration: three launches (four on a check iteration), no host read.  -> the log row on a check iteration, else None"""
        it = self.iteration
        e, mom = self.schedule(it)
        check = (it + 1) % self.check_every == 0
        K.tsne_step(self._y[self._cur], self._y[1 - self._cur], self._update, self._gains, self.P, exaggeration=e, momentum=mom, lr=self.lr,
                    workspace=self._w, grad=self._grad, kl_rows=self._kl_rows if check else None)
        row = self._log_kl(it) if check else None
        self._cur ^= 1
        self.iteration = it + 1
        return row

    def fit(self, feats):
        self.prepare(feats)
        best = {}                                    # per stage (False: exaggerated): (the lowest KL so far, its iteration)
        while self.iteration < self.max_iter:
            it = self.iteration
            row = self.step()
            if row is not None and self.early_stop:
                kl, gnorm = self._read(row)[:2]
                second = it >= self.STOP_LYING
                low, low_it = best.get(second, (float("inf"), self.STOP_LYING if second else 0))
                stop = gnorm <= self.MIN_GRAD_NORM
                if kl < low:
                    best[second] = (kl, it)
                elif it - low_it > (300 if second else 250):
                    stop = True
                if stop and second:
                    break
                if stop:                             # sklearn ends the exaggerated stage and goes on with the second
                    self.iteration = self.STOP_LYING
        return self._finish()

    def _finish(self):
        # the KL of the final embedding: a gradient without an update
        g, _ = K.tsne_gradient(self._y[self._cur], self.P, 1.0, workspace=self._w, kl_rows=self._kl_rows)
        self._grad = g
        self._log_kl(self.iteration)
        self.log = self._read(self._log[:self._log_rows])                                # the one copy
        self.embedding_ = self._y[self._cur]
        self.kl_divergence_ = float(self.log[-1, 0])
        self.n_iter_ = self.iteration
        return self


def tsne(feats, targets=None, **kw):
    """The embedding the reference's mains plot: feats / targets as ``steps.rsp_train`` returns them (device float32 [n, D]; targets
    pass through untouched for the plot's colours).  -> dict with ``embedding`` (DEVICE float32 [n, 2]: hand ``.cpu()`` of it to
    matplotlib), ``kl_divergence``, ``n_iter`` and ``targets``.  kw: ``Tsne``'s arguments.  One copy to the host, of the log."""
    t = Tsne(**kw).fit(feats)
    return dict(embedding=t.embedding_, kl_divergence=t.kl_divergence_, n_iter=t.n_iter_, targets=targets, log=t.log)


def neighbour_preservation(x, y, k):
    """The mean share of each point's k nearest neighbours in x (device float32 [n, D], D <= 2044) that are also among its k nearest in
    y (device float32 [n, d]): two ``kernels.euclidean_topk`` calls and one scalar copy.  The small quantitative companion of the
    embedding."""
    ix, _ = K.euclidean_topk(x.contiguous(), k)
    iy, _ = K.euclidean_topk(y.contiguous(), k)
    both = ((ix[:, :, None] == iy[:, None, :]) & (ix[:, :, None] >= 0)).any(2)
    return float(both.sum().item()) / (ix.shape[0] * k)


# ---- linear probe: the reference's `--modules 64` ("fine-tune only classifier") as the convex problem it is
class LinearProbe:
    """Linear evaluation of fixed features: multinomial logistic regression (``loss="softmax"``) or ridge regression (``"squared"``,
    BreastPathQ's MSE head) of device features, fitted by a host float64 L-BFGS (``lbfgs.minimize``) whose every value and gradient is
    ONE fused device evaluation (``kernels.linprobe_eval``; csrc/linprobe.hip).

    Objective: ``sum_i s_i l_i / sum_i s_i + (lam / 2) ||W||^2`` with ``lam = 1 / (C * sum_i s_i)`` (``C=``, sklearn's inverse
    regularisation strength; default 1.0) or ``lam = l2`` (``l2=``) -- state one, not both; the intercept is not penalised.  For three
    or more classes that is sklearn 1.7.2's ``LogisticRegression(C=C)``; the softmax form is used for EVERY class count (the
    reference's two-logit Camelyon16 head), so for two classes the optimum equals sklearn's binary model at ``C_sklearn = 2 C`` with
    ``W = [-w / 2, +w / 2]``.  ``class_weight="balanced"`` is sklearn's (``n / (classes present * count)``; their sum is n);
    ``loss="squared"`` with ``l2 = lam`` is ``Ridge(alpha = lam * n)``.  normalize="l2": rows through ``kernels.l2_normalize`` first,
    in ``fit`` and in every query.  Standardising features, an L1 penalty and other solvers are out of scope.

    Host traffic.  Features, labels and weights never leave the device.  One evaluation is one ``linprobe_eval`` and ONE copy to the
    host, of the value and the gradient: 8 (1 + C (D + 1)) bytes, through the one read site ``_read``; ``reads`` counts its calls, and
    after ``fit`` it EQUALS ``n_eval_``.  With ``n_classes`` stated there is no other read: the penalty needs ``sum_i s_i`` on the host,
    which is n without weights and under "balanced"; labels are then taken to lie in [0, n_classes) (the kernel leaves a row outside
    it out of the data term, but n still counts it).  Without ``n_classes`` the largest label is read off the device first, and with a
    ``sample_weight`` its sum is (one scalar copy each, counted in ``setup_reads``).

    After ``fit(feats, targets, sample_weight=None)`` (feats device float32 [n, D], D % 4 == 0, 4 <= D <= 2048; integer labels [n], or
    float targets [n] / [n, C] for "squared"): ``coef_`` [C, D] and ``intercept_`` [C] (device float32: the point the last evaluation
    was made at), ``n_iter_``, ``n_eval_``, ``status_`` ("converged" | "precision" | "max_iter": lbfgs.py), ``log`` (array
    [iterations, 4]: objective, max|g|, step, evaluations), ``objective_``, ``grad_max_``.  ``decision_function`` / ``predict`` /
    ``predict_proba`` / ``score`` run on device queries (``kernels.linprobe_logits``, ``kernels.predict``); ``score`` (accuracy, or
    R^2 for "squared") makes one scalar copy.  ``to_classifier(classifier)`` copies W, b into a ``net.FinetuneResNet``'s
    ``classifier[0]``, so the ``*_test`` drop-ins run with the fitted head."""

    def __init__(self, C=None, *, l2=None, loss="softmax", fit_intercept=True, normalize=None, class_weight=None, tol=1e-4,
                 max_iter=1000, history=10, n_classes=None, groups=None):
        if C is not None and l2 is not None:
            raise ValueError("LinearProbe: state C or l2, not both")
        if loss not in K.LINPROBE_LOSSES:
            raise ValueError(f"LinearProbe: loss = {loss!r} outside {tuple(K.LINPROBE_LOSSES)}")
        if normalize not in (None, "l2"):
            raise ValueError(f"LinearProbe: normalize = {normalize!r} outside (None, 'l2')")
        if class_weight not in (None, "balanced"):
            raise ValueError(f"LinearProbe: class_weight = {class_weight!r} outside (None, 'balanced')")
        if class_weight is not None and loss != "softmax":
            raise ValueError("LinearProbe: class_weight applies to the softmax loss")
        if l2 is None and not float(1.0 if C is None else C) > 0:
            raise ValueError("LinearProbe: C must be > 0")
        if l2 is not None and not float(l2) >= 0:
            raise ValueError("LinearProbe: l2 must be >= 0")
        self.C, self.l2 = (None if l2 is not None else float(1.0 if C is None else C)), (None if l2 is None else float(l2))
        self.loss, self.fit_intercept, self.normalize, self.class_weight = loss, bool(fit_intercept), normalize, class_weight
        self.tol, self.max_iter, self.history, self.n_classes, self.groups = float(tol), int(max_iter), int(history), n_classes, groups
        self.reads = self.setup_reads = 0
        self.coef_ = self.intercept_ = None

    # the one read site of the fit's loop
    def _read(self, t):
        self.reads += 1
        return t.cpu().numpy()

    def _features(self, feats):
        if not isinstance(feats, torch.Tensor) or not feats.is_cuda or feats.dtype != torch.float32 or feats.dim() != 2:
            raise K.L.SslcrError("LinearProbe: device float32 [n, D] expected (no CPU fallback)")
        return K.l2_normalize(feats) if self.normalize == "l2" else feats.contiguous()

    def fit(self, feats, targets, sample_weight=None):
        from . import lbfgs
        x = self._features(feats.detach())
        n, D = x.shape
        dev = x.device
        self.reads = self.setup_reads = 0
        targets = targets.to(dev)
        if self.loss == "softmax":
            if targets.is_floating_point():
                raise ValueError("LinearProbe: integer labels expected for the softmax loss (loss='squared' takes float targets)")
            y = targets.reshape(-1).long()
            if self.n_classes is None:
                self.setup_reads += 1
                Cn = int(y.max().item()) + 1
            else:
                Cn = int(self.n_classes)
        else:
            y = targets.float().reshape(n, -1).contiguous()
            Cn = y.shape[1]
        s, total = None, float(n)
        if sample_weight is not None:
            s = sample_weight.to(dev, torch.float32).reshape(-1)
        if self.class_weight == "balanced":
            counts = torch.bincount(y.clamp(0, Cn - 1), minlength=Cn).double()
            cw = (float(n) / ((counts > 0).sum().double() * counts.clamp_min(1.0))).float()
            s = cw[y.clamp(0, Cn - 1)] if s is None else s * cw[y.clamp(0, Cn - 1)]
        if sample_weight is not None:
            self.setup_reads += 1
            total = float(s.double().sum().item())
        lam = self.l2 if self.l2 is not None else 1.0 / (self.C * total)
        self.n_classes_, self.lam_ = Cn, lam
        E = Cn * (D + 1)
        buf = torch.empty(1 + E, dtype=torch.float64, device=dev)

        def fun(theta):
            th32 = torch.from_numpy(theta.astype(np.float32).reshape(Cn, D + 1)).to(dev)
            w, b = th32[:, :D].contiguous(), th32[:, D].contiguous()
            K.linprobe_eval(x, y, w, b, self.loss, s, self.groups, out=buf)
            flat = self._read(buf)                                                           # the one copy: value and gradient
            W = theta.reshape(Cn, D + 1)[:, :D]
            g = flat[1:].reshape(Cn, D + 1).copy()
            g[:, :D] += lam * W
            if not self.fit_intercept:
                g[:, D] = 0.0
            return float(flat[0]) + 0.5 * lam * float((W * W).sum()), g.ravel()

        r = lbfgs.minimize(fun, np.zeros(E), tol=self.tol, max_iter=self.max_iter, history=self.history)
        th32 = torch.from_numpy(r.x.astype(np.float32).reshape(Cn, D + 1)).to(dev)
        self.coef_, self.intercept_ = th32[:, :D].contiguous(), th32[:, D].contiguous()
        self.theta_ = r.x.reshape(Cn, D + 1)
        self.n_iter_, self.n_eval_, self.status_, self.log = r.n_iter, r.n_eval, r.status, r.log
        self.objective_, self.grad_max_ = r.f, float(np.abs(r.g).max())
        return self

    def _fitted(self):
        if self.coef_ is None:
            raise RuntimeError("LinearProbe: fit() first")

    def decision_function(self, feats):
        """device float32 [n, C]: ``feats W^T + b``, no sync"""
        self._fitted()
        return K.linprobe_logits(self._features(feats), self.coef_, self.intercept_, self.groups)

    def predict(self, feats):
        """softmax: device int64 [n], the lowest index of the row maximum; squared: the outputs [n, C] themselves.  No sync."""
        z = self.decision_function(feats)
        return z if self.loss == "squared" else K.predict(z)["pred"]

    def predict_proba(self, feats):
        if self.loss != "softmax":
            raise ValueError("LinearProbe.predict_proba: the softmax loss only")
        return K.predict(self.decision_function(feats), scores=True, pred=False)["scores"]

    def score(self, feats, targets):
        """accuracy (softmax) or R^2 over all outputs (squared): one scalar copy"""
        p = self.predict(feats)
        t = targets.to(p.device)
        if self.loss == "softmax":
            return float((p == t.reshape(-1).long()).double().mean().item())
        t = t.double().reshape(p.shape)
        return float((1.0 - ((p.double() - t) ** 2).sum() / ((t - t.mean(0)) ** 2).sum()).item())

    def to_classifier(self, classifier):
        """W, b into ``classifier.classifier[0]`` (``net.FinetuneResNet``: nn.Linear(768, n_classes)), in place"""
        self._fitted()
        if self.normalize is not None:
            raise ValueError("LinearProbe.to_classifier: a probe of normalised features is not the head of the raw ones")
        lin = classifier.classifier[0]
        if tuple(lin.weight.shape) != tuple(self.coef_.shape):
            raise ValueError(f"LinearProbe.to_classifier: the head is {list(lin.weight.shape)}, the probe {list(self.coef_.shape)}")
        with torch.no_grad():
            lin.weight.copy_(self.coef_)
            lin.bias.copy_(self.intercept_)
        return classifier


def linear_probe(feats, targets, *, queries=None, query_targets=None, sample_weight=None, **kw):
    """How good are these embeddings: a ``LinearProbe`` fitted on (feats, targets) -- ``steps.rsp_train``'s ``final_feats,
    final_targets`` as they are -- and scored on ``queries`` / ``query_targets`` (without them: the fit's training figures).  Integer
    targets -> ``knn_probe``'s dict (``accuracy`` and the other figures of ``metrics_from_confusion``, ``confusion``, ``pred``); float
    targets (``loss="squared"`` is implied) -> ``pred`` and ``mse``.  Plus ``probe``, the fitted object.  sample_weight: ``fit``'s (device
    float32 [n]; its sum is read once).  kw: ``LinearProbe``'s.  One
    copy per evaluation during the fit (see ``LinearProbe``) and one of the final numbers."""
    if targets.is_floating_point():
        kw.setdefault("loss", "squared")
    probe = LinearProbe(**kw).fit(feats, targets, sample_weight=sample_weight)
    q = feats if queries is None else queries
    qt = (targets if query_targets is None else query_targets).to(q.device)
    if probe.loss == "squared":
        pred = probe.predict(q)
        truth = qt.float().reshape(pred.shape)
        flat = torch.cat([pred.reshape(-1), ((pred - truth) ** 2).mean().reshape(1)]).cpu().numpy()
        return dict(pred=flat[:-1].reshape(tuple(pred.shape)).squeeze(-1) if pred.shape[1] == 1 else flat[:-1].reshape(tuple(pred.shape)),
                    mse=float(flat[-1]), probe=probe)
    Cn = probe.n_classes_
    cm = torch.zeros((Cn, Cn), dtype=torch.int64, device=q.device)
    qt = qt.reshape(-1).long().contiguous()
    r = K.predict(probe.decision_function(q), qt, confusion=cm)
    flat = torch.cat([cm.reshape(-1), r["pred"]]).cpu().numpy()                           # the one copy
    cm = flat[:Cn * Cn].reshape(Cn, Cn)
    if int(cm.sum()) != r["pred"].numel():
        raise ValueError(f"linear_probe: {r['pred'].numel() - int(cm.sum())} query targets lie outside [0, {Cn}): state n_classes to cover them")
    out = metrics_from_confusion(cm)
    out.update(confusion=cm, pred=flat[Cn * Cn:], probe=probe)
    return out
