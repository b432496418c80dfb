"""Device-resident tile mining for RSP (resolution sequence prediction) pretraining.

The reference's ``Vectorize_WSIs.get_wsi_patches`` (dataset.py:386-446, Pretraining_v2/dataset.py:268-316) walks a candidate grid over the
level-2 image, converts every candidate tile to CIELAB (v1, util.py:18-23) or HSV (v2, Pretraining_v2/util.py:9-13) on the CPU to decide
whether it is tissue, cuts three tiles per kept candidate from three pyramid levels (``__getitem__``), and ``sorted_sequence``
(dataset.py:27-70) stores six orderings of every triplet in host memory.  Here the three levels are uploaded once as uint8 [H, W, 3] and

* the per-pixel predicate is evaluated ONCE per pixel into a bit plane (``kernels.tissue_bits``), the mean a* of the v1 criterion
  summed on the device (``kernels.lab_a_sum``) and read by the predicate's launch without a host sync;
* every candidate's count is a few popcounts on that plane (``kernels.tile_popcount``); the host reads the keep flags once;
* the coordinate tables restate the reference's expressions in Python ints and floats exactly as written (``triplet_origins``);
* a batch is one launch that cuts the three tiles of every sample and applies its ordering (``kernels.rsp_gather``): the virtual
  dataset has 6 T samples, sample k = triplet k // 6 under ordering k % 6, and none of it is materialised.

openslide I/O is not part of this package: the caller reads the levels (``np.asarray(slide.read_region((0, 0), l,
slide.level_dimensions[l]).convert('RGB'))``), the overview image of the v1 criterion and ``slide.level_downsamples``.

Unpinned: the CIELAB chain against scikit-image itself; ``read_region``'s level-pixel origin, taken as
``int(level0 / downsample)``, against openslide for downsamples that are no integers; and, for such downsamples, the window the
predicate looks at, which is the candidate's own (xpos, ypos) here where the reference's round trip ``int(int(ds * xpos) / ds)`` can land
one pixel to the left.  What a tile holds outside its level is the caller's statement (``fill``), as for ``WsiDeviceLoader``.
"""
import numpy as np
import torch

from . import kernels as K

ORDERINGS = ((0, 1, 2), (0, 2, 1), (1, 2, 0), (1, 0, 2), (2, 0, 1), (2, 1, 0))    # sorting_orders over (hr, lr1, lr2), dataset.py:39
CRITERIA = {"v1": ("lab_a", 0.15, 0.95), "v2": ("hsv_s", 0.1, 0.75)}            # isforeground's defaults: (mode, mu_percent, thresh)


def srgb_linear_table():
    """float64 [256]: skimage 0.15 rgb2xyz's linearisation of ``img_as_float(u8)``, NumPy's own ``power`` -- what the device looks up"""
    c = np.multiply(np.arange(256), 1.0 / 255, dtype=np.float64)
    out = c / 12.92
    mask = c > 0.04045
    out[mask] = np.power((c[mask] + 0.055) / 1.055, 2.4)
    return out


def _pair(v):
    if isinstance(v, (tuple, list)):
        a, b = v
        return int(a), int(b)
    return int(v), int(v)


def candidate_grid(iw, ih, tile, stride):
    """-> (xpos [nx], ypos [ny]) Python int lists: ``range(sw, iw - 1 - pw, sw)`` and ``range(sh, ih - 1 - ph, sh)`` (dataset.py:424-425).
    The reference visits ``for ypos: for xpos``: candidate (j, i) is number ``j * nx + i``.  tile, stride: an int or (h, w)."""
    (ph, pw), (sh, sw) = _pair(tile), _pair(stride)
    if min(ph, pw, sh, sw) < 1:
        raise ValueError(f"candidate_grid: tile = {tile}, stride = {stride}")
    return list(range(sw, int(iw) - 1 - pw, sw)), list(range(sh, int(ih) - 1 - ph, sh))


def triplet_origins(xpos, ypos, downsamples, tile, variant):
    """The three ``read_region`` calls of ``Vectorize_WSIs.__getitem__`` for candidates (xpos[k], ypos[k]) of the level-2 grid ->
    int32 arrays (hr, lr1, lr2), each [n, 2] of (left, top) in the pixels of ITS level.  downsamples = level_downsamples of
    (hr, lr1, lr2) as floats; tile: an int or (h, w).  The level-0 expressions are the reference's, in Python ints and floats:
      "v1" (dataset.py:335-371)               lr1 and hr START at the centre of the lr2 tile
      "v2" (Pretraining_v2/dataset.py:234-255) the three tiles are concentric
    and the level-pixel origin is ``int(level0 / downsample)``."""
    if variant not in ("v1", "v2"):
        raise ValueError(f"triplet_origins: variant {variant!r} outside ('v1', 'v2')")
    tile_h, tile_w = _pair(tile)
    mhr, mlr, m = (float(d) for d in downsamples)
    if min(mhr, mlr, m) <= 0.0:
        raise ValueError(f"triplet_origins: downsamples = {tuple(downsamples)}")
    out = [np.empty((len(xpos), 2), dtype=np.int64) for _ in range(3)]
    for k, (x, y) in enumerate(zip(xpos, ypos)):
        x, y = int(x), int(y)
        lr2 = (int(m * x), int(m * y))
        if variant == "v1":
            lr1 = (int(int(int(m * (x + (tile_w / 2))) / mlr) * mlr), int(int(int(m * (y + (tile_h / 2))) / mlr) * mlr))
            hr = (int(int(int(m * (x + (tile_w / 2))) / mhr) * mhr), int(int(int(m * (y + (tile_h / 2))) / mhr) * mhr))
        else:
            lr1 = (int(int(int(int(m * (x + (tile_w / 2))) / mlr) - int(tile_w / 2)) * mlr),
                   int(int(int(int(m * (y + (tile_h / 2))) / mlr) - int(tile_h / 2)) * mlr))
            hr = (int(int(int(int(m * (x + (tile_w / 2))) / mhr) - int(tile_w / 2)) * mhr),
                  int(int(int(int(m * (y + (tile_h / 2))) / mhr) - int(tile_h / 2)) * mhr))
        for t, (l0, ds) in zip(out, ((hr, mhr), (lr1, mlr), (lr2, m))):
            t[k] = (int(l0[0] / ds), int(l0[1] / ds))
    for t in out:
        if len(t) and (t.min() < -(1 << 31) or t.max() >= 1 << 31):
            raise ValueError("triplet_origins: a tile coordinate does not fit int32")
    return tuple(t.astype(np.int32) for t in out)


def _device_u8(name, img, device):
    t = torch.as_tensor(img)
    if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3:
        raise ValueError(f"{name}: uint8 images [H, W, 3] expected")
    if not t.is_cuda:
        t = t.to(torch.device(device if device is not None else "cuda"), non_blocking=True)
    return t.contiguous()


def _criterion(criterion, variant):
    mode, mu_percent, thresh = CRITERIA[variant] if criterion is None else criterion
    if mode not in K.TISSUE_MODES:
        raise ValueError(f"criterion {mode!r} outside {sorted(K.TISSUE_MODES)}")
    return mode, float(mu_percent), float(thresh)


def tissue_plane(lr2, criterion, overview=None):
    """the bit plane of the level-2 image (device uint8 [H, W, 3]) under criterion = (mode, mu_percent, thresh): "hsv_s" thresholds
    s at mu_percent; "lab_a" thresholds a* at (1 + mu_percent) * mean a* of ``overview`` (device uint8), the mean staying on the device"""
    mode, mu_percent, _ = criterion
    if mode == "hsv_s":
        return K.tissue_bits(lr2, "hsv_s", mu_percent)
    if overview is None:
        raise ValueError("the lab_a criterion needs the overview image its mean a* is taken over")
    lin = torch.from_numpy(srgb_linear_table()).to(lr2.device)
    total = K.lab_a_sum(overview, lin)
    return K.tissue_bits(lr2, "lab_a", lin=lin, thr_sum=total, factor=1 + mu_percent, count=float(overview.shape[0] * overview.shape[1]))


def mine_tiles(levels, downsamples, tile, stride, *, variant="v1", criterion=None, overview=None, device=None):
    """``get_wsi_patches`` up to the tile bytes.  levels = (hr, lr1, lr2) uint8 [H, W, 3], host or device; downsamples: their
    level_downsamples; criterion: (mode, mu_percent, thresh), default the variant's ``isforeground``; overview: the lowest-level image of
    the lab_a criterion.  -> dict: ``levels`` (device tensors), ``xpos`` / ``ypos`` (the kept candidates, reference order), ``count`` and
    ``keep`` (numpy [ny, nx]), ``xy`` = the int32 tables (hr, lr1, lr2) of ``triplet_origins``.  One host read: the keep flags."""
    if len(levels) != 3 or len(downsamples) != 3:
        raise ValueError("mine_tiles: three levels (hr, lr1, lr2) and their three downsamples expected")
    tile = int(tile)
    crit = _criterion(criterion, variant)
    levels = tuple(_device_u8("mine_tiles", lv, device) for lv in levels)
    lr2 = levels[2]
    if overview is not None:
        overview = _device_u8("mine_tiles", overview, lr2.device)
    ih, iw = lr2.shape[0], lr2.shape[1]
    xs, ys = candidate_grid(iw, ih, tile, stride)
    bits = tissue_plane(lr2, crit, overview)
    count, keep = K.tile_popcount(bits, iw, _pair(tile), _pair(stride), crit[2])
    keep, count = keep.cpu().numpy().astype(bool), count.cpu().numpy()
    jj, ii = np.nonzero(keep)                                      # row-major: the reference's loop order
    xpos, ypos = [xs[i] for i in ii], [ys[j] for j in jj]
    return {"levels": levels, "xpos": xpos, "ypos": ypos, "count": count, "keep": keep,
            "xy": triplet_origins(xpos, ypos, downsamples, tile, variant)}


class RspDeviceLoader:
    """The loader of the RSP pretraining scripts over ONE slide whose three pyramid levels sit in HBM: what
    ``DataLoader(sorted_sequence(*get_wsi_patches(slide)))`` yields, without the host pipeline.  levels = (hr, lr1, lr2) and overview:
    host or device uint8 [H, W, 3], uploaded once; downsamples: their level_downsamples; tile: the (square) tile side; stride: an int
    or (h, w); variant "v1" / "v2": the coordinate expressions; criterion: (mode, mu_percent, thresh), default the variant's.
    ``len()`` counts batches as a DataLoader does (``drop_last``).  Iterating yields ``(Data_1, Data_2, Data_3, Class_labels)``: device
    uint8 [n, 3, tile, tile] tiles and int64 [n] labels.  shuffle draws ``torch.randperm(6 T, generator=)`` on the host per epoch and
    uploads it once.  ``triplets`` = T; a slide without tissue has length 0."""

    def __init__(self, levels, downsamples, tile, stride, batch_size, *, variant="v1", criterion=None, overview=None, shuffle=False,
                 generator=None, drop_last=False, fill=0, device=None):
        if int(batch_size) < 1 or int(tile) < 1:
            raise ValueError("RspDeviceLoader: batch_size and tile must be positive")
        if not 0 <= int(fill) <= 255:
            raise ValueError(f"RspDeviceLoader: fill = {fill} outside [0, 255]")
        mined = mine_tiles(levels, downsamples, tile, stride, variant=variant, criterion=criterion, overview=overview, device=device)
        self.levels = mined["levels"]
        dev = self.levels[0].device
        self.tile, self.batch_size, self.fill = int(tile), int(batch_size), int(fill)
        self.shuffle, self.generator, self.drop_last = bool(shuffle), generator, bool(drop_last)
        self.xpos, self.ypos, self.keep, self.count = mined["xpos"], mined["ypos"], mined["keep"], mined["count"]
        self.xy_host = mined["xy"]
        self.xy = tuple(torch.from_numpy(t).to(dev) for t in self.xy_host)
        self.triplets = len(self.xpos)
        self._order = torch.arange(6 * self.triplets, dtype=torch.int64).to(dev)

    def samples(self):
        return 6 * self.triplets

    def __len__(self):
        n = self.samples()
        return n // self.batch_size if self.drop_last else (n + self.batch_size - 1) // self.batch_size

    def batch(self, idx, out=None):
        """the samples ``idx`` (device int64 [n]) of the virtual dataset -> (Data_1, Data_2, Data_3, Class_labels)"""
        return K.rsp_gather(self.levels, self.xy, idx, self.tile, fill=self.fill, out=out)

    def __iter__(self):
        n = self.samples()
        order = self._order
        if self.shuffle and n:
            order = torch.randperm(n, generator=self.generator).to(order.device)
        for b in range(len(self)):
            yield self.batch(order[b * self.batch_size:min((b + 1) * self.batch_size, n)])
