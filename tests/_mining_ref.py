"""NumPy restatement of the host pipeline that builds RSP pretraining batches -- ``Vectorize_WSIs.get_wsi_patches`` with ``isforeground``
and ``sorted_sequence`` (dataset.py:27-70, 335-446 with util.py:18-23; Pretraining_v2/dataset.py:22-60, 219-316 with
Pretraining_v2/util.py:9-13) -- over an in-memory pyramid, and a seeded synthetic pyramid.  Test infrastructure: it imports neither the
reference, nor openslide, nor scikit-image.

PARITY UNPINNED against scikit-image, which is installed nowhere the tests run: ``lab_a`` follows the PUBLISHED source of the pinned
version (0.15.0, skimage/color/colorconv.py: rgb2lab = xyz2lab(rgb2xyz(.)) with illuminant D65 and the 2 degree observer); the HSV form
uses ``tests/_colour_ref.rgb2hsv``, which is pinned against ``colorsys``.  ``Pyramid.read_region`` stands in for openslide: the
level-pixel origin of a level-0 location is ``int(level0 / downsample)``, pixels outside the level are 0 (transparent -> black after
``.convert('RGB')``); unpinned against openslide for downsamples that are no integers.

The loops are the reference's statement by statement; only the file output (``.save``, ``os.makedirs``) is left out.
"""
import numpy as np

from _colour_ref import as_float, rgb2hsv

XYZ_FROM_RGB = np.array([[0.412453, 0.357580, 0.180423], [0.212671, 0.715160, 0.072169], [0.019334, 0.119193, 0.950227]])
D65_2 = (0.95047, 1.0, 1.08883)                                     # get_xyz_coords("D65", "2")
SORTING_ORDERS = [[0, 1, 2], [0, 2, 1], [1, 2, 0], [1, 0, 2], [2, 0, 1], [2, 1, 0]]


# ------------------------------------------------------------------------------------------------ CIELAB a*
def rgb2xyz(img_u8):
    """skimage 0.15.0 rgb2xyz on a uint8 image: img_as_float, the sRGB linearisation, ``arr @ xyz_from_rgb.T``"""
    arr = as_float(img_u8)
    mask = arr > 0.04045
    arr[mask] = np.power((arr[mask] + 0.055) / 1.055, 2.4)
    arr[~mask] /= 12.92
    return arr @ XYZ_FROM_RGB.T.copy()


def lab_a(img_u8):
    """-> float64 [H, W]: channel 1 of skimage 0.15.0 rgb2lab (xyz2lab with D65 / 2): a* = 500 (f(X / Xn) - f(Y / Yn))"""
    arr = rgb2xyz(img_u8) / np.array(D65_2)
    mask = arr > 0.008856
    arr[mask] = np.power(arr[mask], 1.0 / 3.0)
    arr[~mask] = 7.787 * arr[~mask] + 16.0 / 116.0
    return 500.0 * (arr[..., 0] - arr[..., 1])


def lab_a_rows(img_u8):
    """the same chain with the matrix product written as the row-by-column loop the device evaluates (no BLAS in it): the operand the
    device is compared with.  ``lab_a`` (NumPy's matmul) differs from it by rounding only (tests/test_mining_cpu.py bounds it)."""
    arr = as_float(img_u8)
    mask = arr > 0.04045
    arr[mask] = np.power((arr[mask] + 0.055) / 1.055, 2.4)
    arr[~mask] /= 12.92
    f = []
    for row, white in zip(XYZ_FROM_RGB[:2], D65_2[:2]):
        t = ((arr[..., 0] * row[0] + arr[..., 1] * row[1]) + arr[..., 2] * row[2]) / white
        m = t > 0.008856
        out = 7.787 * t + 16.0 / 116.0
        out[m] = np.power(t[m], 1.0 / 3.0)
        f.append(out)
    return 500.0 * (f[0] - f[1])


# ------------------------------------------------------------------------------------------------ isforeground, both forms
def foreground_pixels_v1(tile_u8, mu, mu_percent=0.15):
    """util.py:20-21: ``lab[..., 1] > (1 + mu_percent) * mu``"""
    return lab_a_rows(tile_u8) > (1 + mu_percent) * mu


def foreground_pixels_v2(tile_u8, mu_percent=0.1):
    """Pretraining_v2/util.py:11-12: ``hsv[..., 1] > mu_percent``"""
    return rgb2hsv(as_float(tile_u8))[..., 1] > mu_percent


def isforeground_v1(tile_u8, mu, mu_percent=0.15, thresh=0.95):
    lab = foreground_pixels_v1(tile_u8, mu, mu_percent)
    return np.count_nonzero(lab) / lab.size >= thresh


def isforeground_v2(tile_u8, mu_percent=0.1, thresh=0.75):
    hsv = foreground_pixels_v2(tile_u8, mu_percent)
    return np.count_nonzero(hsv) / hsv.size >= thresh


def mean_a(overview_u8):
    """dataset.py:402-403: ``mu = np.mean(lab[..., 1])``"""
    return np.mean(lab_a_rows(overview_u8))


# ------------------------------------------------------------------------------------------------ an in-memory slide
class Pyramid:
    """what the loops need of an openslide handle: levels[l] uint8 [H, W, 3], level_downsamples, level_dimensions (w, h), read_region"""

    def __init__(self, levels, downsamples, overview=None):
        self.levels = [np.ascontiguousarray(lv) for lv in levels]
        self.level_downsamples = tuple(float(d) for d in downsamples)
        self.level_dimensions = tuple((lv.shape[1], lv.shape[0]) for lv in self.levels)
        self.level_count = len(self.levels)
        self.overview = overview

    def level_origin(self, location, level):
        ds = self.level_downsamples[level]
        return int(location[0] / ds), int(location[1] / ds)

    def read_region(self, location, level, size, fill=0):
        img = self.levels[level]
        x0, y0 = self.level_origin(location, level)
        w, h = size
        out = np.full((h, w, 3), fill, np.uint8)
        ys, xs = np.arange(y0, y0 + h), np.arange(x0, x0 + w)
        yin, xin = (ys >= 0) & (ys < img.shape[0]), (xs >= 0) & (xs < img.shape[1])
        out[np.ix_(yin, xin)] = img[np.ix_(ys[yin], xs[xin])]
        return out


def getitem_v1(scan, x, y, tile_w, tile_h, levels=(0, 1, 2)):
    """dataset.py:322-384 -> (lr2, lr1, hr) tiles and their level-0 locations"""
    hr_level, lr_level_1, lr_level_2 = levels
    m = scan.level_downsamples[lr_level_2]
    loc_lr2 = (int(m * x), int(m * y))
    mlr = scan.level_downsamples[lr_level_1]
    left, up = int(int(int(m * (x + (tile_w / 2))) / mlr) * mlr), int(
        int(int(m * (y + (tile_h / 2))) / mlr) * mlr)
    mhr = scan.level_downsamples[hr_level]
    left_hr, up_hr = int(int(int(m * (x + (tile_w / 2))) / mhr) * mhr), int(
        int(int(m * (y + (tile_h / 2))) / mhr) * mhr)
    return loc_lr2, (left, up), (left_hr, up_hr)


def getitem_v2(scan, x, y, tile_w, tile_h, levels=(0, 1, 2)):
    """Pretraining_v2/dataset.py:219-266"""
    hr_level, lr_level_1, lr_level_2 = levels
    m = scan.level_downsamples[lr_level_2]
    loc_lr2 = (int(m * x), int(m * y))
    mlr = scan.level_downsamples[lr_level_1]
    left, up = int(int(int(int(m * (x + (tile_w / 2))) / mlr) - int(tile_w / 2)) * mlr), int(int(int(int(m * (y + (tile_h / 2))) / mlr) - int(tile_h / 2)) * mlr)
    mhr = scan.level_downsamples[hr_level]
    left_hr, up_hr = int(int(int(int(m * (x + (tile_w / 2))) / mhr) - int(tile_w / 2)) * mhr), int(int(int(int(m * (y + (tile_h / 2))) / mhr) - int(tile_h / 2)) * mhr)
    return loc_lr2, (left, up), (left_hr, up_hr)


def get_wsi_patches(scan, tile, stride, variant, fill=0, mu_percent=None, thresh=None):
    """both ``get_wsi_patches`` loops (dataset.py:386-446 with scan.overview as the lowest-level image; Pretraining_v2/dataset.py:268-316)
    -> (image_tiles_hr, image_tiles_lr1, image_tiles_lr2, kept) with the tiles uint8 [T, tile, tile, 3] (empty lists where nothing is
    kept, as the reference) and kept = [(xpos, ypos)] in visiting order"""
    tile_h = tile_w = tile
    sh, sw = (stride, stride) if np.isscalar(stride) else stride
    kw = {k: v for k, v in (("mu_percent", mu_percent), ("thresh", thresh)) if v is not None}
    if variant == "v1":
        mu = mean_a(scan.overview)
    iw, ih = scan.level_dimensions[2]
    ph, pw = tile_h, tile_w
    image_tiles_hr, image_tiles_lr1, image_tiles_lr2, kept = [], [], [], []
    for ypos in range(sh, ih - 1 - ph, sh):
        for xpos in range(sw, iw - 1 - pw, sw):
            xph, yph = int(scan.level_downsamples[2] * xpos), int(scan.level_downsamples[2] * ypos)
            wsi = scan.read_region((xph, yph), 2, (tile_w, tile_h), fill)
            fg = isforeground_v1(wsi, mu, **kw) if variant == "v1" else isforeground_v2(wsi, **kw)
            if fg:
                locs = (getitem_v1 if variant == "v1" else getitem_v2)(scan, xpos, ypos, tile_w, tile_h)
                image_tiles_lr2.append(scan.read_region(locs[0], 2, (tile_w, tile_h), fill))
                image_tiles_lr1.append(scan.read_region(locs[1], 1, (tile_w, tile_h), fill))
                image_tiles_hr.append(scan.read_region(locs[2], 0, (tile_w, tile_h), fill))
                kept.append((xpos, ypos))
    if len(image_tiles_hr) != 0:
        image_tiles_hr = np.stack(image_tiles_hr, axis=0).astype('uint8')
        image_tiles_lr1 = np.stack(image_tiles_lr1, axis=0).astype('uint8')
        image_tiles_lr2 = np.stack(image_tiles_lr2, axis=0).astype('uint8')
    return image_tiles_hr, image_tiles_lr1, image_tiles_lr2, kept


def sorted_sequence(all_image_tiles_hr, all_image_tiles_lr1, all_image_tiles_lr2):
    """dataset.py:27-70"""
    Data_1, Data_2, Data_3, Class_labels = [], [], [], []
    for index in range(len(all_image_tiles_hr)):
        tuple_images = [all_image_tiles_hr[index], all_image_tiles_lr1[index], all_image_tiles_lr2[index]]
        sorting_orders = SORTING_ORDERS
        labels = [0, 1, 2, 3, 4, 5]
        for i in range(len(sorting_orders)):
            img_ordering = sorting_orders[i]
            Class_ids = np.array([labels[i]])
            Data_1.append(tuple_images[img_ordering[0]])
            Data_2.append(tuple_images[img_ordering[1]])
            Data_3.append(tuple_images[img_ordering[2]])
            Class_labels.append([Class_ids])
    Data_1 = np.stack(Data_1, axis=0).astype('uint8')
    Data_2 = np.stack(Data_2, axis=0).astype('uint8')
    Data_3 = np.stack(Data_3, axis=0).astype('uint8')
    Class_labels = np.stack(Class_labels, axis=0).astype('uint8')
    return Data_1, Data_2, Data_3, Class_labels


# ------------------------------------------------------------------------------------------------ a synthetic slide
def synthetic_pyramid(seed, w2=134, h2=90, factor=2, downsamples=None):
    """-> Pyramid of three levels, level 2 of w2 x h2 pixels and each level above ``factor`` times as large, with an overview image at
    half the size of level 2.  Every level draws its own pixels over the SAME geometry: a near-white background N(242, 3) per channel,
    pink tissue discs N((180, 110, 160), 8) (``_discs``: two large ones, seed 1 one that is smaller than any tile), and 1 % white
    speckle over everything.  Measured on the CPU at the default size: seeds 0, 2 and 3 keep 25-43 of the 126 (tile 16 / stride 8) and
    144 (tile 20 / stride 7) candidates under either criterion, up to 6 of them within 2 % of the threshold; seed 1 keeps none; no
    level-2 pixel of seeds 0-3 has a* within 1e-9 of 1.15 mu; NumPy's matmul moves a* by at most 1.2e-13 against ``lab_a_rows``."""
    rs = np.random.RandomState(seed)
    discs = _discs(rs, seed)
    sizes = [(w2 * factor * factor, h2 * factor * factor), (w2 * factor, h2 * factor), (w2, h2), (w2 // 2, h2 // 2)]
    imgs = []
    for w, h in sizes:
        yy, xx = np.mgrid[0:h, 0:w]
        u, v = (xx + 0.5) / w, (yy + 0.5) / h                       # geometry in units of the image
        tissue = np.zeros((h, w), bool)
        for cx, cy, r in discs:
            tissue |= (u - cx) ** 2 * (w2 / h2) ** 2 + (v - cy) ** 2 <= r * r
        img = rs.normal(242, 3, (h, w, 3))
        img[tissue] = rs.normal((180, 110, 160), 8, (int(tissue.sum()), 3))
        img[rs.random_sample((h, w)) < 0.01] = 255
        imgs.append(np.clip(img, 0, 255).astype(np.uint8))
    if downsamples is None:
        downsamples = (1.0, float(factor), float(factor * factor))
    return Pyramid(imgs[:3], downsamples, overview=imgs[3])


def _discs(rs, seed):
    """(cx, cy, r) in units of the image (r in units of its height).  Seed 1 is the slide without usable tissue: one disc smaller than
    any tile the tests use."""
    if seed == 1:
        return [(0.5, 0.5, 0.04)]
    return [(rs.uniform(0.25, 0.75), rs.uniform(0.3, 0.7), rs.uniform(0.22, 0.38)) for _ in range(2)]
