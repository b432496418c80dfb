"""Shared by tests/golden/make_resize_golden.py and the resize tests: the seeded inputs, the case table of the kernel tests, and
``expected`` -- Pillow's answer, live where Pillow imports, else the recorded one (tests/golden/resize_pil.npz, Pillow 12.2.0), else
the NumPy restatement (tests/_resize_ref.py, which tests/test_resize_cpu.py holds equal to Pillow)."""
import os

import numpy as np

import _resize_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resize_pil.npz")
FILTERS = ("box", "bilinear", "hamming", "bicubic", "lanczos")

# name -> (H, W, seed, binary): binary = an image of 0 / 255 only, so that bicubic and lanczos overshoot and clip at both ends
SOURCES = {"bw64": (64, 64, 101, True), "r37": (37, 53, 102, False), "r9": (9, 7, 103, False), "r33": (33, 65, 104, False)}


def source(name):
    h, w, seed, binary = SOURCES[name]
    rs = np.random.RandomState(seed)
    if binary:
        return (rs.randint(0, 2, size=(h, w, 3)) * 255).astype(np.uint8)
    return rs.randint(0, 256, size=(h, w, 3), dtype=np.uint8)


def big_source(h, w):
    """a deterministic uint8 [h, w, 3] too large to record: a multiplicative hash of the index"""
    i = np.arange(h * w * 3, dtype=np.uint64)
    return ((i * np.uint64(2654435761) >> np.uint64(11)) & np.uint64(255)).astype(np.uint8).reshape(h, w, 3)


def frac_box(h, w):
    return (1.25, 0.5, w - 0.75, h - 1.5)


# (id, source, (oh, ow), box): the smallest shapes at which each thing can still go wrong
CASES = [("down2", "bw64", (32, 32), None),             # an even down-scale of the 0 / 255 image
         ("odd", "r37", (19, 27), None),                # odd, non-integer scale; windows clipped at both edges; OW % 4 != 0, pitch 159
         ("up", "r9", (19, 27), None),                  # up-scale: filterscale clamped to 1
         ("h_only", "r37", (37, 27), None),             # one pass only, each axis
         ("v_only", "r37", (19, 53), None),
         ("one", "r37", (1, 1), None),                  # a window over the whole image
         ("box_same", "r33", (33, 65), frac_box(33, 65))]      # same size, fractional box: both passes
NEAREST_CASES = [("bw64", (32, 32)), ("r37", (19, 27)), ("r9", (19, 27)), ("r37", (37, 27)), ("r37", (1, 1))]
# five boxes for one launch over five images of r37-sized sources -> (19, 27)
BOXES5 = [(0.0, 0.0, 53.0, 37.0), (1.25, 0.5, 52.25, 35.5), (10.0, 3.0, 40.5, 30.25), (0.0, 0.0, 26.5, 18.5), (20.0, 10.0, 53.0, 37.0)]
BOX_FILTERS = ("bilinear", "bicubic")
BIG_CASES = [((8, 8192), (8, 8)), ((9, 8192), (8, 8))]          # LANCZOS; (h, w) -> (oh, ow): one pass / both passes, far past the fused LDS
LOADER = dict(n=10, hw=64, image_size=32, batch_size=4, seed=105)
# What tests/golden/resize_pil.npz records, (source, (oh, ow), filter, box): the small cases of every filter, and each larger thing
# once -- the clipped overshoot, each single pass, the same-size box, a per-image box, NEAREST.  A case that is not recorded falls
# through to the restatement, which tests/test_resize_cpu.py holds equal to Pillow and to every recorded array.
RECORDED_INPUTS = ("r37", "r9")
RECORDED = [(s, hw, f, b) for f in FILTERS for cid, s, hw, b in CASES if cid in ("odd", "up", "one")] + \
           [("bw64", (32, 32), f, None) for f in ("bicubic", "lanczos")] + \
           [("r37", (37, 27), "bilinear", None), ("r37", (19, 53), "bilinear", None), ("r33", (33, 65), "bilinear", frac_box(33, 65)),
            ("r37", (19, 27), "bilinear", BOXES5[2]), ("r37", (19, 27), "nearest", None), ("r9", (19, 27), "nearest", None)]


def loader_patches():
    c = LOADER
    return np.random.RandomState(c["seed"]).randint(0, 256, size=(c["n"], c["hw"], c["hw"], 3), dtype=np.uint8)


def key(src, out_hw, name, box):
    b = "full" if box is None else ",".join(f"{v:g}" for v in box)
    return f"{src}|{out_hw[0]}x{out_hw[1]}|{name}|{b}"


def pillow():
    try:
        from PIL import Image
        return Image
    except ImportError:
        return None


def pil_resize(img, out_hw, name, box=None):
    """the live Pillow; img uint8 [H, W] or [H, W, 3]"""
    Image = pillow()
    return np.asarray(Image.fromarray(img).resize((out_hw[1], out_hw[0]), getattr(Image, name.upper()), box=box))


_golden = None


def golden():
    global _golden
    if _golden is None:
        with np.load(GOLDEN) as z:
            _golden = {k: z[k] for k in z.files}
    return _golden


def expected(img, out_hw, name, box=None, k=None):
    """Pillow's resize of img (uint8 [H, W, 3], or [H, W]: mode L): live, else recorded under ``k`` (recorded for RGB; an L image is
    then channel 0 of its RGB source, and resizing is per channel), else restated"""
    if pillow() is not None:
        return pil_resize(img, out_hw, name, box)
    if k is not None and k in golden():
        g = golden()[k]
        return g if img.ndim == 3 else g[..., 0]
    return R.resize(img, (out_hw[1], out_hw[0]), name, box)
