#!/usr/bin/env python
"""Generate tests/golden/randaug_v2.npz by running the REFERENCE's own RSP v2 RandAugment ops (Pretraining_v2/models/randaugment.py)
on small seeded images.

Run in the build container only (needs the reference checkout and Pillow):   python tests/golden/make_randaug_v2.py
The reference's Python never travels; only the input / output arrays written here do.

Aids (none of them reference source): MagicMock stubs for ``skimage`` (and ``scipy`` where missing), which only the two colour
augmenters behind ``hed`` / ``hsv`` import -- those two ops are not recorded.  The goldens pin the Pillow that is installed where
this runs (recorded as ``pillow_version``; 12.2.0 for the committed file); the reference's own environment pins an older Pillow.

Layout of the file (arrays only):
  pool                 the op names in augment_pool() order
  img_<j>              input images, [H, W, 3] uint8
  op_case              [K, 4] int64: (pool index, image index, ``random`` seed set before the call, sign drawn: 1 / 0, -1 = none)
  op_val               [K] float64: the raw ``val`` handed to the op function
  op_out_<j>           [K_j, H, W, 3]: the op function's outputs for the cases of image j, in case order
  pipe_case            [P, 4] int64: (n, m, image index, seed for random.seed and np.random.seed before RandAugment(n, m)(img))
  pipe_out_<p>         [H, W, 3]: the output of that call
"""
import contextlib
import importlib
import importlib.abc
import importlib.machinery
import io
import os
import random
import sys
from unittest import mock

import numpy as np
import PIL

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("SSLCR_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.join(REF, "Pretraining_v2"))

STUBS = ["skimage"]
try:
    import scipy  # noqa: F401
except ImportError:
    STUBS.append("scipy")


class _StubFinder(importlib.abc.MetaPathFinder, importlib.abc.Loader):
    def find_spec(self, name, path=None, target=None):
        if name.split(".")[0] in STUBS:
            return importlib.machinery.ModuleSpec(name, self, is_package=True)
        return None

    def create_module(self, spec):
        m = mock.MagicMock(name=spec.name)
        m.__path__ = []
        m.__name__ = spec.name
        m.__spec__ = spec
        return m

    def exec_module(self, module):
        pass


sys.meta_path.insert(0, _StubFinder())
ra = importlib.import_module("models.randaugment")

POOL = [f.__name__ for f, _, _ in ra.augment_pool()]
SIGNED = ("rotate", "translate_x", "translate_y", "shear_x", "shear_y")
ENHANCE = ("contrast", "brightness", "sharpness", "color")
HOST = ("hed", "hsv")


def images():
    rs = np.random.RandomState(20240)
    out = [rs.randint(0, 256, (17, 33, 3)),                                    # odd, H != W
           rs.randint(0, 256, (48, 40, 3)),
           rs.randint(0, 256, (32, 40, 3)),                                    # one constant channel
           rs.randint(60, 124, (24, 20, 3)),                                   # narrow range 60..123
           rs.randint(0, 256, (16, 15, 3)),                                    # 240 pixels: equalize's step is 0
           np.add.outer(np.arange(20) * 7, np.arange(28) * 5)[..., None] + np.array([0, 60, 130])]      # structured ramps
    out[2][..., 1] = 77
    return [np.ascontiguousarray(a.astype(np.uint8)) for a in out]


def seed_with_sign(sign, start):
    s = start
    while True:
        random.seed(s)
        if random.choice([1, 0]) == sign:
            return s
        s += 1


def main():
    imgs = images()
    arrays = {"pool": np.array(POOL), "pillow_version": np.array(PIL.__version__)}
    for j, im in enumerate(imgs):
        arrays[f"img_{j}"] = im
    cases, vals, outs = [], [], {j: [] for j in range(len(imgs))}
    for name in POOL:
        if name in HOST:
            continue
        fn = getattr(ra, name)
        if name in ENHANCE:
            grid = [(v, None) for v in (1.0, 3.3, 5.0, 9.5)]                  # factor 0.28, 0.694, exactly 1.0, 1.81
        elif name in SIGNED:
            grid = [(v, s) for v in (2.3, 10.0) for s in (1, 0)]
        else:
            grid = [(1.0, None)]
        for j, im in enumerate(imgs):
            for k, (v, sign) in enumerate(grid):
                seed = 1000 * len(cases) + 7 if sign is None else seed_with_sign(sign, 1000 * len(cases) + 7)
                random.seed(seed)
                out = np.asarray(fn(im.copy(), v))
                assert out.shape == im.shape and out.dtype == np.uint8, (name, out.shape, out.dtype)
                cases.append((POOL.index(name), j, seed, -1 if sign is None else sign))
                vals.append(v)
                outs[j].append(out.copy())
    arrays["op_case"] = np.array(cases, dtype=np.int64)
    arrays["op_val"] = np.array(vals, dtype=np.float64)
    for j, o in outs.items():
        arrays[f"op_out_{j}"] = np.stack(o)

    # whole RandAugment(n, m) calls; only seeds whose sample avoids hed / hsv (those two need scikit-image)
    pipe = []
    for n, m in ((2, 3), (3, 10)):
        seed, found = 0, 0
        while found < 6:
            seed += 1
            random.seed(seed)
            names = [f.__name__ for f, _, _ in random.sample(ra.augment_pool(), k=n)]
            if any(nm in HOST for nm in names):
                continue
            j = found % len(imgs)
            random.seed(seed)
            np.random.seed(seed)
            with contextlib.redirect_stdout(io.StringIO()):                    # the reference prints every val
                out = np.asarray(ra.RandAugment(n, m)(imgs[j].copy()))
            arrays[f"pipe_out_{len(pipe)}"] = out.copy()
            pipe.append((n, m, j, seed))
            found += 1
    arrays["pipe_case"] = np.array(pipe, dtype=np.int64)
    path = os.path.join(HERE, "randaug_v2.npz")
    np.savez_compressed(path, **arrays)
    print(f"wrote {path}: {len(cases)} op cases, {len(pipe)} pipeline cases, Pillow {PIL.__version__}, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
