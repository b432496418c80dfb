#!/usr/bin/env python
"""Stream time of the evaluation-mask kernels (csrc/evalmask.hip) and of the host code they replace, in one process.

    python tools/evalmask_bench.py [--iters 20] [--iters-worst 20] [--out profiles/evalmask_bench.json]

Input: the 1536 x 3072 truth mask of tools/annotation_bench.py's polygon set (48 star-shaped polygons at resolution 64), cells of
0.243 * 64 um: the 75 um dilation is the squared-distance limit 6.
Figures, each with median / min / max of HIP events around ONE call over ``launches`` calls after two warm-up calls:
  edt_limit6        kernels.distance_transform_sq(truth, 6, invert=True, below=True) (two launches), what evaluation_mask runs;
                    ``bytes`` = 19 per cell at the least: the mask read by both sweeps (2), the row distances written, read back by
                    the backward sweep and read by the column pass (12), the result (4) and the byte mask (1) written
  edt_unlimited     the unlimited transform of the same mask (distance to the nearest truth cell), 18 bytes per cell; ``scipy_ms`` =
                    scipy.ndimage.distance_transform_edt on this host, ``equal`` = sqrt(float64(result)) has its bits
  edt_lone_zero     the unlimited transform's worst case: one zero cell in the corner of a mask of ones (every column walks to it)
  fill_holes        kernels.fill_holes of the dilated mask (complement, the labeller's six launches, a memset, border, apply);
                    ``bytes`` = 16 per cell (1 + 1, the labeller's 5, 4 memset, 4 + 1); ``scipy_ms`` = binary_fill_holes, ``equal``
  moments           kernels.region_moments over the labels of the filled mask (one launch), ``bytes`` = 4 per cell;
                    ``numpy_ms`` = six np.bincount over the host labels, ``equal``
  evaluation_mask   inference.evaluation_mask whole, from the device truth mask to the host dict (one read of L, one copy);
                    ``scipy_chain_ms`` = the challenge's steps on this host (EDT, threshold, fill, label, bincount moments)
  byte_compare      the yardstick the README quotes for streaming kernels: ``torch.eq`` of two uint8 tensors of 4 bytes per cell
                    (12 bytes per cell moved); ``over_byte_compare`` of a piece = its time / the compare's time for its ``bytes``
Prints one JSON line; --out also writes it."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def host_moments(labels, n):
    l = labels.ravel().astype(np.int64)
    x, y = (v.ravel().astype(np.float64) for v in np.indices(labels.shape))     # every sum stays below 2^53 at this size
    return np.stack([np.bincount(l, weights=w, minlength=n + 1)[1:n + 1] for w in (np.ones_like(x), x, y, x * x, y * y, x * y)],
                    1).astype(np.int64).reshape(n, 6)


def bench(a):
    import torch
    from annotation_bench import MASK, RESOLUTION, make_annotation, timed
    from scipy import ndimage as ndi
    from ssl_cr_histo_amd import inference as I
    from ssl_cr_histo_amd import kernels as K
    from ssl_cr_histo_amd.annotation import Annotation
    if not torch.cuda.is_available():
        raise SystemExit("evalmask_bench: no GPU visible; nothing here is measured without one")
    dev = torch.device("cuda", 0)
    truth = Annotation().from_vertices(make_annotation(a.seed)).to_device(dev).mask(MASK, RESOLUTION)
    th = truth.cpu().numpy() != 0
    n = th.size
    cell_um = 0.243 * RESOLUTION
    limit = K.distance_limit(75.0 / (cell_um * 2.0))
    res = dict(tool="evalmask_bench", device=torch.cuda.get_device_name(0), mask=list(MASK), cells=n, inside_share=float(th.mean()),
               cell_um=cell_um, limit=limit)

    # ---- the yardstick
    u, v = (torch.randint(0, 256, (4 * n,), dtype=torch.uint8, device=dev) for _ in range(2))
    st = timed(lambda: torch.eq(u, v), a.iters)
    st["bytes"] = 12 * n
    st["tbps"] = st["bytes"] / (st["median_ms"] * 1e-3) / 1e12
    res["byte_compare"] = st

    def rated(st, nbytes):
        st["bytes"] = nbytes
        st["tbps"] = nbytes / (st["median_ms"] * 1e-3) / 1e12
        st["over_byte_compare"] = res["byte_compare"]["tbps"] / st["tbps"]
        return st

    # ---- the distance transform: as evaluation_mask runs it, unlimited, and the unlimited worst case
    res["edt_limit6"] = rated(timed(lambda: K.distance_transform_sq(truth, limit, invert=True, below=True), a.iters), 19 * n)
    dist2, binary = K.distance_transform_sq(truth, limit, invert=True, below=True)
    st = rated(timed(lambda: K.distance_transform_sq(truth, None, invert=True), a.iters), 18 * n)
    t0 = time.time()
    want = ndi.distance_transform_edt(~th)
    st["scipy_ms"] = (time.time() - t0) * 1e3
    got = K.distance_transform_sq(truth, None, invert=True).cpu().numpy()
    st["equal"] = bool(np.array_equal(np.sqrt(got.astype(np.float64)).view(np.uint64), want.view(np.uint64)))
    st["max_distance"] = float(np.sqrt(float(got.max())))
    res["edt_unlimited"] = st
    lone = torch.ones(MASK, dtype=torch.uint8, device=dev)
    lone[0, 0] = 0
    st = rated(timed(lambda: K.distance_transform_sq(lone), a.iters_worst), 18 * n)
    xs, ys = np.arange(MASK[0], dtype=np.int64), np.arange(MASK[1], dtype=np.int64)
    st["equal"] = bool(np.array_equal(K.distance_transform_sq(lone).cpu().numpy(), xs[:, None] ** 2 + ys[None, :] ** 2))
    res["edt_lone_zero"] = st
    res["edt_limit6"]["equal"] = bool(np.array_equal(dist2.cpu().numpy(), np.minimum(got, limit)) and
                                      np.array_equal(binary.cpu().numpy() != 0, got < limit))

    # ---- hole filling
    st = rated(timed(lambda: K.fill_holes(binary), a.iters), 16 * n)
    filled = K.fill_holes(binary)
    bh = binary.cpu().numpy() != 0
    t0 = time.time()
    want = ndi.binary_fill_holes(bh)
    st["scipy_ms"] = (time.time() - t0) * 1e3
    st["equal"] = bool(np.array_equal(filled.cpu().numpy() != 0, want))
    st["filled_cells"] = int(want.sum() - bh.sum())
    res["fill_holes"] = st

    # ---- moments
    labels, count = K.label_components(filled, 2)
    nl = int(count.item())
    st = rated(timed(lambda: K.region_moments(labels, nl), a.iters), 4 * n)
    lh = labels.cpu().numpy()
    t0 = time.time()
    want = host_moments(lh, nl)
    st["numpy_ms"] = (time.time() - t0) * 1e3
    st["equal"] = bool(np.array_equal(K.region_moments(labels, nl).cpu().numpy(), want))
    st["components"] = nl
    res["moments"] = st

    # ---- the whole
    st = timed(lambda: I.evaluation_mask(truth, cell_um=cell_um), a.iters)
    ev = I.evaluation_mask(truth, cell_um=cell_um)
    t0 = time.time()
    d = ndi.distance_transform_edt(~th)
    f = ndi.binary_fill_holes(d < 75.0 / (cell_um * 2.0))
    hl, hn = ndi.label(f, structure=np.ones((3, 3)))
    hm = host_moments(hl, hn)
    st["scipy_chain_ms"] = (time.time() - t0) * 1e3
    st["equal"] = bool(hn == ev["n_lesions"] and np.array_equal(ev["labels"].cpu().numpy(), hl) and np.array_equal(ev["moments"], hm))
    st["lesions"], st["itc"] = ev["n_lesions"], int(len(ev["itc"]))
    st["truth_lesions"] = int(K.label_components(truth, 2)[1].item())
    res["evaluation_mask"] = st
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--iters-worst", type=int, default=20)
    p.add_argument("--seed", type=int, default=7)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    line = json.dumps(bench(a))
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
