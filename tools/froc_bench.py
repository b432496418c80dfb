#!/usr/bin/env python
"""Stream time of the lesion-scoring kernels (csrc/froc.hip) and of the host code they replace, in one process.

    python tools/froc_bench.py [--iters 20] [--iters-nms 5] [--radius 12] [--sigma 1.0] [--out profiles/froc_bench.json]

Input: the 1536 x 3072 truth mask of tools/annotation_bench.py's polygon set (48 star-shaped polygons at resolution 64), and a
synthetic probability map of that shape: 1.0f on 95 % of the cells inside the polygons (the plateaus a saturated softmax leaves),
uniform noise below 0.45 elsewhere, and one cell in a thousand raised to a random value in (0.5, 1) (stray peaks).
Figures, each with median / min / max of HIP events around ONE call over ``launches`` calls after two warm-up calls:
  label_c2 / label_c1   kernels.label_components (six launches) at connectivity 2 / 1; ``bytes`` = 5 per cell, the mask read once and
                        the labels written once; ``components``; ``scipy_ms`` = scipy.ndimage.label on this host, ``equal`` its answer
  smooth                kernels.gaussian_smooth (two launches), ``bytes`` = 16 per cell (two passes, read and write)
  nms                   kernels.nms whole, host reads included (HIP events around the call; ``--iters-nms`` calls), per ``read_every``:
                        ``rounds`` / ``host_reads`` / ``candidates`` / ``detections``; the default ``read_every`` is the best found
  nms_numpy_ms          the sequential NumPy loop of tests/_froc_ref.py on this host; ``nms_equal`` = the device's list is its list
  hits                  kernels.lesion_hits (one launch, areas included), ``bytes`` = 4 per cell
  lesion_scores         inference.lesion_scores whole, from device tensors to the host dict
  byte_compare          the yardstick the README quotes for streaming kernels: ``torch.eq`` of two uint8 tensors of 4 bytes per cell
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


def bench(a):
    import torch
    import _froc_ref as R
    from annotation_bench import MASK, RESOLUTION, make_annotation, timed
    from ssl_cr_histo_amd import inference as I
    from ssl_cr_histo_amd import kernels as K
    from ssl_cr_histo_amd.annotation import Annotation
    if not torch.cuda.is_available():
        raise SystemExit("froc_bench: no GPU visible; nothing here is measured without one")
    dev = torch.device("cuda", 0)
    truth = Annotation().from_vertices(make_annotation(a.seed)).to_device(dev).mask(MASK, RESOLUTION)
    th = truth.cpu().numpy() != 0
    n = th.size
    rs = np.random.RandomState(a.seed + 2)
    pm = (rs.rand(*MASK) * 0.45).astype(np.float32)
    peaks = rs.rand(*MASK) < 0.001
    pm[peaks] = (0.5 + 0.499 * rs.rand(int(peaks.sum()))).astype(np.float32)
    pm[th & (rs.rand(*MASK) < 0.95)] = 1.0
    pmd = torch.from_numpy(pm).to(dev)
    res = dict(tool="froc_bench", device=torch.cuda.get_device_name(0), mask=list(MASK), cells=n, inside_share=float(th.mean()),
               radius=a.radius, sigma=a.sigma, threshold=0.5)

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

    # ---- components
    from scipy import ndimage as ndi
    for c in (2, 1):
        labels, count = K.label_components(truth, c)
        st = rated(timed(lambda: K.label_components(truth, c), a.iters), 5 * n)
        st["components"] = int(count.item())
        t0 = time.time()
        want, nl = ndi.label(th, ndi.generate_binary_structure(2, c))
        st["scipy_ms"] = (time.time() - t0) * 1e3
        st["equal"] = bool(nl == st["components"] and np.array_equal(labels.cpu().numpy(), want))
        res[f"label_c{c}"] = st
    labels, count = K.label_components(truth, 2)
    nl = int(count.item())

    # ---- smoothing
    res["smooth"] = rated(timed(lambda: K.gaussian_smooth(pmd, a.sigma), a.iters), 16 * n)
    res["smooth"]["taps"] = len(K.gaussian_weights(a.sigma))

    # ---- NMS, on the map as given (the plateaus stay exact), per read_every
    cap = a.max_detections

    rows = {}
    for every in (1, 2, 4, 8, 16, 32, 64):
        stats = {}
        k = K.nms(pmd, 0.5, a.radius, cap, read_every=every, stats=stats)[2]
        row = timed(lambda: K.nms(pmd, 0.5, a.radius, cap, read_every=every), a.iters_nms)
        row.update(stats, detections=k)
        rows[str(every)] = row
    res["nms"] = rows
    res["nms_best_read_every"] = int(min(rows.items(), key=lambda kv: kv[1]["median_ms"])[0])
    det_xy, det_prob, k = K.nms(pmd, 0.5, a.radius, cap)
    t0 = time.time()
    want = R.nms(pm, 0.5, a.radius)
    res["nms_numpy_ms"] = (time.time() - t0) * 1e3
    xy, pr = det_xy.cpu().numpy(), det_prob.cpu().numpy()
    res["nms_equal"] = bool([(int(xy[i, 0]), int(xy[i, 1]), float(pr[i])) for i in range(k)] == want)

    # ---- hits and the whole
    res["hits"] = rated(timed(lambda: K.lesion_hits(labels, nl, det_xy, det_prob, k), a.iters), 4 * n)
    res["lesion_scores"] = timed(lambda: I.lesion_scores(pmd, truth, threshold=0.5, radius=a.radius, sigma=0.0, max_detections=cap), a.iters)
    res["lesion_scores_smoothed"] = timed(lambda: I.lesion_scores(pmd, truth, threshold=0.5, radius=a.radius, sigma=a.sigma,
                                                                  max_detections=cap), a.iters)
    got = I.lesion_scores(pmd, truth, threshold=0.5, radius=a.radius, max_detections=cap)
    res["lesions"], res["lesions_hit"], res["false_positives"] = nl, int((got["tp_prob"] > 0).sum()), int(len(got["fp_prob"]))
    res["froc_score_one_slide"] = I.froc(got["fp_prob"], got["tp_prob"], 1, nl)["score"]
    return res


def dump(res, path):
    line = json.dumps(res)
    if path:
        with open(path, "w") as f:
            f.write(line + "\n")
    return line


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--iters-nms", type=int, default=5)
    p.add_argument("--radius", type=int, default=12)
    p.add_argument("--sigma", type=float, default=1.0)
    p.add_argument("--max-detections", type=int, default=16384)
    p.add_argument("--seed", type=int, default=7)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    print(dump(bench(a), a.out))


if __name__ == "__main__":
    main()
