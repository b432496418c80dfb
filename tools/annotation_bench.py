#!/usr/bin/env python
"""Stream time of the annotation kernels (ssl_cr_histo_amd/annotation.py) and the host loop they replace, in one process.

    python tools/annotation_bench.py [--iters 20] [--iters-uncut 5] [--threads 16] [--sub-mask 16384] [--sub-centres 8192]
                                     [--out profiles/annotation_bench.json]

Input: a seeded synthetic annotation of 48 star-shaped polygons with 64 ... 4096 integer vertices each (about 60 k vertices), radii
1 500 ... 15 000 level-0 pixels, in a 98 304 x 196 608 level-0 frame.  Figures, each with median / min / max of HIP events around ONE
launch over ``launches`` launches after two warm-up launches:
  mask_*      the truth mask 1536 x 3072 at resolution 64 (the kernel's grid source) -- ``exact`` (the integer path) and ``f64`` (the
              chain as written), each with the cull (``cull``: the polygons' bounds) and without (``uncut``: bounds = None; these
              launches run for a good part of a second, so ``--iters-uncut`` of them)
  centres_*   200 000 explicit random integer centres, with the cull, both paths
  confusion   sslcr_map_confusion with 64 thresholds on a random map of the mask's shape, the truth mask above, 70 % tissue
``edge_tests`` is points x vertices, what a loop without any cull evaluates.  ``edge_tests_executed`` counts what the launch did
evaluate, lane slots included: for every wave (64 points: an 8 x 8 block of cells, or 64 consecutive centres) and every polygon the
wave walks -- a lane inside the polygon's bounds (when given) that no earlier polygon holds -- 64 x the polygon's vertices; recomputed on
the host from the kernel's own ``first`` output.  ``edge_tests_culled`` is the difference, ``tests_per_s`` = executed / median.
  numpy_*     the restatement of tests/_annotation_ref.py (one polygon at a time over all points, first hit kept) on ``--threads``
              threads of this host over a SUBSAMPLE of the points (``subsample`` of them, evenly spaced), ``scaled_ms`` = its time x
              points / subsample; ``equal`` says whether the device's answers on the subsample are the restatement's.
Prints one JSON line; --out also writes it."""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FRAME = (98304, 196608)
MASK, RESOLUTION = (1536, 3072), 64


def make_annotation(seed):
    rs = np.random.RandomState(seed)
    sizes = (64 + (4096 - 64) * np.linspace(0, 1, 48) ** 2.3).round().astype(int)
    polys = []
    for n in rs.permutation(sizes):
        radius = rs.uniform(1500, 15000)
        centre = (rs.uniform(radius, FRAME[0] - radius), rs.uniform(radius, FRAME[1] - radius))
        ang = np.sort(rs.uniform(0, 2 * np.pi, n))
        r = rs.uniform(0.6, 1.0, n) * radius
        polys.append(np.round(np.stack([centre[0] + r * np.cos(ang), centre[1] + r * np.sin(ang)], 1)))
    return polys


def timed(fn, iters):
    """HIP events around each of ``iters`` calls (after two warm-up calls), one synchronise at the end -> ms stats"""
    import torch
    fn(); fn()
    torch.cuda.synchronize()
    pairs = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        pairs.append((e0, e1))
    torch.cuda.synchronize()
    v = sorted(x.elapsed_time(y) for x, y in pairs)
    return dict(median_ms=v[len(v) // 2], min_ms=v[0], max_ms=v[-1], launches=len(v))


def executed(points_by_wave, first_by_wave, sizes, bounds):
    """lane slots the launch evaluated: per wave [W, 64] of points and first hits, per polygon 64 x vertices where any lane is wanted"""
    x, y = points_by_wave[..., 0], points_by_wave[..., 1]
    valid = ~np.isnan(x)
    total = 0
    for q, n in enumerate(sizes):
        want = valid & ((first_by_wave < 0) | (first_by_wave >= q))
        if bounds is not None:
            b = bounds[q]
            want &= (x >= b[0]) & (y >= b[1]) & (x <= b[2]) & (y <= b[3])
        total += int(want.any(1).sum()) * 64 * int(n)
    return total


def grid_waves(nx, ny, step, first):
    """the kernel's lane map of the grid source: 8 x 8 cells per wave; cells past the mask are NaN"""
    tx, ty = (nx + 7) // 8, (ny + 7) // 8
    xs = np.full(tx * 8, np.nan)
    ys = np.full(ty * 8, np.nan)
    xs[:nx] = np.arange(nx) * step
    ys[:ny] = np.arange(ny) * step
    px = np.broadcast_to(xs[:, None], (tx * 8, ty * 8))
    py = np.broadcast_to(ys[None, :], (tx * 8, ty * 8))
    px = np.where(np.isnan(py), np.nan, px)
    f = np.full((tx * 8, ty * 8), -1, dtype=np.int32)
    f[:nx, :ny] = first

    def waves(a):
        return a.reshape(tx, 8, ty, 8).transpose(0, 2, 1, 3).reshape(tx * ty, 64)
    return np.stack([waves(px), waves(py)], -1), waves(f)


def list_waves(pts, first):
    n = len(pts)
    w = (n + 63) // 64
    p = np.full((w * 64, 2), np.nan)
    p[:n] = pts
    f = np.full(w * 64, -1, dtype=np.int32)
    f[:n] = first
    return p.reshape(w, 64, 2), f.reshape(w, 64)


def numpy_first(pts, polys, threads):
    import _annotation_ref as R
    parts = np.array_split(pts, threads)
    t0 = time.time()
    with ThreadPoolExecutor(threads) as pool:
        out = list(pool.map(lambda p: R.inside_first(p, polys)[1], parts))
    return np.concatenate(out), time.time() - t0


def bench(a):
    import torch
    from ssl_cr_histo_amd import kernels as K
    from ssl_cr_histo_amd.annotation import Annotation
    if not torch.cuda.is_available():
        raise SystemExit("annotation_bench: no GPU visible; nothing here is measured without one")
    dev = torch.device("cuda", 0)
    polys = make_annotation(a.seed)
    ann = Annotation().from_vertices(polys).to_device(dev)
    vertices, offsets, bounds, vexact = ann._on_device(True)
    host_bounds = ann.packed(True)[2]
    sizes = [len(p) for p in polys]
    V = sum(sizes)
    assert vexact
    res = dict(tool="annotation_bench", device=torch.cuda.get_device_name(0), threads=a.threads, polygons=len(polys), vertices=V,
               frame=list(FRAME), mask=list(MASK), resolution=RESOLUTION, chunk=K.PIP_CHUNK)

    def run(key, iters, waves_of, npoints, **kw):
        inside, first = K.points_in_polygons(first=True, **kw)
        torch.cuda.synchronize()
        out = (inside, first)
        st = timed(lambda: K.points_in_polygons(first=True, out=out, **kw), iters)
        pw, fw = waves_of(first.cpu().numpy())
        st["edge_tests"] = int(npoints) * V
        st["edge_tests_executed"] = executed(pw, fw, sizes, host_bounds if kw.get("bounds") is not None else None)
        st["edge_tests_culled"] = st["edge_tests"] - st["edge_tests_executed"]
        st["tests_per_s"] = st["edge_tests_executed"] / (st["median_ms"] * 1e-3)
        res[key] = st
        return inside, first

    # ---- (a) the truth mask
    grid = (0, 0, RESOLUTION, MASK[0], MASK[1])
    common = dict(points=None, vertices=vertices, offsets=offsets, grid=grid)
    outs = {}
    for name, exact in (("exact", True), ("f64", False)):
        for cull, b, iters in (("cull", bounds, a.iters), ("uncut", None, a.iters_uncut)):
            outs[name, cull] = run(f"mask_{name}_{cull}", iters, lambda f: grid_waves(MASK[0], MASK[1], RESOLUTION, f), MASK[0] * MASK[1],
                                   bounds=b, exact=exact, **common)
    truth, first = outs["exact", "cull"]
    res["mask_paths_equal"] = bool(all(torch.equal(first, o[1]) and torch.equal(truth, o[0]) for o in outs.values()))
    res["mask_inside_share"] = float(truth.float().mean())
    flat = np.linspace(0, MASK[0] * MASK[1] - 1, a.sub_mask).astype(np.int64)
    sub = np.stack([(flat // MASK[1]) * RESOLUTION, (flat % MASK[1]) * RESOLUTION], 1).astype(np.float64)
    want, dt = numpy_first(sub, polys, a.threads)
    res["numpy_mask"] = dict(subsample=int(len(sub)), points=MASK[0] * MASK[1], ms=dt * 1e3, scaled_ms=dt * 1e3 * MASK[0] * MASK[1] / len(sub),
                             equal=bool(np.array_equal(first.cpu().numpy().reshape(-1)[flat], want)))

    # ---- (b) explicit centres
    rs = np.random.RandomState(a.seed + 1)
    centres = np.stack([rs.randint(0, FRAME[0], a.centres), rs.randint(0, FRAME[1], a.centres)], 1).astype(np.float64)
    pts = torch.from_numpy(centres).to(dev)
    for name, exact in (("exact", True), ("f64", False)):
        _, cfirst = run(f"centres_{name}_cull", a.iters, lambda f: list_waves(centres, f), a.centres, points=pts, vertices=vertices,
                        offsets=offsets, bounds=bounds, exact=exact)
    pick = np.linspace(0, a.centres - 1, a.sub_centres).astype(np.int64)
    want, dt = numpy_first(centres[pick], polys, a.threads)
    res["numpy_centres"] = dict(subsample=int(len(pick)), points=a.centres, ms=dt * 1e3, scaled_ms=dt * 1e3 * a.centres / len(pick),
                                equal=bool(np.array_equal(cfirst.cpu().numpy()[pick], want)))

    # ---- (c) the thresholded confusion counts
    g = torch.Generator(device=dev).manual_seed(a.seed)
    pm = torch.rand(MASK, generator=g, device=dev)
    tissue = (torch.rand(MASK, generator=g, device=dev) < 0.7).to(torch.uint8)
    thr = torch.linspace(0, 1, 64, device=dev)
    cm = K.map_confusion(pm, truth, tissue, thr)
    st = timed(lambda: K.map_confusion(pm, truth, tissue, thr), a.iters)          # (each call also zeroes its [64, 2, 2] output)
    st["bytes"] = 6 * MASK[0] * MASK[1]
    st["tbps"] = st["bytes"] / (st["median_ms"] * 1e-3) / 1e12
    t0 = time.time()
    pmh, th, tih, thh = pm.cpu().numpy(), truth.cpu().numpy() != 0, tissue.cpu().numpy() != 0, thr.cpu().numpy()
    want = np.zeros((64, 2, 2), dtype=np.int64)
    for t in range(64):
        ge = pmh[tih] >= thh[t]
        for u in (0, 1):
            for v in (0, 1):
                want[t, u, v] = np.count_nonzero((th[tih] == u) & (ge == v))
    st["numpy_ms"] = (time.time() - t0) * 1e3
    st["equal"] = bool(np.array_equal(cm.cpu().numpy(), want))
    res["confusion"] = st
    for key in ("mask_exact_cull", "centres_exact_cull"):
        res[key]["numpy_scaled_over_device"] = res["numpy_" + key.split("_")[0]]["scaled_ms"] / res[key]["median_ms"]
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--iters-uncut", type=int, default=5)
    p.add_argument("--threads", type=int, default=16)
    p.add_argument("--centres", type=int, default=200000)
    p.add_argument("--sub-mask", type=int, default=16384)
    p.add_argument("--sub-centres", type=int, default=8192)
    p.add_argument("--seed", type=int, default=7)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    res = bench(a)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
