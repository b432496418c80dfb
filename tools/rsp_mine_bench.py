#!/usr/bin/env python
"""Stream time of device-resident RSP tile mining (ssl_cr_histo_amd/mining.py) and the host pipeline it replaces, in one process.

    python tools/rsp_mine_bench.py [--slide 16384] [--factor 2] [--tile 256] [--stride 128] [--batch 384] [--iters 20] [--threads 16]
                                   [--out profiles/rsp_mine_bench.json]

Inputs: a seeded synthetic slide made on the device -- level 0 of ``--slide`` x ``--slide`` pixels, levels 1 and 2 each ``--factor``
times smaller, an overview image 8 times smaller than level 2 -- from one coarse tissue map (discs of pink N((180, 110, 160), 8) on a
near-white background, 1 % white speckle), every level with its own noise.  Figures, each named for what it is:
  bits_hsv_s / bits_lab_a   HIP events around ONE sslcr_tissue_bits launch over level 2 (lab_a with the threshold read on the device)
  lab_a_sum                 ... around sslcr_lab_a_sum over the overview image (both stages)
  popcount                  ... around sslcr_tile_popcount over the candidate grid
  gather                    ... around ONE sslcr_rsp_gather of ``--batch`` samples (3 x batch tiles), shuffled sample indices
  byte_compare              the yardstick the README quotes for byte kernels: ``torch.eq`` of two uint8 batches of the gather's output
                            size (reads 2 bytes and writes 1 per element), HIP events, same process
Each with median / min / max over ``--iters`` launches after a warm-up, the bytes the kernel must move computed from the shapes, and
the rate that gives (``tbps``: requested bytes, not HBM traffic -- overlapping tiles are served by the caches).
  mine_device               host clock around ``mining.mine_tiles`` on levels already in HBM, ending in the one host read of the keep flags
  mine_numpy                host clock around the predicate loop of ``get_wsi_patches`` (tests/_mining_ref.py: every candidate tile
                            converted on its own, as the reference does) on ``--threads`` threads of this host
for both criteria; ``keep_equal`` says whether the two agree on every candidate.  Prints one JSON line; --out also writes it."""
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


def make_pyramid(a, dev):
    """-> (levels (hr, lr1, lr2), overview), device uint8 [H, W, 3]"""
    import torch
    g = torch.Generator(device=dev).manual_seed(a.seed)
    side2 = a.slide // (a.factor * a.factor)
    coarse = 512
    rs = np.random.RandomState(a.seed)
    yy, xx = np.mgrid[0:coarse, 0:coarse] / coarse
    tissue = np.zeros((coarse, coarse), bool)
    for _ in range(6):
        cx, cy, r = rs.uniform(0.15, 0.85), rs.uniform(0.15, 0.85), rs.uniform(0.08, 0.22)
        tissue |= (xx - cx) ** 2 + (yy - cy) ** 2 <= r * r
    tissue = torch.from_numpy(tissue).to(dev)
    out = []
    for side in (a.slide, a.slide // a.factor, side2, side2 // 8):
        idx = (torch.arange(side, device=dev) * coarse) // side
        m = tissue[idx][:, idx]
        img = torch.empty((side, side, 3), dtype=torch.uint8, device=dev)
        for c, (pink, white) in enumerate(((180, 242), (110, 242), (160, 242))):
            noise = torch.randint(-12, 13, (side, side), generator=g, device=dev, dtype=torch.int16)
            img[..., c] = (torch.where(m, pink, white) + noise).clamp_(0, 255).to(torch.uint8)
        img[torch.rand((side, side), generator=g, device=dev) < 0.01] = 255
        out.append(img)
    return tuple(out[:3]), out[3]


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


def with_rate(stats, nbytes):
    stats["bytes"] = int(nbytes)
    stats["tbps"] = nbytes / (stats["median_ms"] * 1e-3) / 1e12
    return stats


def numpy_keep(lr2, overview, tile, stride, variant, threads):
    """the predicate loop of get_wsi_patches, candidate by candidate, rows of the grid spread over ``threads`` threads"""
    import _mining_ref as MR
    ih, iw = lr2.shape[:2]
    ys, xs = list(range(stride, ih - 1 - tile, stride)), list(range(stride, iw - 1 - tile, stride))
    mu = MR.mean_a(overview) if variant == "v1" else None

    def row(y):
        if variant == "v1":
            return [MR.isforeground_v1(lr2[y:y + tile, x:x + tile], mu) for x in xs]
        return [MR.isforeground_v2(lr2[y:y + tile, x:x + tile]) for x in xs]
    with ThreadPoolExecutor(threads) as pool:
        return np.array(list(pool.map(row, ys)), dtype=bool).reshape(len(ys), len(xs))


def bench(a):
    import torch
    from ssl_cr_histo_amd import kernels as K
    from ssl_cr_histo_amd import mining
    if not torch.cuda.is_available():
        raise SystemExit("rsp_mine_bench: no GPU visible; nothing here is measured without one")
    dev = torch.device("cuda", 0)
    levels, overview = make_pyramid(a, dev)
    torch.cuda.synchronize()
    lr2 = levels[2]
    H, W = lr2.shape[:2]
    S, B = a.tile, a.batch
    ds = (1.0, float(a.factor), float(a.factor * a.factor))
    res = dict(tool="rsp_mine_bench", slide=a.slide, factor=a.factor, level2=[H, W], tile=S, stride=a.stride, batch=B,
               device=torch.cuda.get_device_name(0), threads=a.threads)

    # ---- the kernels, one launch each
    lin = torch.from_numpy(mining.srgb_linear_table()).to(dev)
    total = K.lab_a_sum(overview, lin)
    npx = float(overview.shape[0] * overview.shape[1])
    bits = K.tissue_bits(lr2, "hsv_s", 0.1)
    plane_bytes = 3 * H * W + 4 * bits.shape[1] * H
    res["bits_hsv_s"] = with_rate(timed(lambda: K.tissue_bits(lr2, "hsv_s", 0.1, out=bits), a.iters), plane_bytes)
    res["bits_lab_a"] = with_rate(timed(lambda: K.tissue_bits(lr2, "lab_a", lin=lin, thr_sum=total, factor=1.15, count=npx, out=bits),
                                        a.iters), plane_bytes)
    res["lab_a_sum"] = with_rate(timed(lambda: K.lab_a_sum(overview, lin, out=total), a.iters), 3 * npx)
    K.tissue_bits(lr2, "hsv_s", 0.1, out=bits)
    count, keep = K.tile_popcount(bits, W, (S, S), (a.stride, a.stride), 0.75)
    ncand = count.numel()
    res["popcount"] = with_rate(timed(lambda: K.tile_popcount(bits, W, (S, S), (a.stride, a.stride), 0.75), a.iters),
                                ncand * S * 4 * ((S + 31) // 32 + 1) + 5 * ncand)
    res["popcount"]["candidates"] = int(ncand)
    res["popcount"]["plane_bytes_over_image_bytes"] = 4 * bits.shape[1] * H / (3 * H * W)

    # ---- the whole mining pass, both criteria, against the NumPy restatement
    lr2_host, ov_host = lr2.cpu().numpy(), overview.cpu().numpy()
    mined = {}
    for variant in ("v2", "v1"):
        mining.mine_tiles(levels, ds, S, a.stride, variant=variant, overview=overview)          # warm-up
        torch.cuda.synchronize()
        t0 = time.time()
        mined[variant] = mining.mine_tiles(levels, ds, S, a.stride, variant=variant, overview=overview)
        dt_dev = time.time() - t0
        t0 = time.time()
        want = numpy_keep(lr2_host, ov_host, S, a.stride, variant, a.threads)
        dt_np = time.time() - t0
        got = mined[variant]["keep"]
        res["mine_" + variant] = dict(criterion=mining.CRITERIA[variant][0], mine_device_ms=dt_dev * 1e3, mine_numpy_ms=dt_np * 1e3,
                                      speedup=dt_np / dt_dev, candidates=int(got.size), kept=int(got.sum()),
                                      keep_equal=bool(np.array_equal(got, want)), keep_differs=int((got != want).sum()))

    # ---- one batch of the gather, and the byte-compare yardstick at its output size
    m = mined["v2"]
    T = len(m["xpos"])
    if T == 0:
        raise SystemExit("rsp_mine_bench: the synthetic slide kept no candidate")
    xy = tuple(torch.from_numpy(t).to(dev) for t in m["xy"])
    order = torch.randperm(6 * T, generator=torch.Generator().manual_seed(a.seed)).to(dev)
    idxs = [order[(k * B) % max(1, 6 * T - B):][:B].contiguous() for k in range(4)]
    n = int(idxs[0].numel())
    out = tuple(torch.empty((n, 3, S, S), dtype=torch.uint8, device=dev) for _ in range(3)) + (torch.empty(n, dtype=torch.int64, device=dev),)
    it = iter(range(1 << 30))
    res["gather"] = with_rate(timed(lambda: K.rsp_gather(levels, xy, idxs[next(it) % 4], S, out=out), a.iters), 2 * 3 * n * 3 * S * S)
    res["gather"].update(samples=n, triplets=T, tiles=3 * n)
    res["byte_compare"] = with_rate(timed(lambda: torch.eq(out[0], out[1]), a.iters), 3 * n * 3 * S * S)
    for key in ("bits_hsv_s", "bits_lab_a", "gather"):
        res[key]["rate_over_byte_compare"] = res[key]["tbps"] / res["byte_compare"]["tbps"]
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--slide", type=int, default=16384)
    p.add_argument("--factor", type=int, default=2)
    p.add_argument("--tile", type=int, default=256)
    p.add_argument("--stride", type=int, default=128)
    p.add_argument("--batch", type=int, default=384)
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--threads", type=int, default=16)
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
