#!/usr/bin/env python
"""Tiles/s of WSI inference (``steps.camelyon16_test``) with the slide in HBM against the host-fed path it replaces, in one process.

    python tools/wsi_bench.py [--slide 16384] [--resolution 64] [--tile 256] [--batch 1024] [--dtype bf16] [--host-batches K] [--out FILE]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o wsi -- python tools/wsi_bench.py --kernel-leg
    python tools/wsi_bench.py --stats DIR/.../wsi_kernel_stats.csv [--merge FILE]          (no device: reads the profiler's table)

Inputs: a seeded synthetic slide of ``--slide`` x ``--slide`` pixels, a seeded tissue mask at ``--resolution`` with about 45 % tissue
(indexed [x, y] as the reference's), ``--tile``-pixel tiles in batches of ``--batch``.  Figures, each named for what it is:
  host_path     the parent's path: per batch the tiles are cut on the host into float32 NCHW (what DatasetCamelyon16_test hands its
                loader, 786 KB per 256-pixel tile) and go through the unchanged branch of ``camelyon16_test`` (pageable upload, one
                ``.cpu()`` per batch, host scatter).  Host clock around the call; ``--host-batches K`` stops it after K batches (the
                rate is per tile either way) because the full slide is tens of GB of host traffic.
  device_path   ``WsiDeviceLoader``: host clock around ``camelyon16_test`` (ends in the one copy of the map), every batch; the
                one-time upload of the slide's bytes is reported beside it (``upload_ms``) and counted in ``tiles_per_s_with_upload``.
  stream_ms     HIP events around gather + forward + predict of each full batch, queued back to back (median / min / max)
  forward_ms    HIP events around the forward alone on the same, already gathered, batches
The two maps are compared over the tiles both paths served (``map_max_abs_diff``).  ``--kernel-leg`` runs only gathers of one batch
and, as the yardstick the README quotes for byte kernels, an element-wise byte compare of two such batches (``torch.eq``: reads
2 x 3 S^2 bytes per tile as the gather moves, and writes 3 S^2 of bools), for a profiler run of its own; ``--stats`` turns that run's table into TB/s.
Prints one JSON line; --out also writes it to a file."""
import argparse
import csv
import json
import os
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_inputs(a):
    rs = np.random.RandomState(a.seed)
    slide = rs.randint(0, 256, size=(a.slide, a.slide, 3), dtype=np.uint8)
    side = a.slide // a.resolution
    mask = rs.rand(side, side) < 0.45
    mask[0, 0] = mask[-1, -1] = True
    return slide, mask


def build_model(dev):
    import torch
    from ssl_cr_histo_amd import net
    torch.manual_seed(0)
    model, cls = net.TripletNet_Finetune("resnet18"), net.FinetuneResNet(2)
    return model.to(dev), cls.to(dev)


class HostLoader:
    """the reference loader's batches, cut from the slide array on the host: float32 NCHW tiles, zero outside the slide"""

    def __init__(self, slide, mask, x_idcs, y_idcs, xy, S, B, max_batches):
        self.dataset = types.SimpleNamespace(mask=mask)
        self.slide, self.x, self.y, self.xy, self.S, self.B = slide, x_idcs, y_idcs, xy, S, B
        nb = (len(x_idcs) + B - 1) // B
        self.nb = min(nb, max_batches) if max_batches else nb
        self.tiles = min(len(x_idcs), self.nb * B)

    def __len__(self):
        return self.nb

    def __iter__(self):
        import torch
        S, (RH, RW, _) = self.S, self.slide.shape
        for b in range(self.nb):
            lo, hi = b * self.B, min((b + 1) * self.B, len(self.x))
            out = np.zeros((hi - lo, 3, S, S), dtype=np.float32)
            for k in range(lo, hi):
                left, top = int(self.xy[k, 0]), int(self.xy[k, 1])
                y0, y1, x0, x1 = max(top, 0), min(top + S, RH), max(left, 0), min(left + S, RW)
                if y0 < y1 and x0 < x1:
                    out[k - lo, :, y0 - top:y1 - top, x0 - left:x1 - left] = self.slide[y0:y1, x0:x1].transpose(2, 0, 1)
            yield torch.from_numpy(out), torch.from_numpy(self.x[lo:hi].copy()), torch.from_numpy(self.y[lo:hi].copy())


def events_ms(pairs):
    v = sorted(a.elapsed_time(b) for a, b in pairs)
    return dict(median=v[len(v) // 2], min=v[0], max=v[-1], batches=len(v))


def bench(a):
    import torch
    from ssl_cr_histo_amd import engine as E
    from ssl_cr_histo_amd import kernels as K
    from ssl_cr_histo_amd import steps
    from ssl_cr_histo_amd.inference import WsiDeviceLoader, tile_origins
    if not torch.cuda.is_available():
        raise SystemExit("wsi_bench: no GPU visible; nothing here is measured without one")
    dev = torch.device("cuda", 0)
    eng = E.Engine(dev, a.dtype)
    E.set_engine(eng)
    slide, mask = make_inputs(a)
    model, cls = build_model(dev)
    args = types.SimpleNamespace(print_freq=0)
    S, B = a.tile, a.batch
    x_idcs, y_idcs, xy = tile_origins(mask, a.resolution, S)
    res = dict(tool="wsi_bench", slide=a.slide, resolution=a.resolution, tile=S, batch=B, dtype=a.dtype, tiles=int(len(x_idcs)),
               tissue=float(mask.mean()), device=torch.cuda.get_device_name(0))

    t0 = time.time()
    loader = WsiDeviceLoader(slide, mask, S, B, resolution=a.resolution)
    torch.cuda.synchronize()
    res["upload_ms"] = (time.time() - t0) * 1e3

    # warm-up: every shape of the timed windows (a full batch and the ragged last one), both input dtypes
    net = eng.bind(model, cls)
    model.eval(); cls.eval()
    for lo, hi in (loader.ranges()[0], loader.ranges()[-1]):
        t = loader.tiles(lo, hi)
        net.forward((t,), train=False)
        net.forward((t.float(),), train=False)
    torch.cuda.synchronize()

    # (b) the device path, whole slide
    t0 = time.time()
    map_b = steps.camelyon16_test(args, model, cls, loader)
    dt_b = time.time() - t0
    res["device_path"] = dict(seconds=dt_b, tiles=int(len(x_idcs)), tiles_per_s=len(x_idcs) / dt_b,
                              tiles_per_s_with_upload=len(x_idcs) / (dt_b + res["upload_ms"] / 1e3))

    # (a) the parent's path: host-cut float32 tiles through the unchanged branch
    host = HostLoader(slide, mask, x_idcs, y_idcs, xy, S, B, a.host_batches)
    t0 = time.time()
    map_a = steps.camelyon16_test(args, model, cls, host)
    dt_a = time.time() - t0
    res["host_path"] = dict(seconds=dt_a, tiles=host.tiles, batches=len(host), tiles_per_s=host.tiles / dt_a)
    served = np.zeros(mask.shape, bool)
    served[x_idcs[:host.tiles], y_idcs[:host.tiles]] = True
    res["map_max_abs_diff"] = float(np.abs(map_a[served] - map_b[served]).max())
    res["speedup_tiles_per_s"] = res["device_path"]["tiles_per_s"] / res["host_path"]["tiles_per_s"]
    res["device_not_slower"] = bool(res["device_path"]["tiles_per_s"] >= res["host_path"]["tiles_per_s"])

    # stream time per full batch (gather + forward + predict) and the forward alone on the same batches
    full = [r for r in loader.ranges() if r[1] - r[0] == B][:a.event_batches]
    probs = torch.zeros(mask.shape, dtype=torch.float32, device=dev)
    pairs = []
    for lo, hi in full:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _, out = net.forward((loader.tiles(lo, hi),), train=False)
        K.predict(out, pred=False, col=-1, map=probs, map_index=loader.map_index[lo:hi])
        e1.record()
        pairs.append((e0, e1))
    torch.cuda.synchronize()
    res["stream_ms"] = events_ms(pairs)
    tiles = [loader.tiles(lo, hi) for lo, hi in full[:4]]
    pairs = []
    for k in range(len(full)):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        net.forward((tiles[k % len(tiles)],), train=False)
        e1.record()
        pairs.append((e0, e1))
    torch.cuda.synchronize()
    res["forward_ms"] = events_ms(pairs)
    res["stream_tiles_per_s"] = B / (res["stream_ms"]["median"] / 1e3)
    res["forward_tiles_per_s"] = B / (res["forward_ms"]["median"] / 1e3)
    return res


def kernel_leg(a):
    """gathers of one batch and the byte-compare yardstick, for a profiler run of its own"""
    import torch
    from ssl_cr_histo_amd.inference import WsiDeviceLoader
    if not torch.cuda.is_available():
        raise SystemExit("wsi_bench: no GPU visible; nothing here is measured without one")
    slide, mask = make_inputs(a)
    loader = WsiDeviceLoader(slide, mask, a.tile, a.batch, resolution=a.resolution)
    ranges = [r for r in loader.ranges() if r[1] - r[0] == a.batch]
    out = [torch.empty((a.batch, 3, a.tile, a.tile), dtype=torch.uint8, device=loader.region.device) for _ in range(2)]
    for it in range(a.kernel_iters):
        lo, hi = ranges[it % len(ranges)]
        loader.tiles(lo, hi, out=out[it & 1])
    for _ in range(a.kernel_iters):
        torch.eq(out[0], out[1])
    torch.cuda.synchronize()
    return dict(tool="wsi_bench", leg="kernel", tile=a.tile, batch=a.batch, iters=a.kernel_iters)


def stats(a):
    """the profiler's kernel table -> time and TB/s of the gather and of the byte compare"""
    per_tile = 3 * a.tile * a.tile
    res = dict(tool="wsi_bench", leg="kernel_stats", tile=a.tile, batch=a.batch, gather_bytes=2 * per_tile * a.batch,
               compare_bytes=3 * per_tile * a.batch)
    with open(a.stats) as f:
        for row in csv.DictReader(f):
            name = row["Name"]
            key = "gather" if "wsi_gather_kernel" in name else "compare" if "CompareEq" in name else None
            if key and key + "_us" not in res:
                us = float(row["AverageNs"]) / 1e3
                res[key + "_us"], res[key + "_min_us"], res[key + "_calls"] = us, float(row["MinNs"]) / 1e3, int(row["Calls"])
                res[key + "_tbps"] = res[key + "_bytes"] / (us * 1e-6) / 1e12
                res[key + "_kernel"] = name[:120]
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--slide", type=int, default=16384)
    p.add_argument("--resolution", type=int, default=64)
    p.add_argument("--tile", type=int, default=256)
    p.add_argument("--batch", type=int, default=1024)
    p.add_argument("--dtype", default="bf16")
    p.add_argument("--seed", type=int, default=7)
    p.add_argument("--host-batches", type=int, default=0, help="stop the host path after this many batches (0: the whole slide)")
    p.add_argument("--event-batches", type=int, default=16)
    p.add_argument("--kernel-leg", action="store_true")
    p.add_argument("--kernel-iters", type=int, default=20)
    p.add_argument("--stats", default=None, help="a rocprofv3 kernel-stats csv of a --kernel-leg run")
    p.add_argument("--merge", default=None, help="with --stats: a JSON file of an earlier run to add the kernel figures to")
    p.add_argument("--out", default=None)
    a = p.parse_args()
    if a.stats:
        res = stats(a)
        if a.merge:
            with open(a.merge) as f:
                base = json.load(f)
            base["kernel"] = res
            res = base
    elif a.kernel_leg:
        res = kernel_leg(a)
    else:
        res = bench(a)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
