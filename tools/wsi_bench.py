#!/usr/bin/env python
"""Tiles/s of WSI inference (``steps.camelyon16_test``) with the slide in HBM against the host-fed path it replaces, in one process.

    python tools/wsi_bench.py [--slide 16384] [--resolution 64] [--tile 256] [--batch 1024] [--dtype bf16] [--host-batches K] [--out FILE]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o wsi -- python tools/wsi_bench.py --kernel-leg
    python tools/wsi_bench.py --stats DIR/.../wsi_kernel_stats.csv [--merge FILE]          (no device: reads the profiler's table)
    python tools/wsi_bench.py --tta d4 [...]                     the same run, then the slide again with args.tta = d4 (``tta`` in the result)
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o wsi -- python tools/wsi_bench.py --kernel-leg --tta d4
    python tools/wsi_bench.py --tta d4 --trace DIR/.../wsi_kernel_trace.csv [--table-out FILE.csv] [--merge FILE]   (no device)

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
``--tta SPEC`` (test-time augmentation over D4): ``tta.stream_ms`` is HIP events around the G oriented gathers + G forwards + the one
predict_tta of each full batch; the yardstick is G x the plain ``stream_ms`` of the same process (``ratio_to_G_plain``,
``excess_us_per_batch``).  With ``--kernel-leg`` the oriented gather of every listed code runs beside the identity gather, and
``--trace`` turns that run's per-dispatch trace into one row per code.
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
    if a.tta:
        res["tta"] = bench_tta(a, eng, net, model, cls, loader, full, res["stream_ms"]["median"], map_b)
    return res


def tta_spec(text):
    """--tta: a set name ('d4', 'rot90', 'flips') or comma-separated codes ('3,5')"""
    from ssl_cr_histo_amd.inference import d4_codes
    return d4_codes(text if not text[0].isdigit() else [int(v) for v in text.split(",")])


def bench_tta(a, eng, net, model, cls, loader, full, plain_stream_ms, plain_map):
    """the same slide with args.tta, beside the plain figures of this process: host clock around ``camelyon16_test`` and HIP events
    around the G oriented gathers + G forwards + one predict_tta of each full batch.  The yardstick is G times the plain path's
    stream time per batch; what exceeds it is the cost of orienting the gathers and of the reduce."""
    import torch
    from ssl_cr_histo_amd import kernels as K
    from ssl_cr_histo_amd import steps
    codes = tta_spec(a.tta)
    G, B = len(codes), a.batch
    args = types.SimpleNamespace(print_freq=0, tta=codes)
    lo, hi = full[0]
    for g in codes:                                                   # warm-up: the oriented gather of every code
        loader.tiles(lo, hi, orient=g)
    torch.cuda.synchronize()
    t0 = time.time()
    map_t = steps.camelyon16_test(args, model, cls, loader)
    dt = time.time() - t0
    n = len(loader.dataset)
    out = dict(spec=a.tta, codes=list(codes), G=G, device_path=dict(seconds=dt, tiles=n, tiles_per_s=n / dt, forwards_per_s=n * G / dt),
               map_max_abs_diff_to_plain=float(np.abs(map_t - plain_map).max()))
    probs = torch.zeros(loader.dataset.mask.shape, dtype=torch.float32, device=loader.region.device)
    pairs = []
    for lo, hi in full:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ens = torch.empty((G, hi - lo, net.ncls), dtype=torch.float32, device=probs.device)
        for k, g in enumerate(codes):
            ens[k].copy_(net.forward((loader.tiles(lo, hi, orient=g),), train=False)[1])
        K.predict_tta(ens, pred=False, col=-1, map=probs, map_index=loader.map_index[lo:hi])
        e1.record()
        pairs.append((e0, e1))
    torch.cuda.synchronize()
    out["stream_ms"] = events_ms(pairs)
    med = out["stream_ms"]["median"]
    out["plain_stream_ms_median"] = plain_stream_ms
    out["yardstick_ms"] = G * plain_stream_ms
    out["ratio_to_G_plain"] = med / (G * plain_stream_ms)
    out["excess_us_per_batch"] = (med - G * plain_stream_ms) * 1e3
    out["stream_tiles_per_s"] = B / (med / 1e3)
    return out


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
    codes = tta_spec(a.tta) if a.tta else ()
    # with --tta: the oriented gather, the codes in turn (so that a drift of the clock spreads over all of them), every dispatch on
    # the NEXT batch of the slide as the identity loop above: each reads source bytes that the dispatches before it did not leave in
    # the caches.  (In camelyon16_test only the first listed code of a batch reads a cold source; the other G - 1 re-read it warm.)
    # --tta-warm: all codes of a round on ONE batch, after an identity gather of it (not counted: its own kernel) warmed the source.
    for it in range(a.kernel_iters * len(codes)):
        lo, hi = ranges[(it // len(codes) if a.tta_warm else it) % len(ranges)]
        if a.tta_warm and it % len(codes) == 0:
            loader.tiles(lo, hi, out=out[0])
        loader.tiles(lo, hi, out=out[1 if a.tta_warm else it & 1], orient=codes[it % len(codes)])
    for _ in range(a.kernel_iters):
        torch.eq(out[0], out[1])
    torch.cuda.synchronize()
    return dict(tool="wsi_bench", leg="kernel", tile=a.tile, batch=a.batch, iters=a.kernel_iters, codes=list(codes))


def trace_table(a):
    """a rocprofv3 kernel TRACE (one row per dispatch) of a ``--kernel-leg --tta SPEC`` run -> one row per orientation code of the
    oriented gather beside the identity gather (sslcr_wsi_gather) and the byte compare of the same trace: calls, mean / min / max us
    and requested TB/s.  The k-th oriented dispatch carries code codes[k % G] (``kernel_leg`` issues them in turn)."""
    codes = tta_spec(a.tta)
    per_tile = 3 * a.tile * a.tile
    with open(a.trace) as f:
        rows = list(csv.DictReader(f))
    col = {k.lower(): k for k in rows[0]}
    name, t0, t1 = col["kernel_name"], col["start_timestamp"], col["end_timestamp"]
    rows.sort(key=lambda r: int(r[t0]))
    groups = {}
    k = 0
    for r in rows:
        us = (int(r[t1]) - int(r[t0])) / 1e3
        if "d4_bytes_kernel" in r[name]:
            groups.setdefault(f"gather_d4 code {codes[k % len(codes)]}", []).append(us)
            k += 1
        elif "wsi_gather_kernel" in r[name]:
            groups.setdefault("gather (identity, sslcr_wsi_gather)", []).append(us)
        elif "CompareEq" in r[name]:
            groups.setdefault("byte compare (torch.eq)", []).append(us)
    table = []
    for key, v in groups.items():
        nbytes = (3 if key.startswith("byte") else 2) * per_tile * a.batch
        table.append(dict(kernel=key, calls=len(v), mean_us=sum(v) / len(v), min_us=min(v), max_us=max(v),
                          requested_tbps=nbytes / (sum(v) / len(v) * 1e-6) / 1e12))
    if a.table_out:
        with open(a.table_out, "w", newline="") as f:
            w = csv.DictWriter(f, fieldnames=list(table[0]))
            w.writeheader()
            for row in table:
                w.writerow({k: (f"{v:.3f}" if isinstance(v, float) else v) for k, v in row.items()})
    return dict(tool="wsi_bench", leg="kernel_trace", tile=a.tile, batch=a.batch, codes=list(codes), table=table)


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
    p.add_argument("--tta", default=None, help="a D4 set ('d4', 'rot90', 'flips') or codes '3,5': also measure args.tta = SPEC")
    p.add_argument("--tta-warm", action="store_true", help="with --kernel-leg --tta: every code of a round on one, already read, batch")
    p.add_argument("--trace", default=None, help="a rocprofv3 kernel-trace csv of a --kernel-leg --tta run: the per-code table")
    p.add_argument("--table-out", default=None, help="with --trace: write the table as csv")
    p.add_argument("--out", default=None)
    a = p.parse_args()
    if a.trace:
        res = trace_table(a)
        if a.merge:
            with open(a.merge) as f:
                base = json.load(f)
            base["kernel"] = res
            res = base
    elif a.stats:
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
