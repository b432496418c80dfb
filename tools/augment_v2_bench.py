#!/usr/bin/env python
"""Images/s of the device-side RSP v2 RandAugment against the host chain it replaces, on one batch of uint8 tiles.

    python tools/augment_v2_bench.py [--tiles 384] [--size 256] [--n 2] [--m 3] [--iters 20] [--threads 16] [--full-pool] [--colour-op hed|hsv] [--out FILE]

Device leg: ``RandAugmentV2Device(n, m)`` on an [N, H, W, 3] batch that sits in HBM.  Three figures, each named for what it is:
  device_ms   HIP events around the launches of one batch with the draws already made (stream time, first launch to last kernel;
              it contains the gaps in which the host builds and uploads the per-slot tables)
  plan_ms     host clock around the draws of one batch (``plan``), no device work
  call_ms     host clock around the whole call, draws included, ending in a device synchronise
Host leg: the same plans executed tile by tile with the Pillow calls of Pretraining_v2/models/randaugment.py:44-172 on a pool of
``--threads`` threads (Pillow releases the GIL inside its C loops).  Without Pillow the NumPy restatement of tests/_pil_ref.py is
timed instead, and ``host_leg`` in the output says which of the two it was.

The plans are drawn like the reference draws them, except that a tile whose sample holds ``hed`` or ``hsv`` is drawn again: those
two ops need scikit-image on either side and are not what this default run measures.  Prints one JSON line; --out also writes it to a file.

--full-pool samples the whole pool instead, ``colour_ops="device"``: no tile is drawn again, ``hed`` / ``hsv`` run through
``sslcr_randaug_v2_colour``, and the host leg runs the NumPy restatement of the two (tests/_colour_ref.py -- what a ``host_ops`` user
without scikit-image would pass).  The JSON then also carries, from the same process: ``no_colour_device_ms_median`` (the default
run's figure), and per colour op alone -- all tiles take it -- ``<op>_kernel_us`` (HIP events around back-to-back calls of the C entry
with the tables already on the device, each call on a fresh copy of the batch: kernel time, hed with its byte-sum pass), ``<op>_tbps`` (bytes the launches move over that
time: 2 x 3 H W per tile, + 3 H W for hed's sum pass) and ``host_<op>_ms`` (the restatement on ``--threads`` threads).
"""
import argparse
import json
import os
import random
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RSP_STEP_MS_PER_384 = 9.6       # README status, round 6: the RSP pretraining step this augmentation feeds


def draw_plan(aug, count):
    rows = []
    while len(rows) < count:
        (row,) = aug.plan(1)
        if not any(name in aug.HOST for name, _, _ in row):
            rows.append(row)
    return rows


def pillow_chain():
    from PIL import Image, ImageEnhance, ImageOps
    enh = {"contrast": ImageEnhance.Contrast, "brightness": ImageEnhance.Brightness, "sharpness": ImageEnhance.Sharpness, "color": ImageEnhance.Color}

    def op(img, name, val, sign):
        if name == "identity":
            return img
        im = Image.fromarray(img)
        if name in enh:
            return np.asarray(enh[name](im).enhance(val / 10 * 1.8 + 0.1))
        if name == "autocontrast":
            return np.asarray(ImageOps.autocontrast(im))
        if name == "equalize":
            return np.asarray(ImageOps.equalize(im))
        lv = val / 10 * {"rotate": 30., "translate_x": 10., "translate_y": 10., "shear_x": 0.3, "shear_y": 0.3}[name]
        lv = lv if sign == 1 else -lv
        if name == "rotate":
            return np.asarray(im.rotate(angle=lv))
        if name == "translate_x":
            return np.asarray(im.transform(im.size, Image.AFFINE, (1, 0, lv, 0, 1, 0)))
        if name == "translate_y":
            return np.asarray(im.transform(im.size, Image.AFFINE, (1, 0, 0, 0, 1, lv)))
        a = (1, lv, 0, 0, 1, 0) if name == "shear_x" else (1, 0, 0, lv, 1, 0)
        return np.asarray(im.transform(im.size, Image.AFFINE, a, Image.BICUBIC))
    return op


def device_ms(aug, batch, plans, warmup):
    """median / min / max stream time and host wall time of aug.run over plans[warmup:]"""
    for p in plans[:warmup]:
        aug.run(batch, p)
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in plans[warmup:]]
    t0 = time.perf_counter()
    for (a, b), p in zip(ev, plans[warmup:]):
        a.record()
        aug.run(batch, p)
        b.record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3 / len(ev)
    return sorted(a.elapsed_time(b) for a, b in ev), wall


def colour_kernel_us(A, batch, name, reps=20):
    """stream time of ONE sslcr_randaug_v2_colour call in which every tile takes ``name``, tables already on the device.  Every timed
    call works on a fresh copy of the batch of its own (``reps`` copies, restored outside the timed region): the call is in place,
    and hed applied over and over to one buffer drives the image mean out of the cutoff range, after which the calls skip the
    arithmetic.  Checked from the result: every tile of every copy must have changed."""
    from ssl_cr_histo_amd import _lib as L
    n, h, w = batch.shape[0], batch.shape[1], batch.shape[2]
    draws = (0.11, -0.07, 0.05, 0.04, -0.06, 0.02) if name == "hed" else (0.21, 0.17, 0.0)
    works = [torch.empty_like(batch) for _ in range(reps)]
    t_op = torch.full((n,), A._V2_COLOUR[name], dtype=torch.int32, device=batch.device)
    t_p = torch.tensor([A.colour_param_row(name, draws)] * n, dtype=torch.float64, device=batch.device)
    bsum = torch.empty((n,), dtype=torch.int64, device=batch.device)
    inv, fwd = A.v2_hed_matrices()
    descs = [L.AugV2ColourDesc(L.ptr(wk), L.ptr(t_op), L.ptr(t_p), L.ptr(bsum), A.HED_CUTOFF[0], A.HED_CUTOFF[1],
                               (L.f32 * 9)(*inv.reshape(-1).tolist()), (L.f32 * 9)(*fwd.reshape(-1).tolist()), 1 << A._V2_COLOUR[name], n, h, w, 1)
             for wk in works]
    times = []
    for rep in range(4):
        for wk in works:
            wk.copy_(batch)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for d in descs:
            L.check(L.lib().sslcr_randaug_v2_colour(d, L.stream_ptr()))
        b.record()
        torch.cuda.synchronize()
        for wk in works:
            if not bool((wk != batch).flatten(1).any(1).all()):
                raise SystemExit(f"augment_v2_bench: a timed {name} call left a tile unchanged (cutoff hit?): the figure would not be the op's")
        if rep:
            times.append(a.elapsed_time(b) * 1e3 / reps)
    return sorted(times)[len(times) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=384)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--n", type=int, default=2)
    ap.add_argument("--m", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--full-pool", action="store_true", help='sample hed / hsv too and run them on the device (colour_ops="device")')
    ap.add_argument("--colour-op", choices=("hed", "hsv"), default=None, help="time only this op's kernels (the per-op leg of --full-pool) and exit")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("augment_v2_bench: no GPU; a timing from anything else says nothing about the device path")
    from ssl_cr_histo_amd import augment as A

    rs = np.random.RandomState(0)
    host_batch = rs.randint(0, 256, (args.tiles, args.size, args.size, 3)).astype(np.uint8)
    batch = torch.from_numpy(host_batch).cuda()
    if args.colour_op:
        print(json.dumps({"tool": "augment_v2_bench", "tiles": args.tiles, "size": args.size,
                          f"{args.colour_op}_kernel_us": round(colour_kernel_us(A, batch, args.colour_op), 2)}))
        return
    # the (empty) host ops only let plan() draw a row that names hed / hsv; draw_plan keeps no such row
    aug = A.RandAugmentV2Device(args.n, args.m, random.Random(1), np.random.RandomState(1), host_ops=dict.fromkeys(A.RandAugmentV2Device.HOST))
    draw = draw_plan
    plans = [draw(aug, args.tiles) for _ in range(args.warmup + args.iters)]
    extra = {}
    if args.full_pool:
        extra["no_colour_device_ms_median"] = round(device_ms(aug, batch, plans, args.warmup)[0][args.iters // 2], 4)
        aug = A.RandAugmentV2Device(args.n, args.m, random.Random(1), np.random.RandomState(1), colour_ops="device")
        draw = lambda aug, count: aug.plan(count)      # noqa: E731  the whole pool: nothing is drawn again
        plans = [draw(aug, args.tiles) for _ in range(args.warmup + args.iters)]
        names = [name for p in plans for row in p for name, _, _ in row]
        extra["colour_tile_fraction"] = round(sum(any(nm in aug.HOST for nm, _, _ in row) for p in plans for row in p) / (len(plans) * args.tiles), 4)
        extra["hed_slots"], extra["hsv_slots"] = names.count("hed"), names.count("hsv")

    device_ms_sorted, run_wall_ms = device_ms(aug, batch, plans, args.warmup)

    t0 = time.perf_counter()
    for _ in range(args.iters):
        draw(aug, args.tiles)
    plan_ms = (time.perf_counter() - t0) * 1e3 / args.iters
    t0 = time.perf_counter()
    for _ in range(args.iters):
        aug.run(batch, draw(aug, args.tiles))
    torch.cuda.synchronize()
    call_ms = (time.perf_counter() - t0) * 1e3 / args.iters

    try:
        op = pillow_chain()
        import PIL
        host_leg = f"Pillow {PIL.__version__}"
    except ImportError:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import _pil_ref as R
        op, host_leg = R.apply_op, "NumPy restatement (tests/_pil_ref.py); Pillow is not importable here"

    if args.full_pool:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import _colour_ref as CR
        pil_op = op

        def op(img, name, val, third):
            if name == "hed":
                return CR.hed_f32(img, third)
            if name == "hsv":
                return CR.hsv(img, *third)
            return pil_op(img, name, val, third)
        host_leg += "; hed / hsv: NumPy restatement (tests/_colour_ref.py)"
        moved = {"hed": 9, "hsv": 6}                 # bytes per pixel: read + write, and hed's sum pass reads once more
        with ThreadPoolExecutor(args.threads) as pool:
            for name, fn in (("hed", lambda im: CR.hed_f32(im, (0.11, -0.07, 0.05, 0.04, -0.06, 0.02))), ("hsv", lambda im: CR.hsv(im, 0.21, 0.17))):
                us = colour_kernel_us(A, batch, name)
                extra[f"{name}_kernel_us"] = round(us, 2)
                extra[f"{name}_tbps"] = round(moved[name] * args.tiles * args.size * args.size / us * 1e-6, 3)
                ts = []
                for rep in range(3):
                    t0 = time.perf_counter()
                    list(pool.map(fn, host_batch))
                    if rep:
                        ts.append((time.perf_counter() - t0) * 1e3)
                extra[f"host_{name}_ms"] = round(min(ts), 2)

    def one(args_):
        img, row = args_
        for name, val, sign in row:
            img = op(img, name, val, sign)
        return img
    host_ms = []
    with ThreadPoolExecutor(args.threads) as pool:
        for rep in range(args.host_reps + 1):
            t0 = time.perf_counter()
            list(pool.map(one, zip(host_batch, plans[rep % len(plans)])))
            if rep:                                   # the first pass warms the pool
                host_ms.append((time.perf_counter() - t0) * 1e3)
    host_med = sorted(host_ms)[len(host_ms) // 2]
    dev_med = device_ms_sorted[len(device_ms_sorted) // 2]
    res = {"tool": "augment_v2_bench", "tiles": args.tiles, "size": args.size, "n": args.n, "m": args.m, "iters": args.iters,
           "device": torch.cuda.get_device_name(0),
           "device_ms_median": round(dev_med, 4), "device_ms_min": round(device_ms_sorted[0], 4), "device_ms_max": round(device_ms_sorted[-1], 4),
           "run_wall_ms": round(run_wall_ms, 4), "plan_ms": round(plan_ms, 4), "call_ms": round(call_ms, 4),
           "device_images_per_s": round(args.tiles / dev_med * 1e3, 1), "call_images_per_s": round(args.tiles / call_ms * 1e3, 1),
           "host_leg": host_leg, "host_threads": args.threads, "host_ms_median": round(host_med, 3),
           "host_images_per_s": round(args.tiles / host_med * 1e3, 1),
           "rsp_step_ms_per_384": RSP_STEP_MS_PER_384,
           "device_over_rsp_step": round(dev_med / (RSP_STEP_MS_PER_384 * args.tiles / 384), 4),
           "call_over_rsp_step": round(call_ms / (RSP_STEP_MS_PER_384 * args.tiles / 384), 4)}
    if args.full_pool:
        res["pool"] = 'full, colour_ops="device"'
        res.update(extra)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
