#!/usr/bin/env python
"""Stream time of the device-side v1 RandAugment ops (sslcr_randaug_v1_slot) on one batch of uint8 images, one process, one box.

    python tools/augment_v1_bench.py [--images 640] [--size 256] [--n 2] [--iters 20] [--host-images 16] [--threads 16] [--out profiles/augv1_bench.json]

The batch is the unlabeled batch of the consistency step: 640 images of 256 x 256 (what the hed note of csrc/augment.hip uses).
Per figure the median of ``--iters`` calls with min and max, HIP events around each call, after 3 warm-up calls:

  ops.<name>.us       ONE sslcr_randaug_v1_slot call in which every image takes the op, tables already on the device (kernel time of
                      the slot's launches: the COPY instance that finds nothing to do, the op's instance, for resize both passes)
  ops.<name>.x_eq     that time over ``eq_us``
  eq_us               the project's usual yardstick in the same process: a torch.eq that moves the same bytes as a slot (3 H W read
                      + 3 H W written per image; the eq reads two tensors and writes one of a third of that each)
  randaugment.*       RandAugmentDevice(n, 10, cv_ops="device") whole on the NCHW batch: ``device_ms`` events around ``run`` with the
                      draws already made (it contains the gaps in which the host builds and uploads the slot tables), ``plan_ms`` the
                      host clock around the draws, ``call_ms`` the host clock around the whole call ending in a synchronise
  host.<name>.ms_per_image   the NumPy restatement (tests/_cv_ref.py) of the op on the host, the stand-in for a ``host_ops`` callable
                      (OpenCV is not importable here): ``--host-images`` images on ``--threads`` threads, wall time per image;
                      ``batch_ms_extrapolated`` scales it to the batch and is named for what it is

Prints one JSON line; --out also writes it to a file.  No ratio is a pass mark: the figures say what the ops cost next to a copy.
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
sys.path.insert(0, os.path.join(ROOT, "tests"))


def stats(ts):
    ts = sorted(ts)
    return {"median": round(ts[len(ts) // 2], 3), "min": round(ts[0], 3), "max": round(ts[-1], 3)}


def timed(fn, iters, warmup=3):
    """HIP-event time of each of ``iters`` calls of fn, in microseconds"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) * 1e3 for a, b in ev]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=640)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--n", type=int, default=2)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--host-images", type=int, default=16)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("augment_v1_bench: no GPU; a timing from anything else says nothing about the device path")
    from ssl_cr_histo_amd import _lib as L
    from ssl_cr_histo_amd import augment as A
    import _cv_ref as R

    N, S = args.images, args.size
    dev = torch.device("cuda")
    host = np.random.RandomState(0).randint(0, 256, (N, S, S, 3)).astype(np.uint8)
    src = torch.from_numpy(host).to(dev).permute(0, 3, 1, 2).contiguous()
    dst = torch.empty_like(src)
    fwd = A.rotation_matrix((S, S), 33.0, 0.8, 0.05, -0.02)
    inv = A.invert_affine(fwd)
    s1 = int(S * 1.1)
    seed = 0x0123456789ABCDEF
    cases = {"copy": (A.V1_COPY, [0, 0, 0, 0], [0.0] * 6), "blur3": (A.V1_BLUR, [3, 0, 0, 0], [0.0] * 6),
             "blur5": (A.V1_BLUR, [5, 0, 0, 0], [0.0] * 6), "blur7": (A.V1_BLUR, [7, 0, 0, 0], [0.0] * 6),
             "hsv": (A.V1_HSV, [1, -1, 1, 0], [0.0] * 6), "warp": (A.V1_WARP, [1, 0, 0, 0], inv),
             "resize": (A.V1_RESIZE, [s1, 10, 10, 0], [0.0] * 6),
             "noise": (A.V1_NOISE, [seed & 0xFFFFFFFF, seed >> 32, 0, 0], [10.0] + [0.0] * 5)}
    work, wsmax = A.v1_workspace(N, S, s1, dev)
    wtab = A._warp_table_on(dev)
    # the yardstick: an eq whose traffic equals a slot's (2 * 3 H W per image)
    third = 2 * N * S * S
    ea, eb = torch.zeros(third, dtype=torch.uint8, device=dev), torch.zeros(third, dtype=torch.uint8, device=dev)
    eo = torch.empty(third, dtype=torch.bool, device=dev)
    eq_us = stats(timed(lambda: torch.eq(ea, eb, out=eo), args.iters))
    ops, keep = {}, []
    for name, (code, ip, dp) in cases.items():
        t_op = torch.full((N,), code, dtype=torch.int32, device=dev)
        t_ip = torch.from_numpy(np.tile(np.array(ip, np.int64).astype(np.uint32).view(np.int32)[None], (N, 1))).to(dev)
        t_dp = torch.tensor([dp] * N, dtype=torch.float64, device=dev)
        d = L.AugV1Desc(L.ptr(src), L.ptr(dst), L.ptr(t_op), None, L.ptr(t_ip), L.ptr(t_dp), L.ptr(wtab), L.ptr(work), wsmax, 1 << code,
                        N, S, S, 0, 0)
        keep.append((t_op, t_ip, t_dp))
        st = stats(timed(lambda d=d: L.check(L.lib().sslcr_randaug_v1_slot(d, L.stream_ptr())), args.iters))
        changed = bool((dst != src).flatten(1).any(1).all())
        if changed == (name == "copy"):
            raise SystemExit(f"augment_v1_bench: the timed {name} call did not do its work")
        ops[name] = {"us": st, "x_eq": round(st["median"] / eq_us["median"], 2), "gbps": round(2 * 3 * N * S * S / st["median"] * 1e-3, 1)}

    aug = A.RandAugmentDevice(args.n, 10, random.Random(1), np.random.RandomState(1), cv_ops="device")
    plans = [aug.plan(N) for _ in range(args.iters + 3)]
    it = iter(plans)
    dev_us = stats(timed(lambda: aug.run(src, next(it)), args.iters))
    t0 = time.perf_counter()
    for _ in range(args.iters):
        aug.plan(N)
    plan_ms = (time.perf_counter() - t0) * 1e3 / args.iters
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.iters):
        aug(src)
    torch.cuda.synchronize()
    call_ms = (time.perf_counter() - t0) * 1e3 / args.iters

    tab = R.warp_table()
    host_fns = {"blur7": lambda im: R.blur(im, 7), "hsv": lambda im: R.shift_hsv(im, 1, -1, 1), "warp": lambda im: R.warp_affine(im, inv, 1, 0, tab),
                "resize": lambda im: R.scale_resize_crop(im, s1, 10, 10), "noise": lambda im: R.gaussian_noise(im, 10.0, seed)[0]}
    hostres = {}
    with ThreadPoolExecutor(args.threads) as pool:
        for name, fn in host_fns.items():
            ts = []
            for rep in range(3):
                t0 = time.perf_counter()
                list(pool.map(fn, host[:args.host_images]))
                if rep:
                    ts.append((time.perf_counter() - t0) * 1e3)
            per = min(ts) / args.host_images
            hostres[name] = {"ms_per_image": round(per, 3), "batch_ms_extrapolated": round(per * N, 1)}
    res = {"tool": "augment_v1_bench", "images": N, "size": S, "iters": args.iters, "device": torch.cuda.get_device_name(0),
           "eq_us": eq_us, "slot_bytes": 2 * 3 * N * S * S, "ops": ops,
           "randaugment": {"n": args.n, "m": 10, "device_ms": {k: round(v / 1e3, 3) for k, v in dev_us.items()}, "plan_ms": round(plan_ms, 3),
                           "call_ms": round(call_ms, 3), "images_per_s": round(N / call_ms * 1e3, 1)},
           "host_leg": f"NumPy restatement (tests/_cv_ref.py), {args.host_images} images on {args.threads} threads", "host": hostres}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
