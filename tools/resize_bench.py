#!/usr/bin/env python
"""Stream time of the resize kernels (csrc/resample.hip) and of what they are measured against, in one process on one box.

    python tools/resize_bench.py [--iters 20] [--patches 1024] [--set 2048] [--out profiles/resize_bench.json]

Kernel leg.  ``patches`` patches of 512 x 512 x 3 (HWC, what the datasets hold) -> 256 x 256 CHW (what the engine takes), bilinear and
lanczos, in both forms (``form='fused'`` and ``form='two_pass'``).  Per filter and form: median / min / max of HIP events around ONE
``kernels.pil_resize`` call over ``iters`` calls after two warm-up calls; ``bytes`` = the bytes the form has to move (source read once +
destination written once; the two-pass form also writes and reads its intermediate); ``over_byte_compare`` = its median over the
median of the project's yardstick for streaming kernels, a ``torch.eq`` of two uint8 tensors sized so that it moves the SAME number of
bytes (2 read + 1 written per element), in the same process; ``equal_to_pillow`` on the first 8 patches.
``pillow_16_threads_ms``: the same batch through ``PIL.Image.resize`` on a pool of 16 threads of this host (Pillow releases the GIL),
host clock, the better of two runs.

Loop leg.  ``steps.bpq_test`` (bf16 engine) over a synthetic set of ``set`` patches of 512 x 512, batches of 64, by the host clock around
the call (it ends in the copy of its results): fed by ``inference.PatchDeviceLoader`` (patches resident; the upload is made before the
clock starts, as a resident loader's is made once per run) and fed by a host loader that resizes every patch with Pillow on one thread
(the reference's ``__getitem__``), each the better of two runs.
Prints one JSON line; --out also writes it."""
import argparse
import json
import os
import sys
import time
import types
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

SRC, DST = 512, 256


def bench(a):
    import torch
    from PIL import Image
    from annotation_bench import timed
    from ssl_cr_histo_amd import engine as E
    from ssl_cr_histo_amd import kernels as K
    from ssl_cr_histo_amd import net, steps
    from ssl_cr_histo_amd.inference import PatchDeviceLoader
    if not torch.cuda.is_available():
        raise SystemExit("resize_bench: no GPU visible; nothing here is measured without one")
    dev = torch.device("cuda", 0)
    rs = np.random.RandomState(a.seed)
    host = rs.randint(0, 256, size=(a.patches, SRC, SRC, 3), dtype=np.uint8)
    x = torch.from_numpy(host).to(dev)
    out = torch.empty((a.patches, 3, DST, DST), dtype=torch.uint8, device=dev)
    res = dict(tool="resize_bench", device=torch.cuda.get_device_name(0), patches=a.patches, src=[SRC, SRC, 3], dst=[3, DST, DST],
               pillow=__import__("PIL").__version__, plan={})
    src_b, dst_b = x.numel(), out.numel()
    for name in ("bilinear", "lanczos"):
        plan = K.resample_plan((SRC, SRC), (DST, DST), name, n=a.patches, out_layout="chw")
        res["plan"][name] = plan
        row = {}
        for form in ("fused", "two_pass"):
            moved = src_b + dst_b + (0 if form == "fused" else 2 * a.patches * 3 * SRC * DST)
            n_eq = moved // 3
            u, v = (torch.randint(0, 256, (n_eq,), dtype=torch.uint8, device=dev) for _ in range(2))
            cmp = timed(lambda: torch.eq(u, v), a.iters)
            del u, v
            t = timed(lambda: K.pil_resize(x, (DST, DST), name, out=out, out_layout="chw", form=form), a.iters)
            t["bytes"] = moved
            t["TB_per_s"] = moved / t["median_ms"] / 1e9
            t["byte_compare"] = cmp
            t["over_byte_compare"] = t["median_ms"] / cmp["median_ms"]
            want = np.stack([np.asarray(Image.fromarray(p).resize((DST, DST), getattr(Image, name.upper()))) for p in host[:8]])
            t["equal_to_pillow"] = bool(np.array_equal(out[:8].cpu().numpy().transpose(0, 2, 3, 1), want))
            row[form] = t
        row["fused_over_two_pass"] = row["fused"]["median_ms"] / row["two_pass"]["median_ms"]

        def pil_all():
            f = getattr(Image, name.upper())
            with ThreadPoolExecutor(16) as pool:
                list(pool.map(lambda p: np.asarray(Image.fromarray(p).resize((DST, DST), f)), host))
        best = 1e30
        for _ in range(2):
            t0 = time.time()
            pil_all()
            best = min(best, (time.time() - t0) * 1e3)
        row["pillow_16_threads_ms"] = best
        row["pillow_16_threads_over_fused"] = best / row["fused"]["median_ms"]
        res[name] = row
    del x, out
    # ---- the loop: bpq_test over a synthetic set
    E.set_engine(E.Engine(dev, "bf16"))
    model, cls = net.TripletNet_Finetune("resnet18").to(dev), net.FinetuneResNet(1).to(dev)
    n, B = a.set, 64
    patches = host[np.arange(n) % a.patches]                                # the set, in host memory (1.6 GB at 2048)
    ta = torch.from_numpy(rs.rand(n).astype(np.float32))
    args = types.SimpleNamespace(print_freq=0)

    class HostLoader:                                                       # the reference's loader: Pillow per patch, one thread
        def __len__(self):
            return (n + B - 1) // B

        def __iter__(self):
            for lo in range(0, n, B):
                tiles = np.stack([np.asarray(Image.fromarray(p).resize((DST, DST), Image.BILINEAR)) for p in patches[lo:lo + B]])
                yield torch.from_numpy(tiles).permute(0, 3, 1, 2).contiguous(), ta[lo:lo + B], ta[lo:lo + B]

    def clock(loader):
        best, outv = 1e30, None
        for _ in range(2):
            torch.cuda.synchronize()
            t0 = time.time()
            outv = steps.bpq_test(args, model, cls, loader)
            best = min(best, time.time() - t0)
        return best, outv

    dl = PatchDeviceLoader(patches, ta, ta, image_size=DST, batch_size=B, device=dev)
    dl.tiles(0, 1)                                                          # the one upload, outside the clock
    torch.cuda.synchronize()
    t_dev, o_dev = clock(dl)
    t_host, o_host = clock(HostLoader())
    res["bpq_test"] = dict(patches=n, batch=B, mode="bf16", device_loader_s=t_dev, host_pillow_loader_s=t_host,
                           device_loader_patches_per_s=n / t_dev, host_pillow_loader_patches_per_s=n / t_host,
                           speedup=t_host / t_dev, outputs_equal=bool(torch.equal(o_dev[0], o_host[0]) and torch.equal(o_dev[1], o_host[1])))
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--patches", type=int, default=1024)
    p.add_argument("--set", type=int, default=2048)
    p.add_argument("--seed", type=int, default=11)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    line = json.dumps(bench(a))
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
