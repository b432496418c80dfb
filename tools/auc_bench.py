#!/usr/bin/env python
"""Stream time of the ranking kernels (csrc/rank.hip) and of what they are measured against, in one process.

    python tools/auc_bench.py [--iters 20] [--sigma 1.0] [--out profiles/auc_bench.json]

Workloads:
  map            the 1536 x 3072 probability map of tools/froc_bench.py against its truth mask, every cell a tissue cell: 1.0f on 95 % of
                 the cells inside the polygons, so one run of ties covers most of the positives
  map_smoothed   kernels.gaussian_smooth of that map (sigma): the plateaus' rims dissolve into distinct values
  kather         a [7180, 9] float32 softmax with random targets, the size of the Kather test set: nine rows sorted in one call
Figures per workload, each with median / min / max of HIP events around ONE call over ``launches`` calls after two warm-up calls:
  rank_keys      kernels.rank_keys (one launch)
  sort_pairs     kernels.sort_pairs alone on the keys and values rank_keys wrote (its copies of the inputs included: 12 launches)
  auc_counts     kernels.auc_counts whole: keys, the sort, the three count launches; no copy to the host
  auc            inference.map_auc (the maps) / inference.roc_auc(multi_class='ovr') (kather) whole, its host copy and division included
  torch_sort     the yardstick: ``torch.sort(stable=True)`` of the same keys as int32 rows in the same order (it returns int64 indices)
  byte_compare   the yardstick for streaming kernels: ``torch.eq`` of two uint8 tensors of 4 bytes per key (12 bytes per key moved)
  sklearn_ms     ``sklearn.metrics.roc_auc_score`` of the same scores on this host, once; ``difference`` = |device - sklearn| and
                 ``bound`` = n 2^-53
Prints one JSON line; --out also writes it."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def bench(a):
    import torch
    from sklearn.metrics import roc_auc_score
    from annotation_bench import MASK, RESOLUTION, make_annotation, timed
    from ssl_cr_histo_amd import inference as I
    from ssl_cr_histo_amd import kernels as K
    from ssl_cr_histo_amd.annotation import Annotation
    if not torch.cuda.is_available():
        raise SystemExit("auc_bench: no GPU visible; nothing here is measured without one")
    dev = torch.device("cuda", 0)
    truth = Annotation().from_vertices(make_annotation(a.seed)).to_device(dev).mask(MASK, RESOLUTION)
    th = truth.cpu().numpy() != 0
    rs = np.random.RandomState(a.seed + 2)                          # tools/froc_bench.py's map, draw for draw
    pm = (rs.rand(*MASK) * 0.45).astype(np.float32)
    peaks = rs.rand(*MASK) < 0.001
    pm[peaks] = (0.5 + 0.499 * rs.rand(int(peaks.sum()))).astype(np.float32)
    pm[th & (rs.rand(*MASK) < 0.95)] = 1.0
    pmd = torch.from_numpy(pm).to(dev)
    tissue = torch.ones(MASK, dtype=torch.uint8, device=dev)
    smooth = K.gaussian_smooth(pmd, a.sigma)
    logits = rs.randn(7180, 9) * 2
    e = np.exp(logits - logits.max(1, keepdims=True))
    soft = (e / e.sum(1, keepdims=True)).astype(np.float32)
    kt = rs.randint(0, 9, 7180)
    res = dict(tool="auc_bench", device=torch.cuda.get_device_name(0), mask=list(MASK), inside_share=float(th.mean()), sigma=a.sigma,
               sort_tile=K.SORT_TILE, scan_trip=K.RANK_SCAN_TRIP)

    def workload(scores, target, valid, auc, host_scores, host_target, multi):
        row = {}
        flat = scores.reshape(scores.shape[0], -1) if multi else scores.reshape(-1)
        keys, values, _ = K.rank_keys(flat, target, positive=None if multi else [1], valid=valid)
        Cn, n = keys.shape
        row["rows"], row["keys_per_row"] = Cn, n
        u, v = (torch.randint(0, 256, (4 * Cn * n,), dtype=torch.uint8, device=dev) for _ in range(2))
        cmp = timed(lambda: torch.eq(u, v), a.iters)
        cmp["bytes"] = 12 * Cn * n
        row["byte_compare"] = cmp
        row["rank_keys"] = timed(lambda: K.rank_keys(flat, target, positive=None if multi else [1], valid=valid), a.iters)
        ws = K.sort_workspace(Cn, n, dev)
        row["sort_pairs"] = timed(lambda: K.sort_pairs(keys, values, workspace=ws), a.iters)
        signed = (keys.view(torch.int32) ^ torch.tensor(-(1 << 31), dtype=torch.int32, device=dev)).contiguous()    # int32 order = uint32 order
        row["torch_sort"] = timed(lambda: torch.sort(signed, dim=1, stable=True), a.iters)
        got_k, got_v = K.sort_pairs(keys, values=None, workspace=ws)
        want_k, want_i = torch.sort(signed, dim=1, stable=True)
        row["sort_equals_torch"] = bool(torch.equal(got_v.view(torch.int32).long(), want_i)
                                        and torch.equal(got_k.view(torch.int32), want_k ^ torch.tensor(-(1 << 31), dtype=torch.int32, device=dev)))
        row["auc_counts"] = timed(lambda: K.auc_counts(flat, target, positive=None if multi else [1], valid=valid), a.iters)
        row["auc"] = timed(auc, a.iters)
        row["value"] = auc()
        t0 = time.time()
        want = roc_auc_score(host_target, host_scores, multi_class="ovr") if multi else roc_auc_score(host_target, host_scores)
        row["sklearn_ms"] = (time.time() - t0) * 1e3
        row["difference"], row["bound"] = abs(row["value"] - want), len(host_target) * 2.0 ** -53
        for key in ("rank_keys", "sort_pairs", "auc_counts", "auc", "torch_sort"):
            row[key]["over_byte_compare"] = row[key]["median_ms"] / cmp["median_ms"]
        row["sort_pairs"]["over_torch_sort"] = row["sort_pairs"]["median_ms"] / row["torch_sort"]["median_ms"]
        return row

    tflat = (truth.reshape(-1) != 0).to(torch.int64)
    res["map"] = workload(pmd, tflat, None, lambda: I.map_auc(pmd, truth, tissue), pm.reshape(-1), th.reshape(-1), False)
    sm = smooth.cpu().numpy()
    res["map_smoothed"] = workload(smooth, tflat, None, lambda: I.map_auc(smooth, truth, tissue), sm.reshape(-1), th.reshape(-1), False)
    sd, td = torch.from_numpy(soft).to(dev), torch.from_numpy(kt).to(dev)
    res["kather"] = workload(sd, td, None, lambda: I.roc_auc(sd, td, multi_class="ovr"), soft.astype(np.float64), kt, True)
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
    p.add_argument("--sigma", type=float, default=1.0)
    p.add_argument("--seed", type=int, default=7)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    print(dump(bench(a), a.out))


if __name__ == "__main__":
    main()
