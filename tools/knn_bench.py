"""Times of the fused k-NN top-k (kernels.knn_topk) on the shapes the probe meets, against torch.mm + torch.topk in the same process
and sklearn's brute force on the host.  One process, one GPU, HIP events, the median of --calls calls with min and max.

    python tools/knn_bench.py [--out profiles/knn_bench.json] [--calls 20] [--no-sklearn]

FLOPs are the 2 nq nb D of the similarity; the share of peak is against the 157.3 TF of the fp32 MFMA pipe.  torch's route writes and
re-reads the whole nq x nb product; it has no total order on ties and no exclude_self, so for the leave-one-out shape it is timed
with k + 1 neighbours (the caller would drop the self match on the host)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_F32_MFMA = 157.3e12
SHAPES = [dict(name="kather", nq=7180, nb=100000, D=768, k=20, loo=False),
          dict(name="leave_one_out", nq=20000, nb=20000, D=768, k=20, loo=True),
          dict(name="few_queries", nq=64, nb=100000, D=768, k=20, loo=False)]


def timed(fn, calls, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return dict(median_ms=float(np.median(ms)), min_ms=float(min(ms)), max_ms=float(max(ms)), calls=calls)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_bench.json"))
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--no-sklearn", action="store_true")
    a = ap.parse_args()
    from ssl_cr_histo_amd import kernels as K
    dev = torch.device("cuda", 0)
    rows = []
    for sh in SHAPES:
        g = torch.Generator(device=dev).manual_seed(1)
        bank = K.l2_normalize(torch.randn(sh["nb"], sh["D"], device=dev, generator=g))
        q = bank if sh["loo"] else K.l2_normalize(torch.randn(sh["nq"], sh["D"], device=dev, generator=g))
        nq, nb, D, k = sh["nq"], sh["nb"], sh["D"], sh["k"]
        flop = 2.0 * nq * nb * D
        ex = 0 if sh["loo"] else None
        row = dict(sh, flop=flop, plan=K.knn_plan(nq, nb, D, k))
        fused = timed(lambda: K.knn_topk(q, bank, k, exclude_self=ex), a.calls)
        fused.update(tflops=flop / fused["median_ms"] / 1e9, share_of_fp32_mfma_peak=flop / fused["median_ms"] / 1e9 / (PEAK_F32_MFMA / 1e12))
        row["fused"] = fused
        if row["plan"]["slices"] > 1:                              # what the slices buy: the same call on one slice
            one = timed(lambda: K.knn_topk(q, bank, k, exclude_self=ex, slices=1), max(3, a.calls // 4), warmup=1)
            row["fused_one_slice"] = one
        kk = k + 1 if sh["loo"] else k
        tor = timed(lambda: torch.topk(torch.mm(q, bank.t()), kk, dim=1), a.calls)
        tor.update(tflops=flop / tor["median_ms"] / 1e9)
        row["torch_mm_topk"] = tor
        row["fused_ms_over_torch_ms"] = fused["median_ms"] / tor["median_ms"]      # above 1: torch's route is the faster one
        # agreement of the two routes (torch's product is another summation order: near ties may swap)
        fs, fi = K.knn_topk(q, bank, k, exclude_self=ex)
        prod = torch.mm(q, bank.t())
        if sh["loo"]:
            prod.fill_diagonal_(float("-inf"))
        ti = torch.topk(prod, k, dim=1)[1]
        del prod
        row["index_agreement_with_torch"] = float((fi.long() == ti).float().mean())
        s1 = K.knn_topk(q, bank, k, exclude_self=ex, slices=1)
        row["equal_bits_one_slice"] = bool(torch.equal(s1[0].view(torch.int32), fs.view(torch.int32)) and torch.equal(s1[1], fi))
        if not a.no_sklearn:
            from sklearn.neighbors import NearestNeighbors
            bh, qh = bank.cpu().numpy(), q.cpu().numpy()
            t0 = time.time()
            nn = NearestNeighbors(n_neighbors=kk, algorithm="brute", metric="cosine", n_jobs=16).fit(bh)
            nn.kneighbors(qh)
            row["sklearn_brute_16_threads_s"] = time.time() - t0
            row["sklearn_ms_over_fused_ms"] = row["sklearn_brute_16_threads_s"] * 1e3 / fused["median_ms"]
        print(json.dumps(row), flush=True)
        rows.append(row)
        del bank, q
    out = dict(device=torch.cuda.get_device_name(0), peak_fp32_mfma_tflops=PEAK_F32_MFMA / 1e12, shapes=rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
