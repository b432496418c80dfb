"""Times of the device t-SNE (inference.Tsne, csrc/tsne.hip) at Kather's size and at 20 000 points, against the same iteration written
with torch.cdist over dense n x n matrices in the same process, and sklearn's Barnes-Hut on the host.  One process, one GPU, HIP
events, the median of --calls calls with min and max; the whole fit by the host clock.

    python tools/tsne_bench.py [--out profiles/tsne_bench.json] [--calls 20] [--no-sklearn]

Per iteration the C-ABI has two entries: sslcr_tsne_repulsion (the O(n^2) launch and the one-workgroup fold of Z, timed together) and
sslcr_tsne_update.  The rate figure counts the n (n - 1) ordered pairs of the repulsive sum, 13 fp32 VALU instructions = 16 flop each
(2 subtractions, a product, an fma, an addition, v_rcp_f32, a product, an addition, two fmas), against the 157.3 TF fp32 vector peak."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_F32_VECTOR = 157.3e12
FLOP_PER_PAIR = 16
SHAPES = [dict(name="kather", n=7180, D=512), dict(name="twenty_thousand", n=20000, D=512)]


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


def features(n, D, dev):
    g = torch.Generator(device=dev).manual_seed(1)
    centres = 3.0 * torch.randn(9, D, device=dev, generator=g)
    return (centres[torch.arange(n, device=dev) % 9] + torch.randn(n, D, device=dev, generator=g)).contiguous()


def torch_iteration(y, update, gains, rows, col, val, exaggeration, momentum, lr):
    """the same iteration in torch over dense n x n matrices (float32)"""
    q = 1.0 / (1.0 + torch.cdist(y, y).square_())
    q.fill_diagonal_(0.0)
    Z = q.sum(dtype=torch.float64)
    w = q * q
    rep = (w.sum(1, keepdim=True) * y - w @ y).double() / Z
    pq = (val * q[rows, col])[:, None] * (y[rows] - y[col])
    attr = torch.zeros_like(y, dtype=torch.float64).index_add_(0, rows, pq.double())
    grad = (4.0 * (exaggeration * attr - rep)).float()
    inc = update * grad < 0
    gains.copy_(torch.where(inc, gains + 0.2, gains * 0.8).clamp_(min=0.01))
    update.mul_(momentum).sub_(lr * gains * grad)
    y.add_(update)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tsne_bench.json"))
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--no-sklearn", action="store_true")
    a = ap.parse_args()
    from ssl_cr_histo_amd import _lib as L
    from ssl_cr_histo_amd import inference as I
    from ssl_cr_histo_amd import kernels as K
    dev = torch.device("cuda", 0)
    out_rows = []
    for sh in SHAPES:
        n, D = sh["n"], sh["D"]
        x = features(n, D, dev)
        row = dict(sh, plan=K.tsne_plan(n), k=I.Tsne.neighbours(n, 30.0))
        k = row["k"]
        xc = I.Tsne.center(x).contiguous()
        idx, d2 = K.euclidean_topk(xc, k)
        cond, _ = K.tsne_affinities(d2, 30.0)
        setup = dict(euclidean_topk=timed(lambda: K.euclidean_topk(xc, k), a.calls), affinities=timed(lambda: K.tsne_affinities(d2, 30.0), a.calls),
                     joint=timed(lambda: K.tsne_joint(idx, cond), a.calls), pca_init=timed(lambda: I.Tsne.pca_init(xc), max(3, a.calls // 4)))
        row["setup"] = setup
        t = I.Tsne(max_iter=1000).prepare(x)
        for _ in range(300):                         # past the exaggerated stage: the embedding has spread
            t.step()
        y, y2 = t.state["y"], torch.empty_like(t.state["y"])
        rowptr, col, val = t.P
        w = t._w
        grad, u2, g2 = torch.empty_like(y), t._update.clone(), t._gains.clone()
        d = L.TsneGradDesc(L.ptr(y), L.ptr(y2), L.ptr(u2), L.ptr(g2), L.ptr(grad), L.ptr(rowptr), L.ptr(col), L.ptr(val),
                           L.ptr(w["ws"]), L.ptr(w["Z"]), None, n, w["slices"], col.numel(), 1.0, 0.8, t.lr, 0.01)
        rep = timed(lambda: L.check(L.lib().sslcr_tsne_repulsion(d, L.stream_ptr())), a.calls)
        pairs = float(n) * (n - 1)
        rep.update(pairs_per_s=pairs / rep["median_ms"] * 1e3, tflops=pairs * FLOP_PER_PAIR / rep["median_ms"] / 1e9,
                   share_of_fp32_vector_peak=pairs * FLOP_PER_PAIR / rep["median_ms"] * 1e3 / PEAK_F32_VECTOR)
        upd = timed(lambda: L.check(L.lib().sslcr_tsne_update(d, L.stream_ptr())), a.calls)
        step = timed(t.step, a.calls)
        kl_rows = torch.empty(n, dtype=torch.float64, device=dev)
        log_row = torch.zeros(4, dtype=torch.float64, device=dev)
        klt = timed(lambda: K.tsne_kl(kl_rows, grad, w["Z"], log_row, 0), a.calls)
        row["per_iteration"] = dict(repulsion_and_z_fold=rep, update=upd, kl_log_row=klt, step_as_queued_from_python=step)
        # the dense torch yardstick, from the same state
        nnz = int(rowptr[-1].item())
        rows_ = torch.repeat_interleave(torch.arange(n, device=dev), (rowptr[1:] - rowptr[:-1]).long())
        ty, tu, tg = y.clone(), t._update.clone(), t._gains.clone()
        tor = timed(lambda: torch_iteration(ty, tu, tg, rows_, col[:nnz].long(), val[:nnz], 1.0, 0.8, t.lr), a.calls)
        row["torch_dense_iteration"] = tor
        row["torch_ms_over_device_ms"] = tor["median_ms"] / step["median_ms"]
        del ty, tu, tg
        # the whole fit by the host clock
        torch.cuda.synchronize()
        t0 = time.time()
        f = I.Tsne(max_iter=1000).fit(x)
        torch.cuda.synchronize()
        row["fit_1000_iterations_s"] = time.time() - t0
        row["fit_kl"] = f.kl_divergence_
        row["fit_host_reads"] = f.reads
        if not a.no_sklearn:
            from sklearn.manifold import TSNE
            xh = x.cpu().numpy()
            t0 = time.time()
            sk = TSNE(method="barnes_hut", init="pca", n_jobs=16, random_state=0)
            sk.fit_transform(xh)
            row["sklearn_barnes_hut_16_threads_s"] = time.time() - t0
            row["sklearn_kl"] = float(sk.kl_divergence_)
            row["sklearn_s_over_device_s"] = row["sklearn_barnes_hut_16_threads_s"] / row["fit_1000_iterations_s"]
        print(json.dumps(row), flush=True)
        out_rows.append(row)
    out = dict(device=torch.cuda.get_device_name(0), peak_fp32_vector_tflops=PEAK_F32_VECTOR / 1e12, flop_per_pair=FLOP_PER_PAIR, shapes=out_rows)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
