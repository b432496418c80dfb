"""Times of the fused linear-probe evaluation (kernels.linprobe_eval) against the stream rate of the same bytes and against torch's
four-launch route, and of the whole fit against sklearn's LogisticRegression on the host.  One process, one GPU, HIP events, the
median of --calls calls with min and max.

    python tools/linprobe_bench.py [--out profiles/linprobe_bench.json] [--calls 20] [--no-sklearn]

The evaluation's bound is the one read of X, 4 n D bytes: the yardstick is a ``torch.eq`` of two float32 tensors that moves the same
4 n D bytes in the same process (it reads n D / 2 elements of each and writes a byte per pair: within 1/8 of a pure read).  torch's
route: logits = addmm, log_softmax, the residual, residual^T @ X -- it reads X twice and writes the logits and the residual out.  The
ratios are reported as they come out, whichever side wins."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [dict(name="kather_100k", n=100000, D=768, C=9), dict(name="wide_many_classes", n=100000, D=2048, C=64)]
FIT = dict(n=100000, D=768, C=9, C_reg=1.0, tol=1e-4)


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


def torch_route(x, y1h, w, b):
    z = torch.addmm(b, x, w.t())
    lp = torch.log_softmax(z, 1)
    r = (lp.exp() - y1h) / x.shape[0]
    return -(lp * y1h).sum() / x.shape[0], r.t() @ x, r.sum(0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "linprobe_bench.json"))
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--no-sklearn", action="store_true")
    a = ap.parse_args()
    from ssl_cr_histo_amd import inference as I
    from ssl_cr_histo_amd import kernels as K
    dev = torch.device("cuda", 0)
    rows = []
    for sh in SHAPES:
        n, D, C = sh["n"], sh["D"], sh["C"]
        g = torch.Generator(device=dev).manual_seed(1)
        x = torch.randn(n, D, device=dev, generator=g)
        w = torch.randn(C, D, device=dev, generator=g) * 0.05
        b = torch.zeros(C, device=dev)
        y = torch.randint(0, C, (n,), device=dev, generator=g)
        y1h = torch.nn.functional.one_hot(y, C).float()
        nbytes = 4.0 * n * D
        row = dict(sh, bytes=nbytes, plan=K.linprobe_plan(n, D, C))
        buf = torch.empty(1 + C * (D + 1), dtype=torch.float64, device=dev)
        # the three launches alone: descriptor and workspace built once, the C entry called directly (the Python wrapper's tensor
        # checks and allocations cost the host more than the evaluation costs the device: timed separately below)
        from ssl_cr_histo_amd import _lib as L
        ws = torch.empty(row["plan"]["workspace_bytes"] // 16 + 1, dtype=torch.complex128, device=dev)
        desc = L.LinprobeDesc(L.ptr(x), L.ptr(w), L.ptr(b), L.ptr(y), None, None, L.ptr_at(buf, 0), L.ptr_at(buf, 8), None, L.ptr(ws),
                              n, D, C, 0, 0)
        lib, st = L.lib(), L.stream_ptr()
        fused = timed(lambda: L.check(lib.sslcr_linprobe_eval(desc, st)), a.calls)
        row["wrapper_call"] = timed(lambda: K.linprobe_eval(x, y, w, b, out=buf), a.calls)
        fused["tb_per_s"] = nbytes / fused["median_ms"] / 1e9
        row["fused_eval"] = fused
        half = x.view(-1)[: n * D // 2], x.view(-1)[n * D // 2:]
        out8 = torch.empty(n * D // 2, dtype=torch.bool, device=dev)
        eq = timed(lambda: torch.eq(half[0], half[1], out=out8), a.calls)
        eq["tb_per_s"] = nbytes / eq["median_ms"] / 1e9
        row["torch_eq_same_bytes"] = eq
        tor = timed(lambda: torch_route(x, y1h, w, b), a.calls)
        row["torch_four_launch_route"] = tor
        row["fused_ms_over_stream_ms"] = fused["median_ms"] / eq["median_ms"]          # 1 = the stream rate of one read of X
        row["fused_ms_over_torch_ms"] = fused["median_ms"] / tor["median_ms"]          # above 1: torch's route is the faster one
        v, gr = K.linprobe_eval(x, y, w, b)
        tv, tg, tb = torch_route(x, y1h, w, b)
        row["value_rel_diff_to_torch"] = float(abs(v.item() - tv.item()) / abs(tv.item()))
        row["grad_max_rel_diff_to_torch"] = float((gr[:, :D].float() - tg).abs().max() / tg.abs().max())
        print(json.dumps(row), flush=True)
        rows.append(row)
        del x, y1h, out8
    # the whole fit by the host clock, Gaussian clusters
    n, D, C = FIT["n"], FIT["D"], FIT["C"]
    rng = np.random.default_rng(0)
    centres = rng.standard_normal((C, D)).astype(np.float32)
    yh = rng.integers(0, C, n)
    xh = centres[yh] + 4.0 * rng.standard_normal((n, D)).astype(np.float32)
    xd, yd = torch.from_numpy(xh).to(dev), torch.from_numpy(yh).to(dev)
    I.LinearProbe(C=FIT["C_reg"], n_classes=C, tol=FIT["tol"], max_iter=2).fit(xd, yd)    # warm-up
    torch.cuda.synchronize()
    t0 = time.time()
    probe = I.LinearProbe(C=FIT["C_reg"], n_classes=C, tol=FIT["tol"]).fit(xd, yd)
    torch.cuda.synchronize()
    fit = dict(FIT, device_fit_s=time.time() - t0, status=probe.status_, n_iter=probe.n_iter_, n_eval=probe.n_eval_, reads=probe.reads,
               grad_max=probe.grad_max_, train_accuracy=probe.score(xd, yd))
    if not a.no_sklearn:
        import sklearn
        from sklearn.linear_model import LogisticRegression
        from threadpoolctl import threadpool_limits
        with threadpool_limits(limits=16):
            t0 = time.time()
            m = LogisticRegression(C=FIT["C_reg"], tol=FIT["tol"], max_iter=1000).fit(xh, yh)
            fit.update(sklearn_version=sklearn.__version__, sklearn_16_threads_s=time.time() - t0, sklearn_n_iter=int(m.n_iter_[0]),
                       sklearn_train_accuracy=float(m.score(xh, yh)))
        fit["sklearn_s_over_device_s"] = fit["sklearn_16_threads_s"] / fit["device_fit_s"]
    print(json.dumps(fit), flush=True)
    out = dict(device=torch.cuda.get_device_name(0), shapes=rows, fit=fit)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
