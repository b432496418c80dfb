#!/usr/bin/env python
"""What gradient accumulation costs on the headline shape (bench.py's SSL_CR step: 192 + 448 student, 448 teacher images of 256x256,
bf16, Adam, full fine-tune), measured with HIP events on one MI355X.  Device-only: inputs are seeded and resident in HBM, nothing
outside the repository is read.

    python tools/grad_accum_bench.py [--reps 12] [--steps 10] [--dtype bf16] [--out FILE]

  1. sslcr_grad_accumulate alone on two buffers of the engine's gradient count (stream time per call, bytes moved / time);
  2. the stream time of an ACCUMULATING micro-step (micro-batch 1 of k = 2: 96 + 224 student, 224 teacher images) against the SAME
     micro-step without accumulation, alternating, `--reps` of each; the difference against (bytes the design moves) / 4.7 TB/s,
     grad_sumsq_kernel's measured rate on this buffer (profiles/optim_groups_ab.txt).  The design: the backward writes into a
     second flat buffer (cleared instead of the first: no extra bytes), then grads[i] = grads[i] + new[i] over the trainable range
     reads 2 and writes 1 float per element = 12 bytes per gradient element;
  3. images/s of whole optimizer steps at k = 1, 2, 4 over the same global batch (k micro-steps + one Adam step).
Prints the report; --out also writes it to a file."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SUMSQ_TBS = 4.7          # grad_sumsq_kernel on the engine's gradient buffer, profiles/optim_groups_ab.txt


def synth_u8(shape, seed, device):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randint(0, 256, shape, dtype=torch.uint8, generator=g).to(device)


def build_nets(device):
    from ssl_cr_histo_amd import net
    torch.manual_seed(42)
    return net.TripletNet_Finetune("resnet18").to(device), net.FinetuneResNet(1).to(device)


def timed(fn, stream):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from ssl_cr_histo_amd import engine as E
    from ssl_cr_histo_amd import kernels as K
    from ssl_cr_histo_amd import steps
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    eng = E.set_engine(E.Engine(dev, args.dtype))
    stream = torch.cuda.current_stream(dev)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    nx, nu, hw = 192, 448, 256
    mt, ct = build_nets(dev)
    ms, cs = build_nets(dev)
    mt.eval(); ct.eval(); ms.train(); cs.train()
    for p in list(mt.parameters()) + list(ct.parameters()):
        p.requires_grad = False
    te, st = eng.bind(mt, ct), eng.bind(ms, cs)
    opt = torch.optim.Adam(list(ms.parameters()) + list(cs.parameters()), lr=1e-4, betas=(0.9, 0.999), weight_decay=1e-4)
    x, u_w, u_s = synth_u8((nx, 3, hw, hw), 1234, dev), synth_u8((nu, 3, hw, hw), 2234, dev), synth_u8((nu, 3, hw, hw), 3234, dev)
    y = torch.rand(nx, generator=torch.Generator().manual_seed(4234)).to(dev)
    count = sum((p.numel() + 63) // 64 * 64 for p in st.params)            # the flat gradient buffer: every parameter padded to 64
    say(f"gradient accumulation on the headline shape ({nx}+{nu} student, {nu} teacher, {hw}x{hw}, {args.dtype}, Adam), {torch.cuda.get_device_name(dev)}")
    say(f"flat gradient buffer: {count} floats = {count * 4 / 1e6:.1f} MB; the sum moves 12 bytes per element = {count * 12 / 1e6:.1f} MB "
        f"-> {count * 12 / SUMSQ_TBS / 1e6:.1f} us at {SUMSQ_TBS} TB/s")

    # ---- 1. the kernel alone
    a, b = torch.randn(count, device=dev), torch.randn(count, device=dev) * 1e-3
    for _ in range(5):
        K.grad_accumulate(a, b)
    calls = 50
    ms_k = sorted(timed(lambda: [K.grad_accumulate(a, b) for _ in range(calls)], stream) / calls for _ in range(5))
    us = ms_k[2] * 1e3
    say(f"1. sslcr_grad_accumulate alone, {calls} calls back to back, 5 rounds: median {us:.2f} us per call (min {ms_k[0] * 1e3:.2f}, max "
        f"{ms_k[-1] * 1e3:.2f}) = {count * 12 / us / 1e6:.2f} TB/s")
    del a, b

    # ---- 2. the micro-step with and without accumulation, alternating
    def micro(j, k, acc):
        (xa, xb), (ua, ub) = steps.micro_ranges(nx, k)[j], steps.micro_ranges(nu, k)[j]
        return eng.step_ssl_cr(te, st, "mse", x[xa:xb], y[xa:xb], u_w[ua:ub], u_s[ua:ub], 1.0, nx_global=nx, nu_global=nu, accumulate=acc)
    for _ in range(3):
        micro(0, 2, False); micro(1, 2, True)
    torch.cuda.synchronize()
    off, on = [], []
    for _ in range(args.reps):
        off.append(timed(lambda: micro(1, 2, False), stream))
        on.append(timed(lambda: micro(1, 2, True), stream))
    m_off, m_on = statistics.median(off), statistics.median(on)
    say(f"2. micro-step 1 of k = 2 (96+224 student, 224 teacher), stream time, {args.reps} alternating pairs:")
    say(f"   without accumulation: median {m_off:.3f} ms (min {min(off):.3f}, max {max(off):.3f})")
    say(f"   accumulating:         median {m_on:.3f} ms (min {min(on):.3f}, max {max(on):.3f})")
    say(f"   added: median {1e3 * (m_on - m_off):.1f} us, of the minima {1e3 * (min(on) - min(off)):.1f} us; pairwise median "
        f"{1e3 * statistics.median(b - a for a, b in zip(off, on)):.1f} us; {count * 12 / SUMSQ_TBS / 1e6:.1f} us = bytes / {SUMSQ_TBS} TB/s")

    # ---- 3. whole optimizer steps over the same global batch
    say(f"3. whole steps over the same global batch (k micro-steps + one Adam step), HIP events over {args.steps} steps after 3 warm-up steps:")
    for k in (1, 2, 4):
        def step():
            if k == 1:
                eng.step_ssl_cr(te, st, "mse", x, y, u_w, u_s, 1.0)
            else:
                for j in range(k):
                    micro(j, k, j > 0)
            st.optimizer_step(opt)
        for _ in range(3):
            step()
        torch.cuda.synchronize()
        t = timed(lambda: [step() for _ in range(args.steps)], stream) / args.steps
        say(f"   k = {k}: {t:.3f} ms per optimizer step = {(nx + 2 * nu) / t * 1e3:.0f} images/s")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
