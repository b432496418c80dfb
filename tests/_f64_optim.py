"""float64 references with per-element bounds for the grouped optimizer step: AdamW (sslcr_opt_desc.kind 2) and the global gradient
norm / clipping coefficient (sslcr_grad_norm).  Adam and SGD-Nesterov are _f64.optimizer_ref; optimizer_ref() below dispatches on
the kind so that a test can walk a group table.  tests/test_optim_groups_cpu.py pins every reference here to torch.optim.AdamW /
Adam / SGD(nesterov=True) and torch.nn.utils.clip_grad_norm_ on float64 tensors (1e-12 relative over three steps).

AdamW, one step from a non-zero fp32 state (optim.hip: opt_row + opt_update_g).  u-counts per line of the kernel:
  keep = 1 - lr * wd                                     [2]  e_keep = u (|keep| + lr wd)       (a contraction to one fma only lowers it)
  pd = p * keep                                          [1]  e_pd = u |pd| + |p| e_keep
  g = graw * gs                                          [1]  e_g = u |g|          (gs = grad_scale * coef: exact for grad_scale = 1)
  m' = fmaf(b1, m, (1 - b1) * g)                         [3]  e_m = 3u (|b1 m| + |(1 - b1) g|) + (1 - b1) e_g
  v' = fmaf(b2, v, (1 - b2) * g * g)                     [4]  e_v = 4u (b2 v + (1 - b2) g^2) + (1 - b2) 2 |g| e_g
  denom = sqrtf(v') / sqrtf(bc2) + eps                   [4]  rel. 4u + e_v / (2 v')  (v' > 0: the state starts away from zero)
  p' = pd - (lr / bc1) * (m' / denom)                    [3 on the step, 1 on the difference]

Gradient norm (optim.hip: grad_sumsq_kernel + grad_norm_finalize_kernel):
  sum = sum_i (double)g_i * (double)g_i   every product exact (48 significand bits); n - 1 + partials double additions in a fixed
                                          order: relative error of the sum <= (n + partials) 2^-53, of its square root half that
  norm = (float)sqrt(sum)                 the double sqrt and the rounding to fp32
  => |norm - norm64| <= (2^-24 + (n + partials + 8) 2^-53) norm64
  coef = fminf(1, max_norm / (norm + 1e-6f))   three further fp32 roundings (the constant 1e-6f, the sum, the quotient) on top of
                                          the propagated norm error: |coef - c64| <= 3u c64 + c64 e_norm / (norm64 + 1e-6), with
                                          c64 = max_norm / (norm64 + 1e-6) before the clamp; min(1, .) is 1-Lipschitz, and where
                                          c64 - that bound >= 1 (max_norm = inf included) the kernel's value is exactly 1.0f.
"""
import math

import torch

import _f64 as B
from _f64 import U, f32


def adamw_ref(p, graw, s1, s2, *, lr, beta1, beta2, eps, wd, bc1, bc2, grad_scale=1.0, **_unused):
    """-> dict name -> (want64, bound) for p, s1, s2; every scalar as the fp32 the kernel receives"""
    lr, beta1, beta2, eps, wd, bc1, bc2, gs = (f32(v) for v in (lr, beta1, beta2, eps, wd, bc1, bc2, grad_scale))
    p, graw, m, v = p.double(), graw.double(), s1.double(), s2.double()
    keep = 1 - lr * wd
    e_keep = U * (abs(keep) + lr * wd)
    pd = p * keep
    e_pd = U * pd.abs() + p.abs() * e_keep
    g = graw * gs
    e_g = U * g.abs()
    m1 = beta1 * m + (1 - beta1) * g
    e_m = 3 * U * ((beta1 * m).abs() + ((1 - beta1) * g).abs()) + (1 - beta1) * e_g
    v1 = beta2 * v + (1 - beta2) * g * g
    e_v = 4 * U * (beta2 * v + (1 - beta2) * g * g) + (1 - beta2) * 2 * g.abs() * e_g
    root = torch.sqrt(v1) / math.sqrt(bc2)
    denom = root + eps
    e_den = 4 * U * denom + root * e_v / (2 * v1)
    step = (lr / bc1) * (m1 / denom)
    e_step = 3 * U * step.abs() + (lr / bc1) * (e_m / denom + m1.abs() * e_den / (denom * denom))
    p1 = pd - step
    return dict(p=(p1, U * p1.abs() + e_pd + e_step), s1=(m1, e_m), s2=(v1, e_v))


def optimizer_ref(kind, p, graw, s1, s2, **hp):
    """one row of a group table: kind 0 Adam / 1 SGD-Nesterov (_f64.optimizer_ref), 2 AdamW"""
    hp = {k: v for k, v in hp.items() if k != "kind"}
    if kind == 2:
        return adamw_ref(p, graw, s1, s2, **hp)
    return B.optimizer_ref(kind, p, graw, s1, s2 if s2 is not None else torch.zeros_like(s1), **hp)


def grad_norm_ref(g, max_norm, partials):
    """g: every gradient element the kernel reduces (any shape) -> dict(norm=(norm64, bound), coef=(coef64, bound), exact_one=bool);
    max_norm as the fp32 the kernel receives"""
    max_norm = f32(max_norm)
    g = g.detach().cpu().double().flatten()
    n = g.numel()
    norm = math.sqrt(float((g * g).sum()))
    e_norm = (2.0 ** -24 + (n + partials + 8) * 2.0 ** -53) * norm
    raw = float(max_norm) / (norm + 1e-6)                       # +inf for max_norm = inf
    if math.isinf(raw):
        return dict(norm=(norm, e_norm), coef=(1.0, 0.0), exact_one=True)
    e_raw = 3 * U * raw + raw * e_norm / (norm + 1e-6)
    return dict(norm=(norm, e_norm), coef=(min(1.0, raw), e_raw), exact_one=raw - e_raw >= 1.0)
