"""The linear probe restated in float64 (NumPy), its per-element device bounds (torch float64, in the manner of _f64.py), and the
inputs the tests share.  sklearn 1.7.2 pins the objective (tests/test_linprobe_cpu.py); nothing here imports it.

Objective (theta = [W | b], float64 [C][D + 1]):
    F(theta) = sum_i s_i l_i / sum_i s_i + (lam / 2) ||W||^2,   the intercept unpenalised,
    softmax:  l_i = logsumexp(z_i) - z_{i, y_i}      squared:  l_i = 1/2 sum_c (z_ic - t_ic)^2,      z = X W^T + b.
With lam = 1 / (C_reg * sum_i s_i) that is sklearn's LogisticRegression(C = C_reg) objective divided by C_reg * sum_i s_i for three or
more classes; for two classes sklearn fits ONE logit w with C_sklearn: the softmax form at C_reg = C_sklearn / 2 has its optimum at
W = [-w / 2, +w / 2].  Squared with lam equals Ridge(alpha = lam * n) divided by 2 n.

Device bounds (u = 2^-24, X = _f64.EXPLOG_ULP, LAM = 8; E_z the logit bound of a row, Emax its greatest over the row's classes):
  logit     _f64.bound over the D products (fp32 operands) with the bias inside the epilogue count.
  row loss  the device evaluates l at ITS logits: |l(z') - l(z)| <= Emax + E_zy (logsumexp is 1-Lipschitz in the sup norm); the
            evaluation itself errs by _f64.ce_rows's e_row (d_c = z_c - m [1], expf [X], the C-term sum [(C - 1)], logf [X]; the final
            additions are in float64 on the device, ce_rows counts them in float32: a little spare).
            squared: sum_c (|z - t| E_z + E_z^2 / 2), the arithmetic being float64.
  value     sum_i |s_i| e_i / |sum_i s_i|, plus 2^-50 of the magnitude for the float64 sums.
  residual  r = fl32(s (p_c - [c = y])): p errs by p_c (2 Emax e^(2 Emax) [softmax is 2 p_c-Lipschitz] + (|d_c| + X) u [expf] + rel_s
            [the sum]) and the one rounding adds u |p_c - [c = y]| (+ TINY: a flushed subnormal); squared: |s| (E_z + u |z - t|).
  gradient  sum_i |x_id| e_r,ic, plus (LAM sqrt(rows a workgroup owns) + 1) u sum_i |r_ic x_id| for each workgroup's fp32 chain, all
            over |sum_i s_i|; the fold is float64.
"""
import functools
import math
import os

import numpy as np
import torch

import _f64 as f


RATIOS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "linprobe_ratios.txt")
RATIOS_HEAD = ("# the linear probe's measured figures: worst observed / bound of the device comparisons on the MI355X (tests/test_linprobe_gpu.py:\n"
               "# worst_*, fit_*), and max|g| of the float64 restatement at sklearn's solutions (tests/test_linprobe_cpu.py: sklearn_*);\n"
               "# each test rewrites its own lines when it runs\n")


def record(name, value):
    """profiles/linprobe_ratios.txt: one ``name value`` line per measured figure, rewritten in name order"""
    lines = {}
    if os.path.exists(RATIOS):
        with open(RATIOS) as fh:
            lines = dict(ln.split(None, 1) for ln in fh.read().splitlines() if ln.strip() and not ln.startswith("#"))
    lines[name] = f"{value:.4g}"
    with open(RATIOS, "w") as fh:
        fh.write(RATIOS_HEAD + "".join(f"{k} {v}\n" for k, v in sorted(lines.items())))


def fma_chain_logits(x, w, b):
    """[n, C] float32 logits as the device forms them: acc = fmaf(x_d, w_d, acc) over d in RISING order from +0, then ONE float32
    addition of b.  The product of two float32 values is exact in float64; its sum with the accumulator is rounded to 53 bits and then
    to 24, which differs from the single rounding of fmaf only where the 53-bit sum lands on a float32 tie (about 2^-29 of the steps)."""
    x, w, b = np.asarray(x, np.float32), np.asarray(w, np.float32), np.asarray(b, np.float32)
    acc = np.zeros((x.shape[0], w.shape[0]), np.float32)
    for d in range(x.shape[1]):
        acc = (x[:, d, None].astype(np.float64) * w[None, :, d].astype(np.float64) + acc.astype(np.float64)).astype(np.float32)
    return acc + b[None, :]


# ------------------------------------------------------------------------------------------------ float64 restatement (NumPy)
def data_term(X, y, W, b, loss="softmax", s=None):
    """-> (value, gW [C, D], gb [C], Z): the weighted mean loss over the rows and its gradient, float64.  softmax: rows with a label
    outside [0, C) are left out of both sums."""
    X, W, b = np.asarray(X, np.float64), np.asarray(W, np.float64), np.asarray(b, np.float64)
    n, C = X.shape[0], W.shape[0]
    s = np.ones(n) if s is None else np.asarray(s, np.float64)
    Z = X @ W.T + b
    if loss == "softmax":
        y = np.asarray(y).astype(np.int64)
        ok = (y >= 0) & (y < C)
        s = np.where(ok, s, 0.0)
        yc = np.where(ok, y, 0)
        m = Z.max(1, keepdims=True)
        E = np.exp(Z - m)
        S = E.sum(1, keepdims=True)
        rows = (m + np.log(S))[:, 0] - Z[np.arange(n), yc]
        R = E / S
        R[np.arange(n), yc] -= 1.0
    else:
        T = np.asarray(y, np.float64).reshape(n, C)
        R = Z - T
        rows = 0.5 * (R * R).sum(1)
    tot = s.sum()
    R = R * s[:, None]
    return float((s * rows).sum() / tot), R.T @ X / tot, R.sum(0) / tot, Z


def objective(theta, X, y, n_classes, loss="softmax", lam=0.0, s=None, fit_intercept=True):
    """-> (F, g) for theta flat [C (D + 1)], rows [W_c | b_c]; without an intercept column D is held at 0 (its gradient is 0)"""
    D = X.shape[1]
    th = np.asarray(theta, np.float64).reshape(n_classes, D + 1)
    W, b = th[:, :D], th[:, D] if fit_intercept else np.zeros(n_classes)
    v, gW, gb, _ = data_term(X, y, W, b, loss, s)
    g = np.concatenate([gW + lam * W, (gb if fit_intercept else np.zeros(n_classes))[:, None]], 1)
    return v + 0.5 * lam * float((W * W).sum()), g.ravel()


def objective_f32(theta, X, y, n_classes, lam):
    """the softmax objective evaluated in float32 throughout (NumPy float32 arithmetic): a noisy evaluator for the solver's tests"""
    D = X.shape[1]
    th = np.asarray(theta, np.float32).reshape(n_classes, D + 1)
    X = np.asarray(X, np.float32)
    W, b = th[:, :D], th[:, D]
    Z = X @ W.T + b
    m = Z.max(1, keepdims=True)
    E = np.exp(Z - m)
    S = E.sum(1, keepdims=True)
    n = X.shape[0]
    rows = (m + np.log(S))[:, 0] - Z[np.arange(n), y]
    R = E / S
    R[np.arange(n), y] -= np.float32(1)
    inv = np.float32(1.0 / n)
    g = np.concatenate([R.T @ X * inv + np.float32(lam) * W, (R.sum(0) * inv)[:, None]], 1)
    F = rows.sum(dtype=np.float32) * inv + np.float32(0.5 * lam) * (W * W).sum(dtype=np.float32)
    return float(F), g.astype(np.float64).ravel()


def clusters(n, D, C, seed, spread=1.0):
    """Gaussian clusters: C centres N(0, 1) in D dimensions, rows = centre + spread * N(0, 1) -> (X float32 [n, D], y int64 [n])"""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((C, D))
    y = rng.integers(0, C, n)
    y[:C] = np.arange(C)                            # every class present
    X = centres[y] + spread * rng.standard_normal((n, D))
    return X.astype(np.float32), y.astype(np.int64)


# the end-to-end inputs (n, D, C): the float64 restatement alone converges on each at tol = 1e-4 (test_linprobe_cpu.py)
E2E_CASES = [(300, 16, 4), (1000, 64, 9), (2048, 768, 9), (4097, 68, 17), (65, 4, 2)]
E2E_C_REG = 1.0


@functools.lru_cache(maxsize=None)
def e2e_inputs(n, D, C):
    return clusters(n, D, C, seed=1000 + n + D + C, spread=1.0 if D >= 16 else 0.5)


# ------------------------------------------------------------------------------------------------ per-element device bounds
def kernel_inputs(n, D, C, loss, seed, weighted):
    """(x, y, w, b, s) as CPU torch tensors: |logits| of order 1 .. 4, an out-of-range label and a zero weight where there is room"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((n, D), generator=g)
    w = torch.randn((C, D), generator=g) * (2.0 / math.sqrt(D))
    b = torch.randn((C,), generator=g) * 0.5
    if loss == "softmax":
        y = torch.randint(0, C, (n,), generator=g)
        if n >= 3:
            y[1] = C                                # out of range: the row is left out
        if n >= 5:
            y[4] = -1
    else:
        y = torch.randn((n, C), generator=g)
    s = None
    if weighted:
        s = torch.rand((n,), generator=g) + 0.25
        if n >= 4:
            s[3] = 0.0
    return x, y, w, b, s


def device_bounds(x, y, w, b, loss, s, rows_per_group):
    """-> dict of float64 CPU tensors: logits / e_logits [n, C], value / e_value (floats), grad / e_grad [C, D + 1]"""
    n, D = x.shape
    C = w.shape[0]
    z, mag = f.linear_ref(x, w, bias=b.double())
    e_z = f.bound(z, mag, D, 0, fp32_operands=True)
    sw = torch.ones(n, dtype=torch.float64) if s is None else s.double()
    xd = x.double()
    if loss == "softmax":
        ok = (y >= 0) & (y < C)
        sw = torch.where(ok, sw, torch.zeros_like(sw))
        yc = torch.where(ok, y, torch.zeros_like(y))
        rows, e_rows, _, _ = f.ce_rows(z, yc, 1.0)
        emax = e_z.amax(1)
        e_rows = e_rows + emax + e_z.gather(1, yc.view(-1, 1)).squeeze(1)
        m = z.amax(1, keepdim=True)
        d = z - m
        ex = torch.exp(d)
        S = ex.sum(1, keepdim=True)
        p = ex / S
        rel_s = ((p * (d.abs() + f.EXPLOG_ULP)).sum(1, keepdim=True) + (C - 1)) * f.U
        onehot = torch.zeros_like(z).scatter_(1, yc.view(-1, 1), 1.0)
        r = (p - onehot) * sw[:, None]
        em = emax[:, None]
        e_r = sw.abs()[:, None] * (p * (2.0 * em * torch.exp(2.0 * em) + (d.abs() + f.EXPLOG_ULP) * f.U + rel_s) + f.U * (p - onehot).abs() + f.TINY)
    else:
        t = y.double()
        diff = z - t
        rows = 0.5 * (diff * diff).sum(1)
        e_rows = (diff.abs() * e_z + 0.5 * e_z * e_z).sum(1)
        r = diff * sw[:, None]
        e_r = sw.abs()[:, None] * (e_z + f.U * diff.abs() + f.TINY)
    tot = float(sw.sum())
    value = float((sw * rows).sum()) / tot
    e_value = (float((sw.abs() * e_rows).sum()) + 2.0 ** -50 * float((sw.abs() * rows.abs()).sum())) / abs(tot)
    x1 = torch.cat([xd, torch.ones((n, 1), dtype=torch.float64)], 1)
    grad = r.t() @ x1 / tot
    chain = (f.LAM * math.sqrt(rows_per_group) + 1.0) * f.U
    e_grad = (e_r.t() @ x1.abs() + chain * (r.abs().t() @ x1.abs())) / abs(tot) + 2.0 ** -50 * grad.abs()      # (the fold and its division: float64)
    return dict(logits=z, e_logits=e_z, value=value, e_value=e_value, grad=grad, e_grad=e_grad)
