"""float64 references with per-element error bounds, for the per-kernel GPU tests and their CPU self-test.

Each reference computes, in float64, the operation a kernel performs on the operands AS THE KERNEL SEES THEM (inputs already
rounded to the storage dtype, the prologue operand rounded the way the kernel rounds it), together with a magnitude companion:
the same operation on absolute values.  A kernel result must then hold, element by element,

    |got - y64| <= u_out*|y64| + (u_out + 1) * (LAM*sqrt(n) + EPI [+ 1 for fp32 operands]) * 2^-24 * mag

Derivation.  The kernel forms v, the fp32 result before the output rounding; got = round(v).
  * bf16 operands: a bf16 x bf16 product is exact in fp32, so the only fp32 error of the reduction is its n - 1 additions.
    By Higham & Mary (probabilistic rounding error analysis, SIAM J. Sci. Comput. 2019) |sum error| <= LAM*sqrt(n)*u*sum|x_i w_i|
    with probability >= 1 - 2*exp(-LAM^2 / 2): LAM = 8 fails ~2.5e-14 of elements by chance.  fp32 operands add at most u per
    product, u*mag in all.
  * the epilogue is at most EPI = 4 rounded fp32 operations on values bounded by mag (scale multiply or fma, bias add, residual
    add, the add into an existing fp32 value): EPI*u*mag.  ReLU is 1-Lipschitz, so the bound of the pre-activation carries over.
  * |v - y64| <= E (the two items above); the RNE output rounding adds |round(v) - v| <= u_out*|v| <= u_out*(|y64| + E).
    u_out = 2^-8 for bf16 output (8 significand bits), 0 for fp32 output.
No element is excused: a single element over its bound fails the check.

BatchNorm partial statistics are sums over the fp32 ACCUMULATOR (before the output rounding): per channel the error of
sum(acc) is at most sum(E_i) + LAM*sqrt(M)*u*sum|acc|, that of sum(acc^2) at most sum(2|acc|E_i + E_i^2) + LAM*sqrt(M)*u*sum(acc^2)
(each fp32 fmaf(q, q, s) of the kernel is one rounding of the running sum), M the number of pixels summed.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24          # fp32 unit roundoff
U_BF16 = 2.0 ** -8      # bf16 unit roundoff (RNE, 8 significand bits)
LAM = 8.0               # Higham & Mary's probabilistic constant
EPI = 4.0               # rounded fp32 operations after the reduction (see the module text)

THREADS = 16            # the float64 references run on at most this many CPU threads
if torch.get_num_threads() > THREADS:
    torch.set_num_threads(THREADS)


def storage(t, dtype):
    """round an fp32 value to the engine storage dtype (0 fp32, 1 bf16, RNE) -> float64"""
    t = t.float()
    return (t.to(torch.bfloat16) if dtype == 1 else t).double()


def xform(x, scale, shift, relu, dtype):
    """the consumer-side BatchNorm apply as every conv / wgrad prologue does it: q = fmaf(x, scale, shift) (one rounding to fp32),
    clamp at 0 with in_relu, round to the storage dtype.  (x * scale + shift is exact in float64 for a bf16 x and fp32 scale /
    shift unless their exponents lie more than ~2^20 apart, and even then the float64 -> fp32 rounding differs from fmaf's only
    on an exact float64 tie.)  -> float64"""
    q = (x.double() * scale.double() + shift.double()).float()
    if relu:
        q = q.clamp_min(0.0)
    return storage(q, dtype)


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def epilogue(acc, amag, *, out_scale=None, bias=None, residual=None, relu=False):
    """y = relu(acc * out_scale + bias + residual) in float64, and its magnitude companion"""
    y, mag = acc, amag
    if out_scale is not None:
        s = out_scale.double()
        y, mag = y * s, mag * s.abs()
    if bias is not None:
        b = bias.double()
        y, mag = y + b, mag + b.abs()
    if residual is not None:
        r = residual.double()
        y, mag = y + r, mag + r.abs()
    if relu:
        y = y.clamp_min(0.0)
    return y, mag


def conv_fwd(x, w, stride, pad, **epi):
    """x NHWC, w KRSC (as the kernel reads them) -> (y64, mag, acc64, accmag), NHWC float64; reduction length R*S*C"""
    wd = w.double().permute(0, 3, 1, 2)
    acc = _nhwc(F.conv2d(_nchw(x.double()), wd, None, stride, pad))
    amag = _nhwc(F.conv2d(_nchw(x.double().abs()), wd.abs(), None, stride, pad))
    y, mag = epilogue(acc, amag, **epi)
    return y, mag, acc, amag


def conv_dgrad(dy, w, stride, pad, in_hw, residual=None):
    """input gradient of the conv (dy NHWC, w KRSC) -> (dx64, mag) NHWC [+ residual]; reduction length R*S*K"""
    K, R, S, C = w.shape
    shape = (dy.shape[0], C, in_hw[0], in_hw[1])
    wd = w.double().permute(0, 3, 1, 2)
    dx = _nhwc(torch.nn.grad.conv2d_input(shape, wd, _nchw(dy.double()), stride, pad))
    mag = _nhwc(torch.nn.grad.conv2d_input(shape, wd.abs(), _nchw(dy.double().abs()), stride, pad))
    return epilogue(dx, mag, residual=residual)


def conv_wgrad(x, dy, w_shape, stride, pad, base=None):
    """weight gradient (x, dy NHWC) -> (dw64, mag) KRSC [+ the fp32 dW it accumulates into]; reduction length N*OH*OW"""
    K, R, S, C = w_shape
    dw = torch.nn.grad.conv2d_weight(_nchw(x.double()), (K, C, R, S), _nchw(dy.double()), stride, pad)
    mag = torch.nn.grad.conv2d_weight(_nchw(x.double().abs()), (K, C, R, S), _nchw(dy.double().abs()), stride, pad)
    return epilogue(dw.permute(0, 2, 3, 1).contiguous(), mag.permute(0, 2, 3, 1).contiguous(),
                    residual=None if base is None else base.double())


def bound(y64, mag, n, out_dtype, fp32_operands=False):
    """per-element bound of |got - y64| (module text); out_dtype 1 = bf16 output, 0 = fp32 output"""
    u_out = U_BF16 if out_dtype == 1 else 0.0
    e = (LAM * math.sqrt(n) + EPI + (1.0 if fp32_operands else 0.0)) * U
    return u_out * y64.abs() + (1.0 + u_out) * e * mag


def ratio(got, want, bnd):
    """err / bound per element (inf where the bound is 0 and the element differs, or where got is not finite)"""
    got = got.detach().cpu().double()
    err = (got - want).abs()
    r = torch.where(bnd > 0, err / bnd.clamp_min(1e-300), torch.where(err > 0, math.inf, 0.0))
    return torch.where(torch.isfinite(got), r, torch.full_like(r, math.inf))


def report(what, kernel, worst):
    print(f"[f64] {what} | {kernel} | worst err/bound {worst:.4f}")


def check(got, want, bnd, what, kernel="", dims="nhwk"):
    """assert every element within its bound; on failure name the worst element (index over `dims`) and the kernel"""
    r = ratio(got, want, bnd)
    i = int(r.flatten().argmax())
    worst = float(r.flatten()[i])
    if not worst <= 1.0:
        idx = tuple(int(v) for v in np.unravel_index(i, tuple(r.shape)))
        g = float(got.detach().cpu().double().flatten()[i])
        raise AssertionError(f"{what} [{kernel}]: worst err/bound {worst:.3g} at ({','.join(dims[:len(idx)])}) = {idx}: "
                             f"got {g!r} want {float(want.flatten()[i])!r} bound {float(bnd.flatten()[i]):.3e}; "
                             f"{int((r > 1).sum())} of {r.numel()} elements over")
    report(what, kernel, worst)
    return worst


def stats_bound(acc, amag, n, fp32_operands=False):
    """-> (sum64, sumsq64, bound of sum, bound of sumsq) per channel of the accumulator acc [..., K] (module text)"""
    K = acc.shape[-1]
    a = acc.reshape(-1, K)
    e = bound(a, amag.reshape(-1, K), n, 0, fp32_operands)
    g = LAM * math.sqrt(a.shape[0]) * U
    return a.sum(0), (a * a).sum(0), e.sum(0) + g * a.abs().sum(0), (2 * a.abs() * e + e * e).sum(0) + g * (a * a).sum(0)


def check_stats(stats, acc, amag, n, what, kernel="", fp32_operands=False):
    """stats: the kernel's partial rows [rows, 2, K] fp32 (summed here in double)"""
    st = stats.detach().cpu().double().sum(0)
    s, ss, bs, bss = stats_bound(acc, amag, n, fp32_operands)
    w1 = check(st[0], s, bs, what + " sum", kernel, dims="k")
    w2 = check(st[1], ss, bss, what + " sumsq", kernel, dims="k")
    return max(w1, w2)
