"""CPU self-test of the float64 per-element bounds (tests/_f64.py) that the per-kernel GPU tests apply.

A torch emulation of what a bf16 conv kernel computes -- bf16 operands, fp32 accumulation, the fp32 epilogue
y = relu(fmaf(acc, out_scale, bias) + residual), RNE to bf16 -- must pass the bound, and every fault below must fail it.  The five
precision faults are ones the per-kernel suite's close() (max|got - want| <= tol * max|want| against the fp32 oracle) accepts: the
written reason close() alone is not enough.  The indexing faults fail both checks."""
import pytest
import torch
import torch.nn.functional as F

import _f64 as B
from oracle import kernels_ref as R
from test_kernels_gpu import TOL, close, q, rnd

PRECISION = ["trunc", "bias_bf16", "scale_bf16", "acc_bf16", "channel"]
INDEXING = ["halo_row", "chunk", "neighbour"]
SHAPES = [(2, 16, 16, 64, 64, True), (2, 8, 8, 512, 128, False)]        # N, H, W, C, K, residual: one channel slab / eight


def _conv32(x, w):
    return F.conv2d(x.permute(0, 3, 1, 2), w.permute(0, 3, 1, 2), None, 1, 1).permute(0, 2, 3, 1).contiguous()


def _rne(t):
    return t.float().to(torch.bfloat16).float()


def _trunc(t):
    return (t.float().contiguous().view(torch.int32) & -65536).view(torch.float32)


def _fmaf(a, b, c):
    # one rounding of a * b + c to fp32 (a * b is exact in float64; the float64 sum is rounded once more only below 2^-53)
    return (a.double() * b.double() + c.double()).float()


def emulate(x, w, scale, bias, res, fault=None):
    """the kernel's arithmetic, or the arithmetic with one fault"""
    wf = w.clone()
    if fault == "chunk":
        wf[:, 1, 1, 16:32] = 0.0                 # the centre tap loses one 16-channel chunk
    acc = _conv32(x, wf)
    if fault == "halo_row":
        h = x.shape[1] // 2
        xl = x.clone()
        xl[:, h] = 0.0                           # output row h - 1 (a tile's last) without input row h (its halo row)
        acc[:, h - 1] = _conv32(xl, wf)[:, h - 1]
    if fault == "acc_bf16":
        acc = _rne(acc)                          # double rounding: the accumulator to bf16 ahead of the epilogue
    s = _rne(scale) if fault == "scale_bf16" else scale
    b = _rne(bias) if fault == "bias_bf16" else bias
    v = _fmaf(acc, s, b)
    if res is not None:
        v = v + res
    v = v.clamp_min(0.0)
    if fault == "channel":
        v[..., 5] *= 1.0 + 2.0 ** -7             # one output channel off by a factor
    y = _trunc(v) if fault == "trunc" else _rne(v)
    if fault == "neighbour":
        y[:, 3, 4] = y[:, 3, 5]                  # one pixel written from its right-hand neighbour
    return y, acc


def operands(shape, seed=11):
    N, H, W, C, K, with_res = shape
    x = q(rnd(seed, (N, H, W, C)), 1)
    w = q(rnd(seed + 1, (K, 3, 3, C), 0.05), 1)
    scale = rnd(seed + 2, (K,)).abs() + 0.25
    scale[::3] *= -1.0
    bias = rnd(seed + 3, (K,))
    res = q(rnd(seed + 4, (N, H, W, K)), 1) if with_res else None
    return x, w, scale, bias, res


def reference(x, w, scale, bias, res):
    y64, mag, acc64, amag = B.conv_fwd(x, w, 1, 1, out_scale=scale, bias=bias, residual=res, relu=True)
    n = 9 * x.shape[-1]
    return y64, B.bound(y64, mag, n, 1), acc64, amag, n


@pytest.mark.parametrize("shape", SHAPES)
def test_correct_result_passes(shape):
    x, w, scale, bias, res = operands(shape)
    y64, bnd, acc64, amag, n = reference(x, w, scale, bias, res)
    y, acc = emulate(x, w, scale, bias, res)
    B.check(y, y64, bnd, "emulated bf16 conv")
    # statistics of the fp32 accumulator: fp32 partial sums of 64 pixels each (a wave's rows), summed in double by the check
    K = acc.shape[-1]
    rows = acc.reshape(-1, 64, K)
    B.check_stats(torch.stack([rows.sum(1), (rows * rows).sum(1)], 1), acc64, amag, n, "emulated statistics")


@pytest.mark.parametrize("fault", PRECISION + INDEXING)
@pytest.mark.parametrize("shape", SHAPES)
def test_fault_fails_the_bound(shape, fault):
    x, w, scale, bias, res = operands(shape)
    y64, bnd, _, _, _ = reference(x, w, scale, bias, res)
    y, _ = emulate(x, w, scale, bias, res, fault)
    with pytest.raises(AssertionError, match="worst err/bound"):
        B.check(y, y64, bnd, fault)


@pytest.mark.parametrize("fault", PRECISION)
@pytest.mark.parametrize("shape", SHAPES)
def test_close_accepts_the_precision_faults(shape, fault):
    x, w, scale, bias, res = operands(shape)
    y, _ = emulate(x, w, scale, bias, res, fault)
    close(y, R.conv_fwd(x, w, 1, 1, bias=bias, residual=res, relu=True, out_scale=scale), TOL[1], fault)


@pytest.mark.parametrize("fault", INDEXING)
@pytest.mark.parametrize("shape", SHAPES)
def test_close_rejects_the_indexing_faults(shape, fault):
    x, w, scale, bias, res = operands(shape)
    y, _ = emulate(x, w, scale, bias, res, fault)
    with pytest.raises(AssertionError):
        close(y, R.conv_fwd(x, w, 1, 1, bias=bias, residual=res, relu=True, out_scale=scale), TOL[1], fault)


def test_wgrad_partial_slab_rounded_to_bf16_fails():
    """a weight gradient folded from fp32 partial slabs (one per pixel split) into a non-zero dW passes; the same fold with one
    slab rounded to bf16 fails"""
    N, H, W, C, K = 4, 16, 16, 64, 128
    x, dy = q(rnd(31, (N, H, W, C)), 1), q(rnd(32, (N, H, W, K)), 1)
    base = rnd(33, (K, 3, 3, C))
    want, mag = B.conv_wgrad(x, dy, (K, 3, 3, C), 1, 1, base=base)
    bnd = B.bound(want, mag, N * H * W, 0)
    slabs = [torch.nn.grad.conv2d_weight(x[i:i + 1].permute(0, 3, 1, 2), (K, C, 3, 3), dy[i:i + 1].permute(0, 3, 1, 2), 1, 1)
             .permute(0, 2, 3, 1) for i in range(N)]

    def fold(parts):
        out = base.clone()
        for p in parts:
            out = out + p
        return out
    B.check(fold(slabs), want, bnd, "wgrad from fp32 slabs", dims="krsc")
    slabs[2] = _rne(slabs[2])
    with pytest.raises(AssertionError, match="worst err/bound"):
        B.check(fold(slabs), want, bnd, "wgrad with a slab rounded to bf16", dims="krsc")


# ---------------------------------------------------------------- the input-gradient forms beside par4 (route ops dgrad_t, dgrad_parity, scatter)
def _dgrad32(dy, w, stride, pad, hw):
    shape = (dy.shape[0], w.shape[-1], hw[0], hw[1])
    return torch.nn.grad.conv2d_input(shape, w.permute(0, 3, 1, 2), dy.permute(0, 3, 1, 2), stride, pad).permute(0, 2, 3, 1).contiguous()


def _dgrad_operands(dtype, R, pad, N=3, H=9, W=11, C=64, K=128):
    OH, OW = (H + 2 * pad - R) // 2 + 1, (W + 2 * pad - R) // 2 + 1
    return q(rnd(41, (N, OH, OW, K)), dtype), q(rnd(42, (K, R, R, C), 0.05), dtype), q(rnd(43, (N, H, W, C)), dtype), (H, W)


def _parity_emul(dy, w, res, hw, dtype, fault=None):
    """four launches, one per input-pixel parity class, each with the filter taps of its mask only: fp32 accumulation, the fp32
    residual add, the storage rounding; every launch writes its own class of one NaN-filled buffer"""
    out = torch.full(tuple(res.shape), float("nan"))
    for ph, pw, mask, taps in B.parity_classes():
        keep = [t for t in range(9) if mask >> t & 1]
        if fault == "dropped_tap" and (ph, pw) == (1, 1):
            keep = keep[:-1]                                   # the class of four taps visits three
        wm = torch.zeros_like(w)
        for t in keep:
            wm[:, t // 3, t % 3] = w[:, t // 3, t % 3]
        v = _dgrad32(dy, wm, 2, 1, hw) + res
        if fault == "residual_twice":
            v = v + res
        before = out.clone()
        out[:, ph::2, pw::2] = (_rne(v) if dtype == 1 else v)[:, ph::2, pw::2]
        if fault == "foreign_class" and (ph, pw) == (0, 1):
            out[:, 0, 0] = out[:, 0, 1]                        # a launch that also writes a pixel of class (0, 0)
        B.check_parity_launch(before, out, ph, pw, "emulated parity launch")
    return out


@pytest.mark.parametrize("dtype", [0, 1])
def test_dgrad_parity_bound(dtype):
    dy, w, res, hw = _dgrad_operands(dtype, 3, 1)
    K = dy.shape[-1]
    assert [(c[2], c[3]) for c in B.parity_classes()] == [(0b000010000, 1), (0b000101000, 2), (0b010000010, 2), (0b101000101, 4)]
    want, mag = B.conv_dgrad(dy, w, 2, 1, hw, residual=res)
    bnd = B.parity_bound(want, mag, K, dtype, dtype == 0)
    # each class's bound is the plain one at its own length, below the 9 K bound of the whole filter
    assert bool((bnd < B.bound(want, mag, 9 * K, dtype, dtype == 0)).all())
    assert torch.equal(bnd[:, 1::2, 1::2], B.bound(want, mag, 4 * K, dtype, dtype == 0)[:, 1::2, 1::2])
    B.check(_parity_emul(dy, w, res, hw, dtype), want, bnd, "emulated dgrad by parity classes")
    # ... and the transposed plain form (one launch, all nine taps) against the plain bound
    one = _dgrad32(dy, w, 2, 1, hw) + res
    B.check(_rne(one) if dtype == 1 else one, want, B.bound(want, mag, 9 * K, dtype, dtype == 0), "emulated transposed dgrad")
    for fault in ("dropped_tap", "residual_twice"):
        y = _parity_emul(dy, w, res, hw, dtype, fault)
        with pytest.raises(AssertionError, match="worst err/bound"):
            B.check(y, want, bnd, fault)
    with pytest.raises(AssertionError, match="changed a pixel of another class"):
        _parity_emul(dy, w, res, hw, dtype, "foreign_class")
    hole = torch.full(tuple(res.shape), float("nan"))
    with pytest.raises(AssertionError, match="unwritten"):
        B.check_parity_launch(hole, hole, 0, 0, "a launch that writes nothing")


@pytest.mark.parametrize("dtype", [0, 1])
def test_scatter_accumulate_bound(dtype):
    """the 1x1 / 2 input gradient as the kernel forms it: a 1x1 conv of dY, added in fp32 onto the stored base at the even positions"""
    dy, w, base, hw = _dgrad_operands(dtype, 1, 0, N=2, H=9, W=8, C=128, K=256)
    K = dy.shape[-1]
    want, mag = B.conv_dgrad(dy, w, 2, 0, hw, residual=base)
    bnd = B.bound(want, mag, K, dtype, dtype == 0)
    g = torch.einsum("nhwk,kc->nhwc", dy, w[:, 0, 0])

    def emul(fault=None):
        v = base.clone()
        v[:, ::2, ::2] += g
        if fault == "residual_twice":
            v[:, ::2, ::2] += base[:, ::2, ::2]
        if fault == "odd_position":
            v[:, 1, 2] += g[:, 0, 1]                           # the gradient of (0, 2) lands on (1, 2) as well
        if fault == "odd_rewritten":
            v[:, 1, 1] = v[:, 1, 1] * (1.0 + 2.0 ** -20)       # an unreached position written back through another rounding
        return _rne(v) if dtype == 1 else v
    assert int(B.scatter_reach(base.shape).sum()) == 5 * 4
    B.check_scatter(emul(), base, want, bnd, "emulated scatter-accumulate")
    with pytest.raises(AssertionError, match="worst err/bound"):
        B.check_scatter(emul("residual_twice"), base, want, bnd, "residual_twice")
    with pytest.raises(AssertionError, match="does not reach"):
        B.check_scatter(emul("odd_position"), base, want, bnd, "odd_position")
    if dtype == 0:          # (in bf16 a change of 2^-20 rounds away: the stored value is the base's again)
        with pytest.raises(AssertionError, match="does not reach"):
            B.check_scatter(emul("odd_rewritten"), base, want, bnd, "odd_rewritten")


# ====================================================================================================================
# The non-conv families (BatchNorm finalize / apply / backward, pooling, heads, losses): for each, an emulation of the kernel in fp32
# torch -- the kernel's operations, in another summation order -- passes its bound, and every injected fault fails it.
# CLOSE_ACCEPTS records which of the faults close() (max error against the tensor's maximum) lets through.
# ====================================================================================================================
import math  # noqa: E402

import numpy as np  # noqa: E402

CLOSE_ACCEPTS = {
    "var_fp32": True, "finalize_scale_bf16": True, "act_scale_bf16": True, "stride": False, "argmax_last": True, "window_shift": False,
    "cC_without_mean": False, "gemm_k_group": True, "accumulate_ignored": False, "ce_no_max": False, "loss_scale": False,
}


def _accepted(fn):
    try:
        fn()
        return True
    except AssertionError:
        return False


def _fails(fn):
    with pytest.raises(AssertionError):
        fn()


# ---------------------------------------------------------------- bn_finalize
def _finalize_case(rows=200, C=64, k=16, seed=760):
    g = np.random.RandomState(seed)
    mu, sd = g.standard_normal(C) * 2.0, np.abs(g.standard_normal(C)) + 0.5
    mu[0], sd[0] = 1e3, 1.0
    sd[1], mu[1] = 0.0, 2.5
    v = mu[None, None, :] + sd[None, None, :] * g.standard_normal((rows, k, C))
    part = torch.from_numpy(np.stack([v.sum(1), (v * v).sum(1)], 1).astype(np.float32))
    return part, float(rows * k), rnd(761, (C,)).abs() + 0.5, rnd(762, (C,)), rnd(763, (C,)), rnd(764, (C,)).abs() + 0.5


def _finalize_emul(part, count, gamma, beta, rm, rv, replay, fault=None):
    eps, mom = float(np.float32(1e-5)), torch.tensor(0.1, dtype=torch.float32)
    if fault == "var_fp32":
        s, ss = part[:, 0].sum(0), part[:, 1].sum(0)
        mean = s / np.float32(count)
        var = (ss / np.float32(count) - mean * mean).clamp_min(0).double()
        mean = mean.double()
    else:
        p = part.double().flip(0)                              # double, rows in the opposite order
        mean = p[:, 0].sum(0) / count
        var = (p[:, 1].sum(0) / count - mean * mean).clamp_min(0)
    invstd = 1.0 / torch.sqrt(var + eps)
    sc = gamma.double() * invstd
    if fault == "finalize_scale_bf16":
        sc = _rne(sc).double()
    sh = beta.double() - mean * sc
    unb = var * count / (count - 1.0)
    rm, rv = rm.clone(), rv.clone()
    for _ in range(replay):
        rm = (1 - mom) * rm + mom * mean.float()
        rv = (1 - mom) * rv + mom * unb.float()
    return dict(scale=sc.float(), shift=sh.float(), mean=mean.float(), invstd=invstd.float(), running_mean=rm, running_var=rv)


def _finalize_check(out, ref):
    for k, t in out.items():
        w, e = ref[k]
        B.check(t.view(w.shape), w, e, "bn_finalize " + k, dims="zc")


def test_bn_finalize_bound():
    part, count, gamma, beta, rm, rv = _finalize_case()
    ref = B.bn_finalize_ref(part, count, gamma, beta, rm, rv, replay=3)
    _finalize_check(_finalize_emul(part, count, gamma, beta, rm, rv, 3), ref)
    assert float(ref["invstd"][0][0, 1]) == pytest.approx(1.0 / math.sqrt(float(np.float32(1e-5))))      # the constant channel clamps to var = 0
    want32 = {k: v[0].float() for k, v in ref.items()}
    for fault in ("var_fp32", "finalize_scale_bf16"):
        out = _finalize_emul(part, count, gamma, beta, rm, rv, 3, fault)
        _fails(lambda: _finalize_check(out, ref))
        # close() as test_bn_forward_chain applies it: the scale / shift go through bn_act's output, tolerance 3e-4 of the maximum
        x = rnd(765, (64, 64))
        y = lambda d: x * d["scale"].view(1, -1) + d["shift"].view(1, -1)      # noqa: E731
        assert _accepted(lambda: close(y(out)[:, 1:], y(want32)[:, 1:], 3e-4 if fault == "var_fp32" else 1.5e-2)) == CLOSE_ACCEPTS[fault]


# ---------------------------------------------------------------- bn_act (and the cached-constant defect)
def _act_case(dtype, pixels=1500, C=40):
    x, res = q(rnd(771, (pixels, 1, 1, C), 2.0), dtype), q(rnd(772, (pixels, 1, 1, C)), dtype)
    sc, rsc = rnd(773, (C,)).abs() + 0.25, rnd(774, (C,)).abs() + 0.25
    sc[::3] *= -1.0
    sc[0] *= 1e3
    sc[1] *= 1e-3
    return x, res, sc, rnd(775, (C,)), rsc, rnd(776, (C,))


def _act_emul(x, res, sc, sh, rsc, rsh, dtype, fault=None, cap=1):
    C = x.shape[-1]
    epc = 8 if dtype == 1 else 4
    cols = C // epc
    if fault == "act_scale_bf16":
        sc = _rne(sc)
    if fault == "stride":
        # a grid capped at `cap` workgroups without the rounding: chunk i runs with the constants of column (i mod stride) mod cols
        items = x.numel() // epc
        col = B.cached_column(items, cols, B.capped_grid(items, cap))
        ch = (col.view(-1, 1) * epc + torch.arange(epc).view(1, -1)).reshape(x.shape)
        sc, sh, rsc, rsh = sc[ch], sh[ch], rsc[ch], rsh[ch]
    v = (_fmaf(x, sc, sh) + _fmaf(res, rsc, rsh)).clamp_min(0.0)
    return _rne(v) if dtype == 1 else v


@pytest.mark.parametrize("dtype", [0, 1])
def test_bn_act_bound(dtype):
    x, res, sc, sh, rsc, rsh = _act_case(dtype)
    want, mag = B.bn_act_ref(x, sc, sh, res, rsc, rsh, relu=True)
    bnd = B.bound(want, mag, 0, dtype)
    B.check(_act_emul(x, res, sc, sh, rsc, rsh, dtype), want, bnd, "emulated bn_act")
    # the fix's launch rule: the same cap, rounded -- no thread meets a foreign chunk
    C, epc = x.shape[-1], 8 if dtype == 1 else 4
    items = x.numel() // epc
    assert int((B.cached_column(items, C // epc, B.rounded_grid(items, C // epc, 1)) != torch.arange(items) % (C // epc)).sum()) == 0
    for fault in ("act_scale_bf16", "stride"):
        y = _act_emul(x, res, sc, sh, rsc, rsh, dtype, fault)
        _fails(lambda: B.check(y, want, bnd, fault))
        got = _accepted(lambda: close(y, want.float(), 3e-4 if dtype == 0 else 1.5e-2, fault))
        assert got == (CLOSE_ACCEPTS[fault] and (dtype == 1 or fault != "act_scale_bf16")), (fault, dtype, got)


def test_cached_constant_defect_counts():
    """the index arithmetic of the defect: with the part's 768-workgroup cap, cols = 5 on 204800 chunks hands 8192 chunks foreign
    constants, cols = 7 on 250000 chunks 53392; cols = 3 and every power of two none; the rounded grid none anywhere"""
    for cols, items, wrong in ((5, 204800, 8192), (7, 250000, 53392), (3, 204800, 0), (8, 400000, 0), (10, 204800, None), (6, 250000, 0)):
        col = torch.arange(items) % cols
        n = int((B.cached_column(items, cols, B.capped_grid(items, 768)) != col).sum())
        assert n == wrong or (wrong is None and n > 0), (cols, items, n)
        assert int((B.cached_column(items, cols, B.rounded_grid(items, cols, 768)) != col).sum()) == 0
    for cols in (1, 2, 4, 8, 16, 32, 64, 128, 256):            # every ResNet width: the launch does not change
        for items in (100, 196608, 196609, 10 ** 7):
            assert B.rounded_grid(items, cols, 768) == B.capped_grid(items, 768)


# ---------------------------------------------------------------- max-pool forward / backward, avg-pool
def _pool_emul(x, sc, sh, dtype, fault=None):
    N, H, W, C = x.shape
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    v = _fmaf(x, sc, sh).clamp_min(0.0)
    best = torch.full((N, OH, OW, C), -math.inf)
    arg = torch.zeros((N, OH, OW, C), dtype=torch.long)
    for wi in range(9):
        for oh in range(OH):
            h = 2 * oh - 1 + wi // 3
            if fault == "window_shift" and oh == OH - 1:
                h -= 1                                        # the last output row reads its window one row too high
            if h < 0 or h >= H:
                continue
            ws = [(ow, 2 * ow - 1 + wi % 3) for ow in range(OW) if 0 <= 2 * ow - 1 + wi % 3 < W]
            if not ws:
                continue
            o, w = torch.tensor([a for a, _ in ws]), torch.tensor([b for _, b in ws])
            cand = v[:, h][:, w]
            cur = best[:, oh][:, o]
            take = (cand >= cur) if fault == "argmax_last" else (cand > cur)
            best[:, oh, o] = torch.where(take, cand, cur)
            arg[:, oh, o] = torch.where(take, torch.full_like(arg[:, oh][:, o], wi), arg[:, oh][:, o])
    arg = torch.where(best > 0, arg, torch.full_like(arg, 9))
    return (_rne(best) if dtype == 1 else best), arg


@pytest.mark.parametrize("dtype", [0, 1])
@pytest.mark.parametrize("hw", [(9, 7), (16, 16)])
def test_pool_bounds(hw, dtype):
    N, (H, W), C = 2, hw, 24
    x = q(rnd(781, (N, H, W, C), 2.0), dtype)
    sc, sh = rnd(782, (C,)), rnd(783, (C,))
    sc[1], sh[1] = 0.0, 0.25
    r = B.maxpool_ref(x, sc, sh, dtype)
    assert B.capped(r["unsure"], "near-ties") == 0
    ref_t, idx = F.max_pool2d(F.relu(x.double() * sc.double() + sh.double()).permute(0, 3, 1, 2), 3, 2, 1, return_indices=True)
    assert torch.equal(r["y"], ref_t.permute(0, 2, 3, 1))

    def codes_ok(arg):
        assert bool(((arg == r["code"]) | r["unsure"]).all()), "argmax codes differ from the float64 window"
    y, arg = _pool_emul(x, sc, sh, dtype)
    B.check(y, r["y"], r["bnd"], "emulated max-pool")
    codes_ok(arg)
    # backward through the codes, avg-pool forward / backward: fp32 in another order
    dyp = q(rnd(784, tuple(y.shape)), dtype)
    want, mag = B.maxpool_bwd_ref(dyp, arg, r["pre"], hw)
    act = F.relu(x.double() * sc.double() + sh.double()).permute(0, 3, 1, 2).requires_grad_(True)
    F.max_pool2d(act, 3, 2, 1).backward(dyp.double().permute(0, 3, 1, 2))
    if dtype == 0:                                             # without exact ties autograd routes the gradient the same way
        B.check((act.grad * (act > 0)).permute(0, 2, 3, 1).float()[..., 2:], want[..., 2:], B.bound(want, mag, 0, 0)[..., 2:], "autograd max-pool backward")
    a64, amag, n = B.avgpool_ref(y)
    B.check(y.flip(1).flip(2).sum((1, 2)) * np.float32(1.0 / n), a64, B.bound(a64, amag, n, 0), "emulated avg-pool", dims="nc")
    # faults
    yl, argl = _pool_emul(x, sc, sh, dtype, "argmax_last")
    B.check(yl, r["y"], r["bnd"], "argmax_last values")        # the values are right ...
    _fails(lambda: codes_ok(argl))                             # ... the codes are not (the scale == 0 channel ties everywhere)
    assert _accepted(lambda: close(yl, r["y"].float(), 1e-6 if dtype == 0 else 1e-2)) == CLOSE_ACCEPTS["argmax_last"]
    ys, _ = _pool_emul(x, sc, sh, dtype, "window_shift")
    _fails(lambda: B.check(ys, r["y"], r["bnd"], "window_shift"))
    assert _accepted(lambda: close(ys, r["y"].float(), 1e-6 if dtype == 0 else 1e-2)) == CLOSE_ACCEPTS["window_shift"]


# ---------------------------------------------------------------- bn_bwd: the two sums and dx = cA g + cB x + cC
def _bwd_case(dtype, shape=(3, 10, 10, 128)):
    N, H, W, C = shape
    x = rnd(791, shape, 2.0) + 0.7
    x[..., 2] = rnd(792, shape[:3]) + 30.0                    # mean / std = 30
    x = q(x, dtype)
    dy = q(rnd(793, shape), dtype)
    gamma, beta = rnd(794, (C,)).abs() + 0.5, rnd(795, (C,))
    xs = x.double().reshape(-1, C)
    mean, invstd = xs.mean(0), 1.0 / torch.sqrt(xs.var(0, unbiased=False) + 1e-5)
    return x, dy, (gamma.double() * invstd).float(), (beta.double() - mean * gamma.double() * invstd).float(), mean.float(), invstd.float()


def _bwd_emul(g, x, sc, invstd, mean, count, dtype, fault=None):
    C = x.shape[-1]
    g2, x2 = g.reshape(-1, C), x.reshape(-1, C)
    # the reduce pass: fp32 running sums of 25 pixels each (another grouping than the kernel's), then double
    s0 = g2.reshape(-1, 25, C).sum(1).double().sum(0)
    s1 = (g2 * (x2 - mean)).reshape(-1, 25, C).sum(1).double().sum(0)
    sums = torch.stack([s0, s1])
    invM = np.float32(1.0 / count)
    m0, m1 = s0.float() * invM, s1.float() * invM
    cB = -sc * invstd * invstd * m1
    cC = -sc * m0 - (0.0 if fault == "cC_without_mean" else cB * mean)
    d = _fmaf(sc, g, _fmaf(cB, x, cC))
    return sums, (_rne(d) if dtype == 1 else d)


@pytest.mark.parametrize("dtype", [0, 1])
def test_bn_bwd_bounds(dtype):
    x, dy, sc, sh, mean, invstd = _bwd_case(dtype)
    C, count = x.shape[-1], x.numel() // x.shape[-1]
    g64, gmag = B.bn_bwd_g(dy, x, sc, sh, relu_from_x=True)
    g = g64.float()
    sums, dx = _bwd_emul(g, x, sc, invstd, mean, count, dtype)
    s64, sb = B.bn_bwd_sums_ref(g64, gmag, x, mean)
    B.check(sums.view(1, 2, C), s64, sb, "emulated bn_bwd sums", dims="zsc")
    want, bnd = B.bn_bwd_apply_ref(g64, x, sc, invstd, mean, sums, count, dtype)
    B.check(dx, want, bnd, "emulated bn_bwd dx")
    base_g, base_b = rnd(796, (C,)), rnd(797, (C,))
    wg, bg, wb, bb = B.bn_param_grads_ref(sums, invstd, base_g, base_b)
    B.check(base_g + (sums[1] * invstd.double()).float(), wg, bg, "emulated dgamma", dims="c")
    B.check(base_b + sums[0].float(), wb, bb, "emulated dbeta", dims="c")
    # a reduce pass that rounds (x - mean) to bf16 fails the sums' bound
    bad = torch.stack([sums[0], (g * _rne(x - mean)).reshape(-1, C).double().sum(0)])
    _fails(lambda: B.check(bad.view(1, 2, C), s64, sb, "sums with x - mean in bf16", dims="zsc"))
    _, dxf = _bwd_emul(g, x, sc, invstd, mean, count, dtype, "cC_without_mean")
    _fails(lambda: B.check(dxf, want, bnd, "cC_without_mean"))
    assert _accepted(lambda: close(dxf, want.float(), 5e-4 if dtype == 0 else 2e-2)) == CLOSE_ACCEPTS["cC_without_mean"]


def test_bn_bwd_pooled_reduce_bound():
    """(x - mean) recovered from the stored pool output: the emulation in fp32 passes; recovered without the shift it fails"""
    N, H, W, C = 2, 15, 13, 16
    x = q(rnd(801, (N, H, W, C), 2.0) + 0.7, 1)
    sc, sh, mean = rnd(802, (C,)).abs() + 0.25, rnd(803, (C,)), rnd(804, (C,))
    sc[5], sh[5] = 0.0, 0.25
    y, arg = _pool_emul(x, sc, sh, 1)
    dyp = q(rnd(805, tuple(y.shape)), 1)
    s64, sb = B.bn_bwd_pool_sums_ref(dyp, y, arg, x, sc, sh, mean)

    def emul(with_shift=True):
        rinv = torch.where(sc != 0, 1.0 / sc, torch.zeros_like(sc))
        xm = (y - (sh if with_shift else 0.0)) * rinv - mean
        n = torch.arange(N).view(N, 1, 1).expand(y.shape[:3])
        a5 = arg[..., 5].clamp_max(8)
        h = 2 * torch.arange(y.shape[1]).view(1, -1, 1) - 1 + a5 // 3
        w = 2 * torch.arange(y.shape[2]).view(1, 1, -1) - 1 + a5 % 3
        xm[..., 5] = x[n, h.clamp(0, H - 1), w.clamp(0, W - 1), 5] - mean[5]
        d = torch.where(y > 0, dyp, torch.zeros_like(dyp))
        return torch.stack([d.reshape(-1, C).flip(0).sum(0).double(), (d * xm).reshape(-1, C).flip(0).sum(0).double()])
    B.check(emul(), s64, sb, "emulated pooled reduce", dims="sc")
    _fails(lambda: B.check(emul(False), s64, sb, "pooled reduce without the shift", dims="sc"))


# ---------------------------------------------------------------- heads
@pytest.mark.parametrize("shape", [(37, 70, 10), (96, 256, 64)])
def test_linear_bounds(shape):
    M, Kd, Nn = shape
    x, w, b, base = rnd(811, (M, Kd)), rnd(812, (Nn, Kd), 0.03), rnd(813, (Nn,)), rnd(814, (M, Nn))
    want, mag = B.linear_ref(x, w, bias=b, base=base)
    bnd = B.bound(want, mag, Kd, 0, True)

    def emul(k_end=Kd, accumulate=True):
        acc = torch.zeros((M, Nn))
        for k0 in range(0, k_end, 4):                          # fp32, four k at a time in rising order (the kernel: interleaved over four waves)
            acc = acc + x[:, k0:min(k0 + 4, k_end)] @ w[:, k0:min(k0 + 4, k_end)].t()
        return acc + b + (base if accumulate else 0.0)
    B.check(emul(), want, bnd, "emulated linear", dims="mn")
    for fault, y in (("gemm_k_group", emul(k_end=(Kd - 1) // 4 * 4)), ("accumulate_ignored", emul(accumulate=False))):
        _fails(lambda: B.check(y, want, bnd, fault, dims="mn"))
        assert _accepted(lambda: close(y, want.float(), 5e-2 if fault == "gemm_k_group" else 5e-5)) == CLOSE_ACCEPTS[fault], fault
    g = rnd(815, (M, Nn))
    want, mag = B.colsum_ref(g, b)
    B.check(b + g.flip(0).sum(0), want, B.bound(want, mag, M, 0), "emulated db", dims="n")


# ---------------------------------------------------------------- losses
X_EMUL = 2.0        # the emulation's expf / logf: float64 rounded to fp32 (1 u), doubled like the device constant


def _exp32(t):
    return torch.exp(t.double()).float()


def _ce_emul(l, y, w, no_max=False):
    m = torch.zeros((l.shape[0], 1)) if no_max else l.amax(1, keepdim=True)
    s = _exp32(l - m).flip(1).sum(1, keepdim=True)
    lse = m + torch.log(s.double()).float()
    onehot = torch.zeros_like(l).scatter_(1, y.view(-1, 1), 1.0)
    return (lse - l.gather(1, y.view(-1, 1))).squeeze(1), (_exp32(l - lse) - onehot) * np.float32(w)


@pytest.mark.parametrize("C", [2, 9, 64])
def test_loss_bounds(C):
    nx = 300
    l = rnd(821 + C, (nx, C))
    l = l * (80.0 / float(l.abs().max()))
    l[0] += 100.0
    l[1] -= 100.0
    y = torch.from_numpy(np.random.RandomState(822).randint(0, C, (nx,)).astype(np.int64))
    inx = float(np.float32(1.0 / nx))
    rows, e_rows, dl, e_dl = B.ce_rows(l, y, inx, X=X_EMUL)
    lx, ex = B.loss_total(rows, e_rows, inx, 0)

    def check(r, d, what):
        B.check((r.flip(0).sum() * np.float32(inx)).view(1), torch.tensor([lx], dtype=torch.float64), torch.tensor([ex], dtype=torch.float64), what + " loss", dims="i")
        B.check(d, dl, e_dl, what + " dlogits", dims="nc")
    r, d = _ce_emul(l, y, inx)
    check(r, d, "emulated cross-entropy")
    rf, df = _ce_emul(l, y, inx, no_max=True)
    _fails(lambda: check(rf, df, "ce_no_max"))
    assert _accepted(lambda: close(df, dl.float(), 1e-5)) == CLOSE_ACCEPTS["ce_no_max"]
    # mse over C columns: the mean takes 1 / (nx * C)
    t = rnd(823, (nx,)).abs() * 40.0
    sq, dm, e_dm = B.mse_rows(l, t.view(-1, 1).expand(nx, C), inx)
    lm, em = B.loss_total(sq, torch.zeros(()), inx / C, 3)
    d32 = l - t.view(-1, 1)
    B.check(((d32 * d32).flip(0).sum() * (np.float32(inx) / np.float32(C))).view(1), torch.tensor([lm], dtype=torch.float64),
            torch.tensor([em], dtype=torch.float64), "emulated mse", dims="i")
    B.check(2.0 * d32 * np.float32(inx) / np.float32(C), dm, e_dm, "emulated mse dlogits", dims="nc")
    bad = ((d32 * d32).sum() * np.float32(inx)).view(1)
    _fails(lambda: B.check(bad, torch.tensor([lm], dtype=torch.float64), torch.tensor([em], dtype=torch.float64), "loss_scale", dims="i"))
    assert _accepted(lambda: close(bad, torch.tensor([lm]), 1e-5)) == CLOSE_ACCEPTS["loss_scale"]
    p, pb = B.softmax_col_ref(l, C - 1, X=X_EMUL)
    m = l.amax(1, keepdim=True)
    B.check(_exp32(l - m)[:, C - 1] / _exp32(l - m).sum(1), p, pb, "emulated softmax_col", dims="n")


# ---------------------------------------------------------------- optimizer step
@pytest.mark.parametrize("kind", [0, 1])
def test_optimizer_bounds(kind):
    n = 20000
    p, g, m, v = rnd(831, (n,), 0.1), rnd(832, (n,)), rnd(833, (n,), 0.3), rnd(834, (n,)).abs() * 0.5 + 0.01
    hp = dict(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, wd=1e-4, momentum=0.9, bc1=1 - 0.9 ** 4, bc2=1 - 0.999 ** 4, first_step=0)
    ref = B.optimizer_ref(kind, p, g, m, v, **hp)
    c = {k: torch.tensor(x, dtype=torch.float32) for k, x in hp.items()}

    def emul(fault=None):
        gg = _fmaf(c["wd"], p, g)
        if kind == 0:
            m1 = _fmaf(c["beta1"], m, (1 - c["beta1"]) * gg)
            v1 = _fmaf(c["beta2"], v, (1 - c["beta2"]) * gg * gg)
            den = v1.sqrt() / (1.0 if fault == "no_bias_correction" else c["bc2"].sqrt()) + c["eps"]
            return dict(p=p - (c["lr"] / c["bc1"]) * (m1 / den), s1=m1, s2=v1)
        buf = _fmaf(c["momentum"], m, gg)
        d = buf if fault == "no_nesterov" else _fmaf(c["momentum"], buf, gg)
        return dict(p=p - c["lr"] * d, s1=buf)
    for k, t in emul().items():
        B.check(t, *ref[k], f"emulated optimizer {k}", dims="i")
    bad = emul("no_bias_correction" if kind == 0 else "no_nesterov")
    _fails(lambda: B.check(bad["p"], *ref["p"], "optimizer fault", dims="i"))
    # close() at the existing test's 2e-5 of the largest parameter
    assert _accepted(lambda: close(bad["p"], ref["p"][0].float(), 2e-5)) is False


# ====================================================================================================================
# The fp8 (e4m3) conv path: the float64 quantiser against torch's own conversion, an fp32 torch emulation of the kernel against the
# bound, and the faults the issue names -- each fails the bound on row a of tests/fp8_cases.py; the last column records whether
# close(..., 1.2e-2), the check tests/test_fp8_gpu.py had, accepts it.
# ====================================================================================================================
import _fp8 as F8  # noqa: E402

FP8_ROW_A = (1, 16, 16, 128, 128)
EVAL, TRAIN = "", "in_scale relu_in stats"
FP8_FAULTS = [            # fault, flags, x_scale, close(1.2e-2) accepts
    ("flush", EVAL, 1.0, True),                  # e4m3 subnormals flushed to zero
    ("trunc", EVAL, 1.0, True),                  # truncation instead of rounding
    ("trunc", TRAIN, 1.0, False),
    ("ties_away", EVAL, 1.0, True),              # ties away from zero: the eval flags, where bf16 activations sit on e4m3 ties
    ("dequant_next", EVAL, 1.0, False),          # dequant of channel k taken from k + 1
    ("dequant_next", TRAIN, 1.0, False),
    ("scale_without_xs", TRAIN, 0.25, False),    # in_scale not multiplied by x_scale
    ("scale_without_xs", TRAIN, 3.0, False),
    ("halo_pixel", EVAL, 1.0, False),            # one halo pixel of one tile dropped
    ("halo_pixel", TRAIN, 1.0, True),            # (the 1e3 in_scale channel sets close()'s scale: the lost tap disappears under it)
]


def _to8(t):
    return t.clamp(-448.0, 448.0).float().to(torch.float8_e4m3fn).float().double()


def test_e4m3_quantiser_equals_torch_conversion():
    codes = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).float()
    fin = codes[torch.isfinite(codes)].double().sort().values
    assert fin.numel() == 254 and float(fin.abs().max()) == 448.0
    assert torch.equal(B.e4m3(fin), fin)
    mid = (fin[1:] + fin[:-1]) / 2                # 253 midpoints (the one between -0 and +0 is 0): every tie of the format
    assert mid.numel() == 253
    assert torch.equal(B.e4m3(mid), _to8(mid))
    grid = torch.linspace(-460.0, 460.0, 200001, dtype=torch.float64).float().double()
    assert torch.equal(B.e4m3(grid), _to8(grid))
    tiny = torch.tensor([2.0 ** -10, 2.0 ** -10 * (1 + 2.0 ** -20), 3 * 2.0 ** -10, 2.0 ** -9, -2.0 ** -10], dtype=torch.float64)
    assert B.e4m3(tiny).tolist() == [0.0, 2.0 ** -9, 2.0 ** -8, 2.0 ** -9, -0.0]
    assert bool(torch.signbit(B.e4m3(tiny))[4])


def test_fp8_pack_and_scale_update_references():
    w = rnd(841, (8, 4, 3, 3), 0.05)
    w[3] = 0.0
    w[5] *= 448.0 * 2.0 ** -15 / float(w[5].abs().max())
    w[5].view(-1)[int(w[5].abs().argmax())] = 448.0 * 2.0 ** -15
    wq, dq, _ = B.fp8_pack_ref(w)
    assert float(dq[3]) == 1.0 and float(wq[3].abs().max()) == 0.0
    assert float(dq[5]) == 2.0 ** -15 and float(wq[5].abs().max()) == 448.0
    top = wq.abs().flatten(1).max(1).values
    assert bool(((top > 224.0) & (top <= 448.0))[[0, 1, 2, 4, 5, 6, 7]].all())
    wo, do, _ = R.fp8_weight_pack(w)              # the fp32 oracle's restatement, on filters away from the frexp edge
    keep = [0, 1, 2, 3, 4, 6, 7]
    assert torch.equal(wq.permute(0, 3, 1, 2)[keep], wo.double()[keep]) and torch.equal(dq[keep], do.double()[keep])
    s = torch.tensor([[3.0, 224.0], [3.0, 448.0], [3.0, 223.0], [3.0, 225.0], [3.0, 0.0], [3.0, float("nan")], [3.0, float("inf")],
                      [3.0, 3.2e38], [3.0, 1e-30], [3.0, 1e30], [3.0, -1.0]])
    assert B.fp8_scale_update_ref(s).tolist() == [[1.0, 0.0], [0.5, 0.0], [1.0, 0.0], [0.5, 0.0], [3.0, 0.0], [3.0, 0.0], [3.0, 0.0], [3.0, 0.0],
                                                  [65536.0, 0.0], [2.0 ** -16, 0.0], [3.0, 0.0]]


@pytest.mark.parametrize("shape", [(2, 16, 16, 128, 128), (2, 16, 16, 512, 128)])
def test_fp8_emulation_holds_the_bound(shape):
    t = F8.inputs(shape)
    for flags in (EVAL, TRAIN, "in_scale stats", "bias residual relu"):
        r = F8.reference(shape, flags, 1.0, t)
        y, st = F8.emulate(shape, flags, 1.0, t)
        B.check(y, r["y"], r["bnd"], f"emulated fp8 conv [{flags}]")
        if "stats" in flags:
            B.check_stats(st, r["acc"], r["amag"], r["n"], "emulated fp8 statistics")      # (without the alignment term: fp32 sums)
    # the fp32 accumulation alone (no bf16 rounding of the output) sits far inside the bound: the room the MFMA's summation has
    r = F8.reference(shape, TRAIN, 1.0, t)
    _, st = F8.emulate(shape, TRAIN, 1.0, t)
    e = B.bound(r["acc"], r["amag"], r["n"], 0)
    xq, _ = B.fp8_activations(t["x"], 1.0, t["in_scale"], t["in_shift"], True)
    wq, dq, _ = B.fp8_pack_ref(t["w"])
    acc32 = F.conv2d(xq.float().permute(0, 3, 1, 2), wq.float().permute(0, 3, 1, 2), None, 1, 1).permute(0, 2, 3, 1) * dq.float()
    assert B.check(acc32, r["acc"], e, "fp32 convolution of the quantised operands") < 0.1


def test_fp8_flush_under_a_saturated_channel_is_what_the_alignment_term_costs():
    """with the train flags channel 0 (in_scale about 1e3) saturates at 448 in every instruction: the measured alignment term of the fp8
    MFMA (B.FP8_MFMA_U) is then larger than what flushed subnormals change -- bound() alone rejects the fault there (2.8 x on 77
    elements), the fp8 bound does not.  The rows without the transform keep rejecting it (FP8_FAULTS)."""
    t = F8.inputs(FP8_ROW_A)
    r = F8.reference(FP8_ROW_A, TRAIN, 1.0, t)
    y, _ = F8.emulate(FP8_ROW_A, TRAIN, 1.0, t, "flush")
    _fails(lambda: B.check(y, r["y"], B.bound(r["y"], r["mag"], r["n"], 1), "flush, bound() alone"))
    B.check(y, r["y"], r["bnd"], "flush, with the alignment term")


def test_fp8_amax_interval():
    """with ReLU and a large negative pre-activation the interval is wide, without ReLU it is a point"""
    t = F8.inputs(FP8_ROW_A)
    hi, lo = F8.reference(FP8_ROW_A, TRAIN, 1.0, t)["amax"]
    assert hi > 1e5 and lo < hi / 2 and lo > 448.0
    hi, lo = F8.reference(FP8_ROW_A, "in_scale stats", 1.0, t)["amax"]
    assert hi == lo
    hi, lo = F8.reference(FP8_ROW_A, EVAL, 16.0, t)["amax"]
    assert hi == lo == 1000.0


@pytest.mark.parametrize("fault, flags, xs, close_accepts", FP8_FAULTS, ids=[f"{f[0]}-{'train' if f[1] else 'eval'}-xs{f[2]:g}" for f in FP8_FAULTS])
def test_fp8_fault_fails_the_bound(fault, flags, xs, close_accepts):
    t = F8.inputs(FP8_ROW_A)
    r = F8.reference(FP8_ROW_A, flags, xs, t)
    y, _ = F8.emulate(FP8_ROW_A, flags, xs, t, fault)
    with pytest.raises(AssertionError, match="worst err/bound"):
        B.check(y, r["y"], r["bnd"], fault)
    assert _accepted(lambda: close(y, r["y"].float(), 1.2e-2, fault)) == close_accepts
