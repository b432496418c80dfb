"""Thin torch-tensor front end of the per-kernel C-ABI entry points (include/sslcr.h).

Tensors are only device memory here: every function fills a descriptor with raw pointers/sizes and calls
libsslcr.so on the current HIP stream.  Activations NHWC, weights KRSC; ``dtype`` 0 = fp32, 1 = bf16.
"""
import torch

from . import _lib as L

F32, BF16 = 0, 1


def tdtype(dtype):
    return torch.bfloat16 if dtype == BF16 else torch.float32


def _dt(t):
    if t.dtype == torch.bfloat16:
        return BF16
    if t.dtype == torch.float32:
        return F32
    raise TypeError(f"unsupported activation dtype {t.dtype}")


def _chk(*ts):
    for t in ts:
        if t is not None:
            if not t.is_cuda:
                raise L.SslcrError("sslcr kernels need device tensors (no CPU fallback)")
            if not t.is_contiguous():
                raise L.SslcrError("sslcr kernels need contiguous tensors")


def _out(out, shape, dtype, device, rule):
    """``out`` as the caller gave it, held to shape, dtype and device (rule: the error's text), or a new tensor of them"""
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    if out.dtype != dtype or tuple(out.shape) != tuple(shape) or out.device != device:
        raise L.SslcrError(rule)
    return out


def _u8(t):
    """a bool tensor viewed as uint8 (the same bytes, False = 0 and True = 1); any other tensor as it is, for the caller's dtype check"""
    return t.view(torch.uint8) if t.dtype == torch.bool else t


def switches():
    """the library's SSLCR_* environment switches as it read them (include/sslcr.h, the table above sslcr_switch_info): {name: {group,
    rule, when, default, set, value, meaning}} in the table's order.  Needs no device; `set` and `value` are what THIS process runs with
    -- a misspelt variable shows up here as a switch that is not set."""
    lib, out, r = L.lib(), {}, L.SwitchRow()
    for i in range(lib.sslcr_switch_count()):
        L.check(lib.sslcr_switch_info(i, r))
        out[r.name.decode()] = {"group": r.group.decode(), "rule": r.rule.decode(), "when": r.when.decode(), "default": r.dflt,
                                "set": bool(r.is_set), "value": r.value, "meaning": r.meaning.decode()}
    return out


last_conv_kernel = ""        # kernel instance the most recent conv2d() launched (rocprofv3 spelling), for tests / profiles
last_wgrad_kernel = ""       # ... and the most recent conv2d_wgrad()
last_stem_wgrad_kernel = ""  # ... and the most recent stem_wgrad_pool()


def conv2d(x, w, stride, pad, *, in_scale=None, in_shift=None, in_relu=False, bias=None, residual=None, relu=False,
           want_stats=False, out=None, transposed=False, out_hw=None, osh=1, accumulate=False, pixel_hw=None,
           pix_mul=0, pix_off=(0, 0), tap_mask=0, mask=None, par4=False, seg_images=0, out_scale=None):
    """x NHWC [N,H,W,C], w KRSC [K,R,S,C] -> y NHWC (+ partial stats [rows,2,K] fp32).

    out_scale [K] (with bias): y = epilogue(acc * out_scale + bias): eval-mode BatchNorm with its scale kept out of the filters.
    transposed=True is the dgrad gather: pixel space = the conv's input (pixel_hw), x = dY, w = [C][R][S][K].
    mask = (x_bn [like y], scale [K], shift [K], mean [K]): BatchNorm-backward front end, see sslcr_conv_desc.mask_x.
    seg_images > 0: N / seg_images segments in one launch (in_scale / in_shift [nseg, C]; stats rows split by segment)."""
    _chk(x, w, in_scale, in_shift, bias, residual, out, out_scale)
    dt = _dt(x)
    N, H, W, C = x.shape
    K, R, S, C2 = w.shape
    assert C2 == C and w.dtype == x.dtype
    if transposed:
        PH, PW = pixel_hw
    else:
        PH, PW = (H + 2 * pad - R) // stride + 1, (W + 2 * pad - S) // stride + 1
    OH, OW = out_hw if out_hw is not None else (PH * osh, PW * osh)
    y = out if out is not None else torch.empty((N, OH, OW, K), dtype=x.dtype, device=x.device)
    d = L.ConvDesc(L.ptr(x), L.ptr(w), L.ptr(y), L.ptr(in_scale), L.ptr(in_shift), L.ptr(bias), L.ptr(residual), None,
                   N, H, W, C, K, R, S, stride, pad, PH, PW, OH, OW, osh, int(transposed), int(in_relu), int(relu),
                   int(accumulate), int(pix_mul), int(pix_off[0]), int(pix_off[1]), int(tap_mask))
    d.par4 = int(par4)
    d.out_scale = L.ptr(out_scale)
    if seg_images:
        d.seg_images = int(seg_images)
        d.seg_stride = int(in_scale.stride(0)) if in_scale is not None and in_scale.dim() == 2 else 0
        if not L.lib().sslcr_conv2d_segments_ok(dt, d):
            raise L.SslcrError("conv2d: no segment form for this shape / dtype")
    if mask is not None:
        _chk(*mask)
        d.mask_x, d.mask_scale, d.mask_shift, d.mask_mean = (L.ptr(t) for t in mask)
    stats = None
    if want_stats:
        rows = L.lib().sslcr_conv2d_partial_rows(d)
        # NaN-poisoned: the launch must write every row it announced (a row left as found once went unnoticed here and blew up
        # the engine's BatchNorm, whose scratch is reused)
        stats = torch.full((rows, 2, K), float("nan"), dtype=torch.float32, device=x.device)
        d.stats = L.ptr(stats)
    global last_conv_kernel
    last_conv_kernel = L.lib().sslcr_conv2d_kernel_name(dt, d).decode()
    L.check(L.lib().sslcr_conv2d(dt, d, L.stream_ptr()))
    return (y, stats) if want_stats else y


def conv2d_s2_pair(x, w3, w1, *, bias3=None, bias1=None, relu3=False, want_stats=False, scale3=None, scale1=None):
    """a downsampling BasicBlock's conv1 (3x3 / 2 / pad 1, w3 [K,3,3,C]) and projection (1x1 / 2, w1 [K,1,1,C]) of ONE input in one
    launch (sslcr_conv2d_s2_pair) -> (y3, yd) or (y3, yd, stats3, statsd)"""
    _chk(x, w3, w1, bias3, bias1, scale3, scale1)
    dt = _dt(x)
    N, H, W, C = x.shape
    K = w3.shape[0]
    assert w3.shape == (K, 3, 3, C) and w1.shape == (K, 1, 1, C)
    PH, PW = H // 2, W // 2
    y3 = torch.empty((N, PH, PW, K), dtype=x.dtype, device=x.device)
    yd = torch.empty_like(y3)
    d3 = L.ConvDesc(L.ptr(x), L.ptr(w3), L.ptr(y3), None, None, L.ptr(bias3), None, None,
                    N, H, W, C, K, 3, 3, 2, 1, PH, PW, PH, PW, 1, 0, 0, int(relu3), 0, 0, 0, 0, 0)
    d1 = L.ConvDesc(L.ptr(x), L.ptr(w1), L.ptr(yd), None, None, L.ptr(bias1), None, None,
                    N, H, W, C, K, 1, 1, 2, 0, PH, PW, PH, PW, 1, 0, 0, 0, 0, 0, 0, 0, 0)
    d3.out_scale, d1.out_scale = L.ptr(scale3), L.ptr(scale1)
    s3 = sd = None
    if want_stats:
        rows = L.lib().sslcr_conv2d_partial_rows(d3)
        s3 = torch.full((rows, 2, K), float("nan"), dtype=torch.float32, device=x.device)
        sd = torch.full((rows, 2, K), float("nan"), dtype=torch.float32, device=x.device)
        d3.stats, d1.stats = L.ptr(s3), L.ptr(sd)
    if not L.lib().sslcr_conv2d_s2_pair_ok(dt, d3, d1):
        raise L.SslcrError("conv2d_s2_pair: not served")
    L.check(L.lib().sslcr_conv2d_s2_pair(dt, d3, d1, L.stream_ptr()))
    return (y3, yd, s3, sd) if want_stats else (y3, yd)


def pack_conv_fp8(w_kcrs, *, bn=None, eps=1e-5):
    """PyTorch [K,C,3,3] fp32 -> (w8 [K,3,3,C] uint8 = OCP e4m3 bits, w_dequant [K] fp32, bias [K] | None): per-output-channel
    power-of-two scale (amax -> (224, 448]); bn = (gamma, beta, running_mean, running_var) folds eval-mode BatchNorm."""
    _chk(w_kcrs)
    K, C, R, S = w_kcrs.shape
    assert R == 3 and S == 3
    dev = w_kcrs.device
    w8 = torch.empty((K, 3, 3, C), dtype=torch.uint8, device=dev)
    dq = torch.empty(K, dtype=torch.float32, device=dev)
    bias = torch.empty(K, dtype=torch.float32, device=dev) if bn is not None else None
    g, b, rm, rv = bn if bn is not None else (None, None, None, None)
    d = L.PackFp8Desc(L.ptr(w_kcrs), L.ptr(w8), L.ptr(dq), L.ptr(g), L.ptr(b), L.ptr(rm), L.ptr(rv), eps, L.ptr(bias), K, C)
    L.check(L.lib().sslcr_pack_conv_fp8(d, L.stream_ptr()))
    return w8, dq, bias


def conv2d_fp8(x, w8, w_dequant, *, x_scale=1.0, in_scale=None, in_shift=None, in_relu=False, bias=None, residual=None, relu=False,
               want_stats=False, amax_out=None, x_scale_dev=None, out=None):
    """fp8 (e4m3) forward conv 3x3 / stride 1 / pad 1: x bf16 NHWC [N,H,W,C], w8 [K,3,3,C] e4m3 bits -> y bf16 NHWC (+ stats).
    x_scale_dev: a device float read instead of x_scale (the form the engine's delayed scaling uses)."""
    _chk(x, w8, w_dequant, in_scale, in_shift, bias, residual, amax_out, x_scale_dev, out)
    assert x.dtype == torch.bfloat16 and w8.dtype == torch.uint8
    N, H, W, C = x.shape
    K = w8.shape[0]
    assert tuple(w8.shape) == (K, 3, 3, C) and w_dequant.dtype == torch.float32 and w_dequant.numel() == K
    assert all(t is None or (t.dtype == torch.float32 and t.numel() == C) for t in (in_scale, in_shift))
    assert bias is None or (bias.dtype == torch.float32 and bias.numel() == K)
    assert residual is None or (residual.dtype == torch.bfloat16 and tuple(residual.shape) == (N, H, W, K))
    assert all(t is None or (t.dtype == torch.float32 and t.numel() >= 1) for t in (amax_out, x_scale_dev))
    y = out if out is not None else torch.empty((N, H, W, K), dtype=torch.bfloat16, device=x.device)
    assert y.dtype == torch.bfloat16 and tuple(y.shape) == (N, H, W, K)
    d = L.ConvDesc(L.ptr(x), None, L.ptr(y), L.ptr(in_scale), L.ptr(in_shift), L.ptr(bias), L.ptr(residual), None,
                   N, H, W, C, K, 3, 3, 1, 1, H, W, H, W, 1, 0, int(in_relu), int(relu), 0, 0, 0, 0, 0)
    q = L.Fp8Desc(L.ptr(w8), L.ptr(w_dequant), float(x_scale), L.ptr(x_scale_dev), L.ptr(amax_out))
    stats = None
    if want_stats:
        rows = L.lib().sslcr_conv2d_fp8_partial_rows(d)
        stats = torch.full((rows, 2, K), float("nan"), dtype=torch.float32, device=x.device)
        d.stats = L.ptr(stats)
    global last_conv_kernel
    last_conv_kernel = L.lib().sslcr_conv2d_fp8_kernel_name(d).decode()
    L.check(L.lib().sslcr_conv2d_fp8(d, q, L.stream_ptr()))
    return (y, stats) if want_stats else y


def fp8_scale_update(slots):
    """delayed scaling: slots [n, 2] fp32 = (x_scale, amax since the last update), updated in place (sslcr_fp8_scale_update)"""
    _chk(slots)
    assert slots.dtype == torch.float32 and slots.dim() == 2 and slots.shape[1] == 2
    L.check(L.lib().sslcr_fp8_scale_update(L.ptr(slots), slots.shape[0], L.stream_ptr()))


def conv2d_wgrad(x, dy, dw, R, S, stride, pad, *, in_scale=None, in_shift=None, in_relu=False, seg_images=0):
    """accumulate dW [K,R,S,C] fp32 += wgrad(x NHWC, dy NHWC).  seg_images > 0: in_scale / in_shift are [N // seg_images, C],
    one producer BatchNorm per segment of seg_images images."""
    _chk(x, dy, dw, in_scale, in_shift)
    N, H, W, C = x.shape
    _, OH, OW, K = dy.shape
    assert dw.shape == (K, R, S, C) and dw.dtype == torch.float32
    d = L.WgradDesc(L.ptr(x), L.ptr(dy), L.ptr(dw), L.ptr(in_scale), L.ptr(in_shift), int(in_relu),
                    N, H, W, C, K, R, S, stride, pad, OH, OW, int(seg_images), C if seg_images else 0)
    global last_wgrad_kernel
    last_wgrad_kernel = L.lib().sslcr_conv2d_wgrad_kernel_name(_dt(x), d).decode()
    L.check(L.lib().sslcr_conv2d_wgrad(_dt(x), d, L.stream_ptr()))


def pack_conv(w_kcrs, dtype, *, fwd=True, dgrad=False, bn=None, eps=1e-5, dgrad_flip=False, unfold=False):
    """PyTorch [K,C,R,S] fp32 -> (w_fwd [K,R,S,C], w_dgrad [C,R,S,K], bias[K]|None) in engine dtype.
    bn = (gamma, beta, running_mean, running_var) folds eval-mode BatchNorm into w_fwd/bias; with unfold the filter stays plain and
    the BatchNorm scale is returned as a fourth value (sslcr_pack_desc.scale_out -> sslcr_conv_desc.out_scale)."""
    _chk(w_kcrs)
    K, C, R, S = w_kcrs.shape
    dev = w_kcrs.device
    wf = torch.empty((K, R, S, C), dtype=tdtype(dtype), device=dev) if fwd else None
    wd = torch.empty((C, R, S, K), dtype=tdtype(dtype), device=dev) if dgrad else None
    bias = torch.empty(K, dtype=torch.float32, device=dev) if bn is not None else None
    g, b, rm, rv = bn if bn is not None else (None, None, None, None)
    scale = torch.empty(K, dtype=torch.float32, device=dev) if (unfold and bn is not None) else None
    d = L.PackDesc(L.ptr(w_kcrs), L.ptr(wf), L.ptr(wd), L.ptr(g), L.ptr(b), L.ptr(rm), L.ptr(rv), eps, L.ptr(bias),
                   K, C, R, S, int(dgrad_flip), L.ptr(scale))
    L.check(L.lib().sslcr_pack_conv(dtype, d, L.stream_ptr()))
    return (wf, wd, bias, scale) if unfold else (wf, wd, bias)


def pack_stem(w_kcrs, dtype, *, bn=None, eps=1e-5, unfold=False):
    _chk(w_kcrs)
    dev = w_kcrs.device
    wf = torch.empty((64, 7, 8, 4), dtype=tdtype(dtype), device=dev)
    bias = torch.empty(64, dtype=torch.float32, device=dev) if bn is not None else None
    g, b, rm, rv = bn if bn is not None else (None, None, None, None)
    scale = torch.empty(64, dtype=torch.float32, device=dev) if (unfold and bn is not None) else None
    d = L.PackDesc(L.ptr(w_kcrs), L.ptr(wf), None, L.ptr(g), L.ptr(b), L.ptr(rm), L.ptr(rv), eps, L.ptr(bias), 64, 3, 7, 7, 0, L.ptr(scale))
    L.check(L.lib().sslcr_pack_stem(dtype, d, L.stream_ptr()))
    return (wf, bias, scale) if unfold else (wf, bias)


def stem_conv(x_nchw, w_packed, *, bias=None, relu=False, want_stats=False, x2=None, out_scale=None):
    """x NCHW uint8|fp32 [N,3,H,W] (optionally followed by a second segment x2, read in place of a torch.cat)
    -> NHWC [N(+N2),OH,OW,64] in w_packed's dtype (+ partial stats)."""
    _chk(x_nchw, w_packed, bias, x2)
    N, _, H, W = x_nchw.shape
    n_split = 0
    if x2 is not None:
        assert x2.dtype == x_nchw.dtype and x2.shape[1:] == x_nchw.shape[1:]
        n_split, N = N, N + x2.shape[0]
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    assert x_nchw.dtype in (torch.uint8, torch.float32)
    y = torch.empty((N, OH, OW, 64), dtype=w_packed.dtype, device=x_nchw.device)
    _chk(out_scale)
    d = L.StemDesc(L.ptr(x_nchw), L.ptr(w_packed), L.ptr(y), L.ptr(bias), None, N, H, W, OH, OW,
                   int(x_nchw.dtype == torch.float32), int(relu), L.ptr(x2), int(n_split), L.ptr(out_scale))
    stats = None
    if want_stats:
        rows = L.lib().sslcr_stem_partial_rows(d)
        stats = torch.full((rows, 2, 64), float("nan"), dtype=torch.float32, device=x_nchw.device)
        d.stats = L.ptr(stats)
    L.check(L.lib().sslcr_stem_conv(_dt(w_packed), d, L.stream_ptr()))
    return (y, stats) if want_stats else y


def stem_conv_pool(x_nchw, w_packed, bias, *, x2=None, out_scale=None):
    """eval-mode stem in one launch: conv1 (folded BatchNorm: bias) -> ReLU -> maxpool 3x3/2 pad 1 -> NHWC [N, OH/2, OW/2, 64] (bf16)."""
    _chk(x_nchw, w_packed, bias, x2)
    N, _, H, W = x_nchw.shape
    n_split = 0
    if x2 is not None:
        n_split, N = N, N + x2.shape[0]
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    POH, POW = OH // 2, OW // 2
    y = torch.empty((N, POH, POW, 64), dtype=w_packed.dtype, device=x_nchw.device)
    _chk(out_scale)
    d = L.StemDesc(L.ptr(x_nchw), L.ptr(w_packed), L.ptr(y), L.ptr(bias), None, N, H, W, OH, OW,
                   int(x_nchw.dtype == torch.float32), 1, L.ptr(x2), int(n_split), L.ptr(out_scale))
    L.check(L.lib().sslcr_stem_conv_pool(_dt(w_packed), d, POH, POW, L.stream_ptr()))
    return y


def stem_wgrad(x_nchw, dy, dw, *, x2=None):
    _chk(x_nchw, dy, dw, x2)
    N, _, H, W = x_nchw.shape
    n_split = 0
    if x2 is not None:
        assert x2.dtype == x_nchw.dtype and x2.shape[1:] == x_nchw.shape[1:]
        n_split, N = N, N + x2.shape[0]
    _, OH, OW, _ = dy.shape
    d = L.StemWgradDesc(L.ptr(x_nchw), L.ptr(dy), L.ptr(dw), N, H, W, OH, OW, int(x_nchw.dtype == torch.float32),
                        L.ptr(x2), int(n_split))
    L.check(L.lib().sslcr_stem_wgrad(_dt(dy), d, L.stream_ptr()))


def stem_wgrad_pool(x_nchw, dw, raw, scale, shift, mean, invstd, pool, *, x2=None, count=None, dgamma=None, dbeta=None):
    """conv1 wgrad straight from the pooled gradient: pool = (pooled_dy, argmax[, pooled y]); raw = conv1's output.  Runs the
    pool-form BatchNorm-backward reduce pass, then the fused apply + wgrad kernel.  -> sums[2,64] fp64"""
    _chk(x_nchw, dw, raw, scale, shift, mean, invstd, x2, dgamma, dbeta)
    N, _, H, W = x_nchw.shape
    n_split = 0
    if x2 is not None:
        n_split, N = N, N + x2.shape[0]
    _, OH, OW, Cn = raw.shape
    pixels = raw.numel() // Cn
    sums = torch.zeros((2, Cn), dtype=torch.float64, device=raw.device)
    pdy, pam = pool[0], pool[1]
    _chk(pdy, pam)
    b = L.BnBwdDesc(None, L.ptr(raw), None, L.ptr(scale), L.ptr(shift), L.ptr(mean), L.ptr(invstd), L.ptr(sums),
                    None, None, pixels, Cn, 1, float(count if count is not None else pixels),
                    L.ptr(pdy), L.ptr(pam), OH, OW, pdy.shape[1], pdy.shape[2], None, 0)
    if len(pool) > 2 and pool[2] is not None:
        _chk(pool[2])
        b.pool_y = L.ptr(pool[2])
    if dgamma is not None:
        b.dgamma, b.dbeta, b.pg_scale = L.ptr(dgamma), L.ptr(dbeta), 1.0
    # the reduce pass of the pool form never touches dx; the C-ABI check wants the pointer for the plain form only
    L.check(L.lib().sslcr_bn_bwd_reduce(_dt(raw), b, L.stream_ptr()))
    w = L.StemWgradDesc(L.ptr(x_nchw), None, L.ptr(dw), N, H, W, OH, OW, int(x_nchw.dtype == torch.float32),
                        L.ptr(x2), int(n_split))
    global last_stem_wgrad_kernel
    last_stem_wgrad_kernel = L.lib().sslcr_stem_wgrad_pool_kernel_name(_dt(raw), w).decode()
    L.check(L.lib().sslcr_stem_wgrad_pool(_dt(raw), w, b, L.stream_ptr()))
    return sums


def bn_finalize(partials, count, gamma, beta, *, running_mean=None, running_var=None, nbt=None, momentum=0.1,
                eps=1e-5, replay=1, nseg=1, one_launch=True):
    """partial rows [rows,2,C] -> (scale, shift, mean, invstd); running stats updated in place `replay` times.
    nseg > 1: the rows are nseg equal segments, the outputs are [nseg, C] (count = elements per channel of one segment)."""
    _chk(partials, gamma, beta, running_mean, running_var, nbt)
    rows, _, Cn = partials.shape
    dev = partials.device
    shape = (nseg, Cn) if nseg > 1 else (Cn,)
    scale, shift, mean, invstd = (torch.empty(shape, dtype=torch.float32, device=dev) for _ in range(4))
    stage = torch.empty((max(nseg, 1), 32, 2, Cn), dtype=torch.float64, device=dev)
    # one_launch: pass ticket words, as the engine does -- the ticketed one-launch form runs where SSLCR_BN_ONE_LAUNCH=1 is set,
    # else the two launches (same bits); False: no ticket words, always the two launches
    tickets = torch.zeros((Cn + 31) // 32, dtype=torch.int32, device=dev) if one_launch else None
    d = L.BnFinalizeDesc(L.ptr(partials), rows, Cn, float(count), L.ptr(gamma), L.ptr(beta), L.ptr(scale), L.ptr(shift),
                         L.ptr(mean), L.ptr(invstd), L.ptr(running_mean), L.ptr(running_var), L.ptr(nbt), momentum, eps,
                         replay, None, None, L.ptr(stage), nseg if nseg > 1 else 0, Cn if nseg > 1 else 0, L.ptr(tickets))
    L.check(L.lib().sslcr_bn_finalize(d, L.stream_ptr()))
    return scale, shift, mean, invstd


def bn_act(x, scale, shift, *, res=None, rscale=None, rshift=None, relu=True, nseg=1, want_bits=False):
    """nseg > 1: x is nseg equal segments along its first dimension, scale / shift (/ rscale / rshift) are [nseg, C].
    want_bits (bf16): -> (y, bits uint8 [numel / 8]), bit (e & 7) of byte e >> 3 = (y.flatten()[e] > 0)  (sslcr_bn_act_desc.ybits)."""
    _chk(x, scale, shift, res, rscale, rshift)
    y = torch.empty_like(x)
    Cn = x.shape[-1]
    d = L.BnActDesc(L.ptr(x), L.ptr(scale), L.ptr(shift), L.ptr(res), L.ptr(rscale), L.ptr(rshift), L.ptr(y),
                    x.numel() // Cn, Cn, int(relu), nseg if nseg > 1 else 0, Cn if nseg > 1 else 0)
    bits = None
    if want_bits:
        if x.dtype != torch.bfloat16:
            raise ValueError("bn_act: the sign mask (sslcr_bn_act_desc.ybits) is written in bf16 only")
        bits = torch.full((x.numel() // 8,), 0xa5, dtype=torch.uint8, device=x.device)
        d.ybits = L.ptr(bits)
    L.check(L.lib().sslcr_bn_act(_dt(x), d, L.stream_ptr()))
    return (y, bits) if want_bits else y


def bn_relu_maxpool(x, scale, shift):
    """maxpool3x3/2 pad 1 of relu(scale * x + shift) -> (y, argmax codes); scale = shift = None: plain max-pool of x -> (y, None)."""
    _chk(x, scale, shift)
    N, H, W, Cn = x.shape
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    y = torch.empty((N, OH, OW, Cn), dtype=x.dtype, device=x.device)
    am = torch.empty((N, OH, OW, Cn), dtype=torch.uint8, device=x.device) if scale is not None else None
    d = L.PoolFwdDesc(L.ptr(x), L.ptr(scale), L.ptr(shift), L.ptr(y), L.ptr(am), N, H, W, Cn, OH, OW)
    L.check(L.lib().sslcr_bn_relu_maxpool(_dt(x), d, L.stream_ptr()))
    return y, am


def maxpool_relu_bwd(dy, argmax, x, scale, shift):
    _chk(dy, argmax, x, scale, shift)
    N, H, W, Cn = x.shape
    _, OH, OW, _ = dy.shape
    dx = torch.empty_like(x)
    d = L.PoolBwdDesc(L.ptr(dy), L.ptr(argmax), L.ptr(x), L.ptr(scale), L.ptr(shift), L.ptr(dx), N, H, W, Cn, OH, OW)
    L.check(L.lib().sslcr_maxpool_relu_bwd(_dt(x), d, L.stream_ptr()))
    return dx


def avgpool_fwd(x):
    _chk(x)
    N, H, W, Cn = x.shape
    y = torch.empty((N, Cn), dtype=torch.float32, device=x.device)
    L.check(L.lib().sslcr_avgpool_fwd(_dt(x), L.ptr(x), L.ptr(y), N, H * W, Cn, L.stream_ptr()))
    return y


def avgpool_bwd(dy, shape, dtype):
    _chk(dy)
    N, H, W, Cn = shape
    dx = torch.empty(shape, dtype=tdtype(dtype), device=dy.device)
    L.check(L.lib().sslcr_avgpool_bwd(dtype, L.ptr(dy), L.ptr(dx), N, H * W, Cn, L.stream_ptr()))
    return dx


def bn_bwd(dy, x, scale, shift, mean, invstd, *, yact=None, relu_from_x=False, want_g=False, count=None, pool=None,
           g_in_reduce=False, nseg=1, dgamma=None, dbeta=None, yact_bits=None, sums=None):
    """-> (dx, sums[2,C] fp64, g|None).  g_in_reduce: the reduce pass writes g and the apply pass reads it (needs yact, want_g).
    sums (fp64 [2, C]): the apply pass alone, from the caller's sums -- for widths sslcr_bn_bwd_reduce does not serve.
    nseg > 1: x is nseg equal segments along its first dimension with constants [nseg, C]; sums come back [nseg, 2, C];
    dgamma / dbeta (fp32 [C], accumulated into) take every segment's contribution."""
    _chk(x, scale, shift, mean, invstd, yact, dgamma, dbeta)
    if dy is not None:
        _chk(dy)
    Cn = x.shape[-1]
    pixels = x.numel() // Cn
    apply_only = sums is not None
    if not apply_only:
        sums = torch.zeros((nseg, 2, Cn) if nseg > 1 else (2, Cn), dtype=torch.float64, device=x.device)
    dx = torch.empty_like(x)
    g = torch.empty_like(x) if want_g else None
    d = L.BnBwdDesc(L.ptr(dy), L.ptr(x), L.ptr(yact), L.ptr(scale), L.ptr(shift), L.ptr(mean), L.ptr(invstd), L.ptr(sums),
                    L.ptr(dx), L.ptr(g), pixels, Cn, int(relu_from_x), float(count if count is not None else pixels // nseg),
                    None, None, 0, 0, 0, 0, None, int(g_in_reduce))
    if dgamma is not None:
        d.dgamma, d.dbeta, d.pg_scale = L.ptr(dgamma), L.ptr(dbeta), 1.0
    if yact_bits is not None:     # the sign mask of yact as sslcr_bn_act wrote it: read instead of yact (which stays in the descriptor)
        _chk(yact_bits)
        d.yact_bits = L.ptr(yact_bits)
    if nseg > 1:
        d.nseg, d.seg_stride, d.sums_stride = nseg, Cn, 2 * Cn
    if pool is not None:          # pool = (pooled_dy [N,OH,OW,C], argmax u8[, pooled output y]): dy arrives through the stem max-pool
        pdy, pam = pool[0], pool[1]
        _chk(pdy, pam)
        d.pool_dy, d.pool_argmax = L.ptr(pdy), L.ptr(pam)
        if len(pool) > 2 and pool[2] is not None:
            _chk(pool[2])
            d.pool_y = L.ptr(pool[2])
        d.pH, d.pW, d.pOH, d.pOW = x.shape[1], x.shape[2], pdy.shape[1], pdy.shape[2]
    if not apply_only:
        L.check(L.lib().sslcr_bn_bwd_reduce(_dt(x), d, L.stream_ptr()))
    L.check(L.lib().sslcr_bn_bwd_apply(_dt(x), d, L.stream_ptr()))
    return dx, sums, g


def bn_param_grads(sums, invstd, dgamma, dbeta):
    _chk(sums, invstd, dgamma, dbeta)
    L.check(L.lib().sslcr_bn_param_grads(L.ptr(sums), L.ptr(invstd), L.ptr(dgamma), L.ptr(dbeta), invstd.numel(),
                                         L.stream_ptr()))


def linear_fwd(x, w, b, relu=False):
    _chk(x, w, b)
    M, K = x.shape
    N = w.shape[0]
    y = torch.empty((M, N), dtype=torch.float32, device=x.device)
    L.check(L.lib().sslcr_linear_fwd(L.ptr(x), L.ptr(w), L.ptr(b), L.ptr(y), M, N, K, int(relu), L.stream_ptr()))
    return y


def linear_bwd(x, w, dy, *, yact=None, dw=None, db=None, want_dx=True, dx=None, dx_accumulate=False):
    _chk(x, w, dy, yact, dw, db, dx)
    M, K = x.shape
    N = w.shape[0]
    if want_dx and dx is None:
        dx = torch.empty((M, K), dtype=torch.float32, device=x.device)
    scratch = torch.empty((M, N), dtype=torch.float32, device=x.device)
    L.check(L.lib().sslcr_linear_bwd(L.ptr(x), L.ptr(w), L.ptr(dy), L.ptr(yact), L.ptr(dx) if want_dx else None,
                                     L.ptr(dw), L.ptr(db), M, N, K, int(dx_accumulate), L.ptr(scratch), L.stream_ptr()))
    return dx


class LossOptions:
    """Options of the cross-entropy losses (include/sslcr.h: sslcr_loss_opts).  Supervised term: ``class_weight`` (a sequence or
    tensor of C floats), ``label_smoothing`` and ``ignore_index`` of ``F.cross_entropy(..., reduction='mean')``.  Consistency term:
    ``threshold`` tau -- FixMatch's confidence mask ``max_probs.ge(tau)`` with ``(loss * mask).mean()`` -- and ``temperature`` T --
    0: hard pseudo labels (the reference), T > 0: UDA's soft targets ``softmax(logits_teacher / T)``.  The defaults are the
    reference's losses, computed in the step functions by the launches the engine has always issued -- which expect every target to
    be a class id: rows labelled -100 are left out, as torch does, once any option is set (and by ``kernels.loss(opts=...)`` always).
    Pure host object; the weight's device copy is made once per device, on first use."""

    def __init__(self, class_weight=None, label_smoothing=0.0, ignore_index=-100, threshold=0.0, temperature=0.0):
        if class_weight is not None:
            class_weight = torch.as_tensor(class_weight).detach().to("cpu", torch.float32).reshape(-1).contiguous()
        self.class_weight = class_weight
        self.label_smoothing, self.ignore_index = float(label_smoothing), int(ignore_index)
        self.threshold, self.temperature = float(threshold), float(temperature)
        if not 0.0 <= self.label_smoothing < 1.0:
            raise ValueError(f"label_smoothing must lie in [0, 1) (got {label_smoothing!r})")
        if not 0.0 <= self.threshold <= 1.0:
            raise ValueError(f"threshold must lie in [0, 1] (got {threshold!r})")
        if not self.temperature >= 0.0:
            raise ValueError(f"temperature must be >= 0 (got {temperature!r})")
        self._dev = {}

    @classmethod
    def from_criterion(cls, criterion, threshold=0.0, temperature=0.0):
        """the options an ``nn.CrossEntropyLoss`` carries (weight, label_smoothing, ignore_index); only reduction='mean' is served"""
        if not isinstance(criterion, torch.nn.CrossEntropyLoss):
            raise TypeError(f"LossOptions.from_criterion: an nn.CrossEntropyLoss expected (got {type(criterion).__name__})")
        if criterion.reduction != "mean":
            raise ValueError(f"LossOptions.from_criterion: reduction={criterion.reduction!r}: only reduction='mean' is served")
        return cls(criterion.weight, getattr(criterion, "label_smoothing", 0.0), criterion.ignore_index, threshold, temperature)

    def is_default(self):
        return self.class_weight is None and self.label_smoothing == 0.0 and self.ignore_index == -100 and self.threshold == 0.0 and \
            self.temperature == 0.0

    def needs_denominator(self):
        """True when a step that holds only PART of the global batch (a micro-batch, a shard) must be handed the batch's divisor:
        for every non-default options object.  With weights or an ignore_index in use 'mean' divides by a data-dependent sum; and
        once any option is set, rows labelled -100 are left out as in torch, so even then the divisor is the kept rows of the
        whole batch, which no part can know from its own rows (without weights and without ignored rows it is the row count, and
        1 / it has the bits of the constant the engine otherwise uses)."""
        return not self.is_default()

    def weight_on(self, device, C=None):
        """the [C] fp32 device copy of class_weight (None without weights)"""
        if self.class_weight is None:
            return None
        if C is not None and self.class_weight.numel() != C:
            raise ValueError(f"class_weight has {self.class_weight.numel()} entries for {C} classes")
        key = str(torch.device(device))
        if key not in self._dev:
            self._dev[key] = self.class_weight.to(device)
        return self._dev[key]

    def c_opts(self, device, C, denominator=None, stats=None):
        """-> (sslcr_loss_opts, the tensors its pointers name: keep them until the launch has run)"""
        w = self.weight_on(device, C)
        o = L.LossOpts(L.ptr(w), self.label_smoothing, self.ignore_index, self.threshold, self.temperature, L.ptr(denominator), L.ptr(stats))
        return o, (w, denominator, stats)

    def __repr__(self):
        w = None if self.class_weight is None else self.class_weight.tolist()
        return (f"LossOptions(class_weight={w}, label_smoothing={self.label_smoothing}, ignore_index={self.ignore_index}, "
                f"threshold={self.threshold}, temperature={self.temperature})")


def ce_denominator(target_i, C, class_weight=None, ignore_index=-100):
    """-> device tensor [sum of class_weight[y] over the rows with y != ignore_index, number of those rows] (sslcr_ce_denominator):
    the divisor of ``F.cross_entropy(weight=, ignore_index=, reduction='mean')``, left on the device.  No sync, no atomics."""
    _chk(target_i, class_weight)
    if target_i.dtype != torch.int64 or target_i.dim() != 1:
        raise L.SslcrError("ce_denominator: a 1-D int64 target tensor expected")
    out2 = torch.empty(2, dtype=torch.float32, device=target_i.device)
    L.check(L.lib().sslcr_ce_denominator(L.ptr(target_i) if target_i.numel() else None, target_i.numel(), int(C), L.ptr(class_weight),
                                         int(ignore_index), L.ptr(out2), L.stream_ptr()))
    return out2


def loss(kind, logits, *, logits_t=None, target_f=None, target_i=None, nx, lambda_u=1.0, want_grad=True,
         nx_global=None, nu_global=None, opts=None, denominator=None, stats=None):
    """opts: a LossOptions (None: sslcr_loss itself); denominator: device [1+] fp32, the supervised term's divisor over the whole
    global batch (``ce_denominator``); stats: device [2] fp32 that receives {#confident rows, sum of max-probs}."""
    _chk(logits, logits_t, target_f, target_i, denominator, stats)
    Ns, Cn = logits.shape
    nu = Ns - nx
    dl = torch.zeros_like(logits) if want_grad else None
    out = torch.zeros(4, dtype=torch.float32, device=logits.device)
    d = L.LossDesc(kind, L.ptr(logits), L.ptr(logits_t), L.ptr(target_f), L.ptr(target_i), L.ptr(dl), L.ptr(out), nx, nu,
                   Cn, lambda_u, 1.0 / (nx_global or nx), 1.0 / max(1, (nu_global or nu)))
    if opts is None and denominator is None and stats is None:
        L.check(L.lib().sslcr_loss(d, L.stream_ptr()))
    else:
        o, keep = (opts if opts is not None else LossOptions()).c_opts(logits.device, Cn, denominator, stats)
        L.check(L.lib().sslcr_loss_ex(d, o, L.stream_ptr()))
    return out, dl


def softmax_col(logits, col=-1):
    """softmax(logits, dim=1)[:, col] for fp32 logits [N, C] (test_Camelyon16.py:58-60)."""
    _chk(logits)
    n, c = logits.shape
    out = torch.empty(n, dtype=torch.float32, device=logits.device)
    L.check(L.lib().sslcr_softmax_col(L.ptr(logits), L.ptr(out), n, c, col % c, L.stream_ptr()))
    return out


def _predict_desc(who, logits, n, c, target, scores, pred, confusion, col, map, map_index):
    """what ``predict`` and ``predict_tta`` share once n and C are known: the rules for target / map_index / confusion / map, the
    output dict, and the sslcr_predict_desc over both -> ``(out, desc)``"""
    dev = logits.device
    for name, t in (("target", target), ("map_index", map_index)):
        if t is not None and (t.dtype != torch.int64 or t.shape != (n,) or t.device != dev):
            raise L.SslcrError(f"{who}: {name} must be an int64 tensor [{n}] on {dev}")
    if confusion is not None:
        if confusion.dtype != torch.int64 or confusion.shape != (c, c) or confusion.device != dev:
            raise L.SslcrError(f"{who}: confusion must be an int64 tensor [{c}, {c}] on {dev}")
        if target is None:
            raise L.SslcrError(f"{who}: confusion needs target")
    if map is not None:
        if map.dtype != torch.float32 or map.device != dev:
            raise L.SslcrError(f"{who}: map must be an fp32 tensor on {dev}")
        if map_index is None:
            raise L.SslcrError(f"{who}: map needs map_index")
        if not -c <= col < c:
            raise L.SslcrError(f"{who}: col = {col} outside [-{c}, {c})")
    out = {}
    if scores:
        out["scores"] = torch.empty((n, c), dtype=torch.float32, device=dev)
    if pred:
        out["pred"] = torch.empty(n, dtype=torch.int64, device=dev)
    d = L.PredictDesc(L.ptr(logits) if n else None, n, c, L.ptr(target), L.ptr(out.get("scores")), L.ptr(out.get("pred")), L.ptr(confusion),
                      col % c, L.ptr(map), L.ptr(map_index), map.numel() if map is not None else 0)
    return out, d


def predict(logits, target=None, *, scores=False, pred=True, confusion=None, col=-1, map=None, map_index=None):
    """What a test() loop takes from a batch of fp32 logits [n, C] (1 <= C <= 64), in one launch (sslcr_predict) -> dict with
    ``scores`` [n, C] fp32 = softmax over the row (scores=True) and ``pred`` [n] int64 = torch.argmax's index (pred=True: the lowest
    index of the row maximum, a NaN is the maximum).  confusion: int64 [C, C] device tensor, ``confusion[target, pred] += 1`` in
    place, across calls (rows with target outside [0, C) are skipped; needs target, int64 [n]).  map: a contiguous fp32 device tensor,
    ``map.view(-1)[map_index[i]] = softmax(logits[i])[col]`` (map_index int64 [n], no duplicates; col may be negative), the value
    bit for bit ``softmax_col``'s.  n = 0 is a no-op.  No sync."""
    _chk(logits, target, confusion, map, map_index)
    if logits.dtype != torch.float32 or logits.dim() != 2:
        raise L.SslcrError("predict: fp32 logits [n, C] expected")
    n, c = logits.shape
    if not 1 <= c <= 64:
        raise L.SslcrError(f"predict: C = {c} outside [1, 64]")
    out, d = _predict_desc("predict", logits, n, c, target, scores, pred, confusion, col, map, map_index)
    L.check(L.lib().sslcr_predict(d, L.stream_ptr()))
    return out


def predict_tta(logits, target=None, *, mode=0, scores=False, pred=True, confusion=None, col=-1, map=None, map_index=None):
    """``predict`` over an ensemble: fp32 logits [G, n, C] (1 <= G <= 8), one launch (sslcr_predict_tta).  mode 0: the fp32
    left-to-right sum of the members' softmax probabilities divided by float32(G); mode 1: the same mean of the raw outputs (a
    regression head; scores only).  ``pred`` is the lowest index of the maximum of the mean (a NaN is the maximum), the confusion
    matrix counts every row ONCE, ``map`` receives the mean's column ``col``.  With G = 1 every output has ``predict``'s bits.  No sync."""
    _chk(logits, target, confusion, map, map_index)
    if logits.dtype != torch.float32 or logits.dim() != 3:
        raise L.SslcrError("predict_tta: fp32 logits [G, n, C] expected")
    G, n, c = logits.shape
    if not 1 <= G <= 8:
        raise L.SslcrError(f"predict_tta: G = {G} outside [1, 8]")
    if not 1 <= c <= 64:
        raise L.SslcrError(f"predict_tta: C = {c} outside [1, 64]")
    if mode not in (0, 1):
        raise L.SslcrError(f"predict_tta: mode = {mode} outside {{0, 1}}")
    if mode == 1 and (pred or confusion is not None or map is not None):
        raise L.SslcrError("predict_tta: mode 1 (raw outputs) has no map, pred or confusion")
    out, p = _predict_desc("predict_tta", logits, n, c, target, scores, pred, confusion, col, map, map_index)
    L.check(L.lib().sslcr_predict_tta(L.PredictTtaDesc(p, G, mode), L.stream_ptr()))
    return out


def d4_transform(x, orient, out=None):
    """``out[n] = d4(x[n], orient[n])`` (sslcr_d4_transform; the codes of ``inference.d4_apply``) for a uint8 or float32 device batch
    [N, Cn, S, S]; orient: device int32 [N].  Out of place: ``out`` must not overlap ``x``.  No sync."""
    _chk(x, orient, out)
    if x.dtype not in (torch.uint8, torch.float32) or x.dim() != 4:
        raise L.SslcrError("d4_transform: a uint8 or float32 batch [N, Cn, S, S] expected")
    n, cn, h, w = x.shape
    if h != w:
        raise L.SslcrError(f"d4_transform: tiles must be square (got {h} x {w})")
    if orient.dtype != torch.int32 or orient.shape != (n,) or orient.device != x.device:
        raise L.SslcrError(f"d4_transform: orient must be an int32 tensor [{n}] on the batch's device")
    out = _out(out, x.shape, x.dtype, x.device, "d4_transform: out must have the batch's dtype, shape and device")
    d = L.D4Desc(L.ptr(x) if n else None, L.ptr(out) if n else None, L.ptr(orient) if n else None, n, cn, h, w, x.element_size())
    L.check(L.lib().sslcr_d4_transform(d, L.stream_ptr()))
    return out


def wsi_gather(region, xy, size, *, origin=(0, 0), fill=0, out=None, orient=None):
    """uint8 tiles [N, 3, size, size] cut from ONE device-resident slide region, uint8 [RH, RW, 3] (sslcr_wsi_gather):
    ``out[n, c, i, j] = region[top - origin[1] + i, left - origin[0] + j, c]`` with (left, top) = xy[n] (device int32 [N, 2], level-0
    coordinates; origin = those of region[0, 0]), ``fill`` where the pixel lies outside the region.  orient: None, or a device int32
    [N] of D4 codes -- tile n is written as ``d4(tile, orient[n])`` (sslcr_wsi_gather_d4; ``inference.d4_apply``).  No sync."""
    _chk(region, xy, out, orient)
    if region.dtype != torch.uint8 or region.dim() != 3 or region.shape[2] != 3:
        raise L.SslcrError("wsi_gather: a uint8 region [RH, RW, 3] expected")
    if xy.dtype != torch.int32 or xy.dim() != 2 or xy.shape[1] != 2 or xy.device != region.device:
        raise L.SslcrError("wsi_gather: xy must be an int32 tensor [N, 2] on the region's device")
    n, size = xy.shape[0], int(size)
    if size < 1 or not 0 <= int(fill) <= 255:
        raise L.SslcrError(f"wsi_gather: size = {size}, fill = {fill}")
    RH, RW = region.shape[0], region.shape[1]
    if RH < 1 or RW < 1 or RH >= 1 << 31 or RW >= 1 << 31:
        raise L.SslcrError(f"wsi_gather: region of {RH} x {RW} pixels")
    out = _out(out, (n, 3, size, size), torch.uint8, region.device,
               f"wsi_gather: out must be a uint8 tensor [{n}, 3, {size}, {size}] on the region's device")
    d = L.WsiGatherDesc(L.ptr(region), L.ptr(xy) if n else None, L.ptr(out) if n else None, int(origin[0]), int(origin[1]), n, RH, RW, size,
                        int(fill))
    if orient is None:
        L.check(L.lib().sslcr_wsi_gather(d, L.stream_ptr()))
        return out
    if orient.dtype != torch.int32 or orient.shape != (n,) or orient.device != region.device:
        raise L.SslcrError(f"wsi_gather: orient must be an int32 tensor [{n}] on the region's device")
    if n:
        L.check(L.lib().sslcr_wsi_gather_d4(d, L.ptr(orient), L.stream_ptr()))
    return out


def _hwc_u8(name, img):
    if img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] != 3:
        raise L.SslcrError(f"{name}: a uint8 image [H, W, 3] expected")
    H, W = img.shape[0], img.shape[1]
    if H < 1 or W < 1 or H >= 1 << 31 or W >= (1 << 31) - 32:
        raise L.SslcrError(f"{name}: image of {H} x {W} pixels")
    return H, W


def _f64_dev(name, what, t, n, dev):
    if t is None or t.dtype != torch.float64 or t.numel() != n or t.device != dev:
        raise L.SslcrError(f"{name}: {what} must be a float64 tensor of {n} element(s) on {dev}")


TISSUE_MODES = L.TISSUE_MODES


def tissue_bits(img, mode, threshold=None, *, lin=None, thr_sum=None, factor=1.0, count=0.0, pitch=None, out=None):
    """The foreground predicate of ``isforeground`` as one bit per pixel of a device uint8 image [H, W, 3] (sslcr_tissue_bits) -> int32
    [H, pitch]: bit ``x & 31`` of dword ``x >> 5`` of row y is pixel (x, y), pad bits zero; pitch >= ceil(W / 32) (the default).
    mode "hsv_s": ``s > threshold`` in float64 (equal to a NumPy restatement); mode "lab_a": ``a* > threshold`` with ``lin``, the 256
    linearised channel values as device float64.  The threshold is the Python float ``threshold``, or -- thr_sum, a device float64 of
    one element -- ``factor * (thr_sum / count)`` read on the device (``lab_a_sum`` wrote it; nothing syncs).  No sync."""
    _chk(img, lin, thr_sum, out)
    H, W = _hwc_u8("tissue_bits", img)
    if mode not in TISSUE_MODES:
        raise L.SslcrError(f"tissue_bits: mode {mode!r} outside {sorted(TISSUE_MODES)}")
    if (threshold is None) == (thr_sum is None):
        raise L.SslcrError("tissue_bits: exactly one of threshold and thr_sum")
    if mode == "lab_a":
        _f64_dev("tissue_bits", "lin", lin, 256, img.device)
    if thr_sum is not None:
        _f64_dev("tissue_bits", "thr_sum", thr_sum, 1, img.device)
        if not float(count) > 0.0:
            raise L.SslcrError(f"tissue_bits: count = {count} with thr_sum")
    words = (W + 31) // 32
    pitch = words if pitch is None else int(pitch)
    if pitch < words:
        raise L.SslcrError(f"tissue_bits: pitch = {pitch} < ceil({W} / 32)")
    out = _out(out, (H, pitch), torch.int32, img.device, f"tissue_bits: out must be an int32 tensor [{H}, {pitch}] on the image's device")
    d = L.TissueBitsDesc(L.ptr(img), L.ptr(out), L.ptr(lin), L.ptr(thr_sum), 0.0 if threshold is None else float(threshold),
                         float(factor), float(count), H, W, pitch, TISSUE_MODES[mode])
    L.check(L.lib().sslcr_tissue_bits(d, L.stream_ptr()))
    return out


def lab_a_sum(img, lin, out=None):
    """-> device float64 [1]: the sum of CIELAB a* over a device uint8 image [H, W, 3] (sslcr_lab_a_sum), ``np.mean(lab[..., 1])``'s
    numerator; lin as for ``tissue_bits``.  Fixed slices and fixed trees: two runs give the same bits.  No sync."""
    _chk(img, lin, out)
    H, W = _hwc_u8("lab_a_sum", img)
    _f64_dev("lab_a_sum", "lin", lin, 256, img.device)
    if out is None:
        out = torch.empty(1, dtype=torch.float64, device=img.device)
    else:
        _f64_dev("lab_a_sum", "out", out, 1, img.device)
    partials = torch.empty(L.LAB_SUM_PARTIALS, dtype=torch.float64, device=img.device)
    d = L.LabASumDesc(L.ptr(img), L.ptr(lin), L.ptr(partials), L.ptr(out), H, W)
    L.check(L.lib().sslcr_lab_a_sum(d, L.stream_ptr()))
    return out


def tile_popcount(bits, width, tile, stride, thresh):
    """The candidate grid of ``get_wsi_patches`` over a bit plane int32 [H, pitch] of an image ``width`` pixels wide
    (sslcr_tile_popcount); tile = (ph, pw), stride = (sh, sw).  -> (count int32 [ny, nx], keep uint8 [ny, nx]) for
    ``ypos in range(sh, H - 1 - ph, sh)``, ``xpos in range(sw, W - 1 - pw, sw)``: the set bits of every window and
    ``count / (ph * pw) >= thresh`` in float64.  An empty grid gives empty tensors.  No sync."""
    _chk(bits)
    if bits.dtype != torch.int32 or bits.dim() != 2:
        raise L.SslcrError("tile_popcount: an int32 bit plane [H, pitch] expected")
    H, pitch = bits.shape
    W = int(width)
    (ph, pw), (sh, sw) = (int(v) for v in tile), (int(v) for v in stride)
    if min(H, W, ph, pw, sh, sw) < 1 or pitch < (W + 31) // 32:
        raise L.SslcrError(f"tile_popcount: H = {H}, W = {W}, pitch = {pitch}, tile = {(ph, pw)}, stride = {(sh, sw)}")
    ny, nx = len(range(sh, H - 1 - ph, sh)), len(range(sw, W - 1 - pw, sw))
    count = torch.empty((ny, nx), dtype=torch.int32, device=bits.device)
    keep = torch.empty((ny, nx), dtype=torch.uint8, device=bits.device)
    if ny and nx:
        d = L.TilePopcountDesc(L.ptr(bits), L.ptr(count), L.ptr(keep), float(thresh), H, W, pitch, ph, pw, sh, sw, ny, nx)
        L.check(L.lib().sslcr_tile_popcount(d, L.stream_ptr()))
    return count, keep


def rsp_gather(levels, xy, idx, size, *, fill=0, out=None):
    """One RSP batch from device-resident pyramid levels (sslcr_rsp_gather, one launch).  levels = (hr, lr1, lr2), uint8 [RH, RW, 3]
    each; xy = three device int32 [T, 2] tables of (left, top) in the pixels of their level; idx: device int64 [N] of sample indices
    into the 6 T samples ``sorted_sequence`` would build (sample k = triplet k // 6 under ordering k % 6).  -> (Data_1, Data_2,
    Data_3, label): uint8 [N, 3, size, size] each and int64 [N] = k % 6; ``fill`` where a tile leaves its level.  out: the four
    tensors to write into.  No sync."""
    if len(levels) != 3 or len(xy) != 3:
        raise L.SslcrError("rsp_gather: three levels and three coordinate tables expected")
    _chk(*levels, *xy, idx, *(out or ()))
    dev = levels[0].device
    hw = [_hwc_u8("rsp_gather", lv) for lv in levels]
    T = xy[0].shape[0] if xy[0].dim() == 2 else -1
    for t in xy:
        if t.dtype != torch.int32 or t.shape != (T, 2) or t.device != dev:
            raise L.SslcrError("rsp_gather: xy must be three int32 tensors [T, 2] on the levels' device")
    if T < 1:
        raise L.SslcrError("rsp_gather: no triplets (T = 0)")
    if any(lv.device != dev for lv in levels) or idx.dtype != torch.int64 or idx.dim() != 1 or idx.device != dev:
        raise L.SslcrError("rsp_gather: idx must be an int64 tensor [N] on the levels' device")
    n, size = idx.shape[0], int(size)
    if size < 1 or not 0 <= int(fill) <= 255:
        raise L.SslcrError(f"rsp_gather: size = {size}, fill = {fill}")
    if out is None:
        out = tuple(torch.empty((n, 3, size, size), dtype=torch.uint8, device=dev) for _ in range(3)) + \
            (torch.empty(n, dtype=torch.int64, device=dev),)
    else:
        if len(out) != 4 or any(o.dtype != torch.uint8 or o.shape != (n, 3, size, size) or o.device != dev for o in out[:3]) or \
                out[3].dtype != torch.int64 or out[3].shape != (n,) or out[3].device != dev:
            raise L.SslcrError(f"rsp_gather: out must be three uint8 tensors [{n}, 3, {size}, {size}] and an int64 tensor [{n}]")
    if n:
        vp3 = L.vp * 3
        d = L.RspGatherDesc(vp3(*(lv.data_ptr() for lv in levels)), vp3(*(t.data_ptr() for t in xy)), L.ptr(idx),
                            vp3(*(o.data_ptr() for o in out[:3])), L.ptr(out[3]), (L.i32 * 3)(*(h for h, _ in hw)),
                            (L.i32 * 3)(*(w for _, w in hw)), T, n, size, int(fill))
        L.check(L.lib().sslcr_rsp_gather(d, L.stream_ptr()))
    return tuple(out)


PIP_CHUNK = L.PIP_CHUNK       # the edges one staged chunk of points_in_polygons holds
PIP_EXACT_MAX = 1 << 24       # the integer path's precondition: integer coordinates of at most this magnitude


def pip_exact_ok(values):
    """the precondition of the integer path, checked on the host: every value an integer of magnitude <= 2^24.  values: a tensor (a
    device tensor costs one sync), a NumPy array, or a sequence of Python ints (a grid's x0, y0 and last coordinates)."""
    if torch.is_tensor(values):
        if values.numel() == 0:
            return True
        return bool(((values == values.round()) & (values.abs() <= PIP_EXACT_MAX)).all().item())
    import numpy as np
    v = np.asarray(values)
    if v.size == 0:
        return True
    if v.dtype == object:                                          # Python ints beyond int64
        return all(isinstance(k, int) and abs(k) <= PIP_EXACT_MAX for k in v.ravel().tolist())
    with np.errstate(invalid="ignore"):
        return bool(np.all((v == np.round(v)) & (np.abs(v) <= PIP_EXACT_MAX)))


def _grid_extremes(grid):
    x0, y0, step, nx, ny = (int(v) for v in grid)
    return [x0, y0, x0 + max(nx - 1, 0) * step, y0 + max(ny - 1, 0) * step]


def points_in_polygons(points, vertices, offsets, *, grid=None, bounds=None, first=False, exact=None, out=None):
    """The crossing-number test of ``Polygon.inside`` for every point against a polygon set (sslcr_points_in_polygons, one launch).
    vertices: device float64 [V, 2] (x, y); offsets: device int32 [P + 1], polygon p = vertices[offsets[p]:offsets[p + 1]]; bounds:
    None (no culling) or device float64 [P, 4] (xmin, ymin, xmax, ymax).  The points are EITHER ``points``, device float64 [N, 2], OR
    (points=None) ``grid=(x0, y0, step, nx, ny)``: point ``i * ny + j`` is ``(x0 + i * step, y0 + j * step)`` in Python ints.
    -> ``inside`` uint8 [N] ([nx, ny] for a grid): 1 where any polygon contains the point; with first=True ``(inside, first)``, first
    int32 of the same shape = the lowest index of a containing polygon, or -1.  A polygon of fewer than 3 vertices contains nothing.
    exact: True / False forces the integer path / the float64 chain; None checks the integer path's precondition on the host
    (``pip_exact_ok`` on vertices and points: integers of magnitude <= 2^24, one sync per device tensor) and takes it where it holds.
    out: ``inside``, or ``(inside, first)``, to write into.  No sync with exact given."""
    if (points is None) == (grid is None):
        raise L.SslcrError("points_in_polygons: exactly one of points and grid")
    _chk(points, vertices, offsets, bounds)
    dev = vertices.device
    if vertices.dtype != torch.float64 or vertices.dim() != 2 or vertices.shape[1] != 2:
        raise L.SslcrError("points_in_polygons: vertices must be a float64 tensor [V, 2]")
    if offsets.dtype != torch.int32 or offsets.dim() != 1 or offsets.numel() < 1 or offsets.device != dev:
        raise L.SslcrError("points_in_polygons: offsets must be an int32 tensor [P + 1] on the vertices' device")
    V, P = vertices.shape[0], offsets.numel() - 1
    if bounds is not None and (bounds.dtype != torch.float64 or bounds.shape != (P, 4) or bounds.device != dev):
        raise L.SslcrError(f"points_in_polygons: bounds must be a float64 tensor [{P}, 4] on the vertices' device")
    if points is not None:
        if points.dtype != torch.float64 or points.dim() != 2 or points.shape[1] != 2 or points.device != dev:
            raise L.SslcrError("points_in_polygons: points must be a float64 tensor [N, 2] on the vertices' device")
        n, shape = points.shape[0], (points.shape[0],)
        x0 = y0 = step = nx = ny = 0
    else:
        x0, y0, step, nx, ny = (int(v) for v in grid)
        if nx < 0 or ny < 0 or step < 0 or nx * ny >= 1 << 31:
            raise L.SslcrError(f"points_in_polygons: grid = {tuple(grid)}")
        n, shape = nx * ny, (nx, ny)
    if exact is None:
        exact = pip_exact_ok(vertices) and pip_exact_ok(points if points is not None else _grid_extremes(grid))
    outs = (out,) if torch.is_tensor(out) else tuple(out or ())
    _chk(*outs)
    if len(outs) > (2 if first else 1):
        raise L.SslcrError("points_in_polygons: out is inside, or (inside, first)")
    inside = outs[0] if outs else torch.empty(shape, dtype=torch.uint8, device=dev)
    which = (outs[1] if len(outs) == 2 else torch.empty(shape, dtype=torch.int32, device=dev)) if first else None
    for name, t, dt in (("inside", inside, torch.uint8), ("first", which, torch.int32)):
        if t is not None and (t.dtype != dt or tuple(t.shape) != shape or t.device != dev):
            raise L.SslcrError(f"points_in_polygons: {name} must be a {dt} tensor {list(shape)} on the vertices' device")
    d = L.PipDesc(L.ptr(vertices) if V else None, L.ptr(offsets), L.ptr(bounds) if P else None,
                  L.ptr(points) if points is not None and n else None, L.ptr(inside) if n else None,
                  L.ptr(which) if which is not None and n else None, x0, y0, step, n, nx, ny, P, V, int(bool(exact)))
    if n:
        L.check(L.lib().sslcr_points_in_polygons(d, L.stream_ptr()))
    return (inside, which) if first else inside


def map_confusion(map, truth, tissue, thresholds):
    """-> device int64 [T, 2, 2]: ``confusion[t, truth, map >= thresholds[t]]`` counted over the cells with ``tissue != 0`` in one pass
    (sslcr_map_confusion).  map: device float32 [X, Y]; truth, tissue: device uint8 (or bool) [X, Y], nonzero = set; thresholds: 1 <= T
    <= 64 float32 values, a device tensor or anything ``torch.as_tensor`` takes.  Integer counts, exact.  No sync."""
    _chk(map, truth, tissue)
    if map.dtype != torch.float32 or map.dim() != 2 or map.numel() < 1:
        raise L.SslcrError("map_confusion: a float32 map [X, Y] expected")
    masks = []
    for name, m in (("truth", truth), ("tissue", tissue)):
        m = _u8(m)
        if m.dtype != torch.uint8 or m.shape != map.shape or m.device != map.device:
            raise L.SslcrError(f"map_confusion: {name} must be a uint8 tensor {list(map.shape)} on the map's device")
        masks.append(m)
    thr = torch.as_tensor(thresholds, dtype=torch.float32).reshape(-1).to(map.device).contiguous()
    T = thr.numel()
    if not 1 <= T <= 64:
        raise L.SslcrError(f"map_confusion: T = {T} outside [1, 64]")
    out = torch.zeros((T, 2, 2), dtype=torch.int64, device=map.device)
    d = L.MapConfusionDesc(L.ptr(map), L.ptr(masks[0]), L.ptr(masks[1]), L.ptr(thr), L.ptr(out), map.shape[0], map.shape[1], T)
    L.check(L.lib().sslcr_map_confusion(d, L.stream_ptr()))
    return out


SMOOTH_MAX_R = L.SMOOTH_MAX_R       # the largest tap radius gaussian_smooth takes
NMS_READ_EVERY = 32                 # rounds of nms between two host reads of the "undecided left" word (tools/froc_bench.py)


def _map2d(name, t, dtype):
    if t.dtype != dtype or t.dim() != 2 or t.numel() < 1 or t.numel() >= 1 << 31:
        raise L.SslcrError(f"{name}: a {dtype} tensor [X, Y] of 1 ... 2^31 - 1 cells expected")


def _mask2d(name, mask):
    """a device mask [X, Y] of 1 ... 2^31 - 1 cells, uint8 or bool -> the mask as uint8"""
    _chk(mask)
    mask = _u8(mask)
    _map2d(name, mask, torch.uint8)
    return mask


def _label_work(n, device):
    """the labeller's scratch for n cells: n parents, and one count per run of ``LABEL_RUN_CELLS`` cells (include/sslcr.h: work)"""
    return torch.empty(n + (n + L.LABEL_RUN_CELLS - 1) // L.LABEL_RUN_CELLS, dtype=torch.int32, device=device)


def label_components(mask, connectivity=2):
    """-> ``(labels, count)``: device int32 [X, Y], 0 where ``mask`` is 0 and else the number of the cell's connected component, and
    device int32 [1] = the number of components L (sslcr_label_components).  mask: device uint8 (or bool) [X, Y]; connectivity 2 = 8
    neighbours, 1 = 4.  Components are numbered 1..L by the order of each component's first cell, as ``scipy.ndimage.label`` does.
    Integer atomics whose order does not reach the result.  No sync."""
    mask = _mask2d("label_components", mask)
    if connectivity not in (1, 2):
        raise L.SslcrError(f"label_components: connectivity = {connectivity} outside {{1, 2}}")
    n = mask.numel()
    labels = torch.empty(mask.shape, dtype=torch.int32, device=mask.device)
    count = torch.empty(1, dtype=torch.int32, device=mask.device)
    work = _label_work(n, mask.device)
    d = L.LabelDesc(L.ptr(mask), L.ptr(labels), L.ptr(count), L.ptr(work), mask.shape[0], mask.shape[1], int(connectivity))
    L.check(L.lib().sslcr_label_components(d, L.stream_ptr()))
    return labels, count


def gaussian_weights(sigma):
    """the 2R + 1 float32 taps of ``gaussian_smooth``: exp(-k^2 / (2 sigma^2)) in float64, normalised to sum 1, cast; R = int(4 sigma + 0.5)"""
    import numpy as np
    R = int(4.0 * float(sigma) + 0.5)
    k = np.arange(-R, R + 1, dtype=np.float64)
    w = np.exp(-(k * k) / (2.0 * float(sigma) * float(sigma)))
    return (w / w.sum()).astype(np.float32)


def gaussian_smooth(map, sigma):
    """-> device float32 [X, Y]: the separable Gaussian of ``map`` in float32, edge mode "nearest", axis 0 then axis 1, every tap one
    product and one sum (sslcr_gaussian_smooth; the taps are ``gaussian_weights(sigma)``).  sigma == 0 returns ``map`` itself without a
    launch.  No sync."""
    _chk(map)
    _map2d("gaussian_smooth", map, torch.float32)
    if not sigma >= 0:
        raise L.SslcrError(f"gaussian_smooth: sigma = {sigma}")
    if sigma == 0:
        return map
    w = gaussian_weights(sigma)
    R = (len(w) - 1) // 2
    if R > SMOOTH_MAX_R:
        raise L.SslcrError(f"gaussian_smooth: R = {R} > {SMOOTH_MAX_R}")
    wd = torch.from_numpy(w).to(map.device)
    tmp, dst = torch.empty_like(map), torch.empty_like(map)
    d = L.SmoothDesc(L.ptr(map), L.ptr(tmp), L.ptr(dst), L.ptr(wd), map.shape[0], map.shape[1], R)
    L.check(L.lib().sslcr_gaussian_smooth(d, L.stream_ptr()))
    return dst


def nms(map, threshold, radius, max_detections=4096, *, read_every=None, stats=None):
    """Greedy non-maximum suppression of a map (include/sslcr.h has the definition) -> ``(det_xy, det_prob, count)``: device int32
    [max_detections, 2], float32 [max_detections] and the number of detections K as a Python int; rows ``[:K]`` are the selected cells
    in the order of the sequential loop.  map: device float32 [X, Y]; a cell is a candidate iff ``map > float32(threshold)``.
    Launches: candidates, then rounds in batches of ``read_every`` (default ``NMS_READ_EVERY``), then collect.  Host reads: the
    candidate count, one "undecided left" word per batch, K.  The rounds are bounded by the candidate count + 1 and ``SslcrError`` is
    raised when they run out; it is raised too when K > max_detections (nothing is written past the capacity).
    stats: a dict that receives ``candidates``, ``rounds`` and ``host_reads``."""
    import numpy as np
    _chk(map)
    _map2d("nms", map, torch.float32)
    radius, cap = int(radius), int(max_detections)
    if radius < 1 or cap < 1:
        raise L.SslcrError(f"nms: radius = {radius}, max_detections = {cap}")
    every = NMS_READ_EVERY if read_every is None else int(read_every)
    if every < 1:
        raise L.SslcrError(f"nms: read_every = {every}")
    dev, n = map.device, map.numel()
    state = torch.empty(map.shape, dtype=torch.uint8, device=dev)
    cand = torch.empty(n, dtype=torch.int32, device=dev)
    stage = torch.empty(cap, dtype=torch.int32, device=dev)
    counters = torch.empty(4, dtype=torch.int32, device=dev)
    det_xy = torch.zeros((cap, 2), dtype=torch.int32, device=dev)
    det_prob = torch.zeros(cap, dtype=torch.float32, device=dev)
    d = L.NmsDesc(L.ptr(map), L.ptr(state), L.ptr(cand), L.ptr(stage), L.ptr(counters), L.ptr(det_xy), L.ptr(det_prob),
                  float(np.float32(threshold)), map.shape[0], map.shape[1], min(radius, max(map.shape)), cap, 0)
    lib, st = L.lib(), L.stream_ptr()
    L.check(lib.sslcr_nms_candidates(d, st))
    d.ncand = ncand = int(counters[0].item())
    rounds, reads, left = 0, 1, ncand
    while left:
        if rounds > ncand:                                         # every round decides at least one candidate: cannot happen
            raise L.SslcrError(f"nms: {left} of {ncand} candidates undecided after {rounds} rounds")
        batch = min(every, ncand + 1 - rounds)
        L.check(lib.sslcr_nms_rounds(d, batch, st))
        rounds += batch
        left = int(counters[1].item())
        reads += 1
    L.check(lib.sslcr_nms_collect(d, st))
    count = int(counters[2].item())
    reads += 1
    if stats is not None:
        stats.update(candidates=ncand, rounds=rounds, host_reads=reads)
    if count > cap:
        raise L.SslcrError(f"nms: {count} detections, max_detections = {cap}")
    return det_xy, det_prob, count


def lesion_hits(labels, n_lesions, det_xy, det_prob, n_det, *, ignore=None, areas=True):
    """The hit test of a detection list against labelled lesions (sslcr_lesion_hits, one launch) -> ``(hit, tp_prob, areas)``:
    ``hit`` int32 [max_detections], rows past the detections 0, = the label under each detection (0: a false positive); ``tp_prob``
    float32 [L] = the best probability among the detections that hit lesion l + 1 and are not on a label in ``ignore``, 0 where there
    is none; ``areas`` int64 [L] = the lesions' cell counts (None with areas=False).  labels: device int32 [X, Y]; n_lesions: L as a
    Python int; det_xy / det_prob: what ``nms`` returns; n_det: a device int32 [1] tensor or a Python int; ignore: labels, any
    sequence.  No sync."""
    _chk(labels, det_xy, det_prob)
    _map2d("lesion_hits", labels, torch.int32)
    dev, cap, nl = labels.device, det_prob.numel(), int(n_lesions)
    if det_xy.dtype != torch.int32 or tuple(det_xy.shape) != (cap, 2) or det_prob.dtype != torch.float32 or cap < 1 or nl < 0:
        raise L.SslcrError("lesion_hits: det_xy int32 [K, 2], det_prob float32 [K] with K >= 1 and n_lesions >= 0 expected")
    if not torch.is_tensor(n_det):
        n_det = torch.tensor([int(n_det)], dtype=torch.int32)
    n_det = n_det.to(dev, torch.int32).reshape(1).contiguous()
    ign = torch.as_tensor(list(ignore) if ignore is not None else [], dtype=torch.int32).reshape(-1).to(dev)
    hit = torch.zeros(cap, dtype=torch.int32, device=dev)
    tp = torch.zeros(nl, dtype=torch.float32, device=dev)
    ar = torch.zeros(nl, dtype=torch.int64, device=dev) if areas else None
    d = L.HitsDesc(L.ptr(labels), L.ptr(det_xy), L.ptr(det_prob), L.ptr(n_det), L.ptr(ign) if ign.numel() else None, L.ptr(hit),
                   L.ptr(tp) if nl else None, L.ptr(ar) if areas and nl else None, labels.shape[0], labels.shape[1], nl, cap, ign.numel())
    L.check(L.lib().sslcr_lesion_hits(d, L.stream_ptr()))
    return hit, tp, ar


EDT_ROW_CELLS = L.EDT_ROW_CELLS     # cells of a row that distance_transform_sq sweeps per chunk (a carry joins the chunks)
EDT_UNLIMITED = (1 << 31) - 1


def _sq_shape(name, t):
    if t.shape[0] ** 2 + t.shape[1] ** 2 >= 1 << 31:
        raise L.SslcrError(f"{name}: X^2 + Y^2 = {t.shape[0] ** 2 + t.shape[1] ** 2} >= 2^31 (a squared distance must fit an int32)")


def distance_limit(T):
    """the smallest integer k >= 0 with ``sqrt(float64(k)) >= T``: for an exact squared distance d2, ``d2 < k`` iff ``sqrt(d2) < T``
    (the float64 square root is monotone).  Host arithmetic; T: a finite float."""
    import math
    T = float(T)
    if not math.isfinite(T):
        raise ValueError(f"distance_limit: T = {T}")
    if T <= 0.0:
        return 0
    k = int(math.ceil(T * T))
    while k > 0 and math.sqrt(float(k - 1)) >= T:   # T * T is rounded: settle the last unit against the definition
        k -= 1
    while math.sqrt(float(k)) < T:
        k += 1
    return k


def distance_transform_sq(mask, limit=None, *, invert=False, below=False):
    """-> device int32 [X, Y]: ``min(limit, the exact squared Euclidean distance to the nearest zero cell of mask)``, 0 on the zero
    cells (sslcr_edt_squared, two launches, integer arithmetic only: two calls give equal bits).  ``limit=None`` is the unlimited
    transform (``EDT_UNLIMITED`` = INT32_MAX); a mask without a zero cell gives ``limit`` everywhere.  ``sqrt`` of the unlimited
    result in float64 is ``scipy.ndimage.distance_transform_edt(mask)``.  mask: device uint8 (or bool) [X, Y], any non-zero value
    set, with X^2 + Y^2 < 2^31.  invert=True measures the distance to the nearest SET cell instead (the zero cells are those with
    mask != 0); below=True returns ``(out, out < limit as uint8)``, written by the same launch.  No sync."""
    mask = _mask2d("distance_transform_sq", mask)
    _sq_shape("distance_transform_sq", mask)
    limit = EDT_UNLIMITED if limit is None else int(limit)
    if not 0 <= limit <= EDT_UNLIMITED:
        raise L.SslcrError(f"distance_transform_sq: limit = {limit} outside [0, 2^31 - 1]")
    out = torch.empty(mask.shape, dtype=torch.int32, device=mask.device)
    work = torch.empty(mask.shape, dtype=torch.int32, device=mask.device)
    under = torch.empty(mask.shape, dtype=torch.uint8, device=mask.device) if below else None
    d = L.EdtDesc(L.ptr(mask), L.ptr(out), L.ptr(under), L.ptr(work), mask.shape[0], mask.shape[1], limit, 1 if invert else 0)
    L.check(L.lib().sslcr_edt_squared(d, L.stream_ptr()))
    return (out, under) if below else out


def fill_holes(mask):
    """-> device uint8 [X, Y] of 0 / 1: ``mask != 0``, or a background cell whose connectivity-1 background component touches no cell
    of the array's border -- ``scipy.ndimage.binary_fill_holes`` (sslcr_fill_holes: the complement, ``label_components`` on it, a
    border pass, the apply pass; no host read in between).  mask: device uint8 (or bool) [X, Y].  No sync."""
    mask = _mask2d("fill_holes", mask)
    n, dev = mask.numel(), mask.device
    out = torch.empty(mask.shape, dtype=torch.uint8, device=dev)
    labels = torch.empty(n, dtype=torch.int32, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    work = _label_work(n, dev)
    d = L.FillDesc(L.ptr(mask), L.ptr(out), L.ptr(labels), L.ptr(count), L.ptr(work), mask.shape[0], mask.shape[1])
    L.check(L.lib().sslcr_fill_holes(d, L.stream_ptr()))
    return out


def region_moments(labels, n):
    """-> device int64 [n, 6]: for label l + 1, over its cells (x, y): area, sum x, sum y, sum x^2, sum y^2, sum x y
    (sslcr_region_moments, one launch; integer atomics, exact, and below 2^62 under the shape bound X^2 + Y^2 < 2^31).  labels: device
    int32 [X, Y] as ``label_components`` returns; n: the number of labels as a Python int (0: no launch).  No sync."""
    _chk(labels)
    _map2d("region_moments", labels, torch.int32)
    _sq_shape("region_moments", labels)
    n = int(n)
    if n < 0:
        raise L.SslcrError(f"region_moments: n = {n}")
    out = torch.zeros((n, 6), dtype=torch.int64, device=labels.device)
    d = L.MomentsDesc(L.ptr(labels), L.ptr(out) if n else None, labels.shape[0], labels.shape[1], n)
    L.check(L.lib().sslcr_region_moments(d, L.stream_ptr()))
    return out


SORT_TILE = L.SORT_TILE             # keys one workgroup handles per radix pass; also the elements of one auc_counts block
RANK_SCAN_TRIP = L.RANK_SCAN_TRIP   # tiles (sort_pairs) / blocks (auc_counts) one trip of the partial scan covers; a carry joins the trips


def _rows_u32(name, t):
    if not t.is_cuda or t.dim() not in (1, 2) or t.numel() < 1 or t.dtype not in (torch.uint32, torch.int32):
        raise L.SslcrError(f"{name}: a non-empty device uint32 (or int32, read as uint32) tensor [n] or [B, n] expected (no CPU fallback)")
    if (t.shape[0] if t.dim() == 2 else 1) > 65535 or t.shape[-1] >= 1 << 31:
        raise L.SslcrError(f"{name}: at most 65535 rows of fewer than 2^31 keys")
    return t.contiguous()


def sort_workspace(B, n, device):
    """the scratch ``sort_pairs`` needs for B rows of n keys (sslcr_sort_workspace_bytes), as a device int32 tensor"""
    return torch.empty(L.lib().sslcr_sort_workspace_bytes(int(B), int(n)) // 4, dtype=torch.int32, device=device)


def sort_pairs(keys, values=None, *, bits=(0, 32), workspace=None):
    """-> ``(keys, values)`` sorted ascending by the bits ``[lo, hi)`` of the keys, every row on its own: a stable LSD radix sort
    (sslcr_sort_pairs; 3 launches per 8-bit digit, the row in the grid).  keys: device uint32 [n] or [B, n] (int32 is read as its
    bits); values: the same shape, uint32 / int32, or None = the index within the row (the stable ``argsort``).  Keys equal in the bit
    range keep their input order; two calls give equal bits.  The inputs are left as they were (the sort works on a copy and a second
    buffer); workspace: ``sort_workspace(B, n, device)`` to reuse across calls.  Results come back as uint32.  No sync."""
    keys = _rows_u32("sort_pairs", keys)
    shape = keys.shape
    B, n = (shape[0], shape[1]) if keys.dim() == 2 else (1, shape[0])
    lo, hi = int(bits[0]), int(bits[1])
    if not 0 <= lo <= hi <= 32:
        raise L.SslcrError(f"sort_pairs: bits = ({lo}, {hi}) outside 0 <= lo <= hi <= 32")
    dev = keys.device
    if values is None:
        vals = torch.arange(n, dtype=torch.int32, device=dev).repeat(B)
    else:
        values = _rows_u32("sort_pairs", values)
        if values.shape != shape or values.device != dev:
            raise L.SslcrError(f"sort_pairs: values {list(values.shape)} must match keys {list(shape)} on one device")
        vals = values.clone()
    k = [keys.clone().view(torch.int32).reshape(-1), None]
    v = [vals.view(torch.int32).reshape(-1), None]
    k[1], v[1] = torch.empty_like(k[0]), torch.empty_like(v[0])
    if workspace is None:
        workspace = sort_workspace(B, n, dev)
    if workspace.device != dev or workspace.numel() * workspace.element_size() < L.lib().sslcr_sort_workspace_bytes(B, n):
        raise L.SslcrError("sort_pairs: workspace too small or on another device (sort_workspace(B, n, device))")
    d = L.SortDesc((L.vp * 2)(k[0].data_ptr(), k[1].data_ptr()), (L.vp * 2)(v[0].data_ptr(), v[1].data_ptr()), L.ptr(workspace), B, n, lo, hi)
    L.check(L.lib().sslcr_sort_pairs(d, L.stream_ptr()))
    at = ((hi - lo + 7) // 8) & 1
    return k[at].view(torch.uint32).reshape(shape), v[at].view(torch.uint32).reshape(shape)


def rank_keys(scores, target, *, positive=None, valid=None):
    """-> ``(keys, values, nan)``: device uint32 [C, n], uint32 [C, n], int64 [C] (sslcr_rank_keys, one launch).  scores: device float32
    [n, C] or [n] (C = 1); target: device integer [n]; positive: the class column c scores, C integers (None = ``arange(C)``); valid:
    device uint8 / bool [n], zero = leave the element out (None = all in).  ``keys[c]`` orders as ``scores[:, c]`` does under float
    compares (-0 ties with +0); ``values[c]`` is 1 where ``target == positive[c]``, else 0, and 2 on an element left out or NaN;
    ``nan[c]`` counts the NaN scores among the valid elements.  No sync."""
    _chk(scores, target)
    if scores.dtype != torch.float32 or scores.dim() not in (1, 2) or scores.numel() < 1:
        raise L.SslcrError("rank_keys: non-empty float32 scores [n] or [n, C] expected")
    scores = scores.contiguous()
    n, Cn = scores.shape[0], (scores.shape[1] if scores.dim() == 2 else 1)
    dev = scores.device
    if target.is_floating_point() or target.numel() != n or target.device != dev:
        raise L.SslcrError(f"rank_keys: {n} integer targets on the scores' device expected")
    target = target.reshape(-1).to(torch.int64).contiguous()
    if not 1 <= Cn <= 65535 or n >= 1 << 31:
        raise L.SslcrError(f"rank_keys: C = {Cn} outside [1, 65535] or n = {n} >= 2^31")
    if positive is not None:
        positive = torch.as_tensor(positive, dtype=torch.int64).reshape(-1).to(dev).contiguous()
        if positive.numel() != Cn:
            raise L.SslcrError(f"rank_keys: {positive.numel()} positive classes for {Cn} columns")
    if valid is not None:
        _chk(valid)
        valid = _u8(valid)
        if valid.dtype != torch.uint8 or valid.numel() != n or valid.device != dev:
            raise L.SslcrError(f"rank_keys: valid must be {n} uint8 / bool flags on the scores' device")
        valid = valid.reshape(-1).contiguous()
    keys = torch.empty((Cn, n), dtype=torch.int32, device=dev)
    values = torch.empty((Cn, n), dtype=torch.int32, device=dev)
    nan = torch.empty(Cn, dtype=torch.int64, device=dev)
    d = L.RankKeysDesc(L.ptr(scores), L.ptr(target), L.ptr(valid), L.ptr(positive), L.ptr(keys), L.ptr(values), L.ptr(nan), n, Cn)
    L.check(L.lib().sslcr_rank_keys(d, L.stream_ptr()))
    return keys.view(torch.uint32), values.view(torch.uint32), nan


def auc_counts(scores, target, *, positive=None, valid=None):
    """-> device int64 [C, 4] = ``(U2, P, N, nan)`` per column: P / N the valid positives / negatives, ``U2 = sum over positives i and
    negatives j of 2 [s_i > s_j] + [s_i == s_j]`` exactly, so the column's ROC-AUC is ``U2 / (2 P N)``; nan = the valid elements with a
    NaN score, which are in none of the other three.  ``rank_keys``, ``sort_pairs`` of the C rows in one call, then sslcr_auc_counts
    (block partials, one scan, one apply pass); integer arithmetic throughout, two calls give equal bits.  Arguments as ``rank_keys``.
    No sync."""
    keys, values, nan = rank_keys(scores, target, positive=positive, valid=valid)
    Cn, n = keys.shape
    # the sort's second buffers and result: rank_keys' own outputs are the first buffers, nothing is cloned
    k = [keys.view(torch.int32), torch.empty((Cn, n), dtype=torch.int32, device=keys.device)]
    v = [values.view(torch.int32), torch.empty((Cn, n), dtype=torch.int32, device=keys.device)]
    ws = sort_workspace(Cn, n, keys.device)
    d = L.SortDesc((L.vp * 2)(k[0].data_ptr(), k[1].data_ptr()), (L.vp * 2)(v[0].data_ptr(), v[1].data_ptr()), L.ptr(ws), Cn, n, 0, 32)
    L.check(L.lib().sslcr_sort_pairs(d, L.stream_ptr()))      # 4 passes: the result is back in the first buffers
    counts = torch.empty((Cn, 4), dtype=torch.int64, device=keys.device)
    work = torch.empty(L.lib().sslcr_auc_workspace_bytes(Cn, n) // 4, dtype=torch.int32, device=keys.device)
    a = L.AucDesc(L.ptr(k[0]), L.ptr(v[0]), L.ptr(nan), L.ptr(counts), L.ptr(work), n, Cn)
    L.check(L.lib().sslcr_auc_counts(a, L.stream_ptr()))
    return counts


# ---- k-nearest-neighbour feature probe (csrc/knn.hip)
KNN_TILE, KNN_CHUNK, KNN_MAX_K, KNN_MAX_D = L.KNN_TILE, L.KNN_CHUNK, L.KNN_MAX_K, L.KNN_MAX_D
KNN_FORMS = L.KNN_FORMS
KNN_VOTES = L.KNN_VOTES


def knn_plan(nq, nb, dim, k, slices=None):
    """what ``knn_topk`` launches for these sizes (sslcr_knn_plan; host only, no device needed): dict with ``form`` ("direct" |
    "sliced"), ``tile_q``, ``tile_b``, ``chunk``, ``slices``, ``tiles_per_slice``, ``grid`` (workgroups of the two launches),
    ``lds_bytes`` and ``workspace_bytes``.  slices: the hint (None / 0 = the plan's choice)."""
    p = L.KnnPlan()
    L.check(L.lib().sslcr_knn_plan(int(nq), int(nb), int(dim), int(k), int(slices or 0), p))
    out = {f: getattr(p, f) for f, _ in L.KnnPlan._fields_}
    out["grid"] = tuple(p.grid)
    out["form"] = KNN_FORMS[p.form]
    return out


def _f32_rows(name, t):
    if not t.is_cuda:
        raise L.SslcrError(f"{name}: device tensors expected (no CPU fallback)")
    if t.dtype != torch.float32 or t.dim() != 2:
        raise L.SslcrError(f"{name}: float32 [n, D] expected, got {t.dtype} {list(t.shape)}")
    return t.contiguous()


def knn_topk(queries, bank, k, *, nb_valid=None, exclude_self=None, slices=None, out=None):
    """-> ``(scores, indices)``: device float32 [nq, k] and int32 [nq, k], per query the k bank rows with the greatest dot product,
    best first (sslcr_knn_topk: a fused fp32 MFMA similarity and top-k, the [nq, nb] product never reaches memory; two launches).
    queries [nq, D], bank [nb, D]: device float32, D % 4 == 0, 4 <= D <= 2048; 1 <= k <= 64.  Every score is an fp32 fma chain over
    D in rising order, whatever the plan: ``slices`` (the bank slices of the grid; None = the plan's choice) changes no bit.  The
    order is total: the greater score first, of equal scores (-0 == +0) the lower bank index; a NaN score ranks below every number.
    nb_valid: search rows ``[0, nb_valid)`` only; exclude_self: an offset o >= 0 (True = 0) making query i ignore bank row i + o, for
    leave-one-out when the queries are rows of the bank.  With fewer than k admissible rows the trailing slots are index -1 and score
    -inf.  out: ``(scores, indices)`` to write into.  No sync."""
    queries, bank = _f32_rows("knn_topk", queries), _f32_rows("knn_topk", bank)
    (nq, D), nb = queries.shape, bank.shape[0]
    if bank.shape[1] != D or bank.device != queries.device:
        raise L.SslcrError(f"knn_topk: queries {list(queries.shape)} and bank {list(bank.shape)} must share D and the device")
    nb_valid = nb if nb_valid is None else int(nb_valid)
    if not 0 <= nb_valid <= nb:
        raise L.SslcrError(f"knn_topk: nb_valid = {nb_valid} outside [0, {nb}]")
    if 1 <= nb_valid < nb:                           # the prefix IS the bank: the plan and its slices are sized for the rows searched
        bank, nb = bank[:nb_valid], nb_valid
    if exclude_self is None or exclude_self is False:
        off = -1
    else:
        off = 0 if exclude_self is True else int(exclude_self)
        if off < 0:
            raise L.SslcrError("knn_topk: exclude_self must be an offset >= 0 (or True = 0)")
    p = L.KnnPlan()
    L.check(L.lib().sslcr_knn_plan(nq, nb, D, int(k), int(slices or 0), p))
    dev = queries.device
    scores = _out(out[0] if out else None, (nq, k), torch.float32, dev, f"knn_topk: out[0] must be float32 [{nq}, {k}] on the queries' device")
    indices = _out(out[1] if out else None, (nq, k), torch.int32, dev, f"knn_topk: out[1] must be int32 [{nq}, {k}] on the queries' device")
    _chk(scores, indices)
    ws = torch.empty(max(1, p.workspace_bytes // 8), dtype=torch.int64, device=dev)
    d = L.KnnDesc(L.ptr(queries), L.ptr(bank), L.ptr(scores), L.ptr(indices), L.ptr(ws), nq, nb, D, int(k), nb_valid, off, int(slices or 0))
    L.check(L.lib().sslcr_knn_topk(d, L.stream_ptr()))
    return scores, indices


def l2_normalize(x, eps=1e-12, out=None):
    """-> ``x / max(||x||, eps)`` per row of a device float32 [n, D] (sslcr_l2_normalize, one wave per row):
    ``torch.nn.functional.normalize(x, dim=1)`` with the norm summed in float64 in a fixed order, rounded to float32 once, and one
    correctly rounded float32 division per element.  out may be x.  No sync."""
    x = _f32_rows("l2_normalize", x)
    y = _out(out, x.shape, torch.float32, x.device, "l2_normalize: out must match x")
    _chk(y)
    L.check(L.lib().sslcr_l2_normalize(L.ptr(x), L.ptr(y), x.shape[0], x.shape[1], float(eps), L.stream_ptr()))
    return y


def knn_vote(indices, scores, labels=None, targets=None, *, n_classes=None, weights="uniform", temperature=0.07, query_labels=None,
             confusion=None):
    """What a k-NN classifier or regressor makes of ``knn_topk``'s output (sslcr_knn_vote, one launch, no sync).  indices / scores:
    device int32 / float32 [nq, k].  Classification (``labels``: device integer [nb] bank labels, ``n_classes`` <= 64): -> dict with
    ``pred`` int64 [nq], ``votes`` float32 [nq, C] and, with ``query_labels`` (device integer [nq]), ``confusion`` int64 [C, C] (rows =
    query labels; pass ``confusion=`` to accumulate into an existing matrix).  weights "uniform": integer counts, the most votes win, a
    tie goes to the lowest class (sklearn's ``KNeighborsClassifier``); "softmax": ``expf((s - s_0) / temperature)`` summed per class in
    rank order (the DINO / InstDisc weighted vote).  Regression (``targets``: device float32 [nb]): -> dict with ``pred`` float32 [nq],
    the float32 mean of the neighbours' targets summed in rank order.  A slot with index -1 takes no part."""
    _chk(indices, scores, labels, targets, query_labels, confusion)
    if indices.dtype != torch.int32 or indices.dim() != 2:
        raise L.SslcrError("knn_vote: int32 indices [nq, k] expected")
    nq, k = indices.shape
    dev = indices.device
    if (labels is None) == (targets is None):
        raise L.SslcrError("knn_vote: exactly one of labels (classification) and targets (regression) expected")
    if scores is not None and (scores.dtype != torch.float32 or scores.shape != indices.shape or scores.device != dev):
        raise L.SslcrError("knn_vote: scores must be float32 of the indices' shape and device")
    if targets is not None:
        if targets.dtype != torch.float32 or targets.dim() != 1 or targets.device != dev:
            raise L.SslcrError("knn_vote: float32 targets [nb] on the indices' device expected")
        pred = torch.empty(nq, dtype=torch.float32, device=dev)
        d = L.KnnVoteDesc(L.ptr(indices), L.ptr(scores), None, L.ptr(targets), None, None, L.ptr(pred), None, None, nq, k, targets.numel(), 1,
                          L.KNN_VOTES["regress"], 0.0)
        L.check(L.lib().sslcr_knn_vote(d, L.stream_ptr()))
        return dict(pred=pred)
    if weights not in ("uniform", "softmax"):
        raise L.SslcrError(f"knn_vote: weights = {weights!r} outside ('uniform', 'softmax')")
    if labels.is_floating_point() or labels.dim() != 1 or labels.device != dev:
        raise L.SslcrError("knn_vote: integer labels [nb] on the indices' device expected")
    if n_classes is None:
        raise L.SslcrError("knn_vote: n_classes expected (reading it off the labels would synchronise)")
    Cn = int(n_classes)
    labels = labels.to(torch.int64).contiguous()
    if weights == "softmax" and scores is None:
        raise L.SslcrError("knn_vote: the softmax vote needs scores")
    if query_labels is not None:
        if query_labels.is_floating_point() or query_labels.numel() != nq or query_labels.device != dev:
            raise L.SslcrError(f"knn_vote: {nq} integer query_labels on the indices' device expected")
        query_labels = query_labels.reshape(-1).to(torch.int64).contiguous()
        if confusion is None and 1 <= Cn <= 64:
            confusion = torch.zeros((Cn, Cn), dtype=torch.int64, device=dev)
        elif confusion is not None and (confusion.dtype != torch.int64 or tuple(confusion.shape) != (Cn, Cn) or confusion.device != dev):
            raise L.SslcrError(f"knn_vote: confusion must be int64 [{Cn}, {Cn}] on the indices' device")
    elif confusion is not None:
        raise L.SslcrError("knn_vote: confusion needs query_labels")
    pred = torch.empty(nq, dtype=torch.int64, device=dev)
    votes = torch.empty((nq, max(Cn, 0)), dtype=torch.float32, device=dev)
    d = L.KnnVoteDesc(L.ptr(indices), L.ptr(scores), L.ptr(labels), None, L.ptr(query_labels), L.ptr(pred), None, L.ptr(votes), L.ptr(confusion),
                      nq, k, labels.numel(), Cn, L.KNN_VOTES[weights], float(temperature))
    L.check(L.lib().sslcr_knn_vote(d, L.stream_ptr()))
    out = dict(pred=pred, votes=votes)
    if confusion is not None:
        out["confusion"] = confusion
    return out


# ---- t-SNE embedding (csrc/tsne.hip)
TSNE_TILE, TSNE_CHUNK, TSNE_MAX_SLICES, TSNE_MAX_N, TSNE_LOG_COLS = L.TSNE_TILE, L.TSNE_CHUNK, L.TSNE_MAX_SLICES, L.TSNE_MAX_N, L.TSNE_LOG_COLS


def tsne_plan(n, slices=None):
    """what the t-SNE gradient launches for n points (sslcr_tsne_plan; host only, no device needed): dict with ``tile`` (rows of a
    repulsion workgroup), ``chunk`` (points per LDS stage), ``slices`` (column slices S), ``chunks_per_slice``, ``grid`` (workgroups
    of the repulsion, the Z fold and the update), ``lds_bytes`` and ``workspace_bytes``.  slices: the hint (None / 0 = the plan's)."""
    p = L.TsnePlan()
    L.check(L.lib().sslcr_tsne_plan(int(n), int(slices or 0), p))
    out = {f: getattr(p, f) for f, _ in L.TsnePlan._fields_}
    out["grid"] = tuple(p.grid)
    return out


def euclidean_topk(x, k, *, slices=None):
    """-> ``(indices, dist2)``: device int32 [n, k] and float32 [n, k], per row of x (device float32 [n, D], D <= 2044) its k nearest
    OTHER rows by squared Euclidean distance, nearest first.  The search is ``knn_topk`` unchanged, on the query rows ``[x, 1, 0..]``
    against the bank rows ``[x, -|x|^2 / 2, 0..]`` (the width padded to a multiple of 4; the norm summed in float64, rounded once) with
    ``exclude_self``: the greatest dot product is the least distance, and the order is ``knn_topk``'s total order.  The distances are
    then recomputed directly (sslcr_tsne_pair_dist2: float64 sum over rising d, rounded to float32 once).  With fewer than k other
    rows the trailing slots are index -1 and distance +inf.  Centre x first where its mean is far from 0.  No sync."""
    x = _f32_rows("euclidean_topk", x)
    n, D = x.shape
    W = (D + 1 + 3) // 4 * 4
    if not 2 <= n <= TSNE_MAX_N or W > KNN_MAX_D:
        raise L.SslcrError(f"euclidean_topk: n = {n} outside [2, 2^20] or D = {D} above {KNN_MAX_D - 4}")
    q = torch.zeros((n, W), dtype=torch.float32, device=x.device)
    q[:, :D] = x
    b = q.clone()
    q[:, D] = 1.0
    b[:, D] = (-0.5 * x.double().square().sum(1)).float()
    _, indices = knn_topk(q, b, k, exclude_self=True, slices=slices)
    dist2 = torch.empty((n, k), dtype=torch.float32, device=x.device)
    L.check(L.lib().sslcr_tsne_pair_dist2(L.ptr(x), L.ptr(indices), L.ptr(dist2), n, D, int(k), L.stream_ptr()))
    return indices, dist2


def tsne_affinities(dist2, perplexity):
    """-> ``(P, beta)``: device float32 [n, k] and float64 [n]: sklearn's ``_binary_search_perplexity`` on float32 squared distances
    [n, k], k <= 64 (sslcr_tsne_affinities, one wave per row): the conditional p_{j|i} at the beta whose entropy is log(perplexity)
    to 1e-5, found in at most 100 steps from beta = 1.  No sync."""
    dist2 = _f32_rows("tsne_affinities", dist2)
    n, k = dist2.shape
    if not 1 <= k <= KNN_MAX_K or not 2 <= n <= TSNE_MAX_N or not float(perplexity) > 0:
        raise L.SslcrError(f"tsne_affinities: k = {k} outside [1, 64], n = {n} outside [2, 2^20] or perplexity = {perplexity} not > 0")
    P = torch.empty_like(dist2)
    beta = torch.empty(n, dtype=torch.float64, device=dist2.device)
    L.check(L.lib().sslcr_tsne_affinities(L.ptr(dist2), L.ptr(P), L.ptr(beta), n, k, float(perplexity), L.stream_ptr()))
    return P, beta


def tsne_joint(indices, P):
    """-> ``(rowptr, col, val)``: the symmetric joint affinities p_ij = (p_{j|i} + p_{i|j}) / (2 n) as CSR: device int32 [n + 1], int32
    [2 n k] and float32 [2 n k], columns rising within a row.  ``col`` / ``val`` have the CAPACITY 2 n k; the first ``rowptr[n]`` entries
    are the matrix (reading that count is the caller's copy; nothing here synchronises).  The 2 n k directed entries are sorted by
    two stable ``sort_pairs`` passes (column, then row); adjacent equal pairs are merged -- at most two meet, their float64 sum is
    exact -- divided by 2 n in float64 and rounded to float32.  Two calls return equal bits.  A slot with index -1 takes no part."""
    _chk(indices, P)
    if indices.dtype != torch.int32 or indices.dim() != 2 or P.dtype != torch.float32 or P.shape != indices.shape or P.device != indices.device:
        raise L.SslcrError("tsne_joint: int32 indices [n, k] and float32 P [n, k] on one device expected")
    n, k = indices.shape
    if not 2 <= n <= TSNE_MAX_N:
        raise L.SslcrError(f"tsne_joint: n = {n} outside [2, 2^20]")
    dev = indices.device
    i = torch.arange(n, dtype=torch.int32, device=dev).repeat_interleave(k)
    j = indices.reshape(-1)
    # an empty slot (-1) sorts past every row as the pair (n, n) and is dropped by the row count below
    miss = j < 0
    full = torch.full_like(j, n)
    r = torch.cat([torch.where(miss, full, i), torch.where(miss, full, j)])
    c = torch.cat([torch.where(miss, full, j), torch.where(miss, full, i)])
    v = torch.cat([P.reshape(-1), P.reshape(-1)]).double()
    bits = (0, max(1, int(n).bit_length()))
    c1, o1 = (t.view(torch.int32).long() for t in sort_pairs(c, bits=bits))             # by column ...
    r2, o2 = (t.view(torch.int32).long() for t in sort_pairs(r[o1], bits=bits))         # ... then, stably, by row
    c2, v2 = c1[o2], v[o1[o2]]
    first = torch.ones_like(r2, dtype=torch.bool)
    first[1:] = (r2[1:] != r2[:-1]) | (c2[1:] != c2[:-1])
    seg = torch.cumsum(first, 0) - 1
    M = r2.numel()
    val = torch.zeros(M, dtype=torch.float64, device=dev).index_add_(0, seg, v2)        # at most two addends a cell: exact, any order
    col = torch.zeros(M, dtype=torch.int32, device=dev).scatter_(0, seg, c2.int())      # equal values where two meet
    counts = torch.zeros(n + 2, dtype=torch.int64, device=dev).index_add_(0, r2 + 1, first.long())
    rowptr = torch.cumsum(counts[:n + 1], 0).int()
    return rowptr, col, (val / (2.0 * n)).float()


def _tsne_P(name, P, n, dev):
    rowptr, col, val = P
    _chk(rowptr, col, val)
    if (rowptr.dtype != torch.int32 or rowptr.numel() != n + 1 or col.dtype != torch.int32 or val.dtype != torch.float32 or col.numel() != val.numel()
            or any(t.device != dev for t in P)):
        raise L.SslcrError(f"{name}: P = (rowptr int32 [{n + 1}], col int32 [nnz], val float32 [nnz]) on y's device expected")
    return rowptr, col, val


def _tsne_y(name, y):
    if not y.is_cuda or y.dtype != torch.float32 or y.dim() != 2 or y.shape[1] != 2 or not y.is_contiguous():
        raise L.SslcrError(f"{name}: contiguous device float32 [n, 2] expected (no CPU fallback)")
    if not 2 <= y.shape[0] <= TSNE_MAX_N:
        raise L.SslcrError(f"{name}: n = {y.shape[0]} outside [2, 2^20]")
    return y.shape[0]


def tsne_workspace(n, device, slices=None):
    """the scratch a t-SNE gradient needs (``tsne_plan(n, slices)["workspace_bytes"]`` and the float64 Z): dict of device tensors"""
    p = tsne_plan(n, slices)
    return dict(ws=torch.empty(max(1, p["workspace_bytes"] // 4), dtype=torch.float32, device=device),
                Z=torch.empty(1, dtype=torch.float64, device=device), slices=int(slices or 0))


def tsne_gradient(y, P, exaggeration=1.0, *, slices=None, workspace=None, kl_rows=None):
    """-> ``(grad, Z)``: device float32 [n, 2] and float64 [1]: sklearn's exact ``_kl_divergence`` gradient
    4 (exaggeration sum_j p_ij q_ij (y_i - y_j) - (1 / Z) sum_{j != i} q_ij^2 (y_i - y_j)) of the embedding y (device float32 [n, 2])
    under the joint affinities ``P = (rowptr, col, val)`` (``tsne_joint``).  Three launches: sslcr_tsne_repulsion (the exact O(n^2)
    sum, grid = row tiles x ``slices``, and the fold of Z) and sslcr_tsne_update without a state.  kl_rows: device float64 [n] to
    receive every row's share of the KL divergence.  Two calls return equal bits; ``slices`` changes only where the float32 partial
    sums are cut.  No sync."""
    n = _tsne_y("tsne_gradient", y)
    rowptr, col, val = _tsne_P("tsne_gradient", P, n, y.device)
    w = workspace or tsne_workspace(n, y.device, slices)
    grad = torch.empty_like(y)
    d = L.TsneGradDesc(L.ptr(y), None, None, None, L.ptr(grad), L.ptr(rowptr), L.ptr(col), L.ptr(val), L.ptr(w["ws"]), L.ptr(w["Z"]), L.ptr(kl_rows),
                       n, w["slices"], col.numel(), float(exaggeration), 0.0, 0.0, 0.0)
    L.check(L.lib().sslcr_tsne_repulsion(d, L.stream_ptr()))
    L.check(L.lib().sslcr_tsne_update(d, L.stream_ptr()))
    return grad, w["Z"]


def tsne_step(y, y_out, update, gains, P, *, exaggeration, momentum, lr, min_gain=0.01, workspace=None, slices=None, grad=None, kl_rows=None):
    """one t-SNE iteration (three launches, no sync): the gradient of ``tsne_gradient`` at y, then sklearn's ``_gradient_descent``
    update: ``gains`` += 0.2 where ``update * grad < 0`` else *= 0.8, floored at min_gain; ``update`` = momentum update - lr gains grad
    (both in place); ``y_out`` = y + update.  y_out is the OTHER of two ping-pong buffers: other rows still read y.  -> grad."""
    n = _tsne_y("tsne_step", y)
    rowptr, col, val = _tsne_P("tsne_step", P, n, y.device)
    for t in (y_out, update, gains):
        if _tsne_y("tsne_step", t) != n or t.device != y.device:
            raise L.SslcrError("tsne_step: y, y_out, update and gains must share shape and device")
    if y_out.data_ptr() == y.data_ptr():
        raise L.SslcrError("tsne_step: y_out must not be y")
    w = workspace or tsne_workspace(n, y.device, slices)
    grad = torch.empty_like(y) if grad is None else grad
    d = L.TsneGradDesc(L.ptr(y), L.ptr(y_out), L.ptr(update), L.ptr(gains), L.ptr(grad), L.ptr(rowptr), L.ptr(col), L.ptr(val), L.ptr(w["ws"]),
                       L.ptr(w["Z"]), L.ptr(kl_rows), n, w["slices"], col.numel(), float(exaggeration), float(momentum), float(lr), float(min_gain))
    L.check(L.lib().sslcr_tsne_repulsion(d, L.stream_ptr()))
    L.check(L.lib().sslcr_tsne_update(d, L.stream_ptr()))
    return grad


def tsne_kl(kl_rows, grad, Z, log_row, iteration):
    """``log_row`` (device float64 [4]) = (sum of kl_rows, |grad|_2, Z, iteration) (sslcr_tsne_kl, one workgroup, no sync)"""
    _chk(kl_rows, grad, Z, log_row)
    L.check(L.lib().sslcr_tsne_kl(L.ptr(kl_rows), L.ptr(grad), L.ptr(Z), L.ptr(log_row), kl_rows.numel(), int(iteration), L.stream_ptr()))
    return log_row


def grad_norm(flat, max_norm=float("inf")):
    """-> device tensor [norm, coef] for a 1-D fp32 tensor (any length, any 4-byte-aligned view): its 2-norm, summed in double in a
    fixed order, and min(1, max_norm / (norm + 1e-6)) -- torch.nn.utils.clip_grad_norm_'s two numbers (sslcr_grad_norm).  No sync."""
    if not flat.is_cuda or flat.dtype != torch.float32 or flat.dim() != 1 or (flat.numel() > 1 and flat.stride(0) != 1):
        raise L.SslcrError("grad_norm: a dense 1-D fp32 device tensor expected (no CPU fallback)")
    partials = torch.empty(L.lib().sslcr_grad_norm_partials(), dtype=torch.float64, device=flat.device)
    out2 = torch.empty(2, dtype=torch.float32, device=flat.device)
    L.check(L.lib().sslcr_grad_norm(L.ptr(flat), flat.numel(), float(max_norm), L.ptr(partials), L.ptr(out2), L.stream_ptr()))
    return out2


def grad_accumulate(dst, src):
    """dst += src in place for two dense 1-D fp32 device tensors of one length (any length, any 4-byte-aligned views, which may sit
    at different offsets mod 16 and must not overlap): one IEEE fp32 add per element, autograd's ``.grad +=``
    (sslcr_grad_accumulate).  -> dst.  No sync."""
    for t in (dst, src):
        if not t.is_cuda or t.dtype != torch.float32 or t.dim() != 1 or (t.numel() > 1 and t.stride(0) != 1):
            raise L.SslcrError("grad_accumulate: dense 1-D fp32 device tensors expected (no CPU fallback)")
    if dst.numel() != src.numel() or dst.device != src.device:
        raise L.SslcrError(f"grad_accumulate: dst has {dst.numel()} elements on {dst.device}, src {src.numel()} on {src.device}")
    L.check(L.lib().sslcr_grad_accumulate(L.ptr(dst), L.ptr(src), dst.numel(), L.stream_ptr()))
    return dst


# ---- Pillow-exact resize (csrc/resample.hip; the definition stands in include/sslcr.h)
RESAMPLE_FILTERS = L.RESAMPLE_FILTERS
_FAKE = 4096                  # a non-NULL "device pointer" for plan queries: sslcr_resample_plan reads NULL-ness only
_RESAMPLE_CACHE_MAX = 64      # table sets kept (a loader uses one; a random-scale crop a new one per batch)
_resample_cache = {}


def resize_output_size(h, w, size):
    """-> (oh, ow) of ``torchvision.transforms.Resize(size)`` for an image of h x w.  An int: the shorter edge becomes ``size`` and
    the other ``int(size * long / short)`` (torchvision's ``_compute_resized_output_size``); a pair is taken as (h, w).
    PARITY UNPINNED against torchvision (it is not installed where the goldens are made): the rule is transcribed,
    the tests hold it to literal values."""
    h, w = int(h), int(w)
    if h < 1 or w < 1:
        raise ValueError(f"resize_output_size: image of {h} x {w}")
    if isinstance(size, (tuple, list)) and len(size) == 2:
        oh, ow = int(size[0]), int(size[1])
    else:
        if isinstance(size, (tuple, list)):
            if len(size) != 1:
                raise ValueError(f"resize_output_size: size = {size!r}")
            size = size[0]
        short, long = (w, h) if w <= h else (h, w)
        new_short, new_long = int(size), int(int(size) * long / short)
        ow, oh = (new_short, new_long) if w <= h else (new_long, new_short)
    if oh < 1 or ow < 1:
        raise ValueError(f"resize_output_size: size = {size!r} gives {oh} x {ow}")
    return oh, ow


def resample_axis(in_size, in0, in1, out_size, resample, k_stride=None):
    """-> (k int32 [out_size, k_stride], bounds int32 [out_size, 2]) of one axis, host numpy (sslcr_resample_coeffs; no device).
    SslcrError where the entry refuses: an unknown filter, a box outside the axis, a table no int32 pass can take."""
    import numpy as np
    code = resample_filter_code(resample)
    ks = L.lib().sslcr_resample_ksize(float(in0), float(in1), int(out_size), code)
    if ks < 1:
        raise L.SslcrError(f"resample_axis: no table for [{in0}, {in1}) -> {out_size} with filter {resample!r}")
    stride = ks if k_stride is None else int(k_stride)
    k = np.zeros((int(out_size), stride), dtype=np.int32)
    b = np.zeros((int(out_size), 2), dtype=np.int32)
    L.check(L.lib().sslcr_resample_coeffs(int(in_size), float(in0), float(in1), int(out_size), code, k.ctypes.data, stride, b.ctypes.data))
    return k, b


def resample_filter_code(resample):
    """a filter name ('nearest', 'box', 'bilinear', 'hamming', 'bicubic', 'lanczos') or Pillow's code -> the SSLCR_RESAMPLE_* code;
    ValueError for anything else"""
    if isinstance(resample, str):
        if resample.lower() not in RESAMPLE_FILTERS:
            raise ValueError(f"unknown resample filter {resample!r} (known: {sorted(RESAMPLE_FILTERS)})")
        return RESAMPLE_FILTERS[resample.lower()]
    if int(resample) not in RESAMPLE_FILTERS.values():
        raise ValueError(f"unknown resample filter code {resample!r}")
    return int(resample)                     # Pillow's Image.Resampling members are these ints


def _resample_boxes(box, n, IH, IW, nearest):
    """box -> (float64 [T, 4] distinct boxes, int32 [n] set of each image or None), rounded to float32 and checked as Pillow does"""
    import numpy as np
    if box is None:
        return np.array([[0.0, 0.0, IW, IH]]), None
    if nearest:
        raise ValueError("pil_resize: NEAREST takes box=None only (Pillow walks a box in fixed point: not reproduced)")
    b = np.asarray(box, dtype=np.float32).astype(np.float64)         # Pillow parses the box into C floats
    if b.shape == (4,):
        b, index = b[None], None
    elif b.ndim == 2 and b.shape == (n, 4):
        b, inv = np.unique(b, axis=0, return_inverse=True)
        index = np.ascontiguousarray(inv.reshape(-1).astype(np.int32))
    else:
        raise ValueError(f"pil_resize: box must be None, one (left, upper, right, lower) or an array [{n}, 4]")
    if len(b):
        if (b[:, :2] < 0).any():
            raise ValueError("box offset can't be negative")
        if (b[:, 2] > IW).any() or (b[:, 3] > IH).any():
            raise ValueError("box can't exceed original image size")
        if (b[:, 2] - b[:, 0] <= 0).any() or (b[:, 3] - b[:, 1] <= 0).any():
            raise ValueError("box can't be empty")
    return b, index


class _ResampleTables:
    """the table sets of one (sizes, boxes, filter): host arrays (the plan reads the bounds) and their per-device uploads"""

    def __init__(self, IH, IW, OH, OW, code, boxes):
        import numpy as np
        self.T, self.nearest = len(boxes), int(code == RESAMPLE_FILTERS["nearest"])
        self.k, self.b, self.ks, self.dev, self.index = [None, None], [None, None], [1, 1], {}, {}
        for axis, (isz, osz, lo, hi) in enumerate(((IW, OW, boxes[:, 0], boxes[:, 2]), (IH, OH, boxes[:, 1], boxes[:, 3]))):
            # Pillow skips the pass of an axis exactly when outSize == inSize, in0 == 0 and in1 == outSize.  In a batch of several
            # boxes the pass runs for all once one of them needs it: the table of an axis that could be skipped is the identity
            # (one coefficient of 2^22 at the pixel itself, the rest round to 0), so the bytes are the same.
            if osz == isz and (lo == 0).all() and (hi == osz).all():
                continue
            ks = max(L.lib().sslcr_resample_ksize(float(a), float(c), osz, code) for a, c in zip(lo, hi))
            parts = [resample_axis(isz, a, c, osz, code, ks) for a, c in zip(lo, hi)]
            self.k[axis] = np.ascontiguousarray(np.stack([p[0] for p in parts]))
            self.b[axis] = np.ascontiguousarray(np.stack([p[1] for p in parts]))
            self.ks[axis] = ks

    def on(self, device):
        if device not in self.dev:
            self.dev[device] = [None if a is None else torch.from_numpy(a).to(device) for a in (self.k[0], self.b[0], self.k[1], self.b[1])]
        return self.dev[device]

    def index_on(self, device, index):
        """the per-image set index on the device: uploaded when this (tables, device, index) is first seen, then reused"""
        key = (device, index.tobytes())
        if key not in self.index:
            while len(self.index) >= 8:
                self.index.pop(next(iter(self.index)))
            self.index[key] = torch.from_numpy(index).to(device)
        return self.index[key]


def _resample_tables(IH, IW, OH, OW, code, boxes):
    key = (IH, IW, OH, OW, code, boxes.tobytes())
    t = _resample_cache.get(key)
    if t is None:
        while len(_resample_cache) >= _RESAMPLE_CACHE_MAX:
            _resample_cache.pop(next(iter(_resample_cache)))
        t = _resample_cache[key] = _ResampleTables(IH, IW, OH, OW, code, boxes)
    return t


_RESAMPLE_FORMS = {None: 0, "fused": 1, "two_pass": 2}


def _resample_desc(t, ptrs, index_ptr, N, C, IH, IW, OH, OW, src_chw, dst_chw, form):
    if form not in _RESAMPLE_FORMS:
        raise ValueError(f"pil_resize: form = {form!r} (None, 'fused' or 'two_pass')")
    src, dst, kx, bx, ky, by = ptrs
    host = [None if a is None else a.ctypes.data for a in t.b]
    return L.ResampleDesc(src, dst, kx, bx, ky, by, index_ptr, host[0], host[1], None, N, C, IH, IW, OH, OW, t.ks[0], t.ks[1], max(t.T, 1),
                          int(src_chw), int(dst_chw), t.nearest, _RESAMPLE_FORMS[form])


def _resample_plan(d):
    p = L.ResamplePlan()
    L.check(L.lib().sslcr_resample_plan(d, p))
    return p


def resample_plan(in_hw, size, resample="bilinear", box=None, *, n=1, channels=3, layout="hwc", out_layout=None, form=None):
    """What ``pil_resize`` would launch for n images of in_hw = (h, w) -> size = (ow, oh): sslcr_resample_plan's answer as a dict --
    form ('fused', 'two_pass', 'horizontal', 'vertical', 'gather'), fused_ok, tile (w, h), window (rows, cols), grid, lds_bytes,
    workspace_bytes.  Host only: no device is needed.  SslcrError where the entry refuses (form='fused' where it does not fit)."""
    IH, IW = int(in_hw[0]), int(in_hw[1])
    OW, OH = int(size[0]), int(size[1])
    code = resample_filter_code(resample)
    boxes, index = _resample_boxes(box, n, IH, IW, code == RESAMPLE_FILTERS["nearest"])
    t = _resample_tables(IH, IW, OH, OW, code, boxes)
    fake = [_FAKE, _FAKE] + [None if a is None else _FAKE for a in (t.k[0], t.b[0], t.k[1], t.b[1])]
    d = _resample_desc(t, fake, None if index is None else _FAKE, n, channels, IH, IW, OH, OW, layout == "chw",
                       (out_layout or layout) == "chw", form)
    p = _resample_plan(d)
    return {"form": L.RESAMPLE_FORMS[p.form], "fused_ok": bool(p.fused_ok), "tile": (p.tile_w, p.tile_h), "window": (p.rows, p.cols),
            "grid": (p.grid[0], p.grid[1]), "lds_bytes": int(p.lds_bytes), "workspace_bytes": int(p.workspace_bytes)}


def _resize_layout(x, layout):
    if layout is None:
        layout = "hwc" if x.shape[3] in (1, 3) else "chw"
    if layout not in ("hwc", "chw"):
        raise ValueError(f"pil_resize: layout = {layout!r} ('hwc' or 'chw')")
    n, a, b, c = x.shape
    C, H, W = (c, a, b) if layout == "hwc" else (a, b, c)
    if C not in (1, 3):
        raise L.SslcrError(f"pil_resize: {C} channels in a {layout} batch of shape {tuple(x.shape)} (modes L and RGB: 1 or 3)")
    return layout, n, C, H, W


def pil_resize(x, size, resample="bilinear", box=None, out=None, out_layout=None, form=None, *, layout=None):
    """``PIL.Image.resize(size, resample, box)`` of every image of a device uint8 batch, byte for byte (sslcr_resample; pinned to
    Pillow 12.2.0 by tests/test_resize_*.py).  x: [N, H, W, C] ('hwc') or [N, C, H, W] ('chw'), C in {1, 3}; layout=None takes 'hwc'
    when the last dimension is 1 or 3, else 'chw'.  size = (ow, oh), as Pillow's.  resample: 'nearest', 'box', 'bilinear', 'hamming',
    'bicubic', 'lanczos' or Pillow's code.  box: None, one (left, upper, right, lower), or a host array [N, 4] -- every image its
    own box, still one launch (the distinct boxes become table sets, chosen per image by a device index).  A box is rounded to
    float32 and checked as Pillow does.  out / out_layout: the result's buffer / layout (default: x's layout).  form: None = the
    plan's choice; 'fused' / 'two_pass' force one (SslcrError where 'fused' does not fit).  The coefficient tables are made on the
    host once per (sizes, box, filter) and uploaded once per device, and so is the per-image index of an [N, 4] box.  A call whose
    tables are cached launches without a sync; the FIRST call of a (sizes, box, filter) builds the tables on the host and copies
    them from pageable memory, which blocks the host until the copy is done -- a batch with fresh boxes every call (a random-scale
    crop) pays that every call.  The uploads are ordered on the stream that is current at that first call: a later call on ANOTHER
    stream must be ordered after it by the caller (the loaders here use one stream)."""
    _chk(x, out)
    if x.dtype != torch.uint8 or x.dim() != 4:
        raise L.SslcrError("pil_resize: a uint8 batch [N, H, W, C] or [N, C, H, W] expected")
    layout, N, C, IH, IW = _resize_layout(x, layout)
    out_layout = out_layout or layout
    if out_layout not in ("hwc", "chw"):
        raise ValueError(f"pil_resize: out_layout = {out_layout!r} ('hwc' or 'chw')")
    OW, OH = int(size[0]), int(size[1])
    if OW < 1 or OH < 1:
        raise ValueError("height and width must be > 0")
    code = resample_filter_code(resample)
    boxes, index = _resample_boxes(box, N, IH, IW, code == RESAMPLE_FILTERS["nearest"])
    shape = (N, OH, OW, C) if out_layout == "hwc" else (N, C, OH, OW)
    out = _out(out, shape, torch.uint8, x.device, f"pil_resize: out must be a uint8 tensor {list(shape)} on the batch's device")
    if N == 0:
        return out
    t = _resample_tables(IH, IW, OH, OW, code, boxes)
    tables = t.on(x.device)
    idx = None if index is None else t.index_on(x.device, index)
    d = _resample_desc(t, [L.ptr(x), L.ptr(out)] + [L.ptr(a) for a in tables], L.ptr(idx), N, C, IH, IW, OH, OW, layout == "chw",
                       out_layout == "chw", form)
    p = _resample_plan(d)
    work = None
    if p.workspace_bytes:
        work = torch.empty(p.workspace_bytes, dtype=torch.uint8, device=x.device)
        d.workspace = L.ptr(work)
    L.check(L.lib().sslcr_resample(d, L.stream_ptr()))
    return out


# ---- linear probe over fixed features (csrc/linprobe.hip)
LINPROBE_LOSSES, LINPROBE_FORMS = L.LINPROBE_LOSSES, L.LINPROBE_FORMS
LINPROBE_TILE, LINPROBE_CHUNK, LINPROBE_MAX_C, LINPROBE_MAX_D = L.LINPROBE_TILE, L.LINPROBE_CHUNK, L.LINPROBE_MAX_C, L.LINPROBE_MAX_D


def _linprobe_loss(name, loss):
    if loss not in LINPROBE_LOSSES:
        raise L.SslcrError(f"{name}: loss = {loss!r} outside {tuple(LINPROBE_LOSSES)}")
    return LINPROBE_LOSSES[loss]


def _linprobe_plan(n, dim, n_classes, loss, groups):
    p = L.LinprobePlan()
    L.check(L.lib().sslcr_linprobe_plan(int(n), int(dim), int(n_classes), int(loss), int(groups or 0), p))
    return p


def linprobe_plan(n, dim, n_classes, loss="softmax", groups=None):
    """what ``linprobe_eval`` launches for these sizes (sslcr_linprobe_plan; host only, no device needed): dict with ``form``
    ("staged": the row tile is fetched once and serves both products | "streamed": wide D, read twice), ``tile_rows``, ``groups`` (G),
    ``tiles_per_group``, ``col_slices``, ``chunk``, ``class_blocks``, ``grid`` (workgroups of the three launches), ``lds_bytes`` and
    ``workspace_bytes``.  groups: a hint > 0 forces G (None / 0 = the plan's choice)."""
    p = _linprobe_plan(n, dim, n_classes, _linprobe_loss("linprobe_plan", loss), groups)
    out = {f: getattr(p, f) for f, _ in L.LinprobePlan._fields_}
    out["grid"] = tuple(p.grid)
    out["form"] = LINPROBE_FORMS[p.form]
    return out


def _linprobe_wb(name, x, w, b):
    x = _f32_rows(name, x)
    n, D = x.shape
    if w.dtype != torch.float32 or w.dim() != 2 or w.shape[1] != D or w.device != x.device:
        raise L.SslcrError(f"{name}: w must be float32 [C, {D}] on x's device, got {w.dtype} {list(w.shape)}")
    Cn = w.shape[0]
    if b.dtype != torch.float32 or tuple(b.shape) != (Cn,) or b.device != x.device:
        raise L.SslcrError(f"{name}: b must be float32 [{Cn}] on x's device")
    return x, w.contiguous(), b.contiguous(), n, D, Cn


def linprobe_eval(x, y, w, b, loss="softmax", sample_weight=None, groups=None, want_logits=False, out=None, logits_out=None):
    """-> ``(value, grad)`` or ``(value, grad, logits)``: the weighted mean loss of the linear classifier ``x w^T + b`` over the rows of
    x and its gradient, fused (sslcr_linprobe_eval: x is read once where a 32-row tile fits LDS; three launches, no sync).  x: device
    float32 [n, D], D % 4 == 0, 4 <= D <= 2048; w float32 [C, D], b float32 [C], 1 <= C <= 64.  loss "softmax": y integer labels [n],
    a label outside [0, C) leaves its row out of the sums AND of the weight total; "squared": y float32 [n, C], 1/2 sum_c (z - t)^2.
    sample_weight: float32 [n] or None.  ``value`` is a 0-d float64 view and ``grad`` a float64 [C, D + 1] view (columns 0 .. D - 1 =
    d/dW, column D = d/db) of ONE device buffer of 1 + C (D + 1) float64 -- ``value.base`` -- so that a caller copies both with one
    copy; ``out``: that buffer, to write into.  logits: float32 [n, C] (want_logits; ``logits_out``: the tensor to write them into).  The data term only: a penalty is the caller's.
    groups: the plan's hint (None = its choice); two calls with the same groups return equal bits."""
    code = _linprobe_loss("linprobe_eval", loss)
    x, w, b, n, D, Cn = _linprobe_wb("linprobe_eval", x, w, b)
    dev = x.device
    labels = targets = None
    if code == LINPROBE_LOSSES["softmax"]:
        if y.is_floating_point() or y.dim() != 1 or y.shape[0] != n or y.device != dev:
            raise L.SslcrError(f"linprobe_eval: {n} integer labels on x's device expected")
        labels = y.long().contiguous()
    else:
        if y.dtype != torch.float32 or tuple(y.shape) != (n, Cn) or y.device != dev:
            raise L.SslcrError(f"linprobe_eval: float32 targets [{n}, {Cn}] on x's device expected")
        targets = y.contiguous()
    if sample_weight is not None:
        if sample_weight.dtype != torch.float32 or tuple(sample_weight.shape) != (n,) or sample_weight.device != dev:
            raise L.SslcrError(f"linprobe_eval: sample_weight must be float32 [{n}] on x's device")
        sample_weight = sample_weight.contiguous()
    p = _linprobe_plan(n, D, Cn, code, groups)
    E = Cn * (D + 1)
    buf = _out(out, (1 + E,), torch.float64, dev, f"linprobe_eval: out must be float64 [{1 + E}] on x's device")
    _chk(buf)
    logits = None
    if want_logits or logits_out is not None:
        logits = _out(logits_out, (n, Cn), torch.float32, dev, f"linprobe_eval: logits_out must be float32 [{n}, {Cn}] on x's device")
        _chk(logits)
    ws = torch.empty(p.workspace_bytes // 16 + 1, dtype=torch.complex128, device=dev)       # 16-byte elements
    d = L.LinprobeDesc(L.ptr(x), L.ptr(w), L.ptr(b), L.ptr(labels), L.ptr(targets), L.ptr(sample_weight), L.ptr_at(buf, 0), L.ptr_at(buf, 8),
                       L.ptr(logits), L.ptr(ws), n, D, Cn, code, int(groups or 0))
    L.check(L.lib().sslcr_linprobe_eval(d, L.stream_ptr()))
    value, grad = buf[0], buf[1:].view(Cn, D + 1)
    return (value, grad, logits) if logits is not None else (value, grad)


def linprobe_logits(x, w, b, groups=None, out=None):
    """-> float32 [n, C] = ``x w^T + b`` for device float32 queries x [n, D] (sslcr_linprobe_logits): the first product of
    ``linprobe_eval`` alone -- the same fp32 chain over D in rising order plus one addition of b -- so its bits equal the ``logits``
    ``linprobe_eval`` returns for the same rows, whatever the plan.  No sync."""
    x, w, b, n, D, Cn = _linprobe_wb("linprobe_logits", x, w, b)
    p = _linprobe_plan(n, D, Cn, 0, groups)
    logits = _out(out, (n, Cn), torch.float32, x.device, f"linprobe_logits: out must be float32 [{n}, {Cn}] on x's device")
    _chk(logits)
    ws = torch.empty(p.workspace_bytes // 16 + 1, dtype=torch.complex128, device=x.device)
    d = L.LinprobeDesc(L.ptr(x), L.ptr(w), L.ptr(b), None, None, None, None, None, L.ptr(logits), L.ptr(ws), n, D, Cn, 0, int(groups or 0))
    L.check(L.lib().sslcr_linprobe_logits(d, L.stream_ptr()))
    return logits
