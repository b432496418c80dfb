"""Case table of the non-conv kernels (data only): BatchNorm finalize / apply / backward, pooling, the fp32 heads and the losses.

    (op, dtype, shape, flags, branch)

op      the C-ABI entry point under test, without its sslcr_ prefix.
dtype   0 fp32, 1 bf16 (None where the kernel is fp32 only).
shape   per op, see the section comments.  N = None: the test derives the batch from the device, as the smallest N whose 16-byte
        chunks exceed the grid cap of ew_grid() by 4 % -- cap = 3 * CUs workgroups * 256 threads (bn_eltwise.hip: "THREE workgroups per
        CU"), so that the grid-stride loops take a second trip on whatever part the suite runs on.
flags   space-separated words the test turns into descriptor fields.
branch  which launcher branch the row takes, quoting the condition from the source.
"""

# ---- sslcr_bn_finalize: shape = (rows, C, nseg); every row carries a channel with mean / std = 1e3 (channel 0) and a constant channel
# (channel 1: the variance is exactly 0); flags: count1 = one element per channel (count = 1: unbiased variance = variance)
BN_FINALIZE = [
    ("bn_finalize", None, (1, 40, 1), "", "splits = rows / 32 -> 'if (splits < 1) splits = 1'; cdiv(C, 32) = 2 channel blocks, the second ragged"),
    ("bn_finalize", None, (1, 64, 1), "count1", "'a.count > 1.0 ? var * a.count / (a.count - 1.0) : var' -- the else arm"),
    ("bn_finalize", None, (31, 64, 1), "", "one split: the 8 row lanes walk 'for (; r + 8 < r1; r += 16)' then the 'r += 8' tail"),
    ("bn_finalize", None, (200, 512, 1), "", "splits = 200 / 32 = 6: per = 34 rows, the last split ragged"),
    ("bn_finalize", None, (2048, 64, 1), "", "rows / 32 = 64 -> 'if (splits > SPLITS) splits = SPLITS' (32)"),
    ("bn_finalize", None, (93, 64, 3), "", "nseg = 3: 'const int rows = a.rows / nseg' = 31 per segment, running statistics updated segment by segment"),
    ("bn_finalize", None, (600, 512, 3), "", "nseg = 3, 200 rows and 6 splits per segment"),
    ("bn_finalize", None, (6144, 40, 3), "", "nseg = 3, 2048 rows per segment: splits capped at 32"),
]

# ---- sslcr_bn_act: shape = (N, H, W, C); flags: res (+ residual), bnres (+ bn(residual)), relu, nseg3, bits (bf16: ybits)
_SMALL, _F32_OVER, _BF16_OVER = (3, 10, 10, 64), (None, 64, 64, 64), (None, 64, 64, 64)
BN_ACT = [(op, dt, _SMALL, fl, "one trip: 'b * 256 >= work_items' (ew_grid_cols returns the uncapped grid)")
          for op in ("bn_act",) for dt in (0, 1) for fl in ("", "relu", "res", "res relu", "bnres", "bnres relu bits" if dt else "bnres relu")]
BN_ACT += [
    ("bn_act", 0, (6, 10, 10, 64), "bnres relu nseg3", "grid y = segment: 'dim3(ew_grid_cols(per * (a.C / 4), a.C / 4), nseg)'"),
    ("bn_act", 1, (6, 10, 10, 64), "bnres relu nseg3 bits", "grid y = segment, ybits at 'blockIdx.y * total + i'"),
    ("bn_act", 0, _F32_OVER, "bnres relu", "capped grid, cols = 16: 'b > cap ? cap : b', m = cols / gcd(cols, 256) = 1 -- the launch is ew_grid()'s"),
    ("bn_act", 1, _BF16_OVER, "bnres relu bits", "capped grid, cols = 8: second trip of 'i += gridDim.x * 256' with m = 1"),
]

# ---- the cached-constant defect: widths whose chunks per pixel (cols) do not divide the capped stride.  shape = (N, H, W, C) of the
# tensor the grid-stride loop walks (the pooled OUTPUT for bn_relu_maxpool: its input is [N, 2H, 2W, C])
STRIDE = [
    ("bn_act", 1, (None, 40, 25, 40), "bnres relu bits", "cols = 5: capped grid rounded down to a multiple of m = 5 ('b - b % m')"),
    ("bn_act", 0, (None, 20, 25, 40), "bnres relu", "cols = 10: m = 10 / gcd(10, 256) = 5"),
    ("bn_relu_maxpool", 1, (None, 40, 25, 40), "", "generic form ('256 % cols' != 0), cols = 5, capped grid"),
    ("bn_relu_maxpool", 0, (None, 20, 25, 40), "", "generic form, cols = 10, capped grid"),
    ("bn_relu_maxpool", 1, (None, 40, 25, 56), "", "generic form, cols = 7: m = 7"),
    ("bn_bwd_apply", 1, (None, 40, 25, 40), "relu_from_x", "direct descriptor (launch_bn_bwd_reduce returns hipErrorInvalidValue: bn_bwd_reduce_cols, '(256 % cols) != 0'), cols = 5"),
    ("bn_bwd_apply", 0, (None, 20, 25, 40), "yact", "direct descriptor, cols = 10"),
]

# ---- pooling: shape = (N, H, W, C) of the INPUT.  Every row runs bn_relu_maxpool (values, codes), maxpool_relu_bwd, avgpool_fwd and
# avgpool_bwd on the pooled map; channel 1 has scale == 0 (every window element ties: the first one wins, code 0 or 9 by the shift)
POOL = [("pool", dt, (3, h, w, C), "",
         ("row form: 'cols <= 256 && 256 % cols == 0'" if C in (64, 512) else "generic form: cols = %d does not divide 256" % (C // (8 if dt else 4))))
        for dt in (0, 1) for C in (64, 24, 40, 512) for (h, w) in ((1, 1), (2, 2), (9, 7), (16, 16))]
POOL += [
    ("pool", 1, (None, 64, 64, 64), "bwd_only", "maxpool_relu_bwd / avgpool_bwd above the cap: second trip of 'i += gridDim.x * 256'"),
    ("pool", 0, (None, 64, 64, 64), "bwd_only", "the same in fp32 (cols = 16)"),
]

# ---- sslcr_bn_bwd_reduce / _apply: shape = (N, H, W, C); flags: the mode (yact, yact_bits, yact_gir = g_in_reduce, from_x, plain, pool =
# gather through the max-pool, pool_y = pooled reduce), nseg3.  Channel 2 of every row has mean / std = 30.
BN_BWD = [("bn_bwd", dt, (3, 10, 10, 128), m, "256-thread form: blocks = cdiv(cdiv(300, rpp), 8) < 512")
          for dt in (0, 1) for m in ("yact", "yact_gir", "from_x", "plain")]
BN_BWD += [
    ("bn_bwd", 1, (3, 10, 10, 128), "yact_bits", "'EPC == 8 && a.yact_bits': the mask read as one bit per element"),
    ("bn_bwd", 0, (3, 10, 10, 128), "yact_gir nseg3", "grid y = segment (bn_bwd_segment), 100 pixels each"),
    ("bn_bwd", 1, (3, 10, 10, 128), "from_x nseg3", "grid y = segment"),
    ("bn_bwd", 1, (3, 10, 10, 128), "plain nseg3", "grid y = segment"),
    # 'big = blocks >= 512': blocks = cdiv(cdiv(pixels, rpp), 8), rpp = 256 / cols.  bf16 C = 512: cols = 64, rpp = 4 -> pixels >= 16353;
    # fp32 C = 512: cols = 128, rpp = 2 -> pixels >= 8177.  (pixels * C is the same for every width: 512 * 8 * 256 * EPC elements.)
    ("bn_bwd", 1, (16, 32, 32, 512), "yact", "1024-thread form: 16384 pixels -> blocks = 512, b4 = cdiv(cdiv(16384, 16), 8) = 128 workgroups"),
    ("bn_bwd", 1, (16, 32, 32, 512), "plain", "1024-thread form"),
    ("bn_bwd", 0, (8, 32, 32, 512), "from_x", "1024-thread form, fp32: 8192 pixels -> blocks = 512, b4 = 128"),
    ("bn_bwd", 0, (4, 15, 13, 64), "pool", "'a.pool_dy ? run(std::true_type{})': bn_bwd_reduce_kernel<T, NB, POOL = true>, the gather of bn_bwd_g (windows: bn_bwd.hpp), ragged map; apply: bn_bwd_apply_pool_kernel on 2x2 blocks"),
    ("bn_bwd", 1, (4, 15, 13, 64), "pool", "the same in bf16"),
    ("bn_bwd", 0, (4, 16, 16, 64), "pool", "gather form, even map"),
    ("bn_bwd", 1, (4, 16, 16, 64), "pool", "gather form, even map, bf16"),
    ("bn_bwd", 0, (4, 15, 13, 64), "pool_y", "'a.pool_dy && a.pool_y': bn_bwd_reduce_pool_kernel on the pooled tensors; a scale == 0 channel fetches x"),
    ("bn_bwd", 1, (4, 15, 13, 64), "pool_y", "the same in bf16"),
    ("bn_bwd", 0, (4, 16, 16, 64), "pool_y", "pooled reduce, even map"),
    ("bn_bwd", 1, (4, 16, 16, 64), "pool_y", "pooled reduce, even map, bf16"),
]

# ---- heads: shape = (M, K, N) of y[M, N] = x[M, K] w[N, K]^T; every row runs forward (bias + ReLU, and plain), dx and dw / db into
# non-zero buffers, with and without the ReLU mask
GEMM = [
    ("linear", None, (96, 1024, 512), "", "LDS form in forward and dx: 'M % 32 == 0 && N % 32 == 0 && K % 64 == 0'; dw reduces over M = 96, not % 64 -> direct form"),
    ("linear", None, (32, 64, 32), "", "LDS form, one chunk ('nchunks > 1' false) in the forward; dx / dw direct (reduction 32)"),
    ("linear", None, (37, 1024, 512), "", "direct form: ragged M tile ('row < M'), four waves share K in 64-wide chunks"),
    ("linear", None, (6, 512, 10), "", "direct form: ragged N ('jv'), dx reduces over N = 10: the scalar k-tail 'k0 + e < K' inside one 4-group"),
    ("linear", None, (5, 70, 2), "", "direct form: K = 70 is no multiple of 4 -- 'k0 + 3 < K' fails on the last group, scalar tail"),
    ("linear", None, (300, 66, 1), "", "direct form: N = 1, K = 66; dw reduces over M = 300 = 64 * 4 + 44: a second trip of 'kb += 256'"),
]

# ---- losses: shape = (kind, C, nx, nu); logits scaled so that max |logit| = 80; flags: shift = rows 0 / 1 carry an offset of +100 / -100
# (cross-entropy is shift invariant; a kernel without the max subtraction overflows / underflows there)
LOSS = [("loss", None, (kind, C, 300, 700 if kind in (0, 1) else 0), fl, "'for (int i = threadIdx.x; i < a.nx; i += 256)' takes a second trip (nx = 300)"
         + ("; 'i < a.nu' takes three (nu = 700)" if kind in (0, 1) else ""))
        for (kind, C) in ((0, 1), (1, 2), (1, 9), (2, 6), (3, 1), (1, 64), (2, 64)) for fl in (("", "shift") if kind in (1, 2) else ("",))]
SOFTMAX = [("softmax_col", None, (1000, C), "", "four workgroups, the last ragged ('if (i >= n) return')") for C in (2, 9)]

CASES = BN_FINALIZE + BN_ACT + STRIDE + POOL + BN_BWD + GEMM + LOSS + SOFTMAX

