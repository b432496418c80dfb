"""Route table of the conv kernels (data only).  Each row names one case:

    (op, dtype, (N, H, W, C, K, R, stride, pad), flags, name, tail)

op      fwd: sslcr_conv2d forward; s2pair: sslcr_conv2d_s2_pair (3x3 / 2 + 1x1 / 2 of one input); dgrad: the stride-2 input gradient
        in the engine's par4 form (x = dY [N, OH, OW, K], w = [C][R][S][K], transposed, pix_mul 2); wgrad: sslcr_conv2d_wgrad.
        The other input-gradient forms, each with x = dY and w = [C][R][S][K]:
        dgrad_t: the transposed plain form with a residual (pixel space = the conv's input), stride 1 or 2;
        dgrad_parity: the stride-2 gradient as four launches, one per input-pixel parity class (pix_mul 2, pix_off, tap_mask), with a
        residual -- every launch of the row is the named instance;
        scatter: the 1x1 / 2 gradient as a plain 1x1 conv of dY scattered to the even positions (osh 2) and accumulated into dX.
        The shape is the forward conv's: x [N, H, W, C], w [K, R, R, C].
dtype   0 fp32, 1 bf16.
flags   the descriptor fields the engine sets: stats, in_scale (with in_relu), bias, residual, relu, out_scale, mask (the
        BatchNorm-backward front end, sslcr_conv_desc.mask_x), seg=<images per segment>.
name    exactly what sslcr_conv2d_kernel_name / sslcr_conv2d_wgrad_kernel_name return for the descriptor (for s2pair, the instance
        sslcr_conv2d_s2_pair launches: the single conv's with PAIR = true).
tail    the instance of the second, 64-kout launch where the four-image-tile form splits a shape into head + tail, else None.

ROUTES holds a row for every instance tools/route_sweep.py's grid can name (tests/test_kernel_routes_cpu.py walks the grid and fails
with the name and the smallest descriptor of an instance that has none).  UNLAUNCHABLE: name -> the refusing condition, for an
instance that a descriptor can name but no descriptor launches under the default switches.  BEYOND_THE_GRID: instances with a
row that only descriptors outside the sweep's grid name.
"""
H16 = "sslcr::conv3x3_h16_kernel<unsigned short, "
H16F = "sslcr::conv3x3_h16_kernel<float, "
TAIL = H16 + "64, 2, false, false, false, 8>"
TAIL_XF = H16 + "64, 2, true, false, false, 8>"
IG = "sslcr::conv_igemm_kernel<unsigned short, 64, 64>"
IGF = "sslcr::conv_igemm_kernel<float, 64, 64>"
Q = "sslcr::conv3x3_halo256_kernel<unsigned short, "
QF = "sslcr::conv3x3_halo256_kernel<float, "
HALO = "sslcr::conv3x3_halo_kernel<unsigned short, ...>"
HALOF = "sslcr::conv3x3_halo_kernel<float, ...>"

ROUTES = [
    # ---- bf16 forward: every instance of the step's profile, and the edges where these kernels go wrong
    ("fwd", 1, (2, 32, 32, 128, 128, 3, 1, 1), "bias residual relu", H16 + "128, 2, false, false, false, 16>", None),
    ("fwd", 1, (2, 32, 32, 128, 128, 3, 1, 1), "out_scale bias residual relu", "sslcr::conv3x3_h16s_kernel<unsigned short, 128, 2, false, 16>", None),
    ("fwd", 1, (2, 32, 32, 128, 128, 3, 1, 1), "stats", H16 + "128, 2, false, false, true, 16>", None),
    ("fwd", 1, (2, 32, 32, 128, 128, 3, 1, 1), "in_scale stats", H16 + "128, 2, true, false, true, 16>", None),
    ("fwd", 1, (33, 32, 32, 64, 256, 3, 1, 1), "stats", H16 + "128, 2, false, false, true, 16>", None),      # 264 items: a walk into the next kout block
    ("fwd", 1, (2, 16, 16, 64, 64, 3, 1, 1), "bias residual relu", "sslcr::conv3x3_pp64_kernel<false, 1>", None),
    ("fwd", 1, (2, 16, 16, 64, 64, 3, 1, 1), "stats", "sslcr::conv3x3_pp64_kernel<false, 0>", None),
    ("fwd", 1, (2, 16, 16, 64, 64, 3, 1, 1), "mask stats", "sslcr::conv3x3_pp64_kernel<false, 2>", None),
    ("fwd", 1, (2, 16, 16, 64, 64, 3, 1, 1), "in_scale stats", "sslcr::conv3x3_pp64_kernel<true, 0>", None),
    ("fwd", 1, (4, 8, 8, 512, 512, 3, 1, 1), "bias residual relu", H16 + "128, 2, false, false, false, 8>", None),
    ("fwd", 1, (4, 8, 8, 512, 512, 3, 1, 1), "out_scale bias residual relu", "sslcr::conv3x3_h16s_kernel<unsigned short, 128, 2, false, 8>", None),
    ("fwd", 1, (4, 8, 8, 512, 512, 3, 1, 1), "stats", H16 + "128, 2, false, false, true, 8>", None),
    ("fwd", 1, (4, 8, 8, 256, 512, 3, 1, 1), "in_scale stats", H16 + "128, 2, true, false, true, 8>", None),
    # the 8x8 head + 64-kout tail launches (N = 320: 64 tail images, N = 640: 128)
    ("fwd", 1, (320, 8, 8, 64, 512, 3, 1, 1), "bias residual relu", H16 + "128, 2, false, false, false, 8>", TAIL),
    ("fwd", 1, (320, 8, 8, 64, 512, 3, 1, 1), "in_scale stats", H16 + "128, 2, true, false, true, 8>", TAIL_XF),
    ("fwd", 1, (640, 8, 8, 64, 512, 3, 1, 1), "stats", H16 + "128, 2, false, false, true, 8>", TAIL),
    ("fwd", 1, (640, 8, 8, 64, 512, 3, 1, 1), "out_scale bias relu", "sslcr::conv3x3_h16s_kernel<unsigned short, 128, 2, false, 8>",
     "sslcr::conv3x3_h16s_kernel<unsigned short, 64, 2, false, 8>"),
    # N not a multiple of the four-image tile: the 8-wide halo kernel (N even), the generic kernel (N odd)
    ("fwd", 1, (6, 8, 8, 128, 128, 3, 1, 1), "stats", "sslcr::conv3x3_halo_kernel<unsigned short, ...>", None),
    ("fwd", 1, (5, 8, 8, 128, 128, 3, 1, 1), "stats", IG, None),
    # gather kernels on ragged maps
    ("fwd", 1, (10, 30, 34, 64, 128, 3, 2, 1), "stats", "sslcr::conv_dma_kernel<unsigned short, 128, 128>", None),
    ("fwd", 1, (10, 30, 34, 128, 64, 3, 2, 1), "stats", "sslcr::conv_dma_kernel<unsigned short, 256, 64>", None),
    ("fwd", 1, (3, 9, 11, 64, 128, 3, 2, 1), "stats", IG, None),
    # segments: 1 and 8
    ("fwd", 1, (2, 16, 16, 64, 64, 3, 1, 1), "in_scale stats seg=2", "sslcr::conv3x3_pp64_kernel<true, 0>", None),
    ("fwd", 1, (8, 16, 16, 64, 64, 3, 1, 1), "in_scale stats seg=1", "sslcr::conv3x3_pp64_kernel<true, 0>", None),
    ("fwd", 1, (8, 16, 16, 128, 128, 3, 1, 1), "in_scale stats seg=1", H16 + "128, 2, true, false, true, 16>", None),
    ("fwd", 1, (8, 8, 8, 512, 512, 3, 1, 1), "in_scale stats seg=4", H16 + "128, 2, true, false, true, 8>", None),
    # the 224-input layer maps (56 / 28 / 14 / 7)
    ("fwd", 1, (2, 56, 56, 64, 64, 3, 1, 1), "in_scale stats", "sslcr::conv3x3_halo_kernel<unsigned short, ...>", None),
    ("fwd", 1, (2, 56, 56, 64, 128, 3, 2, 1), "stats", IG, None),
    ("fwd", 1, (2, 28, 28, 128, 128, 3, 1, 1), "in_scale stats", IG, None),
    ("fwd", 1, (2, 14, 14, 256, 256, 3, 1, 1), "in_scale stats", IG, None),
    ("fwd", 1, (4, 7, 7, 512, 512, 3, 1, 1), "in_scale stats", IG, None),
    # ---- bf16 stride-2 pair and dgrad
    ("s2pair", 1, (8, 32, 32, 64, 128, 3, 2, 1), "stats", "sslcr::conv_s2_kernel<true, false>", None),
    ("s2pair", 1, (8, 32, 32, 64, 128, 3, 2, 1), "out_scale bias relu", "sslcr::conv_s2_kernel<true, true>", None),
    ("dgrad", 1, (2, 32, 32, 64, 128, 3, 2, 1), "", "sslcr::conv_s2d_kernel", None),
    # ---- bf16 weight gradients
    ("wgrad", 1, (2, 16, 16, 64, 64, 3, 1, 1), "", "sslcr::wgrad3x3_halo_kernel<unsigned short, 16, 1>", None),
    ("wgrad", 1, (8, 16, 16, 64, 128, 3, 1, 1), "in_scale seg=1", "sslcr::wgrad3x3_halo_kernel<unsigned short, 16, 2>", None),
    ("wgrad", 1, (5, 32, 32, 128, 128, 3, 1, 1), "in_scale", "sslcr::wgrad3x3_dma_kernel<16, true>", None),
    ("wgrad", 1, (5, 32, 32, 128, 128, 3, 1, 1), "", "sslcr::wgrad3x3_dma_kernel<16, false>", None),
    ("wgrad", 1, (34, 8, 8, 64, 128, 3, 1, 1), "in_scale", "sslcr::wgrad3x3_dma_kernel<8, true>", None),
    ("wgrad", 1, (34, 8, 8, 64, 128, 3, 1, 1), "", "sslcr::wgrad3x3_dma_kernel<8, false>", None),
    ("wgrad", 1, (16, 16, 16, 128, 128, 3, 1, 1), "in_scale seg=2", "sslcr::wgrad3x3_dma_kernel<16, true>", None),
    ("wgrad", 1, (2, 32, 32, 64, 128, 3, 2, 1), "", "sslcr::wgrad_s2_kernel<16>", None),
    ("wgrad", 1, (2, 16, 16, 64, 128, 3, 2, 1), "", "sslcr::wgrad_s2_kernel<8>", None),
    ("wgrad", 1, (2, 16, 16, 64, 128, 1, 2, 0), "", "sslcr::wgrad_kernel<unsigned short, 1, 2>", None),
    ("wgrad", 1, (2, 56, 56, 64, 64, 3, 1, 1), "in_scale", "sslcr::wgrad3x3_halo_kernel<unsigned short, 8, 1>", None),
    ("wgrad", 1, (2, 56, 56, 64, 128, 3, 2, 1), "", "sslcr::wgrad_kernel<unsigned short, 9, 2>", None),
    ("wgrad", 1, (2, 28, 28, 128, 128, 3, 1, 1), "in_scale", "sslcr::wgrad_kernel<unsigned short, 9, 2>", None),
    ("wgrad", 1, (4, 7, 7, 512, 512, 3, 1, 1), "in_scale", "sslcr::wgrad_kernel<unsigned short, 9, 2>", None),
    # ---- fp32: the ResNet18 layer shapes at 256 x 256 input (64 / 32 / 16 / 8) ...
    ("fwd", 0, (2, 64, 64, 64, 64, 3, 1, 1), "in_scale stats", H16F + "64, 2, true, false, false, 16>", None),
    ("fwd", 0, (2, 64, 64, 64, 64, 3, 1, 1), "out_scale bias residual relu", "sslcr::conv3x3_h16s_kernel<float, 64, 2, false, 16>", None),
    ("fwd", 0, (2, 64, 64, 64, 128, 3, 2, 1), "stats", "sslcr::conv_dma_kernel<float, 128, 128>", None),
    ("fwd", 0, (2, 64, 64, 64, 128, 1, 2, 0), "stats", "sslcr::conv_dma_kernel<float, 128, 128>", None),
    ("fwd", 0, (2, 32, 32, 128, 128, 3, 1, 1), "in_scale stats", H16F + "128, 2, true, false, false, 16>", None),
    ("fwd", 0, (2, 32, 32, 128, 256, 3, 2, 1), "stats", IGF, None),
    ("fwd", 0, (2, 16, 16, 256, 256, 3, 1, 1), "in_scale stats", H16F + "128, 2, true, false, false, 16>", None),
    ("fwd", 0, (2, 16, 16, 256, 512, 3, 2, 1), "stats", IGF, None),
    ("fwd", 0, (4, 8, 8, 512, 512, 3, 1, 1), "in_scale stats", H16F + "128, 2, true, false, false, 8>", None),
    ("dgrad", 0, (8, 32, 32, 64, 128, 3, 2, 1), "", "sslcr::conv_dma_kernel<float, 256, 64>", None),
    ("wgrad", 0, (2, 64, 64, 64, 64, 3, 1, 1), "in_scale", "sslcr::wgrad3x3_halo_kernel<float, 16, 1>", None),
    ("wgrad", 0, (2, 64, 64, 64, 128, 3, 2, 1), "", "sslcr::wgrad_kernel<float, 9, 1>", None),
    ("wgrad", 0, (2, 64, 64, 64, 128, 1, 2, 0), "", "sslcr::wgrad_kernel<float, 1, 1>", None),
    ("wgrad", 0, (4, 8, 8, 512, 512, 3, 1, 1), "in_scale", "sslcr::wgrad3x3_halo_kernel<float, 8, 1>", None),
    # ... and at Kather's 224 x 224 (56 / 28 / 14 / 7)
    ("fwd", 0, (2, 56, 56, 64, 64, 3, 1, 1), "in_scale stats", "sslcr::conv3x3_halo_kernel<float, ...>", None),
    ("fwd", 0, (2, 56, 56, 64, 128, 3, 2, 1), "stats", IGF, None),
    ("fwd", 0, (2, 56, 56, 64, 128, 1, 2, 0), "stats", IGF, None),
    ("fwd", 0, (2, 28, 28, 128, 128, 3, 1, 1), "in_scale stats", IGF, None),
    ("fwd", 0, (2, 14, 14, 256, 256, 3, 1, 1), "in_scale stats", IGF, None),
    ("fwd", 0, (4, 7, 7, 512, 512, 3, 1, 1), "in_scale stats", IGF, None),
    ("wgrad", 0, (2, 56, 56, 64, 64, 3, 1, 1), "in_scale", "sslcr::wgrad3x3_halo_kernel<float, 8, 1>", None),
    ("wgrad", 0, (2, 28, 28, 128, 128, 3, 1, 1), "in_scale", "sslcr::wgrad_kernel<float, 9, 1>", None),
    ("wgrad", 0, (4, 7, 7, 512, 512, 3, 1, 1), "in_scale", "sslcr::wgrad_kernel<float, 9, 1>", None),
    # ---- the instances the router answers that no profiled step launched: the smallest descriptor of each
    # fp32 without the producer transform (the fp32 engine's stride-1 input gradients and its eval epilogues)
    ("fwd", 0, (1, 16, 16, 64, 128, 3, 1, 1), "bias residual relu", H16F + "128, 2, false, false, false, 16>", None),
    ("fwd", 0, (1, 16, 16, 64, 128, 3, 1, 1), "stats", H16F + "128, 2, false, false, false, 16>", None),
    ("fwd", 0, (4, 8, 8, 64, 128, 3, 1, 1), "bias residual relu", H16F + "128, 2, false, false, false, 8>", None),
    ("fwd", 0, (4, 8, 8, 64, 128, 3, 1, 1), "stats", H16F + "128, 2, false, false, false, 8>", None),
    ("fwd", 0, (1, 16, 16, 64, 64, 3, 1, 1), "bias residual relu", H16F + "64, 2, false, false, false, 16>", None),
    ("fwd", 0, (1, 16, 16, 64, 64, 3, 1, 1), "stats", H16F + "64, 2, false, false, false, 16>", None),
    ("fwd", 0, (1, 16, 16, 64, 128, 3, 1, 1), "out_scale bias residual relu", "sslcr::conv3x3_h16s_kernel<float, 128, 2, false, 16>", None),
    ("fwd", 0, (4, 8, 8, 64, 128, 3, 1, 1), "out_scale bias residual relu", "sslcr::conv3x3_h16s_kernel<float, 128, 2, false, 8>", None),
    # bf16 64-kout blocks on 16x16 tiles, the filter ring (C != 64: not the resident bank)
    ("fwd", 1, (1, 16, 16, 128, 64, 3, 1, 1), "stats", H16 + "64, 2, false, false, false, 16>", None),
    ("fwd", 1, (1, 16, 16, 128, 64, 3, 1, 1), "bias residual relu", H16 + "64, 2, false, false, false, 16>", None),
    ("fwd", 1, (1, 16, 16, 128, 64, 3, 1, 1), "in_scale stats", H16 + "64, 2, true, false, false, 16>", None),
    ("fwd", 1, (1, 16, 16, 128, 64, 3, 1, 1), "out_scale bias relu", "sslcr::conv3x3_h16s_kernel<unsigned short, 64, 2, false, 16>", None),
    ("fwd", 1, (1, 16, 16, 128, 64, 3, 1, 1), "out_scale bias residual relu", "sslcr::conv3x3_h16s_kernel<unsigned short, 64, 2, false, 16>", None),
    # the bf16 128-kout producer transform without the RAW output stage (any in_scale descriptor that is not plain statistics): the
    # sweep's flag sets do not reach these two (BEYOND_THE_GRID)
    ("fwd", 1, (1, 16, 16, 64, 128, 3, 1, 1), "in_scale bias relu", H16 + "128, 2, true, false, false, 16>", None),
    ("fwd", 1, (4, 8, 8, 64, 128, 3, 1, 1), "in_scale bias relu", H16 + "128, 2, true, false, false, 8>", None),
    ("fwd", 1, (33, 32, 32, 128, 64, 3, 1, 1), "stats", H16 + "64, 2, false, false, false, 16>", None),      # 132 items of 64 kouts
    ("fwd", 1, (65, 32, 32, 128, 64, 3, 1, 1), "stats", H16 + "64, 2, false, false, false, 16>", None),      # 260 items: a second round on 256 CUs
    # conv3x3_halo256: 8x8 maps with K % 128 != 0 ...
    ("fwd", 1, (4, 8, 8, 64, 64, 3, 1, 1), "stats", Q + "8, 64, 1, true>", None),                # ONE: the single channel slab
    ("fwd", 1, (4, 8, 8, 128, 64, 3, 1, 1), "bias residual relu", Q + "8, 64, 2, false>", None),
    ("fwd", 1, (4, 8, 8, 128, 64, 3, 1, 1), "stats", Q + "8, 64, 2, false>", None),
    ("fwd", 0, (4, 8, 8, 64, 64, 3, 1, 1), "", QF + "8, 64, 2, false>", None),
    ("fwd", 0, (4, 8, 8, 64, 64, 3, 1, 1), "in_scale stats", QF + "8, 64, 2, false>", None),
    # ... and every tileable descriptor with in_scale + residual (conv_h16_mode hands them over)
    ("fwd", 1, (1, 16, 16, 64, 128, 3, 1, 1), "in_scale residual", Q + "16, 128, 2, false>", None),
    ("fwd", 0, (1, 16, 16, 64, 128, 3, 1, 1), "in_scale residual", QF + "16, 128, 2, false>", None),
    ("fwd", 1, (1, 16, 16, 64, 64, 3, 1, 1), "in_scale residual", Q + "16, 64, 1, true>", None),
    ("fwd", 1, (1, 16, 16, 128, 64, 3, 1, 1), "in_scale residual", Q + "16, 64, 2, false>", None),
    ("fwd", 0, (1, 16, 16, 64, 64, 3, 1, 1), "in_scale residual", QF + "16, 64, 2, false>", None),
    # four-image tiles in 128-kout blocks.  launch_qt runs a last round of at most half the CUs as 64-kout items: N = 4 is ALL tail (one
    # tile: only the 64-kout instance launches); N = 320 at K = 512 launches 64 head tiles of the named instance and 16 tail tiles
    ("fwd", 1, (4, 8, 8, 64, 128, 3, 1, 1), "in_scale residual", Q + "8, 128, 2, false>", Q + "8, 64, 2, false>"),
    ("fwd", 0, (4, 8, 8, 64, 128, 3, 1, 1), "in_scale residual", QF + "8, 128, 2, false>", QF + "8, 64, 2, false>"),
    ("fwd", 1, (320, 8, 8, 64, 512, 3, 1, 1), "in_scale residual", Q + "8, 128, 2, false>", Q + "8, 64, 2, false>"),
    ("fwd", 0, (320, 8, 8, 64, 512, 3, 1, 1), "in_scale residual", QF + "8, 128, 2, false>", QF + "8, 64, 2, false>"),
    # conv3x3_halo: the name elides (TW, BKO); one row per form and dtype (TW 16: W % 16 == 0 with H % 16 != 0; BKO 128: K % 128 == 0)
    ("fwd", 1, (2, 8, 16, 64, 64, 3, 1, 1), "in_scale stats", HALO, None),        # TW 16, BKO 64
    ("fwd", 1, (2, 8, 16, 64, 128, 3, 1, 1), "in_scale stats", HALO, None),       # TW 16, BKO 128
    ("fwd", 1, (2, 24, 8, 64, 64, 3, 1, 1), "bias residual relu", HALO, None),    # TW 8, BKO 64 (three tile rows)
    ("fwd", 1, (2, 24, 8, 64, 128, 3, 1, 1), "in_scale residual", HALO, None),    # TW 8, BKO 128
    ("fwd", 0, (2, 8, 16, 64, 64, 3, 1, 1), "in_scale stats", HALOF, None),       # TW 16, BKO 64
    ("fwd", 0, (2, 8, 16, 64, 128, 3, 1, 1), "in_scale stats", HALOF, None),      # TW 16, BKO 128
    ("fwd", 0, (2, 24, 8, 64, 64, 3, 1, 1), "bias residual relu", HALOF, None),   # TW 8, BKO 64
    ("fwd", 0, (2, 24, 8, 64, 128, 3, 1, 1), "in_scale residual", HALOF, None),   # TW 8, BKO 128
    # conv_igemm with 128-pixel blocks (65 536 pixels and more): Kather's 224-input layer1 in train mode at an odd batch >= 21
    ("fwd", 1, (21, 56, 56, 64, 64, 3, 1, 1), "in_scale stats", "sslcr::conv_igemm_kernel<unsigned short, 128, 64>", None),
    ("fwd", 1, (21, 56, 56, 64, 128, 3, 1, 1), "in_scale stats", "sslcr::conv_igemm_kernel<unsigned short, 128, 128>", None),
    ("fwd", 0, (21, 56, 56, 64, 64, 3, 1, 1), "in_scale stats", "sslcr::conv_igemm_kernel<float, 128, 64>", None),
    ("fwd", 0, (21, 56, 56, 32, 128, 3, 1, 1), "in_scale stats", "sslcr::conv_igemm_kernel<float, 128, 128>", None),
    # the 3x3 / 2 forward as a single launch (the s2pair rows reach these instances only through an equal-bits comparison)
    ("fwd", 1, (2, 64, 64, 64, 128, 3, 2, 1), "stats", "sslcr::conv_s2_kernel<false, false>", None),
    ("fwd", 1, (2, 64, 64, 64, 128, 3, 2, 1), "bias relu", "sslcr::conv_s2_kernel<false, true>", None),
    ("wgrad", 1, (2, 8, 8, 64, 128, 3, 1, 1), "", "sslcr::wgrad3x3_halo_kernel<unsigned short, 8, 2>", None),
    ("wgrad", 1, (2, 8, 8, 64, 128, 3, 1, 1), "in_scale", "sslcr::wgrad3x3_halo_kernel<unsigned short, 8, 2>", None),
    ("wgrad", 1, (3, 9, 11, 64, 64, 3, 2, 1), "", "sslcr::wgrad_kernel<unsigned short, 9, 1>", None),
    ("wgrad", 1, (3, 9, 11, 64, 64, 1, 2, 0), "", "sslcr::wgrad_kernel<unsigned short, 1, 1>", None),
    # ---- the input-gradient forms beside par4: on the DMA gather kernel, on the generic kernel, both dtypes
    # (the plain transposed form at stride 2 has no uniform pixel parity per workgroup: conv_dma_bp refuses it at every size, so the
    # large ragged map runs on the generic kernel too; at stride 1 the DMA kernel takes it from 2048 pixels on)
    ("dgrad_t", 1, (10, 30, 34, 64, 128, 3, 2, 1), "residual", IG, None),
    ("dgrad_t", 0, (10, 30, 34, 64, 128, 3, 2, 1), "residual", IGF, None),
    ("dgrad_t", 1, (3, 30, 34, 64, 128, 3, 1, 1), "residual", "sslcr::conv_dma_kernel<unsigned short, 256, 64>", None),
    ("dgrad_t", 0, (3, 30, 34, 64, 128, 3, 1, 1), "residual", "sslcr::conv_dma_kernel<float, 256, 64>", None),
    ("dgrad_t", 1, (3, 9, 11, 64, 128, 3, 2, 1), "residual", IG, None),
    ("dgrad_t", 0, (3, 9, 11, 64, 128, 3, 2, 1), "residual", IGF, None),
    ("dgrad_t", 1, (2, 16, 16, 64, 64, 3, 1, 1), "residual", IG, None),
    ("dgrad_t", 0, (2, 16, 16, 64, 64, 3, 1, 1), "residual", IGF, None),
    # (each class is bounded with its own reduction length: the taps its mask keeps -- 1, 2, 2, 4 -- times K)
    ("dgrad_parity", 1, (10, 30, 34, 64, 128, 3, 2, 1), "residual", "sslcr::conv_dma_kernel<unsigned short, 256, 64>", None),
    ("dgrad_parity", 0, (10, 30, 34, 64, 128, 3, 2, 1), "residual", "sslcr::conv_dma_kernel<float, 256, 64>", None),
    ("dgrad_parity", 1, (3, 9, 11, 64, 128, 3, 2, 1), "residual", IG, None),
    ("dgrad_parity", 0, (3, 9, 11, 64, 128, 3, 2, 1), "residual", IGF, None),
    ("scatter", 1, (10, 32, 32, 128, 256, 1, 2, 0), "accumulate", "sslcr::conv_dma_kernel<unsigned short, 128, 128>", None),
    ("scatter", 0, (10, 32, 32, 128, 256, 1, 2, 0), "accumulate", "sslcr::conv_dma_kernel<float, 128, 128>", None),
    ("scatter", 1, (2, 8, 8, 128, 256, 1, 2, 0), "accumulate", IG, None),
    ("scatter", 0, (2, 8, 8, 128, 256, 1, 2, 0), "accumulate", IGF, None),
]

UNLAUNCHABLE = {}

# instances with a row that the sweep's grid does not name (its flag sets carry in_scale only beside plain statistics, a mask or a
# residual); found by walking every subset of the flags over the grid's shapes
BEYOND_THE_GRID = (H16 + "128, 2, true, false, false, 16>", H16 + "128, 2, true, false, false, 8>")
