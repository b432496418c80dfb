"""The library's SSLCR_* environment switches and the routes behind them (data only).  The library's own table of them is
kernels.switches(); all but two rows are read once per process, so a test of one sets it in the environment of a fresh child process
(tests/test_switch_routes_cpu.py, tests/test_switch_routes_gpu.py).

ROUTING                switch -> the value that turns its default off, for the switches that change which instance the router answers.
SWITCH_ROUTES          switch -> rows of the shape of kernel_routes.ROUTES, (op, dtype, shape, flags, name, tail); `name` is what the
                       router answers WITH the switch set, the trailing comment names the instance that serves the descriptor by
                       default.  One row per (default -> switched) transition, at the smallest descriptor of tools/route_sweep.py's
                       grid that makes it: without any one row the closure of tests/test_switch_routes_cpu.py fails.
LARGER_ROUTES          rows of the same shape beside the table (see there).
ONLY_BEHIND_A_SWITCH   the instances that the default routing answers for no descriptor: every flag set that reaches one has a row.
REFUSED                rows that the switched router names and the launcher refuses (the route plan's `ok`), with the refusing line.
FORMS, ENGINE          switch -> value, for the switches that select a kernel form without changing a routed name, and the engine's.
COVERED_ELSEWHERE      switch -> the test that sets it.
OUT_OF_SCOPE           switch -> why no test sets it.
"""
from kernel_routes import H16, IG, Q, QF

ROUTING = {"SSLCR_PP64": "0", "SSLCR_H16_TW8": "0", "SSLCR_H16_RAW": "0", "SSLCR_S2": "0", "SSLCR_S2D": "0", "SSLCR_S2W": "0",
           "SSLCR_WG_DMA": "0", "SSLCR_WGRAD_WIDE": "0"}

# the resident-filter-bank (WR = true) forms of the h16 family: bf16 64 -> 64 without the ping-pong kernel
WR = H16 + "64, 2, false, true, false, 16>"
WR_XF = H16 + "64, 2, true, true, false, 16>"
WR_S = "sslcr::conv3x3_h16s_kernel<unsigned short, 64, 2, true, 16>"
ONLY_BEHIND_A_SWITCH = (WR, WR_XF, WR_S)

PP = (1, 16, 16, 64, 64, 3, 1, 1)            # one tile, one item, one workgroup
PP_WALK = (320, 16, 16, 64, 64, 3, 1, 1)     # 320 items on 256 workgroups: the bank is loaded once and serves a second item
L4 = (4, 8, 8, 64, 128, 3, 1, 1)             # one four-image tile; on conv3x3_halo256 it runs as the 64-kout tail launch alone
L4_HEAD = (320, 8, 8, 64, 256, 3, 1, 1)      # 80 tiles x 2 kout blocks = 160 items > half the CUs: every item is a 128-kout one
Q128, Q128F, Q64, Q64F = Q + "8, 128, 2, false>", QF + "8, 128, 2, false>", Q + "8, 64, 2, false>", QF + "8, 64, 2, false>"
L2 = (1, 16, 16, 64, 128, 3, 1, 1)
S2 = (2, 64, 64, 64, 128, 3, 2, 1)
DMA128, DMA256 = "sslcr::conv_dma_kernel<unsigned short, 128, 128>", "sslcr::conv_dma_kernel<unsigned short, 256, 64>"
WG92, WG91 = "sslcr::wgrad_kernel<unsigned short, 9, 2>", "sslcr::wgrad_kernel<unsigned short, 9, 1>"
WH16, WH8 = "sslcr::wgrad3x3_halo_kernel<unsigned short, 16, 2>", "sslcr::wgrad3x3_halo_kernel<unsigned short, 8, 2>"

SWITCH_ROUTES = {
    "SSLCR_PP64": [
        ("fwd", 1, PP, "", WR, None),                                 # conv3x3_pp64_kernel<false, 0>
        ("fwd", 1, PP, "bias", WR, None),                             # conv3x3_pp64_kernel<false, 0>
        ("fwd", 1, PP, "bias relu", WR, None),                        # conv3x3_pp64_kernel<false, 0>
        ("fwd", 1, PP, "relu", WR, None),                             # conv3x3_pp64_kernel<false, 0>
        ("fwd", 1, PP, "stats", WR, None),                            # conv3x3_pp64_kernel<false, 0>
        ("fwd", 1, PP, "stats bias", WR, None),                       # conv3x3_pp64_kernel<false, 0>
        ("fwd", 1, PP, "residual", WR, None),                         # conv3x3_pp64_kernel<false, 1>
        ("fwd", 1, PP, "bias residual relu", WR, None),               # conv3x3_pp64_kernel<false, 1>
        ("fwd", 1, PP, "mask stats", WR, None),                       # conv3x3_pp64_kernel<false, 2>
        ("fwd", 1, PP, "in_scale stats", WR_XF, None),                # conv3x3_pp64_kernel<true, 0>
        ("fwd", 1, PP, "out_scale bias", WR_S, None),                 # conv3x3_pp64_kernel<false, 0>
        ("fwd", 1, PP, "out_scale bias relu", WR_S, None),            # conv3x3_pp64_kernel<false, 0>
        ("fwd", 1, PP, "out_scale bias residual relu", WR_S, None),   # conv3x3_pp64_kernel<false, 1>
    ],
    "SSLCR_H16_TW8": [
        ("fwd", 0, L4, "bias residual relu", Q128F, Q64F),            # conv3x3_h16_kernel<float, 128, 2, false, false, false, 8>
        ("fwd", 0, L4, "in_scale stats", Q128F, Q64F),                # conv3x3_h16_kernel<float, 128, 2, true, false, false, 8>
        ("fwd", 1, L4, "bias residual relu", Q128, Q64),              # conv3x3_h16_kernel<unsigned short, 128, 2, false, false, false, 8>
        ("fwd", 1, L4, "stats", Q128, Q64),                           # conv3x3_h16_kernel<unsigned short, 128, 2, false, false, true, 8>
        ("fwd", 1, L4, "in_scale stats", Q128, Q64),                  # conv3x3_h16_kernel<unsigned short, 128, 2, true, false, true, 8>
        ("fwd", 0, L4, "out_scale bias residual relu", Q128F, Q64F),  # conv3x3_h16s_kernel<float, 128, 2, false, 8>
        ("fwd", 1, L4, "out_scale bias residual relu", Q128, Q64),    # conv3x3_h16s_kernel<unsigned short, 128, 2, false, 8>
    ],
    "SSLCR_H16_RAW": [      # statistics through the general output stage
        ("fwd", 1, L2, "stats", H16 + "128, 2, false, false, false, 16>", None),         # <..., false, false, true, 16>
        ("fwd", 1, L4, "stats", H16 + "128, 2, false, false, false, 8>", None),          # <..., false, false, true, 8>
        ("fwd", 1, L2, "in_scale stats", H16 + "128, 2, true, false, false, 16>", None),  # <..., true, false, true, 16>
        ("fwd", 1, L4, "in_scale stats", H16 + "128, 2, true, false, false, 8>", None),   # <..., true, false, true, 8>
    ],
    "SSLCR_S2": [           # the 3x3 / 2 forward on the DMA gather kernel, at shapes it never sees by default
        ("fwd", 1, S2, "stats", DMA128, None),                        # conv_s2_kernel<false, false>
        ("fwd", 1, S2, "bias relu", DMA128, None),                    # conv_s2_kernel<false, true>
    ],
    "SSLCR_S2D": [          # the stride-2 input gradient, four parity classes in one launch (par4)
        ("dgrad", 1, (2, 64, 64, 128, 64, 3, 2, 1), "", DMA128, None),       # conv_s2d_kernel
        ("dgrad", 1, (2, 64, 64, 64, 64, 3, 2, 1), "", DMA256, None),        # conv_s2d_kernel
        ("dgrad", 1, (1, 32, 32, 64, 64, 3, 2, 1), "", IG, None),            # conv_s2d_kernel
    ],
    "SSLCR_S2W": [
        ("wgrad", 1, (1, 32, 32, 64, 128, 3, 2, 1), "", WG92, None),         # wgrad_s2_kernel<16>
        ("wgrad", 1, (1, 16, 16, 64, 128, 3, 2, 1), "", WG92, None),         # wgrad_s2_kernel<8>
    ],
    "SSLCR_WG_DMA": [
        ("wgrad", 1, (3, 32, 32, 64, 128, 3, 1, 1), "", WH16, None),         # wgrad3x3_dma_kernel<16, false>
        ("wgrad", 1, (3, 32, 32, 64, 128, 3, 1, 1), "in_scale", WH16, None),  # wgrad3x3_dma_kernel<16, true>
        ("wgrad", 1, (2, 56, 56, 64, 128, 3, 1, 1), "", WH8, None),          # wgrad3x3_dma_kernel<8, false>
        ("wgrad", 1, (2, 56, 56, 64, 128, 3, 1, 1), "in_scale", WH8, None),  # wgrad3x3_dma_kernel<8, true>
    ],
    "SSLCR_WGRAD_WIDE": [
        ("wgrad", 1, (1, 7, 7, 64, 128, 1, 2, 0), "", "sslcr::wgrad_kernel<unsigned short, 1, 1>", None),      # wgrad_kernel<unsigned short, 1, 2>
        ("wgrad", 1, (1, 7, 7, 64, 128, 3, 2, 1), "", WG91, None),           # wgrad_kernel<unsigned short, 9, 2>
    ],
}

# Larger descriptors of the grid beside the table: each makes a transition that SWITCH_ROUTES already holds, at a size where the
# instance can go wrong in a way its smallest descriptor cannot show.
LARGER_ROUTES = {
    "SSLCR_PP64": [         # 320 items on 256 workgroups: the resident bank is loaded once and serves a workgroup's second item
        ("fwd", 1, PP_WALK, "stats", WR, None),                                # conv3x3_pp64_kernel<false, 0>
        ("fwd", 1, PP_WALK, "in_scale stats", WR_XF, None),                    # conv3x3_pp64_kernel<true, 0>
        ("fwd", 1, PP_WALK, "out_scale bias residual relu", WR_S, None),       # conv3x3_pp64_kernel<false, 1>
    ],
    "SSLCR_H16_TW8": [      # 160 items: the named 128-kout instance launches (at N = 4 only its 64-kout tail does)
        ("fwd", 0, L4_HEAD, "in_scale stats", Q128F, None),                    # conv3x3_h16_kernel<float, 128, 2, true, false, false, 8>
        ("fwd", 1, L4_HEAD, "stats", Q128, None),                              # conv3x3_h16_kernel<unsigned short, 128, 2, false, false, true, 8>
        ("fwd", 1, L4_HEAD, "in_scale stats", Q128, None),                     # conv3x3_h16_kernel<unsigned short, 128, 2, true, false, true, 8>
        ("fwd", 1, L4_HEAD, "out_scale bias residual relu", Q128, None),       # conv3x3_h16s_kernel<unsigned short, 128, 2, false, 8>
    ],
    "SSLCR_S2": [
        ("fwd", 1, S2, "out_scale bias relu", DMA128, None),                   # conv_s2_kernel<false, true>
    ],
}

# conv_plan: "if (a.par4) ok = false" on the generic kernel -- the one-launch parity form exists in the DMA-gather kernels only; the
# engine reads par4_one_launch and runs the four classes one by one there (the dgrad_parity rows of kernel_routes.ROUTES)
REFUSED = {("dgrad", 1, (1, 32, 32, 64, 64, 3, 2, 1), "", IG, None): "conv_route.cpp: the generic kernel has no one-launch parity form"}

FORMS = {"SSLCR_GEMM_LDS": "0", "SSLCR_STEM_POOL_FORM": "1", "SSLCR_POOL_BANDS": "1", "SSLCR_WG_STAGGER": "0"}
ENGINE = {"SSLCR_YBITS": "0", "SSLCR_BN_PAIR_G": "0"}

COVERED_ELSEWHERE = {
    "SSLCR_SEGMENTS": "tests/test_engine_gpu2.py::test_triplet_branches_as_segments_equal_pass_by_pass",
    "SSLCR_BN_PAIR": "tests/test_engine_gpu2.py::test_bn_backward_pair_equals_the_separate_passes",
    "SSLCR_FUSE_STEM_BWD": "tests/test_engine_gpu2.py::test_fused_stem_backward_is_the_same_step",
    "SSLCR_BN_ONE_LAUNCH": "tests/test_kernels_gpu.py::test_bn_finalize_one_launch_same_bits",
    "SSLCR_COMM_SELFTEST": "tests/test_engine_gpu.py::test_collective_code_path_selftest_world1",
}
OUT_OF_SCOPE = {
    "SSLCR_BN_REPEAT": "measurement only: it repeats the BatchNorm launches, which changes the running statistics by design",
    "SSLCR_EW_CAP": "the suite's above-the-cap rows derive their sizes from the default cap: a second cap is a second table",
    "SSLCR_UNFOLD_EVAL": "0 is a different, documented accuracy regime: it belongs with the bf16 yardsticks",
    "SSLCR_STEM_POOL": "0 falls back to the stem and pool kernels that test_stem_f64 / test_pool_f64 bound at the same shapes",
}
