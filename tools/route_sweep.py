#!/usr/bin/env python3
"""CPU-only dump of the library's routing: tools/route_sweep.py --lib PATH > dump.txt.  Walks a fixed grid of conv and weight-gradient
descriptors in a fixed order and prints, per descriptor and dtype, what sslcr_conv2d_kernel_name / _partial_rows / _segments_ok /
_s2_pair_ok and sslcr_conv2d_wgrad_kernel_name answer.  Nothing is launched.  Two builds route alike where their dumps are identical
(one process per library: the routing caches its switches in statics); the counts of distinct names go to stderr.  Rows are never
asked for with seg_images > N (a library from before the route plan divides by zero there).  walk() is the grid itself:
tests/test_kernel_routes_cpu.py walks it too, and asks that every name it answers has a row in tests/kernel_routes.py."""
import argparse
import ctypes as C
import itertools
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ssl_cr_histo_amd import _lib as L  # noqa: E402

FAKE = 4096        # a non-NULL pointer for the descriptor fields that select a route
NS = (1, 2, 3, 4, 5, 6, 8, 33, 128, 320, 640)
MAPS = ((7, 7), (8, 8), (9, 11), (14, 14), (16, 16), (28, 28), (30, 34), (32, 32), (56, 56), (64, 64), (8, 16), (16, 8))
CK = ((64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 512), (512, 512), (64, 256), (128, 64), (32, 64), (64, 512))
RSP = ((3, 1, 1), (3, 2, 1), (1, 2, 0), (1, 1, 0))
FLAGS = ("", "stats", "in_scale stats", "bias", "bias relu", "bias residual relu", "out_scale bias", "out_scale bias relu",
         "out_scale bias residual relu", "mask stats", "in_scale mask stats", "residual", "in_scale residual", "stats bias", "relu", "accumulate")
SEGS = (0, 1, 2, 4)


def conv_desc(N, H, W, C, K, R, stride, pad, flags, seg):
    f = flags.split()
    p = lambda k: FAKE if k in f else None      # noqa: E731
    PH, PW = (H + 2 * pad - R) // stride + 1, (W + 2 * pad - R) // stride + 1
    d = L.ConvDesc(FAKE, FAKE, FAKE, p("in_scale"), p("in_scale"), p("bias"), p("residual"), p("stats"), N, H, W, C, K, R, R, stride, pad,
                   PH, PW, PH, PW, 1, 0, int("in_scale" in f), int("relu" in f), int("accumulate" in f), 0, 0, 0, 0)
    d.out_scale = p("out_scale")
    if "mask" in f:
        d.mask_x = d.mask_scale = d.mask_shift = d.mask_mean = FAKE
    d.seg_images, d.seg_stride = seg, C if seg else 0
    return d


def dgrad_descs(N, H, W, C, K):
    """the stride-2 3x3 input gradient as the engine asks for it: x = dY [N, H/2, W/2, K]; plain, par4, one parity class with its taps"""
    oh, ow = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    for form in ("plain", "par4", "parity"):
        d = L.ConvDesc(FAKE, FAKE, FAKE, None, None, None, None, None, N, oh, ow, K, C, 3, 3, 2, 1, H, W, H, W, 1, 1, 0, 0, 0, 0, 0, 0, 0)
        if form != "plain":
            d.pix_mul, d.PH, d.PW = 2, H // 2, W // 2
        if form == "par4":
            d.par4 = 1
        if form == "parity":
            d.pix_off_h = d.pix_off_w = 1
            d.tap_mask = 0b101000101
        yield form, d


def walk():
    """the grid in its fixed order -> (kind, tag, descriptor, pair, size): kind "conv" (the public conv descriptors), "dgrad" (the
    stride-2 input-gradient forms) or "wgrad"; tag: the descriptor as the dump prints it; pair: the 1x1 / 2 descriptor that
    sslcr_conv2d_s2_pair_ok is asked about beside a 3x3 / 2 one, else None; size: a measure to order descriptors by (multiply-adds,
    then the number of flags).  Every descriptor is asked for both dtypes, 0 then 1."""
    for N, (H, W), (Cc, K), (R, s, pad) in itertools.product(NS, MAPS, CK, RSP):
        shape = f"{N}x{H}x{W} {Cc}->{K} k{R}s{s}p{pad}"
        OH, OW = (H + 2 * pad - R) // s + 1, (W + 2 * pad - R) // s + 1
        macs = N * OH * OW * R * R * Cc * K
        for flags, seg in itertools.product(FLAGS, SEGS):
            if seg > N:
                continue
            d = conv_desc(N, H, W, Cc, K, R, s, pad, flags, seg)
            pair = conv_desc(N, H, W, Cc, K, 1, 2, 0, flags.replace("relu", ""), seg) if (R, s) == (3, 2) else None
            yield "conv", f"conv {shape} [{flags}] seg={seg}", d, pair, (macs, len(flags.split()) + (seg > 0))
        if (R, s) == (3, 2):
            for form, d in dgrad_descs(N, H, W, Cc, K):
                yield "dgrad", f"dgrad {shape} {form}", d, None, (macs, 0)
        for xf, seg in itertools.product((None, FAKE), SEGS):
            w = L.WgradDesc(FAKE, FAKE, FAKE, xf, xf, int(bool(xf)), N, H, W, Cc, K, R, R, s, pad, OH, OW, seg, Cc if seg else 0)
            yield "wgrad", f"wgrad {shape} xf={int(bool(xf))} seg={seg}", w, None, (macs, int(bool(xf)) + (seg > 0))


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--lib", required=True)
    ap.add_argument("--switched", action="store_true", help="dump the routes under the SSLCR_* variables that are set (two builds under one switch)")
    args = ap.parse_args()
    set_ = sorted(k for k in os.environ if k.startswith("SSLCR_"))
    if set_ and not args.switched:
        sys.exit(f"unset {set_}: the routing reads its switches once into statics, so this dump would not be the default routes")
    lib = C.CDLL(args.lib)
    for fn in ("sslcr_conv2d_kernel_name", "sslcr_conv2d_partial_rows", "sslcr_conv2d_segments_ok", "sslcr_conv2d_s2_pair_ok",
               "sslcr_conv2d_wgrad_kernel_name"):
        getattr(lib, fn).restype, getattr(lib, fn).argtypes = L.SIGNATURES[fn]
    out, cnames, wnames = [], set(), set()
    for kind, tag, d, pair, _ in walk():
        for dt in (0, 1):
            if kind == "wgrad":
                name = lib.sslcr_conv2d_wgrad_kernel_name(dt, d).decode()
                wnames.add(name)
                out.append(f"{tag} dt={dt} | {name}")
                continue
            name = lib.sslcr_conv2d_kernel_name(dt, d).decode()
            cnames.add(name)
            pok = lib.sslcr_conv2d_s2_pair_ok(dt, d, pair) if pair is not None else "-"
            out.append(f"{tag} dt={dt} | {name} rows={lib.sslcr_conv2d_partial_rows(d)} seg={lib.sslcr_conv2d_segments_ok(dt, d)} pair={pok}")
    sys.stdout.write("\n".join(out) + "\n")
    print(f"{len(out)} lines, {len(cnames)} conv names, {len(wnames)} wgrad names", file=sys.stderr)


if __name__ == "__main__":
    main()
