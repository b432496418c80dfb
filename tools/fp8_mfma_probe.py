"""How the scaled 16x16x128 fp8 MFMA sums its 128 products: a probe through the fp8 conv kernel (sslcr_conv2d_fp8).

Only the centre tap of the 3x3 filters is non-zero, so every output element is ONE instruction's worth of products (C = 128) and
eight instructions of zeros.  Channel 0 carries one large product (448 x 256 in quantised units), channels 1 .. 127 products of
about 2^-j x 256 with random signs; every operand is exactly representable in e4m3, the weight scale is 2^8 for every filter, and
bias = -448 takes the large term out again in the fp32 epilogue, so that the bf16 output shows what is left of the small products.
Printed: the error against float64 beyond the bf16 output rounding, in units of 2^-24 x (the large product), with and without the
large product.  The figures recorded in tests/_f64.py (FP8_MFMA_MEASURED_U) come from this script on an MI355X.

    python tools/fp8_mfma_probe.py
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import _f64 as B  # noqa: E402
from ssl_cr_histo_amd import kernels as K  # noqa: E402

DEV = "cuda:0"


def main():
    g = torch.Generator().manual_seed(5)
    shape = (1, 16, 16, 128)

    def signed_significands(size):      # +-(1.000 .. 1.875): the e4m3 significands
        return torch.randint(8, 16, size, generator=g).float() / 8.0 * (torch.randint(0, 2, size, generator=g).float() * 2 - 1)
    for big in (448.0, 0.0):
        for j in (0, 4, 8, 10, 12, 14, 16):
            jx = min(j, 6)                                   # 2^-j split between the activation and the weight side
            x = signed_significands(shape) * 2.0 ** -jx
            x[..., 0] = big
            w = torch.zeros((128, 128, 3, 3))
            w[:, :, 1, 1] = signed_significands((128, 128)) * 2.0 ** -(j - jx) / 2.0
            w[:, 0, 1, 1] = 1.0
            w8, dq, _ = K.pack_conv_fp8(w.to(DEV))
            wq, dq_ref, _ = B.fp8_pack_ref(w)
            xq, _ = B.fp8_activations(x, 1.0)
            assert torch.equal(dq.cpu().double(), dq_ref) and float(dq_ref[0]) == 2.0 ** -8 and torch.equal(xq, x.double())
            y = K.conv2d_fp8(x.to(DEV).to(torch.bfloat16), w8, dq, bias=torch.full((128,), -big, device=DEV)).float().cpu().double()
            acc, _, _ = B.fp8_conv_ref(xq, wq, dq_ref, 1.0)
            want = acc - big
            err = (y - want).abs()
            beyond = (err - B.U_BF16 * want.abs()).clamp_min(0.0)
            unit = B.U * max(big, 1.0)
            print(f"large product {big:5.0f} x 256, small ones 2^-{j:<2d} x 256: mean |want| {float(want.abs().mean()):.3e}, "
                  f"error beyond the bf16 rounding: worst {float(beyond.max()) / unit:8.1f}, mean {float(beyond.mean()) / unit:8.1f} "
                  f"[2^-24 x {max(big, 1.0):g}]")


if __name__ == "__main__":
    main()
