"""Case table of the fp8 (e4m3) forward conv path (data only): conv_fp8.hip through sslcr_conv2d_fp8.

    (shape (N, H, W, C, K), flags, x_scale, name, branch)

shape   N = None: the test derives the batch from the device's compute-unit count (torch.cuda.get_device_properties(0).
        multi_processor_count; the CPU route test takes 256, the fallback of device_cus()) by WALK_N below, so that the persistent
        workgroups walk more than one tile on whatever part runs the suite.  A launch has cus / (K / 128) tile walkers; the walk needs
        more tiles than that, and its work is about cus * 128 * C * 256 * 18 FLOP whatever K is: these are the smallest shapes that walk.
flags   space-separated words the test turns into descriptor fields: in_scale (the producer transform on the load path: XF = true),
        relu_in (in_relu = 1; without it lo_clamp = -448), stats, bias, residual, relu.
x_scale the host x_scale of the launch.  3.0 is the non-power-of-two case: in_scale * xs and dq / xs then round.
name    the instance the launch must be, as rocprofv3 spells it.
branch  the source condition the row exists for, quoted from conv_fp8.hip.
"""

# N = mul * (ceil(cus / div) + add) for the rows with N = None, keyed by (H, W, C, K): (div, add, mul)
WALK_N = {
    (32, 32, 128, 128): (4, 6, 1),
    (16, 16, 256, 256): (2, 5, 1),
    (16, 16, 384, 128): (1, 7, 1),
    (8, 8, 128, 128): (1, 9, 4),
    (8, 8, 256, 512): (4, 3, 4),
}

_SMALL = [
    ((1, 16, 16, 128, 128), "one tile on a grid of cus walkers: 'if (gx > ntiles) gx = ntiles'"),
    ((3, 32, 48, 128, 256), "tiles_w = 3 != tiles_h = 2 in tile_coords ('t % tiles_w; t /= tiles_w; t % tiles_h'); two kout blocks on grid y: 'k0 = blockIdx.y * BKO'"),
    ((2, 16, 16, 512, 128), "four slabs, no walk: 'if (nslabs > 1) set_affine(pslab)' and the 'slab * 256' offset of load_chunk"),
    ((4, 8, 8, 512, 512), "8x8 form ('a.H == 8 && a.W == 8 && a.N % 4 == 0'): one tile of four images, four slabs, four kout blocks"),
]
_WALK = [
    ((None, 32, 32, 128, 128), "walk with one slab: 'my_tiles = (ntiles - blockIdx.x + gridDim.x - 1) / gridDim.x' is 2 on some workgroups and 1 on the rest"),
    ((None, 16, 16, 256, 256), "walk x 2 slabs: 'nst = my_tiles * nslabs', gx = cus / 2"),
    ((None, 16, 16, 384, 128), "walk x 3 slabs: the halo buffer parity 's & 1' differs between consecutive tiles of a workgroup"),
    ((None, 8, 8, 128, 128), "8x8 form walking: 'n0 = (t / tiles_h) * NI' with NI = 4, the 'TW == 16 ? ... :' arms of pbase and the epilogue offsets"),
    ((None, 8, 8, 256, 512), "8x8 form walking, two slabs, gx = cus / 4"),
]
_SETS = ["", "in_scale relu_in stats", "in_scale stats", "bias residual relu", "in_scale relu_in bias residual relu stats"]


def _name(shape, flags):
    return "sslcr::conv3x3_fp8_kernel<%d, %s>" % (16 if shape[1] % 16 == 0 else 8, "true" if "in_scale" in flags.split() else "false")


CASES = [(s, fl, 1.0, _name(s, fl), br) for s, br in _SMALL for fl in _SETS]
CASES += [(s, "in_scale relu_in stats", xs, _name(s, "in_scale"), br + "; 's_scale[c] = a.in_scale[c] * xs' and 'dq = d4[jj] / xs' with xs = %g" % xs)
          for s, br in _SMALL for xs in (0.25, 16.0, 3.0)]
CASES += [(s, fl, 4.0, _name(s, fl), br) for s, br in _WALK for fl in ("in_scale relu_in stats", "bias residual relu")]
