"""The rows of the float64 step replay (tests/test_backward_replay_gpu.py) and, per (row, block), the FORM WORD the engine must report
through sslcr_net_debug_tensor's flags: which of its forms each stage of the block takes.  Computed on the CPU from the router's query
entries (sslcr_conv2d_kernel_name, sslcr_conv2d_partial_rows, sslcr_conv2d_segments_ok, sslcr_conv2d_s2_pair_ok,
sslcr_conv2d_wgrad_kernel_name), with the descriptors block_plan / Backward::enter of csrc/engine.cpp build; nothing is launched.

Two decisions have no query entry and are restated here from the source:
  * seg_bn: every unsharded, unprofiled multi-pass backward (Backward::enter: no dtype and no shape enters it) -- fp32 TripletNets included;
  * the paired BatchNorm backward (bn_bwd_pair_ok): bn2 and the projection's BatchNorm of one pass, i.e. a projection block whose
    BatchNorm backward does not run as segments."""
import os
import re

FAKE = 4096        # a non-NULL pointer for the descriptor fields that select a route

# bits of the form word (include/sslcr.h)
MASK, SEG_BN, SEG_DG, C2_BATCHED, BN_PAIR, PAR4_ONE, FWD_SEG, FWD_PAIR = (1 << b for b in range(8))
BIT_NAMES = ("mask", "seg_bn", "seg_dg", "c2_batched", "bn_pair", "par4_one", "fwd_seg", "fwd_pair")

BLOCK_CFG = ((64, 64, 1), (64, 64, 1), (64, 128, 2), (128, 128, 1), (128, 256, 2), (256, 256, 1), (256, 512, 2), (512, 512, 1))

# key -> (dtype name, TripletNet?, images per pass, H = W)
ROWS = {
    "A": ("bf16", True, 12, 256),          # segments in all blocks
    "B": ("bf16", True, 4, 128),           # pass-by-pass forward, segmented backward
    "C": ("fp32", True, 2, 64),            # no conv takes segments
    "D-bf16": ("bf16", False, 8, 256),     # the production composition: step_ssl_cr, 2 labelled + 6 unlabelled images
    "D-fp32": ("fp32", False, 8, 256),
    "E-bf16": ("bf16", False, 4, 224),     # 56 / 28 / 14 / 7 maps: ragged parity dgrad, generic forms
    "E-fp32": ("fp32", False, 4, 224),
}


def out_dim(h, k, s, p):
    return (h + 2 * p - k) // s + 1


def block_dims(hw):
    """-> [(xh, oh)] per block: input and output side of the (square) maps"""
    h = out_dim(out_dim(hw, 7, 2, 3), 3, 2, 1)
    dims = []
    for _, _, s in BLOCK_CFG:
        o = out_dim(h, 3, s, 1)
        dims.append((h, o))
        h = o
    return dims


def word_str(w):
    return "+".join(n for b, n in enumerate(BIT_NAMES) if w >> b & 1) or "-"


def _conv(N, H, C, K, R, stride, pad, *, pro=False, seg=0, seg_stride=0, mask=False, stats=True):
    from ssl_cr_histo_amd import _lib as L
    P = out_dim(H, R, stride, pad)
    xf = FAKE if pro else None
    d = L.ConvDesc(FAKE, FAKE, FAKE, xf, xf, None, None, FAKE if stats else None, N, H, H, C, K, R, R, stride, pad, P, P, P, P, 1, 0,
                   int(pro), 0, 0, 0, 0, 0, 0)
    if mask:
        d.mask_x = d.mask_scale = d.mask_shift = d.mask_mean = FAKE
    if seg:
        d.seg_images, d.seg_stride = seg, seg_stride
    return d


def _tile16(name):
    # ConvRoute::H16 / PP64 (engine.cpp: tile16)
    return name.startswith("sslcr::conv3x3_h16") or name.startswith("sslcr::conv3x3_pp64") or name.startswith("sslcr::conv_pp64")


def _wgrad_halo_tw(name):
    """wgrad_halo_tw as the instance name spells it: wgrad3x3_halo_kernel<T, TW, KH>, wgrad3x3_dma_kernel<TW, ...>; 0: another family"""
    m = re.match(r"sslcr::wgrad3x3_halo_kernel<[^,]+, (\d+),", name) or re.match(r"sslcr::wgrad3x3_dma_kernel<(\d+),", name)
    return int(m.group(1)) if m else 0


def expected_forms(lib, key):
    """-> the eight form words of row `key`"""
    from ssl_cr_histo_amd import _lib as L
    dtype, triplet, N, hw = ROWS[key]
    dt = 1 if dtype == "bf16" else 0
    npass = 3 if triplet else 1
    dims = block_dims(hw)
    stride_floats = 20 * 4 * 512          # alloc_passes: the saved statistics of one pass

    def fwd(i, nseg):
        """block_plan -> (seg_ok, paired)"""
        cin, cout, s = BLOCK_CFG[i]
        xh, oh = dims[i]
        seg = N if nseg > 1 else 0
        c1 = _conv(nseg * N, xh, cin, cout, 3, s, 1, seg=seg)
        c2 = _conv(nseg * N, oh, cout, cout, 3, 1, 1, pro=True, seg=seg, seg_stride=stride_floats)
        r1, r2 = lib.sslcr_conv2d_partial_rows(c1), lib.sslcr_conv2d_partial_rows(c2)
        ok = bool(lib.sslcr_conv2d_segments_ok(dt, c1) and lib.sslcr_conv2d_segments_ok(dt, c2)) and r1 % nseg == 0 and r2 % nseg == 0
        paired = False
        if s == 2:
            ds = _conv(nseg * N, xh, cin, cout, 1, 2, 0, seg=seg)
            paired = bool(lib.sslcr_conv2d_s2_pair_ok(dt, c1, ds))
            rd = r1 if paired else lib.sslcr_conv2d_partial_rows(ds)
            ok = ok and bool(lib.sslcr_conv2d_segments_ok(dt, ds)) and rd % nseg == 0
        return ok, paired

    fwd_seg = triplet and dt == 1 and all(fwd(i, 3)[0] for i in range(8))       # segments_servable
    words = []
    for i, (cin, cout, s) in enumerate(BLOCK_CFG):
        xh, oh = dims[i]
        w = 0
        if fwd_seg:
            w |= FWD_SEG
        if fwd(i, npass if fwd_seg else 1)[1]:
            w |= FWD_PAIR
        # Backward::enter
        seg_bn = npass > 1
        seg_dg = c2_batched = False
        if npass > 1:
            q = L.WgradDesc(FAKE, FAKE, FAKE, FAKE, FAKE, 1, N * npass, oh, oh, cout, cout, 3, 3, 1, 1, oh, oh, N, stride_floats)
            tw = _wgrad_halo_tw(lib.sslcr_conv2d_wgrad_kernel_name(dt, q).decode())
            c2_batched = tw != 0 and (tw == 16 or N % 2 == 0)
            m = _conv(N * npass, oh, cout, cout, 3, 1, 1, mask=True, seg=N, seg_stride=stride_floats, stats=False)
            seg_dg = _tile16(lib.sslcr_conv2d_kernel_name(dt, m).decode()) and bool(lib.sslcr_conv2d_segments_ok(dt, m)) and \
                lib.sslcr_conv2d_partial_rows(m) % npass == 0
        m1 = _conv(N, oh, cout, cout, 3, 1, 1, mask=True, stats=False)
        if seg_dg or _tile16(lib.sslcr_conv2d_kernel_name(dt, m1).decode()):
            w |= MASK
        w |= (SEG_BN if seg_bn else 0) | (SEG_DG if seg_dg else 0) | (C2_BATCHED if c2_batched else 0)
        if s == 2 and not seg_bn:
            w |= BN_PAIR
        if s == 2 and xh % 2 == 0:
            # the par4 descriptor of Backward::input_grad: x = dRaw1 [., oh, oh, cout], pixel space = the input's parity planes
            q4 = L.ConvDesc(FAKE, FAKE, FAKE, None, None, None, None, None, N * npass, oh, oh, cout, cin, 3, 3, 2, 1, xh // 2, xh // 2, xh, xh,
                            1, 1, 0, 0, 0, 2, 0, 0, 0)
            q4.par4 = 1
            name = lib.sslcr_conv2d_kernel_name(dt, q4).decode()
            # conv_dma serves it -- itself, or conv_s2d in its place (bf16); fp32 never takes conv_s2d, so there the name says which
            one = "conv_dma" in name or ("conv_s2d" in name and "conv_dma" in lib.sslcr_conv2d_kernel_name(0, q4).decode())
            if one:
                w |= PAR4_ONE
        words.append(w)
    return words


def stats_rows(lib, key, i, word):
    """-> (conv1, conv2, projection | None): the statistics rows PER PASS that block i's forward convs hand the finalize, in the form
    `word` says the forward took (block_plan)"""
    _, _, N, hw = ROWS[key]
    nseg = 3 if word & FWD_SEG else 1
    cin, cout, s = BLOCK_CFG[i]
    xh, oh = block_dims(hw)[i]
    seg = N if nseg > 1 else 0
    r1 = lib.sslcr_conv2d_partial_rows(_conv(nseg * N, xh, cin, cout, 3, s, 1, seg=seg))
    r2 = lib.sslcr_conv2d_partial_rows(_conv(nseg * N, oh, cout, cout, 3, 1, 1, pro=True, seg=seg, seg_stride=20 * 4 * 512))
    rd = None
    if s == 2:
        rd = r1 if word & FWD_PAIR else lib.sslcr_conv2d_partial_rows(_conv(nseg * N, xh, cin, cout, 1, 2, 0, seg=seg))
    return r1 // nseg, r2 // nseg, None if rd is None else rd // nseg


def closure_gaps(table):
    """table: {key: [8 words]} -> the bits that are not both on in some (row, block) and off in another"""
    words = [w for ws in table.values() for w in ws]
    return [n for b, n in enumerate(BIT_NAMES) if not (any(w >> b & 1 for w in words) and any(not (w >> b & 1) for w in words))]


# what the rows were chosen for: (key, bit, blocks where it is on).  A routing change that moves one of these fails on the CPU
STATED = (
    ("A", FWD_SEG, range(8)), ("A", SEG_BN, range(8)), ("A", SEG_DG, range(6)), ("A", C2_BATCHED, range(8)), ("A", FWD_PAIR, (2, 4)),
    ("B", FWD_SEG, ()), ("B", SEG_BN, range(8)), ("B", SEG_DG, range(4)),
    ("C", FWD_SEG, ()), ("C", SEG_DG, ()), ("C", FWD_PAIR, ()), ("C", C2_BATCHED, range(4)),
    ("D-bf16", SEG_BN, ()), ("D-bf16", BN_PAIR, (2, 4, 6)), ("D-bf16", PAR4_ONE, (2, 4)), ("D-bf16", MASK, range(6)),
    ("D-bf16", FWD_PAIR, (2, 4)), ("D-fp32", FWD_PAIR, ()), ("D-fp32", BN_PAIR, (2, 4, 6)),
    ("E-bf16", FWD_PAIR, ()), ("E-fp32", FWD_PAIR, ()), ("E-bf16", PAR4_ONE, (2,)), ("E-fp32", PAR4_ONE, (2,)), ("E-bf16", MASK, ()),
)

if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from ssl_cr_histo_amd import _lib
    for k in ROWS:
        print(k, [word_str(w) for w in expected_forms(_lib.lib(), k)])
