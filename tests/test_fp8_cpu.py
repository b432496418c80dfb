"""CPU-only: the fp8 case table (tests/fp8_cases.py) against the library's routing -- every row maps to exactly its instance and
announces 4 partial rows per tile -- the descriptors the fp8 kernel does not serve, and the argument check that keeps a descriptor
with in_scale but no in_shift from ever reaching a device.  (No device here: N = None rows take 256 compute units, the fallback of
device_cus().)"""
import os

import pytest
import torch

import _fp8 as F8
from fp8_cases import CASES

FAKE = 4096        # a non-NULL pointer for the descriptor fields that select a route (nothing is launched)
CUS = 256


@pytest.fixture(scope="module")
def lib():
    from ssl_cr_histo_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    return _lib.lib()


def desc(shape, flags="", stride=1):
    from ssl_cr_histo_amd import _lib as L
    N, H, W, C, K = shape
    f = F8.flags_of(flags)
    p = lambda k: FAKE if k in f else None      # noqa: E731
    OH, OW = (H + 2 - 3) // stride + 1, (W + 2 - 3) // stride + 1
    d = L.ConvDesc(FAKE, None, FAKE, p("in_scale"), p("in_scale"), p("bias"), p("residual"), p("stats"), N, H, W, C, K, 3, 3, stride, 1,
                   OH, OW, OH, OW, 1, 0, int("relu_in" in f), int("relu" in f), 0, 0, 0, 0, 0)
    return d


def case_id(r):
    return f"{'x'.join(str(v) for v in r[0])}-{r[1].replace(' ', '+') or 'plain'}-xs{r[2]:g}"


def test_table_is_the_one_the_issue_sets():
    """9 shapes; the four small ones with five flag sets at x_scale 1 and the train set at 0.25, 16 and 3; the five walking ones with
    two flag sets at x_scale 4"""
    assert len(CASES) == 4 * (5 + 3) + 5 * 2
    assert len({r[0] for r in CASES}) == 9
    assert {r[2] for r in CASES} == {1.0, 0.25, 16.0, 3.0, 4.0}
    assert {r[3] for r in CASES} == {"sslcr::conv3x3_fp8_kernel<%d, %s>" % (tw, xf) for tw in (16, 8) for xf in ("true", "false")}


@pytest.mark.parametrize("row", CASES, ids=[case_id(r) for r in CASES])
def test_row_maps_to_exactly_its_instance(lib, row):
    shape, flags, _, name, _ = row
    shape = F8.batch(shape, CUS)
    d = desc(shape, flags)
    assert lib.sslcr_conv2d_fp8_kernel_name(d).decode() == name
    assert lib.sslcr_conv2d_fp8_partial_rows(d) == 4 * F8.tiles(shape)
    if row[0][0] is None:      # the rows that exist for the walk do walk; the others do not
        assert F8.tiles(shape) > F8.walkers(shape, CUS)
    else:
        assert F8.tiles(shape) <= F8.walkers(shape, CUS)


@pytest.mark.parametrize("cus", [64, 80, 104, 228, 256, 304])
def test_walking_rows_walk_on_any_part(cus):
    for shape, _, _, _, _ in CASES:
        if shape[0] is None:
            s = F8.batch(shape, cus)
            assert F8.tiles(s) > F8.walkers(s, cus) and (s[1] != 8 or s[0] % 4 == 0), (cus, s)
            assert s[0] * s[1] * s[2] * s[3] * 2 < 1 << 32


UNSERVED = [
    ("six images of 8x8: N % 4", (6, 8, 8, 128, 128), {}),
    ("8x16 map: neither form", (2, 8, 16, 128, 128), {}),
    ("C = 64", (2, 16, 16, 64, 128), {}),
    ("C = 640 > 512", (2, 16, 16, 640, 128), {}),
    ("K = 192", (2, 16, 16, 128, 192), {}),
    ("stride 2", (2, 32, 32, 128, 128), {"stride": 2}),
    ("out_scale set", (2, 16, 16, 128, 128), {"out_scale": FAKE}),
    ("mask_x", (2, 16, 16, 128, 128), {"mask_x": FAKE}),
]


@pytest.mark.parametrize("what, shape, extra", UNSERVED, ids=[u[0].replace(" ", "_") for u in UNSERVED])
def test_unserved_descriptors_report_no_rows_and_no_name(lib, what, shape, extra):
    d = desc(shape, "stats", stride=extra.get("stride", 1))
    for k, v in extra.items():
        if k != "stride":
            setattr(d, k, v)
    assert lib.sslcr_conv2d_fp8_partial_rows(d) == 0, what
    assert lib.sslcr_conv2d_fp8_kernel_name(d) == b"", what
    assert lib.sslcr_conv2d_fp8_partial_rows(None) == 0 and lib.sslcr_conv2d_fp8_kernel_name(None) == b""
    # ... and the served neighbour of each is served: the refusal is the one property varied
    assert lib.sslcr_conv2d_fp8_partial_rows(desc((4, 16, 16, 128, 128), "stats")) == 16


@pytest.mark.skipif(torch.cuda.is_available(), reason="a descriptor that lacks in_shift must never be able to reach a device")
def test_in_scale_without_in_shift_is_refused(lib):
    """the kernel's load path reads a.in_shift[c] whenever in_scale is set: sslcr_conv2d_fp8 refuses the descriptor before any launch"""
    from ssl_cr_histo_amd import _lib as L
    d = desc((1, 16, 16, 128, 128), "in_scale relu_in")
    d.in_shift = None
    q = L.Fp8Desc(FAKE, FAKE, 1.0, None, None)
    assert lib.sslcr_conv2d_fp8(d, q, None) == -1
    assert b"in_shift" in lib.sslcr_last_error()
    d.in_scale = None
    d.x = None                 # (the neighbouring check still answers first for its own case)
    assert lib.sslcr_conv2d_fp8(d, q, None) == -1
    assert b"null tensor" in lib.sslcr_last_error()
    assert lib.sslcr_fp8_scale_update(None, 4, None) == -1
