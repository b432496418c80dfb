"""CPU-only: the host logic of gradient accumulation (library version 9) -- how a loader batch is cut into micro-batches, the
``args.micro_batches`` default, and the two new entry points' declarations and argument checks."""
import os
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from ssl_cr_histo_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    from ssl_cr_histo_amd import engine  # noqa: F401  registers engine signatures
    return _lib.lib()


def test_micro_ranges_is_shard_range():
    """a micro-batch is a shard in time: the same contiguous cut as the ranks', covering [0, n) without gaps, remainders to the lowest"""
    from ssl_cr_histo_amd import steps
    from ssl_cr_histo_amd.dist import shard_range
    for n in range(1, 13):
        for k in range(1, n + 1):
            r = steps.micro_ranges(n, k)
            assert r == [shard_range(n, j, k) for j in range(k)]
            assert len(r) == k and r[0][0] == 0 and r[-1][1] == n
            assert all(a[1] == b[0] for a, b in zip(r, r[1:]))
            sizes = [hi - lo for lo, hi in r]
            assert min(sizes) >= 1 and sizes == sorted(sizes, reverse=True) and max(sizes) - min(sizes) <= 1
            assert sizes.count(max(sizes)) == (n % k or k)


@pytest.mark.parametrize("n,k", [(1, 2), (3, 4), (5, 12), (4, 0), (4, -1)])
def test_micro_ranges_refuses_empty_micro_batches(n, k):
    from ssl_cr_histo_amd import steps
    with pytest.raises(ValueError) as e:
        steps.micro_ranges(n, k)
    assert str(n) in str(e.value) and str(k) in str(e.value)


def test_micro_batches_defaults_to_one():
    from ssl_cr_histo_amd import steps
    assert steps._micro_k(types.SimpleNamespace(lambda_u=1.0)) == 1
    assert steps._micro_k(types.SimpleNamespace(micro_batches=None)) == 1
    assert steps._micro_k(types.SimpleNamespace(micro_batches=1)) == 1
    assert steps._micro_k(types.SimpleNamespace(micro_batches=4)) == 4


def test_the_two_entry_points_are_declared():
    """include/sslcr.h declares both (tests/test_abi_cpu.py holds exports == header == ctypes signatures), with their prototypes"""
    import re
    from ssl_cr_histo_amd import build
    names = build.header_symbols()
    assert "sslcr_grad_accumulate" in names and "sslcr_net_set_grad_accumulate" in names
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "sslcr.h")).read(), flags=re.S)
    flat = " ".join(src.split())
    assert "int sslcr_grad_accumulate(float* dst, const float* src, size_t n, void* stream);" in flat
    assert "int sslcr_net_set_grad_accumulate(sslcr_net* net, int on);" in flat


def test_version_and_argument_checks(lib):
    """argument checks run before any device work"""
    import ctypes as C
    assert lib.sslcr_version() >= 9
    assert lib.sslcr_net_set_grad_accumulate(None, 1) == -1
    assert b"null" in lib.sslcr_last_error()
    assert lib.sslcr_grad_accumulate(None, None, 4, None) == -1
    assert b"null" in lib.sslcr_last_error()
    assert lib.sslcr_grad_accumulate(C.c_void_p(4098), C.c_void_p(4096), 4, None) == -1          # a base that is not 4-byte aligned
    assert b"alignment" in lib.sslcr_last_error()
    assert lib.sslcr_grad_accumulate(None, None, 0, None) == 0                                   # n = 0: nothing to do, nothing launched
