"""CPU-only: the relocating shim of tests/_arena.py proved on the host.  Its logic does not depend on the device, so here the tensors are
CPU tensors and the "kernels" are ctypes.memmove / memset on the pointers the patched _lib.ptr returned; and the alignment table the
shim places by is held to the words of include/sslcr.h."""
import ctypes as C
import math

import pytest
import torch

import _arena as A
import _f64 as B
from ssl_cr_histo_amd import _lib as L
from ssl_cr_histo_amd import kernels as K

FILL = 0x7F


class FakeLib:
    """stands in for libsslcr.so: an entry point is a Python function over the raw pointers of its descriptor"""

    def __init__(self, **entries):
        self.__dict__.update(entries)
        self.seen = []

    def sslcr_last_error(self):
        return b"fake_entry: invalid argument (refused)"


def _copy(dst, src, n):
    C.memmove(dst, src, n)
    return 0


def _bn_act(x, y, scale=None):
    return L.BnActDesc(L.ptr(x), L.ptr(scale), None, None, None, None, L.ptr(y), 1, 8, 0, 0, 0)


@pytest.fixture(autouse=True)
def _no_fault_leaks(monkeypatch):
    monkeypatch.setattr(A, "FAULTED", [])


@pytest.mark.parametrize("fill", A.FILLS)
def test_results_arrive_and_the_caller_sees_poison_where_nothing_was_written(fill, monkeypatch):
    """the fake kernel copies x to y but skips y's last element: the caller's y holds x, then `fill`; an `empty` made through
    kernels.torch is all `fill` before the launch"""
    x = torch.arange(64, dtype=torch.float32)
    lib = FakeLib(sslcr_bn_act=lambda dt, d, st: _copy(d.y, d.x, 63 * 4))
    with A.arena(fill, monkeypatch, device="cpu", lib=lib) as a:
        y = K.torch.empty(64, dtype=torch.float32)
        assert bool((y.view(torch.uint8) == fill).all())
        assert bool((K.torch.empty_like(x).view(torch.uint8) == fill).all())
        assert bool((K.torch.empty_strided((4, 4), (4, 1), dtype=torch.bfloat16).view(torch.uint8) == fill).all())
        assert K.torch.float32 is torch.float32 and K.torch.zeros(2).tolist() == [0.0, 0.0]
        L.check(L.lib().sslcr_bn_act(0, _bn_act(x, y), None))
        assert a.launches == 1 and a.calls == 1
    assert torch.equal(y[:63], x[:63])
    assert bool((y[63:].view(torch.uint8) == fill).all())
    assert K.torch is torch and L.ptr(x).value == x.data_ptr()          # the patches are gone


@pytest.mark.parametrize("where, offset", [("front", -1), ("behind", 256), ("far", 256 + A.GUARD - 1), ("first", -A.GUARD)])
def test_a_byte_out_of_range_is_reported_with_tensor_and_offset(where, offset, monkeypatch):
    x, y = torch.zeros(64), torch.zeros(64)

    def kernel(dt, d, st):
        C.memset(d.y + offset, 0x01, 1)
        return _copy(d.y, d.x, 256)
    with A.arena(FILL, monkeypatch, device="cpu", lib=FakeLib(sslcr_bn_act=kernel)):
        with pytest.raises(AssertionError) as e:
            L.check(L.lib().sslcr_bn_act(0, _bn_act(x, y), None))
    msg = str(e.value)
    assert "tensor 1 of the call" in msg and "shape (64,) torch.float32" in msg and f"offset {offset} relative" in msg, msg


def test_a_write_into_an_input_guard_names_the_input(monkeypatch):
    x, y = torch.zeros(32, dtype=torch.bfloat16), torch.zeros(64)
    with A.arena(FILL, monkeypatch, device="cpu", lib=FakeLib(sslcr_bn_act=lambda dt, d, st: C.memset(d.x + 64, 0, 3) and 0)):
        with pytest.raises(AssertionError, match=r"tensor 0 of the call, shape \(32,\) torch.bfloat16.*offset 64 relative"):
            L.check(L.lib().sslcr_bn_act(1, _bn_act(x, y), None))


def test_views_keep_their_distance_and_a_storage_is_placed_once(monkeypatch):
    big = torch.arange(1024, dtype=torch.float32)
    a_view, b_view = big[128:256], big[512:]
    other = torch.zeros(8)
    with A.arena(FILL, monkeypatch, device="cpu") as a:
        pa, pb, pa2, po = L.ptr(a_view).value, L.ptr(b_view).value, L.ptr(a_view).value, L.ptr(other).value
        assert pb - pa == b_view.data_ptr() - a_view.data_ptr() == (512 - 128) * 4
        assert pa2 == pa and len(a.regions) == 2
        assert pa != a_view.data_ptr() and a.find(po) is not a.find(pa)
        # the region holds the WHOLE storage: what a descriptor reaches past the view by its own strides is there
        assert (C.c_float * 1).from_address(pa + (1023 - 128) * 4)[0] == 1023.0
        assert L.ptr(None) is None


@pytest.mark.parametrize("align", [4, 8, 16])
def test_every_base_is_aligned_to_A_and_to_no_multiple_of_2A(align, monkeypatch):
    """through fields whose stated alignment is 4, 8 and 16: bn_bwd's scale, sums and x"""
    field = {4: "scale", 8: "sums", 16: "x"}[align]
    assert A.align_of("sslcr_bn_bwd_desc", field) == align
    seen = []
    lib = FakeLib(sslcr_bn_bwd_reduce=lambda dt, d, st: seen.append(getattr(d, field)) or 0)
    with A.arena(FILL, monkeypatch, device="cpu", lib=lib) as a:
        for n in (1, 3, 64, 1001):          # several sizes, several allocations
            t = torch.arange(n, dtype=torch.float64)
            d = L.BnBwdDesc()
            setattr(d, field, L.ptr(t).value)
            L.check(L.lib().sslcr_bn_bwd_reduce(0, d, None))
            p = seen[-1]
            assert p % align == 0 and p % (2 * align) == align, (n, hex(p))
            assert getattr(d, field) == p and (C.c_double * n).from_address(p)[n - 1] == n - 1          # moved with its bytes
        assert a.launches == 4


def test_two_pointers_into_one_storage_move_together(monkeypatch):
    """x and x2 of the stem are two views of one batch (a slice along the first dimension is contiguous as it stands): the region moves
    once, to the 4 bytes the header states for both, and BOTH pointers follow it"""
    batch = torch.arange(64, dtype=torch.float32).reshape(4, 16)
    seen = []
    lib = FakeLib(sslcr_stem_conv=lambda dt, d, st: seen.append((d.x, d.x2, (C.c_float * 1).from_address(d.x)[0], (C.c_float * 1).from_address(d.x2)[0])) or 0)
    with A.arena(FILL, monkeypatch, device="cpu", lib=lib) as a:
        d = L.StemDesc(L.ptr(batch[:1]), None, None)
        d.x2 = L.ptr(batch[1:])
        L.check(L.lib().sslcr_stem_conv(0, d, None))
        assert len(a.regions) == 1
    x, x2, v, v2 = seen[0]
    assert x % 8 == 4 and x2 - x == 64 and (v, v2) == (0.0, 16.0)


def test_a_descriptor_launched_twice_keeps_valid_pointers(monkeypatch):
    """kernels.bn_bwd launches reduce and apply from ONE descriptor: the second launch makes no ptr() call, reads what the first
    one wrote and its own result reaches the caller"""
    x, sums, dx = torch.arange(8, dtype=torch.float32), torch.zeros(8), torch.zeros(8)
    lib = FakeLib(sslcr_bn_bwd_reduce=lambda dt, d, st: _copy(d.sums, d.x, 32), sslcr_bn_bwd_apply=lambda dt, d, st: _copy(d.dx, d.sums, 32))
    with A.arena(FILL, monkeypatch, device="cpu", lib=lib) as a:
        d = L.BnBwdDesc()
        d.x, d.sums, d.dx = L.ptr(x), L.ptr(sums), L.ptr(dx)
        L.check(L.lib().sslcr_bn_bwd_reduce(0, d, None))
        assert torch.equal(sums, x) and d.sums % 16 == 8
        L.check(L.lib().sslcr_bn_bwd_apply(0, d, None))
        assert a.launches == 1 and a.calls == 2
    assert torch.equal(dx, x)


def test_a_table_in_device_memory_is_moved_too(monkeypatch):
    """sslcr_optimizer_step reads its sslcr_tensor_desc rows from device memory: the rows' pointers are corrected there"""
    p, g = torch.arange(5, dtype=torch.float32), torch.ones(5)
    seen = []

    def step(descs, n, max_n, o, st):
        t = (L.TensorDesc * n).from_address(descs.value)
        seen.append((descs.value, t[0].p, t[0].g))
        for i in range(t[0].n):
            (C.c_float * 1).from_address(t[0].p + 4 * i)[0] += (C.c_float * 1).from_address(t[0].g + 4 * i)[0]
        return 0
    with A.arena(FILL, monkeypatch, device="cpu", lib=FakeLib(sslcr_optimizer_step=step)):
        descs = (L.TensorDesc * 1)()
        descs[0] = L.TensorDesc(L.ptr(p), L.ptr(g), None, None, 5)
        dd = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8)
        L.check(L.lib().sslcr_optimizer_step(L.ptr(dd), 1, 5, None, None))
    table, pp, pg = seen[0]
    assert table % 16 == 8 and pp % 8 == 4 and pg % 8 == 4
    assert p.tolist() == [1.0, 2.0, 3.0, 4.0, 5.0]


def test_a_refusal_still_raises_after_the_copy_back_and_the_guard_check(monkeypatch):
    x, y = torch.arange(64, dtype=torch.float32), torch.zeros(64)
    damage = []

    def kernel(dt, d, st):
        if damage:
            C.memset(d.y - 4, 0, 1)
        return _copy(d.y, d.x, 256) - 1
    with A.arena(FILL, monkeypatch, device="cpu", lib=FakeLib(sslcr_bn_act=kernel)):
        with pytest.raises(L.SslcrError, match="invalid argument"):
            L.check(L.lib().sslcr_bn_act(0, _bn_act(x, y), None))
        assert torch.equal(y, x)          # copied back although the call failed
        damage.append(1)                  # ... and a damaged guard outranks the refusal
        with pytest.raises(AssertionError, match="offset -4 relative"):
            L.check(L.lib().sslcr_bn_act(0, _bn_act(x, y), None))
    assert not A.FAULTED


def test_a_fault_closes_the_arena(monkeypatch):
    class Faulting(FakeLib):
        def sslcr_last_error(self):
            return b"conv2d: an illegal memory access was encountered"
    x = torch.zeros(4)
    with A.arena(FILL, monkeypatch, device="cpu", lib=Faulting(sslcr_bn_act=lambda dt, d, st: -1)):
        with pytest.raises(L.SslcrError):
            L.check(L.lib().sslcr_bn_act(0, _bn_act(x, x), None))
    assert A.FAULTED and "illegal memory access" in A.FAULTED[0]
    with pytest.raises(AssertionError, match="not started"):
        with A.arena(FILL, monkeypatch, device="cpu"):
            pass
    A.FAULTED.clear()
    with pytest.raises(RuntimeError):          # any other exception inside the block (a HIP error surfacing in torch) does the same
        with A.arena(FILL, monkeypatch, device="cpu"):
            raise RuntimeError("HIP error")
    assert A.FAULTED == ["RuntimeError: HIP error"]


def test_guard_covers_two_rows_of_every_map(monkeypatch):
    with A.arena(FILL, monkeypatch, device="cpu"):
        L.ptr(torch.zeros((1, 2, 32, 512)))                      # fp32 512 channels x 32 columns: 64 KiB per row, two rows = GUARD
        L.ptr(torch.zeros((1, 3, 256, 256)))                     # the stem's NCHW image: a row is W elements
        with pytest.raises(AssertionError, match="two rows"):
            L.ptr(torch.zeros((1, 2, 33, 512)))


@pytest.mark.parametrize("poison", [float("nan"), 3.3895313892515355e38, 3.3961513649220713e38, float("inf")])
def test_f64_checks_reject_poison(poison):
    """what an arena leaves in an element no kernel wrote -- a NaN (0xFF..) or 3.39e38 (0x7F7F..) -- fails tests/_f64.py's check and
    check_stats, in a result and in a partial row"""
    assert torch.tensor([0x7F7F7F7F], dtype=torch.int32).view(torch.float32).item() == 3.3961513649220713e38
    assert torch.tensor([0x7F7F], dtype=torch.int16).view(torch.bfloat16).float().item() == 3.3895313892515355e38
    assert math.isnan(torch.tensor([-1], dtype=torch.int32).view(torch.float32).item())
    assert math.isnan(torch.tensor([-1], dtype=torch.int16).view(torch.bfloat16).float().item())
    want = torch.linspace(-1, 1, 24, dtype=torch.float64).reshape(1, 2, 3, 4)
    bnd = torch.full_like(want, 1e-3)
    B.check(want.float(), want, bnd, "clean")
    for dtype in (torch.float32, torch.bfloat16):
        got = want.to(dtype)
        B.check(got, want, torch.full_like(want, 1e-2), "clean")
        got.view(-1)[7] = poison
        with pytest.raises(AssertionError):
            B.check(got, want, torch.full_like(want, 1e-2), "poisoned")
    acc = want.reshape(-1, 4)
    rows = torch.stack([acc.sum(0), (acc * acc).sum(0)]).float().reshape(1, 2, 4).repeat(3, 1, 1) / 3
    B.check_stats(rows, acc, acc.abs(), 9, "clean rows")
    for which in (0, 1):
        bad = rows.clone()
        bad[2, which, 1] = poison
        with pytest.raises(AssertionError):
            B.check_stats(bad, acc, acc.abs(), 9, "poisoned rows")


def test_alignment_table_is_the_headers():
    """every pointer of the training entry points has an alignment stated in include/sslcr.h ("Alignment (owner): ..."), and
    tests/_arena.py places by exactly those numbers: the same owners, the same pointers, the same bytes -- both ways"""
    from ssl_cr_histo_amd import engine  # noqa: F401  registers its mirrors
    stated = A.header_alignments()
    params = A.header_params()
    owners = set(A.STRUCT_ALIGN)
    for entry, spec in A.ENTRY_ALIGN.items():
        assert entry in L.SIGNATURES and len(params[entry]) == len(L.SIGNATURES[entry][1]), entry
        plain = {}
        for name, ctype in zip(params[entry], L.SIGNATURES[entry][1]):
            if name == "stream":
                continue
            if isinstance(spec.get(name), str):          # a descriptor: its struct states its fields
                assert ctype is C.POINTER(L.MIRRORS[spec[name]]), (entry, name)
                owners.add(spec[name])
            elif ctype is L.vp:
                plain[name] = A.align_of(entry, name)
            else:
                assert name not in spec, (entry, name)
        assert set(spec) <= set(params[entry]), entry
        if plain:
            assert stated.get(entry) == plain, (entry, stated.get(entry), plain)
        else:
            assert entry not in stated, entry
    assert owners == set(A.STRUCT_ALIGN), "a descriptor of ENTRY_ALIGN without a row in STRUCT_ALIGN"
    for owner, fields in A.STRUCT_ALIGN.items():
        pointers = [f for f, t in L.MIRRORS[owner]._fields_ if t is L.vp]
        assert set(fields) <= set(pointers), owner
        assert stated.get(owner) == {f: A.align_of(owner, f) for f in pointers}, (owner, stated.get(owner))
    assert set(stated) == set(A.STRUCT_ALIGN) | {e for e in A.ENTRY_ALIGN if e in stated}
    assert {v for d in stated.values() for v in d.values()} == {1, 4, 8, 16}
    # the entry points the issue of the arena names are all here
    for entry in ("sslcr_conv2d", "sslcr_conv2d_wgrad", "sslcr_conv2d_s2_pair", "sslcr_conv2d_fp8", "sslcr_stem_conv", "sslcr_bn_act",
                  "sslcr_bn_relu_maxpool", "sslcr_linear_fwd", "sslcr_loss", "sslcr_optimizer_step"):
        assert entry in A.ENTRY_ALIGN
