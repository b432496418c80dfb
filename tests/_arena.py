"""The relocating shim of tests/test_arena_gpu.py: every tensor the library sees moved into a poisoned arena at the least alignment
the ABI allows (no product code: three attributes of ssl_cr_histo_amd._lib and one of ssl_cr_histo_amd.kernels are patched while
`arena(fill, monkeypatch)` is open).

What PyTorch's caching allocator hides from the per-kernel tests, and what the arena does about it:
  * an out-of-range read comes back as the zero that padding must be (fresh pages), or as an earlier test's finite activations:
    here every operand sits between two GUARD-byte bands of the byte `fill`, so an over-read that reaches a sum poisons it;
  * an element a ragged tail forgot to write keeps the previous, nearly identical result (torch.empty hands the block back): here
    kernels.torch is a proxy whose empty / empty_like / empty_strided return tensors whose bytes are all `fill`;
  * a write past an output lands in allocator slack: here every check() asserts that every guard byte still equals `fill`;
  * every base address is a multiple of 256: here a pointer sits at an address that is a multiple of the alignment A that
    include/sslcr.h states for it ("Alignment (owner): ...") and NOT a multiple of 2 A.
The fills: 0xFF.. is a NaN in bf16, fp32 and fp64, but v_max (fmaxf(x, 0), the max-pool) drops a NaN; 0x7F7F.. is 3.39e38 in bf16 and
fp32, finite, positive and larger than anything the cases produce: it survives a max and a ReLU.  Each covers the other's blind spot.

`_lib.ptr(t)` relocates the whole storage behind t (the tests pass slices, and segment descriptors reach past a view by their own
strides) into a region of its own: GUARD bytes of fill, the storage's bytes, GUARD bytes of fill; a storage is placed once (memoised
by its base address: x passed as x and as residual aliases in the arena as it does outside) and a later ptr() of it copies the
caller's bytes in again.  ptr() cannot know which field its result goes to, so it places at the default alignment of 16; the proxy
that `_lib.lib()` returns knows the entry point, reads the pointer fields of the descriptors (and the pointer arguments) of a call,
and where the header states another alignment for a field it shifts the region's bytes to that alignment and corrects the field --
the table sslcr_optimizer_step reads from device memory included.
`_lib.check(rc)` ends a call: in a `finally` around the original check every placed storage is copied back over the caller's
tensor (on the current stream, the one the launch used), the device is synchronised and every guard byte is compared with `fill`; a
changed byte fails with the tensor's position in the call, shape and dtype and the first changed offset relative to the region
(negative: in front, >= nbytes: behind).  The original check's SslcrError still propagates.
The regions live until the context closes, not until the call ends: kernels.bn_bwd and kernels.stem_wgrad_pool launch a second
entry point from the descriptor the first one was given, so the addresses in it must stay valid (and hold the first launch's
results).  Every check therefore copies back and inspects every region of the context; holding the caller's storages also keeps the
allocator from handing an address out twice while it is memoised.

A fault stops the file: any exception out of the library that is not an AssertionError or an SslcrError of argument validation (a
HIP error above all) is recorded in FAULTED, and arena() refuses to open again -- nothing more goes onto the device.

What this cannot see: an over-read whose value is discarded (harmless inside an arena, a fault at an allocation's last page), and
anything behind the engine's own arena (sslcr_net_* never calls _lib.ptr per tensor)."""
import contextlib
import ctypes as C
import os
import re

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 128 * 1024         # bytes of fill on either side of a storage: two map rows of the widest operand, fp32 32 x 512 channels (asserted per 4-D operand)
SLAB = 32                  # twice the largest alignment: a region's anchor is a multiple of it, the data starts A bytes behind the anchor
DEFAULT_ALIGN = 16
FILLS = (0xFF, 0x7F)
FAULTED = []               # the first fault: nothing more goes onto the device from a file that uses the arena

# ---- the alignment include/sslcr.h states ("Alignment (owner): names N-byte aligned; ..."), restated: owner -> {pointer: A}, a
# pointer that is not listed has DEFAULT_ALIGN.  tests/test_arena_cpu.py holds this table to the header's words, both ways.
_CH4 = dict.fromkeys(("in_scale", "in_shift"), 4)
STRUCT_ALIGN = {
    "sslcr_conv_desc": {**_CH4, "mask_scale": 4, "mask_shift": 4, "mask_mean": 4},
    "sslcr_fp8_desc": {"x_scale_dev": 4, "amax_out": 4},
    "sslcr_wgrad_desc": {**_CH4, "dw": 4},
    "sslcr_stem_desc": {"x": 4, "x2": 4, "bias": 4, "stats": 4, "out_scale": 4},
    "sslcr_stem_wgrad_desc": {"x": 4, "x2": 4, "dw": 4},
    "sslcr_bn_finalize_desc": {**dict.fromkeys(("partials", "gamma", "beta", "scale", "shift", "mean", "invstd", "running_mean", "running_var",
                                                "tickets"), 4), **dict.fromkeys(("num_batches_tracked", "sums_out", "sums_in", "stage"), 8)},
    "sslcr_bn_act_desc": {"scale": 4, "shift": 4, "rscale": 4, "rshift": 4, "ybits": 1},
    "sslcr_pool_fwd_desc": {"scale": 4, "shift": 4, "argmax": 8},
    "sslcr_pool_bwd_desc": {"scale": 4, "shift": 4, "argmax": 8},
    "sslcr_bn_bwd_desc": {**dict.fromkeys(("scale", "shift", "mean", "invstd", "dgamma", "dbeta"), 4), "sums": 8, "pool_argmax": 8, "yact_bits": 1},
    "sslcr_loss_desc": {**dict.fromkeys(("logits", "logits_t", "target_f", "dlogits", "out"), 4), "target_i": 8},
    "sslcr_loss_opts": {"class_weight": 4, "denominator": 4, "stats": 4},
    "sslcr_tensor_desc": dict.fromkeys(("p", "g", "s1", "s2", "w_fwd", "w_dgrad"), 4),
}
# entry point -> {parameter: the struct it points to | the alignment of a plain pointer parameter}
ENTRY_ALIGN = {
    "sslcr_conv2d": {"d": "sslcr_conv_desc"},
    "sslcr_conv2d_s2_pair": {"c1": "sslcr_conv_desc", "ds": "sslcr_conv_desc"},
    "sslcr_conv2d_fp8": {"d": "sslcr_conv_desc", "q": "sslcr_fp8_desc"},
    "sslcr_conv2d_wgrad": {"d": "sslcr_wgrad_desc"},
    "sslcr_stem_conv": {"d": "sslcr_stem_desc"},
    "sslcr_stem_conv_pool": {"d": "sslcr_stem_desc"},
    "sslcr_stem_wgrad": {"d": "sslcr_stem_wgrad_desc"},
    "sslcr_stem_wgrad_pool": {"w": "sslcr_stem_wgrad_desc", "bn": "sslcr_bn_bwd_desc"},
    "sslcr_bn_finalize": {"d": "sslcr_bn_finalize_desc"},
    "sslcr_bn_act": {"d": "sslcr_bn_act_desc"},
    "sslcr_bn_relu_maxpool": {"d": "sslcr_pool_fwd_desc"},
    "sslcr_maxpool_relu_bwd": {"d": "sslcr_pool_bwd_desc"},
    "sslcr_avgpool_fwd": {"x": 16, "y": 4},
    "sslcr_avgpool_bwd": {"dy": 4, "dx": 16},
    "sslcr_bn_bwd_reduce": {"d": "sslcr_bn_bwd_desc"},
    "sslcr_bn_bwd_apply": {"d": "sslcr_bn_bwd_desc"},
    "sslcr_bn_param_grads": {"sums": 8, "invstd": 4, "dgamma": 4, "dbeta": 4},
    "sslcr_linear_fwd": dict.fromkeys(("x", "w", "b", "y"), 4),
    "sslcr_linear_bwd": dict.fromkeys(("x", "w", "dy", "yact", "dx", "dw", "db", "scratch"), 4),
    "sslcr_loss": {"d": "sslcr_loss_desc"},
    "sslcr_loss_ex": {"d": "sslcr_loss_desc", "opts": "sslcr_loss_opts"},
    "sslcr_ce_denominator": {"target_i": 8, "class_weight": 4, "out2": 4},
    "sslcr_softmax_col": {"logits": 4, "out": 4},
    "sslcr_optimizer_step": {"device_descs": 8},
    "sslcr_optimizer_step_groups": {"device_descs": 8, "coef_dev": 4},
}
DEVICE_TABLES = {"sslcr_optimizer_step": "sslcr_tensor_desc", "sslcr_optimizer_step_groups": "sslcr_tensor_desc"}   # (device_descs, ntensors)


def header_text():
    with open(os.path.join(ROOT, "include", "sslcr.h")) as f:
        return f.read()


def header_params(text=None):
    """entry point -> the names of its parameters, in order, from the prototypes of include/sslcr.h"""
    text = re.sub(r"/\*.*?\*/", "", header_text() if text is None else text, flags=re.S)
    out = {}
    for m in re.finditer(r"\b(sslcr_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        names = [re.sub(r"\[.*", "", p).split()[-1].lstrip("*") for p in m.group(2).split(",") if p.strip() and p.strip() != "void"]
        out[m.group(1)] = names
    return out


def header_alignments(text=None):
    """owner (a struct or an entry point) -> {pointer: bytes}, from the "Alignment (owner): a, b 16-byte aligned; c 4-byte aligned."
    comments of include/sslcr.h"""
    text = header_text() if text is None else text
    out = {}
    for m in re.finditer(r"Alignment \((sslcr_\w+)\):(.*?)(?:\.\s\s|\.?\s*\*/)", text, flags=re.S):          # a statement ends with ".  " or the comment
        d = out.setdefault(m.group(1), {})
        for part in re.sub(r"\([^()]*\)", "", m.group(2)).split(";"):
            g = re.match(r"\s*([\w\s,]+?)\s+(\d+)-byte\s+aligned", part.replace("\n", " "))
            assert g, (m.group(1), part)
            for name in g.group(1).split(","):
                assert name.strip() not in d, (m.group(1), name)
                d[name.strip()] = int(g.group(2))
    return out


def align_of(owner, name):
    """the stated alignment of pointer `name` of `owner` (a struct, or an entry point's plain pointer parameter)"""
    if owner in STRUCT_ALIGN:
        return STRUCT_ALIGN[owner].get(name, DEFAULT_ALIGN)
    v = ENTRY_ALIGN[owner].get(name, DEFAULT_ALIGN)
    assert isinstance(v, int), (owner, name)
    return v


def _storage_bytes(t):
    """the whole storage behind t as a uint8 tensor (shares the memory, keeps it alive)"""
    return torch.empty(0, dtype=torch.uint8, device=t.device).set_(t.untyped_storage())


class _Region:
    """one relocated storage: GUARD bytes of fill | pad to an anchor | A bytes | the storage's bytes | fill"""

    def __init__(self, t, fill, position):
        self.src = _storage_bytes(t)
        self.base, self.nbytes = t.untyped_storage().data_ptr(), self.src.numel()
        self.fill, self.position, self.shape, self.dtype = fill, position, tuple(t.shape), t.dtype
        self.buf = torch.full((2 * GUARD + 2 * SLAB + self.nbytes,), fill, dtype=torch.uint8, device=t.device)
        self.anchor = GUARD + (-(self.buf.data_ptr() + GUARD)) % SLAB
        self.A = DEFAULT_ALIGN
        self.data().copy_(self.src)

    @property
    def start(self):
        return self.anchor + self.A

    @property
    def addr(self):
        return self.buf.data_ptr() + self.start

    def data(self):
        return self.buf[self.start:self.start + self.nbytes]

    def realign(self, A):
        """the same bytes at the anchor + A: an address that is a multiple of A and of no 2 A (A | 16)"""
        assert A in (1, 2, 4, 8, 16), A
        keep = self.data().clone()
        self.buf[self.anchor:self.anchor + SLAB + self.nbytes].fill_(self.fill)
        self.A = A
        self.data().copy_(keep)

    def damage(self):
        """a 0-d bool tensor: some guard byte differs from fill"""
        return (self.buf[:self.start] != self.fill).any() | (self.buf[self.start + self.nbytes:] != self.fill).any()

    def first_damage(self):
        """the first changed guard byte as an offset relative to the region (None: intact)"""
        front = (self.buf[:self.start] != self.fill).nonzero()
        if front.numel():
            return int(front[0]) - self.start
        back = (self.buf[self.start + self.nbytes:] != self.fill).nonzero()
        return self.nbytes + int(back[0]) if back.numel() else None


class Arena:
    def __init__(self, fill, device):
        assert 0 <= fill <= 255
        self.fill, self.device = fill, torch.device(device)
        self.regions = {}          # storage base address -> _Region, in order of placement
        self.touched = []          # the regions ptr() returned since the last check(), in order: a tensor's position in the call
        self.launches = 0          # check() calls with at least one relocated pointer
        self.calls = 0
        self._check = None         # the original _lib.check

    # -- _lib.ptr
    def ptr(self, t):
        if t is None:
            return None
        assert t.device.type == self.device.type, f"a {t.device} tensor in an arena on {self.device}"
        if t.untyped_storage().nbytes() == 0:
            return C.c_void_p(t.data_ptr())
        if t.dim() == 4:          # NHWC map, KRSC filter or the stem's NCHW image: the last two dimensions are at least one map row
            row = t.shape[2] * t.shape[3] * t.element_size() if t.shape[1] != 3 else t.shape[3] * t.element_size()
            assert GUARD >= 2 * row, f"GUARD = {GUARD} < two rows of {tuple(t.shape)} {t.dtype}"
        base = t.untyped_storage().data_ptr()
        r = self.regions.get(base)
        if r is None or r.nbytes != t.untyped_storage().nbytes():
            r = self.regions[base] = _Region(t, self.fill, len(self.touched))
        else:
            r.data().copy_(r.src)          # what the caller holds now
        if r not in self.touched:
            r.position = len(self.touched)
            self.touched.append(r)
        return C.c_void_p(r.addr + (t.data_ptr() - base))

    # -- _lib.lib: the entry points of ENTRY_ALIGN move their pointers to the stated alignment
    def find(self, address):
        for r in self.regions.values():
            if r.addr <= address < r.addr + r.nbytes:
                return r
        return None

    def call(self, entry, fn, *args):
        """fn(*args) with every pointer of the call at its stated alignment.  Every pointer is located first (a region moved on behalf
        of one field would leave the other pointers into it stale: x and x2 of one batch), then a region whose alignment differs is
        moved once, then every pointer is rewritten where it stands: descriptor field, argument or row of a device-memory table."""
        from ssl_cr_histo_amd import _lib as L
        spec, args = ENTRY_ALIGN[entry], list(args)
        refs = []          # (write the new address, the address as it stands, alignment, what)

        def fields(s, owner, what):
            for name, ftype in s._fields_:
                if ftype is C.c_void_p and getattr(s, name):
                    refs.append((lambda v, s=s, name=name: setattr(s, name, v), getattr(s, name), align_of(owner, name), f"{what}->{name}"))
        for i, (pname, a) in enumerate(zip(PARAMS[entry], args)):
            if isinstance(a, C.Structure) and isinstance(spec.get(pname), str):
                fields(a, spec[pname], f"{entry}: {pname}")
            elif isinstance(a, C.c_void_p) and a.value and pname != "stream":
                refs.append((lambda v, i=i: args.__setitem__(i, C.c_void_p(v)), a.value, align_of(entry, pname), f"{entry}: {pname}"))
        table = None
        if entry in DEVICE_TABLES and self.find(args[0].value) is not None:          # (device_descs, ntensors, ...)
            owner, n = DEVICE_TABLES[entry], args[1]
            cls, tr = L.MIRRORS[owner], self.find(args[0].value)
            toff = args[0].value - tr.addr
            table = (cls * n).from_buffer_copy(bytes(tr.data()[toff:toff + n * C.sizeof(cls)].cpu().numpy()))
            for j in range(n):
                fields(table[j], owner, f"{entry}: device_descs[{j}]")
        located = [(write, self.find(addr), addr, A, what) for write, addr, A, what in refs]
        located = [(write, r, addr - r.addr, A, what) for write, r, addr, A, what in located if r is not None]
        wants = {}
        for _, r, _, A, what in located:
            assert wants.setdefault(r.base, (A, what))[0] == A, f"{what} wants {A}-byte alignment of a storage that {wants[r.base][1]} holds at {wants[r.base][0]}"
        for _, r, _, A, _ in located:
            if r.A != A:
                r.realign(A)
        for write, r, off, _, _ in located:
            write(r.addr + off)
        if table is not None:
            tr.data()[toff:toff + len(bytes(table))].copy_(torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8))
        return fn(*args)

    # -- _lib.check
    def check(self, rc):
        from ssl_cr_histo_amd import _lib as L
        self.calls += 1
        if self.touched:
            self.launches += 1
        try:
            try:
                self._check(rc)
            except L.SslcrError as e:
                if "invalid argument" not in str(e):          # not argument validation: a HIP error out of a launch
                    FAULTED.append(f"{e}")
                raise
        finally:
            self._end_call()

    def _end_call(self):
        touched, self.touched = self.touched, []
        try:
            for r in self.regions.values():
                r.src.copy_(r.data())
            if self.device.type == "cuda":
                torch.cuda.synchronize()
            if self.regions and bool(torch.stack([r.damage() for r in self.regions.values()]).any()):
                for r in self.regions.values():
                    off = r.first_damage()
                    if off is not None:
                        where = f"tensor {r.position} of the call" if r in touched else "a tensor of an earlier call"
                        raise AssertionError(f"guard band of {where}, shape {r.shape} {r.dtype}, {r.nbytes} bytes at alignment {r.A}: first "
                                             f"changed byte at offset {off} relative to the region (negative: in front, >= {r.nbytes}: behind)")
        except AssertionError:
            raise
        except Exception as e:
            FAULTED.append(f"{type(e).__name__}: {e}")
            raise


class _LibProxy:
    def __init__(self, arena, real):
        self._arena, self._real = arena, real

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if name not in ENTRY_ALIGN:
            return fn
        return lambda *args: self._arena.call(name, fn, *args)


class _TorchProxy:
    """torch for ssl_cr_histo_amd.kernels: every attribute forwarded, except that an empty tensor's bytes are all `fill`"""

    def __init__(self, fill):
        self._fill = fill

    def __getattr__(self, name):
        return getattr(torch, name)

    def _poisoned(self, t):
        if t.untyped_storage().nbytes():
            _storage_bytes(t).fill_(self._fill)
        return t

    def empty(self, *a, **k):
        return self._poisoned(torch.empty(*a, **k))

    def empty_like(self, *a, **k):
        return self._poisoned(torch.empty_like(*a, **k))

    def empty_strided(self, *a, **k):
        return self._poisoned(torch.empty_strided(*a, **k))


PARAMS = header_params()


@contextlib.contextmanager
def arena(fill, monkeypatch, device="cuda", lib=None):
    """-> the Arena, with _lib.ptr / _lib.check / _lib.lib and kernels.torch patched until the block ends.  device: where the tensors
    live ("cpu": the shim's own tests, tests/test_arena_cpu.py); lib: an object that stands in for libsslcr.so there."""
    from ssl_cr_histo_amd import _lib as L
    from ssl_cr_histo_amd import kernels as K
    assert not FAULTED, f"not started: {FAULTED[0]}"
    a = Arena(fill, device)
    a._check, real_lib = L.check, L.lib
    proxy = []

    def lib_proxy():
        if not proxy:
            proxy.append(_LibProxy(a, lib if lib is not None else real_lib()))
        return proxy[0]
    with monkeypatch.context() as m:
        m.setattr(L, "ptr", a.ptr)
        m.setattr(L, "check", a.check)
        m.setattr(L, "lib", lib_proxy)
        m.setattr(K, "torch", _TorchProxy(fill))
        try:
            yield a
        except (AssertionError, L.SslcrError):
            raise
        except Exception as e:          # a HIP error surfacing in torch, above all
            FAULTED.append(f"{type(e).__name__}: {e}")
            raise
