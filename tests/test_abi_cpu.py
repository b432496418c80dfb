"""CPU-only: the C-ABI library builds for gfx950, loads, and exports every symbol include/sslcr.h declares;
the product path refuses to run without the MI355X (no CPU/PyTorch fallback)."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from ssl_cr_histo_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    from ssl_cr_histo_amd import engine  # noqa: F401  registers engine signatures
    return _lib.lib()


def header_symbols():
    src = open(os.path.join(ROOT, "include", "sslcr.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(sslcr_[a-z0-9_]+)\s*\(", src)))


def test_every_declared_symbol_is_exported_and_bound(lib):
    from ssl_cr_histo_amd import _lib
    names = header_symbols()
    assert len(names) >= 40
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/sslcr.h but not exported by libsslcr.so"
    missing = [n for n in names if n not in _lib.SIGNATURES]
    assert not missing, f"no ctypes signature for {missing}"
    extra = [n for n in _lib.SIGNATURES if n not in names]
    assert not extra, f"bound but not declared in the header: {extra}"


def test_version_and_error_string(lib):
    assert lib.sslcr_version() >= 4      # the ABI notes in include/sslcr.h refer to this number
    assert isinstance(lib.sslcr_last_error(), bytes)


def test_argument_validation_without_gpu(lib):
    """descriptor checks run before any device work: bad arguments return -1 with a message."""
    from ssl_cr_histo_amd import _lib as L
    d = L.ConvDesc()
    assert lib.sslcr_conv2d(0, d, None) == -1
    assert b"null tensor" in lib.sslcr_last_error()
    assert lib.sslcr_conv2d(7, d, None) == -1
    assert b"dtype" in lib.sslcr_last_error()
    assert lib.sslcr_net_forward(None, 0, None, None, None, 0, 1, 64, 64, None, None, None) == -1
    # the alignment include/sslcr.h states for the pointers of the training entry points ("Alignment (owner): ..."): one pointer per
    # entry point at an aligned fake address plus half its alignment -> -1 and the pointer's name, decided from the value alone.
    # (Every descriptor here would also fail a later check, or is complete only in the pointer under test: nothing can launch.)
    import ctypes as C
    F = 0x7F0000010000

    def D(cls, **kw):
        d = cls()
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    conv = dict(x=F, w=F, y=F)
    bn_bwd = dict(dy=F, x=F, sums=F, mean=F, dx=F, invstd=F, scale=F, shift=F)
    rows = [
        ("d->bias", 16, lambda p: lib.sslcr_conv2d(1, D(L.ConvDesc, bias=p, **conv), None)),
        ("d->x", 16, lambda p: lib.sslcr_conv2d(0, D(L.ConvDesc, **dict(conv, x=p)), None)),
        ("d->in_scale", 4, lambda p: lib.sslcr_conv2d(1, D(L.ConvDesc, in_scale=p, **conv), None)),
        ("ds->y", 16, lambda p: lib.sslcr_conv2d_s2_pair(1, D(L.ConvDesc, **conv), D(L.ConvDesc, **dict(conv, y=p)), None)),
        ("c1->stats", 16, lambda p: lib.sslcr_conv2d_s2_pair(1, D(L.ConvDesc, stats=p, **conv), D(L.ConvDesc, **conv), None)),
        ("q->w_dequant", 16, lambda p: lib.sslcr_conv2d_fp8(D(L.ConvDesc, **conv), D(L.Fp8Desc, w8=F, w_dequant=p), None)),
        ("q->amax_out", 4, lambda p: lib.sslcr_conv2d_fp8(D(L.ConvDesc, **conv), D(L.Fp8Desc, w8=F, w_dequant=F, amax_out=p), None)),
        ("d->dy", 16, lambda p: lib.sslcr_conv2d_wgrad(1, D(L.WgradDesc, x=F, dy=p, dw=F), None)),
        ("d->dw", 4, lambda p: lib.sslcr_conv2d_wgrad(0, D(L.WgradDesc, x=F, dy=F, dw=p), None)),
        ("d->x", 4, lambda p: lib.sslcr_stem_conv(1, D(L.StemDesc, x=p, w=F, y=F), None)),
        ("d->w", 16, lambda p: lib.sslcr_stem_conv_pool(1, D(L.StemDesc, x=F, w=p, y=F), 0, 0, None)),
        ("d->dy", 16, lambda p: lib.sslcr_stem_wgrad(1, D(L.StemWgradDesc, x=F, dy=p, dw=F, x2=F, n_split=-1), None)),
        ("bn->pool_argmax", 8, lambda p: lib.sslcr_stem_wgrad_pool(1, D(L.StemWgradDesc, x=F, dw=F),
                                                                   D(L.BnBwdDesc, pool_dy=F, pool_argmax=p, **bn_bwd), None)),
        ("d->stage", 8, lambda p: lib.sslcr_bn_finalize(D(L.BnFinalizeDesc, C=1, partials=F, stage=p), None)),
        ("d->gamma", 4, lambda p: lib.sslcr_bn_finalize(D(L.BnFinalizeDesc, C=1, partials=F, stage=F, gamma=p), None)),
        ("d->res", 16, lambda p: lib.sslcr_bn_act(1, D(L.BnActDesc, x=F, y=F, scale=F, shift=F, res=p, C=4), None)),
        ("d->x", 16, lambda p: lib.sslcr_bn_relu_maxpool(0, D(L.PoolFwdDesc, x=p, y=F), None)),
        ("d->argmax", 8, lambda p: lib.sslcr_maxpool_relu_bwd(1, D(L.PoolBwdDesc, x=F, dy=F, dx=F, argmax=p), None)),
        ("x", 16, lambda p: lib.sslcr_avgpool_fwd(1, p, F, 1, 1, 8, None)),
        ("dy", 4, lambda p: lib.sslcr_avgpool_bwd(1, p, F, 1, 1, 8, None)),
        ("d->sums", 8, lambda p: lib.sslcr_bn_bwd_reduce(1, D(L.BnBwdDesc, g_in_reduce=1, **dict(bn_bwd, sums=p)), None)),
        ("d->gout", 16, lambda p: lib.sslcr_bn_bwd_apply(0, D(L.BnBwdDesc, g_in_reduce=1, gout=p, **bn_bwd), None)),
        ("sums", 8, lambda p: lib.sslcr_bn_param_grads(p, F, F, F, 8, None)),
        ("b", 4, lambda p: lib.sslcr_linear_fwd(F, F, p, F, 1, 1, 1, 0, None)),
        ("scratch", 4, lambda p: lib.sslcr_linear_bwd(F, F, F, None, None, None, None, 1, 1, 1, 0, p, None)),
        ("d->target_i", 8, lambda p: lib.sslcr_loss(D(L.LossDesc, logits=F, out=F, nx=1, C=2, target_i=p), None)),
        ("o->class_weight", 4, lambda p: lib.sslcr_loss_ex(D(L.LossDesc, logits=F, out=F, nx=1, C=2), D(L.LossOpts, class_weight=p, label_smoothing=2.0), None)),
        ("target_i", 8, lambda p: lib.sslcr_ce_denominator(p, 1, 2, None, -100, F, None)),
        ("out", 4, lambda p: lib.sslcr_softmax_col(F, p, 1, 2, 0, None)),
        ("device_descs", 8, lambda p: lib.sslcr_optimizer_step(p, 1, 1, D(L.OptDesc, kind=9), None)),
        ("coef_dev", 4, lambda p: lib.sslcr_optimizer_step_groups(F, 1, 1, D(L.OptDesc, kind=9), 1, p, None)),
    ]
    from ssl_cr_histo_amd import engine  # noqa: F401
    for name, align, call in rows:
        assert call(C.c_void_p(F + align // 2) if "->" not in name else F + align // 2) == -1, name
        msg = lib.sslcr_last_error().decode()
        assert f"({name} must be {align}-byte aligned)" in msg, (name, msg)
    # every entry point the alignment table of tests/_arena.py covers has a row above (its message names the entry point: __func__)
    import _arena
    hit = set()
    for name, align, call in rows:
        call(C.c_void_p(F + align // 2) if "->" not in name else F + align // 2)
        hit.add(lib.sslcr_last_error().decode().split(":")[0])
    assert hit | {"sslcr_optimizer_step"} >= set(_arena.ENTRY_ALIGN), sorted(set(_arena.ENTRY_ALIGN) - hit)


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-GPU behaviour")
def test_product_path_fails_loudly_without_gpu(lib):
    from ssl_cr_histo_amd import _lib as L
    from ssl_cr_histo_amd import engine, kernels, net
    with pytest.raises(L.SslcrError):
        engine.Engine()
    x = torch.zeros(1, 8, 8, 64)
    w = torch.zeros(64, 3, 3, 64)
    with pytest.raises(L.SslcrError):
        kernels.conv2d(x, w, 1, 1)
    m = net.TripletNet_Finetune("resnet18")
    with pytest.raises(RuntimeError):
        m(torch.zeros(1, 3, 64, 64))


def test_product_never_imports_the_oracle():
    """oracle/ is test infrastructure: nothing under ssl_cr_histo_amd/ may import it."""
    pkg = os.path.join(ROOT, "ssl_cr_histo_amd")
    for dp, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                txt = open(os.path.join(dp, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", txt, flags=re.M), os.path.join(dp, f)


def test_ctypes_mirrors_match_the_header_layout(tmp_path):
    """every struct include/sslcr.h defines against its ctypes mirror in _lib.MIRRORS (engine.py registers its three there): the same
    set of structs, the same fields in the same order, the same size, the same offset of every field (a small C program over the
    header, compiled with the host gcc).  A struct or a field added on one side only fails here by name; it would otherwise show up
    as garbage pointers on the GPU."""
    import ctypes as C
    import shutil
    import subprocess
    from ssl_cr_histo_amd import _lib as L
    from ssl_cr_histo_amd import build
    from ssl_cr_histo_amd import engine  # noqa: F401  registers its mirrors
    structs = build.header_structs()
    assert len(structs) == len(re.findall(r"^typedef struct \w+ \{", open(os.path.join(ROOT, "include", "sslcr.h")).read(), flags=re.M))
    assert sorted(L.MIRRORS) == sorted(structs), f"header only: {sorted(set(structs) - set(L.MIRRORS))}, mirrors only: {sorted(set(L.MIRRORS) - set(structs))}"
    for cname, cls in L.MIRRORS.items():
        have = [f for f, _ in cls._fields_]
        assert have == structs[cname], (f"{cname}: header only {[f for f in structs[cname] if f not in have]}, "
                                        f"mirror only {[f for f in have if f not in structs[cname]]}, or another order")
    if not shutil.which("gcc"):
        pytest.skip("no host C compiler")
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "sslcr.h"', 'int main(void) {']
    for cname, cls in L.MIRRORS.items():
        lines.append(f'  printf("{cname} . %zu\\n", sizeof({cname}));')
        for fname, _ in cls._fields_:
            lines.append(f'  printf("{cname} {fname} %zu\\n", offsetof({cname}, {fname}));')
    lines += ['  return 0;', '}']
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    r = subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    want = {}
    for ln in out.splitlines():
        cname, fname, v = ln.split()
        want[(cname, fname)] = int(v)
    for cname, cls in L.MIRRORS.items():
        for fname, _ in cls._fields_:
            assert getattr(cls, fname).offset == want[(cname, fname)], f"{cname}.{fname}"
        assert C.sizeof(cls) == want[(cname, ".")], f"sizeof {cname}: header {want[(cname, '.')]} vs ctypes {C.sizeof(cls)}"
    assert L.PredictTtaDesc.p.size == C.sizeof(L.PredictDesc)


def test_mirrored_constants_match_the_header():
    """every #define the Python layer mirrors (_lib.CONSTANTS: macro name -> value) against include/sslcr.h, the names kernels.py
    re-exports against _lib's, and the two values the kernels' fixtures are written for"""
    from ssl_cr_histo_amd import _lib as L
    from ssl_cr_histo_amd import build
    from ssl_cr_histo_amd import kernels as K
    defs = build.header_defines()
    assert len(L.CONSTANTS) >= 22
    for name, value in L.CONSTANTS.items():
        assert name in defs, f"{name} is not an integer #define of include/sslcr.h"
        assert defs[name] == value, f"{name}: header {defs[name]} vs _lib {value}"
    # every code of a mirrored family is mirrored: a filter, form or tissue mode added to the header alone fails by name
    forms = {"SSLCR_RESAMPLE_" + f.upper() for f in L.RESAMPLE_FORMS}
    for name in defs:
        if name.startswith(("SSLCR_RESAMPLE_", "SSLCR_TISSUE_")):
            assert name in L.CONSTANTS, name
    assert forms <= set(defs)
    for name in ("PIP_CHUNK", "SMOOTH_MAX_R", "EDT_ROW_CELLS", "SORT_TILE", "RANK_SCAN_TRIP", "RESAMPLE_FILTERS", "TISSUE_MODES"):
        assert getattr(K, name) == getattr(L, name), name
    assert defs["SSLCR_SMOOTH_MAX_R"] == 64 and defs["SSLCR_EDT_ROW_CELLS"] == 1024
