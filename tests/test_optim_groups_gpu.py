"""Grouped optimizer step on the MI355X, through the C-ABI: param groups, AdamW and global-norm clipping (include/sslcr.h, library
version 8).  Bounds and references: tests/_f64_optim.py and _f64.optimizer_ref (pinned to torch by tests/test_optim_groups_cpu.py).
The network is the fixed ResNet18, so the small problem is a batch of 4 at 64x64 (layer4 sees 2x2)."""
import copy
import ctypes as CT
import math
import struct

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import cases as C  # noqa: E402
from oracle import steps as S  # noqa: E402

import _f64 as B  # noqa: E402
import _f64_optim as BO  # noqa: E402
from _util import merged, oracle_state  # noqa: E402
from test_engine_gpu import DEV, _engine, build, ns, state_of  # noqa: E402
from test_engine_gpu2 import _run_ranks  # noqa: E402

PARTIALS = 1024
A_LR, B_WD = 1e-3, 1e-2


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------------ 1. the norm kernels alone
def _engine_grad_count():
    """elements of the engine's flat gradient buffer: every parameter padded to 64 (csrc/engine.cpp: goff)"""
    from oracle import model as OM
    specs = list(OM.net_param_specs()) + list(OM.classifier_param_specs("finetune", 2))
    return sum((int(np.prod(s)) + 63) // 64 * 64 for _, s, _ in specs)


def _check_norm(view, max_norm, what):
    from ssl_cr_histo_amd import _lib as L
    from ssl_cr_histo_amd import kernels as K
    assert L.lib().sslcr_grad_norm_partials() == PARTIALS
    out = K.grad_norm(view, max_norm)
    again = K.grad_norm(view, max_norm)
    assert _same_bits(out, again), what
    norm, coef = (float(v) for v in out.cpu().double())
    r = BO.grad_norm_ref(view, max_norm, PARTIALS)
    en = abs(norm - r["norm"][0]) / r["norm"][1] if r["norm"][1] > 0 else (0.0 if norm == r["norm"][0] else math.inf)
    ec = abs(coef - r["coef"][0]) / r["coef"][1] if r["coef"][1] > 0 else (0.0 if coef == r["coef"][0] else math.inf)
    print(f"[f64] grad_norm {what} max_norm {max_norm:.4g}: norm {norm!r} (err/bound {en:.3f}) coef {coef!r} (err/bound {ec:.3f})")
    assert en <= 1.0 and ec <= 1.0, (what, norm, r["norm"], coef, r["coef"])
    if r["exact_one"]:
        assert struct.unpack("<I", struct.pack("<f", coef))[0] == 0x3F800000, (what, coef)
    return norm, coef


@pytest.mark.parametrize("n,offset", [(1, 0), (255, 0), (256, 0), (257, 0), (2304, 0), (1000003, 0), (1000003, 3), ("engine", 0), ("engine", 1)])
def test_grad_norm_kernel(n, offset):
    """fewer elements than workgroups, ragged head and tail, a slice base that is only 4-byte aligned, and the engine's own count"""
    n = _engine_grad_count() if n == "engine" else n
    g = torch.from_numpy(np.random.RandomState(7100 + n % 997).standard_normal(n + offset).astype(np.float32))
    g[:: max(1, (n + offset) // 7)] = 1e4                       # a handful of outliers
    view = g.to(DEV)[offset:]
    assert view.data_ptr() % 16 == (4 * offset) % 16
    norm64 = math.sqrt(float((view.cpu().double() ** 2).sum()))
    _check_norm(view, 0.5 * norm64, f"n={n}+{offset} clipped")
    _check_norm(view, 2.0 * norm64, f"n={n}+{offset} max_norm above the norm")           # coef bits exactly 0x3f800000
    _check_norm(view, math.inf, f"n={n}+{offset} inf")
    zeros = torch.zeros(n + offset, device=DEV)[offset:]
    assert _check_norm(zeros, 1.0, f"n={n}+{offset} zeros") == (0.0, 1.0)


# ------------------------------------------------------------------------------------------------ engine helpers
def _net(dtype, classes=2):
    eng = _engine(dtype)
    ms, cs = build("finetune", "finetune", classes, True)
    ms.train(); cs.train()
    return eng, ms, cs, eng.bind(ms, cs)


def _fwd_bwd(eng, st, seed=7200, classes=2):
    x, y = C.u8(seed, (4, 3, 64, 64)), C.ints(seed + 1, (4,), classes)
    return eng.step_supervised(st, "ce", [x], y, train=True)


def _packs(st):
    """every block conv's train-mode shadow weights as the conv kernels read them (sslcr_net_debug_tensor kinds 15..20):
    forward and dgrad pack of conv1, conv2 and, in layer{2,3,4}.0, the projection"""
    out = {}
    for block in range(8):
        for kind in range(15, 21 if block in (2, 4, 6) else 19):
            out[(block, kind)] = st.debug_tensor(block, kind)[0]
    assert len(out) == 8 * 4 + 3 * 2
    return out


def _same_packs(a, b):
    pa, pb = _packs(a), _packs(b)
    for k in pa:
        assert pa[k].shape == pb[k].shape and torch.equal(pa[k].cpu().view(torch.int16 if pa[k].dtype == torch.bfloat16 else torch.int32),
                                                          pb[k].cpu().view(torch.int16 if pb[k].dtype == torch.bfloat16 else torch.int32)), k


def _groups(st):
    convs = [p for p in st.params if p.dim() == 4]
    vecs = [p for p in st.params if p.dim() == 1]            # every BatchNorm weight / bias and the heads' biases
    heads = [p for p in st.params if p.dim() == 2]
    return [dict(params=convs, lr=A_LR, weight_decay=B_WD), dict(params=vecs, weight_decay=0.0), dict(params=heads, lr=10 * A_LR)]


def _optimizer(name, groups):
    if name == "adam":
        return torch.optim.Adam(groups, lr=A_LR / 2, betas=(0.9, 0.999), weight_decay=B_WD / 4)
    if name == "adamw":
        return torch.optim.AdamW(groups, lr=A_LR / 2, betas=(0.9, 0.99), weight_decay=B_WD / 4)
    return torch.optim.SGD(groups, lr=A_LR / 2, momentum=0.9, weight_decay=B_WD / 4, nesterov=True)


def _seed_state(opt, params, seed=7300):
    """a non-zero state (the Adam denominator's bound needs v > 0), the same on every net that passes the same seed"""
    sgd = isinstance(opt, torch.optim.SGD)
    for i, p in enumerate(params):
        rs = np.random.RandomState(seed + i)
        m = torch.from_numpy(rs.standard_normal(tuple(p.shape)).astype(np.float32) * 1e-2).to(p.device)
        if sgd:
            opt.state[p] = dict(momentum_buffer=m)
        else:
            v = torch.from_numpy((np.abs(rs.standard_normal(tuple(p.shape))) * 1e-4 + 1e-6).astype(np.float32)).to(p.device)
            opt.state[p] = dict(step=torch.tensor(3.0), exp_avg=m, exp_avg_sq=v)


def _snapshot(opt, st):
    sgd = isinstance(opt, torch.optim.SGD)
    p = [q.detach().cpu().clone() for q in st.params]
    s1 = [opt.state[q]["momentum_buffer" if sgd else "exp_avg"].cpu().clone() for q in st.params]
    s2 = [None if sgd else opt.state[q]["exp_avg_sq"].cpu().clone() for q in st.params]
    return p, s1, s2


def _check_step(what, opt, st, before, grads, rows, gmap, coef=1.0):
    """every element of every parameter and state tensor against its group row's float64 bound; no element is excused"""
    sgd = isinstance(opt, torch.optim.SGD)
    p0, m0, v0 = before
    worst = 0.0
    for i, q in enumerate(st.params):
        row = rows[gmap[i]]
        ref = BO.optimizer_ref(row["kind"], p0[i].flatten(), grads[i].flatten(), m0[i].flatten(), None if sgd else v0[i].flatten(),
                               grad_scale=coef, **{k: v for k, v in row.items() if k != "kind"})
        got = dict(p=q, s1=opt.state[q]["momentum_buffer" if sgd else "exp_avg"])
        if not sgd:
            got["s2"] = opt.state[q]["exp_avg_sq"]
        for k, t in got.items():
            worst = max(worst, B.check(t.detach().flatten(), *ref[k], f"{what} {st.param_names[i]} (group {gmap[i]}) {k}", "optimizer_chunks_kernel", dims="i"))
    return worst


# ------------------------------------------------------------------------------------------------ 2. grouped step through the engine
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["adam", "adamw", "sgd"])
def test_grouped_step_holds_the_bounds(name, dtype):
    """three groups -- convs (lr a, wd b), BatchNorm parameters and biases (wd 0), head weights (lr 10a) -- cover all three branches
    of the chunks kernel: 3x3 convs with K and C multiples of 16 (LDS tiles), the 1x1 projections and the stem (parameter order),
    the vectors and the head matrices (plain)"""
    from ssl_cr_histo_amd import engine as E
    eng, ms, cs, st = _net(dtype)
    _fwd_bwd(eng, st)
    grads = [st.grad(i).cpu() for i in range(len(st.params))]
    opt = _optimizer(name, _groups(st))
    _seed_state(opt, st.params)
    before = _snapshot(opt, st)
    rows, gmap = E.plan_optimizer(opt, st.params, st.param_names)
    assert len(rows) == 3 and sorted(set(gmap)) == [0, 1, 2]
    st.optimizer_step(opt)
    assert st.last_grad_norm is None
    worst = _check_step(f"{name}/{dtype}", opt, st, before, grads, rows, gmap)
    print(f"[{dtype}] grouped {name}: worst err/bound {worst:.3f}")
    if name != "sgd":
        assert all(float(opt.state[q]["step"]) == 4.0 for q in st.params)


# ------------------------------------------------------------------------------------------------ 3. same bits as the one-row entry
@pytest.mark.parametrize("clip", [None, math.inf])
@pytest.mark.parametrize("name", ["adam", "sgd"])
def test_one_group_is_bit_equal_to_the_one_row_entry(name, clip):
    """one group through sslcr_net_optimizer_step_groups (BoundNet.optimizer_step) against sslcr_net_optimizer_step on a second net
    bound from a copy: parameters, state and both shadow packs of every block conv bit-equal, and so are the next train-mode
    forward and backward that read the packs.  sslcr_net_optimizer_step forwards to the grouped entry with one row and no
    clipping, so clip=None pins the two entries' plumbing (rows, group map, state pointers) to each other and clip=inf pins the
    coefficient path (coef exactly 1.0 read from the device) to the path without one.  Neither can show the parent's bits; the
    unchanged tests from before the group table (test_optimizer_step_f64, the fp32 post-step snapshots of the engine goldens) and
    a parent / this-library comparison of bench.py --dump-outputs (profiles/optim_groups_ab.txt) stand for that."""
    from ssl_cr_histo_amd import _lib as L
    eng, ms, cs, st = _net("bf16")
    ms2, cs2 = copy.deepcopy(ms), copy.deepcopy(cs)
    st2 = eng.bind(ms2, cs2)
    assert st2 is not st
    _fwd_bwd(eng, st); _fwd_bwd(eng, st2)
    for i in (0, 30, 65):
        assert _same_bits(st.grad(i), st2.grad(i))
    hp = dict(lr=1e-3, weight_decay=1e-2)
    mk = (lambda ps: torch.optim.Adam(ps, **hp)) if name == "adam" else (lambda ps: torch.optim.SGD(ps, momentum=0.9, nesterov=True, **hp))
    opt, opt2 = mk(st.params), mk(st2.params)
    _seed_state(opt, st.params); _seed_state(opt2, st2.params)
    st.optimizer_step(opt, max_grad_norm=clip)
    if clip is not None:
        assert float(st.last_grad_norm[1]) == 1.0 and float(st.last_grad_norm[0]) > 0.0
    sgd = name == "sgd"
    s1 = [opt2.state[q]["momentum_buffer" if sgd else "exp_avg"] for q in st2.params]
    s2 = [None if sgd else opt2.state[q]["exp_avg_sq"] for q in st2.params]
    a1, a2 = (CT.c_void_p * len(s1))(*[t.data_ptr() for t in s1]), (CT.c_void_p * len(s1))(*[None if t is None else t.data_ptr() for t in s2])
    o = (L.OptDesc(1, 1e-3, 0.0, 0.0, 0.0, 1e-2, 0.9, 1.0, 1.0, 0, 1.0) if sgd else
         L.OptDesc(0, 1e-3, 0.9, 0.999, 1e-8, 1e-2, 0.0, 1 - 0.9 ** 4, 1 - 0.999 ** 4, 0, 1.0))
    L.check(L.lib().sslcr_net_optimizer_step(st2.handle, CT.byref(o), a1, a2, L.stream_ptr()))
    st2._note_buffers_changed()
    torch.cuda.synchronize()
    for i, (p, q) in enumerate(zip(st.params, st2.params)):
        assert _same_bits(p, q), st.param_names[i]
        assert _same_bits(opt.state[p]["momentum_buffer" if sgd else "exp_avg"], s1[i]), st.param_names[i]
        if not sgd:
            assert _same_bits(opt.state[p]["exp_avg_sq"], s2[i]), st.param_names[i]
    _same_packs(st, st2)
    r, r2 = _fwd_bwd(eng, st, seed=7210), _fwd_bwd(eng, st2, seed=7210)
    assert _same_bits(r["logits"], r2["logits"]) and _same_bits(r["losses"], r2["losses"])
    for i in range(len(st.params)):
        assert _same_bits(st.grad(i), st2.grad(i)), st.param_names[i]


# ------------------------------------------------------------------------------------------------ 4. clipped step
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_clipped_grouped_step(dtype):
    """max_grad_norm = half the float64 norm of the fetched gradients: [norm, coef] within the bounds of test 1, the update within
    the bounds of test 2 with the reference fed the device's own coef (checked separately, as bn_bwd_apply_ref takes the
    kernel's own sums)"""
    from ssl_cr_histo_amd import engine as E
    eng, ms, cs, st = _net(dtype)
    _fwd_bwd(eng, st)
    grads = [st.grad(i).cpu() for i in range(len(st.params))]
    flat = torch.cat([g.flatten() for g in grads])
    norm64 = math.sqrt(float((flat.double() ** 2).sum()))
    assert norm64 > 0
    same = st.grad_norm(0.5 * norm64)
    opt = _optimizer("adamw", _groups(st))
    _seed_state(opt, st.params)
    before = _snapshot(opt, st)
    rows, gmap = E.plan_optimizer(opt, st.params, st.param_names)
    st.optimizer_step(opt, max_grad_norm=0.5 * norm64)
    norm, coef = (float(v) for v in st.last_grad_norm.cpu().double())
    assert _same_bits(same, st.last_grad_norm)                         # BoundNet.grad_norm: the same two kernels on their own
    # the kernel reduces the padded flat buffer: the padding is zero, so only the element COUNT of the bound changes
    r = BO.grad_norm_ref(flat, 0.5 * norm64, PARTIALS)
    e_norm = (2.0 ** -24 + (_engine_grad_count() + PARTIALS + 8) * 2.0 ** -53) * r["norm"][0]
    raw = B.f32(0.5 * norm64) / (r["norm"][0] + 1e-6)
    e_coef = 3 * B.U * raw + raw * e_norm / (r["norm"][0] + 1e-6)
    print(f"[{dtype}] clipped step: norm {norm!r} vs {r['norm'][0]!r} (err/bound {abs(norm - r['norm'][0]) / e_norm:.3f}), "
          f"coef {coef!r} (err/bound {abs(coef - raw) / e_coef:.3f})")
    assert abs(norm - r["norm"][0]) <= e_norm and abs(coef - raw) <= e_coef and 0.49 < coef < 0.51
    worst = _check_step(f"clipped adamw/{dtype}", opt, st, before, grads, rows, gmap, coef=coef)
    print(f"[{dtype}] clipped grouped adamw: worst err/bound {worst:.3f}")


# ------------------------------------------------------------------------------------------------ 5. shadow weights under groups
def test_shadow_weights_after_a_grouped_clipped_step():
    """bf16: the update writes the conv kernels' shadow packs itself.  The packs and the next train-mode forward must equal, bit for
    bit, those of a net freshly bound from the updated fp32 parameters (whose packs sslcr_net_pack derives)"""
    eng, ms, cs, st = _net("bf16")
    _fwd_bwd(eng, st)
    opt = _optimizer("adamw", _groups(st))
    _seed_state(opt, st.params)
    st.optimizer_step(opt, max_grad_norm=0.5 * float(st.grad_norm()[0]))
    assert 0.49 < float(st.last_grad_norm[1]) < 0.51
    ms2, cs2 = build("finetune", "finetune", 2, True)
    ms2.load_state_dict(ms.state_dict()); cs2.load_state_dict(cs.state_dict())
    ms2.train(); cs2.train()
    st2 = eng.bind(ms2, cs2)
    r, r2 = _fwd_bwd(eng, st, seed=7220), _fwd_bwd(eng, st2, seed=7220)
    assert _same_bits(r["logits"], r2["logits"]) and _same_bits(r["feats"], r2["feats"])
    _same_packs(st, st2)
    for i in (0, 3, 27, 60):
        assert _same_bits(st.grad(i), st2.grad(i)), st.param_names[i]             # (the dgrad packs, through the backward)


def test_clipped_step_with_a_frozen_prefix():
    """the norm is ONE reduction over the flat gradient buffer, which relies on frozen parameters' ranges (and the padding) being
    zero: after a full backward has filled every range, freeze the first 30 parameters (conv1 .. layer2.1), run another
    backward and clip -- [norm, coef] must be that of the trainable parameters' fetched gradients alone, the frozen parameters
    must keep their bits, the trainable ones hold the bounds"""
    from ssl_cr_histo_amd import engine as E
    eng, ms, cs, st = _net("fp32")
    _fwd_bwd(eng, st)                                      # every range of the buffer written once
    for p in st.params[:30]:
        p.requires_grad = False
    try:
        _fwd_bwd(eng, st, seed=7230)
        live = [i for i, p in enumerate(st.params) if p.requires_grad]
        assert live == list(range(30, 66))
        grads = {i: st.grad(i).cpu() for i in live}
        flat = torch.cat([g.flatten() for g in grads.values()])
        norm64 = math.sqrt(float((flat.double() ** 2).sum()))
        opt = torch.optim.AdamW([dict(params=[p for p in st.params[30:] if p.dim() != 1]),
                                 dict(params=[p for p in st.params[30:] if p.dim() == 1], weight_decay=0.0)], lr=A_LR, weight_decay=B_WD)
        _seed_state(opt, st.params[30:])
        frozen = [p.detach().cpu().clone() for p in st.params[:30]]
        p0 = {i: st.params[i].detach().cpu().clone() for i in live}
        m0 = {i: opt.state[st.params[i]]["exp_avg"].cpu().clone() for i in live}
        v0 = {i: opt.state[st.params[i]]["exp_avg_sq"].cpu().clone() for i in live}
        rows, gmap = E.plan_optimizer(opt, st.params, st.param_names)
        assert gmap[:30] == [-1] * 30
        st.optimizer_step(opt, max_grad_norm=0.5 * norm64)
        norm, coef = (float(v) for v in st.last_grad_norm.cpu().double())
        e_norm = (2.0 ** -24 + (_engine_grad_count() + PARTIALS + 8) * 2.0 ** -53) * norm64
        raw = B.f32(0.5 * norm64) / (norm64 + 1e-6)
        e_coef = 3 * B.U * raw + raw * e_norm / (norm64 + 1e-6)
        assert abs(norm - norm64) <= e_norm and abs(coef - raw) <= e_coef, (norm, norm64, coef, raw)
        for a, p in zip(frozen, st.params[:30]):
            assert _same_bits(a, p)
        for i in live:
            row = rows[gmap[i]]
            ref = BO.optimizer_ref(row["kind"], p0[i].flatten(), grads[i].flatten(), m0[i].flatten(), v0[i].flatten(), grad_scale=coef,
                                   **{k: v for k, v in row.items() if k != "kind"})
            B.check(st.params[i].detach().flatten(), *ref["p"], f"frozen prefix {st.param_names[i]} p", "optimizer_chunks_kernel", dims="i")
    finally:
        for p in st.params:
            p.requires_grad = True


# ------------------------------------------------------------------------------------------------ 6. virtual ranks
def test_virtual_ranks_hold_identical_norm_and_parameters():
    """world 2: each rank reduces the all-reduced gradient buffer on its own, in the same fixed order -- both must hold
    bit-identical [norm, coef] and, after the grouped clipped step, bit-identical parameters; no collective for the norm"""
    from ssl_cr_histo_amd import engine as E
    world, nx = 2, 4
    x, y = C.u8(7400, (nx, 3, 64, 64)), C.ints(7401, (nx,), 2)

    def one_step(eng, r):
        ms, cs = build("finetune", "finetune", 2, True)
        ms.train(); cs.train()
        st = eng.bind(ms, cs)
        lo, hi = r * nx // world, (r + 1) * nx // world
        eng.step_supervised(st, "ce", [x[lo:hi]], y[lo:hi], train=True, n_global=nx)
        free = st.grad_norm()
        opt = _optimizer("adamw", _groups(st))
        _seed_state(opt, st.params)
        st.optimizer_step(opt, max_grad_norm=0.5 * float(free[0]))
        torch.cuda.current_stream().synchronize()
        return dict(norm=st.last_grad_norm.cpu(), free=free.cpu(), params=[p.detach().cpu() for p in st.params])

    vc = E.VirtualComm(world)
    engines = [E.Engine(DEV, "fp32") for _ in range(world)]
    for r, e in enumerate(engines):
        e.init_comm_virtual(vc, r, world)
    a, b = _run_ranks(world, lambda r: one_step(engines[r], r))
    assert _same_bits(a["norm"], b["norm"]) and _same_bits(a["free"], b["free"]) and _same_bits(a["free"][:1], a["norm"][:1])
    assert 0.49 < float(a["norm"][1]) < 0.51
    for i, (p, q) in enumerate(zip(a["params"], b["params"])):
        assert _same_bits(p, q), i


# ------------------------------------------------------------------------------------------------ 7. steps pass-through
class _ClippedAdamW:
    """what the oracle's step functions call: zero_grad() / step() = clip_grad_norm_ then torch.optim.AdamW"""

    def __init__(self, p, max_norm, lr, wd):
        self.all = [v for v in p.values()]
        back = [v for k, v in p.items() if not k.startswith(("fc.", "classifier."))]
        head = [v for k, v in p.items() if k.startswith(("fc.", "classifier."))]
        assert len(back) == 60 and len(head) == 6
        self.opt = torch.optim.AdamW([dict(params=back), dict(params=head, lr=10 * lr, weight_decay=0.0)], lr=lr, weight_decay=wd)
        self.max_norm = max_norm

    def zero_grad(self):
        for v in self.all:
            v.grad = None

    def step(self):
        torch.nn.utils.clip_grad_norm_(self.all, self.max_norm)
        self.opt.step()


def _oracle_run(batches, hw, dtype, threads, max_norm, lr, wd):
    keep = torch.get_num_threads()
    torch.set_num_threads(threads)
    try:
        p_net, b_net, p_cls = oracle_state("finetune", 9, False)
        p = merged(p_net, p_cls)
        p = type(p)((k, v.to(dtype).requires_grad_(True)) for k, v in p.items())
        b = type(b_net)((k, v.to(dtype) if v.is_floating_point() else v.clone()) for k, v in b_net.items())
        opt = _ClippedAdamW(p, max_norm, lr, wd)
        losses, accs = [], []
        for xb, yb in batches:
            x = xb.reshape(-1, 3, hw, hw).to(dtype)
            r = S.supervised_step("ce", p, b, opt, x, yb.reshape(-1).long())
            losses.append(r["loss"])
            accs.append(r["acc"])
        out = {k: v.detach().double() for k, v in p.items()}
        out.update({k: v.double() for k, v in b.items() if v.is_floating_point()})
        out["loss_steps"] = torch.tensor(losses, dtype=torch.float64)
        out["acc_steps"] = torch.tensor(accs, dtype=torch.float64)
        return out
    finally:
        torch.set_num_threads(keep)


def _dist(a, b):
    a, b = torch.as_tensor(a).double().flatten(), torch.as_tensor(b).double().flatten()
    return float((a - b).norm() / (b.norm() + 1e-300))


def test_kather_sup_train_passes_clip_grad_norm_through():
    """steps.kather_sup_train with args.clip_grad_norm and a two-group AdamW (fp32 engine) against the same three steps of the
    oracle on the CPU with torch.optim.AdamW and clip_grad_norm_.  The trajectory-yardstick rule: the CPU oracle runs in float64
    and in float32 at 1 and at 8 threads; per key (every parameter and BatchNorm running statistic) the engine's relative L2
    distance from the float64 run may be at most 4 x the larger float32 distance (a different reduction order over three
    steps).  A key on which both float32 runs equal float64 to the bit is held to 1e-6.

    That per-key rule is the issue's, and it is applied as stated.  The checks of the returned values are additional to it:
    the same three steps run once more, one batch per call on a second pair of modules, so that every step's loss is seen, and
    each step's loss holds the same rule on its own (at most 4 x the larger float32 distance of THAT step's loss).  The
    returned loss must be the mean of those three (1e-6) and, as a consequence of the per-step bounds and of losses being
    positive, lies within 4 x the largest per-step float32 distance.  It is NOT compared with the distance of the float32
    runs' average: one run's per-step errors have either sign and cancel there by luck (measured: -1.8e-4 and +2.9e-4 at steps
    2 and 3 give 8.1e-5 on the average, against which the engine's 4.7e-4 would be 5.8 x; the two thread counts are nearly the
    same computation, so the second run is no independent draw).  Measured on the MI355X: engine per-step 6.5e-4 and 3.4e-4
    (3.7 x and 1.2 x the float32 runs' 1.8e-4 and 2.9e-4; step 1 equals them to the bit).  The returned accuracy may differ
    from the float64 run's by one of the 18 predictions (the allowance the Kather config-1 test gives the fp32 engine)."""
    from ssl_cr_histo_amd import steps
    hw, lr, wd, max_norm = 64, 1e-3, 1e-2, 1.0
    batches = [(C.u8(7500 + i, (2, 3, 3, hw, hw)), C.ints(7550 + i, (2, 3), 9)) for i in range(3)]
    _engine("fp32")
    ms, cs = build("finetune", "finetune", 9, False)
    named = list(ms.named_parameters())
    back = [p for k, p in named if not k.startswith("fc.")]
    head = [p for k, p in named if k.startswith("fc.")] + list(cs.parameters())
    assert len(back) == 60 and len(head) == 6
    opt = torch.optim.AdamW([dict(params=back), dict(params=head, lr=10 * lr, weight_decay=0.0)], lr=lr, weight_decay=wd)
    ret = steps.kather_sup_train(ns(image_size=hw, clip_grad_norm=max_norm), ms, cs, batches, torch.nn.CrossEntropyLoss(), opt, 1)
    got = {k: v.double() for k, v in state_of(ms, cs).items() if v.is_floating_point()}
    ref64 = _oracle_run(batches, hw, torch.float64, 8, max_norm, lr, wd)
    ref32 = [_oracle_run(batches, hw, torch.float32, t, max_norm, lr, wd) for t in (1, 8)]
    l64, a64 = ref64.pop("loss_steps"), float(ref64.pop("acc_steps").mean())
    l32 = [r.pop("loss_steps") for r in ref32]
    for r in ref32:
        r.pop("acc_steps")
    # the same steps, one batch per call, for the per-step losses
    ms1, cs1 = build("finetune", "finetune", 9, False)
    named1 = list(ms1.named_parameters())
    opt1 = torch.optim.AdamW([dict(params=[p for k, p in named1 if not k.startswith("fc.")]),
                              dict(params=[p for k, p in named1 if k.startswith("fc.")] + list(cs1.parameters()), lr=10 * lr, weight_decay=0.0)],
                             lr=lr, weight_decay=wd)
    steps_l = [float(steps.kather_sup_train(ns(image_size=hw, clip_grad_norm=max_norm), ms1, cs1, [b], torch.nn.CrossEntropyLoss(), opt1, 1)[0])
               for b in batches]
    for t in range(3):
        yard_t = max(abs(float(r[t] - l64[t])) / float(l64[t]) for r in l32)
        d_t = abs(steps_l[t] - float(l64[t])) / float(l64[t])
        print(f"[fp32] step {t + 1} loss {steps_l[t]!r} vs float64 {float(l64[t])!r}: rel {d_t:.3e}, float32 distance {yard_t:.3e}")
        assert d_t <= (4 * yard_t if yard_t > 0 else 1e-6), (t, d_t, yard_t)
    assert abs(float(ret[0]) - float(np.mean(steps_l))) <= 1e-6 * float(np.mean(steps_l)), (ret[0], steps_l)
    yard_loss = max(float(((r - l64).abs() / l64.abs()).max()) for r in l32)
    d_loss = abs(float(ret[0]) - float(l64.mean())) / float(l64.mean())
    print(f"[fp32] returned loss {float(ret[0])!r} vs float64 {float(l64.mean())!r}: rel {d_loss:.3e}, largest float32 per-step distance {yard_loss:.3e}")
    assert yard_loss > 0 and d_loss <= 4 * yard_loss, (d_loss, yard_loss)
    assert abs(float(ret[1]) - a64) <= 1.0 / 18 + 1e-9, (ret[1], a64)
    assert set(got) == set(ref64), set(got) ^ set(ref64)
    worst, worst_key = 0.0, None
    fails = []
    for k in sorted(ref64):
        yard = max(_dist(r[k], ref64[k]) for r in ref32)
        d = _dist(got[k], ref64[k])
        if yard == 0.0:
            if d > 1e-6:
                fails.append((k, d, "float32 runs equal float64 to the bit: 1e-6"))
            continue
        if d / yard > worst:
            worst, worst_key = d / yard, k
        if d > 4 * yard:
            fails.append((k, d, yard))
    print(f"[fp32] kather_sup_train, clipped two-group AdamW, three steps: worst engine / float32-oracle distance ratio {worst:.3f} at {worst_key}")
    assert not fails, fails
