"""Gradient accumulation on the MI355X (include/sslcr.h, library version 9): sslcr_grad_accumulate alone, the engine's ordered
sum prev + new in every mode, off == the behaviour without it, frozen prefixes, the oracle's accumulated .grad, clipping of the
sum, the epoch functions with args.micro_batches and the sharded path.  The network is the fixed ResNet18, so the small problem is
64x64 inputs (layer4 sees 2x2) with 1-4 images per micro-batch (256x256 where eval_BreastPathQ_SSL_CR hard-codes it)."""
import copy
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import cases as C  # noqa: E402
from oracle import steps as S  # noqa: E402

import _f64 as B  # noqa: E402
import _f64_optim as BO  # noqa: E402
from _util import merged, oracle_state, rel_err  # noqa: E402
from test_engine_gpu import DEV, TOLS, _engine, build, freeze, ns, relx, state_of  # noqa: E402
from test_engine_gpu2 import _run_ranks  # noqa: E402
from test_optim_groups_gpu import (PARTIALS, _bits, _check_step, _engine_grad_count, _groups, _optimizer, _same_bits,  # noqa: E402
                                   _seed_state, _snapshot)

HW = 64


# ------------------------------------------------------------------------------------------------ 1. the kernel alone
def _same_or_both_nan(got, want, what):
    got, want = got.cpu(), want.cpu()
    assert torch.equal(torch.isnan(got), torch.isnan(want)), what
    ok = ~torch.isnan(want)
    assert torch.equal(_bits(got)[ok], _bits(want)[ok]), what


@pytest.mark.parametrize("offs", [(0, 0), (1, 0), (0, 3), (1, 3)])
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 2304, 1000003, "engine"])
def test_grad_accumulate_kernel(n, offs):
    """dst[i] = dst[i] + src[i] bit for bit against torch CPU: fewer elements than one quad, ragged head and tail, more than one
    trip of the grid, the engine's own gradient count; bases 0 / 4 / 12 bytes past a 16-byte boundary, each side on its own; the
    four guard elements on either side of both ranges keep their bits; two runs agree"""
    from ssl_cr_histo_amd import kernels as K
    n = _engine_grad_count() if n == "engine" else n
    G = 4
    rs = np.random.RandomState(7600 + n % 991 + 7 * offs[0] + offs[1])

    def data(off):
        t = torch.from_numpy(rs.standard_normal(G + off + n + G).astype(np.float32))
        v = t[G + off:G + off + n]
        if n:
            v[::max(1, n // 7)] = 1e4                                        # a handful of outliers
        return t, v
    (dbuf, dv), (sbuf, sv) = data(offs[0]), data(offs[1])
    inf, nan = math.inf, math.nan
    # zeros of both signs against each other, infinities (inf + -inf = NaN), NaN on either side
    special = [(0.0, 0.0), (-0.0, -0.0), (0.0, -0.0), (-0.0, 0.0), (inf, 1.0), (1.0, -inf), (inf, -inf), (inf, inf), (nan, 1.0), (2.0, nan),
               (-0.0, 3.0)]
    for j, (a, b) in enumerate(special):
        if n:
            i = (j * 23 + 1) % n
            dv[i], sv[i] = a, b
    want = dbuf.clone()
    want[G + offs[0]:G + offs[0] + n] = dv + sv                               # torch CPU: one fp32 add per element
    runs = []
    for _ in range(2):
        d, s = dbuf.to(DEV), sbuf.to(DEV)
        dview, sview = d[G + offs[0]:G + offs[0] + n], s[G + offs[1]:G + offs[1] + n]
        if n:
            assert dview.data_ptr() % 16 == 4 * offs[0] and sview.data_ptr() % 16 == 4 * offs[1]
        K.grad_accumulate(dview, sview)
        torch.cuda.synchronize()
        _same_or_both_nan(d, want, f"n={n} offsets {offs}: dst (guards included)")
        _same_or_both_nan(s, sbuf, f"n={n} offsets {offs}: src was written")
        runs.append(d.cpu())
    assert torch.equal(_bits(runs[0]), _bits(runs[1]))


# ------------------------------------------------------------------------------------------------ engine helpers
def _nets(workload, classes=None):
    if workload == "rsp":
        return build("triplet", "mlp", 6, False)
    return build("finetune", "finetune", classes if classes is not None else (1 if workload == "ssl_cr_mse" else 2), True)


def _inputs(workload, nx, nu, seed):
    if workload == "rsp":
        return dict(xs=[C.u8(seed + j, (nx, 3, HW, HW)) for j in range(3)], y=C.ints(seed + 9, (nx,), 6))
    kind = "mse" if workload == "ssl_cr_mse" else "ce"
    return dict(x=C.u8(seed, (nx, 3, HW, HW)), u_w=C.u8(seed + 1, (nu, 3, HW, HW)), u_s=C.u8(seed + 2, (nu, 3, HW, HW)),
                y=C.f32(seed + 3, (nx,)) if kind == "mse" else C.ints(seed + 3, (nx,), 2), kind=kind)


class _Side:
    """one (student[, teacher]) pair bound to the engine; micro(j) runs micro-batch j of k with the FULL batch's global counts"""

    def __init__(self, eng, workload, ms, cs, mt=None, ct=None):
        self.eng, self.workload, self.ms, self.cs = eng, workload, ms, cs
        ms.train(); cs.train()
        self.st = eng.bind(ms, cs)
        self.te = None
        if mt is not None:
            freeze(mt, 64)
            mt.eval(); ct.eval()
            self.te = eng.bind(mt, ct)

    def clone(self):
        mt = copy.deepcopy(self.te.model) if self.te is not None else None
        ct = copy.deepcopy(self.te.classifier) if self.te is not None else None
        return _Side(self.eng, self.workload, copy.deepcopy(self.ms), copy.deepcopy(self.cs), mt, ct)

    def micro(self, d, j, k, accumulate, world=1):
        from ssl_cr_histo_amd import steps
        if self.workload == "rsp":
            n = d["y"].shape[0]
            a, b = steps.micro_ranges(n, k)[j]
            return self.eng.step_supervised(self.st, "ce", [x[a:b] for x in d["xs"]], d["y"][a:b], train=True, n_global=n * world,
                                            accumulate=accumulate)
        nx, nu = d["x"].shape[0], d["u_w"].shape[0]
        (a, b), (c, e) = steps.micro_ranges(nx, k)[j], steps.micro_ranges(nu, k)[j]
        return self.eng.step_ssl_cr(self.te, self.st, d["kind"], d["x"][a:b], d["y"][a:b], d["u_w"][c:e], d["u_s"][c:e], 0.7,
                                    nx_global=nx * world, nu_global=nu * world, accumulate=accumulate)

    def grads(self):
        return [self.st.grad(i).cpu() for i in range(len(self.st.params))]

    def state(self):
        return state_of(self.ms, self.cs)


def _pair(dtype, workload, classes=None):
    eng = _engine(dtype)
    ms, cs = _nets(workload, classes)
    mt, ct = (None, None) if workload == "rsp" else _nets(workload, classes)
    a = _Side(eng, workload, ms, cs, mt, ct)
    return eng, a, a.clone()


def _ordered_sum(parts):
    """((g0 + g1) + g2) ... per parameter, in fp32 on the CPU"""
    out = [g.clone() for g in parts[0]]
    for p in parts[1:]:
        out = [a + b for a, b in zip(out, p)]
    return out


def _assert_same_state(a, b, what):
    sa, sb = a.state(), b.state()
    assert set(sa) == set(sb)
    for key, v in sa.items():
        if v.is_floating_point():
            assert _same_bits(v, sb[key]), (what, key)
        else:
            assert torch.equal(v, sb[key]), (what, key)


def _accumulate_and_compare(a, b, d, k, what):
    """A accumulates (j > 0), B runs the same sequence without and is read after every micro-step: A's gradient must be the ordered
    fp32 sum of B's, bit for bit, and every buffer the forwards update must have evolved identically"""
    parts = []
    for j in range(k):
        ra, rb = a.micro(d, j, k, accumulate=j > 0), b.micro(d, j, k, accumulate=False)
        assert _same_bits(ra["losses"], rb["losses"]) and _same_bits(ra["logits"], rb["logits"]), (what, j)
        parts.append(b.grads())
    want = _ordered_sum(parts)
    for i, (g, w) in enumerate(zip(a.grads(), want)):
        assert _same_bits(g, w), (what, a.st.param_names[i])
    _assert_same_state(a, b, what)
    return want


# ------------------------------------------------------------------------------------------------ 2. + 3. ordered sum; off means off
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp8"])
@pytest.mark.parametrize("workload", ["ssl_cr_mse", "ssl_cr_ce", "rsp"])
def test_accumulated_gradient_is_the_ordered_sum(workload, dtype):
    """three ragged micro-steps (SSL_CR: nx = 5 -> 2, 2, 1 and nu = 7 -> 3, 2, 2; RSP: n = 6) on two deep-copied nets of one engine.
    B runs the same sequence (not each micro-batch alone), so the states -- the fp8 delayed scales included -- evolve identically.
    Then one more step with accumulate=False on both: off means off, the accumulated buffer leaves no trace"""
    eng, a, b = _pair(dtype, workload)
    d = _inputs(workload, 6 if workload == "rsp" else 5, 7, 7700)
    _accumulate_and_compare(a, b, d, 3, f"{workload}/{dtype}")
    d2 = _inputs(workload, 4, 4, 7720)
    ra, rb = a.micro(d2, 0, 1, accumulate=False), b.micro(d2, 0, 1, accumulate=False)
    assert _same_bits(ra["losses"], rb["losses"])
    for i, (g, w) in enumerate(zip(a.grads(), b.grads())):
        assert _same_bits(g, w), ("off after on", a.st.param_names[i])
    _assert_same_state(a, b, "off after on")


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_on_before_the_first_backward_is_off(dtype):
    """a net that has had no backward has no prev: set_grad_accumulate(1) before its FIRST backward gives the bits of a net that
    never accumulated (no read of an unwritten buffer)"""
    eng, a, b = _pair(dtype, "ssl_cr_ce")
    d = _inputs("ssl_cr_ce", 4, 4, 7740)
    from ssl_cr_histo_amd import _lib as L
    xin = torch.cat((d["x"], d["u_s"]))
    _, logits = b.st.forward((xin,), train=True)
    dl = torch.from_numpy(np.random.RandomState(7741).standard_normal(tuple(logits.shape)).astype(np.float32)).to(DEV)
    b.st.backward(dl)
    want = b.grads()

    def raw_backward():
        """a fresh train-mode forward (the gradient depends on the batch statistics only), then sslcr_net_backward itself: the
        net's sticky mode decides, not BoundNet.backward's argument"""
        _, lg = a.st.forward((xin,), train=True)
        assert _same_bits(lg, logits)
        L.check(L.lib().sslcr_net_backward(a.st.handle, L.ptr(dl), L.stream_ptr()))
        return a.grads()
    a.st.set_grad_accumulate(1)
    for i, (g, w) in enumerate(zip(raw_backward(), want)):
        assert _same_bits(g, w), a.st.param_names[i]
    for i, (g, w) in enumerate(zip(raw_backward(), want)):              # sticky: the second backward adds
        assert _same_bits(g, w + w), a.st.param_names[i]
    a.st.forward((xin,), train=True)
    a.st.backward(dl)                                                   # BoundNet.backward sets the mode on every call: default off
    for i, (g, w) in enumerate(zip(a.grads(), want)):
        assert _same_bits(g, w), a.st.param_names[i]


# ------------------------------------------------------------------------------------------------ 4. frozen prefix
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_frozen_prefix_is_neither_touched_nor_paid_for(dtype):
    """the reference's default freeze (60: heads only) with k = 2, after a full backward has written every range of the buffer:
    the same ordered-sum equality, and every frozen parameter's gradient range is all zero"""
    eng, a, b = _pair(dtype, "ssl_cr_mse")
    d = _inputs("ssl_cr_mse", 4, 6, 7760)
    for s in (a, b):
        s.micro(d, 0, 1, accumulate=False)                      # every range written once
    assert float(a.st.grad(0).abs().max()) > 0
    for s in (a, b):
        freeze(s.ms, 60)
    _accumulate_and_compare(a, b, d, 2, f"freeze 60/{dtype}")
    for i in range(60):
        assert not a.st.params[i].requires_grad and float(a.st.grad(i).abs().max()) == 0.0, a.st.param_names[i]
    assert all(float(a.st.grad(i).abs().max()) > 0 for i in range(60, 66))


# ------------------------------------------------------------------------------------------------ 5. against the oracle
class _NoStep:
    """what oracle.steps calls around loss.backward(): nothing is cleared and nothing updated, so .grad accumulates"""

    def zero_grad(self):
        pass

    def step(self):
        pass


def _oracle_nets(dtype, workload, classes):
    if workload == "rsp":
        p_net, b_net, p_cls = oracle_state("mlp", 6, False)
    else:
        p_net, b_net, p_cls = oracle_state("finetune", classes, True)
    p = merged(p_net, p_cls)
    p = type(p)((k, v.to(dtype).requires_grad_(True)) for k, v in p.items())
    b = type(b_net)((k, v.to(dtype) if v.is_floating_point() else v.clone()) for k, v in b_net.items())
    return p, b


def _oracle_accumulate(ps, bs, pt, bt, d, k, dtype, lambda_u=0.7):
    """oracle.steps.ssl_cr_step per micro-batch (equal cuts) with the no-op optimizer: .grad accumulates, then / k.
    -> (mean of the micro losses [loss, loss_x, loss_u] = the global-batch loss, feats in the single step's row order)"""
    from ssl_cr_histo_amd import steps
    nx, nu = d["x"].shape[0], d["u_w"].shape[0]
    assert nx % k == 0 and nu % k == 0, "the / k composition needs equal cuts"
    losses, fx, fu = np.zeros(3), [], []
    for (a, b), (c, e) in zip(steps.micro_ranges(nx, k), steps.micro_ranges(nu, k)):
        y = d["y"][a:b]
        r = S.ssl_cr_step(d["kind"], ps, bs, pt, bt, _NoStep(), d["x"][a:b].to(dtype), y.to(dtype) if d["kind"] == "mse" else y,
                          d["u_w"][c:e].to(dtype), d["u_s"][c:e].to(dtype), lambda_u)
        losses += np.array([r["loss"], r["loss_x"], r["loss_u"]]) / k
        fx.append(r["feats"][:b - a]); fu.append(r["feats"][b - a:])
    with torch.no_grad():
        for v in ps.values():
            if v.grad is not None:
                v.grad /= k
    return losses, torch.cat(fx + fu)


def _l2(a, b):
    a, b = torch.as_tensor(a).double().flatten(), torch.as_tensor(b).double().flatten()
    return float((a - b).norm() / (b.norm() + 1e-300))


def test_accumulated_gradient_vs_the_oracle():
    """one ssl_cr_mse step, nx = 4, nu = 6, k = 2 in fp32 mode against the oracle's accumulated .grad (float64 copies), per
    parameter within max(3e-3, 3 x the oracle's own fp32-vs-float64 relative L2): DESIGN section 2's fp32 gradient rule; the
    summed losses within 1e-3 of the global-batch loss"""
    eng, a, _ = _pair("fp32", "ssl_cr_mse")
    d = _inputs("ssl_cr_mse", 4, 6, 7780)
    k = 2
    res = [a.micro(d, j, k, accumulate=j > 0) for j in range(k)]
    got = [g.double() for g in a.grads()]
    losses = torch.stack([r["losses"] for r in res]).sum(0).cpu().double()
    ref = {}
    for dt in (torch.float32, torch.float64):
        ps, bs = _oracle_nets(dt, "ssl_cr_mse", 1)
        pt, bt = _oracle_nets(dt, "ssl_cr_mse", 1)
        l, _ = _oracle_accumulate(ps, bs, pt, bt, d, k, dt)
        ref[dt] = (l, [v.grad.detach().double() for v in ps.values()])
    l64, g64 = ref[torch.float64]
    bad = []
    for i, name in enumerate(a.st.param_names):
        yard = _l2(ref[torch.float32][1][i], g64[i])
        e = _l2(got[i], g64[i])
        print(f"   {i:2d} {name:44s} engine {e:.2e}  oracle fp32 {yard:.2e}")
        if e > max(3e-3, 3 * yard):
            bad.append((name, e, yard))
    assert not bad, bad
    for i in range(3):
        assert abs(float(losses[i]) - l64[i]) <= 1e-3 * abs(l64[i]), (i, losses, l64)


# ------------------------------------------------------------------------------------------------ 6. clipping sees the sum
def test_clipping_sees_the_accumulated_gradient():
    """after an accumulated backward grad_norm() is the norm of what grad(i) reads back (the bound of test_clipped_grouped_step),
    and optimizer_step(max_grad_norm = half of it) updates within _f64_optim.optimizer_ref's bounds for that coefficient"""
    from ssl_cr_histo_amd import engine as E
    eng, a, _ = _pair("fp32", "ssl_cr_ce")
    d = _inputs("ssl_cr_ce", 4, 6, 7800)
    single = a.clone()
    for j in range(2):
        a.micro(d, j, 2, accumulate=j > 0)
    single.micro(d, 1, 2, accumulate=False)
    st = a.st
    grads = a.grads()
    assert not _same_bits(grads[0], single.grads()[0])                      # (the sum, not the last micro-step's gradient)
    flat = torch.cat([g.flatten() for g in grads])
    r = BO.grad_norm_ref(flat, math.inf, PARTIALS)
    norm64 = r["norm"][0]
    e_norm = (2.0 ** -24 + (_engine_grad_count() + PARTIALS + 8) * 2.0 ** -53) * norm64
    free = st.grad_norm()
    assert abs(float(free[0]) - norm64) <= e_norm and float(free[1]) == 1.0, (free, norm64)
    opt = _optimizer("adamw", _groups(st))
    _seed_state(opt, st.params)
    before = _snapshot(opt, st)
    rows, gmap = E.plan_optimizer(opt, st.params, st.param_names)
    st.optimizer_step(opt, max_grad_norm=0.5 * norm64)
    norm, coef = (float(v) for v in st.last_grad_norm.cpu().double())
    raw = B.f32(0.5 * norm64) / (norm64 + 1e-6)
    e_coef = 3 * B.U * raw + raw * e_norm / (norm64 + 1e-6)
    assert abs(norm - norm64) <= e_norm and abs(coef - raw) <= e_coef and 0.49 < coef < 0.51, (norm, norm64, coef, raw)
    worst = _check_step("clipped adamw on the accumulated gradient", opt, st, before, grads, rows, gmap, coef=coef)
    print(f"[fp32] clipped step on an accumulated gradient: worst err/bound {worst:.3f}")


# ------------------------------------------------------------------------------------------------ 7. the epoch functions
def _oracle_clip_and_step(ps, opt, max_norm):
    torch.nn.utils.clip_grad_norm_([v for v in ps.values() if v.grad is not None], max_norm)
    opt.step()
    for v in ps.values():
        v.grad = None


def _check_state(got, ps, bs, rtol):
    """tests/_util.check_snapshot's two rules -- L2 norm and largest element error relative to the tensor's largest element -- on
    EVERY tensor of the oracle's post-epoch state; num_batches_tracked exactly"""
    want = {k: v.detach() for k, v in ps.items()}
    want.update(bs)
    assert set(want) <= set(got), set(want) - set(got)
    for k, w in want.items():
        g = got[k]
        if not w.is_floating_point():
            assert int(g) == int(w), (k, int(g), int(w))
            continue
        l2 = float(w.double().norm())
        assert abs(float(g.double().norm()) - l2) <= rtol * l2 + 1e-6, (k, "l2")
        scale = float(w.abs().max()) + 1e-12
        err = float((g.float() - w).abs().max())
        assert err <= rtol * scale + 1e-7, (k, err, scale)


def _same_outputs(r1, r2, what):
    for x, y in zip(r1, r2):
        if torch.is_tensor(x):
            assert _same_bits(x, y) if x.is_floating_point() else torch.equal(x.cpu(), y.cpu()), what
        else:
            assert x == y, what


def test_bpq_cr_epoch_with_micro_batches():
    """steps.bpq_cr_train, fp32, two loader batches (6 labeled + 4 unlabeled 256x256 images each: eval_BreastPathQ_SSL_CR
    hard-codes the side), micro_batches = 2, clip_grad_norm set, against the oracle composition of the test above followed by
    clip_grad_norm_ and the oracle's Adam: the tolerances test_bpq_cr_epoch_vs_reference applies to its fp32 rows (1e-3 on the
    returned averages and features, 5e-3 on the post-epoch state); shapes as with k = 1; micro_batches = 1 == no attribute"""
    from ssl_cr_histo_amd import steps
    _engine("fp32")
    lr, wd, lam, max_norm, k = 1e-4, 1e-4, 1.0, 1.0, 2
    labeled = [(C.u8(7900 + i, (2, 3, 3, 256, 256)), C.f32(7950 + i, (2, 3))) for i in range(2)]
    unlabeled = [(C.u8(7910 + i, (4, 3, 256, 256)), C.u8(7960 + i, (4, 3, 256, 256))) for i in range(2)]

    def run(**extra):
        mt, ct = build("finetune", "finetune", 1, True)
        ms, cs = build("finetune", "finetune", 1, True)
        freeze(mt, 64)
        opt = torch.optim.Adam(list(ms.parameters()) + list(cs.parameters()), lr=lr, betas=(0.9, 0.999), weight_decay=wd)
        ret = steps.bpq_cr_train(ns(lambda_u=lam, clip_grad_norm=max_norm, **extra), mt, ms, ct, cs, labeled, unlabeled, opt, 1)
        return ret, state_of(ms, cs)
    ret, state = run(micro_batches=k)
    # the oracle: per loader batch k accumulating micro-steps, / k, clip, Adam
    ps, bs = _oracle_nets(torch.float32, "ssl_cr_mse", 1)
    pt, bt = _oracle_nets(torch.float32, "ssl_cr_mse", 1)
    oopt = S.Adam(ps.values(), lr, (0.9, 0.999), 1e-8, wd)
    avg, feats = np.zeros(3), []
    for (x, y), (u_w, u_s) in zip(labeled, unlabeled):
        d = dict(x=x.reshape(-1, 3, 256, 256), y=y.reshape(-1), u_w=u_w, u_s=u_s, kind="mse")
        l, f = _oracle_accumulate(ps, bs, pt, bt, d, k, torch.float32, lam)
        _oracle_clip_and_step(ps, oopt, max_norm)
        avg += l / len(labeled)
        feats.append(f)
    ts, tf, tp = TOLS["fp32"]
    for i in range(3):
        assert relx(ret[i], avg[i]) <= ts, (i, ret[i], avg[i])
    assert rel_err(ret[3].cpu(), torch.cat(feats)) <= tf
    assert torch.equal(ret[4].cpu(), torch.cat([y for _, y in labeled]))
    _check_state(state, ps, bs, tp)
    ret1, state1 = run(micro_batches=1)
    ret0, state0 = run()
    assert [tuple(t.shape) for t in ret[3:]] == [tuple(t.shape) for t in ret0[3:]] and len(ret) == len(ret0)
    _same_outputs(ret1, ret0, "micro_batches = 1 vs no attribute")
    for key, v in state0.items():
        assert torch.equal(v, state1[key]), key
    with pytest.raises(ValueError) as e:
        run(micro_batches=5)                                  # nu = 4
    assert "5" in str(e.value) and "6" in str(e.value) and "4" in str(e.value)


def test_rsp_epoch_with_micro_batches():
    """steps.rsp_train (_rsp_epoch), fp32, two loader batches of 8 triplets at 64x64, micro_batches = 2, clip_grad_norm set,
    against oracle.steps.rsp_step per micro-batch with the no-op optimizer, / k, clip_grad_norm_, the oracle's SGD-Nesterov:
    the tolerances test_rsp_epoch_and_lookahead_vs_reference applies to its fp32 rows; rsp_validate ignores the attribute"""
    from ssl_cr_histo_amd import steps
    _engine("fp32")
    lr, wd, max_norm, k, n = 0.01, 1e-4, 1.0, 2, 8
    batches = [(C.u8(8000 + i, (n, 3, HW, HW)), C.u8(8020 + i, (n, 3, HW, HW)), C.u8(8040 + i, (n, 3, HW, HW)),
                C.ints(8060 + i, (n, 1), 6).to(torch.uint8)) for i in range(2)]

    def run(**extra):
        model, cls = build("triplet", "mlp", 6, False)
        opt = torch.optim.SGD(list(model.parameters()) + list(cls.parameters()), lr=lr, momentum=0.9, weight_decay=wd, nesterov=True)
        args = ns(tile_h=HW, tile_w=HW, clip_grad_norm=max_norm, **extra)
        ret = steps.rsp_train(args, model, cls, batches, torch.nn.CrossEntropyLoss(), opt, 1)
        return ret, state_of(model, cls), (args, model, cls)
    ret, state, (args, model, cls) = run(micro_batches=k)
    ps, bs = _oracle_nets(torch.float32, "rsp", 6)
    oopt = S.SGDNesterov(ps.values(), lr, 0.9, wd)
    loss = correct = 0.0
    feats = []
    for i1, i2, i3, t in batches:
        t = t.long().reshape(-1)
        for a, b in steps.micro_ranges(n, k):
            r = S.rsp_step(ps, bs, _NoStep(), i1[a:b].float(), i2[a:b].float(), i3[a:b].float(), t[a:b], True)
            loss += r["loss"] / k / len(batches)
            correct += r["acc"] * (b - a)
            feats.append(r["feats"])
        with torch.no_grad():
            for v in ps.values():
                v.grad /= k
        _oracle_clip_and_step(ps, oopt, max_norm)
    ts, tf, tp = TOLS["fp32"]
    assert relx(ret[0], loss) <= ts, (ret[0], loss)
    assert ret[1] == correct / (n * len(batches)), (ret[1], correct)
    assert rel_err(ret[2].cpu(), torch.cat(feats)) <= tf
    assert torch.equal(ret[3].cpu(), torch.cat([t.long().reshape(-1) for *_, t in batches]))
    _check_state(state, ps, bs, tp)
    v2 = steps.rsp_validate(args, model, cls, batches, torch.nn.CrossEntropyLoss(), 1)        # micro_batches still set: ignored
    v1 = steps.rsp_validate(ns(tile_h=HW, tile_w=HW), model, cls, batches, torch.nn.CrossEntropyLoss(), 1)
    assert v1 == v2
    ret1, state1, _ = run(micro_batches=1)
    ret0, state0, _ = run()
    assert [tuple(t.shape) for t in ret[2:]] == [tuple(t.shape) for t in ret0[2:]] and len(ret) == len(ret0)
    _same_outputs(ret1, ret0, "micro_batches = 1 vs no attribute")
    for key, v in state0.items():
        assert torch.equal(v, state1[key]), key
    with pytest.raises(ValueError) as e:
        run(micro_batches=9)
    assert "9" in str(e.value) and "8" in str(e.value)


# ------------------------------------------------------------------------------------------------ 8. sharded
def test_virtual_ranks_accumulate_identically():
    """world 2 (virtual ranks), k = 2, fp32, ssl_cr_mse: the sum is taken after the bucket all-reduces, so both ranks add identical
    buffers -- identical parameter bits after the optimizer step -- and their gradient is, within the 2e-5 relative L2 of
    test_virtual_ranks_equal_the_single_device_step at world 2, that of the 1-rank k = 2 run whose micro-batch j is the
    concatenation of the ranks' micro-batch j"""
    from ssl_cr_histo_amd import engine as E
    world, k, nx, nu = 2, 2, 8, 12                        # per micro-batch 4 + 6 images, per rank 2 + 3 of them
    d = _inputs("ssl_cr_mse", nx, nu, 8100)

    def run(eng, r, w):
        ms, cs = _nets("ssl_cr_mse")
        mt, ct = _nets("ssl_cr_mse")
        side = _Side(eng, "ssl_cr_mse", ms, cs, mt, ct)
        opt = torch.optim.SGD(list(ms.parameters()) + list(cs.parameters()), lr=1e-2, momentum=0.9, weight_decay=1e-4, nesterov=True)
        losses = []
        for j in range(k):
            (a, b), (c, e) = ((j * nx // k, (j + 1) * nx // k), (j * nu // k, (j + 1) * nu // k))        # micro-batch j of the global batch
            xa, xb = a + r * (b - a) // w, a + (r + 1) * (b - a) // w                                    # this rank's rows of it
            ua, ub = c + r * (e - c) // w, c + (r + 1) * (e - c) // w
            res = eng.step_ssl_cr(side.te, side.st, "mse", d["x"][xa:xb], d["y"][xa:xb], d["u_w"][ua:ub], d["u_s"][ua:ub], 0.7,
                                  nx_global=nx, nu_global=nu, accumulate=j > 0)
            losses.append(res["losses"])
        grads = [g.double() for g in side.grads()]
        side.st.optimizer_step(opt, max_grad_norm=1.0)
        torch.cuda.current_stream().synchronize()
        return dict(grads=grads, params=[p.detach().cpu() for p in side.st.params], losses=torch.stack(losses).sum(0).cpu().double())

    single = run(E.Engine(DEV, "fp32"), 0, 1)
    vc = E.VirtualComm(world)
    engines = [E.Engine(DEV, "fp32") for _ in range(world)]
    for r, e in enumerate(engines):
        e.init_comm_virtual(vc, r, world)
    ranks = _run_ranks(world, lambda r: run(engines[r], r, world))
    for i, (p, q) in enumerate(zip(ranks[0]["params"], ranks[1]["params"])):
        assert _same_bits(p, q), i
    for i, (p, q) in enumerate(zip(ranks[0]["grads"], ranks[1]["grads"])):
        assert torch.equal(p, q), i
    worst = 0.0
    for o in ranks:
        for i, (g, w) in enumerate(zip(o["grads"], single["grads"])):
            e = _l2(g, w)
            worst = max(worst, e)
            assert e <= 2e-5, (i, e)
    total = ranks[0]["losses"] + ranks[1]["losses"]
    assert torch.allclose(total[:3], single["losses"][:3], rtol=1e-5, atol=1e-7), (total, single["losses"])
    print(f"[fp32] world 2, k = 2: worst per-parameter gradient deviation from the single-device accumulated step {worst:.2e}")
