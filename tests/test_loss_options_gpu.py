"""Loss options on the MI355X (include/sslcr.h, library version 10): sslcr_loss_ex and sslcr_ce_denominator alone, then the step
entries, accumulation, virtual ranks and the epoch functions with them.  The yardstick everywhere is torch on the CPU in float64 --
F.cross_entropy(weight=, label_smoothing=, ignore_index=), softmax, log_softmax, autograd for dlogits -- with test_linear_and_loss's
tolerances for this kernel family: 1e-5 * max(1, |ref|) on the three losses, close(dlogits, ref, 1e-5), exact counts.  NaN cases
compare as "both NaN".  The network is the fixed ResNet18, so the engine problems are 64x64 inputs with a handful of images."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import cases as C  # noqa: E402

from test_engine_gpu import DEV, _engine, build, freeze, ns  # noqa: E402
from test_engine_gpu2 import _run_ranks  # noqa: E402
from test_grad_accum_gpu import _ordered_sum, _same_or_both_nan  # noqa: E402
from test_optim_groups_gpu import _bits, _same_bits  # noqa: E402

HW = 64
MARGIN = 1e-4           # no teacher max-prob may lie this close to the threshold: a condition of the test, not a tolerance


def _k():
    from ssl_cr_histo_amd import kernels as K
    return K


def _opts(**kw):
    from ssl_cr_histo_amd import LossOptions
    return LossOptions(**kw)


def rnd(seed, shape, scale=1.0):
    return torch.from_numpy(np.random.RandomState(seed).standard_normal(shape).astype(np.float32) * scale)


# ------------------------------------------------------------------------------------------------ the float64 yardstick
def ref_loss(kind, logits, logits_t, y, nx, lam, o, nu_global=None):
    """torch float64 on the CPU of the fp32 inputs: -> dict(losses [loss, loss_x, loss_u], correct, dlogits, stats [#confident, sum
    of max-probs], maxp)"""
    lg = logits.detach().cpu().double().requires_grad_(True)
    y = y.cpu()
    w = None if o.class_weight is None else o.class_weight.double()
    lx = F.cross_entropy(lg[:nx], y, weight=w, ignore_index=o.ignore_index, label_smoothing=o.label_smoothing)
    keep = y != o.ignore_index
    correct = int(((lg[:nx].argmax(1) == y) & keep).sum())
    nu = lg.shape[0] - nx
    lu, conf, maxp = torch.zeros((), dtype=torch.float64), 0, torch.zeros(0, dtype=torch.float64)
    if kind == 1 and nu > 0:
        lt = logits_t.detach().cpu().double()
        maxp, hard = torch.softmax(lt, -1).max(-1)
        mask = maxp >= o.threshold
        if o.temperature == 0.0:
            ce = F.cross_entropy(lg[nx:], hard, reduction="none")
        else:
            ce = -(torch.softmax(lt / o.temperature, -1) * torch.log_softmax(lg[nx:], -1)).sum(-1)
        lu = (ce * mask.double()).sum() / (nu_global or nu)
        conf = int(mask.sum())
    total = lx + lam * lu
    total.backward()
    return dict(losses=[float(total), float(lx), float(lu)], correct=correct, dlogits=lg.grad, stats=[conf, float(maxp.sum())], maxp=maxp)


def check_against_ref(out, dl, stats, ref, what):
    o = out.cpu().double()
    for i, name in enumerate(("loss", "loss_x", "loss_u")):
        r = ref["losses"][i]
        if np.isnan(r):
            assert np.isnan(float(o[i])), (what, name, float(o[i]))
        else:
            assert abs(float(o[i]) - r) <= 1e-5 * max(1.0, abs(r)), (what, name, float(o[i]), r)
    assert int(o[3]) == ref["correct"], (what, "correct", float(o[3]), ref["correct"])
    if dl is not None:
        got, want = dl.cpu().double(), ref["dlogits"]
        assert torch.equal(torch.isnan(got), torch.isnan(want)), (what, "NaN pattern of dlogits")
        ok = ~torch.isnan(want)
        if ok.any():
            err, scale = float((got[ok] - want[ok]).abs().max()), float(want[ok].abs().max()) + 1e-20
            assert err <= 1e-5 * scale, f"{what}: dlogits max err {err:.3e} vs scale {scale:.3e}"
    if stats is not None:
        s = stats.cpu().double()
        assert float(s[0]) == ref["stats"][0], (what, "confident rows", float(s[0]), ref["stats"][0])
        assert abs(float(s[1]) - ref["stats"][1]) <= 1e-5 * max(1.0, abs(ref["stats"][1])), (what, "sum of max-probs")


def margin_ok(maxp, tau):
    return bool(((maxp - tau).abs() > MARGIN).all())


# ------------------------------------------------------------------------------------------------ 1. sslcr_ce_denominator
@pytest.mark.parametrize("n", [0, 1, 255, 257, 2560])
def test_ce_denominator(n):
    """against w[y][keep].sum(): exact with small-integer weights, 1e-6 relative otherwise; the count exactly; twice the same bits"""
    K = _k()
    Cn = 9
    rs = np.random.RandomState(9100 + n)
    y = torch.from_numpy(rs.randint(0, Cn, (n,)).astype(np.int64))
    for ignore in (-100, 4):
        yi = y.clone()
        if ignore == -100 and n:
            yi[::5] = -100
        keep = yi != ignore
        for integer in (True, False):
            w = torch.from_numpy((rs.randint(0, 8, (Cn,)) if integer else rs.uniform(0.1, 3.0, (Cn,))).astype(np.float32))
            want = float(w.double()[yi[keep]].sum())
            got = K.ce_denominator(yi.to(DEV), Cn, w.to(DEV), ignore).cpu()
            again = K.ce_denominator(yi.to(DEV), Cn, w.to(DEV), ignore).cpu()
            assert torch.equal(_bits(got), _bits(again))
            assert float(got[1]) == float(keep.sum()), (n, ignore, got)
            if integer:
                assert float(got[0]) == want, (n, ignore, got, want)
            else:
                assert abs(float(got[0]) - want) <= 1e-6 * abs(want), (n, ignore, got, want)
        got = K.ce_denominator(yi.to(DEV), Cn, None, ignore).cpu()              # no weights: 1 per kept row
        assert float(got[0]) == float(keep.sum()) == float(got[1])


# ------------------------------------------------------------------------------------------------ 2. defaults == sslcr_loss
@pytest.mark.parametrize("kind,Cn", [(0, 1), (1, 2), (1, 9), (2, 6), (3, 1)])
def test_default_options_equal_sslcr_loss_bit_for_bit(kind, Cn):
    """default LossOptions through sslcr_loss_ex against sslcr_loss, all five kinds (test_linear_and_loss's cases); for the
    cross-entropy kinds also with a stats buffer, which takes the NEW kernel: its default arithmetic is sslcr_loss's"""
    K = _k()
    nx, nu = 6, 14 if kind in (0, 1) else 0
    lg, lt = rnd(65 + Cn, (nx + nu, Cn), 2.0).to(DEV), rnd(66 + Cn, (max(nu, 1), Cn), 2.0).to(DEV)
    if kind in (0, 3):
        kw = dict(target_f=rnd(67, (nx,)).abs().to(DEV), logits_t=lt if kind == 0 else None)
    else:
        kw = dict(target_i=torch.from_numpy(np.random.RandomState(68).randint(0, Cn, (nx,)).astype(np.int64)).to(DEV),
                  logits_t=lt if kind == 1 else None)
    out0, dl0 = K.loss(kind, lg, nx=nx, lambda_u=0.7, **kw)
    out1, dl1 = K.loss(kind, lg, nx=nx, lambda_u=0.7, opts=_opts(), **kw)
    assert _same_bits(out0, out1) and _same_bits(dl0, dl1)
    if kind in (1, 2):
        stats = torch.full((2,), -1.0, device=DEV)
        out2, dl2 = K.loss(kind, lg, nx=nx, lambda_u=0.7, opts=_opts(), stats=stats, **kw)
        assert _same_bits(out0, out2) and _same_bits(dl0, dl2)
        assert float(stats[0]) == nu


# ------------------------------------------------------------------------------------------------ 3. the kernel against float64
SHAPES = [(2, 1, 0), (2, 6, 14), (9, 6, 14), (9, 300, 257), (64, 6, 14), (64, 300, 257), (2, 300, 0), (9, 1, 257), (64, 1, 0)]
SUP = ["weights", "ignore-100-some", "ignore-valid-some", "ignore-100-all", "ignore-valid-all", "zero-weight-only", "zero-weight-among",
       "smooth", "smooth+weights+ignore", "smooth+zero-weight-only", "smooth+ignore-100-all"]
CONS = [(0.0, 0.0), (0.6, 0.0), (1.0, 0.0), (0.0, 0.5), (0.6, 1.0), (0.6, 0.5), (0.0, 1.0)]
T_SCALE = {2: 2.0, 9: 2.0, 64: 4.5}     # teacher logits: randn * this, so that 0.6 splits the rows at every class count


def _teacher(Cn, nu, seed):
    return rnd(seed, (max(nu, 1), Cn), T_SCALE[Cn])


def _sup_case(name, Cn, nx, seed):
    """-> (targets [nx] int64, LossOptions keyword arguments)"""
    rs = np.random.RandomState(seed)
    y = torch.from_numpy(rs.randint(0, Cn, (nx,)).astype(np.int64))
    w = torch.from_numpy(rs.uniform(0.25, 3.0, (Cn,)).astype(np.float32))
    kw = {}
    if "smooth" in name:
        kw["label_smoothing"] = 0.1
    if name == "weights":
        kw["class_weight"] = w
    elif name == "ignore-100-some":
        y[::3] = -100
    elif name == "ignore-valid-some":
        y[::3] = 1
        kw["ignore_index"] = 1
    elif name in ("ignore-100-all", "smooth+ignore-100-all"):
        y[:] = -100
    elif name == "ignore-valid-all":
        y[:] = 1
        kw["ignore_index"] = 1
    elif name in ("zero-weight-only", "smooth+zero-weight-only"):       # only classes of weight zero present: 0 / 0
        w[0] = 0.0
        y[:] = 0
        kw["class_weight"] = w
    elif name == "zero-weight-among":
        w[0] = 0.0
        y[::2] = 0
        kw["class_weight"] = w
    elif name == "smooth+weights+ignore":
        w[Cn - 1] = 0.0
        y[::4] = 1
        kw.update(class_weight=w, ignore_index=1)
    return y, kw


def test_threshold_condition_on_the_cpu():
    """no float64 teacher max-prob of the kernel tests lies within 1e-4 of a threshold, and 0.6 splits the rows wherever there are
    14 or more (checked here so that a changed seed shows up by name)"""
    for Cn, nx, nu in SHAPES:
        if nu == 0:
            continue
        maxp = torch.softmax(_teacher(Cn, nu, 9300 + Cn + nu).double(), -1).max(-1)[0]
        for tau in (0.6, 1.0):
            assert margin_ok(maxp, tau), (Cn, nu, tau)
        assert 0 < int((maxp >= 0.6).sum()) < nu, (Cn, nu)
        assert int((maxp >= 1.0).sum()) == 0


@pytest.mark.parametrize("sup", SUP)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "C%d-nx%d-nu%d" % s)
def test_loss_ex_against_float64(shape, sup):
    """every supervised case at every shape (nx = 300: the strided row loop past one pass of the workgroup; nu = 257: one row past
    it), each with one of the (threshold, temperature) pairs in turn; kind 2 where there are no unlabeled rows (every other such
    case: kind 1 with nu = 0).  Then the same call with the denominator supplied from sslcr_ce_denominator over the same rows:
    the same bits."""
    K = _k()
    Cn, nx, nu = shape
    i = SUP.index(sup)
    tau, T = CONS[(i + SHAPES.index(shape)) % len(CONS)] if nu else (0.0, 0.0)
    kind = 1 if (nu or i % 2 == 0) else 2
    y, kw = _sup_case(sup, Cn, nx, 9200 + 17 * i + Cn + nx)
    o = _opts(threshold=tau, temperature=T, **kw)
    lg, lt = rnd(9250 + i + Cn + nx, (nx + nu, Cn), 2.0), _teacher(Cn, nu, 9300 + Cn + nu)
    lam = 0.7
    ref = ref_loss(kind, lg, lt, y, nx, lam, o)
    if nu:
        assert margin_ok(ref["maxp"], tau)                                   # before the GPU is touched
    common = dict(logits_t=lt.to(DEV) if kind == 1 and nu else None, target_i=y.to(DEV), nx=nx, lambda_u=lam, opts=o)
    stats = torch.full((2,), -1.0, device=DEV)
    out, dl = K.loss(kind, lg.to(DEV), stats=stats, **common)
    what = f"C={Cn} nx={nx} nu={nu} {sup} tau={tau} T={T} kind={kind}"
    check_against_ref(out, dl, stats, ref, what)
    w = o.weight_on(DEV, Cn)
    den = K.ce_denominator(y.to(DEV), Cn, w, o.ignore_index)
    out2, dl2 = K.loss(kind, lg.to(DEV), denominator=den, **common)
    _same_or_both_nan(out2, out, what + ": losses with the denominator supplied")
    _same_or_both_nan(dl2, dl, what + ": dlogits with the denominator supplied")
    out3, none = K.loss(kind, lg.to(DEV), want_grad=False, **common)        # the validation form: no dlogits
    assert none is None
    _same_or_both_nan(out3, out, what + ": losses without dlogits")


@pytest.mark.parametrize("cons", CONS, ids=lambda c: "tau%g-T%g" % c)
@pytest.mark.parametrize("shape", [s for s in SHAPES if s[2]], ids=lambda s: "C%d-nx%d-nu%d" % s)
def test_consistency_options_against_float64(shape, cons):
    """every (threshold, temperature) pair at every shape with unlabeled rows, supervised term plain: all rows pass (0), some
    (0.6), none (1.0); hard labels (T = 0) and soft targets (0.5 sharpens, 1 is the teacher's own softmax)"""
    K = _k()
    Cn, nx, nu = shape
    tau, T = cons
    o = _opts(threshold=tau, temperature=T)
    y = torch.from_numpy(np.random.RandomState(9400 + Cn).randint(0, Cn, (nx,)).astype(np.int64))
    lg, lt = rnd(9450 + Cn + nu, (nx + nu, Cn), 2.0), _teacher(Cn, nu, 9300 + Cn + nu)
    ref = ref_loss(1, lg, lt, y, nx, 0.7, o, nu_global=2 * nu)
    assert margin_ok(ref["maxp"], tau)
    stats = torch.full((2,), -1.0, device=DEV)
    out, dl = K.loss(1, lg.to(DEV), logits_t=lt.to(DEV), target_i=y.to(DEV), nx=nx, lambda_u=0.7, nu_global=2 * nu, opts=o, stats=stats)
    check_against_ref(out, dl, stats, ref, f"C={Cn} nx={nx} nu={nu} tau={tau} T={T}")
    if tau == 0.0:
        assert float(stats[0]) == nu
    if tau == 1.0:
        assert float(stats[0]) == 0 and float(out[2]) == 0.0 and float(dl[nx:].abs().max()) == 0.0


def test_loss_ex_errors_on_the_device_path():
    """what the library refuses stays refused with real tensors: an MSE kind with an option, and an option out of range"""
    from ssl_cr_histo_amd import _lib as L
    K = _k()
    lg = rnd(1, (4, 1)).to(DEV)
    with pytest.raises(L.SslcrError):
        K.loss(3, lg, target_f=rnd(2, (4,)).to(DEV), nx=4, opts=_opts(label_smoothing=0.1))
    with pytest.raises(L.SslcrError):
        K.loss(2, rnd(1, (4, 3)).to(DEV), target_i=torch.zeros(4, dtype=torch.int64, device=DEV), nx=4, opts=_opts(threshold=0.5))


def test_a_target_that_is_no_class_id_gives_nan_not_a_stray_read():
    """torch raises for a target outside [0, C) that is not ignore_index; without a sync the signal is a NaN divisor: NaN losses,
    zero dlogits on that row, and sslcr_ce_denominator's sum NaN with the count of the valid rows"""
    K = _k()
    lg = rnd(9470, (6, 3), 2.0).to(DEV)
    for bad in (3, -1, 1 << 40):
        y = torch.tensor([0, 1, bad, 2, -100, 1], dtype=torch.int64).to(DEV)
        out, dl = K.loss(2, lg, target_i=y, nx=6, opts=_opts(label_smoothing=0.1))
        assert bool(torch.isnan(out[:2]).all()) and float(dl[2].abs().max()) == 0.0 and float(dl[4].abs().max()) == 0.0
        den = K.ce_denominator(y, 3, None, -100).cpu()
        assert bool(torch.isnan(den[0])) and float(den[1]) == 4


def test_threshold_zero_makes_no_test_of_the_teacher():
    """a teacher row with a NaN logit propagates at threshold 0 exactly as in sslcr_loss (no mask test at all): the same bits"""
    K = _k()
    nx, nu, Cn = 4, 5, 3
    lg, lt = rnd(9480, (nx + nu, Cn), 2.0).to(DEV), rnd(9481, (nu, Cn), 2.0)
    lt[1, 2] = float("nan")
    y = torch.tensor([0, 1, 2, 1], dtype=torch.int64).to(DEV)
    out0, dl0 = K.loss(1, lg, logits_t=lt.to(DEV), target_i=y, nx=nx, lambda_u=0.7)
    out1, dl1 = K.loss(1, lg, logits_t=lt.to(DEV), target_i=y, nx=nx, lambda_u=0.7, opts=_opts())
    _same_or_both_nan(out1, out0, "losses")
    _same_or_both_nan(dl1, dl0, "dlogits")


# ------------------------------------------------------------------------------------------------ engine helpers
LAM = 0.7


class _Nets:
    """a student (and, for the consistency workloads, a frozen eval-mode teacher) bound to one engine"""

    def __init__(self, eng, workload, classes, nets=None):
        self.eng, self.workload, self.classes = eng, workload, classes
        mk = (lambda: build("triplet", "mlp", classes, False)) if workload == "rsp" else (lambda: build("finetune", "finetune", classes, True))
        self.ms, self.cs, self.mt, self.ct = nets if nets is not None else (mk() + (mk() if workload != "rsp" else (None, None)))
        self.ms.train(); self.cs.train()
        self.st = eng.bind(self.ms, self.cs)
        self.te = None
        if self.mt is not None:
            freeze(self.mt, 64)
            self.mt.eval(); self.ct.eval()
            self.te = eng.bind(self.mt, self.ct)

    def clone(self):
        return _Nets(self.eng, self.workload, self.classes, tuple(copy.deepcopy(m) for m in (self.ms, self.cs, self.mt, self.ct)))

    def step(self, d, rows=None, urows=None, **kw):
        a, b = rows if rows is not None else (0, d["y"].shape[0])
        if self.workload == "rsp":
            return self.eng.step_supervised(self.st, "ce", [x[a:b] for x in d["xs"]], d["y"][a:b], train=True, **kw)
        c, e = urows if urows is not None else (0, d["u_w"].shape[0])
        return self.eng.step_ssl_cr(self.te, self.st, "ce", d["x"][a:b], d["y"][a:b], d["u_w"][c:e], d["u_s"][c:e], LAM, **kw)

    def grads(self):
        return [self.st.grad(i).cpu() for i in range(len(self.st.params))]


def _data(workload, nx, nu, classes, seed, y=None):
    y = torch.as_tensor(y, dtype=torch.int64) if y is not None else C.ints(seed + 3, (nx,), classes)
    if workload == "rsp":
        return dict(xs=[C.u8(seed + j, (nx, 3, HW, HW)) for j in range(3)], y=y)
    return dict(x=C.u8(seed, (nx, 3, HW, HW)), u_w=C.u8(seed + 1, (nu, 3, HW, HW)), u_s=C.u8(seed + 2, (nu, 3, HW, HW)), y=y)


def _tau_between(maxp):
    """a threshold in the widest gap of the sorted max-probs: some rows pass, some do not, none within MARGIN (asserted)"""
    s = torch.sort(maxp.double().cpu())[0]
    gaps = s[1:] - s[:-1]
    j = int(gaps.argmax())
    assert float(gaps[j]) > 4 * MARGIN, "the teacher's max-probs leave no gap for a threshold"
    return float((s[j] + s[j + 1]) / 2)


def _teacher_maxp(nets, u_w):
    _, lt = nets.te.forward((u_w,), train=False)
    return torch.softmax(lt.double().cpu(), -1).max(-1)[0], lt


def _losses_close(got, want, what):
    got, want = got.cpu().double(), torch.as_tensor(want, dtype=torch.float64)
    for i in range(len(want)):
        assert abs(float(got[i]) - float(want[i])) <= 1e-5 * max(1.0, abs(float(want[i]))), (what, i, got.tolist(), want.tolist())


# ------------------------------------------------------------------------------------------------ 4. composition
def test_step_with_options_is_forward_loss_backward():
    """sslcr_step_ssl_cr with every option set against its building blocks on a deep copy -- BoundNet.forward(train) ->
    kernels.loss(opts) -> BoundNet.backward(dlogits): the same gradient bits; the step's losses and stats against torch float64
    on the logits the step returned.  Then sslcr_step_supervised the same way (train, and train=False: the validation loss)."""
    from ssl_cr_histo_amd import _lib as L
    K = _k()
    eng = _engine("fp32")
    a = _Nets(eng, "ssl_cr_ce", 3)
    b = a.clone()
    d = _data("ssl_cr_ce", 5, 6, 3, 9500, y=[0, 2, 1, 1, 0])
    maxp, lt0 = _teacher_maxp(a, d["u_w"])
    o = _opts(class_weight=[0.5, 2.0, 3.0], label_smoothing=0.1, ignore_index=1, threshold=_tau_between(maxp), temperature=0.5)
    r = a.step(d, loss_options=o)
    assert _same_bits(r["logits_t"], lt0)
    ref = ref_loss(1, r["logits"], r["logits_t"], d["y"], 5, LAM, o)
    assert margin_ok(ref["maxp"], o.threshold) and 0 < ref["stats"][0] < 6
    check_against_ref(r["losses"], None, r["stats"], ref, "step_ssl_cr with options")
    _, logits = b.st.forward((torch.cat((d["x"], d["u_s"])),), train=True)
    assert _same_bits(logits, r["logits"])
    out, dl = K.loss(1, logits, logits_t=lt0, target_i=d["y"].to(DEV), nx=5, lambda_u=LAM, opts=o)
    assert _same_bits(out, r["losses"])
    b.st.backward(dl)
    for i, (g, w) in enumerate(zip(a.grads(), b.grads())):
        assert _same_bits(g, w), a.st.param_names[i]
    assert float(a.st.grad(len(a.st.params) - 1).abs().max()) > 0
    # student-only step, kind 2
    o2 = _opts(class_weight=[0.5, 2.0, 3.0], ignore_index=1)
    r2 = a.eng.step_supervised(a.st, "ce", [d["x"]], d["y"], train=True, loss_options=o2)
    check_against_ref(r2["losses"], None, None, ref_loss(2, r2["logits"], None, d["y"], 5, 0.0, o2), "step_supervised with options")
    _, lg2 = b.st.forward((d["x"],), train=True)
    assert _same_bits(lg2, r2["logits"])
    out2, dl2 = K.loss(2, lg2, target_i=d["y"].to(DEV), nx=5, opts=o2)
    b.st.backward(dl2)
    for i, (g, w) in enumerate(zip(a.grads(), b.grads())):
        assert _same_bits(g, w), a.st.param_names[i]
    rv = a.eng.step_supervised(a.st, "ce", [d["x"]], d["y"], train=False, loss_options=o2)
    check_against_ref(rv["losses"], None, None, ref_loss(2, rv["logits"], None, d["y"], 5, 0.0, o2), "validation step with options")
    with pytest.raises(ValueError):
        a.eng.step_supervised(a.st, "mse", [d["x"]], d["y"].float(), train=False, loss_options=o2)
    with pytest.raises(L.SslcrError):
        a.eng.step_supervised(a.st, "ce", [d["x"]], d["y"], train=False, loss_options=_opts(threshold=0.5))     # no consistency term


# ------------------------------------------------------------------------------------------------ 5. accumulation
@pytest.mark.parametrize("case", ["weights+ignore", "smoothing-only+rows-100"])
@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("workload", ["ssl_cr_ce", "rsp"])
def test_accumulation_with_the_batch_denominator(workload, k, case):
    """weighted + ignore-index CE -- and smoothing-only options on a batch with rows labelled -100, whose first micro-batch (k = 2)
    is ignored entirely: its own divisor would be 0 / 0 -- as k micro-steps through steps._ssl_cr_step / _sup_step (one denominator launch per batch, handed
    to every micro-step).  The micro-batches have different class mixes -- the first holds only the lightest class, the last the
    heaviest and the ignored rows -- so a divisor taken per micro-batch would be off by a factor.
      * the accumulated gradient is the ordered fp32 sum of the micro-steps' own gradients (a second copy runs the same micro-steps
        without accumulating, with the same batch denominator), bit for bit;
      * the summed losses are the k = 1 losses of the whole batch on the logits the micro-steps returned: torch float64 on the
        concatenated logits, and the engine's own kernel in ONE call over them (train-mode BatchNorm uses each micro-batch's
        statistics, so a k = 1 step of the network itself has other logits: the comparison is of the loss, on the same logits)."""
    from ssl_cr_histo_amd import steps
    K = _k()
    eng = _engine("fp32")
    classes = 6 if workload == "rsp" else 3
    n, nu = 6, 6
    if case == "weights+ignore":
        w, ig = [0.25, 1.0, 4.0, 1.5, 0.5, 2.0][:classes], 1
        y = [0, 0, 0, 1, 2, 2] if k == 2 else [0, 0, 1, 0, 2, 1]            # ignore_index 1; micro-batches (3, 3) / (2, 2, 2)
        o = _opts(class_weight=w, ignore_index=1)
    else:
        w, ig = [1.0] * classes, -100
        y = [-100, -100, -100, 0, 1, 2] if k == 2 else [-100, -100, 0, -100, 2, 1]
        o = _opts(label_smoothing=0.1)
    a = _Nets(eng, workload, classes)
    b = a.clone()
    d = _data(workload, n, nu, classes, 9600 + k, y=y)
    if workload == "rsp":
        r = steps._sup_step(eng, a.st, "ce", d["xs"], d["y"], k, o)
    else:
        r = steps._ssl_cr_step(eng, a.te, a.st, "ce", d["x"], d["y"], d["u_w"], d["u_s"], LAM, k, o)
    den = K.ce_denominator(d["y"].to(DEV), classes, o.weight_on(DEV, classes), ig)
    want_den = float(torch.tensor(w, dtype=torch.float64)[d["y"][d["y"] != ig]].sum())
    assert float(den[0]) == want_den and float(den[1]) == float((d["y"] != ig).sum())
    parts, micro_den = [], []
    for j, ((lo, hi), (ulo, uhi)) in enumerate(zip(steps.micro_ranges(n, k), steps.micro_ranges(nu, k))):
        kw = dict(n_global=n) if workload == "rsp" else dict(nx_global=n, nu_global=nu)
        b.step(d, (lo, hi), (ulo, uhi), loss_options=o, denominator=den, **kw)
        parts.append(b.grads())
        yj = d["y"][lo:hi]
        micro_den.append(float(torch.tensor(w, dtype=torch.float64)[yj[yj != ig]].sum()))
    assert max(micro_den) > 2 * min(micro_den), micro_den                    # the mixes differ: per-micro-batch divisors would show
    for i, (g, want) in enumerate(zip(a.grads(), _ordered_sum(parts))):
        assert _same_bits(g, want), (a.st.param_names[i])
    if workload == "rsp":
        ref = ref_loss(2, r["logits"], None, d["y"], n, 0.0, o)
        out1, _ = K.loss(2, r["logits"].contiguous(), target_i=d["y"].to(DEV), nx=n, opts=o, want_grad=False)
    else:
        ref = ref_loss(1, r["logits"], r["logits_t"], d["y"], n, LAM, o)
        out1, _ = K.loss(1, r["logits"].contiguous(), logits_t=r["logits_t"].contiguous(), target_i=d["y"].to(DEV), nx=n, lambda_u=LAM,
                         opts=o, want_grad=False)
    assert not any(np.isnan(v) for v in ref["losses"])
    _losses_close(r["losses"], ref["losses"], f"{workload} k={k}: summed losses vs float64 on the whole batch")
    _losses_close(r["losses"], out1.cpu()[:3], f"{workload} k={k}: summed losses vs one call on the whole batch")
    assert int(r["losses"][3]) == ref["correct"] == int(out1[3])


# ------------------------------------------------------------------------------------------------ 6. virtual ranks
@pytest.mark.parametrize("case", ["weights+ignore", "smoothing-only+rows-100"])
def test_virtual_ranks_share_the_global_denominator(case):
    """world 2, uneven class mixes per rank (rank 0: the light class and the ignored rows, rank 1: the heavy class; second case:
    smoothing-only options, every row of rank 0 labelled -100), through
    steps._ssl_cr_step: one denominator launch and one 2-float all-reduce per step.  Losses summed over ranks, the all-reduced
    gradient and the post-step parameters against the one-rank step on the concatenated batch, to the fp32 bounds of
    test_virtual_ranks_equal_the_single_device_step (losses rtol 1e-5, gradients 2e-5 and state 1e-5 relative L2)."""
    from ssl_cr_histo_amd import engine as E
    from ssl_cr_histo_amd import steps
    world, nx, nu, classes = 2, 6, 6, 3
    if case == "weights+ignore":
        o = _opts(class_weight=[0.25, 1.0, 4.0], ignore_index=1, label_smoothing=0.1)
        d = _data("ssl_cr_ce", nx, nu, classes, 9700, y=[0, 1, 0, 2, 2, 2])
    else:
        o = _opts(label_smoothing=0.1)
        d = _data("ssl_cr_ce", nx, nu, classes, 9700, y=[-100, -100, -100, 2, 0, 1])

    def run(eng, r, w):
        nets = _Nets(eng, "ssl_cr_ce", classes)
        opt = torch.optim.SGD(list(nets.ms.parameters()) + list(nets.cs.parameters()), lr=1e-2, momentum=0.9, weight_decay=1e-4, nesterov=True)
        (a, b), (c, e) = (r * nx // w, (r + 1) * nx // w), (r * nu // w, (r + 1) * nu // w)
        res = steps._ssl_cr_step(eng, nets.te, nets.st, "ce", d["x"][a:b], d["y"][a:b], d["u_w"][c:e], d["u_s"][c:e], LAM, 1, o)
        grads = [g.double() for g in nets.grads()]
        nets.st.optimizer_step(opt)
        torch.cuda.current_stream().synchronize()
        return dict(losses=res["losses"].cpu().double(), grads=grads, params=[p.detach().cpu().double() for p in nets.st.params],
                    logits=res["logits"].cpu(), logits_t=res["logits_t"].cpu())

    single = run(E.Engine(DEV, "fp32"), 0, 1)
    ref = ref_loss(1, single["logits"], single["logits_t"], d["y"], nx, LAM, o)
    _losses_close(single["losses"], ref["losses"], "one rank vs float64")
    vc = E.VirtualComm(world)
    engines = [E.Engine(DEV, "fp32") for _ in range(world)]
    for r, e in enumerate(engines):
        e.init_comm_virtual(vc, r, world)
    ranks = _run_ranks(world, lambda r: run(engines[r], r, world))
    total = ranks[0]["losses"] + ranks[1]["losses"]
    assert torch.allclose(total[:3], single["losses"][:3], rtol=1e-5, atol=1e-7), (total, single["losses"])
    assert float(total[3]) == float(single["losses"][3])
    for o_ in ranks:
        for i, (g, want) in enumerate(zip(o_["grads"], single["grads"])):
            assert float((g - want).norm() / (want.norm() + 1e-30)) <= 2e-5, i
        for i, (p, want) in enumerate(zip(o_["params"], single["params"])):
            assert float((p - want).norm() / (want.norm() + 1e-30)) <= 1e-5, i
    for i, (p, q) in enumerate(zip(ranks[0]["params"], ranks[1]["params"])):
        assert torch.equal(p, q), i
    vc.close()


# ------------------------------------------------------------------------------------------------ 7. the epoch functions
def _record(eng, name, log):
    orig = getattr(eng, name)

    def wrapped(*a, **kw):
        r = orig(*a, **kw)
        log.append((a, kw, r))
        return r
    setattr(eng, name, wrapped)
    return lambda: delattr(eng, name)


def test_epoch_functions_with_loss_options():
    """kather_cr_train (two loader batches of 4 labeled + 4 unlabeled 256x256 images: the reference hard-codes the side) and
    cam_cr_validate with args.loss_options: the returned averages against torch float64 recomputed from the logits every step
    returned (recorded by a wrapper around the engine's step methods), args.loss_stats against the recorded teacher logits"""
    from ssl_cr_histo_amd import steps
    eng = _engine("fp32")
    classes = 3
    mt, ct = build("finetune", "finetune", classes, True)
    ms, cs = build("finetune", "finetune", classes, True)
    freeze(mt, 64)
    ys = [[0, 1, 2, 2], [1, 1, 0, 2]]
    labeled = [(C.u8(9800 + i, (4, 3, 256, 256)), torch.tensor(ys[i])) for i in range(2)]
    unlabeled = [(C.u8(9810 + i, (4, 3, 256, 256)), C.u8(9820 + i, (4, 3, 256, 256))) for i in range(2)]
    te = eng.bind(mt, ct)
    mt.eval(); ct.eval()
    # raw 0..255 images at 256x256 saturate a random-weight head (every max-prob 1): shrink the teacher's linear head so that its
    # largest logit is 2 and the max-probs spread
    top = max(float(te.forward((u,), train=False)[1].abs().max()) for u, _ in unlabeled)
    with torch.no_grad():
        for p in ct.parameters():
            p.mul_(2.0 / top)
    maxp = torch.cat([torch.softmax(te.forward((u,), train=False)[1].double().cpu(), -1).max(-1)[0] for u, _ in unlabeled])
    o = _opts(class_weight=[0.5, 2.0, 3.0], ignore_index=1, label_smoothing=0.1, threshold=_tau_between(maxp))
    opt = torch.optim.Adam(list(ms.parameters()) + list(cs.parameters()), lr=1e-4)
    log = []
    undo = _record(eng, "step_ssl_cr", log)
    try:
        args = ns(lambda_u=LAM, loss_options=o)
        ret = steps.kather_cr_train(args, mt, ms, ct, cs, labeled, unlabeled, opt, 1)
    finally:
        undo()
    assert len(log) == 2 and all(kw["loss_options"] is o and kw["denominator"] is None for _, kw, _ in log)
    refs = [ref_loss(1, r["logits"], r["logits_t"], torch.tensor(y), 4, LAM, o) for (_, _, r), y in zip(log, ys)]
    assert all(margin_ok(r["maxp"], o.threshold) for r in refs)
    for i in range(3):
        want = float(np.mean([r["losses"][i] for r in refs]))
        assert abs(ret[i] - want) <= 1e-5 * max(1.0, abs(want)), (i, ret, want)
    assert ret[3] == sum(r["correct"] for r in refs) / 8
    conf, tot = sum(r["stats"][0] for r in refs), sum(r["stats"][1] for r in refs)
    assert args.loss_stats["rows"] == 8 and args.loss_stats["confident"] == conf and args.loss_stats["mask_rate"] == conf / 8
    assert abs(args.loss_stats["mean_max_prob"] - tot / 8) <= 1e-5
    assert 0 < conf < 8
    # validation: tumor / normal loaders of 64x64 tiles, two batches, weighted with an ignored class
    ms2, cs2 = build("finetune", "finetune", classes, True)
    ov = _opts(class_weight=[0.5, 2.0, 3.0], ignore_index=2)
    tumor = [(C.u8(9830 + i, (3, 3, HW, HW)), torch.tensor([1, 1, 2])) for i in range(2)]
    normal = [(C.u8(9840 + i, (3, 3, HW, HW)), torch.tensor([0, 2, 0])) for i in range(2)]
    log = []
    undo = _record(eng, "step_supervised", log)
    try:
        loss, acc = steps.cam_cr_validate(ns(loss_options=ov), ms2, cs2, tumor, normal, 1)
    finally:
        undo()
    assert len(log) == 2 and all(kw["train"] is False for _, kw, _ in log)
    refs = [ref_loss(2, r["logits"], None, a[3], 6, 0.0, ov) for a, _, r in log]
    want = float(np.mean([r["losses"][0] for r in refs]))
    assert abs(loss - want) <= 1e-5 * max(1.0, abs(want)), (loss, want)
    assert acc == sum(r["correct"] for r in refs) / 12
    # the MSE loop refuses, on the device as well
    with pytest.raises(ValueError):
        steps.bpq_cr_validate(ns(loss_options=ov), ms2, cs2, [], 1)


# ------------------------------------------------------------------------------------------------ 8. off is off
@pytest.mark.parametrize("off", ["none", "defaults"])
@pytest.mark.parametrize("workload", ["ssl_cr_ce", "rsp"])
def test_off_is_off(workload, off):
    """a step with loss_options=None (or all-default options) after a step that had options: the bits of a fresh net's default
    step -- the library's sticky options are reset per call -- and, under sslcr_profile, as many recorded launches"""
    eng = _engine("fp32")
    classes = 6 if workload == "rsp" else 3
    a = _Nets(eng, workload, classes)
    b = a.clone()
    d1, d2 = _data(workload, 4, 4, classes, 9900), _data(workload, 4, 4, classes, 9920)
    w = [0.25, 1.0, 4.0, 1.5, 0.5, 2.0][:classes]
    ra0 = a.step(d1, loss_options=_opts(class_weight=w, ignore_index=1, label_smoothing=0.1))
    rb0 = b.step(d1)                                                        # the same forward (running statistics), plain loss
    assert _same_bits(ra0["logits"], rb0["logits"]) and not _same_bits(ra0["losses"][:2], rb0["losses"][:2])
    assert "stats" in ra0 and "stats" not in rb0
    kw = {} if off == "none" else dict(loss_options=_opts())

    def profiled(nets, **kw):
        eng.profile(1)
        r = nets.step(d2, **kw)
        torch.cuda.synchronize()
        n = sum(eng.profile_read(which)["launches"] for which in (0, 1))
        eng.profile(0)
        return r, n
    (ra, na), (rb, nb) = profiled(a, **kw), profiled(b)
    assert na == nb and na > 0, (na, nb)
    assert "stats" not in ra
    assert _same_bits(ra["losses"], rb["losses"]) and _same_bits(ra["logits"], rb["logits"])
    for i, (g, want) in enumerate(zip(a.grads(), b.grads())):
        assert _same_bits(g, want), a.st.param_names[i]
