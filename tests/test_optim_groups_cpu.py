"""CPU side of the grouped optimizer step (param groups, AdamW, global-norm clipping).

1. The float64 references the GPU tests apply (tests/_f64_optim.py, _f64.optimizer_ref) equal torch.optim.Adam / AdamW /
   SGD(nesterov=True) and torch.nn.utils.clip_grad_norm_ on float64 CPU tensors over three steps, to 1e-12 relative.  The
   references take every scalar as the fp32 the kernel receives, so the hyperparameters here are exact in fp32 (powers of two;
   betas 0.5 / 0.75, whose bias corrections 1 - beta^t are exact for t <= 3).
2. Self-test of the bounds, as test_bounds_cpu.py does for the existing kernels: a float32 NumPy restatement of the kernel's
   arithmetic holds them, a deliberately wrong variant does not.
3. engine.plan_optimizer, the pure torch-optimizer -> (group rows, group_of_param) mapping."""
import math

import numpy as np
import pytest
import torch

import _f64 as B
import _f64_optim as BO

HP = dict(lr=2.0 ** -7, beta1=0.5, beta2=0.75, eps=2.0 ** -20, wd=2.0 ** -4, momentum=0.5)
SHAPES = [(7, 5, 3, 3), (33,), (4, 9)]


def _t(seed, shape, scale=1.0):
    return torch.from_numpy(np.random.RandomState(seed).standard_normal(shape) * scale)            # float64


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


# ---------------------------------------------------------------- 1. the references are torch
@pytest.mark.parametrize("scale", [1.0, 0.5])
@pytest.mark.parametrize("kind", [0, 1, 2])
def test_references_equal_torch_over_three_steps(kind, scale):
    """scale: the gradient is multiplied by it before the step (what a clipping coefficient does); the reference takes it as
    grad_scale, torch sees pre-scaled gradients -- this pins WHERE the coefficient enters (in front of the L2 decay term)."""
    ps = [torch.nn.Parameter(_t(100 + i, s)) for i, s in enumerate(SHAPES)]
    if kind == 0:
        opt = torch.optim.Adam(ps, lr=HP["lr"], betas=(HP["beta1"], HP["beta2"]), eps=HP["eps"], weight_decay=HP["wd"])
    elif kind == 2:
        opt = torch.optim.AdamW(ps, lr=HP["lr"], betas=(HP["beta1"], HP["beta2"]), eps=HP["eps"], weight_decay=HP["wd"])
    else:
        opt = torch.optim.SGD(ps, lr=HP["lr"], momentum=HP["momentum"], weight_decay=HP["wd"], nesterov=True)
    mine = [p.detach().clone() for p in ps]
    s1 = [torch.zeros_like(p) for p in mine]
    s2 = [torch.zeros_like(p) for p in mine]
    for t in (1, 2, 3):
        grads = [_t(200 + 10 * t + i, s) for i, s in enumerate(SHAPES)]
        for p, g in zip(ps, grads):
            p.grad = g * scale
        opt.step()
        hp = dict(HP, bc1=1 - HP["beta1"] ** t, bc2=1 - HP["beta2"] ** t, first_step=int(t == 1), grad_scale=scale)
        for i, g in enumerate(grads):
            r = BO.optimizer_ref(kind, mine[i], g, s1[i], s2[i], **hp)
            mine[i], s1[i] = r["p"][0], r["s1"][0]
            if kind != 1:
                s2[i] = r["s2"][0]
            assert _rel(mine[i], ps[i].detach()) <= 1e-12, (kind, t, i)
            st = opt.state[ps[i]]
            assert _rel(s1[i], st["momentum_buffer"] if kind == 1 else st["exp_avg"]) <= 1e-12, (kind, t, i)
            if kind != 1:
                assert _rel(s2[i], st["exp_avg_sq"]) <= 1e-12, (kind, t, i)


def test_norm_reference_equals_clip_grad_norm():
    for t in (1, 2, 3):
        grads = [_t(300 + 10 * t + i, s) for i, s in enumerate(SHAPES)]
        ps = [torch.nn.Parameter(torch.zeros(s, dtype=torch.float64)) for s in SHAPES]
        for max_norm in (0.5, 3.0, 1e3, math.inf):
            for p, g in zip(ps, grads):
                p.grad = g.clone()
            total = float(torch.nn.utils.clip_grad_norm_(ps, max_norm))
            r = BO.grad_norm_ref(torch.cat([g.flatten() for g in grads]), max_norm, 1024)
            assert abs(r["norm"][0] - total) <= 1e-12 * total
            want = torch.cat([g.flatten() for g in grads]) * r["coef"][0]
            assert _rel(torch.cat([p.grad.flatten() for p in ps]), want) <= 1e-12, (t, max_norm)
            assert r["exact_one"] == (max_norm >= 1e3)


# ---------------------------------------------------------------- 2. the bounds hold the kernel's arithmetic and nothing else
def _fma32(a, b, c):
    return (np.float64(a) * np.float64(b) + np.float64(c)).astype(np.float32)


def _kernel32(kind, p, graw, m, v, hp, coef=None, fault=None):
    """optim.hip: opt_row + opt_update_g in float32 NumPy (fault: 'coupled' = AdamW's decay put into the gradient instead,
    'no_coef' = the clipping coefficient left out)"""
    f = {k: np.float32(x) for k, x in hp.items()}
    one = np.float32(1)
    gs = one if coef is None or fault == "no_coef" else one * np.float32(coef)
    p, graw, m, v = (t.numpy().astype(np.float32) for t in (p, graw, m, v))
    if kind == 2 and fault != "coupled":
        p = p * (one - f["lr"] * f["wd"])
        g = graw * gs
    else:
        g = _fma32(f["wd"], p, graw * gs)
    if kind != 1:
        m1 = _fma32(f["beta1"], m, (one - f["beta1"]) * g)
        v1 = _fma32(f["beta2"], v, (one - f["beta2"]) * g * g)
        den = np.sqrt(v1) / np.sqrt(f["bc2"]) + f["eps"]
        return dict(p=p - (f["lr"] / f["bc1"]) * (m1 / den), s1=m1, s2=v1)
    buf = _fma32(f["momentum"], m, g)
    return dict(p=p - f["lr"] * _fma32(f["momentum"], buf, g), s1=buf)


def _fails(fn):
    with pytest.raises(AssertionError):
        fn()


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_optimizer_bounds_hold_the_kernel_arithmetic(kind):
    n = 20000
    rs = np.random.RandomState(840 + kind)
    p, g, m = (torch.from_numpy(rs.standard_normal(n).astype(np.float32) * s) for s in (0.1, 1.0, 0.3))
    v = torch.from_numpy((np.abs(rs.standard_normal(n)) * 0.5 + 0.01).astype(np.float32))
    hp = dict(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, wd=1e-2, momentum=0.9, bc1=1 - 0.9 ** 4, bc2=1 - 0.999 ** 4, first_step=0)
    coef = float(np.float32(0.37))
    for c in (None, coef):
        ref = BO.optimizer_ref(kind, p, g, m, v, grad_scale=1.0 if c is None else c, **hp)
        for k, t in _kernel32(kind, p, g, m, v, hp, c).items():
            B.check(torch.from_numpy(t), *ref[k], f"emulated optimizer kind {kind} {k}", dims="i")
    # the clipping coefficient left out
    ref = BO.optimizer_ref(kind, p, g, m, v, grad_scale=coef, **hp)
    bad = _kernel32(kind, p, g, m, v, hp, coef, fault="no_coef")
    _fails(lambda: B.check(torch.from_numpy(bad["p"]), *ref["p"], "coef left out", dims="i"))
    if kind == 2:                       # AdamW run as Adam: coupled (L2) decay in place of the decoupled one
        bad = _kernel32(kind, p, g, m, v, hp, coef, fault="coupled")
        _fails(lambda: B.check(torch.from_numpy(bad["p"]), *ref["p"], "coupled decay", dims="i"))
        _fails(lambda: B.check(torch.from_numpy(bad["s1"]), *ref["s1"], "coupled decay (exp_avg)", dims="i"))


def _norm32(g, max_norm, blocks=1024, fault=None):
    """grad_sumsq_kernel + grad_norm_finalize_kernel: slices summed in double, partials folded in double, fp32 tail
    (fault 'fp32_sum': a running fp32 sum instead)"""
    g = g.numpy().astype(np.float32)
    if fault == "fp32_sum":
        s = np.float64(np.cumsum(g * g, dtype=np.float32)[-1]) if g.size else np.float64(0)
    else:
        per = -(-g.size // blocks) if g.size else 1
        s = np.float64(0)
        for b in range(0, g.size, per):
            s += np.sum(g[b:b + per].astype(np.float64) ** 2)
    norm = np.float32(np.sqrt(s))
    with np.errstate(divide="ignore"):
        coef = np.minimum(np.float32(1), np.float32(max_norm) / (norm + np.float32(1e-6)))
    return float(norm), float(coef)


@pytest.mark.parametrize("n", [1, 257, 1000003])
def test_norm_bounds_hold_the_kernel_arithmetic(n):
    g = torch.from_numpy(np.random.RandomState(850).standard_normal(n).astype(np.float32))
    g[:: max(1, n // 5)] = 1e4
    norm64 = math.sqrt(float((g.double() ** 2).sum()))
    for max_norm in (0.5 * norm64, 2.0 * norm64, math.inf):
        r = BO.grad_norm_ref(g, max_norm, 1024)
        norm, coef = _norm32(g, max_norm)
        assert abs(norm - r["norm"][0]) <= r["norm"][1]
        assert abs(coef - r["coef"][0]) <= r["coef"][1]
        if r["exact_one"]:
            assert coef == 1.0
    assert BO.grad_norm_ref(torch.zeros(5), 1.0, 1024)["exact_one"] and _norm32(torch.zeros(5), 1.0) == (0.0, 1.0)
    if n > 1000:
        r = BO.grad_norm_ref(g[1:] * 1e-4, 1.0, 1024)            # (without the outliers a running fp32 sum drifts visibly)
        norm, _ = _norm32(g[1:] * 1e-4, 1.0, fault="fp32_sum")
        assert abs(norm - r["norm"][0]) > r["norm"][1]


# ---------------------------------------------------------------- 3. plan_optimizer
@pytest.fixture(scope="module")
def modules():
    from ssl_cr_histo_amd import net
    m, c = net.TripletNet_Finetune("resnet18"), net.FinetuneResNet(2)
    names = ["model." + k for k, _ in m.named_parameters()] + ["classifier." + k for k, _ in c.named_parameters()]
    return m, c, names


def _three_groups(params, names):
    convs = [p for p in params if p.dim() == 4]
    vecs = [p for p in params if p.dim() == 1]
    heads = [p for p in params if p.dim() == 2]
    assert len(convs) == 20 and len(heads) == 3 and len(convs) + len(vecs) + len(heads) == len(params) == 66
    return convs, vecs, heads


def test_plan_three_groups(modules):
    from ssl_cr_histo_amd import engine as E
    m, c, names = modules
    params = [p for _, p in m.named_parameters()] + [p for _, p in c.named_parameters()]
    convs, vecs, heads = _three_groups(params, names)
    opt = torch.optim.AdamW([dict(params=convs, lr=1e-3, weight_decay=1e-2), dict(params=vecs, weight_decay=0.0),
                             dict(params=heads, lr=1e-2, betas=(0.8, 0.9))], lr=3e-4, betas=(0.9, 0.999), eps=1e-7, weight_decay=5e-2)
    rows, gmap = E.plan_optimizer(opt, params, names)
    assert [r["kind"] for r in rows] == [2, 2, 2]
    assert [(r["lr"], r["wd"], r["beta1"], r["beta2"], r["eps"]) for r in rows] == [
        (1e-3, 1e-2, 0.9, 0.999, 1e-7), (3e-4, 0.0, 0.9, 0.999, 1e-7), (1e-2, 5e-2, 0.8, 0.9, 1e-7)]
    assert [(r["bc1"], r["bc2"]) for r in rows] == [(1 - 0.9, 1 - 0.999), (1 - 0.9, 1 - 0.999), (1 - 0.8, 1 - 0.9)]      # step 1
    assert gmap == [0 if p.dim() == 4 else 1 if p.dim() == 1 else 2 for p in params]
    assert gmap[0] == 0 and gmap[1] == 1 and gmap[60] == 2 and gmap[61] == 1          # conv1, bn1.weight, fc.0.weight, fc.0.bias
    # a recorded step count: the bias corrections are those of the step about to be taken, per group's betas
    for p in params:
        opt.state[p] = dict(step=torch.tensor(4.0), exp_avg=torch.zeros_like(p), exp_avg_sq=torch.zeros_like(p))
    rows, _ = E.plan_optimizer(opt, params, names)
    assert rows[0]["bc1"] == 1 - 0.9 ** 5 and rows[2]["bc2"] == 1 - 0.9 ** 5 and rows[2]["bc1"] == 1 - 0.8 ** 5
    # Adam and SGD kinds; first_step per group
    rows, _ = E.plan_optimizer(torch.optim.Adam(params, lr=1e-4, weight_decay=1e-4), params)
    assert len(rows) == 1 and rows[0]["kind"] == 0 and rows[0]["wd"] == 1e-4
    sgd = torch.optim.SGD([dict(params=convs + vecs), dict(params=heads, momentum=0.5)], lr=0.1, momentum=0.9, nesterov=True)
    for p in heads:
        sgd.state[p]["momentum_buffer"] = torch.zeros_like(p)
    rows, gmap = E.plan_optimizer(sgd, params)
    assert [(r["kind"], r["momentum"], r["first_step"]) for r in rows] == [(1, 0.9, 1), (1, 0.5, 0)]
    # frozen parameters are outside every group: -1
    for p in params[:60]:
        p.requires_grad = False
    try:
        rows, gmap = E.plan_optimizer(torch.optim.AdamW(params[60:]), params, names)
        assert gmap == [-1] * 60 + [0] * 6
    finally:
        for p in params:
            p.requires_grad = True


def test_plan_refuses_what_it_cannot_express(modules):
    from ssl_cr_histo_amd import _lib as L
    from ssl_cr_histo_amd import engine as E
    m, c, names = modules
    params = [p for _, p in m.named_parameters()] + [p for _, p in c.named_parameters()]
    convs, vecs, heads = _three_groups(params, names)

    def groups(*gs):
        opt = torch.optim.AdamW([dict(params=[torch.nn.Parameter(torch.zeros(1))])], lr=1e-3)
        opt.param_groups = [dict(opt.param_groups[0], params=list(g)) for g in gs]        # (torch itself refuses overlapping groups)
        return opt
    with pytest.raises(L.SslcrError, match=r"model\.model\.conv1\.weight.*groups 0 and 1|model\.conv1\.weight.*groups 0 and 1"):
        E.plan_optimizer(groups(convs + vecs, heads + [params[0]]), params, names)
    with pytest.raises(L.SslcrError, match=r"classifier\.classifier\.0\.bias.*in no param group"):
        E.plan_optimizer(groups(convs, vecs[:-1], heads), params, names)
    params[3].requires_grad = False
    try:
        with pytest.raises(L.SslcrError, match=names[3].replace(".", r"\.") + r" is frozen"):
            E.plan_optimizer(groups(convs, vecs, heads), params, names)
    finally:
        params[3].requires_grad = True
    with pytest.raises(L.SslcrError, match="9 param groups"):
        E.plan_optimizer(groups(*([params[i:i + 8] for i in range(0, 64, 8)] + [params[64:]])), params, names)
    with pytest.raises(L.SslcrError, match="RMSprop"):
        E.plan_optimizer(torch.optim.RMSprop(params), params, names)
    stranger = torch.nn.Parameter(torch.zeros(2, 3))
    with pytest.raises(L.SslcrError, match=r"\(2, 3\).*no parameter"):
        E.plan_optimizer(groups(params, [stranger]), params, names)
    with pytest.raises(NotImplementedError, match="nesterov"):
        E.plan_optimizer(torch.optim.SGD(params, lr=0.1, momentum=0.9), params, names)


def test_lookahead_caches_the_union_of_the_groups(modules):
    from ssl_cr_histo_amd.lookahead import Lookahead
    m, c, names = modules
    params = [p for _, p in m.named_parameters()] + [p for _, p in c.named_parameters()]
    convs, vecs, heads = _three_groups(params, names)
    la = Lookahead(torch.optim.AdamW([dict(params=convs), dict(params=vecs, weight_decay=0.0), dict(params=heads, lr=1e-2)], lr=1e-3))
    assert set(map(id, la.state)) == set(map(id, params)) and len(la.param_groups) == 3


def test_every_train_function_passes_clip_grad_norm_through():
    """steps.*_train hand args.clip_grad_norm (None when the namespace has none) to BoundNet.optimizer_step"""
    import inspect
    from ssl_cr_histo_amd import engine as E
    from ssl_cr_histo_amd import steps
    assert list(inspect.signature(E.BoundNet.optimizer_step).parameters) == ["self", "optimizer", "max_grad_norm"]
    assert inspect.signature(E.BoundNet.optimizer_step).parameters["max_grad_norm"].default is None
    for fn in (steps.bpq_cr_train, steps.cam_cr_train, steps.kather_cr_train, steps._rsp_epoch, steps.cam_sup_train, steps.bpq_sup_train,
               steps.kather_sup_train):
        src = inspect.getsource(fn)
        assert src.count("optimizer_step(") == 1 and 'max_grad_norm=getattr(args, "clip_grad_norm", None)' in src, fn.__name__
