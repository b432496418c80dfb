"""The linear probe on the MI355X (csrc/linprobe.hip, include/sslcr.h) against tests/_linprobe_ref.py.

The value, EVERY gradient element and EVERY logit must lie inside the per-element float64 bounds derived in _linprobe_ref.py from the
operation count, under every plan; two calls must give equal bits and ``linprobe_logits`` the bits of ``linprobe_eval``'s logits.  End
to end, the device fit of ``inference.LinearProbe`` must end "converged" with the FLOAT64 gradient of the restatement at the returned
point below tol + the kernel's gradient bound: first-order optimality of sklearn's own objective, with no fitted number.  Neither the
reference nor sklearn is read here.

Measured on the MI355X (profiles/linprobe_ratios.txt): worst observed / bound 0.13 (logits), 0.025 (gradient), 0.012 (value) -- the
bounds carry _f64's probabilistic constant LAM = 8 and twice the measured expf / logf error."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _f64 as f  # noqa: E402
import _linprobe_ref as R  # noqa: E402

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
record = R.record


# every n, D and C of the issue's lists at least once; (300, 1100) adds the streamed form with a ragged last chunk and two column slices
CASES = [(1, 4, 2, "softmax"), (63, 68, 9, "softmax"), (64, 768, 1, "squared"), (65, 2048, 16, "softmax"), (257, 4, 17, "softmax"),
         (4097, 68, 64, "softmax"), (257, 2048, 64, "squared"), (4097, 768, 9, "softmax"), (63, 768, 17, "squared"), (300, 1100, 17, "softmax")]
_CACHE = {}
_WORST = {"value": 0.0, "grad": 0.0, "logits": 0.0}


def case_inputs(case, weighted=True):
    key = (case, weighted)
    if key not in _CACHE:
        n, D, Cn, loss = case
        host = R.kernel_inputs(n, D, Cn, loss, seed=100 + n + D + Cn, weighted=weighted)
        _CACHE[key] = (host, tuple(None if t is None else t.to(DEV) for t in host))
    return _CACHE[key]


def run(case, groups, weighted=True, want_logits=True):
    """one evaluation into NaN-filled outputs -> (value, grad, logits) on the device, the plan"""
    from ssl_cr_histo_amd import kernels as K
    n, D, Cn, loss = case
    _, (x, y, w, b, s) = case_inputs(case, weighted)
    out = torch.full((1 + Cn * (D + 1),), float("nan"), dtype=torch.float64, device=DEV)
    lg = torch.full((n, Cn), float("nan"), dtype=torch.float32, device=DEV) if want_logits else None
    r = K.linprobe_eval(x, y, w, b, loss, s, groups, want_logits, out=out, logits_out=lg)
    assert r[0].dtype == torch.float64 and r[1].shape == (Cn, D + 1) and r[1].data_ptr() == out.data_ptr() + 8
    assert not want_logits or r[2] is lg
    return r, K.linprobe_plan(n, D, Cn, loss, groups)


@pytest.mark.parametrize("groups", [1, 2, 7, None])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
def test_value_gradient_and_logits_within_their_float64_bounds(case, groups):
    n, D, Cn, loss = case
    (v, g, lg), p = run(case, groups)
    (x, y, w, b, s), _ = case_inputs(case)
    ref = R.device_bounds(x, y, w, b, loss, s, p["tiles_per_group"] * p["tile_rows"])
    what = f"linprobe {case} groups={groups} {p['form']} G={p['groups']} S={p['col_slices']}"
    rl = f.check(lg, ref["logits"], ref["e_logits"], what + " logits", "linprobe_kernel", "nc")
    rg = f.check(g, ref["grad"], ref["e_grad"], what + " grad", "linprobe_kernel", "cd")
    rv = abs(float(v) - ref["value"]) / ref["e_value"]
    print(f"[f64] {what} value | err/bound {rv:.4f}")
    assert np.isfinite(float(v)) and rv <= 1.0, (float(v), ref["value"], ref["e_value"])
    for k, r in (("value", rv), ("grad", rg), ("logits", rl)):
        if r > _WORST[k]:
            _WORST[k] = r
            record("worst_" + k, r)


@pytest.mark.parametrize("case", [(65, 2048, 16, "softmax"), (63, 768, 17, "squared")], ids=lambda c: "-".join(map(str, c)))
def test_unweighted_rows_take_weight_one(case):
    n, D, Cn, loss = case
    (v, g), p = run(case, None, weighted=False, want_logits=False)
    (x, y, w, b, s), _ = case_inputs(case, False)
    assert s is None
    ref = R.device_bounds(x, y, w, b, loss, None, p["tiles_per_group"] * p["tile_rows"])
    f.check(g, ref["grad"], ref["e_grad"], f"linprobe {case} unweighted grad", "linprobe_kernel", "cd")
    assert abs(float(v) - ref["value"]) <= ref["e_value"]


def test_left_out_rows_and_zero_weights_contribute_nothing():
    """a row with a label outside [0, C) or with weight 0 changes no bit of the value and gradient when its features change, and an
    out-of-range label is left out of the weight sum: relabelling it in range changes the value"""
    from ssl_cr_histo_amd import kernels as K
    case = (257, 68, 9, "softmax")
    _, (x, y, w, b, s) = case_inputs(case)
    assert int(y[1]) == 9 and int(y[4]) == -1 and float(s[3]) == 0.0
    v0, g0 = K.linprobe_eval(x, y, w, b, "softmax", s)
    x2 = x.clone()
    x2[[1, 3, 4]] = 1000.0
    v1, g1 = K.linprobe_eval(x2, y, w, b, "softmax", s)
    assert torch.equal(v0, v1) and torch.equal(g0, g1)
    y2 = y.clone()
    y2[1] = 0
    v2, _ = K.linprobe_eval(x, y2, w, b, "softmax", s)
    assert not torch.equal(v0, v2)
    # every row left out: 0 / 0
    v3, g3 = K.linprobe_eval(x, torch.full_like(y, -1), w, b, "softmax", s)
    assert torch.isnan(v3) and torch.isnan(g3).all()


@pytest.mark.parametrize("case", [(4097, 768, 9, "softmax"), (257, 2048, 64, "squared"), (300, 1100, 17, "softmax")], ids=lambda c: "-".join(map(str, c)))
def test_equal_bits_from_two_calls_and_from_the_logits_entry(case):
    from ssl_cr_histo_amd import kernels as K
    _, (x, y, w, b, s) = case_inputs(case)
    (v0, g0, l0), _ = run(case, None)
    (v1, g1, l1), _ = run(case, None)
    assert torch.equal(v0, v1) and torch.equal(g0, g1) and torch.equal(l0, l1)
    (_, _, l7), _ = run(case, 7)
    assert torch.equal(l0, l7)                                          # a logit does not depend on the plan
    out = torch.full((case[0], case[2]), float("nan"), device=DEV)
    assert K.linprobe_logits(x, w, b, out=out) is out and torch.equal(out, l0)
    assert torch.equal(K.linprobe_logits(x, w, b, groups=3), l0)


@pytest.mark.parametrize("case", [(257, 68, 9, "softmax"), (63, 768, 17, "squared"), (65, 2048, 16, "softmax")], ids=lambda c: "-".join(map(str, c)))
def test_logits_have_the_bits_of_the_fmaf_chain_in_rising_d(case):
    """the header's definition of a logit, held by bits: an fmaf chain over d in rising order from +0, then one float32 addition of
    b (the restatement rounds twice per step, which differs from fmaf on about 2^-29 of the steps: below 1e-3 expected mismatches
    over these cases' 4e6 steps)"""
    (_, _, lg), _ = run(case, None)
    (x, y, w, b, s), _ = case_inputs(case)
    want = R.fma_chain_logits(x.numpy(), w.numpy(), b.numpy())
    got = lg.cpu().numpy()
    assert np.array_equal(got.view(np.int32), want.view(np.int32)), np.argwhere(got != want)[:5]


# ------------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("n,D,Cn", R.E2E_CASES)
def test_device_fit_is_first_order_optimal_for_the_float64_objective(n, D, Cn):
    from ssl_cr_histo_amd import inference as I
    from ssl_cr_histo_amd import kernels as K
    X, y = R.e2e_inputs(n, D, Cn)
    tol = 1e-4
    probe = I.LinearProbe(C=R.E2E_C_REG, n_classes=Cn, tol=tol).fit(torch.from_numpy(X).to(DEV), torch.from_numpy(y).to(DEV))
    assert probe.status_ == "converged", (probe.status_, probe.n_iter_, probe.n_eval_, probe.grad_max_)
    assert probe.reads == probe.n_eval_ and probe.setup_reads == 0     # one copy per evaluation and no other read
    assert probe.log.shape == (probe.n_iter_, 4) and probe.grad_max_ <= tol
    theta = probe.theta_
    assert np.array_equal(theta[:, :D].astype(np.float32), probe.coef_.cpu().numpy())
    assert np.array_equal(theta[:, D].astype(np.float32), probe.intercept_.cpu().numpy())
    lam = 1.0 / (R.E2E_C_REG * n)
    assert probe.lam_ == lam
    _, g = R.objective(theta.ravel(), X.astype(np.float64), y, Cn, "softmax", lam)
    p = K.linprobe_plan(n, D, Cn)
    ref = R.device_bounds(torch.from_numpy(X), torch.from_numpy(y), probe.coef_.cpu(), probe.intercept_.cpu(), "softmax", None,
                          p["tiles_per_group"] * p["tile_rows"])
    slack = float(ref["e_grad"].max())
    worst = float(np.abs(g).max())
    print(f"[linprobe] fit ({n}, {D}, {Cn}): {probe.n_iter_} iterations, {probe.n_eval_} evaluations, float64 max|g| {worst:.3e} "
          f"(tol {tol:g} + kernel bound {slack:.2e})")
    assert worst <= tol + slack
    record(f"fit_{n}_{D}_{Cn}_grad_over_limit", worst / (tol + slack))
    # the fitted model separates its training clusters at least as well as chance by a wide margin, and the entries agree
    xq = torch.from_numpy(X).to(DEV)
    pred = probe.predict(xq)
    assert torch.equal(pred, probe.decision_function(xq).argmax(1)) and probe.score(xq, torch.from_numpy(y)) > 1.5 / Cn
    pr = probe.predict_proba(xq)
    assert pr.shape == (n, Cn) and torch.allclose(pr.sum(1), torch.ones(n, device=DEV), atol=1e-5)


def _limit(probe, X, y, loss, s=None):
    """tol + the kernel's gradient bound at the returned point (the greatest element of _linprobe_ref.device_bounds' e_grad)"""
    from ssl_cr_histo_amd import kernels as K
    n, D = X.shape
    p = K.linprobe_plan(n, D, probe.n_classes_, loss)
    ref = R.device_bounds(torch.from_numpy(np.asarray(X, np.float32)), torch.from_numpy(y), probe.coef_.cpu(), probe.intercept_.cpu(), loss,
                          None if s is None else torch.from_numpy(np.asarray(s, np.float32)), p["tiles_per_group"] * p["tile_rows"])
    return probe.tol + float(ref["e_grad"].max())


def test_options_squared_loss_balanced_weights_and_the_probe_dict():
    from ssl_cr_histo_amd import inference as I
    X, y = R.e2e_inputs(300, 16, 4)
    xd, yd = torch.from_numpy(X).to(DEV), torch.from_numpy(y).to(DEV)
    # balanced: the float64 gradient with sklearn's weights n / (classes * count), whose sum is n
    probe = I.LinearProbe(C=0.5, n_classes=4, class_weight="balanced").fit(xd, yd)
    s = (300 / (4 * np.bincount(y, minlength=4)))[y]
    _, g = R.objective(probe.theta_.ravel(), X.astype(np.float64), y, 4, "softmax", 1.0 / (0.5 * 300), s)
    assert probe.status_ == "converged" and probe.setup_reads == 0 and np.abs(g).max() <= _limit(probe, X, y, "softmax", s)
    # sample weights: their sum is read once, before the loop
    sw = torch.rand(300, device=DEV) + 0.5
    probe = probe_w = I.LinearProbe(n_classes=4).fit(xd, yd, sample_weight=sw)
    s64 = sw.cpu().double().numpy()
    _, g = R.objective(probe.theta_.ravel(), X.astype(np.float64), y, 4, "softmax", 1.0 / s64.sum(), s64)
    assert probe.status_ == "converged" and probe.setup_reads == 1 and probe.reads == probe.n_eval_ and np.abs(g).max() <= _limit(probe, X, y, "softmax", s64)
    # squared loss = ridge; no intercept; normalised rows
    T = torch.from_numpy(np.random.default_rng(2).standard_normal((300, 3)).astype(np.float32))
    probe = I.LinearProbe(l2=0.03, loss="squared", fit_intercept=False, normalize="l2", tol=1e-5).fit(xd, T.to(DEV))
    Xn = (X.astype(np.float64).T / np.maximum(np.linalg.norm(X.astype(np.float64), axis=1), 1e-12)).T
    _, g = R.objective(probe.theta_.ravel(), Xn, T.numpy(), 3, "squared", 0.03, None, False)
    assert probe.status_ == "converged" and (probe.theta_[:, 16] == 0).all() and np.abs(g).max() <= _limit(probe, Xn, T.numpy(), "squared")
    assert probe.predict(xd).shape == (300, 3) and probe.score(xd, T) <= 1.0
    with pytest.raises(ValueError):
        probe.to_classifier(None)
    # the entry point: knn_probe's dict, on the training rows and on queries
    r = I.linear_probe(xd, yd, n_classes=4)
    assert {"accuracy", "confusion", "pred", "weighted_f1", "probe"} <= set(r) and r["confusion"].sum() == 300
    assert r["accuracy"] == np.trace(r["confusion"]) / 300 and np.array_equal(r["pred"], r["probe"].predict(xd).cpu().numpy())
    r2 = I.linear_probe(xd[:200], yd[:200], queries=xd[200:], query_targets=yd[200:], n_classes=4)
    assert r2["confusion"].sum() == 100 and r2["pred"].shape == (100,)
    rw = I.linear_probe(xd, yd, n_classes=4, sample_weight=sw)                             # the weighted fit through the entry point
    assert rw["probe"].setup_reads == 1 and np.array_equal(rw["probe"].theta_, probe_w.theta_)
    r3 = I.linear_probe(xd, T[:, 0].to(DEV), l2=0.1)
    assert set(r3) == {"pred", "mse", "probe"} and r3["pred"].shape == (300,) and r3["mse"] >= 0
    with pytest.raises(ValueError):
        I.linear_probe(xd, torch.where(yd == 3, 7, yd), n_classes=4)


def test_to_classifier_and_steps_linear_probe_through_a_real_net():
    """48 labelled tiles of 64 x 64 in two classes through a BoundNet in fp32 mode: the fitted head installed in the classifier makes
    the engine's eval forward reproduce ``predict``"""
    from oracle import cases as C
    from ssl_cr_histo_amd import steps
    from test_engine_gpu import _engine, build, ns
    eng = _engine("fp32")
    model, cls = build("finetune", "finetune", 2, True)
    batches = [(C.u8(700 + n, (16, 3, 64, 64)), C.ints(750 + n, (16,), 2)) for n in range(3)]
    r = steps.linear_probe(ns(), model, cls, batches)
    probe = r["probe"]
    assert probe.status_ in ("converged", "precision") and probe.n_classes_ == 2 and probe.reads == probe.n_eval_ and probe.setup_reads == 0
    assert r["confusion"].sum() == 48 and r["pred"].shape == (48,)
    net = eng.bind(model, cls)
    feats = torch.cat([net.forward((x.to(DEV),), train=False)[0].clone() for x, _ in batches])
    assert np.array_equal(probe.predict(feats).cpu().numpy(), r["pred"])
    probe.to_classifier(cls)
    logits = torch.cat([eng.bind(model, cls).forward((x.to(DEV),), train=False)[1].clone() for x, _ in batches])
    z = probe.decision_function(feats)
    assert torch.allclose(logits, z, rtol=1e-4, atol=1e-4 * float(z.abs().max()))
    clear = (z[:, 0] - z[:, 1]).abs() > 1e-3 * z.abs().max()             # rows whose two logits stand clear of the heads' rounding
    assert clear.any() and torch.equal(logits.argmax(1)[clear], probe.predict(feats)[clear])
    r2 = steps.linear_probe(ns(), model, cls, batches[:2], batches[2:], C=0.1)
    assert r2["confusion"].sum() == 16
