"""CPU-only: the linear probe's plan and argument validation (host side of the C-ABI, no device), the NumPy float64 restatement
(tests/_linprobe_ref.py) against central differences and against sklearn 1.7.2's solutions, and the host L-BFGS."""
import ctypes as C
import os

import numpy as np
import pytest

import _linprobe_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from ssl_cr_histo_amd import _lib
    return _lib.lib()


# ---------------------------------------------------------------------------------------------------------------- plan
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 4097, 100000])
@pytest.mark.parametrize("D", [4, 68, 768, 1024, 1028, 1100, 2048])
@pytest.mark.parametrize("Cn,loss", [(1, "squared"), (2, "softmax"), (9, "softmax"), (16, "softmax"), (17, "softmax"), (33, "squared"), (64, "softmax")])
def test_plan_covers_rows_columns_and_partials(lib, n, D, Cn, loss):
    from ssl_cr_histo_amd import _lib as L
    from ssl_cr_histo_amd import kernels as K
    p = K.linprobe_plan(n, D, Cn, loss)
    tiles, Dp = -(-n // L.LINPROBE_TILE), -(-D // 16) * 16
    G, S, CB = p["groups"], p["col_slices"], p["class_blocks"]
    assert p["tile_rows"] == L.LINPROBE_TILE
    assert CB == (1 if Cn <= 16 else 2 if Cn <= 32 else 4) and 16 * CB >= Cn
    assert 1 <= G <= min(tiles, 512) and G * p["tiles_per_group"] >= tiles
    assert (G - 1) * p["tiles_per_group"] < tiles                       # the plan's own choice leaves no workgroup empty
    assert 1 <= S <= 4 and S * 4 * (32 // CB) * 16 >= Dp                # four waves of at most 32 / CB column blocks a slice
    assert p["form"] == ("staged" if D <= 1024 else "streamed")         # the form word names the route
    assert p["chunk"] == (Dp if p["form"] == "staged" else L.LINPROBE_CHUNK)
    assert 0 < p["lds_bytes"] <= 160 * 1024
    assert p["grid"] == (-(-16 * CB * Dp // 256), G * S, -(-Cn * (D + 1) // 64))
    al = lambda v: -(-v // 16) * 16
    assert p["workspace_bytes"] == al(4 * 16 * CB * Dp) + al(16 * G) + al(4 * G * Cn * (D + 1))
    assert G * Cn * (D + 1) <= 512 * Cn * (D + 1)                       # a few hundred sets of partials, never one per tile


@pytest.mark.parametrize("hint", [1, 2, 7, 129, 5000])
def test_plan_honours_the_groups_hint(lib, hint):
    from ssl_cr_histo_amd import _lib as L
    from ssl_cr_histo_amd import kernels as K
    p = K.linprobe_plan(4097, 768, 9, groups=hint)                      # 129 tiles
    assert p["groups"] == min(hint, 129, L.LINPROBE_MAX_GROUPS)
    assert p["groups"] * p["tiles_per_group"] >= 129


def test_plan_refusals(lib):
    from ssl_cr_histo_amd import _lib as L
    plan = L.LinprobePlan()
    for args, word in (((0, 4, 2, 0, 0), b"n outside"), ((2 ** 31 - 64, 4, 2, 0, 0), b"n outside"), ((1, 6, 2, 0, 0), b"D % 4"),
                       ((1, 0, 2, 0, 0), b"D % 4"), ((1, 2052, 2, 0, 0), b"D % 4"), ((1, 4, 0, 0, 0), b"C outside"),
                       ((1, 4, 65, 0, 0), b"C outside"), ((1, 4, 2, 2, 0), b"loss outside"), ((1, 4, 2, 0, -1), b"groups < 0")):
        assert lib.sslcr_linprobe_plan(*args, plan) == -1, args
        msg = lib.sslcr_last_error()
        assert msg.startswith(b"sslcr_linprobe_plan: invalid argument") and word in msg, (args, msg)
    assert lib.sslcr_linprobe_plan(1, 4, 2, 0, 0, None) == -1
    assert lib.sslcr_linprobe_plan(2 ** 31 - 65, 4, 2, 0, 0, plan) == 0


# ---------------------------------------------------------------------------------------------------------------- symbols and refusals
def test_symbols_declared_bound_and_exported(lib):
    from ssl_cr_histo_amd import _lib as L
    from ssl_cr_histo_amd import build
    names = ("sslcr_linprobe_plan", "sslcr_linprobe_eval", "sslcr_linprobe_logits")
    declared = build.header_symbols()
    for n in names:
        assert n in declared and n in L.SIGNATURES and hasattr(lib, n), n
    assert lib.sslcr_version() == 16                                    # additive: the entries are told by their symbols
    defs = build.header_defines()
    for k, v in L.LINPROBE_LOSSES.items():
        assert defs["SSLCR_LINPROBE_" + k.upper()] == v
    for v, k in enumerate(L.LINPROBE_FORMS):
        assert defs["SSLCR_LINPROBE_" + k.upper()] == v
    from ssl_cr_histo_amd import kernels as K
    for name in ("LINPROBE_TILE", "LINPROBE_CHUNK", "LINPROBE_MAX_C", "LINPROBE_MAX_D", "LINPROBE_LOSSES", "LINPROBE_FORMS"):
        assert getattr(K, name) == getattr(L, name), name


def test_entry_refusals_without_a_device(lib):
    """descriptor checks run before any device work: -1 and a message that names the entry and, for alignment, the pointer"""
    from ssl_cr_histo_amd import _lib as L
    F = 0x7F0000010000

    def D(**kw):
        base = dict(x=F, w=F, b=F, labels=F, targets=F, value=F, grad=F, logits=F, workspace=F, n=5, D=8, C=3, loss=0, groups=0)
        base.update(kw)
        d = L.LinprobeDesc()
        for k, v in base.items():
            setattr(d, k, v)
        return d
    for fn in (lib.sslcr_linprobe_eval, lib.sslcr_linprobe_logits):
        name = fn.__name__.encode() if hasattr(fn, "__name__") else b""
        assert fn(None, None) == -1 and b"null descriptor" in lib.sslcr_last_error()
        for kw, word in ((dict(n=0), b"n outside"), (dict(D=6), b"D % 4"), (dict(C=65), b"C outside"), (dict(groups=-1), b"groups < 0"),
                         (dict(x=None), b"null tensor"), (dict(w=None), b"null tensor"), (dict(b=None), b"null tensor"),
                         (dict(workspace=None), b"null tensor")):
            assert fn(D(**kw), None) == -1, kw
            msg = lib.sslcr_last_error()
            assert word in msg and msg.startswith(name), (kw, msg)
    for kw, word in ((dict(loss=2), b"loss outside"), (dict(value=None), b"null value / grad"), (dict(grad=None), b"null value / grad"),
                     (dict(labels=None), b"needs labels"), (dict(loss=1, targets=None), b"needs targets")):
        assert lib.sslcr_linprobe_eval(D(**kw), None) == -1, kw
        assert word in lib.sslcr_last_error(), (kw, lib.sslcr_last_error())
    assert lib.sslcr_linprobe_logits(D(logits=None), None) == -1 and b"null logits" in lib.sslcr_last_error()
    # alignment, in the form tests/test_abi_cpu.py holds the training entries to: "(d->name must be N-byte aligned)"
    for field, align in (("x", 16), ("workspace", 16), ("labels", 8), ("value", 8), ("grad", 8), ("w", 4), ("b", 4), ("targets", 4),
                         ("sample_weight", 4), ("logits", 4)):
        assert lib.sslcr_linprobe_eval(D(**{field: F + align // 2}), None) == -1, field
        msg = lib.sslcr_last_error().decode()
        assert msg.startswith("sslcr_linprobe_eval:") and f"(d->{field} must be {align}-byte aligned)" in msg, (field, msg)
    assert lib.sslcr_linprobe_logits(D(x=F + 8), None) == -1
    assert "sslcr_linprobe_logits:" in lib.sslcr_last_error().decode() and "(d->x must be 16-byte aligned)" in lib.sslcr_last_error().decode()


def test_wrappers_refuse_host_tensors(lib):
    import torch
    from ssl_cr_histo_amd import _lib as L
    from ssl_cr_histo_amd import inference as I
    from ssl_cr_histo_amd import kernels as K
    x, w, b = torch.zeros(5, 8), torch.zeros(3, 8), torch.zeros(3)
    with pytest.raises(L.SslcrError):
        K.linprobe_eval(x, torch.zeros(5, dtype=torch.int64), w, b)
    with pytest.raises(L.SslcrError):
        K.linprobe_logits(x, w, b)
    with pytest.raises(L.SslcrError):
        I.LinearProbe().fit(x, torch.zeros(5, dtype=torch.int64))
    with pytest.raises(ValueError):
        I.LinearProbe(C=1.0, l2=0.1)
    with pytest.raises(ValueError):
        I.LinearProbe(loss="hinge")


# ---------------------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("loss,weighted,intercept", [("softmax", False, True), ("softmax", True, True), ("squared", True, True),
                                                      ("softmax", False, False)])
def test_restatement_gradient_against_central_differences(loss, weighted, intercept):
    rng = np.random.default_rng(3)
    n, D, Cn = 40, 8, 3
    X = rng.standard_normal((n, D))
    y = rng.integers(0, Cn, n) if loss == "softmax" else rng.standard_normal((n, Cn))
    if loss == "softmax":
        y[2] = Cn                                                        # an out-of-range label: left out of both sums
    s = rng.random(n) + 0.25 if weighted else None
    theta = 0.3 * rng.standard_normal(Cn * (D + 1))
    if not intercept:
        theta.reshape(Cn, D + 1)[:, D] = 0.0
    fun = lambda t: R.objective(t, X, y, Cn, loss, 0.05, s, intercept)
    _, g = fun(theta)
    h = 1e-6
    for i in range(theta.size):
        if not intercept and i % (D + 1) == D:
            assert g[i] == 0.0
            continue
        e = np.zeros_like(theta)
        e[i] = h
        num = (fun(theta + e)[0] - fun(theta - e)[0]) / (2 * h)
        assert abs(num - g[i]) <= 1e-8 + 1e-7 * abs(g[i]), (i, num, g[i])   # central differences: h^2 f''' / 6 + 2^-53 f / h ~ 1e-10


# The gradient of the restatement AT sklearn's solution (tol = 1e-10).  Measured on these four cases (profiles/linprobe_ratios.txt):
# the largest max|g| is 2.545e-8 (balanced; 9.3e-9 multinomial, 6.8e-10 two classes, 1.8e-16 ridge); the threshold is 10 x that.
SKLEARN_GRAD_MAX = 2.545e-7
_SK = {}


def _sk_data():
    if not _SK:
        rng = np.random.default_rng(11)
        X3, y3 = R.clusters(300, 12, 4, seed=5, spread=2.0)
        X2, y2 = R.clusters(257, 8, 2, seed=6, spread=2.0)
        yb = np.where(rng.random(300) < 0.8, 0, y3)                       # unbalanced classes for "balanced"
        yb[:4] = np.arange(4)
        T = rng.standard_normal((200, 3))
        Xr = rng.standard_normal((200, 10))
        _SK.update(X3=X3.astype(np.float64), y3=y3, X2=X2.astype(np.float64), y2=y2, yb=yb, Xr=Xr, T=T)
    return _SK


def _theta(coef, intercept):
    return np.concatenate([np.atleast_2d(coef), np.asarray(intercept).reshape(-1, 1)], 1).ravel()


@pytest.mark.parametrize("case", ["multinomial", "two_class", "balanced", "ridge"])
def test_restatement_is_stationary_at_sklearns_solution(case):
    sklearn = pytest.importorskip("sklearn")
    from sklearn.linear_model import LogisticRegression, Ridge
    d = _sk_data()
    Creg = 0.7
    if case == "multinomial":
        X, y = d["X3"], d["y3"]
        m = LogisticRegression(C=Creg, tol=1e-10, max_iter=100000).fit(X, y)
        _, g = R.objective(_theta(m.coef_, m.intercept_), X, y, 4, "softmax", 1.0 / (Creg * len(y)))
    elif case == "two_class":
        X, y = d["X2"], d["y2"]
        m = LogisticRegression(C=2.0 * Creg, tol=1e-10, max_iter=100000).fit(X, y)           # sklearn's one logit w at 2 C ...
        W = np.concatenate([-0.5 * m.coef_, 0.5 * m.coef_])                                  # ... is the softmax form's [-w / 2, +w / 2]
        b = np.concatenate([-0.5 * m.intercept_, 0.5 * m.intercept_])
        _, g = R.objective(_theta(W, b), X, y, 2, "softmax", 1.0 / (Creg * len(y)))
    elif case == "balanced":
        X, y = d["X3"], d["yb"]
        m = LogisticRegression(C=Creg, tol=1e-10, max_iter=100000, class_weight="balanced").fit(X, y)
        counts = np.bincount(y, minlength=4)
        s = (len(y) / (4 * counts))[y]                                                       # sklearn's "balanced"; their sum is n
        assert abs(s.sum() - len(y)) < 1e-9
        _, g = R.objective(_theta(m.coef_, m.intercept_), X, y, 4, "softmax", 1.0 / (Creg * s.sum()), s)
    else:
        X, T = d["Xr"], d["T"]
        lam = 0.03
        m = Ridge(alpha=lam * len(X), tol=1e-12, solver="cholesky").fit(X, T)
        _, g = R.objective(_theta(m.coef_, m.intercept_), X, T, 3, "squared", lam)
    worst = float(np.abs(g).max())
    print(f"[linprobe] sklearn {sklearn.__version__} {case}: max|g| of the restatement at sklearn's solution {worst:.3e}")
    R.record(f"sklearn_{case}_max_grad", worst)
    assert worst <= SKLEARN_GRAD_MAX, worst


# ---------------------------------------------------------------------------------------------------------------- the solver
@pytest.mark.parametrize("n,D,Cn", R.E2E_CASES)
def test_lbfgs_converges_with_the_float64_evaluator(n, D, Cn):
    from ssl_cr_histo_amd import lbfgs
    X, y = R.e2e_inputs(n, D, Cn)
    X64 = X.astype(np.float64)
    lam = 1.0 / (R.E2E_C_REG * n)
    r = lbfgs.minimize(lambda t: R.objective(t, X64, y, Cn, "softmax", lam), np.zeros(Cn * (D + 1)), tol=1e-4)
    assert r.status == "converged", (r.status, r.n_iter, r.n_eval)
    assert np.abs(r.g).max() <= 1e-4 and r.n_eval <= 200
    assert np.array_equal(r.x, r.x.astype(np.float32).astype(np.float64))                    # the iterate IS a float32 point
    f, g = R.objective(r.x, X64, y, Cn, "softmax", lam)
    assert f == r.f and np.array_equal(g, r.g)                                               # ... and was evaluated where it is held
    print(f"[linprobe] lbfgs float64 ({n}, {D}, {Cn}): {r.n_iter} iterations, {r.n_eval} evaluations, max|g| {np.abs(r.g).max():.2e}")


def test_lbfgs_reports_precision_below_the_evaluators_noise():
    from ssl_cr_histo_amd import lbfgs
    n, D, Cn = 257, 8, 3
    X, y = R.clusters(n, D, Cn, seed=9)
    lam = 1.0 / (0.01 * n)
    calls = [0]

    def fun(t):
        calls[0] += 1
        return R.objective_f32(t, X, y, Cn, lam)
    r = lbfgs.minimize(fun, np.zeros(Cn * (D + 1)), tol=1e-5, max_iter=1000)
    assert r.status == "precision", (r.status, r.n_iter, float(np.abs(r.g).max()))
    assert calls[0] == r.n_eval <= 1000 * 40                             # bounded: it gave up, it did not spin
    # the same problem with the float64 evaluator converges: the status is about the evaluator, not the problem
    X64 = X.astype(np.float64)
    r64 = lbfgs.minimize(lambda t: R.objective(t, X64, y, Cn, "softmax", lam), np.zeros(Cn * (D + 1)), tol=1e-5)
    assert r64.status == "converged"


def test_lbfgs_stops_at_max_iter_and_at_a_stationary_start():
    from ssl_cr_histo_amd import lbfgs
    X, y = R.e2e_inputs(300, 16, 4)
    X64 = X.astype(np.float64)
    fun = lambda t: R.objective(t, X64, y, 4, "softmax", 1.0 / 300)
    r = lbfgs.minimize(fun, np.zeros(4 * 17), tol=1e-12, max_iter=3)
    assert r.status == "max_iter" and r.n_iter == 3 and r.log.shape == (3, 4)
    r0 = lbfgs.minimize(lambda t: (float(t @ t), 2 * t), np.zeros(5))
    assert r0.status == "converged" and r0.n_iter == 0 and r0.n_eval == 1
