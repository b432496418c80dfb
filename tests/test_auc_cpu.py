"""CPU-only: the definitions the device ranking metrics are held to (tests/_auc_ref.py) against sklearn, the key map, the errors of
``inference.roc_auc``, and the host-side intraclass correlations."""
import os
import warnings

import numpy as np
import pytest

import _auc_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _targets(rs, n, C):
    t = rs.randint(0, C, n)
    t[:C] = np.arange(C)[:n]                                        # every class present (n >= C)
    return t


# ---------------------------------------------------------------------------------------------------------------- restatement
@pytest.mark.parametrize("n", [2, 3, 17, 257, 4097, 20000])
def test_restatement_against_sklearn_binary(n):
    """sklearn's trapezoid is a float64 sum of at most n terms whose total is at most 1: |difference| <= n 2^-53.  Measured here over
    these sizes and score sets: the worst ratio to that bound was 0.0046."""
    from sklearn.metrics import roc_auc_score
    rs = np.random.RandomState(n)
    for name, s in R.score_sets(n, 100 + n).items():
        t = _targets(rs, n, 2)
        c = R.counts(s, t, positive=[1])
        want = roc_auc_score(t, s)
        got = R.auc_from_counts(c)
        print(name, n, abs(got - want) / (n * 2.0 ** -53))
        assert abs(got - want) <= n * 2.0 ** -53, (name, n)
        if n <= 257:
            assert c[0, 0] == R.u2_brute(s, t == 1)
        assert c[0, 1] == (t == 1).sum() and c[0, 2] == (t != 1).sum() and c[0, 3] == 0


@pytest.mark.parametrize("average", ["macro", "weighted"])
@pytest.mark.parametrize("n", [40, 7180])
def test_restatement_against_sklearn_one_vs_rest(n, average):
    """the nine-class one-vs-rest figure under both averages, same bound (measured here: 0.0)"""
    from sklearn.metrics import roc_auc_score
    rs = np.random.RandomState(n + 1)
    logits = rs.randn(n, 9).astype(np.float32) * 2
    t = _targets(rs, n, 9)
    e = np.exp(logits.astype(np.float64) - logits.max(1, keepdims=True))
    p = e / e.sum(1, keepdims=True)                                 # float64 rows that sum to 1 under sklearn's check
    p32 = p.astype(np.float32)                                      # sslcr_predict's precision; sklearn takes rows that sum to 1 within 1e-5
    c = R.counts(p32, t)
    want = roc_auc_score(t, p32.astype(np.float64), multi_class="ovr", average=average)
    got = R.auc_from_counts(c, average)
    print(n, average, abs(got - want) / (n * 2.0 ** -53))
    assert abs(got - want) <= n * 2.0 ** -53


def test_brute_force_definition_on_ties_zeros_and_masks():
    rs = np.random.RandomState(5)
    for n in (1, 2, 5, 64, 300):
        for name, s in R.score_sets(n, n).items():
            pos = rs.rand(n) < 0.4
            valid = rs.rand(n) < 0.7
            u2, P, N, nan = R.counts_1d(s, pos, valid)
            assert (u2, P, N, nan) == (R.u2_brute(s[valid], pos[valid]), int((pos & valid).sum()), int((~pos & valid).sum()), 0), (name, n)
    s = np.array([0.5, np.nan, 0.25, np.nan, 0.75], dtype=np.float32)
    assert R.counts_1d(s, np.array([1, 1, 0, 0, 0], bool), np.array([1, 1, 1, 0, 1], bool)) == (2, 1, 2, 1)     # 0.5 > 0.25 only; one valid NaN


# ---------------------------------------------------------------------------------------------------------------- key map
def test_key_map_is_strictly_monotone_and_ties_the_zeros():
    f = np.finfo(np.float32)
    tiny = np.float32(1e-45)                                        # the smallest denormal
    ladder = np.array([-np.inf, -f.max, -1.0, -f.tiny, -tiny, 0.0, tiny, f.tiny, 1.0, f.max, np.inf], dtype=np.float32)
    k = R.key_map(ladder).astype(np.int64)
    assert np.all(np.diff(k) > 0)
    z = R.key_map(np.array([0.0, -0.0], dtype=np.float32))
    assert z[0] == z[1] == 0x80000000
    rs = np.random.RandomState(3)
    v = rs.randn(4000).astype(np.float32) * np.float32(10.0) ** rs.randint(-30, 30, 4000).astype(np.float32)
    kv = R.key_map(v).astype(np.int64)
    i, j = rs.randint(0, 4000, 20000), rs.randint(0, 4000, 20000)
    assert np.array_equal(v[i] < v[j], kv[i] < kv[j]) and np.array_equal(v[i] == v[j], kv[i] == kv[j])


# ---------------------------------------------------------------------------------------------------------------- errors
def test_the_four_sklearn_errors():
    from sklearn.metrics import roc_auc_score
    from ssl_cr_histo_amd import inference as I
    rs = np.random.RandomState(9)
    s, t = rs.rand(20).astype(np.float32), _targets(rs, 20, 2)
    # 1. a NaN score
    bad = s.copy()
    bad[3] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        roc_auc_score(t, bad)
    with pytest.raises(ValueError, match="NaN"):
        I.auc_from_counts(R.counts(bad, t, positive=[1]))
    # 2. one class only
    for only in (0, 1):
        # sklearn raised this as a ValueError up to 1.5 and warns (returning nan) since: either way it gives no figure
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            with pytest.raises((ValueError, Warning), match="Only one class (is )?present"):
                roc_auc_score(np.full(20, only), s)
        with pytest.raises(ValueError, match="Only one class present"):
            I.auc_from_counts(R.counts(s, np.full(20, only), positive=[1]))
    # 3. multi-class scores without multi_class='ovr': refused before any device work
    p = rs.rand(20, 3).astype(np.float32)
    t3 = _targets(rs, 20, 3)
    with pytest.raises(ValueError, match="multi_class must be in"):
        roc_auc_score(t3, p.astype(np.float64) / p.astype(np.float64).sum(1, keepdims=True))
    with pytest.raises(ValueError, match="multi_class must be in"):
        I.roc_auc(p, t3)
    # 4. under one-vs-rest, a class of range(C) absent from the targets
    t_missing = np.where(t3 == 2, 0, t3)
    with pytest.raises(ValueError, match="Number of classes in y_true not equal"):
        roc_auc_score(t_missing, p.astype(np.float64) / p.astype(np.float64).sum(1, keepdims=True), multi_class="ovr")
    with pytest.raises(ValueError, match="Number of classes in y_true not equal"):
        I.auc_from_counts(R.counts(p, t_missing), multi=True)
    # the figures where nothing is wrong
    assert I.auc_from_counts(R.counts(s, t, positive=[1])) == R.auc_from_counts(R.counts(s, t, positive=[1]))
    for average in ("macro", "weighted", None):
        assert np.array_equal(I.auc_from_counts(R.counts(p, t3), multi=True, average=average), R.auc_from_counts(R.counts(p, t3), average))


# ---------------------------------------------------------------------------------------------------------------- ICC
SHROUT_FLEISS = [[9, 2, 5, 8], [6, 1, 3, 2], [8, 4, 6, 8], [7, 1, 2, 6], [10, 5, 6, 9], [6, 2, 4, 7]]


def test_icc_on_shrout_and_fleiss_table():
    """Shrout & Fleiss (1979), table 2 and 4: 0.17, 0.29, 0.71, 0.44, 0.62, 0.91 (here 0.1657, 0.2898, 0.7148, 0.4428, 0.6201, 0.9093)"""
    from ssl_cr_histo_amd import inference as I
    r = I.icc(SHROUT_FLEISS)
    assert list(r["Type"]) == ["ICC1", "ICC2", "ICC3", "ICC1k", "ICC2k", "ICC3k"]
    assert [round(float(v), 2) for v in r["ICC"]] == [0.17, 0.29, 0.71, 0.44, 0.62, 0.91]
    assert np.allclose(r["ICC"], [0.1657, 0.2898, 0.7148, 0.4428, 0.6201, 0.9093], atol=5e-5, rtol=0)
    assert list(r["df1"]) == [5] * 6 and list(r["df2"]) == [18, 15, 15, 18, 15, 15]
    assert np.allclose(r["F"], [1.7947, 11.0272, 11.0272, 1.7947, 11.0272, 11.0272], atol=5e-5, rtol=0)
    assert r["CI95"].shape == (6, 2) and r["pval"].shape == (6,)
    try:
        import scipy.stats  # noqa: F401
    except ImportError:
        assert np.isnan(r["pval"]).all() and np.isnan(r["CI95"]).all()
    else:
        assert np.all(r["CI95"][:, 0] < r["ICC"]) and np.all(r["ICC"] < r["CI95"][:, 1]) and np.all((r["pval"] > 0) & (r["pval"] < 1))


@pytest.mark.parametrize("shape", [(2, 2), (6, 4), (11, 2), (50, 3)])
def test_icc_equals_the_literal_restatement(shape):
    """the vectorised two-pass sums against loops over the table: the same deviations squared, summed in another order -- a relative
    2 n k 2^-53 on every sum of squares, which the six ratios of differences amplify by at most the condition of MSR - MSW; the
    tables here keep MSR well above MSW, and 1e-12 covers it with room"""
    from ssl_cr_histo_amd import inference as I
    rs = np.random.RandomState(shape[0] * 10 + shape[1])
    x = rs.rand(shape[0], 1) * 3 + rs.rand(*shape) * 0.5 + rs.rand(1, shape[1]) * 0.2
    want, ms = R.icc_literal(x)
    got = I.icc(x)
    m = I.icc_mean_squares(x)
    for key in ("MSR", "MSW", "MSC", "MSE"):
        assert abs(m[key] - ms[key]) <= 1e-13 * abs(ms[key]), key
    assert (m["n"], m["k"]) == shape
    assert np.allclose(got["ICC"], want, rtol=0, atol=1e-12)


def test_bpq_icc_is_icc_of_the_three_stacked_pairs():
    import torch
    from ssl_cr_histo_amd import inference as I
    rs = np.random.RandomState(12)
    a = rs.rand(11).astype(np.float32)
    b = (a + rs.randn(11) * 0.05).astype(np.float32)
    m = (a + rs.randn(11) * 0.1).astype(np.float32)
    r = I.bpq_icc(torch.from_numpy(m), torch.from_numpy(a), torch.from_numpy(b))
    assert list(r) == ["MA", "MB", "AB"]
    for key, (u, v) in dict(MA=(m, a), MB=(m, b), AB=(a, b)).items():
        want = I.icc(np.stack([u, v], 1).astype(np.float64))
        for field in ("ICC", "F", "df1", "df2", "pval", "CI95"):
            assert np.array_equal(r[key][field], want[field], equal_nan=True), (key, field)
    with pytest.raises(ValueError):
        I.icc(np.zeros((1, 2)))
    with pytest.raises(ValueError):
        I.bpq_icc(m, a, b[:5])


# ---------------------------------------------------------------------------------------------------------------- the C-ABI
def test_the_new_header_symbols_are_declared_bound_and_exported():
    from ssl_cr_histo_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    names = {"sslcr_sort_pairs", "sslcr_sort_workspace_bytes", "sslcr_rank_keys", "sslcr_auc_counts", "sslcr_auc_workspace_bytes"}
    assert names <= set(build.header_symbols()) and names <= set(_lib.SIGNATURES)
    lib = _lib.lib()
    for n in names:
        assert hasattr(lib, n)
    assert lib.sslcr_version() == 16
    # sizes: hist [B][256][tiles] + tot [B][256] ints; 8 ints per block and column; 0 for refused arguments
    T = _lib.SORT_TILE
    assert lib.sslcr_sort_workspace_bytes(3, 2 * T + 1) == 3 * 256 * (3 + 1) * 4 and lib.sslcr_sort_workspace_bytes(0, 5) == 0
    assert lib.sslcr_auc_workspace_bytes(9, T) == 9 * 1 * 8 * 4 and lib.sslcr_auc_workspace_bytes(1, 0) == 0
    # descriptor checks run before any device work
    assert lib.sslcr_sort_pairs(_lib.SortDesc(), None) == -1 and b"B outside" in lib.sslcr_last_error()
    assert lib.sslcr_rank_keys(_lib.RankKeysDesc(), None) == -1 and b"n < 1" in lib.sslcr_last_error()
    assert lib.sslcr_auc_counts(_lib.AucDesc(), None) == -1 and b"n < 1" in lib.sslcr_last_error()
