"""The evaluation-mask definitions without a device: the NumPy restatements of tests/_evalmask_ref.py against scipy and brute force,
``distance_limit``, ``major_axis_lengths`` against closed forms, exact rationals and the central-moment chain, ``evaluation_mask``'s
host logic over the restatements against the challenge's steps chained with scipy, and the C-ABI's declarations and argument checks."""
import math
import os

import numpy as np
import pytest

import _evalmask_ref as R
import _froc_ref as FR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1), (1, 9), (9, 1), (5, 5), (7, 12), (23, 17)]


def _masks(n=20):
    rs = np.random.RandomState(11)
    for X, Y in SHAPES:
        for k in range(n):
            yield (rs.rand(X, Y) < rs.choice([0.3, 0.5, 0.7, 0.95])).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------- restatements
def test_distance_restatement_is_scipy_bit_for_bit_and_equals_brute_force():
    ndi = pytest.importorskip("scipy.ndimage")
    for m in _masks():
        d2 = R.d2(m)
        assert np.array_equal(d2, R.d2_brute(m))
        if (m == 0).any():                                         # scipy's answer without a zero cell is meaningless
            got = np.sqrt(d2.astype(np.float64))
            assert np.array_equal(got.view(np.uint64), ndi.distance_transform_edt(m).view(np.uint64))
        else:
            assert (d2 == R.INT32_MAX).all()
        for limit in (0, 1, 6, 24):
            assert np.array_equal(R.d2(m, limit), np.minimum(d2, limit))
            assert np.array_equal(R.d2(m, limit, invert=True), R.d2_brute(m == 0, limit))


def test_distance_patterns_against_brute_force():
    for X, Y in ((1, 1), (1, 70), (33, 65)):
        for name, m in R.edt_patterns(X, Y):
            assert np.array_equal(R.d2(m), R.d2_brute(m)), (X, Y, name)
            assert np.array_equal(R.d2(m, 6), R.d2_brute(m, 6)), (X, Y, name)


def test_fill_restatement_is_scipy():
    ndi = pytest.importorskip("scipy.ndimage")
    for m in _masks():
        assert np.array_equal(R.fill(m), ndi.binary_fill_holes(m).astype(np.uint8))
    for X, Y in ((12, 12), (33, 65), (50, 100)):
        for name, m in R.hole_patterns(X, Y):
            assert np.array_equal(R.fill(m), ndi.binary_fill_holes(m).astype(np.uint8)), (X, Y, name)


def test_fill_patterns_do_what_they_are_built_for():
    got = dict((name, (m, R.fill(m))) for name, m in R.hole_patterns(50, 100))
    m, f = got["ring"]
    assert f.sum() == 49 and m.sum() == 24
    m, f = got["ring with a diagonal leak"]
    assert f.sum() == 48 and f[2, 3] == 0 and f[3, 4] == 1          # joined to the outside diagonally only: filled
    m, f = got["ring whose hole touches the border"]
    assert np.array_equal(f, m != 0)
    m, f = got["nested rings"]
    assert f[:50, :50].all() and not f[:, 50:].any()
    m, f = got["frame"]
    assert f.all()
    assert not got["zero"][1].any() and got["one"][1].all()


def test_moments_restatement():
    labels = np.array([[1, 1, 0], [0, 2, 2], [0, 0, 2]], np.int32)
    assert R.moments(labels, 2).tolist() == [[2, 0, 1, 0, 1, 0], [3, 4, 5, 6, 9, 7]]
    assert R.moments(labels, 0).shape == (0, 6)


# ---------------------------------------------------------------------------------------------------------------- distance_limit
def test_distance_limit():
    from ssl_cr_histo_amd import kernels as K
    cases = [(75.0 / (0.243 * 32 * 2), 24), (75.0 / (0.243 * 64 * 2), 6), (2.0, 4), (5.0, 25), (math.sqrt(5.0), 5), (0.5, 1)]
    assert abs(cases[0][0] - 4.8225) < 1e-4 and abs(cases[1][0] - 2.4113) < 1e-4
    for T, want in cases:
        assert K.distance_limit(T) == want == R.limit_of(T), T
    rs = np.random.RandomState(0)
    for T in list(rs.uniform(0, 14.2, 200)) + [math.sqrt(k) for k in range(201)] + [np.nextafter(math.sqrt(k), 99.0) for k in range(201)]:
        limit = K.distance_limit(T)
        for k in range(201):
            assert (math.sqrt(float(k)) < T) == (k < limit), (T, k)
    assert K.distance_limit(0.0) == 0 == K.distance_limit(-1.0)
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError):
            K.distance_limit(bad)


# ---------------------------------------------------------------------------------------------------------------- major axis
def _moments_of(cells):
    xs, ys = np.asarray(cells, dtype=object).T
    return [len(xs), sum(xs), sum(ys), sum(x * x for x in xs), sum(y * y for y in ys), sum(x * y for x, y in zip(xs, ys))]


def test_major_axis_closed_forms():
    from ssl_cr_histo_amd import inference as I
    rows = [_moments_of([(7, 9)])]
    want = [0.0]
    for n in (2, 3, 30, 1000):
        rows.append(_moments_of([(5, 100 + k) for k in range(n)]))           # a line along y
        rows.append(_moments_of([(40000 + k, 3) for k in range(n)]))         # and along x, far from the origin
        want += [4.0 * math.sqrt((n * n - 1) / 12.0)] * 2
    for a, b in ((3, 5), (5, 3), (4, 4), (17, 60)):
        rows.append(_moments_of([(100 + i, 200 + j) for i in range(a) for j in range(b)]))
        want.append(4.0 * math.sqrt((max(a, b) ** 2 - 1) / 12.0))
    got = I.major_axis_lengths(np.asarray(rows, dtype=np.int64))
    assert got.dtype == np.float64 and got[0] == 0.0
    assert np.allclose(got, want, rtol=2.0 ** -48, atol=0.0)
    assert I.major_axis_lengths(np.zeros((0, 6), np.int64)).shape == (0,)


def _random_components():
    rs = np.random.RandomState(5)
    for k in range(40):
        X, Y = rs.randint(1, 360), rs.randint(1, 360)               # at most 2^17 cells: the bound of the central-moment chain
        m = rs.rand(X, Y) < rs.choice([0.02, 0.3, 0.9])
        m[rs.randint(X), rs.randint(Y)] = True
        x0, y0 = (0, 0) if k % 2 else (rs.randint(0, 46000 - X), rs.randint(0, 46000 - Y))
        xs, ys = np.nonzero(m)
        yield xs + x0, ys + y0


def test_major_axis_against_exact_rationals_and_the_central_moment_chain():
    """2^-48 relative against exact rationals: fewer than 16 correctly rounded operations (three quotients, each rounded once from
    exact integers, then sums, halvings, two products, two square roots), none of which cancels against l1, every intermediate of
    the l1 sum being non-negative and at most l1.  1e-10 relative against the central-moment chain: that chain sums N <= 2^17 terms
    per moment, N * 2^-53 = 1.5e-11."""
    from ssl_cr_histo_amd import inference as I
    for xs, ys in _random_components():
        assert len(xs) <= 1 << 17
        row = _moments_of(list(zip(xs.tolist(), ys.tolist())))
        got = float(I.major_axis_lengths(np.asarray([row], dtype=np.int64))[0])
        exact = R.major_axis_exact(row)
        if exact == 0:
            assert got == 0.0
            continue
        assert abs(R.Decimal(got) - exact) <= exact * R.Decimal(2) ** -48, (got, exact)
        central = R.major_axis_central(xs - xs.min(), ys - ys.min())        # translation-invariant; the chain wants small coordinates
        assert abs(got - central) <= 1e-10 * got, (got, central)


# ---------------------------------------------------------------------------------------------------------------- the chain
def _challenge(truth, cell_um, dilate_um=75.0, itc_um=275.0):
    """the challenge's steps with scipy: computeEvaluationMask (EDT of the complement, threshold, fill, label at connectivity 2) and
    computeITCList's threshold, the axis lengths from the central-moment chain (scikit-image is not required)"""
    ndi = pytest.importorskip("scipy.ndimage")
    distance = ndi.distance_transform_edt(255 - (np.asarray(truth) != 0).astype(np.uint8) * 255)
    binary = distance < dilate_um / (cell_um * 2.0)
    filled = ndi.binary_fill_holes(binary)
    labels, n = ndi.label(filled, structure=np.ones((3, 3)))
    major = R.major_axes_central(labels, n)
    return filled.astype(np.uint8), labels.astype(np.int32), n, major, [l + 1 for l in range(n) if major[l] < itc_um / cell_um]


TRUTHS = [("blobs", R.blob_truth, R.CELL_UM), ("blobs, coarse cells", R.blob_truth, 0.243 * 128), ("fixture", R.fixture_truth, R.CELL_UM),
          ("fixture negative", lambda: R.fixture_truth(positive=False), 0.243 * 32)]


@pytest.mark.parametrize("case", TRUTHS, ids=lambda c: c[0])
def test_the_restatement_chain_is_the_challenge_chain_and_the_itc_band_is_empty(case):
    _, make, cell_um = case
    truth = make()
    filled, labels, n, major, itc = _challenge(truth, cell_um)
    ref = R.evaluation(truth, cell_um)
    assert np.array_equal(ref["mask"], filled) and ref["n_lesions"] == n and np.array_equal(ref["labels"], labels)
    assert ref["itc"].tolist() == itc and np.array_equal(ref["major_axis"], major)
    assert n >= 2 and R.band_is_empty(ref["major_axis"], 275.0 / cell_um)


def test_blob_mask_holds_what_it_is_built_for():
    ref = R.evaluation(R.blob_truth(), R.CELL_UM)
    assert ref["limit"] == 6 and ref["n_lesions"] == 9
    assert 0 < len(ref["itc"]) < ref["n_lesions"]
    assert ref["mask"][86:98, 91:103].all()                         # the ring's hole is filled
    truth_n = FR.label(R.blob_truth(), 2)[1]
    assert truth_n > ref["n_lesions"]                               # the dilation merged lesions


class _HostKernels:
    """the four kernels evaluation_mask calls, as the restatements over host tensors"""

    def __init__(self):
        self.calls = []

    def distance_transform_sq(self, mask, limit=None, *, invert=False, below=False):
        import torch
        self.calls.append("distance_transform_sq")
        out = R.d2(mask.numpy(), limit, invert)
        lim = R.INT32_MAX if limit is None else limit
        return (torch.from_numpy(out), torch.from_numpy((out < lim).astype(np.uint8))) if below else torch.from_numpy(out)

    def fill_holes(self, mask):
        import torch
        self.calls.append("fill_holes")
        return torch.from_numpy(R.fill(mask.numpy()))

    def label_components(self, mask, connectivity=2):
        import torch
        self.calls.append("label_components")
        labels, n = FR.label(mask.numpy(), connectivity)
        return torch.from_numpy(labels), torch.tensor([n], dtype=torch.int32)

    def region_moments(self, labels, n):
        import torch
        self.calls.append("region_moments")
        return torch.from_numpy(R.moments(labels.numpy(), n))


@pytest.mark.parametrize("case", TRUTHS, ids=lambda c: c[0])
def test_evaluation_mask_host_logic_over_the_restatements_equals_the_challenge_chain(case, monkeypatch):
    import torch
    from ssl_cr_histo_amd import inference as I
    from ssl_cr_histo_amd import kernels as K
    _, make, cell_um = case
    truth = make()
    host = _HostKernels()
    for name in ("distance_transform_sq", "fill_holes", "label_components", "region_moments"):
        monkeypatch.setattr(K, name, getattr(host, name))
    filled, labels, n, major, itc = _challenge(truth, cell_um)
    for given in (torch.from_numpy(truth), truth != 0, (truth * 200).astype(np.int64)):
        host.calls.clear()
        ev = I.evaluation_mask(given, cell_um=cell_um, device="cpu")
        assert host.calls == ["distance_transform_sq", "fill_holes", "label_components", "region_moments"]
        assert np.array_equal(ev["mask"].numpy(), filled) and np.array_equal(ev["labels"].numpy(), labels) and ev["n_lesions"] == n
        assert ev["moments"].dtype == np.int64 and np.array_equal(ev["moments"], R.moments(labels, n))
        assert ev["major_axis"].dtype == np.float64 and np.allclose(ev["major_axis"], major, rtol=1e-10, atol=0.0)
        assert ev["itc"].dtype == np.int64 and ev["itc"].tolist() == itc
        assert ev["limit"] == K.distance_limit(75.0 / (cell_um * 2.0))
    wide = I.evaluation_mask(truth, cell_um=cell_um, dilate_um=150.0, itc_um=100.0, connectivity=1, device="cpu")
    assert wide["limit"] == K.distance_limit(150.0 / (cell_um * 2.0)) > ev["limit"] and wide["mask"].sum() > ev["mask"].sum()
    assert wide["itc"].tolist() == [l + 1 for l in range(wide["n_lesions"]) if wide["major_axis"][l] < 100.0 / cell_um]
    with pytest.raises(ValueError):
        I.evaluation_mask(truth, cell_um=0.0, device="cpu")


# ---------------------------------------------------------------------------------------------------------------- the C-ABI
@pytest.fixture(scope="module")
def lib():
    from ssl_cr_histo_amd import _lib as L
    from ssl_cr_histo_amd import build
    if not os.path.exists(L.LIB_PATH):
        build.build()
    from ssl_cr_histo_amd import engine  # noqa: F401  registers engine signatures
    return L.lib()


ENTRIES = ("sslcr_edt_squared", "sslcr_fill_holes", "sslcr_region_moments")


def test_the_entries_are_declared_exported_and_bound(lib):
    from ssl_cr_histo_amd import _lib as L
    from ssl_cr_histo_amd import build
    assert lib.sslcr_version() >= 15
    assert set(ENTRIES) <= set(build.header_symbols()) and set(ENTRIES) <= set(L.SIGNATURES)
    for name in ENTRIES:
        assert hasattr(lib, name)
    with open(os.path.join(ROOT, "include", "sslcr.h")) as f:
        text = f.read()
    assert "UNPINNED" in text and "PINNED instead" in text


OK, ODD = 0x10000, 0x10001            # stand-ins for device pointers: an argument error returns before anything reads them


def _rejected(lib, rc, what):
    assert rc == -1
    msg = lib.sslcr_last_error()
    assert b"invalid argument" in msg and what in msg, msg


def _desc(cls, pointers, **values):
    d = cls()
    for name, _ in cls._fields_:
        if name in pointers:
            setattr(d, name, OK)
    for k, v in values.items():
        setattr(d, k, v)
    return d


def test_argument_errors(lib):
    from ssl_cr_histo_amd import _lib as L

    def edt(**kw):
        return lib.sslcr_edt_squared(_desc(L.EdtDesc, ("mask", "out", "work"), **dict(dict(X=4, Y=4, limit=6, invert=0, out=OK + 64), **kw)), None)

    def fill(**kw):
        return lib.sslcr_fill_holes(_desc(L.FillDesc, ("mask", "out", "labels", "count", "work"), **dict(dict(X=4, Y=4, out=OK + 64), **kw)), None)

    def mom(**kw):
        return lib.sslcr_region_moments(_desc(L.MomentsDesc, ("labels", "moments"), **dict(dict(X=4, Y=4, L=2), **kw)), None)

    for call, entry in ((edt, lib.sslcr_edt_squared), (fill, lib.sslcr_fill_holes), (mom, lib.sslcr_region_moments)):
        _rejected(lib, entry(None, None), b"null descriptor")
        for X, Y in ((0, 4), (4, 0), (-1, 4), (1 << 16, 1 << 15)):
            _rejected(lib, call(X=X, Y=Y), b"map shape")
    for call in (edt, mom):                                        # X * Y < 2^31 but a squared distance would not fit
        for X, Y in ((46341, 1), (1, 46341), (32768, 32768), (40000, 23500)):
            _rejected(lib, call(X=X, Y=Y), b"X^2 + Y^2")
    _rejected(lib, edt(limit=-1), b"limit")
    _rejected(lib, edt(invert=2), b"invert")
    for p in ("mask", "out", "work"):
        _rejected(lib, edt(**{p: None}), b"null tensor")
        _rejected(lib, edt(**{p: ODD}), b"alignment")
    _rejected(lib, edt(out=OK, work=OK), b"aliases")
    for p in ("mask", "out", "labels", "count", "work"):
        _rejected(lib, fill(**{p: None}), b"null tensor")
    for p in ("out", "labels", "count", "work"):
        _rejected(lib, fill(**{p: ODD}), b"alignment")
    _rejected(lib, fill(out=OK), b"aliases")
    _rejected(lib, mom(L=-1), b"L < 0")
    _rejected(lib, mom(labels=None), b"null tensor")
    _rejected(lib, mom(moments=None), b"null moments")
    _rejected(lib, mom(labels=ODD), b"alignment")
    _rejected(lib, mom(moments=OK + 4), b"alignment")


def test_wrappers_refuse_host_tensors_and_bad_arguments():
    import torch
    from ssl_cr_histo_amd import _lib as L
    from ssl_cr_histo_amd import kernels as K
    m = torch.zeros((4, 4), dtype=torch.uint8)
    for call in (lambda: K.distance_transform_sq(m), lambda: K.fill_holes(m), lambda: K.region_moments(m.int(), 1)):
        with pytest.raises(L.SslcrError, match="device tensors"):
            call()
