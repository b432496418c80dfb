"""Camelyon16 lesion scoring, the part that needs no device: the restatements of tests/_froc_ref.py against scipy where it is
installed (labelling, smoothing) and against one another (the round-based NMS definition against the sequential loop), ``inference.froc``
and ``FrocMeter`` against the literal transcription, the layout of the new descriptors and every documented argument error of the new
entries, which the C-ABI rejects before any launch."""
import os

import numpy as np
import pytest

import _froc_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------------------- labelling
@pytest.mark.parametrize("connectivity", [1, 2])
def test_labeller_numbers_like_scipy(connectivity):
    ndi = pytest.importorskip("scipy.ndimage")
    structure = ndi.generate_binary_structure(2, connectivity)
    rs = np.random.RandomState(10 + connectivity)
    masks = [rs.rand(rs.randint(1, 40), rs.randint(1, 40)) < d for d in (0.3, 0.45, 0.6) for _ in range(40)]
    masks += [R.u_shape(9, 7), R.comb(8, 11), R.spiral(13, 17), R.checkerboard(6, 9), R.corner_blobs(40, 70)]
    for m in masks:
        want, n = ndi.label(m, structure)
        got, k = R.label(m, connectivity)
        assert k == n and np.array_equal(got, want)


def test_labeller_patterns_have_the_components_they_are_built_for():
    assert R.label(R.spiral(33, 65), 1)[1] == 1 and R.label(R.spiral(33, 65), 2)[1] == 1
    assert R.label(R.checkerboard(33, 65), 2)[1] == 1 and R.label(R.checkerboard(33, 65), 1)[1] == (33 * 65 + 1) // 2
    assert R.label(R.comb(33, 65), 1)[1] == 1 and R.label(R.u_shape(33, 65), 1)[1] == 1
    assert R.label(R.corner_blobs(130, 67), 2)[1] == 2 and R.label(R.corner_blobs(130, 67), 1)[1] == 4
    lab, n = R.label(np.array([[0, 1, 0, 1], [1, 1, 0, 1], [0, 0, 0, 0], [1, 0, 1, 1]]), 1)
    assert n == 4 and lab.tolist() == [[0, 1, 0, 2], [1, 1, 0, 2], [0, 0, 0, 0], [3, 0, 4, 4]]      # numbered by first cell


# ---------------------------------------------------------------------------------------------------------------- smoothing
@pytest.mark.parametrize("sigma", [0.5, 1.0, 2.0])
def test_float32_smoothing_chain_against_scipy_float64(sigma):
    """Bound.  u = 2^-24 is float32's unit roundoff, T = 2R + 1 the tap count, the map lies in [0, 1] and the float64 weights sum to
    1, so every partial sum stays within [0, 1] up to rounding.  One pass differs from its exact value by at most: u from the weights'
    cast (each w_k moves by a factor 1 + d, |d| <= u, and sum w_k v_k <= 1), u from the T products (each off by u w_k v_k), and T u from
    the T sums (each off by u times a partial sum <= 1): (T + 2) u.  The second pass carries the first's error through weights that
    sum to 1 and adds its own: 2 (T + 2) u = (2 T + 4) u to first order.  The bound asserted is (4 T + 2) u >= (2 T + 4) u for T >= 1,
    which leaves the second-order terms (a factor 1 + O(T u)) and scipy's own float64 rounding (2^-53 per operation) far inside it.
    scipy's ``gaussian_filter(mode="nearest")`` truncates at 4 sigma, the same R, and filters axis 0 first."""
    ndi = pytest.importorskip("scipy.ndimage")
    T = 2 * int(4 * sigma + 0.5) + 1
    bound = (4 * T + 2) * 2.0 ** -24
    rs = np.random.RandomState(int(sigma * 10))
    for shape in ((1, 1), (5, 3), (40, 57)):
        a = rs.rand(*shape).astype(np.float32)
        a[rs.rand(*shape) < 0.2] = 0.0
        a[rs.rand(*shape) < 0.2] = 1.0
        got = R.smooth(a, sigma)
        assert got.dtype == np.float32
        want = ndi.gaussian_filter(a.astype(np.float64), sigma, mode="nearest")
        err = float(np.abs(got.astype(np.float64) - want).max())
        print(f"sigma {sigma} shape {shape}: max error {err:.3e}, bound {bound:.3e}")
        assert err <= bound


def test_smoothing_weights_and_identity():
    from ssl_cr_histo_amd import kernels as K
    for sigma in (0.5, 1.0, 2.0, 16.0):
        w = K.gaussian_weights(sigma)
        assert w.dtype == np.float32 and len(w) == 2 * int(4 * sigma + 0.5) + 1 and np.array_equal(w, R.gaussian_weights(sigma))
        assert np.array_equal(w, w[::-1]) and abs(float(w.astype(np.float64).sum()) - 1) <= len(w) * 2.0 ** -25
    a = np.random.RandomState(0).rand(4, 5).astype(np.float32)
    assert R.smooth(a, 0) is not None and np.array_equal(R.smooth(a, 0), a)
    assert np.array_equal(R.smooth(np.ones((6, 4), np.float32) * 0.0, 1.0), np.zeros((6, 4), np.float32))


# ---------------------------------------------------------------------------------------------------------------- NMS
def test_round_based_definition_equals_the_sequential_loop():
    rs = np.random.RandomState(3)
    most = 0
    for k in range(60):
        a = rs.rand(rs.randint(1, 14), rs.randint(1, 14)).astype(np.float32)
        if k % 2:
            a = (np.round(a * 8) / 8).astype(np.float32)           # eighths: ties abound
        if k % 5 == 0:
            a[rs.rand(*a.shape) < 0.1] = np.nan
        r = int(rs.randint(1, 5))
        want = R.nms(a, 0.5, r)
        got, rounds = R.nms_rounds(a, 0.5, r)
        assert got == want
        most = max(most, rounds)
    assert most >= 3
    plateau = np.full((12, 12), 0.75, np.float32)
    got, rounds = R.nms_rounds(plateau, 0.5, 3)
    assert got == R.nms(plateau, 0.5, 3) and len(got) == 16 and rounds > 4
    ramp = np.linspace(0.6, 0.9, 60, dtype=np.float32)[None, :]
    got, rounds = R.nms_rounds(ramp, 0.5, 2)
    assert got == R.nms(ramp, 0.5, 2) and len(got) == 20 and rounds == 2 * len(got)


def test_a_selected_cell_does_not_remove_a_cell_that_precedes_it():
    """r = 2 on one row: y = 1 (0.99), 2 (0.95), 3 (0.9), 5 (0.8).  Cell 5 has no predecessor whose window holds it and is selected in
    round 1; its window [3, 7) holds cell 3, which PRECEDES it and is still undecided then (it waits for 2, which waits for 1).  Cell 2
    falls to 1, so 3 is selected in round 3: a schedule that let 5 remove 3 would lose it."""
    a = np.zeros((1, 8), np.float32)
    a[0, [1, 2, 3, 5]] = [0.99, 0.95, 0.9, 0.8]
    want = [(0, 1, float(np.float32(0.99))), (0, 3, float(np.float32(0.9))), (0, 5, float(np.float32(0.8)))]
    assert R.nms(a, 0.5, 2) == want
    got, rounds = R.nms_rounds(a, 0.5, 2)
    assert got == want and rounds == 3


def test_nms_threshold_and_nan_are_no_candidates():
    a = np.array([[0.5, np.nan, 0.5000001, 0.2]], np.float32)
    assert R.nms(a, 0.5, 1) == [(0, 2, float(np.float32(0.5000001)))] == R.nms_rounds(a, 0.5, 1)[0]


# ---------------------------------------------------------------------------------------------------------------- FROC
def _froc_cases():
    rs = np.random.RandomState(5)
    yield [], [], 1, 0                                             # nothing at all
    yield [0.9, 0.7], [], 2, 0                                     # no lesions
    yield [], [0.0, 0.0, 0.0], 3, 3                                # no detections: every lesion keeps 0
    yield [0.75, 0.5, 0.75], [0.75, 0.0, 0.5, 1.0], 2, 4           # ties between FP and TP probabilities
    for _ in range(20):
        nf, nt = rs.randint(0, 40), rs.randint(0, 12)
        fp = np.round(rs.rand(nf) * 16) / 16 if rs.rand() < 0.5 else rs.rand(nf)
        tp = np.where(rs.rand(nt) < 0.3, 0.0, np.round(rs.rand(nt) * 16) / 16)
        yield fp.astype(np.float32), tp.astype(np.float32), int(rs.randint(1, 5)), nt


def test_froc_equals_the_transcription():
    from ssl_cr_histo_amd import inference as I
    for fp, tp, n_slides, n_lesions in _froc_cases():
        avg_fp, sens, score = R.froc(fp, tp, n_slides, n_lesions)
        got = I.froc(fp, tp, n_slides, n_lesions)
        assert np.array_equal(got["avg_fp"], avg_fp) and np.array_equal(got["sensitivity"], sens) and got["score"] == score
        assert got["avg_fp"][-1] == 0 and got["sensitivity"][-1] == 0 and 0 <= got["score"] <= 1
    assert I.froc([], [], 1, 0)["score"] == 0
    # one slide, two lesions both found above every false positive: sensitivity 1 at every operating point
    assert I.froc([0.6, 0.55], [0.9, 0.8], 1, 2)["score"] == R.froc([0.6, 0.55], [0.9, 0.8], 1, 2)[2] > 0.9


def test_froc_meter_concatenates_slides_and_leaves_ignored_lesions_out():
    from ssl_cr_histo_amd import inference as I
    slides = [dict(fp_prob=np.array([0.9, 0.6]), tp_prob=np.array([0.8, 0.0, 0.7]), n_lesions=3, ignore=np.array([2])),
              dict(fp_prob=np.array([]), tp_prob=np.array([]), n_lesions=0, ignore=np.array([], dtype=np.int64)),
              dict(fp_prob=np.array([0.7]), tp_prob=np.array([0.0, 0.95]), n_lesions=2, ignore=np.array([], dtype=np.int64))]
    meter = I.FrocMeter()
    for s in slides:
        meter.update(s)
    got = meter.result()
    avg_fp, sens, score = R.froc([0.9, 0.6, 0.7], [0.8, 0.7, 0.0, 0.95], 3, 4)
    assert np.array_equal(got["avg_fp"], avg_fp) and np.array_equal(got["sensitivity"], sens) and got["score"] == score
    assert I.FrocMeter().result()["score"] == 0


def test_hits_restatement():
    labels = np.array([[1, 1, 0], [0, 0, 2], [3, 0, 2]], np.int32)
    det = [(0, 0, 0.9), (2, 2, 0.8), (0, 1, 0.95), (1, 0, 0.7), (2, 0, 0.6)]
    hit, tp, fp = R.hits(labels, 3, det, ignore=(3,))
    assert hit.tolist() == [1, 2, 1, 0, 3] and fp == [0.7]
    assert tp.tolist() == [np.float32(0.95), np.float32(0.8), 0.0]


# ---------------------------------------------------------------------------------------------------------------- the C-ABI
@pytest.fixture(scope="module")
def lib():
    from ssl_cr_histo_amd import _lib as L
    from ssl_cr_histo_amd import build
    if not os.path.exists(L.LIB_PATH):
        build.build()
    from ssl_cr_histo_amd import engine  # noqa: F401  registers engine signatures
    return L.lib()


ENTRIES = ("sslcr_label_components", "sslcr_gaussian_smooth", "sslcr_nms_candidates", "sslcr_nms_rounds", "sslcr_nms_collect",
           "sslcr_lesion_hits")


def test_the_entries_are_declared_exported_and_bound(lib):
    from ssl_cr_histo_amd import _lib as L
    from ssl_cr_histo_amd import build
    assert lib.sslcr_version() >= 15
    assert set(ENTRIES) <= set(build.header_symbols()) and set(ENTRIES) <= set(L.SIGNATURES)
    for name in ENTRIES:
        assert hasattr(lib, name)


OK, ODD = 0x10000, 0x10001            # stand-ins for device pointers: an argument error returns before anything reads them


def _rejected(lib, rc, what):
    assert rc == -1
    msg = lib.sslcr_last_error()
    assert b"invalid argument" in msg and what in msg, msg


def _desc(cls, pointers, **ints):
    d = cls()
    for name, _ in cls._fields_:
        if name in pointers:
            setattr(d, name, OK)
    for k, v in ints.items():
        setattr(d, k, v)
    return d


def _shape_errors(lib, call, make):
    for X, Y in ((0, 4), (4, 0), (-1, 4), (1 << 16, 1 << 15), (46341, 46341)):      # X < 1, Y < 1, X * Y >= 2^31
        _rejected(lib, call(make(X=X, Y=Y)), b"map shape")


def test_label_components_argument_errors(lib):
    from ssl_cr_histo_amd import _lib as L
    ptrs = ("mask", "labels", "count", "work")

    def make(**kw):
        return _desc(L.LabelDesc, ptrs, **dict(dict(X=4, Y=4, connectivity=2), **kw))

    def call(d):
        return lib.sslcr_label_components(d, None)
    _rejected(lib, lib.sslcr_label_components(None, None), b"null descriptor")
    _shape_errors(lib, call, make)
    for c in (0, 3, -1):
        _rejected(lib, call(make(connectivity=c)), b"connectivity")
    for p in ptrs:
        _rejected(lib, call(make(**{p: None})), b"null tensor")
        _rejected(lib, call(make(**{p: ODD})), b"alignment")


def test_gaussian_smooth_argument_errors(lib):
    from ssl_cr_histo_amd import _lib as L
    ptrs = ("src", "tmp", "dst", "weights")

    def make(**kw):
        d = _desc(L.SmoothDesc, ptrs, **dict(dict(X=4, Y=4, R=2), **kw))
        if "tmp" not in kw:
            d.tmp = OK + 0x1000
        return d

    def call(d):
        return lib.sslcr_gaussian_smooth(d, None)
    _rejected(lib, lib.sslcr_gaussian_smooth(None, None), b"null descriptor")
    _shape_errors(lib, call, make)
    for R_ in (65, -1, 1000):
        _rejected(lib, call(make(R=R_)), b"R outside")
    for p in ptrs:
        _rejected(lib, call(make(**{p: None})), b"null tensor")
        _rejected(lib, call(make(**{p: ODD})), b"alignment")
    _rejected(lib, call(make(tmp=OK)), b"aliases")


def test_nms_argument_errors(lib):
    from ssl_cr_histo_amd import _lib as L
    ptrs = ("map", "state", "cand", "stage", "counters", "det_xy", "det_prob")

    def make(**kw):
        return _desc(L.NmsDesc, ptrs, **dict(dict(X=4, Y=4, radius=1, max_detections=8, ncand=0, threshold=0.5), **kw))
    calls = (lambda d: lib.sslcr_nms_candidates(d, None), lambda d: lib.sslcr_nms_rounds(d, 1, None),
             lambda d: lib.sslcr_nms_collect(d, None))
    for call in calls:
        _rejected(lib, call(None), b"null descriptor")
        _shape_errors(lib, call, make)
        for r in (0, -3):
            _rejected(lib, call(make(radius=r)), b"radius < 1")
        _rejected(lib, call(make(max_detections=0)), b"max_detections")
        for n in (-1, 17):
            _rejected(lib, call(make(ncand=n)), b"ncand")
        for p in ptrs:
            _rejected(lib, call(make(**{p: None})), b"null tensor")
            _rejected(lib, call(make(**{p: ODD})), b"alignment")
    _rejected(lib, lib.sslcr_nms_rounds(make(), -1, None), b"rounds < 0")


def test_lesion_hits_argument_errors(lib):
    from ssl_cr_histo_amd import _lib as L
    ptrs = ("labels", "det_xy", "det_prob", "n_det", "ignore", "hit", "tp_prob", "areas")

    def make(**kw):
        return _desc(L.HitsDesc, ptrs, **dict(dict(X=4, Y=4, L=2, max_detections=8, n_ignore=1), **kw))

    def call(d):
        return lib.sslcr_lesion_hits(d, None)
    _rejected(lib, lib.sslcr_lesion_hits(None, None), b"null descriptor")
    _shape_errors(lib, call, make)
    for kw in (dict(L=-1), dict(max_detections=0), dict(n_ignore=-1)):
        _rejected(lib, call(make(**kw)), b"n_ignore >= 0")
    for p in ("labels", "det_xy", "det_prob", "n_det", "hit"):
        _rejected(lib, call(make(**{p: None})), b"null tensor")
    _rejected(lib, call(make(tp_prob=None)), b"null tp_prob")
    _rejected(lib, call(make(ignore=None)), b"null ignore")
    for p in ptrs:
        _rejected(lib, call(make(**{p: ODD})), b"alignment")
    _rejected(lib, call(make(areas=OK + 4)), b"areas alignment")


def test_wrappers_refuse_host_tensors_and_bad_arguments():
    import torch
    from ssl_cr_histo_amd import _lib as L
    from ssl_cr_histo_amd import kernels as K
    with pytest.raises(L.SslcrError):
        K.label_components(torch.zeros(4, 4, dtype=torch.uint8))
    with pytest.raises(L.SslcrError):
        K.gaussian_smooth(torch.zeros(4, 4), 1.0)
    with pytest.raises(L.SslcrError):
        K.nms(torch.zeros(4, 4), 0.5, 2)
    with pytest.raises(L.SslcrError):
        K.lesion_hits(torch.zeros(4, 4, dtype=torch.int32), 0, torch.zeros(4, 2, dtype=torch.int32), torch.zeros(4), 0)
