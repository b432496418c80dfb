"""The Camelyon16 evaluation mask on the MI355X.  Every comparison is equality with the NumPy restatements of tests/_evalmask_ref.py:
the squared distances (unlimited and at limits 1, 6, 24), the filled masks, the int64 moments, and ``evaluation_mask`` /
``lesion_scores(evaluation=)`` against the restatements chained on the host."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _evalmask_ref as R  # noqa: E402
import _froc_ref as FR  # noqa: E402

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROW = 1024                                                         # SSLCR_EDT_ROW_CELLS: the cells of a row the EDT's row pass sweeps per chunk
# the labeller's 16 x 64 tile and the EDT's 4 x 64 tile: below one tile, no multiples of it, several tiles along either axis; then
# rows of one chunk + 3 cells (every row but the first starts off a dword), of two chunks + 5, and one of exactly one chunk
SHAPES = [(1, 1), (1, 70), (70, 1), (33, 65), (130, 67), (257, 300)]
EDT_SHAPES = SHAPES + [(3, ROW + 3), (2, 2 * ROW + 5), (5, ROW)]
LIMITS = (None, 1, 6, 24)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---------------------------------------------------------------------------------------------------------------- distance transform
@pytest.mark.parametrize("shape", EDT_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_squared_distances_equal_the_restatement_and_two_calls_agree_bit_for_bit(shape):
    from ssl_cr_histo_amd import kernels as K
    assert K.EDT_ROW_CELLS == ROW
    for name, mask in R.edt_patterns(*shape):
        m = _dev(mask)
        full = R.d2(mask)                                          # d2(mask, limit) = min(d2(mask), limit): tests/test_evalmask_cpu.py
        for limit in LIMITS:
            want = full if limit is None else np.minimum(full, limit)
            got = K.distance_transform_sq(m, limit)
            again, below = K.distance_transform_sq(m, limit, below=True)
            assert got.dtype == torch.int32 and got.shape == m.shape and below.dtype == torch.uint8
            assert np.array_equal(got.cpu().numpy(), want), (name, limit)
            assert torch.equal(got, again), (name, limit)
            assert np.array_equal(below.cpu().numpy(), want < (R.INT32_MAX if limit is None else limit)), (name, limit)
        if name == "all one":
            assert bool((K.distance_transform_sq(m) == R.INT32_MAX).all()) and bool((K.distance_transform_sq(m, 6) == 6).all())
        assert np.array_equal(m.cpu().numpy(), mask)               # the input is left alone


def test_squared_distances_of_a_bool_mask_an_unaligned_row_pitch_and_the_inverted_sense():
    """Y = 67: no row but the first starts on a dword, and the last dword of the array is partial"""
    from ssl_cr_histo_amd import kernels as K
    mask = np.random.RandomState(5).rand(19, 67) < 0.9
    mask[-1, -3:] = [True, False, True]
    for limit in LIMITS:
        assert np.array_equal(K.distance_transform_sq(_dev(mask), limit).cpu().numpy(), R.d2(mask, limit))
        got, below = K.distance_transform_sq(_dev(mask), limit, invert=True, below=True)
        want = R.d2(mask, limit, invert=True)
        assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(got.cpu().numpy(), R.d2(~mask, limit))
        assert np.array_equal(below.cpu().numpy(), want < (R.INT32_MAX if limit is None else limit))


def test_squared_distances_are_scipys_distances():
    ndi = pytest.importorskip("scipy.ndimage")
    from ssl_cr_histo_amd import kernels as K
    mask = (np.random.RandomState(9).rand(130, 67) < 0.97).astype(np.uint8)
    got = K.distance_transform_sq(_dev(mask)).cpu().numpy()
    assert np.array_equal(np.sqrt(got.astype(np.float64)).view(np.uint64), ndi.distance_transform_edt(mask).view(np.uint64))


def test_distance_transform_refuses_what_it_cannot_hold():
    from ssl_cr_histo_amd import _lib as L
    from ssl_cr_histo_amd import kernels as K
    with pytest.raises(L.SslcrError, match="2\\^31"):
        K.distance_transform_sq(torch.zeros((46341, 1), dtype=torch.uint8, device=DEV))
    with pytest.raises(L.SslcrError, match="limit"):
        K.distance_transform_sq(torch.zeros((4, 4), dtype=torch.uint8, device=DEV), -1)
    with pytest.raises(L.SslcrError):
        K.distance_transform_sq(torch.zeros((4, 4), dtype=torch.int32, device=DEV))


# ---------------------------------------------------------------------------------------------------------------- hole filling
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_filled_masks_equal_the_restatement(shape):
    from ssl_cr_histo_amd import kernels as K
    names = []
    for name, mask in R.hole_patterns(*shape):
        m = _dev(mask)
        got = K.fill_holes(m)
        assert got.dtype == torch.uint8 and got.shape == m.shape
        assert np.array_equal(got.cpu().numpy(), R.fill(mask)), name
        assert torch.equal(got, K.fill_holes(m)) and np.array_equal(m.cpu().numpy(), mask), name
        names.append(name)
    assert {"zero", "one", "random0.55", "random0.7"} <= set(names)
    if shape == (257, 300):
        assert {"ring", "ring with a diagonal leak", "ring whose hole touches the border", "nested rings", "rings across tiles"} <= set(names)


def test_filled_bool_mask_is_scipys():
    ndi = pytest.importorskip("scipy.ndimage")
    from ssl_cr_histo_amd import kernels as K
    mask = np.random.RandomState(2).rand(130, 67) < 0.6
    assert np.array_equal(K.fill_holes(_dev(mask)).cpu().numpy(), ndi.binary_fill_holes(mask).astype(np.uint8))


# ---------------------------------------------------------------------------------------------------------------- moments
def _label_patterns(X, Y):
    rs = np.random.RandomState(1000 * X + Y)
    yield "zero", np.zeros((X, Y), np.uint8)
    yield "one", np.ones((X, Y), np.uint8)                         # one component spanning the whole array
    yield "spiral", FR.spiral(X, Y)
    yield "checkerboard", FR.checkerboard(X, Y)
    yield "comb", FR.comb(X, Y)
    yield "u", FR.u_shape(X, Y)
    yield "corner", FR.corner_blobs(X, Y)
    for density in (0.3, 0.45, 0.6):
        yield f"random{density}", (rs.rand(X, Y) < density).astype(np.uint8)


def _moments_fast(labels, n):
    """the restatement's sums with bincount on int64 weights held exactly (every partial sum here stays far below 2^53)"""
    l = labels.ravel().astype(np.int64)
    x, y = (v.ravel().astype(np.float64) for v in np.indices(labels.shape))
    cols = [np.bincount(l, weights=w, minlength=n + 1)[1:n + 1] for w in (np.ones_like(x), x, y, x * x, y * y, x * y)]
    return np.stack(cols, 1).astype(np.int64).reshape(n, 6)


@pytest.mark.parametrize("connectivity", [2, 1])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_moments_equal_the_integer_sums(shape, connectivity):
    from ssl_cr_histo_amd import kernels as K
    for name, mask in _label_patterns(*shape):
        labels, count = K.label_components(_dev(mask), connectivity)
        n = int(count.item())
        got = K.region_moments(labels, n)
        assert got.dtype == torch.int64 and tuple(got.shape) == (n, 6), name
        want = _moments_fast(labels.cpu().numpy(), n)
        assert np.array_equal(got.cpu().numpy(), want), name
        assert torch.equal(got, K.region_moments(labels, n)), name
        if name == "one":
            X, Y = shape
            sx, sy, sxx, syy = X * (X - 1) // 2, Y * (Y - 1) // 2, (X - 1) * X * (2 * X - 1) // 6, (Y - 1) * Y * (2 * Y - 1) // 6
            assert n == 1 and got.cpu().numpy()[0].tolist() == [X * Y, Y * sx, X * sy, Y * sxx, X * syy, sx * sy]
        if name == "zero":
            assert n == 0 and got.numel() == 0


def test_moments_restatement_agrees_with_the_fast_form_and_labels_outside_the_range_are_left_out():
    from ssl_cr_histo_amd import kernels as K
    mask = (np.random.RandomState(4).rand(33, 65) < 0.45).astype(np.uint8)
    labels, n = FR.label(mask, 2)
    assert np.array_equal(R.moments(labels, n), _moments_fast(labels, n))
    got = K.region_moments(_dev(labels), n - 3)                    # the last three labels are outside 1..n - 3
    assert np.array_equal(got.cpu().numpy(), R.moments(labels, n)[:n - 3])
    assert K.region_moments(_dev(labels), 0).shape == (0, 6)


# ---------------------------------------------------------------------------------------------------------------- end to end
@functools.lru_cache(maxsize=None)
def _truths():
    from ssl_cr_histo_amd.annotation import Annotation
    fixture = Annotation().from_json(R.FIXTURE).to_device(DEV).mask((100, 100), 4, True).cpu().numpy()
    assert np.array_equal(fixture, R.fixture_truth())
    return {"fixture": (fixture, R.evaluation(fixture, R.CELL_UM)), "blobs": (R.blob_truth(), R.evaluation(R.blob_truth(), R.CELL_UM))}


@pytest.mark.parametrize("which", ["fixture", "blobs"])
def test_evaluation_mask_equals_the_restatements_chained_on_the_host(which):
    from ssl_cr_histo_amd import inference as I
    truth, ref = _truths()[which]
    threshold = 275.0 / R.CELL_UM
    assert R.band_is_empty(ref["major_axis"], threshold)           # the ITC decision is a float comparison: nothing sits at it
    for given in (_dev(truth), truth != 0):
        ev = I.evaluation_mask(given, cell_um=R.CELL_UM)
        assert ev["mask"].is_cuda and ev["mask"].dtype == torch.uint8 and ev["labels"].dtype == torch.int32
        assert np.array_equal(ev["mask"].cpu().numpy(), ref["mask"]) and np.array_equal(ev["labels"].cpu().numpy(), ref["labels"])
        assert ev["n_lesions"] == ref["n_lesions"] and ev["limit"] == ref["limit"] == 6
        assert ev["moments"].dtype == np.int64 and np.array_equal(ev["moments"], ref["moments"])
        assert ev["major_axis"].dtype == np.float64 and np.allclose(ev["major_axis"], ref["major_axis"], rtol=1e-10, atol=0.0)
        assert R.band_is_empty(ev["major_axis"], threshold)
        assert ev["itc"].tolist() == ref["itc"].tolist()
    if which == "blobs":
        assert 0 < len(ref["itc"]) < ref["n_lesions"]


def _map_for(truth, mask, seed):
    """saturated inside the truth, noise below the threshold elsewhere, stray blobs, and peaks in the dilation's rim"""
    rs = np.random.RandomState(seed)
    pm = (rs.rand(*truth.shape) * 0.45).astype(np.float32)
    pm[(truth != 0) & (rs.rand(*truth.shape) < 0.9)] = 1.0
    rim = np.argwhere((mask != 0) & (truth == 0))
    for x, y in rim[rs.choice(len(rim), 12, replace=False)]:
        pm[x, y] = np.float32(rs.choice([0.625, 0.75, 0.875]))
    for _ in range(6):
        x, y = rs.randint(0, truth.shape[0] - 5), rs.randint(0, truth.shape[1] - 5)
        pm[x:x + 5, y:y + 5] = np.float32(rs.choice([0.625, 0.75, 0.875]))
    return pm


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
        assert np.asarray(a[k]).dtype == np.asarray(b[k]).dtype, k


@pytest.mark.parametrize("which", ["fixture", "blobs"])
def test_lesion_scores_with_an_evaluation_mask(which):
    from ssl_cr_histo_amd import inference as I
    truth, ref = _truths()[which]
    pm = _map_for(truth, ref["mask"], 3)
    ev = I.evaluation_mask(_dev(truth), cell_um=R.CELL_UM)
    got = I.lesion_scores(_dev(pm), None, threshold=0.5, radius=2, evaluation=ev)
    _same(got, I.lesion_scores(_dev(pm), ev["mask"], threshold=0.5, radius=2, ignore=ev["itc"]))
    _same(got, I.lesion_scores(pm, truth, threshold=0.5, radius=2, evaluation=ev))        # truth is not used
    # against the restatements chained on the host
    det = FR.nms(pm, 0.5, 2)
    hit, tp, fp = FR.hits(ref["labels"], ref["n_lesions"], det, ref["itc"].tolist())
    assert [(int(x), int(y), float(p)) for x, y, p in got["detections"]] == det
    assert np.array_equal(got["hit"], hit) and np.array_equal(got["tp_prob"], tp.astype(np.float64))
    assert np.array_equal(got["fp_prob"], np.asarray(fp, dtype=np.float64))
    assert got["n_lesions"] == ref["n_lesions"] and got["ignore"].tolist() == ref["itc"].tolist()
    assert np.array_equal(got["areas"], ref["moments"][:, 0])
    # an explicit ignore list overrides the ITC list
    none = I.lesion_scores(_dev(pm), None, threshold=0.5, radius=2, evaluation=ev, ignore=())
    assert none["ignore"].tolist() == [] and np.array_equal(none["tp_prob"], FR.hits(ref["labels"], ref["n_lesions"], det)[1].astype(np.float64))
    # the dilation turns false positives of the raw truth mask into hits
    raw = I.lesion_scores(_dev(pm), _dev(truth), threshold=0.5, radius=2)
    assert len(raw["fp_prob"]) > len(none["fp_prob"])
    with pytest.raises(ValueError, match="shape"):
        I.lesion_scores(_dev(pm[:, :-1]), None, evaluation=ev)


def test_lesion_scores_without_an_evaluation_is_what_it_was():
    """the same call as before the evaluation mask existed, bits against the restatement chain (as tests/test_froc_gpu.py holds it)"""
    from ssl_cr_histo_amd import inference as I
    truth, ref = _truths()["blobs"]
    pm = _map_for(truth, ref["mask"], 4)
    for sigma, ignore in ((0.0, None), (1.0, (2,))):
        labels, n = FR.label(truth, 2)
        det = FR.nms(FR.smooth(pm, sigma), 0.5, 6)
        hit, tp, fp = FR.hits(labels, n, det, ignore or ())
        got = I.lesion_scores(_dev(pm), _dev(truth), threshold=0.5, radius=6, sigma=sigma, ignore=ignore)
        assert sorted(got) == ["areas", "detections", "fp_prob", "hit", "ignore", "n_lesions", "tp_prob"]
        assert [(int(x), int(y), float(p)) for x, y, p in got["detections"]] == det and got["n_lesions"] == n
        assert np.array_equal(got["hit"], hit) and np.array_equal(got["tp_prob"], tp.astype(np.float64))
        assert np.array_equal(got["fp_prob"], np.asarray(fp, dtype=np.float64))
        assert np.array_equal(got["areas"], np.bincount(labels.ravel(), minlength=n + 1)[1:])
        assert got["ignore"].tolist() == sorted(ignore or ())
