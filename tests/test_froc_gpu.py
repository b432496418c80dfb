"""Camelyon16 lesion scoring on the MI355X.  Every bound is equality with the NumPy restatements of tests/_froc_ref.py: the component
labels and their count, the float32 smoothing chain bit for bit, the NMS detection list in the sequential loop's order, the hit
test, the areas, and ``lesion_scores`` / ``FrocMeter`` against the restatements chained on the host."""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _froc_ref as R  # noqa: E402

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "annotation_small.json")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---------------------------------------------------------------------------------------------------------------- labelling
# against the kernel's 16 x 64 tile: below one tile, no multiples of it, three tiles and more along either axis
SHAPES = [(1, 1), (1, 70), (70, 1), (33, 65), (130, 67), (257, 300)]


def _patterns(X, Y):
    rs = np.random.RandomState(1000 * X + Y)
    yield "zero", np.zeros((X, Y), np.uint8)
    yield "one", np.ones((X, Y), np.uint8)
    yield "spiral", R.spiral(X, Y)
    yield "checkerboard", R.checkerboard(X, Y)
    yield "comb", R.comb(X, Y)
    yield "u", R.u_shape(X, Y)
    yield "corner", R.corner_blobs(X, Y)
    for density in (0.3, 0.45, 0.6):                               # around both percolation thresholds
        yield f"random{density}", (rs.rand(X, Y) < density).astype(np.uint8) * rs.randint(1, 256, (X, Y)).astype(np.uint8)


@pytest.mark.parametrize("connectivity", [2, 1])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_labels_equal_the_flood_fill_and_two_calls_agree_bit_for_bit(shape, connectivity):
    from ssl_cr_histo_amd import kernels as K
    for name, mask in _patterns(*shape):
        want, n = R.label(mask, connectivity)
        m = _dev(mask)
        labels, count = K.label_components(m, connectivity)
        again, count2 = K.label_components(m, connectivity)
        assert labels.dtype == torch.int32 and labels.shape == m.shape and count.dtype == torch.int32
        assert int(count.item()) == n == int(count2.item()), (name, int(count.item()), n)
        assert np.array_equal(labels.cpu().numpy(), want), name
        assert torch.equal(labels, again), name


@pytest.mark.parametrize("connectivity", [1, 2])
def test_labels_when_the_run_offsets_take_a_second_trip(connectivity):
    """515 x 520 = 267800 cells are 262 runs of SSLCR_LABEL_RUN_CELLS = 1024: the one workgroup that turns the runs' root counts into
    offsets scans 256 of them per trip, so the last six runs are numbered from the first trip's carry (257 x 300 above makes 76 runs)"""
    from ssl_cr_histo_amd import kernels as K
    X, Y = 515, 520
    assert (X * Y + 1023) // 1024 > 256
    rs = np.random.RandomState(1000 * X + Y)
    cases = [("one", np.ones((X, Y), np.uint8)), ("checkerboard", R.checkerboard(X, Y))]
    for density in (0.45, 0.6):
        cases.append((f"random{density}", (rs.rand(X, Y) < density).astype(np.uint8) * rs.randint(1, 256, (X, Y)).astype(np.uint8)))
    for name, mask in cases:
        want, n = R.label(mask, connectivity)
        m = _dev(mask)
        labels, count = K.label_components(m, connectivity)
        again, count2 = K.label_components(m, connectivity)
        assert int(count.item()) == n == int(count2.item()), (name, int(count.item()), n)
        assert np.array_equal(labels.cpu().numpy(), want), name
        assert torch.equal(labels, again), name


def test_labels_of_a_bool_mask_and_an_unaligned_row_pitch():
    """Y = 67: no row but the first starts on a dword, and the last dword of the array is partial"""
    from ssl_cr_histo_amd import kernels as K
    mask = np.random.RandomState(5).rand(19, 67) < 0.5
    mask[-1, -3:] = True
    labels, count = K.label_components(_dev(mask), 1)
    want, n = R.label(mask, 1)
    assert int(count.item()) == n and np.array_equal(labels.cpu().numpy(), want)


# ---------------------------------------------------------------------------------------------------------------- smoothing
@pytest.mark.parametrize("sigma", [0.5, 1.0, 2.0])
@pytest.mark.parametrize("shape", [(1, 1), (5, 3), (70, 130)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_smoothing_has_the_bits_of_the_float32_chain(shape, sigma):
    from ssl_cr_histo_amd import kernels as K
    rs = np.random.RandomState(int(10 * sigma) + shape[0])
    a = rs.rand(*shape).astype(np.float32)
    a[rs.rand(*shape) < 0.25] = 0.0                                # exact 0 and 1 plateaus
    a[rs.rand(*shape) < 0.25] = 1.0
    if shape[0] > 20:
        a[10:30, 40:90] = 1.0
        a[40:60, 5:35] = 0.0
    src = _dev(a)
    got = K.gaussian_smooth(src, sigma)
    assert got.dtype == torch.float32 and got.data_ptr() != src.data_ptr()
    assert np.array_equal(got.cpu().numpy().view(np.uint32), R.smooth(a, sigma).view(np.uint32))
    assert np.array_equal(src.cpu().numpy(), a)                    # the input is left alone
    assert K.gaussian_smooth(src, 0.0) is src                      # sigma == 0: no launch, the map as given


# ---------------------------------------------------------------------------------------------------------------- NMS
def _nms_cases():
    rs = np.random.RandomState(21)
    a = rs.rand(45, 77).astype(np.float32)
    yield "random r3", a, 0.5, 3
    yield "random r1", a, 0.9, 1
    yield "random r12", rs.rand(130, 90).astype(np.float32), 0.7, 12
    yield "eighths", (np.round(rs.rand(50, 40) * 8) / 8).astype(np.float32), 0.5, 3
    yield "eighths r2", (np.round(rs.rand(33, 65) * 8) / 8).astype(np.float32), 0.25, 2
    yield "plateau", np.full((40, 40), 0.75, np.float32), 0.5, 3
    yield "ramp", np.linspace(0.6, 0.9, 200, dtype=np.float32)[None, :], 0.5, 2
    yield "r beyond both sides", rs.rand(9, 13).astype(np.float32), 0.1, 40
    yield "r beyond one side", rs.rand(150, 20).astype(np.float32), 0.6, 70
    at = rs.rand(20, 30).astype(np.float32)
    at[at > 0.5] = 0.5                                             # exactly at the threshold: no candidates
    at[3, 4], at[17, 29] = np.float32(0.5) + np.float32(2.0 ** -24), 0.5
    yield "at the threshold", at, 0.5, 2
    nan = rs.rand(25, 25).astype(np.float32)
    nan[rs.rand(25, 25) < 0.2] = np.nan
    yield "nan", nan, 0.6, 2
    corners = rs.rand(31, 47).astype(np.float32) * np.float32(0.9)
    corners[0, 0] = corners[0, -1] = corners[-1, 0] = corners[-1, -1] = 1.0
    yield "corners", corners, 0.5, 4
    yield "nothing", np.zeros((7, 9), np.float32), 0.5, 3
    yield "one cell", np.ones((1, 1), np.float32), 0.5, 1


def _run_nms(a, thr, r, cap=4096, **kw):
    from ssl_cr_histo_amd import kernels as K
    xy, prob, k = K.nms(_dev(a), thr, r, cap, **kw)
    assert xy.dtype == torch.int32 and tuple(xy.shape) == (cap, 2) and prob.dtype == torch.float32 and tuple(prob.shape) == (cap,)
    xy, prob = xy.cpu().numpy(), prob.cpu().numpy()
    return [(int(xy[i, 0]), int(xy[i, 1]), float(prob[i])) for i in range(k)]


@pytest.mark.parametrize("case", list(_nms_cases()), ids=lambda c: c[0])
def test_nms_equals_the_sequential_loop(case):
    name, a, thr, r = case
    want = R.nms(a, thr, r)
    stats = {}
    got = _run_nms(a, thr, r, stats=stats)
    print(f"{name}: {len(want)} detections, {stats}")
    assert got == want
    with np.errstate(invalid="ignore"):
        assert stats["candidates"] == int(np.count_nonzero(a > np.float32(thr)))
    assert stats["rounds"] <= stats["candidates"] + 1
    if name == "at the threshold":
        assert want == [(3, 4, float(np.float32(0.5) + np.float32(2.0 ** -24)))]
    if name == "corners":
        assert {(0, 0), (0, 46), (30, 0), (30, 46)} <= {(x, y) for x, y, _ in got}
    if name == "nothing":
        assert got == [] and stats["rounds"] == 0


def test_nms_ramp_goes_through_the_bounded_host_loop_in_batches():
    """1 x 200, r = 2: every third cell from the right is selected and each decision waits for the one before it, 134 steps by the
    definition.  A thread decides its cell at most once per launch and the 64 lanes of a wave read their states before any of them
    stores, so a launch advances the chain by at most one step in each of the four waves: at least 134 / 4 rounds."""
    from ssl_cr_histo_amd import kernels as K
    a = np.linspace(0.6, 0.9, 200, dtype=np.float32)[None, :]
    want = R.nms(a, 0.5, 2)
    assert len(want) == 67
    for every in (1, 5, None):
        stats = {}
        assert _run_nms(a, 0.5, 2, read_every=every, stats=stats) == want
        print(f"ramp, read_every {every}: {stats}")
        batch = every or K.NMS_READ_EVERY
        assert 34 <= stats["rounds"] <= 201 and stats["host_reads"] >= 2 + -(-34 // batch)


def test_nms_over_capacity_raises_and_writes_nothing_past_it():
    from ssl_cr_histo_amd import _lib as L
    from ssl_cr_histo_amd import kernels as K
    a = np.random.RandomState(8).rand(40, 40).astype(np.float32)
    want = R.nms(a, 0.5, 1)
    assert len(want) > 100
    with pytest.raises(L.SslcrError, match="max_detections"):
        K.nms(_dev(a), 0.5, 1, 100)
    assert _run_nms(a, 0.5, 1, len(want)) == want                   # exactly the capacity: fine
    # the entries themselves, on buffers with 64 canary entries behind the capacity
    cap, m = 100, _dev(a)
    state = torch.empty(m.shape, dtype=torch.uint8, device=DEV)
    cand = torch.empty(m.numel(), dtype=torch.int32, device=DEV)
    stage = torch.full((cap + 64,), -7, dtype=torch.int32, device=DEV)
    counters = torch.full((4 + 64,), -7, dtype=torch.int32, device=DEV)
    det_xy = torch.full((cap + 64, 2), -7, dtype=torch.int32, device=DEV)
    det_prob = torch.full((cap + 64,), -7.0, dtype=torch.float32, device=DEV)
    d = L.NmsDesc(L.ptr(m), L.ptr(state), L.ptr(cand), L.ptr(stage), L.ptr(counters), L.ptr(det_xy), L.ptr(det_prob), 0.5, 40, 40, 1, cap, 0)
    L.check(L.lib().sslcr_nms_candidates(d, L.stream_ptr()))
    d.ncand = int(counters[0].item())
    assert d.ncand == int(np.count_nonzero(a > np.float32(0.5)))
    for _ in range(d.ncand + 1):
        L.check(L.lib().sslcr_nms_rounds(d, 4, L.stream_ptr()))
        if int(counters[1].item()) == 0:
            break
    L.check(L.lib().sslcr_nms_collect(d, L.stream_ptr()))
    assert int(counters[2].item()) == len(want) > cap
    for t in (stage[cap:], counters[4:], det_xy[cap:], det_prob[cap:]):
        assert bool((t == -7).all())
    assert sorted(cand[:d.ncand].cpu().tolist()) == np.flatnonzero(a.ravel() > np.float32(0.5)).tolist()


# ---------------------------------------------------------------------------------------------------------------- hits
@functools.lru_cache(maxsize=None)
def _lesions():
    mask = np.zeros((50, 70), np.uint8)
    mask[2:9, 3:20] = 1                                            # lesion 1
    mask[5, 40] = 1                                                # lesion 2: one cell
    mask[20:45, 60:70] = 1                                         # lesion 3
    mask[30:33, 10:50] = 1                                         # lesion 4
    mask[49, 0] = 1                                                # lesion 5: nothing hits it
    return mask, R.label(mask, 2)


@pytest.mark.parametrize("ignore", [(), (2,), (4, 1), (9,)])
def test_hits_best_probabilities_and_areas(ignore):
    from ssl_cr_histo_amd import kernels as K
    mask, (want_labels, n) = _lesions()
    assert n == 5
    labels, count = K.label_components(_dev(mask), 2)
    det = [(3, 5, 0.9), (0, 0, 0.85), (8, 19, 0.95), (5, 40, 0.7), (31, 49, 0.65), (31, 50, 0.64), (44, 69, 0.6), (25, 60, 0.6),
           (49, 69, 0.55), (30, 10, 0.51)]
    cap = 16
    xy = np.full((cap, 2), 3, np.int32)
    prob = np.full(cap, 0.99, np.float32)                          # rows past the count: not read
    xy[:len(det)] = [(x, y) for x, y, _ in det]
    prob[:len(det)] = [p for _, _, p in det]
    want_hit, want_tp, want_fp = R.hits(want_labels, n, [(x, y, float(np.float32(p))) for x, y, p in det], ignore)
    assert want_hit.tolist() == [1, 0, 1, 2, 4, 0, 3, 3, 0, 4]      # on and off lesions, two detections on one lesion
    for n_det in (len(det), torch.tensor([len(det)], dtype=torch.int32, device=DEV)):
        hit, tp, areas = K.lesion_hits(labels, int(count.item()), _dev(xy), _dev(prob), n_det, ignore=ignore)
        assert hit.dtype == torch.int32 and tp.dtype == torch.float32 and areas.dtype == torch.int64
        assert np.array_equal(hit.cpu().numpy()[:len(det)], want_hit) and not hit[len(det):].any()
        assert np.array_equal(tp.cpu().numpy().view(np.uint32), want_tp.view(np.uint32))
        assert np.array_equal(areas.cpu().numpy(), np.bincount(want_labels.ravel(), minlength=n + 1)[1:])
    assert [p for (x, y, p), h in zip(det, want_hit) if h == 0] == [0.85, 0.64, 0.55] and len(want_fp) == 3
    assert K.lesion_hits(labels, n, _dev(xy), _dev(prob), 0, areas=False)[2] is None


def test_areas_of_many_lesions_and_no_lesions():
    from ssl_cr_histo_amd import kernels as K
    mask = (np.random.RandomState(3).rand(130, 67) < 0.45).astype(np.uint8)
    want, n = R.label(mask, 1)
    labels, count = K.label_components(_dev(mask), 1)
    xy, prob = torch.zeros((4, 2), dtype=torch.int32, device=DEV), torch.zeros(4, device=DEV)
    hit, tp, areas = K.lesion_hits(labels, int(count.item()), xy, prob, 0)
    assert np.array_equal(areas.cpu().numpy(), np.bincount(want.ravel(), minlength=n + 1)[1:]) and not tp.any() and not hit.any()
    labels, count = K.label_components(torch.zeros((5, 6), dtype=torch.uint8, device=DEV))
    hit, tp, areas = K.lesion_hits(labels, int(count.item()), xy, prob, 2)
    assert int(count.item()) == 0 and tp.numel() == 0 and areas.numel() == 0 and hit.tolist() == [0, 0, 0, 0]


# ---------------------------------------------------------------------------------------------------------------- end to end
def _slide(flag, seed, shape=(100, 100), resolution=4):
    """the fixture's polygons as a truth mask, and a map that saturates at 1.0 inside them, with noise and stray peaks outside"""
    from ssl_cr_histo_amd.annotation import Annotation
    truth = Annotation().from_json(FIXTURE).to_device(DEV).mask(shape, resolution, flag)
    rs = np.random.RandomState(seed)
    t = truth.cpu().numpy() != 0
    pm = (rs.rand(*shape) * 0.45).astype(np.float32)
    pm[t & (rs.rand(*shape) < 0.9)] = 1.0
    for _ in range(6):                                             # 5 x 5 blobs: they outlive the smoothing
        x, y = rs.randint(0, shape[0] - 5), rs.randint(0, shape[1] - 5)
        pm[x:x + 5, y:y + 5] = np.float32(rs.choice([0.625, 0.75, 0.875]))
    return truth, t, pm


def _chain(t, pm, threshold, radius, sigma, connectivity, ignore):
    labels, n = R.label(t, connectivity)
    det = R.nms(R.smooth(pm, sigma), threshold, radius)
    hit, tp, fp = R.hits(labels, n, det, ignore)
    return labels, n, det, hit, tp, fp


@pytest.mark.parametrize("sigma,ignore", [(0.0, None), (1.0, (2,))])
def test_lesion_scores_and_froc_meter_against_the_host_chain(sigma, ignore):
    from ssl_cr_histo_amd import inference as I
    meter, fps, tps = I.FrocMeter(), [], []
    for flag, seed, as_host in ((True, 1, False), (False, 2, True)):
        truth, t, pm = _slide(flag, seed)
        labels, n, det, hit, tp, fp = _chain(t, pm, 0.5, 6, sigma, 2, ignore or ())
        assert n >= 2 and len(det) > n and len(fp) >= 1
        got = I.lesion_scores(pm if as_host else _dev(pm), t if as_host else truth, threshold=0.5, radius=6, sigma=sigma, ignore=ignore)
        assert got["n_lesions"] == n and got["detections"].shape == (len(det), 3) and got["detections"].dtype == np.float64
        assert [(int(x), int(y), float(p)) for x, y, p in got["detections"]] == det
        assert np.array_equal(got["hit"], hit) and np.array_equal(got["tp_prob"], tp.astype(np.float64))
        assert np.array_equal(got["fp_prob"], np.asarray(fp, dtype=np.float64))
        assert np.array_equal(got["areas"], np.bincount(labels.ravel(), minlength=n + 1)[1:])
        assert got["ignore"].tolist() == sorted(ignore or ())
        meter.update(got)
        fps += fp
        tps += [p for l, p in enumerate(tp, 1) if l not in (ignore or ())]
    res = meter.result()
    avg_fp, sens, score = R.froc(fps, tps, 2, len(tps))
    assert np.array_equal(res["avg_fp"], avg_fp) and np.array_equal(res["sensitivity"], sens) and res["score"] == score
    want = I.froc(fps, tps, 2, len(tps))
    assert res["score"] == want["score"] and 0 < res["score"] <= 1
