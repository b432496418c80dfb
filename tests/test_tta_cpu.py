"""CPU-only: the host side of test-time augmentation over D4 -- the three C-ABI entries (header, ctypes, exports, descriptor layout,
argument checks), the orientation codes (``inference.d4_apply`` / ``d4_codes``) against explicit NumPy compositions and against the
index formula include/sslcr.h pins for the kernels, and the rule that ``args.tta`` absent or None issues the calls of the plain path."""
import ctypes as C
import itertools
import os
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sslcr_d4_transform", "sslcr_wsi_gather_d4", "sslcr_predict_tta")


@pytest.fixture(scope="module")
def lib():
    from ssl_cr_histo_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    return _lib.lib()


def test_header_ctypes_and_exports_agree_on_the_new_entries(lib):
    from ssl_cr_histo_amd import _lib, build
    names = build.header_symbols()
    for n in NEW:
        assert n in names, f"{n} not declared in include/sslcr.h"
        assert n in _lib.SIGNATURES, f"no ctypes signature for {n}"
        assert hasattr(lib, n), f"{n} not exported by libsslcr.so"
    assert lib.sslcr_version() >= 13
    assert len(names) >= 87                                  # the three entries are additive


def test_new_descriptor_mirrors_match_the_header_layout():
    """(sizes and offsets: tests/test_abi_cpu.py, for every mirror)  The ensemble's size limit, and the plain descriptor embedded whole"""
    from ssl_cr_histo_amd import _lib as L
    from ssl_cr_histo_amd import build
    assert build.header_defines()["SSLCR_TTA_MAX"] == 8
    assert {"sslcr_d4_desc", "sslcr_predict_tta_desc"} <= set(L.MIRRORS)
    assert L.PredictTtaDesc.p.size == C.sizeof(L.PredictDesc)


# ---------------------------------------------------------------------------------------------------------------- the codes
def _tile():
    t = np.arange(3 * 5 * 5, dtype=np.int32).reshape(3, 5, 5)           # every element distinct: no symmetry of any kind
    return (t * 7 + 3) % 251


def test_d4_apply_is_flip_then_quarter_turns():
    from ssl_cr_histo_amd.inference import d4_apply
    t = _tile()
    hflip, vflip = np.flip(t, -1), np.flip(t, -2)
    rot = lambda a, k: np.rot90(a, k, axes=(-2, -1))                    # counter-clockwise
    want = {0: t, 1: rot(t, 1), 2: rot(t, 2), 3: rot(t, 3),
            4: hflip, 5: rot(hflip, 1), 6: rot(hflip, 2), 7: rot(hflip, 3)}
    for g in range(8):
        got = d4_apply(t, g)
        assert got.shape == t.shape and got.dtype == t.dtype and got.flags["C_CONTIGUOUS"]
        assert np.array_equal(got, want[g]), g
    # the same elements under their usual names
    assert np.array_equal(d4_apply(t, 2), np.flip(t, (-2, -1)))                       # half turn
    assert np.array_equal(d4_apply(t, 6), vflip)                                      # h-flip then a half turn = vertical flip
    assert np.array_equal(d4_apply(t, 5), np.swapaxes(t, -1, -2))                     # transpose
    assert np.array_equal(d4_apply(t, 7), np.flip(np.swapaxes(t, -1, -2), (-2, -1)))  # anti-transpose
    assert np.array_equal(d4_apply(t, 1)[:, 0, :], t[:, :, -1])                       # ccw: the last column becomes the first row
    # leading axes of any count; torch tensors are taken too
    assert np.array_equal(d4_apply(t[None, None], 3)[0, 0], want[3]) and np.array_equal(d4_apply(t[0], 5), want[5][0])
    assert np.array_equal(d4_apply(torch.from_numpy(t), 7), want[7])
    for bad in (-1, 8):
        with pytest.raises(ValueError):
            d4_apply(t, bad)
    with pytest.raises(ValueError, match="square"):
        d4_apply(np.zeros((3, 4, 5)), 1)


def test_the_eight_orientations_differ_and_are_closed_under_composition():
    from ssl_cr_histo_amd.inference import d4_apply
    t = _tile()
    imgs = [d4_apply(t, g) for g in range(8)]
    for a, b in itertools.combinations(range(8), 2):
        assert not np.array_equal(imgs[a], imgs[b]), (a, b)
    table = np.empty((8, 8), int)
    for g, h in itertools.product(range(8), repeat=2):
        both = d4_apply(imgs[g], h)
        hits = [c for c in range(8) if np.array_equal(both, imgs[c])]
        assert len(hits) == 1, (g, h, hits)
        table[g, h] = hits[0]
    assert all(sorted(table[g]) == list(range(8)) and sorted(table[:, g]) == list(range(8)) for g in range(8))    # a group table
    assert all(table[g, 0] == g and table[0, g] == g for g in range(8))
    inverse = {g: int(np.where(table[g] == 0)[0][0]) for g in range(8)}
    assert inverse == {0: 0, 1: 3, 2: 2, 3: 1, 4: 4, 5: 5, 6: 6, 7: 7}                 # the reflections are their own inverses


@pytest.mark.parametrize("S", [1, 4, 5])
def test_header_index_formula_is_d4_apply(S):
    """include/sslcr.h: d4(t, g)[i][j] = t[si][sj] -- the arithmetic the kernels carry out"""
    from ssl_cr_histo_amd.inference import d4_apply
    t = np.random.RandomState(S).randint(0, 256, size=(2, S, S)).astype(np.uint8)
    for g in range(8):
        k, f = g & 3, g >> 2
        got = np.empty_like(t)
        for i, j in itertools.product(range(S), repeat=2):
            a, b = (j, i) if k & 1 else (i, j)
            si = S - 1 - a if k >> 1 else a
            sj = S - 1 - b if (((k + 1) >> 1) & 1) ^ f else b
            got[:, i, j] = t[:, si, sj]
        assert np.array_equal(got, d4_apply(t, g)), g


def test_d4_codes_named_sets_and_rejections():
    from ssl_cr_histo_amd.inference import D4_SETS, d4_codes
    assert d4_codes("d4") == (0, 1, 2, 3, 4, 5, 6, 7)
    assert d4_codes("rot90") == (0, 1, 2, 3)
    assert d4_codes("flips") == (0, 4, 6)
    assert set(D4_SETS) == {"d4", "rot90", "flips"}
    assert d4_codes((3, 5)) == (3, 5) and d4_codes([7]) == (7,) and d4_codes(np.array([2, 0])) == (2, 0)       # the order is kept
    assert all(type(g) is int for g in d4_codes(np.array([2, 0])))
    for bad in ((1, 1), (0, 4, 0), (8,), (-1,), (0, 1.5), (True,), (), "rot180", 3, None):
        with pytest.raises(ValueError):
            d4_codes(bad)


# ---------------------------------------------------------------------------------------------------------------- argument checks
def test_argument_errors_are_decided_before_any_launch(lib):
    """no device here: every call below must return before it touches one"""
    from ssl_cr_histo_amd import _lib as L
    one, far = C.c_void_p(1 << 12), C.c_void_p(1 << 20)      # non-null pointers that are never followed

    def err(rc, word):
        assert rc == -1
        assert word in lib.sslcr_last_error(), lib.sslcr_last_error()

    # sslcr_d4_transform: src, dst, orient, N, Cn, H, W, elem_bytes
    good = L.D4Desc(one, far, one, 2, 3, 8, 8, 1)
    assert lib.sslcr_d4_transform(None, None) == -1
    for fields, word in (({"src": None}, b"null"), ({"dst": None}, b"null"), ({"orient": None}, b"null"), ({"N": -1}, b"N >= 0"),
                         ({"Cn": 0}, b"Cn >= 1"), ({"H": 0, "W": 0}, b"H >= 1"), ({"W": 9}, b"square"), ({"H": 7}, b"square"),
                         ({"elem_bytes": 2}, b"elem_bytes"), ({"elem_bytes": 4, "src": C.c_void_p((1 << 12) + 2)}, b"aligned"),
                         ({"orient": C.c_void_p((1 << 12) + 1)}, b"orient"),
                         ({"dst": one}, b"overlap"),                                          # in place
                         ({"dst": C.c_void_p((1 << 12) + 2 * 3 * 64 - 1)}, b"overlap"),       # the last byte of src
                         ({"src": C.c_void_p((1 << 20) + 5)}, b"overlap")):
        d = L.D4Desc.from_buffer_copy(good)
        for k, v in fields.items():
            setattr(d, k, v)
        err(lib.sslcr_d4_transform(d, None), word)
    d = L.D4Desc.from_buffer_copy(good)
    d.N, d.src, d.dst, d.orient = 0, None, None, None
    assert lib.sslcr_d4_transform(d, None) == 0                # N == 0: a no-op

    # sslcr_wsi_gather_d4: the plain gather's rules, with or without a table
    g = L.WsiGatherDesc(one, one, one, 0, 0, 1, 8, 8, 4, 0)
    assert lib.sslcr_wsi_gather_d4(None, one, None) == -1 and lib.sslcr_wsi_gather_d4(None, None, None) == -1
    for orient in (one, None):
        for field, bad, word in (("S", 0, b"S >= 1"), ("N", -1, b"N >= 0"), ("src", None, b"null"), ("xy", None, b"null"),
                                 ("dst", None, b"null"), ("fill", 256, b"fill"), ("RH", 0, b"region")):
            d = L.WsiGatherDesc.from_buffer_copy(g)
            setattr(d, field, bad)
            err(lib.sslcr_wsi_gather_d4(d, orient, None), word)
    err(lib.sslcr_wsi_gather_d4(g, C.c_void_p((1 << 12) + 2), None), b"orient")
    d = L.WsiGatherDesc.from_buffer_copy(g)
    d.N, d.xy, d.dst = 0, None, None
    assert lib.sslcr_wsi_gather_d4(d, one, None) == 0 and lib.sslcr_wsi_gather_d4(d, None, None) == 0

    # sslcr_predict_tta: sslcr_predict's rules and three of its own
    def tta(G=2, mode=0, **kw):
        p = L.PredictDesc(one, 4, 9, None, None, None, None, 0, None, None, 0)
        for k, v in kw.items():
            setattr(p, k, v)
        return L.PredictTtaDesc(p, G, mode)

    eight = C.c_void_p(1 << 13)
    assert lib.sslcr_predict_tta(None, None) == -1
    for d, word in ((tta(G=0), b"G outside"), (tta(G=9), b"G outside"), (tta(G=-1), b"G outside"), (tta(mode=2), b"mode outside"),
                    (tta(mode=-1), b"mode outside"), (tta(mode=1, map=one, map_index=one), b"mode 1"), (tta(mode=1, pred=eight), b"mode 1"),
                    (tta(mode=1, confusion=eight, target=one), b"mode 1"),
                    (tta(C=0), b"C <= 64"), (tta(C=65), b"C <= 64"), (tta(n=-1), b"n >= 0"), (tta(logits=None), b"null logits"),
                    (tta(confusion=eight), b"confusion needs target"), (tta(map=one), b"map_index"),
                    (tta(map=one, map_index=one, col=9), b"col"), (tta(map=one, map_index=one, col=-1), b"col")):
        err(lib.sslcr_predict_tta(d, None), word)
    assert lib.sslcr_predict_tta(tta(n=0, logits=None), None) == 0            # n == 0: a no-op
    assert lib.sslcr_predict_tta(tta(G=8, mode=1, n=0), None) == 0
    # the plain entry kept its own words
    p = L.PredictDesc(one, 4, 9, None, None, None, eight, 0, None, None, 0)
    err(lib.sslcr_predict(p, None), b"confusion needs target")


def test_wrappers_refuse_host_tensors_and_bad_shapes():
    from ssl_cr_histo_amd import _lib as L
    from ssl_cr_histo_amd import kernels as K
    with pytest.raises(L.SslcrError, match="device tensors"):
        K.d4_transform(torch.zeros((1, 3, 4, 4), dtype=torch.uint8), torch.zeros(1, dtype=torch.int32))
    with pytest.raises(L.SslcrError, match="device tensors"):
        K.predict_tta(torch.zeros((2, 4, 9)))


# ---------------------------------------------------------------------------------------------------------------- args.tta unset
class _FakeNet:
    ncls = 2

    def __init__(self):
        self.forwards = 0

    def forward(self, xs, train):
        assert train is False
        self.forwards += 1
        n = xs[0].shape[0]
        return torch.zeros((n, 768)), torch.zeros((n, self.ncls))


class _FakeEngine:
    device = torch.device("cpu")

    def __init__(self):
        self.net = _FakeNet()

    def bind(self, model, classifier):
        return self.net


@pytest.fixture()
def wsi_spies(monkeypatch):
    """camelyon16_test on a WsiDeviceLoader whose region stays in host memory, with the engine and the three kernel wrappers replaced
    by recorders: which calls a run ISSUES is decided on the host"""
    from ssl_cr_histo_amd import kernels as K
    from ssl_cr_histo_amd import steps
    from ssl_cr_histo_amd.inference import WsiDeviceLoader
    calls = {"predict": [], "predict_tta": [], "wsi_gather": []}

    def predict(logits, target=None, **kw):
        calls["predict"].append((tuple(logits.shape), sorted(kw)))
        return {}

    def predict_tta(logits, target=None, **kw):
        calls["predict_tta"].append((tuple(logits.shape), sorted(kw)))
        return {}

    def wsi_gather(region, xy, size, *, origin=(0, 0), fill=0, out=None, orient=None):
        calls["wsi_gather"].append(None if orient is None else orient.tolist())
        return torch.zeros((xy.shape[0], 3, size, size), dtype=torch.uint8)

    eng = _FakeEngine()
    monkeypatch.setattr(K, "predict", predict)
    monkeypatch.setattr(K, "predict_tta", predict_tta)
    monkeypatch.setattr(K, "wsi_gather", wsi_gather)
    monkeypatch.setattr(steps, "get_engine", lambda device=None, dtype=None: eng)
    region = np.zeros((32, 48, 3), np.uint8)
    loader = WsiDeviceLoader(region, np.ones((6, 4), bool), 8, 5, device="cpu")            # 24 tiles: four batches of 5 and one of 4
    assert loader.dataset.resolution == 8 and len(loader) == 5
    model = torch.nn.Linear(1, 1)
    return calls, eng, loader, lambda args: steps.camelyon16_test(args, model, model, loader)


def test_tta_absent_or_none_issues_the_calls_of_the_plain_path(wsi_spies):
    calls, eng, loader, run = wsi_spies
    for args in (types.SimpleNamespace(print_freq=0), types.SimpleNamespace(print_freq=0, tta=None)):
        for v in calls.values():
            v.clear()
        eng.net.forwards = 0
        out = run(args)
        assert out.shape == (6, 4) and out.dtype == np.float64
        assert calls["predict_tta"] == []
        assert calls["wsi_gather"] == [None] * 5                                     # the plain gather, once per batch
        assert [c[0] for c in calls["predict"]] == [(5, 2)] * 4 + [(4, 2)]           # sslcr_predict, once per batch
        assert all(c[1] == ["col", "map", "map_index", "pred"] for c in calls["predict"])
        assert eng.net.forwards == 5


def test_tta_set_issues_g_gathers_and_forwards_and_one_reduce_per_batch(wsi_spies):
    calls, eng, loader, run = wsi_spies
    run(types.SimpleNamespace(print_freq=0, tta="flips"))
    assert calls["predict"] == []
    assert [c[0] for c in calls["predict_tta"]] == [(3, 5, 2)] * 4 + [(3, 4, 2)]
    assert all(c[1] == ["col", "map", "map_index", "pred"] for c in calls["predict_tta"])
    assert eng.net.forwards == 15
    want = []
    for n in (5, 5, 5, 5, 4):
        want += [[g] * n for g in (0, 4, 6)]                                          # one code for the whole range, in the order listed
    assert calls["wsi_gather"] == want
    with pytest.raises(ValueError):
        run(types.SimpleNamespace(print_freq=0, tta=(1, 1)))
    with pytest.raises(ValueError):
        run(types.SimpleNamespace(print_freq=0, tta="rot45"))


def test_tta_selection_of_the_other_loops():
    from ssl_cr_histo_amd import steps
    assert steps._tta_codes(types.SimpleNamespace()) is None and steps._tta_codes(types.SimpleNamespace(tta=None)) is None
    assert steps._tta_codes(types.SimpleNamespace(tta="rot90")) == (0, 1, 2, 3)
    assert steps._tta_codes(types.SimpleNamespace(tta=[6, 1])) == (6, 1)
    # non-square inputs raise before anything is uploaded or launched
    o = steps._Orientations(_FakeEngine(), (0, 1))
    with pytest.raises(ValueError, match="square"):
        next(o.members(torch.zeros((2, 3, 8, 9), dtype=torch.uint8)))
    with pytest.raises(ValueError, match="square"):
        next(o.members(torch.zeros((3, 8, 8), dtype=torch.uint8)))
