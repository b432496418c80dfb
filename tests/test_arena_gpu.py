"""The float64 bodies of tests/test_kernels_gpu.py and tests/test_fp8_gpu.py once more, with every tensor the library sees relocated
into a poisoned arena at the least alignment include/sslcr.h allows (tests/_arena.py): every operand between two 128 KiB bands of the
fill byte, every wrapper-made output filled with it, every pointer at a multiple of its stated alignment A and of no 2 A.  The bodies
run unchanged and their own float64 bounds judge the values (no tolerance here): an over-read that reaches a sum, an element a
ragged tail left unwritten and a kernel that assumed more alignment than the header states all show as a NaN (fill 0xFF) or as
3.39e38 (fill 0x7F, which survives the ReLU and the max-pool that drop a NaN) in a checked tensor; a write out of range shows in the
guard check that ends every call.  Both fills, every row of tests/kernel_routes.py, every row of tests/nonconv_cases.py and
tests/fp8_cases.py whose batch is fixed, the stem bodies over their own parameter lists, the optimizer step for both kinds.

A fault stops the file (tests/_arena.py: FAULTED): every later test fails at once without launching."""
import itertools

import pytest

import _arena as A
import nonconv_cases as NC
import test_fp8_gpu as F8T
import test_kernels_gpu as T
from fp8_cases import CASES as F8_CASES
from kernel_routes import ROUTES

pytestmark = pytest.mark.gpu

fills = pytest.mark.parametrize("fill", A.FILLS, ids=[f"fill{f:02X}" for f in A.FILLS])

# op of tests/nonconv_cases.py -> the body that runs its rows in tests/test_kernels_gpu.py
BODIES = {"bn_finalize": T.test_bn_finalize_f64, "bn_act": T.test_bn_act_f64, "pool": T.test_pool_f64, "bn_bwd": T.test_bn_bwd_f64,
          "linear": T.test_linear_f64, "loss": T.test_loss_f64, "softmax_col": T.test_softmax_col_f64}
# ... and of the rows that exist only above the grid cap (N = None: sized from the device, too large for a per-call copy)
ABOVE_THE_CAP = {"bn_relu_maxpool": T.test_maxpool_generic_above_the_cap_f64, "bn_bwd_apply": T.test_bn_bwd_apply_odd_width_above_the_cap_f64}


def _sized_from_the_device(shape):
    return shape[0] is None


NONCONV = [r for r in NC.CASES if not _sized_from_the_device(r[2])]
FP8 = [r for r in F8_CASES if not _sized_from_the_device(r[0])]


def _own_params(fn):
    """the parameter sets of a parametrised test of another module, from its own marks -> [kwargs]"""
    axes = []
    for m in fn.pytestmark:
        if m.name == "parametrize":
            names = [n.strip() for n in m.args[0].split(",")]
            axes.append([dict(zip(names, v if len(names) > 1 else (v,))) for v in m.args[1]])
    return [{k: v for d in combo for k, v in d.items()} for combo in itertools.product(*axes)]


def _kw_id(kw):
    return "-".join(f"{k}={'x'.join(map(str, v)) if isinstance(v, tuple) else v}" for k, v in sorted(kw.items()))


def run_in_arena(fill, monkeypatch, body, *args, **kwargs):
    """the body, unchanged, inside arena(fill): at least one launch of it must have gone through relocated pointers"""
    if A.FAULTED:
        pytest.fail(f"not started: {A.FAULTED[0]}")
    with A.arena(fill, monkeypatch) as a:
        body(*args, **kwargs)
    assert a.launches >= 1, f"{a.calls} calls reached the library, none through a relocated pointer"
    return a


def test_only_rows_sized_from_the_device_are_left_out():
    """conditions of this file over the tables: a row is left out only if its batch is None, every other row has a body here, and
    every routed conv instance is covered (all of ROUTES: no row of it is sized from the device)"""
    for row in NC.CASES:
        if _sized_from_the_device(row[2]):
            assert row not in NONCONV and row[0] in set(BODIES) | set(ABOVE_THE_CAP), row
        else:
            assert row in NONCONV and row[0] in BODIES and None not in row[2], row
    assert {r[0] for r in NC.STRIDE} >= set(ABOVE_THE_CAP) and all(_sized_from_the_device(r[2]) for r in NC.STRIDE)
    assert len(NONCONV) + sum(_sized_from_the_device(r[2]) for r in NC.CASES) == len(NC.CASES) and len(NONCONV) >= 90
    for row in F8_CASES:
        assert (row in FP8) == (None not in row[0]), row
    assert len(FP8) >= 30
    assert all(None not in r[2] for r in ROUTES) and len(ROUTES) >= 136
    assert {r[0] for r in ROUTES} == {"fwd", "s2pair", "dgrad", "dgrad_t", "dgrad_parity", "scatter", "wgrad"}
    assert len(_own_params(T.test_stem_f64)) == 16 and len(_own_params(T.test_stem_conv_pool_f64)) == 10
    assert _own_params(T.test_optimizer_step_f64) == [{"kind": "adam"}, {"kind": "sgd"}]
    assert A.FILLS == (0xFF, 0x7F) and A.GUARD == 128 * 1024


@fills
@pytest.mark.parametrize("row", ROUTES, ids=[f"{r[0]}-{r[1]}-{'x'.join(map(str, r[2]))}-{r[3].replace(' ', '+')}" for r in ROUTES])
def test_conv_route_in_arena(row, fill, monkeypatch):
    run_in_arena(fill, monkeypatch, T.test_conv_route_f64, row)


@fills
@pytest.mark.parametrize("row", NONCONV, ids=[T._nc_id(r) for r in NONCONV])
def test_nonconv_in_arena(row, fill, monkeypatch):
    run_in_arena(fill, monkeypatch, BODIES[row[0]], row)


@fills
@pytest.mark.parametrize("kw", _own_params(T.test_stem_f64), ids=_kw_id)
def test_stem_in_arena(kw, fill, monkeypatch):
    run_in_arena(fill, monkeypatch, T.test_stem_f64, **kw)


@fills
@pytest.mark.parametrize("kw", _own_params(T.test_stem_conv_pool_f64), ids=_kw_id)
def test_stem_conv_pool_in_arena(kw, fill, monkeypatch):
    run_in_arena(fill, monkeypatch, T.test_stem_conv_pool_f64, **kw)


@fills
@pytest.mark.parametrize("kind", ["adam", "sgd"])
def test_optimizer_step_in_arena(kind, fill, monkeypatch):
    a = run_in_arena(fill, monkeypatch, T.test_optimizer_step_f64, kind)
    assert a.launches >= 2          # the step itself and the pack of the updated parameter


@fills
@pytest.mark.parametrize("row", FP8, ids=[F8T._f8_id(r) for r in FP8])
def test_conv_fp8_in_arena(row, fill, monkeypatch):
    run_in_arena(fill, monkeypatch, F8T.test_conv_fp8_f64, row)
