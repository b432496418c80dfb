"""The kernels and kernel / shape combinations that only an SSLCR_* switch reaches (tests/switch_routes.py), against float64.  The
library reads each of these switches once per process, so every test starts ONE fresh child process with the switch in its environment; the
child runs the existing float64 bodies of tests/test_kernels_gpu.py on the switch's rows (the derived per-element bounds of
tests/_f64.py: no tolerance of its own here), catches AssertionError per row and leaves {row: "ok" | message} in a file.  This
process never opens the device: a test's child is the only process on it.  A child that ends by a signal, aborts, or runs out of
time fails its test and every later test of the file at once, without another process being started."""
import json
import os
import subprocess
import sys

import pytest

import nonconv_cases as NC
import switch_routes as SR
from kernel_routes import ROUTES

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FAULTED = []          # the first child that faulted or hung: nothing more goes onto the device from this file


def row_id(r):
    return f"{r[0]}-{r[1]}-{'x'.join(map(str, r[2]))}-{r[3].replace(' ', '+')}"


# ---------------------------------------------------------------- the child's side
def _attempt(results, out, key, fn, *args):
    """one row: an AssertionError is the row's result; anything else (a HIP error above all) ends the child"""
    try:
        fn(*args)
        results[key] = "ok"
    except AssertionError as e:
        results[key] = f"AssertionError: {e}"[:4000]
    with open(out, "w") as f:
        json.dump(results, f)


def _refused(T, row):
    """a REFUSED row: the router names the instance, sslcr_conv2d returns an error and writes nothing"""
    import torch
    from ssl_cr_histo_amd import _lib as L
    K = T._k()
    op, dt, (N, H, W, C, Ko, R, stride, pad), _, name, _ = row
    assert op == "dgrad"
    OH, OW = (H + 2 * pad - R) // stride + 1, (W + 2 * pad - R) // stride + 1
    dy, w = T.q(T.rnd(514, (N, OH, OW, Ko)), dt), T.q(T.rnd(513, (Ko, R, R, C), 0.05), dt)
    dx = torch.full((N, H, W, C), float("nan"), dtype=K.tdtype(dt), device=T.DEV)
    with pytest.raises(L.SslcrError):
        K.conv2d(T.to_dev(dy, dt), T.to_dev(w.permute(3, 1, 2, 0).contiguous(), dt), stride, pad, transposed=True, out=dx, out_hw=(H, W),
                 pixel_hw=(OH, OW), pix_mul=2, par4=True)
    assert K.last_conv_kernel == name, K.last_conv_kernel
    torch.cuda.synchronize()
    assert bool(torch.isnan(dx.float()).all()), "the refused launch wrote to its output"


def _stem_pool_form(T, shape, split, in_u8):
    T.test_stem_wgrad_from_pooled_gradient(shape, split, in_u8, 1)
    name = T._k().last_stem_wgrad_kernel
    assert name.startswith("sslcr::stem_wgrad_kernel<unsigned short, ") and "pool2" not in name, name


def child(switch, out):
    """every row of `switch` (set in this process' environment by the parent) -> {row id: "ok" | message} in the file `out`"""
    import test_kernels_gpu as T
    value = {**SR.ROUTING, **SR.FORMS}[switch]
    assert os.environ[switch] == value
    # ... and the library saw it: the row is set, to the value the parent gave (a misspelt name would leave the default in place)
    seen = T._k().switches()[switch]
    assert seen["set"] is True and seen["value"] == int(value), (switch, seen)
    results = {}
    if switch in SR.ROUTING:
        for row in SR.SWITCH_ROUTES[switch] + SR.LARGER_ROUTES.get(switch, []):
            if row in SR.REFUSED:
                _attempt(results, out, row_id(row), _refused, T, row)
            else:
                _attempt(results, out, row_id(row), T.test_conv_route_f64, row)
    for row in FORM_ROWS.get(switch, ()):
        kind = row[0]
        if kind in ("linear", "pool", "many_rows", "stem"):
            print(f"\n[row] {form_id(row)}")       # (test_conv_route_f64 heads its [f64] lines itself)
        if kind == "linear":
            _attempt(results, out, form_id(row), T.test_linear_f64, row)
        elif kind == "pool":
            _attempt(results, out, form_id(row), T.test_pool_f64, row)
        elif kind == "many_rows":
            _attempt(results, out, form_id(row), T.test_bn_relu_maxpool_many_rows, row[1])
        elif kind == "stem":
            _attempt(results, out, form_id(row), _stem_pool_form, T, *row[1:])
        else:
            _attempt(results, out, form_id(row), T.test_conv_route_f64, row)


# ---------------------------------------------------------------- the parent's side
def run_child(code, env, what):
    """one fresh child process -> its CompletedProcess; a fault or a hang fails the test and closes the file"""
    if FAULTED:
        pytest.fail(f"not started: {FAULTED[0]}")
    code = f"import sys; sys.path[:0] = [{ROOT!r}, {HERE!r}]\n" + code
    try:
        r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                           timeout=300)
    except subprocess.TimeoutExpired as e:
        FAULTED.append(f"the child of {what} did not end within 300 s")
        tail = e.stdout[-3000:] if isinstance(e.stdout, str) else (e.stdout or b"")[-3000:].decode(errors="replace")
        pytest.fail(f"{FAULTED[0]}\n{tail}")
    if r.returncode < 0 or r.returncode in (134, 139) or "illegal memory access" in r.stdout:
        FAULTED.append(f"the child of {what} ended with status {r.returncode}")
        pytest.fail(f"{FAULTED[0]}\n{r.stdout[-3000:]}")
    return r


def rows_ok(switch, value, tmp_path, want):
    out = tmp_path / "rows.json"
    r = run_child(f"import test_switch_routes_gpu as S\nS.child({switch!r}, {str(out)!r})\n", {switch: value}, f"{switch}={value}")
    print(f"\n[switch] {switch}={value}")
    print("\n".join(l for l in r.stdout.splitlines() if l.startswith(("[row]", "[f64]"))))
    results = json.loads(out.read_text()) if out.exists() else {}
    assert r.returncode == 0, f"after {len(results)} of {len(want)} rows:\n{r.stdout[-3000:]}"
    assert list(results) == want
    bad = {k: v for k, v in results.items() if v != "ok"}
    assert not bad, "\n".join(f"{k}: {v}" for k, v in bad.items())


@pytest.mark.parametrize("switch", list(SR.ROUTING))
def test_switch_route_f64(switch, tmp_path):
    """every row behind a routing switch: the launch is exactly the instance the switched router names, and y, the BatchNorm partial
    statistics and dW hold the float64 per-element bounds (test_kernels_gpu.test_conv_route_f64); a REFUSED row is refused"""
    rows_ok(switch, SR.ROUTING[switch], tmp_path, [row_id(r) for r in SR.SWITCH_ROUTES[switch] + SR.LARGER_ROUTES.get(switch, [])])


def _first_row_of(name):
    return next(r for r in ROUTES if r[4] == name)


FORM_ROWS = {
    # the direct-fetch GEMM on the two shapes that take the LDS form by default
    "SSLCR_GEMM_LDS": [r for r in NC.GEMM if r[2] in ((96, 1024, 512), (32, 64, 32))],
    # pool_row_range's banded branch is taken only where gridDim.x % 8 == 0, and launch_bn_relu_maxpool's row form launches
    # min(N * OH, 4096) workgroups: of the row-form rows (N = 3) the 16x16 maps launch 3 * 8 = 24 workgroups, one row each in eight
    # bands of three (the 1x1, 2x2 and 9x7 maps launch 3, 3 and 15 and keep the interleaved walk); many_rows launches 4096
    # workgroups for 130 * 32 = 4160 rows -- 512 per band, some of them walking two rows -- in both dtypes, and the plain form of
    # maxpool_rows_kernel beside bn_relu_maxpool_rows_kernel
    "SSLCR_POOL_BANDS": [r for r in NC.POOL if r[2][3] in (64, 512) and not r[3]] + [("many_rows", 0), ("many_rows", 1)],
    # the single-role stem_wgrad_kernel<unsigned short, INF32, POOL = true>: bf16 runs the role-split stem_wgrad_pool2_kernel by default
    "SSLCR_STEM_POOL_FORM": [("stem", shape, split, in_u8) for shape, split in (((3, 64, 64), 0), ((2, 56, 40), 0), ((5, 30, 34), 2),
                                                                                 ((1, 256, 256), 0), ((40, 64, 64), 16))
                             for in_u8 in (True, False)],
    # the unstaggered fold behind wgrad3x3_dma_kernel: one row per <TW, XF>
    "SSLCR_WG_STAGGER": [_first_row_of(f"sslcr::wgrad3x3_dma_kernel<{tw}, {xf}>") for tw in (16, 8) for xf in ("true", "false")],
}


def form_id(r):
    if r[0] in ("linear", "pool"):        # (as test_kernels_gpu._nc_id spells a row of tests/nonconv_cases.py)
        op, dt, shape, flags, _ = r
        return f"{op}{ {None: '', 0: '-f32', 1: '-bf16'}[dt]}-{'x'.join(map(str, shape))}" + ("-" + flags.replace(" ", "+") if flags else "")
    if r[0] == "many_rows":
        return f"many_rows-{r[1]}"
    if r[0] == "stem":
        return f"stem-{'x'.join(map(str, r[1]))}-split{r[2]}-{'u8' if r[3] else 'f32'}"
    return row_id(r)


@pytest.mark.parametrize("switch", list(SR.FORMS))
def test_switch_form_f64(switch, tmp_path):
    """the kernel forms behind the switches that change no routed name, through the bodies that bound them by default"""
    assert FORM_ROWS[switch]
    rows_ok(switch, SR.FORMS[switch], tmp_path, [form_id(r) for r in FORM_ROWS[switch]])


# ---------------------------------------------------------------- the engine's switches
# The smallest step at which layer2.0 takes the paired BatchNorm backward with the mask as bits: bn_bwd_pair_ok has no size condition
# (one pass: nseg <= 1, equal C and pixels), ybits_of asks that every block's N * h * w * C bits fill whole 128-byte lines (a multiple
# of 1024 elements); at 64 x 64 input layer4's 2 x 2 x 512 map does for every N.  N = 2, so that no BatchNorm sees a single image.
STEP = ("bf16", 2, 64)
PAIR = "sslcr::bn_bwd_apply_pair_kernel<unsigned short>"
ENGINE_RUNS = {"default": {}, "ybits0": {"SSLCR_YBITS": "0"}, "g0": {"SSLCR_BN_PAIR_G": "0"}, "ybits0_g0": {"SSLCR_YBITS": "0", "SSLCR_BN_PAIR_G": "0"}}


def test_engine_switches_leave_every_gradient_bit(tmp_path):
    """one bf16 supervised step with SSLCR_YBITS=0 (bn2's reduce pass reads the saved output, not its sign bits), with SSLCR_BN_PAIR_G=0
    (the paired reduce writes no g: the apply pass forms it again from dOut and the bits), with both and with neither, one child after the
    other.  The mask is y > 0 either way and g is the same product of the same operands, so every gradient has the default's bits.
    What shows that a form was taken: the profile books the paired apply pass with 5 tensor passes where it reads g and with 5.0625
    where it reads dOut and the bits (keep_g = 0), so the g0 run's bytes are 1.0125 of the default's; with SSLCR_YBITS=0 beside it there
    are no bits, the engine keeps g, and the bytes are the default's again -- which is how SSLCR_YBITS=0 is seen to be read.  The run
    with SSLCR_YBITS=0 alone books what the default books: nothing the step reports tells it from the default."""
    import torch
    dtype, n, hw = STEP
    runs = {}
    for key, env in ENGINE_RUNS.items():
        path = tmp_path / f"{key}.pt"
        r = run_child(f"import test_engine_gpu2 as T\nT._supervised_step_gradients({dtype!r}, {n}, {str(path)!r}, hw={hw})\n", env, f"the step with {env}")
        assert r.returncode == 0, (key, r.stdout[-3000:])
        runs[key] = torch.load(path)
    base = runs["default"]
    assert PAIR in base["kernels"] and len(base["grads"]) >= 62
    assert all(bool(torch.isfinite(g).all()) for g in base["grads"]) and float(base["grads"][0].abs().max()) > 0
    for key, run in runs.items():
        want = 1.0125 if key == "g0" else 1.0
        got = run["bytes"][PAIR] / base["bytes"][PAIR]
        print(f"[{key}] bytes booked for the paired apply pass / the default's: {got:.6f}")
        assert abs(got - want) < 1e-5, (key, got)
        differ = [i for i, (a, b) in enumerate(zip(run["grads"], base["grads"])) if not torch.equal(a, b)]
        assert len(run["grads"]) == len(base["grads"]) and not differ, (key, differ)
