"""CPU-only: the route table (tests/kernel_routes.py) against the library's routing -- each row's descriptor maps to exactly its
kernel name -- and against the step's profiles: every conv / stride-2 / stride-2 dgrad / wgrad instance that a profiled step
launched has a row; and against everything the router can answer: every instance named over the grid of tools/route_sweep.py has a
row, and the family whose name elides its tile arguments a row per form.  (No device here: device_cus() falls back to 256, the MI355X's count, which the routing of the persistent
kernels depends on.)"""
import csv
import os
import re

import pytest

from kernel_routes import ROUTES
from switch_routes import ROUTING

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the routing caches these A/B switches in statics: a set one would route (and pass) a different table.  Every routing switch of
# tests/switch_routes.py (the routes behind them have a table and a walk of their own: tests/test_switch_routes_cpu.py)
SWITCHES = tuple(ROUTING) + ("SSLCR_BN_ONE_LAUNCH",)
FAKE = 4096        # a non-NULL pointer for the descriptor fields that select a route (nothing is launched)


@pytest.fixture(scope="module")
def lib():
    set_ = [k for k in SWITCHES if k in os.environ]
    assert not set_, f"unset {set_}: the kernel routing reads them once into statics, so this table would not be what runs"
    from ssl_cr_histo_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    return _lib.lib()


def flags_of(spec):
    f = {}
    for t in spec.split():
        k, _, v = t.partition("=")
        f[k] = int(v) if v else True
    return f


def conv_desc(op, shape, spec, par=None):
    from ssl_cr_histo_amd import _lib as L
    N, H, W, C, K, R, stride, pad = shape
    f = flags_of(spec)
    p = lambda k: FAKE if f.get(k) else None      # noqa: E731
    PH, PW = (H + 2 * pad - R) // stride + 1, (W + 2 * pad - R) // stride + 1
    if op == "dgrad":      # x = dY [N, PH, PW, K], w = [C][R][S][K], pixel space = the input's four parity planes
        d = L.ConvDesc(FAKE, FAKE, FAKE, None, None, None, None, None, N, PH, PW, K, C, R, R, stride, pad, PH, PW, H, W, 1, 1, 0, 0, 0, 2,
                       0, 0, 0)
        d.par4 = 1
        return d
    if op == "dgrad_t":    # the transposed plain form: pixel space = the conv's input, with a residual
        return L.ConvDesc(FAKE, FAKE, FAKE, None, None, None, FAKE, None, N, PH, PW, K, C, R, R, stride, pad, H, W, H, W, 1, 1, 0, 0, 0, 0,
                          0, 0, 0)
    if op == "dgrad_parity":       # one input-pixel parity class: par = (ph, pw, tap_mask, taps) of _f64.parity_classes()
        ph, pw, tap_mask, _ = par
        return L.ConvDesc(FAKE, FAKE, FAKE, None, None, None, FAKE, None, N, PH, PW, K, C, R, R, stride, pad, (H - ph + 1) // 2,
                          (W - pw + 1) // 2, H, W, 1, 1, 0, 0, 0, 2, ph, pw, tap_mask)
    if op == "scatter":    # the 1x1 / 2 input gradient: a plain 1x1 conv of dY, scattered to the even positions and accumulated
        return L.ConvDesc(FAKE, FAKE, FAKE, None, None, None, None, None, N, PH, PW, K, C, 1, 1, 1, 0, PH, PW, H, W, 2, 0, 0, 0, 1, 0,
                          0, 0, 0)
    d = L.ConvDesc(FAKE, FAKE, FAKE, p("in_scale"), p("in_scale"), p("bias"), p("residual"), p("stats"), N, H, W, C, K, R, R, stride,
                   pad, PH, PW, PH, PW, 1, 0, int(bool(f.get("in_scale"))), int(bool(f.get("relu"))), 0, 0, 0, 0, 0)
    d.out_scale = p("out_scale")
    if f.get("mask"):
        d.mask_x = d.mask_scale = d.mask_shift = d.mask_mean = FAKE
    if f.get("seg"):
        d.seg_images, d.seg_stride = f["seg"], C
    return d


def wgrad_desc(shape, spec):
    from ssl_cr_histo_amd import _lib as L
    N, H, W, C, K, R, stride, pad = shape
    f = flags_of(spec)
    OH, OW = (H + 2 * pad - R) // stride + 1, (W + 2 * pad - R) // stride + 1
    xf = FAKE if f.get("in_scale") else None
    return L.WgradDesc(FAKE, FAKE, FAKE, xf, xf, int(bool(xf)), N, H, W, C, K, R, R, stride, pad, OH, OW, f.get("seg", 0),
                       C if f.get("seg") else 0)


@pytest.mark.parametrize("row", ROUTES, ids=[f"{r[0]}-{r[1]}-{'x'.join(map(str, r[2]))}-{r[3].replace(' ', '+')}" for r in ROUTES])
def test_route_maps_to_exactly_its_kernel(lib, row):
    op, dt, shape, spec, name, tail = row
    if op == "wgrad":
        assert lib.sslcr_conv2d_wgrad_kernel_name(dt, wgrad_desc(shape, spec)).decode() == name
        return
    if op == "s2pair":
        N, H, W, C, K, R, stride, pad = shape
        d3 = conv_desc("fwd", shape, spec)
        d1 = conv_desc("fwd", (N, H, W, C, K, 1, 2, 0), spec.replace("relu", ""))
        assert lib.sslcr_conv2d_s2_pair_ok(dt, d3, d1) == 1
        single = lib.sslcr_conv2d_kernel_name(dt, d3).decode()
        # conv_s2_name(a, pair): the pair launches the same EVAL instance with PAIR = true
        assert single.startswith("sslcr::conv_s2_kernel<false, ") and single.replace("<false, ", "<true, ") == name, single
        return
    if op == "dgrad_parity":       # four launches, one per class: every one is the row's instance
        import _f64 as B
        for par in B.parity_classes():
            assert lib.sslcr_conv2d_kernel_name(dt, conv_desc(op, shape, spec, par)).decode() == name, par
        return
    d = conv_desc(op, shape, spec)
    assert lib.sslcr_conv2d_kernel_name(dt, d).decode() == name
    if flags_of(spec).get("seg"):
        assert lib.sslcr_conv2d_segments_ok(dt, d) == 1


def _table_names():
    from fp8_cases import CASES as FP8_CASES       # the fp8 instances have their own table (tests/test_fp8_cpu.py maps its rows)
    return {r[4] for r in ROUTES} | {r[5] for r in ROUTES if r[5]} | {r[3] for r in FP8_CASES}


def _is_route(name):
    # conv / stride-2 / stride-2 dgrad / wgrad instances; wgrad_fold_kernel is the ordered fold of the wgrad slabs, launched behind
    # a wgrad instance (no descriptor routes to it)
    return re.match(r"sslcr::(conv|wgrad)", name) and "wgrad_fold" not in name


def test_every_profiled_instance_has_a_row():
    with open(os.path.join(ROOT, "profiles", "r06_final_kernel_stats.csv")) as f:
        names = [row["Name"] for row in csv.DictReader(f)]
    insts = {re.sub(r"^void ", "", n).split("(")[0] for n in names}
    insts = {n for n in insts if _is_route(n)}
    assert len(insts) >= 25
    missing = sorted(insts - _table_names())
    assert not missing, f"profiled instances without a route row: {missing}"


def test_every_truncated_profile_name_has_a_row():
    """profiles/r06_final_rsp_kstats.txt prints the names cut off: match them by prefix"""
    table = _table_names()
    found = 0
    with open(os.path.join(ROOT, "profiles", "r06_final_rsp_kstats.txt")) as f:
        for line in f:
            m = re.search(r"(sslcr::\S.*)$", line.rstrip())
            if not m or not _is_route(m.group(1)):
                continue
            prefix = m.group(1).split("(")[0]
            found += 1
            assert any(t.startswith(prefix) for t in table), f"no route row starts with {prefix!r}"
    assert found >= 15


@pytest.fixture(scope="module")
def swept(lib):
    """tools/route_sweep.py's whole grid (nothing is launched) -> {"conv" | "wgrad": {name: (size, tag, dtype) of the smallest descriptor
    that the router answers with this name}}"""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import route_sweep
    finally:
        sys.path.remove(os.path.join(ROOT, "tools"))
    found = {"conv": {}, "wgrad": {}}
    for kind, tag, d, _, size in route_sweep.walk():
        fn, names = (lib.sslcr_conv2d_wgrad_kernel_name, found["wgrad"]) if kind == "wgrad" else (lib.sslcr_conv2d_kernel_name, found["conv"])
        for dt in (0, 1):
            name = fn(dt, d).decode()
            if name not in names or size < names[name][0]:
                names[name] = (size, tag, dt)
    return found


def _unreachable_by_name(name):
    # the PAIR = true instances: sslcr_conv2d_s2_pair launches them; the name query answers for the single conv (PAIR = false).
    # BEYOND_THE_GRID: named only by flag sets the grid does not hold (test_route_maps_to_exactly_its_kernel pins their rows)
    from kernel_routes import BEYOND_THE_GRID
    return name.startswith("sslcr::conv_s2_kernel<true, ") or name in BEYOND_THE_GRID


def missing_rows(swept, routes, unlaunchable):
    """-> the failure lines of the closure: every swept name without a row (with the smallest descriptor that reaches it), and every
    row name that the grid should reach and does not"""
    conv_rows = {r[4] for r in routes if r[0] != "wgrad"} | {r[5] for r in routes if r[5]}
    wgrad_rows = {r[4] for r in routes if r[0] == "wgrad"}
    lines = []
    for kind, rows in (("conv", conv_rows), ("wgrad", wgrad_rows)):
        for name, (_, tag, dt) in sorted(swept[kind].items()):
            if name not in rows and name not in unlaunchable:
                lines.append(f"no route row for {name}: smallest descriptor {tag} dt={dt}")
        # (the tail column holds second launches: some of them no descriptor names)
        for name in sorted({r[4] for r in routes if (r[0] == "wgrad") == (kind == "wgrad")} - set(swept[kind])):
            if not _unreachable_by_name(name):
                lines.append(f"the route row's {kind} name {name} is answered for no descriptor of the grid")
    return lines


def test_every_routable_instance_has_a_row(swept):
    """every conv and wgrad instance that the router can answer over the sweep's grid has a row (or stands in UNLAUNCHABLE with the
    condition that refuses it), and every row names an instance that the router answers: the two sets are equal, whatever their size"""
    from kernel_routes import UNLAUNCHABLE
    lines = missing_rows(swept, ROUTES, UNLAUNCHABLE)
    assert not lines, "\n".join(lines)
    assert {r[4] for r in ROUTES} <= _table_names()
    from kernel_routes import BEYOND_THE_GRID
    assert not set(BEYOND_THE_GRID) & (set(swept["conv"]) | set(swept["wgrad"])), "BEYOND_THE_GRID names an instance the grid reaches"
    assert set(BEYOND_THE_GRID) <= {r[4] for r in ROUTES}
    stale = sorted(set(UNLAUNCHABLE) - set(swept["conv"]) - set(swept["wgrad"]))
    assert not stale, f"UNLAUNCHABLE names an instance the router no longer answers: {stale}"


def test_a_deleted_row_fails_the_closure_with_its_instance(swept):
    """the closure notices a missing row: without the rows of one instance it names that instance and a descriptor for it"""
    for victim in ("sslcr::conv3x3_halo256_kernel<unsigned short, 8, 64, 1, true>", "sslcr::wgrad_kernel<unsigned short, 9, 1>",
                   "sslcr::conv_igemm_kernel<float, 128, 128>"):
        lines = missing_rows(swept, [r for r in ROUTES if victim not in (r[4], r[5])], {})
        assert len(lines) == 1 and lines[0].startswith(f"no route row for {victim}: smallest descriptor "), lines


def halo_form(shape):
    """the (TW, BKO) instance of conv3x3_halo_kernel behind the elided name: conv_halo_tw's `a.W % 16 == 0 -> 16, else 8` and
    halo_pick's `a.K % 128 == 0 -> 128, else 64`"""
    W, K = shape[2], shape[4]
    return (16 if W % 16 == 0 else 8, 128 if K % 128 == 0 else 64)


def test_every_form_of_the_halo_family_has_a_row():
    for dt, t in ((0, "float"), (1, "unsigned short")):
        forms = {halo_form(r[2]) for r in ROUTES if r[0] == "fwd" and r[1] == dt and r[4] == f"sslcr::conv3x3_halo_kernel<{t}, ...>"}
        assert forms == {(16, 128), (16, 64), (8, 128), (8, 64)}, (t, sorted(forms))


@pytest.mark.parametrize("shape, seg", [((1, 16, 16, 64, 64, 3, 1, 1), 2), ((1, 16, 16, 128, 128, 3, 1, 1), 2), ((4, 8, 8, 512, 512, 3, 1, 1), 8)],
                         ids=["pp64", "h16", "h16-4img"])
def test_segment_larger_than_the_batch_has_no_rows(lib, shape, seg):
    """seg_images > N on the kernels whose grid is split among the segments (N / seg_images = 0 groups): no rows and no segment form --
    the grid arithmetic behind sslcr_conv2d_partial_rows used to divide by that zero"""
    d = conv_desc("fwd", shape, f"stats seg={seg}")
    assert lib.sslcr_conv2d_partial_rows(d) == -1
    assert lib.sslcr_conv2d_segments_ok(1, d) == 0


# ---------------------------------------------------------------- the forms of the engine step (tests/step_forms.py)
@pytest.fixture(scope="module")
def step_forms(lib):
    import step_forms as SF
    return SF, {k: SF.expected_forms(lib, k) for k in SF.ROWS}


def test_step_replay_rows_take_the_forms_they_were_chosen_for(step_forms):
    """the form word the engine must report per (row, block) of the float64 step replay (tests/test_backward_replay_gpu.py asserts the
    tap's flags equal it): each row still takes the forms it stands for"""
    SF, table = step_forms
    for key, bit, on in SF.STATED:
        got = [i for i, w in enumerate(table[key]) if w & bit]
        assert got == list(on), f"row {key}: {SF.word_str(bit)} is on in blocks {got}, the row was chosen for {list(on)}"


def test_every_form_bit_is_on_somewhere_and_off_elsewhere(step_forms):
    """set closure: a form that no (row, block) takes, or that every one takes, is a form the replay cannot tell from its sibling"""
    SF, table = step_forms
    assert SF.closure_gaps(table) == []
    # ... and the check itself notices: without row A nothing runs the forward as segments
    assert SF.closure_gaps({k: v for k, v in table.items() if k != "A"}) == ["fwd_seg"]
