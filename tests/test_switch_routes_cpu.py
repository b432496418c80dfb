"""CPU-only: the routes behind the library's A/B switches (tests/switch_routes.py).  The routing switches are read once per
process, so every switch is walked in a fresh child process with the variable in its environment: one walk of tools/route_sweep.py's
grid per routing switch, all started side by side, and one walk of the default routing in this process.  The closure: every distinct
(default instance -> switched instance) transition of every switch has a row in SWITCH_ROUTES whose descriptor makes exactly that
transition, and every row makes a transition the sweep shows.  The inventory: every row of the library's switch table
(kernels.switches()) is classified, and no file of csrc/ but the table's reads the environment."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import switch_routes as SR
from test_kernel_routes_cpu import conv_desc, wgrad_desc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TOOLS = os.path.join(ROOT, "tools")


def row_id(r):
    return f"{r[0]}-{r[1]}-{'x'.join(map(str, r[2]))}-{r[3].replace(' ', '+')}"


def row_tag(r):
    """the row's descriptor as tools/route_sweep.py's walk() tags it (its seg field: 0 where the row has none), or None where the row's
    op is not one the grid holds"""
    op, _, (N, H, W, C, K, R, s, pad), spec = r[:4]
    shape = f"{N}x{H}x{W} {C}->{K} k{R}s{s}p{pad}"
    toks = spec.split()
    seg = next((int(t[4:]) for t in toks if t.startswith("seg=")), 0)
    flags = " ".join(t for t in toks if not t.startswith("seg="))
    if op == "fwd":
        return f"conv {shape} [{flags}] seg={seg}"
    if op == "dgrad":
        return f"dgrad {shape} par4"
    if op == "wgrad":
        return f"wgrad {shape} xf={int('in_scale' in toks)} seg={seg}"
    return None


def all_rows(switch):
    return SR.SWITCH_ROUTES[switch] + SR.LARGER_ROUTES.get(switch, [])


def answer(lib, row):
    """what the router of this process answers for a row of the table"""
    op, dt, shape, spec = row[:4]
    if op == "wgrad":
        return lib.sslcr_conv2d_wgrad_kernel_name(dt, wgrad_desc(shape, spec)).decode()
    return lib.sslcr_conv2d_kernel_name(dt, conv_desc(op, shape, spec)).decode()


def walk_names(lib):
    """the whole grid, in walk()'s order, each descriptor for dtype 0 then 1 -> (the distinct names, an index into them per answer)"""
    if TOOLS not in sys.path:
        sys.path.insert(0, TOOLS)
    import route_sweep
    names, idx = {}, []
    for kind, _, d, _, _ in route_sweep.walk():
        fn = lib.sslcr_conv2d_wgrad_kernel_name if kind == "wgrad" else lib.sslcr_conv2d_kernel_name
        for dt in (0, 1):
            idx.append(names.setdefault(fn(dt, d).decode(), len(names)))
    return list(names), np.asarray(idx, dtype=np.int16)


def child_main(switch, out):
    """in the child (the switch is in its environment): the walk, and the answers for the switch's rows"""
    from ssl_cr_histo_amd import _lib
    lib = _lib.lib()
    names, idx = walk_names(lib)
    np.save(out + ".npy", idx)
    with open(out + ".json", "w") as f:
        json.dump({"names": names, "rows": [answer(lib, r) for r in all_rows(switch)]}, f)


@pytest.fixture(scope="module")
def walks(tmp_path_factory):
    """-> (tags, sizes, default, {switch: (names, row names)}, {switch: default row names}): tag (with its dtype), size and the default
    routing's name per answer of the grid; per switch the child's name per answer and per row of the switch, and this process' name
    per row"""
    set_ = sorted(k for k in os.environ if k.startswith("SSLCR_"))
    assert not set_, f"unset {set_}: the default walk of this process would not be the default routing"
    from ssl_cr_histo_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    tmp = tmp_path_factory.mktemp("switch_walks")
    procs = {}
    for sw, off in SR.ROUTING.items():
        code = (f"import sys; sys.path[:0] = [{ROOT!r}, {HERE!r}]\n"
                f"import test_switch_routes_cpu as T\nT.child_main({sw!r}, {str(tmp / sw)!r})\n")
        procs[sw] = subprocess.Popen([sys.executable, "-c", code], env=dict(os.environ, **{sw: off}), stdout=subprocess.PIPE,
                                     stderr=subprocess.STDOUT, text=True)
    lib = _lib.lib()
    names, idx = walk_names(lib)
    default = np.asarray(names, dtype=object)[idx]
    import route_sweep
    tags, sizes = [], []
    for _, tag, _, _, size in route_sweep.walk():
        for dt in (0, 1):
            tags.append(f"{tag} dt={dt}")
            sizes.append(size)
    switched = {}
    for sw, p in procs.items():
        out, _ = p.communicate(timeout=900)
        assert p.returncode == 0, f"{sw}: {out[-3000:]}"
        with open(str(tmp / sw) + ".json") as f:
            j = json.load(f)
        switched[sw] = (np.asarray(j["names"], dtype=object)[np.load(str(tmp / sw) + ".npy")], j["rows"])
        assert len(switched[sw][0]) == len(default)
    return tags, sizes, default, switched, {sw: [answer(lib, r) for r in all_rows(sw)] for sw in SR.ROUTING}


def transitions(tags, sizes, default, names):
    """{(default name, switched name): {tag of each answer that makes the transition}} and the smallest such tag per transition"""
    changed = np.nonzero(default != names)[0]
    sets, smallest = {}, {}
    for i in changed:
        k = (default[i], names[i])
        sets.setdefault(k, set()).add(tags[i])
        if k not in smallest or sizes[i] < smallest[k][0]:
            smallest[k] = (sizes[i], tags[i])
    return sets, {k: v[1] for k, v in smallest.items()}


def flag_sets(tags):
    return {re.search(r"\[(.*)\]", t).group(1) for t in tags if t.startswith("conv ")}


def row_faults(switch, rows, row_default, row_switched, sets):
    """-> (a failure line per row that names another instance than the switched router answers, that the switch does not move, or whose
    descriptor makes no transition of the sweep; {transition: the tags of the rows that make it})"""
    lines = []
    have = {}
    for r, d, s in zip(rows, row_default, row_switched):
        tag = row_tag(r)
        tag = tag and f"{tag} dt={r[1]}"
        if s != r[4]:
            lines.append(f"{switch}: the row {row_id(r)} names {r[4]}, the router answers {s}")
        elif d == s:
            lines.append(f"{switch}: the row {row_id(r)} is served by {s} with and without the switch: it tests nothing")
        elif tag not in sets.get((d, s), ()):
            lines.append(f"{switch}: the sweep does not show the row {row_id(r)} going {d} -> {s}")
        else:
            have.setdefault((d, s), set()).add(tag)
    return lines, have


def closure_gaps(switch, rows, row_default, row_switched, sets, smallest):
    """the failure lines of one switch's closure: the rows' own faults, a transition of the sweep without a row (with the smallest
    descriptor that makes it), and for the instances that exist behind a switch alone a flag set without a row"""
    lines, have = row_faults(switch, rows, row_default, row_switched, sets)
    for (d, s), tags in sorted(sets.items()):
        if (d, s) not in have:
            lines.append(f"{switch}: no row for the transition {d} -> {s}: smallest descriptor {smallest[(d, s)]}")
        elif s in SR.ONLY_BEHIND_A_SWITCH:
            for fl in sorted(flag_sets(tags) - flag_sets(have[(d, s)])):
                lines.append(f"{switch}: no row for the transition {d} -> {s} with the flags [{fl}]")
    return lines


@pytest.fixture(scope="module")
def closure(walks):
    tags, sizes, default, switched, row_defaults = walks
    out = {}
    for sw in SR.ROUTING:
        names, row_names = switched[sw]
        out[sw] = (row_defaults[sw], row_names) + transitions(tags, sizes, default, names)
    return out


def test_the_tables_name_the_same_switches():
    assert set(SR.SWITCH_ROUTES) == set(SR.ROUTING) and set(SR.LARGER_ROUTES) <= set(SR.ROUTING)
    every = [r for sw in SR.ROUTING for r in all_rows(sw)]
    assert set(SR.REFUSED) <= set(every)
    groups = (SR.ROUTING, SR.FORMS, SR.ENGINE, SR.COVERED_ELSEWHERE, SR.OUT_OF_SCOPE)
    assert sum(len(g) for g in groups) == len(set().union(*groups)), "a switch stands in two groups"


@pytest.mark.parametrize("switch", list(SR.ROUTING))
def test_every_transition_behind_a_switch_has_a_row(closure, switch):
    """set equality, both ways: every (default -> switched) pair among the changed answers of the grid has a row making exactly that
    transition; every row names what the switched router answers, differs from its default, and makes a transition the sweep shows"""
    row_default, row_switched, sets, smallest = closure[switch]
    assert sets, f"{switch}={SR.ROUTING[switch]} changes no answer of the grid"
    n = len(SR.SWITCH_ROUTES[switch])
    lines = closure_gaps(switch, SR.SWITCH_ROUTES[switch], row_default[:n], row_switched[:n], sets, smallest)
    # the larger descriptors beside the table: they count for no transition, and each makes one
    lines += row_faults(switch, SR.LARGER_ROUTES.get(switch, []), row_default[n:], row_switched[n:], sets)[0]
    assert not lines, "\n".join(lines)


def test_only_behind_a_switch_is_what_the_walks_say(walks):
    """ONLY_BEHIND_A_SWITCH: the instances some switch answers and the default routing answers for no descriptor of the grid"""
    _, _, default, switched, _ = walks
    from kernel_routes import ROUTES
    known = set(default) | {r[4] for r in ROUTES} | {r[5] for r in ROUTES if r[5]}
    found = set().union(*(set(names) for names, _ in switched.values())) - known
    assert found == set(SR.ONLY_BEHIND_A_SWITCH)


def test_a_deleted_row_fails_the_closure_and_names_the_transition(closure):
    """without any one row the closure names that row's transition and a descriptor (or, behind SSLCR_PP64=0, its flag set)"""
    for sw, rows in SR.SWITCH_ROUTES.items():
        row_default, row_switched, sets, smallest = closure[sw]
        for i, r in enumerate(rows):
            keep = [j for j in range(len(rows)) if j != i]
            lines = closure_gaps(sw, [rows[j] for j in keep], [row_default[j] for j in keep], [row_switched[j] for j in keep], sets, smallest)
            head = f"{sw}: no row for the transition {row_default[i]} -> {r[4]}"
            assert len(lines) == 1 and lines[0].startswith(head), (row_id(r), lines)
            assert lines[0].endswith(f"with the flags [{r[3]}]") or re.search(r": smallest descriptor (conv|dgrad|wgrad) \d+x\d+x\d+ ", lines[0]), lines


def getenv_files(csrc):
    """the files of csrc that read the environment: any getenv at all, a getenv("SSLCR_...") among them"""
    found = set()
    for name in sorted(os.listdir(csrc)):
        with open(os.path.join(csrc, name), errors="replace") as f:
            if re.search(r"\bgetenv\s*\(", f.read()):
                found.add(name)
    return found


def test_every_switch_the_library_reads_is_classified(tmp_path):
    """a new switch arrives with a test or with a stated reason for having none.  The inventory is the library's own table
    (kernels.switches()); the walk over the sources holds that the table's file is the only one of csrc/ that reads the environment,
    so that no switch exists beside the table"""
    from ssl_cr_histo_amd import kernels
    table = kernels.switches()
    classified = set(SR.ROUTING) | set(SR.FORMS) | set(SR.ENGINE) | set(SR.COVERED_ELSEWHERE) | set(SR.OUT_OF_SCOPE)
    assert set(table) == classified
    # each row's group is where tests/switch_routes.py files the switch
    by_group = {g: {sw for sw, row in table.items() if row["group"] == g} for g in ("routing", "form", "engine", "measurement")}
    assert sum(len(v) for v in by_group.values()) == len(table), "a row with a group of its own"
    assert by_group["routing"] == set(SR.ROUTING) and by_group["form"] == set(SR.FORMS)
    assert by_group["measurement"] == {"SSLCR_BN_REPEAT", "SSLCR_EW_CAP"} <= set(SR.OUT_OF_SCOPE)
    assert set(SR.ENGINE) | set(SR.COVERED_ELSEWHERE) <= by_group["engine"]
    csrc = os.path.join(ROOT, "ssl_cr_histo_amd", "csrc")
    assert getenv_files(csrc) == {"switches.cpp"}
    # ... and the scan itself notices one more
    (tmp_path / "new.hip").write_text('static const bool on = [] { const char* e = getenv("SSLCR_NEW"); return !e; }();\n')
    assert getenv_files(str(tmp_path)) == {"new.hip"}


def test_covered_elsewhere_names_tests_that_exist():
    for sw, where in SR.COVERED_ELSEWHERE.items():
        path, _, test = where.partition("::")
        with open(os.path.join(ROOT, path)) as f:
            text = f.read()
        assert re.search(rf"^def {test}\(", text, flags=re.M), where
        assert sw in text, f"{where} does not name {sw}"
