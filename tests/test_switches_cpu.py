"""CPU-only: the library's switch table (csrc/switches.cpp, listed by sslcr_switch_info / kernels.switches()) reads every string as
its rule says.  The `process` rows are parsed once per process, so every string gets ONE fresh child process with all 23 variables set
to it; the children load the library, ask for the listing and never open a device.  What each (rule, string) pair must give is the
literal table below: it restates what every switch did when each site parsed its own variable (atoi / first character / presence),
and profiles/switch_table_rules.txt holds the routing switches' side of it against that library."""
import json
import os
import re
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

STRINGS = [None, "", "0", "1", "2", "-1", "00", "01", " 0", "off", "0x1"]          # None: the variable is not set
# rule -> the value in use per string of STRINGS, in order ("d": the row's default)
EXPECT = {
    "ATOI":    ["d", 0, 0, 1, 1, 1, 0, 1, 0, 0, 0],          # atoi(e) != 0
    "LEAD0":   ["d", 1, 0, 1, 1, 1, 0, 0, 1, 1, 0],          # e[0] != '0'
    "PRESENT": ["d", 1, 1, 1, 1, 1, 1, 1, 1, 1, 1],          # set at all
    "INT":     ["d", 0, 0, 1, 2, -1, 0, 1, 0, 0, 0],         # atoi(e)
}
# the INT rows that hold a set value to a range
EXPECT_INT = {
    "SSLCR_BN_REPEAT": ["d", 1, 1, 1, 2, 1, 1, 1, 1, 1, 1],                          # below 1 becomes 1
    "SSLCR_EW_CAP":    ["d", 256, 256, 256, 256, 256, 256, 256, 256, 256, 256],      # below 256 becomes 256
}
EW_CAP = {"100": 256, "256": 256, "65536": 65535}
DEFAULTS = {1: {"SSLCR_PP64", "SSLCR_H16_TW8", "SSLCR_H16_RAW", "SSLCR_S2", "SSLCR_S2D", "SSLCR_S2W", "SSLCR_WG_DMA", "SSLCR_WGRAD_WIDE",
                "SSLCR_GEMM_LDS", "SSLCR_WG_STAGGER", "SSLCR_SEGMENTS", "SSLCR_BN_PAIR", "SSLCR_BN_PAIR_G", "SSLCR_YBITS",
                "SSLCR_UNFOLD_EVAL", "SSLCR_STEM_POOL", "SSLCR_FUSE_STEM_BWD", "SSLCR_BN_REPEAT"},
            0: {"SSLCR_POOL_BANDS", "SSLCR_BN_ONE_LAUNCH", "SSLCR_COMM_SELFTEST", "SSLCR_EW_CAP"},
            2: {"SSLCR_STEM_POOL_FORM"}}
RULES = {"LEAD0": {"SSLCR_SEGMENTS", "SSLCR_WGRAD_WIDE"}, "PRESENT": {"SSLCR_COMM_SELFTEST"},
         "INT": {"SSLCR_STEM_POOL_FORM", "SSLCR_WG_STAGGER", "SSLCR_BN_REPEAT", "SSLCR_EW_CAP"}}      # every other row: ATOI
CALL = {"SSLCR_FUSE_STEM_BWD", "SSLCR_COMM_SELFTEST"}
NAMES = sorted(set().union(*DEFAULTS.values()))

CHILD = f"""import sys; sys.path[:0] = [{ROOT!r}]
import json, os
from ssl_cr_histo_amd import kernels
first = kernels.switches()
# after the first query: a `call` row sees a changed environment, a `process` row does not
os.environ["SSLCR_FUSE_STEM_BWD"] = "0"; os.environ["SSLCR_COMM_SELFTEST"] = ""; os.environ["SSLCR_PP64"] = "0"; os.environ["SSLCR_EW_CAP"] = "999"
import torch
json.dump({{"first": first, "later": kernels.switches(), "device": torch.cuda.is_initialized()}}, open(sys.argv[1], "w"))
"""


@pytest.fixture(scope="module")
def listings(tmp_path_factory):
    """{key: the child's result}: key = a string of STRINGS (every variable set to it; None: none set) or ("EW_CAP", s)"""
    assert not sorted(k for k in os.environ if k.startswith("SSLCR_")), "unset every SSLCR_* variable: the children inherit them"
    from ssl_cr_histo_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    tmp = tmp_path_factory.mktemp("switches")
    envs = {s: ({} if s is None else {n: s for n in NAMES}) for s in STRINGS}
    envs.update({("EW_CAP", s): {"SSLCR_EW_CAP": s} for s in EW_CAP})
    procs = {}
    for i, (key, env) in enumerate(envs.items()):
        out = str(tmp / f"{i}.json")
        procs[key] = (out, subprocess.Popen([sys.executable, "-c", CHILD, out], env=dict(os.environ, **env), stdout=subprocess.PIPE,
                                            stderr=subprocess.STDOUT, text=True))
    got = {}
    for key, (out, p) in procs.items():
        text, _ = p.communicate(timeout=600)
        assert p.returncode == 0, f"{key!r}: {text[-3000:]}"
        with open(out) as f:
            got[key] = json.load(f)
        assert got[key]["device"] is False, "the listing opened the device"
    return got


def test_the_table_is_the_23_switches_with_their_rules_and_defaults(listings):
    t = listings[None]["first"]
    assert sorted(t) == NAMES and len(t) == 23
    for name, row in t.items():
        assert row["rule"] == next((r for r, names in RULES.items() if name in names), "ATOI"), name
        assert row["default"] == next(d for d, names in DEFAULTS.items() if name in names), name
        assert row["when"] == ("call" if name in CALL else "process"), name
        assert row["set"] is False and row["value"] == row["default"], name
        assert row["group"] in ("routing", "form", "engine", "measurement") and len(row["meaning"]) > 20, name


@pytest.mark.parametrize("i", range(1, len(STRINGS)), ids=[repr(s) for s in STRINGS[1:]])
def test_every_rule_reads_the_string_as_its_literal_row_says(listings, i):
    t = listings[STRINGS[i]]["first"]
    bad = {}
    for name, row in t.items():
        want = EXPECT_INT.get(name, EXPECT[row["rule"]])[i]
        if not (row["set"] is True and row["value"] == want):
            bad[name] = (row["rule"], row["set"], row["value"], "want", want)
    assert not bad, (STRINGS[i], bad)


def test_ew_cap_is_held_to_its_range(listings):
    for s, want in EW_CAP.items():
        row = listings[("EW_CAP", s)]["first"]["SSLCR_EW_CAP"]
        assert row["set"] is True and row["value"] == want, (s, row)
        others = {n: r for n, r in listings[("EW_CAP", s)]["first"].items() if n != "SSLCR_EW_CAP"}
        assert all(r["set"] is False and r["value"] == r["default"] for r in others.values())


def test_process_rows_are_read_once_and_call_rows_at_every_query(listings):
    """the child changes four variables after its first query: the two `call` rows follow, the `process` rows keep what they read"""
    first, later = listings[None]["first"], listings[None]["later"]
    assert (later["SSLCR_FUSE_STEM_BWD"]["set"], later["SSLCR_FUSE_STEM_BWD"]["value"]) == (True, 0)
    assert (later["SSLCR_COMM_SELFTEST"]["set"], later["SSLCR_COMM_SELFTEST"]["value"]) == (True, 1)
    for name in NAMES:
        if name not in CALL:
            assert later[name] == first[name], name


def test_the_listing_refuses_an_index_outside_the_table():
    from ssl_cr_histo_amd import _lib as L
    lib, r = L.lib(), L.SwitchRow()
    n = lib.sslcr_switch_count()
    assert n == 23 and lib.sslcr_switch_info(n - 1, r) == 0 and r.name.startswith(b"SSLCR_")
    for i in (-1, n):
        assert lib.sslcr_switch_info(i, r) == -1 and b"index" in lib.sslcr_last_error()
    assert lib.sslcr_switch_info(0, None) == -1


def test_the_header_lists_the_rows_of_the_library(listings):
    """the comment table of include/sslcr.h: the same names in the same order, each with the row's rule, when, group and default"""
    with open(os.path.join(ROOT, "include", "sslcr.h")) as f:
        rows = re.findall(r"^ \*   (SSLCR_\w+) +(\w+) +(\w+) +(\w+) +(-?\d+)$", f.read(), flags=re.M)
    t = listings[None]["first"]
    assert [r[0] for r in rows] == list(t)
    for name, rule, when, group, default in rows:
        assert (rule, when, group, int(default)) == (t[name]["rule"], t[name]["when"], t[name]["group"], t[name]["default"]), name
