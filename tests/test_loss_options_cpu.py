"""CPU-only side of the loss options (include/sslcr.h, library version 10): the new entry points are declared, exported and bound,
sslcr_loss_opts has the header's layout, the argument errors that are decided before any launch, LossOptions and its
from_criterion helper, the MSE loops' refusal, _plain_ce's unchanged refusal, and the host rule that says when a loader batch needs
a denominator launch and an all-reduce (never for the defaults)."""
import os
import re
from types import SimpleNamespace as ns

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sslcr_loss_ex", "sslcr_ce_denominator", "sslcr_net_set_loss_opts")


@pytest.fixture(scope="module")
def lib():
    from ssl_cr_histo_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build()
    from ssl_cr_histo_amd import engine  # noqa: F401  registers engine signatures
    return _lib.lib()


def _header():
    return open(os.path.join(ROOT, "include", "sslcr.h")).read()


def test_new_symbols_are_declared_exported_and_bound(lib):
    from ssl_cr_histo_amd import _lib
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), f"{name} is not declared in include/sslcr.h"
        assert hasattr(lib, name), f"{name} is not exported by libsslcr.so"
        assert name in _lib.SIGNATURES, f"no ctypes signature for {name}"
    assert re.search(r"typedef struct sslcr_loss_opts\s*{", code)


def test_version_is_10(lib):
    assert lib.sslcr_version() >= 10
    assert "10 = loss options" in _header()


def test_header_names_the_torch_call_each_field_restates():
    m = re.search(r"typedef struct sslcr_loss_opts \{(.*?)\} sslcr_loss_opts;", _header(), flags=re.S)
    body = m.group(1)
    for field, call in (("class_weight", "F.cross_entropy(weight=)"), ("label_smoothing", "F.cross_entropy(label_smoothing=)"),
                        ("ignore_index", "F.cross_entropy(ignore_index=)")):
        line = [ln for ln in body.splitlines() if re.search(r"\b%s;" % field, ln)]
        assert line and call in line[0], (field, line)


def test_loss_opts_layout_matches_the_header():
    """the fields of the mirror, by name and order (their offsets and the size: tests/test_abi_cpu.py, for every mirror)"""
    from ssl_cr_histo_amd import _lib as L
    names = [f for f, _ in L.LossOpts._fields_]
    assert names == ["class_weight", "label_smoothing", "ignore_index", "threshold", "temperature", "denominator", "stats"]
    assert L.MIRRORS["sslcr_loss_opts"] is L.LossOpts


def _desc(kind, Cn=2, nx=4, nu=0):
    """a descriptor whose pointers are never followed: every call below must fail on the host, before any launch"""
    from ssl_cr_histo_amd import _lib as L
    fake = 0x1000
    return L.LossDesc(kind, fake, fake, fake, fake, None, fake, nx, nu, Cn, 1.0, 1.0 / nx, 1.0)


def _opts(**kw):
    from ssl_cr_histo_amd import _lib as L
    d = dict(class_weight=None, label_smoothing=0.0, ignore_index=-100, threshold=0.0, temperature=0.0, denominator=None, stats=None)
    d.update(kw)
    return L.LossOpts(*[d[f] for f, _ in L.LossOpts._fields_])


@pytest.mark.parametrize("kind,Cn,kw,msg", [
    (0, 1, dict(label_smoothing=0.1), b"MSE"),
    (3, 1, dict(ignore_index=0), b"MSE"),
    (0, 1, dict(threshold=0.5), b"MSE"),
    (3, 1, dict(class_weight=0x1000), b"MSE"),
    (3, 1, dict(stats=0x1000), b"MSE"),
    (1, 65, dict(label_smoothing=0.1), b"args"),
    (2, 2, dict(label_smoothing=1.0), b"label_smoothing"),
    (2, 2, dict(label_smoothing=-0.1), b"label_smoothing"),
    (2, 2, dict(label_smoothing=float("nan")), b"label_smoothing"),
    (1, 2, dict(threshold=1.5), b"threshold"),
    (1, 2, dict(threshold=-0.1), b"threshold"),
    (1, 2, dict(temperature=-1.0), b"temperature"),
    (2, 2, dict(threshold=0.5), b"kind 1"),
    (2, 2, dict(temperature=0.5), b"kind 1"),
])
def test_loss_ex_argument_errors_before_any_launch(lib, kind, Cn, kw, msg):
    assert lib.sslcr_loss_ex(_desc(kind, Cn), _opts(**kw), None) == -1
    assert msg in lib.sslcr_last_error(), lib.sslcr_last_error()


def test_other_argument_errors_before_any_launch(lib):
    assert lib.sslcr_loss_ex(None, _opts(label_smoothing=0.1), None) == -1
    assert lib.sslcr_loss_ex(None, None, None) == -1                           # NULL opts: sslcr_loss's own check
    assert lib.sslcr_ce_denominator(0x1000, 4, 65, None, -100, 0x1000, None) == -1
    assert lib.sslcr_ce_denominator(0x1000, -1, 2, None, -100, 0x1000, None) == -1
    assert lib.sslcr_ce_denominator(0x1000, 4, 2, None, -100, None, None) == -1
    assert lib.sslcr_net_set_loss_opts(None, None) == -1
    assert b"null net" in lib.sslcr_last_error()


def test_loss_options_object():
    from ssl_cr_histo_amd import LossOptions
    from ssl_cr_histo_amd import kernels as K
    assert LossOptions is K.LossOptions
    o = LossOptions()
    assert o.is_default() and not o.needs_denominator()
    assert (o.class_weight, o.label_smoothing, o.ignore_index, o.threshold, o.temperature) == (None, 0.0, -100, 0.0, 0.0)
    for kw in (dict(label_smoothing=0.1), dict(threshold=0.95), dict(temperature=0.4)):
        o = LossOptions(**kw)
        assert not o.is_default() and o.needs_denominator(), kw
    for kw in (dict(class_weight=[1.0, 2.0]), dict(ignore_index=1), dict(class_weight=torch.ones(3), label_smoothing=0.1)):
        o = LossOptions(**kw)
        assert not o.is_default() and o.needs_denominator(), kw
    assert LossOptions(class_weight=[1, 3]).class_weight.dtype == torch.float32
    for bad in (dict(label_smoothing=1.0), dict(label_smoothing=-0.5), dict(threshold=1.1), dict(threshold=-0.1), dict(temperature=-1)):
        with pytest.raises(ValueError):
            LossOptions(**bad)
    with pytest.raises(ValueError):
        LossOptions(class_weight=[1.0, 2.0]).weight_on("cpu", 3)


def test_from_criterion():
    from ssl_cr_histo_amd import LossOptions
    assert LossOptions.from_criterion(torch.nn.CrossEntropyLoss()).is_default()
    w = torch.tensor([0.25, 1.0, 4.0], dtype=torch.float64)
    o = LossOptions.from_criterion(torch.nn.CrossEntropyLoss(weight=w, label_smoothing=0.1, ignore_index=2), threshold=0.9)
    assert torch.equal(o.class_weight, w.float()) and o.label_smoothing == pytest.approx(0.1) and o.ignore_index == 2
    assert o.threshold == 0.9 and o.temperature == 0.0
    for red in ("sum", "none"):
        with pytest.raises(ValueError) as e:
            LossOptions.from_criterion(torch.nn.CrossEntropyLoss(reduction=red))
        assert red in str(e.value)
    with pytest.raises(TypeError):
        LossOptions.from_criterion(torch.nn.MSELoss())


def test_mse_loops_refuse_options():
    """decided before the engine is asked for: no device needed.  Absent, None and all-default options pass that check"""
    from ssl_cr_histo_amd import LossOptions, steps
    o = LossOptions(label_smoothing=0.1)
    calls = {"bpq_cr_train": lambda a: steps.bpq_cr_train(a, None, None, None, None, [], [], None, 1),
             "bpq_cr_validate": lambda a: steps.bpq_cr_validate(a, None, None, [], 1),
             "bpq_sup_train": lambda a: steps.bpq_sup_train(a, None, None, [], None, None, 1)}
    for name, call in calls.items():
        with pytest.raises(ValueError) as e:
            call(ns(loss_options=o, lambda_u=1.0))
        assert name in str(e.value) and "mse" in str(e.value).lower()
        for ok in (ns(lambda_u=1.0), ns(loss_options=None, lambda_u=1.0), ns(loss_options=LossOptions(), lambda_u=1.0)):
            assert steps._loss_options(ok, mse=name) is None                # absent, None and the defaults pass the loop's check
    with pytest.raises(TypeError):
        steps._loss_options(ns(loss_options=torch.nn.CrossEntropyLoss()))
    assert steps._loss_options(ns()) is None and steps._loss_options(ns(loss_options=LossOptions())) is None
    assert steps._loss_options(ns(loss_options=o)) is o


def test_plain_ce_still_refuses_a_criterion_with_options():
    from ssl_cr_histo_amd import steps
    steps._plain_ce(torch.nn.CrossEntropyLoss(), "x")
    for bad in (torch.nn.CrossEntropyLoss(weight=torch.ones(6)), torch.nn.CrossEntropyLoss(label_smoothing=0.1),
                torch.nn.CrossEntropyLoss(ignore_index=3)):
        with pytest.raises(NotImplementedError) as e:
            steps._plain_ce(bad, "x")
        assert "args.loss_options" in str(e.value)


def test_denominator_plan():
    """a launch whenever any option is set AND the step holds part of the global batch (rows labelled -100 are left out once an
    option is set, so even smoothing-only options divide by the kept rows of the whole batch); an all-reduce only on top of a
    launch, with more than one rank; nothing for None or the defaults, and nothing on one rank with k = 1"""
    from ssl_cr_histo_amd import LossOptions, steps
    plain = [None, LossOptions()]
    data = [LossOptions(class_weight=[1.0, 2.0]), LossOptions(ignore_index=0), LossOptions(class_weight=[1.0, 2.0], label_smoothing=0.1),
            LossOptions(label_smoothing=0.1), LossOptions(threshold=0.9, temperature=0.5)]
    for k in (1, 2, 3):
        for world in (1, 2, 8):
            for o in plain:
                assert steps.denominator_plan(o, k, world) == (False, False), (o, k, world)
            for o in data:
                assert steps.denominator_plan(o, k, world) == (k > 1 or world > 1, world > 1), (o, k, world)
