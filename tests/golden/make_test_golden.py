#!/usr/bin/env python
"""Generate tests/golden/kather_test.npz and tests/golden/bpq_test.npz by running the REFERENCE's own test() functions on CPU:
eval_Kather_SSL_CR.test (:182-245), eval_Kather_SSL.test (:154-213), eval_BreastPathQ_SSL_CR.test (:178-242) and
eval_BreastPathQ_SSL.test (:152-216).

Run in the build container only (needs the reference checkout, as make_golden.py):   python tests/golden/make_test_golden.py
The reference's Python never travels; the inputs come from the seeded generators of oracle.cases (tests/_inference_util.py), so the
files hold outputs only.  Everything else -- stubs, seeded weights, the slice of eval_Kather_SSL.py that parses -- is make_golden.py's.
"""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))            # tests/: _inference_util, _f64

import make_golden as G                              # noqa: E402  (sets up the reference import path and the stubs)
import _inference_util as U                          # noqa: E402


def gen_kather(out):
    c = U.TEST_CASES["kather"]
    model, cls = G.build("finetune", "finetune", c["classes"], rand_stats=True)
    U.scale_head(cls, c["head_scale"])
    m = importlib.import_module("eval_Kather_SSL_CR")
    pred, target, score = m.test(G.args_ns(), model, cls, U.kather_test_batches())
    top2 = score.double().topk(2, dim=1).values
    margin = (top2[:, 0] - top2[:, 1]).numpy()
    share = float((margin > U.MARGIN).mean())
    if share < U.MARGIN_SHARE:
        raise SystemExit(f"kather_test: only {share:.2f} of the rows have a top-2 margin above {U.MARGIN}: change the seed")
    out["kather_test/pred"], out["kather_test/target"], out["kather_test/score"] = pred.numpy(), target.numpy(), score.numpy()
    out["kather_test/margin"] = margin
    pred2, target2 = G.kather_sup_module().test(G.args_ns(), model, cls, U.kather_test_batches(), torch.nn.CrossEntropyLoss())
    out["kather_test/sup_pred"], out["kather_test/sup_target"] = pred2.numpy(), target2.numpy()
    print(f"kather_test: {len(pred)} rows, margin share {share:.2f}, score range {float(score.min()):.3f}..{float(score.max()):.3f}, pred {pred.tolist()}")


def gen_bpq(out):
    c = U.TEST_CASES["bpq"]
    model, cls = G.build("finetune", "finetune", c["classes"], rand_stats=True)
    m = importlib.import_module("eval_BreastPathQ_SSL_CR")
    o, f, ta, tb = m.test(G.args_ns(), model, cls, U.bpq_test_batches())
    out["bpq_test/outputs"], out["bpq_test/feats"], out["bpq_test/targetsA"], out["bpq_test/targetsB"] = (v.numpy() for v in (o, f, ta, tb))
    m2 = importlib.import_module("eval_BreastPathQ_SSL")
    o2, f2, ta2, tb2 = m2.test(G.args_ns(), model, cls, torch.nn.MSELoss(), U.bpq_test_batches())
    out["bpq_test/sup_outputs"], out["bpq_test/sup_feats"] = o2.numpy(), f2.numpy()
    print(f"bpq_test: outputs {o.tolist()}")


def main():
    for name, fn in (("kather_test", gen_kather), ("bpq_test", gen_bpq)):
        out = {}
        with torch.no_grad():
            fn(out)
        np.savez_compressed(os.path.join(HERE, f"{name}.npz"), **out)
        print("wrote", name)


if __name__ == "__main__":
    main()
