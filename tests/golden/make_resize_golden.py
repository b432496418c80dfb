#!/usr/bin/env python
"""Generate tests/golden/resize_pil.npz: what Pillow's ``Image.resize`` returns for the cases of the resize kernel tests
(tests/_resize_cases.py), so that the GPU tests hold their bound -- EQUALITY -- where Pillow is not installed.

Run where Pillow is installed:   python tests/golden/make_resize_golden.py
The file pins the Pillow that is installed where this runs (``pillow_version``; 12.2.0 for the committed file).

Layout (arrays only):
  pillow_version        the version string
  in_<source>           two of the seeded inputs, [H, W, 3] uint8 (tests/test_resize_cpu.py checks that the seeds still give them)
  <source>|<oh>x<ow>|<filter>|<box>     the output of Image.fromarray(in).resize((ow, oh), filter, box=box), [oh, ow, 3] uint8, for the
                        cases of tests/_resize_cases.py:RECORDED; <box> is "full" or the four numbers.  The L-mode cases are
                        channel 0 of these: Pillow resizes per channel.
  big...|...            the two LANCZOS cases whose input is too large to record (tests/_resize_cases.py:big_source)
A few tens of kilobytes: the cases that are not recorded fall through to the restatement (tests/_resize_ref.py), which
tests/test_resize_cpu.py holds equal to every array here.
"""
import os
import sys

import numpy as np
import PIL

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import _resize_cases as RC  # noqa: E402


def main():
    out = {"pillow_version": np.array(PIL.__version__)}
    for name in RC.RECORDED_INPUTS:
        out["in_" + name] = RC.source(name)
    for src, hw, f, box in RC.RECORDED:
        out[RC.key(src, hw, f, box)] = RC.pil_resize(RC.source(src), hw, f, box)
    for (h, w), hw in RC.BIG_CASES:
        out[RC.key(f"big{h}x{w}", hw, "lanczos", None)] = RC.pil_resize(RC.big_source(h, w), hw, "lanczos")
    path = os.path.join(HERE, "resize_pil.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {len(out)} arrays, {os.path.getsize(path)} bytes, Pillow {PIL.__version__}")


if __name__ == "__main__":
    main()
