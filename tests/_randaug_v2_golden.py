"""Reader of tests/golden/randaug_v2.npz (written by tests/golden/make_randaug_v2.py from the reference's own op functions)."""
import os

import numpy as np

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "randaug_v2.npz")


class Golden:
    def __init__(self):
        z = np.load(PATH)
        self.pool = [str(s) for s in z["pool"]]
        self.pillow_version = str(z["pillow_version"])
        self.images = []
        while f"img_{len(self.images)}" in z.files:
            self.images.append(z[f"img_{len(self.images)}"])
        seen = [0] * len(self.images)
        self.op_cases = []          # (name, image index, val, seed, sign or None, expected)
        for (op, j, seed, sign), val in zip(z["op_case"], z["op_val"]):
            self.op_cases.append((self.pool[op], int(j), float(val), int(seed), None if sign < 0 else int(sign), z[f"op_out_{j}"][seed_idx(seen, j)]))
        self.pipe_cases = [(int(n), int(m), int(j), int(seed), z[f"pipe_out_{p}"]) for p, (n, m, j, seed) in enumerate(z["pipe_case"])]


def seed_idx(seen, j):
    seen[j] += 1
    return seen[j] - 1


_G = None


def golden():
    global _G
    if _G is None:
        _G = Golden()
    return _G
