#!/usr/bin/env python3
"""The converged picture the quality tests of tests/test_svgf_model_cpu.py measure against: 200 x 200
Cornell under the scene's camera moved by (0.3, 0.2, 0), the mean of iterations 1 .. 1024 on the oracle (iterations 1 .. 4 one by
one as the test accumulates them, the rest in parallel).  Half a minute of CPU that every run of the suite would repeat, so it is
run once and the result committed (tests/golden/svgf_ref.npz); the test then traces only the 64 + 4 iterations it filters.

    python3 tests/golden/make_svgf_ref.py

Stored: the mean [200 * 200, 3] float32, the iteration count, the frame size, the move."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import pyoracle as po  # noqa: E402
from gpu_common import _resized  # noqa: E402

W = H = 200
MOVE = (0.3, 0.2, 0.0)
ITERATIONS = 1024


def main():
    po.build()
    z = np.load(os.path.join(ROOT, "tests", "golden", "scenes.npz"))
    cam = _resized(z["cornell__camera"], W, H)
    cam["position"][0] += np.asarray(MOVE, dtype=np.float32)
    cam["lookAt"][0] += np.asarray(MOVE, dtype=np.float32)
    tr = po.Tracer(z["cornell__geoms"], z["cornell__materials"], cam, int(z["cornell__depth"]))
    acc = np.zeros((W * H, 3), dtype=np.float32)
    for it in range(1, 5):
        tr.image[:] = 0
        tr.iterate(it, threads=8)
        acc = (acc + tr.image).astype(np.float32)
    tr.image[:] = acc
    tr.iterate_parallel(5, ITERATIONS - 4, 8)
    mean = (tr.image / np.float32(ITERATIONS)).astype(np.float32)
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "svgf_ref.npz"), mean=mean, iterations=np.int32(ITERATIONS),
                        width=np.int32(W), height=np.int32(H), move=np.asarray(MOVE, dtype=np.float32))
    print("done: %d iterations" % ITERATIONS)


if __name__ == "__main__":
    main()
