#!/usr/bin/env python3
"""The converged picture the quality test of tests/test_albedo_model_cpu.py measures against:
scenes/cornell_textured.txt at 128 x 128 with its textures, the mean of iterations 1 .. 1024 of tests/texture_model.py's
Model.  Minutes of CPU, so it is run once and the result committed (tests/golden/albedo_ref.npz); the test then traces only
its own 64 iterations.

    python3 tests/golden/make_albedo_ref.py [iterations]

Stored: the mean [128 * 128, 3] float32, the iteration count, the frame size."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge  # noqa: E402
from oracle import pyoracle as po  # noqa: E402
import texture_model as tm  # noqa: E402
from gpu_common import _resized  # noqa: E402

W = H = 128


def main():
    iters = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    pt = ge.load_package()                       # (the host-side scene loader only: no GPU, no library call)
    pt.build_host()
    po.build()
    s = pt.load_scene(os.path.join(ROOT, "scenes", "cornell_textured.txt"))
    m = tm.Model(po, s.geoms, s.materials, _resized(s.camera, W, H), s.traceDepth)
    for k, t in dict(s.textures).items():
        m.set_texture(k, t)
    t0 = time.time()
    for it in range(1, iters + 1):
        m.iterate(it)
        if it % 64 == 0:
            print("iteration %4d/%d  %.0f s" % (it, iters, time.time() - t0), flush=True)
    mean = (m.image / np.float32(iters)).astype(np.float32)
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "albedo_ref.npz"), mean=mean, iterations=np.int32(iters),
                        width=np.int32(W), height=np.int32(H))
    print("done: %d iterations, %.0f s" % (iters, time.time() - t0))


if __name__ == "__main__":
    main()
