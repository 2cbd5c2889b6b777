"""Makes tests/golden/sky_ref.npz: the converged picture tests/test_sky_model_cpu.py measures its two estimators against --
scenes/open_sky_sun.txt at 16 x 16 under the test's sun sky, the PLAIN model (no direct lighting: the oracle's stages and the
miss lookup, tests/direct_model.py with direct=False) at depth 2, the mean of ITERATIONS iterations from iteration 1001 on
(the test's own runs use iterations 1 .. 48).  Takes minutes; run from the repository root:
    python tests/golden/make_sky_ref.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import __graft_entry__ as ge  # noqa: E402
import direct_model as dm  # noqa: E402
import test_sky_model_cpu as t  # noqa: E402
from oracle import pyoracle as po  # noqa: E402

ITERATIONS = 65536


def main():
    pt = ge.load_package()
    pt.build_host()
    po.build()
    geoms, mats, cam, _ = t.load(pt, "open_sky_sun", 16, 16)
    texels = t.sun_sky(pt, 16)
    m = dm.Model(po, geoms, mats, cam, 2, direct=False)
    m.set_environment(texels)
    total = np.zeros((256, 3), dtype=np.float64)
    for it in range(1001, 1001 + ITERATIONS):
        pix, col = m.colours(it)                                         # one path per pixel
        total[pix] += col
    np.savez_compressed(os.path.join(HERE, "sky_ref.npz"), mean=(total / ITERATIONS).astype(np.float32), texels=texels,
                        iterations=np.int32(ITERATIONS))
    print("sky_ref.npz: mean %.6f over %d iterations" % ((total / ITERATIONS).mean(), ITERATIONS))


if __name__ == "__main__":
    main()
