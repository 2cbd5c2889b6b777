"""One process for `rocprofv3 --kernel-trace --stats -- python profiles/denoise/denoise_once.py`: 800x800 Cornell, a batch of
16 iterations, then TWO pt_denoise calls (levels 5, with the RGBA form) with the camera unchanged.  The trace must show
k_gbuffer once, k_atrous 2 x 5 times, and no tonemap kernel (the last level writes the RGBA bytes itself)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

pt = ge.load_package()
z = np.load(os.path.join(ROOT, "tests", "golden", "scenes.npz"))
scene = pt.Scene(z["cornell__geoms"], z["cornell__materials"], z["cornell__camera"], int(z["cornell__depth"]))
pt.pathtraceInit(scene, flags=pt.PT_COMPACT, max_batch=16)
pt.trace_batch(1, 16, None)
for _ in range(2):
    img, rgba = pt.denoise(16, 5, 1.0, 0.35, 0.5, rgba=True)
print("denoised mean: min %.4f max %.4f" % (float(img.min()), float(img.max())))
pt.pathtraceFree()
