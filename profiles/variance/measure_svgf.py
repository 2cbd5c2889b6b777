"""Device times of pt_denoise_svgf's three kernels beside a level of k_atrous_var and device-to-device copies of the bytes they move,
on the GPU in front of you -> svgf_times.json.

    python profiles/variance/measure_svgf.py [--out profiles/variance/svgf_times.json] [--reps 30]

profiles/variance/measure.py's method: for 800x800 (cornell) and 3840x2160 (cornell_4k), in a PT_MOMENTS session: a batch of
iterations and one pt_denoise_svgf at the scene's camera, the camera moved by (0.3, 0.2, 0), one iteration there, then `reps` rounds
of ptdbg_svgf_times -- k_reproject_svgf, k_svgf_blend, k_svgf_spatial with every pixel below the threshold and with none, level 0
from the records and level 1 of k_atrous_var, and copies of 112, 88 and 52 bytes per pixel --, HIP events on the session's stream,
medians."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

ITEMS = ("k_reproject_svgf", "k_svgf_blend", "k_svgf_spatial_all_pixels", "k_svgf_spatial_no_pixel", "k_atrous_var_level0_from_records",
         "k_atrous_var_level1", "copy_112_bytes_per_pixel", "copy_88_bytes_per_pixel", "copy_52_bytes_per_pixel")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "variance", "svgf_times.json"))
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    pt = ge.load_package()
    L = pt.library()
    L.ptdbg_svgf_times.argtypes = [C.POINTER(pt.VarianceParams), C.POINTER(pt.TemporalParams), C.c_int, C.c_int, C.c_int, C.c_void_p]
    z = np.load(os.path.join(ROOT, "tests", "golden", "scenes.npz"))
    out = {"levels": 5, "reps": a.reps, "frames": []}
    prm, tmp = pt.VarianceParams(5, 4.0, 0.35, 0.5), pt.TemporalParams(64, 0.1, 0.1)
    for name, spp in (("cornell", 16), ("cornell_4k", 4)):
        cam = z[name + "__camera"]
        w, h = (int(v) for v in cam[0]["resolution"])
        depth = int(z[name + "__depth"])
        scene = pt.Scene(z[name + "__geoms"], z[name + "__materials"], cam, depth)
        pt.pathtraceInit(scene, flags=pt.PT_COMPACT | pt.PT_MOMENTS, max_batch=spp)
        try:
            pt.trace_batch(1, spp, None)
            pt.denoise_svgf(spp, prm, tmp, 4)
            moved = cam.copy()
            moved["position"][0] += np.array([0.3, 0.2, 0.0], dtype=np.float32)
            moved["lookAt"][0] += np.array([0.3, 0.2, 0.0], dtype=np.float32)
            pt.set_camera(moved, depth)
            pt.clear_image()
            pt.trace_batch(1, 1, None)
            ms = np.zeros((a.reps, len(ITEMS)), dtype=np.float32)
            if L.ptdbg_svgf_times(C.byref(prm), C.byref(tmp), 4, 1, a.reps, ms.ctypes.data) != 0:
                raise SystemExit("ptdbg_svgf_times: %s" % L.pt_last_error().decode())
            med = np.median(ms.astype(np.float64), axis=0)
            frame = {"scene": name, "width": w, "height": h, "iterations_first_view": spp, "sustained_clock_ghz": pt.probe_clock(2000),
                     "median_ms": {k: float(v) for k, v in zip(ITEMS, med)}}
            out["frames"].append(frame)
            print(json.dumps(frame))
        finally:
            pt.pathtraceFree()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
