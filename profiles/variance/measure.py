"""Device times of pt_denoise_variance's launches beside pt_denoise's, and of the gather kernel with and without the moments, on
the GPU in front of you -> variance_times.json.

    python profiles/variance/measure.py [--out profiles/variance/variance_times.json] [--reps 30]

profiles/denoise/measure.py's method: for 800x800 (cornell) and 3840x2160 (cornell_4k), in a PT_MOMENTS session after a batch of
iterations, `reps` rounds of every level of k_atrous (levels 5, sigmas 1.0 / 0.35 / 0.5; ptdbg_denoise_times) and of k_atrous_var
(levels 5, sigmas 4 / 0.35 / 0.5; ptdbg_variance_times), HIP events on the session's stream, medians.  The gather: 800x800, batches
of 64 iterations with pt_set_profiling, the mean device time of the gather launch per batch, without and with PT_MOMENTS."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "variance", "variance_times.json"))
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    pt = ge.load_package()
    L = pt.library()
    L.ptdbg_denoise_times.argtypes = [C.POINTER(pt.DenoiseParams), C.c_int, C.c_int, C.c_void_p]
    L.ptdbg_variance_times.argtypes = [C.POINTER(pt.VarianceParams), C.c_int, C.c_int, C.c_void_p]
    z = np.load(os.path.join(ROOT, "tests", "golden", "scenes.npz"))
    levels = 5
    out = {"levels": levels, "reps": a.reps, "frames": [], "gather_64spp_800x800": {}}
    for name, spp in (("cornell", 16), ("cornell_4k", 4)):
        cam = z[name + "__camera"]
        w, h = (int(v) for v in cam[0]["resolution"])
        scene = pt.Scene(z[name + "__geoms"], z[name + "__materials"], cam, int(z[name + "__depth"]))
        pt.pathtraceInit(scene, flags=pt.PT_COMPACT | pt.PT_MOMENTS, max_batch=spp)
        try:
            pt.trace_batch(1, spp, None)
            plain = np.zeros((a.reps, levels + 2), dtype=np.float32)
            prm = pt.DenoiseParams(levels, 1.0, 0.35, 0.5)
            if L.ptdbg_denoise_times(C.byref(prm), spp, a.reps, plain.ctypes.data) != 0:
                raise SystemExit("ptdbg_denoise_times: %s" % L.pt_last_error().decode())
            guided = np.zeros((a.reps, levels), dtype=np.float32)
            vrm = pt.VarianceParams(levels, 4.0, 0.35, 0.5)
            if L.ptdbg_variance_times(C.byref(vrm), spp, a.reps, guided.ctypes.data) != 0:
                raise SystemExit("ptdbg_variance_times: %s" % L.pt_last_error().decode())
            mp, mg = np.median(plain.astype(np.float64), axis=0)[1:1 + levels], np.median(guided.astype(np.float64), axis=0)
            frame = {"scene": name, "width": w, "height": h, "iterations": spp, "sustained_clock_ghz": pt.probe_clock(2000),
                     "levels": [{"level": l, "step": 1 << l, "k_atrous_median_ms": float(mp[l]), "k_atrous_var_median_ms": float(mg[l]),
                                 "ratio": float(mg[l] / mp[l])} for l in range(levels)],
                     "k_atrous_sum_ms": float(mp.sum()), "k_atrous_var_sum_ms": float(mg.sum())}
            out["frames"].append(frame)
            print(json.dumps(frame))
        finally:
            pt.pathtraceFree()
    cam = z["cornell__camera"]
    scene = pt.Scene(z["cornell__geoms"], z["cornell__materials"], cam, int(z["cornell__depth"]))
    for key, extra in (("k_gather", 0), ("k_gather_moments", pt.PT_MOMENTS)):
        pt.pathtraceInit(scene, flags=pt.PT_COMPACT | extra, max_batch=64)
        try:
            pt.trace_batch(1, 64, None)                            # warm-up
            pt.set_profiling(True)
            for k in range(1, 9):
                pt.trace_batch(1 + 64 * k, 64, None)
            ms, launches = pt.get_profile()["gather"]
            out["gather_64spp_800x800"][key] = {"mean_ms": ms / max(1, launches), "launches": int(launches)}
        finally:
            pt.pathtraceFree()
    print(json.dumps(out["gather_64spp_800x800"]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
