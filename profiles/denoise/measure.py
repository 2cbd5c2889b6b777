"""Device times of pt_denoise's launches on the GPU in front of you -> denoise_times.json.

    python profiles/denoise/measure.py [--out profiles/denoise/denoise_times.json] [--reps 30]

For 800x800 (cornell) and 3840x2160 (cornell_4k): after a batch of iterations and one warm-up pt_denoise, `reps` rounds of
k_gbuffer, every level of k_atrous (levels 5, sigmas 1.0 / 0.35 / 0.5) and a device-to-device hipMemcpyAsync of the 56 bytes
per pixel one level moves (44 read + 12 written; the copy itself reads AND writes that many), all timed with HIP events on
the session's stream in one process (ptdbg_denoise_times); medians, the sustained shader clock (pt_probe_clock) and the
ratio level time / copy time."""
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "denoise", "denoise_times.json"))
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    pt = ge.load_package()
    L = pt.library()
    L.ptdbg_denoise_times.argtypes = [C.POINTER(pt.DenoiseParams), C.c_int, C.c_int, C.c_void_p]
    z = np.load(os.path.join(ROOT, "tests", "golden", "scenes.npz"))
    levels = 5
    out = {"levels": levels, "sigmas": [1.0, 0.35, 0.5], "reps": a.reps, "frames": []}
    for name, spp in (("cornell", 16), ("cornell_4k", 4)):
        cam = z[name + "__camera"]
        w, h = (int(v) for v in cam[0]["resolution"])
        scene = pt.Scene(z[name + "__geoms"], z[name + "__materials"], cam, int(z[name + "__depth"]))
        pt.pathtraceInit(scene, flags=pt.PT_COMPACT, max_batch=spp)
        try:
            pt.trace_batch(1, spp, None)
            prm = pt.DenoiseParams(levels, 1.0, 0.35, 0.5)
            ms = np.zeros((a.reps, levels + 2), dtype=np.float32)
            rc = L.ptdbg_denoise_times(C.byref(prm), spp, a.reps, ms.ctypes.data)
            if rc != 0:
                raise SystemExit("ptdbg_denoise_times: %s" % L.pt_last_error().decode())
            ghz = pt.probe_clock(2000)
            med = np.median(ms.astype(np.float64), axis=0)
            lo, hi = ms.min(axis=0), ms.max(axis=0)
            copy_ms = float(med[-1])
            npix = w * h
            frame = {"scene": name, "width": w, "height": h, "iterations": spp, "sustained_clock_ghz": ghz,
                     "k_gbuffer_ms": {"median": float(med[0]), "min": float(lo[0]), "max": float(hi[0])},
                     "copy_d2d": {"bytes": npix * 56, "median_ms": copy_ms, "min_ms": float(lo[-1]), "max_ms": float(hi[-1]),
                                  "GB_per_s_copied": npix * 56 / (copy_ms * 1e-3) / 1e9},
                     "k_atrous_levels": []}
            for l in range(levels):
                m = float(med[1 + l])
                frame["k_atrous_levels"].append({"level": l, "step": 1 << l, "median_ms": m, "min_ms": float(lo[1 + l]),
                                                 "max_ms": float(hi[1 + l]), "level_over_copy": m / copy_ms,
                                                 "GB_per_s_moved": npix * 56 / (m * 1e-3) / 1e9})
            frame["filter_ms_sum_of_medians"] = float(med[1:1 + levels].sum())
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
