"""Device times of the filters with first-hit albedo demodulation switched off and on, on the GPU in front of you ->
albedo_times.json.

    python profiles/denoise/measure_albedo.py [--out profiles/denoise/albedo_times.json] [--reps 30]

scenes/cornell_textured.txt with its textures (PT_TEXTURES) at 800x800 (16 spp) and at 3840x2160 (4 spp): after a batch of
iterations, `reps` times alternately pt_set_denoise_albedo(0) and (1), each followed by one ptdbg_denoise_times round (its own
warm-up call first): k_gbuffer forced -- the ALB form when the switch is on --, every level of k_atrous (levels 5, sigmas 1.0 /
0.35 / 0.5; with the switch on level 0 divides as it loads and level 4 multiplies as it stores) and a device-to-device
hipMemcpyAsync of the bytes one level moves (56 per pixel, 68 for a demodulating level), all timed with HIP events on the
session's stream in one process; medians."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402


def resized(cam, w, h):
    """the camera at another resolution: pixelLength = 2 * tan(fov) / resolution, as the scene loader computes it"""
    c = cam.copy()
    c["resolution"][0] = (w, h)
    yscaled = np.tan(np.float32(c["fov"][0][1]) * np.float32(np.pi / 180))
    xscaled = np.float32(yscaled * np.float32(w) / np.float32(h))
    c["pixelLength"][0] = (np.float32(2 * xscaled / np.float32(w)), np.float32(2 * yscaled / np.float32(h)))
    return c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "denoise", "albedo_times.json"))
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    pt = ge.load_package()
    L = pt.library()
    L.ptdbg_denoise_times.argtypes = [C.POINTER(pt.DenoiseParams), C.c_int, C.c_int, C.c_void_p]
    s = pt.load_scene(os.path.join(ROOT, "scenes", "cornell_textured.txt"))
    levels = 5
    out = {"scene": "cornell_textured", "levels": levels, "sigmas": [1.0, 0.35, 0.5], "reps": a.reps, "frames": []}
    for w, h, spp in ((800, 800, 16), (3840, 2160, 4)):
        scene = pt.Scene(s.geoms, s.materials, resized(s.camera, w, h), s.traceDepth)
        pt.pathtraceInit(scene, flags=pt.PT_COMPACT | pt.PT_TEXTURES, max_batch=spp)
        try:
            for k, t in dict(s.textures).items():
                pt.set_texture(k, t)
            pt.trace_batch(1, spp, None)
            prm = pt.DenoiseParams(levels, 1.0, 0.35, 0.5)
            ms = np.zeros((2, a.reps, levels + 2), dtype=np.float32)
            for rep in range(a.reps):
                for on in (0, 1):
                    pt.set_denoise_albedo(on)
                    rc = L.ptdbg_denoise_times(C.byref(prm), spp, 1, ms[on, rep].ctypes.data)
                    if rc != 0:
                        raise SystemExit("ptdbg_denoise_times: %s" % L.pt_last_error().decode())
            npix = w * h
            frame = {"width": w, "height": h, "iterations": spp, "sustained_clock_ghz": pt.probe_clock(2000)}
            for on, name in ((0, "switch_off"), (1, "switch_on")):
                med = np.median(ms[on].astype(np.float64), axis=0)
                lo, hi = ms[on].min(axis=0), ms[on].max(axis=0)
                per_px = 68 if on else 56
                frame[name] = {"k_gbuffer_ms": {"median": float(med[0]), "min": float(lo[0]), "max": float(hi[0])},
                               "k_atrous_levels_ms": [{"level": l, "median": float(med[1 + l]), "min": float(lo[1 + l]), "max": float(hi[1 + l])}
                                                      for l in range(levels)],
                               "filter_ms_sum_of_medians": float(med[1:1 + levels].sum()),
                               "copy_d2d": {"bytes_per_pixel": per_px, "median_ms": float(med[-1]), "min_ms": float(lo[-1]), "max_ms": float(hi[-1]),
                                            "GB_per_s_copied": npix * per_px / (float(med[-1]) * 1e-3) / 1e9}}
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
