"""Device times of pt_denoise_temporal's launches on the GPU in front of you -> temporal_times.json.

    python profiles/denoise/measure_temporal.py [--out profiles/denoise/temporal_times.json] [--reps 30]

For 800x800 (cornell) and 3840x2160 (cornell_4k): a batch of iterations and a temporal call at the scene's camera, the camera
and its lookAt translated by (0.3, 0.2, 0), pt_clear_image, one iteration; then, where the next temporal call reprojects, one
warm-up round and `reps` rounds of k_reproject, k_temporal_blend, level 0 from the blended plane (k_atrous<false>, step 1),
level 0 from the running sum (k_atrous<true>: what pt_denoise runs), level 1 (k_atrous<false>, step 2) and
device-to-device hipMemcpyAsync of the bytes the two new kernels move (96 and 44 per pixel; a copy reads AND writes that
many), all timed with HIP events on the session's stream in one process (ptdbg_temporal_times); medians, the sustained
shader clock (pt_probe_clock), the share of pixels that found history and, of the wave-wide gathers of k_reproject, the
share that was one contiguous run of pixels (the model's projection, tests/temporal_model.py, on the device's G-buffers)."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge  # noqa: E402

ITEMS = ("k_reproject", "k_temporal_blend", "level0_k_atrous_false_step1", "level0_k_atrous_true", "level1_k_atrous_false_step2",
         "copy_d2d_96B", "copy_d2d_44B")
MOVE = (0.3, 0.2, 0.0)


def gather_shape(q, w, h):
    """of the waves (64 consecutive pixels of a row) with at least one gather: the share whose gathered pixels are
    consecutive in lane order, and the mean number of 128-byte lines of the old G-buffer plane (16 B per pixel) they touch"""
    runs = lines = waves = 0
    for y in range(h):
        row = q[y * w:(y + 1) * w]
        for x0 in range(0, w, 64):
            v = row[x0:x0 + 64]
            lane = np.flatnonzero(v >= 0)
            if lane.size == 0:
                continue
            waves += 1
            qq = v[lane]
            runs += bool((np.diff(qq) == np.diff(lane)).all())
            lines += np.unique(qq // 8).size
    return runs / max(1, waves), lines / max(1, waves)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "denoise", "temporal_times.json"))
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    pt = ge.load_package()
    L = pt.library()
    L.ptdbg_temporal_times.argtypes = [C.POINTER(pt.DenoiseParams), C.POINTER(pt.TemporalParams), C.c_int, C.c_int, C.c_void_p]
    z = np.load(os.path.join(ROOT, "tests", "golden", "scenes.npz"))
    out = {"levels": 5, "sigmas": [4.0, 0.35, 0.5], "temporal": [64, 0.1, 0.1], "move": list(MOVE), "reps": a.reps, "frames": []}
    for name, spp in (("cornell", 16), ("cornell_4k", 4)):
        cam = z[name + "__camera"]
        w, h = (int(v) for v in cam[0]["resolution"])
        depth = int(z[name + "__depth"])
        scene = pt.Scene(z[name + "__geoms"], z[name + "__materials"], cam, depth)
        pt.pathtraceInit(scene, flags=pt.PT_COMPACT, max_batch=spp)
        try:
            prm, tmp = pt.DenoiseParams(5, 4.0, 0.35, 0.5), pt.TemporalParams(64, 0.1, 0.1)
            pt.trace_batch(1, spp, None)
            pt.denoise_temporal(spp, prm, tmp)
            g_old = pt.gbuffer()
            moved = cam.copy()
            moved["position"][0] += np.asarray(MOVE, dtype=np.float32)
            moved["lookAt"][0] += np.asarray(MOVE, dtype=np.float32)
            pt.set_camera(moved, depth)
            pt.clear_image()
            pt.trace_batch(1, 1, None)
            ms = np.zeros((a.reps, len(ITEMS)), dtype=np.float32)
            rc = L.ptdbg_temporal_times(C.byref(prm), C.byref(tmp), 1, a.reps, ms.ctypes.data)
            if rc != 0:
                raise SystemExit("ptdbg_temporal_times: %s" % L.pt_last_error().decode())
            ghz = pt.probe_clock(2000)
            length = pt.history()[1]
            import temporal_model as tm
            npix = w * h
            old = {"camera": cam, "g": g_old, "C": np.zeros((npix, 3), np.float32), "N": np.ones(npix, np.float32)}
            g_new, mats = pt.gbuffer(), z[name + "__materials"]
            _, hn, q = tm.reproject(old, g_new, mats, w, h, 64, 0.1, 0.1)
            valid, qa = tm.project(cam, g_new["position"], w, h)
            m = np.clip(g_new["materialId"], 0, None)
            diffuse = (g_new["materialId"] >= 0) & (mats["hasReflective"][m] == 0) & (mats["hasRefractive"][m] == 0)
            attempted = np.where(valid & diffuse, qa, -1)          # the lanes that gather, whether or not the tests then pass
            runs, lines = gather_shape(attempted, w, h)
            med = np.median(ms.astype(np.float64), axis=0)
            frame = {"scene": name, "width": w, "height": h, "sustained_clock_ghz": ghz,
                     "share_with_history": float((length > 0).mean()), "share_with_history_model": float((hn > 0).mean()),
                     "gather_waves_contiguous_share": runs, "gather_lines_128B_per_wave_mean": lines, "gather_lines_128B_per_wave_ideal": 8.0}
            for k, item in enumerate(ITEMS):
                frame[item] = {"median_ms": float(med[k]), "min_ms": float(ms[:, k].min()), "max_ms": float(ms[:, k].max())}
            frame["k_reproject"]["bytes"] = npix * 96
            frame["k_temporal_blend"]["bytes"] = npix * 44
            frame["k_reproject"]["over_copy"] = float(med[0] / med[5])
            frame["k_temporal_blend"]["over_copy"] = float(med[1] / med[6])
            frame["k_reproject"]["over_level1"] = float(med[0] / med[4])
            frame["k_temporal_blend"]["over_level1"] = float(med[1] / med[4])
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
