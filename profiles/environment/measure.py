"""DESIGN.md section 6.16, "cost with a map": C2 (800x800 Cornell, depth 8, 64 iterations per step, bench.py's timed region: steps
enqueued back to back, one synchronisation) with a 64 x 64 environment map and with none, alternating, three runs each in one
process; scenes/open_sky.txt at 800x800 for information.  The sustained shader clock is probed while the steps run.
    python profiles/environment/measure.py [OUT.json]       (default: profiles/environment/map_cost.json)"""
import json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge
pt = ge.load_package()
import torch

def run(scene, texels, steps=20, warmup=5, batch=64):
    pt.pathtraceInit(scene, flags=pt.PT_COMPACT, max_batch=batch)
    try:
        if texels is not None:
            pt.set_environment(texels)
        it = 1
        for _ in range(warmup):
            pt.trace_batch_async(it, batch); it += batch
        pt.synchronize()
        r0 = pt.counters()[0]
        t0 = time.perf_counter()
        for k in range(steps):
            pt.trace_batch_async(it, batch); it += batch
            if k == steps // 2:
                ghz = pt.probe_clock(200)
        pt.synchronize()
        dt = time.perf_counter() - t0
        rays = pt.counters()[0] - r0
        w, h = scene.resolution
        img = pt.get_image(w * h)
        return {"ms_per_step": dt / steps * 1e3, "mrays_per_s": rays / dt / 1e6, "rays_per_step": rays / steps, "sustained_ghz": ghz,
                "mean_of_image": float(img.mean() / (it - 1))}
    finally:
        pt.pathtraceFree()

out = {"workload": "800x800, depth 8, PT_COMPACT, 64 iterations per step, 5 warm-up + 20 timed steps, back to back, one synchronisation"}
cornell = pt.load_scene(os.path.join(ROOT, "scenes", "cornell.txt"))
sky = pt.load_scene(os.path.join(ROOT, "scenes", "open_sky.txt"))
rng = np.random.default_rng(64)
tex = rng.uniform(0, 2, (6, 64, 64, 3)).astype(np.float32)
out["c2_none"], out["c2_map64"] = [], []
for k in range(3):
    out["c2_none"].append(run(cornell, None))
    out["c2_map64"].append(run(cornell, tex))
grad = pt.gradient_cubemap(64, (0.25, 0.45, 1.0), (0.9, 0.85, 0.8), (0.3, 0.25, 0.2))
out["open_sky_gradient64"] = [run(sky, grad) for _ in range(2)]
out["open_sky_none"] = [run(sky, None)]
print(json.dumps(out, indent=1))
dest = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "environment", "map_cost.json")
with open(dest, "w") as f:
    json.dump(out, f, indent=1)
