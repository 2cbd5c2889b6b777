"""DESIGN.md section 6.19, "cost of the flag" (reported, not gated: there is no parent to hold it against): C2's steps (800x800,
depth 8, 64 iterations per step, bench.py's timed region: steps enqueued back to back, one synchronisation) on
scenes/cornell_textured.txt in a session with PT_TEXTURES and the scene's textures set and in one without the flag, alternating,
three runs each in one process -- and the per-call form (one pt_trace per iteration, synchronous, no host image), where the
textured session runs a kernel per bounce and the other a single launch.
    python profiles/textures/measure.py [OUT.json]       (default: profiles/textures/texture_cost.json)"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge
pt = ge.load_package()


def set_textures(scene, flags):
    if flags & pt.PT_TEXTURES:
        for m, tex in scene.textures.items():
            pt.set_texture(m, tex)


def run_steps(scene, flags, steps=20, warmup=5, batch=64):
    s = pt.Scene(scene.geoms, scene.materials, scene.camera, scene.traceDepth)
    pt.pathtraceInit(s, flags=flags, max_batch=batch)
    try:
        set_textures(scene, flags)
        it = 1
        for _ in range(warmup):
            pt.trace_batch_async(it, batch); it += batch
        pt.synchronize()
        r0 = pt.counters()[0]
        t0 = time.perf_counter()
        for k in range(steps):
            pt.trace_batch_async(it, batch); it += batch
        pt.synchronize()
        dt = time.perf_counter() - t0
        rays = pt.counters()[0] - r0
        w, h = s.resolution
        img = pt.get_image(w * h)
        return {"ms_per_step": dt / steps * 1e3, "mrays_per_s": rays / dt / 1e6, "grays_per_s": rays / dt / 1e9, "rays_per_step": rays / steps,
                "mean_of_image": float(img.mean() / (it - 1))}
    finally:
        pt.pathtraceFree()


def run_calls(scene, flags, calls=200, warmup=20):
    s = pt.Scene(scene.geoms, scene.materials, scene.camera, scene.traceDepth)
    pt.pathtraceInit(s, flags=flags, max_batch=1)
    try:
        set_textures(scene, flags)
        L = pt.library()
        for it in range(1, warmup + 1):
            L.pt_trace(None, 0, it, None)
        t0 = time.perf_counter()
        for it in range(warmup + 1, warmup + calls + 1):
            if L.pt_trace(None, 0, it, None) != 0:
                raise pt.PtError(L.pt_last_error().decode())
        dt = time.perf_counter() - t0
        st = pt.get_stats()
        return {"ms_per_call": dt / calls * 1e3, "bounces": int(st.bounces), "rays_per_call": int(st.rays)}
    finally:
        pt.pathtraceFree()


out = {"workload": "800x800 scenes/cornell_textured.txt, depth 8, PT_COMPACT with PT_TEXTURES and the scene's three textures, and without the flag; steps: 64 iterations per step, 5 warm-up + "
                   "20 timed, back to back, one synchronisation; calls: 20 warm-up + 200 timed synchronous pt_trace calls, no host image"}
scene = pt.load_scene(os.path.join(ROOT, "scenes", "cornell_textured.txt"))
for key in ("steps_textured", "steps_plain", "calls_textured", "calls_plain"):
    out[key] = []
for k in range(3):
    out["steps_textured"].append(run_steps(scene, pt.PT_COMPACT | pt.PT_TEXTURES))
    out["steps_plain"].append(run_steps(scene, pt.PT_COMPACT))
for k in range(3):
    out["calls_textured"].append(run_calls(scene, pt.PT_COMPACT | pt.PT_TEXTURES))
    out["calls_plain"].append(run_calls(scene, pt.PT_COMPACT))
med = lambda rows, f: sorted(r[f] for r in rows)[1]
out["median_ms_per_step"] = {"textured": med(out["steps_textured"], "ms_per_step"), "plain": med(out["steps_plain"], "ms_per_step")}
out["median_ms_per_call"] = {"textured": med(out["calls_textured"], "ms_per_call"), "plain": med(out["calls_plain"], "ms_per_call")}
out["step_cost"] = out["median_ms_per_step"]["textured"] / out["median_ms_per_step"]["plain"] - 1.0
out["call_cost"] = out["median_ms_per_call"]["textured"] / out["median_ms_per_call"]["plain"] - 1.0
print(json.dumps(out, indent=1))
dest = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "textures", "texture_cost.json")
with open(dest, "w") as f:
    json.dump(out, f, indent=1)
