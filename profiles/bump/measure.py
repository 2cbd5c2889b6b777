"""DESIGN.md section 6.22, the two measurements on the kernels that change (the SH_TEX forms of k_bounce):
  textured   one run of profiles/textures/measure.py's textured step -- scenes/cornell_textured.txt at 800 x 800, depth 8,
             PT_COMPACT | PT_TEXTURES with the scene's three textures and NO bump map, 64 iterations per step, 5 warm-up + 20 timed
             steps back to back, one synchronisation -- as one JSON line.  textured_ab.sh runs it on a built checkout of the parent
             commit (whose library has no bump maps: this file uses nothing newer than pt_set_texture there) and on this tree,
             alternating; textured_ab.py applies section 6.16's rule to the six lines.
  bump       the cost of a bump map (reported, not gated): scenes/cornell_bumped.txt with its three maps and without any, both in
             a PT_TEXTURES session, alternating, three runs each: C2's step and the per-call form, as section 6.19 reports them.
    python profiles/bump/measure.py textured [TREE]      TREE: the checkout whose library is measured (default: this one)
    python profiles/bump/measure.py bump [OUT.json]      (default: profiles/bump/bump_cost.json)"""
import json, os, sys, time
HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
mode = sys.argv[1] if len(sys.argv) > 1 else "bump"
ROOT = os.path.abspath(sys.argv[2]) if mode == "textured" and len(sys.argv) > 2 else HERE
sys.path.insert(0, ROOT)
os.chdir(ROOT)
import __graft_entry__ as ge
pt = ge.load_package()


def run_steps(scene, flags, textures, maps, steps=20, warmup=5, batch=64):
    s = pt.Scene(scene.geoms, scene.materials, scene.camera, scene.traceDepth)
    pt.pathtraceInit(s, flags=flags, max_batch=batch)
    try:
        for m, tex in textures.items():
            pt.set_texture(m, tex)
        for m, tex in maps.items():
            pt.set_bump_map(m, tex)
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
        return {"ms_per_step": dt / steps * 1e3, "grays_per_s": rays / dt / 1e9, "rays_per_step": rays / steps, "mean_of_image": float(img.mean() / (it - 1))}
    finally:
        pt.pathtraceFree()


def run_calls(scene, flags, textures, maps, calls=200, warmup=20):
    s = pt.Scene(scene.geoms, scene.materials, scene.camera, scene.traceDepth)
    pt.pathtraceInit(s, flags=flags, max_batch=1)
    try:
        for m, tex in textures.items():
            pt.set_texture(m, tex)
        for m, tex in maps.items():
            pt.set_bump_map(m, tex)
        L = pt.library()
        for it in range(1, warmup + 1):
            L.pt_trace(None, 0, it, None)
        t0 = time.perf_counter()
        for it in range(warmup + 1, warmup + calls + 1):
            if L.pt_trace(None, 0, it, None) != 0:
                raise pt.PtError(L.pt_last_error().decode())
        dt = time.perf_counter() - t0
        return {"ms_per_call": dt / calls * 1e3}
    finally:
        pt.pathtraceFree()


if mode == "textured":
    scene = pt.load_scene(os.path.join(HERE, "scenes", "cornell_textured.txt"))
    r = run_steps(scene, pt.PT_COMPACT | pt.PT_TEXTURES, scene.textures, {})
    r["tree"] = ROOT
    print(json.dumps(r))
else:
    scene = pt.load_scene(os.path.join(HERE, "scenes", "cornell_bumped.txt"))
    F = pt.PT_COMPACT | pt.PT_TEXTURES
    out = {"workload": "800x800 scenes/cornell_bumped.txt, depth 8, PT_COMPACT | PT_TEXTURES with the scene's three bump maps and with none (today's kernels, "
                       "k_iteration per call); steps: 64 iterations per step, 5 warm-up + 20 timed, back to back, one synchronisation; calls: 20 warm-up + 200 "
                       "timed synchronous pt_trace calls, no host image",
           "steps_bumped": [], "steps_plain": [], "calls_bumped": [], "calls_plain": []}
    for k in range(3):
        out["steps_bumped"].append(run_steps(scene, F, {}, scene.bump_maps))
        out["steps_plain"].append(run_steps(scene, F, {}, {}))
    for k in range(3):
        out["calls_bumped"].append(run_calls(scene, F, {}, scene.bump_maps))
        out["calls_plain"].append(run_calls(scene, F, {}, {}))
    med = lambda rows, f: sorted(r[f] for r in rows)[1]
    out["median_ms_per_step"] = {"bumped": med(out["steps_bumped"], "ms_per_step"), "plain": med(out["steps_plain"], "ms_per_step")}
    out["median_ms_per_call"] = {"bumped": med(out["calls_bumped"], "ms_per_call"), "plain": med(out["calls_plain"], "ms_per_call")}
    out["step_cost"] = out["median_ms_per_step"]["bumped"] / out["median_ms_per_step"]["plain"] - 1.0
    out["call_ratio"] = out["median_ms_per_call"]["bumped"] / out["median_ms_per_call"]["plain"]
    print(json.dumps(out, indent=1))
    dest = sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, "profiles", "bump", "bump_cost.json")
    with open(dest, "w") as f:
        json.dump(out, f, indent=1)
