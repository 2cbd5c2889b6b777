"""DESIGN.md section 6.26, the cost with normals (reported, not gated): C4's steps -- Cornell with the 100 032-triangle UV sphere at
800 x 800, depth 8, PT_COMPACT | PT_MESH_BVH | PT_SMOOTH_NORMALS -- with meshes.uv_sphere's analytic normals and with none (today's
kernels), and scenes/cornell_smooth.txt at 800 x 800 through the loop over every triangle and through the hierarchy, with the file's
normals and with none; alternating, three runs each; 16 iterations per step, 3 warm-up + 10 timed steps back to back, one
synchronisation.
    python profiles/smooth/measure.py [OUT.json]      (default: profiles/smooth/smooth_cost.json)"""
import json, os, sys, time
HERE = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, HERE)
os.chdir(HERE)
import __graft_entry__ as ge
pt = ge.load_package()


def run_steps(scene, flags, normals, steps=10, warmup=3, batch=16):
    s = pt.Scene(scene.geoms, scene.materials, scene.camera, scene.traceDepth, triangles=scene.triangles, meshes=scene.meshes)
    pt.pathtraceInit(s, flags=flags | pt.PT_SMOOTH_NORMALS, max_batch=batch)
    try:
        if normals is not None:
            pt.set_vertex_normals(normals)
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


def c4_scene():
    """bench.py's C4: scenes/cornell.txt plus meshes.uv_sphere's 100 032 triangles of material 1"""
    base = pt.load_scene(os.path.join(HERE, "scenes", "cornell.txt"))
    tris, vn = pt.meshes.uv_sphere(n_lat=97, n_lon=521, normals=True)
    geoms, tris, meshes = pt.meshes.add_mesh(base.geoms, tris, material_id=1)
    return pt.Scene(geoms, base.materials, base.camera, base.traceDepth, triangles=tris, meshes=meshes), vn


med = lambda rows: sorted(r["ms_per_step"] for r in rows)[1]
out = {"workload": "800 x 800, depth 8, 16 iterations per step, 3 warm-up + 10 timed steps back to back, one synchronisation; PT_SMOOTH_NORMALS sessions "
                   "with normals set (the SMOOTH forms) and with none (today's kernels), alternating, three runs each"}
c4, c4n = c4_scene()
smooth = pt.load_scene(os.path.join(HERE, "scenes", "cornell_smooth.txt"))
for name, scene, vn, flags in (("c4 bvh", c4, c4n, pt.PT_COMPACT | pt.PT_MESH_BVH), ("cornell_smooth bvh", smooth, smooth.vertex_normals, pt.PT_COMPACT | pt.PT_MESH_BVH),
                               ("cornell_smooth loop", smooth, smooth.vertex_normals, pt.PT_COMPACT)):
    rows = {"smooth": [], "faceted": []}
    for k in range(3):
        rows["smooth"].append(run_steps(scene, flags, vn))
        rows["faceted"].append(run_steps(scene, flags, None))
    out[name] = dict(rows, median_ms_per_step={k: med(v) for k, v in rows.items()}, step_cost=med(rows["smooth"]) / med(rows["faceted"]) - 1.0)
print(json.dumps({k: (v if isinstance(v, str) else {"median_ms_per_step": v["median_ms_per_step"], "step_cost": v["step_cost"]}) for k, v in out.items()}, indent=1))
dest = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "profiles", "smooth", "smooth_cost.json")
with open(dest, "w") as f:
    json.dump(out, f, indent=1)
