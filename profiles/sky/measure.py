"""DESIGN.md section 6.24, "cost and gain of the flag" (reported, not gated: there is no parent to hold it against):
scenes/open_sky_sun.txt at 800 x 800 under the sun sky of the tests at 64 texels a side.
* steps: bench.py's timed region (64 iterations per step, steps enqueued back to back, one synchronisation) with PT_DIRECT_LIGHT |
  PT_DIRECT_SKY at depth 3 and at depth 4 and without the flags at depth 4, alternating, three runs each in one process.  Flagged
  depth 3 and plain depth 4 have the same expectation.
* error: the relative L2 distance of the mean of 64 iterations (1 .. 64) of flagged depth 3 and of plain depth 4 to a converged
  picture -- flagged depth 3, iterations 100001 .. 100000 + 64 * 256 --, and what that makes at equal time (the error falls with
  the square root of the time).
* pt_set_environment's host time in a flagged session for maps of 64 and of 1024 texels a side (five calls each: it builds the
  sampling tables and uploads them) and in a session without the flags.
    python profiles/sky/measure.py [OUT.json]       (default: profiles/sky/sky_cost.json)"""
import json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge
import sky_model as sm
pt = ge.load_package()
SKY = pt.PT_DIRECT_LIGHT | pt.PT_DIRECT_SKY


def open_session(scene, flags, depth, texels, batch=64):
    s = pt.Scene(scene.geoms, scene.materials, scene.camera, depth)
    pt.pathtraceInit(s, flags=flags, max_batch=batch)
    pt.set_environment(texels)
    return s


def run_steps(scene, flags, depth, texels, steps=20, warmup=5, batch=64):
    s = open_session(scene, flags, depth, texels, batch)
    try:
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
        return {"ms_per_step": dt / steps * 1e3, "mrays_per_s": rays / dt / 1e6, "rays_per_step": rays / steps,
                "mean_of_image": float(pt.get_image(w * h).mean() / (it - 1))}
    finally:
        pt.pathtraceFree()


def mean_image(scene, flags, depth, texels, first, count, batch=64):
    s = open_session(scene, flags, depth, texels, batch)
    try:
        for k in range(count // batch):
            pt.trace_batch_async(first + k * batch, batch)
        pt.synchronize()
        w, h = s.resolution
        return pt.get_image(w * h).astype(np.float64) / count
    finally:
        pt.pathtraceFree()


def rel_l2(a, b):
    return float(np.sqrt(((a - b) ** 2).sum()) / np.sqrt((b ** 2).sum()))


def set_environment_ms(scene, flags, texels, calls=5):
    s = pt.Scene(scene.geoms, scene.materials, scene.camera, 3)
    pt.pathtraceInit(s, flags=flags, max_batch=4)
    try:
        out = []
        for _ in range(calls):
            t0 = time.perf_counter()
            pt.set_environment(texels)
            out.append((time.perf_counter() - t0) * 1e3)
        return out
    finally:
        pt.pathtraceFree()


scene = pt.load_scene(os.path.join(ROOT, "scenes", "open_sky_sun.txt"))
texels = sm.sun_sky(pt, 64)
out = {"workload": "800x800 scenes/open_sky_sun.txt under tests/sky_model.py's sun sky at 64 texels a side; steps: 64 iterations per step, "
                   "5 warm-up + 20 timed, back to back, one synchronisation"}
for key in ("steps_sky_depth3", "steps_sky_depth4", "steps_plain_depth4"):
    out[key] = []
for k in range(3):
    out["steps_sky_depth3"].append(run_steps(scene, pt.PT_COMPACT | SKY, 3, texels))
    out["steps_sky_depth4"].append(run_steps(scene, pt.PT_COMPACT | SKY, 4, texels))
    out["steps_plain_depth4"].append(run_steps(scene, pt.PT_COMPACT, 4, texels))
med = lambda rows, f: sorted(r[f] for r in rows)[1]
out["median_ms_per_step"] = {k: med(out[k], "ms_per_step") for k in ("steps_sky_depth3", "steps_sky_depth4", "steps_plain_depth4")}
conv = mean_image(scene, pt.PT_COMPACT | SKY, 3, texels, 100001, 64 * 256)
e_sky = rel_l2(mean_image(scene, pt.PT_COMPACT | SKY, 3, texels, 1, 64), conv)
e_plain = rel_l2(mean_image(scene, pt.PT_COMPACT, 4, texels, 1, 64), conv)
t_sky, t_plain = out["median_ms_per_step"]["steps_sky_depth3"], out["median_ms_per_step"]["steps_plain_depth4"]
out["rel_l2_after_64_iterations"] = {"sky_depth3": e_sky, "plain_depth4": e_plain, "converged": "flagged depth 3, 16384 iterations from 100001"}
# error ~ 1 / sqrt(time): the plain session's error after the time the flagged one takes for its 64 iterations
out["rel_l2_at_equal_time"] = {"sky_depth3": e_sky, "plain_depth4": e_plain * (t_plain / t_sky) ** 0.5, "ms": t_sky}
out["time_to_equal_error_plain_over_sky"] = (e_plain / e_sky) ** 2 * t_plain / t_sky
out["set_environment_ms"] = {"flagged_n64": set_environment_ms(scene, pt.PT_COMPACT | SKY, texels),
                             "flagged_n1024": set_environment_ms(scene, pt.PT_COMPACT | SKY, sm.sun_sky(pt, 1024)),
                             "plain_n64": set_environment_ms(scene, pt.PT_COMPACT, texels),
                             "plain_n1024": set_environment_ms(scene, pt.PT_COMPACT, sm.sun_sky(pt, 1024))}
print(json.dumps(out, indent=1))
dest = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "sky", "sky_cost.json")
with open(dest, "w") as f:
    json.dump(out, f, indent=1)
