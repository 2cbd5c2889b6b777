"""GPU parity, direct lighting (PT_DIRECT_LIGHT; include/ptmi355.h): with the flag and traceDepth D the
last bounce of a diffuse hit aims a final ray at a sampled light, and the path has D + 1 bounces.  Everything is compared bit
for bit with the numpy model (tests/direct_model.py: the oracle's own stages, the two bounces the flag changes recomputed),
under both launch plans where a plan exists: the two probes, every pipeline that honours the flag, batches, lanes, windows
traced ahead, the stepping interface with its statistics, tiles, an environment map with PT_GLOSSY, the refusals and the
headless host.  A final ray that misses needs a light no ray can hit: a flat emissive cube (one scale 0: two parallelogram
elements, a singular transform) across the open side of the box, under the map."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import __graft_entry__ as ge  # noqa: E402,F401
import direct_model as dm  # noqa: E402
import glossy_model as gm  # noqa: E402
from gpu_common import pt, launch_plan, bits, assert_paths_equal, _resized  # noqa: E402,F401

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 50, 37                                              # 1850 paths: 28 full waves and one of 58
F32 = np.float32
M31 = 2 ** 31 - 1
_cache = {}


def same(got, want, what=""):
    bad = (bits(got) != bits(want)).any(axis=-1)
    assert not bad.any(), "%s: %d of %d differ, first %d" % (what, bad.sum(), bad.size, np.nonzero(bad.reshape(-1))[0][0])


def texels(n=4):
    return np.random.default_rng(1000 * n + 1).uniform(0, 2, (6, n, n, 3)).astype(np.float32)


def two_lamps(pt):
    if "two" not in _cache:
        s = pt.load_scene(os.path.join(ROOT, "scenes", "cornell_two_lamps.txt"))
        _cache["two"] = (s.geoms, s.materials, _resized(s.camera, W, H), s.traceDepth)
    return _cache["two"]


def shell_scene(pt):
    """cornell_two_lamps inside a large emitting ellipsoid: every point of the box is INSIDE one element's primitive."""
    geoms, mats, cam, depth = two_lamps(pt)
    shell = geoms[7:8].copy()
    S = np.diag([40.0, 30.0, 50.0, 1.0])
    S[:3, 3] = (0, 5, 0)
    inv = np.linalg.inv(S)
    shell["transform"][0], shell["inverseTransform"][0], shell["invTranspose"][0] = S.T.astype(F32), inv.T.astype(F32), inv.astype(F32)
    shell["materialid"] = 0
    return np.concatenate([geoms, shell]), mats, cam, depth


# ---- pt_probe_direct_sample ----------------------------------------------------------------------------------------------------
def seeds_at_cdf_entries(table):
    """Engine seeds whose FIRST draw is a given u0 = k / 2^31 (the engine's state after one step is k + 1): k at every cdf entry
    below 1, one below and above it, and one and two float32 steps below and above."""
    inv = pow(48271, -1, M31)
    out = []
    for c in table["cdf"][:-1]:
        k = int(round(float(c) * 2 ** 31))
        step = max(1, int(np.spacing(F32(k))))
        for dk in (0, -1, 1, -step, step, -2 * step, 2 * step):
            s1 = k + dk + 1
            if 1 <= s1 < M31:
                out.append((s1 * inv) % M31)
    return np.array(out, dtype=np.uint32)


def sample_records(pt, po, geoms, mats, n):
    rng = np.random.default_rng(7 * n + len(geoms))
    table = dm.light_elements(np.ascontiguousarray(geoms).view(po.GEOM_DT), np.ascontiguousarray(mats).view(po.MATERIAL_DT))
    crafted = seeds_at_cdf_entries(table)
    seeds = np.concatenate([crafted, rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)])[:n]
    P = (rng.uniform(-4.9, 4.9, (n, 3)) + (0, 5, 0)).astype(F32)
    P[3::9] = (F32(0), F32(9), F32(0)) + rng.uniform(-0.05, 0.05, (len(P[3::9]), 3)).astype(F32)     # inside the cube lamp
    P[5::9] = (F32(2.5), F32(3), F32(1)) + rng.uniform(-0.2, 0.2, (len(P[5::9]), 3)).astype(F32)     # inside the lamp ball
    normals = gm.random_unit(rng, n)                                # any side: back-facing draws end at step 6
    normals[::4] = (0, 1, 0)
    return table, P, normals, seeds


@pytest.mark.parametrize("scene", ["two lamps", "inside a shell"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_sample_probe_equals_the_model(pt, po, n, scene):
    """Both element kinds, P inside and outside the element's primitive, back-facing draws, u0 at and next to every cdf entry."""
    geoms, mats, _, _ = two_lamps(pt) if scene == "two lamps" else shell_scene(pt)
    table, P, normals, seeds = sample_records(pt, po, geoms, mats, n)
    g = np.ascontiguousarray(geoms).view(po.GEOM_DT)
    d, w, e, info = dm.sample(po, g, table, P, normals, gm.probe_states(po, seeds))
    gd, gw, ge_ = pt.probe_direct_sample(geoms, mats, P, normals, seeds)
    assert (ge_ == e).all(), np.nonzero(ge_ != e)[0][:5]
    same(gw[:, None], w[:, None], "weight")
    same(gd, d, "direction")
    assert (gw[~info["ok"]] == 0).all() and (gd[~info["ok"]] == 0).all()
    if n == 257:
        kinds = table["kind"][e]
        assert (kinds == dm.SPHERE).any() and (kinds == dm.CUBE).any() and 0 < info["ok"].mean() < 1
        assert info["inside"].any() and (~info["inside"]).any() and len(np.unique(e)) == len(table)
    if n == 257 and scene == "two lamps":
        # at a cdf entry the draw belongs to the NEXT element (u0 < cdf[e] is strict)
        first = table["cdf"][0]
        k = int(round(float(first) * 2 ** 31))
        s = np.array([((k + 1) * pow(48271, -1, M31)) % M31], dtype=np.uint32)
        assert po.u01_sequence(int(s[0]), 1)[0] == first
        assert pt.probe_direct_sample(geoms, mats, P[:1], normals[:1], s)[2][0] == 1


def test_sample_probe_refusals_and_empty_table(pt):
    geoms, mats, _, _ = two_lamps(pt)
    L = pt.library()
    z3, z1, zi = np.zeros((2, 3), F32), np.zeros(2, F32), np.zeros(2, np.int32)
    sd = np.zeros(2, np.uint32)
    g, m = np.ascontiguousarray(geoms), np.ascontiguousarray(mats)

    def call(gp, ng, mp, nm, P, n, s, count, d, w, e):
        return L.pt_probe_direct_sample(gp, ng, mp, nm, P, n, s, count, d, w, e)

    ok = (g.ctypes.data, len(g), m.ctypes.data, len(m), z3.ctypes.data, z3.ctypes.data, sd.ctypes.data, 2, z3.ctypes.data, z1.ctypes.data, zi.ctypes.data)
    assert call(*ok) == 0
    for k, v in ((7, -1), (7, (1 << 26) + 1), (3, 0), (4, None), (5, None), (6, None), (8, None), (9, None), (10, None), (2, None), (1, -1)):
        bad = list(ok)
        bad[k] = v
        assert call(*bad) == -1, k
    assert call(*(ok[:7] + (0, None, None, None))) == 0                 # count == 0 launches nothing
    dark = mats.copy()
    dark["emittance"] = 0
    d, w, e = pt.probe_direct_sample(geoms, dark, z3, z3, sd)
    assert (d == 0).all() and (w == 0).all() and (e == -1).all()


# ---- pt_probe_shade_scatter_direct ---------------------------------------------------------------------------------------------
def shade_records(pt, po, n, depth, trace_depth, it):
    """(geoms, materials, paths, isects, outside, hit_geom): cornell_two_lamps with a mirror and a glass material appended; hits
    on every material, misses, dead paths; at depth == trace_depth the winner is the target, the other emitter, a wall or nothing."""
    geoms, mats, _, _ = two_lamps(pt)
    extra = np.zeros(2, dtype=pt.MATERIAL_DT)
    extra["color"], extra["spec_color"] = (0.3, 0.4, 0.5), (0.9, 0.8, 0.7)
    extra["hasReflective"][0], extra["hasRefractive"][1], extra["indexOfRefraction"][1] = 1, 1, 1.5
    mats = np.concatenate([mats, extra])
    rng = np.random.default_rng(1000 * depth + n)
    p = np.zeros(n, dtype=pt.PATH_DT)
    x = np.zeros(n, dtype=pt.ISECT_DT)
    p["origin"] = (rng.uniform(-4.5, 4.5, (n, 3)) + (0, 5, 0)).astype(F32)
    p["direction"] = gm.random_unit(rng, n)
    p["color"] = rng.uniform(0.05, 1.0, (n, 3)).astype(F32)
    p["pixelIndex"] = rng.integers(-2 ** 31, 2 ** 31, n, dtype=np.int64).astype(np.int32)
    p["remainingBounces"] = rng.choice(np.array([0, 1, 2, 8], dtype=np.int32), n, p=[0.08, 0.3, 0.3, 0.32])
    x["normal"] = -p["direction"]                                  # faces the ray ...
    x["normal"][::3] = gm.random_unit(rng, len(x[::3]))              # ... or anything
    x["t"] = np.where(rng.random(n) < 0.1, -1.0, rng.uniform(0.5, 6.0, n)).astype(F32)
    x["materialId"] = rng.integers(0, len(mats), n).astype(np.int32)
    outside = (rng.random(n) < 0.5).astype(np.uint8)
    hit = None
    if depth == trace_depth:
        g = np.ascontiguousarray(geoms).view(po.GEOM_DT)
        table = dm.light_elements(g, np.ascontiguousarray(mats).view(po.MATERIAL_DT))
        target = dm.target_geoms(po, table, it, p["pixelIndex"], depth - 1)
        other = np.where(target == 0, 7, 0)
        hit = np.choose(rng.integers(0, 4, n), [target, other, np.full(n, 3), np.full(n, -1)]).astype(np.int32)
        x["t"] = np.where(hit < 0, -1.0, np.abs(x["t"])).astype(F32)
        x["materialId"] = geoms["materialid"][np.maximum(hit, 0)]
        assert all(((hit == v) & (p["remainingBounces"] > 0)).any() for v in (0, 7, 3, -1)) or n < 63
    return geoms, mats, p, x, outside, hit


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_shade_probe_equals_the_model(pt, po, n):
    D = 3
    for it, depth in ((1, D - 2), (3, D - 1), (100000, D - 1), (5, D), (100000, D)):
        geoms, mats, p, x, outside, hit = shade_records(pt, po, n, depth, D, it)
        want = dm.shade_direct(po, it, depth, D, geoms, mats, p, x, outside, hit).view(pt.PATH_DT)
        got = pt.probe_shade_scatter_direct(it, depth, D, geoms, mats, p, x, outside, hit)
        assert_paths_equal(got, want, n)
        live = p["remainingBounces"] > 0
        assert got[~live].tobytes() == p[~live].tobytes()
        if n == 257:
            alive = got["remainingBounces"] > 0
            if depth == D:
                assert not alive.any() and (got["color"][live] != 0).any() and (got["color"][live] == 0).all(axis=1).any()
                scored = live & (got["color"] != 0).any(axis=1)
                assert 0.1 < scored[live].mean() < 0.5             # a quarter are aimed at what they hit
            elif depth == D - 1:
                assert alive.any() and (got["remainingBounces"][alive] == 1).all()
                diffuse = live & (x["t"] > 0) & (x["materialId"] >= 1) & (x["materialId"] <= 3)
                assert (alive <= diffuse).all() and 0 < alive[diffuse].mean() < 1
            else:
                assert (got["remainingBounces"][alive] == 2).all() and alive.any()


def test_shade_probe_refusals(pt):
    geoms, mats, p, x, outside, hit = shade_records(pt, None, 8, 1, 3, 1)
    L = pt.library()
    g, m = np.ascontiguousarray(geoms), np.ascontiguousarray(mats)
    h = np.zeros(8, np.int32)
    ok = [1, 1, 3, g.ctypes.data, len(g), m.ctypes.data, len(m), p.ctypes.data, x.ctypes.data, outside.ctypes.data, h.ctypes.data, 8]
    assert L.pt_probe_shade_scatter_direct(*ok) == 0
    for k, v in ((11, -1), (11, (1 << 26) + 1), (6, 0), (7, None), (8, None), (5, None), (1, -1), (1, 4), (2, 0), (2, 64), (3, None)):
        bad = list(ok)
        bad[k] = v
        assert L.pt_probe_shade_scatter_direct(*bad) == -1, k
    final = list(ok)
    final[1], final[10] = 3, None                                   # the final ray needs hit_geom
    assert L.pt_probe_shade_scatter_direct(*final) == -1
    x2 = x.copy()
    x2["t"][0], x2["materialId"][0] = 1.0, len(m)
    bad = list(ok)
    bad[8] = x2.ctypes.data
    assert L.pt_probe_shade_scatter_direct(*bad) == -1 and b"material" in L.pt_last_error()
    empty = list(ok)
    empty[11] = 0
    assert L.pt_probe_shade_scatter_direct(*empty) == 0


# ---- whole pipelines -----------------------------------------------------------------------------------------------------------
def scene_arrays(pt, scenes, name):
    """(geoms, materials, camera at W x H, depth, triangles, meshes)"""
    if name == "cornell":
        s = scenes["cornell"]
        return s["geoms"], s["materials"], _resized(s["camera"], W, H), s["depth"], None, None
    if name == "two lamps":
        return two_lamps(pt) + (None, None)
    if name == "two lamps depth 1":
        g, m, c, _ = two_lamps(pt)
        return g, m, c, 1, None, None
    if name == "cornell glossy":
        s = pt.load_scene(os.path.join(ROOT, "scenes", "cornell_glossy.txt"))
        return s.geoms, s.materials, _resized(s.camera, W, H), s.traceDepth, None, None
    if name == "many primitives":                                  # 17 primitives: past the own-surface form's 15
        g, m, c, d = two_lamps(pt)
        blocks = [dm.placed(pt.GEOM_DT, dm.CUBE, 2 + (k & 1), (-3 + 3 * (k % 3), 0.3, -3 + 3 * (k // 3)), (0.6, 0.6, 0.6), (0, 15 * k, 0)) for k in range(9)]
        return np.concatenate([g] + blocks), m, c, 4, None, None
    if name == "open lamp":                                        # cornell_glossy with a flat lamp across the open side, facing in
        s = pt.load_scene(os.path.join(ROOT, "scenes", "cornell_glossy.txt"))
        flat = dm.placed(pt.GEOM_DT, dm.CUBE, 0, (0, 5, 4.99), (6, 6, 0), (0, 180, 0))
        return np.concatenate([s.geoms, flat]), s.materials, _resized(s.camera, W, H), s.traceDepth, None, None
    if name == "mesh":                                             # a matte triangle soup in cornell_two_lamps without its ball
        import mesh_cases
        g, m, c, d = two_lamps(pt)
        tris = mesh_cases.soup(pt.TRI_DT, np.random.default_rng(11), n=50)
        keep = np.concatenate([g[:6], g[7:8]])
        geoms, tris, meshes = pt.meshes.add_mesh(keep, tris, material_id=1)
        return geoms, m, c, 4, tris, meshes
    if name == "mesh light only":                                  # the only emitter is a mesh: nothing to sample
        import mesh_cases
        s = scenes["cornell"]
        mats = s["materials"].copy()
        mats["emittance"][0] = 0
        mats["emittance"][4], mats["hasReflective"][4] = 4.0, 0
        tris = mesh_cases.soup(pt.TRI_DT, np.random.default_rng(5), n=30)
        geoms, tris, meshes = pt.meshes.add_mesh(s["geoms"][:6], tris, material_id=4)
        return geoms, mats, _resized(s["camera"], W, H), s["depth"], tris, meshes
    raise KeyError(name)


def reference(pt, po, scenes, name, count, env=False, glossy=False, snapshots=False):
    """The model's running sums after iterations 1 .. count, the live counts of every iteration and (snapshots) the live paths
    after every bounce; computed once per module and never written afterwards."""
    key = (name, count, env, glossy, snapshots)
    if key not in _cache:
        geoms, mats, cam, depth, tris, meshes = scene_arrays(pt, scenes, name)
        m = dm.Model(po, geoms, mats, cam, depth, tris=tris, meshes=meshes, glossy=glossy)
        if env:
            m.set_environment(texels())
        out, live, snaps = [], [], []
        for it in range(1, count + 1):
            per_bounce = [] if snapshots else None
            out.append(m.iterate(it, per_bounce).copy())
            live.append(list(m.live))
            snaps.append(per_bounce)
        for a in out:
            a.setflags(write=False)
        _cache[key] = (out, live, snaps, dict(m.counts))
    return _cache[key]


def session(pt, scenes, name, flags, **kw):
    geoms, mats, cam, depth, tris, meshes = scene_arrays(pt, scenes, name)
    scene = pt.Scene(geoms, mats, cam, depth, triangles=tris, meshes=meshes) if tris is not None else pt.Scene(geoms, mats, cam, depth)
    pt.pathtraceInit(scene, flags=flags | pt.PT_DIRECT_LIGHT, **kw)
    return depth


def check_stats(pt, depth, live):
    st = pt.get_stats()
    assert st.bounces == depth + 1 and list(st.live[:depth + 2]) == live + [0], (st.bounces, list(st.live[:depth + 2]), live)
    assert st.rays == sum(live) and live[depth] > 0


def trace_six_then_four(pt, want, live, depth):
    for it in range(1, 7):
        same(pt.pathtrace(None, 0, it), want[it - 1], "iteration %d" % it)
        check_stats(pt, depth, live[it - 1])
    img = np.zeros((W * H, 3), dtype=np.float32)
    pt.trace_batch(7, 4, img)
    same(img, want[9], "batch of 4")
    same(pt.get_image(W * H), want[9], "device image")
    st = pt.get_stats()
    assert st.bounces == depth + 1 and list(st.live[:depth + 1]) == [sum(l[d] for l in live[6:10]) for d in range(depth + 1)]


PIPELINES = {"compact": lambda pt: pt.PT_COMPACT, "plain": lambda pt: 0, "sort fused": lambda pt: pt.PT_COMPACT | pt.PT_SORT_MATERIAL,
             "bvh": lambda pt: pt.PT_COMPACT | pt.PT_MESH_BVH}


@pytest.mark.parametrize("name, flags", [("cornell", "compact"), ("cornell", "plain"), ("cornell", "sort fused"),
                                         ("two lamps", "compact"), ("two lamps", "plain"), ("two lamps", "sort fused"),
                                         ("mesh", "compact"), ("mesh", "bvh"), ("many primitives", "compact"), ("two lamps depth 1", "compact"),
                                         ("two lamps depth 1", "plain")])
def test_pipelines(pt, po, scenes, launch_plan, name, flags):
    """Six pt_trace calls, then a pt_trace_batch of 4, with the statistics of every call: D + 1 bounces, live[D] = the final rays."""
    want, live, _, counts = reference(pt, po, scenes, name, 10)
    depth = session(pt, scenes, name, PIPELINES[flags](pt), max_batch=4)
    try:
        trace_six_then_four(pt, want, live, depth)
    finally:
        pt.pathtraceFree()
    assert counts["sampled"] > 1000 and 0 < counts["step 6"] < counts["sampled"] and 0 < counts["occluded"] < counts["final rays"]
    if name != "cornell":
        assert counts["sphere"] > 100 and counts["cube"] > 100


def test_glossy_and_environment_together(pt, po, scenes, launch_plan):
    """cornell_glossy under a 4 x 4 map with PT_GLOSSY: the ENV x GLOSSY x DIRECT instantiations, fused and sorted.  The box is
    open towards the camera, so ordinary rays read the map; a final ray never does."""
    want, live, _, counts = reference(pt, po, scenes, "cornell glossy", 10, env=True, glossy=True)
    for flags in (pt.PT_COMPACT, pt.PT_COMPACT | pt.PT_SORT_MATERIAL, 0):
        depth = session(pt, scenes, "cornell glossy", flags | pt.PT_GLOSSY, max_batch=4)
        try:
            pt.set_environment(texels())
            trace_six_then_four(pt, want, live, depth)
        finally:
            pt.pathtraceFree()
    assert counts["hits"] > 1000 and counts["occluded"] > 0 and (bits(want[9]) != 0).any(axis=1).mean() > 0.9


def test_final_rays_that_miss_under_a_map_leave_nothing(pt, po, scenes, launch_plan):
    """PT_GLOSSY and a 4 x 4 map, and a light that cannot be hit: the final rays aimed at the flat lamp across the open side leave
    the scene.  They end with colour 0 -- the map is not sampled -- while ordinary rays that leave read it."""
    want, live, _, counts = reference(pt, po, scenes, "open lamp", 10, env=True, glossy=True)
    assert counts["final missed"] > 100 and counts["final missed"] < counts["final rays"] and counts["occluded"] >= counts["final missed"]
    assert len(pt.light_elements(*scene_arrays(pt, scenes, "open lamp")[:2])) == 6 + 2
    for flags in (pt.PT_COMPACT, pt.PT_COMPACT | pt.PT_SORT_MATERIAL, 0):
        depth = session(pt, scenes, "open lamp", flags | pt.PT_GLOSSY, max_batch=4)
        try:
            pt.set_environment(texels())
            trace_six_then_four(pt, want, live, depth)
        finally:
            pt.pathtraceFree()


def test_asynchronous_batches_on_lanes(pt, po, scenes, launch_plan):
    want, _, _, _ = reference(pt, po, scenes, "two lamps", 16)
    session(pt, scenes, "two lamps", pt.PT_COMPACT, max_batch=4)
    try:
        for k in range(4):
            pt.trace_batch_async(1 + 4 * k, 4)
        pt.synchronize()
        same(pt.get_image(W * H), want[15])
    finally:
        pt.pathtraceFree()


def test_lookahead_session(pt, po, scenes, launch_plan):
    """PT_LOOKAHEAD | PT_PIN_IMAGE | PT_HOST_SPARSE: eight calls, the host image after every one."""
    want, _, _, _ = reference(pt, po, scenes, "two lamps", 10)
    L = pt.library()
    buf = np.full((W * H, 3), -7.0, dtype=np.float32)
    session(pt, scenes, "two lamps", pt.PT_COMPACT | pt.PT_LOOKAHEAD | pt.PT_PIN_IMAGE | pt.PT_HOST_SPARSE, max_batch=8, pin_image=False)
    try:
        for it in range(1, 9):
            assert L.pt_trace(None, 0, it, buf.ctypes.data) == 0, L.pt_last_error()
            same(buf, want[it - 1], "host image after iteration %d" % it)
        same(pt.get_image(W * H), want[7], "device image")
    finally:
        pt.pathtraceFree()


@pytest.mark.parametrize("name", ["two lamps", "two lamps depth 1"])
def test_stepping_interface(pt, po, scenes, launch_plan, name):
    """pt_trace_begin / pt_trace_bounce through bounce D with pt_export_paths after every bounce: the pool is the model's live
    paths, in order -- after bounce D - 1 the final rays -- and pt_get_stats reports D + 1 bounces."""
    want, live, snaps, _ = reference(pt, po, scenes, name, 2, snapshots=True)
    depth = session(pt, scenes, name, pt.PT_COMPACT, max_batch=2)
    try:
        for it in (1, 2):
            pt.trace_begin(it, 1)
            for d in range(depth + 1):
                n_live = pt.trace_bounce(d)
                paths, n = pt.export_paths(W * H)
                ref = snaps[it - 1][d]
                assert n_live == n == len(ref), (it, d, n_live, n, len(ref))
                assert_paths_equal(paths, ref, n)
                if d == depth - 1:
                    assert n == live[it - 1][depth] > 0 and (paths["remainingBounces"][:n] == 1).all()
            with pytest.raises(pt.PtError):
                pt.trace_bounce(depth + 1)
            pt.trace_end()
            check_stats(pt, depth, live[it - 1])
            same(pt.get_image(W * H), want[it - 1], "iteration %d" % it)
    finally:
        pt.pathtraceFree()


@pytest.mark.parametrize("form", ["devices", "tile"])
def test_tiles_and_devices(pt, po, scenes, launch_plan, form):
    """A session over two contexts (devices=[0, 0]) delivers the frame; a session that is tile 1 of 2 (strips of 8 rows) its
    own rows, zeros elsewhere."""
    want, _, _, _ = reference(pt, po, scenes, "two lamps", 10)
    kw = dict(devices=[0, 0]) if form == "devices" else dict(tile=(1, 2, 8))
    own = np.ones(H, dtype=bool) if form == "devices" else (np.arange(H) // 8) % 2 == 1
    mask = np.repeat(own, W)

    def expect(a):
        return np.where(mask[:, None], a, np.float32(0))

    session(pt, scenes, "two lamps", pt.PT_COMPACT, max_batch=4, **kw)
    try:
        for it in (1, 2, 3):
            same(pt.pathtrace(None, 0, it), expect(want[it - 1]), "iteration %d" % it)
        img = np.zeros((W * H, 3), dtype=np.float32)
        pt.trace_batch(4, 4, img)
        same(img, expect(want[6]), "batch")
    finally:
        pt.pathtraceFree()


# ---- the flag ------------------------------------------------------------------------------------------------------------------
def test_a_scene_without_cube_or_sphere_lights_is_the_plain_oracle(pt, po, scenes, launch_plan):
    geoms, mats, cam, depth, tris, meshes = scene_arrays(pt, scenes, "mesh light only")
    oracle = po.Tracer(np.ascontiguousarray(geoms).view(po.GEOM_DT), np.ascontiguousarray(mats).view(po.MATERIAL_DT), cam, depth,
                       flags=po.F_COMPACT, trig=po.TRIG_SHARED, tris=np.ascontiguousarray(tris).view(po.TRI_DT),
                       meshes=np.ascontiguousarray(meshes).view(po.MESH_DT))
    assert len(pt.light_elements(geoms, mats)) == 0
    session(pt, scenes, "mesh light only", pt.PT_COMPACT, max_batch=4)
    try:
        for it in range(1, 4):
            st = oracle.iterate(it)
            same(pt.pathtrace(None, 0, it), oracle.image, "iteration %d" % it)
            gs = pt.get_stats()
            assert gs.bounces == st.bounces <= depth and list(gs.live[:depth + 1]) == list(st.live[:depth]) + [0]
        oracle.iterate_parallel(4, 4, 4)
        pt.trace_batch(4, 4)
        same(pt.get_image(W * H), oracle.image, "batch")
        assert (oracle.image != 0).any()
    finally:
        pt.pathtraceFree()


def test_the_flag_changes_the_picture_and_nothing_without_it(pt, po, scenes, launch_plan):
    """cornell_two_lamps without the flag is the plain oracle's image; with it, depth 1 shows the directly lit scene."""
    geoms, mats, cam, depth, _, _ = scene_arrays(pt, scenes, "two lamps")
    oracle = po.Tracer(np.ascontiguousarray(geoms).view(po.GEOM_DT), np.ascontiguousarray(mats).view(po.MATERIAL_DT), cam, depth,
                       flags=po.F_COMPACT, trig=po.TRIG_SHARED)
    pt.pathtraceInit(pt.Scene(geoms, mats, cam, depth), flags=pt.PT_COMPACT, max_batch=4)
    try:
        for it in range(1, 4):
            oracle.iterate(it)
            same(pt.pathtrace(None, 0, it), oracle.image, "iteration %d" % it)
    finally:
        pt.pathtraceFree()
    lit, _, _, _ = reference(pt, po, scenes, "two lamps depth 1", 10)
    plain1 = po.Tracer(np.ascontiguousarray(geoms).view(po.GEOM_DT), np.ascontiguousarray(mats).view(po.MATERIAL_DT), cam, 1,
                       flags=po.F_COMPACT, trig=po.TRIG_SHARED)
    plain1.iterate_parallel(1, 10, 4)
    assert ((plain1.image != 0).any(axis=1)).mean() < 0.1 < 0.5 < ((lit[9] != 0).any(axis=1)).mean()


def test_refusals(pt, scenes):
    geoms, mats, cam, depth, _, _ = scene_arrays(pt, scenes, "two lamps")
    D = pt.PT_DIRECT_LIGHT

    def refused(flags, d=depth, g=geoms, m=mats, word=None):
        with pytest.raises(pt.PtError) as e:
            try:
                pt.pathtraceInit(pt.Scene(g, m, cam, d), flags=flags)
            finally:
                pt.pathtraceFree()
        assert word is None or word in str(e.value), str(e.value)

    refused(D | pt.PT_UNFUSED, word="PT_UNFUSED")
    refused(D | pt.PT_COMPACT | pt.PT_CACHE_FIRST, word="PT_CACHE_FIRST")
    refused(D | pt.PT_SORT_MATERIAL, word="two-kernel")             # no compaction: the two-kernel form
    refused(D | pt.PT_COMPACT, d=64, word="trace_depth")
    many = np.concatenate([geoms[:1]] * 171 + [geoms[1:]])           # 171 cube lamps: 1026 elements
    refused(D | pt.PT_COMPACT, g=many, word="light elements")
    pt.pathtraceInit(pt.Scene(geoms, mats, cam, 63), flags=D | pt.PT_COMPACT)
    try:
        with pytest.raises(pt.PtError):
            pt.set_camera(cam, 64)
        pt.set_camera(cam, 2)
        assert pt.library().pt_trace(None, 0, 1, None) == 0          # (pt.pathtrace would hand the scene's depth over again)
        assert pt.get_stats().bounces == 3
    finally:
        pt.pathtraceFree()
    pt.pathtraceInit(pt.Scene(geoms, mats, cam, 64), flags=pt.PT_COMPACT)   # without the flag depth 64 stays legal
    pt.pathtraceFree()


def test_fake_shader_ignores_the_flag(pt, scenes, launch_plan):
    geoms, mats, cam, depth, _, _ = scene_arrays(pt, scenes, "two lamps")
    imgs = []
    for direct in (0, pt.PT_DIRECT_LIGHT):
        pt.pathtraceInit(pt.Scene(geoms, mats, cam, depth), flags=pt.PT_FAKE_SHADER | direct)
        try:
            pt.pathtrace(None, 0, 1)
            imgs.append(pt.pathtrace(None, 0, 2).copy())
            assert pt.get_stats().bounces == 1
        finally:
            pt.pathtraceFree()
    assert imgs[0].tobytes() == imgs[1].tobytes() and (imgs[0] != 0).any()


# ---- the headless host ---------------------------------------------------------------------------------------------------------
def test_ptbench_direct(pt, po, tmp_path):
    """ptbench --direct renders scenes/cornell_two_lamps.txt (here at 48 x 48, depth 3): the raw running sum it saves is the
    model's; without the switch, the plain model's."""
    w = h = 48
    iters = 4
    txt = open(os.path.join(ROOT, "scenes", "cornell_two_lamps.txt")).read()
    assert "RES         800 800" in txt and "DEPTH       8" in txt
    scene_file = tmp_path / "cornell_two_lamps.txt"
    scene_file.write_text(txt.replace("RES         800 800", "RES         %d %d" % (w, h)).replace("DEPTH       8", "DEPTH       3"))
    s = pt.load_scene(str(scene_file))
    assert s.traceDepth == 3
    for switch in (["--direct"], []):
        out = tmp_path / ("direct%d" % len(switch))
        p = subprocess.run([pt.build_ptbench(), str(scene_file), "--iters", str(iters), "--save-sum", "--out", str(out)] + switch,
                           capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout + p.stderr
        got = pt.load_pfm(str(out) + ".%dsamp.sum.pfm" % iters, w, h)
        m = dm.Model(po, s.geoms, s.materials, s.camera, s.traceDepth, direct=bool(switch))
        for it in range(1, iters + 1):
            m.iterate(it)
        same(got, m.image, "ptbench %s" % " ".join(switch))
        assert (m.counts.get("sampled", 0) > 0) == bool(switch)
