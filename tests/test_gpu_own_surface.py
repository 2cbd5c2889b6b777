"""GPU parity, own-surface early miss once per ray: between two bounces of the fused compacting k_bounce a survivor's pid
carries the primitive it has just left (bits 26..29, geom + 1), and the next bounce evaluates the exact one-axis early
miss against that primitive's row once per ray instead of once per primitive (csrc/pt_k_intersect.hpp: cull_scene<.., OWN>,
csrc/pt_k_scene.hpp: own_surface_miss).  The cull only decides which exact tests run, so nothing
observable may change: live counts, pool order, every exported path (pixelIndex without stray bits), final colours and
images stay bit-identical to the oracle -- on C2, with rotated cubes (general rows), glass cubes (origins inside their own
primitive), walls that overlap in the corners, scenes at and beyond the code space (the plan falls back), 64-sample and
stepped batches, PT_LOOKAHEAD windows, and across sessions of pipelines that never see the bits.

Mutation note (done once by hand, not committed): a build that pairs the row of one primitive with the ring entry of
another (own_surface_miss building its key from `own` instead of `own - 1`) fails this file at bounce 1 of the first
iteration; one that merely records another primitive does not, and must not -- the row test is exact for whichever
primitive's row it reads.  HISTORY.md ("Own-surface early miss once per ray") has both.

The plan's fallback by PATH COUNT (batches beyond 2^26 paths) is pinned on the CPU through pt_probe_own_surface_plan
(tests/test_own_surface_cpu.py); here test_code_space asks the same probe about the primitive count."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import __graft_entry__ as ge  # noqa: E402,F401
from gpu_common import pt, launch_plan, bits, assert_paths_equal, _after, _resized  # noqa: E402,F401

pytestmark = pytest.mark.gpu

OWN_MAX_GEOMS = 15          # csrc/pt_types.hpp: codes 1..15 in four bits of the pid


def _pixels(s):
    return int(s["camera"]["resolution"][0][0]) * int(s["camera"]["resolution"][0][1])


def _stepped_iterations(pt, po, s, flags, iterations):
    """Step every bounce of one-sample batches, export after each one and hold the pool against the oracle's snapshot
    (the exported pixelIndex sequence included: a stray bit of the pid would move it); then the live counts and the image."""
    n = _pixels(s)
    oflags = (po.F_COMPACT if flags & pt.PT_COMPACT else 0) | (po.F_SORT if flags & pt.PT_SORT_MATERIAL else 0)
    ref = po.Tracer(s["geoms"].view(po.GEOM_DT), s["materials"], s["camera"], s["depth"], flags=oflags, trig=po.TRIG_SHARED)
    for it in iterations:
        snaps = []
        st = ref.iterate(it, snapshots=snaps)
        pt.trace_begin(it, 1)
        for snap in snaps:
            d = snap["depth"]
            n_live = pt.trace_bounce(d)
            paths, live = pt.export_paths(n)
            if flags & pt.PT_COMPACT:
                assert n_live == snap["n_live"] == live, (it, d)
                assert ((paths["pixelIndex"][:live] >= 0) & (paths["pixelIndex"][:live] < n)).all(), (it, d)
                assert_paths_equal(paths, _after(snaps, d, ref), live)
            else:
                alive = paths["pixelIndex"] >= 0
                wp = _after(snaps, d, ref)
                assert (alive == (wp["remainingBounces"] > 0)[:len(alive)]).all()
                assert_paths_equal(paths[alive], wp[:len(alive)][alive], int(alive.sum()))
        for d in range(len(snaps), s["depth"]):
            pt.trace_bounce(d)
        pt.trace_end()
        gs = pt.get_stats()
        assert list(gs.live[:s["depth"]]) == list(st.live[:s["depth"]]), it
        assert gs.rays == st.rays
        assert pt.get_image(n).tobytes() == ref.image.tobytes(), it


def _batch(pt, po, s, iter0, count, max_batch=None):
    """One batch of `count` samples in a session of its own: rays traced and the image."""
    n = _pixels(s)
    pt.pathtraceInit(pt.Scene(s["geoms"], s["materials"], s["camera"], s["depth"]), flags=pt.PT_COMPACT, max_batch=max_batch or count)
    try:
        ref = po.Tracer(s["geoms"].view(po.GEOM_DT), s["materials"], s["camera"], s["depth"], flags=po.F_COMPACT, trig=po.TRIG_SHARED)
        pt.trace_batch(iter0, count)
        rays = ref.iterate_parallel(iter0, count, min(count, 8))
        assert pt.get_stats().rays == rays
        assert (bits(pt.get_image(n)) == bits(ref.image)).all()
    finally:
        pt.pathtraceFree()


def _geoms(pt, rows):
    """rows: (type, materialid, translation, rotation, scale); matrices by the host library's loader code."""
    H = pt.host_binding.host_library()
    g = np.zeros(len(rows), dtype=pt.GEOM_DT)
    for k, (ty, mat, tr, rot, sc) in enumerate(rows):
        g[k]["type"], g[k]["materialid"] = ty, mat
        g[k]["translation"], g[k]["rotation"], g[k]["scale"] = tr, rot, sc
        H.pth_build_geom_matrices(g.ctypes.data + k * pt.GEOM_DT.itemsize)
    return g


CUBE, SPHERE = 1, 0
# materials of cornell_glass_64: 0 light, 1 white, 2 red, 3 green, 4 mirror, 5 glass
ROOM = [(CUBE, 0, (0, 10, 0), (0, 0, 0), (3, 0.3, 3)), (CUBE, 1, (0, 0, 0), (0, 0, 0), (10, 0.01, 10)),
        (CUBE, 1, (0, 10, 0), (0, 0, 90), (0.01, 10, 10)), (CUBE, 1, (0, 5, -5), (0, 90, 0), (0.01, 10, 10)),
        (CUBE, 2, (-5, 5, 0), (0, 0, 0), (0.01, 10, 10)), (CUBE, 3, (5, 5, 0), (0, 0, 0), (0.01, 10, 10))]


def _scene(pt, scenes, rows, w=48, h=48, depth=8):
    base = scenes["cornell_glass_64"]
    return {"geoms": _geoms(pt, rows), "materials": base["materials"], "camera": _resized(base["camera"], w, h), "depth": depth}


def _rotated_scene(pt, scenes):
    """A diffuse cube turned about y (its largest rows are general ones: reject mode 4) that paths leave and come back to
    from the walls and from its neighbours, a turned glass cube (paths travel inside their own primitive: the row test must
    not fire there, and fires when they have left), a turned mirror slab and a glass ball."""
    return _scene(pt, scenes, ROOM + [(CUBE, 1, (-2.2, 2.0, -1.0), (0, 30, 0), (2.0, 4.0, 2.0)),
                                      (CUBE, 5, (1.6, 2.2, 0.5), (20, 40, 10), (2.5, 2.5, 2.5)),
                                      (CUBE, 4, (0.0, 6.5, -3.0), (35, 0, 45), (4.0, 0.2, 3.0)),
                                      (SPHERE, 5, (2.5, 6.0, -1.5), (0, 0, 0), (2.5, 2.5, 2.5))])


def _crowded_scene(pt, scenes, ngeoms):
    rows = list(ROOM)
    rng = np.random.default_rng(5)
    for k in range(ngeoms - len(ROOM)):
        ty = SPHERE if k % 3 == 1 else CUBE
        rows.append((ty, (1, 4, 5, 2, 3)[k % 5], (-3.5 + 1.75 * (k % 5), 1.2 + 2.4 * (k // 5), -2.0 + 1.5 * (k % 3)),
                     tuple(rng.uniform(-60, 60, 3)) if k % 2 else (0, 0, 0), tuple(rng.uniform(0.8, 1.6, 3))))
    return _scene(pt, scenes, rows, 32, 32)


def _corner_scene(pt, scenes):
    """A small room of THICK walls that run through each other at every edge and corner, the light sunk into the ceiling:
    a path that leaves one wall near an edge starts inside the padded (and the exact) box of its neighbour."""
    t = 1.0
    rows = [(CUBE, 0, (0, 7.4, 0), (0, 0, 0), (4, 1.0, 4)),
            (CUBE, 1, (0, -0.5, 0), (0, 0, 0), (9, t, 9)), (CUBE, 1, (0, 7.5, 0), (0, 0, 0), (9, t, 9)),
            (CUBE, 1, (0, 3.5, -3.5), (0, 0, 0), (9, 9, t)), (CUBE, 2, (-3.5, 3.5, 0), (0, 0, 0), (t, 9, 9)),
            (CUBE, 3, (3.5, 3.5, 0), (0, 0, 0), (t, 9, 9)), (CUBE, 4, (3.0, 0.5, -3.0), (0, 45, 0), (2, 2, 2)),
            (CUBE, 1, (-3.0, 0.4, -3.0), (0, 0, 0), (1.5, 1.5, 1.5))]
    s = _scene(pt, scenes, rows, 48, 48)
    cam = s["camera"].copy()
    cam["position"][0] = (0.0, 3.5, 6.0)
    cam["lookAt"][0] = (0.0, 3.5, 0.0)
    s["camera"] = cam
    return s


@pytest.mark.parametrize("scene_name", ["cornell", "cornell_glass_64"])
@pytest.mark.parametrize("flags_name", ["fused", "cache"])
def test_export_after_every_bounce(pt, po, scenes, scene_name, flags_name):
    """C2 and a diffuse + mirror + glass scene: the exported pool after every bounce is the oracle's and its pids carry no
    stray bits, in fused sessions (own-surface form) and first-bounce-cache ones (which keep the per-primitive form)."""
    s = scenes[scene_name]
    flags = {"fused": pt.PT_COMPACT, "cache": pt.PT_COMPACT | pt.PT_CACHE_FIRST}[flags_name]
    pt.pathtraceInit(pt.Scene(s["geoms"], s["materials"], s["camera"], s["depth"]), flags=flags)
    try:
        _stepped_iterations(pt, po, s, flags, (1, 2))
    finally:
        pt.pathtraceFree()


@pytest.mark.parametrize("scene_lds", ["1", "0"])
def test_rotated_and_glass_cubes(pt, po, scenes, monkeypatch, scene_lds):
    """General rows (mode 4) and origins inside the own primitive, the rows gathered from LDS and from global memory."""
    monkeypatch.setenv("PTMI355_SCENE_LDS", scene_lds)
    s = _rotated_scene(pt, scenes)
    rej = pt.cull_boxes(s["geoms"], (0.0, 5.0, 10.5))[2]
    assert rej[6, 0] == 4 and rej[7, 0] == 4 and rej[8, 0] == 4, rej[:, 0]        # the turned cubes have general rows
    pt.pathtraceInit(pt.Scene(s["geoms"], s["materials"], s["camera"], s["depth"]), flags=pt.PT_COMPACT, max_batch=4)
    try:
        _stepped_iterations(pt, po, s, pt.PT_COMPACT, (1, 2, 3))
    finally:
        pt.pathtraceFree()
    _batch(pt, po, s, 4, 16)


@pytest.mark.parametrize("ngeoms", [OWN_MAX_GEOMS - 1, OWN_MAX_GEOMS, OWN_MAX_GEOMS + 1])
def test_code_space(pt, po, scenes, ngeoms):
    """One primitive below the code space, exactly at it (geom 14 travels as code 15) and one beyond (the plan keeps the
    per-primitive form): each equal to the oracle, stepped and as a batch."""
    assert pt.probe_own_surface_plan(32 * 32 * 4, ngeoms) == (ngeoms <= OWN_MAX_GEOMS)
    s = _crowded_scene(pt, scenes, ngeoms)
    assert len(s["geoms"]) == ngeoms
    pt.pathtraceInit(pt.Scene(s["geoms"], s["materials"], s["camera"], s["depth"]), flags=pt.PT_COMPACT, max_batch=4)
    try:
        _stepped_iterations(pt, po, s, pt.PT_COMPACT, (1, 2))
    finally:
        pt.pathtraceFree()
    _batch(pt, po, s, 3, 4)


def test_corner_room(pt, po, scenes):
    """Walls that run through each other: corner paths start inside two boxes and are candidates of the neighbour."""
    s = _corner_scene(pt, scenes)
    pt.pathtraceInit(pt.Scene(s["geoms"], s["materials"], s["camera"], s["depth"]), flags=pt.PT_COMPACT, max_batch=4)
    try:
        _stepped_iterations(pt, po, s, pt.PT_COMPACT, (1, 2))
    finally:
        pt.pathtraceFree()
    _batch(pt, po, s, 3, 8)


@pytest.mark.parametrize("scene_name", ["cornell_64", "cornell_glass_64"])
def test_64_sample_batch(pt, po, scenes, scene_name):
    """One batch of 64 samples per pixel, twice."""
    s = scenes[scene_name]
    n = _pixels(s)
    pt.pathtraceInit(pt.Scene(s["geoms"], s["materials"], s["camera"], s["depth"]), flags=pt.PT_COMPACT, max_batch=64)
    ref = po.Tracer(s["geoms"], s["materials"], s["camera"], s["depth"], flags=po.F_COMPACT, trig=po.TRIG_SHARED)
    for iter0 in (1, 65):
        pt.trace_batch(iter0, 64)
        rays = ref.iterate_parallel(iter0, 64, 8)
        assert pt.get_stats().rays == rays
        assert (bits(pt.get_image(n)) == bits(ref.image)).all(), iter0
    pt.pathtraceFree()


def test_stepped_batch_of_two_samples(pt, po, scenes):
    """A stepped batch whose pool holds two samples (pids up to twice the pixel count beside the primitive's bits)."""
    s = _rotated_scene(pt, scenes)
    n = _pixels(s)
    pt.pathtraceInit(pt.Scene(s["geoms"], s["materials"], s["camera"], s["depth"]), flags=pt.PT_COMPACT, max_batch=2)
    ref = po.Tracer(s["geoms"].view(po.GEOM_DT), s["materials"], s["camera"], s["depth"], flags=po.F_COMPACT, trig=po.TRIG_SHARED)
    pt.trace_begin(3, 2)
    for d in range(s["depth"]):
        pt.trace_bounce(d)
        paths, live = pt.export_paths(2 * n)
        assert len(paths) == live
        assert ((paths["pixelIndex"] >= 0) & (paths["pixelIndex"] < n)).all(), d
    pt.trace_end()
    rays = ref.iterate_parallel(3, 2, 2)
    assert pt.get_stats().rays == rays
    assert (bits(pt.get_image(n)) == bits(ref.image)).all()
    pt.pathtraceFree()


def test_lookahead_windows(pt, po, scenes):
    """PT_LOOKAHEAD: windows of up to eight iterations traced ahead of the calls, the image after every call."""
    s = _rotated_scene(pt, scenes)
    pt.pathtraceInit(pt.Scene(s["geoms"], s["materials"], s["camera"], s["depth"]),
                     flags=pt.PT_COMPACT | pt.PT_LOOKAHEAD, max_batch=8)
    ref = po.Tracer(s["geoms"].view(po.GEOM_DT), s["materials"], s["camera"], s["depth"], flags=po.F_COMPACT, trig=po.TRIG_SHARED)
    for it in range(1, 22):
        img = pt.pathtrace(None, 0, it)
        ref.iterate(it)
        assert (bits(img) == bits(ref.image)).all(), it
    pt.pathtraceFree()


def test_pipeline_switch_between_sessions(pt, po, scenes):
    """Sort on, then off, then the unfused and non-compacting pipelines, a scene with a triangle mesh under both mesh
    modes, the fused pipeline in between and at the end, on one device and on the same pools' memory: the sessions that
    cull per primitive must never see a primitive's bits in a pid, and the fused ones must strip every one."""
    s = _rotated_scene(pt, scenes)
    scene = pt.Scene(s["geoms"], s["materials"], s["camera"], s["depth"])
    n = _pixels(s)
    tris = pt.meshes.uv_sphere(center=(0.0, 3.0, 1.0), radius=1.2, n_lat=6, n_lon=10)
    mg = np.zeros(1, dtype=pt.GEOM_DT)
    mg["type"], mg["materialid"], mg["scale"] = 2, 4, 1.0
    for k in ("transform", "inverseTransform", "invTranspose"):
        mg[k][0] = np.eye(4, dtype=np.float32)
    mgeoms = np.concatenate([s["geoms"], mg])
    mm = np.zeros(1, dtype=pt.MESH_DT)
    mm["geom_index"], mm["first_triangle"], mm["triangle_count"] = len(mgeoms) - 1, 0, len(tris)
    for flags in (pt.PT_COMPACT | pt.PT_SORT_MATERIAL, pt.PT_COMPACT, pt.PT_COMPACT | pt.PT_SORT_MATERIAL | pt.PT_UNFUSED,
                  pt.PT_COMPACT | pt.PT_UNFUSED, pt.PT_COMPACT, 0, "mesh", "mesh_bvh", pt.PT_COMPACT):
        if isinstance(flags, str):
            mflags = pt.PT_COMPACT | (pt.PT_MESH_BVH if flags == "mesh_bvh" else 0)
            pt.pathtraceInit(pt.Scene(mgeoms, s["materials"], s["camera"], s["depth"], triangles=tris, meshes=mm), flags=mflags, max_batch=4)
            ref = po.Tracer(mgeoms.view(po.GEOM_DT), s["materials"], s["camera"], s["depth"], flags=po.F_COMPACT, trig=po.TRIG_SHARED,
                            tris=tris.view(po.TRI_DT), meshes=mm.view(po.MESH_DT))
            try:
                for it in (1, 2):
                    img = pt.pathtrace(None, 0, it)
                    ref.iterate(it)
                    assert img.tobytes() == ref.image.tobytes(), (flags, it)
                pt.trace_batch(3, 4)
                ref.iterate_parallel(3, 4, 4)
                assert (bits(pt.get_image(n)) == bits(ref.image)).all(), flags
            finally:
                pt.pathtraceFree()
            continue
        pt.pathtraceInit(scene, flags=flags, max_batch=4)
        try:
            _stepped_iterations(pt, po, s, flags, (1,))
            oflags = (po.F_COMPACT if flags & pt.PT_COMPACT else 0) | (po.F_SORT if flags & pt.PT_SORT_MATERIAL else 0)
            ref = po.Tracer(s["geoms"].view(po.GEOM_DT), s["materials"], s["camera"], s["depth"], flags=oflags, trig=po.TRIG_SHARED)
            ref.iterate(1)
            pt.trace_batch(2, 4)                                # a batch behind the stepped iteration, same accumulation buffer
            ref.iterate_parallel(2, 4, 4)
            assert (bits(pt.get_image(n)) == bits(ref.image)).all(), flags
        finally:
            pt.pathtraceFree()
