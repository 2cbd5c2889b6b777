"""GPU parity, smooth shading of triangle meshes (PT_SMOOTH_NORMALS; include/ptmi355.h): per-vertex normals
replace a mesh triangle's facet normal in the shader.  Everything is compared bit for bit with the numpy model
(tests/smooth_model.py), under both launch plans: the probe, every pipeline that honours the flag, batches on the lanes, normals
set, removed and set again in the middle of a window traced ahead, the stepping interface, a tile, two contexts, the furnace, the
G-buffer and the albedo, the refusals and the headless host.  Frames of 40 x 26 and 130 x 9, meshes of 12 to 640 triangles, at most
4 iterations."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import __graft_entry__ as ge  # noqa: E402,F401
import smooth_cases as cases  # noqa: E402
import smooth_model as sm  # noqa: E402
from gpu_common import pt, launch_plan, bits, assert_paths_equal, _resized  # noqa: E402,F401

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
_cache = {}


def same(got, want, what=""):
    bad = (bits(got) != bits(want)).any(axis=-1)
    assert not bad.any(), "%s: %d of %d differ, first %d" % (what, bad.sum(), bad.size, np.nonzero(bad.reshape(-1))[0][0])


# ---- the probe -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_probe_smooth_normal_equals_the_model(pt, n):
    tris, vn, k, o, d = cases.hostile_records(pt, n)
    got = pt.probe_smooth_normal(tris, vn, k, o, d)
    want = sm.smooth_normal(tris, vn, k, o, d)
    assert (got[1] == want[1]).all(), np.nonzero(got[1] != want[1])[0][:5]
    same(got[0], want[0], "n = %d" % n)
    host = pt.smooth_normal(tris, vn, k, o, d)
    assert (host[1] == got[1]).all()
    same(host[0], got[0], "the host entry point")
    if n == 257:
        assert got[1].sum() > 40 and (~got[1]).sum() > 60
        waves = got[1][:256].reshape(4, 64)
        assert (waves.any(axis=1) & ~waves.all(axis=1)).all()            # smoothed and faceted lanes in every wave
    zero = pt.probe_smooth_normal(tris, np.zeros_like(vn), k, o, d)
    assert not zero[1].any()
    same(zero[0], sm.facet_normals(tris)[k], "all-zero normals")
    assert pt.probe_smooth_normal(tris, vn, k[:0], o[:0], d[:0])[0].shape == (0, 3)


# ---- whole pipelines -------------------------------------------------------------------------------------------------------------
def reference(pt, po, name, count=4, env=False, glossy=False, snapshots=False, script=None):
    """The model's running sums after iterations 1 .. count (computed once per module, never written afterwards).  script: {iteration:
    'drop' | 'set'} -- what happens to the normals after that iteration."""
    key = (name, count, env, glossy, snapshots, None if script is None else tuple(sorted(script.items())))
    if key not in _cache:
        geoms, mats, cam, depth, tris, meshes, vn = cases.scene_arrays(pt, name)
        m = sm.Model(po, geoms, mats, cam, depth, tris=tris, meshes=meshes, glossy=glossy)
        m.set_vertex_normals(vn)
        if env:
            m.set_environment(cases.env_texels())
        npix = int(cam["resolution"][0][0]) * int(cam["resolution"][0][1])
        out, snaps, live = [], [], []
        for it in range(1, count + 1):
            per_bounce = []
            out.append(m.iterate(it, per_bounce).copy())
            snaps.append(per_bounce if snapshots else None)
            # the paths traced at bounce d are the live paths that enter it: every pixel at bounce 0, then the survivors of d - 1
            entering = [npix] + [len(p) for p in per_bounce]
            live.append((entering + [0] * depth)[:depth])
            if script and it in script:
                m.set_vertex_normals(None if script[it] == "drop" else vn)
        for a in out:
            a.setflags(write=False)
        _cache[key] = (out, snaps, dict(m.stats, live=live))
    return _cache[key]


def check_counts(pt, stats, iterations, depth):
    """pt_stats of the last call against the model: the paths traced per bounce summed over the call's iterations, their sum, and the
    number of bounces that traced any."""
    live = [sum(stats["live"][it - 1][d] for it in iterations) for d in range(depth)]
    gs = pt.get_stats()
    assert list(gs.live[:depth]) == live, (iterations, list(gs.live[:depth]), live)
    assert gs.rays == sum(live) and gs.bounces == max(d + 1 for d in range(depth) if live[d] > 0)


def session(pt, name, flags, normals=True, **kw):
    geoms, mats, cam, depth, tris, meshes, vn = cases.scene_arrays(pt, name)
    scene = pt.Scene(geoms, mats, cam, depth, triangles=tris, meshes=meshes)
    pt.pathtraceInit(scene, flags=flags | pt.PT_SMOOTH_NORMALS, **kw)
    if normals:
        pt.set_vertex_normals(vn)
    w, h = scene.resolution
    return depth, vn, w * h


def trace_two_then_two(pt, want, npix, stats, depth):
    """Running sums, live counts and ray counts after every call against the model."""
    for it in (1, 2):
        same(pt.pathtrace(None, 0, it), want[it - 1], "iteration %d" % it)
        check_counts(pt, stats, (it,), depth)
    img = np.zeros((npix, 3), dtype=F32)
    pt.trace_batch(3, 2, img)
    same(img, want[3], "batch of 2")
    check_counts(pt, stats, (3, 4), depth)
    same(pt.get_image(npix), want[3], "device image")
    assert pt.counters()[0] == sum(sum(row) for row in stats["live"][:4])        # every ray since pt_init


PIPELINES = {"compact": lambda pt: pt.PT_COMPACT, "plain": lambda pt: 0, "sort fused": lambda pt: pt.PT_COMPACT | pt.PT_SORT_MATERIAL,
             "bvh": lambda pt: pt.PT_COMPACT | pt.PT_MESH_BVH, "bvh plain": lambda pt: pt.PT_MESH_BVH}


@pytest.mark.parametrize("name, flags", [("cornell", "compact"), ("cornell", "plain"), ("cornell", "sort fused"), ("cornell", "bvh"),
                                         ("cornell", "bvh plain"), ("depth 1", "compact"), ("depth 2", "bvh"), ("wide", "compact"),
                                         ("wide", "bvh"), ("hostile", "compact"), ("hostile", "bvh"), ("glass", "compact"),
                                         ("glass", "sort fused"), ("one zero", "compact"), ("one zero", "bvh"),
                                         ("seventeen", "compact"), ("seventeen", "bvh")])
def test_pipelines(pt, po, launch_plan, name, flags):
    """Two pt_trace calls, then a pt_trace_batch of 2."""
    want, _, stats = reference(pt, po, name)
    assert stats["smoothed"] > 50
    depth, _, npix = session(pt, name, PIPELINES[flags](pt), max_batch=2)
    try:
        trace_two_then_two(pt, want, npix, stats, depth)
        # (the normals stay set across the calls)
        assert pt.get_vertex_normals() is not None
    finally:
        pt.pathtraceFree()


def test_glossy_and_environment_together(pt, po, launch_plan):
    """PT_GLOSSY under a 4 x 4 map: the ENV x GLOSSY x SMOOTH instantiations, through the loop, the hierarchy and the fused sort."""
    want, _, stats = reference(pt, po, "glossy", env=True, glossy=True)
    assert stats["smoothed mirror"] > 50
    for flags in (pt.PT_COMPACT, pt.PT_COMPACT | pt.PT_MESH_BVH, pt.PT_COMPACT | pt.PT_SORT_MATERIAL):
        depth, _, npix = session(pt, "glossy", flags | pt.PT_GLOSSY, max_batch=2)
        try:
            pt.set_environment(cases.env_texels())
            trace_two_then_two(pt, want, npix, stats, depth)
        finally:
            pt.pathtraceFree()


def test_asynchronous_batches_on_lanes(pt, po, launch_plan):
    want, _, stats = reference(pt, po, "cornell")
    for flags in (pt.PT_COMPACT, pt.PT_COMPACT | pt.PT_MESH_BVH):
        _, _, npix = session(pt, "cornell", flags, max_batch=2)
        try:
            for k in range(2):
                pt.trace_batch_async(1 + 2 * k, 2)
            pt.synchronize()
            same(pt.get_image(npix), want[3])
            assert pt.counters()[0] == sum(sum(row) for row in stats["live"][:4])      # the rays of both batches
        finally:
            pt.pathtraceFree()


def test_lookahead_window_across_removal_and_return_of_the_normals(pt, po, launch_plan):
    """PT_LOOKAHEAD | PT_PIN_IMAGE | PT_HOST_SPARSE: the normals are removed after the first call and set again after the third --
    both in the middle of a window traced ahead: the host image after every call is the model's."""
    want, _, _ = reference(pt, po, "cornell", script={1: "drop", 3: "set"})
    L = pt.library()
    _, vn, npix = session(pt, "cornell", pt.PT_COMPACT | pt.PT_LOOKAHEAD | pt.PT_PIN_IMAGE | pt.PT_HOST_SPARSE, max_batch=8, pin_image=False)
    buf = np.full((npix, 3), -7.0, dtype=F32)
    try:
        for it in (1, 2, 3, 4):
            assert L.pt_trace(None, 0, it, buf.ctypes.data) == 0, L.pt_last_error()
            same(buf, want[it - 1], "host image after iteration %d" % it)
            if it == 1:
                pt.set_vertex_normals(None)
                assert pt.get_vertex_normals() is None
            if it == 3:
                pt.set_vertex_normals(vn)
        same(pt.get_image(npix), want[3], "device image")
    finally:
        pt.pathtraceFree()


@pytest.mark.parametrize("name, flags", [("cornell", "compact"), ("depth 1", "compact"), ("hostile", "bvh")])
def test_stepping_interface(pt, po, launch_plan, name, flags):
    want, snaps, _ = reference(pt, po, name, 2, snapshots=True)
    depth, _, npix = session(pt, name, PIPELINES[flags](pt), max_batch=2)
    try:
        for it in (1, 2):
            pt.trace_begin(it, 1)
            for d in range(depth):
                n_live = pt.trace_bounce(d)
                paths, n = pt.export_paths(npix)
                ref = snaps[it - 1][d] if d < len(snaps[it - 1]) else snaps[it - 1][-1][:0]
                assert n_live == n == len(ref), (it, d, n_live, n, len(ref))
                assert_paths_equal(paths, ref, n)
            pt.trace_end()
            same(pt.get_image(npix), want[it - 1], "iteration %d" % it)
    finally:
        pt.pathtraceFree()


@pytest.mark.parametrize("form", ["devices", "tile"])
def test_tiles_and_devices(pt, po, launch_plan, form):
    """A session over two contexts (devices=[0, 0]: each with its own copy of the normals) delivers the frame; a session that is tile
    1 of 2 (strips of 8 rows) its own rows, zeros elsewhere."""
    want, _, _ = reference(pt, po, "cornell")
    kw = dict(devices=[0, 0]) if form == "devices" else dict(tile=(1, 2, 8))
    own = np.ones(cases.H, dtype=bool) if form == "devices" else (np.arange(cases.H) // 8) % 2 == 1
    mask = np.repeat(own, cases.W)

    def expect(a):
        return np.where(mask[:, None], a, F32(0))

    _, vn, npix = session(pt, "cornell", pt.PT_COMPACT, max_batch=2, **kw)
    try:
        for it in (1, 2):
            same(pt.pathtrace(None, 0, it), expect(want[it - 1]), "iteration %d" % it)
        img = np.zeros((npix, 3), dtype=F32)
        pt.trace_batch(3, 2, img)
        same(img, expect(want[3]), "batch")
        assert pt.get_vertex_normals().tobytes() == vn.tobytes()
    finally:
        pt.pathtraceFree()


def test_furnace(pt, po, launch_plan):
    """The 320-triangle ball with exact albedo 0.5 under a constant sky of 1, depth 4: a guarded direction leaves a convex body, so
    every pixel whose camera ray hits the ball holds exactly 0.5 * k after k iterations, every other k -- whatever the model says."""
    s = cases.loaded(pt)
    ball = s.meshes[0]
    a, b = int(ball["first_triangle"]), int(ball["first_triangle"]) + int(ball["triangle_count"])
    mats = np.zeros(1, dtype=pt.MATERIAL_DT)
    mats["color"] = 0.5
    geoms, tris, meshes = pt.meshes.add_mesh(np.zeros(0, dtype=pt.GEOM_DT), s.triangles[a:b].copy(), material_id=0)
    cam = s.camera.copy()
    cam["position"][0] = (-2.0, 2.5, 3.0)
    cam["lookAt"][0] = (-2.0, 2.5, 0.0)
    cam["view"][0], cam["up"][0], cam["right"][0] = (0, 0, -1), (0, 1, 0), (1, 0, 0)
    cam = _resized(cam, 24, 24)
    paths = po.generate_rays(cam, 4)
    x, _ = po.compute_intersections(paths, np.ascontiguousarray(geoms).view(po.GEOM_DT), np.ascontiguousarray(tris).view(po.TRI_DT),
                                    np.ascontiguousarray(meshes).view(po.MESH_DT))
    hit = np.zeros(24 * 24, dtype=bool)
    hit[paths["pixelIndex"]] = x["t"] > 0
    assert 60 < hit.sum() < 24 * 24
    for flags in (pt.PT_COMPACT, pt.PT_COMPACT | pt.PT_MESH_BVH):
        pt.pathtraceInit(pt.Scene(geoms, mats, cam, 4, triangles=tris, meshes=meshes), flags=flags, max_batch=4,
                         vertex_normals=s.vertex_normals[a:b])
        try:
            pt.set_environment(np.ones((6, 1, 1, 3), dtype=F32))
            for k in (1, 2, 3, 4):
                img = pt.pathtrace(None, 0, k)
                assert (img[hit] == F32(0.5 * k)).all(), (k, np.unique(img[hit]))
                assert (img[~hit] == F32(k)).all(), k
        finally:
            pt.pathtraceFree()


# ---- what the normals leave alone ----------------------------------------------------------------------------------------------------
def test_no_normals_and_zero_normals_are_the_plain_oracle(pt, po, launch_plan):
    geoms, mats, cam, depth, tris, meshes, vn = cases.scene_arrays(pt, "cornell")
    for flags in (pt.PT_COMPACT, pt.PT_COMPACT | pt.PT_MESH_BVH):
        for zero in (False, True):
            oracle = po.Tracer(np.ascontiguousarray(geoms).view(po.GEOM_DT), np.ascontiguousarray(mats).view(po.MATERIAL_DT), cam, depth,
                               flags=po.F_COMPACT, trig=po.TRIG_SHARED, tris=np.ascontiguousarray(tris).view(po.TRI_DT),
                               meshes=np.ascontiguousarray(meshes).view(po.MESH_DT))
            _, _, npix = session(pt, "cornell", flags, normals=False, max_batch=2)
            try:
                if zero:
                    pt.set_vertex_normals(np.zeros_like(vn))
                for it in (1, 2):
                    st = oracle.iterate(it)
                    same(pt.pathtrace(None, 0, it), oracle.image, "iteration %d" % it)
                    gs = pt.get_stats()
                    assert gs.bounces == st.bounces and list(gs.live[:depth]) == list(st.live[:depth])
                assert (oracle.image != 0).any()
            finally:
                pt.pathtraceFree()


def test_gbuffer_and_albedo_are_unchanged_by_the_normals(pt, launch_plan):
    got = []
    for with_normals in (False, True):
        session(pt, "cornell", pt.PT_COMPACT, normals=with_normals, max_batch=2)
        try:
            pt.pathtrace(None, 0, 1)
            gb = pt.gbuffer()
            alb = pt.albedo()
            got.append([gb[k].tobytes() for k in sorted(gb)] + [alb.tobytes()])
        finally:
            pt.pathtraceFree()
    assert got[0] == got[1]


def test_get_vertex_normals_returns_what_was_set(pt, launch_plan):
    depth, vn, npix = session(pt, "hostile", pt.PT_COMPACT, max_batch=2)
    try:
        geoms, mats, cam, _, _, _, _ = cases.scene_arrays(pt, "hostile")
        pt.pathtrace(None, 0, 1)
        pt.set_camera(cam, depth)
        pt.clear_image()
        got = pt.get_vertex_normals()
        assert got.shape == vn.shape and got.tobytes() == vn.tobytes()   # (NaN and infinities included: bytes, not values)
        L = pt.library()
        small = np.zeros((10, 9), F32)
        n = C.c_int(0)
        assert L.pt_get_vertex_normals(small.ctypes.data, 10, C.byref(n)) < 0 and n.value == len(vn)     # too small: the size is reported
        pt.set_vertex_normals(None)
        assert pt.get_vertex_normals() is None
    finally:
        pt.pathtraceFree()


def test_refusals(pt):
    geoms, mats, cam, depth, tris, meshes, vn = cases.scene_arrays(pt, "cornell")
    L = pt.library()
    scene = pt.Scene(geoms, mats, cam, depth, triangles=tris, meshes=meshes)
    k = C.c_int(0)

    def says(rc, text):                                              # PT_ERR_INVALID and the whole message
        assert rc == -1 and L.pt_last_error() == text.encode(), (rc, L.pt_last_error())

    pt.pathtraceFree()
    with pytest.raises(pt.PtError):                                  # before pt_init
        pt.set_vertex_normals(vn)
    with pytest.raises(pt.PtError):
        pt.get_vertex_normals()
    pt.pathtraceInit(scene, flags=pt.PT_COMPACT)                     # a session without the flag
    try:
        with pytest.raises(pt.PtError):
            pt.set_vertex_normals(vn)
        with pytest.raises(pt.PtError):
            pt.get_vertex_normals()
        says(L.pt_set_vertex_normals(None, -1), "pt_set_vertex_normals: the session was not initialised with PT_SMOOTH_NORMALS")
        says(L.pt_get_vertex_normals(None, 0, None), "pt_get_vertex_normals: the session was not initialised with PT_SMOOTH_NORMALS")
    finally:
        pt.pathtraceFree()
    S = pt.PT_SMOOTH_NORMALS
    many = np.concatenate([mats] * 13)                               # 65 materials: the sort takes its two-kernel form
    for flags, m in ((S | pt.PT_UNFUSED, mats), (S | pt.PT_CACHE_FIRST, mats), (S | pt.PT_COMPACT | pt.PT_TEXTURES, mats),
                     (S | pt.PT_COMPACT | pt.PT_DIRECT_LIGHT, mats), (S | pt.PT_COMPACT | pt.PT_SORT_MATERIAL, many)):
        with pytest.raises(pt.PtError, match="PT_SMOOTH_NORMALS"):
            pt.pathtraceInit(pt.Scene(geoms, m, cam, depth, triangles=tris, meshes=meshes), flags=flags)
        pt.pathtraceFree()
    pt.pathtraceInit(scene, flags=pt.PT_COMPACT | S)
    try:
        assert L.pt_set_vertex_normals(vn.ctypes.data, len(vn) - 1) < 0 and b"the session has" in L.pt_last_error()
        assert L.pt_set_vertex_normals(vn.ctypes.data, len(vn) + 1) < 0
        assert L.pt_set_vertex_normals(vn.ctypes.data, -1) < 0
        assert L.pt_set_vertex_normals(None, len(vn)) < 0 and b"null" in L.pt_last_error()
        assert L.pt_get_vertex_normals(None, 0, None) < 0
        for count in (len(vn) - 1, len(vn) + 1):
            says(L.pt_set_vertex_normals(vn.ctypes.data, count), "pt_set_vertex_normals: %d triangles, the session has %d" % (count, len(vn)))
        says(L.pt_set_vertex_normals(None, -1), "pt_set_vertex_normals: num_triangles = -1")
        says(L.pt_set_vertex_normals(None, len(vn) + 1), "pt_set_vertex_normals: null normals with num_triangles = %d" % (len(vn) + 1))
        says(L.pt_get_vertex_normals(None, 0, None), "pt_get_vertex_normals: null num_triangles")
        assert L.pt_set_vertex_normals(None, 0) == 0 and pt.get_vertex_normals() is None
        assert L.pt_set_vertex_normals(vn.ctypes.data, len(vn)) == 0
        out = np.zeros_like(vn)
        says(L.pt_get_vertex_normals(out.ctypes.data, len(vn) - 1, C.byref(k)),
             "pt_get_vertex_normals: room for %d triangles, the session has %d" % (len(vn) - 1, len(vn)))
        assert k.value == len(vn) and not out.any()
        says(L.pt_get_vertex_normals(None, len(vn), C.byref(k)), "pt_get_vertex_normals: room for 0 triangles, the session has %d" % len(vn))
        assert L.pt_get_vertex_normals(out.ctypes.data, len(vn), C.byref(k)) == 0 and out.tobytes() == vn.tobytes()
    finally:
        pt.pathtraceFree()


def test_fake_shader_ignores_the_normals(pt, launch_plan):
    geoms, mats, cam, depth, tris, meshes, vn = cases.scene_arrays(pt, "cornell")
    imgs = []
    for flag in (0, pt.PT_SMOOTH_NORMALS):
        pt.pathtraceInit(pt.Scene(geoms, mats, cam, depth, triangles=tris, meshes=meshes), flags=pt.PT_FAKE_SHADER | flag)
        try:
            if flag:
                pt.set_vertex_normals(vn)
            pt.pathtrace(None, 0, 1)
            imgs.append(pt.pathtrace(None, 0, 2).copy())
        finally:
            pt.pathtraceFree()
    assert imgs[0].tobytes() == imgs[1].tobytes() and (imgs[0] != 0).any()


# ---- the headless host -------------------------------------------------------------------------------------------------------------
def test_ptbench_smooth(pt, po, tmp_path):
    """ptbench --smooth renders scenes/cornell_smooth.txt (here at 32 x 32, depth 3): the raw running sum it saves is the model's;
    without the switch, the plain model's."""
    w = h = 32
    iters = 4
    txt = open(os.path.join(ROOT, "scenes", "cornell_smooth.txt")).read()
    assert "RES         800 800" in txt and "DEPTH       8" in txt
    scene_file = tmp_path / "cornell_smooth.txt"
    scene_file.write_text(txt.replace("RES         800 800", "RES         %d %d" % (w, h)).replace("DEPTH       8", "DEPTH       3")
                          .replace("mesh ball_320.obj", "mesh " + os.path.join(ROOT, "scenes", "ball_320.obj")))
    s = pt.load_scene(str(scene_file))
    assert s.traceDepth == 3 and s.vertex_normals.shape == (640, 3, 3)
    for switch in (["--smooth"], []):
        out = tmp_path / ("smooth%d" % len(switch))
        p = subprocess.run([pt.build_ptbench(), str(scene_file), "--iters", str(iters), "--save-sum", "--out", str(out)] + switch,
                           capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout + p.stderr
        assert ("vertex normals: 640 of 640 triangles" in p.stdout) == bool(switch)
        got = pt.load_pfm(str(out) + ".%dsamp.sum.pfm" % iters, w, h)
        m = sm.Model(po, s.geoms, s.materials, s.camera, s.traceDepth, tris=s.triangles, meshes=s.meshes)
        if switch:
            m.set_vertex_normals(s.vertex_normals)
        for it in range(1, iters + 1):
            m.iterate(it)
        same(got, m.image, "ptbench %s" % " ".join(switch))
        assert (m.stats.get("smoothed", 0) > 0) == bool(switch)
