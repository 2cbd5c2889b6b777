"""GPU parity, environment lighting (include/ptmi355.h: pt_set_environment): a path whose ray leaves the
scene ends with throughput * E(d), E the nearest texel of a cube map.  Everything is compared bit for bit with the numpy model
(tests/environment_model.py: the oracle's own stages plus the one changed exit), under both launch plans: the probe, every
pipeline, batches, lanes, windows traced ahead, the stepping interface, tiles and several devices."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import __graft_entry__ as ge  # noqa: E402,F401
import environment_model as em  # noqa: E402
from gpu_common import pt, launch_plan, bits, _resized  # noqa: E402,F401
from environment_model import edge_directions, random_directions  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 50, 37                                              # 1850 pixels: not a multiple of 64 or 256
_cache = {}


def texels(n, seed=1):
    return np.random.default_rng(1000 * n + seed).uniform(0, 2, (6, n, n, 3)).astype(np.float32)


def scene_arrays(pt, scenes, name, w=W, h=H):
    """(geoms, materials, camera at w x h, depth)"""
    if name == "open_sky":
        s = pt.load_scene(os.path.join(ROOT, "scenes", "open_sky.txt"))
        return s.geoms, s.materials, _resized(s.camera, w, h), s.traceDepth
    s = scenes[name]
    return s["geoms"], s["materials"], _resized(s["camera"], w, h), s["depth"]


def reference(pt, po, scenes, name, count, aa=False, w=W, h=H, n=4, switch=None):
    """The model's running sums after iterations 1 .. count (computed once per module, never written afterwards).
    switch = (iteration, texels): the map changes before that iteration."""
    key = (name, count, aa, w, h, n, None if switch is None else switch[0])
    if key not in _cache:
        geoms, mats, cam, depth = scene_arrays(pt, scenes, name, w, h)
        m = em.Model(po, geoms, mats, cam, depth, aa=aa)
        m.set_environment(texels(n))
        out = []
        for it in range(1, count + 1):
            if switch is not None and it == switch[0]:
                m.set_environment(switch[1])
            out.append(m.iterate(it).copy())
        for a in out:
            a.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def same(got, want, what=""):
    bad = (bits(got) != bits(want)).any(axis=-1)
    assert not bad.any(), "%s: %d of %d pixels differ, first %d" % (what, bad.sum(), bad.size, np.nonzero(bad.reshape(-1))[0][0])


# ---- the probe ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 4, 64, 1024])
def test_probe_equals_the_model(pt, n):
    rng = np.random.default_rng(n)
    edges, _ = edge_directions()
    d = np.concatenate([random_directions(rng, 4096), edges])
    thr = rng.uniform(-1, 2, (len(d), 3)).astype(np.float32)
    thr[::9] = 0
    t = texels(n)
    got = pt.probe_environment(t, d, thr)
    same(got, em.miss_colour(t, d, thr), "n = %d" % n)
    assert (bits(pt.probe_environment(None, d, thr)) == 0).all()            # no map: +0


@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, 257])
def test_probe_counts(pt, count):
    rng = np.random.default_rng(count)
    d = random_directions(rng, count).reshape(count, 3)
    thr = rng.uniform(0, 1, (count, 3)).astype(np.float32)
    t = texels(4)
    got = pt.probe_environment(t, d, thr)
    assert got.shape == (count, 3)
    same(got, em.miss_colour(t, d, thr))


def test_probe_refusals(pt):
    L = pt.library()
    t, d = texels(1), np.zeros((4, 3), np.float32)
    p = lambda a: a.ctypes.data                                   # noqa: E731
    for args in ((p(t), 1, p(d), p(d), -1, p(d)), (p(t), 1, None, p(d), 4, p(d)), (p(t), 1, p(d), None, 4, p(d)),
                 (p(t), 1, p(d), p(d), 4, None), (None, 1, p(d), p(d), 4, p(d)), (p(t), 1025, p(d), p(d), 4, p(d)),
                 (p(t), -1, p(d), p(d), 4, p(d))):
        assert L.pt_probe_environment(*args) == -1, args
        assert b"pt_probe_environment" in L.pt_last_error()
    assert L.pt_probe_environment(None, 0, None, None, 0, None) == 0


# ---- every pipeline ----------------------------------------------------------------------------------------------------
def flag_sets(pt):
    return {"compact": pt.PT_COMPACT, "plain": 0, "compact+sort": pt.PT_COMPACT | pt.PT_SORT_MATERIAL,
            "unfused": pt.PT_UNFUSED, "unfused+sort": pt.PT_UNFUSED | pt.PT_SORT_MATERIAL,
            "cache+compact": pt.PT_CACHE_FIRST | pt.PT_COMPACT, "aa+compact": pt.PT_AA_JITTER | pt.PT_COMPACT}


@pytest.mark.parametrize("flags", ["compact", "plain", "compact+sort", "unfused", "unfused+sort", "cache+compact", "aa+compact"])
@pytest.mark.parametrize("name", ["cornell", "open_sky"])
def test_pipelines(pt, po, scenes, launch_plan, name, flags):
    """Six pt_trace calls, then a pt_trace_batch of 4."""
    want = reference(pt, po, scenes, name, 10, aa=flags.startswith("aa"))
    geoms, mats, cam, depth = scene_arrays(pt, scenes, name)
    scene = pt.Scene(geoms, mats, cam, depth)
    pt.pathtraceInit(scene, flags=flag_sets(pt)[flags], max_batch=4)
    try:
        pt.set_environment(texels(4))
        for it in range(1, 7):
            same(pt.pathtrace(None, 0, it), want[it - 1], "iteration %d" % it)
        img = np.zeros((W * H, 3), dtype=np.float32)
        pt.trace_batch(7, 4, img)
        same(img, want[9], "batch")
        same(pt.get_image(W * H), want[9], "device image")
    finally:
        pt.pathtraceFree()
    assert (bits(want[9]) != 0).any(axis=1).mean() > 0.9           # a lit picture, not a black one


def test_stepping_interface(pt, po, scenes, launch_plan):
    want = reference(pt, po, scenes, "cornell", 10)
    geoms, mats, cam, depth = scene_arrays(pt, scenes, "cornell")
    pt.pathtraceInit(pt.Scene(geoms, mats, cam, depth), flags=pt.PT_COMPACT, max_batch=2)
    try:
        pt.set_environment(texels(4))
        for it in (1, 2):
            pt.trace_begin(it, 1)
            for d in range(depth):
                pt.trace_bounce(d)
            pt.trace_end()
            same(pt.get_image(W * H), want[it - 1], "iteration %d" % it)
    finally:
        pt.pathtraceFree()


def test_glass_scene(pt, po, scenes, launch_plan):
    """64 x 36, depth 16: refracted paths leave through the map."""
    w, h = 64, 36
    want = reference(pt, po, scenes, "cornell_glass", 5, w=w, h=h)
    geoms, mats, cam, depth = scene_arrays(pt, scenes, "cornell_glass", w, h)
    assert depth == 16
    for flags in (pt.PT_COMPACT, pt.PT_COMPACT | pt.PT_SORT_MATERIAL):
        pt.pathtraceInit(pt.Scene(geoms, mats, cam, depth), flags=flags, max_batch=2)
        try:
            pt.set_environment(texels(4))
            for it in (1, 2, 3):
                same(pt.pathtrace(None, 0, it), want[it - 1], "iteration %d" % it)
            img = np.zeros((w * h, 3), dtype=np.float32)
            pt.trace_batch(4, 2, img)
            same(img, want[4], "batch")
        finally:
            pt.pathtraceFree()


@pytest.mark.parametrize("bvh", [False, True])
def test_mesh_scene(pt, po, scenes, launch_plan, bvh):
    """A triangle soup of tests/mesh_cases.py at its smallest size inside the open box: through the every-triangle loop and
    through the hierarchy and its pre-pass."""
    import mesh_cases
    s = scenes["cornell"]
    cam = _resized(s["camera"], W, H)
    tris = mesh_cases.soup(pt.TRI_DT, np.random.default_rng(11), n=50)
    geoms, tris, meshes = pt.meshes.add_mesh(s["geoms"][:6], tris, material_id=4)
    key = "mesh"
    if key not in _cache:
        m = em.Model(po, geoms, s["materials"], cam, s["depth"], tris=tris, meshes=meshes)
        m.set_environment(texels(4))
        _cache[key] = [m.iterate(it).copy() for it in range(1, 6)]
    want = _cache[key]
    scene = pt.Scene(geoms, s["materials"], cam, s["depth"], triangles=tris, meshes=meshes)
    pt.pathtraceInit(scene, flags=pt.PT_COMPACT | (pt.PT_MESH_BVH if bvh else 0), max_batch=2)
    try:
        pt.set_environment(texels(4))
        for it in (1, 2, 3):
            same(pt.pathtrace(None, 0, it), want[it - 1], "iteration %d" % it)
        img = np.zeros((W * H, 3), dtype=np.float32)
        pt.trace_batch(4, 2, img)
        same(img, want[4], "batch")
    finally:
        pt.pathtraceFree()


# ---- windows traced ahead, lanes, tiles, devices ---------------------------------------------------------------------
@pytest.mark.parametrize("frame", ["50x37 pageable", "352x250 page-locked"])
def test_lookahead_map_changes_inside_a_window(pt, po, scenes, launch_plan, frame):
    """PT_LOOKAHEAD | PT_PIN_IMAGE | PT_HOST_SPARSE, the host image after every call.  20 calls, the map changes after call 9:
    in the middle of the window [5, 12], with [13, 20] already traced ahead.  From iteration 10 on the images are the model's with
    the new map -- nothing traced ahead with the old one is served.  The second frame is above the 1 MiB from which
    PT_PIN_IMAGE page-locks the image and the calls' gathers write it themselves (10 calls, the change after call 6)."""
    w, h, calls, change = (W, H, 20, 10) if frame.startswith("50x37") else (352, 250, 10, 7)
    second = texels(2, seed=7)
    want = reference(pt, po, scenes, "cornell", calls, w=w, h=h, switch=(change, second))
    geoms, mats, cam, depth = scene_arrays(pt, scenes, "cornell", w, h)
    L = pt.library()
    out = (C.c_uint64 * 4)()
    buf = np.full((w * h, 3), -7.0, dtype=np.float32)
    pt.pathtraceInit(pt.Scene(geoms, mats, cam, depth), flags=pt.PT_COMPACT | pt.PT_LOOKAHEAD | pt.PT_PIN_IMAGE | pt.PT_HOST_SPARSE,
                     max_batch=8, pin_image=False)
    try:
        pt.set_environment(texels(4))
        for it in range(1, calls + 1):
            if it == change:
                assert L.ptdbg_lookahead(out) == 0
                discarded = int(out[2])
                pt.set_environment(second)
                assert L.ptdbg_lookahead(out) == 0 and int(out[2]) > discarded       # the windows are void
            assert L.pt_trace(None, 0, it, buf.ctypes.data) == 0, L.pt_last_error()
            same(buf, want[it - 1], "host image after iteration %d" % it)
        same(pt.get_image(w * h), want[calls - 1], "device image")
    finally:
        pt.pathtraceFree()


@pytest.mark.parametrize("form", ["devices", "tile"])
def test_tiles_and_devices(pt, po, scenes, launch_plan, form):
    """A session over two contexts (devices=[0, 0]) delivers the frame; a session that is tile 1 of 2 (strips of 8 rows) its
    own rows, zeros elsewhere."""
    want = reference(pt, po, scenes, "cornell", 10)
    geoms, mats, cam, depth = scene_arrays(pt, scenes, "cornell")
    kw = dict(devices=[0, 0]) if form == "devices" else dict(tile=(1, 2, 8))
    own = np.ones(H, dtype=bool) if form == "devices" else (np.arange(H) // 8) % 2 == 1
    mask = np.repeat(own, W)

    def expect(a):
        return np.where(mask[:, None], a, np.float32(0))

    pt.pathtraceInit(pt.Scene(geoms, mats, cam, depth), flags=pt.PT_COMPACT, max_batch=4, **kw)
    try:
        pt.set_environment(texels(4))
        for it in (1, 2, 3):
            same(pt.pathtrace(None, 0, it), expect(want[it - 1]), "iteration %d" % it)
        img = np.zeros((W * H, 3), dtype=np.float32)
        pt.trace_batch(4, 4, img)
        same(img, expect(want[6]), "batch")
        got = pt.get_environment()
        assert got is not None and got.tobytes() == texels(4).tobytes()
    finally:
        pt.pathtraceFree()


def test_asynchronous_batches_on_lanes(pt, po, scenes, launch_plan):
    want = reference(pt, po, scenes, "cornell", 16)
    geoms, mats, cam, depth = scene_arrays(pt, scenes, "cornell")
    pt.pathtraceInit(pt.Scene(geoms, mats, cam, depth), flags=pt.PT_COMPACT, max_batch=4)
    try:
        pt.set_environment(texels(4))
        for k in range(4):
            pt.trace_batch_async(1 + 4 * k, 4)
        pt.synchronize()
        same(pt.get_image(W * H), want[15])
    finally:
        pt.pathtraceFree()


# ---- the session's state ---------------------------------------------------------------------------------------------
def test_state_of_the_session(pt, po, scenes, launch_plan):
    """The map survives pt_set_camera and pt_clear_image, reads back as given, leaves the running sum alone when it changes,
    ends with pt_free; None brings the oracle's image back."""
    s = scenes["cornell"]
    geoms, mats, cam, depth = scene_arrays(pt, scenes, "cornell")
    want = reference(pt, po, scenes, "cornell", 10)
    oracle = po.Tracer(geoms, mats, cam, depth, flags=po.F_COMPACT, trig=po.TRIG_SHARED)
    scene = pt.Scene(geoms, mats, cam, depth)
    n = W * H
    pt.pathtraceInit(scene, flags=pt.PT_COMPACT, max_batch=2)
    try:
        assert pt.get_environment() is None                          # pt_init starts black
        t = texels(4)
        pt.set_environment(t)
        assert pt.get_environment().tobytes() == t.tobytes()
        t[:] = 0                                                     # the library keeps its own copy
        same(pt.pathtrace(None, 0, 1), want[0])                      # (pathtrace forwards the camera: pt_set_camera)
        pt.clear_image()
        pt.set_camera(cam, depth)
        same(pt.pathtrace(None, 0, 1), want[0], "after pt_clear_image")
        same(pt.pathtrace(None, 0, 2), want[1])
        pt.set_environment(None)                                     # the sum stays; the next iteration is the oracle's
        assert pt.get_environment() is None
        same(pt.get_image(n), want[1], "the sum after the map has gone")
        oracle.image[:] = want[1]
        oracle.iterate(3)
        same(pt.pathtrace(None, 0, 3), oracle.image, "iteration 3 without a map")
        pt.clear_image()
        oracle.image[:] = 0
        for it in (1, 2):
            oracle.iterate(it)
            same(pt.pathtrace(None, 0, it), oracle.image, "black sky, iteration %d" % it)
        pt.set_environment(texels(4))
        pt.pathtraceFree()
        pt.pathtraceInit(scene, flags=pt.PT_COMPACT, max_batch=2)   # pt_free / pt_init starts black
        assert pt.get_environment() is None
        oracle.image[:] = 0
        oracle.iterate(1)
        same(pt.pathtrace(None, 0, 1), oracle.image, "after pt_free / pt_init")
    finally:
        pt.pathtraceFree()
    assert s["depth"] == depth


def test_fake_shader_ignores_the_map(pt, scenes, launch_plan):
    geoms, mats, cam, depth = scene_arrays(pt, scenes, "cornell")
    scene = pt.Scene(geoms, mats, cam, depth)
    imgs = []
    for with_map in (False, True):
        pt.pathtraceInit(scene, flags=pt.PT_FAKE_SHADER)
        try:
            if with_map:
                pt.set_environment(texels(4))
            pt.pathtrace(None, 0, 1)
            imgs.append(pt.pathtrace(None, 0, 2).copy())
        finally:
            pt.pathtraceFree()
    assert imgs[0].tobytes() == imgs[1].tobytes() and (imgs[0] != 0).any()


def test_refusals(pt, scenes):
    geoms, mats, cam, depth = scene_arrays(pt, scenes, "cornell")
    L = pt.library()
    t = texels(2)
    n = C.c_int(0)
    pt.pathtraceInit(pt.Scene(geoms, mats, cam, depth))
    try:
        for size in (-1, 1025):
            assert L.pt_set_environment(t.ctypes.data, size) == -1 and b"pt_set_environment" in L.pt_last_error()
            assert L.pt_last_error() == b"pt_set_environment: n = %d outside [0, 1024]" % size
            assert L.pt_set_environment(None, size) == -1            # (the size is looked at before the texels)
            assert L.pt_last_error() == b"pt_set_environment: n = %d outside [0, 1024]" % size
        assert L.pt_set_environment(None, 2) == -1 and b"pt_set_environment" in L.pt_last_error()
        assert L.pt_last_error() == b"pt_set_environment: null texels with n = 2"
        assert L.pt_get_environment(None, 0, None) == -1
        assert L.pt_last_error() == b"pt_get_environment: null n"
        assert pt.get_environment() is None                          # a refused call changes nothing
        pt.set_environment(t)
        assert L.pt_get_environment(t.ctypes.data, 23, C.byref(n)) == -1 and n.value == 2      # room for 23 of 24 texels
        assert L.pt_last_error() == b"pt_get_environment: room for 23 texels, the map has 24"
        assert L.pt_get_environment(None, 24, C.byref(n)) == -1
        assert L.pt_last_error() == b"pt_get_environment: room for 0 texels, the map has 24"
        assert L.pt_set_environment(None, 0) == 0 and L.pt_set_environment(t.ctypes.data, 0) == 0
        assert pt.get_environment() is None
    finally:
        pt.pathtraceFree()
    assert L.pt_set_environment(t.ctypes.data, 2) == -1 and b"pt_set_environment" in L.pt_last_error()     # before pt_init
    assert L.pt_last_error() == b"pt_set_environment: not initialised"


# ---- the headless host -------------------------------------------------------------------------------------------------
def test_ptbench_sky(pt, po, tmp_path):
    """ptbench --sky bakes the gradient in C++ and renders scenes/open_sky.txt (here at 100 x 75) under it: the raw running sum
    it saves equals the model's under binding.gradient_cubemap's texels.  Route: the Python bake -- the two bakes are the same
    float64 operations in the same order, so the texels are not read back through pt_get_environment."""
    w, h, iters = 100, 75, 4
    txt = open(os.path.join(ROOT, "scenes", "open_sky.txt")).read()
    assert "RES         800 800" in txt
    scene_file = tmp_path / "open_sky.txt"
    scene_file.write_text(txt.replace("RES         800 800", "RES         %d %d" % (w, h)))
    sky = (16, (0.25, 0.45, 1.0), (0.9, 0.85, 0.8), (0.3, 0.25, 0.2))
    arg = "%d," % sky[0] + ",".join(repr(v) for c in sky[1:] for v in c)
    p = subprocess.run([pt.build_ptbench(), str(scene_file), "--iters", str(iters), "--sky", arg, "--save-sum", "--out", str(tmp_path / "sky")],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "sky: 16 x 16 x 6 texels" in p.stdout
    got = pt.load_pfm(str(tmp_path / ("sky.%dsamp.sum.pfm" % iters)), w, h)
    s = pt.load_scene(str(scene_file))
    m = em.Model(po, s.geoms, s.materials, s.camera, s.traceDepth)
    m.set_environment(pt.gradient_cubemap(*sky))
    for it in range(1, iters + 1):
        m.iterate(it)
    same(got, m.image)
    assert (got > 0).all(axis=1).mean() > 0.9 and re.search(r"Saved .*sky\.4samp\.png", p.stdout)
