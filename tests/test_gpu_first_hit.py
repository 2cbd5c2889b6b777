"""GPU parity, bounce 0 from the first-hit table: a pinhole camera without jitter sends the same ray
through every pixel in every iteration, so the plain fused pipeline intersects bounce 0 once per camera (k_cache_first: t,
normal, material, outside and the winning primitive per pixel) and every later bounce 0 only looks its hit up and shades it
(k_bounce<MODE_CACHE0>).  Only the work moves: rays counted, live counts, pool order, pending directions, the primitive a
survivor carries to bounce 1, final colours and images stay bit-identical to the oracle.  Every case that expects the form
asks the library whether it engaged (ptdbg_first_hit: fills of the table, bounce-0 launches that read it).

Batches take the per-bounce plan here (PTMI355_WHOLE_MAX=0): k_iteration never reads the table."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import __graft_entry__ as ge  # noqa: E402,F401
import environment_model as em  # noqa: E402
import glossy_model as gm  # noqa: E402
from gpu_common import pt, bits, assert_paths_equal, _after, _resized  # noqa: E402,F401
from test_gpu_own_surface import _rotated_scene, _crowded_scene  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 64, 48                                              # 3072 pixels: 48 tiles


@pytest.fixture(autouse=True)
def per_bounce_plan(monkeypatch):
    monkeypatch.setenv("PTMI355_WHOLE_MAX", "0")


def first_hit(pt):
    """(fills of the table, bounce-0 launches that read it) since pathtraceInit"""
    out = (C.c_ulonglong * 2)()
    assert pt.library().ptdbg_first_hit(out) == 0
    return int(out[0]), int(out[1])


def small(scenes, name, w=W, h=H):
    s = scenes[name]
    return {"geoms": s["geoms"], "materials": s["materials"], "camera": _resized(s["camera"], w, h), "depth": s["depth"]}


def tracer(po, s, cam=None, image=None, **kw):
    ref = po.Tracer(s["geoms"].view(po.GEOM_DT), s["materials"], s["camera"] if cam is None else cam, s["depth"],
                    flags=kw.pop("flags", po.F_COMPACT), trig=po.TRIG_SHARED, **kw)
    if image is not None:
        ref.image[:] = image
    return ref


def oracle_batch(ref, iter0, count, depth):
    """`count` iterations one after the other: (rays, live[] summed over the samples); ref.image is the running sum."""
    rays, live = 0, np.zeros(depth, dtype=np.int64)
    for it in range(iter0, iter0 + count):
        st = ref.iterate(it)
        rays += st.rays
        live += np.array(st.live[:depth], dtype=np.int64)
    return rays, list(live)


def check_batch(pt, ref, s, iter0, count, what=""):
    n = len(ref.image)
    pt.trace_batch(iter0, count)
    rays, live = oracle_batch(ref, iter0, count, s["depth"])
    gs = pt.get_stats()
    assert gs.rays == rays, what
    assert list(gs.live[:s["depth"]]) == live, what
    assert (bits(pt.get_image(n)) == bits(ref.image)).all(), what


def init(pt, s, flags=None, **kw):
    pt.pathtraceInit(pt.Scene(s["geoms"], s["materials"], s["camera"], s["depth"]), flags=pt.PT_COMPACT if flags is None else flags, **kw)


@pytest.mark.parametrize("name", ["cornell", "cornell_glass"])
@pytest.mark.parametrize("compact", [True, False])
def test_batches(pt, po, scenes, name, compact):
    """Two 5-sample batches in a row: one fill, one table launch per batch."""
    s = small(scenes, name)
    init(pt, s, flags=pt.PT_COMPACT if compact else 0, max_batch=5)
    try:
        ref = tracer(po, s, flags=po.F_COMPACT if compact else 0)
        check_batch(pt, ref, s, 1, 5, "first batch")
        check_batch(pt, ref, s, 6, 5, "second batch")
        assert first_hit(pt) == (1, 2)
    finally:
        pt.pathtraceFree()


@pytest.mark.parametrize("name", ["cornell", "cornell_glass"])
def test_stepped(pt, po, scenes, name):
    """Every bounce of iterations 1-3 stepped and exported: the pool after bounce 0 (written from the table) and after every
    later bounce (bounce 1 reads the primitive bounce 0 tagged) is the oracle's, the pixelIndex sequence included."""
    s = small(scenes, name)
    n = W * H
    init(pt, s)
    try:
        ref = tracer(po, s)
        for it in (1, 2, 3):
            snaps = []
            st = ref.iterate(it, snapshots=snaps)
            pt.trace_begin(it, 1)
            for snap in snaps:
                d = snap["depth"]
                n_live = pt.trace_bounce(d)
                paths, live = pt.export_paths(n)
                assert n_live == snap["n_live"] == live, (it, d)
                assert ((paths["pixelIndex"][:live] >= 0) & (paths["pixelIndex"][:live] < n)).all(), (it, d)
                assert_paths_equal(paths, _after(snaps, d, ref), live)
            for d in range(len(snaps), s["depth"]):
                pt.trace_bounce(d)
            pt.trace_end()
            gs = pt.get_stats()
            assert list(gs.live[:s["depth"]]) == list(st.live[:s["depth"]]), it
            assert gs.rays == st.rays
            assert pt.get_image(n).tobytes() == ref.image.tobytes(), it
        assert first_hit(pt) == (1, 3)
    finally:
        pt.pathtraceFree()


def moved_cameras(cam):
    """The camera as given, moved sideways, turned away from the box (every ray misses) and far outside the scene."""
    side = cam.copy()
    side["position"][0][0] += 0.75
    away = cam.copy()
    away["view"][0] = -cam["view"][0]
    away["right"][0] = -cam["right"][0]
    far = cam.copy()
    far["position"][0][2] += 150.0
    return [("as given", cam), ("sideways", side), ("turned away", away), ("far outside", far)]


def test_camera(pt, po, scenes):
    """One batch after each camera move equals a fresh session's (the oracle from an empty image); the table is filled once
    per distinct camera, and setting the same camera again fills nothing."""
    s = small(scenes, "cornell")
    init(pt, s, max_batch=3)
    try:
        for k, (what, cam) in enumerate(moved_cameras(s["camera"])):
            pt.set_camera(cam, s["depth"])
            pt.set_camera(cam, s["depth"])
            pt.clear_image()
            ref = tracer(po, s, cam=cam)
            check_batch(pt, ref, s, 1 + 3 * k, 3, what)
            if what == "turned away":
                assert pt.get_stats().live[1] == 0                  # every ray missed
            assert first_hit(pt) == (k + 1, 2 * k + 1), what
            pt.set_camera(cam, s["depth"])                          # the same camera: the table stands
            check_batch(pt, ref, s, 40 + 3 * k, 3, what + ", again")
            assert first_hit(pt) == (k + 1, 2 * k + 2), what
    finally:
        pt.pathtraceFree()


def test_jitter_never_reads_the_table(pt, po, scenes):
    s = small(scenes, "cornell")
    init(pt, s, flags=pt.PT_COMPACT | pt.PT_AA_JITTER, max_batch=3)
    try:
        ref = tracer(po, s, flags=po.F_COMPACT | po.F_AA)
        check_batch(pt, ref, s, 1, 3)
        check_batch(pt, ref, s, 4, 3)
        assert first_hit(pt) == (0, 0)
    finally:
        pt.pathtraceFree()


def test_lens_on_and_off(pt, po, scenes):
    """A lens set after pt_init: no table launch while the rays differ from iteration to iteration; with the lens off again
    the form engages again, on the table it filled before (the camera has not moved)."""
    s = small(scenes, "cornell")
    init(pt, s, max_batch=3)
    try:
        ref = tracer(po, s)
        check_batch(pt, ref, s, 1, 3, "pinhole")
        assert first_hit(pt) == (1, 1)
        pt.set_lens(0.4, 9.0)
        ref = tracer(po, s, image=ref.image, lens=(0.4, 9.0))
        check_batch(pt, ref, s, 4, 3, "lens")
        assert first_hit(pt) == (1, 1)
        pt.set_lens(0.0, 0.0)
        ref = tracer(po, s, image=ref.image)
        check_batch(pt, ref, s, 7, 3, "pinhole again")
        assert first_hit(pt) == (1, 2)
    finally:
        pt.pathtraceFree()


def inside_glass(pt, scenes):
    """The rotated scene of the own-surface tests with the eye at the centre of its turned glass cube: outside = 0 at the
    first hit of every pixel."""
    s = _rotated_scene(pt, scenes)
    cam = s["camera"].copy()
    cam["position"][0] = (1.6, 2.2, 0.5)
    s["camera"] = cam
    return s


@pytest.mark.parametrize("shape", ["50x30", "rotated and glass cubes", "eye inside a glass cube", "16 primitives", "70 primitives"])
def test_shapes(pt, po, scenes, shape):
    """A frame whose last tile has 28 lanes and whose tiles have no candidate masks; general rows and a first hit from inside
    (outside = 0); a scene beyond the own-surface code space; one beyond the candidate masks."""
    s = {"50x30": lambda: small(scenes, "cornell", 50, 30), "rotated and glass cubes": lambda: _rotated_scene(pt, scenes),
         "eye inside a glass cube": lambda: inside_glass(pt, scenes), "16 primitives": lambda: _crowded_scene(pt, scenes, 16),
         "70 primitives": lambda: _crowded_scene(pt, scenes, 70)}[shape]()
    if shape == "16 primitives":
        assert not pt.probe_own_surface_plan(32 * 32 * 3, 16)
    init(pt, s, max_batch=3)
    try:
        ref = tracer(po, s)
        if shape == "eye inside a glass cube":
            snaps = []
            tracer(po, s).iterate(1, snapshots=snaps)
            t0 = snaps[0]["isects"]["t"]
            assert (t0 > 0).all()                                   # (every camera ray ends on the cube's inside)
        check_batch(pt, ref, s, 1, 3)
        check_batch(pt, ref, s, 4, 3)
        assert first_hit(pt) == (1, 2)
    finally:
        pt.pathtraceFree()


def test_tile_of_a_frame(pt, po, scenes):
    """Tile 1 of 3 (strips of 8 rows) of 64 x 48: local and global pixel indices differ; the table is indexed by the local one."""
    s = small(scenes, "cornell")
    n = W * H
    own = pt.sharding.tile_pixel_indices(1, 3, 8, W, H)
    init(pt, s, max_batch=3, tile=(1, 3, 8))
    try:
        ref = tracer(po, s)
        img = np.zeros((n, 3), dtype=np.float32)
        for iter0 in (1, 4):
            pt.trace_batch(iter0, 3, img)
            ref.iterate_parallel(iter0, 3, 3)
            assert pt.get_stats().live[0] == 3 * len(own)
            assert (bits(img[own]) == bits(ref.image[own])).all(), iter0
        assert first_hit(pt) == (1, 2)
    finally:
        pt.pathtraceFree()


def test_environment_session(pt, po, scenes):
    """An open scene under a cube map: the pixels at the frame's edge miss at bounce 0 (t = -1 in the table) and end with the
    map's texel."""
    scn = pt.load_scene(os.path.join(ROOT, "scenes", "open_sky.txt"))
    cam = _resized(scn.camera, 50, 37)
    tex = np.random.default_rng(4001).uniform(0, 2, (6, 4, 4, 3)).astype(np.float32)
    m = em.Model(po, scn.geoms, scn.materials, cam, scn.traceDepth)
    m.set_environment(tex)
    pt.pathtraceInit(pt.Scene(scn.geoms, scn.materials, cam, scn.traceDepth), flags=pt.PT_COMPACT, max_batch=3)
    try:
        pt.set_environment(tex)
        for iter0 in (1, 4):
            pt.trace_batch(iter0, 3)
            for it in range(iter0, iter0 + 3):
                want = m.iterate(it)
            assert pt.get_stats().live[1] < 3 * 50 * 37             # some camera rays leave the scene
            assert (bits(pt.get_image(50 * 37)) == bits(want)).all(), iter0
        assert first_hit(pt) == (1, 2)
    finally:
        pt.pathtraceFree()


def test_glossy_session(pt, po, scenes):
    scn = pt.load_scene(os.path.join(ROOT, "scenes", "cornell_glossy.txt"))
    cam = _resized(scn.camera, 50, 37)
    m = gm.Model(po, scn.geoms, scn.materials, cam, scn.traceDepth)
    pt.pathtraceInit(pt.Scene(scn.geoms, scn.materials, cam, scn.traceDepth), flags=pt.PT_COMPACT | pt.PT_GLOSSY, max_batch=3)
    try:
        for iter0 in (1, 4):
            pt.trace_batch(iter0, 3)
            for it in range(iter0, iter0 + 3):
                want = m.iterate(it)
            assert (bits(pt.get_image(50 * 37)) == bits(want)).all(), iter0
        assert first_hit(pt) == (1, 2)
    finally:
        pt.pathtraceFree()


def test_asynchronous_batches_on_lanes(pt, po, scenes):
    """Four batches enqueued back to back right after pt_init, and four more right after a camera change: the fill is enqueued
    by the first of them while the others go to other lanes.  (An unordered fill would show as a flaky failure, not a steady
    one: the ordering argument is written down at the fill, csrc/pt_h_enqueue.hpp.)"""
    s = small(scenes, "cornell_glass")
    n = W * H
    init(pt, s, max_batch=4)
    try:
        ref = tracer(po, s)
        for k in range(4):
            pt.trace_batch_async(1 + 4 * k, 4)
        cam2 = s["camera"].copy()
        cam2["position"][0][0] -= 1.25
        pt.set_camera(cam2, s["depth"])
        for k in range(4, 8):
            pt.trace_batch_async(1 + 4 * k, 4)
        pt.synchronize()
        ref.iterate_parallel(1, 16, 4)
        ref = tracer(po, s, cam=cam2, image=ref.image)
        ref.iterate_parallel(17, 16, 4)
        assert (bits(pt.get_image(n)) == bits(ref.image)).all()
        assert first_hit(pt) == (2, 8)
    finally:
        pt.pathtraceFree()


def test_lookahead_windows_across_a_camera_change(pt, po, scenes):
    """PT_LOOKAHEAD: windows traced ahead of the calls read the table; the camera the host hands over changes between two
    calls, the windows traced for the old one are void and the table is filled again before the next window's bounce 0."""
    s = small(scenes, "cornell")
    scene = pt.Scene(s["geoms"], s["materials"], s["camera"], s["depth"])
    pt.pathtraceInit(scene, flags=pt.PT_COMPACT | pt.PT_LOOKAHEAD, max_batch=8)
    try:
        ref = tracer(po, s)
        for it in range(1, 11):
            img = pt.pathtrace(None, 0, it)
            ref.iterate(it)
            assert (bits(img) == bits(ref.image)).all(), it
        fills, launches = first_hit(pt)
        assert fills == 1 and launches >= 2
        cam2 = s["camera"].copy()
        cam2["position"][0][1] += 0.5
        scene.camera = cam2
        ref = tracer(po, s, cam=cam2, image=ref.image)
        for it in range(11, 21):
            img = pt.pathtrace(None, 0, it)
            ref.iterate(it)
            assert (bits(img) == bits(ref.image)).all(), it
        fills2, launches2 = first_hit(pt)
        assert fills2 == 2 and launches2 >= launches + 2
    finally:
        pt.pathtraceFree()
