"""GPU parity, bounces 0 and 1 in one launch: where a compacting batch's bounce 0 takes the first-hit table
by itself and a plain bounce 1 follows, the batch's first launch (k_bounce<MODE_FIRST2>) shades bounce 0 from the table in
registers and runs the survivors through bounce 1's pipeline in the lanes they have -- the pool between the two bounces is never
written.  Only the work moves: image, rays counted and live counts stay bit-identical to the oracle.  Every case asks the
library whether the form engaged (ptdbg_first_two: such launches since pathtraceInit), the cases that must not take it included.

Batches take the per-bounce plan here (PTMI355_WHOLE_MAX=0): k_iteration never reads the table."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import __graft_entry__ as ge  # noqa: E402,F401
import direct_model as dm  # noqa: E402
import environment_model as em  # noqa: E402
import glossy_model as gm  # noqa: E402
import test_gpu_direct as td  # noqa: E402
import test_gpu_textures as tt  # noqa: E402
from gpu_common import pt, bits, _resized  # noqa: E402,F401
from test_gpu_first_hit import small, tracer, check_batch, init, first_hit, moved_cameras  # noqa: E402
from test_gpu_own_surface import _rotated_scene, _crowded_scene  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 64, 48


@pytest.fixture(autouse=True)
def per_bounce_plan(monkeypatch):
    monkeypatch.setenv("PTMI355_WHOLE_MAX", "0")


def first_two(pt):
    """launches that did bounces 0 and 1 since pathtraceInit"""
    out = (C.c_ulonglong * 1)()
    assert pt.library().ptdbg_first_two(out) == 0
    return int(out[0])


def with_depth(s, depth):
    return dict(s, depth=depth)


@pytest.mark.parametrize("name", ["cornell", "cornell_glass"])
def test_batches(pt, po, scenes, name):
    """Two 5-sample batches in a row: one fused launch per batch; the table is filled once and read by both."""
    s = small(scenes, name)
    init(pt, s, max_batch=5)
    try:
        ref = tracer(po, s)
        check_batch(pt, ref, s, 1, 5, "first batch")
        check_batch(pt, ref, s, 6, 5, "second batch")
        assert first_two(pt) == 2
        assert first_hit(pt) == (1, 2)
    finally:
        pt.pathtraceFree()


@pytest.mark.parametrize("w, h, batch", [(31, 29, 3), (130, 9, 3), (1, 1, 3), (64, 48, 1), (31, 29, 7)])
def test_shapes_at_the_edges(pt, po, scenes, w, h, batch):
    """A last tile of 3 lanes; a wide, flat frame; one pixel (tile_pixels == 1 in sample_of, far more waves than tiles); batches
    of one sample and of max_batch."""
    s = small(scenes, "cornell", w, h)
    init(pt, s, max_batch=7)
    try:
        ref = tracer(po, s)
        check_batch(pt, ref, s, 1, batch)
        check_batch(pt, ref, s, 1 + batch, batch)
        assert first_two(pt) == 2
    finally:
        pt.pathtraceFree()


@pytest.mark.parametrize("depth, fused", [(2, True), (3, True), (1, False)])
def test_depths(pt, po, scenes, depth, fused):
    """Depth 2: bounce 1 is the last bounce -- nothing survives it, nothing is deferred.  Depth 1: there is no bounce 1 to take."""
    s = with_depth(small(scenes, "cornell_glass"), depth)
    init(pt, s, max_batch=3)
    try:
        ref = tracer(po, s)
        check_batch(pt, ref, s, 1, 3)
        check_batch(pt, ref, s, 4, 3)
        assert first_two(pt) == (2 if fused else 0)
        assert first_hit(pt) == (1, 2)
    finally:
        pt.pathtraceFree()


def test_bounce_0_ends_everything_and_camera_moves(pt, po, scenes):
    """Turned away and out of sight every path ends at bounce 0: live[1] == 0 and the image stays zero.  ("Far outside", 150 units
    back, still has the box on the view axis, where the ray of pixel (W / 2, H / 2) runs: that pixel's three samples are all of
    bounce 1 -- the oracle's count, compared by check_batch -- so a camera 15 000 units back and 100 to the side stands beside
    it: its axis passes the box and its other rays are hundreds of units apart there.)  Every camera move costs one refill of
    the table, and the form is taken again."""
    s = small(scenes, "cornell")
    init(pt, s, max_batch=3)
    try:
        gone = s["camera"].copy()
        gone["position"][0][2] += 15000.0
        gone["position"][0][0] += 100.0
        for k, (what, cam) in enumerate(moved_cameras(s["camera"]) + [("out of sight", gone)]):
            pt.set_camera(cam, s["depth"])
            pt.clear_image()
            ref = tracer(po, s, cam=cam)
            check_batch(pt, ref, s, 1 + 3 * k, 3, what)
            if what == "far outside":
                assert pt.get_stats().live[1] <= 3, what
            if what in ("turned away", "out of sight"):
                assert pt.get_stats().live[1] == 0, what
                assert not bits(pt.get_image(W * H)).any(), what
            assert first_hit(pt) == (k + 1, k + 1), what
            assert first_two(pt) == k + 1, what
    finally:
        pt.pathtraceFree()


@pytest.mark.parametrize("shape", ["rotated and glass cubes", "16 primitives", "70 primitives"])
def test_own_surface_and_crowded_scenes(pt, po, scenes, shape):
    """General reject rows on the own-surface form; scenes past OWN_MAX_GEOMS (and past the candidate masks): the form without it."""
    s = {"rotated and glass cubes": lambda: _rotated_scene(pt, scenes), "16 primitives": lambda: _crowded_scene(pt, scenes, 16),
         "70 primitives": lambda: _crowded_scene(pt, scenes, 70)}[shape]()
    if shape != "rotated and glass cubes":
        assert not pt.probe_own_surface_plan(32 * 32 * 3, len(s["geoms"]))
    init(pt, s, max_batch=3)
    try:
        ref = tracer(po, s)
        check_batch(pt, ref, s, 1, 3)
        check_batch(pt, ref, s, 4, 3)
        assert first_two(pt) == 2
    finally:
        pt.pathtraceFree()


def test_environment_session(pt, po, scenes):
    """An open scene under a cube map: pixels at the frame's edge miss at bounce 0 and end with the map's texel, written behind
    their tile's bounce-1 survivors; paths that leave at bounce 1 read it too.  Then a camera under which every ray misses."""
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
            assert 0 < pt.get_stats().live[1] < 3 * 50 * 37        # some camera rays leave the scene
            assert (bits(pt.get_image(50 * 37)) == bits(want)).all(), iter0
        assert first_two(pt) == 2
        away = moved_cameras(cam)[2][1]
        m2 = em.Model(po, scn.geoms, scn.materials, away, scn.traceDepth)
        m2.set_environment(tex)
        pt.set_camera(away, scn.traceDepth)
        pt.clear_image()
        pt.trace_batch(7, 3)
        for it in range(7, 10):
            want = m2.iterate(it)
        assert pt.get_stats().live[1] == 0
        assert bits(want).any() and (bits(pt.get_image(50 * 37)) == bits(want)).all()
        assert first_two(pt) == 3
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
        assert first_two(pt) == 2
    finally:
        pt.pathtraceFree()


def test_stepping_interface_keeps_its_launches(pt, po, scenes):
    s = small(scenes, "cornell")
    n = W * H
    init(pt, s)
    try:
        ref = tracer(po, s)
        for it in (1, 2):
            st = ref.iterate(it)
            pt.trace_begin(it, 1)
            for d in range(s["depth"]):
                pt.trace_bounce(d)
            pt.trace_end()
            gs = pt.get_stats()
            assert list(gs.live[:s["depth"]]) == list(st.live[:s["depth"]]) and gs.rays == st.rays
            assert pt.get_image(n).tobytes() == ref.image.tobytes(), it
        assert first_hit(pt) == (1, 2) and first_two(pt) == 0
    finally:
        pt.pathtraceFree()


@pytest.mark.parametrize("what", ["non-compacting", "PT_CACHE_FIRST", "PT_AA_JITTER", "lens"])
def test_sessions_that_do_not_take_it(pt, po, scenes, what):
    s = small(scenes, "cornell")
    flags = {"non-compacting": 0, "PT_CACHE_FIRST": pt.PT_COMPACT | pt.PT_CACHE_FIRST, "PT_AA_JITTER": pt.PT_COMPACT | pt.PT_AA_JITTER,
             "lens": pt.PT_COMPACT}[what]
    oflags = {"non-compacting": 0, "PT_AA_JITTER": po.F_COMPACT | po.F_AA}.get(what, po.F_COMPACT)
    init(pt, s, flags=flags, max_batch=3)
    try:
        kw = {}
        if what == "lens":
            pt.set_lens(0.4, 9.0)
            kw["lens"] = (0.4, 9.0)
        ref = tracer(po, s, flags=oflags, **kw)
        check_batch(pt, ref, s, 1, 3)
        check_batch(pt, ref, s, 4, 3)
        assert first_two(pt) == 0
        assert first_hit(pt) == ((1, 2) if what in ("non-compacting", "PT_CACHE_FIRST") else (0, 0))
    finally:
        pt.pathtraceFree()


def test_texture_set_does_not_take_it(pt, po, scenes):
    want, _, _ = tt.reference(pt, po, scenes, "textured")
    tt.session(pt, scenes, "textured", pt.PT_COMPACT, max_batch=2)
    try:
        tt.trace_two_then_two(pt, want)
        assert first_two(pt) == 0
    finally:
        pt.pathtraceFree()


def test_direct_light_at_depth_2_does_not_take_it(pt, po, scenes):
    """traceDepth 2 with lights to sample: bounce 1 is the sampling bounce, a DIRECT form.  At depth 4 bounces 0 and 1 are plain."""
    g, mats, cam, _ = td.two_lamps(pt)
    for depth, fused in ((2, 0), (4, 1)):
        m = dm.Model(po, g, mats, cam, depth)
        pt.pathtraceInit(pt.Scene(g, mats, cam, depth), flags=pt.PT_COMPACT | pt.PT_DIRECT_LIGHT, max_batch=2)
        try:
            pt.trace_batch(1, 2)
            for it in (1, 2):
                want = m.iterate(it)
            assert (bits(pt.get_image(td.W * td.H)) == bits(want)).all(), depth
            assert first_two(pt) == fused, depth
        finally:
            pt.pathtraceFree()


def test_asynchronous_batches_on_lanes(pt, po, scenes):
    s = small(scenes, "cornell_glass")
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
        assert (bits(pt.get_image(W * H)) == bits(ref.image)).all()
        assert first_hit(pt) == (2, 8) and first_two(pt) == 8
    finally:
        pt.pathtraceFree()


def test_lookahead_windows_across_a_camera_change(pt, po, scenes):
    s = small(scenes, "cornell")
    scene = pt.Scene(s["geoms"], s["materials"], s["camera"], s["depth"])
    pt.pathtraceInit(scene, flags=pt.PT_COMPACT | pt.PT_LOOKAHEAD, max_batch=8)
    try:
        ref = tracer(po, s)
        for it in range(1, 11):
            img = pt.pathtrace(None, 0, it)
            ref.iterate(it)
            assert (bits(img) == bits(ref.image)).all(), it
        assert first_two(pt) == first_hit(pt)[1] >= 2
        cam2 = s["camera"].copy()
        cam2["position"][0][1] += 0.5
        scene.camera = cam2
        ref = tracer(po, s, cam=cam2, image=ref.image)
        for it in range(11, 21):
            img = pt.pathtrace(None, 0, it)
            ref.iterate(it)
            assert (bits(img) == bits(ref.image)).all(), it
        fills, launches = first_hit(pt)
        assert fills == 2 and first_two(pt) == launches >= 4
    finally:
        pt.pathtraceFree()


def test_tile_of_a_frame(pt, po, scenes):
    """Tile 1 of 3 (strips of 8 rows) of 64 x 48: the table is indexed by the tile's local pixel."""
    s = small(scenes, "cornell")
    own = pt.sharding.tile_pixel_indices(1, 3, 8, W, H)
    init(pt, s, max_batch=3, tile=(1, 3, 8))
    try:
        ref = tracer(po, s)
        img = np.zeros((W * H, 3), dtype=np.float32)
        for iter0 in (1, 4):
            pt.trace_batch(iter0, 3, img)
            ref.iterate_parallel(iter0, 3, 3)
            assert pt.get_stats().live[0] == 3 * len(own)
            assert (bits(img[own]) == bits(ref.image[own])).all(), iter0
        assert first_two(pt) == 2
    finally:
        pt.pathtraceFree()


def test_session_over_two_contexts(pt, po, scenes):
    """devices = [0, 0]: each context traces the strips it owns with a table of its own; the counter sums the contexts."""
    s = small(scenes, "cornell")
    init(pt, s, max_batch=3, devices=[0, 0], tile=(0, 1, 8))
    try:
        ref = tracer(po, s)
        img = np.zeros((W * H, 3), dtype=np.float32)
        for iter0 in (1, 4):
            pt.trace_batch(iter0, 3, img)
            ref.iterate_parallel(iter0, 3, 3)
            assert (bits(img) == bits(ref.image)).all(), iter0
        assert first_two(pt) == 4 and first_hit(pt) == (2, 4)
    finally:
        pt.pathtraceFree()


def test_ab_control(pt, po, scenes, monkeypatch):
    """PTMI355_FIRST_TWO=0 (an experiments build only): bounce 0 stays a launch of its own."""
    if not pt.has_experiments():
        pytest.skip("PTMI355_FIRST_TWO is read by -DPT_EXPERIMENTS builds only")
    monkeypatch.setenv("PTMI355_FIRST_TWO", "0")
    s = small(scenes, "cornell")
    init(pt, s, max_batch=3)
    try:
        ref = tracer(po, s)
        check_batch(pt, ref, s, 1, 3)
        assert first_two(pt) == 0 and first_hit(pt) == (1, 1)
    finally:
        pt.pathtraceFree()
