"""GPU parity, bounce 0 from the first-state table: in a session without PT_GLOSSY, refractive material or
environment map the launch that does bounces 0 and 1 (section 6.23) reads, per pixel, what bounce 0 leaves of the camera ray --
ends with colour 0, ends with a constant colour, diffuse hit (point, normal, throughput) or fixed direction (a mirror) -- from a
table filled once per camera (k_bounce<MODE_STATE2>), and a 64-path tile none of whose paths survives bounce 0 never enters the
pipeline.  Only the work moves: image, rays counted and live counts stay bit-identical to the oracle.  Every case asks the library
whether the form engaged (ptdbg_first_state: such launches since pathtraceInit), the sessions that must not take it included, and
the sessions that switch between the forms on the way -- a map, textures or a lens set and removed, traceDepth changed, pt_free
and pt_init between scenes with and without glass -- after every step.

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
import texture_model as tm  # noqa: E402
from gpu_common import pt, bits, _resized  # noqa: E402,F401
from test_gpu_first_hit import small, tracer, check_batch, init, first_hit, moved_cameras  # noqa: E402
from test_gpu_first_two import first_two, with_depth  # noqa: E402
from test_gpu_own_surface import _rotated_scene, _scene, ROOM, CUBE, SPHERE  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 64, 48


@pytest.fixture(autouse=True)
def per_bounce_plan(monkeypatch):
    monkeypatch.setenv("PTMI355_WHOLE_MAX", "0")


def first_state(pt):
    """launches whose bounce 0 came from the first-state table since pathtraceInit"""
    out = (C.c_ulonglong * 1)()
    assert pt.library().ptdbg_first_state(out) == 0
    return int(out[0])


def turned(cam, degrees):
    """The camera turned about its up axis."""
    c = cam.copy()
    a = np.float32(np.deg2rad(degrees))
    v, r = cam["view"][0].astype(np.float32), cam["right"][0].astype(np.float32)
    c["view"][0] = np.cos(a) * v + np.sin(a) * r
    c["right"][0] = np.cos(a) * r - np.sin(a) * v
    return c


def stepped_back(cam, by):
    c = cam.copy()
    c["position"][0][2] += by
    return c


def looking_at_the_light(cam):
    """From inside the box, low and in front, up at the ceiling light: the middle of the frame is the emitter."""
    c = cam.copy()
    c["position"][0] = (0.0, 2.0, 4.0)
    v = np.array([0.0, 8.0, -4.0], dtype=np.float32)
    v /= np.float32(np.sqrt(np.float32(80.0)))
    c["view"][0] = v
    c["right"][0] = (1.0, 0.0, 0.0)
    c["up"][0] = (0.0, -v[2], v[1])
    return c


def without_glass(s, instead):
    """The scene with its glass primitives given material `instead` and the glass material gone (materials of cornell_glass_64:
    0 light, 1 white, 2 red, 3 green, 4 mirror, 5 glass)."""
    g = s["geoms"].copy()
    g["materialid"][g["materialid"] == 5] = instead
    return dict(s, geoms=g, materials=s["materials"][:5].copy())


def two_batches(pt, po, s, batch, max_batch, taken=True, **kw):
    init(pt, s, max_batch=max_batch, **kw)
    try:
        ref = tracer(po, s)
        check_batch(pt, ref, s, 1, batch, "first batch")
        check_batch(pt, ref, s, 1 + batch, batch, "second batch")
        assert first_two(pt) == 2
        assert first_state(pt) == (2 if taken else 0)
        assert first_hit(pt) == (1, 2)
    finally:
        pt.pathtraceFree()


@pytest.mark.parametrize("w, h", [(64, 4), (128, 3), (31, 29), (130, 9), (1, 1), (64, 48)])
def test_frames(pt, po, scenes, w, h):
    """64 x 4 and 128 x 3: whole tiles, the ended-tile words apply; 31 x 29 and 130 x 9: they do not, only the test after the record
    load skips; one pixel; 64 x 48 has the mirror ball in view (the fixed-direction kind)."""
    two_batches(pt, po, small(scenes, "cornell", w, h), 3, 3)


@pytest.mark.parametrize("batch", [1, 3, 7])
def test_batch_sizes(pt, po, scenes, batch):
    two_batches(pt, po, small(scenes, "cornell"), batch, 7)


@pytest.mark.parametrize("depth, taken", [(2, True), (3, True), (1, False)])
def test_depths(pt, po, scenes, depth, taken):
    """Depth 2: bounce 1 is the last bounce.  Depth 1: there is no bounce 1, so no launch of the two."""
    s = with_depth(small(scenes, "cornell"), depth)
    init(pt, s, max_batch=3)
    try:
        ref = tracer(po, s)
        check_batch(pt, ref, s, 1, 3)
        check_batch(pt, ref, s, 4, 3)
        assert first_state(pt) == first_two(pt) == (2 if taken else 0)
    finally:
        pt.pathtraceFree()


@pytest.mark.parametrize("w, h", [(64, 4), (64, 48), (31, 29)])
def test_cameras(pt, po, scenes, w, h):
    """One batch after each camera move, against a fresh oracle: as given; sideways; turned away, where every pixel ends with
    colour 0 -- every tile is skipped, live[1] == 0, the image stays zero --; far outside and stepped back, where whole rows of
    tiles end and others do not (the words differ from tile to tile at 64 wide); turned by 25 and 40 degrees, where ended and
    live pixels share tiles; looking at the light, where the constant colour is summed once per sample in sample order.  Every
    move refills the table and the counts follow it."""
    s = small(scenes, "cornell", w, h)
    cam = s["camera"]
    cams = moved_cameras(cam) + [("stepped back", stepped_back(cam, 30.0)), ("turned 25", turned(cam, 25.0)),
                                 ("turned 40", turned(cam, 40.0)), ("at the light", looking_at_the_light(cam))]
    init(pt, s, max_batch=3)
    try:
        for k, (what, c) in enumerate(cams):
            pt.set_camera(c, s["depth"])
            pt.clear_image()
            ref = tracer(po, s, cam=c)
            check_batch(pt, ref, s, 1 + 3 * k, 3, what)
            live = pt.get_stats().live
            if what == "turned away":
                assert live[1] == 0, what
                assert not bits(pt.get_image(w * h)).any(), what
            # (at 64 x 4 the four rows are 0.5 apart in slope: they pass above and below a box 30 units further away, and the
            # light 9 units away sits between the two middle rows)
            if what in ("turned 25", "turned 40") or (h >= 29 and what in ("stepped back", "at the light")):
                assert 0 < live[1] < live[0], what
            if what == "at the light" and h >= 29:
                img = pt.get_image(w * h).reshape(h, w, 3)
                assert (img[h // 2, w // 2] > 0).all(), what
            assert first_hit(pt) == (k + 1, k + 1), what
            assert first_state(pt) == first_two(pt) == k + 1, what
    finally:
        pt.pathtraceFree()


@pytest.mark.parametrize("shape", ["mirror cube", "rotated cubes"])
def test_own_surface_bits_of_the_record(pt, po, scenes, shape):
    """A mirror cube in the room; the rotated scene of the own-surface tests with its glass made mirror (general reject rows, a
    turned mirror slab, a mirror ball): the record names the primitive a survivor leaves."""
    if shape == "mirror cube":
        s = _scene(pt, scenes, ROOM + [(CUBE, 4, (1.5, 2.0, 0.0), (0, 30, 0), (3.0, 4.0, 3.0)), (SPHERE, 1, (-2.5, 2.0, 1.0), (0, 0, 0), (3, 3, 3))])
        s = dict(s, materials=s["materials"][:5].copy())
    else:
        s = without_glass(_rotated_scene(pt, scenes), 4)
    assert pt.probe_own_surface_plan(48 * 48 * 3, len(s["geoms"]))
    two_batches(pt, po, s, 3, 3)


@pytest.mark.parametrize("w, h", [(64, 48), (31, 29)])
def test_lamp_without_red(pt, po, scenes, w, h):
    """The lamp's colour (0, 0.8, 0.6), seen directly: those pixels end with a colour whose first component is 0 -- a constant
    colour all the same (put_final's test looks at all three components), not the kind that ends with 0."""
    s = small(scenes, "cornell", w, h)
    mats = s["materials"].copy()
    assert mats["emittance"][0] > 0
    mats["color"][0] = (0.0, 0.8, 0.6)
    s = dict(s, materials=mats, camera=looking_at_the_light(s["camera"]))
    snaps = []
    tracer(po, s).iterate(1, snapshots=snaps)
    p = snaps[0]["paths"]
    seen = (p["remainingBounces"] == 0) & (p["color"][:, 0] == 0) & (p["color"][:, 1] > 0)
    assert seen.sum() >= 8
    two_batches(pt, po, s, 3, 3)


def test_glass_keeps_the_per_sample_form(pt, po, scenes):
    """A refractive material anywhere in the scene: the Fresnel choice draws from the sample's engine at bounce 0."""
    two_batches(pt, po, small(scenes, "cornell_glass"), 3, 3, taken=False)
    two_batches(pt, po, _rotated_scene(pt, scenes), 3, 3, taken=False)


def test_environment_map_keeps_the_per_sample_form(pt, po, scenes):
    """While a map is set a miss is a fifth kind; with the map taken away again the session reads its table
    (test_environment_map_set_removed_and_set_again)."""
    scn = pt.load_scene(os.path.join(ROOT, "scenes", "open_sky.txt"))
    cam = _resized(scn.camera, 50, 37)
    tex = np.random.default_rng(4001).uniform(0, 2, (6, 4, 4, 3)).astype(np.float32)
    m = em.Model(po, scn.geoms, scn.materials, cam, scn.traceDepth)
    m.set_environment(tex)
    pt.pathtraceInit(pt.Scene(scn.geoms, scn.materials, cam, scn.traceDepth), flags=pt.PT_COMPACT, max_batch=3)
    try:
        pt.set_environment(tex)
        pt.trace_batch(1, 3)
        for it in range(1, 4):
            want = m.iterate(it)
        assert (bits(pt.get_image(50 * 37)) == bits(want)).all()
        assert first_two(pt) == 1 and first_state(pt) == 0
    finally:
        pt.pathtraceFree()


# ---- transitions inside one session ------------------------------------------------------------------------------------------------
# Each step traces one batch of 3 and compares the running sum bit for bit; after it, `counters` must be (launches from the
# first-state table, launches of bounces 0 and 1, (fills of the first-hit table, bounce-0 launches that read it)) as
# enqueue_bounce and pt_set_camera imply: the first-hit form (auto0) does not ask about the map or the depth, so its table -- and
# the first-state records k_cache_first writes in the same pass -- is filled by the first batch without lens and textures and
# stands until the camera moves; the first-state form asks per launch for depth >= 2 and no map.
FRAMES = [(64, 48), (64, 4)]


def counters(pt):
    return first_state(pt), first_two(pt), first_hit(pt)


def model_batch(pt, m, n, iter0, what):
    pt.trace_batch(iter0, 3)
    for it in range(iter0, iter0 + 3):
        want = m.iterate(it)
    assert (bits(pt.get_image(n)) == bits(want)).all(), what


@pytest.mark.parametrize("w, h", FRAMES)
def test_environment_map_set_removed_and_set_again(pt, po, scenes, w, h):
    """Map set: the per-sample form, which fills the tables -- (0, 1, (1, 1)); map removed: the table form on the records filled
    under the map -- (1, 2, (1, 2)); map set again: the per-sample form -- (1, 3, (1, 3))."""
    s = small(scenes, "cornell", w, h)
    tex = np.random.default_rng(4001).uniform(0, 2, (6, 4, 4, 3)).astype(np.float32)
    m = em.Model(po, s["geoms"], s["materials"], s["camera"], s["depth"])
    init(pt, s, max_batch=3)
    try:
        for k, (env, want) in enumerate([(tex, (0, 1, (1, 1))), (None, (1, 2, (1, 2))), (tex, (1, 3, (1, 3)))]):
            pt.set_environment(env)
            m.set_environment(env)
            model_batch(pt, m, w * h, 1 + 3 * k, k)
            assert counters(pt) == want, k
    finally:
        pt.pathtraceFree()


@pytest.mark.parametrize("w, h", FRAMES)
def test_textures_set_removed_and_one_set_back(pt, po, scenes, w, h):
    """PT_TEXTURES without PT_GLOSSY on cornell_textured against texture_model.Model.  Textures set: the TEX forms, no table --
    (0, 0, (0, 0)); all removed: the session launches what one without the flag does, and the tables are filled at that moment
    -- (1, 1, (1, 1)); one set back: the TEX forms again -- (1, 1, (1, 1))."""
    scn = pt.load_scene(os.path.join(ROOT, "scenes", "cornell_textured.txt"))
    cam = _resized(scn.camera, w, h)
    textures = dict(scn.textures)
    back = min(textures)
    m = tm.Model(po, scn.geoms, scn.materials, cam, scn.traceDepth)
    pt.pathtraceInit(pt.Scene(scn.geoms, scn.materials, cam, scn.traceDepth), flags=pt.PT_COMPACT | pt.PT_TEXTURES, max_batch=3)
    try:
        steps = [(textures, (0, 0, (0, 0))), ({k: None for k in textures}, (1, 1, (1, 1))), ({back: textures[back]}, (1, 1, (1, 1)))]
        for k, (change, want) in enumerate(steps):
            for mat, t in change.items():
                pt.set_texture(mat, t)
                m.set_texture(mat, t)
            model_batch(pt, m, w * h, 1 + 3 * k, k)
            assert counters(pt) == want, k
        assert m.tinted > 0
    finally:
        pt.pathtraceFree()


@pytest.mark.parametrize("w, h", FRAMES)
def test_lens_set_and_back_to_a_pinhole(pt, po, scenes, w, h):
    """A lens from the start: rays differ per sample, no table -- (0, 0, (0, 0)); pinhole: the tables are filled now --
    (1, 1, (1, 1)); lens again: nothing reads them -- (1, 1, (1, 1)); pinhole: the camera has not moved, no second fill --
    (2, 2, (1, 2))."""
    s = small(scenes, "cornell", w, h)
    init(pt, s, max_batch=3)
    try:
        image = None
        steps = [((0.4, 9.0), (0, 0, (0, 0))), ((0.0, 0.0), (1, 1, (1, 1))), ((0.4, 9.0), (1, 1, (1, 1))), ((0.0, 0.0), (2, 2, (1, 2)))]
        for k, (lens, want) in enumerate(steps):
            pt.set_lens(*lens)
            ref = tracer(po, s, image=image, **({"lens": lens} if lens[0] > 0 else {}))
            check_batch(pt, ref, s, 1 + 3 * k, 3, k)
            image = ref.image
            assert counters(pt) == want, k
    finally:
        pt.pathtraceFree()


@pytest.mark.parametrize("w, h", FRAMES)
def test_depth_changes_under_one_camera(pt, po, scenes, w, h):
    """traceDepth 1 -> 3 -> 2 -> 8 through pt_set_camera with the camera's bytes unchanged: one fill in all, at depth 1, by the
    first-hit form (there is no bounce 1) -- (0, 0, (1, 1)); its records are what a bounce 0 that is not the last leaves, and depth
    3 reads them -- (1, 1, (1, 2)); depth 2, where bounce 1 is the last -- (2, 2, (1, 3)); depth 8 -- (3, 3, (1, 4))."""
    s = with_depth(small(scenes, "cornell", w, h), 1)
    init(pt, s, max_batch=3)
    try:
        image = None
        for k, (depth, want) in enumerate([(1, (0, 0, (1, 1))), (3, (1, 1, (1, 2))), (2, (2, 2, (1, 3))), (8, (3, 3, (1, 4)))]):
            s = with_depth(s, depth)
            pt.set_camera(s["camera"], depth)
            ref = tracer(po, s, image=image)
            check_batch(pt, ref, s, 1 + 3 * k, 3, depth)
            image = ref.image
            assert counters(pt) == want, depth
    finally:
        pt.pathtraceFree()


@pytest.mark.parametrize("w, h", FRAMES)
def test_fill_on_a_lane_under_a_map_then_the_table_form(pt, po, scenes, w, h):
    """Four asynchronous batches of 3 under a map (the per-sample form; the first of them enqueues the fill of both tables from its
    lane), the map removed with no synchronisation of the caller's, four more (the table form, on other lanes than the one that
    filled): one synchronize, one image -- (4, 8, (1, 8))."""
    s = small(scenes, "cornell", w, h)
    tex = np.random.default_rng(4001).uniform(0, 2, (6, 4, 4, 3)).astype(np.float32)
    m = em.Model(po, s["geoms"], s["materials"], s["camera"], s["depth"])
    init(pt, s, max_batch=3)
    try:
        pt.set_environment(tex)
        for k in range(4):
            pt.trace_batch_async(1 + 3 * k, 3)
        pt.set_environment(None)
        for k in range(4, 8):
            pt.trace_batch_async(1 + 3 * k, 3)
        pt.synchronize()
        m.set_environment(tex)
        for it in range(1, 25):
            if it == 13:
                m.set_environment(None)
            want = m.iterate(it)
        assert (bits(pt.get_image(w * h)) == bits(want)).all()
        assert counters(pt) == (4, 8, (1, 8))
    finally:
        pt.pathtraceFree()


def test_free_and_init_between_glass_free_and_glass_scenes(pt, po, scenes):
    """pt_free / pt_init in a row: Cornell 64 x 4 (table and words), cornell_glass 31 x 29 (no table), Cornell 31 x 29 (table
    without words), Cornell 64 x 4 (words again)."""
    two_batches(pt, po, small(scenes, "cornell", 64, 4), 3, 3)
    two_batches(pt, po, small(scenes, "cornell_glass", 31, 29), 3, 3, taken=False)
    two_batches(pt, po, small(scenes, "cornell", 31, 29), 3, 3)
    two_batches(pt, po, small(scenes, "cornell", 64, 4), 3, 3)


@pytest.mark.parametrize("w, h", [(64, 4), (31, 29), (64, 48)])
def test_frames_without_the_scene_in_lds(pt, po, scenes, monkeypatch, w, h):
    """test_frames with the scene gathered from global memory (PTMI355_SCENE_LDS=0): the two other instantiations."""
    monkeypatch.setenv("PTMI355_SCENE_LDS", "0")
    two_batches(pt, po, small(scenes, "cornell", w, h), 3, 3)


def test_glossy_session_keeps_the_per_sample_form(pt, po, scenes):
    scn = pt.load_scene(os.path.join(ROOT, "scenes", "cornell_glossy.txt"))
    cam = _resized(scn.camera, 50, 37)
    m = gm.Model(po, scn.geoms, scn.materials, cam, scn.traceDepth)
    pt.pathtraceInit(pt.Scene(scn.geoms, scn.materials, cam, scn.traceDepth), flags=pt.PT_COMPACT | pt.PT_GLOSSY, max_batch=3)
    try:
        pt.trace_batch(1, 3)
        for it in range(1, 4):
            want = m.iterate(it)
        assert (bits(pt.get_image(50 * 37)) == bits(want)).all()
        assert first_two(pt) == 1 and first_state(pt) == 0
    finally:
        pt.pathtraceFree()


@pytest.mark.parametrize("what", ["non-compacting", "PT_CACHE_FIRST", "PT_AA_JITTER", "lens"])
def test_sessions_without_the_launch_of_two(pt, po, scenes, what):
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
        assert first_two(pt) == 0 and first_state(pt) == 0
    finally:
        pt.pathtraceFree()


def test_texture_set_does_not_take_it(pt, po, scenes):
    want, _, _ = tt.reference(pt, po, scenes, "textured")
    tt.session(pt, scenes, "textured", pt.PT_COMPACT, max_batch=2)
    try:
        tt.trace_two_then_two(pt, want)
        assert first_state(pt) == 0
    finally:
        pt.pathtraceFree()


def test_direct_light_at_depth_2_does_not_take_it(pt, po, scenes):
    """traceDepth 2 with lights to sample: bounce 1 is a DIRECT form, no launch of the two.  At depth 4 bounces 0 and 1 are plain
    (the lamp scene has no dielectric)."""
    g, mats, cam, _ = td.two_lamps(pt)
    glass = bool((mats["hasRefractive"] > 0).any())
    for depth, fused in ((2, 0), (4, 1)):
        m = dm.Model(po, g, mats, cam, depth)
        pt.pathtraceInit(pt.Scene(g, mats, cam, depth), flags=pt.PT_COMPACT | pt.PT_DIRECT_LIGHT, max_batch=2)
        try:
            pt.trace_batch(1, 2)
            for it in (1, 2):
                want = m.iterate(it)
            assert (bits(pt.get_image(td.W * td.H)) == bits(want)).all(), depth
            assert first_two(pt) == fused, depth
            assert first_state(pt) == (0 if glass else fused), depth
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
        assert first_hit(pt) == (1, 2) and first_state(pt) == 0
    finally:
        pt.pathtraceFree()


def test_asynchronous_batches_on_lanes(pt, po, scenes):
    s = small(scenes, "cornell")
    init(pt, s, max_batch=4)
    try:
        ref = tracer(po, s)
        for k in range(4):
            pt.trace_batch_async(1 + 4 * k, 4)
        cam2 = turned(s["camera"], 25.0)
        pt.set_camera(cam2, s["depth"])
        for k in range(4, 8):
            pt.trace_batch_async(1 + 4 * k, 4)
        pt.synchronize()
        ref.iterate_parallel(1, 16, 4)
        ref = tracer(po, s, cam=cam2, image=ref.image)
        ref.iterate_parallel(17, 16, 4)
        assert (bits(pt.get_image(W * H)) == bits(ref.image)).all()
        assert first_hit(pt) == (2, 8) and first_state(pt) == 8
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
        assert first_state(pt) == first_hit(pt)[1] >= 2
        cam2 = stepped_back(s["camera"], 30.0)
        scene.camera = cam2
        ref = tracer(po, s, cam=cam2, image=ref.image)
        for it in range(11, 21):
            img = pt.pathtrace(None, 0, it)
            ref.iterate(it)
            assert (bits(img) == bits(ref.image)).all(), it
        fills, launches = first_hit(pt)
        assert fills == 2 and first_state(pt) == launches >= 4
    finally:
        pt.pathtraceFree()


def test_tile_of_a_frame(pt, po, scenes):
    """Tile 1 of 3 (strips of 8 rows) of 64 x 48: records and words are indexed by the tile's local pixel."""
    s = small(scenes, "cornell")
    s = dict(s, camera=stepped_back(s["camera"], 30.0))
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
        assert first_state(pt) == 2
    finally:
        pt.pathtraceFree()


def test_session_over_two_contexts(pt, po, scenes):
    """devices = [0, 0]: each context has a table of its own; the counter sums the contexts."""
    s = small(scenes, "cornell")
    init(pt, s, max_batch=3, devices=[0, 0], tile=(0, 1, 8))
    try:
        ref = tracer(po, s)
        img = np.zeros((W * H, 3), dtype=np.float32)
        for iter0 in (1, 4):
            pt.trace_batch(iter0, 3, img)
            ref.iterate_parallel(iter0, 3, 3)
            assert (bits(img) == bits(ref.image)).all(), iter0
        assert first_state(pt) == 4 and first_hit(pt) == (2, 4)
    finally:
        pt.pathtraceFree()


def test_ab_control(pt, po, scenes, monkeypatch):
    """PTMI355_FIRST_STATE=0 (an experiments build only): the launch of the two shades bounce 0 per sample."""
    if not pt.has_experiments():
        pytest.skip("PTMI355_FIRST_STATE is read by -DPT_EXPERIMENTS builds only")
    monkeypatch.setenv("PTMI355_FIRST_STATE", "0")
    s = small(scenes, "cornell")
    init(pt, s, max_batch=3)
    try:
        ref = tracer(po, s)
        check_batch(pt, ref, s, 1, 3)
        assert first_state(pt) == 0 and first_two(pt) == 1
    finally:
        pt.pathtraceFree()
