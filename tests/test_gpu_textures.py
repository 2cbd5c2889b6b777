"""GPU parity, texture mapping (PT_TEXTURES; include/ptmi355.h): a cube texture per material multiplies
material.color at hits on spheres and cubes.  Everything is compared bit for bit with the numpy model (tests/texture_model.py:
the oracle's own stages, shaded on a per-path material table), under both launch plans: the two probes, every pipeline that
honours the flag, batches on the lanes, a window traced ahead across a change of textures, the stepping interface, a tile, two
contexts, the refusals and the headless host.  Frames of 31 x 29 (899 paths: fourteen full waves and one of 3), at most 4
iterations."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import __graft_entry__ as ge  # noqa: E402,F401
import direct_model as dm  # noqa: E402
import glossy_model as gm  # noqa: E402
import scatter_common as sc  # noqa: E402
import texture_model as tm  # noqa: E402
from gpu_common import pt, launch_plan, bits, assert_paths_equal, _resized  # noqa: E402,F401

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 31, 29
F32 = np.float32
_cache = {}


def same(got, want, what=""):
    bad = (bits(got) != bits(want)).any(axis=-1)
    assert not bad.any(), "%s: %d of %d differ, first %d" % (what, bad.sum(), bad.size, np.nonzero(bad.reshape(-1))[0][0])


def random_texture(n, seed=0):
    return np.random.default_rng(1000 * n + seed).uniform(0, 2, (6, n, n, 3)).astype(F32)


def env_texels():
    return np.random.default_rng(4001).uniform(0, 2, (6, 4, 4, 3)).astype(F32)


def textured(pt):
    if "textured" not in _cache:
        s = pt.load_scene(os.path.join(ROOT, "scenes", "cornell_textured.txt"))
        _cache["textured"] = (s.geoms, s.materials, _resized(s.camera, W, H), s.traceDepth, dict(s.textures))
    return _cache["textured"]


# ---- the probes ----------------------------------------------------------------------------------------------------------------
def lookup_records(pt, n):
    """n (primitive, world point, colour) records on the primitives of cornell_textured and a mesh primitive: points on and
    near the surfaces, some far away, a zero and a NaN object-space point."""
    geoms, _, _, _, _ = textured(pt)
    geoms = np.concatenate([geoms, dm.placed(pt.GEOM_DT, tm.MESH, 1, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))])
    rng = np.random.default_rng(31 * n + 5)
    h = rng.integers(0, len(geoms), n).astype(np.int32)
    obj = rng.uniform(-0.5, 0.5, (n, 3))
    ax = rng.integers(0, 3, n)
    obj[np.arange(n), ax] = np.where(rng.random(n) < 0.5, -0.5, 0.5)     # on a face of the unit cube
    obj[1::5] = obj[1::5] / np.linalg.norm(obj[1::5], axis=1)[:, None] * 0.5
    obj[2::7] *= 30.0
    M = np.asarray(geoms["transform"][h], dtype=np.float64)              # [count, col, row]
    pts = (np.einsum("ncr,nc->nr", M[:, :3, :3], obj) + M[:, 3, :3]).astype(F32)
    if n > 8:
        pts[3] = geoms["translation"][h[3]]                              # the primitive's centre: object-space 0 (or next to it)
        pts[4] = np.nan
    col = rng.uniform(0, 1.5, (n, 3)).astype(F32)
    return geoms, h, pts, col


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_probe_texture_equals_the_model(pt, n):
    geoms, h, pts, col = lookup_records(pt, n)
    for tn in (1, 4, 1024):
        tex = random_texture(tn)
        got = pt.probe_texture(geoms, h, pts, tex, col)
        same(got, tm.tint(geoms, h, pts, tex, col), "n = %d" % tn)
        k = pt.texture_texel(geoms, h, pts, tn)
        assert (k == tm.texel_index(geoms, h, pts, tn)).all()
        same(got[k < 0], col[k < 0], "no texel: the colour as it is")
        if n == 257:
            assert (k < 0).any() and (k >= 0).sum() > 150 and (tn == 1 or len(np.unique(k)) > 5)
    same(pt.probe_texture(geoms, h, pts, np.ones((6, 4, 4, 3), F32), col), col, "all-1.0 texture")
    assert pt.probe_texture(geoms, h[:0], pts[:0], random_texture(4), col[:0]).shape == (0, 3)


def test_probe_texture_refusals(pt):
    geoms, h, pts, col = lookup_records(pt, 4)
    L = pt.library()
    tex = random_texture(2).reshape(-1, 3)
    out = np.zeros_like(col)
    ok = [geoms.ctypes.data, len(geoms), h.ctypes.data, pts.ctypes.data, 4, tex.ctypes.data, 2, col.ctypes.data, out.ctypes.data]
    assert L.pt_probe_texture(*ok) == 0
    for k, v in ((4, -1), (4, (1 << 26) + 1), (0, None), (2, None), (3, None), (5, None), (6, 0), (6, 1025), (7, None), (8, None)):
        bad = list(ok)
        bad[k] = v
        assert L.pt_probe_texture(*bad) < 0, k
    bad = list(ok)
    hb = np.array([0, 1, len(geoms), 0], dtype=np.int32)
    bad[2] = hb.ctypes.data
    assert L.pt_probe_texture(*bad) < 0 and b"primitive" in L.pt_last_error()
    empty = list(ok)
    empty[4] = 0
    assert L.pt_probe_texture(*empty) == 0


def scatter_records(pt, po, n):
    """n (path, intersection, primitive) records inside cornell_textured: random rays from inside the box, their real nearest
    hits, every remainingBounces from 1 (the last bounce) up, a few dead paths and misses."""
    geoms, mats, _, _, _ = textured(pt)
    rng = np.random.default_rng(17 * n + 3)
    paths = np.zeros(n, dtype=po.PATH_DT)
    paths["origin"] = (rng.uniform(-4.5, 4.5, (n, 3)) + (0, 5, 0)).astype(F32)
    paths["direction"] = gm.random_unit(rng, n)
    paths["direction"][::6] = (0, 0, 1)                                  # out of the open side: misses
    paths["color"] = rng.uniform(0, 1, (n, 3)).astype(F32)
    paths["pixelIndex"] = rng.integers(0, 4096, n)
    paths["remainingBounces"] = rng.integers(1, 4, n)
    if n > 8:
        paths["remainingBounces"][7] = 0
    g = np.ascontiguousarray(geoms).view(po.GEOM_DT)
    isects, outside = po.compute_intersections(np.ascontiguousarray(paths), g, None, None)
    hg = tm.hit_geoms(po, g, None, None, paths, isects)
    return geoms, mats, paths, isects, outside, hg


@pytest.mark.parametrize("deferred", [0, 1])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_probe_shade_scatter_textured_equals_the_model(pt, po, n, deferred):
    geoms, mats, paths, isects, outside, hg = scatter_records(pt, po, n)
    for tn in (1, 4, 1024):
        tex = {0: random_texture(tn, 1), 5: random_texture(tn, 2), 6: random_texture(4, 3), 4: random_texture(tn, 4)}
        want = tm.shade_textured(po, 3, 2, geoms, mats, tex, paths, isects, outside, hg)
        got = pt.probe_shade_scatter_textured(3, 2, mats, paths, isects, geoms, hg, tex, outside=outside, deferred=bool(deferred))
        sc.assert_same_paths(got, want, (n, tn))                        # (a path that ends keeps the ray it came with)
        ended = got["remainingBounces"] == 0
        assert (bits(got["origin"][ended]) == bits(paths["origin"][ended])).all() and (bits(got["direction"][ended]) == bits(paths["direction"][ended])).all()
    plain = pt.probe_shade_scatter(3, 2, mats, paths, isects, outside, bool(deferred))
    assert_paths_equal(pt.probe_shade_scatter_textured(3, 2, mats, paths, isects, geoms, hg, {}, outside=outside, deferred=bool(deferred)), plain, n)
    ones = {m: np.ones((6, 2, 2, 3), F32) for m in range(len(mats))}
    assert_paths_equal(pt.probe_shade_scatter_textured(3, 2, mats, paths, isects, geoms, hg, ones, outside=outside, deferred=bool(deferred)), plain, n)
    if n == 257:
        assert (bits(want["color"]) != bits(plain["color"])).any() and (hg < 0).any() and (hg == 7).any() and (hg == 3).any()


def test_probe_shade_scatter_textured_refusals(pt, po):
    geoms, mats, paths, isects, outside, hg = scatter_records(pt, po, 8)
    L = pt.library()
    g, m, p = np.ascontiguousarray(geoms), np.ascontiguousarray(mats), paths.copy()
    x, o, h = np.ascontiguousarray(isects), np.ascontiguousarray(outside, dtype=np.uint8), np.ascontiguousarray(hg, dtype=np.int32)
    tex = random_texture(2).reshape(-1, 3)
    tn, toff = np.zeros(len(m), np.int32), np.zeros(len(m), np.int32)
    tn[5] = 2
    ok = [3, 2, m.ctypes.data, len(m), p.ctypes.data, x.ctypes.data, o.ctypes.data, 8, 0, g.ctypes.data, len(g), h.ctypes.data,
          tex.ctypes.data, tn.ctypes.data, toff.ctypes.data]
    assert L.pt_probe_shade_scatter_textured(*ok) == 0
    for k, v in ((7, -1), (7, (1 << 26) + 1), (3, 0), (2, None), (4, None), (5, None), (8, 2), (9, None), (11, None), (12, None), (13, None),
                 (14, None)):
        bad = list(ok)
        bad[k] = v
        assert L.pt_probe_shade_scatter_textured(*bad) < 0, k
    hb = h.copy()
    hb[np.nonzero(x["t"] > 0)[0][0]] = len(g)
    bad = list(ok)
    bad[11] = hb.ctypes.data
    assert L.pt_probe_shade_scatter_textured(*bad) < 0 and b"primitive" in L.pt_last_error()
    tb = tn.copy()
    tb[1] = 1025
    bad = list(ok)
    bad[13] = tb.ctypes.data
    assert L.pt_probe_shade_scatter_textured(*bad) < 0
    empty = list(ok)
    empty[7] = 0
    assert L.pt_probe_shade_scatter_textured(*empty) == 0


# ---- whole pipelines -----------------------------------------------------------------------------------------------------------
def scene_arrays(pt, scenes, name):
    """(geoms, materials, camera at W x H, depth, triangles, meshes, textures)"""
    if name == "textured":
        g, m, c, d, t = textured(pt)
        return g, m, c, d, None, None, t
    if name == "depth 1":
        g, m, c, _, t = textured(pt)
        return g, m, c, 1, None, None, t
    if name == "one texture":                                        # Cornell, a random texture on the matte white of floor, ceiling and back wall
        s = scenes["cornell"]
        return s["geoms"], s["materials"], _resized(s["camera"], W, H), s["depth"], None, None, {1: random_texture(4, 7)}
    if name == "emitter":                                            # ... on the lamp: colour * (mcol * emittance)
        s = scenes["cornell"]
        return s["geoms"], s["materials"], _resized(s["camera"], W, H), s["depth"], None, None, {0: random_texture(4, 8)}
    if name == "many primitives":                                    # 17 primitives: past the own-surface form's 15
        g, m, c, _, t = textured(pt)
        blocks = [dm.placed(pt.GEOM_DT, tm.CUBE, 5 + (k & 1), (-3 + 3 * (k % 3), 0.3, -3 + 3 * (k // 3)), (0.6, 0.6, 0.6), (0, 15 * k, 0)) for k in range(9)]
        return np.concatenate([g] + blocks), m, c, 4, None, None, t
    if name == "mesh":                                               # a triangle soup of the matte ball's material: its texture is ignored there
        import mesh_cases
        g, m, c, _, t = textured(pt)
        tris = mesh_cases.soup(pt.TRI_DT, np.random.default_rng(11), n=50)
        geoms, tris, meshes = pt.meshes.add_mesh(g, tris, material_id=6)
        return geoms, m, c, 4, tris, meshes, t
    if name == "glossy":                                             # cornell_glossy: textures on a matte and on a lobed material
        s = pt.load_scene(os.path.join(ROOT, "scenes", "cornell_glossy.txt"))
        return s.geoms, s.materials, _resized(s.camera, W, H), s.traceDepth, None, None, {1: random_texture(4, 9), 4: random_texture(4, 10)}
    raise KeyError(name)


def reference(pt, po, scenes, name, count=4, env=False, glossy=False, snapshots=False, drop_after=None):
    """The model's running sums after iterations 1 .. count (computed once per module, never written afterwards); drop_after:
    the textures are removed after that iteration."""
    key = (name, count, env, glossy, snapshots, drop_after)
    if key not in _cache:
        geoms, mats, cam, depth, tris, meshes, tex = scene_arrays(pt, scenes, name)
        m = tm.Model(po, geoms, mats, cam, depth, tris=tris, meshes=meshes, glossy=glossy)
        for k, t in tex.items():
            m.set_texture(k, t)
        if env:
            m.set_environment(env_texels())
        out, snaps = [], []
        for it in range(1, count + 1):
            per_bounce = [] if snapshots else None
            out.append(m.iterate(it, per_bounce).copy())
            snaps.append(per_bounce)
            if drop_after == it:
                for k in tex:
                    m.set_texture(k, None)
        for a in out:
            a.setflags(write=False)
        _cache[key] = (out, snaps, m.tinted)
    return _cache[key]


def session(pt, scenes, name, flags, textures=True, **kw):
    geoms, mats, cam, depth, tris, meshes, tex = scene_arrays(pt, scenes, name)
    scene = pt.Scene(geoms, mats, cam, depth, triangles=tris, meshes=meshes) if tris is not None else pt.Scene(geoms, mats, cam, depth)
    pt.pathtraceInit(scene, flags=flags | pt.PT_TEXTURES, **kw)
    if textures:
        for k, t in tex.items():
            pt.set_texture(k, t)
    return depth, tex


def trace_two_then_two(pt, want):
    for it in (1, 2):
        same(pt.pathtrace(None, 0, it), want[it - 1], "iteration %d" % it)
    img = np.zeros((W * H, 3), dtype=F32)
    pt.trace_batch(3, 2, img)
    same(img, want[3], "batch of 2")
    same(pt.get_image(W * H), want[3], "device image")


PIPELINES = {"compact": lambda pt: pt.PT_COMPACT, "plain": lambda pt: 0, "sort fused": lambda pt: pt.PT_COMPACT | pt.PT_SORT_MATERIAL,
             "bvh": lambda pt: pt.PT_COMPACT | pt.PT_MESH_BVH}


@pytest.mark.parametrize("name, flags", [("textured", "compact"), ("textured", "plain"), ("textured", "sort fused"),
                                         ("one texture", "compact"), ("one texture", "plain"), ("one texture", "sort fused"),
                                         ("mesh", "compact"), ("mesh", "bvh"), ("mesh", "sort fused"), ("many primitives", "compact"),
                                         ("depth 1", "compact"), ("depth 1", "plain"), ("emitter", "compact")])
def test_pipelines(pt, po, scenes, launch_plan, name, flags):
    """Two pt_trace calls, then a pt_trace_batch of 2."""
    want, _, tinted = reference(pt, po, scenes, name)
    assert tinted > 100                                              # (the lamp alone is a small target: 179 hits in four frames)
    session(pt, scenes, name, PIPELINES[flags](pt), max_batch=2)
    try:
        trace_two_then_two(pt, want)
    finally:
        pt.pathtraceFree()


def test_glossy_and_environment_together(pt, po, scenes, launch_plan):
    """cornell_glossy under a 4 x 4 map with PT_GLOSSY: the ENV x GLOSSY x TEX instantiations, fused, sorted and uncompacted."""
    want, _, tinted = reference(pt, po, scenes, "glossy", env=True, glossy=True)
    assert tinted > 200
    for flags in (pt.PT_COMPACT, pt.PT_COMPACT | pt.PT_SORT_MATERIAL, 0):
        session(pt, scenes, "glossy", flags | pt.PT_GLOSSY, max_batch=2)
        try:
            pt.set_environment(env_texels())
            trace_two_then_two(pt, want)
        finally:
            pt.pathtraceFree()


def test_asynchronous_batches_on_lanes(pt, po, scenes, launch_plan):
    want, _, _ = reference(pt, po, scenes, "textured")
    session(pt, scenes, "textured", pt.PT_COMPACT, max_batch=2)
    try:
        for k in range(2):
            pt.trace_batch_async(1 + 2 * k, 2)
        pt.synchronize()
        same(pt.get_image(W * H), want[3])
    finally:
        pt.pathtraceFree()


def test_lookahead_window_across_a_change_of_textures(pt, po, scenes, launch_plan):
    """PT_LOOKAHEAD | PT_PIN_IMAGE | PT_HOST_SPARSE: the textures are set and, two calls later, removed -- in the middle of a
    window traced ahead with them: the host image after every call is the model's."""
    want, _, _ = reference(pt, po, scenes, "textured", drop_after=2)
    L = pt.library()
    buf = np.full((W * H, 3), -7.0, dtype=F32)
    _, tex = session(pt, scenes, "textured", pt.PT_COMPACT | pt.PT_LOOKAHEAD | pt.PT_PIN_IMAGE | pt.PT_HOST_SPARSE, max_batch=8, pin_image=False)
    try:
        for it in (1, 2, 3, 4):
            assert L.pt_trace(None, 0, it, buf.ctypes.data) == 0, L.pt_last_error()
            same(buf, want[it - 1], "host image after iteration %d" % it)
            if it == 2:
                for k in tex:
                    pt.set_texture(k, None)
                assert all(pt.get_texture(k) is None for k in tex)
        same(pt.get_image(W * H), want[3], "device image")
    finally:
        pt.pathtraceFree()


@pytest.mark.parametrize("name", ["textured", "depth 1"])
def test_stepping_interface(pt, po, scenes, launch_plan, name):
    want, snaps, _ = reference(pt, po, scenes, name, 2, snapshots=True)
    depth, _ = session(pt, scenes, name, pt.PT_COMPACT, max_batch=2)
    try:
        for it in (1, 2):
            pt.trace_begin(it, 1)
            for d in range(depth):
                n_live = pt.trace_bounce(d)
                paths, n = pt.export_paths(W * H)
                ref = snaps[it - 1][d] if d < len(snaps[it - 1]) else snaps[it - 1][-1][:0]
                assert n_live == n == len(ref), (it, d, n_live, n, len(ref))
                assert_paths_equal(paths, ref, n)
            pt.trace_end()
            same(pt.get_image(W * H), want[it - 1], "iteration %d" % it)
    finally:
        pt.pathtraceFree()


@pytest.mark.parametrize("form", ["devices", "tile"])
def test_tiles_and_devices(pt, po, scenes, launch_plan, form):
    """A session over two contexts (devices=[0, 0]: each with its own copy of the textures) delivers the frame; a session that is
    tile 1 of 2 (strips of 8 rows) its own rows, zeros elsewhere."""
    want, _, _ = reference(pt, po, scenes, "textured")
    kw = dict(devices=[0, 0]) if form == "devices" else dict(tile=(1, 2, 8))
    own = np.ones(H, dtype=bool) if form == "devices" else (np.arange(H) // 8) % 2 == 1
    mask = np.repeat(own, W)

    def expect(a):
        return np.where(mask[:, None], a, F32(0))

    _, tex = session(pt, scenes, "textured", pt.PT_COMPACT, max_batch=2, **kw)
    try:
        for it in (1, 2):
            same(pt.pathtrace(None, 0, it), expect(want[it - 1]), "iteration %d" % it)
        img = np.zeros((W * H, 3), dtype=F32)
        pt.trace_batch(3, 2, img)
        same(img, expect(want[3]), "batch")
        for k, t in tex.items():
            assert pt.get_texture(k).tobytes() == t.tobytes()
    finally:
        pt.pathtraceFree()


# ---- the flag ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ones", [False, True])
def test_no_texture_and_all_one_textures_are_the_plain_oracle(pt, po, scenes, launch_plan, ones):
    geoms, mats, cam, depth, _, _, _ = scene_arrays(pt, scenes, "textured")
    oracle = po.Tracer(np.ascontiguousarray(geoms).view(po.GEOM_DT), np.ascontiguousarray(mats).view(po.MATERIAL_DT), cam, depth,
                       flags=po.F_COMPACT, trig=po.TRIG_SHARED)
    session(pt, scenes, "textured", pt.PT_COMPACT, textures=False, max_batch=2)
    try:
        if ones:
            for m in range(len(mats)):
                pt.set_texture(m, np.ones((6, 3, 3, 3), dtype=F32))
        for it in (1, 2):
            st = oracle.iterate(it)
            same(pt.pathtrace(None, 0, it), oracle.image, "iteration %d" % it)
            gs = pt.get_stats()
            assert gs.bounces == st.bounces and list(gs.live[:depth]) == list(st.live[:depth])
        oracle.iterate_parallel(3, 2, 2)
        pt.trace_batch(3, 2)
        same(pt.get_image(W * H), oracle.image, "batch")
        assert (oracle.image != 0).any()
    finally:
        pt.pathtraceFree()


def test_get_texture_returns_what_was_set(pt, scenes, launch_plan):
    geoms, mats, cam, depth, _, _, tex = scene_arrays(pt, scenes, "textured")
    session(pt, scenes, "textured", pt.PT_COMPACT, max_batch=2)
    try:
        big = random_texture(1024, 5)
        pt.set_texture(2, big)
        pt.pathtrace(None, 0, 1)
        pt.set_camera(cam, depth)
        pt.clear_image()
        for k, t in tex.items():
            got = pt.get_texture(k)
            assert got.shape == t.shape and got.tobytes() == t.tobytes(), k
        assert pt.get_texture(2).tobytes() == big.tobytes() and pt.get_texture(1) is None
        L = pt.library()
        small = np.zeros((10, 3), F32)
        n = C.c_int(0)
        assert L.pt_get_texture(5, small.ctypes.data, 10, C.byref(n)) < 0 and n.value == 64      # too small: the size is reported
        pt.set_texture(2, None)
        assert pt.get_texture(2) is None
    finally:
        pt.pathtraceFree()


def test_refusals(pt, scenes):
    geoms, mats, cam, depth, _, _, _ = scene_arrays(pt, scenes, "textured")
    T = pt.PT_TEXTURES

    def refused(flags, word):
        with pytest.raises(pt.PtError) as e:
            try:
                pt.pathtraceInit(pt.Scene(geoms, mats, cam, depth), flags=flags)
            finally:
                pt.pathtraceFree()
        assert word in str(e.value), str(e.value)

    refused(T | pt.PT_UNFUSED, "PT_UNFUSED")
    refused(T | pt.PT_COMPACT | pt.PT_CACHE_FIRST, "PT_CACHE_FIRST")
    refused(T | pt.PT_SORT_MATERIAL, "two-kernel")                   # no compaction: the two-kernel form
    refused(T | pt.PT_COMPACT | pt.PT_DIRECT_LIGHT, "PT_DIRECT_LIGHT")
    tex = np.ones((6, 2, 2, 3), dtype=F32)
    L = pt.library()
    k = C.c_int(0)

    def says(rc, text):                                              # PT_ERR_INVALID and the whole message
        assert rc == -1 and L.pt_last_error() == text.encode(), (rc, L.pt_last_error())

    pt.pathtraceInit(pt.Scene(geoms, mats, cam, depth), flags=pt.PT_COMPACT)        # a session without the flag
    try:
        with pytest.raises(pt.PtError):
            pt.set_texture(0, tex)
        with pytest.raises(pt.PtError):
            pt.get_texture(0)
        # (the flag is looked at before the material, the material before the size)
        says(L.pt_set_texture(-1, tex.ctypes.data, -1), "pt_set_texture: the session was not initialised with PT_TEXTURES")
        says(L.pt_get_texture(-1, None, 0, None), "pt_get_texture: the session was not initialised with PT_TEXTURES")
    finally:
        pt.pathtraceFree()
    pt.pathtraceInit(pt.Scene(geoms, mats, cam, depth), flags=pt.PT_COMPACT | T)
    try:
        for m in (-1, len(mats)):
            with pytest.raises(pt.PtError):
                pt.set_texture(m, tex)
            with pytest.raises(pt.PtError):
                pt.get_texture(m)
            says(L.pt_set_texture(m, None, -1), "pt_set_texture: material %d outside [0, %d)" % (m, len(mats)))
            says(L.pt_get_texture(m, None, 0, None), "pt_get_texture: material %d outside [0, %d)" % (m, len(mats)))
        assert L.pt_set_texture(0, tex.ctypes.data, -1) < 0 and L.pt_set_texture(0, tex.ctypes.data, 1025) < 0
        for n in (-1, 1025):
            says(L.pt_set_texture(0, None, n), "pt_set_texture: n = %d outside [0, 1024]" % n)
        assert L.pt_set_texture(0, None, 2) < 0 and b"null" in L.pt_last_error()
        says(L.pt_set_texture(0, None, 2), "pt_set_texture: null texels with n = 2")
        assert L.pt_get_texture(0, None, 0, None) < 0
        says(L.pt_get_texture(0, None, 0, None), "pt_get_texture: null n")
        assert pt.get_texture(0) is None                             # a refused call changes nothing
        pt.set_texture(0, tex)
        out = np.zeros((24, 3), dtype=F32)
        says(L.pt_get_texture(0, out.ctypes.data, 23, C.byref(k)), "pt_get_texture: room for 23 texels, the texture has 24")
        assert k.value == 2 and not out.any()
        says(L.pt_get_texture(0, None, 24, C.byref(k)), "pt_get_texture: room for 0 texels, the texture has 24")
        assert L.pt_get_texture(0, out.ctypes.data, 24, C.byref(k)) == 0 and out.tobytes() == tex.tobytes()
        assert L.pt_set_texture(0, None, 0) == 0 and L.pt_set_texture(0, tex.ctypes.data, 0) == 0 and pt.get_texture(0) is None
    finally:
        pt.pathtraceFree()


def test_fake_shader_ignores_the_flag(pt, scenes, launch_plan):
    geoms, mats, cam, depth, _, _, tex = scene_arrays(pt, scenes, "textured")
    imgs = []
    for flag in (0, pt.PT_TEXTURES):
        pt.pathtraceInit(pt.Scene(geoms, mats, cam, depth), flags=pt.PT_FAKE_SHADER | flag)
        try:
            if flag:
                for k, t in tex.items():
                    pt.set_texture(k, t)
            pt.pathtrace(None, 0, 1)
            imgs.append(pt.pathtrace(None, 0, 2).copy())
        finally:
            pt.pathtraceFree()
    assert imgs[0].tobytes() == imgs[1].tobytes() and (imgs[0] != 0).any()
    pt.pathtraceInit(pt.Scene(geoms, mats, cam, depth), flags=pt.PT_FAKE_SHADER | pt.PT_TEXTURES | pt.PT_UNFUSED)    # not refused
    pt.pathtraceFree()


# ---- the headless host ---------------------------------------------------------------------------------------------------------
def test_ptbench_textures(pt, po, tmp_path):
    """ptbench --textures renders scenes/cornell_textured.txt (here at 32 x 32, depth 3): the raw running sum it saves is the
    model's; without the switch, the plain model's."""
    w = h = 32
    iters = 3
    txt = open(os.path.join(ROOT, "scenes", "cornell_textured.txt")).read()
    assert "RES         800 800" in txt and "DEPTH       8" in txt
    scene_file = tmp_path / "cornell_textured.txt"
    scene_file.write_text(txt.replace("RES         800 800", "RES         %d %d" % (w, h)).replace("DEPTH       8", "DEPTH       3"))
    s = pt.load_scene(str(scene_file))
    assert s.traceDepth == 3 and len(s.textures) == 3
    for switch in (["--textures"], []):
        out = tmp_path / ("tex%d" % len(switch))
        p = subprocess.run([pt.build_ptbench(), str(scene_file), "--iters", str(iters), "--save-sum", "--out", str(out)] + switch,
                           capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout + p.stderr
        assert ("textures: 3 of 7 materials" in p.stdout) == bool(switch)
        got = pt.load_pfm(str(out) + ".%dsamp.sum.pfm" % iters, w, h)
        m = tm.Model(po, s.geoms, s.materials, s.camera, s.traceDepth)
        if switch:
            for k, t in s.textures.items():
                m.set_texture(k, t)
        for it in range(1, iters + 1):
            m.iterate(it)
        same(got, m.image, "ptbench %s" % " ".join(switch))
        assert (m.tinted > 0) == bool(switch)
