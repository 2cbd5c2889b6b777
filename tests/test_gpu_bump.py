"""GPU parity, bump mapping (PT_TEXTURES; include/ptmi355.h): a cube bump map per material perturbs the
shading normal at hits on spheres and cubes.  Everything is compared bit for bit with the numpy model (tests/bump_model.py),
under both launch plans: the two probes, every pipeline that honours the flag, a bump map with and without a colour texture,
batches on the lanes, a window traced ahead across the removal of the maps, the stepping interface, a tile, two contexts, the
furnace, the G-buffer and the albedo, the refusals and the headless host.  Frames of 31 x 29, at most 4 iterations."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import __graft_entry__ as ge  # noqa: E402,F401
import bump_model as bm  # noqa: E402
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


def random_bump(n, seed=0, scale=0.8):
    t = np.random.default_rng(1000 * n + seed).normal(0, scale, (6, n, n, 3)).astype(F32)
    if n > 1:
        t[:, 0, :, :2] = 0                                               # a row of flat texels: not perturbed
    return t


def random_texture(n, seed=0):
    return np.random.default_rng(2000 * n + seed).uniform(0, 2, (6, n, n, 3)).astype(F32)


def env_texels():
    return np.random.default_rng(4001).uniform(0, 2, (6, 4, 4, 3)).astype(F32)


def bumped(pt):
    if "bumped" not in _cache:
        s = pt.load_scene(os.path.join(ROOT, "scenes", "cornell_bumped.txt"))
        _cache["bumped"] = (s.geoms, s.materials, _resized(s.camera, W, H), s.traceDepth, dict(s.bump_maps))
    return _cache["bumped"]


def probe_scene(pt):
    """cornell_bumped plus a glass ball (material 7) and a mesh primitive."""
    geoms, mats, _, _, _ = bumped(pt)
    glass = np.zeros(1, dtype=mats.dtype)
    glass["color"], glass["spec_color"], glass["hasRefractive"], glass["indexOfRefraction"] = 1, (0.9, 0.95, 1.0), 1, 1.5
    geoms = np.concatenate([geoms, dm.placed(pt.GEOM_DT, tm.SPHERE, 7, (-1.0, 7.0, 1.5), (3.5, 3.0, 3.5), (0.0, 25.0, 10.0)),
                            dm.placed(pt.GEOM_DT, tm.MESH, 6, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))])
    return geoms, np.concatenate([mats, glass])


# ---- the probes ----------------------------------------------------------------------------------------------------------------
def normal_records(pt, n):
    """n (primitive, world point, reported normal, ray direction) records on the primitives of probe_scene: points on and near the
    surfaces, some far away, a zero and a NaN object-space point; normals of either sign, directions of either side."""
    geoms, _ = probe_scene(pt)
    rng = np.random.default_rng(31 * n + 5)
    h = rng.integers(0, len(geoms), n).astype(np.int32)
    obj = rng.uniform(-0.5, 0.5, (n, 3))
    ax = rng.integers(0, 3, n)
    sign = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    obj[np.arange(n), ax] = 0.5 * sign                                   # on a face of the unit cube
    ball = geoms["type"][h] == tm.SPHERE
    obj[ball] = obj[ball] / np.linalg.norm(obj[ball], axis=1)[:, None] * 0.5
    obj[2::7] *= 30.0
    M = np.asarray(geoms["transform"][h], dtype=np.float64)              # [count, col, row]
    pts = (np.einsum("ncr,nc->nr", M[:, :3, :3], obj) + M[:, 3, :3]).astype(F32)
    u = np.zeros((n, 3))
    u[np.arange(n), ax] = sign
    Mn = np.where(ball[:, None, None], np.asarray(geoms["invTranspose"][h], dtype=np.float64), M)
    nr = np.einsum("ncr,nc->nr", Mn[:, :3, :3], np.where(ball[:, None], obj, u))
    with np.errstate(all="ignore"):
        nr = (nr / np.linalg.norm(nr, axis=1)[:, None]).astype(F32)
    nr[5::9] *= F32(-1)                                                  # hits from inside
    I = gm.random_unit(rng, n)
    with np.errstate(all="ignore"):
        away = gm.dot3(I, nr) > 0
    I[away & (np.arange(n) % 4 != 0)] *= F32(-1)
    if n > 8:
        pts[3] = geoms["translation"][h[3]]                              # the primitive's centre: object-space 0 (or next to it)
        pts[4] = np.nan
    return geoms, h, pts, nr, I


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_probe_bump_normal_equals_the_model(pt, n):
    geoms, h, pts, nr, I = normal_records(pt, n)
    for tn in (1, 4, 1024):
        tex = random_bump(tn)
        if tn == 4:
            tex[2, 1, :, 0] = np.nan
        got = pt.probe_bump_normal(geoms, h, pts, nr, I, tex)
        want = bm.bump_normal(geoms, h, pts, nr, I, tex)
        assert (got[1] == want[1]).all(), (tn, np.nonzero(got[1] != want[1])[0][:5])
        same(got[0], want[0], "n = %d" % tn)
        host = pt.bump_normal(geoms, h, pts, nr, I, tex)
        assert (host[1] == got[1]).all()
        same(host[0], got[0], "the host entry point")
        same(got[0][~got[1]], nr[~got[1]], "not perturbed: the reported normal")
        if n == 257:
            assert got[1].sum() > 60 and (~got[1]).sum() > 60 and not got[1][geoms["type"][h] == tm.MESH].any()
            waves = got[1][:256].reshape(4, 64)
            assert (waves.any(axis=1) & ~waves.all(axis=1)).all()        # perturbed and unperturbed lanes in every wave
    zero = pt.probe_bump_normal(geoms, h, pts, nr, I, np.zeros((6, 4, 4, 3), F32))
    assert not zero[1].any()
    same(zero[0], nr, "all-zero map")
    assert pt.probe_bump_normal(geoms, h[:0], pts[:0], nr[:0], I[:0], random_bump(4))[0].shape == (0, 3)


def test_probe_bump_normal_refusals(pt):
    geoms, h, pts, nr, I = normal_records(pt, 4)
    L = pt.library()
    tex = random_bump(2).reshape(-1, 3)
    out = np.zeros_like(pts)
    flag = np.zeros(4, dtype=np.uint8)
    ok = [geoms.ctypes.data, len(geoms), h.ctypes.data, pts.ctypes.data, nr.ctypes.data, I.ctypes.data, 4, tex.ctypes.data, 2, out.ctypes.data,
          flag.ctypes.data]
    assert L.pt_probe_bump_normal(*ok) == 0
    for k, v in ((6, -1), (6, (1 << 26) + 1), (0, None), (2, None), (3, None), (4, None), (5, None), (7, None), (8, 0), (8, 1025), (9, None),
                 (10, None)):
        bad = list(ok)
        bad[k] = v
        assert L.pt_probe_bump_normal(*bad) < 0, k
    bad = list(ok)
    hb = np.array([0, 1, len(geoms), 0], dtype=np.int32)
    bad[2] = hb.ctypes.data
    assert L.pt_probe_bump_normal(*bad) < 0 and b"primitive" in L.pt_last_error()
    empty = list(ok)
    empty[6] = 0
    assert L.pt_probe_bump_normal(*empty) == 0


def scatter_records(pt, po, n):
    """n (path, intersection, primitive) records inside probe_scene: random rays from inside the box -- some from inside the glass
    and the other balls --, their real nearest hits, every remainingBounces from 1 (the last bounce) up, a dead path, misses."""
    geoms, mats = probe_scene(pt)
    rng = np.random.default_rng(17 * n + 3)
    paths = np.zeros(n, dtype=po.PATH_DT)
    paths["origin"] = (rng.uniform(-4.5, 4.5, (n, 3)) + (0, 5, 0)).astype(F32)
    paths["origin"][1::5] = (np.array([-1.0, 7.0, 1.5]) + rng.uniform(-0.8, 0.8, (len(paths[1::5]), 3))).astype(F32)     # inside the glass
    paths["direction"] = gm.random_unit(rng, n)
    paths["direction"][::6] = (0, 0, 1)                                  # out of the open side: misses
    paths["color"] = rng.uniform(0, 1, (n, 3)).astype(F32)
    paths["pixelIndex"] = rng.integers(0, 4096, n)
    paths["remainingBounces"] = rng.integers(1, 4, n)
    if n > 8:
        paths["remainingBounces"][7] = 0
    g = np.ascontiguousarray(geoms[:-1]).view(po.GEOM_DT)               # (the mesh primitive has no triangles: never hit)
    isects, outside = po.compute_intersections(np.ascontiguousarray(paths), g, None, None)
    hg = tm.hit_geoms(po, g, None, None, paths, isects)
    return geoms, mats, paths, isects, outside, hg


def probe_maps(tn):
    return {0: random_bump(tn, 1), 4: random_bump(tn, 2, 1.5), 5: random_bump(tn, 3, 1.5), 6: random_bump(4, 4, 1.5), 7: random_bump(tn, 5)}


@pytest.mark.parametrize("deferred", [0, 1])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_probe_shade_scatter_bumped_equals_the_model(pt, po, n, deferred):
    geoms, mats, paths, isects, outside, hg = scatter_records(pt, po, n)
    tex = {5: random_texture(4, 2), 1: random_texture(4, 3)}
    for tn in (1, 4, 1024):
        maps = probe_maps(tn)
        stats = {}
        want = bm.shade_bumped(po, 3, 2, geoms, mats, tex, maps, paths, isects, outside, hg, stats=stats)
        got = pt.probe_shade_scatter_bumped(3, 2, mats, paths, isects, geoms, hg, tex, maps, outside=outside, deferred=bool(deferred))
        sc.assert_same_paths(got, want, (n, tn))                        # (a path that ends keeps the ray it came with)
        if n == 257 and tn == 4:
            # the records cover: every material kind, perturbed and not, the guard on a mirror and on a diffuse surface
            nrm, flag = bm.shading_normals(po, np.ascontiguousarray(geoms).view(po.GEOM_DT), maps, paths, isects, hg)
            mat = isects["materialId"]
            live = (isects["t"] > 0) & (paths["remainingBounces"] > 1)
            for m in (4, 5, 6, 7):
                assert (flag & live & (mat == m)).any() and (~flag & live & (mat == m)).any(), m
            assert ((mat == 7) & live & (outside == 0)).any() and ((mat == 7) & live & (outside != 0)).any()
            assert ((mat == 0) & (isects["t"] > 0)).any() and (~(isects["t"] > 0)).any() and (paths["remainingBounces"] == 1).any()
            loose = bm.shade_bumped(po, 3, 2, geoms, mats, tex, maps, paths, isects, outside, hg, use_guard=False)
            fired = (bits(loose["direction"]) != bits(want["direction"])).any(axis=1)
            assert (fired & (mat == 4)).any() and (fired & ((mat == 5) | (mat == 6))).any() and not (fired & (mat == 7)).any()
            assert stats["guarded"] == fired.sum()
            # perturbed lanes never defer: both forms of the call give these bytes (checked above for `deferred` 0 and 1), and they
            # differ from the unbumped shader's
            flat = pt.probe_shade_scatter_textured(3, 2, mats, paths, isects, geoms, hg, tex, outside=outside, deferred=bool(deferred))
            assert (bits(flat["direction"]) != bits(got["direction"])).any(axis=1)[flag & live & (mat != 0)].all()      # (0: the lamp, where paths end)
    textured = pt.probe_shade_scatter_textured(3, 2, mats, paths, isects, geoms, hg, tex, outside=outside, deferred=bool(deferred))
    zero = {m: np.zeros((6, 2, 2, 3), F32) for m in range(len(mats))}
    assert_paths_equal(pt.probe_shade_scatter_bumped(3, 2, mats, paths, isects, geoms, hg, tex, zero, outside=outside, deferred=bool(deferred)), textured, n)
    assert_paths_equal(pt.probe_shade_scatter_bumped(3, 2, mats, paths, isects, geoms, hg, tex, {}, outside=outside, deferred=bool(deferred)), textured, n)


def test_probe_shade_scatter_bumped_refusals(pt, po):
    geoms, mats, paths, isects, outside, hg = scatter_records(pt, po, 8)
    L = pt.library()
    g, m, p = np.ascontiguousarray(geoms), np.ascontiguousarray(mats), paths.copy()
    x, o, h = np.ascontiguousarray(isects), np.ascontiguousarray(outside, dtype=np.uint8), np.ascontiguousarray(hg, dtype=np.int32)
    tex = random_bump(2).reshape(-1, 3)
    tn, toff = np.zeros(len(m), np.int32), np.zeros(len(m), np.int32)
    bn, boff = np.zeros(len(m), np.int32), np.zeros(len(m), np.int32)
    bn[5] = 2
    ok = [3, 2, m.ctypes.data, len(m), p.ctypes.data, x.ctypes.data, o.ctypes.data, 8, 0, g.ctypes.data, len(g), h.ctypes.data,
          None, tn.ctypes.data, toff.ctypes.data, tex.ctypes.data, bn.ctypes.data, boff.ctypes.data]
    assert L.pt_probe_shade_scatter_bumped(*ok) == 0
    for k, v in ((7, -1), (7, (1 << 26) + 1), (3, 0), (2, None), (4, None), (5, None), (8, 2), (9, None), (11, None), (13, None), (14, None),
                 (15, None), (16, None), (17, None)):
        bad = list(ok)
        bad[k] = v
        assert L.pt_probe_shade_scatter_bumped(*bad) < 0, k
    for k, v in ((1, 1025), (2, -1)):
        bb = bn.copy()
        bb[k] = v
        bad = list(ok)
        bad[16] = bb.ctypes.data
        assert L.pt_probe_shade_scatter_bumped(*bad) < 0
    empty = list(ok)
    empty[7] = 0
    assert L.pt_probe_shade_scatter_bumped(*empty) == 0


# ---- whole pipelines -----------------------------------------------------------------------------------------------------------
FURNACE = """MATERIAL 0
RGB         .5 .5 .5
SPECEX      0
SPECRGB     0 0 0
REFL        0
REFR        0
REFRIOR     0
EMITTANCE   0

CAMERA
RES         24 24
FOVY        15
ITERATIONS  4
DEPTH       4
FILE        furnace
EYE         0.0 0.3 6
LOOKAT      0 0 0
UP          0 1 0

OBJECT 0
sphere
material 0
TRANS       0 0 0
ROTAT       10 20 30
SCALE       2.5 2.5 2.5

BUMPMAP 0
STUDS       16 3 1.0
"""


def scene_arrays(pt, scenes, name):
    """(geoms, materials, camera at W x H, depth, triangles, meshes, textures, bump maps)"""
    g, m, c, d, b = bumped(pt)
    if name == "bumped":
        return g, m, c, d, None, None, {}, b
    if name == "depth 1":
        return g, m, c, 1, None, None, {}, b
    if name == "both":                                               # a bump map and a colour texture on one material, and each alone
        return g, m, c, 4, None, None, {5: random_texture(4, 7), 1: random_texture(4, 8)}, {5: b[5], 6: b[6]}
    if name == "many primitives":                                    # 17 primitives: past the own-surface form's 15
        blocks = [dm.placed(pt.GEOM_DT, tm.CUBE, 5 + (k & 1), (-3 + 3 * (k % 3), 0.3, -3 + 3 * (k // 3)), (0.6, 0.6, 0.6), (0, 15 * k, 0)) for k in range(9)]
        return np.concatenate([g] + blocks), m, c, 4, None, None, {}, b
    if name == "mesh":                                               # a triangle soup of the matte ball's material: its map is ignored there
        import mesh_cases
        tris = mesh_cases.soup(pt.TRI_DT, np.random.default_rng(11), n=50)
        geoms, tris, meshes = pt.meshes.add_mesh(g, tris, material_id=6)
        return geoms, m, c, 4, tris, meshes, {}, b
    if name == "glossy":                                             # cornell_glossy: maps on a matte and on a lobed material
        s = pt.load_scene(os.path.join(ROOT, "scenes", "cornell_glossy.txt"))
        return s.geoms, s.materials, _resized(s.camera, W, H), s.traceDepth, None, None, {}, {1: random_bump(4, 9, 0.4), 4: random_bump(4, 10, 0.4)}
    raise KeyError(name)


def reference(pt, po, scenes, name, count=4, env=False, glossy=False, snapshots=False, drop_after=None):
    """The model's running sums after iterations 1 .. count (computed once per module, never written afterwards); drop_after:
    the bump maps are removed after that iteration."""
    key = (name, count, env, glossy, snapshots, drop_after)
    if key not in _cache:
        geoms, mats, cam, depth, tris, meshes, tex, maps = scene_arrays(pt, scenes, name)
        m = bm.Model(po, geoms, mats, cam, depth, tris=tris, meshes=meshes, glossy=glossy)
        for k, t in tex.items():
            m.set_texture(k, t)
        for k, t in maps.items():
            m.set_bump_map(k, t)
        if env:
            m.set_environment(env_texels())
        out, snaps = [], []
        for it in range(1, count + 1):
            per_bounce = [] if snapshots else None
            out.append(m.iterate(it, per_bounce).copy())
            snaps.append(per_bounce)
            if drop_after == it:
                for k in maps:
                    m.set_bump_map(k, None)
        for a in out:
            a.setflags(write=False)
        _cache[key] = (out, snaps, m.bumped)
    return _cache[key]


def session(pt, scenes, name, flags, maps=True, **kw):
    geoms, mats, cam, depth, tris, meshes, tex, bmaps = scene_arrays(pt, scenes, name)
    scene = pt.Scene(geoms, mats, cam, depth, triangles=tris, meshes=meshes) if tris is not None else pt.Scene(geoms, mats, cam, depth)
    pt.pathtraceInit(scene, flags=flags | pt.PT_TEXTURES, **kw)
    if maps:
        for k, t in bmaps.items():                                   # (the maps first: a session with a bump map and no texture yet)
            pt.set_bump_map(k, t)
        for k, t in tex.items():
            pt.set_texture(k, t)
    return depth, bmaps


def trace_two_then_two(pt, want):
    for it in (1, 2):
        same(pt.pathtrace(None, 0, it), want[it - 1], "iteration %d" % it)
    img = np.zeros((W * H, 3), dtype=F32)
    pt.trace_batch(3, 2, img)
    same(img, want[3], "batch of 2")
    same(pt.get_image(W * H), want[3], "device image")


PIPELINES = {"compact": lambda pt: pt.PT_COMPACT, "plain": lambda pt: 0, "sort fused": lambda pt: pt.PT_COMPACT | pt.PT_SORT_MATERIAL,
             "bvh": lambda pt: pt.PT_COMPACT | pt.PT_MESH_BVH}


@pytest.mark.parametrize("name, flags", [("bumped", "compact"), ("bumped", "plain"), ("bumped", "sort fused"),
                                         ("both", "compact"), ("both", "plain"), ("mesh", "compact"), ("mesh", "bvh"),
                                         ("many primitives", "compact"), ("depth 1", "compact")])
def test_pipelines(pt, po, scenes, launch_plan, name, flags):
    """Two pt_trace calls, then a pt_trace_batch of 2."""
    want, _, count = reference(pt, po, scenes, name)
    assert count > 100
    session(pt, scenes, name, PIPELINES[flags](pt), max_batch=2)
    try:
        trace_two_then_two(pt, want)
    finally:
        pt.pathtraceFree()


def test_glossy_and_environment_together(pt, po, scenes, launch_plan):
    """cornell_glossy under a 4 x 4 map with PT_GLOSSY: the ENV x GLOSSY x TEX instantiations, fused and sorted."""
    want, _, count = reference(pt, po, scenes, "glossy", env=True, glossy=True)
    assert count > 200
    for flags in (pt.PT_COMPACT, pt.PT_COMPACT | pt.PT_SORT_MATERIAL):
        session(pt, scenes, "glossy", flags | pt.PT_GLOSSY, max_batch=2)
        try:
            pt.set_environment(env_texels())
            trace_two_then_two(pt, want)
        finally:
            pt.pathtraceFree()


def test_asynchronous_batches_on_lanes(pt, po, scenes, launch_plan):
    want, _, _ = reference(pt, po, scenes, "bumped")
    session(pt, scenes, "bumped", pt.PT_COMPACT, max_batch=2)
    try:
        for k in range(2):
            pt.trace_batch_async(1 + 2 * k, 2)
        pt.synchronize()
        same(pt.get_image(W * H), want[3])
    finally:
        pt.pathtraceFree()


def test_lookahead_window_across_the_removal_of_the_maps(pt, po, scenes, launch_plan):
    """PT_LOOKAHEAD | PT_PIN_IMAGE | PT_HOST_SPARSE: the maps are set and, two calls later, removed -- in the middle of a window
    traced ahead with them: the host image after every call is the model's."""
    want, _, _ = reference(pt, po, scenes, "bumped", drop_after=2)
    L = pt.library()
    buf = np.full((W * H, 3), -7.0, dtype=F32)
    _, maps = session(pt, scenes, "bumped", pt.PT_COMPACT | pt.PT_LOOKAHEAD | pt.PT_PIN_IMAGE | pt.PT_HOST_SPARSE, max_batch=8, pin_image=False)
    try:
        for it in (1, 2, 3, 4):
            assert L.pt_trace(None, 0, it, buf.ctypes.data) == 0, L.pt_last_error()
            same(buf, want[it - 1], "host image after iteration %d" % it)
            if it == 2:
                for k in maps:
                    pt.set_bump_map(k, None)
                assert all(pt.get_bump_map(k) is None for k in maps)
        same(pt.get_image(W * H), want[3], "device image")
    finally:
        pt.pathtraceFree()


@pytest.mark.parametrize("name", ["bumped", "depth 1"])
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
    """A session over two contexts (devices=[0, 0]: each with its own copy of the maps) delivers the frame; a session that is tile
    1 of 2 (strips of 8 rows) its own rows, zeros elsewhere."""
    want, _, _ = reference(pt, po, scenes, "bumped")
    kw = dict(devices=[0, 0]) if form == "devices" else dict(tile=(1, 2, 8))
    own = np.ones(H, dtype=bool) if form == "devices" else (np.arange(H) // 8) % 2 == 1
    mask = np.repeat(own, W)

    def expect(a):
        return np.where(mask[:, None], a, F32(0))

    _, maps = session(pt, scenes, "bumped", pt.PT_COMPACT, max_batch=2, **kw)
    try:
        for it in (1, 2):
            same(pt.pathtrace(None, 0, it), expect(want[it - 1]), "iteration %d" % it)
        img = np.zeros((W * H, 3), dtype=F32)
        pt.trace_batch(3, 2, img)
        same(img, expect(want[3]), "batch")
        for k, t in maps.items():
            assert pt.get_bump_map(k).tobytes() == t.tobytes()
    finally:
        pt.pathtraceFree()


def test_furnace(pt, po, tmp_path, launch_plan):
    """One matte ball of colour 0.5 with studs of slope 1.0 under a constant environment of 1.0, depth 4, 24 x 24, 4 iterations
    through pt_trace_batch: every pixel whose first hit is the ball sums to exactly 2.0 per channel, every other to 4.0 -- whatever
    the model says (tests/test_bump_model_cpu.py has the model's side, and shows that the guard is what makes it so)."""
    (tmp_path / "furnace.txt").write_text(FURNACE)
    s = pt.load_scene(str(tmp_path / "furnace.txt"))
    paths = po.generate_rays(s.camera, s.traceDepth)
    isects, _ = po.compute_intersections(paths, np.ascontiguousarray(s.geoms).view(po.GEOM_DT), None, None)
    hit = np.zeros(24 * 24, dtype=bool)
    hit[paths["pixelIndex"]] = isects["t"] > 0
    assert 100 < hit.sum() < 24 * 24
    pt.pathtraceInit(pt.Scene(s.geoms, s.materials, s.camera, s.traceDepth), flags=pt.PT_COMPACT | pt.PT_TEXTURES, max_batch=4)
    try:
        pt.set_environment(np.ones((6, 1, 1, 3), dtype=F32))
        pt.set_bump_map(0, s.bump_maps[0])
        img = np.zeros((24 * 24, 3), dtype=F32)
        pt.trace_batch(1, 4, img)
        assert (img[hit] == F32(2.0)).all(), np.unique(img[hit])
        assert (img[~hit] == F32(4.0)).all()
    finally:
        pt.pathtraceFree()


# ---- what a map leaves alone ---------------------------------------------------------------------------------------------------
def test_gbuffer_and_albedo_are_unchanged_by_a_map(pt, scenes, launch_plan):
    geoms, mats, cam, depth, _, _, tex, maps = scene_arrays(pt, scenes, "both")
    got = []
    for with_maps in (False, True):
        pt.pathtraceInit(pt.Scene(geoms, mats, cam, depth), flags=pt.PT_COMPACT | pt.PT_TEXTURES, max_batch=2)
        try:
            for k, t in tex.items():
                pt.set_texture(k, t)
            if with_maps:
                for k, t in maps.items():
                    pt.set_bump_map(k, t)
            pt.pathtrace(None, 0, 1)
            gb = pt.gbuffer()
            alb = pt.albedo()
            if with_maps:
                pt.set_bump_map(5, None)                             # ... and the albedo plane is not invalidated
                assert pt.albedo().tobytes() == alb.tobytes()
            got.append([gb[k].tobytes() for k in sorted(gb)] + [alb.tobytes()])
        finally:
            pt.pathtraceFree()
    assert got[0] == got[1]


def test_all_zero_maps_are_the_plain_oracle(pt, po, scenes, launch_plan):
    geoms, mats, cam, depth, _, _, _, _ = scene_arrays(pt, scenes, "bumped")
    oracle = po.Tracer(np.ascontiguousarray(geoms).view(po.GEOM_DT), np.ascontiguousarray(mats).view(po.MATERIAL_DT), cam, depth,
                       flags=po.F_COMPACT, trig=po.TRIG_SHARED)
    session(pt, scenes, "bumped", pt.PT_COMPACT, maps=False, max_batch=2)
    try:
        for m in range(len(mats)):
            pt.set_bump_map(m, np.zeros((6, 3, 3, 3), dtype=F32))
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


def test_get_bump_map_returns_what_was_set(pt, scenes, launch_plan):
    geoms, mats, cam, depth, _, _, _, maps = scene_arrays(pt, scenes, "bumped")
    session(pt, scenes, "bumped", pt.PT_COMPACT, max_batch=2)
    try:
        big = random_bump(1024, 5)
        pt.set_bump_map(2, big)
        pt.pathtrace(None, 0, 1)
        pt.set_camera(cam, depth)
        pt.clear_image()
        pt.set_texture(1, random_texture(4, 1))                      # the maps survive pt_set_texture
        for k, t in maps.items():
            got = pt.get_bump_map(k)
            assert got.shape == t.shape and got.tobytes() == t.tobytes(), k
        assert pt.get_bump_map(2).tobytes() == big.tobytes() and pt.get_bump_map(1) is None and pt.get_texture(2) is None
        L = pt.library()
        small = np.zeros((10, 3), F32)
        n = C.c_int(0)
        assert L.pt_get_bump_map(5, small.ctypes.data, 10, C.byref(n)) < 0 and n.value == 64      # too small: the size is reported
        pt.set_bump_map(2, None)
        assert pt.get_bump_map(2) is None
    finally:
        pt.pathtraceFree()


def interleaved_steps(pt, po):
    """Textures and bump maps of materials A < B set, replaced and removed in turn -- A's maps change size, which moves B's texels
    in the session's arrays -- on cornell_bumped at 40 x 26, depth 3.  Returns (geoms, materials, camera, depth, the materials looked
    at, steps [(kind, material, texels or None)], the running sum of iterations 1 and 2 after every step): the numpy model's, the
    plain oracle's once nothing is left.  Computed once per module, never written afterwards."""
    if "interleaved" not in _cache:
        geoms, mats, cam, _, _ = bumped(pt)
        cam, depth = _resized(cam, 40, 26), 3
        A, B, other = 1, 5, 6
        steps = [("bump", A, random_bump(4, 21)),                        # before any texture: the TEX forms read a texture table of zeros
                 ("texture", B, random_texture(1, 22)), ("texture", A, random_texture(3, 23)), ("texture", A, random_texture(4, 24)),
                 ("texture", B, None), ("bump", A, None), ("texture", A, None)]
        held = {"texture": {}, "bump": {}}
        want = []
        for kind, m, t in steps:
            held[kind][m] = t
            model = bm.Model(po, geoms, mats, cam, depth)
            for k, v in held["texture"].items():
                model.set_texture(k, v)
            for k, v in held["bump"].items():
                model.set_bump_map(k, v)
            for it in (1, 2):
                model.iterate(it)
            want.append(model.image.copy())
        assert all(v is None for d in held.values() for v in d.values())
        oracle = po.Tracer(np.ascontiguousarray(geoms).view(po.GEOM_DT), np.ascontiguousarray(mats).view(po.MATERIAL_DT), cam, depth,
                           flags=po.F_COMPACT, trig=po.TRIG_SHARED)
        for it in (1, 2):
            oracle.iterate(it)
        want[-1] = oracle.image.copy()
        for k in range(1, len(want)):                                    # every step shows in the picture
            assert (bits(want[k]) != bits(want[k - 1])).any(), k
        for a in want:
            a.setflags(write=False)
        _cache["interleaved"] = (geoms, mats, cam, depth, (A, B, other), steps, want)
    return _cache["interleaved"]


def test_interleaved_set_replace_remove(pt, po, launch_plan):
    """After every step of interleaved_steps: the getters give back what the test holds for each material, and a fresh render of
    two iterations is the model's bit for bit -- the maps of the materials a call did not name are where the new tables say."""
    geoms, mats, cam, depth, looked_at, steps, want = interleaved_steps(pt, po)
    pt.pathtraceInit(pt.Scene(geoms, mats, cam, depth), flags=pt.PT_COMPACT | pt.PT_TEXTURES, max_batch=2)
    try:
        held = {"texture": {}, "bump": {}}
        setters = {"texture": pt.set_texture, "bump": pt.set_bump_map}
        getters = {"texture": pt.get_texture, "bump": pt.get_bump_map}
        for k, (kind, m, t) in enumerate(steps):
            setters[kind](m, t)
            held[kind][m] = t
            for kind2 in held:
                for m2 in looked_at:
                    got, kept = getters[kind2](m2), held[kind2].get(m2)
                    assert (got is None) if kept is None else (got is not None and got.shape == kept.shape and got.tobytes() == kept.tobytes()), \
                        (k, kind2, m2)
            pt.clear_image()
            pt.pathtrace(None, 0, 1)
            same(pt.pathtrace(None, 0, 2), want[k], "after step %d (%s of material %d)" % (k, kind, m))
    finally:
        pt.pathtraceFree()


def test_refusals(pt, scenes):
    geoms, mats, cam, depth, _, _, _, _ = scene_arrays(pt, scenes, "bumped")
    tex = np.ones((6, 2, 2, 3), dtype=F32)
    L = pt.library()
    k = C.c_int(0)

    def says(rc, text):                                              # PT_ERR_INVALID and the whole message
        assert rc == -1 and L.pt_last_error() == text.encode(), (rc, L.pt_last_error())

    pt.pathtraceFree()
    with pytest.raises(pt.PtError):                                  # before pt_init
        pt.set_bump_map(0, tex)
    pt.pathtraceInit(pt.Scene(geoms, mats, cam, depth), flags=pt.PT_COMPACT)        # a session without the flag
    try:
        with pytest.raises(pt.PtError):
            pt.set_bump_map(0, tex)
        with pytest.raises(pt.PtError):
            pt.get_bump_map(0)
        # (the flag is looked at before the material, the material before the size)
        says(L.pt_set_bump_map(-1, tex.ctypes.data, -1), "pt_set_bump_map: the session was not initialised with PT_TEXTURES")
        says(L.pt_get_bump_map(-1, None, 0, None), "pt_get_bump_map: the session was not initialised with PT_TEXTURES")
    finally:
        pt.pathtraceFree()
    pt.pathtraceInit(pt.Scene(geoms, mats, cam, depth), flags=pt.PT_COMPACT | pt.PT_TEXTURES)
    try:
        for m in (-1, len(mats)):
            with pytest.raises(pt.PtError):
                pt.set_bump_map(m, tex)
            with pytest.raises(pt.PtError):
                pt.get_bump_map(m)
            says(L.pt_set_bump_map(m, None, -1), "pt_set_bump_map: material %d outside [0, %d)" % (m, len(mats)))
            says(L.pt_get_bump_map(m, None, 0, None), "pt_get_bump_map: material %d outside [0, %d)" % (m, len(mats)))
        assert L.pt_set_bump_map(0, tex.ctypes.data, -1) < 0 and L.pt_set_bump_map(0, tex.ctypes.data, 1025) < 0
        for n in (-1, 1025):
            says(L.pt_set_bump_map(0, None, n), "pt_set_bump_map: n = %d outside [0, 1024]" % n)
        assert L.pt_set_bump_map(0, None, 2) < 0 and b"null" in L.pt_last_error()
        says(L.pt_set_bump_map(0, None, 2), "pt_set_bump_map: null texels with n = 2")
        assert L.pt_get_bump_map(0, None, 0, None) < 0
        says(L.pt_get_bump_map(0, None, 0, None), "pt_get_bump_map: null n")
        assert pt.get_bump_map(0) is None                            # a refused call changes nothing
        pt.set_bump_map(0, tex)
        out = np.zeros((24, 3), dtype=F32)
        says(L.pt_get_bump_map(0, out.ctypes.data, 23, C.byref(k)), "pt_get_bump_map: room for 23 texels, the map has 24")
        assert k.value == 2 and not out.any()
        says(L.pt_get_bump_map(0, None, 24, C.byref(k)), "pt_get_bump_map: room for 0 texels, the map has 24")
        assert L.pt_get_bump_map(0, out.ctypes.data, 24, C.byref(k)) == 0 and out.tobytes() == tex.tobytes()
        assert L.pt_set_bump_map(0, None, 0) == 0 and L.pt_set_bump_map(0, tex.ctypes.data, 0) == 0 and pt.get_bump_map(0) is None
    finally:
        pt.pathtraceFree()


def test_fake_shader_ignores_a_bump_map(pt, scenes, launch_plan):
    geoms, mats, cam, depth, _, _, _, maps = scene_arrays(pt, scenes, "bumped")
    imgs = []
    for flag in (0, pt.PT_TEXTURES):
        pt.pathtraceInit(pt.Scene(geoms, mats, cam, depth), flags=pt.PT_FAKE_SHADER | flag)
        try:
            if flag:
                for k, t in maps.items():
                    pt.set_bump_map(k, t)
            pt.pathtrace(None, 0, 1)
            imgs.append(pt.pathtrace(None, 0, 2).copy())
        finally:
            pt.pathtraceFree()
    assert imgs[0].tobytes() == imgs[1].tobytes() and (imgs[0] != 0).any()


# ---- the headless host ---------------------------------------------------------------------------------------------------------
def test_ptbench_bump_maps(pt, po, tmp_path):
    """ptbench --textures renders scenes/cornell_bumped.txt (here at 32 x 32, depth 3): the raw running sum it saves is the model's;
    without the switch, the plain model's."""
    w = h = 32
    iters = 3
    txt = open(os.path.join(ROOT, "scenes", "cornell_bumped.txt")).read()
    assert "RES         800 800" in txt and "DEPTH       8" in txt
    scene_file = tmp_path / "cornell_bumped.txt"
    scene_file.write_text(txt.replace("RES         800 800", "RES         %d %d" % (w, h)).replace("DEPTH       8", "DEPTH       3"))
    s = pt.load_scene(str(scene_file))
    assert s.traceDepth == 3 and len(s.bump_maps) == 3
    for switch in (["--textures"], []):
        out = tmp_path / ("bump%d" % len(switch))
        p = subprocess.run([pt.build_ptbench(), str(scene_file), "--iters", str(iters), "--save-sum", "--out", str(out)] + switch,
                           capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout + p.stderr
        assert ("bump maps: 3 of 7 materials" in p.stdout) == bool(switch)
        got = pt.load_pfm(str(out) + ".%dsamp.sum.pfm" % iters, w, h)
        m = bm.Model(po, s.geoms, s.materials, s.camera, s.traceDepth)
        if switch:
            for k, t in s.bump_maps.items():
                m.set_bump_map(k, t)
        for it in range(1, iters + 1):
            m.iterate(it)
        same(got, m.image, "ptbench %s" % " ".join(switch))
        assert (m.bumped > 0) == bool(switch)
