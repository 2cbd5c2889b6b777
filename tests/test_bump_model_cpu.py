"""Bump mapping (PT_TEXTURES) on the CPU: the numpy model of tests/bump_model.py against the texture
model and the oracle where a bump map changes nothing, pt_bump_normal against the model, a closed form, a furnace that does not
depend on the model's own arithmetic, the scene format's BUMPMAP blocks, the refusals that need no device and the stand-alone
sanitizer driver.  No GPU; frames of at most 24 x 24."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import __graft_entry__ as ge  # noqa: E402
import bump_model as bm  # noqa: E402
import direct_model as dm  # noqa: E402
import environment_model as em  # noqa: E402
import glossy_model as gm  # noqa: E402
import texture_model as tm  # noqa: E402
from gpu_common import _resized, bits  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
_cache = {}


@pytest.fixture(scope="module")
def pt():
    p = ge.load_package()
    p.build()
    p.build_host()
    return p


def load(pt, name, w, h):
    key = (name, w, h)
    if key not in _cache:
        s = pt.load_scene(os.path.join(ROOT, "scenes", name + ".txt"))
        _cache[key] = (s.geoms, s.materials, _resized(s.camera, w, h), s.traceDepth, dict(s.bump_maps))
    return _cache[key]


def random_bump(n, seed=0, scale=0.5):
    return np.random.default_rng(77 * n + seed).normal(0, scale, (6, n, n, 3)).astype(F32)


def turned_geoms(pt):
    """A turned, non-uniformly scaled cube, an ellipsoid, a mesh primitive, and a cube and a sphere scaled 100 : 1."""
    return np.concatenate([dm.placed(pt.GEOM_DT, tm.CUBE, 0, (1.0, -2.0, 0.5), (2.0, 0.5, 3.0), (20.0, 35.0, -50.0)),
                           dm.placed(pt.GEOM_DT, tm.SPHERE, 0, (-1.0, 0.25, 4.0), (1.0, 2.5, 0.75), (10.0, 0.0, 70.0)),
                           dm.placed(pt.GEOM_DT, tm.MESH, 0, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)),
                           dm.placed(pt.GEOM_DT, tm.CUBE, 0, (0.0, 0.0, 0.0), (1.0, 100.0, 1.0)),
                           dm.placed(pt.GEOM_DT, tm.SPHERE, 0, (0.0, 0.0, 0.0), (100.0, 1.0, 1.0))])


def to_world(g, q):
    M = np.asarray(g["transform"], dtype=np.float64).T                   # stored m[col][row]
    with np.errstate(all="ignore"):
        return (np.asarray(q, dtype=np.float64) @ M[:3, :3].T + M[:3, 3]).astype(F32)


def surface_points():
    """Object-space points: all six faces with their edges and corners, the hand-pinned directions, random ones."""
    d, _ = em.edge_directions()
    faces = []
    for axis in range(3):
        for s in (-0.5, 0.5):
            for a in (-0.5, -0.2, 0.0, 0.3, 0.5):
                for b in (-0.5, 0.1, 0.5):
                    q = [0.0, 0.0, 0.0]
                    q[axis], q[(axis + 1) % 3], q[(axis + 2) % 3] = s, a, b
                    faces.append(q)
    return np.concatenate([d[np.isfinite(d).all(axis=1)].astype(np.float64), np.array(faces), np.random.default_rng(5).normal(size=(300, 3))]), d


def normals_and_dirs(geoms, g, pts, rng):
    """A plausible reported normal per point -- the outward normal of the face or of the ellipsoid, now and then its negative (a hit
    from inside) -- and ray directions of either side."""
    one = geoms[np.full(len(pts), g)]
    with np.errstate(all="ignore"):
        q = dm.multiply_mv(one["inverseTransform"], pts, 1)
        if int(geoms["type"][g]) == tm.SPHERE:
            nr = gm.normalize3(dm.multiply_mv(one["invTranspose"], q, 0)).astype(F32)
        else:
            ax = np.argmax(np.abs(q), axis=1)
            u = np.zeros((len(pts), 3), dtype=F32)
            u[np.arange(len(pts)), ax] = np.sign(q[np.arange(len(pts)), ax])
            nr = gm.normalize3(dm.multiply_mv(one["transform"], u, 0)).astype(F32)
    nr[::9] = -nr[::9]
    I = gm.random_unit(rng, len(pts))
    with np.errstate(all="ignore"):
        flip = gm.dot3(I, nr) > 0
    I[flip & (np.arange(len(pts)) % 4 != 0)] *= F32(-1)                  # three in four face the normal
    return nr, I


def same_normals(got, want, what):
    (gn, gf), (wn, wf) = got, want
    assert (gf == wf).all(), (what, np.nonzero(gf != wf)[0][:5])
    bad = (bits(gn) != bits(wn)).any(axis=1)
    assert not bad.any(), (what, int(bad.sum()), np.nonzero(bad)[0][:5])


# ---- pt_bump_normal ----------------------------------------------------------------------------------------------------------------
def test_bump_normal_is_the_model(pt):
    geoms = turned_geoms(pt)
    obj, raw = surface_points()
    rng = np.random.default_rng(23)
    rejected_late = 0
    for n, scale in ((1, 0.5), (4, 0.5), (7, 2.0), (1024, 0.5), (4, 400.0)):
        tex = random_bump(n, 1, scale)
        if n == 7:
            tex[1::3, :, :, 0] = np.nan                                   # NaN texels: not perturbed
            tex[:, 2, :, :2] = 0                                          # zero texels: not perturbed
        for g in range(len(geoms)):
            pts = np.concatenate([to_world(geoms[g], obj), raw])          # ... and the raw cases: NaN and zero points among them
            nr, I = normals_and_dirs(geoms, g, pts, rng)
            h = np.full(len(pts), g, dtype=np.int32)
            got = pt.bump_normal(geoms, h, pts, nr, I, tex)
            want = bm.bump_normal(geoms, h, pts, nr, I, tex)
            same_normals(got, want, (n, g))
            assert (bits(got[0][~got[1]]) == bits(nr[~got[1]])).all()      # not perturbed: the reported normal, bit for bit
            if g == 2:
                assert not got[1].any()                                   # a mesh has no parametrisation
            elif scale < 100:
                assert got[1].sum() > 100, (n, g, got[1].sum())
            with np.errstate(all="ignore"):
                length = np.sqrt((got[0][got[1]].astype(np.float64) ** 2).sum(axis=1))
                assert (np.abs(length - 1) < 1e-6).all()
                assert (gm.dot3(got[0][got[1]], nr[got[1]]) > 0).all() and (gm.dot3(I[got[1]], got[0][got[1]]) < 0).all()
                if scale >= 100 and g in (3, 4):
                    # a slope of hundreds under a 100 : 1 scale: the normal turns almost into the surface, and steps 7 / 8 reject
                    entered = (gm.dot3(I, nr) < 0) & (tm.texel_index(geoms, h, pts, n) >= 0)
                    rejected_late += int((entered & ~got[1]).sum())
    assert rejected_late > 50
    assert len(pt.bump_normal(geoms, np.zeros(0, np.int32), np.zeros((0, 3), F32), np.zeros((0, 3), F32), np.zeros((0, 3), F32), random_bump(2))[1]) == 0


def test_bump_normal_by_hand(pt):
    """The sign fix of step 7, the exit face of step 1, the zero texel of step 4 and the face's two in-plane axes of step 5."""
    unit = np.concatenate([dm.placed(pt.GEOM_DT, tm.CUBE, 0, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)),
                           dm.placed(pt.GEOM_DT, tm.SPHERE, 0, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))])
    tex = np.zeros((6, 1, 1, 3), dtype=F32)
    tex[..., 0], tex[..., 1] = 0.75, -0.25                                # (da, db) on every face
    x, nx = np.array([[1, 0, 0]], F32), np.array([[-1, 0, 0]], F32)
    P = np.array([[0.5, 0.1, 0.2]], F32)
    # cube, face +x from outside: u = (1, da, db), normalised
    ns, f = pt.bump_normal(unit, [0], P, x, nx, tex)
    want = np.array([1, 0.75, -0.25]) / np.linalg.norm([1, 0.75, -0.25])
    assert f[0] and np.abs(ns[0] - want).max() < 2e-7
    # cube from inside: the test reports the exit face, which the ray does not face
    ns, f = pt.bump_normal(unit, [0], P, x, x, tex)
    assert not f[0] and (ns[0] == x[0]).all()
    # sphere from inside: reported normal -x; u = 2 q + (0, da, db) points outwards and is turned round
    ns, f = pt.bump_normal(unit, [1], P, nx, x, tex)
    u = 2 * P[0].astype(np.float64) + (0, 0.75, -0.25)
    assert f[0] and ns[0, 0] < 0 and np.abs(ns[0] + u / np.linalg.norm(u)).max() < 2e-7
    same_normals((ns, f), bm.bump_normal(unit, [1], P, nx, x, tex), "inside")
    # faces -y and +z: a < b are (x, z) and (x, y)
    ns, f = pt.bump_normal(unit, [0, 0], np.array([[0.1, -0.5, 0.2], [0.1, 0.2, 0.5]], F32), np.array([[0, -1, 0], [0, 0, 1]], F32),
                           np.array([[0, 1, 0], [0, 0, -1]], F32), tex)
    assert f.all()
    assert np.abs(ns[0] - np.array([0.75, -1, -0.25]) / np.linalg.norm([0.75, -1, -0.25])).max() < 2e-7
    assert np.abs(ns[1] - np.array([0.75, -0.25, 1]) / np.linalg.norm([0.75, -0.25, 1])).max() < 2e-7
    # an all-zero map perturbs nothing
    ns, f = pt.bump_normal(unit, [0, 1], np.concatenate([P, P]), np.concatenate([x, x]), np.concatenate([nx, nx]), np.zeros((6, 2, 2, 3), F32))
    assert not f.any() and (ns == x).all()


def test_bump_normal_refusals(pt):
    L = pt.library()
    geoms = turned_geoms(pt)
    h = np.zeros(2, dtype=np.int32)
    p = np.ones((2, 3), dtype=F32)
    tex = random_bump(4).reshape(-1, 3)
    out = np.zeros((2, 3), dtype=F32)
    flag = np.zeros(2, dtype=np.uint8)
    ok = [geoms.ctypes.data, len(geoms), h.ctypes.data, p.ctypes.data, p.ctypes.data, p.ctypes.data, 2, tex.ctypes.data, 4, out.ctypes.data,
          flag.ctypes.data]
    assert L.pt_bump_normal(*ok) == 0
    for k, v in ((6, -1), (0, None), (2, None), (3, None), (4, None), (5, None), (7, None), (8, 0), (8, 1025), (8, -4), (9, None), (10, None)):
        bad = list(ok)
        bad[k] = v
        assert L.pt_bump_normal(*bad) < 0, k
        assert b"pt_bump_normal" in L.pt_last_error()
    for hb in ([0, len(geoms)], [-1, 0]):
        bad = list(ok)
        hb = np.array(hb, dtype=np.int32)
        bad[2] = hb.ctypes.data
        assert L.pt_bump_normal(*bad) < 0 and b"primitive" in L.pt_last_error()
    empty = list(ok)
    empty[6] = 0
    for k in (2, 3, 4, 5, 9, 10):
        empty[k] = None
    assert L.pt_bump_normal(*empty) == 0


# ---- the model where the answer is known ---------------------------------------------------------------------------------------------
def test_model_without_map_and_with_zero_maps_is_the_texture_model_and_the_oracle(pt, po):
    geoms, mats, cam, depth, _ = load(pt, "cornell_bumped", 24, 20)
    plain = bm.Model(po, geoms, mats, cam, depth)
    zero = bm.Model(po, geoms, mats, cam, depth)
    for m in range(len(mats)):
        zero.set_bump_map(m, np.zeros((6, 3, 3, 3), dtype=F32))
    textured = tm.Model(po, geoms, mats, cam, depth)
    oracle = po.Tracer(np.ascontiguousarray(geoms).view(po.GEOM_DT), np.ascontiguousarray(mats).view(po.MATERIAL_DT), cam, depth,
                       flags=po.F_COMPACT, trig=po.TRIG_SHARED)
    for it in (1, 2, 3):
        oracle.iterate(it)
        textured.iterate(it)
        assert plain.iterate(it).tobytes() == oracle.image.tobytes(), it
        assert zero.iterate(it).tobytes() == oracle.image.tobytes(), it
        assert textured.image.tobytes() == oracle.image.tobytes(), it
    assert plain.bumped == 0 and zero.bumped == 0 and zero.guarded == 0 and (oracle.image != 0).any()


def test_constant_slope_on_a_mirror_cube_in_closed_form(pt, po):
    """A constant-slope map (s, 0) on an axis-aligned unit mirror cube: the scattered direction is reflect(I, normalize(axis +
    s e_a)) -- here in float64 from the inputs.  The path from I to the direction has about fifteen roundings of 2^-24 on
    unit-scale values (the point, q, the divide, w, the normalise, the dot and the reflection): 9e-7; the bound is four times that."""
    s = 0.3
    cube = dm.placed(pt.GEOM_DT, tm.CUBE, 0, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    mats = np.zeros(1, dtype=pt.MATERIAL_DT)
    mats["color"], mats["spec_color"], mats["hasReflective"] = 1, 1, 1
    tex = np.zeros((6, 2, 2, 3), dtype=F32)
    tex[..., 0] = s
    rng = np.random.default_rng(41)
    n = 600
    paths = np.zeros(n, dtype=po.PATH_DT)
    target = rng.uniform(-0.4, 0.4, (n, 3))
    axis = rng.integers(0, 3, n)
    sign = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    target[np.arange(n), axis] = 0.5 * sign
    origin = target * 1.0
    origin[np.arange(n), axis] = sign * rng.uniform(2, 4, n)
    origin += rng.uniform(-1.5, 1.5, (n, 3)) * (np.arange(3)[None, :] != axis[:, None])
    paths["origin"] = origin.astype(F32)
    d = target - origin
    paths["direction"] = (d / np.linalg.norm(d, axis=1)[:, None]).astype(F32)
    paths["color"], paths["remainingBounces"], paths["pixelIndex"] = 1, 3, np.arange(n)
    g = np.ascontiguousarray(cube).view(po.GEOM_DT)
    isects, outside = po.compute_intersections(np.ascontiguousarray(paths), g, None, None)
    assert (isects["t"] > 0).all()
    hg = np.zeros(n, dtype=np.int32)
    stats = {}
    post = bm.shade_bumped(po, 1, 0, cube, mats, {}, {0: tex}, paths, isects, outside, hg, stats=stats)
    I = paths["direction"].astype(np.float64)
    nr = np.asarray(isects["normal"], dtype=np.float64).reshape(-1, 3)
    ax = np.argmax(np.abs(nr), axis=1)
    assert (ax == axis).all()
    u = nr.copy()
    u[np.arange(n), np.where(ax == 0, 1, 0)] = s                         # e_a: the earlier of the two in-plane axes
    ns = u / np.linalg.norm(u, axis=1)[:, None]
    facing = (I * ns).sum(axis=1) < -1e-3                                # step 8 holds with a margin
    want = I - 2 * (I * ns).sum(axis=1)[:, None] * ns
    leaves = (want * nr).sum(axis=1) > 1e-3                              # ... and the guard does not fire
    ok = facing & leaves
    assert ok.sum() > 400 and stats["bumped"] >= ok.sum()
    err = np.abs(post["direction"][ok].astype(np.float64) - want[ok]).max()
    print("closed form: %d records, max |error| %.3g" % (ok.sum(), err))
    assert err <= 4e-6
    assert (post["remainingBounces"][ok] == 2).all()
    plain = tm.shade_textured(po, 1, 0, cube, mats, {}, paths, isects, outside, hg)
    assert np.abs(plain["direction"][ok].astype(np.float64) - want[ok]).max() > 0.1      # the flat mirror is somewhere else


# ---- furnace: independent of the model's own arithmetic -----------------------------------------------------------------------------
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


def furnace_scene(pt, tmp_path):
    (tmp_path / "furnace.txt").write_text(FURNACE)
    s = pt.load_scene(str(tmp_path / "furnace.txt"))
    assert s.bump_maps[0].tobytes() == bm.studs(16, 3, 1.0).tobytes() and s.traceDepth == 4
    return s


def furnace_first_hits(po, s):
    paths = po.generate_rays(s.camera, s.traceDepth)
    isects, _ = po.compute_intersections(paths, np.ascontiguousarray(s.geoms).view(po.GEOM_DT), None, None)
    hit = np.zeros(24 * 24, dtype=bool)
    hit[paths["pixelIndex"]] = isects["t"] > 0
    return hit


def test_furnace(pt, po, tmp_path):
    """One matte ball of colour 0.5 with studs of slope 1.0 under a constant environment of 1.0, depth 4, 24 x 24, 4 iterations: a
    guarded direction leaves a convex body, so every sample of a pixel whose first hit is the ball is 0.5 and the pixel sums to
    exactly 2.0 per channel -- as it does without a map.  Without the guard some directions enter the ball and it does not."""
    s = furnace_scene(pt, tmp_path)
    hit = furnace_first_hits(po, s)
    assert 100 < hit.sum() < 24 * 24
    images = {}
    for name, maps, use_guard in (("plain", {}, True), ("bumped", s.bump_maps, True), ("no guard", s.bump_maps, False)):
        m = bm.Model(po, s.geoms, s.materials, s.camera, s.traceDepth, use_guard=use_guard)
        m.set_environment(np.ones((6, 1, 1, 3), dtype=F32))
        for k, t in maps.items():
            m.set_bump_map(k, t)
        for it in (1, 2, 3, 4):
            m.iterate(it)
        images[name] = (m.image.copy(), m.bumped, m.guarded)
    for name in ("plain", "bumped"):
        img = images[name][0]
        assert (img[hit] == F32(2.0)).all(), (name, np.unique(img[hit]))
        assert (img[~hit] == F32(4.0)).all()                              # the environment itself
    assert images["plain"][1] == 0 and images["bumped"][1] > 500 and images["bumped"][2] > 0
    broken = (images["no guard"][0][hit] != F32(2.0)).any(axis=1)
    print("furnace: %d first hits, %d perturbed, %d guarded, %d pixels off without the guard" % (hit.sum(), images["bumped"][1],
                                                                                                  images["bumped"][2], broken.sum()))
    assert broken.any()


# ---- the scene format ---------------------------------------------------------------------------------------------------------------
def test_loader_studs_is_studs_bumpmap(pt):
    s = pt.load_scene(os.path.join(ROOT, "scenes", "cornell_bumped.txt"))
    want = {5: (64, 8, 0.6), 6: (32, 4, 0.5), 4: (32, 6, 0.3)}
    assert sorted(s.bump_maps) == sorted(want) and s.textures == {}
    for m, (n, cells, slope) in want.items():
        assert s.bump_maps[m].shape == (6, n, n, 3) and s.bump_maps[m].dtype == F32
        assert s.bump_maps[m].tobytes() == pt.studs_bumpmap(n, cells, slope).tobytes(), m
        assert s.bump_maps[m].tobytes() == bm.studs(n, cells, slope).tobytes(), m
        assert set(np.unique(s.bump_maps[m]).tolist()) == {0.0, float(F32(slope)), -float(F32(slope))}
    for n, cells, slope in ((1, 1, 2.0), (5, 3, 0.1), (8, 8, -0.7), (7, 16, 1e-3), (1024, 1024, 0.25)):
        if n < 1024:
            assert pt.studs_bumpmap(n, cells, slope).tobytes() == bm.studs(n, cells, slope).tobytes(), (n, cells)
        else:                                                            # the largest map: one row and one column in Python integers
            big = pt.studs_bumpmap(n, cells, slope)
            side = [F32(slope) * F32(-1 if (v * cells * 4 // n) % 4 == 0 else 1 if (v * cells * 4 // n) % 4 == 3 else 0) for v in range(n)]
            assert big.shape == (6, n, n, 3) and (big[5, 1000, :, 0] == side).all() and (big[0, :, 7, 1] == side).all() and (big[..., 2] == 0).all()
    assert len(s.geoms) == 8 and len(s.materials) == 7 and int(s.geoms["materialid"][3]) == 5 and int(s.geoms["materialid"][6]) == 4
    with pytest.raises(pt.PtError):
        pt.studs_bumpmap(0, 1, 1.0)
    base = pt.load_scene(os.path.join(ROOT, "scenes", "cornell.txt"))
    assert base.bump_maps == {} and base.textures == {}


def test_pfm_bump_map_round_trips(pt, tmp_path):
    rng = np.random.default_rng(3)
    n = 5
    tex = rng.normal(0, 1, (6, n, n, 3)).astype(F32)
    pt.save_pfm(str(tmp_path / "bump.pfm"), tex.reshape(-1, 3), n, 6 * n, 1.0)
    src = open(os.path.join(ROOT, "scenes", "cornell.txt")).read()
    (tmp_path / "scene.txt").write_text(src + "\n\nBUMPMAP 1\nPFM bump.pfm\n\nBUMPMAP 0\nSTUDS 2 2 0.5\n\nTEXTURE 1\nCHECKER 2 2 0 0 0 1 1 1\n")
    s = pt.load_scene(str(tmp_path / "scene.txt"))
    base = pt.load_scene(os.path.join(ROOT, "scenes", "cornell.txt"))
    assert sorted(s.bump_maps) == [0, 1] and sorted(s.textures) == [1]
    assert s.bump_maps[1].tobytes() == tex.tobytes()
    assert s.bump_maps[0].tobytes() == pt.studs_bumpmap(2, 2, 0.5).tobytes()
    assert s.geoms.tobytes() == base.geoms.tobytes() and s.materials.tobytes() == base.materials.tobytes()
    for bad in ("BUMPMAP 99\nSTUDS 2 2 1\n", "BUMPMAP 0\nSTUDS 0 2 1\n", "BUMPMAP 0\nSTUDS 2 2\n", "BUMPMAP 0\nPFM missing.pfm\n",
                "BUMPMAP 0\nCHECKER 2 2 0 0 0 1 1 1\n", "BUMPMAP\nSTUDS 2 2 1\n", "TEXTURE 0\nSTUDS 2 2 1\n"):
        (tmp_path / "bad.txt").write_text(src + "\n\n" + bad)
        with pytest.raises(pt.PtError):
            pt.load_scene(str(tmp_path / "bad.txt"))


def test_scene_bump_maps_change_the_picture(pt, po):
    geoms, mats, cam, depth, maps = load(pt, "cornell_bumped", 24, 20)
    m = bm.Model(po, geoms, mats, cam, depth)
    for k, t in maps.items():
        m.set_bump_map(k, t)
    plain = tm.Model(po, geoms, mats, cam, depth)
    m.iterate(1)
    plain.iterate(1)
    assert m.bumped > 100 and (bits(m.image) != bits(plain.image)).any()
    for k in maps:
        m.set_bump_map(k, None)
    m.image[:] = 0
    assert m.iterate(1).tobytes() == plain.image.tobytes()


# ---- refusals that need no device ---------------------------------------------------------------------------------------------------
def test_set_and_get_bump_map_before_init(pt):
    pt.pathtraceFree()
    L = pt.library()
    tex = np.ones((6, 2, 2, 3), dtype=F32)
    n = C.c_int(7)
    assert L.pt_set_bump_map(0, tex.ctypes.data, 2) < 0 and b"pt_set_bump_map" in L.pt_last_error()
    assert L.pt_get_bump_map(0, None, 0, C.byref(n)) < 0 and b"pt_get_bump_map" in L.pt_last_error()
    with pytest.raises(pt.PtError):
        pt.set_bump_map(0, tex)
    with pytest.raises(pt.PtError):
        pt.get_bump_map(0)


# ---- the host code under the sanitizers ------------------------------------------------------------------------------------------------
def test_bump_host_code_under_the_sanitizers(tmp_path):
    """tests/tools/bump_main.cpp, a program of its own: STUDS and the steps behind pt_bump_normal (csrc/pt_bump.hpp) under
    AddressSanitizer and UBSan.  Nothing sanitized is loaded into this process."""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ not found")
    exe = str(tmp_path / "bump_main")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "tools", "bump_main.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "bump_main: ok" in r.stdout and not r.stderr, r.stdout + r.stderr
