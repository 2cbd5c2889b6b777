"""Texture mapping (PT_TEXTURES) on the CPU: the numpy model of tests/texture_model.py against the
oracle where a texture changes nothing or something exact, pt_texture_texel against the model, the census of texels reached, the
scene format's TEXTURE blocks and the refusals that need no device.  No GPU; frames of at most 24 x 24."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import __graft_entry__ as ge  # noqa: E402
import direct_model as dm  # noqa: E402
import environment_model as em  # noqa: E402
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
        _cache[key] = (s.geoms, s.materials, _resized(s.camera, w, h), s.traceDepth)
    return _cache[key]


def oracle_for(po, geoms, mats, cam, depth):
    return po.Tracer(np.ascontiguousarray(geoms).view(po.GEOM_DT), np.ascontiguousarray(mats).view(po.MATERIAL_DT), cam, depth,
                     flags=po.F_COMPACT, trig=po.TRIG_SHARED)


def turned_geoms(pt):
    """A turned, non-uniformly scaled cube, an ellipsoid and a mesh primitive."""
    return np.concatenate([dm.placed(pt.GEOM_DT, tm.CUBE, 0, (1.0, -2.0, 0.5), (2.0, 0.5, 3.0), (20.0, 35.0, -50.0)),
                           dm.placed(pt.GEOM_DT, tm.SPHERE, 0, (-1.0, 0.25, 4.0), (1.0, 2.5, 0.75), (10.0, 0.0, 70.0)),
                           dm.placed(pt.GEOM_DT, tm.MESH, 0, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))])


def to_world(g, q):
    """Object-space points through one primitive's transform, in float64 rounded once (input to the lookup)."""
    M = np.asarray(g["transform"], dtype=np.float64).T                   # stored m[col][row]
    q = np.asarray(q, dtype=np.float64)
    with np.errstate(all="ignore"):
        return (q @ M[:3, :3].T + M[:3, 3]).astype(F32)


# ---- pt_texture_texel -------------------------------------------------------------------------------------------------------------
def test_texture_texel_is_the_model(pt):
    geoms = turned_geoms(pt)
    rng = np.random.default_rng(11)
    d, _ = em.edge_directions()
    faces = []                                                           # all six faces, their edges and corners, in object space
    for axis in range(3):
        for s in (-0.5, 0.5):
            for a in (-0.5, -0.2, 0.0, 0.3, 0.5):
                for b in (-0.5, 0.1, 0.5):
                    q = [0.0, 0.0, 0.0]
                    q[axis], q[(axis + 1) % 3], q[(axis + 2) % 3] = s, a, b
                    faces.append(q)
    obj = np.concatenate([d[np.isfinite(d).all(axis=1)].astype(np.float64), np.array(faces), rng.normal(size=(300, 3))])
    for n in (1, 4, 7, 1024):
        for g in range(3):
            pts = np.concatenate([to_world(geoms[g], obj), d])           # ... and the raw cases: NaN and zero points among them
            h = np.full(len(pts), g, dtype=np.int32)
            got = pt.texture_texel(geoms, h, pts, n)
            want = tm.texel_index(geoms, h, pts, n)
            assert (got == want).all(), (n, g)
            if g == 2:
                assert (got == -1).all()                                 # a mesh has no parametrisation
            else:
                assert (got >= 0).sum() > 300 and (got < 6 * n * n).all()
    # identity primitives: the lookup is the environment's on the point itself, hand-pinned cases included
    unit = np.concatenate([dm.placed(pt.GEOM_DT, tm.CUBE, 0, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)),
                           dm.placed(pt.GEOM_DT, tm.SPHERE, 0, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))])
    d, k = em.edge_directions()
    fin = np.isfinite(d).all(axis=1) | np.isnan(d).any(axis=1)           # (0 * inf = NaN in the matrix product: the model's to say)
    for g in (0, 1):
        got = pt.texture_texel(unit, np.full(len(d), g, np.int32), d, 4)
        assert (got[fin] == k[fin]).all() and fin.sum() >= len(d) - 2
        assert (got == tm.texel_index(unit, np.full(len(d), g), d, 4)).all()
    nan = np.array([[np.nan, 0, 0], [0, 0, 0], [-0.0, 0.0, 0.0], [np.nan, np.nan, np.nan]], dtype=F32)
    assert (pt.texture_texel(unit, np.zeros(4, np.int32), nan, 4) == -1).all()
    assert len(pt.texture_texel(unit, np.zeros(0, np.int32), np.zeros((0, 3), F32), 4)) == 0


def test_texture_texel_refusals(pt):
    L = pt.library()
    geoms = turned_geoms(pt)
    h = np.zeros(2, dtype=np.int32)
    p = np.ones((2, 3), dtype=F32)
    out = np.zeros(2, dtype=np.int32)

    def call(g, ng, hh, pp, count, n, oo):
        return L.pt_texture_texel(None if g is None else g.ctypes.data, ng, None if hh is None else hh.ctypes.data,
                                  None if pp is None else pp.ctypes.data, count, n, None if oo is None else oo.ctypes.data)

    assert call(geoms, 3, h, p, 2, 4, out) == 0
    assert call(geoms, 3, None, None, 0, 4, None) == 0
    for bad in ((geoms, 3, h, p, -1, 4, out), (geoms, 3, None, p, 2, 4, out), (geoms, 3, h, None, 2, 4, out), (geoms, 3, h, p, 2, 4, None),
                (None, 3, h, p, 2, 4, out), (geoms, 3, h, p, 2, 0, out), (geoms, 3, h, p, 2, 1025, out), (geoms, 3, h, p, 2, -4, out),
                (geoms, 3, np.array([0, 3], np.int32), p, 2, 4, out), (geoms, 3, np.array([-1, 0], np.int32), p, 2, 4, out)):
        assert call(*bad) < 0, bad[1:]
        assert b"pt_texture_texel" in L.pt_last_error()


def test_every_texel_is_reached(pt):
    """n = 4: hit points on a unit cube and on a unit sphere reach all 96 texels."""
    unit = np.concatenate([dm.placed(pt.GEOM_DT, tm.CUBE, 0, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)),
                           dm.placed(pt.GEOM_DT, tm.SPHERE, 0, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))])
    c = (np.arange(16) + 0.5) / 16.0 - 0.5
    a, b = (v.reshape(-1) for v in np.meshgrid(c, c))
    cube = []
    for axis in range(3):
        for s in (-0.5, 0.5):
            q = np.zeros((len(a), 3))
            q[:, axis] = s
            rest = [k for k in range(3) if k != axis]
            q[:, rest[0]], q[:, rest[1]] = a, b
            cube.append(q)
    cube = np.concatenate(cube).astype(F32)
    sphere = (cube / np.linalg.norm(cube, axis=1)[:, None] * 0.5).astype(F32)
    for g, pts in ((0, cube), (1, sphere)):
        k = pt.texture_texel(unit, np.full(len(pts), g, np.int32), pts, 4)
        assert (k == tm.texel_index(unit, np.full(len(pts), g), pts, 4)).all()
        assert sorted(set(k.tolist())) == list(range(96)), g


# ---- the model where the answer is the oracle's --------------------------------------------------------------------------------------
def test_model_without_texture_and_with_exact_textures_is_the_oracle(pt, po):
    geoms, mats, cam, depth = load(pt, "cornell_textured", 24, 20)
    plain = tm.Model(po, geoms, mats, cam, depth)
    ones = tm.Model(po, geoms, mats, cam, depth)
    half = tm.Model(po, geoms, mats, cam, depth)
    for m in range(len(mats)):
        ones.set_texture(m, np.ones((6, 3, 3, 3), dtype=F32))
        half.set_texture(m, np.full((6, 5, 5, 3), 0.5, dtype=F32))
    halved = mats.copy()
    halved["color"] = (mats["color"] * F32(0.5)).astype(F32)             # exact in binary32
    oracle, oracle_half = oracle_for(po, geoms, mats, cam, depth), oracle_for(po, geoms, halved, cam, depth)
    for it in (1, 2, 3):
        oracle.iterate(it)
        oracle_half.iterate(it)
        assert plain.iterate(it).tobytes() == oracle.image.tobytes(), it
        assert ones.iterate(it).tobytes() == oracle.image.tobytes(), it
        assert half.iterate(it).tobytes() == oracle_half.image.tobytes(), it
    assert plain.tinted == 0 and ones.tinted > 1000 and half.tinted == ones.tinted
    assert oracle.image.tobytes() != oracle_half.image.tobytes() and (oracle.image != 0).any()


def test_scene_textures_change_the_picture_where_they_should(pt, po):
    """cornell_textured.txt with its own textures: pixels differ from the plain oracle, and removing the textures again gives
    the plain model."""
    s = pt.load_scene(os.path.join(ROOT, "scenes", "cornell_textured.txt"))
    geoms, mats, cam, depth = load(pt, "cornell_textured", 24, 20)
    m = tm.Model(po, geoms, mats, cam, depth)
    for k, tex in s.textures.items():
        m.set_texture(k, tex)
    oracle = oracle_for(po, geoms, mats, cam, depth)
    m.iterate(1)
    oracle.iterate(1)
    assert m.tinted > 100 and (bits(m.image) != bits(oracle.image)).any()
    with np.errstate(all="ignore"):
        assert (m.image <= oracle.image).all()                           # every texel of the scene is <= 1
    for k in s.textures:
        m.set_texture(k, None)
    m.image[:] = 0
    assert m.iterate(1).tobytes() == oracle.image.tobytes()


# ---- the scene format ---------------------------------------------------------------------------------------------------------------
def test_loader_checker_is_checker_cubemap(pt):
    s = pt.load_scene(os.path.join(ROOT, "scenes", "cornell_textured.txt"))
    want = {5: (64, 8, (1, 1, 1), (.25, .3, .6)), 6: (32, 4, (1, 1, 1), (.2, .2, .2)), 0: (8, 8, (1, 1, 1), (.96, .96, .9))}
    assert sorted(s.textures) == sorted(want)
    for m, (n, cells, c0, c1) in want.items():
        assert s.textures[m].shape == (6, n, n, 3) and s.textures[m].dtype == F32
        assert s.textures[m].tobytes() == pt.checker_cubemap(n, cells, c0, c1).tobytes(), m
    for n, cells in ((1, 1), (5, 3), (8, 8), (7, 16)):                   # the integer rule, texel by texel
        assert pt.checker_cubemap(n, cells, (0, .5, 1), (1, 2, 3)).tobytes() == tm.checker(n, cells, (0, .5, 1), (1, 2, 3)).tobytes()
    assert len(s.geoms) == 8 and len(s.materials) == 7 and int(s.geoms["materialid"][3]) == 5
    with pytest.raises(pt.PtError):
        pt.checker_cubemap(0, 1, (0, 0, 0), (1, 1, 1))


def test_scene_without_texture_blocks_loads_as_before(pt, golden):
    z = golden["scenes"]
    s = pt.load_scene(os.path.join(ROOT, "scenes", "cornell.txt"))
    assert s.textures == {}
    assert s.geoms.tobytes() == z["cornell__geoms"].tobytes() and s.materials.tobytes() == z["cornell__materials"].tobytes()
    assert s.camera.tobytes() == z["cornell__camera"].tobytes() and s.traceDepth == int(z["cornell__depth"])


def test_pfm_texture_round_trips(pt, tmp_path):
    rng = np.random.default_rng(3)
    n = 5
    tex = rng.uniform(0, 2, (6, n, n, 3)).astype(F32)
    pt.save_pfm(str(tmp_path / "tex.pfm"), tex.reshape(-1, 3), n, 6 * n, 1.0)
    src = open(os.path.join(ROOT, "scenes", "cornell.txt")).read()
    (tmp_path / "scene.txt").write_text(src + "\n\nTEXTURE 1\nPFM tex.pfm\n\nTEXTURE 0\nCHECKER 2 2 0 0 0 1 1 1\n")
    s = pt.load_scene(str(tmp_path / "scene.txt"))
    base = pt.load_scene(os.path.join(ROOT, "scenes", "cornell.txt"))
    assert sorted(s.textures) == [0, 1]
    assert s.textures[1].tobytes() == tex.tobytes()
    assert s.textures[0].tobytes() == pt.checker_cubemap(2, 2, (0, 0, 0), (1, 1, 1)).tobytes()
    assert s.geoms.tobytes() == base.geoms.tobytes() and s.materials.tobytes() == base.materials.tobytes()
    for bad in ("TEXTURE 99\nCHECKER 2 2 0 0 0 1 1 1\n", "TEXTURE 0\nCHECKER 0 2 0 0 0 1 1 1\n", "TEXTURE 0\nPFM missing.pfm\n",
                "TEXTURE 0\nSTRIPES 2\n", "TEXTURE\nCHECKER 2 2 0 0 0 1 1 1\n"):
        (tmp_path / "bad.txt").write_text(src + "\n\n" + bad)
        with pytest.raises(pt.PtError):
            pt.load_scene(str(tmp_path / "bad.txt"))
    pt.save_pfm(str(tmp_path / "wide.pfm"), tex.reshape(-1, 3), 6 * n, n, 1.0)      # not n wide and 6 n tall
    (tmp_path / "bad.txt").write_text(src + "\n\nTEXTURE 0\nPFM wide.pfm\n")
    with pytest.raises(pt.PtError):
        pt.load_scene(str(tmp_path / "bad.txt"))


# ---- refusals that need no device ---------------------------------------------------------------------------------------------------
def test_set_and_get_texture_before_init(pt):
    pt.pathtraceFree()
    L = pt.library()
    tex = np.ones((6, 2, 2, 3), dtype=F32)
    n = C.c_int(7)
    assert L.pt_set_texture(0, tex.ctypes.data, 2) < 0 and b"pt_set_texture" in L.pt_last_error()
    assert L.pt_get_texture(0, None, 0, C.byref(n)) < 0 and b"pt_get_texture" in L.pt_last_error()
    with pytest.raises(pt.PtError):
        pt.set_texture(0, tex)
    with pytest.raises(pt.PtError):
        pt.get_texture(0)
    assert pt.PT_TEXTURES == 1 << 14
