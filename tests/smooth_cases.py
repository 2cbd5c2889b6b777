"""The scenes, cameras and hostile records that tests/test_smooth_model_cpu.py and tests/test_gpu_smooth.py share (PT_SMOOTH_NORMALS;
DESIGN.md section 6.26): scenes/cornell_smooth.txt's content as the loader hands it over, varied in Python; every seed is literal."""
import os

import numpy as np

import direct_model as dm
import mesh_cases
import texture_model as tm
from gpu_common import _resized

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
W, H = 40, 26                     # the frames of the GPU module: 40 x 26 and, for the wide cases, 130 x 9
WIDE = (130, 9)
_cache = {}

CASES = ("cornell", "depth 1", "depth 2", "wide", "hostile", "glass", "one zero", "seventeen", "glossy")


def env_texels():
    return np.random.default_rng(4001).uniform(0, 2, (6, 4, 4, 3)).astype(F32)


def loaded(pt):
    if "loaded" not in _cache:
        _cache["loaded"] = pt.load_scene(os.path.join(ROOT, "scenes", "cornell_smooth.txt"))
    return _cache["loaded"]


def scene_arrays(pt, name):
    """(geoms, materials, camera, depth, triangles, meshes, normals [T, 3, 3]) of one case.
    cornell / depth 1 / depth 2 / wide: the scene file at depth 5, 1, 2 and at 130 x 9;
    hostile: every 7th triangle's normals face away (step 4), every 11th's are zero, every 13th's lean 80 degrees, one is NaN, one
    infinite, one of length 1e-20 and one of length 1e20;
    glass: the matte ball is a dielectric;  one zero: the mirror ball's normals are all zero;
    seventeen: nine more cubes on the floor (seventeen primitives);  glossy: the mirror has SPECEX 40."""
    s = loaded(pt)
    geoms, mats, tris, meshes = s.geoms.copy(), s.materials.copy(), s.triangles.copy(), s.meshes.copy()
    vn = s.vertex_normals.copy()
    w, h = WIDE if name == "wide" else (W, H)
    cam = _resized(s.camera, w, h)
    depth = {"depth 1": 1, "depth 2": 2}.get(name, 5)
    if name == "hostile":
        n = len(vn)
        vn[0::7] *= F32(-1)
        vn[3::11] = 0
        t = np.arange(5, n, 13)
        with np.errstate(all="ignore"):                                  # (a triangle of both progressions: NaN normals)
            lean = np.cross(vn[t, 0], np.array([0.3, 0.5, 0.8]))
            lean /= np.linalg.norm(lean, axis=1)[:, None]
            vn[t] = (vn[t] * np.cos(np.radians(80)) + lean[:, None, :] * np.sin(np.radians(80))).astype(F32)
        vn[2, 1, 0] = np.nan
        vn[4, 2] = np.inf
        vn[6] *= F32(1e-20)
        vn[8] *= F32(1e20)
    if name == "glass":
        glass = np.zeros(1, dtype=mats.dtype)
        glass["color"], glass["spec_color"], glass["hasRefractive"], glass["indexOfRefraction"] = 1, (0.9, 0.95, 1.0), 1, 1.5
        mats = np.concatenate([mats, glass])
        geoms["materialid"][6] = len(mats) - 1
    if name == "one zero":
        m = meshes[1]
        vn[int(m["first_triangle"]):int(m["first_triangle"]) + int(m["triangle_count"])] = 0
    if name == "seventeen":
        blocks = [dm.placed(pt.GEOM_DT, tm.CUBE, 2 + (k & 1), (-3 + 3 * (k % 3), 0.3, -3 + 3 * (k // 3)), (0.6, 0.6, 0.6), (0, 15 * k, 0)) for k in range(9)]
        geoms = np.concatenate([geoms] + blocks)
        assert len(geoms) == 17
    if name == "glossy":
        mats["spec_exponent"][4] = 40.0
    return geoms, mats, cam, depth, tris, meshes, vn


def quad(pt, m):
    """A flat quad (two triangles in y = 0, facing +y) whose six corner normals are the one vector m."""
    tris = np.zeros(2, dtype=pt.TRI_DT)
    tris["v0"] = [(-1, 0, -1), (-1, 0, -1)]
    tris["v1"] = [(-1, 0, 1), (1, 0, 1)]
    tris["v2"] = [(1, 0, 1), (1, 0, -1)]
    return tris, np.broadcast_to(np.asarray(m, dtype=F32), (2, 3, 3)).copy()


def hostile_records(pt, count=257):
    """`count` (triangle, ray) records on a 12-triangle soup (mesh_cases.soup): rays aimed at vertices, edge midpoints and centroids
    from either side; per-triangle normals that are the facet normal leaning per corner, zero, NaN, infinite, tangential, facing
    away, and of length 1e-20 and 1e20.  Returns (triangles, normals, tri, origins, dirs)."""
    rng = np.random.default_rng(2601)
    tris = mesh_cases.soup(pt.TRI_DT, rng, n=12)
    tris["v2"][1] = tris["v0"][1] + (tris["v1"][1] - tris["v0"][1]) * F32(0.5) + F32(0.3)      # (no sliver: a facet normal exists)
    v = np.stack([tris["v0"], tris["v1"], tris["v2"]], axis=1).astype(np.float64)
    fn = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    fn /= np.linalg.norm(fn, axis=1)[:, None]
    tg = v[:, 1] - v[:, 0]
    tg /= np.linalg.norm(tg, axis=1)[:, None]
    vn = np.stack([fn + 0.4 * (j - 1) * tg for j in range(3)], axis=1)
    vn[1] = 0
    vn[2, 1, 1] = np.nan
    vn[3, 0] = np.inf
    vn[4] = tg[4]
    vn[5] *= -1
    vn[6] *= 1e-20
    vn[7] *= 1e20
    vn[8, 2] = 0                                                         # one zero corner
    vn[9] /= np.linalg.norm(vn[9], axis=1)[:, None]                      # unit normals
    vn = vn.astype(F32)
    k = rng.integers(0, 12, count).astype(np.int32)
    k[:min(count, 12)] = np.arange(min(count, 12))
    bary = np.array([(1, 0, 0), (0, 1, 0), (0, 0, 1), (0.5, 0.5, 0), (0, 0.5, 0.5), (0.5, 0, 0.5), (1 / 3, 1 / 3, 1 / 3)])
    b = bary[np.arange(count) % 7]
    target = (v[k] * b[:, :, None]).sum(axis=1)
    side = np.where(np.arange(count) % 5 == 3, -1.0, 1.0)               # every fifth from behind
    o = target + fn[k] * (side * rng.uniform(0.05, 4.0, count))[:, None] + rng.normal(size=(count, 3)) * 0.5
    d = target - o
    d /= np.linalg.norm(d, axis=1)[:, None]
    return tris, vn, k, o.astype(F32), d.astype(F32)
