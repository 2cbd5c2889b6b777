"""The cube face-normal table (csrc/pt_k_scene.hpp: k_face_normals, GREC_FACE): the exact-test pass no longer evaluates
normalize(transform * face) for every cube hit; the winner's normal comes from a per-(geom, face code) table built at
pt_init, and the best key carries the face code (geom << 4 | code << 1 | outside).  Normals, distances, materials and
the outside flag stay bit-identical to the oracle's loop over every primitive."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import __graft_entry__ as ge  # noqa: E402,F401
from gpu_common import pt, launch_plan, bits  # noqa: E402,F401

pytestmark = pytest.mark.gpu

SCALES = [(1.0, 1.0, 1.0), (2.0, 0.5, 3.0), (1e-3, 1e-3, 1e-3), (1e-5, 2.0, 1e-4), (0.01, 7.0, 0.2), (-1.0, 2.0, 0.5),
          (1.5, -0.25, 1.0), (-0.3, -0.3, -0.3), (40.0, 0.02, 1.0)]


def _cubes(pt, rng, scales):
    H = pt.host_binding.host_library()
    g = np.zeros(len(scales), dtype=pt.GEOM_DT)
    for k, c in enumerate(g):
        c["type"] = 1
        c["materialid"] = 1 + k % 4
        c["translation"] = rng.uniform(-2, 2, 3) + (0, 5, 0)
        c["rotation"] = rng.uniform(-180, 180, 3) if k % 3 else (0.0, 0.0, 0.0)
        c["scale"] = scales[k]
        H.pth_build_geom_matrices(g.ctypes.data + k * pt.GEOM_DT.itemsize)
    return g


def _face_rays(geom, rng, per_face=64):
    """Rays that hit each of the six faces of a cube from outside (entry face) and from inside (exit face): every face
    code 0..5 wins from both sides.  float32 [n, 6]."""
    T = geom["transform"].astype(np.float64).T
    out = []
    for axis in range(3):
        for s in (-1.0, 1.0):
            e = np.zeros(3)
            e[axis] = s
            target = 0.5 * e + rng.uniform(-0.4, 0.4, (per_face, 3)) * (1 - np.abs(e))
            for start in (2.5 * e + rng.uniform(-0.3, 0.3, (per_face, 3)), rng.uniform(-0.3, 0.3, (per_face, 3))):
                o = np.concatenate([start, np.ones((per_face, 1))], 1) @ T.T
                t = np.concatenate([target, np.ones((per_face, 1))], 1) @ T.T
                out.append(np.concatenate([o[:, :3], t[:, :3] - o[:, :3]], 1))
    return np.concatenate(out).astype(np.float32)


def _paths(pt, rays):
    p = np.zeros(len(rays), dtype=pt.PATH_DT)
    p["origin"], p["direction"] = rays[:, :3], rays[:, 3:]
    p["color"] = 1.0
    p["pixelIndex"] = np.arange(len(rays))
    p["remainingBounces"] = 8
    return p


def _check(pt, po, geoms, s, rays):
    paths = _paths(pt, rays)
    pt.pathtraceInit(pt.Scene(geoms, s["materials"], s["camera"], s["depth"]))
    got, got_out = pt.intersect_once(paths)
    pt.pathtraceFree()
    want, want_out = po.compute_intersections(paths.view(po.PATH_DT), geoms.view(po.GEOM_DT))
    assert (bits(got["t"]) == bits(want["t"])).all()
    assert (bits(got["normal"]) == bits(want["normal"])).all()
    assert (got["materialId"] == want["materialId"]).all()
    hit = want["t"] > 0
    assert (got_out[hit] == want_out[hit]).all()
    return want, want_out


@pytest.mark.parametrize("scene_lds", ["1", "0"])
def test_face_table_random_cubes(pt, po, scenes, monkeypatch, scene_lds):
    """Every face of rotated, non-uniformly scaled, tiny and mirrored (negative scale) cubes, hit from outside and from
    inside, each cube alone and all together: the table's normal equals the oracle's per-hit normal bit for bit -- with
    the records staged in LDS and gathered from global memory."""
    monkeypatch.setenv("PTMI355_SCENE_LDS", scene_lds)
    s = scenes["cornell"]
    rng = np.random.default_rng(2027)
    cubes = _cubes(pt, rng, SCALES)
    for k in range(len(cubes)):
        rays = _face_rays(cubes[k], rng)
        want, want_out = _check(pt, po, cubes[k:k + 1], s, rays)
        hit = want["t"] > 0
        assert hit.mean() > 0.8, k
        assert want_out[hit].min() == 0 and want_out[hit].max() == 1
    rays = np.concatenate([_face_rays(c, rng, 16) for c in cubes])
    _check(pt, po, np.concatenate([s["geoms"], cubes]), s, rays)


def test_tied_duplicates_report_the_lower_geom(pt, po, scenes):
    """Two cubes that occupy the same space -- a copy, and a mirror image (scale -1 along x: the same distances bit for
    bit, the opposite face code on the x faces) -- and two identical spheres, in both orders: every hit ties exactly
    in t, and the lower geom wins with its own material and face normal, as in the reference's strict t_min > t scan."""
    s = scenes["cornell"]
    rng = np.random.default_rng(7)
    H = pt.host_binding.host_library()
    base = _cubes(pt, rng, [(1.5, 0.75, 2.0)])[0]
    g = np.zeros(6, dtype=pt.GEOM_DT)
    for k in range(6):
        g[k] = base
        g[k]["materialid"] = 1 + k % 4
    g[1]["scale"] = (-1.5, 0.75, 2.0)
    for k in (3, 4):
        g[k]["type"] = 0
        g[k]["translation"] = base["translation"] + (6.0, 0.0, 0.0)
    g[5]["scale"] = (1.5, 0.75, -2.0)
    for k in range(6):
        H.pth_build_geom_matrices(g.ctypes.data + k * pt.GEOM_DT.itemsize)
    rays = np.concatenate([_face_rays(g[0], rng), _face_rays(g[3], rng, 32)])
    for order in ([0, 1, 2, 3, 4, 5], [1, 0, 5, 4, 3, 2]):
        geoms = g[order].copy()
        want, _ = _check(pt, po, geoms, s, rays)
        hit = want["t"] > 0
        assert hit.sum() > 600
        # the winner is the first geom of its kind in the list: cubes and spheres do not overlap
        cube_first, sphere_first = geoms["materialid"][0], geoms["materialid"][3]
        assert set(np.unique(want["materialId"][hit])) == {cube_first, sphere_first}


def test_many_primitives_from_global_memory(pt, po, scenes, monkeypatch):
    """400 random cubes and spheres with the scene gathered from global memory (PTMI355_SCENE_LDS=0): intersections of
    rays at every primitive, and the image and live counts of two iterations, equal the oracle's."""
    monkeypatch.setenv("PTMI355_SCENE_LDS", "0")
    import cull_model
    s = scenes["cornell_64"]
    rng = np.random.default_rng(31)
    H = pt.host_binding.host_library()
    ng = 400
    geoms = np.zeros(ng, dtype=pt.GEOM_DT)
    for g in geoms:
        g["type"] = rng.integers(2)
        g["materialid"] = rng.integers(len(s["materials"]))
        g["translation"] = rng.uniform(-4.5, 4.5, 3) + (0, 5, 0)
        g["rotation"] = rng.uniform(-180, 180, 3)
        g["scale"] = rng.uniform(0.1, 0.8, 3) * rng.choice([-1.0, 1.0], 3)
    geoms[0] = s["geoms"][0]                                         # the light
    for k in range(1, ng):
        H.pth_build_geom_matrices(geoms.ctypes.data + k * pt.GEOM_DT.itemsize)
    rays = cull_model.stress_rays(geoms, rng, per_geom=60)
    big = scenes["cornell"]
    _check(pt, po, geoms, big, rays)
    scene = pt.Scene(geoms, s["materials"], s["camera"], 4)
    ref = po.Tracer(geoms.view(po.GEOM_DT), s["materials"], s["camera"], 4, flags=po.F_COMPACT, trig=po.TRIG_SHARED)
    pt.pathtraceInit(scene, flags=pt.PT_COMPACT)
    for it in (1, 2):
        img = pt.pathtrace(None, 0, it)
        st = ref.iterate(it)
        assert list(pt.get_stats().live[:4]) == list(st.live[:4]), it
    assert img.tobytes() == ref.image.tobytes()
    pt.pathtraceFree()
