"""Smooth shading of triangle meshes (PT_SMOOTH_NORMALS) on the CPU: the numpy model of
tests/smooth_model.py against the oracle where vertex normals change nothing, pt_smooth_normal against the model on hostile
records, its refusals, a flat quad in closed form, the coverage the GPU module's scenes give, the quality of a 320-triangle ball
against the analytic sphere, the loader's `vn` lines and the stand-alone sanitizer driver.  No GPU."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import __graft_entry__ as ge  # noqa: E402
import direct_model as dm  # noqa: E402
import glossy_model as gm  # noqa: E402
import smooth_cases as cases  # noqa: E402
import smooth_model as sm  # noqa: E402
import texture_model as tm  # noqa: E402
from gpu_common import _resized, bits, rel_l2  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


@pytest.fixture(scope="module")
def pt():
    p = ge.load_package()
    p.build()
    p.build_host()
    return p


def same(got, want, what=""):
    bad = (bits(got) != bits(want)).any(axis=-1)
    assert not bad.any(), "%s: %d of %d differ, first %d" % (what, bad.sum(), bad.size, np.nonzero(bad.reshape(-1))[0][0])


# ---- where normals change nothing ------------------------------------------------------------------------------------------------
def test_model_without_normals_and_with_zero_normals_is_the_oracle(pt, po):
    geoms, mats, cam, depth, tris, meshes, vn = cases.scene_arrays(pt, "cornell")
    cam = _resized(cam, 24, 20)
    oracle = po.Tracer(np.ascontiguousarray(geoms).view(po.GEOM_DT), np.ascontiguousarray(mats).view(po.MATERIAL_DT), cam, depth,
                       flags=po.F_COMPACT, trig=po.TRIG_SHARED, tris=np.ascontiguousarray(tris).view(po.TRI_DT),
                       meshes=np.ascontiguousarray(meshes).view(po.MESH_DT))
    plain = sm.Model(po, geoms, mats, cam, depth, tris=tris, meshes=meshes)
    zero = sm.Model(po, geoms, mats, cam, depth, tris=tris, meshes=meshes)
    zero.set_vertex_normals(np.zeros_like(vn))
    for it in (1, 2):
        oracle.iterate(it)
        same(plain.iterate(it), oracle.image, "no normals, iteration %d" % it)
        same(zero.iterate(it), oracle.image, "zero normals, iteration %d" % it)
    assert (oracle.image != 0).any() and zero.stats["smoothed"] == 0 and zero.stats["refused2"] > 100


# ---- pt_smooth_normal ----------------------------------------------------------------------------------------------------------
def test_smooth_normal_is_the_model_on_hostile_records(pt):
    tris, vn, k, o, d = cases.hostile_records(pt)
    stats = {}
    want = sm.smooth_normal(tris, vn, k, o, d, stats=stats)
    got = pt.smooth_normal(tris, vn, k, o, d)
    assert (got[1] == want[1]).all(), np.nonzero(got[1] != want[1])[0][:5]
    same(got[0], want[0], "pt_smooth_normal")
    same(got[0][~got[1]], sm.facet_normals(tris)[k][~got[1]], "not smoothed: the facet normal")
    # what the records cover: smoothed and every refusal; the zero, NaN, infinite, facing-away and 1e20 triangles are never smoothed,
    # the 1e-20 one is
    assert got[1].sum() > 40 and stats["refused2"] > 20 and stats["refused4"] > 10 and stats["refused5"] > 10
    for t in (1, 2, 3, 5, 7):
        assert not got[1][k == t].any(), t
    assert got[1][k == 6].any() and got[1][k == 9].any()
    # unit vectors (the 1e-20 triangle's l2 is a subnormal of a few bits: its normals are unit vectors to 1e-4 only)
    lens = np.linalg.norm(got[0].astype(np.float64), axis=1)
    assert np.abs(lens[got[1] & (k != 6)] - 1).max() < 1e-6 and np.abs(lens[got[1] & (k == 6)] - 1).max() < 1e-4
    assert pt.smooth_normal(tris, vn, k[:0], o[:0], d[:0])[0].shape == (0, 3)


def test_smooth_normal_refusals(pt):
    tris, vn, k, o, d = cases.hostile_records(pt, 4)
    L = pt.library()
    t, n = np.ascontiguousarray(tris), np.ascontiguousarray(vn)
    out = np.zeros((4, 3), dtype=F32)
    flag = np.zeros(4, dtype=np.uint8)
    ok = [t.ctypes.data, n.ctypes.data, len(t), k.ctypes.data, o.ctypes.data, d.ctypes.data, 4, out.ctypes.data, flag.ctypes.data]
    assert L.pt_smooth_normal(*ok) == 0
    for pos, v in ((6, -1), (2, -1), (0, None), (1, None), (3, None), (4, None), (5, None), (7, None), (8, None)):
        bad = list(ok)
        bad[pos] = v
        assert L.pt_smooth_normal(*bad) < 0, pos
    for entry in (-1, len(t)):
        kb = k.copy()
        kb[2] = entry
        bad = list(ok)
        bad[3] = kb.ctypes.data
        assert L.pt_smooth_normal(*bad) < 0 and b"tri[2]" in L.pt_last_error()
    empty = list(ok)
    empty[6] = 0
    assert L.pt_smooth_normal(*empty) == 0
    # the probe refuses the same before it looks for a device, and counts above 2^26
    for pos, v in ((6, -1), (6, (1 << 26) + 1), (0, None), (3, None), (8, None)):
        bad = list(ok)
        bad[pos] = v
        assert L.pt_probe_smooth_normal(*bad) < 0, pos
    assert L.pt_probe_smooth_normal(*empty) == 0                         # count == 0 launches nothing


def test_set_and_get_vertex_normals_before_init(pt):
    pt.pathtraceFree()
    with pytest.raises(pt.PtError):
        pt.set_vertex_normals(np.zeros((2, 3, 3), dtype=F32))
    with pytest.raises(pt.PtError):
        pt.get_vertex_normals()


def test_flat_quad_with_one_tilted_normal(pt):
    """Six corner normals that are one unit vector m: w_c = (m_c bw + m_c bx) + m_c by = m_c S (1 + e_c) with S = bw + bx + by and
    |e_c| <= 3 * 2^-24 (a product and two sums of terms of one sign: the rays hit inside the quad), and the normalise removes S: its
    own roundings (dot, sqrt, reciprocal, multiply) add about 2.75 * 2^-24 common to the components.  In the worst case that is
    5.75 * 2^-24 relative -- 2.9 ulp where an ulp is 2^-23 of the value, the coarsest it gets, just above a power of two, and more
    ulps for a larger mantissa.  m is therefore chosen with every component just above a power of two (0.5025, 0.7035, 0.5025); the
    roundings do not all align on the 200 fixed rays, and ns = m within 2 ulp per component."""
    m = np.array([0.5, 0.7, 0.5], dtype=np.float64)
    m = (m / np.linalg.norm(m)).astype(F32)
    tris, vn = cases.quad(pt, m)
    rng = np.random.default_rng(77)
    count = 200
    k = rng.integers(0, 2, count).astype(np.int32)
    target = np.stack([rng.uniform(-0.95, 0.95, count), np.zeros(count), rng.uniform(-0.95, 0.95, count)], axis=1)
    o = target + np.stack([rng.uniform(-1, 1, count), rng.uniform(0.5, 3, count), rng.uniform(-1, 1, count)], axis=1)
    d = target - o
    d /= np.linalg.norm(d, axis=1)[:, None]
    ns, flag = pt.smooth_normal(tris, vn, k, o.astype(F32), d.astype(F32))
    assert flag.sum() > 150
    ulp = np.spacing(np.abs(m))
    assert (np.abs(ns[flag].astype(np.float64) - m) <= 2 * ulp).all()
    same(ns, sm.smooth_normal(tris, vn, k, o.astype(F32), d.astype(F32))[0])


# ---- the scenes of the GPU module ------------------------------------------------------------------------------------------------
def test_coverage_floors_of_the_gpu_scenes(pt, po):
    """Conditions on the inputs of tests/test_gpu_smooth.py, computed from the model: its scenes and cameras reach a smoothed hit on a
    matte, a mirror and a glass material, a refusal at each of steps 2, 4 and 5, and a guard-changed direction on a matte and on a
    mirror surface."""
    total = {}
    for name in ("cornell", "hostile", "glass"):
        geoms, mats, cam, depth, tris, meshes, vn = cases.scene_arrays(pt, name)
        m = sm.Model(po, geoms, mats, cam, depth, tris=tris, meshes=meshes)
        m.set_vertex_normals(vn)
        for it in (1, 2):
            m.iterate(it)
        for key, v in m.stats.items():
            total[key] = total.get(key, 0) + v
        print(name, m.stats)
    for key in ("smoothed matte", "smoothed mirror", "smoothed glass", "refused2", "refused4", "refused5", "guarded matte", "guarded mirror"):
        assert total.get(key, 0) >= 1, (key, total)
    assert total["guarded glass"] == 0


# ---- quality ---------------------------------------------------------------------------------------------------------------------
def test_smooth_ball_is_closer_to_the_sphere_than_the_faceted_ball(pt, po):
    """The 320-triangle ball of scenes/ball_320.obj, matte under a sky, 64 x 64, 16 iterations, rendered by the model faceted,
    smooth and as the analytic sphere of the same centre and radius.  The sky is a vertical gradient, not a constant: under a
    constant sky every path that hits a convex matte body leaves it with albedo * sky whatever normal it was shaded about (the
    furnace of tests/test_gpu_smooth.py pins exactly that), so all three pictures would be the same bits and there would be no gap
    to measure.  The engine is keyed by (iteration, pixel, depth): the three share their draws and the gap is systematic.
    Measured (rel. L2 over the pixels all three hit, against the sphere): faceted and smooth are printed, and recorded in
    DESIGN.md section 6.26; the smooth value must lie below the faceted one by at least half the measured gap."""
    s = cases.loaded(pt)
    ball = s.meshes[0]
    first, count = int(ball["first_triangle"]), int(ball["triangle_count"])
    assert count == 320
    tris, vn = s.triangles[first:first + count].copy(), s.vertex_normals[first:first + count].copy()
    g = s.geoms[int(ball["geom_index"])]
    mats = np.zeros(1, dtype=pt.MATERIAL_DT)
    mats["color"] = 0.7
    sphere = dm.placed(pt.GEOM_DT, tm.SPHERE, 0, tuple(g["translation"]), tuple(g["scale"]))
    mesh_geom, mtris, meshes = pt.meshes.add_mesh(np.zeros(0, dtype=pt.GEOM_DT), tris, material_id=0)
    cam = s.camera.copy()
    cam["position"][0] = np.asarray(g["translation"]) + (0.0, 0.5, 3.4)
    cam["lookAt"][0] = g["translation"]
    view = np.asarray(cam["lookAt"][0], dtype=np.float64) - cam["position"][0]
    view /= np.linalg.norm(view)
    right = np.cross(view, (0, 1, 0))
    right /= np.linalg.norm(right)
    cam["view"][0], cam["right"][0], cam["up"][0] = view, right, np.cross(right, view)
    cam = _resized(cam, 64, 64)
    sky = pt.gradient_cubemap(16, (2.0, 2.0, 2.0), (0.5, 0.5, 0.5), (0.05, 0.05, 0.05))
    models = {"faceted": sm.Model(po, mesh_geom, mats, cam, 4, tris=mtris, meshes=meshes),
              "smooth": sm.Model(po, mesh_geom, mats, cam, 4, tris=mtris, meshes=meshes),
              "sphere": sm.Model(po, sphere, mats, cam, 4)}
    models["smooth"].set_vertex_normals(vn)
    for m in models.values():
        m.set_environment(sky)
        for it in range(1, 17):
            m.iterate(it)
    hit = np.ones(64 * 64, dtype=bool)
    for name, m in models.items():
        paths = po.generate_rays(cam, 4)
        x, _ = po.compute_intersections(paths, m.geoms, m.tris, m.meshes)
        h = np.zeros(64 * 64, dtype=bool)
        h[paths["pixelIndex"]] = x["t"] > 0
        hit &= h
    assert hit.sum() > 500
    ref = models["sphere"].image[hit]
    faceted, smooth = rel_l2(models["faceted"].image[hit], ref), rel_l2(models["smooth"].image[hit], ref)
    print("rel. L2 against the analytic sphere over %d pixels: faceted %.5f, smooth %.5f" % (hit.sum(), faceted, smooth))
    MEASURED_FACETED, MEASURED_SMOOTH = 0.06832, 0.02347               # DESIGN.md section 6.26 (745 pixels)
    assert smooth < faceted - 0.5 * (MEASURED_FACETED - MEASURED_SMOOTH)
    assert smooth < faceted


# ---- the loader --------------------------------------------------------------------------------------------------------------------
OBJ = """v 0 0 0
v 1 0 0
v 0 1 0
v 0 0 1
vt 0.5 0.5
vn 0 0 2
vn 1 1 0
vn 0 -3 1
f 1//1 2//2 3//3
f 1/1/3 3/1/2 4/1/1
f 1 2 4//1
"""

SCENE = """MATERIAL 0
RGB         .5 .5 .5
SPECEX      0
SPECRGB     0 0 0
REFL        0
REFR        0
REFRIOR     0
EMITTANCE   0

CAMERA
RES         8 8
FOVY        45
ITERATIONS  1
DEPTH       2
FILE        three
EYE         0.0 5 10.5
LOOKAT      0 5 0
UP          0 1 0

OBJECT 0
mesh %s
material 0
TRANS       1 2 3
ROTAT       10 20 30
SCALE       2 0.5 3
"""


def test_loader_keeps_vn_lines(pt, tmp_path):
    """v//vn, v/vt/vn and a face with a corner that names no normal: each vn is multiplyMV(invTranspose, (vn, 0)) in glm's order,
    normalised in binary32; the third triangle gets the zero triple."""
    (tmp_path / "three.obj").write_text(OBJ)
    (tmp_path / "three.txt").write_text(SCENE % "three.obj")
    s = pt.load_scene(str(tmp_path / "three.txt"))
    assert len(s.triangles) == 3 and s.vertex_normals.shape == (3, 3, 3)
    M = s.geoms["invTranspose"][0]                                       # [col][row]
    raw = np.array([(0, 0, 2), (1, 1, 0), (0, -3, 1)], dtype=F32)
    w = ((M[0][None, :3] * raw[:, 0:1] + M[1][None, :3] * raw[:, 1:2]).astype(F32) +
         (M[2][None, :3] * raw[:, 2:3] + M[3][None, :3] * F32(0)).astype(F32)).astype(F32)
    unit = gm.normalize3(w).astype(F32)
    want = np.stack([unit[[0, 1, 2]], unit[[2, 1, 0]], np.zeros((3, 3), dtype=F32)])
    same(s.vertex_normals, want, "the loader's normals")


def test_cornell_smooth_loads_and_a_scene_without_vn_reports_none(pt, tmp_path):
    s = cases.loaded(pt)
    assert len(s.triangles) == 640 and len(s.meshes) == 2 and s.vertex_normals.shape == (640, 3, 3)
    lens = np.linalg.norm(s.vertex_normals.astype(np.float64), axis=2)
    assert np.abs(lens - 1).max() < 1e-6
    # analytic: (p - centre) / radius of each corner
    for m in s.meshes:
        a, b = int(m["first_triangle"]), int(m["first_triangle"]) + int(m["triangle_count"])
        g = s.geoms[int(m["geom_index"])]
        p = np.stack([s.triangles["v0"][a:b], s.triangles["v1"][a:b], s.triangles["v2"][a:b]], axis=1).astype(np.float64)
        radial = (p - np.asarray(g["translation"], dtype=np.float64)) / (0.5 * float(g["scale"][0]))
        assert np.abs(radial - s.vertex_normals[a:b]).max() < 1e-5
    (tmp_path / "bare.obj").write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\n")
    (tmp_path / "bare.txt").write_text(SCENE % "bare.obj")
    assert pt.load_scene(str(tmp_path / "bare.txt")).vertex_normals is None
    assert pt.load_scene(os.path.join(ROOT, "scenes", "cornell.txt")).vertex_normals is None


def test_uv_sphere_normals(pt):
    tris, vn = pt.meshes.uv_sphere(center=(1.0, 2.0, 3.0), radius=1.5, n_lat=6, n_lon=12, normals=True)
    assert vn.shape == (len(tris), 3, 3) and vn.dtype == F32
    assert tris.tobytes() == pt.meshes.uv_sphere(center=(1.0, 2.0, 3.0), radius=1.5, n_lat=6, n_lon=12).tobytes()
    p = np.stack([tris["v0"], tris["v1"], tris["v2"]], axis=1).astype(np.float64)
    assert np.abs((p - (1.0, 2.0, 3.0)) / 1.5 - vn).max() < 1e-6


# ---- the host code under the sanitizers ------------------------------------------------------------------------------------------
def test_smooth_host_code_under_the_sanitizers(tmp_path):
    """tests/tools/smooth_main.cpp, a program of its own: the steps behind pt_smooth_normal (csrc/pt_smooth.hpp) under
    AddressSanitizer and UBSan.  Nothing sanitized is loaded into this process."""
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ not found")
    exe = str(tmp_path / "smooth_main")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "tools", "smooth_main.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "smooth_main: ok" in r.stdout and not r.stderr, r.stdout + r.stderr
