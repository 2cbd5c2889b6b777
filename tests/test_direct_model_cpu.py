"""Direct lighting (PT_DIRECT_LIGHT) on the CPU: the numpy model of tests/direct_model.py against the
oracle where the flag changes nothing, its pieces against the oracle's functions and pt_light_elements, the sample's weight
against closed forms, and the estimator against the plain one it must agree with in expectation.  No GPU; frames of at most
24 x 24."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import __graft_entry__ as ge  # noqa: E402
import direct_model as dm  # noqa: E402
import glossy_model as gm  # noqa: E402
from gpu_common import _resized, bits, rel_l2  # noqa: E402

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


def trs(pt, kind, material, trans, scale, rot=(0.0, 0.0, 0.0)):
    """One primitive under T * Rx Ry Rz * S, matrices in float64 rounded once (input to the specification, not part of it)."""
    g = np.zeros(1, dtype=pt.GEOM_DT)
    rx, ry, rz = (np.radians(a) for a in rot)
    Rx = np.array([[1, 0, 0], [0, np.cos(rx), -np.sin(rx)], [0, np.sin(rx), np.cos(rx)]])
    Ry = np.array([[np.cos(ry), 0, np.sin(ry)], [0, 1, 0], [-np.sin(ry), 0, np.cos(ry)]])
    Rz = np.array([[np.cos(rz), -np.sin(rz), 0], [np.sin(rz), np.cos(rz), 0], [0, 0, 1]])
    M = np.eye(4)
    M[:3, :3] = Rx @ Ry @ Rz @ np.diag(scale)
    M[:3, 3] = trans
    with np.errstate(all="ignore"):
        inv = np.linalg.inv(M) if abs(np.linalg.det(M)) > 0 else np.full((4, 4), np.nan)
    g["type"], g["materialid"] = kind, material
    g["translation"], g["rotation"], g["scale"] = trans, rot, scale
    g["transform"][0] = M.T.astype(F32)                                  # stored m[col][row]
    g["inverseTransform"][0] = inv.T.astype(F32)
    g["invTranspose"][0] = inv.astype(F32)                               # (inv^T)^T
    return g


def two_materials(pt, emittance=3.0):
    m = np.zeros(2, dtype=pt.MATERIAL_DT)
    m["color"] = 1.0
    m["emittance"][0] = emittance
    return m


# ---- where the flag changes nothing -----------------------------------------------------------------------------------------------
def test_without_cube_or_sphere_lights_the_model_is_the_oracle(pt, po):
    """A scene whose lamp does not emit, and one whose only light is a mesh: the flagged model is the oracle's iteration."""
    import mesh_cases
    geoms, mats, cam, depth = load(pt, "cornell", 20, 16)
    dark = mats.copy()
    dark["emittance"] = 0
    lit = dark.copy()
    lit["emittance"][4] = 4.0                                            # the mesh's material emits
    lit["hasReflective"][4] = 0
    tris = mesh_cases.soup(pt.TRI_DT, np.random.default_rng(5), n=30)
    g2, tris, meshes = pt.meshes.add_mesh(geoms[:6], tris, material_id=4)
    for gs, ms, tr, me in ((geoms, dark, None, None), (g2, lit, tris, meshes)):
        m = dm.Model(po, gs, ms, cam, depth, tris=tr, meshes=me)
        assert not m.direct and len(m.table) == 0
        oracle = po.Tracer(np.ascontiguousarray(gs).view(po.GEOM_DT), np.ascontiguousarray(ms).view(po.MATERIAL_DT), cam, depth,
                           flags=po.F_COMPACT, trig=po.TRIG_SHARED, tris=None if tr is None else np.ascontiguousarray(tr).view(po.TRI_DT),
                           meshes=None if me is None else np.ascontiguousarray(me).view(po.MESH_DT))
        for it in (1, 2, 3):
            m.iterate(it)
            oracle.iterate(it)
            assert m.image.tobytes() == oracle.image.tobytes(), it
    assert (m.image != 0).any()                                          # the mesh lights its scene


# ---- the pieces ---------------------------------------------------------------------------------------------------------------------
def test_draws_and_multiply_mv_are_the_oracles(pt, po):
    rng = np.random.default_rng(2)
    seeds = rng.integers(0, 2 ** 32, 64, dtype=np.uint64).astype(np.uint32)
    geoms, mats, _, _ = load(pt, "cornell_two_lamps", 8, 8)
    geoms = np.ascontiguousarray(geoms).view(po.GEOM_DT)
    table = dm.light_elements(geoms, mats)
    P = rng.uniform(-4, 4, (64, 3)).astype(F32) + F32([0, 5, 0])
    _, _, e, info = dm.sample(po, geoms, table, P, gm.random_unit(rng, 64), gm.probe_states(po, seeds))
    for k, s in enumerate(seeds):
        u = po.u01_sequence(int(s), 3)
        assert [bits(info["u"][j][k:k + 1])[0] for j in range(3)] == list(bits(u))
        want = next((j for j in range(len(table)) if u[0] < table["cdf"][j]), len(table) - 1)
        assert e[k] == want
    L = po.lib()
    M = rng.normal(size=(200, 4, 4)).astype(F32)
    v = rng.normal(size=(200, 3)).astype(F32)
    for w in (0.0, 1.0):
        got = dm.multiply_mv(M, v, w)
        for k in range(len(M)):
            r = L.pto_multiply_mv(po._p(np.ascontiguousarray(M[k])), po.Vec4(float(v[k, 0]), float(v[k, 1]), float(v[k, 2]), w))
            assert list(bits(got[k])) == list(bits(np.array([r.x, r.y, r.z], dtype=F32))), (k, w)


def degenerate_scene(pt):
    mats = two_materials(pt)
    geoms = np.concatenate([
        trs(pt, dm.CUBE, 0, (0, 9, 0), (1.5, 0.3, 1.5), (20, 35, 0)),      # six faces
        trs(pt, dm.CUBE, 1, (0, 0, 0), (10, 0.01, 10)),                    # does not emit
        trs(pt, dm.SPHERE, 0, (2.5, 3, 1), (1.2, 0.8, 1.6), (30, 0, 40)),
        trs(pt, dm.CUBE, 0, (1, 1, 1), (2, 0, 3)),                         # flat: four faces of area 0 are left out, two stay
        trs(pt, dm.SPHERE, 0, (1, 1, 1), (0, 1, 1)),                       # |det| = 0: left out
        trs(pt, dm.CUBE, 0, (1, 1, 1), (1e30, 1e30, 1)),                   # two faces of area 1e60: not a binary32 number, left out
        trs(pt, 2, 0, (0, 0, 0), (1, 1, 1)),                               # a mesh is never an element
    ])
    return geoms, mats


def test_light_elements_equal_the_model(pt, po):
    for geoms, mats in (load(pt, "cornell_two_lamps", 8, 8)[:2], load(pt, "cornell", 8, 8)[:2], degenerate_scene(pt)):
        want = dm.light_elements(np.ascontiguousarray(geoms).view(po.GEOM_DT), np.ascontiguousarray(mats).view(po.MATERIAL_DT))
        got = pt.light_elements(geoms, mats)
        assert got.dtype.itemsize == dm.LIGHT_DT.itemsize == 68
        assert got.tobytes() == want.tobytes(), (len(got), len(want))
        assert len(got) and got["cdf"][-1] == 1 and (np.diff(got["cdf"]) >= 0).all() and (got["area"] > 0).all()
    geoms, mats = degenerate_scene(pt)
    t = pt.light_elements(geoms, mats)
    assert list(np.bincount(t["geom"], minlength=7)) == [6, 0, 1, 2, 0, 4, 0] and np.isfinite(t.view(np.float32).reshape(len(t), 17)[:, 2:]).all()
    two = load(pt, "cornell_two_lamps", 8, 8)
    t = pt.light_elements(two[0], two[1])
    assert list(t["geom"]) == [0] * 6 + [7] and list(t["kind"]) == [dm.CUBE] * 6 + [dm.SPHERE]
    # the cube lamp: |ea x eb| = the product of the two scales up to rounding; outward normals in opposite pairs
    assert np.allclose(t["area"][:6], [0.45, 0.45, 2.25, 2.25, 0.45, 0.45], rtol=1e-6)
    assert np.allclose(t["normal"][0], -t["normal"][1], atol=1e-7) and np.allclose(np.linalg.norm(t["normal"][:6], axis=1), 1, atol=1e-6)
    centre = np.array([0, 9, 0])
    mid = t["c0"][:6] + 0.5 * t["ea"][:6] + 0.5 * t["eb"][:6]
    assert ((mid - centre) * t["normal"][:6]).sum(axis=1).min() > 0
    # no lights at all: an empty table
    dark = two[1].copy()
    dark["emittance"] = 0
    assert len(pt.light_elements(two[0], dark)) == 0


def test_light_elements_refusals(pt):
    geoms, mats, _, _ = load(pt, "cornell_two_lamps", 8, 8)
    L = pt.library()
    g = np.ascontiguousarray(geoms)
    m = np.ascontiguousarray(mats)
    out = np.full(7, -1, dtype=np.int8).repeat(68).view(pt.LIGHT_DT)
    assert L.pt_light_elements(g.ctypes.data, len(g), m.ctypes.data, len(m), out.ctypes.data, 6) == 7      # too small: the count ...
    assert (out.view(np.int8) == -1).all()                                                                # ... and nothing written
    assert L.pt_light_elements(g.ctypes.data, len(g), m.ctypes.data, len(m), None, 0) == 7
    assert L.pt_light_elements(g.ctypes.data, len(g), m.ctypes.data, len(m), out.ctypes.data, 7) == 7 and (out["area"] > 0).all()
    assert L.pt_light_elements(g.ctypes.data, -1, m.ctypes.data, len(m), None, 0) == -1
    assert L.pt_light_elements(None, 2, m.ctypes.data, len(m), None, 0) == -1
    assert L.pt_light_elements(g.ctypes.data, len(g), None, 2, None, 0) == -1
    assert L.pt_light_elements(g.ctypes.data, len(g), m.ctypes.data, len(m), None, 3) == -1
    assert L.pt_light_elements(g.ctypes.data, len(g), m.ctypes.data, len(m), out.ctypes.data, -1) == -1
    bad = g.copy()
    bad["materialid"][7] = len(m)
    assert L.pt_light_elements(bad.ctypes.data, len(bad), m.ctypes.data, len(m), None, 0) == -1
    assert b"material" in L.pt_last_error()
    with pytest.raises(ValueError):
        dm.light_elements(bad, m)
    assert L.pt_light_elements(None, 0, m.ctypes.data, len(m), None, 0) == 0                               # an empty scene


# ---- the weight against closed forms ----------------------------------------------------------------------------------------------
N_DRAWS = 20000


def draws(po, geoms, mats, P, n, seed):
    geoms = np.ascontiguousarray(geoms).view(po.GEOM_DT)
    table = dm.light_elements(geoms, np.ascontiguousarray(mats).view(po.MATERIAL_DT))
    seeds = np.random.default_rng(seed).integers(0, 2 ** 32, N_DRAWS, dtype=np.uint64).astype(np.uint32)
    Ps = np.tile(np.asarray(P, dtype=F32), (N_DRAWS, 1))
    ns = np.tile(np.asarray(n, dtype=F32), (N_DRAWS, 1))
    return dm.sample(po, geoms, table, Ps, ns, gm.probe_states(po, seeds)) + (table,)


def within_five_standard_errors(samples, want):
    s = np.asarray(samples, dtype=np.float64)
    se = s.std(ddof=1) / np.sqrt(len(s))
    assert se > 0 and abs(s.mean() - want) <= 5 * se, (s.mean(), want, se)


def test_weight_of_a_uniform_sphere(pt, po):
    """A sphere of radius R seen from distance d along n: the form factor is R^2 / d^2."""
    R, d = 0.75, 3.0
    geoms = trs(pt, dm.SPHERE, 0, (0, 0, d), (2 * R, 2 * R, 2 * R))
    _, w, _, info, _ = draws(po, geoms, two_materials(pt), (0, 0, 0), (0, 0, 1), 1)
    assert 0.2 < info["ok"].mean() < 0.8                                 # the far side is back-facing: step 6
    within_five_standard_errors(w, R * R / (d * d))


def test_weight_of_a_parallelogram_lamp(pt, po):
    """The turned cube lamp of cornell_two_lamps from a point on the floor, against quadrature of cos cos / (pi r^2)."""
    geoms = trs(pt, dm.CUBE, 0, (0, 9, 0), (1.5, 0.3, 1.5), (20, 35, 0))
    P, n = np.array([1.0, 0.0, 0.5]), np.array([0.0, 1.0, 0.0])
    _, w, e, info, table = draws(po, geoms, two_materials(pt), P, n, 2)
    assert len(np.unique(e)) == 6 and 0 < info["ok"].mean() < 1
    G = 400
    u = (np.arange(G) + 0.5) / G
    uu, vv = np.meshgrid(u, u, indexing="ij")
    total = 0.0
    for el in table:
        y = el["c0"].astype(np.float64) + uu[..., None] * el["ea"].astype(np.float64) + vv[..., None] * el["eb"].astype(np.float64)
        v = y - P
        r2 = (v * v).sum(-1)
        dr = v / np.sqrt(r2)[..., None]
        cs = np.maximum((dr * n).sum(-1), 0)
        cl = np.maximum(-(dr * el["normal"].astype(np.float64)).sum(-1), 0)
        total += (cs * cl / (np.pi * r2)).mean() * float(el["area"])
    within_five_standard_errors(w, total)


def test_area_measure_of_an_ellipsoid(pt, po):
    """The mean of A over the uniform object-space draws is the ellipsoid's area (quadrature of |dS| over the parameter square)."""
    a, b, c = 0.6, 0.4, 0.8                                              # SCALE 1.2 .8 1.6
    geoms = trs(pt, dm.SPHERE, 0, (2.5, 3, 1), (2 * a, 2 * b, 2 * c), (30, 0, 40))
    _, _, _, info, table = draws(po, geoms, two_materials(pt), (0, 0, 0), (0, 1, 0), 3)
    G = 1200
    th = (np.arange(G) + 0.5) / G * np.pi
    ph = (np.arange(G) + 0.5) / G * 2 * np.pi
    T, Ph = np.meshgrid(th, ph, indexing="ij")
    # |x_theta x x_phi| of x = (a sin t cos p, b sin t sin p, c cos t)
    dS = np.sin(T) * np.sqrt((b * c * np.sin(T) * np.cos(Ph)) ** 2 + (a * c * np.sin(T) * np.sin(Ph)) ** 2 + (a * b * np.cos(T)) ** 2)
    area = dS.mean() * np.pi * 2 * np.pi
    within_five_standard_errors(info["A"], area)
    assert abs(float(table["area"][0]) - np.pi * (8 * a * b * c) ** (2.0 / 3.0)) < 1e-5      # the nominal area: a selection mass


def test_a_point_inside_an_emitting_sphere_faces_it(pt, po):
    geoms = trs(pt, dm.SPHERE, 0, (0, 0, 0), (6, 4, 8), (10, 20, 30))
    _, w, _, info, _ = draws(po, geoms, two_materials(pt), (0.5, -0.3, 1.0), (0, 0, 1), 4)
    assert info["inside"].all() and (info["cl"] > 0).all()
    assert 0.3 < info["ok"].mean() < 0.7 and (w[info["ok"]] > 0).all()   # the half behind n ends at step 6


# ---- the estimator --------------------------------------------------------------------------------------------------------------------
def frame_means(model_or_tracer, count, keep):
    """The mean over pixels and channels of the own frame of each of the iterations 1 .. count of a fresh model (the running
    sum's increments), and a copy of the running sum after iteration `keep`."""
    out, kept = [], None
    assert not model_or_tracer.image.any()
    prev = model_or_tracer.image.astype(np.float64)
    for it in range(1, count + 1):
        model_or_tracer.iterate(it)
        cur = model_or_tracer.image.astype(np.float64)
        out.append((cur - prev).mean())
        prev = cur
        if it == keep:
            kept = model_or_tracer.image.copy()
    return np.array(out), kept


def two_lamps_runs(pt, po):
    """Shared by the two tests below: 16 x 16, the flagged model at depth 2 and the plain oracle at depth 3, 48 iterations each."""
    if "runs" not in _cache:
        geoms, mats, cam, _ = load(pt, "cornell_two_lamps", 16, 16)
        assert not ((mats["hasReflective"] > 0) | (mats["hasRefractive"] > 0)).any()
        g, m = np.ascontiguousarray(geoms).view(po.GEOM_DT), np.ascontiguousarray(mats).view(po.MATERIAL_DT)
        flagged = dm.Model(po, g, m, cam, 2)
        plain = po.Tracer(g, m, cam, 3, flags=po.F_COMPACT, trig=po.TRIG_SHARED)
        a, img_a16 = frame_means(flagged, 48, 16)
        b, img_b16 = frame_means(plain, 48, 16)
        # one iteration's frame each: the increments add up to the running sum
        assert len(a) == len(b) == 48 and abs(a.sum() - flagged.image.mean(dtype=np.float64)) < 1e-9 and abs(b.sum() - plain.image.mean(dtype=np.float64)) < 1e-9
        _cache["runs"] = (a, b, img_a16, img_b16, (g, m, cam), dict(flagged.counts))
    return _cache["runs"]


def test_the_flagged_estimator_agrees_with_one_more_plain_bounce(pt, po):
    """E[flag, depth 2] = E[no flag, depth 3] in a scene without specular surfaces: the frame means over N = 48 iterations agree
    within 5 standard errors of their difference (from the per-iteration frame means: the iterations are independent)."""
    a, b, _, _, _, counts = two_lamps_runs(pt, po)
    se = np.sqrt(a.var(ddof=1) / len(a) + b.var(ddof=1) / len(b))
    print("frame mean: flagged depth 2 %.6f, plain depth 3 %.6f, standard error of the difference %.6f" % (a.mean(), b.mean(), se))
    assert se > 0 and abs(a.mean() - b.mean()) <= 5 * se
    assert counts["sphere"] > 0 and counts["cube"] > 0


def test_sixteen_flagged_iterations_are_closer_to_the_converged_image(pt, po):
    a, b, img_a16, img_b16, (g, m, cam), _ = two_lamps_runs(pt, po)
    ref = po.Tracer(g, m, cam, 3, flags=po.F_COMPACT, trig=po.TRIG_SHARED)
    count = 8192
    ref.iterate_parallel(1001, count, 8)
    conv = ref.image.astype(np.float64) / count
    ea, eb = rel_l2(img_a16.astype(np.float64) / 16, conv), rel_l2(img_b16.astype(np.float64) / 16, conv)
    print("relative L2 to the converged plain depth-3 image after 16 iterations: flagged depth 2 %.4f, plain depth 3 %.4f (ratio %.3f)"
          % (ea, eb, ea / eb))
    assert ea < eb


def test_every_branch_is_seen_on_cornell(pt, po):
    """Step-6 exits and occluded final rays on cornell.txt (the mirror ball ends its last-bounce hits with colour 0)."""
    geoms, mats, cam, depth = load(pt, "cornell", 16, 16)
    m = dm.Model(po, geoms, mats, cam, depth)
    for it in (1, 2):
        m.iterate(it)
    c = m.counts
    print("cornell 16 x 16, 2 iterations: %r; live %r" % (c, m.live))
    assert 0 < c["step 6"] < c["sampled"] and 0 < c["occluded"] < c["final rays"]
    assert c["final rays"] == c["sampled"] - c["step 6"] and len(m.live) == depth + 1 and m.live[depth] > 0


# ---- the host code under the sanitizers ---------------------------------------------------------------------------------------------
def test_light_elements_driver_runs_clean_under_the_sanitizers(tmp_path):
    """csrc/pt_lights.hpp compiled into its stand-alone driver with ASan and UBSan and run as a program of its own (nothing
    sanitized is loaded into this process): scaled, flat, singular, huge and non-finite primitives, a table past the limit."""
    exe = str(tmp_path / "light_elements_main")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "tools", "light_elements_main.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "light_elements_main: ok" in r.stdout and not r.stderr, r.stdout + r.stderr
