"""First-hit albedo demodulation in the filters (pt_set_denoise_albedo / pt_albedo) on the CPU: the numpy
model of tests/albedo_model.py against atrous_model where the albedo is 1, the clamp, the albedo plane of
scenes/cornell_textured.txt, the refusals that need no device, and that the switch does what it is for -- on the textured
surfaces of a 64-spp picture the demodulated filter leaves at most 0.75 of the plain filter's error.  No GPU; frames of at most
24 x 24 except for the quality test (128 x 128, its converged reference is tests/golden/albedo_ref.npz)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import __graft_entry__ as ge  # noqa: E402
import albedo_model as alm  # noqa: E402
import atrous_model as am  # noqa: E402
import direct_model as dm  # noqa: E402
import texture_model as tm  # noqa: E402
from gpu_common import _resized, bits, rel_l2  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
W, H = 24, 24
DEFAULT = (1.0, 0.35, 0.5)
_cache = {}


@pytest.fixture(scope="module")
def pt():
    p = ge.load_package()
    p.build()
    p.build_host()
    return p


def textured(pt, w=W, h=H):
    key = ("textured", w, h)
    if key not in _cache:
        s = pt.load_scene(os.path.join(ROOT, "scenes", "cornell_textured.txt"))
        _cache[key] = (s.geoms, s.materials, _resized(s.camera, w, h), s.traceDepth, dict(s.textures))
    return _cache[key]


def first_hits(po, geoms, cam, depth, tris=None, meshes=None):
    return am.gbuffer_from_oracle(po, cam, depth, np.ascontiguousarray(geoms).view(po.GEOM_DT),
                                  None if tris is None else tris.view(po.TRI_DT), None if meshes is None else meshes.view(po.MESH_DT))


def traced_sum(po, geoms, mats, cam, depth, textures, iters):
    m = tm.Model(po, geoms, mats, cam, depth)
    for k, t in textures.items():
        m.set_texture(k, t)
    for it in range(1, iters + 1):
        m.iterate(it)
    return m.image.copy()


# ---- the refusals that need no device -------------------------------------------------------------------------------------------
def test_entry_points_before_init(pt):
    L = pt.library()
    pt.pathtraceFree()
    assert L.pt_set_denoise_albedo(1) == -1
    assert b"pt_set_denoise_albedo" in L.pt_last_error() and b"not initialised" in L.pt_last_error()
    assert L.pt_set_denoise_albedo(0) == -1
    assert L.pt_albedo(None) == -1
    assert b"pt_albedo" in L.pt_last_error() and b"not initialised" in L.pt_last_error()
    assert L.pt_set_denoise_albedo(2) == -1 and b"pt_set_denoise_albedo" in L.pt_last_error()
    with pytest.raises(pt.PtError):
        pt.albedo()
    with pytest.raises(pt.PtError):
        pt.set_denoise_albedo(True)


# ---- albedo 1 everywhere: the plain filter, bit for bit ---------------------------------------------------------------------------
def test_unit_albedo_is_the_plain_filter(pt, po):
    geoms, mats, cam, depth, _ = textured(pt)
    mats = mats.copy()
    plain = (mats["hasReflective"] == 0) & (mats["hasRefractive"] == 0)
    assert plain.sum() == 6 and (~plain).sum() == 1
    col = mats["color"].copy()
    col[plain] = 1.0
    mats["color"] = col
    A = alm.albedo(po, geoms, mats, {}, cam, depth)
    assert (bits(A) == bits(F32(1.0))).all()
    g = first_hits(po, geoms, cam, depth)
    nrm, pos = g["normal"].reshape(H, W, 3), g["position"].reshape(H, W, 3)
    image = traced_sum(po, geoms, mats, cam, depth, {}, 2).reshape(H, W, 3)
    assert (image > 0).any()
    for levels in (0, 1, 5):
        got = alm.denoise(image, 2, A.reshape(H, W, 3), nrm, pos, levels, *DEFAULT)
        want = am.denoise(image, 2, nrm, pos, levels, *DEFAULT)
        assert (bits(got) == bits(want)).all(), levels


def test_levels_0_is_the_mean(pt, po):
    geoms, mats, cam, depth, tex = textured(pt)
    A = alm.albedo(po, geoms, mats, tex, cam, depth).reshape(H, W, 3)
    assert (A != 1).any()
    g = first_hits(po, geoms, cam, depth)
    image = np.random.default_rng(3).uniform(0, 9, (H, W, 3)).astype(F32)
    got = alm.denoise(image, 3, A, g["normal"].reshape(H, W, 3), g["position"].reshape(H, W, 3), 0, *DEFAULT)
    assert (bits(got) == bits((image / F32(3)).astype(F32))).all()
    t = alm.Temporal(W, H, np.ascontiguousarray(mats).view(po.MATERIAL_DT))
    got = t.call(image.reshape(-1, 3), 3, cam, g, A=A, levels=0)
    assert (bits(got) == bits((image / F32(3)).astype(F32).reshape(-1, 3))).all()


def test_temporal_model_without_albedo_is_temporal_model(pt, po):
    import temporal_model as tpm
    geoms, mats, cam, depth, tex = textured(pt)
    m = np.ascontiguousarray(mats).view(po.MATERIAL_DT)
    g = first_hits(po, geoms, cam, depth)
    image = np.random.default_rng(4).uniform(0, 9, (W * H, 3)).astype(F32)
    ours, theirs = alm.Temporal(W, H, m), tpm.Temporal(W, H, m)
    assert (bits(ours.call(image, 2, cam, g, levels=2)) == bits(theirs.call(image, 2, cam, g, levels=2))).all()
    A = alm.albedo(po, geoms, mats, tex, cam, depth)
    on = ours.call(image, 2, cam, g, A=A, levels=2)
    want = alm.denoise(image.reshape(H, W, 3), 2, A.reshape(H, W, 3), g["normal"].reshape(H, W, 3), g["position"].reshape(H, W, 3), 2, *DEFAULT)
    assert (bits(on) == bits(want.reshape(-1, 3))).all()            # no history yet: pt_denoise with the switch on
    assert (bits(ours.cur["C"]) == bits(theirs.cur["C"])).all()     # cur stays in modulated colour


# ---- the clamp ------------------------------------------------------------------------------------------------------------------
CLAMP_IN = [[0.0, -1.0, np.nan], [np.inf, 2.0 ** -7, 2.0 ** -6], [0.5, 64.0, 65.0]]
CLAMP_OUT = [[2.0 ** -6, 2.0 ** -6, 2.0 ** -6], [64.0, 2.0 ** -6, 2.0 ** -6], [0.5, 64.0, 64.0]]


def clamp_scene(pt, w=W, h=H):
    """Three matte bands across the frame, one per row of CLAMP_IN; the corners of the frame miss."""
    geoms, mats, cam, depth, _ = textured(pt, w, h)
    table = np.zeros(3, dtype=mats.dtype)
    table["color"] = np.array(CLAMP_IN, dtype=F32)
    bands = np.concatenate([dm.placed(pt.GEOM_DT, tm.CUBE, k, (0.0, 5.0 + 6.0 * (k - 1), 0.0), (16.0, 5.0, 0.1)) for k in range(3)])
    return bands, table, cam, depth


def test_clamp(pt, po):
    assert (bits(alm.clamp(np.array(CLAMP_IN, dtype=F32))) == bits(np.array(CLAMP_OUT, dtype=F32))).all()
    assert alm.clamp(np.array([-np.inf, -0.0, 1.0, 63.999996], dtype=F32)).tolist() == [2.0 ** -6, 2.0 ** -6, 1.0, float(F32(63.999996))]
    geoms, mats, cam, depth = clamp_scene(pt)
    A = alm.albedo(po, geoms, mats, {}, cam, depth)
    g = first_hits(po, geoms, cam, depth)
    for k in range(3):
        sel = g["materialId"] == k
        assert sel.sum() > 40
        assert (bits(A[sel]) == bits(np.array(CLAMP_OUT[k], dtype=F32))).all(), k
    miss = g["materialId"] < 0
    assert miss.sum() > 20 and (bits(A[miss]) == bits(F32(1.0))).all()
    assert np.isfinite(A).all() and (A >= F32(2.0 ** -6)).all() and (A <= 64).all()


# ---- the albedo plane of cornell_textured ---------------------------------------------------------------------------------------
def test_albedo_of_cornell_textured(pt, po):
    geoms, mats, cam, depth, tex = textured(pt)
    assert sorted(tex) == [0, 5, 6]
    A = alm.albedo(po, geoms, mats, tex, cam, depth)
    g = first_hits(po, geoms, cam, depth)
    mat = g["materialId"]
    one = bits(F32(1.0))
    assert (mat == 4).sum() > 5 and (bits(A[mat == 4]) == one).all()                       # the mirror ball
    wide = _resized(cam, 24, 8)                                                             # a wide frame sees past the box
    gw = first_hits(po, geoms, wide, depth)
    Aw = alm.albedo(po, geoms, mats, tex, wide, depth)
    assert (gw["materialId"] < 0).sum() > 10 and (bits(Aw[gw["materialId"] < 0]) == one).all()   # misses
    for m in (1, 2, 3):                                                                     # untextured walls: material.color
        assert (mat == m).sum() > 10
        assert (bits(A[mat == m]) == bits(mats["color"][m])).all(), m
    checks = {5: [(1.0, 1.0, 1.0), (0.25, 0.3, 0.6)], 6: [(1.0, 1.0, 1.0), (0.2, 0.2, 0.2)]}
    for m, pair in checks.items():                                                          # exactly the two checker values times material.color
        sel = A[mat == m]
        want = [(mats["color"][m] * np.array(c, dtype=F32)).astype(F32) for c in pair]
        is0 = (bits(sel) == bits(want[0])).all(axis=1)
        is1 = (bits(sel) == bits(want[1])).all(axis=1)
        assert (is0 | is1).all() and is0.sum() >= 2 and is1.sum() >= 2, m
    # without the textures: material.color on every hit that is not specular
    plain = alm.albedo(po, geoms, mats, {}, cam, depth)
    for m in (0, 1, 2, 3, 5, 6):
        assert (bits(plain[mat == m]) == bits(mats["color"][m])).all(), m
    assert (bits(plain[mat == 4]) == one).all()
    assert (bits(plain) != bits(A)).any()


def test_mesh_hits_read_material_color(pt, po):
    """A mesh primitive of the matte ball's material, which has a texture: no parametrisation, no tint."""
    import mesh_cases
    geoms, mats, cam, depth, tex = textured(pt)
    tris = mesh_cases.soup(pt.TRI_DT, np.random.default_rng(11), n=50)
    geoms, tris, meshes = pt.meshes.add_mesh(geoms, tris, material_id=6)
    A = alm.albedo(po, geoms, mats, tex, cam, depth, tris, meshes)
    paths = po.generate_rays(cam, depth)
    gg, tt, mm = np.ascontiguousarray(geoms).view(po.GEOM_DT), tris.view(po.TRI_DT), meshes.view(po.MESH_DT)
    isects, _ = po.compute_intersections(paths, gg, tt, mm)
    hg = tm.hit_geoms(po, gg, tt, mm, paths, isects)
    on_mesh = hg == len(geoms) - 1
    assert on_mesh.sum() >= 3
    assert (bits(A[on_mesh]) == bits(mats["color"][6])).all()
    ball = (hg == 7)
    assert ball.sum() > 5 and (bits(A[ball]) != bits(mats["color"][6])).any()              # the sphere of the same material is tinted


# ---- what the switch is for -----------------------------------------------------------------------------------------------------
def test_quality_on_textured_surfaces(pt, po, golden):
    """cornell_textured at 128 x 128, levels 5, sigmas 1.0 / 0.35 / 0.5, 64 iterations against the model's own 1024 (the golden
    file; tests/golden/make_albedo_ref.py).  Relative L2 errors, measured: textured first hits (1688 pixels) raw 0.5068, plain
    filter 0.3308, demodulated 0.1685 (ratio 0.51, bound 0.75 -- halfway between that and "no better"); whole frame 0.1184 /
    0.0576 / 0.0430.  Both models are deterministic: these are fixed numbers."""
    w = h = 128
    z = golden["albedo_ref"]
    assert int(z["iterations"]) == 1024 and int(z["width"]) == w and int(z["height"]) == h
    ref = z["mean"].astype(F32)
    geoms, mats, cam, depth, tex = textured(pt, w, h)
    image = traced_sum(po, geoms, mats, cam, depth, tex, 64).reshape(h, w, 3)
    g = first_hits(po, geoms, cam, depth)
    nrm, pos = g["normal"].reshape(h, w, 3), g["position"].reshape(h, w, 3)
    A = alm.albedo(po, geoms, mats, tex, cam, depth).reshape(h, w, 3)
    plain = am.denoise(image, 64, nrm, pos, 5, *DEFAULT).reshape(-1, 3)
    dem = alm.denoise(image, 64, A, nrm, pos, 5, *DEFAULT).reshape(-1, 3)
    raw = (image / F32(64)).reshape(-1, 3)
    textured_mats = sorted(m for m in tex if not mats["emittance"][m] > 0)
    assert textured_mats == [5, 6]
    mask = np.isin(g["materialId"], textured_mats)
    e = {k: (rel_l2(v[mask], ref[mask]), rel_l2(v, ref)) for k, v in (("raw", raw), ("plain", plain), ("demodulated", dem))}
    for k, v in e.items():
        print("%-12s textured first hits (%d px) %.4f   whole frame %.4f" % (k, int(mask.sum()), v[0], v[1]))
    assert int(mask.sum()) == 1688
    assert e["demodulated"][0] <= 0.75 * e["plain"][0]
    assert e["demodulated"][1] < e["plain"][1]
