"""GPU parity, direct lighting that samples the environment map (PT_DIRECT_SKY with PT_DIRECT_LIGHT; include/ptmi355.h, DESIGN.md
section 6.24): while a map is set it is one more light element behind the lamps', and a final ray aimed at it scores the map
where it leaves the scene.  Everything is compared bit for bit with the numpy model (tests/sky_model.py, on top of
tests/direct_model.py), under both launch plans where a plan exists: the two probes -- engine seeds and pixel indices crafted so
that a draw lands at and next to a table entry --, every pipeline that honours the flags, batches on the lanes, a session that
traces ahead while its map comes, goes and comes back, the stepping interface with its statistics, tiles, the refusal, the
headless host and a furnace whose expectation is exactly 1."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import __graft_entry__ as ge  # noqa: E402,F401
import direct_model as dm  # noqa: E402
import glossy_model as gm  # noqa: E402
import sky_model as sm  # noqa: E402
from gpu_common import pt, launch_plan, bits, assert_paths_equal, _resized  # noqa: E402,F401

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 50, 37                                              # 1850 paths: 28 full waves and one of 58
F32 = np.float32
M31 = 2 ** 31 - 1
INV = pow(48271, -1, M31)
_cache = {}


def same(got, want, what=""):
    bad = (bits(got) != bits(want)).any(axis=-1)
    assert not bad.any(), "%s: %d of %d differ, first %d" % (what, bad.sum(), bad.size, np.nonzero(bad.reshape(-1))[0][0])


def sky(pt, n=16):
    if ("sky", n) not in _cache:
        t = sm.sun_sky(pt, n) if n > 1 else sm.gradient(pt, 1)
        _cache[("sky", n)] = (t, sm.tables(t))
    return _cache[("sky", n)]


# ---- crafted engines -------------------------------------------------------------------------------------------------------------
def seed_for_draw(k, which):
    """The engine seed whose draw number `which` (0-based) is k / 2^31: the state after which + 1 steps is k + 1."""
    return ((k + 1) * pow(INV, which + 1, M31)) % M31


def near(c):
    """k / 2^31 at the float32 c, one integer below and above it, and one and two float32 steps below and above."""
    k = int(round(float(c) * 2 ** 31))
    step = max(1, int(np.spacing(F32(k))))
    return [k + dk for dk in (0, -1, 1, -step, step, -2 * step, 2 * step) if 0 <= k + dk < M31 - 1]


def utilhash(a):
    a = ((a + 0x7ed55d16) + (a << 12)) & 0xffffffff
    a = ((a ^ 0xc761c23c) ^ (a >> 19)) & 0xffffffff
    a = ((a + 0x165667b1) + (a << 5)) & 0xffffffff
    a = ((a + 0xd3a2646c) ^ (a << 9)) & 0xffffffff
    a = ((a + 0xfd7046c5) + (a << 3)) & 0xffffffff
    a = ((a ^ 0xb55a4f09) ^ (a >> 16)) & 0xffffffff
    return a


def utilhash_inverse(y):
    """utilhash is a bijection of the 32-bit words: every step is an odd multiple plus a constant, an xorshift, or an addition
    xored with a left shift (solved from the low bits up)."""
    M = 0xffffffff
    b = y ^ 0xb55a4f09
    a = b ^ (b >> 16)
    a = ((a - 0xfd7046c5) * pow(9, -1, 2 ** 32)) & M
    y, a, m = a, 0, 0
    while m < 32:                                                       # y = (a + C) ^ (a << 9): a's low m bits give the next 9
        m += 9
        mask = (1 << m) - 1
        a = (((y ^ (a << 9)) & mask) - 0xd3a2646c) & mask
    a &= M
    a = ((a - 0x165667b1) * pow(33, -1, 2 ** 32)) & M
    b = a ^ 0xc761c23c
    a = b ^ (b >> 19)
    return ((a - 0x7ed55d16) * pow(4097, -1, 2 ** 32)) & M


def pixel_for_state(state, it, depth):
    """The pixelIndex (int32) whose engine makeSeededRandomEngine(it, pixel, depth) starts in `state` (1 <= state < 2^31 - 1)."""
    key = (1 << 31) | (depth << 22) | it
    p = utilhash_inverse(state ^ utilhash(key))
    return p - 2 ** 32 if p >= 2 ** 31 else p


def test_crafted_engines(po):
    L = po.lib()
    for a in (0, 1, 12345, 0xdeadbeef, 0xffffffff):
        assert L.pto_utilhash(a) == utilhash(a) and utilhash_inverse(utilhash(a)) == a
    for which in (0, 1, 2):
        s = seed_for_draw(2 ** 30, which)
        assert po.u01_sequence(s, which + 1)[which] == 0.5
        p = pixel_for_state(s, 7, 2)
        assert L.pto_make_seeded_engine(7, p, 2) == s


# ---- pt_probe_sky_sample -------------------------------------------------------------------------------------------------------
def sample_seeds(po, tab, count, rng):
    """Seeds whose second draw sits at and next to row cdf entries, seeds whose third draw sits at and next to an entry of the
    column cdf of the very row their second draw picks (found by trying every entry: one in 6 n fits), and random ones."""
    n = tab["n"]
    rows = tab["rowcdf"][:-1]
    pick = rows if len(rows) <= 12 else rows[rng.choice(len(rows), 12, replace=False)]
    crafted = [seed_for_draw(k, 1) for c in pick for k in near(c)]
    cols = []
    if 1 < n <= 5:
        for r in range(6 * n):
            for c in tab["colcdf"][r, :-1]:
                for k in near(c):
                    s = seed_for_draw(k, 2)
                    if min(int(np.searchsorted(tab["rowcdf"], po.u01_sequence(s, 2)[1], side="right")), 6 * n - 1) == r:
                        cols.append(s)
        assert len(cols) > 0
    out = np.array(cols[:40] + crafted, dtype=np.uint32)
    extra = rng.integers(0, 2 ** 32, count, dtype=np.uint64).astype(np.uint32)
    return np.concatenate([out, extra])[:count], len(cols)


@pytest.mark.parametrize("map_n", [1, 2, 5, 64])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_sky_sample_probe_equals_the_model(pt, po, n, map_n):
    """Maps of 1, 2, 5 and 64 texels a side: u1 and u2 at and next to cdf entries, normals on any side (back-facing draws end
    the path), NaN normals (cs > 0 is false)."""
    texels, tab = sky(pt, map_n)
    rng = np.random.default_rng(100 * map_n + n)
    seeds, ncols = sample_seeds(po, tab, n, rng)
    normals = gm.random_unit(rng, n)
    normals[::4] = (0, 1, 0)
    normals[6::16] = np.nan
    d, w, k, info = sm.probe_sky_sample(po, texels, normals, gm.probe_states(po, seeds), sky=tab)
    gd, gw, gk = pt.probe_sky_sample(texels, normals, seeds)
    assert (gk == k).all(), np.nonzero(gk != k)[0][:5]
    same(gw[:, None], w[:, None], "weight")
    same(gd, d, "direction")
    assert (gw[~info["ok"]] == 0).all() and (gd[~info["ok"]] == 0).all() and (gw >= 0).all()
    if n == 257:
        assert 0 < info["ok"].mean() < 1 and not info["ok"][6::16].any() and (map_n == 1 or len(np.unique(k)) > 4)
    if n == 257 and map_n == 2:
        # at a cdf entry the draw belongs to the NEXT row (u1 < rowcdf[r] is strict)
        s = np.array([seed_for_draw(int(round(float(tab["rowcdf"][3]) * 2 ** 31)), 1)], dtype=np.uint32)
        assert po.u01_sequence(int(s[0]), 2)[1] == tab["rowcdf"][3]
        assert pt.probe_sky_sample(texels, normals[:1], s)[2][0] // 2 == 4 and ncols > 0


def test_sky_sample_probe_on_a_large_map(pt, po):
    """1024 texels a side, one texel 10^6 times the rest: 6144 rows, 6.3 M column entries behind the record."""
    if "big" not in _cache:
        t = np.ones((6, 1024, 1024, 3), dtype=F32)
        t[2, 300, 700] = F32(1e6)
        _cache["big"] = (t, sm.tables(t))
    texels, tab = _cache["big"]
    rng = np.random.default_rng(9)
    n = 257
    seeds, _ = sample_seeds(po, tab, n, rng)
    normals = np.tile(np.array([0, 1, 0], dtype=F32), (n, 1))
    d, w, k, info = sm.probe_sky_sample(po, texels, normals, gm.probe_states(po, seeds), sky=tab)
    gd, gw, gk = pt.probe_sky_sample(texels, normals, seeds)
    assert (gk == k).all() and (k == (2 * 1024 + 300) * 1024 + 700).sum() > 10 and len(np.unique(k)) > 50
    same(gw[:, None], w[:, None], "weight")
    same(gd, d, "direction")


def test_sky_sample_probe_refusals_and_maps_without_an_element(pt):
    L = pt.library()
    t = np.ones((6, 2, 2, 3), dtype=F32)
    z3, z1, zi, sd = np.zeros((2, 3), F32), np.zeros(2, F32), np.zeros(2, np.int32), np.zeros(2, np.uint32)
    ok = [t.ctypes.data, 2, z3.ctypes.data, sd.ctypes.data, 2, z3.ctypes.data, z1.ctypes.data, zi.ctypes.data]
    assert L.pt_probe_sky_sample(*ok) == 0
    for k, v in ((0, None), (1, -1), (1, 1025), (2, None), (3, None), (4, -1), (4, (1 << 26) + 1), (5, None), (6, None), (7, None)):
        bad = list(ok)
        bad[k] = v
        assert L.pt_probe_sky_sample(*bad) == -1, k
    assert L.pt_probe_sky_sample(t.ctypes.data, 2, None, None, 0, None, None, None) == 0      # count == 0 launches nothing
    for dark in (np.zeros((6, 2, 2, 3), F32), np.full((6, 2, 2, 3), np.nan, F32), None):
        d, w, k = pt.probe_sky_sample(dark, np.ones((2, 3), F32), sd)
        assert (d == 0).all() and (w == 0).all() and (k == -1).all()


# ---- pt_probe_shade_scatter_direct_sky ---------------------------------------------------------------------------------------------
def two_lamps(pt):
    if "two" not in _cache:
        s = pt.load_scene(os.path.join(ROOT, "scenes", "cornell_two_lamps.txt"))
        _cache["two"] = (s.geoms, s.materials, _resized(s.camera, W, H), s.traceDepth)
    return _cache["two"]


def shade_records(pt, po, n, depth, trace_depth, it, table):
    """cornell_two_lamps with a mirror and a glass material appended; hits on every material, misses, dead paths, back-facing and
    NaN normals.  The first records' pixel indices are crafted: the engine of bounce trace_depth - 1 draws u0 at and next to 0.5,
    the boundary between the lamps and the sky.  At depth == trace_depth the winner is the target, another primitive or nothing
    -- whatever the ray was aimed at."""
    geoms, mats, _, _ = two_lamps(pt)
    extra = np.zeros(2, dtype=pt.MATERIAL_DT)
    extra["color"], extra["spec_color"] = (0.3, 0.4, 0.5), (0.9, 0.8, 0.7)
    extra["hasReflective"][0], extra["hasRefractive"][1], extra["indexOfRefraction"][1] = 1, 1, 1.5
    mats = np.concatenate([mats, extra])
    rng = np.random.default_rng(1000 * depth + n)
    p = np.zeros(n, dtype=pt.PATH_DT)
    x = np.zeros(n, dtype=pt.ISECT_DT)
    p["origin"] = (rng.uniform(-4.5, 4.5, (n, 3)) + (0, 5, 0)).astype(F32)
    p["direction"] = gm.random_unit(rng, n)
    p["color"] = rng.uniform(0.05, 1.0, (n, 3)).astype(F32)
    p["pixelIndex"] = rng.integers(-2 ** 31, 2 ** 31, n, dtype=np.int64).astype(np.int32)
    boundary = [pixel_for_state(seed_for_draw(k, 0), it, trace_depth - 1) for k in near(F32(0.5))]
    p["pixelIndex"][:len(boundary)] = boundary[:n]
    p["remainingBounces"] = rng.choice(np.array([0, 1, 2, 8], dtype=np.int32), n, p=[0.08, 0.3, 0.3, 0.32])
    p["remainingBounces"][:len(boundary)] = 2
    x["normal"] = gm.random_unit(rng, n)                             # any side: back-facing draws end the path
    x["normal"][::3] = (0, 1, 0)
    if depth == trace_depth - 1:                                     # (at a plain bounce a NaN normal scatters to a NaN whose bits nobody pins)
        x["normal"][10::17] = np.nan
    x["t"] = np.where(rng.random(n) < 0.1, -1.0, rng.uniform(0.5, 6.0, n)).astype(F32)
    x["materialId"] = rng.integers(0, len(mats), n).astype(np.int32)
    x["materialId"][:len(boundary)] = 1                              # matte: the crafted records sample
    x["t"][:len(boundary)] = np.abs(x["t"][:len(boundary)])
    outside = (rng.random(n) < 0.5).astype(np.uint8)
    hit = None
    if depth == trace_depth:
        target = dm.target_geoms(po, table, it, p["pixelIndex"], depth - 1)
        other = np.where(target == 0, 7, 0)
        hit = np.choose(rng.integers(0, 4, n), [np.where(target >= 0, target, 3), other, np.full(n, 3), np.full(n, -1)]).astype(np.int32)
        x["t"] = np.where(hit < 0, -1.0, np.abs(x["t"])).astype(F32)
        x["materialId"] = geoms["materialid"][np.maximum(hit, 0)]
    return geoms, mats, p, x, outside, hit


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_shade_probe_equals_the_model(pt, po, n):
    """Lamps and sky together under maps of 2, 5 and 64 texels a side, at a plain bounce, the sampling bounce and the final ray."""
    D = 3
    geoms, mats, _, _ = two_lamps(pt)
    lamps = dm.light_elements(np.ascontiguousarray(geoms).view(po.GEOM_DT), np.ascontiguousarray(mats).view(po.MATERIAL_DT))
    for map_n, it, depth in ((2, 1, D - 2), (5, 3, D - 1), (64, 100000, D - 1), (2, 5, D), (64, 100000, D), (1, 9, D - 1), (1, 9, D)):
        texels, tab = sky(pt, map_n)
        table = sm.light_table(lamps, tab)
        geoms, mats, p, x, outside, hit = shade_records(pt, po, n, depth, D, it, table)
        want = sm.shade_direct(po, it, depth, D, geoms, mats, p, x, texels, outside, hit).view(pt.PATH_DT)
        got = pt.probe_shade_scatter_direct_sky(it, depth, D, geoms, mats, p, x, texels, outside, hit)
        assert_paths_equal(got, want, n)
        live = p["remainingBounces"] > 0
        assert got[~live].tobytes() == p[~live].tobytes()
        target = dm.target_geoms(po, table, it, p["pixelIndex"], D - 1)
        if n >= 7:
            # the crafted records: u0 = 0.5 and above it picks the sky, anything below it the last lamp
            assert (target[:7] == -1).any() and (target[:7] == 7).any()
        if n == 257:
            aimed = live & (target == -1)
            alive = got["remainingBounces"] > 0
            if depth == D:
                scored = (got["color"] != 0).any(axis=1)
                assert not alive.any() and (scored & aimed & (hit == -1)).any() and not (scored & aimed & (hit >= 0)).any()
                assert not (scored & live & ~aimed & (hit == -1)).any() and (scored & live & ~aimed).any()
            elif depth == D - 1:
                matte = live & (x["t"] > 0) & (x["materialId"] >= 1) & (x["materialId"] <= 3)
                assert (alive <= matte).all() and (alive & aimed).any() and (alive & ~aimed).any() and (matte & aimed & ~alive).any()
                assert (got["remainingBounces"][alive] == 1).all()
    # no map: pt_probe_shade_scatter_direct itself
    geoms, mats, p, x, outside, hit = shade_records(pt, po, n, D - 1, D, 3, lamps)
    assert pt.probe_shade_scatter_direct_sky(3, D - 1, D, geoms, mats, p, x, None, outside).tobytes() == \
        pt.probe_shade_scatter_direct(3, D - 1, D, geoms, mats, p, x, outside).tobytes()


def test_shade_probe_refusals(pt, po):
    geoms, mats, _, _ = two_lamps(pt)
    lamps = dm.light_elements(np.ascontiguousarray(geoms).view(po.GEOM_DT), np.ascontiguousarray(mats).view(po.MATERIAL_DT))
    geoms, mats, p, x, outside, _ = shade_records(pt, po, 8, 1, 3, 1, lamps)
    L = pt.library()
    g, m = np.ascontiguousarray(geoms), np.ascontiguousarray(mats)
    h = np.zeros(8, np.int32)
    t = np.ones((6, 2, 2, 3), dtype=F32)
    ok = [1, 1, 3, g.ctypes.data, len(g), m.ctypes.data, len(m), p.ctypes.data, x.ctypes.data, outside.ctypes.data, h.ctypes.data, 8, t.ctypes.data, 2]
    assert L.pt_probe_shade_scatter_direct_sky(*ok) == 0
    for k, v in ((11, -1), (6, 0), (7, None), (8, None), (1, 4), (2, 64), (12, None), (13, -1), (13, 1025)):
        bad = list(ok)
        bad[k] = v
        assert L.pt_probe_shade_scatter_direct_sky(*bad) == -1, k
    final = list(ok)
    final[1], final[10] = 3, None                                   # the final ray needs hit_geom
    assert L.pt_probe_shade_scatter_direct_sky(*final) == -1


# ---- whole pipelines -----------------------------------------------------------------------------------------------------------
def scene_arrays(pt, name):
    """(geoms, materials, camera at W x H, depth, triangles, meshes)"""
    if name.startswith("open sky"):                                 # the sky is the only element; "open sky 8": depth 8
        if "open" not in _cache:
            s = pt.load_scene(os.path.join(ROOT, "scenes", "open_sky_sun.txt"))
            _cache["open"] = (s.geoms, s.materials, _resized(s.camera, W, H))
        return _cache["open"] + (int(name.split()[-1]), None, None)
    if name == "two lamps":                                        # the box is open towards the camera: lamps and sky
        return two_lamps(pt) + (None, None)
    if name == "glossy":
        s = pt.load_scene(os.path.join(ROOT, "scenes", "cornell_glossy.txt"))
        return s.geoms, s.materials, _resized(s.camera, W, H), s.traceDepth, None, None
    if name == "many primitives":                                  # 17 primitives: past the own-surface form's 15
        g, m, c, d = two_lamps(pt)
        blocks = [dm.placed(pt.GEOM_DT, dm.CUBE, 2 + (k & 1), (-3 + 3 * (k % 3), 0.3, -3 + 3 * (k // 3)), (0.6, 0.6, 0.6), (0, 15 * k, 0)) for k in range(9)]
        return np.concatenate([g] + blocks), m, c, 4, None, None
    if name == "mesh":                                             # a matte triangle soup in cornell_two_lamps without its ball
        import mesh_cases
        g, m, c, d = two_lamps(pt)
        tris = mesh_cases.soup(pt.TRI_DT, np.random.default_rng(11), n=50)
        keep = np.concatenate([g[:6], g[7:8]])
        geoms, tris, meshes = pt.meshes.add_mesh(keep, tris, material_id=1)
        return geoms, m, c, 4, tris, meshes
    raise KeyError(name)


def reference(pt, po, name, count, glossy=False, snapshots=False):
    """The model's running sums after iterations 1 .. count under the shared sun sky, the live counts of every iteration and
    (snapshots) the live paths after every bounce; computed once per module and never written afterwards."""
    key = (name, count, glossy, snapshots)
    if key not in _cache:
        geoms, mats, cam, depth, tris, meshes = scene_arrays(pt, name)
        m = sm.Model(po, geoms, mats, cam, depth, tris=tris, meshes=meshes, glossy=glossy)
        m.set_environment(sky(pt)[0])
        out, live, snaps = [], [], []
        for it in range(1, count + 1):
            per_bounce = [] if snapshots else None
            out.append(m.iterate(it, per_bounce).copy())
            live.append(list(m.live))
            snaps.append(per_bounce)
        for a in out:
            a.setflags(write=False)
        _cache[key] = (out, live, snaps, dict(m.counts))
    return _cache[key]


def session(pt, name, flags, env=True, **kw):
    geoms, mats, cam, depth, tris, meshes = scene_arrays(pt, name)
    scene = pt.Scene(geoms, mats, cam, depth, triangles=tris, meshes=meshes) if tris is not None else pt.Scene(geoms, mats, cam, depth)
    pt.pathtraceInit(scene, flags=flags | pt.PT_DIRECT_LIGHT | pt.PT_DIRECT_SKY, **kw)
    if env:
        pt.set_environment(sky(pt)[0])
    return depth


def check_stats(pt, depth, live):
    """D + 1 entries of live; pt_stats.bounces = the last bounce that traced a ray, + 1 (D + 1 whenever a final ray was traced)."""
    st = pt.get_stats()
    assert len(live) == depth + 1 and list(st.live[:depth + 2]) == live + [0], (list(st.live[:depth + 2]), live)
    assert st.bounces == max(d + 1 for d in range(depth + 1) if live[d]) and st.rays == sum(live), (st.bounces, live)


def trace_six_then_four(pt, want, live, depth):
    for it in range(1, 7):
        same(pt.pathtrace(None, 0, it), want[it - 1], "iteration %d" % it)
        check_stats(pt, depth, live[it - 1])
    img = np.zeros((W * H, 3), dtype=np.float32)
    pt.trace_batch(7, 4, img)
    same(img, want[9], "batch of 4")
    same(pt.get_image(W * H), want[9], "device image")
    st = pt.get_stats()
    assert list(st.live[:depth + 1]) == [sum(l[d] for l in live[6:10]) for d in range(depth + 1)]
    assert any(l[depth] > 0 for l in live[:6]) and (st.bounces == depth + 1) == (st.live[depth] > 0)


PIPELINES = {"compact": lambda pt: pt.PT_COMPACT, "plain": lambda pt: 0, "sort fused": lambda pt: pt.PT_COMPACT | pt.PT_SORT_MATERIAL,
             "bvh": lambda pt: pt.PT_COMPACT | pt.PT_MESH_BVH}


@pytest.mark.parametrize("name, flags", [("open sky 1", "compact"), ("open sky 1", "plain"), ("open sky 2", "compact"), ("open sky 2", "sort fused"),
                                         ("open sky 8", "compact"), ("open sky 8", "plain"),
                                         ("two lamps", "compact"), ("two lamps", "plain"), ("two lamps", "sort fused"),
                                         ("mesh", "compact"), ("mesh", "bvh"), ("many primitives", "compact")])
def test_pipelines(pt, po, launch_plan, name, flags):
    """Six pt_trace calls, then a pt_trace_batch of 4, with the statistics of every call: D + 1 bounces, live[D] = the final rays."""
    want, live, _, counts = reference(pt, po, name, 10)
    depth = session(pt, name, PIPELINES[flags](pt), max_batch=4)
    try:
        trace_six_then_four(pt, want, live, depth)
    finally:
        pt.pathtraceFree()
    assert counts["sky aimed"] > 0 and counts["sky cs exits"] > 0 and counts["sky scored"] > 0 and counts["sky occluded"] > 0
    if name == "open sky 1":
        assert counts["sky aimed"] > 1000 and counts["sky cs exits"] > 100 and counts["sky scored"] > 100 and counts["sky occluded"] > 20
    if name.startswith("open sky"):
        assert counts["lamp aimed"] == 0
    else:
        assert counts["sky aimed"] > 500 and counts["lamp aimed"] > 500 and counts["step 6"] > 100 and counts["sky scored"] > 50
        assert counts["occluded"] > counts["sky occluded"] > 100


def test_glossy(pt, po, launch_plan):
    """cornell_glossy with PT_GLOSSY: the ENV x GLOSSY x DIRECT instantiations, fused and sorted."""
    want, live, _, counts = reference(pt, po, "glossy", 10, glossy=True)
    for flags in (pt.PT_COMPACT, pt.PT_COMPACT | pt.PT_SORT_MATERIAL, 0):
        depth = session(pt, "glossy", flags | pt.PT_GLOSSY, max_batch=4)
        try:
            trace_six_then_four(pt, want, live, depth)
        finally:
            pt.pathtraceFree()
    assert counts["hits"] > 1000 and counts["sky scored"] > 0 and counts["lamp aimed"] > 0


def test_five_batches_on_the_lanes(pt, po, launch_plan):
    want, _, _, _ = reference(pt, po, "two lamps", 20)
    session(pt, "two lamps", pt.PT_COMPACT, max_batch=4)
    try:
        for k in range(5):
            pt.trace_batch_async(1 + 4 * k, 4)
        pt.synchronize()
        same(pt.get_image(W * H), want[19])
    finally:
        pt.pathtraceFree()


def test_lookahead_session_whose_map_comes_and_goes(pt, po, launch_plan):
    """PT_LOOKAHEAD | PT_PIN_IMAGE | PT_HOST_SPARSE on the sky-only scene: a map, a black one (the element disappears and a batch
    runs D bounces instead of D + 1; the windows traced ahead are void), the map again in the middle of a window.  The host image
    after every call."""
    geoms, mats, cam, depth, _, _ = scene_arrays(pt, "open sky 2")
    texels = sky(pt)[0]
    black = np.zeros((6, 4, 4, 3), dtype=F32)
    m = sm.Model(po, geoms, mats, cam, depth)
    L = pt.library()
    buf = np.full((W * H, 3), -7.0, dtype=np.float32)
    session(pt, "open sky 2", pt.PT_COMPACT | pt.PT_LOOKAHEAD | pt.PT_PIN_IMAGE | pt.PT_HOST_SPARSE, env=False, max_batch=8, pin_image=False)
    try:
        it = 0
        for env, calls, bounces in ((texels, 3, depth + 1), (black, 3, depth), (texels, 5, depth + 1)):
            pt.set_environment(env)
            m.set_environment(env)
            assert (m.sky is not None) == (bounces == depth + 1)
            for _ in range(calls):
                it += 1
                assert L.pt_trace(None, 0, it, buf.ctypes.data) == 0, L.pt_last_error()
                same(buf, m.iterate(it), "host image after iteration %d" % it)
        same(pt.get_image(W * H), m.image, "device image")
    finally:
        pt.pathtraceFree()


@pytest.mark.parametrize("name", ["two lamps", "open sky 1"])
def test_stepping_interface(pt, po, launch_plan, name):
    """pt_trace_begin / pt_trace_bounce through bounce D with pt_export_paths after every bounce: the pool is the model's live
    paths, in order -- after bounce D - 1 the final rays, aimed at lamps and at the sky -- and pt_get_stats reports D + 1 bounces."""
    want, live, snaps, _ = reference(pt, po, name, 2, snapshots=True)
    depth = session(pt, name, pt.PT_COMPACT, max_batch=2)
    try:
        for it in (1, 2):
            pt.trace_begin(it, 1)
            for d in range(depth + 1):
                n_live = pt.trace_bounce(d)
                paths, n = pt.export_paths(W * H)
                ref = snaps[it - 1][d]
                assert n_live == n == len(ref), (it, d, n_live, n, len(ref))
                assert_paths_equal(paths, ref, n)
                if d == depth - 1:
                    assert n == live[it - 1][depth] > 0 and (paths["remainingBounces"][:n] == 1).all()
            with pytest.raises(pt.PtError):
                pt.trace_bounce(depth + 1)
            pt.trace_end()
            check_stats(pt, depth, live[it - 1])
            same(pt.get_image(W * H), want[it - 1], "iteration %d" % it)
    finally:
        pt.pathtraceFree()


@pytest.mark.parametrize("form", ["devices", "tile"])
def test_tiles_and_devices(pt, po, launch_plan, form):
    """A session over two contexts (devices=[0, 0]: both build the tables) delivers the frame; a session that is tile 1 of 2
    (strips of 8 rows) its own rows, zeros elsewhere."""
    want, _, _, _ = reference(pt, po, "two lamps", 10)
    kw = dict(devices=[0, 0]) if form == "devices" else dict(tile=(1, 2, 8))
    own = np.ones(H, dtype=bool) if form == "devices" else (np.arange(H) // 8) % 2 == 1
    mask = np.repeat(own, W)

    def expect(a):
        return np.where(mask[:, None], a, np.float32(0))

    session(pt, "two lamps", pt.PT_COMPACT, max_batch=4, **kw)
    try:
        for it in (1, 2, 3):
            same(pt.pathtrace(None, 0, it), expect(want[it - 1]), "iteration %d" % it)
        img = np.zeros((W * H, 3), dtype=np.float32)
        pt.trace_batch(4, 4, img)
        same(img, expect(want[6]), "batch")
    finally:
        pt.pathtraceFree()


# ---- the flag ------------------------------------------------------------------------------------------------------------------
def test_a_flagged_session_without_a_map_is_the_direct_session(pt, po, launch_plan):
    """No map, then a black one: direct_model.Model bit for bit, D + 1 bounces for the lamps alone.  Then the sun sky arrives in
    the same session and the sky's element with it."""
    geoms, mats, cam, depth, _, _ = scene_arrays(pt, "two lamps")
    a = dm.Model(po, geoms, mats, cam, depth)
    session(pt, "two lamps", pt.PT_COMPACT, env=False, max_batch=4)
    try:
        for it in (1, 2):
            same(pt.pathtrace(None, 0, it), a.iterate(it), "iteration %d" % it)
            check_stats(pt, depth, list(a.live))
        black = np.zeros((6, 2, 2, 3), dtype=F32)
        pt.set_environment(black)
        a.set_environment(black)
        same(pt.pathtrace(None, 0, 3), a.iterate(3), "under a black map")
        b = sm.Model(po, geoms, mats, cam, depth)
        b.image = a.image.copy()
        b.set_environment(sky(pt)[0])
        pt.set_environment(sky(pt)[0])
        same(pt.pathtrace(None, 0, 4), b.iterate(4), "under the sun sky")
        assert b.counts["sky aimed"] > 0
    finally:
        pt.pathtraceFree()
    # the sky-only scene: without a map there is nothing to sample, D bounces at the most and a black picture
    depth = session(pt, "open sky 2", pt.PT_COMPACT, env=False, max_batch=4)
    try:
        assert not pt.pathtrace(None, 0, 1).any() and pt.get_stats().bounces <= depth
        pt.set_environment(sky(pt)[0])
        want, live, _, _ = reference(pt, po, "open sky 2", 10)
        pt.clear_image()
        same(pt.pathtrace(None, 0, 1), want[0], "after the map arrived")
        check_stats(pt, depth, live[0])
        pt.set_environment(None)
        pt.pathtrace(None, 0, 2)
        assert pt.get_stats().bounces <= depth
    finally:
        pt.pathtraceFree()


def test_the_sky_flag_needs_the_direct_flag(pt):
    geoms, mats, cam, depth, _, _ = scene_arrays(pt, "two lamps")
    with pytest.raises(pt.PtError) as e:
        try:
            pt.pathtraceInit(pt.Scene(geoms, mats, cam, depth), flags=pt.PT_COMPACT | pt.PT_DIRECT_SKY)
        finally:
            pt.pathtraceFree()
    assert "PT_DIRECT_LIGHT" in str(e.value)
    assert pt.PT_DIRECT_SKY == 1 << 15


def test_fake_shader_ignores_both_flags(pt, launch_plan):
    geoms, mats, cam, depth, _, _ = scene_arrays(pt, "two lamps")
    imgs = []
    for extra in (0, pt.PT_DIRECT_SKY, pt.PT_DIRECT_LIGHT | pt.PT_DIRECT_SKY):
        pt.pathtraceInit(pt.Scene(geoms, mats, cam, depth), flags=pt.PT_FAKE_SHADER | extra)
        try:
            pt.set_environment(sky(pt)[0])
            pt.pathtrace(None, 0, 1)
            imgs.append(pt.pathtrace(None, 0, 2).copy())
            assert pt.get_stats().bounces == 1
        finally:
            pt.pathtraceFree()
    assert imgs[0].tobytes() == imgs[1].tobytes() == imgs[2].tobytes() and (imgs[0] != 0).any()


# ---- the headless host ---------------------------------------------------------------------------------------------------------
def test_ptbench_direct_sky(pt, po, tmp_path):
    """ptbench --direct-sky --sky ... --sun ... renders scenes/open_sky_sun.txt (here at 48 x 48, depth 2): the raw running sum it
    saves is the model's; with --direct alone the map is not sampled."""
    w = h = 48
    iters = 4
    txt = open(os.path.join(ROOT, "scenes", "open_sky_sun.txt")).read()
    assert "RES         800 800" in txt and "DEPTH       4" in txt
    scene_file = tmp_path / "open_sky_sun.txt"
    scene_file.write_text(txt.replace("RES         800 800", "RES         %d %d" % (w, h)).replace("DEPTH       4", "DEPTH       2"))
    s = pt.load_scene(str(scene_file))
    assert s.traceDepth == 2
    sky_arg = "16," + ",".join(repr(float(v)) for v in sm.ZENITH + sm.HORIZON + sm.GROUND)
    sun_arg = ",".join(repr(float(v)) for v in sm.SUN_DIR + (sm.SUN_COS,) + sm.SUN_RGB)
    for switch in (["--direct-sky"], ["--direct"]):
        out = tmp_path / ("sky%d" % len(switch[0]))
        p = subprocess.run([pt.build_ptbench(), str(scene_file), "--iters", str(iters), "--save-sum", "--out", str(out), "--sky", sky_arg,
                            "--sun", sun_arg] + switch, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stdout + p.stderr
        got = pt.load_pfm(str(out) + ".%dsamp.sum.pfm" % iters, w, h)
        m = (sm.Model if switch == ["--direct-sky"] else dm.Model)(po, s.geoms, s.materials, s.camera, s.traceDepth)
        m.set_environment(sky(pt)[0])
        for it in range(1, iters + 1):
            m.iterate(it)
        same(got, m.image, "ptbench %s" % " ".join(switch))
        assert (m.counts.get("sky aimed", 0) > 0) == (switch == ["--direct-sky"])


# ---- a furnace -------------------------------------------------------------------------------------------------------------------
def test_furnace(pt, po):
    """A constant sky of 1 and one matte ball of colour 1 at depth 1: a pixel that sees the ball has expectation EXACTLY 1 (the
    ball is convex: a final ray that leaves its surface outwards leaves the scene), every other pixel is 1.  The mean over those
    pixels of 64 iterations is within 5 standard errors (from the 64 per-iteration means) of 1; no frame carries a negative or
    NaN value."""
    s = pt.load_scene(os.path.join(ROOT, "scenes", "open_sky_sun.txt"))
    cam = _resized(s.camera, W, H)
    ball = dm.placed(pt.GEOM_DT, dm.SPHERE, 0, (0, 3, 0), (8, 8, 8))
    mats = np.zeros(1, dtype=pt.MATERIAL_DT)
    mats["color"] = 1.0
    rays = po.generate_rays(cam, 1)
    isects, _ = po.compute_intersections(rays, np.ascontiguousarray(ball).view(po.GEOM_DT))
    on_ball = np.zeros(W * H, dtype=bool)
    on_ball[rays["pixelIndex"][isects["t"] > 0]] = True
    assert 100 < on_ball.sum() < W * H - 100
    pt.pathtraceInit(pt.Scene(ball, mats, cam, 1), flags=pt.PT_COMPACT | pt.PT_DIRECT_LIGHT | pt.PT_DIRECT_SKY, max_batch=4)
    try:
        pt.set_environment(np.ones((6, 4, 4, 3), dtype=F32))
        means = []
        for it in range(1, 65):
            pt.clear_image()
            frame = pt.pathtrace(None, 0, it).astype(np.float64)
            assert np.isfinite(frame).all() and (frame >= 0).all()
            assert (frame[~on_ball] == 1).all()
            means.append(frame[on_ball].mean())
    finally:
        pt.pathtraceFree()
    means = np.array(means)
    se = means.std(ddof=1) / np.sqrt(len(means))
    print("furnace: mean %.5f, standard error %.5f" % (means.mean(), se))
    assert se > 0 and abs(means.mean() - 1) <= 5 * se
