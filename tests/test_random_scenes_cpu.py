"""The random scenes of tests/random_scenes.py, from the models alone (no device): what tests/test_gpu_random_scenes.py compares
the kernels with cannot be vacuous.  The generator is deterministic and builds, seed by seed, the scene the fuzz tool's inline code
always built; every model image, G-buffer, albedo plane and filter output of the chosen seeds is finite (zero-scale primitives
stay in, so the device's byte comparison is never one of NaN payloads); and, summed over each session's seed list, the scenes reach
the branches the sessions are there for -- stated as floors, not as measurements.  The same for the lists of the newer streams:
smoothed hits on every kind of material and every refusal (SMOOTH_SEEDS), sky samples that score and that are occluded (SKY_SEEDS),
and images that are not the pinhole's (CAMERA_SEEDS)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import __graft_entry__ as ge  # noqa: E402
import random_scenes as rs  # noqa: E402

W, H = rs.W, rs.H
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pt():
    p = ge.load_package()
    p.build_host()
    return p


def historical(pt, seed):
    """The scene construction of tests/tools/fuzz_gpu.py's main() as it stood before it moved to random_scenes.draw, draw for draw
    (its PTMI355_WHOLE_MAX coin is returned, not applied): (geoms, materials, camera, depth, coin, the next draw of the stream)."""
    Hl = pt.host_binding.host_library()
    z = np.load(os.path.join(ROOT, "tests", "golden", "scenes.npz"))
    rng = np.random.default_rng(seed)
    nm = int(rng.integers(2, 12))
    mats = np.zeros(nm, dtype=pt.MATERIAL_DT)
    for m in mats:
        m["color"] = rng.uniform(0.1, 1.0, 3)
        m["spec_color"] = rng.uniform(0.5, 1.0, 3)
        kind = rng.integers(4)
        m["hasReflective"], m["hasRefractive"] = (1.0, 0.0) if kind == 1 else ((0.0, 1.0) if kind == 2 else (0.0, 0.0))
        m["indexOfRefraction"] = rng.uniform(1.05, 2.5)
        m["emittance"] = rng.uniform(1, 6) if kind == 3 else 0.0
    mats[0]["emittance"] = 4.0
    ng = int(rng.integers(1, 40))
    geoms = np.zeros(ng, dtype=pt.GEOM_DT)
    for k, g in enumerate(geoms):
        g["type"] = rng.integers(2)
        g["materialid"] = rng.integers(nm)
        g["translation"] = rng.uniform(-5, 5, 3) + (0, 5, 0)
        g["rotation"] = rng.uniform(-180, 180, 3) * (rng.random() < 0.6) + rng.choice([0.0, 90.0, 180.0, 45.0], 3) * (rng.random() < 0.3)
        sc = rng.uniform(0.2, 4.0, 3)
        r = rng.random()
        if r < 0.2:
            sc[rng.integers(3)] = rng.choice([0.02, 0.005, 0.001])
        elif r < 0.25:
            sc = np.full(3, rng.choice([30.0, 100.0]))
        elif r < 0.3:
            sc = np.full(3, rng.choice([1e-2, 1e-4]))
        elif r < 0.33:
            sc[rng.integers(3)] = 0.0
        g["scale"] = sc
        Hl.pth_build_geom_matrices(geoms.ctypes.data + k * pt.GEOM_DT.itemsize)
    depth = int(rng.integers(1, 12))
    cam = np.array(z["cornell_64__camera"], copy=True).reshape(1)
    r = rng.random()
    if r < 0.5:
        cam["position"][0] += rng.uniform(-3, 3, 3).astype(np.float32)
    elif r < 0.6:
        cam["position"][0] += (rng.uniform(-1, 1, 3) * rng.choice([30.0, 300.0])).astype(np.float32)
    if rng.random() < 0.2:
        a = rng.uniform(-0.8, 0.8)
        cam["view"][0] = np.float32([np.sin(a), 0.0, np.cos(a)]) * np.float32(np.sign(cam["view"][0][2]) or 1.0)
    coin = bool(rng.random() < 0.5)
    return geoms, mats, cam, depth, coin, rng.random()


# ---- determinism -----------------------------------------------------------------------------------------------------------------
def test_seed_lists_are_sixteen_literal_seeds():
    for seeds in (rs.PLAIN_SEEDS, rs.GLOSSY_SEEDS, rs.TEXTURED_SEEDS, rs.DIRECT_SEEDS, rs.FILTER_SEEDS):
        assert len(seeds) == 16 and len(set(seeds)) == 16 and len(rs.groups(seeds)) == 4
    assert len(rs.MESH_SEEDS) == 4


@pytest.mark.parametrize("seed", sorted(set(rs.PLAIN_SEEDS + rs.TEXTURED_SEEDS + rs.DIRECT_SEEDS + rs.STATE_SEEDS + (1, 2, 3, 1000, 1049))))
def test_a_seed_builds_the_scene_it_always_built(pt, seed):
    """At the tool's 64 x 64 the new function's bytes are the old inline code's -- geoms, materials, camera, depth, the launch-plan
    coin and the place the stream stands at afterwards; at 40 x 26 only the camera's resolution and pixel lengths differ."""
    old = historical(pt, seed)
    new = rs.draw(pt, seed, 64, 64)
    for a, b in zip(old[:3], new[:3]):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    assert old[3] == new[3] and old[4] == new[4] and old[5] == new[5].random()
    again = rs.scene(pt, seed, 64, 64)
    assert [a.tobytes() for a in again[:3]] == [a.tobytes() for a in new[:3]] and again[3] == new[3]
    small = rs.scene(pt, seed, W, H)
    assert small[0].tobytes() == new[0].tobytes() and small[1].tobytes() == new[1].tobytes() and small[3] == new[3]
    for k in small[2].dtype.names:
        if k not in ("resolution", "pixelLength"):
            assert small[2][k].tobytes() == new[2][k].tobytes(), k
    assert tuple(small[2]["resolution"][0]) == (W, H)


def test_the_second_stream_is_deterministic_and_leaves_the_scene_alone(pt):
    for seed in rs.TEXTURED_SEEDS[:4]:
        geoms, mats, cam, depth = rs.scene(pt, seed, W, H)
        before = mats.tobytes()
        a = rs.features(seed, mats, depth)
        rs.camera_features(seed), rs.sky_of(pt, seed), rs.normals_of(pt, seed, rs.mesh_of(pt, seed, rs.scene(pt, seed, W, H)[0], len(mats))[1])
        b = rs.features(seed, mats, depth)                               # (the newer streams in between: they are streams of their own)
        assert mats.tobytes() == before
        assert a.materials.tobytes() == b.materials.tobytes() and sorted(a.textures) == sorted(b.textures)
        assert all(a.textures[k].tobytes() == b.textures[k].tobytes() for k in a.textures)
        assert all(a.bump_maps[k].tobytes() == b.bump_maps[k].tobytes() for k in a.bump_maps)
        assert (a.sky is None) == (b.sky is None) and (a.sky is None or a.sky.tobytes() == b.sky.tobytes())
        plain = a.materials.copy()
        plain["spec_exponent"] = 0
        assert plain.tobytes() == before and set(np.unique(a.materials["spec_exponent"])) <= {0.0, 2.0, 50.0, 1e4}
        for t in list(a.textures.values()) + list(a.bump_maps.values()):
            assert t.shape[1] in (1, 4, 8) and t.shape == (6, t.shape[1], t.shape[1], 3) and np.abs(t).max() < 16
        assert 1 <= a.direct_depth <= min(depth, rs.MAX_DEPTH - 1)


# ---- the scenes are the hostile ones ---------------------------------------------------------------------------------------------
def test_geometry_floors(pt, po):
    for seeds in (rs.PLAIN_SEEDS, rs.GLOSSY_SEEDS, rs.TEXTURED_SEEDS, rs.DIRECT_SEEDS, rs.FILTER_SEEDS):
        scenes = [rs.scene(pt, s, W, H) for s in seeds]
        assert sum(bool(rs.zero_scaled(g).any()) for g, _, _, _ in scenes) >= 2           # zero-scale primitives stay in
        for g, _, _, _ in scenes:
            z = rs.zero_scaled(g)
            assert not np.isfinite(g["inverseTransform"][z]).any(axis=(1, 2)).any() or not z.any()
        counts = [len(g) for g, _, _, _ in scenes]
        assert max(counts) >= 17 and min(counts) <= 16                                   # either side of the own-surface form's 15 + 1
        depths = {d for _, _, _, d in scenes}
        assert 1 in depths and 2 in depths and max(depths) >= 8
        facts = [rs.first_hit_facts(po, pt, s, W, H) for s in seeds]
        assert max(f[0] for f in facts) > 0.25                                            # a frame with more than a quarter misses
        assert any(f[1] for f in facts)                                                   # a camera inside a primitive
        thin = np.concatenate([g["scale"].min(axis=1) for g, _, _, _ in scenes])
        big = np.concatenate([g["scale"].max(axis=1) for g, _, _, _ in scenes])
        assert (thin == np.float32(0.001)).any() and (big >= 100).any() and (big == np.float32(1e-4)).any()


def finite(*arrays):
    return all(np.isfinite(a).all() for a in arrays)


# ---- the sessions' references: finite, and not vacuous ---------------------------------------------------------------------------
def test_plain_session_images_are_finite(pt, po):
    for seed in rs.PLAIN_SEEDS:
        for oflags in (po.F_COMPACT, 0, po.F_COMPACT | po.F_SORT):
            run = rs.plain_run(po, pt, seed, W, H, oflags)
            assert finite(*run.images.values()), seed
        assert finite(*rs.plain_run(po, pt, seed, W, H, po.F_COMPACT, cam=rs.scene(pt, rs.next_seed(rs.PLAIN_SEEDS, seed), W, H)[2]).images.values())
    lit = sum(bool((rs.plain_run(po, pt, s, W, H, po.F_COMPACT).images[9] != 0).any()) for s in rs.PLAIN_SEEDS)
    assert lit >= 8


def total(dicts, key):
    return sum(d.get(key, 0) for d in dicts)


def test_glossy_session_floors(pt, po):
    counts = []
    for seed in rs.GLOSSY_SEEDS:
        run, c, f = rs.glossy_run(po, pt, seed, W, H)
        assert finite(*run.images.values()), seed
        counts.append(c)
    assert total(counts, "hits") >= 1000 and total(counts, "h fallback") > 0 and total(counts, "r fallback") > 0
    skies = [rs.glossy_run(po, pt, s, W, H)[2].sky is not None for s in rs.GLOSSY_SEEDS]
    assert any(skies) and not all(skies)


def test_textured_session_floors(pt, po):
    counts = []
    for seed in rs.TEXTURED_SEEDS:
        run, c, f = rs.textured_run(po, pt, seed, W, H)
        assert finite(*run.images.values()), seed
        A, out = rs.albedo_run(po, pt, seed, W, H)
        assert finite(A, out), seed
        counts.append(c)
    assert total(counts, "tinted") >= 10000 and total(counts, "bumped") >= 5000 and total(counts, "guarded") >= 100
    assert total(counts, "hits") >= 1000 and total(counts, "h fallback") > 0 and total(counts, "r fallback") > 0
    assert sum(bool((rs.albedo_run(po, pt, s, W, H)[0] != 1).any()) for s in rs.TEXTURED_SEEDS) >= 8
    # the removal after iteration 3 takes something away in most seeds
    fs = [rs.textured_run(po, pt, s, W, H)[2] for s in rs.TEXTURED_SEEDS]
    assert sum(rs.dropped(f)[0] is not None for f in fs) >= 8 and sum(rs.dropped(f)[1] is not None for f in fs) >= 8


def test_direct_session_floors(pt, po):
    counts = []
    for seed in rs.DIRECT_SEEDS:
        assert 0 < rs.light_table_size(po, pt, seed, W, H) <= 1024, seed               # no seed of the list is ever skipped
        run, c, f, elements = rs.direct_run(po, pt, seed, W, H)
        assert finite(*run.images.values()), seed
        counts.append(c)
    assert total(counts, "sampled") >= 1000 and total(counts, "sphere") > 0 and total(counts, "cube") > 0 and total(counts, "inside") >= 1
    final, occluded = total(counts, "final rays"), total(counts, "occluded")
    assert final >= 300 and 0 < occluded < final                                         # some are occluded, some score
    assert total(counts, "hits") >= 1000 and total(counts, "h fallback") > 0 and total(counts, "r fallback") > 0


def test_filter_session_floors(pt, po):
    kept = []
    for seed in rs.FILTER_SEEDS:
        fr = rs.filter_run(po, pt, seed, rs.next_seed(rs.FILTER_SEEDS, seed), W, H)
        for g in fr["g"]:
            assert finite(g["t"], g["normal"], g["position"]), seed
        assert finite(*fr["images"]) and finite(*fr["denoise"].values()), seed
        for res, hc, hn in fr["temporal"]:
            assert finite(res, hc, hn), seed
        assert fr["kept"][0] == 0
        kept += fr["kept"][1:]
    assert max(kept) > 0.5 and min(kept) < 0.05                                           # history that survives a move, and history that does not
    far = [np.abs(rs.filter_run(po, pt, s, rs.next_seed(rs.FILTER_SEEDS, s), W, H)["g"][0]["position"]).max() for s in rs.FILTER_SEEDS]
    assert max(far) >= 50


# ---- the first-state table's list ------------------------------------------------------------------------------------------------
def test_first_state_list_is_glass_free_and_literal(pt):
    assert len(rs.STATE_SEEDS) == 16 and len(set(rs.STATE_SEEDS)) == 16 and len(rs.groups(rs.STATE_SEEDS)) == 4
    for seed in rs.STATE_SEEDS:
        mats = rs.scene(pt, seed, W, H)[1]
        assert not (mats["hasRefractive"] > 0).any(), seed                                # pt_init gives the session its table
    assert set(rs.STATE_DIRECT_SEEDS) <= set(rs.STATE_SEEDS) and len(set(rs.STATE_DIRECT_SEEDS)) == len(rs.STATE_DIRECT_SEEDS)


def on(facts, cond):
    return sum(bool(cond(f)) for f in facts)


def test_first_state_list_floors(pt, po):
    """What the oracle's bounce-0 snapshots say about the list (random_scenes.first_state_facts), as floors."""
    w, h = rs.STATE_FRAME
    facts = [rs.first_state_facts(po, pt, s, w, h) for s in rs.STATE_SEEDS]
    for f in facts:
        assert sum(f.count.values()) == w * h and sum(f.tiles.values()) == w * h // 64
    for kind in rs.STATE_KINDS:
        assert on(facts, lambda f: f.count[kind] > 0) >= 6, kind
    assert on(facts, lambda f: all(f.count[k] > 0 for k in rs.STATE_KINDS)) >= 3          # all four kinds in one frame
    assert on(facts, lambda f: f.tiles["ended"] > 0 and f.tiles["mixed"] > 0) >= 5         # tiles the words skip beside tiles they do not
    assert on(facts, lambda f: f.tiles["ended"] == w * h // 64) >= 1
    assert on(facts, lambda f: f.tiles["ended"] == 0) >= 5
    assert on(facts, lambda f: f.primitives <= 16) >= 3 and on(facts, lambda f: f.primitives == 16) >= 1
    assert on(facts, lambda f: f.primitives >= 17) >= 8                                   # either side of the own-surface form's 15 + 1
    assert on(facts, lambda f: f.depth == 1) == 1 and on(facts, lambda f: f.depth == 2) >= 2 and on(facts, lambda f: f.depth >= 8) >= 3
    assert sum(bool(rs.zero_scaled(rs.scene(pt, s, w, h)[0]).any()) for s in rs.STATE_SEEDS) >= 4
    assert on(facts, lambda f: f.inside) >= 6
    # 40 x 26: no words, the kinds still occur
    small = [rs.first_state_facts(po, pt, s, W, H) for s in rs.STATE_SEEDS]
    for kind in rs.STATE_KINDS:
        assert on(small, lambda f: f.count[kind] > 0) >= 2, kind


def test_first_state_session_images_are_finite(pt, po):
    frames = [(s,) + rs.STATE_FRAME for s in rs.STATE_SEEDS] + [(s, W, H) for s in rs.STATE_SEEDS] + [(rs.STATE_SEEDS[0],) + rs.WIDE]
    for seed, w, h in frames:
        assert finite(*rs.plain_run(po, pt, seed, w, h, po.F_COMPACT).images.values()), (seed, w, h)
        cam2 = rs.scene(pt, rs.next_seed(rs.STATE_SEEDS, seed), w, h)[2]
        assert finite(*rs.plain_run(po, pt, seed, w, h, po.F_COMPACT, cam=cam2).images.values()), (seed, w, h)
    lit = sum(bool((rs.plain_run(po, pt, s, *rs.STATE_FRAME, po.F_COMPACT).images[9] != 0).any()) for s in rs.STATE_SEEDS)
    assert lit >= 8


def test_first_state_direct_subset(pt, po):
    assert len(rs.STATE_DIRECT_SEEDS) >= 6
    lit = 0
    for seed in rs.STATE_DIRECT_SEEDS:
        for w, h in (rs.STATE_FRAME, (W, H)):
            geoms, mats, cam, depth = rs.scene(pt, seed, w, h)
            assert depth >= rs.STATE_DIRECT_MIN_DEPTH, seed                              # bounces 0 and 1 are plain ones
            assert 0 < rs.light_table_size(po, pt, seed, w, h) <= 1024, seed
            run, counts, elements = rs.plain_direct_run(po, pt, seed, w, h)
            assert finite(*run.images.values()), seed
            lit += counts.get("final rays", 0)
    assert lit >= 300                                                                     # the sessions do reach their final rays


def test_mesh_session_images_are_finite(pt, po):
    for seed in rs.MESH_SEEDS:
        assert finite(*rs.plain_run(po, pt, seed, W, H, po.F_COMPACT, mesh=True).images.values()), seed
        run, c, f = rs.textured_run(po, pt, seed, W, H, mesh=True)
        assert finite(*run.images.values()), seed
    assert sum(rs.textured_run(po, pt, s, W, H, mesh=True)[1]["tinted"] for s in rs.MESH_SEEDS) > 0


# ---- the newer streams: camera features, vertex normals, sampled skies ----------------------------------------------------------
NEW_LISTS = (rs.SMOOTH_SEEDS, rs.SKY_SEEDS, rs.CAMERA_SEEDS)


def test_new_seed_lists_are_literal_and_group_in_fours():
    assert len(rs.SMOOTH_SEEDS) == 8 and len(rs.CAMERA_SEEDS) == 8 and len(rs.SKY_SEEDS) == 16
    for seeds in NEW_LISTS:
        assert all(type(s) is int for s in seeds) and len(set(seeds)) == len(seeds)
        assert len(seeds) % 4 == 0 and all(len(g) == 4 for g in rs.groups(seeds))
    assert set(rs.SKY_OPENED) <= set(rs.SKY_SEEDS) and len(set(rs.SKY_OPENED)) == len(rs.SKY_OPENED)


def test_the_newer_streams_are_deterministic_and_leave_the_scene_alone(pt):
    """camera_features, normals_of, sky_of and opened(): the same values twice, and scene() and features() byte for byte what they
    were before the call."""
    def snapshot(seed):
        geoms, mats, cam, depth = rs.scene(pt, seed, W, H)
        f = rs.features(seed, mats, depth)
        parts = [geoms.tobytes(), mats.tobytes(), cam.tobytes(), bytes([depth]), f.materials.tobytes(), b"" if f.sky is None else f.sky.tobytes()]
        parts += [f.textures[k].tobytes() for k in sorted(f.textures)] + [f.bump_maps[k].tobytes() for k in sorted(f.bump_maps)]
        return parts

    for seed in sorted(set(rs.SMOOTH_SEEDS[:3] + rs.SKY_SEEDS[:5] + rs.CAMERA_SEEDS[:3])):
        before = snapshot(seed)
        geoms, mats, cam, depth = rs.scene(pt, seed, W, H)
        kept = geoms.tobytes()
        a, b = rs.camera_features(seed), rs.camera_features(seed)
        assert a == b and type(a[0]) is bool and a[1][0] in rs.RADII and a[1][1] in rs.FOCALS
        _, tris, _ = rs.mesh_of(pt, seed, geoms, len(mats))
        tri_bytes = tris.tobytes()
        n1, n2 = rs.normals_of(pt, seed, tris), rs.normals_of(pt, seed, tris)
        assert n1.dtype == np.float32 and n1.shape == (len(tris), 3, 3) and n1.tobytes() == n2.tobytes() and tris.tobytes() == tri_bytes
        s1, s2 = rs.sky_of(pt, seed), rs.sky_of(pt, seed)
        assert s1[0].tobytes() == s2[0].tobytes() and s1[1] is s2[1] and type(s1[1]) is bool
        assert s1[0].dtype == np.float32 and s1[0].shape[1] in (1, 4, 16) and s1[0].shape == (6, s1[0].shape[1], s1[0].shape[1], 3)
        assert np.isfinite(s1[0]).all() and (s1[0] >= 0).all()
        o1, o2 = rs.opened(geoms), rs.opened(geoms)
        assert o1.tobytes() == o2.tobytes() and geoms.tobytes() == kept and 1 <= len(o1) <= len(geoms)
        assert (o1["scale"].max(axis=1) < 30).all() or len(o1) == 1
        assert snapshot(seed) == before


def test_normals_of_is_hostile(pt):
    """What smooth_cases' hostile scene does to its normals, on the soup: every 7th triangle faces away, every 11th is zero, a NaN,
    an infinite corner, lengths of 1e-20 and 1e20, a single zero corner; no facet normal that is not finite gets in."""
    import smooth_model
    seed = rs.SMOOTH_SEEDS[0]
    geoms, mats, cam, depth = rs.scene(pt, seed, W, H)
    _, tris, _ = rs.mesh_of(pt, seed, geoms, len(mats))
    vn = rs.normals_of(pt, seed, tris)
    fn = smooth_model.facet_normals(tris)
    flat = tris.copy()                                                                    # a zero-area triangle has no facet normal:
    flat["v1"][20] = flat["v2"][20] = flat["v0"][20]                                      # its base is 0, its corners the lean alone
    assert not np.isfinite(smooth_model.facet_normals(flat)[20]).any()
    vf = rs.normals_of(pt, seed, flat)
    assert np.isfinite(vf[20]).all() and vf[20].any() and np.abs(vf[20]).max() < 4 and vf[21].tobytes() == vn[21].tobytes()
    bad = ~np.isfinite(vn).all(axis=(1, 2))
    assert sorted(np.nonzero(bad)[0].tolist()) == [2, 4]                                  # only the two that were put there
    assert np.isnan(vn[2, 1, 0]) and np.isinf(vn[4, 2]).all()
    assert not vn[3::11].any() and not vn[10, 2].any() and vn[10, 0].any() and vn[10, 1].any()
    ok = np.isfinite(fn).all(axis=1)
    mean = vn.astype(np.float64).mean(axis=1)
    with np.errstate(all="ignore"):
        side = (mean * fn).sum(axis=1)
    plain = np.ones(len(tris), dtype=bool)
    plain[[2, 4, 6, 8, 10]] = False
    plain[3::11] = False
    away = np.zeros(len(tris), dtype=bool)
    away[0::7] = True
    assert (side[ok & plain & away] < 0).mean() > 0.9 and (side[ok & plain & ~away] > 0).mean() > 0.9
    assert 0 < np.abs(vn[6]).max() < 1e-18 and np.abs(vn[8]).max() > 1e18


def test_smooth_session_floors(pt, po):
    stats, differ = [], 0
    for seed in rs.SMOOTH_SEEDS:
        run, st, s = rs.smooth_run(po, pt, seed, W, H)
        assert sorted(run.images) == list(range(1, 8)) and finite(*run.images.values()), seed
        kept = rs.smooth_run(po, pt, seed, W, H, last=5, keep=True)[0]
        assert kept.images[3].tobytes() == run.images[3].tobytes()
        differ += kept.images[5].tobytes() != run.images[5].tobytes()
        stats.append(st)
    for kind in ("smoothed matte", "smoothed mirror", "smoothed glass"):
        assert sum(st.get(kind, 0) > 0 for st in stats) >= 2, kind
    assert total(stats, "guarded") >= 100
    assert total(stats, "refused2") > 0 and total(stats, "refused4") > 0 and total(stats, "refused5") > 0
    assert differ >= 6                                                                    # the removal takes something away
    scenes = [rs.scene(pt, s, W, H) for s in rs.SMOOTH_SEEDS]
    assert max(len(g) for g, _, _, _ in scenes) >= 17 and min(d for _, _, _, d in scenes) <= 2
    assert finite(*rs.smooth_run(po, pt, rs.SMOOTH_SEEDS[0], *rs.WIDE)[0].images.values())


def test_sky_session_floors(pt, po):
    import glossy_model as gm
    counts, sessions = [], []
    for seed in rs.SKY_SEEDS:
        run, c, s, elements = rs.sky_run(po, pt, seed, W, H)
        assert sorted(run.images) == list(range(1, 8)) and finite(*run.images.values()), seed
        assert 1 <= elements <= 1024, seed                                                # the lamps' elements and the sky's: no seed is ever skipped
        assert c.get("negative or nan weights", 0) == 0, seed
        assert len(run.live[1]) == s.depth + 1 and len(run.live[7]) == s.depth + 1         # D + 1 bounces while a map is set
        assert len(run.live[4]) == (s.depth + 1 if elements > 1 else s.depth), seed           # ... or lamps' elements exist
        assert not s.lamps_off or elements == 1, seed
        assert s.lamps_off == (not (s.materials["emittance"] > 0).any())
        assert (seed in rs.SKY_OPENED) == (len(s.geoms) < len(rs.scene(pt, seed, W, H)[0])), seed
        if s.lamps_off:                                                                   # without its map the session is the plain one
            m = gm.Model(po, s.geoms, s.materials, s.cam, s.depth, glossy=True)
            m.image = run.images[3].copy()
            for it in (4, 5):
                m.iterate(it)
            assert m.image.tobytes() == run.images[5].tobytes(), seed
        counts.append(c)
        sessions.append(s)
    assert total(counts, "sky aimed") >= 1000 and total(counts, "lamp aimed") >= 1000
    assert total(counts, "sky scored") >= 100 and sum(c.get("sky scored", 0) > 0 for c in counts) >= 4
    assert total(counts, "sky occluded") > 0
    assert sum(s.lamps_off for s in sessions) >= 2
    assert any(s.texels.shape[1] == 1 for s in sessions) and any(s.depth == 1 for s in sessions)
    assert finite(*rs.sky_run(po, pt, rs.SKY_SEEDS[0], *rs.WIDE)[0].images.values())


def test_camera_list_floors(pt, po):
    feats = [rs.camera_features(s) for s in rs.CAMERA_SEEDS]
    assert sum(aa and not lens[0] > 0 for aa, lens in feats) >= 2                         # jitter only
    assert sum(lens[0] > 0 and not aa for aa, lens in feats) >= 2                         # a lens only: the sessions that call pt_set_lens
    assert sum(aa and lens[0] > 0 for aa, lens in feats) >= 2
    assert any(lens[0] == 2.0 for _, lens in feats) and any(lens[0] > 0 and lens[1] == 0.5 for _, lens in feats)
    scenes = [rs.scene(pt, s, W, H) for s in rs.CAMERA_SEEDS]
    assert max(len(g) for g, _, _, _ in scenes) >= 17
    # depth 1 with lamps: bounce 0 of the direct session is a DIRECT bounce that generates its rays
    assert any(d == 1 and 0 < rs.light_table_size(po, pt, s, W, H) <= 1024 for s, (_, _, _, d) in zip(rs.CAMERA_SEEDS, scenes))
    assert all(rs.light_table_size(po, pt, s, W, H) <= 1024 for s in rs.CAMERA_SEEDS)     # no direct session of the list is refused
    glass_free = [s for s, (_, m, _, _) in zip(rs.CAMERA_SEEDS, scenes) if not (m["hasRefractive"] > 0).any()]
    assert len(glass_free) >= 2
    # ... of which one has a lens only and depth 2 or more: its pinhole stretch takes the first-state table
    assert any(rs.lens_only(s) and rs.scene(pt, s, W, H)[3] >= 2 for s in glass_free)


@pytest.mark.parametrize("kind", rs.CAMERA_KINDS)
def test_camera_sessions_depend_on_the_camera(pt, po, kind):
    """Every image of every camera run is finite, and after iteration 3 it is not the pinhole session's: no comparison on the
    device can pass by ignoring the jitter or the lens.  A seed with a lens and no jitter goes on for five iterations, the others
    for one."""
    for seed in rs.CAMERA_SEEDS:
        run = rs.camera_run(po, pt, kind, seed, W, H)
        plan = run.plan
        assert sorted(run.images) == list(range(1, plan.last + (6 if rs.lens_only(seed) else 2))), seed
        assert finite(*run.images.values()), seed
        pinhole = rs.camera_run(po, pt, kind, seed, W, H, camera=False, last=3)
        assert pinhole.images[3].tobytes() != run.images[3].tobytes(), seed
        assert len(run.stepped) == run.live[plan.step][1] if len(run.live[plan.step]) > 1 else True
        if kind == "moments":
            assert finite(*run.moments[plan.last])
    assert finite(*rs.camera_run(po, pt, kind, rs.CAMERA_SEEDS[0], *rs.WIDE).images.values())


def test_wide_frames_are_finite(pt, po):
    w, h = rs.WIDE
    assert finite(*rs.plain_run(po, pt, rs.PLAIN_SEEDS[0], w, h, po.F_COMPACT).images.values())
    assert finite(*rs.glossy_run(po, pt, rs.GLOSSY_SEEDS[0], w, h)[0].images.values())
    assert finite(*rs.textured_run(po, pt, rs.TEXTURED_SEEDS[0], w, h)[0].images.values())
    assert finite(*rs.direct_run(po, pt, rs.DIRECT_SEEDS[0], w, h)[0].images.values())
    fr = rs.filter_run(po, pt, rs.FILTER_SEEDS[0], rs.FILTER_SEEDS[1], w, h)
    assert finite(*fr["images"]) and finite(*fr["denoise"].values()) and all(finite(*t) for t in fr["temporal"])
    assert all(finite(g["t"], g["normal"], g["position"]) for g in fr["g"])
    assert finite(*rs.albedo_run(po, pt, rs.TEXTURED_SEEDS[0], w, h))
