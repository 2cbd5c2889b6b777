"""PT_SORT_MATERIAL at its key-count edges: the three device forms of the sort -- fused (k_bounce<..., SORT>, up to 64 materials),
wave-private two-kernel (k_sort_hist + k_shade_sorted_w, up to 64 bins) and workgroup-wide two-kernel (k_sort_hist +
k_shade_sorted, 65 to 2048 bins) -- on the mosaic rooms of tests/sort_cases.py, whose 1 to 2047 materials put up to 47 keys
into a tile and 136 into a chunk, against the CPU oracle's stable sort: bit for bit, bounce by bounce and through whole calls.
tests/test_sort_cases_cpu.py holds the oracle's order against its specification and shows what the rooms cover.

Which form a session takes is pt_init's and enqueue_bounce's rule (sort_cases.form_of restates it); the session exposes one fact
about it, the profile's `sort` stage -- k_sort_hist's launches, none in the fused form.  Wave-private against workgroup-wide is
the rule's word alone: nbins <= 64 or not."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import __graft_entry__ as ge  # noqa: E402,F401
import sort_cases as sc  # noqa: E402
from gpu_common import pt, launch_plan, bits, assert_paths_equal  # noqa: E402,F401

pytestmark = pytest.mark.gpu

COMPACTING = [r for r in sc.RUNS if sc.BY_ID[r[0]].compact]
UNCOMPACTED = [r for r in sc.RUNS if not sc.BY_ID[r[0]].compact]
DEPTH = sc.DEPTH


def session(pt, case, frame, flags=None, max_batch=1, materials=None, room=None):
    geoms, mats = sc.scene_of(pt, case) if room is None else room
    scene = pt.Scene(geoms, mats if materials is None else materials, sc.camera(*frame), DEPTH)
    pt.pathtraceInit(scene, flags=case.pt_flags(pt) if flags is None else flags, max_batch=max_batch)
    return scene


def at(case, frame, it=None, d=None):
    s = "case %s (%d materials, %s form, %d x %d)" % (case.id, case.M, case.form, frame[0], frame[1])
    if it is not None:
        s += ", iteration %d" % it
    if d is not None:
        s += ", bounce %d" % d
    return s


def check_order(po, pt, case, frame, ref, it, d, got_pix, want_pix):
    """The pool's pixel-index sequence; a mismatch names the first differing slot, both pixel indices and both keys."""
    if len(got_pix) == len(want_pix) and (got_pix == want_pix).all():
        return
    pool = sc.entering(po, ref, frame, it, d)
    keys = dict(zip(pool["pixelIndex"].tolist(), sc.keys_entering(po, sc.scene_of(pt, case)[0], case.M, pool).tolist()))
    m = min(len(got_pix), len(want_pix))
    diff = np.nonzero(got_pix[:m] != want_pix[:m])[0]
    slot = int(diff[0]) if len(diff) else m
    g = int(got_pix[slot]) if slot < len(got_pix) else None
    w = int(want_pix[slot]) if slot < len(want_pix) else None
    pytest.fail("%s: %d of %d pool slots differ, the first is slot %d (%% 64 = %d, %% 128 = %d, %% 512 = %d): pixel %s with key %s, "
                "the oracle has pixel %s with key %s there (miss bin = %d)"
                % (at(case, frame, it, d), len(diff) + abs(len(got_pix) - len(want_pix)), max(len(got_pix), len(want_pix)), slot,
                   slot % 64, slot % 128, slot % 512, g, keys.get(g), w, keys.get(w), case.M))


def check_counts(pt, case, frame, what, live, rays):
    gs = pt.get_stats()
    assert list(gs.live[:DEPTH]) == list(live), "%s, %s: live counts %s, the oracle's %s" % (at(case, frame), what, list(gs.live[:DEPTH]), list(live))
    assert gs.rays == rays, "%s, %s: %d rays, the oracle's %d" % (at(case, frame), what, gs.rays, rays)


def check_image(case, frame, what, got, want):
    bad = (bits(got) != bits(want)).any(axis=1)
    if bad.any():
        p = int(np.nonzero(bad)[0][0])
        pytest.fail("%s, %s: %d of %d pixels differ, the first is pixel %d: %s, the oracle's %s"
                    % (at(case, frame), what, int(bad.sum()), len(bad), p, got[p].tolist(), want[p].tolist()))


@pytest.mark.parametrize("run", COMPACTING, ids=sc.run_id)
def test_bounce_by_bounce(pt, po, run):
    """Iterations 1 and 2 through the stepping interface: after every bounce the live count, the pool's pixel-index sequence and
    the full path state are the oracle's; the bounces after the pool has emptied are launched too (n = 0, a zeroed table)."""
    case, frame = sc.BY_ID[run[0]], run[1]
    ref = sc.reference(po, pt, case, frame)
    n = frame[0] * frame[1]
    session(pt, case, frame)
    try:
        for it in (1, 2):
            snaps = ref.snaps[it]
            pt.trace_begin(it, 1)
            for d in range(DEPTH):
                n_live = pt.trace_bounce(d)
                paths, live = pt.export_paths(n)
                want_n = snaps[d]["n_live"] if d < len(snaps) else 0
                assert n_live == live == want_n == len(paths), "%s: %d live paths (export: %d), the oracle's %d" % (at(case, frame, it, d), n_live, live, want_n)
                if want_n:
                    want = snaps[d]["paths"]
                    check_order(po, pt, case, frame, ref, it, d, paths["pixelIndex"], want["pixelIndex"][:want_n])
                    try:
                        assert_paths_equal(paths, want, want_n)
                    except AssertionError as e:
                        pytest.fail("%s: the pool's order is the oracle's, its path state is not (%s)" % (at(case, frame, it, d), e))
            pt.trace_end()
            check_counts(pt, case, frame, "stepped iteration %d" % it, ref.live[it], ref.rays[it])
            check_image(case, frame, "stepped iteration %d" % it, pt.get_image(n), ref.images[it])
    finally:
        pt.pathtraceFree()


@pytest.mark.parametrize("run", sc.RUNS, ids=sc.run_id)
def test_whole_calls(pt, po, run):
    """Three pathtrace() calls (below 65 bins bounce 0 is k_shade_sorted_w<..., GEN>), then one batch of three in a session of its
    own (sample_of != 0; 18 chunks at 64 x 48): image, live counts and rays -- and the profile's `sort` stage says whether the
    two-kernel form ran."""
    case, frame = sc.BY_ID[run[0]], run[1]
    ref = sc.reference(po, pt, case, frame)
    n = frame[0] * frame[1]
    session(pt, case, frame)
    try:
        pt.set_profiling(True)
        for it in sc.ITERATIONS:
            img = pt.pathtrace(None, 0, it)
            check_counts(pt, case, frame, "pathtrace(%d)" % it, ref.live[it], ref.rays[it])
            check_image(case, frame, "pathtrace(%d)" % it, img, ref.images[it])
        ms, launches = pt.get_profile()["sort"]
        if case.form == "fused":
            assert (ms, launches) == (0.0, 0), "%s: k_sort_hist ran %d times in a session that should take the fused form" % (at(case, frame), launches)
        else:
            assert launches == len(sc.ITERATIONS) * DEPTH and ms > 0.0, \
                "%s: k_sort_hist ran %d times (%.3f ms), expected once per bounce" % (at(case, frame), launches, ms)
    finally:
        pt.pathtraceFree()
    session(pt, case, frame, max_batch=3)
    try:
        img = np.zeros((n, 3), dtype=np.float32)
        pt.trace_batch(1, 3, img)
        check_image(case, frame, "trace_batch(1, 3)", img, ref.images[3])
        if case.compact:
            live = [sum(ref.live[it][d] for it in sc.ITERATIONS) for d in range(DEPTH)]
            check_counts(pt, case, frame, "trace_batch(1, 3)", live, sum(ref.rays[it] for it in sc.ITERATIONS))
    finally:
        pt.pathtraceFree()


@pytest.mark.parametrize("run", UNCOMPACTED, ids=sc.run_id)
def test_uncompacted_bounce_by_bounce(pt, po, run):
    """PT_SORT_MATERIAL without compaction: ended paths stay in the pool, so the alive paths are compared as a set keyed by pixel
    index -- the same pixels alive after every bounce, their state the oracle's bit for bit."""
    case, frame = sc.BY_ID[run[0]], run[1]
    ref = sc.reference(po, pt, case, frame)
    n = frame[0] * frame[1]
    session(pt, case, frame)
    try:
        for it in (1, 2):
            snaps = ref.snaps[it]
            pt.trace_begin(it, 1)
            for d in range(DEPTH):
                pt.trace_bounce(d)
                paths, _ = pt.export_paths(n)
                got = paths[paths["pixelIndex"] >= 0]
                got = got[np.argsort(got["pixelIndex"], kind="stable")]
                if d < len(snaps):
                    want = snaps[d]["paths"]
                    want = want[want["remainingBounces"] > 0]
                    want = want[np.argsort(want["pixelIndex"], kind="stable")]
                else:
                    want = got[:0]
                same = len(got) == len(want) and (got["pixelIndex"] == want["pixelIndex"]).all()
                assert same, "%s: %d paths alive, the oracle's %d; pixels alive on one side only: %s" % (
                    at(case, frame, it, d), len(got), len(want), np.setxor1d(got["pixelIndex"], want["pixelIndex"])[:8].tolist())
                try:
                    assert_paths_equal(got, want, len(want))
                except AssertionError as e:
                    pytest.fail("%s: the same pixels are alive, their state differs (%s)" % (at(case, frame, it, d), e))
            pt.trace_end()
            check_counts(pt, case, frame, "stepped iteration %d" % it, ref.live[it], ref.rays[it])
            check_image(case, frame, "stepped iteration %d" % it, pt.get_image(n), ref.images[it])
    finally:
        pt.pathtraceFree()


def long_batch(pt, po, workgroups):
    """One batch of the g65 room with more 512-path chunks than `workgroups`: the image -- every pixel's sum in iteration order --
    and the ray count against the oracle's (its iterations on the host's threads, computed once per batch length)."""
    case, frame = sc.BY_ID["g65"], sc.FRAME
    n = frame[0] * frame[1]
    count = (workgroups * sc.CHUNK) // n + 2
    assert -(-count * n // sc.CHUNK) > workgroups and count * n < 1 << 22
    key = ("long batch", count)
    if key not in sc._cache:
        geoms, mats = sc.scene_of(pt, case)
        ref = po.Tracer(np.ascontiguousarray(geoms).view(po.GEOM_DT), mats.view(po.MATERIAL_DT), sc.camera(*frame), DEPTH,
                        flags=case.oracle_flags(po), trig=po.TRIG_SHARED)
        sc._cache[key] = (ref, ref.iterate_parallel(1, count, min(16, os.cpu_count() or 1)))
    ref, rays = sc._cache[key]
    session(pt, case, frame, max_batch=count)
    try:
        img = np.zeros((n, 3), dtype=np.float32)
        pt.trace_batch(1, count, img)
        got = pt.get_stats().rays
        assert got == rays, "%s, trace_batch(1, %d): %d rays, the oracle's %d" % (at(case, frame), count, got, rays)
        check_image(case, frame, "trace_batch(1, %d)" % count, img, ref.image)
    finally:
        pt.pathtraceFree()


def test_several_chunks_per_workgroup(pt, po):
    """The sort kernels' grid is one workgroup per 512-path chunk up to eight per CU; past that a workgroup walks several chunks
    and phase E of k_shade_sorted moves its output positions on from one to the next, while the workgroups at the end of the
    grid own no chunk at all.  One batch of the g65 room with more chunks than that (342 iterations of 64 x 48 on 256 CUs: 2052
    chunks for 2048 workgroups, a table of 66 x 2048 words through the scan's stepped path)."""
    import torch
    long_batch(pt, po, 8 * torch.cuda.get_device_properties(0).multi_processor_count)


def sky(pt):
    return pt.gradient_cubemap(4, (0.5, 0.7, 1.6), (1.0, 0.9, 0.7), (0.2, 0.15, 0.1))


@pytest.mark.parametrize("glossy", [False, True], ids=["environment", "environment + glossy"])
def test_workgroup_form_shading_variants(pt, po, glossy):
    """The ENV and ENV x GLOSSY instantiations of k_shade_sorted (65 materials, 64 x 48): under a 4-texel gradient sky the open
    front's misses -- 1051, some 435 and some 230 in the first three bounces (tests/test_sort_cases_cpu.py) -- end with the map's
    radiance; with PT_GLOSSY the room's mirrors and glass carry exponents.  Image and live counts equal the models'."""
    import glossy_model as gm
    case, frame = sc.BY_ID["g65"], sc.FRAME
    geoms, mats = sc.scene_of(pt, case)
    mats = mats.copy()
    if glossy:
        kind = np.arange(case.M) % 8
        mats["spec_exponent"] = np.where(kind == sc.MIRROR, 50.0, np.where(kind == sc.GLASS, 200.0, 0.0))
        model = gm.Model(po, geoms, mats, sc.camera(*frame), DEPTH, glossy=True)
    else:
        import environment_model as em
        model = em.Model(po, geoms, mats.view(po.MATERIAL_DT), sc.camera(*frame), DEPTH)
    model.set_environment(sky(pt))
    counter = gm.Model(po, geoms, mats, sc.camera(*frame), DEPTH, glossy=glossy)       # the live counts: the survivors of every bounce
    n = frame[0] * frame[1]
    session(pt, case, frame, flags=case.pt_flags(pt) | (pt.PT_GLOSSY if glossy else 0), materials=mats)
    try:
        pt.set_environment(sky(pt))
        for it in (1, 2):
            want = model.iterate(it)
            snaps = []
            counter.colours(it, snaps)
            live = ([n] + [len(s) for s in snaps] + [0] * DEPTH)[:DEPTH]
            img = pt.pathtrace(None, 0, it)
            got = list(pt.get_stats().live[:DEPTH])
            assert got == live, "%s, pathtrace(%d): live counts %s, the model's %s" % (at(case, frame), it, got, live)
            check_image(case, frame, "pathtrace(%d) under the sky%s" % (it, " with PT_GLOSSY" if glossy else ""), img, want)
        assert live[1] > 0 and np.isfinite(want).all()
    finally:
        pt.pathtraceFree()


def test_the_limit(pt, po):
    """2047 materials initialise (the g2047 cases); 2048 are refused with PT_SORT_MATERIAL, the session stays usable -- the same
    2048-material room under PT_COMPACT alone is the oracle's; the flags that need the fused form initialise at 64 materials and
    are refused at 65 with their own messages."""
    frame = sc.FRAME
    n = frame[0] * frame[1]
    room = sc.mosaic_room(pt, 2048, seed=sc.SEED)
    scene = pt.Scene(room[0], room[1], sc.camera(*frame), DEPTH)
    L = pt.library()
    try:
        for flags in (pt.PT_COMPACT | pt.PT_SORT_MATERIAL, pt.PT_SORT_MATERIAL):
            with pytest.raises(pt.PtError):
                pt.pathtraceInit(scene, flags=flags)
            assert L.pt_last_error().decode() == "pt_init: PT_SORT_MATERIAL keeps one bin per material in LDS: at most 2047 materials"
        pt.pathtraceInit(scene, flags=pt.PT_COMPACT)
        ref = po.Tracer(np.ascontiguousarray(room[0]).view(po.GEOM_DT), room[1].view(po.MATERIAL_DT), sc.camera(*frame), DEPTH,
                        flags=po.F_COMPACT, trig=po.TRIG_SHARED)
        st = ref.iterate(1)
        img = pt.pathtrace(None, 0, 1)
        assert list(pt.get_stats().live[:DEPTH]) == list(st.live[:DEPTH])
        assert img.tobytes() == ref.image.tobytes()
        pt.pathtraceFree()
        sort = pt.PT_COMPACT | pt.PT_SORT_MATERIAL
        refused = {
            pt.PT_DIRECT_LIGHT: "pt_init: PT_DIRECT_LIGHT cannot be combined with the two-kernel form of PT_SORT_MATERIAL, which this "
                                "session would take (its intersection planes do not carry the winning primitive)",
            pt.PT_TEXTURES: "pt_init: PT_TEXTURES cannot be combined with the two-kernel form of PT_SORT_MATERIAL, which this "
                            "session would take (its intersection planes do not carry the winning primitive)",
            pt.PT_SMOOTH_NORMALS: "pt_init: PT_SMOOTH_NORMALS cannot be combined with the two-kernel form of PT_SORT_MATERIAL, which this "
                                  "session would take (its intersection planes carry one normal and no triangle)",
        }
        for flag, text in refused.items():
            session(pt, sc.BY_ID["f64"], frame, flags=sort | flag)          # 64 materials: the fused form carries the primitive
            pt.pathtraceFree()
            with pytest.raises(pt.PtError):
                session(pt, sc.BY_ID["g65"], frame, flags=sort | flag)
            assert L.pt_last_error().decode() == text
    finally:
        pt.pathtraceFree()


@pytest.mark.parametrize("name", ["w63 workgroup-wide", "f63 workgroup-wide", "g65 one workgroup per CU"])
def test_experiment_forms(pt, po, monkeypatch, name):
    """A -DPT_EXPERIMENTS build only: w63 and f63 with PTMI355_SORT_WAVE=0 (f63 with PTMI355_SORT_FUSED=0 beside it, so that its
    flags reach the two-kernel form at all) run k_shade_sorted with 64 bins, its materials in LDS, bounce by bounce; g65 with
    PTMI355_SORT_WGS=1 has one workgroup per CU, so a batch of 44 iterations gives them several chunks each."""
    if not pt.has_experiments():
        pytest.skip("PTMI355_SORT_WAVE / PTMI355_SORT_FUSED / PTMI355_SORT_WGS are read by -DPT_EXPERIMENTS builds only")
    case = sc.BY_ID[name.split()[0]]
    env = {"w63": {"PTMI355_SORT_WAVE": "0"}, "f63": {"PTMI355_SORT_WAVE": "0", "PTMI355_SORT_FUSED": "0"}, "g65": {"PTMI355_SORT_WGS": "1"}}[case.id]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if case.id == "g65":
        import torch
        long_batch(pt, po, torch.cuda.get_device_properties(0).multi_processor_count)
        return
    frame = sc.FRAME
    ref = sc.reference(po, pt, case, frame)
    n = frame[0] * frame[1]
    session(pt, case, frame)
    try:
        pt.set_profiling(True)
        for it in (1, 2):
            snaps = ref.snaps[it]
            pt.trace_begin(it, 1)
            for d in range(DEPTH):
                n_live = pt.trace_bounce(d)
                paths, live = pt.export_paths(n)
                want_n = snaps[d]["n_live"] if d < len(snaps) else 0
                assert n_live == live == want_n, at(case, frame, it, d)
                if want_n:
                    check_order(po, pt, case, frame, ref, it, d, paths["pixelIndex"], snaps[d]["paths"]["pixelIndex"][:want_n])
                    assert_paths_equal(paths, snaps[d]["paths"], want_n)
            pt.trace_end()
            check_image(case, frame, "stepped iteration %d" % it, pt.get_image(n), ref.images[it])
        assert pt.get_profile()["sort"][1] == 2 * DEPTH, "%s: the two-kernel form did not run" % at(case, frame)
    finally:
        pt.pathtraceFree()
