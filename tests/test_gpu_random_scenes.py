"""GPU parity on random hostile scenes (tests/random_scenes.py: the fuzz tool's generator -- arbitrary rotations, slabs of 0.001,
scales of 100 and 1e-4, zero scales, enclosing shells, an eye inside primitives, up to 39 primitives, depths 1 to 11) for every
shading feature and the filters, which the other modules hold against their models on Cornell-shaped scenes only: the first-hit
table and k_bounce<MODE_FIRST2>, the own-surface early miss and the cube face table, environment maps, PT_GLOSSY, PT_DIRECT_LIGHT,
PT_TEXTURES with bump maps, the G-buffer, pt_albedo, the A-trous filter and its reprojected history.

Every session is the tool's call sequence -- pt_trace_batch(1, 2), one pathtrace(), five batches on the lanes, pt_get_image --
at 40 x 26 (16 full waves and a 16-lane tail; several tiles of the fused kernels), the first seed of a list also at 130 x 9, under
both launch plans; running sums are compared byte for byte with the numpy models (computed here, once per seed; no golden files),
live and ray counters wherever the model counts them.  A test item is one group of four seeds under one session.
The first-state table (k_bounce<MODE_STATE2>) has a list of its own, rs.STATE_SEEDS: scenes without a
refractive material, which also run at 64 x 16 -- whole 64-pixel tiles, so the ended-tile words are read -- and every such session
asks ptdbg_first_state whether each launch of bounces 0 and 1 was the table form.
Three more lists run what the lists above never carried: rs.SMOOTH_SEEDS puts vertex normals on the mesh session's soup
(PT_SMOOTH_NORMALS: normals that lean, face away, vanish, are NaN or infinite, and go and come back in mid-session); rs.SKY_SEEDS
samples the sky as a light (PT_DIRECT_SKY: maps of 1 to 16 texels, with the lamps and without, a map that leaves and another that
arrives, so that nlights changes under the session); rs.CAMERA_SEEDS runs every kind of session under PT_AA_JITTER and the thin
lens -- the GEN forms of every shader, k_raygen through the stepping interface, and pt_set_lens switching between a lens and the
pinhole while ptdbg_first_two and ptdbg_first_state say whether the tables of repeating camera rays were used --, PT_MOMENTS included.
tests/test_random_scenes_cpu.py shows from the models alone that the seed lists reach the branches named above.

A failure names the seed, the session, the number of differing pixels, the first of them with both values, and the bounce at which
that pixel's path ended in the model (per iteration): enough to go straight to the stepping interface."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import __graft_entry__ as ge  # noqa: E402,F401
import random_scenes as rs  # noqa: E402
from gpu_common import pt, launch_plan, bits  # noqa: E402,F401

pytestmark = pytest.mark.gpu

W, H = rs.W, rs.H
F32 = np.float32


def first_two(pt):
    """launches that did bounces 0 and 1 since pathtraceInit"""
    out = (C.c_ulonglong * 1)()
    assert pt.library().ptdbg_first_two(out) == 0
    return int(out[0])


def frames(seeds, group):
    """(seed, w, h) of a group: every seed at 40 x 26, the list's first seed also at 130 x 9."""
    out = [(s, W, H) for s in group]
    if seeds[0] in group:
        out.append((seeds[0],) + rs.WIDE)
    return out


class Report:
    """Collects what differs in one test item, so that one run shows every seed of the group."""

    def __init__(self, session, plan):
        self.session, self.plan, self.lines = session, plan, []

    def image(self, seed, w, what, got, want, run=None, its=()):
        bad = (bits(got) != bits(want)).any(axis=1)
        if not bad.any():
            return True
        p = int(np.nonzero(bad)[0][0])
        ends = ", ".join("%d: %d" % (it, run.ended[it][p]) for it in its) if run is not None else "-"
        self.lines.append("seed %d, %s [%s], %s: %d of %d pixels differ; first pixel %d (x %d, y %d): got %r, want %r; its path ended at "
                          "bounce (iteration: bounce) %s" % (seed, self.session, self.plan, what, int(bad.sum()), len(bad), p, p % w, p // w,
                                                             got[p].tolist(), want[p].tolist(), ends))
        return False

    def equal(self, seed, what, got, want):
        if got != want:
            self.lines.append("seed %d, %s [%s], %s: got %r, want %r" % (seed, self.session, self.plan, what, got, want))

    def paths(self, seed, w, what, got, want):
        """The live paths of two pools, each ordered by its pixelIndex: every field, bit for bit."""
        got, want = (p[p["remainingBounces"] > 0] for p in (got, want))
        got, want = (p[np.argsort(p["pixelIndex"], kind="stable")] for p in (got, want))
        if len(got) != len(want) or (got["pixelIndex"] != want["pixelIndex"]).any():
            self.lines.append("seed %d, %s [%s], %s: %d live paths, want %d; pixels that are live on one side only: %s" %
                              (seed, self.session, self.plan, what, len(got), len(want),
                               sorted(set(got["pixelIndex"].tolist()) ^ set(want["pixelIndex"].tolist()))[:8]))
            return
        bad = got["remainingBounces"] != want["remainingBounces"]
        for f in ("origin", "direction", "color"):
            bad |= (bits(got[f]) != bits(want[f])).any(axis=1)
        if bad.any():
            k = int(np.nonzero(bad)[0][0])
            p = int(got["pixelIndex"][k])
            self.lines.append("seed %d, %s [%s], %s: %d of %d paths differ; first pixel %d (x %d, y %d): got %r, want %r" %
                              (seed, self.session, self.plan, what, int(bad.sum()), len(bad), p, p % w, p // w, got[k].tolist(), want[k].tolist()))

    def done(self):
        assert not self.lines, "\n".join(self.lines)


def trace_sequence(pt, rep, seed, w, h, run, depth, counters=True, rays=None, last=9, what=""):
    """The tool's calls against a model's run: a batch of two with the host image, pathtrace() per call, batches nobody waits for on
    the lanes, the device image.  counters: pt_get_stats' live and ray counts after the two synchronous calls."""
    n = w * h
    img = np.zeros((n, 3), dtype=F32)
    pt.trace_batch(1, 2, img)
    rep.image(seed, w, what + "batch of 2", img, run.images[2], run, (1, 2))
    if counters:
        gs = pt.get_stats()
        live = run.live_sum((1, 2), depth)
        rep.equal(seed, what + "live counts of the batch", list(gs.live[:depth]), live)
        rep.equal(seed, what + "rays of the batch", int(gs.rays), sum(live) if rays is None else rays[1] + rays[2])
    got = pt.pathtrace(None, 0, 3)
    rep.image(seed, w, what + "pathtrace(3)", got, run.images[3], run, (3,))
    if counters:
        gs = pt.get_stats()
        rep.equal(seed, what + "live counts of iteration 3", list(gs.live[:depth]), run.live_sum((3,), depth))
    if last == 3:
        return
    for it0, count in rs.BATCHES:
        if it0 + count - 1 <= last:
            pt.trace_batch_async(it0, count)
    pt.synchronize()
    rep.image(seed, w, what + "after the lanes", pt.get_image(n), run.images[last], run, range(4, last + 1))


# ---- plain sessions against the oracle ---------------------------------------------------------------------------------------------
PLAIN = {"compact": lambda pt, po: (pt.PT_COMPACT, po.F_COMPACT), "non-compacting": lambda pt, po: (0, 0),
         "sorted": lambda pt, po: (pt.PT_COMPACT | pt.PT_SORT_MATERIAL, po.F_COMPACT | po.F_SORT)}


@pytest.mark.parametrize("group", rs.groups(rs.PLAIN_SEEDS))
@pytest.mark.parametrize("pipeline", list(PLAIN))
def test_plain_sessions(pt, po, launch_plan, pipeline, group):
    """PT_COMPACT, 0 and PT_COMPACT | PT_SORT_MATERIAL against po.Tracer.  The compacting session says whether its batches began
    with the fused bounce 0 + 1 (ptdbg_first_two) wherever the rule of DESIGN.md section 6.23 takes it -- a kernel per bounce,
    depth 2 or more --, and runs again under the NEXT seed's perturbed camera: the first-hit table is refilled and reused."""
    rep = Report("plain " + pipeline, launch_plan)
    for seed, w, h in frames(rs.PLAIN_SEEDS, group):
        geoms, mats, cam, depth = rs.scene(pt, seed, w, h)
        flags, oflags = PLAIN[pipeline](pt, po)
        scene = pt.Scene(geoms, mats, cam, depth)
        pt.pathtraceInit(scene, flags=flags, max_batch=2)
        try:
            run = rs.plain_run(po, pt, seed, w, h, oflags)
            trace_sequence(pt, rep, seed, w, h, run, depth, counters=pipeline != "non-compacting", rays=run.rays)
            if pipeline == "compact":
                fused = launch_plan == "one launch per bounce" and depth >= 2
                if fused:
                    rep.equal(seed, "fused bounce 0 + 1 launches > 0", first_two(pt) > 0, True)
                before = first_two(pt)
                cam2 = rs.scene(pt, rs.next_seed(rs.PLAIN_SEEDS, seed), w, h)[2]
                scene.camera = cam2
                pt.set_camera(cam2, depth)
                pt.clear_image()
                run2 = rs.plain_run(po, pt, seed, w, h, oflags, cam=cam2)
                trace_sequence(pt, rep, seed, w, h, run2, depth, rays=run2.rays, what="camera of seed %d: " % rs.next_seed(rs.PLAIN_SEEDS, seed))
                if fused:
                    rep.equal(seed, "fused launches under the second camera > 0", first_two(pt) > before, True)
        finally:
            pt.pathtraceFree()
    rep.done()


# ---- the first-state table on glass-free scenes ----------------------------------------------------------
def first_state(pt):
    """launches whose bounce 0 came from the first-state table since pathtraceInit"""
    out = (C.c_ulonglong * 1)()
    assert pt.library().ptdbg_first_state(out) == 0
    return int(out[0])


def state_frames(seeds, group):
    """(seed, w, h) of a group: every seed at 64 x 16 (whole tiles: the ended-tile words exist) and at 40 x 26 (they do not), the
    list's first seed also at 130 x 9."""
    out = [(s,) + rs.STATE_FRAME for s in group] + [(s, W, H) for s in group]
    if seeds[0] in group:
        out.append((seeds[0],) + rs.WIDE)
    return out


def state_counters(pt, rep, seed, what, launch_plan, depth, before=0):
    """Every launch of bounces 0 and 1 of these sessions is the table form; a kernel per bounce at depth 2 or more makes some."""
    two, state = first_two(pt), first_state(pt)
    rep.equal(seed, what + "launches from the first-state table == launches of bounces 0 and 1", state, two)
    if depth == 1:
        rep.equal(seed, what + "launches of bounces 0 and 1 at depth 1", two, 0)
    elif launch_plan == "one launch per bounce":
        rep.equal(seed, what + "launches from the first-state table rose above %d" % before, state > before, True)
    return state


STATE_CASES = [(g, "1") for g in rs.groups(rs.STATE_SEEDS)] + [(rs.groups(rs.STATE_SEEDS)[0], "0")]


@pytest.mark.parametrize("group, scene_lds", STATE_CASES)
def test_first_state_sessions(pt, po, launch_plan, monkeypatch, group, scene_lds):
    """PT_COMPACT on the scenes without a refractive material against po.Tracer, the call sequence of test_plain_sessions under the
    seed's camera and under the NEXT seed's: bounce 0 of every launch of the two comes from the per-pixel table
    (k_bounce<MODE_STATE2>), whose records here are of all four kinds in odd mixtures -- an eye inside an emitter, frames that
    mostly miss, mirror hits from inside, slabs of 0.001 -- and whose ended-tile words are read at 64 x 16.  The first group runs
    once more with the scene gathered from global memory (PTMI355_SCENE_LDS=0: the two other instantiations)."""
    if scene_lds == "0":
        monkeypatch.setenv("PTMI355_SCENE_LDS", "0")
    rep = Report("first state" + (", scene not in LDS" if scene_lds == "0" else ""), launch_plan)
    for seed, w, h in state_frames(rs.STATE_SEEDS, group):
        geoms, mats, cam, depth = rs.scene(pt, seed, w, h)
        scene = pt.Scene(geoms, mats, cam, depth)
        pt.pathtraceInit(scene, flags=pt.PT_COMPACT, max_batch=2)
        try:
            at = "%d x %d: " % (w, h)
            run = rs.plain_run(po, pt, seed, w, h, po.F_COMPACT)
            trace_sequence(pt, rep, seed, w, h, run, depth, rays=run.rays, what=at)
            before = state_counters(pt, rep, seed, at, launch_plan, depth)
            other = rs.next_seed(rs.STATE_SEEDS, seed)
            cam2 = rs.scene(pt, other, w, h)[2]
            scene.camera = cam2
            pt.set_camera(cam2, depth)
            pt.clear_image()
            run2 = rs.plain_run(po, pt, seed, w, h, po.F_COMPACT, cam=cam2)
            at += "camera of seed %d: " % other
            trace_sequence(pt, rep, seed, w, h, run2, depth, rays=run2.rays, what=at)
            state_counters(pt, rep, seed, at, launch_plan, depth, before)
        finally:
            pt.pathtraceFree()
    rep.done()


@pytest.mark.parametrize("seed", [rs.STATE_SEEDS[0], rs.STATE_SEEDS[2]])
def test_first_state_tile_of_a_frame(pt, po, launch_plan, seed):
    """The list's first seed (no pixel ends with 0) and its third (whole-ended tiles beside mixed ones) at 64 x 16 as tile 1 of 2 in
    strips of 4 rows: 512 local pixels, so the words exist, and records and words are indexed by the tile's local pixel.  Compared
    over the tile's own pixels."""
    w, h = rs.STATE_FRAME
    rep = Report("first state, tile 1 of 2", launch_plan)
    geoms, mats, cam, depth = rs.scene(pt, seed, w, h)
    own = pt.sharding.tile_pixel_indices(1, 2, 4, w, h)
    assert len(own) == 512
    run = rs.plain_run(po, pt, seed, w, h, po.F_COMPACT)
    pt.pathtraceInit(pt.Scene(geoms, mats, cam, depth), flags=pt.PT_COMPACT, max_batch=2, tile=(1, 2, 4))
    try:
        img = np.zeros((w * h, 3), dtype=F32)
        for iter0 in (1, 3, 5):
            pt.trace_batch(iter0, 2, img)
            rep.equal(seed, "paths of the batch at %d" % iter0, int(pt.get_stats().live[0]), 2 * len(own))
            bad = (bits(img[own]) != bits(run.images[iter0 + 1][own])).any(axis=1)
            if bad.any():
                p = int(own[np.nonzero(bad)[0][0]])
                rep.lines.append("seed %d, %s [%s], batch at %d: %d of %d pixels differ; first pixel %d (x %d, y %d): got %r, want %r; its "
                                 "path ended at bounce %d" % (seed, rep.session, rep.plan, iter0, int(bad.sum()), len(own), p, p % w, p // w,
                                                              img[p].tolist(), run.images[iter0 + 1][p].tolist(), run.ended[iter0 + 1][p]))
        two, state = first_two(pt), first_state(pt)
        rep.equal(seed, "launches from the first-state table == launches of bounces 0 and 1", state, two)
        if launch_plan == "one launch per bounce":
            rep.equal(seed, "launches from the first-state table", state, 3 if depth >= 2 else 0)
    finally:
        pt.pathtraceFree()
    rep.done()


@pytest.mark.parametrize("group", rs.groups(rs.STATE_DIRECT_SEEDS))
def test_first_state_direct_sessions(pt, po, launch_plan, group):
    """PT_COMPACT | PT_DIRECT_LIGHT without PT_GLOSSY and without a sky, at depth 3 or more, against direct_model.Model: bounces 0
    and 1 are plain ones, so the launch of the two reads the table; D + 1 bounces counted."""
    rep = Report("first state + direct", launch_plan)
    for seed, w, h in state_frames(rs.STATE_DIRECT_SEEDS, group):
        geoms, mats, cam, depth = rs.scene(pt, seed, w, h)
        run, _, elements = rs.plain_direct_run(po, pt, seed, w, h)
        assert depth >= rs.STATE_DIRECT_MIN_DEPTH and 0 < elements <= 1024, seed     # (tests/test_random_scenes_cpu.py asserts it)
        pt.pathtraceInit(pt.Scene(geoms, mats, cam, depth), flags=pt.PT_COMPACT | pt.PT_DIRECT_LIGHT, max_batch=2)
        try:
            at = "%d x %d: " % (w, h)
            trace_sequence(pt, rep, seed, w, h, run, depth + 1, what=at)
            state_counters(pt, rep, seed, at, launch_plan, depth)
        finally:
            pt.pathtraceFree()
    rep.done()


# ---- sky + glossy -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", rs.groups(rs.GLOSSY_SEEDS))
def test_sky_and_glossy_sessions(pt, po, launch_plan, group):
    """PT_COMPACT | PT_GLOSSY with the seed's sky (or none) against glossy_model.Model: the GGX lobe at grazing hits, inside shells."""
    rep = Report("sky + glossy", launch_plan)
    for seed, w, h in frames(rs.GLOSSY_SEEDS, group):
        geoms, mats, cam, depth = rs.scene(pt, seed, w, h)
        run, _, f = rs.glossy_run(po, pt, seed, w, h)
        pt.pathtraceInit(pt.Scene(geoms, f.materials, cam, depth), flags=pt.PT_COMPACT | pt.PT_GLOSSY, max_batch=2)
        try:
            if f.sky is not None:
                pt.set_environment(f.sky)
            trace_sequence(pt, rep, seed, w, h, run, depth)
        finally:
            pt.pathtraceFree()
    rep.done()


# ---- textures + bumps + sky + glossy -----------------------------------------------------------------------------------------------
def textured_session(pt, rep, seed, w, h, run, f, geoms, cam, depth, flags, counters, tris=None, meshes=None):
    scene = pt.Scene(geoms, f.materials, cam, depth, triangles=tris, meshes=meshes) if tris is not None else pt.Scene(geoms, f.materials, cam, depth)
    pt.pathtraceInit(scene, flags=flags | pt.PT_TEXTURES | pt.PT_GLOSSY, max_batch=2)
    try:
        for k, t in f.bump_maps.items():
            pt.set_bump_map(k, t)
        for k, t in f.textures.items():
            pt.set_texture(k, t)
        if f.sky is not None:
            pt.set_environment(f.sky)
        trace_sequence(pt, rep, seed, w, h, run, depth, counters=counters, last=3)
        b, t = rs.dropped(f)
        if b is not None:
            pt.set_bump_map(b, None)
        if t is not None:
            pt.set_texture(t, None)
        for it in (4, 5):
            pt.trace_batch_async(it, 1)
        pt.synchronize()
        rep.image(seed, w, "after a bump map and a texture were removed", pt.get_image(w * h), run.images[5], run, (4, 5))
    finally:
        pt.pathtraceFree()


TEXTURED = {"compact": lambda pt: pt.PT_COMPACT, "non-compacting": lambda pt: 0, "sorted": lambda pt: pt.PT_COMPACT | pt.PT_SORT_MATERIAL}


@pytest.mark.parametrize("group", rs.groups(rs.TEXTURED_SEEDS))
@pytest.mark.parametrize("pipeline", list(TEXTURED))
def test_textured_and_bumped_sessions(pt, po, launch_plan, pipeline, group):
    """PT_TEXTURES | PT_GLOSSY with the seed's checker textures, bump maps (studs and noise, 1 to 8 texels a side, slopes up to 3),
    sky and exponents against bump_model.Model: texel lookups on 100 : 1 primitives, the guard on slivers.  After iteration 3 one
    bump map and one texture are removed; two more iterations follow on the lanes."""
    rep = Report("textures + bumps " + pipeline, launch_plan)
    for seed, w, h in frames(rs.TEXTURED_SEEDS, group):
        geoms, mats, cam, depth = rs.scene(pt, seed, w, h)
        run, _, f = rs.textured_run(po, pt, seed, w, h)
        textured_session(pt, rep, seed, w, h, run, f, geoms, cam, depth, TEXTURED[pipeline](pt), pipeline != "non-compacting")
    rep.done()


# ---- direct + sky + glossy ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", rs.groups(rs.DIRECT_SEEDS))
def test_direct_light_sessions(pt, po, launch_plan, group):
    """PT_COMPACT | PT_DIRECT_LIGHT | PT_GLOSSY against direct_model.Model: points inside an emitting sphere, degenerate elements
    (zero-area ones are not in the table), D + 1 bounces counted."""
    rep = Report("direct + sky + glossy", launch_plan)
    for seed, w, h in frames(rs.DIRECT_SEEDS, group):
        geoms, mats, cam, depth = rs.scene(pt, seed, w, h)
        elements = rs.light_table_size(po, pt, seed, w, h)
        if elements == 0 or elements > 1024:                         # (decided from the model; no seed of the list is such a one:
            pytest.skip("seed %d: %d light elements" % (seed, elements))     # tests/test_random_scenes_cpu.py asserts it)
        run, _, f, _ = rs.direct_run(po, pt, seed, w, h)
        pt.pathtraceInit(pt.Scene(geoms, f.materials, cam, f.direct_depth), flags=pt.PT_COMPACT | pt.PT_DIRECT_LIGHT | pt.PT_GLOSSY, max_batch=2)
        try:
            if f.sky is not None:
                pt.set_environment(f.sky)
            trace_sequence(pt, rep, seed, w, h, run, f.direct_depth + 1)
        finally:
            pt.pathtraceFree()
    rep.done()


# ---- with a mesh -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hierarchy", [False, True])
@pytest.mark.parametrize("session", ["plain", "textured"])
def test_sessions_with_a_mesh(pt, po, launch_plan, session, hierarchy):
    """A soup of 300 triangles beside the random primitives, through the loop over every triangle and through PT_MESH_BVH; in the
    textured session the mesh's material may carry a texture and a bump map, which hits on the mesh ignore."""
    rep = Report("mesh, %s, %s" % (session, "hierarchy" if hierarchy else "loop"), launch_plan)
    extra = pt.PT_MESH_BVH if hierarchy else 0
    for seed in rs.MESH_SEEDS:
        geoms, mats, cam, depth = rs.scene(pt, seed, W, H)
        geoms, tris, meshes = rs.mesh_of(pt, seed, geoms, len(mats))
        if session == "plain":
            run = rs.plain_run(po, pt, seed, W, H, po.F_COMPACT, mesh=True)
            pt.pathtraceInit(pt.Scene(geoms, mats, cam, depth, triangles=tris, meshes=meshes), flags=pt.PT_COMPACT | extra, max_batch=2)
            try:
                trace_sequence(pt, rep, seed, W, H, run, depth, rays=run.rays)
            finally:
                pt.pathtraceFree()
        else:
            run, _, f = rs.textured_run(po, pt, seed, W, H, mesh=True)
            textured_session(pt, rep, seed, W, H, run, f, geoms, cam, depth, pt.PT_COMPACT | extra, True, tris, meshes)
    rep.done()


# ---- smooth normals, the sampled sky, jitter and the lens --------------------------------------------------------------------------
def init_session(pt, scene, flags, run, **kw):
    """pt_init for a model's run: PT_AA_JITTER where its camera jitters, lens= where it has a lens (rs.CameraPlan)."""
    plan = run.plan
    pt.pathtraceInit(scene, flags=flags | (pt.PT_AA_JITTER if plan.aa else 0), max_batch=2, lens=plan.kw()["lens"], **kw)


def on_the_lanes(pt, batches):
    for it0, count in batches:
        pt.trace_batch_async(it0, count)
    pt.synchronize()


def table_counters(pt):
    return first_two(pt), first_state(pt)


def camera_tail(pt, rep, seed, w, h, run, stepped, tables=None):
    """What follows a camera session's own sequence (rs.CameraPlan).  Iteration last + 1: through pt_trace_begin / pt_trace_bounce /
    pt_trace_end where `stepped` -- k_raygen generates the rays there, not a bounce kernel's GEN form -- with pt_export_paths after
    bounce 0 against the model's live paths; through pt_trace elsewhere.  A session with a lens and no jitter then calls
    pt_set_lens(0, 0), runs two iterations that the pinhole model continues on the same running sum, sets its lens again and runs two
    more.  tables = (depth, glass_free, launch plan) in the plain compacting session: with a kernel per bounce and depth >= 2 the
    pinhole stretch must take bounces 0 and 1 from the first-hit table (and from the first-state table where no material refracts),
    and no stretch under the lens may."""
    plan, n = run.plan, w * h
    it = plan.step
    if stepped:
        pt.trace_begin(it, 1)
        for d in range(len(run.live[it])):
            pt.trace_bounce(d)
            if d == 0:
                rep.paths(seed, w, "pt_export_paths after the stepped bounce 0 of iteration %d" % it, pt.export_paths(n)[0], run.stepped)
        pt.trace_end()
        rep.image(seed, w, "after the stepped iteration %d" % it, pt.get_image(n), run.images[it], run, (it,))
    else:
        rep.image(seed, w, "pathtrace(%d)" % it, pt.pathtrace(None, 0, it), run.images[it], run, (it,))
    if not plan.switch:
        return
    fused = tables is not None and tables[2] == "one launch per bounce" and tables[0] >= 2
    img = np.zeros((n, 3), dtype=F32)
    c0 = table_counters(pt)
    pt.set_lens(0.0, 0.0)
    pt.trace_batch(it + 1, 2, img)
    rep.image(seed, w, "two iterations after pt_set_lens(0, 0)", img, run.images[it + 2], run, (it + 1, it + 2))
    c1 = table_counters(pt)
    pt.set_lens(*plan.lens)
    pt.trace_batch(it + 3, 2, img)
    rep.image(seed, w, "two iterations after pt_set_lens%r" % (plan.lens,), img, run.images[it + 4], run, (it + 3, it + 4))
    c2 = table_counters(pt)
    if tables is not None:
        rep.equal(seed, "launches of bounces 0 and 1 from the tables under the lens (before, after the pinhole stretch)", (c0, c2), ((0, 0), c1))
        if fused:
            rep.equal(seed, "launches from the first-hit table rose in the pinhole stretch", c1[0] > 0, True)
            rep.equal(seed, "launches from the first-state table in the pinhole stretch", c1[1], c1[0] if tables[1] else 0)


def smooth_session(pt, po, rep, seed, w, h, flags, counters=True, camera=False, stepped=False, extras=False):
    """PT_SMOOTH_NORMALS | PT_GLOSSY on the soup with rs.normals_of and the seed's sky against smooth_model.Model: iterations 1-3,
    the normals removed, 4-5 on the lanes, the normals set again, 6-7 on the lanes.  extras: pt_get_vertex_normals returns the bytes
    that were set (NaN payloads included), and pt_gbuffer and pt_albedo are those of the same session without normals."""
    run, _, s = rs.smooth_run(po, pt, seed, w, h, camera=camera)
    scene = pt.Scene(s.geoms, s.materials, s.cam, s.depth, triangles=s.tris, meshes=s.meshes)
    planes = []
    for normals in ((True, False) if extras else (True,)):
        init_session(pt, scene, flags | pt.PT_SMOOTH_NORMALS | pt.PT_GLOSSY, run)
        try:
            if s.sky is not None:
                pt.set_environment(s.sky)
            if normals:
                pt.set_vertex_normals(s.normals)
                trace_sequence(pt, rep, seed, w, h, run, s.depth, counters=counters, last=3)
                pt.set_vertex_normals(None)
                on_the_lanes(pt, ((4, 1), (5, 1)))
                rep.image(seed, w, "after the normals were removed", pt.get_image(w * h), run.images[5], run, (4, 5))
                pt.set_vertex_normals(s.normals)
                on_the_lanes(pt, ((6, 2),))
                rep.image(seed, w, "after the normals were set again", pt.get_image(w * h), run.images[7], run, (6, 7))
                if camera:
                    camera_tail(pt, rep, seed, w, h, run, stepped)
            else:
                pt.pathtrace(None, 0, 1)
            if extras:
                got = pt.get_vertex_normals()
                if normals:
                    rep.equal(seed, "pt_get_vertex_normals returns the bytes that were set", got is not None and got.tobytes() == s.normals.tobytes(), True)
                else:
                    rep.equal(seed, "pt_get_vertex_normals without normals is None", got is None, True)
                g = pt.gbuffer()
                planes.append([(k, g[k]) for k in sorted(g)] + [("albedo", pt.albedo())])
        finally:
            pt.pathtraceFree()
    if extras:
        for (k, got), (_, want) in zip(*planes):
            planes_equal(rep, seed, w, "with normals and without: " + k, got.reshape(w * h, -1), want.reshape(w * h, -1))


SMOOTH = {"loop": lambda pt: pt.PT_COMPACT, "hierarchy": lambda pt: pt.PT_COMPACT | pt.PT_MESH_BVH}


@pytest.mark.parametrize("group", rs.groups(rs.SMOOTH_SEEDS))
@pytest.mark.parametrize("mesh", list(SMOOTH))
def test_smooth_sessions(pt, po, launch_plan, mesh, group):
    """The SH_SMOOTH forms on the hostile soup: slivers and metre-sized triangles under normals that lean, face away, vanish, are NaN,
    infinite, 1e-20 and 1e20 long; mirror and glass hits about smoothed normals with the guard behind them; normals that go and
    come back between batches on the lanes.  The first group also runs non-compacting and through the fused sort."""
    rep = Report("smooth, " + mesh, launch_plan)
    for seed, w, h in frames(rs.SMOOTH_SEEDS, group):
        smooth_session(pt, po, rep, seed, w, h, SMOOTH[mesh](pt), extras=True)
        if rs.SMOOTH_SEEDS[0] in group and (w, h) == (W, H):
            extra = pt.PT_MESH_BVH if mesh == "hierarchy" else 0
            rep.session = "smooth, %s, non-compacting" % mesh
            smooth_session(pt, po, rep, seed, w, h, extra, counters=False)
            if mesh == "loop":                                           # (with the hierarchy the sort takes its two-kernel form: refused)
                rep.session = "smooth, loop, sorted"
                smooth_session(pt, po, rep, seed, w, h, pt.PT_COMPACT | pt.PT_SORT_MATERIAL)
            rep.session = "smooth, " + mesh
    rep.done()


def sampled_sky_session(pt, po, rep, seed, w, h, camera=False, stepped=False):
    """PT_COMPACT | PT_DIRECT_LIGHT | PT_DIRECT_SKY | PT_GLOSSY against sky_model.Model on rs.sky_session(): iterations 1-3 under
    the seed's map, 4-5 without a map -- nlights falls back to the lamps', to 0 where the lamps are off: then no bounce D is traced
    --, 6-7 on the lanes under the next seed's map.  D + 1 live counts wherever a call is waited for."""
    run, _, s, _ = rs.sky_run(po, pt, seed, w, h, camera=camera)
    init_session(pt, pt.Scene(s.geoms, s.materials, s.cam, s.depth), pt.PT_COMPACT | pt.PT_DIRECT_LIGHT | pt.PT_DIRECT_SKY | pt.PT_GLOSSY, run)
    try:
        pt.set_environment(s.texels)
        trace_sequence(pt, rep, seed, w, h, run, s.depth + 1, last=3)
        pt.set_environment(None)
        img = np.zeros((w * h, 3), dtype=F32)
        pt.trace_batch(4, 2, img)
        rep.image(seed, w, "after the map was removed", img, run.images[5], run, (4, 5))
        live = (run.live_sum((4, 5), s.depth + 1) + [0])[:s.depth + 1]
        rep.equal(seed, "live counts without a map", list(pt.get_stats().live[:s.depth + 1]), live)
        if s.lamps_off:
            rep.equal(seed, "final rays without a map and without lamps", live[s.depth], 0)
        pt.set_environment(s.other)
        on_the_lanes(pt, ((6, 1), (7, 1)))
        rep.image(seed, w, "under the map of seed %d" % (seed + 1), pt.get_image(w * h), run.images[7], run, (6, 7))
        if camera:
            camera_tail(pt, rep, seed, w, h, run, stepped)
    finally:
        pt.pathtraceFree()


@pytest.mark.parametrize("group", rs.groups(rs.SKY_SEEDS))
def test_sampled_sky_sessions(pt, po, launch_plan, group):
    """The sky as a light on the random scenes: maps of 1, 4 and 16 texels a side, with the lamps and as the only light, final rays
    that leave through gaps between primitives and final rays that do not, a map that goes and another that arrives."""
    rep = Report("sampled sky", launch_plan)
    for seed, w, h in frames(rs.SKY_SEEDS, group):
        sampled_sky_session(pt, po, rep, seed, w, h)
    rep.done()


def camera_session(pt, po, rep, kind, seed, w, h, stepped, launch_plan):
    """One of rs.CAMERA_KINDS under the seed's rs.camera_features(): the session's own sequence, then camera_tail."""
    if kind.startswith("smooth"):
        return smooth_session(pt, po, rep, seed, w, h, SMOOTH[kind.split()[1]](pt), camera=True, stepped=stepped)
    if kind == "sampled sky":
        return sampled_sky_session(pt, po, rep, seed, w, h, camera=True, stepped=stepped)
    geoms, mats, cam, depth = rs.scene(pt, seed, w, h)
    run = rs.camera_run(po, pt, kind, seed, w, h)
    if kind.startswith("plain") or kind == "moments":
        flags = PLAIN[kind[6:]](pt, po)[0] if kind != "moments" else pt.PT_COMPACT | pt.PT_MOMENTS
        init_session(pt, pt.Scene(geoms, mats, cam, depth), flags, run, **(dict(pin_image=False) if kind == "moments" else {}))
        try:
            trace_sequence(pt, rep, seed, w, h, run, depth, counters=kind != "plain non-compacting", rays=run.rays)
            if kind == "moments":
                for name, got, want in zip(("M1", "M2"), pt.get_moments(), run.moments[run.plan.last]):
                    planes_equal(rep, seed, w, name + " after iteration %d" % run.plan.last, got.reshape(-1, 1), want.reshape(-1, 1))
            glass_free = not (mats["hasRefractive"] > 0).any()
            camera_tail(pt, rep, seed, w, h, run, stepped, (depth, glass_free, launch_plan) if kind == "plain compact" else None)
            if kind == "moments":
                for name, got, want in zip(("M1", "M2"), pt.get_moments(), run.moments[run.plan.end]):
                    planes_equal(rep, seed, w, name + " after iteration %d" % run.plan.end, got.reshape(-1, 1), want.reshape(-1, 1))
        finally:
            pt.pathtraceFree()
        return
    f = rs.features(seed, mats, depth)
    if kind == "textures + bumps":
        scene, flags, last = pt.Scene(geoms, f.materials, cam, depth), pt.PT_COMPACT | pt.PT_TEXTURES | pt.PT_GLOSSY, 3
    elif kind == "sky + glossy":
        scene, flags, last = pt.Scene(geoms, f.materials, cam, depth), pt.PT_COMPACT | pt.PT_GLOSSY, 9
    else:
        assert kind == "direct + sky + glossy"
        depth = f.direct_depth
        scene, flags, last = pt.Scene(geoms, f.materials, cam, depth), pt.PT_COMPACT | pt.PT_DIRECT_LIGHT | pt.PT_GLOSSY, 9
    init_session(pt, scene, flags, run)
    try:
        if kind == "textures + bumps":
            for k, t in f.bump_maps.items():
                pt.set_bump_map(k, t)
            for k, t in f.textures.items():
                pt.set_texture(k, t)
        if f.sky is not None:
            pt.set_environment(f.sky)
        trace_sequence(pt, rep, seed, w, h, run, len(run.live[1]), last=last)
        if kind == "textures + bumps":
            b, t = rs.dropped(f)
            if b is not None:
                pt.set_bump_map(b, None)
            if t is not None:
                pt.set_texture(t, None)
            on_the_lanes(pt, ((4, 1), (5, 1)))
            rep.image(seed, w, "after a bump map and a texture were removed", pt.get_image(w * h), run.images[5], run, (4, 5))
        camera_tail(pt, rep, seed, w, h, run, stepped)
    finally:
        pt.pathtraceFree()


@pytest.mark.parametrize("group", rs.groups(rs.CAMERA_SEEDS))
@pytest.mark.parametrize("kind", rs.CAMERA_KINDS)
def test_camera_sessions(pt, po, launch_plan, kind, group):
    """PT_AA_JITTER and the thin lens under every shading feature: the GEN forms of SH_DIRECT, SH_TEX and SH_SMOOTH, a depth-1 direct
    session whose bounce 0 is a DIRECT bounce that generates its rays, k_raygen through the stepping interface for the group's first
    seed, and pt_set_lens switching the camera's rays between a lens and the pinhole in the middle of a session: the tables that
    depend on rays that repeat (the first-hit and first-state tables, the camera masks) come and go with it."""
    rep = Report("camera, " + kind, launch_plan)
    for seed, w, h in frames(rs.CAMERA_SEEDS, group):
        camera_session(pt, po, rep, kind, seed, w, h, seed == group[0] and (w, h) == (W, H), launch_plan)
    rep.done()


# ---- the filters -------------------------------------------------------------------------------------------------------------------
def planes_equal(rep, seed, w, what, got, want):
    diff = bits(got) != bits(want)
    if diff.any():
        p = int(np.nonzero(diff.reshape(len(got), -1).any(axis=1))[0][0])
        rep.lines.append("seed %d, %s [%s], %s: %d of %d words differ; first pixel %d (x %d, y %d): got %r, want %r" %
                         (seed, rep.session, rep.plan, what, int(diff.sum()), diff.size, p, p % w, p // w, got[p].tolist(), want[p].tolist()))


@pytest.mark.parametrize("group", rs.groups(rs.FILTER_SEEDS))
def test_filters(pt, po, launch_plan, group):
    """On the plain compacting session after two iterations: pt_gbuffer against the oracle's first hits (|position| up to hundreds,
    a depth discontinuity at nearly every pixel), pt_denoise at 1 and 5 levels, and pt_denoise_temporal with pt_history under the
    seed's camera, after a move of (0.3, 0.2, 0) and under the next seed's perturbed camera, which leaves positions behind the old
    camera and off its frame -- every pixel against atrous_model and temporal_model."""
    rep = Report("filters", launch_plan)
    for seed, w, h in frames(rs.FILTER_SEEDS, group):
        geoms, mats, cam, depth = rs.scene(pt, seed, w, h)
        fr = rs.filter_run(po, pt, seed, rs.next_seed(rs.FILTER_SEEDS, seed), w, h)
        scene = pt.Scene(geoms, mats, cam, depth)
        pt.pathtraceInit(scene, flags=pt.PT_COMPACT, max_batch=2)
        try:
            for k, c in enumerate(fr["cams"]):
                if k:
                    scene.camera = c
                    pt.set_camera(c, depth)
                    pt.clear_image()
                pt.trace_batch(1, 2)
                what = ("own camera", "moved camera", "camera of the next seed")[k]
                if not rep.image(seed, w, what + ": running sum", pt.get_image(w * h), fr["images"][k]):
                    continue
                g = pt.gbuffer()
                for key in ("t", "normal", "position", "materialId"):
                    planes_equal(rep, seed, w, what + ": G-buffer " + key, g[key], fr["g"][k][key])
                if k == 0:
                    for levels in (1, 5):
                        planes_equal(rep, seed, w, "pt_denoise, %d levels" % levels, pt.denoise(2, levels, *rs.SIGMAS), fr["denoise"][levels])
                got = pt.denoise_temporal(2, pt.DenoiseParams(5, *rs.SIGMAS), pt.TemporalParams(64, 0.1, 0.1))
                hc, hn = pt.history()
                want, whc, whn = fr["temporal"][k]
                planes_equal(rep, seed, w, what + ": history lengths", hn, whn)
                planes_equal(rep, seed, w, what + ": history colours", hc, whc)
                planes_equal(rep, seed, w, what + ": pt_denoise_temporal", got, want)
        finally:
            pt.pathtraceFree()
    rep.done()


@pytest.mark.parametrize("group", rs.groups(rs.TEXTURED_SEEDS))
def test_albedo_and_the_demodulating_filter(pt, po, launch_plan, group):
    """On the textured session after three iterations: pt_albedo against albedo_model (tinted first hits on stretched primitives,
    the clamp) and pt_denoise with the switch on."""
    rep = Report("albedo", launch_plan)
    for seed, w, h in frames(rs.TEXTURED_SEEDS, group):
        geoms, mats, cam, depth = rs.scene(pt, seed, w, h)
        run, _, f = rs.textured_run(po, pt, seed, w, h)
        A, want = rs.albedo_run(po, pt, seed, w, h)
        pt.pathtraceInit(pt.Scene(geoms, f.materials, cam, depth), flags=pt.PT_COMPACT | pt.PT_TEXTURES | pt.PT_GLOSSY, max_batch=3)
        try:
            for k, t in f.bump_maps.items():
                pt.set_bump_map(k, t)
            for k, t in f.textures.items():
                pt.set_texture(k, t)
            if f.sky is not None:
                pt.set_environment(f.sky)
            pt.trace_batch(1, 3)
            if rep.image(seed, w, "running sum", pt.get_image(w * h), run.images[3], run, (1, 2, 3)):
                planes_equal(rep, seed, w, "pt_albedo", pt.albedo(), A)
                pt.set_denoise_albedo(True)
                planes_equal(rep, seed, w, "pt_denoise on irradiance, 3 levels", pt.denoise(3, 3, *rs.SIGMAS), want)
        finally:
            pt.pathtraceFree()
    rep.done()
