"""GPU parity, deferred diffuse directions: where the next bounce is the fused compacting k_bounce, a diffuse survivor
is stored with its hit normal in the direction row and a pending mark in its pid, and that bounce -- or pt_export_paths
-- draws the direction (csrc/pt_k_bounce.hpp: tile_load<RESOLVE>).  Nothing observable may change:
live counts, pool order, every exported path, final colours and images stay bit-identical to the oracle, in stepped
and batched sessions, under PT_LOOKAHEAD, on the producers the plan lets defer (the fused kernel, the first-bounce
cache) and across sessions whose pipelines never resolve (sort, unfused, non-compacting)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import __graft_entry__ as ge  # noqa: E402,F401
from gpu_common import pt, launch_plan, bits, assert_paths_equal, _after  # noqa: E402,F401

pytestmark = pytest.mark.gpu


def _stepped_iterations(pt, po, s, flags, iterations):
    """Step every bounce of one-sample batches, export after each one and hold the pool against the oracle's snapshot;
    then the live counts and the image."""
    n = int(s["camera"]["resolution"][0][0]) * int(s["camera"]["resolution"][0][1])
    oflags = (po.F_COMPACT if flags & pt.PT_COMPACT else 0) | (po.F_SORT if flags & pt.PT_SORT_MATERIAL else 0)
    ref = po.Tracer(s["geoms"], s["materials"], s["camera"], s["depth"], flags=oflags, trig=po.TRIG_SHARED)
    for it in iterations:
        snaps = []
        st = ref.iterate(it, snapshots=snaps)
        pt.trace_begin(it, 1)
        for snap in snaps:
            d = snap["depth"]
            n_live = pt.trace_bounce(d)
            paths, live = pt.export_paths(n)
            if flags & pt.PT_COMPACT:
                assert n_live == snap["n_live"] == live, (it, d)
                assert_paths_equal(paths, _after(snaps, d, ref), live)
            else:
                alive = paths["pixelIndex"] >= 0
                wp = _after(snaps, d, ref)
                assert (alive == (wp["remainingBounces"] > 0)[:len(alive)]).all()
                assert_paths_equal(paths[alive], wp[:len(alive)][alive], int(alive.sum()))
        for d in range(len(snaps), s["depth"]):
            pt.trace_bounce(d)
        pt.trace_end()
        gs = pt.get_stats()
        assert list(gs.live[:s["depth"]]) == list(st.live[:s["depth"]]), it
        assert gs.rays == st.rays
        assert pt.get_image(n).tobytes() == ref.image.tobytes(), it


@pytest.mark.parametrize("scene_name", ["cornell", "cornell_glass_64"])
@pytest.mark.parametrize("flags_name", ["fused", "cache"])
def test_export_after_every_bounce(pt, po, scenes, scene_name, flags_name):
    """C2 and a diffuse + mirror + glass scene: the exported pool after every bounce is the oracle's, pending directions
    drawn by the export; the first-bounce cache's k_bounce defers too."""
    s = scenes[scene_name]
    flags = {"fused": pt.PT_COMPACT, "cache": pt.PT_COMPACT | pt.PT_CACHE_FIRST}[flags_name]
    pt.pathtraceInit(pt.Scene(s["geoms"], s["materials"], s["camera"], s["depth"]), flags=flags)
    _stepped_iterations(pt, po, s, flags, (1, 2))
    pt.pathtraceFree()


@pytest.mark.parametrize("scene_name", ["cornell_64", "cornell_glass_64"])
def test_64_sample_batch(pt, po, scenes, scene_name):
    """One batch of 64 samples per pixel: the resolving loads draw with the engine of their sample's iteration."""
    s = scenes[scene_name]
    n = int(s["camera"]["resolution"][0][0]) * int(s["camera"]["resolution"][0][1])
    pt.pathtraceInit(pt.Scene(s["geoms"], s["materials"], s["camera"], s["depth"]), flags=pt.PT_COMPACT, max_batch=64)
    ref = po.Tracer(s["geoms"], s["materials"], s["camera"], s["depth"], flags=po.F_COMPACT, trig=po.TRIG_SHARED)
    for iter0 in (1, 65):
        pt.trace_batch(iter0, 64)
        rays = ref.iterate_parallel(iter0, 64, 8)
        assert pt.get_stats().rays == rays
        assert (bits(pt.get_image(n)) == bits(ref.image)).all(), iter0
    pt.pathtraceFree()


def test_stepped_batch_of_two_samples(pt, po, scenes):
    """A stepped batch whose pool holds two samples: every bounce resolves what the one before it left pending."""
    s = scenes["cornell_glass_64"]
    n = int(s["camera"]["resolution"][0][0]) * int(s["camera"]["resolution"][0][1])
    pt.pathtraceInit(pt.Scene(s["geoms"], s["materials"], s["camera"], s["depth"]), flags=pt.PT_COMPACT, max_batch=2)
    ref = po.Tracer(s["geoms"], s["materials"], s["camera"], s["depth"], flags=po.F_COMPACT, trig=po.TRIG_SHARED)
    pt.trace_begin(3, 2)
    for d in range(s["depth"]):
        pt.trace_bounce(d)
        paths, live = pt.export_paths(2 * n)
        assert len(paths) == live
        assert (np.abs(np.linalg.norm(paths["direction"].astype(np.float64), axis=1) - 1.0) < 1e-5).all(), d
    pt.trace_end()
    rays = ref.iterate_parallel(3, 2, 2)
    assert pt.get_stats().rays == rays
    assert (bits(pt.get_image(n)) == bits(ref.image)).all()
    pt.pathtraceFree()


def test_lookahead_windows(pt, po, scenes):
    """PT_LOOKAHEAD: windows of up to eight iterations traced ahead of the calls, the image after every call."""
    s = scenes["cornell_glass_64"]
    pt.pathtraceInit(pt.Scene(s["geoms"], s["materials"], s["camera"], s["depth"]),
                     flags=pt.PT_COMPACT | pt.PT_LOOKAHEAD, max_batch=8)
    ref = po.Tracer(s["geoms"], s["materials"], s["camera"], s["depth"], flags=po.F_COMPACT, trig=po.TRIG_SHARED)
    for it in range(1, 22):
        img = pt.pathtrace(None, 0, it)
        ref.iterate(it)
        assert (bits(img) == bits(ref.image)).all(), it
    pt.pathtraceFree()


def test_pipeline_switch_between_sessions(pt, po, scenes):
    """Sort on, then off, then the unfused and non-compacting pipelines, then the fused one again, on one device: the
    sessions that never resolve must never see a pending slot, and the ones that do must draw every one."""
    s = scenes["cornell_glass_64"]
    scene = pt.Scene(s["geoms"], s["materials"], s["camera"], s["depth"])
    for flags in (pt.PT_COMPACT | pt.PT_SORT_MATERIAL, pt.PT_COMPACT, pt.PT_COMPACT | pt.PT_SORT_MATERIAL | pt.PT_UNFUSED,
                  pt.PT_COMPACT | pt.PT_UNFUSED, 0, pt.PT_COMPACT):
        pt.pathtraceInit(scene, flags=flags, max_batch=4)
        _stepped_iterations(pt, po, s, flags, (1,))
        n = int(s["camera"]["resolution"][0][0]) * int(s["camera"]["resolution"][0][1])
        oflags = (po.F_COMPACT if flags & pt.PT_COMPACT else 0) | (po.F_SORT if flags & pt.PT_SORT_MATERIAL else 0)
        ref = po.Tracer(s["geoms"], s["materials"], s["camera"], s["depth"], flags=oflags, trig=po.TRIG_SHARED)
        ref.iterate(1)
        pt.trace_batch(2, 4)                                # a batch behind the stepped iteration, same accumulation buffer
        ref.iterate_parallel(2, 4, 4)
        assert (bits(pt.get_image(n)) == bits(ref.image)).all(), flags
        pt.pathtraceFree()
