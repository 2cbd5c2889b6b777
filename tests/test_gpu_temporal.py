"""GPU: pt_denoise_temporal / pt_history / pt_history_reset (include/ptmi355.h).  Every comparison is
bit for bit on every pixel against tests/temporal_model.py fed with the oracle's G-buffers and the device's own running
sums: the reprojected history planes, the blended and filtered result and its RGBA form, across one and two camera moves,
with specular first hits, a mesh under PT_MESH_BVH and a rotation that puts part of the frame outside the old one.  The
calls leave the session alone (PT_LOOKAHEAD windows included), pt_denoise and the temporal calls do not disturb each other,
bad arguments and sessions that hold a tile are refused, the buffers are allocated once, and ptbench --move writes a picture
that is closer to the converged one than the filter alone gets.  Under both launch plans."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import __graft_entry__ as ge  # noqa: E402,F401
import atrous_model as am  # noqa: E402
import temporal_model as tm  # noqa: E402
from gpu_common import pt, launch_plan, bits, rel_l2, _resized  # noqa: E402,F401

pytestmark = pytest.mark.gpu

FILT = (5, 4.0, 0.35, 0.5)
TEMP = (64, 0.1, 0.1)
MOVE = (0.3, 0.2, 0.0)


def moved(cam, d):
    """position and lookAt translated by d: view / up / right stay"""
    c = cam.copy()
    c["position"][0] += np.asarray(d, dtype=np.float32)
    c["lookAt"][0] += np.asarray(d, dtype=np.float32)
    return c


def turned(cam, d):
    """lookAt moved by d, position kept; view / right / up recomputed from them (right from view and up, normalised)"""
    c = cam.copy()
    c["lookAt"][0] += np.asarray(d, dtype=np.float32)
    v = (c["lookAt"][0] - c["position"][0]).astype(np.float32)
    v = (v / np.float32(np.sqrt((v * v).sum()))).astype(np.float32)
    r = np.cross(v, c["up"][0]).astype(np.float32)
    r = (r / np.float32(np.sqrt((r * r).sum()))).astype(np.float32)
    c["view"][0], c["right"][0], c["up"][0] = v, r, np.cross(r, v).astype(np.float32)
    return c


def launches(pt):
    """(k_reproject, k_temporal_blend) launches since pt_init"""
    out = (C.c_uint64 * 2)()
    assert pt.library().ptdbg_temporal(out) == 0
    return tuple(int(v) for v in out)


def hip_runtime():
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return C.CDLL(line.split()[-1])
    raise AssertionError("no HIP runtime loaded")


def free_memory():
    hip = hip_runtime()
    hip.hipMemGetInfo.argtypes = [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return int(free.value)


def same(got, want, what):
    diff = bits(got) != bits(want)
    assert not diff.any(), "%s: %d of %d words differ" % (what, int(diff.sum()), diff.size)


class Pair:
    """the device's temporal calls beside the model's: every call compares the result, its RGBA form and the history planes"""

    def __init__(self, pt, w, h, materials):
        self.pt, self.n = pt, w * h
        self.model = tm.Temporal(w, h, materials)

    def call(self, iters, cam, g, filt=FILT, temp=TEMP, what=""):
        pt = self.pt
        image_sum = pt.get_image(self.n)
        got, px = pt.denoise_temporal(iters, pt.DenoiseParams(*filt), pt.TemporalParams(*temp), rgba=True)
        want = self.model.call(image_sum, iters, cam, g, *filt, max_history=temp[0], ptol=temp[1], ntol=temp[2])
        assert np.isfinite(want).all()
        hc, hn = pt.history()
        same(hn, self.model.hn, what + " Hn")
        same(hc, self.model.hc, what + " Hc")
        same(got, want, what + " result")
        assert px.tobytes() == am.rgba8(want).tobytes(), what + " RGBA"
        only = pt.denoise_temporal(iters, pt.DenoiseParams(*filt), pt.TemporalParams(*temp))          # without the RGBA form
        assert only.tobytes() == got.tobytes()
        return got


def oracle_gbuffer(po, cam, depth, geoms, tris=None, meshes=None):
    if tris is None:
        return am.gbuffer_from_oracle(po, cam, depth, geoms)
    return am.gbuffer_from_oracle(po, cam, depth, geoms.view(po.GEOM_DT), tris.view(po.TRI_DT), meshes.view(po.MESH_DT))


# ---- 4. Cornell 800 x 800: one move, more samples, the move back ------------------------------------------------------------
def test_cornell_800_two_moves(pt, po, scenes, launch_plan):
    s = scenes["cornell"]
    w = h = 800
    n = w * h
    cam_a = s["camera"]
    cam_b = moved(cam_a, MOVE)
    g_a = oracle_gbuffer(po, cam_a, s["depth"], s["geoms"])
    g_b = oracle_gbuffer(po, cam_b, s["depth"], s["geoms"])
    scene = pt.Scene(s["geoms"], s["materials"], cam_a, s["depth"])
    pt.pathtraceInit(scene, flags=pt.PT_COMPACT, max_batch=16)
    try:
        pt.trace_batch(1, 16, None)
        plain = pt.denoise(16, *FILT)
        pair = Pair(pt, w, h, s["materials"])
        first = pair.call(16, cam_a, g_a, what="first call")
        same(first, plain, "first temporal call against pt_denoise")
        assert not pt.history()[1].any()
        assert launches(pt) == (0, 2)

        pt.set_camera(cam_b, s["depth"])
        pt.clear_image()
        pt.trace_batch(1, 1, None)
        pair.call(1, cam_b, g_b, what="moved, 1 spp")
        share = float((pair.model.hn > 0).mean())
        print("share of pixels with history after the move: %.3f" % share)
        assert 0.5 < share < 0.95 and (pair.model.hn[pair.model.hn > 0] == 16).all()
        assert launches(pt) == (1, 4)                              # one reprojection per camera change, one blend per call
        hist = [a.copy() for a in pt.history()]
        pt.trace_batch(2, 3, None)
        pair.call(4, cam_b, g_b, what="moved, 4 spp")
        again = pt.history()
        assert again[0].tobytes() == hist[0].tobytes() and again[1].tobytes() == hist[1].tobytes()
        assert launches(pt) == (1, 6)

        # back to the first camera: history of history, capped
        pt.set_camera(cam_a, s["depth"])
        pt.clear_image()
        pt.trace_batch(1, 1, None)
        pair.call(1, cam_a, g_a, temp=(10, 0.1, 0.1), what="moved back, 1 spp")
        hn = pair.model.hn
        lengths = set(np.unique(hn).tolist())                      # none / B's own 4 samples / B's 4 + A's 16, capped at 10
        assert lengths <= {0.0, 4.0, 10.0} and {0.0, 10.0} <= lengths, lengths
        assert (hn == 10).sum() > n // 2
        assert launches(pt) == (2, 8)
    finally:
        pt.pathtraceFree()


# ---- 5. specular first hits, a mesh through the hierarchy, a rotation ----------------------------------------------------------
def test_glass_1280x720_one_move(pt, po, scenes, launch_plan):
    s = scenes["cornell_glass"]
    w, h = 1280, 720
    cam_a = _resized(s["camera"], w, h)
    cam_b = moved(cam_a, MOVE)
    g_a = oracle_gbuffer(po, cam_a, s["depth"], s["geoms"])
    g_b = oracle_gbuffer(po, cam_b, s["depth"], s["geoms"])
    scene = pt.Scene(s["geoms"], s["materials"], cam_a, s["depth"])
    pt.pathtraceInit(scene, flags=pt.PT_COMPACT, max_batch=16)
    try:
        pt.trace_batch(1, 16, None)
        pair = Pair(pt, w, h, s["materials"])
        pair.call(16, cam_a, g_a, what="first call")
        pt.set_camera(cam_b, s["depth"])
        pt.clear_image()
        pt.trace_batch(1, 2, None)
        pair.call(2, cam_b, g_b, what="moved")
        mat = g_b["materialId"]
        mats = s["materials"]
        specular = (mat >= 0) & ((mats["hasReflective"][np.clip(mat, 0, None)] != 0) | (mats["hasRefractive"][np.clip(mat, 0, None)] != 0))
        assert specular.sum() > 1000 and not pair.model.hn[specular].any()       # mirror and glass first hits carry no history
        diffuse = (mat >= 0) & ~specular                         # a small move: most diffuse points were in the first view too
        assert (pair.model.hn[diffuse] > 0).mean() > 0.5
    finally:
        pt.pathtraceFree()


def test_mesh_bvh_one_move(pt, po, scenes, launch_plan):
    s = scenes["cornell"]
    w, h = 256, 192
    cam_a = _resized(s["camera"], w, h)
    cam_b = moved(cam_a, (-0.4, 0.3, 0.5))
    tris = pt.meshes.uv_sphere(center=(1.5, 3.0, 1.0), radius=1.5, n_lat=24, n_lon=48)
    geoms, tris, meshes = pt.meshes.add_mesh(s["geoms"], tris, material_id=2)
    g_a = oracle_gbuffer(po, cam_a, s["depth"], geoms, tris, meshes)
    g_b = oracle_gbuffer(po, cam_b, s["depth"], geoms, tris, meshes)
    scene = pt.Scene(geoms, s["materials"], cam_a, s["depth"], triangles=tris, meshes=meshes)
    pt.pathtraceInit(scene, flags=pt.PT_COMPACT | pt.PT_MESH_BVH, max_batch=8)
    try:
        pt.trace_batch(1, 8, None)
        pair = Pair(pt, w, h, s["materials"])
        pair.call(8, cam_a, g_a, what="first call")
        pt.set_camera(cam_b, s["depth"])
        pt.clear_image()
        pt.trace_batch(1, 1, None)
        pair.call(1, cam_b, g_b, what="moved")
        on_mesh = g_b["materialId"] == 2
        assert (pair.model.hn[on_mesh] > 0).sum() > 100 and (pair.model.hn[g_b["materialId"] >= 0] > 0).mean() > 0.5
    finally:
        pt.pathtraceFree()


def test_rotation_97x61_part_of_the_frame_comes_from_outside(pt, po, scenes, launch_plan):
    """The first view is the scene's camera turned to the right (lookAt moved by (4, 0.5, 0), position kept), so that the left
    of the box is outside its frame; the second is the scene's own: the lookAt moved back, a rotation about the same position.
    (Turning AWAY from the scene's camera reprojects nothing outside: that camera sees the whole box.)"""
    s = scenes["cornell"]
    w, h = 97, 61
    cam_b = _resized(s["camera"], w, h)
    cam_a = turned(cam_b, (4.0, 0.5, 0.0))
    assert cam_b["view"].tobytes() != cam_a["view"].tobytes() and cam_b["position"].tobytes() == cam_a["position"].tobytes()
    g_a = oracle_gbuffer(po, cam_a, s["depth"], s["geoms"])
    g_b = oracle_gbuffer(po, cam_b, s["depth"], s["geoms"])
    # the case is what it is meant to be (oracle and model alone: 472 of 3136 hit pixels lie outside the first frame)
    valid, _ = tm.project(cam_a, g_b["position"], w, h)
    outside = (g_b["materialId"] >= 0) & ~valid
    assert outside.sum() > 100
    scene = pt.Scene(s["geoms"], s["materials"], cam_a, s["depth"])
    pt.pathtraceInit(scene, flags=pt.PT_COMPACT, max_batch=16)
    try:
        pt.trace_batch(1, 16, None)
        pair = Pair(pt, w, h, s["materials"])
        pair.call(16, cam_a, g_a, filt=(6, 1.0, 0.35, 0.5), what="first call")
        pt.set_camera(cam_b, s["depth"])
        pt.clear_image()
        pt.trace_batch(1, 1, None)
        pair.call(1, cam_b, g_b, filt=(6, 1.0, 0.35, 0.5), what="turned")
        assert not pair.model.hn[outside].any()                  # a point outside the first frame has no history
        assert (pair.model.hn > 0).sum() > 1000                  # and the rest of the frame does (model: 2505 pixels)
    finally:
        pt.pathtraceFree()


# ---- 6. reset; pt_denoise and the temporal calls side by side ---------------------------------------------------------------
def test_reset_and_interleaved_plain_calls(pt, po, scenes, launch_plan):
    s = scenes["cornell"]
    w, h = 320, 200
    n = w * h
    cam_a = _resized(s["camera"], w, h)
    cam_b = moved(cam_a, MOVE)
    g_a = oracle_gbuffer(po, cam_a, s["depth"], s["geoms"])
    g_b = oracle_gbuffer(po, cam_b, s["depth"], s["geoms"])
    scene = pt.Scene(s["geoms"], s["materials"], cam_a, s["depth"])
    filt = (4, 2.0, 0.35, 0.5)

    def run(interleave):
        """temporal results (A, B at 1 spp, B at 3 spp, after a reset) and, when interleaved, the pt_denoise results between them"""
        pt.pathtraceInit(scene, flags=pt.PT_COMPACT, max_batch=8)
        try:
            plain, temporal = [], []
            pair = Pair(pt, w, h, s["materials"])
            pt.trace_batch(1, 8, None)
            if interleave:
                plain.append(pt.denoise(8, *filt))
            temporal.append(pair.call(8, cam_a, g_a, filt=filt, what="A"))
            if interleave:
                plain.append(pt.denoise(8, 2, 1.0))
            pt.set_camera(cam_b, s["depth"])
            pt.clear_image()
            pt.trace_batch(1, 1, None)
            if interleave:
                plain.append(pt.denoise(1, *filt))              # computes B's G-buffer before the temporal call needs A's
            temporal.append(pair.call(1, cam_b, g_b, filt=filt, what="B, 1 spp"))
            pt.trace_batch(2, 2, None)
            if interleave:
                plain.append(pt.denoise(3, *filt))
            temporal.append(pair.call(3, cam_b, g_b, filt=filt, what="B, 3 spp"))
            if interleave:
                hist = pt.history()
                plain.append(pt.denoise(3, 0))
                assert pt.history()[1].tobytes() == hist[1].tobytes() and pt.history()[0].tobytes() == hist[0].tobytes()
            pt.history_reset()
            pair.model.reset()
            assert not pt.history()[1].any() and not pt.history()[0].any()
            temporal.append(pair.call(3, cam_b, g_b, filt=filt, what="after the reset"))
            same(temporal[-1], pt.denoise(3, *filt), "after the reset: pt_denoise")
            assert not pt.history()[1].any()
            return plain, temporal
        finally:
            pt.pathtraceFree()

    plain, temporal = run(True)
    _, alone = run(False)
    for a, b in zip(temporal, alone):
        assert a.tobytes() == b.tobytes()
    # pt_denoise between temporal calls returns what it returns without them
    pt.pathtraceInit(scene, flags=pt.PT_COMPACT, max_batch=8)
    try:
        pt.trace_batch(1, 8, None)
        want = [pt.denoise(8, *filt), pt.denoise(8, 2, 1.0)]
        pt.set_camera(cam_b, s["depth"])
        pt.clear_image()
        pt.trace_batch(1, 1, None)
        want.append(pt.denoise(1, *filt))
        pt.trace_batch(2, 2, None)
        want += [pt.denoise(3, *filt), pt.denoise(3, 0)]
        with pytest.raises(pt.PtError):
            pt.history()                                        # no temporal call in this session
        pt.history_reset()                                      # nothing to forget: fine
    finally:
        pt.pathtraceFree()
    assert len(want) == len(plain)
    for a, b in zip(plain, want):
        assert a.tobytes() == b.tobytes()


# ---- 7. the session is left alone -----------------------------------------------------------------------------------------
def test_session_is_unchanged_by_temporal_calls(pt, scenes, launch_plan):
    s = scenes["cornell"]
    cam = _resized(s["camera"], 256, 256)
    n = 256 * 256
    scene = pt.Scene(s["geoms"], s["materials"], cam, s["depth"])
    pt.pathtraceInit(scene, flags=pt.PT_COMPACT, max_batch=4)
    try:
        pt.trace_batch(1, 4, None)
        pt.trace_batch_async(5, 4)                             # still in flight when the filter is asked for
        pt.denoise_temporal(8)
        image, rays, counters = pt.get_image(n).copy(), pt.total_rays(), pt.counters()
        st = pt.get_stats()
        stats = (st.bounces, st.rays, list(st.live), st.total_rays, st.total_iterations)
        pt.denoise_temporal(8, pt.DenoiseParams(3, 1.0, 0.35, 0.5))
        pt.history()
        pt.history_reset()
        pt.denoise_temporal(8, pt.DenoiseParams(0, 1.0, 0.35, 0.5))
        st = pt.get_stats()
        assert pt.get_image(n).tobytes() == image.tobytes()
        assert pt.total_rays() == rays and pt.counters() == counters
        assert (st.bounces, st.rays, list(st.live), st.total_rays, st.total_iterations) == stats
        # and tracing goes on as if nothing had happened
        pt.trace_batch(9, 4, None)
        after = pt.get_image(n).copy()
    finally:
        pt.pathtraceFree()
    pt.pathtraceInit(scene, flags=pt.PT_COMPACT, max_batch=4)
    try:
        for it in (1, 5, 9):
            pt.trace_batch(it, 4, None)
        assert pt.get_image(n).tobytes() == after.tobytes()
    finally:
        pt.pathtraceFree()


def test_lookahead_windows_survive_temporal_calls(pt, po, scenes, launch_plan):
    """PT_PIN_IMAGE | PT_HOST_SPARSE | PT_LOOKAHEAD, max_batch 16, iterations 1..40, a pt_denoise_temporal after calls 1, 7, 16 and
    17: the host image after EVERY call is the oracle's running sum, every result is the model's on that sum, and the rays
    served add up to the run without the calls (a discarded window would show as re-traced rays)."""
    s = scenes["cornell"]
    w, h = 400, 300
    cam = _resized(s["camera"], w, h)
    n = w * h
    depth = s["depth"]
    scene = pt.Scene(s["geoms"], s["materials"], cam, depth)
    L = pt.library()
    flags = pt.PT_COMPACT | pt.PT_LOOKAHEAD | pt.PT_PIN_IMAGE | pt.PT_HOST_SPARSE
    g = am.gbuffer_from_oracle(po, cam, depth, s["geoms"])
    filt = (4, 1.0, 0.35, 0.5)

    def book():
        out = (C.c_uint64 * 4)()
        assert L.ptdbg_lookahead(out) == 0
        return tuple(int(v) for v in out)

    def run(calls_after):
        buf = np.full((n, 3), -7.0, dtype=np.float32)
        ref = po.Tracer(s["geoms"], s["materials"], cam, depth, flags=po.F_COMPACT, trig=po.TRIG_SHARED)
        model = tm.Temporal(w, h, s["materials"])
        pt.pathtraceInit(scene, flags=flags, max_batch=16, pin_image=False)
        try:
            served = 0
            for it in range(1, 41):
                assert L.pt_trace(None, 0, it, buf.ctypes.data) == 0, L.pt_last_error()
                ref.iterate(it, threads=8)
                assert (bits(buf) == bits(ref.image)).all(), "host image after iteration %d" % it
                served += pt.get_stats().rays
                if it in calls_after:
                    b0 = book()
                    got = pt.denoise_temporal(it, pt.DenoiseParams(*filt))
                    want = model.call(ref.image, it, cam, g, *filt)
                    same(got, want, "temporal result after iteration %d" % it)
                    assert book() == b0                        # no window enqueued, missed or discarded by the call
                    assert (bits(buf) == bits(ref.image)).all()
                    assert (bits(pt.get_image(n)) == bits(ref.image)).all()
            return served, book()[:3], pt.counters()
        finally:
            pt.pathtraceFree()

    plain = run(())
    with_calls = run((1, 7, 16, 17))
    assert with_calls[0] == plain[0]
    assert with_calls[1] == plain[1] and plain[1][2] == 0      # the same windows, none thrown away
    assert with_calls[2][1:] == plain[2][1:]


# ---- 8. errors, life time, memory ---------------------------------------------------------------------------------------------
def test_bad_arguments_and_tiled_sessions_are_refused(pt, po, scenes, launch_plan):
    s = scenes["cornell_64"]
    scene = pt.Scene(s["geoms"], s["materials"], s["camera"], s["depth"])
    L = pt.library()
    n = 64 * 64

    def refused(word, levels=5, sc=1.0, sn=0.35, sp=0.5, it=4, null=False, cap=64, tp=0.1, tn=0.1, tnull=False):
        prm = pt.DenoiseParams(levels, sc, sn, sp)
        tmp = pt.TemporalParams(cap, tp, tn)
        rc = L.pt_denoise_temporal(None if null else C.byref(prm), None if tnull else C.byref(tmp), it, None, None)
        assert rc == -1, (word, levels, sc, sn, sp, it, cap, tp, tn)
        assert word.encode() in L.pt_last_error() and b"pt_denoise_temporal" in L.pt_last_error(), L.pt_last_error()

    pt.pathtraceFree()
    refused("not initialised")
    pt.pathtraceInit(scene, flags=pt.PT_COMPACT, max_batch=4)
    try:
        pt.trace_batch(1, 4, None)
        refused("params", null=True)
        refused("temporal", tnull=True)
        refused("levels", levels=-1)
        refused("levels", levels=11)
        for name, key in (("sigma_color", "sc"), ("sigma_normal", "sn"), ("sigma_position", "sp"),
                          ("position_tolerance", "tp"), ("normal_tolerance", "tn")):
            for bad in (0.0, -1.0, float("nan"), float("inf"), 1e-30):       # 1e-30: its square is not a normal number
                refused(name, **{key: bad})
        refused("sigma_color", levels=10, sc=1e-17)
        refused("iter", it=0)
        refused("max_history", cap=-1)
        refused("max_history", cap=(1 << 20) + 1)
        assert L.pt_history(None, None) == -1 and b"pt_history" in L.pt_last_error()      # no temporal call yet
        img = pt.denoise_temporal(4, pt.DenoiseParams(10, 2e-16, 0.35, 0.5), pt.TemporalParams(1 << 20, 2e-19, 2e-19))
        assert img.shape == (n, 3)
        assert pt.denoise_temporal(4, temporal=pt.TemporalParams(0, 0.1, 0.1)).shape == (n, 3)
        assert L.pt_history(None, None) == 0
        ref = po.Tracer(s["geoms"], s["materials"], s["camera"], s["depth"], flags=po.F_COMPACT, trig=po.TRIG_SHARED)
        for it in range(1, 9):
            ref.iterate(it)
        pt.trace_batch(5, 4, None)                                 # the session still traces correctly
        assert (bits(pt.get_image(n)) == bits(ref.image)).all()
    finally:
        pt.pathtraceFree()
    for kw in (dict(devices=[0, 0]), dict(tile=(0, 2, 8))):
        pt.pathtraceInit(scene, flags=pt.PT_COMPACT, max_batch=4, **kw)
        try:
            pt.trace_batch(1, 4, None)
            before = pt.get_image(n).copy()
            refused("tile")
            assert L.pt_history(None, None) == -1 and b"tile" in L.pt_last_error()
            assert L.pt_history_reset() == -1 and b"tile" in L.pt_last_error()
            pt.trace_batch(5, 4, None)
            assert pt.get_image(n).tobytes() != before.tobytes()
            if "devices" in kw:
                assert (bits(pt.get_image(n)) == bits(ref.image)).all()
        finally:
            pt.pathtraceFree()


def test_free_ends_the_history_and_the_buffers_are_allocated_once(pt, po, scenes, launch_plan):
    s = scenes["cornell"]
    w, h = 512, 512
    n = w * h
    cam_a = _resized(s["camera"], w, h)
    cam_b = moved(cam_a, MOVE)
    scene = pt.Scene(s["geoms"], s["materials"], cam_a, s["depth"])
    filt = pt.DenoiseParams(2, 1.0, 0.35, 0.5)
    pt.pathtraceInit(scene, flags=pt.PT_COMPACT, max_batch=4)
    try:
        pt.trace_batch(1, 4, None)
        pt.denoise_temporal(4, filt)
        pt.set_camera(cam_b, s["depth"])
        pt.denoise_temporal(4, filt)                           # the second call, the first with a reprojection: everything is allocated
        assert (pt.history()[1] > 0).sum() > n // 2
        free = free_memory()
        results = {}
        for k in range(20):
            cam = cam_a if k % 2 == 0 else cam_b
            pt.set_camera(cam, s["depth"])
            got = pt.denoise_temporal(4, filt)
            assert np.isfinite(got).all()
            results[k] = got
        assert free_memory() == free
        assert launches(pt) == (21, 22)
    finally:
        pt.pathtraceFree()
    # a new session starts without history: the first temporal call at the moved camera is pt_denoise
    pt.pathtraceInit(scene, flags=pt.PT_COMPACT, max_batch=4)
    try:
        with pytest.raises(pt.PtError):
            pt.history()
        pt.set_camera(cam_b, s["depth"])
        pt.trace_batch(1, 4, None)
        got = pt.denoise_temporal(4, filt)
        same(got, pt.denoise(4, 2, 1.0, 0.35, 0.5), "first temporal call of a new session")
        assert not pt.history()[1].any() and launches(pt) == (0, 1)
    finally:
        pt.pathtraceFree()


# ---- 9. the headless host ------------------------------------------------------------------------------------------------------
def test_ptbench_move_writes_three_pictures_and_the_temporal_one_is_closer(pt, po, scenes, tmp_path, launch_plan):
    from PIL import Image
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = pt.build_ptbench()
    base = str(tmp_path / "r")
    p = subprocess.run([exe, os.path.join(root, "scenes", "cornell.txt"), "--iters", "16", "--out", base, "--denoise", "5,4.0,0.35,0.5",
                        "--move", "0.3,0.2,0,1"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "move (0.3, 0.2, 0), 1 iterations" in p.stdout, p.stdout
    pics = {}
    for kind in ("", ".denoised", ".temporal"):
        path = "%s.moved.1samp%s.png" % (base, kind)
        assert os.path.exists(path), path
        pics[kind] = np.asarray(Image.open(path).convert("RGB"), dtype=np.float64).reshape(-1, 3) / 255.0
    assert os.path.exists(base + ".16samp.png") and os.path.exists(base + ".16samp.denoised.png")
    # the converged picture of the moved view: 256 spp on this device, through the same 8-bit rule
    s = scenes["cornell"]
    cam_b = moved(s["camera"], MOVE)
    scene = pt.Scene(s["geoms"], s["materials"], cam_b, s["depth"])
    pt.pathtraceInit(scene, flags=pt.PT_COMPACT, max_batch=32)
    try:
        for it in range(1, 257, 32):
            pt.trace_batch(it, 32, None)
        conv = pt.image_to_rgb8(pt.get_image(800 * 800), 800, 800, 256.0).reshape(-1, 3).astype(np.float64) / 255.0
    finally:
        pt.pathtraceFree()
    e = {k: rel_l2(v, conv) for k, v in pics.items()}
    print("rel-L2 against 256 spp of the moved view (8-bit pictures): raw %.4f, denoised %.4f, temporal %.4f" % (e[""], e[".denoised"], e[".temporal"]))
    assert e[".temporal"] < e[".denoised"]
    # --move without --denoise is refused
    p = subprocess.run([exe, os.path.join(root, "scenes", "cornell.txt"), "--iters", "1", "--out", base, "--move", "0.3,0.2,0,1"],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode != 0 and "--denoise" in p.stderr
