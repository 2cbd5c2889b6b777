"""GPU: pt_denoise_svgf / pt_svgf_history / pt_svgf_variance / pt_svgf_reset (include/ptmi355.h).  Every
comparison is bit for bit on every pixel against tests/svgf_model.py fed with the oracle's G-buffers and the device's own running
sums and moments: the four reprojected history planes, var_0 from both estimates, the filtered result, its RGBA form and the device
plane -- without history (where the call is pt_denoise_variance), on first calls where every pixel takes the spatial estimate, across
one and two camera moves, caps, a jump to a camera that sees nothing, specular first hits, a frame of misses and random hostile
scenes.  The call leaves the session and the three other filters alone, launches exactly what the specification counts, allocates
once, and refuses what it must; ptbench --svgf writes the model's pictures.  Under both launch plans.  Frames are a few thousand
pixels; the module opens no tiled and no multi-device session except, in its LAST test, to see them refused."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import __graft_entry__ as ge  # noqa: E402,F401
import atrous_model as am  # noqa: E402
import random_scenes as rs  # noqa: E402
import svgf_model as sm  # noqa: E402
import variance_model as vm  # noqa: E402
from gpu_common import pt, launch_plan, bits, _resized  # noqa: E402,F401

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIG = (4.0, 0.35, 0.5)
TEMP = (64, 0.1, 0.1)
MOVE = (0.3, 0.2, 0.0)
_g = {}


def moved(cam, d):
    """position and lookAt translated by d: view / up / right stay"""
    c = cam.copy()
    c["position"][0] += np.asarray(d, dtype=np.float32)
    c["lookAt"][0] += np.asarray(d, dtype=np.float32)
    return c


def away(cam):
    """looking out of the open side of the box: every pixel misses"""
    c = cam.copy()
    c["view"][0] = -cam["view"][0]
    c["right"][0] = -cam["right"][0]
    return c


def inside(cam):
    """the scene's camera 6.5 units forward, inside the box: every pixel of a flat, wide frame hits a wall (from outside, 6 % of
    130 x 9 do)"""
    return moved(cam, (0.0, 0.0, -6.5))


def same(got, want, what):
    bad = bits(got) != bits(want)
    assert not bad.any(), "%s: %d of %d words differ, first at %d" % (what, int(bad.sum()), bad.size, int(np.nonzero(bad.reshape(-1))[0][0]))


def counts(pt):
    """(k_reproject_svgf, k_svgf_blend, k_svgf_spatial, G-buffer copies, k_atrous_var, k_variance_mean) since pt_init"""
    a, b = (C.c_uint64 * 4)(), (C.c_uint64 * 2)()
    assert pt.library().ptdbg_svgf(a) == 0 and pt.library().ptdbg_variance(b) == 0
    return tuple(int(v) for v in a) + tuple(int(v) for v in b)


def hip_runtime():
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return C.CDLL(line.split()[-1])
    raise AssertionError("no HIP runtime loaded")


def read_device(ptr, nbytes):
    hip = hip_runtime()
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    buf = np.zeros(nbytes, dtype=np.uint8)
    assert hip.hipMemcpy(buf.ctypes.data, ptr, nbytes, 2) == 0          # hipMemcpyDeviceToHost
    return buf


def free_memory():
    hip = hip_runtime()
    hip.hipMemGetInfo.argtypes = [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return int(free.value)


def gbuffer(po, s, cam):
    """the oracle's first hits of scene s under cam: once per module, never written afterwards"""
    key = (id(s["geoms"]), cam.tobytes())
    if key not in _g:
        _g[key] = am.gbuffer_from_oracle(po, cam, s["depth"], s["geoms"])
    return _g[key]


def init(pt, s, cam, max_batch=4, moments=True):
    pt.pathtraceInit(pt.Scene(s["geoms"], s["materials"], cam, s["depth"]), flags=pt.PT_COMPACT | (pt.PT_MOMENTS if moments else 0),
                     max_batch=max_batch, pin_image=False)


def trace(pt, first, last):
    """iterations first .. last in batches of up to four"""
    it = first
    while it <= last:
        k = min(4, last - it + 1)
        pt.trace_batch(it, k, None)
        it += k


def view(pt, cam, depth):
    """what an interactive host does when the camera moves"""
    pt.set_camera(cam, depth)
    pt.clear_image()


class Pair:
    """the device's calls beside the model's: every call compares the four history planes, var_0, the result, its RGBA form, the
    device plane and the launches the call made"""

    def __init__(self, pt, w, h, materials):
        self.pt, self.w, self.h, self.n = pt, w, h, w * h
        self.model = sm.Svgf(w, h, materials)

    def reset(self):
        self.pt.svgf_reset()
        self.model.reset()

    def call(self, iters, cam, g, levels=5, sig=SIG, temp=TEMP, below=4, what=""):
        pt, n = self.pt, self.n
        image_sum, (m1, m2) = pt.get_image(n), pt.get_moments()
        first = self.model.cur is None
        changed = not first and self.model.cur["camera"].tobytes() != np.ascontiguousarray(cam).tobytes()
        before = counts(pt)
        got, px = pt.denoise_svgf(iters, pt.VarianceParams(levels, *sig), pt.TemporalParams(*temp), below, rgba=True)
        made = tuple(a - b for a, b in zip(counts(pt), before))
        assert made == (int(changed), 1, int(below > 0), int(changed or first), levels, 0), (what, made)
        with np.errstate(all="ignore"):
            want = self.model.call(image_sum, m1, m2, iters, cam, g, levels, *sig, max_history=temp[0], ptol=temp[1], ntol=temp[2],
                                   spatial_below=below)
        hc, h1, h2, hn = pt.svgf_history()
        same(hn, self.model.hn, what + " Hn")
        same(hc, self.model.hc, what + " Hc")
        same(h1, self.model.h1, what + " H1")
        same(h2, self.model.h2, what + " H2")
        same(pt.svgf_variance(), self.model.var0, what + " var_0")
        same(got, want, what + " result, %d levels" % levels)
        assert px.tobytes() == am.rgba8(want).tobytes(), what + " RGBA"
        same(read_device(pt.denoised_device_ptr(), n * 12).view(np.float32).reshape(n, 3), want, what + " device plane")
        return got


# ---- 1. without history and spatial estimate: pt_denoise_variance ------------------------------------------------------------
@pytest.mark.parametrize("w, h", [(31, 29), (130, 9)])
def test_without_history_and_spatial_estimate_it_is_pt_denoise_variance(pt, po, scenes, launch_plan, w, h):
    s = scenes["cornell"]
    cam = _resized(s["camera"], w, h)
    g = gbuffer(po, s, cam)
    init(pt, s, cam)
    try:
        pair = Pair(pt, w, h, s["materials"])
        done = 0
        for it in (1, 2, 5):
            trace(pt, done + 1, it)
            done = it
            for levels in (0, 1, 3, 5):
                got = pair.call(it, cam, g, levels, below=0, what="iter %d" % it)
                same(got, pt.denoise_variance(it, levels, *SIG), "iter %d, %d levels: pt_denoise_variance" % (it, levels))
                same(pt.svgf_variance(), pt.variance(), "iter %d, %d levels: pt_variance" % (it, levels))
            assert not pair.model.hn.any()
    finally:
        pt.pathtraceFree()


# ---- 2. the first call of a view: every pixel takes the spatial estimate ------------------------------------------------------
@pytest.mark.parametrize("w, h", [(64, 16), (67, 5), (130, 9)])
def test_first_calls_take_the_spatial_estimate_everywhere(pt, po, scenes, launch_plan, w, h):
    """64 x 16: whole waves and workgroups, the halo outside the frame on every side; 67 x 5: a frame lower than the halo is wide,
    the last three pixels of a row in a workgroup of their own; 130 x 9: three workgroups across.  From inside the box: every pixel
    hits."""
    s = scenes["cornell"]
    cam = inside(_resized(s["camera"], w, h))
    g = gbuffer(po, s, cam)
    assert (g["t"] > 0).all()
    init(pt, s, cam)
    try:
        pair = Pair(pt, w, h, s["materials"])
        for it, levels in ((1, 5), (2, 1), (3, 0)):
            trace(pt, it, it)
            pair.reset()
            pair.call(it, cam, g, levels, below=4, what="iter %d" % it)
            m = pair.model
            assert (m.cur["N"] == it).all()
            vt = sm.temporal_variance(m.cur["U1"], m.cur["U2"], m.cur["N"])
            assert (bits(m.var0) != bits(vt)).sum() > int((g["t"] > 0).sum()) // 2     # the spatial estimate is another number
        pair.call(3, cam, g, 5, below=3, what="iter 3, spatial_below 3")  # N' = 3 is not below 3: the temporal estimate everywhere
        same(pair.model.var0, vm.var0(*pt.get_moments(), 3), "var_0 at the threshold")
    finally:
        pt.pathtraceFree()


# ---- 3. one move, two moves, caps, a jump ------------------------------------------------------------------------------------
def test_moves_caps_and_a_jump(pt, po, scenes, launch_plan):
    s = scenes["cornell"]
    w, h = 31, 29
    depth = s["depth"]
    cam_a = _resized(s["camera"], w, h)
    cam_b, cam_c, cam_z = moved(cam_a, MOVE), moved(cam_a, (-0.2, 0.1, 0.1)), away(cam_a)
    g_a, g_b, g_c, g_z = (gbuffer(po, s, c) for c in (cam_a, cam_b, cam_c, cam_z))
    assert not (g_z["t"] > 0).any()
    init(pt, s, cam_a)
    try:
        pair = Pair(pt, w, h, s["materials"])
        m = pair.model
        trace(pt, 1, 8)
        pair.call(8, cam_a, g_a, 5, what="A, 8 spp")
        assert not m.hn.any() and (m.cur["N"] == 8).all()
        view(pt, cam_b, depth)
        trace(pt, 1, 1)
        pair.call(1, cam_b, g_b, 5, what="B, 1 spp")
        has = m.hn > 0
        assert 0.5 < has.mean() < 0.95 and (m.hn[has] == 8).all() and (m.h2[has] > 0).any()
        kept = [p.copy() for p in pt.svgf_history()]
        trace(pt, 2, 3)
        pair.call(3, cam_b, g_b, 1, what="B, 3 spp, the same camera")
        for a, b in zip(kept, pt.svgf_history()):
            assert a.tobytes() == b.tobytes()
        pt.clear_image()                                       # without a camera change: this view's samples go, the history stays
        trace(pt, 1, 1)
        pair.call(1, cam_b, g_b, 0, what="B after pt_clear_image")
        for a, b in zip(kept, pt.svgf_history()):
            assert a.tobytes() == b.tobytes()
        assert (m.cur["N"][has] == 9).all() and (m.cur["N"][~has] == 1).all()
        view(pt, cam_a, depth)
        trace(pt, 1, 1)
        pair.call(1, cam_a, g_a, 5, temp=(5, 0.1, 0.1), what="back at A, a cap that bites")
        lengths = set(np.unique(m.hn).tolist())                # none / B's own sample / B's 1 + A's 8, capped at 5
        assert lengths <= {0.0, 1.0, 5.0} and {0.0, 5.0} <= lengths, lengths
        view(pt, cam_c, depth)
        trace(pt, 1, 2)
        pair.call(2, cam_c, g_c, 1, temp=(1, 0.1, 0.1), what="C, max_history 1")
        assert set(np.unique(m.hn).tolist()) == {0.0, 1.0} and (m.cur["N"].max() == 3)
        view(pt, cam_b, depth)
        trace(pt, 1, 1)
        pair.call(1, cam_b, g_b, 1, temp=(0, 0.1, 0.1), what="B, max_history 0")
        assert (m.q >= 0).any() and not m.hn.any()
        view(pt, cam_z, depth)
        trace(pt, 1, 1)
        pair.call(1, cam_z, g_z, 5, what="a camera that sees nothing")
        assert not m.hn.any() and not m.var0.any()
        view(pt, cam_a, depth)
        trace(pt, 1, 1)
        pair.call(1, cam_a, g_a, 0, what="A after the jump")
        assert not m.hn.any()                                   # the old view's first hits are all misses
        assert counts(pt)[:4] == (6, 9, 9, 7)
    finally:
        pt.pathtraceFree()


def test_a_small_move_leaves_waves_with_and_without_short_histories(pt, po, scenes, launch_plan):
    """130 x 9 after 8 spp and a small move, 1 spp: a wave is 64 consecutive pixels of a row -- some have history everywhere (N' = 9:
    they leave k_svgf_spatial before their first tap), some have pixels without (disocclusions, the frame's edge).  From inside
    the box (model: 12 of 27 waves, 4 of 9 workgroups have a short history)."""
    s = scenes["cornell"]
    w, h = 130, 9
    cam_a = inside(_resized(s["camera"], w, h))
    cam_b = moved(cam_a, (0.05, 0.02, 0.0))
    g_a, g_b = gbuffer(po, s, cam_a), gbuffer(po, s, cam_b)
    init(pt, s, cam_a)
    try:
        pair = Pair(pt, w, h, s["materials"])
        trace(pt, 1, 8)
        pair.call(8, cam_a, g_a, 5, what="A")
        view(pt, cam_b, s["depth"])
        trace(pt, 1, 1)
        pair.call(1, cam_b, g_b, 5, what="B")
        low = (pair.model.cur["N"] < 4).reshape(h, w)
        waves = [bool(low[y, x:x + 64].any()) for y in range(h) for x in range(0, w, 64)]
        groups = [bool(low[y:y + 4, x:x + 64].any()) for y in range(0, h, 4) for x in range(0, w, 64)]
        print("waves with a short history: %d of %d; workgroups: %d of %d" % (sum(waves), len(waves), sum(groups), len(groups)))
        assert 0 < sum(waves) < len(waves) and 0 < sum(groups) < len(groups)
        vt = sm.temporal_variance(*[pair.model.cur[k] for k in ("U1", "U2", "N")])
        assert (bits(pair.model.var0)[~low.reshape(-1)] == bits(vt)[~low.reshape(-1)]).all()
    finally:
        pt.pathtraceFree()


def test_mirror_and_glass_get_no_history_and_take_the_spatial_estimate(pt, po, scenes, launch_plan):
    s = scenes["cornell_glass"]
    w, h = 31, 29
    cam_a = _resized(s["camera"], w, h)
    cam_b = moved(cam_a, MOVE)
    g_a, g_b = gbuffer(po, s, cam_a), gbuffer(po, s, cam_b)
    init(pt, s, cam_a)
    try:
        pair = Pair(pt, w, h, s["materials"])
        trace(pt, 1, 8)
        pair.call(8, cam_a, g_a, 5, what="A")
        view(pt, cam_b, s["depth"])
        trace(pt, 1, 2)
        pair.call(2, cam_b, g_b, 5, what="B")
        mat, mats = g_b["materialId"], s["materials"]
        specular = (mat >= 0) & ((mats["hasReflective"][np.clip(mat, 0, None)] != 0) | (mats["hasRefractive"][np.clip(mat, 0, None)] != 0))
        assert specular.sum() >= 8 and not pair.model.hn[specular].any() and (pair.model.cur["N"][specular] == 2).all()
        diffuse = (mat >= 0) & ~specular
        assert (pair.model.hn[diffuse] > 0).mean() > 0.5
    finally:
        pt.pathtraceFree()


def test_a_frame_whose_every_pixel_misses(pt, po, scenes, launch_plan):
    s = scenes["cornell"]
    w, h = 31, 29
    cam_a = away(_resized(s["camera"], w, h))
    cam_b = moved(cam_a, MOVE)
    g_a, g_b = gbuffer(po, s, cam_a), gbuffer(po, s, cam_b)
    assert not (g_a["t"] > 0).any() and not (g_b["t"] > 0).any()
    init(pt, s, cam_a)
    try:
        pair = Pair(pt, w, h, s["materials"])
        trace(pt, 1, 2)
        assert not pt.get_image(w * h).any()
        pair.call(2, cam_a, g_a, 5, what="A")
        view(pt, cam_b, s["depth"])
        trace(pt, 1, 1)
        pair.call(1, cam_b, g_b, 2, what="B")
        assert not pair.model.hn.any() and not pair.model.var0.any()
    finally:
        pt.pathtraceFree()


# ---- 4. beside the other filters ----------------------------------------------------------------------------------------------
def test_colour_and_lengths_are_those_of_a_parallel_temporal_sequence(pt, po, scenes, launch_plan):
    s = scenes["cornell"]
    w, h = 31, 29
    n = w * h
    cam_a = _resized(s["camera"], w, h)
    cams = [cam_a, moved(cam_a, MOVE), moved(cam_a, MOVE), cam_a]
    init(pt, s, cam_a)
    try:
        for k, (cam, iters) in enumerate(zip(cams, (8, 1, 3, 2))):
            if k in (1, 3):
                view(pt, cam, s["depth"])
            trace(pt, 1 if k != 2 else 2, iters)
            temp = pt.TemporalParams(10, 0.1, 0.1)
            t = pt.denoise_temporal(iters, pt.DenoiseParams(0, 1.0, 0.35, 0.5), temp)
            v = pt.denoise_svgf(iters, pt.VarianceParams(0, *SIG), temp, 4)
            same(v, t, "call %d: C" % k)                        # levels = 0: both return c0
            hc, _, _, hn = pt.svgf_history()
            thc, thn = pt.history()
            same(hc, thc, "call %d: Hc" % k)
            same(hn, thn, "call %d: Hn" % k)
        assert (hn == 10).any() and (hn == 0).any()
    finally:
        pt.pathtraceFree()


def test_the_four_filters_interleaved_across_moves_do_not_disturb_each_other(pt, po, scenes, launch_plan):
    s = scenes["cornell"]
    w, h = 31, 29
    cam_a = _resized(s["camera"], w, h)
    cam_b = moved(cam_a, MOVE)
    stages = ((cam_a, 4, "dtvs"), (cam_b, 1, "svtd"), (cam_b, 3, "tsdv"), (cam_a, 1, "vdst"))

    def run(which):
        out = {k: [] for k in "dtvs"}
        init(pt, s, cam_a)
        try:
            cur = cam_a
            for cam, iters, order in stages:
                if cam is not cur:
                    view(pt, cam, s["depth"])
                    cur = cam
                    trace(pt, 1, iters)
                else:
                    trace(pt, 1 if iters == 4 else 2, iters)
                for f in order:
                    if f not in which:
                        continue
                    if f == "d":
                        out[f].append(pt.denoise(iters, 3, 1.0, 0.35, 0.5))
                    elif f == "t":
                        out[f].append(pt.denoise_temporal(iters, pt.DenoiseParams(3, 1.0, 0.35, 0.5)))
                    elif f == "v":
                        out[f].append(pt.denoise_variance(iters, 3, *SIG))
                    else:
                        out[f].append(pt.denoise_svgf(iters, pt.VarianceParams(3, *SIG)))
                if "t" in which:
                    out["t"] += list(pt.history())              # pt_history and pt_variance report their own calls
                if "v" in which:
                    out["v"].append(pt.variance())
                if "s" in which:
                    out["s"] += list(pt.svgf_history()) + [pt.svgf_variance()]
            return out
        finally:
            pt.pathtraceFree()

    together = run("dtvs")
    for f in "dtvs":
        alone = run(f)[f]
        assert len(alone) == len(together[f]) > 0
        for k, (a, b) in enumerate(zip(together[f], alone)):
            assert a.tobytes() == b.tobytes(), "filter %s, result %d" % (f, k)


def test_session_is_unchanged_by_the_call(pt, scenes, launch_plan):
    s = scenes["cornell"]
    w = h = 64
    n = w * h
    cam = _resized(s["camera"], w, h)

    def stats():
        st = pt.get_stats()
        return (st.bounces, st.rays, list(st.live), st.total_rays, st.total_iterations)

    def first_bounce_of(it):
        pt.trace_begin(it, 1)
        pt.trace_bounce(0)
        paths, live = pt.export_paths(n)
        pt.trace_end()
        return paths.tobytes(), live

    def run(filtered):
        init(pt, s, cam)
        try:
            pt.trace_batch(1, 4, None)
            pt.trace_batch_async(5, 4)                         # still in flight when the filter is asked for
            if filtered:
                pt.denoise_svgf(8)
            image, rays, counters, moments, st = pt.get_image(n).copy(), pt.total_rays(), pt.counters(), pt.get_moments(), stats()
            if filtered:
                pt.denoise_svgf(8, pt.VarianceParams(3, *SIG))
                pt.svgf_history()
                pt.svgf_variance()
                pt.svgf_reset()
                pt.denoise_svgf(8, pt.VarianceParams(0, *SIG), spatial_below=0)
                assert pt.get_image(n).tobytes() == image.tobytes()
                assert pt.total_rays() == rays and pt.counters() == counters and stats() == st
                for a, b in zip(moments, pt.get_moments()):
                    assert a.tobytes() == b.tobytes()
            pt.trace_batch(9, 4, None)                         # and tracing goes on as if nothing had happened
            return pt.get_image(n).copy(), pt.get_moments(), first_bounce_of(13)
        finally:
            pt.pathtraceFree()

    a, b = run(True), run(False)
    assert a[0].tobytes() == b[0].tobytes() and a[2] == b[2]
    for x, y in zip(a[1], b[1]):
        assert x.tobytes() == y.tobytes()


# ---- 5. life time, memory ---------------------------------------------------------------------------------------------------
def test_reset_free_and_reinit_end_the_history(pt, po, scenes, launch_plan):
    s = scenes["cornell"]
    w, h = 31, 29
    cam_a = _resized(s["camera"], w, h)
    cam_b = moved(cam_a, MOVE)
    g_b = gbuffer(po, s, cam_b)
    init(pt, s, cam_a)
    try:
        assert pt.library().pt_svgf_reset() == 0               # nothing to forget: fine
        trace(pt, 1, 4)
        pt.denoise_svgf(4)
        view(pt, cam_b, s["depth"])
        trace(pt, 1, 2)
        pt.denoise_svgf(2)
        assert (pt.svgf_history()[3] > 0).any()
        pt.svgf_reset()
        for plane in pt.svgf_history():
            assert not plane.any()
        pair = Pair(pt, w, h, s["materials"])                   # after the reset the call is a session's first
        pair.call(2, cam_b, g_b, 3, what="after the reset")
        assert not pair.model.hn.any()
    finally:
        pt.pathtraceFree()
    init(pt, s, cam_a)                                          # a new session starts without history
    try:
        with pytest.raises(pt.PtError, match="pt_svgf_history"):
            pt.svgf_history()
        view(pt, cam_b, s["depth"])
        trace(pt, 1, 2)
        pair = Pair(pt, w, h, s["materials"])
        pair.call(2, cam_b, g_b, 3, what="first call of a new session")
        assert counts(pt)[:4] == (0, 1, 1, 1)
    finally:
        pt.pathtraceFree()


def test_twenty_calls_between_two_cameras_allocate_nothing(pt, scenes, launch_plan):
    s = scenes["cornell"]
    w, h = 64, 16
    cam_a = _resized(s["camera"], w, h)
    cam_b = moved(cam_a, MOVE)
    prm = pt.VarianceParams(2, *SIG)
    init(pt, s, cam_a)
    try:
        trace(pt, 1, 4)
        pt.denoise_svgf(4, prm)
        pt.set_camera(cam_b, s["depth"])
        pt.denoise_svgf(4, prm)                                # the second call, the first with a reprojection: everything is allocated
        free = free_memory()
        for k in range(20):
            pt.set_camera(cam_a if k % 2 == 0 else cam_b, s["depth"])
            assert np.isfinite(pt.denoise_svgf(4, prm)).all()
        assert free_memory() == free
        assert counts(pt) == (21, 22, 22, 22, 44, 0)
    finally:
        pt.pathtraceFree()


# ---- 6. random hostile scenes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1029, 1000, 1002, 1028])
def test_random_scenes_across_a_move_and_a_jump(pt, po, launch_plan, seed):
    """the filters' group of test_gpu_random_scenes.py: the seed's camera, a move of (0.3, 0.2, 0), the next seed's perturbed camera
    (positions behind the old camera and off its frame), two fresh iterations each"""
    w, h = rs.W, rs.H
    assert (w, h) == (40, 26) and seed in rs.FILTER_SEEDS
    geoms, mats, cam, depth = rs.scene(pt, seed, w, h)
    cams = [cam, rs.moved(cam, rs.MOVE), rs.scene(pt, rs.next_seed(rs.FILTER_SEEDS, seed), w, h)[2]]
    pt.pathtraceInit(pt.Scene(geoms, mats, cam, depth), flags=pt.PT_COMPACT | pt.PT_MOMENTS, max_batch=2, pin_image=False)
    try:
        pair = Pair(pt, w, h, mats)
        for k, c in enumerate(cams):
            if k:
                view(pt, c, depth)
            pt.trace_batch(1, 2, None)
            g = rs.first_hits(po, pt, seed, w, h, None if k == 0 else c)
            pair.call(2, c, g, (5, 1, 5)[k], sig=(4.0,) + tuple(rs.SIGMAS[1:]), what=("own camera", "moved camera", "camera of the next seed")[k])
    finally:
        pt.pathtraceFree()


# ---- 7. the headless host -------------------------------------------------------------------------------------------------------
def test_ptbench_svgf_with_and_without_a_move(pt, po, scenes, tmp_path, launch_plan):
    from PIL import Image
    txt = open(os.path.join(ROOT, "scenes", "cornell.txt")).read().replace("RES         800 800", "RES         64 64")
    scene_file = tmp_path / "cornell64.txt"
    scene_file.write_text(txt)
    exe = pt.build_ptbench()
    s = scenes["cornell_64"]
    w = h = 64

    def render(cam, iters):
        tr = po.Tracer(s["geoms"], s["materials"], cam, s["depth"])
        acc = np.zeros((w * h, 3), dtype=np.float32)
        m1, m2 = np.zeros(w * h, np.float32), np.zeros(w * h, np.float32)
        for it in range(1, iters + 1):
            tr.image[:] = 0
            tr.iterate(it)
            acc = (acc + tr.image).astype(np.float32)
            m1, m2 = vm.accumulate(m1, m2, tr.image)
        return acc, m1, m2

    def picture(path):
        return np.asarray(Image.open(str(path)).convert("RGB"), dtype=np.uint8).tobytes()

    first = render(s["camera"], 8)
    g_a = am.gbuffer_from_oracle(po, s["camera"], s["depth"], s["geoms"])
    p = subprocess.run([exe, str(scene_file), "--iters", "8", "--batch", "4", "--out", str(tmp_path / "r"), "--svgf", "5,4.0,0.35,0.5,3"],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "svgf: 5 levels" in p.stdout and "spatial below 3, max_history 64" in p.stdout
    model = sm.Svgf(w, h, s["materials"])
    want = model.call(*first, 8, s["camera"], g_a, 5, *SIG, spatial_below=3)
    assert picture(tmp_path / "r.8samp.svgf.png") == pt.image_to_rgb8(want, w, h, 1.0).tobytes()
    # with --move: the moved view filtered with the history of the first view; --temporal's values are the history's
    cam_b = moved(s["camera"], MOVE)
    g_b = am.gbuffer_from_oracle(po, cam_b, s["depth"], s["geoms"])
    second = render(cam_b, 2)
    p = subprocess.run([exe, str(scene_file), "--iters", "8", "--batch", "4", "--out", str(tmp_path / "m"), "--denoise", "5,4.0,0.35,0.5",
                        "--svgf", "5,4.0,0.35,0.5", "--move", "0.3,0.2,0,2", "--temporal", "6,0.1,0.1"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "spatial below 4, max_history 6" in p.stdout and "svgf, moved view" in p.stdout
    model = sm.Svgf(w, h, s["materials"])
    want_a = model.call(*first, 8, s["camera"], g_a, 5, *SIG, max_history=6, spatial_below=4)
    want_b = model.call(*second, 2, cam_b, g_b, 5, *SIG, max_history=6, spatial_below=4)
    assert (model.hn == 6).any()
    assert picture(tmp_path / "m.8samp.svgf.png") == pt.image_to_rgb8(want_a, w, h, 1.0).tobytes()
    assert picture(tmp_path / "m.moved.2samp.svgf.png") == pt.image_to_rgb8(want_b, w, h, 1.0).tobytes()
    p = subprocess.run([exe, str(scene_file), "--iters", "2", "--out", str(tmp_path / "bad"), "--svgf", "5,4,0.35,0.5,-1"],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode != 0 and "spatial_below" in p.stderr


# ---- 8. errors (LAST: the only sessions of this module that hold a tile of a frame are opened here, to be refused) ---------------------
def test_every_refusal(pt, scenes, launch_plan):
    s = scenes["cornell"]
    w = h = 31
    n = w * h
    cam = _resized(s["camera"], w, h)
    L = pt.library()
    buf = np.zeros(n, dtype=np.float32)

    def refused(word, levels=5, sl=4.0, sn=0.35, sp=0.5, it=4, null=False, cap=64, tp=0.1, tn=0.1, tnull=False, below=4):
        prm, tmp = pt.VarianceParams(levels, sl, sn, sp), pt.TemporalParams(cap, tp, tn)
        rc = L.pt_denoise_svgf(None if null else C.byref(prm), None if tnull else C.byref(tmp), below, it, None, None)
        assert rc == -1, (word, levels, sl, sn, sp, it, cap, tp, tn, below)
        assert word.encode() in L.pt_last_error() and L.pt_last_error().startswith(b"pt_denoise_svgf"), L.pt_last_error()

    def the_others(word, reset_too=True):
        for name, call in (("pt_svgf_history", lambda: L.pt_svgf_history(None, buf.ctypes.data, None, None)),
                           ("pt_svgf_variance", lambda: L.pt_svgf_variance(buf.ctypes.data)), ("pt_svgf_reset", L.pt_svgf_reset)):
            if name == "pt_svgf_reset" and not reset_too:
                continue
            assert call() == -1 and L.pt_last_error().startswith(name.encode()) and word.encode() in L.pt_last_error(), L.pt_last_error()

    pt.pathtraceFree()
    refused("not initialised")
    the_others("not initialised")
    init(pt, s, cam, moments=False)                            # a session without the flag
    try:
        pt.trace_batch(1, 2, None)
        refused("PT_MOMENTS")
        the_others("no pt_denoise_svgf call", reset_too=False)
        assert L.pt_svgf_reset() == 0
    finally:
        pt.pathtraceFree()
    init(pt, s, cam)
    try:
        pt.trace_batch(1, 2, None)
        the_others("no pt_denoise_svgf call", reset_too=False)
        refused("params", null=True)
        refused("levels", levels=-1)
        refused("levels", levels=11)
        for name, key in (("sigma_luminance", "sl"), ("sigma_normal", "sn"), ("sigma_position", "sp"), ("position_tolerance", "tp"),
                          ("normal_tolerance", "tn")):
            for bad in (0.0, -1.0, float("nan"), float("inf"), 1e-33 if key == "sl" else 1e-30):
                refused(name, **{key: bad})
        refused("iter", it=0)
        refused("temporal", tnull=True)
        refused("max_history", cap=-1)
        refused("max_history", cap=(1 << 20) + 1)
        refused("spatial_below", below=-1)
        refused("spatial_below", below=(1 << 20) + 1)
        # the order: pt_denoise_variance's refusals, then the temporal parameters', then spatial_below
        refused("levels", levels=11, cap=-1, below=-1)
        refused("iter", it=0, tnull=True, below=-1)
        refused("max_history", cap=-1, below=-1)
        the_others("no pt_denoise_svgf call", reset_too=False)  # a refused call is no call
        got = pt.denoise_svgf(2, pt.VarianceParams(10, 2e-32, 0.35, 0.5), pt.TemporalParams(1 << 20, 2e-19, 2e-19), 1 << 20)
        assert got.shape == (n, 3)
        assert L.pt_svgf_history(None, None, None, None) == 0 and L.pt_svgf_variance(None) == 0
    finally:
        pt.pathtraceFree()
    for kw in (dict(tile=(0, 2, 8)), dict(devices=[0, 0])):    # sessions that hold a tile: pt_init refuses the flag, the calls the tile
        pt.pathtraceInit(pt.Scene(s["geoms"], s["materials"], cam, s["depth"]), flags=pt.PT_COMPACT, max_batch=4, pin_image=False, **kw)
        try:
            refused("tile")
            the_others("tile")
        finally:
            pt.pathtraceFree()
