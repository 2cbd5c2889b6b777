"""GPU: pt_gbuffer / pt_denoise (include/ptmi355.h).  The G-buffer equals the oracle's first hits bit for
bit, the filter equals tests/atrous_model.py bit for bit on every pixel, neither call changes anything in the session
(PT_LOOKAHEAD windows included), bad arguments and sessions that hold a tile are refused, and ptbench --denoise writes the
model's picture.  Under both launch plans."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import __graft_entry__ as ge  # noqa: E402,F401
import atrous_model as am  # noqa: E402
from gpu_common import pt, launch_plan, bits, _resized  # noqa: E402,F401

pytestmark = pytest.mark.gpu

DEFAULT = (1.0, 0.35, 0.5)


def launches(pt):
    """(k_gbuffer, k_atrous, k_denoise_mean) launches since pt_init"""
    out = (C.c_uint64 * 3)()
    assert pt.library().ptdbg_denoise(out) == 0
    return tuple(int(v) for v in out)


def read_device(ptr, nbytes):
    """hipMemcpy device -> host through the HIP runtime this process already holds"""
    path = None
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            path = line.split()[-1]
            break
    assert path, "no HIP runtime loaded"
    hip = C.CDLL(path)
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    buf = np.zeros(nbytes, dtype=np.uint8)
    assert hip.hipMemcpy(buf.ctypes.data, ptr, nbytes, 2) == 0          # hipMemcpyDeviceToHost
    return buf


def assert_gbuffer_equal(got, want):
    assert (bits(got["t"]) == bits(want["t"])).all(), "t"
    assert (bits(got["normal"]) == bits(want["normal"])).all(), "normal"
    assert (bits(got["position"]) == bits(want["position"])).all(), "position"
    hit = want["t"] > 0
    assert (got["materialId"][hit] == want["materialId"][hit]).all() and (got["materialId"][~hit] == -1).all(), "materialId"
    assert 0 < int(hit.sum()) < len(hit)


def mesh_scene(pt, s):
    tris = pt.meshes.uv_sphere(center=(1.5, 3.0, 1.0), radius=1.5, n_lat=24, n_lon=48)          # 2208 triangles
    return pt.meshes.add_mesh(s["geoms"], tris, material_id=2)


# ---- 1. the G-buffer, bit for bit against the oracle ------------------------------------------------------------------
@pytest.mark.parametrize("case", ["cornell", "cornell_glass", "lamp_ball", "mesh loop", "mesh bvh"])
def test_gbuffer_equals_the_oracle(pt, po, scenes, launch_plan, case):
    flags = pt.PT_COMPACT
    tris = meshes = None
    if case.startswith("mesh"):
        s = scenes["cornell"]
        cam = _resized(s["camera"], 256, 192)
        geoms, tris, meshes = mesh_scene(pt, s)
        if case == "mesh bvh":
            flags |= pt.PT_MESH_BVH
    else:
        s = scenes[case]
        geoms = s["geoms"]
        cam = _resized(s["camera"], 1280, 720) if case == "cornell_glass" else s["camera"]
    scene = pt.Scene(geoms, s["materials"], cam, s["depth"], triangles=tris, meshes=meshes)
    pt.pathtraceInit(scene, flags=flags)
    try:
        got = pt.gbuffer()
        want = am.gbuffer_from_oracle(po, cam, s["depth"], geoms.view(po.GEOM_DT) if tris is not None else geoms,
                                      None if tris is None else tris.view(po.TRI_DT), None if meshes is None else meshes.view(po.MESH_DT))
        assert_gbuffer_equal(got, want)
        assert launches(pt)[0] == 1
        again = pt.gbuffer()                                   # kept: the camera has not changed
        assert launches(pt)[0] == 1
        for k in got:
            assert got[k].tobytes() == again[k].tobytes()
    finally:
        pt.pathtraceFree()


def test_gbuffer_ignores_jitter_and_lens_and_follows_the_camera(pt, po, scenes, launch_plan):
    s = scenes["cornell"]
    cam = _resized(s["camera"], 320, 200)
    scene = pt.Scene(s["geoms"], s["materials"], cam, s["depth"])
    pt.pathtraceInit(scene, flags=pt.PT_COMPACT)
    plain = pt.gbuffer()
    pt.pathtraceFree()
    pt.pathtraceInit(scene, flags=pt.PT_COMPACT | pt.PT_AA_JITTER, lens=(0.2, 9.0))
    try:
        pt.trace_batch(1, 1, None)
        got = pt.gbuffer()
        for k in plain:
            assert got[k].tobytes() == plain[k].tobytes(), k
        assert_gbuffer_equal(got, am.gbuffer_from_oracle(po, cam, s["depth"], s["geoms"]))
        moved = cam.copy()
        moved["position"][0][0] += 0.75
        moved["position"][0][1] -= 0.5
        pt.set_camera(moved, s["depth"])
        n0 = launches(pt)[0]
        got = pt.gbuffer()
        assert launches(pt)[0] == n0 + 1
        assert_gbuffer_equal(got, am.gbuffer_from_oracle(po, moved, s["depth"], s["geoms"]))
        pt.set_camera(moved, s["depth"])                       # the same camera again: nothing is recomputed
        pt.gbuffer()
        assert launches(pt)[0] == n0 + 1
    finally:
        pt.pathtraceFree()


# ---- 2. the filter, bit for bit against the model ---------------------------------------------------------------------
def check_filter(pt, w, h, iters, g, image_sum, levels, sig):
    """every level count in `levels` (ascending) with sigmas `sig`: host floats, RGBA bytes and the device plane"""
    n = w * h
    nrm, pos = g["normal"].reshape(h, w, 3), g["position"].reshape(h, w, 3)
    c = (image_sum.reshape(h, w, 3) / np.float32(iters)).astype(np.float32)
    done = 0
    for lv in levels:
        while done < lv:
            c = am.level(c, nrm, pos, 1 << done, np.float32(sig[0]) * np.float32(2.0 ** -done), sig[1], sig[2])
            done += 1
        got, px = pt.denoise(iters, lv, *sig, rgba=True)
        want = c.reshape(n, 3)
        assert np.isfinite(want).all()
        diff = bits(got) != bits(want)
        assert not diff.any(), "levels %d, sigmas %r: %d of %d floats differ" % (lv, sig, int(diff.sum()), diff.size)
        assert px.tobytes() == am.rgba8(want).tobytes(), "RGBA, levels %d" % lv
        dev = read_device(pt.denoised_device_ptr(), n * 12).view(np.float32).reshape(n, 3)
        assert (bits(dev) == bits(want)).all(), "device plane, levels %d" % lv
        only = pt.denoise(iters, lv, *sig)                     # without the RGBA form
        assert only.tobytes() == got.tobytes()


def test_filter_equals_the_model_cornell_800(pt, po, scenes, launch_plan):
    s = scenes["cornell"]
    w = h = 800
    scene = pt.Scene(s["geoms"], s["materials"], s["camera"], s["depth"])
    pt.pathtraceInit(scene, flags=pt.PT_COMPACT, max_batch=16)
    try:
        img = np.zeros((w * h, 3), dtype=np.float32)
        pt.trace_batch(1, 16, img)
        g = pt.gbuffer()
        assert_gbuffer_equal(g, am.gbuffer_from_oracle(po, s["camera"], s["depth"], s["geoms"]))
        before = launches(pt)
        check_filter(pt, w, h, 16, g, img, [0, 1, 2, 3, 4, 5], DEFAULT)
        # per call: exactly `levels` filter launches (levels = 0: the mean kernel), and no G-buffer launch with the camera unchanged
        after = launches(pt)
        assert after[0] == before[0] and after[1] - before[1] == 2 * (1 + 2 + 3 + 4 + 5) and after[2] - before[2] == 2
        check_filter(pt, w, h, 16, g, img, [5], (0.45, 0.35, 0.2))
        check_filter(pt, w, h, 16, g, img, [5], (4.0, 0.35, 1.0))
    finally:
        pt.pathtraceFree()


def test_filter_equals_the_model_glass_1280x720(pt, po, scenes, launch_plan):
    s = scenes["cornell_glass"]
    w, h = 1280, 720
    cam = _resized(s["camera"], w, h)
    scene = pt.Scene(s["geoms"], s["materials"], cam, s["depth"])
    pt.pathtraceInit(scene, flags=pt.PT_COMPACT, max_batch=16)
    try:
        img = np.zeros((w * h, 3), dtype=np.float32)
        pt.trace_batch(1, 16, img)
        g = am.gbuffer_from_oracle(po, cam, s["depth"], s["geoms"])
        check_filter(pt, w, h, 16, g, img, [5], DEFAULT)
        assert launches(pt)[0] == 1                            # the first pt_denoise computed the G-buffer itself, once
    finally:
        pt.pathtraceFree()


def test_filter_equals_the_model_97x61_seven_levels(pt, po, scenes, launch_plan):
    """steps 32 and 64 put most or all off-centre taps outside a 97 x 61 image"""
    s = scenes["cornell"]
    w, h = 97, 61
    cam = _resized(s["camera"], w, h)
    scene = pt.Scene(s["geoms"], s["materials"], cam, s["depth"])
    pt.pathtraceInit(scene, flags=pt.PT_COMPACT, max_batch=16)
    try:
        img = np.zeros((w * h, 3), dtype=np.float32)
        pt.trace_batch(1, 16, img)
        g = am.gbuffer_from_oracle(po, cam, s["depth"], s["geoms"])
        check_filter(pt, w, h, 16, g, img, [6, 7], DEFAULT)
    finally:
        pt.pathtraceFree()


# ---- 3. the session is left alone --------------------------------------------------------------------------------------
def test_session_is_unchanged_by_gbuffer_and_denoise(pt, scenes, launch_plan):
    s = scenes["cornell"]
    cam = _resized(s["camera"], 256, 256)
    n = 256 * 256
    scene = pt.Scene(s["geoms"], s["materials"], cam, s["depth"])
    pt.pathtraceInit(scene, flags=pt.PT_COMPACT, max_batch=4)
    try:
        pt.trace_batch(1, 4, None)
        pt.trace_batch_async(5, 4)                             # still in flight when the filter is asked for
        pt.denoise(8)
        image, rays, counters = pt.get_image(n).copy(), pt.total_rays(), pt.counters()
        st = pt.get_stats()
        stats = (st.bounces, st.rays, list(st.live), st.total_rays, st.total_iterations)
        pt.gbuffer()
        pt.denoise(8, 3)
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


def test_lookahead_windows_survive_the_filter(pt, po, scenes, launch_plan):
    """PT_PIN_IMAGE | PT_HOST_SPARSE | PT_LOOKAHEAD, max_batch 16, iterations 1..40, a pt_denoise after calls 1, 7, 16 and 17:
    the host image after EVERY call is the oracle's running sum, every denoised image is the model's on that sum, and the rays
    served add up to the run without the filter (a discarded window would show as re-traced rays)."""
    s = scenes["cornell"]
    w, h = 400, 300                                            # 1.44 MB of image: page-locked
    cam = _resized(s["camera"], w, h)
    n = w * h
    depth = s["depth"]
    scene = pt.Scene(s["geoms"], s["materials"], cam, depth)
    L = pt.library()
    flags = pt.PT_COMPACT | pt.PT_LOOKAHEAD | pt.PT_PIN_IMAGE | pt.PT_HOST_SPARSE
    g = am.gbuffer_from_oracle(po, cam, depth, s["geoms"])
    nrm, pos = g["normal"].reshape(h, w, 3), g["position"].reshape(h, w, 3)

    def book():
        out = (C.c_uint64 * 4)()
        assert L.ptdbg_lookahead(out) == 0
        return tuple(int(v) for v in out)

    def run(denoise_after):
        buf = np.full((n, 3), -7.0, dtype=np.float32)
        ref = po.Tracer(s["geoms"], s["materials"], cam, depth, flags=po.F_COMPACT, trig=po.TRIG_SHARED)
        pt.pathtraceInit(scene, flags=flags, max_batch=16, pin_image=False)
        try:
            served = 0
            for it in range(1, 41):
                assert L.pt_trace(None, 0, it, buf.ctypes.data) == 0, L.pt_last_error()
                ref.iterate(it, threads=8)
                assert (bits(buf) == bits(ref.image)).all(), "host image after iteration %d" % it
                served += pt.get_stats().rays
                if it in denoise_after:
                    b0 = book()
                    got = pt.denoise(it, 4)
                    want = am.denoise(ref.image.reshape(h, w, 3), it, nrm, pos, 4, *DEFAULT).reshape(n, 3)
                    assert (bits(got) == bits(want)).all(), "denoised image after iteration %d" % it
                    assert book() == b0                        # no window enqueued, missed or discarded by the filter
                    assert (bits(buf) == bits(ref.image)).all()
                    assert (bits(pt.get_image(n)) == bits(ref.image)).all()
            return served, book()[:3], pt.counters()
        finally:
            pt.pathtraceFree()

    plain = run(())
    with_filter = run((1, 7, 16, 17))
    assert with_filter[0] == plain[0]
    assert with_filter[1] == plain[1] and plain[1][2] == 0     # the same windows, none thrown away
    assert with_filter[2][1:] == plain[2][1:]


# ---- 4. errors ---------------------------------------------------------------------------------------------------------
def test_bad_arguments_and_tiled_sessions_are_refused(pt, po, scenes, launch_plan):
    s = scenes["cornell_64"]
    scene = pt.Scene(s["geoms"], s["materials"], s["camera"], s["depth"])
    L = pt.library()
    n = 64 * 64

    def refused(word, levels=5, sc=1.0, sn=0.35, sp=0.5, it=4, null=False):
        prm = pt.DenoiseParams(levels, sc, sn, sp)
        assert L.pt_denoise(None if null else C.byref(prm), it, None, None) == -1, (word, levels, sc, sn, sp, it)
        assert word.encode() in L.pt_last_error(), L.pt_last_error()

    pt.pathtraceFree()
    refused("not initialised")
    pt.pathtraceInit(scene, flags=pt.PT_COMPACT, max_batch=4)
    try:
        pt.trace_batch(1, 4, None)
        refused("params", null=True)
        refused("levels", levels=-1)
        refused("levels", levels=11)
        for name, key in (("sigma_color", "sc"), ("sigma_normal", "sn"), ("sigma_position", "sp")):
            for bad in (0.0, -1.0, float("nan"), float("inf"), 1e-30):       # 1e-30: its square is not a normal number
                refused(name, **{key: bad})
        refused("sigma_color", levels=10, sc=1e-17)                # fine at level 0, (1e-17 * 2^-9)^2 is not normal
        refused("iter", it=0)
        refused("iter", it=-3)
        assert pt.denoise(4, 10, 2e-16).shape == (n, 3)            # the smallest that passes: (2e-16 * 2^-9)^2 = 1.5e-37
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
            assert L.pt_gbuffer(None, None, None, None) == -1 and b"tile" in L.pt_last_error()
            assert L.pt_denoised_device_image() is None
            pt.trace_batch(5, 4, None)
            assert pt.get_image(n).tobytes() != before.tobytes()
            if "devices" in kw:
                assert (bits(pt.get_image(n)) == bits(ref.image)).all()
        finally:
            pt.pathtraceFree()


# ---- 5. the headless host ----------------------------------------------------------------------------------------------
def test_ptbench_writes_the_denoised_picture(pt, po, scenes, tmp_path, launch_plan):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    txt = open(os.path.join(root, "scenes", "cornell.txt")).read().replace("RES         800 800", "RES         64 64")
    scene_file = tmp_path / "cornell64.txt"
    scene_file.write_text(txt)
    exe = pt.build_ptbench()
    p = subprocess.run([exe, str(scene_file), "--iters", "16", "--batch", "4", "--out", str(tmp_path / "r"),
                        "--denoise", "5,1.0,0.35,0.5"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "denoise: 5 levels" in p.stdout
    from PIL import Image
    s = scenes["cornell_64"]
    ref = po.Tracer(s["geoms"], s["materials"], s["camera"], s["depth"])
    for it in range(1, 17):
        ref.iterate(it)
    raw = np.asarray(Image.open(str(tmp_path / "r.16samp.png")).convert("RGB"), dtype=np.uint8)
    assert raw.tobytes() == pt.image_to_rgb8(ref.image, 64, 64, 16.0).tobytes()
    g = am.gbuffer_from_oracle(po, s["camera"], s["depth"], s["geoms"])
    want = am.denoise(ref.image.reshape(64, 64, 3), 16, g["normal"].reshape(64, 64, 3), g["position"].reshape(64, 64, 3), 5, *DEFAULT)
    got = np.asarray(Image.open(str(tmp_path / "r.16samp.denoised.png")).convert("RGB"), dtype=np.uint8)
    assert got.tobytes() == pt.image_to_rgb8(want.reshape(-1, 3), 64, 64, 1.0).tobytes()
    # a bad specification is refused by the library, with its message
    p = subprocess.run([exe, str(scene_file), "--iters", "2", "--out", str(tmp_path / "bad"), "--denoise", "11,1,1,1"],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode != 0 and "levels" in p.stderr
