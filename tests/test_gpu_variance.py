"""GPU: PT_MOMENTS and pt_denoise_variance (include/ptmi355.h).  The two moment planes equal
tests/variance_model.py bit for bit after batches, single calls, asynchronous batches on the lanes and the stepping interface, in
every kind of session, while image, statistics and ray counters stay those of the unflagged session; the filter and pt_variance
equal the model bit for bit on every pixel; the filter leaves the session, pt_denoise's results and the temporal history alone;
every refusal is exercised; ptbench --variance writes the model's picture.  Under both launch plans."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import __graft_entry__ as ge  # noqa: E402,F401
import atrous_model as am  # noqa: E402
import glossy_model as gm  # noqa: E402
import variance_model as vm  # noqa: E402
from gpu_common import pt, launch_plan, bits, _resized  # noqa: E402,F401

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIG = (4.0, 0.35, 0.5)
LAST = 14                                                  # iterations a moments session traces (trace_all)
_cache = {}


def same(got, want, what=""):
    bad = bits(got) != bits(want)
    assert not bad.any(), "%s: %d of %d words differ, first at %d" % (what, int(bad.sum()), bad.size, int(np.nonzero(bad.reshape(-1))[0][0]))


def launches(pt):
    """(k_gbuffer, k_atrous, k_denoise_mean, k_atrous_var, k_variance_mean) launches since pt_init"""
    a, b = (C.c_uint64 * 3)(), (C.c_uint64 * 2)()
    assert pt.library().ptdbg_denoise(a) == 0 and pt.library().ptdbg_variance(b) == 0
    return tuple(int(v) for v in a) + tuple(int(v) for v in b)


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


# ---- the sessions and their per-sample colours (computed once per module, never written afterwards) -----------------------
def session_arrays(pt, scenes, case, w, h):
    """(geoms, materials, camera, depth, triangles, meshes, session flags, oracle flags, environment)"""
    s = scenes["cornell"]
    geoms, mats, depth, tris, meshes, env = s["geoms"], s["materials"], s["depth"], None, None, None
    flags, oflags = pt.PT_COMPACT, 1
    cam = s["camera"]
    if case == "plain":
        flags, oflags = 0, 0
    elif case == "sort fused":
        flags |= pt.PT_SORT_MATERIAL
    elif case == "fake":
        flags, oflags = pt.PT_FAKE_SHADER, 4
    elif case in ("mesh loop", "mesh bvh"):
        t = pt.meshes.uv_sphere(center=(1.5, 3.0, 1.0), radius=1.5, n_lat=6, n_lon=10)
        geoms, tris, meshes = pt.meshes.add_mesh(s["geoms"], t, material_id=2)
        if case == "mesh bvh":
            flags |= pt.PT_MESH_BVH
    elif case == "glossy sky":
        ls = pt.load_scene(os.path.join(ROOT, "scenes", "open_sky_glossy.txt"))
        geoms, mats, cam, depth = ls.geoms, ls.materials, ls.camera, ls.traceDepth
        flags |= pt.PT_GLOSSY
        env = np.random.default_rng(4001).uniform(0, 2, (6, 4, 4, 3)).astype(np.float32)
    elif case == "glass":
        s = scenes["cornell_glass"]
        geoms, mats, depth, cam = s["geoms"], s["materials"], s["depth"], s["camera"]
    else:
        assert case == "compact", case
    return geoms, mats, _resized(cam, w, h), depth, tris, meshes, flags, oflags, env


def samples(pt, po, scenes, case, w, h, count=LAST):
    """Per-sample colours of iterations 1 .. count, [n, 3] each: one oracle iteration into a zeroed image (0 + c = c), or the
    feature's own model where the oracle has no such session."""
    key = (case, w, h, count)
    if key not in _cache:
        geoms, mats, cam, depth, tris, meshes, _, oflags, env = session_arrays(pt, scenes, case, w, h)
        out = []
        if env is not None:
            m = gm.Model(po, geoms, mats, cam, depth)
            m.set_environment(env)
            for it in range(1, count + 1):
                pix, col = m.colours(it)
                c = np.zeros((w * h, 3), dtype=np.float32)
                c[pix] = col
                out.append(c)
        else:
            kw = {} if tris is None else dict(tris=tris.view(po.TRI_DT), meshes=meshes.view(po.MESH_DT))
            tr = po.Tracer(geoms.view(po.GEOM_DT) if tris is not None else geoms, mats, cam, depth, flags=oflags, trig=po.TRIG_SHARED, **kw)
            for it in range(1, count + 1):
                tr.image[:] = 0
                tr.iterate(it, threads=0 if case == "fake" else 8)    # (the oracle's threaded form has no fake shader)
                out.append(tr.image.copy())
        sums, m1s, m2s = [], [], []
        acc = np.zeros((w * h, 3), dtype=np.float32)
        m1, m2 = np.zeros(w * h, np.float32), np.zeros(w * h, np.float32)
        for c in out:
            acc = (acc + c).astype(np.float32)
            m1, m2 = vm.accumulate(m1, m2, c)
            sums.append(acc)
            m1s.append(m1)
            m2s.append(m2)
        for a in out + sums + m1s + m2s:
            a.setflags(write=False)
        _cache[key] = (out, sums, m1s, m2s)
    return _cache[key]


def init(pt, scenes, case, w, h, extra=0, moments=True, **kw):
    geoms, mats, cam, depth, tris, meshes, flags, _, env = session_arrays(pt, scenes, case, w, h)
    scene = pt.Scene(geoms, mats, cam, depth, triangles=tris, meshes=meshes) if tris is not None else pt.Scene(geoms, mats, cam, depth)
    kw.setdefault("max_batch", 2)
    kw.setdefault("pin_image", False)
    pt.pathtraceInit(scene, flags=flags | extra | (pt.PT_MOMENTS if moments else 0), **kw)
    if env is not None:
        pt.set_environment(env)
    return depth


def stats_tuple(pt):
    st = pt.get_stats()
    return (st.bounces, st.rays, list(st.live), st.total_rays, st.total_iterations)


def trace_all(pt, case, depth, n, check=None):
    """Iterations 1 .. LAST: a batch of two, one pt_trace, five asynchronous batches, the stepping interface.  Returns what an
    unflagged session must reproduce: (image, statistics) after every stage, and the ray counters at the end."""
    seen = []

    def stage(it, what):
        seen.append((pt.get_image(n).copy(), stats_tuple(pt)))
        if check:
            check(it, what)

    img = np.zeros((n, 3), dtype=np.float32)
    pt.trace_batch(1, 2, img)
    assert img.tobytes() == pt.get_image(n).tobytes()
    stage(2, "a batch of two")
    got = pt.pathtrace(None, 0, 3)
    assert np.asarray(got).tobytes() == pt.get_image(n).tobytes()
    stage(3, "one pt_trace")
    for k in range(5):
        pt.trace_batch_async(4 + 2 * k, 2)
    pt.synchronize()
    stage(13, "five asynchronous batches")
    pt.trace_begin(14, 1)
    for d in range(1 if case == "fake" else depth):
        pt.trace_bounce(d)
    pt.trace_end()
    stage(14, "the stepping interface")
    return seen, pt.total_rays(), pt.counters()


# ---- 1. the moments ----------------------------------------------------------------------------------------------------
CASES = [("compact", 31, 29), ("compact", 130, 9), ("plain", 31, 29), ("sort fused", 31, 29), ("fake", 31, 29), ("mesh loop", 31, 29),
         ("mesh bvh", 31, 29), ("glossy sky", 31, 29)]


@pytest.mark.parametrize("case, w, h", CASES)
def test_moments_equal_the_model_and_the_session_is_the_unflagged_one(pt, po, scenes, launch_plan, case, w, h):
    n = w * h
    _, sums, m1s, m2s = samples(pt, po, scenes, case, w, h)

    def check(it, what):
        same(pt.get_image(n), sums[it - 1], "%s: image" % what)
        m1, m2 = pt.get_moments()
        same(m1, m1s[it - 1], "%s: M1" % what)
        same(m2, m2s[it - 1], "%s: M2" % what)

    depth = init(pt, scenes, case, w, h)
    try:
        m1, m2 = pt.get_moments()
        assert not m1.any() and not m2.any()                   # zeroed by pt_init
        flagged = trace_all(pt, case, depth, n, check)
        assert (m2s[-1] > 0).any()
        pt.clear_image()
        m1, m2 = pt.get_moments()
        assert not m1.any() and not m2.any() and not pt.get_image(n).any()
    finally:
        pt.pathtraceFree()
    init(pt, scenes, case, w, h, moments=False)
    try:
        plain = trace_all(pt, case, depth, n)
    finally:
        pt.pathtraceFree()
    for k, (a, b) in enumerate(zip(flagged[0], plain[0])):
        assert a[0].tobytes() == b[0].tobytes(), "image after stage %d" % k
        assert a[1] == b[1], "pt_stats after stage %d" % k
    assert flagged[1:] == plain[1:]                            # pt_total_rays, pt_get_counters


def test_lookahead_flags_are_given_and_ignored(pt, po, scenes, launch_plan):
    """PT_LOOKAHEAD | PT_PIN_IMAGE | PT_HOST_SPARSE beside PT_MOMENTS: no window is traced, the host image is complete after every
    call and pt_get_stats reports every call's rays."""
    w, h = 31, 29
    n = w * h
    _, sums, m1s, m2s = samples(pt, po, scenes, "compact", w, h)
    L = pt.library()
    buf = np.full((n, 3), -7.0, dtype=np.float32)
    init(pt, scenes, "compact", w, h, extra=pt.PT_LOOKAHEAD | pt.PT_PIN_IMAGE | pt.PT_HOST_SPARSE, max_batch=8)
    try:
        rays = []
        for it in range(1, 9):
            assert L.pt_trace(None, 0, it, buf.ctypes.data) == 0, L.pt_last_error()
            same(buf, sums[it - 1], "host image after iteration %d" % it)
            rays.append(pt.get_stats().rays)
        m1, m2 = pt.get_moments()
        same(m1, m1s[7], "M1")
        same(m2, m2s[7], "M2")
        book = (C.c_uint64 * 4)()
        assert L.ptdbg_lookahead(book) == 0 and tuple(book)[:3] == (0, 0, 0)
        assert min(rays) >= n and sum(rays) == pt.total_rays()
    finally:
        pt.pathtraceFree()


def test_set_image_and_set_moments_resume_bit_for_bit(pt, po, scenes, launch_plan):
    w, h = 31, 29
    n = w * h
    _, sums, m1s, m2s = samples(pt, po, scenes, "compact", w, h)
    init(pt, scenes, "compact", w, h)
    try:
        pt.trace_batch(1, 2, None)
        pt.trace_batch(3, 2, None)
        image, (m1, m2) = pt.get_image(n).copy(), pt.get_moments()
    finally:
        pt.pathtraceFree()
    depth = init(pt, scenes, "compact", w, h)                 # free / re-init: a new session starts from zero
    try:
        assert not pt.get_moments()[0].any()
        pt.set_image(image)
        a, b = pt.get_moments()
        assert not a.any() and not b.any()                     # pt_set_image leaves the moments alone
        pt.set_moments(m1, m2)
        cam = session_arrays(pt, scenes, "compact", w, h)[2]
        pt.set_camera(cam, depth)                              # ... and so does pt_set_camera
        same(pt.get_moments()[0], m1s[3], "M1 after pt_set_moments")
        for it in (5, 7, 9):
            pt.trace_batch(it, 2, None)
        same(pt.get_image(n), sums[9], "image")
        a, b = pt.get_moments()
        same(a, m1s[9], "M1")
        same(b, m2s[9], "M2")
    finally:
        pt.pathtraceFree()


# ---- 2. the filter -------------------------------------------------------------------------------------------------------
def gbuffer_of(pt, po, scenes, case, w, h):
    key = ("g", case, w, h)
    if key not in _cache:
        geoms, _, cam, depth = session_arrays(pt, scenes, case, w, h)[:4]
        _cache[key] = am.gbuffer_from_oracle(po, cam, depth, geoms)
    return _cache[key]


def check_variance_filter(pt, w, h, it, g, image_sum, m1, m2, levels, sig=SIG):
    """every level count in `levels` (ascending): host floats, RGBA bytes, the device plane and pt_variance"""
    n = w * h
    nrm, pos = g["normal"].reshape(h, w, 3), g["position"].reshape(h, w, 3)
    c = (image_sum.reshape(h, w, 3) / np.float32(it)).astype(np.float32)
    v0 = vm.var0(m1, m2, it)
    v = v0.reshape(h, w)
    done = 0
    for lv in levels:
        while done < lv:
            c, v = vm.level(c, v, nrm, pos, 1 << done, *sig)
            done += 1
        before = launches(pt)
        got, px = pt.denoise_variance(it, lv, *sig, rgba=True)
        after = launches(pt)
        assert after[1:3] == before[1:3] and after[3] - before[3] == lv and after[4] - before[4] == (1 if lv == 0 else 0)
        want = c.reshape(n, 3)
        assert np.isfinite(want).all()
        same(got, want, "iter %d, levels %d" % (it, lv))
        assert px.tobytes() == am.rgba8(want).tobytes(), "RGBA, levels %d" % lv
        dev = read_device(pt.denoised_device_ptr(), n * 12).view(np.float32).reshape(n, 3)
        same(dev, want, "device plane, levels %d" % lv)
        same(pt.variance(), v0, "pt_variance, levels %d" % lv)
        assert pt.denoise_variance(it, lv, *sig).tobytes() == got.tobytes()         # without the RGBA form


@pytest.mark.parametrize("case, w, h", [("compact", 31, 29), ("compact", 130, 9), ("compact", 67, 5), ("compact", 64, 16), ("glass", 31, 29)])
def test_filter_equals_the_model(pt, po, scenes, launch_plan, case, w, h):
    n = w * h
    _, sums, m1s, m2s = samples(pt, po, scenes, case, w, h, 16)
    g = gbuffer_of(pt, po, scenes, case, w, h)
    assert 0 < int((g["t"] > 0).sum()) < n
    init(pt, scenes, case, w, h, max_batch=4)
    try:
        done = 0
        for it in (1, 2, 5, 16):
            while done < it:
                step = min(4, it - done)
                pt.trace_batch(done + 1, step, None)
                done += step
            same(pt.get_moments()[1], m2s[it - 1], "M2 after %d" % it)
            check_variance_filter(pt, w, h, it, g, sums[it - 1], m1s[it - 1], m2s[it - 1], [0, 1, 2, 3, 5, 7])
        assert launches(pt)[0] == 1                            # the G-buffer once: the camera never changed
        assert not vm.var0(m1s[0], m2s[0], 1).any()            # iter = 1: exactly 0
        other = (0.5, 0.2, 1.5)
        check_variance_filter(pt, w, h, 16, g, sums[15], m1s[15], m2s[15], [3], other)
    finally:
        pt.pathtraceFree()


def test_filter_on_a_frame_whose_every_pixel_misses(pt, po, scenes, launch_plan):
    w, h = 31, 29
    n = w * h
    geoms, mats, cam, depth = session_arrays(pt, scenes, "compact", w, h)[:4]
    away = cam.copy()
    away["view"][0] = -cam["view"][0]                          # looking out of the open side of the box
    away["right"][0] = -cam["right"][0]
    g = am.gbuffer_from_oracle(po, away, depth, geoms)
    assert not (g["t"] > 0).any()
    pt.pathtraceInit(pt.Scene(geoms, mats, away, depth), flags=pt.PT_COMPACT | pt.PT_MOMENTS, max_batch=2, pin_image=False)
    try:
        pt.trace_batch(1, 2, None)
        image, (m1, m2) = pt.get_image(n), pt.get_moments()
        assert not image.any() and not m1.any() and not m2.any()
        check_variance_filter(pt, w, h, 2, g, image, m1, m2, [0, 2, 5])
    finally:
        pt.pathtraceFree()


# ---- 3. beside the other filters; the session is left alone ------------------------------------------------------------------
def test_interleaving_with_denoise_and_temporal_and_the_albedo_switch(pt, po, scenes, launch_plan):
    w, h = 31, 29
    n = w * h
    _, sums, m1s, m2s = samples(pt, po, scenes, "compact", w, h)
    g = gbuffer_of(pt, po, scenes, "compact", w, h)
    nrm, pos = g["normal"].reshape(h, w, 3), g["position"].reshape(h, w, 3)
    want_v = vm.denoise(sums[3].reshape(h, w, 3), m1s[3].reshape(h, w), m2s[3].reshape(h, w), 4, nrm, pos, 3, *SIG).reshape(n, 3)
    want_d = am.denoise(sums[3].reshape(h, w, 3), 4, nrm, pos, 3, 1.0, 0.35, 0.5).reshape(n, 3)
    init(pt, scenes, "compact", w, h, max_batch=4)
    try:
        pt.trace_batch(1, 4, None)
        temporal = pt.denoise_temporal(4)
        hist = [a.copy() for a in pt.history()]
        v1, p1 = pt.denoise_variance(4, 3, *SIG, rgba=True)
        d, pd = pt.denoise(4, 3, rgba=True)
        same(read_device(pt.denoised_device_ptr(), n * 12).view(np.float32).reshape(n, 3), want_d, "pt_denoise's device plane")
        v2, p2 = pt.denoise_variance(4, 3, *SIG, rgba=True)
        same(read_device(pt.denoised_device_ptr(), n * 12).view(np.float32).reshape(n, 3), want_v, "pt_denoise_variance's device plane")
        d2, pd2 = pt.denoise(4, 3, rgba=True)
        for got in (v1, v2):
            same(got, want_v, "pt_denoise_variance beside pt_denoise")
        for got in (d, d2):
            same(got, want_d, "pt_denoise beside pt_denoise_variance")
        assert p1.tobytes() == p2.tobytes() == am.rgba8(want_v).tobytes() and pd.tobytes() == pd2.tobytes() == am.rgba8(want_d).tobytes()
        for a, b in zip(hist, pt.history()):
            assert a.tobytes() == b.tobytes()                  # the temporal history is untouched ...
        assert pt.denoise_temporal(4).tobytes() == temporal.tobytes()
        pt.set_denoise_albedo(True)                            # ... and the albedo switch changes nothing
        same(pt.denoise_variance(4, 3, *SIG), want_v, "with pt_set_denoise_albedo(1)")
        pt.set_denoise_albedo(False)
    finally:
        pt.pathtraceFree()


def test_session_is_unchanged_by_the_variance_filter(pt, scenes, launch_plan):
    w = h = 64
    n = w * h
    init(pt, scenes, "compact", w, h, max_batch=4)
    try:
        pt.trace_batch(1, 4, None)
        pt.trace_batch_async(5, 4)                             # still in flight when the filter is asked for
        pt.denoise_variance(8)
        image, rays, counters, moments = pt.get_image(n).copy(), pt.total_rays(), pt.counters(), pt.get_moments()
        stats = stats_tuple(pt)
        pt.denoise_variance(8, 3)
        pt.variance()
        assert pt.get_image(n).tobytes() == image.tobytes()
        assert pt.total_rays() == rays and pt.counters() == counters and stats_tuple(pt) == stats
        for a, b in zip(moments, pt.get_moments()):
            assert a.tobytes() == b.tobytes()
        pt.trace_batch(9, 4, None)                             # and tracing goes on as if nothing had happened
        after, after_m = pt.get_image(n).copy(), pt.get_moments()
    finally:
        pt.pathtraceFree()
    init(pt, scenes, "compact", w, h, max_batch=4)
    try:
        for it in (1, 5, 9):
            pt.trace_batch(it, 4, None)
        assert pt.get_image(n).tobytes() == after.tobytes()
        for a, b in zip(after_m, pt.get_moments()):
            assert a.tobytes() == b.tobytes()
    finally:
        pt.pathtraceFree()


# ---- 4. errors -------------------------------------------------------------------------------------------------------------
def test_every_refusal(pt, scenes, launch_plan):
    w = h = 31
    n = w * h
    L = pt.library()
    buf = np.zeros(n, dtype=np.float32)

    def refused(word, levels=5, sl=4.0, sn=0.35, sp=0.5, it=4, null=False):
        prm = pt.VarianceParams(levels, sl, sn, sp)
        assert L.pt_denoise_variance(None if null else C.byref(prm), it, None, None) == -1, (word, levels, sl, sn, sp, it)
        assert word.encode() in L.pt_last_error() and b"pt_denoise_variance" in L.pt_last_error(), L.pt_last_error()

    def all_four(word, moments_word=None):
        refused(word)
        for name, call, wd in (("pt_get_moments", lambda: L.pt_get_moments(buf.ctypes.data, None), moments_word or word),
                               ("pt_set_moments", lambda: L.pt_set_moments(buf.ctypes.data, buf.ctypes.data), moments_word or word),
                               ("pt_variance", lambda: L.pt_variance(None), word)):
            assert call() == -1 and name.encode() in L.pt_last_error() and wd.encode() in L.pt_last_error(), L.pt_last_error()

    pt.pathtraceFree()
    all_four("not initialised")
    init(pt, scenes, "compact", w, h, moments=False)         # a session without the flag
    try:
        pt.trace_batch(1, 2, None)
        all_four("PT_MOMENTS")
    finally:
        pt.pathtraceFree()
    init(pt, scenes, "compact", w, h)
    try:
        pt.trace_batch(1, 2, None)
        assert L.pt_variance(None) == -1 and b"no pt_denoise_variance call" in L.pt_last_error()
        refused("params", null=True)
        refused("levels", levels=-1)
        refused("levels", levels=11)
        for name, key in (("sigma_luminance", "sl"), ("sigma_normal", "sn"), ("sigma_position", "sp")):
            for bad in (0.0, -1.0, float("nan"), float("inf"), 1e-30 if key != "sl" else 1e-33):
                refused(name, **{key: bad})
        refused("iter", it=0)
        refused("iter", it=-3)
        assert pt.denoise_variance(2, 2, 2e-32).shape == (n, 3)        # the smallest that passes: 2e-32 * 2^-20 = 1.9e-38
        assert L.pt_set_moments(None, buf.ctypes.data) == -1 and b"null" in L.pt_last_error()
        assert L.pt_set_moments(buf.ctypes.data, None) == -1 and b"null" in L.pt_last_error()
        assert L.pt_get_moments(None, None) == 0 and L.pt_get_moments(buf.ctypes.data, None) == 0
    finally:
        pt.pathtraceFree()
    for kw in (dict(devices=[0, 0]), dict(tile=(0, 2, 8))):    # pt_init refuses the flag in sessions that hold a tile
        with pytest.raises(pt.PtError, match="PT_MOMENTS"):
            init(pt, scenes, "compact", w, h, **kw)
        pt.pathtraceFree()
        init(pt, scenes, "compact", w, h, moments=False, **kw)
        try:
            all_four("tile", "PT_MOMENTS")                     # (the filters refuse the tile; the moments' calls the missing flag)
        finally:
            pt.pathtraceFree()


# ---- 5. the headless host ---------------------------------------------------------------------------------------------------
def test_ptbench_writes_the_variance_filtered_picture(pt, po, scenes, tmp_path, launch_plan):
    txt = open(os.path.join(ROOT, "scenes", "cornell.txt")).read().replace("RES         800 800", "RES         64 64")
    scene_file = tmp_path / "cornell64.txt"
    scene_file.write_text(txt)
    exe = pt.build_ptbench()
    p = subprocess.run([exe, str(scene_file), "--iters", "16", "--batch", "4", "--out", str(tmp_path / "r"), "--denoise", "5,1.0,0.35,0.5",
                        "--variance", "5,4.0,0.35,0.5"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "variance: 5 levels" in p.stdout and "denoise: 5 levels" in p.stdout
    from PIL import Image
    s = scenes["cornell_64"]
    tr = po.Tracer(s["geoms"], s["materials"], s["camera"], s["depth"])
    acc = np.zeros((64 * 64, 3), dtype=np.float32)
    m1, m2 = np.zeros(64 * 64, np.float32), np.zeros(64 * 64, np.float32)
    for it in range(1, 17):
        tr.image[:] = 0
        tr.iterate(it)
        acc = (acc + tr.image).astype(np.float32)
        m1, m2 = vm.accumulate(m1, m2, tr.image)
    raw = np.asarray(Image.open(str(tmp_path / "r.16samp.png")).convert("RGB"), dtype=np.uint8)
    assert raw.tobytes() == pt.image_to_rgb8(acc, 64, 64, 16.0).tobytes()
    g = am.gbuffer_from_oracle(po, s["camera"], s["depth"], s["geoms"])
    nrm, pos = g["normal"].reshape(64, 64, 3), g["position"].reshape(64, 64, 3)
    want = vm.denoise(acc.reshape(64, 64, 3), m1.reshape(64, 64), m2.reshape(64, 64), 16, nrm, pos, 5, *SIG)
    got = np.asarray(Image.open(str(tmp_path / "r.16samp.variance.png")).convert("RGB"), dtype=np.uint8)
    assert got.tobytes() == pt.image_to_rgb8(want.reshape(-1, 3), 64, 64, 1.0).tobytes()
    plain = am.denoise(acc.reshape(64, 64, 3), 16, nrm, pos, 5, 1.0, 0.35, 0.5)
    got = np.asarray(Image.open(str(tmp_path / "r.16samp.denoised.png")).convert("RGB"), dtype=np.uint8)
    assert got.tobytes() == pt.image_to_rgb8(plain.reshape(-1, 3), 64, 64, 1.0).tobytes()
    p = subprocess.run([exe, str(scene_file), "--iters", "2", "--out", str(tmp_path / "bad"), "--variance", "11,1,1,1"],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode != 0 and "levels" in p.stderr
