"""GPU: first-hit albedo demodulation in the filters (pt_set_denoise_albedo / pt_albedo; include/ptmi355.h).
Everything is compared with tests/albedo_model.py bit for bit on every pixel, under both launch plans: the albedo plane, pt_denoise
and pt_denoise_temporal with the switch on, the state the switch and the plane follow, that the calls leave the session alone
(PT_LOOKAHEAD windows included), the refusals and the headless host.  A filter workgroup is 64 x 4 pixels and the staged halo is 2:
frames of 31 x 29, 64 x 4, 65 x 5, 97 x 61 and 130 x 9 (three workgroup columns, a partial last workgroup row); at most 4 iterations."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import __graft_entry__ as ge  # noqa: E402,F401
import albedo_model as alm  # noqa: E402
import atrous_model as am  # noqa: E402
import direct_model as dm  # noqa: E402
import texture_model as tm  # noqa: E402
from gpu_common import pt, launch_plan, bits, _resized  # noqa: E402,F401

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
DEFAULT = (1.0, 0.35, 0.5)
FRAMES = [(31, 29), (64, 4), (65, 5), (130, 9)]
_cache = {}


def same(got, want, what=""):
    bad = (bits(got) != bits(want)).reshape(len(got), -1).any(axis=-1)
    assert not bad.any(), "%s: %d of %d differ, first %d" % (what, bad.sum(), bad.size, np.nonzero(bad)[0][0])


def launches(pt):
    """(k_gbuffer, k_atrous, k_denoise_mean) launches since pt_init"""
    out = (C.c_uint64 * 3)()
    assert pt.library().ptdbg_denoise(out) == 0
    return tuple(int(v) for v in out)


def random_texture(n, seed=0):
    return np.random.default_rng(1000 * n + seed).uniform(0, 2, (6, n, n, 3)).astype(F32)


def textured(pt):
    if "textured" not in _cache:
        s = pt.load_scene(os.path.join(ROOT, "scenes", "cornell_textured.txt"))
        _cache["textured"] = (s.geoms, s.materials, s.camera, s.traceDepth, dict(s.textures))
    return _cache["textured"]


def bands(pt):
    """Three wide bands that fill the frame: a textured emitter, and two matte materials with the clamp's edge values."""
    mats = np.zeros(3, dtype=pt.MATERIAL_DT)
    mats["color"] = np.array([[1.0, 0.9, 0.8], [0.0, np.nan, 2.0 ** -7], [65.0, 0.5, 2.0 ** -6]], dtype=F32)
    mats["emittance"][0] = 5.0
    geoms = np.concatenate([dm.placed(pt.GEOM_DT, tm.CUBE, k, (0.0, 5.0 + 6.0 * (k - 1), 0.0), (400.0, 6.0, 0.1)) for k in range(3)])
    return geoms, mats


def scene_arrays(pt, scenes, case):
    """(geoms, materials, camera at 800 x 800, depth, triangles, meshes, flags beside PT_COMPACT, textures to set, textures in effect)"""
    g, m, c, d, t = textured(pt)
    if case == "textured":
        return g, m, c, d, None, None, pt.PT_TEXTURES, t, t
    if case == "no PT_TEXTURES":
        return g, m, c, d, None, None, 0, {}, {}
    if case == "flag without a texture":
        return g, m, c, d, None, None, pt.PT_TEXTURES, {}, {}
    if case == "fake shader":                                          # the reference's shader ignores the textures: so does the plane
        return g, m, c, d, None, None, pt.PT_TEXTURES | pt.PT_FAKE_SHADER, t, {}
    if case == "glass":
        s = scenes["cornell_glass"]
        return s["geoms"], s["materials"], s["camera"], s["depth"], None, None, 0, {}, {}
    if case in ("mesh loop", "mesh bvh"):                              # a triangle soup of the matte ball's material: its texture is ignored there
        import mesh_cases
        tris = mesh_cases.soup(pt.TRI_DT, np.random.default_rng(11), n=50)
        geoms, tris, meshes = pt.meshes.add_mesh(g, tris, material_id=6)
        return geoms, m, c, d, tris, meshes, pt.PT_TEXTURES | (pt.PT_MESH_BVH if case == "mesh bvh" else 0), t, t
    if case in ("emitter", "clamp edges"):
        geoms, mats = bands(pt)
        tex = {0: random_texture(4, 8)}
        return geoms, mats, c, d, None, None, pt.PT_TEXTURES, tex, tex
    raise KeyError(case)


def open_session(pt, scenes, case, w, h, **kw):
    geoms, mats, cam, depth, tris, meshes, flags, to_set, tex = scene_arrays(pt, scenes, case)
    cam = _resized(cam, w, h)
    scene = pt.Scene(geoms, mats, cam, depth, triangles=tris, meshes=meshes) if tris is not None else pt.Scene(geoms, mats, cam, depth)
    flags |= kw.pop("flags", 0 if flags & pt.PT_FAKE_SHADER else pt.PT_COMPACT)
    pt.pathtraceInit(scene, flags=flags, **kw)
    for k, t in to_set.items():
        pt.set_texture(k, t)
    return geoms, mats, cam, depth, tris, meshes, tex


def first_hits(po, geoms, cam, depth, tris=None, meshes=None):
    return am.gbuffer_from_oracle(po, cam, depth, np.ascontiguousarray(geoms).view(po.GEOM_DT),
                                  None if tris is None else tris.view(po.TRI_DT), None if meshes is None else meshes.view(po.MESH_DT))


def planes(g, w, h):
    return g["normal"].reshape(h, w, 3), g["position"].reshape(h, w, 3)


def model_on(image, iters, A, g, w, h, levels, sig=DEFAULT):
    nrm, pos = planes(g, w, h)
    return alm.denoise(image.reshape(h, w, 3), iters, A.reshape(h, w, 3), nrm, pos, levels, *sig).reshape(-1, 3)


def model_off(image, iters, g, w, h, levels, sig=DEFAULT):
    nrm, pos = planes(g, w, h)
    return am.denoise(image.reshape(h, w, 3), iters, nrm, pos, levels, *sig).reshape(-1, 3)


# ---- 1. the albedo plane ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["textured", "no PT_TEXTURES", "flag without a texture", "fake shader", "glass", "mesh loop", "mesh bvh",
                                  "emitter", "clamp edges"])
def test_albedo_equals_the_model(pt, po, scenes, launch_plan, case):
    for w, h in FRAMES:
        geoms, mats, cam, depth, tris, meshes, tex = open_session(pt, scenes, case, w, h)
        try:
            got = pt.albedo()
            want = alm.albedo(po, geoms, mats, tex, cam, depth, tris, meshes)
            same(got, want, "%s %d x %d" % (case, w, h))
            assert launches(pt) == (1, 0, 0)
            assert pt.albedo().tobytes() == got.tobytes() and launches(pt)[0] == 1          # kept: nothing changed
            assert pt.library().pt_albedo(None) == 0 and launches(pt)[0] == 1
            # the launch that wrote the plane wrote the G-buffer too: pt_gbuffer finds it made
            g = pt.gbuffer()
            assert launches(pt)[0] == 1
            ref = first_hits(po, geoms, cam, depth, tris, meshes)
            for k in ("t", "normal", "position"):
                assert (bits(g[k]) == bits(ref[k])).all(), k
            mat = ref["materialId"]
            one = bits(F32(1.0))
            if case == "textured" and (w, h) == (31, 29):
                assert (got[mat == 5] != got[mat == 5][0]).any() and (got[mat == 6] != got[mat == 6][0]).any()   # the checks are there
                assert (bits(got[mat == 4]) == one).all() and (mat == 4).sum() > 5
            if case in ("no PT_TEXTURES", "flag without a texture", "fake shader"):
                for m in (0, 1, 2, 3, 5, 6):
                    assert (bits(got[mat == m]) == bits(mats["color"][m])).all(), m
            if case == "glass":
                spec = (mats["hasReflective"][np.maximum(mat, 0)] > 0) | (mats["hasRefractive"][np.maximum(mat, 0)] > 0)
                assert (bits(got[spec | (mat < 0)]) == one).all() and (mat < 0).sum() > 0
                assert (spec & (mat >= 0)).sum() > 3 or (w, h) != (31, 29)
            if case.startswith("mesh"):
                paths = po.generate_rays(cam, depth)
                gg, tt, mm = np.ascontiguousarray(geoms).view(po.GEOM_DT), tris.view(po.TRI_DT), meshes.view(po.MESH_DT)
                hg = tm.hit_geoms(po, gg, tt, mm, paths, po.compute_intersections(paths, gg, tt, mm)[0])
                on_mesh = hg == len(geoms) - 1
                assert (bits(got[on_mesh]) == bits(mats["color"][6])).all()
                if (w, h) == (31, 29):
                    assert on_mesh.sum() > 5 and (bits(got[hg == 7]) != bits(mats["color"][6])).any()
            if case == "emitter":
                lamp = got[mat == 0]
                assert len(lamp) > 3 and (bits(lamp) != bits(mats["color"][0])).any()       # tinted: material.color times a texel
            if case == "clamp edges":
                assert (mat == 1).sum() > 3 and (mat == 2).sum() > 3
                same(got[mat == 1], np.broadcast_to(np.array([2.0 ** -6] * 3, dtype=F32), got[mat == 1].shape), "0, NaN, 2^-7")
                same(got[mat == 2], np.broadcast_to(np.array([64.0, 0.5, 2.0 ** -6], dtype=F32), got[mat == 2].shape), "65, 0.5, 2^-6")
        finally:
            pt.pathtraceFree()


# ---- 2. pt_denoise with the switch on ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w, h", [(31, 29), (97, 61), (130, 9)])
def test_denoise_switched_on_equals_the_model(pt, po, scenes, launch_plan, w, h):
    geoms, mats, cam, depth, _, _, tex = open_session(pt, scenes, "textured", w, h, max_batch=4)
    try:
        n = w * h
        image = np.zeros((n, 3), dtype=F32)
        pt.trace_batch(1, 4, image)
        if (w, h) == (31, 29):                                       # the sum the filter reads is the texture model's
            m = tm.Model(po, geoms, mats, cam, depth)
            for k, t in tex.items():
                m.set_texture(k, t)
            for it in range(1, 5):
                m.iterate(it)
            same(image, m.image, "running sum")
        g = first_hits(po, geoms, cam, depth)
        A = alm.albedo(po, geoms, mats, tex, cam, depth)
        assert (A != 1).any()
        pt.set_denoise_albedo(True)
        assert launches(pt) == (0, 0, 0)
        got = pt.denoise(4, 0, *DEFAULT)                             # levels = 0: the mean, nothing demodulated, no G-buffer
        same(got, (image / F32(4)).astype(F32), "levels 0")
        assert launches(pt) == (0, 0, 1)
        filt = 0
        for lv in (1, 2, 3, 7):
            got, px = pt.denoise(4, lv, *DEFAULT, rgba=True)
            want = model_on(image, 4, A, g, w, h, lv)
            assert np.isfinite(want).all()
            same(got, want, "levels %d" % lv)
            assert px.tobytes() == am.rgba8(want).tobytes(), "RGBA, levels %d" % lv
            filt += lv
            assert launches(pt) == (1, filt, 1)                      # one launch per level; the G-buffer (with the plane) once
            assert (bits(want) != bits(model_off(image, 4, g, w, h, lv))).any()
        other = (0.45, 0.35, 0.2)
        same(pt.denoise(4, 2, *other), model_on(image, 4, A, g, w, h, 2, other), "other sigmas")
        same(pt.albedo(), A, "the plane the filter used")
        assert launches(pt) == (1, filt + 2, 1)
    finally:
        pt.pathtraceFree()


# ---- 3. state -----------------------------------------------------------------------------------------------------------------------
def test_on_off_on(pt, po, scenes, launch_plan):
    w, h = 65, 5
    geoms, mats, cam, depth, _, _, tex = open_session(pt, scenes, "textured", w, h, max_batch=2)
    try:
        image = np.zeros((w * h, 3), dtype=F32)
        pt.trace_batch(1, 2, image)
        g = first_hits(po, geoms, cam, depth)
        A = alm.albedo(po, geoms, mats, tex, cam, depth)
        off, on = model_off(image, 2, g, w, h, 3), model_on(image, 2, A, g, w, h, 3)
        assert (bits(off) != bits(on)).any()
        before = pt.denoise(2, 3)
        same(before, off, "before the switch")
        pt.set_denoise_albedo(1)
        same(pt.denoise(2, 3), on, "on")
        pt.set_denoise_albedo(0)
        between = pt.denoise(2, 3)
        assert between.tobytes() == before.tobytes()
        pt.set_denoise_albedo(True)
        same(pt.denoise(2, 3), on, "on again")
        assert launches(pt) == (2, 12, 0)                            # the plain G-buffer, then once more for the plane
    finally:
        pt.pathtraceFree()


def test_textures_and_camera_are_followed(pt, po, scenes, launch_plan):
    """A texture set, changed and removed between calls, then a camera change: the plane and the filter follow each, and nothing
    is recomputed when nothing changed.  The switch survives pt_clear_image, pt_set_camera and pt_set_texture."""
    w, h = 31, 29
    geoms, mats, cam, depth, _, _, _ = open_session(pt, scenes, "flag without a texture", w, h, max_batch=2)
    try:
        n = w * h
        pt.trace_batch(1, 2, None)
        pt.set_denoise_albedo(True)
        g = first_hits(po, geoms, cam, depth)
        count = 0

        def check(tex, what, camera=cam, gb=g, fresh=True):
            nonlocal count
            image = pt.get_image(n).copy()
            A = alm.albedo(po, geoms, mats, tex, camera, depth)
            same(pt.denoise(2, 2), model_on(image, 2, A, gb, w, h, 2), what)
            count += 1 if fresh else 0
            assert launches(pt)[0] == count, what
            same(pt.albedo(), A, what + ": the plane")
            assert launches(pt)[0] == count, what
            return A

        plain = check({}, "no texture")
        first = random_texture(4, 1)
        pt.set_texture(5, first)
        a1 = check({5: first}, "a texture set")
        assert (bits(a1) != bits(plain)).any()
        pt.set_texture(5, first.copy())                              # the same texels again: the table has not changed
        check({5: first}, "the same texture again", fresh=False)
        pt.set_texture(3, None)                                      # removing what is not there: neither
        check({5: first}, "nothing removed", fresh=False)
        second = random_texture(4, 2)
        pt.set_texture(5, second)
        a2 = check({5: second}, "the texture changed")
        assert (bits(a2) != bits(a1)).any()
        pt.set_texture(6, random_texture(8, 3))
        check({5: second, 6: random_texture(8, 3)}, "a second texture")
        pt.set_texture(5, None)
        pt.set_texture(6, None)
        same(check({}, "the textures removed"), plain, "back to material.color")
        pt.clear_image()
        pt.trace_batch(1, 2, None)
        check({}, "after pt_clear_image", fresh=False)
        moved = cam.copy()
        moved["position"][0][0] += 0.75
        moved["position"][0][1] -= 0.5
        pt.set_camera(moved, depth)
        pt.set_texture(6, first)
        gm_ = first_hits(po, geoms, moved, depth)
        check({6: first}, "a camera change and a texture", camera=moved, gb=gm_)
        pt.set_camera(cam, depth)
        check({6: first}, "the camera back", camera=cam, gb=g)
    finally:
        pt.pathtraceFree()
    # the switch ends with pt_free: a new session filters colour
    geoms, mats, cam, depth, _, _, tex = open_session(pt, scenes, "textured", w, h, max_batch=2)
    try:
        image = np.zeros((n, 3), dtype=F32)
        pt.trace_batch(1, 2, image)
        same(pt.denoise(2, 2), model_off(image, 2, g, w, h, 2), "a new session")
    finally:
        pt.pathtraceFree()


def test_plane_goes_stale_with_a_texel_and_with_nothing_else(pt, po, scenes, launch_plan):
    """k_gbuffer launches count what is recomputed (40 x 26): a material's own texels set again and bump maps set, replaced and
    removed leave the plane as it is; one changed texel does not."""
    w, h = 40, 26
    geoms, mats, cam, depth, _, _, _ = open_session(pt, scenes, "flag without a texture", w, h, max_batch=2)
    try:
        tex = random_texture(4, 11)
        pt.set_texture(5, tex)
        plane = pt.albedo().copy()
        same(plane, alm.albedo(po, geoms, mats, {5: tex}, cam, depth), "the plane")
        assert launches(pt)[0] == 1
        pt.set_texture(5, tex.copy())                                # the identical texture
        assert pt.albedo().tobytes() == plane.tobytes() and launches(pt)[0] == 1
        bump = np.random.default_rng(12).normal(0, 0.8, (6, 4, 4, 3)).astype(F32)
        for m, t in ((5, bump), (6, bump[:, :2, :2]), (5, bump[:, :3, :3]), (5, None)):
            pt.set_bump_map(m, t)
            assert pt.albedo().tobytes() == plane.tobytes() and launches(pt)[0] == 1, m
        one = tex.copy()
        one[3, 2, 1, 2] = np.nextafter(one[3, 2, 1, 2], F32(4))      # one float of one texel, by one ulp
        pt.set_texture(5, one)
        same(pt.albedo(), alm.albedo(po, geoms, mats, {5: one}, cam, depth), "one texel changed")
        assert launches(pt)[0] == 2
        pt.set_texture(5, one.copy())
        pt.albedo()
        assert launches(pt)[0] == 2
    finally:
        pt.pathtraceFree()


def test_unit_albedo_switched_on_is_switched_off(pt, po, scenes, launch_plan):
    w, h = 97, 61
    g0, mats, cam, depth, _ = textured(pt)
    mats = mats.copy()
    col = mats["color"].copy()
    col[(mats["hasReflective"] == 0) & (mats["hasRefractive"] == 0)] = 1.0
    mats["color"] = col
    cam = _resized(cam, w, h)
    pt.pathtraceInit(pt.Scene(g0, mats, cam, depth), flags=pt.PT_COMPACT, max_batch=2)
    try:
        image = np.zeros((w * h, 3), dtype=F32)
        pt.trace_batch(1, 2, image)
        off = [pt.denoise(2, lv) for lv in (0, 1, 4)]
        pt.set_denoise_albedo(True)
        assert (bits(pt.albedo()) == bits(F32(1.0))).all()
        for k, lv in enumerate((0, 1, 4)):
            assert pt.denoise(2, lv).tobytes() == off[k].tobytes(), lv
        g = first_hits(po, g0, cam, depth)
        same(off[2], model_off(image, 2, g, w, h, 4), "levels 4")
    finally:
        pt.pathtraceFree()


# ---- 4. pt_denoise_temporal with the switch on ------------------------------------------------------------------------------------
def test_temporal_switched_on_equals_the_model(pt, po, scenes, launch_plan):
    """One camera move at 97 x 61: the history, the blend (levels = 0) and the filtered result against the model; the history and
    the blend are those of the switch off."""
    w, h = 97, 61
    n = w * h

    def run(on):
        geoms, mats, cam, depth, _, _, tex = open_session(pt, scenes, "textured", w, h, max_batch=2)
        model = alm.Temporal(w, h, np.ascontiguousarray(mats).view(po.MATERIAL_DT))
        out = []
        try:
            pt.set_denoise_albedo(on)
            moved = cam.copy()
            moved["position"][0][0] += 0.75
            moved["position"][0][1] -= 0.5
            for k, camera in enumerate((cam, moved)):
                if k:
                    pt.set_camera(camera, depth)
                    pt.clear_image()
                image = np.zeros((n, 3), dtype=F32)
                pt.trace_batch(1, 2, image)
                g = first_hits(po, geoms, camera, depth)
                A = alm.albedo(po, geoms, mats, tex, camera, depth) if on else None
                for lv in (0, 3, 1):
                    prm = pt.DenoiseParams(lv, *DEFAULT)
                    got, px = pt.denoise_temporal(2, prm, rgba=True)
                    want = model.call(image, 2, camera, g, A=A, levels=lv)
                    same(got, want, "camera %d, levels %d, switch %r" % (k, lv, on))
                    assert px.tobytes() == am.rgba8(want).tobytes()
                    hc, hn = pt.history()
                    same(hc, model.hc, "history colours")
                    same(hn.reshape(-1, 1), model.hn.reshape(-1, 1), "history lengths")
                    out.append((got.copy(), hc.copy(), hn.copy()))
                if k:
                    assert (model.hn > 0).sum() > n // 4
                # pt_denoise beside the temporal calls: the plane is this camera's
                want = model_on(image, 2, A, g, w, h, 2) if on else model_off(image, 2, g, w, h, 2)
                same(pt.denoise(2, 2), want, "pt_denoise, camera %d" % k)
            return out
        finally:
            pt.pathtraceFree()

    off, on = run(False), run(True)
    for k in range(len(off)):
        assert on[k][1].tobytes() == off[k][1].tobytes() and on[k][2].tobytes() == off[k][2].tobytes()       # pt_history
    for k in (0, 3):                                                 # levels = 0: c0, in modulated colour
        assert on[k][0].tobytes() == off[k][0].tobytes()
    assert on[1][0].tobytes() != off[1][0].tobytes() and on[4][0].tobytes() != off[4][0].tobytes()


# ---- 5. the session is left alone -------------------------------------------------------------------------------------------------
def test_session_is_unchanged_by_the_switch_the_plane_and_the_filter(pt, scenes, launch_plan):
    w, h = 65, 5
    n = w * h

    def start():
        return open_session(pt, scenes, "textured", w, h, max_batch=2)

    start()
    try:
        pt.trace_batch(1, 2, None)
        pt.trace_batch_async(3, 2)                                   # still in flight when the plane is asked for
        pt.set_denoise_albedo(True)
        pt.albedo()
        image, rays, counters = pt.get_image(n).copy(), pt.total_rays(), pt.counters()
        st = pt.get_stats()
        stats = (st.bounces, st.rays, list(st.live), st.total_rays, st.total_iterations)
        pt.set_denoise_albedo(False)
        pt.set_denoise_albedo(True)
        pt.albedo()
        pt.denoise(4, 3)
        st = pt.get_stats()
        assert pt.get_image(n).tobytes() == image.tobytes()
        assert pt.total_rays() == rays and pt.counters() == counters
        assert (st.bounces, st.rays, list(st.live), st.total_rays, st.total_iterations) == stats
        pt.trace_batch(5, 2, None)
        after = pt.get_image(n).copy()
    finally:
        pt.pathtraceFree()
    start()
    try:
        for it in (1, 3, 5):
            pt.trace_batch(it, 2, None)
        assert pt.get_image(n).tobytes() == after.tobytes()
    finally:
        pt.pathtraceFree()


def test_lookahead_windows_survive(pt, po, scenes, launch_plan):
    """PT_PIN_IMAGE | PT_HOST_SPARSE | PT_LOOKAHEAD, one pt_trace per iteration: the switch, the plane and a switched-on pt_denoise
    after calls 1 and 2 enqueue, miss and discard no window, and the rays served add up to the run without them."""
    w, h = 31, 29
    n = w * h
    L = pt.library()

    def book():
        out = (C.c_uint64 * 4)()
        assert L.ptdbg_lookahead(out) == 0
        return tuple(int(v) for v in out)

    def run(filter_after):
        buf = np.full((n, 3), -7.0, dtype=F32)
        geoms, mats, cam, depth, _, _, tex = open_session(pt, scenes, "textured", w, h, max_batch=8, pin_image=False,
                                                          flags=pt.PT_COMPACT | pt.PT_LOOKAHEAD | pt.PT_PIN_IMAGE | pt.PT_HOST_SPARSE)
        try:
            g = first_hits(po, geoms, cam, depth)
            A = alm.albedo(po, geoms, mats, tex, cam, depth)
            served, sums = 0, []
            for it in (1, 2, 3, 4):
                assert L.pt_trace(None, 0, it, buf.ctypes.data) == 0, L.pt_last_error()
                served += pt.get_stats().rays
                sums.append(buf.copy())
                if it in filter_after:
                    b0 = book()
                    pt.set_denoise_albedo(True)
                    same(pt.albedo(), A, "the plane after call %d" % it)
                    same(pt.denoise(it, 3), model_on(buf, it, A, g, w, h, 3), "the filter after call %d" % it)
                    assert book() == b0
                    assert pt.get_image(n).tobytes() == buf.tobytes() == sums[-1].tobytes()
            return served, book()[:3], sums
        finally:
            pt.pathtraceFree()

    plain, filtered = run(()), run((1, 2))
    assert filtered[0] == plain[0]                                   # (a discarded window would show as re-traced rays)
    assert filtered[1] == plain[1] and plain[1][2] == 0              # the same windows, none thrown away
    for a, b in zip(plain[2], filtered[2]):
        assert a.tobytes() == b.tobytes()


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals(pt, po, scenes, launch_plan):
    w, h = 31, 29
    L = pt.library()
    geoms, mats, cam, depth, _, _, tex = open_session(pt, scenes, "textured", w, h, max_batch=2)
    try:
        pt.trace_batch(1, 2, None)
        image = pt.get_image(w * h).copy()
        g = first_hits(po, geoms, cam, depth)
        for bad in (2, -1, 256):
            assert L.pt_set_denoise_albedo(bad) == -1 and b"enable" in L.pt_last_error(), bad
        same(pt.denoise(2, 2), model_off(image, 2, g, w, h, 2), "a refused call leaves the switch off")
        pt.set_denoise_albedo(1)
        assert L.pt_set_denoise_albedo(2) == -1
        A = alm.albedo(po, geoms, mats, tex, cam, depth)
        same(pt.denoise(2, 2), model_on(image, 2, A, g, w, h, 2), "... and on")
    finally:
        pt.pathtraceFree()
    for kw in (dict(devices=[0, 0]), dict(tile=(0, 2, 8))):
        open_session(pt, scenes, "textured", w, h, max_batch=2, **kw)
        try:
            pt.trace_batch(1, 2, None)
            for enable in (0, 1):
                assert L.pt_set_denoise_albedo(enable) == -1 and b"tile" in L.pt_last_error() and b"pt_set_denoise_albedo" in L.pt_last_error()
            assert L.pt_albedo(None) == -1 and b"tile" in L.pt_last_error() and b"pt_albedo" in L.pt_last_error()
            pt.trace_batch(3, 2, None)                               # the session still traces
        finally:
            pt.pathtraceFree()
    assert L.pt_set_denoise_albedo(1) == -1 and b"not initialised" in L.pt_last_error()
    assert L.pt_albedo(None) == -1 and b"not initialised" in L.pt_last_error()


# ---- 7. the headless host ---------------------------------------------------------------------------------------------------------
def test_ptbench_albedo_writes_the_models_picture(pt, po, scenes, tmp_path, launch_plan):
    w, h = 33, 30
    txt = open(os.path.join(ROOT, "scenes", "cornell_textured.txt")).read()
    assert "RES         800 800" in txt
    scene_file = tmp_path / "textured_small.txt"
    scene_file.write_text(txt.replace("RES         800 800", "RES         %d %d" % (w, h)))
    exe = pt.build_ptbench()
    p = subprocess.run([exe, str(scene_file), "--iters", "4", "--batch", "2", "--textures", "--out", str(tmp_path / "r"),
                        "--denoise", "3,1.0,0.35,0.5", "--albedo"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "denoise: 3 levels" in p.stdout and "albedo demodulated" in p.stdout
    from PIL import Image
    s = pt.load_scene(str(scene_file))
    m = tm.Model(po, s.geoms, s.materials, s.camera, s.traceDepth)
    for k, t in dict(s.textures).items():
        m.set_texture(k, t)
    for it in range(1, 5):
        m.iterate(it)
    raw = np.asarray(Image.open(str(tmp_path / "r.4samp.png")).convert("RGB"), dtype=np.uint8)
    assert raw.tobytes() == pt.image_to_rgb8(m.image, w, h, 4.0).tobytes()
    g = first_hits(po, s.geoms, s.camera, s.traceDepth)
    A = alm.albedo(po, s.geoms, s.materials, dict(s.textures), s.camera, s.traceDepth)
    want = model_on(m.image, 4, A, g, w, h, 3)
    got = np.asarray(Image.open(str(tmp_path / "r.4samp.denoised.png")).convert("RGB"), dtype=np.uint8)
    assert got.tobytes() == pt.image_to_rgb8(want, w, h, 1.0).tobytes()
    assert got.tobytes() != pt.image_to_rgb8(model_off(m.image, 4, g, w, h, 3), w, h, 1.0).tobytes()
    p = subprocess.run([exe, str(scene_file), "--iters", "2", "--textures", "--out", str(tmp_path / "bad"), "--albedo"],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode != 0 and "--denoise" in p.stderr
