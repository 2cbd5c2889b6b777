"""The specification of pt_denoise_temporal as tests/temporal_model.py models it, checked on the
CPU: the model's invariants, and that it does what it is for -- the first frame after a camera move, with the history of
the previous view blended in, is at least twice as close to the converged image of the new view as the filter alone can
make it.  Also: the new entry points before pt_init."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import __graft_entry__ as ge  # noqa: E402
import atrous_model as am  # noqa: E402
import temporal_model as tm  # noqa: E402
from gpu_common import _resized, rel_l2  # noqa: E402

F = np.float32


def moved(cam, d):
    """position and lookAt translated by d: view / up / right stay"""
    c = cam.copy()
    c["position"][0] += np.asarray(d, dtype=np.float32)
    c["lookAt"][0] += np.asarray(d, dtype=np.float32)
    return c


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def materials_of(kinds):
    """a material table: 'd' diffuse, 'm' mirror, 'g' glass"""
    m = np.zeros(len(kinds), dtype=ge.load_package().MATERIAL_DT)
    for i, k in enumerate(kinds):
        m["hasReflective"][i] = 1.0 if k == "m" else 0.0
        m["hasRefractive"][i] = 1.0 if k == "g" else 0.0
    return m


def simple_camera(w, h):
    cam = np.zeros(1, dtype=ge.load_package().CAMERA_DT)
    cam["resolution"][0] = (w, h)
    cam["position"][0] = (0, 0, 0)
    cam["lookAt"][0] = (0, 0, -1)
    cam["view"][0] = (0, 0, -1)
    cam["up"][0] = (0, 1, 0)
    cam["right"][0] = (1, 0, 0)
    cam["pixelLength"][0] = (0.25, 0.25)
    return cam


def plane_gbuffer(cam, w, h, mat, depth=4.0):
    """first hits of cam's pinhole rays on the plane z = -depth (its view axis is -z), material `mat` [n]"""
    c = cam[0]
    y, x = np.divmod(np.arange(w * h), w)
    d = (c["view"][None, :] - c["right"][None, :] * (c["pixelLength"][0] * (x[:, None] - w * 0.5))
         - c["up"][None, :] * (c["pixelLength"][1] * (y[:, None] - h * 0.5)))
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    t = (-depth - c["position"][2]) / d[:, 2]
    pos = c["position"][None, :] + d * t[:, None]
    n = len(t)
    return {"t": t.astype(np.float32), "position": pos.astype(np.float32),
            "normal": np.tile(np.array([0, 0, 1], np.float32), (n, 1)), "materialId": np.asarray(mat, dtype=np.int32).reshape(n)}


# ---- 1. invariants -----------------------------------------------------------------------------------------------------
def test_no_history_is_the_plain_filter_bit_for_bit():
    rng = np.random.default_rng(11)
    w, h = 23, 17
    cam = simple_camera(w, h)
    g = plane_gbuffer(cam, w, h, np.zeros(w * h))
    g["normal"] = rng.standard_normal((w * h, 3)).astype(np.float32)
    s = (rng.random((w * h, 3)) * 40).astype(np.float32)
    st = tm.Temporal(w, h, materials_of("d"))
    for levels in (0, 3):
        got = st.call(s, 16, cam, g, levels, 4.0, 0.35, 0.5)
        want = am.denoise(s.reshape(h, w, 3), 16, g["normal"].reshape(h, w, 3), g["position"].reshape(h, w, 3), levels, 4.0, 0.35, 0.5)
        assert (bits(got) == bits(want.reshape(-1, 3))).all()
        assert not st.hn.any() and not st.hc.any()             # the same camera again: the history stays what it was, nothing
        st.reset()


def test_identical_camera_maps_every_valid_pixel_to_itself(po, scenes):
    for name, (w, h) in (("cornell", (200, 200)), ("cornell_glass", (160, 90))):
        s = scenes[name]
        cam = _resized(s["camera"], w, h)
        g = am.gbuffer_from_oracle(po, cam, s["depth"], s["geoms"])
        n = w * h
        old = {"camera": cam, "g": g, "C": np.ones((n, 3), np.float32), "N": np.full(n, 7, np.float32)}
        hc, hn, q = tm.reproject(old, g, s["materials"], w, h, 64, 0.1, 0.1)
        mat = g["materialId"]
        diffuse = (mat >= 0) & (s["materials"]["hasReflective"][np.clip(mat, 0, None)] == 0) & \
                  (s["materials"]["hasRefractive"][np.clip(mat, 0, None)] == 0)
        assert (q[diffuse] == np.arange(n)[diffuse]).all(), name
        assert (q[~diffuse] == -1).all() and not hn[~diffuse].any() and not hc[~diffuse].any()
        assert (hn[diffuse] == 7).all() and (hc[diffuse] == 1).all()
        assert 0 < int(diffuse.sum()) < n
        if name == "cornell_glass":
            assert int(((mat >= 0) & ~diffuse).sum()) > 0      # specular first hits are in the frame


def test_max_history_zero_means_no_history():
    w, h = 16, 12
    cam = simple_camera(w, h)
    g = plane_gbuffer(cam, w, h, np.zeros(w * h))
    old = {"camera": cam, "g": g, "C": np.full((w * h, 3), 0.5, np.float32), "N": np.full(w * h, 9, np.float32)}
    new = moved(cam, (0.25, 0, 0))
    g2 = plane_gbuffer(new, w, h, np.zeros(w * h))
    hc, hn, q = tm.reproject(old, g2, materials_of("d"), w, h, 0, 0.1, 0.1)
    assert (q >= 0).any() and not hn.any()
    s = np.random.default_rng(3).random((w * h, 3)).astype(np.float32)
    c0, nn = tm.blend(s, 2, hc, hn)
    assert (bits(c0) == bits(s / F(2))).all() and (nn == 2).all()


def test_hand_made_cases_without_history():
    w, h = 16, 12
    n = w * h
    cam = simple_camera(w, h)
    mats = materials_of("dmg")
    g_old = plane_gbuffer(cam, w, h, np.zeros(n))
    old = {"camera": cam, "g": g_old, "C": np.full((n, 3), 0.5, np.float32), "N": np.full(n, 9, np.float32)}
    new = moved(cam, (0.25, 0, 0))                              # a quarter of a pixel's footprint at depth 4 (pixel = 1.0 there)
    base = plane_gbuffer(new, w, h, np.zeros(n))
    hc, hn, q = tm.reproject(old, base, mats, w, h, 64, 0.1, 0.1)
    inside = q >= 0
    assert inside.sum() > n // 2 and (hn[inside] == 9).all()
    P = int(np.flatnonzero(inside)[n // 4])

    def one(change):
        g = {k: v.copy() for k, v in base.items()}
        o = {"camera": old["camera"], "g": {k: v.copy() for k, v in g_old.items()}, "C": old["C"], "N": old["N"].copy()}
        change(g, o)
        hc, hn, q = tm.reproject(o, g, mats, w, h, 64, 0.1, 0.1)
        return float(hn[P]), hc[P].tolist(), int(q[P])

    assert one(lambda g, o: None) == (9.0, [0.5, 0.5, 0.5], int(q[P]))

    def mirror(g, o):
        g["materialId"][P] = 1
        o["g"]["materialId"][:] = 1

    def glass(g, o):
        g["materialId"][P] = 2
        o["g"]["materialId"][:] = 2

    def miss(g, o):
        g["materialId"][P] = -1
        g["t"][P] = -1
        g["position"][P] = 0
        g["normal"][P] = 0

    def behind(g, o):
        g["position"][P] = (0.0, 0.0, 3.0)                      # the old camera looks down -z from the origin

    def outside(g, o):
        g["position"][P] = (40.0, 0.0, -4.0)                    # 40 pixels to the side in a 16-pixel frame

    def other_material(g, o):
        o["g"]["materialId"][:] = 1
        o["g"]["materialId"][0] = 0

    def other_position(g, o):
        o["g"]["position"][:, 2] -= 1.0                         # a surface one unit further: 0.1 * t = 0.4 is exceeded

    def other_normal(g, o):
        o["g"]["normal"][:] = (0, 1, 0)

    def nan_position(g, o):
        g["position"][P] = np.nan

    for change in (mirror, glass, miss, behind, outside, other_material, other_position, other_normal, nan_position):
        assert one(change) == (0.0, [0.0, 0.0, 0.0], -1), change.__name__


def test_two_moves_carry_and_cap_the_length():
    w, h = 16, 12
    n = w * h
    mats = materials_of("d")
    rng = np.random.default_rng(9)
    cams = [simple_camera(w, h)]
    cams.append(moved(cams[0], (1.0, 0, 0)))                    # one pixel's footprint at depth 4, then one more in y
    cams.append(moved(cams[0], (1.0, 1.0, 0)))
    gs = [plane_gbuffer(c, w, h, np.zeros(n)) for c in cams]
    st = tm.Temporal(w, h, mats)
    s0 = rng.random((n, 3)).astype(np.float32) * 16
    st.call(s0, 16, cams[0], gs[0], 0, max_history=20)
    assert (st.cur["N"] == 16).all()
    s1 = rng.random((n, 3)).astype(np.float32) * 8
    st.call(s1, 8, cams[1], gs[1], 0, max_history=20)
    has = st.hn > 0
    assert 0 < has.sum() < n
    assert (st.hn[has] == 16).all() and (st.cur["N"][has] == 24).all() and (st.cur["N"][~has] == 8).all()
    q1, n1, c1 = st.q.copy(), st.cur["N"].copy(), st.cur["C"].copy()
    want = (s1[has] + (s0[q1[has]] / F(16)) * F(16)) / F(24)
    assert (bits(c1[has]) == bits(want.astype(np.float32))).all()
    # the same camera again, more samples: the history stays, the sum replaces the sum
    s1b = s1 + rng.random((n, 3)).astype(np.float32)
    st.call(s1b, 9, cams[1], gs[1], 0, max_history=20)
    assert (st.hn[has] == 16).all() and (st.cur["N"][has] == 25).all() and (st.q == q1).all()
    # the second move: history of history, capped at 20
    s2 = rng.random((n, 3)).astype(np.float32)
    st.call(s2, 1, cams[2], gs[2], 0, max_history=20)
    has2 = st.hn > 0
    src = st.q[has2]
    assert (st.hn[has2] == np.minimum(st.cur["N"][has2] - 1, 20)).all()
    prev_n = np.where(has, 25, 9)[src]
    assert (st.hn[has2] == np.minimum(prev_n, 20)).all() and (st.hn[has2][prev_n == 25] == 20).all() and (st.hn[has2][prev_n == 9] == 9).all()
    assert (prev_n == 25).any() and (prev_n == 9).any()
    st.reset()
    assert st.cur is None and not st.hn.any()


# ---- 2. what it is for -------------------------------------------------------------------------------------------------
def test_history_halves_the_error_of_the_first_frame_after_a_move(po, scenes):
    """200x200 Cornell on the oracle: 64 spp at the scene's camera, camera and lookAt translated by (0.3, 0.2, 0), 1 spp there.
    History (max_history 64, tolerances 0.1 / 0.1) + filter (5 / 4.0 / 0.35 / 0.5) against the same filter alone, rel-L2 to
    the 1024-spp image of the new view.  Measured with this model: 0.1451 against 0.8091 (ratio 0.179), 80.0 % of the pixels
    with history, 82.8 % hit anything."""
    s = scenes["cornell"]
    w = h = 200
    filt = (5, 4.0, 0.35, 0.5)
    cam_a = _resized(s["camera"], w, h)
    cam_b = moved(cam_a, (0.3, 0.2, 0.0))
    g_a = am.gbuffer_from_oracle(po, cam_a, s["depth"], s["geoms"])
    g_b = am.gbuffer_from_oracle(po, cam_b, s["depth"], s["geoms"])
    tr = po.Tracer(s["geoms"], s["materials"], cam_a, s["depth"])
    tr.iterate_parallel(1, 64, 8)
    st = tm.Temporal(w, h, s["materials"])
    st.call(tr.image, 64, cam_a, g_a, *filt, max_history=64, ptol=0.1, ntol=0.1)
    tr = po.Tracer(s["geoms"], s["materials"], cam_b, s["depth"])
    tr.iterate_parallel(1, 1, 8)
    s1 = tr.image.copy()
    tr.iterate_parallel(2, 1023, 8)
    conv = tr.image / F(1024)
    temporal = st.call(s1, 1, cam_b, g_b, *filt, max_history=64, ptol=0.1, ntol=0.1)
    plain = am.denoise(s1.reshape(h, w, 3), 1, g_b["normal"].reshape(h, w, 3), g_b["position"].reshape(h, w, 3), *filt).reshape(-1, 3)
    share = float((st.hn > 0).mean())
    e_t, e_p = rel_l2(temporal, conv), rel_l2(plain, conv)
    print("rel-L2 against 1024 spp of the new view: with history %.4f, filter alone %.4f, ratio %.3f; share of pixels with history %.3f, hit %.3f"
          % (e_t, e_p, e_t / e_p, share, float((g_b["t"] > 0).mean())))
    assert 0.5 < share < 0.95
    assert e_t <= 0.5 * e_p


# ---- 3. before pt_init -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pt():
    ge.load_package().build()
    return ge.load_package()


def test_temporal_entry_points_before_init_fail_cleanly(pt):
    L = pt.library()
    pt.pathtraceFree()
    prm = pt.DenoiseParams(5, 1.0, 0.35, 0.5)
    tmp = pt.TemporalParams(64, 0.1, 0.1)
    assert L.pt_denoise_temporal(C.byref(prm), C.byref(tmp), 16, None, None) == -1
    assert b"pt_denoise_temporal" in L.pt_last_error() and b"not initialised" in L.pt_last_error()
    assert L.pt_history(None, None) == -1
    assert b"pt_history" in L.pt_last_error() and b"not initialised" in L.pt_last_error()
    assert L.pt_history_reset() == -1
    assert b"pt_history_reset" in L.pt_last_error() and b"not initialised" in L.pt_last_error()
    for call in (lambda: pt.denoise_temporal(16), pt.history, pt.history_reset):
        with pytest.raises(pt.PtError):
            call()
