"""The specification of pt_denoise_svgf as tests/svgf_model.py models it, checked on the CPU: the model's
invariants -- without history and spatial estimate it IS pt_denoise_variance, its colour and sample counts ARE pt_denoise_temporal's,
the moments travel with the colour, both variance estimates are zero on a constant image and the spatial one measures iid noise --
and what it is for: after a camera move, at 1, 2 and 4 samples per pixel, it is closer to the converged picture of the new view than
the variance-guided filter alone, whatever the exposure.  Also: the four entry points before pt_init."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import __graft_entry__ as ge  # noqa: E402
import atrous_model as am  # noqa: E402
import svgf_model as sm  # noqa: E402
import temporal_model as tm  # noqa: E402
import variance_model as vm  # noqa: E402
from gpu_common import _resized, rel_l2  # noqa: E402
from test_temporal_model_cpu import bits, materials_of, moved, plane_gbuffer, simple_camera  # noqa: E402

F = np.float32
SIG = (4.0, 0.35, 0.5)


def random_session(rng, n, iters):
    """per-sample colours of `iters` iterations and what a PT_MOMENTS session holds after them: (sum, M1, M2)"""
    acc = np.zeros((n, 3), np.float32)
    m1, m2 = np.zeros(n, np.float32), np.zeros(n, np.float32)
    for _ in range(iters):
        c = (rng.random((n, 3)) * 3).astype(np.float32)
        acc = (acc + c).astype(np.float32)
        m1, m2 = vm.accumulate(m1, m2, c)
    return acc, m1, m2


# ---- 1. invariants -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iters", [1, 2, 5, 16])
def test_no_history_no_spatial_estimate_is_pt_denoise_variance_bit_for_bit(iters):
    rng = np.random.default_rng(100 + iters)
    w, h = 23, 17
    cam = simple_camera(w, h)
    g = plane_gbuffer(cam, w, h, np.zeros(w * h))
    g["normal"] = rng.standard_normal((w * h, 3)).astype(np.float32)
    acc, m1, m2 = random_session(rng, w * h, iters)
    st = sm.Svgf(w, h, materials_of("d"))
    nrm, pos = g["normal"].reshape(h, w, 3), g["position"].reshape(h, w, 3)
    for levels in (0, 1, 3):
        got = st.call(acc, m1, m2, iters, cam, g, levels, *SIG, spatial_below=0)
        want = vm.denoise(acc.reshape(h, w, 3), m1.reshape(h, w), m2.reshape(h, w), iters, nrm, pos, levels, *SIG)
        assert (bits(got) == bits(want.reshape(-1, 3))).all()
        assert (bits(st.var0) == bits(vm.var0(m1, m2, iters))).all()
        assert not st.hn.any() and not st.h1.any() and not st.h2.any() and not st.hc.any()
        st.reset()


def test_colour_and_sample_counts_are_the_temporal_filters():
    """the same calls, the same parameters: C, N and the colour history equal temporal_model.Temporal's planes"""
    w, h = 16, 12
    n = w * h
    rng = np.random.default_rng(5)
    cams = [simple_camera(w, h)]
    cams += [moved(cams[0], (1.0, 0, 0)), moved(cams[0], (1.0, 1.0, 0))]
    gs = [plane_gbuffer(c, w, h, np.zeros(n)) for c in cams]
    a, b = sm.Svgf(w, h, materials_of("d")), tm.Temporal(w, h, materials_of("d"))
    for k, iters in ((0, 16), (1, 2), (1, 3), (2, 1), (0, 4)):
        acc, m1, m2 = random_session(rng, n, iters)
        a.call(acc, m1, m2, iters, cams[k], gs[k], 1, *SIG, max_history=20)
        b.call(acc, iters, cams[k], gs[k], 1, 1.0, 0.35, 0.5, max_history=20)
        assert (bits(a.cur["C"]) == bits(b.cur["C"])).all() and (bits(a.cur["N"]) == bits(b.cur["N"])).all()
        assert (bits(a.hc) == bits(b.hc)).all() and (bits(a.hn) == bits(b.hn)).all() and (a.q == b.q).all()
    assert (a.hn > 0).any() and (a.hn == 0).any()


def test_identical_camera_keeps_the_history_and_max_history_zero_means_none():
    w, h = 16, 12
    n = w * h
    rng = np.random.default_rng(6)
    cam_a = simple_camera(w, h)
    cam_b = moved(cam_a, (1.0, 0, 0))
    g_a, g_b = plane_gbuffer(cam_a, w, h, np.zeros(n)), plane_gbuffer(cam_b, w, h, np.zeros(n))
    st = sm.Svgf(w, h, materials_of("d"))
    first = random_session(rng, n, 8)
    st.call(*first, 8, cam_a, g_a, 0)
    second = random_session(rng, n, 1)
    st.call(*second, 1, cam_b, g_b, 0)
    kept = [p.copy() for p in (st.hc, st.h1, st.h2, st.hn)]
    assert (st.hn > 0).any()
    third = random_session(rng, n, 2)                           # the same camera: the sum replaces the sum, the history stays
    st.call(*third, 2, cam_b, g_b, 0)
    for p, q in zip(kept, (st.hc, st.h1, st.h2, st.hn)):
        assert p.tobytes() == q.tobytes()
    has = st.hn > 0
    assert (st.cur["N"][has] == 10).all() and (st.cur["N"][~has] == 2).all()
    st = sm.Svgf(w, h, materials_of("d"))
    st.call(*first, 8, cam_a, g_a, 0)
    st.call(*second, 1, cam_b, g_b, 0, max_history=0)
    assert (st.q >= 0).any() and not st.hn.any()
    assert (bits(st.cur["C"]) == bits(second[0])).all() and (bits(st.cur["U1"]) == bits(second[1])).all() and (st.cur["N"] == 1).all()


def test_two_moves_carry_and_cap_the_length_and_the_moments_travel():
    w, h = 16, 12
    n = w * h
    rng = np.random.default_rng(9)
    cams = [simple_camera(w, h)]
    cams += [moved(cams[0], (1.0, 0, 0)), moved(cams[0], (1.0, 1.0, 0))]
    gs = [plane_gbuffer(c, w, h, np.zeros(n)) for c in cams]
    st = sm.Svgf(w, h, materials_of("d"))
    s0 = random_session(rng, n, 16)
    st.call(*s0, 16, cams[0], gs[0], 0, max_history=20)
    assert (bits(st.cur["U1"]) == bits(s0[1] / F(16))).all() and (bits(st.cur["U2"]) == bits(s0[2] / F(16))).all()
    s1 = random_session(rng, n, 8)
    st.call(*s1, 8, cams[1], gs[1], 0, max_history=20)
    has, q1 = st.hn > 0, st.q.copy()
    assert 0 < has.sum() < n and (st.hn[has] == 16).all() and (st.cur["N"][has] == 24).all() and (st.cur["N"][~has] == 8).all()
    assert (bits(st.h1[has]) == bits((s0[1] / F(16))[q1[has]])).all() and (bits(st.h2[has]) == bits((s0[2] / F(16))[q1[has]])).all()
    want = ((s1[1][has] + (s0[1] / F(16))[q1[has]] * F(16)) / F(24)).astype(np.float32)
    assert (bits(st.cur["U1"][has]) == bits(want)).all()
    u1_b, u2_b, n_b = st.cur["U1"].copy(), st.cur["U2"].copy(), st.cur["N"].copy()
    s2 = random_session(rng, n, 1)
    st.call(*s2, 1, cams[2], gs[2], 0, max_history=20)          # history of history, capped at 20
    has2 = st.hn > 0
    src = st.q[has2]
    assert (st.hn[has2] == np.minimum(n_b[src], 20)).all() and (n_b[src] == 24).any() and (n_b[src] == 8).any()
    assert (bits(st.h1[has2]) == bits(u1_b[src])).all() and (bits(st.h2[has2]) == bits(u2_b[src])).all()
    st.reset()
    assert st.cur is None and not st.hn.any() and not st.h1.any() and not st.h2.any()


def test_constant_image_has_variance_zero_from_both_estimates():
    w, h = 23, 17
    n = w * h
    cam = simple_camera(w, h)
    g = plane_gbuffer(cam, w, h, np.zeros(n))
    c = np.tile(np.array([0.7, 0.3, 1.9], np.float32), (n, 1))
    for iters in (1, 2, 3, 7):
        acc = np.zeros((n, 3), np.float32)
        m1, m2 = np.zeros(n, np.float32), np.zeros(n, np.float32)
        for _ in range(iters):
            acc = (acc + c).astype(np.float32)
            m1, m2 = vm.accumulate(m1, m2, c)
        for below in (0, 1 << 20):
            st = sm.Svgf(w, h, materials_of("d"))
            got = st.call(acc, m1, m2, iters, cam, g, 2, *SIG, spatial_below=below)
            # zero up to rounding: u2 - u1 * u1 is a few ulps of l^2 either side of 0 (fmaxf cuts the negative side), and the 49
            # weighted sums of the spatial estimate carry at most 49 roundings each: (3 * 49 / 2 + 4) eps l^2 < 100 eps l^2
            assert st.var0.max() <= 100 * np.finfo(np.float32).eps * float(vm.lum(c[0])) ** 2
            assert np.abs(got - acc / F(iters)).max() <= 1e-5
    st = sm.Svgf(w, h, materials_of("d"))
    st.call(c, *vm.accumulate(np.zeros(n, np.float32), np.zeros(n, np.float32), c), 1, cam, g, 0, *SIG, spatial_below=0)
    assert not st.var0.any()                                    # one sample, the temporal estimate: l * l - l * l exactly


def test_spatial_estimate_measures_iid_noise_on_a_flat_region():
    """1 spp, grey samples v ~ U(0, 1) on a region with one normal and one position: every tap weighs 1, and an interior pixel's
    estimate is the biased sample variance of its n = 49 taps, s^2 = mean(l^2) - mean(l)^2.  For iid l with variance sigma^2 = 1 / 12
    and fourth central moment mu4 = 1 / 80:  E s^2 = sigma^2 (n - 1) / n,  Var s^2 = (n - 1)^2 mu4 / n^3 - (n - 1)(n - 3) sigma^4 /
    n^3.  Windows 7 pixels apart share no tap, so the mean of K of them has variance Var s^2 / K; the test allows 5 standard
    deviations of that mean around E s^2 (K = 100: +- 6.4 % of sigma^2)."""
    w = h = 76                                                  # centres 3, 10, .., 66 in both directions: 10 x 10 disjoint windows
    npx = w * h
    rng = np.random.default_rng(77)
    v = rng.random(npx).astype(np.float32)
    c = np.repeat(v[:, None], 3, axis=1)
    m1, m2 = vm.accumulate(np.zeros(npx, np.float32), np.zeros(npx, np.float32), c)
    cam = simple_camera(w, h)
    g = plane_gbuffer(cam, w, h, np.zeros(npx))
    g["position"][:] = (0.0, 0.0, -4.0)
    st = sm.Svgf(w, h, materials_of("d"))
    st.call(c, m1, m2, 1, cam, g, 0, *SIG, spatial_below=4)
    centres = np.arange(3, 70, 7)
    est = st.var0.reshape(h, w)[np.ix_(centres, centres)].astype(np.float64)
    n, k = 49, est.size
    sigma2, mu4 = 1.0 / 12.0, 1.0 / 80.0
    mean = sigma2 * (n - 1) / n
    var = (n - 1) ** 2 * mu4 / n ** 3 - (n - 1) * (n - 3) * sigma2 ** 2 / n ** 3
    bound = 5.0 * np.sqrt(var / k)
    print("spatial estimate over %d disjoint windows: mean %.5f, expected %.5f +- %.5f (sigma^2 = %.5f)" % (k, est.mean(), mean, bound, sigma2))
    assert k == 100 and abs(est.mean() - mean) <= bound
    assert not sm.temporal_variance(st.cur["U1"], st.cur["U2"], st.cur["N"]).any()      # what the temporal estimate has at 1 spp


# ---- 2. what it is for, on oracle and model alone --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cornell_move(po, scenes, golden):
    """200 x 200 Cornell on the oracle (the set-up of test_history_halves_the_error_of_the_first_frame_after_a_move): 64 spp at the
    scene's camera, a move by (0.3, 0.2, 0), the running sum and the moments after 1, 2 and 4 samples there, and the mean of 1024
    (tests/golden/svgf_ref.npz, written by tests/golden/make_svgf_ref.py: the same oracle calls, run once)."""
    s = scenes["cornell"]
    w = h = 200
    z = golden["svgf_ref"]
    assert int(z["iterations"]) == 1024 and int(z["width"]) == w and int(z["height"]) == h and z["move"].tolist() == [F(0.3), F(0.2), 0.0]
    cam_a = _resized(s["camera"], w, h)
    cam_b = moved(cam_a, (0.3, 0.2, 0.0))
    g_a = am.gbuffer_from_oracle(po, cam_a, s["depth"], s["geoms"])
    g_b = am.gbuffer_from_oracle(po, cam_b, s["depth"], s["geoms"])

    def accumulate(tr, upto, keep):
        acc = np.zeros((w * h, 3), dtype=np.float32)
        m1, m2 = np.zeros(w * h, np.float32), np.zeros(w * h, np.float32)
        at = {}
        for it in range(1, upto + 1):
            tr.image[:] = 0
            tr.iterate(it, threads=8)
            acc = (acc + tr.image).astype(np.float32)
            m1, m2 = vm.accumulate(m1, m2, tr.image)
            if it in keep:
                at[it] = (acc.copy(), m1.copy(), m2.copy())
        return acc, at

    _, at_a = accumulate(po.Tracer(s["geoms"], s["materials"], cam_a, s["depth"]), 64, (64,))
    _, at_b = accumulate(po.Tracer(s["geoms"], s["materials"], cam_b, s["depth"]), 4, (1, 2, 4))
    conv = z["mean"].astype(np.float32)
    return dict(w=w, h=h, mats=s["materials"], cam_a=cam_a, cam_b=cam_b, g_a=g_a, g_b=g_b, a=at_a[64], b=at_b, conv=conv)


FILT = (5, 4.0, 0.35, 0.5)
TEMP = dict(max_history=64, ptol=0.1, ntol=0.1)


def _errors(ref, scale=1.0):
    """relative L2 against 1024 spp of the moved view at 1, 2, 4 spp: {spp: (pt_denoise_variance alone, SVGF, pt_denoise_temporal)},
    and SVGF without history at 2 spp; every radiance of both views x scale (sums and M1 by scale, M2 by its square: exact for powers of two)"""
    w, h, k = ref["w"], ref["h"], F(scale)
    nrm, pos = ref["g_b"]["normal"].reshape(h, w, 3), ref["g_b"]["position"].reshape(h, w, 3)
    conv = ref["conv"] * k
    sv, tp = sm.Svgf(w, h, ref["mats"]), tm.Temporal(w, h, ref["mats"])
    acc, m1, m2 = ref["a"]
    sv.call(acc * k, m1 * k, m2 * (k * k), 64, ref["cam_a"], ref["g_a"], *FILT, spatial_below=4, **TEMP)
    tp.call(acc * k, 64, ref["cam_a"], ref["g_a"], *FILT, **TEMP)
    out = {}
    for spp in (1, 2, 4):
        acc, m1, m2 = ref["b"][spp]
        acc, m1, m2 = acc * k, m1 * k, m2 * (k * k)
        alone = vm.denoise(acc.reshape(h, w, 3), m1.reshape(h, w), m2.reshape(h, w), spp, nrm, pos, *FILT).reshape(-1, 3)
        svgf = sv.call(acc, m1, m2, spp, ref["cam_b"], ref["g_b"], *FILT, spatial_below=4, **TEMP)
        temporal = tp.call(acc, spp, ref["cam_b"], ref["g_b"], *FILT, **TEMP)
        out[spp] = (rel_l2(alone, conv), rel_l2(svgf, conv), rel_l2(temporal, conv))
    acc, m1, m2 = ref["b"][2]
    fresh = sm.Svgf(w, h, ref["mats"]).call(acc * k, m1 * k, m2 * (k * k), 2, ref["cam_b"], ref["g_b"], *FILT, spatial_below=4, **TEMP)
    return out, rel_l2(fresh, conv), float((sv.hn > 0).mean())


# measured with this model (the test prints them; DESIGN.md section 6.28 has the table); each bound is the measured ratio + 10 %
#   spp  pt_denoise_variance  SVGF    pt_denoise_temporal      SVGF without history
#    1   1.1134               0.1093  0.1451
#    2   0.2286               0.0863  0.0690                   0.1836
#    4   0.1385               0.0555  0.0517
# SVGF is ahead of pt_denoise_temporal at 1 spp and behind it at 2 and 4 (the temporal filter's sigma_color = 4 suits this scene and
# exposure; under another exposure it does not, see the last test)
MEASURED_SVGF_TO_VARIANCE = {1: 0.0982, 2: 0.3776, 4: 0.4006}
MEASURED_SVGF_TO_TEMPORAL = {1: 0.7536, 2: 1.2515, 4: 1.0741}
MEASURED_SPATIAL_ALONE_2SPP = 0.8034


def test_svgf_after_a_move_against_the_variance_filter_alone_and_the_temporal_filter(cornell_move):
    out, fresh, share = _errors(cornell_move)
    for spp, (alone, svgf, temporal) in out.items():
        print("%d spp after the move: pt_denoise_variance %.4f, SVGF %.4f (ratio %.4f), pt_denoise_temporal %.4f (SVGF / temporal %.4f)"
              % (spp, alone, svgf, svgf / alone, temporal, svgf / temporal))
    print("2 spp, SVGF without history (the spatial fallback alone): %.4f against %.4f (ratio %.4f); share of pixels with history %.3f"
          % (fresh, out[2][0], fresh / out[2][0], share))
    assert 0.5 < share < 0.95
    for spp, (alone, svgf, temporal) in out.items():
        assert svgf < alone
        assert svgf / alone <= 1.1 * MEASURED_SVGF_TO_VARIANCE[spp]
        assert svgf / temporal <= 1.1 * MEASURED_SVGF_TO_TEMPORAL[spp]
    assert fresh < out[2][0] and fresh / out[2][0] <= 1.1 * MEASURED_SPATIAL_ALONE_2SPP


def test_svgf_does_not_care_about_the_exposure(cornell_move):
    """Every radiance and both moment planes of both views x 8 and x 1/8 (M2 x 64 and x 1/64 -- exact): SVGF's error at 2 spp after the
    move stays within 2 %, section 6.27's tolerance for its own test of this kind (the floor 2^-40 is the only term that does not
    scale); pt_denoise_temporal's at its fixed sigma_color is printed beside it."""
    base = _errors(cornell_move)[0][2]
    for name, scale in (("x 8", 8.0), ("x 1/8", 0.125)):
        e = _errors(cornell_move, scale)[0][2]
        print("2 spp after the move %-6s SVGF %.4f (x 1: %.4f), pt_denoise_temporal %.4f (x 1: %.4f)" % (name, e[1], base[1], e[2], base[2]))
        assert abs(e[1] / base[1] - 1) <= 0.02


# ---- 3. before pt_init -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pt():
    ge.load_package().build()
    return ge.load_package()


def test_svgf_entry_points_before_init_name_themselves(pt):
    L = pt.library()
    pt.pathtraceFree()
    prm, tmp = pt.VarianceParams(5, 4.0, 0.35, 0.5), pt.TemporalParams(64, 0.1, 0.1)
    buf = np.zeros(16, dtype=np.float32)
    calls = {"pt_denoise_svgf": lambda: L.pt_denoise_svgf(C.byref(prm), C.byref(tmp), 4, 16, None, None),
             "pt_svgf_history": lambda: L.pt_svgf_history(None, buf.ctypes.data, None, None),
             "pt_svgf_variance": lambda: L.pt_svgf_variance(buf.ctypes.data),
             "pt_svgf_reset": lambda: L.pt_svgf_reset()}
    for name, call in calls.items():
        assert call() == -1, name
        assert name.encode() in L.pt_last_error() and b"not initialised" in L.pt_last_error(), L.pt_last_error()
    assert not buf.any()
    for fn in (lambda: pt.denoise_svgf(16), pt.svgf_history, pt.svgf_variance, pt.svgf_reset):
        with pytest.raises(pt.PtError):
            fn()
