"""The specification of PT_MOMENTS / pt_denoise_variance as tests/variance_model.py models it, checked on
the CPU: the filter's invariants, the one-pass moments against float64, and that it does what it is for -- on oracle and model
alone, a filter whose stop is the pixel's own measured noise beats pt_denoise's constant stop at low sample counts and does not
care about the exposure.  Also: the four new entry points before pt_init."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import __graft_entry__ as ge  # noqa: E402
import atrous_model as am  # noqa: E402
import variance_model as vm  # noqa: E402
from gpu_common import _resized, rel_l2  # noqa: E402

F = np.float32


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _random_gbuffer(rng, h, w):
    nrm = rng.standard_normal((h, w, 3)).astype(np.float32)
    nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True).astype(np.float32)
    pos = (rng.standard_normal((h, w, 3)) * 3).astype(np.float32)
    miss = rng.random((h, w)) < 0.2
    nrm[miss] = 0
    pos[miss] = 0
    return nrm, pos


# ---- the model's invariants ---------------------------------------------------------------------------------------------
def test_constant_image_stays_constant_whatever_the_moments():
    """Whatever the G-buffer and the variance plane, a constant image is a fixed point up to the summation's rounding: 25 rounded
    additions and a divide per level, 26 x 2^-24 relative per level (the bound of test_atrous_model_cpu.py)."""
    rng = np.random.default_rng(15)
    h, w = 37, 53
    nrm, pos = _random_gbuffer(rng, h, w)
    for value in (0.73, 3.0e-3, 41.5):
        c = np.full((h, w, 3), value, dtype=np.float32)
        var = (rng.random((h, w)) * (value * value)).astype(np.float32)
        var[rng.random((h, w)) < 0.3] = 0                      # (pixels without measured noise: the floor)
        for lv in range(6):
            c, var = vm.level(c, var, nrm, pos, 1 << lv, 4.0, 0.35, 0.5)
            err = float(np.abs(c.astype(np.float64) / np.float64(F(value)) - 1).max())
            bound = (lv + 1) * 26 * 2.0 ** -24
            print("constant %g, level %d: %.3e (bound %.3e)" % (value, lv, err, bound))
            assert err <= bound
            assert np.isfinite(var).all() and (var >= 0).all()


def test_zero_levels_is_the_mean_and_var0_bit_for_bit():
    rng = np.random.default_rng(16)
    h, w = 17, 23
    nrm, pos = _random_gbuffer(rng, h, w)
    s = (rng.random((h, w, 3)) * 40).astype(np.float32)
    m1 = (rng.random((h, w)) * 40).astype(np.float32)
    m2 = (m1 * m1 / F(16) * (1 + rng.random((h, w)))).astype(np.float32)
    got, var = vm.denoise(s, m1, m2, 16, nrm, pos, 0, 4.0, 0.35, 0.5, with_var=True)
    assert got.dtype == np.float32 and (bits(got) == bits(s / F(16))).all()
    mu = m1 / F(16)
    want = np.fmax(m2 / F(16) - mu * mu, F(0)) / F(15)
    assert var.dtype == np.float32 and (bits(var) == bits(want)).all() and (var > 0).any()


def test_variance_of_a_flat_region_shrinks_by_the_kernels_sum_of_squares():
    """Constant colour, constant variance, a flat G-buffer: every weight is 1, so var' = var * sum wt^2 / (sum wt)^2 of the B3
    kernel -- (1/256 + 1/16 + 9/64 + 1/16 + 1/256)^2 = 0.2734375^2 -- wherever no tap leaves the image; 25 products, 50 rounded
    additions, a product and a divide: 80 x 2^-24 relative."""
    h, w = 24, 31
    c = np.full((h, w, 3), 0.6, dtype=np.float32)
    var = np.full((h, w), 0.0123, dtype=np.float32)
    nrm = np.zeros((h, w, 3), np.float32)
    nrm[..., 1] = 1
    pos = np.zeros((h, w, 3), np.float32)
    for step in (1, 2, 4):
        c2, v2 = vm.level(c, var, nrm, pos, step, 4.0, 0.35, 0.5)
        inner = v2[2 * step:h - 2 * step, 2 * step:w - 2 * step].astype(np.float64)
        want = float(F(0.0123)) * 0.2734375 ** 2
        err = float(np.abs(inner / want - 1).max())
        print("step %d: %.3e (bound %.3e)" % (step, err, 80 * 2.0 ** -24))
        assert inner.size > 0 and err <= 80 * 2.0 ** -24
        assert (v2 >= inner.min() * (1 - 1e-6)).all()          # fewer taps at the border average less, never more


def test_noise_free_pixels_have_variance_zero():
    """M2 = M1^2 / n exactly representable: var_0 is exactly 0 -- directly, and through two equal samples (M2 / 2 = fl(l * l) = mu * mu)."""
    m1 = np.array([4.0, 1.0, 0.0], dtype=np.float32)
    m2 = np.array([2.0, 0.125, 0.0], dtype=np.float32)          # n = 8: l = 0.5, 0.125, 0
    assert (bits(vm.var0(m1, m2, 8)) == 0).all()
    rng = np.random.default_rng(17)
    c = (rng.random((500, 3)) * 3).astype(np.float32)
    a, b = vm.moments([c, c])
    assert (bits(vm.var0(a, b, 2)) == 0).all() and (a > 0).all()
    one = vm.moments([c])
    assert (bits(vm.var0(one[0], one[1], 1)) == 0).all()       # one sample: M2 = fl(l * l) = mu * mu, exactly 0


def test_moments_against_float64():
    """var_0 from the one-pass binary32 moments against float64 on the same luminances.  With u = 2^-24, S2 = mean of l^2 and
    s2 = S2 - mean^2: M2 carries n + 1 roundings per term (the product, n additions), M2 / n one more -- (n + 2) u S2 --; mu = M1 / n
    carries n + 1, its square 2 n + 3 -- times mean^2 <= S2 --; the subtraction, the divide by n - 1 and the conversion of n - 1 add
    3 u of the result.  So |var_0 / exact - 1| <= ((3 n + 5) S2 / s2 + 3) u to first order: the bound below with 1 / (1 - k u) for
    the higher orders.  S2 / s2 is the condition number of the one-pass formula; the samples are gamma-like, as a path tracer's."""
    rng = np.random.default_rng(18)
    u = 2.0 ** -24
    for n in (2, 5, 16, 64, 300):
        cols = [(rng.gamma(0.7, 1.5, (2000, 3)) * (rng.random((2000, 1)) < 0.8)).astype(np.float32) for _ in range(n)]
        m1, m2 = vm.moments(cols)
        got = vm.var0(m1, m2, n).astype(np.float64)
        L = np.stack([vm.lum(c) for c in cols]).astype(np.float64)          # the binary32 luminances: the moments' input
        S2, mean = (L * L).mean(axis=0), L.mean(axis=0)
        s2 = S2 - mean * mean
        exact = s2 / max(n - 1, 1)
        ok = s2 > 8 * (3 * n + 5) * u * S2                                   # k u < 1 / 4: where the bound says anything at all
        k = (3 * n + 5) * S2[ok] / s2[ok] + 3
        bound = k * u / (1 - k * u)
        err = np.abs(got[ok] / exact[ok] - 1)
        print("n = %d: largest error / bound %.3f over %d pixels (largest error %.3e)" % (n, float((err / bound).max()), int(ok.sum()), float(err.max())))
        assert ok.sum() > 1500 and (err <= bound).all()


# ---- quality, on oracle and model alone -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cornell_200(po, scenes):
    """200 x 200 Cornell on the oracle (the setup of test_filtered_16spp_cornell_...): per-sample colours from one iteration into a
    zeroed image, the running sum and the moments after 2, 4, 16 and 64 of them, and the mean of 1024."""
    s = scenes["cornell"]
    w = h = 200
    cam = _resized(s["camera"], w, h)
    g = am.gbuffer_from_oracle(po, cam, s["depth"], s["geoms"])
    tr = po.Tracer(s["geoms"], s["materials"], cam, s["depth"])
    acc = np.zeros((w * h, 3), dtype=np.float32)
    m1, m2 = np.zeros(w * h, np.float32), np.zeros(w * h, np.float32)
    at = {}
    for it in range(1, 65):
        tr.image[:] = 0
        tr.iterate(it, threads=8)
        acc = (acc + tr.image).astype(np.float32)
        m1, m2 = vm.accumulate(m1, m2, tr.image)
        if it in (2, 4, 16, 64):
            at[it] = (acc.copy(), m1.copy(), m2.copy())
    tr.image[:] = acc
    tr.iterate_parallel(65, 1024 - 64, 8)
    conv = tr.image / F(1024)
    return dict(w=w, h=h, nrm=g["normal"].reshape(h, w, 3), pos=g["position"].reshape(h, w, 3), at=at, conv=conv)


def _errors(ref, spp, scale=1.0):
    """(raw, pt_denoise at its documented sigmas, variance-guided at sigma_l = 4) relative L2 against 1024 spp"""
    w, h = ref["w"], ref["h"]
    acc, m1, m2 = ref["at"][spp]
    k = F(scale)
    acc, m1, m2, conv = acc * k, m1 * k, m2 * (k * k), ref["conv"] * k
    raw = rel_l2(acc / F(spp), conv)
    plain = am.denoise(acc.reshape(h, w, 3), spp, ref["nrm"], ref["pos"], 5, 1.0, 0.35, 0.5)
    guided = vm.denoise(acc.reshape(h, w, 3), m1.reshape(h, w), m2.reshape(h, w), spp, ref["nrm"], ref["pos"], 5, 4.0, 0.35, 0.5)
    return raw, rel_l2(plain.reshape(-1, 3), conv), rel_l2(guided.reshape(-1, 3), conv)


def test_variance_guided_filter_against_pt_denoise_on_cornell(cornell_200):
    """Relative L2 against 1024 spp, levels 5, pt_denoise at 1.0 / 0.35 / 0.5, variance-guided at 4 / 0.35 / 0.5.  The issue's
    prototype (an additive 2^-20 where the final model has a floor) measured:
        spp   raw     pt_denoise  variance-guided  ratio
         2    0.798   0.778       0.233
         4    0.568   0.458       0.136            0.30   (asserted <= 0.5)
        16    0.281   0.0937      0.0708           0.76   (asserted <= 0.9)
        64    0.135   0.0430      0.0452           1.05   (asserted <= 1.15)
    The final model's values are printed by this test and stand in DESIGN.md section 6.27."""
    out = {spp: _errors(cornell_200, spp) for spp in (2, 4, 16, 64)}
    for spp, (raw, plain, guided) in out.items():
        print("%3d spp: raw %.4f, pt_denoise %.4f, variance-guided %.4f, ratio %.3f" % (spp, raw, plain, guided, guided / plain))
    assert out[16][2] <= 0.9 * out[16][1]
    assert out[4][2] <= 0.5 * out[4][1]
    assert out[64][2] <= 1.15 * out[64][1]


def test_variance_guided_filter_does_not_care_about_the_exposure(cornell_200):
    """The 16-spp picture with every radiance x 8 and x 1/8 (sum and M1 scaled by 8, M2 by 64, and their inverses -- exact): the
    variance-guided error stays within 2 % (the floor 2^-40 is the only term that does not scale; the prototype's values were equal
    to four digits), while pt_denoise's constant stop meets another picture: under the brighter lamp its error is more than 1.5 x
    the unscaled one (prototype: 0.278 against 0.0937; under the dimmer lamp 0.0762, the stop then over-blurs a little less)."""
    base = _errors(cornell_200, 16)
    bright, dim = _errors(cornell_200, 16, 8.0), _errors(cornell_200, 16, 0.125)
    for name, e in (("x 1", base), ("x 8", bright), ("x 1/8", dim)):
        print("16 spp %-6s raw %.4f, pt_denoise %.4f, variance-guided %.4f" % (name, e[0], e[1], e[2]))
    for e in (bright, dim):
        assert abs(e[2] / base[2] - 1) <= 0.02
    assert bright[1] > 1.5 * base[1]


# ---- the entry points before pt_init ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pt():
    ge.load_package().build()
    return ge.load_package()


def test_variance_entry_points_before_init_name_themselves(pt):
    L = pt.library()
    pt.pathtraceFree()
    prm = pt.VarianceParams(5, 4.0, 0.35, 0.5)
    buf = np.zeros(16, dtype=np.float32)
    calls = {"pt_get_moments": lambda: L.pt_get_moments(buf.ctypes.data, buf.ctypes.data),
             "pt_set_moments": lambda: L.pt_set_moments(buf.ctypes.data, buf.ctypes.data),
             "pt_denoise_variance": lambda: L.pt_denoise_variance(C.byref(prm), 16, None, None),
             "pt_variance": lambda: L.pt_variance(buf.ctypes.data)}
    for name, call in calls.items():
        assert call() == -1, name
        assert name.encode() in L.pt_last_error() and b"not initialised" in L.pt_last_error(), L.pt_last_error()
    assert not buf.any()
    for fn in (pt.get_moments, pt.variance, lambda: pt.denoise_variance(16), lambda: pt.set_moments(buf, buf)):
        with pytest.raises(pt.PtError):
            fn()
    assert pt.PT_MOMENTS == 1 << 17 and C.sizeof(pt.VarianceParams) == 16
