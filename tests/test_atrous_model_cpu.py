"""The specification of pt_denoise as tests/atrous_model.py models it, checked on the CPU: the
edge-stopping function against float64, the filter's invariants, and that it does what it is for -- a 16-spp Cornell
image is at least twice as close to the converged one after filtering.  Also: the new entry points before pt_init."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import __graft_entry__ as ge  # noqa: E402
import atrous_model as am  # noqa: E402
from gpu_common import _resized, rel_l2  # noqa: E402


def test_exp_neg_against_float64():
    """Dense grid of [0, 25]: within 2^-18 relative of exp(-x) (measured 1.35e-6 = 2^-19.5 on 2 000 001 points; the margin
    covers a grid that lands on a worse point, the Taylor remainder alone is 1e-7)."""
    x = np.linspace(0, 25, 2000001).astype(np.float32)
    e = am.exp_neg(x).astype(np.float64)
    err = float(np.abs(e / np.exp(-x.astype(np.float64)) - 1).max())
    print("exp_neg: largest relative error %.3e (bound %.3e)" % (err, 2.0 ** -18))
    assert err < 2.0 ** -18
    assert e.dtype == np.float64 and am.exp_neg(x).dtype == np.float32


def test_exp_neg_edges():
    one = am.exp_neg(np.zeros(3, dtype=np.float32))
    assert (one.view(np.uint32) == np.float32(1.0).view(np.uint32)).all()          # exp_neg(0) == 1 exactly
    at25 = am.exp_neg(np.array([25.0], dtype=np.float32))
    above = am.exp_neg(np.array([25.000002, 26.0, 1e3, 1e30, np.inf], dtype=np.float32))
    assert (above.view(np.uint32) == at25.view(np.uint32)[0]).all()                # arguments above 25 give exp_neg(25)
    assert float(at25[0]) > 1e-11                                                  # a normal number, far from the denormals
    assert (am.exp_neg(np.linspace(0, 30, 100001).astype(np.float32)) <= 1.0).all()


def _random_gbuffer(rng, h, w):
    nrm = rng.standard_normal((h, w, 3)).astype(np.float32)
    nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True).astype(np.float32)
    pos = (rng.standard_normal((h, w, 3)) * 3).astype(np.float32)
    miss = rng.random((h, w)) < 0.2
    nrm[miss] = 0
    pos[miss] = 0
    return nrm, pos


def test_constant_image_stays_constant():
    """Whatever the G-buffer, a constant image is a fixed point up to the summation's rounding: 25 rounded additions and a
    divide per level, so 26 x 2^-24 relative per level."""
    rng = np.random.default_rng(5)
    h, w = 61, 97
    nrm, pos = _random_gbuffer(rng, h, w)
    for value in (0.73, 3.0e-3, 41.5):
        c0 = np.full((h, w, 3), value, dtype=np.float32)
        c = c0.copy()
        for lv in range(7):
            c = am.level(c, nrm, pos, 1 << lv, np.float32(1.0) * np.float32(2.0 ** -lv), 0.35, 0.5)
            err = float(np.abs(c.astype(np.float64) / np.float64(np.float32(value)) - 1).max())
            bound = (lv + 1) * 26 * 2.0 ** -24
            print("constant %g, level %d: %.3e (bound %.3e)" % (value, lv, err, bound))
            assert err <= bound


def test_zero_levels_is_the_mean_bit_for_bit():
    rng = np.random.default_rng(6)
    h, w = 17, 23
    nrm, pos = _random_gbuffer(rng, h, w)
    s = (rng.random((h, w, 3)) * 40).astype(np.float32)
    got = am.denoise(s, 16, nrm, pos, 0, 1.0, 0.35, 0.5)
    want = s / np.float32(16)
    assert got.dtype == np.float32 and (got.view(np.uint32) == want.view(np.uint32)).all()


def test_weights_respect_edges():
    """Two half-planes with different normals and colours: with a small sigma_normal nothing bleeds across the edge."""
    h, w = 32, 32
    nrm = np.zeros((h, w, 3), np.float32)
    nrm[:, :16, 0] = 1
    nrm[:, 16:, 1] = 1
    pos = np.zeros((h, w, 3), np.float32)
    c = np.zeros((h, w, 3), np.float32)
    c[:, :16] = 0.2
    c[:, 16:] = 0.8
    out = am.denoise(c, 1, nrm, pos, 3, 10.0, 0.05, 1.0)            # |dn|^2 / sn^2 = 2 / 0.0025 -> clamped at 25: weight 1.4e-11
    assert np.abs(out[:, :16] - 0.2).max() < 1e-6 and np.abs(out[:, 16:] - 0.8).max() < 1e-6


def test_rgba8_rule():
    rgb = np.array([[0.0, 1.0, 0.5], [2.0, -1.0, np.nan], [0.999999, 1.0 / 255, np.inf]], dtype=np.float32)
    got = am.rgba8(rgb)
    assert got.tolist() == [[0, 255, 127, 0], [255, 0, 0, 0], [254, 1, 255, 0]]


def test_filtered_16spp_cornell_is_twice_as_close_to_the_converged_image(po, scenes):
    """200x200 Cornell on the oracle: 16 spp against 1024 spp.  levels 5, sigmas 1.0 / 0.35 / 0.5 must at least halve the
    relative L2 error (measured on oracle + model alone: 0.0937 against 0.2811, ratio 0.33)."""
    s = scenes["cornell"]
    w = h = 200
    cam = _resized(s["camera"], w, h)
    g = am.gbuffer_from_oracle(po, cam, s["depth"], s["geoms"])
    miss = float((g["t"] < 0).mean())
    assert 0.05 < miss < 0.5                                         # both branches of the G-buffer are well populated
    tr = po.Tracer(s["geoms"], s["materials"], cam, s["depth"])
    tr.iterate_parallel(1, 16, 8)
    s16 = tr.image.copy()
    tr.iterate_parallel(17, 1024 - 16, 8)
    conv = tr.image / np.float32(1024)
    raw = rel_l2(s16 / np.float32(16), conv)
    dn = am.denoise(s16.reshape(h, w, 3), 16, g["normal"].reshape(h, w, 3), g["position"].reshape(h, w, 3), 5, 1.0, 0.35, 0.5)
    den = rel_l2(dn.reshape(-1, 3), conv)
    print("rel-L2 against 1024 spp: raw %.4f, denoised %.4f, ratio %.3f, miss share %.3f" % (raw, den, den / raw, miss))
    assert den < 0.5 * raw


@pytest.fixture(scope="module")
def pt():
    ge.load_package().build()
    return ge.load_package()


def test_denoise_entry_points_before_init_fail_cleanly(pt):
    L = pt.library()
    pt.pathtraceFree()
    prm = pt.DenoiseParams(5, 1.0, 0.35, 0.5)
    assert L.pt_gbuffer(None, None, None, None) == -1
    assert b"pt_gbuffer" in L.pt_last_error() and b"not initialised" in L.pt_last_error()
    assert L.pt_denoise(C.byref(prm), 16, None, None) == -1
    assert b"pt_denoise" in L.pt_last_error() and b"not initialised" in L.pt_last_error()
    assert L.pt_denoised_device_image() is None
    with pytest.raises(pt.PtError):
        pt.denoise(16)
    with pytest.raises(pt.PtError):
        pt.gbuffer()
