"""ptd::shade_scatter -- this project's completion of the reference's empty scatterRay (csrc/pt_device.hpp)
-- ON THE DEVICE, one function at a time, through pt_probe_shade_scatter (include/ptmi355.h), in the form the kernels that
sample at once call it and in the deferring form followed by what the next bounce's load does (tile_load<RESOLVE>):

  a. against the oracle's pto_shade_scatter, bit for bit, at the wave and block edges, with every branch populated;
  b. against the REFERENCE's own glm::reflect / glm::refract (tests/golden/glmfuncs.npz), bit for bit;
  c. against physics that needs no oracle: Snell's law, unit length and coplanarity of the refracted direction, no refraction
     beyond the critical angle, Schlick's R(0) at normal incidence, which colour each branch multiplies by;
  d. a furnace through the production pipelines: inside an emitter, a mirror or glass ball changes nothing but its own factor.

The checks themselves are in tests/scatter_common.py; tests/test_scatter_spec_cpu.py runs them on the oracle and pins what
they presuppose (how many fixture rows refract, the branch shares, the bounds)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import __graft_entry__ as ge  # noqa: E402,F401
import scatter_common as sc  # noqa: E402
from gpu_common import pt, launch_plan, bits, _resized  # noqa: E402,F401

pytestmark = pytest.mark.gpu


def _device_shade(pt, deferred):
    def shade(it, depth, materials, paths, isects, outside):
        return pt.probe_shade_scatter(it, depth, materials, paths, isects, outside, deferred=deferred)
    return shade


@pytest.fixture(params=[False, True], ids=["sampled at once", "deferred"])
def shade(pt, request):
    return _device_shade(pt, request.param)


@pytest.fixture(scope="module")
def reference(po):
    """The 4096 records and the oracle's answer under each (iter, depth), computed once (the oracle treats every record on
    its own, so the answer for the first n records is the first n of it)."""
    p, x, outside = sc.records()
    mats = sc.material_table()
    want = {key: sc.oracle_shade(po)(key[0], key[1], mats, p, x, outside) for key in sc.KEYS}
    want[None] = sc.oracle_shade(po)(3, 2, mats, p, x, None)
    for v in want.values():
        v.setflags(write=False)
    return p, x, outside, mats, want


# ---- a. the oracle, bit for bit --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", sc.KEYS, ids=lambda k: "iter %d depth %d" % k)
@pytest.mark.parametrize("n", sc.SIZES)
def test_equals_the_oracle(pt, reference, n, key):
    """color, pixelIndex, remainingBounces of every record and the ray of every path that goes on equal the oracle's; both
    forms return the same bytes; a path that ends keeps the ray it came with; the arguments are not written."""
    p, x, outside, mats, want = reference
    before = p[:n].tobytes()
    got = pt.probe_shade_scatter(key[0], key[1], mats, p[:n], x[:n], outside[:n], deferred=False)
    got_deferred = pt.probe_shade_scatter(key[0], key[1], mats, p[:n], x[:n], outside[:n], deferred=True)
    assert len(got) == n and p[:n].tobytes() == before
    assert got.tobytes() == got_deferred.tobytes()
    sc.assert_same_paths(got, want[key][:n], (n, key))
    ended = got["remainingBounces"] == 0
    assert (bits(got["origin"][ended]) == bits(p[:n]["origin"][ended])).all()
    assert (bits(got["direction"][ended]) == bits(p[:n]["direction"][ended])).all()


def test_outside_defaults_to_one(pt, reference):
    p, x, outside, mats, want = reference
    for deferred in (False, True):
        sc.assert_same_paths(pt.probe_shade_scatter(3, 2, mats, p, x, None, deferred=deferred), want[None])
    assert want[None].tobytes() != want[(3, 2)].tobytes()


def test_every_branch_is_populated(pt, reference):
    """At least 5 % of the 4096 records each: miss, emitter, ended on the last bounce, mirror, glass refracted, glass reflected,
    diffuse -- on the device's own outputs."""
    p, x, outside, mats, want = reference
    for key in sc.KEYS:
        got = pt.probe_shade_scatter(key[0], key[1], mats, p, x, outside)
        share = {k: float(v.mean()) for k, v in sc.branches(p, x, got).items()}
        assert set(share) == set(sc.BRANCHES) and min(share.values()) >= 0.05, share
        untouched = p["remainingBounces"] <= 0
        assert untouched.any() and got[untouched].tobytes() == p[untouched].tobytes()


def test_empty_and_refused_calls(pt, reference):
    """n == 0 is no error; a hit on a material outside the table is refused on the host and nothing runs."""
    p, x, outside, mats, want = reference
    assert len(pt.probe_shade_scatter(1, 0, mats, p[:0], x[:0], outside[:0])) == 0
    y = x[:65].copy()
    y["t"][64], y["materialId"][64] = 1.0, len(mats)
    with pytest.raises(pt.PtError, match="record 64"):
        pt.probe_shade_scatter(1, 0, mats, p[:65], y, outside[:65])
    with pytest.raises(pt.PtError):
        pt.probe_shade_scatter(1, 0, mats, p[:65], x[:64], None)


# ---- b. the reference's own glm --------------------------------------------------------------------------------------------
def test_mirror_equals_glm_reflect(shade, po, golden):
    assert sc.check_glm_mirror(shade, po, golden["glmfuncs"]) == 512


def test_refraction_equals_glm_refract(shade, po, golden):
    """271 fixture rows x engines 0..15: what did not reflect went along glm::refract(I, N, eta), bit for bit, from
    P + I * 0.0002f; the 150 rows of total internal reflection reflect from P under every engine.  At least 100 rows are
    compared with glm::refract (118 on the oracle)."""
    compared, tir = sc.check_glm_refraction(shade, po, golden["glmfuncs"])
    print("rows compared with glm::refract: %d, total internal reflection: %d" % (compared, tir))
    assert compared >= 100 and tir == 150


# ---- c. physics ------------------------------------------------------------------------------------------------------------
def test_snell(shade):
    """Below 4e-6 each (eight times the largest figure measured on the oracle, 5.2e-7 / 6.9e-7 / 6.9e-8: a binary32 chain of about
    ten roundings); no row whose float64 k is below -1e-5 refracts."""
    worst, forbidden, beyond, refracted = sc.snell(shade)
    print("Snell %.2e, unit length %.2e, coplanarity %.2e; %d refracted, %d of %d beyond the critical angle refracted"
          % (worst[0], worst[1], worst[2], refracted, forbidden, beyond))
    assert refracted > 30000 and beyond > 30000
    assert (worst < 4e-6).all()
    assert forbidden == 0


def test_schlick_at_normal_incidence(shade):
    """The reflected share of 65536 engines lies within four binomial standard deviations of ((1 - n) / (1 + n))^2 (four is a
    chosen margin; on the oracle the shares are 0.04025, 0.02014 and 0.16924, within 0.4)."""
    for ior, outside, share, r0, sd in sc.schlick_normal_incidence(shade):
        print("ior %.2f outside %d: reflected %.5f, R(0) %.5f, %.2f sigma" % (ior, outside, share, r0, (share - r0) / sd))
        assert abs(share - r0) <= 4 * sd, (ior, outside)


def test_colours(shade, reference):
    p, x, outside = reference[:3]
    sc.check_colours(shade, p, x, outside)


# ---- d. furnace, through the production pipelines --------------------------------------------------------------------------
SHELLS = pytest.mark.parametrize("shell", [sc.SPHERE, sc.CUBE], ids=["round shell", "cubic shell"])
BALLS = pytest.mark.parametrize("ball", [sc.SPHERE, sc.CUBE], ids=["ball", "turned cube"])
HOW = pytest.mark.parametrize("how", ["pt_trace_batch", "pt_trace"])
N_PIX = sc.FURNACE_SIZE * sc.FURNACE_SIZE


def _session(pt, s, how):
    scene = pt.Scene(s["geoms"], s["materials"], s["camera"], s["depth"])
    pt.pathtraceInit(scene, flags=pt.PT_COMPACT, max_batch=sc.FURNACE_ITERATIONS if how == "pt_trace_batch" else 1)


def _sum_of_32(pt, how):
    if how == "pt_trace_batch":
        pt.trace_batch(1, sc.FURNACE_ITERATIONS)
        return pt.get_image(N_PIX)
    for it in range(1, sc.FURNACE_ITERATIONS + 1):
        img = pt.pathtrace(None, 0, it)
    return np.array(img)


@SHELLS
@BALLS
@HOW
@pytest.mark.parametrize("spec", [1.0, 0.5])
def test_mirror_furnace(pt, scenes, shell, ball, how, spec):
    """specular.color 1: every pixel's sum is 32 x (2, 1, 0.5) exactly.  0.5: the pixels whose first hit (pt_gbuffer) is the
    mirror hold exactly 32 x (1, 0.5, 0.25), all others 32 x (2, 1, 0.5); the mirror covers more than 5 % of the frame."""
    s = sc.furnace_scene(pt, scenes, _resized, shell, ball, sc.material(spec=(spec,) * 3, mirror=1.0))
    _session(pt, s, how)
    try:
        on_ball = pt.gbuffer()["materialId"] == 1
        img = _sum_of_32(pt, how)
    finally:
        pt.pathtraceFree()
    assert on_ball.mean() > 0.05
    want = np.where(on_ball[:, None], np.float32(spec), np.float32(1.0)) * (np.float32(sc.FURNACE_ITERATIONS) * sc.LIGHT)[None, :]
    assert (bits(img) == bits(want)).all()


@SHELLS
@BALLS
@HOW
def test_glass_furnace_one_sample_at_a_time(pt, scenes, shell, ball, how):
    """A glass ball (ior 1.5, specular.color 0.5) inside the emitter, one sample at a time (pt_clear_image, one iteration): off
    the ball every sample is (2, 1, 0.5) exactly; on it the red channel over 2 is 0 or 2^-k, 1 <= k <= 15 -- one factor of
    0.5 per interaction with the glass, up to fifteen before the sixteenth bounce reaches the emitter -- and green and blue
    are red x 0.5 and red x 0.25.

    NOT asserted: that no sample on the ball is 0 (an exact glass furnace).  On the oracle about half of the ball's samples (47 %
    on the sphere, 65 % on the turned cube) end at depth 16 with colour 0: the completion spec's step of 0.0002 along the incoming direction does not always cross the
    surface of a scaled sphere, because getPointOnRay stops 0.0001 short twice (in object space, then along the world ray),
    so a refracted path may meet the surface it has just passed again, from the side it came from.  That is the spec's
    behaviour, which the device reproduces bit for bit (test_gpu_parity), not a device bug."""
    s = sc.furnace_scene(pt, scenes, _resized, shell, ball, sc.material(spec=(0.5,) * 3, glass=1.0, ior=1.5))
    allowed = np.concatenate([[0.0], 2.0 ** -np.arange(1, 16)]).astype(np.float32)
    _session(pt, s, how)
    try:
        on_ball = pt.gbuffer()["materialId"] == 1
        assert on_ball.mean() > 0.05
        for it in range(1, sc.FURNACE_ITERATIONS + 1):
            pt.clear_image()
            if how == "pt_trace_batch":
                pt.trace_batch(it, 1)
                img = pt.get_image(N_PIX)
            else:
                img = np.array(pt.pathtrace(None, 0, it))
            assert (bits(img[~on_ball]) == bits(sc.LIGHT)[None, :]).all(), it
            red = img[on_ball, 0]
            assert np.isin(red * np.float32(0.5), allowed).all(), it
            assert (bits(img[on_ball, 1]) == bits(red * np.float32(0.5))).all(), it
            assert (bits(img[on_ball, 2]) == bits(red * np.float32(0.25))).all(), it
    finally:
        pt.pathtraceFree()
