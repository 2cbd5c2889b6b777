"""The completion of scatterRay on the ORACLE, held against evidence that is not the oracle: the reference's
own glm::reflect / glm::refract vectors (tests/golden/glmfuncs.npz), Snell's law, Schlick's R(0) and a furnace.  These pin the
conditions tests/test_gpu_scatter_probe.py relies on when it runs the same checks (tests/scatter_common.py) on the device through
pt_probe_shade_scatter -- how many fixture rows refract, that every branch of the record set is populated, that the furnace is
exact where it is asserted to be.  Also: pt_probe_shade_scatter's refusals, which need no device."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import __graft_entry__ as ge  # noqa: E402
import scatter_common as sc  # noqa: E402
from gpu_common import _resized  # noqa: E402


@pytest.fixture(scope="module")
def pt():
    ge.load_package().build()
    return ge.load_package()


def test_mirror_rows_equal_glm_reflect(po, golden):
    assert sc.check_glm_mirror(sc.oracle_shade(po), po, golden["glmfuncs"]) == 512


def test_refraction_rows_equal_glm_refract(po, golden):
    """271 rows have the face-forward normal N; 150 of them are total internal reflection, and of the other 121 all but a few
    refract under one of the sixteen engines: at least 100 rows are compared with glm::refract."""
    z = golden["glmfuncs"]
    rows, tir = sc.glm_refraction_rows(z)
    assert len(rows) == 271 and int(tir.sum()) == 150
    compared, n_tir = sc.check_glm_refraction(sc.oracle_shade(po), po, z)
    print("rows compared with glm::refract: %d, total internal reflection: %d" % (compared, n_tir))
    assert compared >= 100 and n_tir == 150


def test_every_branch_is_populated(po):
    """The record set of the bit-for-bit GPU test: each of the seven branches takes at least 5 % of the 4096 records under
    every (iter, depth) the test runs."""
    p, x, outside = sc.records()
    for it, depth in sc.KEYS:
        out = sc.oracle_shade(po)(it, depth, sc.material_table(), p, x, outside)
        share = {k: float(v.mean()) for k, v in sc.branches(p, x, out).items()}
        print(it, depth, " ".join("%s %.3f" % kv for kv in share.items()))
        assert set(share) == set(sc.BRANCHES) and min(share.values()) >= 0.05, share
        untouched = p["remainingBounces"] <= 0
        assert untouched.any() and out[untouched].tobytes() == p[untouched].tobytes()


def test_snell_schlick_and_colours(po):
    """The bounds of the GPU test, on the oracle (4e-6: a binary32 chain of about ten roundings; four standard deviations)."""
    shade = sc.oracle_shade(po)
    worst, forbidden, beyond, refracted = sc.snell(shade)
    print("Snell %.2e, unit length %.2e, coplanarity %.2e; %d refracted, %d of %d beyond the critical angle refracted"
          % (worst[0], worst[1], worst[2], refracted, forbidden, beyond))
    assert refracted > 30000 and beyond > 30000
    assert (worst < 4e-6).all() and forbidden == 0
    for ior, outside, share, r0, sd in sc.schlick_normal_incidence(shade):
        print("ior %.2f outside %d: reflected %.5f, R(0) %.5f, %.2f sigma" % (ior, outside, share, r0, (share - r0) / sd))
        assert abs(share - r0) <= 4 * sd
    sc.check_colours(shade, *sc.records())


@pytest.mark.parametrize("ball", [sc.SPHERE, sc.CUBE], ids=["ball", "turned cube"])
@pytest.mark.parametrize("shell", [sc.SPHERE, sc.CUBE], ids=["round shell", "cubic shell"])
def test_mirror_furnace_on_the_oracle(pt, po, scenes, shell, ball):
    """Inside an emitter, around a mirror: with specular.color 1 every pixel's sum is 32 x (2, 1, 0.5) exactly; with 0.5 the
    pixels whose first hit is the mirror hold exactly half of that, and they are more than 5 % of the frame."""
    for spec in (1.0, 0.5):
        s = sc.furnace_scene(pt, scenes, _resized, shell, ball, sc.material(spec=(spec,) * 3, mirror=1.0))
        tr = po.Tracer(s["geoms"].view(po.GEOM_DT), s["materials"].view(po.MATERIAL_DT), s["camera"], s["depth"], flags=po.F_COMPACT,
                       trig=po.TRIG_SHARED)
        first, _ = po.compute_intersections(po.generate_rays(s["camera"][0], s["depth"]), s["geoms"].view(po.GEOM_DT))
        assert (first["t"] > 0).all()
        on_ball = first["materialId"] == 1
        tr.iterate_parallel(1, sc.FURNACE_ITERATIONS, 8)
        want = np.where(on_ball[:, None], np.float32(spec), np.float32(1.0)) * (np.float32(sc.FURNACE_ITERATIONS) * sc.LIGHT)[None, :]
        assert want.dtype == np.float32 and on_ball.mean() > 0.05
        assert (sc.bits(tr.image) == sc.bits(want)).all()


def test_probe_refuses_bad_arguments_without_a_device(pt):
    """Everything pt_probe_shade_scatter refuses is refused on the host, before a device is looked for; a valid call without a
    device fails with PT_ERR_DEVICE (there is no CPU fallback), with one it runs."""
    import torch
    L = pt.library()
    mats = sc.material_table().view(pt.MATERIAL_DT)
    p, x, outside = sc.records(64)

    def ptr(a):
        return None if a is None else a.ctypes.data_as(C.c_void_p)

    def call(n=64, nm=len(mats), deferred=0, m=mats, null_paths=False, isects=x, out=outside):
        q = p.copy()
        return L.pt_probe_shade_scatter(1, 0, ptr(m), nm, None if null_paths else ptr(q), ptr(isects), ptr(out), n, deferred), q

    for kw in ({"n": -1}, {"nm": 0}, {"nm": -3}, {"deferred": 2}, {"deferred": -1}, {"m": None}, {"null_paths": True}, {"isects": None}):
        rc, q = call(**kw)
        assert rc == -1 and b"pt_probe_shade_scatter" in L.pt_last_error(), kw
        assert q.tobytes() == p.tobytes()
    for bad in (len(mats), -1, 2 ** 31 - 1):                    # a hit on a material outside the table: never launched
        y = x.copy()
        y["t"][37], y["materialId"][37] = 2.0, bad
        rc, q = call(isects=y)
        assert rc == -1 and b"record 37" in L.pt_last_error() and q.tobytes() == p.tobytes(), bad
    y = x.copy()
    y["t"][37], y["materialId"][37] = -1.0, 999                 # a miss reads no material
    assert call(n=0, m=None, null_paths=True, isects=None, out=None)[0] == 0       # nothing to do: nothing launched
    rc, q = call(isects=y)
    if torch.cuda.is_available():
        assert rc == 0 and q["remainingBounces"][37] == 0
    else:
        assert rc == -2 and b"no HIP device" in L.pt_last_error() and q.tobytes() == p.tobytes()
        with pytest.raises(pt.PtError):
            pt.probe_shade_scatter(1, 0, mats, p, x, outside)
