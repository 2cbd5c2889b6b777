"""GPU: PT_MOMENTS and pt_denoise_variance on the random hostile scenes of tests/random_scenes.py (arbitrary rotations, slabs,
scales of 100 and 1e-4, an eye inside primitives: a depth discontinuity at nearly every pixel, |position| up to hundreds) -- one
session over the first four filter seeds at 40 x 26: the moments after a batch of two and one pt_trace against
tests/variance_model.py on the oracle's per-sample colours, then pt_denoise_variance at 1 and 5 levels and pt_variance, every
pixel bit for bit.  Under both launch plans."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import __graft_entry__ as ge  # noqa: E402,F401
import random_scenes as rs  # noqa: E402
import variance_model as vm  # noqa: E402
from gpu_common import pt, launch_plan, bits  # noqa: E402,F401

pytestmark = pytest.mark.gpu

W, H = rs.W, rs.H
SIG = (4.0,) + tuple(rs.SIGMAS[1:])
_refs = {}


def reference(po, pt, seed):
    """(running sum, M1, M2) after iterations 1 .. 3 and the model's pictures {levels: (plane, var_0)}: once per seed"""
    if seed not in _refs:
        geoms, mats, cam, depth = rs.scene(pt, seed, W, H)
        tr = po.Tracer(np.ascontiguousarray(geoms).view(po.GEOM_DT), mats.view(po.MATERIAL_DT), cam, depth, flags=po.F_COMPACT, trig=po.TRIG_SHARED)
        acc = np.zeros((W * H, 3), dtype=np.float32)
        m1, m2 = np.zeros(W * H, np.float32), np.zeros(W * H, np.float32)
        for it in (1, 2, 3):
            tr.image[:] = 0
            tr.iterate(it)
            acc = (acc + tr.image).astype(np.float32)
            m1, m2 = vm.accumulate(m1, m2, tr.image)
        g = rs.first_hits(po, pt, seed, W, H)
        nrm, pos = g["normal"].reshape(H, W, 3), g["position"].reshape(H, W, 3)
        with np.errstate(all="ignore"):
            pictures = {lv: vm.denoise(acc.reshape(H, W, 3), m1.reshape(H, W), m2.reshape(H, W), 3, nrm, pos, lv, *SIG).reshape(-1, 3) for lv in (1, 5)}
            v0 = vm.var0(m1, m2, 3)
        _refs[seed] = (acc, m1, m2, pictures, v0)
    return _refs[seed]


def test_moments_and_the_variance_filter_on_random_scenes(pt, po, launch_plan):
    lines = []

    def equal(seed, what, got, want):
        bad = bits(got) != bits(want)
        if bad.any():
            p = int(np.nonzero(bad.reshape(len(got), -1).any(axis=1))[0][0])
            lines.append("seed %d [%s], %s: %d of %d words differ; first pixel %d (x %d, y %d): got %r, want %r" %
                         (seed, launch_plan, what, int(bad.sum()), bad.size, p, p % W, p // W, got[p].tolist(), want[p].tolist()))

    for seed in rs.FILTER_SEEDS[:4]:
        geoms, mats, cam, depth = rs.scene(pt, seed, W, H)
        acc, m1, m2, pictures, v0 = reference(po, pt, seed)
        pt.pathtraceInit(pt.Scene(geoms, mats, cam, depth), flags=pt.PT_COMPACT | pt.PT_MOMENTS, max_batch=2, pin_image=False)
        try:
            pt.trace_batch(1, 2)
            pt.pathtrace(None, 0, 3)
            equal(seed, "running sum", pt.get_image(W * H), acc)
            g1, g2 = pt.get_moments()
            equal(seed, "M1", g1, m1)
            equal(seed, "M2", g2, m2)
            for lv in (1, 5):
                equal(seed, "pt_denoise_variance, %d levels" % lv, pt.denoise_variance(3, lv, *SIG), pictures[lv])
            equal(seed, "pt_variance", pt.variance(), v0)
        finally:
            pt.pathtraceFree()
    assert not lines, "\n".join(lines)
