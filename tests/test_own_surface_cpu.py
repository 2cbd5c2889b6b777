"""CPU side of the own-surface form of the cull (tests/own_surface_model.py; the GPU side is
tests/test_gpu_own_surface.py): the launch plan's thresholds, the straight-line row test against the per-mode forms, and
the candidate sets of the two forms."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cull_model  # noqa: E402
import own_surface_model as osm  # noqa: E402


@pytest.fixture(scope="module")
def pt():
    import __graft_entry__ as ge
    p = ge.load_package()
    p.build()
    p.library()
    return p


def test_plan_thresholds(pt):
    """The pid keeps 26 bits for the path and four for geom + 1: batches of up to 2^26 paths, scenes of up to 15 primitives,
    the plain fused compacting pipeline only.  C2 at 64 spp, C3 and C5 at 4 spp are inside."""
    plan = pt.probe_own_surface_plan
    assert plan(1, 1) and plan(1 << 26, 15)
    assert not plan((1 << 26) + 1, 15) and not plan(1 << 26, 16) and not plan(1 << 30, 7) and not plan(1 << 32, 7)
    assert not plan(1000, 0) and not plan(1000, 7, plain_fused=False)
    assert plan(800 * 800 * 64, 7) and plan(59_000_000, 15) and plan(3840 * 2160 * 4, 9)
    assert not plan(3840 * 2160 * 16, 9)


def _random_cubes(pt, rng, n):
    H = pt.host_binding.host_library()
    g = np.zeros(n, dtype=pt.GEOM_DT)
    for k, c in enumerate(g):
        c["type"] = 1 if k % 4 else 0
        c["translation"] = rng.uniform(-4, 4, 3) + (0, 5, 0)
        c["rotation"] = rng.uniform(-180, 180, 3) if k % 3 else (0.0, 0.0, (0.0, 90.0)[k % 2])     # 90 degrees: -4.4e-8 off the diagonal
        sc = rng.uniform(0.3, 4.0, 3)
        if k % 5 == 0:
            sc[rng.integers(3)] = 0.01
        c["scale"] = sc
        H.pth_build_geom_matrices(g.ctypes.data + k * pt.GEOM_DT.itemsize)
    return g


@pytest.mark.parametrize("seed", range(4))
def test_straight_line_row_equals_the_per_mode_forms(pt, seed):
    """For rays leaving random faces of random cubes (outside and inside), own_miss in the straight-line order equals the
    per-primitive form's row test bit for bit, whatever the row's mode (0..2 diagonal, 4 general, 3 none)."""
    rng = np.random.default_rng(40 + seed)
    geoms = _random_cubes(pt, rng, 12)
    _, _, rej = pt.cull_boxes(geoms, (0.0, 5.0, 10.5))
    rays, own = osm.leaving_rays(geoms, rng)
    modes = set()
    fired = 0
    for g in np.unique(own):
        r = rays[own == g]
        a, b = osm.own_miss(r, rej[g, 1:5]), osm.per_mode_miss(r, rej[g])
        assert (a == b).all(), (g, rej[g])
        modes.add(int(rej[g, 0]))
        fired += int(a.sum())
    assert 4 in modes and modes & {0, 1, 2} and fired > 100
    for g in np.flatnonzero(geoms["type"] != 1):                  # spheres: a row of zeros, never a miss
        assert rej[g, 0] == 3 and not osm.own_miss(rays, rej[g, 1:5]).any()


@pytest.mark.parametrize("seed", range(3))
def test_candidates_are_a_superset(pt, seed):
    """Per primitive, the own-surface form keeps every candidate the per-primitive form keeps (it drops only the own
    primitive, by the same statement); what it adds are rays inside ANOTHER primitive's padded box that the row test of that
    primitive would have removed."""
    rng = np.random.default_rng(70 + seed)
    geoms = _random_cubes(pt, rng, 10)
    boxes, rmax, rej = pt.cull_boxes(geoms, (0.0, 5.0, 10.5))
    rays, own = osm.leaving_rays(geoms, rng, per_face=30)
    new = osm.candidates_own(rays, own, boxes.reshape(-1, 2, 3), rmax, rej)
    extra = 0
    for g in range(len(geoms)):
        old, _ = cull_model.candidates(rays, boxes[g].reshape(2, 3), rmax, rej[g])
        assert not (old & ~new[g]).any(), g
        assert (new[g][own == g] == old[own == g]).all(), g       # the own primitive: the same decision
        extra += int((new[g] & ~old).sum())
    assert extra >= 0
