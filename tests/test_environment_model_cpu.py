"""Environment lighting without a GPU: the numpy model of DESIGN.md section 6.16 (tests/environment_model.py) against the
oracle and against itself, and the library's host-only entry points against the model."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import __graft_entry__ as ge  # noqa: E402
import environment_model as em  # noqa: E402
from environment_model import edge_directions, random_directions  # noqa: E402
from gpu_common import bits, _resized  # noqa: E402

W, H = 50, 37


def test_ties_and_edge_directions():
    d, want = edge_directions()
    got = em.texel_index(d, 4)
    assert got.tolist() == want.tolist(), [(d[i].tolist(), int(got[i]), int(want[i])) for i in np.nonzero(got != want)[0]]
    e = em.radiance(np.arange(6 * 4 * 4 * 3, dtype=np.float32).reshape(6, 4, 4, 3) + 1, d)
    assert (e[want < 0] == 0).all() and (e[want >= 0] > 0).all()


def test_lookup_census_reaches_every_texel():
    rng = np.random.default_rng(5)
    k = em.texel_index(random_directions(rng, 200000), 4)
    assert k.min() >= 0 and k.max() == 95
    assert (np.bincount(k, minlength=96) > 0).all()
    for n in (1, 64, 1024):                                        # never outside the map, whatever its size
        k = em.texel_index(random_directions(rng, 20000), n)
        assert k.min() >= 0 and k.max() < 6 * n * n


def test_host_lookup_equals_the_model():
    pt = ge.load_package()
    rng = np.random.default_rng(6)
    d, want = edge_directions()
    assert pt.environment_texel(d, 4).tolist() == want.tolist()
    more = np.concatenate([d, random_directions(rng, 100000)])
    for n in (1, 4, 64, 1024):
        assert (pt.environment_texel(more, n) == em.texel_index(more, n)).all(), n
    assert len(pt.environment_texel(np.zeros((0, 3), np.float32), 4)) == 0
    for bad in (0, -1, 1025):
        with pytest.raises(pt.PtError, match="pt_environment_texel"):
            pt.environment_texel(d, bad)


def test_entry_points_before_pt_init():
    pt = ge.load_package()
    L = pt.library()
    L.pt_free()
    tex = np.ones((6, 1, 1, 3), dtype=np.float32)
    n = C.c_int(-5)
    assert L.pt_set_environment(tex.ctypes.data, 1) == -1                       # PT_ERR_INVALID
    assert b"pt_set_environment" in L.pt_last_error()
    assert L.pt_set_environment(None, 0) == -1
    assert b"pt_set_environment" in L.pt_last_error()
    assert L.pt_get_environment(tex.ctypes.data, 6, C.byref(n)) == -1
    assert b"pt_get_environment" in L.pt_last_error()
    with pytest.raises(pt.PtError, match="pt_set_environment"):
        pt.set_environment(tex)
    with pytest.raises(pt.PtError, match="pt_get_environment"):
        pt.get_environment()


def test_gradient_cubemap_is_the_formula_at_texel_centres():
    pt = ge.load_package()
    z, h, g = (0.2, 0.4, 1.0), (0.9, 0.9, 0.8), (0.3, 0.25, 0.2)
    t = pt.gradient_cubemap(8, z, h, g)
    assert t.shape == (6, 8, 8, 3) and t.dtype == np.float32
    # every texel centre looks itself up, and carries the gradient of its own direction
    c = (np.arange(8) + 0.5) / 8 * 2 - 1
    for face in range(6):
        axis, sign = face >> 1, -1.0 if face & 1 else 1.0
        for j in (0, 3, 7):
            for i in (0, 4, 7):
                v = [0.0, 0.0, 0.0]
                v[axis] = sign
                rest = [k for k in range(3) if k != axis]
                v[rest[0]], v[rest[1]] = c[i], c[j]
                assert em.texel_index(np.array([v], dtype=np.float32), 8)[0] == (face * 8 + j) * 8 + i
                y = v[1] / np.sqrt(v[0] ** 2 + v[1] ** 2 + v[2] ** 2)
                want = np.array(h) + (np.array(z) - h) * max(y, 0.0) + (np.array(g) - h) * max(-y, 0.0)
                assert np.allclose(t[face, j, i], want, rtol=0, atol=1e-6)
    assert (bits(t[2, 3:5, 3:5]) != bits(t[3, 3:5, 3:5])).any()          # zenith and ground differ
    with pytest.raises(pt.PtError):
        pt.gradient_cubemap(0, z, h, g)


def test_model_without_an_environment_is_the_oracle(po, scenes):
    s = scenes["cornell"]
    cam = _resized(s["camera"], W, H)
    ref = po.Tracer(s["geoms"], s["materials"], cam, s["depth"], flags=po.F_COMPACT, trig=po.TRIG_SHARED)
    ref.iterate_parallel(1, 6, 4)
    m = em.Model(po, s["geoms"], s["materials"], cam, s["depth"])
    for it in range(1, 7):
        m.iterate(it)
    assert (bits(m.image) == bits(ref.image)).all()
    assert 0.8 < m.misses / m.paths_ended < 0.9                    # the open box: most paths end in a miss


@pytest.mark.parametrize("n", [1, 4, 64])
def test_a_random_map_changes_almost_every_pixel(po, scenes, n):
    s = scenes["cornell"]
    cam = _resized(s["camera"], W, H)
    rng = np.random.default_rng(40 + n)
    black = em.Model(po, s["geoms"], s["materials"], cam, s["depth"])
    lit = em.Model(po, s["geoms"], s["materials"], cam, s["depth"])
    lit.set_environment(rng.uniform(0, 2, (6, n, n, 3)).astype(np.float32))
    for it in range(1, 7):
        black.iterate(it)
        lit.iterate(it)
    changed = (bits(black.image) != bits(lit.image)).any(axis=1).mean()
    assert changed > 0.95, changed


def test_furnace(po, scenes):
    """Floor and mirror ball under a constant environment of 1: nothing emits and nothing absorbs more than a surface's
    albedo, so a pixel after k iterations holds at most k -- exactly k where the camera ray sees the sky."""
    s = scenes["cornell"]
    cam = _resized(s["camera"], W, H)
    geoms = s["geoms"][[1, 6]]
    m = em.Model(po, geoms, s["materials"], cam, s["depth"])
    m.set_environment(np.ones((6, 2, 2, 3), dtype=np.float32))
    k = 4
    for it in range(1, k + 1):
        m.iterate(it)
    assert m.image.max() == k and m.image.min() >= 0
    first, _ = po.compute_intersections(po.generate_rays(cam, s["depth"]), geoms.view(po.GEOM_DT))
    sky = ~(first["t"] > 0)
    assert sky.any() and (m.image[sky] == k).all()
    assert (m.image[~sky] < k).all() and m.image[~sky].mean() > 0.5 * k
