"""Direct lighting that samples the environment map (PT_DIRECT_SKY) on the CPU: the numpy model of
tests/sky_model.py against direct_model.Model where the flag changes nothing, its tables against pt_sky_table, the sampled
directions against the lookup they must invert, the sample's weight against the cosine sampler it replaces, and the estimator
against the plain one it must agree with in expectation.  No GPU; frames of 16 x 16."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import __graft_entry__ as ge  # noqa: E402
import direct_model as dm  # noqa: E402
import environment_model as em  # noqa: E402
import glossy_model as gm  # noqa: E402
import sky_model as sm  # noqa: E402
from gpu_common import _resized, bits, rel_l2  # noqa: E402
from sky_model import SUN_DIR, gradient, sun_sky  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
_cache = {}


@pytest.fixture(scope="module")
def pt():
    p = ge.load_package()
    p.build()
    p.build_host()
    return p


def load(pt, name, w, h):
    key = (name, w, h)
    if key not in _cache:
        s = pt.load_scene(os.path.join(ROOT, "scenes", name + ".txt"))
        _cache[key] = (s.geoms, s.materials, _resized(s.camera, w, h), s.traceDepth)
    return _cache[key]


def one_bright_texel(n, factor, seed=3):
    """Uniform noise in [0.5, 1.5) with ONE texel `factor` times 1."""
    t = np.random.default_rng(seed + n).uniform(0.5, 1.5, (6, n, n, 3)).astype(F32)
    t[2, n // 3, (2 * n) // 3] = F32(factor)
    return t


# ---- where the flag changes nothing -----------------------------------------------------------------------------------------------
def test_without_a_map_the_model_is_the_direct_model(pt, po):
    """No map, and a map that yields no element (black): direct_model.Model bit for bit, final bounce and live counts included."""
    geoms, mats, cam, _ = load(pt, "cornell_two_lamps", 16, 16)
    black = np.zeros((6, 2, 2, 3), dtype=F32)
    for env in (None, black):
        a, b = sm.Model(po, geoms, mats, cam, 2), dm.Model(po, geoms, mats, cam, 2)
        a.set_environment(env)
        b.set_environment(env)
        assert a.sky is None and len(a.table) == len(b.table) == 7
        for it in (1, 2, 3):
            a.iterate(it)
            b.iterate(it)
            assert a.image.tobytes() == b.image.tobytes() and a.live == b.live, it
        assert (a.image != 0).any()
    # the sky-only scene without a map: no light element at all, the plain oracle's iteration (black)
    geoms, mats, cam, _ = load(pt, "open_sky_sun", 16, 16)
    m = sm.Model(po, geoms, mats, cam, 2)
    assert not m.direct
    m.iterate(1)
    assert not m.image.any() and len(m.live) == 0


# ---- the tables -------------------------------------------------------------------------------------------------------------------
def check_tables(pt, texels):
    sky = sm.tables(texels)
    got = pt.sky_table(texels)
    assert sky is not None and got is not None
    row, col = got
    n = sky["n"]
    assert row.shape == (6 * n, 2) and col.shape == (6 * n, n, 2)
    for name, a, b in (("rowcdf", row[:, 0], sky["rowcdf"]), ("rowinv", row[:, 1], sky["rowinv"]),
                       ("colcdf", col[:, :, 0], sky["colcdf"]), ("colinv", col[:, :, 1], sky["colinv"])):
        assert (bits(a) == bits(b)).all(), (name, n, int((bits(a) != bits(b)).sum()))
    # every difference of the rounded tables is > 0: every row and every column can be drawn, every inv is finite
    assert (np.diff(np.concatenate([[0.0], row[:, 0].astype(np.float64)])) > 0).all()
    assert (np.diff(np.concatenate([np.zeros((6 * n, 1)), col[:, :, 0].astype(np.float64)], axis=1), axis=1) > 0).all()
    assert np.isfinite(row[:, 1]).all() and np.isfinite(col[:, :, 1]).all() and row[-1, 0] == 1 and (col[:, -1, 0] == 1).all()
    return sky


@pytest.mark.parametrize("n", [1, 2, 5, 64])
def test_sky_table_equals_the_model(pt, n):
    rng = np.random.default_rng(n)
    check_tables(pt, rng.uniform(0, 2, (6, n, n, 3)).astype(F32))
    check_tables(pt, one_bright_texel(n, 2000.0))
    check_tables(pt, sun_sky(pt, n))
    t = np.zeros((6, n, n, 3), dtype=F32)                                # black rows, and texels that do not count
    t[5, n - 1, n - 1] = (0, 2, 0)
    t[0, 0, 0] = (np.nan, 1, 1)
    if n > 1:
        t[1, 0, 1], t[1, 1, 0] = (np.inf, 0, 0), (-5, 1, 1)
    sky = check_tables(pt, t)
    assert sky["m"][0, 0] == 0 and (n == 1 or (sky["m"][n, 1] == 0 and sky["m"][n + 1, 0] == 0))


def test_sky_table_of_a_large_map_with_a_tiny_sun(pt):
    """n = 1024, one texel 10^6 times the rest: the two 1/17 mixtures keep every row and every column reachable in binary32."""
    n = 1024
    t = np.ones((6, n, n, 3), dtype=F32)
    t[2, 300, 700] = F32(1e6)
    t0 = time.time()
    sky = check_tables(pt, t)
    print("n = 1024: model and pt_sky_table in %.1f s" % (time.time() - t0))
    r = 2 * n + 300
    p_row = 1.0 / float(sky["rowinv"][r])
    p_col = 1.0 / float(sky["colinv"][r, 700])
    assert p_row * p_col > 0.1, (p_row, p_col)                           # the sun's texel draws most of the mass it holds


def test_maps_without_an_element_and_the_refusals(pt):
    L = pt.library()
    for v in (0.0, np.nan, -1.0, np.inf):
        t = np.full((6, 3, 3, 3), v, dtype=F32)
        assert sm.tables(t) is None and pt.sky_table(t) is None
    assert sm.tables(None) is None and pt.sky_table(None) is None
    t = np.ones((6, 2, 2, 3), dtype=F32)
    row, col = np.full((12, 2), -1, F32), np.full((12, 2, 2), -1, F32)
    assert L.pt_sky_table(t.ctypes.data, 2, None, None) == 1            # the outputs are optional
    assert L.pt_sky_table(t.ctypes.data, 2, row.ctypes.data, None) == 1 and (row[:, 0] > 0).all()
    assert L.pt_sky_table(t.ctypes.data, 2, None, col.ctypes.data) == 1 and (col[:, :, 0] > 0).all()
    assert L.pt_sky_table(None, 0, None, None) == 0 and L.pt_sky_table(t.ctypes.data, 0, None, None) == 0
    assert L.pt_sky_table(None, 2, None, None) == -1 and b"null texels" in L.pt_last_error()
    assert L.pt_sky_table(t.ctypes.data, -1, None, None) == -1 and L.pt_sky_table(t.ctypes.data, 1025, None, None) == -1
    row[:] = -1
    assert L.pt_sky_table(np.zeros((6, 2, 2, 3), F32).ctypes.data, 2, row.ctypes.data, None) == 0 and (row == -1).all()   # nothing written


def test_light_table_with_and_without_lamps(pt, po):
    geoms, mats, _, _ = load(pt, "cornell_two_lamps", 16, 16)
    lamps = dm.light_elements(np.ascontiguousarray(geoms).view(po.GEOM_DT), np.ascontiguousarray(mats).view(po.MATERIAL_DT))
    sky = sm.tables(sun_sky(pt, 4))
    both = sm.light_table(lamps, sky)
    assert len(both) == 8 and both["kind"][-1] == sm.SKY and both["geom"][-1] == -1 and both["cdf"][-1] == 1 and both["inv_p"][-1] == 2
    assert (both["cdf"][:7].astype(np.float64) * 2 == lamps["cdf"]).all() and (both["inv_p"][:7] == lamps["inv_p"].astype(np.float64) * 2).all()
    assert both["cdf"][6] == F32(0.5)
    alone = sm.light_table(lamps[:0], sky)
    assert len(alone) == 1 and alone["inv_p"][0] == 1 and alone["cdf"][0] == 1
    assert sm.light_table(lamps, None) is lamps


# ---- the sampler -------------------------------------------------------------------------------------------------------------------
N_DRAWS = 20000


def sky_draws(po, texels, normal, seed, count=N_DRAWS):
    seeds = np.random.default_rng(seed).integers(0, 2 ** 32, count, dtype=np.uint64).astype(np.uint32)
    ns = np.tile(np.asarray(normal, dtype=F32), (count, 1))
    return sm.probe_sky_sample(po, texels, ns, gm.probe_states(po, seeds)) + (seeds,)


@pytest.mark.parametrize("n", [1, 2, 5, 64])
def test_a_sampled_direction_reads_the_texel_drawn(pt, po, n):
    """The sampler inverts the lookup: texel_index(direction) is the texel (r, i) drawn -- except for draws within two float32
    steps of a texel edge (or of the cube's edge, where the major axis changes), which rounding may carry across.  Under 1 %."""
    texels = sun_sky(pt, n) if n > 1 else gradient(pt, 1)
    d, w, texel, info, _ = sky_draws(po, texels, (0, 1, 0), 10 + n, 8000)
    raw = info["raw_dir"]
    k = em.texel_index(raw, n)
    u1, u2, u3, u4 = info["u"]
    s = float(sm.tables(texels)["s"])
    a = (info["i"] + u3.astype(np.float64)) * s - 1.0
    b = ((info["r"] % n) + u4.astype(np.float64)) * s - 1.0
    step = 2 * np.spacing(F32(1))
    edge = np.zeros(len(a), dtype=bool)
    for c in (a, b):
        f = (c + 1.0) / s                                               # texel coordinate: near an integer = near an edge
        edge |= np.abs(f - np.round(f)) * s <= 2 * step
        edge |= np.abs(np.abs(c) - 1.0) <= 2 * step
    wrong = k != texel
    print("n = %d: %d of %d draws near an edge, %d read another texel" % (n, edge.sum(), len(edge), wrong.sum()))
    assert not (wrong & ~edge).any(), np.nonzero(wrong & ~edge)[0][:5]
    assert edge.mean() < 0.01
    assert (texel >= 0).all() and (texel < 6 * n * n).all()
    if n > 1:
        assert len(np.unique(texel // (n * n))) == 6                     # every face is drawn (the mixture sees to the dark ones)
    # a unit vector, and the upper hemisphere of the normal only
    ok = info["ok"]
    assert 0.2 < ok.mean() < 1 and (d[~ok] == 0).all() and (w[~ok] == 0).all() and (w[ok] > 0).all()
    assert np.abs(np.sqrt((d[ok].astype(np.float64) ** 2).sum(axis=1)) - 1).max() < 1e-6 and (d[ok][:, 1] > 0).all()


def test_the_draws_are_the_oracles(pt, po):
    texels = sun_sky(pt, 8)
    _, _, texel, info, seeds = sky_draws(po, texels, (0, 1, 0), 77, 32)
    sky = sm.tables(texels)
    for k, s in enumerate(seeds):
        u = po.u01_sequence(int(s), 5)
        assert [bits(info["u"][j][k:k + 1])[0] for j in range(4)] == list(bits(u[1:]))
        r = next((j for j in range(48) if u[1] < sky["rowcdf"][j]), 47)
        i = next((j for j in range(8) if u[2] < sky["colcdf"][r, j]), 7)
        assert texel[k] == r * 8 + i


def mean_radiance(texels, dirs):
    return em.radiance(texels, dirs).astype(np.float64).mean(axis=1)


@pytest.mark.parametrize("sky_name", ["gradient", "sun"])
@pytest.mark.parametrize("normal", [(0.0, 1.0, 0.0), (-0.6, -0.48, -0.64)], ids=["up", "sun below the horizon"])
def test_weighted_draws_against_the_cosine_sampler(pt, po, sky_name, normal):
    """The mean of w E(d) over 20 000 sky draws against the mean of E under the oracle's cosine hemisphere sampler (both
    estimate the integral of E cos / pi over the normal's hemisphere), within 5 standard errors of the two spreads combined."""
    texels = gradient(pt, 16) if sky_name == "gradient" else sun_sky(pt, 16)
    d, w, _, info, _ = sky_draws(po, texels, normal, 5)
    sun = np.asarray(SUN_DIR) / np.linalg.norm(SUN_DIR)
    assert (np.dot(sun, normal) < -0.5) == (normal[0] < 0)
    a = w.astype(np.float64) * mean_radiance(texels, d)
    seeds = np.random.default_rng(6).integers(0, 2 ** 32, N_DRAWS, dtype=np.uint64).astype(np.uint32)
    dirs, _ = gm.hemisphere(po, np.tile(np.asarray(normal, dtype=F32), (N_DRAWS, 1)), gm.probe_states(po, seeds))
    b = mean_radiance(texels, dirs)
    se = np.sqrt(a.var(ddof=1) / len(a) + b.var(ddof=1) / len(b))
    print("%s, normal %r: sky sampler %.5f +- %.5f, cosine sampler %.5f +- %.5f" %
          (sky_name, normal, a.mean(), np.sqrt(a.var(ddof=1) / len(a)), b.mean(), np.sqrt(b.var(ddof=1) / len(b))))
    assert se > 0 and abs(a.mean() - b.mean()) <= 5 * se
    assert (w >= 0).all() and np.isfinite(w).all() and 0 < info["ok"].mean() < 1


# ---- the estimator --------------------------------------------------------------------------------------------------------------------
def frame_means(model, count, keep):
    out, kept = [], None
    assert not model.image.any()
    prev = model.image.astype(np.float64)
    for it in range(1, count + 1):
        model.iterate(it)
        cur = model.image.astype(np.float64)
        out.append((cur - prev).mean())
        prev = cur
        if it == keep:
            kept = model.image.copy()
    return np.array(out), kept


def open_sky_runs(pt, po):
    """Shared by the tests below: open_sky_sun at 16 x 16 under the sun sky, the flagged model at depth 1 and the plain model
    (direct_model.Model without the flag: the oracle's stages and the miss lookup) at depth 2, 48 iterations each."""
    if "runs" not in _cache:
        geoms, mats, cam, _ = load(pt, "open_sky_sun", 16, 16)
        assert not ((mats["hasReflective"] > 0) | (mats["hasRefractive"] > 0) | (mats["emittance"] > 0)).any()
        texels = sun_sky(pt, 16)
        flagged = sm.Model(po, geoms, mats, cam, 1)
        plain = dm.Model(po, geoms, mats, cam, 2, direct=False)
        flagged.set_environment(texels)
        plain.set_environment(texels)
        assert flagged.direct and len(flagged.table) == 1 and not plain.direct
        a, img_a16 = frame_means(flagged, 48, 16)
        b, img_b16 = frame_means(plain, 48, 16)
        _cache["runs"] = (a, b, img_a16, img_b16, dict(flagged.counts), list(flagged.live))
    return _cache["runs"]


def test_the_flagged_estimator_agrees_with_one_more_plain_bounce(pt, po):
    """E[flags, depth 1] = E[no flag, depth 2] in a scene without specular surfaces, sky light included: the frame means over
    N = 48 iterations agree within 5 standard errors of their difference (from the per-iteration frame means)."""
    a, b, _, _, _, live = open_sky_runs(pt, po)
    se = np.sqrt(a.var(ddof=1) / len(a) + b.var(ddof=1) / len(b))
    print("frame mean: flagged depth 1 %.6f, plain depth 2 %.6f, standard error of the difference %.6f" % (a.mean(), b.mean(), se))
    assert se > 0 and abs(a.mean() - b.mean()) <= 5 * se
    assert len(live) == 2 and live[1] > 0


def test_sixteen_flagged_iterations_are_closer_to_the_converged_image(pt, po, golden):
    """After 16 iterations the flagged depth-1 model is at a relative L2 distance of 0.1691 from the converged plain depth-2
    image (tests/golden/sky_ref.npz; tests/golden/make_sky_ref.py made it) and the plain depth-2 model at 0.7204: a ratio of
    0.235.  The bound is halfway between that and 1."""
    _, _, img_a16, img_b16, _, _ = open_sky_runs(pt, po)
    z = golden["sky_ref"]
    assert z["texels"].tobytes() == sun_sky(pt, 16).tobytes()            # the reference is this scene under this sky
    conv = z["mean"].astype(np.float64)
    ea, eb = rel_l2(img_a16.astype(np.float64) / 16, conv), rel_l2(img_b16.astype(np.float64) / 16, conv)
    print("relative L2 to the converged plain depth-2 image after 16 iterations: flagged depth 1 %.4f, plain depth 2 %.4f (ratio %.3f)"
          % (ea, eb, ea / eb))
    assert ea / eb < (0.235 + 1) / 2


def test_every_branch_is_seen(pt, po):
    """open_sky_sun (the sky alone) and cornell_two_lamps with its front open under the same sky (lamps and sky): sky-aimed and
    lamp-aimed draws, cs <= 0 exits, sky-aimed rays that score and that are occluded, lamp-aimed rays that miss."""
    _, _, _, _, c, _ = open_sky_runs(pt, po)
    print("open_sky_sun 16 x 16, depth 1, 48 iterations: %r" % (c,))
    assert c["sky aimed"] == c["sampled"] > 4000 and c["lamp aimed"] == 0
    assert c["sky cs exits"] > 100 and c["sky scored"] > 1000 and c["sky occluded"] > 100 and c["negative or nan weights"] == 0
    assert c["final rays"] == c["sampled"] - c["sky cs exits"] == c["sky scored"] + c["sky occluded"]
    geoms, mats, cam, _ = load(pt, "cornell_two_lamps", 16, 16)
    m = sm.Model(po, geoms, mats, cam, 2)
    m.set_environment(sun_sky(pt, 16))
    for it in range(1, 7):
        m.iterate(it)
    c = m.counts
    print("cornell_two_lamps 16 x 16, depth 2, 6 iterations: %r; live %r" % (c, m.live))
    assert c["sky aimed"] > 100 and c["lamp aimed"] > 100 and c["sky cs exits"] > 10 and c["step 6"] > 10
    assert c["sky scored"] > 5 and c["sky occluded"] > 50 and c["negative or nan weights"] == 0
    # a lamp-aimed ray that misses needs a lamp no ray can hit: the flat lamp across the open side
    flat = dm.placed(pt.GEOM_DT, dm.CUBE, 0, (0, 5, 4.99), (6, 6, 0), (0, 180, 0))
    m = sm.Model(po, np.concatenate([geoms, flat]), mats, cam, 2)
    m.set_environment(sun_sky(pt, 16))
    for it in range(1, 4):
        m.iterate(it)
    print("... with a flat lamp across the open side: %r" % (m.counts,))
    assert m.counts["lamp missed"] > 10 and m.counts["sky scored"] > 0


# ---- the host code under the sanitizers ---------------------------------------------------------------------------------------------
def test_sky_table_driver_runs_clean_under_the_sanitizers(tmp_path):
    """csrc/pt_lights.hpp compiled into its stand-alone driver with ASan and UBSan and run as a program of its own (nothing
    sanitized is loaded into this process): maps of 1 to 256 texels a side, a sun 10^6 times the rest, black rows, texels that
    are black, NaN, infinite or negative, no map."""
    exe = str(tmp_path / "sky_table_main")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "tools", "sky_table_main.cpp")]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "sky_table_main: ok" in r.stdout and not r.stderr, r.stdout + r.stderr
