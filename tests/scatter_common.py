"""What tests/test_gpu_scatter_probe.py (the device, through pt_probe_shade_scatter) and tests/test_scatter_spec_cpu.py (the
oracle) share: the records, and the checks that rest on something other than the oracle -- the reference's own glm vectors
(tests/golden/glmfuncs.npz), Snell's law, Schlick's R(0), the furnace.  Every check takes a `shade` callable
(iter, depth, materials, paths, isects, outside) -> paths afterwards, so the same assertions run on both."""
import ctypes as C

import numpy as np

# byte-compatible with the package's and the oracle's dtypes of the same names
MATERIAL_DT = np.dtype([("color", "<f4", 3), ("spec_exponent", "<f4"), ("spec_color", "<f4", 3),
                        ("hasReflective", "<f4"), ("hasRefractive", "<f4"),
                        ("indexOfRefraction", "<f4"), ("emittance", "<f4")])
PATH_DT = np.dtype([("origin", "<f4", 3), ("direction", "<f4", 3), ("color", "<f4", 3),
                    ("pixelIndex", "<i4"), ("remainingBounces", "<i4")])
ISECT_DT = np.dtype([("t", "<f4"), ("normal", "<f4", 3), ("materialId", "<i4")])

IORS = (1.5, 1.33, 2.4)
EMITTER, DIFFUSE, MIRROR, GLASS0 = 0, 1, 2, 3        # GLASS0 + k: glass of IORS[k]
SIZES = (1, 63, 64, 65, 4096)                        # partial and full waves and blocks
KEYS = ((1, 0), (3, 2), (100000, 7))                 # (iter, depth)
BRANCHES = ("miss", "emitter", "last bounce", "mirror", "glass refracted", "glass reflected", "diffuse")


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def material(color=(1, 1, 1), spec=(1, 1, 1), mirror=0.0, glass=0.0, ior=0.0, emittance=0.0):
    m = np.zeros(1, dtype=MATERIAL_DT)
    m["color"], m["spec_color"] = color, spec
    m["hasReflective"], m["hasRefractive"], m["indexOfRefraction"], m["emittance"] = mirror, glass, ior, emittance
    return m


def material_table():
    """One emitter, one diffuse, one mirror, glass at 1.5 / 1.33 / 2.4; mirror and glass with a specular colour that is not
    their colour, so that a mixed-up colour shows."""
    rows = [material(color=(1.0, 0.9, 0.8), emittance=5.0), material(color=(0.7, 0.6, 0.5)),
            material(color=(0.2, 0.3, 0.4), spec=(0.9, 0.8, 0.7), mirror=1.0)]
    for k, ior in enumerate(IORS):
        rows.append(material(color=(0.3, 0.2, 0.1), spec=(0.95 - 0.1 * k, 0.85, 0.75 + 0.1 * k), glass=1.0, ior=ior))
    return np.concatenate(rows)


def unit_vectors(rng, n):
    v = rng.standard_normal((n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def records(n=4096, seed=20260117):
    """(paths, isects, outside) from a fixed seed: unit normals, unit incoming directions with both signs of dot(I, n), hits
    and misses (t = -1), outside 0 and 1, remainingBounces in {0, 1, 2, 8}, any int32 for a pixelIndex.  A shorter set is
    a prefix of the longest one."""
    rng = np.random.default_rng(seed)
    p = np.zeros(n, dtype=PATH_DT)
    x = np.zeros(n, dtype=ISECT_DT)
    p["origin"] = rng.uniform(-10, 10, (n, 3)).astype(np.float32)
    p["direction"] = unit_vectors(rng, n)
    p["color"] = rng.uniform(0.05, 1.0, (n, 3)).astype(np.float32)
    p["pixelIndex"] = rng.integers(-2 ** 31, 2 ** 31, n, dtype=np.int64).astype(np.int32)
    p["remainingBounces"] = rng.choice(np.array([0, 1, 2, 8], dtype=np.int32), n, p=[0.08, 0.12, 0.4, 0.4])
    x["normal"] = unit_vectors(rng, n)
    x["t"] = np.where(rng.random(n) < 0.1, -1.0, rng.uniform(0.5, 20.0, n)).astype(np.float32)
    x["materialId"] = rng.choice(np.arange(6, dtype=np.int32), n, p=[0.1, 0.15, 0.15, 0.2, 0.2, 0.2])
    outside = (rng.random(n) < 0.5).astype(np.uint8)
    return p, x, outside


def face_forward(I, n):
    """float64: the normal that opposes I."""
    I, n = I.astype(np.float64), n.astype(np.float64)
    return np.where(((I * n).sum(1) > 0)[:, None], -n, n)


def branches(paths, isects, out):
    """Which branch of the shader each record took, from the inputs and -- for glass, where the engine decides -- from the side
    of the surface the new direction points to (float64)."""
    rb, t, m = paths["remainingBounces"], isects["t"], isects["materialId"]
    live, hit = rb > 0, isects["t"] > 0
    scat = live & hit & (m != EMITTER) & (rb > 1)
    through = (out["direction"].astype(np.float64) * face_forward(paths["direction"], isects["normal"])).sum(1) < 0
    return {"miss": live & ~hit, "emitter": live & hit & (m == EMITTER), "last bounce": live & hit & (m != EMITTER) & (rb == 1),
            "mirror": scat & (m == MIRROR), "glass refracted": scat & (m >= GLASS0) & through,
            "glass reflected": scat & (m >= GLASS0) & ~through, "diffuse": scat & (m == DIFFUSE)}


def oracle_shade(po):
    def shade(it, depth, materials, paths, isects, outside):
        out = np.array(paths, dtype=po.PATH_DT, copy=True)
        m = np.ascontiguousarray(materials).view(po.MATERIAL_DT)
        x = np.ascontiguousarray(isects).view(po.ISECT_DT)
        o = None if outside is None else np.ascontiguousarray(outside, dtype=np.uint8)
        po.lib().pto_shade_scatter(it, depth, len(out), po._p(x), po._p(o), po._p(out), po._p(m), po.TRIG_SHARED)
        return out.view(PATH_DT)
    return shade


def assert_same_paths(got, want, what=""):
    """color, pixelIndex and remainingBounces of every path; the ray of the paths that go on (a path that ends keeps the ray
    it came with on the device, while the oracle scatters before it zeroes a last-bounce path)."""
    assert (got["remainingBounces"] == want["remainingBounces"]).all(), what
    assert (got["pixelIndex"] == want["pixelIndex"]).all(), what
    assert (bits(got["color"]) == bits(want["color"])).all(), what
    on = want["remainingBounces"] > 0
    assert (bits(got["origin"][on]) == bits(want["origin"][on])).all(), what
    assert (bits(got["direction"][on]) == bits(want["direction"][on])).all(), what


# ---- the reference's own glm (tests/golden/glmfuncs.npz: I, N, eta, reflect, refract) ------------------------------------
def _glm_paths(z, rows, seeds, rng):
    """One record per (row, seed): the row's I from a random origin, hit at a random distance on a surface of normal N."""
    k = len(seeds)
    p = np.zeros(len(rows) * k, dtype=PATH_DT)
    x = np.zeros(len(p), dtype=ISECT_DT)
    p["origin"] = np.repeat(rng.uniform(-10, 10, (len(rows), 3)).astype(np.float32), k, axis=0)
    p["direction"] = np.repeat(z["I"][rows], k, axis=0)
    p["color"] = 1.0
    p["pixelIndex"] = np.tile(np.asarray(seeds, dtype=np.int32), len(rows))
    p["remainingBounces"] = 8
    x["t"] = np.repeat(rng.uniform(0.5, 20.0, len(rows)).astype(np.float32), k)
    x["normal"] = np.repeat(z["N"][rows], k, axis=0)
    return p, x


def point_on_ray(po, paths, isects):
    """getPointOnRay (intersections.h:27-29) by the oracle's transcription, which tests/test_oracle_golden.py holds against the
    reference's own on the same fixture."""
    out = np.zeros((len(paths), 3), dtype=np.float32)
    L = po.lib()
    for i in range(len(paths)):
        v = L.pto_get_point_on_ray(po.ray(paths["origin"][i], paths["direction"][i]), C.c_float(isects["t"][i]))
        out[i] = (v.x, v.y, v.z)
    return out


def check_glm_mirror(shade, po, z):
    """All 512 rows on a mirror: the new direction is glm::reflect(I, N) bit for bit, from the hit point."""
    rows = np.arange(len(z["I"]))
    p, x = _glm_paths(z, rows, [0], np.random.default_rng(3))
    x["materialId"] = MIRROR
    out = shade(1, 0, material_table(), p, x, None)
    assert (out["remainingBounces"] == 7).all()
    assert (bits(out["direction"]) == bits(z["reflect"])).all()
    assert (bits(out["origin"]) == bits(point_on_ray(po, p, x))).all()
    return len(rows)


def glm_refraction_rows(z):
    """The rows where the spec's binary32 dot(N, I) is negative, so that the face-forward normal is N itself: (rows, total
    internal reflection by glm's own account -- glm::refract takes the root of k < 0 and returns NaNs)."""
    s = z["N"] * z["I"]                                          # glm::dot: (x + y) + z
    rows = np.nonzero(((s[:, 0] + s[:, 1]) + s[:, 2]) < 0)[0]
    return rows, np.isnan(z["refract"][rows]).all(axis=1)


def check_glm_refraction(shade, po, z):
    """Each row under its own eta -- the fixture's (float)(1 / 1.5) as ior 1.5 seen from outside (1.0f / 1.5f is that float), 1.5,
    1.33 and 2.4 as ior = eta seen from inside -- with engines 0..15: a run that did not reflect went along glm::refract(I, N,
    eta) bit for bit, from P + I * 0.0002f; a row of total internal reflection reflects from P under every engine.  Returns
    (rows that refracted at least once, rows of total internal reflection)."""
    rows, tir = glm_refraction_rows(z)
    seeds = np.arange(16)
    p, x = _glm_paths(z, rows, seeds, np.random.default_rng(4))
    eta = z["eta"][rows]
    from_outside = eta == np.float32(1.0) / np.float32(1.5)
    assert (from_outside | np.isin(eta, np.array(IORS, dtype=np.float32))).all()
    mat = np.where(from_outside, GLASS0, GLASS0 + np.argmin(np.abs(eta[:, None] - np.array(IORS, dtype=np.float32)[None, :]), axis=1))
    x["materialId"] = np.repeat(mat, 16)
    outside = np.repeat(from_outside.astype(np.uint8), 16)
    out = shade(1, 0, material_table(), p, x, outside)
    assert (out["remainingBounces"] == 7).all()
    P = point_on_ray(po, p, x)
    want_refl = np.repeat(z["reflect"][rows], 16, axis=0)
    want_refr = np.repeat(z["refract"][rows], 16, axis=0)
    reflected = (bits(out["direction"]) == bits(want_refl)).all(axis=1)
    assert (bits(out["origin"][reflected]) == bits(P[reflected])).all()
    step = P + p["direction"] * np.float32(0.0002)               # binary32 throughout
    assert step.dtype == np.float32
    assert (bits(out["direction"][~reflected]) == bits(want_refr[~reflected])).all()
    assert (bits(out["origin"][~reflected]) == bits(step[~reflected])).all()
    per_row = reflected.reshape(len(rows), 16)
    assert per_row[tir].all()                                    # total internal reflection: every engine reflects
    return int((~per_row).any(axis=1).sum()), int(tir.sum())


# ---- physics (float64 on the outputs) ------------------------------------------------------------------------------------
def glass_records(I, n, material_id, pixel=None):
    p = np.zeros(len(I), dtype=PATH_DT)
    x = np.zeros(len(I), dtype=ISECT_DT)
    p["direction"], p["color"], p["remainingBounces"] = I, 1.0, 8
    p["pixelIndex"] = np.arange(len(I)) if pixel is None else pixel
    x["t"], x["normal"], x["materialId"] = 1.0, n, material_id
    return p, x


def snell(shade, count=20000):
    """For each ior x outside, `count` random unit (I, n) pairs at (iter 3, depth 2).  On the refracted outputs: the largest
    |sin(theta_t) - eta sin(theta_i)| (sines as the norms of the cross products with the face-forward normal), ||d| - 1| and
    |d . (I x n)| (the triple product: d lies in the plane of I and n); and how many of the rows whose float64
    k = 1 - eta^2 (1 - cos^2(theta_i)) is below -1e-5 refracted, of how many."""
    rng = np.random.default_rng(11)
    worst = np.zeros(3)
    forbidden = beyond = refracted = 0
    for k, ior in enumerate(IORS):
        for outside in (1, 0):
            I, n = unit_vectors(rng, count), unit_vectors(rng, count)
            p, x = glass_records(I, n, GLASS0 + k)
            out = shade(3, 2, material_table(), p, x, np.full(count, outside, dtype=np.uint8))
            eta = float(np.float32(1.0) / np.float32(ior)) if outside else float(np.float32(ior))
            nn = face_forward(I, n)
            I64, d = I.astype(np.float64), out["direction"].astype(np.float64)
            cos_i = -(I64 * nn).sum(1)
            crit = 1.0 - eta * eta * (1.0 - cos_i * cos_i)
            thr = (d * nn).sum(1) < 0
            beyond += int((crit < -1e-5).sum())
            forbidden += int((thr & (crit < -1e-5)).sum())
            refracted += int(thr.sum())
            sin_i = np.linalg.norm(np.cross(I64, nn), axis=1)
            sin_t = np.linalg.norm(np.cross(d, nn), axis=1)
            worst = np.maximum(worst, [np.abs(sin_t - eta * sin_i)[thr].max(), np.abs(np.linalg.norm(d, axis=1) - 1.0)[thr].max(),
                                       np.abs((d * np.cross(I64, nn)).sum(1))[thr].max()])
    return worst, forbidden, beyond, refracted


def schlick_normal_incidence(shade, count=65536):
    """I = (0, 0, -1) on n = (0, 0, 1) with engines 0 .. count - 1 at (iter 1, depth 0): for each ior x outside, (reflected share,
    ((1 - n) / (1 + n))^2, binomial standard deviation)."""
    I = np.tile(np.array([0, 0, -1], dtype=np.float32), (count, 1))
    n = np.tile(np.array([0, 0, 1], dtype=np.float32), (count, 1))
    res = []
    for k, ior in enumerate(IORS):
        for outside in (1, 0):
            p, x = glass_records(I, n, GLASS0 + k)
            out = shade(1, 0, material_table(), p, x, np.full(count, outside, dtype=np.uint8))
            up = out["direction"][:, 2] > 0
            assert (np.abs(out["direction"][:, 2]) > 0.3).all() and not out["direction"][:, :2].any()
            r0 = ((1.0 - ior) / (1.0 + ior)) ** 2
            res.append((ior, outside, float(up.mean()), r0, float(np.sqrt(r0 * (1.0 - r0) / count))))
    return res


def check_colours(shade, paths, isects, outside):
    """Mirror and glass multiply by specular.color, diffuse by color, the emitter by color * emittance: binary32 products,
    bit for bit (iter 3, depth 2)."""
    mats = material_table()
    out = shade(3, 2, mats, paths, isects, outside)
    b = branches(paths, isects, out)
    m = mats[isects["materialId"]]
    c = paths["color"]
    for name in ("mirror", "glass refracted", "glass reflected"):
        assert b[name].any() and (bits(out["color"][b[name]]) == bits((c * m["spec_color"])[b[name]])).all(), name
    assert b["diffuse"].any() and (bits(out["color"][b["diffuse"]]) == bits((c * m["color"])[b["diffuse"]])).all()
    e = b["emitter"]
    assert e.any() and (bits(out["color"][e]) == bits((c * (m["color"] * m["emittance"][:, None]))[e])).all()
    for name in ("miss", "last bounce"):
        assert b[name].any() and not out["color"][b[name]].any(), name


# ---- furnace -------------------------------------------------------------------------------------------------------------
SPHERE, CUBE = 0, 1
LIGHT = np.array([2.0, 1.0, 0.5], dtype=np.float32)             # colour (1, 0.5, 0.25) x emittance 2
FURNACE_ITERATIONS, FURNACE_DEPTH, FURNACE_SIZE = 32, 16, 48


def furnace_scene(pt, scenes, resized, shell, ball, ball_material):
    """A shell of an emitter (1, 0.5, 0.25) x 2 around the camera of cornell_glass_64 and a ball of `ball_material` in front
    of it: whatever a path does at the ball, it ends at the shell."""
    H = pt.host_binding.host_library()
    rows = [(shell, 0, (0, 5, 0), (0, 0, 0), (60, 60, 60)),
            (ball, 1, (0, 5, 0), (20, 35, 10) if ball == CUBE else (0, 0, 0), (6, 6, 6))]
    g = np.zeros(len(rows), dtype=pt.GEOM_DT)
    for k, (ty, mat, tr, rot, sc) in enumerate(rows):          # matrices by the host library's loader code
        g[k]["type"], g[k]["materialid"] = ty, mat
        g[k]["translation"], g[k]["rotation"], g[k]["scale"] = tr, rot, sc
        H.pth_build_geom_matrices(g.ctypes.data + k * pt.GEOM_DT.itemsize)
    mats = np.concatenate([material(color=(1.0, 0.5, 0.25), emittance=2.0), ball_material]).view(pt.MATERIAL_DT)
    return {"geoms": g, "materials": mats, "camera": resized(scenes["cornell_glass_64"]["camera"], FURNACE_SIZE, FURNACE_SIZE),
            "depth": FURNACE_DEPTH}
