"""Direct lighting that samples the environment map (PT_DIRECT_SKY; DESIGN.md section 6.24, include/ptmi355.h) in numpy: the
sampling tables (float64 on the float32 texels, running sums in index order, every stored value rounded once), the sky's branch
of the sampler and the final ray's rule (float32, one rounding per operation in the order written, none fused), and whole
iterations on top of direct_model.Model: the oracle's draws, environment_model.miss_colour and texel_index.  Without a map --
or with a map that yields no element -- every function here hands over to direct_model, so the model IS direct_model.Model."""
import numpy as np

import direct_model as dm
import environment_model as em
import glossy_model as gm

F32 = np.float32
F64 = np.float64
ONE = F32(1)
SKY = 2                                                             # the element's kind; its geom is -1
# the sky the tests share (input to the specification, not part of it): README's gradient with a sun of 14 degrees half angle
ZENITH, HORIZON, GROUND = (0.25, 0.45, 1.0), (0.9, 0.85, 0.8), (0.3, 0.25, 0.2)
SUN_DIR, SUN_COS, SUN_RGB = (1.0, 2.0, 1.5), 0.97, (60.0, 55.0, 45.0)


def gradient(pt, n):
    return pt.gradient_cubemap(n, ZENITH, HORIZON, GROUND)


def sun_sky(pt, n=16):
    return pt.sun_on_cubemap(gradient(pt, n), SUN_DIR, SUN_COS, SUN_RGB)


# ---- the tables ----------------------------------------------------------------------------------------------------------------
def _emit(mass):
    """(cdf, inv) float32 along the last axis of `mass` (float64): the running sum over its last value, the last entry forced
    to 1; inv = 1 / the difference of the ROUNDED entries.  np.cumsum accumulates in index order, as the host's loop does."""
    run = np.cumsum(mass, axis=-1)
    with np.errstate(all="ignore"):
        cdf = (run / run[..., -1:]).astype(F32)
        cdf[..., -1] = ONE
        wide = cdf.astype(F64)
        prev = np.concatenate([np.zeros_like(wide[..., :1]), wide[..., :-1]], axis=-1)
        inv = (1.0 / (wide - prev)).astype(F32)
    return cdf, inv


def tables(texels):
    """The sky element of a cube map ([6, n, n, 3] or flat), or None when it yields none: dict(n, rowcdf [6n], rowinv [6n],
    colcdf [6n, n], colinv [6n, n], K, s, m [6n, n] float64, T)."""
    if texels is None:
        return None
    t, n = em._flat(texels)
    t = t.astype(F64)
    with np.errstate(all="ignore"):
        lum = (0.2126 * t[:, 0] + 0.7152 * t[:, 1]) + 0.0722 * t[:, 2]
        lum = np.where(np.isfinite(lum) & (lum > 0), lum, 0.0)
    c = (2.0 * np.arange(n, dtype=F64) + 1.0) / float(n) - 1.0          # texel centres: ac from i, bc from j
    bc, ac = np.meshgrid(c, c, indexing="ij")
    q = (1.0 + ac * ac) + bc * bc
    J = 1.0 / (q * np.sqrt(q))
    m = (lum.reshape(6, n, n) * J[None]).reshape(6 * n, n)
    T = float(np.cumsum(m.reshape(-1))[-1])
    if not (np.isfinite(T) and T > 0):
        return None
    rowsum = np.cumsum(m, axis=1)[:, -1]
    rowcdf, rowinv = _emit(rowsum + T / (16.0 * 6 * n))
    mass = np.where((rowsum == 0)[:, None], 1.0, m + (rowsum / (16.0 * n))[:, None])
    colcdf, colinv = _emit(mass)
    return dict(n=n, rowcdf=rowcdf, rowinv=rowinv, colcdf=colcdf, colinv=colinv, K=F32(4.0 / ((np.pi * n) * n)), s=F32(2.0 / n), m=m, T=T)


def light_table(lamps, sky):
    """The device's table as a LIGHT_DT array: the lamps' elements alone (sky None), or at half their probability with the
    sky's element behind them."""
    if sky is None:
        return lamps
    out = np.zeros(len(lamps) + 1, dtype=dm.LIGHT_DT)
    out[:len(lamps)] = lamps
    out["cdf"][:len(lamps)] = lamps["cdf"] * F32(0.5)
    with np.errstate(all="ignore"):
        out["inv_p"][:len(lamps)] = lamps["inv_p"] * F32(2)
    out["geom"][-1], out["kind"][-1], out["cdf"][-1], out["inv_p"][-1] = -1, SKY, ONE, F32(2 if len(lamps) else 1)
    return out


# ---- the sampler ---------------------------------------------------------------------------------------------------------------
def sample_sky(po, sky, normals, u1, u2, states, inv_p):
    """The sky's branch for one record per row, the engines `states` having drawn u0, u1, u2: (dir, w, texel, info)."""
    n = sky["n"]
    nr = np.ascontiguousarray(normals, dtype=F32).reshape(-1, 3)
    u3, st = gm.u01(po, states)
    u4, st = gm.u01(po, st)
    r = np.minimum(np.searchsorted(sky["rowcdf"], u1, side="right"), 6 * n - 1).astype(np.int64)
    i = np.zeros(len(r), dtype=np.int64)
    for lo in range(0, len(r), 4096):                                   # the smallest i with u2 < colcdf[r, i]
        sl = slice(lo, lo + 4096)
        i[sl] = (sky["colcdf"][r[sl]] <= u2[sl, None]).sum(axis=1)
    i = np.minimum(i, n - 1)
    face, j = r // n, r % n
    axis = face >> 1
    s = sky["s"]
    with np.errstate(all="ignore"):
        a = ((i.astype(F32) + u3) * s - ONE).astype(F32)
        b = ((j.astype(F32) + u4) * s - ONE).astype(F32)
        sg = np.where(face & 1, F32(-1), ONE).astype(F32)
        v = np.where((axis == 0)[:, None], np.stack([sg, a, b], axis=1),
                     np.where((axis == 1)[:, None], np.stack([a, sg, b], axis=1), np.stack([a, b, sg], axis=1))).astype(F32)
        l2 = (ONE + a * a) + b * b
        rl = ONE / np.sqrt(l2)
        d = (v * rl[:, None]).astype(F32)
        Jd = (rl * rl) * rl
        cs = gm.dot3(nr, d)
        ok = cs > 0
        w = (((cs * Jd) * (sky["rowinv"][r] * sky["colinv"][r, i])) * (sky["K"] * F32(inv_p))).astype(F32)
    assert d.dtype == F32 and w.dtype == F32 and Jd.dtype == F32 and a.dtype == F32
    texel = (r * n + i).astype(np.int32)
    d = np.where(ok[:, None], d, F32(0)).astype(F32)
    w = np.where(ok, w, F32(0)).astype(F32)
    return d, w, texel, dict(ok=ok, cs=cs, u=(u1, u2, u3, u4), r=r, i=i, raw_dir=(v * rl[:, None]).astype(F32))


def probe_sky_sample(po, texels, normals, states, sky=None):
    """pt_probe_sky_sample: the sky as the only element.  (dir, w, texel, info); texel -1 where the map yields no element.
    sky: tables(texels) where the caller has them."""
    sky = tables(texels) if sky is None else sky
    count = len(states)
    if sky is None:
        return np.zeros((count, 3), F32), np.zeros(count, F32), np.full(count, -1, np.int32), None
    _, st = gm.u01(po, states)
    u1, st = gm.u01(po, st)
    u2, st = gm.u01(po, st)
    return sample_sky(po, sky, normals, u1, u2, st, 1)


def sample(po, geoms, table, sky, P, n, states):
    """direct_model.sample on the table with the sky's element: (dir, w, e, info); info["sky"] marks the lanes that picked it."""
    d, w, e, info = dm.sample(po, geoms, table, P, n, states)          # (the sky's lanes compute rubbish here, replaced below)
    k = np.nonzero(table["kind"][e] == SKY)[0]
    info["sky"] = table["kind"][e] == SKY
    if len(k):
        u0, u1, u2 = info["u"]
        st = states
        for _ in range(3):
            _, st = gm.u01(po, st)
        sd, sw, _, si = sample_sky(po, sky, np.ascontiguousarray(n, dtype=F32).reshape(-1, 3)[k], u1[k], u2[k], st[k], table["inv_p"][-1])
        d[k], w[k] = sd, sw
        info["ok"][k] = si["ok"]
        info["inside"][k] = False
    return d, w, e, info


# ---- the two bounces -----------------------------------------------------------------------------------------------------------
def sampling_bounce(po, it, depth, geoms, materials, table, sky, pre, isects, after, counts=None):
    """direct_model.sampling_bounce with the sampler above."""
    if sky is None:
        return dm.sampling_bounce(po, it, depth, geoms, materials, table, pre, isects, after, counts)
    out = after.copy()
    mats = materials[np.clip(isects["materialId"], 0, len(materials) - 1)]
    hit = (isects["t"] > 0) & ~(mats["emittance"] > 0) & (pre["remainingBounces"] > 0)
    spec = (mats["hasReflective"] > 0) | (mats["hasRefractive"] > 0)
    k = np.nonzero(hit & ~spec)[0]
    col = out["color"]
    col[hit] = 0
    org, dr = out["origin"], out["direction"]
    org[hit], dr[hit] = pre["origin"][hit], pre["direction"][hit]
    rem = out["remainingBounces"]
    rem[hit] = 0
    rem[~hit & (pre["remainingBounces"] > 0)] = 0
    if len(k):
        P = dm.point_on_ray(po, pre["origin"][k], pre["direction"][k], isects["t"][k])
        with np.errstate(all="ignore"):
            c = (pre["color"][k] * mats["color"][k]).astype(F32)
        d, w, e, info = sample(po, geoms, table, sky, P, isects["normal"][k], gm.seeded_states(po, it, pre["pixelIndex"][k], depth))
        ok = info["ok"]
        with np.errstate(all="ignore"):
            col[k[ok]] = (c[ok] * w[ok][:, None]).astype(F32)
        org[k[ok]], dr[k[ok]] = P[ok], d[ok]
        rem[k[ok]] = 1
        if counts is not None:
            sk = info["sky"]
            for name, v in (("sampled", len(k)), ("step 6", int((~ok & ~sk).sum())), ("sky aimed", int(sk.sum())),
                            ("lamp aimed", int((~sk).sum())), ("sky cs exits", int((~ok & sk).sum())),
                            ("negative or nan weights", int((~(w >= 0)).sum()))):
                counts[name] = counts.get(name, 0) + v
    out["color"], out["origin"], out["direction"], out["remainingBounces"] = col, org, dr, rem
    return out


def score(po, it, depth, materials, table, geoms, paths, t, hit_geom, texels, counts=None):
    """direct_model.score, and the sky's rule: a ray whose target is -1 ends with colour * E(direction) when t > 0 is false and
    with 0 on any hit."""
    out, wins = dm.score(po, it, depth, materials, table, geoms, paths, t, hit_geom)
    if texels is None or not len(table) or table["kind"][-1] != SKY:
        return out, wins
    live = paths["remainingBounces"] > 0
    target = dm.target_geoms(po, table, it, paths["pixelIndex"], depth - 1)
    aimed = live & (target == -1)
    miss = aimed & ~(t > 0)
    col = out["color"]
    col[aimed] = 0
    col[miss] = em.miss_colour(texels, paths["direction"][miss], paths["color"][miss])
    out["color"] = col
    wins = np.where(aimed, miss, wins)
    if counts is not None:
        lamp = live & ~aimed
        for name, v in (("sky scored", int(miss.sum())), ("sky occluded", int((aimed & ~miss).sum())), ("lamp missed", int((lamp & ~(t > 0)).sum()))):
            counts[name] = counts.get(name, 0) + v
    return out, wins


def shade_direct(po, it, depth, trace_depth, geoms, materials, paths, isects, texels, outside=None, hit_geom=None):
    """pt_probe_shade_scatter_direct_sky on caller records: the paths afterwards."""
    sky = tables(texels)
    if sky is None:
        return dm.shade_direct(po, it, depth, trace_depth, geoms, materials, paths, isects, outside, hit_geom)
    geoms = np.ascontiguousarray(geoms).view(po.GEOM_DT)
    mats = np.ascontiguousarray(materials).view(po.MATERIAL_DT)
    table = light_table(dm.light_elements(geoms, mats), sky)
    pre = np.array(paths, dtype=po.PATH_DT, copy=True)
    x = np.ascontiguousarray(isects).view(po.ISECT_DT)
    live = pre["remainingBounces"] > 0
    if depth == trace_depth:
        out, _ = score(po, it, depth, mats, table, geoms, pre, x["t"], np.asarray(hit_geom, dtype=np.int32), texels)
        return out
    high = pre.copy()
    high["remainingBounces"] = np.where(live, 3, pre["remainingBounces"])
    after = gm.shade_scatter(po, it, depth, mats, high, x, outside, glossy=False)
    if depth == trace_depth - 1:
        return sampling_bounce(po, it, depth, geoms, mats, table, sky, pre, x, after)
    ended = live & ~(after["remainingBounces"] > 0)
    after["remainingBounces"] = np.where(live, np.where(ended, 0, trace_depth - depth), pre["remainingBounces"])
    return after


# ---- whole iterations ------------------------------------------------------------------------------------------------------------
class Model(dm.Model):
    """The running sum of a PT_DIRECT_LIGHT | PT_DIRECT_SKY session.  set_environment rebuilds the light table: the sky's
    element comes and goes with the map, and with it -- in a scene without lamps -- the final bounce."""

    def __init__(self, po, geoms, materials, cam, depth, **kw):
        super().__init__(po, geoms, materials, cam, depth, **kw)
        self.lamps = self.table
        self.sky = None

    def set_environment(self, texels):
        super().set_environment(texels)
        self.sky = tables(self.texels)
        self.table = light_table(self.lamps, self.sky)
        self.direct = len(self.table) > 0

    def colours(self, it, snapshots=None):
        if self.sky is None:
            return super().colours(it, snapshots)
        po, D = self.po, self.depth
        if self.aa or self.lens[0] > 0:
            paths = po.generate_rays_ex(self.cam, D, it, aa=self.aa, lens=self.lens, trig=po.TRIG_SHARED)
        else:
            paths = po.generate_rays(self.cam, D)
        paths["remainingBounces"] += 1
        self.live = [0] * (D + 1)
        for d in range(D):
            idx = np.nonzero(paths["remainingBounces"] > 0)[0]
            if len(idx) == 0:
                break
            self.live[d] = len(idx)
            pre = np.ascontiguousarray(paths[idx])
            isects, outside = po.compute_intersections(pre, self.geoms, self.tris, self.meshes)
            missed = ~(isects["t"] > 0)
            sub = gm.shade_scatter(po, it, d, self.materials, pre, isects, outside, self.glossy, self.counts)
            if d == D - 1:
                sub = sampling_bounce(po, it, d, self.geoms, self.materials, self.table, self.sky, pre, isects, sub, self.counts)
            col = sub["color"]
            col[missed] = em.miss_colour(self.texels, pre["direction"][missed], pre["color"][missed])
            sub["color"] = col
            paths[idx] = sub
            if snapshots is not None:
                snapshots.append(paths[paths["remainingBounces"] > 0].copy())
        idx = np.nonzero(paths["remainingBounces"] > 0)[0]
        if len(idx):                                                     # bounce D: the final rays
            self.live[D] = len(idx)
            sub = np.ascontiguousarray(paths[idx])
            target = dm.target_geoms(po, self.table, it, sub["pixelIndex"], D - 1)
            t, wins = dm.winners(po, self.geoms, self.tris, self.meshes, sub, np.maximum(target, 0))
            sub, scored = score(po, it, D, self.materials, self.table, self.geoms, sub, t, np.where(wins & (target >= 0), target, -2),
                                self.texels, self.counts)
            paths[idx] = sub
            self.counts["final rays"] = self.counts.get("final rays", 0) + len(idx)
            self.counts["occluded"] = self.counts.get("occluded", 0) + int((~scored).sum())
            self.counts["final missed"] = self.counts.get("final missed", 0) + int((~(t > 0)).sum())
            if snapshots is not None:
                snapshots.append(paths[:0].copy())
        return paths["pixelIndex"].copy(), paths["color"].copy()
