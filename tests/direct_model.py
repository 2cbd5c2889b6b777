"""Direct lighting (PT_DIRECT_LIGHT; DESIGN.md section 6.18, include/ptmi355.h) in numpy: the light element table (float64 on
the float32 entries of the transform, every stored value rounded once), the sampler and the final ray's scoring rule (float32,
one rounding per operation in the order written, none fused), and whole iterations composed from the oracle's own stages as
glossy_model.Model composes them -- so that an environment map and PT_GLOSSY compose -- with the two bounces the flag changes
recomputed: at bounce D - 1 every hit on a surface that does not emit is replaced (a mirror or dielectric ends with colour 0,
a diffuse hit draws a point on a light), and bounce D scores a final ray only when the primitive it was aimed at wins.  The
oracle reports no winning primitive: it is found with compute_intersections on the whole scene, on the target alone and on
the primitives before it.  The draws, the engine, multiplyMV's order and the shared sin / cos are the oracle's."""
import numpy as np

import environment_model as em
import glossy_model as gm

F32 = np.float32
ONE = F32(1)
TWO_PI = gm.TWO_PI
PI32 = F32(np.pi)
SPHERE, CUBE = 0, 1
MAX_ELEMENTS = 1024
LIGHT_DT = np.dtype([("geom", "<i4"), ("kind", "<i4"), ("c0", "<f4", 3), ("ea", "<f4", 3), ("eb", "<f4", 3), ("normal", "<f4", 3),
                     ("area", "<f4"), ("cdf", "<f4"), ("inv_p", "<f4")])
assert LIGHT_DT.itemsize == 68


# ---- the light element table -------------------------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def det3(M):
    """Determinant of the upper 3 x 3 of a [4, 4] float32 matrix stored m[col][row], in float64: cofactors of the first row."""
    m = np.asarray(M, dtype=np.float64)
    a, b, c = m[0, 0], m[1, 0], m[2, 0]
    d, e, f = m[0, 1], m[1, 1], m[2, 1]
    g, h, i = m[0, 2], m[1, 2], m[2, 2]
    return (a * (e * i - f * h) - b * (d * i - f * g)) + c * (d * h - e * g)


def light_elements(geoms, materials):
    """The table pt_init builds, a LIGHT_DT array.  ValueError: a cube or sphere names a material outside the table."""
    rows = []
    with np.errstate(all="ignore"):
        for gi in range(len(geoms)):
            g = geoms[gi]
            kind = int(g["type"])
            if kind not in (SPHERE, CUBE):
                continue
            mid = int(g["materialid"])
            if mid < 0 or mid >= len(materials):
                raise ValueError("geom %d: material %d of %d" % (gi, mid, len(materials)))
            if not materials[mid]["emittance"] > 0:
                continue
            M = np.asarray(g["transform"], dtype=np.float64)             # M[col][row]
            if kind == SPHERE:
                e = np.zeros((), dtype=LIGHT_DT)
                e["geom"], e["kind"] = gi, SPHERE
                e["area"] = F32(np.pi * np.power(np.abs(det3(M)), 2.0 / 3.0))
                rows.append(e)
                continue
            for axis in range(3):
                for neg in range(2):
                    a = 1 if axis == 0 else 0                              # the other two axes in x, y, z order
                    b = 1 if axis == 2 else 2
                    corner = [0.0, 0.0, 0.0]
                    corner[axis], corner[a], corner[b] = (-0.5 if neg else 0.5), -0.5, -0.5
                    c0 = ((M[0, :3] * corner[0] + M[1, :3] * corner[1]) + M[2, :3] * corner[2]) + M[3, :3]
                    ea, eb = M[a, :3], M[b, :3]
                    out_dir = -M[axis, :3] if neg else M[axis, :3]
                    n = np.array([ea[1] * eb[2] - ea[2] * eb[1], ea[2] * eb[0] - ea[0] * eb[2], ea[0] * eb[1] - ea[1] * eb[0]])
                    area = np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
                    u = n / area
                    if (u[0] * out_dir[0] + u[1] * out_dir[1]) + u[2] * out_dir[2] < 0.0:
                        u = -u
                    e = np.zeros((), dtype=LIGHT_DT)
                    e["geom"], e["kind"] = gi, CUBE
                    e["c0"], e["ea"], e["eb"], e["normal"] = c0.astype(F32), ea.astype(F32), eb.astype(F32), u.astype(F32)
                    e["area"] = F32(area)
                    rows.append(e)
        rows = [e for e in rows if np.isfinite(e["area"]) and e["area"] > 0]
        out = np.zeros(len(rows), dtype=LIGHT_DT)
        for k, e in enumerate(rows):
            out[k] = e
        total = 0.0
        for e in out:
            total += float(e["area"])
        run = 0.0
        for k in range(len(out)):
            run += float(out["area"][k])
            out["cdf"][k] = F32(run / total)
            out["inv_p"][k] = F32(total / float(out["area"][k]))
        if len(out):
            out["cdf"][-1] = ONE
    return out


def placed(dtype, kind, material, trans, scale, rot=(0.0, 0.0, 0.0)):
    """One primitive under T * Rx Ry Rz * S (degrees) as a one-element array of the geom dtype `dtype`: the matrices in float64,
    rounded once -- input to the specification, not part of it.  A scale of 0 makes the transform singular: its inverse (and
    inverse transpose) has no finite entry then, and no ray ever hits the primitive."""
    g = np.zeros(1, dtype=dtype)
    rx, ry, rz = (np.radians(a) for a in rot)
    Rx = np.array([[1, 0, 0], [0, np.cos(rx), -np.sin(rx)], [0, np.sin(rx), np.cos(rx)]])
    Ry = np.array([[np.cos(ry), 0, np.sin(ry)], [0, 1, 0], [-np.sin(ry), 0, np.cos(ry)]])
    Rz = np.array([[np.cos(rz), -np.sin(rz), 0], [np.sin(rz), np.cos(rz), 0], [0, 0, 1]])
    M = np.eye(4)
    M[:3, :3] = Rx @ Ry @ Rz @ np.diag(np.asarray(scale, dtype=np.float64))
    M[:3, 3] = trans
    inv = np.linalg.inv(M) if all(s != 0 for s in scale) else np.full((4, 4), np.nan)
    g["type"], g["materialid"] = kind, material
    g["translation"], g["rotation"], g["scale"] = trans, rot, scale
    g["transform"][0] = M.T.astype(F32)                                  # stored m[col][row]
    g["inverseTransform"][0] = inv.T.astype(F32)
    g["invTranspose"][0] = inv.astype(F32)                               # (inv^T)^T
    return g


# ---- multiplyMV, the sampler ---------------------------------------------------------------------------------------------------
def multiply_mv(M, v, w):
    """The reference's multiplyMV as the oracle transcribes it (pto_multiply_mv), row by row: M [count, 4, 4] float32 stored
    m[col][row], v [count, 3], w the fourth component: (m0 * x + m1 * y) + (m2 * z + m3 * w)."""
    M = np.asarray(M, dtype=F32)
    v = np.asarray(v, dtype=F32)
    w = F32(w)
    with np.errstate(all="ignore"):
        out = [(M[:, 0, r] * v[:, 0] + M[:, 1, r] * v[:, 1]) + (M[:, 2, r] * v[:, 2] + M[:, 3, r] * w) for r in range(3)]
    return np.stack(out, axis=1).astype(F32)


def pick(table, u0):
    """The smallest e with u0 < cdf[e], E - 1 if none."""
    return np.minimum(np.searchsorted(table["cdf"], u0, side="right"), len(table) - 1).astype(np.int32)


def sample(po, geoms, table, P, n, states):
    """Steps 1 to 7 for one record per row: (dir, w, e, info).  dir and w are 0 where step 6 ends the path; info holds `ok`,
    the element's area measure `A`, `cl` after the inside flip, `inside`, the point `y` and the three draws."""
    P = np.ascontiguousarray(P, dtype=F32).reshape(-1, 3)
    n = np.ascontiguousarray(n, dtype=F32).reshape(-1, 3)
    u0, st = gm.u01(po, states)
    u1, st = gm.u01(po, st)
    u2, st = gm.u01(po, st)
    e = pick(table, u0)
    el = table[e]
    g = geoms[el["geom"]]
    sphere = el["kind"] == SPHERE
    with np.errstate(all="ignore"):
        # parallelogram
        y = ((el["c0"] + el["ea"] * u1[:, None]) + el["eb"] * u2[:, None]).astype(F32)
        nl = el["normal"].astype(F32).copy()
        A = el["area"].astype(F32).copy()
        # sphere
        k = np.nonzero(sphere)[0]
        if len(k):
            z = ONE - F32(2) * u1[k]
            r = np.sqrt(np.fmax(ONE - z * z, F32(0)))
            sa, ca = gm.sincos(po, u2[k] * TWO_PI)
            s = (np.stack([r * ca, r * sa, z], axis=1) * F32(0.5)).astype(F32)
            y[k] = multiply_mv(g["transform"][k], s, 1)
            q = multiply_mv(g["invTranspose"][k], s, 0)
            ln = np.sqrt(gm.dot3(q, q))
            nl[k] = q * (ONE / ln)[:, None]
            detpi = np.array([F32(np.pi * np.abs(det3(m))) for m in g["transform"][k]], dtype=F32)
            A[k] = detpi * (ln * F32(2))
        v = (y - P).astype(F32)
        d2 = gm.dot3(v, v)
        d = (v * (ONE / np.sqrt(d2))[:, None]).astype(F32)
        cs = gm.dot3(n, d)
        cl = -gm.dot3(nl, d)
        o = multiply_mv(g["inverseTransform"], P, 1)
        inside = np.where(sphere, gm.dot3(o, o) < F32(0.25), (np.abs(o) < F32(0.5)).all(axis=1))
        cl = np.where(inside, -cl, cl).astype(F32)
        ok = (d2 > 0) & (cs > 0) & (cl > 0)
        w = (((cs * cl) * (A * el["inv_p"])) / (d2 * PI32)).astype(F32)
    assert y.dtype == F32 and d.dtype == F32 and w.dtype == F32 and A.dtype == F32
    d = np.where(ok[:, None], d, F32(0)).astype(F32)
    w = np.where(ok, w, F32(0)).astype(F32)
    return d, w, e, dict(ok=ok, A=A, cl=cl, inside=inside, y=y, u=(u0, u1, u2), cs=cs, d2=d2)


def point_on_ray(po, origin, direction, t):
    L = po.lib()
    out = np.zeros((len(t), 3), dtype=F32)
    for k in range(len(t)):
        p = L.pto_get_point_on_ray(po.ray(origin[k], direction[k]), float(t[k]))
        out[k] = (p.x, p.y, p.z)
    return out


def target_geoms(po, table, it, pixels, depth):
    """The primitive each final ray was aimed at: the first draw of the engine of the bounce that aimed it."""
    u0, _ = gm.u01(po, gm.seeded_states(po, it, pixels, depth))
    return table["geom"][pick(table, u0)].astype(np.int32)


# ---- the two bounces the flag changes ------------------------------------------------------------------------------------------
def sampling_bounce(po, it, depth, geoms, materials, table, pre, isects, after, counts=None):
    """Bounce D - 1: `after` = the oracle's shade of `pre` (made with remainingBounces high enough that it zeroes nothing);
    every hit on a surface that does not emit is replaced.  A path that ends keeps the ray it came with.  Survivors leave
    with remainingBounces = 1."""
    out = after.copy()
    mats = materials[np.clip(isects["materialId"], 0, len(materials) - 1)]
    hit = (isects["t"] > 0) & ~(mats["emittance"] > 0) & (pre["remainingBounces"] > 0)
    spec = (mats["hasReflective"] > 0) | (mats["hasRefractive"] > 0)
    ended = hit.copy()
    k = np.nonzero(hit & ~spec)[0]
    col = out["color"]
    col[hit] = 0
    org, dr = out["origin"], out["direction"]
    org[hit], dr[hit] = pre["origin"][hit], pre["direction"][hit]
    rem = out["remainingBounces"]
    rem[hit] = 0
    rem[~hit & (pre["remainingBounces"] > 0)] = 0                       # emitters and misses ended in the oracle's pass
    if len(k) and len(table):
        P = point_on_ray(po, pre["origin"][k], pre["direction"][k], isects["t"][k])
        with np.errstate(all="ignore"):
            c = (pre["color"][k] * mats["color"][k]).astype(F32)
        d, w, e, info = sample(po, geoms, table, P, isects["normal"][k], gm.seeded_states(po, it, pre["pixelIndex"][k], depth))
        ok = info["ok"]
        with np.errstate(all="ignore"):
            col[k[ok]] = (c[ok] * w[ok][:, None]).astype(F32)
        org[k[ok]], dr[k[ok]] = P[ok], d[ok]
        rem[k[ok]] = 1
        ended[k[ok]] = False
        if counts is not None:
            counts["sampled"] = counts.get("sampled", 0) + len(k)
            counts["step 6"] = counts.get("step 6", 0) + int((~ok).sum())
            counts["inside"] = counts.get("inside", 0) + int(info["inside"].sum())
            kinds = table["kind"][e]
            counts["sphere"] = counts.get("sphere", 0) + int((kinds == SPHERE).sum())
            counts["cube"] = counts.get("cube", 0) + int((kinds == CUBE).sum())
    out["color"], out["origin"], out["direction"], out["remainingBounces"] = col, org, dr, rem
    return out


def score(po, it, depth, materials, table, geoms, paths, t, hit_geom):
    """Bounce D on records whose winner is known (t, hit_geom): colour *= material.color * emittance of the target when it
    won, 0 otherwise; every path ends."""
    out = paths.copy()
    live = paths["remainingBounces"] > 0
    target = target_geoms(po, table, it, paths["pixelIndex"], depth - 1) if len(table) else np.full(len(paths), -2, np.int32)
    wins = live & (t > 0) & (hit_geom == target)
    m = materials[geoms["materialid"][np.maximum(target, 0)]]
    with np.errstate(all="ignore"):
        e = (m["color"] * m["emittance"][:, None]).astype(F32)
        col = np.where(wins[:, None], (paths["color"] * e).astype(F32), F32(0)).astype(F32)
    c = out["color"]
    c[live] = col[live]
    out["color"] = c
    out["remainingBounces"] = np.where(live, 0, paths["remainingBounces"])
    return out, wins


def winners(po, geoms, tris, meshes, paths, target):
    """(t of the scene's nearest hit, whether the primitive `target[i]` is path i's winner): its t > 0 equals the scene's t bit
    for bit and no primitive before it has that t (the reference loop: strict less, the lowest index on ties)."""
    paths = np.ascontiguousarray(paths)
    isects, _ = po.compute_intersections(paths, geoms, tris, meshes)
    t_all = isects["t"]
    wins = np.zeros(len(paths), dtype=bool)
    for g in np.unique(target):
        sel = np.nonzero(target == g)[0]
        sub = np.ascontiguousarray(paths[sel])
        own, _ = po.compute_intersections(sub, np.ascontiguousarray(geoms[g:g + 1]))
        same = (t_all[sel] > 0) & (bits(own["t"]) == bits(t_all[sel]))
        if g > 0:
            before_meshes = None
            if meshes is not None:
                keep = meshes[meshes["geom_index"] < g]
                before_meshes = np.ascontiguousarray(keep) if len(keep) else None
            before, _ = po.compute_intersections(sub, np.ascontiguousarray(geoms[:g]), tris, before_meshes)
            same &= ~((before["t"] > 0) & (bits(before["t"]) == bits(t_all[sel])))
        wins[sel] = same
    return t_all, wins


def shade_direct(po, it, depth, trace_depth, geoms, materials, paths, isects, outside=None, hit_geom=None):
    """pt_probe_shade_scatter_direct on caller records: the paths afterwards."""
    geoms = np.ascontiguousarray(geoms).view(po.GEOM_DT)
    mats = np.ascontiguousarray(materials).view(po.MATERIAL_DT)
    table = light_elements(geoms, mats)
    pre = np.array(paths, dtype=po.PATH_DT, copy=True)
    x = np.ascontiguousarray(isects).view(po.ISECT_DT)
    live = pre["remainingBounces"] > 0
    if depth == trace_depth:
        out, _ = score(po, it, depth, mats, table, geoms, pre, x["t"], np.asarray(hit_geom, dtype=np.int32))
        return out
    high = pre.copy()
    high["remainingBounces"] = np.where(live, 3, pre["remainingBounces"])
    after = gm.shade_scatter(po, it, depth, mats, high, x, outside, glossy=False)
    if depth == trace_depth - 1:
        return sampling_bounce(po, it, depth, geoms, mats, table, pre, x, after)
    ended = live & ~(after["remainingBounces"] > 0)
    after["remainingBounces"] = np.where(live, np.where(ended, 0, trace_depth - depth), pre["remainingBounces"])
    return after


# ---- whole iterations ------------------------------------------------------------------------------------------------------------
class Model(gm.Model):
    """The running sum of a PT_DIRECT_LIGHT session (direct=False: of one without the flag): `iterate(it)` adds iteration `it`
    to `image`.  glossy and set_environment as in glossy_model.Model.  `live` = the paths traced at each bounce of the last
    iteration (D + 1 entries with the flag), `counts` the routes taken since the model was made."""

    def __init__(self, po, geoms, materials, cam, depth, tris=None, meshes=None, aa=False, lens=(0.0, 0.0), glossy=False, direct=True):
        super().__init__(po, geoms, materials, cam, depth, tris=tris, meshes=meshes, aa=aa, lens=lens, glossy=glossy)
        self.table = light_elements(self.geoms, self.materials) if direct else np.zeros(0, dtype=LIGHT_DT)
        if len(self.table) > MAX_ELEMENTS:
            raise ValueError("%d light elements" % len(self.table))
        self.direct = len(self.table) > 0
        self.live = []

    def colours(self, it, snapshots=None):
        if not self.direct:
            return super().colours(it, snapshots)
        po, D = self.po, self.depth
        if self.aa or self.lens[0] > 0:
            paths = po.generate_rays_ex(self.cam, D, it, aa=self.aa, lens=self.lens, trig=po.TRIG_SHARED)
        else:
            paths = po.generate_rays(self.cam, D)
        paths["remainingBounces"] += 1                                  # D + 1 bounces; the camera's engine slot stays D
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
                sub = sampling_bounce(po, it, d, self.geoms, self.materials, self.table, pre, isects, sub, self.counts)
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
            target = target_geoms(po, self.table, it, sub["pixelIndex"], D - 1)
            t, wins = winners(po, self.geoms, self.tris, self.meshes, sub, target)
            sub, scored = score(po, it, D, self.materials, self.table, self.geoms, sub, t, np.where(wins, target, -1))
            paths[idx] = sub
            self.counts["final rays"] = self.counts.get("final rays", 0) + len(idx)
            self.counts["occluded"] = self.counts.get("occluded", 0) + int((~scored).sum())
            self.counts["final missed"] = self.counts.get("final missed", 0) + int((~(t > 0)).sum())
            if snapshots is not None:
                snapshots.append(paths[:0].copy())
        return paths["pixelIndex"].copy(), paths["color"].copy()
