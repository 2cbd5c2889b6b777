"""Bump mapping (PT_TEXTURES; DESIGN.md section 6.22, include/ptmi355.h) in numpy float32: the shading normal a hit reads from its
material's cube bump map (steps 1-8 of the specification), and whole iterations composed as texture_model.Model composes them:
the oracle's pto_shade_scatter reads the normal from the intersection record the caller hands it, so the model replaces
`normal` per path for the perturbed hits, as texture_model replaces `color`; the oracle itself is not changed.  After
the shader the guard reflects a surviving mirror or diffuse direction that does not leave the reported surface.  Every
operation is binary32 with one rounding, none is fused."""
import numpy as np

import direct_model as dm
import environment_model as em
import glossy_model as gm
import texture_model as tm

F32 = np.float32
SPHERE, CUBE, MESH = tm.SPHERE, tm.CUBE, tm.MESH


def _face(q):
    """env_texel's own major axis (ties go to the earlier axis) and the sign of the major component."""
    x, y, z = q[:, 0], q[:, 1], q[:, 2]
    ax, ay, az = np.abs(x), np.abs(y), np.abs(z)
    with np.errstate(all="ignore"):
        axis0 = (ax >= ay) & (ax >= az)
        axis1 = ~axis0 & (ay >= az)
        axis = np.where(axis0, 0, np.where(axis1, 1, 2))
        major = np.where(axis0, x, np.where(axis1, y, z))
        return axis, major < 0


def bump_normal(geoms, hit_geom, points, normals, dirs, texels):
    """Steps 1-8 on records of one map: (normals [count, 3] float32, perturbed [count] bool); the reported normal where the hit
    is not perturbed, and for mesh primitives."""
    t, n = em._flat(texels)
    h = np.asarray(hit_geom, dtype=np.int64).reshape(-1)
    P = np.ascontiguousarray(points, dtype=F32).reshape(-1, 3)
    nr = np.ascontiguousarray(normals, dtype=F32).reshape(-1, 3)
    I = np.ascontiguousarray(dirs, dtype=F32).reshape(-1, 3)
    if len(h) == 0:
        return nr.copy(), np.zeros(0, dtype=bool)
    g = geoms[h]
    cube = g["type"] == CUBE
    with np.errstate(all="ignore"):
        ok = (cube | (g["type"] == SPHERE)) & (gm.dot3(I, nr) < 0)              # 1
        q = dm.multiply_mv(g["inverseTransform"], P, 1)                         # 2
        k = em.texel_index(q, n)                                                # 3
        axis, negative = _face(q)
        ok &= k >= 0
        e = t[np.maximum(k, 0)]                                                 # 4
        da, db = e[:, 0], e[:, 1]
        ok &= ~((da == 0) & (db == 0))
        major = np.where(negative, F32(-1), F32(1)).astype(F32)                 # 5
        uc = np.stack([np.where(axis == 0, major, da),
                       np.where(axis == 0, da, np.where(axis == 1, major, db)),
                       np.where(axis == 2, major, db)], axis=1).astype(F32)
        q2 = (q + q).astype(F32)
        us = np.stack([np.where(axis != 0, q2[:, 0] + da, q2[:, 0]),
                       np.where(axis == 0, q2[:, 1] + da, np.where(axis == 2, q2[:, 1] + db, q2[:, 1])),
                       np.where(axis != 2, q2[:, 2] + db, q2[:, 2])], axis=1).astype(F32)
        u = np.where(cube[:, None], uc, us).astype(F32)
        M = np.where(cube[:, None, None], g["transform"], g["invTranspose"]).astype(F32)
        w = dm.multiply_mv(M, u, 0)                                             # 6
        ns = gm.normalize3(w).astype(F32)
        s = gm.dot3(ns, nr)                                                     # 7
        ns = np.where((s < 0)[:, None], -ns, ns).astype(F32)
        ok &= gm.dot3(ns, nr) > 0
        ok &= gm.dot3(I, ns) < 0                                                # 8
    return np.where(ok[:, None], ns, nr).astype(F32), ok


def shading_normals(po, geoms, bump_maps, paths, isects, hit_geom):
    """The normal every record is shaded with, [count, 3] float32, and which records are perturbed.  bump_maps: {material:
    [6, n, n, 3]}."""
    nrm = np.ascontiguousarray(isects["normal"], dtype=F32).reshape(-1, 3).copy()
    flag = np.zeros(len(nrm), dtype=bool)
    hg = np.asarray(hit_geom)
    hit = (isects["t"] > 0) & (hg >= 0)
    for m, bm in bump_maps.items():
        sel = np.nonzero(hit & (isects["materialId"] == m))[0]
        if len(sel) == 0:
            continue
        P = dm.point_on_ray(po, paths["origin"][sel], paths["direction"][sel], isects["t"][sel])
        nrm[sel], flag[sel] = bump_normal(geoms, hg[sel], P, nrm[sel], paths["direction"][sel], bm)
    return nrm, flag


def guard(po, materials, post, isects, reported, perturbed):
    """The guard on the shaded paths `post`: a surviving perturbed path on a mirror, or on a surface that is neither mirror nor
    dielectric, whose new direction has dot(dir, nr) > 0 false takes reflect(dir, nr), not renormalised.  In place; returns
    how many directions it changed."""
    mats = materials[np.clip(isects["materialId"], 0, len(materials) - 1)]
    mirror = mats["hasReflective"] > 0
    glass = mats["hasRefractive"] > 0
    d = np.ascontiguousarray(post["direction"], dtype=F32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        sel = np.nonzero(perturbed & (post["remainingBounces"] > 0) & (mirror | ~glass) & ~(gm.dot3(d, reported) > 0))[0]
    if len(sel):
        d = d.copy()
        d[sel] = gm.reflect3(po, d[sel], reported[sel])
        post["direction"] = d
    return len(sel)


def shade_bumped(po, it, depth, geoms, materials, textures, bump_maps, paths, isects, outside, hit_geom, glossy=False, counts=None,
                 use_guard=True, stats=None):
    """One pass of the textured shader with bump maps, as the kernels run it: lookup, shader about the perturbed normal, guard.
    Returns the paths.  stats: a dict whose 'bumped' and 'guarded' are counted up."""
    mats = np.ascontiguousarray(materials).view(po.MATERIAL_DT)
    g = np.ascontiguousarray(geoms).view(po.GEOM_DT)
    x = np.ascontiguousarray(isects).view(po.ISECT_DT).copy()
    pre = np.array(paths, dtype=po.PATH_DT, copy=True)
    if len(pre) == 0:
        return pre
    reported = np.ascontiguousarray(x["normal"], dtype=F32).reshape(-1, 3).copy()
    nrm, flag = shading_normals(po, g, bump_maps, pre, x, hit_geom)
    x["normal"] = nrm.reshape(x["normal"].shape)
    post = tm.shade_textured(po, it, depth, g, mats, textures, pre, x, outside, hit_geom, glossy, counts)
    changed = guard(po, mats, post, x, reported, flag) if use_guard else 0
    if stats is not None:
        stats["bumped"] = stats.get("bumped", 0) + int(flag.sum())
        stats["guarded"] = stats.get("guarded", 0) + changed
    return post


class Model(tm.Model):
    """The running sum of a PT_TEXTURES session with bump maps: texture_model.Model plus set_bump_map(material, texels or
    None).  use_guard=False (tests only) leaves the guard out."""

    def __init__(self, po, geoms, materials, cam, depth, tris=None, meshes=None, aa=False, lens=(0.0, 0.0), glossy=False, use_guard=True):
        super().__init__(po, geoms, materials, cam, depth, tris=tris, meshes=meshes, aa=aa, lens=lens, glossy=glossy)
        self.bump_maps = {}
        self.use_guard = use_guard
        self.bumped = 0                                                  # hits shaded about a perturbed normal
        self.guarded = 0                                                 # directions the guard changed

    def set_bump_map(self, material, texels):
        if texels is None:
            self.bump_maps.pop(int(material), None)
        else:
            self.bump_maps[int(material)] = np.array(texels, dtype=F32, copy=True)

    def colours(self, it, snapshots=None):
        if not self.bump_maps:
            return super().colours(it, snapshots)
        po = self.po
        if self.aa or self.lens[0] > 0:
            paths = po.generate_rays_ex(self.cam, self.depth, it, aa=self.aa, lens=self.lens, trig=po.TRIG_SHARED)
        else:
            paths = po.generate_rays(self.cam, self.depth)
        for d in range(self.depth):
            idx = np.nonzero(paths["remainingBounces"] > 0)[0]
            if len(idx) == 0:
                break
            sub = np.ascontiguousarray(paths[idx])
            isects, outside = po.compute_intersections(sub, self.geoms, self.tris, self.meshes)
            missed = ~(isects["t"] > 0)
            throughput = sub["color"][missed].copy()
            direction = sub["direction"][missed].copy()
            hg = tm.hit_geoms(po, self.geoms, self.tris, self.meshes, sub, isects)
            kinds = self.geoms["type"][np.maximum(hg, 0)]
            self.tinted += int(((hg >= 0) & (kinds != MESH) & np.isin(isects["materialId"], list(self.textures))).sum())
            stats = {}
            sub = shade_bumped(po, it, d, self.geoms, self.materials, self.textures, self.bump_maps, sub, isects, outside, hg,
                               self.glossy, self.counts, self.use_guard, stats)
            self.bumped += stats.get("bumped", 0)
            self.guarded += stats.get("guarded", 0)
            col = sub["color"]
            col[missed] = em.miss_colour(self.texels, direction, throughput)
            sub["color"] = col
            paths[idx] = sub
            if snapshots is not None:
                snapshots.append(paths[paths["remainingBounces"] > 0].copy())
        return paths["pixelIndex"].copy(), paths["color"].copy()


def studs(n, cells, slope):
    """The scene format's STUDS rule, texel by texel in Python integers (what binding.studs_bumpmap and the loader are held
    against): every stored value is 0 or +-slope exactly."""
    out = np.zeros((6, n, n, 3), dtype=F32)

    def side(v):
        p = (v * cells * 4 // n) % 4
        return -1 if p == 0 else 1 if p == 3 else 0

    for face in range(6):
        for j in range(n):
            for i in range(n):
                out[face, j, i, 0] = F32(slope) * F32(side(i))
                out[face, j, i, 1] = F32(slope) * F32(side(j))
    return out
