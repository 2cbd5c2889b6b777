"""Smooth shading of triangle meshes (PT_SMOOTH_NORMALS; DESIGN.md section 6.26, include/ptmi355.h) in numpy float32: the shading
normal a mesh hit interpolates from its triangle's three vertex normals (steps 1-5 of the specification), and whole iterations
composed as bump_model.Model composes them: compute_intersections for the hits, texture_model.hit_geoms for the primitive,
po.mesh_winners for the triangle, the shading normal replaced per path, the oracle's pto_shade_scatter, then bump_model.guard.
The oracle itself is not changed.  Every operation is binary32 with one rounding, none is fused; cross and dot in glm's order."""
import numpy as np

import bump_model as bm
import environment_model as em
import glossy_model as gm
import texture_model as tm

F32 = np.float32
ONE = F32(1)
MESH = tm.MESH


def facet_normals(tris):
    """normalize(cross(e1, e2)) with e1 = fl(v1 - v0), e2 = fl(v2 - v0): the normal the intersection reports, [n, 3]."""
    v0 = np.ascontiguousarray(tris["v0"], dtype=F32).reshape(-1, 3)
    e1 = (np.ascontiguousarray(tris["v1"], dtype=F32).reshape(-1, 3) - v0).astype(F32)
    e2 = (np.ascontiguousarray(tris["v2"], dtype=F32).reshape(-1, 3) - v0).astype(F32)
    with np.errstate(all="ignore"):
        return gm.normalize3(gm.cross3(e1, e2).astype(F32)).astype(F32)


def smooth_normal(tris, normals, tri, origins, dirs, reported=None, stats=None):
    """Steps 1-5 on records (triangle tri[i], ray origins[i], dirs[i]): (normals [count, 3] float32, smoothed [count] bool); the
    reported normal (default: the facet normal) where the hit is not smoothed.  stats: a dict whose 'refused2', 'refused4' and
    'refused5' are counted up (the first step that refuses a record)."""
    k = np.asarray(tri, dtype=np.int64).reshape(-1)
    o = np.ascontiguousarray(origins, dtype=F32).reshape(-1, 3)
    I = np.ascontiguousarray(dirs, dtype=F32).reshape(-1, 3)
    vn = np.ascontiguousarray(normals, dtype=F32).reshape(-1, 3, 3)
    if len(k) == 0:
        return np.zeros((0, 3), dtype=F32), np.zeros(0, dtype=bool)
    t = tris[k]
    v0 = np.ascontiguousarray(t["v0"], dtype=F32).reshape(-1, 3)
    e1 = (np.ascontiguousarray(t["v1"], dtype=F32).reshape(-1, 3) - v0).astype(F32)
    e2 = (np.ascontiguousarray(t["v2"], dtype=F32).reshape(-1, 3) - v0).astype(F32)
    with np.errstate(all="ignore"):
        nr = gm.normalize3(gm.cross3(e1, e2).astype(F32)).astype(F32) if reported is None else \
            np.ascontiguousarray(reported, dtype=F32).reshape(-1, 3)
        p = gm.cross3(I, e2).astype(F32)                                        # 1
        a = gm.dot3(e1, p).astype(F32)
        f = (ONE / a).astype(F32)
        s = (o - v0).astype(F32)
        bx = (f * gm.dot3(s, p)).astype(F32)
        q = gm.cross3(s, e1).astype(F32)
        by = (f * gm.dot3(I, q)).astype(F32)
        bw = ((ONE - bx) - by).astype(F32)
        n0, n1, n2 = vn[k, 0], vn[k, 1], vn[k, 2]
        w = ((n0 * bw[:, None] + n1 * bx[:, None]) + n2 * by[:, None]).astype(F32)      # 2
        l2 = gm.dot3(w, w).astype(F32)
        ok2 = (l2 > 0) & np.isfinite(l2)
        ns = (w * (ONE / np.sqrt(l2))[:, None]).astype(F32)                     # 3
        ok4 = gm.dot3(ns, nr) > 0                                               # 4
        ok5 = gm.dot3(I, ns) < 0                                                # 5
    ok = ok2 & ok4 & ok5
    if stats is not None:
        stats["refused2"] = stats.get("refused2", 0) + int((~ok2).sum())
        stats["refused4"] = stats.get("refused4", 0) + int((ok2 & ~ok4).sum())
        stats["refused5"] = stats.get("refused5", 0) + int((ok2 & ok4 & ~ok5).sum())
    return np.where(ok[:, None], ns, nr).astype(F32), ok


def hit_triangles(po, geoms, tris, meshes, paths, hit_geom):
    """The winning triangle (its index in `tris`) of every path whose winner is a mesh primitive, -1 elsewhere."""
    out = np.full(len(paths), -1, dtype=np.int32)
    hg = np.asarray(hit_geom)
    if meshes is None:
        return out
    for m in meshes:
        geom, first, count = (int(v) for v in m.tolist())                # (geom index, first triangle, triangle count: either dtype's names)
        sel = np.nonzero(hg == geom)[0]
        if len(sel) == 0:
            continue
        idx, _ = po.mesh_winners(tris, np.ascontiguousarray(paths[sel]), first, count)
        assert (idx >= 0).all(), "a mesh hit without a winning triangle"
        out[sel] = idx
    return out


def shade_smooth(po, it, depth, geoms, materials, tris, meshes, normals, paths, isects, outside, glossy=False, counts=None, stats=None):
    """One pass of the shader with vertex normals, as the kernels run it: steps 1-5 on the mesh hits, shader about the smoothed
    normal, guard.  Returns the paths.  stats: a dict that receives 'smoothed', 'refused2/4/5', 'guarded' and, per material
    kind ('matte', 'mirror', 'glass'), 'smoothed <kind>' and 'guarded <kind>'."""
    mats = np.ascontiguousarray(materials).view(po.MATERIAL_DT)
    g = np.ascontiguousarray(geoms).view(po.GEOM_DT)
    x = np.ascontiguousarray(isects).view(po.ISECT_DT).copy()
    pre = np.array(paths, dtype=po.PATH_DT, copy=True)
    if len(pre) == 0:
        return pre
    reported = np.ascontiguousarray(x["normal"], dtype=F32).reshape(-1, 3).copy()
    nrm = reported.copy()
    flag = np.zeros(len(pre), dtype=bool)
    hg = tm.hit_geoms(po, g, tris, meshes, pre, x)
    # (the last bounce reads no normal and leaves no survivor: the kernels skip the lookup there, and nothing can tell)
    tri = hit_triangles(po, g, tris, meshes, pre, hg)
    sel = np.nonzero((tri >= 0) & (x["t"] > 0))[0]
    if len(sel):
        nrm[sel], flag[sel] = smooth_normal(tris, normals, tri[sel], pre["origin"][sel], pre["direction"][sel], reported[sel], stats)
    x["normal"] = nrm.reshape(x["normal"].shape)
    post = gm.shade_scatter(po, it, depth, mats, pre, x, outside, glossy, counts)
    before = np.ascontiguousarray(post["direction"], dtype=F32).reshape(-1, 3).copy()
    changed = bm.guard(po, mats, post, x, reported, flag)
    if stats is not None:
        m = mats[np.clip(x["materialId"], 0, len(mats) - 1)]
        kind = np.where(m["hasRefractive"] > 0, 2, np.where(m["hasReflective"] > 0, 1, 0))
        moved = (tm.bits(before) != tm.bits(np.ascontiguousarray(post["direction"], dtype=F32).reshape(-1, 3))).any(axis=1)
        live = pre["remainingBounces"] > 1                              # (not the last bounce, where the normal is not read)
        emit = m["emittance"] > 0
        stats["smoothed"] = stats.get("smoothed", 0) + int(flag.sum())
        stats["guarded"] = stats.get("guarded", 0) + changed
        for c, name in enumerate(("matte", "mirror", "glass")):
            stats["smoothed " + name] = stats.get("smoothed " + name, 0) + int((flag & live & ~emit & (kind == c)).sum())
            stats["guarded " + name] = stats.get("guarded " + name, 0) + int((moved & (kind == c)).sum())
    return post


class Model(gm.Model):
    """The running sum of a PT_SMOOTH_NORMALS session: glossy_model.Model (glossy and set_environment as there) plus
    set_vertex_normals(normals [num_triangles, 3, 3] or None).  Without normals every call is the parent's."""

    def __init__(self, po, geoms, materials, cam, depth, tris=None, meshes=None, aa=False, lens=(0.0, 0.0), glossy=False):
        super().__init__(po, geoms, materials, cam, depth, tris=tris, meshes=meshes, aa=aa, lens=lens, glossy=glossy)
        self.normals = None
        self.stats = {}

    def set_vertex_normals(self, normals):
        self.normals = None if normals is None else np.array(normals, dtype=F32, copy=True).reshape(-1, 3, 3)
        assert self.normals is None or len(self.normals) == len(self.tris)

    def colours(self, it, snapshots=None):
        if self.normals is None:
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
            sub = shade_smooth(po, it, d, self.geoms, self.materials, self.tris, self.meshes, self.normals, sub, isects, outside,
                               self.glossy, self.counts, self.stats)
            col = sub["color"]
            col[missed] = em.miss_colour(self.texels, direction, throughput)
            sub["color"] = col
            paths[idx] = sub
            if snapshots is not None:
                snapshots.append(paths[paths["remainingBounces"] > 0].copy())
        return paths["pixelIndex"].copy(), paths["color"].copy()
