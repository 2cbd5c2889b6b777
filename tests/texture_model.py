"""Texture mapping (PT_TEXTURES; DESIGN.md section 6.19, include/ptmi355.h) in numpy float32: the texel a hit point reads --
environment_model.texel_index applied to the oracle's multiplyMV of the hit primitive's inverseTransform -- the tinted
material colour mcol, and whole iterations composed from the oracle's own stages as glossy_model.Model composes them (so
that an environment map and PT_GLOSSY compose), shaded through pto_shade_scatter on a PER-PATH material table whose `color`
is mcol: the oracle itself is not changed.  The oracle reports no winning primitive: it is found by intersecting the
primitives alone, as direct_model.winners does.  Every operation is binary32 with one rounding, none is fused."""
import numpy as np

import direct_model as dm
import environment_model as em
import glossy_model as gm

F32 = np.float32
SPHERE, CUBE, MESH = 0, 1, 2


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def texel_index(geoms, hit_geom, points, n):
    """Steps 2-3: the texel each (primitive, world point) pair reads in a texture of n x n texels per face, [count] int32;
    -1 where the specification assigns none (a zero or NaN object-space point) and for mesh primitives."""
    h = np.asarray(hit_geom, dtype=np.int64).reshape(-1)
    p = np.ascontiguousarray(points, dtype=F32).reshape(-1, 3)
    if len(h) == 0:
        return np.zeros(0, dtype=np.int32)
    g = geoms[h]
    q = dm.multiply_mv(g["inverseTransform"], p, 1)
    k = em.texel_index(q, n)
    return np.where((g["type"] == SPHERE) | (g["type"] == CUBE), k, -1).astype(np.int32)


def tint(geoms, hit_geom, points, texels, colour):
    """Step 4 on records of one texture: colour * T[k] per component, colour where k < 0."""
    t, n = em._flat(texels)
    c = np.ascontiguousarray(colour, dtype=F32).reshape(-1, 3)
    k = texel_index(geoms, hit_geom, points, n)
    with np.errstate(all="ignore"):
        return np.where((k >= 0)[:, None], (c * t[np.maximum(k, 0)]).astype(F32), c).astype(F32)


def hit_geoms(po, geoms, tris, meshes, paths, isects):
    """The winning primitive of every path, [count] int32, -1 for a miss: the first primitive whose t alone equals the
    scene's t bit for bit (the reference loop: strict less, the lowest index on ties)."""
    paths = np.ascontiguousarray(paths)
    t_all = isects["t"]
    out = np.full(len(paths), -1, dtype=np.int32)
    todo = t_all > 0
    for g in range(len(geoms)):
        sel = np.nonzero(todo)[0]
        if len(sel) == 0:
            break
        one = np.ascontiguousarray(geoms[g:g + 1])
        m = None
        if int(one["type"][0]) == MESH:
            if meshes is None:
                continue
            m = np.ascontiguousarray(meshes[meshes["geom_index"] == g]).copy()
            if len(m) == 0:
                continue
            m["geom_index"] = 0
        own, _ = po.compute_intersections(np.ascontiguousarray(paths[sel]), one, tris if m is not None else None, m)
        same = (own["t"] > 0) & (bits(own["t"]) == bits(t_all[sel]))
        out[sel[same]] = g
        todo[sel[same]] = False
    assert not todo.any(), "a hit without a winning primitive"
    return out


def mcol(po, geoms, materials, textures, paths, isects, hit_geom):
    """The colour that stands for material.color at every record, [count, 3] float32 (the material's own for a record without
    a hit, a texture or a parametrisation).  textures: {material: [6, n, n, 3]}."""
    mats = materials[np.clip(isects["materialId"], 0, len(materials) - 1)]
    col = mats["color"].astype(F32).copy()
    hit = (isects["t"] > 0) & (np.asarray(hit_geom) >= 0)
    for m, tex in textures.items():
        sel = np.nonzero(hit & (isects["materialId"] == m))[0]
        if len(sel) == 0:
            continue
        P = dm.point_on_ray(po, paths["origin"][sel], paths["direction"][sel], isects["t"][sel])
        col[sel] = tint(geoms, np.asarray(hit_geom)[sel], P, tex, col[sel])
    return col


def shade_textured(po, it, depth, geoms, materials, textures, paths, isects, outside, hit_geom, glossy=False, counts=None):
    """One pass of the shader with mcol in place of material.color: pto_shade_scatter (through glossy_model.shade_scatter) on a
    per-path material table.  Returns the paths."""
    mats = np.ascontiguousarray(materials).view(po.MATERIAL_DT)
    x = np.ascontiguousarray(isects).view(po.ISECT_DT).copy()
    pre = np.array(paths, dtype=po.PATH_DT, copy=True)
    if len(pre) == 0:
        return pre
    table = mats[np.clip(x["materialId"], 0, len(mats) - 1)].copy()
    table["color"] = mcol(po, np.ascontiguousarray(geoms).view(po.GEOM_DT), mats, textures, pre, x, hit_geom)
    x["materialId"] = np.arange(len(x), dtype=np.int32)
    return gm.shade_scatter(po, it, depth, table, pre, x, outside, glossy, counts)


class Model(gm.Model):
    """The running sum of a PT_TEXTURES session: `iterate(it)` adds iteration `it` to `image`.  glossy and set_environment
    as in glossy_model.Model; set_texture(material, texels or None)."""

    def __init__(self, po, geoms, materials, cam, depth, tris=None, meshes=None, aa=False, lens=(0.0, 0.0), glossy=False):
        super().__init__(po, geoms, materials, cam, depth, tris=tris, meshes=meshes, aa=aa, lens=lens, glossy=glossy)
        self.textures = {}
        self.tinted = 0                                                  # hits that read a texel, since the model was made

    def set_texture(self, material, texels):
        if texels is None:
            self.textures.pop(int(material), None)
        else:
            self.textures[int(material)] = np.array(texels, dtype=F32, copy=True)

    def colours(self, it, snapshots=None):
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
            if self.textures:
                hg = hit_geoms(po, self.geoms, self.tris, self.meshes, sub, isects)
                kinds = self.geoms["type"][np.maximum(hg, 0)]
                self.tinted += int(((hg >= 0) & (kinds != MESH) & np.isin(isects["materialId"], list(self.textures))).sum())
                sub = shade_textured(po, it, d, self.geoms, self.materials, self.textures, sub, isects, outside, hg, self.glossy, self.counts)
            else:
                sub = gm.shade_scatter(po, it, d, self.materials, sub, isects, outside, self.glossy, self.counts)
            col = sub["color"]
            col[missed] = em.miss_colour(self.texels, direction, throughput)
            sub["color"] = col
            paths[idx] = sub
            if snapshots is not None:
                snapshots.append(paths[paths["remainingBounces"] > 0].copy())
        return paths["pixelIndex"].copy(), paths["color"].copy()


def checker(n, cells, colour0, colour1):
    """The scene format's CHECKER rule, texel by texel in Python integers (what binding.checker_cubemap and the loader are
    held against)."""
    out = np.zeros((6, n, n, 3), dtype=F32)
    col = (np.asarray(colour0, dtype=F32), np.asarray(colour1, dtype=F32))
    for face in range(6):
        for j in range(n):
            for i in range(n):
                out[face, j, i] = col[(i * cells // n + j * cells // n + face) & 1]
    return out
