"""Environment lighting (include/ptmi355.h: pt_set_environment) in numpy float32: the lookup E(d),
and whole iterations composed from the oracle's own stages -- generate_rays, compute_intersections, pto_shade_scatter --
with the one change the specification makes: a path whose intersection has t <= 0 ends with colour = throughput * E(d),
d the direction of the ray that missed.  With no environment the loop is the oracle's iteration, bit for bit
(tests/test_environment_model_cpu.py).  Every operation is binary32 with one rounding, none is fused."""
import ctypes as C

import numpy as np

F32 = np.float32


def texel_index(dirs, n):
    """The texel each direction reads in a map of n x n texels per face, [count] int32; -1 where the specification assigns
    none (a zero direction, or NaN on its major axis)."""
    d = np.ascontiguousarray(dirs, dtype=F32).reshape(-1, 3)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    ax, ay, az = np.abs(x), np.abs(y), np.abs(z)
    with np.errstate(all="ignore"):
        axis0 = (ax >= ay) & (ax >= az)
        axis1 = ~axis0 & (ay >= az)
        axis = np.where(axis0, 0, np.where(axis1, 1, 2))
        m = np.where(axis0, ax, np.where(axis1, ay, az)).astype(F32)
        major = np.where(axis0, x, np.where(axis1, y, z))
        a = np.where(axis0, y, x).astype(F32)                      # the other two components in x, y, z order
        b = np.where(axis == 2, y, z).astype(F32)
        ok = m > 0                                                  # False for 0 and for NaN
        face = 2 * axis + (major < 0)
        ms = np.where(ok, m, F32(1))
        u, v = (a / ms).astype(F32), (b / ms).astype(F32)           # correctly rounded divides
        fi = ((u * F32(0.5) + F32(0.5)).astype(F32) * F32(n)).astype(F32)
        fj = ((v * F32(0.5) + F32(0.5)).astype(F32) * F32(n)).astype(F32)
        # u, v lie in [-1, 1]: both products are >= 0.  (NaN only for a direction with two infinite or a NaN minor
        # component: coordinate 0, never an index outside the map.)
        i = np.minimum(np.fmax(fi, F32(0)).astype(np.int32), n - 1)
        j = np.minimum(np.fmax(fj, F32(0)).astype(np.int32), n - 1)
    return np.where(ok, (face * n + j) * n + i, -1).astype(np.int32)


def _flat(texels):
    t = np.ascontiguousarray(texels, dtype=F32)
    n = int(round((t.size / 18.0) ** 0.5))
    assert t.size == 18 * n * n and n >= 1, t.shape
    return t.reshape(6 * n * n, 3), n


def radiance(texels, dirs):
    """E(d), [count, 3] float32: the nearest texel, (0, 0, 0) for a direction without one."""
    t, n = _flat(texels)
    k = texel_index(dirs, n)
    return np.where((k >= 0)[:, None], t[np.maximum(k, 0)], F32(0)).astype(F32)


def miss_colour(texels, dirs, throughput):
    """throughput * E(d) per component; +0 with no environment (texels None)."""
    c = np.ascontiguousarray(throughput, dtype=F32).reshape(-1, 3)
    if texels is None:
        return np.zeros_like(c)
    with np.errstate(all="ignore"):
        return (c * radiance(texels, dirs)).astype(F32)


class Model:
    """The running sum of a session with an environment: `iterate(it)` adds iteration `it` to `image`."""

    def __init__(self, po, geoms, materials, cam, depth, tris=None, meshes=None, aa=False, lens=(0.0, 0.0)):
        self.po = po
        self.geoms = np.ascontiguousarray(geoms).view(po.GEOM_DT)
        self.materials = np.ascontiguousarray(materials)
        self.cam, self.depth = cam, int(depth)
        self.tris = None if tris is None else np.ascontiguousarray(tris).view(po.TRI_DT)
        self.meshes = None if meshes is None else np.ascontiguousarray(meshes).view(po.MESH_DT)
        self.aa, self.lens = aa, lens
        w, h = (int(v) for v in np.asarray(cam["resolution"]).reshape(2))
        self.n = w * h
        self.image = np.zeros((self.n, 3), dtype=F32)
        self.texels = None
        self.misses = self.paths_ended = 0

    def set_environment(self, texels):
        self.texels = None if texels is None else np.array(texels, dtype=F32, copy=True)

    def colours(self, it):
        """(pixelIndex, final colour) of every path of iteration `it`."""
        po = self.po
        if self.aa or self.lens[0] > 0:
            paths = po.generate_rays_ex(self.cam, self.depth, it, aa=self.aa, lens=self.lens, trig=po.TRIG_SHARED)
        else:
            paths = po.generate_rays(self.cam, self.depth)
        n = len(paths)
        L = po.lib()
        for d in range(self.depth):
            # the live paths, packed (every stage is per path, keyed by pixelIndex: the order does not matter)
            idx = np.nonzero(paths["remainingBounces"] > 0)[0]
            if len(idx) == 0:
                break
            sub = np.ascontiguousarray(paths[idx])
            isects, outside = po.compute_intersections(sub, self.geoms, self.tris, self.meshes)
            missed = ~(isects["t"] > 0)
            throughput = sub["color"][missed].copy()
            direction = sub["direction"][missed].copy()
            L.pto_shade_scatter(it, d, len(sub), isects.ctypes.data_as(C.c_void_p), outside.ctypes.data_as(C.c_void_p),
                                sub.ctypes.data_as(C.c_void_p), self.materials.ctypes.data_as(C.c_void_p), po.TRIG_SHARED)
            col = sub["color"]
            col[missed] = miss_colour(self.texels, direction, throughput)
            sub["color"] = col
            paths[idx] = sub
            self.misses += int(missed.sum())
        self.paths_ended += n
        return paths["pixelIndex"].copy(), paths["color"].copy()

    def iterate(self, it):
        pix, col = self.colours(it)
        self.image[pix] = (self.image[pix] + col).astype(F32)      # one path per pixel: one addition per pixel and iteration
        return self.image


# ---- directions the tests share ----------------------------------------------------------------------------------------
INF, NAN = np.float32(np.inf), np.float32(np.nan)


def edge_directions():
    """(directions, texel index at n = 4) the specification pins by hand: ties, the six axes, u = +-1 exactly, no direction."""
    cases = [
        # the six axis directions: the centre of each face rounds up to texel (2, 2)
        ((1, 0, 0), (0 * 4 + 2) * 4 + 2), ((-1, 0, 0), (1 * 4 + 2) * 4 + 2),
        ((0, 1, 0), (2 * 4 + 2) * 4 + 2), ((0, -1, 0), (3 * 4 + 2) * 4 + 2),
        ((0, 0, 1), (4 * 4 + 2) * 4 + 2), ((0, 0, -1), (5 * 4 + 2) * 4 + 2),
        # ties go to the earlier axis: |x| == |y| -> x (u = y / |x| = +-1: i = n - 1 or 0)
        ((1, 1, 0), (0 * 4 + 2) * 4 + 3), ((1, -1, 0), (0 * 4 + 2) * 4 + 0), ((-1, 1, 0), (1 * 4 + 2) * 4 + 3),
        ((0, 1, 1), (2 * 4 + 3) * 4 + 2), ((0, -1, 1), (3 * 4 + 3) * 4 + 2), ((0, 1, -1), (2 * 4 + 0) * 4 + 2),
        ((1, 0, 1), (0 * 4 + 3) * 4 + 2), ((-1, 0, -1), (1 * 4 + 0) * 4 + 2),
        # all three equal: axis 0, both coordinates at the clamp
        ((1, 1, 1), (0 * 4 + 3) * 4 + 3), ((-1, -1, -1), (1 * 4 + 0) * 4 + 0), ((2.5, -2.5, 2.5), (0 * 4 + 3) * 4 + 0),
        # u = +-1 exactly with v elsewhere; scale does not matter
        ((3, 3, 1.5), (0 * 4 + 3) * 4 + 3), ((3, -3, -1.5), (0 * 4 + 1) * 4 + 0), ((1e-30, 1e-30, 0), (0 * 4 + 2) * 4 + 3),
        ((1e30, 0, -1e30), (0 * 4 + 0) * 4 + 2),
        # no direction: zero (either sign) and NaN have no texel; an infinite major component divides the others to 0
        ((0, 0, 0), -1), ((-0.0, 0, 0), -1), ((NAN, NAN, NAN), -1), ((NAN, 0, 0), -1), ((0, NAN, 0), -1), ((0, 0, NAN), -1),
        ((INF, 0, 0), (0 * 4 + 2) * 4 + 2), ((0, -INF, 1), (3 * 4 + 2) * 4 + 2),
    ]
    d = np.array([c[0] for c in cases], dtype=np.float32)
    k = np.array([c[1] for c in cases], dtype=np.int32)
    return d, k


def random_directions(rng, count):
    d = rng.normal(size=(count, 3)).astype(np.float32)
    d[::7] *= np.float32(1e-20)                                   # scale must not matter
    d[3::11, rng.integers(3)] = 0                                  # a zero component
    return d
