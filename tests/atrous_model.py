"""numpy float32 model of the edge-avoiding A-trous filter (Dammertz et al. 2010) that pt_denoise runs on the device:
DESIGN.md section 6.14 / include/ptmi355.h.  All arithmetic is binary32, one rounding per operation, in the order written
there, no FMA -- the device's result equals this model's bit for bit (tests/test_gpu_denoise.py).  Vectorised per tap:
five levels of 800x800 take a few seconds."""
import math

import numpy as np

F = np.float32
H5 = np.array([1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16], dtype=np.float32)
EXP_C = [F(((-1.0) ** i) / math.factorial(i)) for i in range(9)]        # Taylor of e^-r, degree 8
X_MAX = F(25.0)
LOG2E = F(1.44269504)
LN2 = F(0.693147182)


def exp_neg(x):
    """exp(-x) for x >= 0, the edge-stopping function (the specification's own: libm's and the device's expf differ)."""
    x = np.minimum(np.asarray(x, dtype=np.float32), X_MAX)
    k = np.floor(x * LOG2E)
    r = x - k * LN2
    p = np.full_like(r, EXP_C[8])
    for i in range(7, -1, -1):
        p = p * r + EXP_C[i]
    return np.minimum(np.ldexp(p, -k.astype(np.int32)).astype(np.float32), F(1.0))


def d2(a, b):
    d = a - b
    return d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]          # left to right


def level(c, nrm, pos, step, sc, sn, sp):
    """One level with taps `step` pixels apart on [H, W, 3] float32 arrays; a tap outside the image is skipped."""
    hh, ww, _ = c.shape
    s = np.zeros_like(c)
    cum = np.zeros((hh, ww), np.float32)
    sc2, sn2, sp2 = F(sc) * F(sc), F(sn) * F(sn), F(sp) * F(sp)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            oy, ox = dy * step, dx * step
            y0, y1 = max(0, -oy), min(hh, hh - oy)
            x0, x1 = max(0, -ox), min(ww, ww - ox)
            if y0 >= y1 or x0 >= x1:
                continue
            P = (slice(y0, y1), slice(x0, x1))
            Q = (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))
            w = exp_neg(d2(c[P], c[Q]) / sc2) * exp_neg(d2(nrm[P], nrm[Q]) / sn2) * exp_neg(d2(pos[P], pos[Q]) / sp2)
            wt = w * (H5[dy + 2] * H5[dx + 2])
            s[P] = s[P] + c[Q] * wt[..., None]
            cum[P] = cum[P] + wt
    return s / cum[..., None]


def denoise(image_sum, iteration, nrm, pos, levels, sc, sn, sp):
    """The filter: image_sum [H, W, 3] (the running sum), nrm / pos [H, W, 3] (the G-buffer); returns the denoised mean."""
    c = (np.asarray(image_sum, dtype=np.float32) / F(iteration)).astype(np.float32)
    for i in range(levels):
        c = level(c, nrm, pos, 1 << i, F(sc) * F(2.0 ** -i), sn, sp)
    return c


def rgba8(rgb):
    """sendImageToPBO's rule with divisor 1 on [n, 3] float32: (int)((double)c * 255.0) clamped to [0, 255]; alpha 0."""
    v = np.asarray(rgb, dtype=np.float32).astype(np.float64) * 255.0
    v = np.where(np.isnan(v), 0.0, v)
    q = np.clip(np.trunc(np.clip(v, -1e9, 1e9)), 0, 255).astype(np.uint8)
    out = np.zeros(q.shape[:-1] + (4,), dtype=np.uint8)
    out[..., :3] = q
    return out


def gbuffer_from_oracle(po, cam, depth, geoms, triangles=None, meshes=None):
    """The G-buffer as the specification defines it, from the oracle: generate_rays + compute_intersections, position =
    origin + direction * t in float32 (one multiply, one add per component); zeros / -1 on a miss."""
    paths = po.generate_rays(cam, depth)
    kw = {}
    if triangles is not None:
        kw = {"tris": triangles, "meshes": meshes}
    isects, _ = po.compute_intersections(paths, geoms, **kw)
    t = isects["t"].astype(np.float32)
    hit = t > 0
    o = paths["origin"].astype(np.float32)
    d = paths["direction"].astype(np.float32)
    pos = np.where(hit[:, None], o + d * t[:, None], F(0)).astype(np.float32)
    nrm = np.where(hit[:, None], isects["normal"], F(0)).astype(np.float32)
    mat = np.where(hit, isects["materialId"], -1).astype(np.int32)
    tt = np.where(hit, t, F(-1.0)).astype(np.float32)
    return {"t": tt, "normal": nrm, "position": pos, "materialId": mat}
