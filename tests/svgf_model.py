"""numpy float32 model of pt_denoise_svgf (include/ptmi355.h) on top of variance_model.py and
temporal_model.py: the luminance moments reprojected with the colour across camera moves, the variance estimated from them
-- temporally where a pixel's history is long enough, from its 7 x 7 neighbourhood where it is not -- and section 6.27's
levels on the blended colour (SVGF, Schied et al. 2017).  All arithmetic is binary32, one rounding per operation in the order
written, no FMA -- the device's planes equal these bit for bit (tests/test_gpu_svgf.py)."""
import numpy as np

import temporal_model as tm
import variance_model as vm

F = np.float32


def reproject(old, g, materials, w, h, max_history, ptol, ntol):
    """old = {"camera", "g", "C" [n, 3], "U1" [n], "U2" [n], "N" [n]} reprojected for the G-buffer g of the new camera: section
    6.15's tests (temporal_model.reproject), the moments gathered at the same Q; (Hc, H1, H2, Hn, Q)."""
    hc, hn, q = tm.reproject(old, g, materials, w, h, max_history, ptol, ntol)
    ok = q >= 0
    qq = np.where(ok, q, 0)
    h1 = np.where(ok, old["U1"][qq], F(0)).astype(np.float32)
    h2 = np.where(ok, old["U2"][qq], F(0)).astype(np.float32)
    return hc, h1, h2, hn, q


def blend(image_sum, m1, m2, iteration, hc, h1, h2, hn):
    """c0 = (sum + Hc * Hn) / N', u1 = (M1 + H1 * Hn) / N', u2 = (M2 + H2 * Hn) / N', N' = (float)iter + Hn"""
    c0, nn = tm.blend(image_sum, iteration, hc, hn)
    u1 = ((np.asarray(m1, dtype=np.float32) + h1 * hn) / nn).astype(np.float32)
    u2 = ((np.asarray(m2, dtype=np.float32) + h2 * hn) / nn).astype(np.float32)
    return c0, u1, u2, nn


def temporal_variance(u1, u2, nn):
    """vt = fmaxf(u2 - u1 * u1, 0) / fmaxf(N' - 1, 1)"""
    return (np.fmax(u2 - u1 * u1, F(0)) / np.fmax(nn - F(1), F(1))).astype(np.float32)


def spatial_variance(u1, u2, nn, nrm, pos, sn, sp):
    """The 7 x 7 estimate on u1, u2, nn [H, W] and nrm, pos [H, W, 3]: dy outer, taps outside the image skipped, the weights
    those of the levels' normal and position stops; fmaxf(s2 / cum - (s1 / cum)^2, 0) / N'."""
    hh, ww = u1.shape
    s1 = np.zeros((hh, ww), np.float32)
    s2 = np.zeros((hh, ww), np.float32)
    cum = np.zeros((hh, ww), np.float32)
    sn2, sp2 = F(sn) * F(sn), F(sp) * F(sp)
    for dy in range(-3, 4):
        for dx in range(-3, 4):
            y0, y1 = max(0, -dy), min(hh, hh - dy)
            x0, x1 = max(0, -dx), min(ww, ww - dx)
            if y0 >= y1 or x0 >= x1:
                continue
            P = (slice(y0, y1), slice(x0, x1))
            Q = (slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx))
            w = vm.exp_neg(vm.d2(nrm[P], nrm[Q]) / sn2) * vm.exp_neg(vm.d2(pos[P], pos[Q]) / sp2)
            s1[P] = s1[P] + u1[Q] * w
            s2[P] = s2[P] + u2[Q] * w
            cum[P] = cum[P] + w
    a, b = s1 / cum, s2 / cum
    return (np.fmax(b - a * a, F(0)) / nn).astype(np.float32)


def variance(u1, u2, nn, nrm, pos, w, h, spatial_below, sn, sp):
    """var_0 [n]: the spatial estimate where N' < (float)spatial_below, the temporal one elsewhere"""
    vt = temporal_variance(u1, u2, nn)
    low = nn < F(spatial_below)
    if not low.any():
        return vt
    vs = spatial_variance(u1.reshape(h, w), u2.reshape(h, w), nn.reshape(h, w), nrm.reshape(h, w, 3), pos.reshape(h, w, 3), sn, sp)
    return np.where(low, vs.reshape(-1), vt).astype(np.float32)


class Svgf:
    """The state pt_denoise_svgf carries from call to call (its own: not pt_denoise_temporal's)."""

    def __init__(self, w, h, materials):
        self.w, self.h, self.materials = w, h, materials
        self.reset()

    def reset(self):
        n = self.w * self.h
        self.cur = None
        self.hc = np.zeros((n, 3), dtype=np.float32)
        self.h1 = np.zeros(n, dtype=np.float32)
        self.h2 = np.zeros(n, dtype=np.float32)
        self.hn = np.zeros(n, dtype=np.float32)
        self.q = np.full(n, -1, dtype=np.int64)
        self.var0 = None

    def call(self, image_sum, m1, m2, iteration, camera, g, levels=5, sl=4.0, sn=0.35, sp=0.5, max_history=64, ptol=0.1, ntol=0.1,
             spatial_below=4):
        """one pt_denoise_svgf(params, temporal, spatial_below, iteration) with the session's camera `camera`, whose G-buffer is
        g, running sum image_sum [n, 3] and moments m1, m2 [n]; returns the denoised mean [n, 3] (var_0 stays in self.var0)"""
        w, h = self.w, self.h
        cam = np.ascontiguousarray(camera).copy()
        if self.cur is not None and self.cur["camera"].tobytes() != cam.tobytes():
            self.hc, self.h1, self.h2, self.hn, self.q = reproject(self.cur, g, self.materials, w, h, max_history, ptol, ntol)
        c0, u1, u2, nn = blend(image_sum, np.asarray(m1).reshape(-1), np.asarray(m2).reshape(-1), iteration, self.hc, self.h1, self.h2, self.hn)
        nrm, pos = g["normal"].astype(np.float32), g["position"].astype(np.float32)
        self.var0 = variance(u1, u2, nn, nrm, pos, w, h, spatial_below, sn, sp)
        self.cur = {"camera": cam, "g": g, "C": c0, "U1": u1, "U2": u2, "N": nn}
        c, v = c0.reshape(h, w, 3), self.var0.reshape(h, w)
        for i in range(levels):
            c, v = vm.level(c, v, nrm.reshape(h, w, 3), pos.reshape(h, w, 3), 1 << i, sl, sn, sp)
        return c.reshape(-1, 3)
