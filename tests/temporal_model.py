"""numpy float32 model of pt_denoise_temporal (include/ptmi355.h) on top of atrous_model: the
reprojection of the previous temporal call's record into the current camera's grid, the blend with the running sum, the
state the calls carry.  All arithmetic is binary32, one rounding per operation, in the order written there, no FMA (dot
products are written out term by term: `@` / np.dot may fuse or reorder) -- the device's planes equal these bit for bit
(tests/test_gpu_temporal.py)."""
import numpy as np

import atrous_model as am

F = np.float32


def dot(v, a):
    """v [n, 3] float32 with the camera vector a (3 floats), left to right"""
    a = np.asarray(a, dtype=np.float32).reshape(3)
    return v[:, 0] * a[0] + v[:, 1] * a[1] + v[:, 2] * a[2]


def project(cam, pos, w, h):
    """The inverse of generateRayFromCamera for camera record `cam`, nearest pixel: (valid [n] bool, Q [n] int64; Q = 0
    where not valid) for world positions pos [n, 3]."""
    c = cam.reshape(-1)[0]
    v = (pos - np.asarray(c["position"], dtype=np.float32).reshape(1, 3)).astype(np.float32)
    z = dot(v, c["view"])
    pl = np.asarray(c["pixelLength"], dtype=np.float32).reshape(2)
    with np.errstate(all="ignore"):
        xs = F(w) * F(0.5) - dot(v, c["right"]) / (z * pl[0])
        ys = F(h) * F(0.5) - dot(v, c["up"]) / (z * pl[1])
        fx = np.floor(xs + F(0.5))
        fy = np.floor(ys + F(0.5))
        valid = (z > 0) & (fx >= 0) & (fx < F(w)) & (fy >= 0) & (fy < F(h))          # (false on NaN)
    q = np.where(valid, fy, 0).astype(np.int64) * w + np.where(valid, fx, 0).astype(np.int64)
    return valid, q


def reproject(old, g, materials, w, h, max_history, ptol, ntol):
    """old = {"camera", "g", "C" [n, 3], "N" [n]} reprojected for the G-buffer g of the new camera: (Hc [n, 3], Hn [n], Q [n]
    with -1 where the pixel has no history)."""
    n = w * h
    mat = g["materialId"].astype(np.int64)
    m = np.clip(mat, 0, len(materials) - 1)
    ok = (mat >= 0) & (mat < len(materials)) & (materials["hasReflective"][m] == 0) & (materials["hasRefractive"][m] == 0)
    pos, nrm, t = g["position"].astype(np.float32), g["normal"].astype(np.float32), g["t"].astype(np.float32)
    valid, q = project(old["camera"], pos, w, h)
    ok &= valid
    og = old["g"]
    ok &= og["materialId"][q] == g["materialId"]
    lim = F(ptol) * t
    with np.errstate(all="ignore"):
        ok &= am.d2(og["position"][q].astype(np.float32), pos) <= lim * lim
        ok &= am.d2(og["normal"][q].astype(np.float32), nrm) <= F(ntol) * F(ntol)
    hc = np.where(ok[:, None], old["C"][q], F(0)).astype(np.float32)
    hn = np.where(ok, np.minimum(old["N"][q], F(max_history)), F(0)).astype(np.float32)
    assert hc.shape == (n, 3) and hn.shape == (n,)
    return hc, hn, np.where(ok, q, -1)


def blend(image_sum, iteration, hc, hn):
    """c0 = (sum + Hc * Hn) / ((float)iter + Hn), N = (float)iter + Hn"""
    s = np.asarray(image_sum, dtype=np.float32).reshape(-1, 3)
    nn = (F(iteration) + hn).astype(np.float32)
    return ((s + hc * hn[:, None]) / nn[:, None]).astype(np.float32), nn


def filtered(c0, g, w, h, levels, sc, sn, sp):
    """the levels of atrous_model on c0 [n, 3]"""
    c = c0.reshape(h, w, 3)
    nrm, pos = g["normal"].reshape(h, w, 3).astype(np.float32), g["position"].reshape(h, w, 3).astype(np.float32)
    for i in range(levels):
        c = am.level(c, nrm, pos, 1 << i, F(sc) * F(2.0 ** -i), sn, sp)
    return c.reshape(-1, 3)


class Temporal:
    """The state pt_denoise_temporal carries from call to call."""

    def __init__(self, w, h, materials):
        self.w, self.h, self.materials = w, h, materials
        self.reset()

    def reset(self):
        self.cur = None
        self.hc = np.zeros((self.w * self.h, 3), dtype=np.float32)
        self.hn = np.zeros(self.w * self.h, dtype=np.float32)
        self.q = np.full(self.w * self.h, -1, dtype=np.int64)

    def call(self, image_sum, iteration, camera, g, levels=5, sc=1.0, sn=0.35, sp=0.5, max_history=64, ptol=0.1, ntol=0.1):
        """one pt_denoise_temporal(params, temporal, iteration) with the session's camera `camera`, whose G-buffer is g and
        whose running sum is image_sum [n, 3]; returns the denoised mean [n, 3]"""
        cam = np.ascontiguousarray(camera).copy()
        if self.cur is not None and self.cur["camera"].tobytes() != cam.tobytes():
            self.hc, self.hn, self.q = reproject(self.cur, g, self.materials, self.w, self.h, max_history, ptol, ntol)
        c0, nn = blend(image_sum, iteration, self.hc, self.hn)
        self.cur = {"camera": cam, "g": g, "C": c0, "N": nn}
        return filtered(c0, g, self.w, self.h, levels, sc, sn, sp)
