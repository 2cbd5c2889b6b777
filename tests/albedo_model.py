"""numpy float32 model of first-hit albedo demodulation in the filters (pt_set_denoise_albedo / pt_albedo; include/ptmi355.h,
DESIGN.md section 6.20) on top of atrous_model, temporal_model and texture_model, none of which is changed: the albedo plane
of a camera, pt_denoise and pt_denoise_temporal with the switch on.  All arithmetic is binary32, one rounding per operation,
in the order written there, no FMA -- the device's planes equal these bit for bit (tests/test_gpu_albedo.py)."""
import numpy as np

import atrous_model as am
import temporal_model as tpm
import texture_model as tm

F = np.float32
A_MIN = F(2.0 ** -6)
A_MAX = F(2.0 ** 6)


def clamp(v):
    """a = fminf(fmaxf(v, 2^-6), 2^6) per component with C's fmaxf / fminf: a NaN gives 2^-6"""
    return np.fmin(np.fmax(np.asarray(v, dtype=np.float32), A_MIN), A_MAX).astype(np.float32)


def albedo(po, geoms, materials, textures, cam, depth, tris=None, meshes=None):
    """The albedo plane of camera `cam`, [npix, 3] float32: 1 on a miss and on a specular first hit, the clamped mcol of every
    other first hit.  textures: {material: [6, n, n, 3]} -- the textures the session's bounce kernels shade with (an empty
    dict for a session without PT_TEXTURES, with PT_FAKE_SHADER or without a texture set)."""
    geoms = np.ascontiguousarray(geoms).view(po.GEOM_DT)
    mats = np.ascontiguousarray(materials).view(po.MATERIAL_DT)
    if tris is not None:
        tris, meshes = np.ascontiguousarray(tris).view(po.TRI_DT), np.ascontiguousarray(meshes).view(po.MESH_DT)
    paths = po.generate_rays(cam, depth)
    isects, _ = po.compute_intersections(paths, geoms, tris, meshes)
    hit = isects["t"] > 0
    textures = dict(textures or {})
    if textures:
        hg = tm.hit_geoms(po, geoms, tris, meshes, paths, isects)
    else:
        hg = np.where(hit, 0, -1).astype(np.int32)
    v = tm.mcol(po, geoms, mats, textures, paths, isects, hg)
    m = mats[np.clip(isects["materialId"], 0, len(mats) - 1)]
    with np.errstate(invalid="ignore"):
        specular = (m["hasReflective"] > 0) | (m["hasRefractive"] > 0)
    plain = hit & ~specular
    return np.where(plain[:, None], clamp(v), F(1.0)).astype(np.float32)


def denoise(image_sum, iteration, A, nrm, pos, levels, sc, sn, sp):
    """pt_denoise with the switch on: image_sum, A, nrm, pos [H, W, 3]; returns the denoised mean.  c_0 = (sum / iter) / A, the
    levels of atrous_model on c, the result times A; levels = 0 is the mean untouched."""
    mean = (np.asarray(image_sum, dtype=np.float32) / F(iteration)).astype(np.float32)
    if levels == 0:
        return mean
    A = np.asarray(A, dtype=np.float32).reshape(mean.shape)
    with np.errstate(all="ignore"):
        c = (mean / A).astype(np.float32)
        for i in range(levels):
            c = am.level(c, nrm, pos, 1 << i, F(sc) * F(2.0 ** -i), sn, sp)
        return (c * A).astype(np.float32)


class Temporal(tpm.Temporal):
    """pt_denoise_temporal's state with the switch: steps 1 and 2 (reprojection, blend, cur) are temporal_model's, in modulated
    colour; step 3 filters c0 / A and multiplies back.  A = None: the switch is off."""

    def call(self, image_sum, iteration, camera, g, A=None, levels=5, sc=1.0, sn=0.35, sp=0.5, max_history=64, ptol=0.1, ntol=0.1):
        cam = np.ascontiguousarray(camera).copy()
        if self.cur is not None and self.cur["camera"].tobytes() != cam.tobytes():
            self.hc, self.hn, self.q = tpm.reproject(self.cur, g, self.materials, self.w, self.h, max_history, ptol, ntol)
        c0, nn = tpm.blend(image_sum, iteration, self.hc, self.hn)
        self.cur = {"camera": cam, "g": g, "C": c0, "N": nn}
        if A is None or levels == 0:
            return tpm.filtered(c0, g, self.w, self.h, levels, sc, sn, sp)
        A = np.asarray(A, dtype=np.float32).reshape(-1, 3)
        with np.errstate(all="ignore"):
            c = tpm.filtered((c0 / A).astype(np.float32), g, self.w, self.h, levels, sc, sn, sp)
            return (c * A).astype(np.float32)
