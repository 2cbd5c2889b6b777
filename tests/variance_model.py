"""numpy float32 model of PT_MOMENTS and pt_denoise_variance (include/ptmi355.h): the per-pixel luminance
moments a flagged session keeps, and the A-trous filter whose colour stop is the pixel's own measured noise (the core of SVGF,
Schied et al. 2017) on top of atrous_model.py's exp_neg / d2 / H5 / rgba8.  All arithmetic is binary32, one rounding per
operation in the order written, no FMA -- the device's result equals this model's bit for bit (tests/test_gpu_variance.py)."""
import numpy as np

from atrous_model import F, H5, d2, exp_neg, rgba8  # noqa: F401

LUM = (F(0.2126), F(0.7152), F(0.0722))                     # PT_DIRECT_SKY's weights
G3 = np.array([1 / 4, 1 / 2, 1 / 4], dtype=np.float32)
VAR_FLOOR = F(2.0 ** -40)


def lum(c):
    """(0.2126f r + 0.7152f g) + 0.0722f b on [..., 3] float32"""
    c = np.asarray(c, dtype=np.float32)
    return (LUM[0] * c[..., 0] + LUM[1] * c[..., 1]) + LUM[2] * c[..., 2]


def accumulate(m1, m2, sample):
    """One iteration gathered: M1 + l, M2 + l * l with l the luminance of the colour the iteration's path ended with ([n, 3]
    float32; a path that ended with colour 0 has l = 0).  Returns the new planes."""
    l = lum(sample)
    return (m1 + l).astype(np.float32), (m2 + l * l).astype(np.float32)


def moments(samples):
    """The planes after the iterations `samples` (an iterable of [n, 3] float32 per-sample colours), from zero, in order."""
    m1 = m2 = None
    for s in samples:
        if m1 is None:
            m1, m2 = np.zeros(len(s), np.float32), np.zeros(len(s), np.float32)
        m1, m2 = accumulate(m1, m2, s)
    return m1, m2


def var0(m1, m2, iteration):
    """The variance of the MEAN's luminance: fmaxf(M2 / n - mu * mu, 0) / fmaxf(n - 1, 1), mu = M1 / n (C's fmaxf: a NaN gives the
    other operand).  iteration = 1 gives exactly 0."""
    n = F(iteration)
    mu = np.asarray(m1, dtype=np.float32) / n
    return (np.fmax(np.asarray(m2, dtype=np.float32) / n - mu * mu, F(0)) / np.fmax(n - F(1), F(1))).astype(np.float32)


def prefilter(var):
    """gv: the 3 x 3 Gaussian {1/4, 1/2, 1/4}^2 of var [H, W], coordinates clamped to the image, dy outer, from acc = 0"""
    hh, ww = var.shape
    ys, xs = np.arange(hh), np.arange(ww)
    acc = np.zeros((hh, ww), np.float32)
    for dy in (-1, 0, 1):
        yy = np.clip(ys + dy, 0, hh - 1)
        for dx in (-1, 0, 1):
            xx = np.clip(xs + dx, 0, ww - 1)
            acc = acc + var[yy][:, xx] * (G3[dy + 1] * G3[dx + 1])
    return acc


def level(c, var, nrm, pos, step, sl, sn, sp):
    """One level with taps `step` pixels apart on c, nrm, pos [H, W, 3] and var [H, W]; a tap outside the image is skipped.
    Returns (c', var')."""
    hh, ww, _ = c.shape
    den = F(sl) * np.sqrt(np.fmax(prefilter(var), VAR_FLOOR))
    L = lum(c)
    s = np.zeros_like(c)
    vs = np.zeros((hh, ww), np.float32)
    cum = np.zeros((hh, ww), np.float32)
    sn2, sp2 = F(sn) * F(sn), F(sp) * F(sp)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            oy, ox = dy * step, dx * step
            y0, y1 = max(0, -oy), min(hh, hh - oy)
            x0, x1 = max(0, -ox), min(ww, ww - ox)
            if y0 >= y1 or x0 >= x1:
                continue
            P = (slice(y0, y1), slice(x0, x1))
            Q = (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))
            w = exp_neg(np.abs(L[P] - L[Q]) / den[P]) * exp_neg(d2(nrm[P], nrm[Q]) / sn2) * exp_neg(d2(pos[P], pos[Q]) / sp2)
            wt = w * (H5[dy + 2] * H5[dx + 2])
            s[P] = s[P] + c[Q] * wt[..., None]
            vs[P] = vs[P] + var[Q] * (wt * wt)
            cum[P] = cum[P] + wt
    return s / cum[..., None], vs / (cum * cum)


def denoise(image_sum, m1, m2, iteration, nrm, pos, levels, sl, sn, sp, with_var=False):
    """pt_denoise_variance: image_sum [H, W, 3] (the running sum), m1 / m2 [H, W] (the moments), nrm / pos [H, W, 3] (the
    G-buffer); returns the denoised mean (with_var: and the variance that travelled with it).  sl is not halved per level."""
    c = (np.asarray(image_sum, dtype=np.float32) / F(iteration)).astype(np.float32)
    v = var0(m1, m2, iteration)
    for i in range(levels):
        c, v = level(c, v, nrm, pos, 1 << i, sl, sn, sp)
    return (c, v) if with_var else c
