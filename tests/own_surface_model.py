"""Numpy model of the own-surface form of the cull (csrc/pt_k_scene.hpp: own_surface_miss, csrc/pt_k_intersect.hpp:
cull_scene<.., OWN>) beside tests/cull_model.py's model of the per-primitive form: the row test in the straight-line
order, once per ray against the row of the primitive the ray leaves."""
import numpy as np

import cull_model

F = np.float32


def own_miss(rays, row):
    """rays[n, 6] float32; row[4] = the primitive's reject row (zeros: none).  (m0 x + m1 y) + (m2 z + m3) for the origin,
    (m0 x + m1 y) + m2 z for the direction, every operation rounded to binary32 -- whatever the row's mode."""
    o, d, row = rays[:, :3].astype(F), rays[:, 3:].astype(F), np.asarray(row, dtype=F)
    with np.errstate(all="ignore"):
        qk = ((row[0] * o[:, 0]).astype(F) + (row[1] * o[:, 1]).astype(F)).astype(F) + ((row[2] * o[:, 2]).astype(F) + row[3]).astype(F)
        vk = ((row[0] * d[:, 0]).astype(F) + (row[1] * d[:, 1]).astype(F)).astype(F) + (row[2] * d[:, 2]).astype(F)
        qk, vk = qk.astype(F), vk.astype(F)
        return (np.abs(qk) > F(0.5)) & ((qk * vk).astype(F) > F(0))


def per_mode_miss(rays, reject):
    """the per-primitive form's row test alone (cull_model.candidates without the box): reject = (mode, row[4])"""
    inf_box = np.array([[-np.inf] * 3, [np.inf] * 3], dtype=F)
    with_row, wild = cull_model.candidates(rays, inf_box, F(np.inf), reject)
    return ~with_row & ~wild


def candidates_own(rays, own, boxes, rmax, rejects):
    """the own-surface form: per primitive g, box & ~(own == g & own_miss) | wild.  own[n]: the primitive each ray left
    (-1: none).  Returns [ngeoms, n]."""
    miss = np.zeros(len(rays), dtype=bool)
    for g in range(len(boxes)):
        sel = own == g
        if sel.any():
            miss[sel] = own_miss(rays[sel], rejects[g, 1:5])
    out = []
    for g in range(len(boxes)):
        box_only, wild = cull_model.candidates(rays, boxes[g], rmax, None)
        out.append((box_only & ~((own == g) & miss)) | wild)
    return np.array(out)


def leaving_rays(geoms, rng, per_face=40):
    """Rays that start a hair above (outside) or below (inside: glass) a random point of every face of every cube of
    `geoms`, heading anywhere; float32 [n, 6] and the primitive each one leaves."""
    rays, own = [], []
    for g, c in enumerate(geoms):
        if int(c["type"]) != 1:
            continue
        T = c["transform"].astype(np.float64).T
        for axis in range(3):
            for sgn in (-1.0, 1.0):
                e = np.zeros(3)
                e[axis] = sgn
                p = 0.5 * e + rng.uniform(-0.5, 0.5, (per_face, 3)) * (1 - np.abs(e))
                pw = (np.concatenate([p, np.ones((per_face, 1))], 1) @ T.T)[:, :3]
                nw = (T[:3, :3] @ e)
                nw = nw / max(np.linalg.norm(nw), 1e-30)
                side = np.where(rng.random(per_face) < 0.75, 1.0, -1.0)[:, None]
                o = pw + side * nw * rng.choice([1e-6, 1e-5, 1e-4, 3e-4], (per_face, 1))
                d = rng.normal(size=(per_face, 3))
                d /= np.linalg.norm(d, axis=1, keepdims=True)
                rays.append(np.concatenate([o, d], 1))
                own += [g] * per_face
    return np.concatenate(rays).astype(F), np.array(own)
