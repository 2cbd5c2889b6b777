// Bump mapping (PT_TEXTURES): steps 1-8 of the specification, shared by the kernels, the probes and the
// host-only entry point pt_bump_normal.  Plain C++ apart from the device's normalise: a host compiler takes this file alone
// (tests/tools/bump_main.cpp drives it under the sanitizers), pt_device.hpp includes it for the device.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define PT_BUMP_FN __host__ __device__ __forceinline__
#else
#define PT_BUMP_FN inline
#endif

namespace ptd {

constexpr uint32_t BUMP_SPHERE = 0, BUMP_CUBE = 1;      // pt_geom_type's PT_SPHERE, PT_CUBE (include/ptmi355.h)
// a bump map's texel as the device keeps it: the two slopes, one 8-byte load
struct alignas(8) bump_texel { float da, db; };

// env_texel that also reports the face it chose: the major axis (0 x, 1 y, 2 z; ties go to the earlier axis) and whether the
// major component is negative.  The same arithmetic, kept beside env_texel instead of under it so that the kernels that
// call env_texel alone compile to what they were.  Host and device.
PT_BUMP_FN int env_texel_face(float dx, float dy, float dz, int n, int &axis, bool &negative) {
    const float ax = __builtin_fabsf(dx), ay = __builtin_fabsf(dy), az = __builtin_fabsf(dz);
    float m, major, a, b;
    if (ax >= ay && ax >= az) { axis = 0; m = ax; major = dx; a = dy; b = dz; }
    else if (ay >= az)        { axis = 1; m = ay; major = dy; a = dx; b = dz; }
    else                      { axis = 2; m = az; major = dz; a = dx; b = dy; }
    negative = major < 0.0f;
    if (!(m > 0.0f)) return -1;
    const int face = 2 * axis + (negative ? 1 : 0);
    const float u = a / m, v = b / m;
    const float fn = (float)n;
    const int i = (int)__builtin_fmaxf((u * 0.5f + 0.5f) * fn, 0.0f), j = (int)__builtin_fmaxf((v * 0.5f + 0.5f) * fn, 0.0f);
    return (face * n + (j < n - 1 ? j : n - 1)) * n + (i < n - 1 ? i : n - 1);
}
// steps 1 and 3-8 of section 6.22 for a hit at the object-space point q (step 2: q = multiplyMV(inverseTransform, (P, 1))) of
// a sphere or cube (`type`) whose gather record is `rec` (inverseTransform, transform, a sphere's invTranspose: 12 words each,
// 4 columns x 3 rows).  I: the ray's direction, nr: the normal the intersection test reported, B: the map's texels {da, db},
// n x n per face.  True when the hit is perturbed: ns is then the shading normal; false leaves ns alone.  Host and device --
// the device normalises through the kernels' gated form, the host by glm's v * (1 / sqrt(dot)), which it equals bit for bit.
template <typename P> PT_BUMP_FN bool bump_normal_q(uint32_t type, P rec, float qx, float qy, float qz,
                                                                             float Ix, float Iy, float Iz, float nrx, float nry, float nrz,
                                                                             const bump_texel *B, int n, float &nsx, float &nsy, float &nsz) {
    if (!((Ix * nrx + Iy * nry) + Iz * nrz < 0.0f)) return false;          // 1: the inside of a cube reports the exit face
    int axis;
    bool negative;
    const int k = env_texel_face(qx, qy, qz, n, axis, negative);           // 3
    if (k < 0) return false;
    const bump_texel e = B[k];                                                  // 4 (a NaN goes on to step 6)
    if (e.da == 0.0f && e.db == 0.0f) return false;
    // 5: da goes to the earlier of the two in-plane axes, db to the later (selects, no indexed array: registers only)
    float ux, uy, uz;
    int off;
    if (type == BUMP_CUBE) {
        const float major = negative ? -1.0f : 1.0f;
        ux = axis == 0 ? major : e.da;
        uy = axis == 0 ? e.da : axis == 1 ? major : e.db;
        uz = axis == 2 ? major : e.db;
        off = 12;                                                           // 6: cube_normal's rule, the transform
    } else {
        ux = qx + qx; uy = qy + qy; uz = qz + qz;
        if (axis != 0) ux = ux + e.da;
        if (axis == 0) uy = uy + e.da; else if (axis == 2) uy = uy + e.db;
        if (axis != 2) uz = uz + e.db;
        off = 24;                                                           //    a sphere's, the inverse transpose
    }
    const float wx = (rec[off + 0] * ux + rec[off + 3] * uy) + (rec[off + 6] * uz + rec[off + 9] * 0.0f);
    const float wy = (rec[off + 1] * ux + rec[off + 4] * uy) + (rec[off + 7] * uz + rec[off + 10] * 0.0f);
    const float wz = (rec[off + 2] * ux + rec[off + 5] * uy) + (rec[off + 8] * uz + rec[off + 11] * 0.0f);
    float x, y, z;
#if defined(__HIP_DEVICE_COMPILE__)
    const f3 w = normalize(mk(wx, wy, wz));                                 // (declared by pt_device.hpp, which includes this file)
    x = w.x; y = w.y; z = w.z;
#else
    const float inv_len = 1.0f / __builtin_sqrtf((wx * wx + wy * wy) + wz * wz);
    x = wx * inv_len; y = wy * inv_len; z = wz * inv_len;
#endif
    if ((x * nrx + y * nry) + z * nrz < 0.0f) { x = -x; y = -y; z = -z; }   // 7: a sphere hit from inside
    if (!((x * nrx + y * nry) + z * nrz > 0.0f)) return false;
    if (!((Ix * x + Iy * y) + Iz * z < 0.0f)) return false;                // 8
    nsx = x; nsy = y; nsz = z;
    return true;
}
// steps 1-8 from the world point P (step 2 as texture_texel computes it)
template <typename P> PT_BUMP_FN bool bump_normal(uint32_t type, P rec, float px, float py, float pz,
                                                                           float Ix, float Iy, float Iz, float nrx, float nry, float nrz,
                                                                           const bump_texel *B, int n, float &nsx, float &nsy, float &nsz) {
    const float qx = (rec[0] * px + rec[3] * py) + (rec[6] * pz + rec[9]);
    const float qy = (rec[1] * px + rec[4] * py) + (rec[7] * pz + rec[10]);
    const float qz = (rec[2] * px + rec[5] * py) + (rec[8] * pz + rec[11]);
    return bump_normal_q(type, rec, qx, qy, qz, Ix, Iy, Iz, nrx, nry, nrz, B, n, nsx, nsy, nsz);
}
}  // namespace ptd

#undef PT_BUMP_FN
