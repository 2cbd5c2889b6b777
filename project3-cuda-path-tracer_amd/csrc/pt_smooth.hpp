// Smooth shading of triangle meshes (PT_SMOOTH_NORMALS): steps 1-5 of the specification, shared by the
// kernels, the probe and the host-only entry point pt_smooth_normal.  Plain C++ apart from the device's normalise: a host
// compiler takes this file alone (tests/tools/smooth_main.cpp drives it under the sanitizers), pt_device.hpp includes it for
// the device.  Binary32, one rounding per operation in the order written (the library and the driver are built with
// -ffp-contract=off).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define PT_SMOOTH_FN __host__ __device__ __forceinline__
#else
#define PT_SMOOTH_FN inline
#endif

namespace ptd {

// steps 1-5 of section 6.26 for a hit of the ray (o, I) on a triangle whose record `tv` holds v0, e1 = fl(v1 - v0), e2 = fl(v2 - v0)
// (nine words, as the device's triangle records begin) and whose vertex normals are `vn` = n0, n1, n2 (nine words).  nr: the
// facet normal the intersection reported.  True when the hit is smoothed: ns is then the shading normal; false leaves ns alone.
// Host and device -- the device normalises through the kernels' gated form, the host by glm's v * (1 / sqrt(dot)), which it
// equals bit for bit.
template <typename T, typename N> PT_SMOOTH_FN bool smooth_normal(T tv, N vn, float ox, float oy, float oz, float Ix, float Iy, float Iz,
                                                                  float nrx, float nry, float nrz, float &nsx, float &nsy, float &nsz) {
    const float v0x = tv[0], v0y = tv[1], v0z = tv[2], e1x = tv[3], e1y = tv[4], e1z = tv[5], e2x = tv[6], e2y = tv[7], e2z = tv[8];
    // 1: the barycentrics of glm::intersectRayTriangle, as ptd::ray_triangle computed them (cross and dot in glm's order)
    const float px = Iy * e2z - e2y * Iz, py = Iz * e2x - e2z * Ix, pz = Ix * e2y - e2x * Iy;
    const float a = (e1x * px + e1y * py) + e1z * pz;
    const float f = 1.0f / a;
    const float sx = ox - v0x, sy = oy - v0y, sz = oz - v0z;
    const float bx = f * ((sx * px + sy * py) + sz * pz);
    const float qx = sy * e1z - e1y * sz, qy = sz * e1x - e1z * sx, qz = sx * e1y - e1x * sy;
    const float by = f * ((Ix * qx + Iy * qy) + Iz * qz);
    const float bw = (1.0f - bx) - by;
    // 2: the interpolated normal; an all-zero triple (or anything without a finite positive length) leaves the hit faceted
    const float wx = (vn[0] * bw + vn[3] * bx) + vn[6] * by;
    const float wy = (vn[1] * bw + vn[4] * bx) + vn[7] * by;
    const float wz = (vn[2] * bw + vn[5] * bx) + vn[8] * by;
    const float l2 = (wx * wx + wy * wy) + wz * wz;
    if (!(l2 > 0.0f && l2 < __builtin_inff())) return false;
    // 3
    float x, y, z;
#if defined(__HIP_DEVICE_COMPILE__)
    const f3 w = normalize(mk(wx, wy, wz));                                 // (declared by pt_device.hpp, which includes this file)
    x = w.x; y = w.y; z = w.z;
#else
    const float inv_len = 1.0f / __builtin_sqrtf(l2);
    x = wx * inv_len; y = wy * inv_len; z = wz * inv_len;
#endif
    if (!((x * nrx + y * nry) + z * nrz > 0.0f)) return false;              // 4: meshes are one-sided, no flip
    if (!((Ix * x + Iy * y) + Iz * z < 0.0f)) return false;                 // 5
    nsx = x; nsy = y; nsz = z;
    return true;
}
}  // namespace ptd

#undef PT_SMOOTH_FN
