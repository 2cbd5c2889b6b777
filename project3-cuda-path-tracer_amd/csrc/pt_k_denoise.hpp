// pt_k_denoise.hpp -- the first-hit G-buffer of the current camera (k_gbuffer) and the edge-avoiding A-trous wavelet filter of
// the accumulated image (k_atrous, k_denoise_mean); Dammertz et al. 2010, the specification in DESIGN.md section 6.14
// (one of the kernel-family headers of libptmi355.so, included by pt_kernels.hpp in dependency order; ptmi355.hip is the
// only translation unit)
#pragma once

namespace {

// G-buffer layout: two 16-byte records per pixel, the filter's tap is two 16-byte loads
//   gA[pixel] = {normal.x, normal.y, normal.z, t}          (a miss: 0, 0, 0, -1)
//   gB[pixel] = {position.x, position.y, position.z, bits(materialId)}     (a miss: 0, 0, 0, -1)
// The ray is generateRayFromCamera's pinhole ray whatever the session's jitter / lens (camera_ray with a zero Lens draws
// nothing); the first hit goes through the cull / exact-test code of every other kernel that intersects (k_cache_first is
// the same loop with another output).  Whole-frame sessions only: local pixel = pixelIndex.
// (Register budget: PT_MIN_WAVES waves per SIMD like k_cache_first, except with the every-triangle loop inline, which does
// not fit 128 registers -- k_cache_first spills 28-33 there --: two waves per SIMD for a kernel that runs once per camera.)
template <int MESH, bool SLDS>
__global__ __launch_bounds__(BLOCK, MESH == MESH_TILES ? 2 : PT_MIN_WAVES) void k_gbuffer(float4 *__restrict__ gA, float4 *__restrict__ gB, SceneDev sc,
                                                                  pt_camera cam, TileMap map) {
    extern __shared__ __attribute__((aligned(16))) float lds_raw[];
    const LdsCarve lc = carve_lds(lds_raw, sc, SLDS);
    const SceneAcc acc = stage_scene<SLDS>(lc.scene, sc);
    WaveQ q{lc.pw, 0, 0};
    const uint32_t n = (uint32_t)map.tile_pixels;
    const uint32_t tiles = (n + BLOCK - 1) / BLOCK;
    for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const uint32_t j = tile * BLOCK + threadIdx.x;
        const bool active = j < n;
        f3 ro = ptd::mk(cam.position.x, cam.position.y, cam.position.z), rd = ptd::mk(0, 0, 1);
        if (active) camera_ray(cam, Lens{0, 0.0f, 0.0f}, 0, 0, (int)j, map.W, ro, rd);
        MeshBest mb;
        cull_scene<MESH>(sc, acc, q, 0, lc.tri, active, ro, rd, mb, nullptr);
        drain_to(q, acc, q.total);
        if (active) {
            float t; f3 nrm; int mat, outside;
            tile_result(q, 0, acc, sc.tris, mb, t, nrm, mat, outside);
            float4 a = make_float4(0.0f, 0.0f, 0.0f, -1.0f), b = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(-1));
            if (t > 0.0f) {
                // position = origin + direction * t, per component one multiply then one add (not getPointOnRay)
                a = make_float4(nrm.x, nrm.y, nrm.z, t);
                b = make_float4(ro.x + rd.x * t, ro.y + rd.y * t, ro.z + rd.z * t, __int_as_float(mat));
            }
            gA[j] = a; gB[j] = b;
        }
    }
}

// exp(-x) for x >= 0, the edge-stopping function: the device's expf and libm's differ, so the specification carries its own
// (as DESIGN.md section 4 does for sin / cos).  Clamp at 25, k = floor(x log2 e), r = x - k ln 2, the degree-8 Taylor
// polynomial of e^-r by Horner (one multiply and one add per step, no FMA: -ffp-contract=off), scaled by 2^-k -- a
// multiplication by an exact power of two (k <= 36: normal numbers throughout), which is what ldexpf does.
__device__ __forceinline__ float exp_neg(float x) {
    constexpr float c0 = 1.0f, c1 = -1.0f, c2 = (float)(1.0 / 2.0), c3 = (float)(-1.0 / 6.0), c4 = (float)(1.0 / 24.0),
                    c5 = (float)(-1.0 / 120.0), c6 = (float)(1.0 / 720.0), c7 = (float)(-1.0 / 5040.0), c8 = (float)(1.0 / 40320.0);
    x = fminf(x, 25.0f);
    const float k = floorf(x * 1.44269504f);
    const float r = x - k * 0.693147182f;
    float p = c8;
    p = p * r + c7; p = p * r + c6; p = p * r + c5; p = p * r + c4;
    p = p * r + c3; p = p * r + c2; p = p * r + c1; p = p * r + c0;
    const float s = __uint_as_float((uint32_t)(127 - (int)k) << 23);
    return fminf(p * s, 1.0f);
}

__device__ __forceinline__ float dist2(float ax, float ay, float az, float bx, float by, float bz) {
    const float dx = ax - bx, dy = ay - by, dz = az - bz;
    return dx * dx + dy * dy + dz * dz;          // left to right
}

// One level of the filter with step `step`: c'[P] = sum over the 5 x 5 taps Q = P + (dx, dy) * step inside the image of
// c[Q] * w(P, Q) * h[dy] h[dx], divided by the sum of the weights; w = exp_neg(|dc|^2 / sc2) exp_neg(|dn|^2 / sn2) exp_neg(|dp|^2 / sp2).
// One lane per pixel, a workgroup = a tile of 64 x 4 pixels, a wave = 64 consecutive pixels of a row, so every tap of a wave
// is one contiguous 768-byte (colour, packed float3) and two contiguous 1-KiB (G-buffer) requests straight from global
// memory.  A row's five taps are loaded together (addresses of taps outside the image are clamped to the centre and their
// results dropped); the accumulation runs in the specification's order, dy outer, dx inner, and a tap outside the image
// touches neither sum.  The kernel is bound by its arithmetic (three correctly rounded divides and three exp_neg per tap),
// not by these loads: a level costs the same at step 1 and at step 16, and with every tap reading the centre pixel it is
// 8 % faster -- which is why the taps are NOT staged in LDS.
// FIRST (level 0, step 1): `cin` is the accumulation buffer's running sum and every colour the level reads is sum / div, the
// mean sendImageToPBO shows (div = (float)iter) -- no separate pass writes the mean down.  The workgroup forms the means of
// its tile plus the halo of 2 once, in LDS (68 x 8 pixels: 6.4 divides per pixel), and the taps' colours come from there;
// 12-byte entries, so consecutive lanes are 3 banks apart and a wave's read is conflict-free.  Dividing per tap instead (78
// divides per pixel, the same quotients) measured 0.92 against 0.72 ms at 3840x2160 (profiles/denoise/ab_level0_forms.json).
// `rgba` (the last level, optional): tonemap_pixel of the result with divisor 1.
constexpr int AT_LW = 64 + 4, AT_LH = WAVES + 4;       // a workgroup's tile with the halo of a step-1 level
template <bool FIRST>
__global__ __launch_bounds__(BLOCK) void k_atrous(const float *__restrict__ cin, const float4 *__restrict__ gA,
                                                  const float4 *__restrict__ gB, float *__restrict__ cout,
                                                  uint8_t *__restrict__ rgba, int W, int H, int step, float div,
                                                  float sc2, float sn2, float sp2) {
    __shared__ float mean_lds[FIRST ? AT_LH * AT_LW * 3 : 1];
    const int tx = (int)(threadIdx.x & 63), ty = (int)(threadIdx.x >> 6);
    const int x = (int)blockIdx.x * 64 + tx;
    const int y = (int)blockIdx.y * WAVES + ty;
    if (FIRST) {                                               // (step == 1)
        const int x0 = (int)blockIdx.x * 64 - 2, y0 = (int)blockIdx.y * WAVES - 2;
        for (int i = (int)threadIdx.x; i < AT_LH * AT_LW; i += BLOCK) {
            const int ly = i / AT_LW, lx = i - ly * AT_LW;
            const int gx = x0 + lx, gy = y0 + ly;
            if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
                const size_t Q = (size_t)gy * (size_t)W + (size_t)gx;
                mean_lds[3 * i + 0] = cin[3 * Q + 0] / div; mean_lds[3 * i + 1] = cin[3 * Q + 1] / div; mean_lds[3 * i + 2] = cin[3 * Q + 2] / div;
            }
        }
        __syncthreads();
    }
    if (x >= W || y >= H) return;
    const size_t P = (size_t)y * (size_t)W + (size_t)x;
    const int Pl = (ty + 2) * AT_LW + tx + 2;                 // this pixel's entry of mean_lds
    constexpr float h[5] = {1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
    float cr, cg, cb;
    if (FIRST) { cr = mean_lds[3 * Pl + 0]; cg = mean_lds[3 * Pl + 1]; cb = mean_lds[3 * Pl + 2]; }
    else { cr = cin[3 * P + 0]; cg = cin[3 * P + 1]; cb = cin[3 * P + 2]; }
    const float4 nP = gA[P], pP = gB[P];
    float sr = 0.0f, sg = 0.0f, sb = 0.0f, cum = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        const int yy = y + dy * step;
        if (yy < 0 || yy >= H) continue;                       // (the same for the whole wave)
        const size_t row = (size_t)yy * (size_t)W;
        float qr[5], qg[5], qb[5];
        float4 qn[5], qp[5];
        bool in[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const int xx = x + (k - 2) * step;
            in[k] = xx >= 0 && xx < W;
            const size_t Q = in[k] ? row + (size_t)xx : P;
            if (FIRST) {
                const int Ql = in[k] ? Pl + dy * AT_LW + (k - 2) : Pl;
                qr[k] = mean_lds[3 * Ql + 0]; qg[k] = mean_lds[3 * Ql + 1]; qb[k] = mean_lds[3 * Ql + 2];
            } else {
                qr[k] = cin[3 * Q + 0]; qg[k] = cin[3 * Q + 1]; qb[k] = cin[3 * Q + 2];
            }
            qn[k] = gA[Q]; qp[k] = gB[Q];
        }
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            if (!in[k]) continue;
            const float r = qr[k], g = qg[k], b = qb[k];
            const float w = exp_neg(dist2(cr, cg, cb, r, g, b) / sc2) * exp_neg(dist2(nP.x, nP.y, nP.z, qn[k].x, qn[k].y, qn[k].z) / sn2) *
                            exp_neg(dist2(pP.x, pP.y, pP.z, qp[k].x, qp[k].y, qp[k].z) / sp2);
            const float wt = w * (h[dy + 2] * h[k]);
            sr = sr + r * wt; sg = sg + g * wt; sb = sb + b * wt;
            cum = cum + wt;
        }
    }
    const float outr = sr / cum, outg = sg / cum, outb = sb / cum;      // cum >= 9/64: the centre tap has w = 1
    cout[3 * P + 0] = outr; cout[3 * P + 1] = outg; cout[3 * P + 2] = outb;
    if (rgba) reinterpret_cast<uchar4 *>(rgba)[P] = tonemap_pixel(outr, outg, outb, 1);
}

// levels = 0: the result is the mean itself
__global__ __launch_bounds__(BLOCK) void k_denoise_mean(const float *__restrict__ image, float *__restrict__ cout,
                                                        uint8_t *__restrict__ rgba, uint32_t npix, float div) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= npix) return;
    const float r = image[3 * (size_t)i + 0] / div, g = image[3 * (size_t)i + 1] / div, b = image[3 * (size_t)i + 2] / div;
    cout[3 * (size_t)i + 0] = r; cout[3 * (size_t)i + 1] = g; cout[3 * (size_t)i + 2] = b;
    if (rgba) reinterpret_cast<uchar4 *>(rgba)[i] = tonemap_pixel(r, g, b, 1);
}

}  // namespace
