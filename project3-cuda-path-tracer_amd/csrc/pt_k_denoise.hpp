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
// ALB (pt_set_denoise_albedo / pt_albedo): the same launch also writes the albedo plane the filter
// demodulates by, gC[pixel] = {a.r, a.g, a.b} -- PACKED float3 like every colour plane k_atrous reads (12 bytes per pixel
// where a float4 would move 16, and the staging loop of k_atrous reads it beside the running sum with the same index).
// A miss and a specular hit (the shader's own tests: hasReflective > 0, hasRefractive > 0) give 1; every other hit the
// colour the shader puts where material.color stands -- ptd::texture_mcol called as tile_shade<.., SH_TEX> calls it while
// the session launches its textured kernels (alb.tab != nullptr), plain material.color otherwise, no gather -- clamped per
// component to [2^-6, 2^6] (fmaxf first: a NaN gives 2^-6).  The instantiations without ALB do not touch `alb`.
constexpr float ALB_MIN = 0.015625f, ALB_MAX = 64.0f;
struct GbAlbedo { float *plane; const int2 *tab; const float4 *tex; };
__device__ __forceinline__ float albedo_clamp(float v) { return fminf(fmaxf(v, ALB_MIN), ALB_MAX); }
template <int MESH, bool SLDS, bool ALB = false>
__global__ __launch_bounds__(BLOCK, MESH == MESH_TILES ? 2 : PT_MIN_WAVES) void k_gbuffer(float4 *__restrict__ gA, float4 *__restrict__ gB, SceneDev sc,
                                                                  pt_camera cam, TileMap map, GbAlbedo alb) {
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
            float t; f3 nrm; int mat, outside, geom = -1;
            if constexpr (ALB) tile_result(q, 0, acc, sc.tris, mb, t, nrm, mat, outside, geom);
            else tile_result(q, 0, acc, sc.tris, mb, t, nrm, mat, outside);
            float4 a = make_float4(0.0f, 0.0f, 0.0f, -1.0f), b = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(-1));
            if (t > 0.0f) {
                // position = origin + direction * t, per component one multiply then one add (not getPointOnRay)
                a = make_float4(nrm.x, nrm.y, nrm.z, t);
                b = make_float4(ro.x + rd.x * t, ro.y + rd.y * t, ro.z + rd.z * t, __int_as_float(mat));
            }
            gA[j] = a; gB[j] = b;
            if constexpr (ALB) {
                f3 v = ptd::mk(1.0f, 1.0f, 1.0f);
                if (t > 0.0f) {
                    const float *m = acc.mats + mat * ptd::MAT_WORDS;
                    if (!(m[6] > 0.0f) && !(m[7] > 0.0f)) {
                        if (alb.tab != nullptr)
                            v = ptd::texture_mcol(acc.mats, mat, acc.ginfo[geom] >> 28, acc.grec + (size_t)geom * GREC_WORDS, ro, rd, t,
                                                  alb.tab, alb.tex);
                        else
                            v = ptd::mk(m[0], m[1], m[2]);
                        v = ptd::mk(albedo_clamp(v.x), albedo_clamp(v.y), albedo_clamp(v.z));
                    }
                }
                alb.plane[3 * (size_t)j + 0] = v.x; alb.plane[3 * (size_t)j + 1] = v.y; alb.plane[3 * (size_t)j + 2] = v.z;
            }
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
// DM (pt_set_denoise_albedo), two independent bits, `alb` = the albedo plane A (packed float3):
//   AT_DIV (FIRST only): the staging loop also loads A[Q] and stores (cin[Q] / div) / A[Q] -- 12 more bytes and 3 more
//     divides per staged pixel, the taps unchanged.  A temporal call's blended plane comes through here with div = 1.0f
//     (x / 1.0f = x exactly) instead of the per-tap loads of k_atrous<false>: dividing per tap would be 78 divides per pixel.
//   AT_MUL (the last level): out = (s / cum) * A[P], and `rgba` from that.
// DM = 0 does not touch `alb`: the two instantiations of a session without the switch.
constexpr int AT_LW = 64 + 4, AT_LH = WAVES + 4;       // a workgroup's tile with the halo of a step-1 level
constexpr int AT_DIV = 1, AT_MUL = 2;
template <bool FIRST, int DM = 0>
__global__ __launch_bounds__(BLOCK) void k_atrous(const float *__restrict__ cin, const float4 *__restrict__ gA,
                                                  const float4 *__restrict__ gB, float *__restrict__ cout,
                                                  uint8_t *__restrict__ rgba, int W, int H, int step, float div,
                                                  float sc2, float sn2, float sp2, const float *__restrict__ alb) {
    static_assert(FIRST || !(DM & AT_DIV), "the divide on load belongs to the staged form");
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
                if constexpr ((DM & AT_DIV) != 0) {
                    const float sr0 = cin[3 * Q + 0], sg0 = cin[3 * Q + 1], sb0 = cin[3 * Q + 2];
                    const float ar = alb[3 * Q + 0], ag = alb[3 * Q + 1], ab = alb[3 * Q + 2];
                    mean_lds[3 * i + 0] = (sr0 / div) / ar; mean_lds[3 * i + 1] = (sg0 / div) / ag; mean_lds[3 * i + 2] = (sb0 / div) / ab;
                } else {
                    mean_lds[3 * i + 0] = cin[3 * Q + 0] / div; mean_lds[3 * i + 1] = cin[3 * Q + 1] / div; mean_lds[3 * i + 2] = cin[3 * Q + 2] / div;
                }
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
    float outr = sr / cum, outg = sg / cum, outb = sb / cum;            // cum >= 9/64: the centre tap has w = 1
    if constexpr ((DM & AT_MUL) != 0) { outr = outr * alb[3 * P + 0]; outg = outg * alb[3 * P + 1]; outb = outb * alb[3 * P + 2]; }
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

// ---- the filter steered by the pixels' own noise (pt_denoise_variance) ------------------------------
// k_atrous's geometry -- one lane per pixel, a workgroup = 64 x 4 pixels, a wave = 64 consecutive pixels of a row, a row's five
// taps loaded together -- on ping-pong planes of 16-byte records {r, g, b, var}: a tap is one aligned float4 load beside the two
// G-buffer records, and the variance of the mean travels through the levels with the colour (var' = sum var[Q] wt^2 / cum^2).
// The colour stop is |L[P] - L[Q]| / den[P], L = luminance of the record's colour, den = sl * sqrt(max(gv, 2^-40)) with gv the
// 3 x 3 Gaussian {1/4, 1/2, 1/4}^2 of var around P, coordinates clamped to the image: nine scalar loads per pixel, once.
// sl is NOT halved per level.  The root is the kernels' own (ptd::sqrt_normal_range: correctly rounded on [2^-102, 2^128),
// and the floor keeps its argument inside).
// FIRST (level 0, step 1): the workgroup forms c_0 = sum / div and var_0 = fmaxf(M2 / div - mu * mu, 0) / vdiv, mu = M1 / div
// (vdiv = fmaxf(div - 1, 1), formed by the host), for its tile plus the halo of 2 once, in LDS, as k_atrous<true> forms its
// means; taps and the prefilter's nine values come from there (the clamped neighbours of a pixel inside the image are inside
// the image and within the halo), and var_0 of the own pixel goes to `var0` (pt_variance).  16-byte entries: a ds_read_b128 of 16
// consecutive lanes covers the 64 banks once.
// `out3` (the last level): the result as the packed float3 plane pt_denoised_device_image returns, and `rgba` from it
// (optional); the levels before write `cout`.
constexpr float VAR_FLOOR = 9.094947017729282e-13f;         // 2^-40
__device__ __forceinline__ float var_of_mean(float m1, float m2, float div, float vdiv) {
    const float mu = m1 / div;
    return fmaxf(m2 / div - mu * mu, 0.0f) / vdiv;
}
template <bool FIRST>
__global__ __launch_bounds__(BLOCK) void k_atrous_var(const float *__restrict__ sum, const float *__restrict__ m1,
                                                      const float *__restrict__ m2, const float4 *__restrict__ cin,
                                                      const float4 *__restrict__ gA, const float4 *__restrict__ gB,
                                                      float4 *__restrict__ cout, float *__restrict__ var0, float *__restrict__ out3,
                                                      uint8_t *__restrict__ rgba, int W, int H, int step, float div, float vdiv,
                                                      float sl, float sn2, float sp2) {
    __shared__ float4 tile_lds[FIRST ? AT_LH * AT_LW : 1];
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
                tile_lds[i] = make_float4(sum[3 * Q + 0] / div, sum[3 * Q + 1] / div, sum[3 * Q + 2] / div, var_of_mean(m1[Q], m2[Q], div, vdiv));
            }
        }
        __syncthreads();
    }
    if (x >= W || y >= H) return;
    const size_t P = (size_t)y * (size_t)W + (size_t)x;
    const int Pl = (ty + 2) * AT_LW + tx + 2;                 // this pixel's entry of tile_lds
    constexpr float h[5] = {1.0f / 16.0f, 1.0f / 4.0f, 3.0f / 8.0f, 1.0f / 4.0f, 1.0f / 16.0f};
    constexpr float g3[3] = {1.0f / 4.0f, 1.0f / 2.0f, 1.0f / 4.0f};
    const float4 cP = FIRST ? tile_lds[Pl] : cin[P];
    // the 3 x 3 Gaussian of the variance around P: clamped coordinates, none skipped, dy outer
    float pv[9];
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
        const int yy = min(max(y + dy, 0), H - 1);
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const int xx = min(max(x + dx, 0), W - 1);
            if (FIRST) pv[(dy + 1) * 3 + dx + 1] = tile_lds[Pl + (yy - y) * AT_LW + (xx - x)].w;
            else pv[(dy + 1) * 3 + dx + 1] = cin[(size_t)yy * (size_t)W + (size_t)xx].w;
        }
    }
    float gv = 0.0f;
#pragma unroll
    for (int k = 0; k < 9; ++k) gv = gv + pv[k] * (g3[k / 3] * g3[k % 3]);
    const float den = sl * ptd::sqrt_normal_range(fmaxf(gv, VAR_FLOOR));
    const float LP = luminance(cP.x, cP.y, cP.z);
    const float4 nP = gA[P], pP = gB[P];
    float sr = 0.0f, sg = 0.0f, sb = 0.0f, sv = 0.0f, cum = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        const int yy = y + dy * step;
        if (yy < 0 || yy >= H) continue;                       // (the same for the whole wave)
        const size_t row = (size_t)yy * (size_t)W;
        float4 qc[5], qn[5], qp[5];
        bool in[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const int xx = x + (k - 2) * step;
            in[k] = xx >= 0 && xx < W;
            const size_t Q = in[k] ? row + (size_t)xx : P;
            if (FIRST) qc[k] = tile_lds[in[k] ? Pl + dy * AT_LW + (k - 2) : Pl];
            else qc[k] = cin[Q];
            qn[k] = gA[Q]; qp[k] = gB[Q];
        }
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            if (!in[k]) continue;
            const float4 q = qc[k];
            const float w = exp_neg(fabsf(LP - luminance(q.x, q.y, q.z)) / den) *
                            exp_neg(dist2(nP.x, nP.y, nP.z, qn[k].x, qn[k].y, qn[k].z) / sn2) *
                            exp_neg(dist2(pP.x, pP.y, pP.z, qp[k].x, qp[k].y, qp[k].z) / sp2);
            const float wt = w * (h[dy + 2] * h[k]);
            sr = sr + q.x * wt; sg = sg + q.y * wt; sb = sb + q.z * wt;
            sv = sv + q.w * (wt * wt);
            cum = cum + wt;
        }
    }
    const float outr = sr / cum, outg = sg / cum, outb = sb / cum;      // cum >= 9/64: the centre tap has w = 1
    if (FIRST) var0[P] = cP.w;
    if (out3) {
        out3[3 * P + 0] = outr; out3[3 * P + 1] = outg; out3[3 * P + 2] = outb;
        if (rgba) reinterpret_cast<uchar4 *>(rgba)[P] = tonemap_pixel(outr, outg, outb, 1);
    } else {
        cout[P] = make_float4(outr, outg, outb, sv / (cum * cum));
    }
}

// levels = 0: the result is the mean itself, and var_0 beside it
__global__ __launch_bounds__(BLOCK) void k_variance_mean(const float *__restrict__ sum, const float *__restrict__ m1,
                                                         const float *__restrict__ m2, float *__restrict__ out3,
                                                         float *__restrict__ var0, uint8_t *__restrict__ rgba, uint32_t npix,
                                                         float div, float vdiv) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= npix) return;
    const float r = sum[3 * (size_t)i + 0] / div, g = sum[3 * (size_t)i + 1] / div, b = sum[3 * (size_t)i + 2] / div;
    out3[3 * (size_t)i + 0] = r; out3[3 * (size_t)i + 1] = g; out3[3 * (size_t)i + 2] = b;
    var0[i] = var_of_mean(m1[i], m2[i], div, vdiv);
    if (rgba) reinterpret_cast<uchar4 *>(rgba)[i] = tonemap_pixel(r, g, b, 1);
}

// ---- history across camera moves (pt_denoise_temporal) -------------------------------------------
// Reprojection: for pixel P of the NEW camera's grid (its G-buffer gA / gB), the pixel Q of the OLD camera `A` that saw the
// same surface point -- the inverse of generateRayFromCamera, nearest pixel -- and, when Q's first hit is that point (same
// material, position within ptol * t, normal within ntol: ntol2 = ntol * ntol), the old view's colour and sample count
// (capped) as P's history; Hc = Hn = 0 otherwise.  Specular first hits carry none (what they show depends on the view):
// the material's hasReflective / hasRefractive words of the scene's staged records.  One lane per pixel, a wave = 64
// consecutive pixels of a row (k_atrous's layout): the own records are two contiguous 1-KiB requests, the gather at Q is
// 32 + 12 + 4 bytes per lane, issued together before any of the tests reads them.  Neighbouring lanes land on neighbouring
// Q wherever the surface is smooth.  Every Q is inside the old grid by the test on fx / fy; a material index outside the
// table reads nothing.
__global__ __launch_bounds__(BLOCK) void k_reproject(const float4 *__restrict__ gA, const float4 *__restrict__ gB,
                                                     const float4 *__restrict__ oA, const float4 *__restrict__ oB,
                                                     const float *__restrict__ oC, const float *__restrict__ oN,
                                                     const float *__restrict__ mats, int nmats, pt_camera A,
                                                     float *__restrict__ Hc, float *__restrict__ Hn, int W, int H, float cap,
                                                     float ptol, float ntol2) {
    const int x = (int)blockIdx.x * 64 + (int)(threadIdx.x & 63);
    const int y = (int)blockIdx.y * WAVES + (int)(threadIdx.x >> 6);
    if (x >= W || y >= H) return;
    const size_t P = (size_t)y * (size_t)W + (size_t)x;
    const float4 n = gA[P], p = gB[P];
    const int mat = __float_as_int(p.w);
    float hr = 0.0f, hg = 0.0f, hb = 0.0f, hn = 0.0f;
    bool ok = mat >= 0 && mat < nmats;
    if (ok) ok = mats[(size_t)mat * ptd::MAT_WORDS + 6] == 0.0f && mats[(size_t)mat * ptd::MAT_WORDS + 7] == 0.0f;
    if (ok) {
        const float vx = p.x - A.position.x, vy = p.y - A.position.y, vz = p.z - A.position.z;
        const float z = vx * A.view.x + vy * A.view.y + vz * A.view.z;
        if (z > 0.0f) {
            const float xs = (float)W * 0.5f - (vx * A.right.x + vy * A.right.y + vz * A.right.z) / (z * A.pixelLength[0]);
            const float ys = (float)H * 0.5f - (vx * A.up.x + vy * A.up.y + vz * A.up.z) / (z * A.pixelLength[1]);
            const float fx = floorf(xs + 0.5f), fy = floorf(ys + 0.5f);
            if (fx >= 0.0f && fx < (float)W && fy >= 0.0f && fy < (float)H) {          // (false on NaN)
                const size_t Q = (size_t)((int)fy * W + (int)fx);
                const float4 qn = oA[Q], qp = oB[Q];
                const float qr = oC[3 * Q + 0], qg = oC[3 * Q + 1], qb = oC[3 * Q + 2], qlen = oN[Q];
                const float lim = ptol * n.w;
                if (__float_as_int(qp.w) == mat && dist2(qp.x, qp.y, qp.z, p.x, p.y, p.z) <= lim * lim &&
                    dist2(qn.x, qn.y, qn.z, n.x, n.y, n.z) <= ntol2) {
                    hr = qr; hg = qg; hb = qb;
                    hn = fminf(qlen, cap);
                }
            }
        }
    }
    Hc[3 * P + 0] = hr; Hc[3 * P + 1] = hg; Hc[3 * P + 2] = hb;
    Hn[P] = hn;
}

// The blend: c0 = (sum + Hc * Hn) / (div + Hn) per channel, N = div + Hn (div = (float)iter) -- with Hn = 0 the mean
// pt_denoise filters.  Streaming: a lane takes four consecutive pixels, 48 bytes of each packed-float3 plane as three
// 16-byte accesses and the lengths as one (VEC: every plane is 16-byte aligned, which the library's own allocations are;
// a caller's accumulation buffer may not be); the pixels after the last whole group of four go one per lane.
// `rgba` (levels = 0, optional): tonemap_pixel of c0 with divisor 1.
__device__ __forceinline__ float blend1(float s, float hc, float hn, float den) { return (s + hc * hn) / den; }
template <bool VEC>
__global__ __launch_bounds__(BLOCK) void k_temporal_blend(const float *__restrict__ sum, const float *__restrict__ Hc,
                                                          const float *__restrict__ Hn, float *__restrict__ Cout,
                                                          float *__restrict__ Nout, uint8_t *__restrict__ rgba, uint32_t npix,
                                                          float div) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    const uint32_t groups = VEC ? npix / 4 : 0;
    if (VEC && i < groups) {
        const float4 *s4 = reinterpret_cast<const float4 *>(sum) + 3 * (size_t)i;
        const float4 *h4 = reinterpret_cast<const float4 *>(Hc) + 3 * (size_t)i;
        const float4 s0 = s4[0], s1 = s4[1], s2 = s4[2], h0 = h4[0], h1 = h4[1], h2 = h4[2];
        const float4 l = reinterpret_cast<const float4 *>(Hn)[i];
        const float4 d = make_float4(div + l.x, div + l.y, div + l.z, div + l.w);
        // floats 0..11 of the group: pixel 0 = 0 1 2, pixel 1 = 3 4 5, pixel 2 = 6 7 8, pixel 3 = 9 10 11
        const float4 c0 = make_float4(blend1(s0.x, h0.x, l.x, d.x), blend1(s0.y, h0.y, l.x, d.x), blend1(s0.z, h0.z, l.x, d.x),
                                      blend1(s0.w, h0.w, l.y, d.y));
        const float4 c1 = make_float4(blend1(s1.x, h1.x, l.y, d.y), blend1(s1.y, h1.y, l.y, d.y), blend1(s1.z, h1.z, l.z, d.z),
                                      blend1(s1.w, h1.w, l.z, d.z));
        const float4 c2 = make_float4(blend1(s2.x, h2.x, l.z, d.z), blend1(s2.y, h2.y, l.w, d.w), blend1(s2.z, h2.z, l.w, d.w),
                                      blend1(s2.w, h2.w, l.w, d.w));
        float4 *o4 = reinterpret_cast<float4 *>(Cout) + 3 * (size_t)i;
        o4[0] = c0; o4[1] = c1; o4[2] = c2;
        reinterpret_cast<float4 *>(Nout)[i] = d;
        if (rgba) {
            uchar4 *px = reinterpret_cast<uchar4 *>(rgba) + 4 * (size_t)i;
            px[0] = tonemap_pixel(c0.x, c0.y, c0.z, 1); px[1] = tonemap_pixel(c0.w, c1.x, c1.y, 1);
            px[2] = tonemap_pixel(c1.z, c1.w, c2.x, 1); px[3] = tonemap_pixel(c2.y, c2.z, c2.w, 1);
        }
        return;
    }
    // one pixel per lane: everything (not VEC), or the npix % 4 pixels after the groups (the lanes right behind them)
    const uint32_t P = VEC ? groups * 4 + (i - groups) : i;
    if (P >= npix) return;
    const float l = Hn[P], d = div + l;
    const float r = blend1(sum[3 * (size_t)P + 0], Hc[3 * (size_t)P + 0], l, d), g = blend1(sum[3 * (size_t)P + 1], Hc[3 * (size_t)P + 1], l, d),
                b = blend1(sum[3 * (size_t)P + 2], Hc[3 * (size_t)P + 2], l, d);
    Cout[3 * (size_t)P + 0] = r; Cout[3 * (size_t)P + 1] = g; Cout[3 * (size_t)P + 2] = b;
    Nout[P] = d;
    if (rgba) reinterpret_cast<uchar4 *>(rgba)[P] = tonemap_pixel(r, g, b, 1);
}

// ---- reprojected moments and the spatial variance estimate (pt_denoise_svgf) ------------------------
// k_reproject's tests, in its order, with the wider gather at Q: the two G-buffer records, the colour, the two normalised moments
// u1 = M1 / N, u2 = M2 / N and the sample count of the old view -- 32 + 12 + 4 + 4 + 4 bytes per lane, issued as one group before
// any test reads them.  The same layout (one lane per pixel, a wave = 64 consecutive pixels of a row), the same bounds: every Q is
// inside the old grid by the test on fx / fy, a material index outside the table reads nothing.
__global__ __launch_bounds__(BLOCK) void k_reproject_svgf(const float4 *__restrict__ gA, const float4 *__restrict__ gB,
                                                          const float4 *__restrict__ oA, const float4 *__restrict__ oB,
                                                          const float *__restrict__ oC, const float *__restrict__ oU1,
                                                          const float *__restrict__ oU2, const float *__restrict__ oN,
                                                          const float *__restrict__ mats, int nmats, pt_camera A,
                                                          float *__restrict__ Hc, float *__restrict__ H1, float *__restrict__ H2,
                                                          float *__restrict__ Hn, int W, int H, float cap, float ptol, float ntol2) {
    const int x = (int)blockIdx.x * 64 + (int)(threadIdx.x & 63);
    const int y = (int)blockIdx.y * WAVES + (int)(threadIdx.x >> 6);
    if (x >= W || y >= H) return;
    const size_t P = (size_t)y * (size_t)W + (size_t)x;
    const float4 n = gA[P], p = gB[P];
    const int mat = __float_as_int(p.w);
    float hr = 0.0f, hg = 0.0f, hb = 0.0f, h1 = 0.0f, h2 = 0.0f, hn = 0.0f;
    bool ok = mat >= 0 && mat < nmats;
    if (ok) ok = mats[(size_t)mat * ptd::MAT_WORDS + 6] == 0.0f && mats[(size_t)mat * ptd::MAT_WORDS + 7] == 0.0f;
    if (ok) {
        const float vx = p.x - A.position.x, vy = p.y - A.position.y, vz = p.z - A.position.z;
        const float z = vx * A.view.x + vy * A.view.y + vz * A.view.z;
        if (z > 0.0f) {
            const float xs = (float)W * 0.5f - (vx * A.right.x + vy * A.right.y + vz * A.right.z) / (z * A.pixelLength[0]);
            const float ys = (float)H * 0.5f - (vx * A.up.x + vy * A.up.y + vz * A.up.z) / (z * A.pixelLength[1]);
            const float fx = floorf(xs + 0.5f), fy = floorf(ys + 0.5f);
            if (fx >= 0.0f && fx < (float)W && fy >= 0.0f && fy < (float)H) {          // (false on NaN)
                const size_t Q = (size_t)((int)fy * W + (int)fx);
                const float4 qn = oA[Q], qp = oB[Q];
                const float qr = oC[3 * Q + 0], qg = oC[3 * Q + 1], qb = oC[3 * Q + 2];
                const float q1 = oU1[Q], q2 = oU2[Q], qlen = oN[Q];
                const float lim = ptol * n.w;
                if (__float_as_int(qp.w) == mat && dist2(qp.x, qp.y, qp.z, p.x, p.y, p.z) <= lim * lim &&
                    dist2(qn.x, qn.y, qn.z, n.x, n.y, n.z) <= ntol2) {
                    hr = qr; hg = qg; hb = qb;
                    h1 = q1; h2 = q2;
                    hn = fminf(qlen, cap);
                }
            }
        }
    }
    Hc[3 * P + 0] = hr; Hc[3 * P + 1] = hg; Hc[3 * P + 2] = hb;
    H1[P] = h1; H2[P] = h2;
    Hn[P] = hn;
}

// The blend of colour and moments: N' = div + Hn, c0 = (sum + Hc * Hn) / N' per channel (k_temporal_blend's expression), u1 = (M1 +
// H1 * Hn) / N', u2 = (M2 + H2 * Hn) / N', vt = fmaxf(u2 - u1 * u1, 0) / fmaxf(N' - 1, 1).  Streaming, 44 bytes in and 44 out per
// pixel: C / U1 / U2 / N (the next camera's history), the record {c0, vt} k_atrous_var<false> reads as `cin`, and vt once more in
// the var_0 plane (pt_svgf_variance; k_svgf_spatial replaces it where a pixel's history is short).  VEC: a lane takes four
// consecutive pixels, the packed-float3 planes as three 16-byte accesses and the scalar planes as one (every plane 16-byte aligned:
// the library's own allocations are, a caller's accumulation buffer and the second moment plane of a frame whose pixel count is no
// multiple of 4 may not be); the pixels after the last whole group of four go one per lane.
// `rgba` (levels = 0, optional): tonemap_pixel of c0 with divisor 1.
struct SvgfBlend {
    const float *sum, *m1, *m2, *Hc, *H1, *H2, *Hn;
    float *C, *U1, *U2, *N, *var0;
    float4 *rec;
    uint8_t *rgba;
};
__device__ __forceinline__ float svgf_vt(float u1, float u2, float nn) { return fmaxf(u2 - u1 * u1, 0.0f) / fmaxf(nn - 1.0f, 1.0f); }
template <bool VEC>
__global__ __launch_bounds__(BLOCK) void k_svgf_blend(SvgfBlend a, uint32_t npix, float div) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    const uint32_t groups = VEC ? npix / 4 : 0;
    if (VEC && i < groups) {
        const float4 *s4 = reinterpret_cast<const float4 *>(a.sum) + 3 * (size_t)i;
        const float4 *h4 = reinterpret_cast<const float4 *>(a.Hc) + 3 * (size_t)i;
        const float4 s0 = s4[0], s1 = s4[1], s2 = s4[2], h0 = h4[0], h1 = h4[1], h2 = h4[2];
        const float4 l4 = reinterpret_cast<const float4 *>(a.Hn)[i];
        const float4 m14 = reinterpret_cast<const float4 *>(a.m1)[i], m24 = reinterpret_cast<const float4 *>(a.m2)[i];
        const float4 g14 = reinterpret_cast<const float4 *>(a.H1)[i], g24 = reinterpret_cast<const float4 *>(a.H2)[i];
        const float s[12] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w, s2.x, s2.y, s2.z, s2.w};
        const float hc[12] = {h0.x, h0.y, h0.z, h0.w, h1.x, h1.y, h1.z, h1.w, h2.x, h2.y, h2.z, h2.w};
        const float l[4] = {l4.x, l4.y, l4.z, l4.w};
        const float m1[4] = {m14.x, m14.y, m14.z, m14.w}, m2[4] = {m24.x, m24.y, m24.z, m24.w};
        const float g1[4] = {g14.x, g14.y, g14.z, g14.w}, g2[4] = {g24.x, g24.y, g24.z, g24.w};
        float c[12], d[4], u1[4], u2[4], vt[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            d[k] = div + l[k];
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) c[3 * k + ch] = blend1(s[3 * k + ch], hc[3 * k + ch], l[k], d[k]);
            u1[k] = blend1(m1[k], g1[k], l[k], d[k]);
            u2[k] = blend1(m2[k], g2[k], l[k], d[k]);
            vt[k] = svgf_vt(u1[k], u2[k], d[k]);
        }
        float4 *o4 = reinterpret_cast<float4 *>(a.C) + 3 * (size_t)i;
        o4[0] = make_float4(c[0], c[1], c[2], c[3]); o4[1] = make_float4(c[4], c[5], c[6], c[7]); o4[2] = make_float4(c[8], c[9], c[10], c[11]);
        reinterpret_cast<float4 *>(a.U1)[i] = make_float4(u1[0], u1[1], u1[2], u1[3]);
        reinterpret_cast<float4 *>(a.U2)[i] = make_float4(u2[0], u2[1], u2[2], u2[3]);
        reinterpret_cast<float4 *>(a.N)[i] = make_float4(d[0], d[1], d[2], d[3]);
        reinterpret_cast<float4 *>(a.var0)[i] = make_float4(vt[0], vt[1], vt[2], vt[3]);
#pragma unroll
        for (int k = 0; k < 4; ++k) a.rec[4 * (size_t)i + k] = make_float4(c[3 * k + 0], c[3 * k + 1], c[3 * k + 2], vt[k]);
        if (a.rgba) {
            uchar4 *px = reinterpret_cast<uchar4 *>(a.rgba) + 4 * (size_t)i;
#pragma unroll
            for (int k = 0; k < 4; ++k) px[k] = tonemap_pixel(c[3 * k + 0], c[3 * k + 1], c[3 * k + 2], 1);
        }
        return;
    }
    // one pixel per lane: everything (not VEC), or the npix % 4 pixels after the groups (the lanes right behind them)
    const uint32_t P = VEC ? groups * 4 + (i - groups) : i;
    if (P >= npix) return;
    const float l = a.Hn[P], d = div + l;
    const float r = blend1(a.sum[3 * (size_t)P + 0], a.Hc[3 * (size_t)P + 0], l, d), g = blend1(a.sum[3 * (size_t)P + 1], a.Hc[3 * (size_t)P + 1], l, d),
                b = blend1(a.sum[3 * (size_t)P + 2], a.Hc[3 * (size_t)P + 2], l, d);
    const float u1 = blend1(a.m1[P], a.H1[P], l, d), u2 = blend1(a.m2[P], a.H2[P], l, d);
    const float vt = svgf_vt(u1, u2, d);
    a.C[3 * (size_t)P + 0] = r; a.C[3 * (size_t)P + 1] = g; a.C[3 * (size_t)P + 2] = b;
    a.U1[P] = u1; a.U2[P] = u2; a.N[P] = d; a.var0[P] = vt;
    a.rec[P] = make_float4(r, g, b, vt);
    if (a.rgba) reinterpret_cast<uchar4 *>(a.rgba)[P] = tonemap_pixel(r, g, b, 1);
}

// The spatial estimate for pixels whose history is short (N' < below): over the 7 x 7 taps Q around P inside the image, dy outer,
// w = exp_neg(|dn|^2 / sn2) * exp_neg(|dp|^2 / sp2), s1 += u1[Q] * w, s2 += u2[Q] * w, cum += w; var_0 = fmaxf(s2 / cum - (s1 /
// cum)^2, 0) / N'[P] (the centre tap has w = 1: cum >= 1).  k_atrous's geometry.  Each wave first says whether any of its lanes is
// short; a workgroup with no such wave leaves before it loads anything, and in the others a wave without one leaves after the staging
// and before its first tap (both branches are wave-uniform) -- after a camera move only disoccluded regions, mirrors and glass take
// the loop.  The workgroup stages its tile plus the halo of 3 in LDS, 70 x 10 entries of two float4, {normal, u1} and {position,
// u2} (the records' t and material are not needed): 22400 bytes, and a ds_read_b128 of 16 consecutive lanes covers the 64 banks
// once.  A short pixel's estimate replaces .w of its own record and its entry of the var_0 plane; nothing else is written.
constexpr int SV_R = 3, SV_LW = 64 + 2 * SV_R, SV_LH = WAVES + 2 * SV_R;
__global__ __launch_bounds__(BLOCK) void k_svgf_spatial(const float *__restrict__ U1, const float *__restrict__ U2,
                                                        const float *__restrict__ N, const float4 *__restrict__ gA,
                                                        const float4 *__restrict__ gB, float4 *__restrict__ rec,
                                                        float *__restrict__ var0, int W, int H, float below, float sn2, float sp2) {
    __shared__ float4 nrm_lds[SV_LH * SV_LW], pos_lds[SV_LH * SV_LW];
    __shared__ int wave_short[WAVES];
    const int tx = (int)(threadIdx.x & 63), ty = (int)(threadIdx.x >> 6);
    const int x = (int)blockIdx.x * 64 + tx;
    const int y = (int)blockIdx.y * WAVES + ty;
    const bool inside = x < W && y < H;
    const size_t P = inside ? (size_t)y * (size_t)W + (size_t)x : 0;
    const float nn = inside ? N[P] : 0.0f;
    const bool low = inside && nn < below;
    const bool wave_low = __ballot(low) != 0ull;
    if (tx == 0) wave_short[ty] = wave_low ? 1 : 0;
    __syncthreads();
    bool any = false;
#pragma unroll
    for (int k = 0; k < WAVES; ++k) any = any || wave_short[k] != 0;
    if (!any) return;                                          // (the same for the whole workgroup)
    const int x0 = (int)blockIdx.x * 64 - SV_R, y0 = (int)blockIdx.y * WAVES - SV_R;
    for (int i = (int)threadIdx.x; i < SV_LH * SV_LW; i += BLOCK) {
        const int ly = i / SV_LW, lx = i - ly * SV_LW;
        const int gx = x0 + lx, gy = y0 + ly;
        if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
            const size_t Q = (size_t)gy * (size_t)W + (size_t)gx;
            const float4 qn = gA[Q], qp = gB[Q];
            nrm_lds[i] = make_float4(qn.x, qn.y, qn.z, U1[Q]);
            pos_lds[i] = make_float4(qp.x, qp.y, qp.z, U2[Q]);
        }
    }
    __syncthreads();
    if (!wave_low) return;                                     // (the same for the whole wave)
    if (!low) return;
    const int Pl = (ty + SV_R) * SV_LW + tx + SV_R;            // this pixel's entry
    const float4 nP = nrm_lds[Pl], pP = pos_lds[Pl];
    float s1 = 0.0f, s2 = 0.0f, cum = 0.0f;
#pragma unroll 1
    for (int dy = -SV_R; dy <= SV_R; ++dy) {
        const int yy = y + dy;
        if (yy < 0 || yy >= H) continue;                       // (the same for the whole wave)
#pragma unroll
        for (int dx = -SV_R; dx <= SV_R; ++dx) {
            const int xx = x + dx;
            if (xx < 0 || xx >= W) continue;
            const float4 qn = nrm_lds[Pl + dy * SV_LW + dx], qp = pos_lds[Pl + dy * SV_LW + dx];
            const float w = exp_neg(dist2(nP.x, nP.y, nP.z, qn.x, qn.y, qn.z) / sn2) * exp_neg(dist2(pP.x, pP.y, pP.z, qp.x, qp.y, qp.z) / sp2);
            s1 = s1 + qn.w * w; s2 = s2 + qp.w * w;
            cum = cum + w;
        }
    }
    const float am = s1 / cum, bm = s2 / cum;
    const float v = fmaxf(bm - am * am, 0.0f) / nn;
    rec[P].w = v;
    var0[P] = v;
}

}  // namespace
