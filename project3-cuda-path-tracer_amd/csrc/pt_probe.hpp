// pt_probe.hpp -- known-answer probes of libptmi355.so (included by ptmi355.hip only, before pt_multi.hpp): the device functions of
// pt_device.hpp that restate third-party arithmetic the reference merely calls -- thrust's minstd_rand + u01
// (pathtrace.cu:41-45, interactions.h:12-13), the sin / cos binding of interactions.h:40-41 and
// calculateRandomDirectionInHemisphere (interactions.h:10-42) -- and this project's own completion of the empty scatterRay
// (interactions.h:69-79: ptd::shade_scatter) run on caller data, so that a test can hold them against published constants,
// the reference's glm vectors and the oracle one function at a time instead of through whole images.
// No session needed: the probes run on the calling thread's current HIP device, and their entry points are the exported symbols
// themselves (global scope; include/ptmi355.h has declared them extern "C") -- pt_multi.hpp has nothing to dispatch for them.
#pragma once

namespace {

__global__ void k_probe_rng(const uint32_t *seeds, int n, int draws, uint32_t *state, float *u) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t st = ptd::lcg_seed(seeds[i]);
    float last = 0.0f;
    for (int k = 0; k < draws; ++k) last = ptd::u01(st);
    if (state) state[i] = st;
    if (u) u[i] = last;
}

__global__ void k_probe_sincos(const float *x, uint32_t first_bits, uint32_t n, float *s, float *c, unsigned long long *sum) {
    unsigned long long as = 0, ac = 0;
    // 64-bit index: n may be anything up to 2^32 - 1 (the whole binary32 range) and the stride must not wrap
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (uint64_t)gridDim.x * blockDim.x) {
        const float v = x ? x[k] : __uint_as_float(first_bits + (uint32_t)k);
        float sv, cv;
        ptd::sincos_shared(v, sv, cv);
        if (s) s[k] = sv;
        if (c) c[k] = cv;
        as += (unsigned long long)__float_as_uint(sv) * (2ull * k + 1ull);
        ac += (unsigned long long)__float_as_uint(cv) * (2ull * k + 1ull);
    }
    if (sum) { atomicAdd(&sum[0], as); atomicAdd(&sum[1], ac); }
}

__global__ void k_probe_sqrt(uint32_t first_bits, uint32_t n, unsigned long long *bad) {
    unsigned long long b0 = 0, b1 = 0;
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (uint64_t)gridDim.x * blockDim.x) {
        const float x = __uint_as_float(first_bits + (uint32_t)k);
        const float s = ptd::sqrt_normal_range(x);
        // (as normalize_unit chooses: the four-addition form inside its gate)
        const float q = (x >= ptd::NEAR_ONE_LO && x <= ptd::NEAR_ONE_HI) ? ptd::rsqrt_near_one(x) : ptd::rsqrt_of_root(x);
        const float s_ref = __builtin_sqrtf(x);                  // (hipcc: correctly rounded by default)
        const float q_ref = 1.0f / s_ref;
        b0 += __float_as_uint(s) != __float_as_uint(s_ref);
        b1 += __float_as_uint(q) != __float_as_uint(q_ref);
    }
    if (b0) atomicAdd(&bad[0], b0);
    if (b1) atomicAdd(&bad[1], b1);
}

__global__ void k_probe_hemisphere(const float *normals, const uint32_t *seeds, int n, float *dirs) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t st = ptd::lcg_seed(seeds[i]);
    const f3 d = ptd::hemisphere(ptd::mk(normals[3 * i], normals[3 * i + 1], normals[3 * i + 2]), st);
    dirs[3 * i] = d.x; dirs[3 * i + 1] = d.y; dirs[3 * i + 2] = d.z;
}

// the GGX lobe of PT_GLOSSY through the kernels' own ptd::lobe, seeded like k_probe_hemisphere
__global__ void k_probe_glossy_lobe(const float *normals, const uint32_t *seeds, const float *alpha2, int n, float *dirs) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t st = ptd::lcg_seed(seeds[i]);
    const f3 d = ptd::lobe(ptd::mk(normals[3 * i], normals[3 * i + 1], normals[3 * i + 2]), st, alpha2[i]);
    dirs[3 * i] = d.x; dirs[3 * i + 1] = d.y; dirs[3 * i + 2] = d.z;
}

// ---- what the shade-scatter probes share: one lane per (path, intersection) record, host structs as they are.  Each kernel is
// probe_load, its own call of the shader, probe_resolve_pending where that call can defer, probe_store ----
// record i into locals; false for a lane past the records and for a path that has ended (the oracle's compaction-off mode:
// untouched).  outside == nullptr: every hit is from outside
__device__ __forceinline__ bool probe_load(const pt_path_segment *paths, const pt_shadeable_intersection *isects, const uint8_t *outside, int n,
                                           int i, pt_path_segment &p, pt_shadeable_intersection &x, ptd::PathState &ps, int &out) {
    if (i >= n) return false;
    p = paths[i];
    if (p.remainingBounces <= 0) return false;
    x = isects[i];
    ps.o = ptd::mk(p.ray.origin.x, p.ray.origin.y, p.ray.origin.z);
    ps.d = ptd::mk(p.ray.direction.x, p.ray.direction.y, p.ray.direction.z);
    ps.c = ptd::mk(p.color.x, p.color.y, p.color.z);
    out = outside ? (outside[i] ? 1 : 0) : 1;
    return true;
}
// what the next bounce's load does with a pending direction (pt_k_bounce.hpp: tile_load<RESOLVE>, whose `depth - 1`
// is this bounce's depth): the same engine, the same sampler, on the normal the scatter left in the direction
__device__ __forceinline__ void probe_resolve_pending(ptd::PathState &ps, int iter, int pixel, int depth) {
    uint32_t rng = ptd::seeded_engine(iter, pixel, depth);
    ps.d = ptd::hemisphere(ps.d, rng);
}
// a path that ends keeps the ray it came with
__device__ __forceinline__ void probe_store(pt_path_segment *q, const ptd::PathState &ps, bool alive, int remaining) {
    if (alive) {
        q->ray.origin.x = ps.o.x; q->ray.origin.y = ps.o.y; q->ray.origin.z = ps.o.z;
        q->ray.direction.x = ps.d.x; q->ray.direction.y = ps.d.y; q->ray.direction.z = ps.d.z;
    }
    q->color.x = ps.c.x; q->color.y = ps.c.y; q->color.z = ps.c.z;
    q->remainingBounces = remaining;
}

// one pass of the loop body's shader (pathtrace.cu:224-266 with scatterRay completed) through the kernels'
// own ptd::shade_scatter.  defer != 0: the deferring kernels' call -- a diffuse survivor comes back with the hit normal for a
// direction and draws it afterwards, as the next bounce's load does.  GLOSSY: the form a PT_GLOSSY session's kernels call
template <bool GLOSSY>
__global__ __launch_bounds__(64) void k_probe_shade_scatter(int iter, int depth, const float *__restrict__ mats, pt_path_segment *paths,
                                                             const pt_shadeable_intersection *__restrict__ isects,
                                                             const uint8_t *__restrict__ outside, int n, int defer) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    pt_path_segment p;
    pt_shadeable_intersection x;
    ptd::PathState ps;
    int out;
    if (!probe_load(paths, isects, outside, n, i, p, x, ps, out)) return;
    bool deferred = false;
    const bool alive = ptd::shade_scatter<GLOSSY>(ps, x.t, ptd::mk(x.surfaceNormal.x, x.surfaceNormal.y, x.surfaceNormal.z), x.materialId,
                                          out, mats, iter, p.pixelIndex, depth, p.remainingBounces == 1,
                                          defer != 0, &deferred);
    if (deferred) probe_resolve_pending(ps, iter, p.pixelIndex, depth);
    probe_store(paths + i, ps, alive, alive ? p.remainingBounces - 1 : 0);
}

// PT_TEXTURES' lookup and multiply through the kernels' own ptd::texture_tint: one lane per (primitive,
// world point, colour) record; inv: 12 words per primitive (inverseTransform, 4 columns x 3 rows), type: PT_SPHERE / PT_CUBE / mesh
__global__ __launch_bounds__(64) void k_probe_texture(const float *__restrict__ inv, const int32_t *__restrict__ type, const int32_t *__restrict__ hit_geom,
                                                       const float *__restrict__ points, int count, const float4 *__restrict__ texels, int n,
                                                       const float *__restrict__ colour_in, float *__restrict__ colour_out) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= count) return;
    const int g = hit_geom[i];
    f3 c = ptd::mk(colour_in[3 * i], colour_in[3 * i + 1], colour_in[3 * i + 2]);
    if (type[g] == PT_SPHERE || type[g] == PT_CUBE)
        c = ptd::texture_tint(c, inv + (size_t)g * 12, ptd::mk(points[3 * i], points[3 * i + 1], points[3 * i + 2]), texels, n);
    colour_out[3 * i] = c.x; colour_out[3 * i + 1] = c.y; colour_out[3 * i + 2] = c.z;
}

// k_probe_shade_scatter through the textured form of the shader, as tile_shade<.., SH_TEX> calls it: mcol from ptd::texture_mcol on
// the record's primitive (hit_geom) and the texture table, then shade_scatter<false, false, true>
__global__ __launch_bounds__(64) void k_probe_shade_scatter_textured(int iter, int depth, const float *__restrict__ mats, pt_path_segment *paths,
                                                                      const pt_shadeable_intersection *__restrict__ isects,
                                                                      const uint8_t *__restrict__ outside, int n, int defer,
                                                                      const float *__restrict__ inv, const int32_t *__restrict__ type,
                                                                      const int32_t *__restrict__ hit_geom, const float4 *__restrict__ texels,
                                                                      const int2 *__restrict__ tab) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    pt_path_segment p;
    pt_shadeable_intersection x;
    ptd::PathState ps;
    int out;
    if (!probe_load(paths, isects, outside, n, i, p, x, ps, out)) return;
    bool deferred = false;
    f3 mcol = ptd::mk(0.0f, 0.0f, 0.0f);
    if (x.t > 0.0f) {
        const int g = hit_geom[i];
        mcol = ptd::texture_mcol(mats, x.materialId, (uint32_t)type[g], inv + (size_t)g * 12, ps.o, ps.d, x.t, tab, texels);
    }
    const bool alive = ptd::shade_scatter<false, false, true>(ps, x.t, ptd::mk(x.surfaceNormal.x, x.surfaceNormal.y, x.surfaceNormal.z), x.materialId,
                                                              out, mats, iter, p.pixelIndex, depth, p.remainingBounces == 1,
                                                              defer != 0, &deferred, nullptr, nullptr, 0, &mcol);
    if (deferred) probe_resolve_pending(ps, iter, p.pixelIndex, depth);
    probe_store(paths + i, ps, alive, alive ? p.remainingBounces - 1 : 0);
}

// bump mapping through the kernels' own ptd::bump_normal: one lane per (primitive, world point, reported
// normal, ray direction) record; rec: 36 words per primitive (inverseTransform, transform, invTranspose, 4 columns x 3 rows each)
__global__ __launch_bounds__(64) void k_probe_bump_normal(const float *__restrict__ rec, const int32_t *__restrict__ type, const int32_t *__restrict__ hit_geom,
                                                           const float *__restrict__ points, const float *__restrict__ normals,
                                                           const float *__restrict__ dirs, int count, const ptd::bump_texel *__restrict__ texels, int n,
                                                           float *__restrict__ out_normals, uint8_t *__restrict__ perturbed) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= count) return;
    const int g = hit_geom[i];
    float x = normals[3 * i], y = normals[3 * i + 1], z = normals[3 * i + 2];
    bool hit = false;
    if (type[g] == PT_SPHERE || type[g] == PT_CUBE)
        hit = ptd::bump_normal((uint32_t)type[g], rec + (size_t)g * 36, points[3 * i], points[3 * i + 1], points[3 * i + 2],
                               dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2], x, y, z, texels, n, x, y, z);
    out_normals[3 * i] = x; out_normals[3 * i + 1] = y; out_normals[3 * i + 2] = z;
    perturbed[i] = hit ? 1 : 0;
}

// smooth mesh normals through the kernels' own ptd::smooth_normal: one lane per (triangle, ray) record.
// rec: the device's triangle records (TRI_WORDS each: v0, e1, e2); vn: nine floats per triangle.  The reported normal is the
// facet normal tile_result computes.
__global__ __launch_bounds__(64) void k_probe_smooth_normal(const float *__restrict__ rec, const float *__restrict__ vn, const int32_t *__restrict__ tri,
                                                             const float *__restrict__ origins, const float *__restrict__ dirs, int count,
                                                             float *__restrict__ out_normals, uint8_t *__restrict__ smoothed) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= count) return;
    const float *tv = rec + (size_t)tri[i] * TRI_WORDS;
    const ptd::f3 nr = ptd::normalize(ptd::cross(ptd::mk(tv[3], tv[4], tv[5]), ptd::mk(tv[6], tv[7], tv[8])));
    float x = nr.x, y = nr.y, z = nr.z;
    const bool hit = ptd::smooth_normal(tv, vn + (size_t)tri[i] * 9, origins[3 * i], origins[3 * i + 1], origins[3 * i + 2],
                                        dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2], nr.x, nr.y, nr.z, x, y, z);
    out_normals[3 * i] = x; out_normals[3 * i + 1] = y; out_normals[3 * i + 2] = z;
    smoothed[i] = hit ? 1 : 0;
}

// k_probe_shade_scatter_textured through ptd::shade_scatter_tex, the call of tile_shade<.., SH_TEX>: lookup, shader, guard
__global__ __launch_bounds__(64) void k_probe_shade_scatter_bumped(int iter, int depth, const float *__restrict__ mats, pt_path_segment *paths,
                                                                    const pt_shadeable_intersection *__restrict__ isects,
                                                                    const uint8_t *__restrict__ outside, int n, int defer,
                                                                    const float *__restrict__ rec, const int32_t *__restrict__ type,
                                                                    const int32_t *__restrict__ hit_geom, const float4 *__restrict__ texels,
                                                                    const int2 *__restrict__ tab, const ptd::bump_texel *__restrict__ bumps,
                                                                    const int2 *__restrict__ btab) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    pt_path_segment p;
    pt_shadeable_intersection x;
    ptd::PathState ps;
    int out;
    if (!probe_load(paths, isects, outside, n, i, p, x, ps, out)) return;
    bool deferred = false;
    const int g = x.t > 0.0f ? hit_geom[i] : 0;
    const bool alive = ptd::shade_scatter_tex<false>(ps, x.t, ptd::mk(x.surfaceNormal.x, x.surfaceNormal.y, x.surfaceNormal.z), x.materialId,
                                                     out, mats, iter, p.pixelIndex, depth, p.remainingBounces == 1,
                                                     defer != 0, &deferred, nullptr, (uint32_t)type[g], rec + (size_t)g * 36, tab, texels, btab, bumps);
    if (deferred) probe_resolve_pending(ps, iter, p.pixelIndex, depth);
    probe_store(paths + i, ps, alive, alive ? p.remainingBounces - 1 : 0);
}

// PT_DIRECT_LIGHT's sampler through the kernels' own ptd::direct_sample, seeded like k_probe_hemisphere
__global__ __launch_bounds__(64) void k_probe_direct_sample(const float *__restrict__ lights, int nlights, const float *__restrict__ P,
                                                             const float *__restrict__ nrm, const uint32_t *__restrict__ seeds, int count,
                                                             float *__restrict__ dir, float *__restrict__ weight, int32_t *__restrict__ element) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= count) return;
    uint32_t st = ptd::lcg_seed(seeds[i]);
    f3 d;
    float w;
    int e;
    (void)ptd::direct_sample(lights, nlights, ptd::mk(P[3 * i], P[3 * i + 1], P[3 * i + 2]), ptd::mk(nrm[3 * i], nrm[3 * i + 1], nrm[3 * i + 2]), st, d, w, e);
    dir[3 * i] = d.x; dir[3 * i + 1] = d.y; dir[3 * i + 2] = d.z;
    weight[i] = w;
    element[i] = e;
}

// PT_DIRECT_SKY's branch of the sampler through ptd::direct_sample on a table whose only element is the
// sky: one lane per (normal, engine seed) record, P = 0 (the sky's branch does not read it)
__global__ __launch_bounds__(64) void k_probe_sky_sample(const float *__restrict__ lights, int nlights, const float *__restrict__ nrm,
                                                          const uint32_t *__restrict__ seeds, int count, float *__restrict__ dir,
                                                          float *__restrict__ weight, int32_t *__restrict__ texel) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= count) return;
    uint32_t st = ptd::lcg_seed(seeds[i]);
    f3 d;
    float w;
    int e, k = -1;
    (void)ptd::direct_sample(lights, nlights, ptd::mk(0.0f, 0.0f, 0.0f), ptd::mk(nrm[3 * i], nrm[3 * i + 1], nrm[3 * i + 2]), st, d, w, e, &k);
    dir[3 * i] = d.x; dir[3 * i + 1] = d.y; dir[3 * i + 2] = d.z;
    weight[i] = w;
    texel[i] = k;
}

// k_probe_shade_scatter through the direct form of the shader, as tile_shade<.., SH_DIRECT> calls it at bounce `depth` of a session of
// traceDepth `trace_depth`: the scatter with last_bounce = (depth == trace_depth - 1), or -- depth == trace_depth -- the final ray's
// scoring rule on the winning primitive hit_geom[i].  env_n > 0 (pt_probe_shade_scatter_direct_sky): the table may end with the
// sky's element, and a final ray aimed at it reads the map `env` where it misses
__global__ __launch_bounds__(64) void k_probe_shade_scatter_direct(int iter, int depth, int trace_depth, const float *__restrict__ mats,
                                                                    const float *__restrict__ lights, int nlights, pt_path_segment *paths,
                                                                    const pt_shadeable_intersection *__restrict__ isects,
                                                                    const uint8_t *__restrict__ outside, const int32_t *__restrict__ hit_geom, int n,
                                                                    const float4 *__restrict__ env, int env_n) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    pt_path_segment p;
    pt_shadeable_intersection x;
    ptd::PathState ps;
    int out;
    if (!probe_load(paths, isects, outside, n, i, p, x, ps, out)) return;
    bool alive = false;
    if (depth == trace_depth) {
        const int target = nlights > 0 ? ptd::direct_target(lights, nlights, iter, p.pixelIndex, depth - 1) : -2;
        if (env_n > 0 && target == -1) {                   // PT_DIRECT_SKY: a sky-aimed ray scores on a miss only (tile_shade)
            if (!(x.t > 0.0f)) ps.c = ptd::miss_colour(ps.c, ps.d, env, env_n);
            else ps.c = ptd::mk(0.0f, 0.0f, 0.0f);
        } else if (x.t > 0.0f && hit_geom[i] == target) {
            const float *m = mats + x.materialId * ptd::MAT_WORDS;
            ps.c = ptd::mul(ps.c, ptd::scale(ptd::mk(m[0], m[1], m[2]), m[9]));
        } else {
            ps.c = ptd::mk(0.0f, 0.0f, 0.0f);
        }
    } else {
        alive = ptd::shade_scatter<false, true>(ps, x.t, ptd::mk(x.surfaceNormal.x, x.surfaceNormal.y, x.surfaceNormal.z), x.materialId,
                                                out, mats, iter, p.pixelIndex, depth, depth == trace_depth - 1,
                                                false, nullptr, nullptr, lights, nlights);
    }
    probe_store(paths + i, ps, alive, alive ? trace_depth - depth : 0);
}

// the miss exit's colour through the kernels' own ptd::miss_colour: one lane per (direction, throughput) pair
__global__ __launch_bounds__(64) void k_probe_environment(const float4 *__restrict__ texels, int n, const float *__restrict__ dirs,
                                                           const float *__restrict__ throughput, int count, float *__restrict__ colour) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= count) return;
    const f3 c = ptd::miss_colour(ptd::mk(throughput[3 * i], throughput[3 * i + 1], throughput[3 * i + 2]),
                                  ptd::mk(dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2]), texels, n);
    colour[3 * i] = c.x; colour[3 * i + 1] = c.y; colour[3 * i + 2] = c.z;
}

// the shader clock while whatever else is running runs: one wave counts its cycle counter (s_memtime) against the constant
// 100-MHz counter (s_memrealtime) for `ticks` of the latter.  Sixteen scalar registers: it has to fit beside a persistent
// grid that leaves 32 of a SIMD's 800 free (pt_k_image.hpp: k_gather_one).  Ends by itself: the real-time counter advances.
__global__ __launch_bounds__(64) __attribute__((amdgpu_num_sgpr(16), amdgpu_num_vgpr(32))) void k_probe_clock(unsigned long long *out, unsigned ticks) {
    if (threadIdx.x != 0) return;
    const unsigned long long t0 = wall_clock64(), c0 = clock64();
    unsigned long long t1 = t0;
    while (t1 - t0 < (unsigned long long)ticks) { __builtin_amdgcn_s_sleep(8); t1 = wall_clock64(); }
    const unsigned long long c1 = clock64();
    out[0] = c1 - c0; out[1] = t1 - t0;
}

// the every-triangle loop's first stage (pt_k_trisweep.hpp) on caller rays, through mesh_sweep's own device code: one wave per
// 64 rays builds its B operands (tri_ray_operands) and evaluates every group of 16 records (tri_group_form); written out are
// each ray's 32 slots as ray_slots made them (before the LDS shuffle), its class (0 plain, 1 far, 2 wild) and the raw binary32
// result of every (ray, record) pair, padding records included: form[ray * n64 + record]
__global__ __launch_bounds__(64) void k_probe_tri_form(const pt_half8 *__restrict__ recs, int n64, float gx, float gy, float gz, float ir,
                                                        float rmax, const float *o, const float *d, int n, _Float16 *slots, int32_t *cls,
                                                        float *form) {
    __shared__ pt_half8 scratch[32 * 4];
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 64 + lane;
    const bool active = i < n;
    f3 ro = ptd::mk(0.0f, 0.0f, 0.0f), rd = ptd::mk(0.0f, 0.0f, 0.0f);
    if (active) { ro = ptd::mk(o[3 * i], o[3 * i + 1], o[3 * i + 2]); rd = ptd::mk(d[3 * i], d[3 * i + 1], d[3 * i + 2]); }
    const bool wild = cull_ray(ro, rd, rmax).wild;                  // (k_bounce: m_wild, the same test against the scene's bound)
    pt_half8 mine[4], bf[4];
    bool far;
    tri_ray_operands(scratch, gx, gy, gz, ir, ro, rd, ballot64(active), ballot64(wild), mine, far, bf);
    if (active) {
        if (slots)
            for (int q = 0; q < 4; ++q)
                for (int k = 0; k < 8; ++k) slots[(size_t)i * 32 + 8 * q + k] = mine[q][k];
        if (cls) cls[i] = wild ? 2 : far ? 1 : 0;
    }
    if (!form) return;                                              // (wave-uniform)
    const pt_half8 *rec = recs + (size_t)(lane & 15) * 4 + (lane >> 4);
    for (int g = 0; g < (n64 >> 4); ++g) {
        pt_float4v acc[4];
        (void)tri_group_form(rec[(size_t)g * 64], bf, acc);
        for (int gI = 0; gI < 4; ++gI)
            for (int r = 0; r < 4; ++r) {
                const int ray = blockIdx.x * 64 + 16 * gI + (lane & 15);
                if (ray < n) form[(size_t)ray * n64 + 16 * g + 4 * (lane >> 4) + r] = acc[gI][r];
            }
    }
}

// device scratch of one probe call: freed on every exit path.  A failed allocation or upload sticks: the call site asks ok() once,
// after its last buffer
struct ProbeBufs {
    std::vector<void *> mem;
    bool failed = false;
    ~ProbeBufs() { for (void *p : mem) if (p) (void)hipFree(p); }
    void *get(size_t bytes, const void *init) {
        void *p = nullptr;
        if (failed || hipMalloc(&p, bytes ? bytes : 4) != hipSuccess) { failed = true; return nullptr; }
        mem.push_back(p);
        if (init ? hipMemcpy(p, init, bytes, hipMemcpyHostToDevice) != hipSuccess : hipMemset(p, 0, bytes ? bytes : 4) != hipSuccess) failed = true;
        return failed ? nullptr : p;
    }
    // `count` elements of the caller's array on the device; an array the caller left out (nullptr) stays nullptr
    template <typename T> T *in(const T *host, size_t count) { return host ? (T *)get(count * sizeof(T), host) : nullptr; }
    // `count` zeroed elements for the kernel to write
    template <typename T> T *out(size_t count) { return (T *)get(count * sizeof(T), nullptr); }
    bool ok() const { return !failed; }
    // ... and back (a result the caller did not ask for, host == nullptr, is skipped)
    template <typename T> hipError_t fetch(T *host, const T *dev, size_t count) {
        return host ? hipMemcpy(host, dev, count * sizeof(T), hipMemcpyDeviceToHost) : hipSuccess;
    }
};

// what entry point `who` answers when its buffers could not be made
int probe_no_device(const char *who) {
    (void)hipGetLastError();
    return fail(PT_ERR_DEVICE, "%s: no HIP device / out of memory (this library has no CPU fallback)", who);
}

// every record that hits (t > 0) names a material of the table
int probe_check_materials(const char *who, const pt_shadeable_intersection *isects, int n, int num_materials) {
    for (int i = 0; i < n; ++i)
        if (isects[i].t > 0.0f && (isects[i].materialId < 0 || isects[i].materialId >= num_materials))
            return fail(PT_ERR_INVALID, "%s: record %d hits material %d of %d", who, i, isects[i].materialId, num_materials);
    return PT_OK;
}
// ... and a primitive of the scene; isects == nullptr: the records are primitives and points, and every one is looked at
int probe_check_geoms(const char *who, const pt_shadeable_intersection *isects, const int32_t *hit_geom, int n, int num_geoms) {
    for (int i = 0; i < n; ++i)
        if ((!isects || isects[i].t > 0.0f) && (hit_geom[i] < 0 || hit_geom[i] >= num_geoms))
            return fail(PT_ERR_INVALID, "%s: record %d names primitive %d of %d", who, i, hit_geom[i], num_geoms);
    return PT_OK;
}

// (texels in the session's device layouts: rgb_quads / bump_pairs, pt_h_state.hpp)
// a per-material table of cube maps (`what`: "texture" / "bump map"; material m: n[m] x n[m] texels per face from texel offset[m],
// n[m] == 0: none) as the kernels read it, {offset, n} per material, and the texels it reaches
int probe_cube_table(const char *who, const char *what, int num_materials, const int32_t *n, const int32_t *offset, std::vector<int2> &tab,
                     size_t &reach) {
    tab.resize((size_t)num_materials);
    reach = 0;
    for (int m = 0; m < num_materials; ++m) {
        if (n[m] < 0 || n[m] > 1024 || (n[m] > 0 && offset[m] < 0))
            return fail(PT_ERR_INVALID, "%s: material %d has a %s of n = %d at offset %d", who, m, what, n[m], offset[m]);
        if (n[m] > 0) reach = std::max(reach, (size_t)offset[m] + (size_t)6 * (size_t)n[m] * (size_t)n[m]);
        tab[(size_t)m] = make_int2(n[m] > 0 ? offset[m] : 0, n[m]);
    }
    return PT_OK;
}

// the arguments every shade-scatter probe takes (deferred: 0 where the probe has none); true: refuse.  Everything is refused
// before anything is launched: the kernels never index past the material table
bool probe_shade_args_bad(int n, int num_materials, int deferred, const pt_path_segment *paths, const pt_shadeable_intersection *isects,
                          const pt_material *materials) {
    return n < 0 || n > (1 << 26) || num_materials < 1 || (deferred != 0 && deferred != 1) || (n > 0 && (!paths || !isects || !materials));
}

// the records of a shade-scatter probe on the device -- pt_init's own material records, the paths, the intersections, `outside`
// where the caller gave it -- with room for the probe's own inputs; after the launch, finish() brings the paths back
struct ShadeRecords : ProbeBufs {
    const float *mats;
    pt_path_segment *paths, *host_paths;
    const pt_shadeable_intersection *isects;
    const uint8_t *outside;
    size_t n;
    ShadeRecords(const pt_material *materials, int num_materials, bool glossy, pt_path_segment *paths_, const pt_shadeable_intersection *isects_,
                 const uint8_t *outside_, int n_) : host_paths(paths_), n((size_t)n_) {
        std::vector<float> mrec((size_t)num_materials * ptd::MAT_WORDS, 0.0f);
        one::pack_materials(materials, num_materials, mrec.data(), glossy);
        mats = in(mrec.data(), mrec.size());
        paths = in(paths_, n);
        isects = in(isects_, n);
        outside = in(outside_, n);
    }
    dim3 grid() const { return dim3((unsigned)((n + 63) / 64)); }
    int finish() {
        HIPCHK(hipGetLastError());
        HIPCHK(fetch(host_paths, paths, n));
        HIPCHK(hipDeviceSynchronize());
        return PT_OK;
    }
};

// pt_probe_shade_scatter (glossy = false) and pt_probe_shade_scatter_glossy (true): `who` names the entry point in messages
int probe_shade_scatter(const char *who, bool glossy, int iter, int depth, const pt_material *materials, int num_materials,
                        pt_path_segment *paths, const pt_shadeable_intersection *isects, const uint8_t *outside, int n, int deferred) {
    if (probe_shade_args_bad(n, num_materials, deferred, paths, isects, materials)) return fail(PT_ERR_INVALID, "%s: bad argument", who);
    const int rc = probe_check_materials(who, isects, n, num_materials);
    if (rc) return rc;
    if (n == 0) return PT_OK;
    ShadeRecords r(materials, num_materials, glossy, paths, isects, outside, n);
    if (!r.ok()) return probe_no_device(who);
    if (glossy) hipLaunchKernelGGL(k_probe_shade_scatter<true>, r.grid(), dim3(64), 0, 0, iter, depth, r.mats, r.paths, r.isects, r.outside, n, deferred);
    else hipLaunchKernelGGL(k_probe_shade_scatter<false>, r.grid(), dim3(64), 0, 0, iter, depth, r.mats, r.paths, r.isects, r.outside, n, deferred);
    return r.finish();
}

// the light table of a probe call: pt_init's own functions; -1 with the message set
int probe_light_records(const char *who, const pt_geom *geoms, int num_geoms, const pt_material *materials, int num_materials,
                        std::vector<float> &rec) {
    if (num_geoms < 0 || num_materials < 1 || !materials || (num_geoms > 0 && !geoms)) return fail(PT_ERR_INVALID, "%s: bad argument", who);
    std::vector<pt_light_element> el;
    const int ne = ptlight::elements(geoms, num_geoms, materials, num_materials, el);
    if (ne < 0) return fail(PT_ERR_INVALID, "%s: a cube or sphere names a material outside [0, %d)", who, num_materials);
    if (ne > ptlight::MAX_ELEMENTS) return fail(PT_ERR_INVALID, "%s: %d light elements (at most %d)", who, ne, ptlight::MAX_ELEMENTS);
    ptlight::records(geoms, el, rec);
    return ne;
}

// both direct forms of the shader probe: texels == nullptr -- the lamps' table; otherwise the table of a PT_DIRECT_SKY session
// under the map (texels, env_n), as pt_set_environment makes it
int probe_shade_scatter_direct(const char *who, int iter, int depth, int trace_depth, const pt_geom *geoms, int num_geoms,
                               const pt_material *materials, int num_materials, pt_path_segment *paths,
                               const pt_shadeable_intersection *isects, const uint8_t *outside, const int32_t *hit_geom, int n,
                               const float *texels, int env_n) {
    if (probe_shade_args_bad(n, num_materials, 0, paths, isects, materials) || trace_depth < 1 || trace_depth > MAX_DEPTH - 1 || depth < 0 ||
        depth > trace_depth || (n > 0 && depth == trace_depth && !hit_geom))
        return fail(PT_ERR_INVALID, "%s: bad argument", who);
    const int rc = probe_check_materials(who, isects, n, num_materials);
    if (rc) return rc;
    std::vector<float> rec;
    int ne = probe_light_records(who, geoms, num_geoms, materials, num_materials, rec);
    if (ne < 0) return ne;
    if (n == 0) return PT_OK;
    std::vector<float> quad;
    if (texels && env_n > 0) {
        std::vector<float> rows, cols, all;
        if (ptlight::sky_table(texels, env_n, rows, cols)) {
            ne = ptlight::sky_records(rec, env_n, rows, cols, all);
            rec.swap(all);
        }
        quad = rgb_quads(texels, (size_t)6 * (size_t)env_n * (size_t)env_n);
    } else {
        env_n = 0;
    }
    ShadeRecords r(materials, num_materials, false, paths, isects, outside, n);
    const float *d_l = ne > 0 ? r.in(rec.data(), rec.size()) : nullptr;
    const float4 *d_env = env_n > 0 ? (const float4 *)r.in(quad.data(), quad.size()) : nullptr;
    const int32_t *d_hit = r.in(hit_geom, (size_t)n);
    if (!r.ok()) return probe_no_device(who);
    hipLaunchKernelGGL(k_probe_shade_scatter_direct, r.grid(), dim3(64), 0, 0, iter, depth, trace_depth, r.mats, d_l, ne, r.paths, r.isects, r.outside,
                       d_hit, n, d_env, env_n);
    return r.finish();
}

// ---- texture mapping (PT_TEXTURES) ----
// the primitives of a probe call as the lookups read them: inverseTransform as 12 words (4 columns x 3 rows) and the type
void texture_geoms(const pt_geom *geoms, int num_geoms, std::vector<float> &inv, std::vector<int32_t> &type) {
    inv.assign((size_t)std::max(1, num_geoms) * 12, 0.0f);
    type.assign((size_t)std::max(1, num_geoms), (int32_t)PT_TRIANGLE_MESH);
    for (int g = 0; g < num_geoms; ++g) {
        for (int c = 0; c < 4; ++c)
            for (int r = 0; r < 3; ++r) inv[(size_t)g * 12 + c * 3 + r] = geoms[g].inverseTransform.m[c][r];
        type[(size_t)g] = (int32_t)geoms[g].type;
    }
}
// the refusals pt_texture_texel and pt_probe_texture share; 0 when the arguments are sound
int texture_args(const char *who, const pt_geom *geoms, int num_geoms, const int32_t *hit_geom, const float *points, int count, int n) {
    if (count < 0 || num_geoms < 0 || n < 1 || n > 1024 || (num_geoms > 0 && !geoms) || (count > 0 && (!hit_geom || !points)))
        return fail(PT_ERR_INVALID, "%s: bad argument (count %d, %d geoms, n %d)", who, count, num_geoms, n);
    return probe_check_geoms(who, nullptr, hit_geom, count, num_geoms);
}

// ---- bump mapping (PT_TEXTURES) ----
// the primitives as ptd::bump_normal reads them: inverseTransform, transform, invTranspose, 12 words each, and the type
void bump_geoms(const pt_geom *geoms, int num_geoms, std::vector<float> &rec, std::vector<int32_t> &type) {
    rec.assign((size_t)std::max(1, num_geoms) * 36, 0.0f);
    type.assign((size_t)std::max(1, num_geoms), (int32_t)PT_TRIANGLE_MESH);
    for (int g = 0; g < num_geoms; ++g) {
        const pt_mat4 *ms[3] = {&geoms[g].inverseTransform, &geoms[g].transform, &geoms[g].invTranspose};
        for (int m = 0; m < 3; ++m)
            for (int c = 0; c < 4; ++c)
                for (int r = 0; r < 3; ++r) rec[(size_t)g * 36 + m * 12 + c * 3 + r] = ms[m]->m[c][r];
        type[(size_t)g] = (int32_t)geoms[g].type;
    }
}
int bump_args(const char *who, const pt_geom *geoms, int num_geoms, const int32_t *hit_geom, const float *points, const float *normals,
              const float *dirs, int count, const float *texels, int n, float *out_normals, uint8_t *perturbed) {
    const int rc = texture_args(who, geoms, num_geoms, hit_geom, points, count, n);
    if (rc) return rc;
    if (!texels || (count > 0 && (!normals || !dirs || !out_normals || !perturbed)))
        return fail(PT_ERR_INVALID, "%s: null array (count %d)", who, count);
    return PT_OK;
}

}  // namespace

// ---- the entry points (include/ptmi355.h) ----
int pt_probe_rng(const uint32_t *seeds, int n, int draws, uint32_t *state, float *u) {
    if (n < 0 || draws < 0 || (n > 0 && !seeds)) return fail(PT_ERR_INVALID, "pt_probe_rng: bad argument");
    if (n == 0) return PT_OK;
    ProbeBufs b;
    const uint32_t *d_seeds = b.in(seeds, (size_t)n);
    uint32_t *d_state = b.out<uint32_t>((size_t)n);
    float *d_u = b.out<float>((size_t)n);
    if (!b.ok()) return probe_no_device("pt_probe_rng");
    hipLaunchKernelGGL(k_probe_rng, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, d_seeds, n, draws, d_state, d_u);
    HIPCHK(hipGetLastError());
    HIPCHK(b.fetch(state, d_state, (size_t)n));
    HIPCHK(b.fetch(u, d_u, (size_t)n));
    HIPCHK(hipDeviceSynchronize());
    return PT_OK;
}

int pt_probe_sincos(const float *x, uint32_t first_bits, uint32_t n, float *s, float *c, uint64_t sum[2]) {
    if (n == 0) { if (sum) sum[0] = sum[1] = 0; return PT_OK; }
    // arrays of n floats (inputs or outputs) are bounded; the array-free form (arguments from first_bits, checksums only)
    // may sweep every binary32 value
    if ((x || s || c) && n > (1u << 28)) return fail(PT_ERR_INVALID, "pt_probe_sincos: %u elements with arrays (at most 2^28)", n);
    ProbeBufs b;
    const float *d_x = b.in(x, (size_t)n);
    float *d_s = s ? b.out<float>((size_t)n) : nullptr;
    float *d_c = c ? b.out<float>((size_t)n) : nullptr;
    unsigned long long *d_sum = b.out<unsigned long long>(2);
    if (!b.ok()) return probe_no_device("pt_probe_sincos");
    const unsigned blocks = (unsigned)std::min<uint64_t>(((uint64_t)n + 255) / 256, 4096);
    hipLaunchKernelGGL(k_probe_sincos, dim3(blocks), dim3(256), 0, 0, d_x, first_bits, n, d_s, d_c, d_sum);
    HIPCHK(hipGetLastError());
    HIPCHK(b.fetch(s, d_s, (size_t)n));
    HIPCHK(b.fetch(c, d_c, (size_t)n));
    HIPCHK(b.fetch((unsigned long long *)sum, d_sum, 2));
    HIPCHK(hipDeviceSynchronize());
    return PT_OK;
}

int pt_probe_sqrt(uint32_t first_bits, uint32_t n, uint64_t mismatch[2]) {
    if (!mismatch) return fail(PT_ERR_INVALID, "pt_probe_sqrt: null result");
    mismatch[0] = mismatch[1] = 0;
    if (n == 0) return PT_OK;
    ProbeBufs b;
    unsigned long long *d_bad = b.out<unsigned long long>(2);
    if (!b.ok()) return probe_no_device("pt_probe_sqrt");
    const unsigned blocks = (unsigned)std::min<uint64_t>(((uint64_t)n + 255) / 256, 8192);
    hipLaunchKernelGGL(k_probe_sqrt, dim3(blocks), dim3(256), 0, 0, first_bits, n, d_bad);
    HIPCHK(hipGetLastError());
    HIPCHK(b.fetch((unsigned long long *)mismatch, d_bad, 2));
    HIPCHK(hipDeviceSynchronize());
    return PT_OK;
}

int pt_probe_clock(int microseconds, double *ghz) {
    if (!ghz || microseconds < 1 || microseconds > 100000) return fail(PT_ERR_INVALID, "pt_probe_clock: bad argument");
    *ghz = 0.0;
    unsigned long long *h = nullptr, *d = nullptr;
    hipStream_t st = nullptr;
    int lo = 0, hi = 0;
    if (hipHostMalloc((void **)&h, 16, hipHostMallocMapped) != hipSuccess || hipHostGetDevicePointer((void **)&d, h, 0) != hipSuccess) {
        (void)hipGetLastError();
        if (h) (void)hipHostFree(h);
        return fail(PT_ERR_DEVICE, "pt_probe_clock: no HIP device / no mappable host memory (this library has no CPU fallback)");
    }
    h[0] = h[1] = 0;
    if (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess) { (void)hipGetLastError(); lo = hi = 0; }
    hipError_t e = hipStreamCreateWithPriority(&st, hipStreamNonBlocking, hi);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_probe_clock, dim3(1), dim3(64), 0, st, d, (unsigned)microseconds * 100u);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(st);       // (this stream only: whatever else is enqueued keeps running)
        (void)hipStreamDestroy(st);
    }
    const unsigned long long cycles = h[0], ticks = h[1];
    (void)hipHostFree(h);
    if (e != hipSuccess) return fail(PT_ERR_DEVICE, "pt_probe_clock: %s", hipGetErrorString(e));
    if (!ticks) return fail(PT_ERR_INTERNAL, "pt_probe_clock: the probe left no counts");
    *ghz = (double)cycles / ((double)ticks * 10.0);              // cycles per nanosecond
    return PT_OK;
}

int pt_probe_own_surface_plan(uint64_t paths, int ngeoms, int plain_fused) {
    return own_surface_plan(paths, ngeoms, plain_fused != 0) ? 1 : 0;
}

int pt_probe_hemisphere(const float *normals, const uint32_t *seeds, int n, float *dirs) {
    if (n < 0 || (n > 0 && (!normals || !seeds || !dirs))) return fail(PT_ERR_INVALID, "pt_probe_hemisphere: bad argument");
    if (n == 0) return PT_OK;
    ProbeBufs b;
    const float *d_n = b.in(normals, 3 * (size_t)n);
    const uint32_t *d_seeds = b.in(seeds, (size_t)n);
    float *d_d = b.out<float>(3 * (size_t)n);
    if (!b.ok()) return probe_no_device("pt_probe_hemisphere");
    hipLaunchKernelGGL(k_probe_hemisphere, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, d_n, d_seeds, n, d_d);
    HIPCHK(hipGetLastError());
    HIPCHK(b.fetch(dirs, d_d, 3 * (size_t)n));
    HIPCHK(hipDeviceSynchronize());
    return PT_OK;
}

int pt_glossy_alpha2(const float *exponents, int count, float *alpha2) {
    if (count < 0 || (count > 0 && (!exponents || !alpha2))) return fail(PT_ERR_INVALID, "pt_glossy_alpha2: bad argument (count %d)", count);
    for (int i = 0; i < count; ++i) alpha2[i] = one::glossy_alpha2(exponents[i]);      // pt_init's own function
    return PT_OK;
}

int pt_probe_glossy_lobe(const float *normals, const uint32_t *seeds, const float *alpha2, int n, float *dirs) {
    if (n < 0 || (n > 0 && (!normals || !seeds || !alpha2 || !dirs))) return fail(PT_ERR_INVALID, "pt_probe_glossy_lobe: bad argument");
    if (n == 0) return PT_OK;
    ProbeBufs b;
    const float *d_n = b.in(normals, 3 * (size_t)n);
    const uint32_t *d_seeds = b.in(seeds, (size_t)n);
    const float *d_a = b.in(alpha2, (size_t)n);
    float *d_d = b.out<float>(3 * (size_t)n);
    if (!b.ok()) return probe_no_device("pt_probe_glossy_lobe");
    hipLaunchKernelGGL(k_probe_glossy_lobe, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, d_n, d_seeds, d_a, n, d_d);
    HIPCHK(hipGetLastError());
    HIPCHK(b.fetch(dirs, d_d, 3 * (size_t)n));
    HIPCHK(hipDeviceSynchronize());
    return PT_OK;
}

int pt_probe_shade_scatter(int iter, int depth, const pt_material *materials, int num_materials, pt_path_segment *paths,
                           const pt_shadeable_intersection *isects, const uint8_t *outside, int n, int deferred) {
    return probe_shade_scatter("pt_probe_shade_scatter", false, iter, depth, materials, num_materials, paths, isects, outside, n, deferred);
}

int pt_probe_shade_scatter_glossy(int iter, int depth, const pt_material *materials, int num_materials, pt_path_segment *paths,
                                  const pt_shadeable_intersection *isects, const uint8_t *outside, int n, int deferred) {
    return probe_shade_scatter("pt_probe_shade_scatter_glossy", true, iter, depth, materials, num_materials, paths, isects, outside, n,
                               deferred);
}

int pt_probe_direct_sample(const pt_geom *geoms, int num_geoms, const pt_material *materials, int num_materials, const float *P,
                           const float *n, const uint32_t *seeds, int count, float *dir, float *weight, int32_t *element) {
    if (count < 0 || count > (1 << 26) || (count > 0 && (!P || !n || !seeds || !dir || !weight || !element)))
        return fail(PT_ERR_INVALID, "pt_probe_direct_sample: bad argument");
    std::vector<float> rec;
    const int ne = probe_light_records("pt_probe_direct_sample", geoms, num_geoms, materials, num_materials, rec);
    if (ne < 0) return ne;
    if (count == 0) return PT_OK;
    if (ne == 0) {
        for (int i = 0; i < count; ++i) { dir[3 * i] = dir[3 * i + 1] = dir[3 * i + 2] = 0.0f; weight[i] = 0.0f; element[i] = -1; }
        return PT_OK;
    }
    ProbeBufs b;
    const float *d_l = b.in(rec.data(), rec.size());
    const float *d_p = b.in(P, 3 * (size_t)count);
    const float *d_n = b.in(n, 3 * (size_t)count);
    const uint32_t *d_s = b.in(seeds, (size_t)count);
    float *d_d = b.out<float>(3 * (size_t)count);
    float *d_w = b.out<float>((size_t)count);
    int32_t *d_e = b.out<int32_t>((size_t)count);
    if (!b.ok()) return probe_no_device("pt_probe_direct_sample");
    hipLaunchKernelGGL(k_probe_direct_sample, dim3((unsigned)((count + 63) / 64)), dim3(64), 0, 0, d_l, ne, d_p, d_n, d_s, count, d_d, d_w, d_e);
    HIPCHK(hipGetLastError());
    HIPCHK(b.fetch(dir, d_d, 3 * (size_t)count));
    HIPCHK(b.fetch(weight, d_w, (size_t)count));
    HIPCHK(b.fetch(element, d_e, (size_t)count));
    HIPCHK(hipDeviceSynchronize());
    return PT_OK;
}

int pt_probe_shade_scatter_direct(int iter, int depth, int trace_depth, const pt_geom *geoms, int num_geoms, const pt_material *materials,
                                  int num_materials, pt_path_segment *paths, const pt_shadeable_intersection *isects,
                                  const uint8_t *outside, const int32_t *hit_geom, int n) {
    return probe_shade_scatter_direct("pt_probe_shade_scatter_direct", iter, depth, trace_depth, geoms, num_geoms, materials, num_materials,
                                      paths, isects, outside, hit_geom, n, nullptr, 0);
}

int pt_probe_shade_scatter_direct_sky(int iter, int depth, int trace_depth, const pt_geom *geoms, int num_geoms, const pt_material *materials,
                                      int num_materials, pt_path_segment *paths, const pt_shadeable_intersection *isects,
                                      const uint8_t *outside, const int32_t *hit_geom, int n, const float *texels, int env_n) {
    const char *who = "pt_probe_shade_scatter_direct_sky";
    if (env_n < 0 || env_n > 1024 || (env_n > 0 && !texels)) return fail(PT_ERR_INVALID, "%s: bad map (n = %d)", who, env_n);
    return probe_shade_scatter_direct(who, iter, depth, trace_depth, geoms, num_geoms, materials, num_materials, paths, isects, outside,
                                      hit_geom, n, texels, env_n);
}

int pt_probe_sky_sample(const float *texels, int n, const float *normals, const uint32_t *seeds, int count, float *dir, float *weight,
                        int32_t *texel) {
    if (n < 0 || n > 1024 || (n > 0 && !texels) || count < 0 || count > (1 << 26) || (count > 0 && (!normals || !seeds || !dir || !weight || !texel)))
        return fail(PT_ERR_INVALID, "pt_probe_sky_sample: bad argument (n = %d, count = %d)", n, count);
    if (count == 0) return PT_OK;
    std::vector<float> rows, cols, rec;
    if (!texels || n == 0 || !ptlight::sky_table(texels, n, rows, cols)) {
        for (int i = 0; i < count; ++i) { dir[3 * i] = dir[3 * i + 1] = dir[3 * i + 2] = 0.0f; weight[i] = 0.0f; texel[i] = -1; }
        return PT_OK;
    }
    const int ne = ptlight::sky_records(std::vector<float>(), n, rows, cols, rec);
    ProbeBufs b;
    const float *d_l = b.in(rec.data(), rec.size());
    const float *d_n = b.in(normals, 3 * (size_t)count);
    const uint32_t *d_s = b.in(seeds, (size_t)count);
    float *d_d = b.out<float>(3 * (size_t)count);
    float *d_w = b.out<float>((size_t)count);
    int32_t *d_t = b.out<int32_t>((size_t)count);
    if (!b.ok()) return probe_no_device("pt_probe_sky_sample");
    hipLaunchKernelGGL(k_probe_sky_sample, dim3((unsigned)((count + 63) / 64)), dim3(64), 0, 0, d_l, ne, d_n, d_s, count, d_d, d_w, d_t);
    HIPCHK(hipGetLastError());
    HIPCHK(b.fetch(dir, d_d, 3 * (size_t)count));
    HIPCHK(b.fetch(weight, d_w, (size_t)count));
    HIPCHK(b.fetch(texel, d_t, (size_t)count));
    HIPCHK(hipDeviceSynchronize());
    return PT_OK;
}

int pt_texture_texel(const pt_geom *geoms, int num_geoms, const int32_t *hit_geom, const float *points, int count, int n, int32_t *index) {
    const int rc = texture_args("pt_texture_texel", geoms, num_geoms, hit_geom, points, count, n);
    if (rc) return rc;
    if (count > 0 && !index) return fail(PT_ERR_INVALID, "pt_texture_texel: null index");
    std::vector<float> inv;
    std::vector<int32_t> type;
    texture_geoms(geoms, num_geoms, inv, type);
    for (int i = 0; i < count; ++i) {
        const int g = hit_geom[i];
        index[i] = (type[(size_t)g] == PT_SPHERE || type[(size_t)g] == PT_CUBE)
                       ? ptd::texture_texel(inv.data() + (size_t)g * 12, points[3 * i], points[3 * i + 1], points[3 * i + 2], n) : -1;
    }
    return PT_OK;
}

int pt_probe_texture(const pt_geom *geoms, int num_geoms, const int32_t *hit_geom, const float *points, int count, const float *texels, int n,
                     const float *colour_in, float *colour_out) {
    const int rc = texture_args("pt_probe_texture", geoms, num_geoms, hit_geom, points, count, n);
    if (rc) return rc;
    if (count > (1 << 26) || !texels || (count > 0 && (!colour_in || !colour_out)))
        return fail(PT_ERR_INVALID, "pt_probe_texture: bad argument (count %d)", count);
    if (count == 0) return PT_OK;
    std::vector<float> inv;
    std::vector<int32_t> type;
    texture_geoms(geoms, num_geoms, inv, type);
    const std::vector<float> quad = rgb_quads(texels, (size_t)6 * (size_t)n * (size_t)n);
    ProbeBufs b;
    const float4 *d_tex = (const float4 *)b.in(quad.data(), quad.size());
    const float *d_inv = b.in(inv.data(), inv.size());
    const int32_t *d_type = b.in(type.data(), type.size());
    const int32_t *d_hit = b.in(hit_geom, (size_t)count);
    const float *d_pts = b.in(points, 3 * (size_t)count);
    const float *d_in = b.in(colour_in, 3 * (size_t)count);
    float *d_out = b.out<float>(3 * (size_t)count);
    if (!b.ok()) return probe_no_device("pt_probe_texture");
    hipLaunchKernelGGL(k_probe_texture, dim3((unsigned)((count + 63) / 64)), dim3(64), 0, 0, d_inv, d_type, d_hit, d_pts, count, d_tex, n, d_in, d_out);
    HIPCHK(hipGetLastError());
    HIPCHK(b.fetch(colour_out, d_out, 3 * (size_t)count));
    HIPCHK(hipDeviceSynchronize());
    return PT_OK;
}

int pt_probe_shade_scatter_textured(int iter, int depth, const pt_material *materials, int num_materials, pt_path_segment *paths,
                                    const pt_shadeable_intersection *isects, const uint8_t *outside, int n, int deferred,
                                    const pt_geom *geoms, int num_geoms, const int32_t *hit_geom, const float *tex_texels,
                                    const int32_t *tex_n, const int32_t *tex_offset) {
    const char *who = "pt_probe_shade_scatter_textured";
    if (probe_shade_args_bad(n, num_materials, deferred, paths, isects, materials) || num_geoms < 0 || (num_geoms > 0 && !geoms) ||
        (n > 0 && !hit_geom) || !tex_n || !tex_offset)
        return fail(PT_ERR_INVALID, "%s: bad argument", who);
    std::vector<int2> tab;
    size_t total = 0;                                              // texels the table reaches
    int rc = probe_check_materials(who, isects, n, num_materials);
    if (!rc) rc = probe_check_geoms(who, isects, hit_geom, n, num_geoms);
    if (!rc) rc = probe_cube_table(who, "texture", num_materials, tex_n, tex_offset, tab, total);
    if (rc) return rc;
    if (total > 0 && !tex_texels) return fail(PT_ERR_INVALID, "%s: null tex_texels", who);
    if (total > (size_t)0x7fffffff) return fail(PT_ERR_INVALID, "%s: %zu texels in all (at most 2^31 - 1)", who, total);
    if (n == 0) return PT_OK;
    std::vector<float> inv;
    std::vector<int32_t> type;
    texture_geoms(geoms, num_geoms, inv, type);
    const std::vector<float> quad = rgb_quads(tex_texels, total);
    ShadeRecords r(materials, num_materials, false, paths, isects, outside, n);
    const float *d_inv = r.in(inv.data(), inv.size());
    const int32_t *d_type = r.in(type.data(), type.size());
    const int32_t *d_hit = r.in(hit_geom, (size_t)n);
    const float4 *d_tex = (const float4 *)r.in(quad.data(), quad.size());
    const int2 *d_tab = r.in(tab.data(), tab.size());
    if (!r.ok()) return probe_no_device(who);
    hipLaunchKernelGGL(k_probe_shade_scatter_textured, r.grid(), dim3(64), 0, 0, iter, depth, r.mats, r.paths, r.isects, r.outside, n, deferred,
                       d_inv, d_type, d_hit, d_tex, d_tab);
    return r.finish();
}

int pt_bump_normal(const pt_geom *geoms, int num_geoms, const int32_t *hit_geom, const float *points, const float *normals, const float *dirs,
                   int count, const float *texels, int n, float *out_normals, uint8_t *perturbed) {
    const int rc = bump_args("pt_bump_normal", geoms, num_geoms, hit_geom, points, normals, dirs, count, texels, n, out_normals, perturbed);
    if (rc) return rc;
    std::vector<float> rec;
    std::vector<int32_t> type;
    bump_geoms(geoms, num_geoms, rec, type);
    const std::vector<float> pair = bump_pairs(texels, (size_t)6 * (size_t)n * (size_t)n);
    for (int i = 0; i < count; ++i) {
        const int g = hit_geom[i];
        float x = normals[3 * i], y = normals[3 * i + 1], z = normals[3 * i + 2];
        bool hit = false;
        if (type[(size_t)g] == PT_SPHERE || type[(size_t)g] == PT_CUBE)
            hit = ptd::bump_normal((uint32_t)type[(size_t)g], rec.data() + (size_t)g * 36, points[3 * i], points[3 * i + 1], points[3 * i + 2],
                                   dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2], x, y, z, (const ptd::bump_texel *)pair.data(), n, x, y, z);
        out_normals[3 * i] = x; out_normals[3 * i + 1] = y; out_normals[3 * i + 2] = z;
        perturbed[i] = hit ? 1 : 0;
    }
    return PT_OK;
}

int pt_probe_bump_normal(const pt_geom *geoms, int num_geoms, const int32_t *hit_geom, const float *points, const float *normals, const float *dirs,
                         int count, const float *texels, int n, float *out_normals, uint8_t *perturbed) {
    const int rc = bump_args("pt_probe_bump_normal", geoms, num_geoms, hit_geom, points, normals, dirs, count, texels, n, out_normals, perturbed);
    if (rc) return rc;
    if (count > (1 << 26)) return fail(PT_ERR_INVALID, "pt_probe_bump_normal: bad argument (count %d)", count);
    if (count == 0) return PT_OK;
    std::vector<float> rec;
    std::vector<int32_t> type;
    bump_geoms(geoms, num_geoms, rec, type);
    const std::vector<float> pair = bump_pairs(texels, (size_t)6 * (size_t)n * (size_t)n);
    ProbeBufs b;
    const ptd::bump_texel *d_tex = (const ptd::bump_texel *)b.in(pair.data(), pair.size());
    const float *d_rec = b.in(rec.data(), rec.size());
    const int32_t *d_type = b.in(type.data(), type.size());
    const int32_t *d_hit = b.in(hit_geom, (size_t)count);
    const float *d_pts = b.in(points, 3 * (size_t)count);
    const float *d_nrm = b.in(normals, 3 * (size_t)count);
    const float *d_dir = b.in(dirs, 3 * (size_t)count);
    float *d_out = b.out<float>(3 * (size_t)count);
    uint8_t *d_flag = b.out<uint8_t>((size_t)count);
    if (!b.ok()) return probe_no_device("pt_probe_bump_normal");
    hipLaunchKernelGGL(k_probe_bump_normal, dim3((unsigned)((count + 63) / 64)), dim3(64), 0, 0, d_rec, d_type, d_hit, d_pts, d_nrm, d_dir, count,
                       d_tex, n, d_out, d_flag);
    HIPCHK(hipGetLastError());
    HIPCHK(b.fetch(out_normals, d_out, 3 * (size_t)count));
    HIPCHK(b.fetch(perturbed, d_flag, (size_t)count));
    HIPCHK(hipDeviceSynchronize());
    return PT_OK;
}

// ---- smooth mesh normals (PT_SMOOTH_NORMALS) ----
namespace {
int smooth_args(const char *who, const pt_triangle *triangles, const float *normals, int num_triangles, const int32_t *tri, const float *origins,
                const float *dirs, int count, float *out_normals, uint8_t *smoothed) {
    if (count < 0 || num_triangles < 0) return fail(PT_ERR_INVALID, "%s: bad argument (count %d, num_triangles %d)", who, count, num_triangles);
    if ((num_triangles > 0 && (!triangles || !normals)) || (count > 0 && (!tri || !origins || !dirs || !out_normals || !smoothed)))
        return fail(PT_ERR_INVALID, "%s: null array (count %d)", who, count);
    for (int i = 0; i < count; ++i)
        if (tri[i] < 0 || tri[i] >= num_triangles) return fail(PT_ERR_INVALID, "%s: tri[%d] = %d outside [0, %d)", who, i, tri[i], num_triangles);
    return PT_OK;
}
// the triangles as the device records hold them (pt_init): v0, e1 = fl(v1 - v0), e2 = fl(v2 - v0)
std::vector<float> smooth_records(const pt_triangle *triangles, int num_triangles) {
    std::vector<float> rec((size_t)std::max(1, num_triangles) * TRI_WORDS, 0.0f);
    for (int i = 0; i < num_triangles; ++i) {
        const pt_triangle &t = triangles[i];
        float *r = rec.data() + (size_t)i * TRI_WORDS;
        r[0] = t.v0.x; r[1] = t.v0.y; r[2] = t.v0.z;
        r[3] = t.v1.x - t.v0.x; r[4] = t.v1.y - t.v0.y; r[5] = t.v1.z - t.v0.z;
        r[6] = t.v2.x - t.v0.x; r[7] = t.v2.y - t.v0.y; r[8] = t.v2.z - t.v0.z;
    }
    return rec;
}
}  // namespace

int pt_smooth_normal(const pt_triangle *triangles, const float *normals, int num_triangles, const int32_t *tri, const float *origins,
                     const float *dirs, int count, float *out_normals, uint8_t *smoothed) {
    const int rc = smooth_args("pt_smooth_normal", triangles, normals, num_triangles, tri, origins, dirs, count, out_normals, smoothed);
    if (rc) return rc;
    const std::vector<float> rec = smooth_records(triangles, num_triangles);
    for (int i = 0; i < count; ++i) {
        const float *tv = rec.data() + (size_t)tri[i] * TRI_WORDS;
        // the facet normal of tile_result: glm's normalize(cross(e1, e2))
        const float cx = tv[4] * tv[8] - tv[7] * tv[5], cy = tv[5] * tv[6] - tv[8] * tv[3], cz = tv[3] * tv[7] - tv[6] * tv[4];
        const float inv_len = 1.0f / __builtin_sqrtf((cx * cx + cy * cy) + cz * cz);
        const float nrx = cx * inv_len, nry = cy * inv_len, nrz = cz * inv_len;
        float x = nrx, y = nry, z = nrz;
        const bool hit = ptd::smooth_normal(tv, normals + (size_t)tri[i] * 9, origins[3 * i], origins[3 * i + 1], origins[3 * i + 2],
                                            dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2], nrx, nry, nrz, x, y, z);
        out_normals[3 * i] = x; out_normals[3 * i + 1] = y; out_normals[3 * i + 2] = z;
        smoothed[i] = hit ? 1 : 0;
    }
    return PT_OK;
}

int pt_probe_smooth_normal(const pt_triangle *triangles, const float *normals, int num_triangles, const int32_t *tri, const float *origins,
                           const float *dirs, int count, float *out_normals, uint8_t *smoothed) {
    // (the bound on the count first: smooth_args reads every tri entry)
    if (count > (1 << 26)) return fail(PT_ERR_INVALID, "pt_probe_smooth_normal: bad argument (count %d)", count);
    const int rc = smooth_args("pt_probe_smooth_normal", triangles, normals, num_triangles, tri, origins, dirs, count, out_normals, smoothed);
    if (rc) return rc;
    if (count == 0) return PT_OK;
    const std::vector<float> rec = smooth_records(triangles, num_triangles);
    ProbeBufs b;
    const float *d_rec = b.in(rec.data(), rec.size());
    const float *d_vn = b.in(normals, 9 * (size_t)num_triangles);
    const int32_t *d_tri = b.in(tri, (size_t)count);
    const float *d_org = b.in(origins, 3 * (size_t)count);
    const float *d_dir = b.in(dirs, 3 * (size_t)count);
    float *d_out = b.out<float>(3 * (size_t)count);
    uint8_t *d_flag = b.out<uint8_t>((size_t)count);
    if (!b.ok()) return probe_no_device("pt_probe_smooth_normal");
    hipLaunchKernelGGL(k_probe_smooth_normal, dim3((unsigned)((count + 63) / 64)), dim3(64), 0, 0, d_rec, d_vn, d_tri, d_org, d_dir, count, d_out, d_flag);
    HIPCHK(hipGetLastError());
    HIPCHK(b.fetch(out_normals, d_out, 3 * (size_t)count));
    HIPCHK(b.fetch(smoothed, d_flag, (size_t)count));
    HIPCHK(hipDeviceSynchronize());
    return PT_OK;
}

int pt_probe_shade_scatter_bumped(int iter, int depth, const pt_material *materials, int num_materials, pt_path_segment *paths,
                                  const pt_shadeable_intersection *isects, const uint8_t *outside, int n, int deferred,
                                  const pt_geom *geoms, int num_geoms, const int32_t *hit_geom, const float *tex_texels,
                                  const int32_t *tex_n, const int32_t *tex_offset, const float *bump_texels, const int32_t *bump_n,
                                  const int32_t *bump_offset) {
    const char *who = "pt_probe_shade_scatter_bumped";
    if (probe_shade_args_bad(n, num_materials, deferred, paths, isects, materials) || num_geoms < 0 || (num_geoms > 0 && !geoms) ||
        (n > 0 && !hit_geom) || !tex_n || !tex_offset || !bump_n || !bump_offset)
        return fail(PT_ERR_INVALID, "%s: bad argument", who);
    std::vector<int2> tab, btab;
    size_t total = 0, btotal = 0;                                  // texels the two tables reach
    int rc = probe_check_materials(who, isects, n, num_materials);
    if (!rc) rc = probe_check_geoms(who, isects, hit_geom, n, num_geoms);
    if (!rc) rc = probe_cube_table(who, "texture", num_materials, tex_n, tex_offset, tab, total);
    if (!rc) rc = probe_cube_table(who, "bump map", num_materials, bump_n, bump_offset, btab, btotal);
    if (rc) return rc;
    if ((total > 0 && !tex_texels) || (btotal > 0 && !bump_texels)) return fail(PT_ERR_INVALID, "%s: null texels", who);
    if (total > (size_t)0x7fffffff || btotal > (size_t)0x7fffffff) return fail(PT_ERR_INVALID, "%s: %zu texels in all (at most 2^31 - 1)", who, std::max(total, btotal));
    if (n == 0) return PT_OK;
    std::vector<float> rec;
    std::vector<int32_t> type;
    bump_geoms(geoms, num_geoms, rec, type);
    const std::vector<float> quad = rgb_quads(tex_texels, total), pair = bump_pairs(bump_texels, btotal);
    ShadeRecords r(materials, num_materials, false, paths, isects, outside, n);
    const float *d_rec = r.in(rec.data(), rec.size());
    const int32_t *d_type = r.in(type.data(), type.size());
    const int32_t *d_hit = r.in(hit_geom, (size_t)n);
    const float4 *d_tex = (const float4 *)r.in(quad.data(), quad.size());
    const int2 *d_tab = r.in(tab.data(), tab.size());
    const ptd::bump_texel *d_bump = (const ptd::bump_texel *)r.in(pair.data(), pair.size());
    const int2 *d_btab = r.in(btab.data(), btab.size());
    if (!r.ok()) return probe_no_device(who);
    hipLaunchKernelGGL(k_probe_shade_scatter_bumped, r.grid(), dim3(64), 0, 0, iter, depth, r.mats, r.paths, r.isects, r.outside, n, deferred,
                       d_rec, d_type, d_hit, d_tex, d_tab, d_bump, d_btab);
    return r.finish();
}

int pt_environment_texel(const float *dirs, int count, int n, int32_t *index) {
    if (count < 0 || n < 1 || n > 1024 || (count > 0 && (!dirs || !index)))
        return fail(PT_ERR_INVALID, "pt_environment_texel: bad argument (count %d, n %d)", count, n);
    for (int i = 0; i < count; ++i) index[i] = ptd::env_texel(dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2], n);
    return PT_OK;
}

int pt_probe_environment(const float *texels, int n, const float *dirs, const float *throughput, int count, float *colour) {
    if (count < 0 || n < 0 || n > 1024 || (n > 0 && !texels) || (count > 0 && (!dirs || !throughput || !colour)))
        return fail(PT_ERR_INVALID, "pt_probe_environment: bad argument (count %d, n %d)", count, n);
    if (count == 0) return PT_OK;
    const std::vector<float> quad = rgb_quads(texels, (size_t)6 * (size_t)n * (size_t)n);
    ProbeBufs b;
    const float4 *d_tex = (const float4 *)b.in(quad.data(), quad.size());
    const float *d_dirs = b.in(dirs, 3 * (size_t)count);
    const float *d_thr = b.in(throughput, 3 * (size_t)count);
    float *d_col = b.out<float>(3 * (size_t)count);
    if (!b.ok()) return probe_no_device("pt_probe_environment");
    hipLaunchKernelGGL(k_probe_environment, dim3((unsigned)((count + 63) / 64)), dim3(64), 0, 0, d_tex, n, d_dirs, d_thr, count, d_col);
    HIPCHK(hipGetLastError());
    HIPCHK(b.fetch(colour, d_col, 3 * (size_t)count));
    HIPCHK(hipDeviceSynchronize());
    return PT_OK;
}

int pt_probe_tri_form(const pt_triangle *triangles, int count, float origin_bound, const float *origins, const float *directions, int n,
                      uint16_t *ray_slots, int32_t *ray_class, float *form) {
    if (count < 0 || n < 0 || (count > 0 && !triangles) || (n > 0 && (!origins || !directions)))
        return fail(PT_ERR_INVALID, "pt_probe_tri_form: bad argument");
    const int n64 = (count + 63) & ~63;
    if ((int64_t)n * std::max(n64, 32) > (1 << 28)) return fail(PT_ERR_INVALID, "pt_probe_tri_form: %d rays x %d records (at most 2^28)", n, n64);
    if (count == 0 || n == 0) return n64;
    std::vector<uint16_t> recs((size_t)n64 * 32);
    float frame[4];
    const int got = pt_tri_records(triangles, count, origin_bound, recs.data(), frame);   // upload_tri_bounds' own calls
    if (got != n64) return got < 0 ? got : fail(PT_ERR_INTERNAL, "pt_probe_tri_form: %d records, expected %d", got, n64);
    ProbeBufs b;
    const pt_half8 *d_rec = (const pt_half8 *)b.in(recs.data(), recs.size());
    const float *d_o = b.in(origins, 3 * (size_t)n);
    const float *d_d = b.in(directions, 3 * (size_t)n);
    _Float16 *d_slots = ray_slots ? b.out<_Float16>(32 * (size_t)n) : nullptr;
    int32_t *d_cls = ray_class ? b.out<int32_t>((size_t)n) : nullptr;
    float *d_form = form ? b.out<float>((size_t)n * n64) : nullptr;
    if (!b.ok()) return probe_no_device("pt_probe_tri_form");
    hipLaunchKernelGGL(k_probe_tri_form, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, 0, d_rec, n64, frame[0], frame[1], frame[2], frame[3],
                       origin_bound, d_o, d_d, n, d_slots, d_cls, d_form);
    HIPCHK(hipGetLastError());
    HIPCHK(b.fetch((_Float16 *)ray_slots, d_slots, 32 * (size_t)n));
    HIPCHK(b.fetch(ray_class, d_cls, (size_t)n));
    HIPCHK(b.fetch(form, d_form, (size_t)n * n64));
    HIPCHK(hipDeviceSynchronize());
    return n64;
}
