// pt_h_denoise.hpp -- pt_gbuffer / pt_denoise / pt_denoised_device_image of ONE context (namespace one): the first-hit G-buffer of
// the current camera and the edge-avoiding A-trous filter of the running sum (kernels: pt_k_denoise.hpp)
// (one of the host-side headers of libptmi355.so, included by ptmi355.hip -- the only translation unit -- in dependency order)
#pragma once

namespace one {

// Both calls READ the session and change nothing in it.  Their launches go to the session's launch stream, behind
// everything enqueued before them (the gathers of asynchronous batches are on that stream; a call served from a
// PT_LOOKAHEAD window has drained its gather's stream before it returned), read the scene records and the accumulation
// buffer, and write buffers of their own: no window is discarded -- the lanes go on tracing beside these launches --, no
// pool, intersection plane or staging buffer is touched, no counter moves.  Both end with the launch stream drained.
static int denoise_session_ok(const char *who) {
    if (!R.live) return fail(PT_ERR_INVALID, "%s: not initialised", who);
    if (R.map.tile_count > 1)
        return fail(PT_ERR_INVALID, "%s: this session holds one tile of the frame (tile_count = %d), not the frame", who, R.map.tile_count);
    return PT_OK;
}

// the G-buffer of R.cam: computed once per camera, kept until the camera's bytes differ
static int ensure_gbuffer(void) {
    if (!R.gb_mem) HIPCHK(hipMalloc((void **)&R.gb_mem, (size_t)R.npix * 2 * sizeof(float4)));
    if (R.gb_valid && memcmp(&R.gb_cam, &R.cam, sizeof R.cam) == 0) return PT_OK;
    float4 *gA = R.gb_mem, *gB = R.gb_mem + R.npix;
    const int blocks = std::min(R.grid, (R.npix + BLOCK - 1) / BLOCK);
    PT_MESH_DISPATCH(hipLaunchKernelGGL((k_gbuffer<MESH, SLDS>), dim3(blocks), dim3(BLOCK), R.lds_bytes, R.stream, gA, gB, R.scene,
                                        R.cam, R.map));
    HIPCHK(hipGetLastError());
    R.dn_launches[0]++;
    R.gb_cam = R.cam; R.gb_valid = true;
    return PT_OK;
}

// level l of the filter: step 2^l, from the accumulation buffer (l = 0: the mean is formed as it is read) or the plane the
// level before wrote, into plane l & 1
static int launch_atrous(int l, float div, float sc2, float sn2, float sp2, uint8_t *rgba) {
    const float4 *gA = R.gb_mem, *gB = R.gb_mem + R.npix;
    const dim3 grid((unsigned)((R.map.W + 63) / 64), (unsigned)((R.map.H + WAVES - 1) / WAVES));
    const int out = l & 1;
    if (l == 0)
        hipLaunchKernelGGL(k_atrous<true>, grid, dim3(BLOCK), 0, R.stream, (const float *)R.image, gA, gB, R.dn_plane[out], rgba,
                           R.map.W, R.map.H, 1, div, sc2, sn2, sp2);
    else
        hipLaunchKernelGGL(k_atrous<false>, grid, dim3(BLOCK), 0, R.stream, (const float *)R.dn_plane[out ^ 1], gA, gB, R.dn_plane[out],
                           rgba, R.map.W, R.map.H, 1 << l, 1.0f, sc2, sn2, sp2);
    HIPCHK(hipGetLastError());
    R.dn_launches[1]++;
    return PT_OK;
}

int pt_gbuffer(float *normals, float *positions, float *t, int32_t *material) {
    int rc = denoise_session_ok("pt_gbuffer");
    if (rc) return rc;
    rc = ensure_gbuffer();
    if (rc) return rc;
    const size_t n = (size_t)R.npix;
    std::vector<float4> host;
    try { host.resize(2 * n); } catch (...) { return fail(PT_ERR_NOMEM, "pt_gbuffer: no host memory for %zu pixels", n); }
    HIPCHK(hipMemcpyAsync(host.data(), R.gb_mem, 2 * n * sizeof(float4), hipMemcpyDeviceToHost, R.stream));
    HIPCHK(hipStreamSynchronize(R.stream));
    for (size_t i = 0; i < n; ++i) {
        const float4 a = host[i], b = host[n + i];
        if (normals) { normals[3 * i + 0] = a.x; normals[3 * i + 1] = a.y; normals[3 * i + 2] = a.z; }
        if (t) t[i] = a.w;
        if (positions) { positions[3 * i + 0] = b.x; positions[3 * i + 1] = b.y; positions[3 * i + 2] = b.z; }
        if (material) memcpy(&material[i], &b.w, 4);
    }
    return PT_OK;
}

int pt_denoise(const pt_denoise_params *params, int iter, float *host_rgb, uint8_t *host_rgba) {
    if (!R.live) return fail(PT_ERR_INVALID, "pt_denoise: not initialised");
    if (!params) return fail(PT_ERR_INVALID, "pt_denoise: params is null");
    const int levels = params->levels;
    if (levels < 0 || levels > 10) return fail(PT_ERR_INVALID, "pt_denoise: levels %d outside [0, 10]", levels);
    const float sig[3] = {params->sigma_color, params->sigma_normal, params->sigma_position};
    const char *names[3] = {"sigma_color", "sigma_normal", "sigma_position"};
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(sig[k]) || !(sig[k] > 0.0f))
            return fail(PT_ERR_INVALID, "pt_denoise: %s = %g is not a finite number > 0", names[k], (double)sig[k]);
    // the squares the kernels divide by: sigma_color halves with every level (Dammertz; exact), the others stay.  Each must
    // be a normal number: 0 / 0 at the centre tap otherwise.
    float sc2[10];
    const float sn2 = sig[1] * sig[1], sp2 = sig[2] * sig[2];
    if (!std::isnormal(sn2)) return fail(PT_ERR_INVALID, "pt_denoise: sigma_normal = %g: its square is not a normal binary32 number", (double)sig[1]);
    if (!std::isnormal(sp2)) return fail(PT_ERR_INVALID, "pt_denoise: sigma_position = %g: its square is not a normal binary32 number", (double)sig[2]);
    for (int l = 0; l < std::max(1, levels); ++l) {
        const float s = sig[0] * ldexpf(1.0f, -l);
        const float s2 = s * s;
        if (!std::isnormal(s2))
            return fail(PT_ERR_INVALID, "pt_denoise: sigma_color = %g: the square of sigma_color * 2^-%d is not a normal binary32 number", (double)sig[0], l);
        sc2[l] = s2;
    }
    if (iter < 1) return fail(PT_ERR_INVALID, "pt_denoise: iter %d < 1", iter);
    int rc = denoise_session_ok("pt_denoise");
    if (rc) return rc;
    const size_t n = (size_t)R.npix;
    for (int k = 0; k < 2; ++k)
        if (!R.dn_plane[k]) HIPCHK(hipMalloc((void **)&R.dn_plane[k], n * 3 * sizeof(float)));
    if (host_rgba && !R.dn_rgba) HIPCHK(hipMalloc((void **)&R.dn_rgba, n * 4));
    uint8_t *rgba = host_rgba ? R.dn_rgba : (uint8_t *)nullptr;
    const float div = (float)iter;
    int out = 0;
    if (levels == 0) {
        hipLaunchKernelGGL(k_denoise_mean, dim3((unsigned)((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, R.stream, (const float *)R.image,
                           R.dn_plane[0], rgba, (uint32_t)n, div);
        HIPCHK(hipGetLastError());
        R.dn_launches[2]++;
    } else {
        rc = ensure_gbuffer();
        if (rc) return rc;
        for (int l = 0; l < levels; ++l) {
            out = l & 1;
            rc = launch_atrous(l, div, sc2[l], sn2, sp2, l == levels - 1 ? rgba : (uint8_t *)nullptr);
            if (rc) return rc;
        }
    }
    R.dn_result = R.dn_plane[out];
    if (host_rgb) HIPCHK(hipMemcpyAsync(host_rgb, R.dn_result, n * 3 * sizeof(float), hipMemcpyDeviceToHost, R.stream));
    if (host_rgba) HIPCHK(hipMemcpyAsync(host_rgba, R.dn_rgba, n * 4, hipMemcpyDeviceToHost, R.stream));
    HIPCHK(hipStreamSynchronize(R.stream));
    return PT_OK;
}

float *pt_denoised_device_image(void) { return R.live ? R.dn_result : nullptr; }

// diagnostics (ptdbg_denoise_times, not in include/ptmi355.h): device times of the filter's launches, HIP events on the
// session's stream.  After one pt_denoise(params, iter) as warm-up, `reps` rounds of: k_gbuffer (forced), every level of
// k_atrous, and a device-to-device hipMemcpyAsync of the 56 bytes per pixel one level moves (colour + two G-buffer planes
// in, colour out: the streaming yardstick).  ms[rep * (levels + 2) + k]: k = 0 the G-buffer, 1 .. levels the levels,
// levels + 1 the copy.  The result of the last round is a valid pt_denoise result.
int denoise_times(const pt_denoise_params *params, int iter, int reps, float *ms) {
    int rc = one::pt_denoise(params, iter, nullptr, nullptr);
    if (rc) return rc;
    if (reps < 1 || !ms || params->levels < 1) return fail(PT_ERR_INVALID, "ptdbg_denoise_times: reps >= 1, levels >= 1 and a buffer");
    const int levels = params->levels, items = levels + 2;
    const size_t copy_bytes = (size_t)R.npix * 56;
    void *src = nullptr, *dst = nullptr;
    std::vector<hipEvent_t> ev((size_t)2 * items, nullptr);
    auto cleanup = [&] {
        for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
        if (src) (void)hipFree(src);
        if (dst) (void)hipFree(dst);
    };
    auto run = [&]() -> int {
        HIPCHK(hipMalloc(&src, copy_bytes));
        HIPCHK(hipMalloc(&dst, copy_bytes));
        HIPCHK(hipMemsetAsync(src, 0, copy_bytes, R.stream));
        for (auto &e : ev) HIPCHK(hipEventCreate(&e));
        const float sn2 = params->sigma_normal * params->sigma_normal, sp2 = params->sigma_position * params->sigma_position;
        for (int rep = -1; rep < reps; ++rep) {              // (-1: the copy's warm-up)
            HIPCHK(hipEventRecord(ev[0], R.stream));
            R.gb_valid = false;
            int r = ensure_gbuffer();
            if (r) return r;
            HIPCHK(hipEventRecord(ev[1], R.stream));
            for (int l = 0; l < levels; ++l) {
                const float s = params->sigma_color * ldexpf(1.0f, -l);
                HIPCHK(hipEventRecord(ev[2 * (l + 1)], R.stream));
                r = launch_atrous(l, (float)iter, s * s, sn2, sp2, nullptr);
                if (r) return r;
                HIPCHK(hipEventRecord(ev[2 * (l + 1) + 1], R.stream));
            }
            HIPCHK(hipEventRecord(ev[2 * (levels + 1)], R.stream));
            HIPCHK(hipMemcpyAsync(dst, src, copy_bytes, hipMemcpyDeviceToDevice, R.stream));
            HIPCHK(hipEventRecord(ev[2 * (levels + 1) + 1], R.stream));
            HIPCHK(hipStreamSynchronize(R.stream));
            if (rep < 0) continue;
            for (int k = 0; k < items; ++k) HIPCHK(hipEventElapsedTime(&ms[(size_t)rep * items + k], ev[2 * k], ev[2 * k + 1]));
        }
        return PT_OK;
    };
    rc = run();
    cleanup();
    return rc;
}

}  // namespace one
