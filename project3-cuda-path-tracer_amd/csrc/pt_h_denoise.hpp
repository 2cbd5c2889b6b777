// pt_h_denoise.hpp -- pt_gbuffer / pt_denoise / pt_denoised_device_image of ONE context (namespace one): the first-hit G-buffer of
// the current camera and the edge-avoiding A-trous filter of the running sum (kernels: pt_k_denoise.hpp);
// pt_denoise_temporal / pt_history / pt_history_reset: the same filter on the sum blended with what earlier cameras had
// accumulated, looked up through the two cameras' G-buffers
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

// the G-buffer of R.cam: computed once per camera, kept until the camera's bytes differ.  `albedo` (pt_albedo, the filters
// of a session with pt_set_denoise_albedo(1)): the albedo plane of R.cam as well -- made by the same
// launch (the ALB form of k_gbuffer, which rewrites the G-buffer of an unchanged camera in place with the values it holds),
// kept until the camera's bytes differ or pt_set_texture changes the session's table (alb_valid).
static int ensure_gbuffer(bool albedo = false) {
    if (!R.gb_mem) HIPCHK(hipMalloc((void **)&R.gb_mem, (size_t)R.npix * 2 * sizeof(float4)));
    if (albedo && !R.alb_mem) HIPCHK(hipMalloc((void **)&R.alb_mem, (size_t)R.npix * 3 * sizeof(float)));
    const bool same = memcmp(&R.gb_cam, &R.cam, sizeof R.cam) == 0;
    const bool need_alb = albedo && !(R.alb_valid && memcmp(&R.alb_cam, &R.cam, sizeof R.cam) == 0);
    if (R.gb_valid && same && !need_alb) return PT_OK;
    // the record of the last temporal call refers to this allocation and to another camera: it keeps it, the new camera's
    // G-buffer goes to the second allocation (which exists: only a temporal call sets tp_cur)
    if (!same && R.tp_cur && R.tp_gb == R.gb_mem) std::swap(R.gb_mem, R.gb_alt);
    float4 *gA = R.gb_mem, *gB = R.gb_mem + R.npix;
    const int blocks = std::min(R.grid, (R.npix + BLOCK - 1) / BLOCK);
    if (need_alb) {
        // tinted only while the session's bounce kernels are launched in their textured form (bounce_args, launch_k_bounce)
        const bool textured = R.tex.count > 0 && !(R.flags & PT_FAKE_SHADER);
        const GbAlbedo alb{R.alb_mem, textured ? (const int2 *)R.tex.d_tab : (const int2 *)nullptr,
                           textured ? (const float4 *)R.tex.d_texels : (const float4 *)nullptr};
        PT_MESH_DISPATCH(hipLaunchKernelGGL((k_gbuffer<MESH, SLDS, true>), dim3(blocks), dim3(BLOCK), R.lds_bytes, R.stream, gA, gB,
                                            R.scene, R.cam, R.map, alb));
    } else {
        const GbAlbedo alb{nullptr, nullptr, nullptr};
        PT_MESH_DISPATCH(hipLaunchKernelGGL((k_gbuffer<MESH, SLDS, false>), dim3(blocks), dim3(BLOCK), R.lds_bytes, R.stream, gA, gB,
                                            R.scene, R.cam, R.map, alb));
    }
    HIPCHK(hipGetLastError());
    R.dn_launches[0]++;
    R.gb_cam = R.cam; R.gb_valid = true;
    if (need_alb) { R.alb_cam = R.cam; R.alb_valid = true; }
    return PT_OK;
}

// level l of the filter: step 2^l, from the accumulation buffer (l = 0: the mean is formed as it is read) or the plane the
// level before wrote, into plane l & 1.  `c0` (l = 0 of a temporal call): the blended colours, read as they are.
// `dm` (a session with pt_set_denoise_albedo(1)): AT_DIV at level 0 -- the staged form divides by the
// albedo plane as it loads, a temporal call's c0 included (div = 1.0f) --, AT_MUL at the last level; the levels between
// are the launches of a session without the switch.  Still one launch per level.
static int launch_atrous(int l, float div, float sc2, float sn2, float sp2, uint8_t *rgba, const float *c0 = nullptr, int dm = 0) {
    const float4 *gA = R.gb_mem, *gB = R.gb_mem + R.npix;
    const dim3 grid((unsigned)((R.map.W + 63) / 64), (unsigned)((R.map.H + WAVES - 1) / WAVES));
    const int out = l & 1;
    const float *none = nullptr, *alb = R.alb_mem;
    if (l == 0 && (dm & AT_DIV)) {
        const float *src = c0 ? c0 : (const float *)R.image;
        const float d = c0 ? 1.0f : div;
        if (dm & AT_MUL)
            hipLaunchKernelGGL((k_atrous<true, AT_DIV | AT_MUL>), grid, dim3(BLOCK), 0, R.stream, src, gA, gB, R.dn_plane[out], rgba, R.map.W,
                               R.map.H, 1, d, sc2, sn2, sp2, alb);
        else
            hipLaunchKernelGGL((k_atrous<true, AT_DIV>), grid, dim3(BLOCK), 0, R.stream, src, gA, gB, R.dn_plane[out], rgba, R.map.W,
                               R.map.H, 1, d, sc2, sn2, sp2, alb);
    } else if (l == 0 && c0)
        hipLaunchKernelGGL(k_atrous<false>, grid, dim3(BLOCK), 0, R.stream, c0, gA, gB, R.dn_plane[out], rgba, R.map.W, R.map.H, 1, 1.0f,
                           sc2, sn2, sp2, none);
    else if (l == 0)
        hipLaunchKernelGGL(k_atrous<true>, grid, dim3(BLOCK), 0, R.stream, (const float *)R.image, gA, gB, R.dn_plane[out], rgba,
                           R.map.W, R.map.H, 1, div, sc2, sn2, sp2, none);
    else if (dm & AT_MUL)
        hipLaunchKernelGGL((k_atrous<false, AT_MUL>), grid, dim3(BLOCK), 0, R.stream, (const float *)R.dn_plane[out ^ 1], gA, gB,
                           R.dn_plane[out], rgba, R.map.W, R.map.H, 1 << l, 1.0f, sc2, sn2, sp2, alb);
    else
        hipLaunchKernelGGL(k_atrous<false>, grid, dim3(BLOCK), 0, R.stream, (const float *)R.dn_plane[out ^ 1], gA, gB, R.dn_plane[out],
                           rgba, R.map.W, R.map.H, 1 << l, 1.0f, sc2, sn2, sp2, none);
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

// the bits launch_atrous gets for level l of `levels` in a session whose switch is on
static int albedo_bits(int l, int levels) { return R.alb_on ? ((l == 0 ? AT_DIV : 0) | (l == levels - 1 ? AT_MUL : 0)) : 0; }

// pt_set_denoise_albedo / pt_albedo.  Like pt_gbuffer they read the session and change nothing in
// it: the switch is a word of the host's, the plane a buffer of its own behind everything enqueued on the launch stream.
int pt_set_denoise_albedo(int enable) {
    int rc = denoise_session_ok("pt_set_denoise_albedo");
    if (rc) return rc;
    if (enable != 0 && enable != 1) return fail(PT_ERR_INVALID, "pt_set_denoise_albedo: enable %d is neither 0 nor 1", enable);
    R.alb_on = enable == 1;
    return PT_OK;
}

int pt_albedo(float *rgb) {
    int rc = denoise_session_ok("pt_albedo");
    if (rc) return rc;
    rc = ensure_gbuffer(true);
    if (rc) return rc;
    if (rgb) HIPCHK(hipMemcpyAsync(rgb, R.alb_mem, (size_t)R.npix * 3 * sizeof(float), hipMemcpyDeviceToHost, R.stream));
    HIPCHK(hipStreamSynchronize(R.stream));
    return PT_OK;
}

// what pt_denoise and pt_denoise_temporal (`who`) refuse, in this order; the squares the kernels divide by
static int denoise_args_ok(const char *who, const pt_denoise_params *params, int iter, float sc2[10], float &sn2, float &sp2) {
    if (!R.live) return fail(PT_ERR_INVALID, "%s: not initialised", who);
    if (!params) return fail(PT_ERR_INVALID, "%s: params is null", who);
    const int levels = params->levels;
    if (levels < 0 || levels > 10) return fail(PT_ERR_INVALID, "%s: levels %d outside [0, 10]", who, levels);
    const float sig[3] = {params->sigma_color, params->sigma_normal, params->sigma_position};
    const char *names[3] = {"sigma_color", "sigma_normal", "sigma_position"};
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(sig[k]) || !(sig[k] > 0.0f))
            return fail(PT_ERR_INVALID, "%s: %s = %g is not a finite number > 0", who, names[k], (double)sig[k]);
    // sigma_color halves with every level (Dammertz; exact), the others stay.  Each square must be a normal number: 0 / 0 at
    // the centre tap otherwise.
    sn2 = sig[1] * sig[1]; sp2 = sig[2] * sig[2];
    if (!std::isnormal(sn2)) return fail(PT_ERR_INVALID, "%s: sigma_normal = %g: its square is not a normal binary32 number", who, (double)sig[1]);
    if (!std::isnormal(sp2)) return fail(PT_ERR_INVALID, "%s: sigma_position = %g: its square is not a normal binary32 number", who, (double)sig[2]);
    for (int l = 0; l < std::max(1, levels); ++l) {
        const float s = sig[0] * ldexpf(1.0f, -l);
        const float s2 = s * s;
        if (!std::isnormal(s2))
            return fail(PT_ERR_INVALID, "%s: sigma_color = %g: the square of sigma_color * 2^-%d is not a normal binary32 number", who, (double)sig[0], l);
        sc2[l] = s2;
    }
    if (iter < 1) return fail(PT_ERR_INVALID, "%s: iter %d < 1", who, iter);
    return denoise_session_ok(who);
}

int pt_denoise(const pt_denoise_params *params, int iter, float *host_rgb, uint8_t *host_rgba) {
    float sc2[10], sn2, sp2;
    int rc = denoise_args_ok("pt_denoise", params, iter, sc2, sn2, sp2);
    if (rc) return rc;
    const int levels = params->levels;
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
        rc = ensure_gbuffer(R.alb_on);
        if (rc) return rc;
        for (int l = 0; l < levels; ++l) {
            out = l & 1;
            rc = launch_atrous(l, div, sc2[l], sn2, sp2, l == levels - 1 ? rgba : (uint8_t *)nullptr, nullptr, albedo_bits(l, levels));
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

// ---- history across camera moves ----------------------------------------------------------------
// cur (camera `A`, G-buffer gb, colours C, sample counts N) reprojected into the grid of R.cam, whose G-buffer is R.gb_mem
static int launch_reproject(const pt_camera &A, const float4 *gb, const float *C, const float *N, const pt_temporal_params &tp) {
    const dim3 grid((unsigned)((R.map.W + 63) / 64), (unsigned)((R.map.H + WAVES - 1) / WAVES));
    hipLaunchKernelGGL(k_reproject, grid, dim3(BLOCK), 0, R.stream, (const float4 *)R.gb_mem, (const float4 *)(R.gb_mem + R.npix), gb,
                       gb + R.npix, C, N, R.scene.mats, R.scene.nmats, A, R.tp_hc, R.tp_hn, R.map.W, R.map.H, (float)tp.max_history,
                       tp.position_tolerance, tp.normal_tolerance * tp.normal_tolerance);
    HIPCHK(hipGetLastError());
    R.tp_launches[0]++;
    return PT_OK;
}

// the running sum blended with the history into C / N: one launch
static int launch_blend(float div, float *C, float *N, uint8_t *rgba) {
    const uint32_t n = (uint32_t)R.npix;
    if (((uintptr_t)R.image & 15) == 0)         // (a caller's accumulation buffer, pt_scene_desc::device_image, may sit anywhere)
        hipLaunchKernelGGL(k_temporal_blend<true>, dim3((n / 4 + 3 + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, R.stream, (const float *)R.image,
                           (const float *)R.tp_hc, (const float *)R.tp_hn, C, N, rgba, n, div);
    else
        hipLaunchKernelGGL(k_temporal_blend<false>, dim3((n + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, R.stream, (const float *)R.image,
                           (const float *)R.tp_hc, (const float *)R.tp_hn, C, N, rgba, n, div);
    HIPCHK(hipGetLastError());
    R.tp_launches[1]++;
    return PT_OK;
}

static int temporal_args_ok(const char *who, const pt_temporal_params *tp) {
    if (!tp) return fail(PT_ERR_INVALID, "%s: temporal is null", who);
    if (tp->max_history < 0 || tp->max_history > (1 << 20))
        return fail(PT_ERR_INVALID, "%s: max_history %d outside [0, %d]", who, tp->max_history, 1 << 20);
    const float tol[2] = {tp->position_tolerance, tp->normal_tolerance};
    const char *names[2] = {"position_tolerance", "normal_tolerance"};
    for (int k = 0; k < 2; ++k) {
        if (!std::isfinite(tol[k]) || !(tol[k] > 0.0f))
            return fail(PT_ERR_INVALID, "%s: %s = %g is not a finite number > 0", who, names[k], (double)tol[k]);
        if (!std::isnormal(tol[k] * tol[k]))
            return fail(PT_ERR_INVALID, "%s: %s = %g: its square is not a normal binary32 number", who, names[k], (double)tol[k]);
    }
    return PT_OK;
}

// the temporal call's buffers: the second G-buffer, two colour and two length planes, the history (80 bytes per pixel
// with the first G-buffer)
static int ensure_temporal(void) {
    if (R.tp_ready) return PT_OK;
    const size_t n = (size_t)R.npix;
    if (!R.gb_alt) HIPCHK(hipMalloc((void **)&R.gb_alt, n * 2 * sizeof(float4)));
    for (int k = 0; k < 2; ++k) {
        if (!R.tp_c[k]) HIPCHK(hipMalloc((void **)&R.tp_c[k], n * 3 * sizeof(float)));
        if (!R.tp_n[k]) HIPCHK(hipMalloc((void **)&R.tp_n[k], n * sizeof(float)));
    }
    if (!R.tp_hc) HIPCHK(hipMalloc((void **)&R.tp_hc, n * 3 * sizeof(float)));
    if (!R.tp_hn) HIPCHK(hipMalloc((void **)&R.tp_hn, n * sizeof(float)));
    HIPCHK(hipMemsetAsync(R.tp_hc, 0, n * 3 * sizeof(float), R.stream));
    HIPCHK(hipMemsetAsync(R.tp_hn, 0, n * sizeof(float), R.stream));
    R.tp_cur = false; R.tp_k = 0;
    R.tp_ready = true;
    return PT_OK;
}

int pt_denoise_temporal(const pt_denoise_params *params, const pt_temporal_params *temporal, int iter, float *host_rgb,
                        uint8_t *host_rgba) {
    float sc2[10], sn2, sp2;
    int rc = denoise_args_ok("pt_denoise_temporal", params, iter, sc2, sn2, sp2);
    if (rc) return rc;
    rc = temporal_args_ok("pt_denoise_temporal", temporal);
    if (rc) return rc;
    const int levels = params->levels;
    const size_t n = (size_t)R.npix;
    for (int k = 0; k < 2; ++k)
        if (!R.dn_plane[k]) HIPCHK(hipMalloc((void **)&R.dn_plane[k], n * 3 * sizeof(float)));
    if (host_rgba && !R.dn_rgba) HIPCHK(hipMalloc((void **)&R.dn_rgba, n * 4));
    uint8_t *rgba = host_rgba ? R.dn_rgba : (uint8_t *)nullptr;
    rc = ensure_temporal();
    if (rc) return rc;
    rc = ensure_gbuffer(R.alb_on && levels > 0);   // (a camera other than cur's: into the allocation cur does not refer to)
    if (rc) return rc;
    if (R.tp_cur && memcmp(&R.tp_cam, &R.cam, sizeof R.cam) != 0) {
        rc = launch_reproject(R.tp_cam, R.tp_gb, R.tp_c[R.tp_k], R.tp_n[R.tp_k], *temporal);
        if (rc) return rc;
        R.tp_k ^= 1;                            // the planes the history was read from stay whole until the next camera change
    }
    float *c0 = R.tp_c[R.tp_k];
    rc = launch_blend((float)iter, c0, R.tp_n[R.tp_k], levels == 0 ? rgba : (uint8_t *)nullptr);
    if (rc) return rc;
    R.tp_cur = true; R.tp_cam = R.cam; R.tp_gb = R.gb_mem;
    int out = 0;
    for (int l = 0; l < levels; ++l) {
        out = l & 1;
        rc = launch_atrous(l, 1.0f, sc2[l], sn2, sp2, l == levels - 1 ? rgba : (uint8_t *)nullptr, c0, albedo_bits(l, levels));
        if (rc) return rc;
    }
    R.dn_result = levels == 0 ? c0 : R.dn_plane[out];
    if (host_rgb) HIPCHK(hipMemcpyAsync(host_rgb, R.dn_result, n * 3 * sizeof(float), hipMemcpyDeviceToHost, R.stream));
    if (host_rgba) HIPCHK(hipMemcpyAsync(host_rgba, R.dn_rgba, n * 4, hipMemcpyDeviceToHost, R.stream));
    HIPCHK(hipStreamSynchronize(R.stream));
    return PT_OK;
}

int pt_history(float *rgb, float *length) {
    int rc = denoise_session_ok("pt_history");
    if (rc) return rc;
    if (!R.tp_ready) return fail(PT_ERR_INVALID, "pt_history: no pt_denoise_temporal call since pt_init");
    const size_t n = (size_t)R.npix;
    if (rgb) HIPCHK(hipMemcpyAsync(rgb, R.tp_hc, n * 3 * sizeof(float), hipMemcpyDeviceToHost, R.stream));
    if (length) HIPCHK(hipMemcpyAsync(length, R.tp_hn, n * sizeof(float), hipMemcpyDeviceToHost, R.stream));
    HIPCHK(hipStreamSynchronize(R.stream));
    return PT_OK;
}

int pt_history_reset(void) {
    int rc = denoise_session_ok("pt_history_reset");
    if (rc) return rc;
    if (!R.tp_ready) return PT_OK;              // nothing to forget
    const size_t n = (size_t)R.npix;
    HIPCHK(hipMemsetAsync(R.tp_hc, 0, n * 3 * sizeof(float), R.stream));
    HIPCHK(hipMemsetAsync(R.tp_hn, 0, n * sizeof(float), R.stream));
    HIPCHK(hipStreamSynchronize(R.stream));
    R.tp_cur = false; R.tp_gb = nullptr;
    return PT_OK;
}

// ---- the filter steered by per-pixel luminance moments (PT_MOMENTS) --------------------------------
// pt_denoise's contract: synchronous, on the launch stream behind everything enqueued, reads the session (running sum, the two
// moment planes, the G-buffer it shares with pt_denoise) and writes buffers of its own -- not pt_denoise's planes, not the
// temporal history --; no counter moves.  The albedo switch is not read.
static int variance_args_ok(const char *who, const pt_variance_params *params, int iter, float &sn2, float &sp2) {
    if (!R.live) return fail(PT_ERR_INVALID, "%s: not initialised", who);
    if (!params) return fail(PT_ERR_INVALID, "%s: params is null", who);
    const int levels = params->levels;
    if (levels < 0 || levels > 10) return fail(PT_ERR_INVALID, "%s: levels %d outside [0, 10]", who, levels);
    const float sig[3] = {params->sigma_luminance, params->sigma_normal, params->sigma_position};
    const char *names[3] = {"sigma_luminance", "sigma_normal", "sigma_position"};
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(sig[k]) || !(sig[k] > 0.0f))
            return fail(PT_ERR_INVALID, "%s: %s = %g is not a finite number > 0", who, names[k], (double)sig[k]);
    sn2 = sig[1] * sig[1]; sp2 = sig[2] * sig[2];
    if (!std::isnormal(sn2)) return fail(PT_ERR_INVALID, "%s: sigma_normal = %g: its square is not a normal binary32 number", who, (double)sig[1]);
    if (!std::isnormal(sp2)) return fail(PT_ERR_INVALID, "%s: sigma_position = %g: its square is not a normal binary32 number", who, (double)sig[2]);
    // the smallest divisor a tap meets is sigma_luminance * sqrt(2^-40): a normal number, or the centre tap is 0 / 0
    if (!std::isnormal(sig[0] * ldexpf(1.0f, -20)))
        return fail(PT_ERR_INVALID, "%s: sigma_luminance = %g: sigma_luminance * 2^-20 is not a normal binary32 number", who, (double)sig[0]);
    if (iter < 1) return fail(PT_ERR_INVALID, "%s: iter %d < 1", who, iter);
    const int rc = denoise_session_ok(who);
    if (rc) return rc;
    if (!R.mom_mem) return fail(PT_ERR_INVALID, "%s: the session was initialised without PT_MOMENTS", who);
    return PT_OK;
}

static int ensure_variance(bool rgba) {
    const size_t n = (size_t)R.npix;
    for (int k = 0; k < 2; ++k)
        if (!R.vr_plane[k]) HIPCHK(hipMalloc((void **)&R.vr_plane[k], n * sizeof(float4)));
    if (!R.vr_var0) HIPCHK(hipMalloc((void **)&R.vr_var0, n * sizeof(float)));
    if (!R.vr_out) HIPCHK(hipMalloc((void **)&R.vr_out, n * 3 * sizeof(float)));
    if (rgba && !R.dn_rgba) HIPCHK(hipMalloc((void **)&R.dn_rgba, n * 4));
    return PT_OK;
}

// level l of `levels`: step 2^l, from the sum and the moments (l = 0) or the plane the level before wrote, into plane l & 1 --
// the last one into vr_out (and `rgba`).  `c0` (l = 0 of pt_denoise_svgf): the blended {colour, var_0} records, read as they are.
static int launch_atrous_var(int l, int levels, float div, float sl, float sn2, float sp2, uint8_t *rgba, const float4 *c0 = nullptr) {
    const float4 *gA = R.gb_mem, *gB = R.gb_mem + R.npix;
    const dim3 grid((unsigned)((R.map.W + 63) / 64), (unsigned)((R.map.H + WAVES - 1) / WAVES));
    const bool last = l == levels - 1;
    float4 *out = R.vr_plane[l & 1];
    float *out3 = last ? R.vr_out : (float *)nullptr;
    const float vdiv = fmaxf(div - 1.0f, 1.0f);
    const float *m1 = R.mom_mem, *m2 = R.mom_mem + R.npix;
    if (l == 0 && c0)
        hipLaunchKernelGGL(k_atrous_var<false>, grid, dim3(BLOCK), 0, R.stream, (const float *)nullptr, m1, m2, c0, gA, gB, out,
                           (float *)nullptr, out3, last ? rgba : (uint8_t *)nullptr, R.map.W, R.map.H, 1, div, vdiv, sl, sn2, sp2);
    else if (l == 0)
        hipLaunchKernelGGL(k_atrous_var<true>, grid, dim3(BLOCK), 0, R.stream, (const float *)R.image, m1, m2, (const float4 *)nullptr, gA, gB,
                           out, R.vr_var0, out3, last ? rgba : (uint8_t *)nullptr, R.map.W, R.map.H, 1, div, vdiv, sl, sn2, sp2);
    else
        hipLaunchKernelGGL(k_atrous_var<false>, grid, dim3(BLOCK), 0, R.stream, (const float *)nullptr, m1, m2, (const float4 *)R.vr_plane[(l & 1) ^ 1],
                           gA, gB, out, (float *)nullptr, out3, last ? rgba : (uint8_t *)nullptr, R.map.W, R.map.H, 1 << l, div, vdiv, sl, sn2, sp2);
    HIPCHK(hipGetLastError());
    R.vr_launches[0]++;
    return PT_OK;
}

int pt_denoise_variance(const pt_variance_params *params, int iter, float *host_rgb, uint8_t *host_rgba) {
    float sn2, sp2;
    int rc = variance_args_ok("pt_denoise_variance", params, iter, sn2, sp2);
    if (rc) return rc;
    rc = ensure_variance(host_rgba != nullptr);
    if (rc) return rc;
    const int levels = params->levels;
    const size_t n = (size_t)R.npix;
    uint8_t *rgba = host_rgba ? R.dn_rgba : (uint8_t *)nullptr;
    const float div = (float)iter;
    if (levels == 0) {
        hipLaunchKernelGGL(k_variance_mean, dim3((unsigned)((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, R.stream, (const float *)R.image,
                           (const float *)R.mom_mem, (const float *)(R.mom_mem + R.npix), R.vr_out, R.vr_var0, rgba, (uint32_t)n, div,
                           fmaxf(div - 1.0f, 1.0f));
        HIPCHK(hipGetLastError());
        R.vr_launches[1]++;
    } else {
        rc = ensure_gbuffer();
        if (rc) return rc;
        for (int l = 0; l < levels; ++l) {
            rc = launch_atrous_var(l, levels, div, params->sigma_luminance, sn2, sp2, rgba);
            if (rc) return rc;
        }
    }
    R.vr_called = true;
    R.dn_result = R.vr_out;
    if (host_rgb) HIPCHK(hipMemcpyAsync(host_rgb, R.vr_out, n * 3 * sizeof(float), hipMemcpyDeviceToHost, R.stream));
    if (host_rgba) HIPCHK(hipMemcpyAsync(host_rgba, R.dn_rgba, n * 4, hipMemcpyDeviceToHost, R.stream));
    HIPCHK(hipStreamSynchronize(R.stream));
    return PT_OK;
}

int pt_variance(float *host_var) {
    int rc = denoise_session_ok("pt_variance");
    if (rc) return rc;
    if (!R.mom_mem) return fail(PT_ERR_INVALID, "pt_variance: the session was initialised without PT_MOMENTS");
    if (!R.vr_called) return fail(PT_ERR_INVALID, "pt_variance: no pt_denoise_variance call since pt_init");
    if (host_var) HIPCHK(hipMemcpyAsync(host_var, R.vr_var0, (size_t)R.npix * sizeof(float), hipMemcpyDeviceToHost, R.stream));
    HIPCHK(hipStreamSynchronize(R.stream));
    return PT_OK;
}

// ---- reprojected moments and the spatial variance fallback (pt_denoise_svgf) ------------------------
// pt_denoise_variance's contract, with a history of its own: cur's planes, a copy of cur's G-buffer, the history and the records
// level 0 reads (100 bytes per pixel) beside the levels' planes it shares with pt_denoise_variance.  ensure_gbuffer's two-allocation
// swap is not involved: whatever allocation the current camera's G-buffer is in, cur's copy is refreshed from it once per camera
// change, after the reprojection has read the old one.
static int ensure_svgf(void) {
    if (R.sv_ready) return PT_OK;
    const size_t n = (size_t)R.npix;
    if (!R.sv_gb) HIPCHK(hipMalloc((void **)&R.sv_gb, n * 2 * sizeof(float4)));
    if (!R.sv_rec) HIPCHK(hipMalloc((void **)&R.sv_rec, n * sizeof(float4)));
    for (float **p : {&R.sv_c, &R.sv_hc})
        if (!*p) HIPCHK(hipMalloc((void **)p, n * 3 * sizeof(float)));
    for (float **p : {&R.sv_u1, &R.sv_u2, &R.sv_n, &R.sv_h1, &R.sv_h2, &R.sv_hn, &R.sv_var0})
        if (!*p) HIPCHK(hipMalloc((void **)p, n * sizeof(float)));
    HIPCHK(hipMemsetAsync(R.sv_hc, 0, n * 3 * sizeof(float), R.stream));
    for (float *p : {R.sv_h1, R.sv_h2, R.sv_hn}) HIPCHK(hipMemsetAsync(p, 0, n * sizeof(float), R.stream));
    R.sv_cur = false;
    R.sv_ready = true;
    return PT_OK;
}

// cur (camera sv_cam, G-buffer sv_gb, planes sv_c / sv_u1 / sv_u2 / sv_n) reprojected into the grid of R.cam, whose G-buffer is R.gb_mem
static int launch_reproject_svgf(const pt_temporal_params &tp) {
    const dim3 grid((unsigned)((R.map.W + 63) / 64), (unsigned)((R.map.H + WAVES - 1) / WAVES));
    hipLaunchKernelGGL(k_reproject_svgf, grid, dim3(BLOCK), 0, R.stream, (const float4 *)R.gb_mem, (const float4 *)(R.gb_mem + R.npix),
                       (const float4 *)R.sv_gb, (const float4 *)(R.sv_gb + R.npix), (const float *)R.sv_c, (const float *)R.sv_u1,
                       (const float *)R.sv_u2, (const float *)R.sv_n, R.scene.mats, R.scene.nmats, R.sv_cam, R.sv_hc, R.sv_h1, R.sv_h2,
                       R.sv_hn, R.map.W, R.map.H, (float)tp.max_history, tp.position_tolerance, tp.normal_tolerance * tp.normal_tolerance);
    HIPCHK(hipGetLastError());
    R.sv_launches[0]++;
    return PT_OK;
}

static int launch_svgf_blend(float div, uint8_t *rgba) {
    const uint32_t n = (uint32_t)R.npix;
    const float *m1 = R.mom_mem, *m2 = R.mom_mem + R.npix;
    const SvgfBlend a{(const float *)R.image, m1, m2, R.sv_hc, R.sv_h1, R.sv_h2, R.sv_hn, R.sv_c, R.sv_u1, R.sv_u2, R.sv_n, R.sv_var0, R.sv_rec, rgba};
    // (a caller's accumulation buffer may sit anywhere; the second moment plane starts npix floats behind the first)
    if ((((uintptr_t)R.image | (uintptr_t)m1 | (uintptr_t)m2) & 15) == 0)
        hipLaunchKernelGGL(k_svgf_blend<true>, dim3((n / 4 + 3 + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, R.stream, a, n, div);
    else
        hipLaunchKernelGGL(k_svgf_blend<false>, dim3((n + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, R.stream, a, n, div);
    HIPCHK(hipGetLastError());
    R.sv_launches[1]++;
    return PT_OK;
}

static int launch_svgf_spatial(int below, float sn2, float sp2) {
    const dim3 grid((unsigned)((R.map.W + 63) / 64), (unsigned)((R.map.H + WAVES - 1) / WAVES));
    hipLaunchKernelGGL(k_svgf_spatial, grid, dim3(BLOCK), 0, R.stream, (const float *)R.sv_u1, (const float *)R.sv_u2, (const float *)R.sv_n,
                       (const float4 *)R.gb_mem, (const float4 *)(R.gb_mem + R.npix), R.sv_rec, R.sv_var0, R.map.W, R.map.H, (float)below, sn2, sp2);
    HIPCHK(hipGetLastError());
    R.sv_launches[2]++;
    return PT_OK;
}

static int svgf_args_ok(const char *who, const pt_variance_params *params, const pt_temporal_params *temporal, int spatial_below, int iter,
                        float &sn2, float &sp2) {
    int rc = variance_args_ok(who, params, iter, sn2, sp2);
    if (rc) return rc;
    rc = temporal_args_ok(who, temporal);
    if (rc) return rc;
    if (spatial_below < 0 || spatial_below > (1 << 20))
        return fail(PT_ERR_INVALID, "%s: spatial_below %d outside [0, %d]", who, spatial_below, 1 << 20);
    return PT_OK;
}

int pt_denoise_svgf(const pt_variance_params *params, const pt_temporal_params *temporal, int spatial_below, int iter, float *host_rgb,
                    uint8_t *host_rgba) {
    float sn2, sp2;
    int rc = svgf_args_ok("pt_denoise_svgf", params, temporal, spatial_below, iter, sn2, sp2);
    if (rc) return rc;
    rc = ensure_variance(host_rgba != nullptr);
    if (rc) return rc;
    rc = ensure_svgf();
    if (rc) return rc;
    const int levels = params->levels;
    const size_t n = (size_t)R.npix;
    uint8_t *rgba = host_rgba ? R.dn_rgba : (uint8_t *)nullptr;
    rc = ensure_gbuffer();
    if (rc) return rc;
    const bool changed = R.sv_cur && memcmp(&R.sv_cam, &R.cam, sizeof R.cam) != 0;
    if (changed) {
        rc = launch_reproject_svgf(*temporal);
        if (rc) return rc;
    }
    if (changed || !R.sv_cur) {                // cur's G-buffer from now on: this camera's
        HIPCHK(hipMemcpyAsync(R.sv_gb, R.gb_mem, n * 2 * sizeof(float4), hipMemcpyDeviceToDevice, R.stream));
        R.sv_launches[3]++;
    }
    rc = launch_svgf_blend((float)iter, levels == 0 ? rgba : (uint8_t *)nullptr);
    if (rc) return rc;
    R.sv_cur = true; R.sv_cam = R.cam;
    if (spatial_below > 0) {
        rc = launch_svgf_spatial(spatial_below, sn2, sp2);
        if (rc) return rc;
    }
    for (int l = 0; l < levels; ++l) {
        rc = launch_atrous_var(l, levels, (float)iter, params->sigma_luminance, sn2, sp2, rgba, R.sv_rec);
        if (rc) return rc;
    }
    R.dn_result = levels == 0 ? R.sv_c : R.vr_out;
    if (host_rgb) HIPCHK(hipMemcpyAsync(host_rgb, R.dn_result, n * 3 * sizeof(float), hipMemcpyDeviceToHost, R.stream));
    if (host_rgba) HIPCHK(hipMemcpyAsync(host_rgba, R.dn_rgba, n * 4, hipMemcpyDeviceToHost, R.stream));
    HIPCHK(hipStreamSynchronize(R.stream));
    return PT_OK;
}

int pt_svgf_history(float *rgb, float *u1, float *u2, float *length) {
    int rc = denoise_session_ok("pt_svgf_history");
    if (rc) return rc;
    if (!R.sv_ready) return fail(PT_ERR_INVALID, "pt_svgf_history: no pt_denoise_svgf call since pt_init");
    const size_t n = (size_t)R.npix;
    if (rgb) HIPCHK(hipMemcpyAsync(rgb, R.sv_hc, n * 3 * sizeof(float), hipMemcpyDeviceToHost, R.stream));
    if (u1) HIPCHK(hipMemcpyAsync(u1, R.sv_h1, n * sizeof(float), hipMemcpyDeviceToHost, R.stream));
    if (u2) HIPCHK(hipMemcpyAsync(u2, R.sv_h2, n * sizeof(float), hipMemcpyDeviceToHost, R.stream));
    if (length) HIPCHK(hipMemcpyAsync(length, R.sv_hn, n * sizeof(float), hipMemcpyDeviceToHost, R.stream));
    HIPCHK(hipStreamSynchronize(R.stream));
    return PT_OK;
}

int pt_svgf_variance(float *host_var) {
    int rc = denoise_session_ok("pt_svgf_variance");
    if (rc) return rc;
    if (!R.sv_ready) return fail(PT_ERR_INVALID, "pt_svgf_variance: no pt_denoise_svgf call since pt_init");
    if (host_var) HIPCHK(hipMemcpyAsync(host_var, R.sv_var0, (size_t)R.npix * sizeof(float), hipMemcpyDeviceToHost, R.stream));
    HIPCHK(hipStreamSynchronize(R.stream));
    return PT_OK;
}

int pt_svgf_reset(void) {
    int rc = denoise_session_ok("pt_svgf_reset");
    if (rc) return rc;
    if (!R.sv_ready) return PT_OK;              // nothing to forget
    const size_t n = (size_t)R.npix;
    HIPCHK(hipMemsetAsync(R.sv_hc, 0, n * 3 * sizeof(float), R.stream));
    for (float *p : {R.sv_h1, R.sv_h2, R.sv_hn}) HIPCHK(hipMemsetAsync(p, 0, n * sizeof(float), R.stream));
    HIPCHK(hipStreamSynchronize(R.stream));
    R.sv_cur = false;
    return PT_OK;
}

// diagnostics (ptdbg_svgf_times, not in include/ptmi355.h): device times of the call's launches, HIP events on the session's stream.
// Called where a call would reproject (cur at another camera exists): after one warm-up round, `reps` rounds of k_reproject_svgf,
// k_svgf_blend, k_svgf_spatial with every pixel below the threshold (1 << 20) and with none (0: every workgroup leaves), level 0
// from the records (k_atrous_var<false>, step 1), level 1 (step 2), and device-to-device copies of the bytes the three new kernels
// move (112, 88 and 52 per pixel; the spatial pass without its halo).  ms[rep * 9 + k] in that order.  The rounds' blends overwrite
// the planes cur stands for, so the history ends here: the call finishes with pt_svgf_reset.
int svgf_times(const pt_variance_params *params, const pt_temporal_params *temporal, int spatial_below, int iter, int reps, float *ms) {
    float sn2, sp2;
    int rc = svgf_args_ok("ptdbg_svgf_times", params, temporal, spatial_below, iter, sn2, sp2);
    if (rc) return rc;
    if (reps < 1 || !ms || params->levels < 2) return fail(PT_ERR_INVALID, "ptdbg_svgf_times: reps >= 1, levels >= 2 and a buffer");
    if (!R.sv_ready || !R.sv_cur || memcmp(&R.sv_cam, &R.cam, sizeof R.cam) == 0)
        return fail(PT_ERR_INVALID, "ptdbg_svgf_times: needs the record of a pt_denoise_svgf call at another camera");
    constexpr int items = 9;
    const size_t n = (size_t)R.npix;
    rc = ensure_variance(false);
    if (rc) return rc;
    rc = ensure_gbuffer();
    if (rc) return rc;
    const size_t copy_bytes[3] = {n * 112, n * 88, n * 52};
    void *src = nullptr, *dst = nullptr;
    std::vector<hipEvent_t> ev((size_t)2 * items, nullptr);
    auto cleanup = [&] {
        for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
        if (src) (void)hipFree(src);
        if (dst) (void)hipFree(dst);
    };
    auto run = [&]() -> int {
        HIPCHK(hipMalloc(&src, copy_bytes[0]));
        HIPCHK(hipMalloc(&dst, copy_bytes[0]));
        HIPCHK(hipMemsetAsync(src, 0, copy_bytes[0], R.stream));
        for (auto &e : ev) HIPCHK(hipEventCreate(&e));
        // the blend overwrites the planes the reprojection reads: a round's reprojection sees the round before's blend, which
        // changes values, not the work
        for (int rep = -1; rep < reps; ++rep) {
            int r = PT_OK;
            for (int k = 0; k < items && r == PT_OK; ++k) {
                HIPCHK(hipEventRecord(ev[2 * k], R.stream));
                switch (k) {
                case 0: r = launch_reproject_svgf(*temporal); break;
                case 1: r = launch_svgf_blend((float)iter, nullptr); break;
                case 2: r = launch_svgf_spatial(1 << 20, sn2, sp2); break;
                case 3: r = launch_svgf_spatial(0, sn2, sp2); break;
                case 4: r = launch_atrous_var(0, params->levels, (float)iter, params->sigma_luminance, sn2, sp2, nullptr, R.sv_rec); break;
                case 5: r = launch_atrous_var(1, params->levels, (float)iter, params->sigma_luminance, sn2, sp2, nullptr); break;
                default: HIPCHK(hipMemcpyAsync(dst, src, copy_bytes[k - 6], hipMemcpyDeviceToDevice, R.stream)); break;
                }
                HIPCHK(hipEventRecord(ev[2 * k + 1], R.stream));
            }
            if (r) return r;
            HIPCHK(hipStreamSynchronize(R.stream));
            if (rep < 0) continue;
            for (int k = 0; k < items; ++k) HIPCHK(hipEventElapsedTime(&ms[(size_t)rep * items + k], ev[2 * k], ev[2 * k + 1]));
        }
        return PT_OK;
    };
    rc = run();
    cleanup();
    if (rc) return rc;
    return one::pt_svgf_reset();
}

// diagnostics (ptdbg_variance_times, not in include/ptmi355.h): device times of every level of k_atrous_var, HIP events on the
// session's stream, denoise_times' method: one pt_denoise_variance as warm-up, then `reps` rounds; ms[rep * levels + l].  The
// result of the last round is that call's.
int variance_times(const pt_variance_params *params, int iter, int reps, float *ms) {
    int rc = one::pt_denoise_variance(params, iter, nullptr, nullptr);
    if (rc) return rc;
    if (reps < 1 || !ms || params->levels < 1) return fail(PT_ERR_INVALID, "ptdbg_variance_times: reps >= 1, levels >= 1 and a buffer");
    const int levels = params->levels;
    std::vector<hipEvent_t> ev((size_t)2 * levels, nullptr);
    auto run = [&]() -> int {
        for (auto &e : ev) HIPCHK(hipEventCreate(&e));
        const float sn2 = params->sigma_normal * params->sigma_normal, sp2 = params->sigma_position * params->sigma_position;
        for (int rep = 0; rep < reps; ++rep) {
            for (int l = 0; l < levels; ++l) {
                HIPCHK(hipEventRecord(ev[2 * l], R.stream));
                const int r = launch_atrous_var(l, levels, (float)iter, params->sigma_luminance, sn2, sp2, nullptr);
                if (r) return r;
                HIPCHK(hipEventRecord(ev[2 * l + 1], R.stream));
            }
            HIPCHK(hipStreamSynchronize(R.stream));
            for (int l = 0; l < levels; ++l) HIPCHK(hipEventElapsedTime(&ms[(size_t)rep * levels + l], ev[2 * l], ev[2 * l + 1]));
        }
        return PT_OK;
    };
    rc = run();
    for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
    return rc;
}

// diagnostics (ptdbg_denoise_times, not in include/ptmi355.h): device times of the filter's launches, HIP events on the
// session's stream.  After one pt_denoise(params, iter) as warm-up, `reps` rounds of: k_gbuffer (forced), every level of
// k_atrous, and a device-to-device hipMemcpyAsync of the 56 bytes per pixel one level moves (colour + two G-buffer planes
// in, colour out: the streaming yardstick).  ms[rep * (levels + 2) + k]: k = 0 the G-buffer, 1 .. levels the levels,
// levels + 1 the copy.  The result of the last round is a valid pt_denoise result.  In a session with
// pt_set_denoise_albedo(1) the rounds are the switched-on call's: the ALB form of k_gbuffer (forced), the first and last level
// in their demodulating forms, and 68 bytes per pixel in the copy (what such a first or last level moves).
int denoise_times(const pt_denoise_params *params, int iter, int reps, float *ms) {
    int rc = one::pt_denoise(params, iter, nullptr, nullptr);
    if (rc) return rc;
    if (reps < 1 || !ms || params->levels < 1) return fail(PT_ERR_INVALID, "ptdbg_denoise_times: reps >= 1, levels >= 1 and a buffer");
    const int levels = params->levels, items = levels + 2;
    const size_t copy_bytes = (size_t)R.npix * (R.alb_on ? 68 : 56);
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
            R.gb_valid = false; R.alb_valid = false;
            int r = ensure_gbuffer(R.alb_on);
            if (r) return r;
            HIPCHK(hipEventRecord(ev[1], R.stream));
            for (int l = 0; l < levels; ++l) {
                const float s = params->sigma_color * ldexpf(1.0f, -l);
                HIPCHK(hipEventRecord(ev[2 * (l + 1)], R.stream));
                r = launch_atrous(l, (float)iter, s * s, sn2, sp2, nullptr, nullptr, albedo_bits(l, levels));
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

// diagnostics (ptdbg_temporal_times, not in include/ptmi355.h): device times of the temporal call's launches, HIP events on
// the session's stream.  Called where a temporal call would reproject (a record of another camera exists): after one
// warm-up round, `reps` rounds of k_reproject, k_temporal_blend, level 0 from the blended plane (k_atrous<false>, step 1),
// level 0 from the running sum (k_atrous<true>, what pt_denoise runs), level 1 (k_atrous<false>, step 2) and
// device-to-device copies of the bytes the two new kernels move (96 and 44 per pixel).  ms[rep * 7 + k] in that order.
// Every launch writes what the pt_denoise_temporal call at the end writes again: the state afterwards is that call's.
int temporal_times(const pt_denoise_params *params, const pt_temporal_params *temporal, int iter, int reps, float *ms) {
    float sc2[10], sn2, sp2;
    int rc = denoise_args_ok("ptdbg_temporal_times", params, iter, sc2, sn2, sp2);
    if (rc) return rc;
    rc = temporal_args_ok("ptdbg_temporal_times", temporal);
    if (rc) return rc;
    if (reps < 1 || !ms || params->levels < 2) return fail(PT_ERR_INVALID, "ptdbg_temporal_times: reps >= 1, levels >= 2 and a buffer");
    if (!R.tp_ready || !R.tp_cur || memcmp(&R.tp_cam, &R.cam, sizeof R.cam) == 0)
        return fail(PT_ERR_INVALID, "ptdbg_temporal_times: needs the record of a temporal call at another camera");
    constexpr int items = 7;
    const size_t n = (size_t)R.npix;
    for (int k = 0; k < 2; ++k)
        if (!R.dn_plane[k]) HIPCHK(hipMalloc((void **)&R.dn_plane[k], n * 3 * sizeof(float)));
    rc = ensure_gbuffer();
    if (rc) return rc;
    const size_t copy_bytes[2] = {n * 96, n * 44};
    void *src = nullptr, *dst = nullptr;
    std::vector<hipEvent_t> ev((size_t)2 * items, nullptr);
    auto cleanup = [&] {
        for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
        if (src) (void)hipFree(src);
        if (dst) (void)hipFree(dst);
    };
    auto run = [&]() -> int {
        HIPCHK(hipMalloc(&src, copy_bytes[0]));
        HIPCHK(hipMalloc(&dst, copy_bytes[0]));
        HIPCHK(hipMemsetAsync(src, 0, copy_bytes[0], R.stream));
        for (auto &e : ev) HIPCHK(hipEventCreate(&e));
        float *c0 = R.tp_c[R.tp_k ^ 1], *n0 = R.tp_n[R.tp_k ^ 1];
        for (int rep = -1; rep < reps; ++rep) {
            int r = PT_OK;
            for (int k = 0; k < items && r == PT_OK; ++k) {
                HIPCHK(hipEventRecord(ev[2 * k], R.stream));
                switch (k) {
                case 0: r = launch_reproject(R.tp_cam, R.tp_gb, R.tp_c[R.tp_k], R.tp_n[R.tp_k], *temporal); break;
                case 1: r = launch_blend((float)iter, c0, n0, nullptr); break;
                case 2: r = launch_atrous(0, 1.0f, sc2[0], sn2, sp2, nullptr, c0); break;
                case 3: r = launch_atrous(0, (float)iter, sc2[0], sn2, sp2, nullptr); break;
                case 4: r = launch_atrous(1, 1.0f, sc2[1], sn2, sp2, nullptr); break;
                default: HIPCHK(hipMemcpyAsync(dst, src, copy_bytes[k - 5], hipMemcpyDeviceToDevice, R.stream)); break;
                }
                HIPCHK(hipEventRecord(ev[2 * k + 1], R.stream));
            }
            if (r) return r;
            HIPCHK(hipStreamSynchronize(R.stream));
            if (rep < 0) continue;
            for (int k = 0; k < items; ++k) HIPCHK(hipEventElapsedTime(&ms[(size_t)rep * items + k], ev[2 * k], ev[2 * k + 1]));
        }
        return PT_OK;
    };
    rc = run();
    cleanup();
    if (rc) return rc;
    return one::pt_denoise_temporal(params, temporal, iter, nullptr, nullptr);
}

}  // namespace one
