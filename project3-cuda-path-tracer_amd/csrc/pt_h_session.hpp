// pt_h_session.hpp -- one context's state (Renderer), error reporting, event profiling, small helpers
// (one of the host-side headers of libptmi355.so, included by ptmi355.hip -- the only translation unit -- in dependency order)
#pragma once

namespace {

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
constexpr size_t ERR_BYTES = 512;
char g_err[ERR_BYTES] = "";
// where fail() writes: the calling thread's buffer.  The host's thread uses g_err (pt_last_error); every worker thread
// of the multi-device layer (pt_multi.hpp) has its own, copied into g_err when its job fails.
thread_local char *t_err = g_err;

int fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(t_err, ERR_BYTES, fmt, ap);
    va_end(ap);
    return code;
}

#define HIPCHK(expr)                                                                            \
    do {                                                                                        \
        hipError_t e_ = (expr);                                                                 \
        if (e_ != hipSuccess)                                                                   \
            return fail(PT_ERR_DEVICE, "HIP error (%s:%d): %s: %s", __builtin_strrchr(__FILE__, '/') ? __builtin_strrchr(__FILE__, '/') + 1 : __FILE__, __LINE__, #expr, \
                        hipGetErrorString(e_));                                                 \
    } while (0)

// At most one cube map per material, in the device's `Texel`.  keep[m] / n[m]: material m's map as the caller gave it, RGB
// (the getters; both empty until the first map is set); d_texels: every map's texels back to back; d_tab: per material {offset
// in texels, n}; count: maps set.  The device's two are rebuilt whenever a map is set or removed (pt_h_state.hpp: cube_replace).
template <class Texel> struct CubeMaps {
    std::vector<std::vector<float>> keep;
    std::vector<int> n;
    Texel *d_texels = nullptr;
    int2 *d_tab = nullptr;
    int count = 0;
};

constexpr int OV_MAX_LANES = 8;
struct Renderer {
    bool live = false;
    pt_scene_desc desc{};
    pt_camera cam{};
    int trace_depth = 0;
    uint32_t flags = 0;
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    TileMap map{};
    int npix = 0;                 // full frame
    uint32_t cap = 0;             // pool capacity = max_batch * tile_pixels
    int max_batch = 1;
    float *pool_mem[2] = {nullptr, nullptr};
    Pool pool[2]{};
    int cur = 0;                  // pool holding the current live prefix
    float *isect_mem = nullptr;
    uint32_t *sort_table = nullptr;
    float *cache_mem = nullptr;   // first-hit table: Isect::FIRST_HIT_BYTES per pixel of the tile (PT_CACHE_FIRST, and every session whose bounce 0 can take the table form)
    bool cache_valid = false;     // ... holds R.cam's first hits (cleared by pt_set_camera; filled by the next bounce 0 that reads it)
    bool first_hit_enabled = true;    // PTMI355_FIRST_HIT=0: only PT_CACHE_FIRST sessions read the table (the A/B control)
    bool first_hit_refence = false;   // the batch being enqueued on a lane filled the table: the next one starts from enter_lanes' event
    bool first_two_enabled = true;    // PTMI355_FIRST_TWO=0: bounce 0 of the table form stays a launch of its own (the A/B control)
    uint64_t first_two_launches = 0;  // launches that did bounces 0 and 1 (k_bounce<MODE_FIRST2>) since pt_init (ptdbg_first_two)
    // the first-state table (pt_types.hpp: the FS_ kinds): filled with the first-hit table by the same
    // kernel, valid when it is (cache_valid).  Only sessions whose bounce 0 is fixed per pixel up to the diffuse draw have one:
    // no PT_GLOSSY, no refractive material (pt_init)
    float *state_mem = nullptr;       // first_state_bytes(tile_pixels)
    uint32_t *state_ended = nullptr;  // one word per 64 local pixels (tile_pixels % 64 == 0 only)
    bool first_state_enabled = true;  // PTMI355_FIRST_STATE=0: the launch of bounces 0 and 1 shades bounce 0 per sample (the A/B control)
    uint64_t first_state_launches = 0;   // launches of k_bounce<MODE_STATE2> since pt_init (ptdbg_first_state); each is also a first_two launch
    uint64_t first_hit_fills = 0, first_hit_launches = 0;  // k_cache_first launches / bounce-0 launches of the table form since pt_init (ptdbg_first_hit)
    Isect isect{};
    float *final_mem = nullptr;   // float4[cap]: {r, g, b, stamp} of the paths that ended with a non-zero colour, index = pid
    uint32_t fin_serial = 0;      // stamp of the current batch's entries (never 0; a wrap clears the buffer)
    float *image = nullptr;
    bool own_image = false;
    float *d_geoms = nullptr, *d_mats = nullptr, *d_tris = nullptr;
    float *d_cull = nullptr, *d_grec = nullptr;
    float *d_tri_bound = nullptr;  // every-triangle loop, stage 1: the triangles' 64-byte records for the matrix pipe (upload_tri_bounds)
    size_t tri_bound_words = 0;
    std::vector<float> grec_frames;   // per geom {g, 1 / Rm} of a mesh's records (device copy: geom record words G_INV + 7 .. + 10)
    uint32_t *d_ginfo = nullptr;
    double cull_eye_reach = 0.0;  // |camera position|_1 the cull boxes were made for
    std::vector<pt_geom> geoms_keep;   // host copies (pt_set_camera may have to remake the cull boxes)
    std::vector<pt_triangle> tris_keep;
    std::vector<pt_mesh> meshes_keep;
    std::vector<float> grec_keep;      // the geom records as uploaded (PT_MESH_BVH rewrites the meshes' words when the trees are rebuilt)
    bool scene_lds = true;        // gather records + materials staged in LDS (else read through the vector cache)
    SceneDev scene{};
    float4 *d_env = nullptr;               // pt_set_environment: the cube map on the device (BounceArgs::env), {r, g, b, 0} per texel
    int env_n = 0;                         // ... its texels per face edge; 0: none (the kernels without ENV are launched)
    std::vector<float> env_keep;           // ... and as the caller gave it (pt_get_environment)
    // PT_DIRECT_LIGHT: the light element table on the device (BounceArgs::lights, ptd::LIGHT_WORDS
    // dwords per element) and its size.  nlights > 0 only in a session that has the flag, is not PT_FAKE_SHADER and whose
    // scene has a cube or sphere that emits: such a session runs trace_depth + 1 bounces (session_bounces), a kernel each.
    float *d_lights = nullptr;
    int nlights = 0;
    // PT_DIRECT_SKY: the lamps' records as pt_init made them.  In a flagged session nlights CHANGES
    // when a map arrives or goes (pt_set_environment: + 1 for the sky's element, and the two tables behind the records)
    std::vector<float> lamp_rec;
    // PT_TEXTURES: the materials' cube textures, {r, g, b, 0} per texel, and their cube bump maps,
    // {da, db} per texel (section 6.22).  tex.count + bump.count > 0: the session launches the TEX forms of k_bounce, a kernel
    // per bounce.
    CubeMaps<float4> tex;
    CubeMaps<ptd::bump_texel> bump;
    // PT_SMOOTH_NORMALS: the per-vertex normals, 9 floats per triangle in the order of
    // pt_scene_desc::triangles -- vn_keep as the caller gave them (pt_get_vertex_normals), d_vnormals the device's copy.  Null /
    // empty: none set; otherwise the SMOOTH forms, a kernel per bounce.
    std::vector<float> vn_keep;
    float *d_vnormals = nullptr;
    size_t lds_bytes = 0;
    Control *ctl = nullptr;
    Persist *persist = nullptr;
    uint32_t *iter_counts = nullptr;       // k_iteration: traced counts [bounce][workgroup] (BounceArgs::iter_counts); one per lane
    size_t iter_counts_bytes = 0;
    HostStats *h_stats = nullptr, *d_stats = nullptr;   // page-locked, device-mapped: the last workgroup of a synchronous call's k_iteration writes pt_stats' numbers here
    bool want_host_stats = false;          // this call ends in collect_stats (pt_trace / pt_trace_batch)
    uint32_t host_stats_serial = 0;        // != 0: the batch just enqueued leaves its counts in h_stats under this serial
    bool self_gathered = false;            // the batch just enqueued did finalGather inside k_iteration (no k_gather)
    uint32_t *dir_mem = nullptr;  // per bounce: count[Wp], base[Wp+4]
    size_t dir_stride = 0;        // words per bounce
    int cur_dir = -1;             // bounce whose directory describes pool[cur] (-1: dense)
    uint32_t max_tiles = 0;
    size_t flag_words = 0;                   // mesh pre-pass: 64-bit flag words per parity (one bit per physical pool slot)
    size_t ctl_bytes = 0;         // Control, zeroed per batch
    int grid = 0;                 // persistent grid size
    int grid_iter = 0;            // k_iteration's own (its register budget differs from the bounce kernels'): the co-resident maximum
    int grid_iter_cur = 0;        // ... and what the batch just enqueued was launched with (iter_grid_for)
    int iter_tpw = 4;             // under the lanes k_iteration's grid is sized for this many tiles per wave (0: always the whole grid; PTMI355_ITER_TPW) ...
    int iter_wgs_per_cu_all = 15; // ... but not below this many workgroups per CU over all lanes together (PTMI355_ITER_WGS_ALL)
    bool ov_lanes_set = false;    // PTMI355_OVERLAP named a lane count
    int ov_streams = 2;           // launch streams the lanes share (lane k uses stream k % ov_streams); PTMI355_LANE_STREAMS
    int cus = 0;
    int grid_sort = 0;            // workgroups of the material-sort kernels (k_sort_hist / k_shade_sorted)
    bool sort_wave = true;        // <= 64 keys: k_shade_sorted_w (PTMI355_SORT_WAVE=0 forces the workgroup-wide kernel)
    int sort_runs = 1;            // runs of tiles per wave of the fused sort (k_bounce); PTMI355_SORT_RUNS
    int sort_keys = 0;            // > 0: PT_SORT_MATERIAL in its fused form -- survivors placed by material, K = sort_keys ranges per wave (pt_types.hpp: RangeDir)
    bool sorted_isects = false;   // the last bounce was shaded in material order (the intersection planes keep the order the bounce received)
    bool gen_fused = false;       // bounce 0 of the current batch generates its own rays
    bool gen_sort = false;        // ... in the sorted pipeline (k_intersect + k_shade_sorted_w), no k_raygen either
    Lens lens{0, 0.0f, 0.0f};     // PT_AA_JITTER / thin lens (pt_scene_desc, pt_set_lens)
    uint64_t whole_max_paths = 6000000;  // batches up to this many paths run as ONE launch (k_iteration); PTMI355_WHOLE_MAX
    uint64_t whole_max_host_paths = 16000000;   // ... one iteration with a page-locked host image: up to this many (PTMI355_WHOLE_MAX_HOST)
    bool whole = false;           // the current batch did
    // Batches whose caller does not wait for them overlap on the device (enqueue_batch): each runs on a LANE --
    // a launch stream of its own and its own set of the buffers a batch in flight owns
    struct Bufs {
        float *pool_mem[2]; Pool pool[2]; float *final_mem; Control *ctl; uint32_t *dir_mem;
        float4 *mesh_hit; unsigned long long *mesh_flags[2]; uint32_t *iter_counts;
    };
    struct Lane {
        hipStream_t stream = nullptr;
        Bufs b{};                                 // lane 0: the session's own
        hipEvent_t traced = nullptr, gathered = nullptr;
        bool gathered_valid = false;
        hipStream_t la_stream = nullptr;          // PT_LOOKAHEAD: its stream of the tracing compute units (ensure_la_masks)
    } lane[OV_MAX_LANES];
    Lane *lane_cur = nullptr;     // the lane whose buffers and stream currently stand in for the session's (while its batch is enqueued)
    hipStream_t lane_main = nullptr;   // ... and the session's launch stream meanwhile
    size_t pool_bytes = 0, final_bytes = 0, dir_bytes = 0, mesh_hit_bytes = 0;   // of one set (init_impl)
    int ov_lanes = 4;             // PTMI355_OVERLAP=n: n lanes (0: every batch on the launch stream); 4 measured best, 3 worst (profiles/r03/variants_overlap*.log)
    double ov_budget_gb = 64.0;   // PTMI355_OVERLAP_GB: HBM the extra lanes may take
    hipEvent_t ov_enter = nullptr;
    bool ov_ready = false;        // lanes allocated
    bool ov_enabled = true;
    bool ov_ok = false;           // this call does not wait for its own result (async entry points)
    bool ov_active = false;       // the last thing enqueued was an overlapped batch
    int ov_next = 0;
    // PT_LOOKAHEAD: windows of consecutive iterations traced ahead of pt_trace's caller (pt_h_api.hpp: la_*).  A ring of
    // LA_SLOTS windows, slot j on lane j (consecutive slots on alternating launch streams): la_cur is the window being
    // consumed, the slots after it hold the windows that follow it -- up to LA_AHEAD of them traced ahead, overlapping on
    // the two launch streams like asynchronous batches; `next` = the sample the next consecutive call consumes; a window is
    // only ever served to calls whose camera / depth / lens are byte-equal to what it was traced with.  Three ahead on four
    // lanes measured 0.066 ms per call against 0.070 for two (and 0.054 against 0.056 without a host image); six lanes with
    // four or five ahead: the same as three (profiles/r06/lookahead_ab_windows_ahead.txt).
    static constexpr int LA_SLOTS = 4, LA_AHEAD = 3;
    struct LaWindow {
        bool valid = false;       // enqueued and not yet consumed or discarded
        bool inflight = false;    // enqueued, and the launch stream has not been ordered behind its last launch yet
        int iter0 = 0, count = 0, next = 0;
        uint32_t stamp = 0;       // of its final colours
        pt_camera cam{}; int depth = 0; Lens lens{0, 0.0f, 0.0f};
        Control *ctl = nullptr;   // its lane's control block (statistics of the window)
        bool masked = false;      // traced on the lane's masked stream
    } la[LA_SLOTS];
    int la_cur = 0;               // the slot being consumed
    // Calls that write a host image: their gathers run on la_cus compute units of their own (la_gstream, CU-masked), the
    // windows on the others (Lane::la_stream, a persistent grid of grid_la workgroups) -- DESIGN 6.13.  0: never.
    int la_cus = 24, grid_la = 0, per_cu = 0;
    bool la_masks_ready = false, la_masks_failed = false;
    uint64_t la_masked_windows = 0, la_masked_calls = 0;
    bool la_masked_last = false;  // the last batch on a lane went to its masked stream (the next one on a plain stream orders itself behind the launch stream)
    hipStream_t la_gstream = nullptr;
    hipEvent_t la_rs_event = nullptr;
    bool la_tracing = false;      // the batch being enqueued is a window: no k_gather, only its counters (enqueue_end)
    uint64_t la_misses = 0, la_windows = 0, la_discards = 0;   // calls that had to trace their own window first / windows enqueued / windows thrown away
    // a tiled context (tile_count > 1): where its local pixels sit in the frame, for k_gather_one_tiled (la_tiles_ok: the
    // division magic for the strip span holds); la_shared_device: other contexts of this session trace on the same device,
    // so the CU masks are not taken (ensure_la_masks)
    TileGather la_tg{};
    bool la_tiles_ok = false, la_shared_device = false;
    Control *last_ctl = nullptr;  // the control block of the last batch (collect_stats)
    float *epi_host = nullptr;    // pt_trace: the caller's image, device-mapped, for k_iteration's own gather (this call only)
    bool epi_done = false;        // ... and k_iteration took it
    bool epi_direct_enabled = true;   // PTMI355_EPI_DIRECT=0: such launches keep the final-colour buffer and gather per wave at their end
    bool defer_enabled = true;    // PTMI355_DEFER_DIR=0: every scatter stores its direction (no PENDING_DIR slots; the A/B control)
    bool own_enabled = true;      // PTMI355_OWN_SURFACE=0: every bounce culls with the per-primitive row test (no OWN_MASK bits; the A/B control)
    bool own_form = false;        // the launch being enqueued is k_bounce's own-surface form (enqueue_bounce decides, launch_bounce_at reads)
    bool pool_own = false;        // pool[cur]'s pids carry OWN_MASK bits (pt_export_paths strips them)
    bool host_sparse_enabled = false; // PT_HOST_SPARSE (implied by PT_SHARED_IMAGE): only the pixels whose sum changed are written to a host image the launch wrote last
    uint64_t image_epoch = 0;     // bumped by everything that changes the accumulation buffer
    float *host_synced = nullptr; // the (device-mapped) host image that held exactly the buffer's content at epoch host_epoch
    uint64_t host_epoch = 0;
    bool epi_enabled = true;      // PTMI355_HOST_EPILOGUE=0: always copy after the iteration
    bool pin_enabled = true;      // PTMI355_PIN=0: never page-lock caller buffers (copies take the runtime's pageable path)
    int mesh_mode = MESH_NONE;    // MESH_TILES: every triangle per ray; MESH_BVH: PT_MESH_BVH culling
    float *d_bvh_nodes = nullptr, *d_bvh_tris = nullptr, *d_bvh_top = nullptr;
    std::vector<float> mesh_grids;           // per mesh: lo xyz, hi xyz of its box grid (contains every box of its tree)
    unsigned long long *d_cam_mask = nullptr;   // bounce-0 tile mask (BounceArgs::cam_mask)
    bool cam_mask_valid = false;
    unsigned long long *d_cull0 = nullptr;      // bounce-0 candidate primitives per camera tile (BounceArgs::cull0)
    uint32_t cull0_tiles = 0;                   // 0: not applicable (> 64 primitives, tile_pixels not a multiple of 64, switched off)
    int4 *d_bvh_meshes = nullptr;
    float4 *mesh_hit = nullptr;              // mesh pre-pass results (k_mesh), one per pool slot
    unsigned long long *mesh_flags[2] = {nullptr, nullptr};   // one flag per pool slot: "mesh_hit[slot] is valid" (bounce parity)
    bool mesh_marked = false;                // the last bounce flagged the next bounce's mesh candidates
    int grid_mesh = 0;
    pt_bvh_info bvh_info{};
    // host buffers the caller hands to pt_trace (scene->state.image): page-locked once so that the per-call copy of
    // the running sum (pathtrace.cu:389-390) runs at PCIe speed instead of through the runtime's staging
    struct HostReg { void *ptr; size_t bytes; void *dev; };   // dev: the device's address of the mapping (looked up once)
    std::vector<HostReg> host_regs;
    // PT_ASYNC_IMAGE: snapshot of the running sum per call (device), copied out on a second stream while the next
    // call traces
    float *snap[2] = {nullptr, nullptr};
    hipStream_t copy_stream = nullptr;
    hipEvent_t ev_snap[2] = {nullptr, nullptr}, ev_copied[2] = {nullptr, nullptr};
    uint64_t async_calls = 0;
    // PT_ASYNC_IMAGE through the launch's own host writes (pt_trace, one launch per iteration): completion events of such
    // launches, the event the NEXT asynchronous call waits for before it returns (a copy's or a launch's), and the last
    // copy-engine transfer a launch that writes the host buffer itself has to come after
    hipEvent_t ev_direct[2] = {nullptr, nullptr};
    int direct_k = 0;
    hipEvent_t async_prev = nullptr, dma_last = nullptr;
    bool async_direct_enabled = true;     // PTMI355_ASYNC_DIRECT=0: always snapshot + copy engine
    unsigned int *dbg_counts = nullptr;   // PTMI355_DBG_COUNTS=<words>: buffer for an instrumented kernel build's block counts (BounceArgs::dbg_counts)
    size_t dbg_words = 0;
    // pt_gbuffer / pt_denoise (pt_h_denoise.hpp): buffers of their own, allocated on first use.  The G-buffer is the one of
    // camera gb_cam and is kept until the camera differs; the filter's levels ping-pong between the two colour planes
    // (packed float3), dn_result = the plane the last pt_denoise left its result in.
    float4 *gb_mem = nullptr;     // gA[npix] {normal, t}, then gB[npix] {position, materialId}
    bool gb_valid = false;
    pt_camera gb_cam{};
    float *dn_plane[2] = {nullptr, nullptr};
    uint8_t *dn_rgba = nullptr;
    float *dn_result = nullptr;
    uint64_t dn_launches[3] = {0, 0, 0};   // k_gbuffer / k_atrous / k_denoise_mean launches since pt_init (ptdbg_denoise)
    // pt_set_denoise_albedo / pt_albedo: the switch, and the albedo plane (packed float3) of camera
    // alb_cam -- one per session, written by the ALB form of k_gbuffer, stale once pt_set_texture changes the table
    bool alb_on = false, alb_valid = false;
    float *alb_mem = nullptr;
    pt_camera alb_cam{};
    // pt_denoise_temporal (pt_h_denoise.hpp), allocated by the first temporal call.  `cur` = what the
    // last temporal call saw: its camera, its G-buffer (tp_gb: gb_mem or gb_alt -- when the camera changes while cur refers
    // to gb_mem, ensure_gbuffer swaps the two allocations instead of overwriting it), the blended colour tp_c[tp_k] and its
    // sample count tp_n[tp_k]; the other pair is what the next camera change blends into.  tp_hc / tp_hn: the history in the
    // grid of cur's camera, all zero whenever there is no cur.
    float4 *gb_alt = nullptr, *tp_gb = nullptr;
    bool tp_ready = false, tp_cur = false;
    pt_camera tp_cam{};
    float *tp_c[2] = {nullptr, nullptr}, *tp_n[2] = {nullptr, nullptr};
    int tp_k = 0;
    float *tp_hc = nullptr, *tp_hn = nullptr;
    uint64_t tp_launches[2] = {0, 0};      // k_reproject / k_temporal_blend launches since pt_init (ptdbg_temporal)
    // PT_MOMENTS / pt_denoise_variance (pt_h_denoise.hpp).  mom_mem: M1[npix] then M2[npix], the luminance
    // moments k_gather<true> keeps beside the running sum -- allocated by pt_init in a flagged session only (non-null = flagged).
    // The filter's buffers, allocated by its first call: vr_plane = the levels' ping-pong planes of {r, g, b, var} records,
    // vr_var0 = var_0 of the last call's input (pt_variance; vr_called: there was one), vr_out = the result (packed float3).
    float *mom_mem = nullptr;
    float4 *vr_plane[2] = {nullptr, nullptr};
    float *vr_var0 = nullptr, *vr_out = nullptr;
    bool vr_called = false;
    uint64_t vr_launches[2] = {0, 0};      // k_atrous_var / k_variance_mean launches since pt_init (ptdbg_variance)
    // pt_denoise_svgf (pt_h_denoise.hpp), allocated by its first call: a state of its own, not the temporal
    // call's.  `cur` = what the last call saw: its camera, a COPY of its G-buffer (sv_gb: ensure_gbuffer's two allocations belong to
    // pt_denoise_temporal), the blended colour sv_c, the normalised moments sv_u1 / sv_u2 and the sample count sv_n; sv_hc / sv_h1 /
    // sv_h2 / sv_hn: the history in the grid of cur's camera, all zero whenever there is no cur; sv_rec: the {c0, var_0} records level
    // 0 reads; sv_var0: var_0 as the levels received it (pt_svgf_variance).  The levels ping-pong through vr_plane into vr_out.
    bool sv_ready = false, sv_cur = false;
    pt_camera sv_cam{};
    float4 *sv_gb = nullptr, *sv_rec = nullptr;
    float *sv_c = nullptr, *sv_u1 = nullptr, *sv_u2 = nullptr, *sv_n = nullptr;
    float *sv_hc = nullptr, *sv_h1 = nullptr, *sv_h2 = nullptr, *sv_hn = nullptr, *sv_var0 = nullptr;
    uint64_t sv_launches[4] = {0, 0, 0, 0};   // k_reproject_svgf / k_svgf_blend / k_svgf_spatial launches, G-buffer copies (ptdbg_svgf)
    void *scratch = nullptr;      // export / import staging
    size_t scratch_bytes = 0;
    // stepping state
    int step_iter0 = 0, step_count = 0, step_depth = 0;
    bool in_step = false;
    pt_stats stats{};
    // optional per-kernel HIP-event timing
    bool profiling = false;
    std::vector<hipEvent_t> ev;       // pairs (start, stop)
    std::vector<int> ev_stage;        // stage of each recorded pair
    size_t ev_used = 0;               // pairs recorded since the last drain
    pt_profile prof{};
};

// One context = one device's renderer (the reference has one file-static set of buffers, pathtrace.cu:70-75).  A
// single-device session uses g_single on the caller's thread; a multi-device session (pt_multi.hpp) owns one context
// per device, each driven by its own host thread.  `R` is the context of the calling thread.
Renderer g_single;
thread_local Renderer *t_ctx = &g_single;
#define R (*t_ctx)

constexpr size_t EV_PAIRS = 2048;

int drain_events(void) {
    if (R.ev_used == 0) return PT_OK;
    HIPCHK(hipStreamSynchronize(R.stream));
    for (size_t k = 0; k < R.ev_used; ++k) {
        float ms = 0.0f;
        HIPCHK(hipEventElapsedTime(&ms, R.ev[2 * k], R.ev[2 * k + 1]));
        R.prof.ms[R.ev_stage[k] & 0xff] += (double)ms;
        R.prof.launches[R.ev_stage[k] & 0xff] += 1 + (R.ev_stage[k] >> 8);      // (a launch that did two bounces: StageTimer::two_bounces)
    }
    R.ev_used = 0;
    return PT_OK;
}

struct StageTimer {                  // brackets one launch when profiling is on
    bool on;
    size_t k;
    StageTimer(int stage) : on(false), k(0) {
        if (!R.profiling) return;
        if (R.ev_used >= EV_PAIRS && drain_events() != PT_OK) return;
        k = R.ev_used++;
        R.ev_stage[k] = stage;
        on = hipEventRecord(R.ev[2 * k], R.stream) == hipSuccess;
    }
    ~StageTimer() { if (on) (void)hipEventRecord(R.ev[2 * k + 1], R.stream); }
    // the bracketed launch does a batch's bounces 0 and 1 (enqueue_bounce): pt_profile::launches[PT_STAGE_BOUNCE] counts bounces, so
    // that a profile's count stays steps x bounces whichever plan the batch took
    void two_bounces() { if (on) R.ev_stage[k] |= 0x100; }
};

Pool carve_pool(float *mem, uint32_t cap) { return Pool{mem, cap}; }

// magic / shift for n / d, d >= 1, exact for all 32-bit n (checked on probes in pt_init)
void make_div_magic(uint32_t d, uint32_t *magic, uint32_t *shift) {
    if (d == 1) { *magic = 0; *shift = 0; return; }                     // handled separately in sample_of
    uint32_t L = 31;
    while (!((d >> L) & 1u)) --L;                                       // floor(log2 d)
    if ((d & (d - 1)) == 0) { *magic = 0; *shift = L - 1; return; }     // power of two: (n >> 1) >> (L - 1)
    const uint64_t num = 1ull << (32 + L);
    uint64_t m = num / d, rem = num % d;
    m += m;
    const uint64_t twice = rem + rem;
    if (twice >= d) m += 1;
    *magic = (uint32_t)(m + 1);
    *shift = L;
}

int tile_rows(int tile_index, int tile_count, int strip_rows, int H) {
    if (tile_count <= 1) return H;
    int rows = 0;
    for (int y = 0; y < H; ++y)
        if ((y / strip_rows) % tile_count == tile_index) rows++;
    return rows;
}

int ensure_isect(void) {
    if (R.isect_mem) return PT_OK;
    HIPCHK(hipMalloc(&R.isect_mem, (size_t)R.cap * 5 * 4));
    R.isect = Isect{R.isect_mem, R.cap};
    return PT_OK;
}

int ensure_scratch(size_t bytes) {
    if (bytes <= R.scratch_bytes) return PT_OK;
    if (R.scratch) (void)hipFree(R.scratch);
    R.scratch = nullptr; R.scratch_bytes = 0;
    HIPCHK(hipMalloc(&R.scratch, bytes));
    R.scratch_bytes = bytes;
    return PT_OK;
}

// bounces a batch of this session runs: traceDepth, and the final ray of PT_DIRECT_LIGHT behind them
int session_bounces(void) { return R.trace_depth + (R.nlights > 0 ? 1 : 0); }
// a session whose light count follows the environment map: PT_DIRECT_SKY (with PT_DIRECT_LIGHT, pt_init sees to that)
bool sky_session(void) { return (R.flags & PT_DIRECT_SKY) && (R.flags & PT_DIRECT_LIGHT) && !(R.flags & PT_FAKE_SHADER); }
// ... and the most bounces a batch of depth `trace_depth` can run in this session, whatever map comes later
int session_bounces_max(int trace_depth) { return trace_depth + ((R.nlights > 0 || sky_session()) ? 1 : 0); }

RangeDir tile_dir(int depth) {
    const uint32_t W = (uint32_t)R.grid * WAVES * (uint32_t)(R.sort_keys > 0 ? R.sort_runs : 1);     // runs of tiles
    const uint32_t nr = W * (uint32_t)std::max(1, R.sort_keys);
    if (depth < 0) return RangeDir{nullptr, W, nr};
    return RangeDir{R.dir_mem + (size_t)depth * R.dir_stride, W, nr};
}


}  // namespace
