// ptbench.cpp -- headless host: the reference's main.cpp / runCuda() loop without GLFW
// (src/main.cpp:33-76,101-147): load the scene, recompute the camera, pathtraceFree();
// pathtraceInit(); pathtrace() x ITERATIONS; saveImage(); pathtraceFree().
//
//   ptbench SCENEFILE.txt [--iters N] [--batch B] [--out BASENAME] [--sort] [--no-compact]
//           [--cache-first] [--bvh] [--aa] [--lens RADIUS FOCAL] [--pfm] [--device D] [--tile R/K] [--strip-rows S]
//           [--gpus K | --devices D0,D1,...] [--save-sum] [--resume SUMFILE.pfm [--start N]]
//           [--per-call [--warmup W] [--no-lookahead]] [--denoise LEVELS,SC,SN,SP] [--move DX,DY,DZ,ITERS] [--temporal CAP,TOL_P,TOL_N]
//           [--sky N,ZR,ZG,ZB,HR,HG,HB,GR,GG,GB] [--sun X,Y,Z,COS,R,G,B] [--glossy] [--direct] [--direct-sky] [--textures] [--albedo]
//           [--smooth] [--variance LEVELS,SL,SN,SP] [--svgf LEVELS,SL,SN,SP[,SPATIAL_BELOW]]
//
// --svgf LEVELS,SL,SN,SP[,SPATIAL_BELOW]: the session is initialised with PT_MOMENTS and, after the last iteration, pt_denoise_svgf
// (--variance's filter on colour and moments blended with the history, a 7 x 7 spatial variance estimate for pixels with fewer than
// SPATIAL_BELOW samples, default 4; include/ptmi355.h) writes BASE.<N>samp.svgf.png beside --variance's
// picture.  With --move it also writes BASE.moved.<ITERS>samp.svgf.png: the moved view filtered with the history of the first view.
// max_history and the two tolerances are --temporal's (default 64,0.1,0.1), the values --move passes to pt_denoise_temporal.  Not
// with --resume.
//
// --smooth: PT_SMOOTH_NORMALS -- the `vn` normals of the scene's mesh files (pthost.h: pth_scene_vertex_normals) are uploaded with
// pt_set_vertex_normals after pathtraceInit; mesh hits are shaded about the interpolated normal (include/ptmi355.h, DESIGN.md
// section 6.26).  scenes/cornell_smooth.txt.  Without the switch the normals are loaded and ignored.
//
// --albedo (needs --denoise): pt_set_denoise_albedo(1) before the first filtered picture -- every one of them, the --move /
// --temporal ones included, is filtered as colour / first-hit albedo and multiplied back (include/ptmi355.h, DESIGN.md section
// 6.20), which keeps the texels of --textures apart where the colour stop alone cannot.
//
// --textures: PT_TEXTURES -- the cube textures the scene's TEXTURE blocks declare (pthost.h: pth_scene_texture) are uploaded with
// pt_set_texture after pathtraceInit; each multiplies its material's colour on spheres and cubes (include/ptmi355.h, DESIGN.md
// section 6.19).  scenes/cornell_textured.txt.  The bump maps of its BUMPMAP blocks go up with pt_set_bump_map the same way (DESIGN.md
// section 6.22; scenes/cornell_bumped.txt).  Without the switch the blocks are loaded and ignored.
//
// --direct: PT_DIRECT_LIGHT -- the last bounce of a path that hits a diffuse surface aims a final ray at a sampled point of an
// emissive cube or sphere (DEPTH + 1 bounces; include/ptmi355.h).  scenes/cornell_two_lamps.txt.
//
// --direct-sky: PT_DIRECT_LIGHT | PT_DIRECT_SKY -- the environment map (--sky) is one more light element of that sampler, and a
// final ray aimed at it scores where it leaves the scene.  scenes/open_sky_sun.txt.
// --sun X,Y,Z,COS,R,G,B (needs --sky): every texel of the baked map whose centre direction c has dot(c, (X,Y,Z) / |(X,Y,Z)|) >= COS
// is replaced by (R, G, B) -- float64, operation for operation what binding.sun_on_cubemap does (the same texels bit for bit).
//
// --glossy: PT_GLOSSY -- a mirror or dielectric whose material has SPECEX > 0 scatters about a sampled microfacet normal (a GGX
// lobe of alpha^2 = 2 / (SPECEX + 2); include/ptmi355.h).  Without it SPECEX is ignored (scenes/cornell_glossy.txt then renders
// as scenes/cornell.txt).
//
// --sky N,ZR,ZG,ZB,HR,HG,HB,GR,GG,GB: environment lighting (pt_set_environment) from a gradient baked here into a cube map of
// N x N texels per face: horizon + (zenith - horizon) * max(y, 0) + (ground - horizon) * max(-y, 0) at the texel centres, y = the
// unit direction's second component -- float64 rounded to float32 once, operation for operation what binding.gradient_cubemap
// bakes (the same texels bit for bit).  Set after pathtraceInit, before the first iteration; rays that leave the scene read it.
//
// --denoise LEVELS,SC,SN,SP: after the last iteration, the edge-avoiding A-trous filter (pt_denoise: LEVELS levels, sigmas
// of colour / normal / position) of the accumulated image; BASE.<N>samp.denoised.png is written beside the image through the
// same saveImage pipeline (clamp, x255, truncate -- on the denoised mean), and one line reports the filter's time.
//
// --variance LEVELS,SL,SN,SP: the session is initialised with PT_MOMENTS and, after the last iteration, the filter steered by the
// pixels' own measured noise (pt_denoise_variance: LEVELS levels, sigmas of luminance -- in standard deviations -- / normal /
// position) writes BASE.<N>samp.variance.png beside --denoise's picture, the same way; one line reports its time.  Not with
// --resume: a saved sum does not carry the moments.
//
// --move DX,DY,DZ,ITERS (needs --denoise): what an interactive host does when the camera moves.  After the render and its
// denoised picture: one pt_denoise_temporal on the finished view (it becomes the history), position and lookAt translated by
// (DX, DY, DZ), pt_set_camera, pt_clear_image, ITERS iterations, and three pictures of the moved view: BASE.moved.<ITERS>samp.png
// (the mean), ....denoised.png (pt_denoise) and ....temporal.png (pt_denoise_temporal: the history blended in, the same filter);
// one line reports the times.  --temporal CAP,TOL_P,TOL_N: max_history and the position / normal tolerances (default 64,0.1,0.1).
//
// --batch B: iterations per launch sequence (default: up to 64 and ~40 M paths, as the shim sizes its windows; 1 = one
// pathtrace() per iteration); every batch but the last is enqueued without waiting, so consecutive batches overlap on the
// device.  The image is the same bit for bit whatever B.
//
// --save-sum / --resume: a render across several runs (C5's 5000 spp across GPU leases).  The running sum is the whole
// state the reference carries from one iteration to the next (dev_image, pathtrace.cu:71,84,389): --save-sum writes it
// raw (BASE.<N>samp.sum.pfm, exact), --resume loads it (pt_set_image) and continues with iteration N + 1 (N from
// --start or from the "<N>samp" of the file name) up to --iters: bit for bit the image of the uninterrupted run.
//
// --gpus K / --devices LIST: ONE process renders the frame on several GPUs: the library tiles it over the devices
// (interleaved strips of S rows), traces every tile on its own host thread and gathers the tiles' sums onto the first
// device over RCCL after every call (include/ptmi355.h: pt_scene_desc::devices); the image is the single-GPU image.
//
// --tile R/K: this process renders only tile R of K (the rows y with (y / S) % K == R, global pixelIndex and RNG
// keys unchanged), so K processes -- one per GPU, --device each -- render one frame between them; the other rows
// of its image stay zero and the K raw sums (--pfm) add up, exactly, to the single-process image.
//
// --per-call: the reference's host pattern as the drop-in shim runs it -- ONE pt_trace per iteration, every call handing over
// the page-locked host image, with the shim's flags (PT_COMPACT | PT_PIN_IMAGE | PT_HOST_SPARSE | PT_LOOKAHEAD, max_batch by the
// shim's rule; --no-lookahead drops PT_LOOKAHEAD).  Each call is timed on the host clock (pt_trace returns with the image
// complete); after W warm-up calls (default 64) it prints the median and mean ms per call and Grays/s = rays per iteration
// (pt_get_stats over the whole run) over the MEAN call -- the calls that start a window wait for it, so the median alone
// overstates what a run of calls delivers.  Works with --devices / --gpus.
//
// Links libptmi355.so (the HIP library) and host/pthost.cpp.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "pthost.h"

int main(int argc, char **argv) {
    if (argc < 2) {
        printf("Usage: %s SCENEFILE.txt [--iters N] [--batch B] [--out BASE] [--sort] [--no-compact] [--cache-first] "
               "[--bvh] [--aa] [--lens RADIUS FOCAL] [--pfm] [--device D] [--tile R/K] [--strip-rows S] "
               "[--gpus K | --devices D0,D1,...] [--save-sum] [--resume SUMFILE.pfm [--start N]] "
               "[--per-call [--warmup W] [--no-lookahead]] [--denoise LEVELS,SC,SN,SP] [--move DX,DY,DZ,ITERS] "
               "[--temporal CAP,TOL_P,TOL_N] [--sky N,ZR,ZG,ZB,HR,HG,HB,GR,GG,GB] [--sun X,Y,Z,COS,R,G,B] [--glossy] [--direct] [--direct-sky] [--textures] [--albedo] [--smooth] "
               "[--variance LEVELS,SL,SN,SP] [--svgf LEVELS,SL,SN,SP[,SPATIAL_BELOW]] (history: --temporal's values, default 64,0.1,0.1)\n", argv[0]);
        return 1;
    }
    int iters = -1, batch = 0, device = 0, tile_index = 0, tile_count = 1, strip_rows = 8;
    unsigned flags = PT_COMPACT | PT_PIN_IMAGE | PT_HOST_SPARSE;      // `image` below lives until pt_free and is only read here
    bool pfm = false, save_sum = false, per_call = false, lookahead = true;
    int warmup = 64;
    bool denoise = false, albedo = false;
    pt_denoise_params dn = {0, 0.0f, 0.0f, 0.0f};
    bool variance = false;
    pt_variance_params vr = {0, 0.0f, 0.0f, 0.0f};
    bool svgf = false;
    pt_variance_params sv = {0, 0.0f, 0.0f, 0.0f};
    int spatial_below = 4;
    bool move = false;
    float move_by[3] = {0.0f, 0.0f, 0.0f};
    int move_iters = 0;
    pt_temporal_params tp = {64, 0.1f, 0.1f};
    int sky_n = 0;
    double sky[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};          // zenith, horizon, ground
    bool sun = false;
    double sun_v[7] = {0, 0, 0, 0, 0, 0, 0};              // direction, cosine of the half angle, colour
    std::string resume;
    int start = -1;
    float lens_radius = 0.0f, focal_distance = 0.0f;
    std::string out;
    std::vector<int32_t> devices;
    for (int i = 2; i < argc; ++i) {
        std::string a = argv[i];
        if (a == "--iters" && i + 1 < argc) iters = atoi(argv[++i]);
        else if (a == "--batch" && i + 1 < argc) batch = atoi(argv[++i]);
        else if (a == "--out" && i + 1 < argc) out = argv[++i];
        else if (a == "--device" && i + 1 < argc) device = atoi(argv[++i]);
        else if (a == "--sort") flags |= PT_SORT_MATERIAL;
        else if (a == "--no-compact") flags &= ~PT_COMPACT;
        else if (a == "--cache-first") flags |= PT_CACHE_FIRST;
        else if (a == "--bvh") flags |= PT_MESH_BVH;
        else if (a == "--aa") flags |= PT_AA_JITTER;
        else if (a == "--glossy") flags |= PT_GLOSSY;
        else if (a == "--direct") flags |= PT_DIRECT_LIGHT;
        else if (a == "--direct-sky") flags |= PT_DIRECT_LIGHT | PT_DIRECT_SKY;
        else if (a == "--sun" && i + 1 < argc) {
            if (sscanf(argv[++i], "%lf,%lf,%lf,%lf,%lf,%lf,%lf", &sun_v[0], &sun_v[1], &sun_v[2], &sun_v[3], &sun_v[4], &sun_v[5], &sun_v[6]) != 7) {
                fprintf(stderr, "--sun wants X,Y,Z,COS,R,G,B\n");
                return 1;
            }
            sun = true;
        }
        else if (a == "--textures") flags |= PT_TEXTURES;
        else if (a == "--smooth") flags |= PT_SMOOTH_NORMALS;
        else if (a == "--albedo") albedo = true;
        else if (a == "--lens" && i + 2 < argc) { lens_radius = (float)atof(argv[++i]); focal_distance = (float)atof(argv[++i]); }
        else if (a == "--pfm") pfm = true;
        else if (a == "--save-sum") save_sum = true;
        else if (a == "--resume" && i + 1 < argc) resume = argv[++i];
        else if (a == "--start" && i + 1 < argc) start = atoi(argv[++i]);
        else if (a == "--tile" && i + 1 < argc) {
            if (sscanf(argv[++i], "%d/%d", &tile_index, &tile_count) != 2 || tile_count < 1 || tile_index < 0 || tile_index >= tile_count) {
                fprintf(stderr, "--tile wants R/K with 0 <= R < K\n");
                return 1;
            }
        }
        else if (a == "--per-call") per_call = true;
        else if (a == "--warmup" && i + 1 < argc) warmup = atoi(argv[++i]);
        else if (a == "--no-lookahead") lookahead = false;
        else if (a == "--denoise" && i + 1 < argc) {
            int lv = 0;
            if (sscanf(argv[++i], "%d,%f,%f,%f", &lv, &dn.sigma_color, &dn.sigma_normal, &dn.sigma_position) != 4) {
                fprintf(stderr, "--denoise wants LEVELS,SIGMA_COLOR,SIGMA_NORMAL,SIGMA_POSITION\n");
                return 1;
            }
            dn.levels = lv; denoise = true;
        }
        else if (a == "--variance" && i + 1 < argc) {
            int lv = 0;
            if (sscanf(argv[++i], "%d,%f,%f,%f", &lv, &vr.sigma_luminance, &vr.sigma_normal, &vr.sigma_position) != 4) {
                fprintf(stderr, "--variance wants LEVELS,SIGMA_LUMINANCE,SIGMA_NORMAL,SIGMA_POSITION\n");
                return 1;
            }
            vr.levels = lv; variance = true; flags |= PT_MOMENTS;
        }
        else if (a == "--svgf" && i + 1 < argc) {
            int lv = 0;
            const int got = sscanf(argv[++i], "%d,%f,%f,%f,%d", &lv, &sv.sigma_luminance, &sv.sigma_normal, &sv.sigma_position, &spatial_below);
            if (got != 4 && got != 5) {
                fprintf(stderr, "--svgf wants LEVELS,SIGMA_LUMINANCE,SIGMA_NORMAL,SIGMA_POSITION[,SPATIAL_BELOW]\n");
                return 1;
            }
            sv.levels = lv; svgf = true; flags |= PT_MOMENTS;
        }
        else if (a == "--move" && i + 1 < argc) {
            if (sscanf(argv[++i], "%f,%f,%f,%d", &move_by[0], &move_by[1], &move_by[2], &move_iters) != 4 || move_iters < 1) {
                fprintf(stderr, "--move wants DX,DY,DZ,ITERS with ITERS >= 1\n");
                return 1;
            }
            move = true;
        }
        else if (a == "--temporal" && i + 1 < argc) {
            int cap = 0;
            if (sscanf(argv[++i], "%d,%f,%f", &cap, &tp.position_tolerance, &tp.normal_tolerance) != 3) {
                fprintf(stderr, "--temporal wants MAX_HISTORY,POSITION_TOLERANCE,NORMAL_TOLERANCE\n");
                return 1;
            }
            tp.max_history = cap;
        }
        else if (a == "--sky" && i + 1 < argc) {
            if (sscanf(argv[++i], "%d,%lf,%lf,%lf,%lf,%lf,%lf,%lf,%lf,%lf", &sky_n, &sky[0], &sky[1], &sky[2], &sky[3], &sky[4], &sky[5],
                       &sky[6], &sky[7], &sky[8]) != 10 || sky_n < 1 || sky_n > 1024) {
                fprintf(stderr, "--sky wants N,ZR,ZG,ZB,HR,HG,HB,GR,GG,GB with 1 <= N <= 1024\n");
                return 1;
            }
        }
        else if (a == "--strip-rows" && i + 1 < argc) strip_rows = atoi(argv[++i]);
        else if (a == "--gpus" && i + 1 < argc) { devices.clear(); for (int k = 0, n = atoi(argv[++i]); k < n; ++k) devices.push_back(k); }
        else if (a == "--devices" && i + 1 < argc) {
            devices.clear();
            for (const char *p = argv[++i]; *p;) { devices.push_back((int32_t)strtol(p, (char **)&p, 10)); if (*p == ',') ++p; else if (*p) { fprintf(stderr, "--devices wants D0,D1,...\n"); return 1; } }
        }
        else { fprintf(stderr, "unknown option %s\n", a.c_str()); return 1; }
    }
    pth_scene *sc = pth_load_scene(argv[1]);
    if (!sc) { fprintf(stderr, "%s\n", pth_last_error()); return 1; }
    if (iters < 0) iters = sc->iterations;
    if (sun && sky_n < 1) { fprintf(stderr, "--sun needs --sky (the map it is painted on)\n"); return 1; }
    if (albedo && !denoise) { fprintf(stderr, "--albedo needs --denoise (the filter it switches to irradiance)\n"); return 1; }
    if (variance && !resume.empty()) { fprintf(stderr, "--variance does not combine with --resume (a saved sum does not carry the moments)\n"); return 1; }
    if (svgf && !resume.empty()) { fprintf(stderr, "--svgf does not combine with --resume (a saved sum does not carry the moments)\n"); return 1; }
    if (move && !denoise) { fprintf(stderr, "--move needs --denoise (the filter its pictures go through)\n"); return 1; }
    if (per_call) {
        flags |= PT_PIN_IMAGE | PT_HOST_SPARSE | (lookahead ? PT_LOOKAHEAD : 0u);
        if (!resume.empty()) { fprintf(stderr, "--per-call does not combine with --resume\n"); return 1; }
    }
    if (batch < 1) {                                      // not given: as the shim sizes its windows -- up to 64 iterations and ~40 M paths per batch
        const long long pixels = (long long)sc->camera.resolution[0] * sc->camera.resolution[1];
        const long long k = 41000000LL / (pixels > 0 ? pixels : 1);
        batch = (int)(k < 4 ? 4 : (k > 64 ? 64 : k));
    }
    const int W = sc->camera.resolution[0], H = sc->camera.resolution[1];
    printf("scene %s: %d geoms, %d materials, %d triangles, %dx%d, depth %d, %d iterations\n", argv[1],
           sc->num_geoms, sc->num_materials, sc->num_triangles, W, H, sc->trace_depth, iters);

    pt_scene_desc d;
    memset(&d, 0, sizeof d);
    d.geoms = sc->geoms; d.num_geoms = sc->num_geoms;
    d.materials = sc->materials; d.num_materials = sc->num_materials;
    d.triangles = sc->triangles; d.num_triangles = sc->num_triangles;
    d.meshes = sc->meshes; d.num_meshes = sc->num_meshes;
    d.camera = sc->camera; d.trace_depth = sc->trace_depth; d.flags = flags; d.device = device;
    d.tile_index = tile_index; d.tile_count = tile_count; d.strip_rows = strip_rows; d.max_batch = batch;
    d.lens_radius = lens_radius; d.focal_distance = focal_distance;
    if (!devices.empty()) { d.devices = devices.data(); d.num_devices = (int32_t)devices.size(); }
    pt_free();                                            // main.cpp:126
    if (pt_init(&d) != PT_OK) { fprintf(stderr, "pathtraceInit: %s\n", pt_last_error()); return 1; }

    if (sky_n > 0) {
        // texel (face, j, i): the direction through its centre has 1 (or -1) on the face's axis and the centres' coordinates
        // on the other two, in x, y, z order (include/ptmi355.h: pt_set_environment)
        const int n = sky_n;
        std::vector<float> tex((size_t)6 * n * n * 3);
        for (int face = 0; face < 6; ++face)
            for (int j = 0; j < n; ++j)
                for (int i = 0; i < n; ++i) {
                    const double ca = ((double)i + 0.5) / (double)n * 2.0 - 1.0, cb = ((double)j + 0.5) / (double)n * 2.0 - 1.0;
                    const int axis = face >> 1;
                    double v[3];
                    v[axis] = (face & 1) ? -1.0 : 1.0;
                    v[axis == 0 ? 1 : 0] = ca;
                    v[axis == 2 ? 1 : 2] = cb;
                    const double y = v[1] / std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
                    const double up = y > 0.0 ? y : 0.0, down = -y > 0.0 ? -y : 0.0;
                    float *t = &tex[(((size_t)face * n + j) * n + i) * 3];
                    for (int k = 0; k < 3; ++k) {
                        const double z = sky[k], h = sky[3 + k], g = sky[6 + k];
                        t[k] = (float)(h + (z - h) * up + (g - h) * down);
                    }
                    if (sun) {
                        const double sl = std::sqrt(sun_v[0] * sun_v[0] + sun_v[1] * sun_v[1] + sun_v[2] * sun_v[2]);
                        const double ln = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
                        const double cosine = (v[0] * (sun_v[0] / sl) + v[1] * (sun_v[1] / sl) + v[2] * (sun_v[2] / sl)) / ln;
                        if (cosine >= sun_v[3]) for (int k = 0; k < 3; ++k) t[k] = (float)sun_v[4 + k];
                    }
                }
        if (pt_set_environment(tex.data(), n) != PT_OK) { fprintf(stderr, "pt_set_environment: %s\n", pt_last_error()); return 1; }
        printf("sky: %d x %d x 6 texels\n", n, n);
    }

    if (flags & PT_TEXTURES) {                            // the scene's TEXTURE blocks (pthost.h: pth_scene_texture)
        int set = 0;
        for (int m = 0; m < sc->num_materials; ++m) {
            const float *tex = nullptr;
            int n = 0;
            if (pth_scene_texture(sc, m, &tex, &n) != 0) { fprintf(stderr, "%s\n", pth_last_error()); return 1; }
            if (n == 0) continue;
            if (pt_set_texture(m, tex, n) != PT_OK) { fprintf(stderr, "pt_set_texture: %s\n", pt_last_error()); return 1; }
            ++set;
        }
        printf("textures: %d of %d materials\n", set, sc->num_materials);
        int bumps = 0;                                    // ... and its BUMPMAP blocks (pthost.h: pth_scene_bump_map)
        for (int m = 0; m < sc->num_materials; ++m) {
            const float *tex = nullptr;
            int n = 0;
            if (pth_scene_bump_map(sc, m, &tex, &n) != 0) { fprintf(stderr, "%s\n", pth_last_error()); return 1; }
            if (n == 0) continue;
            if (pt_set_bump_map(m, tex, n) != PT_OK) { fprintf(stderr, "pt_set_bump_map: %s\n", pt_last_error()); return 1; }
            ++bumps;
        }
        if (bumps > 0) printf("bump maps: %d of %d materials\n", bumps, sc->num_materials);
    }

    if (flags & PT_SMOOTH_NORMALS) {                      // the `vn` normals of the scene's mesh files (pthost.h: pth_scene_vertex_normals)
        const float *vn = nullptr;
        int nt = 0;
        if (pth_scene_vertex_normals(sc, &vn, &nt) != 0) { fprintf(stderr, "%s\n", pth_last_error()); return 1; }
        if (nt > 0 && pt_set_vertex_normals(vn, nt) != PT_OK) { fprintf(stderr, "pt_set_vertex_normals: %s\n", pt_last_error()); return 1; }
        printf("vertex normals: %d of %d triangles\n", nt, sc->num_triangles);
    }

    std::vector<float> image((size_t)W * H * 3, 0.0f);    // scene->state.image
    int iteration = 0;
    if (!resume.empty()) {
        if (start < 0) {                                   // BASE.<N>samp.sum.pfm
            const size_t e = resume.rfind("samp");
            size_t b = e;
            while (b != std::string::npos && b > 0 && resume[b - 1] >= '0' && resume[b - 1] <= '9') --b;
            if (e == std::string::npos || b == e) { fprintf(stderr, "--resume: no <N>samp in %s, say --start N\n", resume.c_str()); return 1; }
            start = atoi(resume.substr(b, e - b).c_str());
        }
        if (start < 0 || start > iters) { fprintf(stderr, "--resume: %d iterations done, %d wanted\n", start, iters); return 1; }
        if (pth_read_pfm(resume.c_str(), image.data(), W, H) != 0) { fprintf(stderr, "%s\n", pth_last_error()); return 1; }
        if (pt_set_image(image.data()) != PT_OK) { fprintf(stderr, "pt_set_image: %s\n", pt_last_error()); return 1; }
        iteration = start;
        printf("resumed %s: %d iterations done\n", resume.c_str(), start);
    }
    const int first_iteration = iteration;
    const auto t0 = std::chrono::steady_clock::now();
    if (per_call) {                                        // runCuda() through the shim: one pathtrace() per iteration, image every call
        std::vector<double> ms;
        long long served = 0;                              // rays as pt_get_stats reports them: every iteration once, whole
        for (; iteration < iters; ++iteration) {
            const auto c0 = std::chrono::steady_clock::now();
            if (pt_trace(NULL, 0, iteration + 1, image.data()) != PT_OK) { fprintf(stderr, "pathtrace: %s\n", pt_last_error()); return 1; }
            const auto c1 = std::chrono::steady_clock::now();
            if (iteration >= warmup) ms.push_back(std::chrono::duration<double, std::milli>(c1 - c0).count());
            pt_stats st;
            if (pt_get_stats(&st) != PT_OK) { fprintf(stderr, "pt_get_stats: %s\n", pt_last_error()); return 1; }
            served += st.rays;
        }
        if (ms.empty()) { fprintf(stderr, "--per-call: no call after %d warm-up calls (--iters %d)\n", warmup, iters); return 1; }
        std::vector<double> sorted = ms;
        std::sort(sorted.begin(), sorted.end());
        const double med = sorted[sorted.size() / 2];
        double mean = 0.0;
        for (double v : ms) mean += v;
        mean /= (double)ms.size();
        const double rays_per_iter = (double)served / (double)iters;
        printf("per-call: %zu calls after %d warm-up, median %.4f ms, mean %.4f ms, p10 %.4f, p90 %.4f; %.0f rays per iteration: "
               "%.2f Grays/s (mean call; %.2f at the median) (lookahead %s, max_batch %d, %d device(s))\n",
               ms.size(), warmup, med, mean, sorted[sorted.size() / 10], sorted[sorted.size() * 9 / 10], rays_per_iter,
               rays_per_iter / (mean * 1e-3) / 1e9, rays_per_iter / (med * 1e-3) / 1e9, lookahead ? "on" : "off", batch, pt_num_devices());
    }
    while (iteration < iters) {                            // runCuda: iteration++ ; pathtrace(pbo, 0, iteration)
        const int n = (iters - iteration < batch) ? iters - iteration : batch;
        const int last = (iteration + n == iters);
        // every batch but the last is only enqueued: consecutive batches overlap on the device; the last one
        // waits for all of them and brings the image
        int rc = (n == 1) ? pt_trace(NULL, 0, iteration + 1, last ? image.data() : NULL)
                 : last   ? pt_trace_batch(iteration + 1, n, image.data())
                          : pt_trace_batch_async(iteration + 1, n);
        if (rc != PT_OK) { fprintf(stderr, "pathtrace: %s\n", pt_last_error()); return 1; }
        iteration += n;
    }
    const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    const long long rays = pt_total_rays();
    printf("%d iterations, %lld rays, %.3f s, %.1f Mrays/s on %d device(s), tile exchange: %s\n", iteration - first_iteration, rays, sec, rays / sec / 1e6,
           pt_num_devices(), pt_exchange_transport());
    if (iteration == first_iteration && pt_get_image(image.data()) != PT_OK) { fprintf(stderr, "%s\n", pt_last_error()); return 1; }

    if (out.empty()) out = std::string(sc->image_name[0] ? sc->image_name : "render");
    char name[512];
    snprintf(name, sizeof name, "%s.%dsamp.png", out.c_str(), iteration);   // saveImage(): <FILE>.<time>.<N>samp
    std::vector<uint8_t> rgb((size_t)W * H * 3);
    pth_image_to_rgb8(image.data(), W, H, (float)iteration, rgb.data());
    if (pth_write_png(name, rgb.data(), W, H) != 0) { fprintf(stderr, "%s\n", pth_last_error()); return 1; }
    printf("Saved %s.\n", name);
    if (albedo && pt_set_denoise_albedo(1) != PT_OK) { fprintf(stderr, "pt_set_denoise_albedo: %s\n", pt_last_error()); return 1; }
    if (denoise) {
        // the first call computes the G-buffer of this camera as well; the second is the filter alone
        std::vector<float> mean((size_t)W * H * 3);
        const auto d0 = std::chrono::steady_clock::now();
        if (pt_denoise(&dn, iteration, NULL, NULL) != PT_OK) { fprintf(stderr, "pt_denoise: %s\n", pt_last_error()); return 1; }
        const auto d1 = std::chrono::steady_clock::now();
        if (pt_denoise(&dn, iteration, mean.data(), NULL) != PT_OK) { fprintf(stderr, "pt_denoise: %s\n", pt_last_error()); return 1; }
        const auto d2 = std::chrono::steady_clock::now();
        printf("denoise: %d levels, sigmas %g / %g / %g%s: %.3f ms with the G-buffer, %.3f ms the filter alone (with the copy of the result)\n",
               dn.levels, dn.sigma_color, dn.sigma_normal, dn.sigma_position, albedo ? ", albedo demodulated" : "", std::chrono::duration<double, std::milli>(d1 - d0).count(),
               std::chrono::duration<double, std::milli>(d2 - d1).count());
        snprintf(name, sizeof name, "%s.%dsamp.denoised.png", out.c_str(), iteration);
        pth_image_to_rgb8(mean.data(), W, H, 1.0f, rgb.data());
        if (pth_write_png(name, rgb.data(), W, H) != 0) { fprintf(stderr, "%s\n", pth_last_error()); return 1; }
        printf("Saved %s.\n", name);
    }
    if (variance) {
        // as above: the first call may compute the G-buffer (it shares --denoise's), the second is the filter alone
        std::vector<float> mean((size_t)W * H * 3);
        const auto d0 = std::chrono::steady_clock::now();
        if (pt_denoise_variance(&vr, iteration, NULL, NULL) != PT_OK) { fprintf(stderr, "pt_denoise_variance: %s\n", pt_last_error()); return 1; }
        const auto d1 = std::chrono::steady_clock::now();
        if (pt_denoise_variance(&vr, iteration, mean.data(), NULL) != PT_OK) { fprintf(stderr, "pt_denoise_variance: %s\n", pt_last_error()); return 1; }
        const auto d2 = std::chrono::steady_clock::now();
        printf("variance: %d levels, sigmas %g / %g / %g: %.3f ms the first call, %.3f ms the filter alone (with the copy of the result)\n",
               vr.levels, vr.sigma_luminance, vr.sigma_normal, vr.sigma_position, std::chrono::duration<double, std::milli>(d1 - d0).count(),
               std::chrono::duration<double, std::milli>(d2 - d1).count());
        snprintf(name, sizeof name, "%s.%dsamp.variance.png", out.c_str(), iteration);
        pth_image_to_rgb8(mean.data(), W, H, 1.0f, rgb.data());
        if (pth_write_png(name, rgb.data(), W, H) != 0) { fprintf(stderr, "%s\n", pth_last_error()); return 1; }
        printf("Saved %s.\n", name);
    }
    if (svgf) {
        // the session's first call: no history yet, every pixel below SPATIAL_BELOW samples takes the spatial estimate
        std::vector<float> mean((size_t)W * H * 3);
        const auto d0 = std::chrono::steady_clock::now();
        if (pt_denoise_svgf(&sv, &tp, spatial_below, iteration, mean.data(), NULL) != PT_OK) { fprintf(stderr, "pt_denoise_svgf: %s\n", pt_last_error()); return 1; }
        const auto d1 = std::chrono::steady_clock::now();
        printf("svgf: %d levels, sigmas %g / %g / %g, spatial below %d, max_history %d, tolerances %g / %g: %.3f ms (with the copy of the result)\n",
               sv.levels, sv.sigma_luminance, sv.sigma_normal, sv.sigma_position, spatial_below, tp.max_history, tp.position_tolerance,
               tp.normal_tolerance, std::chrono::duration<double, std::milli>(d1 - d0).count());
        snprintf(name, sizeof name, "%s.%dsamp.svgf.png", out.c_str(), iteration);
        pth_image_to_rgb8(mean.data(), W, H, 1.0f, rgb.data());
        if (pth_write_png(name, rgb.data(), W, H) != 0) { fprintf(stderr, "%s\n", pth_last_error()); return 1; }
        printf("Saved %s.\n", name);
    }
    if (pfm) {
        snprintf(name, sizeof name, "%s.%dsamp.pfm", out.c_str(), iteration);
        pth_write_pfm(name, image.data(), W, H, (float)iteration);
        printf("Saved %s.\n", name);
    }
    if (save_sum) {
        snprintf(name, sizeof name, "%s.%dsamp.sum.pfm", out.c_str(), iteration);
        if (pth_write_pfm(name, image.data(), W, H, 1.0f) != 0) { fprintf(stderr, "%s\n", pth_last_error()); return 1; }
        printf("Saved %s.\n", name);
    }
    if (move) {
        std::vector<float> mean((size_t)W * H * 3);
        const auto m0 = std::chrono::steady_clock::now();
        if (pt_denoise_temporal(&dn, &tp, iteration, NULL, NULL) != PT_OK) { fprintf(stderr, "pt_denoise_temporal: %s\n", pt_last_error()); return 1; }
        const auto m1 = std::chrono::steady_clock::now();
        pt_camera cam = sc->camera;
        cam.position.x += move_by[0]; cam.position.y += move_by[1]; cam.position.z += move_by[2];
        cam.lookAt.x += move_by[0]; cam.lookAt.y += move_by[1]; cam.lookAt.z += move_by[2];
        if (pt_set_camera(&cam, sc->trace_depth) != PT_OK) { fprintf(stderr, "pt_set_camera: %s\n", pt_last_error()); return 1; }
        if (pt_clear_image() != PT_OK) { fprintf(stderr, "pt_clear_image: %s\n", pt_last_error()); return 1; }
        const auto m2 = std::chrono::steady_clock::now();
        for (int it = 0; it < move_iters;) {
            const int n = (move_iters - it < batch) ? move_iters - it : batch;
            const int rc = (n == 1) ? pt_trace(NULL, 0, it + 1, NULL) : pt_trace_batch(it + 1, n, NULL);
            if (rc != PT_OK) { fprintf(stderr, "pathtrace: %s\n", pt_last_error()); return 1; }
            it += n;
        }
        if (pt_get_image(image.data()) != PT_OK) { fprintf(stderr, "pt_get_image: %s\n", pt_last_error()); return 1; }
        const auto m3 = std::chrono::steady_clock::now();
        snprintf(name, sizeof name, "%s.moved.%dsamp.png", out.c_str(), move_iters);
        pth_image_to_rgb8(image.data(), W, H, (float)move_iters, rgb.data());
        if (pth_write_png(name, rgb.data(), W, H) != 0) { fprintf(stderr, "%s\n", pth_last_error()); return 1; }
        printf("Saved %s.\n", name);
        const auto m4 = std::chrono::steady_clock::now();
        if (pt_denoise(&dn, move_iters, mean.data(), NULL) != PT_OK) { fprintf(stderr, "pt_denoise: %s\n", pt_last_error()); return 1; }
        const auto m5 = std::chrono::steady_clock::now();
        snprintf(name, sizeof name, "%s.moved.%dsamp.denoised.png", out.c_str(), move_iters);
        pth_image_to_rgb8(mean.data(), W, H, 1.0f, rgb.data());
        if (pth_write_png(name, rgb.data(), W, H) != 0) { fprintf(stderr, "%s\n", pth_last_error()); return 1; }
        printf("Saved %s.\n", name);
        const auto m6 = std::chrono::steady_clock::now();
        if (pt_denoise_temporal(&dn, &tp, move_iters, mean.data(), NULL) != PT_OK) { fprintf(stderr, "pt_denoise_temporal: %s\n", pt_last_error()); return 1; }
        const auto m7 = std::chrono::steady_clock::now();
        snprintf(name, sizeof name, "%s.moved.%dsamp.temporal.png", out.c_str(), move_iters);
        pth_image_to_rgb8(mean.data(), W, H, 1.0f, rgb.data());
        if (pth_write_png(name, rgb.data(), W, H) != 0) { fprintf(stderr, "%s\n", pth_last_error()); return 1; }
        printf("Saved %s.\n", name);
        if (svgf) {                                        // the first view's call above is the history
            const auto s0 = std::chrono::steady_clock::now();
            if (pt_denoise_svgf(&sv, &tp, spatial_below, move_iters, mean.data(), NULL) != PT_OK) { fprintf(stderr, "pt_denoise_svgf: %s\n", pt_last_error()); return 1; }
            const auto s1 = std::chrono::steady_clock::now();
            snprintf(name, sizeof name, "%s.moved.%dsamp.svgf.png", out.c_str(), move_iters);
            pth_image_to_rgb8(mean.data(), W, H, 1.0f, rgb.data());
            if (pth_write_png(name, rgb.data(), W, H) != 0) { fprintf(stderr, "%s\n", pth_last_error()); return 1; }
            printf("Saved %s.\n", name);
            printf("svgf, moved view: %.3f ms pt_denoise_svgf with the reprojection (with the copy of the result)\n",
                   std::chrono::duration<double, std::milli>(s1 - s0).count());
        }
        auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
            return std::chrono::duration<double, std::milli>(b - a).count();
        };
        printf("move (%g, %g, %g), %d iterations, max_history %d, tolerances %g / %g: %.3f ms the temporal call on the finished view, "
               "%.3f ms the %d iterations of the moved view, %.3f ms pt_denoise with its G-buffer, %.3f ms pt_denoise_temporal with the reprojection "
               "(both with the copy of the result)\n", move_by[0], move_by[1], move_by[2], move_iters, tp.max_history, tp.position_tolerance,
               tp.normal_tolerance, ms(m0, m1), ms(m2, m3), move_iters, ms(m4, m5), ms(m6, m7));
    }
    pt_free();
    pth_free_scene(sc);
    return 0;
}
