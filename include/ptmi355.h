/*
 * ptmi355.h -- C-ABI of libptmi355.so, the MI355X-native (gfx950, HIP) wavefront
 * path tracer that replaces the hot path of CIS565 Project3-CUDA-Path-Tracer.
 *
 * The reference exposes the path as three C++ free functions
 *     void pathtraceInit(Scene *scene);                         src/pathtrace.h:6
 *     void pathtraceFree();                                     src/pathtrace.h:7
 *     void pathtrace(uchar4 *pbo, int frame, int iteration);    src/pathtrace.h:8
 * called only from runCuda() (src/main.cpp:126-127,137,143).  `Scene` holds
 * std::vector / std::string / ifstream (src/scene.h:13-26) and cannot cross a C
 * boundary, so the C-ABI takes the same information as plain pointers + sizes;
 * project3-cuda-path-tracer_amd/host/pathtrace_shim.cpp provides the three
 * reference signatures on top of it.
 *
 * Struct layouts are byte-identical to src/sceneStructs.h:15-76 as compiled for
 * x86-64 (sizes/offsets in SURVEY.md 8b; asserted in csrc/ptmi355.hip).
 *
 * Contract (same as the reference, src/pathtrace.cu:70-75): one renderer
 * instance per process, not re-entrant, calls are synchronous unless stated.
 * One instance may drive several GPUs of the node (pt_scene_desc::devices):
 * that stays invisible to the caller, who still sees one frame.
 * Every int-returning entry point returns PT_OK (0) or a negative pt_status;
 * pt_last_error() then describes the failure.  The library never falls back
 * to a CPU path: without a HIP device every call fails with PT_ERR_DEVICE.
 *
 * Environment.  The shipped library reads exactly these nine variables, at
 * pt_init (PTMI355_RCCL_LIB: when RCCL is first needed).  NONE of them changes a
 * result: images, per-bounce statistics and path order are bit-identical under
 * every setting (each is exercised against the default by a `-m gpu` test, named
 * in brackets); they select launch plans, transports and memory budgets.
 *   PTMI355_DEVICES="0,1,.."|"all"  tile the frame over these GPUs for a host that knows one device
 *                                   (pt_scene_desc::devices below)          [test_devices_from_the_environment_and_the_reference_host]
 *   PTMI355_XCHG=rccl|peer          transport of the in-library tile exchange (default: RCCL when every
 *                                   context has its own device, peer copies otherwise)  [test_rccl_calls_with_a_communicator_of_one]
 *   PTMI355_RCCL_LIB=/path/librccl.so.1  the RCCL library to dlopen before the default names
 *                                                                            [test_rccl_library_named_by_the_environment]
 *   PTMI355_WHOLE_MAX=<paths>       largest batch (paths) traced as ONE launch (k_iteration; default 6 000 000);
 *                                   0 = a kernel per bounce for every batch   [the launch_plan fixture: most parity tests run under both]
 *   PTMI355_WHOLE_MAX_HOST=<paths>  the same limit for a pt_trace call that hands over a host image (default
 *                                   16 000 000)                              [test_4k_one_iteration_per_call_into_the_host_image]
 *   PTMI355_OVERLAP=0|1|n           consecutive asynchronous batches overlap on n lanes (1 = default lane count,
 *                                   0 = strictly one after the other)        [test_overlapped_small_batches]
 *   PTMI355_OVERLAP_GB=<GB>         memory the lanes' extra path pools may take (they are dropped when it does
 *                                   not suffice)                             [test_overlapped_small_batches]
 *   PTMI355_CULL0=0|1               the per-camera bounce-0 candidate masks (k_cull0_mask) off / on  [test_bounce0_candidate_masks]
 *   PTMI355_SCENE_LDS=0             scene records read through the vector cache instead of staged in LDS (what
 *                                   scenes too large for LDS get anyway)     [test_scene_gathers_from_global_memory]
 * Everything else rounds 1-4 switched through the environment (occupancy, stream-layout and transport experiments,
 * test hooks) exists only in a build with -DPT_EXPERIMENTS (profiles/tools/build_variant.sh); pt_version() of such a
 * build ends in "+experiments".
 */
#ifndef PTMI355_H
#define PTMI355_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- POD mirrors of src/sceneStructs.h ---------------------------------- */
typedef struct pt_vec3 { float x, y, z; } pt_vec3;                 /* glm::vec3, 12 B */
typedef struct pt_mat4 { float m[4][4]; } pt_mat4;                 /* glm::mat4, m[col][row] */

enum pt_geom_type { PT_SPHERE = 0, PT_CUBE = 1,                    /* sceneStructs.h:10-13 */
                    PT_TRIANGLE_MESH = 2 };                        /* extension (INSTRUCTION.md:123-128) */

typedef struct pt_ray { pt_vec3 origin, direction; } pt_ray;       /* sceneStructs.h:15-18, 24 B */

typedef struct pt_geom {                                           /* sceneStructs.h:20-29, 236 B */
    int32_t type;
    int32_t materialid;
    pt_vec3 translation, rotation, scale;
    pt_mat4 transform, inverseTransform, invTranspose;
} pt_geom;

typedef struct pt_material {                                       /* sceneStructs.h:31-41, 44 B */
    pt_vec3 color;
    struct { float exponent; pt_vec3 color; } specular;
    float hasReflective, hasRefractive, indexOfRefraction, emittance;
} pt_material;

typedef struct pt_camera {                                         /* sceneStructs.h:43-52, 84 B */
    int32_t resolution[2];
    pt_vec3 position, lookAt, view, up, right;
    float fov[2];
    float pixelLength[2];
} pt_camera;

typedef struct pt_path_segment {                                   /* sceneStructs.h:62-67, 44 B */
    pt_ray ray;
    pt_vec3 color;
    int32_t pixelIndex;
    int32_t remainingBounces;
} pt_path_segment;

typedef struct pt_shadeable_intersection {                         /* sceneStructs.h:72-76, 20 B */
    float t;
    pt_vec3 surfaceNormal;
    int32_t materialId;
} pt_shadeable_intersection;

/* world-space triangle soup for PT_TRIANGLE_MESH geoms (no reference counterpart) */
typedef struct pt_triangle { pt_vec3 v0, v1, v2; } pt_triangle;    /* 36 B */
typedef struct pt_mesh { int32_t geom_index, first_triangle, triangle_count; } pt_mesh;

/* ---- status codes ---------------------------------------------------------- */
enum pt_status {
    PT_OK = 0,
    PT_ERR_INVALID = -1,      /* bad argument / called in the wrong state */
    PT_ERR_DEVICE = -2,       /* HIP runtime error (pt_last_error has hipGetErrorString) */
    PT_ERR_NOMEM = -3,
    PT_ERR_INTERNAL = -4      /* kernel-side watchdog tripped (look-back spin bound) */
};

/* ---- run-time toggles (the compile-time #defines the assignment asks for,
 *      INSTRUCTION.md:77-89, as flags) ------------------------------------- */
enum pt_flags {
    PT_COMPACT       = 1u << 0,  /* stable live-path compaction after every bounce */
    PT_SORT_MATERIAL = 1u << 1,  /* live paths stably sorted by the materialId they hit (INSTRUCTION.md:78-86): the pool
                                    order after every bounce is the stable partition of that sorted order.  With
                                    compaction and up to 64 materials the survivors are PLACED by material as the fused
                                    kernel writes them (csrc/pt_types.hpp: RangeDir); PT_UNFUSED | PT_SORT_MATERIAL, or
                                    no compaction, runs the separate intersect -> key histogram -> sorted-shade kernels */
    PT_FAKE_SHADER   = 1u << 2,  /* the reference as shipped: one bounce + shadeFakeMaterial
                                    (pathtrace.cu:224-266,339-377) */
    PT_CACHE_FIRST   = 1u << 3,  /* cache the bounce-0 intersections (INSTRUCTION.md:87-89): a table of every pixel's first
                                    hit (t, normal, material, inside / outside, primitive), filled once per camera by the
                                    first batch that needs it; bounce 0 of every batch looks its hits up instead of
                                    intersecting.  Results are bit-identical either way, and the ray counters still count
                                    bounce-0 paths (pt_stats.rays, pt_total_rays: one ray per live path and bounce, whether
                                    its intersection was computed or looked up).
                                    The plain fused pipeline (no PT_UNFUSED, PT_SORT_MATERIAL, PT_FAKE_SHADER, no triangle
                                    meshes) uses the same table WITHOUT the flag whenever its camera rays repeat -- no
                                    PT_AA_JITTER, no lens at the time of the call, no texture set, bounce 0 not one of
                                    PT_DIRECT_LIGHT's two sampling bounces -- except for batches small enough to run as one
                                    launch.  The flag forces the table form for every batch (no one-launch iterations, no
                                    PT_LOOKAHEAD windows) and keeps its refusals: PT_AA_JITTER, a lens, PT_DIRECT_LIGHT,
                                    PT_TEXTURES. */
    PT_UNFUSED       = 1u << 4,  /* debug: separate intersect / shade kernels with the
                                    ShadeableIntersection planes materialised in HBM */
    PT_MESH_BVH      = 1u << 5,  /* cull triangle tests with a bounding-volume hierarchy built at
                                    pt_init (INSTRUCTION.md:129-139,218-240); same winner as the
                                    loop over every triangle */
    PT_AA_JITTER     = 1u << 6,  /* stochastic antialiasing: jitter each camera ray inside its
                                    pixel (the TODO at pathtrace.cu:134; INSTRUCTION.md:110).
                                    Excludes PT_CACHE_FIRST (INSTRUCTION.md:113). */
    PT_PIN_IMAGE     = 1u << 8,  /* opt-in: the host image handed to pt_trace / pt_trace_batch is ONE buffer that stays
                                    allocated at its address until pt_free (the reference's scene->state.image is: sized at
                                    load, scene.cpp:145-147).  The library then page-locks it on first use and, when an
                                    iteration runs as one launch, lets the kernel write the running sums into it over PCIe
                                    while it is still tracing -- EVERY pixel, every call, like the reference's cudaMemcpy
                                    (pathtrace.cu:389-390): whatever the host did to the buffer between two calls is
                                    overwritten.  Without the flag every call copies into whatever buffer it is given
                                    (pageable path): buffers may be freed or reallocated between calls. */
    PT_HOST_SPARSE   = 1u << 10, /* opt-in, with PT_PIN_IMAGE / PT_ASYNC_IMAGE: the host promises to only READ the image
                                    between calls (the reference's host does: main.cpp:78-99 reads it in saveImage, nothing
                                    writes it).  From the second consecutive pt_trace on the launch then writes only the
                                    pixels whose sum changed (a path that ends with colour 0 adds nothing: four in five at
                                    800x800 Cornell): 0.133 ms per call against 0.236.  The library tracks everything IT
                                    does to the accumulation buffer (batches, pt_clear_image, pt_set_image, another host
                                    buffer) and writes every pixel again after such a change; a write by the HOST into the
                                    buffer is not seen -- such pixels stay as the host left them until their sum changes. */
    PT_SHARED_IMAGE  = 1u << 9,  /* tiled sessions (tile_count > 1), pt_trace: host_image_sum is ONE frame shared by all the
                                    ranks that tile it (every process maps the same memory, e.g. POSIX shared memory) under the
                                    rules of PT_PIN_IMAGE and PT_HOST_SPARSE, which it implies.  A rank's launch writes the pixels of its OWN tile
                                    into it and nothing else, so the ranks assemble the frame in host memory with no exchange
                                    between them: it holds the sum after iteration i once every rank's call for i has returned.
                                    Without the flag a tiled session copies its whole accumulation buffer (zeros outside its
                                    tile).  Needs a mappable buffer, and iterations that run as one launch unless the call is
                                    served from a PT_LOOKAHEAD window (whose gather writes the tile's pixels): PT_ERR_INVALID if not. */
    PT_LOOKAHEAD     = 1u << 11, /* opt-in: pt_trace TRACES AHEAD of its caller.  The reference's host calls ONE pathtrace() per
                                    iteration (main.cpp:130-140) and a path's whole life is a function of (iteration, pixelIndex,
                                    depth) alone, so the iterations to come can be traced before they are asked for.  pt_trace(iter)
                                    then traces a WINDOW [iter, iter + n) as one path pool (n grows 4, 16, .. up to max_batch; up to three
                                    further windows are traced ahead, beside the one being consumed) and
                                    keeps every sample's final colours; the calls for iter + 1 .. iter + n - 1 only run finalGather
                                    for their own sample -- image[pixel] += colour, the same single addition per pixel and
                                    iteration, in iteration order -- write the pixels whose sum changed into the host image
                                    (PT_PIN_IMAGE | PT_HOST_SPARSE; every pixel otherwise) and tonemap the PBO, while the NEXT
                                    window is already being traced beside them.  state.image, the PBO and the device's
                                    accumulation buffer are complete when each call returns, bit for bit what the same calls
                                    produce without the flag.  A window is discarded (and the iteration traced afresh) when
                                    `iter` is not the next consecutive one, when camera, traceDepth or lens differ from what it
                                    was traced with, and by pt_clear_image, pt_set_image, batches and the stepping interface.
                                    What differs: pt_get_stats reports a window's counts ONCE, with the call that starts
                                    consuming it (the calls served from it afterwards report rays = 0: the sums over a run of
                                    calls are exact), and pt_total_rays / pt_get_counters count a window when it is traced,
                                    ahead of its calls (iterations traced ahead and then discarded stay counted).  With a
                                    page-locked host image (PT_PIN_IMAGE | PT_HOST_SPARSE) on a 256-CU device the windows are
                                    traced on 232 compute units and the calls' gathers write the image from the other 24
                                    (CU-masked streams of the library's own; results unchanged) -- only by a context that is
                                    alone on its device: contexts of one session that share a device trace and gather on plain
                                    streams.  Tiled sessions trace their windows over their own tile: a rank of the process
                                    form (tile_count > 1) writes only its tile's pixels into a PT_SHARED_IMAGE frame (the frame
                                    holds the sum after iteration i once every rank's call for i has returned, as without the
                                    flag); in a session over several devices every context serves its tile from its own windows
                                    and writes its pixels into the host image, with no exchange, when the call has no PBO and
                                    the host image is page-locked for every device (PT_PIN_IMAGE) or absent (pt_get_image /
                                    pt_device_image then assemble the frame); a call with a PBO or a pageable host image, and
                                    every batch, takes the plain path after every context's windows are discarded.  On the
                                    fused pipelines; ignored elsewhere (PT_UNFUSED, PT_FAKE_SHADER, PT_CACHE_FIRST, two-kernel
                                    sort, PT_ASYNC_IMAGE, max_batch < 2). */
    PT_GLOSSY        = 1u << 12, /* opt-in: imperfect specular surfaces.  pt_material::specular.exponent, which is ignored
                                    without the flag, gives a mirror (hasReflective > 0) or a dielectric (hasRefractive > 0)
                                    a GGX lobe: the ray scatters about a sampled microfacet normal instead of the surface
                                    normal ("glossy reflection and frosted glass" below).  Exponent 0,
                                    negative, NaN or infinite: no lobe, today's path with today's draws.  Diffuse surfaces,
                                    emitters, the miss exit and the last-bounce rule are untouched; PT_FAKE_SHADER ignores
                                    the flag.  Honoured by every pipeline that shades. */
    PT_DIRECT_LIGHT  = 1u << 13, /* opt-in: direct lighting.  The last bounce of a path that hits a diffuse surface, which
                                    ends with colour 0 without the flag, aims a FINAL RAY at a random point of an emissive
                                    cube or sphere instead: with traceDepth D a path has D + 1 bounces, and the final ray
                                    scores only if its nearest hit is the primitive it was aimed at ("direct lighting"
                                    below).  Its expectation is that of a plain session of depth
                                    D + 1 in a scene without specular surfaces.  Bounces 0 .. D - 2, emitters, misses,
                                    mirrors and dielectrics are untouched; mesh emitters are not sampled, the environment map
                                    only with PT_DIRECT_SKY; a scene without an emissive cube or sphere renders as without the flag, bit for
                                    bit.  pt_stats reports D + 1 bounces (live[D] = the final rays), pt_trace_bounce accepts
                                    depth D.  Honoured by the fused pipelines (with and without PT_COMPACT, the fused form of
                                    PT_SORT_MATERIAL, meshes with and without PT_MESH_BVH), which run such a session a kernel
                                    per bounce, whatever PTMI355_WHOLE_MAX says: the one-launch kernel has no direct form.
                                    Refused by pt_init (PT_ERR_INVALID) with PT_UNFUSED, with PT_CACHE_FIRST, with a
                                    PT_SORT_MATERIAL session that would take the two-kernel form (their intersection planes
                                    do not carry the winning primitive; extending them is a later change), with
                                    trace_depth > 63 (pt_stats::live has 64 entries; pt_set_camera refuses that depth
                                    likewise) and with more than 1024 light elements.  PT_FAKE_SHADER ignores the flag. */
    PT_TEXTURES      = 1u << 14, /* opt-in: texture mapping.  A material may carry a CUBE TEXTURE (pt_set_texture): at a hit on
                                    a sphere or cube the texel that the object-space hit point reads multiplies material.color
                                    -- at the emitter exit and in the diffuse multiply ("texture mapping" below; DESIGN.md
                                    section 6.19).  specular.color, every draw, origins and directions are untouched; hits on
                                    meshes, on materials without a texture and misses are as without the flag; a flagged
                                    session with no texture set is the plain session bit for bit and launches its kernels.
                                    While a texture is set the session runs a kernel per bounce, whatever PTMI355_WHOLE_MAX
                                    says: the one-launch kernel has no textured form.  Honoured by the fused pipelines (with
                                    and without PT_COMPACT, the fused form of PT_SORT_MATERIAL, meshes with and without
                                    PT_MESH_BVH).  Refused by pt_init (PT_ERR_INVALID) with PT_UNFUSED, with PT_CACHE_FIRST,
                                    with a PT_SORT_MATERIAL session that would take the two-kernel form (their intersection
                                    planes do not carry the winning primitive) and with PT_DIRECT_LIGHT (the textured form of
                                    the direct kernels is a later change).  PT_FAKE_SHADER ignores the flag. */
    PT_DIRECT_SKY    = 1u << 15, /* opt-in, with PT_DIRECT_LIGHT: the environment map, while one is set, is one more light
                                    element behind the lamps' -- the sampling bounce picks it with probability 1/2 (1 in a
                                    scene without lamps), draws a direction from a table built over the map's texels and the
                                    final ray scores the map's radiance where it leaves the scene ("direct lighting samples the
                                    environment map" below).  Without a map, or with a map that yields
                                    no element (no texel with a finite luminance > 0), the session is the PT_DIRECT_LIGHT
                                    session bit for bit.  The light count, and with it the number of bounces (pt_stats, live[D],
                                    pt_trace_bounce), follows pt_set_environment.  The sampler ignores the cosine and
                                    visibility: on a featureless sky it is noisier than the ordinary bounce, under a small
                                    bright region far quieter.  Refused by pt_init (PT_ERR_INVALID) without PT_DIRECT_LIGHT;
                                    PT_FAKE_SHADER ignores both. */
    PT_SMOOTH_NORMALS = 1u << 16, /* opt-in: smooth shading of triangle meshes.  While per-vertex normals are set
                                    (pt_set_vertex_normals) a hit on a mesh triangle is shaded about the normal interpolated
                                    from its three corners instead of the facet normal ("smooth shading" below; DESIGN.md
                                    section 6.26).  Colours, origins, t, misses, spheres, cubes and the ray counters are
                                    untouched; a flagged session with no normals set, or with all-zero normals, is the plain
                                    session bit for bit.  While normals are set the session runs a kernel per bounce.  Honoured
                                    by the fused pipelines (with and without PT_COMPACT, the fused form of PT_SORT_MATERIAL,
                                    meshes with and without PT_MESH_BVH, PT_GLOSSY, an environment map).  Refused by pt_init
                                    (PT_ERR_INVALID) with PT_UNFUSED, with PT_CACHE_FIRST, with a PT_SORT_MATERIAL session that
                                    would take the two-kernel form (their planes carry one normal, and the guard needs two)
                                    and with PT_TEXTURES or PT_DIRECT_LIGHT (the combined kernel forms are a later change).
                                    PT_FAKE_SHADER ignores the flag. */
    PT_MOMENTS       = 1u << 17, /* opt-in: the session keeps, beside the running sum, two float planes of per-pixel LUMINANCE
                                    MOMENTS -- M1 += l, M2 += l * l for every iteration gathered, in iteration order, l =
                                    (0.2126f r + 0.7152f g) + 0.0722f b of the colour that iteration's path ended with (0 for a
                                    path that ended with colour 0) -- which pt_denoise_variance turns into the noise estimate
                                    that steers its filter ("the filter steered by the pixels' own noise" below; DESIGN.md
                                    section 6.27).  The image, pt_stats, the ray counters and pt_export_paths are those of the
                                    unflagged session bit for bit.  Every sample of a flagged session is gathered by the gather
                                    kernel: a one-iteration call does not gather inside its launch, a host image is handed
                                    over by the plain copies, and PT_LOOKAHEAD is ignored (as with PT_ASYNC_IMAGE or
                                    PT_CACHE_FIRST).  Batches, asynchronous batches, the stepping interface and every shading
                                    flag (PT_FAKE_SHADER included) work unchanged.  8 bytes per pixel, zeroed by pt_init,
                                    released by pt_free.  Refused by pt_init (PT_ERR_INVALID) with tile_count > 1 or several
                                    devices. */
    PT_ASYNC_IMAGE   = 1u << 7  /* opt-in: pt_trace / pt_trace_batch return without waiting; the copy of the
                                    running sum into host_image_sum overlaps the NEXT call's tracing and is
                                    complete when the next pt_trace / pt_trace_batch returns, or after
                                    pt_synchronize, pt_get_image or pt_free (pt_get_stats needs pt_synchronize).  (pt_trace: the launch
                                    writes the page-locked buffer itself, as under PT_PIN_IMAGE; with PT_HOST_SPARSE only the
                                    pixels that changed.)  Off = the reference's synchronous pathtrace()
                                    (pathtrace.cu:389-392).  Implies the lifetime rule of PT_PIN_IMAGE for the buffers
                                    handed over (they are read by a copy that is still running when the call returns). */
};

typedef struct pt_scene_desc {
    const pt_geom *geoms;          int32_t num_geoms;       /* scene->geoms  (scene.h:23) */
    const pt_material *materials;  int32_t num_materials;   /* scene->materials (scene.h:24) */
    const pt_triangle *triangles;  int32_t num_triangles;   /* optional */
    const pt_mesh *meshes;         int32_t num_meshes;      /* optional */
    pt_camera camera;                                       /* scene->state.camera */
    int32_t trace_depth;                                    /* scene->state.traceDepth */
    uint32_t flags;                                         /* pt_flags */
    int32_t device;                /* HIP device ordinal */
    void *stream;                  /* hipStream_t to launch on, NULL = a private stream */
    /* frame tiling for multi-GPU: this instance owns the rows y with
     * (y / strip_rows) % tile_count == tile_index.  {0,1,*} = whole frame. */
    int32_t tile_index, tile_count, strip_rows;
    int32_t max_batch;             /* iterations in flight in pt_trace_batch (>=1) */
    float *device_image;           /* optional caller-owned device buffer, W*H*3 floats,
                                      used as the accumulation buffer (e.g. a torch tensor
                                      handed to RCCL); NULL = library-owned */
    /* thin-lens depth of field (INSTRUCTION.md:111): rays start on a disc of this radius
     * around camera.position and meet the pinhole ray on the plane focal_distance along
     * camera.view.  0 (a zeroed descriptor) = the reference's pinhole camera. */
    float lens_radius, focal_distance;
    /* Several GPUs of one node behind this one session (SURVEY 8b "Threading", 8e): the frame is tiled over
     * devices[0..num_devices) in interleaved strips of strip_rows rows (0 = 8), every device traces its tile on its
     * own host thread and stream, and after every pt_trace / batch the tiles' running sums travel to devices[0] over
     * RCCL (one grouped ncclSend / ncclRecv exchange on a communicator from ncclCommInitAll; peer copies where RCCL
     * cannot be used), which assembles the frame pt_trace hands back -- bit-identical to the single-device image
     * (global pixelIndex as RNG key).  num_devices == 0 (a zeroed descriptor): the single device `device`, unless
     * the environment names several (PTMI355_DEVICES="0,1,2,3" | "all": the reference's host, which knows one
     * device -- preview.cpp:107 -- then needs no change).  With several devices: `device`, tile_index / tile_count
     * are ignored (tile_count must be 0 or 1), `stream` and `device_image` belong to devices[0], PT_ASYNC_IMAGE is
     * ignored (calls that hand over a host image are synchronous) and the stepping interface is unavailable. */
    const int32_t *devices;
    int32_t num_devices;
} pt_scene_desc;

typedef struct pt_stats {
    int32_t  bounces;              /* bounces executed in the last iteration / batch */
    int64_t  rays;                 /* sum over bounces of live paths traced (the metric's numerator) */
    int32_t  live[64];             /* live[d] = paths traced at bounce d, last iteration / batch */
    int64_t  total_rays;           /* since pt_init */
    int64_t  total_iterations;
} pt_stats;

/* pathtraceInit (pathtrace.cu:79-98): copies geoms/materials/triangles to the
 * device, allocates the path pool, zeroes the accumulation buffer. */
int pt_init(const pt_scene_desc *desc);

/* pathtraceFree (pathtrace.cu:100-112): idempotent, safe before the first init
 * (main.cpp:126 calls it that way). */
void pt_free(void);

/* The reference re-reads camera + traceDepth from the Scene on every
 * pathtrace() (pathtrace.cu:285-286); the shim forwards them here each call.
 * Resolution must not change between pt_init and pt_free. */
int pt_set_camera(const pt_camera *camera, int trace_depth);
int pt_set_lens(float lens_radius, float focal_distance);   /* see pt_scene_desc */

/* ---- environment lighting: a ray that leaves the scene reads a cube map ------------------------------------------------
 * Without a map a path whose ray hits nothing ends with colour 0 (pathtrace.cu:262-264): only emitters give light.  With
 * one it ends with colour = throughput * E(d) per component, d = the direction of the ray that missed exactly as it was
 * traced.  E(d) is the NEAREST texel of a cube map of n x n texels per face (DESIGN.md section 6.16 has the complete
 * specification; binary32, one rounding per operation, no FMA; tests/environment_model.py is its numpy form, and the
 * device's result equals it bit for bit):
 *   axis  = 0 if |d.x| >= |d.y| and |d.x| >= |d.z|, else 1 if |d.y| >= |d.z|, else 2;  m = |d[axis]|;  !(m > 0): E = 0
 *   face  = 2 * axis + (d[axis] < 0);  (a, b) = the other two components in x, y, z order (no mirroring per face)
 *   i     = min((int)((a / m * 0.5f + 0.5f) * (float)n), n - 1), j likewise from b;  texel (face * n + j) * n + i
 * The "remainingBounces reaches 0 -> colour 0" rule is unchanged, and so are the G-buffer and the filters (a miss keeps
 * t = -1; its pixel now carries colour in the running sum).
 * pt_set_environment: texels = host array of 6 * n * n RGB float32 triples, index ((face * n + j) * n + i) * 3, copied to
 * the device(s); texels == NULL or n == 0: no environment (the state after pt_init).  Session state: it survives
 * pt_set_camera and pt_clear_image and ends with pt_free.  The call synchronises the session and discards the
 * PT_LOOKAHEAD windows, as a camera change does; it does not touch the accumulation buffer (the host decides whether to
 * pt_clear_image).  Non-finite texels propagate as in any multiplication.  Honoured by every pipeline -- batches,
 * asynchronous batches, windows, the stepping interface, tiled sessions, sessions over several devices -- except
 * PT_FAKE_SHADER (the reference as shipped), which ignores it.
 * pt_get_environment: *n = the size set (0: none; nothing else is written then); the texels as they were given, when
 * capacity_texels >= 6 * n * n (PT_ERR_INVALID otherwise, with *n set).
 * PT_ERR_INVALID: before pt_init; n outside [0, 1024]; texels == NULL with n > 0. */
int pt_set_environment(const float *texels, int n);
int pt_get_environment(float *texels, int capacity_texels, int *n);
/* host-only (no GPU): the texel index the specification assigns to each of `count` directions (dirs: count x 3 floats) in
 * a map of n x n texels per face (n in [1, 1024]), -1 where it assigns none */
int pt_environment_texel(const float *dirs, int count, int n, int32_t *index);

/* ---- texture mapping (PT_TEXTURES): one cube texture per material, on spheres and cubes -------------------------------------
 * All arithmetic binary32, one rounding per operation in the order written, no FMA (tests/texture_model.py is the numpy form,
 * and the device's result equals it bit for bit).  A cube texture is 6 * n * n RGB float32 texels,
 * index ((face * n + j) * n + i) * 3, n in [1, 1024]: the layout of pt_set_environment.  At a hit with t > 0 on primitive g
 * of type PT_SPHERE or PT_CUBE whose material m has a texture T of size n:
 *   P = getPointOnRay's point, as the shader computes it;  q = multiplyMV(g.inverseTransform, (P, 1));
 *   k = the texel pt_environment_texel assigns to q (major-axis ties to the earlier axis, face = 2 * axis + (negative ? 1 : 0),
 *       the other two components in x, y, z order without mirroring, nearest texel, clamped; -1 for a zero or NaN point);
 *   mcol = k >= 0 ? (color.x * T[k].r, color.y * T[k].g, color.z * T[k].b) : color
 * and mcol stands exactly where material.color stands: the emitter exit (colour *= mcol * emittance) and the diffuse multiply.
 * For a cube this is planar mapping of the face that was hit, for a sphere the cube-sphere mapping.  Mirrors and dielectrics
 * look as before (specular.color has no texture).  Meshes have no parametrisation: their hits read material.color as it is.
 * pt_gbuffer, pt_denoise and pt_denoise_temporal are unchanged: they filter the textured running sum, unless the host asks
 * them to demodulate by the first hit's albedo (pt_set_denoise_albedo, below).  PT_TEXTURES together with PT_DIRECT_LIGHT is a
 * later change.
 * pt_set_texture: copies the texels to the device(s) -- every context of a session over several devices keeps its own copy;
 * texels == NULL or n == 0 removes that material's texture.  Session state: it survives pt_set_camera and pt_clear_image and
 * ends with pt_free.  The call synchronises the session and discards the PT_LOOKAHEAD windows, as pt_set_environment does, and
 * leaves the accumulation buffer alone.
 * pt_get_texture: the contract of pt_get_environment, per material.
 * PT_ERR_INVALID (both): before pt_init; a session without PT_TEXTURES; material outside [0, num_materials); n outside
 * [0, 1024]; texels == NULL with n > 0. */
int pt_set_texture(int material, const float *texels, int n);
int pt_get_texture(int material, float *texels, int capacity_texels, int *n);
/* host-only (no GPU): the texel index k of the steps above for each of `count` (primitive hit_geom[i], world point points[3 i ..])
 * pairs in a texture of n x n texels per face; -1 where the specification assigns none, and for mesh primitives.
 * PT_ERR_INVALID: a negative count, a null array with count > 0, a hit_geom entry outside [0, num_geoms), n outside [1, 1024]. */
int pt_texture_texel(const pt_geom *geoms, int num_geoms, const int32_t *hit_geom, const float *points, int count, int n, int32_t *index);

/* ---- bump mapping (PT_TEXTURES): one cube bump map per material perturbs the shading normal of spheres and cubes -------------
 * All arithmetic binary32, one rounding per operation in the order written, no FMA (tests/bump_model.py is the numpy form, and
 * the device's result equals it bit for bit).  A bump map has pt_set_texture's layout, 6 * n * n RGB
 * float32 texels with n in [1, 1024]; a texel is (da, db, unused): the two slopes added to the object-space normal along the
 * face's two in-plane axes (the negative height gradient, raw floats).  A material may carry a texture, a bump map, both or
 * neither.  At a hit with t > 0 on primitive g of type PT_SPHERE or PT_CUBE whose material has a bump map B of size n, with I
 * the ray's direction and nr the normal the intersection test reported:
 *   1  dot(I, nr) < 0 is false: not perturbed (the inside of a cube reports the exit face)
 *   2  P and q as for a texture (above)
 *   3  k = the texel of q, axis / negative = its major axis and sign; k < 0: not perturbed
 *   4  (da, db) = (B[k].r, B[k].g); da == 0 && db == 0: not perturbed (a NaN goes on)
 *   5  a < b the other two axes in x, y, z order.  Cube: u[axis] = negative ? -1 : 1, u[a] = da, u[b] = db.
 *      Sphere: u = q + q, then u[a] = u[a] + da, u[b] = u[b] + db
 *   6  w = multiplyMV(cube ? g.transform : g.invTranspose, (u, 0));  ns = normalize(w) = w * (1 / sqrt(dot(w, w)))
 *   7  dot(ns, nr) < 0: ns = -ns (a sphere hit from inside); then dot(ns, nr) > 0 is false: not perturbed
 *   8  dot(I, ns) < 0 is false: not perturbed
 * A perturbed hit is shaded with ns where nr stands (the glossy lobe, the mirror, the dielectric, the diffuse sampler; the same
 * engine, the same draws).  Then, for a survivor whose material is a mirror or is neither mirror nor dielectric, a new direction
 * with dot(dir, nr) > 0 false becomes reflect(dir, nr), not renormalised.  Everything else -- colours, origins, the emitter
 * and last-bounce exits, misses, meshes, the G-buffer's normals, pt_albedo, the filters, the ray counters -- is unchanged, and a
 * hit that is not perturbed is shaded exactly as without a map.  While a texture or a bump map is set the session runs a kernel
 * per bounce, as section 6.19 says of textures.
 * pt_set_bump_map / pt_get_bump_map: the contracts, refusals, synchronisation and per-context copies of pt_set_texture /
 * pt_get_texture.  The state survives pt_set_camera, pt_clear_image and pt_set_texture, ends with pt_free, and does not
 * invalidate the albedo plane.  PT_FAKE_SHADER ignores it. */
int pt_set_bump_map(int material, const float *texels, int n);
int pt_get_bump_map(int material, float *texels, int capacity_texels, int *n);
/* host-only (no GPU): steps 1-8 for each of `count` records (primitive hit_geom[i], world point points[3 i ..], reported normal
 * normals[3 i ..], ray direction dirs[3 i ..]) on one map of n x n texels per face: out_normals = ns and perturbed = 1 where the
 * hit is perturbed, out_normals = the reported normal and perturbed = 0 elsewhere and for mesh primitives.
 * PT_ERR_INVALID: what pt_texture_texel refuses, and a null texels, normals, dirs, out_normals or perturbed with count > 0. */
int pt_bump_normal(const pt_geom *geoms, int num_geoms, const int32_t *hit_geom, const float *points, const float *normals, const float *dirs,
                   int count, const float *texels, int n, float *out_normals, uint8_t *perturbed);

/* ---- smooth shading (PT_SMOOTH_NORMALS): per-vertex normals replace a mesh triangle's facet normal in the shader ---------------
 * All arithmetic binary32, one rounding per operation in the order written, no FMA (tests/smooth_model.py is the numpy form, and
 * the device's result equals it bit for bit).  The normals are world-space, as pt_triangle is: nine floats
 * n0, n1, n2 per triangle, indexed by the ORIGINAL triangle index (the order of pt_scene_desc::triangles) in both mesh modes.
 * They need not be unit vectors.  At a hit with t > 0 whose winner is triangle k of a mesh primitive, with (v0, e1 = fl(v1 - v0),
 * e2 = fl(v2 - v0)) as the device records hold them, the ray (o, I), nr the facet normal the intersection reported and n0, n1, n2
 * the normals of k:
 *   1  the barycentrics of glm::intersectRayTriangle as the intersection computed them:  p = cross(I, e2);  a = dot(e1, p);
 *      f = 1 / a;  s = o - v0;  bx = f * dot(s, p);  q = cross(s, e1);  by = f * dot(I, q);  bw = (1 - bx) - by
 *   2  w = (n0 * bw + n1 * bx) + n2 * by per component;  l2 = dot(w, w);  l2 not a finite number > 0: not smoothed (an all-zero
 *      triple therefore means "this triangle stays faceted")
 *   3  ns = w * (1 / sqrt(l2))
 *   4  dot(ns, nr) > 0 is false: not smoothed (meshes are one-sided: there is no flip)
 *   5  dot(I, ns) < 0 is false: not smoothed
 * A smoothed hit is shaded with ns where nr stands (the glossy lobe, the mirror, the dielectric, the diffuse sampler; the same
 * engine, the same draws).  Then the guard of bump mapping applies: a survivor whose material is a mirror or is neither mirror
 * nor dielectric and whose new direction has dot(dir, nr) > 0 false takes reflect(dir, nr), not renormalised.  Everything else --
 * colours, origins, t, outside, the emitter and last-bounce exits, misses, spheres and cubes, the ray counters, pt_stats -- is
 * unchanged, and a hit that is not smoothed is shaded exactly as without normals.  pt_gbuffer, pt_albedo and the filters keep the
 * FACET normal; handing them the shading normal is a later change.
 * pt_set_vertex_normals(normals, num_triangles): num_triangles must equal the session's; (NULL, 0) removes the normals.  The
 * call synchronises the session, discards the PT_LOOKAHEAD windows and leaves the accumulation buffer alone; the state survives
 * pt_set_camera and pt_clear_image and ends with pt_free; every context of a multi-device session keeps its own copy.
 * pt_get_vertex_normals: *num_triangles = the count set (0: none; `normals` may then be NULL); otherwise copies 9 floats per
 * triangle as they were set when capacity_triangles suffices.
 * PT_ERR_INVALID (both): before pt_init; a session without PT_SMOOTH_NORMALS; a count that differs from the session's; a null
 * array with a positive count (the getter: too small a capacity, a null num_triangles). */
int pt_set_vertex_normals(const float *normals, int num_triangles);
int pt_get_vertex_normals(float *normals, int capacity_triangles, int *num_triangles);
/* host-only (no GPU): steps 1-5 for each of `count` records (triangle tri[i], ray origins[3 i ..], dirs[3 i ..]) with nr the
 * facet normal normalize(cross(e1, e2)): out_normals = ns and smoothed = 1 where the hit is smoothed, out_normals = nr and
 * smoothed = 0 elsewhere.  The ray need not hit the triangle: the arithmetic is the same.
 * PT_ERR_INVALID: a negative count, a null array with count > 0, a tri entry outside [0, num_triangles). */
int pt_smooth_normal(const pt_triangle *triangles, const float *normals, int num_triangles, const int32_t *tri, const float *origins,
                     const float *dirs, int count, float *out_normals, uint8_t *smoothed);

/* ---- glossy reflection and frosted glass (PT_GLOSSY): SPECEX gives the specular surfaces a GGX lobe ------------------------
 * All arithmetic binary32, one rounding per operation in the order written, no FMA (tests/glossy_model.py is the numpy form,
 * and the device's result equals it bit for bit).
 *   alpha2  per material, on the host at pt_init: !(exponent > 0) -> 0, else (float)(2.0 / ((double)exponent + 2.0)).  0 means
 *           "no lobe" (exponent 0, negative, NaN; +inf rounds there).  pt_glossy_alpha2 below is that function.
 *   lobe(ng, rng, a2):  u1 = u01(rng), u2 = u01(rng);  keep = 1 - u1;  up = sqrt(keep / (keep + a2 * u1));  from over = sqrt(1 - up * up)
 *           on calculateRandomDirectionInHemisphere (interactions.h:10-42) verbatim -- the directionNotNormal choice on ng, the
 *           two normalised cross products, around = u2 * TWO_PI through the shared sin / cos, (up * ng + (cos * over) * p1) +
 *           (sin * over) * p2, not renormalised.  GGX normal sampling with alpha^2 = 2 / (exponent + 2): cos^2(theta) =
 *           (1 - u1) / (1 + (a2 - 1) u1), its denominator written as a sum of non-negative terms (no cancellation as u1 -> 1).
 *   at a hit on a mirror or dielectric with a2 > 0:  I = the ray's direction, n = the reported normal, ng = dot(I, n) > 0 ? -n : n;
 *           rng = makeSeededRandomEngine(iter, pixel, depth);  h = lobe(ng, rng, a2);  !(dot(I, h) < 0) -> h = ng.
 *   mirror: r = reflect(I, h);  !(dot(r, ng) > 0) -> r = reflect(I, ng) (a reflected ray never enters the surface it left);
 *           origin and colour as without the flag.
 *   dielectric: the branch of the completion spec with h in place of n (its face-forward step leaves h alone, `outside` is
 *           unchanged); the Fresnel choice is the engine's THIRD draw; whatever direction comes out is kept.
 *   everything else -- a2 == 0, diffuse, emitters, misses (with or without an environment map), the last bounce -- draws and
 *           computes what it does without the flag.
 * pt_glossy_alpha2: host only (no GPU); alpha2[i] for each of `count` exponents.  PT_ERR_INVALID: count < 0, a null array with
 * count > 0. */
int pt_glossy_alpha2(const float *exponents, int count, float *alpha2);

/* ---- direct lighting (PT_DIRECT_LIGHT): the last bounce aims at a sampled light ----------------------------------------------
 * With the flag and traceDepth D: bounces 0 .. D - 2 are today's; bounce D - 1 is today's last bounce except that a hit on a
 * diffuse surface survives with a ray aimed at a sampled point of a light and its colour multiplied by the sample's weight;
 * bounce D traces that final ray like any other and ends every path (DESIGN.md section 6.18 has the complete specification;
 * binary32, one rounding per operation in the order written, no FMA; tests/direct_model.py is its numpy form, and the device's
 * result equals it bit for bit).
 * Light elements, on the host at pt_init (binary64 on the binary32 entries of pt_geom::transform M, every stored value rounded
 * once), primitives in index order, only PT_SPHERE / PT_CUBE whose material has emittance > 0:
 *   cube:   six parallelograms, face f = 2 * axis + (negative side ? 1 : 0): c0 = M * (corner, 1), the corner with the face's
 *           coordinate (+-0.5) on `axis` and -0.5 on the other two; ea, eb = the columns of M of the other two axes in x, y, z
 *           order; normal = (ea x eb) / |ea x eb| signed away from the cube's centre; area = |ea x eb|.
 *   sphere: one element (c0, ea, eb, normal = 0); area = pi * |det M3|^(2/3), exact for a uniform scale, a selection mass otherwise.
 *   an element whose area is not a finite number > 0 is left out; cdf[e] = (running sum of the areas) / total, the last forced
 *   to 1.0f; inv_p[e] = total / area[e].  E = 0: the flag has no effect.  E > 1024: pt_init fails.
 * Sampling at a diffuse hit of bounce D - 1 (P = getPointOnRay's point, n = the reported normal, c = colour * material.color):
 *   rng = makeSeededRandomEngine(iter, pixel, D - 1); u0, u1, u2 = its first three draws; e = the smallest index with
 *   u0 < cdf[e] (E - 1 if none).
 *   parallelogram: y = (c0 + ea * u1) + eb * u2;  nl = normal;  A = area.
 *   sphere: z = 1 - 2 * u1;  r = sqrt(max(1 - z * z, 0));  (sin, cos) of u2 * TWO_PI by the shared sin / cos;
 *           s = 0.5 * (r * cos, r * sin, z);  y = multiplyMV(transform, (s, 1));  q = multiplyMV(invTranspose, (s, 0));
 *           len = sqrt(dot(q, q));  nl = q * (1 / len);  A = (float)(pi * |det M3|) * (len * 2) -- the exact area measure of
 *           the uniform object-space draw on any ellipsoid.
 *   v = y - P;  d2 = dot(v, v);  dir = v * (1 / sqrt(d2));  cs = dot(n, dir);  cl = -dot(nl, dir);  with o =
 *   multiplyMV(inverseTransform, (P, 1)): P is inside the element's primitive when every |o_k| < 0.5 (cube) / dot(o, o) < 0.25
 *   (sphere), and then cl = -cl (a scene enclosed in its light).
 *   any of d2 > 0, cs > 0, cl > 0 false (NaN is false): the path ends with colour 0, no ray is traced.  Otherwise
 *   w = ((cs * cl) * (A * inv_p[e])) / (d2 * (float)pi), colour = c * w, origin P, direction dir: one more bounce.
 * Final ray (bounce D): its target is the primitive of element e, recomputed from the same engine's first draw.  It scores
 *   colour *= material.color * emittance when t > 0 and the winning primitive (strict less, lowest index on ties) is the
 *   target; everything else -- another primitive in front, another emitter, a miss, with or without an environment map -- ends
 *   with colour 0 (PT_DIRECT_SKY, below, adds the sky's element and its rule).  Nothing draws at bounce D; the camera's engine slot stays D.
 * pt_light_elements: host only (no GPU), pt_init's own function.  Returns E, or the required count when `capacity` is too
 * small, in which case nothing is written; out may be NULL with capacity 0.  PT_ERR_INVALID: a negative count, a null array
 * with a positive count, an emitting candidate's materialid outside the table. */
typedef struct pt_light_element {
    int32_t geom, kind;            /* the primitive's index; PT_SPHERE or PT_CUBE (one face of it) */
    pt_vec3 c0, ea, eb, normal;    /* the parallelogram c0 + ea * u + eb * v and its outward unit normal; 0 for a sphere */
    float area, cdf, inv_p;
} pt_light_element;
int pt_light_elements(const pt_geom *geoms, int num_geoms, const pt_material *materials, int num_materials,
                      pt_light_element *out, int capacity);

/* ---- direct lighting samples the environment map (PT_DIRECT_SKY, with PT_DIRECT_LIGHT) ------------------------------------------
 * The device side is binary32, one rounding per operation in the order written, no FMA; the host tables are binary64 on the
 * binary32 texels, every stored value rounded once; tests/sky_model.py is the numpy form and the device equals it bit for bit.
 * Sampling tables, built on the host by pt_set_environment in a flagged session from the 6 n n texels.  Row r = face * n + j
 * (6 n rows), texel k = r * n + i.
 *   lum_k = (0.2126 r + 0.7152 g) + 0.0722 b of the texel, 0 where that is not a finite number > 0.
 *   J_k = 1 / (q sqrt(q)), q = (1 + ac ac) + bc bc, at the texel centre ac = (2 i + 1) / n - 1, bc likewise from j.
 *   m_k = lum_k J_k;  T = the sum of m_k in index order; T not a finite number > 0: there is no sky element.
 *   rows:    M_r = (sum over i of m_k, in order) + T / (16 * 6 n);  rowcdf[r] = (float)(running sum of M / its last value), the
 *            last forced to 1.0f;  rowinv[r] = (float)(1 / ((double)rowcdf[r] - (double)rowcdf[r - 1])), rowcdf[-1] = 0: the
 *            probability the ROUNDED table selects with.
 *   columns: within row r, c_k = m_k + (the row's sum) / (16 n), c_k = 1 when the row's sum is 0;  colcdf and colinv built
 *            from c as rowcdf and rowinv are from M, row by row.  The two 1/17 mixtures keep every row and column reachable.
 * Light table: with E lamp elements and a sky element a lamp's cdf is halved and its inv_p doubled; element E is the sky -- kind
 *   2, geom -1, cdf 1.0f, inv_p 2 (1 when E = 0) -- with K = (float)(4 / (pi n n)), s = (float)(2.0 / n) and n.  Up to 1024 lamp
 *   elements plus the sky.  pt_light_elements is unchanged.
 * Sampling at bounce D - 1: u0, u1, u2 as above; e = the smallest index with u0 < cdf[e].  A lamp proceeds as above.  The sky
 *   draws u3, u4:  r = the smallest index with u1 < rowcdf[r] (6 n - 1 if none);  i = the smallest with u2 < colcdf[r n + i]
 *   (n - 1 if none);  face = r / n, j = r % n, axis = face >> 1;  a = ((float)i + u3) * s - 1, b = ((float)j + u4) * s - 1;
 *   v[axis] = (face & 1) ? -1 : 1, the other two axes in x, y, z order get a, b (pt_environment_texel's mapping inverted);
 *   l2 = (1 + a a) + b b;  rl = 1 / sqrt(l2);  dir = v * rl;  Jd = (rl * rl) * rl;  cs = dot(n, dir).  cs > 0 false (NaN
 *   included): the path ends with colour 0.  Otherwise w = ((cs * Jd) * (rowinv[r] * colinv[r n + i])) * (K * inv_p[e]),
 *   colour = (colour * material.color) * w, origin P, direction dir, one more bounce.  No inside test, no cl.
 * Final ray (bounce D): the target of a sky-aimed ray is -1.  It scores when t > 0 is false: colour = the session's ordinary
 *   miss lookup on the direction as traced (whichever texel that reads) times colour.  Any hit ends it with 0; a lamp-aimed ray
 *   that misses still ends with 0.  Nothing draws at bounce D.
 * pt_sky_table: host only (no GPU), pt_set_environment's own function.  1: the map yields a sky element and row (6 n pairs
 * {cdf, inv}) and col (6 n n pairs, row by row) are written -- each may be NULL; 0: no element (n == 0 or texels == NULL
 * included), nothing written.  PT_ERR_INVALID: n outside [0, 1024], texels == NULL with n > 0. */
int pt_sky_table(const float *texels, int n, float *row, float *col);

/* pathtrace (pathtrace.cu:284-393): one iteration `iter` (1-based; RNG key and
 * tonemap divisor).  pbo_rgba: optional DEVICE pointer to W*H RGBA8 (the mapped
 * GL PBO in the reference), may be NULL.  host_image_sum: optional HOST buffer
 * of W*H*3 floats that receives the running sum (scene->state.image,
 * pathtrace.cu:389-390), may be NULL.  Synchronous: the buffer is complete
 * when the call returns, and belongs to the caller again (it may be freed).
 * With PT_PIN_IMAGE (see there) buffers of 1 MiB and more are page-locked on
 * first use and written by the kernel itself. */
int pt_trace(uint8_t *pbo_rgba, int frame, int iter, float *host_image_sum);

/* `count` consecutive iterations iter0..iter0+count-1 traced as one path pool
 * (count <= max_batch); bit-identical image to `count` pt_trace calls. */
int pt_trace_batch(int iter0, int count, float *host_image_sum);

/* Asynchronous form: enqueue only; pt_synchronize() waits.  Consecutive calls may OVERLAP on the device (each batch on
 * one of up to four launch streams with its own path pools; their memory is allocated on first use, within
 * PTMI355_OVERLAP_GB; PTMI355_OVERLAP=0 switches this off): the image is still summed in iteration order, bit for bit,
 * and everything enqueued afterwards on the session's stream -- pt_trace, pt_get_image, pt_tonemap, pt_synchronize --
 * comes after every batch enqueued before it. */
int pt_trace_batch_async(int iter0, int count);
int pt_synchronize(void);

/* ---- stepping interface (parity tests drive the loop bounce by bounce) ----- */
int pt_trace_begin(int iter0, int count);            /* generateRayFromCamera, pathtrace.cu:329 */
int pt_trace_bounce(int depth, int *n_live_after);   /* one pass of the loop body, :340-377 + 8.0 */
int pt_trace_end(void);                              /* finalGather, :380-381 */
/* current path pool as the reference's AoS (live prefix first); returns count */
int pt_export_paths(pt_path_segment *host_paths, int capacity, int *n_live);
/* ShadeableIntersection records of the last bounce (PT_UNFUSED / sort / fake-shader modes) */
int pt_export_intersections(pt_shadeable_intersection *host_isects, uint8_t *host_outside,
                            int capacity);
/* computeIntersections (pathtrace.cu:149-213) on caller-supplied rays: host AoS in,
 * host AoS out; runs the production intersect kernel. */
int pt_intersect_once(const pt_path_segment *host_paths, int n,
                      pt_shadeable_intersection *host_isects, uint8_t *host_outside);

/* ---- results ----------------------------------------------------------------- */
int pt_get_image(float *host_image_sum);             /* W*H*3 floats, running sum */
int pt_tonemap(uint8_t *host_rgba, int iter);        /* sendImageToPBO (pathtrace.cu:48-68) to host */
int pt_clear_image(void);
/* Resume an accumulation: the running sum becomes `host_image_sum` (W*H*3 floats, e.g. what pt_get_image / the host's
 * PFM dump returned after iteration k); tracing iterations k+1.. then yields, bit for bit, the image of the
 * uninterrupted run -- the running sum is the whole state the reference carries from one iteration to the next
 * (dev_image, pathtrace.cu:71,84,389; the iteration number is the caller's).  Synchronises the session first.  A PT_MOMENTS
 * session carries its two moment planes as well, which this call leaves alone: a host that resumes one calls pt_set_moments too. */
int pt_set_image(const float *host_image_sum);
float *pt_device_image(void);                        /* device pointer of the accumulation buffer */

/* ---- first-hit G-buffer and edge-avoiding A-trous filter (Dammertz et al. 2010) of the accumulated image -------------
 * What the course's next project adds to this renderer: a usable picture after 10-20 samples.  All arithmetic is binary32,
 * one rounding per operation, no FMA (DESIGN.md section 6.14 has the complete specification; tests/atrous_model.py is its
 * numpy form, and the device's result equals it bit for bit).
 * G-buffer: for every pixel of the CURRENT camera (pt_set_camera) the first hit of the reference's generateRayFromCamera
 * ray -- pinhole, unjittered, the same every iteration, also in sessions with PT_AA_JITTER or a lens -- found by the
 * production cull / exact-test code: t (-1 on a miss), surface normal, materialId (-1 on a miss) and position = origin +
 * direction * t (one multiply, one add per component; normal = position = 0 on a miss).  Computed once per camera and kept.
 * Filter: c_0 = running sum / (float)iter; level l = 0 .. levels - 1 is a 5 x 5 B3-spline kernel {1/16, 1/4, 3/8, 1/4, 1/16}^2 with
 * taps 2^l pixels apart (taps outside the image are skipped), each weighted by exp_neg(|dc|^2 / sc^2) exp_neg(|dn|^2 / sn^2)
 * exp_neg(|dp|^2 / sp^2) with sc = sigma_color * 2^-l, sn = sigma_normal, sp = sigma_position, normalised by the sum of
 * the weights.  levels = 0 returns the mean.
 * Both calls are synchronous, run on the session's stream after everything enqueued before them (asynchronous batches
 * included) and READ the session only: accumulation buffer, path pools, statistics and counters (G-buffer rays are not
 * counted), host image and the PT_LOOKAHEAD windows stay exactly as they were.  Their buffers (G-buffer, two colour
 * planes) are allocated on first use and released by pt_free.  Under PT_LOOKAHEAD the sum filtered is the one the last
 * served call left (what pt_get_image returns).
 * PT_ERR_INVALID: before pt_init; params == NULL; levels outside [0, 10]; a sigma that is not a finite number > 0 or whose
 * square at any level (sigma_color * 2^-l included) is not a normal binary32 number; iter < 1; a tiled session (tile_count > 1)
 * or one over several devices -- those hold a tile, not the frame; extending the filter to them is a later change. */
typedef struct pt_denoise_params { int32_t levels; float sigma_color, sigma_normal, sigma_position; } pt_denoise_params;
/* first hits of the current camera's pinhole rays; every output optional (host pointers): normals, positions W*H*3
 * floats, t W*H floats, material W*H int32 */
int pt_gbuffer(float *normals, float *positions, float *t, int32_t *material);
/* A-trous filter of the running sum after `iter` iterations; host_rgb (W*H*3 floats, the denoised MEAN) and
 * host_rgba (W*H*4 bytes: sendImageToPBO's rule with divisor 1) optional; the result also stays on the device */
int pt_denoise(const pt_denoise_params *params, int iter, float *host_rgb, uint8_t *host_rgba);
float *pt_denoised_device_image(void);   /* device pointer of the last result (W*H*3 floats), NULL before the first pt_denoise */

/* ---- the filter with history: what earlier cameras accumulated, reprojected through the G-buffers --------------------
 * A host that moves the camera (pt_set_camera + pt_clear_image) starts again at one sample per pixel, where the filter
 * has nothing to work with.  The pixels of a diffuse surface do not depend on the view: pt_denoise_temporal looks up, for
 * every pixel of the current camera, what the previous temporal call's camera had accumulated at the same surface point,
 * blends it in weighted by its sample count, and filters that (DESIGN.md section 6.15 has the complete specification,
 * binary32, one rounding per operation, no FMA; tests/temporal_model.py is its numpy form, equal bit for bit).
 * State: `cur` = {camera, G-buffer, colours C, sample counts N} of the last temporal call, and the history Hc, Hn in the
 * grid of cur's camera; none after pt_init and after pt_history_reset.  A call with the session's camera K:
 *   1. cur exists with other camera bytes than K: Hc, Hn = cur reprojected into K's grid.  Pixel P with first hit {n, p, t,
 *      mat} gets history only if mat >= 0 is neither reflective nor refractive; v = p - cur.position, z = dot(v, cur.view) > 0;
 *      fx = floorf(W * 0.5f - dot(v, cur.right) / (z * cur.pixelLength[0]) + 0.5f) in [0, W), fy likewise with up / H (the
 *      inverse of generateRayFromCamera, nearest pixel Q); cur's first hit at Q has the same material, a position within
 *      position_tolerance * t of p and a normal within normal_tolerance of n.  Then Hc[P] = C[Q], Hn[P] = min(N[Q],
 *      max_history); Hc[P] = Hn[P] = 0 otherwise.  The same camera bytes: Hc, Hn stay (this camera's samples are in the
 *      running sum; a pt_clear_image without a camera change drops them and keeps what came before).
 *   2. c0 = (sum + Hc * Hn) / ((float)iter + Hn) per channel; cur = {K, its G-buffer, C = c0, N = (float)iter + Hn}.
 *   3. pt_denoise's levels on c0.  With Hn = 0 everywhere the call equals pt_denoise bit for bit.
 * Synchronous, on the session's stream, and READS the session exactly as pt_denoise does; pt_denoise neither reads nor
 * disturbs the history, and the two may be interleaved freely.  80 bytes per pixel (a second G-buffer, two colour and two
 * length planes, the history) are allocated by the first temporal call and released by pt_free, which ends the history.
 * PT_ERR_INVALID: everything pt_denoise refuses; temporal == NULL; max_history outside [0, 1 << 20]; a tolerance that is
 * not a finite number > 0 or whose square is not a normal binary32 number; pt_history before the first temporal call. */
typedef struct pt_temporal_params {
    int32_t max_history;          /* cap on the sample count history may weigh in with, [0, 1 << 20]; 0 = history never used */
    float   position_tolerance;   /* relative to the hit distance t of the new view; finite, > 0 */
    float   normal_tolerance;     /* on |n_new - n_old|; finite, > 0 */
} pt_temporal_params;
/* pt_denoise with history: same outputs, same validation of `params`, same refusals (tiled / multi-device sessions) */
int pt_denoise_temporal(const pt_denoise_params *params, const pt_temporal_params *temporal, int iter,
                        float *host_rgb, uint8_t *host_rgba);
/* the history as the last pt_denoise_temporal used it, in the grid of that call's camera; both optional host pointers:
 * rgb W*H*3 floats, length W*H floats (0 = no history for the pixel) */
int pt_history(float *rgb, float *length);
int pt_history_reset(void);       /* forget everything; the next temporal call equals pt_denoise bit for bit */

/* ---- the filters on irradiance: first-hit albedo demodulation ---------------------------------------------------------------
 * A texture on a flat wall has one normal and one plane: only the colour stop keeps its texels apart, and at 16-64 samples
 * that stop sits inside the noise.  With the switch on, pt_denoise and pt_denoise_temporal filter colour / albedo and return
 * filtered * albedo (DESIGN.md section 6.20 has the complete specification; tests/albedo_model.py is its numpy form, equal bit
 * for bit).  All arithmetic binary32, one rounding per operation in the order written, no FMA.
 * Albedo plane A[P], for pixel P of the current camera, from the G-buffer's first hit (pinhole, unjittered, production cull and
 * exact tests, the winner by strict less with the lowest index on ties):
 *   a miss (!(t > 0)): (1, 1, 1);  a material with hasReflective > 0 or hasRefractive > 0 (the shader's tests): (1, 1, 1) --
 *   such a pixel shows another surface and material.color does not multiply it;
 *   every other hit, diffuse or emitter: v = mcol, the colour the shader puts where material.color stands -- the texture
 *   section's mcol (P = getPointOnRay's point, not the G-buffer's position) on a sphere or cube while the session launches its
 *   textured kernels (PT_TEXTURES without PT_FAKE_SHADER, at least one texture set), plain material.color everywhere else
 *   (meshes, PT_FAKE_SHADER, no texture set);  then per component a = fminf(fmaxf(v, 2^-6), 2^6) -- C's fmaxf / fminf: a NaN
 *   gives 2^-6.  (A texel below 1/64 therefore receives up to 1/64 of its neighbours' irradiance; the upper clamp keeps
 *   inf * 0 out.)
 * The plane is recomputed when the camera's bytes differ from those it was made for and after a pt_set_texture that changed
 * a texel or a size; it is kept otherwise.  12 bytes per pixel, allocated on first use, released by pt_free.
 * pt_denoise with the switch on, levels >= 1: c_0[P] = (sum[P] / (float)iter) / A[P] per component (two divides, the mean
 * first); the levels as above on c -- the colour stop compares demodulated colours, the sigmas are unchanged --; the result is
 * c_levels[P] * A[P], and the RGBA bytes come from that.  levels = 0 returns the mean untouched.
 * pt_denoise_temporal with the switch on: steps 1 and 2 are unchanged -- history, blend, cur.C and pt_history stay in
 * modulated colour (a diffuse surface's colour, texture included, does not depend on the view) --; step 3 filters c0 / A and
 * multiplies back as above; levels = 0 returns c0.
 * Where A is 1 in every component of every pixel the results equal those of the switch off bit for bit (x / 1 * 1), and
 * switching on and off again restores them bit for bit.  A switched-on call still launches one kernel per level (the first
 * divides as it loads, the last multiplies as it stores) and the G-buffer kernel only when the plane is stale.
 * pt_set_denoise_albedo: 0 / 1; off after pt_init.  Session state: it survives pt_set_camera, pt_clear_image and
 * pt_set_texture and ends with pt_free.  pt_albedo: the plane of the current camera as the filter would use it, whatever the
 * switch says (rgb: W*H*3 floats, host; NULL computes the plane and copies nothing).  Both are synchronous, sit on the
 * session's stream behind everything enqueued, and like pt_gbuffer read the session and change nothing in it: no
 * PT_LOOKAHEAD window is discarded and no counter moves.
 * PT_ERR_INVALID (both): before pt_init; a tiled session (tile_count > 1) or one over several devices; enable outside {0, 1}.
 * Out of scope: demodulating by specular.color or by the albedo seen through a mirror or glass; history kept demodulated. */
int pt_set_denoise_albedo(int enable);
int pt_albedo(float *rgb);

/* ---- the filter steered by the pixels' own noise: per-pixel luminance moments (PT_MOMENTS) ------------------------------------
 * pt_denoise's colour stop is a constant in absolute radiance units that fits one scene, sample count and exposure.  A session
 * with PT_MOMENTS measures every pixel's noise instead, and pt_denoise_variance stops at a multiple of it -- the core of SVGF
 * (Schied et al. 2017) on top of Dammertz' filter (DESIGN.md section 6.27 has the complete specification; tests/variance_model.py
 * is its numpy form, equal bit for bit).  All arithmetic binary32, one rounding per operation in the order written, no FMA;
 * lum(c) = (0.2126f * c.r + 0.7152f * c.g) + 0.0722f * c.b;  n = (float)iter.
 * Moments: see PT_MOMENTS above.  pt_get_moments copies them to the host (W*H floats each, either pointer may be NULL) and
 * synchronises like pt_get_image; pt_set_moments replaces them (both pointers required) and is the companion of pt_set_image:
 * pt_set_image leaves the moments alone, so a host that RESUMES an accumulation calls BOTH.  pt_clear_image zeroes the moments
 * with the sum; pt_set_camera leaves them alone, as it does the sum.  PT_ERR_INVALID: before pt_init; a session without the
 * flag; a NULL pointer to pt_set_moments.
 * Filter:  c_0[P] = sum[P] / n per channel;  mu = M1[P] / n;  var_0[P] = fmaxf(M2[P] / n - mu * mu, 0) / fmaxf(n - 1, 1) -- the
 * variance of the MEAN; iter = 1 gives exactly 0.  Level l = 0 .. levels - 1, step s = 2^l, on (c, var):
 *   gv[P]  = the 3 x 3 Gaussian {1/4, 1/2, 1/4}^2 of var around P: acc = acc + var[Q] * (g[dy] * g[dx]) from 0, dy outer, the
 *            coordinates of Q clamped to the image, none skipped;
 *   den[P] = sigma_luminance * sqrt(fmaxf(gv[P], 2^-40)), the root correctly rounded;
 *   for the 5 x 5 taps Q = P + (dx s, dy s) of pt_denoise's kernel h, dy outer, those outside the image skipped:
 *     w = exp_neg(fabsf(lum(c[P]) - lum(c[Q])) / den[P]) * exp_neg(|dn|^2 / sn^2) * exp_neg(|dp|^2 / sp^2);  wt = w * (h[dy] * h[dx]);
 *     sum += c[Q] * wt per channel;  vsum += var[Q] * (wt * wt);  cum += wt;
 *   c'[P] = sum / cum;  var'[P] = vsum / (cum * cum).
 * sigma_luminance is NOT halved per level: the variance it multiplies shrinks by itself as the levels average.  levels = 0
 * returns the mean (and var_0 through pt_variance).  The RGBA bytes follow pt_denoise's rule.  Denormal intermediates (l * l of
 * a nearly black sample) follow IEEE; the floor 2^-40 keeps them out of every divisor.  With iter = 1 every den is
 * sigma_luminance * 2^-20 and only taps of equal luminance pass: the first sample of a view is pt_denoise's business.
 * pt_denoise_variance shares pt_denoise's contract: synchronous, on the session's stream behind everything enqueued; it READS the
 * session and changes nothing in it (no counter moves); its buffers (48 bytes per pixel) are allocated on first use and released
 * by pt_free; it uses the same G-buffer, computed once per camera; the result stays on the device, where
 * pt_denoised_device_image returns it; it neither reads nor disturbs pt_denoise's planes or the temporal history.  It IGNORES the
 * pt_set_denoise_albedo switch: demodulation would need the moments of demodulated luminance, a later change.  One launch per
 * level.  pt_variance: var_0 of the last pt_denoise_variance call's input (W*H floats, host; NULL copies nothing).
 * PT_ERR_INVALID: everything pt_denoise refuses (before pt_init; params == NULL; levels outside [0, 10]; iter < 1; sigma_normal or
 * sigma_position not a finite number > 0 or with a square that is not a normal number; tiled / multi-device sessions); a session
 * without PT_MOMENTS; sigma_luminance not a finite number > 0, or sigma_luminance * 2^-20 not a normal binary32 number;
 * pt_variance before the first pt_denoise_variance call.
 * Out of scope: moments in tiled or multi-device sessions and under PT_LOOKAHEAD windows; albedo-demodulated variance.
 * (Temporal accumulation of the moments across camera moves and SVGF's spatial variance estimate: pt_denoise_svgf below.) */
typedef struct pt_variance_params { int32_t levels; float sigma_luminance, sigma_normal, sigma_position; } pt_variance_params;
int pt_get_moments(float *m1, float *m2);
int pt_set_moments(const float *m1, const float *m2);
int pt_denoise_variance(const pt_variance_params *params, int iter, float *host_rgb, uint8_t *host_rgba);
int pt_variance(float *host_var);

/* ---- SVGF: the moments reprojected with the colour, and a spatial variance estimate where the history is short -------------------
 * pt_denoise_temporal carries colour across camera moves but stops at a constant; pt_denoise_variance stops at the measured noise
 * but its moments start again with every view, and the first sample has no variance at all.  pt_denoise_svgf joins them (Schied et
 * al. 2017; DESIGN.md section 6.28 has the complete specification; tests/svgf_model.py is its numpy form, equal bit for bit).
 * Binary32, one rounding per operation in the order written, no FMA, C's fmaxf; lum, exp_neg, d2, the kernel h and the
 * reprojection tests are those of pt_denoise, pt_denoise_temporal and pt_denoise_variance.
 * State, its own (not pt_denoise_temporal's): cur = {camera bytes, G-buffer, C[.,3], U1, U2, N} and the history planes Hc, H1, H2,
 * Hn; after pt_init and after pt_svgf_reset there is no cur and every history plane is 0.  A call with the session's camera K, its
 * G-buffer g and n = (float)iter:
 *   1. cur exists with other camera bytes than K: pt_denoise_temporal's reprojection of cur, the same tests in the same order; on
 *      success Hc[P] = C[Q], H1[P] = U1[Q], H2[P] = U2[Q], Hn[P] = min(N[Q], (float)max_history), otherwise all four are 0.  The same
 *      camera bytes: the history stays.
 *   2. N' = n + Hn;  c0 = (sum + Hc * Hn) / N' per channel;  u1 = (M1 + H1 * Hn) / N';  u2 = (M2 + H2 * Hn) / N'.
 *   3. vt = fmaxf(u2 - u1 * u1, 0) / fmaxf(N' - 1, 1).  Where N'[P] < (float)spatial_below, var_0[P] is the spatial estimate: over the
 *      taps Q = P + (dx, dy), dy = -3 .. 3 outer, dx = -3 .. 3, those outside the image skipped, w = exp_neg(|dn|^2 / sn^2) *
 *      exp_neg(|dp|^2 / sp^2) (the levels' squares), s1 += u1[Q] * w, s2 += u2[Q] * w, cum += w from 0; a = s1 / cum, b = s2 / cum;
 *      var_0[P] = fmaxf(b - a * a, 0) / N'[P].  Elsewhere var_0 = vt.
 *   4. cur = {K, g, C = c0, U1 = u1, U2 = u2, N = N'}: the history is never filtered.
 *   5. pt_denoise_variance's levels on (c0, var_0), sigma_luminance not halved; levels = 0 returns c0.  RGBA bytes by pt_denoise's rule.
 * With spatial_below = 0 and no history the call equals pt_denoise_variance bit for bit at every iter; C and N equal the planes of a
 * pt_denoise_temporal sequence with the same parameters and calls.  spatial_below = 4 is SVGF's value.
 * pt_denoise_variance's contract: synchronous, on the session's stream behind everything enqueued; READS the session and changes
 * nothing in it; ignores the albedo switch; the result stays on the device for pt_denoised_device_image; 100 bytes per pixel (cur
 * with a copy of its G-buffer, the history, the records level 0 reads, var_0) beside the planes it shares with
 * pt_denoise_variance are allocated on first use and released by pt_free, which ends the history.  pt_clear_image, pt_set_image,
 * pt_set_moments and pt_set_camera do not touch the state, and the four filters may be interleaved freely: each returns what it
 * would have returned without the others, pt_history and pt_variance keep reporting their own calls.
 * pt_svgf_history: Hc, H1, H2, Hn as the last call used them (host; every pointer optional; W*H*3, W*H, W*H, W*H floats).
 * pt_svgf_variance: var_0 as the levels of the last call received it (W*H floats, host; NULL copies nothing).  pt_svgf_reset:
 * forget everything.
 * PT_ERR_INVALID, in this order: everything pt_denoise_variance refuses (a session without PT_MOMENTS included); everything
 * pt_denoise_temporal refuses in `temporal`; spatial_below outside [0, 1 << 20]; pt_svgf_history or pt_svgf_variance before the
 * session's first pt_denoise_svgf call. */
int pt_denoise_svgf(const pt_variance_params *params, const pt_temporal_params *temporal, int spatial_below, int iter,
                    float *host_rgb, uint8_t *host_rgba);
int pt_svgf_history(float *rgb, float *u1, float *u2, float *length);
int pt_svgf_variance(float *host_var);
int pt_svgf_reset(void);
int pt_get_stats(pt_stats *stats);
/* rays traced since pt_init, read from the device-side counter (includes
 * asynchronous batches); synchronises the stream.  Negative = pt_status. */
long long pt_total_rays(void);
/* the same counter plus the paths traced at bounce 0 (rays - first = paths that survived a
 * compaction) and the iterations traced */
int pt_get_counters(int64_t *rays, int64_t *first_bounce_rays, int64_t *iterations);

/* Per-kernel timing with HIP events recorded on the launch stream (bench.py's
 * roofline leg).  Off by default; when on, every launch of the per-bounce
 * kernels is bracketed by two events from a preallocated pool. */
enum pt_stage { PT_STAGE_RAYGEN = 0, PT_STAGE_BOUNCE = 1, PT_STAGE_INTERSECT = 2,
                PT_STAGE_SORT = 3, PT_STAGE_GATHER = 4, PT_STAGE_MESH = 5, PT_STAGE_COUNT = 6 };
typedef struct pt_profile {
    double  ms[PT_STAGE_COUNT];        /* summed event-elapsed time per stage */
    int64_t launches[PT_STAGE_COUNT];  /* launches measured; PT_STAGE_BOUNCE: bounces measured -- the one launch that
                                        * does a batch's bounces 0 and 1 counts as two */
} pt_profile;
int pt_set_profiling(int enable);      /* also clears the accumulated profile */
int pt_get_profile(pt_profile *out);   /* synchronises the stream, drains pending events */
/* PT_MESH_BVH: what pt_init built (all meshes together) */
typedef struct pt_bvh_info {
    int32_t nodes, triangles, depth;
    float   pad;                       /* box padding, world units (= 2 x the pad of the spec's hit-point test) */
    float   prune;                     /* additive slack of the distance prune: 0 (none is needed, csrc/pt_bvh.hpp) */
} pt_bvh_info;
int pt_get_bvh_info(pt_bvh_info *out);
/* host-only (no GPU): build the hierarchy of `count` triangles; returns the node count, or the
 * required count when `node_capacity` is too small (nothing written then).  nodes: 16 dwords
 * each (layout in csrc/pt_bvh.hpp); order: leaf slot -> triangle index; grid (8 floats,
 * optional): origin xyz, step xyz of the 16-bit box grid, box padding, prune margin. */
int pt_bvh_build(const pt_triangle *triangles, int count, float *nodes, int node_capacity,
                 int32_t *order, float *grid);
/* host-only (no GPU): the world-space cull boxes pt_init derives for `count` primitives seen from `eye` (3 floats,
 * may be NULL): boxes = count x {lo.xyz, hi.xyz}; *origin_bound = the |origin|_1 up to which they hold.  A ray
 * outside a primitive's box is never handed to the exact test (csrc/pt_cull.hpp has the error bound that makes
 * this identical to the reference's loop over every primitive, pathtrace.cu:176-199).  reject (optional) = count x
 * {mode (0..2 diagonal row k, 4 general row, 3 none), m_k0, m_k1, m_k2, m_k3}: the row of the inverseTransform the
 * kernel's exact one-axis early miss evaluates for cubes (same file). */
int pt_cull_boxes(const pt_geom *geoms, int count, const float *eye, float *boxes, float *origin_bound, float *reject);
/* host-only (no GPU): the per-triangle spheres of the every-triangle loop's first stage for ONE mesh of `count` triangles and
 * ray origins with |origin|_1 <= origin_bound: bounds = ((count + 3) & ~3) x {centre xyz, Rs^2} (padding entries: Rs^2 = -1).
 * A ray whose line passes a centre at more than Rs is never accepted for that triangle by the completion spec
 * (glm::intersectRayTriangle + the hit-point test; csrc/pt_h_scene.hpp: make_tri_bounds has the derivation), so the kernel
 * does not run the exact test for the pair.  Returns the number of entries written. */
int pt_tri_bounds(const pt_triangle *triangles, int count, float origin_bound, float *bounds);
/* host-only (no GPU): the same spheres as the every-triangle loop's first stage reads them -- it evaluates "line passes the centre
 * at more than Rs" on the matrix pipe (v_mfma_f32_16x16x32_f16) as ONE bilinear form per (ray, triangle) pair, in the mesh's own
 * frame (centre g, scale 1 / Rm: every sphere in the unit ball): records = ((count + 63) & ~63) x 32 binary16 K-slots (the triangle's
 * side of the form: csrc/pt_h_scene.hpp: make_tri_records; padding records reach nobody), frame = {gx, gy, gz, 1 / Rm}.  The ray's
 * side and the error budget: csrc/pt_k_trisweep.hpp.  Returns the number of records written. */
int pt_tri_records(const pt_triangle *triangles, int count, float origin_bound, uint16_t *records, float frame[4]);
/* ---- known-answer probes: the DEVICE's own arithmetic on caller data (no session needed, any HIP device) -------
 * pt_probe_rng: thrust::default_random_engine (minstd_rand) as makeSeededRandomEngine constructs it
 * (pathtrace.cu:41-45 -> engine(seed)): for each of the n seeds, seed the engine and draw `draws` times through
 * uniform_real_distribution<float>(0,1) (csrc/pt_device.hpp: lcg_seed, u01); state[i] = the engine's state after the
 * last draw, u[i] = the last draw's value (both optional).  Known answer (C++ [rand.predef]): seed 1, 10 000 draws ->
 * state 399268537.
 * pt_probe_sincos: the shared sin / cos of calculateRandomDirectionInHemisphere (interactions.h:40-41; DESIGN.md
 * section 4) for n arguments, or -- x == NULL -- for the `n` consecutive binary32 values that start at bit pattern
 * `first_bits`, reduced to sum[0] = sum over k of bits(sin) * (2k + 1), sum[1] = the same for cos (mod 2^64): the
 * oracle computes the same two sums on the CPU, so every float of [0, 2 pi] can be compared without moving 9 GB.
 * pt_probe_hemisphere: calculateRandomDirectionInHemisphere (interactions.h:10-42) for n (normal, engine seed)
 * pairs; dirs = n x 3 floats.
 * pt_probe_sqrt: the kernels' sqrt and 1 / sqrt (glm::length / glm::normalize, func_geometric.inl:94-100,153-159:
 * Newton's iteration on v_rsq_f32, csrc/pt_device.hpp: sqrt_newton) against the correctly rounded sqrtf and divide, for
 * the `n` consecutive binary32 values from bit pattern `first_bits` on: mismatch[0] = arguments whose root differs,
 * mismatch[1] = whose reciprocal of the root differs.  Zero for every x in [2^-102, 2^128).  For x in [1 - 2^-12, 1 + 2^-12]
 * the reciprocal is the kernels' four-addition form for vectors that are unit vectors up to rounding (rsqrt_near_one). */
/* pt_probe_clock: the shader clock (GHz) the device holds WHILE whatever is enqueued runs -- one wave counts its cycle counter
 * against the constant 100-MHz counter for `microseconds` on a stream of its own, beside the session's launches (bench.py's
 * `sustained` object: the issue roof is priced at the 2.4 GHz peak, the chip holds 2.1-2.2 under this library's kernels). */
int pt_probe_clock(int microseconds, double *ghz);
int pt_probe_rng(const uint32_t *seeds, int n, int draws, uint32_t *state, float *u);
int pt_probe_sincos(const float *x, uint32_t first_bits, uint32_t n, float *s, float *c, uint64_t sum[2]);
int pt_probe_hemisphere(const float *normals, const uint32_t *seeds, int n, float *dirs);
int pt_probe_sqrt(uint32_t first_bits, uint32_t n, uint64_t mismatch[2]);
/* pt_probe_shade_scatter: one pass of the loop body's shader (pathtrace.cu:224-266 with scatterRay completed)
 * on n caller-supplied (path, intersection) pairs, through the kernels' own shade_scatter (csrc/pt_device.hpp): mirror, Fresnel
 * dielectric, total internal reflection, diffuse, emitter, miss and the last bounce, one lane per pair.  paths (in / out), isects,
 * outside (n bytes: the winning test's `outside`; NULL = 1 for every path) and materials are host arrays.  Per path: remainingBounces
 * <= 0 -> untouched; t > 0 on an emitter -> color *= material.color * emittance, remainingBounces = 0; t > 0 otherwise -> scattered
 * with the engine keyed by (iter, pixelIndex, depth), remainingBounces -= 1, and color = 0 when that reaches 0; t <= 0 -> color = 0,
 * remainingBounces = 0.  A path that ends keeps the ray it came with (the oracle's pto_shade_scatter scatters before it zeroes a
 * last-bounce path: compare `ray` where remainingBounces > 0 afterwards, everything else for every path).  deferred = 0: the call
 * of the kernels that sample a diffuse direction at once; 1: the deferring kernels' call, followed by what the next bounce's load
 * does with a pending direction (csrc/pt_k_bounce.hpp: tile_load) -- the same bytes.  Refused on the host, before anything is
 * launched (PT_ERR_INVALID): n < 0 or above 2^26, a null array with n > 0, num_materials < 1, deferred outside {0, 1}, a record
 * with t > 0 whose materialId is outside [0, num_materials).  n == 0 launches nothing. */
int pt_probe_shade_scatter(int iter, int depth, const pt_material *materials, int num_materials, pt_path_segment *paths,
                           const pt_shadeable_intersection *isects, const uint8_t *outside, int n, int deferred);
/* pt_probe_glossy_lobe: the device's lobe (PT_GLOSSY above; csrc/pt_device.hpp: lobe) for n (normal, engine seed, alpha2) triples,
 * one lane per element, seeded like pt_probe_hemisphere; dirs = n x 3 floats.  PT_ERR_INVALID: n < 0, a null array with n > 0.
 * pt_probe_shade_scatter_glossy: pt_probe_shade_scatter -- its signature, contract and refusals -- through the glossy form of
 * shade_scatter, the one a PT_GLOSSY session's kernels call; alpha2 comes from the materials' exponents as at pt_init.  With every
 * exponent 0 (or any value that means "no lobe") the same bytes as pt_probe_shade_scatter. */
int pt_probe_glossy_lobe(const float *normals, const uint32_t *seeds, const float *alpha2, int n, float *dirs);
int pt_probe_shade_scatter_glossy(int iter, int depth, const pt_material *materials, int num_materials, pt_path_segment *paths,
                                  const pt_shadeable_intersection *isects, const uint8_t *outside, int n, int deferred);
/* pt_probe_environment: the miss exit's lookup and multiply (pt_set_environment above) through the kernels' own device function, one
 * lane per (direction, throughput) pair: colour[i] = throughput[i] * E(dirs[i]) per component (all count x 3 floats), +0 when n == 0.
 * texels as for pt_set_environment.  PT_ERR_INVALID: count < 0, a null array with count > 0, n outside [0, 1024], texels == NULL
 * with n > 0.  count == 0 launches nothing. */
int pt_probe_environment(const float *texels, int n, const float *dirs, const float *throughput, int count, float *colour);
/* pt_probe_texture: PT_TEXTURES' lookup and multiply (above) through the function the kernels call, one lane per record:
 * colour_out = colour_in * T[k], or colour_in where k < 0 or the primitive is a mesh.  No session is needed; count == 0 launches
 * nothing.  PT_ERR_INVALID: the refusals of pt_texture_texel, texels == NULL, count above 2^26.
 * pt_probe_shade_scatter_textured: pt_probe_shade_scatter's signature, contract and refusals through the textured form of
 * shade_scatter as the kernels of a PT_TEXTURES session call it, with the primitives (geoms, hit_geom: n int32, -1 for records with
 * t <= 0) and a texture table as parallel arrays: tex_texels (all textures back to back), tex_n[num_materials] (0 = none),
 * tex_offset[num_materials] (in texels).  A record with t > 0 must name a primitive inside the table. */
int pt_probe_texture(const pt_geom *geoms, int num_geoms, const int32_t *hit_geom, const float *points, int count, const float *texels, int n,
                     const float *colour_in, float *colour_out);
int pt_probe_shade_scatter_textured(int iter, int depth, const pt_material *materials, int num_materials, pt_path_segment *paths,
                                    const pt_shadeable_intersection *isects, const uint8_t *outside, int n, int deferred,
                                    const pt_geom *geoms, int num_geoms, const int32_t *hit_geom, const float *tex_texels,
                                    const int32_t *tex_n, const int32_t *tex_offset);
/* pt_probe_bump_normal: pt_bump_normal's arguments, results and refusals (plus count above 2^26) through the function the kernels
 * call, one lane per record.  No session is needed; count == 0 launches nothing.
 * pt_probe_shade_scatter_bumped: pt_probe_shade_scatter_textured plus a bump table as parallel arrays -- bump_texels (all maps
 * back to back, RGB), bump_n[num_materials] (0 = none), bump_offset[num_materials] (in texels) -- through the whole textured
 * form as the kernels call it while a bump map is set: lookup, shader about the perturbed normal, guard, and no deferral on
 * perturbed lanes (deferred = 0 and 1 give the same bytes there). */
int pt_probe_bump_normal(const pt_geom *geoms, int num_geoms, const int32_t *hit_geom, const float *points, const float *normals, const float *dirs,
                         int count, const float *texels, int n, float *out_normals, uint8_t *perturbed);
int pt_probe_shade_scatter_bumped(int iter, int depth, const pt_material *materials, int num_materials, pt_path_segment *paths,
                                  const pt_shadeable_intersection *isects, const uint8_t *outside, int n, int deferred,
                                  const pt_geom *geoms, int num_geoms, const int32_t *hit_geom, const float *tex_texels,
                                  const int32_t *tex_n, const int32_t *tex_offset, const float *bump_texels, const int32_t *bump_n,
                                  const int32_t *bump_offset);
/* pt_probe_smooth_normal: pt_smooth_normal's arguments, results and refusals (plus count above 2^26) through the function the
 * kernels call (csrc/pt_smooth.hpp: smooth_normal), one lane per record.  No session is needed; count == 0 launches nothing. */
int pt_probe_smooth_normal(const pt_triangle *triangles, const float *normals, int num_triangles, const int32_t *tri, const float *origins,
                           const float *dirs, int count, float *out_normals, uint8_t *smoothed);
/* pt_probe_direct_sample: PT_DIRECT_LIGHT's sampler (above; csrc/pt_device.hpp: direct_sample) on the device through the function
 * the kernels call, one lane per record: for each of `count` (P, n, engine seed) triples (P, n: count x 3 floats; seeded like
 * pt_probe_hemisphere) the direction (count x 3), the weight and the element picked, on the light table of the scene given as for
 * pt_light_elements.  weight = 0 and dir = 0 where the path would end (step 6).  A scene without elements: weight 0, dir 0,
 * element -1, nothing launched.  Refusals as pt_probe_shade_scatter's: count < 0 or above 2^26, a null array with count > 0,
 * num_materials < 1, what pt_light_elements refuses, more than 1024 elements.  count == 0 launches nothing.
 * pt_probe_shade_scatter_direct: pt_probe_shade_scatter's contract through the direct form of shade_scatter, as the kernels of a
 * PT_DIRECT_LIGHT session of traceDepth `trace_depth` call it at bounce `depth` in [0, trace_depth].  The bounce, not
 * remainingBounces, says where a path is: remainingBounces <= 0 -> untouched; a survivor leaves with remainingBounces =
 * trace_depth - depth (what pt_export_paths shows), a path that ends with 0.  depth < trace_depth - 1: the plain scatter;
 * depth == trace_depth - 1: the sampling bounce; depth == trace_depth: the final ray -- hit_geom[i] (n int32, the winning
 * primitive's index, -1 for a miss; read at this depth only, may be NULL otherwise) decides whether it scores. */
int pt_probe_direct_sample(const pt_geom *geoms, int num_geoms, const pt_material *materials, int num_materials, const float *P,
                           const float *n, const uint32_t *seeds, int count, float *dir, float *weight, int32_t *element);
int pt_probe_shade_scatter_direct(int iter, int depth, int trace_depth, const pt_geom *geoms, int num_geoms, const pt_material *materials,
                                  int num_materials, pt_path_segment *paths, const pt_shadeable_intersection *isects,
                                  const uint8_t *outside, const int32_t *hit_geom, int n);
/* pt_probe_sky_sample: PT_DIRECT_SKY's branch of the sampler on the device through the function the kernels call, one lane per
 * (normal, engine seed) record (normals: count x 3 floats; seeded like pt_probe_hemisphere), on a table whose only element is
 * the sky of the map (texels, n): the direction (count x 3), the weight and the texel r * n + i drawn.  weight = 0 and dir = 0
 * where the path would end (cs > 0 false; the texel is still reported).  A map without an element (n == 0 included): weight 0,
 * dir 0, texel -1, nothing launched.  PT_ERR_INVALID: n outside [0, 1024], texels == NULL with n > 0, count < 0 or above 2^26,
 * a null array with count > 0.
 * pt_probe_shade_scatter_direct_sky: pt_probe_shade_scatter_direct on the light table of a PT_DIRECT_SKY session under the map
 * (texels, env_n; env_n == 0: no map, pt_probe_shade_scatter_direct itself).  At depth == trace_depth a ray aimed at the sky scores
 * the map where isects[i].t > 0 is false and ends with 0 on any hit.  (As in pt_probe_shade_scatter_direct a miss at an earlier
 * depth ends with colour 0: the pipelines' miss exit is pt_probe_environment's.)  Refusals as pt_probe_shade_scatter_direct's,
 * and env_n outside [0, 1024] or texels == NULL with env_n > 0. */
int pt_probe_sky_sample(const float *texels, int n, const float *normals, const uint32_t *seeds, int count, float *dir, float *weight,
                        int32_t *texel);
int pt_probe_shade_scatter_direct_sky(int iter, int depth, int trace_depth, const pt_geom *geoms, int num_geoms, const pt_material *materials,
                                      int num_materials, pt_path_segment *paths, const pt_shadeable_intersection *isects,
                                      const uint8_t *outside, const int32_t *hit_geom, int n, const float *texels, int env_n);
/* pt_probe_tri_form: the every-triangle loop's first stage on the device, through the kernel's own code (csrc/pt_k_trisweep.hpp:
 * tri_ray_operands, tri_group_form), for ONE mesh of `count` triangles (records and frame as pt_tri_records makes them) and n rays
 * (origins, directions: n x 3 floats each; rays with |origin|_1 > origin_bound are `wild` as in the kernels).  Per ray (each output
 * optional): ray_slots = its 32 binary16 K-slots, ray_class = 0 plain, 1 far (its line passes the unit ball at a distance), 2 wild;
 * form = n x ((count + 63) & ~63) binary32 results of v_mfma_f32_16x16x32_f16, one per (ray, record), padding records included:
 * the pair is a candidate when the sign bit is set.  Returns the record count; count == 0 launches nothing. */
int pt_probe_tri_form(const pt_triangle *triangles, int count, float origin_bound, const float *origins, const float *directions, int n,
                      uint16_t *ray_slots, int32_t *ray_class, float *form);
/* pt_probe_own_surface_plan: the launch plan's decision (host only, no device) whether a batch of `paths` paths of a scene
 * of `ngeoms` primitives takes the own-surface form of the fused bounce kernel's cull -- the primitive a path has just left
 * travels in bits 26..29 of its pid as geom + 1 -- given that the pipeline is the plain fused compacting one (plain_fused:
 * PT_COMPACT without PT_UNFUSED, PT_SORT_MATERIAL, PT_CACHE_FIRST or triangle meshes).  1: yes, 0: no. */
int pt_probe_own_surface_plan(uint64_t paths, int ngeoms, int plain_fused);
/* devices of the current session (0: not initialised) and how their tiles reach devices[0]: "rccl", "peer"
 * (hipMemcpyPeerAsync) or "none" (one device) */
int pt_num_devices(void);
const char *pt_exchange_transport(void);
const char *pt_last_error(void);
const char *pt_version(void);

#ifdef __cplusplus
}
#endif
#endif /* PTMI355_H */
