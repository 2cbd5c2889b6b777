"""ctypes binding of libptmi355.so.  Mirrors the reference's renderer interface:

    pathtraceInit(scene)            src/pathtrace.h:6   (pathtrace.cu:79-98)
    pathtraceFree()                 src/pathtrace.h:7   (pathtrace.cu:100-112)
    pathtrace(pbo, frame, iter)     src/pathtrace.h:8   (pathtrace.cu:284-393)

`Scene` carries what the reference's Scene/RenderState carry for this path
(scene.h:13-26, sceneStructs.h:54-60) as numpy arrays with the reference's
struct layouts.  There is no CPU fallback: if the HIP library is missing or no
GPU is present, calls raise PtError.
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

# byte-compatible with src/sceneStructs.h (x86-64): 236 / 44 / 84 / 44 / 20 bytes
GEOM_DT = np.dtype([("type", "<i4"), ("materialid", "<i4"), ("translation", "<f4", 3),
                    ("rotation", "<f4", 3), ("scale", "<f4", 3), ("transform", "<f4", (4, 4)),
                    ("inverseTransform", "<f4", (4, 4)), ("invTranspose", "<f4", (4, 4))])
MATERIAL_DT = np.dtype([("color", "<f4", 3), ("spec_exponent", "<f4"), ("spec_color", "<f4", 3),
                        ("hasReflective", "<f4"), ("hasRefractive", "<f4"),
                        ("indexOfRefraction", "<f4"), ("emittance", "<f4")])
CAMERA_DT = np.dtype([("resolution", "<i4", 2), ("position", "<f4", 3), ("lookAt", "<f4", 3),
                      ("view", "<f4", 3), ("up", "<f4", 3), ("right", "<f4", 3),
                      ("fov", "<f4", 2), ("pixelLength", "<f4", 2)])
PATH_DT = np.dtype([("origin", "<f4", 3), ("direction", "<f4", 3), ("color", "<f4", 3),
                    ("pixelIndex", "<i4"), ("remainingBounces", "<i4")])
ISECT_DT = np.dtype([("t", "<f4"), ("normal", "<f4", 3), ("materialId", "<i4")])
TRI_DT = np.dtype([("v0", "<f4", 3), ("v1", "<f4", 3), ("v2", "<f4", 3)])
MESH_DT = np.dtype([("geom_index", "<i4"), ("first_triangle", "<i4"), ("triangle_count", "<i4")])
# pt_light_element (include/ptmi355.h), 68 bytes
LIGHT_DT = np.dtype([("geom", "<i4"), ("kind", "<i4"), ("c0", "<f4", 3), ("ea", "<f4", 3), ("eb", "<f4", 3), ("normal", "<f4", 3),
                     ("area", "<f4"), ("cdf", "<f4"), ("inv_p", "<f4")])

PT_COMPACT, PT_SORT_MATERIAL, PT_FAKE_SHADER, PT_CACHE_FIRST, PT_UNFUSED, PT_MESH_BVH, PT_AA_JITTER, PT_ASYNC_IMAGE, PT_PIN_IMAGE = 1, 2, 4, 8, 16, 32, 64, 128, 256
PT_HOST_SPARSE = 1024
PT_SHARED_IMAGE = 512
PT_LOOKAHEAD = 2048         # pt_trace traces ahead of its caller (include/ptmi355.h)
PT_GLOSSY = 4096            # SPECEX gives mirrors and dielectrics a GGX lobe (include/ptmi355.h)
PT_DIRECT_LIGHT = 8192      # the last bounce aims a final ray at a sampled light (include/ptmi355.h)
PT_DIRECT_SKY = 32768       # ... and the environment map is one more light element (with PT_DIRECT_LIGHT; include/ptmi355.h)
PT_TEXTURES = 16384         # a cube texture per material tints spheres and cubes (include/ptmi355.h)
PT_SMOOTH_NORMALS = 65536   # per-vertex normals smooth the shading of triangle meshes (include/ptmi355.h)
PT_MOMENTS = 131072         # the session keeps per-pixel luminance moments for denoise_variance (include/ptmi355.h)
BVH_NODE_WORDS = 16


class PtError(RuntimeError):
    pass


class _Camera(C.Structure):
    _fields_ = [("raw", C.c_uint8 * 84)]


class _SceneDesc(C.Structure):
    _fields_ = [("geoms", C.c_void_p), ("num_geoms", C.c_int32),
                ("materials", C.c_void_p), ("num_materials", C.c_int32),
                ("triangles", C.c_void_p), ("num_triangles", C.c_int32),
                ("meshes", C.c_void_p), ("num_meshes", C.c_int32),
                ("camera", _Camera), ("trace_depth", C.c_int32), ("flags", C.c_uint32),
                ("device", C.c_int32), ("stream", C.c_void_p),
                ("tile_index", C.c_int32), ("tile_count", C.c_int32), ("strip_rows", C.c_int32),
                ("max_batch", C.c_int32), ("device_image", C.c_void_p),
                ("lens_radius", C.c_float), ("focal_distance", C.c_float),
                ("devices", C.c_void_p), ("num_devices", C.c_int32)]


class Stats(C.Structure):
    _fields_ = [("bounces", C.c_int32), ("rays", C.c_int64), ("live", C.c_int32 * 64),
                ("total_rays", C.c_int64), ("total_iterations", C.c_int64)]


class BvhInfo(C.Structure):
    _fields_ = [("nodes", C.c_int32), ("triangles", C.c_int32), ("depth", C.c_int32),
                ("pad", C.c_float), ("prune", C.c_float)]


class Profile(C.Structure):
    _fields_ = [("ms", C.c_double * 6), ("launches", C.c_int64 * 6)]


class DenoiseParams(C.Structure):
    _fields_ = [("levels", C.c_int32), ("sigma_color", C.c_float), ("sigma_normal", C.c_float),
                ("sigma_position", C.c_float)]


class VarianceParams(C.Structure):
    _fields_ = [("levels", C.c_int32), ("sigma_luminance", C.c_float), ("sigma_normal", C.c_float),
                ("sigma_position", C.c_float)]


class TemporalParams(C.Structure):
    _fields_ = [("max_history", C.c_int32), ("position_tolerance", C.c_float), ("normal_tolerance", C.c_float)]


STAGES = ("raygen", "bounce", "intersect", "sort", "gather", "mesh")


class Scene:
    """What pathtraceInit reads from the reference's Scene* (scene.h:23-25)."""

    def __init__(self, geoms, materials, camera, trace_depth, iterations=1, triangles=None,
                 meshes=None, name="scene"):
        self.geoms = np.ascontiguousarray(geoms, dtype=GEOM_DT)
        self.materials = np.ascontiguousarray(materials, dtype=MATERIAL_DT)
        self.camera = np.ascontiguousarray(camera, dtype=CAMERA_DT).reshape(1)
        self.traceDepth = int(trace_depth)
        self.iterations = int(iterations)
        self.triangles = None if triangles is None else np.ascontiguousarray(triangles, dtype=TRI_DT)
        self.meshes = None if meshes is None else np.ascontiguousarray(meshes, dtype=MESH_DT)
        self.name = name
        w, h = self.camera[0]["resolution"]
        self.image = np.zeros((int(w) * int(h), 3), dtype=np.float32)     # state.image (running sum)

    @property
    def resolution(self):
        w, h = self.camera[0]["resolution"]
        return int(w), int(h)


_lib = None
_scene = None
_host_sparse = False


def library():
    """Load libptmi355.so; raise loudly if the HIP extension has not been built."""
    global _lib
    if _lib is None:
        # PTMI355_LIB: another build of the same library (A/B measurements of kernel variants within one GPU box)
        path = os.environ.get("PTMI355_LIB") or os.path.join(HERE, "libptmi355.so")
        if not os.path.exists(path):
            raise PtError("libptmi355.so is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(there is no CPU fallback)")
        # torch is the plumbing for streams / device buffers / RCCL.  Import it first so the HIP
        # runtime it bundles is the one (and only one) resident in the process: loading the
        # system libamdhip64 first and torch's copy second leaves torch without devices.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(path)
        L.pt_last_error.restype = C.c_char_p
        L.pt_version.restype = C.c_char_p
        L.pt_device_image.restype = C.c_void_p
        L.pt_init.argtypes = [C.POINTER(_SceneDesc)]
        L.pt_set_camera.argtypes = [C.c_void_p, C.c_int]
        L.pt_set_lens.argtypes = [C.c_float, C.c_float]
        L.pt_trace.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        L.pt_trace_batch.argtypes = [C.c_int, C.c_int, C.c_void_p]
        L.pt_trace_batch_async.argtypes = [C.c_int, C.c_int]
        L.pt_trace_begin.argtypes = [C.c_int, C.c_int]
        L.pt_trace_bounce.argtypes = [C.c_int, C.POINTER(C.c_int)]
        L.pt_export_paths.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int)]
        L.pt_export_intersections.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        L.pt_intersect_once.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.pt_get_image.argtypes = [C.c_void_p]
        L.pt_tonemap.argtypes = [C.c_void_p, C.c_int]
        L.pt_get_stats.argtypes = [C.POINTER(Stats)]
        L.pt_total_rays.restype = C.c_int64
        L.pt_get_counters.argtypes = [C.POINTER(C.c_int64)] * 3
        L.pt_set_profiling.argtypes = [C.c_int]
        L.pt_get_profile.argtypes = [C.POINTER(Profile)]
        L.pt_get_bvh_info.argtypes = [C.POINTER(BvhInfo)]
        L.pt_bvh_build.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.pt_cull_boxes.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_float), C.c_void_p]
        L.pt_tri_bounds.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_void_p]
        L.pt_tri_records.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_void_p]
        try:
            L.pt_set_image.argtypes = [C.c_void_p]
            L.pt_probe_rng.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
            L.pt_probe_sincos.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
            L.pt_probe_hemisphere.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
            L.pt_probe_sqrt.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p]
            L.pt_probe_shade_scatter.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
            L.pt_probe_clock.argtypes = [C.c_int, C.POINTER(C.c_double)]
            L.pt_probe_tri_form.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
            L.pt_probe_own_surface_plan.argtypes = [C.c_uint64, C.c_int, C.c_int]
            L.pt_gbuffer.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
            L.pt_denoise.argtypes = [C.POINTER(DenoiseParams), C.c_int, C.c_void_p, C.c_void_p]
            L.pt_denoised_device_image.restype = C.c_void_p
            L.pt_denoise_temporal.argtypes = [C.POINTER(DenoiseParams), C.POINTER(TemporalParams), C.c_int, C.c_void_p, C.c_void_p]
            L.pt_history.argtypes = [C.c_void_p, C.c_void_p]
            L.pt_set_denoise_albedo.argtypes = [C.c_int]
            L.pt_albedo.argtypes = [C.c_void_p]
            L.pt_set_environment.argtypes = [C.c_void_p, C.c_int]
            L.pt_get_environment.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int)]
            L.pt_environment_texel.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
            L.pt_probe_environment.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
            L.pt_glossy_alpha2.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
            L.pt_probe_glossy_lobe.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
            L.pt_probe_shade_scatter_glossy.argtypes = L.pt_probe_shade_scatter.argtypes
            L.pt_light_elements.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
            L.pt_probe_direct_sample.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                                 C.c_void_p, C.c_void_p, C.c_void_p]
            L.pt_probe_shade_scatter_direct.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
            L.pt_sky_table.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
            L.pt_probe_sky_sample.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
            L.pt_probe_shade_scatter_direct_sky.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
            L.pt_set_texture.argtypes = [C.c_int, C.c_void_p, C.c_int]
            L.pt_get_texture.argtypes = [C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
            L.pt_texture_texel.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
            L.pt_probe_texture.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
            L.pt_probe_shade_scatter_textured.argtypes = L.pt_probe_shade_scatter.argtypes + [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                                                                              C.c_void_p, C.c_void_p]
            L.pt_set_bump_map.argtypes = L.pt_set_texture.argtypes
            L.pt_get_bump_map.argtypes = L.pt_get_texture.argtypes
            L.pt_bump_normal.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                         C.c_void_p, C.c_void_p]
            L.pt_probe_bump_normal.argtypes = L.pt_bump_normal.argtypes
            L.pt_probe_shade_scatter_bumped.argtypes = L.pt_probe_shade_scatter_textured.argtypes + [C.c_void_p, C.c_void_p, C.c_void_p]
            L.pt_set_vertex_normals.argtypes = [C.c_void_p, C.c_int]
            L.pt_get_vertex_normals.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int)]
            L.pt_smooth_normal.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
            L.pt_probe_smooth_normal.argtypes = L.pt_smooth_normal.argtypes
            L.pt_get_moments.argtypes = [C.c_void_p, C.c_void_p]
            L.pt_set_moments.argtypes = [C.c_void_p, C.c_void_p]
            L.pt_denoise_variance.argtypes = [C.POINTER(VarianceParams), C.c_int, C.c_void_p, C.c_void_p]
            L.pt_variance.argtypes = [C.c_void_p]
            L.pt_denoise_svgf.argtypes = [C.POINTER(VarianceParams), C.POINTER(TemporalParams), C.c_int, C.c_int, C.c_void_p, C.c_void_p]
            L.pt_svgf_history.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
            L.pt_svgf_variance.argtypes = [C.c_void_p]
        except AttributeError:
            if not os.environ.get("PTMI355_LIB"):        # only an older A/B build (profiles/tools/ab.sh) may lack them
                raise
        L.pt_free.restype = None
        L.pt_exchange_transport.restype = C.c_char_p
        _lib = L
    return _lib


def _chk(rc):
    if rc < 0:
        raise PtError("ptmi355 error %d: %s" % (rc, library().pt_last_error().decode()))
    return rc


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def version():
    return library().pt_version().decode()


def has_experiments():
    """True for a -DPT_EXPERIMENTS build (profiles/tools/build_variant.sh, loaded through PTMI355_LIB): the library then
    reads the experiment / test-hook environment variables of rounds 1-4; the shipped build reads the nine documented in
    include/ptmi355.h and nothing else."""
    return "+experiments" in version()


def pathtraceInit(scene, flags=PT_COMPACT, device=0, stream=None, tile=(0, 1, 8), max_batch=1,
                  device_image=None, lens=(0.0, 0.0), devices=None, pin_image=True, host_sparse=False, vertex_normals=None):
    """pathtraceInit(Scene*) (pathtrace.cu:79-98) + the run-time toggles of include/ptmi355.h.
    devices=[d0, d1, ...]: the frame tiled over several GPUs inside the library (tile[2] = rows per strip).
    pin_image: PT_PIN_IMAGE -- pathtrace() below always hands over scene.image, which lives as long as the scene
    (like the reference's scene->state.image); callers that pass their own short-lived buffers to pt_trace say False.
    host_sparse: PT_HOST_SPARSE -- the caller only READS the image between calls, so a call writes just the pixels whose
    sum changed; pathtrace() then returns a read-only view of scene.image (a host that scribbles on it gets an error
    instead of stale pixels).
    vertex_normals: [num_triangles, 3, 3] float32 -- sets PT_SMOOTH_NORMALS and uploads them (set_vertex_normals)."""
    global _scene, _host_sparse
    if vertex_normals is not None:
        flags |= PT_SMOOTH_NORMALS
    _host_sparse = bool(host_sparse or (flags & PT_HOST_SPARSE))
    d = _SceneDesc()
    d.geoms, d.num_geoms = _p(scene.geoms), len(scene.geoms)
    d.materials, d.num_materials = _p(scene.materials), len(scene.materials)
    d.triangles, d.num_triangles = _p(scene.triangles), 0 if scene.triangles is None else len(scene.triangles)
    d.meshes, d.num_meshes = _p(scene.meshes), 0 if scene.meshes is None else len(scene.meshes)
    C.memmove(C.byref(d.camera), scene.camera.tobytes(), 84)
    d.trace_depth, d.device = scene.traceDepth, device
    d.flags = flags | (PT_PIN_IMAGE if pin_image else 0) | (PT_HOST_SPARSE if host_sparse else 0)
    d.stream = stream
    d.tile_index, d.tile_count, d.strip_rows = tile
    d.max_batch = max_batch
    d.device_image = device_image
    d.lens_radius, d.focal_distance = lens
    devs = None
    if devices is not None:
        devs = np.ascontiguousarray(devices, dtype=np.int32)
        d.devices, d.num_devices = _p(devs), len(devs)
    _chk(library().pt_init(C.byref(d)))
    _scene = scene
    if vertex_normals is not None:
        set_vertex_normals(vertex_normals)


def pathtraceFree():
    """pathtraceFree() (pathtrace.cu:100-112): idempotent."""
    global _scene
    library().pt_free()
    _scene = None


def pathtrace(pbo, frame, iteration, copy_image=True):
    """pathtrace(uchar4 *pbo, int frame, int iter) (pathtrace.cu:284-393).  `pbo` is a device
    pointer (int) or None.  Like the reference (pathtrace.cu:285-286, 389-390) it re-reads the
    camera / traceDepth from the scene and refreshes scene.image (the running sum)."""
    if _scene is None:
        raise PtError("pathtrace: pathtraceInit has not been called")
    L = library()
    _chk(L.pt_set_camera(_p(_scene.camera), _scene.traceDepth))
    _chk(L.pt_trace(pbo, frame, iteration, _p(_scene.image) if copy_image else None))
    if _host_sparse:
        view = _scene.image.view()
        view.setflags(write=False)
        return view
    return _scene.image


def set_lens(lens_radius, focal_distance):
    _chk(library().pt_set_lens(lens_radius, focal_distance))


def set_camera(camera, trace_depth):
    cam = np.ascontiguousarray(camera, dtype=CAMERA_DT).reshape(1)
    _chk(library().pt_set_camera(_p(cam), trace_depth))


def _cube_texels(texels):
    """(texels as [6 * n * n, 3] float32, n) of a cube map given as [6, n, n, 3] or [6 * n * n, 3]."""
    t = np.ascontiguousarray(texels, dtype=np.float32)
    count = t.size // 3
    n = int(round((count / 6.0) ** 0.5))
    if t.size == 0 or t.size % 3 or 6 * n * n != count:
        raise PtError("environment: %s is not 6 * n * n RGB texels" % (t.shape,))
    return t.reshape(count, 3), n


def _set_cube(setter, texels, *material):
    """`setter` (pt_set_environment, or pt_set_texture / pt_set_bump_map with their material) takes the cube map `texels`, or none."""
    if texels is None:
        _chk(setter(*material, None, 0))
        return
    t, n = _cube_texels(texels)
    _chk(setter(*material, _p(t), n))


def _get_cube(getter, *material):
    """The cube map `getter` gives back, [6, n, n, 3] float32, or None."""
    n = C.c_int(0)
    rc = getter(*material, None, 0, C.byref(n))                 # the size: PT_OK with n = 0 when none is set
    if n.value == 0:
        _chk(rc)
        return None
    out = np.zeros((6, n.value, n.value, 3), dtype=np.float32)
    _chk(getter(*material, _p(out), 6 * n.value * n.value, C.byref(n)))
    return out


def set_environment(texels):
    """The cube map a ray that leaves the scene reads (include/ptmi355.h: pt_set_environment): [6, n, n, 3] float32, indexed
    [face, j, i]; None: no environment, a miss ends with colour 0 again.  The running sum is not touched."""
    _set_cube(library().pt_set_environment, texels)


def get_environment():
    """The session's cube map as it was set, [6, n, n, 3] float32, or None."""
    return _get_cube(library().pt_get_environment)


def gradient_cubemap(n, zenith, horizon, ground):
    """A sky for set_environment, [6, n, n, 3] float32: horizon + (zenith - horizon) * max(y, 0) + (ground - horizon) * max(-y, 0)
    at the texel centres, y = the unit direction's second component.  Host arithmetic in float64, rounded to float32 once: the
    texels are input to the lookup's specification, not part of it."""
    n = int(n)
    if n < 1 or n > 1024:
        raise PtError("gradient_cubemap: n = %d outside [1, 1024]" % n)
    z, h, g = (np.asarray(c, dtype=np.float64).reshape(3) for c in (zenith, horizon, ground))
    c = (np.arange(n, dtype=np.float64) + 0.5) / n * 2.0 - 1.0        # texel centres in [-1, 1]
    b, a = np.meshgrid(c, c, indexing="ij")                           # [j, i]: b from j, a from i
    out = np.zeros((6, n, n, 3), dtype=np.float32)
    for face in range(6):
        axis, major = face >> 1, (-1.0 if face & 1 else 1.0)
        comp = [None, None, None]
        comp[axis] = np.full_like(a, major)
        rest = [k for k in range(3) if k != axis]
        comp[rest[0]], comp[rest[1]] = a, b
        y = comp[1] / np.sqrt(comp[0] * comp[0] + comp[1] * comp[1] + comp[2] * comp[2])
        up, down = np.maximum(y, 0.0)[..., None], np.maximum(-y, 0.0)[..., None]
        out[face] = (h + (z - h) * up + (g - h) * down).astype(np.float32)
    return out


def sun_on_cubemap(texels, direction, cos_half_angle, rgb):
    """A copy of the cube map `texels` ([6, n, n, 3]) in which every texel whose centre direction c has dot(c, direction / |direction|)
    >= cos_half_angle is replaced by `rgb`: a sun for PT_DIRECT_SKY to find.  Host arithmetic in float64, the centres as in
    gradient_cubemap; the texels are input to the specification, not part of it."""
    t, n = _cube_texels(texels)
    out = np.array(t, dtype=np.float32, copy=True).reshape(6, n, n, 3)
    d = np.asarray(direction, dtype=np.float64).reshape(3)
    d = d / np.sqrt((d * d).sum())
    col = np.asarray(rgb, dtype=np.float64).reshape(3).astype(np.float32)
    c = (np.arange(n, dtype=np.float64) + 0.5) / n * 2.0 - 1.0
    b, a = np.meshgrid(c, c, indexing="ij")
    for face in range(6):
        axis, major = face >> 1, (-1.0 if face & 1 else 1.0)
        comp = [None, None, None]
        comp[axis] = np.full_like(a, major)
        rest = [k for k in range(3) if k != axis]
        comp[rest[0]], comp[rest[1]] = a, b
        ln = np.sqrt(comp[0] * comp[0] + comp[1] * comp[1] + comp[2] * comp[2])
        cosine = (comp[0] * d[0] + comp[1] * d[1] + comp[2] * d[2]) / ln
        out[face][cosine >= float(cos_half_angle)] = col
    return out


def sky_table(texels):
    """Host-only: the sampling tables a PT_DIRECT_SKY session builds from a cube map (include/ptmi355.h: pt_sky_table): (row [6 n, 2],
    col [6 n, n, 2]) float32 pairs {cdf, inv}, or None when the map yields no sky element."""
    t, n = (None, 0) if texels is None else _cube_texels(texels)
    row = np.zeros((6 * n, 2), dtype=np.float32)
    col = np.zeros((6 * n, n, 2), dtype=np.float32)
    if _chk(library().pt_sky_table(_p(t), n, _p(row), _p(col))) == 0:
        return None
    return row, col


def probe_sky_sample(texels, normals, seeds):
    """PT_DIRECT_SKY's branch of the sampler on the device for (normal, engine seed) pairs on the table of the cube map `texels`
    alone (include/ptmi355.h: pt_probe_sky_sample): (dir [n, 3] float32, weight [n] float32, texel [n] int32); weight 0 and dir
    0 where the path would end, texel -1 where the map yields no element."""
    t, n = (None, 0) if texels is None else _cube_texels(texels)
    nr = np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
    sd = np.ascontiguousarray(seeds, dtype=np.uint32).reshape(-1)
    if len(nr) != len(sd):
        raise PtError("probe_sky_sample: %d normals, %d seeds" % (len(nr), len(sd)))
    d = np.zeros((len(sd), 3), dtype=np.float32)
    w = np.zeros(len(sd), dtype=np.float32)
    k = np.zeros(len(sd), dtype=np.int32)
    _chk(library().pt_probe_sky_sample(_p(t), n, _p(nr), _p(sd), len(sd), _p(d), _p(w), _p(k)))
    return d, w, k


def probe_shade_scatter_direct_sky(iter, depth, trace_depth, geoms, materials, paths, isects, texels, outside=None, hit_geom=None):
    """probe_shade_scatter_direct on the light table of a PT_DIRECT_SKY session under the cube map `texels` (None: no map)
    (include/ptmi355.h: pt_probe_shade_scatter_direct_sky)."""
    g = np.ascontiguousarray(geoms, dtype=GEOM_DT).reshape(-1)
    m = np.ascontiguousarray(materials, dtype=MATERIAL_DT).reshape(-1)
    p = np.array(paths, dtype=PATH_DT, copy=True, order="C").reshape(-1)
    x = np.ascontiguousarray(isects, dtype=ISECT_DT).reshape(-1)
    o = None if outside is None else np.ascontiguousarray(outside, dtype=np.uint8).reshape(-1)
    h = None if hit_geom is None else np.ascontiguousarray(hit_geom, dtype=np.int32).reshape(-1)
    t, n = (None, 0) if texels is None else _cube_texels(texels)
    if len(x) != len(p) or (o is not None and len(o) != len(p)) or (h is not None and len(h) != len(p)):
        raise PtError("probe_shade_scatter_direct_sky: %d paths, %d intersections" % (len(p), len(x)))
    _chk(library().pt_probe_shade_scatter_direct_sky(int(iter), int(depth), int(trace_depth), _p(g), len(g), _p(m), len(m), _p(p), _p(x),
                                                     _p(o), _p(h), len(p), _p(t), n))
    return p


def environment_texel(dirs, n):
    """Host-only: the texel index [count] int32 the specification assigns to each direction of a map of n x n texels per face
    (include/ptmi355.h: pt_environment_texel), -1 where it assigns none."""
    d = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
    out = np.zeros(len(d), dtype=np.int32)
    _chk(library().pt_environment_texel(_p(d), len(d), int(n), _p(out)))
    return out


def probe_environment(texels, dirs, throughput):
    """The miss exit's lookup and multiply on the device (include/ptmi355.h: pt_probe_environment): throughput * E(dirs) per
    component, [count, 3] float32.  texels: a cube map as for set_environment, or None (no map: +0)."""
    t, n = (None, 0) if texels is None else _cube_texels(texels)
    d = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
    c = np.ascontiguousarray(throughput, dtype=np.float32).reshape(-1, 3)
    if len(d) != len(c):
        raise PtError("probe_environment: %d directions, %d throughputs" % (len(d), len(c)))
    out = np.zeros((len(d), 3), dtype=np.float32)
    _chk(library().pt_probe_environment(_p(t), n, _p(d), _p(c), len(d), _p(out)))
    return out


def set_texture(material, texels):
    """The cube texture of one material (include/ptmi355.h: pt_set_texture): [6, n, n, 3] float32, indexed [face, j, i]; None
    removes it.  Sessions initialised with PT_TEXTURES.  The running sum is not touched."""
    _set_cube(library().pt_set_texture, texels, int(material))


def get_texture(material):
    """That material's cube texture as it was set, [6, n, n, 3] float32, or None."""
    return _get_cube(library().pt_get_texture, int(material))


def checker_cubemap(n, cells, colour0, colour1):
    """A checkerboard for set_texture, [6, n, n, 3] float32: texel [face, j, i] takes colour0 or colour1 by the parity of
    i * cells // n + j * cells // n + face -- the integer rule of the scene format's `CHECKER` line (host/pthost.h)."""
    n, cells = int(n), int(cells)
    if n < 1 or n > 1024 or cells < 1 or cells > 1024:
        raise PtError("checker_cubemap: n = %d, cells = %d outside [1, 1024]" % (n, cells))
    col = np.stack([np.asarray(colour0, dtype=np.float32).reshape(3), np.asarray(colour1, dtype=np.float32).reshape(3)])
    k = np.arange(n, dtype=np.int64) * cells // n
    odd = (k[None, None, :] + k[None, :, None] + np.arange(6, dtype=np.int64)[:, None, None]) & 1      # [face, j, i]
    return np.ascontiguousarray(col[odd])


def texture_texel(geoms, hit_geom, points, n):
    """Host-only: the texel index [count] int32 the specification assigns to each (primitive, world point) pair in a texture of
    n x n texels per face (include/ptmi355.h: pt_texture_texel); -1 where it assigns none, and for mesh primitives."""
    g = np.ascontiguousarray(geoms, dtype=GEOM_DT).reshape(-1)
    h = np.ascontiguousarray(hit_geom, dtype=np.int32).reshape(-1)
    pts = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    if len(h) != len(pts):
        raise PtError("texture_texel: %d primitives, %d points" % (len(h), len(pts)))
    out = np.zeros(len(h), dtype=np.int32)
    _chk(library().pt_texture_texel(_p(g), len(g), _p(h), _p(pts), len(h), int(n), _p(out)))
    return out


def probe_texture(geoms, hit_geom, points, texels, colour_in):
    """The texture lookup and multiply on the device through the function the kernels call (include/ptmi355.h: pt_probe_texture):
    colour_in * T[k] per component, or colour_in where there is no texel; [count, 3] float32."""
    g = np.ascontiguousarray(geoms, dtype=GEOM_DT).reshape(-1)
    h = np.ascontiguousarray(hit_geom, dtype=np.int32).reshape(-1)
    pts = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    c = np.ascontiguousarray(colour_in, dtype=np.float32).reshape(-1, 3)
    if len(h) != len(pts) or len(c) != len(pts):
        raise PtError("probe_texture: %d primitives, %d points, %d colours" % (len(h), len(pts), len(c)))
    t, n = _cube_texels(texels)
    out = np.zeros((len(h), 3), dtype=np.float32)
    _chk(library().pt_probe_texture(_p(g), len(g), _p(h), _p(pts), len(h), _p(t), n, _p(c), _p(out)))
    return out


def probe_shade_scatter_textured(iter, depth, materials, paths, isects, geoms, hit_geom, textures, outside=None, deferred=False):
    """probe_shade_scatter through the textured form of the shader, as the kernels of a PT_TEXTURES session call it
    (include/ptmi355.h: pt_probe_shade_scatter_textured).  hit_geom: the winning primitive per pair (-1 for t <= 0);
    textures: {material: [6, n, n, 3] float32}."""
    m = np.ascontiguousarray(materials, dtype=MATERIAL_DT).reshape(-1)
    g = np.ascontiguousarray(geoms, dtype=GEOM_DT).reshape(-1)
    p = np.array(paths, dtype=PATH_DT, copy=True, order="C").reshape(-1)
    x = np.ascontiguousarray(isects, dtype=ISECT_DT).reshape(-1)
    o = None if outside is None else np.ascontiguousarray(outside, dtype=np.uint8).reshape(-1)
    h = np.ascontiguousarray(hit_geom, dtype=np.int32).reshape(-1)
    if len(x) != len(p) or len(h) != len(p) or (o is not None and len(o) != len(p)):
        raise PtError("probe_shade_scatter_textured: %d paths, %d intersections, %d primitives" % (len(p), len(x), len(h)))
    tn = np.zeros(len(m), dtype=np.int32)
    toff = np.zeros(len(m), dtype=np.int32)
    parts, total = [], 0
    for mat in sorted(textures or {}):
        t, n = _cube_texels(textures[mat])
        tn[mat], toff[mat] = n, total
        parts.append(t)
        total += len(t)
    tex = np.ascontiguousarray(np.concatenate(parts)) if parts else None
    _chk(library().pt_probe_shade_scatter_textured(int(iter), int(depth), _p(m), len(m), _p(p), _p(x), _p(o), len(p), 1 if deferred else 0,
                                                   _p(g), len(g), _p(h), _p(tex), _p(tn), _p(toff)))
    return p


def set_bump_map(material, texels):
    """The cube bump map of one material (include/ptmi355.h: pt_set_bump_map): [6, n, n, 3] float32, indexed [face, j, i], a
    texel (da, db, unused); None removes it.  Sessions initialised with PT_TEXTURES.  The running sum is not touched."""
    _set_cube(library().pt_set_bump_map, texels, int(material))


def get_bump_map(material):
    """That material's bump map as it was set, [6, n, n, 3] float32, or None."""
    return _get_cube(library().pt_get_bump_map, int(material))


def _vertex_normals(who, normals):
    n = np.ascontiguousarray(normals, dtype=np.float32)
    if n.size % 9:
        raise PtError("%s: %s is not 9 floats per triangle" % (who, n.shape))
    return n.reshape(-1, 3, 3)


def set_vertex_normals(normals):
    """The per-vertex normals of the session's triangles (include/ptmi355.h: pt_set_vertex_normals): [num_triangles, 3, 3]
    float32, world space, in the order of the scene's triangles; None removes them.  The running sum is not touched."""
    if normals is None:
        _chk(library().pt_set_vertex_normals(None, 0))
        return
    n = _vertex_normals("set_vertex_normals", normals)
    _chk(library().pt_set_vertex_normals(_p(n), len(n)))


def get_vertex_normals():
    """The session's vertex normals as they were set, [num_triangles, 3, 3] float32, or None."""
    k = C.c_int(0)
    L = library()
    rc = L.pt_get_vertex_normals(None, 0, C.byref(k))             # the size: PT_OK with 0 when none are set
    if k.value == 0:
        _chk(rc)
        return None
    out = np.zeros((k.value, 3, 3), dtype=np.float32)
    _chk(L.pt_get_vertex_normals(_p(out), k.value, C.byref(k)))
    return out


def _smooth_records(who, triangles, normals, tri, origins, dirs):
    t = np.ascontiguousarray(triangles, dtype=TRI_DT).reshape(-1)
    n = _vertex_normals(who, normals)
    k = np.ascontiguousarray(tri, dtype=np.int32).reshape(-1)
    o = np.ascontiguousarray(origins, dtype=np.float32).reshape(-1, 3)
    d = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
    if len(n) != len(t) or len(o) != len(k) or len(d) != len(k):
        raise PtError("%s: %d triangles, %d normal triples, %d records, %d origins, %d directions" % (who, len(t), len(n), len(k), len(o), len(d)))
    return t, n, k, o, d


def smooth_normal(triangles, normals, tri, origins, dirs):
    """Host-only: the shading normal of each (triangle, ray) record under per-vertex normals (include/ptmi355.h:
    pt_smooth_normal).  Returns (normals [count, 3] float32, smoothed [count] bool)."""
    t, n, k, o, d = _smooth_records("smooth_normal", triangles, normals, tri, origins, dirs)
    out = np.zeros((len(k), 3), dtype=np.float32)
    flag = np.zeros(len(k), dtype=np.uint8)
    _chk(library().pt_smooth_normal(_p(t), _p(n), len(t), _p(k), _p(o), _p(d), len(k), _p(out), _p(flag)))
    return out, flag.astype(bool)


def probe_smooth_normal(triangles, normals, tri, origins, dirs):
    """smooth_normal on the device through the function the kernels call (include/ptmi355.h: pt_probe_smooth_normal)."""
    t, n, k, o, d = _smooth_records("probe_smooth_normal", triangles, normals, tri, origins, dirs)
    out = np.zeros((len(k), 3), dtype=np.float32)
    flag = np.zeros(len(k), dtype=np.uint8)
    _chk(library().pt_probe_smooth_normal(_p(t), _p(n), len(t), _p(k), _p(o), _p(d), len(k), _p(out), _p(flag)))
    return out, flag.astype(bool)


def studs_bumpmap(n, cells, slope):
    """Bevelled studs for set_bump_map, [6, n, n, 3] float32: the integer rule of the scene format's `STUDS` line
    (host/pthost.h) -- pa = (i * cells * 4 // n) % 4, sa = -1, 0, 0, 1 for pa = 0..3, sb likewise from j, texel
    (slope * sa, slope * sb, 0)."""
    n, cells = int(n), int(cells)
    if n < 1 or n > 1024 or cells < 1 or cells > 1024:
        raise PtError("studs_bumpmap: n = %d, cells = %d outside [1, 1024]" % (n, cells))
    ph = (np.arange(n, dtype=np.int64) * cells * 4 // n) % 4
    s = np.where(ph == 0, -1, np.where(ph == 3, 1, 0)).astype(np.float32) * np.float32(slope)
    out = np.zeros((6, n, n, 3), dtype=np.float32)
    out[..., 0] = s[None, None, :]
    out[..., 1] = s[None, :, None]
    return out


def _bump_records(who, geoms, hit_geom, points, normals, dirs):
    g = np.ascontiguousarray(geoms, dtype=GEOM_DT).reshape(-1)
    h = np.ascontiguousarray(hit_geom, dtype=np.int32).reshape(-1)
    pts = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    nrm = np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
    d = np.ascontiguousarray(dirs, dtype=np.float32).reshape(-1, 3)
    if len(h) != len(pts) or len(nrm) != len(pts) or len(d) != len(pts):
        raise PtError("%s: %d primitives, %d points, %d normals, %d directions" % (who, len(h), len(pts), len(nrm), len(d)))
    return g, h, pts, nrm, d


def bump_normal(geoms, hit_geom, points, normals, dirs, texels):
    """Host-only: the shading normal of each (primitive, world point, reported normal, ray direction) record under one bump map
    (include/ptmi355.h: pt_bump_normal).  Returns (normals [count, 3] float32, perturbed [count] bool)."""
    g, h, pts, nrm, d = _bump_records("bump_normal", geoms, hit_geom, points, normals, dirs)
    t, n = _cube_texels(texels)
    out = np.zeros((len(h), 3), dtype=np.float32)
    flag = np.zeros(len(h), dtype=np.uint8)
    _chk(library().pt_bump_normal(_p(g), len(g), _p(h), _p(pts), _p(nrm), _p(d), len(h), _p(t), n, _p(out), _p(flag)))
    return out, flag.astype(bool)


def probe_bump_normal(geoms, hit_geom, points, normals, dirs, texels):
    """bump_normal on the device through the function the kernels call (include/ptmi355.h: pt_probe_bump_normal)."""
    g, h, pts, nrm, d = _bump_records("probe_bump_normal", geoms, hit_geom, points, normals, dirs)
    t, n = _cube_texels(texels)
    out = np.zeros((len(h), 3), dtype=np.float32)
    flag = np.zeros(len(h), dtype=np.uint8)
    _chk(library().pt_probe_bump_normal(_p(g), len(g), _p(h), _p(pts), _p(nrm), _p(d), len(h), _p(t), n, _p(out), _p(flag)))
    return out, flag.astype(bool)


def _cube_table(maps, count):
    """{material: [6, n, n, 3]} as the probes' parallel arrays: texels back to back, n and offset per material."""
    tn = np.zeros(count, dtype=np.int32)
    toff = np.zeros(count, dtype=np.int32)
    parts, total = [], 0
    for mat in sorted(maps or {}):
        t, n = _cube_texels(maps[mat])
        tn[mat], toff[mat] = n, total
        parts.append(t)
        total += len(t)
    return (np.ascontiguousarray(np.concatenate(parts)) if parts else None), tn, toff


def probe_shade_scatter_bumped(iter, depth, materials, paths, isects, geoms, hit_geom, textures, bump_maps, outside=None, deferred=False):
    """probe_shade_scatter_textured with bump maps ({material: [6, n, n, 3] float32}) through the whole textured form as the
    kernels call it while a bump map is set (include/ptmi355.h: pt_probe_shade_scatter_bumped)."""
    m = np.ascontiguousarray(materials, dtype=MATERIAL_DT).reshape(-1)
    g = np.ascontiguousarray(geoms, dtype=GEOM_DT).reshape(-1)
    p = np.array(paths, dtype=PATH_DT, copy=True, order="C").reshape(-1)
    x = np.ascontiguousarray(isects, dtype=ISECT_DT).reshape(-1)
    o = None if outside is None else np.ascontiguousarray(outside, dtype=np.uint8).reshape(-1)
    h = np.ascontiguousarray(hit_geom, dtype=np.int32).reshape(-1)
    if len(x) != len(p) or len(h) != len(p) or (o is not None and len(o) != len(p)):
        raise PtError("probe_shade_scatter_bumped: %d paths, %d intersections, %d primitives" % (len(p), len(x), len(h)))
    tex, tn, toff = _cube_table(textures, len(m))
    bump, bn, boff = _cube_table(bump_maps, len(m))
    _chk(library().pt_probe_shade_scatter_bumped(int(iter), int(depth), _p(m), len(m), _p(p), _p(x), _p(o), len(p), 1 if deferred else 0,
                                                 _p(g), len(g), _p(h), _p(tex), _p(tn), _p(toff), _p(bump), _p(bn), _p(boff)))
    return p


def trace_batch(iter0, count, host_image=None):
    _chk(library().pt_trace_batch(iter0, count, _p(host_image)))


def trace_batch_async(iter0, count):
    _chk(library().pt_trace_batch_async(iter0, count))


def synchronize():
    _chk(library().pt_synchronize())


def trace_begin(iter0, count=1):
    _chk(library().pt_trace_begin(iter0, count))


def trace_bounce(depth):
    n = C.c_int(0)
    _chk(library().pt_trace_bounce(depth, C.byref(n)))
    return n.value


def trace_end():
    _chk(library().pt_trace_end())


def export_paths(capacity):
    buf = np.zeros(capacity, dtype=PATH_DT)
    live = C.c_int(0)
    n = _chk(library().pt_export_paths(_p(buf), capacity, C.byref(live)))
    return buf[:n], live.value


def export_intersections(capacity):
    buf = np.zeros(capacity, dtype=ISECT_DT)
    out = np.zeros(capacity, dtype=np.uint8)
    n = _chk(library().pt_export_intersections(_p(buf), _p(out), capacity))
    return buf[:n], out[:n]


def intersect_once(paths):
    paths = np.ascontiguousarray(paths, dtype=PATH_DT)
    isects = np.zeros(len(paths), dtype=ISECT_DT)
    outside = np.zeros(len(paths), dtype=np.uint8)
    _chk(library().pt_intersect_once(_p(paths), len(paths), _p(isects), _p(outside)))
    return isects, outside


def get_image(npix):
    img = np.zeros((npix, 3), dtype=np.float32)
    _chk(library().pt_get_image(_p(img)))
    return img


def tonemap(npix, iteration):
    out = np.zeros((npix, 4), dtype=np.uint8)
    _chk(library().pt_tonemap(_p(out), iteration))
    return out


def clear_image():
    _chk(library().pt_clear_image())


def set_image(image_sum):
    """Resume an accumulation: the running sum becomes `image_sum` (W*H*3 floats)."""
    img = np.ascontiguousarray(image_sum, dtype=np.float32)
    _chk(library().pt_set_image(_p(img)))


def gbuffer():
    """First hits of the current camera's pinhole rays (include/ptmi355.h: pt_gbuffer): {"normal": [npix, 3] float32,
    "position": [npix, 3] float32, "t": [npix] float32 (-1: miss), "materialId": [npix] int32 (-1: miss)}."""
    if _scene is None:
        _chk(library().pt_gbuffer(None, None, None, None))          # raises "not initialised"
    w, h = _scene.resolution
    n = w * h
    out = {"normal": np.zeros((n, 3), dtype=np.float32), "position": np.zeros((n, 3), dtype=np.float32),
           "t": np.zeros(n, dtype=np.float32), "materialId": np.zeros(n, dtype=np.int32)}
    _chk(library().pt_gbuffer(_p(out["normal"]), _p(out["position"]), _p(out["t"]), _p(out["materialId"])))
    return out


def denoise(iteration, levels=5, sigma_color=1.0, sigma_normal=0.35, sigma_position=0.5, rgba=False):
    """Edge-avoiding A-trous filter of the running sum after `iteration` iterations (include/ptmi355.h: pt_denoise):
    the denoised MEAN as [npix, 3] float32; with rgba=True also its RGBA8 form, (mean, [npix, 4] uint8)."""
    if _scene is None:
        _chk(library().pt_denoise(None, int(iteration), None, None))   # raises "not initialised"
    w, h = _scene.resolution
    prm = DenoiseParams(int(levels), float(sigma_color), float(sigma_normal), float(sigma_position))
    img = np.zeros((w * h, 3), dtype=np.float32)
    px = np.zeros((w * h, 4), dtype=np.uint8) if rgba else None
    _chk(library().pt_denoise(C.byref(prm), int(iteration), _p(img), _p(px)))
    return (img, px) if rgba else img


def denoise_temporal(iteration, params=None, temporal=None, rgba=False):
    """denoise() with the history of earlier cameras blended in (include/ptmi355.h: pt_denoise_temporal).  `params`: a
    DenoiseParams (default 5, 1.0, 0.35, 0.5), `temporal`: a TemporalParams (default 64, 0.1, 0.1).  The denoised MEAN as
    [npix, 3] float32; with rgba=True also its RGBA8 form."""
    if _scene is None:
        _chk(library().pt_denoise_temporal(None, None, int(iteration), None, None))   # raises "not initialised"
    w, h = _scene.resolution
    prm = params if params is not None else DenoiseParams(5, 1.0, 0.35, 0.5)
    tmp = temporal if temporal is not None else TemporalParams(64, 0.1, 0.1)
    img = np.zeros((w * h, 3), dtype=np.float32)
    px = np.zeros((w * h, 4), dtype=np.uint8) if rgba else None
    _chk(library().pt_denoise_temporal(C.byref(prm), C.byref(tmp), int(iteration), _p(img), _p(px)))
    return (img, px) if rgba else img


def history():
    """The history as the last denoise_temporal() used it, in the grid of that call's camera (include/ptmi355.h: pt_history):
    ([npix, 3] float32 colours, [npix] float32 sample counts; 0 = no history for the pixel)."""
    if _scene is None:
        _chk(library().pt_history(None, None))                              # raises "not initialised"
    w, h = _scene.resolution
    rgb = np.zeros((w * h, 3), dtype=np.float32)
    length = np.zeros(w * h, dtype=np.float32)
    _chk(library().pt_history(_p(rgb), _p(length)))
    return rgb, length


def history_reset():
    """Forget the history: the next denoise_temporal() equals denoise() bit for bit."""
    _chk(library().pt_history_reset())


def set_denoise_albedo(on):
    """The filters' first-hit albedo demodulation on / off (include/ptmi355.h: pt_set_denoise_albedo): denoise() and
    denoise_temporal() filter colour / albedo and return filtered * albedo.  Off after pathtraceInit."""
    _chk(library().pt_set_denoise_albedo(1 if on is True else 0 if on is False else int(on)))


def albedo():
    """The albedo plane of the current camera as the filters would use it (include/ptmi355.h: pt_albedo): [npix, 3] float32."""
    if _scene is None:
        _chk(library().pt_albedo(None))                                     # raises "not initialised"
    w, h = _scene.resolution
    out = np.zeros((w * h, 3), dtype=np.float32)
    _chk(library().pt_albedo(_p(out)))
    return out


def get_moments():
    """The luminance moments a PT_MOMENTS session keeps beside the running sum (include/ptmi355.h: pt_get_moments):
    (M1, M2), [npix] float32 each."""
    if _scene is None:
        _chk(library().pt_get_moments(None, None))                          # raises "not initialised"
    w, h = _scene.resolution
    m1, m2 = np.zeros(w * h, dtype=np.float32), np.zeros(w * h, dtype=np.float32)
    _chk(library().pt_get_moments(_p(m1), _p(m2)))
    return m1, m2


def set_moments(m1, m2):
    """Resume an accumulation's moments, the companion of set_image() (include/ptmi355.h: pt_set_moments)."""
    a, b = np.ascontiguousarray(m1, dtype=np.float32), np.ascontiguousarray(m2, dtype=np.float32)
    _chk(library().pt_set_moments(_p(a), _p(b)))


def denoise_variance(iteration, levels=5, sigma_luminance=4.0, sigma_normal=0.35, sigma_position=0.5, rgba=False):
    """The A-trous filter steered by the pixels' own measured noise (include/ptmi355.h: pt_denoise_variance; a PT_MOMENTS
    session): the denoised MEAN as [npix, 3] float32; with rgba=True also its RGBA8 form, (mean, [npix, 4] uint8)."""
    if _scene is None:
        _chk(library().pt_denoise_variance(None, int(iteration), None, None))   # raises "not initialised"
    w, h = _scene.resolution
    prm = VarianceParams(int(levels), float(sigma_luminance), float(sigma_normal), float(sigma_position))
    img = np.zeros((w * h, 3), dtype=np.float32)
    px = np.zeros((w * h, 4), dtype=np.uint8) if rgba else None
    _chk(library().pt_denoise_variance(C.byref(prm), int(iteration), _p(img), _p(px)))
    return (img, px) if rgba else img


def variance():
    """var_0, the variance of the mean's luminance, of the last denoise_variance() call's input (include/ptmi355.h:
    pt_variance): [npix] float32."""
    if _scene is None:
        _chk(library().pt_variance(None))                                   # raises "not initialised"
    w, h = _scene.resolution
    out = np.zeros(w * h, dtype=np.float32)
    _chk(library().pt_variance(_p(out)))
    return out


def denoise_svgf(iteration, params=None, temporal=None, spatial_below=4, rgba=False):
    """denoise_variance() with the colour AND the moments of earlier cameras blended in, and a 7 x 7 spatial variance estimate for
    pixels with fewer than `spatial_below` samples (include/ptmi355.h: pt_denoise_svgf; a PT_MOMENTS session).  `params`: a
    VarianceParams (default 5, 4.0, 0.35, 0.5), `temporal`: a TemporalParams (default 64, 0.1, 0.1).  The denoised MEAN as
    [npix, 3] float32; with rgba=True also its RGBA8 form."""
    if _scene is None:
        _chk(library().pt_denoise_svgf(None, None, int(spatial_below), int(iteration), None, None))   # raises "not initialised"
    w, h = _scene.resolution
    prm = params if params is not None else VarianceParams(5, 4.0, 0.35, 0.5)
    tmp = temporal if temporal is not None else TemporalParams(64, 0.1, 0.1)
    img = np.zeros((w * h, 3), dtype=np.float32)
    px = np.zeros((w * h, 4), dtype=np.uint8) if rgba else None
    _chk(library().pt_denoise_svgf(C.byref(prm), C.byref(tmp), int(spatial_below), int(iteration), _p(img), _p(px)))
    return (img, px) if rgba else img


def svgf_history():
    """The history as the last denoise_svgf() used it, in the grid of that call's camera (include/ptmi355.h: pt_svgf_history):
    ([npix, 3] colours, [npix] u1, [npix] u2, [npix] sample counts; float32, 0 = no history for the pixel)."""
    if _scene is None:
        _chk(library().pt_svgf_history(None, None, None, None))             # raises "not initialised"
    w, h = _scene.resolution
    rgb = np.zeros((w * h, 3), dtype=np.float32)
    u1, u2, length = (np.zeros(w * h, dtype=np.float32) for _ in range(3))
    _chk(library().pt_svgf_history(_p(rgb), _p(u1), _p(u2), _p(length)))
    return rgb, u1, u2, length


def svgf_variance():
    """var_0 as the levels of the last denoise_svgf() call received it (include/ptmi355.h: pt_svgf_variance): [npix] float32."""
    if _scene is None:
        _chk(library().pt_svgf_variance(None))                              # raises "not initialised"
    w, h = _scene.resolution
    out = np.zeros(w * h, dtype=np.float32)
    _chk(library().pt_svgf_variance(_p(out)))
    return out


def svgf_reset():
    """Forget denoise_svgf()'s history: the next call starts as the session's first."""
    _chk(library().pt_svgf_reset())


def denoised_device_ptr():
    """Device pointer of the last denoise() result (W*H*3 floats), None before the first."""
    return library().pt_denoised_device_image()


def device_image_ptr():
    return library().pt_device_image()


def num_devices():
    return library().pt_num_devices()


def exchange_transport():
    return library().pt_exchange_transport().decode()


def get_stats():
    s = Stats()
    _chk(library().pt_get_stats(C.byref(s)))
    return s


def set_profiling(enable):
    _chk(library().pt_set_profiling(1 if enable else 0))


def get_profile():
    """{stage: (summed ms, launches)} measured with HIP events on the launch stream."""
    p = Profile()
    _chk(library().pt_get_profile(C.byref(p)))
    return {name: (p.ms[i], p.launches[i]) for i, name in enumerate(STAGES)}


def bvh_info():
    info = BvhInfo()
    _chk(library().pt_get_bvh_info(C.byref(info)))
    return info


def bvh_build(triangles):
    """Host-only: the hierarchy pt_init builds under PT_MESH_BVH.  Returns (nodes[n, 16] uint32 -- layout in
    csrc/pt_bvh.hpp --, order[count] int32, grid[8] float32 = origin xyz, step xyz, padding, prune margin)."""
    tris = np.ascontiguousarray(triangles, dtype=TRI_DT)
    L = library()
    need = L.pt_bvh_build(_p(tris), len(tris), None, 0, None, None)
    if need < 0:
        raise PtError(L.pt_last_error().decode())
    nodes = np.zeros((need, BVH_NODE_WORDS), dtype=np.uint32)
    order = np.zeros(max(1, len(tris)), dtype=np.int32)
    grid = np.zeros(8, dtype=np.float32)
    _chk(min(0, L.pt_bvh_build(_p(tris), len(tris), _p(nodes), need, _p(order), _p(grid))))
    return nodes, order[:len(tris)], grid


def cull_boxes(geoms, eye=(0.0, 0.0, 0.0)):
    """Host-only: (boxes[n, 2, 3] float32 = lo / hi, origin bound, reject[n, 5] = mode / row of the inverseTransform)
    pt_init derives for the cull stage."""
    g = np.ascontiguousarray(geoms, dtype=GEOM_DT)
    e = np.asarray(eye, dtype=np.float32)
    out = np.zeros((len(g), 2, 3), dtype=np.float32)
    rej = np.zeros((len(g), 5), dtype=np.float32)
    r = C.c_float(0.0)
    _chk(library().pt_cull_boxes(_p(g), len(g), _p(e), _p(out), C.byref(r), _p(rej)))
    return out, r.value, rej


def tri_bounds(triangles, origin_bound):
    """Host-only: {centre xyz, Rs^2} per triangle of one mesh (the every-triangle loop's first stage)."""
    t = np.ascontiguousarray(triangles, dtype=TRI_DT)
    out = np.zeros(((len(t) + 3) & ~3, 4), dtype=np.float32)
    _chk(library().pt_tri_bounds(_p(t), len(t), float(origin_bound), _p(out)))
    return out[:len(t)]


def tri_records(triangles, origin_bound):
    """Host-only: the triangles' side of the bilinear form the every-triangle loop's first stage evaluates on the matrix pipe:
    (records [n64, 32] float16, frame {gx, gy, gz, 1 / Rm})."""
    t = np.ascontiguousarray(triangles, dtype=TRI_DT)
    n64 = (len(t) + 63) & ~63
    rec = np.zeros((max(n64, 1), 32), dtype=np.float16)
    frame = np.zeros(4, dtype=np.float32)
    n = _chk(library().pt_tri_records(_p(t), len(t), float(origin_bound), _p(rec), _p(frame)))
    return rec[:n], frame


def total_rays():
    """Rays traced since pathtraceInit (device-side counter; synchronises)."""
    r = library().pt_total_rays()
    if r < 0:
        _chk(int(r))
    return int(r)


def counters():
    """(rays, first-bounce rays, iterations) since pathtraceInit, from the device; synchronises."""
    a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
    _chk(library().pt_get_counters(C.byref(a), C.byref(b), C.byref(c)))
    return a.value, b.value, c.value


def probe_rng(seeds, draws):
    """The device's minstd_rand + u01 (csrc/pt_device.hpp): (engine state, last u01) after `draws` draws per seed."""
    sd = np.ascontiguousarray(seeds, dtype=np.uint32)
    st = np.zeros(len(sd), dtype=np.uint32)
    u = np.zeros(len(sd), dtype=np.float32)
    _chk(library().pt_probe_rng(_p(sd), len(sd), int(draws), _p(st), _p(u)))
    return st, u


def probe_sincos(x):
    """The device's shared sin / cos for the float32 arguments x."""
    xs = np.ascontiguousarray(x, dtype=np.float32)
    s = np.zeros(len(xs), dtype=np.float32)
    c = np.zeros(len(xs), dtype=np.float32)
    _chk(library().pt_probe_sincos(_p(xs), 0, len(xs), _p(s), _p(c), None))
    return s, c


def probe_sincos_sums(first_bits, count):
    """(sum of bits(sin) * (2k+1), the same for cos) mod 2^64 over the `count` consecutive float32 values from bit
    pattern `first_bits` on -- what oracle.pyoracle.sincos_sums computes on the CPU."""
    out = np.zeros(2, dtype=np.uint64)
    _chk(library().pt_probe_sincos(None, int(first_bits), int(count), None, None, _p(out)))
    return int(out[0]), int(out[1])


def probe_sqrt(first_bits, count):
    """(arguments whose sqrt differs, whose 1 / sqrt differs) between the kernels' Newton forms and the correctly rounded sqrtf /
    divide, over the `count` consecutive float32 values from bit pattern `first_bits` on."""
    out = np.zeros(2, dtype=np.uint64)
    _chk(library().pt_probe_sqrt(int(first_bits), int(count), _p(out)))
    return int(out[0]), int(out[1])


def probe_clock(microseconds=200):
    """The shader clock in GHz while whatever is enqueued keeps running (one wave, cycle counter against the 100-MHz counter)."""
    ghz = C.c_double(0.0)
    _chk(library().pt_probe_clock(int(microseconds), C.byref(ghz)))
    return float(ghz.value)


def probe_tri_form(triangles, origin_bound, origins, directions):
    """The every-triangle loop's first stage on the device (include/ptmi355.h: pt_probe_tri_form) for one mesh and rays:
    (ray slots [n, 32] float16 before the operand shuffle, class [n] (0 plain, 1 far, 2 wild), form [n, n64] float32: the
    MFMA's result for every (ray, record) pair, padding records included)."""
    t = np.ascontiguousarray(triangles, dtype=TRI_DT)
    o = np.ascontiguousarray(origins, dtype=np.float32).reshape(-1, 3)
    d = np.ascontiguousarray(directions, dtype=np.float32).reshape(-1, 3)
    if len(o) != len(d):
        raise PtError("probe_tri_form: %d origins, %d directions" % (len(o), len(d)))
    n, n64 = len(o), (len(t) + 63) & ~63
    slots = np.zeros((n, 32), dtype=np.float16)
    cls = np.zeros(n, dtype=np.int32)
    form = np.zeros((n, n64), dtype=np.float32)
    got = _chk(library().pt_probe_tri_form(_p(t), len(t), float(origin_bound), _p(o), _p(d), n, _p(slots), _p(cls), _p(form)))
    assert got == n64, (got, n64)
    return slots, cls, form


def probe_own_surface_plan(paths, ngeoms, plain_fused=True):
    """The launch plan's decision (host only): does a batch of `paths` paths of a scene of `ngeoms` primitives take the
    own-surface form of the fused bounce kernel's cull (the primitive left travels in the pid)?"""
    return bool(library().pt_probe_own_surface_plan(int(paths), int(ngeoms), 1 if plain_fused else 0))


def probe_hemisphere(normals, seeds):
    """calculateRandomDirectionInHemisphere on the device for (normal, engine seed) pairs."""
    nr = np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
    sd = np.ascontiguousarray(seeds, dtype=np.uint32)
    out = np.zeros((len(sd), 3), dtype=np.float32)
    _chk(library().pt_probe_hemisphere(_p(nr), _p(sd), len(sd), _p(out)))
    return out


def glossy_alpha2(exponents):
    """Host-only: the GGX lobe's alpha^2 a PT_GLOSSY session derives from each specular exponent (include/ptmi355.h:
    pt_glossy_alpha2), float32; 0 means no lobe."""
    e = np.ascontiguousarray(exponents, dtype=np.float32).reshape(-1)
    out = np.zeros(len(e), dtype=np.float32)
    _chk(library().pt_glossy_alpha2(_p(e), len(e), _p(out)))
    return out


def probe_glossy_lobe(normals, seeds, alpha2):
    """PT_GLOSSY's microfacet normal on the device for (normal, engine seed, alpha2) triples (include/ptmi355.h:
    pt_probe_glossy_lobe), [n, 3] float32.  alpha2: one value per element, or one for all."""
    nr = np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
    sd = np.ascontiguousarray(seeds, dtype=np.uint32).reshape(-1)
    a2 = np.ascontiguousarray(np.broadcast_to(np.asarray(alpha2, dtype=np.float32), sd.shape))
    if len(nr) != len(sd):
        raise PtError("probe_glossy_lobe: %d normals, %d seeds" % (len(nr), len(sd)))
    out = np.zeros((len(sd), 3), dtype=np.float32)
    _chk(library().pt_probe_glossy_lobe(_p(nr), _p(sd), _p(a2), len(sd), _p(out)))
    return out


def light_elements(geoms, materials):
    """Host-only: the light element table a PT_DIRECT_LIGHT session builds at pathtraceInit (include/ptmi355.h:
    pt_light_elements), a LIGHT_DT array; empty when no cube or sphere emits."""
    g = np.ascontiguousarray(geoms, dtype=GEOM_DT).reshape(-1)
    m = np.ascontiguousarray(materials, dtype=MATERIAL_DT).reshape(-1)
    L = library()
    need = _chk(L.pt_light_elements(_p(g), len(g), _p(m), len(m), None, 0))
    out = np.zeros(need, dtype=LIGHT_DT)
    if need:
        assert _chk(L.pt_light_elements(_p(g), len(g), _p(m), len(m), _p(out), need)) == need
    return out


def probe_direct_sample(geoms, materials, P, normals, seeds):
    """PT_DIRECT_LIGHT's sampler on the device for (P, normal, engine seed) triples on the light table of (geoms, materials)
    (include/ptmi355.h: pt_probe_direct_sample): (dir [n, 3] float32, weight [n] float32, element [n] int32); weight 0 and
    dir 0 where the path would end."""
    g = np.ascontiguousarray(geoms, dtype=GEOM_DT).reshape(-1)
    m = np.ascontiguousarray(materials, dtype=MATERIAL_DT).reshape(-1)
    p = np.ascontiguousarray(P, dtype=np.float32).reshape(-1, 3)
    nr = np.ascontiguousarray(normals, dtype=np.float32).reshape(-1, 3)
    sd = np.ascontiguousarray(seeds, dtype=np.uint32).reshape(-1)
    if len(p) != len(sd) or len(nr) != len(sd):
        raise PtError("probe_direct_sample: %d points, %d normals, %d seeds" % (len(p), len(nr), len(sd)))
    d = np.zeros((len(sd), 3), dtype=np.float32)
    w = np.zeros(len(sd), dtype=np.float32)
    e = np.zeros(len(sd), dtype=np.int32)
    _chk(library().pt_probe_direct_sample(_p(g), len(g), _p(m), len(m), _p(p), _p(nr), _p(sd), len(sd), _p(d), _p(w), _p(e)))
    return d, w, e


def probe_shade_scatter_direct(iter, depth, trace_depth, geoms, materials, paths, isects, outside=None, hit_geom=None):
    """probe_shade_scatter through the direct form of the shader, as a PT_DIRECT_LIGHT session of traceDepth `trace_depth` calls
    it at bounce `depth` in [0, trace_depth] (include/ptmi355.h: pt_probe_shade_scatter_direct).  hit_geom: the winning primitive
    per pair (-1: miss), read at depth == trace_depth."""
    g = np.ascontiguousarray(geoms, dtype=GEOM_DT).reshape(-1)
    m = np.ascontiguousarray(materials, dtype=MATERIAL_DT).reshape(-1)
    p = np.array(paths, dtype=PATH_DT, copy=True, order="C").reshape(-1)
    x = np.ascontiguousarray(isects, dtype=ISECT_DT).reshape(-1)
    o = None if outside is None else np.ascontiguousarray(outside, dtype=np.uint8).reshape(-1)
    h = None if hit_geom is None else np.ascontiguousarray(hit_geom, dtype=np.int32).reshape(-1)
    if len(x) != len(p) or (o is not None and len(o) != len(p)) or (h is not None and len(h) != len(p)):
        raise PtError("probe_shade_scatter_direct: %d paths, %d intersections" % (len(p), len(x)))
    _chk(library().pt_probe_shade_scatter_direct(int(iter), int(depth), int(trace_depth), _p(g), len(g), _p(m), len(m), _p(p), _p(x),
                                                 _p(o), _p(h), len(p)))
    return p


def probe_shade_scatter_glossy(iter, depth, materials, paths, isects, outside=None, deferred=False):
    """probe_shade_scatter through the glossy form of the shader, the one a PT_GLOSSY session's kernels call (include/ptmi355.h:
    pt_probe_shade_scatter_glossy); alpha2 comes from the materials' spec_exponent."""
    return probe_shade_scatter(iter, depth, materials, paths, isects, outside, deferred, _glossy=True)


def probe_shade_scatter(iter, depth, materials, paths, isects, outside=None, deferred=False, _glossy=False):
    """One pass of the loop body's shader on the device (include/ptmi355.h: pt_probe_shade_scatter) for (path, intersection)
    pairs: the paths afterwards (PATH_DT; the arguments are not written).  outside: one byte per pair, None = 1 for all;
    deferred: the deferring kernels' call, resolved as the next bounce's load resolves it (the same bytes)."""
    m = np.ascontiguousarray(materials, dtype=MATERIAL_DT)
    p = np.array(paths, dtype=PATH_DT, copy=True, order="C").reshape(-1)
    x = np.ascontiguousarray(isects, dtype=ISECT_DT).reshape(-1)
    o = None if outside is None else np.ascontiguousarray(outside, dtype=np.uint8).reshape(-1)
    if len(x) != len(p) or (o is not None and len(o) != len(p)):
        raise PtError("probe_shade_scatter: %d paths, %d intersections, %s outside flags" % (len(p), len(x), "no" if o is None else len(o)))
    fn = library().pt_probe_shade_scatter_glossy if _glossy else library().pt_probe_shade_scatter
    _chk(fn(int(iter), int(depth), _p(m), len(m), _p(p), _p(x), _p(o), len(p), 1 if deferred else 0))
    return p
