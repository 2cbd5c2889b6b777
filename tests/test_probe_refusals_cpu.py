"""What the session-free entry points refuse, and with which words: every probe of include/ptmi355.h and the host-only
builders beside them, called through the C-ABI with arguments that carry exactly one fault.  The return codes and the
pt_last_error() texts are literals: they were read from the library before the probes' shared plumbing was factored out,
and a reshaped probe has to give the same answers in the same order of checks.  Nothing is launched: every case is refused
(or returns PT_OK for an empty call) before the first allocation, so the module runs without a GPU."""
import ctypes as C

import numpy as np
import pytest

import __graft_entry__ as ge

OK, INVALID, DEVICE = 0, -1, -2
SPHERE, CUBE = 0, 1


@pytest.fixture(scope="module")
def pt():
    ge.load_package().build()
    return ge.load_package()


# ---- sound arguments: two records, two materials (the second emits), two primitives (a sphere, and a cube that emits) ----
def materials(pt):
    m = np.zeros(2, pt.MATERIAL_DT)
    m["color"] = 0.5
    m["emittance"][1] = 5.0
    return m


def geoms(pt, materialid=(0, 1)):
    g = np.zeros(2, pt.GEOM_DT)
    g["type"] = (SPHERE, CUBE)
    g["materialid"] = materialid
    g["scale"] = 1.0
    for f in ("transform", "inverseTransform", "invTranspose"):
        g[f] = np.eye(4, dtype=np.float32)
    return g


def paths(pt):
    p = np.zeros(2, pt.PATH_DT)
    p["direction"] = (0.0, 0.0, -1.0)
    p["color"] = 1.0
    p["pixelIndex"] = (0, 1)
    p["remainingBounces"] = 2
    return p


def isects(pt, material=(0, 0)):
    x = np.zeros(2, pt.ISECT_DT)
    x["t"] = 1.0
    x["normal"] = (0.0, 0.0, 1.0)
    x["materialId"] = material
    return x


def f32(*shape, value=0.0):
    return np.full(shape, value, np.float32)


def i32(*values):
    return np.array(values, np.int32)


def triangle(pt):
    t = np.zeros(1, pt.TRI_DT)
    t["v1"] = (1.0, 0.0, 0.0)
    t["v2"] = (0.0, 1.0, 0.0)
    return t


UNIT_Z = np.tile(np.array([0.0, 0.0, 1.0], np.float32), (2, 1))
MAP = f32(6, 3, value=0.5)                     # a cube map of n = 1: six texels

SCATTER = [("iter", 1), ("depth", 0), ("materials", materials), ("num_materials", 2), ("paths", paths), ("isects", isects),
           ("outside", np.ones(2, np.uint8)), ("n", 2), ("deferred", 0)]
TEXTURED = SCATTER + [("geoms", geoms), ("num_geoms", 2), ("hit_geom", i32(0, 1)), ("tex_texels", MAP), ("tex_n", i32(1, 0)),
                      ("tex_offset", i32(0, 0))]
BUMPED = TEXTURED + [("bump_texels", MAP), ("bump_n", i32(1, 0)), ("bump_offset", i32(0, 0))]
DIRECT = [("iter", 1), ("depth", 0), ("trace_depth", 2), ("geoms", geoms), ("num_geoms", 2), ("materials", materials), ("num_materials", 2),
          ("paths", paths), ("isects", isects), ("outside", np.ones(2, np.uint8)), ("hit_geom", i32(0, 1)), ("n", 2)]
TEXTURE_ARGS = [("geoms", geoms), ("num_geoms", 2), ("hit_geom", i32(0, 1)), ("points", UNIT_Z), ("count", 2)]
BUMP = TEXTURE_ARGS[:4] + [("normals", UNIT_Z), ("dirs", -UNIT_Z), ("count", 2), ("texels", MAP), ("n", 1), ("out_normals", f32(2, 3)),
                           ("perturbed", np.zeros(2, np.uint8))]

# entry point -> its parameters in order, each with a sound value (a callable is given the package and makes a fresh array)
SOUND = {
    "pt_probe_rng": [("seeds", i32(1, 2)), ("n", 2), ("draws", 1), ("state", i32(0, 0)), ("u", f32(2))],
    "pt_probe_sincos": [("x", f32(2)), ("first_bits", 0), ("n", 2), ("s", f32(2)), ("c", f32(2)), ("sum", np.zeros(2, np.uint64))],
    "pt_probe_sqrt": [("first_bits", 0x3f800000), ("n", 2), ("mismatch", np.zeros(2, np.uint64))],
    "pt_probe_clock": [("microseconds", 10), ("ghz", lambda pt: C.pointer(C.c_double()))],
    "pt_probe_hemisphere": [("normals", UNIT_Z), ("seeds", i32(1, 2)), ("n", 2), ("dirs", f32(2, 3))],
    "pt_probe_glossy_lobe": [("normals", UNIT_Z), ("seeds", i32(1, 2)), ("alpha2", f32(2, value=0.01)), ("n", 2), ("dirs", f32(2, 3))],
    "pt_glossy_alpha2": [("exponents", f32(2, value=50.0)), ("count", 2), ("alpha2", f32(2))],
    "pt_probe_shade_scatter": SCATTER,
    "pt_probe_shade_scatter_glossy": SCATTER,
    "pt_probe_shade_scatter_textured": TEXTURED,
    "pt_probe_shade_scatter_bumped": BUMPED,
    "pt_probe_shade_scatter_direct": DIRECT,
    "pt_probe_shade_scatter_direct_sky": DIRECT + [("texels", MAP), ("env_n", 1)],
    "pt_probe_direct_sample": [("geoms", geoms), ("num_geoms", 2), ("materials", materials), ("num_materials", 2), ("P", f32(2, 3)),
                               ("n", UNIT_Z), ("seeds", i32(1, 2)), ("count", 2), ("dir", f32(2, 3)), ("weight", f32(2)),
                               ("element", i32(0, 0))],
    "pt_probe_sky_sample": [("texels", MAP), ("n", 1), ("normals", UNIT_Z), ("seeds", i32(1, 2)), ("count", 2), ("dir", f32(2, 3)),
                            ("weight", f32(2)), ("texel", i32(0, 0))],
    "pt_light_elements": [("geoms", geoms), ("num_geoms", 2), ("materials", materials), ("num_materials", 2),
                          ("out", lambda pt: np.zeros(8, pt.LIGHT_DT)), ("capacity", 8)],
    "pt_sky_table": [("texels", MAP), ("n", 1), ("row", f32(6, 2)), ("col", f32(6, 2))],
    "pt_environment_texel": [("dirs", UNIT_Z), ("count", 2), ("n", 1), ("index", i32(0, 0))],
    "pt_probe_environment": [("texels", MAP), ("n", 1), ("dirs", UNIT_Z), ("throughput", f32(2, 3, value=1.0)), ("count", 2),
                             ("colour", f32(2, 3))],
    "pt_texture_texel": TEXTURE_ARGS + [("n", 1), ("index", i32(0, 0))],
    "pt_probe_texture": TEXTURE_ARGS + [("texels", MAP), ("n", 1), ("colour_in", f32(2, 3, value=1.0)), ("colour_out", f32(2, 3))],
    "pt_bump_normal": BUMP,
    "pt_probe_bump_normal": BUMP,
    "pt_probe_tri_form": [("triangles", triangle), ("count", 1), ("origin_bound", 4.0), ("origins", f32(2, 3)), ("directions", UNIT_Z),
                          ("n", 2), ("ray_slots", np.zeros((2, 32), np.uint16)), ("ray_class", i32(0, 0)), ("form", f32(2, 64))],
    "pt_bvh_build": [("triangles", triangle), ("count", 1), ("nodes", f32(64, 16)), ("node_capacity", 64), ("order", i32(0)),
                     ("grid", f32(8))],
    "pt_tri_bounds": [("triangles", triangle), ("count", 1), ("origin_bound", 4.0), ("bounds", f32(4, 4))],
    "pt_tri_records": [("triangles", triangle), ("count", 1), ("origin_bound", 4.0), ("records", np.zeros((64, 32), np.uint16)),
                       ("frame", f32(4))],
    "pt_cull_boxes": [("geoms", geoms), ("count", 2), ("eye", f32(3)), ("boxes", f32(2, 6)), ("origin_bound", None), ("reject", f32(2, 5))],
}

LAST_MATERIAL = lambda pt: isects(pt, material=(0, 2))         # record 1 hits material 2 of 2
LAST_GEOM = i32(0, 2)                                          # record 1 names primitive 2 of 2
NO_DEVICE = "%s: no HIP device / out of memory (this library has no CPU fallback)"

# (entry point, the one argument that differs from SOUND, return code, pt_last_error() -- None: not looked at, the call succeeds)
REFUSALS = [
    ("pt_probe_rng", {"n": -1}, INVALID, "pt_probe_rng: bad argument"),
    ("pt_probe_rng", {"draws": -1}, INVALID, "pt_probe_rng: bad argument"),
    ("pt_probe_rng", {"n": 0}, OK, None),
    ("pt_probe_sincos", {"n": (1 << 28) + 1}, INVALID, "pt_probe_sincos: 268435457 elements with arrays (at most 2^28)"),
    ("pt_probe_sincos", {"n": 0}, OK, None),
    ("pt_probe_sqrt", {"mismatch": None}, INVALID, "pt_probe_sqrt: null result"),
    ("pt_probe_sqrt", {"n": 0}, OK, None),
    ("pt_probe_clock", {"microseconds": 0}, INVALID, "pt_probe_clock: bad argument"),
    ("pt_probe_clock", {"ghz": None}, INVALID, "pt_probe_clock: bad argument"),
    ("pt_probe_hemisphere", {"n": -1}, INVALID, "pt_probe_hemisphere: bad argument"),
    ("pt_probe_hemisphere", {"dirs": None}, INVALID, "pt_probe_hemisphere: bad argument"),
    ("pt_probe_hemisphere", {"n": 0}, OK, None),
    ("pt_probe_glossy_lobe", {"n": -1}, INVALID, "pt_probe_glossy_lobe: bad argument"),
    ("pt_probe_glossy_lobe", {"alpha2": None}, INVALID, "pt_probe_glossy_lobe: bad argument"),
    ("pt_probe_glossy_lobe", {"n": 0}, OK, None),
    ("pt_glossy_alpha2", {"count": -1}, INVALID, "pt_glossy_alpha2: bad argument (count -1)"),
    ("pt_glossy_alpha2", {"alpha2": None}, INVALID, "pt_glossy_alpha2: bad argument (count 2)"),
    ("pt_glossy_alpha2", {"count": 0}, OK, None),
    # ---- the scatter family ----
    ("pt_probe_shade_scatter", {"n": -1}, INVALID, "pt_probe_shade_scatter: bad argument"),
    ("pt_probe_shade_scatter", {"n": (1 << 26) + 1}, INVALID, "pt_probe_shade_scatter: bad argument"),
    ("pt_probe_shade_scatter", {"deferred": 2}, INVALID, "pt_probe_shade_scatter: bad argument"),
    ("pt_probe_shade_scatter", {"num_materials": 0}, INVALID, "pt_probe_shade_scatter: bad argument"),
    ("pt_probe_shade_scatter", {"paths": None}, INVALID, "pt_probe_shade_scatter: bad argument"),
    ("pt_probe_shade_scatter", {"isects": LAST_MATERIAL}, INVALID, "pt_probe_shade_scatter: record 1 hits material 2 of 2"),
    ("pt_probe_shade_scatter", {"n": 0}, OK, None),
    ("pt_probe_shade_scatter_glossy", {"n": -1}, INVALID, "pt_probe_shade_scatter_glossy: bad argument"),
    ("pt_probe_shade_scatter_glossy", {"deferred": 2}, INVALID, "pt_probe_shade_scatter_glossy: bad argument"),
    ("pt_probe_shade_scatter_glossy", {"isects": LAST_MATERIAL}, INVALID, "pt_probe_shade_scatter_glossy: record 1 hits material 2 of 2"),
    ("pt_probe_shade_scatter_glossy", {"n": 0}, OK, None),
    ("pt_probe_shade_scatter_textured", {"n": -1}, INVALID, "pt_probe_shade_scatter_textured: bad argument"),
    ("pt_probe_shade_scatter_textured", {"deferred": 2}, INVALID, "pt_probe_shade_scatter_textured: bad argument"),
    ("pt_probe_shade_scatter_textured", {"hit_geom": None}, INVALID, "pt_probe_shade_scatter_textured: bad argument"),
    ("pt_probe_shade_scatter_textured", {"tex_offset": None}, INVALID, "pt_probe_shade_scatter_textured: bad argument"),
    ("pt_probe_shade_scatter_textured", {"isects": LAST_MATERIAL}, INVALID, "pt_probe_shade_scatter_textured: record 1 hits material 2 of 2"),
    ("pt_probe_shade_scatter_textured", {"hit_geom": LAST_GEOM}, INVALID, "pt_probe_shade_scatter_textured: record 1 names primitive 2 of 2"),
    ("pt_probe_shade_scatter_textured", {"tex_n": i32(1, 1025)}, INVALID,
     "pt_probe_shade_scatter_textured: material 1 has a texture of n = 1025 at offset 0"),
    ("pt_probe_shade_scatter_textured", {"tex_offset": i32(-1, 0)}, INVALID,
     "pt_probe_shade_scatter_textured: material 0 has a texture of n = 1 at offset -1"),
    ("pt_probe_shade_scatter_textured", {"tex_texels": None}, INVALID, "pt_probe_shade_scatter_textured: null tex_texels"),
    ("pt_probe_shade_scatter_textured", {"tex_offset": i32(0x7fffffff, 0)}, INVALID,
     "pt_probe_shade_scatter_textured: 2147483653 texels in all (at most 2^31 - 1)"),
    ("pt_probe_shade_scatter_textured", {"n": 0}, OK, None),
    ("pt_probe_shade_scatter_bumped", {"n": -1}, INVALID, "pt_probe_shade_scatter_bumped: bad argument"),
    ("pt_probe_shade_scatter_bumped", {"deferred": 2}, INVALID, "pt_probe_shade_scatter_bumped: bad argument"),
    ("pt_probe_shade_scatter_bumped", {"bump_n": None}, INVALID, "pt_probe_shade_scatter_bumped: bad argument"),
    ("pt_probe_shade_scatter_bumped", {"isects": LAST_MATERIAL}, INVALID, "pt_probe_shade_scatter_bumped: record 1 hits material 2 of 2"),
    ("pt_probe_shade_scatter_bumped", {"hit_geom": LAST_GEOM}, INVALID, "pt_probe_shade_scatter_bumped: record 1 names primitive 2 of 2"),
    ("pt_probe_shade_scatter_bumped", {"tex_n": i32(1, 1025)}, INVALID,
     "pt_probe_shade_scatter_bumped: material 1 has a texture of n = 1025 at offset 0"),
    ("pt_probe_shade_scatter_bumped", {"bump_n": i32(1025, 0)}, INVALID,
     "pt_probe_shade_scatter_bumped: material 0 has a bump map of n = 1025 at offset 0"),
    ("pt_probe_shade_scatter_bumped", {"bump_offset": i32(-1, 0)}, INVALID,
     "pt_probe_shade_scatter_bumped: material 0 has a bump map of n = 1 at offset -1"),
    ("pt_probe_shade_scatter_bumped", {"tex_texels": None}, INVALID, "pt_probe_shade_scatter_bumped: null texels"),
    ("pt_probe_shade_scatter_bumped", {"bump_texels": None}, INVALID, "pt_probe_shade_scatter_bumped: null texels"),
    ("pt_probe_shade_scatter_bumped", {"bump_offset": i32(0x7fffffff, 0)}, INVALID,
     "pt_probe_shade_scatter_bumped: 2147483653 texels in all (at most 2^31 - 1)"),
    ("pt_probe_shade_scatter_bumped", {"n": 0}, OK, None),
    ("pt_probe_shade_scatter_direct", {"n": -1}, INVALID, "pt_probe_shade_scatter_direct: bad argument"),
    ("pt_probe_shade_scatter_direct", {"depth": 3}, INVALID, "pt_probe_shade_scatter_direct: bad argument"),
    ("pt_probe_shade_scatter_direct", {"trace_depth": 64}, INVALID, "pt_probe_shade_scatter_direct: bad argument"),
    ("pt_probe_shade_scatter_direct", {"isects": LAST_MATERIAL}, INVALID, "pt_probe_shade_scatter_direct: record 1 hits material 2 of 2"),
    ("pt_probe_shade_scatter_direct", {"num_geoms": -1}, INVALID, "pt_probe_shade_scatter_direct: bad argument"),
    ("pt_probe_shade_scatter_direct", {"geoms": lambda pt: geoms(pt, (0, 2))}, INVALID,
     "pt_probe_shade_scatter_direct: a cube or sphere names a material outside [0, 2)"),
    ("pt_probe_shade_scatter_direct", {"n": 0}, OK, None),
    ("pt_probe_shade_scatter_direct_sky", {"n": -1}, INVALID, "pt_probe_shade_scatter_direct_sky: bad argument"),
    ("pt_probe_shade_scatter_direct_sky", {"depth": 3}, INVALID, "pt_probe_shade_scatter_direct_sky: bad argument"),
    ("pt_probe_shade_scatter_direct_sky", {"env_n": 1025}, INVALID, "pt_probe_shade_scatter_direct_sky: bad map (n = 1025)"),
    ("pt_probe_shade_scatter_direct_sky", {"texels": None}, INVALID, "pt_probe_shade_scatter_direct_sky: bad map (n = 1)"),
    ("pt_probe_shade_scatter_direct_sky", {"isects": LAST_MATERIAL}, INVALID,
     "pt_probe_shade_scatter_direct_sky: record 1 hits material 2 of 2"),
    ("pt_probe_shade_scatter_direct_sky", {"n": 0}, OK, None),
    # ---- the samplers and lookups ----
    ("pt_probe_direct_sample", {"count": -1}, INVALID, "pt_probe_direct_sample: bad argument"),
    ("pt_probe_direct_sample", {"count": (1 << 26) + 1}, INVALID, "pt_probe_direct_sample: bad argument"),
    ("pt_probe_direct_sample", {"num_materials": 0}, INVALID, "pt_probe_direct_sample: bad argument"),
    ("pt_probe_direct_sample", {"geoms": lambda pt: geoms(pt, (0, 2))}, INVALID,
     "pt_probe_direct_sample: a cube or sphere names a material outside [0, 2)"),
    ("pt_probe_direct_sample", {"count": 0}, OK, None),
    ("pt_probe_sky_sample", {"n": 1025}, INVALID, "pt_probe_sky_sample: bad argument (n = 1025, count = 2)"),
    ("pt_probe_sky_sample", {"count": -1}, INVALID, "pt_probe_sky_sample: bad argument (n = 1, count = -1)"),
    ("pt_probe_sky_sample", {"count": 0}, OK, None),
    ("pt_light_elements", {"capacity": -1}, INVALID, "pt_light_elements: bad argument (2 geoms, 2 materials, capacity -1)"),
    ("pt_light_elements", {"geoms": lambda pt: geoms(pt, (0, 2))}, INVALID,
     "pt_light_elements: a cube or sphere names a material outside [0, 2)"),
    ("pt_light_elements", {"num_geoms": 0}, OK, None),
    ("pt_sky_table", {"n": 1025}, INVALID, "pt_sky_table: n = 1025 outside [0, 1024]"),
    ("pt_sky_table", {"texels": None}, INVALID, "pt_sky_table: null texels with n = 1"),
    ("pt_sky_table", {"n": 0}, OK, None),
    ("pt_environment_texel", {"n": 0}, INVALID, "pt_environment_texel: bad argument (count 2, n 0)"),
    ("pt_environment_texel", {"count": -1}, INVALID, "pt_environment_texel: bad argument (count -1, n 1)"),
    ("pt_environment_texel", {"count": 0}, OK, None),
    ("pt_probe_environment", {"n": 1025}, INVALID, "pt_probe_environment: bad argument (count 2, n 1025)"),
    ("pt_probe_environment", {"colour": None}, INVALID, "pt_probe_environment: bad argument (count 2, n 1)"),
    ("pt_probe_environment", {"count": 0}, OK, None),
    ("pt_texture_texel", {"n": 0}, INVALID, "pt_texture_texel: bad argument (count 2, 2 geoms, n 0)"),
    ("pt_texture_texel", {"hit_geom": LAST_GEOM}, INVALID, "pt_texture_texel: record 1 names primitive 2 of 2"),
    ("pt_texture_texel", {"index": None}, INVALID, "pt_texture_texel: null index"),
    ("pt_texture_texel", {"count": 0}, OK, None),
    ("pt_probe_texture", {"n": 1025}, INVALID, "pt_probe_texture: bad argument (count 2, 2 geoms, n 1025)"),
    ("pt_probe_texture", {"hit_geom": LAST_GEOM}, INVALID, "pt_probe_texture: record 1 names primitive 2 of 2"),
    ("pt_probe_texture", {"texels": None}, INVALID, "pt_probe_texture: bad argument (count 2)"),
    ("pt_probe_texture", {"count": 0}, OK, None),
    ("pt_bump_normal", {"n": 0}, INVALID, "pt_bump_normal: bad argument (count 2, 2 geoms, n 0)"),
    ("pt_bump_normal", {"hit_geom": LAST_GEOM}, INVALID, "pt_bump_normal: record 1 names primitive 2 of 2"),
    ("pt_bump_normal", {"perturbed": None}, INVALID, "pt_bump_normal: null array (count 2)"),
    ("pt_bump_normal", {"count": 0}, OK, None),
    ("pt_probe_bump_normal", {"count": -1}, INVALID, "pt_probe_bump_normal: bad argument (count -1, 2 geoms, n 1)"),
    ("pt_probe_bump_normal", {"hit_geom": LAST_GEOM}, INVALID, "pt_probe_bump_normal: record 1 names primitive 2 of 2"),
    ("pt_probe_bump_normal", {"texels": None}, INVALID, "pt_probe_bump_normal: null array (count 2)"),
    ("pt_probe_bump_normal", {"count": 0}, OK, None),
    # ---- meshes ----
    ("pt_probe_tri_form", {"count": -1}, INVALID, "pt_probe_tri_form: bad argument"),
    ("pt_probe_tri_form", {"origins": None}, INVALID, "pt_probe_tri_form: bad argument"),
    ("pt_probe_tri_form", {"n": (1 << 22) + 1}, INVALID, "pt_probe_tri_form: 4194305 rays x 64 records (at most 2^28)"),
    ("pt_probe_tri_form", {"count": 0}, OK, None),
    ("pt_probe_tri_form", {"n": 0}, 64, None),
    ("pt_bvh_build", {"count": -1}, INVALID, "pt_bvh_build: bad triangle list"),
    ("pt_bvh_build", {"triangles": None}, INVALID, "pt_bvh_build: bad triangle list"),
    ("pt_tri_bounds", {"bounds": None}, INVALID, "pt_tri_bounds: bad argument"),
    ("pt_tri_bounds", {"count": 0}, OK, None),
    ("pt_tri_records", {"frame": None}, INVALID, "pt_tri_records: bad argument"),
    ("pt_tri_records", {"count": 0}, OK, None),
    ("pt_cull_boxes", {"boxes": None}, INVALID, "pt_cull_boxes: bad argument"),
    ("pt_cull_boxes", {"count": -1}, INVALID, "pt_cull_boxes: bad argument"),
    ("pt_cull_boxes", {"count": 0}, OK, None),
]

# where a check can pre-empt another, the order is behaviour: two faults, and the one that is reported
ORDER = [
    # the argument check comes before the per-record loops ...
    ("pt_probe_shade_scatter", {"deferred": 2, "isects": LAST_MATERIAL}, INVALID, "pt_probe_shade_scatter: bad argument"),
    ("pt_probe_shade_scatter_direct", {"depth": 3, "isects": LAST_MATERIAL}, INVALID, "pt_probe_shade_scatter_direct: bad argument"),
    ("pt_probe_shade_scatter_direct_sky", {"env_n": 1025, "n": -1}, INVALID, "pt_probe_shade_scatter_direct_sky: bad map (n = 1025)"),
    # ... a record's material before its primitive, the records before the tables, the tables before the light table ...
    ("pt_probe_shade_scatter_textured", {"isects": LAST_MATERIAL, "hit_geom": LAST_GEOM}, INVALID,
     "pt_probe_shade_scatter_textured: record 1 hits material 2 of 2"),
    ("pt_probe_shade_scatter_bumped", {"hit_geom": LAST_GEOM, "tex_n": i32(1, 1025)}, INVALID,
     "pt_probe_shade_scatter_bumped: record 1 names primitive 2 of 2"),
    ("pt_probe_shade_scatter_bumped", {"tex_n": i32(1, 1025), "bump_texels": None}, INVALID,
     "pt_probe_shade_scatter_bumped: material 1 has a texture of n = 1025 at offset 0"),
    ("pt_probe_shade_scatter_direct", {"isects": LAST_MATERIAL, "geoms": lambda pt: geoms(pt, (0, 2))}, INVALID,
     "pt_probe_shade_scatter_direct: record 1 hits material 2 of 2"),
    ("pt_probe_direct_sample", {"count": -1, "num_materials": 0}, INVALID, "pt_probe_direct_sample: bad argument"),
    ("pt_probe_bump_normal", {"hit_geom": LAST_GEOM, "texels": None}, INVALID, "pt_probe_bump_normal: record 1 names primitive 2 of 2"),
    ("pt_probe_texture", {"hit_geom": LAST_GEOM, "texels": None}, INVALID, "pt_probe_texture: record 1 names primitive 2 of 2"),
    # ... and every one of them before `n == 0 -> PT_OK`
    ("pt_probe_shade_scatter_textured", {"n": 0, "tex_n": i32(1, 1025)}, INVALID,
     "pt_probe_shade_scatter_textured: material 1 has a texture of n = 1025 at offset 0"),
    ("pt_probe_shade_scatter_textured", {"n": 0, "tex_texels": None}, INVALID, "pt_probe_shade_scatter_textured: null tex_texels"),
    ("pt_probe_shade_scatter_bumped", {"n": 0, "bump_n": i32(1025, 0)}, INVALID,
     "pt_probe_shade_scatter_bumped: material 0 has a bump map of n = 1025 at offset 0"),
    ("pt_probe_shade_scatter_bumped", {"n": 0, "bump_texels": None}, INVALID, "pt_probe_shade_scatter_bumped: null texels"),
    ("pt_probe_shade_scatter_direct", {"n": 0, "geoms": lambda pt: geoms(pt, (0, 2))}, INVALID,
     "pt_probe_shade_scatter_direct: a cube or sphere names a material outside [0, 2)"),
    ("pt_probe_direct_sample", {"count": 0, "geoms": lambda pt: geoms(pt, (0, 2))}, INVALID,
     "pt_probe_direct_sample: a cube or sphere names a material outside [0, 2)"),
    ("pt_probe_sky_sample", {"count": 0, "n": 1025}, INVALID, "pt_probe_sky_sample: bad argument (n = 1025, count = 0)"),
    ("pt_probe_texture", {"count": 0, "texels": None}, INVALID, "pt_probe_texture: bad argument (count 0)"),
    ("pt_probe_bump_normal", {"count": 0, "texels": None}, INVALID, "pt_probe_bump_normal: null array (count 0)"),
    ("pt_probe_environment", {"count": 0, "n": 1025}, INVALID, "pt_probe_environment: bad argument (count 0, n 1025)"),
]

# one sound one-record call per entry point that allocates on the device: (entry point, what makes it one record)
ALLOCATING = [
    ("pt_probe_rng", {"n": 1}), ("pt_probe_sincos", {"n": 1}), ("pt_probe_sqrt", {"n": 1}), ("pt_probe_hemisphere", {"n": 1}),
    ("pt_probe_glossy_lobe", {"n": 1}), ("pt_probe_shade_scatter", {"n": 1}), ("pt_probe_shade_scatter_glossy", {"n": 1}),
    ("pt_probe_shade_scatter_textured", {"n": 1}), ("pt_probe_shade_scatter_bumped", {"n": 1}), ("pt_probe_shade_scatter_direct", {"n": 1}),
    ("pt_probe_shade_scatter_direct_sky", {"n": 1}), ("pt_probe_direct_sample", {"count": 1}), ("pt_probe_sky_sample", {"count": 1}),
    ("pt_probe_environment", {"count": 1}), ("pt_probe_texture", {"count": 1}), ("pt_probe_bump_normal", {"count": 1}),
    ("pt_probe_tri_form", {"n": 1}),
]


def call(pt, entry, changed):
    """entry(SOUND's arguments with `changed` put in); the arrays live until the call returns."""
    assert set(changed) <= {name for name, _ in SOUND[entry]}, (entry, changed)
    keep, args = [], []
    for name, value in SOUND[entry]:
        value = changed.get(name, value)
        if callable(value):
            value = value(pt)
        if isinstance(value, np.ndarray):
            value = np.ascontiguousarray(value).copy()
            keep.append(value)
            value = value.ctypes.data
        args.append(value)
    L = pt.library()
    rc = getattr(L, entry)(*args)
    return rc, L.pt_last_error().decode()


def case_id(case):
    return "%s-%s" % (case[0][3:], "-".join("%s" % k for k in case[1]))


@pytest.mark.parametrize("case", REFUSALS + ORDER, ids=case_id)
def test_refusal(pt, case):
    entry, changed, want_rc, want_text = case
    rc, text = call(pt, entry, changed)
    assert rc == want_rc, (rc, text)
    if want_text is not None:
        assert text == want_text


def test_every_entry_point_that_can_refuse_is_pinned():
    refused = {entry for entry, _, rc, _ in REFUSALS if rc < 0}
    assert refused == set(SOUND)
    counted = {entry for entry, _ in SOUND.items() if any(name in ("n", "count") for name, _ in SOUND[entry])}
    empty = {entry for entry, changed, rc, _ in REFUSALS if rc >= 0 and list(changed.values()) == [0]}
    assert counted - empty == {"pt_bvh_build"}                 # (an empty mesh still has a tree: a node count, not PT_OK)


@pytest.mark.parametrize("case", ALLOCATING, ids=case_id)
def test_no_device_no_answer(pt, case):
    """Without a GPU a sound call fails at its first allocation, and says which entry point it was."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    entry, changed = case
    rc, text = call(pt, entry, changed)
    assert rc == DEVICE, (rc, text)
    assert text == NO_DEVICE % entry


def test_no_device_no_clock(pt):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    rc, text = call(pt, "pt_probe_clock", {})
    assert rc == DEVICE, (rc, text)
    assert text == "pt_probe_clock: no HIP device / no mappable host memory (this library has no CPU fallback)"
