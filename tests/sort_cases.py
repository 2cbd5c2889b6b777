"""The material sort at its key-count edges, shared by tests/test_sort_cases_cpu.py and tests/test_gpu_sort_keys.py: a room whose
walls are a mosaic of up to 2047 materials, the table of cases (material count, flags, frame -> the device form pt_init and
enqueue_bounce take: csrc/pt_h_api.hpp, csrc/pt_h_enqueue.hpp), the specification of the pool order in numpy, and the oracle's runs
of the cases, computed once per process and read-only from then on.

The three forms: `fused` -- k_bounce<..., SORT>, lane k of a wave counts key k, up to 64 materials;
`wave` -- k_sort_hist + k_shade_sorted_w, up to 64 bins (materials + the miss bin); `workgroup` -- k_sort_hist + k_shade_sorted,
65 to SORT_MAX_BINS = 2048 bins, an LDS counting sort per 512-path chunk."""
import numpy as np

import random_scenes as rs
from gpu_common import _resized

F32 = np.float32
DEPTH = 6
SORT_MAX_BINS = 2048                                                 # csrc/pt_k_sort.hpp
TILE, STRIP, CHUNK = 64, 128, 512                                    # a tile, one wave's two tiles of a chunk, a chunk
N_CUBES, N_SPHERES = 125, 20
N_GEOMS = N_CUBES + N_SPHERES
SPHERE, CUBE = 0, 1
EMITTER, MIRROR, GLASS = 0, 3, 5                                     # material m's kind by m % 8; the rest are matte
FRAME = (64, 48)
# The cases' room.  Every seed tried (0 .. 11) meets the floors of tests/test_sort_cases_cpu.py at 64 x 48; at 67 x 5, where a dozen
# paths survive bounce 0, seed 0 leaves no two survivors with one key (an unstable sort would not show there): 8 leaves them at
# six bounces of the two iterations.
SEED = 8


def mosaic_room(pt, M, seed=0, all_emissive=False):
    """(geoms, materials): the Cornell volume x, z in [-5, 5], y in [0, 10], front open; floor, ceiling, back, left and right
    tiled 5 x 5 by cubes of scale (2, 0.1, 2) laid flat against their wall, 20 spheres of scale 1.5 inside; no rotations.
    materialid = permutation(145) % M, one sphere forced to M - 1 and one tile of the floor to 0.  Material m by m % 8:
    0 an emitter (3), 3 a mirror, 5 glass (1.5), the rest matte -- M = 1 is a room in which every hit ends the path."""
    H = pt.host_binding.host_library()
    rng = np.random.default_rng(seed)
    geoms = np.zeros(N_GEOMS, dtype=pt.GEOM_DT)
    centres = (-4.0, -2.0, 0.0, 2.0, 4.0)
    k = 0
    for wall in ("floor", "ceiling", "back", "left", "right"):
        for a in centres:
            for b in centres:
                g = geoms[k]
                g["type"] = CUBE
                if wall in ("floor", "ceiling"):
                    g["translation"], g["scale"] = (a, 0.0 if wall == "floor" else 10.0, b), (2.0, 0.1, 2.0)
                elif wall == "back":
                    g["translation"], g["scale"] = (a, b + 5.0, -5.0), (2.0, 2.0, 0.1)
                else:
                    g["translation"], g["scale"] = (-5.0 if wall == "left" else 5.0, a + 5.0, b), (0.1, 2.0, 2.0)
                k += 1
    for g in geoms[N_CUBES:]:
        g["type"] = SPHERE
        g["translation"] = rng.uniform(-3.5, 3.5, 3) + (0, 5, 0)
        g["scale"] = 1.5
    ids = rng.permutation(N_GEOMS) % M
    # key 0 and key M - 1 go to a floor tile and a sphere that the flat frames (67 x 5, 130 x 9) see too, where all but a few dozen
    # rays miss -- by exchange with a primitive that has the key, so that every key of the permutation stays in use
    for at, key in ((3, 0), (128, M - 1)):
        other = int(np.nonzero(ids == key)[0][0]) if (ids == key).any() else at
        ids[other], ids[at] = ids[at], key
    geoms["materialid"] = ids
    for k in range(N_GEOMS):
        H.pth_build_geom_matrices(geoms.ctypes.data + k * pt.GEOM_DT.itemsize)
    mats = np.zeros(M, dtype=pt.MATERIAL_DT)
    mats["color"] = rng.uniform(0.3, 1.0, (M, 3))
    mats["spec_color"] = rng.uniform(0.3, 1.0, (M, 3))
    kind = np.arange(M) % 8
    mats["emittance"] = np.where((kind == EMITTER) | all_emissive, 3.0, 0.0)
    mats["hasReflective"] = np.where(kind == MIRROR, 1.0, 0.0)
    mats["hasRefractive"] = np.where(kind == GLASS, 1.0, 0.0)
    mats["indexOfRefraction"] = np.where(kind == GLASS, 1.5, 0.0)
    return geoms, mats


def camera(w, h):
    return _resized(rs.base_camera(), w, h)


def keys_entering(po, geoms, M, paths):
    """The sort keys of a pool before its bounce: the material each path hits, M (the miss bin) where it hits nothing."""
    isects, _ = po.compute_intersections(np.ascontiguousarray(paths), np.ascontiguousarray(geoms).view(po.GEOM_DT))
    return np.where(isects["t"] > 0, isects["materialId"], M).astype(np.int64)


def expected_order(keys, pixel_index, survivors):
    """The specification: the pool after a bounce is the stable sort of the entering pool by key, then the stable partition by
    survival -- the pixel indices of `survivors` in that order."""
    order = np.asarray(pixel_index)[np.argsort(keys, kind="stable")]
    return order[np.isin(order, survivors)]


class Case:
    def __init__(self, id, M, flags, form, frames=(FRAME,), all_emissive=False):
        self.id, self.M, self.flags, self.form, self.frames, self.all_emissive = id, M, flags, form, frames, all_emissive
        self.compact = "COMPACT" in flags
        self.nbins = M + 1

    def pt_flags(self, pt):
        return (pt.PT_COMPACT if self.compact else 0) | pt.PT_SORT_MATERIAL | (pt.PT_UNFUSED if "UNFUSED" in self.flags else 0)

    def oracle_flags(self, po):
        return (po.F_COMPACT if self.compact else 0) | po.F_SORT


CS, CSU = ("COMPACT", "SORT"), ("COMPACT", "SORT", "UNFUSED")
CASES = (
    [Case("f%d" % M, M, CS, "fused") for M in (1, 2, 63, 64)]
    + [Case("w%d" % M, M, CSU, "wave") for M in (1, 62, 63)]         # 2, 63 and 64 bins: lane 63 holds the miss bin
    + [Case("g64", 64, CSU, "workgroup"),                            # 65 bins; the table's 65 x 6 words end on a ragged uint4
       Case("g65", 65, CS, "workgroup", (FRAME, (67, 5), (130, 9))),  # chosen by the count alone
       Case("g127", 127, CS, "workgroup"),                           # 128 bins -> nb 128
       Case("g128", 128, CS, "workgroup"),                           # 129 bins -> nb 132
       Case("g2047", 2047, CS, "workgroup", (FRAME, (128, 72))),     # SORT_MAX_BINS: 2048 x 6 words in one barrier, 2048 x 18 stepped
       Case("g65e", 65, CS, "workgroup", all_emissive=True),         # every bin's count is zeroed
       Case("n63", 63, ("SORT",), "wave"),
       Case("n65", 65, ("SORT",), "workgroup")]
)
BY_ID = {c.id: c for c in CASES}
RUNS = [(c.id, frame) for c in CASES for frame in c.frames]          # every (case, frame) the modules run


def run_id(run):
    return "%s-%dx%d" % (run[0], run[1][0], run[1][1])


def form_of(case):
    """The rule of pt_init / enqueue_bounce, restated: which device form a session of this case takes."""
    if case.compact and "UNFUSED" not in case.flags and case.M <= 64:
        return "fused"
    assert case.nbins <= SORT_MAX_BINS
    return "wave" if case.nbins <= 64 else "workgroup"


class Reference:
    """The oracle's side of one (case, frame): per iteration 1 .. 3 the bounce snapshots (pyoracle.Tracer.iterate), the live
    counts, the rays and the running sum -- `snaps[it]`, `live[it]`, `rays[it]`, `images[it]`."""


_cache = {}
ITERATIONS = (1, 2, 3)


def scene_of(pt, case):
    key = ("scene", case.id)
    if key not in _cache:
        _cache[key] = mosaic_room(pt, case.M, seed=SEED, all_emissive=case.all_emissive)
    return _cache[key]


def _run(po, geoms, mats, cam, oflags):
    ref = po.Tracer(np.ascontiguousarray(geoms).view(po.GEOM_DT), mats.view(po.MATERIAL_DT), cam, DEPTH, flags=oflags, trig=po.TRIG_SHARED)
    r = Reference()
    r.snaps, r.live, r.rays, r.images = {}, {}, {}, {}
    for it in ITERATIONS:
        snaps = []
        st = ref.iterate(it, snapshots=snaps)
        for s in snaps:
            s["paths"].setflags(write=False)
        img = ref.image.copy()
        img.setflags(write=False)
        r.snaps[it], r.live[it], r.rays[it], r.images[it] = snaps, list(st.live[:DEPTH]), int(st.rays), img
    return r


def reference(po, pt, case, frame):
    """The oracle under the case's own flags (F_SORT with or without F_COMPACT)."""
    key = ("ref", case.id, frame)
    if key not in _cache:
        geoms, mats = scene_of(pt, case)
        _cache[key] = _run(po, geoms, mats, camera(*frame), case.oracle_flags(po))
    return _cache[key]


def unsorted_reference(po, pt, case, frame):
    """The oracle with F_COMPACT alone on the same room."""
    key = ("plain", case.id, frame)
    if key not in _cache:
        geoms, mats = scene_of(pt, case)
        _cache[key] = _run(po, geoms, mats, camera(*frame), po.F_COMPACT)
    return _cache[key]


def entering(po, ref, frame, it, d):
    """The pool that enters bounce d of iteration `it` of a compacting run: the camera rays, or the survivors of bounce d - 1."""
    if d == 0:
        return po.generate_rays(camera(*frame), DEPTH)
    s = ref.snaps[it][d - 1]
    return s["paths"][:s["n_live"]]


def distinct_in_runs(keys, run):
    """The largest number of distinct keys in one run of `run` consecutive pool positions."""
    return max(len(np.unique(keys[k:k + run])) for k in range(0, len(keys), run)) if len(keys) else 0


def same_key_pairs_in_a_tile(keys):
    """The largest number of pairs of equal keys inside one 64-path tile."""
    best = 0
    for k in range(0, len(keys), TILE):
        _, counts = np.unique(keys[k:k + TILE], return_counts=True)
        best = max(best, int((counts * (counts - 1) // 2).sum()))
    return best
