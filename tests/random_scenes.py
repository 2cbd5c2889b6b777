"""Random hostile scenes, shared by tests/tools/fuzz_gpu.py, tests/test_gpu_random_scenes.py and
tests/test_random_scenes_cpu.py: cubes and spheres under arbitrary rotations, thin slabs (0.001), scales of 100 and 1e-4, a zero
scale (no finite inverse: the primitive is never hit), enclosing shells, an eye inside primitives, 1 to 39 primitives, depths 1 to
11, random materials.

`scene(pt, seed, w, h)` draws from default_rng(seed) in the order the fuzz tool always drew: seed N is the scene it always was.
Everything newer -- the GGX exponents, textures, bump maps, the sky -- comes from a second stream, default_rng([seed, 1]), in
`features()`, so the first stream never moves.  Further streams follow the same rule: default_rng([seed, 2]) is the mesh session's
soup (`mesh_of`), [seed, 3] the camera's jitter and lens (`camera_features`), [seed, 4] the soup's vertex normals (`normals_of`),
[seed, 5] the sky that is sampled as a light and whether the lamps are off (`sky_of`)."""
import os

import numpy as np

import bump_model as bm
import texture_model as tm
from gpu_common import _resized

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
MAX_DEPTH = 64                                                       # pt_stats::live; a PT_DIRECT_LIGHT session traces depth + 1 bounces
_base = {}


def base_camera():
    """The 64 x 64 Cornell camera every scene's camera is a perturbation of."""
    if "cam" not in _base:
        z = np.load(os.path.join(ROOT, "tests", "golden", "scenes.npz"))
        _base["cam"] = np.array(z["cornell_64__camera"], copy=True).reshape(1)
    return _base["cam"].copy()


def draw(pt, seed, w, h):
    """The first stream, whole: (geoms, materials, camera, depth, per_bounce, rng).  per_bounce is the tool's draw of a launch plan
    (a kernel per bounce, or small batches in one launch) -- the caller's to apply; rng stands where the tool's cull-stress rays
    continue."""
    H = pt.host_binding.host_library()
    rng = np.random.default_rng(seed)
    nm = int(rng.integers(2, 12))
    mats = np.zeros(nm, dtype=pt.MATERIAL_DT)
    for m in mats:
        m["color"] = rng.uniform(0.1, 1.0, 3)
        m["spec_color"] = rng.uniform(0.5, 1.0, 3)
        kind = rng.integers(4)
        m["hasReflective"], m["hasRefractive"] = (1.0, 0.0) if kind == 1 else ((0.0, 1.0) if kind == 2 else (0.0, 0.0))
        m["indexOfRefraction"] = rng.uniform(1.05, 2.5)
        m["emittance"] = rng.uniform(1, 6) if kind == 3 else 0.0
    mats[0]["emittance"] = 4.0
    ng = int(rng.integers(1, 40))
    geoms = np.zeros(ng, dtype=pt.GEOM_DT)
    for k, g in enumerate(geoms):
        g["type"] = rng.integers(2)
        g["materialid"] = rng.integers(nm)
        g["translation"] = rng.uniform(-5, 5, 3) + (0, 5, 0)
        g["rotation"] = rng.uniform(-180, 180, 3) * (rng.random() < 0.6) + rng.choice([0.0, 90.0, 180.0, 45.0], 3) * (rng.random() < 0.3)
        sc = rng.uniform(0.2, 4.0, 3)
        r = rng.random()
        if r < 0.2:
            sc[rng.integers(3)] = rng.choice([0.02, 0.005, 0.001])
        elif r < 0.25:
            sc = np.full(3, rng.choice([30.0, 100.0]))
        elif r < 0.3:
            sc = np.full(3, rng.choice([1e-2, 1e-4]))
        elif r < 0.33:
            sc[rng.integers(3)] = 0.0
        g["scale"] = sc
        H.pth_build_geom_matrices(geoms.ctypes.data + k * pt.GEOM_DT.itemsize)
    depth = int(rng.integers(1, 12))
    # the camera moves too (the bounce-0 candidate masks and the cull boxes' reach follow it): near the scene, far
    # outside it, sometimes looking elsewhere
    cam = _resized(base_camera(), w, h)
    r = rng.random()
    if r < 0.5:
        cam["position"][0] += rng.uniform(-3, 3, 3).astype(np.float32)
    elif r < 0.6:
        cam["position"][0] += (rng.uniform(-1, 1, 3) * rng.choice([30.0, 300.0])).astype(np.float32)
    if rng.random() < 0.2:
        a = rng.uniform(-0.8, 0.8)
        cam["view"][0] = np.float32([np.sin(a), 0.0, np.cos(a)]) * np.float32(np.sign(cam["view"][0][2]) or 1.0)
    per_bounce = bool(rng.random() < 0.5)
    return geoms, mats, cam, depth, per_bounce, rng


def scene(pt, seed, w, h):
    """(geoms, materials, camera at w x h, depth) of seed `seed`."""
    return draw(pt, seed, w, h)[:4]


def zero_scaled(geoms):
    """Which primitives carry a zero scale (their inverse matrices have no finite entry)."""
    return (np.asarray(geoms["scale"]) == 0).any(axis=1)


class Features:
    """What the second stream adds to a scene: `materials` (the scene's with spec_exponent drawn), `textures` and `bump_maps`
    ({material: [6, n, n, 3] float32}), `sky` (a [6, 4, 4, 3] gradient or None), `direct_depth`."""


def _gradient(rng):
    """A 4-texel sky: a colour at the horizon, another overhead, blended by the height of each texel's direction."""
    low, high = rng.uniform(0.0, 1.5, 3), rng.uniform(0.0, 2.5, 3)
    out = np.zeros((6, 4, 4, 3), dtype=F32)
    ramp = (np.arange(4) + 0.5) / 4.0
    for face in range(6):
        for j in range(4):
            for i in range(4):
                s = ramp[(i + j + face) % 4]
                out[face, j, i] = low * (1.0 - s) + high * s
    return out


def features(seed, materials, depth):
    """The second stream, default_rng([seed, 1]): exponents from {0, 2, 50, 1e4} (the lobe off and on); per material a
    checker texture and / or a bump map (studs, or noise with a flat row) of 1, 4 or 8 texels a side with slopes up to 3;
    a sky or none; the depth of the PT_DIRECT_LIGHT session."""
    rng = np.random.default_rng([seed, 1])
    f = Features()
    f.materials = np.array(materials, copy=True)
    f.materials["spec_exponent"] = rng.choice([0.0, 2.0, 50.0, 1e4], len(materials))
    f.textures, f.bump_maps = {}, {}
    for m in range(len(materials)):
        r = rng.random(2)
        n = int(rng.choice([1, 4, 8]))
        cells = int(rng.choice([1, 2, 4]))
        c0, c1 = rng.uniform(0.0, 2.0, 3), rng.uniform(0.0, 2.0, 3)
        slope = float(rng.uniform(0.1, 3.0))
        noise = rng.normal(0, slope, (6, n, n, 3)).astype(F32)
        use_studs = rng.random() < 0.5
        if r[0] < 0.5:
            f.textures[m] = tm.checker(n, min(cells, n), c0, c1)
        if r[1] < 0.4:
            if use_studs:
                f.bump_maps[m] = bm.studs(n, min(cells, n), slope)
            else:
                if n > 1:
                    noise[:, 0, :, :2] = 0                           # a row of flat texels: not perturbed
                f.bump_maps[m] = noise
    f.sky = _gradient(rng) if rng.random() < 0.75 else None
    f.direct_depth = min(int(depth), MAX_DEPTH - 1)
    return f


# ---- the seed lists and what the models say about them (no device) -------------------------------------------------------------
W, H = 40, 26                                                        # 1040 paths: 16 full waves and a 16-lane tail
WIDE = (130, 9)                                                      # one seed of every session also runs flat and wide
BATCHES = ((4, 1), (5, 1), (6, 2), (8, 1), (9, 1))                   # the tool's batches on the lanes, after iterations 1-3
MOVE = (0.3, 0.2, 0.0)
SIGMAS = (1.0, 0.35, 0.5)
_refs = {}
# Chosen with the generator above so that tests/test_random_scenes_cpu.py's floors hold for every list (they are conditions on the
# lists, asserted there).  The first seed of a list also runs at 130 x 9: 1029 has depth 11, 21 primitives, the eye inside one,
# textures, bump maps, both kinds of light element.  1028 is a single primitive that every camera ray misses.
COMMON_SEEDS = (1029, 1000, 1002, 1003, 1004, 1006, 1007, 1008, 1009, 1012, 1014, 1016, 1018, 1022, 1024, 1026)
PLAIN_SEEDS = (1029, 1000, 1002, 1028, 1004, 1006, 1007, 1008, 1009, 1012, 1014, 1016, 1018, 1022, 1024, 1026)
GLOSSY_SEEDS = COMMON_SEEDS
TEXTURED_SEEDS = COMMON_SEEDS
DIRECT_SEEDS = COMMON_SEEDS                                          # every one has between 1 and 1024 light elements
FILTER_SEEDS = PLAIN_SEEDS
MESH_SEEDS = (1029, 1009, 1012, 1024)
# The first-state table's sessions: no seed of the list draws a refractive material, so pt_init gives every
# one of them the table.  They also run at STATE_FRAME, whose 1024 pixels are whole 64-pixel tiles: the ended-tile words exist.
# 1110, 1136, 1176 and 1087 hold all four kinds of record with whole-ended tiles beside mixed ones; 1067 and 1087 have exactly 16
# primitives; 1089 has 4; 1127 and 1013 have the eye inside a primitive; 1073 and 1060 have depth 2 (1060: 38 primitives, two
# zero-scaled); every ray of 1153 misses; every pixel of 1100 is a mirror hit from inside; 1079 has depth 1; 1089, 1127 and 1191 have
# depth 8 or more; in 1009, 1191 and 1188 emitter, mirror and diffuse pixels share tiles and no ray misses.
STATE_SEEDS = (1009, 1191, 1110, 1136, 1176, 1087, 1067, 1089, 1127, 1013, 1073, 1060, 1153, 1188, 1079, 1100)
STATE_FRAME = (64, 16)
# ... of them, the PT_DIRECT_LIGHT session without PT_GLOSSY and sky: depth 3 (1136, the least at which bounces 0 and 1 are plain ones)
# and more, between 1 and 1024 light elements
STATE_DIRECT_SEEDS = (1009, 1110, 1136, 1087, 1089, 1127, 1153, 1100)
STATE_DIRECT_MIN_DEPTH = 3                                           # below it bounce 1 is one of the session's DIRECT bounces
STATE_KINDS = ("drawn", "fixed", "coloured", "zero")                 # FS_DIFFUSE, FS_FIXED, FS_CONST, FS_ZERO
# The smooth sessions (PT_SMOOTH_NORMALS): the soup of mesh_of with normals_of's vertex normals.  Smoothed
# matte hits: 1029 (the soup fills much of the frame; depth 11, 21 primitives) and 1191 (25 primitives); smoothed mirror hits:
# 1002, 1008 and 1022 (depth 2, 31 primitives); smoothed glass hits: 1003 and 1024.  1000 has depth 1: its only bounce is the
# last one, which reads no normal -- steps 4 and 5 still refuse records there, and removing the normals changes nothing.
SMOOTH_SEEDS = (1029, 1002, 1003, 1022, 1191, 1008, 1024, 1000)
# The sampled-sky sessions (PT_DIRECT_SKY).  In the generator's scenes a sample aimed at the sky rarely
# leaves: the primitives of scale 30 and 100 enclose the rest (1029: some 800 aimed final rays, every one occluded).  So the
# seeds of SKY_OPENED run on opened(): the same draw without the primitives whose largest scale component is 30 or more.
# Closed: 1165 (depth 1, 26 primitives, lamps and a 4-texel sky), 1079 (depth 1, lamps off, a 1-texel map), 1392 (two
# primitives), 1029, 1231 (depth 5, lamps off), 1377 (depth 2, lamps off, 1 texel), 1086 (depth 7, 1 texel).  Opened: 1000, 1018,
# 1306 (depth 1, 16 texels; 1000 lamps off), 1060 (38 primitives, depth 2, lamps off, 1 texel), 1291 (1 texel), 1284, 1358
# (depth 4, lamps off), 1283 (depth 6), 1327 (depth 1, lamps off).  A seed's second map is sky_of(seed + 1)'s.
SKY_SEEDS = (1165, 1079, 1392, 1029, 1000, 1018, 1060, 1291, 1231, 1358, 1283, 1377, 1306, 1284, 1086, 1327)
SKY_OPENED = (1000, 1018, 1060, 1291, 1358, 1283, 1306, 1284, 1327)
# The sessions under camera_features(): a lens and no jitter on 1067 (0.35 focused at 0.5; 16 primitives, no refractive material:
# its pinhole stretch reads the first-state table), 1024 (the same lens; glass: the first-hit table alone), 1068 (2.0 at 1000; 25
# primitives, no refractive material) and 1000 (0.05 at 0.5; depth 1, 28 primitives: bounce 0 of its direct sessions is a DIRECT
# bounce that generates its rays); jitter and no lens on 1053 (no refractive material) and 1120 (17 primitives, depth 7); both on
# 1073 (2.0 at 0.5; depth 2, no refractive material) and 1030 (0.35 at 0.5; depth 9, 25 primitives, no refractive material).
CAMERA_SEEDS = (1067, 1024, 1053, 1073, 1068, 1000, 1120, 1030)


def groups(seeds):
    return [tuple(seeds[k:k + 4]) for k in range(0, len(seeds), 4)]


def next_seed(seeds, seed):
    return seeds[(seeds.index(seed) + 1) % len(seeds)]


def moved(cam, d):
    """position and lookAt translated by d: view / up / right stay"""
    c = cam.copy()
    c["position"][0] += np.asarray(d, dtype=F32)
    c["lookAt"][0] += np.asarray(d, dtype=F32)
    return c


def _cached(key, make):
    if key not in _refs:
        _refs[key] = make()
    return _refs[key]


class Run:
    """A model's side of a session: `images[it]` the running sum after iteration it (read-only), `live[it]` the paths traced at
    every bounce of iteration it, `ended[it]` the bounce at which each pixel's path of iteration it ended."""

    def __init__(self, n):
        self.n, self.images, self.live, self.ended = n, {}, {}, {}

    def record(self, it, image, survivors, live=None):
        """survivors: per bounce, the pixelIndex of the paths that survived it"""
        img = image.copy()
        img.setflags(write=False)
        self.images[it] = img
        cnt = np.zeros(self.n, dtype=np.int32)
        for pix in survivors:
            cnt[pix] += 1
        self.ended[it] = cnt
        self.live[it] = list(live) if live is not None else [self.n] + [len(pix) for pix in survivors]

    def live_sum(self, its, depth):
        out = [0] * depth
        for it in its:
            for d, v in enumerate(self.live[it][:depth]):
                out[d] += v
        return out


def mesh_of(pt, seed, geoms, n_materials):
    """The mesh session's soup of 300 triangles (slivers, zero-area and metre-sized ones) from default_rng([seed, 2]):
    (geoms with the mesh primitive, triangles, meshes)."""
    import mesh_cases
    rng = np.random.default_rng([seed, 2])
    tris = mesh_cases.soup(pt.TRI_DT, rng, n=300)
    return pt.meshes.add_mesh(geoms, tris, material_id=int(rng.integers(n_materials)))


RADII, FOCALS = (0.0, 0.05, 0.35, 2.0), (0.5, 9.0, 1e3)


def camera_features(seed):
    """The fourth stream, default_rng([seed, 3]): (aa, (lens radius, focal distance)) -- PT_AA_JITTER or not, a thin lens from a
    pinprick to one two units wide focused in front of the scene, inside it or far behind it.  A radius of 0 is no lens."""
    rng = np.random.default_rng([seed, 3])
    aa = bool(rng.random() < 0.5)
    radius, focal = float(rng.choice(RADII)), float(rng.choice(FOCALS))
    return aa, (radius, focal)


def lens_only(seed):
    aa, lens = camera_features(seed)
    return lens[0] > 0 and not aa


class CameraPlan:
    """How a run of a session uses the seed's camera features.  camera=False: the pinhole, iterations 1 .. last.  camera=True: `aa`
    and `lens` for the model, then iteration last + 1 -- the one the GPU module steps: `Run.stepped` keeps its live paths after
    bounce 0 --; a seed with a lens and no jitter goes on with last + 2 and last + 3 under the pinhole (pt_set_lens(0, 0)) and
    last + 4 and last + 5 under its lens again: `switch` = {iteration: the lens from the iteration after it on}."""

    def __init__(self, seed, camera, last):
        self.aa, self.lens, self.last, self.end, self.step, self.switch = False, (0.0, 0.0), last, last, None, {}
        if camera:
            self.aa, self.lens = camera_features(seed)
            self.step = last + 1
            self.end = last + 1
            if lens_only(seed):
                self.end = last + 5
                self.switch = {last + 1: (0.0, 0.0), last + 3: self.lens}

    def kw(self):
        return dict(aa=self.aa, lens=self.lens if self.lens[0] > 0 else (0.0, 0.0))

    def its(self):
        return range(1, self.end + 1)


def plain_run(po, pt, seed, w, h, oflags, cam=None, mesh=False, last=9, camera=False):
    """po.Tracer over iterations 1 .. last; cam: another camera than the seed's own; camera: CameraPlan."""
    def make():
        geoms, mats, c, depth = scene(pt, seed, w, h)
        tris = meshes = None
        if mesh:
            geoms, tris, meshes = mesh_of(pt, seed, geoms, len(mats))
            tris, meshes = tris.view(po.TRI_DT), meshes.view(po.MESH_DT)
        plan = CameraPlan(seed, camera, last)
        ref = po.Tracer(np.ascontiguousarray(geoms).view(po.GEOM_DT), mats.view(po.MATERIAL_DT), c if cam is None else cam, depth,
                        flags=oflags | (po.F_AA if plan.aa else 0), trig=po.TRIG_SHARED, tris=tris, meshes=meshes, lens=plan.kw()["lens"])
        run = Run(w * h)
        run.plan, run.rays, run.moments = plan, {}, {}
        acc = np.zeros((w * h, 3), dtype=F32)
        m1, m2 = np.zeros(w * h, dtype=F32), np.zeros(w * h, dtype=F32)
        for it in plan.its():
            snaps = []
            if camera:                                                   # per-sample colours, as tests/test_gpu_variance_random_scenes.py
                import variance_model                                    # takes them: the sum is the same sum, and PT_MOMENTS' planes
                ref.image[:] = 0
            st = ref.iterate(it, snapshots=snaps)
            if camera:
                acc = (acc + ref.image).astype(F32)
                m1, m2 = variance_model.accumulate(m1, m2, ref.image)
                run.moments[it] = (m1, m2)
            alive = [s["paths"]["pixelIndex"][s["paths"]["remainingBounces"] > 0] for s in snaps]
            run.record(it, acc if camera else ref.image, alive, live=list(st.live[:depth]))
            run.rays[it] = int(st.rays)
            if it == plan.step:
                p = snaps[0]["paths"]
                run.stepped = p[p["remainingBounces"] > 0].copy()
            if it in plan.switch:
                ref.scene.lensRadius, ref.scene.focalDistance = plan.switch[it]
        return run
    return _cached(("plain", seed, w, h, oflags, None if cam is None else cam.tobytes(), mesh, last, camera), make)


def _model_run(m, n, depth, its, after=None, direct=False, plan=None):
    run = Run(n)
    run.plan = plan
    for it in its:
        snaps = []
        m.iterate(it, snaps)
        run.record(it, m.image, [s["pixelIndex"] for s in snaps], live=list(m.live) if direct and m.direct else None)
        run.live[it] = (run.live[it] + [0] * (depth + 1))[:depth + 1 if direct and m.direct else depth]
        if plan is not None and it == plan.step:
            run.stepped = snaps[0].copy()
        if plan is not None and it in plan.switch:
            m.lens = plan.switch[it]
        if after is not None:
            after(it, m)
    return run


def glossy_run(po, pt, seed, w, h, camera=False, last=9):
    """glossy_model.Model with the seed's sky over iterations 1 .. 9: (run, counts, features)."""
    def make():
        import glossy_model as gm
        geoms, mats, cam, depth = scene(pt, seed, w, h)
        f = features(seed, mats, depth)
        plan = CameraPlan(seed, camera, last)
        m = gm.Model(po, geoms, f.materials, cam, depth, glossy=True, **plan.kw())
        m.set_environment(f.sky)
        run = _model_run(m, w * h, depth, plan.its(), plan=plan)
        return run, {k: v for k, v in m.counts.items() if isinstance(v, int)}, f
    return _cached(("glossy", seed, w, h, camera, last), make)


def dropped(f):
    """The bump map and the texture the textured session removes after iteration 3: the lowest material that has one."""
    return (min(f.bump_maps) if f.bump_maps else None), (min(f.textures) if f.textures else None)


def textured_run(po, pt, seed, w, h, mesh=False, camera=False, last=5):
    """bump_model.Model with the seed's textures, bump maps, sky and exponents: iterations 1-3, one bump map and one texture
    removed, iterations 4-5.  (run, counts, features); counts: tinted, bumped, guarded and the lobe's."""
    def make():
        geoms, mats, cam, depth = scene(pt, seed, w, h)
        f = features(seed, mats, depth)
        tris = meshes = None
        if mesh:
            geoms, tris, meshes = mesh_of(pt, seed, geoms, len(mats))
        plan = CameraPlan(seed, camera, last)
        m = bm.Model(po, geoms, f.materials, cam, depth, tris=tris, meshes=meshes, glossy=True, **plan.kw())
        for k, t in f.textures.items():
            m.set_texture(k, t)
        for k, t in f.bump_maps.items():
            m.set_bump_map(k, t)
        m.set_environment(f.sky)
        b, t = dropped(f)

        def after(it, m):
            if it == 3:
                if b is not None:
                    m.set_bump_map(b, None)
                if t is not None:
                    m.set_texture(t, None)
        run = _model_run(m, w * h, depth, plan.its(), after, plan=plan)
        counts = {k: v for k, v in m.counts.items() if isinstance(v, int)}
        counts.update(tinted=m.tinted, bumped=m.bumped, guarded=m.guarded)
        return run, counts, f
    return _cached(("textured", seed, w, h, mesh, camera, last), make)


def direct_run(po, pt, seed, w, h, camera=False, last=9):
    """direct_model.Model with the seed's sky and exponents over iterations 1 .. 9: (run, counts, features, light elements)."""
    def make():
        import direct_model as dm
        geoms, mats, cam, depth = scene(pt, seed, w, h)
        f = features(seed, mats, depth)
        plan = CameraPlan(seed, camera, last)
        m = dm.Model(po, geoms, f.materials, cam, f.direct_depth, glossy=True, **plan.kw())
        m.set_environment(f.sky)
        run = _model_run(m, w * h, f.direct_depth, plan.its(), direct=True, plan=plan)
        return run, {k: v for k, v in m.counts.items() if isinstance(v, int)}, f, len(m.table)
    return _cached(("direct", seed, w, h, camera, last), make)


def plain_direct_run(po, pt, seed, w, h):
    """direct_model.Model without PT_GLOSSY and without a sky over iterations 1 .. 9, the scene's own materials: (run, counts,
    light elements).  The PT_DIRECT_LIGHT session whose bounces 0 and 1 are plain ones."""
    def make():
        import direct_model as dm
        geoms, mats, cam, depth = scene(pt, seed, w, h)
        depth = min(int(depth), MAX_DEPTH - 1)
        m = dm.Model(po, geoms, mats, cam, depth, glossy=False)
        run = _model_run(m, w * h, depth, range(1, 10), direct=True)
        return run, {k: v for k, v in m.counts.items() if isinstance(v, int)}, len(m.table)
    return _cached(("plain direct", seed, w, h), make)


def normals_of(pt, seed, tris):
    """Vertex normals for the mesh session's soup from default_rng([seed, 4]), [T, 3, 3] float32: the facet normal (0 where a
    zero-area triangle or a sliver has none that is finite) plus a lean of N(0, 0.5) per corner and component, then
    smooth_cases.scene_arrays("hostile")'s treatment: every 7th triangle faces away (step 4 refuses it), every 11th is zero, one
    NaN component, one infinite corner, one triangle of length 1e-20 and one of 1e20, one with a single zero corner."""
    import smooth_model
    rng = np.random.default_rng([seed, 4])
    fn = smooth_model.facet_normals(tris)
    fn = np.where(np.isfinite(fn).all(axis=1)[:, None], fn, F32(0)).astype(F32)
    vn = (fn[:, None, :] + rng.normal(0.0, 0.5, (len(tris), 3, 3))).astype(F32)
    vn[0::7] *= F32(-1)
    vn[3::11] = 0
    vn[2, 1, 0] = np.nan
    vn[4, 2] = np.inf
    vn[6] *= F32(1e-20)
    vn[8] *= F32(1e20)
    vn[10, 2] = 0
    return vn


def sky_of(pt, seed):
    """The sampled sky of a seed from default_rng([seed, 5]): (texels, lamps_off).  A gradient of 1, 4 or 16 texels a side
    (sky_model.gradient) with a sun of the stream's direction, width and colour, or -- one draw in four, where the seed has
    one -- the seed's features().sky.  lamps_off: the session runs on materials whose emittance is 0, the sky its only light."""
    import sky_model
    rng = np.random.default_rng([seed, 5])
    n = int(rng.choice([1, 4, 16]))
    own = bool(rng.random() < 0.25)
    lamps_off = bool(rng.random() < 0.3)
    direction = rng.normal(size=3)
    direction[1] = abs(direction[1]) + 0.2                              # above the horizon
    cos_half = float(rng.choice([0.97, 0.8]))
    rgb = rng.uniform(10.0, 60.0, 3)
    _, mats, _, depth = scene(pt, seed, W, H)
    f = features(seed, mats, depth)
    if own and f.sky is not None:
        return f.sky, lamps_off
    return pt.sun_on_cubemap(sky_model.gradient(pt, n), direction, cos_half, rgb), lamps_off


def opened(geoms):
    """The scene without its enclosing primitives -- those whose largest scale component is 30 or more --, the first primitive
    kept where every one is such: no new draw."""
    keep = np.asarray(geoms["scale"]).max(axis=1) < 30
    if not keep.any():
        keep[0] = True
    return np.ascontiguousarray(geoms[keep])


class SkySession:
    """What the sampled-sky session of a seed runs on: geoms (opened for the seeds of SKY_OPENED), materials (exponents drawn,
    emittance 0 where lamps_off), cam, depth, texels, lamps_off, other (the next seed's map, set for iterations 6-7)."""


def sky_session(pt, seed, w, h):
    s = SkySession()
    geoms, mats, s.cam, depth = scene(pt, seed, w, h)
    f = features(seed, mats, depth)
    s.geoms = opened(geoms) if seed in SKY_OPENED else geoms
    s.depth = f.direct_depth
    s.texels, s.lamps_off = sky_of(pt, seed)
    s.materials = f.materials.copy()
    if s.lamps_off:
        s.materials["emittance"] = 0
    s.other = sky_of(pt, seed + 1)[0]
    return s


def sky_run(po, pt, seed, w, h, camera=False, last=7):
    """sky_model.Model with PT_GLOSSY on sky_session(): iterations 1-3 under the seed's map, 4-5 without a map (direct_model's
    session; the plain one where the lamps are off), 6-7 under the next seed's map.  (run, counts, session, light elements with
    the sky's)."""
    def make():
        import sky_model
        s = sky_session(pt, seed, w, h)
        plan = CameraPlan(seed, camera, last)
        m = sky_model.Model(po, s.geoms, s.materials, s.cam, s.depth, glossy=True, **plan.kw())
        m.set_environment(s.texels)
        elements = len(m.table)

        def after(it, m):
            if it == 3:
                m.set_environment(None)
            if it == 5:
                m.set_environment(s.other)
        run = _model_run(m, w * h, s.depth, plan.its(), after, direct=True, plan=plan)
        return run, {k: v for k, v in m.counts.items() if isinstance(v, int)}, s, elements
    return _cached(("sky", seed, w, h, camera, last), make)


class SmoothSession:
    """What the smooth session of a seed runs on: geoms (with the soup's primitive), materials (exponents drawn), cam, depth, tris,
    meshes, normals (normals_of), sky (features().sky)."""


def smooth_session(pt, seed, w, h):
    s = SmoothSession()
    geoms, mats, s.cam, s.depth = scene(pt, seed, w, h)
    f = features(seed, mats, s.depth)
    s.geoms, s.tris, s.meshes = mesh_of(pt, seed, geoms, len(mats))
    s.materials, s.sky = f.materials, f.sky
    s.normals = normals_of(pt, seed, s.tris)
    return s


def smooth_run(po, pt, seed, w, h, camera=False, last=7, keep=False):
    """smooth_model.Model with PT_GLOSSY on smooth_session(): iterations 1-3 with the normals, 4-5 without them (keep: with them),
    6-7 with them again.  (run, stats, session); stats: smooth_model.Model.stats."""
    def make():
        import smooth_model
        s = smooth_session(pt, seed, w, h)
        plan = CameraPlan(seed, camera, last)
        m = smooth_model.Model(po, s.geoms, s.materials, s.cam, s.depth, tris=s.tris, meshes=s.meshes, glossy=True, **plan.kw())
        m.set_vertex_normals(s.normals)
        m.set_environment(s.sky)

        def after(it, m):
            if it == 3 and not keep:
                m.set_vertex_normals(None)
            if it == 5:
                m.set_vertex_normals(s.normals)
        run = _model_run(m, w * h, s.depth, plan.its(), after, plan=plan)
        return run, dict(m.stats), s
    return _cached(("smooth", seed, w, h, camera, last, keep), make)


# the sessions that run under camera_features(); "moments" is the plain compacting one with PT_MOMENTS, the two smooth ones share a model
CAMERA_KINDS = ("plain compact", "plain non-compacting", "plain sorted", "moments", "sky + glossy", "textures + bumps",
                "direct + sky + glossy", "sampled sky", "smooth loop", "smooth hierarchy")


def camera_run(po, pt, kind, seed, w, h, camera=True, last=None):
    """The model's run of one of CAMERA_KINDS (last: shorter than the session's own sequence)."""
    kw = dict(camera=camera) if last is None else dict(camera=camera, last=last)
    if kind.startswith("plain") or kind == "moments":
        oflags = {"plain non-compacting": 0, "plain sorted": po.F_COMPACT | po.F_SORT}.get(kind, po.F_COMPACT)
        return plain_run(po, pt, seed, w, h, oflags, **kw)
    models = {"sky + glossy": glossy_run, "textures + bumps": textured_run, "direct + sky + glossy": direct_run, "sampled sky": sky_run}
    return models.get(kind, smooth_run)(po, pt, seed, w, h, **kw)[0]


def light_table_size(po, pt, seed, w, h):
    import direct_model as dm
    geoms, mats, _, _ = scene(pt, seed, w, h)
    return len(dm.light_elements(np.ascontiguousarray(geoms).view(po.GEOM_DT), mats.view(po.MATERIAL_DT)))


def first_hits(po, pt, seed, w, h, cam=None):
    """The oracle's G-buffer of the seed's scene under its own camera (or cam)."""
    def make():
        import atrous_model as am
        geoms, mats, c, depth = scene(pt, seed, w, h)
        return am.gbuffer_from_oracle(po, c if cam is None else cam, depth, np.ascontiguousarray(geoms).view(po.GEOM_DT))
    return _cached(("g", seed, w, h, None if cam is None else cam.tobytes()), make)


def filter_run(po, pt, seed, other, w, h):
    """The filters on the plain compacting session after two iterations: the G-buffer, pt_denoise at 1 and 5 levels, and three
    temporal calls -- under the seed's camera, after a move of MOVE, and under seed `other`'s perturbed camera (every time on two
    fresh iterations).  A dict: cams, g, images, denoise {levels: plane}, temporal [(result, Hc, Hn)], kept [share with history]."""
    def make():
        import atrous_model as am
        import temporal_model as tpm
        geoms, mats, cam, depth = scene(pt, seed, w, h)
        cams = [cam, moved(cam, MOVE), scene(pt, other, w, h)[2]]
        out = dict(cams=cams, g=[], images=[], denoise={}, temporal=[], kept=[])
        t = tpm.Temporal(w, h, mats)
        for k, c in enumerate(cams):
            g = first_hits(po, pt, seed, w, h, None if k == 0 else c)
            image = plain_run(po, pt, seed, w, h, po.F_COMPACT, None if k == 0 else c, last=9 if k == 0 else 2).images[2]
            out["g"].append(g)
            out["images"].append(image)
            if k == 0:
                for levels in (1, 5):
                    out["denoise"][levels] = am.denoise(image.reshape(h, w, 3), 2, g["normal"].reshape(h, w, 3), g["position"].reshape(h, w, 3),
                                                        levels, *SIGMAS).reshape(-1, 3)
            res = t.call(image, 2, c, g, 5, *SIGMAS)
            out["temporal"].append((res, t.hc.copy(), t.hn.copy()))
            out["kept"].append(float((t.hn > 0).mean()))
        return out
    return _cached(("filters", seed, other, w, h), make)


def albedo_run(po, pt, seed, w, h):
    """The textured session's albedo plane and the demodulating filter (3 levels) on its running sum after iteration 3."""
    def make():
        import albedo_model as alm
        geoms, mats, cam, depth = scene(pt, seed, w, h)
        run, _, f = textured_run(po, pt, seed, w, h)
        g = first_hits(po, pt, seed, w, h)
        A = alm.albedo(po, geoms, f.materials, f.textures, cam, depth)
        out = alm.denoise(run.images[3].reshape(h, w, 3), 3, A.reshape(h, w, 3), g["normal"].reshape(h, w, 3), g["position"].reshape(h, w, 3),
                          3, *SIGMAS).reshape(-1, 3)
        return A, out
    return _cached(("albedo", seed, w, h), make)


class FirstState:
    """What bounce 0 leaves of a seed's camera rays, per pixel and per 64-pixel tile: `kinds` ([pixels] indices into STATE_KINDS),
    `count` {kind: pixels}, `tiles` {"ended" | "mixed" | "live": tiles}, `inside`, `primitives`, `depth`."""


def first_state_facts(po, pt, seed, w, h):
    """The four kinds of the first-state record read from the oracle's bounce-0 snapshots of iterations
    1 and 2 -- the paths as its shade step and compaction leave them, put back in pixel order: a survivor whose direction has the
    same bits in both iterations carries a fixed direction, one whose direction differs drew it; a path that ended did so with a
    colour or with 0 (put_final's test).  The oracle runs at depth max(depth, 2): the record holds what a bounce 0 that is not
    the last one leaves, whatever the session's depth, and at depth 1 the oracle zeroes every colour that does not end on a light.
    A tile is 64 consecutive pixels (a last, shorter one included): "ended" when every pixel ends with colour 0 (the condition
    of the table's word), "live" when every pixel survives, "mixed" otherwise -- a tile whose pixels all end, some with a colour,
    is mixed: no word skips it."""
    def make():
        geoms, mats, cam, depth = scene(pt, seed, w, h)
        g = np.ascontiguousarray(geoms).view(po.GEOM_DT)
        after = []
        for it in (1, 2):
            ref = po.Tracer(g, mats.view(po.MATERIAL_DT), cam, max(depth, 2), flags=po.F_COMPACT, trig=po.TRIG_SHARED)
            snaps = []
            ref.iterate(it, snapshots=snaps)
            p = snaps[0]["paths"]
            assert snaps[0]["depth"] == 0 and len(p) == w * h
            by_pixel = np.empty_like(p)
            by_pixel[p["pixelIndex"]] = p
            after.append(by_pixel)
        a, b = after
        alive = a["remainingBounces"] > 0
        assert (alive == (b["remainingBounces"] > 0)).all()
        same = (np.ascontiguousarray(a["direction"]).view(np.uint32) == np.ascontiguousarray(b["direction"]).view(np.uint32)).all(axis=1)
        coloured = (a["color"] != 0).any(axis=1)
        f = FirstState()
        f.kinds = np.where(alive, np.where(same, 1, 0), np.where(coloured, 2, 3)).astype(np.int8)
        f.count = {k: int((f.kinds == i).sum()) for i, k in enumerate(STATE_KINDS)}
        f.tiles = {"ended": 0, "mixed": 0, "live": 0}
        for t0 in range(0, w * h, 64):
            k = f.kinds[t0:t0 + 64]
            f.tiles["ended" if (k == 3).all() else "live" if (k <= 1).all() else "mixed"] += 1
        f.inside = first_hit_facts(po, pt, seed, w, h)[1]
        f.primitives, f.depth = len(geoms), depth
        return f
    return _cached(("first state", seed, w, h), make)


def first_hit_facts(po, pt, seed, w, h):
    """(share of the frame's pixels that miss at bounce 0, whether some camera ray starts inside the primitive it hits)"""
    geoms, mats, cam, depth = scene(pt, seed, w, h)
    paths = po.generate_rays(cam, depth)
    isects, outside = po.compute_intersections(paths, np.ascontiguousarray(geoms).view(po.GEOM_DT))
    hit = isects["t"] > 0
    return float((~hit).mean()), bool((hit & (outside == 0)).any())
