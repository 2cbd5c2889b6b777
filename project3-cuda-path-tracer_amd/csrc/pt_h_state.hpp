// pt_h_state.hpp -- the scene state of ONE context that is replaced between calls (namespace one): the environment map, the
// materials' cube textures and bump maps, the triangles' vertex normals, and their getters
// (one of the host-side headers of libptmi355.so, included by ptmi355.hip -- the only translation unit -- in dependency order)
#pragma once

namespace {

// `count` RGB texels as the device keeps them, the first `words` of {r, g, b, 0} each: 4 -- the float4 of a texture or of the
// environment map; 2 -- a bump map's {da, db}
void pack_texels(const float *rgb, size_t count, int words, float *dst) {
    for (size_t k = 0; k < count; ++k)
        for (int w = 0; w < words; ++w) dst[(size_t)words * k + (size_t)w] = w < 3 ? rgb[3 * k + (size_t)w] : 0.0f;
}
// ... as an array of its own, of at least one element (a probe uploads it whatever the count)
std::vector<float> packed_texels(const float *rgb, size_t count, int words) {
    std::vector<float> out(std::max<size_t>(count, 1) * (size_t)words, 0.0f);
    pack_texels(rgb, count, words, out.data());
    return out;
}
std::vector<float> rgb_quads(const float *texels, size_t count) { return packed_texels(texels, count, 4); }
std::vector<float> bump_pairs(const float *texels, size_t count) { return packed_texels(texels, count, 2); }

size_t cube_texels(int n) { return (size_t)6 * (size_t)n * (size_t)n; }

}  // namespace

namespace one {

// All of this is state the launches in flight read.  Before any of it is replaced the host waits for everything the session has
// enqueued, and the windows traced ahead are void, as after a camera change.  The accumulation buffer stays as it is.
// (A setter that left one stream out would free texels under a running k_bounce: every setter below calls this and nothing else.)
static int quiesce(void) {
    const int rc = la_discard(LA_HOST);
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(R.stream));
    for (int k = 0; k < OV_MAX_LANES; ++k) {                    // asynchronous batches on the lanes
        if (R.lane[k].stream) HIPCHK(hipStreamSynchronize(R.lane[k].stream));
        if (R.lane[k].la_stream) HIPCHK(hipStreamSynchronize(R.lane[k].la_stream));
    }
    if (R.la_gstream) HIPCHK(hipStreamSynchronize(R.la_gstream));
    if (R.copy_stream) HIPCHK(hipStreamSynchronize(R.copy_stream));
    R.ov_active = false;
    return PT_OK;
}

// ---- what the entry points share: their refusals, in the order every one of them checks ----
// a cube map handed in: n x n texels per face
static int cube_arg(const char *who, const float *texels, int n) {
    if (n < 0 || n > 1024) return fail(PT_ERR_INVALID, "%s: n = %d outside [0, 1024]", who, n);
    if (n > 0 && !texels) return fail(PT_ERR_INVALID, "%s: null texels with n = %d", who, n);
    return PT_OK;
}
// a material of a PT_TEXTURES session
static int material_arg(const char *who, int material) {
    if (!R.live) return fail(PT_ERR_INVALID, "%s: not initialised", who);
    if (!(R.flags & PT_TEXTURES)) return fail(PT_ERR_INVALID, "%s: the session was not initialised with PT_TEXTURES", who);
    if (material < 0 || material >= R.scene.nmats) return fail(PT_ERR_INVALID, "%s: material %d outside [0, %d)", who, material, R.scene.nmats);
    return PT_OK;
}

// Give back the cube map `keep` (n x n RGB texels per face, as it was set; n == 0: none) -- `noun` is what the message calls it
static int cube_get(const char *who, const char *noun, const float *keep, int kept_n, float *texels, int capacity_texels, int *n) {
    if (!n) return fail(PT_ERR_INVALID, "%s: null n", who);
    *n = kept_n;
    if (kept_n == 0) return PT_OK;
    const size_t count = cube_texels(kept_n);
    if (!texels || capacity_texels < 0 || (size_t)capacity_texels < count)
        return fail(PT_ERR_INVALID, "%s: room for %d texels, the %s has %zu", who, texels ? capacity_texels : 0, noun, count);
    memcpy(texels, keep, count * 12);
    return PT_OK;
}
template <class Texel> static int cube_get(const char *who, const char *noun, const CubeMaps<Texel> &c, int material, float *texels,
                                           int capacity_texels, int *n) {
    const int kept_n = c.n.empty() ? 0 : c.n[(size_t)material];
    return cube_get(who, noun, kept_n ? c.keep[(size_t)material].data() : nullptr, kept_n, texels, capacity_texels, n);
}

// Material `material` of the set `c` takes the map (texels, n) -- n == 0: it loses its map -- and the others keep theirs.  Every
// map's texels sit back to back in ONE device array, rebuilt per call (a host keeps a handful of maps and sets them once), so the
// offsets of the materials behind this one move with its size.  The new array is made before the old one is released: the session
// keeps its old set when the device has no room for the new one.  The table is uploaded also when no map is left.  `nouns`: what
// the message calls the set.
template <class Texel> static int cube_replace(CubeMaps<Texel> &c, const char *who, const char *nouns, int material, const float *texels, int n) {
    constexpr int words = (int)(sizeof(Texel) / sizeof(float));
    const size_t nmats = (size_t)R.scene.nmats;
    if (c.n.empty()) { c.n.assign(nmats, 0); c.keep.resize(nmats); }
    std::vector<int> cn = c.n;
    cn[(size_t)material] = n;
    std::vector<int2> tab(nmats);
    size_t total = 0;
    int count = 0;
    for (size_t m = 0; m < nmats; ++m) {
        tab[m] = make_int2((int)total, cn[m]);
        total += cube_texels(cn[m]);
        if (cn[m] > 0) ++count;
    }
    if (total > (size_t)0x7fffffff) return fail(PT_ERR_INVALID, "%s: %zu texels in all (at most 2^31 - 1)", who, total);
    Texel *d_new = nullptr;
    if (count > 0) {
        std::vector<float> packed(total * (size_t)words);
        for (size_t m = 0; m < nmats; ++m)
            pack_texels(m == (size_t)material ? texels : c.keep[m].data(), cube_texels(cn[m]), words, packed.data() + (size_t)tab[m].x * (size_t)words);
        if (hipMalloc((void **)&d_new, total * sizeof(Texel)) != hipSuccess) {
            (void)hipGetLastError();
            return fail(PT_ERR_NOMEM, "%s: %zu bytes of device memory for the session's %s", who, total * sizeof(Texel), nouns);
        }
        HIPCHK(hipMemcpy(d_new, packed.data(), total * sizeof(Texel), hipMemcpyHostToDevice));
    }
    if (!c.d_tab) HIPCHK(hipMalloc((void **)&c.d_tab, tab.size() * sizeof(int2)));
    HIPCHK(hipMemcpy(c.d_tab, tab.data(), tab.size() * sizeof(int2), hipMemcpyHostToDevice));
    if (c.d_texels) (void)hipFree(c.d_texels);
    c.d_texels = d_new;
    c.n = cn;
    if (n > 0) c.keep[(size_t)material].assign(texels, texels + cube_texels(n) * 3);
    else std::vector<float>().swap(c.keep[(size_t)material]);
    c.count = count;
    return PT_OK;
}

// ---- environment lighting (include/ptmi355.h) ----
// PT_DIRECT_SKY: the device's light table of a flagged session -- the lamps' records alone (texels ==
// nullptr, or a map that yields no element), or the lamps at half their probability, the sky's record and its two tables.
// The caller has synchronised the session: nothing in flight reads the old table.  The light count, and with it the number
// of bounces a batch runs, follows.
static int upload_sky_lights(const float *texels, int n) {
    std::vector<float> rows, cols, rec;
    int count = (int)(R.lamp_rec.size() / (size_t)ptlight::RECORD_WORDS);
    const std::vector<float> *src = &R.lamp_rec;
    if (texels && n > 0 && ptlight::sky_table(texels, n, rows, cols)) {
        count = ptlight::sky_records(R.lamp_rec, n, rows, cols, rec);
        src = &rec;
    }
    if (R.d_lights) { (void)hipFree(R.d_lights); R.d_lights = nullptr; }
    R.nlights = 0;
    if (count == 0) return PT_OK;
    if (hipMalloc((void **)&R.d_lights, src->size() * 4) != hipSuccess) {
        (void)hipGetLastError(); R.d_lights = nullptr;
        return fail(PT_ERR_NOMEM, "pt_set_environment: %zu bytes of device memory for the light table", src->size() * 4);
    }
    HIPCHK(hipMemcpy(R.d_lights, src->data(), src->size() * 4, hipMemcpyHostToDevice));
    R.nlights = count;
    return PT_OK;
}

// Unlike the setters below this one is NOT transactional, and any session takes it: the old map -- and in a sky_session() the
// sky's light element with it -- goes before the new one is allocated, so a call that fails leaves the session without a map.
int pt_set_environment(const float *texels, int n) {
    const char *who = "pt_set_environment";
    if (!R.live) return fail(PT_ERR_INVALID, "%s: not initialised", who);
    int rc = cube_arg(who, texels, n);
    if (!rc) rc = quiesce();
    if (rc) return rc;
    if (!texels) n = 0;
    R.env_n = 0;
    if (R.d_env) { (void)hipFree(R.d_env); R.d_env = nullptr; }
    R.env_keep.clear();
    if (sky_session()) {                                        // the element disappears with the map
        const int rc2 = upload_sky_lights(nullptr, 0);
        if (rc2) return rc2;
    }
    if (n == 0) return PT_OK;
    const size_t count = cube_texels(n);
    const std::vector<float> quad = rgb_quads(texels, count);
    if (hipMalloc((void **)&R.d_env, count * 16) != hipSuccess) {
        (void)hipGetLastError(); R.d_env = nullptr;
        return fail(PT_ERR_NOMEM, "%s: %zu bytes of device memory for a %d x %d x 6 map", who, count * 16, n, n);
    }
    HIPCHK(hipMemcpy(R.d_env, quad.data(), count * 16, hipMemcpyHostToDevice));
    R.env_keep.assign(texels, texels + count * 3);
    R.env_n = n;
    if (sky_session()) return upload_sky_lights(texels, n);
    return PT_OK;
}

int pt_get_environment(float *texels, int capacity_texels, int *n) {
    if (!R.live) return fail(PT_ERR_INVALID, "pt_get_environment: not initialised");
    return cube_get("pt_get_environment", "map", R.env_keep.data(), R.env_n, texels, capacity_texels, n);
}

// ---- texture mapping (include/ptmi355.h) ----
int pt_set_texture(int material, const float *texels, int n) {
    const char *who = "pt_set_texture";
    int rc = material_arg(who, material);
    if (!rc) rc = cube_arg(who, texels, n);
    if (!rc) rc = quiesce();
    if (rc) return rc;
    if (!texels) n = 0;
    // the albedo plane follows the table: stale unless this call leaves every texel as it was
    const int old_n = R.tex.n.empty() ? 0 : R.tex.n[(size_t)material];
    const bool same = old_n == n && (n == 0 || memcmp(R.tex.keep[(size_t)material].data(), texels, cube_texels(n) * 12) == 0);
    rc = cube_replace(R.tex, who, "textures", material, texels, n);
    if (rc) return rc;
    if (!same) R.alb_valid = false;
    return PT_OK;
}

int pt_get_texture(int material, float *texels, int capacity_texels, int *n) {
    const int rc = material_arg("pt_get_texture", material);
    return rc ? rc : cube_get("pt_get_texture", "texture", R.tex, material, texels, capacity_texels, n);
}

// ---- bump mapping (include/ptmi355.h): pt_set_texture's contract with a set of its own.  A texel keeps
// its first two floats {da, db}; the albedo plane reads no normal and stays valid ----
int pt_set_bump_map(int material, const float *texels, int n) {
    const char *who = "pt_set_bump_map";
    int rc = material_arg(who, material);
    if (!rc) rc = cube_arg(who, texels, n);
    if (!rc) rc = quiesce();
    if (rc) return rc;
    if (!texels) n = 0;
    rc = cube_replace(R.bump, who, "bump maps", material, texels, n);
    if (rc) return rc;
    if (!R.tex.d_tab) {             // no pt_set_texture yet: a session with a bump map alone launches the TEX forms, which read a texture table
        const std::vector<int2> none((size_t)R.scene.nmats, make_int2(0, 0));
        HIPCHK(hipMalloc((void **)&R.tex.d_tab, none.size() * sizeof(int2)));
        HIPCHK(hipMemcpy(R.tex.d_tab, none.data(), none.size() * sizeof(int2), hipMemcpyHostToDevice));
    }
    return PT_OK;
}

int pt_get_bump_map(int material, float *texels, int capacity_texels, int *n) {
    const int rc = material_arg("pt_get_bump_map", material);
    return rc ? rc : cube_get("pt_get_bump_map", "map", R.bump, material, texels, capacity_texels, n);
}

// ---- smooth shading of triangle meshes (include/ptmi355.h): one array -- nine floats per triangle, in the
// order of pt_scene_desc::triangles -- that the session keeps when the device has no room for the new one.  pt_gbuffer, pt_albedo and
// the filters keep the facet normal, so nothing of theirs goes stale ----
int pt_set_vertex_normals(const float *normals, int num_triangles) {
    if (!R.live) return fail(PT_ERR_INVALID, "pt_set_vertex_normals: not initialised");
    if (!(R.flags & PT_SMOOTH_NORMALS)) return fail(PT_ERR_INVALID, "pt_set_vertex_normals: the session was not initialised with PT_SMOOTH_NORMALS");
    if (num_triangles < 0) return fail(PT_ERR_INVALID, "pt_set_vertex_normals: num_triangles = %d", num_triangles);
    if (num_triangles > 0 && !normals) return fail(PT_ERR_INVALID, "pt_set_vertex_normals: null normals with num_triangles = %d", num_triangles);
    if (!normals) num_triangles = 0;
    if (num_triangles != 0 && num_triangles != R.desc.num_triangles)
        return fail(PT_ERR_INVALID, "pt_set_vertex_normals: %d triangles, the session has %d", num_triangles, R.desc.num_triangles);
    const int rc = quiesce();
    if (rc) return rc;
    const size_t words = (size_t)num_triangles * 9;
    // (PT_FAKE_SHADER ignores the flag: the normals are kept for pt_get_vertex_normals and no kernel reads them)
    float *d_new = nullptr;
    if (words > 0) {
        if (hipMalloc((void **)&d_new, words * 4) != hipSuccess) {
            (void)hipGetLastError();
            return fail(PT_ERR_NOMEM, "pt_set_vertex_normals: %zu bytes of device memory for the session's vertex normals", words * 4);
        }
        HIPCHK(hipMemcpy(d_new, normals, words * 4, hipMemcpyHostToDevice));
    }
    if (R.d_vnormals) (void)hipFree(R.d_vnormals);
    R.d_vnormals = d_new;
    if (words > 0) R.vn_keep.assign(normals, normals + words);
    else std::vector<float>().swap(R.vn_keep);
    return PT_OK;
}

int pt_get_vertex_normals(float *normals, int capacity_triangles, int *num_triangles) {
    if (!R.live) return fail(PT_ERR_INVALID, "pt_get_vertex_normals: not initialised");
    if (!(R.flags & PT_SMOOTH_NORMALS)) return fail(PT_ERR_INVALID, "pt_get_vertex_normals: the session was not initialised with PT_SMOOTH_NORMALS");
    if (!num_triangles) return fail(PT_ERR_INVALID, "pt_get_vertex_normals: null num_triangles");
    const size_t count = R.vn_keep.size() / 9;
    *num_triangles = (int)count;
    if (count == 0) return PT_OK;
    if (!normals || capacity_triangles < 0 || (size_t)capacity_triangles < count)
        return fail(PT_ERR_INVALID, "pt_get_vertex_normals: room for %d triangles, the session has %zu", normals ? capacity_triangles : 0, count);
    memcpy(normals, R.vn_keep.data(), count * 36);
    return PT_OK;
}

}  // namespace one
