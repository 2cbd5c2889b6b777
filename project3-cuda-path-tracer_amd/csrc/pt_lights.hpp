// pt_lights.hpp -- host side (pt_init, pt_light_elements): the light element table of PT_DIRECT_LIGHT (DESIGN.md section 6.18;
// include/ptmi355.h has the specification).  Plain host C++ on the structs of include/ptmi355.h -- no HIP, no session -- so that
// it can be compiled into a stand-alone program (tests/tools/light_elements_main.cpp, under the sanitizers) as it is.
// Binary64 arithmetic on the binary32 entries of pt_geom::transform, in the order written, every stored value rounded once;
// tests/direct_model.py restates it in numpy operation for operation.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

namespace ptlight {

constexpr int MAX_ELEMENTS = 1024;
constexpr double PI = 3.14159265358979323846264338327950288;
constexpr int RECORD_WORDS = 56;            // ptd::LIGHT_WORDS (pt_device.hpp has the layout)

// determinant of the upper 3 x 3 of a column-major matrix (m[col][row]), cofactors of the first row
inline double det3(const pt_mat4 &M) {
    const double a = M.m[0][0], b = M.m[1][0], c = M.m[2][0];
    const double d = M.m[0][1], e = M.m[1][1], f = M.m[2][1];
    const double g = M.m[0][2], h = M.m[1][2], i = M.m[2][2];
    return (a * (e * i - f * h) - b * (d * i - f * g)) + c * (d * h - e * g);
}

inline bool usable(float area) { return std::isfinite(area) && area > 0.0f; }

// The elements of every PT_SPHERE / PT_CUBE whose material emits, in primitive order; -1: a material index outside the table.
inline int elements(const pt_geom *geoms, int num_geoms, const pt_material *materials, int num_materials, std::vector<pt_light_element> &out) {
    out.clear();
    for (int gi = 0; gi < num_geoms; ++gi) {
        const pt_geom &g = geoms[gi];
        if (g.type != PT_SPHERE && g.type != PT_CUBE) continue;
        if (g.materialid < 0 || g.materialid >= num_materials) return -1;
        if (!(materials[g.materialid].emittance > 0.0f)) continue;
        const pt_mat4 &M = g.transform;
        if (g.type == PT_SPHERE) {
            pt_light_element e;
            memset(&e, 0, sizeof e);
            e.geom = gi; e.kind = PT_SPHERE;
            e.area = (float)(PI * std::pow(std::fabs(det3(M)), 2.0 / 3.0));
            if (usable(e.area)) out.push_back(e);
            continue;
        }
        for (int axis = 0; axis < 3; ++axis)
            for (int neg = 0; neg < 2; ++neg) {
                const int a = axis == 0 ? 1 : 0, b = axis == 2 ? 1 : 2;        // the other two axes in x, y, z order
                double corner[3];
                corner[axis] = neg ? -0.5 : 0.5; corner[a] = -0.5; corner[b] = -0.5;
                double c0[3], ea[3], eb[3], out_dir[3];
                for (int r = 0; r < 3; ++r) {
                    c0[r] = (((double)M.m[0][r] * corner[0] + (double)M.m[1][r] * corner[1]) + (double)M.m[2][r] * corner[2]) + (double)M.m[3][r];
                    ea[r] = M.m[a][r]; eb[r] = M.m[b][r];
                    out_dir[r] = neg ? -(double)M.m[axis][r] : (double)M.m[axis][r];
                }
                const double n[3] = {ea[1] * eb[2] - ea[2] * eb[1], ea[2] * eb[0] - ea[0] * eb[2], ea[0] * eb[1] - ea[1] * eb[0]};
                const double area = std::sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
                double u[3] = {n[0] / area, n[1] / area, n[2] / area};
                if ((u[0] * out_dir[0] + u[1] * out_dir[1]) + u[2] * out_dir[2] < 0.0) { u[0] = -u[0]; u[1] = -u[1]; u[2] = -u[2]; }
                pt_light_element e;
                memset(&e, 0, sizeof e);
                e.geom = gi; e.kind = PT_CUBE;
                e.c0 = {(float)c0[0], (float)c0[1], (float)c0[2]};
                e.ea = {(float)ea[0], (float)ea[1], (float)ea[2]};
                e.eb = {(float)eb[0], (float)eb[1], (float)eb[2]};
                e.normal = {(float)u[0], (float)u[1], (float)u[2]};
                e.area = (float)area;
                if (usable(e.area)) out.push_back(e);
            }
    }
    double total = 0.0;
    for (const pt_light_element &e : out) total += (double)e.area;
    double run = 0.0;
    for (pt_light_element &e : out) {
        run += (double)e.area;
        e.cdf = (float)(run / total);
        e.inv_p = (float)(total / (double)e.area);
    }
    if (!out.empty()) out.back().cdf = 1.0f;
    return (int)out.size();
}

// the device's records (ptd::LIGHT_WORDS dwords each): the element, the sphere's Jacobian factor (float)(pi |det M3|) and the
// three matrices of its primitive, 4 columns x 3 rows as in the geom record
inline void records(const pt_geom *geoms, const std::vector<pt_light_element> &el, std::vector<float> &rec) {
    rec.assign(el.size() * (size_t)RECORD_WORDS, 0.0f);
    for (size_t k = 0; k < el.size(); ++k) {
        const pt_light_element &e = el[k];
        const pt_geom &g = geoms[e.geom];
        float *r = rec.data() + k * (size_t)RECORD_WORDS;
        const int32_t kind = e.kind == PT_SPHERE ? 0 : 1;
        memcpy(&r[0], &kind, 4); memcpy(&r[1], &e.geom, 4);
        r[2] = e.area; r[3] = e.cdf; r[4] = e.inv_p;
        r[5] = (float)(PI * std::fabs(det3(g.transform)));
        const pt_vec3 *v[4] = {&e.c0, &e.ea, &e.eb, &e.normal};
        for (int j = 0; j < 4; ++j) { r[6 + 3 * j] = v[j]->x; r[7 + 3 * j] = v[j]->y; r[8 + 3 * j] = v[j]->z; }
        const pt_mat4 *ms[3] = {&g.inverseTransform, &g.transform, &g.invTranspose};
        for (int m = 0; m < 3; ++m)
            for (int c = 0; c < 4; ++c)
                for (int rr = 0; rr < 3; ++rr) r[18 + 12 * m + c * 3 + rr] = ms[m]->m[c][rr];
    }
}

// ---- PT_DIRECT_SKY: the sampling tables of an environment map -----------------------------------
// Binary64 on the binary32 texels (6 n n RGB triples, pt_set_environment's layout), in the order written, every stored value
// rounded once; tests/sky_model.py restates it in numpy.  Row r = face * n + j, texel k = r * n + i.  `rows`: 6 n pairs
// {cdf, inv}, `cols`: 6 n n pairs, each row's own cdf.  false: the map yields no sky element (nothing is written then).
inline bool sky_table(const float *texels, int n, std::vector<float> &rows, std::vector<float> &cols) {
    if (!texels || n < 1) return false;
    const size_t nn = (size_t)n, R = 6 * nn, count = R * nn;
    std::vector<double> m(count), rowsum(R);
    std::vector<double> jac(nn * nn);
    for (size_t j = 0; j < nn; ++j)
        for (size_t i = 0; i < nn; ++i) {
            const double ac = (double)(2 * i + 1) / (double)n - 1.0, bc = (double)(2 * j + 1) / (double)n - 1.0;
            const double q = (1.0 + ac * ac) + bc * bc;
            jac[j * nn + i] = 1.0 / (q * std::sqrt(q));
        }
    double T = 0.0;
    for (size_t r = 0; r < R; ++r) {
        const size_t j = r % nn;
        double s = 0.0;
        for (size_t i = 0; i < nn; ++i) {
            const size_t k = r * nn + i;
            double lum = (0.2126 * (double)texels[3 * k] + 0.7152 * (double)texels[3 * k + 1]) + 0.0722 * (double)texels[3 * k + 2];
            if (!(std::isfinite(lum) && lum > 0.0)) lum = 0.0;
            m[k] = lum * jac[j * nn + i];
            s += m[k];
            T += m[k];
        }
        rowsum[r] = s;
    }
    if (!(std::isfinite(T) && T > 0.0)) return false;
    rows.assign(2 * R, 0.0f);
    cols.assign(2 * count, 0.0f);
    // a running sum over its total as binary32, the last forced to 1.0f; inv = the reciprocal of the probability the ROUNDED
    // table selects with
    auto emit = [](const double *mass, size_t len, float *out) {
        double total = 0.0;
        for (size_t k = 0; k < len; ++k) total += mass[k];
        double run = 0.0;
        for (size_t k = 0; k < len; ++k) {
            run += mass[k];
            out[2 * k] = (float)(run / total);
        }
        out[2 * (len - 1)] = 1.0f;
        double prev = 0.0;
        for (size_t k = 0; k < len; ++k) {
            out[2 * k + 1] = (float)(1.0 / ((double)out[2 * k] - prev));
            prev = (double)out[2 * k];
        }
    };
    std::vector<double> mass(R > nn ? R : nn);
    const double row_mix = T / (double)(16 * R);
    for (size_t r = 0; r < R; ++r) mass[r] = rowsum[r] + row_mix;
    emit(mass.data(), R, rows.data());
    for (size_t r = 0; r < R; ++r) {
        const double mix = rowsum[r] / (double)(16 * nn);
        for (size_t i = 0; i < nn; ++i) mass[i] = rowsum[r] == 0.0 ? 1.0 : m[r * nn + i] + mix;
        emit(mass.data(), nn, cols.data() + 2 * r * nn);
    }
    return true;
}

// The device's light table of a PT_DIRECT_SKY session: the lamps' records `lamps` (ptlight::records, E = lamps.size() /
// RECORD_WORDS) with cdf halved and inv_p doubled (exact), the sky's record -- kind 2, geom -1, cdf 1, inv_p 2 (1 when it is the
// only element), K = (float)(4 / (pi n n)) in word 5, s = (float)(2.0 / n) in word 6, n in word 7 -- and behind the E + 1
// records the row table and the column table.  Returns the element count, E + 1.
inline int sky_records(const std::vector<float> &lamps, int n, const std::vector<float> &rows, const std::vector<float> &cols, std::vector<float> &rec) {
    const size_t E = lamps.size() / (size_t)RECORD_WORDS;
    rec.assign((E + 1) * (size_t)RECORD_WORDS + rows.size() + cols.size(), 0.0f);
    if (!lamps.empty()) memcpy(rec.data(), lamps.data(), lamps.size() * 4);
    for (size_t e = 0; e < E; ++e) {
        rec[e * RECORD_WORDS + 3] *= 0.5f;
        rec[e * RECORD_WORDS + 4] *= 2.0f;
    }
    float *r = rec.data() + E * (size_t)RECORD_WORDS;
    const int32_t kind = 2, geom = -1, nn = n;
    memcpy(&r[0], &kind, 4); memcpy(&r[1], &geom, 4);
    r[3] = 1.0f; r[4] = E > 0 ? 2.0f : 1.0f;
    r[5] = (float)(4.0 / (PI * (double)n * (double)n));
    r[6] = (float)(2.0 / (double)n);
    memcpy(&r[7], &nn, 4);
    memcpy(r + RECORD_WORDS, rows.data(), rows.size() * 4);
    memcpy(r + RECORD_WORDS + rows.size(), cols.data(), cols.size() * 4);
    return (int)E + 1;
}

}  // namespace ptlight
