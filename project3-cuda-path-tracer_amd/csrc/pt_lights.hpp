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

}  // namespace ptlight
