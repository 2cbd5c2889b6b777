// Stand-alone driver of the host code behind pt_light_elements (csrc/pt_lights.hpp: PT_DIRECT_LIGHT's light element table and the
// device records made from it), for a run under the sanitizers on the CPU:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-omit-frame-pointer -Iinclude \
//       -o light_elements_main tests/tools/light_elements_main.cpp && ./light_elements_main
// Scaled, rotated, flat, singular, huge and non-finite primitives, empty scenes, a table past the limit; exits 0 when every
// invariant of DESIGN.md section 6.18 holds.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../../include/ptmi355.h"
#include "../../project3-cuda-path-tracer_amd/csrc/pt_lights.hpp"

static pt_geom make(int type, int material, double tx, double ty, double tz, double sx, double sy, double sz, double deg) {
    pt_geom g{};
    g.type = type; g.materialid = material;
    const double c = std::cos(deg * ptlight::PI / 180.0), s = std::sin(deg * ptlight::PI / 180.0);
    const double R[3][3] = {{c, -s, 0}, {s, c, 0}, {0, 0, 1}};        // about z
    const double S[3] = {sx, sy, sz};
    for (int col = 0; col < 3; ++col)
        for (int row = 0; row < 3; ++row) g.transform.m[col][row] = (float)(R[row][col] * S[col]);
    g.transform.m[3][0] = (float)tx; g.transform.m[3][1] = (float)ty; g.transform.m[3][2] = (float)tz; g.transform.m[3][3] = 1.0f;
    g.inverseTransform = g.transform; g.invTranspose = g.transform;    // (only copied into the records)
    return g;
}

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "light_elements_main: line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

static int check_table(const std::vector<pt_light_element> &el) {
    float prev = 0.0f;
    for (size_t k = 0; k < el.size(); ++k) {
        CHECK(std::isfinite(el[k].area) && el[k].area > 0.0f);
        CHECK(el[k].cdf >= prev && el[k].cdf <= 1.0f);
        CHECK(el[k].inv_p > 0.0f);
        prev = el[k].cdf;
    }
    if (!el.empty()) CHECK(el.back().cdf == 1.0f);
    return 0;
}

int main() {
    pt_material mats[3] = {};
    mats[0].emittance = 5.0f; mats[1].emittance = 0.0f; mats[2].emittance = std::numeric_limits<float>::quiet_NaN();
    std::vector<pt_geom> geoms = {
        make(PT_CUBE, 0, 0, 9, 0, 1.5, 0.3, 1.5, 35),          // six faces
        make(PT_CUBE, 1, 0, 0, 0, 10, 0.01, 10, 0),            // does not emit
        make(PT_SPHERE, 0, 2.5, 3, 1, 1.2, 0.8, 1.6, 40),      // one element
        make(PT_CUBE, 0, 1, 1, 1, 2, 0, 3, 10),                // flat: two faces
        make(PT_SPHERE, 0, 1, 1, 1, 0, 1, 1, 0),               // singular: none
        make(PT_CUBE, 0, 1, 1, 1, 1e30, 1e30, 1, 0),           // two faces whose area is no binary32 number: four
        make(PT_TRIANGLE_MESH, 0, 0, 0, 0, 1, 1, 1, 0),        // never an element
        make(PT_SPHERE, 2, 0, 0, 0, 1, 1, 1, 0),               // emittance NaN: not > 0
    };
    geoms.push_back(make(PT_CUBE, 0, 0, 0, 0, 1, 1, 1, 0));
    geoms.back().transform.m[0][0] = std::numeric_limits<float>::quiet_NaN();
    geoms.push_back(make(PT_SPHERE, 0, 0, 0, 0, 1, 1, 1, 0));
    geoms.back().transform.m[1][1] = std::numeric_limits<float>::infinity();
    std::vector<pt_light_element> el;
    int n = ptlight::elements(geoms.data(), (int)geoms.size(), mats, 3, el);
    CHECK(n == (int)el.size() && n == 6 + 1 + 2 + 4 + 2);
    if (check_table(el)) return 1;
    std::vector<float> rec;
    ptlight::records(geoms.data(), el, rec);
    CHECK(rec.size() == el.size() * (size_t)ptlight::RECORD_WORDS);
    // an empty scene, a scene without emitters, a null scene
    CHECK(ptlight::elements(nullptr, 0, mats, 3, el) == 0 && el.empty());
    CHECK(ptlight::elements(geoms.data() + 1, 1, mats, 3, el) == 0);
    ptlight::records(geoms.data(), el, rec);
    CHECK(rec.empty());
    // a material index outside the table
    pt_geom bad = geoms[0];
    bad.materialid = 3;
    CHECK(ptlight::elements(&bad, 1, mats, 3, el) == -1);
    bad.materialid = -1;
    CHECK(ptlight::elements(&bad, 1, mats, 3, el) == -1);
    // past the limit: the count is reported, the caller refuses
    std::vector<pt_geom> many(200, geoms[0]);
    n = ptlight::elements(many.data(), (int)many.size(), mats, 3, el);
    CHECK(n == 1200 && n > ptlight::MAX_ELEMENTS);
    if (check_table(el)) return 1;
    ptlight::records(many.data(), el, rec);
    CHECK(rec.size() == 1200u * (size_t)ptlight::RECORD_WORDS);
    // a uniform sphere: the nominal area is the area
    pt_geom ball = make(PT_SPHERE, 0, 0, 0, 0, 3, 3, 3, 25);
    CHECK(ptlight::elements(&ball, 1, mats, 3, el) == 1);
    CHECK(std::fabs(el[0].area - (float)(ptlight::PI * 9.0)) < 1e-4f && el[0].cdf == 1.0f && el[0].inv_p == 1.0f);
    printf("light_elements_main: ok\n");
    return 0;
}
