// Stand-alone driver of the host code behind the scene format's STUDS line (host/pth_studs.h) and pt_bump_normal
// (csrc/pt_bump.hpp: steps 1-8 of DESIGN.md section 6.22), for a run under the sanitizers on the CPU:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-omit-frame-pointer -Iinclude \
//       -o bump_main tests/tools/bump_main.cpp && ./bump_main
// Maps of 1, 5 and 1024 texels a side, points on every face, edge and corner, far away, zero, infinite and NaN, non-finite texels
// and matrices; exits 0 when every texel read lies inside its map (the sanitizer's to say) and every invariant below holds.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../../project3-cuda-path-tracer_amd/csrc/pt_bump.hpp"
#include "../../project3-cuda-path-tracer_amd/host/pth_studs.h"

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "bump_main: line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

// the device's {da, db} pairs of RGB texels, exactly 6 n n of them: a read past the end is the sanitizer's
static std::vector<ptd::bump_texel> pairs(const std::vector<float> &rgb) {
    std::vector<ptd::bump_texel> p(rgb.size() / 3);
    for (size_t k = 0; k < p.size(); ++k) { p[k].da = rgb[3 * k]; p[k].db = rgb[3 * k + 1]; }
    return p;
}

// inverseTransform, transform, invTranspose of a scale (4 columns x 3 rows each)
static void record(float sx, float sy, float sz, float rec[36]) {
    for (int k = 0; k < 36; ++k) rec[k] = 0.0f;
    const float s[3] = {sx, sy, sz};
    for (int a = 0; a < 3; ++a) { rec[a * 3 + a] = 1.0f / s[a]; rec[12 + a * 3 + a] = s[a]; rec[24 + a * 3 + a] = 1.0f / s[a]; }
}

static int run(const std::vector<ptd::bump_texel> &B, int n, const float rec[36], const std::vector<float> &vals, long &perturbed) {
    const float dirs[4][3] = {{-1, 0, 0}, {0.3f, -0.8f, 0.5f}, {0, 0, 1}, {-0.6f, -0.6f, -0.5f}};
    for (uint32_t type = 0; type < 2; ++type)
        for (float x : vals) for (float y : vals) for (float z : vals)
            for (int d = 0; d < 4; ++d) {
                // the reported normal: the major axis of the point, either sign
                float nr[3] = {0, 0, 0};
                const float ax = std::fabs(x), ay = std::fabs(y), az = std::fabs(z);
                const int axis = (ax >= ay && ax >= az) ? 0 : ay >= az ? 1 : 2;
                nr[axis] = (d & 1) ? -1.0f : 1.0f;
                float ns[3] = {7, 7, 7};
                const bool hit = ptd::bump_normal(type, rec, x, y, z, dirs[d][0], dirs[d][1], dirs[d][2], nr[0], nr[1], nr[2], B.data(), n,
                                                  ns[0], ns[1], ns[2]);
                if (!hit) { CHECK(ns[0] == 7 && ns[1] == 7 && ns[2] == 7); continue; }
                ++perturbed;
                const float len = std::sqrt(ns[0] * ns[0] + ns[1] * ns[1] + ns[2] * ns[2]);
                CHECK(std::fabs(len - 1.0f) < 1e-5f);
                CHECK(ns[0] * nr[0] + ns[1] * nr[1] + ns[2] * nr[2] > 0.0f);
                CHECK(dirs[d][0] * ns[0] + dirs[d][1] * ns[1] + dirs[d][2] * ns[2] < 0.0f);
            }
    return 0;
}

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const std::vector<float> vals = {-inf, -1e30f, -3.0f, -0.5f, -0.49999997f, -0.2f, -1e-30f, -0.0f, 0.0f, 1e-38f, 0.1f, 0.5f, 0.50000006f, 40.0f, 1e30f, inf, nan};
    std::vector<float> rgb;
    long perturbed = 0;
    // STUDS: every value 0 or +-slope, the first quarter of a cell slopes down, the last up; the refusals
    for (int n : {1, 2, 5, 16, 1024})
        for (int cells : {1, 3, 1024}) {
            CHECK(pth_studs_texels(n, cells, 0.25f, rgb));
            CHECK(rgb.size() == (size_t)6 * n * n * 3);
            for (size_t k = 0; k < rgb.size(); k += 3) CHECK((rgb[k] == 0.0f || std::fabs(rgb[k]) == 0.25f) && (rgb[k + 1] == 0.0f || std::fabs(rgb[k + 1]) == 0.25f) && rgb[k + 2] == 0.0f);
            CHECK(rgb[0] == -0.25f && rgb[1] == -0.25f);
        }
    CHECK(pth_studs_texels(8, 1, 2.0f, rgb));
    {
        const float want[8] = {-2, -2, 0, 0, 0, 0, 2, 2};
        for (int i = 0; i < 8; ++i) CHECK(rgb[(size_t)i * 3] == want[i] && rgb[(size_t)i * 8 * 3 + 1] == want[i]);
    }
    CHECK(!pth_studs_texels(0, 1, 1.0f, rgb) && !pth_studs_texels(1025, 1, 1.0f, rgb) && !pth_studs_texels(4, 0, 1.0f, rgb) && !pth_studs_texels(4, 1025, 1.0f, rgb));
    // steps 1-8 on studs of every size, on a unit, a 100 : 1 and a non-finite primitive
    float unit[36], thin[36], bad[36];
    record(1, 1, 1, unit);
    record(1, 100, 0.01f, thin);
    record(1, 1, 1, bad);
    bad[0] = nan; bad[12 + 4] = inf; bad[24 + 8] = -inf;
    for (int n : {1, 5, 1024}) {
        CHECK(pth_studs_texels(n, n < 5 ? 1 : 4, 0.7f, rgb));
        const std::vector<ptd::bump_texel> B = pairs(rgb);
        if (run(B, n, unit, vals, perturbed) || run(B, n, thin, vals, perturbed) || run(B, n, bad, vals, perturbed)) return 1;
    }
    CHECK(perturbed > 1000);
    // non-finite and huge texels: never a normal that is not a unit vector
    {
        const int n = 3;
        std::vector<ptd::bump_texel> B((size_t)6 * n * n);
        const float t[6] = {nan, inf, -inf, 1e38f, -1e-45f, 0.0f};
        for (size_t k = 0; k < B.size(); ++k) { B[k].da = t[k % 6]; B[k].db = t[(k / 6) % 6]; }
        long some = 0;
        if (run(B, n, unit, vals, some) || run(B, n, thin, vals, some)) return 1;
    }
    printf("bump_main: ok\n");
    return 0;
}
