// Stand-alone driver of the host code behind pt_smooth_normal (csrc/pt_smooth.hpp: steps 1-5 of DESIGN.md section 6.26), for a
// run under the sanitizers on the CPU:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-omit-frame-pointer -Iinclude \
//       -o smooth_main tests/tools/smooth_main.cpp && ./smooth_main
// Triangle and normal records of exactly nine words each (a read past either is the sanitizer's), rays aimed at vertices, edge
// midpoints and centroids, from the front, the back and in the plane; normals that are zero, NaN, infinite, tangential, facing
// away, and of length 1e-20 and 1e20.  Exits 0 when every invariant below holds.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../../project3-cuda-path-tracer_amd/csrc/pt_smooth.hpp"

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "smooth_main: line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    // v0, e1, e2 of three triangles: a unit right triangle in z = 0, a sliver, a metre-sized tilted one
    const float tris[3][9] = {{0, 0, 0, 1, 0, 0, 0, 1, 0}, {2, 1, -3, 1, 1e-4f, 0, 1.0001f, 0, 1e-6f}, {-40, 5, 7, 90, 3, -20, 10, 80, 15}};
    // what stands for one corner normal
    const float scales[] = {1.0f, 1e-20f, 1e20f, 0.0f, -1.0f};
    const float specials[] = {nan, inf, -inf};
    long smoothed = 0, refused = 0, records = 0;
    for (int k = 0; k < 3; ++k) {
        // exactly nine words each, on the heap
        std::vector<float> tv(tris[k], tris[k] + 9);
        const float *t = tv.data();
        const float cx = t[4] * t[8] - t[7] * t[5], cy = t[5] * t[6] - t[8] * t[3], cz = t[3] * t[7] - t[6] * t[4];
        const float il = 1.0f / std::sqrt((cx * cx + cy * cy) + cz * cz);
        const float nr[3] = {cx * il, cy * il, cz * il};
        // a tangent of the facet
        const float tl = 1.0f / std::sqrt((t[3] * t[3] + t[4] * t[4]) + t[5] * t[5]);
        const float tg[3] = {t[3] * tl, t[4] * tl, t[5] * tl};
        const float bary[7][2] = {{0, 0}, {1, 0}, {0, 1}, {0.5f, 0}, {0, 0.5f}, {0.5f, 0.5f}, {1.0f / 3, 1.0f / 3}};
        for (int b = 0; b < 7; ++b) {
            const float P[3] = {t[0] + bary[b][0] * t[3] + bary[b][1] * t[6], t[1] + bary[b][0] * t[4] + bary[b][1] * t[7],
                                t[2] + bary[b][0] * t[5] + bary[b][1] * t[8]};
            // origins: in front, behind, in the plane, at the point itself, far away, non-finite
            const float side[6] = {2.0f, -2.0f, 0.0f, 0.0f, 1e30f, nan};
            for (int s = 0; s < 6; ++s) {
                float o[3], I[3];
                for (int c = 0; c < 3; ++c) o[c] = P[c] + side[s] * nr[c] + (s == 2 ? 3.0f * tg[c] : 0.25f * tg[c]);
                float dl = 0;
                for (int c = 0; c < 3; ++c) { I[c] = P[c] - o[c]; dl += I[c] * I[c]; }
                dl = std::sqrt(dl);
                for (int c = 0; c < 3; ++c) I[c] = s == 3 ? -nr[c] : I[c] / dl;
                for (int form = 0; form < 5 + 3 + 2; ++form) {
                    std::vector<float> vn(9);
                    for (int j = 0; j < 3; ++j)
                        for (int c = 0; c < 3; ++c) {
                            float v = nr[c] + 0.3f * (float)(j - 1) * tg[c];            // leaning along the tangent, corner by corner
                            if (form < 5) v *= scales[form];
                            else if (form < 8) v = (j == form - 5 && c == 0) ? specials[form - 5] : v;
                            else if (form == 8) v = tg[c];                              // tangential
                            else v = (j == 0) ? 0.0f : v;                               // one zero corner
                            vn[(size_t)3 * j + c] = v;
                        }
                    float ns[3] = {7, 7, 7};
                    const bool hit = ptd::smooth_normal(tv.data(), vn.data(), o[0], o[1], o[2], I[0], I[1], I[2], nr[0], nr[1], nr[2], ns[0], ns[1], ns[2]);
                    ++records;
                    if (!hit) { CHECK(ns[0] == 7 && ns[1] == 7 && ns[2] == 7); ++refused; continue; }
                    ++smoothed;
                    const float len = std::sqrt(ns[0] * ns[0] + ns[1] * ns[1] + ns[2] * ns[2]);
                    CHECK(std::fabs(len - 1.0f) < 1e-5f);
                    CHECK(ns[0] * nr[0] + ns[1] * nr[1] + ns[2] * nr[2] > 0.0f);
                    CHECK(I[0] * ns[0] + I[1] * ns[1] + I[2] * ns[2] < 0.0f);
                    CHECK(form != 2 && form != 3 && form != 4);                         // overflow, zero, facing away: faceted
                }
            }
        }
    }
    CHECK(records == 3 * 7 * 6 * 10 && smoothed > 100 && refused > 100);
    printf("smooth_main: ok\n");
    return 0;
}
