// The bump map of a `STUDS <n> <cells> <slope>` line of a BUMPMAP block (pthost.h), integer arithmetic only: for texel
// (face, j, i), pa = (i * cells * 4 / n) % 4 and sa = -1, 0, 0, 1 for pa = 0, 1, 2, 3; sb likewise from j; the texel is
// (slope * sa, slope * sb, 0).  Bevelled studs: every stored value is 0 or +-slope exactly.  A header of its own so that
// pthost.cpp and tests/tools/bump_main.cpp (the sanitizer driver) compile the same lines.
#pragma once
#include <cstddef>
#include <vector>

inline bool pth_studs_texels(int n, int cells, float slope, std::vector<float> &out) {
    if (n < 1 || n > 1024 || cells < 1 || cells > 1024) return false;
    out.assign((size_t)6 * n * n * 3, 0.0f);
    std::vector<float> side((size_t)n);
    for (int v = 0; v < n; ++v) {
        const int p = (v * cells * 4 / n) % 4;                   // (at most 1023 * 1024 * 4: no overflow)
        side[(size_t)v] = slope * (float)(p == 0 ? -1 : p == 3 ? 1 : 0);
    }
    for (int face = 0; face < 6; ++face)
        for (int j = 0; j < n; ++j)
            for (int i = 0; i < n; ++i) {
                float *o = out.data() + ((size_t)(face * n + j) * n + i) * 3;
                o[0] = side[(size_t)i]; o[1] = side[(size_t)j];
            }
    return true;
}
