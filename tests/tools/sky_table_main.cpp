// Stand-alone driver of the host code behind pt_sky_table (csrc/pt_lights.hpp: PT_DIRECT_SKY's sampling tables and the device's
// light table made from them), for a run under the sanitizers on the CPU:
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-omit-frame-pointer -Iinclude \
//       -o sky_table_main tests/tools/sky_table_main.cpp && ./sky_table_main
// Maps of 1, 2, 5, 64 and 256 texels a side, a sun 10^6 times the rest, black rows, black, NaN, infinite and negative texels,
// a null map; exits 0 when every invariant of DESIGN.md section 6.24 holds.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../../include/ptmi355.h"
#include "../../project3-cuda-path-tracer_amd/csrc/pt_lights.hpp"

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "sky_table_main: line %d: %s\n", __LINE__, #cond); return 1; } } while (0)

// a cdf of `len` pairs {cdf, inv}: increasing strictly, ending with 1, inv the reciprocal of the rounded difference
static int check_cdf(const float *pairs, size_t len) {
    double prev = 0.0;
    for (size_t k = 0; k < len; ++k) {
        const double c = pairs[2 * k];
        CHECK(c > prev && c <= 1.0);
        CHECK(pairs[2 * k + 1] == (float)(1.0 / (c - prev)) && std::isfinite(pairs[2 * k + 1]));
        prev = c;
    }
    CHECK(pairs[2 * (len - 1)] == 1.0f);
    return 0;
}

static int check_map(const std::vector<float> &tex, int n, bool expect) {
    std::vector<float> rows, cols;
    const bool have = ptlight::sky_table(tex.data(), n, rows, cols);
    CHECK(have == expect);
    if (!have) { CHECK(rows.empty() && cols.empty()); return 0; }
    const size_t nn = (size_t)n;
    CHECK(rows.size() == 2 * 6 * nn && cols.size() == 2 * 6 * nn * nn);
    if (check_cdf(rows.data(), 6 * nn)) return 1;
    for (size_t r = 0; r < 6 * nn; ++r)
        if (check_cdf(cols.data() + 2 * r * nn, nn)) return 1;
    // the device's table: with no lamp, and behind three lamps' records
    for (size_t E : {(size_t)0, (size_t)3}) {
        std::vector<float> lamps(E * (size_t)ptlight::RECORD_WORDS, 0.0f), rec;
        for (size_t e = 0; e < E; ++e) { lamps[e * ptlight::RECORD_WORDS + 3] = (float)(e + 1) / (float)E; lamps[e * ptlight::RECORD_WORDS + 4] = 3.0f; }
        const int count = ptlight::sky_records(lamps, n, rows, cols, rec);
        CHECK(count == (int)E + 1 && rec.size() == (E + 1) * (size_t)ptlight::RECORD_WORDS + rows.size() + cols.size());
        const float *s = rec.data() + E * (size_t)ptlight::RECORD_WORDS;
        int32_t kind, geom, side;
        memcpy(&kind, s, 4); memcpy(&geom, s + 1, 4); memcpy(&side, s + 7, 4);
        CHECK(kind == 2 && geom == -1 && side == n && s[3] == 1.0f && s[4] == (E ? 2.0f : 1.0f));
        CHECK(s[5] == (float)(4.0 / (ptlight::PI * n * n)) && s[6] == (float)(2.0 / n));
        for (size_t e = 0; e < E; ++e) CHECK(rec[e * ptlight::RECORD_WORDS + 3] == 0.5f * lamps[e * ptlight::RECORD_WORDS + 3] && rec[e * ptlight::RECORD_WORDS + 4] == 6.0f);
        CHECK(memcmp(s + ptlight::RECORD_WORDS, rows.data(), rows.size() * 4) == 0);
        CHECK(memcmp(s + ptlight::RECORD_WORDS + rows.size(), cols.data(), cols.size() * 4) == 0);
    }
    return 0;
}

int main() {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    uint32_t lcg = 12345u;
    auto next = [&]() { lcg = lcg * 1664525u + 1013904223u; return (float)(lcg >> 8) / 16777216.0f; };
    for (int n : {1, 2, 5, 64, 256}) {
        const size_t count = (size_t)6 * n * n;
        std::vector<float> tex(count * 3);
        for (float &v : tex) v = 0.1f + next();
        if (check_map(tex, n, true)) return 1;
        // a sun 10^6 times the rest, in one texel
        std::vector<float> sun(count * 3, 1.0f);
        sun[3 * (count / 3) + 0] = sun[3 * (count / 3) + 1] = sun[3 * (count / 3) + 2] = 1e6f;
        if (check_map(sun, n, true)) return 1;
        // everything black but one texel: black rows, and texels that do not count (NaN, infinite, negative)
        std::vector<float> one(count * 3, 0.0f);
        one[3 * (count - 1) + 1] = 2.0f;
        if (n > 1) { one[0] = nan; one[4] = inf; one[8] = -3.0f; }
        if (check_map(one, n, true)) return 1;
        // no element: black, NaN, negative, infinite
        for (float v : {0.0f, nan, -1.0f, inf}) {
            std::vector<float> none(count * 3, v);
            if (check_map(none, n, false)) return 1;
        }
    }
    std::vector<float> rows, cols;
    CHECK(!ptlight::sky_table(nullptr, 4, rows, cols) && !ptlight::sky_table(rows.data(), 0, rows, cols));
    printf("sky_table_main: ok\n");
    return 0;
}
