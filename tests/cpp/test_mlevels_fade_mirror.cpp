// test_mlevels_fade_mirror.cpp -- set_coeff_matrix_levels_fade / fade_remaining_levels of the C++ host mirror
// (foo-dsp-bfir_amd/host/brutefir_hip.hpp), used the way a plug-in would: 2 inputs -> 3 outputs, one run() per block of L
// frames, a crossfade to a second filter matrix requested while audio is playing, the tail levels working in blocks of 4 L
// and 8 L behind the head.  Input and filters come from integer recurrences that tests/test_mlevels_fade_gpu.py restates;
// the FNV-1a hash of the output bytes is printed for it.
// Build: g++ -std=c++17 tests/cpp/test_mlevels_fade_mirror.cpp -Lfoo-dsp-bfir_amd/lib -lbfir_hip
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../foo-dsp-bfir_amd/host/brutefir_hip.hpp"

static int g_fail = 0;
#define CHECK(cond, ...)                                        \
    do {                                                        \
        if (!(cond)) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); g_fail++; } \
    } while (0)

int main()
{
    const int L = 512, NI = 2, NO = 3, P = NI * NO, nb = 48, t0 = 11, K = 10;
    const brutefir::multi_level lv{3, {4, 2, 2}, {1, 4, 2}};            // 512 x 4, 2048 x 2, 4096 x 2: D = 0, 2048, 6144; 14336 taps
    // h_{o,i} (row major), set 0 = old, set 1 = new: the sets differ in which pair has no path and in the level a filter ends on
    const int lengths[2][P] = {{11000, 1500, 5000, 0, 2049, 14336}, {1500, 14336, 0, 5000, 11000, 2049}};
    std::vector<float> x((size_t)nb * L * NI), y((size_t)nb * L * NO);
    for (size_t i = 0; i < x.size(); i++)
        x[i] = (float)((double)((((uint64_t)i * 2654435761ull) & 0xffffffffull) >> 8) / 16777216.0 - 0.5);
    std::vector<std::vector<float>> h(2 * P, std::vector<float>(14337));
    std::vector<void *> ph(2 * P);
    for (int set = 0; set < 2; set++)
        for (int p = 0; p < P; p++) {
            for (int n = 0; n < lengths[set][p]; n++) {
                const uint64_t k = ((uint64_t)(n + 1) * (uint64_t)(40503u * (unsigned)(p + 3 + 8 * set))) & 0xffffu;
                h[set * P + p][n] = (float)(((double)k / 65536.0 - 0.5) / (64.0 * (1.0 + (double)n / 64.0)));
            }
            ph[set * P + p] = lengths[set][p] ? h[set * P + p].data() : nullptr;
        }

    brutefir filter(L, lv, 4, brutefir::matrix_io{NI, NO}, BF_SAMPLE_FORMAT_FLOAT_LE, BF_SAMPLE_FORMAT_FLOAT_LE);
    CHECK(filter.create_error() == 0, "create: %s", bfir_strerror(filter.create_error()));
    CHECK(filter.set_coeff_matrix_levels_fade(ph.data() + P, lengths[1], 1.0, K) == BFIR_ERR_STATE, "no coefficients yet");
    CHECK(filter.set_coeff_matrix_levels(ph.data(), lengths[0], 1.0) == 0, "set_coeff_matrix_levels");
    CHECK(filter.fade_remaining_levels() == 0, "no fade yet");
    CHECK(filter.set_coeff_levels_fade(ph.data() + P, NI, 1500, 1.0, K) == BFIR_ERR_UNSUPPORTED, "the diagonal levels fade is refused");
    CHECK(filter.set_coeff_fade(ph.data() + P, NI, 1500, 4, 1.0, K) == BFIR_ERR_UNSUPPORTED, "the uniform fade is refused");
    for (int t = 0; t < nb; t++) {
        if (t == t0) {
            const float keep = h[P + 4][9000];
            h[P + 4][9000] = NAN;                                        // in the last level's part of h_{2,0}
            CHECK(filter.set_coeff_matrix_levels_fade(ph.data() + P, lengths[1], 1.0, K) == -2, "a NaN tap is -2");
            CHECK(filter.is_initialized() && filter.fade_remaining_levels() == 0, "... and the old filters stay");
            h[P + 4][9000] = keep;
            CHECK(filter.set_coeff_matrix_levels_fade(ph.data() + P, lengths[1], 1.0, K) == 0, "set_coeff_matrix_levels_fade");
            CHECK(filter.set_coeff_matrix_levels_fade(ph.data() + P, lengths[1], 1.0, K) == BFIR_ERR_STATE, "a fade is pending");
        }
        CHECK(filter.run(&x[(size_t)t * L * NI], &y[(size_t)t * L * NO]) == 0, "run block %d", t);
        const int left = t < t0 ? 0 : t0 + K - 1 - t;
        CHECK(filter.fade_remaining_levels() == (left > 0 ? left : 0), "fade_remaining_levels after block %d", t);
    }
    uint64_t hash = 0xcbf29ce484222325ull;
    const unsigned char *p = (const unsigned char *)y.data();
    for (size_t i = 0; i < y.size() * sizeof(float); i++) hash = (hash ^ p[i]) * 0x100000001b3ull;
    printf("checksum %016llx\n", (unsigned long long)hash);
    if (g_fail == 0) printf("ALL OK\n");
    return g_fail == 0 ? 0 : 1;
}
