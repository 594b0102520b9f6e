// test_mimo_levels_mirror.cpp -- the multi-level mimo constructor of the C++ host mirror
// (foo-dsp-bfir_amd/host/brutefir_hip.hpp): 10 inputs -> 12 outputs at L = 64 on two levels (2 x 64, 2 x 128), one filter
// per pair of its own length -- some end in the head, some in the tail -- with one pair left without a path; the first blocks
// one run() each and the rest in one run_blocks().  The same filters and frames go through an engine made with the C ABI
// (bfir_engine_create_mimo_levels) and the two outputs are compared byte for byte.  Input and filters come from integer
// recurrences.
// Build: g++ -std=c++17 tests/cpp/test_mimo_levels_mirror.cpp -Lfoo-dsp-bfir_amd/lib -lbfir_hip
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../foo-dsp-bfir_amd/host/brutefir_hip.hpp"

static int g_fail = 0;
#define CHECK(cond, ...)                                        \
    do {                                                        \
        if (!(cond)) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); g_fail++; } \
    } while (0)

int main()
{
    const int L = 64, NI = 10, NO = 12, nb = 11;
    const brutefir::multi_level levels = {2, {2, 2}, {1, 2}};
    const int cap = 2 * L + 2 * 2 * L;   // D_2: the taps the two levels hold
    std::vector<float> x((size_t)nb * L * NI), y((size_t)nb * L * NO), y_c((size_t)nb * L * NO);
    for (size_t i = 0; i < x.size(); i++)
        x[i] = (float)((double)((((uint64_t)i * 2654435761ull) & 0xffffffffull) >> 8) / 16777216.0 - 0.5);
    std::vector<std::vector<float>> h((size_t)NO * NI);
    std::vector<void *> ph((size_t)NO * NI);
    std::vector<int> len((size_t)NO * NI);
    for (int f = 0; f < NO * NI; f++) {
        len[f] = f % 3 == 0 ? cap - 37 - f % 7 : f % 3 == 1 ? 2 * L - f % 5 : 2 * L + 3 + f % 11;   // tail | head only | just past D_1
        h[f].resize(len[f]);
        for (int n = 0; n < len[f]; n++) {
            const uint64_t k = ((uint64_t)(n + 1) * (uint64_t)(40503u * (unsigned)(f + 3))) & 0xffffu;
            h[f][n] = (float)(((double)k / 65536.0 - 0.5) / 64.0);
        }
        ph[f] = h[f].data();
    }
    ph[1 * NI + 7] = nullptr; len[1 * NI + 7] = 0;   // no path from input 7 to output 1

    {
        brutefir wide(L, levels, 4, brutefir::mimo_io{NI, BFIR_MIMO_MAXCHANNELS + 1}, BF_SAMPLE_FORMAT_FLOAT_LE, BF_SAMPLE_FORMAT_FLOAT_LE);
        CHECK(wide.create_error() == BFIR_ERR_ARG && !wide.is_initialized(), "65 outputs are past the limit");
    }
    brutefir filter(L, levels, 4, brutefir::mimo_io{NI, NO}, BF_SAMPLE_FORMAT_FLOAT_LE, BF_SAMPLE_FORMAT_FLOAT_LE);
    CHECK(filter.create_error() == 0, "create: %s", bfir_strerror(filter.create_error()));
    CHECK(!filter.is_initialized(), "no coefficients yet");
    CHECK(filter.delay_init(BFIR_DELAY_INPUT, 16) == BFIR_ERR_UNSUPPORTED, "no delays on a multi-level mimo engine");
    CHECK(filter.delay_init(BFIR_DELAY_OUTPUT, 16) == BFIR_ERR_UNSUPPORTED, "no delays on a multi-level mimo engine");
    CHECK(filter.set_coeff_matrix(ph.data(), cap, 2, 1.0) == BFIR_ERR_UNSUPPORTED, "the uniform call is another kind's");
    CHECK(filter.set_coeff_matrix_levels(ph.data(), len.data(), 1.0) == 0, "set_coeff_matrix_levels");
    CHECK(filter.is_initialized(), "initialised");
    for (int t = 0; t < 3; t++)
        CHECK(filter.run(&x[(size_t)t * L * NI], &y[(size_t)t * L * NO]) == 0, "run block %d", t);
    CHECK(filter.run_blocks(&x[(size_t)3 * L * NI], &y[(size_t)3 * L * NO], nb - 3) == 0, "run_blocks");

    int err = 0;
    bfir_engine *e = bfir_engine_create_mimo_levels(L, levels.n_levels, levels.blocks, levels.ratios, 4, NI, NO, BF_SAMPLE_FORMAT_FLOAT_LE,
                                                    BF_SAMPLE_FORMAT_FLOAT_LE, 0, &err);
    CHECK(e && err == 0, "C ABI create: %s", bfir_strerror(err));
    if (e) {
        CHECK(bfir_engine_set_coeff_matrix_levels(e, (const void *const *)ph.data(), len.data(), 1.0) == 0, "C ABI set");
        CHECK(bfir_engine_run(e, x.data(), y_c.data(), nb) == 0, "C ABI run");
        CHECK(memcmp(y.data(), y_c.data(), y.size() * sizeof(float)) == 0, "the mirror's bytes are the C ABI engine's");
        bfir_engine_destroy(e);
    }
    double ymax = 0.0;
    for (float v : y) ymax = v > ymax ? v : (-v > ymax ? -v : ymax);
    CHECK(ymax > 0.1, "the output carries signal (max %g)", ymax);
    filter.check_overflows();
    if (g_fail == 0) printf("ALL OK\n");
    return g_fail == 0 ? 0 : 1;
}
