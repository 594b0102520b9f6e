// test_levels_mirror.cpp -- the multi-level constructor and set_coeff_levels of the C++ host mirror
// (foo-dsp-bfir_amd/host/brutefir_hip.hpp), used the way a plug-in would: one run() per block of L frames while the
// tail levels work in blocks of 4 L and 8 L behind it.  Input and filters come from integer recurrences that
// tests/test_levels_gpu.py restates; the FNV-1a hash of the output bytes is printed for it.
// Build: g++ -std=c++17 tests/cpp/test_levels_mirror.cpp -Lfoo-dsp-bfir_amd/lib -lbfir_hip
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
    const int L = 512, C = 2, taps = 11000, nb = 48;
    const brutefir::multi_level lv{3, {4, 2, 2}, {1, 4, 2}};            // 512 x 4, 2048 x 2, 4096 x 2: D = 0, 2048, 6144; 14336 taps
    std::vector<float> x((size_t)nb * L * C), y(x.size());
    for (size_t i = 0; i < x.size(); i++)
        x[i] = (float)((double)((((uint64_t)i * 2654435761ull) & 0xffffffffull) >> 8) / 16777216.0 - 0.5);
    std::vector<std::vector<float>> h(C, std::vector<float>(14337));
    std::vector<void *> ph(C);
    for (int c = 0; c < C; c++) {
        for (int n = 0; n < taps; n++) {
            const uint64_t k = ((uint64_t)(n + 1) * (uint64_t)(40503u * (unsigned)(c + 3))) & 0xffffu;
            h[c][n] = (float)(((double)k / 65536.0 - 0.5) / (64.0 * (1.0 + (double)n / 64.0)));
        }
        ph[c] = h[c].data();
    }

    {
        brutefir bad(L, brutefir::multi_level{3, {4, 1, 2}, {1, 4, 4}}, 4, C, BF_SAMPLE_FORMAT_FLOAT_LE, BF_SAMPLE_FORMAT_FLOAT_LE);
        CHECK(bad.create_error() == BFIR_ERR_ARG && !bad.is_initialized(), "D_2 < L_2 is refused");
        brutefir one(L, brutefir::multi_level{1, {4}, {1}}, 4, C, BF_SAMPLE_FORMAT_FLOAT_LE, BF_SAMPLE_FORMAT_FLOAT_LE);
        CHECK(one.create_error() == BFIR_ERR_ARG, "one level is refused");
    }
    brutefir filter(L, lv, 4, C, BF_SAMPLE_FORMAT_FLOAT_LE, BF_SAMPLE_FORMAT_FLOAT_LE);
    CHECK(filter.create_error() == 0, "create: %s", bfir_strerror(filter.create_error()));
    CHECK(!filter.is_initialized(), "no coefficients yet");
    CHECK(filter.set_coeff(ph.data(), C, taps, 4, 1.0) == BFIR_ERR_UNSUPPORTED, "the uniform set_coeff is refused");
    CHECK(filter.set_coeff(ph.data(), C, taps, 1.0) == BFIR_ERR_UNSUPPORTED, "the two-level set_coeff is refused");
    CHECK(filter.set_coeff_levels(ph.data(), C, 14337, 1.0) == BFIR_ERR_ARG, "more taps than the levels hold");
    CHECK(filter.set_coeff_levels(ph.data(), C, taps, 1.0) == 0, "set_coeff_levels");
    CHECK(filter.is_initialized(), "initialised");
    for (int t = 0; t < nb; t++)
        CHECK(filter.run(&x[(size_t)t * L * C], &y[(size_t)t * L * C]) == 0, "run block %d", t);
    uint64_t hash = 0xcbf29ce484222325ull;
    const unsigned char *p = (const unsigned char *)y.data();
    for (size_t i = 0; i < y.size() * sizeof(float); i++) hash = (hash ^ p[i]) * 0x100000001b3ull;
    printf("checksum %016llx\n", (unsigned long long)hash);
    if (g_fail == 0) printf("ALL OK\n");
    return g_fail == 0 ? 0 : 1;
}
