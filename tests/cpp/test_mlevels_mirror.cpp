// test_mlevels_mirror.cpp -- the multi-level matrix constructor, set_coeff_matrix_levels and read_coeff_matrix_levels of the
// C++ host mirror (foo-dsp-bfir_amd/host/brutefir_hip.hpp), used the way a plug-in would: 2 inputs -> 3 outputs, one run()
// per block of L frames while the tail levels work in blocks of 4 L and 8 L behind it.  Input and filters come from
// integer recurrences that tests/test_mlevels_gpu.py restates; the FNV-1a hash of the output bytes is printed for it.
// Build: g++ -std=c++17 tests/cpp/test_mlevels_mirror.cpp -Lfoo-dsp-bfir_amd/lib -lbfir_hip
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
    const int L = 512, NI = 2, NO = 3, nb = 48;
    const brutefir::multi_level lv{3, {4, 2, 2}, {1, 4, 2}};            // 512 x 4, 2048 x 2, 4096 x 2: D = 0, 2048, 6144; 14336 taps
    // h_{o,i}: tap counts that end in level 2, 0, 1, -, 1, 2 (row major); (1, 1) has no path
    const int lengths[NO * NI] = {11000, 1500, 5000, 0, 2049, 14336};
    std::vector<float> x((size_t)nb * L * NI), y((size_t)nb * L * NO);
    for (size_t i = 0; i < x.size(); i++)
        x[i] = (float)((double)((((uint64_t)i * 2654435761ull) & 0xffffffffull) >> 8) / 16777216.0 - 0.5);
    std::vector<std::vector<float>> h(NO * NI, std::vector<float>(14337));
    std::vector<void *> ph(NO * NI);
    for (int p = 0; p < NO * NI; p++) {
        for (int n = 0; n < lengths[p]; n++) {
            const uint64_t k = ((uint64_t)(n + 1) * (uint64_t)(40503u * (unsigned)(p + 3))) & 0xffffu;
            h[p][n] = (float)(((double)k / 65536.0 - 0.5) / (64.0 * (1.0 + (double)n / 64.0)));
        }
        ph[p] = lengths[p] ? h[p].data() : nullptr;
    }

    {
        brutefir bad(L, brutefir::multi_level{3, {4, 1, 2}, {1, 4, 4}}, 4, brutefir::matrix_io{NI, NO}, BF_SAMPLE_FORMAT_FLOAT_LE,
                     BF_SAMPLE_FORMAT_FLOAT_LE);
        CHECK(bad.create_error() == BFIR_ERR_ARG && !bad.is_initialized(), "D_2 < L_2 is refused");
        brutefir wide(L, lv, 4, brutefir::matrix_io{NI, 9}, BF_SAMPLE_FORMAT_FLOAT_LE, BF_SAMPLE_FORMAT_FLOAT_LE);
        CHECK(wide.create_error() == BFIR_ERR_ARG, "nine outputs are refused");
    }
    brutefir filter(L, lv, 4, brutefir::matrix_io{NI, NO}, BF_SAMPLE_FORMAT_FLOAT_LE, BF_SAMPLE_FORMAT_FLOAT_LE);
    CHECK(filter.create_error() == 0, "create: %s", bfir_strerror(filter.create_error()));
    CHECK(!filter.is_initialized(), "no coefficients yet");
    CHECK(filter.set_coeff(ph.data(), NI, 1500, 4, 1.0) == BFIR_ERR_UNSUPPORTED, "the uniform set_coeff is refused");
    CHECK(filter.set_coeff(ph.data(), NI, 1500, 1.0) == BFIR_ERR_UNSUPPORTED, "the two-level set_coeff is refused");
    CHECK(filter.set_coeff_levels(ph.data(), NI, 1500, 1.0) == BFIR_ERR_UNSUPPORTED, "the diagonal levels set_coeff is refused");
    int too_long[NO * NI];
    for (int p = 0; p < NO * NI; p++) too_long[p] = lengths[p];
    too_long[5] = 14337;
    CHECK(filter.set_coeff_matrix_levels(ph.data(), too_long, 1.0) == BFIR_ERR_ARG, "more taps than the levels hold");
    CHECK(filter.set_coeff_matrix_levels(ph.data(), lengths, 1.0) == 0, "set_coeff_matrix_levels");
    CHECK(filter.is_initialized(), "initialised");
    CHECK(filter.fade_remaining_levels() == 0, "no fades on this kind");
    std::vector<float> spec(2 * 4096);
    CHECK(filter.read_coeff_matrix_levels(2, 2, 1, 1, spec.data()) == 0, "spectrum of level 2");
    CHECK(filter.read_coeff_matrix_levels(3, 0, 0, 0, spec.data()) == BFIR_ERR_ARG, "no level 3");
    for (int t = 0; t < nb; t++)
        CHECK(filter.run(&x[(size_t)t * L * NI], &y[(size_t)t * L * NO]) == 0, "run block %d", t);
    uint64_t hash = 0xcbf29ce484222325ull;
    const unsigned char *p = (const unsigned char *)y.data();
    for (size_t i = 0; i < y.size() * sizeof(float); i++) hash = (hash ^ p[i]) * 0x100000001b3ull;
    printf("checksum %016llx\n", (unsigned long long)hash);
    if (g_fail == 0) printf("ALL OK\n");
    return g_fail == 0 ? 0 : 1;
}
