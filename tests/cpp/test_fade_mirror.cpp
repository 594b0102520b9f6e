// test_fade_mirror.cpp -- brutefir::set_coeff_fade / fade_remaining of the C++ host mirror
// (foo-dsp-bfir_amd/host/brutefir_hip.hpp), used the way a plug-in would: one run() per block, the filters
// changed between two blocks with a crossfade instead of a cut.  Input and filters come from integer
// recurrences that tests/test_fade_gpu.py restates; the FNV-1a hash of the output bytes is printed for it.
// Build: g++ -std=c++17 tests/cpp/test_fade_mirror.cpp -Lfoo-dsp-bfir_amd/lib -lbfir_hip
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../foo-dsp-bfir_amd/host/brutefir_hip.hpp"

static int g_fail = 0;
#define CHECK(cond, ...)                                        \
    do {                                                        \
        if (!(cond)) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); g_fail++; } \
    } while (0)

static std::vector<float> taps_of(int c, unsigned salt, int taps)
{
    std::vector<float> h(taps);
    for (int n = 0; n < taps; n++) {
        const uint64_t k = ((uint64_t)(n + 1) * (uint64_t)(40503u * (unsigned)(c + 3) + salt)) & 0xffffu;
        const double v = (double)k / 65536.0 - 0.5;
        h[n] = (float)(v / (8.0 * (1.0 + (double)n)));
    }
    return h;
}

int main()
{
    const int L = 1024, B = 2, C = 2, taps = 1500, t0 = 2, K = 3, nb = 8;
    std::vector<float> x((size_t)nb * L * C), y(x.size());
    for (size_t i = 0; i < x.size(); i++)
        x[i] = (float)((double)((((uint64_t)i * 2654435761ull) & 0xffffffffull) >> 8) / 16777216.0 - 0.5);
    std::vector<std::vector<float>> h_old, h_new;
    for (int c = 0; c < C; c++) { h_old.push_back(taps_of(c, 0, taps)); h_new.push_back(taps_of(c, 977, taps)); }
    std::vector<void *> po(C), pn(C);
    for (int c = 0; c < C; c++) { po[c] = h_old[c].data(); pn[c] = h_new[c].data(); }

    brutefir filter(L, B, 4, C, BF_SAMPLE_FORMAT_FLOAT_LE, BF_SAMPLE_FORMAT_FLOAT_LE, 44100, false);
    CHECK(filter.create_error() == 0, "create: %s", bfir_strerror(filter.create_error()));
    CHECK(filter.set_coeff_fade(pn.data(), C, taps, B, 1.0, K) == BFIR_ERR_STATE, "a fade needs a first set");
    CHECK(filter.set_coeff(po.data(), C, taps, B, 1.0) == 0, "set_coeff");
    CHECK(filter.fade_remaining() == 0, "no fade yet");
    for (int t = 0; t < nb; t++) {
        if (t == t0) {
            CHECK(filter.set_coeff_fade(pn.data(), C, taps, B, 1.0, K) == 0, "set_coeff_fade");
            CHECK(filter.fade_remaining() == K, "fade pending");
        }
        CHECK(filter.run(&x[(size_t)t * L * C], &y[(size_t)t * L * C]) == 0, "run block %d", t);
        const int want = t < t0 ? 0 : (t - t0 + 1 >= K ? 0 : K - (t - t0 + 1));
        CHECK(filter.fade_remaining() == want, "block %d: %d blocks remain, expected %d", t, filter.fade_remaining(), want);
    }
    uint64_t hash = 0xcbf29ce484222325ull;
    const unsigned char *p = (const unsigned char *)y.data();
    for (size_t i = 0; i < y.size() * sizeof(float); i++) hash = (hash ^ p[i]) * 0x100000001b3ull;
    printf("checksum %016llx\n", (unsigned long long)hash);
    if (g_fail == 0) printf("ALL OK\n");
    return g_fail == 0 ? 0 : 1;
}
