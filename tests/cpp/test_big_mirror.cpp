// test_big_mirror.cpp -- the long-partition constructor of the C++ host mirror (foo-dsp-bfir_amd/host/brutefir_hip.hpp),
// used the way a plug-in would: one run() per block of L = 32768 frames.  Input and filters come from integer
// recurrences; a handful of output samples -- the first and last of a block, across block edges, in the ragged last
// partition's reach -- are checked against the direct sum in double precision.
// Build: g++ -std=c++17 tests/cpp/test_big_mirror.cpp -Lfoo-dsp-bfir_amd/lib -lbfir_hip
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
    const int L = 32768, B = 2, C = 2, taps = L + L / 2 + 17, nb = 4;
    std::vector<float> x((size_t)nb * L * C), y(x.size());
    for (size_t i = 0; i < x.size(); i++)
        x[i] = (float)((double)((((uint64_t)i * 2654435761ull) & 0xffffffffull) >> 8) / 16777216.0 - 0.5);
    std::vector<std::vector<float>> h(C, std::vector<float>(taps));
    std::vector<void *> ph(C);
    for (int c = 0; c < C; c++) {
        for (int n = 0; n < taps; n++) {
            const uint64_t k = ((uint64_t)(n + 1) * (uint64_t)(40503u * (unsigned)(c + 3))) & 0xffffu;
            h[c][n] = (float)(((double)k / 65536.0 - 0.5) / 256.0);
        }
        ph[c] = h[c].data();
    }

    {
        brutefir small(16384, brutefir::long_partitions{B}, 4, C, BF_SAMPLE_FORMAT_FLOAT_LE, BF_SAMPLE_FORMAT_FLOAT_LE, 44100, false);
        CHECK(small.create_error() == BFIR_ERR_UNSUPPORTED && !small.is_initialized(), "16384 is the uniform engine's");
    }
    brutefir filter(L, brutefir::long_partitions{B}, 4, C, BF_SAMPLE_FORMAT_FLOAT_LE, BF_SAMPLE_FORMAT_FLOAT_LE, 44100, false);
    CHECK(filter.create_error() == 0, "create: %s", bfir_strerror(filter.create_error()));
    CHECK(!filter.is_initialized(), "no coefficients yet");
    CHECK(filter.set_coeff(ph.data(), C, taps, B, 1.0) == 0, "set_coeff");
    CHECK(filter.is_initialized(), "initialised");
    for (int t = 0; t < nb; t++)
        CHECK(filter.run(&x[(size_t)t * L * C], &y[(size_t)t * L * C]) == 0, "run block %d", t);

    double ymax = 0.0;
    for (float v : y) ymax = std::fmax(ymax, std::fabs((double)v));
    CHECK(ymax > 0.1, "the output carries signal (max %g)", ymax);
    const int at[] = {0, 1, L - 1, L, L + 1, taps - 1, taps, 2 * L - 1, 2 * L, 3 * L + 12345, nb * L - 1};
    double worst = 0.0;
    for (int n : at)
        for (int c = 0; c < C; c++) {
            double want = 0.0;
            for (int k = 0; k < taps && k <= n; k++) want += (double)h[c][k] * (double)x[(size_t)(n - k) * C + c];
            const double err = std::fabs((double)y[(size_t)n * C + c] - want) / ymax;
            worst = std::fmax(worst, err);
            CHECK(err <= 1e-5, "sample %d of channel %d: %g against %g", n, c, (double)y[(size_t)n * C + c], want);
        }
    printf("worst error %.3g of the output's maximum\n", worst);
    if (g_fail == 0) printf("ALL OK\n");
    return g_fail == 0 ? 0 : 1;
}
