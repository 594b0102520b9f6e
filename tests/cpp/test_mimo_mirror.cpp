// test_mimo_mirror.cpp -- the mimo constructor of the C++ host mirror (foo-dsp-bfir_amd/host/brutefir_hip.hpp): 12 inputs
// -> 3 outputs at L = 256, one filter per pair with one pair left without a path, the first blocks one run() each and the
// rest in one run_blocks().  Input and filters come from integer recurrences; every output sample is checked against the
// direct convolution in double precision, summed over the inputs.
// Build: g++ -std=c++17 tests/cpp/test_mimo_mirror.cpp -Lfoo-dsp-bfir_amd/lib -lbfir_hip
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
    const int L = 256, B = 2, NI = 12, NO = 3, taps = L + 100, nb = 5;
    std::vector<float> x((size_t)nb * L * NI), y((size_t)nb * L * NO);
    for (size_t i = 0; i < x.size(); i++)
        x[i] = (float)((double)((((uint64_t)i * 2654435761ull) & 0xffffffffull) >> 8) / 16777216.0 - 0.5);
    std::vector<std::vector<float>> h((size_t)NO * NI, std::vector<float>(taps));
    std::vector<void *> ph((size_t)NO * NI);
    for (int f = 0; f < NO * NI; f++) {
        for (int n = 0; n < taps; n++) {
            const uint64_t k = ((uint64_t)(n + 1) * (uint64_t)(40503u * (unsigned)(f + 3))) & 0xffffu;
            h[f][n] = (float)(((double)k / 65536.0 - 0.5) / 64.0);
        }
        ph[f] = h[f].data();
    }
    ph[1 * NI + 7] = nullptr;   // no path from input 7 to output 1

    {
        brutefir wide(L, B, 4, brutefir::mimo_io{BFIR_MIMO_MAXCHANNELS + 1, NO}, BF_SAMPLE_FORMAT_FLOAT_LE, BF_SAMPLE_FORMAT_FLOAT_LE);
        CHECK(wide.create_error() == BFIR_ERR_ARG && !wide.is_initialized(), "65 inputs are past the limit");
    }
    brutefir filter(L, B, 4, brutefir::mimo_io{NI, NO}, BF_SAMPLE_FORMAT_FLOAT_LE, BF_SAMPLE_FORMAT_FLOAT_LE);
    CHECK(filter.create_error() == 0, "create: %s", bfir_strerror(filter.create_error()));
    CHECK(!filter.is_initialized(), "no coefficients yet");
    CHECK(filter.delay_init(BFIR_DELAY_INPUT, 16) == BFIR_ERR_UNSUPPORTED, "no delays on a mimo engine");
    CHECK(filter.set_coeff(ph.data(), NI, taps, B, 1.0) == BFIR_ERR_UNSUPPORTED, "the diagonal call is another kind's");
    CHECK(filter.set_coeff_matrix(ph.data(), taps, B, 1.0) == 0, "set_coeff_matrix");
    CHECK(filter.is_initialized(), "initialised");
    for (int t = 0; t < 2; t++)
        CHECK(filter.run(&x[(size_t)t * L * NI], &y[(size_t)t * L * NO]) == 0, "run block %d", t);
    CHECK(filter.run_blocks(&x[(size_t)2 * L * NI], &y[(size_t)2 * L * NO], nb - 2) == 0, "run_blocks");

    std::vector<double> want((size_t)nb * L * NO, 0.0);
    double ymax = 0.0;
    for (int o = 0; o < NO; o++)
        for (int i = 0; i < NI; i++) {
            if (!ph[(size_t)o * NI + i]) continue;
            const std::vector<float> &f = h[(size_t)o * NI + i];
            for (int n = 0; n < nb * L; n++) {
                double acc = 0.0;
                for (int k = 0; k < taps && k <= n; k++) acc += (double)f[k] * (double)x[(size_t)(n - k) * NI + i];
                want[(size_t)n * NO + o] += acc;
            }
        }
    for (double v : want) ymax = std::fmax(ymax, std::fabs(v));
    CHECK(ymax > 0.1, "the output carries signal (max %g)", ymax);
    double worst = 0.0;
    for (size_t n = 0; n < want.size(); n++) worst = std::fmax(worst, std::fabs((double)y[n] - want[n]) / ymax);
    CHECK(worst <= 1e-5, "worst error %g of the output's maximum", worst);
    printf("worst error %.3g of the output's maximum\n", worst);
    filter.check_overflows();
    if (g_fail == 0) printf("ALL OK\n");
    return g_fail == 0 ? 0 : 1;
}
