// test_delay_mirror.cpp -- the delay calls of the C++ host mirror (foo-dsp-bfir_amd/host/brutefir_hip.hpp), used the way a
// plug-in would: whole-sample delays on the input side, the sub-sample stage on the output side, one run() per block of L
// frames.  Input and filters come from integer recurrences that tests/test_delay_gpu.py restates; the FNV-1a hash of the
// output bytes is printed for it.
// Build: g++ -std=c++17 tests/cpp/test_delay_mirror.cpp -Lfoo-dsp-bfir_amd/lib -lbfir_hip
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
    const int L = 256, B = 2, C = 2, taps = 500, nb = 10;
    std::vector<float> x((size_t)nb * L * C), y(x.size());
    for (size_t i = 0; i < x.size(); i++)
        x[i] = (float)((double)((((uint64_t)i * 2654435761ull) & 0xffffffffull) >> 8) / 16777216.0 - 0.5);
    std::vector<std::vector<float>> h(C, std::vector<float>(taps));
    std::vector<void *> ph(C);
    for (int c = 0; c < C; c++) {
        for (int n = 0; n < taps; n++) {
            const uint64_t k = ((uint64_t)(n + 1) * (uint64_t)(40503u * (unsigned)(c + 3))) & 0xffffu;
            h[c][n] = (float)(((double)k / 65536.0 - 0.5) / (64.0 * (1.0 + (double)n / 64.0)));
        }
        ph[c] = h[c].data();
    }

    double f[17];
    CHECK(brutefir::subdelay_filter(8, 0, 10, 9.0, 8, f) == 0 && f[8] == 1.0 && f[7] == 0.0, "subdelay 0 is a unit tap");
    CHECK(brutefir::subdelay_filter(8, 10, 10, 9.0, 8, f) == BFIR_ERR_ARG, "|subdelay| >= step_count is refused");

    brutefir filter(L, B, 4, C, BF_SAMPLE_FORMAT_FLOAT_LE, BF_SAMPLE_FORMAT_FLOAT_LE, 44100, false);
    CHECK(filter.create_error() == 0, "create: %s", bfir_strerror(filter.create_error()));
    CHECK(filter.set_coeff(ph.data(), C, taps, B, 1.0) == 0, "set_coeff");
    const int d_in[2] = {300, 17}, d_out[2] = {0, 40}, s_out[2] = {3, -4}, too_long[2] = {301, 0};
    int d[2], s[2];
    CHECK(filter.set_delay(BFIR_DELAY_INPUT, d_in, nullptr, C) == BFIR_ERR_STATE, "set_delay before delay_init");
    CHECK(filter.delay_init(BFIR_DELAY_INPUT, 300) == 0, "delay_init, whole samples");
    CHECK(filter.delay_init(BFIR_DELAY_OUTPUT, 40, 10, 8, 9.0) == 0, "delay_init with the sub-sample stage");
    CHECK(filter.delay_latency(BFIR_DELAY_INPUT) == 0 && filter.delay_latency(BFIR_DELAY_OUTPUT) == 8, "latency");
    CHECK(filter.set_delay(BFIR_DELAY_INPUT, too_long, nullptr, C) == BFIR_ERR_ARG, "a delay past max_delay is refused");
    CHECK(filter.set_delay(BFIR_DELAY_INPUT, d_in, s_out, C) == BFIR_ERR_ARG, "a subdelay without the stage is refused");
    CHECK(filter.set_delay(BFIR_DELAY_INPUT, d_in, nullptr, C) == 0, "set_delay, input");
    CHECK(filter.set_delay(BFIR_DELAY_OUTPUT, d_out, s_out, C) == 0, "set_delay, output");
    CHECK(filter.get_delay(BFIR_DELAY_OUTPUT, d, s, C) == 0 && d[0] == 0 && d[1] == 40 && s[0] == 3 && s[1] == -4, "get_delay");
    for (int t = 0; t < nb; t++)
        CHECK(filter.run(&x[(size_t)t * L * C], &y[(size_t)t * L * C]) == 0, "run block %d", t);
    uint64_t hash = 0xcbf29ce484222325ull;
    const unsigned char *p = (const unsigned char *)y.data();
    for (size_t i = 0; i < y.size() * sizeof(float); i++) hash = (hash ^ p[i]) * 0x100000001b3ull;
    printf("checksum %016llx\n", (unsigned long long)hash);
    if (g_fail == 0) printf("ALL OK\n");
    return g_fail == 0 ? 0 : 1;
}
