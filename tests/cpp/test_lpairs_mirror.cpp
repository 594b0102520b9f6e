// test_lpairs_mirror.cpp -- the pair-list coefficient updates of the C++ host mirror (foo-dsp-bfir_amd/host/brutefir_hip.hpp)
// on a multi-level mimo engine: 10 inputs -> 10 outputs at L = 256, levels 2 x 256 and 2 x 512.  Five blocks with the first
// set; column 4 replaced with set_coeff_matrix_levels_pairs; four blocks; then three pairs of column 1 -- one replaced, one
// shortened to the head level, one removed -- crossfaded over three blocks with set_coeff_matrix_levels_pairs_fade, and the
// rest of the twenty blocks.  Input and filters come from integer recurrences.  The last blocks, behind the fade and
// everything it left in the tail level's ring, are checked against the direct convolution with the final set in double
// precision.
// Build: g++ -std=c++17 tests/cpp/test_lpairs_mirror.cpp -Lfoo-dsp-bfir_amd/lib -lbfir_hip
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

static const int L = 256, NC = 10, D1 = 2 * L, cap = D1 + 2 * 2 * L, nb = 20;

// filter number f of the recurrence with `taps` taps (f < NC NC: the first set; above: the replacements)
static std::vector<float> make_filter(int f, int taps)
{
    std::vector<float> h((size_t)taps);
    for (int n = 0; n < taps; n++) {
        const uint64_t k = ((uint64_t)(n + 1) * (uint64_t)(40503u * (unsigned)(f + 3))) & 0xffffu;
        h[(size_t)n] = (float)(((double)k / 65536.0 - 0.5) / 64.0);
    }
    return h;
}

int main()
{
    std::vector<float> x((size_t)nb * L * NC), y((size_t)nb * L * NC);
    for (size_t i = 0; i < x.size(); i++)
        x[i] = (float)((double)((((uint64_t)i * 2654435761ull) & 0xffffffffull) >> 8) / 16777216.0 - 0.5);
    // the first set: every filter reaches the tail level, a few taps apart
    std::vector<std::vector<float>> h((size_t)NC * NC);
    std::vector<void *> ph((size_t)NC * NC);
    std::vector<int> len((size_t)NC * NC);
    for (int f = 0; f < NC * NC; f++) {
        h[(size_t)f] = make_filter(f, cap - f % 7);
        ph[(size_t)f] = h[(size_t)f].data(); len[(size_t)f] = (int)h[(size_t)f].size();
    }

    const brutefir::multi_level lv = {2, {2, 2}, {1, 2}};
    brutefir filter(L, lv, 4, brutefir::mimo_io{NC, NC}, BF_SAMPLE_FORMAT_FLOAT_LE, BF_SAMPLE_FORMAT_FLOAT_LE);
    CHECK(filter.create_error() == 0, "create: %s", bfir_strerror(filter.create_error()));
    int o1[1] = {0}, i1[1] = {0};
    CHECK(filter.set_coeff_matrix_levels_pairs(1, o1, i1, ph.data(), len.data(), 1.0) == BFIR_ERR_STATE, "nothing to patch yet");
    CHECK(filter.set_coeff_matrix_pairs(1, o1, i1, ph.data(), len[0], 2, 1.0) == BFIR_ERR_UNSUPPORTED, "the uniform kind's call");
    CHECK(filter.set_coeff_matrix_levels(ph.data(), len.data(), 1.0) == 0, "set_coeff_matrix_levels");
    CHECK(filter.run_blocks(&x[0], &y[0], 5) == 0, "first blocks");

    // column 4: every output's filter from input 4
    std::vector<void *> pcol((size_t)NC);
    std::vector<int> outs((size_t)NC), ins((size_t)NC, 4), lcol((size_t)NC);
    for (int o = 0; o < NC; o++) {
        h[(size_t)o * NC + 4] = make_filter(200 + o, cap - o);
        pcol[(size_t)o] = h[(size_t)o * NC + 4].data(); lcol[(size_t)o] = cap - o; outs[(size_t)o] = o;
    }
    CHECK(filter.set_coeff_matrix_levels_pairs(NC, outs.data(), ins.data(), pcol.data(), lcol.data(), 1.0) == 0,
          "set_coeff_matrix_levels_pairs");
    CHECK(filter.is_initialized(), "initialised");
    CHECK(filter.run_blocks(&x[(size_t)5 * L * NC], &y[(size_t)5 * L * NC], 4) == 0, "blocks on the patched set");

    // (0, 1) replaced, (7, 1) shortened to the head level, (3, 1) removed, over three blocks
    int fo[3] = {0, 7, 3}, fi[3] = {1, 1, 1};
    std::vector<float> n0 = make_filter(300, cap - 5), n7 = make_filter(307, D1 - 9);
    void *pf[3] = {n0.data(), n7.data(), nullptr};
    int lf[3] = {(int)n0.size(), (int)n7.size(), 0};
    CHECK(filter.set_coeff_matrix_levels_pairs_fade(3, fo, fi, pf, lf, 1.0, 3) == 0, "set_coeff_matrix_levels_pairs_fade");
    CHECK(filter.fade_remaining_levels() == 3, "three fading blocks ahead");
    CHECK(filter.set_coeff_matrix_levels_pairs_fade(3, fo, fi, pf, lf, 1.0, 3) == BFIR_ERR_STATE, "one fade at a time");
    CHECK(filter.set_coeff_matrix_levels_pairs(3, fo, fi, pf, lf, 1.0) == BFIR_ERR_STATE, "no plain list while a fade runs");
    h[0 * NC + 1] = n0; h[7 * NC + 1] = n7; ph[3 * NC + 1] = nullptr;
    CHECK(filter.run(&x[(size_t)9 * L * NC], &y[(size_t)9 * L * NC]) == 0, "one fading block");
    CHECK(filter.fade_remaining_levels() == 2, "two fading blocks ahead");
    CHECK(filter.run_blocks(&x[(size_t)10 * L * NC], &y[(size_t)10 * L * NC], nb - 10) == 0, "the rest");
    CHECK(filter.fade_remaining_levels() == 0, "the fade is over");

    // blocks 16 .. 19: the final set on the whole stream (the fade ended with block 11, r_max = 2)
    const int n0s = 16 * L;
    std::vector<double> want((size_t)(nb * L - n0s) * NC, 0.0);
    for (int o = 0; o < NC; o++)
        for (int i = 0; i < NC; i++) {
            if (!ph[(size_t)o * NC + i]) continue;
            const std::vector<float> &f = h[(size_t)o * NC + i];
            for (int n = n0s; n < nb * L; n++) {
                double acc = 0.0;
                for (int k = 0; k < (int)f.size() && k <= n; k++) acc += (double)f[(size_t)k] * (double)x[(size_t)(n - k) * NC + i];
                want[(size_t)(n - n0s) * NC + o] += acc;
            }
        }
    double ymax = 0.0, worst = 0.0;
    for (double v : want) ymax = std::fmax(ymax, std::fabs(v));
    CHECK(ymax > 0.1, "the output carries signal (max %g)", ymax);
    for (size_t n = 0; n < want.size(); n++) worst = std::fmax(worst, std::fabs((double)y[(size_t)n0s * NC + n] - want[n]) / ymax);
    CHECK(worst <= 1e-5, "worst error %g of the output's maximum", worst);
    printf("worst error %.3g of the output's maximum\n", worst);
    if (g_fail == 0) printf("ALL OK\n");
    return g_fail == 0 ? 0 : 1;
}
