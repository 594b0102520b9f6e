// test_lbankmix_mirror.cpp -- the bank mixes of the C++ host mirror (foo-dsp-bfir_amd/host/brutefir_hip.hpp) on a multi-level
// mimo engine: 6 inputs -> 6 outputs at L = 256, levels 2 x 256 and 2 x 512, beside a twin that gets entries of its own bank
// through the calls without weights.  Both banks hold 24 entries: 0 .. 9 reach the tail level, 10 and 11 end on the head
// level, 12 .. 23 are the same taps loaded with scale 0.5.  Every mix of the program has an entry of the twin's bank whose
// bytes it must give: (e, 1) is e; (e, 0.5), (e, 0.5) is e (halving and adding the halves are exact); (e, 0.5) is 12 + e
// (a power of two commutes with every rounding of the transform); a dead term takes no part; a row without a live term is
// -1.  The four methods are called in turn -- set_coeff_matrix_levels_bank_mix, _pairs_bank_mix, _pairs_bank_mix_fade,
// _bank_mix_fade -- and after every step the two engines' output bytes are compared.  At the end one pair gets a mix of two
// DIFFERENT entries, 0.75 a + 0.25 b, and the twin the same sum formed on the host as taps: the outputs agree within 1e-5 of
// the largest output, the project's fp32 bound against a reference.  Input and filters come from integer recurrences.
// Build: g++ -std=c++17 tests/cpp/test_lbankmix_mirror.cpp -Lfoo-dsp-bfir_amd/lib -lbfir_hip
#include <cmath>
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

static const int L = 256, NC = 6, D1 = 2 * L, cap = D1 + 2 * 2 * L, nb = 24, NE = 24, T = 2;

static std::vector<float> make_filter(int f, int taps)
{
    std::vector<float> h((size_t)taps);
    for (int n = 0; n < taps; n++) {
        const uint64_t k = ((uint64_t)(n + 1) * (uint64_t)(40503u * (unsigned)(f + 3))) & 0xffffu;
        h[(size_t)n] = (float)(((double)k / 65536.0 - 0.5) / 64.0);
    }
    return h;
}

// the mix of row n that stands for entry `en` of the twin's bank (0 .. 11, 12 .. 23 at half scale, -1), two terms
static void terms_for(int n, int en, int *e2, double *w2)
{
    if (en < 0) { e2[0] = -1; w2[0] = 1.0; e2[1] = 3; w2[1] = 0.0; return; }          // no live term
    if (en >= 12) { e2[0] = en - 12; w2[0] = 0.5; e2[1] = -1; w2[1] = 2.0; return; }  // half, and a term without an entry
    if (n % 2) { e2[0] = en; w2[0] = 0.5; e2[1] = en; w2[1] = 0.5; return; }          // two halves
    e2[0] = 23; w2[0] = 0.0; e2[1] = en; w2[1] = 1.0;                                  // a dead term first, then weight 1
}

int main()
{
    std::vector<float> x((size_t)nb * L * NC), y((size_t)nb * L * NC), yt((size_t)nb * L * NC);
    for (size_t i = 0; i < x.size(); i++)
        x[i] = (float)((double)((((uint64_t)i * 2654435761ull) & 0xffffffffull) >> 8) / 16777216.0 - 0.5);
    std::vector<std::vector<float>> h((size_t)12);
    std::vector<void *> ph((size_t)12);
    std::vector<int> len((size_t)12);
    for (int f = 0; f < 12; f++) {
        h[(size_t)f] = make_filter(f, f < 10 ? cap - f % 7 : D1 - 9 * (f - 9));
        ph[(size_t)f] = h[(size_t)f].data(); len[(size_t)f] = (int)h[(size_t)f].size();
    }

    const brutefir::multi_level lv = {2, {2, 2}, {1, 2}};
    brutefir filter(L, lv, 4, brutefir::mimo_io{NC, NC}, BF_SAMPLE_FORMAT_FLOAT_LE, BF_SAMPLE_FORMAT_FLOAT_LE);
    brutefir twin(L, lv, 4, brutefir::mimo_io{NC, NC}, BF_SAMPLE_FORMAT_FLOAT_LE, BF_SAMPLE_FORMAT_FLOAT_LE);
    CHECK(filter.create_error() == 0 && twin.create_error() == 0, "create: %s", bfir_strerror(filter.create_error()));
    const int one = 0;
    const double w1 = 1.0;
    CHECK(filter.set_coeff_matrix_levels_bank_mix(1, &one, &w1) == BFIR_ERR_STATE, "no bank to take entries from");
    CHECK(filter.set_coeff_matrix_bank_mix(1, &one, &w1) == BFIR_ERR_UNSUPPORTED, "the uniform kinds' call");
    for (brutefir *b : {&filter, &twin}) {
        CHECK(b->levels_bank_create(NE) == 0, "levels_bank_create");
        CHECK(b->levels_bank_load(0, 12, ph.data(), len.data(), 1.0) == 0, "levels_bank_load at scale 1");
        CHECK(b->levels_bank_load(12, 12, ph.data(), len.data(), 0.5) == 0, "levels_bank_load at scale 0.5");
    }

    std::vector<int> ent((size_t)NC * NC), me((size_t)NC * NC * T);
    std::vector<double> mw((size_t)NC * NC * T);
    auto mixes_of = [&](const std::vector<int> &en) {
        for (size_t n = 0; n < en.size(); n++) terms_for((int)n, en[n], &me[n * T], &mw[n * T]);
    };
    size_t at = 0;
    auto both = [&](int blocks, const char *what) {
        CHECK(filter.run_blocks(&x[at], &y[at], blocks) == 0 && twin.run_blocks(&x[at], &yt[at], blocks) == 0, "%s", what);
        CHECK(memcmp(&y[at], &yt[at], (size_t)blocks * L * NC * sizeof(float)) == 0, "%s: the twin's bytes", what);
        at += (size_t)blocks * L * NC;
    };

    // the first set: entries at both scales, two pairs without a path
    for (int n = 0; n < NC * NC; n++) ent[(size_t)n] = (7 * n) % 10 + (n % 3 == 2 ? 12 : 0);
    ent[4] = -1; ent[15] = -1;
    mixes_of(ent);
    CHECK(filter.set_coeff_matrix_levels_bank_mix(T, me.data(), mw.data()) == 0, "set_coeff_matrix_levels_bank_mix");
    CHECK(filter.is_initialized(), "initialised from the bank alone");
    CHECK(twin.set_coeff_matrix_levels_bank(ent.data()) == 0, "twin: set_coeff_matrix_levels_bank");
    for (int level = 0; level < 2; level++) {
        std::vector<float> s0((size_t)2 * L << level), s1((size_t)2 * L << level);
        for (int blk = 0; blk < 2; blk++) {
            CHECK(filter.read_coeff_matrix_levels(level, 1, 2, blk, s0.data()) == 0 &&
                  twin.read_coeff_matrix_levels(level, 1, 2, blk, s1.data()) == 0, "read");
            CHECK(memcmp(s0.data(), s1.data(), s0.size() * sizeof(float)) == 0, "pair (1, 2), level %d, block %d: the twin's spectrum",
                  level, blk);
        }
    }
    both(5, "first blocks");

    // column 4: one shortened to the head level, one removed, the rest replaced
    std::vector<int> outs((size_t)NC), ins((size_t)NC, 4), cent((size_t)NC);
    for (int o = 0; o < NC; o++) { outs[(size_t)o] = o; cent[(size_t)o] = 14 + o; }
    cent[1] = 10; cent[3] = -1;
    mixes_of(cent);
    CHECK(filter.set_coeff_matrix_levels_pairs_bank_mix(NC, outs.data(), ins.data(), T, me.data(), mw.data()) == 0,
          "set_coeff_matrix_levels_pairs_bank_mix");
    CHECK(twin.set_coeff_matrix_levels_pairs_bank(NC, outs.data(), ins.data(), cent.data()) == 0, "twin: set_coeff_matrix_levels_pairs_bank");
    both(4, "blocks on the patched set");

    // (0, 1) replaced, (5, 1) shortened to the head level, (3, 1) removed, over three blocks
    int fo[3] = {0, 5, 3}, fi[3] = {1, 1, 1};
    const std::vector<int> fe = {5, 23, -1};
    mixes_of(fe);
    CHECK(filter.set_coeff_matrix_levels_pairs_bank_mix_fade(3, fo, fi, T, me.data(), mw.data(), 3) == 0,
          "set_coeff_matrix_levels_pairs_bank_mix_fade");
    CHECK(twin.set_coeff_matrix_levels_pairs_bank_fade(3, fo, fi, fe.data(), 3) == 0, "twin: set_coeff_matrix_levels_pairs_bank_fade");
    CHECK(filter.fade_remaining_levels() == 3, "three fading blocks ahead");
    CHECK(filter.set_coeff_matrix_levels_pairs_bank_mix_fade(3, fo, fi, T, me.data(), mw.data(), 3) == BFIR_ERR_STATE, "one fade at a time");
    CHECK(filter.set_coeff_matrix_levels_pairs_bank_mix(3, fo, fi, T, me.data(), mw.data()) == BFIR_ERR_STATE,
          "no plain list while a fade runs");
    both(1, "one fading block");
    CHECK(filter.fade_remaining_levels() == 2, "two fading blocks ahead");
    both(5, "the rest of the fade and blocks behind it");

    // the whole matrix to a rotation of the bank, over two blocks
    for (int n = 0; n < NC * NC; n++) ent[(size_t)n] = (3 * n + 1) % 10 + (n % 4 == 1 ? 12 : 0);
    ent[11] = -1;
    mixes_of(ent);
    CHECK(filter.set_coeff_matrix_levels_bank_mix_fade(T, me.data(), mw.data(), 2) == 0, "set_coeff_matrix_levels_bank_mix_fade");
    CHECK(twin.set_coeff_matrix_levels_bank_fade(ent.data(), 2) == 0, "twin: set_coeff_matrix_levels_bank_fade");
    both(1, "a fading block of the whole matrix");
    both(4, "the rest of the fade and blocks behind it");
    CHECK(filter.fade_remaining_levels() == 0, "the fade is over");

    // a filter between two entries: 0.75 h_2 + 0.25 h_7 for the pair (2, 3); the twin gets the sum as taps
    const int po = 2, pi = 3, pe[2] = {2, 7};
    const double pw[2] = {0.75, 0.25};
    std::vector<float> sum((size_t)cap, 0.0f);
    for (int k = 0; k < 2; k++)
        for (int n = 0; n < len[(size_t)pe[k]]; n++) sum[(size_t)n] += (float)pw[k] * h[(size_t)pe[k]][(size_t)n];
    void *psum = sum.data();
    const int lsum = len[2] > len[7] ? len[2] : len[7];
    CHECK(filter.set_coeff_matrix_levels_pairs_bank_mix(1, &po, &pi, 2, pe, pw) == 0, "a mix of two entries");
    CHECK(twin.set_coeff_matrix_levels_pairs(1, &po, &pi, &psum, &lsum, 1.0) == 0, "twin: the sum as taps");
    const size_t from = at;
    const int rest = nb - (int)(at / ((size_t)L * NC));
    CHECK(filter.run_blocks(&x[at], &y[at], rest) == 0 && twin.run_blocks(&x[at], &yt[at], rest) == 0, "the last blocks");
    double ymax = 0.0, dmax = 0.0;
    for (size_t i = from; i < y.size(); i++) {
        ymax = std::fmax(ymax, std::fabs((double)yt[i]));
        dmax = std::fmax(dmax, std::fabs((double)y[i] - (double)yt[i]));
    }
    CHECK(ymax > 0.1, "the output carries signal (max %g)", ymax);
    CHECK(dmax <= 1e-5 * ymax, "the mix of two entries against the sum as taps: %g of %g", dmax, ymax);
    if (g_fail == 0) printf("ALL OK\n");
    return g_fail == 0 ? 0 : 1;
}
