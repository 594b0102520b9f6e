// test_lbank_mirror.cpp -- the coefficient bank of the C++ host mirror (foo-dsp-bfir_amd/host/brutefir_hip.hpp) on a
// multi-level mimo engine: 10 inputs -> 10 outputs at L = 256, levels 2 x 256 and 2 x 512, beside a twin that gets the same
// filters as host taps.  The bank holds 24 entries: 0 .. 19 reach the tail level, a few taps apart; 20 .. 22 end on the head
// level; 23 stays empty.  The first set comes from the bank (set_coeff_matrix_levels_bank); column 4 is replaced
// (set_coeff_matrix_levels_pairs_bank); three pairs of column 1 fade -- one replaced, one shortened to the head level, one
// removed (set_coeff_matrix_levels_pairs_bank_fade); then the whole matrix fades to a rotation of the bank
// (set_coeff_matrix_levels_bank_fade).  After every step the two engines' output bytes are compared, and levels_bank_read
// against the twin's read_coeff_matrix_levels.  Input and filters come from integer recurrences.
// Build: g++ -std=c++17 tests/cpp/test_lbank_mirror.cpp -Lfoo-dsp-bfir_amd/lib -lbfir_hip
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

static const int L = 256, NC = 10, D1 = 2 * L, cap = D1 + 2 * 2 * L, nb = 22, NE = 24;

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
    std::vector<float> x((size_t)nb * L * NC), y((size_t)nb * L * NC), yt((size_t)nb * L * NC);
    for (size_t i = 0; i < x.size(); i++)
        x[i] = (float)((double)((((uint64_t)i * 2654435761ull) & 0xffffffffull) >> 8) / 16777216.0 - 0.5);
    std::vector<std::vector<float>> h((size_t)NE);
    std::vector<void *> ph((size_t)NE);
    std::vector<int> len((size_t)NE);
    for (int f = 0; f < NE; f++) {
        h[(size_t)f] = make_filter(f, f < 20 ? cap - f % 7 : D1 - 9 * (f - 19));
        ph[(size_t)f] = h[(size_t)f].data(); len[(size_t)f] = (int)h[(size_t)f].size();
    }
    ph[23] = nullptr; len[23] = 0;

    const brutefir::multi_level lv = {2, {2, 2}, {1, 2}};
    brutefir filter(L, lv, 4, brutefir::mimo_io{NC, NC}, BF_SAMPLE_FORMAT_FLOAT_LE, BF_SAMPLE_FORMAT_FLOAT_LE);
    brutefir twin(L, lv, 4, brutefir::mimo_io{NC, NC}, BF_SAMPLE_FORMAT_FLOAT_LE, BF_SAMPLE_FORMAT_FLOAT_LE);
    CHECK(filter.create_error() == 0 && twin.create_error() == 0, "create: %s", bfir_strerror(filter.create_error()));

    std::vector<int> ent((size_t)NC * NC);
    for (int n = 0; n < NC * NC; n++) ent[(size_t)n] = (7 * n) % 20;
    CHECK(filter.levels_bank_entries() == 0, "no bank yet");
    CHECK(filter.bank_create(NE) == BFIR_ERR_UNSUPPORTED, "the uniform kinds' call");
    CHECK(filter.set_coeff_matrix_levels_bank(ent.data()) == BFIR_ERR_STATE, "no bank to take entries from");
    CHECK(filter.levels_bank_create(NE) == 0, "levels_bank_create");
    CHECK(filter.levels_bank_create(NE) == BFIR_ERR_STATE, "one bank per engine");
    CHECK(filter.levels_bank_entries() == NE && filter.levels_bank_length(0) == 0, "%d empty entries", NE);
    CHECK(filter.set_coeff_matrix_levels_bank(ent.data()) == BFIR_ERR_STATE, "the entries are empty");
    CHECK(filter.levels_bank_load(0, 20, ph.data(), len.data(), 1.0) == 0, "levels_bank_load of 20");
    CHECK(filter.levels_bank_load(20, 4, ph.data() + 20, len.data() + 20, 1.0) == 0, "levels_bank_load of 4, head level only");
    CHECK(filter.levels_bank_length(19) == len[19] && filter.levels_bank_blocks(19, 0) == 2 && filter.levels_bank_blocks(19, 1) == 2,
          "a long entry's counts");
    CHECK(filter.levels_bank_length(20) == len[20] && filter.levels_bank_blocks(20, 0) == 2 && filter.levels_bank_blocks(20, 1) == 0,
          "a short entry's counts");
    CHECK(filter.levels_bank_length(23) == 0 && filter.levels_bank_blocks(23, 0) == 0, "an entry loaded as null is empty");
    CHECK(!filter.is_initialized(), "a bank alone sets no filters");

    // the first set
    std::vector<void *> pm((size_t)NC * NC);
    std::vector<int> lm((size_t)NC * NC);
    auto taps_of = [&]() { for (int n = 0; n < NC * NC; n++) { const int en = ent[(size_t)n]; pm[(size_t)n] = en < 0 ? nullptr : ph[(size_t)en]; lm[(size_t)n] = en < 0 ? 0 : len[(size_t)en]; } };
    taps_of();
    CHECK(filter.set_coeff_matrix_levels_bank(ent.data()) == 0, "set_coeff_matrix_levels_bank");
    CHECK(filter.is_initialized(), "initialised from the bank alone");
    CHECK(twin.set_coeff_matrix_levels(pm.data(), lm.data(), 1.0) == 0, "twin: set_coeff_matrix_levels");
    for (int level = 0; level < 2; level++) {
        std::vector<float> s0((size_t)2 * L << level), s1((size_t)2 * L << level);
        for (int blk = 0; blk < 2; blk++) {
            CHECK(filter.levels_bank_read(ent[37], level, blk, s0.data()) == 0 &&
                  twin.read_coeff_matrix_levels(level, 3, 7, blk, s1.data()) == 0, "read");
            CHECK(memcmp(s0.data(), s1.data(), s0.size() * sizeof(float)) == 0, "entry %d, level %d, block %d: the twin's spectrum",
                  ent[37], level, blk);
        }
    }
    size_t at = 0;
    auto both = [&](int blocks, const char *what) {
        CHECK(filter.run_blocks(&x[at], &y[at], blocks) == 0 && twin.run_blocks(&x[at], &yt[at], blocks) == 0, "%s", what);
        CHECK(memcmp(&y[at], &yt[at], (size_t)blocks * L * NC * sizeof(float)) == 0, "%s: the twin's bytes", what);
        at += (size_t)blocks * L * NC;
    };
    both(5, "first blocks");

    // column 4 from entries 10 .. 19
    std::vector<int> outs((size_t)NC), ins((size_t)NC, 4), cent((size_t)NC), lcol((size_t)NC);
    std::vector<void *> pcol((size_t)NC);
    for (int o = 0; o < NC; o++) {
        outs[(size_t)o] = o; cent[(size_t)o] = 10 + o; pcol[(size_t)o] = ph[(size_t)(10 + o)]; lcol[(size_t)o] = len[(size_t)(10 + o)];
    }
    CHECK(filter.set_coeff_matrix_levels_pairs_bank(NC, outs.data(), ins.data(), cent.data()) == 0, "set_coeff_matrix_levels_pairs_bank");
    CHECK(twin.set_coeff_matrix_levels_pairs(NC, outs.data(), ins.data(), pcol.data(), lcol.data(), 1.0) == 0,
          "twin: set_coeff_matrix_levels_pairs");
    both(4, "blocks on the patched set");

    // (0, 1) replaced, (7, 1) shortened to the head level, (3, 1) removed, over three blocks
    int fo[3] = {0, 7, 3}, fi[3] = {1, 1, 1}, fe[3] = {5, 21, -1};
    void *pf[3] = {ph[5], ph[21], nullptr};
    int lf[3] = {len[5], len[21], 0};
    CHECK(filter.set_coeff_matrix_levels_pairs_bank_fade(3, fo, fi, fe, 3) == 0, "set_coeff_matrix_levels_pairs_bank_fade");
    CHECK(twin.set_coeff_matrix_levels_pairs_fade(3, fo, fi, pf, lf, 1.0, 3) == 0, "twin: set_coeff_matrix_levels_pairs_fade");
    CHECK(filter.fade_remaining_levels() == 3, "three fading blocks ahead");
    CHECK(filter.set_coeff_matrix_levels_pairs_bank_fade(3, fo, fi, fe, 3) == BFIR_ERR_STATE, "one fade at a time");
    CHECK(filter.set_coeff_matrix_levels_pairs_bank(3, fo, fi, fe) == BFIR_ERR_STATE, "no plain list while a fade runs");
    both(1, "one fading block");
    CHECK(filter.fade_remaining_levels() == 2, "two fading blocks ahead");
    both(5, "the rest of the fade and blocks behind it");

    // the whole matrix to a rotation of the bank, over two blocks
    for (int n = 0; n < NC * NC; n++) ent[(size_t)n] = (3 * n + 1) % 20;
    ent[11] = -1;
    taps_of();
    CHECK(filter.set_coeff_matrix_levels_bank_fade(ent.data(), 2) == 0, "set_coeff_matrix_levels_bank_fade");
    CHECK(twin.set_coeff_matrix_levels_fade(pm.data(), lm.data(), 1.0, 2) == 0, "twin: set_coeff_matrix_levels_fade");
    both(1, "a fading block of the whole matrix");
    CHECK(filter.levels_bank_destroy() == 0 && filter.levels_bank_entries() == 0, "levels_bank_destroy");
    both(nb - 16, "the rest, without the bank");
    CHECK(filter.fade_remaining_levels() == 0, "the fade is over");
    std::vector<float> s0((size_t)2 * L);
    CHECK(filter.levels_bank_read(0, 0, 0, s0.data()) == BFIR_ERR_STATE, "no bank to read");

    double ymax = 0.0;
    for (float v : y) ymax = v > ymax ? v : (-v > ymax ? -v : ymax);
    CHECK(ymax > 0.1, "the output carries signal (max %g)", ymax);
    if (g_fail == 0) printf("ALL OK\n");
    return g_fail == 0 ? 0 : 1;
}
