// test_bankmix_mirror.cpp -- the bank mixes of the C++ host mirror (foo-dsp-bfir_amd/host/brutefir_hip.hpp) on a mimo engine,
// 10 inputs -> 10 outputs at L = 256: set_coeff_matrix_bank_mix, _bank_mix_fade, _pairs_bank_mix and _pairs_bank_mix_fade
// drive one engine, the C calls of the same names (bfir_engine_...) drive a second one through its handle.  Both hold the same
// bank of 24 filters, loaded in two calls with different partition counts.  After every change the two engines' filter
// stores (read_coeff_matrix, every pair and partition) and output bytes are compared.  One row is also checked against the
// definition: fl(fl(w0 h0) + fl(w1 h1)) of the two entries' spectra as bank_read gives them.
// Build: g++ -std=c++17 tests/cpp/test_bankmix_mirror.cpp -Lfoo-dsp-bfir_amd/lib -lbfir_hip
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

static const int L = 256, B = 2, NC = 10, taps = L + 100, nb = 12, NE = 24, T = 3;
static_assert(T <= BFIR_BANK_MIX_TERMS, "the terms of a call");

static std::vector<float> make_filter(int f)
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
    for (int f = 0; f < NE; f++) { h[(size_t)f] = make_filter(f); ph[(size_t)f] = h[(size_t)f].data(); }

    brutefir filter(L, B, 4, brutefir::mimo_io{NC, NC}, BF_SAMPLE_FORMAT_FLOAT_LE, BF_SAMPLE_FORMAT_FLOAT_LE);
    brutefir twin(L, B, 4, brutefir::mimo_io{NC, NC}, BF_SAMPLE_FORMAT_FLOAT_LE, BF_SAMPLE_FORMAT_FLOAT_LE);
    CHECK(filter.create_error() == 0 && twin.create_error() == 0, "create: %s", bfir_strerror(filter.create_error()));
    bfir_engine *te = twin.handle();

    // the bank of both: entries 0 .. 19 with B partitions, 20 .. 22 with one, 23 empty
    std::vector<int> ent((size_t)NC * NC * T);
    std::vector<double> wt((size_t)NC * NC * T);
    auto fill = [&](int n_rows, int rot) {
        for (int n = 0; n < n_rows; n++)
            for (int j = 0; j < T; j++) {
                ent[(size_t)(n * T + j)] = (7 * n + 5 * j + rot) % 23;
                wt[(size_t)(n * T + j)] = (j == 1 ? -1.0 : 1.0) * (0.25 + 0.125 * ((n + 3 * j + rot) % 7));
            }
    };
    fill(NC * NC, 0);
    ent[4] = -1;                                       // a term without an entry
    ent[11] = 23; wt[11] = 0.0;                        // a term of weight 0 may name the empty entry
    for (int j = 0; j < T; j++) ent[(size_t)(11 * T + j)] = -1;   // pair (1, 1): no path
    CHECK(filter.set_coeff_matrix_bank_mix(T, ent.data(), wt.data()) == BFIR_ERR_STATE, "no bank to take entries from");
    for (brutefir *f : {&filter, &twin}) {
        CHECK(f->bank_create(NE) == 0, "bank_create");
        CHECK(f->bank_load(0, 20, ph.data(), taps, B, 1.0) == 0, "bank_load of 20");
        CHECK(f->bank_load(20, 3, ph.data() + 20, taps, 1, 0.5) == 0, "bank_load of 3, one partition each");
    }
    CHECK(filter.set_coeff_matrix_bank_mix(0, ent.data(), wt.data()) == BFIR_ERR_ARG, "no terms");
    CHECK(filter.set_coeff_matrix_bank_mix(BFIR_BANK_MIX_TERMS + 1, ent.data(), wt.data()) == BFIR_ERR_ARG, "too many terms");
    CHECK(!filter.is_initialized(), "refusals set no filters");

    std::vector<float> s0((size_t)2 * L), s1((size_t)2 * L);
    auto stores = [&](const char *what) {
        for (int o = 0; o < NC; o++)
            for (int i = 0; i < NC; i++)
                for (int blk = 0; blk < B; blk++) {
                    CHECK(filter.read_coeff_matrix(o, i, blk, s0.data()) == 0 && twin.read_coeff_matrix(o, i, blk, s1.data()) == 0, "read");
                    if (memcmp(s0.data(), s1.data(), s0.size() * sizeof(float)) != 0) {
                        CHECK(false, "%s: pair (%d, %d), block %d: the stores differ", what, o, i, blk);
                        return;
                    }
                }
    };
    size_t at = 0;
    auto both = [&](int blocks, const char *what) {
        CHECK(filter.run_blocks(&x[at], &y[at], blocks) == 0 && twin.run_blocks(&x[at], &yt[at], blocks) == 0, "%s", what);
        CHECK(memcmp(&y[at], &yt[at], (size_t)blocks * L * NC * sizeof(float)) == 0, "%s: the twin's bytes", what);
        at += (size_t)blocks * L * NC;
    };

    // the first set
    CHECK(filter.set_coeff_matrix_bank_mix(T, ent.data(), wt.data()) == 0, "set_coeff_matrix_bank_mix");
    CHECK(bfir_engine_set_coeff_matrix_bank_mix(te, T, ent.data(), wt.data()) == 0, "twin: bfir_engine_set_coeff_matrix_bank_mix");
    CHECK(filter.is_initialized(), "initialised from the bank alone");
    stores("the first set");
    {   // pair (0, 2), row 2: three live terms of B partitions each, against the definition
        std::vector<float> e0((size_t)2 * L), e1((size_t)2 * L), e2((size_t)2 * L);
        const int r = 2;
        for (int blk = 0; blk < B; blk++) {
            CHECK(filter.bank_blocks(ent[r * T]) == B && filter.bank_blocks(ent[r * T + 1]) == B && filter.bank_blocks(ent[r * T + 2]) == B,
                  "row 2 names long entries");
            CHECK(filter.bank_read(ent[r * T], blk, e0.data()) == 0 && filter.bank_read(ent[r * T + 1], blk, e1.data()) == 0 &&
                      filter.bank_read(ent[r * T + 2], blk, e2.data()) == 0 && filter.read_coeff_matrix(0, 2, blk, s0.data()) == 0, "read");
            const float w0 = (float)wt[r * T], w1 = (float)wt[r * T + 1], w2 = (float)wt[r * T + 2];
            for (int n = 0; n < 2 * L; n++) {
                volatile float p0 = w0 * e0[(size_t)n], p1 = w1 * e1[(size_t)n], p2 = w2 * e2[(size_t)n];
                volatile float a = p0 + p1;
                s1[(size_t)n] = a + p2;
            }
            CHECK(memcmp(s0.data(), s1.data(), s0.size() * sizeof(float)) == 0, "row 2, block %d: products and sums rounded one by one", blk);
        }
        CHECK(filter.read_coeff_matrix(1, 1, 0, s0.data()) == 0, "read");
        bool zero = true;
        for (float v : s0) zero = zero && v == 0.0f;
        CHECK(zero, "a row without a live term is zeros");
    }
    both(3, "first blocks");

    // column 4 from other mixes
    std::vector<int> outs((size_t)NC), ins((size_t)NC, 4);
    for (int o = 0; o < NC; o++) outs[(size_t)o] = o;
    fill(NC, 3);
    CHECK(filter.set_coeff_matrix_pairs_bank_mix(NC, outs.data(), ins.data(), T, ent.data(), wt.data()) == 0, "set_coeff_matrix_pairs_bank_mix");
    CHECK(bfir_engine_set_coeff_matrix_pairs_bank_mix(te, NC, outs.data(), ins.data(), T, ent.data(), wt.data()) == 0,
          "twin: bfir_engine_set_coeff_matrix_pairs_bank_mix");
    stores("column 4 patched");
    both(2, "blocks on the patched set");

    // (0, 1) and (7, 1) replaced, (3, 1) removed, over three blocks
    int fo[3] = {0, 7, 3}, fi[3] = {1, 1, 1};
    fill(3, 5);
    for (int j = 0; j < T; j++) wt[(size_t)(2 * T + j)] = 0.0;
    CHECK(filter.set_coeff_matrix_pairs_bank_mix_fade(3, fo, fi, T, ent.data(), wt.data(), 3) == 0, "set_coeff_matrix_pairs_bank_mix_fade");
    CHECK(bfir_engine_set_coeff_matrix_pairs_bank_mix_fade(te, 3, fo, fi, T, ent.data(), wt.data(), 3) == 0,
          "twin: bfir_engine_set_coeff_matrix_pairs_bank_mix_fade");
    CHECK(filter.fade_remaining() == 3, "three fading blocks ahead");
    CHECK(filter.set_coeff_matrix_pairs_bank_mix_fade(3, fo, fi, T, ent.data(), wt.data(), 3) == BFIR_ERR_STATE, "one fade at a time");
    both(1, "one fading block");
    CHECK(filter.fade_remaining() == 2, "two fading blocks ahead");
    both(3, "the rest of the fade and a block behind it");
    stores("behind the pairs fade");

    // the whole matrix to other mixes, over two blocks
    fill(NC * NC, 11);
    CHECK(filter.set_coeff_matrix_bank_mix_fade(T, ent.data(), wt.data(), 2) == 0, "set_coeff_matrix_bank_mix_fade");
    CHECK(bfir_engine_set_coeff_matrix_bank_mix_fade(te, T, ent.data(), wt.data(), 2) == 0, "twin: bfir_engine_set_coeff_matrix_bank_mix_fade");
    both(1, "a fading block of the whole matrix");
    CHECK(filter.bank_destroy() == 0 && twin.bank_destroy() == 0, "bank_destroy");
    both(nb - 10, "the rest, without the bank");
    CHECK(filter.fade_remaining() == 0, "the fade is over");
    stores("behind the whole-matrix fade");

    double ymax = 0.0;
    for (float v : y) ymax = v > ymax ? v : (-v > ymax ? -v : ymax);
    CHECK(ymax > 0.1, "the output carries signal (max %g)", ymax);
    if (g_fail == 0) printf("ALL OK\n");
    return g_fail == 0 ? 0 : 1;
}
