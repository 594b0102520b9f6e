// test_level_mix_tables.cpp -- coeff_tables::level_mix_records (foo-dsp-bfir_amd/csrc/coeff_tables.h), the host arithmetic
// behind k_lbank_mix's records, on the host alone and against arrays written out by hand: dead and live terms and the order
// they are compacted in, the per-term per-level counts and their row maxima, weights that convert to 0 or to infinity as a
// float, every refusal and the order of the refusals, and a live term on an entry with taps but count 0 on a tail level.
// The header indexes vectors with numbers that come straight from a caller, so this program is built with the host
// sanitizers and run as it is:
// g++ -std=c++17 -Wall -Werror -fsanitize=address,undefined -fno-sanitize-recover=all tests/cpp/test_level_mix_tables.cpp
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../foo-dsp-bfir_amd/csrc/coeff_tables.h"

using namespace coeff_tables;
typedef std::vector<int> V;

static int g_fail = 0;
#define CHECK(cond, ...)                                        \
    do {                                                        \
        if (!(cond)) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); g_fail++; } \
    } while (0)

static unsigned fbits(float f) { unsigned u; memcpy(&u, &f, sizeof u); return u; }
static unsigned long long dbits(double d) { unsigned long long u; memcpy(&u, &d, sizeof u); return u; }

static_assert(BFIR_BANK_MIX_TERMS == 4 && BFIR_MAX_LEVELS == 4 && kLevelMixTerm == 7 && kLevelMixRec == 32,
              "the expected arrays below are written for four terms on four levels");

// a bank of four entries on a three-level engine: entry 0 reaches every level, entry 1 is empty, entry 2 ends on level 1,
// entry 3 has taps on the head alone
static const V LEN = {900, 0, 300, 40};
static const V NB = {2, 4, 3, 0, /* 1 */ 0, 0, 0, 0, /* 2 */ 2, 1, 0, 0, /* 3 */ 1, 0, 0, 0};
static const int NL = 3;

static int records(int s, const V *list, int n, int nt, const int *en, const double *w, V &rec, V &nb)
{
    return level_mix_records(LEN, NB, NL, s, list, n, nt, en, w, rec, nb);
}

static V term(int en, unsigned lo, unsigned hi) { return V({en, (int)lo, (int)hi, NB[4 * en], NB[4 * en + 1], NB[4 * en + 2], NB[4 * en + 3]}); }

static V record(int row, const std::vector<V> &terms)
{
    V r(kLevelMixRec, 0);
    r[0] = row; r[1] = (int)terms.size();
    for (size_t t = 0; t < terms.size(); t++) std::copy(terms[t].begin(), terms[t].end(), r.begin() + 2 + kLevelMixTerm * t);
    return r;
}

static V slice(const V &v, int j, int w) { return V(v.begin() + j * w, v.begin() + (j + 1) * w); }

static void test_records_and_counts()
{
    V rec, nb;
    // a dead term in the middle (no entry; a zero weight) is compacted away, the live ones keep the listed order
    const int en[] = {2, -1, 0, /* row 1 */ 0, 3, 2, /* row 2 */ -1, 1, 3};
    const double w[] = {0.5, 1.0, -2.0, /* row 1 */ 0.5, 0.0, -2.0, /* row 2 */ 3.0, 0.0, -0.0};
    const V list = {4, 1, 3};
    CHECK(records(4, &list, 3, 3, en, w, rec, nb) == BFIR_OK, "float");
    CHECK(rec.size() == (size_t)3 * kLevelMixRec && nb.size() == (size_t)3 * BFIR_MAX_LEVELS, "sizes");
    CHECK(slice(rec, 0, kLevelMixRec) == record(4, {term(2, fbits(0.5f), 0), term(0, fbits(-2.0f), 0)}), "row 0: entries 2, 0");
    CHECK(slice(rec, 1, kLevelMixRec) == record(1, {term(0, fbits(0.5f), 0), term(2, fbits(-2.0f), 0)}), "row 1: entries 0, 2");
    CHECK(slice(rec, 2, kLevelMixRec) == record(3, {}), "row 2: no live term, a dead one names the empty entry");
    // the row maxima: entry 0 is the longest on every level
    CHECK(slice(nb, 0, 4) == V({2, 4, 3, 0}) && slice(nb, 1, 4) == V({2, 4, 3, 0}) && slice(nb, 2, 4) == V({0, 0, 0, 0}), "row counts");
    // the whole store: row j; the weights as doubles, both words
    CHECK(records(8, nullptr, 3, 3, en, w, rec, nb) == BFIR_OK, "double");
    CHECK(slice(rec, 0, kLevelMixRec) == record(0, {term(2, (unsigned)dbits(0.5), (unsigned)(dbits(0.5) >> 32)),
                                                   term(0, (unsigned)dbits(-2.0), (unsigned)(dbits(-2.0) >> 32))}), "row 0 as doubles");
    CHECK(rec[kLevelMixRec] == 1 && rec[2 * kLevelMixRec] == 2, "the whole store: row j");
    // the maxima come from different terms on different levels, and a dead long entry does not count
    const int e2[] = {3, 2, 0};
    const double w2[] = {1.0, 1.0, 0.0};
    CHECK(records(4, nullptr, 1, 3, e2, w2, rec, nb) == BFIR_OK && rec[1] == 2 && nb == V({2, 1, 0, 0}), "the live terms' counts");
    CHECK(rec[2 + 3] == 1 && rec[2 + 4] == 0 && rec[2 + 7 + 3] == 2 && rec[2 + 7 + 4] == 1, "per term, per level");
    // a live term on an entry with taps but count 0 on a tail level: accepted, count 0 there
    const int e3[] = {3};
    const double w3[] = {-1.5};
    CHECK(records(4, nullptr, 1, 1, e3, w3, rec, nb) == BFIR_OK && rec[1] == 1 && nb == V({1, 0, 0, 0}), "head-only entry, live");
    CHECK(slice(rec, 0, kLevelMixRec) == record(0, {term(3, fbits(-1.5f), 0)}), "its record");
    // a level the engine does not have stays 0 whatever the host table holds there
    const int e0[] = {0};
    const double w1[] = {1.0};
    CHECK(level_mix_records(LEN, NB, 2, 4, nullptr, 1, 1, e0, w1, rec, nb) == BFIR_OK && nb == V({2, 4, 0, 0}) && rec[2 + 5] == 0,
          "two levels");
    // all four terms live: the last fills words 23 .. 29, words 30 and 31 stay 0
    const int e4[] = {2, 0, 3, 0};
    const double w4[] = {1.0, 2.0, 3.0, 4.0};
    CHECK(records(4, nullptr, 1, 4, e4, w4, rec, nb) == BFIR_OK && rec[1] == 4 && nb == V({2, 4, 3, 0}), "four terms");
    CHECK(rec[23] == 0 && rec[24] == (int)fbits(4.0f) && rec[26] == 2 && rec[28] == 3 && rec[30] == 0 && rec[31] == 0, "the last term");
    // no rows
    CHECK(records(4, nullptr, 0, 1, e0, w1, rec, nb) == BFIR_OK && rec.empty() && nb.empty(), "no rows");
}

static void test_weights()
{
    V rec, nb;
    const int e0[] = {0};
    const double big[] = {1e39}, tiny[] = {1e-60}, edge[] = {-3.5e38};
    CHECK(records(4, nullptr, 1, 1, e0, big, rec, nb) == BFIR_ERR_ARG, "1e39 in float");
    CHECK(records(4, nullptr, 1, 1, e0, edge, rec, nb) == BFIR_ERR_ARG, "-3.5e38 rounds past the largest float");
    CHECK(records(8, nullptr, 1, 1, e0, big, rec, nb) == BFIR_OK && rec[1] == 1, "1e39 in double");
    CHECK(records(4, nullptr, 1, 1, e0, tiny, rec, nb) == BFIR_OK && rec[1] == 0 && nb == V({0, 0, 0, 0}), "1e-60 in float is 0");
    CHECK(records(8, nullptr, 1, 1, e0, tiny, rec, nb) == BFIR_OK && rec[1] == 1 && nb == V({2, 4, 3, 0}), "1e-60 in double");
    // ... and so may name the empty entry as a float, not as a double
    const int e1[] = {1};
    CHECK(records(4, nullptr, 1, 1, e1, tiny, rec, nb) == BFIR_OK && rec[1] == 0, "1e-60 on the empty entry, float");
    CHECK(records(8, nullptr, 1, 1, e1, tiny, rec, nb) == BFIR_ERR_STATE, "1e-60 on the empty entry, double");
}

static void test_refusals_and_their_order()
{
    V rec, nb;
    const double nan[] = {std::numeric_limits<double>::quiet_NaN()}, inf[] = {-std::numeric_limits<double>::infinity()};
    const int e0[] = {0}, none[] = {-1};
    for (int s : {4, 8}) {
        CHECK(records(s, nullptr, 1, 1, e0, nan, rec, nb) == BFIR_ERR_ARG, "NaN, s = %d", s);
        CHECK(records(s, nullptr, 1, 1, e0, inf, rec, nb) == BFIR_ERR_ARG, "-Inf, s = %d", s);
        CHECK(records(s, nullptr, 1, 1, none, inf, rec, nb) == BFIR_ERR_ARG, "-Inf in a term without an entry, s = %d", s);
        // the empty entry: a zero weight may name it, a live term may not
        const int e1[] = {0, 1};
        const double zero[] = {1.0, 0.0}, live[] = {1.0, 0.25};
        CHECK(records(s, nullptr, 1, 2, e1, zero, rec, nb) == BFIR_OK && rec[1] == 1, "zero weight on the empty entry, s = %d", s);
        CHECK(records(s, nullptr, 1, 2, e1, live, rec, nb) == BFIR_ERR_STATE, "live term on the empty entry, s = %d", s);
        // an entry outside the bank is refused live or not ...
        const int out[] = {0, 4}, low[] = {0, -2};
        CHECK(records(s, nullptr, 1, 2, out, zero, rec, nb) == BFIR_ERR_ARG, "entry n_entries, weight 0, s = %d", s);
        CHECK(records(s, nullptr, 1, 2, low, zero, rec, nb) == BFIR_ERR_ARG, "entry -2, s = %d", s);
        // ... and before the state, wherever the two stand: in one row, and with the empty entry in an EARLIER row
        const int first[] = {1, 4};
        CHECK(records(s, nullptr, 1, 2, first, live, rec, nb) == BFIR_ERR_ARG, "behind a live empty one in the row, s = %d", s);
        const int rows[] = {1, 0, /* row 1 */ 0, 4};
        const double wr[] = {1.0, 1.0, 1.0, 0.0};
        CHECK(records(s, nullptr, 2, 2, rows, wr, rec, nb) == BFIR_ERR_ARG, "row 0: empty, row 1: outside, s = %d", s);
        const double wn[] = {1.0, 1.0, 1.0, std::numeric_limits<double>::quiet_NaN()};
        const int rows2[] = {1, 0, /* row 1 */ 0, 2};
        CHECK(records(s, nullptr, 2, 2, rows2, wn, rec, nb) == BFIR_ERR_ARG, "row 0: empty, row 1: a NaN weight, s = %d", s);
        CHECK(records(s, nullptr, 2, 2, rows2, wr, rec, nb) == BFIR_ERR_STATE, "row 0: empty, nothing else wrong, s = %d", s);
    }
    // "empty" is the length, not a count: entry 3 has count 0 on level 1 and is no empty entry
    const int e3[] = {3};
    const double w1[] = {1.0};
    CHECK(records(4, nullptr, 1, 1, e3, w1, rec, nb) == BFIR_OK, "count 0 on a tail level is not empty");
}

int main()
{
    test_records_and_counts();
    test_weights();
    test_refusals_and_their_order();
    if (g_fail) { printf("%d FAILED\n", g_fail); return 1; }
    printf("ALL OK\n");
    return 0;
}
