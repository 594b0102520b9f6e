// test_coeff_tables.cpp -- the table builders of foo-dsp-bfir_amd/csrc/coeff_tables.h on the host alone: the list check, the
// patch table, both gather tables and the mix records against arrays written out by hand.  The header indexes vectors with
// numbers that come straight from a caller, so this program is built with the host sanitizers and run as it is:
// g++ -std=c++17 -Wall -Werror -fsanitize=address,undefined -fno-sanitize-recover=all tests/cpp/test_coeff_tables.cpp
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

static const int NO = 2, NI = 3;   // a 3 -> 2 matrix: row o * 3 + i

static int rows_of(const V &outs, const V &ins, V &rows) { return list_rows(NO, NI, (int)outs.size(), outs.data(), ins.data(), rows); }

static void test_list_check()
{
    V rows;
    CHECK(rows_of({1, 0, 0}, {1, 2, 0}, rows) == BFIR_OK && rows == V({4, 2, 0}), "rows in list order");
    CHECK(rows_of({NO - 1}, {NI - 1}, rows) == BFIR_OK && rows == V({NO * NI - 1}), "the last pair");
    // each index at -1 and at its count
    CHECK(rows_of({-1}, {0}, rows) == BFIR_ERR_ARG, "output -1");
    CHECK(rows_of({NO}, {0}, rows) == BFIR_ERR_ARG, "output n_out");
    CHECK(rows_of({0}, {-1}, rows) == BFIR_ERR_ARG, "input -1");
    CHECK(rows_of({0}, {NI}, rows) == BFIR_ERR_ARG, "input n_in");
    CHECK(rows_of({0, 1, NO}, {0, 1, 0}, rows) == BFIR_ERR_ARG, "a bad pair behind good ones");
    // the same pair twice: at the first and the last position, at the first two, at the last two
    CHECK(rows_of({0, 1, 0}, {2, 1, 2}, rows) == BFIR_ERR_ARG, "first and last");
    CHECK(rows_of({0, 0, 1}, {2, 2, 1}, rows) == BFIR_ERR_ARG, "first two");
    CHECK(rows_of({1, 0, 0}, {1, 2, 2}, rows) == BFIR_ERR_ARG, "last two");
    CHECK(rows_of({0, 1}, {1, 0}, rows) == BFIR_OK && rows == V({1, 3}), "(0, 1) and (1, 0) are two pairs");
}

static void test_patch_table()
{
    V nb_new, nb_old;
    for (int r = 0; r < NO * NI; r++) { nb_new.push_back(10 + r); nb_old.push_back(20 + r); }
    const V want = {0, 2, 3, /* output 0 */ 0, 10, 20, 2, 12, 22, /* output 1 */ 1, 14, 24};
    V rows;
    CHECK(rows_of({0, 0, 1}, {0, 2, 1}, rows) == BFIR_OK, "in input order");
    CHECK(patch_table(NO, NI, rows, nb_new, nb_old) == want, "listed in input order");
    CHECK(rows_of({1, 0, 0}, {1, 2, 0}, rows) == BFIR_OK, "out of input order");
    CHECK(patch_table(NO, NI, rows, nb_new, nb_old) == want, "listed out of input order: the same table");
    // an output without a listed pair has an empty range, the first ...
    V tab = patch_table(NO, NI, V({5, 3}), nb_new, nb_old);
    CHECK(tab == V({0, 0, 2, 0, 13, 23, 2, 15, 25}), "output 0 has no pair");
    CHECK(tab[0] == tab[1] && tab[NO] == 2, "empty range; tab[Co] is the list length");
    // ... and the last
    tab = patch_table(NO, NI, V({1}), nb_new, nb_old);
    CHECK(tab == V({0, 1, 1, 1, 11, 21}), "output 1 has no pair");
    CHECK(tab[1] == tab[NO] && tab[NO] == 1, "empty range at the end");
    // the whole matrix listed
    tab = patch_table(NO, NI, V({5, 4, 3, 2, 1, 0}), nb_new, nb_old);
    CHECK(tab.size() == (size_t)(NO + 1 + 3 * NO * NI) && tab[0] == 0 && tab[1] == NI && tab[NO] == NO * NI, "every pair");
    for (int r = 0; r < NO * NI; r++)
        CHECK(tab[NO + 1 + 3 * r] == r % NI && tab[NO + 2 + 3 * r] == 10 + r && tab[NO + 3 + 3 * r] == 20 + r, "triple %d", r);
}

static void test_entries_and_gather_tables()
{
    const V bank_nb = {3, 0, 1};                                 // entry 1 is empty
    const int ok[] = {2, -1, 0}, low[] = {0, -2}, high[] = {0, 3}, empty[] = {2, 1}, both[] = {1, 3};
    V ent;
    CHECK(check_entries(bank_nb, 3, ok, ent) == BFIR_OK && ent == V({2, -1, 0}), "-1 is no path");
    CHECK(check_entries(bank_nb, 2, low, ent) == BFIR_ERR_ARG, "entry -2");
    CHECK(check_entries(bank_nb, 2, high, ent) == BFIR_ERR_ARG, "entry n_entries");
    CHECK(check_entries(bank_nb, 2, empty, ent) == BFIR_ERR_STATE, "an empty entry named");
    CHECK(check_entries(bank_nb, 2, both, ent) == BFIR_ERR_ARG, "the range comes before the state");
    CHECK(entry_count(bank_nb, -1) == 0 && entry_count(bank_nb, 0) == 3, "counts");
    // k_bank_gather's [rows][3], the whole store and a list
    CHECK(gather_table(nullptr, V({2, -1, 0}), bank_nb) == V({0, 2, 1, 1, -1, 0, 2, 0, 3}), "whole store");
    const V list = {5, 1, 3};
    CHECK(gather_table(&list, V({2, -1, 0}), bank_nb) == V({5, 2, 1, 1, -1, 0, 3, 0, 3}), "listed rows");
    CHECK(gather_table(nullptr, V(), bank_nb).empty(), "no rows");
    // k_lbank_gather's [rows][2 + BFIR_MAX_LEVELS]: entry 1 has no partitions on level 1, a -1 entry none anywhere
    static_assert(BFIR_MAX_LEVELS == 4 && kLevelRec == 6, "the expected arrays below are written for four levels");
    const V lbank_nb = {2, 1, 1, 0, /* entry 1 */ 1, 0, 3, 0};
    CHECK(level_gather_table(&list, V({1, -1, 0}), lbank_nb, 3) == V({5, 1, 1, 0, 3, 0, 1, -1, 0, 0, 0, 0, 3, 0, 2, 1, 1, 0}),
          "three levels, listed");
    // a level the engine does not have stays 0 whatever the host table holds there
    CHECK(level_gather_table(nullptr, V({1, 0}), lbank_nb, 2) == V({0, 1, 1, 0, 0, 0, 1, 0, 2, 1, 0, 0}), "two levels, whole store");
}

static unsigned fbits(float f) { unsigned u; memcpy(&u, &f, sizeof u); return u; }
static unsigned long long dbits(double d) { unsigned long long u; memcpy(&u, &d, sizeof u); return u; }

static void test_mix_records()
{
    const V bank_nb = {2, 0, 3};                                 // entry 1 is empty
    static_assert(BFIR_BANK_MIX_TERMS == 4 && kMixRec == 19, "the expected arrays below are written for four terms");
    V rec;
    // a dead term in the middle (no entry; a zero weight) is compacted away, in both precisions
    const int ent3[] = {0, -1, 2, /* row 1 */ 0, 2, 2};
    const double w3[] = {0.5, 1.0, -2.0, /* row 1 */ 0.5, 0.0, -2.0};
    const V list = {4, 1};
    CHECK(mix_records(bank_nb, 4, &list, 2, 3, ent3, w3, rec) == BFIR_OK, "float");
    for (int j = 0; j < 2; j++) {
        V want(kMixRec, 0);
        want[0] = list[j]; want[1] = 3; want[2] = 2;
        want[3] = 0; want[4] = 2; want[5] = (int)fbits(0.5f);
        want[7] = 2; want[8] = 3; want[9] = (int)fbits(-2.0f);
        CHECK(V(rec.begin() + j * kMixRec, rec.begin() + (j + 1) * kMixRec) == want, "float record %d", j);
    }
    CHECK(mix_records(bank_nb, 8, nullptr, 2, 3, ent3, w3, rec) == BFIR_OK, "double");
    CHECK(rec[0] == 0 && rec[kMixRec] == 1, "the whole store: row j");
    CHECK(rec[2] == 2 && rec[5] == (int)(unsigned)dbits(0.5) && rec[6] == (int)(unsigned)(dbits(0.5) >> 32), "0.5 as a double");
    CHECK(rec[7] == 2 && rec[9] == (int)(unsigned)dbits(-2.0) && rec[10] == (int)(unsigned)(dbits(-2.0) >> 32), "-2 as a double");
    CHECK(rec[11] == 0 && rec[12] == 0 && rec[13] == 0 && rec[14] == 0, "behind the live terms: zeros");
    // the row's count is the largest live term's: a dead long entry does not count
    const int ent2[] = {0, 2};
    const double w2[] = {1.0, 0.0};
    CHECK(mix_records(bank_nb, 4, nullptr, 1, 2, ent2, w2, rec) == BFIR_OK && rec[1] == 2 && rec[2] == 1, "the live term's count");
    // no live term: no path
    const int none[] = {-1, 2};
    const double wn[] = {3.0, -0.0};
    CHECK(mix_records(bank_nb, 8, nullptr, 1, 2, none, wn, rec) == BFIR_OK && rec == V(kMixRec, 0), "no live term");
    // finite as a double, infinite as a float; and one that only rounds to zero as a float
    const int e0[] = {0};
    const double big[] = {1e39}, tiny[] = {1e-60};
    CHECK(mix_records(bank_nb, 4, nullptr, 1, 1, e0, big, rec) == BFIR_ERR_ARG, "1e39 in float");
    CHECK(mix_records(bank_nb, 8, nullptr, 1, 1, e0, big, rec) == BFIR_OK && rec[2] == 1, "1e39 in double");
    CHECK(mix_records(bank_nb, 4, nullptr, 1, 1, e0, tiny, rec) == BFIR_OK && rec[2] == 0 && rec[1] == 0, "1e-60 in float is 0");
    CHECK(mix_records(bank_nb, 8, nullptr, 1, 1, e0, tiny, rec) == BFIR_OK && rec[2] == 1 && rec[1] == 2, "1e-60 in double");
    const double nan[] = {std::numeric_limits<double>::quiet_NaN()}, inf[] = {-std::numeric_limits<double>::infinity()};
    for (int s : {4, 8}) {
        CHECK(mix_records(bank_nb, s, nullptr, 1, 1, e0, nan, rec) == BFIR_ERR_ARG, "NaN, s = %d", s);
        CHECK(mix_records(bank_nb, s, nullptr, 1, 1, e0, inf, rec) == BFIR_ERR_ARG, "-Inf, s = %d", s);
        // the empty entry: a zero weight may name it, a live term may not
        const int e1[] = {0, 1};
        const double zero[] = {1.0, 0.0}, live[] = {1.0, 0.25};
        CHECK(mix_records(bank_nb, s, nullptr, 1, 2, e1, zero, rec) == BFIR_OK && rec[2] == 1, "zero weight on an empty entry, s = %d", s);
        CHECK(mix_records(bank_nb, s, nullptr, 1, 2, e1, live, rec) == BFIR_ERR_STATE, "live term on an empty entry, s = %d", s);
        // an entry outside the bank is refused live or not, and before the state
        const int out[] = {1, 3}, low[] = {0, -2};
        CHECK(mix_records(bank_nb, s, nullptr, 1, 2, out, zero, rec) == BFIR_ERR_ARG, "entry n_entries, weight 0, s = %d", s);
        CHECK(mix_records(bank_nb, s, nullptr, 1, 2, out, live, rec) == BFIR_ERR_ARG, "entry n_entries behind a live empty one, s = %d", s);
        CHECK(mix_records(bank_nb, s, nullptr, 1, 2, low, zero, rec) == BFIR_ERR_ARG, "entry -2, s = %d", s);
    }
    // all four terms live
    const int e4[] = {2, 0, 2, 0};
    const double w4[] = {1.0, 2.0, 3.0, 4.0};
    CHECK(mix_records(bank_nb, 4, nullptr, 1, 4, e4, w4, rec) == BFIR_OK && rec[2] == 4 && rec[1] == 3, "four terms");
    CHECK(rec[kMixRec - 4] == 0 && rec[kMixRec - 3] == 2 && rec[kMixRec - 2] == (int)fbits(4.0f), "the last term fills the record");
}

int main()
{
    test_list_check();
    test_patch_table();
    test_entries_and_gather_tables();
    test_mix_records();
    if (g_fail) { printf("%d FAILED\n", g_fail); return 1; }
    printf("ALL OK\n");
    return 0;
}
