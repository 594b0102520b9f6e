// coeff_tables.h -- the host arithmetic that turns the integers a caller hands to a set call (pairs, bank entries, mix terms)
// into the tables the kernels read: k_patch_pairs' table (patch.hip), k_bank_gather's (bank.hip), k_lbank_gather's (lbank.hip),
// k_bank_mix's records (bankmix.hip) and k_lbank_mix's (lbankmix.hip).  Every index and count a kernel takes from a table is
// checked here.
//
// Host only: no HIP header, no engine; plain ints and vectors in, vectors and BFIR_* codes out, so that a stand-alone program
// can run it under the host sanitizers (tests/cpp/test_coeff_tables.cpp).  engine.hip is its one user in the library.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/bfir_hip.h"

namespace coeff_tables {

constexpr int kMixRec = 3 + 4 * BFIR_BANK_MIX_TERMS;          // words of a mix record (kernels.h: BFIR_BANK_MIX_REC)
constexpr int kLevelRec = 2 + BFIR_MAX_LEVELS;                // words of a row of k_lbank_gather's table

// the store row that row j of a call goes to: list[j], or j where the call names the whole store (list == nullptr)
inline int dest_row(const std::vector<int> *list, size_t j) { return list ? (*list)[j] : (int)j; }

// The list of a pairs call, n pairs (outputs[k], inputs[k]) of an n_out x n_in matrix, as the rows o n_in + i of the filter
// store.  BFIR_ERR_ARG: a pair outside the matrix, or the same pair twice.
inline int list_rows(int n_out, int n_in, int n, const int *outputs, const int *inputs, std::vector<int> &rows)
{
    std::vector<char> listed((size_t)n_out * n_in, 0);
    rows.resize((size_t)std::max(n, 0));
    for (int k = 0; k < n; k++) {
        if (outputs[k] < 0 || outputs[k] >= n_out || inputs[k] < 0 || inputs[k] >= n_in) return BFIR_ERR_ARG;
        const int r = outputs[k] * n_in + inputs[k];
        if (listed[r]) return BFIR_ERR_ARG;                     // the same pair twice
        listed[r] = 1;
        rows[k] = r;
    }
    return BFIR_OK;
}

// k_patch_pairs' table: [n_out + 1] row starts, then per output its listed pairs in input order as (input, nb_new, nb_old)
// triples.  list: checked rows; nb_new, nb_old: the partition counts of the two sets, [n_out n_in].
inline std::vector<int> patch_table(int n_out, int n_in, const std::vector<int> &list, const std::vector<int> &nb_new,
                                    const std::vector<int> &nb_old)
{
    std::vector<char> listed((size_t)n_out * n_in, 0);
    for (int r : list) listed[r] = 1;
    std::vector<int> tab((size_t)n_out + 1);
    for (int o = 0; o < n_out; o++) {
        tab[o] = (int)(tab.size() - (n_out + 1)) / 3;
        for (int i = 0; i < n_in; i++) {
            const int r = o * n_in + i;
            if (listed[r]) { tab.push_back(i); tab.push_back(nb_new[r]); tab.push_back(nb_old[r]); }
        }
    }
    tab[n_out] = (int)list.size();
    return tab;
}

// The n entries of a bank call: each -1 (no path) or an entry of the bank.  filled: per entry of the bank, 0 = empty.
// BFIR_ERR_ARG: an entry outside the bank; then BFIR_ERR_STATE: an empty entry named.
inline int check_entries(const std::vector<int> &filled, int n, const int *entries, std::vector<int> &ent)
{
    for (int k = 0; k < n; k++) if (entries[k] < -1 || entries[k] >= (int)filled.size()) return BFIR_ERR_ARG;
    ent.assign(entries, entries + std::max(n, 0));
    for (int en : ent) if (en >= 0 && filled[en] == 0) return BFIR_ERR_STATE;
    return BFIR_OK;
}

// the partition count a row gets from entry en of a bank with the counts bank_nb (-1: no path, none)
inline int entry_count(const std::vector<int> &bank_nb, int en) { return en < 0 ? 0 : bank_nb[en]; }

// k_bank_gather's table, [rows][3]: destination row, entry or -1, partitions
inline std::vector<int> gather_table(const std::vector<int> *list, const std::vector<int> &ent, const std::vector<int> &bank_nb)
{
    std::vector<int> tab;
    tab.reserve(3 * ent.size());
    for (size_t j = 0; j < ent.size(); j++) {
        tab.push_back(dest_row(list, j)); tab.push_back(ent[j]); tab.push_back(entry_count(bank_nb, ent[j]));
    }
    return tab;
}

// k_lbank_gather's table, [rows][2 + BFIR_MAX_LEVELS]: destination row, entry or -1, then the entry's partitions on each of
// the n_levels levels (lbank_nb: [entry][BFIR_MAX_LEVELS]); -1 and the levels the engine does not have: 0
inline std::vector<int> level_gather_table(const std::vector<int> *list, const std::vector<int> &ent,
                                           const std::vector<int> &lbank_nb, int n_levels)
{
    std::vector<int> tab(kLevelRec * ent.size(), 0);
    for (size_t j = 0; j < ent.size(); j++) {
        int *rec = &tab[kLevelRec * j];
        rec[0] = dest_row(list, j); rec[1] = ent[j];
        for (int k = 0; k < n_levels && ent[j] >= 0; k++) rec[2 + k] = lbank_nb[(size_t)ent[j] * BFIR_MAX_LEVELS + k];
    }
    return tab;
}

// The live terms of the n rows of a mix call: row j has the n_terms terms (entries[j n_terms + t], weights[j n_terms + t]) on a
// bank of n_ent entries.  Every weight is converted once to the working precision (s = 4: float, 8: double); a term is live
// iff its entry is >= 0 and the converted weight is not zero.  live gets [n][kLiveRec]: the live terms, then those terms
// compacted to the front in listed order, each (entry, the weight's bits low, high).  BFIR_ERR_ARG: an entry outside the
// bank, live or not, a weight that is not finite or not finite in the working precision.
constexpr int kLiveRec = 1 + 3 * BFIR_BANK_MIX_TERMS;
inline int live_terms(int n_ent, int s, int n, int n_terms, const int *entries, const double *weights, std::vector<int> &live)
{
    live.assign((size_t)std::max(n, 0) * kLiveRec, 0);
    for (int j = 0; j < n; j++) {
        int *r = &live[(size_t)j * kLiveRec];
        for (int t = 0; t < n_terms; t++) {
            const int en = entries[(size_t)j * n_terms + t];
            const double w = weights[(size_t)j * n_terms + t];
            if (en < -1 || en >= n_ent) return BFIR_ERR_ARG;    // live or not
            if (!std::isfinite(w)) return BFIR_ERR_ARG;
            unsigned long long bits;
            bool zero;
            if (s == 4) {
                const float wf = (float)w;
                if (!std::isfinite(wf)) return BFIR_ERR_ARG;    // infinite in the working precision
                unsigned u; memcpy(&u, &wf, sizeof u);
                bits = u; zero = wf == 0.0f;
            } else {
                memcpy(&bits, &w, sizeof bits); zero = w == 0.0;
            }
            if (en < 0 || zero) continue;
            int *term = r + 1 + 3 * r[0]++;
            term[0] = en; term[1] = (int)(unsigned)bits; term[2] = (int)(unsigned)(bits >> 32);
        }
    }
    return BFIR_OK;
}

// k_bank_mix's records for the n rows of a mix call (live_terms: the terms, the conversion, liveness).  rec gets [n][kMixRec]:
// destination row, the row's count (the largest of its live terms'; none live: 0, no path), the live terms, then the live
// terms compacted to the front in listed order, each (entry, its count, the weight's bits low, high).  BFIR_ERR_ARG: as
// live_terms; then BFIR_ERR_STATE: a live term names an empty entry.
inline int mix_records(const std::vector<int> &bank_nb, int s, const std::vector<int> *list, int n, int n_terms,
                       const int *entries, const double *weights, std::vector<int> &rec)
{
    std::vector<int> live;
    rec.assign((size_t)std::max(n, 0) * kMixRec, 0);
    const int rc = live_terms((int)bank_nb.size(), s, n, n_terms, entries, weights, live);
    if (rc != BFIR_OK) return rc;
    for (int j = 0; j < n; j++) {
        const int *lt = &live[(size_t)j * kLiveRec];
        int *r = &rec[(size_t)j * kMixRec];
        r[0] = dest_row(list, (size_t)j); r[2] = lt[0];
        for (int t = 0; t < lt[0]; t++) {
            int *term = r + 3 + 4 * t;
            term[0] = lt[1 + 3 * t]; term[1] = bank_nb[term[0]]; term[2] = lt[2 + 3 * t]; term[3] = lt[3 + 3 * t];
            r[1] = std::max(r[1], term[1]);
        }
    }
    for (int j = 0; j < n; j++) {
        const int *r = &rec[(size_t)j * kMixRec];
        for (int t = 0; t < r[2]; t++) if (r[4 + 4 * t] == 0) return BFIR_ERR_STATE;   // a live term names an empty entry
    }
    return BFIR_OK;
}

// k_lbank_mix's records, the multi-level form of mix_records: the bank is one store per level (lbank_len: the taps of every
// entry, 0 = empty; lbank_nb: [entry][BFIR_MAX_LEVELS] its partitions per level).  rec gets [n][kLevelMixRec]: destination
// row, the live terms, then per live term (entry, the weight's bits low, high, its count on each of BFIR_MAX_LEVELS levels;
// the levels the engine does not have: 0); the rest of a record is zeros.  nb gets [n][BFIR_MAX_LEVELS], the row's count on
// every level: the largest of its live terms' there (none live: 0 everywhere, no path).  A live term may have count 0 on a
// level its entry does not reach.  The refusals are mix_records', "empty" being lbank_len == 0.
constexpr int kLevelMixTerm = 3 + BFIR_MAX_LEVELS;
constexpr int kLevelMixRec = 32;
static_assert(2 + BFIR_BANK_MIX_TERMS * kLevelMixTerm <= kLevelMixRec, "a record holds its terms");
inline int level_mix_records(const std::vector<int> &lbank_len, const std::vector<int> &lbank_nb, int n_levels, int s,
                             const std::vector<int> *list, int n, int n_terms, const int *entries, const double *weights,
                             std::vector<int> &rec, std::vector<int> &nb)
{
    std::vector<int> live;
    rec.assign((size_t)std::max(n, 0) * kLevelMixRec, 0);
    nb.assign((size_t)std::max(n, 0) * BFIR_MAX_LEVELS, 0);
    const int rc = live_terms((int)lbank_len.size(), s, n, n_terms, entries, weights, live);
    if (rc != BFIR_OK) return rc;
    for (int j = 0; j < n; j++) {
        const int *lt = &live[(size_t)j * kLiveRec];
        int *r = &rec[(size_t)j * kLevelMixRec];
        r[0] = dest_row(list, (size_t)j); r[1] = lt[0];
        for (int t = 0; t < lt[0]; t++) {
            int *term = r + 2 + kLevelMixTerm * t;
            term[0] = lt[1 + 3 * t]; term[1] = lt[2 + 3 * t]; term[2] = lt[3 + 3 * t];
            for (int k = 0; k < n_levels && k < BFIR_MAX_LEVELS; k++) {
                term[3 + k] = lbank_nb[(size_t)term[0] * BFIR_MAX_LEVELS + k];
                int &c = nb[(size_t)j * BFIR_MAX_LEVELS + k];
                c = std::max(c, term[3 + k]);
            }
        }
    }
    for (int j = 0; j < n; j++) {
        const int *r = &rec[(size_t)j * kLevelMixRec];
        for (int t = 0; t < r[1]; t++) if (lbank_len[r[2 + kLevelMixTerm * t]] == 0) return BFIR_ERR_STATE;   // a live term names an empty entry
    }
    return BFIR_OK;
}

}   // namespace coeff_tables
