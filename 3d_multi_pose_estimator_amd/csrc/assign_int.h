// The largest sum a one-to-one pairing of rows and columns can collect from a table of non-negative integers: IDTP of
// mpe_track_score_result (rows: ground-truth identities, columns: track ids, entries: frames the two were matched).
// Plain C++, no device code: this step is HOST work.  It runs once per recording, after the state has been read back,
// on a table of a few dozen used rows and columns; the per-frame work is track_score.hip's.
//
// Rectangular shortest-augmenting-path solver (the Hungarian method with potentials, O(n^2 m) for n <= m) over the
// rows and columns that hold a non-zero entry only; all arithmetic in int64, so entries up to 2^31 - 1 and any number
// of rows below 2^31 stay exact.  Header-only so that a stand-alone test program can include it.
#pragma once
#include <cstddef>
#include <cstdint>
#include <limits>
#include <vector>

namespace mpe {

// table: n_rows x n_cols, row stride ld, entries >= 0.  Either count may be 0.
inline int64_t assign_int_max(const int32_t *table, size_t n_rows, size_t n_cols, size_t ld) {
    std::vector<size_t> rows, cols;
    std::vector<char> col_used(n_cols, 0);
    for (size_t r = 0; r < n_rows; ++r) {
        bool any = false;
        for (size_t c = 0; c < n_cols; ++c)
            if (table[r * ld + c] != 0) {
                any = true;
                col_used[c] = 1;
            }
        if (any) rows.push_back(r);
    }
    for (size_t c = 0; c < n_cols; ++c)
        if (col_used[c]) cols.push_back(c);
    if (rows.empty()) return 0;
    // the short side takes the solver's rows
    const bool flip = rows.size() > cols.size();
    const size_t n = flip ? cols.size() : rows.size(), m = flip ? rows.size() : cols.size();
    auto value = [&](size_t i, size_t j) -> int64_t {
        return flip ? (int64_t)table[rows[j] * ld + cols[i]] : (int64_t)table[rows[i] * ld + cols[j]];
    };
    const int64_t INF = std::numeric_limits<int64_t>::max() / 4;
    std::vector<int64_t> u(n + 1, 0), v(m + 1, 0), minv(m + 1);
    std::vector<size_t> p(m + 1, 0), way(m + 1, 0);
    std::vector<char> used(m + 1);
    for (size_t i = 1; i <= n; ++i) {
        p[0] = i;
        size_t j0 = 0;
        minv.assign(m + 1, INF);
        used.assign(m + 1, 0);
        do {
            used[j0] = 1;
            const size_t i0 = p[j0];
            int64_t delta = INF;
            size_t j1 = 0;
            for (size_t j = 1; j <= m; ++j) {
                if (used[j]) continue;
                const int64_t cur = -value(i0 - 1, j - 1) - u[i0] - v[j];          // cost = -value: least cost, largest sum
                if (cur < minv[j]) {
                    minv[j] = cur;
                    way[j] = j0;
                }
                if (minv[j] < delta) {
                    delta = minv[j];
                    j1 = j;
                }
            }
            for (size_t j = 0; j <= m; ++j) {
                if (used[j]) {
                    u[p[j]] += delta;
                    v[j] -= delta;
                } else {
                    minv[j] -= delta;
                }
            }
            j0 = j1;
        } while (p[j0] != 0);
        do {
            const size_t j1 = way[j0];
            p[j0] = p[j1];
            j0 = j1;
        } while (j0 != 0);
    }
    int64_t sum = 0;
    for (size_t j = 1; j <= m; ++j)
        if (p[j] != 0) sum += value(p[j] - 1, j - 1);
    return sum;
}

}  // namespace mpe
