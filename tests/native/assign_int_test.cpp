// csrc/assign_int.h (the one-to-one pairing behind IDTP) against brute force over all pairings: rectangular tables both
// ways, zero rows and columns, ties, entries near 2^31, and empty tables.  Prints "tested N bad M".
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <numeric>
#include <vector>

#include "assign_int.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return (uint32_t)(rng_state >> 32);
}

// the largest sum over all one-to-one pairings: every injection of the short side into the long side
static int64_t brute(const std::vector<int32_t> &t, size_t n, size_t m) {
    if (n == 0 || m == 0) return 0;
    const bool flip = n > m;
    const size_t a = flip ? m : n, b = flip ? n : m;
    std::vector<size_t> perm(b);
    std::iota(perm.begin(), perm.end(), 0);
    int64_t best = 0;
    do {
        int64_t s = 0;
        for (size_t i = 0; i < a; ++i) s += flip ? (int64_t)t[perm[i] * m + i] : (int64_t)t[i * m + perm[i]];
        best = std::max(best, s);
    } while (std::next_permutation(perm.begin(), perm.end()));
    return best;
}

int main() {
    long tested = 0, bad = 0;
    auto check = [&](const std::vector<int32_t> &t, size_t n, size_t m, const char *what) {
        const int64_t got = mpe::assign_int_max(t.data(), n, m, m), want = brute(t, n, m);
        ++tested;
        if (got != want) {
            ++bad;
            std::printf("%s %zux%zu: got %lld want %lld\n", what, n, m, (long long)got, (long long)want);
        }
    };
    check({}, 0, 0, "empty");
    check({}, 0, 5, "no rows");
    check({}, 5, 0, "no columns");
    check(std::vector<int32_t>(12, 0), 3, 4, "all zero");
    check({7}, 1, 1, "one");
    check({5, 5, 5, 5}, 2, 2, "ties");
    check({3, 3, 3, 3, 3, 3}, 2, 3, "ties wide");
    check({3, 3, 3, 3, 3, 3}, 3, 2, "ties tall");
    check({0, 0, 0, 0, 9, 0, 0, 0, 0}, 3, 3, "one entry");
    check({1, 2, 0, 0, 0, 0, 3, 4, 0}, 3, 3, "zero row and column");
    const int32_t big = 2147483647;
    check({big, big - 1, big - 2, big, big - 1, big, big, big - 3, big}, 3, 3, "near 2^31");
    check({big, big, big, big, big, big, big, big, big, big, big, big, big, big, big, big, big, big, big, big, big, big, big, big}, 4, 6,
          "all 2^31 - 1");
    for (int it = 0; it < 600; ++it) {
        const size_t n = 1 + rnd() % 6, m = 1 + rnd() % 7;
        const int kind = it % 4;
        std::vector<int32_t> t(n * m);
        for (auto &x : t) {
            const uint32_t r = rnd();
            if (kind == 0) x = (int32_t)(r % 4);                                   // many ties and zeros
            else if (kind == 1) x = (r & 1) ? 0 : (int32_t)(r % 1000);             // sparse: zero rows and columns
            else if (kind == 2) x = big - (int32_t)(r % 8);                        // near 2^31
            else x = (int32_t)(r % 100000);
        }
        if (kind == 1 && n > 1)
            for (size_t j = 0; j < m; ++j) t[(rnd() % n) * m + j] = 0;
        check(t, n, m, "random");
    }
    // a row stride larger than the width
    {
        std::vector<int32_t> t = {4, 1, 99, 99, 2, 8, 99, 99};
        const int64_t got = mpe::assign_int_max(t.data(), 2, 2, 4);
        ++tested;
        if (got != 12) {
            ++bad;
            std::printf("stride: got %lld want 12\n", (long long)got);
        }
    }
    std::printf("tested %ld bad %ld\n", tested, bad);
    return bad != 0;
}
