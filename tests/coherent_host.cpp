// coherent_host.cpp -- opticomlib_amd/csrc/coherent_tiles.hpp held to brute force on the host: the tiles cover every row once, every symbol's window lies inside
// its tile and halo and nowhere else, the phase groups cover the test phases once, the LDS and grid sizes are what the layout needs, the level decision
// at, below and above every boundary, the Gray code and the jump rule.  A program of its own (test_coherent_cpu.py builds it with AddressSanitizer and UBSan and runs it); no GPU.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "coherent_tiles.hpp"

namespace cpr = ssfm::cpr;

static long long g_checks = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        ++g_checks;                                       \
        if (!(cond)) {                                    \
            std::printf("FAILED %s:%d: ", __FILE__, __LINE__); \
            std::printf(__VA_ARGS__);                     \
            std::printf("\n");                            \
            std::exit(1);                                 \
        }                                                 \
    } while (0)

static void tiles_and_windows() {
    const int T = cpr::kTile;
    const int windows[] = {0, 1, 7, 256};
    for (int W : windows) {
        const int entries = cpr::halo_entries(W);
        CHECK(cpr::search_lds_bytes(W) == (size_t)cpr::kGroup * entries * 8 && cpr::search_lds_bytes(W) <= cpr::kSearchLdsMax, "lds W=%d", W);
        for (int64_t n = 1; n <= 3 * T + W + 2; ++n) {
            const int64_t tiles = cpr::tiles_of(n);
            CHECK(cpr::grid_of(1, n) == tiles && cpr::grid_of(2, n) == 2 * tiles, "grid n=%lld", (long long)n);
            std::vector<int> owner(n, 0);
            for (int64_t t = 0; t < tiles; ++t) {
                const int64_t b = cpr::tile_begin(t), e = cpr::tile_end(t, n);
                CHECK(b < e && e <= n && e - b <= T, "tile %lld of n=%lld", (long long)t, (long long)n);
                const int64_t hb = cpr::halo_begin(t, W), he = cpr::halo_end(t, W, n), base = cpr::halo_base(t, W);
                CHECK(hb == (b - W > 0 ? b - W : 0) && he == (e + W < n ? e + W : n), "halo of tile %lld n=%lld W=%d", (long long)t, (long long)n, W);
                CHECK(hb - base >= 0 && he - base <= entries, "halo of tile %lld n=%lld W=%d leaves the LDS row", (long long)t, (long long)n, W);
                for (int64_t k = b; k < e; ++k) {
                    ++owner[k];
                    const int64_t wb = cpr::window_begin(k, W), we = cpr::window_end(k, W, n);
                    // the window is the brute-force set of j with |j - k| <= W inside the row ...
                    int64_t lo = n, hi = -1;
                    for (int64_t j = (k - W - 2 > 0 ? k - W - 2 : 0); j < n && j <= k + W + 2; ++j)
                        if (std::llabs(j - k) <= W) {
                            lo = j < lo ? j : lo;
                            hi = j > hi ? j : hi;
                        }
                    CHECK(wb == lo && we == hi + 1, "window of k=%lld n=%lld W=%d", (long long)k, (long long)n, W);
                    // ... and lies inside the owner's halo, at LDS entries inside the row
                    CHECK(wb >= hb && we <= he && wb - base >= 0 && we - base <= entries, "window of k=%lld leaves tile %lld (n=%lld W=%d)", (long long)k, (long long)t,
                          (long long)n, W);
                }
            }
            for (int64_t k = 0; k < n; ++k) CHECK(owner[k] == 1, "symbol %lld of n=%lld has %d tiles", (long long)k, (long long)n, owner[k]);
        }
    }
    CHECK(cpr::kSearchLdsMax == 48 * 1024, "LDS at the widest window");
    CHECK(cpr::halo_entries(cpr::kMaxWindow) <= 3 * T, "three entries per thread hold the widest halo");
}

static void phase_groups() {
    for (int B = 2; B <= cpr::kMaxPhases; B += 2) {
        std::vector<int> seen(B, 0);
        const int groups = cpr::groups_of(B);
        for (int g = 0; g < groups; ++g) {
            const int b = cpr::group_begin(g), e = cpr::group_end(g, B);
            CHECK(b < e && e - b <= cpr::kGroup && e <= B, "group %d of B=%d", g, B);
            for (int p = b; p < e; ++p) ++seen[p];
        }
        for (int p = 0; p < B; ++p) CHECK(seen[p] == 1, "phase %d of B=%d in %d groups", p, B, seen[p]);
        CHECK(cpr::group_end(groups - 1, B) == B, "the last group of B=%d", B);
    }
    for (int B = -2; B <= 70; ++B)
        for (int W = -1; W <= 258; W += 37) {
            const bool want = B >= 2 && B <= 64 && B % 2 == 0 && W >= 0 && W <= 256;
            CHECK(cpr::valid_search(B, W, 5, 1) == want && cpr::valid_search(B, W, 5, 2) == want, "limits B=%d W=%d", B, W);
            CHECK(!cpr::valid_search(B, W, 0, 1) && !cpr::valid_search(B, W, 5, 3) && !cpr::valid_search(B, W, cpr::kMaxSymbols + 1, 1), "limits n, rows");
        }
}

static void constellation() {
    const int orders[] = {4, 16, 64, 256};
    for (int M = 0; M <= 300; ++M) {
        bool is = false;
        for (int o : orders) is = is || o == M;
        CHECK(cpr::valid_order(M) == is, "order %d", M);
    }
    for (int M : orders) {
        const int L = cpr::side_of(M), k = cpr::bits_of(M);
        CHECK(L * L == M && (1 << k) == M, "M=%d", M);
        const double a = 1.0 / std::sqrt(2.0 * (M - 1) / 3.0);
        // Gray code: a bijection on 0 ... L - 1 whose neighbours differ in one bit
        std::vector<int> seen(L, 0);
        for (int c = 0; c < L; ++c) {
            const int g = cpr::gray_decode(c);
            CHECK(g >= 0 && g < L && cpr::gray_encode(g) == c, "gray M=%d c=%d", M, c);
            ++seen[g];
            int ref = 0;                                   // bit by bit: b_i = c_i xor b_(i+1)
            for (int i = 8; i >= 0; --i) ref |= (((c >> i) & 1) ^ ((ref >> (i + 1)) & 1)) << i;
            CHECK(g == ref, "gray_decode(%d) = %d, bit by bit %d", c, g, ref);
        }
        for (int g = 0; g < L; ++g) {
            CHECK(seen[g] == 1, "gray level %d of M=%d", g, M);
            if (g) CHECK(__builtin_popcount(cpr::gray_encode(g) ^ cpr::gray_encode(g - 1)) == 1, "gray neighbours %d of M=%d", g, M);
        }
        // unit mean power, and every level decides as itself
        double p = 0.0;
        for (int g = 0; g < L; ++g) {
            const double x = cpr::level_amp(g, a, L);
            p += 2.0 * L * x * x;
            CHECK(cpr::level_of(x, a, L) == g, "level %d of M=%d", g, M);
        }
        CHECK(std::fabs(p / M - 1.0) < 1e-14, "mean power of M=%d: %.17g", M, p / M);
        // the boundaries 2 a m, m = -(L / 2 - 1) ... L / 2 - 1: the upper level at the boundary, the lower one below it
        for (int m = -(L / 2 - 1); m <= L / 2 - 1; ++m) {
            const double x = 2.0 * a * m;
            const int up = m + L / 2;
            CHECK(cpr::level_of(x, a, L) == up, "at boundary %d of M=%d", m, M);
            CHECK(cpr::level_of(x + 1e-9 * a, a, L) == up && cpr::level_of(x - 1e-9 * a, a, L) == up - 1, "beside boundary %d of M=%d", m, M);
            // one ulp beside it the rule is its own float64 expression: x / (2 a) + L / 2 may round onto the boundary
            for (double y : {std::nextafter(x, 10.0), std::nextafter(x, -10.0)}) {
                double v = std::floor(y / (2.0 * a) + L / 2);
                v = v < 0 ? 0 : (v > L - 1 ? L - 1 : v);
                CHECK(cpr::level_of(y, a, L) == (int)v && ((int)v == up || (int)v == up - 1), "an ulp beside boundary %d of M=%d", m, M);
            }
        }
        CHECK(cpr::level_of(0.0, a, L) == L / 2 && cpr::level_of(-0.0, a, L) == L / 2, "+-0 of M=%d", M);
        CHECK(cpr::level_of(-1e300, a, L) == 0 && cpr::level_of(1e300, a, L) == L - 1 && cpr::level_of(-HUGE_VAL, a, L) == 0 && cpr::level_of(HUGE_VAL, a, L) == L - 1,
              "beyond the outer levels of M=%d", M);
        CHECK(cpr::level_of(std::nan(""), a, L) == 0, "NaN of M=%d", M);
        // against the rule as written, on a grid of values
        for (int i = -4000; i <= 4000; ++i) {
            const double x = i * (a * L / 3000.0);
            double v = std::floor(x / (2.0 * a) + L / 2);
            v = v < 0 ? 0 : (v > L - 1 ? L - 1 : v);
            CHECK(cpr::level_of(x, a, L) == (int)v, "level_of(%g) of M=%d", x, M);
        }
    }
}

static void jump_rule() {
    for (int B = 2; B <= cpr::kMaxPhases; B += 2)
        for (int p = 0; p < B; ++p)
            for (int c = 0; c < B; ++c) {
                const int d = c - p, want = 2 * d > B ? -1 : (2 * d < -B ? 1 : 0);
                CHECK(cpr::jump_of(p, c, B) == want, "jump %d -> %d of B=%d", p, c, B);
                if (d == B / 2 || d == -B / 2) CHECK(cpr::jump_of(p, c, B) == 0, "|d| = B / 2 is no jump (B=%d)", B);
                // the unwrapped index moves by less than half a sector's worth of phases... except at |d| = B / 2 exactly
                const int du = d + B * cpr::jump_of(p, c, B);
                CHECK(2 * du <= B && 2 * du >= -B, "unwrapped step %d of B=%d", du, B);
            }
}

int main() {
    tiles_and_windows();
    phase_groups();
    constellation();
    jump_rule();
    std::printf("ok: %lld checks\n", g_checks);
    return 0;
}
