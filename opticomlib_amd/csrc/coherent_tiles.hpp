// coherent_tiles.hpp -- the geometry and the integer rules of the coherent QAM receiver (coherent.hip): the square Gray-mapped constellation and its level
// decision, the tiles, halos and truncated windows of the blind phase search, its phase groups, its grid, its LDS and the jump rule of the unwrap.  Plain
// C++ (constexpr functions of integers and doubles, no HIP type, no library call): the kernels, the entry points' argument checks and a host program
// of its own (tests/coherent_host.cpp) all call these and decide none of it themselves.
#pragma once
#include <cstddef>
#include <cstdint>

namespace ssfm {
namespace cpr {

constexpr int kTile = 256;           // symbols of one row a workgroup owns = its threads (opticomlib_amd/coherent.py mirrors it as CPR_TILE)
constexpr int kMaxWindow = 256;      // W: the window is the 2 W + 1 symbols around a symbol
constexpr int kMaxPhases = 64;       // B: test phases over a quarter turn
constexpr int kGroup = 8;            // test phases whose distances lie in LDS at once
constexpr int kMaxRows = 2;          // a record is (n,) or (2, n)
constexpr int64_t kMaxSymbols = int64_t(1) << 26;      // u = b + B n_k stays an int32: |n_k| <= n / 3 + 1 (two jumps of one sign need a step without one between them)

// ---- the constellation: M = L^2 points, k = log2 M bits per symbol, MSB first, the first k / 2 of them the in-phase level
constexpr bool valid_order(int M) { return M == 4 || M == 16 || M == 64 || M == 256; }
constexpr int side_of(int M) { return M == 4 ? 2 : M == 16 ? 4 : M == 64 ? 8 : 16; }
constexpr int bits_of(int M) { return M == 4 ? 2 : M == 16 ? 4 : M == 64 ? 6 : 8; }
// binary-reflected Gray code: the level whose bits read c, and the bits of level g
constexpr int gray_decode(int c) {
    for (int s = c >> 1; s; s >>= 1) c ^= s;
    return c;
}
constexpr int gray_encode(int g) { return g ^ (g >> 1); }
// amplitude of level g of L with half-spacing a: a (2 g - (L - 1))
constexpr double level_amp(int g, double a, int L) { return a * (double)(2 * g - (L - 1)); }
// decision of a real component: clip(floor(x / (2 a) + L / 2), 0, L - 1).  A value on a boundary takes the upper level, +-0 gives L / 2; a NaN gives 0.
constexpr int level_of(double x, double a, int L) {
    const double v = x / (2.0 * a) + (double)(L / 2);
    if (!(v >= 1.0)) return 0;
    if (v >= (double)(L - 1)) return L - 1;
    return (int)v;                                    // 1 <= v < L - 1: truncation is the floor
}

// ---- the search's limits: B even in 2 ... 64, 0 <= W <= 256, 1 <= n <= 2^26, one or two rows
constexpr bool valid_search(int B, int W, int64_t n, int rows) {
    return B >= 2 && B <= kMaxPhases && B % 2 == 0 && W >= 0 && W <= kMaxWindow && n >= 1 && n <= kMaxSymbols && rows >= 1 && rows <= kMaxRows;
}

// ---- tiles: tile t of a row of n symbols owns [tile_begin, tile_end); its workgroup also computes the distances of the halo, W symbols on each side
// as far as the row goes
constexpr int64_t tiles_of(int64_t n) { return (n + kTile - 1) / kTile; }
constexpr int64_t tile_begin(int64_t t) { return t * kTile; }
constexpr int64_t tile_end(int64_t t, int64_t n) { return (t + 1) * kTile < n ? (t + 1) * kTile : n; }
constexpr int64_t halo_begin(int64_t t, int W) { return tile_begin(t) - W > 0 ? tile_begin(t) - W : 0; }
constexpr int64_t halo_end(int64_t t, int W, int64_t n) { return tile_end(t, n) + W < n ? tile_end(t, n) + W : n; }
// LDS entry e of a tile holds symbol halo_base + e, whether the row reaches that far or not
constexpr int64_t halo_base(int64_t t, int W) { return tile_begin(t) - W; }
constexpr int halo_entries(int W) { return kTile + 2 * W; }
// the window of symbol k, truncated at both ends of the row: [window_begin, window_end)
constexpr int64_t window_begin(int64_t k, int W) { return k - W > 0 ? k - W : 0; }
constexpr int64_t window_end(int64_t k, int W, int64_t n) { return k + W + 1 < n ? k + W + 1 : n; }

// ---- the test phases go through LDS in groups of kGroup: group g holds phases [group_begin, group_end)
constexpr int groups_of(int B) { return (B + kGroup - 1) / kGroup; }
constexpr int group_begin(int g) { return g * kGroup; }
constexpr int group_end(int g, int B) { return (g + 1) * kGroup < B ? (g + 1) * kGroup : B; }
// dynamic LDS of the search: kGroup rows of halo_entries doubles.  Symbol after symbol lies double after double, so the 32 lanes of a half wave read 32
// consecutive doubles -- every one of the 64 banks once -- at every offset of the window, and write them so.
constexpr size_t search_lds_bytes(int W) { return (size_t)kGroup * (size_t)halo_entries(W) * sizeof(double); }
constexpr size_t kSearchLdsMax = search_lds_bytes(kMaxWindow);       // 48 KiB: what a kernel may use unasked

// ---- the grid of the search and of the unwrap: one workgroup per tile and row, row after row
constexpr int64_t grid_of(int rows, int64_t n) { return (int64_t)rows * tiles_of(n); }

// ---- the unwrap: the jump between the chosen phases of neighbouring symbols.  2 d > B: the phase fell over the sector's upper end (-1), 2 d < -B: over
// its lower end (+1); |d| = B / 2 is no jump.  n_k is the running sum of the jumps, u_k = b_k + B n_k
constexpr int jump_of(int prev, int cur, int B) {
    const int d = cur - prev;
    return 2 * d > B ? -1 : (2 * d < -B ? 1 : 0);
}

}  // namespace cpr
}  // namespace ssfm
