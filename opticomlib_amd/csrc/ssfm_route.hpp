// ssfm_route.hpp -- what a plan looks like and which engine a call takes: the shape rules of plan creation and the routes of the fixed-step and the
// adaptive entry points, as pure functions of plain values.  Plain C++ -- no HIP types, no environment, no allocation -- so that a host program can
// hold them to a table (tests/route_host.cpp, tests/test_route_cpu.py).  The kernel headers and ssfm_host.hip include it; nothing is decided twice.
#pragma once
#include <cstdint>
#include <optional>
#include "ssfm_amd.h"
#if defined(__HIPCC__)
#define SSFM_HD __host__ __device__
#else
#define SSFM_HD
#endif
namespace ssfm {
// ----------------------------------------------------------------------------- the shape predicates and their constants: the one copy
constexpr int kLog2MaxDirect = 22;                // the two-kernel engine's own range: N1 <= 512 column points x N2 <= 8192 row points
constexpr int kSplitLog2M = 20, kSplitMaxR = 16;  // sub-sequence length of a split plan (env SSFM_SPLIT_LOG2M = 20 | 21 | 22 overrides: diagnostics), and how many of them at most
constexpr int kMaxTables = 4, kMaxLanes = 8;
constexpr int kAdaptSlots = 64, kAdaptWords = 512;       // kAdaptWords: workgroups of the largest fused adaptive column kernel (2^20 x 2: 256 tiles x 2 rows)
constexpr int kBarShards = 8, kBarWords = 64;     // kBarWords: one-XCD form, a flag word per workgroup (no atomics), behind the shards; then the error word and the ticket counter
constexpr long long medium_max_samples = 1ll << 17;      // samples in all (rows x n) up to which the one-XCD engine is used (measured: a gain up to there)
// C, columns per k_time tile: one 128-byte line per row segment in either precision.  (complex128 used 16 as well
// at first: 512-thread workgroups, one per CU; with 8 the two precisions have the same workgroup shape, two per CU.)
template <typename T> constexpr int cols_per_tile() { return sizeof(T) == 8 ? 8 : 16; }
// the "U16" field layout between the two kernels (complex64, 16-byte units: ssfm_kernels.hpp)
template <typename T> SSFM_HD constexpr bool u16_layout(int N1, int C, int E) { return sizeof(T) == 4 && C == 16 && ((N1 / E) % 4) == 0 && N1 / E >= 4; }
// k_small: one workgroup per row, the whole schedule in one launch.  Points per thread: 8 up to 2048 samples and for
// complex128 (more wavefronts per row; complex128 with 16 would not fit the registers), 16 for complex64 rows of 4096 / 8192.
constexpr int kSmallE16Min = 4096;
template <typename T> constexpr int small_points(int n) { return sizeof(T) == 4 && n >= kSmallE16Min ? 16 : 8; }
template <typename T> constexpr bool small_supported(int n) { return n >= 256 && n <= (sizeof(T) == 4 ? 8192 : 4096) && (n & (n - 1)) == 0; }
template <typename T> constexpr bool small_adapt_supported(int n, int rows) {     // (8192 x 1: 14.8 us per step, chunked 12.7)
    return small_supported<T>(n) && n <= 4096 && rows >= 1 && rows <= 2 && rows * n / small_points<T>(n) <= 512; }
constexpr bool line_half_shape(int N1, int N2, int E, int Ef) { return ((N1 == 256 && E == 8) || (N1 == 512 && E == 16)) && Ef == 16 && N2 >= 1024 && N2 <= 8192; }
// fixed-step runs of a dual-polarisation plan of long rows on the one-XCD engine: one launch per row (ssfm_host.hip run_medium)
constexpr bool medium_rows_split(bool split_ok, int64_t n, int batch) { return split_ok && batch == 2 && n >= (1ll << 16); }

// ----------------------------------------------------------------------------- the shape of a plan
// The environment's overrides as ssfm_host.hip read them at plan creation: empty = not set, else atoi() of the text
struct ShapeKnobs { std::optional<int> split_above, split_log2m, e, ef, ef_fly, lanes, small; };
struct PlanShape {
    int log2_full = 0, split_R = 1;    // the caller's row length is 2^log2_full; split_R > 1: a split plan (ssfm_split.hpp) of split_R sub-sequences per row
    bool too_many = false;             // ... of more sub-sequences than a launch grid takes: no plan (nothing below is set)
    int64_t n = 0;                     // what the kernels work on: `batch` sub-sequences of a split plan, else the caller's rows; n = N1 column points x N2 row points
    int batch = 0, N1 = 0, N2 = 0;
    int E = 16, Ef = 16, Ef_fly = 16;  // points per thread of k_time, of k_freq, and of k_freq where it forms exp(D~ h) itself
    int lanes_wanted = 1, nlanes = 1;  // as asked for (SSFM_LANES or the size rule); as the rows allow
    bool u16 = false, small = false;   // the unit layout between the kernels; the one-workgroup-per-row engine serves this plan
};
template <typename T> PlanShape plan_shape(int64_t n_full, int batch_full, const ShapeKnobs& kn) {
    PlanShape s;
    s.n = n_full; s.batch = batch_full;
    while ((1ll << s.log2_full) < n_full) ++s.log2_full;
    const int kf = s.log2_full;
    int above = kLog2MaxDirect, k = 0;
    if (kn.split_above && *kn.split_above >= kSplitLog2M && *kn.split_above < kLog2MaxDirect) above = *kn.split_above;      // (tests: split plans of 2^21 / 2^22 samples)
    if (kf > above) {
        // a split plan: R sub-sequences of M = 2^20 samples per row (the size the two-kernel engine runs best at; SSFM_SPLIT_LOG2M = 21 | 22: diagnostics)
        int lm = kSplitLog2M;
        if (kn.split_log2m && *kn.split_log2m >= 20 && *kn.split_log2m <= kLog2MaxDirect) lm = *kn.split_log2m;
        if (lm >= kf) lm = kf - 1;
        while ((1 << (kf - lm)) > kSplitMaxR) ++lm;
        s.split_R = 1 << (kf - lm);
        if ((long long)batch_full * s.split_R > 65535) { s.too_many = true; return s; }
        s.n = 1ll << lm; s.batch = batch_full * s.split_R;
    }
    while ((1ll << k) < s.n) ++k;
    // N = N1 * N2: N1 = 2^floor(k/2) up to 256, N2 up to 4096; beyond 2^20: N1 = 512, N2 up to 8192
    const int k1 = k <= 20 ? (k / 2 < 8 ? k / 2 : 8) : 9;
    s.N1 = 1 << k1; s.N2 = 1 << (k - k1);
    // measured: complex64 with 8 points per thread (twice the waves, one more exchange) is 10 % slower;
    // complex128 is 5 % FASTER with 8 (16 need the whole register file: 1 wave per SIMD, AGPR spills)
    s.E = sizeof(T) == 8 ? 8 : 16;
    if (kn.e) s.E = *kn.e == 16 ? 16 : 8;
    // k_freq: complex128 rows run best with 16 points per thread and load-at-use twiddles (256-thread workgroups,
    // two per CU; C1 46.8 -> 44.7 us per step), complex64 rows with 16 and register twiddles (8: 22.2 vs 21.4 us)
    s.Ef = 16;
    // up to 2^17 points a step is bound by launch and instruction latency, not by the exchanges: 8 points
    // per thread in both kernels (twice the wavefronts per workgroup) is 5-19 % faster there (tools/small_n.py:
    // 7.0 -> 5.7 us per step at 2^10..2^12, 8.6 -> 7.9 at 2^15, 11.3 -> 10.3 at 2^17; equal at 2^18, slower above)
    // (complex128 likewise in k_freq: 9.0 -> 7.7 us per step at 2^10, 13.2 -> 12.3 at 2^16, 17.1 -> 15.2 at 2^17 x 2)
    if (k <= 17 && !kn.e) s.E = s.Ef = 8;        // (the environment knobs below still override)
    if (kn.e) s.Ef = s.E;
    if (kn.ef) s.Ef = *kn.ef == 16 ? 16 : 8;
    if (k > 20) s.E = s.Ef = 16;        // the large tiles (N1 = 512, N2 = 8192) exist for 16 points per thread only
    // complex128 rows that form exp(D~ h) in the kernel: 16 points per thread need 256 VGPRs + 164 AGPRs (one wave per SIMD),
    // 8 need 248 (two): adaptive 2^20 x 2 81.3 -> 74.6 us per step (profiles/r02_adaptive_c128_ef.txt).  The operator table's
    // order follows the points per thread, so these rows get their own copy of D~ and of the row twiddles.
    s.Ef_fly = s.Ef;
    if (sizeof(T) == 8 && s.Ef == 16 && k <= 20 && !kn.e && !kn.ef) s.Ef_fly = 8;
    if (kn.ef_fly) s.Ef_fly = k > 20 ? 16 : (*kn.ef_fly == 16 ? 16 : 8);
    // two lanes pay off once a launch is long enough to hide the other lane's gap; below ~2^20 points in
    // all a step is launch-bound and the second stream only doubles the launches (2^14 x 2: 8.1 us per
    // step with one lane, 12.0 with two; 2^18 x 2: 14.1 / 14.2; 2^20 x 2: 25.6 / 22.9 in a 200-step run)
    s.lanes_wanted = kn.lanes ? *kn.lanes : ((long long)s.batch * s.n >= (1ll << 20) ? 2 : 1);
    s.nlanes = s.lanes_wanted < 1 ? 1 : (s.lanes_wanted > kMaxLanes ? kMaxLanes : s.lanes_wanted);
    if (s.nlanes > batch_full) s.nlanes = batch_full;
    while (batch_full % s.nlanes) --s.nlanes;            // (a lane holds whole rows: all sub-sequences of a row of a split plan)
    s.u16 = u16_layout<T>(s.N1, cols_per_tile<T>(), s.E);
    // the unit layout orders the field between the two kernels by N2 / Ef (k_time's Qf): rows of k_freq<FM_FLY> with another number of points per
    // thread would pair every spectrum bin with another bin's operator (SSFM_EF_FLY != Ef: tests/test_fft_edges_gpu.py, part C) -- such plans keep Ef
    if (s.u16) s.Ef_fly = s.Ef;
    s.small = small_supported<T>((int)s.n) && !(kn.small && *kn.small == 0);
    return s;
}

// ----------------------------------------------------------------------------- a fixed-step run
// The plan's switches as they stand when the run is asked for.  has_twA: the plan holds the factor twiddles; medium_shape: ssfm_medium.hpp medium_shape(N1, N2);
// has_run_e0: the events lane_health brackets a run with exist
struct FixedState { bool medium_ok, medium_split_ok, phase_tables, force_fly, profiling, tracing, op_flat_re, has_twA, medium_shape; int lanes_active; bool has_run_e0; };
// fits_tables: Schedule::fits_tables(), at most kMaxTables distinct step sizes; snapshots: the field after every step is asked for; capture: the run is propagate_fixed_capture's
struct FixedRequest { int64_t nsteps; bool fits_tables, snapshots, capture; };
struct FixedRoute {
    // what ssfm_last_run_info reports -- `engine_in_blocks` for a snapshot run whose capture does not fit the device as a whole (the every-step loop), else `engine`
    int engine = SSFM_ENGINE_NONE, engine_in_blocks = SSFM_ENGINE_NONE;
    bool use_tables = false, use_phase = false, small_sched = false, go_small = false, go_medium = false, health = false;
};
template <typename T> FixedRoute fixed_route(const PlanShape& p, const FixedState& s, const FixedRequest& q) {
    FixedRoute r;
    const bool split = p.split_R > 1, int_steps = q.nsteps <= 0x7fffffff;
    r.use_tables = q.fits_tables && !s.force_fly;
    r.small_sched = p.small && r.use_tables && !s.profiling && int_steps;
    // a fibre's operator has one modulus for all frequencies: 4-byte phase tables (ssfm_kernels.hpp FM_PHASE)
    // (complex128: float64 turn fractions, 8 instead of 16 bytes per frequency -- measured -2.5 % at 2^20 x 2 (39.5 against 40.5 us per step) and
    // +5 % at 2^16 x 2, where nothing hides the float64 sincos: from 2^20 samples in all)
    r.use_phase = r.use_tables && s.phase_tables && s.op_flat_re && (sizeof(T) == 8 ? p.n * p.batch >= (1ll << 20) && !split : p.u16);      // (split plans: 4-byte phases in complex64)
    // plans of 2^12 ... 2^17 samples in the unit layout: the whole schedule in one launch on one XCD (ssfm_kernels.hpp k_medium).  Measured against the
    // one-workgroup-per-row kernel of the small plans (k_small): 5.4 against 6.4 us per step at 8192 samples, 5.6 against 3.5 at 4096 -- so from 8192 on
    const bool rows_split = medium_rows_split(s.medium_split_ok, p.n, p.batch);
    const long long med_blocks = (long long)(p.N2 / cols_per_tile<T>()) * (rows_split ? 1 : p.batch);
    const long long med_samples = rows_split ? p.n : p.n * p.batch;
    const bool med_elig = s.medium_ok && sizeof(T) == 4 && p.u16 && p.E == 8 && p.Ef == 8 && s.medium_shape && r.use_tables && !s.profiling
                           && !q.snapshots && s.has_twA && q.nsteps >= 2 && int_steps
                           && med_blocks % kBarShards == 0 && med_blocks <= 64 && med_samples <= medium_max_samples && (r.use_phase || !s.phase_tables || !s.op_flat_re);
    r.go_small = r.small_sched && !q.snapshots && !(med_elig && p.n >= 8192) && !q.capture;      // (a capture run: the two-kernel engine)
    r.go_medium = med_elig && !r.go_small && !q.capture;
    r.engine_in_blocks = split ? SSFM_ENGINE_SPLIT : SSFM_ENGINE_TWO_KERNEL;
    r.engine = (r.go_small || (r.small_sched && q.snapshots)) ? SSFM_ENGINE_SMALL : r.go_medium ? SSFM_ENGINE_MEDIUM : r.engine_in_blocks;
    r.health = !q.snapshots && !r.go_small && !r.go_medium && s.lanes_active > 1 && !s.profiling && !s.tracing && q.nsteps >= 64 && s.has_run_e0 && !q.capture;
    return r;
}

// ----------------------------------------------------------------------------- an adaptive run
struct AdaptSwitches { bool medium_ok, medium_adapt_ok, fused_ok, has_twA, medium_shape; };
// What ssfm_adaptive_begin does: nothing yet (the first ssfm_adaptive_run decides between the one launch and the chunked engine), or the chunked engine's begin
enum AdaptBegin { ADAPT_CHUNKED = 0, ADAPT_DEFER_SMALL = 1, ADAPT_DEFER_MEDIUM = 2 };
template <typename T> AdaptBegin adaptive_route(const PlanShape& p, const AdaptSwitches& s, bool capture, bool single_step) {
    // (4096 x 2: the one-XCD engine, 8.1 us per step, before the one-workgroup kernel that holds both rows, 10.4)
    const long long blocks = (long long)(p.N2 / cols_per_tile<T>()) * p.batch;
    const bool med_adapt = sizeof(T) == 4 && s.medium_ok && s.medium_adapt_ok && s.fused_ok && !capture && !single_step && p.u16 && p.E == 8 && p.Ef == 8 && p.Ef_fly == 8
                           && s.medium_shape && s.has_twA && blocks % kBarShards == 0 && blocks <= kBarWords && p.n * p.batch <= medium_max_samples;
    if (p.small && !capture && small_adapt_supported<T>((int)p.n, p.batch) && !(med_adapt && p.n == 4096 && p.batch == 2)) return ADAPT_DEFER_SMALL;
    return med_adapt ? ADAPT_DEFER_MEDIUM : ADAPT_CHUNKED;
}
// a deferred run becomes one launch when the first ssfm_adaptive_run's budget covers it; a caller that takes the run in pieces gets the chunked engine
constexpr bool adaptive_one_launch(AdaptBegin b, int64_t budget, int max_steps) { return b != ADAPT_CHUNKED && budget >= (int64_t)max_steps; }
// The chunked engine's column pass
// fused: END + BEGIN in one launch that waits for the global maximum inside (TM_MID_A), two launches per step; tile_private: the field between END and BEGIN stays in the Y buffer
struct AdaptPiece { bool fused = false, tile_private = false; };
template <typename T> constexpr long long adaptive_col_blocks(const PlanShape& p) { return (long long)(p.N2 / cols_per_tile<T>()) * p.batch; }
// `cus`: the device's CU count, <= 0 where the query failed (only looked at for grids of more than kAdaptSlots workgroups)
template <typename T> AdaptPiece adaptive_piece(const PlanShape& p, bool fused_ok, bool capture, int cus) {
    // a column kernel of at most 64 workgroups (measured: a gain up to there, profiles/r02_medium_adaptive.txt) waits for the global maximum inside the launch (TM_MID_A); the input is kept
    // for the case that the GPU does not run the grid as a whole (then: the three-launch engine, for good)
    // Larger complex64 grids (up to 512 workgroups = two per CU: 2^20 x 2) take the same kernel with a hand-over that has no counter to
    // serialise on (AdaptState::wgmax): the column pass is then ONE launch per step instead of two -- 64 MiB of field traffic per step
    // instead of 96.
    const long long col_blocks = adaptive_col_blocks<T>(p);
    long long fused_max = sizeof(T) == 4 ? kAdaptWords : kAdaptSlots;
    if (col_blocks > kAdaptSlots && (cus <= 0 || col_blocks > 2ll * cus || col_blocks % 64 != 0))
        fused_max = kAdaptSlots;                              // (the whole grid must be resident at once: two workgroups per CU)
    const bool fused = fused_ok && !capture && (p.N1 == 128 || p.N1 == 256) && col_blocks <= fused_max && p.split_R == 1;
    // (Two engines that drove the polarisations of an adaptive run on two streams, a lane's kernel waiting INSIDE the launch for the other lane's
    // maxima, were built in round 3 and removed in round 4: both lost their A/B -- 36-38 and 28.9-29.7 against 32-33 and 29.6-31.1 us per step at
    // 2^20 x 2, profiles/r03_adaptive_two_lanes.txt, r03_adaptive_fused_large.txt -- and both stall until their patience runs out whenever the
    // runtime maps the plan's two streams to ONE hardware queue, which it does when the number of live streams of the priority class is 3 mod 4:
    // profiles/r04_order_dependence.txt.)
    // U16 plans keep the time-domain field between END and the next BEGIN in the Y buffer, in tile-private 16-byte
    // units (ssfm_kernels.hpp TM_END_Y / TM_BEGIN_Y); a z-resolved capture needs the time-order field after every
    // step and uses the plain modes
    return {fused, p.u16 && !capture && !fused};
}
// a fused run whose first ssfm_adaptive_run does not cover it: a caller that takes the run in pieces gets the three-launch engine (the fused kernel's
// launches are queued a whole run ahead); the field itself stays in the tile-private order until ssfm_adaptive_finish (include/ssfm_amd.h)
inline AdaptPiece adaptive_in_pieces(AdaptPiece a, const PlanShape& p, int step, int64_t budget, int max_steps) {
    if (a.fused && step == 0 && budget < (int64_t)max_steps) { a.fused = false; a.tile_private = p.u16; }
    return a;
}
constexpr int adaptive_engine(const PlanShape& p, bool fused) { return p.split_R > 1 ? SSFM_ENGINE_SPLIT_ADAPT : fused ? SSFM_ENGINE_ADAPT_FUSED : SSFM_ENGINE_ADAPT_3; }
constexpr int adaptive_engine(AdaptBegin one_launch) { return one_launch == ADAPT_DEFER_MEDIUM ? SSFM_ENGINE_MEDIUM_ADAPT : SSFM_ENGINE_SMALL_ADAPT; }
}  // namespace ssfm
