// sos_route.hpp -- which workgroup shape and which form a call of the zero-phase SOS filter takes (sos_filter.hip), as pure functions of plain values.
// Plain C++ -- no HIP types, no environment, no allocation -- so that a host program can hold them to a restatement of the dispatcher they replace
// (tests/sos_route_host.cpp, tests/test_sos_route_cpu.py).  sos_filter.hip reads the knobs, asks here, and switches to the kernel instance.
// `Coefs` is any struct with the arrays b0, b1, b2, a1, a2 (sos_filter.hip's SosCoefs is a kernel argument: its name is part of the kernels' symbols and stays there).
#pragma once
#include <cmath>

namespace ssfm {
namespace sos {

// ----------------------------------------------------------------------------- the constants: the one copy
#ifndef SOS_CHUNK
#define SOS_CHUNK 12
#endif
// Samples per thread.  Two lengths (profiles/r03_sosfilt.txt, section 11): SOS_CHUNK for the three-launch form and for short calls
// (first version: 16 -> 121 us, 32 -> 130 us, 64 -> 158 us per call at 2^20 x 2 complex; later 8 -> 101, 12 -> 90, 16 -> 97; 12 is 4-14 %
// faster than 16 for every shape from 2^14 to 2^20 x 2), kChunkLong for the one-launch form of long calls: fewer threads pay the
// per-chunk scan and look-back, two workgroups per CU instead of three hold the same samples (2^20 x 2 complex128: 47.5 -> 39.8 us,
// 2^20 real 33.0 -> 25.3; short calls lose 10-20 % with it).
constexpr int kChunkShort = SOS_CHUNK;
constexpr int kChunkLong = 18;
constexpr int kWave = 64;          // lanes per wavefront
#ifndef SOS_WAVES
#define SOS_WAVES 4
#endif
// Wavefronts per workgroup W (a template parameter of the kernels; chunks per group = threads per workgroup = 64 W).
// Measured, kernels per call (profiles/r02_sosfilt_shape.txt): 2^20 x 2 complex 87 us with 4, 95 with 2, 88.5 with 3
// (first version: 1 -> 131 us); 2^20 real 45 / 48-50 / 43; but the short calls of a 2^14 ... 2^16-sample link, which
// are a latency chain of four small kernels, run 11-12 % faster with 2 (2^16 real 32.3 -> 28.5 us, 2^14 complex 38.1 ->
// 34.0): `small_call_waves()` picks the small shape up to kSmallChunks chunks in all, SOS_WAVES above.
// Round 6: the small shape is ONE wavefront (SOS_WAVES_SMALL) and is taken wherever its grid is resident at once -- with the look-back near
// (sos_filter_impl.inc group_start_near) a smaller group costs nothing and has no carry between wavefronts: 4-15 % under two wavefronts from 2^14 to
// 2^20 samples (profiles/r06_sos_w1.txt), 15-25 % under the shapes round 5 chose for 2^17 ... 2^20 (profiles/r06_sos_shape_sweep.txt).  Asking the
// compiler for three wavefronts per SIMD so that 2^20 x 2 complex128 fits too (SOS_SMALL_EU=3): no gain there, 2-4 us lost at 2^18 x 2 -- stays 1.
constexpr int kWavesLarge = SOS_WAVES;
#ifndef SOS_WAVES_SMALL
#define SOS_WAVES_SMALL 1
#endif
constexpr int kWavesSmall = SOS_WAVES_SMALL;
constexpr long long kSmallChunks = 16384;
constexpr int kMaxSections = 4;    // Bessel orders up to 8
constexpr int kLookIter = 2;       // a workgroup looks back over at most kLookIter x (its threads) groups: the one-launch form's limit on groups per row
constexpr int kNear = 4;           // ... unless a group's start state is made of its nearest totals alone: at most this many (sos_filter_impl.inc group_start_near)
constexpr int kNearCertain = 4;    // the same depth where the poles alone have to promise it (near_is_certain)
constexpr int kMaxGiveUps = 3, kRestCalls = 1000;      // calls in a row that waited in vain before the one-launch form rests; calls it rests for

// ----------------------------------------------------------------------------- the knobs, as sos_filter.hip reads them for every call
struct Knobs {
    bool one_launch = true;        // SSFM_SOS_ONE_LAUNCH=0: always three launches
    bool near = true;              // SSFM_SOS_NEAR=0: a group's start state from ALL the earlier totals of its row
    bool meet = false;             // SSFM_SOS_MEET=1: one meeting of the workgroups per call instead of two
    bool long_chunk = true;        // SSFM_SOS_LONG_CHUNK=0: never the long chunk
    int waves_force = 0;           // SOS_WAVES_FORCE (test aid): 0 = not set; a value that is neither shape pins none, yet still keeps the dispatcher off the one-wavefront tries
    long long patience = 200000;   // SSFM_SOS_PATIENCE_US in 10 ns ticks: how long a workgroup waits for a total before it gives the call up
};

// ----------------------------------------------------------------------------- geometry: the one copy of the m / nchunks / ngroups arithmetic
struct Geometry { long long m, nchunks, ngroups; };          // padded row length, chunks per row, groups (= workgroups) per row
constexpr Geometry geometry(long long n, int edge, int chunk, int W) {
    const long long m = n + 2ll * edge, nchunks = (m + chunk - 1) / chunk;
    return Geometry{m, nchunks, (nchunks + kWave * W - 1) / (kWave * W)};
}
// what no form takes, in the order a call is refused
enum Refusal { kFits = 0, kTooLong, kTooManyGroups, kTooManyWorkgroups };
constexpr Refusal refusal(const Geometry& g, int rows) {
    if (g.nchunks > (1ll << 30)) return kTooLong;
    if (g.ngroups > kWave * kWave) return kTooManyGroups;                 // (the third table level ends there)
    if (g.ngroups * rows > 0x7fffffffll) return kTooManyWorkgroups;
    return kFits;
}

// A sufficient condition, from the cascade's poles alone, for the powers of the map over `len` samples to be negligible within kNearCertain groups (the
// kernels' own test is on the matrices the host builds, look_of_group_powers; this one lets the dispatcher choose a shape before any table exists): the largest
// pole modulus r has r^(len * kNearCertain) < 1e-60 -- twenty orders below the kernels' threshold for whatever the transient in front of the decay is.
template <class Coefs> bool near_is_certain(const Coefs& c, int ns, long long len, bool near_enabled) {
    if (!near_enabled) return false;
    double r2 = 0.0;
    for (int s = 0; s < ns; ++s) {
        const double a1 = c.a1[s], a2 = c.a2[s], disc = a1 * a1 - 4.0 * a2;
        double m2;
        if (disc < 0.0) m2 = a2;                                             // a complex pair: |z|^2 = a2
        else { const double z = 0.5 * (std::fabs(a1) + std::sqrt(disc)); m2 = z * z; }
        r2 = m2 > r2 ? m2 : r2;
    }
    if (!(r2 < 1.0)) return false;
    return 0.5 * std::log(r2) * (double)len * kNearCertain < -138.2;          // ln 1e-60
}

// How many powers of the group map matter (group_start_near): 1 + the last d <= 64 whose (M^group)^d has an element at or above 1e-40 (or not a number).
// `pwG`: the second level of the tables, [65][K * K].
inline int look_of_group_powers(const double* pwG, int K) {
    int look = 1;
    for (int d = 1; d <= kWave; ++d) {
        const double* P = pwG + (long long)d * K * K;
        double big = 0.0;
        for (int e = 0; e < K * K; ++e) big = std::fabs(P[e]) > big || P[e] != P[e] ? std::fabs(P[e]) : big;
        if (!(big < 1e-40)) look = d + 1;
    }
    return look;
}

// ----------------------------------------------------------------------------- the give-up state: calls IN A ROW that fell back to three launches after waiting in vain
struct GiveUps { int give_ups = 0, rested = 0; };       // from kMaxGiveUps on the form rests, for kRestCalls calls, then gets another try
// The tick before a call's form is decided.  It comes AFTER the call's shape was chosen (choose_shape saw give_ups == kMaxGiveUps): the call that ends a rest
// tries one launch in the shape the dispatcher falls back to, not in the one it would pick for a form it expects to run.  Kept as it was, on purpose.
constexpr GiveUps tick_before_form(GiveUps s) {
    if (s.give_ups >= kMaxGiveUps && ++s.rested >= kRestCalls) { s.give_ups = kMaxGiveUps - 1; s.rested = 0; }
    return s;
}
// ... and after a call that tried one launch (a call that went straight to three launches leaves the state alone)
constexpr GiveUps after_one_launch(GiveUps s, bool gave_up) {
    s.give_ups = gave_up ? s.give_ups + 1 : 0;
    return s;
}

// ----------------------------------------------------------------------------- the shape: chunk length and wavefronts per workgroup
struct Shape { int chunk, W; };
// the workgroup shape of short calls (in whatever form) and of the test aid
constexpr int small_call_waves(long long n, int rows, int edge, const Knobs& kn) {
    if (kn.waves_force == kWavesSmall || kn.waves_force == kWavesLarge) return kn.waves_force;
    return geometry(n, edge, kChunkShort, 1).nchunks * rows <= kSmallChunks ? kWavesSmall : kWavesLarge;
}
// Would a call take the one-launch form in this shape, as far as its poles tell?  (Rows of more than kLookIter x threads groups: only when a group's start
// state needs its nearest totals alone.)  `capacity(chunk, W)`: workgroups of that instance the device holds at once; asked last, and only if all else holds.
template <class Coefs, class Cap>
bool one_launch_expected(Shape s, const Coefs& c, int ns, int ch, long long n, int rows, int edge, const Knobs& kn, int give_ups, Cap&& capacity) {
    const long long group = kWave * s.W, ngroups = geometry(n, edge, s.chunk, s.W).ngroups;
    const bool groups_ok = ngroups <= kLookIter * group || (ch * 2 * ns <= 8 && ngroups <= kWave * kWave && near_is_certain(c, ns, group * s.chunk, kn.near));
    return kn.one_launch && give_ups < kMaxGiveUps && groups_ok && ngroups * rows <= capacity(s.chunk, s.W);
}
// Which shape a call takes (round 6; profiles/r06_sos_shape_sweep.txt, r06_sos_w1.txt -- orders 2 to 8, 8192 ... 2^20 samples, three layouts):
//  1. ONE wavefront per workgroup, short chunk, wherever that grid is resident at once: with the look-back near (group_start_near) a small group costs nothing and has no
//     carry between wavefronts -- the best shape or within 4 % of it everywhere it fits (2^20 float64 15.3 us against 17.7 in four wavefronts of the long chunk);
//  2. one wavefront with the LONG chunk where only that fits (1.5 ... 2.1 M complex samples: 22.5 against 25.4 us at 786 432 x 2);
//  3. four wavefronts of the short chunk while that is at most one workgroup per CU (orders 4 to 8: 15.5 / 34 / 42 us against the long chunk's 17 / 37 / 45);
//  4. four wavefronts of the long chunk (two workgroups per CU hold what three of the short one would); 5. the short chunk in three launches.
// SOS_WAVES_FORCE pins the wavefronts, SSFM_SOS_LONG_CHUNK=0 the short chunk.  `cus`: the device's compute units, 0 if unknown.
template <class Coefs, class Cap>
Shape choose_shape(const Coefs& c, int ns, int ch, long long n, int rows, int edge, const Knobs& kn, int give_ups, int cus, Cap&& capacity) {
    const auto fits = [&](Shape s) { return one_launch_expected(s, c, ns, ch, n, rows, edge, kn, give_ups, capacity); };
    const Shape small_short{kChunkShort, kWavesSmall}, small_long{kChunkLong, kWavesSmall}, large_short{kChunkShort, kWavesLarge}, large_long{kChunkLong, kWavesLarge};
    if (kWavesSmall != kWavesLarge) {
        if (small_call_waves(n, rows, edge, kn) == kWavesSmall) return small_short;
        if (kn.waves_force == 0) {
            if (fits(small_short)) return small_short;
            if (kn.long_chunk && fits(small_long)) return small_long;
            if (kn.long_chunk && cus > 0 && geometry(n, edge, kChunkShort, kWavesLarge).ngroups * rows <= cus && fits(large_short)) return large_short;
        }
    }
    if (kn.long_chunk && fits(large_long)) return large_long;
    return large_short;
}

// ----------------------------------------------------------------------------- the form: one launch or three, and what the one launch meets with
struct Form {
    int launches = 3;
    int look = 0;              // SosLink::look: > 0: a group's start state from its `look` nearest totals; 0: from all of them
    bool tagged = false;       // the totals cross as {value, tag} units (at most 8 doubles per total)
    bool meet = false;         // the single-meeting kernel
};
// `look`: measured on the tables of this filter and shape (look_of_group_powers); `capacity_meet`: capacity of the single-meeting instance, asked only where it would run.
template <class Cap, class CapMeet>
Form choose_form(Shape s, const Geometry& g, int ns, int ch, int rows, const Knobs& kn, int give_ups, int look, Cap&& capacity, CapMeet&& capacity_meet) {
    const bool tagged = ch * 2 * ns <= 8, near_now = tagged && kn.near && look <= kNear;
    const long long grid = g.ngroups * rows;
    Form f;
    if (!(kn.one_launch && give_ups < kMaxGiveUps && (g.ngroups <= kLookIter * kWave * s.W || near_now) && grid <= capacity(s.chunk, s.W))) return f;
    f.launches = 1;
    f.look = near_now ? look : 0;
    f.tagged = tagged;
    f.meet = tagged && kn.meet && f.look >= 1 && f.look <= 2 && grid <= capacity_meet(s.chunk, s.W);
    return f;
}

// what ssfm_sosfiltfilt_last_route reports: wavefronts, chunk, launches, look, tagged, meeting, sections, channels
inline void fill_route(int (&route)[8], Shape s, const Form& f, int ns, int ch) {
    const int r[8] = {s.W, s.chunk, f.launches, f.look, f.tagged, f.meet, ns, ch};
    for (int i = 0; i < 8; ++i) route[i] = r[i];
}

}  // namespace sos
}  // namespace ssfm
