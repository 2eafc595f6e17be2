// Host program of tests/test_route_cpu.py: the shape of a plan and the routes of its entry points (opticomlib_amd/csrc/ssfm_route.hpp) against tables and
// restatements typed from init / propagate_fixed / adaptive_begin / adaptive_begin_chunked / adaptive_run as they stood before the header existed.  Built with
// AddressSanitizer / UBSan; no GPU.  Prints "ok: <cells checked>", exits non-zero on any miss.
#include "ssfm_route.hpp"

#include <cstdint>
#include <cstdio>

using namespace ssfm;

static long long failures = 0, checked = 0;
#define CHECK(cond, ...) do { ++checked; if (!(cond)) { if (++failures <= 40) { std::printf("FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

// ----------------------------------------------------------------------------- shapes, default knobs: every power of two, batch 1, 2, 4, 16
struct ShapeRow { int log2n, split_R, sub_log2n, N1, N2, E, Ef, Ef_fly; bool u16, small; int lanes[4]; };       // lanes at batch 1, 2, 4, 16
static const int kBatches[4] = {1, 2, 4, 16};
static const ShapeRow kC64[] = {
    {8, 1, 8, 16, 16, 8, 8, 8, false, true, {1, 1, 1, 1}},
    {9, 1, 9, 16, 32, 8, 8, 8, false, true, {1, 1, 1, 1}},               // N1 / E = 2 < 4: the plain layout
    {10, 1, 10, 32, 32, 8, 8, 8, true, true, {1, 1, 1, 1}},
    {11, 1, 11, 32, 64, 8, 8, 8, true, true, {1, 1, 1, 1}},
    {12, 1, 12, 64, 64, 8, 8, 8, true, true, {1, 1, 1, 1}},
    {13, 1, 13, 64, 128, 8, 8, 8, true, true, {1, 1, 1, 1}},             // 2^13 x 2: one lane, small
    {14, 1, 14, 128, 128, 8, 8, 8, true, false, {1, 1, 1, 1}},
    {15, 1, 15, 128, 256, 8, 8, 8, true, false, {1, 1, 1, 1}},
    {16, 1, 16, 256, 256, 8, 8, 8, true, false, {1, 1, 1, 2}},
    {17, 1, 17, 256, 512, 8, 8, 8, true, false, {1, 1, 1, 2}},
    {18, 1, 18, 256, 1024, 16, 16, 16, true, false, {1, 1, 2, 2}},
    {19, 1, 19, 256, 2048, 16, 16, 16, true, false, {1, 2, 2, 2}},
    {20, 1, 20, 256, 4096, 16, 16, 16, true, false, {1, 2, 2, 2}},       // 2^20 x 2: two lanes
    {21, 1, 21, 512, 4096, 16, 16, 16, true, false, {1, 2, 2, 2}},
    {22, 1, 22, 512, 8192, 16, 16, 16, true, false, {1, 2, 2, 2}},
    {23, 8, 20, 256, 4096, 16, 16, 16, true, false, {1, 2, 2, 2}},       // 2^23 x 2: split_R 8, sub-plan 2^20 x 16, two lanes
    {24, 16, 20, 256, 4096, 16, 16, 16, true, false, {1, 2, 2, 2}},      // 2^24 x 1: split_R 16, sub-plan 2^20 x 16, one lane
};
static const ShapeRow kC128[] = {
    {8, 1, 8, 16, 16, 8, 8, 8, false, true, {1, 1, 1, 1}},
    {9, 1, 9, 16, 32, 8, 8, 8, false, true, {1, 1, 1, 1}},
    {10, 1, 10, 32, 32, 8, 8, 8, false, true, {1, 1, 1, 1}},
    {11, 1, 11, 32, 64, 8, 8, 8, false, true, {1, 1, 1, 1}},
    {12, 1, 12, 64, 64, 8, 8, 8, false, true, {1, 1, 1, 1}},
    {13, 1, 13, 64, 128, 8, 8, 8, false, false, {1, 1, 1, 1}},
    {14, 1, 14, 128, 128, 8, 8, 8, false, false, {1, 1, 1, 1}},
    {15, 1, 15, 128, 256, 8, 8, 8, false, false, {1, 1, 1, 1}},
    {16, 1, 16, 256, 256, 8, 8, 8, false, false, {1, 1, 1, 2}},
    {17, 1, 17, 256, 512, 8, 8, 8, false, false, {1, 1, 1, 2}},
    {18, 1, 18, 256, 1024, 8, 16, 8, false, false, {1, 1, 2, 2}},
    {19, 1, 19, 256, 2048, 8, 16, 8, false, false, {1, 2, 2, 2}},
    {20, 1, 20, 256, 4096, 8, 16, 8, false, false, {1, 2, 2, 2}},        // 2^20 x 2: 8 / 16 / 8, two lanes
    {21, 1, 21, 512, 4096, 16, 16, 16, false, false, {1, 2, 2, 2}},
    {22, 1, 22, 512, 8192, 16, 16, 16, false, false, {1, 2, 2, 2}},
    {23, 8, 20, 256, 4096, 8, 16, 8, false, false, {1, 2, 2, 2}},
    {24, 16, 20, 256, 4096, 8, 16, 8, false, false, {1, 2, 2, 2}},
};

template <typename T, size_t N> static void check_shapes(const char* prec, const ShapeRow (&rows)[N]) {
    static_assert(N == 17, "2^8 ... 2^24");
    for (const ShapeRow& w : rows)
        for (int b = 0; b < 4; ++b) {
            const PlanShape s = plan_shape<T>(1ll << w.log2n, kBatches[b], ShapeKnobs{});
            CHECK(!s.too_many && s.log2_full == w.log2n && s.split_R == w.split_R && s.n == (1ll << w.sub_log2n) && s.batch == kBatches[b] * w.split_R,
                  "%s 2^%d x %d: split_R %d, sub-plan %lld x %d", prec, w.log2n, kBatches[b], s.split_R, (long long)s.n, s.batch);
            CHECK(s.N1 == w.N1 && s.N2 == w.N2 && s.E == w.E && s.Ef == w.Ef && s.Ef_fly == w.Ef_fly && s.u16 == w.u16 && s.small == w.small,
                  "%s 2^%d x %d: N1 %d N2 %d E %d Ef %d Ef_fly %d u16 %d small %d", prec, w.log2n, kBatches[b], s.N1, s.N2, s.E, s.Ef, s.Ef_fly, (int)s.u16, (int)s.small);
            CHECK(s.nlanes == w.lanes[b], "%s 2^%d x %d: %d lanes, expected %d", prec, w.log2n, kBatches[b], s.nlanes, w.lanes[b]);
        }
}

// ----------------------------------------------------------------------------- knobs: each alone, and the pairs whose precedence init spelled out
template <typename T> static void knob_row(const char* what, int log2n, int batch, const ShapeKnobs& kn, int split_R, int sub_log2n, int E, int Ef, int Ef_fly, bool u16, int lanes, bool small) {
    const PlanShape s = plan_shape<T>(1ll << log2n, batch, kn);
    CHECK(s.split_R == split_R && s.n == (1ll << sub_log2n) && s.E == E && s.Ef == Ef && s.Ef_fly == Ef_fly && s.u16 == u16 && s.nlanes == lanes && s.small == small,
          "%s: split_R %d n %lld E %d Ef %d Ef_fly %d u16 %d lanes %d small %d", what, s.split_R, (long long)s.n, s.E, s.Ef, s.Ef_fly, (int)s.u16, s.nlanes, (int)s.small);
}
static ShapeKnobs knobs() { return ShapeKnobs{}; }
static void check_knobs() {
    ShapeKnobs k;
    k = knobs(); k.e = 8;   knob_row<float>("SSFM_E=8, c64 2^20 x 2", 20, 2, k, 1, 20, 8, 8, 8, true, 2, false);              // then Ef = E
    k = knobs(); k.e = 16;  knob_row<float>("SSFM_E=16, c64 2^14 x 2", 14, 2, k, 1, 14, 16, 16, 16, true, 1, false);          // ... also below 2^17
    k = knobs(); k.e = 16;  knob_row<double>("SSFM_E=16, c128 2^20 x 2", 20, 2, k, 1, 20, 16, 16, 16, false, 2, false);       // (and no Ef_fly = 8 rule)
    k = knobs(); k.e = 12;  knob_row<float>("SSFM_E=12 (neither): 8", 20, 2, k, 1, 20, 8, 8, 8, true, 2, false);
    k = knobs(); k.e = 16;  knob_row<float>("SSFM_E=16, c64 2^9: plain layout", 9, 1, k, 1, 9, 16, 16, 16, false, 1, true);
    k = knobs(); k.ef = 8;  knob_row<float>("SSFM_EF=8, c64 2^20 x 2", 20, 2, k, 1, 20, 16, 8, 8, true, 2, false);
    k = knobs(); k.ef = 16; knob_row<float>("SSFM_EF=16, c64 2^14 x 2", 14, 2, k, 1, 14, 8, 16, 16, true, 1, false);
    k = knobs(); k.ef = 16; knob_row<double>("SSFM_EF=16, c128 2^20 x 2: Ef_fly stays", 20, 2, k, 1, 20, 8, 16, 16, false, 2, false);
    k = knobs(); k.ef = 8;  knob_row<double>("SSFM_EF=8, c128 2^20 x 2", 20, 2, k, 1, 20, 8, 8, 8, false, 2, false);
    k = knobs(); k.e = 8; k.ef = 16; knob_row<float>("SSFM_E=8 SSFM_EF=16: EF wins for Ef", 20, 2, k, 1, 20, 8, 16, 16, true, 2, false);
    k = knobs(); k.ef_fly = 8;  knob_row<float>("SSFM_EF_FLY=8 on a u16 plan: ignored", 20, 2, k, 1, 20, 16, 16, 16, true, 2, false);
    k = knobs(); k.ef_fly = 16; knob_row<float>("SSFM_EF_FLY=16 on a u16 plan of 2^14: ignored", 14, 2, k, 1, 14, 8, 8, 8, true, 1, false);
    k = knobs(); k.ef_fly = 16; knob_row<double>("SSFM_EF_FLY=16, c128 2^20 x 2", 20, 2, k, 1, 20, 8, 16, 16, false, 2, false);
    k = knobs(); k.ef_fly = 16; knob_row<double>("SSFM_EF_FLY=16, c128 2^14 x 2", 14, 2, k, 1, 14, 8, 8, 16, false, 1, false);
    k = knobs(); k.ef_fly = 8;  knob_row<float>("SSFM_EF_FLY=8, c64 2^9 (plain layout)", 9, 1, k, 1, 9, 8, 8, 8, false, 1, true);
    k = knobs(); k.ef_fly = 16; knob_row<float>("SSFM_EF_FLY=16, c64 2^9 (plain layout)", 9, 1, k, 1, 9, 8, 8, 16, false, 1, true);
    k = knobs(); k.e = 8; k.ef = 8; k.ef_fly = 8;      // everything above 2^20: 16 regardless
    knob_row<float>("all 8, c64 2^21", 21, 1, k, 1, 21, 16, 16, 16, true, 1, false);
    knob_row<double>("all 8, c128 2^22", 22, 2, k, 1, 22, 16, 16, 16, false, 2, false);
    knob_row<double>("all 8, c128 2^20", 20, 2, k, 1, 20, 8, 8, 8, false, 2, false);
    k = knobs(); k.split_above = 20;
    knob_row<float>("SSFM_SPLIT_ABOVE=20 at 2^21", 21, 1, k, 2, 20, 16, 16, 16, true, 1, false);
    knob_row<float>("SSFM_SPLIT_ABOVE=20 at 2^22", 22, 1, k, 4, 20, 16, 16, 16, true, 1, false);
    knob_row<float>("SSFM_SPLIT_ABOVE=20 at 2^20", 20, 1, k, 1, 20, 16, 16, 16, true, 1, false);
    knob_row<double>("SSFM_SPLIT_ABOVE=20 at 2^21 x 2, c128", 21, 2, k, 2, 20, 8, 16, 8, false, 2, false);
    k = knobs(); k.split_above = 19; knob_row<float>("SSFM_SPLIT_ABOVE=19: out of range", 21, 1, k, 1, 21, 16, 16, 16, true, 1, false);
    k = knobs(); k.split_above = 22; knob_row<float>("SSFM_SPLIT_ABOVE=22: out of range", 23, 1, k, 8, 20, 16, 16, 16, true, 1, false);
    k = knobs(); k.split_log2m = 21; knob_row<float>("SSFM_SPLIT_LOG2M=21 at 2^24", 24, 1, k, 8, 21, 16, 16, 16, true, 1, false);
    k = knobs(); k.split_log2m = 22; knob_row<float>("SSFM_SPLIT_LOG2M=22 at 2^23", 23, 1, k, 2, 22, 16, 16, 16, true, 1, false);
    k = knobs(); k.split_log2m = 19; knob_row<float>("SSFM_SPLIT_LOG2M=19: out of range", 23, 1, k, 8, 20, 16, 16, 16, true, 1, false);
    k = knobs(); k.split_above = 20; k.split_log2m = 21; knob_row<float>("SSFM_SPLIT_LOG2M=21 at 2^21: one below the row", 21, 1, k, 2, 20, 16, 16, 16, true, 1, false);
    // SSFM_LANES of 0, 1, 2, 3 and 9 against batch 1, 2, 4 and 6 (2^14: the size rule asks for one lane)
    static const int asked[5] = {0, 1, 2, 3, 9}, rows[4] = {1, 2, 4, 6};
    static const int lanes[5][4] = {{1, 1, 1, 1}, {1, 1, 1, 1}, {1, 2, 2, 2}, {1, 2, 2, 3}, {1, 2, 4, 6}};
    for (int a = 0; a < 5; ++a)
        for (int b = 0; b < 4; ++b) {
            k = knobs(); k.lanes = asked[a];
            const PlanShape s = plan_shape<float>(1ll << 14, rows[b], k);
            CHECK(s.nlanes == lanes[a][b] && s.lanes_wanted == asked[a], "SSFM_LANES=%d, %d rows: %d lanes (wanted %d)", asked[a], rows[b], s.nlanes, s.lanes_wanted);
        }
    k = knobs(); k.lanes = 1; knob_row<float>("SSFM_LANES=1, c64 2^20 x 2", 20, 2, k, 1, 20, 16, 16, 16, true, 1, false);
    k = knobs(); k.lanes = 2; knob_row<float>("SSFM_LANES=2 on a split plan of 2^23 x 3: whole rows", 23, 3, k, 8, 20, 16, 16, 16, true, 1, false);
    k = knobs(); k.small = 0; knob_row<float>("SSFM_SMALL=0", 10, 1, k, 1, 10, 8, 8, 8, true, 1, false);
    k = knobs(); k.small = 1; knob_row<float>("SSFM_SMALL=1", 10, 1, k, 1, 10, 8, 8, 8, true, 1, true);
    k = knobs(); k.small = 1; knob_row<float>("SSFM_SMALL=1 where there is no such engine", 14, 1, k, 1, 14, 8, 8, 8, true, 1, false);
    // batch * split_R > 65535 is the error
    CHECK(plan_shape<float>(1ll << 24, 4096, knobs()).too_many, "2^24 x 4096: 65536 sub-sequences");
    CHECK(!plan_shape<float>(1ll << 24, 4095, knobs()).too_many && plan_shape<float>(1ll << 24, 4095, knobs()).batch == 65520, "2^24 x 4095");
    CHECK(plan_shape<double>(1ll << 23, 8192, knobs()).too_many && !plan_shape<double>(1ll << 22, 65535, knobs()).too_many, "2^23 x 8192; 2^22 x 65535 is no split plan");
}

// ----------------------------------------------------------------------------- the predicates
static void check_predicates() {
    static_assert(kLog2MaxDirect == 22 && kMaxTables == 4 && kSmallE16Min == 4096 && kSplitLog2M == 20 && kSplitMaxR == 16 && kAdaptSlots == 64 && kAdaptWords == 512
                  && kBarShards == 8 && kBarWords == 64 && medium_max_samples == 131072 && kMaxLanes == 8 && cols_per_tile<float>() == 16 && cols_per_tile<double>() == 8, "");
    static_assert(small_points<float>(2048) == 8 && small_points<float>(4096) == 16 && small_points<double>(4096) == 8, "");
    static_assert(!small_supported<float>(128) && small_supported<float>(256) && small_supported<float>(8192) && !small_supported<float>(16384) && !small_supported<float>(3000), "");
    static_assert(small_supported<double>(4096) && !small_supported<double>(8192), "");
    static_assert(small_adapt_supported<float>(4096, 2) && !small_adapt_supported<float>(8192, 1) && !small_adapt_supported<float>(2048, 3) && small_adapt_supported<double>(2048, 2)
                  && !small_adapt_supported<double>(4096, 2) && small_adapt_supported<double>(4096, 1) && !small_adapt_supported<float>(256, 0), "");
    static_assert(line_half_shape(256, 1024, 8, 16) && line_half_shape(512, 8192, 16, 16) && !line_half_shape(256, 512, 8, 16) && !line_half_shape(256, 1024, 16, 16) && !line_half_shape(256, 1024, 8, 8), "");
    static_assert(u16_layout<float>(32, 16, 8) && !u16_layout<float>(16, 16, 8) && !u16_layout<double>(256, 8, 8) && !u16_layout<float>(256, 8, 16) && !u16_layout<float>(96, 16, 16), "");
    static_assert(medium_rows_split(true, 65536, 2) && !medium_rows_split(false, 65536, 2) && !medium_rows_split(true, 32768, 2) && !medium_rows_split(true, 65536, 4), "");
    ++checked;
}

// ----------------------------------------------------------------------------- a fixed-step run, as propagate_fixed decided it line by line
struct PlanSwitches { bool medium_ok, medium_split_ok, phase_tables, force_fly, profiling, tracing, op_flat_re, twA, medium_shape_N1_N2; int lanes_active; bool run_e0; };
template <typename T> static void check_fixed_cell(const PlanShape& p, const PlanSwitches& w, int64_t nsteps, bool fits_tables, bool snapshots, bool cap_run) {
    const int64_t n = p.n; const int batch = p.batch, N2 = p.N2, E = p.E, Ef = p.Ef; const bool u16 = p.u16, small = p.small, is_split = p.split_R > 1;
    // (the names below are propagate_fixed's)
    const bool use_tables = fits_tables && !w.force_fly;
    const bool small_sched = small && use_tables && !w.profiling && nsteps <= 0x7fffffff;
    bool use_phase = use_tables && w.phase_tables && w.op_flat_re;
    if (sizeof(T) == 8) use_phase = use_phase && n * batch >= (1ll << 20) && !is_split;
    else use_phase = use_phase && u16;
    const bool medium_rows_split_ = w.medium_split_ok && batch == 2 && n >= (1ll << 16);
    const long long med_blocks = (long long)(N2 / (sizeof(T) == 8 ? 8 : 16)) * (medium_rows_split_ ? 1 : batch);
    const long long med_samples = medium_rows_split_ ? n : n * batch;
    bool med_elig = w.medium_ok && sizeof(T) == 4 && u16 && E == 8 && Ef == 8 && w.medium_shape_N1_N2 && use_tables && !w.profiling;
    med_elig = med_elig && !snapshots && w.twA && nsteps >= 2 && nsteps <= 0x7fffffff;
    med_elig = med_elig && med_blocks % 8 == 0 && med_blocks <= 64 && med_samples <= (1ll << 17) && (use_phase || !w.phase_tables || !w.op_flat_re);
    const bool go_small = small_sched && !snapshots && !(med_elig && n >= 8192) && !cap_run;
    const bool go_medium = med_elig && !go_small && !cap_run;
    int last_engine = (go_small || (small_sched && snapshots)) ? SSFM_ENGINE_SMALL : go_medium ? SSFM_ENGINE_MEDIUM : is_split ? SSFM_ENGINE_SPLIT : SSFM_ENGINE_TWO_KERNEL;
    const bool health = !snapshots && !go_small && !go_medium && w.lanes_active > 1 && !w.profiling && !w.tracing && nsteps >= 64 && w.run_e0 && !cap_run;
    // (the snapshot branch, where the capture did not fit one block: `!(small_sched && block == nsteps + 1)`)
    const int in_blocks = is_split ? SSFM_ENGINE_SPLIT : SSFM_ENGINE_TWO_KERNEL;

    const FixedState st = {w.medium_ok, w.medium_split_ok, w.phase_tables, w.force_fly, w.profiling, w.tracing, w.op_flat_re, w.twA, w.medium_shape_N1_N2, w.lanes_active, w.run_e0};
    const FixedRoute r = fixed_route<T>(p, st, FixedRequest{nsteps, fits_tables, snapshots, cap_run});
    CHECK(r.use_tables == use_tables && r.use_phase == use_phase && r.small_sched == small_sched && r.go_small == go_small && r.go_medium == go_medium && r.health == health
              && r.engine == last_engine && r.engine_in_blocks == in_blocks,
          "fixed %zu-byte %lld x %d, %lld steps, switches %d%d%d%d%d%d%d%d%d lanes %d e0 %d, fits %d snap %d cap %d: engine %d (%d), tables %d phase %d small_sched %d go_small %d go_medium %d health %d",
          sizeof(T), (long long)n, batch, (long long)nsteps, w.medium_ok, w.medium_split_ok, w.phase_tables, w.force_fly, w.profiling, w.tracing, w.op_flat_re, w.twA, w.medium_shape_N1_N2,
          w.lanes_active, w.run_e0, fits_tables, snapshots, cap_run, r.engine, last_engine, r.use_tables, r.use_phase, r.small_sched, r.go_small, r.go_medium, r.health);
}
// the shapes of ssfm_medium.hip (kShapes), restated
static bool medium_shape_of(const PlanShape& p) {
    static const int sh[6][2] = {{64, 64}, {64, 128}, {128, 128}, {128, 256}, {256, 256}, {256, 512}};
    for (const auto& s : sh) if (p.N1 == s[0] && p.N2 == s[1]) return true;
    return false;
}
struct RouteShape { int log2n, batch, split_above; };
static const RouteShape kRouteShapes[] = {{8, 1, 0}, {12, 2, 0}, {13, 2, 0}, {14, 2, 0}, {16, 2, 0}, {18, 2, 0}, {20, 2, 0}, {21, 1, 20}, {23, 2, 0}};
template <typename T> static PlanShape shape_of(const RouteShape& rs) {
    ShapeKnobs k;
    if (rs.split_above) k.split_above = rs.split_above;
    return plan_shape<T>(1ll << rs.log2n, rs.batch, k);
}
template <typename T> static void check_fixed() {
    static const int64_t steps[] = {1, 2, 15, 16, 63, 64, (int64_t)0x7fffffff, (int64_t)0x80000000ll};
    for (const RouteShape& rs : kRouteShapes) {
        const PlanShape p = shape_of<T>(rs);
        for (unsigned bits = 0; bits < (1u << 14); ++bits) {
            auto b = [&](int i) { return ((bits >> i) & 1u) != 0; };
            // (bit 8 set: the plan's medium_shape / twA as the shape has them; clear: the opposite, which a plan never has but the rule must still read)
            const PlanSwitches w = {b(0), b(1), b(2), b(3), b(4), b(5), b(6), b(7) ? (p.u16 || sizeof(T) == 8) : !(p.u16 || sizeof(T) == 8), b(8) ? medium_shape_of(p) : !medium_shape_of(p),
                                    b(9) ? 2 : 1, b(10)};
            for (int64_t ns : steps) check_fixed_cell<T>(p, w, ns, b(11), b(12), b(13));
        }
    }
}
// the cells of tests/test_routes_gpu.py, literally
static void check_fixed_anchors() {
    const PlanSwitches fibre = {true, true, true, false, false, false, true, true, true, 1, false};       // a fibre's operator, every switch as a new plan has it
    struct { int log2n, batch, split_above; bool fits, snap, cap; int engine; } rows[] = {
        {8, 1, 0, true, false, false, SSFM_ENGINE_SMALL},         {13, 2, 0, true, false, false, SSFM_ENGINE_MEDIUM},      {14, 2, 0, true, false, false, SSFM_ENGINE_MEDIUM},
        {12, 2, 0, true, false, false, SSFM_ENGINE_SMALL},        {14, 2, 0, false, false, false, SSFM_ENGINE_TWO_KERNEL}, {14, 2, 0, true, true, false, SSFM_ENGINE_TWO_KERNEL},
        {8, 1, 0, true, true, false, SSFM_ENGINE_SMALL},          {21, 1, 20, true, false, false, SSFM_ENGINE_SPLIT},      {14, 2, 0, true, false, true, SSFM_ENGINE_TWO_KERNEL},
        {18, 2, 0, true, false, false, SSFM_ENGINE_TWO_KERNEL},   {16, 2, 0, true, false, false, SSFM_ENGINE_MEDIUM},      {20, 2, 0, true, false, false, SSFM_ENGINE_TWO_KERNEL},
    };
    for (const auto& c : rows) {
        const PlanShape p = shape_of<float>(RouteShape{c.log2n, c.batch, c.split_above});
        PlanSwitches w = fibre;
        w.medium_shape_N1_N2 = medium_shape_of(p); w.lanes_active = p.nlanes;
        const FixedRoute r = fixed_route<float>(p, FixedState{w.medium_ok, w.medium_split_ok, w.phase_tables, w.force_fly, w.profiling, w.tracing, w.op_flat_re, w.twA, w.medium_shape_N1_N2, w.lanes_active, w.run_e0},
                                                FixedRequest{3, c.fits, c.snap, c.cap});
        CHECK(r.engine == c.engine, "c64 2^%d x %d, 3 steps, fits %d snap %d cap %d: engine %d, expected %d", c.log2n, c.batch, c.fits, c.snap, c.cap, r.engine, c.engine);
    }
    // 2^16 x 2 with the rows in one launch (SSFM_MEDIUM_SPLIT=0): 2^17 samples in 32 workgroups still fit; 2^17 x 2 only with the rows split
    PlanSwitches w = fibre;
    w.medium_split_ok = false;
    const PlanShape p16 = shape_of<float>(RouteShape{16, 2, 0}), p17 = shape_of<float>(RouteShape{17, 2, 0});
    auto engine = [&](const PlanShape& p, const PlanSwitches& s) {
        return fixed_route<float>(p, FixedState{s.medium_ok, s.medium_split_ok, s.phase_tables, s.force_fly, s.profiling, s.tracing, s.op_flat_re, s.twA, true, 1, false}, FixedRequest{3, true, false, false}).engine;
    };
    CHECK(engine(p16, w) == SSFM_ENGINE_MEDIUM && engine(p17, w) == SSFM_ENGINE_TWO_KERNEL && engine(p17, fibre) == SSFM_ENGINE_MEDIUM, "medium_split_ok at 2^16 x 2 / 2^17 x 2");
    // complex128 has no one-XCD engine: 2^14 x 2 with one step size is the two-kernel engine with tables
    const FixedRoute c128 = fixed_route<double>(shape_of<double>(RouteShape{14, 2, 0}), FixedState{true, true, true, false, false, false, true, true, true, 1, false}, FixedRequest{3, true, false, false});
    CHECK(c128.engine == SSFM_ENGINE_TWO_KERNEL && c128.use_tables && !c128.use_phase && !c128.go_medium, "complex128 2^14 x 2, 3 steps of one size");
}

// ----------------------------------------------------------------------------- an adaptive run, as adaptive_begin / adaptive_begin_chunked / adaptive_run decided it
template <typename T> static void check_adaptive() {
    static const int cu_counts[] = {256, 0, -1, 64};          // (0 / -1: the query failed)
    const int max_steps = 64;
    for (const RouteShape& rs : kRouteShapes) {
        const PlanShape p = shape_of<T>(rs);
        const int64_t n = p.n; const int batch = p.batch, N1 = p.N1, N2 = p.N2; const bool is_split = p.split_R > 1;
        for (unsigned bits = 0; bits < (1u << 7); ++bits) {
            auto b = [&](int i) { return ((bits >> i) & 1u) != 0; };
            const bool medium_ok = b(0), medium_adapt_ok = b(1), fused_ok = b(2), twA = b(3), mshape = b(4), capture = b(5), single_step = b(6);
            // adaptive_begin
            bool med_adapt = false;
            if (sizeof(T) == 4) {
                const long long blocks = (long long)(N2 / 16) * batch;
                med_adapt = medium_ok && medium_adapt_ok && fused_ok && !capture && !single_step && p.u16 && p.E == 8 && p.Ef == 8 && p.Ef_fly == 8 && mshape;
                med_adapt = med_adapt && twA && blocks % 8 == 0 && blocks <= 64 && n * batch <= (1ll << 17);
            }
            const bool small_adapt = n >= 256 && n <= 4096 && (n & (n - 1)) == 0 && batch >= 1 && batch <= 2 && batch * n / ((sizeof(T) == 4 && n >= 4096) ? 16 : 8) <= 512;
            AdaptBegin want = ADAPT_CHUNKED;
            if (p.small && !capture && small_adapt && !(med_adapt && n == 4096 && batch == 2)) want = ADAPT_DEFER_SMALL;
            else if (med_adapt) want = ADAPT_DEFER_MEDIUM;
            const AdaptBegin got = adaptive_route<T>(p, AdaptSwitches{medium_ok, medium_adapt_ok, fused_ok, twA, mshape}, capture, single_step);
            CHECK(got == want, "adaptive_begin %zu-byte %lld x %d, switches %d%d%d%d%d capture %d single %d: %d, expected %d", sizeof(T), (long long)n, batch, medium_ok, medium_adapt_ok, fused_ok,
                  twA, mshape, capture, single_step, (int)got, (int)want);
            // adaptive_run on a deferred run: one launch where the budget covers the run, else the chunked engine
            for (int64_t budget : {(int64_t)1, (int64_t)max_steps - 1, (int64_t)max_steps, (int64_t)max_steps + 1}) {
                CHECK(adaptive_one_launch(got, budget, max_steps) == (want != ADAPT_CHUNKED && budget >= max_steps), "one launch: route %d, budget %lld", (int)got, (long long)budget);
                CHECK(adaptive_engine(ADAPT_DEFER_SMALL) == SSFM_ENGINE_SMALL_ADAPT && adaptive_engine(ADAPT_DEFER_MEDIUM) == SSFM_ENGINE_MEDIUM_ADAPT, "the one-launch engines' names");
            }
            // adaptive_begin_chunked
            for (int cus : cu_counts) {
                const long long col_blocks = (long long)(N2 / (sizeof(T) == 8 ? 8 : 16)) * batch;
                long long fused_max = sizeof(T) == 4 ? 512 : 64;
                if (col_blocks > 64 && (cus <= 0 || col_blocks > 2ll * cus || col_blocks % 64 != 0)) fused_max = 64;
                const bool fused = fused_ok && !capture && (N1 == 128 || N1 == 256) && col_blocks <= fused_max && !is_split;
                const bool tile_private = p.u16 && !capture && !fused;
                const AdaptPiece a = adaptive_piece<T>(p, fused_ok, capture, cus);
                CHECK(a.fused == fused && a.tile_private == tile_private && adaptive_col_blocks<T>(p) == col_blocks, "adaptive_begin_chunked %zu-byte %lld x %d fused_ok %d capture %d, %d CUs: fused %d tile_private %d",
                      sizeof(T), (long long)n, batch, fused_ok, capture, cus, a.fused, a.tile_private);
                // adaptive_run: a fused run taken in pieces; and the engine it reports
                for (int step : {0, 5})
                    for (int64_t budget : {(int64_t)max_steps - 1, (int64_t)max_steps}) {
                        bool f2 = fused, t2 = tile_private;
                        if (f2 && step == 0 && budget < max_steps) { f2 = false; t2 = p.u16; }
                        const AdaptPiece a2 = adaptive_in_pieces(a, p, step, budget, max_steps);
                        CHECK(a2.fused == f2 && a2.tile_private == t2, "adaptive_run in pieces: step %d budget %lld", step, (long long)budget);
                        CHECK(adaptive_engine(p, a2.fused) == (is_split ? SSFM_ENGINE_SPLIT_ADAPT : f2 ? SSFM_ENGINE_ADAPT_FUSED : SSFM_ENGINE_ADAPT_3), "adaptive engine");
                    }
            }
        }
    }
}
// the cells of tests/test_routes_gpu.py, literally (max_steps 64, a new plan's switches)
static void check_adaptive_anchors() {
    auto begin32 = [](int log2n, int batch, bool capture) { const PlanShape p = shape_of<float>(RouteShape{log2n, batch, 0}); return adaptive_route<float>(p, AdaptSwitches{true, true, true, true, medium_shape_of(p)}, capture, false); };
    CHECK(begin32(11, 2, false) == ADAPT_DEFER_SMALL && begin32(12, 2, false) == ADAPT_DEFER_MEDIUM && begin32(12, 1, false) == ADAPT_DEFER_SMALL && begin32(16, 2, false) == ADAPT_DEFER_MEDIUM
              && begin32(16, 2, true) == ADAPT_CHUNKED && begin32(11, 2, true) == ADAPT_CHUNKED && begin32(18, 2, false) == ADAPT_CHUNKED, "adaptive_begin, complex64");
    const PlanShape c128 = shape_of<double>(RouteShape{16, 2, 0}), c64 = shape_of<float>(RouteShape{16, 2, 0}), big64 = shape_of<float>(RouteShape{20, 2, 0}), big128 = shape_of<double>(RouteShape{20, 2, 0});
    CHECK(adaptive_route<double>(c128, AdaptSwitches{true, true, true, true, true}, false, false) == ADAPT_CHUNKED, "complex128 2^16 x 2 is chunked");
    CHECK(adaptive_piece<double>(c128, true, false, 256).fused && !adaptive_piece<double>(c128, true, false, 256).tile_private, "complex128 2^16 x 2: adaptive_fused");
    const AdaptPiece cap = adaptive_piece<float>(c64, true, true, 256);
    CHECK(!cap.fused && !cap.tile_private && adaptive_engine(c64, cap.fused) == SSFM_ENGINE_ADAPT_3, "complex64 2^16 x 2 with capture: adaptive_3_launches, plain modes");
    CHECK(adaptive_piece<float>(big64, true, false, 256).fused && !adaptive_piece<float>(big64, true, false, 0).fused && adaptive_piece<float>(big64, true, false, 0).tile_private
              && !adaptive_piece<float>(big64, true, false, 255).fused, "complex64 2^20 x 2: 512 workgroups, fused with two per CU on 256 CUs only");
    CHECK(!adaptive_piece<double>(big128, true, false, 256).fused && !adaptive_piece<double>(big128, true, false, 256).tile_private, "complex128 2^20 x 2: 1024 workgroups");
    const PlanShape split = shape_of<float>(RouteShape{21, 1, 20});
    CHECK(!adaptive_piece<float>(split, true, false, 256).fused && adaptive_engine(split, false) == SSFM_ENGINE_SPLIT_ADAPT, "a split plan: split_adaptive");
}

int main() {
    check_shapes<float>("complex64", kC64);
    check_shapes<double>("complex128", kC128);
    check_knobs();
    check_predicates();
    check_fixed<float>();
    check_fixed<double>();
    check_fixed_anchors();
    check_adaptive<float>();
    check_adaptive<double>();
    check_adaptive_anchors();
    if (failures) { std::printf("%lld of %lld cells failed\n", failures, checked); return 1; }
    std::printf("ok: %lld\n", checked);
    return 0;
}
