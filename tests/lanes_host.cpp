// Host program of tests/test_lanes_cpu.py: lane health (opticomlib_amd/csrc/ssfm_lanes.hpp) against a restatement typed from ssfm_host.hip as it stood before
// the header existed -- make_streams, rate_lanes_at_creation, rate_lane, rate_and_replace_lanes, lane_health, heal_lanes, the tail of propagate_fixed, free_all's
// condition, run_info_impl and the debug hook, with the HIP calls replaced by values handed in (the measured periods, the queue probe's answer, whether a
// candidate stream could be made, whether there was memory for the scratch fields).  The header is driven through the same events the way ssfm_host.hip
// drives it now; after every event all fields, the lane fields of ssfm_run_info, the pool's condition and which stream sits in which lane are compared,
// floats by their bits.  Built with AddressSanitizer / UBSan; no GPU.  Prints "ok: <cells checked>", exits non-zero on any miss.
#include "ssfm_lanes.hpp"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>

using namespace ssfm;

static long long failures = 0, checked = 0;
#define CHECK(cond, ...) do { ++checked; if (!(cond)) { if (++failures <= 40) { std::printf("FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)
static uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

// ----------------------------------------------------------------------------- what the device would have answered
struct Meas { bool err = false, shared = false; float a[2] = {10.f, 10.f}, p[2] = {12.f, 12.f}; };      // one rate_lane call: the queue probe, lane 0 alone twice, the pair twice
struct Cand { bool made = true; Meas m; };
struct Script {                 // one rate_and_replace_lanes call (index g = 1 ... 3: the lane; then round and candidate)
    bool big_rows = false, no_memory = false;
    Meas lane[4];
    Cand cand[4][2][4];
};
struct Look { float ms = 0.f; bool has_e1 = true; Script s[2]; };       // one lane_health call: it can heal twice (the cooldown's heal, then the run's)
static Meas meas(float alone, float pair) { Meas m; m.a[0] = m.a[1] = alone; m.p[0] = m.p[1] = pair; return m; }
static Script script_all(const Meas& m) {
    Script s;
    for (int g = 0; g < 4; ++g) { s.lane[g] = m; for (auto& rd : s.cand[g]) for (Cand& c : rd) c.m = m; }
    return s;
}

// ----------------------------------------------------------------------------- (a) the restatement: PlanT's lane fields and functions before the header
constexpr int kSsfmOk = 0;
struct Parent {
    int nlanes = 1;
    bool lanes_share_queue = false;
    int lanes_active = 1;
    int lanes_remade = 0;
    int lanes_dropped = 0;
    int lane_heals = 0, lane_strikes = 0, lane_suspect = 0, lane_dropped_runs = 0;
    bool lanes_from_pool = false;
    int lane_fault = 0;
    float lane_alone_us = 0.f;
    float lane_pair_us = 0.f;
    float lane_last_us = 0.f;
    float lane_score = 0.f;
    bool lane_check_pending = false;
    int64_t lane_check_launches = 0;
    bool lanes_ok = true;
    // the stand-ins for the device: which stream sits in lane g, the next fresh stream's number, rate_lane calls so far, the heals of the look in flight
    int lane_stream[4] = {0, 1, 2, 3}, next_stream = 4, ratings = 0, heal_no = 0;
    bool big_rows = false;

    int rate_lane(const Meas& m, float* score, float* alone_out, float* pair_out) {
        ++ratings;
        *score = 1e30f;
        if (m.err) return -1;
        if (m.shared) return 2;
        float alone = 1e30f, pair = 0.f;
        for (int r = 0; r < 2; ++r) {
            float a1 = m.a[r], p1 = m.p[r];
            alone = a1 < alone ? a1 : alone;
            pair = p1 > pair ? p1 : pair;
        }
        *score = pair / alone;
        *alone_out = alone; *pair_out = pair;
        if (lane_fault == 2) { *score = 9.f; return 1; }
        return *score > (big_rows ? kLaneGoodRatioBig : kLaneGoodRatio) ? 1 : 0;
    }
    int rate_and_replace_lanes(const Script& s, bool* replaced) {
        big_rows = s.big_rows;
        *replaced = false;
        bool all_good = true;
        for (int g = 1; g < nlanes; ++g) {
            float score = 0.f, alone = 0.f, pair = 0.f;
            int state = rate_lane(s.lane[g], &score, &alone, &pair);
            if (state < 0) return -1;
            for (int round = 0; round < 2 && state > 0; ++round) {
                int cand[4];
                for (int c = 0; c < 4; ++c) cand[c] = s.cand[g][round][c].made ? next_stream++ : -1;
                for (int c = 0; c < 4; ++c) {
                    if (cand[c] < 0 || state == 0) continue;
                    float sc = 0.f, al = 0.f, pr = 0.f;
                    const int st_c = rate_lane(s.cand[g][round][c].m, &sc, &al, &pr);
                    if (st_c >= 0 && (st_c < state || (st_c == state && sc < score))) { state = st_c; score = sc; alone = al; pair = pr; *replaced = true; lane_stream[g] = cand[c]; }
                }
            }
            if (state != 0) all_good = false;
            if (state == 2) lanes_share_queue = true;
            if (g == 1 || score > lane_score) lane_score = score;
            if (state != 2) { lane_alone_us = alone; if (state == 0) lane_pair_us = pair; }
        }
        if (all_good) lanes_share_queue = false;
        lanes_ok = all_good;
        return kSsfmOk;
    }
    int create(int nl, bool pooled, float pool_score, const Script& s) {
        nlanes = nl;
        if (pooled) {
            lane_score = pool_score; lane_alone_us = 0.f; lane_pair_us = 0.f;
            lanes_from_pool = true;
        }
        lanes_active = nlanes;
        if (!(nlanes > 1 && nlanes <= 4)) return kSsfmOk;
        bool replaced = false;
        if (lanes_from_pool && nlanes == 2) lanes_ok = true;
        else if (int rc = rate_and_replace_lanes(s, &replaced)) return rc;
        if (!lanes_ok) lane_strikes = 1;
        return kSsfmOk;
    }
    void run(bool health, bool split, int64_t nsteps) {
        if (health) {
            lane_check_pending = true;
            lane_check_launches = (split ? 4 : 2) * nsteps + 1;
        }
    }
    int lane_health(const Look& in) {
        heal_no = 0;
        if (lanes_dropped && nlanes == 2 && ++lane_dropped_runs >= kLaneDroppedCooldown && lane_heals < kLaneHealsMax) {
            lane_dropped_runs = 0;
            const int before = lane_strikes;
            if (int rc = heal_lanes(in)) return rc;
            if (lanes_ok) { lanes_active = nlanes; lanes_dropped = 0; lane_strikes = 0; }
            else lane_strikes = before;
        }
        if (!lane_check_pending) return kSsfmOk;
        lane_check_pending = false;
        if (lanes_active < 2 || lane_check_launches <= 0 || !in.has_e1) return kSsfmOk;
        float ms = in.ms;
        lane_last_us = ms * 1e3f / (float)lane_check_launches;
        if (lane_pair_us <= 0.f || lane_last_us < lane_pair_us) { lane_pair_us = lane_last_us; lane_suspect = 0; return kSsfmOk; }
        if (lane_heals >= kLaneHealsMax) return kSsfmOk;
        if (lane_last_us > kLaneSlowRatio * lane_pair_us) { lane_suspect = 0; return heal_lanes(in); }
        if (lane_last_us > kLaneSuspectRatio * lane_pair_us) { if (++lane_suspect >= 2) { lane_suspect = 0; return heal_lanes(in); } }
        else lane_suspect = 0;
        return kSsfmOk;
    }
    int heal_lanes(const Look& in) {
        ++lane_heals;
        const Script& s = in.s[heal_no++];
        if (s.no_memory) return kSsfmOk;
        const float seen = lane_pair_us;
        bool replaced = false;
        const int rc = rate_and_replace_lanes(s, &replaced);
        if (rc != kSsfmOk) return rc;
        if (replaced) ++lanes_remade;
        if (lanes_ok) {
            lane_strikes = 0;
            if (!replaced) lane_pair_us = lane_last_us;
            else if (seen > 0.f && seen < lane_pair_us) lane_pair_us = seen;
        } else if (++lane_strikes >= 2) {
            lanes_active = 1;
            lanes_dropped = 1;
        }
        return kSsfmOk;
    }
    bool pool_takes() const { return nlanes == 2 && lanes_ok && !lanes_dropped && !lanes_share_queue && lane_fault == 0; }
    void info(ssfm_run_info* out) const {
        ssfm_run_info r;
        std::memset(&r, 0, sizeof(r));
        r.lanes = lanes_active; r.lanes_configured = nlanes; r.lanes_share_queue = lanes_share_queue ? 1 : 0; r.lanes_remade = lanes_remade; r.lanes_dropped = lanes_dropped;
        r.lane_heals = lane_heals;
        r.lane_alone_us = lane_alone_us; r.lane_pair_us = lane_pair_us; r.lane_last_us = lane_last_us; r.lane_score = lane_score;
        r.lanes_from_pool = lanes_from_pool ? 1 : 0;
        *out = r;
    }
    void fault(int mode) { lane_fault = mode; lane_pair_us = mode ? lane_pair_us * 0.25f : lane_pair_us; }
};

// ----------------------------------------------------------------------------- (b) the header, driven as ssfm_host.hip drives it
struct Tree {
    int nlanes = 1;
    LaneHealth lanes;
    int lane_stream[4] = {0, 1, 2, 3}, next_stream = 4, ratings = 0, heal_no = 0;
    bool big_rows = false;

    int rate_lane(const Meas& m, LaneRating* out) {
        ++ratings;
        if (m.err) return -1;
        float alone[2] = {0.f, 0.f}, pair[2] = {0.f, 0.f};
        for (int r = 0; r < 2 && !m.shared; ++r) { alone[r] = m.a[r]; pair[r] = m.p[r]; }
        *out = ssfm::rate_lane(m.shared, alone, pair, big_rows, lanes.lane_fault);
        return 0;
    }
    int rate_and_replace_lanes(const Script& s, bool* replaced) {
        big_rows = s.big_rows;
        *replaced = false;
        bool all_good = true;
        for (int g = 1; g < nlanes; ++g) {
            LaneRating have;
            if (rate_lane(s.lane[g], &have) < 0) return -1;
            for (int round = 0; round < 2 && have.state > 0; ++round) {
                int cand[4];
                for (int c = 0; c < 4; ++c) cand[c] = s.cand[g][round][c].made ? next_stream++ : -1;
                for (int c = 0; c < 4; ++c) {
                    if (cand[c] < 0 || have.state == 0) continue;
                    LaneRating rc_;
                    if (rate_lane(s.cand[g][round][c].m, &rc_) >= 0 && lane_rating_better(rc_, have)) { have = rc_; *replaced = true; lane_stream[g] = cand[c]; }
                }
            }
            lanes.fold_lane(g, have, &all_good);
        }
        lanes.fold_end(all_good);
        return kSsfmOk;
    }
    int create(int nl, bool pooled, float pool_score, const Script& s) {
        nlanes = nl;
        if (pooled) lanes.took_pair(pool_score);
        lanes.streams_made(nlanes);
        if (!(nlanes > 1 && nlanes <= 4)) return kSsfmOk;
        bool replaced = false;
        if (!lanes.pair_counts_as_rated(nlanes))
            if (int rc = rate_and_replace_lanes(s, &replaced)) return rc;
        lanes.created();
        return kSsfmOk;
    }
    void run(bool health, bool split, int64_t nsteps) {
        if (health) lanes.run_enqueued((split ? 4 : 2) * nsteps + 1);
    }
    int lane_health(const Look& in) {
        heal_no = 0;
        if (lanes.cooldown_due(nlanes)) {
            const int before = lanes.cooldown_begin();
            if (int rc = heal_lanes(in)) return rc;
            lanes.cooldown_end(nlanes, before);
        }
        if (!lanes.look_due(in.has_e1)) return kSsfmOk;
        return lanes.run_measured(in.ms) ? heal_lanes(in) : kSsfmOk;
    }
    int heal_lanes(const Look& in) {
        lanes.heal_begin();
        const Script& s = in.s[heal_no++];
        if (s.no_memory) return kSsfmOk;
        const float seen = lanes.lane_pair_us;
        bool replaced = false;
        const int rc = rate_and_replace_lanes(s, &replaced);
        if (rc != kSsfmOk) return rc;
        lanes.heal_rated(replaced, seen);
        return kSsfmOk;
    }
    void info(ssfm_run_info* out) const {
        ssfm_run_info r;
        std::memset(&r, 0, sizeof(r));
        lanes.fill(&r, nlanes);
        *out = r;
    }
};

// ----------------------------------------------------------------------------- both, event by event
struct Stats { long long drops = 0, comebacks = 0, remade = 0, heals = 0, heals_max = 0, shared = 0, new_normal = 0; };
static Stats stats;
struct Both {
    Parent p;
    Tree t;
    const char* what = "";
    long long ev = 0;
    void same() {
        const LaneHealth& h = t.lanes;
        ++ev;
#define SAME_INT(f) CHECK((long long)p.f == (long long)h.f, "%s event %lld: " #f " parent %lld header %lld", what, ev, (long long)p.f, (long long)h.f)
#define SAME_FLT(f) CHECK(bits(p.f) == bits(h.f), "%s event %lld: " #f " parent %.9g header %.9g", what, ev, (double)p.f, (double)h.f)
        SAME_INT(lanes_active); SAME_INT(lanes_ok); SAME_INT(lanes_dropped); SAME_INT(lanes_remade); SAME_INT(lanes_share_queue); SAME_INT(lanes_from_pool);
        SAME_INT(lane_heals); SAME_INT(lane_strikes); SAME_INT(lane_suspect); SAME_INT(lane_dropped_runs); SAME_INT(lane_fault);
        SAME_FLT(lane_alone_us); SAME_FLT(lane_pair_us); SAME_FLT(lane_last_us); SAME_FLT(lane_score);
        SAME_INT(lane_check_pending); SAME_INT(lane_check_launches);
        ssfm_run_info a, b;
        p.info(&a); t.info(&b);
        CHECK(std::memcmp(&a, &b, sizeof(a)) == 0, "%s event %lld: ssfm_run_info differs", what, ev);
        CHECK(p.pool_takes() == h.pair_may_go_to_pool(t.nlanes), "%s event %lld: the pool's condition", what, ev);
        CHECK(std::memcmp(p.lane_stream, t.lane_stream, sizeof(p.lane_stream)) == 0 && p.next_stream == t.next_stream && p.ratings == t.ratings,
              "%s event %lld: streams %d %d %d / %d %d %d, ratings %d / %d", what, ev, p.lane_stream[1], p.lane_stream[2], p.lane_stream[3], t.lane_stream[1], t.lane_stream[2],
              t.lane_stream[3], p.ratings, t.ratings);
    }
    int create(int nl, bool pooled, float pool_score, const Script& s) {
        const int a = p.create(nl, pooled, pool_score, s), b = t.create(nl, pooled, pool_score, s);
        CHECK(a == b, "%s: create returns %d / %d", what, a, b);
        same();
        return b;
    }
    void run(bool health = true, bool split = false, int64_t nsteps = 80) { p.run(health, split, nsteps); t.run(health, split, nsteps); same(); }
    int look(const Look& in) {
        const LaneHealth before = t.lanes;
        const int a = p.lane_health(in), b = t.lane_health(in);
        CHECK(a == b, "%s: lane_health returns %d / %d", what, a, b);
        same();
        const LaneHealth& h = t.lanes;
        stats.drops += !before.lanes_dropped && h.lanes_dropped; stats.comebacks += before.lanes_dropped && !h.lanes_dropped;
        stats.remade += h.lanes_remade - before.lanes_remade; stats.heals += h.lane_heals - before.lane_heals;
        stats.heals_max += before.lane_heals < kLaneHealsMax && h.lane_heals == kLaneHealsMax; stats.shared += !before.lanes_share_queue && h.lanes_share_queue;
        stats.new_normal += h.lane_heals > before.lane_heals && h.lanes_ok && h.lanes_remade == before.lanes_remade && bits(h.lane_pair_us) == bits(h.lane_last_us);
        return b;
    }
    int look(float ms, const Script& s) { Look in; in.ms = ms; in.s[0] = in.s[1] = s; return look(in); }
    void fault(int mode) { p.fault(mode); t.lanes.debug_fault(mode); same(); }
    // a run of 80 steps (161 launches per lane) whose launch period comes out near `us`, and the look at it
    void run_at(float us, const Script& s) { run(); look(us * 161.f / 1e3f, s); }
    const LaneHealth& h() const { return t.lanes; }
};
static bool near(float x, float want) { return std::fabs(x - want) <= 1e-4f * std::fabs(want); }

static const Meas kGoodM = meas(10.f, 12.f), kBadM = meas(10.f, 30.f);
static Script good() { return script_all(kGoodM); }       // the lane rates 1.2: good, no candidate is made
static Script bad() { return script_all(kBadM); }         // the lane and all eight candidates rate 3.0: in the way, none better, nothing replaced

// ----------------------------------------------------------------------------- the rating: thresholds, the fault hook, the probe's counts
static void check_ratings() {
    const float scores[] = {1.599f, 1.601f, 2.099f, 2.101f};
    const int want_small[] = {0, 1, 1, 1}, want_big[] = {0, 0, 0, 1};
    for (int i = 0; i < 4; ++i)
        for (int big = 0; big < 2; ++big)
            for (int fault = 0; fault < 3; ++fault) {
                const float a[2] = {10.f, 11.f}, p[2] = {9.f, 10.f * scores[i]};        // the better alone (10), the worse pair
                const LaneRating r = rate_lane(false, a, p, big != 0, fault);
                Parent q; q.big_rows = big != 0; q.lane_fault = fault;
                Meas m; m.a[0] = a[0]; m.a[1] = a[1]; m.p[0] = p[0]; m.p[1] = p[1];
                float sc = 0.f, al = 0.f, pr = 0.f;
                const int st = q.rate_lane(m, &sc, &al, &pr);
                CHECK(st == r.state && bits(sc) == bits(r.score) && bits(al) == bits(r.alone_us) && bits(pr) == bits(r.pair_us), "rating %g big %d fault %d", scores[i], big, fault);
                CHECK(bits(r.alone_us) == bits(10.f) && bits(r.pair_us) == bits(10.f * scores[i]), "the better alone, the worse pair");
                if (fault == 2) CHECK(r.state == 1 && bits(r.score) == bits(9.f), "fault 2: {1, 9}");
                else CHECK(r.state == (big ? want_big[i] : want_small[i]) && bits(r.score) == bits(10.f * scores[i] / 10.f), "score %g big %d: state %d", scores[i], big, r.state);
            }
    const float z[2] = {0.f, 0.f};
    const LaneRating sh = rate_lane(true, z, z, false, 2);
    CHECK(sh.state == 2 && bits(sh.score) == bits(1e30f) && sh.alone_us == 0.f && sh.pair_us == 0.f, "a shared queue: state 2, whatever the hook says");
    CHECK(lane_probe_steps(false) == 12 && lane_probe_steps(true) == 4 && kLaneProbeSteps == 12, "probe steps");
    for (int nl = 2; nl <= 4; ++nl)
        for (int steps : {4, 12}) CHECK(lane_spin_ticks(steps, nl) == (long long)(400 * (2 * steps + 1) * nl), "spin ticks");
    CHECK(lane_spin_ticks(12, 2) == 20000ll && lane_spin_ticks(4, 2) == 7200ll, "spin ticks of a two-lane plan");
    CHECK(kLaneGoodRatio == 1.6f && kLaneGoodRatioBig == 2.1f && kLaneSlowRatio == 1.8f && kLaneSuspectRatio == 1.3f && kLaneDroppedCooldown == 32 && kLaneHealsMax == 8, "the constants");
}

// ----------------------------------------------------------------------------- candidates: every order of "better state" and "same state, better score"
static Cand cand_kind(int k) {       // 0 not made, 1 shares a queue, 2 in the way at 3.0, 3 in the way at 2.0, 4 good at 1.5, 5 good at 1.2, 6 the rating fails
    Cand c;
    c.made = k != 0; c.m.shared = k == 1; c.m.err = k == 6;
    const float pair[] = {12.f, 12.f, 30.f, 20.f, 15.f, 12.f, 12.f};
    c.m.p[0] = c.m.p[1] = pair[k];
    return c;
}
static void check_candidates() {
    Meas lane_kinds[3] = {meas(10.f, 25.f), meas(10.f, 25.f), meas(10.f, 13.f)};      // in the way at 2.5; shares a queue; good
    lane_kinds[1].shared = true;
    for (int lk = 0; lk < 3; ++lk) {
        // all eight candidates over five kinds; then the first round over all seven kinds with the second round of one kind
        for (int pass = 0; pass < 2; ++pass) {
            const int base = pass == 0 ? 5 : 7, slots = pass == 0 ? 8 : 5;
            long long total = 1;
            for (int i = 0; i < slots; ++i) total *= base;
            for (long long code = 0; code < total; ++code) {
                Script s;
                s.lane[1] = lane_kinds[lk];
                int digit[8];
                long long c = code;
                for (int i = 0; i < slots; ++i) { digit[i] = (int)(c % base); c /= base; }
                for (int i = 0; i < 8; ++i) s.cand[1][i / 4][i % 4] = cand_kind(digit[i < slots ? i : slots - 1]);
                Both b; b.what = "candidates";
                b.create(2, false, 0.f, s);
                if (lk == 2) CHECK(b.t.ratings == 1 && b.t.lane_stream[1] == 1 && b.h().lanes_ok, "a good lane tries no candidate");
            }
        }
    }
    // typed by hand: an in-the-way lane at 2.5; candidates: in the way at 3.0 (worse), at 2.0 (same state, better score: taken), shared (worse state), good at 1.5 (taken); round over
    Script s;
    s.lane[1] = lane_kinds[0];
    const int kinds[4] = {2, 3, 1, 4};
    for (int c = 0; c < 4; ++c) s.cand[1][0][c] = cand_kind(kinds[c]);
    Both b; b.what = "candidates by hand";
    b.create(2, false, 0.f, s);
    CHECK(b.t.lane_stream[1] == 7 && b.t.next_stream == 8 && b.t.ratings == 5, "stream %d next %d ratings %d", b.t.lane_stream[1], b.t.next_stream, b.t.ratings);
    CHECK(b.h().lanes_ok && bits(b.h().lane_score) == bits(15.f / 10.f) && bits(b.h().lane_pair_us) == bits(15.f) && b.h().lane_strikes == 0, "the good candidate's rating is the plan's");
    // a lane that shares a queue and finds only streams that do: state 2 stays, the flag is set, the periods are not the lane's
    Script sq = script_all(lane_kinds[1]);
    Both q; q.what = "shared queue";
    q.create(2, false, 0.f, sq);
    CHECK(q.h().lanes_share_queue && !q.h().lanes_ok && q.h().lane_strikes == 1 && bits(q.h().lane_score) == bits(1e30f) && q.h().lane_alone_us == 0.f && q.h().lane_pair_us == 0.f
          && q.t.lane_stream[1] == 1 && q.t.ratings == 9, "a shared queue that stays");
}

// ----------------------------------------------------------------------------- plans of three and four lanes: the fold
static void check_more_lanes() {
    Meas kinds[3] = {meas(10.f, 12.f), meas(11.f, 27.5f), meas(10.f, 12.f)};
    kinds[2].shared = true;
    for (int nl = 2; nl <= 4; ++nl)
        for (int code = 0; code < 27; ++code) {
            Script s;
            for (int g = 1; g < 4; ++g) { s.lane[g] = kinds[(code / (g == 1 ? 1 : g == 2 ? 3 : 9)) % 3]; for (auto& rd : s.cand[g]) for (Cand& c : rd) c.made = false; }
            Both b; b.what = "three and four lanes";
            b.create(nl, false, 0.f, s);
            b.run(); b.look(2.f, s);
        }
    // typed by hand, four lanes: lane 1 good (1.2, alone 10, pair 12), lane 2 in the way (2.5, alone 11), lane 3 on a shared queue
    Script s;
    s.lane[1] = kinds[0]; s.lane[2] = kinds[1]; s.lane[3] = kinds[2];
    for (int g = 1; g < 4; ++g) for (auto& rd : s.cand[g]) for (Cand& c : rd) c.made = false;
    Both b; b.what = "four lanes by hand";
    b.create(4, false, 0.f, s);
    CHECK(!b.h().lanes_ok && b.h().lanes_share_queue && b.h().lanes_active == 4 && b.h().lane_strikes == 1, "four lanes: not ok, a shared queue, one strike");
    CHECK(bits(b.h().lane_score) == bits(1e30f) && bits(b.h().lane_alone_us) == bits(11.f) && bits(b.h().lane_pair_us) == bits(12.f), "the worst score, the last unshared lane's alone, the good lane's pair");
    CHECK(!b.h().pair_may_go_to_pool(4), "four lanes never go to the pool");
}

// ----------------------------------------------------------------------------- a run's verdict at its edges
// ms whose period over `launches` launches is exactly `us`, if there is one nearby
static bool ms_for(float us, int64_t launches, float* out) {
    float lo = us * (float)launches / 1e3f, hi = lo;
    for (int i = 0; i < 64; ++i) {
        if (bits(lo * 1e3f / (float)launches) == bits(us)) { *out = lo; return true; }
        if (bits(hi * 1e3f / (float)launches) == bits(us)) { *out = hi; return true; }
        lo = std::nextafterf(lo, 0.f); hi = std::nextafterf(hi, INFINITY);
    }
    return false;
}
static void check_run_edges() {
    // ratios of the plan's best period (12 us from its rating), each twice in a row, for lane_fault 0 / 1 / 2 set before and between the runs
    const float ratios[] = {0.5f, 0.999f, 1.0f, 1.299f, 1.301f, 1.799f, 1.801f, 4.f};
    for (float r1 : ratios)
        for (float r2 : ratios)
            for (int f1 = 0; f1 < 3; ++f1)
                for (int f2 = 0; f2 < 3; ++f2)
                    for (int heal_kind = 0; heal_kind < 2; ++heal_kind) {
                        Both b; b.what = "ratios";
                        b.create(2, false, 0.f, good());
                        b.fault(f1);
                        b.run_at(r1 * b.h().lane_pair_us, heal_kind ? bad() : good());
                        b.fault(f2);
                        b.run_at(r2 * b.h().lane_pair_us, heal_kind ? bad() : good());
                        b.look(1.f, good());          // (nothing pending: a look that only counts)
                    }
    // one float step below, at and above 1.3f x and 1.8f x the best period; the outcomes typed by hand
    int hits[6] = {0, 0, 0, 0, 0, 0};
    for (int k = 0; k < 200; ++k) {
        const float pair = 7.f + 0.013f * (float)k;
        const float t13 = kLaneSuspectRatio * pair, t18 = kLaneSlowRatio * pair;
        const float targets[6] = {std::nextafterf(t13, 0.f), t13, std::nextafterf(t13, INFINITY), std::nextafterf(t18, 0.f), t18, std::nextafterf(t18, INFINITY)};
        const int want_suspect[6] = {0, 0, 1, 1, 1, 0}, want_heals[6] = {0, 0, 0, 0, 0, 1};
        for (int i = 0; i < 6; ++i)
            for (int64_t nsteps : {80, 1000}) {
                float ms = 0.f;
                if (!ms_for(targets[i], 2 * nsteps + 1, &ms)) continue;
                ++hits[i];
                Both b; b.what = "float steps";
                b.create(2, false, 0.f, script_all(meas(pair / 1.25f, pair)));
                CHECK(bits(b.h().lane_pair_us) == bits(pair), "the rating's pair period is the plan's best");
                b.run(true, false, nsteps);
                b.look(ms, bad());
                CHECK(bits(b.h().lane_last_us) == bits(targets[i]) && b.h().lane_suspect == want_suspect[i] && b.h().lane_heals == want_heals[i],
                      "edge %d of pair %.9g: last %.9g suspect %d heals %d", i, (double)pair, (double)b.h().lane_last_us, b.h().lane_suspect, b.h().lane_heals);
                b.run(true, false, nsteps);
                b.look(ms, bad());            // the same again: a suspect's second time is a heal
                CHECK(b.h().lane_heals == (want_suspect[i] || want_heals[i] ? want_heals[i] + 1 : 0), "edge %d twice: heals %d", i, b.h().lane_heals);
            }
    }
    for (int i = 0; i < 6; ++i) CHECK(hits[i] >= 20, "edge %d was reached %d times", i, hits[i]);
    // a look with no run pending, with no events, with no launches, with one lane: nothing is measured
    for (int kind = 0; kind < 4; ++kind) {
        Both b; b.what = "no look";
        b.create(kind == 3 ? 1 : 2, false, 0.f, good());
        if (kind != 0) b.run(true, false, kind == 2 ? -1 : 80);
        Look in; in.ms = 100.f; in.has_e1 = kind != 1; in.s[0] = in.s[1] = bad();
        b.look(in);
        CHECK(b.h().lane_last_us == 0.f && b.h().lane_heals == 0 && !b.h().lane_check_pending, "no look, kind %d", kind);
    }
}

// ----------------------------------------------------------------------------- the stories (the comment above measure_lanes; DESIGN.md "self-healing two-lane plan")
static void check_stories() {
    {   // 1. one moderately slow run is forgiven; two in a row are rated
        Both b; b.what = "story 1";
        b.create(2, false, 0.f, good());
        CHECK(b.h().lanes_active == 2 && b.h().lanes_ok && b.h().lane_strikes == 0 && bits(b.h().lane_score) == bits(12.f / 10.f) && bits(b.h().lane_alone_us) == bits(10.f)
              && bits(b.h().lane_pair_us) == bits(12.f) && !b.h().lanes_from_pool && b.t.ratings == 1, "a good pair at creation");
        b.run_at(18.f, good());
        CHECK(b.h().lane_suspect == 1 && b.h().lane_heals == 0 && near(b.h().lane_last_us, 18.f) && bits(b.h().lane_pair_us) == bits(12.f), "1.5 x once: a suspect");
        b.run_at(12.f, good());
        CHECK(b.h().lane_suspect == 0 && b.h().lane_heals == 0, "a normal run forgives");
        b.run_at(18.f, good());
        CHECK(b.h().lane_suspect == 1 && b.h().lane_heals == 0, "a suspect again");
        b.run_at(18.f, good());
        CHECK(b.h().lane_suspect == 0 && b.h().lane_heals == 1 && b.t.ratings == 2, "twice in a row: rated");
    }
    {   // 2. slow for another reason: the run's period is the plan's normal from now on, and the next run at that level is not rated
        Both b; b.what = "story 2";
        b.create(2, false, 0.f, good());
        b.run_at(48.f, good());
        CHECK(b.h().lane_heals == 1 && b.h().lanes_remade == 0 && b.h().lanes_ok && b.h().lane_strikes == 0 && near(b.h().lane_pair_us, 48.f)
              && bits(b.h().lane_pair_us) == bits(b.h().lane_last_us), "4 x: rated at once, good and unreplaced");
        b.run_at(48.f, bad());
        CHECK(b.h().lane_heals == 1 && b.h().lane_suspect == 0 && b.t.ratings == 2, "the next run at that level is not rated");
        b.run_at(12.f, bad());
        CHECK(b.h().lane_heals == 1 && near(b.h().lane_pair_us, 12.f), "a faster run is the best period again");
    }
    for (int better = 0; better < 2; ++better) {   // 3. a replaced lane keeps the better of the earlier and the rating's period
        Both b; b.what = "story 3";
        b.create(2, false, 0.f, good());
        Script s = bad();
        s.cand[1][0][2].m = meas(10.f, better ? 11.f : 15.f);       // the third candidate is good
        b.run_at(48.f, s);
        CHECK(b.h().lane_heals == 1 && b.h().lanes_remade == 1 && b.h().lanes_ok && b.h().lane_strikes == 0 && b.t.lane_stream[1] == 6 && b.t.ratings == 5, "replaced by the third candidate");
        CHECK(bits(b.h().lane_pair_us) == bits(better ? 11.f : 12.f) && bits(b.h().lane_score) == bits((better ? 11.f : 15.f) / 10.f), "pair %.9g", (double)b.h().lane_pair_us);
    }
    {   // 4. two heals in a row that find no good lane drop the plan; 6. it heals again at its 32nd look and not before
        for (int back = 0; back < 2; ++back) {
            Both b; b.what = "stories 4 and 6";
            b.create(2, false, 0.f, good());
            b.run_at(48.f, bad());
            CHECK(b.h().lane_heals == 1 && b.h().lane_strikes == 1 && b.h().lanes_active == 2 && b.h().lanes_dropped == 0 && !b.h().lanes_ok && b.t.ratings == 1 + 9, "one strike");
            b.run_at(48.f, bad());
            CHECK(b.h().lane_heals == 2 && b.h().lane_strikes == 2 && b.h().lanes_active == 1 && b.h().lanes_dropped == 1 && b.h().lanes_remade == 0, "dropped");
            CHECK(!b.h().pair_may_go_to_pool(2), "a dropped plan's pair does not go to the pool");
            // a loop of run + synchronize: two looks per run (the run is a one-lane run: nothing pending)
            for (int run = 1; run <= 16; ++run) {
                b.look(1.f, back ? good() : bad());
                b.run(false);
                if (run < 16) { b.look(1.f, back ? good() : bad()); CHECK(b.h().lane_heals == 2 && b.h().lane_dropped_runs == 2 * run, "no heal before the 32nd look"); }
            }
            CHECK(b.h().lane_dropped_runs == 31 && b.h().lane_heals == 2, "31 looks");
            b.look(1.f, back ? good() : bad());
            CHECK(b.h().lane_heals == 3 && b.h().lane_dropped_runs == 0, "the 32nd look heals, and the count starts again");
            if (back) CHECK(b.h().lanes_active == 2 && b.h().lanes_dropped == 0 && b.h().lane_strikes == 0 && b.h().lanes_ok && bits(b.h().lane_pair_us) == bits(b.h().lane_last_us), "good lanes come back");
            else CHECK(b.h().lanes_active == 1 && b.h().lanes_dropped == 1 && b.h().lane_strikes == 2 && !b.h().lanes_ok, "bad lanes: still dropped, with the strikes it had");
            if (!back) {
                for (int i = 1; i <= 31; ++i) b.look(1.f, good());
                CHECK(b.h().lane_heals == 3 && b.h().lane_dropped_runs == 31, "31 looks again");
                b.look(1.f, good());
                CHECK(b.h().lane_heals == 4 && b.h().lanes_active == 2 && b.h().lanes_dropped == 0, "the next 32nd look");
            }
        }
    }
    {   // 5. a plan created with no good stream has one strike: its first failed heal drops it
        Both b; b.what = "story 5";
        b.create(2, false, 0.f, bad());
        CHECK(!b.h().lanes_ok && b.h().lane_strikes == 1 && b.h().lanes_active == 2 && b.h().lane_pair_us == 0.f && bits(b.h().lane_alone_us) == bits(10.f)
              && bits(b.h().lane_score) == bits(3.f) && b.t.ratings == 9 && b.t.lane_stream[1] == 1, "no good stream at creation");
        b.run_at(30.f, bad());
        CHECK(b.h().lane_heals == 0 && near(b.h().lane_pair_us, 30.f), "the first long run sets the best period");
        b.run_at(120.f, bad());
        CHECK(b.h().lane_heals == 1 && b.h().lane_strikes == 2 && b.h().lanes_dropped == 1 && b.h().lanes_active == 1, "the first failed heal drops it");
    }
    {   // 7. after kLaneHealsMax heals nothing is rated any more: by slowness ...
        Both b; b.what = "story 7, slow runs";
        b.create(2, false, 0.f, good());
        float us = 12.f;
        for (int i = 1; i <= 8; ++i) { us *= 4.f; b.run_at(us, good()); CHECK(b.h().lane_heals == i, "heal %d", i); }
        b.run_at(us * 4.f, bad());
        CHECK(b.h().lane_heals == 8 && b.t.ratings == 9 && near(b.h().lane_last_us, us * 4.f) && near(b.h().lane_pair_us, us) && b.h().lanes_active == 2, "the ninth slow run is not rated");
    }
    {   // ... or by cooldown
        Both b; b.what = "story 7, cooldown";
        b.create(2, false, 0.f, good());
        b.run_at(48.f, bad()); b.run_at(48.f, bad());
        for (int heal = 3; heal <= 8; ++heal) {
            for (int i = 0; i < 32; ++i) b.look(1.f, bad());
            CHECK(b.h().lane_heals == heal && b.h().lanes_dropped == 1 && b.h().lane_dropped_runs == 0, "cooldown heal %d", heal);
        }
        for (int i = 0; i < 64; ++i) b.look(1.f, good());
        CHECK(b.h().lane_heals == 8 && b.h().lanes_dropped == 1 && b.h().lanes_active == 1 && b.h().lane_dropped_runs == 64, "no ninth heal, the looks are still counted");
    }
    {   // 8. a pooled pair is not rated at creation and is watched like any other
        Both b; b.what = "story 8";
        b.create(2, true, 1.25f, bad());
        CHECK(b.t.ratings == 0 && b.h().lanes_from_pool && b.h().lanes_ok && b.h().lane_strikes == 0 && bits(b.h().lane_score) == bits(1.25f) && b.h().lane_alone_us == 0.f
              && b.h().lane_pair_us == 0.f && b.h().lanes_active == 2 && b.h().pair_may_go_to_pool(2), "a pooled pair");
        ssfm_run_info info;
        b.t.info(&info);
        CHECK(info.lanes == 2 && info.lanes_configured == 2 && info.lanes_from_pool == 1 && info.lane_heals == 0 && bits(info.lane_score) == bits(1.25f) && info.lane_pair_us == 0.f, "its run info");
        b.fault(1);
        CHECK(b.h().lane_pair_us == 0.f, "a quarter of no period is no period");
        b.fault(0);
        b.run_at(12.f, bad());
        CHECK(b.h().lane_heals == 0 && near(b.h().lane_pair_us, 12.f), "the first long run sets the periods");
        b.run_at(48.f, good());
        CHECK(b.h().lane_heals == 1 && b.t.ratings == 1 && b.h().lanes_from_pool, "watched like any other");
    }
    {   // 9. the pool takes a pair only if: two lanes, lanes ok, not dropped, no shared queue, no fault hook
        for (int code = 0; code < 32 * 3; ++code) {
            LaneHealth h; Parent p;
            const int nl = 2 + code / 32;
            p.nlanes = nl;
            h.lanes_ok = p.lanes_ok = code & 1; h.lanes_dropped = p.lanes_dropped = (code >> 1) & 1; h.lanes_share_queue = p.lanes_share_queue = (code >> 2) & 1;
            h.lane_fault = p.lane_fault = ((code >> 3) & 3) % 3;
            const bool want = nl == 2 && (code & 1) && !((code >> 1) & 1) && !((code >> 2) & 1) && ((code >> 3) & 3) % 3 == 0;
            CHECK(h.pair_may_go_to_pool(nl) == want && p.pool_takes() == want, "pool condition %d", code);
        }
        Both b; b.what = "story 9";
        b.create(2, false, 0.f, good());
        CHECK(b.h().pair_may_go_to_pool(2), "a good pair goes to the pool");
        b.fault(1);
        CHECK(!b.h().pair_may_go_to_pool(2) && bits(b.h().lane_pair_us) == bits(3.f), "not with the hook set; the hook quarters the best period");
        b.fault(2);
        CHECK(bits(b.h().lane_pair_us) == bits(0.75f), "... again");
        b.fault(0);
        CHECK(b.h().pair_may_go_to_pool(2) && bits(b.h().lane_pair_us) == bits(0.75f), "the hook cleared");
    }
    {   // (not reachable from the host file, where a dropped plan's runs are one-lane runs that nobody looks at: a run pending at the 32nd look is measured
        // by the lanes that have just come back -- two heals in one look)
        Both b; b.what = "two heals in one look";
        b.create(2, false, 0.f, good());
        b.run_at(48.f, bad()); b.run_at(48.f, bad());
        for (int i = 0; i < 31; ++i) b.look(1.f, bad());
        b.run(true);
        b.look(4.f * 48.f * 161.f / 1e3f, good());
        CHECK(b.t.heal_no == 2 && b.h().lane_heals == 4 && b.h().lanes_active == 2 && b.h().lanes_dropped == 0 && near(b.h().lane_pair_us, 192.f), "heals %d", b.h().lane_heals);
    }
    {   // (a state no event leads to, set by hand on both sides: a heal of a plan that has seen no period yet keeps the rating's)
        Both b; b.what = "nothing seen";
        b.create(2, true, 1.25f, good());
        b.p.lanes_dropped = b.t.lanes.lanes_dropped = 1; b.p.lane_dropped_runs = b.t.lanes.lane_dropped_runs = 31;
        Script s = bad();
        s.cand[1][0][0].m = meas(10.f, 15.f);
        b.look(1.f, s);
        CHECK(b.h().lane_heals == 1 && b.h().lanes_remade == 1 && b.h().lanes_dropped == 0 && bits(b.h().lane_pair_us) == bits(15.f), "pair %.9g", (double)b.h().lane_pair_us);
    }
    {   // no memory for the scratch fields: the heal counts, nothing else changes; a rating that fails: the error goes to the caller before any bookkeeping
        Both b; b.what = "no memory";
        b.create(2, false, 0.f, good());
        Script s = bad(); s.no_memory = true;
        b.run_at(48.f, s);
        CHECK(b.h().lane_heals == 1 && b.h().lanes_ok && b.h().lane_strikes == 0 && bits(b.h().lane_pair_us) == bits(12.f) && b.t.ratings == 1, "no memory");
        Script e = bad(); e.lane[1].err = true;
        b.run();
        Look in; in.ms = 48.f * 161.f / 1e3f; in.s[0] = in.s[1] = e;
        CHECK(b.look(in) == -1 && b.h().lane_heals == 2 && b.h().lane_strikes == 0 && b.h().lanes_remade == 0, "a failed rating");
    }
}

// ----------------------------------------------------------------------------- long pseudo-random event sequences
struct Lcg {
    uint64_t s;
    unsigned next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (unsigned)(s >> 33); }
    unsigned below(unsigned n) { return next() % n; }
};
static Meas random_meas(Lcg& r, int mood) {       // mood 0: mostly good, 1: mixed, 2: mostly bad
    static const float ratios[] = {1.1f, 1.2f, 1.3f, 1.599f, 1.601f, 2.0f, 2.099f, 2.101f, 3.f, 5.f};
    Meas m;
    m.err = r.below(512) == 0;
    m.shared = r.below(mood == 2 ? 4 : 16) == 0;
    for (int i = 0; i < 2; ++i) {
        m.a[i] = 5.f + 0.01f * (float)r.below(1000);
        const unsigned k = mood == 0 ? r.below(4) : mood == 1 ? r.below(10) : 4 + r.below(6);
        m.p[i] = m.a[i] * ratios[k];
    }
    return m;
}
static Script random_script(Lcg& r, int mood) {
    Script s;
    s.big_rows = r.below(4) == 0; s.no_memory = r.below(64) == 0;
    for (int g = 1; g < 4; ++g) {
        s.lane[g] = random_meas(r, mood);
        for (auto& rd : s.cand[g]) for (Cand& c : rd) { c.made = r.below(8) != 0; c.m = random_meas(r, mood); }
    }
    if (r.below(16) == 0)             // (every stream the runtime hands out sits on lane 0's queue)
        for (int g = 1; g < 4; ++g) { s.lane[g].shared = true; for (auto& rd : s.cand[g]) for (Cand& c : rd) c.m.shared = true; }
    return s;
}
static void check_random_sequences() {
    static const float ratios[] = {0.5f, 0.999f, 1.0f, 1.299f, 1.301f, 1.799f, 1.801f, 4.f};
    static const int64_t steps[] = {64, 80, 300, 1000, -1};
    int sequences = 0;
    for (uint64_t seed = 1; seed <= 240; ++seed) {
        Lcg r{0x9E3779B97F4A7C15ull * seed};
        Both b; b.what = "random";
        const int nl = seed % 3 == 0 ? 2 + (int)r.below(3) : 2;
        int mood = (int)r.below(3);
        if (b.create(nl, r.below(4) == 0, 1.f + 0.01f * (float)r.below(100), random_script(r, mood)) != kSsfmOk) continue;
        for (int e = 0; e < 600; ++e) {
            if (e % 60 == 59) mood = (int)r.below(3);
            const unsigned kind = r.below(20);
            if (kind < 9) {
                const bool health = r.below(16) == 0 ? r.below(2) != 0 : b.h().lanes_active > 1;
                b.run(health, r.below(8) == 0, steps[r.below(32) == 0 ? 4 : r.below(4)]);
            } else if (kind < 18) {
                Look in;
                const float L = (float)(b.h().lane_check_launches > 0 ? b.h().lane_check_launches : 161);
                in.ms = b.h().lane_pair_us > 0.f && r.below(8) != 0 ? ratios[r.below(8)] * b.h().lane_pair_us * L / 1e3f : 0.5f + 0.001f * (float)r.below(4000);
                in.has_e1 = r.below(32) != 0;
                in.s[0] = random_script(r, mood); in.s[1] = random_script(r, mood);
                b.look(in);
            } else b.fault((int)r.below(3));
        }
        CHECK(b.ev >= 500, "a sequence of %lld events", b.ev);
        ++sequences;
    }
    CHECK(sequences >= 200, "%d sequences ran to their end", sequences);
    CHECK(stats.drops > 20 && stats.comebacks > 20 && stats.remade > 20 && stats.heals > 200 && stats.heals_max > 5 && stats.shared > 5 && stats.new_normal > 20,
          "the sequences reach every transition: drops %lld comebacks %lld remade %lld heals %lld heals_max %lld shared %lld new_normal %lld", stats.drops, stats.comebacks,
          stats.remade, stats.heals, stats.heals_max, stats.shared, stats.new_normal);
}

int main() {
    check_ratings();
    check_candidates();
    check_more_lanes();
    check_run_edges();
    check_stories();
    check_random_sequences();
    if (failures) { std::printf("%lld of %lld checks failed\n", failures, checked); return 1; }
    std::printf("ok: %lld\n", checked);
    return 0;
}
