// ssfm_lanes.hpp -- lane health: the rule by which a plan of two (or more) lanes rates its streams, looks at every long run, heals a lane, drops to one
// lane, tries its second lane again and hands a good pair of streams to the pool -- as a state machine on plain values.  Plain C++ -- no HIP types, no
// environment, no allocation, no threads -- so that a host program can drive every branch (tests/lanes_host.cpp, tests/test_lanes_cpu.py).  ssfm_host.hip
// measures (streams, events, probe launches, scratch fields) and asks; nothing but the functions below writes a field of LaneHealth.
#pragma once
#include <cstdint>
#include "ssfm_amd.h"
namespace ssfm {
// Which hardware queue the runtime gives a lane's stream decides whether its kernels run beside the other lane's at full rate, one
// after the other (a shared queue) or 3-6 x slower than that (profiles/r04_order_dependence.txt); nothing in the API says which.  Round 4 rated a
// stream at plan creation by a proxy (dependent launches of a 3 us spin kernel) and still met about one slow plan in 25-40 suite runs, silently.
// Round 5: (1) the rating is the real thing -- the launch period of the plan's OWN two kernels with both lanes running against lane 0 alone;
// (2) every fixed-step run of >= 64 steps is looked at afterwards (run_measured: its device time / launches per lane against the best period the
// plan has seen); a run beyond kLaneSlowRatio has the lanes rated again on scratch buffers, a lane that is not good gets another stream
// (`lanes_remade`), and a plan that two healing attempts in a row could not repair drops to one lane (`lanes_dropped`: both rows in one launch on
// the plan's stream -- slower than two good lanes, 2-4 x faster than two bad ones).  ssfm_last_run_info reports all of it.
//
// A lane is good when its launches run beside the other lane's at (nearly) the rate they run alone: the launch period of the plan's OWN kernels with both lanes
// running within kLaneGoodRatio x the period of lane 0 alone (healthy plans measure 1.15-1.3 x, the slow states of profiles/r04_order_dependence.txt 2.3-6 x,
// lanes that share a hardware queue 2 x).  At run time a fixed-step run whose own launch period exceeds kLaneSlowRatio x the best period the plan has seen
// has its lanes rated again (LaneHealth::run_measured).
constexpr float kLaneGoodRatio = 1.6f;
constexpr float kLaneGoodRatioBig = 2.1f;
constexpr float kLaneSlowRatio = 1.8f;
constexpr float kLaneSuspectRatio = 1.3f;        // two checked runs in a row beyond this (round 6: profiles/r05_final_lane_stability.txt had one plan at 1.37 x that 1.8 never sees)
constexpr int kLaneDroppedCooldown = 32;         // looks at the lanes (LaneHealth::cooldown_due) after which a plan that dropped to one lane tries its second lane again
constexpr int kLaneProbeSteps = 12;
constexpr int kLaneHealsMax = 8;

// ----------------------------------------------------------------------------- rating one lane
// (rows of 32 MiB and more -- complex128 plans of 2^21 points up, the lines of long chirp-z runs: a launch is 30-100 us long, a third of the probe steps measure it as well)
constexpr int lane_probe_steps(bool big_rows) { return big_rows ? kLaneProbeSteps / 3 : kLaneProbeSteps; }
// the spin kernel that holds the lanes' queues while the host enqueues a measurement (100 MHz ticks: 4 us per launch to come -- the host needs ~3)
constexpr long long lane_spin_ticks(int steps, int nlanes) { return (long long)(400 * (2 * steps + 1) * nlanes); }
// state 0 = good, 1 = on a queue of its own but in lane 0's way (score = the ratio), 2 = shares a hardware queue with an earlier lane
struct LaneRating { int state = 0; float score = 0.f, alone_us = 0.f, pair_us = 0.f; };
// `alone` / `pair`: the launch period of lane 0 alone and with the lane beside it, measured twice (not looked at for a lane that shares a queue)
inline LaneRating rate_lane(bool shares_queue, const float (&alone_us)[2], const float (&pair_us)[2], bool big_rows, int lane_fault) {
    if (shares_queue) return {2, 1e30f, 0.f, 0.f};
    float alone = 1e30f, pair = 0.f;        // (the slow state is erratic -- one of its readings may look good: the WORSE of two, against the better alone)
    for (int i = 0; i < 2; ++i) { alone = alone_us[i] < alone ? alone_us[i] : alone; pair = pair_us[i] > pair ? pair_us[i] : pair; }
    if (lane_fault == 2) return {1, 9.f, alone, pair};
    // Round 6: a kernel that moves 32 MiB and more per row keeps the memory system busy by itself, and its twin beside it legitimately takes up to twice as long per launch
    // (2^22-point complex128 rows: 1.80-1.82, and two lanes are still 18 % faster per step than one launch for both rows) -- rated against 1.6 such a pair was "in the way",
    // had four replacement streams tried in vain, was never pooled, and every such plan took 117 ms to make (tools/plan_create_time.py).  The slow states measure 2.3-6 x.
    const float score = pair / alone;
    return {score > (big_rows ? kLaneGoodRatioBig : kLaneGoodRatio) ? 1 : 0, score, alone, pair};
}
// a candidate stream rated in the lane's place replaces the lane's stream
constexpr bool lane_rating_better(const LaneRating& cand, const LaneRating& have) { return cand.state < have.state || (cand.state == have.state && cand.score < have.score); }

// ----------------------------------------------------------------------------- the plan's state
struct LaneHealth {
    bool lanes_share_queue = false;    // the plan's lanes could not be given hardware queues of their own (see streams_run_side_by_side)
    int lanes_active = 1;              // lanes a fixed-step run really drives: nlanes, or 1 once a plan that could not be healed has dropped to one lane
    int lanes_remade = 0;              // lane streams replaced at RUN time (a run came out slow, the lanes were rated again and one was not good)
    int lanes_dropped = 0;             // 1: the plan gave up its second lane (two healing attempts in a row found no good stream)
    int lane_heals = 0, lane_strikes = 0, lane_suspect = 0, lane_dropped_runs = 0;
    bool lanes_from_pool = false;      // this plan's lane pair came rated from the process's pool (no probe launches at creation)
    int lane_fault = 0;                // test hook (ssfm_debug_lane_fault): 2 = every rating comes out "in the way"
    float lane_alone_us = 0.f;         // launch period of lane 0's chain alone on the chip (the plan's own kernels; last rating)
    float lane_pair_us = 0.f;          // best launch period seen with all lanes running: the last rating's, or a real run's
    float lane_last_us = 0.f;          // launch period of the last checked fixed-step run (device time / launches per lane)
    float lane_score = 0.f;            // last rating: period with the other lane / period alone
    bool lane_check_pending = false;   // the last run was a two-lane run of >= 64 steps whose period has not been looked at yet
    int64_t lane_check_launches = 0;
    bool lanes_ok = true;

    // ---- plan creation
    void streams_made(int nlanes) { lanes_active = nlanes; }
    // a pair from the pool (the periods are this plan's own kernels': the first long run sets them)
    void took_pair(float score) { lane_score = score; lane_alone_us = 0.f; lane_pair_us = 0.f; lanes_from_pool = true; }
    // true: rated by the plan that made the pair (run_measured watches the runs as for any plan); false: the lanes want a rating now
    bool pair_counts_as_rated(int nlanes) { if (lanes_from_pool && nlanes == 2) lanes_ok = true; return lanes_from_pool && nlanes == 2; }
    void created() { if (!lanes_ok) lane_strikes = 1; }          // (no good stream to be had now: the first run that comes out slow and cannot be healed drops the second lane)

    // ---- a rating of every lane beyond the first, folded into the plan: fold_lane for g = 1 ... nlanes - 1 (`all_good` starts true), then fold_end
    void fold_lane(int g, const LaneRating& r, bool* all_good) {
        if (r.state != 0) *all_good = false;
        if (r.state == 2) lanes_share_queue = true;
        if (g == 1 || r.score > lane_score) lane_score = r.score;
        if (r.state != 2) { lane_alone_us = r.alone_us; if (r.state == 0) lane_pair_us = r.pair_us; }
    }
    void fold_end(bool all_good) { if (all_good) lanes_share_queue = false; lanes_ok = all_good; }

    // ---- run time.  A run of `launches` launches per lane was enqueued between the events a look reads
    void run_enqueued(int64_t launches) { lane_check_pending = true; lane_check_launches = launches; }
    // Every look at the lanes begins here (and counts): a plan that gave up its second lane under contention that may have passed gets one more rating
    // on scratch fields -- cooldown_begin, the heal, cooldown_end: good lanes come back
    bool cooldown_due(int nlanes) { return lanes_dropped && nlanes == 2 && ++lane_dropped_runs >= kLaneDroppedCooldown && lane_heals < kLaneHealsMax; }
    int cooldown_begin() { lane_dropped_runs = 0; return lane_strikes; }
    void cooldown_end(int nlanes, int strikes_before) { if (lanes_ok) { lanes_active = nlanes; lanes_dropped = 0; lane_strikes = 0; } else lane_strikes = strikes_before; }
    // is there a run to look at (`has_events`: the events that bracket it exist)
    bool look_due(bool has_events) {
        const bool pending = lane_check_pending;
        lane_check_pending = false;
        return pending && !(lanes_active < 2 || lane_check_launches <= 0 || !has_events);
    }
    // the run took `ms` on the device: true = heal the lanes
    bool run_measured(float ms) {
        lane_last_us = ms * 1e3f / (float)lane_check_launches;
        if (lane_pair_us <= 0.f || lane_last_us < lane_pair_us) { lane_pair_us = lane_last_us; lane_suspect = 0; return false; }
        if (lane_heals >= kLaneHealsMax) return false;
        if (lane_last_us > kLaneSlowRatio * lane_pair_us) { lane_suspect = 0; return true; }
        // a second look for the moderately slow: one such run is other work on the GPU, two in a row are rated
        if (lane_last_us > kLaneSuspectRatio * lane_pair_us) { if (++lane_suspect >= 2) { lane_suspect = 0; return true; } }
        else lane_suspect = 0;
        return false;
    }
    // a heal: heal_begin, the rating on scratch fields (fold_lane / fold_end), heal_rated with the best period seen before the rating
    void heal_begin() { ++lane_heals; }
    void heal_rated(bool replaced, float seen) {
        if (replaced) ++lanes_remade;
        if (!lanes_ok) { if (++lane_strikes >= 2) { lanes_active = 1; lanes_dropped = 1; } return; }
        lane_strikes = 0;
        // nothing wrong with the lanes (any more).  Not replaced: the run was slow for another reason (other work on the GPU, a profiler) -- its period is
        // what is normal from now on until a faster run is seen, so that every further run at this level is not rated again
        if (!replaced) lane_pair_us = lane_last_us;
        else if (seen > 0.f && seen < lane_pair_us) lane_pair_us = seen;
    }

    // ---- the readers and the test hook
    bool pair_may_go_to_pool(int nlanes) const { return nlanes == 2 && lanes_ok && !lanes_dropped && !lanes_share_queue && lane_fault == 0; }
    void fill(ssfm_run_info* r, int nlanes) const {
        r->lanes = lanes_active; r->lanes_configured = nlanes; r->lanes_share_queue = lanes_share_queue ? 1 : 0; r->lanes_remade = lanes_remade; r->lanes_dropped = lanes_dropped;
        r->lane_heals = lane_heals;
        r->lane_alone_us = lane_alone_us; r->lane_pair_us = lane_pair_us; r->lane_last_us = lane_last_us; r->lane_score = lane_score;
        r->lanes_from_pool = lanes_from_pool ? 1 : 0;
    }
    void debug_fault(int mode) { lane_fault = mode; lane_pair_us = mode ? lane_pair_us * 0.25f : lane_pair_us; }
};
}  // namespace ssfm
