// Host program of tests/test_capture_cpu.py: the capture rings and the adaptive chunks (opticomlib_amd/csrc/ssfm_capture.hpp).
//  1. A restatement typed from ssfm_host.hip, chirpz.hip and manakov.hip as they stood before the header existed -- propagate_fixed_capture, lane_run,
//     capture_helper, propagate_fixed's block, adaptive_set_capture, acap_wants, adaptive_estimate, adaptive_chunks, adaptive_enqueue_chunk,
//     adaptive_send_snapshots and the two lines' estimates -- compared with the header field by field.
//  2. A model of the ring under random scheduling: 1, 2 and 8 producer lanes and the helper, driven by the ring's functions in the order lane_run and
//     capture_helper use them.  The model takes the ring as a parameter and is shown to reject four mutants.
//  3. A model of the adaptive loop (adaptive_chunks / adaptive_enqueue_chunk / adaptive_send_snapshots, host only) over synthetic runs, with the header's
//     rules and with the restatement's, compared and held to its invariants.
// Built with AddressSanitizer / UBSan; no GPU.  Prints "ok: <cells checked>", exits non-zero on any miss.
#include "ssfm_capture.hpp"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

using namespace ssfm;

static long long failures = 0, checked = 0;
#define CHECK(cond, ...) do { ++checked; if (!(cond)) { if (++failures <= 40) { std::printf("FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)
struct Rng {          // (xorshift64*)
    uint64_t s;
    explicit Rng(uint64_t seed) : s(seed * 0x9E3779B97F4A7C15ull + 1) {}
    uint64_t next() { s ^= s >> 12; s ^= s << 25; s ^= s >> 27; return s * 0x2545F4914F6CDD1Dull; }
    int64_t below(int64_t n) { return (int64_t)(next() % (uint64_t)n); }
};

// ----------------------------------------------------------------------------- (1) the restatement
namespace parent {
constexpr int kCapBlocksMax = 8;
static int64_t capture_count(int64_t nsteps, int64_t every) { return every > 0 ? 1 + (nsteps + every - 1) / every : 0; }
// propagate_fixed_capture's locals and what it leaves in CapRun and the plan (cap_block_bytes of a ring made for this run)
struct Cap { int64_t every, per_block, nsnap, nflush, nsteps; int nblocks; size_t fb, bb; };
static Cap capture(size_t fb, int64_t nsteps, int64_t every, bool fields_host) {
    const int64_t nsnap = capture_count(nsteps, every);
    int64_t per_block = 1, nflush = 0;
    int nblocks = 0;
    size_t bb = 0;
    if (fields_host && nsnap > 2) {
        per_block = (int64_t)std::max<size_t>(1, std::min<size_t>((size_t(8) << 20) / fb, 64));
        per_block = std::min<int64_t>(per_block, nsnap - 2);
        nflush = (nsnap - 2 + per_block - 1) / per_block;
        bb = fb * (size_t)per_block;
        nblocks = (int)std::min<int64_t>(nflush, std::max<int64_t>(2, std::min<int64_t>(kCapBlocksMax, (int64_t)((size_t(1) << 30) / bb))));
    }
    return {fields_host ? every : 0, per_block, nsnap, nflush, nsteps, nblocks, fb, bb};
}
// lane_run at step s with the next snapshot k: does it capture, and then: fl, slot, blk, the byte offset of te.F in cap_blocks, the wait (0: none), "leaves"
struct Slot { bool captures; int64_t fl, slot; int blk; size_t offset; int64_t wait; bool leaves; };
static Slot lane_step(const Cap& cr, int64_t s, int64_t k) {
    const bool snaps = cr.every > 0, last = s + 1 == cr.nsteps;
    if (!(snaps && !last && (s + 1) % cr.every == 0)) return {false, 0, 0, 0, 0, 0, false};
    const int64_t j = k - 1, fl = j / cr.per_block, slot = j % cr.per_block;
    const int blk = (int)(fl % cr.nblocks);
    const int64_t wait = slot == 0 && fl >= cr.nblocks ? fl - cr.nblocks + 1 : 0;
    return {true, fl, slot, blk, cr.bb * (size_t)blk + cr.fb * (size_t)slot, wait, slot == cr.per_block - 1 || k == cr.nsnap - 2};
}
// capture_helper's transfer of flush fl
struct Flush { int64_t first, count; size_t host, ring, bytes; };
static Flush flush(const Cap& cr, int64_t fl) {
    const int64_t first = fl * cr.per_block, count = std::min<int64_t>(cr.per_block, cr.nsnap - 2 - first);
    return {first, count, cr.fb * (size_t)(1 + first), cr.bb * (size_t)(fl % cr.nblocks), cr.fb * (size_t)count};
}
// the scalar log (C = cols_per_tile<T>())
struct Log { int per_row; size_t step_doubles, raw_b, red_b; };
static Log log(int N1, int N2, int E, int C, int batch, int64_t nsteps) {
    const int per_row = (N2 / C) * ((N1 * C / E + 63) / 64);
    const size_t step_doubles = (size_t)batch * per_row * 2, raw_b = sizeof(double) * step_doubles * (size_t)(nsteps + 1);
    const size_t red_b = sizeof(double) * 2 * (size_t)batch * (size_t)(nsteps + 1);
    return {per_row, step_doubles, raw_b, red_b};
}
static size_t scal_at(const Log& l, int64_t step, int row0) { return l.step_doubles * (size_t)step + (size_t)row0 * l.per_row * 2; }
// propagate_fixed's block
static int64_t block(int64_t nsteps, size_t free_b, size_t fb) {
    return (int64_t)std::min<size_t>((size_t)(nsteps + 1), std::max<size_t>(1, std::min<size_t>(free_b / 2, size_t(8) << 30) / fb));
}
// adaptive_set_capture, acap_wants and what the chunk functions did with AdaptCap
struct AdaptCap {
    int64_t every = 0;
    std::vector<int64_t> list;
    size_t next_in_list = 0;
    int64_t capacity = 0, count = 0;
    int half_slots = 0, chunk_no = 0;
    bool wants(int64_t after) {
        if (every > 0) return after % every == 0;
        while (next_in_list < list.size() && list[next_in_list] < after) ++next_in_list;
        return next_in_list < list.size() && list[next_in_list] == after;
    }
    bool room(size_t queued) const { return count + (int64_t)queued < capacity; }
    int half() const { return chunk_no & 1; }
    bool half_in_use() const { return chunk_no >= 2; }
    size_t half_offset(size_t fb) const { return fb * (size_t)half_slots * (size_t)(chunk_no & 1); }
    bool cut(size_t queued, int i) const { return (int)queued >= half_slots || (every == 0 && queued >= 4 && i + 1 >= 64); }
    void sent(int64_t taken) { count += taken; ++chunk_no; }
    void reset() { count = 0; next_in_list = 0; chunk_no = 0; }
};
static bool list_valid(const std::vector<int64_t>& list) {
    for (size_t i = 0; i < list.size(); ++i) if (list[i] < 1 || (i && list[i] <= list[i - 1])) return false;
    return true;
}
static int half_slots(size_t fb) { return (int)std::max<size_t>(1, std::min<size_t>(32, (size_t(512) << 20) / fb)); }
static size_t ring_need(size_t fb) { return fb * (size_t)half_slots(fb) * 2; }
static size_t taken(const std::vector<int64_t>& chunk_caps, int64_t steps) {
    size_t k = 0;
    for (; k < chunk_caps.size(); ++k) if (chunk_caps[k] > steps) break;
    return k;
}
// adaptive_estimate of PlanT<T>
constexpr int kAdaptChunkMax = 512;
template <typename T> int adaptive_estimate(T length, T z, T h) {
    const double remain = h > (T)0 ? ((double)length - (double)z) / (double)h : 1.0;
    const int est = remain > 1e6 ? kAdaptChunkMax : (remain <= 24.0 ? (int)remain + 3 : (int)(0.75 * remain) + 1);
    return est < 2 ? 2 : (est > kAdaptChunkMax ? kAdaptChunkMax : est);
}
// chirpz.hip and manakov.hip
static int line_estimate(double length, double z, double h) {
    const double remain = h > 0 ? (length - (z - h)) / h : 1.0;
    int chunk = remain > 1e6 ? 128 : (int)(0.75 * remain) + 1;
    chunk = chunk < 2 ? 2 : (chunk > 128 ? 128 : chunk);
    return chunk;
}
// the head of adaptive_chunks' loop (acap_on: a capture is set; every = acap.every)
static int chunk_next(int chunk, int64_t budget_left, bool acap_on, int64_t every, int step) {
    if ((int64_t)chunk > budget_left) chunk = (int)budget_left;
    if (acap_on) {
        if (every > 0 && (int64_t)chunk > std::max<int64_t>(64, every * 4)) chunk = (int)std::max<int64_t>(64, every * 4);
        if (every > 0 && (int64_t)chunk > every) {
            const int64_t end = (((int64_t)step + chunk) / every) * every;
            if (end > (int64_t)step) chunk = (int)(end - (int64_t)step);
        }
    }
    return chunk;
}
}  // namespace parent

static std::vector<size_t> field_sizes() {
    std::vector<size_t> v;
    for (int k = 10; k <= 32; ++k) v.push_back(size_t(1) << k);
    for (size_t t : {(size_t(8) << 20) / 64, size_t(8) << 20, size_t(128) << 20, size_t(512) << 20, size_t(1) << 30}) { v.push_back(t - 8); v.push_back(t + 8); }      // (an element: 8 bytes)
    return v;
}

// walk: 2 = lane_run's loop over every step, 1 = over the steps that capture and their neighbours (which steps capture does not depend on the field), 0 = a large run, sampled
static void check_ring(size_t fb, int64_t nsteps, int64_t every, bool fields, int walk) {
    const parent::Cap p = parent::capture(fb, nsteps, every, fields);
    const CapRing r = CapRing::make(fb, nsteps, every, fields);
    CHECK(r.every == p.every && r.per_block == p.per_block && r.nsnap == p.nsnap && r.nflush == p.nflush && r.nblocks == p.nblocks && r.nsteps == p.nsteps && r.fb == p.fb &&
          r.block_bytes == p.bb && r.ring_bytes() == p.bb * (size_t)p.nblocks && capture_count(nsteps, every) == p.nsnap,
          "ring fb=%zu nsteps=%lld every=%lld", fb, (long long)nsteps, (long long)every);
    if (p.nblocks > 0) CHECK(p.bb == fb * (size_t)p.per_block && r.end_offset() == fb * (size_t)(p.nsnap - 1), "end offset");
    auto same_slot = [&](int64_t s, int64_t k) {
        const parent::Slot ps = parent::lane_step(p, s, k);
        CHECK(r.captures(s) == ps.captures, "captures fb=%zu nsteps=%lld every=%lld s=%lld", fb, (long long)nsteps, (long long)every, (long long)s);
        if (!ps.captures) return false;
        const CapSlot c = r.slot_of(k - 1);
        CHECK(c.flush == ps.fl && c.slot == ps.slot && c.block == ps.blk && c.offset == ps.offset && c.wait_flushes == ps.wait && c.leaves == ps.leaves,
              "slot fb=%zu nsteps=%lld every=%lld s=%lld k=%lld", fb, (long long)nsteps, (long long)every, (long long)s, (long long)k);
        return true;
    };
    auto same_flush = [&](int64_t fl) {
        const parent::Flush pf = parent::flush(p, fl);
        const CapFlush f = r.flush_of(fl);
        CHECK(f.first == pf.first && f.count == pf.count && f.host_offset == pf.host && f.ring_offset == pf.ring && f.bytes == pf.bytes && f.block == (int)(fl % p.nblocks),
              "flush fb=%zu nsteps=%lld every=%lld fl=%lld", fb, (long long)nsteps, (long long)every, (long long)fl);
    };
    if (walk) {
        int64_t k = 1;
        if (walk == 2 || p.every <= 0) { for (int64_t s = 0; s < nsteps; ++s) if (same_slot(s, k)) ++k; }
        else for (int64_t s = p.every - 1; s < nsteps; s += p.every) { if (s > 0) same_slot(s - 1, k); if (same_slot(s, k)) ++k; }
        CHECK(k == std::max<int64_t>(1, p.every > 0 ? p.nsnap - 1 : 1), "snapshots written: k=%lld nsnap=%lld", (long long)k, (long long)p.nsnap);
        for (int64_t fl = 0; fl < p.nflush; ++fl) same_flush(fl);
    } else if (p.every > 0) {   // a large run: the steps around the head, the first seams, the first wrap and the end
        for (int64_t k : {(int64_t)1, (int64_t)2, p.per_block, p.per_block + 1, p.per_block * p.nblocks, p.per_block * p.nblocks + 1, p.per_block * (p.nblocks + 1) + 1,
                          p.nsnap / 2, p.nsnap - 3, p.nsnap - 2})
            if (k >= 1 && k <= p.nsnap - 2) { same_slot(k * p.every - 1, k); same_slot(k * p.every, k + 1); same_slot(k * p.every - 2 >= 0 ? k * p.every - 2 : 0, k); }
        same_slot(nsteps - 1, p.nsnap - 1);
        for (int64_t fl : {(int64_t)0, (int64_t)1, (int64_t)p.nblocks, p.nflush / 2, p.nflush - 2, p.nflush - 1}) if (fl >= 0 && fl < p.nflush) same_flush(fl);
    }
}

static void restatement() {
    const std::vector<size_t> fbs = field_sizes();
    for (size_t fb : fbs) {
        for (int64_t nsteps = 1; nsteps <= 700; ++nsteps)
            for (int64_t every = 1; every <= nsteps + 1; ++every) check_ring(fb, nsteps, every, true, fb == fbs[0] ? 2 : 1);
        for (int64_t nsteps : {(int64_t)1, (int64_t)7, (int64_t)700, (int64_t)100000, (int64_t)0x7fffffff}) {
            check_ring(fb, nsteps, 0, false, nsteps <= 700 ? 2 : 0);          // the scalar log alone
            for (int64_t every : {(int64_t)1, (int64_t)2, (int64_t)3, (int64_t)63, (int64_t)64, (int64_t)65, (int64_t)100, (int64_t)99999, (int64_t)100000, (int64_t)100001,
                                  (int64_t)0x7ffffffe, (int64_t)0x7fffffff, (int64_t)0x80000000ll})
                if (nsteps > 700) check_ring(fb, nsteps, every, true, 0);
        }
        // the every-step capture's block, the adaptive ring
        for (int64_t nsteps : {(int64_t)1, (int64_t)2, (int64_t)63, (int64_t)1000, (int64_t)100000, (int64_t)0x7fffffff})
            for (size_t free_b : {size_t(0), size_t(1), fb - 1, fb, 2 * fb - 1, 2 * fb, 2 * fb + 1, 4 * fb, fb * 2 * (size_t)nsteps, fb * 2 * (size_t)(nsteps + 1) - 1, fb * 2 * (size_t)(nsteps + 1),
                                  size_t(16) << 30, (size_t(16) << 30) + 2 * fb, size_t(288) << 30}) {
                const int64_t b = parent::block(nsteps, free_b, fb);
                CHECK(snap_block(nsteps, free_b, fb) == b && snap_whole(b, nsteps) == (b == nsteps + 1), "block nsteps=%lld free=%zu fb=%zu", (long long)nsteps, free_b, fb);
            }
        CHECK(acap_half_slots(fb) == parent::half_slots(fb) && acap_ring_bytes(fb) == parent::ring_need(fb), "adaptive ring fb=%zu", fb);
    }
    // the scalar log
    for (int N1 : {16, 64, 128, 256, 512}) for (int N2 : {16, 64, 1024, 2048, 8192}) for (int E : {4, 8, 16}) for (int batch : {1, 2, 3, 8})
        for (int64_t nsteps : {(int64_t)1, (int64_t)7, (int64_t)1000, (int64_t)0x7fffffff}) {
            const parent::Log p4 = parent::log(N1, N2, E, 16, batch, nsteps), p8 = parent::log(N1, N2, E, 8, batch, nsteps);
            const ScalLog l4 = scal_log<float>(N1, N2, E, batch, nsteps), l8 = scal_log<double>(N1, N2, E, batch, nsteps);
            CHECK(l4.per_row == p4.per_row && l4.step_doubles == p4.step_doubles && l4.raw_bytes == p4.raw_b && l4.red_bytes == p4.red_b && l4.bytes() == p4.raw_b + p4.red_b &&
                  l4.reduced_at() == p4.step_doubles * (size_t)(nsteps + 1), "log c64 %d %d %d", N1, N2, E);
            CHECK(l8.per_row == p8.per_row && l8.step_doubles == p8.step_doubles && l8.raw_bytes == p8.raw_b && l8.red_bytes == p8.red_b && l8.bytes() == p8.raw_b + p8.red_b &&
                  l8.reduced_at() == p8.step_doubles * (size_t)(nsteps + 1), "log c128 %d %d %d", N1, N2, E);
            for (int64_t step : {(int64_t)0, (int64_t)1, nsteps}) for (int row0 = 0; row0 < batch; ++row0)
                CHECK(l4.at(step, row0) == parent::scal_at(p4, step, row0) && l8.at(step, row0) == parent::scal_at(p8, step, row0), "scal_at");
        }
    // list validation and the cursor
    Rng rng(7);
    for (int t = 0; t < 20000; ++t) {
        std::vector<int64_t> list((size_t)(1 + rng.below(12)));
        int64_t v = rng.below(3);
        for (auto& x : list) { v += rng.below(8) == 0 ? rng.below(2) - 1 : 1 + rng.below(9); x = v; }
        const bool ok = parent::list_valid(list);
        CHECK(acap_list_valid(list.data(), (int64_t)list.size()) == ok, "list validation");
        if (!ok) continue;
        parent::AdaptCap p; p.list = list;
        CapCursor c; c.list = list.data(); c.n_list = list.size();
        for (int64_t after = 1; after <= list.back() + 2; after += 1 + (rng.below(5) == 0 ? rng.below(4) : 0)) {
            CHECK(c.wants(after) == p.wants(after) && c.next == p.next_in_list, "list cursor");
            if (rng.below(40) == 0) { c.reset(); p.reset(); after = 0; }
        }
    }
    for (int64_t every : {1, 2, 7, 64}) { parent::AdaptCap p; p.every = every; CapCursor c; c.every = every; for (int64_t a = 1; a < 300; ++a) CHECK(c.wants(a) == p.wants(a), "stride cursor"); }
    // the estimate: the plan's in either precision, the lines'
    CHECK(kAdaptChunkMax == parent::kAdaptChunkMax && kLineChunkMax == 128, "caps");
    std::vector<double> remains = {-3.0, -0.5, 0.0, 0.3, 1.0, 1.3, 1.34, 2.0, 23.0, 23.5, 23.999999, 24.0, 24.000001, 24.5, 25.0, 100.0, 169.0, 170.0, 171.0, 680.0, 681.0, 682.0, 683.0, 1000.0,
                                   999999.0, 1e6, 1000000.5, 1000001.0, 1e7, 1e9, 1e12};
    for (double h : {0.0, -0.0, -1.0, -1e-3, 1e-6, 1e-3, 0.01, 0.37, 1.0, 80.0})
        for (double rem : remains) for (double z : {0.0, 1.0, 12.5}) {
            const double L = z + rem * h;
            const float Lf = (float)L, zf = (float)z, hf = (float)h;
            CHECK(chunk_estimate(L - z, h, kAdaptChunkMax, true) == parent::adaptive_estimate<double>(L, z, h), "estimate double L=%g z=%g h=%g", L, z, h);
            CHECK(chunk_estimate((double)Lf - (double)zf, (double)hf, kAdaptChunkMax, true) == parent::adaptive_estimate<float>(Lf, zf, hf), "estimate float L=%g z=%g h=%g", L, z, h);
            CHECK(chunk_estimate(L - (z - h), h, kLineChunkMax, false) == parent::line_estimate(L, z, h), "line estimate L=%g z=%g h=%g", L, z, h);
        }
    for (double rem : remains) {         // what comes out: the clamps at 2 and at the cap, the tail rule around 24
        const int with = chunk_estimate(rem, 1.0, 512, true), without = chunk_estimate(rem, 1.0, 128, false);
        CHECK(with >= 2 && with <= 512 && without >= 2 && without <= 128, "clamps");
        if (rem > 0 && rem <= 24.0) CHECK(with == std::max(2, (int)rem + 3), "tail"); else if (rem > 24.0) CHECK(with == (rem > 1e6 ? 512 : std::min(512, (int)(0.75 * rem) + 1)), "three quarters");
        if (rem > 0) CHECK(without == (rem > 1e6 ? 128 : std::max(2, std::min(128, (int)(0.75 * rem) + 1))), "no tail");
    }
    CHECK(chunk_estimate(24.0, 1.0, 512, true) == 27 && chunk_estimate(24.5, 1.0, 512, true) == 19 && chunk_estimate(24.0, 1.0, 128, false) == 19 && chunk_estimate(5.0, 0.0, 512, true) == 4 &&
          chunk_estimate(5.0, -1.0, 128, false) == 2 && chunk_estimate(1e7, 1.0, 512, true) == 512 && chunk_estimate(1e7, 1.0, 128, false) == 128, "estimate by hand");
    // the chunk of the next enqueue
    for (int64_t left = 1; left <= 2000; ++left)
        for (int64_t every : {0, 1, 2, 7, 16, 17, 64, 500})
            for (int chunk : {1, 2, 3, 16, 27, 63, 64, 65, 128, 255, 256, 511, 512})
                for (int64_t m : {0, 1, 3}) for (int64_t d = -2; d <= 2; ++d) {
                    const int64_t step = m * (every > 0 ? every : 10) + d;
                    if (step < 0) continue;
                    const int a = chunk_next(chunk, left, every, step);
                    CHECK(a == parent::chunk_next(chunk, left, true, every, (int)step) && a >= 1 && a <= chunk && a <= left, "chunk_next %d %lld %lld %lld", chunk, (long long)left, (long long)every, (long long)step);
                    CHECK(chunk_next(chunk, left, 0, step) == parent::chunk_next(chunk, left, false, every, (int)step), "chunk_next without capture");
                }
}

// ----------------------------------------------------------------------------- (2) the ring under random scheduling
// The producers are lane_run's capture branch, the consumer capture_helper's loop over the flushes; a write stands for the END launch (at the earliest moment
// it could run: when it is enqueued), a flush for the transfer with its wait.  R: captures / slot_of / flush_of and CapRing's fields.
struct Cell { int64_t j = -1; bool flushed = true; };
template <typename R> static const char* ring_model(const R& r, int nlanes, int mode, uint64_t seed) {
    const int64_t interior = r.nsnap - 2;
    if (r.nblocks <= 0) return interior > 0 ? "no ring for a run with snapshots" : nullptr;
    const size_t slots = r.ring_bytes() / r.fb;
    if (r.ring_bytes() % r.fb) return "the ring is no whole number of fields";
    std::vector<std::vector<Cell>> ring((size_t)nlanes, std::vector<Cell>(slots));            // (every lane writes its own rows of a slot)
    std::vector<std::vector<int>> host((size_t)nlanes, std::vector<int>((size_t)r.nsnap, 0));
    std::vector<int64_t> s((size_t)nlanes, 0), k((size_t)nlanes, 1), ends_done((size_t)nlanes, 0);
    int64_t flushes_done = 0, fl = 0;
    Rng rng(seed);
    auto lane_done = [&](int g) { return s[(size_t)g] >= r.nsteps; };
    // one move of lane g: up to and with its next capture step.  false: blocked
    auto lane_move = [&](int g, const char** err) {
        size_t G = (size_t)g;
        for (; s[G] < r.nsteps; ++s[G]) {
            if (!r.captures(s[G])) continue;
            const CapSlot c = r.slot_of(k[G] - 1);
            if (c.wait_flushes > r.nflush) { *err = "a lane waits for more flushes than the run has"; return true; }
            if (c.wait_flushes && flushes_done < c.wait_flushes) return false;
            if (c.offset % r.fb || c.offset + r.fb > r.ring_bytes()) { *err = "a slot outside the ring"; return true; }
            if (c.flush < 0 || c.flush >= r.nflush) { *err = "a snapshot of no flush"; return true; }
            Cell& cell = ring[G][c.offset / r.fb];
            if (!cell.flushed) { *err = "a slot written before its content has left"; return true; }
            cell.j = k[G] - 1; cell.flushed = false;
            if (c.leaves) ends_done[G] = c.flush + 1;
            ++k[G]; ++s[G];
            return true;
        }
        return true;
    };
    auto helper_move = [&](const char** err) {
        for (int g = 0; g < nlanes; ++g) if (ends_done[(size_t)g] < fl + 1) return false;
        const CapFlush f = r.flush_of(fl);
        if (f.count < 1 || f.bytes != r.fb * (size_t)f.count) { *err = "a flush of no whole snapshots"; return true; }
        if (f.ring_offset % r.fb || f.ring_offset + f.bytes > r.ring_bytes()) { *err = "a flush reads outside the ring"; return true; }
        if (f.host_offset % r.fb || f.host_offset < r.fb || f.host_offset + f.bytes > r.fb * (size_t)(r.nsnap - 1)) { *err = "a flush writes outside the interior of the host buffer"; return true; }
        for (int g = 0; g < nlanes; ++g)
            for (int64_t i = 0; i < f.count; ++i) {
                Cell& cell = ring[(size_t)g][f.ring_offset / r.fb + (size_t)i];
                const size_t snap = f.host_offset / r.fb + (size_t)i;
                if (cell.flushed || cell.j != f.first + i || cell.j != (int64_t)snap - 1) { *err = "a flush read something else than its snapshots"; return true; }
                cell.flushed = true;
                ++host[(size_t)g][snap];
            }
        flushes_done = ++fl;
        return true;
    };
    for (long long moves = 0;; ++moves) {
        if (moves > 4 * (r.nsteps + r.nflush + 8) * (nlanes + 1)) return "the model did not end";
        int live[kMaxLanes + 1], nlive = 0;          // (nlanes = the helper)
        for (int g = 0; g < nlanes; ++g) if (!lane_done(g)) live[nlive++] = g;
        if (fl < r.nflush) live[nlive++] = nlanes;
        if (nlive == 0) break;
        // mode 0: a random actor; 1: the lanes run ahead as far as they can; 2: the helper first, the lanes one capture at a time
        if (mode == 0) std::swap(live[0], live[rng.below(nlive)]);
        else if (mode == 2) std::rotate(live, live + nlive - (live[nlive - 1] == nlanes ? 1 : 0), live + nlive);
        bool moved = false;
        const char* err = nullptr;
        for (int a = 0; a < nlive && !moved && !err; ++a) moved = live[a] == nlanes ? helper_move(&err) : lane_move(live[a], &err);
        if (err) return err;
        if (!moved) return "every actor is blocked";
    }
    for (int g = 0; g < nlanes; ++g) {
        if (k[(size_t)g] != r.nsnap - 1) return "a lane wrote another number of snapshots";
        for (int64_t snap = 0; snap < r.nsnap; ++snap)
            if (host[(size_t)g][(size_t)snap] != (snap >= 1 && snap <= r.nsnap - 2 ? 1 : 0)) return "a host snapshot did not arrive exactly once";
    }
    return nullptr;
}
// the mutants
struct WaitShort : CapRing { explicit WaitShort(const CapRing& r) : CapRing(r) {}
    CapSlot slot_of(int64_t j) const { CapSlot c = CapRing::slot_of(j); if (c.wait_flushes) --c.wait_flushes; return c; } };
struct NoPartial : CapRing { explicit NoPartial(const CapRing& r) : CapRing(r) {}
    CapSlot slot_of(int64_t j) const { CapSlot c = CapRing::slot_of(j); c.leaves = c.slot == per_block - 1; return c; } };
struct ModPlusOne : CapRing { explicit ModPlusOne(const CapRing& r) : CapRing(r) {}
    CapSlot slot_of(int64_t j) const { CapSlot c = CapRing::slot_of(j); c.block = (int)(c.flush % (nblocks + 1)); c.offset = block_bytes * (size_t)c.block + fb * (size_t)c.slot; return c; }
    CapFlush flush_of(int64_t fl) const { CapFlush f = CapRing::flush_of(fl); f.block = (int)(fl % (nblocks + 1)); f.ring_offset = block_bytes * (size_t)f.block; return f; } };
struct NoClip : CapRing { explicit NoClip(const CapRing& r) : CapRing(r) {}
    CapFlush flush_of(int64_t fl) const { CapFlush f = CapRing::flush_of(fl); f.count = per_block; f.bytes = fb * (size_t)per_block; return f; } };

static long long ring_runs = 0;
static void ring_models() {
    // the restatement's grid, thinned: the field sizes that change the ring's shape, runs up to 700 steps
    const std::vector<size_t> fbs = {size_t(1) << 10, (size_t(8) << 20) / 64 - 8, (size_t(8) << 20) / 64, (size_t(8) << 20) / 64 + 8, size_t(1) << 18, size_t(1) << 20, (size_t(8) << 20) - 8, size_t(8) << 20,
                                     (size_t(8) << 20) + 8, (size_t(128) << 20) - 8, size_t(128) << 20, (size_t(128) << 20) + 8, size_t(512) << 20, (size_t(512) << 20) + 8, size_t(1) << 30,
                                     (size_t(1) << 30) + 8, size_t(1) << 32};
    int64_t caught[4] = {0, 0, 0, 0}, live[4] = {0, 0, 0, 0};
    for (size_t fb : fbs)
        for (int64_t nsteps = 1; nsteps <= 700; nsteps += nsteps < 40 ? 1 : (nsteps < 140 ? 7 : 43))
            for (int64_t every = 1; every <= nsteps + 1; every += every < 6 ? 1 : (every < 40 ? 5 : 61)) {
                const CapRing r = CapRing::make(fb, nsteps, every, true);
                for (int nl : {1, 2, 8})
                    for (int mode = 0; mode < 3; ++mode)
                        for (uint64_t seed = 0; seed < (mode == 0 ? 3u : 1u); ++seed) {
                            const char* err = ring_model(r, nl, mode, seed * 1000 + (uint64_t)nsteps * 7 + (uint64_t)every);
                            ++ring_runs;
                            CHECK(err == nullptr, "ring model fb=%zu nsteps=%lld every=%lld lanes=%d mode=%d: %s", fb, (long long)nsteps, (long long)every, nl, mode, err ? err : "");
                        }
                if (r.nblocks <= 0) continue;
                // each mutant where it changes something, with the lanes running ahead (mode 1) and two lanes
                const int64_t interior = r.nsnap - 2;
                const bool m_live[4] = {r.nflush > r.nblocks, interior % r.per_block != 0, r.nflush > r.nblocks, interior % r.per_block != 0};
                const char* errs[4] = {m_live[0] ? ring_model(WaitShort(r), 2, 1, 1) : nullptr, m_live[1] ? ring_model(NoPartial(r), 2, 1, 1) : nullptr,
                                       m_live[2] ? ring_model(ModPlusOne(r), 2, 1, 1) : nullptr, m_live[3] ? ring_model(NoClip(r), 2, 1, 1) : nullptr};
                for (int m = 0; m < 4; ++m) if (m_live[m]) { ++live[m]; if (errs[m]) ++caught[m]; CHECK(errs[m] != nullptr, "mutant %d passed: fb=%zu nsteps=%lld every=%lld", m, fb, (long long)nsteps, (long long)every); }
            }
    for (int m = 0; m < 4; ++m) CHECK(live[m] > 50 && caught[m] == live[m], "mutant %d: caught %lld of %lld", m, (long long)caught[m], (long long)live[m]);
    // by hand: 2^14 x 2 complex64 (256 KiB: 32 per block, 8 blocks), every step, 258 steps = the first re-use of a block
    const CapRing r = CapRing::make(size_t(1) << 18, 258, 1, true);
    CHECK(r.per_block == 32 && r.nblocks == 8 && r.nflush == 9 && r.nsnap == 259 && r.slot_of(256).wait_flushes == 1 && r.slot_of(256).block == 0 && r.slot_of(256).leaves && r.slot_of(255).leaves &&
          !r.slot_of(254).leaves && r.flush_of(8).count == 1, "the ring of 258 steps");
    CHECK(std::string(ring_model(WaitShort(r), 1, 1, 0)) == "a slot written before its content has left", "wait one short");
    CHECK(std::string(ring_model(NoPartial(r), 8, 0, 3)) == "every actor is blocked", "no partial block");
    CHECK(std::string(ring_model(ModPlusOne(r), 2, 2, 0)) == "a slot outside the ring", "modulo nblocks + 1");
    CHECK(std::string(ring_model(NoClip(r), 2, 0, 5)) == "a flush writes outside the interior of the host buffer", "count not clipped");
    // (the known oddity, kept: fields above 512 MiB get a ring of two blocks = 2 x the field, more than kCapRingBytes)
    const CapRing big = CapRing::make((size_t(1) << 30) + 8, 10, 1, true);
    CHECK(big.nblocks == 2 && big.ring_bytes() == 2 * ((size_t(1) << 30) + 8) && big.ring_bytes() > kCapRingBytes, "the ring of a field above 512 MiB");
}

// ----------------------------------------------------------------------------- (3) the adaptive loop
// A synthetic run: S steps, step i of size h[i], L their sum.  The loop below is adaptive_run called until the run is done: adaptive_chunks,
// adaptive_enqueue_chunk, adaptive_look, adaptive_send_snapshots and adaptive_fall_back with the launches and copies left out.
struct Run {
    std::vector<double> h;        // S sizes
    int64_t budget = 0;           // per adaptive_run call; 0: the whole run
    int64_t every = 0;            // or the list; both empty: no capture
    std::vector<int64_t> list;
    int64_t capacity = 0;
    size_t fb = size_t(1) << 18;
    int fall_back_at = -1;        // the look behind this chunk (counted over the run) finds that the fused engine gave up
};
struct Trace {
    std::vector<int> chunks;                       // as enqueued
    std::vector<int64_t> cap_step, cap_half, cap_slot;
    std::vector<int64_t> taken;
    int64_t n_taken = 0;
    bool ended = false;
    int worst_caps = 0, least_chunk = 1 << 30;
    bool operator==(const Trace& o) const { return chunks == o.chunks && cap_step == o.cap_step && cap_half == o.cap_half && cap_slot == o.cap_slot && taken == o.taken && n_taken == o.n_taken && ended == o.ended; }
};
struct HeaderRules {
    using Cursor = CapCursor;
    static Cursor cursor(const Run& r) { Cursor c; c.every = r.every; c.list = r.list.data(); c.n_list = r.list.size(); c.capacity = r.capacity; c.half_slots = acap_half_slots(r.fb); return c; }
    static int estimate(double L, double z, double h) { return chunk_estimate(L - z, h, kAdaptChunkMax, true); }
    static int next(int chunk, int64_t left, bool on, int64_t every, int step) { return chunk_next(chunk, left, on ? every : 0, step); }
    static size_t taken(const std::vector<int64_t>& caps, int64_t steps) { return caps_taken(caps.data(), caps.size(), steps); }
};
struct ParentRules {
    using Cursor = parent::AdaptCap;
    static Cursor cursor(const Run& r) { Cursor c; c.every = r.every; c.list = r.list; c.capacity = r.capacity; c.half_slots = parent::half_slots(r.fb); return c; }
    static int estimate(double L, double z, double h) { return parent::adaptive_estimate<double>(L, z, h); }
    static int next(int chunk, int64_t left, bool on, int64_t every, int step) { return parent::chunk_next(chunk, left, on, every, step); }
    static size_t taken(const std::vector<int64_t>& caps, int64_t steps) { return parent::taken(caps, steps); }
};
template <typename Rules> static Trace adaptive_model(const Run& run) {
    Trace t;
    const int64_t S = (int64_t)run.h.size();
    std::vector<double> z((size_t)S + 1, 0.0);
    for (int64_t i = 0; i < S; ++i) z[(size_t)i + 1] = z[(size_t)i] + run.h[(size_t)i];
    const double L = z[(size_t)S];
    const bool on = run.every > 0 || !run.list.empty();
    typename Rules::Cursor cur = Rules::cursor(run);
    t.taken.assign((size_t)std::max<int64_t>(run.capacity, 1), -1);
    struct { int64_t steps = 0; double z = 0, h = 0; bool done = false; } now;
    auto state_at = [&](int64_t enqueued) { now.steps = std::min(enqueued, S); now.z = z[(size_t)now.steps]; now.h = now.steps < S ? run.h[(size_t)now.steps] : run.h[(size_t)S - 1]; now.done = now.steps >= S; };
    int step = 0, chunk_count = 0;
    bool fell_back = false;
    state_at(0);
    for (int calls = 0; !now.done; ++calls) {              // adaptive_run
        if (calls > 100000) return t;
        const int64_t budget = run.budget > 0 ? run.budget : (int64_t)1 << 40, first_step = now.steps;
        int chunk = Rules::estimate(L, now.z, now.h);
        while (!now.done && now.steps - first_step < budget) {
            if (t.chunks.size() > 1000000) return t;
            chunk = Rules::next(chunk, budget - (now.steps - first_step), on, cur.every, step);
            std::vector<int64_t> caps;
            const int64_t half = on ? cur.half() : 0;
            if (on && cur.half_offset(run.fb) != run.fb * (size_t)cur.half_slots * (size_t)half) return t;
            for (int i = 0; i < chunk; ++i, ++step)           // adaptive_enqueue_chunk
                if (on && cur.wants((int64_t)step + 1) && cur.room(caps.size())) {
                    t.cap_step.push_back(step + 1); t.cap_half.push_back(half); t.cap_slot.push_back((int64_t)caps.size());
                    caps.push_back((int64_t)step + 1);
                    if (cur.cut(caps.size(), i)) chunk = i + 1;
                }
            t.chunks.push_back(chunk);
            t.worst_caps = std::max(t.worst_caps, (int)caps.size()); t.least_chunk = std::min(t.least_chunk, chunk);
            state_at(step);                                   // adaptive_look
            const bool gave_up = !fell_back && chunk_count++ == run.fall_back_at;
            if (on && !gave_up) {                             // adaptive_send_snapshots
                const size_t taken = Rules::taken(caps, now.steps);
                for (size_t k = 0; k < taken; ++k) t.taken[(size_t)cur.count + k] = caps[k];
                t.n_taken = cur.count + (int64_t)taken;
                cur.sent((int64_t)taken);
            }
            if (gave_up) {                                    // adaptive_fall_back: the same run again from the start
                fell_back = true;
                if (on) { cur.reset(); t.n_taken = 0; }
                step = 0; state_at(0);
                chunk = Rules::estimate(L, now.z, now.h);
                continue;
            }
            if (!now.done) chunk = Rules::estimate(L, now.z, now.h);
        }
    }
    t.ended = true;
    return t;
}
static long long adaptive_runs = 0;
static void adaptive_models() {
    Rng rng(11);
    for (int trial = 0; trial < 6000; ++trial) {
        Run run;
        const int64_t S = trial < 40 ? 1 + trial : 1 + rng.below(trial % 10 == 0 ? 3000 : 500);
        // piecewise step sizes: a few stretches, shrinking or growing, a short last step now and then
        run.h.resize((size_t)S);
        double h = 0.01 + 0.01 * (double)rng.below(200);
        for (int64_t i = 0, left = 0; i < S; ++i) {
            if (left-- <= 0) { left = 1 + rng.below(S); h *= 0.25 + 0.05 * (double)rng.below(60); if (h < 1e-4) h = 1e-4; }
            run.h[(size_t)i] = h;
        }
        if (rng.below(3) == 0) run.h[(size_t)S - 1] *= 0.01 * (double)(1 + rng.below(100));
        run.budget = rng.below(2) ? 0 : 1 + rng.below(rng.below(2) ? 2000 : 70);
        int64_t demand = 0;
        std::vector<int64_t> wanted;
        const int kind = (int)rng.below(5);          // 0: no capture, 1-2: a stride, 3-4: a list
        if (kind == 1 || kind == 2) {
            const int64_t strides[] = {1, 2, 7, 16, 17, 64, 500};
            run.every = strides[rng.below(7)];
            for (int64_t s = run.every; s <= S; s += run.every) wanted.push_back(s);
        } else if (kind >= 3) {
            int64_t v = 0;
            const int64_t nlist = 1 + rng.below(kind == 3 ? 8 : 300);
            for (int64_t i = 0; i < nlist; ++i) { v += 1 + rng.below(kind == 3 ? 100 : 4); run.list.push_back(v); if (v <= S) wanted.push_back(v); }
        }
        demand = (int64_t)wanted.size();
        const int64_t caps[] = {1, std::max<int64_t>(1, demand / 2), std::max<int64_t>(1, demand - 1), std::max<int64_t>(1, demand), demand + 1, demand + 40};
        run.capacity = kind ? caps[rng.below(6)] : 0;
        const size_t fbs[] = {size_t(1) << 18, size_t(1) << 18, size_t(64) << 20, size_t(300) << 20, (size_t(512) << 20) + 8};      // 32, 32, 8, 1 and 1 slots per half
        run.fb = fbs[rng.below(5)];
        if (rng.below(4) == 0) run.fall_back_at = (int)rng.below(6);
        const Trace a = adaptive_model<HeaderRules>(run), b = adaptive_model<ParentRules>(run);
        ++adaptive_runs;
        CHECK(a.ended && b.ended, "trial %d: the loop did not end", trial);
        CHECK(a == b, "trial %d: the header's loop and the restatement's differ (S=%lld every=%lld budget=%lld)", trial, (long long)S, (long long)run.every, (long long)run.budget);
        CHECK(a.least_chunk >= 1, "trial %d: a chunk of %d steps", trial, a.least_chunk);
        CHECK(a.worst_caps <= acap_half_slots(run.fb), "trial %d: %d captures in a chunk", trial, a.worst_caps);
        long long sum = 0;
        for (int c : a.chunks) sum += c;
        CHECK(sum >= S, "trial %d: %lld steps enqueued of %lld", trial, sum, (long long)S);
        if (kind) {
            const int64_t expect = std::min<int64_t>(demand, run.capacity);
            bool same = a.n_taken == expect;
            for (int64_t i = 0; same && i < expect; ++i) same = a.taken[(size_t)i] == wanted[(size_t)i];
            CHECK(same, "trial %d: taken is not the wanted steps (n_taken %lld, expected %lld; S=%lld every=%lld capacity=%lld)", trial, (long long)a.n_taken, (long long)expect, (long long)S,
                  (long long)run.every, (long long)run.capacity);
            for (size_t i = 0; i < a.cap_slot.size(); ++i) CHECK(a.cap_slot[i] < acap_half_slots(run.fb) && (a.cap_half[i] == 0 || a.cap_half[i] == 1), "trial %d: a capture outside its half", trial);
        } else CHECK(a.cap_step.empty() && a.n_taken == 0, "trial %d: captures without a capture", trial);
    }
}

int main() {
    restatement();
    const long long after_restatement = checked;
    ring_models();
    adaptive_models();
    std::printf("%s: %lld (restatement %lld, ring runs %lld, adaptive runs %lld)\n", failures ? "FAILED" : "ok", checked, after_restatement, ring_runs, adaptive_runs);
    return failures ? 1 : 0;
}
