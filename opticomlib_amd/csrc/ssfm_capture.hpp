// ssfm_capture.hpp -- where a z-resolved capture puts its snapshots and how an adaptive run is cut into chunks: the ring of device blocks of a fixed-step
// capture (ssfm_propagate_fixed_capture), its scalar log, the block of an every-step capture, the two-half ring and the cursor of an adaptive capture
// (ssfm_adaptive_set_capture), and the chunk rules of every adaptive driver -- as pure functions of plain values.  Plain C++ -- no HIP types, no
// environment, no allocation, no threads -- so that a host program can run the ring under any interleaving of its actors and the chunk loop over any
// run (tests/capture_host.cpp, tests/test_capture_cpu.py).  ssfm_host.hip, chirpz.hip and manakov.hip ask; the streams, events, atomics and copies are theirs.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include "ssfm_route.hpp"
namespace ssfm {
// ----------------------------------------------------------------------------- the ring of a fixed-step capture
// Snapshot 0 (the input) and the last one (the end field) go to the host straight from the field; the snapshots in between -- j = snapshot number - 1 --
// are written by the capture steps' END launches into slot j % per_block of device block (j / per_block) % nblocks.  A block leaves for the host as soon
// as it is full ("flush" j / per_block): small blocks (8 MiB; one snapshot of a larger field; 64 snapshots at most) keep the transfers beside the run and
// leave little of them behind its end; a ring of up to eight lets the lanes' threads enqueue that far ahead of the transfers.
constexpr size_t kCapBlockBytes = size_t(8) << 20;
constexpr int64_t kCapBlockSnaps = 64;
constexpr int kCapBlocksMax = 8;
// (what the ring holds at most -- as long as two blocks fit: a ring has two blocks at least, so fields above 512 MiB get one of 2 x the field)
constexpr size_t kCapRingBytes = size_t(1) << 30;

constexpr int64_t capture_count(int64_t nsteps, int64_t every) { return every > 0 ? 1 + (nsteps + every - 1) / every : 0; }

// Snapshot j of the ring: where its END launch writes (`offset`: bytes into the ring), what the lane's thread waits for first (wait_flushes > 0: the block is
// written again -- that many flushes must be complete, their transfers through), and whether the block leaves behind it (it is full, or the run's last: the
// lane records its event behind this END)
struct CapSlot { int64_t flush, slot; int block; size_t offset; int64_t wait_flushes; bool leaves; };
// flush fl as the helper sends it: snapshots first + 1 ... first + count of the caller's buffer, from the start of `block`
struct CapFlush { int64_t first, count; size_t host_offset, ring_offset, bytes; int block; };
struct CapRing {
    size_t fb = 0, block_bytes = 0;
    int64_t nsteps = 0, every = 0, per_block = 1, nsnap = 0, nflush = 0;         // every > 0: snapshots are wanted
    int nblocks = 0;                       // 0: no snapshot between the input and the end field
    static CapRing make(size_t fb, int64_t nsteps, int64_t every, bool fields) {
        CapRing r;
        r.fb = fb; r.nsteps = nsteps; r.every = fields ? every : 0; r.nsnap = capture_count(nsteps, every);
        if (!fields || r.nsnap <= 2) return r;
        r.per_block = (int64_t)std::max<size_t>(1, std::min<size_t>(kCapBlockBytes / fb, (size_t)kCapBlockSnaps));
        r.per_block = std::min<int64_t>(r.per_block, r.nsnap - 2);
        r.nflush = (r.nsnap - 2 + r.per_block - 1) / r.per_block;
        r.block_bytes = fb * (size_t)r.per_block;
        r.nblocks = (int)std::min<int64_t>(r.nflush, std::max<int64_t>(2, std::min<int64_t>(kCapBlocksMax, (int64_t)(kCapRingBytes / r.block_bytes))));
        return r;
    }
    size_t ring_bytes() const { return block_bytes * (size_t)nblocks; }
    // is the field after step s (0-based) a snapshot of the ring (the last step's is the end field: not the ring's)
    bool captures(int64_t s) const { return every > 0 && s + 1 != nsteps && (s + 1) % every == 0; }
    CapSlot slot_of(int64_t j) const {
        const int64_t fl = j / per_block, slot = j % per_block;
        const int blk = (int)(fl % nblocks);
        return {fl, slot, blk, block_bytes * (size_t)blk + fb * (size_t)slot, slot == 0 && fl >= nblocks ? fl - nblocks + 1 : 0, slot == per_block - 1 || j == nsnap - 3};
    }
    CapFlush flush_of(int64_t fl) const {
        const int64_t first = fl * per_block, count = std::min<int64_t>(per_block, nsnap - 2 - first);
        const int blk = (int)(fl % nblocks);
        return {first, count, fb * (size_t)(1 + first), block_bytes * (size_t)blk, fb * (size_t)count, blk};
    }
    size_t end_offset() const { return fb * (size_t)(nsnap - 1); }        // the end field is the last snapshot
};

// ----------------------------------------------------------------------------- the scalar log of a capture run
// A pair of doubles per wavefront of the column kernels, row and step -- [step][row][per_row][2], steps 0 ... nsteps -- and behind them the reduced log, a
// pair per row and step.
struct ScalLog {
    int per_row;
    size_t step_doubles, raw_bytes, red_bytes;
    size_t at(int64_t step, int row0) const { return step_doubles * (size_t)step + (size_t)row0 * per_row * 2; }        // (in doubles, as reduced_at)
    size_t reduced_at() const { return raw_bytes / sizeof(double); }
    size_t bytes() const { return raw_bytes + red_bytes; }
};
template <typename T> ScalLog scal_log(int N1, int N2, int E, int batch, int64_t nsteps) {
    const int per_row = (N2 / cols_per_tile<T>()) * ((N1 * cols_per_tile<T>() / E + 63) / 64);
    const size_t step_doubles = (size_t)batch * per_row * 2;
    return {per_row, step_doubles, sizeof(double) * step_doubles * (size_t)(nsteps + 1), sizeof(double) * 2 * (size_t)batch * (size_t)(nsteps + 1)};
}

// ----------------------------------------------------------------------------- the block of an every-step capture (ssfm_propagate_fixed with snapshots)
// up to half the free device memory, 8 GiB at most, one snapshot at least; nsteps + 1 = the whole capture fits
inline int64_t snap_block(int64_t nsteps, size_t free_bytes, size_t fb) {
    return (int64_t)std::min<size_t>((size_t)(nsteps + 1), std::max<size_t>(1, std::min<size_t>(free_bytes / 2, size_t(8) << 30) / fb));
}
constexpr bool snap_whole(int64_t block, int64_t nsteps) { return block == nsteps + 1; }

// ----------------------------------------------------------------------------- the capture of an adaptive run
// The ring: two halves of up to 32 snapshots, 512 MiB each at most -- 1 GiB in all as long as a half holds one snapshot: a half has one slot at least,
// so fields above 512 MiB get a ring of 2 x the field.  Chunk c writes half c & 1; its transfers run beside chunk c + 1 and are waited for before chunk c + 2.
constexpr int kAcapHalfSlots = 32;
constexpr size_t kAcapHalfBytes = size_t(512) << 20;
inline int acap_half_slots(size_t fb) { return (int)std::max<size_t>(1, std::min<size_t>((size_t)kAcapHalfSlots, kAcapHalfBytes / fb)); }
inline size_t acap_ring_bytes(size_t fb) { return fb * (size_t)acap_half_slots(fb) * 2; }
// a list of capture steps: 1-based (the field AFTER step s), ascending
inline bool acap_list_valid(const int64_t* steps, int64_t n) {
    for (int64_t i = 0; i < n; ++i) if (steps[i] < 1 || (i && steps[i] <= steps[i - 1])) return false;
    return true;
}
// which steps capture, how many snapshots are out, which half of the ring is next
struct CapCursor {
    int64_t every = 0;                 // > 0: a stride; 0: the list
    const int64_t* list = nullptr;     // (the caller's storage)
    size_t n_list = 0, next = 0;
    int64_t capacity = 0, count = 0;   // snapshots the host buffer takes; written to it so far (or queued for it)
    int half_slots = 0, chunk_no = 0;
    bool wants(int64_t after) {
        if (every > 0) return after % every == 0;
        while (next < n_list && list[next] < after) ++next;
        return next < n_list && list[next] == after;
    }
    bool room(size_t queued) const { return count + (int64_t)queued < capacity; }
    int half() const { return chunk_no & 1; }
    bool half_in_use() const { return chunk_no >= 2; }      // the transfers of the chunk before the last read it: NOT the last chunk's, which run beside this one
    size_t half_offset(size_t fb) const { return fb * (size_t)half_slots * (size_t)half(); }
    // the chunk ends behind step i of it: its half is full -- or, a list, there is enough to send (four snapshots, 64 steps)
    bool cut(size_t queued, int i) const { return (int)queued >= half_slots || (every == 0 && queued >= 4 && i + 1 >= 64); }
    void sent(int64_t taken) { count += taken; ++chunk_no; }
    void reset() { count = 0; next = 0; chunk_no = 0; }      // the run starts again (a fall-back)
};
// how many of a chunk's captures were really taken: those queued behind the end of the run (at `steps`) were never written
inline size_t caps_taken(const int64_t* chunk_caps, size_t n, int64_t steps) {
    size_t k = 0;
    while (k < n && chunk_caps[k] <= steps) ++k;
    return k;
}

// ----------------------------------------------------------------------------- the chunks of an adaptive run
// An adaptive run is queued in chunks with a look at the state in between (a look drains the queue: 25-40 us).  About to_go / h steps remain (the step
// only shrinks towards the clamp at L): three quarters of them are queued before the next look, `cap` at most.  `tail`: the last two dozen all at once
// and two more -- launches behind the end of the run find `done` and leave (a few us each), where the looks of a tail of 7, 2, 1 steps cost more.
constexpr int kAdaptChunkMax = 512;          // the plan's chunked engine (with the tail rule)
constexpr int kLineChunkMax = 128;           // the chirp-z and Manakov lines (without: their to_go counts from the start of the last step, z - h)
inline int chunk_estimate(double to_go, double h, int cap, bool tail) {
    const double remain = h > 0 ? to_go / h : 1.0;
    const int est = remain > 1e6 ? cap : (tail && remain <= 24.0 ? (int)remain + 3 : (int)(0.75 * remain) + 1);
    return est < 2 ? 2 : (est > cap ? cap : est);
}
// The chunk of the next enqueue at step `step`, from the estimate (or the chunk before): what the budget leaves; under a strided capture (every > 0)
// short chunks -- a chunk's snapshots only leave at the look behind it, and the transfers should run beside the NEXT chunk's kernels: four snapshots per
// chunk, 64 steps at least -- that end right behind a capture step where they can, so that the snapshot leaves at once (the last ones of a run would
// otherwise travel behind its end).
inline int chunk_next(int chunk, int64_t budget_left, int64_t every, int64_t step) {
    if ((int64_t)chunk > budget_left) chunk = (int)budget_left;
    if (every > 0 && (int64_t)chunk > std::max<int64_t>(64, every * 4)) chunk = (int)std::max<int64_t>(64, every * 4);
    if (every > 0 && (int64_t)chunk > every) {
        const int64_t end = ((step + chunk) / every) * every;
        if (end > step) chunk = (int)(end - step);
    }
    return chunk;
}
}  // namespace ssfm
