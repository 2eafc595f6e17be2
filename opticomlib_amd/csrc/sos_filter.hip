// sos_filter.hip -- zero-phase IIR filtering (cascade of second-order sections, forward-backward) on
// gfx950: the arithmetic behind the reference's LPF / BPF (devices.py:1363-1368, :814-823), i.e.
// scipy.signal.sosfiltfilt(sos, x, axis=-1) with its default odd padding of 3*ntaps samples and
// steady-state initial conditions.
//
// A cascade of NS biquads in direct form II transposed is a linear recurrence with a K = 2*NS state
// per channel.  It is parallelised over time by chunks of L = 12 samples, TWO launches per direction:
//   k_chunk_scan  a thread runs the recurrence over ITS chunk from a ZERO state (the chunk's particular
//                 solution p_c); the 64 chunks of a wavefront are combined by a shuffle scan of the affine
//                 maps s -> M s + p_c (M = A^L, the homogeneous map over one chunk), the 4 wavefronts of
//                 the workgroup through LDS: every chunk gets e_c = its start state if the workgroup's
//                 GROUP of 256 chunks started from zero, the group its total T_g;
//   k_apply       a workgroup first forms the true start state of its group,
//                     S_g = (M^256)^g s_0 + sum_{j<g} (M^256)^(g-1-j) T_j,      s_0 = zi * x_0,
//                 by a reduction over all earlier group totals (each lane multiplies by its own power
//                 (M^256)^lane, a wavefront sums with shuffles and applies (M^16384)^a); then a thread
//                 forms its chunk's start state M^(c mod 256) S_g + e_c, re-runs the chunk and writes
//                 the outputs.  The reduction is O(groups^2) over the grid -- 342 groups per 2^20-sample
//                 row, nothing against the sample work -- and replaces a separate, serial scan kernel
//                 (measured 25 us of a 127 us call).
// The powers M^j, (M^256)^j, (M^16384)^j, j = 0..64, are built once per filter on the host from M, which
// itself comes from running the same recurrence on unit states.  A wavefront's 64 chunks are 768
// consecutive samples: they are read (and the outputs written) with coalesced accesses and transposed
// through LDS, so that a thread still walks ITS chunk in order.  Inside a chunk the operation order is
// exactly SciPy's sample loop (fp contraction off); only the chunk start states see a different
// summation order (relative 1e-16 effects).  A complex row is two real channels with the same real
// coefficients, carried by ONE thread (16-byte accesses).  float64 throughout, like SciPy.
//
// Traffic per real sample: forward 8 (chunk) + 8 + 8 (apply: read x, write y1), backward the same
// = 48 B against the algorithmic 16 B (read x once, write y once).
//
// That is the THREE-LAUNCH form (orders 5-8 of long calls, SSFM_SOS_ONE_LAUNCH=0, and the fallback).  Calls whose workgroups are all resident at
// once take ONE launch (k_filtfilt, sos_filter_impl.inc): a workgroup keeps its chunks in registers / LDS from the first load to the last store and
// meets the others twice through the group totals -- 16 B per real sample.  Round 5: the totals of orders up to 4 cross as 16-byte units {value, tag}
// that carry their own validity (no flag, no acknowledgement awaited), the wavefront scan runs inside DPP rows; 32-33 us for 2^20 x 2 complex128
// (profiles/r05_sos_handover_ab.txt).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <vector>

#include "ssfm_common.hpp"
#include "ssfm_owned.hpp"
#include "sos_route.hpp"
#include "sos_tables.hpp"

using ssfm::fail;
using ssfm::kMaxDevices;

namespace {

using namespace ssfm::sos;          // the constants (kWave, the chunk lengths, the wavefront counts, ...), the routes and the tables: sos_route.hpp, sos_tables.hpp

#ifndef SOS_SMALL_EU
#define SOS_SMALL_EU 1
#endif
#ifndef SOS_SMALL_AHEAD
#define SOS_SMALL_AHEAD 1
#endif

struct SosCoefs {
    double b0[kMaxSections], b1[kMaxSections], b2[kMaxSections], a1[kMaxSections], a2[kMaxSections];
};

// The 16-byte sample stores go out write-through (sc1), as the propagator's do -- the next kernel's readers sit on
// other CUs, so a dirty line in this XCD's L2 only adds a flush at the kernel boundary.  2^20 x 2 complex: 90.5 -> 87.5 us,
// other shapes unchanged; non-temporal loads measured 4 % slower (profiles/r02_sosfilt_policy_ab.txt).
// One direction of the forward-backward pass.  Rows hold CH interleaved channels.
struct SosPass {
    const double* src;      // forward: caller's x; backward: y1 (padded forward output, [row][m][CH])
    long long n;            // original samples per row
    long long m;            // padded length n + 2*edge
    long long mv;           // length of the sequence the pass runs over: forward m; backward the whole chunk grid, ngroups * group * kChunk >= m:
                            // the backward sequence is b[i'] = y1[min(mv - 1 - i', m - 1)] -- it STARTS with mv - m copies of y1[m - 1], under which
                            // the initial state zi * y1[m - 1] (scipy: zi * y[-1]) stays where it is (steady state) -- so that backward chunk c'
                            // is forward chunk (chunks - 1 - c') sample for sample, and the forward output pass can run the backward chunk pass
                            // on the outputs it holds in registers
    int edge;
    int backward;
};


namespace chunk_short {
constexpr int kChunk = kChunkShort;
#include "sos_filter_impl.inc"
}  // namespace chunk_short
namespace chunk_long {
constexpr int kChunk = kChunkLong;
#include "sos_filter_impl.inc"
}  // namespace chunk_long

// ---------------------------------------------------------------------------------------------- host
// Scratch memory of the filter, one set per device, grown on demand and kept (a hipMalloc/hipFree pair
// per call cost more than the kernels).  Calls on one device are serialised by `mu`.
struct Workspace {
    std::mutex mu;
    ssfm::Stream stream;
    ssfm::Event ev0, ev1;
    ssfm::DeviceBuffer<double> x_stage;      // a host call's input, and its result over it
    ssfm::DeviceBuffer<double> y1;           // the padded forward output [row][m][CH]; the one-launch form's result where it may not land on the caller's buffer
    ssfm::DeviceBuffer<double> E, E_back;    // three launches: every chunk's start state in a group that starts from zero, forward and backward
    ssfm::DeviceBuffer<double> T;            // ... and the groups' totals, forward then backward
    ssfm::DeviceBuffer<double> tables;       // sos_tables.hpp TableLayout, for the filter and shape of `table_key`
    std::vector<double> table_key;           // sos coefficients, zi, wavefronts and chunk the device tables were built for
    int look = 1 << 30;                      // powers of the group map that matter for that filter (sos_route.hpp look_of_group_powers)
    float last_ms = 0.f;
    // one-launch form (k_filtfilt): group totals + their flags, the call counter the flags are compared with, the host-visible give-up word
    ssfm::DeviceBuffer<double> link_T;
    ssfm::DeviceBuffer<unsigned> link_flag;
    ssfm::DeviceBuffer<unsigned long long> link_U;     // totals that carry their own validity: 16-byte units {value, tag} (sos_filter_impl.inc group_start)
    unsigned long long link_tag = 0;         // the call counter the tags are; never repeated, never 0
    unsigned epoch = 0;
    int* status = nullptr;                   // 64 bytes the kernels write in place: hipHostMallocMapped, which ssfm::PinnedBuffer does not ask for -- so it stays raw
    ssfm::DeviceBuffer<double> meet_tab;     // the single-meeting kernels' maps (sos_tables.hpp MeetLayout), for the filter and row end of `meet_key`
    std::vector<double> meet_key;
    GiveUps gave;                            // sos_route.hpp
    int last_launches = 0;
    int last_route[8] = {0, 0, 0, 0, 0, 0, 0, 0};     // what the last call ran (ssfm_sosfiltfilt_last_route; sos_route.hpp fill_route)
};
// Made once and never destroyed: at process exit the owners above would call hipFree / hipStreamDestroy when the runtime may already be gone.
Workspace& workspace(int device) {
    static Workspace* const all = new Workspace[kMaxDevices];
    return all[device];
}

#define WS_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return fail(SSFM_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); } while (0)

// One call: what the caller gave, and the knobs as the environment holds them now
struct Call {
    const SosCoefs& c;
    const double *sos_key, *zi_h, *x;
    double* y;
    long long n;
    int rows, edge;
    bool on_device;
    Knobs kn;
};
// ... and what `prepare` settles for both forms
struct Prepared {
    Geometry g;
    size_t xbytes;
    const double* d_x;
    double* d_out;       // where the three-launch form writes: the caller's buffer, or the staged input of a host call
};

// SSFM_SOS_MEET=1 is built for the verdict of round 5, correct (the parity tests run it), and NOT the default: the wait it saves (2.8 us at 2^20 x 2 once the look-back
// is near) is paid back by the second pass over the forward outputs and by the contention of workgroups that no wait takes out of step any more -- 27.7-28.8 us
// against 26.8-27.2 (profiles/r06_sos_meet_ab.txt).  SSFM_SOS_PATIENCE_US: default 2 ms.
Knobs read_knobs() {
    Knobs kn;
    if (const char* e = std::getenv("SSFM_SOS_ONE_LAUNCH")) kn.one_launch = std::atoi(e) != 0;
    if (const char* e = std::getenv("SSFM_SOS_NEAR")) kn.near = e[0] != '0';
    if (const char* e = std::getenv("SSFM_SOS_MEET")) kn.meet = e[0] == '1';
    if (const char* e = std::getenv("SSFM_SOS_LONG_CHUNK")) kn.long_chunk = std::atoi(e) != 0;
    if (const char* e = std::getenv("SOS_WAVES_FORCE")) { const int v = std::atoi(e); kn.waves_force = v ? v : -1; }      // (set: never "not set", whatever it holds)
    if (const char* e = std::getenv("SSFM_SOS_PATIENCE_US")) { const long long v = std::atoll(e); if (v > 0) kn.patience = v * 100; }
    return kn;
}

// Refusals, scratch, the filter's tables (rebuilt only when the filter or the shape changes), a host call's input staged
template <class I, int NS, int CH, int W>
int prepare(Workspace& w, const Call& a, Prepared& pr) {
    constexpr int K = 2 * NS, kGroup = kWave * W;
    using Lay = TableLayout<NS, I::chunk>;
    const Geometry g = geometry(a.n, a.edge, I::chunk, W);
    switch (refusal(g, a.rows)) {
        case kTooLong: return fail(SSFM_ERR_UNSUPPORTED, "ssfm_sosfiltfilt: n=%lld too long", a.n);
        case kTooManyGroups: return fail(SSFM_ERR_UNSUPPORTED, "ssfm_sosfiltfilt: n=%lld exceeds %d samples per row", a.n, kWave * kWave * kGroup * I::chunk - 2 * a.edge);
        case kTooManyWorkgroups: return fail(SSFM_ERR_UNSUPPORTED, "ssfm_sosfiltfilt: %d rows of %lld samples exceed the grid", a.rows, a.n);
        case kFits: break;
    }
    pr.g = g;
    pr.xbytes = sizeof(double) * (size_t)a.n * a.rows * CH;
    if (!w.stream) {
        WS_TRY(hipStreamCreateWithFlags(w.stream.out(), hipStreamNonBlocking));
        WS_TRY(hipEventCreate(w.ev0.out()));
        WS_TRY(hipEventCreate(w.ev1.out()));
    }
    const size_t states = sizeof(double) * (size_t)g.ngroups * kGroup * a.rows * CH * K;
    if (!a.on_device) WS_TRY(w.x_stage.reserve(pr.xbytes));
    WS_TRY(w.y1.reserve(sizeof(double) * (size_t)g.m * a.rows * CH));
    WS_TRY(w.E.reserve(states));
    WS_TRY(w.T.reserve(sizeof(double) * (size_t)g.ngroups * a.rows * CH * K * 2));
    WS_TRY(w.E_back.reserve(states));
    WS_TRY(w.tables.reserve(sizeof(double) * Lay::total));
    std::vector<double> key(a.sos_key, a.sos_key + 6 * NS);
    key.insert(key.end(), a.zi_h, a.zi_h + K);
    key.push_back((double)W);                              // the group map is (M^64)^W
    key.push_back((double)I::chunk);                       // the chunk map is A^chunk
    if (key != w.table_key) {
        std::vector<double> tab;
        build_tables<NS, W, I::chunk>(a.c, a.zi_h, tab);
        WS_TRY(hipMemcpyAsync(w.tables.get(), tab.data(), sizeof(double) * tab.size(), hipMemcpyHostToDevice, w.stream));
        WS_TRY(hipStreamSynchronize(w.stream));            // `tab` is a local
        w.table_key = key;
        w.look = look_of_group_powers(tab.data() + Lay::pwG, K);
    }
    pr.d_x = a.x;
    pr.d_out = a.y;
    if (!a.on_device) {
        WS_TRY(hipMemcpyAsync(w.x_stage.get(), a.x, pr.xbytes, hipMemcpyHostToDevice, w.stream));
        pr.d_x = w.x_stage;
        pr.d_out = w.x_stage;          // the backward pass writes the trimmed result over the staged input
    }
    return SSFM_OK;
}

// A link buffer that grows starts zero-filled, on the filter's stream (no tag and no epoch is 0); one that could not be filled is let go, so that the next call makes it anew.
template <class E> int reserve_zeroed(ssfm::DeviceBuffer<E>& b, size_t bytes, hipStream_t stream, bool* grew = nullptr) {
    if (b.get() && bytes <= b.capacity()) return SSFM_OK;
    WS_TRY(b.reserve(bytes));
    const hipError_t e = hipMemsetAsync(b.get(), 0, bytes, stream);
    if (e != hipSuccess) { b.free(); return fail(SSFM_ERR_HIP, "hipMemsetAsync of a link buffer failed: %s", hipGetErrorString(e)); }
    if (grew) *grew = true;
    return SSFM_OK;
}

// The one-launch form's buffers for a grid of `blocks` workgroups whose totals are N doubles, and this call's epoch
int link_buffers(Workspace& w, size_t blocks, size_t N) {
    WS_TRY(w.link_T.reserve(sizeof(double) * 2 * blocks * N));
    bool new_flags = false;
    if (int rc = reserve_zeroed(w.link_flag, sizeof(unsigned) * 2 * blocks, w.stream, &new_flags)) return rc;
    if (new_flags) w.epoch = 0;
    if (int rc = reserve_zeroed(w.link_U, sizeof(unsigned long long) * 2 * blocks * N * 2, w.stream)) return rc;      // tagged totals: 16 bytes per value
    if (!w.status) WS_TRY(hipHostMalloc(&w.status, 64, hipHostMallocMapped));
    if (++w.epoch == 0) {                                  // (the counter wrapped: old flags could match again)
        WS_TRY(hipMemsetAsync(w.link_flag.get(), 0, w.link_flag.capacity(), w.stream));
        w.epoch = 1;
    }
    return SSFM_OK;
}

// The single-meeting kernels' maps of this filter, shape and row end, cached by `meet_key`
template <class I, int NS, int W>
int meet_tables(Workspace& w, const Call& a, const Geometry& g, typename I::Link& L) {
    using Lay = MeetLayout<NS, W>;
    // the maps of the row's last group depend on where the padded row ends inside it
    const long long jl = (g.m - 1) - (g.ngroups - 1) * kWave * W * I::chunk;
    std::vector<double> mkey(w.table_key);
    mkey.push_back((double)jl);
    if (mkey != w.meet_key) {
        if (sizeof(double) * Lay::total > w.meet_tab.capacity()) {
            w.meet_key.clear();
            WS_TRY(w.meet_tab.reserve(sizeof(double) * Lay::total));
        }
        std::vector<double> mt;
        build_meet_tables<NS, W, I::chunk>(a.c, a.zi_h, jl, mt);
        // (if the upload fails, meet_key keeps the previous filter's key over a buffer that may hold part of this one's maps: as it always was)
        WS_TRY(hipMemcpyAsync(w.meet_tab.get(), mt.data(), sizeof(double) * mt.size(), hipMemcpyHostToDevice, w.stream));
        WS_TRY(hipStreamSynchronize(w.stream));
        w.meet_key = mkey;
    }
    L.meetV = w.meet_tab + Lay::Vm;
    L.meetW = w.meet_tab + Lay::Wm;
    return SSFM_OK;
}

#if SOS_TIMELINE
// Dev aid (SOS_TIMELINE_DUMP set): the buffer of the workgroups' clock readings ...
int timeline_buffer(unsigned blocks, long long*& tl) {
    static long long* d_tl = nullptr; static size_t tl_cap = 0;
    if (!std::getenv("SOS_TIMELINE_DUMP")) return SSFM_OK;
    if (tl_cap < blocks) { if (d_tl) (void)hipFree(d_tl); WS_TRY(hipMalloc(&d_tl, sizeof(long long) * 16 * blocks)); tl_cap = blocks; }
    tl = d_tl;
    return SSFM_OK;
}
// ... and what they say.  Per phase: when the first, the median and the last workgroup got there, in us after the first workgroup's start; then a few workgroups' own lines
int timeline_dump(const long long* tl, unsigned blocks) {
    if (!tl) return SSFM_OK;
    std::vector<long long> h((size_t)16 * blocks);
    WS_TRY(hipMemcpy(h.data(), tl, sizeof(long long) * h.size(), hipMemcpyDeviceToHost));
    long long t0 = h[0];
    for (unsigned b = 0; b < blocks; ++b) t0 = h[(size_t)b * 16] < t0 ? h[(size_t)b * 16] : t0;
    static const char* names[14] = {"start", "loaded", "chunk sums", "scanned", "total stored", "flag raised", "forward start state", "forward outputs",
                                    "backward scanned", "backward flag raised", "backward start state", "backward outputs", "end", "(forward chunk state)"};
    constexpr int kMarks = 14;
    for (int i = 0; i < kMarks; ++i) {
        std::vector<double> v;
        for (unsigned b = 0; b < blocks; ++b) v.push_back((h[(size_t)b * 16 + i] - t0) * 0.01);
        std::sort(v.begin(), v.end());
        std::fprintf(stderr, "%2d %-22s first %6.2f  median %6.2f  last %6.2f us\n", i, names[i], v.front(), v[v.size() / 2], v.back());
    }
    const char* path = std::getenv("SOS_TIMELINE_DUMP");
    if (path && path[0] == '/') {          // every workgroup: index, HW_ID, XCC_ID, the marks in us
        if (FILE* f = std::fopen(path, "w")) {
            for (unsigned b = 0; b < blocks; ++b) {
                std::fprintf(f, "%u %lld %lld", b, h[(size_t)b * 16 + 14], h[(size_t)b * 16 + 15] & 0xf);
                for (int i = 0; i < kMarks; ++i) std::fprintf(f, " %.2f", (h[(size_t)b * 16 + i] - t0) * 0.01);
                std::fprintf(f, "\n");
            }
            std::fclose(f);
        }
    }
    for (unsigned b = 0; b < blocks; b += blocks / 6 ? blocks / 6 : 1) {
        std::fprintf(stderr, "  workgroup %4u:", b);
        for (int i = 0; i < kMarks; ++i) std::fprintf(stderr, " %6.2f", (h[(size_t)b * 16 + i] - t0) * 0.01);
        std::fprintf(stderr, "\n");
    }
    return SSFM_OK;
}
#endif

// One launch, when the whole grid is resident at once.  The result never lands on the input (a call that gives up is repeated
// from it): an in-place call's goes to the scratch buffer first and is copied over the input afterwards.  `gave_up`: part of the
// grid never ran beside the rest -- the caller runs three launches from the untouched input.
template <class I, int NS, int CH, int W>
int one_launch(Workspace& w, const Call& a, const Prepared& pr, const Form& f, bool& gave_up) {
    constexpr int K = 2 * NS;
    using Lay = TableLayout<NS, I::chunk>;
    const dim3 grid((unsigned)(pr.g.ngroups * a.rows));
    const bool overlap = a.on_device && !(reinterpret_cast<const char*>(a.y) + pr.xbytes <= reinterpret_cast<const char*>(a.x) ||
                                          reinterpret_cast<const char*>(a.x) + pr.xbytes <= reinterpret_cast<const char*>(a.y));
    if (int rc = link_buffers(w, grid.x, CH * K)) return rc;
    *w.status = 0;
    typename I::Link L;
    L.T = w.link_T; L.flag = w.link_flag; L.status = w.status; L.epoch = w.epoch; L.patience = a.kn.patience;
    L.U = w.link_U; L.tag = ++w.link_tag;
    L.pwT = w.tables + Lay::pwT; L.pwGT = w.tables + Lay::pwGT;
    L.tl = nullptr;
    L.look = f.look;
    L.meetV = nullptr; L.meetW = nullptr;
    if (f.meet)
        if (int rc = meet_tables<I, NS, W>(w, a, pr.g, L)) return rc;
#if SOS_TIMELINE
    if (int rc = timeline_buffer(grid.x, L.tl)) return rc;
#endif
    double* const d_res = (!a.on_device || overlap) ? w.y1.get() : a.y;
    SosPass p;
    p.n = a.n; p.m = pr.g.m; p.edge = a.edge;
    p.backward = 0; p.src = pr.d_x; p.mv = pr.g.m;
    WS_TRY(hipEventRecord(w.ev0, w.stream));
    I::template launch_one<NS, CH, W>(f.meet, grid, w.stream, a.c, p, (int)pr.g.nchunks, (int)pr.g.ngroups, w.tables, d_res, L);
    WS_TRY(hipGetLastError());
    WS_TRY(hipEventRecord(w.ev1, w.stream));
    if (!a.on_device) WS_TRY(hipMemcpyAsync(a.y, d_res, pr.xbytes, hipMemcpyDeviceToHost, w.stream));
    WS_TRY(hipStreamSynchronize(w.stream));
    gave_up = *w.status != 0;
    if (!gave_up && a.on_device && overlap) {
        WS_TRY(hipMemcpyAsync(a.y, d_res, pr.xbytes, hipMemcpyDeviceToDevice, w.stream));
        WS_TRY(hipStreamSynchronize(w.stream));
    }
#if SOS_TIMELINE
    if (int rc = timeline_dump(L.tl, grid.x)) return rc;
#endif
    if (!gave_up) WS_TRY(hipEventElapsedTime(&w.last_ms, w.ev0, w.ev1));
    return SSFM_OK;
}

// One stream: splitting the rows over two streams (as the propagator does) was measured SLOWER here
// (145 vs 121 us for 2 x 2^20 complex) -- every kernel is a short latency chain, not a bandwidth phase.
template <class I, int NS, int CH, int W>
int three_launches(Workspace& w, const Call& a, const Prepared& pr) {
    const dim3 grid((unsigned)(pr.g.ngroups * a.rows));
    SosPass p;
    p.n = a.n; p.m = pr.g.m; p.edge = a.edge;
    WS_TRY(hipEventRecord(w.ev0, w.stream));
    I::template launch_three<NS, CH, W>(grid, w.stream, a.c, p, (int)pr.g.nchunks, (int)pr.g.ngroups, a.rows, w.tables, pr.d_x, w.y1, w.E, w.T, w.E_back, pr.d_out);
    WS_TRY(hipGetLastError());
    WS_TRY(hipEventRecord(w.ev1, w.stream));
    if (!a.on_device) WS_TRY(hipMemcpyAsync(a.y, w.x_stage.get(), pr.xbytes, hipMemcpyDeviceToHost, w.stream));
    WS_TRY(hipStreamSynchronize(w.stream));
    WS_TRY(hipEventElapsedTime(&w.last_ms, w.ev0, w.ev1));
    return SSFM_OK;
}

// A call in the shape run_filter chose: which form it takes (sos_route.hpp choose_form), that form, and the give-up state after it
template <class I, int NS, int CH, int W>
int run_filter_w(Workspace& w, const Call& a) {
    Prepared pr;
    if (int rc = prepare<I, NS, CH, W>(w, a, pr)) return rc;
    const Shape shape{I::chunk, W};
    w.gave = tick_before_form(w.gave);
    // (the single-meeting instance is named first, and in run_filter the instances in their order: the order of first naming is the kernels' order in the code object, kept as it was)
    const auto capacity_meet = [](int, int) -> long long { if constexpr (CH * 2 * NS <= 8) return I::template one_launch_capacity<NS, CH, W, true>(); else return 0; };
    const auto capacity = [](int, int) { return I::template one_launch_capacity<NS, CH, W>(); };
    Form form = choose_form(shape, pr.g, NS, CH, a.rows, a.kn, w.gave.give_ups, w.look, capacity, capacity_meet);
    if (form.launches == 1) {
        bool gave_up = false;
        if (int rc = one_launch<I, NS, CH, W>(w, a, pr, form, gave_up)) return rc;
        w.gave = after_one_launch(w.gave, gave_up);
        if (gave_up) form = Form{};                         // (the three-launch form sums all totals and has neither tags nor flags)
    }
    w.last_launches = form.launches;
    fill_route(w.last_route, shape, form, NS, CH);
    return form.launches == 1 ? SSFM_OK : three_launches<I, NS, CH, W>(w, a, pr);
}

// the device's compute units, 0 while unknown
int compute_units() {
    static int cus = 0;
    if (!cus) { int dev = 0, v = 0; if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess) cus = v; }
    return cus;
}

// The workgroup shape and the chunk length follow the size of the call: the knobs are in `a`, sos_route.hpp choose_shape decides, the instance of that shape runs.
template <int NS, int CH>
int run_filter(Workspace& w, const Call& a) {
    using S = chunk_short::Instances;
    using L = chunk_long::Instances;
    struct Instance { Shape shape; long long (*capacity)(); int (*run)(Workspace&, const Call&); };
    // One wavefront of the short chunk unless the dispatcher names one of the others.  (That instance is named before the table, and each of the others' capacity
    // before its call: the order in which a translation unit first names the kernel instances is their order in the code object, and this is the order it always was.)
    int (*run)(Workspace&, const Call&) = run_filter_w<S, NS, CH, kWavesSmall>;
    static const Instance others[3] = {{{kChunkLong, kWavesSmall}, L::one_launch_capacity<NS, CH, kWavesSmall>, run_filter_w<L, NS, CH, kWavesSmall>},
                                       {{kChunkShort, kWavesLarge}, S::one_launch_capacity<NS, CH, kWavesLarge>, run_filter_w<S, NS, CH, kWavesLarge>},
                                       {{kChunkLong, kWavesLarge}, L::one_launch_capacity<NS, CH, kWavesLarge>, run_filter_w<L, NS, CH, kWavesLarge>}};
    const auto is = [](const Instance& i, int chunk, int W) { return i.shape.chunk == chunk && i.shape.W == W; };
    const auto capacity = [&](int chunk, int W) {
        if (chunk == kChunkShort && W == kWavesSmall) return S::one_launch_capacity<NS, CH, kWavesSmall>();
        for (const Instance& i : others) if (is(i, chunk, W)) return i.capacity();
        return 0ll;
    };
    const Shape s = choose_shape(a.c, NS, CH, a.n, a.rows, a.edge, a.kn, w.gave.give_ups, compute_units(), capacity);
    if (!(s.chunk == kChunkShort && s.W == kWavesSmall))
        for (const Instance& i : others) if (is(i, s.chunk, s.W)) { run = i.run; break; }
    return run(w, a);
}

int sosfiltfilt_impl(int device, const double* sos, const double* zi, int n_sections, const void* x, void* y,
                     int64_t n, int batch, int is_complex, bool on_device) {
    if (!sos || !zi || !x || !y) return fail(SSFM_ERR_INVALID, "ssfm_sosfiltfilt: NULL argument");
    if (n_sections < 1 || n_sections > kMaxSections)
        return fail(SSFM_ERR_UNSUPPORTED, "ssfm_sosfiltfilt: %d sections (supported: 1..%d)", n_sections, kMaxSections);
    if (batch < 1 || n < 1) return fail(SSFM_ERR_INVALID, "ssfm_sosfiltfilt: batch=%d n=%lld", batch, (long long)n);
    SosCoefs c;
    std::memset(&c, 0, sizeof(c));
    int zb = 0, za = 0;
    for (int s = 0; s < n_sections; ++s) {
        const double* r = sos + 6 * s;
        if (r[3] != 1.0) return fail(SSFM_ERR_INVALID, "ssfm_sosfiltfilt: section %d has a0 = %g (must be 1)", s, r[3]);
        c.b0[s] = r[0]; c.b1[s] = r[1]; c.b2[s] = r[2]; c.a1[s] = r[4]; c.a2[s] = r[5];
        zb += r[2] == 0.0; za += r[5] == 0.0;
    }
    const int ntaps = 2 * n_sections + 1 - (zb < za ? zb : za);       // scipy sosfiltfilt
    const int edge = 3 * ntaps;
    if (n <= edge) return fail(SSFM_ERR_INVALID, "The length of the input vector x must be greater than padlen, which is %d.", edge);
    if (is_complex && on_device && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15))
        return fail(SSFM_ERR_INVALID, "ssfm_sosfiltfilt_device: complex buffers must be 16-byte aligned");
    if (int rc = ssfm::use_device(device)) return rc;
    Workspace& w = workspace(device);
    std::lock_guard<std::mutex> lock(w.mu);
    const Call a{c, sos, zi, static_cast<const double*>(x), static_cast<double*>(y), n, batch, edge, on_device, read_knobs()};
#define SOS_CASE(NS) case NS: return is_complex ? run_filter<NS, 2>(w, a) : run_filter<NS, 1>(w, a);
    switch (n_sections) {
        SOS_CASE(1) SOS_CASE(2) SOS_CASE(3)
        default: return is_complex ? run_filter<4, 2>(w, a) : run_filter<4, 1>(w, a);
    }
#undef SOS_CASE
}

}  // namespace

extern "C" int ssfm_sosfiltfilt(int device, const double* sos, const double* zi, int n_sections, const void* x, void* y,
                                int64_t n, int batch, int is_complex, int on_device) {
    return sosfiltfilt_impl(device, sos, zi, n_sections, x, y, n, batch, is_complex, on_device != 0);
}

extern "C" int ssfm_sosfiltfilt_last(int device, float* ms, int* launches) {
    if (device < 0 || device >= kMaxDevices) return fail(SSFM_ERR_NO_DEVICE, "ssfm_sosfiltfilt_last: device %d", device);
    Workspace& w = workspace(device);
    std::lock_guard<std::mutex> lock(w.mu);
    if (ms) *ms = w.last_ms;
    if (launches) *launches = w.last_launches;
    return SSFM_OK;
}

extern "C" int ssfm_sosfiltfilt_last_route(int device, int* route) {
    if (device < 0 || device >= kMaxDevices) return fail(SSFM_ERR_NO_DEVICE, "ssfm_sosfiltfilt_last_route: device %d", device);
    if (!route) return fail(SSFM_ERR_INVALID, "ssfm_sosfiltfilt_last_route: NULL argument");
    Workspace& w = workspace(device);
    std::lock_guard<std::mutex> lock(w.mu);
    for (int i = 0; i < 8; ++i) route[i] = w.last_route[i];
    return SSFM_OK;
}
