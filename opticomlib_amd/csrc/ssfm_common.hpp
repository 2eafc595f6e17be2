// ssfm_common.hpp -- error reporting, the device check, grid sizes and per-call scratch shared by the translation units of _ssfm_amd.so
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>

#include "ssfm_amd.h"

namespace ssfm {

inline thread_local char g_err[512] = "";

inline int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

// ---- entry points of ssfm_host.hip that the library's other translation units use and the C ABI does NOT export (hidden visibility).  Round 5: the
// chirp-z step fragments -- round 4's ABI exported twelve of them, which only devices.py could sequence correctly; the exported surface is now
// ssfm_chirp_setup / _propagate / _propagate_c64 / _transfer / _fourier (csrc/chirpz.hip).
#define SSFM_INTERNAL __attribute__((visibility("hidden")))
// A chirp-z step's two ends folded into the first and the last column launch (TM_BEGIN / TM_END with ChirpIO, ssfm_kernels.hpp): the caller's field A, `n`
// complex128 per row, is read and written directly.  h_dev (nullable, DEVICE double): hh = *h_dev / 2 instead of `hh`; done_dev (nullable, DEVICE int): the
// first and the last launch do nothing when it is set; maxbits_dev (nullable, DEVICE 8 bytes): atomic maximum of the bit pattern of |A|^2 after the step.
struct ChirpStepIO {
    void* A;
    void* P;
    const void* chirp;
    int64_t n;
    double gamma, hh;
    const void* h_dev;
    const void* done_dev;
    void* maxbits_dev;
    int c64_line = 0;        // the plan's line holds complex64 values between the passes (plan_line_half_ok; a complex64 caller's run)
    int lean = 0;            // the table holds `n` entries only (nothing is read from `n` up: the padding is set to zero instead) and the rows go out on the plan's lanes
};
SSFM_INTERNAL void* plan_stream(ssfm_plan* plan);            // the plan's stream / field buffer WITHOUT marking the plan as externally ordered (ssfm_stream does)
SSFM_INTERNAL void* plan_field(ssfm_plan* plan);
// one chirp-z step in five launches: x <- ifft(fft(ifft(fft(x) H0) mul) H1) with the step's ends folded in (complex128 plans, plain layout); asynchronous
SSFM_INTERNAL int plan_chirp_step(ssfm_plan* plan, const void* mul_dev, const ChirpStepIO* io);
// a whole fixed-step run on the plan's line in four launches per step: the line holds A c (zero from `keep` up) on entry and on return; slots 0 / 1 hold the
// convolutions' tables; mul[which[s]] = exp(D~ h_s) / keep below `keep`, zero above.  SSFM_ERR_UNSUPPORTED: a plan in the 16-byte-unit layout
SSFM_INTERNAL int plan_chirp_line_run(ssfm_plan* plan, const void* const* mul, const unsigned char* which, const double* hs, int64_t nsteps, double gamma, int64_t keep, int half);
SSFM_INTERNAL int plan_line_half_ok(ssfm_plan* plan);        // 1: the plan has the passes that keep the line in complex64 between them (ssfm_kernels.hpp time_body, H)
// the one-launch engines: a workgroup per row on a line of <= 4096 points (the plan's precision), or the one-XCD engine of a complex64 line of 2^13 ... 2^17
// points; SSFM_ERR_UNSUPPORTED with the field as it came when the plan has no such engine or its workgroups did not meet
SSFM_INTERNAL int plan_chirp_small(ssfm_plan* plan, void* A, const void* chirp, const void* Dt, int64_t n, double gamma, const double* hs, int64_t nsteps);
SSFM_INTERNAL int plan_chirp_small_adapt(ssfm_plan* plan, void* A, const void* chirp, const void* Dt, int64_t n, double gamma, double length, double phi_max, int f32,
                                         int64_t max_steps, double* z_out, int64_t* steps_out);
SSFM_INTERNAL int plan_chirp_medium(ssfm_plan* plan, void* A, const void* chirp, const void* Dt, int64_t n, double gamma, const double* hs, int64_t nsteps);
SSFM_INTERNAL int plan_chirp_medium_adapt(ssfm_plan* plan, void* A, const void* chirp, const void* Dt, int64_t n, double gamma, double length, double phi_max,
                                          int64_t max_steps, double* z_out, int64_t* steps_out);
SSFM_INTERNAL int64_t plan_length(ssfm_plan* plan, int* batch, int* precision);
constexpr int kWorkSlots = 8;
// A device buffer of at least `bytes` bytes owned by the plan (slot 0 ... kWorkSlots - 1; grows on demand, freed with the plan; contents undefined between calls; a growing
// call waits for the plan's stream): scratch for the driver loops of chirpz.hip (the exp(D~ h) tables, the step control block, the z log) without a
// hipMalloc / hipFree pair per call -- hipFree waits for the whole device and stalls the streams of every other plan
SSFM_INTERNAL int plan_workspace(ssfm_plan* plan, int slot, size_t bytes, void** out);

// What the Manakov line (manakov.hip) works on: the field, D~ in the order of the plan's transfer tables (element i of a table is a function of element i of
// it), the two table slots of ssfm_apply_table (made if need be; their tags are cleared: the caller overwrites them).  The run is recorded as the plan's last
// (SSFM_ENGINE_MANAKOV_LINE).  SSFM_ERR_STATE without a linear operator, SSFM_ERR_UNSUPPORTED for split plans.
struct ManakovPlan {
    void* F;
    const void* D;
    void* tab[2];
    void* stream;
    int64_t n;
    int batch, precision;
};
SSFM_INTERNAL int plan_manakov_begin(ssfm_plan* plan, ManakovPlan* out);
// ... for the Manakov-PMD line (SSFM_ENGINE_MANAKOV_PMD_LINE): its tables hold a row per polarisation and live in the plan's workspace, so `tab` comes
// back empty and the slots of ssfm_apply_table stay as they are
SSFM_INTERNAL int plan_manakov_pmd_begin(ssfm_plan* plan, ManakovPlan* out);
// out <- src brought from the natural frequency order into the order of the plan's transfer tables (both DEVICE, plan_length complex values of the plan's
// type), with the kernel that brings D~ there; asynchronous on the plan's stream
SSFM_INTERNAL int plan_to_table_order(ssfm_plan* plan, const void* src, void* out);
// ssfm_apply_table with a table per batch row: x_b <- ifft(fft(x_b) tabs[b]) -- `tabs` (DEVICE) holds batch * plan_length entries in the tables' order
// (the row pass in FM_TABLE_ROWS, ssfm_kernels.hpp); three launches, asynchronous.  SSFM_ERR_UNSUPPORTED for split plans
SSFM_INTERNAL int plan_apply_row_tables(ssfm_plan* plan, const void* tabs);
SSFM_INTERNAL void plan_count_launches(ssfm_plan* plan, int64_t launches);     // (ssfm_last_propagate_ms's count)

// Philox4x32-10 (Salmon et al., SC'11): ten rounds on the counter `c` under the key (k0, k1) -- the documented device generator of
// ssfm_device_randn (device_mem.hip) and of the PPM tie-breaking with rng="device" (ppm.hip).
__device__ __forceinline__ void philox4x32_10(unsigned (&c)[4], unsigned k0, unsigned k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = (unsigned long long)0xD2511F53u * c[0];
        const unsigned long long p1 = (unsigned long long)0xCD9E8D57u * c[2];
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c[1] ^ k0, n1 = (unsigned)p1;
        const unsigned n2 = (unsigned)(p0 >> 32) ^ c[3] ^ k1, n3 = (unsigned)p0;
        c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}

}  // namespace ssfm

#define HIP_TRY(expr)                                                                               \
    do {                                                                                            \
        hipError_t e_ = (expr);                                                                     \
        if (e_ != hipSuccess)                                                                       \
            return ssfm::fail(SSFM_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_),  \
                              __FILE__, __LINE__);                                                  \
    } while (0)

namespace ssfm {

constexpr int kMaxDevices = 64;          // the per-device pools, caches and workspaces hold this many devices

// The device check of every `int device` entry point: the device exists and fits the per-device tables; it is then the calling thread's device.
inline int use_device(int device) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count || device >= kMaxDevices)
        return fail(SSFM_ERR_NO_DEVICE, "device %d not available", device);
    HIP_TRY(hipSetDevice(device));
    return SSFM_OK;
}

// The entry points that take no device number (a signal is computed where it lies): the device is the one that owns the memory at `p`, which becomes
// the calling thread's device; a pointer that is not device memory is refused before anything is launched.  `who` names the caller in the message.
inline int device_of(const void* p, const char* who, int* device) {
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, p) != hipSuccess || attr.type != hipMemoryTypeDevice) {
        (void)hipGetLastError();
        return fail(SSFM_ERR_INVALID, "%s: %p is not device memory", who, p);
    }
    *device = attr.device;
    return use_device(attr.device);
}

// Workgroups of 256 threads for a grid-stride loop over n items: one per 256 items, at least one, at most `cap`.  The cap is the call site's own:
// where per-block partials are folded (eye, FBG, PSD) a different grid changes the order of the sums.
inline unsigned grid_for(long long n, long long cap) {
    const long long b = (n + 255) / 256;
    return (unsigned)(b < cap ? (b > 0 ? b : 1) : cap);
}

// Per-call scratch from the library's pool (ssfm_device_alloc), handed back on every exit.  The device is synchronised first unless the caller has
// marked the scratch `drained` (nothing of the call is in flight any more, e.g. after a blocking copy on the null stream).
struct Scratch {
    static constexpr int kSlots = 6;
    int device;
    void* p[kSlots] = {};
    size_t b[kSlots] = {};
    int k = 0;
    bool drained = false;
    explicit Scratch(int d) : device(d) {}
    Scratch(const Scratch&) = delete;
    Scratch& operator=(const Scratch&) = delete;
    int get(size_t bytes, void** out) {
        if (k == kSlots) return fail(SSFM_ERR_INVALID, "scratch: more than %d buffers", kSlots);
        if (int rc = ssfm_device_alloc(device, bytes, out)) return rc;
        p[k] = *out;
        b[k++] = bytes;
        return SSFM_OK;
    }
    ~Scratch() {
        if (k && !drained) (void)hipDeviceSynchronize();
        for (int i = 0; i < k; ++i) (void)ssfm_device_free(device, p[i], b[i]);
    }
};

}  // namespace ssfm
