// ppm.hip -- the M-ary pulse-position modulation receiver on gfx950 (reference opticomlib/ppm.py): the encoder / decoder, the per-symbol slot
// decision of SDD and of DSP's hard decision, and HDD's resolution of the symbols that do not hold exactly one ON slot.  float64 and uint8.
//
//   * ssfm_ppm_encode   one thread per output slot: slot j of symbol s is ON when the k bits of s (MSB first) read j;
//   * ssfm_ppm_decode   every nonzero slot at position p emits the k bits of p mod M, in order -- for any input: a count of the nonzero slots
//                       per tile, an exclusive scan of the tile counts, a scatter that ranks the slots inside its tile.  Called with no output
//                       it returns the number of output bits (its one blocking read);
//   * ssfm_ppm_decide   the slot samples x[start + q step] (+ noise) of each symbol, one wave per 64 / min(M, 64) symbols: lane = slot within a
//                       chunk of min(M, 64) slots.  Hard: __ballot(v > thr), popcount and find-first; a symbol with exactly one ON slot writes
//                       its decoded bits and / or its one-hot slots, every symbol writes its ON count.  Soft: np.argmax per symbol (first index
//                       on ties, NaN is the maximum) as a lane-local fold over the chunks and an xor-shuffle fold inside the symbol's lanes;
//   * ssfm_ppm_faulty   the symbols whose ON count is not 1, compacted in ascending order with their counts (count / scan / scatter);
//   * ssfm_ppm_resolve  one thread per faulty symbol: an empty symbol turns slot r ON, a multi-ON symbol keeps its r-th ON slot; r comes from
//                       the caller's list (the reference's NumPy draws) or from Philox4x32-10 keyed by the seed, counter (symbol, stream).
// The slot read is a strided gather, one 8-byte value per `step` samples: its cost is the number of cache lines it touches, not bytes.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "ssfm_amd.h"
#include "ssfm_common.hpp"

using ssfm::fail;
using ssfm::grid_for;
using ssfm::Scratch;
using ssfm::use_device;
using ssfm::philox4x32_10;

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kPerThread = 16;                     // items per thread of a count / scatter tile
constexpr int kTile = kThreads * kPerThread;       // items per tile
constexpr int kMaxM = 1 << 16;



int log2_of(int M) {
    int k = 0;
    while ((1 << (k + 1)) <= M) ++k;
    return k;
}

// ------------------------------------------------------------------------------------------------ encoder
__global__ __launch_bounds__(kThreads) void k_encode(const unsigned char* __restrict__ bits, long long nsym, int M, int k, unsigned char* __restrict__ slots) {
    const long long n = nsym * M;
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads) {
        const long long s = i / M;
        const int j = (int)(i - s * M);
        int v = 0;
        for (int b = 0; b < k; ++b) v = (v << 1) | (bits[s * k + b] != 0);
        slots[i] = v == j;
    }
}

// ------------------------------------------------------------------------------------------------ count / scan / scatter
// Exclusive prefix sum of one int per thread over the workgroup; *total gets the sum.
__device__ int block_exclusive_scan(int v, int* lds, int* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_up(incl, off);
        if (lane >= off) incl += o;
    }
    if (lane == 63) lds[wave] = incl;
    __syncthreads();
    int before = 0, sum = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
        before += w < wave ? lds[w] : 0;
        sum += lds[w];
    }
    __syncthreads();
    *total = sum;
    return before + incl - v;
}

// Whether item i counts: a nonzero slot (decode) or a symbol whose ON count is not 1 (faulty).
struct NonZero {
    const unsigned char* a;
    __device__ bool operator()(long long i) const { return a[i] != 0; }
};
struct Faulty {
    const int* c;
    __device__ bool operator()(long long i) const { return c[i] != 1; }
};

template <class P>
__global__ __launch_bounds__(kThreads) void k_tile_count(P pred, long long n, long long ntiles, long long* __restrict__ counts) {
    __shared__ int lds[kWaves];
    for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const long long i0 = t * kTile + (long long)threadIdx.x * kPerThread;
        int c = 0;
        for (int u = 0; u < kPerThread; ++u) c += (i0 + u < n && pred(i0 + u)) ? 1 : 0;
        int total;
        block_exclusive_scan(c, lds, &total);
        if (threadIdx.x == 0) counts[t] = total;
    }
}

// One workgroup: offs[t] = sum of counts[0 .. t), offs[ntiles] = the total.
__global__ __launch_bounds__(kThreads) void k_scan_tiles(const long long* __restrict__ counts, long long ntiles, long long* __restrict__ offs) {
    __shared__ long long lds[kThreads];
    long long carry = 0;
    for (long long base = 0; base < ntiles; base += kThreads) {
        const long long t = base + threadIdx.x;
        const long long v = t < ntiles ? counts[t] : 0;
        lds[threadIdx.x] = v;
        __syncthreads();
        for (int off = 1; off < kThreads; off <<= 1) {             // Hillis-Steele, inclusive
            const long long o = threadIdx.x >= off ? lds[threadIdx.x - off] : 0;
            __syncthreads();
            lds[threadIdx.x] += o;
            __syncthreads();
        }
        if (t < ntiles) offs[t] = carry + lds[threadIdx.x] - v;
        carry += lds[kThreads - 1];
        __syncthreads();
    }
    if (threadIdx.x == 0) offs[ntiles] = carry;
}

// Decoder scatter: the r-th nonzero slot of the input (position p) writes the k bits of p mod M at out[r k ...], below `cap` bits.
__global__ __launch_bounds__(kThreads) void k_decode_scatter(const unsigned char* __restrict__ slots, long long n, long long ntiles, const long long* __restrict__ offs,
                                                             int M, int k, unsigned char* __restrict__ out, long long cap) {
    __shared__ int lds[kWaves];
    for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const long long i0 = t * kTile + (long long)threadIdx.x * kPerThread;
        int c = 0;
        for (int u = 0; u < kPerThread; ++u) c += (i0 + u < n && slots[i0 + u] != 0) ? 1 : 0;
        int total;
        long long r = offs[t] + block_exclusive_scan(c, lds, &total);
        for (int u = 0; u < kPerThread && c; ++u) {
            const long long p = i0 + u;
            if (p >= n || slots[p] == 0) continue;
            const int v = (int)(p & (M - 1));
            for (int b = 0; b < k; ++b)
                if ((r + 1) * k <= cap) out[r * k + b] = (v >> (k - 1 - b)) & 1;
            ++r;
            --c;
        }
    }
}

// Faulty scatter: the r-th symbol whose count is not 1 goes to idx[r] / cnt[r].
__global__ __launch_bounds__(kThreads) void k_faulty_scatter(const int* __restrict__ counts, long long n, long long ntiles, const long long* __restrict__ offs,
                                                             int* __restrict__ idx, int* __restrict__ cnt) {
    __shared__ int lds[kWaves];
    for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const long long i0 = t * kTile + (long long)threadIdx.x * kPerThread;
        int c = 0;
        for (int u = 0; u < kPerThread; ++u) c += (i0 + u < n && counts[i0 + u] != 1) ? 1 : 0;
        int total;
        long long r = offs[t] + block_exclusive_scan(c, lds, &total);
        for (int u = 0; u < kPerThread && c; ++u) {
            const long long s = i0 + u;
            if (s >= n || counts[s] == 1) continue;
            idx[r] = (int)s;
            cnt[r] = counts[s];
            ++r;
            --c;
        }
    }
}

// ------------------------------------------------------------------------------------------------ slot decision
template <bool U8>
__device__ __forceinline__ double slot_value(const void* x, const double* noise, long long e) {
    if (U8) return ((const unsigned char*)x)[e] != 0 ? 1.0 : 0.0;
    const double v = ((const double*)x)[e];
    return noise ? v + noise[e] : v;
}

// np.argmax order: a NaN beats any number, the lower index wins a tie (between NaNs too)
__device__ __forceinline__ bool better(double av, int aj, double bv, int bj) {
    const bool an = av != av, bn = bv != bv;
    if (an || bn) return an && (!bn || aj < bj);
    return av > bv || (av == bv && aj < bj);
}

// The k bits of `v` (MSB first) from lanes j0 < k and / or the one-hot slots of symbol s from all W lanes of the symbol.
__device__ __forceinline__ void write_symbol(long long s, int v, int j0, int W, int M, int k, unsigned char* bits, unsigned char* slots) {
    if (bits && j0 < k) bits[s * k + j0] = (v >> (k - 1 - j0)) & 1;
    if (slots)
        for (int c = 0; c < M; c += W) slots[s * M + c + j0] = (c + j0) == v;
}

template <bool U8, bool HARD>
__global__ __launch_bounds__(kThreads) void k_decide(const void* __restrict__ x, const double* __restrict__ noise, long long start, long long step, long long nsym,
                                                     int M, int k, double thr, unsigned char* __restrict__ bits, unsigned char* __restrict__ slots,
                                                     int* __restrict__ counts) {
    const int lane = threadIdx.x & 63;
    const int W = M < 64 ? M : 64;                       // lanes per symbol
    const int G = 64 / W;                                // symbols per wave and step
    const int g = lane / W, j0 = lane - g * W;
    const unsigned long long seg = W == 64 ? ~0ull : ((1ull << W) - 1);
    const long long nwaves = (long long)gridDim.x * kWaves;
    for (long long base = ((long long)blockIdx.x * kWaves + (threadIdx.x >> 6)) * G; base < nsym; base += nwaves * G) {   // wave-uniform
        const long long s = base + g;
        const bool valid = s < nsym;
        const long long q0 = s * M;
        if (HARD) {
            int cnt = 0, first = -1;
            for (int c = 0; c < M; c += W) {
                const bool on = valid && slot_value<U8>(x, noise, start + (q0 + c + j0) * step) > thr;
                const unsigned long long m = (__ballot(on) >> (g * W)) & seg;
                if (m && first < 0) first = c + __ffsll((long long)m) - 1;
                cnt += __popcll(m);
            }
            if (!valid) continue;
            if (counts && j0 == 0) counts[s] = cnt;
            if (cnt == 1) write_symbol(s, first, j0, W, M, k, bits, slots);
        } else {
            double bv = 0.0;
            int bj = -1;
            for (int c = 0; c < M; c += W) {
                const double v = valid ? slot_value<U8>(x, noise, start + (q0 + c + j0) * step) : 0.0;
                if (bj < 0 || better(v, c + j0, bv, bj)) { bv = v; bj = c + j0; }
            }
            for (int off = W >> 1; off > 0; off >>= 1) {       // stays inside the symbol's W aligned lanes
                const double ov = __shfl_xor(bv, off);
                const int oj = __shfl_xor(bj, off);
                if (better(ov, oj, bv, bj)) { bv = ov; bj = oj; }
            }
            if (!valid) continue;
            write_symbol(s, bj, j0, W, M, k, bits, slots);
        }
    }
}

// ------------------------------------------------------------------------------------------------ HDD resolution
// Thread per entry: list mode (idx != NULL) takes symbol idx[f] and the draw draws[f]; device mode walks every symbol whose count is not 1 and
// draws r = floor(u32 * bound / 2^32) from Philox4x32-10 (key = seed, counter = (symbol, stream)), bound = M for an empty symbol, else its count.
template <bool U8>
__global__ __launch_bounds__(kThreads) void k_resolve(const void* __restrict__ x, const double* __restrict__ noise, long long start, long long step, long long nsym,
                                                      int M, int k, double thr, const int* __restrict__ counts, const int* __restrict__ idx,
                                                      const int* __restrict__ draws, long long n_list, unsigned long long seed, unsigned long long stream,
                                                      unsigned char* __restrict__ bits, unsigned char* __restrict__ slots) {
    const long long n = idx ? n_list : nsym;
    for (long long f = (long long)blockIdx.x * kThreads + threadIdx.x; f < n; f += (long long)gridDim.x * kThreads) {
        const long long s = idx ? idx[f] : f;
        if (s < 0 || s >= nsym) continue;
        const int cnt = counts[s];
        if (cnt == 1) continue;
        const int bound = cnt == 0 ? M : cnt;
        long long r;
        if (idx) {
            r = draws[f];
        } else {
            unsigned c[4] = {(unsigned)s, (unsigned)((unsigned long long)s >> 32), (unsigned)stream, (unsigned)(stream >> 32)};
            philox4x32_10(c, (unsigned)seed, (unsigned)(seed >> 32));
            r = (long long)(((unsigned long long)c[0] * (unsigned)bound) >> 32);
        }
        r = r < 0 ? 0 : (r >= bound ? bound - 1 : r);
        int v = (int)r;
        if (cnt > 0) {                                     // the r-th ON slot
            v = M - 1;
            for (int j = 0, seen = 0; j < M; ++j)
                if (slot_value<U8>(x, noise, start + (s * M + j) * step) > thr && seen++ == r) { v = j; break; }
        }
        if (bits)
            for (int b = 0; b < k; ++b) bits[s * k + b] = (v >> (k - 1 - b)) & 1;
        if (slots)
            for (int j = 0; j < M; ++j) slots[s * M + j] = j == v;
    }
}

bool pow2_ok(int M) { return M >= 2 && M <= kMaxM && (M & (M - 1)) == 0; }

// count + scan of a predicate over n items: offs (ntiles + 1 entries) in scratch
template <class P>
int count_scan(Scratch& s, P pred, long long n, long long* ntiles_out, long long** offs_out) {
    const long long ntiles = (n + kTile - 1) / kTile;
    void *cnt, *offs;
    if (int rc = s.get(sizeof(long long) * ntiles, &cnt)) return rc;
    if (int rc = s.get(sizeof(long long) * (ntiles + 1), &offs)) return rc;
    const unsigned blocks = (unsigned)(ntiles < 4096 ? ntiles : 4096);
    hipLaunchKernelGGL(k_tile_count<P>, dim3(blocks), dim3(kThreads), 0, 0, pred, n, ntiles, (long long*)cnt);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_scan_tiles, dim3(1), dim3(kThreads), 0, 0, (const long long*)cnt, ntiles, (long long*)offs);
    HIP_TRY(hipGetLastError());
    *ntiles_out = ntiles;
    *offs_out = (long long*)offs;
    return SSFM_OK;
}

unsigned decide_grid(long long nsym, int M) {
    const long long per_wg = (long long)kWaves * (64 / (M < 64 ? M : 64));   // symbols per workgroup and step
    const long long b = (nsym + per_wg - 1) / per_wg;
    return (unsigned)(b < 8192 ? (b > 0 ? b : 1) : 8192);
}

}  // namespace

// ================================================================================================ C ABI
extern "C" int ssfm_ppm_encode(int device, const unsigned char* bits, int64_t nsym, int M, unsigned char* slots) {
    if (!bits || !slots || nsym < 0 || M < 2 || M > kMaxM) return fail(SSFM_ERR_INVALID, "ssfm_ppm_encode: nsym=%lld M=%d", (long long)nsym, M);
    if (nsym == 0) return SSFM_OK;
    if (int rc = use_device(device)) return rc;
    hipLaunchKernelGGL(k_encode, dim3(grid_for(nsym * M, 4096)), dim3(kThreads), 0, 0, bits, (long long)nsym, M, log2_of(M), slots);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());                              // the slots go to callers on other streams (DAC)
    return SSFM_OK;
}

extern "C" int ssfm_ppm_decode(int device, const unsigned char* slots, int64_t n, int M, unsigned char* bits, int64_t cap, int64_t* n_bits) {
    if (!slots || n < 0 || !pow2_ok(M) || (!bits && !n_bits) || cap < 0) return fail(SSFM_ERR_INVALID, "ssfm_ppm_decode: n=%lld M=%d", (long long)n, M);
    if (n_bits && !bits) *n_bits = 0;
    if (n == 0) return SSFM_OK;
    if (int rc = use_device(device)) return rc;
    Scratch s(device);
    long long ntiles, *offs;
    if (int rc = count_scan(s, NonZero{slots}, n, &ntiles, &offs)) return rc;
    const int k = log2_of(M);
    if (bits) {
        const unsigned blocks = (unsigned)(ntiles < 4096 ? ntiles : 4096);
        hipLaunchKernelGGL(k_decode_scatter, dim3(blocks), dim3(kThreads), 0, 0, slots, (long long)n, ntiles, (const long long*)offs, M, k, bits, (long long)cap);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipDeviceSynchronize());
    } else {
        long long total = 0;
        HIP_TRY(hipMemcpy(&total, offs + ntiles, sizeof(total), hipMemcpyDeviceToHost));    // the one blocking read
        *n_bits = total * k;
    }
    s.drained = true;
    return SSFM_OK;
}

extern "C" int ssfm_ppm_decide(int device, const void* x, const double* noise, int is_u8, int64_t start, int64_t step, int64_t nsym, int M, int hard,
                               double thr, unsigned char* bits, unsigned char* slots, int* counts) {
    if (!x || start < 0 || step < 1 || nsym < 0 || nsym > INT32_MAX || !pow2_ok(M) || (!bits && !slots) || (hard && !counts) || (is_u8 && noise))
        return fail(SSFM_ERR_INVALID, "ssfm_ppm_decide: nsym=%lld M=%d hard=%d", (long long)nsym, M, hard);
    if (nsym == 0) return SSFM_OK;
    if (int rc = use_device(device)) return rc;
    const unsigned blocks = decide_grid(nsym, M);
    const int k = log2_of(M);
    const long long a = start, b = step, c = nsym;
#define SSFM_DECIDE(U, H) hipLaunchKernelGGL((k_decide<U, H>), dim3(blocks), dim3(kThreads), 0, 0, x, noise, a, b, c, M, k, thr, bits, slots, counts)
    if (is_u8) {
        if (hard) SSFM_DECIDE(true, true); else SSFM_DECIDE(true, false);
    } else {
        if (hard) SSFM_DECIDE(false, true); else SSFM_DECIDE(false, false);
    }
#undef SSFM_DECIDE
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    return SSFM_OK;
}

extern "C" int ssfm_ppm_faulty(int device, const int* counts, int64_t nsym, int* idx, int* cnt, int64_t* n_faulty) {
    if (!counts || !idx || !cnt || !n_faulty || nsym < 0 || nsym > INT32_MAX) return fail(SSFM_ERR_INVALID, "ssfm_ppm_faulty: nsym=%lld", (long long)nsym);
    *n_faulty = 0;
    if (nsym == 0) return SSFM_OK;
    if (int rc = use_device(device)) return rc;
    Scratch s(device);
    long long ntiles, *offs;
    if (int rc = count_scan(s, Faulty{counts}, nsym, &ntiles, &offs)) return rc;
    const unsigned blocks = (unsigned)(ntiles < 4096 ? ntiles : 4096);
    hipLaunchKernelGGL(k_faulty_scatter, dim3(blocks), dim3(kThreads), 0, 0, counts, (long long)nsym, ntiles, (const long long*)offs, idx, cnt);
    HIP_TRY(hipGetLastError());
    long long total = 0;
    HIP_TRY(hipMemcpy(&total, offs + ntiles, sizeof(total), hipMemcpyDeviceToHost));        // blocking: the scatter has finished too
    s.drained = true;
    *n_faulty = total;
    return SSFM_OK;
}

extern "C" int ssfm_ppm_resolve(int device, const void* x, const double* noise, int is_u8, int64_t start, int64_t step, int64_t nsym, int M, double thr,
                                const int* counts, const int* idx, const int* draws, int64_t n_list, uint64_t seed, uint64_t stream, unsigned char* bits,
                                unsigned char* slots) {
    if (!x || !counts || start < 0 || step < 1 || nsym < 0 || nsym > INT32_MAX || !pow2_ok(M) || (!bits && !slots) || (idx && !draws) || n_list < 0 ||
        (is_u8 && noise))
        return fail(SSFM_ERR_INVALID, "ssfm_ppm_resolve: nsym=%lld M=%d n_list=%lld", (long long)nsym, M, (long long)n_list);
    const long long n = idx ? n_list : nsym;
    if (n == 0) return SSFM_OK;
    if (int rc = use_device(device)) return rc;
    const int k = log2_of(M);
    if (is_u8)
        hipLaunchKernelGGL(k_resolve<true>, dim3(grid_for(n, 4096)), dim3(kThreads), 0, 0, x, noise, (long long)start, (long long)step, (long long)nsym, M, k, thr, counts, idx,
                           draws, (long long)n_list, (unsigned long long)seed, (unsigned long long)stream, bits, slots);
    else
        hipLaunchKernelGGL(k_resolve<false>, dim3(grid_for(n, 4096)), dim3(kThreads), 0, 0, x, noise, (long long)start, (long long)step, (long long)nsym, M, k, thr, counts, idx,
                           draws, (long long)n_list, (unsigned long long)seed, (unsigned long long)stream, bits, slots);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    return SSFM_OK;
}
