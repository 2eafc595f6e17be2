// eye.hip -- the OOK receiver on gfx950: the eye estimator GET_EYE (reference devices.py:1635-1868), the sampler SAMPLER (devices.py:1871-1891)
// and the decision / error count of ook.DSP and BER_analizer (ook.py:63-220).  float64 throughout; no rocPRIM / hipCUB.
//
// What runs here, per GET_EYE call on n samples (n <= 2^21):
//   * ssfm_eye_prepare         real(signal + noise), truncated and rolled (np.roll(x, -sps//2 + 1)) in one pass;
//   * ssfm_eye_resample_stage  the three element-wise steps around the caller's forward / inverse transform that make scipy.signal.resample:
//                              real -> complex, spectrum truncation / zero padding with the Nyquist bin split or folded, real part times m / n;
//   * ssfm_eye_estimate        an LSD radix sort of a copy of the signal (8 passes of 8 bits on the order-preserving bit image), the 1-D
//                              two-means (Lloyd) on the signal, the two shortest 50 % intervals on the sorted copy, the 25-75 % band and the
//                              2-D two-means of its (t, y) points, and the three nearest-value snaps into the pre-resample set of values;
//   * ssfm_eye_levels          the masked moments of the top / bottom clusters in the central 10 % of the eye and the Gaussian KDE of the
//                              central samples on a 500-point grid, with its argmin.
// Every reduction writes one partial per workgroup and a single-workgroup kernel folds the partials in a fixed order: results do not
// depend on scheduling, and two calls on the same input give the same bits.  The Lloyd iterations run in chunks of kLloydChunk launches
// that do nothing once the state block on the device says "converged"; the host looks at that flag once per chunk.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "ssfm_amd.h"
#include "ssfm_common.hpp"

using ssfm::fail;
using ssfm::grid_for;
using ssfm::Scratch;
using ssfm::use_device;

namespace {

#include "eye_levels.inc"                           // kThreads, kRedBlocks, the state block `Slot`, block_sum / fold_partials, the moments and KDE kernels

constexpr int kRadixItems = 8;
constexpr int kTile = kThreads * kRadixItems;      // keys per workgroup and radix pass
constexpr int kLloydChunk = 24;                    // Lloyd steps launched between two looks at the convergence flag
constexpr int kLloydMax = 300;                     // sklearn's max_iter
constexpr int64_t kMaxN = int64_t(1) << 21;

__device__ __forceinline__ unsigned long long order_key(double v) {
    unsigned long long u = (unsigned long long)__double_as_longlong(v);
    if ((u & 0x7fffffffffffffffull) > 0x7ff0000000000000ull) return ~0ull;   // every NaN, of either sign, after +inf (np.sort), in input order
    if (u == 0x8000000000000000ull) u = 0;                         // -0 orders as +0 (NumPy compares them equal): the sort stays stable over both
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

// ------------------------------------------------------------------------------------------------ radix sort
__global__ __launch_bounds__(kThreads) void k_radix_hist(const double* __restrict__ src, long long n, int shift, unsigned* __restrict__ hist, int nblocks) {
    __shared__ unsigned cnt[256];
    cnt[threadIdx.x] = 0;
    __syncthreads();
    const long long base = (long long)blockIdx.x * kTile;
    for (int r = 0; r < kRadixItems; ++r) {
        const long long i = base + r * kThreads + threadIdx.x;
        if (i < n) atomicAdd(&cnt[(order_key(src[i]) >> shift) & 255], 1u);
    }
    __syncthreads();
    hist[(long long)threadIdx.x * nblocks + blockIdx.x] = cnt[threadIdx.x];
}

// exclusive scan in place of every digit's row of `nblocks` counts (hist is digit-major), one workgroup per digit: chunks of 256 x kScanItems
// counts are loaded coalesced into LDS, every thread scans kScanItems consecutive ones, a scan of the 256 thread sums joins them, and the
// chunk's total carries into the next chunk.  totals[d] = the digit's count (the scatter scans the 256 totals itself).
constexpr int kScanItems = 8;
__global__ __launch_bounds__(kThreads) void k_scan_rows(unsigned* __restrict__ hist, int nblocks, unsigned* __restrict__ totals) {
    __shared__ unsigned buf[kThreads * kScanItems];
    __shared__ unsigned part[kThreads];
    __shared__ unsigned carry;
    unsigned* __restrict__ a = hist + (long long)blockIdx.x * nblocks;
    const int tid = threadIdx.x;
    if (tid == 0) carry = 0;
    for (int base = 0; base < nblocks; base += kThreads * kScanItems) {
        for (int q = 0; q < kScanItems; ++q) {
            const int i = base + q * kThreads + tid;
            buf[q * kThreads + tid] = i < nblocks ? a[i] : 0u;
        }
        __syncthreads();
        unsigned s = 0;
        for (int q = 0; q < kScanItems; ++q) s += buf[tid * kScanItems + q];
        part[tid] = s;
        __syncthreads();
        for (int off = 1; off < kThreads; off <<= 1) {
            const unsigned v = tid >= off ? part[tid - off] : 0u;
            __syncthreads();
            part[tid] += v;
            __syncthreads();
        }
        unsigned run = carry + (tid ? part[tid - 1] : 0u);
        for (int q = 0; q < kScanItems; ++q) {
            const unsigned v = buf[tid * kScanItems + q];
            buf[tid * kScanItems + q] = run;
            run += v;
        }
        __syncthreads();                                           // (every thread has read `carry`)
        for (int q = 0; q < kScanItems; ++q) {
            const int i = base + q * kThreads + tid;
            if (i < nblocks) a[i] = buf[q * kThreads + tid];
        }
        if (tid == kThreads - 1) carry += part[kThreads - 1];
        __syncthreads();
    }
    if (tid == 0) totals[blockIdx.x] = carry;
}

// stable scatter: inside a tile the keys keep their order (rounds in order, waves in order, lanes in order)
__global__ __launch_bounds__(kThreads) void k_radix_scatter(const double* __restrict__ src, double* __restrict__ dst, long long n, int shift,
                                                            const unsigned* __restrict__ offs, const unsigned* __restrict__ totals, int nblocks) {
    __shared__ unsigned base[256];
    __shared__ unsigned wc[kWaves][256];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    base[tid] = totals[tid];                                       // exclusive scan of the digits' totals: where each digit starts
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        const unsigned v = tid >= off ? base[tid - off] : 0u;
        __syncthreads();
        base[tid] += v;
        __syncthreads();
    }
    const unsigned start = base[tid] - totals[tid];
    __syncthreads();
    base[tid] = start + offs[(long long)tid * nblocks + blockIdx.x];
    const unsigned long long below = (1ull << lane) - 1ull;
    const long long tb = (long long)blockIdx.x * kTile;
    for (int r = 0; r < kRadixItems; ++r) {
        for (int q = 0; q < kWaves; ++q) wc[q][tid] = 0;
        __syncthreads();
        const long long i = tb + r * kThreads + tid;
        const bool valid = i < n;
        const double v = valid ? src[i] : 0.0;
        const unsigned d = valid ? (unsigned)((order_key(v) >> shift) & 255) : 0u;
        unsigned long long peers = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const unsigned long long m = __ballot((d >> b) & 1u);
            peers &= ((d >> b) & 1u) ? m : ~m;
        }
        const unsigned rank = (unsigned)__popcll(peers & below);
        if (valid && rank == 0) wc[w][d] = (unsigned)__popcll(peers);
        __syncthreads();
        unsigned acc = 0;                                          // thread `tid` owns digit `tid`: exclusive prefix over the waves
        for (int q = 0; q < kWaves; ++q) {
            const unsigned c = wc[q][tid];
            wc[q][tid] = acc;
            acc += c;
        }
        __syncthreads();
        if (valid) dst[base[d] + wc[w][d] + rank] = v;
        __syncthreads();
        base[tid] += acc;
    }
}

int radix_sort(double* keys, double* tmp, unsigned* hist, long long n) {
    const int nblocks = (int)((n + kTile - 1) / kTile);
    double* a = keys;
    double* b = tmp;
    for (int shift = 0; shift < 64; shift += 8) {
        hipLaunchKernelGGL(k_radix_hist, dim3(nblocks), dim3(kThreads), 0, 0, (const double*)a, n, shift, hist, nblocks);
        hipLaunchKernelGGL(k_scan_rows, dim3(256), dim3(kThreads), 0, 0, hist, nblocks, hist + (long long)256 * nblocks);
        hipLaunchKernelGGL(k_radix_scatter, dim3(nblocks), dim3(kThreads), 0, 0, (const double*)a, b, n, shift, (const unsigned*)hist,
                           (const unsigned*)(hist + (long long)256 * nblocks), nblocks);
        double* t = a;
        a = b;
        b = t;
    }
    HIP_TRY(hipGetLastError());                                   // 8 passes: the keys are back in `keys`
    return SSFM_OK;
}

// ------------------------------------------------------------------------------------------------ two-means (Lloyd)
// MODE 0: 1-D Lloyd step on every sample.  MODE 1: count and sum of t over the band v25 < y < v75.  MODE 2: the band split at its mean t
// (the deterministic initialisation).  MODE 3: 2-D Lloyd step on the band.  Distances are formed without fused multiply-adds, as NumPy does.
template <int MODE>
__global__ __launch_bounds__(kThreads) void k_lloyd(const double* __restrict__ y, long long n, const double* __restrict__ tg, int period,
                                                    const double* __restrict__ st, double* __restrict__ part) {
#pragma clang fp contract(off)
    __shared__ double lds[6][kThreads];
    if (MODE == 0 && st[S_DONE1] != 0.0) return;
    if (MODE == 3 && st[S_DONE2] != 0.0) return;
    double v[6] = {0, 0, 0, 0, 0, 0};
    const double c0 = st[S_C0], c1 = st[S_C1];
    const double t0 = st[S_T0], y0 = st[S_Y0], t1 = st[S_T1], y1 = st[S_Y1];
    const double v25 = st[S_V25], v75 = st[S_V75], tm = st[S_TMEAN];
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)kRedBlocks * kThreads) {
        const double x = y[i];
        if (MODE == 0) {
            const bool one = fabs(x - c1) < fabs(x - c0);
            v[one ? 2 : 0] += 1.0;
            v[one ? 3 : 1] += x;
        } else {
            if (!(x > v25 && x < v75)) continue;
            const double t = tg[i % period];
            if (MODE == 1) {
                v[0] += 1.0;
                v[1] += t;
            } else {
                bool one;
                if (MODE == 2) {
                    one = !(t < tm);
                } else {
                    const double a = t - t0, b = x - y0, c = t - t1, d = x - y1;
                    one = c * c + d * d < a * a + b * b;
                }
                v[one ? 3 : 0] += 1.0;
                v[one ? 4 : 1] += t;
                v[one ? 5 : 2] += x;
            }
        }
    }
    block_sum<6>(v, lds);
    if (threadIdx.x < 6) part[blockIdx.x * kPartStride + threadIdx.x] = v[threadIdx.x];
}

template <int MODE>
__global__ __launch_bounds__(kThreads) void k_lloyd_fold(const double* __restrict__ part, double* __restrict__ st) {
    __shared__ double lds[6][kThreads];
    if (MODE == 0 && st[S_DONE1] != 0.0) return;
    if (MODE == 3 && st[S_DONE2] != 0.0) return;
    double v[6];
    fold_partials<6>(part, v, lds);
    if (threadIdx.x) return;
    if (MODE == 0) {
        const double c0 = v[0] > 0 ? v[1] / v[0] : st[S_C0];       // an empty cluster keeps its centre
        const double c1 = v[2] > 0 ? v[3] / v[2] : st[S_C1];
        if (c0 == st[S_C0] && c1 == st[S_C1]) { st[S_DONE1] = 1.0; return; }
        st[S_C0] = c0;
        st[S_C1] = c1;
        st[S_IT1] += 1.0;
        if (st[S_IT1] >= kLloydMax) st[S_DONE1] = 1.0;
    } else if (MODE == 1) {
        st[S_NBAND] = v[0];
        st[S_TMEAN] = v[0] > 0 ? v[1] / v[0] : 0.0;
        st[S_IT2] = 0.0;
        st[S_DONE2] = v[0] < 2 ? 1.0 : 0.0;                       // fewer than 2 points: the reference's `except ValueError` branch
    } else {
        double t0 = v[0] > 0 ? v[1] / v[0] : st[S_T0], y0 = v[0] > 0 ? v[2] / v[0] : st[S_Y0];
        double t1 = v[3] > 0 ? v[4] / v[3] : st[S_T1], y1 = v[3] > 0 ? v[5] / v[3] : st[S_Y1];
        if (MODE == 2) {                                          // an empty half takes the other half's centre
            if (!(v[0] > 0)) { t0 = t1; y0 = y1; }
            if (!(v[3] > 0)) { t1 = t0; y1 = y0; }
        } else if (t0 == st[S_T0] && y0 == st[S_Y0] && t1 == st[S_T1] && y1 == st[S_Y1]) {
            st[S_DONE2] = 1.0;
            return;
        }
        st[S_T0] = t0; st[S_Y0] = y0; st[S_T1] = t1; st[S_Y1] = y1;
        if (MODE == 3) {
            st[S_IT2] += 1.0;
            if (st[S_IT2] >= kLloydMax) st[S_DONE2] = 1.0;
        }
    }
}

// ------------------------------------------------------------------------------------------------ levels from the sorted copy
// a -inf sorts first, a +inf or any NaN last: the two ends of the sorted copy tell whether every sample is finite
__global__ void k_init_1d(const double* __restrict__ sorted, long long n, double* __restrict__ st) {
    for (int k = 0; k < S_COUNT; ++k) st[k] = 0.0;
    const double lo = sorted[0], hi = sorted[n - 1];
    st[S_C0] = lo;                                                 // (min, max): the documented initialisation of the 1-D two-means
    st[S_C1] = hi;
    st[S_NONFINITE] = isfinite(lo) && isfinite(hi) ? 0.0 : 1.0;
}

// vm and the extents of {x < vm} (a prefix of the sorted copy) and {x > vm} (a suffix): two binary searches
__global__ void k_bounds(const double* __restrict__ sorted, long long n, double* __restrict__ st) {
#pragma clang fp contract(off)
    const double vm = (st[S_C0] + st[S_C1]) / 2.0;                 // np.mean of the two centres
    long long lo = 0, hi = n;                                      // first index with x >= vm
    while (lo < hi) { const long long m = (lo + hi) / 2; if (sorted[m] < vm) lo = m + 1; else hi = m; }
    const long long nbot = lo;
    lo = nbot; hi = n;                                             // first index with x > vm
    while (lo < hi) { const long long m = (lo + hi) / 2; if (sorted[m] > vm) hi = m; else lo = m + 1; }
    st[S_VM] = vm;
    st[S_NBOT] = (double)nbot;
    st[S_TOPSTART] = (double)lo;
    st[S_NTOP] = (double)(n - lo);
}

// lag = int(len * percent / 100) of utils.shortest_int (len / 2 at 50 %)
__device__ __forceinline__ long long shortest_lag(long long len, double percent) {
#pragma clang fp contract(off)
    return (long long)((double)len * percent / 100.0);
}

// shortest_int (reference utils.py:1497-1537) on the sorted run [a, a + len): pass 1 the minimum of x[i + lag] - x[i], pass 2 the count and
// the sum of the indices within 1e-10 of it
template <int PASS>
__global__ __launch_bounds__(kThreads) void k_shortest(const double* __restrict__ sorted, const double* __restrict__ st, int top, double percent, double* __restrict__ part) {
    __shared__ double lds[2][kThreads];
    const long long a = top ? (long long)st[S_TOPSTART] : 0, len = (long long)(top ? st[S_NTOP] : st[S_NBOT]);
    const long long lag = shortest_lag(len, percent), m = len - lag;
    const double mind = st[S_MIND];
    double v[2] = {PASS == 1 ? INFINITY : 0.0, 0.0};
    if (len >= 2)
        for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < m; i += (long long)kRedBlocks * kThreads) {
            const double d = sorted[a + i + lag] - sorted[a + i];
            if (PASS == 1) v[0] = d < v[0] ? d : v[0];
            else if (fabs(d - mind) < 1e-10) { v[0] += 1.0; v[1] += (double)i; }
        }
    if (PASS == 1) {
        lds[0][threadIdx.x] = v[0];
        __syncthreads();
        for (int off = kThreads / 2; off > 0; off >>= 1) {
            if (threadIdx.x < off) lds[0][threadIdx.x] = fmin(lds[0][threadIdx.x], lds[0][threadIdx.x + off]);
            __syncthreads();
        }
        if (threadIdx.x == 0) part[blockIdx.x * kPartStride] = lds[0][0];
    } else {
        block_sum<2>(v, lds);
        if (threadIdx.x < 2) part[blockIdx.x * kPartStride + threadIdx.x] = v[threadIdx.x];
    }
}

template <int PASS>
__global__ __launch_bounds__(kThreads) void k_shortest_fold(const double* __restrict__ sorted, const double* __restrict__ part, int top, double percent, double* __restrict__ st) {
    __shared__ double lds[2][kThreads];
    const long long a = top ? (long long)st[S_TOPSTART] : 0, len = (long long)(top ? st[S_NTOP] : st[S_NBOT]);
    if (PASS == 1) {
        double m = INFINITY;
        for (int b = threadIdx.x; b < kRedBlocks; b += kThreads) m = fmin(m, part[b * kPartStride]);
        lds[0][threadIdx.x] = m;
        __syncthreads();
        for (int off = kThreads / 2; off > 0; off >>= 1) {
            if (threadIdx.x < off) lds[0][threadIdx.x] = fmin(lds[0][threadIdx.x], lds[0][threadIdx.x + off]);
            __syncthreads();
        }
        if (threadIdx.x == 0) st[S_MIND] = lds[0][0];
        return;
    }
    double v[2];
    fold_partials<2>(part, v, lds);
    if (threadIdx.x) return;
    double lo = NAN, hi = NAN;
    if (len >= 2 && v[0] >= 1.0) {
        const long long lag = shortest_lag(len, percent);
        const long long idx = v[0] > 1.0 ? (long long)(v[1] / v[0]) : (long long)v[1];     // int(np.mean(i)) on ties
        lo = sorted[a + idx];
        hi = sorted[a + idx + lag];
    }
    st[top ? S_TOP0 : S_BOT0] = lo;
    st[top ? S_TOP1 : S_BOT1] = hi;
}

__global__ void k_levels(double* __restrict__ st) {
#pragma clang fp contract(off)
    const double s1 = (st[S_TOP0] + st[S_TOP1]) / 2.0, s0 = (st[S_BOT0] + st[S_BOT1]) / 2.0;
    const double d01 = s1 - s0;
    st[S_STATE0] = s0;
    st[S_STATE1] = s1;
    st[S_V75] = s1 - 0.25 * d01;
    st[S_V25] = s0 + 0.25 * d01;
    st[S_YCT] = (s0 + s1) / 2.0;
}

// find_nearest(y_set, v): the value of the set closest to v, the lower one on ties -- without building the set
__global__ __launch_bounds__(kThreads) void k_nearest(const double* __restrict__ ys, long long n, const double* __restrict__ st, int target, double* __restrict__ part) {
    __shared__ double ld[kThreads], lv[kThreads];
    const double tv = target == S_YL ? (st[S_T0] <= st[S_T1] ? st[S_Y0] : st[S_Y1])       // argmin / argmax of the centres' t, first on ties
                    : target == S_YR ? (st[S_T1] > st[S_T0] ? st[S_Y1] : st[S_Y0])
                    : st[S_YCT];
    double bd = INFINITY, bv = INFINITY;
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)kRedBlocks * kThreads) {
        const double x = ys[i], d = fabs(x - tv);
        if (d < bd || (d == bd && x < bv)) { bd = d; bv = x; }
    }
    ld[threadIdx.x] = bd;
    lv[threadIdx.x] = bv;
    __syncthreads();
    for (int off = kThreads / 2; off > 0; off >>= 1) {
        if (threadIdx.x < off) {
            const double d = ld[threadIdx.x + off], x = lv[threadIdx.x + off];
            if (d < ld[threadIdx.x] || (d == ld[threadIdx.x] && x < lv[threadIdx.x])) { ld[threadIdx.x] = d; lv[threadIdx.x] = x; }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) { part[blockIdx.x * kPartStride] = ld[0]; part[blockIdx.x * kPartStride + 1] = lv[0]; }
}

__global__ __launch_bounds__(kThreads) void k_nearest_fold(const double* __restrict__ part, int target, double* __restrict__ st) {
    __shared__ double ld[kThreads], lv[kThreads];
    double bd = INFINITY, bv = INFINITY;
    for (int b = threadIdx.x; b < kRedBlocks; b += kThreads) {
        const double d = part[b * kPartStride], x = part[b * kPartStride + 1];
        if (d < bd || (d == bd && x < bv)) { bd = d; bv = x; }
    }
    ld[threadIdx.x] = bd;
    lv[threadIdx.x] = bv;
    __syncthreads();
    for (int off = kThreads / 2; off > 0; off >>= 1) {
        if (threadIdx.x < off) {
            const double d = ld[threadIdx.x + off], x = lv[threadIdx.x + off];
            if (d < ld[threadIdx.x] || (d == ld[threadIdx.x] && x < lv[threadIdx.x])) { ld[threadIdx.x] = d; lv[threadIdx.x] = x; }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) st[target] = lv[0];
}

// ------------------------------------------------------------------------------------------------ element-wise kernels
__global__ __launch_bounds__(kThreads) void k_prepare(const void* __restrict__ sig, const void* __restrict__ noise, int is_complex, long long n, long long shift,
                                                      double* __restrict__ out) {
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads) {
        long long src = (i - shift) % n;                           // np.roll: out[i] = x[(i - shift) mod n]
        if (src < 0) src += n;
        const double a = is_complex ? ((const double2*)sig)[src].x : ((const double*)sig)[src];
        out[i] = noise ? a + (is_complex ? ((const double2*)noise)[src].x : ((const double*)noise)[src]) : a;
    }
}

__global__ __launch_bounds__(kThreads) void k_to_complex(const double* __restrict__ x, long long n, double2* __restrict__ z) {
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads) z[i] = make_double2(x[i], 0.0);
}

// scipy.signal.resample of a real signal, in the full-spectrum form: the bins 0 ... N//2 of X (N = min(n, m)) go to Y at k and (conjugated) at
// m - k; the bin N/2 of an even N is doubled when the signal shrinks and halved when it grows.  Re(ifft(Y)) is then irfft of the half spectrum.
__global__ __launch_bounds__(kThreads) void k_respectrum(const double2* __restrict__ X, long long n, double2* __restrict__ Y, long long m) {
    const long long N = n < m ? n : m, nyq = N / 2 + 1;
    for (long long k = (long long)blockIdx.x * kThreads + threadIdx.x; k < m; k += (long long)gridDim.x * kThreads) {
        const bool neg = k > m / 2;
        const long long j = neg ? m - k : k;
        double2 v = make_double2(0.0, 0.0);
        if (j < nyq) {
            v = X[j];
            if (N % 2 == 0 && j == N / 2) {
                const double f = m < n ? 2.0 : (n < m ? 0.5 : 1.0);
                v.x *= f;
                v.y *= f;
            }
            if (neg) v.y = -v.y;
        }
        Y[k] = v;
    }
}

__global__ __launch_bounds__(kThreads) void k_real_scale(const double2* __restrict__ z, long long m, double scale, double* __restrict__ y) {
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < m; i += (long long)gridDim.x * kThreads) y[i] = z[i].x * scale;
}

__global__ __launch_bounds__(kThreads) void k_sample(const double* __restrict__ x, const double* __restrict__ noise, long long count, long long start,
                                                     long long step, double thr, double* __restrict__ vals, unsigned char* __restrict__ bits) {
    for (long long j = (long long)blockIdx.x * kThreads + threadIdx.x; j < count; j += (long long)gridDim.x * kThreads) {
        const long long i = start + j * step;
        const double v = noise ? x[i] + noise[i] : x[i];
        if (vals) vals[j] = v;
        if (bits) bits[j] = v > thr ? 1 : 0;
    }
}

__global__ __launch_bounds__(kThreads) void k_count_diff(const unsigned char* __restrict__ a, const unsigned char* __restrict__ b, long long n,
                                                         unsigned long long* __restrict__ out) {
    __shared__ double lds[1][kThreads];
    double v[1] = {0.0};
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads) v[0] += a[i] != b[i] ? 1.0 : 0.0;
    block_sum<1>(v, lds);
    if (threadIdx.x == 0) atomicAdd(out, (unsigned long long)v[0]);   // integer atomics: the total does not depend on the order
}



}  // namespace

// ================================================================================================ C ABI
extern "C" int ssfm_device_sort_f64(int device, double* keys, int64_t n) {
    if (!keys || n < 1 || n > kMaxN) return fail(SSFM_ERR_INVALID, "ssfm_device_sort_f64: n=%lld (1 ... 2^21)", (long long)n);
    if (int rc = use_device(device)) return rc;
    Scratch s(device);
    void *tmp, *hist;
    if (int rc = s.get(sizeof(double) * n, &tmp)) return rc;
    if (int rc = s.get(sizeof(unsigned) * 256 * ((n + kTile - 1) / kTile + 1), &hist)) return rc;
    if (int rc = radix_sort(keys, (double*)tmp, (unsigned*)hist, n)) return rc;
    HIP_TRY(hipDeviceSynchronize());
    s.drained = true;
    return SSFM_OK;
}

extern "C" int ssfm_eye_prepare(int device, const void* sig, const void* noise, int is_complex, int64_t n, int64_t shift, double* out) {
    if (!sig || !out || n < 1) return fail(SSFM_ERR_INVALID, "ssfm_eye_prepare: bad argument");
    if (int rc = use_device(device)) return rc;
    hipLaunchKernelGGL(k_prepare, dim3(grid_for(n, 4096)), dim3(kThreads), 0, 0, sig, noise, is_complex, (long long)n, (long long)shift, out);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());                              // the consumers (the plans' transforms, LPF, FIBER) run on other streams
    return SSFM_OK;
}

extern "C" int ssfm_eye_resample_stage(int device, int stage, const void* src, int64_t n, void* dst, int64_t m) {
    if (!src || !dst || n < 1 || m < 1 || stage < 0 || stage > 2) return fail(SSFM_ERR_INVALID, "ssfm_eye_resample_stage: stage=%d n=%lld m=%lld", stage, (long long)n, (long long)m);
    if (int rc = use_device(device)) return rc;
    if (stage == 0)
        hipLaunchKernelGGL(k_to_complex, dim3(grid_for(n, 4096)), dim3(kThreads), 0, 0, (const double*)src, (long long)n, (double2*)dst);
    else if (stage == 1)
        hipLaunchKernelGGL(k_respectrum, dim3(grid_for(m, 4096)), dim3(kThreads), 0, 0, (const double2*)src, (long long)n, (double2*)dst, (long long)m);
    else
        hipLaunchKernelGGL(k_real_scale, dim3(grid_for(m, 4096)), dim3(kThreads), 0, 0, (const double2*)src, (long long)m, (double)m / (double)n, (double*)dst);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());                              // the transforms between the stages run on the plan's (non-blocking) stream
    return SSFM_OK;
}

extern "C" int ssfm_eye_estimate(int device, const double* y, int64_t n, const double* tgrid, int64_t period, const double* yset, int64_t nset, double* out,
                                 int64_t n_out, int64_t* round_trips) {
    if (!y || !tgrid || !yset || !out || n < 2 || n > kMaxN || nset < 1 || period < 2 || period > 4096 || n_out < S_COUNT)
        return fail(SSFM_ERR_INVALID, "ssfm_eye_estimate: n=%lld period=%lld nset=%lld n_out=%lld", (long long)n, (long long)period, (long long)nset, (long long)n_out);
    if (int rc = use_device(device)) return rc;
    Scratch s(device);
    void *sorted, *tmp, *hist, *part, *st, *tg;
    if (int rc = s.get(sizeof(double) * n, &sorted)) return rc;
    if (int rc = s.get(sizeof(double) * n, &tmp)) return rc;
    if (int rc = s.get(sizeof(unsigned) * 256 * ((n + kTile - 1) / kTile + 1), &hist)) return rc;
    if (int rc = s.get(sizeof(double) * kRedBlocks * kPartStride, &part)) return rc;
    if (int rc = s.get(sizeof(double) * 64, &st)) return rc;
    if (int rc = s.get(sizeof(double) * period, &tg)) return rc;
    double* S = (double*)st;
    double* P = (double*)part;
    const double* T = (const double*)tg;
    const long long N = n;
    int64_t trips = 2;                                            // the t-grid upload and the first state read
    HIP_TRY(hipMemcpy(tg, tgrid, sizeof(double) * period, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpyAsync(sorted, y, sizeof(double) * n, hipMemcpyDeviceToDevice, 0));
    if (int rc = radix_sort((double*)sorted, (double*)tmp, (unsigned*)hist, N)) return rc;
    hipLaunchKernelGGL(k_init_1d, dim3(1), dim3(1), 0, 0, (const double*)sorted, N, S);
    const dim3 R(kRedBlocks), B(kThreads);
    auto lloyd1 = [&] {
        for (int k = 0; k < kLloydChunk; ++k) {
            hipLaunchKernelGGL(k_lloyd<0>, R, B, 0, 0, y, N, T, (int)period, (const double*)S, P);
            hipLaunchKernelGGL(k_lloyd_fold<0>, dim3(1), B, 0, 0, (const double*)P, S);
        }
    };
    auto after1 = [&] {                                            // everything from vm to the start of the 2-D two-means
        hipLaunchKernelGGL(k_bounds, dim3(1), dim3(1), 0, 0, (const double*)sorted, N, S);
        for (int top = 0; top < 2; ++top) {
            hipLaunchKernelGGL(k_shortest<1>, R, B, 0, 0, (const double*)sorted, (const double*)S, top, 50.0, P);
            hipLaunchKernelGGL(k_shortest_fold<1>, dim3(1), B, 0, 0, (const double*)sorted, (const double*)P, top, 50.0, S);
            hipLaunchKernelGGL(k_shortest<2>, R, B, 0, 0, (const double*)sorted, (const double*)S, top, 50.0, P);
            hipLaunchKernelGGL(k_shortest_fold<2>, dim3(1), B, 0, 0, (const double*)sorted, (const double*)P, top, 50.0, S);
        }
        hipLaunchKernelGGL(k_levels, dim3(1), dim3(1), 0, 0, S);
        hipLaunchKernelGGL(k_nearest, R, B, 0, 0, yset, (long long)nset, (const double*)S, (int)S_YC, P);
        hipLaunchKernelGGL(k_nearest_fold, dim3(1), B, 0, 0, (const double*)P, (int)S_YC, S);
        hipLaunchKernelGGL(k_lloyd<1>, R, B, 0, 0, y, N, T, (int)period, (const double*)S, P);
        hipLaunchKernelGGL(k_lloyd_fold<1>, dim3(1), B, 0, 0, (const double*)P, S);
        hipLaunchKernelGGL(k_lloyd<2>, R, B, 0, 0, y, N, T, (int)period, (const double*)S, P);
        hipLaunchKernelGGL(k_lloyd_fold<2>, dim3(1), B, 0, 0, (const double*)P, S);
    };
    auto lloyd2 = [&] {
        for (int k = 0; k < kLloydChunk; ++k) {
            hipLaunchKernelGGL(k_lloyd<3>, R, B, 0, 0, y, N, T, (int)period, (const double*)S, P);
            hipLaunchKernelGGL(k_lloyd_fold<3>, dim3(1), B, 0, 0, (const double*)P, S);
        }
        for (int t = S_YL; t <= S_YR; ++t) {
            hipLaunchKernelGGL(k_nearest, R, B, 0, 0, yset, (long long)nset, (const double*)S, t, P);
            hipLaunchKernelGGL(k_nearest_fold, dim3(1), B, 0, 0, (const double*)P, t, S);
        }
    };
    // Speculative order: one chunk of each two-means and everything between them, then one look at the state.  Only a two-means that
    // needs more than kLloydChunk steps costs further looks (and the stages after it are launched again).
    lloyd1();
    after1();
    lloyd2();
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out, S, sizeof(double) * S_COUNT, hipMemcpyDeviceToHost));
    if (out[S_NONFINITE] != 0.0) {                                // no further looks: the caller raises (the state is not an estimate)
        s.drained = true;
        if (round_trips) *round_trips = trips;
        return SSFM_OK;
    }
    while (out[S_DONE1] == 0.0) {
        lloyd1();
        after1();
        lloyd2();
        HIP_TRY(hipMemcpy(out, S, sizeof(double) * S_COUNT, hipMemcpyDeviceToHost));
        ++trips;
    }
    while (out[S_DONE2] == 0.0) {
        lloyd2();
        HIP_TRY(hipMemcpy(out, S, sizeof(double) * S_COUNT, hipMemcpyDeviceToHost));
        ++trips;
    }
    HIP_TRY(hipGetLastError());
    s.drained = true;                                             // (the blocking reads above waited for everything launched here)
    if (round_trips) *round_trips = trips;
    return SSFM_OK;
}

extern "C" int ssfm_eye_levels(int device, const double* y, int64_t n, int64_t period, int64_t k_lo, int64_t k_hi, double y_center, int npts, double* out,
                               int64_t n_out) {
    if (!y || !out || n < 1 || n > kMaxN || period < 1 || n % period != 0 || k_lo < 0 || k_hi < k_lo || k_hi > period || npts < 2 || npts > kKdeThreads ||
        n_out < S_COUNT)
        return fail(SSFM_ERR_INVALID, "ssfm_eye_levels: n=%lld period=%lld k=[%lld, %lld) npts=%d", (long long)n, (long long)period, (long long)k_lo, (long long)k_hi, npts);
    if (int rc = use_device(device)) return rc;
    Centre c;
    c.period = (int)period;
    c.k_lo = (int)k_lo;
    c.w = (int)(k_hi - k_lo);
    c.count = c.w ? (n / period) * c.w : 0;
    const int kblocks = kde_blocks(c);
    Scratch s(device);
    void *part, *st, *kpart;
    if (int rc = s.get(sizeof(double) * kRedBlocks * kPartStride, &part)) return rc;
    if (int rc = s.get(sizeof(double) * 64, &st)) return rc;
    if (int rc = s.get(sizeof(double) * kKdeThreads * (kblocks > 0 ? kblocks : 1), &kpart)) return rc;
    double* S = (double*)st;
    launch_levels(y, c, LevelByValue{}, y_center, npts, S, (double*)part, (double*)kpart);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out, S, sizeof(double) * S_COUNT, hipMemcpyDeviceToHost));
    s.drained = true;
    return SSFM_OK;
}

extern "C" int ssfm_device_sample(int device, const double* x, const double* noise, int64_t start, int64_t step, int64_t count, double thr, double* vals,
                                  unsigned char* bits) {
    if (!x || step < 1 || start < 0 || count < 0 || (!vals && !bits)) return fail(SSFM_ERR_INVALID, "ssfm_device_sample: bad argument");
    if (count == 0) return SSFM_OK;
    if (int rc = use_device(device)) return rc;
    hipLaunchKernelGGL(k_sample, dim3(grid_for(count, 4096)), dim3(kThreads), 0, 0, x, noise, (long long)count, (long long)start, (long long)step, thr, vals, bits);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());                              // the samples / bits go to callers on other streams
    return SSFM_OK;
}

extern "C" int ssfm_device_count_diff(int device, const unsigned char* a, const unsigned char* b, int64_t n, int64_t* out) {
    if (!a || !b || !out || n < 0) return fail(SSFM_ERR_INVALID, "ssfm_device_count_diff: bad argument");
    *out = 0;
    if (n == 0) return SSFM_OK;
    if (int rc = use_device(device)) return rc;
    Scratch s(device);
    void* acc;
    if (int rc = s.get(sizeof(unsigned long long), &acc)) return rc;
    HIP_TRY(hipMemsetAsync(acc, 0, sizeof(unsigned long long), 0));
    hipLaunchKernelGGL(k_count_diff, dim3(grid_for(n, 1024)), dim3(kThreads), 0, 0, a, b, (long long)n, (unsigned long long*)acc);
    HIP_TRY(hipGetLastError());
    unsigned long long h = 0;
    HIP_TRY(hipMemcpy(&h, acc, sizeof(h), hipMemcpyDeviceToHost));
    s.drained = true;
    *out = (int64_t)h;
    return SSFM_OK;
}

// ------------------------------------------------------------------------------------------------ ADC (devices.py:1558-1632)
namespace {

__global__ __launch_bounds__(kThreads) void k_quantize(const double* __restrict__ x, long long n, double vmin, double vmax, long long levels, int as_volts,
                                                       void* __restrict__ out) {
#pragma clang fp contract(off)
    const double span = vmax - vmin, L = (double)levels;
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads) {
        const double q = rint((x[i] - vmin) / span * L);                  // np.round: half to even
        const long long code = (long long)q;                              // .astype(int)
        if (as_volts) ((double*)out)[i] = (double)code / L * span + vmin;
        else ((long long*)out)[i] = code;
    }
}

}  // namespace

extern "C" int ssfm_shortest_int(int device, const double* x, int64_t n, double percent, double* out) {
    const long long lag = (long long)((double)n * percent / 100.0);
    if (!x || !out || n < 2 || n > kMaxN || !(percent > 0 && percent <= 100) || lag < 1 || lag >= n)
        return fail(SSFM_ERR_INVALID, "ssfm_shortest_int: n=%lld percent=%g (lag %lld: 1 ... n - 1; n <= 2^21)", (long long)n, percent, lag);
    if (int rc = use_device(device)) return rc;
    Scratch s(device);
    void *sorted, *tmp, *hist, *part, *st;
    if (int rc = s.get(sizeof(double) * n, &sorted)) return rc;
    if (int rc = s.get(sizeof(double) * n, &tmp)) return rc;
    if (int rc = s.get(sizeof(unsigned) * 256 * ((n + kTile - 1) / kTile + 1), &hist)) return rc;
    if (int rc = s.get(sizeof(double) * kRedBlocks * kPartStride, &part)) return rc;
    if (int rc = s.get(sizeof(double) * 64, &st)) return rc;
    double init[64] = {};
    init[S_NBOT] = (double)n;                                      // the whole sorted copy is the run [0, n)
    HIP_TRY(hipMemcpy(st, init, sizeof(init), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpyAsync(sorted, x, sizeof(double) * n, hipMemcpyDeviceToDevice, 0));
    if (int rc = radix_sort((double*)sorted, (double*)tmp, (unsigned*)hist, n)) return rc;
    double* S = (double*)st;
    double* P = (double*)part;
    const dim3 R(kRedBlocks), B(kThreads);
    hipLaunchKernelGGL(k_shortest<1>, R, B, 0, 0, (const double*)sorted, (const double*)S, 0, percent, P);
    hipLaunchKernelGGL(k_shortest_fold<1>, dim3(1), B, 0, 0, (const double*)sorted, (const double*)P, 0, percent, S);
    hipLaunchKernelGGL(k_shortest<2>, R, B, 0, 0, (const double*)sorted, (const double*)S, 0, percent, P);
    hipLaunchKernelGGL(k_shortest_fold<2>, dim3(1), B, 0, 0, (const double*)sorted, (const double*)P, 0, percent, S);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(init, S, sizeof(init), hipMemcpyDeviceToHost));
    s.drained = true;
    out[0] = init[S_BOT0];
    out[1] = init[S_BOT1];
    return SSFM_OK;
}

extern "C" int ssfm_adc_quantize(int device, const double* x, int64_t n, double vmin, double vmax, int64_t levels, int as_volts, void* out) {
    if (!x || !out || n < 1 || levels < 1) return fail(SSFM_ERR_INVALID, "ssfm_adc_quantize: n=%lld levels=%lld", (long long)n, (long long)levels);
    if (int rc = use_device(device)) return rc;
    hipLaunchKernelGGL(k_quantize, dim3(grid_for(n, 4096)), dim3(kThreads), 0, 0, x, (long long)n, vmin, vmax, (long long)levels, as_volts, out);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    return SSFM_OK;
}
