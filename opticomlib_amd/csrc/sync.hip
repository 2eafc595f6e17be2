// sync.hip -- the data-aided receiver on gfx950: lab.SYNC (reference lab.py:92-155) and lab.GET_EYE_v2 (lab.py:158-273).  float64 throughout.
//
// SYNC correlates the first W = min(len(rx), 2 l) samples of the record with the transmitted slots held `sps` samples each (l samples) and cuts the
// record at the largest of the nc = W - l + 1 lags.  The correlation itself is one circular convolution on a power-of-two complex128 plan of
// M >= W points (ssfm_table_from_field, ssfm_load_padded, ssfm_apply_table); what runs here is
//   * ssfm_load_template      the template written into the plan's field TIME-REVERSED modulo M from the uint8 slots, field[(M - m) mod M] = tx[m]: its
//                             transform is conj(fft(tx)), so the convolution leaves corr[k] = sum_m rx[k + m] tx[m] at field index k, and the lags
//                             k < nc never reach the wrap;
//   * ssfm_sync_peak          {max, first argmax, mean, population std} of the nc lags in two passes: the mean first (with the extrema), then the squared
//                             deviations about it -- corr rides on a mean far above its spread, where E[x^2] - E[x]^2 loses every digit.
// GET_EYE_v2 takes a sample's level from the slot that was sent:
//   * ssfm_eye_levels_known   the moments and the KDE argmin of eye_levels.inc with the level read from bits[slot];
//   * ssfm_eye_split_known    x compacted into `ones` and `zeros`, whole slots in order: a scan over the bits ranks every slot among its level.
// Every reduction adds inside a wavefront with cross-lane shuffles, then across the workgroup's four wavefronts through LDS, writes one partial per
// workgroup, and a single workgroup folds the partials in a fixed order: no float atomics, and two calls on the same input give the same bits.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "ssfm_amd.h"
#include "ssfm_common.hpp"

using ssfm::fail;
using ssfm::grid_for;
using ssfm::Scratch;
using ssfm::device_of;

namespace {

#include "eye_levels.inc"

constexpr int64_t kMaxN = int64_t(1) << 21;        // samples of an eye (as eye.hip)
constexpr int64_t kMaxLags = int64_t(1) << 22;     // lags of a correlation: the longest line of a plan
constexpr int kPeakOut = 4;                        // doubles ssfm_sync_peak returns
enum PeakSlot { P_MAX, P_ARG, P_MEAN, P_STD, P_MIN, P_SUM, P_COUNT };

// ------------------------------------------------------------------------------------------------ the template
__global__ __launch_bounds__(kThreads) void k_load_template(const unsigned char* __restrict__ bits, long long l, int sps, double2* __restrict__ F, long long M) {
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < M; i += (long long)gridDim.x * kThreads) {
        const long long m = i ? M - i : 0;                        // field index i holds tx[(M - i) mod M]
        F[i] = make_double2(m < l && bits[m / sps] ? 1.0 : 0.0, 0.0);
    }
}

// ------------------------------------------------------------------------------------------------ the peak
// NumPy's order of np.max / np.argmax: a NaN is the maximum, the first of equals wins.
__device__ __forceinline__ bool peak_before(double av, long long ai, double bv, long long bi) {
    const bool an = av != av, bn = bv != bv;
    if (an || bn) return an && (!bn || ai < bi);
    return av > bv || (av == bv && ai < bi);
}

struct Peak {
    double mx, mn, sum;
    long long arg;
};

__device__ __forceinline__ void peak_join(Peak& a, double mx, long long arg, double mn, double sum) {
    if (peak_before(mx, arg, a.mx, a.arg)) { a.mx = mx; a.arg = arg; }
    if (mn < a.mn) a.mn = mn;
    a.sum += sum;
}

// a wavefront's 64 values by shuffles (lane 0 holds the result), the four wavefronts through LDS in their order (thread 0 holds the result)
__device__ void peak_block(Peak& p) {
    __shared__ double s_mx[kWaves], s_mn[kWaves], s_sum[kWaves];
    __shared__ long long s_arg[kWaves];
    for (int off = 32; off > 0; off >>= 1)
        peak_join(p, __shfl_down(p.mx, off, 64), __shfl_down(p.arg, off, 64), __shfl_down(p.mn, off, 64), __shfl_down(p.sum, off, 64));
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) { s_mx[w] = p.mx; s_arg[w] = p.arg; s_mn[w] = p.mn; s_sum[w] = p.sum; }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int q = 1; q < kWaves; ++q) peak_join(p, s_mx[q], s_arg[q], s_mn[q], s_sum[q]);
    __syncthreads();
}

__device__ double sum_block(double v) {
    __shared__ double s_v[kWaves];
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if ((threadIdx.x & 63) == 0) s_v[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int q = 1; q < kWaves; ++q) v += s_v[q];
    __syncthreads();
    return v;
}

constexpr long long kNoIndex = 0x7fffffffffffffffll;

// pass 1: the maximum with its first index, the minimum and the sum of x[i stride], i < n
__global__ __launch_bounds__(kThreads) void k_peak(const double* __restrict__ x, long long stride, long long n, double* __restrict__ part) {
    Peak p{-INFINITY, INFINITY, 0.0, kNoIndex};
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads) {
        const double v = x[i * stride];
        peak_join(p, v, i, v, v);
    }
    peak_block(p);
    if (threadIdx.x == 0) {
        double* o = part + (long long)blockIdx.x * kPartStride;
        o[0] = p.mx; o[1] = (double)p.arg; o[2] = p.mn; o[3] = p.sum;      // (an index below 2^53 is exact)
    }
}

// The mean of values that are all equal must be that value, whatever their sum rounds to: it is held inside [min, max], where the true mean lies.
__global__ __launch_bounds__(kThreads) void k_peak_fold(const double* __restrict__ part, int nblocks, long long n, double* __restrict__ st) {
    Peak p{-INFINITY, INFINITY, 0.0, kNoIndex};
    for (int b = threadIdx.x; b < nblocks; b += kThreads) {
        const double* o = part + (long long)b * kPartStride;
        peak_join(p, o[0], o[1] < 9.0e18 ? (long long)o[1] : kNoIndex, o[2], o[3]);
    }
    peak_block(p);
    if (threadIdx.x) return;
    double mean = p.sum / (double)n;
    if (mean < p.mn) mean = p.mn;                                  // (false for a NaN mean: it stays)
    if (mean > p.mx) mean = p.mx;
    st[P_MAX] = p.mx; st[P_ARG] = (double)p.arg; st[P_MEAN] = mean; st[P_MIN] = p.mn; st[P_SUM] = p.sum;
}

// pass 2: the sum of (x - mean)^2
__global__ __launch_bounds__(kThreads) void k_deviation(const double* __restrict__ x, long long stride, long long n, const double* __restrict__ st, double* __restrict__ part) {
#pragma clang fp contract(off)
    const double mean = st[P_MEAN];
    double v = 0.0;
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads) {
        const double d = x[i * stride] - mean;
        v += d * d;
    }
    v = sum_block(v);
    if (threadIdx.x == 0) part[(long long)blockIdx.x * kPartStride] = v;
}

__global__ __launch_bounds__(kThreads) void k_deviation_fold(const double* __restrict__ part, int nblocks, long long n, double* __restrict__ st) {
    double v = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += kThreads) v += part[(long long)b * kPartStride];
    v = sum_block(v);
    if (threadIdx.x == 0) st[P_STD] = sqrt(v / (double)n);        // np.std: ddof 0
}

// ------------------------------------------------------------------------------------------------ the split by known slot
constexpr int kSplitTile = kThreads;               // slots per workgroup: one per thread

// ones among the tile's slots
__global__ __launch_bounds__(kThreads) void k_split_count(const unsigned char* __restrict__ bits, long long nslots, unsigned* __restrict__ counts) {
    __shared__ unsigned wc[kWaves];
    const long long s = (long long)blockIdx.x * kSplitTile + threadIdx.x;
    const unsigned long long m = __ballot(s < nslots && bits[s] != 0);
    if ((threadIdx.x & 63) == 0) wc[threadIdx.x >> 6] = (unsigned)__popcll(m);
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned c = 0;
        for (int q = 0; q < kWaves; ++q) c += wc[q];
        counts[blockIdx.x] = c;
    }
}

// exclusive scan of the tiles' counts in place (one workgroup, chunks of kThreads with a carry); st[S_N1] / st[S_N0] = the slots of either level
__global__ __launch_bounds__(kThreads) void k_split_scan(unsigned* __restrict__ counts, int nblocks, long long nslots, double* __restrict__ st) {
    __shared__ unsigned buf[kThreads];
    __shared__ unsigned carry;
    const int tid = threadIdx.x;
    if (tid == 0) carry = 0;
    __syncthreads();
    for (int base = 0; base < nblocks; base += kThreads) {
        const int i = base + tid;
        const unsigned own = i < nblocks ? counts[i] : 0u;
        buf[tid] = own;
        __syncthreads();
        for (int off = 1; off < kThreads; off <<= 1) {
            const unsigned v = tid >= off ? buf[tid - off] : 0u;
            __syncthreads();
            buf[tid] += v;
            __syncthreads();
        }
        if (i < nblocks) counts[i] = carry + buf[tid] - own;
        __syncthreads();                                           // (every thread has read `carry`)
        if (tid == kThreads - 1) carry += buf[tid];
        __syncthreads();
    }
    if (tid == 0) {
        for (int k = 0; k < S_COUNT; ++k) st[k] = 0.0;
        st[S_N1] = (double)carry;
        st[S_N0] = (double)(nslots - (long long)carry);
    }
}

// Slot s is the r-th of its level, r = the ones before it (or s minus them): its sps samples go to ones[r sps ...] or zeros[r sps ...].  The tile's
// samples are read in order by the whole workgroup, so the loads are contiguous and the stores are contiguous runs of sps samples.
__global__ __launch_bounds__(kThreads) void k_split_copy(const double* __restrict__ x, const unsigned char* __restrict__ bits, long long nslots, int sps,
                                                         const unsigned* __restrict__ before, double* __restrict__ ones, double* __restrict__ zeros) {
    __shared__ unsigned wc[kWaves];
    __shared__ long long dst[kSplitTile];                          // r for a one, -1 - r for a zero
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const long long s0 = (long long)blockIdx.x * kSplitTile, s = s0 + tid;
    const bool one = s < nslots && bits[s] != 0;
    const unsigned long long m = __ballot(one);
    if (lane == 0) wc[w] = (unsigned)__popcll(m);
    __syncthreads();
    long long r1 = before[blockIdx.x] + __popcll(m & ((1ull << lane) - 1ull));
    for (int q = 0; q < w; ++q) r1 += wc[q];
    dst[tid] = one ? r1 : -1 - (s - r1);
    __syncthreads();
    const long long left = nslots - s0;
    const long long total = (left < kSplitTile ? left : kSplitTile) * sps;
    for (long long i = tid; i < total; i += kThreads) {
        const long long q = i / sps, k = i - q * sps, d = dst[q];
        const double v = x[s0 * sps + i];
        if (d >= 0) ones[d * sps + k] = v;
        else zeros[(-1 - d) * sps + k] = v;
    }
}

}  // namespace

// ================================================================================================ C ABI
extern "C" int ssfm_load_template(ssfm_plan* plan, int64_t plan_n, const unsigned char* bits, int64_t nbits, int sps) {
    int prec = 0, rows = 0;
    if (!plan || ssfm::plan_length(plan, &rows, &prec) != plan_n || prec != SSFM_C128 || rows < 1)
        return fail(SSFM_ERR_INVALID, "ssfm_load_template: a complex128 plan of %lld points is needed", (long long)plan_n);
    double2* F = static_cast<double2*>(ssfm::plan_field(plan));
    if (!F || !bits || nbits < 1 || sps < 1 || nbits > plan_n / sps)
        return fail(SSFM_ERR_INVALID, "ssfm_load_template: %lld slots x %d samples for a plan of %lld", (long long)nbits, sps, (long long)plan_n);
    hipLaunchKernelGGL(k_load_template, dim3(grid_for(plan_n, 4096)), dim3(kThreads), 0, static_cast<hipStream_t>(ssfm::plan_stream(plan)), bits,
                       (long long)(nbits * sps), sps, F, (long long)plan_n);
    HIP_TRY(hipGetLastError());
    return SSFM_OK;
}

extern "C" int ssfm_sync_peak(const double* x, int64_t stride, int64_t n, double* out, int64_t n_out) {
    if (!x || !out || n < 1 || n > kMaxLags || stride < 1 || stride > 2 || n_out < kPeakOut)
        return fail(SSFM_ERR_INVALID, "ssfm_sync_peak: n=%lld (1 ... 2^22) stride=%lld (1 or 2) n_out=%lld", (long long)n, (long long)stride, (long long)n_out);
    int device = 0;
    if (int rc = device_of(x, "ssfm_sync_peak", &device)) return rc;
    const unsigned nblocks = grid_for(n, kRedBlocks);
    Scratch s(device);
    void *part, *st;
    if (int rc = s.get(sizeof(double) * nblocks * kPartStride, &part)) return rc;
    if (int rc = s.get(sizeof(double) * 8, &st)) return rc;
    static_assert(P_COUNT <= 8, "peak state");
    double* S = (double*)st;
    double* P = (double*)part;
    hipLaunchKernelGGL(k_peak, dim3(nblocks), dim3(kThreads), 0, 0, x, (long long)stride, (long long)n, P);
    hipLaunchKernelGGL(k_peak_fold, dim3(1), dim3(kThreads), 0, 0, (const double*)P, (int)nblocks, (long long)n, S);
    hipLaunchKernelGGL(k_deviation, dim3(nblocks), dim3(kThreads), 0, 0, x, (long long)stride, (long long)n, (const double*)S, P);
    hipLaunchKernelGGL(k_deviation_fold, dim3(1), dim3(kThreads), 0, 0, (const double*)P, (int)nblocks, (long long)n, S);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out, S, sizeof(double) * kPeakOut, hipMemcpyDeviceToHost));
    s.drained = true;
    return SSFM_OK;
}

extern "C" int ssfm_eye_levels_known(const double* x, int64_t n, int64_t sps, int64_t k_lo, int64_t k_hi, const unsigned char* bits, int npts,
                                     double* out, int64_t n_out) {
    if (!x || !bits || !out || n < 1 || n > kMaxN || sps < 1 || n % sps != 0 || k_lo < 0 || k_hi < k_lo || k_hi > sps || npts < 2 || npts > kKdeThreads ||
        n_out < S_COUNT)
        return fail(SSFM_ERR_INVALID, "ssfm_eye_levels_known: n=%lld sps=%lld k=[%lld, %lld) npts=%d", (long long)n, (long long)sps, (long long)k_lo, (long long)k_hi, npts);
    int device = 0;
    if (int rc = device_of(x, "ssfm_eye_levels_known", &device)) return rc;
    Centre c;
    c.period = (int)sps;
    c.k_lo = (int)k_lo;
    c.w = (int)(k_hi - k_lo);
    c.count = c.w ? (n / sps) * c.w : 0;
    const int kblocks = kde_blocks(c);
    Scratch s(device);
    void *part, *st, *kpart;
    if (int rc = s.get(sizeof(double) * kRedBlocks * kPartStride, &part)) return rc;
    if (int rc = s.get(sizeof(double) * 64, &st)) return rc;
    if (int rc = s.get(sizeof(double) * kKdeThreads * (kblocks > 0 ? kblocks : 1), &kpart)) return rc;
    double* S = (double*)st;
    launch_levels(x, c, LevelBySlot{bits}, 0.0, npts, S, (double*)part, (double*)kpart);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out, S, sizeof(double) * S_COUNT, hipMemcpyDeviceToHost));
    s.drained = true;
    return SSFM_OK;
}

extern "C" int ssfm_eye_split_known(const double* x, int64_t nslots, int64_t sps, const unsigned char* bits, double* ones, double* zeros,
                                    double* out, int64_t n_out) {
    if (!bits || !out || nslots < 1 || sps < 1 || nslots > kMaxN / sps || n_out < S_COUNT || (ones == nullptr) != (zeros == nullptr) || (ones && !x))
        return fail(SSFM_ERR_INVALID, "ssfm_eye_split_known: nslots=%lld sps=%lld n_out=%lld", (long long)nslots, (long long)sps, (long long)n_out);
    int device = 0;
    if (int rc = device_of(bits, "ssfm_eye_split_known", &device)) return rc;
    const int nblocks = (int)((nslots + kSplitTile - 1) / kSplitTile);
    Scratch s(device);
    void *counts, *st;
    if (int rc = s.get(sizeof(unsigned) * nblocks, &counts)) return rc;
    if (int rc = s.get(sizeof(double) * 64, &st)) return rc;
    hipLaunchKernelGGL(k_split_count, dim3(nblocks), dim3(kThreads), 0, 0, bits, (long long)nslots, (unsigned*)counts);
    hipLaunchKernelGGL(k_split_scan, dim3(1), dim3(kThreads), 0, 0, (unsigned*)counts, nblocks, (long long)nslots, (double*)st);
    if (ones)
        hipLaunchKernelGGL(k_split_copy, dim3(nblocks), dim3(kThreads), 0, 0, x, bits, (long long)nslots, (int)sps, (const unsigned*)counts, ones, zeros);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out, st, sizeof(double) * S_COUNT, hipMemcpyDeviceToHost));
    s.drained = true;
    return SSFM_OK;
}
