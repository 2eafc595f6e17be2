// psd.hip -- Welch's power spectral density on gfx950: the device side of opticomlib_amd.get_psd (reference utils.py:2048-2079, which calls
// scipy.signal.welch with a periodic Hann window, noverlap = nperseg // 2, nfft = nperseg, no detrend, scaling = 'spectrum', two-sided, mean
// over the segments).  float64 arithmetic whatever the input type (float64, complex64 or complex128 rows, read in place with a row stride).
//
// Three routes, chosen by the caller (opticomlib_amd/utils.py):
//   1. nperseg = 2^m, 16 <= nperseg <= 8192 (ssfm_welch):   k_welch_pow2 -- a grid of rows x G workgroups, each owning a contiguous range of
//      segments of one row: load in wgfft's pattern P times the window, one fft_line in double, |X_k|^2 accumulated in registers; the
//      workgroup writes its L partial sums -- then k_welch_fold.
//   2. nperseg < 16 (ssfm_welch):                            k_welch_direct -- a direct DFT per (row, segment), one thread per segment at a
//      time, a fixed-order workgroup reduction, one partial per workgroup -- then k_welch_fold.
//   3. everything else (the caller sequences it around the chirp-z transform, devices._ChirpZ):  ssfm_welch_frames writes windowed segments
//      as complex128 rows into a chunk buffer, the plan transforms them, ssfm_welch_accumulate adds |X|^2 of the chunk into one float64
//      accumulator per (row, bin); ssfm_welch_finish applies the scale and the fftshift.
// No float atomics anywhere: every sum runs in a fixed order, so two calls on the same input give the same bits.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <mutex>

#include "ssfm_amd.h"
#include "ssfm_common.hpp"
#include "wgfft.hpp"

using ssfm::fail;
using ssfm::grid_for;
using ssfm::Scratch;
using ssfm::use_device;
using ssfm::cf32;
using ssfm::cf64;

namespace {

constexpr int kThreads = 256;
constexpr int kDirectMax = 15;                     // route 2: nperseg < 16
constexpr int64_t kTargetGroups = 1024;            // route 1 / 2: about four workgroups per CU of the 256-CU part
constexpr int kMinLog2 = 4, kMaxLog2 = 13;         // route 1: 16 ... 8192

// input element -> complex double (a real input has a zero imaginary part)
__device__ __forceinline__ cf64 widen(double v) { cf64 r; r.x = v; r.y = 0.0; return r; }
__device__ __forceinline__ cf64 widen(cf32 v) { cf64 r; r.x = (double)v.x; r.y = (double)v.y; return r; }
__device__ __forceinline__ cf64 widen(cf64 v) { return v; }

// periodic Hann window of length n (scipy.signal.get_window('hann', n)): 0.5 - 0.5 cos(2 pi m / n); [1.0] for n = 1
__device__ __forceinline__ double hann(int64_t m, int64_t n) { return n == 1 ? 1.0 : 0.5 - 0.5 * cospi(2.0 * (double)m / (double)n); }

// ------------------------------------------------------------------------------------------------ route 1
// E = 8 points per thread up to 4096 (radix-8 stages, twiddles in registers); 16 for 8192 (16 * 16 * 16 * 2: at most four stages).  Lines of
// fewer than 256 threads share a workgroup: LINES lines side by side, each with its own LDS row, all on segments of the same row.
__host__ __device__ constexpr int welch_points(int L) { return L == 8192 ? 16 : 8; }
__host__ __device__ constexpr int welch_lines(int L) { return L / welch_points(L) >= kThreads ? 1 : kThreads / (L / welch_points(L)); }
__host__ __device__ constexpr int welch_threads(int L) { return welch_lines(L) * (L / welch_points(L)); }
__host__ __device__ constexpr int pad_shift(int E) { return E == 16 ? 4 : 3; }
__host__ __device__ constexpr int line_elems(int L, int E) { return L + (L >> pad_shift(E)); }      // one pad element per 2^SH (as RowIdx of ssfm_kernels.hpp)
template <int L> constexpr size_t welch_lds() {
    constexpr int E = welch_points(L);
    return (size_t)welch_lines(L) * line_elems(L, E) * sizeof(cf64) + (size_t)ssfm::fft_tw_lds_entries(L, E) * sizeof(cf64);
}
// L = 8192: the line in double is 8192 x 16 B = 128 KiB plus 8 KiB of padding: it fits the 160 KiB only with the single-buffer exchange (BUF = 0)
static_assert(welch_lds<8192>() <= 160 * 1024, "k_welch_pow2<8192>: the line and its LDS twiddles must fit the LDS");

template <int SH> struct PadIdx {
    int off;
    __device__ __forceinline__ int operator()(int e) const { return off + e + (e >> SH); }
};

struct Pow2Args {
    const void* x;           // rows of n input elements, `ld` elements apart
    const cf64* tw;          // stage twiddles of the L-point line (wgfft.hpp "Table layout"), double
    const double* win;       // the window, L entries
    double* part;            // [rows][G][L] partial sums of |X_k|^2, natural bin order
    long long ld;
    long long step;          // nperseg - noverlap
    long long nseg;          // segments per row
    long long spw;           // segments per workgroup
};

template <typename Tin, int L>
__global__ __launch_bounds__(welch_threads(L)) void k_welch_pow2(const Pow2Args a) {
    constexpr int E = welch_points(L);
    constexpr int Q = L / E;
    constexpr int LINES = welch_lines(L);
    constexpr int NT = welch_threads(L);
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    cf64* lds = reinterpret_cast<cf64*>(smem_raw);
    cf64* ldsT = lds + LINES * line_elems(L, E);
    const int tid = threadIdx.x, rr = tid / Q, j = tid - rr * Q;
    const long long row = blockIdx.y, g = blockIdx.x, G = gridDim.x;
    const long long s0 = g * a.spw;
    const long long s1 = s0 + a.spw < a.nseg ? s0 + a.spw : a.nseg;
    const PadIdx<pad_shift(E)> idx{rr * line_elems(L, E)};

    ssfm::LineTw<double, L, E> tw;
    ssfm::line_twiddles_issue<double, L, E>(tw, j, a.tw, ldsT, tid, NT);
    if (ssfm::fft_tw_lds_entries(L, E) > 0) __syncthreads();
    ssfm::line_twiddles_fetch<double, L, E>(tw, j, ldsT);
    // the window stays in registers up to 4096 points; at 8192 (16 points per thread, 256 registers already) it is read with every segment, from L2
    constexpr bool WREG = E == 8;
    double w[WREG ? E : 1], acc[E];
#pragma unroll
    for (int t = 0; t < E; ++t) {
        if constexpr (WREG) w[t] = a.win[j + t * Q];
        acc[t] = 0.0;
    }

    const Tin* __restrict__ xr = reinterpret_cast<const Tin*>(a.x) + row * a.ld;
    // every line of the workgroup runs the same number of transforms (the exchanges hold barriers); a line past the range transforms zeros
    const long long iters = (s1 - s0 + LINES - 1) / LINES;
    for (long long it = 0; it < iters; ++it) {
        const long long s = s0 + it * LINES + rr;
        const bool live = s < s1;
        cf64 v[E];
#pragma unroll
        for (int t = 0; t < E; ++t) {
            v[t] = widen(0.0);
            if (live) {
                const cf64 u = widen(xr[s * a.step + j + t * Q]);
                const double wt = WREG ? w[WREG ? t : 0] : a.win[j + t * Q];
                v[t].x = u.x * wt;
                v[t].y = u.y * wt;
            }
        }
        // XP = 1: with the single buffer, a barrier before the first exchange's writes keeps them behind the last reads of the previous line
        ssfm::fft_line<double, L, E, -1, 1>(v, lds, 0, j, idx, tw);
        if (live) {
#pragma unroll
            for (int t = 0; t < E; ++t) acc[t] += v[t].x * v[t].x + v[t].y * v[t].y;
        }
    }

    double* __restrict__ out = a.part + (row * G + g) * L;
    if constexpr (LINES == 1) {
#pragma unroll
        for (int t = 0; t < E; ++t) out[j + t * Q] = acc[t];
    } else {
        // the lines' sums, added in line order through LDS (the line buffers are free once every thread is past its last transform)
        double* red = reinterpret_cast<double*>(smem_raw);
        __syncthreads();
#pragma unroll
        for (int t = 0; t < E; ++t) red[rr * L + j + t * Q] = acc[t];
        __syncthreads();
        for (int k = tid; k < L; k += NT) {
            double s = 0.0;
            for (int r = 0; r < LINES; ++r) s += red[r * L + k];
            out[k] = s;
        }
    }
}

// The stage twiddles of an L-point double line in thread-load order (what ssfm_host.hip make_line_table computes on the host) and the window.
template <int L>
__global__ __launch_bounds__(kThreads) void k_welch_tables(cf64* __restrict__ tab, double* __restrict__ win) {
    constexpr int E = welch_points(L);
    constexpr int M = ssfm::fft_nstages(L, E);
    const int i0 = blockIdx.x * kThreads + threadIdx.x, stride = gridDim.x * kThreads;
    for (int m = i0; m < L; m += stride) win[m] = hann(m, L);
    for (int S = 1; S < M; ++S) {
        const int R = ssfm::fft_radix(L, S, E), NB = E / R, KU = ssfm::fft_tw_ku(L, S, E), off = ssfm::fft_tw_offset(L, S, E, 8);
        const int count = NB * (R - 1) * KU;
        for (int e = i0; e < count; e += stride) {
            const int ku = e % KU, slot = e / KU, i = slot / (R - 1), u = slot % (R - 1) + 1;
            const int q = ssfm::fft_tw_exponent(L, E, S, i, u, ku) % L;
            double sn, cs;
            sincospi(-2.0 * (double)q / (double)L, &sn, &cs);
            cf64 w; w.x = cs; w.y = sn;
            tab[off + ssfm::fft_tw_index(L, S, E, 8, slot, ku)] = w;
        }
    }
}

// ------------------------------------------------------------------------------------------------ route 2
struct DirectArgs {
    const void* x;
    double* part;            // [rows][G][P]
    long long ld, step, nseg, spw;
    int P;
};
template <typename Tin>
__global__ __launch_bounds__(kThreads) void k_welch_direct(const DirectArgs a) {
    __shared__ double red[kDirectMax][kThreads];
    __shared__ cf64 wt[kDirectMax];                // exp(-2 pi i q / P)
    __shared__ double win[kDirectMax];
    const int tid = threadIdx.x, P = a.P;
    const long long row = blockIdx.y, g = blockIdx.x, G = gridDim.x;
    if (tid < P) {
        double sn, cs;
        sincospi(-2.0 * (double)tid / (double)P, &sn, &cs);
        cf64 w; w.x = cs; w.y = sn;
        wt[tid] = w;
        win[tid] = hann(tid, P);
    }
    __syncthreads();
    const long long s0 = g * a.spw;
    const long long s1 = s0 + a.spw < a.nseg ? s0 + a.spw : a.nseg;
    const Tin* __restrict__ xr = reinterpret_cast<const Tin*>(a.x) + row * a.ld;
    double acc[kDirectMax];
#pragma unroll
    for (int k = 0; k < kDirectMax; ++k) acc[k] = 0.0;
    for (long long s = s0 + tid; s < s1; s += kThreads) {
        cf64 v[kDirectMax];
#pragma unroll
        for (int m = 0; m < kDirectMax; ++m) {
            v[m] = widen(0.0);
            if (m < P) {
                const cf64 u = widen(xr[s * a.step + m]);
                v[m].x = u.x * win[m];
                v[m].y = u.y * win[m];
            }
        }
#pragma unroll
        for (int k = 0; k < kDirectMax; ++k) {
            if (k < P) {
                double re = 0.0, im = 0.0;
                int q = 0;                                   // k m mod P
#pragma unroll
                for (int m = 0; m < kDirectMax; ++m) {
                    if (m < P) {
                        const cf64 w = wt[q];
                        re += v[m].x * w.x - v[m].y * w.y;
                        im += v[m].x * w.y + v[m].y * w.x;
                        q += k;
                        if (q >= P) q -= P;
                    }
                }
                acc[k] += re * re + im * im;
            }
        }
    }
    // fixed-order tree over the workgroup's threads
#pragma unroll
    for (int k = 0; k < kDirectMax; ++k)
        if (k < P) red[k][tid] = acc[k];
    __syncthreads();
    for (int h = kThreads / 2; h > 0; h >>= 1) {
        if (tid < h)
            for (int k = 0; k < P; ++k) red[k][tid] += red[k][tid + h];
        __syncthreads();
    }
    if (tid < P) a.part[(row * G + g) * P + tid] = red[tid][0];
}

// ------------------------------------------------------------------------------------------------ the fold (routes 1 and 2, and route 3's finish)
// A workgroup per (row, tile of kBins output bins): kSlices threads per bin sum every kSlices-th term in ascending order, then the slice sums
// are added in slice order -- a fixed order, and kSlices times the parallelism of one thread per bin.
constexpr int kBins = 16, kSlices = kThreads / kBins;
// out[row][o] = factor * sum_g part[row][g][(o + L - L / 2) % L] (the fftshift of numpy / scipy.fft: out[(k + L // 2) % L] = in[k])
template <typename To>
__global__ __launch_bounds__(kThreads) void k_welch_fold(const double* __restrict__ part, long long G, long long L, double factor, To* __restrict__ out) {
    __shared__ double red[kSlices][kBins];
    const int b = threadIdx.x % kBins, q = threadIdx.x / kBins;
    const long long row = blockIdx.y, o = (long long)blockIdx.x * kBins + b;
    double s = 0.0;
    if (o < L) {
        long long k = o + (L - L / 2);
        if (k >= L) k -= L;
        const double* p = part + row * G * L + k;
        for (long long g = q; g < G; g += kSlices) s += p[g * L];
    }
    red[q][b] = s;
    __syncthreads();
    if (q == 0 && o < L) {
        double t = 0.0;
        for (int i = 0; i < kSlices; ++i) t += red[i][b];
        out[row * L + o] = (To)(t * factor);
    }
}

// ------------------------------------------------------------------------------------------------ route 3
// frames[c][m] = window[m] x[row(first + c)][seg(first + c) * step + m] as complex128, zero for c >= count (the chunk's unused rows)
template <typename Tin>
__global__ __launch_bounds__(kThreads) void k_welch_frames(const Tin* __restrict__ x, long long ld, long long P, long long step, long long nseg,
                                                           long long first, long long count, long long chunk, cf64* __restrict__ frames) {
    const long long total = chunk * P;
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < total; i += (long long)gridDim.x * kThreads) {
        const long long c = i / P, m = i - c * P;
        cf64 v = widen(0.0);
        if (c < count) {
            const long long gs = first + c, row = gs / nseg, s = gs - row * nseg;
            const cf64 u = widen(x[row * ld + s * step + m]);
            const double w = hann(m, P);
            v.x = u.x * w;
            v.y = u.y * w;
        }
        frames[i] = v;
    }
}
// acc[row][k] += sum over the chunk's segments of that row of |frames[c][k]|^2, in the fold's order (kSlices ascending partial sums, added in order)
__global__ __launch_bounds__(kThreads) void k_welch_accumulate(const cf64* __restrict__ frames, long long P, long long nseg, long long first,
                                                               long long count, long long row0, double* __restrict__ acc) {
    __shared__ double red[kSlices][kBins];
    const int b = threadIdx.x % kBins, q = threadIdx.x / kBins;
    const long long row = row0 + blockIdx.y, k = (long long)blockIdx.x * kBins + b;
    const long long a0 = row * nseg > first ? row * nseg : first;
    const long long a1 = (row + 1) * nseg < first + count ? (row + 1) * nseg : first + count;
    double s = 0.0;
    if (k < P)
        for (long long gs = a0 + q; gs < a1; gs += kSlices) {
            const cf64 v = frames[(gs - first) * P + k];
            s += v.x * v.x + v.y * v.y;
        }
    red[q][b] = s;
    __syncthreads();
    if (q == 0 && k < P) {
        double t = acc[row * P + k];
        for (int i = 0; i < kSlices; ++i) t += red[i][b];
        acc[row * P + k] = t;
    }
}



// route 1's tables, per device and line length: generated on the device once, kept for the life of the process (at most 10 x 200 KiB per device)
struct Tables { cf64* tw = nullptr; double* win = nullptr; };
std::mutex g_tab_mu;
Tables g_tab[ssfm::kMaxDevices][kMaxLog2 + 1];

template <int L> int make_tables(Tables& t) {
    constexpr int E = welch_points(L);
    const int entries = ssfm::fft_tw_entries(L, E, 8);
    HIP_TRY(hipMalloc(&t.tw, sizeof(cf64) * (entries > 0 ? entries : 1)));
    HIP_TRY(hipMalloc(&t.win, sizeof(double) * L));
    hipLaunchKernelGGL(k_welch_tables<L>, dim3((L + kThreads - 1) / kThreads), dim3(kThreads), 0, 0, t.tw, t.win);
    HIP_TRY(hipGetLastError());
    return SSFM_OK;
}
int tables(int device, int log2L, Tables* out) {
    std::lock_guard<std::mutex> lock(g_tab_mu);
    Tables& t = g_tab[device][log2L];
    if (!t.tw) {
        int rc = SSFM_ERR_INVALID;
        switch (log2L) {
            case 4: rc = make_tables<16>(t); break;
            case 5: rc = make_tables<32>(t); break;
            case 6: rc = make_tables<64>(t); break;
            case 7: rc = make_tables<128>(t); break;
            case 8: rc = make_tables<256>(t); break;
            case 9: rc = make_tables<512>(t); break;
            case 10: rc = make_tables<1024>(t); break;
            case 11: rc = make_tables<2048>(t); break;
            case 12: rc = make_tables<4096>(t); break;
            case 13: rc = make_tables<8192>(t); break;
        }
        if (rc) {
            (void)hipFree(t.tw);
            (void)hipFree(t.win);
            t = Tables{};
            return rc;
        }
    }
    *out = t;
    return SSFM_OK;
}

template <typename Tin, int L> int launch_pow2(dim3 grid, const Pow2Args& a) {
    constexpr size_t lds = welch_lds<L>();
    if (lds > 48 * 1024) {
        static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(k_welch_pow2<Tin, L>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        HIP_TRY(attr);
    }
    hipLaunchKernelGGL((k_welch_pow2<Tin, L>), grid, dim3(welch_threads(L)), lds, 0, a);
    HIP_TRY(hipGetLastError());
    return SSFM_OK;
}
template <typename Tin> int launch_pow2_any(int log2L, dim3 grid, const Pow2Args& a) {
    switch (log2L) {
        case 4: return launch_pow2<Tin, 16>(grid, a);
        case 5: return launch_pow2<Tin, 32>(grid, a);
        case 6: return launch_pow2<Tin, 64>(grid, a);
        case 7: return launch_pow2<Tin, 128>(grid, a);
        case 8: return launch_pow2<Tin, 256>(grid, a);
        case 9: return launch_pow2<Tin, 512>(grid, a);
        case 10: return launch_pow2<Tin, 1024>(grid, a);
        case 11: return launch_pow2<Tin, 2048>(grid, a);
        case 12: return launch_pow2<Tin, 4096>(grid, a);
        case 13: return launch_pow2<Tin, 8192>(grid, a);
    }
    return fail(SSFM_ERR_INVALID, "welch: no line kernel for 2^%d points", log2L);
}

// segments per workgroup: about kTargetGroups workgroups over all rows, at least `least` segments each (a whole round of a workgroup's lines)
long long per_group(long long rows, long long nseg, long long least) {
    long long spw = (rows * nseg + kTargetGroups - 1) / kTargetGroups;
    if (spw < least) spw = least;
    if (spw > nseg) spw = nseg;
    const long long G = (nseg + spw - 1) / spw;
    return (nseg + G - 1) / G;                     // the same G with the segments spread evenly
}

bool valid_dtype(int dtype) { return dtype == SSFM_C64 || dtype == SSFM_C128 || dtype == SSFM_F64_REAL; }

int fold_out(const double* part, long long rows, long long G, long long L, double factor, int out_f32, void* out_host, void* out_dev) {
    const dim3 grid((unsigned)((L + kBins - 1) / kBins), (unsigned)rows);
    if (out_f32) hipLaunchKernelGGL(k_welch_fold<float>, grid, dim3(kThreads), 0, 0, part, G, L, factor, (float*)out_dev);
    else hipLaunchKernelGGL(k_welch_fold<double>, grid, dim3(kThreads), 0, 0, part, G, L, factor, (double*)out_dev);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out_host, out_dev, (size_t)(rows * L) * (out_f32 ? 4 : 8), hipMemcpyDeviceToHost));      // the one host wait
    return SSFM_OK;
}

}  // namespace

// ================================================================================================ C ABI
extern "C" int ssfm_welch(int device, const void* x, int dtype, int64_t rows, int64_t n, int64_t ld, int64_t nperseg, double factor, int out_f32,
                          void* out) {
    if (!x || !out || !valid_dtype(dtype) || rows < 1 || rows > 65535 || nperseg < 1 || n < nperseg || ld < n)
        return fail(SSFM_ERR_INVALID, "ssfm_welch: dtype=%d rows=%lld n=%lld ld=%lld nperseg=%lld", dtype, (long long)rows, (long long)n, (long long)ld,
                    (long long)nperseg);
    const bool pow2 = (nperseg & (nperseg - 1)) == 0;
    int log2L = 0;
    while ((int64_t(1) << log2L) < nperseg) ++log2L;
    if (!(nperseg <= kDirectMax || (pow2 && log2L >= kMinLog2 && log2L <= kMaxLog2)))
        return fail(SSFM_ERR_INVALID, "ssfm_welch: nperseg=%lld takes the chirp-z route (ssfm_welch_frames)", (long long)nperseg);
    if (int rc = use_device(device)) return rc;
    const long long P = nperseg, noverlap = P / 2, step = P - noverlap, nseg = (n - noverlap) / step;
    const long long spw = per_group(rows, nseg, nperseg <= kDirectMax ? kThreads : 2 * welch_lines((int)nperseg));
    const long long G = (nseg + spw - 1) / spw;
    Scratch s(device);
    void* buf;
    const size_t part_bytes = sizeof(double) * (size_t)(rows * G * P), out_bytes = (size_t)(rows * P) * (out_f32 ? 4 : 8);
    if (int rc = s.get(part_bytes + ((out_bytes + 255) & ~size_t(255)), &buf)) return rc;
    double* part = (double*)((char*)buf + ((out_bytes + 255) & ~size_t(255)));
    const dim3 grid((unsigned)G, (unsigned)rows);
    if (nperseg <= kDirectMax) {
        const DirectArgs a{x, part, (long long)ld, step, nseg, spw, (int)P};
        if (dtype == SSFM_C64) hipLaunchKernelGGL(k_welch_direct<cf32>, grid, dim3(kThreads), 0, 0, a);
        else if (dtype == SSFM_C128) hipLaunchKernelGGL(k_welch_direct<cf64>, grid, dim3(kThreads), 0, 0, a);
        else hipLaunchKernelGGL(k_welch_direct<double>, grid, dim3(kThreads), 0, 0, a);
        HIP_TRY(hipGetLastError());
    } else {
        Tables t;
        if (int rc = tables(device, log2L, &t)) return rc;
        const Pow2Args a{x, t.tw, t.win, part, (long long)ld, step, nseg, spw};
        int rc = dtype == SSFM_C64 ? launch_pow2_any<cf32>(log2L, grid, a) : dtype == SSFM_C128 ? launch_pow2_any<cf64>(log2L, grid, a) : launch_pow2_any<double>(log2L, grid, a);
        if (rc) return rc;
    }
    if (int rc = fold_out(part, rows, G, P, factor / (double)nseg, out_f32, out, buf)) return rc;
    s.drained = true;
    return SSFM_OK;
}

extern "C" int ssfm_welch_frames(int device, const void* x, int dtype, int64_t rows, int64_t n, int64_t ld, int64_t nperseg, int64_t first, int64_t count,
                                 int64_t chunk, void* frames) {
    const long long P = nperseg, noverlap = P / 2, step = P - noverlap, nseg = P >= 1 && n >= P ? (n - noverlap) / step : 0;
    if (!x || !frames || !valid_dtype(dtype) || rows < 1 || nperseg < 1 || n < nperseg || ld < n || first < 0 || count < 0 || count > chunk ||
        first + count > rows * nseg)
        return fail(SSFM_ERR_INVALID, "ssfm_welch_frames: rows=%lld n=%lld nperseg=%lld first=%lld count=%lld chunk=%lld", (long long)rows, (long long)n,
                    (long long)nperseg, (long long)first, (long long)count, (long long)chunk);
    if (int rc = use_device(device)) return rc;
    const dim3 grid(grid_for(chunk * P, 2048));
    if (dtype == SSFM_C64) hipLaunchKernelGGL(k_welch_frames<cf32>, grid, dim3(kThreads), 0, 0, (const cf32*)x, (long long)ld, P, step, nseg, (long long)first, (long long)count, (long long)chunk, (cf64*)frames);
    else if (dtype == SSFM_C128) hipLaunchKernelGGL(k_welch_frames<cf64>, grid, dim3(kThreads), 0, 0, (const cf64*)x, (long long)ld, P, step, nseg, (long long)first, (long long)count, (long long)chunk, (cf64*)frames);
    else hipLaunchKernelGGL(k_welch_frames<double>, grid, dim3(kThreads), 0, 0, (const double*)x, (long long)ld, P, step, nseg, (long long)first, (long long)count, (long long)chunk, (cf64*)frames);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());           // the transform that follows runs on the plan's (non-blocking) stream
    return SSFM_OK;
}

extern "C" int ssfm_welch_accumulate(int device, const void* frames, int64_t nperseg, int64_t rows, int64_t nseg, int64_t first, int64_t count, void* acc) {
    if (!frames || !acc || nperseg < 1 || rows < 1 || nseg < 1 || first < 0 || count < 1 || first + count > rows * nseg)
        return fail(SSFM_ERR_INVALID, "ssfm_welch_accumulate: nperseg=%lld rows=%lld nseg=%lld first=%lld count=%lld", (long long)nperseg, (long long)rows,
                    (long long)nseg, (long long)first, (long long)count);
    if (int rc = use_device(device)) return rc;
    const long long row0 = first / nseg, row1 = (first + count - 1) / nseg;
    hipLaunchKernelGGL(k_welch_accumulate, dim3((unsigned)((nperseg + kBins - 1) / kBins), (unsigned)(row1 - row0 + 1)), dim3(kThreads), 0, 0,
                       (const cf64*)frames, (long long)nperseg, (long long)nseg, (long long)first, (long long)count, row0, (double*)acc);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());           // the chunk buffer is rewritten by the next ssfm_welch_frames
    return SSFM_OK;
}

extern "C" int ssfm_welch_finish(int device, const void* acc, int64_t rows, int64_t nperseg, double factor, int out_f32, void* out) {
    if (!acc || !out || rows < 1 || rows > 65535 || nperseg < 1) return fail(SSFM_ERR_INVALID, "ssfm_welch_finish: rows=%lld nperseg=%lld", (long long)rows, (long long)nperseg);
    if (int rc = use_device(device)) return rc;
    Scratch s(device);
    void* buf;
    if (int rc = s.get((size_t)(rows * nperseg) * (out_f32 ? 4 : 8), &buf)) return rc;
    if (int rc = fold_out((const double*)acc, rows, 1, nperseg, factor, out_f32, out, buf)) return rc;
    s.drained = true;
    return SSFM_OK;
}
