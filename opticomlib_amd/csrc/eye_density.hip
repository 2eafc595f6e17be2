// eye_density.hip -- the density grid of an eye diagram on gfx950: the device side of opticomlib_amd.utils.eye_density (reference utils.py:1593-1787,
// eyediagram: np.histogram2d of the traces' points, scipy.ndimage.gaussian_filter of the counts, and per plotted point the grid value that colours it).
// The record stays where it lies; what comes back is the B x B grid and, when colours are asked for, the T P plotted points.
//
//   ssfm_eye_density_range   k_minmax + k_minmax_fold: minimum, maximum and a non-finite flag of the plotted points in one pass
//   ssfm_eye_density         k_counts: a workgroup owns a run of traces and a run of grid columns, counts in LDS, one integer atomic per nonzero
//                            bin into the global uint32 grid; k_blur twice (axis 0, then axis 1, SciPy's order of terms);
//                            with colours k_colour_gather, k_minmax, k_minmax_fold, k_colour_norm
//   ssfm_eye_fold_range      k_fold_minmax + k_fold_minmax_fold: the same of a general fold's points (EyeFold in eye_density.inc: eye.plot's, reference
//                            typing.py:2718-2788) and of those whose phase passes a mask, with their number
//   ssfm_eye_fold_density    the kernels of ssfm_eye_density over the general fold -- a partial last trace, colours normalised over all points and
//                            kept for the drawn ones -- and k_hist_masked: np.histogram of the masked points, counted in LDS
// Integer counts and minima / maxima only meet across workgroups, every float sum runs in a fixed order: two calls give the same bits.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "ssfm_amd.h"
#include "ssfm_common.hpp"

#define EYE_HD __host__ __device__
#include "eye_density.inc"

using ssfm::fail;
using ssfm::grid_for;
using ssfm::Scratch;

namespace {

constexpr int kThreads = 256;
constexpr int kRedBlocks = 256;                    // workgroups of a minimum / maximum pass
constexpr int kTileWords = 16384;                  // uint32 counters a workgroup holds in LDS (64 KiB: two workgroups per CU)
constexpr long long kChunkPoints = 32768;          // points of a workgroup's traces, all phases taken together (mirrored by utils.EYE_CHUNK_POINTS)
constexpr int kMaxBins = 4096;                     // so that a tile always holds whole columns (kTileWords / kMaxBins = 4)
constexpr long long kMaxSamples = 1LL << 31;       // one bin can take every point: uint32 counters

enum { F_NAN = 1, F_INF = 2 };

// ------------------------------------------------------------------------------------------------ minimum, maximum, non-finite flag
// part[block] = {min, max, flags} of a[i] (+ b[i]), i < count.  NaN never enters min / max (the comparisons are false); an infinity does.
__global__ __launch_bounds__(kThreads) void k_minmax(const double* __restrict__ a, const double* __restrict__ b, long long count, double* __restrict__ part) {
    __shared__ double lmin[kThreads], lmax[kThreads];
    __shared__ int lflag[kThreads];
    double mn = INFINITY, mx = -INFINITY;
    int flag = 0;
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < count; i += (long long)gridDim.x * kThreads) {
        const double v = b ? a[i] + b[i] : a[i];
        if (v < mn) mn = v;
        if (v > mx) mx = v;
        if (v != v) flag |= F_NAN;
        else if (isinf(v)) flag |= F_INF;
    }
    const int tid = threadIdx.x;
    lmin[tid] = mn; lmax[tid] = mx; lflag[tid] = flag;
    __syncthreads();
    for (int off = kThreads / 2; off > 0; off >>= 1) {
        if (tid < off) {
            if (lmin[tid + off] < lmin[tid]) lmin[tid] = lmin[tid + off];
            if (lmax[tid + off] > lmax[tid]) lmax[tid] = lmax[tid + off];
            lflag[tid] |= lflag[tid + off];
        }
        __syncthreads();
    }
    if (tid == 0) {
        part[3 * blockIdx.x] = lmin[0];
        part[3 * blockIdx.x + 1] = lmax[0];
        part[3 * blockIdx.x + 2] = (double)lflag[0];
    }
}
__global__ __launch_bounds__(kThreads) void k_minmax_fold(const double* __restrict__ part, int nblocks, double* __restrict__ out) {
    __shared__ double lmin[kThreads], lmax[kThreads];
    __shared__ int lflag[kThreads];
    const int tid = threadIdx.x;
    double mn = INFINITY, mx = -INFINITY;
    int flag = 0;
    for (int k = tid; k < nblocks; k += kThreads) {
        if (part[3 * k] < mn) mn = part[3 * k];
        if (part[3 * k + 1] > mx) mx = part[3 * k + 1];
        flag |= (int)part[3 * k + 2];
    }
    lmin[tid] = mn; lmax[tid] = mx; lflag[tid] = flag;
    __syncthreads();
    for (int off = kThreads / 2; off > 0; off >>= 1) {
        if (tid < off) {
            if (lmin[tid + off] < lmin[tid]) lmin[tid] = lmin[tid + off];
            if (lmax[tid + off] > lmax[tid]) lmax[tid] = lmax[tid + off];
            lflag[tid] |= lflag[tid + off];
        }
        __syncthreads();
    }
    if (tid == 0) { out[0] = lmin[0]; out[1] = lmax[0]; out[2] = (double)lflag[0]; }
}

// ------------------------------------------------------------------------------------------------ counts
struct CountArgs {
    const double* y;         // the record
    const double* noise;     // nullable, likewise
    EyeFold f;               // point j < f.count is sample f.start + j at phase j mod f.P; the last trace may be partial
    const double* E;         // B + 1 edges of y (NumPy's bits, from the host)
    const int* xbin;         // P entries: the column of phase p (non-decreasing)
    const int* phase_lo;     // groups + 1 entries: column group g holds the phases phase_lo[g] ... phase_lo[g + 1] - 1
    unsigned* counts;        // B x B, counts[ix B + iy]
    long long T, chunk;      // traces in all and per workgroup
    int B, C;                // bins, columns per group (C B <= kTileWords)
};
// grid (trace chunks, column groups).  A column's phases are consecutive (the abscissa rises with the phase), so a group reads a run of w points of
// every trace; its C x B counters live in LDS and are flushed once, nonzero ones only.
__global__ __launch_bounds__(kThreads) void k_counts(const CountArgs a) {
    __shared__ unsigned tile[kTileWords];
    const int g = blockIdx.y, c0 = g * a.C, B = a.B;
    const int p_lo = a.phase_lo[g], w = a.phase_lo[g + 1] - p_lo;
    if (w <= 0) return;                                            // (uniform: a group of columns no phase falls in)
    const int ncols = B - c0 < a.C ? B - c0 : a.C, words = ncols * B;
    for (int k = threadIdx.x; k < words; k += kThreads) tile[k] = 0u;
    __syncthreads();
    const long long t0 = (long long)blockIdx.x * a.chunk;
    const long long t1 = t0 + a.chunk < a.T ? t0 + a.chunk : a.T;
    const long long total = (t1 - t0) * w;
    for (long long i = threadIdx.x; i < total; i += kThreads) {
        const long long t = t0 + i / w;
        const int p = p_lo + (int)(i % w);
        const long long j = t * a.f.P + p;
        if (j >= a.f.count) continue;                              // (the partial last trace of a general fold)
        const long long i_s = eye_fold_sample(a.f, j);
        const double v = a.noise ? a.y[i_s] + a.noise[i_s] : a.y[i_s];
        const int b = eye_bin(a.E, B, v);
        if (b >= 0) atomicAdd(&tile[(a.xbin[p] - c0) * B + b], 1u);
    }
    __syncthreads();
    unsigned* __restrict__ out = a.counts + (long long)c0 * B;
    for (int k = threadIdx.x; k < words; k += kThreads)
        if (tile[k]) atomicAdd(&out[k], tile[k]);
}

// ------------------------------------------------------------------------------------------------ blur
// One pass of scipy.ndimage.correlate1d with a symmetric kernel along AXIS of the B x B grid: w[0] in[i], then (in[i - k] + in[i + k]) w[k] from the
// farthest pair inwards (SciPy's loop), the line continued by reflection.  One thread per element.
template <typename Tin, int AXIS>
__global__ __launch_bounds__(kThreads) void k_blur(const Tin* __restrict__ in, const double* __restrict__ w, int r, int B, double* __restrict__ out) {
#pragma clang fp contract(off)
    const long long e = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (e >= (long long)B * B) return;
    const int i0 = (int)(e / B), i1 = (int)(e % B);
    const int pos = AXIS == 0 ? i0 : i1;
    const long long stride = AXIS == 0 ? B : 1, base = AXIS == 0 ? i1 : (long long)i0 * B;
    double acc = (double)in[e] * w[0];
    for (int k = r; k >= 1; --k) {
        const double lo = (double)in[base + stride * eye_reflect((long long)pos - k, B)];
        const double hi = (double)in[base + stride * eye_reflect((long long)pos + k, B)];
        acc += (lo + hi) * w[k];
    }
    out[e] = acc;
}
__global__ __launch_bounds__(kThreads) void k_widen(const unsigned* __restrict__ in, long long count, double* __restrict__ out) {
    const long long e = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (e < count) out[e] = (double)in[e];
}

// ------------------------------------------------------------------------------------------------ colours
// point j of the fold: value v, grid indices (xidx[phase], iy), colour G[ix, iy]; values and indices are kept for the drawn points
__global__ __launch_bounds__(kThreads) void k_colour_gather(const double* __restrict__ y, const double* __restrict__ noise, EyeFold f, int B,
                                                            const int* __restrict__ xidx, double lo, double hi, const double* __restrict__ G,
                                                            double* __restrict__ pts, int* __restrict__ iy, double* __restrict__ col) {
#pragma clang fp contract(off)
    for (long long j = (long long)blockIdx.x * kThreads + threadIdx.x; j < f.count; j += (long long)gridDim.x * kThreads) {
        const long long i_s = eye_fold_sample(f, j);
        const double v = noise ? y[i_s] + noise[i_s] : y[i_s];
        const int k = eye_grid_index(v, lo, hi, B);
        if (eye_fold_drawn(f, j)) {
            pts[j] = v;
            iy[j] = k;
        }
        col[j] = G[(long long)xidx[eye_fold_phase(f, j)] * B + k];
    }
}
// (c - c_min) / (c_max - c_min); range = {c_min, c_max}.  When the range is 0: `zero` -- zeros for eyediagram (reference utils.py:1718-1720), the
// NaN of 0 / 0 for eye.plot, which divides unguarded (typing.py:2757)
__global__ __launch_bounds__(kThreads) void k_colour_norm(double* __restrict__ col, long long count, const double* __restrict__ range, double zero) {
#pragma clang fp contract(off)
    const double cmin = range[0], span = range[1] - range[0];
    for (long long j = (long long)blockIdx.x * kThreads + threadIdx.x; j < count; j += (long long)gridDim.x * kThreads)
        col[j] = span == 0.0 ? zero : (col[j] - cmin) / span;
}

// ------------------------------------------------------------------------------------------------ the general fold: range and side histogram
// part[block] = {min, max, flags} of the `count` points and {min, max, flags, number} of those whose phase passes the mask (all, without a mask)
__global__ __launch_bounds__(kThreads) void k_fold_minmax(const double* __restrict__ y, EyeFold f, const unsigned char* __restrict__ mask, double* __restrict__ part) {
    __shared__ double lmin[2][kThreads], lmax[2][kThreads], lnum[kThreads];
    __shared__ int lflag[2][kThreads];
    double mn[2] = {INFINITY, INFINITY}, mx[2] = {-INFINITY, -INFINITY}, num = 0.0;
    int flag[2] = {0, 0};
    for (long long j = (long long)blockIdx.x * kThreads + threadIdx.x; j < f.count; j += (long long)gridDim.x * kThreads) {
        const double v = y[eye_fold_sample(f, j)];
        const int sets = eye_fold_masked(f, mask, j) ? 2 : 1;
        for (int k = 0; k < sets; ++k) {
            if (v < mn[k]) mn[k] = v;
            if (v > mx[k]) mx[k] = v;
            if (v != v) flag[k] |= F_NAN;
            else if (isinf(v)) flag[k] |= F_INF;
        }
        if (sets == 2) num += 1.0;                                 // (whole numbers below 2^31: exact in any order)
    }
    const int tid = threadIdx.x;
    for (int k = 0; k < 2; ++k) { lmin[k][tid] = mn[k]; lmax[k][tid] = mx[k]; lflag[k][tid] = flag[k]; }
    lnum[tid] = num;
    __syncthreads();
    for (int off = kThreads / 2; off > 0; off >>= 1) {
        if (tid < off) {
            for (int k = 0; k < 2; ++k) {
                if (lmin[k][tid + off] < lmin[k][tid]) lmin[k][tid] = lmin[k][tid + off];
                if (lmax[k][tid + off] > lmax[k][tid]) lmax[k][tid] = lmax[k][tid + off];
                lflag[k][tid] |= lflag[k][tid + off];
            }
            lnum[tid] += lnum[tid + off];
        }
        __syncthreads();
    }
    if (tid == 0) {
        double* o = part + 7 * blockIdx.x;
        o[0] = lmin[0][0]; o[1] = lmax[0][0]; o[2] = (double)lflag[0][0];
        o[3] = lmin[1][0]; o[4] = lmax[1][0]; o[5] = (double)lflag[1][0]; o[6] = lnum[0];
    }
}
// one workgroup: out (7) = the partials folded
__global__ __launch_bounds__(kThreads) void k_fold_minmax_fold(const double* __restrict__ part, int nblocks, double* __restrict__ out) {
    if (threadIdx.x != 0) return;                                  // at most kRedBlocks partials: one thread reads them in order
    double r[7] = {INFINITY, -INFINITY, 0.0, INFINITY, -INFINITY, 0.0, 0.0};
    for (int b = 0; b < nblocks; ++b) {
        const double* p = part + 7 * b;
        for (int k = 0; k < 6; k += 3) {
            if (p[k] < r[k]) r[k] = p[k];
            if (p[k + 1] > r[k + 1]) r[k + 1] = p[k + 1];
            r[k + 2] = (double)((int)r[k + 2] | (int)p[k + 2]);
        }
        r[6] += p[6];
    }
    for (int k = 0; k < 7; ++k) out[k] = r[k];
}
// np.histogram of the points whose phase passes the mask: H (<= kMaxBins) counters in LDS, the bin by eye_bin among the H + 1 edges, one flush
__global__ __launch_bounds__(kThreads) void k_hist_masked(const double* __restrict__ y, EyeFold f, const unsigned char* __restrict__ mask,
                                                          const double* __restrict__ E, int H, unsigned* __restrict__ hist) {
    __shared__ unsigned bins[kMaxBins];
    for (int k = threadIdx.x; k < H; k += kThreads) bins[k] = 0u;
    __syncthreads();
    for (long long j = (long long)blockIdx.x * kThreads + threadIdx.x; j < f.count; j += (long long)gridDim.x * kThreads) {
        if (!eye_fold_masked(f, mask, j)) continue;
        const int b = eye_bin(E, H, y[eye_fold_sample(f, j)]);
        if (b >= 0) atomicAdd(&bins[b], 1u);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < H; k += kThreads)
        if (bins[k]) atomicAdd(&hist[k], bins[k]);
}

size_t pad256(size_t b) { return (b + 255) & ~size_t(255); }

int check_record(const char* who, const double* y, int64_t n, int64_t sps, int64_t n_traces, EyeGeometry* g) {
    if (!y || n < 1 || n > kMaxSamples || sps < 1 || sps > (1 << 24))
        return fail(SSFM_ERR_INVALID, "%s: n=%lld sps=%lld (1 <= n <= 2^31 samples: the counters are uint32)", who, (long long)n, (long long)sps);
    *g = eye_geometry(n, sps, n_traces);
    if (g->err) return fail(SSFM_ERR_INVALID, "%s: n=%lld sps=%lld n_traces=%lld leave no trace (geometry error %d)", who, (long long)n, (long long)sps, (long long)n_traces, g->err);
    return SSFM_OK;
}

int check_fold(const char* who, const double* y, int64_t n, int64_t start, int64_t count, int64_t period, int64_t trace, int64_t n_draw, EyeFold* f) {
    *f = EyeFold{start, count, period, trace, n_draw, 0};
    if (!y || n < 1 || n > kMaxSamples || period > (1 << 25) || trace > (1 << 25) || (f->err = eye_fold_check(*f, n)))
        return fail(SSFM_ERR_INVALID, "%s: n=%lld start=%lld count=%lld period=%lld trace=%lld n_draw=%lld is no fold of the record (1 <= n <= 2^31, fold error %d)",
                    who, (long long)n, (long long)start, (long long)count, (long long)period, (long long)trace, (long long)n_draw, f->err);
    return SSFM_OK;
}

int minmax(const double* a, const double* b, long long count, double* part, double* out) {
    const int blocks = (int)grid_for(count, kRedBlocks);
    hipLaunchKernelGGL(k_minmax, dim3(blocks), dim3(kThreads), 0, 0, a, b, count, part);
    hipLaunchKernelGGL(k_minmax_fold, dim3(1), dim3(kThreads), 0, 0, (const double*)part, blocks, out);
    HIP_TRY(hipGetLastError());
    return SSFM_OK;
}

// What both density entry points run over the fold f of the record y (+ z): values, indices and colours come back for the drawn points, the colours
// normalised over all f.count, `zero` where their range is 0.  The side histogram (hist non-NULL) takes the points that pass `mask` (f.P bytes)
// into H bins among `hedges`.
struct DensityJob {
    const char* who;
    const double *y, *z;
    EyeFold f;
    double zero;
    const unsigned char* mask;
    int H;
    const double* hedges;
    uint32_t* hist;
};
int density(const DensityJob& J, int64_t bins, const double* yedges, const int32_t* xbin, const double* weights, int64_t radius, uint32_t* counts,
            double* grid, const int32_t* xidx, double min_y, double max_y, double* points, int32_t* iy, double* colors) {
    if (bins < 1 || bins > kMaxBins || !yedges || !xbin || !counts || !grid || (weights && radius < 0) || (xidx && !(points && iy && colors)))
        return fail(SSFM_ERR_INVALID, "%s: bins=%lld (1 ... %d) radius=%lld, or a NULL argument", J.who, (long long)bins, kMaxBins, (long long)radius);
    if (J.hist && (J.H < 1 || J.H > kMaxBins || !J.hedges || !J.mask))
        return fail(SSFM_ERR_INVALID, "%s: hbins=%d (1 ... %d), or a histogram without its mask or edges", J.who, J.H, kMaxBins);
    const int B = (int)bins, P = (int)J.f.P, H = J.hist ? J.H : 0;
    for (int p = 0; p < P; ++p)
        if (xbin[p] < 0 || xbin[p] >= B || (p && xbin[p] < xbin[p - 1]) || (xidx && (xidx[p] < 0 || xidx[p] >= B)))
            return fail(SSFM_ERR_INVALID, "%s: the column table is not a non-decreasing sequence within [0, %d) at phase %d", J.who, B, p);
    int device;
    if (int rc = ssfm::device_of(J.y, J.who, &device)) return rc;

    // the tables, assembled on the host and uploaded in one copy: edges | weights | minimum / maximum block | columns | colour columns | phase runs
    // | histogram edges | histogram counters | phase mask
    const int C = B < kTileWords / B ? B : kTileWords / B, groups = (B + C - 1) / C;
    const int r = weights ? (int)radius : 0;
    const size_t o_w = sizeof(double) * (B + 1), o_red = o_w + sizeof(double) * (r + 1), o_xbin = o_red + sizeof(double) * 3 * (kRedBlocks + 1);
    const size_t o_xidx = o_xbin + sizeof(int) * P, o_phase = o_xidx + sizeof(int) * P;
    const size_t o_hedges = (o_phase + sizeof(int) * (groups + 1) + 7) & ~size_t(7), o_hist = o_hedges + (H ? sizeof(double) * (H + 1) : 0);
    const size_t o_mask = o_hist + sizeof(unsigned) * H, tab_bytes = o_mask + (H ? P : 0);
    std::vector<unsigned char> tab(tab_bytes, 0);
    std::memcpy(tab.data(), yedges, sizeof(double) * (B + 1));
    if (weights) std::memcpy(tab.data() + o_w, weights, sizeof(double) * (r + 1));
    std::memcpy(tab.data() + o_xbin, xbin, sizeof(int) * P);
    if (xidx) std::memcpy(tab.data() + o_xidx, xidx, sizeof(int) * P);
    if (H) {
        std::memcpy(tab.data() + o_hedges, J.hedges, sizeof(double) * (H + 1));
        std::memcpy(tab.data() + o_mask, J.mask, P);
    }
    int* phase = reinterpret_cast<int*>(tab.data() + o_phase);
    for (int gi = 0, p = 0; gi <= groups; ++gi) {                    // the first phase whose column is gi C or beyond
        while (p < P && xbin[p] < gi * C) ++p;
        phase[gi] = gi == groups ? P : p;
    }

    const long long cells = (long long)B * B, npts = J.f.count, keep = xidx ? J.f.n_draw * J.f.L : 0;
    const long long T = (npts + P - 1) / P;
    Scratch s(device);
    void *dtab, *dgrid, *dpts = nullptr;
    if (int rc = s.get(pad256(tab_bytes), &dtab)) return rc;
    const size_t o_tmp = pad256(sizeof(unsigned) * cells), o_out = o_tmp + pad256(sizeof(double) * cells);
    if (int rc = s.get(o_out + sizeof(double) * cells, &dgrid)) return rc;
    const size_t o_col = pad256(sizeof(double) * npts), o_iy = 2 * o_col;
    if (keep)
        if (int rc = s.get(o_iy + sizeof(int) * npts, &dpts)) return rc;
    HIP_TRY(hipMemcpy(dtab, tab.data(), tab_bytes, hipMemcpyHostToDevice));
    unsigned* dcounts = (unsigned*)dgrid;
    double* dtmp = (double*)((char*)dgrid + o_tmp);
    double* dout = (double*)((char*)dgrid + o_out);
    const double* dE = (const double*)dtab;
    const double* dw = (const double*)((char*)dtab + o_w);
    double* dred = (double*)((char*)dtab + o_red);
    HIP_TRY(hipMemsetAsync(dcounts, 0, sizeof(unsigned) * cells, 0));

    long long chunk = kChunkPoints / P;
    if (chunk < 1) chunk = 1;
    const CountArgs ca{J.y, J.z, J.f, dE, (const int*)((char*)dtab + o_xbin), (const int*)((char*)dtab + o_phase), dcounts, T, chunk, B, C};
    hipLaunchKernelGGL(k_counts, dim3((unsigned)((T + chunk - 1) / chunk), (unsigned)groups), dim3(kThreads), 0, 0, ca);
    HIP_TRY(hipGetLastError());

    const dim3 cg((unsigned)((cells + kThreads - 1) / kThreads)), cb(kThreads);
    if (weights) {
        hipLaunchKernelGGL((k_blur<unsigned, 0>), cg, cb, 0, 0, (const unsigned*)dcounts, dw, r, B, dtmp);
        hipLaunchKernelGGL((k_blur<double, 1>), cg, cb, 0, 0, (const double*)dtmp, dw, r, B, dout);
    } else {
        hipLaunchKernelGGL(k_widen, cg, cb, 0, 0, (const unsigned*)dcounts, cells, dout);
    }
    HIP_TRY(hipGetLastError());
    if (H) {                                                         // (the counters were uploaded as zeros with the tables)
        hipLaunchKernelGGL(k_hist_masked, dim3(grid_for(npts, 64)), cb, 0, 0, J.y, J.f, (const unsigned char*)dtab + o_mask,
                           (const double*)((char*)dtab + o_hedges), H, (unsigned*)((char*)dtab + o_hist));
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpy(J.hist, (char*)dtab + o_hist, sizeof(unsigned) * H, hipMemcpyDeviceToHost));
    }
    if (keep) {
        double* dp = (double*)dpts;
        double* dc = (double*)((char*)dpts + o_col);
        int* di = (int*)((char*)dpts + o_iy);
        const dim3 pg(grid_for(npts, 4096));
        hipLaunchKernelGGL(k_colour_gather, pg, cb, 0, 0, J.y, J.z, J.f, B, (const int*)((char*)dtab + o_xidx), min_y, max_y, (const double*)dout, dp, di, dc);
        if (int rc = minmax(dc, nullptr, npts, dred + 3, dred)) return rc;
        hipLaunchKernelGGL(k_colour_norm, dim3(grid_for(keep, 4096)), cb, 0, 0, dc, keep, (const double*)dred, J.zero);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpy(points, dp, sizeof(double) * keep, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(iy, di, sizeof(int) * keep, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(colors, dc, sizeof(double) * keep, hipMemcpyDeviceToHost));
    }
    HIP_TRY(hipMemcpy(counts, dcounts, sizeof(unsigned) * cells, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(grid, dout, sizeof(double) * cells, hipMemcpyDeviceToHost));
    s.drained = true;
    return SSFM_OK;
}

}  // namespace

// ================================================================================================ C ABI
extern "C" int ssfm_eye_density_range(const double* y, const double* noise, int64_t n, int64_t sps, int64_t n_traces, double* out) {
    EyeGeometry g;
    if (!out) return fail(SSFM_ERR_INVALID, "ssfm_eye_density_range: out is NULL");
    if (int rc = check_record("ssfm_eye_density_range", y, n, sps, n_traces, &g)) return rc;
    int device;
    if (int rc = ssfm::device_of(y, "ssfm_eye_density_range", &device)) return rc;
    Scratch s(device);
    void* buf;
    if (int rc = s.get(sizeof(double) * 3 * (kRedBlocks + 1), &buf)) return rc;
    double* part = (double*)buf + 3;
    if (int rc = minmax(y + g.start, noise ? noise + g.start : nullptr, g.T * g.P, part, (double*)buf)) return rc;
    HIP_TRY(hipMemcpy(out, buf, sizeof(double) * 3, hipMemcpyDeviceToHost));
    s.drained = true;
    return SSFM_OK;
}

extern "C" int ssfm_eye_density(const double* y, const double* noise, int64_t n, int64_t sps, int64_t n_traces, int64_t bins, const double* yedges,
                                const int32_t* xbin, const double* weights, int64_t radius, uint32_t* counts, double* grid, const int32_t* xidx,
                                double min_y, double max_y, double* points, int32_t* iy, double* colors) {
    EyeGeometry g;
    if (int rc = check_record("ssfm_eye_density", y, n, sps, n_traces, &g)) return rc;
    const DensityJob J{"ssfm_eye_density", y, noise, EyeFold{g.start, g.T * g.P, g.P, g.P, g.T, 0}, 0.0, nullptr, 0, nullptr, nullptr};
    return density(J, bins, yedges, xbin, weights, radius, counts, grid, xidx, min_y, max_y, points, iy, colors);
}

extern "C" int ssfm_eye_fold_range(const double* y, int64_t n, int64_t start, int64_t count, int64_t period, const uint8_t* mask, double* out) {
    EyeFold f;
    if (!out) return fail(SSFM_ERR_INVALID, "ssfm_eye_fold_range: out is NULL");
    if (int rc = check_fold("ssfm_eye_fold_range", y, n, start, count, period, period, 0, &f)) return rc;
    int device;
    if (int rc = ssfm::device_of(y, "ssfm_eye_fold_range", &device)) return rc;
    Scratch s(device);
    void* buf;
    const size_t o_mask = sizeof(double) * 7 * (kRedBlocks + 1);
    if (int rc = s.get(o_mask + (mask ? (size_t)period : 0), &buf)) return rc;
    unsigned char* dmask = mask ? (unsigned char*)buf + o_mask : nullptr;
    if (mask) HIP_TRY(hipMemcpy(dmask, mask, (size_t)period, hipMemcpyHostToDevice));
    double* part = (double*)buf + 7;
    const int blocks = (int)grid_for(count, kRedBlocks);
    hipLaunchKernelGGL(k_fold_minmax, dim3(blocks), dim3(kThreads), 0, 0, y, f, (const unsigned char*)dmask, part);
    hipLaunchKernelGGL(k_fold_minmax_fold, dim3(1), dim3(kThreads), 0, 0, (const double*)part, blocks, (double*)buf);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out, buf, sizeof(double) * 7, hipMemcpyDeviceToHost));
    s.drained = true;
    return SSFM_OK;
}

extern "C" int ssfm_eye_fold_density(const double* y, int64_t n, int64_t start, int64_t count, int64_t period, int64_t trace, int64_t n_draw, int64_t bins,
                                     const double* yedges, const int32_t* xbin, const double* weights, int64_t radius, uint32_t* counts, double* grid,
                                     const int32_t* xidx, double min_y, double max_y, double* points, int32_t* iy, double* colors, const uint8_t* mask,
                                     int64_t hbins, const double* hedges, uint32_t* hist) {
    EyeFold f;
    if (int rc = check_fold("ssfm_eye_fold_density", y, n, start, count, period, trace, n_draw, &f)) return rc;
    if (hist && (hbins < 1 || hbins > kMaxBins)) return fail(SSFM_ERR_INVALID, "ssfm_eye_fold_density: hbins=%lld (1 ... %d)", (long long)hbins, kMaxBins);
    const DensityJob J{"ssfm_eye_fold_density", y, nullptr, f, (double)NAN, mask, (int)hbins, hedges, hist};
    return density(J, bins, yedges, xbin, weights, radius, counts, grid, xidx, min_y, max_y, points, iy, colors);
}
