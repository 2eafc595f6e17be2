// coherent.hip -- the coherent square-QAM receiver on gfx950: the Gray mapper, the decisions, the blind phase search (BPS) that recovers the carrier
// phase of a record of one sample per symbol, and the sums behind the quarter-turn alignment and the error vector magnitude.  All arithmetic is float64;
// a complex64 sample is widened exactly.  The geometry and every integer rule come from coherent_tiles.hpp.
//
//   * ssfm_qam_encode   one thread per symbol: the k bits (MSB first; a nonzero byte is a 1) as two Gray-coded levels, a (2 g - (L - 1)) each;
//   * ssfm_qam_decide   one thread per symbol: z turned by i^-turns, both components decided (level_of), then the k bits and / or the turned symbol
//                       written;
//   * ssfm_qam_sums     per-workgroup partial sums of z conj(s), |i^-turns z - s|^2 and |s|^2 (s: the reference symbols, or the decisions of the
//                       turned z), folded in a fixed tree and added on the host in block order: the same bits on every call;
//   * ssfm_cpr_power    mean |x|^2 of the symbols read at x[row pitch + start + k step], the same way;
//   * ssfm_cpr_search   the phase search, three launches:
//       k_search        a workgroup owns a tile of kTile symbols of one row and a halo of W on each side.  Its threads read those symbols once (strided,
//                       scaled) and keep them in registers; for each group of kGroup test phases they write the distances d[p][symbol] into LDS, each
//                       once, and every thread then sums the window of its own symbol straight from LDS -- a sum of that window's own terms, nothing
//                       carried from symbol to symbol -- with the running argmin in registers.  The chosen phase of every symbol goes out, and the sum
//                       of the jumps inside the tile;
//       k_tile_offsets  a workgroup per row: the jumps of each tile (those inside it and the one across its lower seam), scanned over the tiles;
//       k_unwrap        a workgroup per tile again: the jumps of its symbols, scanned, on top of the tile's offset give n_k; u_k, the phase and the
//                       symbol turned by the table's entry and the exact quarter turns (-i)^n_k go out.  The symbols are read a second time here.
//     No atomics, no float sum whose order depends on the schedule: the same bits on every call.  A non-finite sample is outside the contract: a NaN
//     compares false, so the argmin stays where the comparison leaves it (at the first phase when every sum is a NaN), every output is still written.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "coherent_tiles.hpp"
#include "ssfm_amd.h"
#include "ssfm_common.hpp"

using ssfm::fail;
using ssfm::grid_for;
using ssfm::Scratch;
namespace cpr = ssfm::cpr;

namespace {

constexpr int kThreads = cpr::kTile;
constexpr int kWaves = kThreads / 64;
constexpr int kSumBlocks = 1024;                   // most workgroups of a reduction: its partials are added on the host in block order
constexpr int kEntriesPerThread = (cpr::halo_entries(cpr::kMaxWindow) + kThreads - 1) / kThreads;

struct Cx {
    double re, im;
};

// sample `i` of a complex64 or complex128 array, widened
template <bool C64>
__device__ __forceinline__ Cx load_cx(const void* x, long long i) {
    if (C64) {
        const float2 v = ((const float2*)x)[i];
        return {(double)v.x, (double)v.y};
    }
    const double2 v = ((const double2*)x)[i];
    return {v.x, v.y};
}

// A strided record: symbol k of row r is scale[r] * x[r pitch + start + k step]
struct Record {
    const void* x;
    long long n, start, step, pitch;
    double scale[cpr::kMaxRows];
};

template <bool C64>
__device__ __forceinline__ Cx load_symbol(const Record& rec, int row, long long k) {
    const Cx v = load_cx<C64>(rec.x, (long long)row * rec.pitch + rec.start + k * rec.step);
    return {v.re * rec.scale[row], v.im * rec.scale[row]};
}

// z i^-t
__device__ __forceinline__ Cx quarter_turns(Cx z, int t) {
    switch (t & 3) {
        case 1: return {z.im, -z.re};
        case 2: return {-z.re, -z.im};
        case 3: return {-z.im, z.re};
        default: return z;
    }
}

// Sum of one double per thread over the workgroup in a fixed tree; every thread gets it.
__device__ double block_sum(double v, double* lds) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) s += lds[w];
    return s;
}

// Inclusive prefix sum of one int per thread over the workgroup; *total gets the sum.
__device__ int block_inclusive_scan(int v, int* lds, int* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_up(incl, off);
        if (lane >= off) incl += o;
    }
    __syncthreads();
    if (lane == 63) lds[wave] = incl;
    __syncthreads();
    int before = 0, sum = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
        before += w < wave ? lds[w] : 0;
        sum += lds[w];
    }
    *total = sum;
    return before + incl;
}

// ------------------------------------------------------------------------------------------------ mapper and decisions
__global__ __launch_bounds__(kThreads) void k_qam_encode(const unsigned char* __restrict__ bits, long long nsym, int k, int L, double a, double2* __restrict__ out) {
    const int half = k / 2;
    for (long long s = (long long)blockIdx.x * kThreads + threadIdx.x; s < nsym; s += (long long)gridDim.x * kThreads) {
        int ci = 0, cq = 0;
        for (int b = 0; b < half; ++b) {
            ci = (ci << 1) | (bits[s * k + b] != 0);
            cq = (cq << 1) | (bits[s * k + half + b] != 0);
        }
        out[s] = make_double2(cpr::level_amp(cpr::gray_decode(ci), a, L), cpr::level_amp(cpr::gray_decode(cq), a, L));
    }
}

__global__ __launch_bounds__(kThreads) void k_qam_decide(const double2* __restrict__ z, long long n, int k, int L, double a, int turns, unsigned char* __restrict__ bits,
                                                         double2* __restrict__ turned) {
    const int half = k / 2;
    for (long long s = (long long)blockIdx.x * kThreads + threadIdx.x; s < n; s += (long long)gridDim.x * kThreads) {
        const Cx v = quarter_turns({z[s].x, z[s].y}, turns);
        const int gi = cpr::level_of(v.re, a, L), gq = cpr::level_of(v.im, a, L);
        if (bits) {
            const int ci = cpr::gray_encode(gi), cq = cpr::gray_encode(gq);
            for (int b = 0; b < half; ++b) {
                bits[s * k + b] = (ci >> (half - 1 - b)) & 1;
                bits[s * k + half + b] = (cq >> (half - 1 - b)) & 1;
            }
        }
        if (turned) turned[s] = make_double2(v.re, v.im);
    }
}

// partial[4 block ...] = sum z conj(s) (re, im), sum |i^-turns z - s|^2, sum |s|^2 over the block's symbols
__global__ __launch_bounds__(kThreads) void k_qam_sums(const double2* __restrict__ z, const double2* __restrict__ ref, long long n, int L, double a, int turns,
                                                       double* __restrict__ partial) {
    __shared__ double lds[kWaves];
    double cr = 0.0, ci = 0.0, e2 = 0.0, s2 = 0.0;
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long long)gridDim.x * kThreads) {
        const Cx raw = {z[i].x, z[i].y};
        const Cx v = quarter_turns(raw, turns);
        Cx s;
        if (ref) s = {ref[i].x, ref[i].y};
        else s = {cpr::level_amp(cpr::level_of(v.re, a, L), a, L), cpr::level_amp(cpr::level_of(v.im, a, L), a, L)};
        cr += raw.re * s.re + raw.im * s.im;
        ci += raw.im * s.re - raw.re * s.im;
        const double dr = v.re - s.re, di = v.im - s.im;
        e2 += dr * dr + di * di;
        s2 += s.re * s.re + s.im * s.im;
    }
    cr = block_sum(cr, lds);
    ci = block_sum(ci, lds);
    e2 = block_sum(e2, lds);
    s2 = block_sum(s2, lds);
    if (threadIdx.x == 0) {
        partial[4 * blockIdx.x + 0] = cr;
        partial[4 * blockIdx.x + 1] = ci;
        partial[4 * blockIdx.x + 2] = e2;
        partial[4 * blockIdx.x + 3] = s2;
    }
}

// partial[row gridDim.x + block] = sum |x|^2 over the block's symbols of the row (the record's scale is not applied)
template <bool C64>
__global__ __launch_bounds__(kThreads) void k_cpr_power(Record rec, double* __restrict__ partial) {
    __shared__ double lds[kWaves];
    const int row = blockIdx.y;
    double p = 0.0;
    for (long long k = (long long)blockIdx.x * kThreads + threadIdx.x; k < rec.n; k += (long long)gridDim.x * kThreads) {
        const Cx v = load_cx<C64>(rec.x, (long long)row * rec.pitch + rec.start + k * rec.step);
        p += v.re * v.re + v.im * v.im;
    }
    p = block_sum(p, lds);
    if (threadIdx.x == 0) partial[(long long)row * gridDim.x + blockIdx.x] = p;
}

// ------------------------------------------------------------------------------------------------ blind phase search
struct Search {
    Record rec;
    int L, B, W;
    double a, phase_step;
    long long tiles;
    double table[2 * cpr::kMaxPhases];     // exp(-i phi_b): re, im
};

// |r - dec(r)|^2
__device__ __forceinline__ double distance2(double rr, double ri, double a, int L) {
    const double dr = rr - cpr::level_amp(cpr::level_of(rr, a, L), a, L), di = ri - cpr::level_amp(cpr::level_of(ri, a, L), a, L);
    return dr * dr + di * di;
}

template <bool C64>
__global__ __launch_bounds__(kThreads) void k_search(Search s, int* __restrict__ bhat, int* __restrict__ counts) {
    extern __shared__ double d[];                                  // [kGroup][entries]; after the last group its head holds the chosen phases
    int* const chosen = (int*)d;                                   // (kThreads + kWaves ints: less than one row of d at W = 0)
    int* const wave_jumps = chosen + kThreads;
    const int tid = threadIdx.x;
    const long long t = blockIdx.x % s.tiles;
    const int row = (int)(blockIdx.x / s.tiles);
    const long long n = s.rec.n;
    const int W = s.W, B = s.B, entries = cpr::halo_entries(W);
    const long long base = cpr::halo_base(t, W), hb = cpr::halo_begin(t, W), he = cpr::halo_end(t, W, n);

    // the tile's symbols and its halo, read once: entry e = tid + c kTile holds symbol base + e
    Cx y[kEntriesPerThread];
    bool have[kEntriesPerThread];
#pragma unroll
    for (int c = 0; c < kEntriesPerThread; ++c) {
        const int e = tid + c * kThreads;
        const long long j = base + e;
        have[c] = e < entries && j >= hb && j < he;
        y[c] = have[c] ? load_symbol<C64>(s.rec, row, j) : Cx{0.0, 0.0};
    }

    const long long k = cpr::tile_begin(t) + tid;
    const bool valid = k < cpr::tile_end(t, n);
    const int wb = valid ? (int)(cpr::window_begin(k, W) - base) : 0, we = valid ? (int)(cpr::window_end(k, W, n) - base) : 0;
    double best_s = 0.0;
    int best_b = 0;
    for (int g = 0; g < cpr::groups_of(B); ++g) {
        const int pb = cpr::group_begin(g), np = cpr::group_end(g, B) - pb;
#pragma unroll
        for (int c = 0; c < kEntriesPerThread; ++c) {
            if (!have[c]) continue;
            const int e = tid + c * kThreads;
            for (int q = 0; q < np; ++q) {
                const double tr = s.table[2 * (pb + q)], ti = s.table[2 * (pb + q) + 1];
                d[q * entries + e] = distance2(y[c].re * tr - y[c].im * ti, y[c].re * ti + y[c].im * tr, s.a, s.L);
            }
        }
        __syncthreads();
        double acc[cpr::kGroup];
#pragma unroll
        for (int q = 0; q < cpr::kGroup; ++q) acc[q] = 0.0;
        for (int e = wb; e < we; ++e) {
#pragma unroll
            for (int q = 0; q < cpr::kGroup; ++q)
                if (q < np) acc[q] += d[q * entries + e];
        }
#pragma unroll
        for (int q = 0; q < cpr::kGroup; ++q) {
            if (q >= np) continue;
            if ((g == 0 && q == 0) || acc[q] < best_s) {
                best_s = acc[q];
                best_b = pb + q;
            }
        }
        __syncthreads();
    }

    // the chosen phases, and the jumps between neighbours inside the tile (the one across the tile's lower seam is k_tile_offsets')
    chosen[tid] = best_b;
    __syncthreads();
    int jump = (valid && tid > 0) ? cpr::jump_of(chosen[tid - 1], best_b, B) : 0;
    if (valid) bhat[(long long)row * n + k] = best_b;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) jump += __shfl_xor(jump, off);
    if ((tid & 63) == 0) wave_jumps[tid >> 6] = jump;
    __syncthreads();
    if (tid == 0) {
        int sum = 0;
        for (int w = 0; w < kWaves; ++w) sum += wave_jumps[w];
        counts[blockIdx.x] = sum;
    }
}

// One workgroup per row: offs[row tiles + t] = the jumps of all symbols below tile t = n_k of the symbol before the tile
__global__ __launch_bounds__(kThreads) void k_tile_offsets(const int* __restrict__ bhat, const int* __restrict__ counts, long long n, long long tiles, int B,
                                                           int* __restrict__ offs) {
    __shared__ int lds[kWaves];
    const int row = blockIdx.x;
    const int* b = bhat + (long long)row * n;
    int carry = 0;
    for (long long t0 = 0; t0 < tiles; t0 += kThreads) {
        const long long t = t0 + threadIdx.x;
        int v = 0;
        if (t < tiles) {
            v = counts[(long long)row * tiles + t];
            if (t > 0) v += cpr::jump_of(b[cpr::tile_begin(t) - 1], b[cpr::tile_begin(t)], B);
        }
        int total;
        const int incl = block_inclusive_scan(v, lds, &total);
        if (t < tiles) offs[(long long)row * tiles + t] = carry + incl - v;
        carry += total;
        __syncthreads();
    }
}

template <bool C64>
__global__ __launch_bounds__(kThreads) void k_unwrap(Search s, const int* __restrict__ bhat, const int* __restrict__ offs, int* __restrict__ index,
                                                     double* __restrict__ phase, double2* __restrict__ symbols) {
    __shared__ int lds[kWaves];
    __shared__ double table[2 * cpr::kMaxPhases];
    const int tid = threadIdx.x;
    if (tid < 2 * s.B) table[tid] = s.table[tid];
    const long long t = blockIdx.x % s.tiles;
    const int row = (int)(blockIdx.x / s.tiles);
    const long long n = s.rec.n, k = cpr::tile_begin(t) + tid;
    const bool valid = k < cpr::tile_end(t, n);
    const int* b = bhat + (long long)row * n;
    const int cur = valid ? b[k] : 0;
    const int jump = (valid && k > 0) ? cpr::jump_of(b[k - 1], cur, s.B) : 0;
    int total;
    const int turns = offs[blockIdx.x] + block_inclusive_scan(jump, lds, &total);      // n_k (the barriers inside also publish the table)
    if (!valid) return;
    const int u = cur + s.B * turns;
    const Cx y = load_symbol<C64>(s.rec, row, k);
    // exp(-i phi_k) = exp(-i phi_b) (-i)^n_k: the table's entry and exact quarter turns
    const Cx e = quarter_turns({table[2 * cur], table[2 * cur + 1]}, turns);
    const long long o = (long long)row * n + k;
    index[o] = u;
    phase[o] = (double)(u - s.B / 2) * s.phase_step;
    symbols[o] = make_double2(y.re * e.re - y.im * e.im, y.re * e.im + y.im * e.re);
}

int check_record(const char* who, const void* x, int rows, int64_t n, int64_t start, int64_t step, int64_t pitch) {
    if (!x || rows < 1 || rows > cpr::kMaxRows || n < 1 || n > cpr::kMaxSymbols || start < 0 || step < 1 || start + (n - 1) * step >= pitch)
        return fail(SSFM_ERR_INVALID, "%s: rows=%d n=%lld start=%lld step=%lld pitch=%lld", who, rows, (long long)n, (long long)start, (long long)step, (long long)pitch);
    return SSFM_OK;
}

}  // namespace

// ================================================================================================ C ABI
extern "C" int ssfm_qam_encode(const unsigned char* bits, int64_t nsym, int M, double a, void* out) {
    if (!bits || !out || nsym < 0 || !cpr::valid_order(M) || !(a > 0.0)) return fail(SSFM_ERR_INVALID, "ssfm_qam_encode: nsym=%lld M=%d a=%g", (long long)nsym, M, a);
    if (nsym == 0) return SSFM_OK;
    int device;
    if (int rc = ssfm::device_of(bits, "ssfm_qam_encode", &device)) return rc;
    hipLaunchKernelGGL(k_qam_encode, dim3(grid_for(nsym, 4096)), dim3(kThreads), 0, 0, bits, (long long)nsym, cpr::bits_of(M), cpr::side_of(M), a, (double2*)out);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    return SSFM_OK;
}

extern "C" int ssfm_qam_decide(const void* z, int64_t n, int M, double a, int turns, unsigned char* bits, void* turned) {
    if (!z || n < 0 || !cpr::valid_order(M) || !(a > 0.0) || turns < 0 || turns > 3 || (!bits && !turned))
        return fail(SSFM_ERR_INVALID, "ssfm_qam_decide: n=%lld M=%d a=%g turns=%d", (long long)n, M, a, turns);
    if (n == 0) return SSFM_OK;
    int device;
    if (int rc = ssfm::device_of(z, "ssfm_qam_decide", &device)) return rc;
    hipLaunchKernelGGL(k_qam_decide, dim3(grid_for(n, 4096)), dim3(kThreads), 0, 0, (const double2*)z, (long long)n, cpr::bits_of(M), cpr::side_of(M), a, turns, bits,
                       (double2*)turned);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    return SSFM_OK;
}

extern "C" int ssfm_qam_sums(const void* z, const void* ref, int64_t n, int M, double a, int turns, double* out) {
    if (!z || !out || n < 1 || turns < 0 || turns > 3 || (!ref && (!cpr::valid_order(M) || !(a > 0.0))))
        return fail(SSFM_ERR_INVALID, "ssfm_qam_sums: n=%lld M=%d a=%g turns=%d", (long long)n, M, a, turns);
    int device;
    if (int rc = ssfm::device_of(z, "ssfm_qam_sums", &device)) return rc;
    Scratch s(device);
    const unsigned blocks = grid_for(n, kSumBlocks);
    void* partial;
    if (int rc = s.get(sizeof(double) * 4 * blocks, &partial)) return rc;
    hipLaunchKernelGGL(k_qam_sums, dim3(blocks), dim3(kThreads), 0, 0, (const double2*)z, (const double2*)ref, (long long)n, ref ? 2 : cpr::side_of(M), a, turns,
                       (double*)partial);
    HIP_TRY(hipGetLastError());
    static thread_local double host[4 * kSumBlocks];
    HIP_TRY(hipMemcpy(host, partial, sizeof(double) * 4 * blocks, hipMemcpyDeviceToHost));          // blocking: the kernel has finished too
    s.drained = true;
    for (int c = 0; c < 4; ++c) out[c] = 0.0;
    for (unsigned b = 0; b < blocks; ++b)
        for (int c = 0; c < 4; ++c) out[c] += host[4 * b + c];
    return SSFM_OK;
}

extern "C" int ssfm_cpr_power(const void* x, int is_c64, int rows, int64_t n, int64_t start, int64_t step, int64_t pitch, double* out) {
    if (int rc = check_record("ssfm_cpr_power", x, rows, n, start, step, pitch)) return rc;
    if (!out) return fail(SSFM_ERR_INVALID, "ssfm_cpr_power: no output");
    int device;
    if (int rc = ssfm::device_of(x, "ssfm_cpr_power", &device)) return rc;
    Scratch s(device);
    const unsigned blocks = grid_for(n, kSumBlocks);
    void* partial;
    if (int rc = s.get(sizeof(double) * rows * blocks, &partial)) return rc;
    Record rec{x, (long long)n, (long long)start, (long long)step, (long long)pitch, {1.0, 1.0}};
    if (is_c64) hipLaunchKernelGGL(k_cpr_power<true>, dim3(blocks, rows), dim3(kThreads), 0, 0, rec, (double*)partial);
    else hipLaunchKernelGGL(k_cpr_power<false>, dim3(blocks, rows), dim3(kThreads), 0, 0, rec, (double*)partial);
    HIP_TRY(hipGetLastError());
    static thread_local double host[cpr::kMaxRows * kSumBlocks];
    HIP_TRY(hipMemcpy(host, partial, sizeof(double) * rows * blocks, hipMemcpyDeviceToHost));
    s.drained = true;
    for (int r = 0; r < rows; ++r) {
        double p = 0.0;
        for (unsigned b = 0; b < blocks; ++b) p += host[(size_t)r * blocks + b];
        out[r] = p / (double)n;
    }
    return SSFM_OK;
}

extern "C" int ssfm_cpr_search(const void* x, int is_c64, int rows, int64_t n, int64_t start, int64_t step, int64_t pitch, const double* scale, int M,
                               double a, int test_phases, int window, const double* table, double phase_step, int32_t* index, double* phase, void* symbols) {
    if (int rc = check_record("ssfm_cpr_search", x, rows, n, start, step, pitch)) return rc;
    if (!scale || !table || !index || !phase || !symbols || !cpr::valid_order(M) || !(a > 0.0) || !cpr::valid_search(test_phases, window, n, rows))
        return fail(SSFM_ERR_INVALID, "ssfm_cpr_search: M=%d a=%g test_phases=%d window=%d n=%lld rows=%d", M, a, test_phases, window, (long long)n, rows);
    int device;
    if (int rc = ssfm::device_of(x, "ssfm_cpr_search", &device)) return rc;
    Search s{};
    s.rec = Record{x, (long long)n, (long long)start, (long long)step, (long long)pitch, {scale[0], rows > 1 ? scale[1] : scale[0]}};
    s.L = cpr::side_of(M);
    s.B = test_phases;
    s.W = window;
    s.a = a;
    s.phase_step = phase_step;
    s.tiles = cpr::tiles_of(n);
    std::memcpy(s.table, table, sizeof(double) * 2 * test_phases);
    const unsigned grid = (unsigned)cpr::grid_of(rows, n);
    Scratch scratch(device);
    void *bhat, *counts, *offs;
    if (int rc = scratch.get(sizeof(int) * (size_t)rows * n, &bhat)) return rc;
    if (int rc = scratch.get(sizeof(int) * grid, &counts)) return rc;
    if (int rc = scratch.get(sizeof(int) * grid, &offs)) return rc;
    const size_t lds = cpr::search_lds_bytes(window);
    static_assert(cpr::kSearchLdsMax <= 48 * 1024, "the search's LDS stays within what a kernel may use unasked");
    if (is_c64) hipLaunchKernelGGL(k_search<true>, dim3(grid), dim3(kThreads), lds, 0, s, (int*)bhat, (int*)counts);
    else hipLaunchKernelGGL(k_search<false>, dim3(grid), dim3(kThreads), lds, 0, s, (int*)bhat, (int*)counts);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_tile_offsets, dim3(rows), dim3(kThreads), 0, 0, (const int*)bhat, (const int*)counts, (long long)n, (long long)s.tiles, test_phases, (int*)offs);
    HIP_TRY(hipGetLastError());
    if (is_c64) hipLaunchKernelGGL(k_unwrap<true>, dim3(grid), dim3(kThreads), 0, 0, s, (const int*)bhat, (const int*)offs, (int*)index, phase, (double2*)symbols);
    else hipLaunchKernelGGL(k_unwrap<false>, dim3(grid), dim3(kThreads), 0, 0, s, (const int*)bhat, (const int*)offs, (int*)index, phase, (double2*)symbols);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    scratch.drained = true;
    return SSFM_OK;
}
