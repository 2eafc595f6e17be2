// manakov.hip -- FIBER / DBP of a dual-polarisation field with Manakov coupling (ssfm_manakov_propagate).
//
// The reference's loop (devices.py:1172-1196) rotates each polarisation by its own |A|^2: a dual-polarisation field is a batch of two scalar fibres.  Here
// the nonlinear phase of both rows follows the power in both,
//     g = gamma kappa,   P = |A_0|^2 + |A_1|^2,   N^ = i g P        (the same for both rows; stale over the step, as the reference's N^)
//     A <- A exp(h/2 N^);  A <- fft(A);  A <- A exp(D~ h);  A <- ifft(A);  A <- A exp(h/2 N^)
//     adaptive:  h = phi_max / max_n(|g| P), then min(h, L - z)
// in the plan's real type (float32 on a complex64 plan: the reference's arithmetic).  Built beside the fused engines from pieces the library has: the
// linear step is the plan's table transform x <- ifft(fft(x) H) (ssfm_apply_table, three launches) with H = exp(D~ h) / n in a table slot, the step
// control is the launch-per-pass line's (chirpz.hip k_chirp_control).  What is new is one pointwise kernel over both rows.  A rotation leaves |A| as it
// is, so P behind the closing half rotation of step k is the P step k + 1 starts from: the closing rotation of one step and the opening one of the next
// are ONE pass -- read both rows and the stale P, write both rows and the new P -- and a fixed step is four launches.  An adaptive step needs max P
// before the opening rotation can be sized: a pass that only reads the rows and reduces the maximum, the one-thread step control, the table
// exp(D~ h) / n formed from the device's h, then the rotation: seven launches.
//
// ssfm_manakov_pmd_propagate: the Manakov-PMD equation in the coarse-step (waveplate) model, one section per step.  Step k of size h turns the axes by a
// unitary U_k behind the opening half rotation and delays the rows against each other by tau = D_p sqrt(h) in the linear step,
//     A <- A exp(h/2 N^);  A <- U_k A;  A <- fft(A);  A_r <- A_r exp(D~ h -+ i w tau / 2);  A <- ifft(A);  A <- A exp(h/2 N^)        (- for row 0: delayed)
// A unitary leaves P as it is, so the fused closing / opening pass, the stale P and the step rule are the plain line's; U_k rides in that pass (no launch
// more), and the linear step is the plan's table transform with a table PER ROW (plan_apply_row_tables: the row pass in FM_TABLE_ROWS).  The launches per
// step are the plain line's; a step reads 2 n table entries where the plain line reads n twice.  The plain line's kernels are the PMD = false
// instantiations and compute what they computed.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "ssfm_amd.h"
#include "ssfm_common.hpp"
#include "ssfm_capture.hpp"
#include "ssfm_kernels.hpp"

using ssfm::fail;
using ssfm::grid_for;

namespace {

using ssfm::cx;

// Step control of an adaptive run: the kernels of a step take its size from here.  Steps are queued ahead of the host's knowledge of the end; `state` says what
// they still have to do: 0 = the run goes on; 1 = z has reached the length (or the step budget is used up): the rotation pass closes the last step into the
// run's RESULT buffer, everything else of the step returns at once; 2 = over: every kernel of the line returns at once.  (The three launches of the table
// transform know nothing of this and go on transforming the plan's field buffer: that is why the last step's result lies somewhere else.)
struct ManakovCtl {
    double h;                  // size of the step about to be taken [km] (a float32 value on a complex64 plan)
    double h_prev;             // ... of the step before it (the closing half rotation's)
    double z;                  // position reached at the end of the step about to be taken
    int state;
    int steps;                 // steps taken so far
    unsigned long long maxbits;    // bit pattern of max P (non-negative values order like integers); a float's in the low word
};

template <typename T> struct Bits;
template <> struct Bits<float> {
    using type = unsigned;
    static __device__ __forceinline__ unsigned of(float v) { return __float_as_uint(v); }
    static __device__ __forceinline__ float back(unsigned long long w) { return __uint_as_float((unsigned)w); }
};
template <> struct Bits<double> {
    using type = unsigned long long;
    static __device__ __forceinline__ unsigned long long of(double v) { return (unsigned long long)__double_as_longlong(v); }
    static __device__ __forceinline__ double back(unsigned long long w) { return __longlong_as_double((long long)w); }
};

// W consecutive samples of a row as 16-byte accesses (complex64: two float4 = 4 samples; complex128: two double2 = 2 samples)
template <typename T> struct Vec;
template <> struct Vec<float> {
    static constexpr int W = 4;
    static __device__ __forceinline__ void load(const ssfm::cf32* p, ssfm::cf32 (&v)[4]) {
        const float4 a = reinterpret_cast<const float4*>(p)[0], b = reinterpret_cast<const float4*>(p)[1];
        v[0] = ssfm::mk<float>(a.x, a.y); v[1] = ssfm::mk<float>(a.z, a.w); v[2] = ssfm::mk<float>(b.x, b.y); v[3] = ssfm::mk<float>(b.z, b.w);
    }
    static __device__ __forceinline__ void store(ssfm::cf32* p, const ssfm::cf32 (&v)[4]) {
        reinterpret_cast<float4*>(p)[0] = make_float4(v[0].x, v[0].y, v[1].x, v[1].y);
        reinterpret_cast<float4*>(p)[1] = make_float4(v[2].x, v[2].y, v[3].x, v[3].y);
    }
    static __device__ __forceinline__ void load_real(const float* p, float (&v)[4]) {
        const float4 a = reinterpret_cast<const float4*>(p)[0];
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    }
    static __device__ __forceinline__ void store_real(float* p, const float (&v)[4]) { reinterpret_cast<float4*>(p)[0] = make_float4(v[0], v[1], v[2], v[3]); }
};
template <> struct Vec<double> {
    static constexpr int W = 2;
    static __device__ __forceinline__ void load(const ssfm::cf64* p, ssfm::cf64 (&v)[2]) {
        const double2 a = reinterpret_cast<const double2*>(p)[0], b = reinterpret_cast<const double2*>(p)[1];
        v[0] = ssfm::mk<double>(a.x, a.y); v[1] = ssfm::mk<double>(b.x, b.y);
    }
    static __device__ __forceinline__ void store(ssfm::cf64* p, const ssfm::cf64 (&v)[2]) {
        reinterpret_cast<double2*>(p)[0] = make_double2(v[0].x, v[0].y);
        reinterpret_cast<double2*>(p)[1] = make_double2(v[1].x, v[1].y);
    }
    static __device__ __forceinline__ void load_real(const double* p, double (&v)[2]) {
        const double2 a = reinterpret_cast<const double2*>(p)[0];
        v[0] = a.x; v[1] = a.y;
    }
    static __device__ __forceinline__ void store_real(double* p, const double (&v)[2]) { reinterpret_cast<double2*>(p)[0] = make_double2(v[0], v[1]); }
};

template <typename T> struct PointArgs {
    cx<T>* F;                  // 2 x n: the plan's field, read (behind the linear step) and written (ahead of the next)
    T* P;                      // n: P of the start of the step that is being closed, then of the step that is being opened
    cx<T>* result;             // adaptive runs: 2 x n, where the last step is closed to (ManakovCtl::state)
    cx<T>* snap;               // fixed step: 2 x n, the field behind the closing half rotation alone goes here as well; nullptr: nowhere
    cx<T>* snaps;              // adaptive: the snapshot buffer, `snap_capacity` fields; step s goes to slot ceil(s / snap_every) - 1
    long long snap_every, snap_capacity;
    ManakovCtl* ctl;           // adaptive runs; nullptr: the step sizes are the arguments'
    long long n;               // samples per row, a multiple of 256
    T g;
    T hh_prev, hh_next;        // half the size of the step being closed / opened (0: there is none)
    int first;                 // 1: nothing is closed -- the run's first opening rotation: P is not read
    int rotate;                // 0: only max P of the field as it lies (the adaptive run's measuring pass)
    // ---- the Manakov-PMD line (k_manakov_point<T, true>): the unitary of the step being OPENED, applied behind the fused rotation
    int scatter;               // 0: none (pmd_scatter = False)
    T U[8];                    // fixed step: U[0][0], U[0][1], U[1][0], U[1][1] as (re, im)
    const T* quats;            // adaptive: (Re a, Im a, Re b, Im b) of U = [[a, b], [-conj b, conj a]] per step, indexed by ManakovCtl::steps
};

// exp(i phi) of W phases through the split-step kernels' own polynomial routines (rotate_all chooses by the largest phase of the thread: the phases of a
// step that resolves the nonlinearity take the short forms without an argument reduction)
template <typename T, int W> __device__ __forceinline__ void unit_rotations(const T (&phi)[W], cx<T> (&u)[W]) {
#pragma unroll
    for (int t = 0; t < W; ++t) u[t] = ssfm::mk<T>((T)1, (T)0);
    ssfm::rotate_all<W>(u, phi);
}

template <typename T, bool PMD>
__global__ __launch_bounds__(256) void k_manakov_point(PointArgs<T> a) {
    constexpr int W = Vec<T>::W;
    T hh_prev = a.hh_prev, hh_next = a.hh_next;
    cx<T>* dst = a.F;
    cx<T>* snap = a.snap;
    if (a.ctl) {
        const int state = a.ctl->state;
        if (state == 2 || (state == 1 && !a.rotate)) return;
        hh_prev = (T)0.5 * (T)a.ctl->h_prev;
        hh_next = (T)0.5 * (T)a.ctl->h;
        if (state == 1) { dst = a.result; hh_next = (T)0; }
        if (a.rotate && a.snaps && !a.first) {
            const long long s = a.ctl->steps, slot = (s + a.snap_every - 1) / a.snap_every - 1;
            if ((s % a.snap_every == 0 || state == 1) && slot >= 0 && slot < a.snap_capacity) snap = a.snaps + (size_t)slot * 2 * (size_t)a.n;
        }
    }
    // the unitary of the step that this pass opens; none on the measuring pass, on a closing pass alone (the run's last, state 1) and in the snapshots
    cx<T> u00, u01, u10, u11;
    bool scatter = false;
    if constexpr (PMD) {
        scatter = a.scatter != 0 && a.rotate != 0 && hh_next != (T)0;
        if (scatter && a.ctl) {
            const T* q = a.quats + 4 * (size_t)a.ctl->steps;
            u00 = ssfm::mk<T>(q[0], q[1]); u01 = ssfm::mk<T>(q[2], q[3]); u10 = ssfm::mk<T>(-q[2], q[3]); u11 = ssfm::mk<T>(q[0], -q[1]);
        } else {
            u00 = ssfm::mk<T>(a.U[0], a.U[1]); u01 = ssfm::mk<T>(a.U[2], a.U[3]); u10 = ssfm::mk<T>(a.U[4], a.U[5]); u11 = ssfm::mk<T>(a.U[6], a.U[7]);
        }
    }
    T pmax = (T)0;
    const long long units = a.n / W;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < units; i += (long long)gridDim.x * blockDim.x) {
        const long long at = i * W;
        cx<T> x0[W], x1[W];
        T po[W], pn[W];
        if (a.rotate && !a.first) Vec<T>::load_real(a.P + at, po);
        Vec<T>::load(a.F + at, x0);
        Vec<T>::load(a.F + a.n + at, x1);
#pragma unroll
        for (int t = 0; t < W; ++t) {
            pn[t] = (x0[t].x * x0[t].x + x0[t].y * x0[t].y) + (x1[t].x * x1[t].x + x1[t].y * x1[t].y);
            pmax = pn[t] > pmax ? pn[t] : pmax;
        }
        if (!a.rotate) continue;
        T phc[W], ph[W];
#pragma unroll
        for (int t = 0; t < W; ++t) {
            phc[t] = a.first ? (T)0 : hh_prev * (a.g * po[t]);
            ph[t] = hh_next != (T)0 ? phc[t] + hh_next * (a.g * pn[t]) : phc[t];
        }
        cx<T> u[W];
        unit_rotations<T, W>(ph, u);
        if (snap) {
            cx<T> s0[W], s1[W];
            if (hh_next != (T)0) {             // (the closing rotation alone; on the last step it IS the step's rotation: the same bits)
                cx<T> uc[W];
                unit_rotations<T, W>(phc, uc);
#pragma unroll
                for (int t = 0; t < W; ++t) { s0[t] = ssfm::cmul(x0[t], uc[t]); s1[t] = ssfm::cmul(x1[t], uc[t]); }
            } else {
#pragma unroll
                for (int t = 0; t < W; ++t) { s0[t] = ssfm::cmul(x0[t], u[t]); s1[t] = ssfm::cmul(x1[t], u[t]); }
            }
            Vec<T>::store(snap + at, s0);
            Vec<T>::store(snap + a.n + at, s1);
        }
#pragma unroll
        for (int t = 0; t < W; ++t) { x0[t] = ssfm::cmul(x0[t], u[t]); x1[t] = ssfm::cmul(x1[t], u[t]); }
        if constexpr (PMD) {
            if (scatter) {
#pragma unroll
                for (int t = 0; t < W; ++t) {
                    const cx<T> p00 = ssfm::cmul(u00, x0[t]), p01 = ssfm::cmul(u01, x1[t]), p10 = ssfm::cmul(u10, x0[t]), p11 = ssfm::cmul(u11, x1[t]);
                    x0[t] = ssfm::mk<T>(p00.x + p01.x, p00.y + p01.y);
                    x1[t] = ssfm::mk<T>(p10.x + p11.x, p10.y + p11.y);
                }
            }
        }
        Vec<T>::store(dst + at, x0);
        Vec<T>::store(dst + a.n + at, x1);
        if (hh_next != (T)0) Vec<T>::store_real(a.P + at, pn);
    }
    if (a.ctl && !a.rotate) {
        // max P: inside the wavefront, across the workgroup's four wavefronts through LDS, then ONE atomic per workgroup on the value's unsigned bits
        __shared__ T wmax[4];
        for (int o = 32; o > 0; o >>= 1) {
            const T other = __shfl_xor(pmax, o);
            pmax = other > pmax ? other : pmax;
        }
        if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = pmax;
        __syncthreads();
        if (threadIdx.x == 0) {
            T m = wmax[0];
            for (int w = 1; w < 4; ++w) m = wmax[w] > m ? wmax[w] : m;
            atomicMax(reinterpret_cast<typename Bits<T>::type*>(&a.ctl->maxbits), Bits<T>::of(m));
        }
    }
}

// The step rule in the plan's real type RT (chirpz.hip k_chirp_control with the hand-over of the last step, ManakovCtl::state):
//   h = phi_max / (|g| max P), clamped to L - z;  z += h.   first = 1: the size of step 0 from the input's maximum.
template <typename RT>
__global__ void k_manakov_control(ManakovCtl* __restrict__ ctl, double* __restrict__ zlog, double phi_max_d, double abs_g_d, double length_d, int max_steps, int first) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (ctl->state == 2) return;
    if (ctl->state == 1) { ctl->state = 2; return; }
    const RT phi_max = (RT)phi_max_d, abs_g = (RT)abs_g_d, L = (RT)length_d;
    const RT z = (RT)ctl->z;
    if (!first) {
        const int steps = ctl->steps + 1;
        ctl->steps = steps;
        zlog[steps] = (double)z;
        if (!(z < L) || steps >= max_steps) { ctl->state = 1; ctl->h_prev = ctl->h; ctl->h = 0.0; return; }
    } else zlog[0] = 0.0;
    const RT amax = Bits<RT>::back(ctl->maxbits);
    RT h = phi_max / (abs_g * amax);
    const RT left = (RT)(L - z);
    h = h < left ? h : left;
    ctl->h_prev = first ? 0.0 : ctl->h;
    ctl->h = (double)h;
    ctl->z = (double)(RT)(z + h);
    ctl->maxbits = 0ull;
}

// tab[i] = exp(D[i] h) / n, D~ in the order of the plan's transfer tables (element for element).  The products in T as the reference forms them
// (complex64 * float32), the transcendental functions in double and rounded once: the arithmetic of the plan's own tables (ssfm_kernels.hpp
// k_make_freq_table, mode 2).  ctl != nullptr: h is the device's.
template <typename T>
__global__ __launch_bounds__(256) void k_manakov_mktab(const cx<T>* __restrict__ D, cx<T>* __restrict__ tab, long long n, T h, T inv_n, const ManakovCtl* __restrict__ ctl) {
    if (ctl) { if (ctl->state != 0) return; h = (T)ctl->h; }
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const cx<T> d = D[i];
        const T xr = d.x * h, xi = d.y * h;
        const T e = (T)exp((double)xr);
        double s, c;
        sincos((double)xi, &s, &c);
        tab[i] = ssfm::mk<T>((e * (T)c) * inv_n, (e * (T)s) * inv_n);
    }
}

// The Manakov-PMD line's tables, one per row: tab[r n + i] = exp(D[i] h + s_r (-i/2) (w[i] tau)) / n, s_0 = +1 (row 0 is delayed by tau / 2), s_1 = -1; `w` =
// the angular frequencies [rad/ps] in the tables' order (real parts), tau = D_p sqrt(h) [ps].  k_manakov_mktab's arithmetic: every product and the sum of the
// two phases in T, one rounding each (no fused multiply-add: with tau = 0 the entries are the plain line's), the transcendental functions in double and
// rounded once.  ctl != nullptr: h is the device's and tau is formed from it, the square root correctly rounded in T.
template <typename T>
__global__ __launch_bounds__(256) void k_manakov_mktab_rows(const cx<T>* __restrict__ D, const cx<T>* __restrict__ w, cx<T>* __restrict__ tab, long long n, T h, T tau, T dp,
                                                            T inv_n, const ManakovCtl* __restrict__ ctl) {
#pragma clang fp contract(off)
    if (ctl) {
        if (ctl->state != 0) return;
        h = (T)ctl->h;
        tau = dp * (T)sqrt((double)h);             // (a float's root through the double's: 53 >= 2 * 24 + 2 bits, the second rounding is innocuous)
    }
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < 2 * n; i += (long long)gridDim.x * blockDim.x) {
        const long long j = i < n ? i : i - n;
        const cx<T> d = D[j];
        const T wt = w[j].x * tau;
        const T xr = d.x * h, xi = d.y * h + (i < n ? (T)-0.5 : (T)0.5) * wt;
        const T e = (T)exp((double)xr);
        double s, c;
        sincos((double)xi, &s, &c);
        tab[i] = ssfm::mk<T>((e * (T)c) * inv_n, (e * (T)s) * inv_n);
    }
}

// What ssfm_manakov_pmd_propagate adds to a run (host side)
struct PmdRun {
    double dp;                 // D_p [ps / sqrt(km)]
    const double* quats;       // nquats x 4, or nullptr: no scattering
    int64_t nquats;
    const double* w;           // n angular frequencies [rad/ps], natural order
};

template <typename T, bool PMD>
int manakov_run(ssfm_plan* plan, const ssfm::ManakovPlan& mp, double g_d, const double* hs, int64_t nsteps, double length, double phi_max, int64_t max_steps,
                void* snaps, int64_t snap_every, int64_t snap_capacity, int64_t chunk_arg, double* z_out, int64_t* steps_out, const PmdRun* pmd = nullptr) {
    const hipStream_t stream = static_cast<hipStream_t>(mp.stream);
    const long long n = mp.n;
    const T inv_n = (T)1 / (T)n;
    const size_t field_bytes = sizeof(cx<T>) * 2 * (size_t)n;
    T* P = nullptr;
    if (int rc = ssfm::plan_workspace(plan, 0, sizeof(T) * (size_t)n, reinterpret_cast<void**>(&P))) return rc;
    const unsigned g_point = grid_for(n / Vec<T>::W, 4096), g_tab = grid_for(PMD ? 2 * n : n, 4096);
    // the PMD line: its two tables of 2 n entries, w in the tables' order (staged through the first table's block), the adaptive run's quaternions
    cx<T>* rowtab[2] = {nullptr, nullptr};
    cx<T>* wperm = nullptr;
    T* quats_dev = nullptr;
    T dp = (T)0;
    if constexpr (PMD) {
        dp = (T)pmd->dp;
        for (int k = 0; k < 2; ++k)
            if (int rc = ssfm::plan_workspace(plan, 4 + k, field_bytes, reinterpret_cast<void**>(&rowtab[k]))) return rc;
        if (int rc = ssfm::plan_workspace(plan, 6, sizeof(cx<T>) * (size_t)n, reinterpret_cast<void**>(&wperm))) return rc;
        if (pmd->quats && !hs)
            if (int rc = ssfm::plan_workspace(plan, 7, sizeof(T) * 4 * (size_t)max_steps, reinterpret_cast<void**>(&quats_dev))) return rc;
        std::vector<cx<T>> wh((size_t)n);
        for (long long i = 0; i < n; ++i) { wh[(size_t)i].x = (T)pmd->w[i]; wh[(size_t)i].y = (T)0; }
        HIP_TRY(hipMemcpyAsync(rowtab[0], wh.data(), sizeof(cx<T>) * (size_t)n, hipMemcpyHostToDevice, stream));
        if (int rc = ssfm::plan_to_table_order(plan, rowtab[0], wperm)) return rc;
        if (quats_dev) {
            std::vector<T> qh(4 * (size_t)max_steps);
            for (size_t i = 0; i < qh.size(); ++i) qh[i] = (T)pmd->quats[i];
            HIP_TRY(hipMemcpyAsync(quats_dev, qh.data(), sizeof(T) * qh.size(), hipMemcpyHostToDevice, stream));
            HIP_TRY(hipStreamSynchronize(stream));           // (the staging vectors go out of scope)
        } else HIP_TRY(hipStreamSynchronize(stream));
    }
    PointArgs<T> pa;
    std::memset(&pa, 0, sizeof(pa));
    pa.F = static_cast<cx<T>*>(mp.F); pa.P = P; pa.n = n; pa.g = (T)g_d; pa.rotate = 1;
    pa.snap_every = snap_every; pa.snap_capacity = snap_capacity;
    int64_t launches = 0;
    auto mktab = [&](int slot, T h, const ManakovCtl* ctl) {
        if constexpr (PMD)
            hipLaunchKernelGGL(k_manakov_mktab_rows<T>, dim3(g_tab), dim3(256), 0, stream, static_cast<const cx<T>*>(mp.D), (const cx<T>*)wperm, rowtab[slot], n, h,
                               dp * std::sqrt(h), dp, inv_n, ctl);
        else
            hipLaunchKernelGGL(k_manakov_mktab<T>, dim3(g_tab), dim3(256), 0, stream, static_cast<const cx<T>*>(mp.D), static_cast<cx<T>*>(mp.tab[slot]), n, h, inv_n, ctl);
        ++launches;
    };
    auto point = [&](const PointArgs<T>& args) {
        hipLaunchKernelGGL((k_manakov_point<T, PMD>), dim3(g_point), dim3(256), 0, stream, args);
        ++launches;
    };
    // the linear step: x <- ifft(fft(x) table), one table for both rows or one per row
    auto linear = [&](int slot) -> int {
        if constexpr (PMD) return ssfm::plan_apply_row_tables(plan, rowtab[slot]);
        else return ssfm_apply_table(plan, slot);
    };
    if constexpr (PMD) { pa.scatter = pmd->quats ? 1 : 0; pa.quats = quats_dev; }

    if (hs) {
        // the at most two sizes of a fixed-h schedule (the body, the clamped last step) get a slot each, made once; a schedule of more sizes remakes the
        // slot that the step before did not use
        T slot_h[2] = {(T)0, (T)0};
        bool slot_set[2] = {false, false};
        int last_slot = 1;
        for (int64_t s = 0; s < nsteps; ++s) {
            const T h = (T)hs[s];
            int slot = -1;
            for (int k = 0; k < 2; ++k)
                if (slot_set[k] && std::memcmp(&slot_h[k], &h, sizeof(T)) == 0) slot = k;
            if (slot < 0) {
                slot = 1 - last_slot;
                mktab(slot, h, nullptr);
                slot_h[slot] = h; slot_set[slot] = true;
            }
            last_slot = slot;
            PointArgs<T> a = pa;
            a.first = s == 0 ? 1 : 0;
            a.hh_prev = s == 0 ? (T)0 : (T)0.5 * (T)hs[s - 1];
            a.hh_next = (T)0.5 * h;
            if (snaps && s > 0 && (s % snap_every == 0)) a.snap = static_cast<cx<T>*>(snaps) + (size_t)(s / snap_every - 1) * 2 * (size_t)n;
            if constexpr (PMD) {
                if (pmd->quats) {                                 // U_s = [[a, b], [-conj b, conj a]], cast to the plan's type
                    const double* q = pmd->quats + 4 * s;
                    const T ar = (T)q[0], ai = (T)q[1], br = (T)q[2], bi = (T)q[3];
                    const T U[8] = {ar, ai, br, bi, -br, bi, ar, -ai};
                    std::memcpy(a.U, U, sizeof(U));
                }
            }
            point(a);
            HIP_TRY(hipGetLastError());
            if (int rc = linear(slot)) return rc;
        }
        PointArgs<T> a = pa;                                      // the last step's closing half rotation
        a.hh_prev = (T)0.5 * (T)hs[nsteps - 1];
        a.hh_next = (T)0;
        if (snaps) a.snap = static_cast<cx<T>*>(snaps) + (size_t)((nsteps + snap_every - 1) / snap_every - 1) * 2 * (size_t)n;
        point(a);
        HIP_TRY(hipGetLastError());
        ssfm::plan_count_launches(plan, launches);
        if (steps_out) *steps_out = nsteps;
        return SSFM_OK;
    }

    ManakovCtl* ctl = nullptr;
    double* zlog = nullptr;
    cx<T>* result = nullptr;
    if (int rc = ssfm::plan_workspace(plan, 1, sizeof(ManakovCtl), reinterpret_cast<void**>(&ctl))) return rc;
    if (int rc = ssfm::plan_workspace(plan, 2, sizeof(double) * (size_t)(max_steps + 1), reinterpret_cast<void**>(&zlog))) return rc;
    if (int rc = ssfm::plan_workspace(plan, 3, field_bytes, reinterpret_cast<void**>(&result))) return rc;
    pa.ctl = ctl; pa.result = result; pa.snaps = static_cast<cx<T>*>(snaps);
    const double ag = g_d < 0 ? -g_d : g_d;
    auto control = [&](int first) {
        hipLaunchKernelGGL(k_manakov_control<T>, dim3(1), dim3(64), 0, stream, ctl, zlog, phi_max, ag, length, (int)max_steps, first);
        ++launches;
    };
    auto measure = [&]() { PointArgs<T> a = pa; a.rotate = 0; point(a); };
    ManakovCtl now;
    HIP_TRY(hipMemsetAsync(ctl, 0, sizeof(ManakovCtl), stream));
    measure();
    control(1);
    mktab(0, (T)0, ctl);
    { PointArgs<T> a = pa; a.first = 1; point(a); }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&now, ctl, sizeof(now), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    while (now.state == 0) {                      // (1: the chunk's last pass has closed the run's last step; 2: steps were queued behind it)
        // the caller's chunk, or: queue most of what remains, then look
        const int chunk = chunk_arg > 0 ? (int)(chunk_arg > 4096 ? 4096 : chunk_arg) : ssfm::chunk_estimate(length - (now.z - now.h), now.h, ssfm::kLineChunkMax, false);
        for (int i = 0; i < chunk; ++i) {
            if (int rc = linear(0)) return rc;
            measure();
            control(0);
            mktab(0, (T)0, ctl);
            point(pa);
        }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&now, ctl, sizeof(now), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
    }
    HIP_TRY(hipMemcpyAsync(mp.F, result, field_bytes, hipMemcpyDeviceToDevice, stream));
    if (z_out) HIP_TRY(hipMemcpyAsync(z_out, zlog, sizeof(double) * (size_t)(now.steps + 1), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    ssfm::plan_count_launches(plan, launches);
    if (steps_out) *steps_out = now.steps;
    return SSFM_OK;
}

// The checks of both entry points (every refusal comes before the first launch and leaves the field as it was), then the run.  pmd != nullptr: the PMD line.
int manakov_entry(const char* who, ssfm_plan* plan, double g, const double* hs, int64_t nsteps, double length, double phi_max, int64_t max_steps,
                  void* snaps, int64_t snap_every, int64_t snap_capacity, int64_t chunk, double* z_out, int64_t* steps_out, const PmdRun* pmd) {
    if (steps_out) *steps_out = 0;
    {
        int batch = 0, prec = 0;
        const int64_t n = ssfm::plan_length(plan, &batch, &prec);
        if (n <= 0) return fail(SSFM_ERR_INVALID, "null plan");
        if (batch != 2) return fail(SSFM_ERR_INVALID, "%s: a plan of two rows (the polarisations) is needed, this one has %d", who, batch);
        if (n % 256 != 0) return fail(SSFM_ERR_INVALID, "%s: %lld samples per row", who, (long long)n);
    }
    if (!std::isfinite(g)) return fail(SSFM_ERR_INVALID, "%s: g = %g", who, g);
    if (snaps && (snap_every < 1 || snap_capacity < 1)) return fail(SSFM_ERR_INVALID, "%s: snap_every = %lld, snap_capacity = %lld", who, (long long)snap_every, (long long)snap_capacity);
    if (!snaps) { snap_every = 1; snap_capacity = 0; }
    if (chunk < 0) return fail(SSFM_ERR_INVALID, "%s: chunk = %lld", who, (long long)chunk);
    if (hs) {
        if (nsteps < 0) return fail(SSFM_ERR_INVALID, "%s: nsteps = %lld", who, (long long)nsteps);
        for (int64_t s = 0; s < nsteps; ++s)
            if (!(hs[s] > 0) || !std::isfinite(hs[s])) return fail(SSFM_ERR_INVALID, "%s: step %lld is %g km (must be positive and finite)", who, (long long)s, hs[s]);
        if (snaps && (nsteps + snap_every - 1) / snap_every > snap_capacity)
            return fail(SSFM_ERR_INVALID, "%s: %lld steps, every %lld: more than %lld snapshots", who, (long long)nsteps, (long long)snap_every, (long long)snap_capacity);
    } else {
        if (max_steps < 1 || max_steps > (1ll << 30)) return fail(SSFM_ERR_INVALID, "%s: max_steps = %lld", who, (long long)max_steps);
        if (!(length > 0) || !std::isfinite(length) || !(phi_max > 0) || !std::isfinite(phi_max) || g == 0.0)
            return fail(SSFM_ERR_INVALID, "%s: an adaptive run needs length > 0, phi_max > 0 and g != 0 (length = %g, phi_max = %g, g = %g)", who, length, phi_max, g);
    }
    if (pmd) {
        if (!(pmd->dp >= 0) || !std::isfinite(pmd->dp)) return fail(SSFM_ERR_INVALID, "%s: dp = %g ps/sqrt(km) (must be finite and not negative)", who, pmd->dp);
        if (!pmd->w) return fail(SSFM_ERR_INVALID, "%s: NULL frequency grid", who);
        if (pmd->quats) {
            const int64_t need = hs ? nsteps : max_steps;
            if (pmd->nquats < need) return fail(SSFM_ERR_INVALID, "%s: %lld unitaries for %lld steps", who, (long long)pmd->nquats, (long long)need);
            for (int64_t i = 0; i < 4 * need; ++i)
                if (!std::isfinite(pmd->quats[i])) return fail(SSFM_ERR_INVALID, "%s: unitary %lld is not finite", who, (long long)(i / 4));
        }
    }
    if (hs && nsteps == 0) return SSFM_OK;
    ssfm::ManakovPlan mp;
    if (int rc = pmd ? ssfm::plan_manakov_pmd_begin(plan, &mp) : ssfm::plan_manakov_begin(plan, &mp)) return rc;
    const bool c64 = mp.precision == SSFM_C64;
    if (pmd) {
        if (c64) return manakov_run<float, true>(plan, mp, g, hs, nsteps, length, phi_max, max_steps, snaps, snap_every, snap_capacity, chunk, z_out, steps_out, pmd);
        return manakov_run<double, true>(plan, mp, g, hs, nsteps, length, phi_max, max_steps, snaps, snap_every, snap_capacity, chunk, z_out, steps_out, pmd);
    }
    if (c64) return manakov_run<float, false>(plan, mp, g, hs, nsteps, length, phi_max, max_steps, snaps, snap_every, snap_capacity, chunk, z_out, steps_out);
    return manakov_run<double, false>(plan, mp, g, hs, nsteps, length, phi_max, max_steps, snaps, snap_every, snap_capacity, chunk, z_out, steps_out);
}

}  // namespace

extern "C" int ssfm_manakov_propagate(ssfm_plan* plan, double g, const double* hs, int64_t nsteps, double length, double phi_max, int64_t max_steps,
                                      void* snaps, int64_t snap_every, int64_t snap_capacity, int64_t chunk, double* z_out, int64_t* steps_out) {
    return manakov_entry("ssfm_manakov_propagate", plan, g, hs, nsteps, length, phi_max, max_steps, snaps, snap_every, snap_capacity, chunk, z_out, steps_out, nullptr);
}

extern "C" int ssfm_manakov_pmd_propagate(ssfm_plan* plan, double g, const double* hs, int64_t nsteps, double length, double phi_max, int64_t max_steps,
                                          void* snaps, int64_t snap_every, int64_t snap_capacity, int64_t chunk, double* z_out, int64_t* steps_out,
                                          double dp, const double* quats, int64_t nquats, const double* w) {
    const PmdRun pmd = {dp, quats, quats ? nquats : 0, w};
    return manakov_entry("ssfm_manakov_pmd_propagate", plan, g, hs, nsteps, length, phi_max, max_steps, snaps, snap_every, snap_capacity, chunk, z_out, steps_out, &pmd);
}
