// ssfm_host.hip -- host side of the C ABI declared in include/ssfm_amd.h: plan, buffers,
// operator tables, launch sequences.  Pure HIP runtime; no torch types anywhere.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <memory>
#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <atomic>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "ssfm_amd.h"
#include "ssfm_common.hpp"
#include "ssfm_kernels.hpp"
#include "ssfm_lanes.hpp"
#include "ssfm_capture.hpp"
#include "ssfm_launch.hpp"
#include "ssfm_medium.hpp"
#include "ssfm_owned.hpp"
#include "ssfm_route.hpp"
#include "ssfm_schedule.hpp"
#include "ssfm_split.hpp"

using namespace ssfm;

namespace {

constexpr int kLog2Min = 8, kLog2Max = 24;      // (above 2^22: split plans, ssfm_split.hpp)
// (kLog2MaxDirect, cols_per_tile, kMaxTables and the other shape rules: ssfm_route.hpp)

// rows per k_freq workgroup: at least 64 threads where the row count allows (N1 >= 16 rows per batch entry)
constexpr int freq_rows(int n2, int e) { return (n2 / e) >= 64 ? 1 : ((64 * e / n2) > 16 ? 16 : (64 * e / n2)); }

// ----------------------------------------------------------------------------- launchers
// E = points per thread: 16 (default) or 8 (twice the waves, half the registers, one more LDS exchange).
template <typename T, int MODE, int N1, int E>
hipError_t launch_time_n1(dim3 grid, hipStream_t s, const TimeArgs<T>& a) {
    constexpr int C = cols_per_tile<T>();
    constexpr bool U16 = u16_layout<T>(N1, C, E);          // the field layout between the kernels (ssfm_kernels.hpp "U16")
    if constexpr (!U16 && MODE > TM_END && MODE != TM_MID_A && MODE != TM_MID_L) return hipErrorInvalidValue;      // (tile-private time-domain modes: U16 plans only)
    else if constexpr (U16 && MODE == TM_MID_L) return hipErrorInvalidValue;                    // (as a launch of its own: plans in the plain layout)
    else if constexpr (MODE == TM_MID_A && N1 != 128 && N1 != 256) return hipErrorInvalidValue;   // (the fused adaptive kernel: plans of 2^14 ... 2^18 samples)
    else {
    constexpr size_t lds = col_pass_lds<T>(N1, C, E);
    if constexpr (MODE == TM_BEGIN || MODE == TM_MID || MODE == TM_END) {
        if (a.scal != nullptr)               // a capture run with the scalar log: the instantiation that keeps it (ssfm_kernels.hpp time_body, LOG)
            return launch_kernel<k_time<T, N1, C, E, MODE, U16, true>, lds>(grid, dim3(N1 * C / E), s, SSFM_TIME_KERNEL_ARGS(a));
    }
    return launch_kernel<k_time<T, N1, C, E, MODE, U16>, lds>(grid, dim3(N1 * C / E), s, SSFM_TIME_KERNEL_ARGS(a));
    }
}
template <typename T, int MODE, int E>
hipError_t launch_time_e(int N1, int batch, hipStream_t s, const TimeArgs<T>& a) {
    const dim3 grid((unsigned)(a.N2 / cols_per_tile<T>()) * batch);
    switch (N1) {
        case 16:  return launch_time_n1<T, MODE, 16, E>(grid, s, a);
        case 32:  return launch_time_n1<T, MODE, 32, E>(grid, s, a);
        case 64:  return launch_time_n1<T, MODE, 64, E>(grid, s, a);
        case 128: return launch_time_n1<T, MODE, 128, E>(grid, s, a);
        case 256: return launch_time_n1<T, MODE, 256, E>(grid, s, a);
        case 512: if constexpr (E == 16) return launch_time_n1<T, MODE, 512, E>(grid, s, a); else break;
    }
    return hipErrorInvalidValue;
}
template <typename T, int MODE>
hipError_t launch_time(int N1, int batch, hipStream_t s, TimeArgs<T> a, int E) {
    a.rows = batch;
    return E == 8 ? launch_time_e<T, MODE, 8>(N1, batch, s, a) : launch_time_e<T, MODE, 16>(N1, batch, s, a);
}

template <typename T, int MODE, int N2, int E, bool U16>
hipError_t launch_freq_u(int nrows, hipStream_t s, const FreqArgs<T>& a) {
    constexpr int ROWS = freq_rows(N2, E);
    constexpr size_t lds = row_pass_lds<T>(N2, E, ROWS);
    if constexpr (MODE == FM_FWD_ONLY || MODE == FM_INV_ONLY)
        return launch_kernel<k_freq_half<T, N2, ROWS, E, MODE, U16>, lds>(dim3(nrows / ROWS), dim3(ROWS * N2 / E), s, SSFM_FREQ_KERNEL_ARGS(a));
    else
        return launch_kernel<k_freq<T, N2, ROWS, E, MODE, U16>, lds>(dim3(nrows / ROWS), dim3(ROWS * N2 / E), s, SSFM_FREQ_KERNEL_ARGS(a));
}
template <typename T, int MODE, int N2, int E>
hipError_t launch_freq_n2(int nrows, hipStream_t s, const FreqArgs<T>& a) {
    // the layout is the plan's (it follows from k_time's tile shape); complex128 plans never use it, and the
    // forward-only transform writes the plain transposed spectrum for its consumers
    if constexpr (sizeof(T) == 4)
        if (a.u16) return launch_freq_u<T, MODE, N2, E, true>(nrows, s, a);
    if constexpr ((MODE == FM_PHASE && sizeof(T) == 4) || MODE == FM_FLY_IM) return hipErrorInvalidValue;      // (complex64 phase / imaginary-part tables: plans in the unit layout only)
    else return launch_freq_u<T, MODE, N2, E, false>(nrows, s, a);
}
template <typename T, int MODE, int E>
hipError_t launch_freq_e(int N2, int nrows, hipStream_t s, const FreqArgs<T>& a) {
    if constexpr (MODE == FM_INV_ONLY) {          // (the inverse half of a split plan's row pass: its sub-sequences are 2^20 ... 2^22 samples long)
        switch (N2) {
            case 4096: return launch_freq_n2<T, MODE, 4096, E>(nrows, s, a);
            case 8192: if constexpr (E == 16) return launch_freq_n2<T, MODE, 8192, E>(nrows, s, a); else break;
        }
        return hipErrorInvalidValue;
    } else
    switch (N2) {
        case 16:   return launch_freq_n2<T, MODE, 16, E>(nrows, s, a);
        case 32:   return launch_freq_n2<T, MODE, 32, E>(nrows, s, a);
        case 64:   return launch_freq_n2<T, MODE, 64, E>(nrows, s, a);
        case 128:  return launch_freq_n2<T, MODE, 128, E>(nrows, s, a);
        case 256:  return launch_freq_n2<T, MODE, 256, E>(nrows, s, a);
        case 512:  return launch_freq_n2<T, MODE, 512, E>(nrows, s, a);
        case 1024: return launch_freq_n2<T, MODE, 1024, E>(nrows, s, a);
        case 2048: return launch_freq_n2<T, MODE, 2048, E>(nrows, s, a);
        case 4096: return launch_freq_n2<T, MODE, 4096, E>(nrows, s, a);
        case 8192: if constexpr (E == 16) return launch_freq_n2<T, MODE, 8192, E>(nrows, s, a); else break;
    }
    return hipErrorInvalidValue;
}
template <typename T, int MODE>
hipError_t launch_freq(int N2, int nrows, hipStream_t s, FreqArgs<T> a, int E) {
    a.rows = nrows / a.N1;
    return E == 8 ? launch_freq_e<T, MODE, 8>(N2, nrows, s, a) : launch_freq_e<T, MODE, 16>(N2, nrows, s, a);
}

// The passes of a chirp-z line whose field is stored as complex64 on a complex128 plan (ssfm_kernels.hpp time_body / freq_body, H): the shapes such plans have
// from 2^18 points up -- 256 column points x 8 per thread, 512 x 16; rows of 1024 ... 8192 points x 16 per thread.
template <int MODE, int N1, int E>
hipError_t launch_time_h_n1(dim3 grid, hipStream_t s, const TimeArgs<double>& a) {
    constexpr int C = cols_per_tile<double>();
    return launch_kernel<k_time_h<double, N1, C, E, MODE>, col_pass_lds<double>(N1, C, E)>(grid, dim3(N1 * C / E), s, SSFM_TIME_KERNEL_ARGS(a));
}
template <int MODE>
hipError_t launch_time_h(int N1, int batch, hipStream_t s, TimeArgs<double> a, int E) {
    a.rows = batch;
    const dim3 grid((unsigned)(a.N2 / cols_per_tile<double>()) * batch);
    if (N1 == 256 && E == 8) return launch_time_h_n1<MODE, 256, 8>(grid, s, a);
    if (N1 == 512 && E == 16) return launch_time_h_n1<MODE, 512, 16>(grid, s, a);
    return hipErrorInvalidValue;
}
template <int N2>
hipError_t launch_freq_h_n2(int nrows, hipStream_t s, const FreqArgs<double>& a, const int* done) {
    constexpr int E = 16, ROWS = freq_rows(N2, E);
    constexpr auto kernel = &k_freq_h<double, N2, ROWS, E, FM_TABLE>;
    constexpr size_t lds = row_pass_lds<double>(N2, E, ROWS);
    const dim3 grid(nrows / ROWS), block(ROWS * N2 / E);
#if SSFM_TRACE
    return launch_kernel<kernel, lds>(grid, block, s, a.F, a.tab, a.tw2, a.st, a.h, a.amp, a.inv_n, a.step, a.N1, a.rows, a.u16, done, a.trace, a.trace_slot);
#else
    return launch_kernel<kernel, lds>(grid, block, s, a.F, a.tab, a.tw2, a.st, a.h, a.amp, a.inv_n, a.step, a.N1, a.rows, a.u16, done);
#endif
}
inline hipError_t launch_freq_h(int N2, int nrows, hipStream_t s, FreqArgs<double> a, const int* done = nullptr) {
    a.rows = nrows / a.N1;
    switch (N2) {
        case 1024: return launch_freq_h_n2<1024>(nrows, s, a, done);
        case 2048: return launch_freq_h_n2<2048>(nrows, s, a, done);
        case 4096: return launch_freq_h_n2<4096>(nrows, s, a, done);
        case 8192: return launch_freq_h_n2<8192>(nrows, s, a, done);
    }
    return hipErrorInvalidValue;
}

template <typename T, int MODE, int R>
hipError_t launch_split_mid_r(hipStream_t s, const SplitArgs<T>& a) {
    constexpr int V = split_positions<T, R>();
    const long long units = (long long)a.N1 * a.N2 / V;
    hipLaunchKernelGGL((k_split_mid<T, R, MODE>), dim3((unsigned)((units + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}
template <typename T, int MODE>
hipError_t launch_split_mid(int R, hipStream_t s, const SplitArgs<T>& a) {
    switch (R) {
        case 2:  return launch_split_mid_r<T, MODE, 2>(s, a);
        case 4:  return launch_split_mid_r<T, MODE, 4>(s, a);
        case 8:  return launch_split_mid_r<T, MODE, 8>(s, a);
        case 16: return launch_split_mid_r<T, MODE, 16>(s, a);
    }
    return hipErrorInvalidValue;
}
template <typename T, bool TO_SUB>
hipError_t launch_split_shuffle(int R, hipStream_t s, cx<T>* sub, cx<T>* nat, long long M, int rows) {
    const dim3 grid((unsigned)((M * rows + 255) / 256));
    switch (R) {
        case 2:  hipLaunchKernelGGL((k_split_shuffle<T, 2, TO_SUB>), grid, dim3(256), 0, s, sub, nat, M, rows); break;
        case 4:  hipLaunchKernelGGL((k_split_shuffle<T, 4, TO_SUB>), grid, dim3(256), 0, s, sub, nat, M, rows); break;
        case 8:  hipLaunchKernelGGL((k_split_shuffle<T, 8, TO_SUB>), grid, dim3(256), 0, s, sub, nat, M, rows); break;
        case 16: hipLaunchKernelGGL((k_split_shuffle<T, 16, TO_SUB>), grid, dim3(256), 0, s, sub, nat, M, rows); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// k_small: one workgroup per row, the whole schedule in one launch (its sizes and points per thread: ssfm_route.hpp small_supported / small_points)
static_assert(kSmallTabs == kMaxTables, "k_small takes one table per cached step size");
// The line lengths of the one-workgroup engines, 256 ... MAXN: f(std::integral_constant<int, n>) for the one that n is
template <int MAXN, typename F>
hipError_t small_size(int n, F&& f) {
    switch (n) {
        case 256:  return f(std::integral_constant<int, 256>());
        case 512:  return f(std::integral_constant<int, 512>());
        case 1024: return f(std::integral_constant<int, 1024>());
        case 2048: return f(std::integral_constant<int, 2048>());
        case 4096: return f(std::integral_constant<int, 4096>());
        case 8192: if constexpr (MAXN >= 8192) return f(std::integral_constant<int, 8192>()); else break;      // (complex64 k_small only)
    }
    return hipErrorInvalidValue;
}
template <typename T>
hipError_t launch_small(int n, int rows, hipStream_t s, const SmallArgs<T>& a) {
    return small_size<(sizeof(T) == 4 ? 8192 : 4096)>(n, [&](auto size) {
        constexpr int N = decltype(size)::value, E = small_points<T>(N);
        return launch_kernel<k_small<T, N, E>, row_pass_lds<T>(N, E, 1)>(dim3(rows), dim3(N / E), s, a);
    });
}

// ---- kernels around k_medium_chirp (chirp_medium below): a complex64 line, the chirp's phase reduced exactly in integers as in chirpz.hip
template <typename T> __device__ __forceinline__ cx<T> cm_chirp_value(long long m, long long n, int conj) {
    const long long r = (m * m) % (2 * n);
    double sn, cs;
    sincospi(-(double)r / (double)n, &sn, &cs);
    return mk<T>((T)cs, (T)(conj ? -sn : sn));
}
// row 0 of the field <- the convolution kernel of Bluestein's identity wrapped around the line: conj(c_m) (which = 0) or c_m (1) at m and M - m, m < n
template <typename T> __global__ __launch_bounds__(256) void k_cm_kernel_line(cx<T>* __restrict__ F, long long n, long long M, int which) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < M; i += (long long)gridDim.x * blockDim.x) {
        const long long m = i < n ? i : (M - i < n ? M - i : -1);
        F[i] = m < 0 ? mk<T>((T)0, (T)0) : cm_chirp_value<T>(m, n, which == 0);
    }
}
// out[m] = exp(D~_m h) / n below n, zero above: the products in T as the reference forms them (complex64 * float32, devices.py:1179), the
// transcendental functions in double and rounded once (as k_make_freq_table)
template <typename T> __global__ __launch_bounds__(256) void k_cm_mul_table(const cx<T>* __restrict__ Dt, cx<T>* __restrict__ out, long long n, long long M, T h, T inv) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < M; i += (long long)gridDim.x * blockDim.x) {
        cx<T> d = mk<T>((T)0, (T)0);
        if (i < n) {
            const cx<T> x = Dt[i];
            const T xr = x.x * h, xi = x.y * h;
            const T e = (T)exp((double)xr);
            double sn, cs;
            sincos((double)xi, &sn, &cs);
            d = mk<T>((e * (T)cs) * inv, (e * (T)sn) * inv);
        }
        out[i] = d;
    }
}
__global__ __launch_bounds__(256) void k_cm_narrow(const cx<double>* __restrict__ src, cx<float>* __restrict__ dst, long long M, int conj) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < M; i += (long long)gridDim.x * blockDim.x)
        dst[i] = mk<float>((float)src[i].x, (float)(conj ? -src[i].y : src[i].y));
}
template <typename T> __global__ __launch_bounds__(256) void k_cm_pre(const cx<T>* __restrict__ A, const cx<T>* __restrict__ chirp, cx<T>* __restrict__ F, long long n, long long M, int batch) {
    const long long total = M * batch;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long r = i / M, m = i - r * M;
        F[i] = m < n ? cmul(A[r * n + m], chirp[m]) : mk<T>((T)0, (T)0);
    }
}
// A <- line conj(c); nothing when the run's workgroups did not meet (*error != 0): the caller's field is then as it was
template <typename T> __global__ __launch_bounds__(256) void k_cm_post(cx<T>* __restrict__ A, const cx<T>* __restrict__ chirp, const cx<T>* __restrict__ F, long long n, long long M, int batch,
                                                                      const unsigned* __restrict__ error) {
    if (*error != 0u) return;
    const long long total = n * batch;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long r = i / n, m = i - r * n;
        A[i] = cmulc(F[r * M + m], chirp[m]);
    }
}

// k_small_chirp: lengths that are not powers of two on one line of the plan's length (complex128), the whole schedule in one launch
// Points per thread: as k_small.  With 8 points on 512 threads the kernels of the 4096-point line spill (320 bytes of scratch per lane: a workgroup
// of 512 threads has 256 registers per thread); with 16 points on 256 threads (measured in round 4) they do not (256 + 120 accumulation registers),
// but four wavefronts per workgroup hide less: fixed step 12.6 us per step at n = 2032 either way, adaptive 23.3 against 16.7 (eight exp(D~ h) per
// thread and step instead of four).  So 8.
template <typename T> constexpr int chirp_points(int n) { return small_points<T>(n); }
template <typename T>
hipError_t launch_small_chirp(int n, int rows, hipStream_t s, const SmallChirpArgs<T>& a) {
    return small_size<4096>(n, [&](auto size) {
        constexpr int N = decltype(size)::value, E = chirp_points<T>(N);
        constexpr size_t lds = row_pass_lds<T>(N, E, 1, N);
        static_assert(lds <= 160 * 1024, "k_small_chirp: the line, its twiddles and H must fit the LDS");
        return launch_kernel<k_small_chirp<T, N, E>, lds>(dim3(rows), dim3(N / E), s, a);
    });
}
template <typename T>
hipError_t launch_small_chirp_adapt(int n, int rows, hipStream_t s, const SmallChirpAdaptArgs<T>& a) {
    return small_size<4096>(n, [&](auto size) {
        constexpr int N = decltype(size)::value, E = chirp_points<T>(N);
        constexpr size_t lds = row_pass_lds<T>(N, E, 1, N);
        static_assert(lds + 256 <= 160 * 1024, "k_small_chirp_adapt: the line, its twiddles and H must fit the LDS");
        return launch_kernel<k_small_chirp_adapt<T, N, E>, lds>(dim3(rows), dim3(N / E), s, a);
    });
}

// k_small_adapt: all rows of the plan in ONE workgroup (they share the step size); at most 512 threads, so that a thread
// may use the whole register file
template <typename T, int N, int ROWS>
hipError_t launch_small_adapt_nr(hipStream_t s, const SmallAdaptArgs<T>& a) {
    constexpr int E = small_points<T>(N);
    if constexpr (ROWS * N / E <= 512) return launch_kernel<k_small_adapt<T, N, E, ROWS>, row_pass_lds<T>(N, E, ROWS)>(dim3(1), dim3(ROWS * N / E), s, a);
    else return hipErrorInvalidValue;
}
template <typename T>
hipError_t launch_small_adapt(int n, int rows, hipStream_t s, const SmallAdaptArgs<T>& a) {
    return small_size<4096>(n, [&](auto size) {
        constexpr int N = decltype(size)::value;
        return rows == 1 ? launch_small_adapt_nr<T, N, 1>(s, a) : launch_small_adapt_nr<T, N, 2>(s, a);
    });
}

// A host thread that enqueues ONE lane's launches.  The host issues a launch per ~3.1 us, a 2^20 x 2 step is four launches per
// 17 us: one thread is 72 % busy with it and falls behind as soon as something slows it down -- in a process that has initialised
// RCCL a launch takes ~4.6 us and the run becomes host-bound (18.3 instead of 17.1 us per step, profiles/r03_host_enqueue.txt).
// With the lanes on threads of their own each thread issues two launches per step.
class LaneWorker {
  public:
    ~LaneWorker() { stop(); }
    void start(int device) {
        if (th_.joinable()) return;
        th_ = std::thread([this, device] {
            (void)hipSetDevice(device);
            std::unique_lock<std::mutex> lk(m_);
            for (;;) {
                cv_.wait(lk, [this] { return has_job_ || quit_; });
                if (!has_job_) return;                       // (quit_: a job handed over but not yet picked up still runs -- a capture run's transfers, a lane's launches)
                std::function<int()> job = std::move(job_);
                has_job_ = false;
                lk.unlock();
                const int rc = job();
                std::string err = rc != SSFM_OK ? std::string(ssfm::g_err) : std::string();
                lk.lock();
                rc_ = rc; err_ = std::move(err); done_ = true;
                cv_.notify_all();
            }
        });
    }
    void submit(std::function<int()> job) {
        std::lock_guard<std::mutex> lk(m_);
        job_ = std::move(job); has_job_ = true; done_ = false;
        cv_.notify_all();
    }
    int wait() {                      // the job's status; its error text becomes this thread's
        std::unique_lock<std::mutex> lk(m_);
        cv_.wait(lk, [this] { return done_; });
        if (rc_ != SSFM_OK) std::snprintf(ssfm::g_err, sizeof(ssfm::g_err), "%s", err_.c_str());
        return rc_;
    }
    void stop() {
        { std::lock_guard<std::mutex> lk(m_); quit_ = true; cv_.notify_all(); }
        if (th_.joinable()) th_.join();
    }
  private:
    std::thread th_;
    std::mutex m_;
    std::condition_variable cv_;
    std::function<int()> job_;
    bool has_job_ = false, done_ = false, quit_ = false;
    int rc_ = SSFM_OK;
    std::string err_;
};

// ----------------------------------------------------------------------------- do two streams share a hardware queue?
// The HIP runtime maps the streams of a priority class onto at most GPU_MAX_HW_QUEUES (4) hardware queues, and a stream created when the class's
// queues are all taken shares one -- possibly the one of the SAME plan's other lane (seen whenever 3 mod 4 other streams of the class were alive:
// profiles/r04_order_dependence.txt).  Kernels of one queue run in order: the plan's lanes would no longer overlap (35 instead of 21 us per step
// in round 1's measurement), and the round-3 engines whose lanes waited for each other inside a kernel stalled until their patience ran out.
// Probe: a kernel on stream a waits (at most `patience` ticks of the 100 MHz clock) for a word that a kernel on stream b sets.
__global__ void k_queue_probe_wait(unsigned* flag, unsigned* seen, long long patience) {
    const long long t0 = wall_clock64();
    unsigned v = 0u;
    while ((v = __hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) == 0u && wall_clock64() - t0 < patience) __builtin_amdgcn_s_sleep(8);
    *seen = v;
}
__global__ void k_queue_probe_set(unsigned* flag) { __hip_atomic_store(flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__global__ void k_queue_probe_spin(long long ticks) {            // a kernel that takes `ticks` of the 100 MHz clock, like a real one takes its microseconds
    const long long t0 = wall_clock64();
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(4);
}
// 1: b's kernel ran beside a's (queues of their own); 0: it did not within 0.2 ms (one queue -- or a GPU too busy to tell); < 0: HIP error
int streams_run_side_by_side(hipStream_t a, hipStream_t b, unsigned* words /* two device words */, hipEvent_t ev) {
    unsigned seen = 0u;
    if (hipMemsetAsync(words, 0, 2 * sizeof(unsigned), a) != hipSuccess) return -1;
    if (hipEventRecord(ev, a) != hipSuccess || hipStreamWaitEvent(b, ev, 0) != hipSuccess) return -1;
    hipLaunchKernelGGL(k_queue_probe_wait, dim3(1), dim3(1), 0, a, words, words + 1, 20000ll);
    // (a second kernel queued behind the waiting one, as every launch of a run has one, does not change the verdict: tried for the slow state that
    // lane_chain_us below is there for)
    hipLaunchKernelGGL(k_queue_probe_set, dim3(1), dim3(1), 0, b, words);
    if (hipGetLastError() != hipSuccess) return -1;
    if (hipMemcpyAsync(&seen, words + 1, sizeof(unsigned), hipMemcpyDeviceToHost, a) != hipSuccess) return -1;
    if (hipStreamSynchronize(a) != hipSuccess || hipStreamSynchronize(b) != hipSuccess) return -1;
    return seen != 0u ? 1 : 0;
}


// Rated lane pairs outlive their plan (round 6): rating a fresh pair costs ~7 ms of probe launches (k_queue_probe_spin was 25 % of an
// adaptive profile), and what the rating finds out -- which hardware queues the runtime gave the two streams -- is a property of the STREAMS, not of the plan.
// A two-lane plan that ends with good lanes hands its pair (the plan's stream and lane 1's) to a per-device pool instead of destroying it; the next two-lane
// plan of the process on that device takes a pooled pair with its rating and skips the probes.  The run-time check (lane_health) stays as it is.
struct LanePair { int device; hipStream_t main, lane; float score, alone_us, pair_us; };
struct LanePool {
    std::mutex m;
    std::vector<LanePair> free;
    static constexpr size_t kMax = 8;
    bool take(int device, LanePair* out) {
        std::lock_guard<std::mutex> lk(m);
        for (size_t i = free.size(); i-- > 0;)
            if (free[i].device == device) { *out = free[i]; free.erase(free.begin() + (long)i); return true; }
        return false;
    }
    bool give(const LanePair& p) {
        std::lock_guard<std::mutex> lk(m);
        if (free.size() >= kMax) return false;
        free.push_back(p);
        return true;
    }
};
LanePool& lane_pool() { static LanePool* p = new LanePool(); return *p; }        // (never destroyed: plans may be closed from atexit handlers)
std::atomic<long long> g_lane_ratings{0}, g_lane_pairs_reused{0};                  // process-wide: ratings made at plan creation / pairs taken from the pool

// ----------------------------------------------------------------------------- plan
struct PlanBase {
    int precision = 0;
    virtual ~PlanBase() {}
};

template <typename T> struct PlanT : PlanBase {
    int device = 0;
    int64_t n = 0;
    int batch = 0;
    int N1 = 0, N2 = 0;
    // Everything the plan holds is a member that frees itself (ssfm_owned.hpp); free_all() below is only what must happen in a certain ORDER before that.
    hipStream_t stream = nullptr;       // == lane_stream[0], which owns it
    Event ev0, ev1;
    // F / Y / P are what the launches read (targs / fargs): the plan's own buffers F_own / Y_own / P_own, except while measure_lanes points them at scratch fields
    cx<T>* F = nullptr;        // batch * n
    cx<T>* Y = nullptr;        // the field between the kernels: == F (plain layout, in place) or a buffer of its own (U16 layout: Y_own)
    T* P = nullptr;            // batch * n
    DeviceBuffer<cx<T>> F_own, Y_own;
    DeviceBuffer<T> P_own;
    DeviceBuffer<cx<T>> twN;      // n
    DeviceBuffer<cx<T>> twA;      // (N1/16)*N2: W_N^m
    DeviceBuffer<cx<T>> twB;      // 16*N2: W_N^(m*N1/16)
    DeviceBuffer<cx<T>> tw1;      // N1
    DeviceBuffer<cx<T>> tw2;      // N2
    DeviceBuffer<cx<T>> dnat;     // n  (D~ or H, natural order, staging)
    DeviceBuffer<cx<T>> dperm;    // n  (D~ transposed order)
    DeviceBuffer<cx<T>> dperm_fly;  // the same for the rows of k_freq<FM_FLY> where they use another number of points per thread (Ef_fly)
    DeviceBuffer<T> dimag_fly;      // a fibre's operator (flat real part) for k_freq<FM_FLY_IM>: the imaginary parts alone (complex64 plans in the unit layout, lazily)
    bool dimag_valid = false;
    DeviceBuffer<cx<T>> tw2_fly;
    DeviceBuffer<cx<T>> scratch;  // batch * n, lazily (ensure_scratch)
    DeviceBuffer<cx<T>> xfer_tab[2];   // resident transfer functions of ssfm_transfer_table (n each, lazily: ensure_xfer)
    struct Tab { T h = 0; DeviceBuffer<cx<T>> ptr; bool valid = false; int kind = 0; };      // kind 0: exp(D~ h)/N as complex numbers; 1: its phases (FM_PHASE)
    Tab tabs[kMaxTables];
    // Re D~ is the same number at every frequency (a fibre: -alpha/2, reference devices.py:1145): |exp(D~ h)| is a scalar and the
    // table may hold phases only.  Decided when the operator is set; env SSFM_PHASE_TABLE=0 keeps the complex tables.
    bool op_flat_re = false;
    T op_re0 = 0;
    bool phase_tables = true;
    bool force_fly = false;    // env SSFM_FORCE_FLY=1 (diagnostic): fixed-step runs form exp(D~ h) in the kernel as adaptive runs do
    int tab_rr = 0;
    // single-launch engine of small plans (ssfm_kernels.hpp k_small): its own row twiddles and operator tables (another order)
    bool small = false;        // env SSFM_SMALL=0 turns it off
    DeviceBuffer<cx<T>> tw_small;
    DeviceBuffer<cx<T>> tw_chirp; // stage twiddles of the line for the chirp-z kernels where they take other points per thread than k_small (made on first use)
    DeviceBuffer<cx<T>> dsmall;   // D~ in the one-line order (k_small_adapt)
    // single-launch engine of medium plans (ssfm_kernels.hpp k_medium): its barrier counters and error word in device memory, a pinned
    // host copy of the error word, and what a repeat of the run on the two-kernel engine needs
    bool medium_ok = true;     // env SSFM_MEDIUM=0, or a run whose barrier once ran out of patience, clears it
    static constexpr size_t kSet = kBarShards + kBarWords + 2;      // one launch's words in medium_st
    DeviceBuffer<unsigned long long> medium_st;    // two sets of: kBarShards counters, kBarWords flag words, the error word, the ticket counter (ensure_medium_state)
    PinnedBuffer<unsigned> medium_err_host;     // two words: a dual-polarisation plan of long rows runs its rows as two launches (run_medium)
    Stream medium_stream2;                      // ... the second one here, on another XCD
    Event medium_ev2;
    bool medium_pending = false;
    bool medium_split_ok = true;   // env SSFM_MEDIUM_SPLIT=0: a dual-polarisation plan's rows stay in one launch
    bool medium_adapt_ok = true;   // env SSFM_MEDIUM_ADAPT=0, or a run whose workgroups once did not all get to run, clears it
    int medium_xcc = -1, medium_xccs = 8;          // the XCD this plan's single-launch runs use, of so many
    std::vector<T> medium_sched;
    double medium_gamma = 0;
    long long medium_patience = 2000000ll;
    bool fused_ok = true;      // TM_MID_A may be used (env SSFM_ADAPT_FUSED=0, or a grid that once did not run as a whole, clears it)
    DeviceBuffer<cx<T>> fused_backup;   // the input of a fused adaptive run, for the fall-back (backup_field)
    Tab stabs[kMaxTables];
    int stab_rr = 0;
    DeviceBuffer<T> d_hs;      // the schedule on the device: step sizes, then one table index per step (upload_schedule)
    std::vector<unsigned char> h_sched;
    DeviceBuffer<AdaptState<T>> st;
    DeviceBuffer<T> zlog;      // (ensure_zlog)
    bool have_op = false;
    // ---- split plans (ssfm_split.hpp; round 6): rows of more than 2^22 samples.  `n` / `batch` / N1 / N2 below describe the SUB-SEQUENCES (n = M samples,
    // batch = rows x R of them) that every kernel of this file works on; `n_full` / `batch_full` are what the caller sees.  The caller's field lives in
    // `Fnat` in natural time order; F holds its sub-sequences x_a[m] = x[a + R m] while runs are in flight (`sub_valid` / `nat_valid`: which of the two
    // is current -- k_split_shuffle converts lazily, so back-to-back runs do not pay it).
    int split_R = 1;
    int64_t n_full = 0;
    int batch_full = 0;
    DeviceBuffer<cx<T>> Fnat;
    DeviceBuffer<double2> split_twA;   // W_N^(a k1), W_N^(a N1 k2) in double (one rounding of their product in k_split_mid)
    DeviceBuffer<double2> split_twB;
    DeviceBuffer<cx<T>> dsplit;        // D~ in the split order [p][k1][k2] (SM_FLY: adaptive runs, more step sizes than tables), lazily
    bool dsplit_valid = false;
    bool sub_valid = true, nat_valid = false;
    bool is_split() const { return split_R > 1; }
    int split_qf() const { return u16 ? N2 / Ef : 0; }          // the order of a sub-row between the row-pass halves: the plan's unit layout, or plain
    T inv_n_full() const { return (T)1 / (T)n_full; }
    // the sub-sequences are current in F (before a run)
    int ensure_sub() {
        if (!is_split() || sub_valid) return SSFM_OK;
        HIP_TRY((launch_split_shuffle<T, true>(split_R, stream, F, Fnat, (long long)n, batch_full)));
        sub_valid = true;
        return SSFM_OK;
    }
    // the natural-order field is current in Fnat (before the caller looks at it)
    int ensure_nat() {
        if (!is_split() || nat_valid) return SSFM_OK;
        HIP_TRY((launch_split_shuffle<T, false>(split_R, stream, F, Fnat, (long long)n, batch_full)));
        nat_valid = true;
        return SSFM_OK;
    }
    void ran() { if (is_split()) { sub_valid = true; nat_valid = false; } }      // a run has advanced F
    // ... and a caller that holds the field's address (ssfm_field_device_ptr / ssfm_stream: `external_order`) finds the natural-order field behind the run on
    // the plan's stream -- and may WRITE it there before the next run, which therefore starts from Fnat again
    int publish_if_external() {
        if (!is_split() || !external_order) return SSFM_OK;
        if (int rc = ensure_nat()) return rc;
        sub_valid = false;
        return SSFM_OK;
    }
    cx<T>* user_field() { return is_split() ? Fnat : F; }
    // the time-order field after a step -> `dst` (DEVICE): a z-resolved capture's snapshot
    hipError_t put_time_order(void* dst) {
        if (is_split()) return launch_split_shuffle<T, false>(split_R, stream, F, static_cast<cx<T>*>(dst), (long long)n, batch_full);
        return hipMemcpyAsync(dst, F, sizeof(cx<T>) * (size_t)n * batch, hipMemcpyDeviceToDevice, stream);
    }
    // the row pass of a split plan: forward row transforms, the pointwise middle (twiddles, radix-R butterfly across the sub-sequences, operator, back),
    // inverse row transforms.  `table`: exp(D~ h) / N in the split order (SM_TABLE), or nullptr: formed in the launch from D~ (SM_FLY; `s` != nullptr:
    // the step size is the device's)
    hipError_t split_freq(const cx<T>* table, T h, const AdaptState<T>* s, int step, int row0, int rows, hipStream_t st_, bool phase = false, T amp = (T)0) {
        FreqArgs<T> fa = fargs(nullptr, 0, s, row0, rows > 0 ? row0 / rows : 0);         // (`s`: launches behind the end of an adaptive run find `done` and leave)
        fa.step = step;
        if (u16) fa.u16 = 2;                 // (the unit layout between the two halves as well: 16-byte accesses on both sides of k_split_mid)
        hipError_t e = launch_freq<T, FM_FWD_ONLY>(N2, N1 * rows, st_, fa, Ef);
        if (e != hipSuccess) return e;
        SplitArgs<T> sa;
        sa.Y = Y + (size_t)row0 * n; sa.G = table ? table : dsplit; sa.twA = split_twA; sa.twB = split_twB; sa.st = s; sa.h = h; sa.inv_n = inv_n_full();
        sa.step = step; sa.N1 = N1; sa.N2 = N2; sa.rows_outer = rows / split_R; sa.Qf = split_qf();
        sa.amp = amp;
        if constexpr (sizeof(T) == 4) { if (table && phase) e = launch_split_mid<T, SM_PHASE>(split_R, st_, sa); else e = table ? launch_split_mid<T, SM_TABLE>(split_R, st_, sa) : launch_split_mid<T, SM_FLY>(split_R, st_, sa); }
        else e = table ? launch_split_mid<T, SM_TABLE>(split_R, st_, sa) : launch_split_mid<T, SM_FLY>(split_R, st_, sa);
        if (e != hipSuccess) return e;
        return launch_freq<T, FM_INV_ONLY>(N2, N1 * rows, st_, fa, Ef);
    }
    // D~ in the split order, for SM_FLY
    int split_fly_ready() {
        if (dsplit_valid) return SSFM_OK;
        HIP_TRY(dsplit.reserve(sizeof(cx<T>) * (size_t)n_full));
        hipLaunchKernelGGL((k_make_split_table<T, 0>), dim3((unsigned)((n_full + 255) / 256)), dim3(256), 0, stream, (const cx<T>*)dnat, dsplit, N1, N2, split_R, (T)0, inv_n_full(), split_qf());
        HIP_TRY(hipGetLastError());
        dsplit_valid = true;
        return SSFM_OK;
    }
    int no_split(const char* what) { return is_split() ? fail(SSFM_ERR_UNSUPPORTED, "%s: not for plans of more than 2^%d samples per row", what, kLog2MaxDirect) : (int)SSFM_OK; }
    // What the staging buffers hold is the PLAN's knowledge, not the caller's: tags[0] labels the linear operator in
    // dnat / dperm, tags[1 + slot] the resident transfer function of a slot.  A caller that has staged something
    // labels it (ssfm_plan_set_tag) and asks later whether it is still there (ssfm_plan_get_tag); every entry point
    // that overwrites or reuses a buffer clears its label here, so a stale label cannot survive.  0 = nothing known.
    uint64_t tags[3] = {0, 0, 0};
    void drop_operator() { have_op = false; tags[0] = 0; dimag_valid = false; dsplit_valid = false; for (auto& t : tabs) t.valid = false; for (auto& t : stabs) t.valid = false; }
    bool timed = false;
    std::atomic<int64_t> last_launches{0};
    // what the last run really did (ssfm_last_run_info): a single-launch engine that falls back is otherwise invisible to the caller
    int last_engine = SSFM_ENGINE_NONE;
    int last_fell_back = 0;
    int64_t fallbacks = 0;
    // ---- lane health (round 5; ssfm_lanes.hpp; rate_lane / lane_health / heal_lanes below measure and ask it)
    LaneHealth lanes;
    Event lane_e0, lane_e1;      // brackets of a rating measurement
    Event run_e0, run_e1;        // brackets of the last run that lane_health looks at (its own pair: ev0 / ev1 are re-recorded by every entry point)
    // ---- z-resolved capture that does not stall the loop (propagate_fixed_capture, round 5): a stream of its own for the transfers, a ring of plan-owned
    // device blocks of snapshots (laid out by ssfm_capture.hpp CapRing, filled by the capture steps' END launches, sent to the host by a helper thread -- cap_worker -- as they fill), the scalar log.
    // Nothing on the device waits across streams: a stream blocked on another stream's event slows every other queue's launches (see propagate_fixed_capture).
    Stream cap_stream;                                    // (ensure_cap_stream)
    std::vector<Event> cap_ev_ends[kMaxLanes];       // per lane and flush: the lane's END that filled the block
    Event cap_ev_in;                                      // on the plan's stream, ahead of the run: the input is in F
    DeviceBuffer<char> cap_blocks;                        // kCapBlocksMax blocks at most, cap_block_bytes each
    DeviceBuffer<char> cap_in;                            // plans whose engine works in place (Y == F): a copy of the input, taken ahead of the run
    size_t cap_block_bytes = 0;
    int cap_nblocks = 0;
    DeviceBuffer<double> cap_scal;                        // the wavefronts' pairs, then the reduced log
    LaneWorker cap_worker;                                // the helper thread of a capture run
    bool cap_pending = false;                             // a capture run's helper may still be at work: the next entry point (use_device) joins it
    // A caller that has asked for ssfm_stream() or ssfm_field_device_ptr() may order its own work behind a run without ssfm_synchronize(): for it a
    // run of the one-launch engine of medium plans is resolved (waited for, checked, repeated on the two-kernel engine if need be) before
    // ssfm_propagate_fixed returns
    bool external_order = false;
    // plan-owned device workspaces that grow on demand (ssfm_plan_workspace): what a driver loop outside this file (chirpz.hip) needs per call
    // without a hipMalloc / hipFree pair per call -- hipFree waits for the whole device and stalls the streams of every other plan
    DeviceBuffer<char> work[kWorkSlots];
    // A buffer that work queued on the plan's stream may still read grows like this everywhere: the stream is drained, then the old block is freed
    template <typename B> int grow(B& b, size_t bytes, size_t slack = 0) {
        if (b.capacity() >= bytes) return SSFM_OK;
        if (b.get()) HIP_TRY(hipStreamSynchronize(stream));
        HIP_TRY(b.reserve(bytes, slack));
        return SSFM_OK;
    }
    int workspace(int slot, size_t bytes, void** out) {
        if (slot < 0 || slot >= kWorkSlots || !out) return fail(SSFM_ERR_INVALID, "ssfm_plan_workspace: slot %d", slot);
        if (int rc = use_device()) return rc;
        if (int rc = grow(work[slot], bytes, bytes / 2 + 256)) return rc;
        *out = work[slot].get();
        return SSFM_OK;
    }
    // ---- what is made on first use, each in one place
    int ensure_scratch() { HIP_TRY(scratch.reserve(sizeof(cx<T>) * n * batch)); return SSFM_OK; }
    int ensure_xfer(int slot) { HIP_TRY(xfer_tab[slot].reserve(sizeof(cx<T>) * n)); return SSFM_OK; }
    int ensure_zlog(int64_t max_steps) { return grow(zlog, sizeof(T) * (size_t)(max_steps + 1)); }
    // the one-launch engines' barrier words (two sets: run_medium's second launch has its own) and the pinned copy of their error words
    int ensure_medium_state() {
        if (medium_st) return SSFM_OK;
        HIP_TRY(medium_st.reserve(sizeof(unsigned long long) * 2 * kSet));
        HIP_TRY(medium_err_host.reserve(2 * sizeof(unsigned)));
        medium_err_host[0] = medium_err_host[1] = 0u;
        return SSFM_OK;
    }
    // the field as it is now, kept for a run that may have to be repeated on another engine
    size_t field_bytes() const { return sizeof(cx<T>) * n * batch; }
    int backup_field() {
        const size_t fb = field_bytes();
        HIP_TRY(fused_backup.reserve(fb));
        HIP_TRY(hipMemcpyAsync(fused_backup, F, fb, hipMemcpyDeviceToDevice, stream));
        return SSFM_OK;
    }
    // a capture's copy stream: normal priority -- the plan's high-priority class keeps its queues for the lanes
    int ensure_cap_stream() {
        if (cap_stream) return SSFM_OK;
        HIP_TRY(hipStreamCreateWithFlags(cap_stream.out(), hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(cap_ev_in.out(), hipEventDisableTiming));
        return SSFM_OK;
    }
    // `hs | which` of a schedule -> d_hs, behind everything queued on the plan's stream; the table indices start `sizeof(T) * size()` bytes in (d_which)
    int upload_schedule(const Schedule<T>& sch) {
        const size_t hb = sizeof(T) * (size_t)sch.size(), need = hb + (size_t)sch.size();
        if (int rc = grow(d_hs, need, need / 2)) return rc;
        HIP_TRY(hipStreamSynchronize(stream));             // the staging vector may still feed the previous run's copy
        h_sched.resize(need);
        std::memcpy(h_sched.data(), sch.steps.data(), hb);
        std::memcpy(h_sched.data() + hb, sch.which.data(), (size_t)sch.size());
        HIP_TRY(hipMemcpyAsync(d_hs, h_sched.data(), need, hipMemcpyHostToDevice, stream));
        return SSFM_OK;
    }
    const unsigned char* d_which(const Schedule<T>& sch) const { return reinterpret_cast<const unsigned char*>(d_hs.get()) + sizeof(T) * (size_t)sch.size(); }
    LaneWorker lane_worker[8];        // (lane g > 0: a host thread of its own for its launches; env SSFM_LANE_THREADS=0: all from the caller's thread)
    bool lane_threads = true;
    bool profiling = false;
    // "lanes": rows are independent (they only share the adaptive step size), so a fixed-step run
    // drives disjoint row groups on separate streams; kernels of different groups overlap, which
    // hides launch gaps and lets one group compute while another waits for memory.
    int nlanes = 1;
    bool u16 = false;          // field layout between the kernels: 16-byte units (ssfm_kernels.hpp "U16")
    int E = 16;                // points per thread of k_time (env SSFM_E = 8 | 16)
    int Ef = 16;               // ... and of k_freq (env SSFM_EF); the two kernels only share the field layout
    int Ef_fly = 16;           // ... and of k_freq when it forms exp(D~ h) itself (adaptive runs, more step sizes than tables)
    Stream lane_stream[kMaxLanes];         // (lane 0's is the plan's `stream`)
    Event lane_ev[kMaxLanes];
    Event fork_ev;
    // per-lane pools of events (profiling).  mode 1: an event after every launch (per-class times, but
    // the marker packets slow a launch-dense run by ~30 %); mode 2: an event after every 64th launch
    // (negligible overhead; the interval is split between the classes by launch count); mode 3: after every
    // kSampleStride launches ONE launch of each class is bracketed by two events (3 extra markers per 16 launches: the
    // host keeps ahead of the GPU) -- kernel_times() then reports those single-launch intervals only.
    struct LaneProf {
        std::vector<Event> ev;
        std::vector<int> c0, c1;          // launches of class 0 / 1 between event i-1 and event i
        size_t n = 0;
        int pend0 = 0, pend1 = 0;
        int sampling = 0;                 // mode 3: launches of the current sample group still to be bracketed
    };
    LaneProf prof[8];
    int prof_mode = 0;
    int prof_mode_run = 0;            // the mode the recorded events were taken in
    static constexpr int kSparseStride = 64;
    static constexpr int kSampleStride = 14;

    int prof_record(LaneProf& p, int lane) {
        if (p.n == p.ev.size()) {
            Event e;
            HIP_TRY(hipEventCreate(e.out()));
            p.ev.push_back(std::move(e));
            p.c0.push_back(0);
            p.c1.push_back(0);
        }
        HIP_TRY(hipEventRecord(p.ev[p.n], lane_stream[lane]));
        p.c0[p.n] = p.pend0; p.c1[p.n] = p.pend1;
        p.pend0 = p.pend1 = 0;
        ++p.n;
        return SSFM_OK;
    }
    // cls < 0: opening event; cls 0/1: a launch of that class was just enqueued; cls 2: closing
    int prof_mark(int cls, int lane = 0) {
        if (!profiling) return SSFM_OK;
        LaneProf& p = prof[lane];
        if (cls < 0) { p.pend0 = p.pend1 = 0; p.sampling = 0; prof_mode_run = prof_mode; return prof_record(p, lane); }
        if (cls == 0) ++p.pend0;
        if (cls == 1) ++p.pend1;
        if (cls == 2) return (p.pend0 + p.pend1) ? prof_record(p, lane) : (int)SSFM_OK;
        if (prof_mode == 3) {
            if (p.sampling > 0) { --p.sampling; return prof_record(p, lane); }              // this interval holds exactly this launch
            if (p.pend0 + p.pend1 >= kSampleStride) { p.sampling = 2; return prof_record(p, lane); }
            return SSFM_OK;
        }
        if (prof_mode == 1 || p.pend0 + p.pend1 >= kSparseStride) return prof_record(p, lane);
        return SSFM_OK;
    }
    int kernel_times(int64_t counts[2], double total_ms[2]) {
        counts[0] = counts[1] = 0;
        total_ms[0] = total_ms[1] = 0.0;
        for (auto& p : prof) {
            if (p.n < 2) continue;
            HIP_TRY(hipEventSynchronize(p.ev[p.n - 1]));
            for (size_t i = 1; i < p.n; ++i) {
                const int tot = p.c0[i] + p.c1[i];
                if (tot == 0) continue;
                if (prof_mode_run == 3 && tot != 1) continue;          // sampled mode: the bracketed single launches only
                float ms = 0.f;
                HIP_TRY(hipEventElapsedTime(&ms, p.ev[i - 1], p.ev[i]));
                counts[0] += p.c0[i];
                counts[1] += p.c1[i];
                total_ms[0] += (double)ms * p.c0[i] / tot;
                total_ms[1] += (double)ms * p.c1[i] / tot;
            }
        }
        return SSFM_OK;
    }

    T inv_n() const { return (T)1 / (T)n; }

    // What has to happen in order before the members free themselves: the helper threads end, the streams drain, and a good pair of lane streams goes
    // to the pool with its rating (lane_pool above) instead of being destroyed.
    int free_all() {
        cap_worker.stop();                                  // (finishes a capture run's transfers first)
        for (auto& w : lane_worker) w.stop();
        if (stream) (void)hipStreamSynchronize(stream);
        if (cap_stream) (void)hipStreamSynchronize(cap_stream);
        if (lanes.pair_may_go_to_pool(nlanes) && stream && lane_stream[1] && lane_stream[1] != stream
            && !std::getenv("SSFM_LANE_POOL_OFF")) {
            (void)hipStreamSynchronize(lane_stream[1]);
            if (lane_pool().give(LanePair{device, stream, lane_stream[1], lanes.lane_score, lanes.lane_alone_us, lanes.lane_pair_us})) {
                (void)lane_stream[0].release(); (void)lane_stream[1].release();
            }
        }
        stream = nullptr;
        return SSFM_OK;
    }
    ~PlanT() override { free_all(); }

    // What plan_shape and the routes (ssfm_route.hpp) decided for this plan; n / batch / N1 / N2 / E / Ef / Ef_fly / u16 / nlanes / small / split_R are its copies
    PlanShape shape;
    static constexpr size_t cb = sizeof(cx<T>);
    static std::optional<int> env_int(const char* text) { return text ? std::optional<int>(std::atoi(text)) : std::nullopt; }
    int init(int dev, int64_t n_, int batch_) {
        n_full = n_; batch_full = batch_;
        const ShapeKnobs knobs = {env_int(std::getenv("SSFM_SPLIT_ABOVE")), env_int(std::getenv("SSFM_SPLIT_LOG2M")), env_int(std::getenv("SSFM_E")), env_int(std::getenv("SSFM_EF")),
                                  env_int(std::getenv("SSFM_EF_FLY")), env_int(std::getenv("SSFM_LANES")), env_int(std::getenv("SSFM_SMALL"))};
        shape = plan_shape<T>(n_, batch_, knobs);
        split_R = shape.split_R;
        if (shape.too_many) return fail(SSFM_ERR_INVALID, "batch=%d rows of 2^%d samples: too many sub-sequences", batch_, shape.log2_full);
        if (is_split()) { sub_valid = false; nat_valid = true; }
        device = dev; n = shape.n; batch = shape.batch;
        N1 = shape.N1; N2 = shape.N2; E = shape.E; Ef = shape.Ef; Ef_fly = shape.Ef_fly; u16 = shape.u16; nlanes = shape.nlanes; small = shape.small;
        HIP_TRY(hipSetDevice(device));
        if (int rc = make_streams()) return rc;
        if (int rc = make_tables()) return rc;
        if (is_split()) if (int rc = make_split_extras()) return rc;
        if (int rc = make_engine_extras()) return rc;
        if (nlanes > 1 && nlanes <= 4) return rate_lanes_at_creation();
        return SSFM_OK;
    }
    // the plan's streams (one per lane) and events
    int make_streams() {
        // All streams of a plan live in the HIGHEST priority class.  The lanes only overlap if their streams
        // sit on different hardware queues; the runtime multiplexes streams onto GPU_MAX_HW_QUEUES (default
        // 4) queues per priority class, and in a process that also holds RCCL's (normal-priority) streams
        // -- torch.distributed with backend nccl -- two normal-priority lanes landed on ONE queue: 35
        // instead of 21 us per step.  A priority class of their own gives the lanes queues of their own;
        // giving them the SAME priority keeps the arbitration between them fair (one high, one normal lane
        // starved the normal one: 26 instead of 16 us per field-step with 4 fields).
        int prio_lo = 0, prio_hi = 0;
        HIP_TRY(hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi));
        // a plan that will drive two lanes takes a rated pair of streams from the process's pool where there is one (lane_pool above)
        LanePair lp;
        if (shape.lanes_wanted == 2 && batch_full >= 2 && batch_full % 2 == 0 && !std::getenv("SSFM_LANE_POOL_OFF") && lane_pool().take(device, &lp)) {
            lane_stream[0].reset(lp.main); lane_stream[1].reset(lp.lane);
            lanes.took_pair(lp.score);
            ++g_lane_pairs_reused;
        }
        if (!lane_stream[0]) HIP_TRY(hipStreamCreateWithPriority(lane_stream[0].out(), hipStreamNonBlocking, prio_hi));
        stream = lane_stream[0];
        for (Event* e : {&ev0, &ev1}) HIP_TRY(hipEventCreate(e->out()));
        if (const char* e = std::getenv("SSFM_LANE_THREADS")) lane_threads = std::atoi(e) != 0;
        HIP_TRY(hipEventCreateWithFlags(fork_ev.out(), hipEventDisableTiming));
        for (int g = 1; g < nlanes; ++g) {
            if (!(lanes.lanes_from_pool && g == 1)) HIP_TRY(hipStreamCreateWithPriority(lane_stream[g].out(), hipStreamNonBlocking, prio_hi));
            HIP_TRY(hipEventCreateWithFlags(lane_ev[g].out(), hipEventDisableTiming));
        }
        lanes.streams_made(nlanes);
        return SSFM_OK;
    }
    // the fields, the twiddle tables of the two kernels and the operator's buffers
    int make_tables() {
        HIP_TRY(F_own.reserve(cb * n * batch));
        HIP_TRY(P_own.reserve(sizeof(T) * n * batch));
        F = F_own; P = P_own;
        Y = F;
        if (u16) { HIP_TRY(Y_own.reserve(cb * n * batch)); Y = Y_own; }
        // inter-pass twiddles W_N^(k1 n2): either the n-entry table in k_time's thread order, or (U16 plans) the two
        // small factor tables the kernel multiplies (ssfm_kernels.hpp twn_compute)
        if (u16 || sizeof(T) == 8) {
            const long long nA = (long long)(N1 / E) * N2, nB = (long long)E * N2;      // [tile][j][c], j < N1/E;  [tile][t][c], t < E
            HIP_TRY(twA.reserve(cb * nA));
            HIP_TRY(twB.reserve(cb * nB));
            const int C_ = cols_per_tile<T>();
            hipLaunchKernelGGL(k_make_tw_tiles<T>, dim3((unsigned)((nA + 255) / 256)), dim3(256), 0, stream, twA.get(), N1 / E, 1ll, N2, C_, (long long)n, (int)u16, N2 / Ef);
            hipLaunchKernelGGL(k_make_tw_tiles<T>, dim3((unsigned)((nB + 255) / 256)), dim3(256), 0, stream, twB.get(), E, (long long)(N1 / E), N2, C_, (long long)n, (int)u16, N2 / Ef);
        } else {
            HIP_TRY(twN.reserve(cb * n));
            hipLaunchKernelGGL(k_make_twN<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, twN.get(), N1, N2, cols_per_tile<T>(), E, (int)u16, N2 / Ef);
        }
        if (int rc = make_line_table(&tw1, N1, E)) return rc;
        if (int rc = make_line_table(&tw2, N2, Ef)) return rc;
        HIP_TRY(dnat.reserve(cb * n_full));
        HIP_TRY(dperm.reserve(cb * n));
        return SSFM_OK;
    }
    // a split plan: the caller's natural-order field and the twiddles of the third factor
    int make_split_extras() {
        HIP_TRY(Fnat.reserve(cb * n_full * batch_full));
        HIP_TRY(hipMemsetAsync(Fnat, 0, cb * n_full * batch_full, stream));
        HIP_TRY(split_twA.reserve(sizeof(double2) * (size_t)split_R * N1));
        HIP_TRY(split_twB.reserve(sizeof(double2) * (size_t)split_R * N2));
        const long long nt = (long long)split_R * (N1 + N2);
        hipLaunchKernelGGL(k_make_split_twiddles, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, stream, split_twA.get(), split_twB.get(), N1, N2, split_R);
        HIP_TRY(hipGetLastError());
        return SSFM_OK;
    }
    // what single engines need: the tables of rows that form exp(D~ h) themselves, the switches, the one-launch engines' XCD and tables, the step state
    int make_engine_extras() {
        if (Ef_fly != Ef) {
            if (int rc = make_line_table(&tw2_fly, N2, Ef_fly)) return rc;
            HIP_TRY(dperm_fly.reserve(cb * n));
        }
        if (const char* e = std::getenv("SSFM_ADAPT_FUSED")) fused_ok = std::atoi(e) != 0;
        if (const char* e = std::getenv("SSFM_MEDIUM")) medium_ok = std::atoi(e) != 0;
        if (const char* e = std::getenv("SSFM_MEDIUM_ADAPT")) medium_adapt_ok = std::atoi(e) != 0;
        if (const char* e = std::getenv("SSFM_MEDIUM_SPLIT")) medium_split_ok = std::atoi(e) != 0;
        if (const char* e = std::getenv("SSFM_FUSED_PATIENCE_TICKS")) medium_patience = std::atoll(e);
        if (const char* e = std::getenv("SSFM_PHASE_TABLE")) phase_tables = std::atoi(e) != 0;
        if (const char* e = std::getenv("SSFM_FORCE_FLY")) force_fly = std::atoi(e) != 0;
        // the XCD this plan's one-launch runs meet on: decided now (the probe launch behind xcc_mask runs once per device, on a stream of its own)
        if (sizeof(T) == 4 && medium_shape(N1, N2) && (medium_ok || medium_adapt_ok)) (void)pick_xcc();
        if (small) {
            if (int rc = make_line_table(&tw_small, (int)n, small_points<T>((int)n))) return rc;
            HIP_TRY(dsmall.reserve(cb * n));
        }
        HIP_TRY(st.reserve(sizeof(AdaptState<T>)));
        HIP_TRY(hipMemsetAsync(P, 0, sizeof(T) * n * batch, stream));
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(stream));
        return SSFM_OK;
    }
    // every lane on a hardware queue of its own, and one on which its kernels really run beside lane 0's (rate_lane): rated with the plan's own
    // kernels on its own buffers, which hold nothing yet -- zeros (a transform of zeros is zeros; D~ = 0 is the identity)
    int rate_lanes_at_creation() {
        for (Event* e : {&lane_e0, &lane_e1, &run_e0, &run_e1}) HIP_TRY(hipEventCreate(e->out()));
        HIP_TRY(hipMemsetAsync(F, 0, cb * n * batch, stream));
        if (Y != F) HIP_TRY(hipMemsetAsync(Y, 0, cb * n * batch, stream));
        HIP_TRY(hipMemsetAsync(dperm, 0, cb * n, stream));
        if (dperm_fly) HIP_TRY(hipMemsetAsync(dperm_fly, 0, cb * n, stream));
        bool replaced = false;
        if (!lanes.pair_counts_as_rated(nlanes)) {
            ++g_lane_ratings;
            if (int rc = rate_and_replace_lanes(F, Y, P, &replaced)) return rc;
        }
        lanes.created();
        HIP_TRY(hipStreamSynchronize(stream));
        return SSFM_OK;
    }

    // ---- lane health: what ssfm_lanes.hpp decides on is measured here
    // Launch period [us] of `steps` steps of the two-kernel engine (BEGIN, k_freq<FLY>, MID ... END) on the lanes of `mask`, on the buffers given (zeros).
    // The lanes' queues are held by a spin kernel while the host enqueues, so that the host's enqueue rate is not part of the figure.
    int measure_lanes(unsigned mask, int steps, cx<T>* Fx, cx<T>* Yx, T* Px, float* us) {
        cx<T>* F0 = F; cx<T>* Y0 = Y; T* P0 = P;
        F = Fx; Y = Yx; P = Px;
        const int rows = batch / nlanes;
        const T hh = (T)0.0625;
        auto body = [&]() -> int {
            hipLaunchKernelGGL(k_queue_probe_spin, dim3(1), dim3(1), 0, stream, lane_spin_ticks(steps, nlanes));
            HIP_TRY(hipEventRecord(fork_ev, stream));
            HIP_TRY(hipEventRecord(lane_e0, stream));
            for (int g = 1; g < nlanes; ++g)
                if (mask & (1u << g)) HIP_TRY(hipStreamWaitEvent(lane_stream[g], fork_ev, 0));
            for (int g = 0; g < nlanes; ++g)
                if (mask & (1u << g)) HIP_TRY((launch_time<T, TM_BEGIN>(N1, rows, lane_stream[g], targs((T)1, 0, hh, nullptr, g * rows, g), E)));
            for (int s_ = 0; s_ < steps; ++s_) {
                for (int g = 0; g < nlanes; ++g)
                    if (mask & (1u << g)) HIP_TRY((launch_freq<T, FM_FLY>(N2, N1 * rows, lane_stream[g], fargs_fly(2 * hh, nullptr, g * rows, g), Ef_fly)));
                for (int g = 0; g < nlanes; ++g) {
                    if (!(mask & (1u << g))) continue;
                    if (s_ + 1 < steps) HIP_TRY((launch_time<T, TM_MID>(N1, rows, lane_stream[g], targs((T)1, hh, hh, nullptr, g * rows, g), E)));
                    else HIP_TRY((launch_time<T, TM_END>(N1, rows, lane_stream[g], targs((T)1, hh, 0, nullptr, g * rows, g), E)));
                }
            }
            for (int g = 1; g < nlanes; ++g) {
                if (!(mask & (1u << g))) continue;
                HIP_TRY(hipEventRecord(lane_ev[g], lane_stream[g]));
                HIP_TRY(hipStreamWaitEvent(stream, lane_ev[g], 0));
            }
            HIP_TRY(hipEventRecord(lane_e1, stream));
            HIP_TRY(hipStreamSynchronize(stream));
            float ms = 0.f;
            HIP_TRY(hipEventElapsedTime(&ms, lane_e0, lane_e1));
            *us = ms * 1e3f / (float)(2 * steps + 1);
            return SSFM_OK;
        };
        const int rc = body();
        F = F0; Y = Y0; P = P0;
        return rc;
    }
    // One lane's rating (ssfm_lanes.hpp LaneRating) from the queue probe and four measurements; < 0: error (g_err set)
    int rate_lane(int g, cx<T>* Fx, cx<T>* Yx, T* Px, LaneRating* out) {
        int shared = 0;
        {
            DeviceBuffer<unsigned> words;
            if (words.reserve(2 * sizeof(unsigned)) != hipSuccess) { (void)hipGetLastError(); return -1; }
            for (int k = 0; k < g && !shared; ++k) {
                const int side = streams_run_side_by_side(lane_stream[k], lane_stream[g], words, fork_ev);
                if (side < 0) return -1;
                shared = side == 0;
            }
        }
        float alone[2] = {0.f, 0.f}, pair[2] = {0.f, 0.f};
        const int probe_steps = lane_probe_steps(big_rows());
        for (int r = 0; r < 2 && !shared; ++r) {
            if (measure_lanes(1u, probe_steps, Fx, Yx, Px, &alone[r]) != SSFM_OK) return -1;
            if (measure_lanes(1u | (1u << g), probe_steps, Fx, Yx, Px, &pair[r]) != SSFM_OK) return -1;
        }
        *out = ssfm::rate_lane(shared != 0, alone, pair, big_rows(), lanes.lane_fault);
#ifdef SSFM_LANE_PROBE_DEBUG
        if (!shared) std::fprintf(stderr, "lane rating: lane %d: %.2f us per launch alone, %.2f with lane 0 beside it\n", g, out->alone_us, out->pair_us);
#endif
        return 0;
    }
    bool big_rows() const { return (size_t)n * sizeof(cx<T>) >= ((size_t)32 << 20); }
    // Rate every lane beyond the first; a lane that is not good tries replacement streams four at a time -- made together, so that the runtime's
    // least-used rule spreads them over the class's hardware queues -- the first good one (else the best one) replaces the lane's stream, the rest go.
    int rate_and_replace_lanes(cx<T>* Fx, cx<T>* Yx, T* Px, bool* replaced) {
        int prio_lo = 0, prio_hi = 0;
        HIP_TRY(hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi));
        *replaced = false;
        bool all_good = true;
        for (int g = 1; g < nlanes; ++g) {
            LaneRating have;
            if (rate_lane(g, Fx, Yx, Px, &have) < 0) return fail(SSFM_ERR_HIP, "lane rating failed: %s", hipGetErrorString(hipGetLastError()));
            for (int round = 0; round < 2 && have.state > 0; ++round) {
                Stream cand[4];                  // (those that do not replace the lane's stream go when the round is over)
                for (auto& c : cand)
                    if (hipStreamCreateWithPriority(c.out(), hipStreamNonBlocking, prio_hi) != hipSuccess) { (void)hipGetLastError(); c.reset(); }
                for (auto& c : cand) {
                    if (!c || have.state == 0) continue;
                    LaneRating rc_;
                    std::swap(c, lane_stream[g]);                       // (rated in the lane's place; swapped back unless it is better)
                    if (rate_lane(g, Fx, Yx, Px, &rc_) >= 0 && lane_rating_better(rc_, have)) { have = rc_; *replaced = true; }
                    else std::swap(c, lane_stream[g]);
                }
            }
            lanes.fold_lane(g, have, &all_good);
        }
        lanes.fold_end(all_good);
        return SSFM_OK;
    }
    // After a two-lane run of >= 64 steps: was it as fast as this plan's lanes can be?  Called before the next run is enqueued and from ssfm_synchronize /
    // ssfm_last_propagate_ms / ssfm_last_run_info (where the run has ended anyway); waits for the run's closing event.
    int lane_health() {
        if (lanes.cooldown_due(nlanes)) {
            const int before = lanes.cooldown_begin();
            if (int rc = heal_lanes()) return rc;
            lanes.cooldown_end(nlanes, before);
        }
        if (!lanes.look_due(run_e1 != nullptr)) return SSFM_OK;
        HIP_TRY(hipEventSynchronize(run_e1));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, run_e0, run_e1));
        return lanes.run_measured(ms) ? heal_lanes() : (int)SSFM_OK;
    }
    int heal_lanes() {
        lanes.heal_begin();
        HIP_TRY(hipStreamSynchronize(stream));
        const size_t cb = sizeof(cx<T>) * (size_t)n * batch;
        DeviceBuffer<cx<T>> Fx_own, Yx_own;          // (scratch fields that live for this rating)
        DeviceBuffer<T> Px_own;
        if (Fx_own.reserve(cb) != hipSuccess) { (void)hipGetLastError(); return SSFM_OK; }       // (no memory for the scratch fields: the run's result is right, only slow)
        if (Y != F && Yx_own.reserve(cb) != hipSuccess) { (void)hipGetLastError(); return SSFM_OK; }
        if (Px_own.reserve(sizeof(T) * (size_t)n * batch) != hipSuccess) { (void)hipGetLastError(); return SSFM_OK; }
        cx<T>* const Fx = Fx_own; cx<T>* const Yx = Y != F ? Yx_own.get() : Fx; T* const Px = Px_own;
        (void)hipMemsetAsync(Fx, 0, cb, stream);
        if (Yx != Fx) (void)hipMemsetAsync(Yx, 0, cb, stream);
        (void)hipMemsetAsync(Px, 0, sizeof(T) * (size_t)n * batch, stream);
        const float seen = lanes.lane_pair_us;
        bool replaced = false;
        const int rc = rate_and_replace_lanes(Fx, Yx, Px, &replaced);
        (void)hipStreamSynchronize(stream);
        if (rc != SSFM_OK) return rc;
        lanes.heal_rated(replaced, seen);
        return SSFM_OK;
    }

    // stage twiddles of a line of length L in thread-load order (wgfft.hpp "Table layout"), computed
    // in double on the host and rounded once
    int make_line_table(DeviceBuffer<cx<T>>* out, int L, int E) {
        const int M = fft_nstages(L, E);
        const int total = fft_tw_entries(L, E, (int)sizeof(T));
        std::vector<cx<T>> tab((size_t)(total > 0 ? total : 1));
        for (int S = 1; S < M; ++S) {
            const int R = fft_radix(L, S, E), NB = E / R, KU = fft_tw_ku(L, S, E), off = fft_tw_offset(L, S, E, (int)sizeof(T));
            for (int i = 0; i < NB; ++i)
                for (int u = 1; u < R; ++u)
                    for (int ku = 0; ku < KU; ++ku) {
                        const int q = fft_tw_exponent(L, E, S, i, u, ku) % L;
                        const double ang = -2.0 * 3.14159265358979323846 * (double)q / (double)L;
                        cx<T> w; w.x = (T)std::cos(ang); w.y = (T)std::sin(ang);
                        if (q == 0) { w.x = (T)1; w.y = (T)0; }
                        if (4 * q == L) { w.x = (T)0; w.y = (T)-1; }
                        if (2 * q == L) { w.x = (T)-1; w.y = (T)0; }
                        if (4 * q == 3 * L) { w.x = (T)0; w.y = (T)1; }
                        tab[(size_t)off + (size_t)fft_tw_index(L, S, E, (int)sizeof(T), i * (R - 1) + (u - 1), ku)] = w;
                    }
        }
        HIP_TRY(out->reserve(sizeof(cx<T>) * tab.size()));
        HIP_TRY(hipMemcpy(out->get(), tab.data(), sizeof(cx<T>) * tab.size(), hipMemcpyHostToDevice));
        return SSFM_OK;
    }

#if SSFM_TRACE
    DeviceBuffer<unsigned long long> trace_buf;
    int trace_cap = 0; std::atomic<int> trace_next{0};
    std::vector<int> trace_kind;        // per slot: kind*16 + lane
    int trace_begin(int launches) {
        if (!std::getenv("SSFM_TRACE_FILE")) return SSFM_OK;
        if (trace_cap < launches) {
            HIP_TRY(trace_buf.reserve(sizeof(unsigned long long) * 1024 * launches));
            trace_cap = launches;
        }
        HIP_TRY(hipMemset(trace_buf, 0, sizeof(unsigned long long) * 1024 * launches));
        trace_next = 0;
        trace_kind.assign(launches, 0);
        return SSFM_OK;
    }
    template <typename A> void trace_tag(A& a, int kind, int lane) {
        a.trace = nullptr; a.trace_slot = 0;
        if (trace_buf) { const int slot = trace_next.fetch_add(1); if (slot < trace_cap) { a.trace = trace_buf; a.trace_slot = slot; trace_kind[slot] = kind * 16 + lane; } }     // (the lanes' host threads tag concurrently)
    }
    int trace_dump() {
        const char* path = std::getenv("SSFM_TRACE_FILE");
        if (!path || !trace_buf) return SSFM_OK;
        HIP_TRY(hipStreamSynchronize(stream));
        const int nt = std::min((int)trace_next, trace_cap);
        std::vector<unsigned long long> raw(1024 * (size_t)nt), h(4 * (size_t)nt);
        HIP_TRY(hipMemcpy(raw.data(), trace_buf, sizeof(unsigned long long) * raw.size(), hipMemcpyDeviceToHost));
        for (int i = 0; i < nt; ++i) {
            unsigned long long fs = ~0ull, ls = 0, fe = ~0ull, le = 0;
            for (int b = 0; b < 256; ++b) {
                const unsigned long long s0 = raw[((size_t)i * 256 + b) * 4], e0 = raw[((size_t)i * 256 + b) * 4 + 1];
                if (s0 == 0) continue;
                fs = s0 < fs ? s0 : fs; ls = s0 > ls ? s0 : ls; fe = e0 < fe ? e0 : fe; le = e0 > le ? e0 : le;
            }
            h[4 * i] = fs; h[4 * i + 1] = ls; h[4 * i + 2] = fe; h[4 * i + 3] = le;
        }
        FILE* f = std::fopen(path, "w");
        if (!f) return SSFM_OK;
        std::fprintf(f, "slot,kind,lane,first_start,last_start,first_end,last_end\n");
        for (int i = 0; i < nt; ++i)
            std::fprintf(f, "%d,%d,%d,%llu,%llu,%llu,%llu\n", i, trace_kind[i] / 16, trace_kind[i] % 16, h[4 * i], h[4 * i + 1], h[4 * i + 2], h[4 * i + 3]);
        std::fclose(f);
        // SSFM_TRACE_RAW=path: every workgroup of launches [first, first + count) of the run (SSFM_TRACE_RAW_FIRST, default the middle; 16 launches)
        if (const char* rp = std::getenv("SSFM_TRACE_RAW")) {
            if (FILE* g = std::fopen(rp, "w")) {
                int first = nt / 2;
                if (const char* e = std::getenv("SSFM_TRACE_RAW_FIRST")) first = std::atoi(e);
                std::fprintf(g, "slot,kind,lane,block,start,end,xcc,hw_id\n");
                for (int i = first; i < first + 16 && i < nt; ++i)
                    for (int b = 0; b < 256; ++b) {
                        const unsigned long long* w = &raw[((size_t)i * 256 + b) * 4];
                        std::fprintf(g, "%d,%d,%d,%d,%llu,%llu,%llu,%llu\n", i, trace_kind[i] / 16, trace_kind[i] % 16, b, w[0], w[1], w[2] >> 32, w[2] & 0xffffffffull);
                    }
                std::fclose(g);
            }
        }
        return SSFM_OK;
    }
#endif

    int use_device() {
        HIP_TRY(hipSetDevice(device));
        if (cap_pending) {                 // a capture run's helper thread: its transfers are complete when it returns
            cap_pending = false;
            if (int rc = cap_worker.wait()) return rc;
        }
        return medium_pending ? finish_medium() : (int)SSFM_OK;
    }
    // A single-launch run of a medium plan is asynchronous like every run; whether one of its barriers ran out of patience is known
    // once it has finished.  The next call that uses the plan looks: on an error the input is restored and the run repeated on the
    // two-kernel engine (and the plan keeps to it).
    int finish_medium() {
        medium_pending = false;
        HIP_TRY(hipStreamSynchronize(stream));
        if (medium_err_host[0] == 0u && medium_err_host[1] == 0u) return SSFM_OK;
        medium_err_host[0] = medium_err_host[1] = 0u;
        medium_gave_up(medium_ok);                 // (ahead of the repeat: it must not choose this engine again)
        HIP_TRY(hipMemcpyAsync(F, fused_backup, sizeof(cx<T>) * n * batch, hipMemcpyDeviceToDevice, stream));
        const std::vector<T> sched = medium_sched;
        if (int rc = propagate_fixed(medium_gamma, sched.data(), (int64_t)sched.size(), nullptr)) return rc;
        HIP_TRY(hipStreamSynchronize(stream));
        last_fell_back = 1;                        // (again: the repeat is a run of its own and cleared it)
        return SSFM_OK;
    }
    // the XCDs a launch's workgroups are dealt to (probe launch, once per device), and this plan's among them: plans take turns
    int pick_xcc() {
        if (medium_xcc >= 0) return SSFM_OK;
        static std::atomic<int> next_plan{0};
        const unsigned mask = xcc_mask(device);
        if (mask == 0u) { medium_ok = medium_adapt_ok = false; return SSFM_OK; }        // (the probe launch failed: the launch-per-pass engines)
        medium_xccs = __builtin_popcount(mask);
        int k = next_plan.fetch_add(1) % medium_xccs;
        for (int b = 0; b < 32; ++b)
            if ((mask >> b) & 1u) { if (k == 0) { medium_xcc = b; break; } --k; }
        return SSFM_OK;
    }
    // ---- the host side of a launch on one XCD, for the four engines that are one (k_medium, k_medium_adapt, k_medium_chirp, k_medium_chirp_adapt)
    // Ahead of the launch: `sets` of the two sets of meeting words zeroed on the plan's stream (a launch meets in one set), the plan's XCD, and what
    // the four argument structs share filled in: the plan's fields and twiddles, where and how long the workgroups of `rows` rows meet.
    template <typename Args>
    int medium_prepare(Args& a, int rows, int sets) {
        if (int rc = ensure_medium_state()) return rc;
        HIP_TRY(hipMemsetAsync(medium_st, 0, sizeof(unsigned long long) * sets * kSet, stream));
        if (int rc = pick_xcc()) return rc;
        a.F = F; a.Y = Y; a.P = P; a.twA = twA; a.twB = twB; a.tw1 = tw1; a.tw2 = tw2;
        medium_meet_in(a, 0);
        a.patience = medium_patience;
        a.xcc = (unsigned)medium_xcc;
        a.rows = rows; a.nblk = (unsigned)((N2 / cols_per_tile<T>()) * rows); a.Qf = N2 / Ef;
        return SSFM_OK;
    }
    // a launch's set of meeting words: the shards and flag words, then the error word, then the ticket counter
    template <typename Args>
    void medium_meet_in(Args& a, int set) {
        a.bar = medium_st + set * kSet;
        a.error = reinterpret_cast<unsigned*>(a.bar + kBarShards + kBarWords);
    }
    // Behind the launch, on stream `s`: its error word (not zero: its workgroups did not meet within the patience) ...
    template <typename Args>
    int medium_verdict(const Args& a, unsigned* gave_up, hipStream_t s) {
        HIP_TRY(hipMemcpyAsync(gave_up, a.error, sizeof(unsigned), hipMemcpyDeviceToHost, s));
        return SSFM_OK;
    }
    // ... and of an adaptive run also the step state's error word (the hand-over of the maxima) and where the run stands; waits for all three
    template <typename Args>
    int medium_adapt_verdict(const Args& a, unsigned gave_up[2], StepState<T>* now) {
        const char* state = reinterpret_cast<const char*>(st.get());
        if (int rc = medium_verdict(a, &gave_up[0], stream)) return rc;
        HIP_TRY(hipMemcpyAsync(&gave_up[1], state + offsetof(AdaptState<T>, error), sizeof(unsigned), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipMemcpyAsync(now, state + offsetof(AdaptState<T>, cur), sizeof(*now), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        return SSFM_OK;
    }
    // A run whose workgroups did not meet: the plan keeps off that engine from here on (`engine_ok`: medium_ok or medium_adapt_ok) and says so
    void medium_gave_up(bool& engine_ok) {
        engine_ok = false;
        ++fallbacks;
        last_fell_back = 1;
    }
    // the whole schedule in one launch (k_medium); `distinct` holds at most kMaxTables step sizes
    int run_medium(T gamma, double gamma_d, const Schedule<T>& sch, bool phase) {
        if constexpr (sizeof(T) != 4) { (void)gamma; (void)gamma_d; (void)sch; (void)phase; return fail(SSFM_ERR_STATE, "the medium engine is complex64 only"); }
        else {
        const std::vector<T>& distinct = sch.distinct;
        const int64_t nsteps = sch.size();
        MediumArgs<T> a;
        std::memset(&a, 0, sizeof(a));
        if (int rc = tables_for(distinct, a.tab, false, phase ? 1 : 0)) return rc;
        for (size_t i = 0; i < distinct.size(); ++i) { const T xr = op_re0 * distinct[i]; a.amp[i] = (T)std::exp((double)xr) * inv_n(); }
        if (int rc = upload_schedule(sch)) return rc;
        if (int rc = backup_field()) return rc;                  // for a repeat on the two-kernel engine
        // The rows of a fixed-step run share nothing: a dual-polarisation plan of long rows (2^16 samples and more) runs them as TWO launches, each
        // on an XCD and a stream of its own (2^16 x 2: 8.3 against 9.25 us per step in one launch; 2^17 x 2 only fits this way)
        const bool two = medium_rows_split(medium_split_ok, n, batch);
        if (int rc = medium_prepare(a, two ? 1 : batch, 2)) return rc;        // (both sets of meeting words: the second launch has its own)
        a.hs = d_hs; a.which = d_which(sch);
        a.gamma = gamma; a.inv_n = inv_n(); a.nsteps = (int)nsteps;
        if (two) {
            if (!medium_stream2) {
                HIP_TRY(hipStreamCreateWithFlags(medium_stream2.out(), hipStreamNonBlocking));
                HIP_TRY(hipEventCreateWithFlags(medium_ev2.out(), hipEventDisableTiming));
            }
            HIP_TRY(hipEventRecord(fork_ev, stream));                  // (behind the uploads and the backup copy, ahead of the first launch)
            HIP_TRY(hipStreamWaitEvent(medium_stream2, fork_ev, 0));
        }
        ++last_launches;
        HIP_TRY(launch_medium(N1, N2, phase, (int)a.nblk, medium_xccs, stream, a));
        // (the run is asynchronous: the words land in pinned memory and finish_medium looks at them when the plan is next used)
        if (int rc = medium_verdict(a, medium_err_host, stream)) return rc;
        medium_err_host[1] = 0u;
        if (two) {
            MediumArgs<T> b = a;
            b.F = F + n; b.Y = Y + n; b.P = P + n;
            medium_meet_in(b, 1);
            // the next XCD of the device's set
            const unsigned mask = xcc_mask(device);
            unsigned nx = (unsigned)medium_xcc;
            do { nx = (nx + 1u) & 31u; } while (!((mask >> nx) & 1u));
            b.xcc = medium_xccs > 1 ? nx : (unsigned)medium_xcc;
            ++last_launches;
            HIP_TRY(launch_medium(N1, N2, phase, (int)b.nblk, medium_xccs, medium_stream2, b));
            if (int rc = medium_verdict(b, medium_err_host + 1, medium_stream2)) return rc;
            HIP_TRY(hipEventRecord(medium_ev2, medium_stream2));
            HIP_TRY(hipStreamWaitEvent(stream, medium_ev2, 0));
        }
        medium_sched = sch.steps;
        medium_gamma = gamma_d;
        medium_pending = true;
        return SSFM_OK;
        }
    }

    int set_operator(const void* host) {
        if (int rc = use_device()) return rc;
        {
            const T* d = static_cast<const T*>(host);             // (re, im) pairs
            bool flat = true;
            for (int64_t i = 1; i < n_full && flat; ++i) flat = std::memcmp(&d[2 * i], &d[0], sizeof(T)) == 0;
            op_flat_re = flat;
            op_re0 = d[0];
            dimag_valid = false;
            dsplit_valid = false;
        }
        HIP_TRY(hipMemcpyAsync(dnat, host, sizeof(cx<T>) * n_full, hipMemcpyHostToDevice, stream));
        if (is_split()) {           // (the operator's split-order forms are made where they are used: tables_for, split_fly_ready)
            HIP_TRY(hipStreamSynchronize(stream));
            for (auto& t : tabs) t.valid = false;
            have_op = true;
            tags[0] = 0;
            return SSFM_OK;
        }
        hipLaunchKernelGGL((k_make_freq_table<T, 0>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream,
                           (const cx<T>*)dnat, dperm, N1, N2, N2 / Ef, (T)0, inv_n());
        if (dperm_fly)
            hipLaunchKernelGGL((k_make_freq_table<T, 0>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream,
                               (const cx<T>*)dnat, dperm_fly, N1, N2, N2 / Ef_fly, (T)0, inv_n());
        if (dsmall)
            hipLaunchKernelGGL((k_make_freq_table<T, 0>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream,
                               (const cx<T>*)dnat, dsmall, 1, (int)n, (int)n / small_points<T>((int)n), (T)0, inv_n());
        HIP_TRY(hipGetLastError());
        // host buffer may be reused by the caller right after return
        HIP_TRY(hipStreamSynchronize(stream));
        for (auto& t : tabs) t.valid = false;
        for (auto& t : stabs) t.valid = false;
        have_op = true;
        tags[0] = 0;
        return SSFM_OK;
    }

    // exp(D~ h)/N for every step size of a schedule (at most kMaxTables), cached per distinct h.  `one_line`: the table of the
    // single-launch engine (N1 = 1: the table index is the frequency index), else the transposed order of k_freq.
    // A slot that holds a table this schedule needs is never the victim of another of its tables (a round-robin victim could
    // be: schedules {a,b}, {c,d}, {a,e} on one plan would have run a's steps with e's table).
    int tables_for(const std::vector<T>& distinct, const cx<T>** out, bool one_line, int kind = 0) {
        Tab* cache = one_line ? stabs : tabs;
        int& rr = one_line ? stab_rr : tab_rr;
        bool pinned[kMaxTables] = {};
        for (size_t i = 0; i < distinct.size(); ++i) {
            out[i] = nullptr;
            for (int k = 0; k < kMaxTables; ++k)
                if (cache[k].valid && cache[k].kind == kind && std::memcmp(&cache[k].h, &distinct[i], sizeof(T)) == 0) { out[i] = cache[k].ptr; pinned[k] = true; }
        }
        for (size_t i = 0; i < distinct.size(); ++i) {
            if (out[i]) continue;
            int v = rr;
            while (pinned[v]) v = (v + 1) % kMaxTables;      // distinct.size() <= kMaxTables: there is one
            Tab& t = cache[v];
            rr = (v + 1) % kMaxTables;
            pinned[v] = true;
            t.valid = false;
            HIP_TRY(t.ptr.reserve(sizeof(cx<T>) * n_full));
            t.kind = kind;
            if (is_split() && kind == 1)
                hipLaunchKernelGGL(k_make_split_phase_table<T>, dim3((unsigned)((n_full + 255) / 256)), dim3(256), 0, stream,
                                   (const cx<T>*)dnat, reinterpret_cast<unsigned*>(t.ptr.get()), N1, N2, split_R, distinct[i], split_qf());
            else if (is_split())
                hipLaunchKernelGGL((k_make_split_table<T, 2>), dim3((unsigned)((n_full + 255) / 256)), dim3(256), 0, stream,
                                   (const cx<T>*)dnat, t.ptr.get(), N1, N2, split_R, distinct[i], inv_n_full(), split_qf());
            else if (one_line)
                hipLaunchKernelGGL((k_make_freq_table<T, 2>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream,
                                   (const cx<T>*)dnat, t.ptr.get(), 1, (int)n, (int)n / small_points<T>((int)n), distinct[i], inv_n());
            else if (kind == 1)
                hipLaunchKernelGGL(k_make_phase_table<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream,
                                   (const cx<T>*)dnat, reinterpret_cast<unsigned*>(t.ptr.get()), N1, N2, N2 / Ef, distinct[i]);
            else
                hipLaunchKernelGGL((k_make_freq_table<T, 2>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream,
                                   (const cx<T>*)dnat, t.ptr.get(), N1, N2, N2 / Ef, distinct[i], inv_n());
            HIP_TRY(hipGetLastError());
            t.h = distinct[i]; t.valid = true;
            out[i] = t.ptr;
        }
        return SSFM_OK;
    }

    TimeArgs<T> targs(T gamma, T hh_prev, T hh_next, AdaptState<T>* s, int row0 = 0, int lane = 0) {
        TimeArgs<T> a;
#if SSFM_TRACE
        trace_tag(a, 0, lane);
#endif
        (void)lane;
        a.F = F + (size_t)row0 * n; a.Y = Y + (size_t)row0 * n; a.P = P + (size_t)row0 * n; a.twN = twN; a.twA = twA; a.twB = twB; a.tw1 = tw1; a.st = s; a.zlog = zlog; a.gamma = gamma;
        a.hh_prev = hh_prev; a.hh_next = hh_next; a.N2 = N2; a.rows = 0; a.Qf = N2 / Ef; a.step = 0; a.derive = 0;
        a.s_in = nullptr; a.s_out = nullptr; a.pkeep = nullptr; a.mul = nullptr;
        return a;
    }
    FreqArgs<T> fargs(const cx<T>* tab, T h, const AdaptState<T>* s, int row0 = 0, int lane = 0) {
        FreqArgs<T> a;
#if SSFM_TRACE
        trace_tag(a, 1, lane);
#endif
        (void)lane;
        a.F = Y + (size_t)row0 * n; a.tab = tab; a.tw2 = tw2; a.st = s; a.h = h; a.inv_n = inv_n(); a.N1 = N1; a.rows = 0; a.u16 = u16 ? 1 : 0; a.step = 0; a.amp = (T)0;
        return a;
    }

    // k_freq<FM_FLY_IM> can serve this plan's adaptive steps: a fibre's operator on a complex64 plan in the unit layout; makes the table on first use
    bool fly_imag_ready() {
        if constexpr (sizeof(T) != 4) return false;
        else {
        if (!u16 || !op_flat_re || Ef_fly % 4 != 0) return false;
        if (!dimag_valid) {
            if (dimag_fly.reserve(sizeof(T) * n) != hipSuccess) { (void)hipGetLastError(); return false; }
            hipLaunchKernelGGL(k_make_imag_table<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, (const cx<T>*)dnat, dimag_fly.get(), N1, N2, N2 / Ef_fly);
            if (hipGetLastError() != hipSuccess) return false;
            dimag_valid = true;
        }
        return true;
        }
    }
    // k_freq<FM_FLY>: D~ and the row twiddles in the order of ITS points per thread
    FreqArgs<T> fargs_fly(T h, const AdaptState<T>* s, int row0 = 0, int lane = 0) {
        FreqArgs<T> a = fargs(dperm_fly ? dperm_fly.get() : dperm.get(), h, s, row0, lane);
        if (tw2_fly) a.tw2 = tw2_fly;
        return a;
    }

    int copy_field_out(void* dst, bool is_device, bool wait) {
        if (int rc = ensure_nat()) return rc;
        HIP_TRY(hipMemcpyAsync(dst, user_field(), sizeof(cx<T>) * n * batch, is_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, stream));
        if (wait) HIP_TRY(hipStreamSynchronize(stream));
        return SSFM_OK;
    }

    // the whole schedule in one launch (k_small); `distinct` holds at most kMaxTables step sizes
    int run_small(T gamma, const Schedule<T>& sch, cx<T>* dsnap = nullptr) {
        SmallArgs<T> a;
        std::memset(&a, 0, sizeof(a));
        if (int rc = tables_for(sch.distinct, a.tab, true)) return rc;
        if (int rc = upload_schedule(sch)) return rc;
        a.F = F; a.hs = d_hs; a.which = d_which(sch); a.tw = tw_small; a.snap = dsnap; a.gamma = gamma; a.nsteps = (int)sch.size();
        ++last_launches;
        HIP_TRY(launch_small<T>((int)n, batch, stream, a));
        return SSFM_OK;
    }

    // What a capture run (propagate_fixed_capture) adds to propagate_fixed's lanes: where the scalar log of a step goes, and what happens at a capture step.
    // Snapshot 0 (the input) and the last one (the end field) go to the host straight from F; the snapshots in between are written by the capture steps'
    // END launches into the ring's slots (ssfm_capture.hpp CapRing: which slot, which block, when it leaves), and a block is sent ("flushed") when it is
    // full -- by the helper thread, which waits ON THE HOST for the lanes' END events and tells the lanes' threads, through `flushes_done`, when a block may
    // be written again.
    struct CapRun {
        CapRing ring;                       // (ring.every > 0: snapshots)
        ScalLog log = {};
        char* host = nullptr;               // the caller's buffer
        double* scalars_host = nullptr;
        double* scal = nullptr;             // the wavefronts' pairs (ScalLog)
        int nlanes = 0;
        std::atomic<int64_t> ends_done[kMaxLanes];     // flushes whose last END event a lane has recorded
        std::atomic<int64_t> flushes_done{0};               // flushes whose transfer is complete (their block may be written again)
        std::atomic<int64_t> input_done{0};                 // the input's transfer is complete (F may be written)
        std::atomic<int64_t> run_queued{0};                 // 1: the run is queued (ev1 recorded), 2: it failed
        std::atomic<int> failed{0};
        double* scal_at(int64_t step, int row0) const { return scal ? scal + log.at(step, row0) : nullptr; }
        bool wait_for(std::atomic<int64_t>& c, int64_t want) {
            for (unsigned spins = 0; c.load(std::memory_order_acquire) < want; ++spins) {
                if (failed.load()) return false;
                if (spins < 4096u) std::this_thread::yield();
                else std::this_thread::sleep_for(std::chrono::microseconds(20));
            }
            return true;
        }
    };
    CapRun cap_cr;                          // (a member: the helper thread works on it after propagate_fixed_capture has returned)
    CapRun* cap_run = nullptr;              // set around the propagate_fixed call of a capture run

    // One fixed-step run as its drivers see it: the caller's arguments, the schedule, the route it takes (ssfm_route.hpp fixed_route) and the two-kernel
    // engine's operator tables.  `nlanes` is lanes_active when the run was asked for (a plan that dropped to one lane drives its rows on one stream).
    struct FixedRun {
        T gamma; const T* h; int64_t nsteps; const Schedule<T>* sch;
        int nlanes, rows;                  // rows per lane
        FixedRoute route;
        std::vector<const cx<T>*> tabptr;
    };
    FixedState fixed_state() {
        return {medium_ok, medium_split_ok, phase_tables, force_fly, profiling, SSFM_TRACE != 0, op_flat_re, twA != nullptr, medium_shape(N1, N2), lanes.lanes_active, run_e0 != nullptr};
    }
    int propagate_fixed(double gamma_d, const T* h, int64_t nsteps, void* snapshots) {
        if (!have_op) return fail(SSFM_ERR_STATE, "ssfm_propagate_fixed: call ssfm_set_linear_operator first");
        if (int rc = use_device()) return rc;
        if (int rc = lane_health()) return rc;             // (the previous run, if it was a long two-lane run: slow lanes are repaired before this one is enqueued)
        last_launches = 0; timed = false;
        if (nsteps <= 0) return SSFM_OK;
        // distinct step sizes -> operator tables (normally 1, +1 for a short last step)
        const Schedule<T> sch(h, nsteps, kMaxTables);
        if (!sch.valid())
            return fail(SSFM_ERR_INVALID, "ssfm_propagate_fixed: step %lld is %g km (must be finite and > 0)", (long long)sch.first_bad, (double)h[sch.first_bad]);
        FixedRun fr = {(T)gamma_d, h, nsteps, &sch, lanes.lanes_active, batch / lanes.lanes_active,
                       fixed_route<T>(shape, fixed_state(), FixedRequest{nsteps, sch.fits_tables(), snapshots != nullptr, cap_run != nullptr}),
                       std::vector<const cx<T>*>(sch.distinct.size(), nullptr)};
        const FixedRoute& r = fr.route;
        if (int rc = ensure_sub()) return rc;
        if (is_split() && !r.use_tables) if (int rc = split_fly_ready()) return rc;
        last_fell_back = 0;
        if (r.use_tables && !r.go_small && !r.go_medium)
            if (int rc = tables_for(sch.distinct, fr.tabptr.data(), false, r.use_phase ? 1 : 0)) return rc;
        for (auto& p : prof) p.n = 0;
        HIP_TRY(hipEventRecord(ev0, stream));
        if (r.health) HIP_TRY(hipEventRecord(run_e0, stream));
        // z-resolved capture (reference devices.py:1150-1152, 1184-1186).  The field after every step is
        // copied device-to-device into a block of up to `block` snapshots -- asynchronous, the step loop
        // never waits for the host -- and a block goes to the host in one transfer.
        int64_t block = 0;
        DeviceBuffer<char> dsnap;                       // (lives for this call)
        if (snapshots != nullptr) {
            size_t free_b = 0, total_b = 0, fb = field_bytes();
            HIP_TRY(hipMemGetInfo(&free_b, &total_b));
            block = snap_block(nsteps, free_b, fb);
            HIP_TRY(dsnap.reserve(fb * (size_t)block));
        }
        const bool whole = snap_whole(block, nsteps);    // a small plan whose whole capture fits the device: the single launch writes every snapshot itself
        last_engine = snapshots != nullptr && !whole ? r.engine_in_blocks : r.engine;
        if (snapshots != nullptr) {
            if (int rc = r.small_sched && whole ? snapshots_small(fr, snapshots, dsnap) : snapshots_every_step(fr, snapshots, dsnap, block)) return rc;
        } else {
#if SSFM_TRACE
            if (int rc = trace_begin((int)(2 * nsteps + 1) * fr.nlanes)) return rc;
#endif
            if (r.go_small) {
                if (int rc = run_small(fr.gamma, sch)) return rc;
            } else if (r.go_medium) {
                if (int rc = run_medium(fr.gamma, gamma_d, sch, r.use_phase)) return rc;
                if (external_order) {          // (see external_order: the caller may consume the field stream-ordered, without ssfm_synchronize)
                    HIP_TRY(hipEventRecord(ev1, stream));
                    timed = true;
                    return finish_medium();
                }
            } else if (int rc = run_lanes(fr)) return rc;
#if SSFM_TRACE
            if (int rc = trace_dump()) return rc;
#endif
        }
        // the common tail
        ran();
        if (int rc = publish_if_external()) return rc;          // (a caller that orders its own work on the stream finds the natural-order field)
        HIP_TRY(hipEventRecord(ev1, stream));
        timed = true;
        if (r.health) {
            HIP_TRY(hipEventRecord(run_e1, stream));
            lanes.run_enqueued((is_split() ? 4 : 2) * nsteps + 1);
        }
        if (snapshots != nullptr) HIP_TRY(hipStreamSynchronize(stream));
        return SSFM_OK;
    }
    // ---- the two-kernel engine's launches.  The sequence of a run is BEGIN, (row pass, MID)*, row pass, END on every lane: lane g drives `rows` rows from
    // row g * rows on lane_stream[g] (one lane: all rows on the plan's stream, which is lane 0's).  The three launches of it, spelled once; the drivers
    // below differ in the ORDER they issue them in.
    hipError_t row_launch(const FixedRun& fr, int64_t s, int row0, int rows, hipStream_t st_) {
        const FixedRoute& r = fr.route;
        const int lane_ = rows > 0 ? row0 / rows : 0;
        const T hs = fr.h[s];
        const cx<T>* const tp = r.use_tables ? fr.tabptr[fr.sch->which[(size_t)s]] : nullptr;
        ++last_launches;
        if (is_split()) {
            last_launches += 2;
            const T xr = op_re0 * hs;
            return split_freq(tp, hs, nullptr, 0, row0, rows, st_, r.use_phase, (T)std::exp((double)xr) * inv_n_full());
        }
        if (r.use_tables) {
            if (r.use_phase) {
                FreqArgs<T> fa = fargs(tp, hs, nullptr, row0, lane_);
                // the modulus as the complex table forms it: e = exp(Re * h) with the product in T, then e * (1/N) (exact: N = 2^k)
                const T xr = op_re0 * hs;
                fa.amp = (T)std::exp((double)xr) * inv_n();
                return launch_freq<T, FM_PHASE>(N2, N1 * rows, st_, fa, Ef);
            }
            return launch_freq<T, FM_TABLE>(N2, N1 * rows, st_, fargs(tp, hs, nullptr, row0, lane_), Ef);
        }
        return launch_freq<T, FM_FLY>(N2, N1 * rows, st_, fargs_fly(hs, nullptr, row0, lane_), Ef_fly);
    }
    hipError_t col_begin(const FixedRun& fr, int g) {
        TimeArgs<T> a = targs(fr.gamma, 0, fr.h[0] * (T)0.5, nullptr, g * fr.rows, g);
        if (cap_run) a.scal = cap_run->scal_at(0, g * fr.rows);
        ++last_launches;
        return launch_time<T, TM_BEGIN>(N1, fr.rows, lane_stream[g], a, E);
    }
    hipError_t row_pass(const FixedRun& fr, int g, int64_t s) { return row_launch(fr, s, g * fr.rows, fr.rows, lane_stream[g]); }
    hipError_t col_after(const FixedRun& fr, int g, int64_t s) {            // MID between two steps, END behind the last one
        const bool last = s + 1 == fr.nsteps;
        TimeArgs<T> a = targs(fr.gamma, fr.h[s] * (T)0.5, last ? (T)0 : fr.h[s + 1] * (T)0.5, nullptr, g * fr.rows, g);
        if (cap_run) a.scal = cap_run->scal_at(s + 1, g * fr.rows);
        ++last_launches;
        return last ? launch_time<T, TM_END>(N1, fr.rows, lane_stream[g], a, E) : launch_time<T, TM_MID>(N1, fr.rows, lane_stream[g], a, E);
    }
    // one lane's launches, start to end.  A capture run (cap_run) adds: the scalar log's address to the column launches, and at a capture step an END
    // launch BESIDE the run -- it only reads the half-transformed field and writes this step's time-order field straight into a slot of a device block
    // (no copy of F); the MID behind it continues exactly as a run without capture does, so the snapshots and the end field are a plain run's, bit for
    // bit.  The lane records an event behind the END that fills a block; the helper thread sends the block to the host once every lane's event is
    // through.  Before a block is written again the lane's THREAD waits (on the host) until the helper has seen its transfer complete: the lanes'
    // threads run ahead of the GPU by at most the ring of blocks, the GPU never waits as long as PCIe keeps up.
    int lane_run(const FixedRun& fr, int g) {
        CapRun* const cr = cap_run;
        const bool snaps = cr && cr->ring.every > 0;
        auto body = [&]() -> int {
            // (round 6 A/B: starting lane 1 of a complex128 run 5 ... 40 us late changes nothing -- 38.6-39.4 against 38.6-38.9 us per step, profiles/r06_c1_ab.txt)
            HIP_TRY(col_begin(fr, g));
            int64_t k = 1;                                       // the next snapshot
            for (int64_t s = 0; s < fr.nsteps; ++s) {
                HIP_TRY(row_pass(fr, g, s));
                const bool last = s + 1 == fr.nsteps;
                if (snaps && cr->ring.captures(s)) {
                    const CapSlot c = cr->ring.slot_of(k - 1);
                    if (c.wait_flushes && !cr->wait_for(cr->flushes_done, c.wait_flushes))      // the block is written again
                        return fail(SSFM_ERR_HIP, "ssfm_propagate_fixed_capture: the transfers failed");
                    TimeArgs<T> te = targs(fr.gamma, fr.h[s] * (T)0.5, 0, nullptr, g * fr.rows, g);
                    te.F = reinterpret_cast<cx<T>*>(cap_blocks + c.offset) + (size_t)(g * fr.rows) * n;
                    ++last_launches;
                    HIP_TRY((launch_time<T, TM_END>(N1, fr.rows, lane_stream[g], te, E)));
                    if (c.leaves) {
                        HIP_TRY(hipEventRecord(cap_ev_ends[g][c.flush], lane_stream[g]));
                        cr->ends_done[g].store(c.flush + 1, std::memory_order_release);
                    }
                    ++k;
                }
                if (last && snaps && !in_place() && !cr->wait_for(cr->input_done, 1))    // (the input's transfer reads F, which the END overwrites)
                    return fail(SSFM_ERR_HIP, "ssfm_propagate_fixed_capture: the transfers failed");
                HIP_TRY(col_after(fr, g, s));
            }
            return SSFM_OK;
        };
        const int rc = body();
        if (rc != SSFM_OK && cr) cr->failed.store(1);
        return rc;
    }
    int fork_lanes(int nl) {
        HIP_TRY(hipEventRecord(fork_ev, stream));
        for (int g = 1; g < nl; ++g) HIP_TRY(hipStreamWaitEvent(lane_stream[g], fork_ev, 0));
        return SSFM_OK;
    }
    int join_lanes(int nl) {
        for (int g = 1; g < nl; ++g) {
            HIP_TRY(hipEventRecord(lane_ev[g], lane_stream[g]));
            HIP_TRY(hipStreamWaitEvent(stream, lane_ev[g], 0));
        }
        return SSFM_OK;
    }
    // the two-kernel engine's run on its lanes: every lane from a host thread of its own, or all of them from this thread
    int run_lanes(const FixedRun& fr) {
        const int nl = fr.nlanes;
        if (cap_run != nullptr && nl == 1) return lane_run(fr, 0);
        if (nl > 1 && ((lane_threads && !profiling && fr.nsteps >= 16) || cap_run != nullptr)) {
            // every lane from a host thread of its own (LaneWorker): lane 0 from this one
            if (int rc = fork_lanes(nl)) return rc;
            for (int g = 1; g < nl; ++g) { lane_worker[g].start(device); lane_worker[g].submit([this, &fr, g] { return lane_run(fr, g); }); }
            int rc = lane_run(fr, 0);
            for (int g = 1; g < nl; ++g) { const int r = lane_worker[g].wait(); if (rc == SSFM_OK) rc = r; }
            if (rc != SSFM_OK) return rc;
            return join_lanes(nl);
        }
        // all lanes from this thread, interleaved: every lane's row pass, then every lane's column pass, step by step (one lane: the plan's stream alone)
        if (nl > 1) if (int rc = fork_lanes(nl)) return rc;
        for (int g = 0; g < nl; ++g) {
            if (int rc = prof_mark(-1, g)) return rc;
            HIP_TRY(col_begin(fr, g));
            if (int rc = prof_mark(0, g)) return rc;
        }
        for (int64_t s = 0; s < fr.nsteps; ++s) {
            for (int g = 0; g < nl; ++g) {
                HIP_TRY(row_pass(fr, g, s));
                if (int rc = prof_mark(1, g)) return rc;
            }
            for (int g = 0; g < nl; ++g) {
                HIP_TRY(col_after(fr, g, s));
                if (int rc = prof_mark(0, g)) return rc;
            }
        }
        for (int g = 0; g < nl; ++g) if (int rc = prof_mark(2, g)) return rc;
        return join_lanes(nl);
    }
    // snapshots of a small plan whose whole capture fits `dsnap`: the single launch writes every snapshot itself
    int snapshots_small(const FixedRun& fr, void* snapshots, DeviceBuffer<char>& dsnap) {
        const size_t fb = field_bytes();
        hipError_t e = hipMemcpyAsync(dsnap, F, fb, hipMemcpyDeviceToDevice, stream);             // the input
        int rc = e == hipSuccess ? run_small(fr.gamma, *fr.sch, reinterpret_cast<cx<T>*>(dsnap.get())) : fail(SSFM_ERR_HIP, "snapshot copy failed: %s", hipGetErrorString(e));
        if (rc == SSFM_OK) {
            e = hipMemcpyAsync(snapshots, dsnap, fb * (size_t)(fr.nsteps + 1), hipMemcpyDeviceToHost, stream);
            if (e == hipSuccess) e = hipStreamSynchronize(stream);
            if (e != hipSuccess) rc = fail(SSFM_ERR_HIP, "snapshot download failed: %s", hipGetErrorString(e));
        }
        dsnap.free();
        return rc;
    }
    // ... of any other plan: BEGIN, row pass, END on the plan's stream for every step, the field copied into `dsnap` behind it; blocks of `block` snapshots go to the host
    int snapshots_every_step(const FixedRun& fr, void* snapshots, DeviceBuffer<char>& dsnap, int64_t block) {
        const size_t fb = field_bytes();
        char* snap = static_cast<char*>(snapshots);
        auto flush = [&](int64_t first, int64_t count) -> int {
            hipError_t e = hipMemcpyAsync(snap + fb * first, dsnap, fb * (size_t)count, hipMemcpyDeviceToHost, stream);
            if (e == hipSuccess) e = hipStreamSynchronize(stream);
            if (e != hipSuccess) return fail(SSFM_ERR_HIP, "snapshot download failed: %s", hipGetErrorString(e));
            return SSFM_OK;
        };
        int64_t first = 0, held = 0;                    // snapshots [first, first + held) are in dsnap
        auto capture = [&]() -> hipError_t { return put_time_order(dsnap + fb * held++); };
        hipError_t ce = capture();
        for (int64_t s = 0; s < fr.nsteps && ce == hipSuccess; ++s) {
            if (held == block) { if (int rc = flush(first, held)) return rc; first += held; held = 0; }
            last_launches += 2;
            ce = launch_time<T, TM_BEGIN>(N1, batch, stream, targs(fr.gamma, 0, fr.h[s] * (T)0.5, nullptr), E);
            if (ce == hipSuccess) ce = row_launch(fr, s, 0, batch, stream);
            if (ce == hipSuccess) ce = launch_time<T, TM_END>(N1, batch, stream, targs(fr.gamma, fr.h[s] * (T)0.5, 0, nullptr), E);
            if (ce == hipSuccess) ce = capture();
        }
        if (ce != hipSuccess) return fail(SSFM_ERR_HIP, "snapshot run failed: %s", hipGetErrorString(ce));
        if (int rc = flush(first, held)) return rc;
        dsnap.free();                                   // (here, not behind the call: the run's closing event goes behind the wait that hipFree is)
        return SSFM_OK;
    }

    // ---- z-resolved capture with a stride and a scalar log (the reference collects the field after EVERY step, devices.py:1150-1152,
    // 1184-1186 -- 16 GiB for the headline run -- and its consumers, devices.py:2326-2563, plot a few hundred of them).  The run keeps the fused two-kernel
    // engine: a capture step ADDS an END launch beside the run, which writes that step's time-order field into a slot of a ring of plan-owned device
    // blocks; a helper thread sends a full block to the caller's (page-locked) buffer on a stream of its own while the run goes on.  The input and the end
    // field go straight from F.  The scalar log is a 16-byte store per wavefront of the column kernels (time_body<..., LOG>, TimeArgs::scal), reduced behind
    // the run.  Asynchronous: the buffers are valid after ssfm_synchronize (or any later call on the plan).
    //
    // NOTHING on the device waits across streams, and that is the point of the helper thread.  The first form of this function ordered the transfers with
    // events (hipStreamWaitEvent on the copy stream behind every lane's END, on the lanes behind the transfers): a stream that sits blocked on an event
    // which is milliseconds away slows the launches of EVERY other queue of the process -- the command processor keeps polling the blocked barrier packet
    // between their dispatches.  tools/attic/barrier_cost.hip, profiles/r05_barrier_cost.txt: two chains of 8.9 us kernels take 17.8 ms with an idle
    // third stream, 19.9 / 21.9 / 40 ms with a third stream blocked on an event 5 / 10 / 40 ms away (whatever its priority), 17.7 ms with a spinning
    // wavefront in its place.  In the capture run that was 1.2-1.4 ms per call (the copy stream's wait for the end of the run, queued 8 ms early -- the
    // host enqueues ahead) and 0.1 ms per snapshot (the marker behind each 0.7 ms transfer): +18-21 % at every = 100 (profiles/r05_capture_ab.txt).
    // Host waits (hipEventSynchronize, hipStreamSynchronize) put nothing into a queue.
    bool in_place() const { return static_cast<const void*>(Y) == static_cast<const void*>(F); }
    int capture_helper() {
        CapRun* const cr = &cap_cr;
        auto body = [&]() -> int {
            const CapRing& ring = cr->ring;
            const bool snaps = ring.every > 0;
            if (snaps) {                                                // snapshot 0: the input, from F
                HIP_TRY(hipEventSynchronize(cap_ev_in));
                HIP_TRY(hipMemcpyAsync(cr->host, in_place() ? cap_in.get() : reinterpret_cast<const char*>(F), ring.fb, hipMemcpyDeviceToHost, cap_stream));
                HIP_TRY(hipStreamSynchronize(cap_stream));
                cr->input_done.store(1, std::memory_order_release);
            }
            for (int64_t fl = 0; fl < ring.nflush; ++fl) {
                for (int g = 0; g < cr->nlanes; ++g) {
                    if (!cr->wait_for(cr->ends_done[g], fl + 1)) return fail(SSFM_ERR_HIP, "ssfm_propagate_fixed_capture: the run failed");
                    HIP_TRY(hipEventSynchronize(cap_ev_ends[g][fl]));
                }
                const CapFlush f = ring.flush_of(fl);
                HIP_TRY(hipMemcpyAsync(cr->host + f.host_offset, cap_blocks + f.ring_offset, f.bytes, hipMemcpyDeviceToHost, cap_stream));
                HIP_TRY(hipStreamSynchronize(cap_stream));
                cr->flushes_done.store(fl + 1, std::memory_order_release);
            }
            if (!cr->wait_for(cr->run_queued, 1) || cr->run_queued.load() != 1) return fail(SSFM_ERR_HIP, "ssfm_propagate_fixed_capture: the run failed");
            HIP_TRY(hipEventSynchronize(ev1));                         // the end of the run on the plan's stream: every lane has joined
            if (snaps) HIP_TRY(hipMemcpyAsync(cr->host + ring.end_offset(), F, ring.fb, hipMemcpyDeviceToHost, cap_stream));      // the end field is the last snapshot
            if (cr->scalars_host) {
                // the log goes to the host behind the run: a pair (mean |A|^2, max |A|^2) per row and step
                double* red = cr->scal + cr->log.reduced_at();
                hipLaunchKernelGGL(k_scal_reduce<0>, dim3((unsigned)((ring.nsteps + 1) * batch)), dim3(64), 0, cap_stream, (const double*)cr->scal, red, cr->log.per_row, 1.0 / (double)n);
                HIP_TRY(hipGetLastError());
                HIP_TRY(hipMemcpyAsync(cr->scalars_host, red, cr->log.red_bytes, hipMemcpyDeviceToHost, cap_stream));
            }
            HIP_TRY(hipStreamSynchronize(cap_stream));
            return SSFM_OK;
        };
        const int rc = body();
        if (rc != SSFM_OK) cr->failed.store(1);
        return rc;
    }
    // a capture run's own resources, made on first use: the copy stream, the ring (made anew for another block size as well), the scalar log -- the wavefronts'
    // pairs, then the log reduced behind the run (k_scal_reduce) -- and an event per lane and flush (an event that is recorded again before its waiter has
    // looked at it would tie a transfer to a LATER END)
    int capture_resources(const CapRing& ring, const ScalLog& log, int nl, bool scalars) {
        if (int rc = ensure_cap_stream()) return rc;
        if (ring.nblocks > 0 && (cap_block_bytes != ring.block_bytes || cap_nblocks < ring.nblocks)) {
            cap_blocks.free(); cap_block_bytes = 0; cap_nblocks = 0;
            HIP_TRY(cap_blocks.reserve(ring.ring_bytes()));
            cap_block_bytes = ring.block_bytes; cap_nblocks = ring.nblocks;
        }
        if (scalars) if (int rc = grow(cap_scal, log.bytes())) return rc;
        for (int g = 0; g < nl; ++g)
            while ((int64_t)cap_ev_ends[g].size() < ring.nflush) {
                Event e;
                HIP_TRY(hipEventCreateWithFlags(e.out(), hipEventDisableTiming));
                cap_ev_ends[g].push_back(std::move(e));
            }
        return SSFM_OK;
    }
    int propagate_fixed_capture(double gamma_d, const T* h, int64_t nsteps, int64_t every, void* fields_host, double* scalars_host) {
        if (!have_op) return fail(SSFM_ERR_STATE, "ssfm_propagate_fixed_capture: call ssfm_set_linear_operator first");
        if (nsteps < 1 || nsteps > 0x7fffffff) return fail(SSFM_ERR_INVALID, "ssfm_propagate_fixed_capture: nsteps=%lld", (long long)nsteps);
        if ((fields_host != nullptr) != (every > 0)) return fail(SSFM_ERR_INVALID, "ssfm_propagate_fixed_capture: `fields` and `every` > 0 go together");
        if (!fields_host && !scalars_host) return fail(SSFM_ERR_INVALID, "ssfm_propagate_fixed_capture: nothing to capture");
        if (int rc = no_split("ssfm_propagate_fixed_capture")) return rc;
        if (int rc = use_device()) return rc;                          // (joins the previous capture run's helper)
        if (int rc = lane_health()) return rc;
        if (const Schedule<T> sch(h, nsteps, kMaxTables); !sch.valid())
            return fail(SSFM_ERR_INVALID, "ssfm_propagate_fixed_capture: step %lld is %g km (must be finite and > 0)", (long long)sch.first_bad, (double)h[sch.first_bad]);
        CapRun& cr = cap_cr;
        cr.ring = CapRing::make(field_bytes(), nsteps, every, fields_host != nullptr); cr.log = scal_log<T>(N1, N2, E, batch, nsteps); cr.nlanes = lanes.lanes_active;
        if (int rc = capture_resources(cr.ring, cr.log, cr.nlanes, scalars_host != nullptr)) return rc;
        cr.host = static_cast<char*>(fields_host); cr.scalars_host = scalars_host; cr.scal = scalars_host ? cap_scal.get() : nullptr;
        for (auto& e : cr.ends_done) e.store(0);
        cr.flushes_done.store(0); cr.input_done.store(0); cr.run_queued.store(0); cr.failed.store(0);
        if (fields_host) {
            // the input is in F once everything queued on the plan's stream so far is through.  The plans whose engine transforms F in place (Y == F:
            // complex128 and the complex64 plans outside the unit layout) overwrite it with their first launch: they keep a copy, made on the plan's stream
            if (in_place()) {
                if (int rc = grow(cap_in, cr.ring.fb)) return rc;
                HIP_TRY(hipMemcpyAsync(cap_in, F, cr.ring.fb, hipMemcpyDeviceToDevice, stream));
            }
            HIP_TRY(hipEventRecord(cap_ev_in, stream));
        }
        cap_worker.start(device);
        cap_worker.submit([this] { return capture_helper(); });
        cap_run = &cr;
        const int run_rc = propagate_fixed(gamma_d, h, nsteps, nullptr);             // (the run itself: propagate_fixed's lanes with the hooks above)
        cap_run = nullptr;
        cr.run_queued.store(run_rc == SSFM_OK ? 1 : 2, std::memory_order_release);
        if (run_rc != SSFM_OK) {
            const std::string err = ssfm::g_err;
            cr.failed.store(1);
            (void)cap_worker.wait();
            (void)hipDeviceSynchronize();
            std::snprintf(ssfm::g_err, sizeof(ssfm::g_err), "%s", err.c_str());
            return run_rc;
        }
        cap_pending = true;
        return SSFM_OK;
    }

    // ---- adaptive run (reference devices.py:1155-1161, 1172-1196 with h = None), in three parts so that a z-resolved
    // capture can go to the host in bounded blocks: adaptive_begin (first step size), adaptive_run (up to `budget`
    // steps; all of them without a capture), adaptive_finish (time-order field, z log).
    struct AdaptRun {
        bool active = false;
        T gamma = 0;
        T length = 0;
        int max_steps = 0;
        int step = 0;                  // index of the next step to launch
        StepState<T> now = {};         // state after the last launched step (host copy)
        bool fused = false, tile_private = false;      // the chunked engine's column pass (ssfm_route.hpp AdaptPiece)
        AdaptBegin deferred = ADAPT_CHUNKED;      // a small or a medium plan without capture: nothing launched yet -- the first adaptive_run decides between
        int single_step = 0;           // the single-launch kernel (budget covers the run; k_small_adapt, or k_medium_adapt on one XCD) and the chunked engine
        T phi_max = 0;
    } ar;
    // ---- z-resolved capture of an adaptive run that keeps the run's engine (ssfm_adaptive_set_capture, round 6).  The reference's own consumer calls FIBER with
    // h = None and return_steps (devices.py:2342); ssfm_adaptive_run(snapshots) reproduces that with three launches per step and a host wait per step.  Here the run
    // keeps its engine (two launches per step, fused, where the plan has it) and a capture step ADDS a launch: k_time<TM_END> behind the step's row pass reads
    // the half-transformed field and writes that step's time-order field into a slot of a ring of plan-owned device blocks (as ssfm_propagate_fixed_capture does);
    // the step number is the host's when it enqueues, the step SIZE the device's (cur[step & 1]: what the fused column launch behind it uses), a launch queued
    // behind the end of the run finds `done` and leaves.  An adaptive run is queued in chunks with a look at the state in between (that look exists anyway):
    // a chunk's snapshots go to one half of the ring and travel to the host on a stream of their own while the next chunk runs into the other half.
    struct AdaptCap {
        bool on = false;
        CapCursor cur;                 // which steps capture, how many snapshots are out, which half of the ring is next (ssfm_capture.hpp)
        std::vector<int64_t> list;     // the cursor's list: ascending step numbers (1-based: the field AFTER step s)
        char* host = nullptr;
        int64_t* taken = nullptr;      // step number of every snapshot written
        int64_t* n_taken = nullptr;
    } acap;
    Event acap_ev[2];      // behind the transfers of the chunk that used half 0 / 1 of the ring (the host waits for it before that half is written again)
    int adaptive_set_capture(int64_t every, const int64_t* steps, int64_t n_steps, void* fields_host, int64_t capacity, int64_t* taken, int64_t* n_taken) {
        if (!ar.active) return fail(SSFM_ERR_STATE, "ssfm_adaptive_set_capture: call ssfm_adaptive_begin first");
        if (ar.step != 0 || (ar.deferred == ADAPT_CHUNKED && ar.now.steps != 0)) return fail(SSFM_ERR_STATE, "ssfm_adaptive_set_capture: the run has started");
        if ((every > 0) == (steps != nullptr && n_steps > 0)) return fail(SSFM_ERR_INVALID, "ssfm_adaptive_set_capture: either a stride or a list of step numbers");
        if (!fields_host || capacity < 1 || !taken || !n_taken) return fail(SSFM_ERR_INVALID, "ssfm_adaptive_set_capture: NULL argument");
        if (int rc = no_split("ssfm_adaptive_set_capture")) return rc;
        if (int rc = use_device()) return rc;
        acap = AdaptCap();
        if (every <= 0) {
            if (!acap_list_valid(steps, n_steps)) return fail(SSFM_ERR_INVALID, "ssfm_adaptive_set_capture: step numbers must ascend from 1");
            acap.list.assign(steps, steps + n_steps);
            acap.cur.list = acap.list.data(); acap.cur.n_list = acap.list.size();
        }
        acap.on = true; acap.cur.every = every > 0 ? every : 0; acap.cur.capacity = capacity; acap.cur.half_slots = acap_half_slots(field_bytes());
        acap.host = static_cast<char*>(fields_host); acap.taken = taken; acap.n_taken = n_taken;
        *n_taken = 0;
        const size_t need = acap_ring_bytes(field_bytes());          // the ring: two halves (ssfm_capture.hpp)
        if (cap_block_bytes * (size_t)cap_nblocks < need) {
            cap_blocks.free(); cap_block_bytes = 0; cap_nblocks = 0;
            HIP_TRY(cap_blocks.reserve(need));
            cap_block_bytes = need; cap_nblocks = 1;
        }
        if (int rc = ensure_cap_stream()) return rc;
        for (auto& e : acap_ev) if (!e) HIP_TRY(hipEventCreateWithFlags(e.out(), hipEventDisableTiming));
        if (ar.deferred != ADAPT_CHUNKED) {            // (a small plan: the capture needs the launch-per-pass engine)
            const AdaptRun keep = ar;
            if (int rc = adaptive_begin_chunked(keep.gamma, keep.length, keep.phi_max, keep.single_step, keep.max_steps, 0)) return rc;
        }
        return SSFM_OK;
    }

    void adaptive_reset(T gamma, T length, T phi_max, int single_step, int max_steps) {
        ar = AdaptRun();
        ar.active = true; ar.gamma = gamma; ar.length = length; ar.phi_max = phi_max; ar.single_step = single_step; ar.max_steps = max_steps;
    }
    int adaptive_begin(double gamma_d, double length, double phi_max, int single_step, int64_t max_steps, int capture) {
        if (!have_op) return fail(SSFM_ERR_STATE, "ssfm_propagate_adaptive: call ssfm_set_linear_operator first");
        if (max_steps < 1 || max_steps > (1ll << 30)) return fail(SSFM_ERR_INVALID, "ssfm_propagate_adaptive: max_steps=%lld", (long long)max_steps);
        if (int rc = use_device()) return rc;
        const T gamma = (T)gamma_d;
        if (int rc = ensure_zlog(max_steps)) return rc;
        last_launches = 0;
        last_fell_back = 0;
        last_engine = SSFM_ENGINE_NONE;
        acap.on = false;
        HIP_TRY(hipEventRecord(ev0, stream));
        const AdaptBegin route = adaptive_route<T>(shape, AdaptSwitches{medium_ok, medium_adapt_ok, fused_ok, twA != nullptr, medium_shape(N1, N2)}, capture != 0, single_step != 0);
        if (route == ADAPT_CHUNKED) return adaptive_begin_chunked(gamma, (T)length, (T)phi_max, single_step, (int)max_steps, capture);
        adaptive_reset(gamma, (T)length, (T)phi_max, single_step, (int)max_steps);
        ar.deferred = route;
        return SSFM_OK;
    }
    AdaptState<T> adapt_host;          // staging copy of the run's parameters (a member: the copy below is asynchronous)
    // what the host reads back during an adaptive run (the step state, the give-up word) lands in page-locked memory: a transfer of a few bytes into
    // pageable memory goes through the runtime's staging path (measured per look at the state: profiles/r05_adaptive_looks.txt)
    struct AdaptLook { StepState<T> now; unsigned gave_up; unsigned pad[3]; };
    PinnedBuffer<AdaptLook> adapt_look;
    int ensure_adapt_look() { HIP_TRY(adapt_look.reserve(sizeof(AdaptLook))); return SSFM_OK; }
    int upload_adapt_state(T gamma, T length, T phi_max, int max_steps) {
        std::memset(&adapt_host, 0, sizeof(adapt_host));
        adapt_host.length = length;
        adapt_host.phi_max = phi_max;
        adapt_host.abs_gamma = gamma < 0 ? -gamma : gamma;
        adapt_host.adaptive = 1;
        adapt_host.max_steps = max_steps;
        adapt_host.patience = 2000000ll;
        if (const char* e = std::getenv("SSFM_FUSED_PATIENCE_TICKS")) adapt_host.patience = std::atoll(e);
        HIP_TRY(hipMemcpyAsync(st, &adapt_host, sizeof(adapt_host), hipMemcpyHostToDevice, stream));
        return SSFM_OK;
    }
    int adaptive_begin_chunked(T gamma, T length, T phi_max, int single_step, int max_steps, int capture) {
        if (int rc = ensure_sub()) return rc;
        if (is_split()) if (int rc = split_fly_ready()) return rc;
        if (int rc = upload_adapt_state(gamma, length, phi_max, max_steps)) return rc;
        if (!single_step) {
            hipLaunchKernelGGL(k_absmax<T>, dim3(1024), dim3(256), 0, stream, (const cx<T>*)F, (long long)n * batch, st);
            ++last_launches;
        }
        hipLaunchKernelGGL(k_step_control<T>, dim3(1), dim3(64), 0, stream, st, zlog, 0, single_step, 0);
        ++last_launches;
        HIP_TRY(hipGetLastError());
        // the first step size comes back at once: it tells how many steps to queue before the first look at the state
        // (a run of a few dozen steps is then two or three chunks, not five: every look is a 25 us stall)
        if (int rc = ensure_adapt_look()) return rc;
        HIP_TRY(hipMemcpyAsync(&adapt_look->now, reinterpret_cast<const char*>(st.get()) + offsetof(AdaptState<T>, cur), sizeof(StepState<T>), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        adaptive_reset(gamma, length, phi_max, single_step, max_steps);
        ar.now = adapt_look->now;
        // the column pass: fused where the whole grid is resident at once (ssfm_route.hpp adaptive_piece; the CU count only matters to grids beyond kAdaptSlots)
        int cus = 0;
        if (adaptive_col_blocks<T>(shape) > kAdaptSlots && hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) cus = 0;
        const AdaptPiece piece = adaptive_piece<T>(shape, fused_ok, capture != 0, cus);
        ar.fused = piece.fused; ar.tile_private = piece.tile_private;
        if (ar.fused) if (int rc = backup_field()) return rc;
        return SSFM_OK;
    }

    // Up to `budget` more steps.  snapshots != NULL: HOST buffer of `budget` fields, the field after each step taken by
    // this call (the caller captured the input itself); the run then synchronises after every step.
    int adaptive_run(int64_t budget, void* snapshots, int64_t* steps_total, int* done) {
        if (!ar.active) return fail(SSFM_ERR_STATE, "ssfm_adaptive_run: no adaptive run in progress");
        if (budget < 1) return fail(SSFM_ERR_INVALID, "ssfm_adaptive_run: budget=%lld", (long long)budget);
        if (int rc = use_device()) return rc;
        int engine = last_engine;              // (a call that finds the run at its end takes no step and leaves the report as it is)
        bool finished = false;                 // the whole run went in one launch
        if (ar.deferred != ADAPT_CHUNKED) {
            if (snapshots != nullptr) return fail(SSFM_ERR_STATE, "ssfm_adaptive_run: the run was not begun with capture");
            const AdaptRun keep = ar;
            if (adaptive_one_launch(keep.deferred, budget, keep.max_steps)) {
                if (int rc = keep.deferred == ADAPT_DEFER_MEDIUM ? run_deferred_medium(keep) : run_deferred_small(keep)) return rc;
                finished = ar.deferred == ADAPT_CHUNKED;
                if (finished) engine = adaptive_engine(keep.deferred);
            }
            // a budgeted caller (one that takes the run in pieces), or a medium run part of whose grid never ran beside the rest: the chunked engine from the start
            if (!finished) if (int rc = adaptive_begin_chunked(keep.gamma, keep.length, keep.phi_max, keep.single_step, keep.max_steps, 0)) return rc;
        }
        if (!finished) if (int rc = adaptive_chunks(budget, snapshots, &engine)) return rc;
        last_engine = engine;
        if (steps_total) *steps_total = ar.now.steps;
        if (done) *done = ar.now.done;
        return SSFM_OK;
    }
    // ---- the deferred run in one launch.  ar.deferred stays as it is where the launch's workgroups did not all meet: the field is the input again
    // a small plan (k_small_adapt); the state and the z log are read once, here
    int run_deferred_small(const AdaptRun& keep) {
        if (int rc = upload_adapt_state(keep.gamma, keep.length, keep.phi_max, keep.max_steps)) return rc;
        SmallAdaptArgs<T> sa;
        sa.F = F; sa.D = dsmall; sa.tw = tw_small; sa.st = st; sa.zlog = zlog; sa.gamma = keep.gamma; sa.inv_n = inv_n(); sa.single_step = keep.single_step;
        ++last_launches;
        HIP_TRY(launch_small_adapt<T>((int)n, batch, stream, sa));
        HIP_TRY(hipMemcpyAsync(&ar.now, reinterpret_cast<const char*>(st.get()) + offsetof(AdaptState<T>, cur), sizeof(ar.now), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        ar.deferred = ADAPT_CHUNKED;
        return SSFM_OK;
    }
    // a medium plan, on one XCD (k_medium_adapt); the input is kept for the case that its workgroups do not all get to run
    int run_deferred_medium([[maybe_unused]] const AdaptRun& keep) {
        if constexpr (sizeof(T) == 4) {
            if (int rc = backup_field()) return rc;
            if (int rc = upload_adapt_state(keep.gamma, keep.length, keep.phi_max, keep.max_steps)) return rc;
            hipLaunchKernelGGL(k_absmax<T>, dim3(1024), dim3(256), 0, stream, (const cx<T>*)F, (long long)n * batch, st);
            hipLaunchKernelGGL(k_step_control<T>, dim3(1), dim3(64), 0, stream, st, zlog, 0, 0, 0);
            last_launches += 2;
            MediumAdaptArgs<T> ma;                              // (no memset: the struct has no padding and every member is assigned)
            if (int rc = medium_prepare(ma, batch, 1)) return rc;        // (one launch for all rows: the first set of meeting words)
            ma.D = dperm; ma.st = st; ma.zlog = zlog;
            ma.gamma = keep.gamma; ma.inv_n = inv_n();
            ++last_launches;
            HIP_TRY(launch_medium_adapt(N1, N2, (int)ma.nblk, medium_xccs, stream, ma));
            unsigned gave_up[2] = {0u, 0u};
            if (int rc = medium_adapt_verdict(ma, gave_up, &ar.now)) return rc;
            if (!gave_up[0] && !gave_up[1]) { ar.deferred = ADAPT_CHUNKED; return SSFM_OK; }
            // part of the grid never ran beside the rest: the same run on the chunked engine, which this plan then keeps to
            medium_gave_up(medium_adapt_ok);
            HIP_TRY(hipMemcpyAsync(F, fused_backup, field_bytes(), hipMemcpyDeviceToDevice, stream));
        }
        return SSFM_OK;
    }
    // ---- the chunked engine: up to `budget` more steps, queued in chunks with a look at the state in between
    int adaptive_estimate() const { return chunk_estimate((double)ar.length - (double)ar.now.z, (double)ar.now.h, kAdaptChunkMax, true); }
    int adaptive_chunks(int64_t budget, void* snapshots, int* engine) {
        const AdaptPiece piece = adaptive_in_pieces(AdaptPiece{ar.fused, ar.tile_private}, shape, ar.step, budget, ar.max_steps);
        ar.fused = piece.fused; ar.tile_private = piece.tile_private;
        const size_t fb = field_bytes();
        char* snap = static_cast<char*>(snapshots);
        if (snap && ar.tile_private) return fail(SSFM_ERR_STATE, "ssfm_adaptive_run: the run was not begun with capture");
        const int first_step = ar.now.steps;
        int chunk = snap ? 1 : adaptive_estimate();
        const bool fly_imag = !is_split() && fly_imag_ready();
        if (acap.on && snap) return fail(SSFM_ERR_STATE, "ssfm_adaptive_run: either ssfm_adaptive_set_capture or `snapshots`");
        while (!ar.now.done && ar.now.steps - first_step < budget) {
            *engine = adaptive_engine(shape, ar.fused);
            chunk = chunk_next(chunk, budget - (ar.now.steps - first_step), acap.on ? acap.cur.every : 0, ar.step);
            // a capture run: this chunk's snapshots go to one half of the ring, whose transfers of two chunks ago are waited for ON THE HOST
            std::vector<int64_t> chunk_caps;
            char* ring_half = nullptr;
            if (acap.on) {
                if (acap.cur.half_in_use()) HIP_TRY(hipEventSynchronize(acap_ev[acap.cur.half()]));
                ring_half = cap_blocks + acap.cur.half_offset(fb);
            }
            if (int rc = adaptive_enqueue_chunk(chunk, fly_imag, ring_half, chunk_caps)) return rc;
            const int before = ar.now.steps;
            unsigned gave_up = 0u;
            if (int rc = adaptive_look(&gave_up)) return rc;
            if (acap.on && !(ar.fused && gave_up)) if (int rc = adaptive_send_snapshots(chunk_caps, ring_half)) return rc;
            if (ar.fused && gave_up) {
                if (int rc = adaptive_fall_back()) return rc;
                chunk = adaptive_estimate();
                continue;
            }
            if (snap && ar.now.steps == before + 1) {        // (chunk = 1: the step just launched was really taken)
                ran();
                if (int rc = copy_field_out(snap + fb * (size_t)(before - first_step), false, true)) return rc;
            }
            if (!snap && !ar.now.done) chunk = adaptive_estimate();       // do not queue far beyond the end
        }
        return SSFM_OK;
    }
    // enqueue one chunk: `chunk` steps from ar.step on (fewer where a capture fills its half of the ring: `chunk` then says how many)
    int adaptive_enqueue_chunk(int& chunk, bool fly_imag, char* ring_half, std::vector<int64_t>& chunk_caps) {
        const size_t fb = field_bytes();
        for (int i = 0; i < chunk; ++i, ++ar.step) {
            TimeArgs<T> tb = targs(ar.gamma, 0, 0, st), te = tb;
            tb.step = te.step = ar.step;
            tb.derive = i != 0;         // the first BEGIN of a chunk finds its state in cur[] (k_step_control wrote it)
            if (ar.fused) {
                // BEGIN once; then FREQ + MID_A per step (MID_A(s) leaves the state of step s + 1 in cur[(s + 1) & 1])
                if (ar.step == 0) { tb.derive = 0; HIP_TRY((launch_time<T, TM_BEGIN>(N1, batch, stream, tb, E))); ++last_launches; }
            } else if (ar.tile_private && ar.step > 0) HIP_TRY((launch_time<T, TM_BEGIN_Y>(N1, batch, stream, tb, E)));
            else HIP_TRY((launch_time<T, TM_BEGIN>(N1, batch, stream, tb, E)));
            FreqArgs<T> fa = fargs_fly(0, st);
            fa.step = ar.step;
            if (is_split()) {
                HIP_TRY(split_freq(nullptr, 0, st, ar.step, 0, batch, stream));
                last_launches += 2;
            } else
            if (fly_imag) {           // (half the operator's bytes: 23.7 -> 22.6 us per step at 2^20 x 2, the same bits)
                fa.tab = reinterpret_cast<const cx<T>*>(dimag_fly.get()); fa.amp = op_re0;
                HIP_TRY((launch_freq<T, FM_FLY_IM>(N2, N1 * batch, stream, fa, Ef_fly)));
            } else
            HIP_TRY((launch_freq<T, FM_FLY>(N2, N1 * batch, stream, fa, Ef_fly)));
            if (acap.on && acap.cur.wants((int64_t)ar.step + 1) && acap.cur.room(chunk_caps.size())) {
                // the capture step's extra launch: this step's time-order field into a ring slot (the step size is the device's: cur[step & 1])
                TimeArgs<T> tc = te;
                tc.F = reinterpret_cast<cx<T>*>(ring_half + fb * chunk_caps.size());
                HIP_TRY((launch_time<T, TM_END>(N1, batch, stream, tc, E)));
                ++last_launches;
                chunk_caps.push_back((int64_t)ar.step + 1);
                if (acap.cur.cut(chunk_caps.size(), i)) chunk = i + 1;          // (the half is full / enough to send: look at the state)
            }
            if (ar.fused) HIP_TRY((launch_time<T, TM_MID_A>(N1, batch, stream, te, E)));
            else if (ar.tile_private) HIP_TRY((launch_time<T, TM_END_Y>(N1, batch, stream, te, E)));
            else HIP_TRY((launch_time<T, TM_END>(N1, batch, stream, te, E)));
            last_launches += ar.fused ? 2 : 3;
        }
        return SSFM_OK;
    }
    // look at the state: where the run stands after the last launched step, for the host (and for the first BEGIN of the next chunk); waits for the chunk
    int adaptive_look(unsigned* gave_up) {
        if (!ar.fused) {
            hipLaunchKernelGGL(k_step_control<T>, dim3(1), dim3(64), 0, stream, st, zlog, 1, 0, ar.step);
            ++last_launches;
        }
        adapt_look->gave_up = 0u;
        HIP_TRY(hipMemcpyAsync(&adapt_look->now, reinterpret_cast<const char*>(st.get()) + offsetof(AdaptState<T>, cur) + sizeof(StepState<T>) * (ar.step & 1),
                               sizeof(StepState<T>), hipMemcpyDeviceToHost, stream));
        if (ar.fused) HIP_TRY(hipMemcpyAsync(&adapt_look->gave_up, reinterpret_cast<const char*>(st.get()) + offsetof(AdaptState<T>, error), sizeof(unsigned), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        ar.now = adapt_look->now; *gave_up = adapt_look->gave_up;
        return SSFM_OK;
    }
    // send the chunk's snapshots: the chunk has run (the look waited for it), its snapshots of steps really taken leave for the host beside the next chunk
    int adaptive_send_snapshots(const std::vector<int64_t>& chunk_caps, const char* ring_half) {
        const size_t fb = field_bytes();
        const size_t taken = caps_taken(chunk_caps.data(), chunk_caps.size(), ar.now.steps);      // (the rest was queued behind the end of the run: never written)
        for (size_t k = 0; k < taken; ++k) {
            HIP_TRY(hipMemcpyAsync(acap.host + fb * (size_t)(acap.cur.count + k), ring_half + fb * k, fb, hipMemcpyDeviceToHost, cap_stream));
            acap.taken[acap.cur.count + k] = chunk_caps[k];
        }
        *acap.n_taken = acap.cur.count + (int64_t)taken;
        HIP_TRY(hipEventRecord(acap_ev[acap.cur.half()], cap_stream));
        acap.cur.sent((int64_t)taken);
        return SSFM_OK;
    }
    // fall back from fused: the grid did not run as a whole (another job holds CUs) -- the same run again on the three-launch engine
    int adaptive_fall_back() {
        const AdaptRun keep = ar;
        if (acap.on) { HIP_TRY(hipStreamSynchronize(cap_stream)); acap.cur.reset(); *acap.n_taken = 0; }
        fused_ok = false;
        last_fell_back = 1;
        ++fallbacks;
        HIP_TRY(hipMemcpyAsync(F, fused_backup, sizeof(cx<T>) * n * batch, hipMemcpyDeviceToDevice, stream));
        return adaptive_begin_chunked(keep.gamma, keep.length, keep.phi_max, keep.single_step, keep.max_steps, 0);
    }

    int adaptive_finish(int64_t* steps_out, double* z_out) {
        if (!ar.active) return fail(SSFM_ERR_STATE, "ssfm_adaptive_finish: no adaptive run in progress");
        if (int rc = use_device()) return rc;
        if (ar.deferred != ADAPT_CHUNKED) {           // finished before any step was asked for: the chunked engine's begin leaves the same state behind
            const AdaptRun keep = ar;
            if (int rc = adaptive_begin_chunked(keep.gamma, keep.length, keep.phi_max, keep.single_step, keep.max_steps, 0)) return rc;
        }
        ar.active = false;
        if (acap.on) { HIP_TRY(hipStreamSynchronize(cap_stream)); acap.on = false; }          // (the caller's snapshots are complete)
        if (ar.tile_private && ar.now.steps > 0) {
            HIP_TRY((launch_time<T, TM_UNPACK>(N1, batch, stream, targs(ar.gamma, 0, 0, nullptr), E)));      // Y buffer -> time-order field
            ++last_launches;
        }
        if (ar.now.steps > 0) ran();
        if (int rc = publish_if_external()) return rc;
        HIP_TRY(hipEventRecord(ev1, stream));
        timed = true;
        if (steps_out) *steps_out = ar.now.steps;
        if (z_out) {
            std::vector<T> zl(ar.now.steps + 1);
            HIP_TRY(hipMemcpyAsync(zl.data(), zlog, sizeof(T) * (ar.now.steps + 1), hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipStreamSynchronize(stream));
            for (int i = 0; i <= ar.now.steps; ++i) z_out[i] = (double)zl[i];
        }
        HIP_TRY(hipStreamSynchronize(stream));
        if (!(ar.now.z >= ar.length) && ar.now.steps >= ar.max_steps)
            return fail(SSFM_ERR_INVALID, "ssfm_propagate_adaptive: max_steps=%lld reached at z=%g of %g km",
                        (long long)ar.max_steps, (double)ar.now.z, (double)ar.length);
        return SSFM_OK;
    }

    int propagate_adaptive(double gamma_d, double length, double phi_max, int single_step, int64_t max_steps,
                           int64_t* steps_out, double* z_out, void* snapshots) {
        if (int rc = adaptive_begin(gamma_d, length, phi_max, single_step, max_steps, snapshots != nullptr)) return rc;
        char* snap = static_cast<char*>(snapshots);
        if (snap) if (int rc = copy_field_out(snap, false, true)) return rc;
        if (int rc = adaptive_run(max_steps, snap ? snap + sizeof(cx<T>) * n * batch : nullptr, nullptr, nullptr)) return rc;
        return adaptive_finish(steps_out, z_out);
    }

    // out = ifft(fft(x) * H): BEGIN/END with gamma = 0 are pure column transforms
    int apply_transfer(const void* H_host) {
        if (int rc = use_device()) return rc;
        const int nrows = N1 * batch;
        if (int rc = ensure_scratch()) return rc;
        cx<T>* hperm = scratch;   // n entries are enough (a split plan: n_full <= n * batch)
        // dnat is a staging buffer: the propagator's own D~ must be re-set after a DM call
        HIP_TRY(hipMemcpyAsync(dnat, H_host, sizeof(cx<T>) * n_full, hipMemcpyHostToDevice, stream));
        drop_operator();
        if (int rc = ensure_sub()) return rc;
        if (is_split())
            hipLaunchKernelGGL((k_make_split_table<T, 1>), dim3((unsigned)((n_full + 255) / 256)), dim3(256), 0, stream, (const cx<T>*)dnat, hperm, N1, N2, split_R, (T)0, inv_n_full(), split_qf());
        else
        hipLaunchKernelGGL((k_make_freq_table<T, 1>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream,
                           (const cx<T>*)dnat, hperm, N1, N2, N2 / Ef, (T)0, inv_n());
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(ev0, stream));
        HIP_TRY((launch_time<T, TM_BEGIN>(N1, batch, stream, targs(0, 0, 0, nullptr), E)));
        if (is_split()) HIP_TRY(split_freq(hperm, 0, nullptr, 0, 0, batch, stream));
        else
        HIP_TRY((launch_freq<T, FM_TABLE>(N2, nrows, stream, fargs(hperm, 0, nullptr), Ef)));
        HIP_TRY((launch_time<T, TM_END>(N1, batch, stream, targs(0, 0, 0, nullptr), E)));
        ran();
        if (int rc = publish_if_external()) return rc;
        HIP_TRY(hipEventRecord(ev1, stream));
        last_launches = is_split() ? 5 : 3;
        timed = true;
        HIP_TRY(hipStreamSynchronize(stream));   // H_host may be released by the caller
        return SSFM_OK;
    }

    int apply_dispersion(double dt_s, double D_s2, void* H_out) {
        if (int rc = use_device()) return rc;
        const int nrows = N1 * batch;
        if (int rc = ensure_scratch()) return rc;
        cx<T>* hperm = scratch;
        cx<T>* hnat = nullptr;
        if (H_out) {                       // dnat doubles as staging for the natural-order H
            hnat = dnat;
            drop_operator();
        }
        const double val = 1.0 / ((double)n_full * dt_s);
        if (int rc = ensure_sub()) return rc;
        if (is_split())
            hipLaunchKernelGGL(k_make_split_dm_table<T>, dim3((unsigned)((n_full + 255) / 256)), dim3(256), 0, stream, hperm, hnat, N1, N2, split_R, val, D_s2, inv_n_full(), split_qf());
        else
        hipLaunchKernelGGL(k_make_dm_table<T>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream,
                           hperm, hnat, N1, N2, N2 / Ef, val, D_s2, inv_n());
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(ev0, stream));
        HIP_TRY((launch_time<T, TM_BEGIN>(N1, batch, stream, targs(0, 0, 0, nullptr), E)));
        if (is_split()) HIP_TRY(split_freq(hperm, 0, nullptr, 0, 0, batch, stream));
        else
        HIP_TRY((launch_freq<T, FM_TABLE>(N2, nrows, stream, fargs(hperm, 0, nullptr), Ef)));
        HIP_TRY((launch_time<T, TM_END>(N1, batch, stream, targs(0, 0, 0, nullptr), E)));
        ran();
        if (int rc = publish_if_external()) return rc;
        HIP_TRY(hipEventRecord(ev1, stream));
        last_launches = is_split() ? 5 : 3;
        timed = true;
        if (H_out) {
            HIP_TRY(hipMemcpyAsync(H_out, hnat, sizeof(cx<T>) * n_full, hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipStreamSynchronize(stream));
        }
        return SSFM_OK;
    }

    // A transfer function kept on the device (slot 0 / 1), and its application x <- ifft(fft(x) * H) WITHOUT a
    // host synchronisation: the building block of the chirp-z path for sizes that are not powers of two.
    int transfer_table(const void* H_host, int slot) {
        if (slot < 0 || slot > 1) return fail(SSFM_ERR_INVALID, "ssfm_transfer_table: slot %d", slot);
        if (int rc = no_split("ssfm_transfer_table")) return rc;
        if (int rc = use_device()) return rc;
        if (int rc = ensure_xfer(slot)) return rc;
        HIP_TRY(hipMemcpyAsync(dnat, H_host, sizeof(cx<T>) * n, hipMemcpyHostToDevice, stream));      // dnat = staging
        drop_operator();
        tags[1 + slot] = 0;
        hipLaunchKernelGGL((k_make_freq_table<T, 1>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream,
                           (const cx<T>*)dnat, xfer_tab[slot], N1, N2, N2 / Ef, (T)0, inv_n());
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(stream));                  // H_host may be released by the caller
        return SSFM_OK;
    }
    // x <- ifft(fft(ifft(fft(x) * H0) * mul) * H1) with the tables of slots 0 and 1 and a time-domain table `mul` (n entries per row, DEVICE, the plan's
    // precision): the two applications of apply_table around a pointwise product, the middle of it -- inverse pass, product, forward pass -- in ONE column
    // launch (k_time<TM_MID> with TimeArgs::mul).  Five launches instead of seven.  Plain layout only (complex128 plans; complex64 plans of the plain layout).
    // `io` (nullable; complex128 plans): a chirp-z step's two ends folded into the first and the last launch (ChirpIO, ssfm_kernels.hpp) -- the caller's
    // field in, the caller's field out, the plan's own field buffer untouched.
    int apply_tables_mul(const void* mul_dev, const ssfm::ChirpStepIO* io = nullptr) {
        if (int rc = no_split("ssfm_apply_tables_mul")) return rc;
        if (!xfer_tab[0] || !xfer_tab[1]) return fail(SSFM_ERR_STATE, "ssfm_apply_tables_mul: slots 0 and 1 must hold tables");
        if (u16) return fail(SSFM_ERR_UNSUPPORTED, "ssfm_apply_tables_mul: not for plans in the 16-byte-unit layout");
        if (!mul_dev) return fail(SSFM_ERR_INVALID, "ssfm_apply_tables_mul: NULL table");
        TimeArgs<T> tb = targs(0, 0, 0, nullptr);
        if (io) {
            if (sizeof(T) != 8) return fail(SSFM_ERR_UNSUPPORTED, "ssfm_chirp_step: complex128 plans only");
            if (!io->A || !io->P || !io->chirp || io->n < 2 || 2 * io->n - 1 > n) return fail(SSFM_ERR_INVALID, "ssfm_chirp_step: bad field description");
            tb.cz.chirp = static_cast<const cx<T>*>(io->chirp); tb.cz.A = static_cast<cx<T>*>(io->A); tb.cz.P = static_cast<T*>(io->P); tb.cz.n = io->n;
            tb.cz.gamma = (T)io->gamma; tb.cz.hh = (T)io->hh; tb.cz.scale = (T)(1.0 / (double)io->n);
            tb.cz.h = static_cast<const double*>(io->h_dev); tb.cz.done = static_cast<const int*>(io->done_dev);
            tb.cz.maxbits = static_cast<unsigned long long*>(io->maxbits_dev);
        }
        if (int rc = use_device()) return rc;
        if (io) last_engine = SSFM_ENGINE_CHIRP_STEPS;
        if (io && (io->lean || io->c64_line)) {
            // Round 6 (the adaptive runs of long lines): the rows on the plan's lanes, the middle pass reads `n` table entries instead of the line's length, and -- a
            // complex64 caller -- the line holds complex64 values between the passes (chirp_line_run has the reasons and the numbers)
            const bool c64_line = io->c64_line != 0;
            if (c64_line && !line_half_ok()) return fail(SSFM_ERR_UNSUPPORTED, "ssfm_chirp_step: no complex64-storage passes for this plan");
            const int L = (nlanes > 1 && batch % nlanes == 0) ? nlanes : 1;
            const int rows = batch / L;
            auto row_ptr = [&](cx<T>* base, int row0) -> cx<T>* {
                return c64_line ? reinterpret_cast<cx<T>*>(reinterpret_cast<cx<float>*>(base) + (size_t)row0 * n) : base + (size_t)row0 * n;
            };
            auto time_launch = [&](auto mode_tag, const TimeArgs<T>& a, hipStream_t st) -> hipError_t {
                constexpr int MODE = decltype(mode_tag)::value;
                if constexpr (sizeof(T) == 8) { if (c64_line) return launch_time_h<MODE>(N1, rows, st, a, E); }
                return launch_time<T, MODE>(N1, rows, st, a, E);
            };
            auto freq_launch = [&](const cx<T>* tab, int g, hipStream_t st) -> hipError_t {
                FreqArgs<T> a = fargs(tab, 0, nullptr, g * rows, g);
                a.F = row_ptr(Y, g * rows);
                if constexpr (sizeof(T) == 8) { if (c64_line) return launch_freq_h(N2, N1 * rows, st, a, tb.cz.done); }
                return launch_freq<T, FM_TABLE>(N2, N1 * rows, st, a, Ef);
            };
            auto lane_st = [&](int g) { return L > 1 ? lane_stream[g] : stream; };
            auto ends = [&](int g) {
                TimeArgs<T> a = tb;
                a.F = row_ptr(F, g * rows); a.Y = row_ptr(Y, g * rows); a.P = P + (size_t)(g * rows) * n;
                a.cz.A = tb.cz.A + (size_t)(g * rows) * io->n; a.cz.P = tb.cz.P + (size_t)(g * rows) * io->n;
                return a;
            };
            if (L > 1) {
                HIP_TRY(hipEventRecord(fork_ev, stream));
                for (int g = 1; g < L; ++g) HIP_TRY(hipStreamWaitEvent(lane_stream[g], fork_ev, 0));
            }
            for (int g = 0; g < L; ++g) HIP_TRY(time_launch(std::integral_constant<int, TM_BEGIN>{}, ends(g), lane_st(g)));
            for (int g = 0; g < L; ++g) HIP_TRY(freq_launch(xfer_tab[0], g, lane_st(g)));
            for (int g = 0; g < L; ++g) {
                TimeArgs<T> tm = targs(0, 0, 0, nullptr, g * rows, g);
                tm.F = row_ptr(F, g * rows); tm.Y = row_ptr(Y, g * rows);
                tm.mul = static_cast<const cx<T>*>(mul_dev);
                tm.cz.done = tb.cz.done;
                if (io->lean) tm.keep = (int)io->n;
                HIP_TRY(time_launch(std::integral_constant<int, TM_MID>{}, tm, lane_st(g)));
            }
            for (int g = 0; g < L; ++g) HIP_TRY(freq_launch(xfer_tab[1], g, lane_st(g)));
            for (int g = 0; g < L; ++g) HIP_TRY(time_launch(std::integral_constant<int, TM_END>{}, ends(g), lane_st(g)));
            for (int g = 1; g < L; ++g) {
                HIP_TRY(hipEventRecord(lane_ev[g], lane_stream[g]));
                HIP_TRY(hipStreamWaitEvent(stream, lane_ev[g], 0));
            }
            last_launches += 5 * L;
            return SSFM_OK;
        }
        HIP_TRY((launch_time<T, TM_BEGIN>(N1, batch, stream, tb, E)));
        HIP_TRY((launch_freq<T, FM_TABLE>(N2, N1 * batch, stream, fargs(xfer_tab[0], 0, nullptr), Ef)));
        TimeArgs<T> tm = targs(0, 0, 0, nullptr);
        tm.mul = static_cast<const cx<T>*>(mul_dev);
        HIP_TRY((launch_time<T, TM_MID>(N1, batch, stream, tm, E)));
        HIP_TRY((launch_freq<T, FM_TABLE>(N2, N1 * batch, stream, fargs(xfer_tab[1], 0, nullptr), Ef)));
        HIP_TRY((launch_time<T, TM_END>(N1, batch, stream, tb, E)));
        last_launches += 5;
        return SSFM_OK;
    }
    // A fixed-step chirp-z run on the plan's line (plain layout), the field already there as A c, zero from `keep` up: the chirps on either side of a step
    // cancel against the neighbouring steps' (c conj(c) = 1; a rotation commutes with them), so a step is FOUR launches -- row pass (slot 0), column
    // pass with the table product (TM_MID_L, mul[which[s]]: exp(D~ h) / n below keep, zero above), row pass (slot 1), column pass with the second half
    // rotation of this step and the first of the next in one (the padding set to zero first) -- instead of the five of ssfm_chirp_step; the caller
    // multiplies by conj(c) when the run is over.
    // half: the line holds complex64 values between the passes (a complex64 caller's run; line_half_ok() says whether this plan has those kernels)
    bool line_half_ok() const { return sizeof(T) == 8 && !u16 && !is_split() && line_half_shape(N1, N2, E, Ef); }
    int chirp_line_run(const void* const* mul, const unsigned char* which, const double* hs, int64_t nsteps, double gamma_d, int64_t keep, int c64_line = 0) {
        if (int rc = no_split("chirp-z")) return rc;
        if (c64_line && !line_half_ok()) return fail(SSFM_ERR_UNSUPPORTED, "ssfm_chirp_line_run: no complex64-storage passes for this plan");
        if (!xfer_tab[0] || !xfer_tab[1]) return fail(SSFM_ERR_STATE, "ssfm_chirp_line_run: slots 0 and 1 must hold tables");
        if (u16) return fail(SSFM_ERR_UNSUPPORTED, "ssfm_chirp_line_run: not for plans in the 16-byte-unit layout");
        if (!mul || !which || !hs || nsteps < 1 || keep < 2 || keep > n) return fail(SSFM_ERR_INVALID, "ssfm_chirp_line_run: bad arguments");
        for (int64_t s = 0; s < nsteps; ++s)
            if (!mul[which[s]]) return fail(SSFM_ERR_INVALID, "ssfm_chirp_line_run: step %lld has no table", (long long)s);
        if (int rc = use_device()) return rc;
        const T gamma = (T)gamma_d, half = (T)0.5;
        // Round 6: the rows go out on the plan's LANES (one stream per half of the rows, as the fixed-step run of a power of two does) -- a column pass is bound by
        // latencies (one wavefront per SIMD in complex128), a row pass by bytes, and side by side they fill each other's gaps: 2^22-point rows x 2, complex128,
        // 176 us per step in one launch per pass against 149 on two lanes (tools/big_n_c128.py).  SSFM_LANES=1: one launch per pass as before.
        const int L = (nlanes > 1 && batch % nlanes == 0) ? nlanes : 1;
        const int rows = batch / L;
        // (c64_line: the field buffers hold complex64 values -- a row starts `n` float pairs after the one before)
        auto row_ptr = [&](cx<T>* base, int row0) -> cx<T>* {
            return c64_line ? reinterpret_cast<cx<T>*>(reinterpret_cast<cx<float>*>(base) + (size_t)row0 * n) : base + (size_t)row0 * n;
        };
        auto TA = [&](T g_, T hp, T hn, int g) {
            TimeArgs<T> a = targs(g_, hp, hn, nullptr, g * rows, g);
            a.F = row_ptr(F, g * rows); a.Y = row_ptr(Y, g * rows);
            return a;
        };
        auto FA = [&](const cx<T>* tab, int g) {
            FreqArgs<T> a = fargs(tab, 0, nullptr, g * rows, g);
            a.F = row_ptr(Y, g * rows);
            return a;
        };
        auto time_launch = [&](auto mode_tag, const TimeArgs<T>& a, hipStream_t st) -> hipError_t {
            constexpr int MODE = decltype(mode_tag)::value;
            if constexpr (sizeof(T) == 8) { if (c64_line) return launch_time_h<MODE>(N1, rows, st, a, E); }
            return launch_time<T, MODE>(N1, rows, st, a, E);
        };
        auto freq_launch = [&](const FreqArgs<T>& a, hipStream_t st) -> hipError_t {
            if constexpr (sizeof(T) == 8) { if (c64_line) return launch_freq_h(N2, N1 * rows, st, a); }
            return launch_freq<T, FM_TABLE>(N2, N1 * rows, st, a, Ef);
        };
        auto lane_st = [&](int g) { return L > 1 ? lane_stream[g] : stream; };
        if (L > 1) {
            HIP_TRY(hipEventRecord(fork_ev, stream));
            for (int g = 1; g < L; ++g) HIP_TRY(hipStreamWaitEvent(lane_stream[g], fork_ev, 0));
        }
        for (int g = 0; g < L; ++g) HIP_TRY(time_launch(std::integral_constant<int, TM_BEGIN>{}, TA(gamma, (T)0, (T)hs[0] * half, g), lane_st(g)));
        for (int64_t s = 0; s < nsteps; ++s) {
            for (int g = 0; g < L; ++g) HIP_TRY(freq_launch(FA(xfer_tab[0], g), lane_st(g)));
            for (int g = 0; g < L; ++g) {
                TimeArgs<T> tl = TA((T)0, (T)0, (T)0, g);
                tl.mul = static_cast<const cx<T>*>(mul[which[s]]);
                tl.keep = (int)keep;
                HIP_TRY(time_launch(std::integral_constant<int, TM_MID_L>{}, tl, lane_st(g)));
            }
            for (int g = 0; g < L; ++g) HIP_TRY(freq_launch(FA(xfer_tab[1], g), lane_st(g)));
            for (int g = 0; g < L; ++g) {
                if (s + 1 < nsteps) {
                    TimeArgs<T> tm = TA(gamma, (T)hs[s] * half, (T)hs[s + 1] * half, g);
                    tm.keep = (int)keep;
                    HIP_TRY(time_launch(std::integral_constant<int, TM_MID>{}, tm, lane_st(g)));
                } else {
                    HIP_TRY(time_launch(std::integral_constant<int, TM_END>{}, TA(gamma, (T)hs[s] * half, (T)0, g), lane_st(g)));
                }
            }
        }
        for (int g = 1; g < L; ++g) {
            HIP_TRY(hipEventRecord(lane_ev[g], lane_stream[g]));
            HIP_TRY(hipStreamWaitEvent(stream, lane_ev[g], 0));
        }
        last_launches += (1 + 4 * nsteps) * L;
        last_engine = SSFM_ENGINE_CHIRP_STEPS;
        last_fell_back = 0;
        return SSFM_OK;
    }
    // A fixed-step chirp-z run of a field of nn <= n / 2 samples per row in ONE launch (k_small_chirp); SSFM_ERR_UNSUPPORTED (nothing launched) when the
    // plan is not a complex128 plan of the one-workgroup-per-row engine.
    int chirp_small(void* A, const void* chirp, const void* Dt, int64_t nn, double gamma, const double* hs, int64_t nsteps) {
        if (int rc = no_split("chirp-z")) return rc;
        if (!small || !tw_small || n > 4096) return fail(SSFM_ERR_UNSUPPORTED, "ssfm_chirp_small: a plan of 256 ... 4096 samples is needed");
        if (!A || !chirp || !Dt || !hs || nn < 2 || 2 * nn - 1 > n || nsteps < 1 || nsteps > 0x7fffffff) return fail(SSFM_ERR_INVALID, "ssfm_chirp_small: bad arguments");
        {
            const Schedule<double> sch(hs, nsteps, kMaxTables);           // (the kernel takes the sizes as float64, whatever the plan's precision)
            if (!sch.valid()) return fail(SSFM_ERR_INVALID, "ssfm_chirp_small: step %lld is %g km (must be finite and > 0)", (long long)sch.first_bad, hs[sch.first_bad]);
        }
        if (int rc = use_device()) return rc;
        const size_t need = sizeof(double) * (size_t)nsteps;
        if (int rc = grow(d_hs, need, need / 2)) return rc;
        HIP_TRY(hipStreamSynchronize(stream));
        HIP_TRY(hipMemcpyAsync(d_hs, hs, need, hipMemcpyHostToDevice, stream));
        HIP_TRY(hipStreamSynchronize(stream));             // (hs is the caller's)
        SmallChirpArgs<T> a;
        a.A = static_cast<cx<T>*>(A); a.chirp = static_cast<const cx<T>*>(chirp); a.Dt = static_cast<const cx<T>*>(Dt); a.hs = reinterpret_cast<const double*>(d_hs.get());
        if (int rc = chirp_line_table(&a.tw)) return rc;
        a.gamma = (T)gamma; a.n = (int)nn; a.nsteps = (int)nsteps;
        last_launches = 1;
        last_engine = SSFM_ENGINE_CHIRP_SMALL; last_fell_back = 0;
        HIP_TRY(launch_small_chirp<T>((int)n, batch, stream, a));
        return SSFM_OK;
    }
    // ... and the adaptive run (k_small_chirp_adapt): the rows' workgroups exchange their maxima through memory every step, so all of them must be
    // resident at once (at most kChirpAdaptRows rows).  Synchronous: the z log and the step count come back.
    int chirp_line_table(const cx<T>** tw) {
        *tw = tw_small.get();
        if (chirp_points<T>((int)n) == small_points<T>((int)n)) return SSFM_OK;
        if (!tw_chirp)
            if (int rc = make_line_table(&tw_chirp, (int)n, chirp_points<T>((int)n))) return rc;
        *tw = tw_chirp.get();
        return SSFM_OK;
    }
    static constexpr int kChirpAdaptRows = 16;
    int chirp_small_adapt(void* A, const void* chirp, const void* Dt, int64_t nn, double gamma, double length, double phi_max, int f32, int64_t max_steps,
                          double* z_out, int64_t* steps_out) {
        if (!small || !tw_small || n > 4096 || batch > kChirpAdaptRows)
            return fail(SSFM_ERR_UNSUPPORTED, "ssfm_chirp_small_adapt: a plan of 256 ... 4096 samples and at most %d rows is needed", kChirpAdaptRows);
        if (!A || !chirp || !Dt || nn < 2 || 2 * nn - 1 > n || max_steps < 1 || max_steps > 0x7ffffff0 || !(length > 0) || !(phi_max > 0) || gamma == 0.0)
            return fail(SSFM_ERR_INVALID, "ssfm_chirp_small_adapt: bad arguments");
        if (int rc = use_device()) return rc;
        const size_t words = 2 * (size_t)batch * 2, need = sizeof(double) * (size_t)(max_steps + 1) + 8 * words + 16;
        if (int rc = grow(d_hs, need, need / 2)) return rc;
        unsigned char* base = reinterpret_cast<unsigned char*>(d_hs.get());
        SmallChirpAdaptArgs<T> a;
        a.A = static_cast<cx<T>*>(A); a.chirp = static_cast<const cx<T>*>(chirp); a.Dt = static_cast<const cx<T>*>(Dt);
        if (int rc = chirp_line_table(&a.tw)) return rc;
        a.xw = reinterpret_cast<unsigned long long*>(base); a.out = reinterpret_cast<int*>(base + 8 * words); a.zlog = reinterpret_cast<double*>(base + 8 * words + 16);
        a.phi_max = phi_max; a.abs_gamma = gamma < 0 ? -gamma : gamma; a.length = length; a.patience = medium_patience;
        a.gamma = (T)gamma; a.n = (int)nn; a.max_steps = (int)max_steps; a.f32 = f32;
        HIP_TRY(hipMemsetAsync(base, 0, 8 * words + 16, stream));
        // the caller's field is kept (a few dozen KiB): rows that had finished when another row's workgroup gave up have stored their result
        void* keep = nullptr;
        const size_t fbytes = sizeof(cx<T>) * (size_t)nn * (size_t)batch;
        if (int rc = workspace(3, fbytes, &keep)) return rc;
        HIP_TRY(hipMemcpyAsync(keep, A, fbytes, hipMemcpyDeviceToDevice, stream));
        last_launches = 1;
        last_engine = SSFM_ENGINE_CHIRP_SMALL_ADAPT; last_fell_back = 0;
        HIP_TRY(launch_small_chirp_adapt<T>((int)n, batch, stream, a));
        int out[3] = {0, 0, 0};
        HIP_TRY(hipMemcpyAsync(out, a.out, sizeof(out), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        if (out[1]) {
            // a busy device: not all rows' workgroups were resident together.  The field is put back as it came (rows that had finished have
            // stored theirs) and the caller's other path can run -- as every other single-launch engine of this library does
            if (out[2] != 0) {
                HIP_TRY(hipMemcpyAsync(A, keep, fbytes, hipMemcpyDeviceToDevice, stream));
                HIP_TRY(hipStreamSynchronize(stream));
            }
            ++fallbacks;
            last_fell_back = 1;
            return fail(SSFM_ERR_UNSUPPORTED, "ssfm_chirp_small_adapt: the rows' workgroups did not meet within the patience; the field is unchanged");
        }
        if (z_out) HIP_TRY(hipMemcpy(z_out, a.zlog, sizeof(double) * (size_t)(out[0] + 1), hipMemcpyDeviceToHost));
        if (steps_out) *steps_out = out[0];
        return SSFM_OK;
    }
    // Can this plan run the one-launch chirp-z engine of 2048 < nn <= n / 2 samples (chirp_medium / chirp_medium_adapt below)?  If so, slots 0 and 1
    // hold the two convolutions' transfer functions for that length when this returns.
    int chirp_medium_tables(int64_t nn) {
        if (int rc = no_split("chirp-z")) return rc;
        if constexpr (sizeof(T) != 4) { (void)nn; return fail(SSFM_ERR_UNSUPPORTED, "ssfm_chirp_medium: complex64 plans only"); }
        else {
        const long long blocks = (long long)(N2 / cols_per_tile<T>()) * batch;
        if (!medium_ok || !u16 || E != 8 || Ef != 8 || !medium_shape(N1, N2) || n < 8192 || blocks % kBarShards != 0 || blocks > 64
            || n * batch > medium_max_samples || medium_xcc < 0)
            return fail(SSFM_ERR_UNSUPPORTED, "ssfm_chirp_medium: a complex64 plan of 2^13 ... 2^17 points (2^17 in all rows) with the one-XCD engine is needed");
        if (nn < 2 || 2 * nn - 1 > n) return fail(SSFM_ERR_INVALID, "ssfm_chirp_medium: %lld samples do not fit a line of %lld", (long long)nn, (long long)n);
        if (int rc = use_device()) return rc;
        const unsigned gM = (unsigned)std::min<long long>((n + 255) / 256, 4096);
        // the two convolutions' transfer functions, generated and transformed on the device once per length (the slots' tags say what they hold)
        const uint64_t want = 0xC412000000000000ull ^ (uint64_t)nn;
        if (!xfer_tab[0] || !xfer_tab[1] || tags[1] != want || tags[2] != want) {
            // ... in DOUBLE on a complex128 plan of the line's length that lives for this block, rounded once: an error of the tables is the same at every
            // step and adds up over a run (tables from the complex64 transform itself: 1.6e-5 ... 2.6e-5 from the reference result after 100 steps, the
            // tolerance is 2e-5; rounded from double: what the data's own rounding leaves).  The kernel of the inverse transform is the conjugate of
            // the forward one's, and both are symmetric on the line: H1 = conj(H0).
            tags[1] = tags[2] = 0;
            for (int slot = 0; slot < 2; ++slot)
                if (int rc = ensure_xfer(slot)) return rc;
            if (int rc = ensure_scratch()) return rc;
            std::unique_ptr<PlanT<double>> wide(new (std::nothrow) PlanT<double>());
            if (!wide) return fail(SSFM_ERR_INVALID, "out of host memory");
            wide->precision = SSFM_C128;
            if (int rc = wide->init(device, n, 1)) return rc;
            hipLaunchKernelGGL(k_cm_kernel_line<double>, dim3(gM), dim3(256), 0, wide->stream, wide->F, (long long)nn, (long long)n, 0);
            if (int rc = wide->field_spectrum()) return rc;
            HIP_TRY(hipStreamSynchronize(wide->stream));
            for (int slot = 0; slot < 2; ++slot) {
                hipLaunchKernelGGL(k_cm_narrow, dim3(gM), dim3(256), 0, stream, (const cx<double>*)wide->scratch, scratch, (long long)n, slot);
                hipLaunchKernelGGL((k_make_freq_table<T, 1>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream,
                                   (const cx<T>*)scratch, xfer_tab[slot], N1, N2, N2 / Ef, (T)0, inv_n());
            }
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipStreamSynchronize(stream));
            HIP_TRY(hipSetDevice(device));
            last_launches += 8;
            tags[1] = tags[2] = want;
        }
        return SSFM_OK;
        }
    }
    // A fixed-step chirp-z run of nn samples per row (2 nn - 1 <= n) on the line of a MEDIUM complex64 plan (2^13 ... 2^17 points) in one launch on one XCD
    // (k_medium_chirp) between two pointwise launches.  Synchronous.  SSFM_ERR_UNSUPPORTED with A as it was: not such a plan, more than kMaxTables step
    // sizes, or the launch's workgroups did not meet within the patience (the engine is then off for this plan).
    int chirp_medium(void* A_, const void* chirp_, const void* Dt_, int64_t nn, double gamma, const double* hs, int64_t nsteps) {
        if constexpr (sizeof(T) != 4) { (void)A_; (void)chirp_; (void)Dt_; (void)nn; (void)gamma; (void)hs; (void)nsteps; return fail(SSFM_ERR_UNSUPPORTED, "ssfm_chirp_medium: complex64 plans only"); }
        else {
        if (!A_ || !chirp_ || !Dt_ || !hs || nsteps < 1 || nsteps > 0x7fffffff) return fail(SSFM_ERR_INVALID, "ssfm_chirp_medium: bad arguments");
        // (the sizes are narrowed first: two float64 sizes that round to one float32 size share a table.  Too many sizes among the steps ahead of a bad one is
        // what the caller hears of, as when the steps were looked at one by one)
        const Schedule<T> sch(hs, nsteps, kMaxTables);
        if (!sch.fits_tables()) return fail(SSFM_ERR_UNSUPPORTED, "ssfm_chirp_medium: more than %d distinct step sizes", kMaxTables);
        if (!sch.valid()) return fail(SSFM_ERR_INVALID, "ssfm_chirp_medium: step %lld is %g km (must be finite and > 0)", (long long)sch.first_bad, hs[sch.first_bad]);
        const std::vector<T>& distinct = sch.distinct;
        last_launches = 0;
        if (int rc = chirp_medium_tables(nn)) return rc;
        cx<T>* A = static_cast<cx<T>*>(A_);
        const cx<T>* chirp = static_cast<const cx<T>*>(chirp_);
        const cx<T>* Dt = static_cast<const cx<T>*>(Dt_);
        const unsigned gM = (unsigned)std::min<long long>((n + 255) / 256, 4096);
        cx<T>* mulbase = nullptr;
        if (int rc = workspace(0, sizeof(cx<T>) * (size_t)n * distinct.size(), reinterpret_cast<void**>(&mulbase))) return rc;
        MediumChirpArgs<T> a;
        std::memset(&a, 0, sizeof(a));
        for (size_t i = 0; i < distinct.size(); ++i) {
            hipLaunchKernelGGL(k_cm_mul_table<T>, dim3(gM), dim3(256), 0, stream, Dt, mulbase + i * (size_t)n, (long long)nn, (long long)n, distinct[i], (T)(1.0 / (double)nn));
            a.mul[i] = mulbase + i * (size_t)n;
            ++last_launches;
        }
        if (int rc = upload_schedule(sch)) return rc;
        // (both sets of meeting words, though the launch meets in the first only: one would do, but the size of the fill shows in a trace of the run
        // and stays as it was.  The plan's XCD is picked already, chirp_medium_tables asks for it: pick_xcc in there returns at once)
        if (int rc = medium_prepare(a, batch, 2)) return rc;
        a.H[0] = xfer_tab[0]; a.H[1] = xfer_tab[1];
        a.hs = d_hs; a.which = d_which(sch);
        a.gamma = (T)gamma; a.n = (int)nn; a.nsteps = (int)nsteps;
        const unsigned gA = (unsigned)std::min<long long>((n * batch + 255) / 256, 4096);
        hipLaunchKernelGGL(k_cm_pre<T>, dim3(gA), dim3(256), 0, stream, (const cx<T>*)A, chirp, F, (long long)nn, (long long)n, batch);
        HIP_TRY(launch_medium_chirp(N1, N2, (int)a.nblk, medium_xccs, stream, a));
        hipLaunchKernelGGL(k_cm_post<T>, dim3(gA), dim3(256), 0, stream, A, chirp, (const cx<T>*)F, (long long)nn, (long long)n, batch, (const unsigned*)a.error);
        HIP_TRY(hipGetLastError());
        last_launches += 3;
        if (int rc = medium_verdict(a, medium_err_host, stream)) return rc;
        HIP_TRY(hipStreamSynchronize(stream));           // (a synchronous call: the verdict is read here, not in finish_medium)
        last_engine = SSFM_ENGINE_CHIRP_MEDIUM;
        last_fell_back = 0;
        if (medium_err_host[0] != 0u) {
            medium_err_host[0] = 0u;
            medium_gave_up(medium_ok);                   // (the fixed-step engine's flag: k_medium_chirp is k_medium's schedule around other row passes)
            return fail(SSFM_ERR_UNSUPPORTED, "ssfm_chirp_medium: the launch's workgroups did not meet within the patience; the field is unchanged");
        }
        return SSFM_OK;
        }
    }
    // ... and the adaptive run (k_medium_chirp_adapt): the step rule of ssfm_chirp_small_adapt in float32.  Synchronous.
    int chirp_medium_adapt(void* A_, const void* chirp_, const void* Dt_, int64_t nn, double gamma_d, double length, double phi_max, int64_t max_steps,
                           double* z_out, int64_t* steps_out) {
        if constexpr (sizeof(T) != 4) { (void)A_; (void)chirp_; (void)Dt_; (void)nn; (void)gamma_d; (void)length; (void)phi_max; (void)max_steps; (void)z_out; (void)steps_out;
                                        return fail(SSFM_ERR_UNSUPPORTED, "ssfm_chirp_medium_adapt: complex64 plans only"); }
        else {
        const long long blocks = (long long)(N2 / cols_per_tile<T>()) * batch;
        if (!medium_adapt_ok || !fused_ok || Ef_fly != 8 || blocks > kBarWords) return fail(SSFM_ERR_UNSUPPORTED, "ssfm_chirp_medium_adapt: the plan's one-launch adaptive engine is off");
        if (!A_ || !chirp_ || !Dt_ || !(gamma_d != 0.0) || !(length > 0) || !(phi_max > 0) || max_steps < 1 || max_steps > (1ll << 30))
            return fail(SSFM_ERR_INVALID, "ssfm_chirp_medium_adapt: bad arguments");
        last_launches = 0;
        if (int rc = chirp_medium_tables(nn)) return rc;
        cx<T>* A = static_cast<cx<T>*>(A_);
        const cx<T>* chirp = static_cast<const cx<T>*>(chirp_);
        if (int rc = ensure_zlog(max_steps)) return rc;
        if (int rc = upload_adapt_state((T)gamma_d, (T)length, (T)phi_max, (int)max_steps)) return rc;
        hipLaunchKernelGGL(k_absmax<T>, dim3(256), dim3(256), 0, stream, (const cx<T>*)A, (long long)nn * batch, st);
        hipLaunchKernelGGL(k_step_control<T>, dim3(1), dim3(64), 0, stream, st, zlog, 0, 0, 0);
        MediumChirpAdaptArgs<T> a;
        std::memset(&a, 0, sizeof(a));
        if (int rc = medium_prepare(a, batch, 1)) return rc;             // (as adaptive_run; the plan's XCD is picked already: chirp_medium_tables asks for it)
        a.H[0] = xfer_tab[0]; a.H[1] = xfer_tab[1]; a.Dt = static_cast<const cx<T>*>(Dt_); a.st = st; a.zlog = zlog;
        a.gamma = (T)gamma_d; a.inv_len = (T)(1.0 / (double)nn); a.n = (int)nn;
        const unsigned gA = (unsigned)std::min<long long>((n * batch + 255) / 256, 4096);
        hipLaunchKernelGGL(k_cm_pre<T>, dim3(gA), dim3(256), 0, stream, (const cx<T>*)A, chirp, F, (long long)nn, (long long)n, batch);
        HIP_TRY(launch_medium_chirp_adapt(N1, N2, (int)a.nblk, medium_xccs, stream, a));
        // (the barriers report through the engine's error word, the hand-over of the maxima through the step state's: the field goes back to the caller
        // -- the post kernel -- only when both are clear and the run is done)
        unsigned gave_up[2] = {0u, 0u};
        StepState<T> fin = {};
        if (int rc = medium_adapt_verdict(a, gave_up, &fin)) return rc;
        last_launches += 5;
        last_engine = SSFM_ENGINE_CHIRP_MEDIUM_ADAPT;
        last_fell_back = 0;
        if (gave_up[0] != 0u || gave_up[1] != 0u || !fin.done) {
            medium_gave_up(medium_adapt_ok);
            return fail(SSFM_ERR_UNSUPPORTED, "ssfm_chirp_medium_adapt: the launch's workgroups did not meet within the patience; the field is unchanged");
        }
        hipLaunchKernelGGL(k_cm_post<T>, dim3(gA), dim3(256), 0, stream, A, chirp, (const cx<T>*)F, (long long)nn, (long long)n, batch, (const unsigned*)a.error);
        HIP_TRY(hipGetLastError());
        if (z_out) {
            std::vector<T> zl((size_t)fin.steps + 1);
            HIP_TRY(hipMemcpyAsync(zl.data(), zlog, sizeof(T) * zl.size(), hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipStreamSynchronize(stream));
            for (size_t i = 0; i < zl.size(); ++i) z_out[i] = (double)zl[i];
        }
        HIP_TRY(hipStreamSynchronize(stream));
        if (steps_out) *steps_out = fin.steps;
        return SSFM_OK;
        }
    }
    // slot <- fft(field): the field itself becomes a resident transfer function (row 0; the field is consumed)
    int table_from_field(int slot) {
        if (int rc = no_split("ssfm_table_from_field")) return rc;
        if (slot < 0 || slot > 1) return fail(SSFM_ERR_INVALID, "ssfm_table_from_field: slot %d", slot);
        if (int rc = use_device()) return rc;
        if (int rc = ensure_xfer(slot)) return rc;
        tags[1 + slot] = 0;
        if (int rc = field_spectrum()) return rc;
        hipLaunchKernelGGL((k_make_freq_table<T, 1>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream,
                           (const cx<T>*)scratch, xfer_tab[slot], N1, N2, N2 / Ef, (T)0, inv_n());
        HIP_TRY(hipGetLastError());
        ++last_launches;
        return SSFM_OK;
    }
    // scratch <- fft(field) of every row, natural frequency order (the field is consumed)
    int field_spectrum() {
        if (int rc = ensure_scratch()) return rc;
        HIP_TRY((launch_time<T, TM_BEGIN>(N1, batch, stream, targs(0, 0, 0, nullptr), E)));
        HIP_TRY((launch_freq<T, FM_FWD_ONLY>(N2, N1 * batch, stream, fargs(dperm, 0, nullptr), Ef)));
        const long long total = (long long)n * batch;
        hipLaunchKernelGGL(k_unpermute<T>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, (const cx<T>*)Y, scratch, N1, N2, batch);
        HIP_TRY(hipGetLastError());
        last_launches += 3;
        return SSFM_OK;
    }
    int apply_table(int slot) {
        if (int rc = no_split("ssfm_apply_table")) return rc;
        if (slot < 0 || slot > 1 || !xfer_tab[slot]) return fail(SSFM_ERR_STATE, "ssfm_apply_table: slot %d holds no table", slot);
        if (int rc = use_device()) return rc;
        HIP_TRY((launch_time<T, TM_BEGIN>(N1, batch, stream, targs(0, 0, 0, nullptr), E)));
        HIP_TRY((launch_freq<T, FM_TABLE>(N2, N1 * batch, stream, fargs(xfer_tab[slot], 0, nullptr), Ef)));
        HIP_TRY((launch_time<T, TM_END>(N1, batch, stream, targs(0, 0, 0, nullptr), E)));
        last_launches += 3;
        return SSFM_OK;
    }
    // apply_table with a table per batch row (FM_TABLE_ROWS): `tabs` holds batch * n entries in the tables' order, row b's from b * n on
    int apply_row_tables(const void* tabs) {
        if (int rc = no_split("ssfm_manakov_pmd_propagate")) return rc;
        if (!tabs) return fail(SSFM_ERR_INVALID, "ssfm_manakov_pmd_propagate: NULL row tables");
        if (int rc = use_device()) return rc;
        HIP_TRY((launch_time<T, TM_BEGIN>(N1, batch, stream, targs(0, 0, 0, nullptr), E)));
        HIP_TRY((launch_freq<T, FM_TABLE_ROWS>(N2, N1 * batch, stream, fargs(static_cast<const cx<T>*>(tabs), 0, nullptr), Ef)));
        HIP_TRY((launch_time<T, TM_END>(N1, batch, stream, targs(0, 0, 0, nullptr), E)));
        last_launches += 3;
        return SSFM_OK;
    }
    // out <- src (n complex values, natural frequency order) in the order of the plan's transfer tables: k_make_freq_table's copy, as D~ is brought there
    int to_table_order(const void* src, void* out) {
        if (int rc = no_split("ssfm_manakov_pmd_propagate")) return rc;
        if (int rc = use_device()) return rc;
        hipLaunchKernelGGL((k_make_freq_table<T, 0>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream,
                           static_cast<const cx<T>*>(src), static_cast<cx<T>*>(out), N1, N2, N2 / Ef, (T)0, inv_n());
        HIP_TRY(hipGetLastError());
        ++last_launches;
        return SSFM_OK;
    }

    int debug_fft(void* dst) {
        if (int rc = no_split("ssfm_debug")) return rc;
        if (int rc = use_device()) return rc;
        const int nrows = N1 * batch;
        if (int rc = ensure_scratch()) return rc;
        HIP_TRY((launch_time<T, TM_BEGIN>(N1, batch, stream, targs(0, 0, 0, nullptr), E)));
        HIP_TRY((launch_freq<T, FM_FWD_ONLY>(N2, nrows, stream, fargs(dperm, 0, nullptr), Ef)));
        const long long total = (long long)n * batch;
        hipLaunchKernelGGL(k_unpermute<T>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream,
                           (const cx<T>*)Y, scratch, N1, N2, batch);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(dst, scratch, sizeof(cx<T>) * total, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        return SSFM_OK;
    }
};

}  // namespace

struct ssfm_plan {
    PlanBase* impl;
};

#define WITH_PLAN(p, expr)                                                          \
    do {                                                                            \
        if ((p) == nullptr || (p)->impl == nullptr) return fail(SSFM_ERR_INVALID, "null plan"); \
        if ((p)->impl->precision == SSFM_C64) { auto* P_ = static_cast<PlanT<float>*>((p)->impl); return (expr); } \
        auto* P_ = static_cast<PlanT<double>*>((p)->impl);                          \
        return (expr);                                                              \
    } while (0)

namespace {
template <typename PT> static int set_field_impl(PT* P_, const void* src, int is_device) {
    if (int rc = P_->use_device()) return rc;
    HIP_TRY(hipMemcpyAsync(P_->user_field(), src, sizeof(*P_->F) * P_->n * P_->batch, is_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, P_->stream));
    if (P_->is_split()) { P_->nat_valid = true; P_->sub_valid = false; }
    if (!is_device) HIP_TRY(hipStreamSynchronize(P_->stream));
    return SSFM_OK;
}

template <typename PT> static int sync_impl(PT* P_) {
    if (int rc = P_->use_device()) return rc;
    HIP_TRY(hipStreamSynchronize(P_->stream));
    return P_->lane_health();
}

template <typename PT> static int last_ms_impl(PT* P_, float* ms, int64_t* launches) {
    if (launches) *launches = P_->last_launches;
    if (ms) {
        *ms = 0.f;
        if (P_->timed) {
            HIP_TRY(hipEventSynchronize(P_->ev1));
            HIP_TRY(hipEventElapsedTime(ms, P_->ev0, P_->ev1));
        }
    }
    return P_->lane_health();
}
}  // namespace

namespace {
template <typename PT> static int run_info_impl(PT* P_, ssfm_run_info* info, size_t bytes) {
    if (int rc = P_->use_device()) return rc;
    if (int rc = P_->lane_health()) return rc;
    ssfm_run_info r;
    std::memset(&r, 0, sizeof(r));
    r.engine = P_->last_engine; r.fell_back = P_->last_fell_back; r.fallbacks_total = P_->fallbacks;
    P_->lanes.fill(&r, P_->nlanes);
    r.lane_ratings_total = g_lane_ratings.load(); r.lane_pairs_reused = g_lane_pairs_reused.load();
    std::memcpy(info, &r, bytes < sizeof(r) ? bytes : sizeof(r));
    return SSFM_OK;
}
}  // namespace

namespace {
// A caller that takes the stream or the field pointer may order its own work behind a run without ssfm_synchronize -- also behind a run that is ALREADY
// queued: a one-launch run of a medium plan that is still pending is resolved here (waited for, checked, repeated on the two-kernel engine if its
// workgroups did not meet), so that what the caller orders on the stream finds the run's real result.  nullptr (ssfm_last_error set) if that fails.
template <typename PT> static bool mark_external(PT* P_) {
    P_->external_order = true;
    // (a capture run's helper thread copies the end field from F on a stream of its own: it is joined here, before the caller can order anything that
    // writes F behind the run -- ADVICE r5: the snapshots' validity "after any later call on the plan" includes these two calls)
    if (P_->is_split() && (P_->use_device() != SSFM_OK || P_->publish_if_external() != SSFM_OK)) return false;      // (the natural-order field, queued on the plan's stream; the caller may write it)
    if (!P_->medium_pending && !P_->cap_pending) return true;
    return P_->use_device() == SSFM_OK;               // (joins the capture helper, resolves a pending one-launch run)
}
// The library's own cross-unit accessors (chirpz.hip writes F on the plan's stream through them): the same join.
template <typename PT> static bool join_helpers(PT* P_) {
    if (!P_->medium_pending && !P_->cap_pending) return true;
    return P_->use_device() == SSFM_OK;
}
}  // namespace

extern "C" {

int ssfm_abi_version(void) { return SSFM_ABI_VERSION; }

const char* ssfm_last_error(void) { return g_err; }

int ssfm_device_count(int* count) {
    if (!count) return fail(SSFM_ERR_INVALID, "count is NULL");
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess) { *count = 0; return fail(SSFM_ERR_NO_DEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e)); }
    *count = c;
    return SSFM_OK;
}

int ssfm_supported_log2n(int precision, int* lo, int* hi) {
    if (precision != SSFM_C64 && precision != SSFM_C128) return fail(SSFM_ERR_UNSUPPORTED, "unknown precision %d", precision);
    if (lo) *lo = kLog2Min;
    if (hi) *hi = kLog2Max;
    return SSFM_OK;
}

int ssfm_plan_create(ssfm_plan** out, int device, int64_t n, int batch, int precision) {
    if (!out) return fail(SSFM_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (precision != SSFM_C64 && precision != SSFM_C128) return fail(SSFM_ERR_UNSUPPORTED, "unknown precision %d", precision);
    if (batch < 1 || batch > 65535) return fail(SSFM_ERR_INVALID, "batch=%d out of range [1, 65535]", batch);
    if (n < (1ll << kLog2Min) || n > (1ll << kLog2Max) || (n & (n - 1)) != 0)
        return fail(SSFM_ERR_UNSUPPORTED, "n=%lld: the HIP path needs a power of two in [2^%d, 2^%d]", (long long)n, kLog2Min, kLog2Max);
    int count = 0;
    if (int rc = ssfm_device_count(&count)) return rc;
    if (device < 0 || device >= count) return fail(SSFM_ERR_NO_DEVICE, "device %d not available (%d visible)", device, count);
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(SSFM_ERR_NO_DEVICE, "device %d is %s; this library is built for gfx950 only", device, prop.gcnArchName);
    ssfm_plan* p = new (std::nothrow) ssfm_plan{nullptr};
    if (!p) return fail(SSFM_ERR_INVALID, "out of host memory");
    int rc;
    if (precision == SSFM_C64) {
        auto* impl = new (std::nothrow) PlanT<float>();
        if (!impl) { delete p; return fail(SSFM_ERR_INVALID, "out of host memory"); }
        impl->precision = precision;
        p->impl = impl;
        rc = impl->init(device, n, batch);
    } else {
        auto* impl = new (std::nothrow) PlanT<double>();
        if (!impl) { delete p; return fail(SSFM_ERR_INVALID, "out of host memory"); }
        impl->precision = precision;
        p->impl = impl;
        rc = impl->init(device, n, batch);
    }
    if (rc != SSFM_OK) { delete p->impl; delete p; return rc; }
    *out = p;
    return SSFM_OK;
}

int ssfm_plan_destroy(ssfm_plan* plan) {
    if (!plan) return SSFM_OK;
    delete plan->impl;
    delete plan;
    return SSFM_OK;
}

int ssfm_set_linear_operator(ssfm_plan* plan, const void* dtilde_host) {
    if (!dtilde_host) return fail(SSFM_ERR_INVALID, "dtilde_host is NULL");
    WITH_PLAN(plan, P_->set_operator(dtilde_host));
}

int ssfm_set_field(ssfm_plan* plan, const void* src, int is_device) {
    if (!src) return fail(SSFM_ERR_INVALID, "src is NULL");
    WITH_PLAN(plan, set_field_impl(P_, src, is_device));
}
int ssfm_get_field(ssfm_plan* plan, void* dst, int is_device) {
    if (!dst) return fail(SSFM_ERR_INVALID, "dst is NULL");
    WITH_PLAN(plan, (P_->use_device() ? SSFM_ERR_HIP : P_->copy_field_out(dst, is_device != 0, true)));
}
void* ssfm_field_device_ptr(ssfm_plan* plan) {
    if (!plan || !plan->impl) return nullptr;
    if (plan->impl->precision == SSFM_C64) { auto* P_ = static_cast<PlanT<float>*>(plan->impl); return mark_external(P_) ? P_->user_field() : nullptr; }
    auto* P_ = static_cast<PlanT<double>*>(plan->impl);
    return mark_external(P_) ? P_->user_field() : nullptr;
}

int ssfm_propagate_fixed(ssfm_plan* plan, double gamma, const void* h_schedule, int64_t nsteps, void* snapshots) {
    if (nsteps < 0) return fail(SSFM_ERR_INVALID, "nsteps=%lld", (long long)nsteps);
    if (nsteps > 0 && !h_schedule) return fail(SSFM_ERR_INVALID, "h_schedule is NULL");
    if (!plan || !plan->impl) return fail(SSFM_ERR_INVALID, "null plan");
    if (plan->impl->precision == SSFM_C64)
        return static_cast<PlanT<float>*>(plan->impl)->propagate_fixed(gamma, static_cast<const float*>(h_schedule), nsteps, snapshots);
    return static_cast<PlanT<double>*>(plan->impl)->propagate_fixed(gamma, static_cast<const double*>(h_schedule), nsteps, snapshots);
}

int ssfm_propagate_fixed_capture(ssfm_plan* plan, double gamma, const void* h_schedule, int64_t nsteps, const ssfm_capture* cap) {
    if (!h_schedule || !cap) return fail(SSFM_ERR_INVALID, "ssfm_propagate_fixed_capture: NULL argument");
    if (!plan || !plan->impl) return fail(SSFM_ERR_INVALID, "null plan");
    if (plan->impl->precision == SSFM_C64)
        return static_cast<PlanT<float>*>(plan->impl)->propagate_fixed_capture(gamma, static_cast<const float*>(h_schedule), nsteps, cap->every, cap->fields, cap->scalars);
    return static_cast<PlanT<double>*>(plan->impl)->propagate_fixed_capture(gamma, static_cast<const double*>(h_schedule), nsteps, cap->every, cap->fields, cap->scalars);
}
int ssfm_propagate_adaptive(ssfm_plan* plan, double gamma, double length, double phi_max, int single_step,
                            int64_t max_steps, int64_t* steps_out, double* z_out, void* snapshots) {
    WITH_PLAN(plan, P_->propagate_adaptive(gamma, length, phi_max, single_step, max_steps, steps_out, z_out, snapshots));
}

int ssfm_adaptive_begin(ssfm_plan* plan, double gamma, double length, double phi_max, int single_step, int64_t max_steps, int capture) {
    WITH_PLAN(plan, P_->adaptive_begin(gamma, length, phi_max, single_step, max_steps, capture));
}
int ssfm_adaptive_run(ssfm_plan* plan, int64_t budget, void* snapshots, int64_t* steps_total, int* done) {
    WITH_PLAN(plan, P_->adaptive_run(budget, snapshots, steps_total, done));
}
int ssfm_adaptive_finish(ssfm_plan* plan, int64_t* steps_out, double* z_out) { WITH_PLAN(plan, P_->adaptive_finish(steps_out, z_out)); }
int ssfm_adaptive_set_capture(ssfm_plan* plan, const ssfm_adaptive_capture* cap) {
    if (!cap) return fail(SSFM_ERR_INVALID, "ssfm_adaptive_set_capture: NULL description");
    WITH_PLAN(plan, P_->adaptive_set_capture(cap->every, cap->steps, cap->n_steps, cap->fields, cap->capacity, cap->taken, cap->n_taken));
}

int ssfm_apply_transfer(ssfm_plan* plan, const void* H_host) {
    if (!H_host) return fail(SSFM_ERR_INVALID, "H_host is NULL");
    WITH_PLAN(plan, P_->apply_transfer(H_host));
}

int ssfm_apply_dispersion(ssfm_plan* plan, double dt_s, double D_s2, void* H_out) {
    if (!(dt_s > 0)) return fail(SSFM_ERR_INVALID, "dt_s must be positive");
    WITH_PLAN(plan, P_->apply_dispersion(dt_s, D_s2, H_out));
}

int ssfm_transfer_table(ssfm_plan* plan, const void* H_host, int slot) {
    if (!H_host) return fail(SSFM_ERR_INVALID, "H_host is NULL");
    WITH_PLAN(plan, P_->transfer_table(H_host, slot));
}
int ssfm_apply_table(ssfm_plan* plan, int slot) { WITH_PLAN(plan, P_->apply_table(slot)); }
int ssfm_table_from_field(ssfm_plan* plan, int slot) { WITH_PLAN(plan, P_->table_from_field(slot)); }
int ssfm_synchronize(ssfm_plan* plan) { WITH_PLAN(plan, sync_impl(P_)); }

void* ssfm_stream(ssfm_plan* plan) {
    if (!plan || !plan->impl) return nullptr;
    if (plan->impl->precision == SSFM_C64) { auto* P_ = static_cast<PlanT<float>*>(plan->impl); return mark_external(P_) ? P_->stream : nullptr; }
    auto* P_ = static_cast<PlanT<double>*>(plan->impl);
    return mark_external(P_) ? P_->stream : nullptr;
}


int ssfm_debug(ssfm_plan* plan, int what, int64_t arg, void* dst) {
    if (what == SSFM_DEBUG_FFT) {
        if (!dst) return fail(SSFM_ERR_INVALID, "ssfm_debug: dst is NULL");
        WITH_PLAN(plan, P_->debug_fft(dst));
    }
    if (what == SSFM_DEBUG_LANE_FAULT) {
        const int mode = (int)arg;
        WITH_PLAN(plan, (P_->lanes.debug_fault(mode), (int)SSFM_OK));
    }
    return fail(SSFM_ERR_INVALID, "ssfm_debug: what = %d", what);
}
int ssfm_last_run_info(ssfm_plan* plan, ssfm_run_info* info, size_t info_bytes) {
    if (!info || info_bytes < 2 * sizeof(int)) return fail(SSFM_ERR_INVALID, "ssfm_last_run_info: info is NULL or too small");
    WITH_PLAN(plan, run_info_impl(P_, info, info_bytes));
}

int ssfm_last_propagate_ms(ssfm_plan* plan, float* ms, int64_t* launches) { WITH_PLAN(plan, last_ms_impl(P_, ms, launches)); }

int ssfm_set_profiling(ssfm_plan* plan, int mode) { WITH_PLAN(plan, (P_->profiling = mode != 0, P_->prof_mode = mode, (int)SSFM_OK)); }
int ssfm_plan_set_tag(ssfm_plan* plan, int which, uint64_t tag) {
    if (which < 0 || which > 2) return fail(SSFM_ERR_INVALID, "ssfm_plan_set_tag: which = %d", which);
    WITH_PLAN(plan, (P_->tags[which] = tag, (int)SSFM_OK));
}
int ssfm_plan_get_tag(ssfm_plan* plan, int which, uint64_t* tag) {
    if (which < 0 || which > 2 || !tag) return fail(SSFM_ERR_INVALID, "ssfm_plan_get_tag: bad argument");
    WITH_PLAN(plan, (*tag = (which == 0 && !P_->have_op) ? 0 : P_->tags[which], (int)SSFM_OK));
}
int ssfm_kernel_times(ssfm_plan* plan, int64_t counts[2], double total_ms[2]) {
    if (!counts || !total_ms) return fail(SSFM_ERR_INVALID, "NULL output");
    WITH_PLAN(plan, P_->kernel_times(counts, total_ms));
}

}  // extern "C"

// ---- the library's own cross-unit entry points (ssfm_common.hpp): not part of the C ABI
namespace ssfm {
void* plan_stream(ssfm_plan* plan) {
    if (!plan || !plan->impl) return nullptr;
    if (plan->impl->precision == SSFM_C64) { auto* P_ = static_cast<PlanT<float>*>(plan->impl); return join_helpers(P_) ? P_->stream : nullptr; }
    auto* P_ = static_cast<PlanT<double>*>(plan->impl);
    return join_helpers(P_) ? P_->stream : nullptr;
}
void* plan_field(ssfm_plan* plan) {
    if (!plan || !plan->impl) return nullptr;
    // (the library's other units work on the field buffer as a line of `plan_length` points: not for split plans, whose F holds sub-sequences)
    if (plan->impl->precision == SSFM_C64) { auto* P_ = static_cast<PlanT<float>*>(plan->impl); return join_helpers(P_) && !P_->is_split() ? (void*)P_->F : nullptr; }
    auto* P_ = static_cast<PlanT<double>*>(plan->impl);
    return join_helpers(P_) && !P_->is_split() ? (void*)P_->F : nullptr;
}
int64_t plan_length(ssfm_plan* plan, int* batch, int* precision) {
    if (!plan || !plan->impl) return 0;
    if (precision) *precision = plan->impl->precision;
    if (plan->impl->precision == SSFM_C64) { auto* P_ = static_cast<PlanT<float>*>(plan->impl); if (batch) *batch = P_->batch_full; return P_->n_full; }
    auto* P_ = static_cast<PlanT<double>*>(plan->impl);
    if (batch) *batch = P_->batch_full;
    return P_->n_full;
}
int plan_workspace(ssfm_plan* plan, int slot, size_t bytes, void** out) { WITH_PLAN(plan, P_->workspace(slot, bytes, out)); }
namespace {
template <typename PT> static int manakov_begin_impl(PT* P_, ManakovPlan* out) {
    if (int rc = P_->no_split("ssfm_manakov_propagate")) return rc;
    if (int rc = P_->use_device()) return rc;
    if (!P_->have_op) return fail(SSFM_ERR_STATE, "ssfm_manakov_propagate: the plan has no linear operator (ssfm_set_linear_operator)");
    for (int slot = 0; slot < 2; ++slot) {
        if (int rc = P_->ensure_xfer(slot)) return rc;
        P_->tags[1 + slot] = 0;
        out->tab[slot] = P_->xfer_tab[slot];
    }
    out->F = P_->F; out->D = P_->dperm; out->stream = P_->stream; out->n = P_->n; out->batch = P_->batch; out->precision = P_->precision;
    P_->last_engine = SSFM_ENGINE_MANAKOV_LINE; P_->last_fell_back = 0; P_->last_launches = 0; P_->timed = false;
    return SSFM_OK;
}
}  // namespace
int plan_manakov_begin(ssfm_plan* plan, ManakovPlan* out) {
    if (!out) return fail(SSFM_ERR_INVALID, "ssfm_manakov_propagate: NULL plan description");
    WITH_PLAN(plan, manakov_begin_impl(P_, out));
}
namespace {
template <typename PT> static int manakov_pmd_begin_impl(PT* P_, ManakovPlan* out) {
    if (int rc = P_->no_split("ssfm_manakov_pmd_propagate")) return rc;
    if (int rc = P_->use_device()) return rc;
    if (!P_->have_op) return fail(SSFM_ERR_STATE, "ssfm_manakov_pmd_propagate: the plan has no linear operator (ssfm_set_linear_operator)");
    out->tab[0] = out->tab[1] = nullptr;             // (the per-row tables live in the plan's workspace: the slots of ssfm_transfer_table stay as they are)
    out->F = P_->F; out->D = P_->dperm; out->stream = P_->stream; out->n = P_->n; out->batch = P_->batch; out->precision = P_->precision;
    P_->last_engine = SSFM_ENGINE_MANAKOV_PMD_LINE; P_->last_fell_back = 0; P_->last_launches = 0; P_->timed = false;
    return SSFM_OK;
}
}  // namespace
int plan_manakov_pmd_begin(ssfm_plan* plan, ManakovPlan* out) {
    if (!out) return fail(SSFM_ERR_INVALID, "ssfm_manakov_pmd_propagate: NULL plan description");
    WITH_PLAN(plan, manakov_pmd_begin_impl(P_, out));
}
int plan_to_table_order(ssfm_plan* plan, const void* src, void* out) { WITH_PLAN(plan, P_->to_table_order(src, out)); }
int plan_apply_row_tables(ssfm_plan* plan, const void* tabs) { WITH_PLAN(plan, P_->apply_row_tables(tabs)); }
void plan_count_launches(ssfm_plan* plan, int64_t launches) {
    if (!plan || !plan->impl) return;
    if (plan->impl->precision == SSFM_C64) static_cast<PlanT<float>*>(plan->impl)->last_launches += launches;
    else static_cast<PlanT<double>*>(plan->impl)->last_launches += launches;
}
int plan_chirp_step(ssfm_plan* plan, const void* mul_dev, const ChirpStepIO* io) {
    if (!io) return fail(SSFM_ERR_INVALID, "chirp step: NULL field description");
    WITH_PLAN(plan, P_->apply_tables_mul(mul_dev, io));
}
int plan_chirp_line_run(ssfm_plan* plan, const void* const* mul, const unsigned char* which, const double* hs, int64_t nsteps, double gamma, int64_t keep, int half) {
    WITH_PLAN(plan, P_->chirp_line_run(mul, which, hs, nsteps, gamma, keep, half));
}
int plan_line_half_ok(ssfm_plan* plan) {
    if (!plan || !plan->impl || plan->impl->precision == SSFM_C64) return 0;
    return static_cast<PlanT<double>*>(plan->impl)->line_half_ok() ? 1 : 0;
}
int plan_chirp_small(ssfm_plan* plan, void* A, const void* chirp, const void* Dt, int64_t n, double gamma, const double* hs, int64_t nsteps) {
    WITH_PLAN(plan, P_->chirp_small(A, chirp, Dt, n, gamma, hs, nsteps));
}
int plan_chirp_small_adapt(ssfm_plan* plan, void* A, const void* chirp, const void* Dt, int64_t n, double gamma, double length, double phi_max, int f32,
                           int64_t max_steps, double* z_out, int64_t* steps_out) {
    WITH_PLAN(plan, P_->chirp_small_adapt(A, chirp, Dt, n, gamma, length, phi_max, f32, max_steps, z_out, steps_out));
}
int plan_chirp_medium(ssfm_plan* plan, void* A, const void* chirp, const void* Dt, int64_t n, double gamma, const double* hs, int64_t nsteps) {
    WITH_PLAN(plan, P_->chirp_medium(A, chirp, Dt, n, gamma, hs, nsteps));
}
int plan_chirp_medium_adapt(ssfm_plan* plan, void* A, const void* chirp, const void* Dt, int64_t n, double gamma, double length, double phi_max, int64_t max_steps,
                            double* z_out, int64_t* steps_out) {
    WITH_PLAN(plan, P_->chirp_medium_adapt(A, chirp, Dt, n, gamma, length, phi_max, max_steps, z_out, steps_out));
}
}  // namespace ssfm
