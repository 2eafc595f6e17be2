// fbg.hip -- the fibre Bragg grating FBG (reference devices.py:1894-2173) on gfx950: the coupled-mode equations
//     dR/dz = j (sig R + k S),  dS/dz = -j (sig S + k R),  sig = delta + s p(z) - F z,  k -> k p(z)
// integrated from z = +1/2 to -1/2 (R = 1, S = 0) for every frequency bin at once, with the step control of
// scipy.integrate.solve_ivp(method="RK45") (SciPy 1.15: _ivp/rk.py RungeKutta._step_impl / rk_step, _ivp/common.py select_initial_step / norm):
// one shared step size, RMS error norm over all 2N complex unknowns.  H = S / R at z = -1/2.
//
// One thread per bin holds R and S in complex128.  Per ATTEMPTED step two launches run on the default stream:
//   * k_step    the six Dormand-Prince stages (FSAL: the first stage is the last of the previous step), y_new, f_new and the sum of
//               |e / scale|^2 per workgroup, into the ping-pong half of the state that is not current;
//   * k_decide  one workgroup: folds the partials in a fixed order (results do not depend on scheduling), accepts or rejects, sets the next
//               h_abs exactly as scipy does (SAFETY, MIN_FACTOR, MAX_FACTOR, the step_rejected cap, min_step, clipping to t_bound) and
//               prepares the next attempt (t, h) in the state block, or raises the done flag.
// Launches after the finish return at once.  The host enqueues kBatch attempts and then reads the state block (one wait per batch).  A
// custom (host) apodization needs p(z) at the six stage positions t + C h, so that path reads the state and uploads p once per attempt.
//
// Arithmetic follows NumPy's expressions (no contraction: #pragma clang fp contract(off)); summation orders of the reductions differ from
// NumPy's, so a step decision can only differ when an error norm lies within a few ulp of 1.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "ssfm_amd.h"
#include "ssfm_common.hpp"

using ssfm::fail;
using ssfm::Scratch;
using ssfm::use_device;

namespace {

constexpr int kThreads = 256;
constexpr int kBatch = 32;                          // attempts enqueued between two looks at the done flag
constexpr int64_t kMaxN = int64_t(1) << 22;
constexpr int kMaxBlocks = int((kMaxN + kThreads - 1) / kThreads);

// the state block (doubles; integers stored exactly)
enum Slot {
    S_T,          // current t (last accepted)
    S_HABS,       // scipy's h_abs
    S_H,          // h of the prepared attempt (t_new - t)
    S_TNEW,       // t_new of the prepared attempt
    S_MINSTEP,    // min_step of the current step
    S_REJ,        // step_rejected (within the current step)
    S_CUR,        // which half of the ping-pong state is current
    S_DONE,       // 0 running, 1 finished, -1 step size too small
    S_STEPS,      // accepted steps (len(sol.t) - 1)
    S_ATTEMPTS,   // attempted steps
    S_H0, S_D1,   // select_initial_step
    S_NORM,       // last error norm
    S_COUNT
};

constexpr double kC[6] = {0.0, 1.0 / 5, 3.0 / 10, 4.0 / 5, 8.0 / 9, 1.0};                // (host: the custom apodization's positions)
__device__ constexpr double kCd[6] = {0.0, 1.0 / 5, 3.0 / 10, 4.0 / 5, 8.0 / 9, 1.0};
__device__ constexpr double kA[6][5] = {
    {0, 0, 0, 0, 0},
    {1.0 / 5, 0, 0, 0, 0},
    {3.0 / 40, 9.0 / 40, 0, 0, 0},
    {44.0 / 45, -56.0 / 15, 32.0 / 9, 0, 0},
    {19372.0 / 6561, -25360.0 / 2187, 64448.0 / 6561, -212.0 / 729, 0},
    {9017.0 / 3168, -355.0 / 33, 46732.0 / 5247, 49.0 / 176, -5103.0 / 18656}};
__device__ constexpr double kB[6] = {35.0 / 384, 0, 500.0 / 1113, 125.0 / 192, -2187.0 / 6784, 11.0 / 84};
__device__ constexpr double kE[7] = {-71.0 / 57600, 0, 71.0 / 16695, -71.0 / 1920, 17253.0 / 339200, -22.0 / 525, 1.0 / 40};

constexpr double kSafety = 0.9, kMinFactor = 0.2, kMaxFactor = 10.0;
constexpr double kErrExp = -1.0 / (4 + 1);         // -1 / (error_estimator_order + 1)
constexpr double kT0 = 0.5, kTBound = -0.5, kDir = -1.0;

struct cd { double r, i; };

// the built-in apodizations of devices.py:2058-2078, scalar z
__device__ double apodize(int apo, double z) {
#pragma clang fp contract(off)
    if (apo == SSFM_FBG_RCOS) {                     // utils.rcos(z, alpha=1, T=2), scalar branch
        const double az = fabs(z);
        if (az <= (1.0 - 1.0) / (2 * 2.0)) return 1.0;
        if (az > (1.0 + 1.0) / (2 * 2.0)) return 0.0;
        return 0.5 * (1.0 + cos(M_PI * 2.0 / 1.0 * (az - (1.0 - 1.0) / (2 * 2.0))));
    }
    if (apo == SSFM_FBG_GAUSSIAN) { const double u = 3 * z; return exp(-4 * log(2.0) * (u * u)); }
    if (apo == SSFM_FBG_PARABOLIC) { const double u = 2 * z; return 1 - u * u; }
    return 1.0;
}

// ode_system of devices.py:2030-2045 for one bin (`apod` false: the uniform grating, s and k are not multiplied)
__device__ __forceinline__ void rhs(double z, double d, double s, double k, double F, bool apod, double p, cd R, cd S, cd& dR, cd& dS) {
#pragma clang fp contract(off)
    if (apod) { s = s * p; k = k * p; }
    const double sg = d + s - F * z;
    const double xr = sg * R.r + k * S.r, xi = sg * R.i + k * S.i;     // sig R + k S
    const double yr = sg * S.r + k * R.r, yi = sg * S.i + k * R.i;     // sig S + k R
    dR = {-xi, xr};                                                    //  j (...)
    dS = {yi, -yr};                                                    // -j (...)
}

__device__ __forceinline__ double sq(cd a) {
#pragma clang fp contract(off)
    return a.r * a.r + a.i * a.i;
}

__device__ void block_sum_store(double v, double* __restrict__ part) {
    __shared__ double lds[kThreads];
    lds[threadIdx.x] = v;
    __syncthreads();
    for (int off = kThreads / 2; off > 0; off >>= 1) {
        if (threadIdx.x < off) lds[threadIdx.x] += lds[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = lds[0];
}

// the nb partials folded in a fixed order by one workgroup (every thread returns the total)
__device__ double fold(const double* __restrict__ part, int nb) {
    __shared__ double lds[kThreads];
    double v = 0.0;
    for (int b = threadIdx.x; b < nb; b += kThreads) v += part[b];
    lds[threadIdx.x] = v;
    __syncthreads();
    for (int off = kThreads / 2; off > 0; off >>= 1) {
        if (threadIdx.x < off) lds[threadIdx.x] += lds[threadIdx.x + off];
        __syncthreads();
    }
    const double r = lds[0];
    __syncthreads();
    return r;
}

struct Problem {
    const double *d, *s, *k;                         // delta L, s L, k L per bin
    const double* pv;                                // custom apodization: p at the stage positions (device, 8 doubles)
    double F, rtol, atol;
    long long n;
    int apo;                                         // SSFM_FBG_*
};

__device__ __forceinline__ double stage_p(const Problem& P, int slot, double z) {
    return P.apo == SSFM_FBG_CUSTOM ? P.pv[slot] : apodize(P.apo, z);
}

// f0 = fun(t0, y0) into f[0]; partials of |y0 / scale|^2 (part) and |f0 / scale|^2 (part + nb)
__global__ __launch_bounds__(kThreads) void k_init0(Problem P, cd* __restrict__ y, cd* __restrict__ f, double* __restrict__ part) {
#pragma clang fp contract(off)
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    double a = 0.0, b = 0.0;
    if (i < P.n) {
        const cd R = {1.0, 0.0}, S = {0.0, 0.0};
        const bool apod = P.apo != SSFM_FBG_UNIFORM;
        cd dR, dS;
        rhs(kT0, P.d[i], P.s[i], P.k[i], P.F, apod, apod ? stage_p(P, 0, kT0) : 1.0, R, S, dR, dS);
        y[i] = R; y[P.n + i] = S;
        f[i] = dR; f[P.n + i] = dS;
        const double scR = P.atol + 1.0 * P.rtol, scS = P.atol + 0.0 * P.rtol;     // atol + |y0| rtol
        a = 1.0 / scR * (1.0 / scR);
        b = sq({dR.r / scR, dR.i / scR}) + sq({dS.r / scS, dS.i / scS});
    }
    block_sum_store(a, part);
    block_sum_store(b, part + gridDim.x);
}

// d0, d1 -> h0 (select_initial_step up to the evaluation of f1)
__global__ __launch_bounds__(kThreads) void k_init0_fold(const double* __restrict__ part, int nb, long long n, double* __restrict__ st) {
#pragma clang fp contract(off)
    const double s0 = fold(part, nb), s1 = fold(part + nb, nb);
    if (threadIdx.x) return;
    const double size = 2.0 * (double)n;
    const double d0 = sqrt(s0) / sqrt(size), d1 = sqrt(s1) / sqrt(size);
    double h0 = (d0 < 1e-5 || d1 < 1e-5) ? 1e-6 : 0.01 * d0 / d1;
    const double interval = fabs(kTBound - kT0);
    h0 = fmin(h0, interval);
    for (int k = 0; k < S_COUNT; ++k) st[k] = 0.0;
    st[S_H0] = h0;
    st[S_D1] = d1;
    st[S_T] = kT0;
}

// f1 = fun(t0 + h0 dir, y0 + h0 dir f0); partials of |(f1 - f0) / scale|^2
__global__ __launch_bounds__(kThreads) void k_init1(Problem P, const cd* __restrict__ f, const double* __restrict__ st, double* __restrict__ part) {
#pragma clang fp contract(off)
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    double a = 0.0;
    if (i < P.n) {
        const double h0 = st[S_H0], hd = h0 * kDir, z = kT0 + h0 * kDir;
        const cd f0R = f[i], f0S = f[P.n + i];
        const cd R = {1.0 + hd * f0R.r, 0.0 + hd * f0R.i}, S = {0.0 + hd * f0S.r, 0.0 + hd * f0S.i};
        const bool apod = P.apo != SSFM_FBG_UNIFORM;
        cd dR, dS;
        rhs(z, P.d[i], P.s[i], P.k[i], P.F, apod, apod ? stage_p(P, 0, z) : 1.0, R, S, dR, dS);
        const double scR = P.atol + 1.0 * P.rtol, scS = P.atol + 0.0 * P.rtol;
        a = sq({(dR.r - f0R.r) / scR, (dR.i - f0R.i) / scR}) + sq({(dS.r - f0S.r) / scS, (dS.i - f0S.i) / scS});
    }
    block_sum_store(a, part);
}

// the start of a step at t: min_step and the clamp of h_abs (step_rejected cleared); then the first attempt is prepared
__device__ void start_step(double* st) {
    const double t = st[S_T];
    const double min_step = 10 * fabs(nextafter(t, kDir * INFINITY) - t);
    double h_abs = st[S_HABS];
    if (h_abs < min_step) h_abs = min_step;                   // (max_step = inf)
    st[S_HABS] = h_abs;
    st[S_MINSTEP] = min_step;
    st[S_REJ] = 0.0;
}

// the head of scipy's attempt loop: h, t_new (clipped to t_bound), h_abs = |h|
__device__ void prepare_attempt(double* st) {
#pragma clang fp contract(off)
    double h_abs = st[S_HABS];
    if (h_abs < st[S_MINSTEP]) { st[S_DONE] = -1.0; return; }
    const double t = st[S_T];
    double h = h_abs * kDir;
    double t_new = t + h;
    if (kDir * (t_new - kTBound) > 0) t_new = kTBound;
    h = t_new - t;
    st[S_H] = h;
    st[S_TNEW] = t_new;
    st[S_HABS] = fabs(h);
}

__global__ __launch_bounds__(kThreads) void k_init1_fold(const double* __restrict__ part, int nb, long long n, double* __restrict__ st) {
#pragma clang fp contract(off)
    const double s2 = fold(part, nb);
    if (threadIdx.x) return;
    const double h0 = st[S_H0], d1 = st[S_D1];
    const double d2 = sqrt(s2) / sqrt(2.0 * (double)n) / h0;
    const double h1 = (d1 <= 1e-15 && d2 <= 1e-15) ? fmax(1e-6, h0 * 1e-3) : pow(0.01 / fmax(d1, d2), 1.0 / (4 + 1));
    double h = 100 * h0;
    h = h1 < h ? h1 : h;
    const double interval = fabs(kTBound - kT0);
    h = interval < h ? interval : h;
    st[S_HABS] = h;
    start_step(st);
    prepare_attempt(st);
}

// one attempted step: stages from the current half `cur` of (y, f), results into the other half
__global__ __launch_bounds__(kThreads) void k_step(Problem P, cd* __restrict__ y, cd* __restrict__ f, const double* __restrict__ st, double* __restrict__ part) {
#pragma clang fp contract(off)
    if (st[S_DONE] != 0.0) return;
    const long long n = P.n, i = (long long)blockIdx.x * kThreads + threadIdx.x;
    const int cur = (int)st[S_CUR];
    const double t = st[S_T], h = st[S_H];
    double e2 = 0.0;
    if (i < n) {
        cd* yc = y + (size_t)cur * 2 * n;
        cd* fc = f + (size_t)cur * 2 * n;
        cd* yn = y + (size_t)(cur ^ 1) * 2 * n;
        cd* fn = f + (size_t)(cur ^ 1) * 2 * n;
        const double d = P.d[i], s = P.s[i], k = P.k[i];
        const bool apod = P.apo != SSFM_FBG_UNIFORM;
        const cd R0 = yc[i], S0 = yc[n + i];
        cd KR[7], KS[7];
        KR[0] = fc[i];
        KS[0] = fc[n + i];
#pragma unroll
        for (int st_ = 1; st_ < 6; ++st_) {                   // K[s] = fun(t + c h, y + (K[:s].T @ a[:s]) h)
            double rr = 0.0, ri = 0.0, sr = 0.0, si = 0.0;
#pragma unroll
            for (int j = 0; j < st_; ++j) {
                rr += KR[j].r * kA[st_][j]; ri += KR[j].i * kA[st_][j];
                sr += KS[j].r * kA[st_][j]; si += KS[j].i * kA[st_][j];
            }
            const cd R = {R0.r + rr * h, R0.i + ri * h}, S = {S0.r + sr * h, S0.i + si * h};
            const double z = t + kCd[st_] * h;
            rhs(z, d, s, k, P.F, apod, apod ? stage_p(P, st_ - 1, z) : 1.0, R, S, KR[st_], KS[st_]);
        }
        double rr = 0.0, ri = 0.0, sr = 0.0, si = 0.0;        // y_new = y + h (K[:-1].T @ B)
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            rr += KR[j].r * kB[j]; ri += KR[j].i * kB[j];
            sr += KS[j].r * kB[j]; si += KS[j].i * kB[j];
        }
        const cd R1 = {R0.r + h * rr, R0.i + h * ri}, S1 = {S0.r + h * sr, S0.i + h * si};
        const double z = t + h;
        rhs(z, d, s, k, P.F, apod, apod ? stage_p(P, 5, z) : 1.0, R1, S1, KR[6], KS[6]);
        double er = 0.0, ei = 0.0, fr = 0.0, fi = 0.0;        // (K.T @ E) h
#pragma unroll
        for (int j = 0; j < 7; ++j) {
            er += KR[j].r * kE[j]; ei += KR[j].i * kE[j];
            fr += KS[j].r * kE[j]; fi += KS[j].i * kE[j];
        }
        const double scR = P.atol + fmax(hypot(R0.r, R0.i), hypot(R1.r, R1.i)) * P.rtol;
        const double scS = P.atol + fmax(hypot(S0.r, S0.i), hypot(S1.r, S1.i)) * P.rtol;
        e2 = sq({er * h / scR, ei * h / scR}) + sq({fr * h / scS, fi * h / scS});
        yn[i] = R1; yn[n + i] = S1;
        fn[i] = KR[6]; fn[n + i] = KS[6];
    }
    block_sum_store(e2, part);
}

// accept / reject (rk.py _step_impl), then the next attempt or the finish (base.py OdeSolver.step)
__global__ __launch_bounds__(kThreads) void k_decide(const double* __restrict__ part, int nb, long long n, double* __restrict__ st) {
#pragma clang fp contract(off)
    if (st[S_DONE] != 0.0) return;
    const double s = fold(part, nb);
    if (threadIdx.x) return;
    const double en = sqrt(s) / sqrt(2.0 * (double)n);
    st[S_NORM] = en;
    st[S_ATTEMPTS] += 1.0;
    double h_abs = st[S_HABS];
    if (en < 1) {
        double factor = en == 0 ? kMaxFactor : fmin(kMaxFactor, kSafety * pow(en, kErrExp));
        if (st[S_REJ] != 0.0) factor = fmin(1.0, factor);
        st[S_HABS] = h_abs * factor;
        st[S_T] = st[S_TNEW];
        st[S_CUR] = 1.0 - st[S_CUR];
        st[S_STEPS] += 1.0;
        if (kDir * (st[S_T] - kTBound) >= 0) { st[S_DONE] = 1.0; return; }
        start_step(st);
    } else {
        const double g = kSafety * pow(en, kErrExp);
        st[S_HABS] = h_abs * (g > kMinFactor ? g : kMinFactor);
        st[S_REJ] = 1.0;
    }
    prepare_attempt(st);
}

// H = S / R (NumPy's complex division), optionally times exp(-j w tau) (the filtfilt correction, w in fftshift order)
__global__ __launch_bounds__(kThreads) void k_finish(const cd* __restrict__ y, const double* __restrict__ st, long long n, cd* __restrict__ H) {
#pragma clang fp contract(off)
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const int cur = (int)st[S_CUR];
    const cd R = y[(size_t)cur * 2 * n + i], S = y[(size_t)cur * 2 * n + n + i];
    cd q;
    const double ar = fabs(R.r), ai = fabs(R.i);
    if (ar >= ai) {
        if (ar == 0.0 && ai == 0.0) { q = {S.r / ar, S.i / ai}; }
        else {
            const double rat = R.i / R.r, scl = 1.0 / (R.r + R.i * rat);
            q = {(S.r + S.i * rat) * scl, (S.i - S.r * rat) * scl};
        }
    } else {
        const double rat = R.r / R.i, scl = 1.0 / (R.i + R.r * rat);
        q = {(S.r * rat + S.i) * scl, (S.i * rat - S.r) * scl};
    }
    H[i] = q;
}

__global__ __launch_bounds__(kThreads) void k_delay(cd* __restrict__ H, cd* __restrict__ Hnat, long long n, double dt, double tau, int apply) {
#pragma clang fp contract(off)
    const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    cd a = H[i];
    if (apply) {
        // w = fftshift(fftfreq(n, dt)) 2 pi: bin i holds frequency index i - n/2 (n even or odd)
        const long long m = i - n / 2;
        const double w = (double)m * (1.0 / ((double)n * dt)) * 2 * M_PI;
        const double ph = -w * tau * 1e-12;                  // Im(-1j w tau 1e-12)
        double sn, cs;
        sincos(ph, &sn, &cs);
        a = {a.r * cs - a.i * sn, a.r * sn + a.i * cs};
        H[i] = a;
    }
    Hnat[(i + n - n / 2) % n] = a;                           // ifftshift: Hnat[j] = H[(j + n/2) % n]
}


}  // namespace

// ================================================================================================ C ABI
extern "C" int ssfm_fbg_solve(int device, int64_t n, const double* delta, const double* s, const double* kappa, double F, int apodization,
                              double rtol, double atol, ssfm_fbg_apo_fn apo_fn, void* apo_user, void* H, int64_t* info) {
    if (!delta || !s || !kappa || !H || !info || n < 1 || n > kMaxN || apodization < SSFM_FBG_UNIFORM || apodization > SSFM_FBG_CUSTOM ||
        (apodization == SSFM_FBG_CUSTOM && !apo_fn) || !(rtol > 0) || !(atol >= 0))
        return fail(SSFM_ERR_INVALID, "ssfm_fbg_solve: n=%lld (1 ... 2^22) apodization=%d rtol=%g atol=%g", (long long)n, apodization, rtol, atol);
    if (int rc = use_device(device)) return rc;
    const int nb = (int)((n + kThreads - 1) / kThreads);
    Scratch sc(device);
    void *coef, *yb, *fb, *part, *stb, *pvb;
    if (int rc = sc.get(sizeof(double) * 3 * n, &coef)) return rc;
    if (int rc = sc.get(sizeof(cd) * 4 * n, &yb)) return rc;               // 2 halves x (R, S)
    if (int rc = sc.get(sizeof(cd) * 4 * n, &fb)) return rc;
    if (int rc = sc.get(sizeof(double) * 2 * kMaxBlocks, &part)) return rc;
    if (int rc = sc.get(sizeof(double) * 64, &stb)) return rc;
    if (int rc = sc.get(sizeof(double) * 8, &pvb)) return rc;
    double* cf = (double*)coef;
    HIP_TRY(hipMemcpy(cf, delta, sizeof(double) * n, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(cf + n, s, sizeof(double) * n, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(cf + 2 * n, kappa, sizeof(double) * n, hipMemcpyHostToDevice));
    Problem P{cf, cf + n, cf + 2 * n, (const double*)pvb, F, rtol, atol, (long long)n, apodization};
    cd* y = (cd*)yb;
    cd* f = (cd*)fb;
    double* pt = (double*)part;
    double* st = (double*)stb;
    double* pv = (double*)pvb;
    const bool custom = apodization == SSFM_FBG_CUSTOM;
    int64_t waits = 1;                                                      // the coefficient upload
    double host[S_COUNT];
    double z[8], p[8];
    auto user = [&](int count) -> int {                                     // p(z) on the host, uploaded (one wait)
        if (apo_fn(z, count, p, apo_user)) return fail(SSFM_ERR_INVALID, "ssfm_fbg_solve: the apodization callback failed");
        HIP_TRY(hipMemcpy(pv, p, sizeof(double) * count, hipMemcpyHostToDevice));
        return SSFM_OK;
    };
    if (custom) {
        z[0] = kT0;
        if (int rc = user(1)) return rc;
    }
    hipLaunchKernelGGL(k_init0, dim3(nb), dim3(kThreads), 0, 0, P, y, f, pt);
    hipLaunchKernelGGL(k_init0_fold, dim3(1), dim3(kThreads), 0, 0, (const double*)pt, nb, (long long)n, st);
    if (custom) {
        HIP_TRY(hipMemcpy(host, st, sizeof(double) * S_COUNT, hipMemcpyDeviceToHost));
        ++waits;
        z[0] = kT0 + host[S_H0] * kDir;
        if (int rc = user(1)) return rc;
    }
    hipLaunchKernelGGL(k_init1, dim3(nb), dim3(kThreads), 0, 0, P, (const cd*)f, (const double*)st, pt);
    hipLaunchKernelGGL(k_init1_fold, dim3(1), dim3(kThreads), 0, 0, (const double*)pt, nb, (long long)n, st);
    HIP_TRY(hipGetLastError());
    for (;;) {
        if (custom) {                                                       // one attempt per look: p at t + C h (stages 1-5) and t + h
            HIP_TRY(hipMemcpy(host, st, sizeof(double) * S_COUNT, hipMemcpyDeviceToHost));
            ++waits;
            if (host[S_DONE] != 0.0) break;
            for (int j = 1; j < 6; ++j) z[j - 1] = host[S_T] + kC[j] * host[S_H];
            z[5] = host[S_T] + host[S_H];
            if (int rc = user(6)) return rc;
            hipLaunchKernelGGL(k_step, dim3(nb), dim3(kThreads), 0, 0, P, y, f, (const double*)st, pt);
            hipLaunchKernelGGL(k_decide, dim3(1), dim3(kThreads), 0, 0, (const double*)pt, nb, (long long)n, st);
        } else {
            for (int b = 0; b < kBatch; ++b) {
                hipLaunchKernelGGL(k_step, dim3(nb), dim3(kThreads), 0, 0, P, y, f, (const double*)st, pt);
                hipLaunchKernelGGL(k_decide, dim3(1), dim3(kThreads), 0, 0, (const double*)pt, nb, (long long)n, st);
            }
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpy(host, st, sizeof(double) * S_COUNT, hipMemcpyDeviceToHost));
            ++waits;
            if (host[S_DONE] != 0.0) break;
        }
    }
    HIP_TRY(hipGetLastError());
    if (host[S_DONE] < 0)
        return fail(SSFM_ERR_STATE, "ssfm_fbg_solve: the step size fell below min_step at z=%.17g (solve_ivp: 'Required step size is less than spacing "
                    "between numbers.')", host[S_T]);
    hipLaunchKernelGGL(k_finish, dim3(nb), dim3(kThreads), 0, 0, (const cd*)y, (const double*)st, (long long)n, (cd*)H);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    ++waits;
    info[0] = (int64_t)host[S_STEPS];
    info[1] = (int64_t)host[S_ATTEMPTS];
    info[2] = waits;
    return SSFM_OK;
}

extern "C" int ssfm_fbg_delay(int device, void* H, void* H_natural, int64_t n, double dt, double tau, int apply) {
    if (!H || !H_natural || H == H_natural || n < 1 || n > kMaxN) return fail(SSFM_ERR_INVALID, "ssfm_fbg_delay: n=%lld", (long long)n);
    if (int rc = use_device(device)) return rc;
    hipLaunchKernelGGL(k_delay, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, 0, (cd*)H, (cd*)H_natural, (long long)n, dt, tau, apply);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    return SSFM_OK;
}
