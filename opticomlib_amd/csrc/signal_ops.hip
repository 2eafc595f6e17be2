// signal_ops.hip -- the algebra of electrical_signal (reference typing.py:1216-1780) on device-resident signals: the operators between two signals
// or a signal and a scalar with the reference's signal / noise rules in one pass, the unary and scalar operations, comparison, slicing, the
// reductions behind power / normalize / sum, unwrap(angle(.)) and the two pointwise ends of filter().  float64 and complex128, (rows, n) with rows = 1.
// The ssfm_field_* entry points at the end are the same algebra for optical_signal (typing.py:2103-2320): rows = 1 or 2, operands that broadcast
// along either axis, and complex64 beside the two double-precision types.  A signal is the field of one row to the slice and the row
// reductions: ssfm_signal_slice launches k_field_slice with row0 = 0, and ssfm_signal_reduce and ssfm_field_reduce share reduce_rows (one
// launch of k_field_reduce, the partials folded on the host), each behind its own argument checks.  The binary entry points stay apart:
// k_signal_binary_c<C1, C2> reads a float64 operand straight into a complex128 result, k_field_binary takes both operands in the result's type.
//
// All of them are bandwidth-bound streaming kernels: 16 bytes per lane and access (a complex128 value, or two float64 values), a grid of at most
// 256 CUs x 8 workgroups with a grid-stride loop, wavefront shuffles and four LDS words per workgroup for the reductions.  The whole file is
// compiled without contraction: `a*b + c` is a rounded product and a rounded sum as in NumPy's loops, so real-typed results are NumPy's bits.
#include <hip/hip_runtime.h>

#include "ssfm_amd.h"
#include "ssfm_common.hpp"

#pragma clang fp contract(off)

using ssfm::fail;
using ssfm::grid_for;
using ssfm::use_device;

namespace {

constexpr long long kGridCap = 2048;        // 256 CUs x 8 workgroups

struct cd { double re, im; };               // one complex128 value
struct r2 { double x, y; };                 // two neighbouring float64 values: the 16-byte unit of the real kernels
struct cf { float re, im; };                // one complex64 value (the field kernels)

__device__ __forceinline__ cd operator+(cd a, cd b) { return {a.re + b.re, a.im + b.im}; }
__device__ __forceinline__ cd operator-(cd a) { return {-a.re, -a.im}; }
__device__ __forceinline__ cd operator*(cd a, cd b) { return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
__device__ __forceinline__ cf operator+(cf a, cf b) { return {a.re + b.re, a.im + b.im}; }
__device__ __forceinline__ cf operator-(cf a) { return {-a.re, -a.im}; }
__device__ __forceinline__ cf operator*(cf a, cf b) { return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }
__device__ __forceinline__ r2 operator+(r2 a, r2 b) { return {a.x + b.x, a.y + b.y}; }
__device__ __forceinline__ r2 operator-(r2 a) { return {-a.x, -a.y}; }
__device__ __forceinline__ r2 operator*(r2 a, r2 b) { return {a.x * b.x, a.y * b.y}; }

// NumPy's complex quotient (Smith's method, the loop behind complex128 / complex128 and complex64 / complex64), in the precision of C
__device__ __forceinline__ double absr(double v) { return fabs(v); }
__device__ __forceinline__ float absr(float v) { return fabsf(v); }
template <typename C> __device__ __forceinline__ C cdiv(C a, C b) {
    using R = decltype(a.re);
    const R br = absr(b.re), bi = absr(b.im);
    if (br >= bi) {
        if (br == R(0) && bi == R(0)) return {a.re / br, a.im / br};
        const R rat = b.im / b.re, scl = R(1) / (b.re + b.im * rat);
        return {(a.re + a.im * rat) * scl, (a.im - a.re * rat) * scl};
    }
    const R rat = b.re / b.im, scl = R(1) / (b.im + b.re * rat);
    return {(a.re * rat + a.im) * scl, (a.im * rat - a.re) * scl};
}

// One operand of a binary operation: signal and (nullable) noise of `len` values, len == 1: the one value for every sample;
// s == nullptr: the scalar (re, im) with no noise.
struct Operand {
    const double* s;
    const double* n;
    long long len;
    double re, im;
};

// value `i` (for r2: values 2i, 2i + 1) of an array of `len` float64 (C = false) or complex128 (C = true) values, as T
template <typename T, bool C> __device__ __forceinline__ T load(const double* p, long long i, long long len) {
    if constexpr (sizeof(T) == sizeof(double)) {
        return p[len == 1 ? 0 : i];
    } else if constexpr (__is_same(T, r2)) {
        if (len == 1) return {p[0], p[0]};
        const double2 v = reinterpret_cast<const double2*>(p)[i];
        return {v.x, v.y};
    } else {
        const long long k = len == 1 ? 0 : i;
        if constexpr (C) {
            const double2 v = reinterpret_cast<const double2*>(p)[k];
            return {v.x, v.y};
        } else {
            return {p[k], 0.0};
        }
    }
}
template <typename T> __device__ __forceinline__ T splat(double re, double im) {
    if constexpr (sizeof(T) == sizeof(double)) return re;
    else if constexpr (__is_same(T, r2)) return {re, re};
    else return {re, im};
}
template <typename T> __device__ __forceinline__ void store(double* p, long long i, T v) {
    if constexpr (sizeof(T) == sizeof(double)) p[i] = v;
    else if constexpr (__is_same(T, r2)) reinterpret_cast<double2*>(p)[i] = make_double2(v.x, v.y);
    else reinterpret_cast<double2*>(p)[i] = make_double2(v.re, v.im);
}

__device__ __forceinline__ bool gt(double a, double b) { return a > b; }
__device__ __forceinline__ bool eq(double a, double b) { return a == b; }
// NumPy orders complex numbers by real part, then imaginary part
__device__ __forceinline__ bool gt(cd a, cd b) { return (a.re > b.re && !isnan(a.im) && !isnan(b.im)) || (a.re == b.re && a.im > b.im); }
__device__ __forceinline__ bool eq(cd a, cd b) { return a.re == b.re && a.im == b.im; }
__device__ __forceinline__ bool eq(cf a, cf b) { return a.re == b.re && a.im == b.im; }

// ---------------------------------------------------------------------------------------------- binary operations
// typing.py:1308-1348 (+, -, *), :1378-1398 (>, ==).  `h1` / `h2`: the operand has noise.  A sum with an absent noise is the other term and a
// product with one is absent (the reference's NULL, typing.py:56-93).  a - b is a + (-b) and b - a is (-a) + b, as the reference forms them.
template <typename T>
__device__ __forceinline__ void binary_one(int op, T s1, T n1, bool h1, T s2, T n2, bool h2, T& so, T& no) {
    switch (op) {
        case SSFM_SIGNAL_ADD:
            so = s1 + s2;
            no = h1 ? (h2 ? n1 + n2 : n1) : n2;
            break;
        case SSFM_SIGNAL_SUB:
            so = s1 + (-s2);
            no = h1 ? (h2 ? n1 + (-n2) : n1) : -n2;
            break;
        case SSFM_SIGNAL_RSUB:
            so = (-s1) + s2;
            no = h1 ? (h2 ? (-n1) + n2 : -n1) : n2;
            break;
        default:        // SSFM_SIGNAL_MUL: s1 n2 + n1 s2 + n1 n2, summed in that order
            so = s1 * s2;
            if (h2) {
                no = s1 * n2;
                if (h1) {
                    no = no + n1 * s2;
                    no = no + n1 * n2;
                }
            } else {
                no = n1 * s2;
            }
            break;
    }
}

template <typename T, bool C1, bool C2>
__device__ __forceinline__ void binary_at(int op, long long i, const Operand& a, const Operand& b, double* out_s, double* out_n, unsigned char* out_b) {
    const bool h1 = a.n != nullptr, h2 = b.n != nullptr;
    const T s1 = load<T, C1>(a.s, i, a.len);
    const T s2 = b.s ? load<T, C2>(b.s, i, b.len) : splat<T>(b.re, b.im);
    const T n1 = h1 ? load<T, C1>(a.n, i, a.len) : splat<T>(0.0, 0.0);
    const T n2 = h2 ? load<T, C2>(b.n, i, b.len) : splat<T>(0.0, 0.0);
    if (op == SSFM_SIGNAL_GT || op == SSFM_SIGNAL_EQ) {
        const T x = h1 ? s1 + n1 : s1, y = h2 ? s2 + n2 : s2;
        if constexpr (__is_same(T, r2)) {
            const unsigned lo = op == SSFM_SIGNAL_GT ? gt(x.x, y.x) : eq(x.x, y.x), hi = op == SSFM_SIGNAL_GT ? gt(x.y, y.y) : eq(x.y, y.y);
            reinterpret_cast<unsigned short*>(out_b)[i] = (unsigned short)(lo | (hi << 8));
        } else {
            out_b[i] = op == SSFM_SIGNAL_GT ? gt(x, y) : eq(x, y);
        }
        return;
    }
    T so, no;
    binary_one<T>(op, s1, n1, h1, s2, n2, h2, so, no);
    store<T>(out_s, i, so);
    if (out_n) store<T>(out_n, i, no);
}

// complex128 result: one value per lane and pass
template <bool C1, bool C2>
__global__ __launch_bounds__(256) void k_signal_binary_c(int op, long long n, Operand a, Operand b, double* __restrict__ out_s, double* __restrict__ out_n,
                                                         unsigned char* __restrict__ out_b) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        binary_at<cd, C1, C2>(op, i, a, b, out_s, out_n, out_b);
}
// float64 result: two values per lane and pass, the odd last one by the first lane
__global__ __launch_bounds__(256) void k_signal_binary_r(int op, long long n, Operand a, Operand b, double* __restrict__ out_s, double* __restrict__ out_n,
                                                         unsigned char* __restrict__ out_b) {
    const long long first = (long long)blockIdx.x * blockDim.x + threadIdx.x, pairs = n >> 1;
    for (long long i = first; i < pairs; i += (long long)gridDim.x * blockDim.x) binary_at<r2, false, false>(op, i, a, b, out_s, out_n, out_b);
    if ((n & 1) && first == 0) binary_at<double, false, false>(op, n - 1, a, b, out_s, out_n, out_b);
}

// ---------------------------------------------------------------------------------------------- unary and scalar operations
__device__ __forceinline__ double pow_real(double x, double p) {
    // NumPy's fast paths of `array ** scalar`: 0.5 is sqrt, -1 is the reciprocal; everything else is pow
    if (p == 0.5) return sqrt(x);
    if (p == -1.0) return 1.0 / x;
    return pow(x, p);
}
// NumPy's complex power for an integer exponent |k| < 100: -1 is NumPy's reciprocal loop (what `array ** -1` calls); a zero base gives 0 (k > 0) or
// NaN + NaN j (k < 0); 1, 2, 3 are products, the others go by squaring, a negative one by the quotient 1 / r
__device__ __forceinline__ cd pow_int(cd a, int k) {
    if (k == -1) {
        if (fabs(a.im) <= fabs(a.re)) {
            const double r = a.im / a.re, d = a.re + a.im * r;
            return {1.0 / d, -r / d};
        }
        const double r = a.re / a.im, d = a.re * r + a.im;
        return {r / d, -1.0 / d};
    }
    if (a.re == 0.0 && a.im == 0.0) {
        if (k > 0) return {0.0, 0.0};
        const double nan = __builtin_nan("");
        return {nan, nan};
    }
    if (k == 1) return a;
    if (k == 2) return a * a;
    if (k == 3) return (a * a) * a;
    cd aa = {1.0, 0.0}, p = a;
    int mask = 1;
    const int m = k < 0 ? -k : k;
    while (true) {
        if (m & mask) aa = aa * p;
        mask <<= 1;
        if (m < mask || mask <= 0) break;
        p = p * p;
    }
    return k < 0 ? cdiv(cd{1.0, 0.0}, aa) : aa;
}
// The principal square root (what `complex128 ** 0.5` is in NumPy: its sqrt loop, C99's csqrt): the special values of C99 Annex G first, then
// t = sqrt((|re| + |z|) / 2) and (t, im / 2t) or its mirror image
__device__ __forceinline__ cd csqrt_(cd a) {
    if (a.re == 0.0 && a.im == 0.0) return {0.0, a.im};
    if (isinf(a.im)) return {__builtin_inf(), a.im};
    if (isnan(a.re)) return {a.re, (a.im - a.im) / (a.im - a.im)};
    if (isinf(a.re)) {
        if (signbit(a.re)) return {fabs(a.im - a.im), copysign(a.re, a.im)};
        return {a.re, copysign(a.im - a.im, a.im)};
    }
    const double t = sqrt((fabs(a.re) + hypot(a.re, a.im)) * 0.5);
    if (a.re >= 0.0) return {t, a.im / (2.0 * t)};
    return {fabs(a.im) / (2.0 * t), copysign(t, a.im)};
}
__device__ __forceinline__ double absv(double a) { return fabs(a); }
__device__ __forceinline__ double absv(cd a) { return hypot(a.re, a.im); }

// float64 -> float64 operations on one value
__device__ __forceinline__ double unary_rr(int op, double v, double p) {
    switch (op) {
        case SSFM_SIGNAL_NEG:      return -v;
        case SSFM_SIGNAL_DIV:      return v / p;
        case SSFM_SIGNAL_FLOORDIV: return floor(v / p);
        case SSFM_SIGNAL_IMAG:     return 0.0;
        case SSFM_SIGNAL_ABS_SIGNAL: case SSFM_SIGNAL_ABS_NOISE: case SSFM_SIGNAL_ABS_ALL: return fabs(v);
        case SSFM_SIGNAL_POW:      return pow_real(v, p);
        default:                   return v;        // CONJ, REAL: the value itself
    }
}

// float64 input, float64 output: two values per lane.  POW2: s^2 and 2 s n + n^2 (typing.py:1412-1414); POW / ABS_ALL: of s + n, no noise out;
// ABS_NOISE: of the noise alone
__global__ __launch_bounds__(256) void k_signal_unary_r(int op, long long n, const double* __restrict__ s, const double* __restrict__ nz, double p,
                                                        double* __restrict__ out_s, double* __restrict__ out_n) {
    const long long first = (long long)blockIdx.x * blockDim.x + threadIdx.x, pairs = n >> 1;
    const bool sum = op == SSFM_SIGNAL_POW || op == SSFM_SIGNAL_ABS_ALL, tail = (n & 1) && first == 0;
    for (long long i = first; i < pairs; i += (long long)gridDim.x * blockDim.x) {
        r2 a = load<r2, false>(op == SSFM_SIGNAL_ABS_NOISE ? nz : s, i, n), b = {0.0, 0.0};
        if (nz && op != SSFM_SIGNAL_ABS_NOISE) b = load<r2, false>(nz, i, n);
        if (sum && nz) a = a + b;
        if (op == SSFM_SIGNAL_POW2) {
            store<r2>(out_s, i, a * a);
            if (out_n) store<r2>(out_n, i, (r2{2.0, 2.0} * a) * b + b * b);
            continue;
        }
        store<r2>(out_s, i, r2{unary_rr(op, a.x, p), unary_rr(op, a.y, p)});
        if (out_n) store<r2>(out_n, i, r2{unary_rr(op, b.x, p), unary_rr(op, b.y, p)});
    }
    if (tail) {
        const long long i = n - 1;
        double a = (op == SSFM_SIGNAL_ABS_NOISE ? nz : s)[i], b = 0.0;
        if (nz && op != SSFM_SIGNAL_ABS_NOISE) b = nz[i];
        if (sum && nz) a = a + b;
        if (op == SSFM_SIGNAL_POW2) {
            out_s[i] = a * a;
            if (out_n) out_n[i] = (2.0 * a) * b + b * b;
        } else {
            out_s[i] = unary_rr(op, a, p);
            if (out_n) out_n[i] = unary_rr(op, b, p);
        }
    }
}

// complex128 result (C: the input is complex128; a float64 input only for the division by a complex scalar)
template <bool C>
__global__ __launch_bounds__(256) void k_signal_unary_c(int op, long long n, const double* __restrict__ s, const double* __restrict__ nz, cd p, int k,
                                                        double* __restrict__ out_s, double* __restrict__ out_n) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        cd a = load<cd, C>(s, i, n), b = {0.0, 0.0};
        if (nz) b = load<cd, C>(nz, i, n);
        cd ra, rb = {0.0, 0.0};
        switch (op) {
            case SSFM_SIGNAL_NEG:  ra = -a; rb = -b; break;
            case SSFM_SIGNAL_CONJ: ra = {a.re, -a.im}; rb = {b.re, -b.im}; break;
            case SSFM_SIGNAL_DIV:  ra = cdiv(a, p); if (nz) rb = cdiv(b, p); break;
            case SSFM_SIGNAL_POW2: ra = a * a; rb = (cd{2.0, 0.0} * a) * b + b * b; break;
            default:               ra = k ? pow_int(nz ? a + b : a, k) : csqrt_(nz ? a + b : a); break;        // POW (k = 0: the exponent 0.5)
        }
        store<cd>(out_s, i, ra);
        if (out_n) store<cd>(out_n, i, rb);
    }
}

// complex128 input, float64 result: |s|, |n|, |s + n|, the real and the imaginary parts
__global__ __launch_bounds__(256) void k_signal_unary_cr(int op, long long n, const double* __restrict__ s, const double* __restrict__ nz,
                                                         double* __restrict__ out_s, double* __restrict__ out_n) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        cd a = load<cd, true>(op == SSFM_SIGNAL_ABS_NOISE ? nz : s, i, n), b = {0.0, 0.0};
        if (nz && op != SSFM_SIGNAL_ABS_NOISE) b = load<cd, true>(nz, i, n);
        switch (op) {
            case SSFM_SIGNAL_REAL: out_s[i] = a.re; if (out_n) out_n[i] = b.re; break;
            case SSFM_SIGNAL_IMAG: out_s[i] = a.im; if (out_n) out_n[i] = b.im; break;
            case SSFM_SIGNAL_ABS_ALL: out_s[i] = absv(nz ? a + b : a); break;
            default: out_s[i] = absv(a); break;     // ABS_SIGNAL, ABS_NOISE
        }
    }
}

// ---------------------------------------------------------------------------------------------- reductions
// One pair of partial sums per workgroup: lanes by shuffles, the four wavefronts through four LDS words (the scheme of k_sum / k_min in
// device_mem.hip).  The grid depends on n alone and the host folds the partials in order, so a result is the same bits every time.
__device__ __forceinline__ double fold_max(double acc, double v) { return (v > acc || isnan(v)) ? v : acc; }        // a NaN stays, as in numpy.max

// One row: `s` (and `nz`) of n values.  A float64 row that starts off 16 bytes (row 1 of a (2, n) field with odd n) gives its first value to
// the lane that also takes the odd last one, so that every pair is read from an aligned address.
__device__ __forceinline__ void reduce_row(int kind, int cplx, const double* __restrict__ s, const double* __restrict__ nz, long long n,
                                           double* __restrict__ partial) {
    double a0 = 0.0, a1 = 0.0;
    const long long first = (long long)blockIdx.x * blockDim.x + threadIdx.x, stride = (long long)gridDim.x * blockDim.x;
    auto take = [&](double re, double im) {
        if (kind == SSFM_SIGNAL_POWER) a0 += cplx ? re * re + im * im : re * re;
        else if (kind == SSFM_SIGNAL_MAXABS) a0 = fold_max(a0, cplx ? hypot(re, im) : fabs(re));
        else { a0 += re; a1 += im; }
    };
    if (cplx) {
        for (long long i = first; i < n; i += stride) {
            cd v = load<cd, true>(s, i, n);
            if (nz) v = v + load<cd, true>(nz, i, n);
            take(v.re, v.im);
        }
    } else {
        const long long head = (reinterpret_cast<uintptr_t>(s) & 15) ? 1 : 0;
        for (long long i = first; i < ((n - head) >> 1); i += stride) {
            r2 v = load<r2, false>(s + head, i, 2);
            if (nz) v = v + load<r2, false>(nz + head, i, 2);
            take(v.x, 0.0);
            take(v.y, 0.0);
        }
        if (first == 0) {
            if (head) take(nz ? s[0] + nz[0] : s[0], 0.0);
            if ((n - head) & 1) take(nz ? s[n - 1] + nz[n - 1] : s[n - 1], 0.0);
        }
    }
    const bool is_max = kind == SSFM_SIGNAL_MAXABS;
    for (int o = 32; o > 0; o >>= 1) {
        const double b0 = __shfl_xor(a0, o), b1 = __shfl_xor(a1, o);
        a0 = is_max ? fold_max(a0, b0) : a0 + b0;
        a1 += b1;
    }
    __shared__ double w[8];
    if ((threadIdx.x & 63) == 0) { w[threadIdx.x >> 6] = a0; w[4 + (threadIdx.x >> 6)] = a1; }
    __syncthreads();
    if (threadIdx.x == 0) {
        partial[2 * blockIdx.x] = is_max ? fold_max(fold_max(w[0], w[1]), fold_max(w[2], w[3])) : w[0] + w[1] + w[2] + w[3];
        partial[2 * blockIdx.x + 1] = w[4] + w[5] + w[6] + w[7];
    }
}
// blockIdx.y: the row of a (rows, n) field (a signal is the field of one row); its partials follow those of the rows before it
__global__ __launch_bounds__(256) void k_field_reduce(int kind, int cplx, const double* __restrict__ s, const double* __restrict__ nz, long long n,
                                                      double* __restrict__ partial) {
    const long long off = (long long)blockIdx.y * n * (cplx ? 2 : 1);
    reduce_row(kind, cplx, s + off, nz ? nz + off : nullptr, n, partial + 2ll * blockIdx.y * gridDim.x);
}

// ---------------------------------------------------------------------------------------------- phase
constexpr double kPi = 3.141592653589793, kTwoPi = 6.283185307179586;

__global__ __launch_bounds__(256) void k_signal_angle(int cplx, const double* __restrict__ s, const double* __restrict__ nz, long long n, double* __restrict__ ang) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        cd v = cplx ? load<cd, true>(s, i, n) : load<cd, false>(s, i, n);
        if (nz) v = v + (cplx ? load<cd, true>(nz, i, n) : load<cd, false>(nz, i, n));
        ang[i] = atan2(v.im, v.re);
    }
}
// wraps[i] = the multiple of 2 pi that numpy.unwrap adds to the step ang[i] - ang[i - 1], decided by NumPy's own expressions in float64:
// ddmod = mod(dd + pi, 2 pi) - pi, with ddmod = pi where it is -pi and dd > 0; no correction where |dd| < pi.  An integer in {-1, 0, 1}, kept as
// a float64 so that ssfm_device_cumsum scans it: sums of integers below 2^53 are exact however the scan groups them.
__global__ __launch_bounds__(256) void k_signal_wraps(const double* __restrict__ ang, long long n, double* __restrict__ wraps) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        double k = 0.0;
        if (i > 0) {
            const double dd = ang[i] - ang[i - 1];
            if (!(fabs(dd) < kPi)) {
                double m = fmod(dd + kPi, kTwoPi);          // numpy.mod: the sign of the divisor
                if (m != 0.0 && m < 0.0) m += kTwoPi;
                double ddmod = m - kPi;
                if (ddmod == -kPi && dd > 0.0) ddmod = kPi;
                k = rint((ddmod - dd) / kTwoPi);            // (NaN stays NaN: the phase from there on is NaN, as NumPy's)
            }
        }
        wraps[i] = k;
    }
}
__global__ __launch_bounds__(256) void k_signal_unwrap(double* __restrict__ ang, const double* __restrict__ turns, long long n) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) ang[i] = ang[i] + kTwoPi * turns[i];
}

// ---------------------------------------------------------------------------------------------- the ends of filter()
__global__ __launch_bounds__(256) void k_signal_pack(const double* __restrict__ re, const double* __restrict__ im, long long n, double2* __restrict__ out) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) out[i] = make_double2(re[i], im[i]);
}
__global__ __launch_bounds__(256) void k_signal_split(const double2* __restrict__ src, long long n, double* __restrict__ re, double* __restrict__ im) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const double2 v = src[i];
        re[i] = v.x;
        if (im) im[i] = v.y;
    }
}

// ---------------------------------------------------------------------------------------------- optical fields
// (rows, n) arrays, rows = 1 or 2, C-contiguous: row 1 starts n values after row 0 (typing.py:2103-2320).  T is double, cd or cf.  An operand
// has its own (rows, len) with rows in {1, the result's} and len in {1, n}: a single row serves both rows, a single value a whole row.
// cd: one value per lane and pass.  double and cf: two (16 bytes).  For odd n row 1 of those starts 8 bytes off a 16-byte boundary: the row's
// first value is peeled (the first lane takes it with the odd last one), so that the pairs of the result, and of every operand of the
// result's shape, lie on 16-byte boundaries; an operand of another shape whose pair does not is read as two values.  The choice depends on
// the row alone, never on the lane.
struct FieldOperand {
    const void* s;
    const void* n;
    long long rows, len;
    double re, im;
};
template <typename T> struct alignas(16) two { T a, b; };

template <typename T> __device__ __forceinline__ T scalar_as(double re, double im) {
    if constexpr (sizeof(T) == sizeof(double) && !__is_same(T, cf)) return re;
    else if constexpr (__is_same(T, cf)) return {(float)re, (float)im};
    else return {re, im};
}
__device__ __forceinline__ bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
// values c, c + 1 of a row of `len` values
template <typename T> __device__ __forceinline__ void fetch2(const T* row, long long c, long long len, T& x, T& y) {
    if (len == 1) { x = y = row[0]; return; }
    const T* q = row + c;
    if (aligned16(q)) {
        const two<T> v = *reinterpret_cast<const two<T>*>(q);
        x = v.a; y = v.b;
    } else {
        x = q[0]; y = q[1];
    }
}
template <typename T> __device__ __forceinline__ void put2(T* row, long long c, T x, T y) {
    T* q = row + c;
    if (aligned16(q)) *reinterpret_cast<two<T>*>(q) = two<T>{x, y};
    else { q[0] = x; q[1] = y; }
}

// W values (1 or 2) from column c on of one row
template <typename T, int W>
__device__ __forceinline__ void field_binary_at(int op, long long c, const T* s1, const T* n1, long long len1, const T* s2, const T* n2, long long len2, T scalar,
                                                T* os, T* on, unsigned char* ob) {
    const bool h1 = n1 != nullptr, h2 = n2 != nullptr;
    T a[2], an[2], b[2], bn[2];
    const T zero = scalar_as<T>(0.0, 0.0);
    an[0] = an[1] = bn[0] = bn[1] = zero;
    b[0] = b[1] = scalar;
    if constexpr (W == 2) {
        fetch2<T>(s1, c, len1, a[0], a[1]);
        if (h1) fetch2<T>(n1, c, len1, an[0], an[1]);
        if (s2) fetch2<T>(s2, c, len2, b[0], b[1]);
        if (h2) fetch2<T>(n2, c, len2, bn[0], bn[1]);
    } else {
        a[0] = s1[len1 == 1 ? 0 : c];
        if (h1) an[0] = n1[len1 == 1 ? 0 : c];
        if (s2) b[0] = s2[len2 == 1 ? 0 : c];
        if (h2) bn[0] = n2[len2 == 1 ? 0 : c];
    }
    if (op == SSFM_SIGNAL_EQ) {
#pragma unroll
        for (int k = 0; k < W; ++k) ob[c + k] = eq(h1 ? a[k] + an[k] : a[k], h2 ? b[k] + bn[k] : b[k]);
        return;
    }
    T so[2], no[2];
#pragma unroll
    for (int k = 0; k < W; ++k) binary_one<T>(op, a[k], an[k], h1, b[k], bn[k], h2, so[k], no[k]);
    if constexpr (W == 2) {
        put2<T>(os, c, so[0], so[1]);
        if (on) put2<T>(on, c, no[0], no[1]);
    } else {
        os[c] = so[0];
        if (on) on[c] = no[0];
    }
}

template <typename T>
__global__ __launch_bounds__(256) void k_field_binary(int op, long long n, FieldOperand a, FieldOperand b, T* __restrict__ out_s, T* __restrict__ out_n,
                                                      unsigned char* __restrict__ out_b) {
    const long long r = blockIdx.y, first = (long long)blockIdx.x * blockDim.x + threadIdx.x, stride = (long long)gridDim.x * blockDim.x;
    const long long o1 = (a.rows == 1 ? 0 : r) * a.len, o2 = (b.rows == 1 ? 0 : r) * b.len;
    const T* s1 = (const T*)a.s + o1;
    const T* n1 = a.n ? (const T*)a.n + o1 : nullptr;
    const T* s2 = b.s ? (const T*)b.s + o2 : nullptr;
    const T* n2 = b.n ? (const T*)b.n + o2 : nullptr;
    T* os = out_s ? out_s + r * n : nullptr;
    T* on = out_n ? out_n + r * n : nullptr;
    unsigned char* ob = out_b ? out_b + r * n : nullptr;
    const T scalar = scalar_as<T>(b.re, b.im);
    if constexpr (sizeof(T) == 16) {
        for (long long c = first; c < n; c += stride) field_binary_at<T, 1>(op, c, s1, n1, a.len, s2, n2, b.len, scalar, os, on, ob);
    } else {
        const long long head = (r * n) & 1, pairs = (n - head) >> 1;
        for (long long i = first; i < pairs; i += stride) field_binary_at<T, 2>(op, head + 2 * i, s1, n1, a.len, s2, n2, b.len, scalar, os, on, ob);
        if (first == 0) {
            if (head) field_binary_at<T, 1>(op, 0, s1, n1, a.len, s2, n2, b.len, scalar, os, on, ob);
            if ((n - head) & 1) field_binary_at<T, 1>(op, n - 1, s1, n1, a.len, s2, n2, b.len, scalar, os, on, ob);
        }
    }
}

// complex64, `count` values in a row (a whole contiguous field): -x, conj(x), x / p in single precision
__global__ __launch_bounds__(256) void k_field_unary_cf(int op, long long count, const cf* __restrict__ s, const cf* __restrict__ nz, cf p, cf* __restrict__ out_s,
                                                        cf* __restrict__ out_n) {
    const long long first = (long long)blockIdx.x * blockDim.x + threadIdx.x, stride = (long long)gridDim.x * blockDim.x;
    auto one = [&](cf v) -> cf {
        if (op == SSFM_SIGNAL_NEG) return -v;
        if (op == SSFM_SIGNAL_CONJ) return {v.re, -v.im};
        return cdiv(v, p);
    };
    for (long long i = first; i < (count >> 1); i += stride) {
        cf x, y;
        fetch2<cf>(s, 2 * i, count, x, y);
        put2<cf>(out_s, 2 * i, one(x), one(y));
        if (nz) {
            fetch2<cf>(nz, 2 * i, count, x, y);
            put2<cf>(out_n, 2 * i, one(x), one(y));
        }
    }
    if ((count & 1) && first == 0) {
        out_s[count - 1] = one(s[count - 1]);
        if (nz) out_n[count - 1] = one(nz[count - 1]);
    }
}

// ---------------------------------------------------------------------------------------------- slicing
// out[r][i] = in[row0 + r][start + i step] of signal and noise (typing.py:1366-1376, :2261-2305; a signal is row 0 of one row); T: a value of 8 or
// of 16 bytes
template <typename T>
__global__ __launch_bounds__(256) void k_field_slice(const T* __restrict__ s, const T* __restrict__ nz, long long n, long long row0, long long start, long long step,
                                                     long long count, T* __restrict__ out_s, T* __restrict__ out_n) {
    const long long src = (row0 + blockIdx.y) * n + start, dst = (long long)blockIdx.y * count;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (long long)gridDim.x * blockDim.x) {
        out_s[dst + i] = s[src + i * step];
        if (nz) out_n[dst + i] = nz[src + i * step];
    }
}

int finish(const char* what) {
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return fail(SSFM_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
    return SSFM_OK;
}

// These entry points take no device number: a signal is computed where it lies, so the device is the one that owns the signal's memory (and a
// pointer that is not device memory is refused before anything is launched).  It becomes the calling thread's device.
int device_of(const void* p, int* device) { return ssfm::device_of(p, "ssfm_signal_*", device); }
bool same_device(const void* p, int device) {
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return attr.type == hipMemoryTypeDevice && attr.device == device;
}

bool operand_ok(const void* s, const void* nz, int64_t len, int64_t n) { return s ? (len == n || len == 1) : nz == nullptr; }

// the per-workgroup partials of one row, folded in order on the host
void fold_partials(int kind, const double* host, int blocks, int64_t n, double* out) {
    double a0 = 0.0, a1 = 0.0;
    for (int i = 0; i < blocks; ++i) {
        const double v = host[2 * i];
        if (kind == SSFM_SIGNAL_MAXABS) a0 = (v > a0 || v != v) ? v : a0;
        else a0 += v;
        a1 += host[2 * i + 1];
    }
    if (kind == SSFM_SIGNAL_POWER) a0 /= (double)n;
    out[0] = a0;
    if (kind == SSFM_SIGNAL_SUM) out[1] = a1;
}

// ssfm_signal_reduce and ssfm_field_reduce behind their own checks: every row of a (rows, n) array in one launch of k_field_reduce, the partials
// read back and folded, two results per row.  The grid depends on n alone, so a row's result does not depend on how many rows there are.
int reduce_rows(const char* what, int device, int kind, int64_t rows, int64_t n, const void* signal, const void* noise, int is_complex, double* out) {
    constexpr int kBlocks = 1024, kMaxRows = 2;
    const int blocks = (int)grid_for(is_complex ? n : (n + 1) / 2, kBlocks);
    const size_t bytes = sizeof(double) * 2 * kBlocks * rows;
    double* partial = nullptr;
    if (int rc = ssfm_device_alloc(device, bytes, (void**)&partial)) return rc;
    hipLaunchKernelGGL(k_field_reduce, dim3(blocks, (unsigned)rows), dim3(256), 0, 0, kind, is_complex, (const double*)signal, (const double*)noise, (long long)n, partial);
    static thread_local double host[2 * kBlocks * kMaxRows];
    hipError_t e = hipMemcpy(host, partial, sizeof(double) * 2 * blocks * rows, hipMemcpyDeviceToHost);
    (void)ssfm_device_free(device, partial, bytes);
    if (e != hipSuccess) return fail(SSFM_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
    for (int64_t r = 0; r < rows; ++r) fold_partials(kind, host + 2 * blocks * r, blocks, n, out + 2 * r);
    return SSFM_OK;
}

}  // namespace

extern "C" int ssfm_signal_binary(int op, int64_t rows, int64_t n, const void* s1, const void* n1, int64_t len1, int complex1, const void* s2,
                                  const void* n2, int64_t len2, int complex2, double re2, double im2, void* out_signal, void* out_noise) {
    if (rows != 1 || n < 1 || !s1 || !out_signal || op < SSFM_SIGNAL_ADD || op > SSFM_SIGNAL_EQ || !operand_ok(s1, n1, len1, n) || !operand_ok(s2, n2, len2, n))
        return fail(SSFM_ERR_INVALID, "ssfm_signal_binary: op=%d rows=%lld n=%lld len1=%lld len2=%lld (rows = 1; lengths n or 1)", op, (long long)rows, (long long)n,
                    (long long)len1, (long long)len2);
    const bool compare = op == SSFM_SIGNAL_GT || op == SSFM_SIGNAL_EQ;
    const bool want_noise = n1 || n2;
    if (!compare && (want_noise != (out_noise != nullptr))) return fail(SSFM_ERR_INVALID, "ssfm_signal_binary: out_noise is needed exactly when an operand has noise");
    int device = 0;
    if (int rc = device_of(s1, &device)) return rc;
    if (s2 && !same_device(s2, device)) return fail(SSFM_ERR_INVALID, "ssfm_signal_binary: the operands lie on different devices");
    const Operand a = {(const double*)s1, (const double*)n1, (long long)len1, 0.0, 0.0};
    const Operand b = {(const double*)s2, (const double*)n2, s2 ? (long long)len2 : 1, re2, im2};
    double* os = compare ? nullptr : (double*)out_signal;
    double* on = compare ? nullptr : (double*)out_noise;
    unsigned char* ob = compare ? (unsigned char*)out_signal : nullptr;
    const bool c1 = complex1 != 0, c2 = complex2 != 0;
    if (!c1 && !c2) {
        hipLaunchKernelGGL(k_signal_binary_r, dim3(grid_for((n + 1) / 2, kGridCap)), dim3(256), 0, 0, op, (long long)n, a, b, os, on, ob);
    } else {
        const dim3 grid(grid_for(n, kGridCap));
        if (c1 && c2) hipLaunchKernelGGL((k_signal_binary_c<true, true>), grid, dim3(256), 0, 0, op, (long long)n, a, b, os, on, ob);
        else if (c1) hipLaunchKernelGGL((k_signal_binary_c<true, false>), grid, dim3(256), 0, 0, op, (long long)n, a, b, os, on, ob);
        else hipLaunchKernelGGL((k_signal_binary_c<false, true>), grid, dim3(256), 0, 0, op, (long long)n, a, b, os, on, ob);
    }
    return finish("ssfm_signal_binary");
}

extern "C" int ssfm_signal_unary(int op, int64_t rows, int64_t n, const void* signal, const void* noise, int is_complex, double p_re, double p_im,
                                 int p_complex, void* out_signal, void* out_noise) {
    if (rows != 1 || n < 1 || !signal || !out_signal || op < SSFM_SIGNAL_NEG || op > SSFM_SIGNAL_POW)
        return fail(SSFM_ERR_INVALID, "ssfm_signal_unary: op=%d rows=%lld n=%lld (rows = 1)", op, (long long)rows, (long long)n);
    const bool single = op == SSFM_SIGNAL_ABS_SIGNAL || op == SSFM_SIGNAL_ABS_NOISE || op == SSFM_SIGNAL_ABS_ALL || op == SSFM_SIGNAL_POW;
    if (single ? out_noise != nullptr : (noise != nullptr) != (out_noise != nullptr))
        return fail(SSFM_ERR_INVALID, "ssfm_signal_unary: op=%d takes out_noise %s", op, single ? "never" : "exactly with noise");
    if (op == SSFM_SIGNAL_ABS_NOISE && !noise) return fail(SSFM_ERR_INVALID, "ssfm_signal_unary: |noise| of a signal without noise");
    if ((op == SSFM_SIGNAL_DIV || op == SSFM_SIGNAL_FLOORDIV) && p_re == 0.0 && (!p_complex || p_im == 0.0))
        return fail(SSFM_ERR_INVALID, "ssfm_signal_unary: division by zero");
    const bool cplx = is_complex != 0, pc = p_complex != 0;
    if (op == SSFM_SIGNAL_FLOORDIV && (cplx || pc)) return fail(SSFM_ERR_INVALID, "ssfm_signal_unary: floor of complex values");
    if (pc && op != SSFM_SIGNAL_DIV) return fail(SSFM_ERR_INVALID, "ssfm_signal_unary: op=%d takes a real parameter", op);
    int k = 0;
    if (op == SSFM_SIGNAL_POW && cplx) {
        if (p_re != 0.5 && (!(p_re == rint(p_re)) || fabs(p_re) >= 100.0 || p_re == 0.0))
            return fail(SSFM_ERR_UNSUPPORTED, "ssfm_signal_unary: complex128 ** %g (integer exponents 0 < |p| < 100, and 0.5, only)", p_re);
        k = p_re == 0.5 ? 0 : (int)p_re;
    }
    int device = 0;
    if (int rc = device_of(signal, &device)) return rc;
    const double* s = (const double*)signal;
    const double* nz = (const double*)noise;
    double* os = (double*)out_signal;
    double* on = (double*)out_noise;
    const dim3 grid(grid_for(n, kGridCap));
    const bool real_out = op == SSFM_SIGNAL_ABS_SIGNAL || op == SSFM_SIGNAL_ABS_NOISE || op == SSFM_SIGNAL_ABS_ALL || op == SSFM_SIGNAL_REAL || op == SSFM_SIGNAL_IMAG;
    if (!cplx && !(op == SSFM_SIGNAL_DIV && pc))
        hipLaunchKernelGGL(k_signal_unary_r, dim3(grid_for((n + 1) / 2, kGridCap)), dim3(256), 0, 0, op, (long long)n, s, nz, p_re, os, on);
    else if (!cplx)
        hipLaunchKernelGGL(k_signal_unary_c<false>, grid, dim3(256), 0, 0, op, (long long)n, s, nz, cd{p_re, p_im}, k, os, on);
    else if (real_out)
        hipLaunchKernelGGL(k_signal_unary_cr, grid, dim3(256), 0, 0, op, (long long)n, s, nz, os, on);
    else
        hipLaunchKernelGGL(k_signal_unary_c<true>, grid, dim3(256), 0, 0, op, (long long)n, s, nz, cd{p_re, pc ? p_im : 0.0}, k, os, on);
    return finish("ssfm_signal_unary");
}

extern "C" int ssfm_signal_slice(int64_t rows, int64_t n, const void* signal, const void* noise, int is_complex, int64_t start, int64_t step,
                                 int64_t count, void* out_signal, void* out_noise) {
    // every index read lies in [0, n): checked here, so that no key reaches the kernel that would read outside the arrays
    const int64_t last = start + (count - 1) * step;
    if (rows != 1 || n < 1 || !signal || !out_signal || count < 1 || step == 0 || start < 0 || start >= n || last < 0 || last >= n ||
        (noise != nullptr) != (out_noise != nullptr))
        return fail(SSFM_ERR_INVALID, "ssfm_signal_slice: rows=%lld n=%lld start=%lld step=%lld count=%lld", (long long)rows, (long long)n, (long long)start,
                    (long long)step, (long long)count);
    int device = 0;
    if (int rc = device_of(signal, &device)) return rc;
    const dim3 grid(grid_for(count, kGridCap));
    if (is_complex)
        hipLaunchKernelGGL(k_field_slice<double2>, grid, dim3(256), 0, 0, (const double2*)signal, (const double2*)noise, (long long)n, 0ll, (long long)start,
                           (long long)step, (long long)count, (double2*)out_signal, (double2*)out_noise);
    else
        hipLaunchKernelGGL(k_field_slice<double>, grid, dim3(256), 0, 0, (const double*)signal, (const double*)noise, (long long)n, 0ll, (long long)start,
                           (long long)step, (long long)count, (double*)out_signal, (double*)out_noise);
    return finish("ssfm_signal_slice");
}

extern "C" int ssfm_signal_reduce(int kind, int64_t rows, int64_t n, const void* signal, const void* noise, int is_complex, double* out) {
    if (rows != 1 || n < 1 || !signal || !out || kind < SSFM_SIGNAL_POWER || kind > SSFM_SIGNAL_SUM)
        return fail(SSFM_ERR_INVALID, "ssfm_signal_reduce: kind=%d rows=%lld n=%lld (rows = 1)", kind, (long long)rows, (long long)n);
    int device = 0;
    if (int rc = device_of(signal, &device)) return rc;
    if (kind == SSFM_SIGNAL_POWER && !noise)        // the power of one array is ssfm_device_reduce's
        return ssfm_device_reduce(device, SSFM_REDUCE_POWER, signal, nullptr, 1, n, is_complex, out);
    return reduce_rows("ssfm_signal_reduce", device, kind, 1, n, signal, noise, is_complex, out);
}

extern "C" int ssfm_signal_phase(int64_t rows, int64_t n, const void* signal, const void* noise, int is_complex, double* out) {
    if (rows != 1 || n < 1 || !signal || !out) return fail(SSFM_ERR_INVALID, "ssfm_signal_phase: rows=%lld n=%lld (rows = 1)", (long long)rows, (long long)n);
    int device = 0;
    if (int rc = device_of(signal, &device)) return rc;
    const dim3 grid(grid_for(n, kGridCap));
    hipLaunchKernelGGL(k_signal_angle, grid, dim3(256), 0, 0, is_complex, (const double*)signal, (const double*)noise, (long long)n, out);
    if (n == 1) return finish("ssfm_signal_phase");
    ssfm::Scratch scratch(device);
    double *wraps = nullptr, *turns = nullptr;
    if (int rc = scratch.get(sizeof(double) * n, (void**)&wraps)) return rc;
    if (int rc = scratch.get(sizeof(double) * n, (void**)&turns)) return rc;
    hipLaunchKernelGGL(k_signal_wraps, grid, dim3(256), 0, 0, (const double*)out, (long long)n, wraps);
    if (int rc = ssfm_device_cumsum(device, turns, wraps, n)) return rc;
    hipLaunchKernelGGL(k_signal_unwrap, grid, dim3(256), 0, 0, out, (const double*)turns, (long long)n);
    return finish("ssfm_signal_phase");
}

extern "C" int ssfm_signal_pack(const double* re, const double* im, int64_t n, void* out) {
    if (n < 1 || !re || !im || !out) return fail(SSFM_ERR_INVALID, "ssfm_signal_pack: bad argument");
    int device = 0;
    if (int rc = device_of(re, &device)) return rc;
    hipLaunchKernelGGL(k_signal_pack, dim3(grid_for(n, kGridCap)), dim3(256), 0, 0, re, im, (long long)n, (double2*)out);
    return finish("ssfm_signal_pack");
}

extern "C" int ssfm_signal_split(const void* src, int64_t n, double* re, double* im) {
    if (n < 1 || !src || !re) return fail(SSFM_ERR_INVALID, "ssfm_signal_split: bad argument");
    int device = 0;
    if (int rc = device_of(src, &device)) return rc;
    hipLaunchKernelGGL(k_signal_split, dim3(grid_for(n, kGridCap)), dim3(256), 0, 0, (const double2*)src, (long long)n, re, im);
    return finish("ssfm_signal_split");
}

// ---------------------------------------------------------------------------------------------- optical fields: entry points
namespace {
bool field_dtype_ok(int dtype) { return dtype == SSFM_C64 || dtype == SSFM_C128 || dtype == SSFM_F64_REAL; }
// an operand's shape against the result's: rows 1 or the result's, len 1 or n; a scalar (s == nullptr) has no noise
bool field_operand_ok(const void* s, const void* nz, int64_t rows_k, int64_t len_k, int64_t rows, int64_t n) {
    return s ? ((rows_k == 1 || rows_k == rows) && (len_k == 1 || len_k == n)) : nz == nullptr;
}
bool base_aligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
}  // namespace

extern "C" int ssfm_field_binary(int op, int dtype, int64_t rows, int64_t n, const void* s1, const void* n1, int64_t rows1, int64_t len1, const void* s2,
                                 const void* n2, int64_t rows2, int64_t len2, double re2, double im2, void* out_signal, void* out_noise) {
    const bool op_ok = op == SSFM_SIGNAL_ADD || op == SSFM_SIGNAL_SUB || op == SSFM_SIGNAL_RSUB || op == SSFM_SIGNAL_MUL || op == SSFM_SIGNAL_EQ;
    if (!s2) rows2 = len2 = 1;
    if (!op_ok || !field_dtype_ok(dtype) || (rows != 1 && rows != 2) || n < 1 || !s1 || !out_signal || !field_operand_ok(s1, n1, rows1, len1, rows, n) ||
        !field_operand_ok(s2, n2, rows2, len2, rows, n) || (rows1 != rows && rows2 != rows) || (len1 != n && len2 != n))
        return fail(SSFM_ERR_INVALID, "ssfm_field_binary: op=%d dtype=%d result (%lld, %lld), operands (%lld, %lld) and (%lld, %lld): rows 1 or 2, each operand "
                    "1 or the result's along either axis", op, dtype, (long long)rows, (long long)n, (long long)rows1, (long long)len1, (long long)rows2, (long long)len2);
    const bool compare = op == SSFM_SIGNAL_EQ;
    if (!compare && ((n1 || n2) != (out_noise != nullptr))) return fail(SSFM_ERR_INVALID, "ssfm_field_binary: out_noise is needed exactly when an operand has noise");
    if (!base_aligned(s1) || !base_aligned(n1) || !base_aligned(s2) || !base_aligned(n2) || !base_aligned(out_signal) || !base_aligned(out_noise))
        return fail(SSFM_ERR_INVALID, "ssfm_field_binary: an array does not start on a 16-byte boundary");
    int device = 0;
    if (int rc = ssfm::device_of(s1, "ssfm_field_*", &device)) return rc;
    for (const void* p : {n1, s2, n2, (const void*)out_signal, (const void*)out_noise})
        if (p && !same_device(p, device)) return fail(SSFM_ERR_INVALID, "ssfm_field_binary: the operands lie on different devices");
    const FieldOperand a = {s1, n1, (long long)rows1, (long long)len1, 0.0, 0.0};
    const FieldOperand b = {s2, n2, (long long)rows2, (long long)len2, re2, im2};
    void* os = compare ? nullptr : out_signal;
    void* on = compare ? nullptr : out_noise;
    unsigned char* ob = compare ? (unsigned char*)out_signal : nullptr;
    const dim3 grid(grid_for(dtype == SSFM_C128 ? n : (n + 1) / 2, kGridCap), (unsigned)rows);
    if (dtype == SSFM_C128) hipLaunchKernelGGL(k_field_binary<cd>, grid, dim3(256), 0, 0, op, (long long)n, a, b, (cd*)os, (cd*)on, ob);
    else if (dtype == SSFM_C64) hipLaunchKernelGGL(k_field_binary<cf>, grid, dim3(256), 0, 0, op, (long long)n, a, b, (cf*)os, (cf*)on, ob);
    else hipLaunchKernelGGL(k_field_binary<double>, grid, dim3(256), 0, 0, op, (long long)n, a, b, (double*)os, (double*)on, ob);
    return finish("ssfm_field_binary");
}

extern "C" int ssfm_field_unary(int op, int dtype, int64_t rows, int64_t n, const void* signal, const void* noise, double p_re, double p_im, int p_complex,
                                void* out_signal, void* out_noise) {
    if (!field_dtype_ok(dtype) || (rows != 1 && rows != 2) || n < 1 || !signal || !out_signal)
        return fail(SSFM_ERR_INVALID, "ssfm_field_unary: op=%d dtype=%d rows=%lld n=%lld (rows 1 or 2)", op, dtype, (long long)rows, (long long)n);
    // a pointwise operation does not see the rows of a contiguous field: the double-precision types are ssfm_signal_unary's, on rows * n values
    if (dtype != SSFM_C64) return ssfm_signal_unary(op, 1, rows * n, signal, noise, dtype == SSFM_C128, p_re, p_im, p_complex, out_signal, out_noise);
    if (op != SSFM_SIGNAL_NEG && op != SSFM_SIGNAL_CONJ && op != SSFM_SIGNAL_DIV)
        return fail(SSFM_ERR_UNSUPPORTED, "ssfm_field_unary: op=%d of complex64 values (neg, conj and the quotient only: widen the field for the others)", op);
    if ((noise != nullptr) != (out_noise != nullptr)) return fail(SSFM_ERR_INVALID, "ssfm_field_unary: op=%d takes out_noise exactly with noise", op);
    const cf p = {(float)p_re, p_complex ? (float)p_im : 0.0f};
    if (op == SSFM_SIGNAL_DIV && p.re == 0.0f && p.im == 0.0f) return fail(SSFM_ERR_INVALID, "ssfm_field_unary: division by zero");
    if (!base_aligned(signal) || !base_aligned(noise) || !base_aligned(out_signal) || !base_aligned(out_noise))
        return fail(SSFM_ERR_INVALID, "ssfm_field_unary: an array does not start on a 16-byte boundary");
    int device = 0;
    if (int rc = ssfm::device_of(signal, "ssfm_field_*", &device)) return rc;
    for (const void* p : {noise, (const void*)out_signal, (const void*)out_noise})
        if (p && !same_device(p, device)) return fail(SSFM_ERR_INVALID, "ssfm_field_unary: signal, noise and results lie on different devices, or in host memory");
    const long long count = rows * n;
    hipLaunchKernelGGL(k_field_unary_cf, dim3(grid_for((count + 1) / 2, kGridCap)), dim3(256), 0, 0, op, count, (const cf*)signal, (const cf*)noise, p, (cf*)out_signal,
                       (cf*)out_noise);
    return finish("ssfm_field_unary");
}

extern "C" int ssfm_field_slice(int dtype, int64_t rows, int64_t n, const void* signal, const void* noise, int64_t row0, int64_t nrows, int64_t start, int64_t step,
                                int64_t count, void* out_signal, void* out_noise) {
    // every row and column read lies inside the field: checked here, so that no key reaches the kernel that would read outside the arrays
    // (count and step are bounded by n before the last index is formed, so that no argument makes it overflow)
    // (one value: any step; more: a step of at most n either way)
    const bool span_ok = n >= 1 && n <= (int64_t(1) << 31) && count >= 1 && count <= n && step != 0 && (count == 1 || (step >= -n && step <= n)) && start >= 0 && start < n;
    const int64_t last = !span_ok ? -1 : (count == 1 ? start : start + (count - 1) * step);
    if (!field_dtype_ok(dtype) || (rows != 1 && rows != 2) || !span_ok || !signal || !out_signal || row0 < 0 || row0 > 1 || nrows < 1 || nrows > 2 || row0 + nrows > rows ||
        last < 0 || last >= n || (noise != nullptr) != (out_noise != nullptr))
        return fail(SSFM_ERR_INVALID, "ssfm_field_slice: dtype=%d rows=%lld n=%lld row0=%lld nrows=%lld start=%lld step=%lld count=%lld", dtype, (long long)rows,
                    (long long)n, (long long)row0, (long long)nrows, (long long)start, (long long)step, (long long)count);
    int device = 0;
    if (int rc = ssfm::device_of(signal, "ssfm_field_*", &device)) return rc;
    for (const void* p : {noise, (const void*)out_signal, (const void*)out_noise})
        if (p && !same_device(p, device)) return fail(SSFM_ERR_INVALID, "ssfm_field_slice: signal, noise and results lie on different devices, or in host memory");
    const dim3 grid(grid_for(count, kGridCap), (unsigned)nrows);
    if (dtype == SSFM_C128)
        hipLaunchKernelGGL(k_field_slice<double2>, grid, dim3(256), 0, 0, (const double2*)signal, (const double2*)noise, (long long)n, (long long)row0, (long long)start,
                           (long long)step, (long long)count, (double2*)out_signal, (double2*)out_noise);
    else        // 8 bytes: a float64 or a complex64 value
        hipLaunchKernelGGL(k_field_slice<double>, grid, dim3(256), 0, 0, (const double*)signal, (const double*)noise, (long long)n, (long long)row0, (long long)start,
                           (long long)step, (long long)count, (double*)out_signal, (double*)out_noise);
    return finish("ssfm_field_slice");
}

extern "C" int ssfm_field_reduce(int kind, int64_t rows, int64_t n, const void* signal, const void* noise, int is_complex, double* out) {
    if ((rows != 1 && rows != 2) || n < 1 || !signal || !out || kind < SSFM_SIGNAL_POWER || kind > SSFM_SIGNAL_SUM)
        return fail(SSFM_ERR_INVALID, "ssfm_field_reduce: kind=%d rows=%lld n=%lld (rows 1 or 2)", kind, (long long)rows, (long long)n);
    if (!base_aligned(signal) || !base_aligned(noise)) return fail(SSFM_ERR_INVALID, "ssfm_field_reduce: an array does not start on a 16-byte boundary");
    int device = 0;
    if (int rc = ssfm::device_of(signal, "ssfm_field_*", &device)) return rc;
    if (noise && !same_device(noise, device)) return fail(SSFM_ERR_INVALID, "ssfm_field_reduce: signal and noise lie on different devices");
    if (int rc = reduce_rows("ssfm_field_reduce", device, kind, rows, n, signal, noise, is_complex, out)) return rc;
    if (kind != SSFM_SIGNAL_SUM)        // (the second result of a row is the sum's imaginary part; 0 for the others)
        for (int64_t r = 0; r < rows; ++r) out[2 * r + 1] = 0.0;
    return SSFM_OK;
}
