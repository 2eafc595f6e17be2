// bits.hip -- the algebra of binary_sequence (reference typing.py:402-1009) on device-resident sequences: ~ & | ^ != (one kernel), concatenation
// and slices of step 1 (the same kernel as a copy), tiling, strided slices and the count of ones.  A sequence is one uint8 per bit; as in ppm.hip
// and sync.hip a nonzero byte counts as 1.  Every kernel here reads `v != 0` and writes exactly 0 or 1, so a result is always a valid sequence.
// Integers only: nothing in this file is a float.
//
// All of them stream: 16 bytes per lane and access, bytewise logic on the four dwords, a grid of at most 256 CUs x 8 workgroups with a grid-stride
// loop.  The vector stores are aligned: the bytes in front of the destination's first 16-byte boundary and behind its last one are written one per
// lane.  A source that does not share the destination's alignment (a concatenation writes at out + len_a, a slice reads at src + start, a tile of
// an odd period never lines up) is read with a 16-byte load at a byte address all the same (load16).  The count aligns its only
// pointer, sums popcounts per lane, folds a wavefront by shuffles and adds one 64-bit integer per workgroup to a zeroed counter: exact, and the
// same number whatever the order.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "ssfm_amd.h"
#include "ssfm_common.hpp"

using ssfm::fail;
using ssfm::grid_for;

namespace {

// [host-emulated: begin]  (tests/bits_host_emulation.cpp compiles the text up to the end mark for the host and runs every lane in turn)
constexpr long long kGridCap = 2048;        // 256 CUs x 8 workgroups
constexpr int kThreads = 256;
constexpr unsigned kOnes = 0x01010101u;
constexpr int kNot = 3, kCopy = 4;          // after SSFM_BITS_AND / _OR / _XOR: the unary forms of k_bits_map

// every byte of w: nonzero -> 1 (bit 0 of a byte becomes the OR of its eight bits; what the shifts carry in from the byte above lands in bits 1 ... 7)
__device__ __forceinline__ unsigned norm4(unsigned w) {
    w |= w >> 4;
    w |= w >> 2;
    w |= w >> 1;
    return w & kOnes;
}
__device__ __forceinline__ uint4 norm16(uint4 v) { return make_uint4(norm4(v.x), norm4(v.y), norm4(v.z), norm4(v.w)); }

// 16 bytes at any byte address: the compiler knows no alignment here, and since the target runs global loads in unaligned access mode it still
// emits ONE 16-byte load (an aligned address costs nothing extra, a misaligned one is the hardware's to split)
__device__ __forceinline__ uint4 load16(const unsigned char* p) {
    uint4 v;
    __builtin_memcpy(&v, p, sizeof(v));
    return v;
}

// on normalised dwords, or on single bits
template <int OP> __device__ __forceinline__ unsigned apply(unsigned x, unsigned y) {
    if constexpr (OP == SSFM_BITS_AND) return x & y;
    else if constexpr (OP == SSFM_BITS_OR) return x | y;
    else if constexpr (OP == SSFM_BITS_XOR) return x ^ y;
    else if constexpr (OP == kNot) return x ^ kOnes;
    else return x;
}

// One operand: `len` bytes at p; with len == 1 the one bit for every index (which is the bit itself in a result of one bit).
struct Src {
    const unsigned char* p;
    long long len;
};

// The split of n destination bytes at `out`: `head` bytes up to the first 16-byte boundary, `nvec` aligned vectors, the rest from `tail` on.
struct Split {
    long long head, nvec, tail;
    __device__ Split(const unsigned char* out, long long n) {
        head = (long long)((16 - (reinterpret_cast<uintptr_t>(out) & 15)) & 15);
        if (head > n) head = n;
        nvec = (n - head) >> 4;
        tail = head + (nvec << 4);
    }
    // the index of edge byte `k` (k < edges(n)): the head first, then the tail
    __device__ long long edges(long long n) const { return head + (n - tail); }
    __device__ long long edge(long long k) const { return k < head ? k : tail + (k - head); }
};

// out[i] = OP(a[i], b[i]), i < n (kNot, kCopy: of a alone; b.p = nullptr)
template <int OP>
__global__ __launch_bounds__(kThreads) void k_bits_map(Src a, Src b, long long n, unsigned char* __restrict__ out) {
    constexpr bool kTwo = OP <= SSFM_BITS_XOR;
    const long long gid = (long long)blockIdx.x * kThreads + threadIdx.x, stride = (long long)gridDim.x * kThreads;
    const Split sp(out, n);
    const bool one_a = a.len == 1, one_b = kTwo && b.len == 1;
    const unsigned bit_a = one_a ? (a.p[0] != 0) : 0u, bit_b = one_b ? (b.p[0] != 0) : 0u;
    for (long long v = gid; v < sp.nvec; v += stride) {
        const long long i = sp.head + (v << 4);
        const uint4 x = one_a ? make_uint4(bit_a * kOnes, bit_a * kOnes, bit_a * kOnes, bit_a * kOnes) : norm16(load16(a.p + i));
        uint4 y = make_uint4(bit_b * kOnes, bit_b * kOnes, bit_b * kOnes, bit_b * kOnes);
        if (kTwo && !one_b) y = norm16(load16(b.p + i));
        *reinterpret_cast<uint4*>(out + i) = make_uint4(apply<OP>(x.x, y.x), apply<OP>(x.y, y.y), apply<OP>(x.z, y.z), apply<OP>(x.w, y.w));
    }
    if (gid < sp.edges(n)) {
        const long long i = sp.edge(gid);
        const unsigned x = one_a ? bit_a : (a.p[i] != 0), y = (kTwo && !one_b) ? (b.p[i] != 0) : bit_b;
        out[i] = (unsigned char)(apply<OP>(x, y) & 1u);
    }
}

// out[i] = src[i mod period], i < total.  A lane's 16 bytes are one load where they do not cross the period's end, and 16 single bytes where they
// do (one vector in period / 16, every vector of a period below 16).  The lane's position in the period advances with the grid stride: two
// divisions per lane, none in the loop.
__global__ __launch_bounds__(kThreads) void k_bits_tile(const unsigned char* __restrict__ src, long long period, long long total, unsigned char* __restrict__ out) {
    const long long gid = (long long)blockIdx.x * kThreads + threadIdx.x, stride = (long long)gridDim.x * kThreads;
    const Split sp(out, total);
    long long s = (sp.head + (gid << 4)) % period;
    const long long hop = (stride << 4) % period;
    for (long long v = gid; v < sp.nvec; v += stride) {
        const long long i = sp.head + (v << 4);
        uint4 r;
        if (s + 16 <= period) {
            r = norm16(load16(src + s));
        } else {
            unsigned w[4] = {0u, 0u, 0u, 0u};
            long long t = s;
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                w[k >> 2] |= (unsigned)(src[t] != 0) << (8 * (k & 3));
                if (++t == period) t = 0;
            }
            r = make_uint4(w[0], w[1], w[2], w[3]);
        }
        *reinterpret_cast<uint4*>(out + i) = r;
        s += hop;
        if (s >= period) s -= period;
    }
    if (gid < sp.edges(total)) {
        const long long i = sp.edge(gid);
        out[i] = src[i % period] != 0;
    }
}

// out[i] = src[start + i step], i < count: a gather, one byte per lane
__global__ __launch_bounds__(kThreads) void k_bits_stride(const unsigned char* __restrict__ src, long long start, long long step, long long count,
                                                          unsigned char* __restrict__ out) {
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < count; i += (long long)gridDim.x * kThreads) out[i] = src[start + i * step] != 0;
}

// [host-emulated: end]

// *acc += the number of nonzero bytes of a[0 .. n)
__global__ __launch_bounds__(kThreads) void k_bits_count(const unsigned char* __restrict__ a, long long n, unsigned long long* __restrict__ acc) {
    const long long gid = (long long)blockIdx.x * kThreads + threadIdx.x, stride = (long long)gridDim.x * kThreads;
    const Split sp(a, n);
    unsigned long long c = 0;
    for (long long v = gid; v < sp.nvec; v += stride) {
        const uint4 x = norm16(*reinterpret_cast<const uint4*>(a + sp.head + (v << 4)));
        c += (unsigned)(__popc(x.x) + __popc(x.y) + __popc(x.z) + __popc(x.w));
    }
    if (gid < sp.edges(n)) c += a[sp.edge(gid)] != 0;
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    __shared__ unsigned long long w[kThreads / 64];
    if ((threadIdx.x & 63) == 0) w[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(acc, w[0] + w[1] + w[2] + w[3]);       // an integer atomic: the total does not depend on the order
}

int finish(const char* what) {
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return fail(SSFM_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
    return SSFM_OK;
}

// As ssfm_signal_*: no device number.  The work runs on the device that owns the first pointer, which becomes the calling thread's device; every
// other pointer must be device memory of that device, or nothing is launched.
int device_of(const void* p, int* device) { return ssfm::device_of(p, "ssfm_bits_*", device); }
bool same_device(const void* p, int device) {
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return attr.type == hipMemoryTypeDevice && attr.device == device;
}

// workgroups for n destination bytes: one lane per 16 bytes, and at least the 30 lanes the edge bytes take (one workgroup has them)
dim3 grid_bytes(long long n) { return dim3(grid_for((n + 15) / 16, kGridCap)); }

template <int OP> void launch_map(Src a, Src b, long long n, unsigned char* out) {
    hipLaunchKernelGGL(k_bits_map<OP>, grid_bytes(n), dim3(kThreads), 0, 0, a, b, n, out);
}

}  // namespace

extern "C" int ssfm_bits_binary(int op, const unsigned char* a, int64_t len_a, const unsigned char* b, int64_t len_b, int64_t n, unsigned char* out) {
    if (n < 0 || op < SSFM_BITS_AND || op > SSFM_BITS_XOR) return fail(SSFM_ERR_INVALID, "ssfm_bits_binary: op=%d n=%lld", op, (long long)n);
    if (n == 0) return SSFM_OK;
    if (!a || !b || !out || (len_a != n && len_a != 1) || (len_b != n && len_b != 1))
        return fail(SSFM_ERR_INVALID, "ssfm_bits_binary: n=%lld len_a=%lld len_b=%lld (lengths n or 1)", (long long)n, (long long)len_a, (long long)len_b);
    int device = 0;
    if (int rc = device_of(a, &device)) return rc;
    if (!same_device(b, device) || !same_device(out, device)) return fail(SSFM_ERR_INVALID, "ssfm_bits_binary: the operands and the result lie on different devices");
    const Src sa = {a, (long long)len_a}, sb = {b, (long long)len_b};
    if (op == SSFM_BITS_AND) launch_map<SSFM_BITS_AND>(sa, sb, n, out);
    else if (op == SSFM_BITS_OR) launch_map<SSFM_BITS_OR>(sa, sb, n, out);
    else launch_map<SSFM_BITS_XOR>(sa, sb, n, out);
    return finish("ssfm_bits_binary");
}

extern "C" int ssfm_bits_not(const unsigned char* a, int64_t n, unsigned char* out) {
    if (n < 0) return fail(SSFM_ERR_INVALID, "ssfm_bits_not: n=%lld", (long long)n);
    if (n == 0) return SSFM_OK;
    if (!a || !out) return fail(SSFM_ERR_INVALID, "ssfm_bits_not: NULL argument");
    int device = 0;
    if (int rc = device_of(a, &device)) return rc;
    if (!same_device(out, device)) return fail(SSFM_ERR_INVALID, "ssfm_bits_not: the operand and the result lie on different devices");
    launch_map<kNot>(Src{a, (long long)n}, Src{nullptr, 0}, n, out);
    return finish("ssfm_bits_not");
}

extern "C" int ssfm_bits_slice(const unsigned char* src, int64_t n, int64_t start, int64_t step, int64_t count, unsigned char* out) {
    if (n < 0 || count < 0 || step == 0 || step == INT64_MIN) return fail(SSFM_ERR_INVALID, "ssfm_bits_slice: n=%lld step=%lld count=%lld", (long long)n, (long long)step, (long long)count);
    if (count == 0) return SSFM_OK;
    // every index read lies in [0, n): checked here by divisions (no product that could overflow), so that no key reaches a kernel that would read
    // outside the sequence
    const bool inside = start >= 0 && start < n && count <= n &&
                        (count == 1 || (step > 0 ? (count - 1) <= (n - 1 - start) / step : (count - 1) <= start / -step));
    if (!src || !out || !inside)
        return fail(SSFM_ERR_INVALID, "ssfm_bits_slice: n=%lld start=%lld step=%lld count=%lld", (long long)n, (long long)start, (long long)step, (long long)count);
    int device = 0;
    if (int rc = device_of(src, &device)) return rc;
    if (!same_device(out, device)) return fail(SSFM_ERR_INVALID, "ssfm_bits_slice: the sequence and the result lie on different devices");
    if (step == 1)
        launch_map<kCopy>(Src{src + start, (long long)count}, Src{nullptr, 0}, count, out);
    else
        hipLaunchKernelGGL(k_bits_stride, dim3(grid_for(count, kGridCap)), dim3(kThreads), 0, 0, src, (long long)start, (long long)step, (long long)count, out);
    return finish("ssfm_bits_slice");
}

extern "C" int ssfm_bits_tile(const unsigned char* src, int64_t n, int64_t reps, unsigned char* out) {
    if (n < 0 || reps < 0 || (n > 0 && reps > INT64_MAX / n)) return fail(SSFM_ERR_INVALID, "ssfm_bits_tile: n=%lld reps=%lld", (long long)n, (long long)reps);
    if (n == 0 || reps == 0) return SSFM_OK;
    if (!src || !out) return fail(SSFM_ERR_INVALID, "ssfm_bits_tile: NULL argument");
    int device = 0;
    if (int rc = device_of(src, &device)) return rc;
    if (!same_device(out, device)) return fail(SSFM_ERR_INVALID, "ssfm_bits_tile: the sequence and the result lie on different devices");
    const long long total = (long long)n * reps;
    hipLaunchKernelGGL(k_bits_tile, grid_bytes(total), dim3(kThreads), 0, 0, src, (long long)n, total, out);
    return finish("ssfm_bits_tile");
}

extern "C" int ssfm_bits_concat(const unsigned char* a, int64_t len_a, const unsigned char* b, int64_t len_b, unsigned char* out) {
    if (len_a < 0 || len_b < 0 || len_a > INT64_MAX - len_b) return fail(SSFM_ERR_INVALID, "ssfm_bits_concat: len_a=%lld len_b=%lld", (long long)len_a, (long long)len_b);
    if (len_a + len_b == 0) return SSFM_OK;
    if ((len_a && !a) || (len_b && !b) || !out) return fail(SSFM_ERR_INVALID, "ssfm_bits_concat: NULL argument");
    int device = 0;
    if (int rc = device_of(out, &device)) return rc;
    if ((len_a && !same_device(a, device)) || (len_b && !same_device(b, device)))
        return fail(SSFM_ERR_INVALID, "ssfm_bits_concat: the sequences and the result lie on different devices");
    if (len_a) launch_map<kCopy>(Src{a, (long long)len_a}, Src{nullptr, 0}, len_a, out);
    if (len_b) launch_map<kCopy>(Src{b, (long long)len_b}, Src{nullptr, 0}, len_b, out + len_a);
    return finish("ssfm_bits_concat");
}

extern "C" int ssfm_bits_count(const unsigned char* a, int64_t n, int64_t* ones) {
    if (!ones || n < 0) return fail(SSFM_ERR_INVALID, "ssfm_bits_count: bad argument");
    *ones = 0;
    if (n == 0) return SSFM_OK;
    if (!a) return fail(SSFM_ERR_INVALID, "ssfm_bits_count: NULL argument");
    int device = 0;
    if (int rc = device_of(a, &device)) return rc;
    ssfm::Scratch s(device);
    void* acc;
    if (int rc = s.get(sizeof(unsigned long long), &acc)) return rc;
    HIP_TRY(hipMemsetAsync(acc, 0, sizeof(unsigned long long), 0));
    hipLaunchKernelGGL(k_bits_count, grid_bytes(n), dim3(kThreads), 0, 0, a, (long long)n, (unsigned long long*)acc);
    HIP_TRY(hipGetLastError());
    unsigned long long h = 0;
    HIP_TRY(hipMemcpy(&h, acc, sizeof(h), hipMemcpyDeviceToHost));
    s.drained = true;
    *ones = (int64_t)h;
    return SSFM_OK;
}
