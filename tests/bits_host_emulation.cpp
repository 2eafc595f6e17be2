// Host emulation of the streaming kernels of opticomlib_amd/csrc/bits.hip (k_bits_map, k_bits_tile, k_bits_stride): the kernels' own text,
// cut out between its two marks into bits_kernels.inc by tests/test_bits_kernels_host.py, compiled for the host with the few HIP names
// below, and every lane of every workgroup run in turn on buffers of exactly the operands' sizes -- under AddressSanitizer a byte read or
// written outside them ends the program.  Sizes around one vector and one workgroup at every source and destination offset modulo 16, and
// results above the grid cap (2048 workgroups x 256 lanes x 16 bytes), where a lane takes a second turn of its grid-stride loop and a
// tile's lanes advance their position in the period.  k_bits_count is not emulated (wavefront shuffles).  Test infrastructure.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
struct uint4 { unsigned x, y, z, w; };
static inline uint4 make_uint4(unsigned x, unsigned y, unsigned z, unsigned w) { return {x, y, z, w}; }
struct dim3 { unsigned x = 1, y = 1, z = 1; };
static dim3 blockIdx, threadIdx, gridDim;
#define __global__
#define __device__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __restrict__
enum { SSFM_BITS_AND = 0, SSFM_BITS_OR = 1, SSFM_BITS_XOR = 2 };
namespace {
#include "bits_kernels.inc"
}
static unsigned grid_for(long long n, long long cap) { long long b = (n + 255) / 256; return (unsigned)(b < cap ? (b > 0 ? b : 1) : cap); }
template <typename F> static void run(long long nbytes, F f) {
    gridDim.x = grid_for((nbytes + 15) / 16, 2048);
    for (blockIdx.x = 0; blockIdx.x < gridDim.x; ++blockIdx.x)
        for (threadIdx.x = 0; threadIdx.x < 256; ++threadIdx.x) f();
}
int main() {
    long long checked = 0;
    const long long sizes[] = {1, 2, 15, 16, 17, 31, 33, 65, 257, 4097, (1LL << 23) + 4097 + 3};
    for (long long n : sizes)
        for (int oa = 0; oa < 16; oa += (n > 5000 ? 16 : 1))
            for (int oo = 0; oo < 16; oo += (n > 5000 ? 16 : (n > 300 ? 5 : 1))) {
                // the payloads are carved from vectors of exactly n + offset bytes so that ASan sees any access past the end
                std::vector<unsigned char> A(n + oa), B(n + 3), O(n + oo), one(1, 7);
                for (long long i = 0; i < n; ++i) { A[oa + i] = (unsigned char)((i * 7 + oa) % 5 == 0 ? 0 : (i % 3 ? 1 : 200)); B[3 + i] = (unsigned char)((i * 11) % 4 == 0); }
                unsigned char *a = A.data() + oa, *b = B.data() + 3, *o = O.data() + oo;
                auto check = [&](auto want, const char* what) {
                    for (long long i = 0; i < n; ++i) if (o[i] != want(i)) { printf("FAIL %s n=%lld oa=%d oo=%d i=%lld got %d\n", what, n, oa, oo, i, o[i]); exit(1); }
                    ++checked;
                };
                run(n, [&] { k_bits_map<SSFM_BITS_XOR>(Src{a, n}, Src{b, n}, n, o); });
                check([&](long long i) { return (a[i] != 0) ^ (b[i] != 0); }, "xor");
                run(n, [&] { k_bits_map<SSFM_BITS_AND>(Src{a, n}, Src{one.data(), 1}, n, o); });
                check([&](long long i) { return (a[i] != 0) & 1; }, "and1");
                run(n, [&] { k_bits_map<kNot>(Src{a, n}, Src{nullptr, 0}, n, o); });
                check([&](long long i) { return a[i] == 0; }, "not");
                run(n, [&] { k_bits_map<kCopy>(Src{a, n}, Src{nullptr, 0}, n, o); });
                check([&](long long i) { return a[i] != 0; }, "copy");
            }
    const long long periods[] = {1, 3, 7, 15, 16, 17, 64, 127, 4097};
    for (long long p : periods)
        for (long long reps : {1LL, 2LL, 3LL, 1000LL, 2100LL})
            for (int oo = 0; oo < 16; oo += 3) {
                const long long total = p * reps;
                if (total > 5000 && oo != 3) continue;
                std::vector<unsigned char> A(p + 5), O(total + oo);
                for (long long i = 0; i < p; ++i) A[5 + i] = (unsigned char)((i * 13 + 1) % 3 == 0 ? 0 : 9);
                unsigned char *a = A.data() + 5, *o = O.data() + oo;
                run(total, [&] { k_bits_tile(a, p, total, o); });
                for (long long i = 0; i < total; ++i) if (o[i] != (a[i % p] != 0)) { printf("FAIL tile p=%lld reps=%lld oo=%d i=%lld\n", p, reps, oo, i); return 1; }
                ++checked;
            }
    {
        const long long n = 4099;
        std::vector<unsigned char> A(n);
        for (long long i = 0; i < n; ++i) A[i] = (unsigned char)(i % 3);
        struct K { long long start, step, count; } keys[] = {{n - 1, -1, n}, {0, 3, (n + 2) / 3}, {n - 5, -2, (n - 5 - 2 + 1) / 2}, {4098, -4098, 2}, {0, 4098, 2}};
        for (auto k : keys) {
            std::vector<unsigned char> O(k.count);
            gridDim.x = grid_for(k.count, 2048);
            for (blockIdx.x = 0; blockIdx.x < gridDim.x; ++blockIdx.x)
                for (threadIdx.x = 0; threadIdx.x < 256; ++threadIdx.x) k_bits_stride(A.data(), k.start, k.step, k.count, O.data());
            for (long long i = 0; i < k.count; ++i) if (O[i] != (A[k.start + i * k.step] != 0)) { printf("FAIL stride\n"); return 1; }
            ++checked;
        }
    }
    printf("ok: %lld cases\n", checked);
    return 0;
}
