// ssfm_medium.hip -- the single-launch fixed-step engine of plans of 2^14 ... 2^17 samples (ssfm_kernels.hpp k_medium), in a
// translation unit of its own (its four shapes x two operator-table kinds are a minute of compile time).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>

#include "ssfm_kernels.hpp"
#include "ssfm_launch.hpp"
#include "ssfm_medium.hpp"

namespace ssfm {
namespace {
// The four kernels: what each takes and its instantiation for a shape
template <int FMODE> struct Fixed {
    using Args = MediumArgs<float>;
    template <int N1, int N2> static constexpr auto kernel = &k_medium<float, N1, N2, 8, FMODE>;
};
struct Adapt {
    using Args = MediumAdaptArgs<float>;
    template <int N1, int N2> static constexpr auto kernel = &k_medium_adapt<float, N1, N2, 8>;
};
struct Chirp {
    using Args = MediumChirpArgs<float>;
    template <int N1, int N2> static constexpr auto kernel = &k_medium_chirp<float, N1, N2, 8>;
};
struct ChirpAdapt {
    using Args = MediumChirpAdaptArgs<float>;
    template <int N1, int N2> static constexpr auto kernel = &k_medium_chirp_adapt<float, N1, N2, 8>;
};

// N1 column points x N2 row points, 8 points per thread, 16 columns per tile: a workgroup does column passes and row passes in the same LDS
constexpr int kShapes[6][2] = {{64, 64}, {64, 128}, {128, 128}, {128, 256}, {256, 256}, {256, 512}};

template <typename K, size_t I = 0>
hipError_t launch_shape(int N1, int N2, int nblk, int xccs, hipStream_t s, const typename K::Args& a) {
    if constexpr (I == sizeof(kShapes) / sizeof(kShapes[0])) return hipErrorInvalidValue;
    else {
        constexpr int S1 = kShapes[I][0], S2 = kShapes[I][1], E = 8, C = 16, ROWS = S1 * C / S2;
        constexpr size_t lds = std::max(col_pass_lds<float>(S1, C, E), row_pass_lds<float>(S2, E, ROWS));
        if (N1 == S1 && N2 == S2) return launch_kernel<K::template kernel<S1, S2>, lds>(dim3(xccs * nblk), dim3(S1 * C / E), s, a);
        return launch_shape<K, I + 1>(N1, N2, nblk, xccs, s, a);
    }
}
}  // namespace

bool medium_shape(int N1, int N2) {
    for (const auto& sh : kShapes)
        if (N1 == sh[0] && N2 == sh[1]) return true;
    return false;
}
// (the kernels stand in the code object in the order in which these name them)
hipError_t launch_medium_adapt(int N1, int N2, int nblk, int xccs, hipStream_t s, const MediumAdaptArgs<float>& a) { return launch_shape<Adapt>(N1, N2, nblk, xccs, s, a); }
hipError_t launch_medium_chirp(int N1, int N2, int nblk, int xccs, hipStream_t s, const MediumChirpArgs<float>& a) { return launch_shape<Chirp>(N1, N2, nblk, xccs, s, a); }
hipError_t launch_medium_chirp_adapt(int N1, int N2, int nblk, int xccs, hipStream_t s, const MediumChirpAdaptArgs<float>& a) { return launch_shape<ChirpAdapt>(N1, N2, nblk, xccs, s, a); }
hipError_t launch_medium(int N1, int N2, bool phase_tables, int nblk, int xccs, hipStream_t s, const MediumArgs<float>& a) {
    return phase_tables ? launch_shape<Fixed<FM_PHASE>>(N1, N2, nblk, xccs, s, a) : launch_shape<Fixed<FM_TABLE>>(N1, N2, nblk, xccs, s, a);
}

namespace {
__global__ void k_xcc_probe(unsigned* mask) {
    if (threadIdx.x == 0) atomicOr(mask, 1u << xcc_id());
}
}  // namespace
unsigned xcc_mask(int device) {
    static std::mutex mu;
    static unsigned cache[64] = {0};
    if (device < 0 || device >= 64) return 0u;
    std::lock_guard<std::mutex> lock(mu);
    if (cache[device]) return cache[device];
    int cur = 0;
    unsigned* d = nullptr;
    unsigned h = 0u;
    hipStream_t s = nullptr;            // (a stream of its own: nothing of this library runs on the legacy stream)
    if (hipGetDevice(&cur) != hipSuccess || cur != device || hipMalloc(&d, sizeof(unsigned)) != hipSuccess) return 0u;
    if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) == hipSuccess) {
        if (hipMemsetAsync(d, 0, sizeof(unsigned), s) == hipSuccess) {
            hipLaunchKernelGGL(k_xcc_probe, dim3(256), dim3(64), 0, s, d);
            if (hipMemcpyAsync(&h, d, sizeof(unsigned), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) h = 0u;
        }
        (void)hipStreamDestroy(s);
    }
    (void)hipFree(d);
    if (h == 0u) return 0u;             // (not cached: a later plan may try again)
    return cache[device] = h;
}
}  // namespace ssfm
