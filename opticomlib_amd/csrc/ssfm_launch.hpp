// ssfm_launch.hpp -- what the launchers of the transform kernels share (ssfm_host.hip, ssfm_medium.hip): the dynamic LDS of a column pass
// and of a row pass, and the launch itself.  Host code only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "ssfm_kernels.hpp"

namespace ssfm {
// A column pass (time_body) of N1 points x C columns, E points per thread: the tile (when the transform exchanges through it at all), the E x C
// staging rows, the twiddles.
template <typename T> constexpr size_t col_pass_lds(int N1, int C, int E) {
    return ((fft_nstages(N1, E) > 1 ? (size_t)N1 * C : 0) + (size_t)E * C + (size_t)fft_tw_lds_entries(N1, E)) * sizeof(cx<T>);
}
// A row pass (freq_body, the one-workgroup engines) of ROWS padded rows of N points, E per thread: the rows (as above), the twiddles, and `extra`
// elements behind them (the small chirp kernels keep H there).
template <typename T> constexpr size_t row_pass_lds(int N, int E, int ROWS, size_t extra = 0) {
    return ((fft_nstages(N, E) > 1 ? (size_t)ROWS * row_lds_elems(N, E) : 0) + (size_t)fft_tw_lds_entries(N, E) + extra) * sizeof(cx<T>);
}

// Launch Kernel with LDS bytes of dynamic LDS.  Above the 48 KiB a kernel may use unasked, the limit is raised first: once per Kernel (the static
// belongs to this instantiation), and a launch after that pays one load and one compare for it.  Kernel and LDS are template arguments for that reason.
template <auto Kernel, size_t LDS, typename... Args>
hipError_t launch_kernel(dim3 grid, dim3 block, hipStream_t s, const Args&... args) {
    if constexpr (LDS > 48 * 1024) {
        static const hipError_t raised = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS);
        if (raised != hipSuccess) return raised;
    }
    hipLaunchKernelGGL(Kernel, grid, block, LDS, s, args...);
    return hipGetLastError();
}
}  // namespace ssfm
