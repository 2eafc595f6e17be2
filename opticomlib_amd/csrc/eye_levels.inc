// eye_levels.inc -- the state block, the block reductions and the moments / KDE kernels of the eye's centre, shared by the blind estimator
// (eye.hip: GET_EYE takes a sample's level from its value, above or below y_center) and the data-aided one (sync.hip: GET_EYE_v2 takes it
// from the slot that was sent).  Included INSIDE the anonymous namespace of each translation unit, after <hip/hip_runtime.h> and <cmath>.

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kRedBlocks = 480;                    // workgroups of a reduction pass (a few per CU of the 256-CU part)
constexpr int kPartStride = 8;                     // doubles per workgroup partial
constexpr int kKdeThreads = 512;                   // one thread per grid point of the KDE (<= 512 points)
constexpr int kKdeTile = 256;                      // central samples held in LDS by one KDE workgroup (~400 workgroups at 10^5 samples)

// The state block: one double per quantity (integers stored exactly).  The host reads it back whole.
enum Slot {
    S_C0, S_C1,                                    // 1-D centres
    S_T0, S_Y0, S_T1, S_Y1,                        // 2-D centres (cluster 0 / 1)
    S_IT1, S_DONE1, S_IT2, S_DONE2,
    S_VM, S_NBOT, S_NTOP, S_TOPSTART,
    S_BOT0, S_BOT1, S_TOP0, S_TOP1,
    S_V25, S_V75, S_STATE0, S_STATE1, S_YCT,      // S_YCT: (state0 + state1) / 2 before the snap
    S_YC, S_YL, S_YR,                              // nearest values in the pre-resample set
    S_NBAND, S_TMEAN, S_MIND,
    S_MU0, S_MU1, S_SD0, S_SD1, S_N0, S_N1, S_NC, S_CMEAN, S_CVAR, S_INVH, S_KDE, S_SINGULAR,
    S_NONFINITE,                                   // the signal holds a NaN or an infinity (sklearn's KMeans.fit rejects it)
    S_COUNT
};
static_assert(S_COUNT <= 64, "state block");

// ------------------------------------------------------------------------------------------------ block reductions
template <int K>
__device__ void block_sum(double (&v)[K], double (*lds)[kThreads]) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int k = 0; k < K; ++k) lds[k][tid] = v[k];
    __syncthreads();
    for (int off = kThreads / 2; off > 0; off >>= 1) {
        if (tid < off) {
#pragma unroll
            for (int k = 0; k < K; ++k) lds[k][tid] += lds[k][tid + off];
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = lds[k][0];
    __syncthreads();
}

// fold the kRedBlocks partials of K doubles in a fixed order (one workgroup)
template <int K>
__device__ void fold_partials(const double* __restrict__ part, double (&v)[K], double (*lds)[kThreads]) {
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = 0.0;
    for (int b = threadIdx.x; b < kRedBlocks; b += kThreads)
#pragma unroll
        for (int k = 0; k < K; ++k) v[k] += part[b * kPartStride + k];
    block_sum<K>(v, lds);
}

__global__ void k_levels_init(double* __restrict__ st, double y_center) {
    for (int k = 0; k < S_COUNT; ++k) st[k] = 0.0;
    st[S_YC] = y_center;
}

// ------------------------------------------------------------------------------------------------ moments and KDE of the eye's centre
// The central samples are those whose t (index mod period) falls in [k_lo, k_hi): sample j of them is  (j / w) * period + k_lo + j % w.
struct Centre {
    long long count;
    int period, k_lo, w;
    __device__ long long index(long long j) const { return (j / w) * period + k_lo + j % w; }
};

// The level of central sample j of value x: 1 the upper one, 0 the lower one, -1 neither.
struct LevelByValue {                              // GET_EYE: above / below y_center
    __device__ int operator()(double x, long long, int, double yc) const { return x > yc ? 1 : (x < yc ? 0 : -1); }
};
struct LevelBySlot {                               // GET_EYE_v2: the slot that was sent (period = samples per slot, so j / w is the slot)
    const unsigned char* bits;
    __device__ int operator()(double, long long j, int w, double) const { return bits[j / w] ? 1 : 0; }
};

template <int PASS, class Level>
__global__ __launch_bounds__(kThreads) void k_moments(const double* __restrict__ y, Centre c, Level level, const double* __restrict__ st, double* __restrict__ part) {
#pragma clang fp contract(off)
    __shared__ double lds[6][kThreads];
    const double yc = st[S_YC], m1 = st[S_MU1], m0 = st[S_MU0], mc = st[S_CMEAN];
    double v[6] = {0, 0, 0, 0, 0, 0};
    for (long long j = (long long)blockIdx.x * kThreads + threadIdx.x; j < c.count; j += (long long)kRedBlocks * kThreads) {
        const double x = y[c.index(j)];
        const int lv = level(x, j, c.w, yc);
        if (PASS == 1) {
            if (lv == 1) { v[0] += 1.0; v[1] += x; }
            if (lv == 0) { v[2] += 1.0; v[3] += x; }
            v[4] += 1.0;
            v[5] += x;
        } else {
            if (lv == 1) { const double d = x - m1; v[0] += d * d; }
            if (lv == 0) { const double d = x - m0; v[1] += d * d; }
            const double d = x - mc;
            v[2] += d * d;
        }
    }
    block_sum<6>(v, lds);
    if (threadIdx.x < 6) part[blockIdx.x * kPartStride + threadIdx.x] = v[threadIdx.x];
}

template <int PASS>
__global__ __launch_bounds__(kThreads) void k_moments_fold(const double* __restrict__ part, double* __restrict__ st) {
    __shared__ double lds[6][kThreads];
    double v[6];
    fold_partials<6>(part, v, lds);
    if (threadIdx.x) return;
    if (PASS == 1) {                                               // np.mean(..., where=...): 0 / 0 = nan for an empty cluster
        st[S_N1] = v[0]; st[S_MU1] = v[1] / v[0];
        st[S_N0] = v[2]; st[S_MU0] = v[3] / v[2];
        st[S_NC] = v[4]; st[S_CMEAN] = v[5] / v[4];
    } else {                                                       // np.std (ddof 0); the KDE's variance with ddof 1, Scott's factor n^(-1/5)
        st[S_SD1] = sqrt(v[0] / st[S_N1]);
        st[S_SD0] = sqrt(v[1] / st[S_N0]);
        const double nc = st[S_NC], var = v[2] / (nc - 1.0);
        st[S_CVAR] = var;
        // (a NaN end of the grid, an empty top or bottom cluster, is no threshold either: scipy's evaluate raises on it)
        const bool ok = nc >= 2.0 && var > 0.0 && isfinite(var) && isfinite(st[S_MU0]) && isfinite(st[S_MU1]);
        st[S_SINGULAR] = ok ? 0.0 : 1.0;
        st[S_INVH] = ok ? 1.0 / (sqrt(var) * pow(nc, -0.2)) : 0.0;
    }
}

// x_k = k * step + mu0 with x_last = mu1 (numpy.linspace)
__device__ __forceinline__ double grid_point(const double* st, int k, int npts) {
#pragma clang fp contract(off)
    const double a = st[S_MU0], b = st[S_MU1];
    if (k == npts - 1) return b;
    const double step = (b - a) / (double)(npts - 1);
    return (double)k * step + a;
}

// each workgroup holds kKdeTile central samples (whitened) in LDS and adds their kernels at every grid point: partial[block][k]
__global__ __launch_bounds__(kKdeThreads) void k_kde(const double* __restrict__ y, Centre c, const double* __restrict__ st, int npts, double* __restrict__ part) {
#pragma clang fp contract(off)
    __shared__ double s[kKdeTile];
    if (st[S_SINGULAR] != 0.0) return;
    const double ih = st[S_INVH];
    const long long j0 = (long long)blockIdx.x * kKdeTile;
    const int cnt = (int)(c.count - j0 < kKdeTile ? c.count - j0 : kKdeTile);
    for (int q = threadIdx.x; q < cnt; q += kKdeThreads) s[q] = y[c.index(j0 + q)] * ih;
    __syncthreads();
    const int k = threadIdx.x;
    if (k >= npts) return;
    const double xw = grid_point(st, k, npts) * ih;
    double acc = 0.0;
    for (int q = 0; q < cnt; ++q) {
        const double d = s[q] - xw;
        acc += exp(-(d * d) / 2.0);
    }
    part[(long long)blockIdx.x * kKdeThreads + k] = acc;
}

// fold the partials per grid point in block order, then the argmin (first index on ties)
__global__ __launch_bounds__(kKdeThreads) void k_kde_argmin(const double* __restrict__ part, int nblocks, int npts, double* __restrict__ st) {
    __shared__ double lv[kKdeThreads];
    __shared__ int li[kKdeThreads];
    if (st[S_SINGULAR] != 0.0) { if (threadIdx.x == 0) st[S_KDE] = -1.0; return; }
    const int k = threadIdx.x;
    double acc = 0.0;
    if (k < npts)
        for (int b = 0; b < nblocks; ++b) acc += part[(long long)b * kKdeThreads + k];
    lv[k] = k < npts ? acc : INFINITY;
    li[k] = k;
    __syncthreads();
    for (int off = kKdeThreads / 2; off > 0; off >>= 1) {
        if (k < off) {
            const double v = lv[k + off];
            const int i = li[k + off];
            if (v < lv[k] || (v == lv[k] && i < li[k])) { lv[k] = v; li[k] = i; }
        }
        __syncthreads();
    }
    if (k == 0) st[S_KDE] = (double)li[0];
}

inline int kde_blocks(const Centre& c) { return (int)((c.count + kKdeTile - 1) / kKdeTile); }

// The seven launches behind ssfm_eye_levels / ssfm_eye_levels_known on the default stream: S the state block (64 doubles), P the kRedBlocks x kPartStride
// partials, K the kde_blocks(c) x kKdeThreads partials of the KDE (all DEVICE).  The caller reads S back.
template <class Level>
void launch_levels(const double* y, const Centre& c, Level level, double y_center, int npts, double* S, double* P, double* K) {
    const dim3 R(kRedBlocks), B(kThreads);
    const int kblocks = kde_blocks(c);
    hipLaunchKernelGGL(k_levels_init, dim3(1), dim3(1), 0, 0, S, y_center);
    hipLaunchKernelGGL((k_moments<1, Level>), R, B, 0, 0, y, c, level, (const double*)S, P);
    hipLaunchKernelGGL(k_moments_fold<1>, dim3(1), B, 0, 0, (const double*)P, S);
    hipLaunchKernelGGL((k_moments<2, Level>), R, B, 0, 0, y, c, level, (const double*)S, P);
    hipLaunchKernelGGL(k_moments_fold<2>, dim3(1), B, 0, 0, (const double*)P, S);
    if (kblocks > 0) hipLaunchKernelGGL(k_kde, dim3(kblocks), dim3(kKdeThreads), 0, 0, y, c, (const double*)S, npts, K);
    hipLaunchKernelGGL(k_kde_argmin, dim3(1), dim3(kKdeThreads), 0, 0, (const double*)K, kblocks, npts, S);
}
