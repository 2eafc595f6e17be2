// sos_filter_impl.inc -- everything of sos_filter.hip that depends on the chunk length: included TWICE, in two namespaces that define
// `kChunk` (samples per thread) -- the short chunk for the three-launch form and for short calls, the long one for the one-launch form
// of long calls (see sos_filter.hip).  No include guard on purpose.
// waves per SIMD asked of the register allocator for the output kernels: three workgroups per CU with the short chunk (52 KiB of LDS
// each), two with the long one (78 KiB)
constexpr int kApplyWaves = kChunk > 12 ? 2 : 3;
template <int CH> struct Smp { double v[CH]; };

template <int CH> __device__ __forceinline__ Smp<CH> ld(const double* p, long long e) {
    Smp<CH> r;
    if constexpr (CH == 2) {
        const double2 q = *reinterpret_cast<const double2*>(p + 2 * e);
        r.v[0] = q.x; r.v[1] = q.y;
    } else {
        r.v[0] = p[e];
    }
    return r;
}
template <int CH> __device__ __forceinline__ void st(double* p, long long e, const Smp<CH>& s) {
    if constexpr (CH == 2) {
        typedef double d2v __attribute__((ext_vector_type(2)));
        d2v q = {s.v[0], s.v[1]};
        asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" : : "v"(reinterpret_cast<d2v*>(p + 2 * e)), "v"(q) : "memory");
    } else p[e] = s.v[0];
}

// sample i of the pass input of the row starting at `base`
// Branch-free on purpose: the lanes of a wavefront at a row's edge take different paths here, and loads behind divergent
// branches cannot be issued together -- the 12 samples of a chunk became 12 to 36 dependent trips to memory, and the two or four
// edge wavefronts of a launch ran twice as long as all the others: they WERE the kernel's duration (19 us with a bulk that is done
// after 10, profiles/r03_sosfilt.txt).  Both candidate samples are loaded unconditionally (indices clamped into the row), the
// odd extension 2 x[end] - x[mirror] (scipy's odd_ext) is formed and one select picks.
template <int CH> __device__ __forceinline__ Smp<CH> sos_input(const SosPass& p, const double* base, long long i) {
    if (p.backward) {                                                            // reversed forward output (wave-uniform branch)
        long long k = p.mv - 1 - i;
        k = k < 0 ? 0 : (k > p.m - 1 ? p.m - 1 : k);                             // (beyond the end: the virtual copies of y1[m - 1])
        return ld<CH>(base, k);
    }
    const long long j = i - p.edge;                                              // position in the row; outside [0, n): odd extension
    const bool left = j < 0, right = j >= p.n;
    long long ia = left ? 0 : (right ? p.n - 1 : j);                             // the row's end sample, or the sample itself
    long long ib = left ? -j : (right ? 2 * (p.n - 1) - j : j);                  // its mirror image
    ib = ib < 0 ? 0 : (ib > p.n - 1 ? p.n - 1 : ib);                             // (only lanes beyond the padded length get here clamped)
    const Smp<CH> a = ld<CH>(base, ia), b = ld<CH>(base, ib);
    Smp<CH> r;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
        const double ext = 2.0 * a.v[c] - b.v[c];
        r.v[c] = (left || right) ? ext : a.v[c];
    }
    return r;
}
template <int CH> __device__ __forceinline__ const double* pass_row(const SosPass& p, int row) {
    return p.src + (long long)row * (p.backward ? p.m : p.n) * CH;
}

template <int NS>
__device__ __forceinline__ double sos_step(const SosCoefs& c, double (&z)[NS][2], double x) {
#pragma clang fp contract(off)       // SciPy's C loop rounds every product: keep the same roundings
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const double xn = x;
        x = c.b0[s] * xn + z[s][0];
        z[s][0] = c.b1[s] * xn - c.a1[s] * x + z[s][1];
        z[s][1] = c.b2[s] * xn - c.a2[s] * x;
    }
    return x;
}

// The same step with fused multiply-adds (5 operations per section instead of 9; each product is no longer rounded on its own, so the
// result differs from SciPy's loop in the last bits -- as the chunk start states do anyway).  The one-launch kernel, whose workgroups
// all compute at the same time, is bound by its float64 instruction count.
template <int NS>
__device__ __forceinline__ double sos_step_fma(const SosCoefs& c, double (&z)[NS][2], double x) {
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const double xn = x;
        x = fma(c.b0[s], xn, z[s][0]);
        z[s][0] = fma(c.b1[s], xn, fma(-c.a1[s], x, z[s][1]));
        z[s][1] = fma(c.b2[s], xn, -c.a2[s] * x);
    }
    return x;
}

// LDS staging of a wavefront's 64 x kChunk samples: element r = chunk * kChunk + t lives at r + r / kChunk
// (one pad element per chunk: a lane's ds_read/ds_write of "its" sample t is bank-conflict free).
constexpr int kWaveSamples = kWave * kChunk;
constexpr int kLdsElems = kWaveSamples + kWave;
__device__ __forceinline__ int lds_pos(int r) { return r + r / kChunk; }

// Is the wavefront's sample range [w0, w0 + 64 * kChunk) of the padded sequence plain memory (no odd extension,
// no ragged end)?  Wave-uniform.
__device__ __forceinline__ bool wave_is_plain(const SosPass& p, long long w0) {
    if (p.backward) return w0 >= p.mv - p.m;                  // (past the virtual copies; the grid ends with the sequence)
    return w0 >= p.edge && w0 + kWaveSamples <= p.edge + p.n;
}

// A wavefront exchanges data through ITS slice of LDS only: DS instructions of one wavefront execute in
// order, so no workgroup barrier is needed -- just keep the compiler from reordering across this point.
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the kChunk input samples of the lane's chunk (all loads issued before the recurrence starts)
template <int CH> __device__ __forceinline__ void load_chunk(const SosPass& p, const double* base, long long w0, int lane, int len, bool plain,
                                                              Smp<CH>* lds, Smp<CH> (&xs)[kChunk]) {
    if (plain) {
        // coalesced: instruction t moves samples w0 + 64 t + lane
        Smp<CH> tmp[kChunk];
#pragma unroll
        for (int t = 0; t < kChunk; ++t) {
            const long long i = w0 + t * kWave + lane;
            tmp[t] = ld<CH>(base, p.backward ? p.mv - 1 - i : i - p.edge);
        }
#pragma unroll
        for (int t = 0; t < kChunk; ++t) lds[lds_pos(t * kWave + lane)] = tmp[t];
        wave_lds_sync();
#pragma unroll
        for (int t = 0; t < kChunk; ++t) xs[t] = lds[lane * (kChunk + 1) + t];
        wave_lds_sync();
    } else {
        const long long i0 = w0 + (long long)lane * kChunk;
#pragma unroll
        for (int t = 0; t < kChunk; ++t) xs[t] = sos_input<CH>(p, base, i0 + t);     // (samples beyond `len` are loaded from clamped positions and never used)
        (void)len;
    }
}

// The two halves of load_chunk's plain path, for a caller with work in between that should not have to keep 12 samples per channel in
// registers meanwhile (k_apply's group reduction): coalesced loads -> the wavefront's LDS slice, and later slice -> this lane's chunk.
template <int CH> __device__ __forceinline__ void chunk_to_lds(const SosPass& p, const double* base, long long w0, int lane, Smp<CH>* lds) {
    Smp<CH> tmp[kChunk];
#pragma unroll
    for (int t = 0; t < kChunk; ++t) {
        const long long i = w0 + t * kWave + lane;
        tmp[t] = ld<CH>(base, p.backward ? p.mv - 1 - i : i - p.edge);
    }
#pragma unroll
    for (int t = 0; t < kChunk; ++t) lds[lds_pos(t * kWave + lane)] = tmp[t];
    wave_lds_sync();
}
// The same for a wavefront at a row's edge or end: sample by sample through sos_input (two coalesced loads and a select each) instead of
// lane by lane -- in the one-launch kernel every workgroup waits for the totals of the row's first group.
template <int CH> __device__ __forceinline__ void chunk_to_lds_edge(const SosPass& p, const double* base, long long w0, int lane, Smp<CH>* lds) {
    Smp<CH> tmp[kChunk];
#pragma unroll
    for (int t = 0; t < kChunk; ++t) {
        const long long b = w0 + t * kWave;                          // (wave-uniform: most of the 12 instructions of an edge wavefront are plain)
        if (b >= p.edge && b + kWave <= p.edge + p.n) tmp[t] = ld<CH>(base, b + lane - p.edge);
        else if (b >= p.mv) {                                        // (beyond the sequence: never used)
#pragma unroll
            for (int c = 0; c < CH; ++c) tmp[t].v[c] = 0.0;
        } else {
            long long i = b + lane;
            i = i < p.mv ? i : p.mv - 1;                          // (beyond the sequence: never used)
            tmp[t] = sos_input<CH>(p, base, i);
        }
    }
#pragma unroll
    for (int t = 0; t < kChunk; ++t) lds[lds_pos(t * kWave + lane)] = tmp[t];
    wave_lds_sync();
}
template <int CH> __device__ __forceinline__ void chunk_from_lds(Smp<CH>* lds, int lane, Smp<CH> (&xs)[kChunk]) {
#pragma unroll
    for (int t = 0; t < kChunk; ++t) xs[t] = lds[lane * (kChunk + 1) + t];
    wave_lds_sync();
}

// y += M x  (M row-major K x K, wave-uniform address).  Every map of this file is a power of the cascade's one-chunk map, and in a
// cascade a section never sees the ones after it: the maps are block lower triangular (2 x 2 blocks, exact zeros above -- the host
// builds them by running the recurrence on unit states), so those products are skipped: 12 of 16 for two sections, 40 of 64 for four.
template <int K, int CH> __device__ __forceinline__ void mat_acc(const double* M, const double (&x)[CH][K], double (&y)[CH][K]) {
#pragma unroll
    for (int r = 0; r < K; ++r)
#pragma unroll
        for (int q = 0; q < K; ++q) {
            if (q / 2 > r / 2) continue;
            const double mrq = M[r * K + q];
#pragma unroll
            for (int c = 0; c < CH; ++c) y[c][r] += mrq * x[c][q];
        }
}

// The scan's doubling steps use M^1, M^2, M^4 ... M^32, the combination of the wavefronts M^64.  Fetching them step by step from
// global memory puts dependent cache misses on the critical path of kernels that only live for microseconds, so a workgroup keeps
// a copy of the seven matrices in LDS (k_chunk_scan: fetched up front by its last wavefront, written after that one's transposes).
constexpr int kScanSteps = 6;
// Inclusive scan over the 64 lanes of a wavefront of the affine maps s -> M s + x_lane (same M in every
// lane): afterwards x_lane = sum_{i <= lane} M^(lane - i) x_i.  lds_pw = the workgroup's LDS copy of the powers.
template <int K, int CH> __device__ __forceinline__ void wave_scan(double (&x)[CH][K], const double* lds_pw) {
    const int lane = threadIdx.x & (kWave - 1);
#pragma unroll
    for (int k = 0; k < kScanSteps; ++k) {
        const int d = 1 << k;
        double up[CH][K];
#pragma unroll
        for (int c = 0; c < CH; ++c)
#pragma unroll
            for (int q = 0; q < K; ++q) {
                const double o = __shfl_up(x[c][q], d, kWave);
                up[c][q] = lane >= d ? o : 0.0;
            }
        mat_acc<K, CH>(lds_pw + k * K * K, up, x);
    }
}
// The same scan in the OPPOSITE lane order (lane 63 first): afterwards x_lane = sum_{i >= lane} M^(i - lane) x_i -- the backward pass's
// chunk order inside the forward pass's wavefront (see SosPass::mv).
template <int K, int CH> __device__ __forceinline__ void wave_scan_rev(double (&x)[CH][K], const double* lds_pw) {
    const int lane = threadIdx.x & (kWave - 1);
#pragma unroll
    for (int k = 0; k < kScanSteps; ++k) {
        const int d = 1 << k;
        double up[CH][K];
#pragma unroll
        for (int c = 0; c < CH; ++c)
#pragma unroll
            for (int q = 0; q < K; ++q) {
                const double o = __shfl_down(x[c][q], d, kWave);
                up[c][q] = lane + d < kWave ? o : 0.0;
            }
        mat_acc<K, CH>(lds_pw + k * K * K, up, x);
    }
}
// x <- M x
template <int K, int CH> __device__ __forceinline__ void mat_apply(const double* M, double (&x)[CH][K]) {
    double y[CH][K];
#pragma unroll
    for (int c = 0; c < CH; ++c)
#pragma unroll
        for (int k = 0; k < K; ++k) y[c][k] = 0.0;
    mat_acc<K, CH>(M, x, y);
#pragma unroll
    for (int c = 0; c < CH; ++c)
#pragma unroll
        for (int k = 0; k < K; ++k) x[c][k] = y[c][k];
}

// state vector s[CH][K] <-> z[NS][2] per channel
template <int NS, int CH, int W>
__global__ __launch_bounds__(kWave * W) void k_chunk_scan(SosPass p, int nchunks, int ngroups, const double* __restrict__ pw,
                                                       const double* __restrict__ G, double* __restrict__ E, double* __restrict__ T) {
    constexpr int K = 2 * NS;
    constexpr int kWaves = W, kGroup = kWave * W;
    __shared__ Smp<CH> lds_all[kWaves][kLdsElems];
    // The staging slices are ALL the LDS of the kernel: the wavefront totals go into each wavefront's own slice and the matrix powers
    // of the scan into the last wavefront's (offset 1 KiB), both written once the owner has finished its transposes.  52 KiB per
    // workgroup: three fit a CU whatever the allocation granule is (54 272 B did not: a 2^20 x 2 call's 684 workgroups ran as two
    // generations, and a launch took twice a workgroup's lifetime -- profiles/r03_sosfilt.txt).
    static_assert((kScanSteps + 1) * K * K * sizeof(double) + 1024 <= sizeof(Smp<CH>) * kLdsElems, "the powers fit the slice");
    double* const lds_pw = reinterpret_cast<double*>(lds_all[kWaves - 1]) + 128;
    const int row = blockIdx.x / ngroups, g = blockIdx.x % ngroups;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wv = tid / kWave;
    const int ch = g * kGroup + tid;
    const long long w0 = ((long long)g * kGroup + wv * kWave) * kChunk;
    const bool plain = wave_is_plain(p, w0);
    // (the last wavefront fetches the scan's matrix powers now and writes them to LDS after its transposes)
    constexpr int kPwEntries = (kScanSteps + 1) * K * K, kPwPerLane = (kPwEntries + kWave - 1) / kWave;
    double pw_stage[kPwPerLane];
    if (wv == kWaves - 1) {
#pragma unroll
        for (int i = 0; i < kPwPerLane; ++i) {
            const int e = lane + i * kWave;
            pw_stage[i] = e < kPwEntries ? pw[((long long)1 << (e / (K * K))) * K * K + e % (K * K)] : 0.0;
        }
    }
    // this lane's M^lane, for the offset of its wavefront inside the group (fetched ahead of its use)
    double Ml[K][K];
#pragma unroll
    for (int r = 0; r < K; ++r)
#pragma unroll
        for (int q = 0; q < K; ++q) Ml[r][q] = pw[(long long)lane * K * K + r * K + q];
    double s[CH][K];
#pragma unroll
    for (int a = 0; a < CH; ++a)
#pragma unroll
        for (int k = 0; k < K; ++k) s[a][k] = 0.0;
    if (plain || ch < nchunks) {
        const double* base = pass_row<CH>(p, row);
        const long long i0 = (long long)ch * kChunk;
        const int len = (int)(i0 + kChunk <= p.mv ? kChunk : p.mv - i0);
        Smp<CH> xs[kChunk];
        load_chunk<CH>(p, base, w0, lane, len, plain, lds_all[wv], xs);
        // The chunk's particular solution -- the state after its samples from a ZERO state -- is linear in the samples:
        // p_c = sum_t G[:, t] x_t, G[:, t] = the state kChunk - 1 - t steps after a unit sample (built on the host by
        // running the recurrence on unit samples).  K fma per sample and channel instead of the 9 NS float64 operations
        // of the recurrence itself, which only the output pass (k_apply) has to run.  A short last chunk ends `len`
        // samples in: its sample t has the weight of sample kChunk - len + t of a full one.
        if (len == kChunk) {
#pragma unroll
            for (int t = 0; t < kChunk; ++t)
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const double g = G[k * kChunk + t];
#pragma unroll
                    for (int a = 0; a < CH; ++a) s[a][k] = fma(g, xs[t].v[a], s[a][k]);
                }
        } else {
            const int off = kChunk - len;
#pragma unroll
            for (int t = 0; t < kChunk; ++t)
                if (t < len) {
#pragma unroll
                    for (int k = 0; k < K; ++k) {
                        const double g = G[k * kChunk + off + t];
#pragma unroll
                        for (int a = 0; a < CH; ++a) s[a][k] = fma(g, xs[t].v[a], s[a][k]);
                    }
                }
        }
    }
    if (wv == kWaves - 1) {
#pragma unroll
        for (int i = 0; i < kPwPerLane; ++i) {
            const int e = lane + i * kWave;
            if (e < kPwEntries) lds_pw[e] = pw_stage[i];
        }
    }
    __syncthreads();                      // lds_pw staged
    wave_scan<K, CH>(s, lds_pw);
    // exclusive prefix = the chunk's start state if its WAVEFRONT started from zero
    double ex[CH][K];
#pragma unroll
    for (int a = 0; a < CH; ++a)
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const double prev = __shfl_up(s[a][k], 1, kWave);
            ex[a][k] = lane ? prev : 0.0;
            if (lane == kWave - 1) reinterpret_cast<double*>(lds_all[wv])[a * K + k] = s[a][k];
        }
    __syncthreads();
    // start state of this wavefront if the GROUP started from zero: ws_{w+1} = M^64 ws_w + tot_w
    const double* M64 = lds_pw + kScanSteps * K * K;
    double ws[CH][K];
#pragma unroll
    for (int a = 0; a < CH; ++a)
#pragma unroll
        for (int k = 0; k < K; ++k) ws[a][k] = 0.0;
    for (int w = 0; w < wv; ++w) {
        mat_apply<K, CH>(M64, ws);
#pragma unroll
        for (int a = 0; a < CH; ++a)
#pragma unroll
            for (int k = 0; k < K; ++k) ws[a][k] += reinterpret_cast<const double*>(lds_all[w])[a * K + k];
    }
    // e_c = M^lane ws + (wavefront-local exclusive prefix)
#pragma unroll
    for (int r = 0; r < K; ++r)
#pragma unroll
        for (int q = 0; q < K; ++q) {
#pragma unroll
            for (int a = 0; a < CH; ++a) ex[a][r] += Ml[r][q] * ws[a][q];
        }
    double* Eo = E + ((long long)row * ngroups * kGroup + ch) * (CH * K);
#pragma unroll
    for (int a = 0; a < CH; ++a)
#pragma unroll
        for (int k = 0; k < K; ++k) Eo[a * K + k] = ex[a][k];
    if (wv == kWaves - 1) {
        // group total = state after the last wavefront
        mat_apply<K, CH>(M64, ws);
        if (lane == 0) {
            double* To = T + ((long long)row * ngroups + g) * (CH * K);
#pragma unroll
            for (int a = 0; a < CH; ++a)
#pragma unroll
                for (int k = 0; k < K; ++k) To[a * K + k] = ws[a][k] + reinterpret_cast<const double*>(lds_all[kWaves - 1])[a * K + k];
        }
    }
}

// kApplyWaves = 3 asks the register allocator for three workgroups per CU (230 -> 168 registers, 120 bytes of scratch per lane), so
// that a 2^20 x 2 call's 683 workgroups would be resident at once instead of 512 + 171: measured SLOWER, 95.9 against 86.5 us of kernels per
// call (profiles/r03_sosfilt.txt) -- the spills cost more than the second, third-full generation.
template <int NS, int CH, int W>
__global__ __launch_bounds__(kWave * W) __attribute__((amdgpu_waves_per_eu(NS <= 2 ? kApplyWaves : 1, 8))) void k_apply(SosCoefs c, SosPass p, int nchunks, int ngroups, const double* __restrict__ zi,
                                                  const double* __restrict__ pw, const double* __restrict__ pwG, const double* __restrict__ pwH,
                                                  const double* __restrict__ E, const double* __restrict__ T,
                                                  double* __restrict__ y1, double* __restrict__ out,
                                                  const double* __restrict__ G, double* __restrict__ E2, double* __restrict__ T2) {
    // E2 != nullptr (forward pass): the kernel also runs the BACKWARD pass's chunk pass on the outputs it holds -- backward chunk c' is
    // this thread's chunk read the other way round (SosPass::mv) -- and leaves its E / T in E2 / T2: no second k_chunk_scan launch, no
    // second read of y1
    constexpr int K = 2 * NS;
    constexpr int kWaves = W, kGroup = kWave * W;
    __shared__ Smp<CH> lds_all[kWaves][kLdsElems];
    __shared__ double lds_m64[K * K];
    __shared__ double red[kWaves][CH * K];
    __shared__ __attribute__((aligned(16))) double c_lds[2];
    const int row = blockIdx.x / ngroups, g = blockIdx.x % ngroups;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wv = tid / kWave;
    const int ch = g * kGroup + tid;
    const long long w0 = ((long long)g * kGroup + wv * kWave) * kChunk;
    const bool plain = wave_is_plain(p, w0);
    const bool active = plain || ch < nchunks;
    const double* base = pass_row<CH>(p, row);
    for (int e = tid; e < K * K; e += kGroup) lds_m64[e] = pw[(long long)kWave * K * K + e];
    // operands fetched ahead of the samples: e_c, this lane's M^lane and (M^256)^lane
    double s[CH][K], Ml[K][K], MG[K][K];
    const double* Eo = E + ((long long)row * ngroups * kGroup + ch) * (CH * K);
#pragma unroll
    for (int a = 0; a < CH; ++a)
#pragma unroll
        for (int k = 0; k < K; ++k) s[a][k] = Eo[a * K + k];
#pragma unroll
    for (int r = 0; r < K; ++r)
#pragma unroll
        for (int q = 0; q < K; ++q) { Ml[r][q] = pw[(long long)lane * K * K + r * K + q]; MG[r][q] = pwG[(long long)lane * K * K + r * K + q]; }
    const long long i0 = (long long)ch * kChunk;
    const int len = (int)(i0 + kChunk <= p.mv ? kChunk : p.mv - i0);
    // the samples: a plain wavefront parks them in its LDS slice until the group's start state is known (they would be 48 registers
    // through the whole reduction: 230 in all, two workgroups per CU, two generations for a 2^20 x 2 call); an edge wavefront keeps them
    // (an edge wavefront loads lane by lane and parks its samples the same way)
    if (active) {
        if (plain) chunk_to_lds<CH>(p, base, w0, lane, lds_all[wv]);
        else {
            Smp<CH> xe[kChunk];
            load_chunk<CH>(p, base, w0, lane, len, false, lds_all[wv], xe);
#pragma unroll
            for (int t = 0; t < kChunk; ++t) lds_all[wv][lane * (kChunk + 1) + t] = xe[t];
            wave_lds_sync();
        }
    }

    // ---- start state of the group: S_g = sum over distances d = 0..g of (M^256)^d v_d,
    //      v_d = T_{g-1-d} for d < g, v_g = s_0 = zi * x_0.  d = 64 a + lane: lane power, then wavefront power.
    double acc[CH][K];
#pragma unroll
    for (int a = 0; a < CH; ++a)
#pragma unroll
        for (int k = 0; k < K; ++k) acc[a][k] = 0.0;
    for (int d0 = 0; d0 <= g; d0 += kGroup) {
        const int d = d0 + tid;
        double v[CH][K], u[CH][K];
        if (d < g) {
            const double* Tj = T + ((long long)row * ngroups + (g - 1 - d)) * (CH * K);
#pragma unroll
            for (int a = 0; a < CH; ++a)
#pragma unroll
                for (int k = 0; k < K; ++k) v[a][k] = Tj[a * K + k];
        } else if (d == g) {
            const Smp<CH> u0 = sos_input<CH>(p, base, 0);
#pragma unroll
            for (int a = 0; a < CH; ++a)
#pragma unroll
                for (int k = 0; k < K; ++k) v[a][k] = zi[k] * u0.v[a];          // zi * x_0 (sosfiltfilt)
        } else {
#pragma unroll
            for (int a = 0; a < CH; ++a)
#pragma unroll
                for (int k = 0; k < K; ++k) v[a][k] = 0.0;
        }
#pragma unroll
        for (int a = 0; a < CH; ++a)
#pragma unroll
            for (int r = 0; r < K; ++r) {
                double t = 0.0;
#pragma unroll
                for (int q = 0; q < K; ++q) t += MG[r][q] * v[a][q];
                u[a][r] = t;
            }
#pragma unroll
        for (int o = kWave / 2; o > 0; o >>= 1)
#pragma unroll
            for (int a = 0; a < CH; ++a)
#pragma unroll
                for (int k = 0; k < K; ++k) u[a][k] += __shfl_xor(u[a][k], o, kWave);
        if (d0 + wv * kWave <= g) mat_acc<K, CH>(pwH + (long long)(d0 / kWave + wv) * K * K, u, acc);      // wave-uniform
    }
    if (lane == 0) {
#pragma unroll
        for (int a = 0; a < CH; ++a)
#pragma unroll
            for (int k = 0; k < K; ++k) red[wv][a * K + k] = acc[a][k];
    }
    __syncthreads();
    double sg[CH][K];
#pragma unroll
    for (int a = 0; a < CH; ++a)
#pragma unroll
        for (int k = 0; k < K; ++k) {
            double t = red[0][a * K + k];
#pragma unroll
            for (int w = 1; w < kWaves; ++w) t += red[w][a * K + k];
            sg[a][k] = t;
        }
    const bool fuse = E2 != nullptr;
    if (!active && !fuse) return;
    Smp<CH> ys[kChunk];                    // this chunk's outputs (kept for the fused chunk pass)
    Smp<CH>* lds = lds_all[wv];
    if (active) {
    Smp<CH> xs[kChunk];
    chunk_from_lds<CH>(lds_all[wv], lane, xs);
    // true start state of the chunk = M^lane (M^64)^wv S_g + e_c
    for (int w = 0; w < wv; ++w) mat_apply<K, CH>(lds_m64, sg);
#pragma unroll
    for (int r = 0; r < K; ++r)
#pragma unroll
        for (int q = 0; q < K; ++q) {
#pragma unroll
            for (int a = 0; a < CH; ++a) s[a][r] += Ml[r][q] * sg[a][q];
        }
    double z[CH][NS][2];
#pragma unroll
    for (int a = 0; a < CH; ++a)
#pragma unroll
        for (int q = 0; q < NS; ++q) { z[a][q][0] = s[a][2 * q]; z[a][q][1] = s[a][2 * q + 1]; }
    double* const dst_f = y1 + (long long)row * p.m * CH;
    double* const dst_b = out + (long long)row * p.n * CH;
    if (plain) {
        // outputs back through LDS, then coalesced stores
#pragma unroll
        for (int t = 0; t < kChunk; ++t) {
#pragma unroll
            for (int a = 0; a < CH; ++a) ys[t].v[a] = sos_step<NS>(c, z[a], xs[t].v[a]);
            lds[lane * (kChunk + 1) + t] = ys[t];
        }
        wave_lds_sync();
#pragma unroll
        for (int t = 0; t < kChunk; ++t) {
            const Smp<CH> y = lds[lds_pos(t * kWave + lane)];
            const long long i = w0 + t * kWave + lane;
            if (!p.backward) st<CH>(dst_f, i, y);
            else {
                // y = reverse(y2)[edge : m - edge]  ->  out[nn] = y2 at forward position nn + edge
                const long long nn = p.mv - 1 - i - p.edge;
                if (nn >= 0 && nn < p.n) st<CH>(dst_b, nn, y);
            }
        }
        wave_lds_sync();
    } else {
#pragma unroll
        for (int t = 0; t < kChunk; ++t)
            if (t < len) {
#pragma unroll
                for (int a = 0; a < CH; ++a) ys[t].v[a] = sos_step<NS>(c, z[a], xs[t].v[a]);
                if (!p.backward) st<CH>(dst_f, i0 + t, ys[t]);
                else {
                    const long long nn = p.mv - 1 - (i0 + t) - p.edge;
                    if (nn >= 0 && nn < p.n) st<CH>(dst_b, nn, ys[t]);
                }
            }
    }
    }
    if (!fuse) return;

    // ---- the backward pass's chunk pass (k_chunk_scan's work) on the outputs of this chunk, read from its end to its start.
    // Positions at and beyond m hold y1[m - 1] (SosPass::mv): the thread that produced it shares it; all such chunks are in the last group.
    const long long last = p.m - 1;
    if (g == ngroups - 1) {
        if ((long long)ch * kChunk <= last && last < (long long)ch * kChunk + kChunk) {
            Smp<CH> cv = ys[0];
#pragma unroll
            for (int t = 1; t < kChunk; ++t) if (i0 + t == last) cv = ys[t];
#pragma unroll
            for (int a = 0; a < CH; ++a) c_lds[a] = cv.v[a];
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < kChunk; ++t)
            if (i0 + t > last) {
#pragma unroll
                for (int a = 0; a < CH; ++a) ys[t].v[a] = c_lds[a];
            }
    }
    // the scan's matrix powers: the last wavefront copies them into its slice (free now), offset 1 KiB
    constexpr int kPwEntries = (kScanSteps + 1) * K * K;
    double* const lds_pw = reinterpret_cast<double*>(lds_all[kWaves - 1]) + 128;
    if (wv == kWaves - 1)
        for (int e = lane; e < kPwEntries; e += kWave) lds_pw[e] = pw[((long long)1 << (e / (K * K))) * K * K + e % (K * K)];
    // this lane's power for the offset of its wavefront inside the group: its backward position in the wavefront is 63 - lane
    double Mb[K][K];
#pragma unroll
    for (int r = 0; r < K; ++r)
#pragma unroll
        for (int q = 0; q < K; ++q) Mb[r][q] = pw[(long long)(kWave - 1 - lane) * K * K + r * K + q];
    double sb[CH][K];
#pragma unroll
    for (int a = 0; a < CH; ++a)
#pragma unroll
        for (int k = 0; k < K; ++k) sb[a][k] = 0.0;
#pragma unroll
    for (int t = 0; t < kChunk; ++t)
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const double gk = G[k * kChunk + t];
#pragma unroll
            for (int a = 0; a < CH; ++a) sb[a][k] = fma(gk, ys[kChunk - 1 - t].v[a], sb[a][k]);
        }
    __syncthreads();                      // lds_pw staged
    wave_scan_rev<K, CH>(sb, lds_pw);
    double exb[CH][K];
    double* const totb = reinterpret_cast<double*>(lds_all[wv]);          // (the wavefront's total, in its own slice)
#pragma unroll
    for (int a = 0; a < CH; ++a)
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const double prev = __shfl_down(sb[a][k], 1, kWave);
            exb[a][k] = lane != kWave - 1 ? prev : 0.0;
            if (lane == 0) totb[a * K + k] = sb[a][k];
        }
    __syncthreads();
    // backward order of the wavefronts: the last one comes first
    double wsb[CH][K];
#pragma unroll
    for (int a = 0; a < CH; ++a)
#pragma unroll
        for (int k = 0; k < K; ++k) wsb[a][k] = 0.0;
    for (int b = 0; b < kWaves - 1 - wv; ++b) {
        mat_apply<K, CH>(lds_m64, wsb);
        const double* tb = reinterpret_cast<const double*>(lds_all[kWaves - 1 - b]);
#pragma unroll
        for (int a = 0; a < CH; ++a)
#pragma unroll
            for (int k = 0; k < K; ++k) wsb[a][k] += tb[a * K + k];
    }
#pragma unroll
    for (int r = 0; r < K; ++r)
#pragma unroll
        for (int q = 0; q < K; ++q) {
#pragma unroll
            for (int a = 0; a < CH; ++a) exb[a][r] += Mb[r][q] * wsb[a][q];
        }
    // backward chunk index of this thread: (chunks in the grid) - 1 - ch; backward group: ngroups - 1 - g
    const long long chb = (long long)ngroups * kGroup - 1 - ch;
    double* Eb = E2 + ((long long)row * ngroups * kGroup + chb) * (CH * K);
#pragma unroll
    for (int a = 0; a < CH; ++a)
#pragma unroll
        for (int k = 0; k < K; ++k) Eb[a * K + k] = exb[a][k];
    if (wv == 0) {
        // group total = state after the last wavefront in backward order (this one)
        mat_apply<K, CH>(lds_m64, wsb);
        if (lane == 0) {
            double* Tb = T2 + ((long long)row * ngroups + (ngroups - 1 - g)) * (CH * K);
            const double* tb = reinterpret_cast<const double*>(lds_all[0]);
#pragma unroll
            for (int a = 0; a < CH; ++a)
#pragma unroll
                for (int k = 0; k < K; ++k) Tb[a * K + k] = wsb[a][k] + tb[a * K + k];
        }
    }
}

// ------------------------------------------------------------------------------------------ one launch
// The whole forward-backward filter in ONE launch, for calls whose workgroups are all resident at once (host: `one_launch_capacity`).
// A workgroup keeps its 256 chunks in registers / LDS from the first load to the last store and meets the others twice, through
// the group totals in HBM: forward it needs the totals of every EARLIER group of its row, backward those of every LATER one.  Each
// total goes out with a flag (= the call's epoch; the flags are never reset); a reader polls the flags of the totals it needs with
// agent-scope loads.  x is read once, the result written once -- 16 B per real sample, the algorithmic minimum, against 51 of the
// three-launch form (no y1, no chunk states in HBM at all).
// With every workgroup in the same phase at the same time nothing hides a trip to memory, and while the samples stream in or out
// such a trip takes microseconds: between the sample loads and the sample stores the kernel touches global memory only for the
// totals -- the scan's matrix powers live in LDS for the whole launch (in the pad elements of the staging slices, which the sample
// traffic never touches), the per-lane powers are asked for ahead of the waits.
// A workgroup that waits longer than `patience` (another process's grid sharing the GPU could keep part of this one out) raises
// `*status` and leaves; the host then repeats the call with the three-launch form (x is never written).
struct SosLink {
    double* T;            // [2][gridDim.x][CH * K]: forward totals (+ the start state's image in group 0's), then backward
    unsigned* flag;       // [2][gridDim.x]
    int* status;          // host-visible
    unsigned epoch;
    long long patience;   // ticks of the 100 MHz clock
    unsigned long long* U;     // tagged totals (orders whose total is at most 8 doubles): [2][gridDim.x][N] 16-byte units {value, tag} -- see group_start
    unsigned long long tag;    // this call's tag: the workspace's call counter, never repeated
    const double* pwT;    // the per-lane powers M^lane, element-major: [K * K][64] -- a wavefront's load of one element is 512 contiguous bytes.  (Round 4
                          // read them lane-major, pw[lane][K * K]: 64 cache lines per load instruction, 12-16 instructions per matrix, four matrices per
                          // thread -- 4 us of a workgroup's 37 went into each of these gathers: profiles/r05_sos_timeline.txt, the groups that wait for nobody.)
    const double* pwGT;   // the same for the group powers (M^group)^lane
    long long* tl;        // SOS_TIMELINE builds: [gridDim.x][16] clock readings of a workgroup's phases (dev aid), else unused
    const double* meetV;  // single-meeting kernels (k_filtfilt<.., true>): [2][K * K][threads] -- the backward state at the start of a thread's chunk that a unit start
                          // state of the thread's GROUP causes through the forward outputs of the chunks behind it; [0]: any whole group, [1]: the row's last
    const double* meetW;  // [2][K * K]: the same at the group's end (what the unit start state adds to the group's backward total)
    int look;             // > 0: (M^group)^d is below 1e-40 in every element from d = look on -- a group's start state is made of its `look` nearest
                          // totals alone (group_start_near); 0: of all of them (group_start)
};
#ifndef SOS_TIMELINE
#define SOS_TIMELINE 0
#endif
#if SOS_TIMELINE
#define SOS_MARK(i) do { if (threadIdx.x == 0 && L.tl) L.tl[(long long)blockIdx.x * 16 + (i)] = wall_clock64(); } while (0)
#else
#define SOS_MARK(i) do { } while (0)
#endif

// No fences in the hand-over: an agent-scope release / acquire is a write-back / invalidate of the XCD's whole L2 on gfx950
// (buffer_wbl2 / buffer_inv sc1), and with 684 workgroups doing both twice a 2^20 x 2 call took 141 us, its workgroups 12 to 55 us
// from "samples loaded" to "total published" (profiles/r03_sosfilt.txt).  Instead the totals are written through (sc1 stores), the
// writer waits for their acknowledgement before it raises the flag, and readers fetch them with sc1 loads, which go past the caches.
typedef double sos_d2v __attribute__((ext_vector_type(2)));

// Doubles `e` of the workgroup's LDS-resident table (scan powers M^1 .. M^32, M^64, then the wavefronts' carries and totals): pad
// element number e / CH of the staging slices (slice-major), component e % CH.  Compile-time `e` -> an immediate offset.
template <int CH> struct PadTable {
    Smp<CH>* slices;       // lds_all[0]
    __device__ __forceinline__ double& operator[](int e) const {
        const int pad = e / CH;
        return slices[(pad / kWave) * kLdsElems + (pad % kWave) * (kChunk + 1) + kChunk].v[e % CH];
    }
};
template <int K, int CH, class Tab> __device__ __forceinline__ void mat_acc_t(const Tab& M, int base, const double (&x)[CH][K], double (&y)[CH][K]) {
#pragma unroll
    for (int r = 0; r < K; ++r)
#pragma unroll
        for (int q = 0; q < K; ++q) {
            if (q / 2 > r / 2) continue;
            const double mrq = M[base + r * K + q];
#pragma unroll
            for (int c = 0; c < CH; ++c) y[c][r] += mrq * x[c][q];
        }
}
template <int K, int CH, class Tab> __device__ __forceinline__ void mat_apply_t(const Tab& M, int base, double (&x)[CH][K]) {
    double y[CH][K];
#pragma unroll
    for (int c = 0; c < CH; ++c)
#pragma unroll
        for (int k = 0; k < K; ++k) y[c][k] = 0.0;
    mat_acc_t<K, CH>(M, base, x, y);
#pragma unroll
    for (int c = 0; c < CH; ++c)
#pragma unroll
        for (int k = 0; k < K; ++k) x[c][k] = y[c][k];
}
// wave_scan / wave_scan_rev with the powers in a PadTable
template <int K, int CH, bool REV, class Tab> __device__ __forceinline__ void wave_scan_t(double (&x)[CH][K], const Tab& pwt) {
    const int lane = threadIdx.x & (kWave - 1);
#pragma unroll
    for (int k = 0; k < kScanSteps; ++k) {
        const int d = 1 << k;
        double up[CH][K];
#pragma unroll
        for (int c = 0; c < CH; ++c)
#pragma unroll
            for (int q = 0; q < K; ++q) up[c][q] = REV ? __shfl_down(x[c][q], d, kWave) : __shfl_up(x[c][q], d, kWave);
        if (REV ? lane + d < kWave : lane >= d) mat_acc_t<K, CH>(pwt, k * K * K, up, x);       // (the others have no partner: one branch instead of 2 N selects)
    }
}

// ---- the same scan with the shifts inside the 16 lanes of a DPP row (round 5).  wave_scan_t moves 8 doubles by ds_bpermute in each of its six steps and
// reads the step's matrix from LDS: 28 LDS operations per step and wavefront, eight wavefronts per CU -- the scan is bound by the LDS pipe (2.6 us of a
// workgroup's 35).  Here: four steps inside the rows (row_shr / row_shl: a DPP move is a VALU operation, lanes without a partner in their row get zeros), then the
// three row totals are read with v_readlane, carried from row to row with M^16 (uniform arithmetic), and every lane adds its row's entering state through ITS power
// M^(position in the row + 1), which it holds in registers (`Mrow`, fetched long before).  12 LDS reads per step instead of 28, four + two steps instead of six.
template <int CTRL> __device__ __forceinline__ double dpp_shift(double v) {
    const unsigned long long b = __builtin_bit_cast(unsigned long long, v);
    const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)b, CTRL, 0xf, 0xf, true);
    const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(b >> 32), CTRL, 0xf, 0xf, true);
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ double lane_of(double v, int src_lane) {          // (src_lane uniform) the value a lane holds, for all: v_readlane
    const unsigned long long b = __builtin_bit_cast(unsigned long long, v);
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)b, src_lane);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(b >> 32), src_lane);
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}
template <int K, int CH, bool REV, int D, class Tab> __device__ __forceinline__ void row_scan_step(double (&x)[CH][K], const Tab& pwt, int k) {
    double up[CH][K];
#pragma unroll
    for (int c = 0; c < CH; ++c)
#pragma unroll
        for (int q = 0; q < K; ++q) up[c][q] = dpp_shift<(REV ? 0x100 : 0x110) + D>(x[c][q]);          // row_shl:D / row_shr:D, zeros from outside the row
    mat_acc_t<K, CH>(pwt, k * K * K, up, x);
}
// Mrow = this lane's M^((lane & 15) + 1) (forward) or M^(16 - (lane & 15)) (REV)
template <int K, int CH, bool REV, class Tab> __device__ __forceinline__ void wave_scan_rows(double (&x)[CH][K], const Tab& pwt, const double (&Mrow)[K][K]) {
    const int lane = threadIdx.x & (kWave - 1);
    row_scan_step<K, CH, REV, 1>(x, pwt, 0);
    row_scan_step<K, CH, REV, 2>(x, pwt, 1);
    row_scan_step<K, CH, REV, 4>(x, pwt, 2);
    row_scan_step<K, CH, REV, 8>(x, pwt, 3);
    // the state entering each row from the rows before it (REV: behind it): Q = R of the neighbouring row + M^16 (the one before)
    double Q[CH][K], mine[CH][K];
#pragma unroll
    for (int c = 0; c < CH; ++c)
#pragma unroll
        for (int q = 0; q < K; ++q) { Q[c][q] = 0.0; mine[c][q] = 0.0; }
    const int row = lane >> 4;
#pragma unroll
    for (int r = 1; r < 4; ++r) {
        // forward: rows 1, 2, 3 in turn, fed by the total of row r - 1 (its lane 15); REV: rows 2, 1, 0, fed by the total of the row above (its lane 0)
        const int src = REV ? 16 * (4 - r) : 16 * (r - 1) + 15;
        if (r > 1) mat_apply_t<K, CH>(pwt, 4 * K * K, Q);                    // M^16
#pragma unroll
        for (int c = 0; c < CH; ++c)
#pragma unroll
            for (int q = 0; q < K; ++q) {
                Q[c][q] += lane_of(x[c][q], src);
                mine[c][q] = row == (REV ? 3 - r : r) ? Q[c][q] : mine[c][q];
            }
    }
    mat_acc<K, CH>(&Mrow[0][0], mine, x);
}

// acc = start state of group number `g` of its pass = sum_{d < g} (M^group)^d T'_{g-1-d}; T'_j = the published totals of the row
// (`Tb`, `Fb`: the row's totals and flags in the pass's own group order).  Waits for each of them: all flags first, then all totals
// in one round of loads.
//
// Round 5: the hand-over is a chain of trips to memory -- total written through, acknowledged (2-4 us at that moment), flag written, flag seen by
// a poll, total fetched: 8-10 us per pass, twice per call, of a 37 us kernel (profiles/r05_sos_timeline.txt: even a group that waits for nobody
// spent 4.5 us at its barrier, behind its own publisher's acknowledgement).  Totals of up to 8 doubles (orders up to 4 complex, 8 real) now
// carry their own validity: a total is N 16-byte units {value, tag}, tag = the workspace's call counter, written by ONE store instruction (lane e
// stores unit e) with no acknowledgement awaited and no flag; a reader polls the units themselves and takes a total when all its tags are this
// call's.  A 16-byte aligned unit is one request to one memory channel, for the store and for the load: it is never seen half-written.
template <int K, int CH, int W, bool TAGGED>
__device__ __forceinline__ void group_start(const SosLink& L, const double* Tb, const unsigned* Fb, const unsigned long long* Ub, int g, const double* __restrict__ pwG,
                                            const double* __restrict__ pwH, double (&acc)[CH][K], int* s_fail) {
    constexpr int kGroup = kWave * W, N = CH * K;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wv = __builtin_amdgcn_readfirstlane(tid / kWave);
    double MG[K][K];
#pragma unroll
    for (int r = 0; r < K; ++r)
#pragma unroll
        for (int q = 0; q < K; ++q) MG[r][q] = L.pwGT[(r * K + q) * kWave + lane];
#pragma unroll
    for (int a = 0; a < CH; ++a)
#pragma unroll
        for (int k = 0; k < K; ++k) acc[a][k] = 0.0;
    const long long t0 = wall_clock64();
    typedef unsigned int sos_u4 __attribute__((ext_vector_type(4)));
    double tv[kLookIter][N];                         // the totals this thread answers for
    if constexpr (TAGGED) {
        const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned long long*>(Ub), 0, g * N * 16, 0x00020000);
        const unsigned tag_lo = (unsigned)L.tag, tag_hi = (unsigned)(L.tag >> 32);
#pragma unroll
        for (int it = 0; it < kLookIter; ++it) {
#pragma unroll
            for (int i = 0; i < N; ++i) tv[it][i] = 0.0;
            if (it * kGroup >= g) continue;              // (uniform)
            const int d = it * kGroup + tid;
            if (d < g) {
                // first the LAST unit alone, until it carries this call's tag (16 bytes per total and round: polling whole totals was 13 MB per round
                // over the grid, and the groups with many totals to fetch started 3-4 us behind those with few); then the whole total, every tag looked at
                const int off = (g - 1 - d) * N * 16;
                for (;;) {
                    const sos_u4 lastu = __builtin_amdgcn_raw_buffer_load_b128(rsrc, off + 16 * (N - 1), 0, 16 /* sc1 */);
                    if (lastu.z == tag_lo && lastu.w == tag_hi) break;
                    if (wall_clock64() - t0 > L.patience) { *s_fail = 1; break; }
                    __builtin_amdgcn_s_sleep(1);            // (8 / 32 / 100 instead of 1: nothing or worse, profiles/r05_sos_handover_ab.txt visit 4)
                }
                for (;;) {
                    sos_u4 raw[N];
#pragma unroll
                    for (int i = 0; i < N; ++i) raw[i] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, off + 16 * i, 0, 16 /* sc1 */);
                    bool ok = true;
#pragma unroll
                    for (int i = 0; i < N; ++i) ok = ok && raw[i].z == tag_lo && raw[i].w == tag_hi;
                    if (ok) {
#pragma unroll
                        for (int i = 0; i < N; ++i) tv[it][i] = __builtin_bit_cast(double, ((unsigned long long)raw[i].y << 32) | raw[i].x);
                        break;
                    }
                    if (wall_clock64() - t0 > L.patience) { *s_fail = 1; break; }
                    __builtin_amdgcn_s_sleep(1);            // (8 / 32 / 100 instead of 1: nothing or worse, profiles/r05_sos_handover_ab.txt visit 4)
                }
            }
        }
    } else {
#pragma unroll
        for (int it = 0; it < kLookIter; ++it) {
            const int d = it * kGroup + tid;
            if (d < g) {
                while (__hip_atomic_load(Fb + (g - 1 - d), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != L.epoch) {
                    if (wall_clock64() - t0 > L.patience) { *s_fail = 1; break; }
                    __builtin_amdgcn_s_sleep(1);            // (8 / 32 / 100 instead of 1: nothing or worse, profiles/r05_sos_handover_ab.txt visit 4)
                }
            }
        }
        // the totals: 16-byte sc1 buffer loads (compiler-tracked; the flat-address form of an sc1 load only exists as inline assembly, whose
        // result registers the compiler would be free to copy or spill before the data is there)
        const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<double*>(Tb), 0, g * N * (int)sizeof(double), 0x00020000);
#pragma unroll
        for (int it = 0; it < kLookIter; ++it) {
            const int d = it * kGroup + tid;
            const int off = d < g ? (g - 1 - d) * N * (int)sizeof(double) : 0x7ffffff0;        // (beyond the descriptor's range: the load returns zeros)
#pragma unroll
            for (int i = 0; i < N; ++i) tv[it][i] = 0.0;
            if (it * kGroup < g) {                       // (uniform)
#pragma unroll
                for (int i = 0; i < N / 2; ++i) {
                    const sos_d2v two = __builtin_bit_cast(sos_d2v, __builtin_amdgcn_raw_buffer_load_b128(rsrc, off + 16 * i, 0, 16 /* sc1 */));
                    tv[it][2 * i] = two.x; tv[it][2 * i + 1] = two.y;
                }
            }
        }
    }
    // per lane: (M^group)^(64 (it W + wv)) (M^group)^lane T' for each round, summed; ONE reduction over the wavefront at the end
#pragma unroll
    for (int it = 0; it < kLookIter; ++it) {
        if (it * kGroup >= g) break;                 // (uniform)
        double u[CH][K], vv[CH][K];
#pragma unroll
        for (int a = 0; a < CH; ++a)
#pragma unroll
            for (int qq = 0; qq < K; ++qq) {
                vv[a][qq] = tv[it][a * K + qq];
                u[a][qq] = 0.0;
            }
        mat_acc<K, CH>(&MG[0][0], vv, u);
        if (it * kGroup + wv * kWave < g) mat_acc<K, CH>(pwH + (long long)(it * W + wv) * K * K, u, acc);      // wave-uniform, scalar loads
    }
    // the sum over the wavefront, for every lane: inside the rows by DPP (two quad permutations, row_half_mirror, row_mirror), the four rows by v_readlane --
    // VALU moves instead of the 96 ds_bpermute of a shuffle butterfly (see wave_scan_rows: the LDS pipe is what this kernel's short phases wait for)
#pragma unroll
    for (int a = 0; a < CH; ++a)
#pragma unroll
        for (int k = 0; k < K; ++k) {
            double v = acc[a][k];
            v += dpp_shift<0xB1>(v);            // quad_perm:[1,0,3,2]
            v += dpp_shift<0x4E>(v);            // quad_perm:[2,3,0,1]
            v += dpp_shift<0x141>(v);           // row_half_mirror
            v += dpp_shift<0x140>(v);           // row_mirror
            acc[a][k] = (lane_of(v, 0) + lane_of(v, 16)) + (lane_of(v, 32) + lane_of(v, 48));
        }
}

// Round 6: the same start state from the NEAREST totals alone.  The group map (M^chunk)^(64 W) is the cascade run over 3072 ... 4608 samples: for every
// filter this library's callers design (cut-offs down to fs / 500: LPF / BPF warn below) its powers fall under 1e-40 within one to three groups -- 1e-126
// after ONE at fs / 100 -- and a term of that size changes no bit of a state of the samples' own magnitude.  The host measures it (`look` = 1 + the last d with
// an element of (M^group)^d at or above 1e-40, over the 64 powers it builds anyway; SosLink::look = 0 when that is more than kNear) and a workgroup then waits
// for `look` totals instead of for all the earlier ones of its row (up to 227 at 2^20: 2.5 us of a wait of 7, profiles/r05_final_sos_timeline.txt).  Every
// wavefront polls and sums by itself -- uniform addresses: one request per instruction -- so no reduction across lanes or wavefronts follows.
template <int K, int CH>
__device__ __forceinline__ void group_start_near(const SosLink& L, const unsigned long long* Ub, int g, const double* __restrict__ pwG, double (&acc)[CH][K], int* s_fail) {
    constexpr int N = CH * K;
    typedef unsigned int sos_u4 __attribute__((ext_vector_type(4)));
#pragma unroll
    for (int a = 0; a < CH; ++a)
#pragma unroll
        for (int k = 0; k < K; ++k) acc[a][k] = 0.0;
    if (g == 0) return;
    const long long t0 = wall_clock64();
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned long long*>(Ub), 0, g * N * 16, 0x00020000);
    const unsigned tag_lo = (unsigned)L.tag, tag_hi = (unsigned)(L.tag >> 32);
    for (int d = 0; d < L.look && d < g; ++d) {
        const int off = (g - 1 - d) * N * 16;
        double vv[CH][K];
        for (;;) {
            sos_u4 raw[N];
#pragma unroll
            for (int i = 0; i < N; ++i) raw[i] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, off + 16 * i, 0, 16 /* sc1 */);
            bool ok = true;
#pragma unroll
            for (int i = 0; i < N; ++i) ok = ok && raw[i].z == tag_lo && raw[i].w == tag_hi;
            if (ok) {
#pragma unroll
                for (int i = 0; i < N; ++i) vv[i / K][i % K] = __builtin_bit_cast(double, ((unsigned long long)raw[i].y << 32) | raw[i].x);
                break;
            }
            if (wall_clock64() - t0 > L.patience) {
                *s_fail = 1;
#pragma unroll
                for (int i = 0; i < N; ++i) vv[i / K][i % K] = 0.0;
                break;
            }
            __builtin_amdgcn_s_sleep(1);
        }
        mat_acc<K, CH>(pwG + (long long)d * K * K, vv, acc);          // (M^group)^d, d = 0: the unit matrix of the host's table
    }
}

// ---- ONE meeting instead of two (round 6; DESIGN.md section 7).  Every group runs BOTH its passes from a zero start state (group 0 from the row's true one)
// and publishes both totals at once: T_g (forward) and T'0_g (backward, of the outputs y0 that the zero start state gives).  The true forward outputs
// are y0 + the zero-input response to the group's true start state S_g, and everything behind them is linear in S_g: the group's backward total is
// T'0_g + Wm S_g and the backward state at the start of a thread's chunk moves by Vm[thread] S_g, with Wm (K x K) and Vm (K x K per thread) run on the host from
// unit states -- one pair for whole groups, one for the row's last group (its ragged end, the virtual copies of the last output and SciPy's zi * y[-1] all
// depend on that output: their share is inside that pair).  With the look-back of group_start_near at most TWO groups deep a workgroup needs
//      S_g      = T_{g-1} + Mg T_{g-2}                                       (forward; Mg = the group map)
//      S'_g     = T'_{g+1} + Mg T'_{g+2},   T'_j = T'0_j + Wm S_j,  S_j from T_{j-1}, T_{j-2}
// that is four forward totals (g-2 .. g+1) and two backward ones: 6 N <= 48 16-byte units, ONE per lane, polled by every wavefront for itself until all carry
// the call's tag.  Terms whose group does not exist are zero.  Then: the zero-input response onto y0, the chunk's backward start state, the backward outputs.
template <int K, int CH>
__device__ __forceinline__ bool meet_states(const SosLink& L, long long f_unit0, long long b_unit0, int g, int gb, int ngroups, const double* __restrict__ pwG,
                                            double (&sd)[CH][K], double (&sb)[CH][K]) {
    constexpr int N = CH * K;
    static_assert(6 * N <= kWave, "one unit per lane");
    typedef unsigned int sos_u4 __attribute__((ext_vector_type(4)));
    const int lane = threadIdx.x & (kWave - 1);
    const int slot = lane / N, e = lane % N;                     // slots 0..3: forward totals g - 2 + slot; 4, 5: backward totals gb - 2 + (slot - 4)
    const int idx = slot < 4 ? g - 2 + slot : gb - 6 + slot;
    const bool wanted = L.look > 1 || slot == 1 || slot == 2 || slot == 5;
    const bool valid = wanted && slot < 6 && idx >= 0 && idx <= ngroups - 2 && (slot < 4 || idx < gb);
    const long long unit = (slot < 4 ? f_unit0 : b_unit0) + (long long)idx * N + e;
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned long long*>(L.U), 0, 0x7ffffff0, 0x00020000);
    const unsigned tag_lo = (unsigned)L.tag, tag_hi = (unsigned)(L.tag >> 32);
    const int off = valid ? (int)(unit * 16) : 0;
    double val = 0.0;
    bool ok = !valid;
    const long long t0 = wall_clock64();
    for (;;) {
        if (!ok) {
            const sos_u4 raw = __builtin_amdgcn_raw_buffer_load_b128(rsrc, off, 0, 16 /* sc1 */);
            if (raw.z == tag_lo && raw.w == tag_hi) {
                ok = true;
                val = __builtin_bit_cast(double, ((unsigned long long)raw.y << 32) | raw.x);
            }
        }
        if (__all(ok)) break;
        if (wall_clock64() - t0 > L.patience) return false;
        __builtin_amdgcn_s_sleep(1);
    }
    const double* Mg = pwG + K * K;
    const auto total = [&](int sl, double (&t)[CH][K]) {
#pragma unroll
        for (int a = 0; a < CH; ++a)
#pragma unroll
            for (int k = 0; k < K; ++k) t[a][k] = lane_of(val, sl * N + a * K + k);
    };
    const auto full_acc = [&](const double* Wm, const double (&x)[CH][K], double (&y)[CH][K]) {
#pragma unroll
        for (int r = 0; r < K; ++r)
#pragma unroll
            for (int q = 0; q < K; ++q) {
                const double m = Wm[r * K + q];
#pragma unroll
                for (int a = 0; a < CH; ++a) y[a][r] += m * x[a][q];
            }
    };
    // (written so that few of the uniform values live at once: the lanes' units stay in `val`, a total is read from there where it is used)
    const bool deep = L.look > 1;                                // (uniform) one group back, or two
    total(1, sd);                                                // S_g = T_{g-1} + Mg T_{g-2}
    if (deep) {
        double f[CH][K];
        total(0, f);
        mat_acc<K, CH>(Mg, f, sd);
    }
    {
        double s1[CH][K];                                        // S_{g+1} = T_g + Mg T_{g-1}
        total(2, s1);
        if (deep) {
            double f[CH][K];
            total(1, f);
            mat_acc<K, CH>(Mg, f, s1);
        }
        total(5, sb);                                            // T'_{g+1} = T'0_{g+1} + Wm S_{g+1}: the backward total number gb - 1
        full_acc(L.meetW + (g + 1 == ngroups - 1 ? K * K : 0), s1, sb);
#pragma unroll
        for (int a = 0; a < CH; ++a)
#pragma unroll
            for (int k = 0; k < K; ++k) sb[a][k] = gb >= 1 ? sb[a][k] : 0.0;
    }
    if (deep && gb >= 2) {
        double s2[CH][K], t2[CH][K];                             // S_{g+2} = T_{g+1} + Mg T_g;  T'_{g+2}: the backward total number gb - 2
        total(3, s2);
        total(2, t2);
        mat_acc<K, CH>(Mg, t2, s2);
        total(4, t2);
        full_acc(L.meetW + (g + 2 == ngroups - 1 ? K * K : 0), s2, t2);
        mat_acc<K, CH>(Mg, t2, sb);
    }
    return true;
}

template <int NS, int CH, int W, bool MEET = false>
__global__ __launch_bounds__(kWave * W) __attribute__((amdgpu_waves_per_eu(NS <= 2 ? (W != kWavesSmall ? kApplyWaves : SOS_SMALL_EU) : 1, 8))) void k_filtfilt(
    SosCoefs c, SosPass p, int nchunks, int ngroups, const double* __restrict__ zi, const double* __restrict__ pw,
    const double* __restrict__ pwG, const double* __restrict__ pwH, const double* __restrict__ G, double* __restrict__ out, SosLink L) {
    constexpr int K = 2 * NS, N = CH * K;
    constexpr int kWaves = W, kGroup = kWave * W;
    constexpr int kPwEntries = (kScanSteps + 1) * K * K;       // M^1, M^2 .. M^32, M^64
    // (one wavefront, long chunk, order-4 complex: the chunk sums' weights G stay in memory -- uniform addresses, the scalar cache -- so that the rest of the table fits the
    // pad elements and EIGHT workgroups fit a CU's LDS: the shape that holds 2^20 x 2 complex128 in one-wavefront workgroups)
    constexpr bool kGGlobal = W == 1 && kChunk > 12 && CH == 2 && NS == 2;
    constexpr int kM64 = kScanSteps * K * K, kCarry = kPwEntries, kTot = kCarry + kWaves * N, kG = kTot + kWaves * N, kTabSize = kG + (kGGlobal ? 0 : K * kChunk);
    constexpr bool kPads = kTabSize <= kWave * kWaves * CH;       // the table fits the slices' pad elements
    constexpr bool kAhead = W == kWavesSmall && SOS_SMALL_AHEAD;
    __shared__ Smp<CH> lds_all[kWaves][kLdsElems];
    __shared__ double red[kWaves][N];
    __shared__ __attribute__((aligned(16))) double c_lds[2];
    __shared__ __attribute__((aligned(16))) int s_fail[4];
    __shared__ __attribute__((aligned(16))) double v0_lds[N];            // the pass's start state zi * (first sample), in the group that holds it
    __shared__ __attribute__((aligned(16))) double tab_lds[kPads ? 2 : kTabSize];
    struct FlatTable { double* t; __device__ __forceinline__ double& operator[](int e) const { return t[e]; } };
    const PadTable<CH> padt{&lds_all[0][0]};
    const FlatTable flatt{tab_lds};
    const auto tabv = [&](int e) -> double& { if constexpr (kPads) return padt[e]; else return flatt[e]; };
    struct TabRef { decltype(tabv) f; __device__ __forceinline__ double& operator[](int e) const { return f(e); } };
    const TabRef tab{tabv};
    const int row = blockIdx.x / ngroups, g = blockIdx.x % ngroups, gb = ngroups - 1 - g;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wv = __builtin_amdgcn_readfirstlane(tid / kWave);
    const int ch = g * kGroup + tid;
    const long long w0 = ((long long)g * kGroup + wv * kWave) * kChunk;
    const bool plain = wave_is_plain(p, w0);
    const bool active = plain || ch < nchunks;
    const double* base = pass_row<CH>(p, row);
    const long long i0 = (long long)ch * kChunk;
    const int len = (int)(i0 + kChunk <= p.mv ? kChunk : p.mv - i0);
    Smp<CH>* const lds = lds_all[wv];
    double* const Tf = L.T + (long long)row * ngroups * N;
    double* const Tbk = L.T + ((long long)gridDim.x + (long long)row * ngroups) * N;
    unsigned* const Ff = L.flag + (long long)row * ngroups;
    unsigned* const Fbk = L.flag + (long long)gridDim.x + (long long)row * ngroups;
    constexpr bool kTagged = N <= 8;                                     // the totals carry their own validity (group_start)
    constexpr bool kRowScan = NS <= 2 && (kChunk > 12 || W == kWavesSmall);       // the wavefront scans with DPP rows (wave_scan_rows; not the shape held to 168 registers); the lane's row power, forward:
    double Mrow[K][K];
    if constexpr (kRowScan) {
#pragma unroll
        for (int r = 0; r < K; ++r)
#pragma unroll
            for (int q = 0; q < K; ++q) Mrow[r][q] = L.pwT[(r * K + q) * kWave + (lane & 15) + 1];
    }
    unsigned long long* const Uf = L.U + (long long)row * ngroups * N * 2;
    unsigned long long* const Ubk = L.U + ((long long)gridDim.x + (long long)row * ngroups) * N * 2;
    // lane e of the publishing wavefront stores unit e = {value e of the total, the call's tag}: one store instruction, one 128-byte line
    const auto publish = [&](unsigned long long* U, int idx, const double (&tot)[CH][K]) {
        double v = 0.0;
#pragma unroll
        for (int e = 0; e < N; ++e) v = lane == e ? tot[e / K][e % K] : v;
        if (lane < N) {
            typedef unsigned long long sos_ul2 __attribute__((ext_vector_type(2)));
            const sos_ul2 unit = {__builtin_bit_cast(unsigned long long, v), L.tag};
            asm volatile("global_store_dwordx4 %0, %1, off sc1" : : "v"(reinterpret_cast<sos_ul2*>(U + ((long long)idx * N + lane) * 2)), "v"(unit) : "memory");
        }
    };
    if (tid == 0) s_fail[0] = 0;
    SOS_MARK(0);
#if SOS_TIMELINE
    if (threadIdx.x == 0 && L.tl) {
        unsigned hw_, xc_;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw_));
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xc_));
        L.tl[(long long)blockIdx.x * 16 + 14] = hw_;
        L.tl[(long long)blockIdx.x * 16 + 15] = xc_;
    }
#endif
    // the scan's powers -> the LDS table (the pads are nobody else's: no barrier needed before the samples use the slices)
    for (int e0 = tid; e0 < kPwEntries + (kGGlobal ? 0 : K * kChunk); e0 += kGroup) {
        const bool is_g = e0 >= kPwEntries;
        const int e = is_g ? kG + (e0 - kPwEntries) : e0;
        const double val = is_g ? G[e0 - kPwEntries] : pw[((long long)1 << (e0 / (K * K))) * K * K + e0 % (K * K)];
        if constexpr (kPads) {
            const int pad = e / CH;
            lds_all[0][(pad / kWave) * kLdsElems + (pad % kWave) * (kChunk + 1) + kChunk].v[e % CH] = val;
        } else tab_lds[e] = val;
    }
    // the image of the pass's start state zi * x_0 under one group map goes out with group 0's total; group 0 itself starts from it
    if (g == 0 && tid == 0) {
        const Smp<CH> u0 = sos_input<CH>(p, base, 0);
#pragma unroll
        for (int a = 0; a < CH; ++a)
#pragma unroll
            for (int k = 0; k < K; ++k) v0_lds[a * K + k] = zi[k] * u0.v[a];
    }

    // ---- forward chunk pass (k_chunk_scan's work; the chunk states stay in registers)
    Smp<CH> xs[kChunk];
    double ex[CH][K];                     // the chunk's start state if its WAVEFRONT started from zero
    {
        double s[CH][K];
#pragma unroll
        for (int a = 0; a < CH; ++a)
#pragma unroll
            for (int k = 0; k < K; ++k) s[a][k] = 0.0;
        if (plain || g * kGroup + wv * kWave < nchunks) {          // (the whole wavefront moves its 768 samples, whichever lanes hold chunks)
            if (plain) chunk_to_lds<CH>(p, base, w0, lane, lds);
            else chunk_to_lds_edge<CH>(p, base, w0, lane, lds);
            chunk_from_lds<CH>(lds, lane, xs);
        }
        SOS_MARK(1);
        __syncthreads();                      // table, s_fail, v0 staged
        if (active) {
            // A short last chunk ends `len` samples in: its sample t has the weight of sample kChunk - len + t of a full one -- the same sum over the
            // samples moved to the chunk's end behind zeros.  The lane reads them again from its slice, shifted (round 4 indexed the weights by a run-time
            // offset instead: the pad-element table's index arithmetic per access made the row's LAST group, whose total every group of the backward pass
            // waits for, 3 us late: profiles/r05_sos_timeline.txt).  The samples themselves stay in the slice for the output pass.
            if (len != kChunk) {
                const int off = kChunk - len;
#pragma unroll
                for (int t = 0; t < kChunk; ++t) {
                    const Smp<CH> v = lds[lane * (kChunk + 1) + (t >= off ? t - off : 0)];
#pragma unroll
                    for (int a = 0; a < CH; ++a) xs[t].v[a] = t >= off ? v.v[a] : 0.0;
                }
            }
#pragma unroll
            for (int t = 0; t < kChunk; ++t)
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const double gk = kGGlobal ? G[k * kChunk + t] : tab[kG + k * kChunk + t];
#pragma unroll
                    for (int a = 0; a < CH; ++a) s[a][k] = fma(gk, xs[t].v[a], s[a][k]);
                }
        }
        SOS_MARK(2);
        if constexpr (kRowScan) wave_scan_rows<K, CH, false>(s, tab, Mrow);
        else wave_scan_t<K, CH, false>(s, tab);
        if constexpr (kRowScan) {              // (the backward scan's row power: asked for now, used after the forward outputs)
#pragma unroll
            for (int r = 0; r < K; ++r)
#pragma unroll
                for (int q = 0; q < K; ++q) Mrow[r][q] = L.pwT[(r * K + q) * kWave + 16 - (lane & 15)];
        }
#pragma unroll
        for (int a = 0; a < CH; ++a)
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const double prev = kRowScan ? dpp_shift<0x138>(s[a][k]) : __shfl_up(s[a][k], 1, kWave);          // (wave_shr:1)
                ex[a][k] = lane ? prev : 0.0;
                if (lane == kWave - 1) tab[kTot + wv * N + a * K + k] = s[a][k];
            }
        __syncthreads();
        SOS_MARK(3);
        // start state of this wavefront if the GROUP started from zero: ws_{w+1} = M^64 ws_w + tot_w.  Kept in the table (wave-uniform).
        double ws[CH][K];
#pragma unroll
        for (int a = 0; a < CH; ++a)
#pragma unroll
            for (int k = 0; k < K; ++k) ws[a][k] = 0.0;
        for (int w = 0; w < wv; ++w) {
            mat_apply_t<K, CH>(tab, kM64, ws);
#pragma unroll
            for (int a = 0; a < CH; ++a)
#pragma unroll
                for (int k = 0; k < K; ++k) ws[a][k] += tab[kTot + w * N + a * K + k];
        }
        if (lane == 0) {
#pragma unroll
            for (int a = 0; a < CH; ++a)
#pragma unroll
                for (int k = 0; k < K; ++k) tab[kCarry + wv * N + a * K + k] = ws[a][k];
        }
        if (wv == kWaves - 1 && g + 1 < ngroups) {
            mat_apply_t<K, CH>(tab, kM64, ws);
#pragma unroll
            for (int a = 0; a < CH; ++a)
#pragma unroll
                for (int k = 0; k < K; ++k) ws[a][k] += tab[kTot + (kWaves - 1) * N + a * K + k];
            if (g == 0) {
                double v0[CH][K];
#pragma unroll
                for (int a = 0; a < CH; ++a)
#pragma unroll
                    for (int k = 0; k < K; ++k) v0[a][k] = v0_lds[a * K + k];
                mat_acc<K, CH>(pwG + K * K, v0, ws);
            }
            if constexpr (kTagged) publish(Uf, g, ws);
            else if (lane == 0) {
#pragma unroll
                for (int a = 0; a < CH; ++a)
#pragma unroll
                    for (int k = 0; k < K; ++k) __hip_atomic_store(Tf + (long long)g * N + a * K + k, ws[a][k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
    SOS_MARK(4);
    // (the samples wait in the wavefront's slice, where the loads put them, while the group's start state is formed)
    // (totals without tags: the flag follows the total once that is acknowledged)
    if (!kTagged && wv == kWaves - 1 && g + 1 < ngroups) {
        asm volatile("s_waitcnt vmcnt(0)" : : : "memory");
        if (lane == 0) __hip_atomic_store(Ff + g, L.epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    SOS_MARK(5);
    // this lane's M^lane, for the offset of its chunk inside the wavefront: asked for ahead of the wait where the registers allow it
    // (the two-wavefront shape of short calls, which are pure latency chains), behind it otherwise (three workgroups per CU: 168 registers)
    double Ml[K][K];
    if constexpr (kAhead) {
#pragma unroll
        for (int r = 0; r < K; ++r)
#pragma unroll
            for (int q = 0; q < K; ++q) Ml[r][q] = L.pwT[(r * K + q) * kWave + lane];
    }
    double sg[CH][K];
    const bool near = MEET || (kTagged && L.look > 0);           // (uniform)
    if constexpr (MEET) {
#pragma unroll
        for (int a = 0; a < CH; ++a)
#pragma unroll
            for (int k = 0; k < K; ++k) sg[a][k] = 0.0;
    } else if (near) group_start_near<K, CH>(L, Uf, g, pwG, sg, s_fail);
    else {
        double acc[CH][K];
        group_start<K, CH, W, kTagged>(L, Tf, Ff, Uf, g, pwG, pwH, acc, s_fail);
        if (lane == 0) {
#pragma unroll
            for (int a = 0; a < CH; ++a)
#pragma unroll
                for (int k = 0; k < K; ++k) red[wv][a * K + k] = acc[a][k];
        }
    }
    if constexpr (!kAhead) {
#pragma unroll
        for (int r = 0; r < K; ++r)
#pragma unroll
            for (int q = 0; q < K; ++q) Ml[r][q] = L.pwT[(r * K + q) * kWave + lane];
    }
    if constexpr (!MEET) {
        __syncthreads();
        if (s_fail[0]) {
            if (tid == 0) __hip_atomic_store(L.status, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            return;
        }
    }
#pragma unroll
    for (int a = 0; a < CH; ++a)
#pragma unroll
        for (int k = 0; k < K; ++k) {
            double t = sg[a][k];
            if (!near) {
                t = red[0][a * K + k];
#pragma unroll
                for (int w = 1; w < kWaves; ++w) t += red[w][a * K + k];
            }
            sg[a][k] = g == 0 ? v0_lds[a * K + k] : t;
        }
    SOS_MARK(6);
    // ---- forward output pass: the chunk from its true start state M^lane ((M^64)^wv S_g + ws) + ex; the outputs replace the samples
    for (int w = 0; w < wv; ++w) mat_apply_t<K, CH>(tab, kM64, sg);
#pragma unroll
    for (int a = 0; a < CH; ++a)
#pragma unroll
        for (int k = 0; k < K; ++k) sg[a][k] += tab[kCarry + wv * N + a * K + k];
    if (active) {
        chunk_from_lds<CH>(lds, lane, xs);
#pragma unroll
        for (int r = 0; r < K; ++r)
#pragma unroll
            for (int q = 0; q < K; ++q) {
#pragma unroll
                for (int a = 0; a < CH; ++a) ex[a][r] += Ml[r][q] * sg[a][q];
            }
        SOS_MARK(13);
        double z[CH][NS][2];
#pragma unroll
        for (int a = 0; a < CH; ++a)
#pragma unroll
            for (int q = 0; q < NS; ++q) { z[a][q][0] = ex[a][2 * q]; z[a][q][1] = ex[a][2 * q + 1]; }
        if (len == kChunk) {
#pragma unroll
            for (int t = 0; t < kChunk; ++t)
#pragma unroll
                for (int a = 0; a < CH; ++a) xs[t].v[a] = sos_step_fma<NS>(c, z[a], xs[t].v[a]);
        } else {
#pragma unroll
            for (int t = 0; t < kChunk; ++t)
                if (t < len) {
#pragma unroll
                    for (int a = 0; a < CH; ++a) xs[t].v[a] = sos_step_fma<NS>(c, z[a], xs[t].v[a]);
                }
        }
    }
    SOS_MARK(7);
    // ---- backward chunk pass on the outputs, read from the chunk's end to its start (SosPass::mv).  Positions at and beyond m hold
    // y1[m - 1]: the thread that produced it shares it; all such chunks are in the last group.
    const long long last = p.m - 1;
    if (gb == 0) {
        if (i0 <= last && last < i0 + kChunk) {
            Smp<CH> cv = xs[0];
#pragma unroll
            for (int t = 1; t < kChunk; ++t) if (i0 + t == last) cv = xs[t];
#pragma unroll
            for (int a = 0; a < CH; ++a) c_lds[a] = cv.v[a];
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < kChunk; ++t)
            if (i0 + t > last) {
#pragma unroll
                for (int a = 0; a < CH; ++a) xs[t].v[a] = c_lds[a];
            }
        if (tid == 0) {
#pragma unroll
            for (int a = 0; a < CH; ++a)
#pragma unroll
                for (int k = 0; k < K; ++k) v0_lds[a * K + k] = zi[k] * c_lds[a];
        }
    }
    double exb[CH][K];
    {
        double sb[CH][K];
#pragma unroll
        for (int a = 0; a < CH; ++a)
#pragma unroll
            for (int k = 0; k < K; ++k) sb[a][k] = 0.0;
#pragma unroll
        for (int t = 0; t < kChunk; ++t)
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const double gk = kGGlobal ? G[k * kChunk + t] : tab[kG + k * kChunk + t];
#pragma unroll
                for (int a = 0; a < CH; ++a) sb[a][k] = fma(gk, xs[kChunk - 1 - t].v[a], sb[a][k]);
            }
        if constexpr (kRowScan) wave_scan_rows<K, CH, true>(sb, tab, Mrow);
        else wave_scan_t<K, CH, true>(sb, tab);
#pragma unroll
        for (int a = 0; a < CH; ++a)
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const double prev = kRowScan ? dpp_shift<0x130>(sb[a][k]) : __shfl_down(sb[a][k], 1, kWave);      // (wave_shl:1)
                exb[a][k] = lane != kWave - 1 ? prev : 0.0;
                if (lane == 0) tab[kTot + wv * N + a * K + k] = sb[a][k];
            }
        __syncthreads();                      // (also: v0_lds of the backward pass staged, every wavefront past its use of the forward carries)
        SOS_MARK(8);
        // backward order of the wavefronts: the last one comes first
        double wsb[CH][K];
#pragma unroll
        for (int a = 0; a < CH; ++a)
#pragma unroll
            for (int k = 0; k < K; ++k) wsb[a][k] = 0.0;
        for (int b = 0; b < kWaves - 1 - wv; ++b) {
            mat_apply_t<K, CH>(tab, kM64, wsb);
#pragma unroll
            for (int a = 0; a < CH; ++a)
#pragma unroll
                for (int k = 0; k < K; ++k) wsb[a][k] += tab[kTot + (kWaves - 1 - b) * N + a * K + k];
        }
        if (lane == 0) {
#pragma unroll
            for (int a = 0; a < CH; ++a)
#pragma unroll
                for (int k = 0; k < K; ++k) tab[kCarry + wv * N + a * K + k] = wsb[a][k];
        }
        if (wv == 0 && gb + 1 < ngroups) {
            mat_apply_t<K, CH>(tab, kM64, wsb);
#pragma unroll
            for (int a = 0; a < CH; ++a)
#pragma unroll
                for (int k = 0; k < K; ++k) wsb[a][k] += tab[kTot + a * K + k];
            if (gb == 0) {
                double v0[CH][K];
#pragma unroll
                for (int a = 0; a < CH; ++a)
#pragma unroll
                    for (int k = 0; k < K; ++k) v0[a][k] = v0_lds[a * K + k];
                mat_acc<K, CH>(pwG + K * K, v0, wsb);
            }
            if constexpr (kTagged) publish(Ubk, gb, wsb);
            else if (lane == 0) {
#pragma unroll
                for (int a = 0; a < CH; ++a)
#pragma unroll
                    for (int k = 0; k < K; ++k) __hip_atomic_store(Tbk + (long long)gb * N + a * K + k, wsb[a][k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
#pragma unroll
    for (int t = 0; t < kChunk; ++t) lds[lane * (kChunk + 1) + t] = xs[t];
    wave_lds_sync();
    if (!kTagged && wv == 0 && gb + 1 < ngroups) {
        asm volatile("s_waitcnt vmcnt(0)" : : : "memory");
        if (lane == 0) __hip_atomic_store(Fbk + gb, L.epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    SOS_MARK(9);
    // this lane's power for the offset of its chunk inside the wavefront: its backward position there is 63 - lane
    double Mb[K][K];
    if constexpr (kAhead) {
#pragma unroll
        for (int r = 0; r < K; ++r)
#pragma unroll
            for (int q = 0; q < K; ++q) Mb[r][q] = L.pwT[(r * K + q) * kWave + (kWave - 1 - lane)];
    }
    double sgb[CH][K];
    double sdl[CH][K];                                           // MEET: the group's true forward start state (zero for group 0, which had it all along)
    double Vr[MEET ? K : 1][MEET ? K : 1], Mlr[MEET ? K : 1][MEET ? K : 1];
    if constexpr (MEET) {
        // this thread's maps, asked for ahead of the wait: Vm, M^lane once more, M^(63 - lane)
        const double* Vm = L.meetV + (long long)(gb == 0 ? K * K : 0) * kGroup + tid;
#pragma unroll
        for (int r = 0; r < K; ++r)
#pragma unroll
            for (int q = 0; q < K; ++q) {
                Vr[r][q] = Vm[(r * K + q) * kGroup];
                Mlr[r][q] = q / 2 > r / 2 ? 0.0 : L.pwT[(r * K + q) * kWave + lane];
                if constexpr (!kAhead) Mb[r][q] = L.pwT[(r * K + q) * kWave + (kWave - 1 - lane)];
            }
        const long long f_unit0 = (long long)row * ngroups * N, b_unit0 = ((long long)gridDim.x + (long long)row * ngroups) * N;
        if (!meet_states<K, CH>(L, f_unit0, b_unit0, g, gb, ngroups, pwG, sdl, sgb)) {
            if (lane == 0) __hip_atomic_store(L.status, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            return;
        }
    } else if (near) group_start_near<K, CH>(L, Ubk, gb, pwG, sgb, s_fail);
    else {
        double acc[CH][K];
        group_start<K, CH, W, kTagged>(L, Tbk, Fbk, Ubk, gb, pwG, pwH, acc, s_fail);
        if (lane == 0) {
#pragma unroll
            for (int a = 0; a < CH; ++a)
#pragma unroll
                for (int k = 0; k < K; ++k) red[wv][a * K + k] = acc[a][k];
        }
    }
    if constexpr (!kAhead && !MEET) {
#pragma unroll
        for (int r = 0; r < K; ++r)
#pragma unroll
            for (int q = 0; q < K; ++q) Mb[r][q] = L.pwT[(r * K + q) * kWave + (kWave - 1 - lane)];
    }
    if constexpr (!MEET) {
        __syncthreads();
        if (s_fail[0]) {
            if (tid == 0) __hip_atomic_store(L.status, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            return;
        }
    }
#pragma unroll
    for (int a = 0; a < CH; ++a)
#pragma unroll
        for (int k = 0; k < K; ++k) {
            double t = sgb[a][k];
            if (!near) {
                t = red[0][a * K + k];
#pragma unroll
                for (int w = 1; w < kWaves; ++w) t += red[w][a * K + k];
            }
            sgb[a][k] = gb == 0 ? v0_lds[a * K + k] : t;
        }
    SOS_MARK(10);
    // ---- backward output pass: the chunk from its end, start state M^(63 - lane) ((M^64)^(W - 1 - wv) S_gb + wsb) + exb
    for (int w = 0; w < kWaves - 1 - wv; ++w) mat_apply_t<K, CH>(tab, kM64, sgb);
#pragma unroll
    for (int a = 0; a < CH; ++a)
#pragma unroll
        for (int k = 0; k < K; ++k) sgb[a][k] += tab[kCarry + wv * N + a * K + k];
    if constexpr (!MEET) chunk_from_lds<CH>(lds, lane, xs);
#pragma unroll
    for (int r = 0; r < K; ++r)
#pragma unroll
        for (int q = 0; q < K; ++q) {
#pragma unroll
            for (int a = 0; a < CH; ++a) exb[a][r] += Mb[r][q] * sgb[a][q];
        }
    if constexpr (MEET) {
        // what the group's true forward start state adds: to the backward state at the start of this chunk (through the outputs of the chunks behind it) ...
#pragma unroll
        for (int r = 0; r < K; ++r)
#pragma unroll
            for (int q = 0; q < K; ++q) {
#pragma unroll
                for (int a = 0; a < CH; ++a) exb[a][r] += Vr[r][q] * sdl[a][q];
            }
        // ... and to this chunk's own forward outputs: the zero-input response from M^lane (M^64)^wv S_g
        for (int w = 0; w < wv; ++w) mat_apply_t<K, CH>(tab, kM64, sdl);
        double z[CH][NS][2];
#pragma unroll
        for (int a = 0; a < CH; ++a)
#pragma unroll
            for (int q = 0; q < NS; ++q) { z[a][q][0] = 0.0; z[a][q][1] = 0.0; }
#pragma unroll
        for (int r = 0; r < K; ++r)
#pragma unroll
            for (int q = 0; q < K; ++q) {
                if (q / 2 > r / 2) continue;
#pragma unroll
                for (int a = 0; a < CH; ++a) z[a][r / 2][r % 2] += Mlr[r][q] * sdl[a][q];
            }
        chunk_from_lds<CH>(lds, lane, xs);                        // (y0; only now: the maps above are dead)
        if (active) {
#pragma unroll
            for (int t = 0; t < kChunk; ++t)
                if (len == kChunk || t < len) {
#pragma unroll
                    for (int a = 0; a < CH; ++a) xs[t].v[a] += sos_step_fma<NS>(c, z[a], 0.0);
                }
        }
        if (gb == 0 && i0 <= last) {                              // the virtual copies behind the row's last output follow it
            Smp<CH> cv = xs[0];
#pragma unroll
            for (int t = 1; t < kChunk; ++t) if (i0 + t == last) cv = xs[t];
#pragma unroll
            for (int t = 0; t < kChunk; ++t)
                if (i0 + t > last) xs[t] = cv;
        }
    }
    {
        double z[CH][NS][2];
#pragma unroll
        for (int a = 0; a < CH; ++a)
#pragma unroll
            for (int q = 0; q < NS; ++q) { z[a][q][0] = exb[a][2 * q]; z[a][q][1] = exb[a][2 * q + 1]; }
#pragma unroll
        for (int t = kChunk - 1; t >= 0; --t) {
#pragma unroll
            for (int a = 0; a < CH; ++a) xs[t].v[a] = sos_step_fma<NS>(c, z[a], xs[t].v[a]);
            lds[lane * (kChunk + 1) + t] = xs[t];
        }
    }
    wave_lds_sync();
    SOS_MARK(11);
    // the result sits where the sample was: padded position k -> out[k - edge]
    double* const dst = out + (long long)row * p.n * CH;
#pragma unroll
    for (int t = 0; t < kChunk; ++t) {
        const Smp<CH> y = lds[lds_pos(t * kWave + lane)];
        const long long nn = w0 + t * kWave + lane - p.edge;
        if (nn >= 0 && nn < p.n) st<CH>(dst, nn, y);
    }
    SOS_MARK(12);
}


// ------------------------------------------------------------------------------------------ host glue
// What has to name a kernel instance of this chunk length; everything else of the host side is sos_filter.hip (its driver takes `Instances` as a parameter).
struct Instances {
    static constexpr int chunk = kChunk;
    using Link = SosLink;

    // Workgroups of k_filtfilt the device holds at once.  The runtime's occupancy answer is cut to what the LDS allows with the 512-byte
    // allocation granule and the 161 280 usable bytes measured on gfx950 (three workgroups of 53 760 B fit a CU, three of 54 272 B do not:
    // profiles/r03_sosfilt.txt) -- a grid that waits for workgroups that cannot start would only end by its patience.
    template <int NS, int CH, int W, bool MEET = false> static long long one_launch_capacity() {
        static long long cap = -1;                                  // (calls are serialised by Workspace::mu)
        if (cap >= 0) return cap;
        int per_cu = 0, cus = 0, dev = 0;
        hipFuncAttributes fa;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
            hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_filtfilt<NS, CH, W, MEET>, kWave * W, 0) != hipSuccess ||
            hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(k_filtfilt<NS, CH, W, MEET>)) != hipSuccess) {
            (void)hipGetLastError();
            return cap = 0;
        }
        const long long lds = ((long long)fa.sharedSizeBytes + 511) / 512 * 512;
        const long long by_lds = lds > 0 ? 161280 / lds : per_cu;
        return cap = (long long)cus * (per_cu < by_lds ? per_cu : by_lds);
    }

    // the one launch; `tab`: the filter's device table (sos_tables.hpp TableLayout); p.src / p.mv set by the caller
    template <int NS, int CH, int W>
    static void launch_one(bool meet, dim3 grid, hipStream_t stream, const SosCoefs& c, const SosPass& p, int nchunks, int ngroups, const double* tab, double* d_res, const SosLink& L) {
        using Lay = ssfm::sos::TableLayout<NS, kChunk>;
        const dim3 block(kWave * W);
        const double *d_zi = tab + Lay::zi, *d_pw = tab + Lay::pw, *d_pwG = tab + Lay::pwG, *d_pwH = tab + Lay::pwH, *d_G = tab + Lay::G;
        if constexpr (CH * 2 * NS <= 8) {
            if (meet) hipLaunchKernelGGL((k_filtfilt<NS, CH, W, true>), grid, block, 0, stream, c, p, nchunks, ngroups, d_zi, d_pw, d_pwG, d_pwH, d_G, d_res, L);
        }
        if (!meet) hipLaunchKernelGGL((k_filtfilt<NS, CH, W>), grid, block, 0, stream, c, p, nchunks, ngroups, d_zi, d_pw, d_pwG, d_pwH, d_G, d_res, L);
    }

    // Three launches per call: chunk pass (forward), output pass (forward) + chunk pass (backward) in one kernel, output pass (backward).
    // d_T: the totals of the forward pass, behind them those of the backward pass; d_E2: E of the backward pass (written by the forward output kernel).
    template <int NS, int CH, int W>
    static void launch_three(dim3 grid, hipStream_t stream, const SosCoefs& c, SosPass p, int nchunks, int ngroups, int rows, const double* tab, const double* d_x, double* d_y1, double* d_E, double* d_T, double* d_E2, double* d_out) {
        using Lay = ssfm::sos::TableLayout<NS, kChunk>;
        constexpr int K = 2 * NS, kGroup = kWave * W;
        const dim3 block(kGroup);
        const double *d_zi = tab + Lay::zi, *d_pw = tab + Lay::pw, *d_pwG = tab + Lay::pwG, *d_pwH = tab + Lay::pwH, *d_G = tab + Lay::G;
        double* d_T2 = d_T + (size_t)ngroups * rows * CH * K;
        p.backward = 0; p.src = d_x; p.mv = p.m;
        hipLaunchKernelGGL((k_chunk_scan<NS, CH, W>), grid, block, 0, stream, p, nchunks, ngroups, d_pw, d_G, d_E, d_T);
        hipLaunchKernelGGL((k_apply<NS, CH, W>), grid, block, 0, stream, c, p, nchunks, ngroups, d_zi, d_pw, d_pwG, d_pwH, (const double*)d_E,
                           (const double*)d_T, d_y1, d_out, d_G, d_E2, d_T2);
        p.backward = 1; p.src = d_y1; p.mv = (long long)ngroups * kGroup * kChunk;
        hipLaunchKernelGGL((k_apply<NS, CH, W>), grid, block, 0, stream, c, p, ngroups * kGroup, ngroups, d_zi, d_pw, d_pwG, d_pwH, (const double*)d_E2,
                           (const double*)d_T2, d_y1, d_out, d_G, (double*)nullptr, (double*)nullptr);
    }
};
