// sos_tables.hpp -- the tables the SOS filter's kernels read (sos_filter.hip, sos_filter_impl.inc), built on the host once per filter, and where each part lies.
// Host-only plain C++, templated on <sections, wavefronts per workgroup, chunk length>; held bit for bit to the builder it replaces by tests/sos_route_host.cpp.
// `Coefs`: any struct with the arrays b0, b1, b2, a1, a2 (sos_route.hpp).
#pragma once
#include <cstddef>
#include <cstring>
#include <vector>

#include "sos_route.hpp"

namespace ssfm {
namespace sos {

// The device table of one filter and shape, in doubles: three levels of powers [65][K * K] -- pw[j] = M^j with M = A^CHUNK the map over one chunk, pwG[j] = (M^(64 W))^j
// (one group of W x 64 chunks), pwH[j] = (M^(64 W))^(64 j) (64 groups) --, G, zi, and pw / pwG once more element-major, [K * K][64] (SosLink::pwT, pwGT).
template <int NS, int CHUNK> struct TableLayout {
    static constexpr size_t K = 2 * NS, kLevel = (size_t)(kWave + 1) * K * K;
    static constexpr size_t pw = 0, pwG = kLevel, pwH = 2 * kLevel, G = 3 * kLevel, zi = G + K * CHUNK, pwT = zi + K, pwGT = pwT + K * K * kWave, total = pwGT + K * K * kWave;
};
// The single-meeting kernels' maps: Vm [2][K * K][threads], then Wm [2][K * K]
template <int NS, int W> struct MeetLayout {
    static constexpr size_t K = 2 * NS, kGroup = (size_t)kWave * W;
    static constexpr size_t Vm = 0, Wm = 2 * K * K * kGroup, total = Wm + 2 * K * K;
};

template <int K> void matmul(const double* A, const double* B, double* C) {
    for (int r = 0; r < K; ++r)
        for (int q = 0; q < K; ++q) {
            double acc = 0.0;
            for (int m2 = 0; m2 < K; ++m2) acc += A[r * K + m2] * B[m2 * K + q];
            C[r * K + q] = acc;
        }
}

// one sample through the cascade (direct form II transposed), in SciPy's operation order
template <int NS, class Coefs> double cascade_step(const Coefs& c, double (&z)[NS][2], double x) {
    for (int s = 0; s < NS; ++s) {
        const double xn = x;
        x = c.b0[s] * xn + z[s][0];
        z[s][0] = c.b1[s] * xn - c.a1[s] * x + z[s][1];
        z[s][1] = c.b2[s] * xn - c.a2[s] * x;
    }
    return x;
}

template <int NS, int W, int CHUNK, class Coefs> void build_tables(const Coefs& c, const double* zi, std::vector<double>& tab) {
    constexpr int K = 2 * NS;
    using Lay = TableLayout<NS, CHUNK>;
    tab.assign(Lay::total, 0.0);
    double M[K * K];
    // column q of A^CHUNK = state after CHUNK zero-input steps from the unit state e_q
    for (int q = 0; q < K; ++q) {
        double z[NS][2];
        for (int s = 0; s < NS; ++s) z[s][0] = z[s][1] = 0.0;
        z[q / 2][q % 2] = 1.0;
        for (int i = 0; i < CHUNK; ++i) (void)cascade_step<NS>(c, z, 0.0);
        for (int r = 0; r < K; ++r) M[r * K + q] = z[r / 2][r % 2];
    }
    // G[k][t]: component k of the state at the end of a chunk whose only non-zero sample is a 1 at position t
    double* G = tab.data() + Lay::G;
    for (int t = 0; t < CHUNK; ++t) {
        double z[NS][2];
        for (int s = 0; s < NS; ++s) z[s][0] = z[s][1] = 0.0;
        for (int i = t; i < CHUNK; ++i) (void)cascade_step<NS>(c, z, i == t ? 1.0 : 0.0);
        for (int k = 0; k < K; ++k) G[(size_t)k * CHUNK + t] = z[k / 2][k % 2];
    }
    for (int level = 0; level < 3; ++level) {
        double* P = tab.data() + (size_t)level * Lay::kLevel;
        for (int r = 0; r < K; ++r) P[r * K + r] = 1.0;
        for (int j = 0; j < kWave; ++j) matmul<K>(M, P + (size_t)j * K * K, P + (size_t)(j + 1) * K * K);
        std::memcpy(M, P + (size_t)kWave * K * K, sizeof(M));                 // M^64 of this level
        if (level == 0) {                                                     // group map = (M^64)^W
            double A[K * K], B[K * K];
            std::memcpy(A, M, sizeof(M));
            for (int w = 1; w < W; ++w) { matmul<K>(M, A, B); std::memcpy(A, B, sizeof(A)); }
            std::memcpy(M, A, sizeof(M));
        }
    }
    std::memcpy(tab.data() + Lay::zi, zi, sizeof(double) * K);
    for (int level = 0; level < 2; ++level) {                                 // pw and pwG element-major
        const double* P = tab.data() + (size_t)level * Lay::kLevel;
        double* T = tab.data() + (level ? Lay::pwGT : Lay::pwT);
        for (int e = 0; e < K * K; ++e)
            for (int j = 0; j < kWave; ++j) T[(size_t)e * kWave + j] = P[(size_t)j * K * K + e];
    }
}

// The single-meeting kernels' maps (meet_states): what a unit start state e_q of a GROUP adds, through the group's forward outputs, to the backward state at the
// start of every chunk of the group (Vm, element-major over the threads) and at the group's end (Wm).  [0]: a whole group; [1]: the row's last group, whose
// sequence ends at position `jl` of the group -- behind it the virtual copies of that output, and the backward pass starts from zi * that output.
template <int NS, int W, int CHUNK, class Coefs> void build_meet_tables(const Coefs& c, const double* zi, long long jl, std::vector<double>& out) {
    constexpr int K = 2 * NS, kGroup = kWave * W;
    constexpr long long Lg = (long long)kGroup * CHUNK;
    using Lay = MeetLayout<NS, W>;
    out.assign(Lay::total, 0.0);
    std::vector<double> dy((size_t)Lg);
    for (int variant = 0; variant < 2; ++variant) {
        double* Vm = out.data() + Lay::Vm + (size_t)variant * K * K * kGroup;
        double* Wm = out.data() + Lay::Wm + (size_t)variant * K * K;
        const long long end = variant ? jl : Lg - 1;
        for (int q = 0; q < K; ++q) {
            double z[NS][2];
            for (int s = 0; s < NS; ++s) z[s][0] = z[s][1] = 0.0;
            z[q / 2][q % 2] = 1.0;
            for (long long j = 0; j <= end; ++j) dy[(size_t)j] = cascade_step<NS>(c, z, 0.0);
            for (long long j = end + 1; j < Lg; ++j) dy[(size_t)j] = dy[(size_t)end];
            double zb[NS][2];
            for (int s = 0; s < NS; ++s) { zb[s][0] = variant ? zi[2 * s] * dy[(size_t)end] : 0.0; zb[s][1] = variant ? zi[2 * s + 1] * dy[(size_t)end] : 0.0; }
            for (int pos = kGroup - 1; pos >= 0; --pos) {
                for (int r = 0; r < K; ++r) Vm[(size_t)(r * K + q) * kGroup + pos] = zb[r / 2][r % 2];
                for (int t = CHUNK - 1; t >= 0; --t) (void)cascade_step<NS>(c, zb, dy[(size_t)pos * CHUNK + t]);
            }
            for (int r = 0; r < K; ++r) Wm[r * K + q] = zb[r / 2][r % 2];
        }
    }
}

}  // namespace sos
}  // namespace ssfm
