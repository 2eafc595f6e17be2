// eye_density.inc -- the three integer rules of the eye diagram's density (eye_density.hip), in plain C++ so that a host program compiles the very
// text the kernels use (tests/eye_density_host.cpp): the trace geometry, the bin of a value among NumPy's edges, SciPy's reflected index and
// the grid index of a plotted point.  Included after EYE_HD is defined (`__host__ __device__` under hipcc, nothing on the host).
#ifndef EYE_HD
#define EYE_HD
#endif

// The traces of an n-sample record (reference utils.py:1651-1673): sps / 2 samples are cut from both ends, a trace is P = 2 sps points, T traces are
// drawn: point j < T P is sample start + j.  err: 1 the record is too short for the cut, 2 fewer than P points are left, 3 no trace to draw.
struct EyeGeometry {
    long long start, points, P, available, T;
    int err;
};
EYE_HD inline EyeGeometry eye_geometry(long long n, long long sps, long long n_traces /* < 0: every available trace */) {
    EyeGeometry g{sps / 2, 0, 2 * sps, 0, 0, 0};
    const long long end = n - sps / 2;
    if (g.start >= end) { g.err = 1; return g; }
    g.points = end - g.start;
    if (g.points < g.P) { g.err = 2; return g; }
    g.available = g.points / g.P;
    g.T = n_traces < 0 || n_traces > g.available ? g.available : n_traces;
    if (g.T == 0) g.err = 3;
    return g;
}

// The bin of v among the B + 1 edges E of numpy.histogramdd: searchsorted(E, v, side='right') - 1, a value equal to the last edge in the last bin;
// -1 for a value no bin holds (an outlier, which NumPy drops: only with an edge that is not finite).  The guess is arithmetic, the decision is made
// by comparisons with E[b] and E[b + 1] alone.
EYE_HD inline int eye_bin(const double* E, int B, double v) {
    const double t = (v - E[0]) / (E[B] - E[0]) * (double)B;
    int b = t >= 0.0 ? (t < (double)(B - 1) ? (int)t : B - 1) : 0;          // (a NaN guess is bin 0)
    while (b > 0 && v < E[b]) --b;
    while (b < B - 1 && v >= E[b + 1]) ++b;
    if (v >= E[b] && v < E[b + 1]) return b;
    return b == B - 1 && v == E[B] ? b : -1;
}

// scipy.ndimage's mode='reflect' (d c b a | a b c d | d c b a), continued periodically: the index in [0, B) that position i of the extended line reads.
EYE_HD inline int eye_reflect(long long i, int B) {
    const long long period = 2LL * B;
    long long m = i % period;
    if (m < 0) m += period;
    return (int)(m < B ? m : period - 1 - m);
}

// The grid index of a plotted value (reference utils.py:1705-1715): clip(int((v - lo) / (hi - lo) * (B - 1)), 0, B - 1), 0 when hi == lo.  IEEE
// subtraction, division and multiplication, truncation toward zero; a product that is NaN or beyond int64 converts as NumPy's cast does on x86-64
// (the most negative integer), which the clip turns into 0.
EYE_HD inline int eye_grid_index(double v, double lo, double hi, int B) {
    const double vn = hi == lo ? 0.0 : (v - lo) / (hi - lo);
    const double t = vn * (double)(B - 1);
    if (!(t > -9.2e18 && t < 9.2e18)) return 0;
    const long long k = (long long)t;
    return (int)(k < 0 ? 0 : (k > B - 1 ? B - 1 : k));
}

// A general fold of the record: point j < count is sample start + j at phase j mod P; the first n_draw L points are drawn, as n_draw traces of L
// points (values and indices come back for those; L = P without resampling).  count need not be a multiple of P or of L.  eye.plot's fold
// (reference typing.py:2718-2764; formed by utils._eye_plot_fold) is start = sps, count = n - sps, P = 2 (sps_resamp or sps), L = 2 sps,
// n_draw = count / L; the geometry above is start = sps / 2, count = T P, L = P, n_draw = T.
struct EyeFold {
    long long start, count, P, L, n_draw;
    int err;
};
// a fold the caller states: 0 when it lies within an n-sample record and its drawn points within its points
EYE_HD inline int eye_fold_check(const EyeFold& f, long long n) {
    if (f.start < 0 || f.count < 1 || f.start > n - f.count) return 1;
    if (f.P < 1 || f.L < 1 || f.n_draw < 0 || f.n_draw > f.count / f.L) return 2;
    return 0;
}
EYE_HD inline long long eye_fold_sample(const EyeFold& f, long long j) { return f.start + j; }
EYE_HD inline int eye_fold_phase(const EyeFold& f, long long j) { return (int)(j % f.P); }
EYE_HD inline bool eye_fold_drawn(const EyeFold& f, long long j) { return j < f.n_draw * f.L; }
// whether point j enters the side histogram: its phase passes the mask (P bytes); a NULL mask passes every point
EYE_HD inline bool eye_fold_masked(const EyeFold& f, const unsigned char* mask, long long j) { return !mask || mask[j % f.P] != 0; }
