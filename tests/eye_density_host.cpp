// The integer rules of csrc/eye_density.inc -- the text the kernels of eye_density.hip compile -- checked on the host against brute force, under
// AddressSanitizer and UBSan (tests/test_eye_density_cpu.py builds and runs this program): the bin of a value among linspace edges, SciPy's
// reflected index, the trace geometry and the grid index of a plotted point.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "eye_density.inc"

static long long g_checks = 0;
#define CHECK(cond, ...)                                                  \
    do {                                                                  \
        ++g_checks;                                                       \
        if (!(cond)) { std::printf("FAILED: " __VA_ARGS__); std::printf("\n"); std::exit(1); } \
    } while (0)

// numpy.linspace(lo, hi, B + 1): arange * step + lo, the last one set to hi
static std::vector<double> linspace_edges(double lo, double hi, int B) {
    std::vector<double> e(B + 1);                                  // exactly B + 1 doubles: a read of E[B + 1] is the sanitizer's
    const double step = (hi - lo) / B;
    for (int k = 0; k <= B; ++k) e[k] = k * step + lo;
    e[B] = hi;
    return e;
}
// searchsorted(side='right') by a linear scan, minus one, the last edge in the last bin; -1 / B -> -1 (an outlier)
static int brute_bin(const std::vector<double>& e, int B, double v) {
    int idx = 0;
    while (idx <= B && !(v < e[idx])) ++idx;                       // the first edge greater than v
    if (v == e[B]) --idx;
    return idx >= 1 && idx <= B ? idx - 1 : -1;
}

static void check_bins() {
    const int Bs[] = {1, 2, 7, 8, 200, 350};
    const double ranges[][2] = {{0.0, 1.0}, {-0.3, 1.7}, {-1e-3, 1e-3}, {1.0, 1.0 + 1e-9}, {-1.5e300, 1.5e300}, {-0.5, 0.5}, {1e300, 1.0000001e300}};
    for (int B : Bs)
        for (auto& r : ranges) {
            const std::vector<double> e = linspace_edges(r[0], r[1], B);
            for (int k = 0; k <= B; ++k)
                for (double v : {e[k], std::nextafter(e[k], -INFINITY), std::nextafter(e[k], INFINITY), k < B ? 0.5 * e[k] + 0.5 * e[k + 1] : e[k]}) {
                    if (v < r[0] || v > r[1]) continue;               // the range is the data's own minimum and maximum
                    const int got = eye_bin(e.data(), B, v), want = brute_bin(e, B, v);
                    CHECK(got == want, "eye_bin B=%d range [%g, %g] v=%.17g: %d, brute force %d", B, r[0], r[1], v, got, want);
                    if (k > 0 && k < B && v == e[k] && e[k] > e[k - 1]) CHECK(got >= k, "an interior edge value falls left of its edge: B=%d k=%d", B, k);
                }
            CHECK(eye_bin(e.data(), B, r[1]) == B - 1, "the last edge is not in the last bin: B=%d", B);
        }
    // an edge that is not finite (a range that overflows, one bin): only the maximum is counted
    const double big = 1.7e308, nan = std::numeric_limits<double>::quiet_NaN();
    const std::vector<double> e{nan, big};
    CHECK(eye_bin(e.data(), 1, big) == 0 && eye_bin(e.data(), 1, -big) == -1 && eye_bin(e.data(), 1, 0.0) == -1, "the bins of [nan, max]");
}

static void check_reflect() {
    for (int B : {1, 2, 7, 8, 200, 350})
        for (int r : {0, 1, 2, 12, 20, 2 * B, 2 * B + 1, 5 * B + 3}) {
            // brute force: the line written out, then its mirror image appended on either side again and again (d c b a | a b c d | d c b a)
            std::vector<int> ext(2 * r + B);
            for (int i = 0; i < B; ++i) ext[r + i] = i;
            for (int i = 1, pos = 0, dir = 1; i <= r; ++i) {          // leftwards: a b c d, then d c b a, ...
                ext[r - i] = pos;
                if (pos + dir < 0 || pos + dir >= B) dir = -dir; else pos += dir;
            }
            for (int i = 1, pos = B - 1, dir = -1; i <= r; ++i) {     // rightwards: d c b a, then a b c d, ...
                ext[r + B - 1 + i] = pos;
                if (pos + dir < 0 || pos + dir >= B) dir = -dir; else pos += dir;
            }
            for (int i = -r; i < B + r; ++i) {
                const int got = eye_reflect(i, B);
                CHECK(got >= 0 && got < B && got == ext[r + i], "eye_reflect(%d, %d) = %d, brute force %d", i, B, got, ext[r + i]);
            }
        }
}

static void check_geometry() {
    for (long long sps : {1, 2, 3, 16, 64})
        for (long long n = 0; n <= 6 * sps + 5; ++n)
            for (long long nt : {-1LL, 0LL, 1LL, 2LL, 3LL, 1000LL}) {
                const EyeGeometry g = eye_geometry(n, sps, nt);
                // brute force: the plotted samples are sps / 2 ... n - sps / 2 - 1, whole traces of 2 sps of them
                long long left = 0;
                for (long long i = 0; i < n; ++i) left += i >= sps / 2 && i < n - sps / 2;
                int err = 0;
                long long T = 0;
                if (left <= 0) err = 1;
                else if (left < 2 * sps) err = 2;
                else {
                    while ((T + 1) * 2 * sps <= left) ++T;
                    if (nt >= 0 && nt < T) T = nt;
                    if (T == 0) err = 3;
                }
                CHECK(g.err == err, "eye_geometry(%lld, %lld, %lld).err = %d, brute force %d", n, sps, nt, g.err, err);
                if (!err) {
                    CHECK(g.T == T && g.P == 2 * sps && g.start == sps / 2, "eye_geometry(%lld, %lld, %lld): T = %lld, brute force %lld", n, sps, nt, g.T, T);
                    CHECK(g.start + g.T * g.P <= n - sps / 2, "the last plotted sample lies beyond the cut");
                }
            }
}

static void check_grid_index() {
    for (int B : {1, 2, 7, 8, 200, 350})
        for (auto& r : {std::pair<double, double>{0.0, 1.0}, {-0.3, 1.7}, {2.0, 2.0}, {-1.7e308, 1.7e308}}) {
            for (int k = 0; k <= 1000; ++k) {
                const double v = r.first + (r.second - r.first) * (k / 1000.0);
                const int got = eye_grid_index(v, r.first, r.second, B);
                CHECK(got >= 0 && got < B, "eye_grid_index(%g, %g, %g, %d) = %d", v, r.first, r.second, B, got);
                if (std::isfinite(r.second - r.first) && r.second > r.first) {
                    const double t = (v - r.first) / (r.second - r.first) * (B - 1);
                    long long want = (long long)t;
                    want = want < 0 ? 0 : (want > B - 1 ? B - 1 : want);
                    CHECK(got == want, "eye_grid_index(%g, %g, %g, %d) = %d, expected %lld", v, r.first, r.second, B, got, want);
                } else {
                    CHECK(got == 0, "a zero or overflowing range gives index 0, got %d", got);
                }
            }
        }
    CHECK(eye_grid_index(std::numeric_limits<double>::quiet_NaN(), 0.0, 1.0, 8) == 0, "a NaN converts to index 0");
}

int main() {
    check_bins();
    check_reflect();
    check_geometry();
    check_grid_index();
    std::printf("ok: %lld checks\n", g_checks);
    return 0;
}
