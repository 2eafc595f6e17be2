// The fold rules of csrc/eye_density.inc that the kernels of eye_density.hip call -- which sample and phase a point has (k_counts, k_colour_gather,
// k_fold_minmax, k_hist_masked), whether it is drawn (k_colour_gather), whether it passes the phase mask, and the check of a stated fold -- on the
// host against brute force, under AddressSanitizer and UBSan (tests/test_eye_plot_cpu.py builds and runs this program).  The fold is the one
// utils._eye_plot_fold hands the entry points (plot_fold below states it again); the brute force is the reference's own construction
// (typing.py:2718-2764): the rolled and cut record, the tiled time grid cut by sps, the rows of the reshaped traces.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "eye_density.inc"

static long long g_checks = 0;
#define CHECK(cond, ...)                                                  \
    do {                                                                  \
        ++g_checks;                                                       \
        if (!(cond)) { std::printf("FAILED: " __VA_ARGS__); std::printf("\n"); std::exit(1); } \
    } while (0)

// Python's floor division
static long long floordiv(long long a, long long b) { return a / b - ((a % b != 0) && ((a < 0) != (b < 0))); }

// eye.plot's fold as opticomlib_amd/utils.py `_eye_plot_fold` forms it
static EyeFold plot_fold(long long n, long long sps, long long s) {
    EyeFold f{sps, n - sps, 2 * s, 2 * sps, 0, 0};
    if (f.count < 1) { f.err = 1; return f; }
    f.n_draw = f.count / f.L;
    return f;
}

static void check_plot_fold() {
    for (long long sps : {1, 2, 3, 4, 5, 16})
        for (long long s : {sps, 2 * sps, 4 * sps, 3LL})
            for (long long n = 0; n <= 7 * sps + 2 * s + 3; ++n) {
                const EyeFold f = plot_fold(n, sps, s);
                // brute force: sample i of the record carries its own index; np.roll(y, -sps // 2)[sps // 2 : -sps // 2]
                std::vector<long long> rolled(n), y_, t_;
                const long long shift = n ? ((floordiv(-sps, 2) % n) + n) % n : 0;      // np.roll(y, k): out[(i + k) mod n] = y[i]
                for (long long i = 0; i < n; ++i) rolled[(i + shift) % n] = i;
                const long long a = sps / 2, b = n + floordiv(-sps, 2);               // the slice [sps // 2 : -sps // 2]
                for (long long i = a; i < b && i < n; ++i) y_.push_back(rolled[i]);
                for (long long i = 0; i < n - sps; ++i) t_.push_back(i % (2 * s));   // t[:-sps], t of period 2 s (phase numbers)
                if (n <= sps) { CHECK(f.err == 1, "plot_fold(%lld, %lld, %lld): no point is left, err = %d", n, sps, s, f.err); continue; }
                CHECK(!f.err && f.count == (long long)y_.size() && f.count == (long long)t_.size(), "plot_fold(%lld, %lld, %lld): count %lld, brute force %zu and %zu",
                      n, sps, s, f.count, y_.size(), t_.size());
                CHECK(eye_fold_check(f, n) == 0, "plot_fold(%lld, %lld, %lld) does not pass its own check", n, sps, s);
                const long long n_traces = (long long)y_.size() / (2 * sps);
                CHECK(f.n_draw == n_traces && f.L == 2 * sps && f.P == 2 * s, "plot_fold(%lld, %lld, %lld): n_draw %lld, brute force %lld", n, sps, s, f.n_draw, n_traces);
                std::vector<unsigned char> mask(f.P);                                  // exactly P bytes: a read beyond is the sanitizer's
                for (long long p = 0; p < f.P; ++p) mask[p] = (p * 7 + n) % 3 == 0;
                long long drawn = 0, masked = 0, brute_masked = 0;
                for (long long j = 0; j < f.count; ++j) {
                    CHECK(eye_fold_sample(f, j) == y_[j] && eye_fold_sample(f, j) < n, "point %lld of (%lld, %lld, %lld) is sample %lld, brute force %lld", j, n, sps, s,
                          eye_fold_sample(f, j), y_[j]);
                    CHECK(eye_fold_phase(f, j) == t_[j], "point %lld of (%lld, %lld, %lld) has phase %d, brute force %lld", j, n, sps, s, eye_fold_phase(f, j), t_[j]);
                    // y_[:n_traces 2 sps].reshape(-1, 2 sps): row j / (2 sps), column j mod (2 sps)
                    const bool in_rows = j < n_traces * 2 * sps;
                    CHECK(eye_fold_drawn(f, j) == in_rows, "point %lld of (%lld, %lld, %lld): drawn %d", j, n, sps, s, (int)eye_fold_drawn(f, j));
                    drawn += in_rows;
                    masked += eye_fold_masked(f, mask.data(), j);
                    brute_masked += mask[t_[j]];
                    CHECK(eye_fold_masked(f, nullptr, j), "no mask passes every point");
                }
                CHECK(drawn == n_traces * 2 * sps && masked == brute_masked, "(%lld, %lld, %lld): %lld drawn, %lld masked, brute force %lld", n, sps, s, drawn, masked, brute_masked);
            }
}

static void check_stated_folds() {
    // a fold the caller states: every (start, count) within the record passes, everything beyond it does not
    for (long long n : {1, 2, 7})
        for (long long start = -1; start <= n + 1; ++start)
            for (long long count = -1; count <= n + 1; ++count)
                for (long long P : {0, 1, 3})
                    for (long long L : {0, 1, 2})
                        for (long long nd = -1; nd <= n + 1; ++nd) {
                            const EyeFold f{start, count, P, L, nd, 0};
                            bool ok = start >= 0 && count >= 1 && P >= 1 && L >= 1 && nd >= 0;
                            if (ok) {
                                for (long long j = 0; j < count; ++j) ok = ok && start + j < n;      // every point is a sample of the record
                                ok = ok && nd * L <= count;                                         // every drawn point is a point
                            }
                            CHECK((eye_fold_check(f, n) == 0) == ok, "eye_fold_check({%lld, %lld, %lld, %lld, %lld}, %lld) = %d, brute force %d", start, count, P, L, nd, n,
                                  eye_fold_check(f, n), (int)ok);
                        }
}

int main() {
    check_plot_fold();
    check_stated_folds();
    std::printf("ok: %lld checks\n", g_checks);
    return 0;
}
