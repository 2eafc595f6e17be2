// Host program of tests/test_schedule_cpu.py: ssfm::Schedule (opticomlib_amd/csrc/ssfm_schedule.hpp) against a brute-force restatement, built with
// AddressSanitizer / UBSan.  K_MAX_TABLES comes from the command line (the test reads kMaxTables out of ssfm_host.hip).
#include "ssfm_schedule.hpp"

#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#ifndef K_MAX_TABLES
#error "K_MAX_TABLES is not set"
#endif

static int failures = 0;
static int checked = 0;
#define CHECK(cond, ...) do { if (!(cond)) { ++failures; std::printf("FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

template <typename A> static bool same_bits(const A& a, const A& b) { return std::memcmp(&a, &b, sizeof(A)) == 0; }

// What the plan's entry points did before there was a Schedule, step by step: the first step that is not finite and > 0 (as given), the sizes narrowed to T,
// the distinct ones by bitwise comparison in order of first appearance, collected until there are kmax + 1 of them.
template <typename T, typename Src> static void check_case(const char* name, const std::vector<Src>& h, int kmax, int64_t want_bad) {
    ++checked;
    const ssfm::Schedule<T> sch(h.data(), (int64_t)h.size(), kmax);
    int64_t bad = -1;
    for (size_t s = 0; s < h.size() && bad < 0; ++s)
        if (!(h[s] > (Src)0) || !std::isfinite((double)h[s])) bad = (int64_t)s;
    CHECK(bad == want_bad, "%s: the case itself: first bad step %lld, stated %lld", name, (long long)bad, (long long)want_bad);
    CHECK(sch.first_bad == want_bad, "%s: first_bad %lld, expected %lld", name, (long long)sch.first_bad, (long long)want_bad);
    CHECK(sch.valid() == (want_bad < 0), "%s: valid()", name);
    if (want_bad >= 0) return;
    CHECK(sch.size() == (int64_t)h.size() && sch.steps.size() == h.size() && sch.which.size() == h.size(), "%s: %lld steps of %zu", name, (long long)sch.size(), h.size());
    std::vector<T> brute;                   // every distinct size, without a limit
    for (size_t s = 0; s < h.size(); ++s) {
        const T v = (T)h[s];
        CHECK(same_bits(sch.steps[s], v), "%s: step %zu", name, s);
        bool seen = false;
        for (const T& d : brute) seen = seen || same_bits(d, v);
        if (!seen) brute.push_back(v);
    }
    const bool fits = brute.size() <= (size_t)kmax;
    CHECK(sch.fits_tables() == fits, "%s: fits_tables() with %zu distinct sizes", name, brute.size());
    const size_t want_n = fits ? brute.size() : (size_t)kmax + 1;
    CHECK(sch.distinct.size() == want_n, "%s: %zu distinct sizes, expected %zu", name, sch.distinct.size(), want_n);
    for (size_t i = 0; i < sch.distinct.size() && i < brute.size(); ++i)
        CHECK(same_bits(sch.distinct[i], brute[i]), "%s: distinct[%zu] is not the %zu-th size to appear", name, i, i);
    for (size_t i = 0; i < sch.distinct.size(); ++i)
        for (size_t j = 0; j < i; ++j) CHECK(!same_bits(sch.distinct[i], sch.distinct[j]), "%s: distinct[%zu] == distinct[%zu]", name, i, j);
    if (brute.size() > (size_t)kmax + 1) return;          // (sizes beyond the collected ones have no index)
    for (size_t s = 0; s < h.size(); ++s) {
        CHECK((size_t)sch.which[s] < sch.distinct.size(), "%s: which[%zu] = %d", name, s, (int)sch.which[s]);
        if ((size_t)sch.which[s] < sch.distinct.size()) CHECK(same_bits(sch.distinct[sch.which[s]], sch.steps[s]), "%s: distinct[which[%zu]] is not step %zu", name, s, s);
    }
}

template <typename T> static void run_all(const char* tn, int kmax) {
    const std::string p = std::string(tn) + ": ";
    auto nm = [&](const std::string& s) { return p + s; };
    check_case<T, T>(nm("one step").c_str(), {(T)0.1}, kmax, -1);
    {
        std::vector<T> h(37, (T)0.25);
        h.back() = (T)0.07;
        check_case<T, T>(nm("constant with a shorter last step").c_str(), h, kmax, -1);
    }
    for (int extra = 0; extra <= 1; ++extra) {          // exactly kmax, exactly kmax + 1 distinct sizes (each twice, interleaved, the first one again at the end)
        std::vector<T> h;
        for (int r = 0; r < 2; ++r)
            for (int i = 0; i < kmax + extra; ++i) h.push_back((T)(0.5 + 0.125 * i));
        h.push_back(h[0]);
        check_case<T, T>(nm(extra ? "kMaxTables + 1 sizes" : "kMaxTables sizes").c_str(), h, kmax, -1);
    }
    {
        // values that are rejected, at the first, a middle and the last index; a denormal is a step like any other
        const T rejected[] = {(T)0.0, (T)-0.0, std::numeric_limits<T>::infinity(), std::numeric_limits<T>::quiet_NaN(), (T)-0.5, -std::numeric_limits<T>::infinity()};
        const size_t len = 9, at[] = {0, 4, len - 1};
        for (const T bad : rejected)
            for (const size_t where : at) {
                std::vector<T> h(len, (T)0.3);
                h[where] = bad;
                check_case<T, T>(nm("a rejected value").c_str(), h, kmax, (int64_t)where);
            }
        {
            std::vector<T> h(len, (T)0.3);              // two bad steps: the first one is reported
            h[2] = (T)-1; h[6] = std::numeric_limits<T>::quiet_NaN();
            check_case<T, T>(nm("two rejected values").c_str(), h, kmax, 2);
        }
        for (const size_t where : at) {
            std::vector<T> h(len, (T)0.3);
            h[where] = std::numeric_limits<T>::denorm_min();
            check_case<T, T>(nm("a denormal").c_str(), h, kmax, -1);
        }
    }
    {
        std::vector<T> h(100000);
        const T three[] = {(T)0.1, (T)0.2, (T)0.05};
        for (size_t s = 0; s < h.size(); ++s) h[s] = three[s % 3];
        check_case<T, T>(nm("100 000 steps of three sizes").c_str(), h, kmax, -1);
    }
}

int main() {
    const int kmax = K_MAX_TABLES;
    run_all<float>("float", kmax);
    run_all<double>("double", kmax);
    // a float64 schedule on a complex64 plan: the sizes are narrowed first, so two that round to one float32 size are one size
    {
        const double a = 0.1, b = std::nextafter(0.1, 1.0);
        CHECK(a != b && (float)a == (float)b, "the case itself");
        const std::vector<double> h = {a, b, 0.2, a, b};
        check_case<float, double>("float from double: two sizes that narrow to one", h, kmax, -1);
        const ssfm::Schedule<float> sch(h.data(), (int64_t)h.size(), kmax);
        CHECK(sch.distinct.size() == 2 && sch.which[0] == 0 && sch.which[1] == 0 && sch.which[2] == 1 && sch.which[3] == 0 && sch.which[4] == 0, "narrowed sizes share a table");
        const ssfm::Schedule<double> wide(h.data(), (int64_t)h.size(), kmax);
        CHECK(wide.distinct.size() == 3, "in float64 they are two sizes");
        // ... and validity is decided on what the caller gave: a float64 size below float32's range is a step (of size 0 once narrowed), as it was
        check_case<float, double>("float from double: a size that narrows to zero", {0.1, 1e-60, 0.1}, kmax, -1);
        check_case<float, double>("float from double: a bad step", {0.1, 0.2, -0.0, 0.1}, kmax, 2);
    }
    {
        const ssfm::Schedule<float> none((const float*)nullptr, 0, kmax);
        CHECK(none.valid() && none.size() == 0 && none.distinct.empty() && none.fits_tables(), "an empty schedule");
    }
    if (failures) { std::printf("%d failures\n", failures); return 1; }
    std::printf("ok: %d cases\n", checked);
    return 0;
}
