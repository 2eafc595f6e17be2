// The step sizes of one fixed-step run, looked at once: are they all usable, which distinct sizes are there (every one needs an operator table), and
// which of them does each step take.  Plain C++ -- no HIP types -- so that a host program can include it (tests/test_schedule_cpu.py).
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

namespace ssfm {

template <typename T> struct Schedule {
    std::vector<T> steps;                   // the step sizes in the plan's precision (a `double` source is narrowed here)
    std::vector<T> distinct;                // in order of first appearance; equal means bitwise equal.  Collection stops at max_tables + 1
    std::vector<unsigned char> which;       // distinct[which[s]] is step s, bit for bit (for every step whose size is among the collected ones)
    int64_t first_bad = -1;                 // the first step that is not finite and > 0 (as the caller gave it, before any narrowing); nothing behind it is looked at
    int max_tables = 0;

    template <typename Src> Schedule(const Src* h, int64_t nsteps, int max_tables_) : max_tables(max_tables_) {
        if (nsteps <= 0) return;
        steps.reserve((size_t)nsteps);
        which.reserve((size_t)nsteps);
        for (int64_t s = 0; s < nsteps; ++s) {
            if (!(h[s] > (Src)0) || !std::isfinite((double)h[s])) { first_bad = s; return; }
            const T v = (T)h[s];
            steps.push_back(v);
            size_t i = 0;
            while (i < distinct.size() && std::memcmp(&distinct[i], &v, sizeof(T)) != 0) ++i;
            if (i == distinct.size()) {
                if (distinct.size() <= (size_t)max_tables) distinct.push_back(v);
                else i = 0;                 // (a size beyond the ones collected: the schedule does not fit the tables, nobody reads its index)
            }
            which.push_back((unsigned char)i);
        }
    }
    bool valid() const { return first_bad < 0; }
    bool fits_tables() const { return distinct.size() <= (size_t)max_tables; }
    int64_t size() const { return (int64_t)steps.size(); }
};

}  // namespace ssfm
