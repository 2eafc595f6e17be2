// Host program of tests/test_sos_route_cpu.py: the SOS filter's dispatcher (opticomlib_amd/csrc/sos_route.hpp) and its tables (sos_tables.hpp) against restatements
// typed from run_filter / one_launch_would_run / run_filter_w / build_tables / build_meet_tables as they stood before the headers existed (sos_filter.hip,
// sos_filter_impl.inc).  Built with AddressSanitizer / UBSan; no GPU.  argv[1]: the filters, one per line -- sections, then 6 coefficients per section, then zi,
// as hexadecimal floats.  Prints "look <filter> <W> <chunk> <look>" per filter and layout, then "ok: <cells checked>"; exits non-zero on any miss.
#include "sos_route.hpp"
#include "sos_tables.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace ssfm::sos;

static long long failures = 0, checked = 0;
#define CHECK(cond, ...) do { ++checked; if (!(cond)) { if (++failures <= 40) { std::printf("FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

struct Coefs { double b0[4], b1[4], b2[4], a1[4], a2[4]; };

// ============================================================================= the parent, restated (its constants as literals)
namespace parent {

struct Env { bool one_launch, near, meet, long_chunk; bool force_set; int force_value; };      // what the getenv() calls answered
struct CapLog { int n = 0; int what[16][3]; void add(int chunk, int W, int meet) { if (n < 16) { what[n][0] = chunk; what[n][1] = W; what[n][2] = meet; } ++n; } };
struct Ctx {
    const Coefs* c; int ns, ch; long long n; int rows, edge; Env env; int give_ups, cus, look;
    long long cap[2][2][2];          // [long chunk][four wavefronts][meet]
    CapLog log;
    long long capacity(int chunk, int W, bool meet) { log.add(chunk, W, meet); return cap[chunk == 18][W == 4][meet]; }
};

static bool near_is_certain(const Ctx& x, long long len) {
    if (!x.env.near) return false;
    double r2 = 0.0;
    for (int s = 0; s < x.ns; ++s) {
        const double a1 = x.c->a1[s], a2 = x.c->a2[s], disc = a1 * a1 - 4.0 * a2;
        double m2;
        if (disc < 0.0) m2 = a2;
        else { const double z = 0.5 * (std::fabs(a1) + std::sqrt(disc)); m2 = z * z; }
        r2 = m2 > r2 ? m2 : r2;
    }
    if (!(r2 < 1.0)) return false;
    return 0.5 * std::log(r2) * (double)len * 4 < -138.2;
}
static bool one_launch_would_run(Ctx& x, int chunk, int W) {
    const int kGroup = 64 * W;
    const long long m = x.n + 2ll * x.edge, nchunks = (m + chunk - 1) / chunk, ngroups = (nchunks + kGroup - 1) / kGroup;
    const bool groups_ok = ngroups <= 2 * kGroup || (x.ch * 2 * x.ns <= 8 && ngroups <= 64 * 64 && near_is_certain(x, (long long)kGroup * chunk));
    return x.env.one_launch && x.give_ups < 3 && groups_ok && ngroups * x.rows <= x.capacity(chunk, W, false);
}
static int sos_waves(const Ctx& x) {
    const long long chunks = (x.n + 2ll * x.edge + 12 - 1) / 12 * x.rows;
    if (x.env.force_set) { const int v = x.env.force_value; if (v == 1 || v == 4) return v; }
    return chunks <= 16384 ? 1 : 4;
}
struct Outcome { int chunk, W, refusal, launches, look, tagged, meet; };
// run_filter_w up to the form: the refusals, then lines 1783-1785 and 1823-1824
static Outcome run_filter_w(Ctx& x, int chunk, int W) {
    Outcome o{chunk, W, 0, 3, 0, 0, 0};
    const int K = 2 * x.ns, kGroup = 64 * W;
    const long long m = x.n + 2ll * x.edge;
    const long long nchunks_ll = (m + chunk - 1) / chunk;
    if (nchunks_ll > (1ll << 30)) { o.refusal = 1; return o; }
    const int nchunks = (int)nchunks_ll;
    const int ngroups = (nchunks + kGroup - 1) / kGroup;
    if (ngroups > 64 * 64) { o.refusal = 2; return o; }
    if ((long long)ngroups * x.rows > 0x7fffffffll) { o.refusal = 3; return o; }
    const long long grid = (long long)ngroups * x.rows;
    const bool near_now = x.ch * K <= 8 && x.env.near && x.look <= 4;
    if (x.env.one_launch && x.give_ups < 3 && (ngroups <= 2 * kGroup || near_now) && grid <= x.capacity(chunk, W, false)) {
        o.launches = 1;
        o.look = near_now ? x.look : 0;
        o.tagged = x.ch * K <= 8;
        bool meet = false;
        if (x.ch * K <= 8) meet = x.env.meet && o.look >= 1 && o.look <= 2 && grid <= x.capacity(chunk, W, true);
        o.meet = meet;
    }
    return o;
}
// run_filter's cascade: the instance it hands the call to, as chunk * 8 + W
static int run_filter(Ctx& x) {
    const bool forced = x.env.force_set;
    const bool long_ok = x.env.long_chunk;
    if (sos_waves(x) == 1) return 12 * 8 + 1;
    if (!forced) {
        if (one_launch_would_run(x, 12, 1)) return 12 * 8 + 1;
        if (long_ok && one_launch_would_run(x, 18, 1)) return 18 * 8 + 1;
        if (long_ok) {
            const long long groups = ((x.n + 2ll * x.edge + 12 - 1) / 12 + 64 * 4 - 1) / (64 * 4);
            if (x.cus > 0 && groups * x.rows <= x.cus && one_launch_would_run(x, 12, 4)) return 12 * 8 + 4;
        }
    }
    if (long_ok && one_launch_would_run(x, 18, 4)) return 18 * 8 + 4;
    return 12 * 8 + 4;
}

template <int K> void matmul(const double* A, const double* B, double* C) {
    for (int r = 0; r < K; ++r)
        for (int q = 0; q < K; ++q) {
            double acc = 0.0;
            for (int m2 = 0; m2 < K; ++m2) acc += A[r * K + m2] * B[m2 * K + q];
            C[r * K + q] = acc;
        }
}
template <int NS, int W, int kChunk> void build_tables(const Coefs& c, std::vector<double>& tab) {
    constexpr int K = 2 * NS, kWaves = W, kWave = 64;
    double M[K * K];
    for (int q = 0; q < K; ++q) {
        double z[NS][2];
        for (int s = 0; s < NS; ++s) z[s][0] = z[s][1] = 0.0;
        z[q / 2][q % 2] = 1.0;
        for (int i = 0; i < kChunk; ++i) {
            double x = 0.0;
            for (int s = 0; s < NS; ++s) {
                const double xn = x;
                x = c.b0[s] * xn + z[s][0];
                z[s][0] = c.b1[s] * xn - c.a1[s] * x + z[s][1];
                z[s][1] = c.b2[s] * xn - c.a2[s] * x;
            }
        }
        for (int r = 0; r < K; ++r) M[r * K + q] = z[r / 2][r % 2];
    }
    std::vector<double> G((size_t)K * kChunk, 0.0);
    for (int t = 0; t < kChunk; ++t) {
        double z[NS][2];
        for (int s = 0; s < NS; ++s) z[s][0] = z[s][1] = 0.0;
        for (int i = t; i < kChunk; ++i) {
            double x = i == t ? 1.0 : 0.0;
            for (int s = 0; s < NS; ++s) {
                const double xn = x;
                x = c.b0[s] * xn + z[s][0];
                z[s][0] = c.b1[s] * xn - c.a1[s] * x + z[s][1];
                z[s][1] = c.b2[s] * xn - c.a2[s] * x;
            }
        }
        for (int k = 0; k < K; ++k) G[(size_t)k * kChunk + t] = z[k / 2][k % 2];
    }
    tab.assign((size_t)3 * (kWave + 1) * K * K, 0.0);
    for (int level = 0; level < 3; ++level) {
        double* P = tab.data() + (size_t)level * (kWave + 1) * K * K;
        for (int r = 0; r < K; ++r) P[r * K + r] = 1.0;
        for (int j = 0; j < kWave; ++j) matmul<K>(M, P + (size_t)j * K * K, P + (size_t)(j + 1) * K * K);
        std::memcpy(M, P + (size_t)kWave * K * K, sizeof(M));
        if (level == 0) {
            double A[K * K], B[K * K];
            std::memcpy(A, M, sizeof(M));
            for (int w = 1; w < kWaves; ++w) { matmul<K>(M, A, B); std::memcpy(A, B, sizeof(A)); }
            std::memcpy(M, A, sizeof(M));
        }
    }
    tab.insert(tab.end(), G.begin(), G.end());
}
// ... and what run_filter_w put behind them (lines 1747-1750), with the look-back depth it measured (1755-1761)
template <int NS, int W, int kChunk> int device_table(const Coefs& c, const double* zi_h, std::vector<double>& tab) {
    constexpr int K = 2 * NS, kWave = 64;
    build_tables<NS, W, kChunk>(c, tab);
    tab.insert(tab.end(), zi_h, zi_h + K);
    for (int level = 0; level < 2; ++level)
        for (int e = 0; e < K * K; ++e)
            for (int j = 0; j < kWave; ++j) tab.push_back(tab[(size_t)level * (kWave + 1) * K * K + (size_t)j * K * K + e]);
    int look = 1;
    for (int d = 1; d <= kWave; ++d) {
        const double* P = tab.data() + (size_t)(kWave + 1) * K * K + (size_t)d * K * K;
        double big = 0.0;
        for (int e = 0; e < K * K; ++e) big = std::fabs(P[e]) > big || P[e] != P[e] ? std::fabs(P[e]) : big;
        if (!(big < 1e-40)) look = d + 1;
    }
    return look;
}
template <int NS, int W, int kChunk> void build_meet_tables(const Coefs& c, const double* zi, long long jl, std::vector<double>& out) {
    constexpr int K = 2 * NS, kGroup = 64 * W;
    constexpr long long Lg = (long long)kGroup * kChunk;
    const auto step = [&](double (&z)[NS][2], double x) {
        for (int s = 0; s < NS; ++s) {
            const double xn = x;
            x = c.b0[s] * xn + z[s][0];
            z[s][0] = c.b1[s] * xn - c.a1[s] * x + z[s][1];
            z[s][1] = c.b2[s] * xn - c.a2[s] * x;
        }
        return x;
    };
    out.assign((size_t)2 * K * K * kGroup + 2 * K * K, 0.0);
    std::vector<double> dy((size_t)Lg);
    for (int variant = 0; variant < 2; ++variant) {
        double* Vm = out.data() + (size_t)variant * K * K * kGroup;
        double* Wm = out.data() + (size_t)2 * K * K * kGroup + (size_t)variant * K * K;
        const long long end = variant ? jl : Lg - 1;
        for (int q = 0; q < K; ++q) {
            double z[NS][2];
            for (int s = 0; s < NS; ++s) z[s][0] = z[s][1] = 0.0;
            z[q / 2][q % 2] = 1.0;
            for (long long j = 0; j <= end; ++j) dy[(size_t)j] = step(z, 0.0);
            for (long long j = end + 1; j < Lg; ++j) dy[(size_t)j] = dy[(size_t)end];
            double zb[NS][2];
            for (int s = 0; s < NS; ++s) { zb[s][0] = variant ? zi[2 * s] * dy[(size_t)end] : 0.0; zb[s][1] = variant ? zi[2 * s + 1] * dy[(size_t)end] : 0.0; }
            for (int pos = kGroup - 1; pos >= 0; --pos) {
                for (int r = 0; r < K; ++r) Vm[(size_t)(r * K + q) * kGroup + pos] = zb[r / 2][r % 2];
                for (int t = kChunk - 1; t >= 0; --t) (void)step(zb, dy[(size_t)pos * kChunk + t]);
            }
            for (int r = 0; r < K; ++r) Wm[r * K + q] = zb[r / 2][r % 2];
        }
    }
}

}  // namespace parent

// ============================================================================= the shape and the form
static Knobs knobs_of(const parent::Env& e) {
    Knobs kn;
    kn.one_launch = e.one_launch; kn.near = e.near; kn.meet = e.meet; kn.long_chunk = e.long_chunk;
    kn.waves_force = !e.force_set ? 0 : e.force_value ? e.force_value : -1;
    return kn;
}
// the header's form decision behind its refusals, as sos_filter.hip chains them, with the capacity questions logged
static parent::Outcome tree_form(const parent::Ctx& x, Shape s, parent::CapLog& log) {
    const Knobs kn = knobs_of(x.env);
    const auto capacity = [&](int chunk, int W) { log.add(chunk, W, 0); return x.cap[chunk == 18][W == 4][0]; };
    const auto capacity_meet = [&](int chunk, int W) { log.add(chunk, W, 1); return x.cap[chunk == 18][W == 4][1]; };
    parent::Outcome o{s.chunk, s.W, 0, 3, 0, 0, 0};
    const Geometry g = geometry(x.n, x.edge, s.chunk, s.W);
    o.refusal = (int)refusal(g, x.rows);
    if (o.refusal) return o;
    const Form f = choose_form(s, g, x.ns, x.ch, x.rows, kn, x.give_ups, x.look, capacity, capacity_meet);
    int route[8];
    fill_route(route, s, f, x.ns, x.ch);
    if (!(route[0] == s.W && route[1] == s.chunk && route[2] == f.launches && route[3] == f.look && route[4] == (int)f.tagged && route[5] == (int)f.meet && route[6] == x.ns && route[7] == x.ch))
        CHECK(false, "fill_route");
    o.launches = f.launches; o.look = f.look; o.tagged = f.tagged; o.meet = f.meet;
    return o;
}

// n on both sides of every size at which a decision changes, for these rows and this edge
static int lengths(int rows, int edge, long long* out) {
    int k = 0;
    const auto both = [&](long long m) { out[k++] = m - 2ll * edge; out[k++] = m + 1 - 2ll * edge; };
    out[k++] = edge + 1; out[k++] = edge + 2;
    both(12ll * (16384 / rows));                               // kSmallChunks chunks in all
    both(12ll * 256 * (256 / rows > 0 ? 256 / rows : 1));      // `cus` = 256 groups of four short-chunk wavefronts in all
    static const int layouts[4][2] = {{12, 1}, {18, 1}, {12, 4}, {18, 4}};
    for (const auto& l : layouts) {
        both((long long)l[0] * 64 * l[1] * 128 * l[1]);        // kLookIter x threads groups per row (128 for one wavefront, 512 for four) ...
        both((long long)l[0] * 64 * l[1] * 128);               // ... and 128 groups whatever the shape
        both((long long)l[0] * 64 * l[1] * 4096);              // 64 x 64 groups per row
    }
    both(12ll << 30); both(18ll << 30);                        // 2^30 chunks
    return k;
}

static void check_decisions() {
    // poles per section count: [0] near_is_certain holds for every layout (a real pair of 0.5 first, then complex pairs of |z|^2 = 0.3), [1] it does not (|z|^2 = 0.999)
    Coefs poles[2];
    std::memset(poles, 0, sizeof(poles));
    for (int s = 0; s < 4; ++s) {
        poles[0].a1[s] = s == 0 ? -0.9 : -1.0; poles[0].a2[s] = s == 0 ? 0.2 : 0.3;
        poles[1].a1[s] = -1.9; poles[1].a2[s] = s == 0 ? 0.999 : 0.5;
    }
    // capacities [table][long][four wavefronts]: none; 256 x {1, 2, 3, 8} in every instance; the four multiples dealt over the instances, twice; unbounded.
    // The single-meeting instance holds 256 fewer.
    constexpr int kCaps = 8;
    long long caps[kCaps][2][2];
    static const int mult[4] = {1, 2, 3, 8};
    for (int t = 0; t < kCaps; ++t)
        for (int i = 0; i < 4; ++i) caps[t][i / 2][i % 2] = t == 0 ? 0 : t == kCaps - 1 ? (1ll << 62) : t <= 4 ? 256ll * mult[t - 1] : 256ll * mult[(i + 2 * t) % 4];
    static const int rows_of[4] = {1, 2, 3, 1000}, forces[4] = {0, 1, 4, 7}, looks[5] = {1, 2, 4, 5, 1 << 30}, cus_of[2] = {0, 256};
    long long ns_list[64];
    for (int ns = 1; ns <= 4; ++ns) for (int ch = 1; ch <= 2; ++ch) for (int ri = 0; ri < 4; ++ri) for (int pi = 0; pi < 2; ++pi) {
        const int edge = 3 * (2 * ns + 1), nn = lengths(rows_of[ri], edge, ns_list);
        CHECK(near_is_certain(poles[pi], ns, 768, true) == (pi == 0) && near_is_certain(poles[pi], ns, 4608, true) == (pi == 0) && !near_is_certain(poles[pi], ns, 4608, false), "poles %d", pi);
        for (int knobs = 0; knobs < 16; ++knobs) for (int fi = 0; fi < 4; ++fi) for (int gu = 0; gu <= 3; ++gu) for (int ci = 0; ci < 2; ++ci)
        for (int t = 0; t < kCaps; ++t) for (int ni = 0; ni < nn; ++ni) {
            parent::Ctx x;
            x.c = &poles[pi]; x.ns = ns; x.ch = ch; x.n = ns_list[ni]; x.rows = rows_of[ri]; x.edge = edge;
            x.env = parent::Env{(knobs & 1) != 0, (knobs & 2) != 0, (knobs & 4) != 0, (knobs & 8) != 0, forces[fi] != 0, forces[fi]};
            x.give_ups = gu; x.cus = cus_of[ci]; x.look = 0;
            for (int i = 0; i < 4; ++i) { x.cap[i / 2][i % 2][0] = caps[t][i / 2][i % 2]; x.cap[i / 2][i % 2][1] = caps[t][i / 2][i % 2] >= 256 && t != kCaps - 1 ? caps[t][i / 2][i % 2] - 256 : caps[t][i / 2][i % 2]; }
            if (x.n <= edge) continue;
            // the shape (it does not see `look`) ...
            const int p_shape = parent::run_filter(x);
            parent::CapLog log;
            const auto capacity = [&](int chunk, int W) { log.add(chunk, W, 0); return x.cap[chunk == 18][W == 4][0]; };
            const Shape s = choose_shape(*x.c, ns, ch, x.n, x.rows, edge, knobs_of(x.env), gu, x.cus, capacity);
            const bool same_asked = log.n == x.log.n && log.n <= 16 && std::memcmp(log.what, x.log.what, sizeof(int) * 3 * log.n) == 0;
            CHECK(p_shape == s.chunk * 8 + s.W && same_asked, "ns %d ch %d rows %d n %lld knobs %d force %d give_ups %d cus %d caps %d poles %d: parent %d x %d (%d capacities asked), header %d x %d (%d asked)",
                  ns, ch, x.rows, x.n, knobs, forces[fi], gu, x.cus, t, pi, p_shape % 8, p_shape / 8, x.log.n, s.W, s.chunk, log.n);
            // ... and the form in the parent's shape, for every look
            for (int li = 0; li < 5; ++li) {
                x.look = looks[li];
                x.log = parent::CapLog();
                const parent::Outcome p = parent::run_filter_w(x, p_shape / 8, p_shape % 8);
                parent::CapLog flog;
                const parent::Outcome q = tree_form(x, Shape{p_shape / 8, p_shape % 8}, flog);
                const bool same = p.refusal == q.refusal && p.launches == q.launches && p.look == q.look && p.tagged == q.tagged && p.meet == q.meet;
                const bool asked = flog.n == x.log.n && flog.n <= 16 && std::memcmp(flog.what, x.log.what, sizeof(int) * 3 * flog.n) == 0;
                CHECK(same && asked, "ns %d ch %d rows %d n %lld knobs %d force %d give_ups %d look %d caps %d, %d x %d: parent refusal %d launches %d look %d tagged %d meet %d (%d capacities asked), "
                      "header refusal %d launches %d look %d tagged %d meet %d (%d asked)", ns, ch, x.rows, x.n, knobs, forces[fi], gu, x.look, t, p.W, p.chunk,
                      p.refusal, p.launches, p.look, p.tagged, p.meet, x.log.n, q.refusal, q.launches, q.look, q.tagged, q.meet, flog.n);
            }
        }
    }
}

// ============================================================================= the give-up state over 2100 calls
// pattern 0: every one-launch call succeeds; 1: every one gives up; 2: the first three give up, the later ones succeed
static void check_give_ups() {
    Coefs c;
    std::memset(&c, 0, sizeof(c));
    c.a1[0] = -1.0; c.a2[0] = 0.3;
    const Knobs kn;
    const auto huge = [](int, int) { return 1ll << 40; };
    const long long n = 300000;          // past kSmallChunks: the dispatcher picks one wavefront only while it expects one launch
    for (int pattern = 0; pattern < 3; ++pattern) {
        int give_ups = 0, rested = 0, third = -1;          // the parent's two counters
        GiveUps g;
        for (int call = 0; call < 2100; ++call) {
            // the parent: run_filter reads give_ups, then run_filter_w ticks (line 1782), tries one launch if give_ups < 3, and counts
            const int p_shape_saw = give_ups;
            if (give_ups >= 3 && ++rested >= 1000) { give_ups = 3 - 1; rested = 0; }
            const int p_form_saw = give_ups;
            const bool p_tried = give_ups < 3;
            const bool gives_up = pattern == 1 || (pattern == 2 && third < 0);
            if (p_tried) { if (gives_up) ++give_ups; else give_ups = 0; }
            if (pattern && third < 0 && give_ups == 3) third = call;
            // the header
            const int shape_saw = g.give_ups;
            const Shape s = choose_shape(c, 1, 2, n, 1, 9, kn, g.give_ups, 256, huge);
            g = tick_before_form(g);
            const int form_saw = g.give_ups;
            const Form f = choose_form(s, geometry(n, 9, s.chunk, s.W), 1, 2, 1, kn, g.give_ups, 1, huge, huge);
            if (f.launches == 1) g = after_one_launch(g, gives_up);
            CHECK(g.give_ups == give_ups && g.rested == rested && (f.launches == 1) == p_tried && shape_saw == p_shape_saw && form_saw == p_form_saw,
                  "pattern %d call %d: parent {%d, %d, tried %d}, header {%d, %d, tried %d}", pattern, call, give_ups, rested, (int)p_tried, g.give_ups, g.rested, f.launches == 1);
            CHECK((s.W == kWavesSmall) == (shape_saw < kMaxGiveUps), "pattern %d call %d: shape %d x %d with give_ups %d", pattern, call, s.W, s.chunk, shape_saw);
            if (third >= 0 && call == third + kRestCalls)          // the retry: its shape chosen while the form still rested, its form after the tick
                CHECK(shape_saw == 3 && form_saw == 2 && f.launches == 1 && s.W == kWavesLarge && s.chunk == kChunkShort, "pattern %d: the retry call saw %d then %d, ran %d x %d in %d launches",
                      pattern, shape_saw, form_saw, s.W, s.chunk, f.launches);
        }
        CHECK(pattern == 0 ? third < 0 : third == 2, "pattern %d: third give-up at call %d", pattern, third);
    }
}

// ============================================================================= the tables
static bool same_bits(const std::vector<double>& a, const std::vector<double>& b) { return a.size() == b.size() && std::memcmp(a.data(), b.data(), sizeof(double) * a.size()) == 0; }

template <int NS, int W, int CHUNK> static void check_tables(int filter, const Coefs& c, const double* zi) {
    constexpr int K = 2 * NS;
    using Lay = TableLayout<NS, CHUNK>;
    using Meet = MeetLayout<NS, W>;
    std::vector<double> want, got;
    const int look = parent::device_table<NS, W, CHUNK>(c, zi, want);
    build_tables<NS, W, CHUNK>(c, zi, got);
    CHECK(same_bits(want, got) && got.size() == Lay::total, "filter %d, %d sections, W %d chunk %d: the device table (%zu doubles against %zu)", filter, NS, W, CHUNK, got.size(), want.size());
    CHECK(Lay::pwG == 65u * K * K && Lay::pwH == 2u * 65 * K * K && Lay::G == 3u * 65 * K * K && Lay::zi == Lay::G + K * CHUNK && Lay::pwT == Lay::zi + K && Lay::pwGT == Lay::pwT + 64u * K * K,
          "layout of %d sections, chunk %d", NS, CHUNK);
    CHECK(look_of_group_powers(got.data() + Lay::pwG, K) == look, "filter %d W %d chunk %d: look %d", filter, W, CHUNK, look);
    std::printf("look %d %d %d %d\n", filter, W, CHUNK, look);
    const long long ends[3] = {0, CHUNK, 64ll * W * CHUNK - 1};          // the row ends on the group's first sample, one chunk in, on its last sample
    for (long long jl : ends) {
        parent::build_meet_tables<NS, W, CHUNK>(c, zi, jl, want);
        build_meet_tables<NS, W, CHUNK>(c, zi, jl, got);
        CHECK(same_bits(want, got) && got.size() == Meet::total && Meet::Wm == 2u * K * K * 64 * W, "filter %d, %d sections, W %d chunk %d, jl %lld: the meet tables", filter, NS, W,
              CHUNK, jl);
    }
}
template <int NS> static void check_layouts(int filter, const Coefs& c, const double* zi) {
    check_tables<NS, 1, 12>(filter, c, zi); check_tables<NS, 4, 12>(filter, c, zi); check_tables<NS, 1, 18>(filter, c, zi); check_tables<NS, 4, 18>(filter, c, zi);
}
static int check_filters(const char* path) {
    FILE* f = std::fopen(path, "r");
    if (!f) { std::printf("cannot read %s\n", path); return 0; }
    int ns = 0, filters = 0;
    while (std::fscanf(f, "%d", &ns) == 1 && ns >= 1 && ns <= 4) {
        Coefs c;
        std::memset(&c, 0, sizeof(c));
        double zi[8], r[6];
        char word[64];
        const auto next = [&]() { return std::fscanf(f, "%63s", word) == 1 ? std::strtod(word, nullptr) : std::nan(""); };
        for (int s = 0; s < ns; ++s) {
            for (double& v : r) v = next();
            c.b0[s] = r[0]; c.b1[s] = r[1]; c.b2[s] = r[2]; c.a1[s] = r[4]; c.a2[s] = r[5];
        }
        for (int k = 0; k < 2 * ns; ++k) zi[k] = next();
        switch (ns) {
            case 1: check_layouts<1>(filters, c, zi); break;
            case 2: check_layouts<2>(filters, c, zi); break;
            case 3: check_layouts<3>(filters, c, zi); break;
            default: check_layouts<4>(filters, c, zi); break;
        }
        ++filters;
    }
    std::fclose(f);
    return filters;
}

int main(int argc, char** argv) {
    if (argc < 2) { std::printf("usage: %s <filters file>\n", argv[0]); return 2; }
    CHECK(geometry(1000, 15, 12, 1).m == 1030 && geometry(1000, 15, 12, 1).nchunks == 86 && geometry(1000, 15, 12, 1).ngroups == 2 && geometry(1000, 15, 18, 4).ngroups == 1, "geometry");
    check_decisions();
    check_give_ups();
    const int filters = check_filters(argv[1]);
    CHECK(filters == 24, "%d filters read", filters);
    if (failures) { std::printf("%lld of %lld checks failed\n", failures, checked); return 1; }
    std::printf("ok: %lld\n", checked);
    return 0;
}
