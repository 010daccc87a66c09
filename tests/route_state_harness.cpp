// Host-only harness of tests/test_route_state_cpu.py: the engine's host state machines (stereo-depth_amd/csrc/smx_route.h:
// the lane ledger and the content switches with their per-call decision step) against models, compiled as plain C++ under
// AddressSanitizer + UndefinedBehaviorSanitizer.  It runs the very lines enqueue() runs; no HIP runtime, no GPU.
//
// Part A, LaneLedger against a brute-force model that keeps what every lane has entered since the other lane last waited
// for it (exact unions of pair slots and of output bytes):
//   safety      the model sees an unordered overlap of pair slots or output bytes  =>  the ledger asked for the wait
//   precision   pair range outside the other lane's hull of pair slots, output disjoint from its outputs, and that lane
//               never held more than OUT_RANGES_MAX disjoint non-adjacent outputs since it was last waited for
//               =>  no wait; the two steady states of include/stereo_mi355x.h run without a single wait
//   bounded     out_live[k].size() <= OUT_RANGES_MAX; stored ranges neither overlap nor touch
// Part B, ContentSwitch / RouteState against the documented rules, with reports delivered late, per lane in either order,
// rewritten, and sequence numbers started next to the 32-bit wrap; and the liveness sweep: for every cycle of eligible (E)
// and ineligible (I) calls, every phase and lag, the switch is off again within 64 + lag + 1 eligible calls once the
// content is back below `lo`.
//
// Output: one line per violation (the first few of each kind), one "liveness-cycle" line per cycle of the table in the
// issue, and the summary line
//   "route-state entries <n> waits <n> fallbacks <n> steady_entries <n> calls <n> probes <n> reports <n> liveness_cases <n> violations <n>".
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <deque>
#include <map>
#include <random>
#include <string>
#include <vector>

#include "smx_route.h"

using smx::CallKind;
using smx::CallRoute;
using smx::ContentSwitch;
using smx::HostHints;
using smx::LaneLedger;
using smx::RouteState;

static long g_violations = 0;
static std::map<std::string, long> g_by_kind;
#define VIOLATION(kind, ...)                                  \
    do {                                                      \
        g_violations++;                                       \
        if (g_by_kind[kind]++ < 8) {                          \
            std::printf("violation %s: ", kind);              \
            std::printf(__VA_ARGS__);                         \
            std::printf("\n");                                \
        }                                                     \
    } while (0)

// ------------------------------------------------------------------------------------------------ part A: the lane ledger
// An exact union of half-open intervals (touching intervals are merged: the same set of points).
struct IntervalSet {
    std::map<uintptr_t, uintptr_t> iv;   // lo -> hi
    void add(uintptr_t lo, uintptr_t hi) {
        auto it = iv.lower_bound(lo);
        if (it != iv.begin() && std::prev(it)->second >= lo) --it;
        while (it != iv.end() && it->first <= hi) {
            lo = std::min(lo, it->first);
            hi = std::max(hi, it->second);
            it = iv.erase(it);
        }
        iv[lo] = hi;
    }
    bool overlaps(uintptr_t lo, uintptr_t hi) const {
        auto it = iv.lower_bound(hi);            // first interval starting at or after hi: cannot overlap
        if (it == iv.begin()) return false;
        --it;
        return it->second > lo;
    }
    void clear() { iv.clear(); }
};

struct LaneModel {
    IntervalSet pairs, out;
    size_t max_components = 0;   // the most disjoint non-adjacent outputs held since the other lane last waited for this one
    struct Raw { int lo, hi; uintptr_t olo, ohi; };
    std::vector<Raw> raw;        // every entry itself, while there are few: cross-checks the interval sets
    void clear() { pairs.clear(); out.clear(); raw.clear(); max_components = 0; }
};

struct LedgerRun {
    LaneLedger ledger;
    LaneModel model[2];
    long entries = 0, waits = 0, fallbacks = 0, spurious = 0;

    bool enter(int k, int lo, int hi, uintptr_t olo, uintptr_t ohi) {
        const int o = 1 - k;
        LaneModel &mo = model[o], &mk = model[k];
        const bool pair_clash = mo.pairs.overlaps((uintptr_t)lo, (uintptr_t)hi), out_clash = mo.out.overlaps(olo, ohi);
        if (mo.raw.size() <= 2000) {
            bool rp = false, ro = false;
            for (const LaneModel::Raw &r : mo.raw) {
                rp = rp || (lo < r.hi && r.lo < hi);
                ro = ro || (olo < r.ohi && r.olo < ohi);
            }
            if (rp != pair_clash || ro != out_clash) VIOLATION("model", "the interval sets and the raw entries disagree at entry %ld", entries);
        }
        bool outside_hull = true;
        if (!mo.pairs.iv.empty())
            outside_hull = (uintptr_t)hi <= mo.pairs.iv.begin()->first || (uintptr_t)lo >= mo.pairs.iv.rbegin()->second;
        const bool got = ledger.enter(k, lo, hi, olo, ohi);
        entries++;
        if ((pair_clash || out_clash) && !got)
            VIOLATION("ledger-safety", "entry %ld lane %d pairs [%d, %d) out [%#zx, %#zx): unordered overlap (%s) and no wait",
                      entries, k, lo, hi, (size_t)olo, (size_t)ohi, pair_clash ? "pair slots" : "output bytes");
        if (got && outside_hull && !out_clash && mo.max_components <= LaneLedger::OUT_RANGES_MAX)
            VIOLATION("ledger-precision", "entry %ld lane %d pairs [%d, %d) out [%#zx, %#zx): a wait although the other lane (%zu outputs at most) shares nothing",
                      entries, k, lo, hi, (size_t)olo, (size_t)ohi, mo.max_components);
        if (got) {
            waits++;
            if (!pair_clash && !out_clash) spurious++;
            mo.clear();
        }
        mk.pairs.add((uintptr_t)lo, (uintptr_t)hi);
        mk.out.add(olo, ohi);
        if (mk.raw.size() <= 2000) mk.raw.push_back({lo, hi, olo, ohi});
        if (mk.out.iv.size() > LaneLedger::OUT_RANGES_MAX && mk.max_components <= LaneLedger::OUT_RANGES_MAX) fallbacks++;
        mk.max_components = std::max(mk.max_components, mk.out.iv.size());
        // boundedness, and (while no fallback has fired) the ledger holds exactly the model's union
        for (int l = 0; l < 2; ++l) {
            const std::vector<LaneLedger::OutRange> &live = ledger.out_live[l];
            if (live.size() > LaneLedger::OUT_RANGES_MAX) VIOLATION("ledger-bounded", "entry %ld: lane %d holds %zu ranges", entries, l, live.size());
            for (size_t i = 0; i < live.size(); ++i)
                for (size_t j = i + 1; j < live.size(); ++j)
                    if (live[i].lo <= live[j].hi && live[j].lo <= live[i].hi)
                        VIOLATION("ledger-bounded", "entry %ld: lane %d stores ranges that overlap or touch", entries, l);
            if (model[l].max_components <= LaneLedger::OUT_RANGES_MAX) {
                std::vector<LaneLedger::OutRange> s = live;
                std::sort(s.begin(), s.end(), [](const LaneLedger::OutRange &a, const LaneLedger::OutRange &b) { return a.lo < b.lo; });
                bool same = s.size() == model[l].out.iv.size();
                size_t i = 0;
                if (same)
                    for (const auto &m : model[l].out.iv) {
                        same = same && s[i].lo == m.first && s[i].hi == m.second;
                        ++i;
                    }
                if (!same) VIOLATION("ledger-exact", "entry %ld: lane %d's stored outputs are not the union of what it entered", entries, l);
            }
        }
        return got;
    }
    // enqueue()'s two call patterns on an engine of B pair slots
    void split_call(int n, uintptr_t out, uintptr_t pair_bytes) {
        const int n0 = (n + 1) / 2;
        enter(1, n0, n, out + (uintptr_t)n0 * pair_bytes, out + (uintptr_t)n * pair_bytes);     // lane 1 first
        enter(0, 0, n0, out, out + (uintptr_t)n0 * pair_bytes);
    }
    int next_small_lane = 0;
    void small_call(int B, int n, uintptr_t out, uintptr_t pair_bytes) {
        const int lane = next_small_lane;
        next_small_lane ^= 1;
        const int first = lane * (B / 2);
        enter(lane, first, first + n, out, out + (uintptr_t)n * pair_bytes);
    }
};

struct LedgerTotals { long entries = 0, waits = 0, fallbacks = 0, steady = 0; };

static void ledger_sweep(LedgerTotals &t) {
    std::mt19937_64 rng(20240917);
    auto rnd = [&](uint64_t lo, uint64_t hi) { return lo + rng() % (hi - lo + 1); };
    const uintptr_t TOP = UINTPTR_MAX;
    // steady state 1 (header): every call split the same way, outputs from a ring of up to 32 buffers
    for (int rep = 0; rep < 40; ++rep) {
        LedgerRun r;
        const int n = (int)rnd(2, 96), ring = (int)rnd(1, 32);
        const uintptr_t pb = rnd(1, 1 << 20), gap = rnd(0, 3), base = rep % 4 == 3 ? TOP - (uintptr_t)ring * ((uintptr_t)n * pb + gap) : rnd(1, 1ull << 40);
        for (int i = 0; i < 200; ++i) r.split_call(n, base + (uintptr_t)(i % ring) * ((uintptr_t)n * pb + gap), pb);
        if (r.waits) VIOLATION("ledger-steady", "split calls of %d pairs over a ring of %d outputs: %ld waits", n, ring, r.waits);
        t.entries += r.entries; t.steady += r.entries; t.waits += r.waits;
    }
    // steady state 2 (header): small calls alternating over the two buffer halves, ring of an even number of non-adjacent outputs
    // (up to 32 per lane)
    for (int rep = 0; rep < 60; ++rep) {
        LedgerRun r;
        const int B = 2 * (int)rnd(1, 48), n = (int)rnd(1, B / 2), ring = 2 * (int)rnd(1, 32);
        const uintptr_t pb = rnd(1, 1 << 20), gap = rnd(1, 2), stride = (uintptr_t)n * pb + gap;
        const uintptr_t base = rep % 4 == 3 ? TOP - (uintptr_t)ring * stride : rnd(1, 1ull << 40);
        for (int i = 0; i < 400; ++i) r.small_call(B, n, base + (uintptr_t)(i % ring) * stride, pb);
        if (r.waits) VIOLATION("ledger-steady", "small calls of %d pairs (max_batch %d) over a ring of %d outputs: %ld waits", n, B, ring, r.waits);
        t.entries += r.entries; t.steady += r.entries; t.waits += r.waits;
    }
    // everything mixed, in phases, on one ledger
    for (int rep = 0; rep < 6; ++rep) {
        LedgerRun r;
        const int B = 2 * (int)rnd(1, 48);
        while (r.entries < 25000) {
            const int phase = (int)rnd(0, 6), len = (int)rnd(1, 300);
            const uintptr_t pb = rnd(1, 1 << 16);
            const int ring = (int)rnd(2, 100);
            const uintptr_t gap = phase == 2 ? 0 : (phase == 3 ? 1 : rnd(1, 4096));
            const uintptr_t slot = (uintptr_t)B * pb + gap;
            const uintptr_t base = rnd(0, 4) == 0 ? TOP - (uintptr_t)ring * slot : rnd(0, 1ull << 44);
            for (int i = 0; i < len; ++i) {
                const uintptr_t out = base + (uintptr_t)(i % ring) * slot;
                switch (phase) {
                case 0: r.split_call((int)rnd(2, B), out, pb); break;                         // split calls of changing size
                case 1: case 2: case 3:                                                      // rings of 2 .. 100 outputs: gaps, zero-gap, one byte
                    if (2 * 1 <= B) r.small_call(B, (int)rnd(1, B / 2), out, pb);
                    break;
                case 4: {                                                                    // repeated and partly overlapping outputs
                    const uintptr_t o = base + rnd(0, 3) * (pb / 2 + 1);
                    if (rnd(0, 1)) r.small_call(B, (int)rnd(1, B / 2), o, pb); else r.split_call((int)rnd(2, B), o, pb);
                    break;
                }
                case 5: {                                                                    // anything: any lane, any slots, any bytes
                    const int lo = (int)rnd(0, B - 1), hi = (int)rnd(lo + 1, B);
                    const uintptr_t olo = rnd(0, 1) ? rnd(0, 1 << 12) : TOP - rnd(1, 1 << 12), len_b = rnd(1, 64);
                    r.enter((int)rnd(0, 1), lo, hi, olo, olo > TOP - len_b ? TOP : olo + len_b);
                    break;
                }
                default:                                                                     // every other slot of one big tensor, one pair each
                    r.small_call(B, 1, base + (uintptr_t)(2 * (i % ring)) * pb, pb);
                }
            }
        }
        t.entries += r.entries; t.waits += r.waits; t.fallbacks += r.fallbacks;
    }
}

// ------------------------------------------------------------------------------------------------ part B: the content switches
// The documented rules of one switch (smx_route.h, include/stereo_mi355x.h: smx_route_info), kept apart from its code.
struct SwitchModel {
    float hi, lo;
    bool on = false, pending = false;
    int period = 16;
    unsigned seen[2] = {0, 0};
    float last = -1.f;
    long probes = 0, doublings_this_probe = 0;
};

struct Flight { long at; unsigned long long word; };

struct Sim {
    RouteState rs;
    HostHints hints{};
    SwitchModel model[2] = {{0.10f, 0.07f}, {0.50f, 0.40f}};      // 0: fast, 1: filt
    std::deque<Flight> flight[2][2];                              // [switch][lane], in order per lane (a lane is one stream)
    long call = 0, probes = 0, reports = 0;
    int jitter = 3;                                               // the halves of a split call arrive up to jitter - 1 calls apart
    std::mt19937_64 rng;
    explicit Sim(uint64_t seed, unsigned seq0 = 0) : rng(seed) { rs.fast.seq = rs.filt.seq = seq0; }

    ContentSwitch &sw(int s) { return s == 0 ? rs.fast : rs.filt; }
    unsigned long long *words(int s) { return s == 0 ? hints.fast_density : hints.filter_density; }

    void deliver() {
        for (int s = 0; s < 2; ++s) {
            const int first = (int)(rng() & 1);                    // the two lane words in either order
            for (int q = 0; q < 2; ++q) {
                const int lane = first ^ q;
                std::deque<Flight> &f = flight[s][lane];
                while (!f.empty() && f.front().at <= call) {
                    words(s)[lane] = f.front().word;
                    f.pop_front();
                }
                if ((rng() & 7) == 0) words(s)[lane] = *(volatile unsigned long long *)&words(s)[lane];    // a rewrite of the same word
            }
        }
    }
    // what the rules say the words just read must do to the switch
    void check_observe(int s) {
        SwitchModel &m = model[s];
        const ContentSwitch &c = sw(s);
        float sum = 0.f;
        int fresh = 0;
        for (int lane = 0; lane < 2; ++lane) {
            const unsigned sq = (unsigned)(words(s)[lane] >> 32), bits = (unsigned)words(s)[lane];
            if (sq == 0 || sq == m.seen[lane]) continue;           // nothing reported / counted already
            m.seen[lane] = sq;
            float v;
            std::memcpy(&v, &bits, sizeof(v));
            sum += v;
            fresh++;
        }
        if (fresh) {
            m.last = sum / (float)fresh;                           // the halves of a split call: one observation
            if (!m.on && m.last > m.hi) { m.on = true; m.period = 16; }
            else if (m.on && m.last < m.lo) m.on = false;
            else if (m.on && m.pending && m.period < 64) {
                m.period *= 2;
                if (++m.doublings_this_probe > 1) VIOLATION("switch-doubling", "switch %d call %ld: one probe doubled the period twice", s, call);
            }
            m.pending = false;
        }
        if (c.on != m.on || c.period != m.period || c.pending != m.pending || c.last != m.last)
            VIOLATION("switch-observe", "switch %d call %ld: on %d period %d pending %d last %g, the rules give %d %d %d %g", s, call,
                      (int)c.on, c.period, (int)c.pending, (double)c.last, (int)m.on, m.period, (int)m.pending, (double)m.last);
        if (c.period != 16 && c.period != 32 && c.period != 64) VIOLATION("switch-period", "switch %d call %ld: period %d", s, call, c.period);
    }
    // One call of the engine: the reports that have arrived, the decision, the launches' sequence numbers, their reports.
    // halves: 1 = unsplit, 2 = split (lane 1 first); report_mask: which ranges of the call report on the default route.
    CallRoute step(const CallKind &kind, int halves, int report_mask, float content[2], int lag, int forced_fast, int exact_filter, int small_lane = 0) {
        deliver();
        const bool on_before[2] = {rs.fast.on, rs.filt.on};
        rs.read_hints(hints);
        for (int s = 0; s < 2; ++s) {
            check_observe(s);
            if (!on_before[s] && sw(s).on && !(sw(s).last > model[s].hi)) VIOLATION("switch-rule", "switch %d: on without an observation above hi", s);
            if (on_before[s] && !sw(s).on && !(sw(s).last < model[s].lo)) VIOLATION("switch-rule", "switch %d: off without an observation below lo", s);
        }
        const int cd_before[2] = {rs.fast.countdown, rs.filt.countdown};
        const bool pend_before[2] = {rs.fast.pending, rs.filt.pending};
        const CallRoute r = rs.decide_call(kind, forced_fast, exact_filter);
        const bool forced[2] = {forced_fast >= 0, exact_filter != 0}, eligible[2] = {kind.fast_reports, kind.filter_reports};
        const bool alt[2] = {r.fast_dense, !r.use_filter};
        if (forced[0] && r.fast_dense != (forced_fast == 1)) VIOLATION("switch-forced", "call %ld: forced form not taken", call);
        if (forced[1] && r.use_filter != (exact_filter > 0)) VIOLATION("switch-forced", "call %ld: forced route not taken", call);
        for (int s = 0; s < 2; ++s) {
            ContentSwitch &c = sw(s);
            if (forced[s] && (c.countdown != cd_before[s] || c.pending != pend_before[s]))
                VIOLATION("switch-forced", "switch %d call %ld: a forced choice moved the countdown", s, call);
            if (!forced[s] && !eligible[s] && (c.countdown != cd_before[s] || c.pending != pend_before[s]))
                VIOLATION("probe-spent", "switch %d call %ld: a call that cannot report counted down %d -> %d%s", s, call, cd_before[s], c.countdown,
                          c.pending && !pend_before[s] ? " and took the probe" : "");
            if (!forced[s] && !c.on && alt[s]) VIOLATION("switch-rule", "switch %d call %ld: the alternative while off", s, call);
            if (!forced[s] && eligible[s] && c.on && !alt[s]) {     // a probe
                probes++;
                model[s].probes++;
                model[s].doublings_this_probe = 0;
            }
            model[s].pending = c.pending;                          // (set by the decision step only; cleared by observations)
            // the launches: the default route of an eligible call reports, one sequence number per reporting range
            if (eligible[s] && !alt[s]) {
                for (int h = 0; h < halves; ++h) {
                    if (!(report_mask >> h & 1)) continue;
                    const int lane = halves == 2 ? 1 - h : small_lane;
                    const unsigned seq = c.next_seq();
                    if (seq == 0) VIOLATION("switch-seq", "switch %d call %ld: sequence number 0 handed out", s, call);
                    const float v = content[s] * (halves == 2 ? (h ? 1.03f : 0.97f) : 1.f);
                    unsigned bits;
                    std::memcpy(&bits, &v, sizeof(bits));
                    long at = call + 1 + lag + (halves == 2 ? (long)(rng() % (unsigned)jitter) : 0);
                    std::deque<Flight> &f = flight[s][lane];
                    if (!f.empty() && f.back().at > at) at = f.back().at;        // a lane delivers in order
                    f.push_back({at, ((unsigned long long)seq << 32) | bits});
                    reports++;
                }
            }
        }
        call++;
        return r;
    }
};

struct SwitchTotals { long calls = 0, probes = 0, reports = 0, cases = 0; };

// random calls of every kind, content wandering across the thresholds, forced choices in some runs
static void switch_rules_sweep(SwitchTotals &t) {
    for (int run = 0; run < 60; ++run) {
        Sim sim(1000 + run, run % 3 == 0 ? 0xfffffff0u + (unsigned)run % 8 : (unsigned)run);
        const int forced_fast = run % 10 == 7 ? 1 : (run % 10 == 8 ? 0 : -1), exact_filter = run % 10 == 5 ? 1 : (run % 10 == 6 ? -1 : 0);
        const int lag_max = run % 41;
        float content[2] = {0.05f, 0.2f};
        for (int i = 0; i < 4000; ++i) {
            if (sim.rng() % 97 == 0) content[0] = (float)(sim.rng() % 1000) / 1000.f * 0.3f;
            if (sim.rng() % 89 == 0) content[1] = (float)(sim.rng() % 1000) / 1000.f;
            const int k = (int)(sim.rng() % 4);
            CallKind kind{};
            kind.fast_reports = k == 0 && forced_fast < 0;           // (a forced form never reports: smx_plan.h plan_range)
            kind.filter_reports = k == 1;
            const int halves = sim.rng() % 3 == 0 ? 2 : 1;
            const int mask = halves == 2 ? 1 + (int)(sim.rng() % 3) : 1;
            sim.step(kind, halves, mask, content, (int)(sim.rng() % (unsigned)(lag_max + 1)), forced_fast, exact_filter, (int)(sim.rng() & 1));
        }
        t.calls += sim.call; t.probes += sim.probes; t.reports += sim.reports;
    }
}

// liveness: cycle[i] = 'E' (the call can report to the switch under test) or 'I' (it cannot)
static long liveness_case(int s, const std::string &cycle, int phase, int lag, int warm, SwitchTotals &t, long *worst) {
    Sim sim(7 * (uint64_t)warm + (uint64_t)lag, s == 0 ? 0xffffffc0u : 5u);
    sim.jitter = 1;                                               // (`lag` is exact here: the bound depends on it)
    float content[2] = {0.9f, 0.9f};
    size_t pos = (size_t)phase;
    auto call = [&]() {
        const bool e = cycle[pos++ % cycle.size()] == 'E';
        CallKind kind{};
        (s == 0 ? kind.fast_reports : kind.filter_reports) = e;
        if (!e && (sim.rng() & 1)) (s == 0 ? kind.filter_reports : kind.fast_reports) = true;     // a call of the other kind, or of neither
        const int halves = sim.rng() % 4 == 0 ? 2 : 1;
        sim.step(kind, halves, halves == 2 ? 3 : 1, content, lag, -1, 0, (int)(sim.rng() & 1));
        return e;
    };
    int guard = 0;
    while (!sim.sw(s).on && guard++ < 200) call();                // noise: the switch goes on
    for (int i = 0; i < warm; ++i) call();
    content[0] = 0.03f;                                           // smooth again, below both `lo`
    content[1] = 0.2f;
    long eligible = 0;
    const long bound = 64 + lag + 1;
    while (eligible <= bound + 200) {
        if (call()) eligible++;
        // (the call just made has read the hints: the switch's state is what that call saw)
        if (!sim.sw(s).on) break;
    }
    t.calls += sim.call; t.probes += sim.probes; t.reports += sim.reports; t.cases++;
    if (eligible > *worst) *worst = eligible;
    return eligible > bound ? eligible : 0;
}

static void liveness_sweep(SwitchTotals &t) {
    std::vector<std::string> cycles = {"E", "EI", "EIII", "EEI"};           // the table of the issue first
    const size_t table = cycles.size();
    std::mt19937_64 rng(99);
    for (int len = 2; len <= 16; ++len) {
        cycles.push_back("E" + std::string((size_t)len - 1, 'I'));
        for (int k = 0; k < 1; ++k) {
            std::string c((size_t)len, 'I');
            for (char &ch : c) ch = rng() % 2 ? 'E' : 'I';
            c[rng() % c.size()] = 'E';
            cycles.push_back(c);
        }
    }
    const int lags[] = {0, 1, 3, 10, 16, 17, 31, 40};
    const int warms[] = {0, 1, 3, 7, 15, 16, 31, 150};
    for (size_t ci = 0; ci < cycles.size(); ++ci) {
        long failed = 0, cases = 0, worst = 0;
        for (int s = 0; s < 2; ++s)
            for (int phase = 0; phase < (int)cycles[ci].size(); ++phase)
                for (int lag : lags)
                    for (int warm : warms) {
                        const long over = liveness_case(s, cycles[ci], phase, lag, warm, t, &worst);
                        cases++;
                        if (over) {
                            failed++;
                            VIOLATION("liveness", "switch %d cycle %s phase %d lag %d warm %d: still on after %ld eligible calls (bound %d)", s,
                                      cycles[ci].c_str(), phase, lag, warm, over > 64 + lag + 1 + 200 ? -1L : over, 64 + lag + 1);
                        }
                    }
        if (ci < table || failed)
            std::printf("liveness-cycle %s: %ld of %ld cases over the bound, worst %ld eligible calls\n", cycles[ci].c_str(), failed, cases, worst);
    }
}

int main() {
    LedgerTotals lt;
    ledger_sweep(lt);
    SwitchTotals st;
    switch_rules_sweep(st);
    liveness_sweep(st);
    for (const auto &kv : g_by_kind) std::printf("violations of kind %s: %ld\n", kv.first.c_str(), kv.second);
    std::printf("route-state entries %ld waits %ld fallbacks %ld steady_entries %ld calls %ld probes %ld reports %ld liveness_cases %ld violations %ld\n",
                lt.entries, lt.waits, lt.fallbacks, lt.steady, st.calls, st.probes, st.reports, st.cases, g_violations);
    return g_violations ? 1 : 0;
}
