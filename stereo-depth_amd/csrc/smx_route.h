// smx_route.h -- the host-side state machines of the engine's enqueue(): which launch plan a call takes (the two content
// switches and the grid hint) and when one stream lane has to wait for the other (the lane ledger).
//
// Plain C++: no HIP include and no HIP call, so that tests/route_state_harness.cpp can compile the very lines the engine
// runs as host code under a sanitizer and check them against a model.  smx_engine.hip owns the pinned memory, the streams
// and the events; everything here is arithmetic on host state.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace smx {

// Pinned host words the kernels write without any synchronisation (system-scope stores): hints for the NEXT calls'
// launch plans, never dependencies -- every plan gives the same bits, only the time differs.
struct HostHints {
    unsigned long long filter_density[2];   // per stream lane: (seq << 32) | float bits: candidate density of the last filtered launch
    unsigned long long grid;                // (epoch << 1) | pair 0 of that call was off the exact grid (k_refine_auto)
    unsigned long long fast_density[2];     // per stream lane: (seq << 32) | float bits: second-pass marches / first-pass marches of the last sparse fast launch
};

// A launch-plan choice between a default and an alternative route that follows what earlier calls' kernels reported through
// one HostHints word per stream lane.  Above `hi` the engine takes the alternative and probes the default route every
// `period` calls OF THE SWITCH'S OWN KIND -- calls whose default route has a launch that reports to it (CallKind) -- (16,
// doubling to 64 while the probes keep failing); below `lo` it comes back.  Calls of another kind and forced choices do
// not call decide(), so the countdown stands still and an armed probe is never spent on a call that cannot report;
// reports are observed all the same.
struct ContentSwitch {
    static constexpr int LANES = 2;               // one report word per stream lane (smx_engine::LANES)
    float hi, lo;
    bool on = false;                              // the alternative is the current choice
    int period = 16, countdown = 0;
    bool pending = false;                         // a probe call has been issued and its report has not been evaluated yet
    unsigned seq = 0, seen[LANES] = {0, 0};       // last sequence number handed to a launch / seen per lane
    float last = -1.f;                            // the last observation, -1: none yet

    // Takes the reports that have arrived by now (no synchronisation: whatever has arrived, has arrived).  The two halves
    // of a split call report separately: they are ONE observation.  Returns whether anything was fresh.
    bool observe(const unsigned long long (&words)[LANES]) {
        float sum = 0.f;
        int fresh = 0;
        for (int k = 0; k < LANES; ++k) {
            const unsigned long long w = *(const volatile unsigned long long *)&words[k];
            const unsigned sq = (unsigned)(w >> 32);
            if (sq == 0 || sq == seen[k]) continue;
            seen[k] = sq;
            const unsigned bits = (unsigned)(w & 0xffffffffull);
            float v;
            std::memcpy(&v, &bits, sizeof(v));
            sum += v;
            fresh++;
        }
        if (!fresh) return false;
        last = sum / (float)fresh;
        if (!on && last > hi) {
            on = true;
            period = 16;
            countdown = period;
        } else if (on && last < lo) {
            on = false;
        } else if (on && pending && period < 64) {   // a probe that failed: look again later (once per probe,
            period *= 2;                              // however many reports its halves send, whenever they arrive)
        }
        pending = false;
        return true;
    }
    // The route of a call of this switch's kind being enqueued: true = the alternative.  While `on`, every period-th such
    // call is a probe: it takes the default route, which reports what it found.
    bool decide() {
        if (!on) return false;
        if (--countdown > 0) return true;
        countdown = period;
        pending = true;
        return false;
    }
    // Sequence number for the next reporting launch (0 means "nothing reported").
    unsigned next_seq() {
        if (++seq == 0) seq = 1;
        return seq;
    }
};

// What enqueue() knows about a call before it decides: whether the call, on the switch's DEFAULT route, would enqueue a
// launch that reports to that switch (computed once per call from the launch plans of its range(s): both halves of a
// split call take the same decision).
struct CallKind {
    bool fast_reports;        // the sparse form of the fast kernel would run and publish hints->fast_density
    bool filter_reports;      // the filtered exact-order route would run and publish hints->filter_density
};

// The decision for one call.
struct CallRoute {
    bool fast_dense;          // the dense form of the fast kernel
    bool use_filter;          // the filtered exact-order route
    int grid_hint;            // f32 gray, few pairs: the last reported call was on (0) / off (1) the exact grid; -1: no report yet
};

// The content-dependent launch-plan state of one engine and its per-call decision step.
struct RouteState {
    // Content-aware route of off-grid (RGB) batches.  The filtered route pays a fixed filter pass to evaluate fewer
    // disparities in exact order; on real scenes (flat cost curves in untextured and occluded regions) the candidate
    // sets cover most of the range and the dense kernel alone is faster.  The sparse kernel reports the density of
    // every filtered launch (hints->filter_density); filt.on: the dense route.
    // Break-even density, measured (profiles/r03_rgb_routes.txt, 32 pairs per call): the filter's two passes cost 0.89-0.93 ms,
    // the sparse kernel 0.19 ms + 1.1 x density x the dense kernel's 2.24-2.7 ms: the routes tie at a density of 0.45 (C5,
    // 96 disparities) to 0.56 (the reference's pair at its calibrated range, which reports 0.65 and loses 12 % filtered).
    ContentSwitch filt{0.50f, 0.40f};             // hi, lo
    // Form of the fast kernel by content: the sparse form reports which share of the disparities its second pass revisited
    // (hints->fast_density; banded surfaces 0.05, scene-like 0.17, real texture / noise ~1); fast.on: the dense form.
    // Measured per 64 C2 pairs (tools/content_breakdown.py, SMX_DEBUG_HINTS=1): the sparse form takes 0.68 ms at a ratio of 0.047
    // (banded surfaces), 0.85 at 0.166 (scene-like ramp) and 1.20 at 0.97 (noise) -- the first marches of the second pass are the
    // expensive ones, they deliver to many rows -- the dense form 0.80 ms whatever the content: the curves cross near 0.13.
    // (The latency shape's curves cross lower -- its dense form costs a banded C2 frame 0.3 us and saves a scene-like one 8 -- and
    // its windows are 12 rows, not 27: the same ramp reports 0.133 there.  One pair of thresholds a little below the crossing.)
    ContentSwitch fast{0.10f, 0.07f};             // hi, lo
    int grid_hint = -1;

    // Reads the hint words the kernels of earlier calls have published by now into the state the launch plans of the next
    // call follow: the two content switches and the grid hint.  Returns whether the fast kernel's report was fresh.
    bool read_hints(const HostHints &h) {
        filt.observe(h.filter_density);
        const bool fresh = fast.observe(h.fast_density);
        const unsigned long long g = *(const volatile unsigned long long *)&h.grid;
        grid_hint = g == 0ull ? -1 : (int)(g & 1ull);      // (the word carries the call counter, which starts at 1: 0 = nothing reported)
        return fresh;
    }

    // The decision step of one call, after read_hints.  forced_fast_dense: SMX_FAST_DENSE (1 / 0: always / never, -1: by
    // content); exact_filter: smx_config (1 / -1: always / never filtered, 0: by content).
    // (a forced choice -- SMX_FAST_DENSE, exact_filter = 1 / -1 -- leaves its switch's countdown alone)
    // A call that cannot report to a switch follows the switch's current choice and leaves its countdown alone as well: a
    // probe spent on such a call brings no report, and a call pattern whose period divides the probe period (one gray and
    // one RGB batch per frame, batches and single frames alternately) would put EVERY probe on the wrong kind of call --
    // the switch then never comes back from its alternative (tests/route_state_harness.cpp: liveness).
    CallRoute decide_call(const CallKind &kind, int forced_fast_dense, int exact_filter) {
        CallRoute r{};
        r.fast_dense = forced_fast_dense >= 0 ? forced_fast_dense == 1 : (kind.fast_reports ? fast.decide() : fast.on);
        r.use_filter = exact_filter == 0 ? !(kind.filter_reports ? filt.decide() : filt.on) : exact_filter > 0;
        r.grid_hint = grid_hint;
        return r;
    }
};

// What the two stream lanes have in flight that the other lane has not been ordered behind yet.  The lanes run unordered
// against each other, which is safe only while they work on disjoint pair slots of the engine's buffers and write disjoint
// output bytes; enter() says when the entering lane has to wait for the other lane's tail first.
struct LaneLedger {
    static constexpr int LANES = 2;
    int hull_lo[LANES] = {}, hull_hi[LANES] = {}; // pairs [lo, hi) lane k has worked on since the other lane last waited for it
    // ... and the caller's output bytes lane k has written since then: two calls whose `out` ranges overlap are ordered
    // (the later call wins, as on one stream), everything else runs side by side.  Disjoint ranges are kept apart (a
    // hull would make a ring of output buffers look like one range); more than OUT_RANGES_MAX of them synchronise the lanes.
    struct OutRange { uintptr_t lo, hi; };
    static constexpr size_t OUT_RANGES_MAX = 32;
    std::vector<OutRange> out_live[LANES];

    // Lane k is about to work on pair slots [lo, hi) and to write the output bytes [olo, ohi).  Returns whether lane k has
    // to wait for the tail of the other lane first (the caller records / waits; the other lane's entries are forgotten:
    // all of its work so far is then ordered before lane k's next), and remembers what lane k now has in flight.
    bool enter(int k, int lo, int hi, uintptr_t olo, uintptr_t ohi) {
        const int o = 1 - k;
        bool clash = hull_hi[o] > hull_lo[o] && lo < hull_hi[o] && hull_lo[o] < hi;
        for (const OutRange &r : out_live[o]) clash = clash || (olo < r.hi && r.lo < ohi);
        if (clash) {
            hull_lo[o] = hull_hi[o] = 0;          // all of lane o's work so far is now ordered before lane k's next
            out_live[o].clear();
        }
        if (hull_hi[k] > hull_lo[k]) { lo = lo < hull_lo[k] ? lo : hull_lo[k]; hi = hi > hull_hi[k] ? hi : hull_hi[k]; }
        hull_lo[k] = lo;
        hull_hi[k] = hi;
        // remember the output range (merged with the ranges of this lane it touches)
        OutRange mine{olo, ohi};
        std::vector<OutRange> &live = out_live[k];
        for (size_t i = 0; i < live.size();) {
            if (mine.lo <= live[i].hi && live[i].lo <= mine.hi) {
                mine.lo = mine.lo < live[i].lo ? mine.lo : live[i].lo;
                mine.hi = mine.hi > live[i].hi ? mine.hi : live[i].hi;
                live[i] = live.back();
                live.pop_back();
                i = 0;                                   // the grown range may now touch an earlier one
            } else {
                ++i;
            }
        }
        if (live.size() >= OUT_RANGES_MAX) {
            // too many disjoint outputs to keep apart: fall back to their hull (a superset: at worst a wait too many)
            for (const OutRange &r : live) {
                mine.lo = mine.lo < r.lo ? mine.lo : r.lo;
                mine.hi = mine.hi > r.hi ? mine.hi : r.hi;
            }
            live.clear();
        }
        live.push_back(mine);
        return clash;
    }
};

}  // namespace smx
