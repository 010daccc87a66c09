"""The engine's content switches, grid hint and stream lanes under interleaving (include/stereo_mi355x.h: stream lanes,
smx_route_info; stereo-depth_amd/csrc/smx_route.h).

tests/test_gpu_engine_rules.py drives every one of these pieces of host state in isolation: one switch at a time, one kind
of call per test, a host synchronisation after almost every call.  Here every kind of call -- gray f32 on and off the
grid, u8, RGB f32 / u8, LR; 1 .. 96 pairs; a caller's stream, a side stream or the lanes -- is mixed on ONE engine while
the content changes and the kernels' reports are still in flight, and two and four host threads drive an engine each.
Every comparison is bitwise against the oracle (multi_block_matching_cost_aggregation.cu:54-88,
wta_disparity_selection.cu:22-30, secondary_matching.cu:24-71 and the fills); the routes only ever change the time.

State is asserted only after a segment's synchronisation: how far the host runs ahead of the device inside a segment is
not knowable, so nothing inside one depends on when a report arrives.  (The host-side rules themselves -- ledger sizes and
waits, probe countdowns -- are the business of tests/test_route_state_cpu.py; no ABI exposes them.)"""
import collections
import ctypes as C
import gc
import threading
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import stereo_synthetic as syn                      # noqa: E402
from lr_ref import lr_rule                          # noqa: E402
from oracle_lib import OracleConfig                 # noqa: E402


@pytest.fixture(scope="module")
def cd():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import cuda_depth
    return cuda_depth


SIZES = (1, 2, 3, 4, 8, 15, 16, 17, 31, 48, 96)
OFF = np.float32(0.3)                               # off the exact grid, and not integer-valued (float step 6)


def _flip(a):
    return np.ascontiguousarray(a[..., ::-1])


class Pool:
    """A cyclic pool of distinct pairs of one entry on the device, with the oracle's maps: a call takes `n` consecutive
    pairs from an offset of its own, so calls differ in their inputs while the oracle runs once per distinct pair."""

    def __init__(self, name, entry, pairs, expected, length):
        self.name, self.entry, self.period = name, entry, len(pairs)
        idx = [i % len(pairs) for i in range(length)]
        dt = np.uint8 if entry.endswith("u8") else np.float32
        self.L = torch.from_numpy(np.stack([pairs[i][0] for i in idx]).astype(dt)).cuda()
        self.R = torch.from_numpy(np.stack([pairs[i][1] for i in idx]).astype(dt)).cuda()
        self.E = torch.from_numpy(np.stack([expected[i] for i in idx])).cuda()
        self.gray = entry.startswith("gray")


class Driver:
    """One engine, its trace and the bookkeeping of who wrote which output slot last."""

    def __init__(self, cd, sm, H, W):
        self.cd, self.sm, self.H, self.W = cd, sm, H, W
        self.main = torch.cuda.current_stream()
        self.side = torch.cuda.Stream()
        self.last_caller = None
        self.trace = []                      # one dict per call (and per segment end): the call and route_info() after it
        self.counts = collections.Counter()
        self.calls = 0
        self.seg = None

    # ---- segments
    def begin(self, name, slots):
        self.seg = name
        self.arena = torch.zeros((slots, self.H, self.W), device="cuda")
        self.writers = []                    # (slot, n, pool, offset, call number) in call order
        self.bump = 0
        self.extra = []                      # (tensor, expected numpy, label): outputs outside the arena (LR)
        self.eligible = collections.Counter()
        torch.cuda.synchronize()             # the arena is zeroed before any lane writes into it

    def slot_for(self, n, rng, reuse=0.15):
        if self.writers and (self.bump + n > self.arena.shape[0] or rng.random() < reuse):
            fit = [w[0] for w in self.writers if w[0] + n <= self.arena.shape[0]]
            if fit:
                return fit[int(rng.integers(len(fit)))]                        # an earlier call's output: the later call wins
        assert self.bump + n <= self.arena.shape[0], "test bug: the segment's output arena is too small"
        s = self.bump
        self.bump += n
        return s

    def call(self, pool, off, n, where, slot, single=False):
        sm = self.sm
        l, r, out = pool.L[off:off + n], pool.R[off:off + n], self.arena[slot:slot + n]
        assert l.shape[0] == n and out.shape[0] == n, "test bug: pool or arena too short"
        if where == "lanes":
            sm.compute_disparity_map_batch(l, r, out=out, engine_streams=True)
        else:
            s = self.main if where == "cur" else self.side
            if self.last_caller is not None and self.last_caller is not s:
                s.wait_stream(self.last_caller)          # calls on one engine are serialised by the caller: stream order, no host wait
            self.last_caller = s
            with torch.cuda.stream(s):
                if single:                               # the single-frame entries return the engine's persistent output
                    assert n == 1
                    fn = sm.compute_disparity_map_gray if pool.gray else sm.compute_disparity_map
                    out[0].copy_(fn(l[0], r[0]))
                else:
                    sm.compute_disparity_map_batch(l, r, out=out)
        self.writers.append((slot, n, pool, off, self.calls))
        self._record(pool.name, pool.entry, n, where, single)
        g = sm.match_geometry(n)
        window = g["kernel"] == "fast_window"
        if pool.gray and (window or g["band_rows"] == 12):
            self.eligible["fast"] += 1
        if not pool.gray and window:
            self.eligible["filter"] += 1

    def lr_call(self, pool, off, n, expected):
        out = torch.zeros((n, self.H, self.W), device="cuda")
        s = self.main
        if self.last_caller is not None and self.last_caller is not s:
            s.wait_stream(self.last_caller)
        self.last_caller = s
        self.sm.compute_disparity_map_batch_lr(pool.L[off:off + n], pool.R[off:off + n], out=out)
        self.extra.append((out, expected, "LR call"))
        self._record(pool.name, "lr_" + pool.entry, n, "cur", False)

    def _record(self, name, entry, n, where, single):
        info = self.sm.route_info()                      # a host read of what has arrived, not a synchronisation
        self.trace.append(dict(seg=self.seg, call=self.calls, pool=name, entry=entry, n=n, where=where, single=single, **info))
        self.counts[(entry, where, "single" if single else "batch")] += 1
        self.counts[("pool", name)] += 1
        self.calls += 1

    def end(self):
        """join, ONE synchronisation, every output of the segment against the oracle, the state after it."""
        self.sm.join()
        torch.cuda.synchronize()
        last = {}
        for slot, n, pool, off, k in self.writers:       # later calls overwrite earlier ones
            for i in range(n):
                last[slot + i] = (pool, off + i, k)
        by_pool = collections.defaultdict(list)
        for slot, (pool, idx, k) in last.items():
            by_pool[pool].append((slot, idx, k))
        for pool, items in by_pool.items():
            for c in range(0, len(items), 256):
                chunk = items[c:c + 256]
                slots = torch.tensor([s for s, _, _ in chunk], device="cuda")
                idx = torch.tensor([i for _, i, _ in chunk], device="cuda")
                same = (self.arena[slots] == pool.E[idx]).flatten(1).all(dim=1).cpu().numpy()
                if not same.all():
                    bad = [(chunk[j][2], chunk[j][0]) for j in np.nonzero(~same)[0][:8]]
                    calls = {k: self.trace_of(k) for k, _ in bad}
                    raise AssertionError(f"segment {self.seg}: outputs differ from the oracle (call, slot): {bad}; calls: {calls}")
        for out, expected, label in self.extra:
            assert np.array_equal(out.cpu().numpy(), expected), f"segment {self.seg}: {label}"
        info = self.sm.route_info()
        self.trace.append(dict(seg=self.seg, call=None, pool="(after the synchronisation)", entry="", n=0, where="", single=False, **info))
        del self.arena
        return info

    def trace_of(self, k):
        t = next(t for t in self.trace if t["call"] == k)
        return {key: t[key] for key in ("seg", "pool", "entry", "n", "where", "single", "route_dense", "fast_dense", "offgrid_hint")}

    def transitions(self, key):
        seq = []
        for t in self.trace:
            if not seq or seq[-1] != t[key]:
                seq.append(t[key])
        return seq


def _contains_in_order(seq, want):
    it = iter(seq)
    return all(any(x == w for x in it) for w in want)


def test_every_kind_of_call_on_one_engine_while_the_content_changes(cd, oracle_omp):
    """One engine (150 x 700, K = 2, 64 disparities, max_batch 96, lanes split from 16 pairs, default exact_filter), a
    seeded schedule of segments of back-to-back calls with no host synchronisation inside; after each segment one
    synchronisation, every output against the oracle (for shared output memory: the later call's), then the state:

      smooth        smooth gray and structured RGB, every kind and size, an LR call between lane calls -> both switches off
      noise         noise of every kind mixed with small calls                                          -> both on
      flip          noise, then (in the middle of the segment) 65 smooth gray and 65 structured RGB batches strictly
                    alternating: probes and their reports straddle the flip                             -> both off again
      flip-single   the same with the cycle gray batch, single gray frame, RGB batch, single RGB frame   -> both off again
      probes        noise, both on, 40 eligible calls of each kind: the first probe fails               -> probe_period > 16
      grid          single f32 gray frames on / off the grid between batches and one-launch AUTO calls of 2 - 4 mixed
                    pairs on the lanes                                                                  -> offgrid_hint 0, then 1
      ring          84 one-pair lane calls into every other slot of one tensor without a join (each lane passes 32 live
                    output ranges: the ledger falls back to their hull), then a heavy RGB call into slots inside the hull,
                    a light gray call into one of the same slots (it must win) and a call into a never-written gap

    A switch that counted every call down, whatever its kind, put every probe of one of the two switches on the other
    kind's calls in the flip segments (their cycles divide the probe period): with that logic the flip segment ended with
    fast_dense still 1 on an MI355X."""
    H, W, K, D, B = 150, 700, 2, 64, 96
    cfg = cd.StereoMatchingConfiguration(height=H, width=W, downscale_factor=K, min_disparity=0, max_disparity=D - 1)
    ocfg = OracleConfig(height=H, width=W, downscale_factor=K, min_disparity=0, max_disparity=D - 1)
    t_start = time.time()

    # ---- content: a handful of distinct pairs per kind; the oracle runs once per distinct (entry, pair)
    smooth = []
    for i in range(3):                                   # one fronto-parallel surface per pair
        l = syn.make_pair(H, W, D, K, 40 + i)[0]
        smooth.append((l, np.roll(l, -K * (5 + 9 * i), axis=1).copy()))
    noise = [syn.make_noise_pair(H, W, 30 + i) for i in range(3)]
    struct = [syn.random_rgb_pair(H, W, D, K, 80 + i) for i in range(3)]
    rng = np.random.default_rng(9)
    cnoise = [(rng.integers(0, 256, (3, H, W)).astype(np.float32), rng.integers(0, 256, (3, H, W)).astype(np.float32)) for _ in range(2)]
    off = lambda p: ((p[0] + OFF).astype(np.float32), p[1])          # noqa: E731
    mixed = [smooth[0], off(smooth[0]), smooth[1], off(smooth[1])]   # pair 0 of a call on the grid at even offsets
    mixed_noise = [noise[0], off(noise[0])]
    offgrid = [off(smooth[0]), off(smooth[1])]
    oracle_runs = [0]

    def run(pairs):
        oracle_runs[0] += len(pairs)
        return [oracle_omp.run(ocfg, np.ascontiguousarray(l, np.float32), np.ascontiguousarray(r, np.float32)) for l, r in pairs]

    e_smooth, e_noise, e_struct, e_cnoise = run(smooth), run(noise), run(struct), run(cnoise)
    e_off = run(offgrid)
    e_mixed = [e_smooth[0], e_off[0], e_smooth[1], e_off[1]]
    e_mixed_noise = [e_noise[0]] + run([mixed_noise[1]])
    for p in smooth + noise + struct + cnoise:           # the u8 entries see the same values: one oracle map serves both
        assert all(np.array_equal(x, np.rint(x)) and x.min() >= 0 and x.max() <= 255 for x in p)
    P = {
        "g_smooth": Pool("g_smooth", "gray_f32", smooth, e_smooth, B + 3), "g_noise": Pool("g_noise", "gray_f32", noise, e_noise, B + 3),
        "u_smooth": Pool("u_smooth", "gray_u8", smooth, e_smooth, B + 3), "u_noise": Pool("u_noise", "gray_u8", noise, e_noise, B + 3),
        "g_mixed": Pool("g_mixed", "gray_f32", mixed, e_mixed, 8), "g_mixed_noise": Pool("g_mixed_noise", "gray_f32", mixed_noise, e_mixed_noise, 6),
        "g_off": Pool("g_off", "gray_f32", offgrid, e_off, 6),
        "c_struct": Pool("c_struct", "rgb_f32", struct, e_struct, B + 3), "c_noise": Pool("c_noise", "rgb_f32", cnoise, e_cnoise, B + 2),
        "c8_struct": Pool("c8_struct", "rgb_u8", struct, e_struct, B + 3), "c8_noise": Pool("c8_noise", "rgb_u8", cnoise, e_cnoise, B + 2),
    }
    # the LR call: (L_i, R_i) and the mirrored problem through the oracle, then the rule of tests/lr_ref.py
    lr_n = 2
    mirrored = run([(_flip(smooth[i][1]), _flip(smooth[i][0])) for i in range(lr_n)])
    lr_expected = np.stack([lr_rule(e_smooth[i], _flip(mirrored[i])) for i in range(lr_n)])
    torch.cuda.synchronize()                             # engine-stream calls need complete inputs
    t_oracle = time.time() - t_start

    sm = cd.StereoMatching(cfg, max_batch=B, overlap_min_pairs=16)
    # ---- preamble (synchronising): these sizes still reach the routes this test is about
    info = sm.route_info()
    assert info["filter_available"] == 1 and info["route_dense"] == 0 and info["fast_dense"] == 0 and info["offgrid_hint"] == -1, info
    g48, g3, g1 = sm.match_geometry(48), sm.match_geometry(3), sm.match_geometry(1)
    assert g48["kernel"] == "fast_window", f"48 pairs on a caller's stream no longer take the throughput shape: {g48}"
    assert g3["kernel"] == "fast_split" and g3["band_rows"] == 12, f"3 pairs no longer take the latency shape at 12-row bands: {g3}"
    assert g1["kernel"] == "fast_split" and g1["band_rows"] != 12, g1
    assert sm.overlap_lanes(96) == 2 and sm.overlap_lanes(16) == 2 and sm.overlap_lanes(15) == 1
    sm.profile_begin(1)
    out = sm.compute_disparity_map_batch(P["c_struct"].L[:48], P["c_struct"].R[:48])
    prof = sm.profile_end()
    assert prof["match_fast"][1] == 1, f"48 RGB pairs on a caller's stream no longer reach the filtered route: {prof}"
    assert torch.equal(out, P["c_struct"].E[:48])
    sm.profile_begin(1)
    out = sm.compute_disparity_map_batch(P["c_struct"].L[:96], P["c_struct"].R[:96], engine_streams=True)
    sm.join()
    prof = sm.profile_end()
    assert prof["match_fast"][1] == 2, f"the halves of 96 RGB pairs on the lanes no longer reach the filtered route: {prof}"
    assert sm.match_geometry(96)["kernel"] == "fast_window"
    torch.cuda.synchronize()
    assert torch.equal(out, P["c_struct"].E[:96])
    assert 0.0 < sm.route_info()["candidate_density"] < 0.40, sm.route_info()
    assert torch.equal(sm.compute_disparity_map_gray(P["g_smooth"].L[0], P["g_smooth"].R[0]), P["g_smooth"].E[0])
    torch.cuda.synchronize()
    assert sm.route_info()["offgrid_hint"] == 0
    sm.profile_begin(1)
    out = sm.compute_disparity_map_batch(P["g_mixed"].L[:3], P["g_mixed"].R[:3])
    prof = sm.profile_end()
    assert prof["match_exact"][1] == 0 and prof["match_fast"][1] == 1, f"3 mixed pairs no longer take the one-launch AUTO kernel: {prof}"
    assert torch.equal(out, P["g_mixed"].E[:3])
    info = sm.route_info()
    assert info["route_dense"] == 0 and info["fast_dense"] == 0, info

    d = Driver(cd, sm, H, W)
    rng = np.random.default_rng(20240917)
    WHERE = ("lanes", "cur", "side")

    def pick_where():
        return WHERE[int(rng.choice(3, p=(0.5, 0.3, 0.2)))]

    def random_call(content):
        """Any kind, size, stream and output."""
        kind = int(rng.choice(6, p=(0.22, 0.18, 0.16, 0.22, 0.14, 0.08)))
        where = pick_where()
        n = int(rng.choice(SIZES))
        if kind == 0:
            pool = P["g_smooth" if content == "smooth" else "g_noise"]
        elif kind == 1:
            pool = P["u_smooth" if content == "smooth" else "u_noise"]
        elif kind == 2:                                  # 2 - 4 pairs of which some are off the grid
            pool, n = P["g_mixed" if content == "smooth" else "g_mixed_noise"], int(rng.integers(2, 5))
        elif kind == 3:
            pool = P["c_struct" if content == "smooth" else "c_noise"]
        elif kind == 4:
            pool = P["c8_struct" if content == "smooth" else "c8_noise"]
        else:                                            # off-grid gray, a few pairs
            pool, n = (P["g_off"], int(rng.integers(1, 5))) if content == "smooth" else (P["g_mixed_noise"], int(rng.integers(1, 5)))
        o = int(rng.integers(0, pool.L.shape[0] - n + 1))
        single = n == 1 and where != "lanes" and rng.random() < 0.5
        d.call(pool, o, n, where, d.slot_for(n, rng), single)

    def eligible_call(pool, reuse=0.0):
        """A batch that can report to its switch: the throughput shape on a caller's stream or in both halves on the lanes."""
        n, where = ((48, "cur"), (48, "side"), (48, "lanes"), (96, "lanes"))[int(rng.choice(4, p=(0.35, 0.15, 0.35, 0.15)))]
        d.call(pool, int(rng.integers(0, pool.L.shape[0] - n + 1)), n, where, d.slot_for(n, rng, reuse))

    def single_frame(pool):
        where = pick_where()
        d.call(pool, int(rng.integers(0, pool.L.shape[0])), 1, where, d.slot_for(1, rng), where != "lanes" and rng.random() < 0.5)

    # ---- smooth: both switches stay off
    d.begin("smooth", 2600)
    eligible_call(P["g_smooth"])
    eligible_call(P["c_struct"])
    for k in range(44):
        random_call("smooth")
        if k == 20:                                      # an LR call between lane calls
            d.call(P["g_smooth"], 1, 8, "lanes", d.slot_for(8, rng, 0))
            d.lr_call(P["g_smooth"], 0, lr_n, lr_expected)
            d.call(P["u_smooth"], 2, 17, "lanes", d.slot_for(17, rng, 0))
    info = d.end()
    assert info["route_dense"] == 0 and info["fast_dense"] == 0, ("smooth", info)

    # ---- noise: both go on
    def noise_segment(name, calls):
        d.begin(name, 2600)
        eligible_call(P["g_noise"])
        eligible_call(P["c_noise"])
        for _ in range(calls):
            random_call("noise")
        eligible_call(P["u_noise"])
        eligible_call(P["c8_noise"])
        info = d.end()
        assert d.eligible["fast"] >= 2 and d.eligible["filter"] >= 2, d.eligible
        assert info["route_dense"] == 1 and info["fast_dense"] == 1 and info["candidate_density"] > 0.5, (name, info)

    noise_segment("noise", 30)

    # ---- the content flips in the middle of a segment, both switches on; gray, RGB, gray, RGB ...
    d.begin("flip", 3000)
    for _ in range(8):
        random_call("noise")
    before = dict(d.eligible)
    for i in range(65):
        eligible_call(P["g_smooth" if i % 3 else "u_smooth"], reuse=0.5)
        eligible_call(P["c_struct" if i % 3 else "c8_struct"], reuse=0.5)
    assert d.eligible["fast"] - before.get("fast", 0) >= 65 and d.eligible["filter"] - before.get("filter", 0) >= 65, d.eligible
    info = d.end()
    assert info["route_dense"] == 0 and info["fast_dense"] == 0, ("after 65 eligible calls of each kind on smooth content", info)

    # ---- ... and with the cycle batch, single frame, batch, single frame
    noise_segment("noise-2", 6)
    d.begin("flip-single", 3000)
    for _ in range(6):
        random_call("noise")
    before = dict(d.eligible)
    for i in range(65):
        eligible_call(P["g_smooth"], reuse=0.5)
        single_frame(P["g_smooth"] if i % 2 else P["u_smooth"])
        eligible_call(P["c_struct"], reuse=0.5)
        single_frame(P["c_struct"] if i % 2 else P["c8_struct"])
    assert d.eligible["fast"] - before.get("fast", 0) == 65 and d.eligible["filter"] - before.get("filter", 0) == 65, d.eligible
    info = d.end()
    assert info["route_dense"] == 0 and info["fast_dense"] == 0, ("batch, single frame, batch, single frame on smooth content", info)

    # ---- noise with both switches on: the first probe (the 16th eligible call at the latest) fails and the period grows
    noise_segment("noise-3", 6)
    assert d.trace[-1]["probe_period"] == 16
    d.begin("probes", 3000)
    for i in range(40):
        eligible_call(P["g_noise"], reuse=0.5)
        eligible_call(P["c_noise"], reuse=0.5)
        if i % 5 == 0:
            random_call("noise")
    assert d.eligible["fast"] >= 40 and d.eligible["filter"] >= 40, d.eligible
    info = d.end()
    assert info["route_dense"] == 1 and info["fast_dense"] == 1 and info["probe_period"] > 16, ("a failed probe doubles the period", info)

    # ---- the grid hint: single f32 gray frames on / off the grid between batches and one-launch AUTO calls on the lanes
    d.begin("grid-on", 400)
    for k in range(24):
        r = k % 6
        if r == 0:
            d.call(P["g_off"], int(rng.integers(0, 6)), 1, "cur" if k % 12 else "side", d.slot_for(1, rng), True)
        elif r == 1:
            d.call(P["g_smooth"], int(rng.integers(0, 40)), 31, "lanes", d.slot_for(31, rng))
        elif r == 2:
            d.call(P["g_mixed"], 2 * int(rng.integers(0, 3)), int(rng.integers(2, 5)), "lanes", d.slot_for(4, rng, 0))
        elif r == 3:
            single_frame(P["g_smooth"])
        elif r == 4:
            d.call(P["u_smooth"], 0, 16, "lanes", d.slot_for(16, rng))
        else:
            d.call(P["g_mixed"], 1, 3, "lanes", d.slot_for(3, rng, 0))           # pair 0 off the grid
    for _ in range(3):                                   # the last reports: on the grid (a caller's stream: behind every lane call)
        d.call(P["g_smooth"], int(rng.integers(0, 9)), 1, "cur", d.slot_for(1, rng, 0), True)
    info = d.end()
    assert info["offgrid_hint"] == 0, ("grid-on", info)
    d.begin("grid-off", 400)
    for k in range(18):                                  # the host knows "on the grid" now: 2 - 4 mixed pairs take ONE launch
        r = k % 3
        if r == 0:
            d.call(P["g_mixed"], 2 * int(rng.integers(0, 3)), int(rng.integers(2, 5)), "lanes", d.slot_for(4, rng, 0))
        elif r == 1:
            d.call(P["c_struct"], int(rng.integers(0, 9)), 15, "lanes", d.slot_for(15, rng))
        else:
            d.call(P["g_smooth"], int(rng.integers(0, 9)), 1, "lanes", d.slot_for(1, rng))
    for _ in range(3):
        d.call(P["g_off"], int(rng.integers(0, 6)), 1, "cur", d.slot_for(1, rng, 0), True)
    info = d.end()
    assert info["offgrid_hint"] == 1, ("grid-off", info)

    # ---- more live output ranges than the ledger keeps apart, no join
    d.begin("ring", 200)
    for i in range(84):                                  # every other slot: the ranges neither touch nor merge
        d.call(P["g_smooth"] if i % 4 else P["g_noise"], i % 7, 1, "lanes", 2 * i)
    d.call(P["c_noise"], 0, 3, "lanes", 10)              # heavy, into slots 10 .. 12 inside the hull (11 was a gap)
    d.call(P["g_smooth"], 5, 1, "lanes", 11)             # light, one of the same slots: the later call must win
    d.call(P["u_noise"], 3, 1, "lanes", 169)             # a never-written gap
    d.call(P["g_smooth"], 6, 2, "lanes", 20)             # ... and across a written slot, a gap and the next slot's edge
    d.end()

    # ---- the whole trace
    rd, fd, hint, period = d.transitions("route_dense"), d.transitions("fast_dense"), d.transitions("offgrid_hint"), d.transitions("probe_period")
    per = collections.Counter()
    for key, v in d.counts.items():
        if key[0] != "pool":
            per[" ".join(key)] += v
    print(f"\ninterleaved trace: {d.calls} engine calls, {oracle_runs[0]} oracle runs ({t_oracle:.1f} s), {time.time() - t_start:.1f} s in all")
    print("  calls per entry, stream and form: " + ", ".join(f"{k}: {v}" for k, v in sorted(per.items())))
    print("  calls per content pool: " + ", ".join(f"{k[1]}: {v}" for k, v in sorted(d.counts.items()) if k[0] == "pool"))
    print(f"  route_dense {rd}\n  fast_dense {fd}\n  offgrid_hint {hint}\n  probe_period {period}")
    assert d.calls >= 200
    assert _contains_in_order(rd, [0, 1, 0]) and _contains_in_order(fd, [0, 1, 0]), (rd, fd)
    assert 0 in hint and 1 in hint, hint
    for entry in ("gray_f32", "gray_u8", "rgb_f32", "rgb_u8", "lr_gray_f32"):
        assert any(k[0] == entry for k in d.counts), entry
    for where in WHERE:
        assert any(len(k) == 3 and k[1] == where for k in d.counts), where


# ----------------------------------------------------------------------------- host threads
SHAPES = ((64, 200, 2, 32), (96, 320, 2, 48), (150, 700, 2, 64), (80, 256, 1, 32))


class Worker:
    """One host thread: an engine of its own shape, its own stream, inputs and outputs."""

    def __init__(self, cd, oracle, index, calls=40):
        H, W, K, D = SHAPES[index % len(SHAPES)]
        self.H, self.W, self.index, self.calls = H, W, index, calls
        self.cfg = cd.StereoMatchingConfiguration(height=H, width=W, downscale_factor=K, min_disparity=0, max_disparity=D - 1)
        ocfg = OracleConfig(height=H, width=W, downscale_factor=K, min_disparity=0, max_disparity=D - 1)
        gray = [syn.make_pair(H, W, D, K, 500 + 10 * index + i)[:2] for i in range(3)]
        rgb = [syn.random_rgb_pair(H, W, D, K, 600 + 10 * index + i) for i in range(2)]
        self.g = Pool(f"t{index}_gray", "gray_f32", gray, [oracle.run(ocfg, l, r) for l, r in gray], 11)
        self.c = Pool(f"t{index}_rgb", "rgb_f32", rgb, [oracle.run(ocfg, l, r) for l, r in rgb], 10)
        self.engine = cd.StereoMatching(self.cfg, max_batch=8, overlap_min_pairs=4)
        self.stream = torch.cuda.Stream()
        self.plan = []
        for k in range(calls):
            n = (1, 2, 4, 8, 3)[k % 5]
            pool = self.c if k % 3 == 2 else self.g
            self.plan.append((pool, k % 3, n, k % 2 == 0, torch.zeros((n, H, W), device="cuda")))
        self.error = None
        self.short_lived = []
        self.short_out = [torch.zeros((1, H, W), device="cuda") for _ in range(20)]

    def run(self, cd, barrier, short_lived=0):
        try:
            barrier.wait(timeout=60)
            with torch.cuda.stream(self.stream):
                for k, (pool, off, n, lanes, out) in enumerate(self.plan):
                    self.engine.compute_disparity_map_batch(pool.L[off:off + n], pool.R[off:off + n], out=out, engine_streams=lanes)
                    if short_lived and k % 2 == 0 and len(self.short_lived) < short_lived:
                        # create, use once, drop: smx_create / the LDS caps / the lane-stream pool / smx_destroy beside
                        # the other threads' enqueues
                        e = cd.StereoMatching(self.cfg, max_batch=2)
                        j = len(self.short_lived)
                        o = self.short_out[j]
                        e.compute_disparity_map_batch(self.g.L[j % 9:j % 9 + 1], self.g.R[j % 9:j % 9 + 1], out=o, engine_streams=j % 2 == 0)
                        e.join()
                        self.short_lived.append((o, j % 9))
                        del e
                self.engine.join()
            self.stream.synchronize()
        except BaseException as exc:                                 # noqa: BLE001 (reported by the main thread)
            self.error = exc

    def check(self):
        assert self.error is None, f"thread {self.index}: {self.error!r}"
        for k, (pool, off, n, lanes, out) in enumerate(self.plan):
            assert torch.equal(out, pool.E[off:off + n]), f"thread {self.index} call {k} ({pool.name}, {n} pairs, {'lanes' if lanes else 'stream'})"
        for j, (o, i) in enumerate(self.short_lived):
            assert torch.equal(o[0], self.g.E[i]), f"thread {self.index}: short-lived engine {j}"


def _run_threads(targets, limit=240):
    threads = [threading.Thread(target=t, daemon=True) for t in targets]
    for t in threads:
        t.start()
    deadline = time.time() + limit
    for t in threads:
        t.join(max(0.0, deadline - time.time()))
    alive = [i for i, t in enumerate(threads) if t.is_alive()]
    assert not alive, f"threads {alive} still running after {limit} s"


@pytest.mark.parametrize("threads", [2, 4])
def test_one_engine_per_host_thread_on_one_device(cd, oracle_omp, threads):
    """include/stereo_mi355x.h: "Different engines may be driven from different host threads".  The engines of a device
    share one pair of lane streams (reference-counted under a lock), the process-wide LDS attributes are raised once per
    device, and ctypes drops the GIL around every call: each thread makes 40 calls alternating the lanes and a stream of
    its own on an engine of its own shape, joined and synchronised only at the end, while thread 0 also creates, uses once
    and drops 20 short-lived engines.  Every output of every thread against the oracle."""
    workers = [Worker(cd, oracle_omp, i) for i in range(threads)]
    torch.cuda.synchronize()                             # inputs and zeroed outputs complete
    barrier = threading.Barrier(threads)
    _run_threads([lambda w=w: w.run(cd, barrier, 20 if w.index == 0 else 0) for w in workers])
    torch.cuda.synchronize()
    for w in workers:
        w.check()
    assert len(workers[0].short_lived) == 20
    del workers
    gc.collect()


def test_last_error_is_per_thread(cd):
    """smx_last_error() returns the calling thread's last failure: two threads make different invalid calls straight
    through the C ABI (refused before the device is touched) and each reads its own message afterwards."""
    from cuda_depth import _native as N
    H, W = 64, 96
    sms = [cd.StereoMatching(cd.StereoMatchingConfiguration(height=H, width=W, min_disparity=0, max_disparity=15), max_batch=8)
           for _ in range(2)]
    buf = [torch.zeros((9, H, W), device="cuda") for _ in range(3)]
    torch.cuda.synchronize()
    barrier = threading.Barrier(2)
    seen = [None, None]

    def body(i):
        try:
            n = 0 if i == 0 else 9
            barrier.wait(timeout=60)
            rc = N.LIB.smx_compute_gray_batch(sms[i]._handle, n, buf[0].data_ptr(), buf[1].data_ptr(), buf[2].data_ptr(), C.c_void_p(0))
            barrier.wait(timeout=60)                     # both failures have happened before either message is read
            seen[i] = (rc, N.last_error())
        except BaseException as exc:                     # noqa: BLE001
            seen[i] = exc

    _run_threads([lambda: body(0), lambda: body(1)], limit=120)
    assert seen[0] == (-1, "batch size 0 outside [1, max_batch=8]"), seen
    assert seen[1] == (-1, "batch size 9 outside [1, max_batch=8]"), seen
