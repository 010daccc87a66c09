"""The one-launch AUTO kernel (k_match_auto.h) at large batches.

After an on-grid call of at most 4 pairs, f32 gray AUTO calls in the latency shape take one launch that branches per pair
on the device-side grid flag.  The workgroups of an off-grid pair become disparity slices: each writes partial arg-max
records into the calling lane's region of the slice buffer, and the last slice of a tile to take a ticket merges the tile.
The record count grows with the pairs of the call (nsplit slices x n pairs), so these calls go up to the engine's
max_batch = 64, with off-grid pairs among the last indices (b >= 16 included), on the caller's stream and back to back on
both stream lanes.  A call whose records would not fit the lane's region takes the two gated launches instead
(k_match_auto.h: match_auto_small_applicable).  Every pair is compared bit for bit with the oracle
(multi_block_matching_cost_aggregation.cu:54-88, wta_disparity_selection.cu:22-30)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import stereo_synthetic as syn                      # noqa: E402
from oracle_lib import OracleConfig                 # noqa: E402

MAX_BATCH = 64


@pytest.fixture(scope="module")
def cd():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import cuda_depth
    return cuda_depth


def _offgrid(n):
    """Indices of the off-grid pairs of a call of n pairs: pair 0 stays on the grid, the others sit among the last
    indices (every third from the middle on, and the last)."""
    return {1, n - 1} | set(range(n // 2 + 1, n, 3)) if n > 1 else set()


class _Pairs:
    """Distinct synthetic pairs per slot index (on the exact grid, or moved off it by + 0.3) and their oracle maps."""

    def __init__(self, oracle, H, W, K, D, seed0):
        self.oracle, self.H, self.W, self.K, self.D, self.seed0 = oracle, H, W, K, D, seed0
        self.ocfg = OracleConfig(height=H, width=W, downscale_factor=K, min_disparity=0, max_disparity=D - 1)
        self.cache = {}

    def get(self, i, off):
        key = (i, off)
        if key not in self.cache:
            l, r, _ = syn.make_pair(self.H, self.W, self.D, self.K, self.seed0 + i)
            if off:
                l = (l + np.float32(0.3)).astype(np.float32)       # off the grid, not integer-valued
            self.cache[key] = (l, r, self.oracle.run(self.ocfg, l, r))
        return self.cache[key]

    def batch(self, n, off):
        items = [self.get(i, i in off) for i in range(n)]
        tl = torch.from_numpy(np.stack([it[0] for it in items])).cuda()
        tr = torch.from_numpy(np.stack([it[1] for it in items])).cuda()
        return tl, tr, [it[2] for it in items]


def _check(got, want, off, what):
    bad = [i for i in range(len(want)) if not np.array_equal(got[i], want[i])]
    assert not bad, f"{what}: pairs {bad} differ from the oracle (off-grid pairs {sorted(off)})"


@pytest.mark.parametrize("H,W,K,D,calls,lane_calls", [
    (128, 256, 2, 64, (5, 16, 17, 19, 24, 32, 48, 64), (17, 24, 32, 17, 24, 32)),
    (64, 128, 1, 32, (5, 16, 17, 19, 24, 32, 48, 64), (17, 24, 32, 17, 24, 32)),
    (96, 160, 2, 32, (5, 16, 17, 19, 24, 32, 48, 64), (17, 24, 32, 17, 24, 32)),
    (375, 1242, 2, 128, (5, 12), ()),                  # C2: 12 pairs is the largest batch in the latency shape
])
def test_one_launch_auto_kernel_at_large_batches(cd, oracle_omp, H, W, K, D, calls, lane_calls):
    cfg = cd.StereoMatchingConfiguration(height=H, width=W, downscale_factor=K, min_disparity=0, max_disparity=D - 1)
    sm = cd.StereoMatching(cfg, max_batch=MAX_BATCH)
    pairs = _Pairs(oracle_omp, H, W, K, D, 1200)

    # an on-grid call of 4 pairs first: its report moves the later calls to the one-launch kernel
    tl, tr, want = pairs.batch(4, set())
    _check(sm.compute_disparity_map_batch(tl, tr).cpu().numpy(), want, set(), "on-grid call")
    assert sm.route_info()["offgrid_hint"] == 0

    large_in_one_launch = 0
    for n in calls:
        # the one-launch kernel serves the latency shape only (the split fast kernel); the sizes above keep it
        assert sm.match_geometry(n)["kernel"] == "fast_split", (n, sm.match_geometry(n))
        off = _offgrid(n)
        tl, tr, want = pairs.batch(n, off)
        sm.profile_begin(1)
        out = sm.compute_disparity_map_batch(tl, tr).cpu().numpy()
        prof = sm.profile_end()
        one = prof["match_exact"][1] == 0 and prof["match_fast"][1] == 1
        if n <= 16:
            assert one, (n, prof)                      # ONE aggregation launch: the records fit the lane's region
        else:
            # one launch when the records fit, else the two gated launches
            assert one or (prof["match_exact"][1] == 1 and prof["match_fast"][1] == 1), (n, prof)
            large_in_one_launch += one
        _check(out, want, off, f"{n} pairs")
        assert sm.route_info()["offgrid_hint"] == 0                   # pair 0 is on the grid
    if any(n > 16 for n in calls):
        assert large_in_one_launch > 0, "no call of more than 16 pairs took the one-launch kernel"

    # back to back on the stream lanes: consecutive calls of up to max_batch / 2 pairs alternate between the lanes and
    # the halves of the pair slots, so both lanes' record regions and tickets are live at once
    torch.cuda.synchronize()
    pending = []
    for n in lane_calls:
        off = _offgrid(n)
        tl, tr, want = pairs.batch(n, off)
        torch.cuda.synchronize()
        o = torch.zeros((n, H, W), device="cuda")
        sm.compute_disparity_map_batch(tl, tr, out=o, engine_streams=True)
        pending.append((o, tl, tr, want, off, n))
    sm.join()
    torch.cuda.synchronize()
    for k, (o, _, _, want, off, n) in enumerate(pending):
        _check(o.cpu().numpy(), want, off, f"lanes, call {k} of {n} pairs")
