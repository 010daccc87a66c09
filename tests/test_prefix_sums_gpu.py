"""The fast aggregation kernel on content whose box sums come close to 2^24, against the oracle.

At K <= 2 the kernel takes its box sums as differences of prefix sums down the tile rows (k_match_fast.h:
fast_pass_pair<..., PREFIX>), which is bit-exact while every prefix is an exact float32 integer: the largest, PH at tile row
TH + 10, reaches (TH + 11) * 48,195 * K^2 units on saturated content -- 11.4 M of the 16.8 M at the stacked bands' 48 rows and
K = 2 (tests/test_prefix_sums_cpu.py has the arithmetic).  The synthetic pairs of the other suites stay far below that, so
the content here is
  (a) both images all 255: every term saturated, every prefix at its maximum, every disparity ties (the winner is 0);
  (b) uint8 noise in {254, 255}: near-saturated sums whose lowest bits vary -- what a rounded prefix would lose;
  (c) one banded and one noise pair of stereo_synthetic: ordinary winners, for the indices and the neighbour planes.
Every case is one engine-stream call large enough for the throughput shape, at K = 2 and K = 1, in the forms that march
the prefix code: the stacked bands forced (48 rows in pass 1, 24 in the second pass), forbidden (tall bands), the dense form
forced; 49 rows (a second band of one row) and 33 disparities (an unpaired last disparity) stacked.  One single-pair call
takes a latency shape (the 8- and 10-row ones keep the sliding sums, the 12-row one takes the prefixes: whichever the plan
picks must match).  One K = 4 case shows that the K = 4 kernels, which keep the sliding sums, still match at saturation.
The final map, the WTA index and the three cost planes are compared bit for bit with the oracle, which is pure
integer-valued float32 arithmetic on this content (no tolerance)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import stereo_synthetic as syn                      # noqa: E402
import test_gpu_parity as parity                    # noqa: E402
from test_stacked_bands_gpu import _throughput_pairs    # noqa: E402


@pytest.fixture(scope="module")
def cd():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import cuda_depth
    return cuda_depth


@pytest.fixture(scope="module")
def cus(cd):
    cfg = cd.StereoMatchingConfiguration(height=64, width=96, min_disparity=0, max_disparity=15)
    return cd.StereoMatching(cfg).route_info()["compute_units"]


def _content(H, W, D, K):
    """(a), (b) and the two pairs of (c): uint8-valued float32 images."""
    rng = np.random.default_rng(1000 * K + H)
    sat = np.full((H, W), 255, np.float32)
    near = [rng.integers(254, 256, (H, W)).astype(np.float32) for _ in range(2)]
    return [(sat, sat.copy()), (near[0], near[1]), syn.make_pair(H, W, D, K, 81)[:2], syn.make_noise_pair(H, W, 82)]


_ORACLE = {}


def _oracle_runs(oracle, ocfg, key, pairs):
    """(map, intermediates) of every distinct pair, computed once per shape and shared by the forms that run it."""
    if key not in _ORACLE:
        _ORACLE[key] = [oracle.run(ocfg, l, r, intermediates=True, volumes=True) for l, r in pairs]
    return _ORACLE[key]


def _call(cd, cfg, tl, tr, n, env, monkeypatch):
    from cuda_depth import _native as N
    for k in ("SMX_FAST_STACK", "SMX_FAST_DENSE"):
        if k in env:
            monkeypatch.setenv(k, env[k])                           # read once, in smx_create
        else:
            monkeypatch.delenv(k, raising=False)
    sm = cd.StereoMatching(cfg, max_batch=n, overlap_min_pairs=-1)
    out = sm.compute_disparity_map_batch(tl, tr, engine_streams=True)
    sm.join()
    torch.cuda.synchronize()
    geo = sm.match_geometry(n)
    stages = {k: torch.stack([sm.intermediate(st, i) for i in range(n)]) for k, st in
              (("wta", N.STAGE_WTA), ("costs", N.STAGE_MBM_COSTS), ("refined", N.STAGE_REFINED), ("down_left", N.STAGE_DOWN_LEFT),
               ("down_right", N.STAGE_DOWN_RIGHT))}
    stages["out"] = out.clone()
    return geo, stages


STACKED, TALL, DENSE = ({"SMX_FAST_STACK": "1", "SMX_FAST_DENSE": "0"}, {"SMX_FAST_STACK": "0", "SMX_FAST_DENSE": "0"},
                        {"SMX_FAST_STACK": "0", "SMX_FAST_DENSE": "1"})
SHAPES = [
    # name, pooled h, pooled w, pooled disparities, form, band rows the geometry must report
    ("57x190_stacked", 57, 190, 64, STACKED, (48,)),
    ("57x190_tall", 57, 190, 64, TALL, (24, 27, 32)),
    ("57x190_dense", 57, 190, 64, DENSE, (24, 27)),
    ("49x100_stacked_one_row_band", 49, 100, 64, STACKED, (48,)),
    ("98x190_d33_unpaired_last", 98, 190, 33, STACKED, (48,)),
]
CASES = [(f"{s[0]}_k{K}", K) + s[1:] for K in (2, 1) for s in SHAPES] + [("25x100_stacked_k4_sliding_sums", 4, 25, 100, 64, STACKED, (48,))]


@pytest.mark.parametrize("name,K,h,w,Dd,env,bands", CASES, ids=[c[0] for c in CASES])
def test_near_saturated_batches_against_the_oracle(cd, oracle_omp, monkeypatch, cus, name, K, h, w, Dd, env, bands):
    H, W, D = h * K, w * K, Dd * K
    n = _throughput_pairs(h, w, cus)
    cfg, ocfg = parity._cfgs(cd, H, W, K, 0, D - 1)
    pairs = _content(H, W, D, K)
    if K == 4:
        pairs = pairs[:2]                                           # content (a) and (b)
    idx = torch.arange(n, device="cuda") % len(pairs)
    tl, tr = (torch.from_numpy(np.stack([p[k] for p in pairs])).to(torch.uint8).cuda()[idx].contiguous() for k in (0, 1))
    geo, got = _call(cd, cfg, tl, tr, n, env, monkeypatch)
    assert geo["kernel"] == "fast_window" and geo["band_rows"] in bands, geo
    for i, (ref_out, ref) in enumerate(_oracle_runs(oracle_omp, ocfg, (K, h, w, Dd), pairs)):
        for j in sorted({i, i + len(pairs) * ((n - 1 - i) // len(pairs))}):       # the pair's first and last copy in the batch
            assert int(idx[j]) == i
            parity._check({k: v[j].cpu().numpy() for k, v in got.items()}, ref_out, ref, 0)
    sat_wta = got["wta"][0].cpu().numpy()
    assert not sat_wta.any(), "saturated pair: every disparity ties, the first one wins"


@pytest.mark.parametrize("K", [2, 1])
def test_single_pair_calls_in_a_latency_shape(cd, oracle_omp, monkeypatch, K):
    h, w, Dd = 57, 190, 64
    H, W, D = h * K, w * K, Dd * K
    for k in ("SMX_FAST_STACK", "SMX_FAST_DENSE"):
        monkeypatch.delenv(k, raising=False)
    cfg, ocfg = parity._cfgs(cd, H, W, K, 0, D - 1)
    pairs = _content(H, W, D, K)
    for (l, r), (ref_out, ref) in zip(pairs, _oracle_runs(oracle_omp, ocfg, (K, h, w, Dd), pairs)):
        im = parity._run_hip(cd, cfg, l, r, "auto")
        assert im["flag"] == 0                                      # on the grid: the fast kernel ran
        parity._check(im, ref_out, ref, 0)
