"""The two per-pair flags of the gray f32 prologues (k_prologue.h: k_prologue_k2, k_prologue_k4) on pairs that are clean except
for ONE value.

Flag 1 (SMX_STAGE_GRID_FLAG): some pooled value is off the 1/K^2 grid or outside [0, 255] -- the oracle's rule, evaluated here
on the oracle's own pooled planes.  Flag 2 (some full-resolution value is not an integer in [0, 255]) has no stage of its own:
it decides whether step 6 may read the byte planes, whose bytes for such a value are truncated or saturated, so the route the
call took shows in the map -- every stage has to equal the oracle's bit for bit, also for the values that stay on the pooled
grid (-1 and 256 inside a 2 x 2 or 4 x 4 block of integers).  What this cannot see: a flag 2 raised for nothing (on -0.0, on
the zero-filled columns behind the image or on the clamped second row) only sends step 6 to its float kernel, which computes
the same bits; the interface has no stage that reports flag 2, so "raises neither flag" is asserted for flag 1 and shown for
flag 2 only as far as the map goes.  The calls are AUTO calls: last_match_mode() is asserted.
Planted: NaN, -1, 255.5, 256, 0.5, 1e9 and -0.0 (clean); at the first element, the last element (on the odd-height image the
row that the pool clamps) and in row 1 of the odd-height image; in the left and in the right image; K = 2 and K = 4."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import test_gpu_parity as parity                    # noqa: E402

W, DMAX = 64, 7
VALUES = [("nan", np.nan), ("minus_1", -1.0), ("255_5", 255.5), ("256", 256.0), ("0_5", 0.5), ("1e9", 1.0e9), ("minus_0", -0.0)]
POSITIONS = [(32, 0, 0), (32, 31, W - 1), (33, 0, 0), (33, 32, W - 1), (33, 1, 17)]       # H, row, column


@pytest.fixture(scope="module")
def cd():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import cuda_depth
    return cuda_depth


def _clean_pair(H):
    """Integer-valued in [16, 200]: one planted -1 or 256 leaves every pooled mean inside [0, 255]."""
    rng = np.random.default_rng(4100 + H)
    left = rng.integers(16, 201, (H, W)).astype(np.float32)
    right = np.roll(left, -3, axis=1).copy()
    right[::3] = np.clip(right[::3] + 1, 16, 200)
    return left, right


def _oracle_grid_flag(ref, K):
    """The oracle's rule on its pooled planes: every value a multiple of 1/K^2 in [0, 255]."""
    bad = False
    for k in ("down_left", "down_right"):
        p = ref[k].astype(np.float32)
        s = p * np.float32(K * K)
        with np.errstate(invalid="ignore"):
            bad = bad or not bool(np.all((s == np.rint(s)) & (p >= 0) & (p <= 255)))
    return bad


@pytest.mark.parametrize("K", [2, 4])
def test_an_all_integer_pair_raises_neither_flag(cd, oracle_omp, K):
    for H in (32, 33):
        cfg, ocfg = parity._cfgs(cd, H, W, K, 0, DMAX)
        left, right = _clean_pair(H)
        ref_out, ref = oracle_omp.run(ocfg, left, right, intermediates=True, volumes=True)
        im = parity._run_hip(cd, cfg, left, right, "auto")
        assert not _oracle_grid_flag(ref, K) and im["flag"] == 0 and im["mode"] == "auto"
        parity._check(im, ref_out, ref, 0)


@pytest.mark.parametrize("K", [2, 4])
@pytest.mark.parametrize("name,value", VALUES, ids=[v[0] for v in VALUES])
def test_one_planted_value(cd, oracle_omp, K, name, value):
    for H, y, x in POSITIONS:
        cfg, ocfg = parity._cfgs(cd, H, W, K, 0, DMAX)
        for which in ("left", "right"):
            left, right = _clean_pair(H)
            (left if which == "left" else right)[y, x] = np.float32(value)
            ref_out, ref = oracle_omp.run(ocfg, left, right, intermediates=True, volumes=True)
            im = parity._run_hip(cd, cfg, left, right, "auto")
            want = _oracle_grid_flag(ref, K)
            where = f"{name} in the {which} image of {H} x {W} at ({y}, {x}), K = {K}"
            print(f"{where}: grid flag {im['flag']}, the oracle's rule {int(want)}")
            assert (im["flag"] != 0) == want and im["mode"] == "auto", where
            # what the rule gives for each case (a check of this test's own cases).  In the last row of the odd-height image
            # the pool clamps: the planted value is summed K times and a half lands on the grid again.
            if name in ("minus_1", "256", "minus_0") or (name in ("255_5", "0_5") and y == H - 1 and H % 2 == 1):
                assert not want, where                    # on the pooled grid: only the second flag can keep step 6 off the bytes
            else:
                assert want, where
            if name != "nan":                             # (a NaN cost has no order: the flag is the check there)
                parity._check(im, ref_out, ref, 0)
