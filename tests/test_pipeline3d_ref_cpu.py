"""CPU tests of the cases that tests/test_pipeline3d_chain_gpu.py runs on the device: the reference of the whole of
DepthEstimationPipeline.process() (pipeline3d_ref.Pipeline3DRef) alone over every case of pipeline3d_cases.  The cases cover
every pair of levels, and none of them is vacuous: the matched maps are fused, tracked, followed, spilled and rendered for
real.  The conditions are conditions on the inputs -- the scene, Q, the path and the seeds of pipeline3d_cases -- not on the
code under test; NOTES.md has the values the reference gave."""
import numpy as np
import pytest

import pipeline3d_cases as pc
import rectify_ref
from pairwise import uncovered_pairs

CASE_INDICES = list(range(len(pc.CASES)))
FLAT_AT = pc.ORDER.index(pc.FLAT)


def _valid(d, inv):
    return np.isfinite(d) & (d != np.float32(inv))


def test_every_pair_of_levels_is_covered():
    assert uncovered_pairs(pc.FACTORS, pc.CASES) == []
    assert len(set(pc.IDS)) == len(pc.CASES)
    assert any(tuple(kw.get("follow_anchor", (0.5, 0.5, 0.5))) != (0.5, 0.5, 0.5) for kw in pc.FOLLOW.values())


def test_the_frames_fill_the_disparity_range():
    """The scene's true disparities from the first pose reach most of the configured range."""
    truth = pc.scene().render(pc.path()[0], pc.H, pc.W, pc.FX, pc.CX, pc.CY, pc.BASE)
    assert pc.DMIN <= truth.min() and truth.max() >= 0.9 * pc.DMAX and (truth <= pc.DMAX).mean() > 0.97


@pytest.mark.parametrize("index", CASE_INDICES, ids=pc.IDS)
def test_case_is_not_vacuous(index):
    case, results = pc.CASES[index], pc.expected(index)
    assert len(results) == len(pc.ORDER) + 1
    inv = case["inv"]
    for k, r in enumerate(results):
        flat = k == FLAT_AT
        assert (len(r["cloud"]["points"]) == 0) == flat, f"frame {k}: cloud of {len(r['cloud']['points'])} points"
        assert _valid(r["disparity"], inv).any() or flat
    assert (results[-1]["state"]["weight"] > 0).any()
    before, lost_frame = results[FLAT_AT - 1]["state"], results[FLAT_AT]["state"]
    if case["poses"] == "tracked":
        lost = [bool(r["lost"]) for r in results]
        assert lost[FLAT_AT], "the flat frame must be lost"
        assert sum(lost) <= 2, f"lost frames {lost}"
        for k, r in enumerate(results):
            if k != FLAT_AT and not r["lost"]:
                err = np.linalg.norm(r["pose"][:3, 3] - pc.true_pose(k)[:3, 3])
                assert err < 2 * pc.VS, f"frame {k}: the tracked pose is {err / pc.VS:.2f} voxels off the path"
        assert np.array_equal(results[FLAT_AT]["pose"], results[FLAT_AT - 1]["pose"])
        assert results[FLAT_AT]["shift"] == (0, 0, 0) and results[FLAT_AT]["spilled"] == []
        for name in ("tsdf", "weight", "color"):                      # the volume is unchanged by the lost frame
            a, b = before[name], lost_frame[name]
            assert (a is None and b is None) or np.array_equal(a.view(np.uint8), b.view(np.uint8)), name
        assert before["offset"] == lost_frame["offset"] and before["origin"] == lost_frame["origin"]
    else:
        assert all(r["lost"] is None and r["pose"] is None for r in results)
    shifts = [r["shift"] for r in results]
    if case["follow"] == "off":
        assert all(s == (0, 0, 0) for s in shifts) and results[-1]["state"]["offset"] == (0, 0, 0)
    else:
        assert any(s != (0, 0, 0) for s in shifts[:len(pc.ORDER)]), "the path must move the volume"
        assert tuple(sum(s[a] for s in shifts) for a in range(3)) == results[-1]["state"]["offset"]
    boxes = [b for r in results for b in r["spilled"]]
    if case["follow"] == "spill":
        assert any((b["weight"] > 0).any() for b in boxes), "a spilled box must hold measured voxels"
        for r in results:
            assert len(r["spilled"]) == sum(c != 0 for c in r["shift"])
    else:
        assert boxes == []
    if case["render"]:
        for k, r in enumerate(results[1:], 1):
            share = float((r["model"] != np.float32(inv)).mean())
            assert share >= 0.2, f"frame {k}: the model map hits a surface in {share:.2f} of its pixels"
    else:
        assert all(r["model"] is None for r in results)
    if case["lrconf"]:
        for k, r in enumerate(results):
            if k == FLAT_AT:
                continue
            ok = _valid(r["disparity"], inv)
            rejected = ok & ~(r["confidence"] >= np.float32(0.1))
            assert rejected.any() and (ok & ~rejected).any(), f"frame {k}: min_confidence rejects {int(rejected.sum())}"
            assert ((r["confidence"] > 0) & (r["confidence"] < 1)).any(), "fractional weights"
    else:
        assert all(r["confidence"] is None for r in results)
    if case["rect"]:
        left_valid = rectify_ref.valid_mask(pc.rectification()[0], (pc.RAW_H, pc.RAW_W))
        assert results[0]["left"] is not None and (~left_valid).any() and left_valid.mean() > 0.9


def test_a_follow_case_shifts_on_two_axes_at_once():
    shifts = [r["shift"] for i in CASE_INDICES if pc.CASES[i]["follow"] != "off" for r in pc.expected(i)[:len(pc.ORDER)]]
    assert any(sum(c != 0 for c in s) >= 2 for s in shifts), shifts
