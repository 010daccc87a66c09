"""The rule of smx_track_camera on the CPU: tests/track_ref.py, the NumPy twin written from the header, on the analytic
scene of tests/tsdf_ref.py.  The model view is the exact depth of the scene with its face normals at one pose of a small
orbit, the frame the exact disparity at the next pose, 0.218 m and 0.333 degrees away; tracking starts from the model's
pose.  The bound, 0.02 m and 0.1 degrees, is a tenth of the start; a float64 prototype of the rule reached 0.0015 m and
0.020 degrees.  Then the deep-tree frames of tests/track_cases.py: that they reach every form of the solve kernel's sum
tree and that a wrong order of the tiles would change the sums they compare.  No GPU."""
import functools
import os
import re

import numpy as np
import pytest

import raycast_cases as cases
import track_cases as tc
import track_ref as tr
import tsdf_ref as ref

f32 = np.float32
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "stereo-depth_amd", "csrc")
H, W, FX, B, CX, CY = 60, 80, 80.0, 0.54, 39.75, 29.0
Q = cases.reprojection(FX, CX, CY, B)
MAX_DISTANCE, DEPTH_RANGE = 0.3, (0.0, 12.0)
BOUND_M, BOUND_DEG = 0.02, 0.1


def scene_view(scene, pose):
    """(depth [H, W] f32 with NaN for a miss, normals [3, H, W] f32, 0 for a miss) of the scene from pose."""
    d = scene.render(pose, H, W, FX, CX, CY, B)
    hit = d > 0
    with np.errstate(divide="ignore"):
        z = np.where(hit, FX * B / d.astype(np.float64), np.nan)
    v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    m = np.asarray(pose, np.float64)
    dirs = np.stack([(u - CX) / FX, (v - CY) / FX, np.ones_like(u)], -1).reshape(-1, 3) @ m[:3, :3].T
    pts = m[:3, 3] + dirs * np.nan_to_num(z).reshape(-1, 1)
    nrm, _ = scene.face_normals(pts, 0.0)
    nrm = np.where(hit.reshape(-1, 1), nrm, 0.0)
    return z.astype(f32), np.ascontiguousarray(nrm.T.reshape(3, H, W).astype(f32))


@functools.lru_cache(maxsize=None)
def setup():
    scene = ref.demo_scene()
    poses = ref.orbit_poses(24)
    depth, nrm = scene_view(scene, poses[0])
    model = tr.model_view(depth, nrm, Q, poses[0])
    frame = scene.render(poses[1], H, W, FX, CX, CY, B)
    return scene, poses, model, frame


def track(frame, pose_in, model, **kw):
    kw.setdefault("max_distance", MAX_DISTANCE)
    kw.setdefault("depth_range", DEPTH_RANGE)
    return tr.track_ref(frame, Q, pose_in, model, **kw)


def test_the_start_is_as_far_as_the_issue_says():
    _, poses, _, _ = setup()
    m, deg = tr.pose_error(poses[0], poses[1])
    assert abs(m - 0.218) < 0.001 and abs(deg - 0.333) < 0.001


@pytest.mark.parametrize("schedule", [tr.DEFAULT_SCHEDULE, ((1, 10),)], ids=["coarse_to_fine", "ten_at_stride_1"])
def test_tracks_the_next_orbit_pose(schedule):
    _, poses, model, frame = setup()
    out = track(frame, poses[0], model, schedule=schedule)
    m, deg = tr.pose_error(out["pose"], poses[1])
    print(f"{schedule}: error {m:.5f} m {deg:.4f} deg, info {out['info']}, rms {out['rms']:.5f}")
    assert out["info"][0] == 0 and out["info"][1] == sum(k for _, k in schedule)
    assert m <= BOUND_M and deg <= BOUND_DEG
    assert out["info"][2] * 2 >= out["info"][3] > 0                   # most accepted pixels end as inliers


def test_the_sums_equal_a_plain_float64_einsum():
    _, poses, model, frame = setup()
    pts = tr.frame_points(frame, Q, depth_range=DEPTH_RANGE)
    for stride in (1, 2, 3, 4):
        terms = tr.pixel_terms(pts, tr.model_view(0, 0, Q, poses[0])["c2w"], model, stride, MAX_DISTANCE)
        got = tr.reduce_terms(terms)
        want = np.einsum("khw->k", terms)
        assert got[29] > 100
        np.testing.assert_allclose(got, want, rtol=1e-9, atol=0)
        assert got[tr.TERMS] == pts[4][::stride, ::stride].sum()


def test_one_iteration_is_the_normal_equations_of_its_terms():
    """sums -> solve is the least-squares twist of the rows: compare with numpy's solver on the same float64 sums."""
    _, poses, model, frame = setup()
    out = track(frame, poses[0], model, schedule=((1, 1),))
    A = tr.information(out["sums"])
    x = tr.solve(np.concatenate([out["sums"], [0.0]]), 1e-6)
    np.testing.assert_allclose(x, np.linalg.solve(A, out["sums"][21:27]), rtol=1e-8)
    assert np.all(np.linalg.eigvalsh(A) > 0)


def test_cayley_is_a_rotation():
    C = tr.cayley([f32(0.03), f32(-0.2), f32(0.11)]).astype(np.float64)
    np.testing.assert_allclose(C @ C.T, np.eye(3), atol=3e-7)
    assert abs(np.linalg.det(C) - 1.0) < 3e-7
    assert np.array_equal(tr.cayley([f32(0)] * 3), np.eye(3, dtype=f32))


def assert_lost(out, pose_in):
    assert out["info"][0] == 1
    assert np.array_equal(out["pose"].view(np.uint32), np.asarray(pose_in, f32)[:3].view(np.uint32))


def test_lost_when_the_model_view_is_all_misses():
    _, poses, model, frame = setup()
    empty = dict(model, depth=np.full((H, W), np.nan, f32), normals=np.zeros((3, H, W), f32))
    out = track(frame, poses[0], empty)
    assert_lost(out, poses[0])
    assert out["info"][1] == 1 and out["info"][2] == 0 and out["info"][3] > 0 and np.isnan(out["rms"])


def test_lost_when_the_start_is_5_m_away():
    _, poses, model, frame = setup()
    start = poses[0].copy()
    start[:3, 3] += [5.0, 0.0, 0.0]
    out = track(frame, start, model)
    assert_lost(out, start)
    assert out["info"][2] < 100


def test_lost_when_the_frame_sees_one_plane_only():
    _, poses, _, _ = setup()
    ground = ref.Scene(ground_y=1.5)
    depth, nrm = scene_view(ground, poses[0])
    out = track(ground.render(poses[1], H, W, FX, CX, CY, B), poses[0], tr.model_view(depth, nrm, Q, poses[0]))
    assert out["info"][2] >= 100                                      # plenty of inliers: the pivot rule caught it
    assert_lost(out, poses[0])


# ---- the deep-tree frames of tests/track_cases.py: what tests/test_track_tree_gpu.py relies on, from the twin alone --------

def workspace_constant(name):
    pattern = rf"^#define {name} (\d+)\b" if name.startswith("SMX_") else rf"\b{name} = (\d+)[,;]"
    found = re.findall(pattern, open(os.path.join(CSRC, "smx_workspace.h")).read(), flags=re.MULTILINE)
    assert len(found) == 1, name
    return int(found[0])


def test_the_tree_cases_reach_every_form_of_the_solve():
    """The grid arithmetic restated in track_cases.py uses the library's constants, every case has the len it names,
    and together they take all four forms of k_track_solve: len 2, len 4 and leaves of eight under one to six levels."""
    assert (tc.TILE_COLS, tc.GROUP_TILES) == (workspace_constant("TRK_COLS"), workspace_constant("TRK_WAVES"))
    assert tc.TILE_ROWS == workspace_constant("SMX_TRK_ROWS") == tr.ROWS and tc.TILE_COLS == tr.COLS
    solve = open(os.path.join(CSRC, "k_track.h")).read()
    assert f"constexpr int TRK_CHUNKS = {tc.CHUNKS};" in solve and "constexpr int TRK_STACK = 6;" in solve
    for shape, stride, want in tc.TREE_CASES:
        assert tc.tree_len(shape, stride) == want, (shape, stride, tc.tree_len(shape, stride))
        assert (shape, ((stride, 1),)) in tc.TREE_RUNS
    assert {n for _, _, n in tc.TREE_CASES} == tc.TREE_LENS == {2, 4, 8, 16, 32, 64, 256}
    assert tc.track_grid(tc.LIMIT_SHAPE, 1)["tiles"] == workspace_constant("TRK_MAX_TILES")
    assert tc.track_grid((tc.LIMIT_SHAPE[0] + 4, tc.LIMIT_SHAPE[1]), 1)["tiles"] > workspace_constant("TRK_MAX_TILES")
    assert tc.track_grid((1027, 193), 1)["groups"] == 257             # one partial in chunk 16, the rest past the bound
    assert [tc.tree_len(tc.TREE_MIXED[0], s) for s, _ in tc.TREE_MIXED[1]] == [8, 16, 64]
    assert all(tc.tree_len(s, 1) == 1 for s in tc.FRAME_SHAPES + (tc.SEQ_SHAPE,))   # what the other files reach


@pytest.mark.parametrize("run", tc.TREE_RUNS, ids=tc.run_id)
def test_a_tree_case_would_show_a_wrong_order(run):
    """The twin tracks the case, every group of four tiles holds inliers (so no partial is the +0.0 that any order sums
    right), and three wrong orders each change the bits of one of the sums 0..27: the tiles one after the other, the
    pairs tree over the tile columns, and the right tree with its leaves of eight partials added in turn."""
    shape, schedule = run
    want = tc.tree_expected(run)
    grid = tc.track_grid(shape, schedule[-1][0])
    tiles = want["tiles"]
    assert want["info"][0] == 0 and want["info"][1] == sum(k for _, k in schedule)
    assert 2 * want["info"][2] >= want["info"][3] > 0
    assert tiles.shape == (tr.TERMS + 1, grid["tiles"])
    partials = tc.group_partials(tiles)
    assert partials.shape[1] == grid["groups"] and (partials[29] != 0).all()
    right = tc.sums_in_order(tiles, grid, "tree")
    assert np.array_equal(right[:tr.TERMS].view(np.uint64), want["sums"].view(np.uint64))
    for order in ("left_to_right", "column_major", "leaves_in_turn"):
        changed = int((tc.sums_in_order(tiles, grid, order)[:28].view(np.uint64) != right[:28].view(np.uint64)).sum())
        print(f"{tc.run_id(run)}: {order} changes {changed} of the sums 0..27")
        assert changed >= 1, order


@pytest.mark.parametrize("stride", [1, 3])
def test_bands_of_tile_rows_give_the_unbanded_bits(stride):
    shape, schedule = (1027, 193), ((stride, 2),)
    d, Q = tc.scaled_frame(shape)
    whole, banded = (tr.track_ref(d, Q, tc.start_pose(tc.TREE_VIEW), tc.model(tc.TREE_VIEW), schedule=schedule,
                                  confidence=tc.wide_confidence(shape), keep_tiles=True, band_tile_rows=band, **tc.PARAMS)
                     for band in (None, 7))
    assert tc.track_grid(shape, stride)["ty"] % 7 != 0                # the last band is a partial one
    tc.assert_same(banded, whole, "banded")
    assert np.array_equal(banded["tiles"].view(np.uint64), whole["tiles"].view(np.uint64))


def test_a_tolerance_stops_the_schedule_early():
    _, poses, model, frame = setup()
    out = track(frame, poses[0], model, rot_eps=1e-3, trans_eps=2e-3)
    assert out["info"][0] == 0 and 1 <= out["info"][1] < 19
    full = track(frame, poses[0], model)
    assert full["info"][1] == 19
    assert track(frame, poses[0], model, schedule=())["info"][1] == 0
