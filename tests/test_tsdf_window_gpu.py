"""The windowed copy of a TSDF volume on the device (include/stereo_mi355x.h: smx_tsdf_window) and what TSDFVolume builds
on it.  The kernel against its NumPy twin (tests/tsdf_window_ref.py) as 32-bit words, with guard bands around every
output; shift, window and the spill boxes of TSDFVolume against the twin; a sphere cut by a shift, whose surface the
boxes and the shifted volume hold between them only with a margin; a volume that follows the camera against a large
fixed one, bit for bit; render and track after a shift against the same window of the unshifted volume; graph replay."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import tsdf_follow_cases as fc                      # noqa: E402
import tsdf_window_ref as wref                      # noqa: E402

SENTINEL = 0xDEADBEEF
GUARDS = (5, 6, 7)                                   # words before each output: three different 16-byte phases
SOURCE_DIMS = [(13, 7, 5), (1, 6, 4), (67, 9, 6), (130, 3, 3), (517, 3, 2), (4096, 1, 2)]
OTHER_DIMS = [(5, 3, 2), (16, 7, 9), (131, 4, 3)]
MIXED_STARTS = [(-2, 1, -1), (3, -2, 2), (-5, -3, 4), (1, 1, 1), (-1, -1, -1), (4, -6, -2), (-64, 2, 1), (7, 0, -3),
                (200, 0, 0), (0, -100, 0), (-131, -4, -3), (66, 8, 5)]
# Rows of more than 64 quads: a lane of window_row takes a second trip from 260 voxels on (259 with a head of 3 words is
# the last width without one), production volumes are 512 wide and the entry takes 4096.  source dims -> the windows'
# dims; x0 puts lo and hi (the row's voxels that have a source) inside the first 64 quads and past them.
LONG_ROWS = {(517, 3, 2): [(259, 2, 2), (260, 2, 2), (261, 2, 2), (263, 2, 2), (515, 2, 2)], (4096, 1, 2): [(4096, 1, 2)]}
LONG_X0 = (-300, -257, -1, 0, 1, 2, 3, 255, 258, 300)


@pytest.fixture(scope="module")
def cd():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import cuda_depth
    return cuda_depth


@pytest.fixture(scope="module")
def native(cd):
    from cuda_depth import _native
    return _native


def dev_words(a: np.ndarray) -> "torch.Tensor":
    """uint32 words as an int32 device tensor."""
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda()


def words(t: "torch.Tensor") -> np.ndarray:
    """Any 4-byte-per-voxel state tensor as uint32 words [nz, ny, nx]."""
    a = t.detach().cpu().contiguous().numpy()
    if a.dtype == np.uint8:
        return a.view(np.uint32)[..., 0]
    return a.view(np.uint32)


def starts_for(dims, out_dims):
    """One axis at a time, around both volumes' ends (n: the source's and the window's size on that axis), then mixed;
    for the long rows LONG_X0 alone and beside a row and a slice that have no source."""
    if dims in LONG_ROWS:
        return [(x0, 0, 0) for x0 in LONG_X0] + [(x0, 1, -1) for x0 in LONG_X0[::3]] + [(dims[0] - 257, 0, 0), (-dims[0] + 1, 0, 0)]
    out = []
    for axis in range(3):
        values = set()
        for n in {dims[axis], out_dims[axis]}:
            values |= {-n - 1, -n, -(n - 1), -5, -1, 0, 1, 3, 4, n - 1, n, n + 1}
        for v in sorted(values):
            s = [0, 0, 0]
            s[axis] = v
            out.append(tuple(s))
    return out + MIXED_STARTS


def random_state(rng, dims, colour=True):
    nx, ny, nz = dims
    return {"tsdf": wref.random_words(rng, (nz, ny, nx)), "weight": wref.random_words(rng, (nz, ny, nx)),
            "color": wref.random_words(rng, (nz, ny, nx)) if colour else None}


def load_state(vol, state):
    """The volume's state set to the words of `state`, bit for bit."""
    vol.tsdf.view(torch.int32).copy_(dev_words(state["tsdf"]))
    vol.weight.view(torch.int32).copy_(dev_words(state["weight"]))
    if state["color"] is not None:
        vol.color.view(torch.int32).copy_(dev_words(state["color"])[..., None])


def volume_words(vol):
    return {"tsdf": words(vol.tsdf), "weight": words(vol.weight), "color": None if vol.color is None else words(vol.color)}


def assert_state(got, want, what):
    for k in ("tsdf", "weight", "color"):
        if want[k] is None:
            assert got[k] is None, f"{what}: {k}"
            continue
        assert got[k].shape == want[k].shape, f"{what}: {k} shape {got[k].shape} != {want[k].shape}"
        bad = np.argwhere(got[k] != want[k])
        assert bad.size == 0, f"{what}: {k}: {len(bad)} words differ, first at (k, j, i) = {tuple(bad[0])}"


# ---- the kernel against the twin ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("colour", [True, False])
@pytest.mark.parametrize("dims", SOURCE_DIMS)
def test_kernel_matches_the_twin(native, dims, colour):
    rng = np.random.default_rng(sum(dims) + colour)
    nx, ny, nz = dims
    state = random_state(rng, dims, colour)
    names = ("tsdf", "weight", "color")[:3 if colour else 2]
    src = {k: dev_words(state[k]) for k in names}
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for out_dims in LONG_ROWS.get(dims, [dims] + OTHER_DIMS):
        bx, by, bz = out_dims
        count = bx * by * bz
        bufs = {k: torch.empty(g + count + 9, dtype=torch.int32, device="cuda") for k, g in zip(names, GUARDS)}
        ptr = {k: bufs[k].data_ptr() + 4 * g for k, g in zip(names, GUARDS)}
        pending = []
        for start in starts_for(dims, out_dims):
            for b in bufs.values():
                b.fill_(SENTINEL - 2 ** 32)
            rc = native.LIB.smx_tsdf_window(0, nx, ny, nz, src["tsdf"].data_ptr(), src["weight"].data_ptr(),
                                            src["color"].data_ptr() if colour else None, *start, bx, by, bz, ptr["tsdf"],
                                            ptr["weight"], ptr["color"] if colour else None, stream)
            assert rc == 0, native.last_error()
            pending.append((start, {k: b.clone() for k, b in bufs.items()}))
        torch.cuda.synchronize()
        for start, outs in pending:
            for k, g in zip(names, GUARDS):
                got = outs[k].cpu().numpy().view(np.uint32)
                what = f"{k} of window {start} + {out_dims} of {dims}"
                assert (got[:g] == SENTINEL).all() and (got[g + count:] == SENTINEL).all(), f"{what}: guard band written"
                want = wref.window_ref(state[k], start, out_dims)
                bad = np.argwhere(got[g:g + count].reshape(bz, by, bx) != want)
                assert bad.size == 0, f"{what}: {len(bad)} words differ, first at (k, j, i) = {tuple(bad[0])}"


def test_window_crops_and_grows(cd):
    rng = np.random.default_rng(3)
    dims, vs, origin = (13, 7, 5), 0.125, (-1.0, 0.5, 2.0)
    for colour in (True, False):
        vol = cd.TSDFVolume(dims, vs, origin, color=colour, truncation=0.5, max_weight=7.0)
        state = random_state(rng, dims, colour)
        load_state(vol, state)
        for start, out_dims in (((2, 1, 1), (6, 4, 3)), ((-3, -2, -1), (20, 12, 8)), ((5, 0, -2), (13, 7, 5))):
            win = vol.window(start, out_dims)
            assert isinstance(win, cd.TSDFVolume) and win.dims == out_dims and (win.color is not None) == colour
            assert (win.voxel_size, win.truncation, win.max_weight, win.device) == (vs, 0.5, 7.0, vol.device)
            assert win.offset == start and win.origin == wref.origin_ref(origin, start, vs)
            assert_state(volume_words(win), wref.window_state(state, start, out_dims), f"window {start} {out_dims}")
            again = win.window((1, 0, 0), (3, 3, 3))                 # a window of a window: the offsets add
            assert again.offset == (start[0] + 1, start[1], start[2])
            assert again.origin == wref.origin_ref(origin, again.offset, vs)
        assert vol.offset == (0, 0, 0) and vol.origin == origin
        assert_state(volume_words(vol), state, "the source is untouched")


# ---- shift ------------------------------------------------------------------------------------------------------------------

def test_shift_semantics(cd):
    rng = np.random.default_rng(11)
    dims, vs, origin = (67, 9, 6), 0.1, (0.3, -0.45, 1.7)
    vol = cd.TSDFVolume(dims, vs, origin)
    state = random_state(rng, dims)
    load_state(vol, state)
    first = (vol.tsdf, vol.weight, vol.color)
    assert vol.shift((0, 0, 0)) == [] and vol._spare is None
    assert all(a is b for a, b in zip(first, (vol.tsdf, vol.weight, vol.color))), "(0, 0, 0) must not swap the state"
    d1 = (5, -2, 1)
    assert vol.shift(d1) == []
    state = wref.window_state(state, d1, dims)
    assert_state(volume_words(vol), state, f"shift {d1}")
    assert vol.offset == d1 and vol.origin == wref.origin_ref(origin, d1, vs)
    second = (vol.tsdf, vol.weight, vol.color)
    assert all(a is not b for a, b in zip(first, second)), "the state tensors are different tensors after a shift"
    assert [t.data_ptr() for t in vol._spare] == [t.data_ptr() for t in first]
    d2 = (-64, 3, 0)
    vol.shift(d2)
    state = wref.window_state(state, d2, dims)
    assert_state(volume_words(vol), state, f"then shift {d2}")
    total = tuple(a + b for a, b in zip(d1, d2))
    assert vol.offset == total and vol.origin == wref.origin_ref(origin, total, vs)
    # the spare is reused: the third state is the first state's memory again
    assert [t.data_ptr() for t in (vol.tsdf, vol.weight, vol.color)] == [t.data_ptr() for t in first]
    assert [t.data_ptr() for t in vol._spare] == [t.data_ptr() for t in second]
    vol.reset()
    assert vol.offset == total and int(vol.weight.count_nonzero().item()) == 0, "reset keeps the offset"
    vol.release_spare()
    assert vol._spare is None
    vol.shift((1, 0, 0))
    assert vol._spare is not None and vol.offset == (total[0] + 1, total[1], total[2])


@pytest.mark.parametrize("d", [(3, 0, 0), (0, -2, 0), (0, 0, 4), (-5, 2, -1), (70, 0, 0)])
def test_shift_there_and_back(cd, d):
    rng = np.random.default_rng(17)
    dims = (67, 9, 6)
    vol = cd.TSDFVolume(dims, 0.1, (0.0, 0.0, 0.0))
    state = random_state(rng, dims)
    load_state(vol, state)
    vol.shift(d)
    vol.shift(tuple(-c for c in d))
    assert vol.offset == (0, 0, 0) and vol.origin == (0.0, 0.0, 0.0)
    nz, ny, nx = state["tsdf"].shape
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    stayed = ((i - d[0] >= 0) & (i - d[0] < nx) & (j - d[1] >= 0) & (j - d[1] < ny) & (k - d[2] >= 0) & (k - d[2] < nz))
    want = {name: None if a is None else np.where(stayed, a, 0).astype(np.uint32) for name, a in state.items()}
    assert_state(volume_words(vol), want, f"shift {d} and back")
    assert stayed.any() == (abs(d[0]) < nx)


# ---- spill ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("margin", [0, 1, 2])
@pytest.mark.parametrize("d", [(0, 0, 2), (-3, 0, 0), (2, -1, 0), (1, 1, -1)])
def test_spill_boxes_hold_what_left(cd, d, margin):
    rng = np.random.default_rng(23 + margin)
    dims, vs, origin = (13, 7, 5), 0.25, (1.0, -2.0, 0.5)
    vol = cd.TSDFVolume(dims, vs, origin)
    vol.shift((2, 0, -1))                                             # a volume that has moved before
    before_offset = vol.offset
    state = random_state(rng, dims)
    load_state(vol, state)
    boxes = vol.shift(d, spill=True, margin=margin)
    want = wref.spill_boxes_ref(dims, d, margin)
    assert len(boxes) == len(want) == sum(c != 0 for c in d)
    for box, (start, size) in zip(boxes, want):
        assert isinstance(box, cd.TSDFVolume) and box.dims == size
        moved = tuple(a + b for a, b in zip(before_offset, start))
        assert box.offset == moved and box.origin == wref.origin_ref(origin, moved, vs)
        assert_state(volume_words(box), wref.window_state(state, start, size), f"box {start} {size} of shift {d}")
    assert_state(volume_words(vol), wref.window_state(state, d, dims), f"shift {d} with spill")
    assert vol.shift(d) == []                                         # without spill nothing comes back


def sphere_volume(cd, dims, vs, origin, centre, radius):
    """A volume holding the exact truncated distance to a sphere, every voxel measured once."""
    vol = cd.TSDFVolume(dims, vs, origin, color=False)
    nx, ny, nz = dims
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    c = np.stack([origin[0] + (i + 0.5) * vs, origin[1] + (j + 0.5) * vs, origin[2] + (k + 0.5) * vs], axis=-1)
    sdf = np.linalg.norm(c - np.asarray(centre), axis=-1) - radius
    vol.tsdf.copy_(torch.from_numpy(np.clip(sdf / vol.truncation, -1.0, 1.0).astype(np.float32)))
    vol.weight.fill_(1.0)
    return vol


def point_sets(cd, volumes, vs):
    """(the points of the volumes' extractions as a set of coordinates rounded to 1e-4 voxels, the set of voxel cells
    that voxel_downsample at vs makes of all of them together)."""
    clouds = [v.extract_point_cloud(normals=False) for v in volumes]
    pts = torch.cat([c.points for c in clouds])
    raw = {tuple(p) for p in np.round(pts.cpu().numpy().astype(np.float64) / vs * 1e4).astype(np.int64).tolist()}
    down = cd.voxel_downsample(cd.PointCloud(points=pts.contiguous(), colors=None, normals=None), vs)
    cells = {tuple(p) for p in np.floor(down.points.cpu().numpy().astype(np.float64) / vs).astype(np.int64).tolist()}
    return raw, cells


@pytest.mark.parametrize("d", [(0, 0, 5), (-6, 0, 0), (8, -7, 0)])
def test_the_margin_keeps_the_seam(cd, d):
    """A sphere cut by the leaving plane(s): what the boxes and the shifted volume hold between them is the unshifted
    volume's surface with margin=1 (the duplicates in the margin layer and in the boxes' shared corner vanish in the
    set and under voxel_downsample) and lacks the crossings between leaving and staying voxels with margin=0.  Both
    as the set of the points themselves and as the set of cells that voxel_downsample at voxel_size makes of them
    (duplicates move a cell's centroid, not the cell); with two leaving planes every cell of a lost crossing also holds
    another point, so there only the points themselves are strictly fewer."""
    dims, vs, origin = (24, 20, 22), 0.125, (-1.5, -1.25, 0.5)
    centre, radius = (0.05, -0.02, 1.9), 0.9
    whole_raw, whole_cells = point_sets(cd, [sphere_volume(cd, dims, vs, origin, centre, radius)], vs)
    assert len(whole_raw) > 500
    sizes = {}
    for margin in (1, 0):
        vol = sphere_volume(cd, dims, vs, origin, centre, radius)
        boxes = vol.shift(d, spill=True, margin=margin)
        raw, cells = point_sets(cd, boxes + [vol], vs)
        sizes[margin] = (len(raw), len(cells))
        if margin == 1:
            assert raw == whole_raw and cells == whole_cells
        else:
            assert raw < whole_raw and cells <= whole_cells, "without a margin the seam's crossings must be missing"
            assert cells < whole_cells or sum(c != 0 for c in d) > 1
    assert sizes[0][0] < sizes[1][0]


# ---- a moving volume equals a cropped fixed one ----------------------------------------------------------------------------

def test_a_following_volume_equals_a_cropped_fixed_one(cd):
    VS, BIG_DIMS, SMALL_DIMS, SMALL_AT, small_origin = fc.VS, fc.BIG_DIMS, fc.SMALL_DIMS, fc.SMALL_AT, fc.SMALL_ORIGIN
    Q = fc.q_matrix(cd)
    poses, maps, images = fc.path_frames(8)
    big = cd.TSDFVolume(BIG_DIMS, VS, fc.BIG_ORIGIN)
    small = cd.TSDFVolume(SMALL_DIMS, VS, small_origin)
    offsets, shifts = [], 0
    for pose, d, img in zip(poses, maps, images):
        before = wref.origin_ref(small_origin, offsets[-1] if offsets else (0, 0, 0), VS)
        moved, boxes = small.follow(pose)
        assert boxes == [] and moved == wref.follow_ref(pose[:3, 3], before, SMALL_DIMS, VS)
        shifts += moved != (0, 0, 0)
        offsets.append(small.offset)
        td, ti = torch.from_numpy(d).cuda(), torch.from_numpy(img).cuda()
        big.integrate(td, Q, pose, image=ti, depth_range=fc.DEPTH_RANGE)
        small.integrate(td, Q, pose, image=ti, depth_range=fc.DEPTH_RANGE)
    assert shifts >= 2, f"the path must move the volume at least twice, offsets {offsets}"
    assert small.origin == wref.origin_ref(small_origin, offsets[-1], VS)
    # the voxels of the final window that were inside the window at every frame, from the recorded offsets
    nx, ny, nz = SMALL_DIMS
    mask = np.ones((nz, ny, nx), bool)
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    last = offsets[-1]
    for off in offsets:
        for idx, n, a in ((i, nx, 0), (j, ny, 1), (k, nz, 2)):
            at = idx + last[a] - off[a]
            mask &= (at >= 0) & (at < n)
    assert mask.mean() >= 0.25, f"the path leaves only {mask.mean():.3f} of the volume inside every window"
    x0, y0, z0 = (a + b for a, b in zip(SMALL_AT, last))
    assert x0 >= 0 and y0 >= 0 and z0 >= 0 and x0 + nx <= BIG_DIMS[0] and y0 + ny <= BIG_DIMS[1] and z0 + nz <= BIG_DIMS[2]
    measured = 0
    for name in ("tsdf", "weight", "color"):
        got = words(getattr(small, name))
        want = words(getattr(big, name))[z0:z0 + nz, y0:y0 + ny, x0:x0 + nx]
        bad = np.argwhere((got != want) & mask)
        assert bad.size == 0, f"{name}: {len(bad)} voxels differ from the fixed volume, first at (k, j, i) = {tuple(bad[0])}"
        if name == "weight":
            measured = int(((got != 0) & mask).sum())
    assert measured > 2000, f"only {measured} compared voxels were ever measured"


# ---- render and track after a shift ---------------------------------------------------------------------------------------

def test_render_and_track_after_a_shift(cd):
    Q, SMALL_DIMS, FRAME_H, FRAME_W = fc.q_matrix(cd), fc.SMALL_DIMS, fc.FRAME_H, fc.FRAME_W
    poses, maps, images = fc.path_frames(4, fc.VIEW_START, fc.VIEW_STEP)
    vol = cd.TSDFVolume(SMALL_DIMS, fc.VS, fc.VIEW_ORIGIN)
    for pose, d, img in zip(poses[:3], maps, images):
        vol.integrate(torch.from_numpy(d).cuda(), Q, pose, image=torch.from_numpy(img).cuda(), depth_range=fc.DEPTH_RANGE)
    d = (3, -2, 6)
    window = vol.window(d, SMALL_DIMS)                                # built from the unshifted volume
    vol.shift(d)
    assert vol.origin == window.origin and vol.offset == window.offset == d
    pose = poses[3]                                                   # inside both windows
    a = vol.render(Q, pose, (FRAME_H, FRAME_W))
    b = window.render(Q, pose, (FRAME_H, FRAME_W))
    assert int((a.disparity != -1.0).sum().item()) > 500, "the view must see the surface"
    for name in ("disparity", "depth", "normals", "colors", "weight"):
        ta, tb = getattr(a, name), getattr(b, name)
        if ta.dtype == torch.uint8:
            assert torch.equal(ta, tb), name
        else:
            assert torch.equal(ta.view(torch.int32), tb.view(torch.int32)), name
    frame = torch.from_numpy(maps[3]).cuda()
    guess = np.array(poses[2])
    ra = vol.track(frame, Q, guess, depth_range=fc.DEPTH_RANGE, **fc.TRACKING)
    rb = window.track(frame, Q, guess, depth_range=fc.DEPTH_RANGE, **fc.TRACKING)
    assert not bool(ra.lost) and int(ra.inliers) > 200
    assert torch.equal(ra.pose.view(torch.int32), rb.pose.view(torch.int32))
    assert torch.equal(ra.rms.view(torch.int32), rb.rms.view(torch.int32))
    assert torch.equal(ra.normal_equations.view(torch.int64), rb.normal_equations.view(torch.int64))
    assert (bool(ra.lost), int(ra.iterations), int(ra.inliers), int(ra.accepted)) == \
        (bool(rb.lost), int(rb.iterations), int(rb.inliers), int(rb.accepted))


# ---- graph capture ----------------------------------------------------------------------------------------------------------

def test_graph_replay_of_one_launch(cd, native):
    rng = np.random.default_rng(31)
    dims, start = (67, 9, 6), (-3, 2, 1)
    nx, ny, nz = dims
    state = random_state(rng, dims)
    src = {k: dev_words(v) for k, v in state.items()}
    eager = {k: torch.zeros_like(v) for k, v in src.items()}
    replayed = {k: torch.full_like(v, 0x5A5A5A5A) for k, v in src.items()}

    def launch(out, stream):
        rc = native.LIB.smx_tsdf_window(0, nx, ny, nz, src["tsdf"].data_ptr(), src["weight"].data_ptr(),
                                        src["color"].data_ptr(), *start, nx, ny, nz, out["tsdf"].data_ptr(),
                                        out["weight"].data_ptr(), out["color"].data_ptr(), C.c_void_p(stream))
        assert rc == 0, native.last_error()

    launch(eager, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        launch(replayed, s.cuda_stream)
    torch.cuda.synchronize()
    for f in range(2):
        if f == 1:                                                    # new source values, the same graph
            state = random_state(rng, dims)
            for k in src:
                src[k].copy_(dev_words(state[k]))
            launch(eager, torch.cuda.current_stream().cuda_stream)
        graph.replay()
        torch.cuda.synchronize()
        for k in src:
            want = wref.window_ref(state[k], start, dims)
            assert np.array_equal(replayed[k].cpu().numpy().view(np.uint32), want), f"replay {f}: {k}"
            assert torch.equal(replayed[k], eager[k]), f"replay {f}: {k} against the eager call"
