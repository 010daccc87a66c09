"""Merging TSDF volumes on the device (include/stereo_mi355x.h: smx_tsdf_merge) and what is built on it.  The kernel
against its NumPy twin (tests/tsdf_merge_ref.py) as 32-bit words, the destination inside guard bands; TSDFVolume.merge's
placement, region and refusals; two volumes fused from the even and the odd frames, merged, against one volume fused from
all of them; volumes moved out and back through a TSDFSpillStore, word for word; a camera that goes out and comes home,
followed through the store, against a large fixed volume, bit for bit; graph replay; the pipeline's spill_store."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import tsdf_follow_cases as fc                      # noqa: E402
import tsdf_merge_ref as mref                       # noqa: E402
import tsdf_return_cases as rc                      # noqa: E402
import tsdf_window_ref as wref                      # noqa: E402

SENTINEL = 0xDEADBEEF
GUARDS = (5, 6, 7)                                   # words before each destination array: three 16-byte phases
DEST_DIMS = [(13, 7, 5), (67, 9, 6), (517, 3, 2)]    # odd widths: row starts at every 16-byte phase
SOURCE_DIMS = [(5, 3, 2), (3, 7, 9), (131, 4, 3), (300, 2, 2)]      # (3, 7, 9): narrower than a quad
# (300, 2, 2) on the 517 destination: rows of more than 64 quads, a lane's second trip
LONG_X0 = (-257, -1, 0, 1, 2, 3, 255)
# a lane takes two quads per trip: rows of more than 128 quads for its second trip, at every phase and past both ends
LONGER = {(1100, 1, 2): [(1061, 1, 2)]}
LONGER_X0 = (-530, -3, -1, 0, 1, 2, 3, 36, 39, 40, 600)
MIXED = [(-2, 1, -1), (3, -2, 2), (-5, -3, 4), (1, 1, 1), (-1, -1, -1), (4, -6, -2), (7, 0, -3), (2, 3, 1)]
MAX_WEIGHT = 3.0                                     # 2.5 + 1 and 2.5 + 2.5 reach the cap, 1 + 1 does not
WEIGHTS = np.array([0.0, -0.0, 1.0, 2.5, MAX_WEIGHT, -2.0, np.nan], np.float32).view(np.uint32)


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
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda()


def words(t: "torch.Tensor") -> np.ndarray:
    a = t.detach().cpu().contiguous().numpy()
    if a.dtype == np.uint8:
        return a.view(np.uint32)[..., 0]
    return a.view(np.uint32)


def load_state(vol, state):
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


def placements_for(dst, src):
    """Per axis around both ends of the destination (n) for a source of s voxels, then mixed; the long rows: LONG_X0."""
    if dst == (517, 3, 2) and src == (300, 2, 2):
        return [(x0, 0, 0) for x0 in LONG_X0] + [(x0, 1, -1) for x0 in LONG_X0[::3]] + [(217, 0, 0), (218, 1, 0)]
    if dst in LONGER:
        return [(x0, 0, 0) for x0 in LONGER_X0] + [(x0, 0, 1) for x0 in LONGER_X0[::3]] + [(1, 0, -1)]
    out = []
    for axis in range(3):
        n, s = dst[axis], src[axis]
        for v in sorted({-s - 1, -s, -(s - 1), -5, -1, 0, 1, 3, 4, n - s - 1, n - s, n - s + 1, n - 1, n, n + 1}):
            p = [0, 0, 0]
            p[axis] = v
            out.append(tuple(p))
    return out + MIXED


def regions_for(src, index):
    """The whole source, a 1-voxel region and strict sub-boxes, in turn."""
    sx, sy, sz = src
    kinds = [None, ((sx // 2, sy // 2, sz // 2), (1, 1, 1)),
             ((min(1, sx - 1), 0, min(1, sz - 1)), (max(1, sx - 2), sy, max(1, sz - 1))),
             ((0, min(1, sy - 1), 0), (max(1, sx - 1), max(1, sy - 1), sz)),
             ((sx - 1, 0, 0), (1, sy, sz))]
    return kinds[index % len(kinds)]


def make_state(rng, dims, colour, wild):
    """Weights from WEIGHTS.  wild (FILL, where the rule only copies or skips): any bits in tsdf and colour, NaNs,
    infinities and denormals planted.  Otherwise (AVERAGE) finite tsdf in [-1, 1] and a zero fourth colour byte where the
    weight is > 0 -- where the arithmetic can run -- and wild words where it is not: those are skipped or overwritten."""
    nx, ny, nz = dims
    shape = (nz, ny, nx)
    weight = rng.choice(WEIGHTS, shape)
    tsdf, col = wref.random_words(rng, shape), wref.random_words(rng, shape)
    if not wild:
        with np.errstate(invalid="ignore"):
            on = weight.view(np.float32) > 0
        tsdf = np.where(on, rng.uniform(-1, 1, shape).astype(np.float32).view(np.uint32), tsdf)
        col = np.where(on, col & np.uint32(0xFFFFFF), col)
    return {"tsdf": tsdf, "weight": weight, "color": col if colour else None}


# ---- the kernel against the twin ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("colour", [True, False])
@pytest.mark.parametrize("mode", ["fill", "average"])
@pytest.mark.parametrize("dims", DEST_DIMS + list(LONGER))
def test_kernel_matches_the_twin(native, dims, mode, colour):
    rng = np.random.default_rng(sum(dims) + 2 * colour + (mode == "fill"))
    nx, ny, nz = dims
    count = nx * ny * nz
    names = ("tsdf", "weight", "color")[:3 if colour else 2]
    dst_state = make_state(rng, dims, colour, mode == "fill")
    dst_dev = {k: dev_words(dst_state[k]).reshape(-1) for k in names}
    bufs = {k: torch.empty(g + count + 9, dtype=torch.int32, device="cuda") for k, g in zip(names, GUARDS)}
    ptr = {k: bufs[k].data_ptr() + 4 * g for k, g in zip(names, GUARDS)}
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    changed_calls = 0
    for src_dims in LONGER.get(dims, SOURCE_DIMS):
        sx, sy, sz = src_dims
        src_state = make_state(rng, src_dims, colour, mode == "fill")
        src = {k: dev_words(src_state[k]) for k in names}
        pending = []
        for index, placement in enumerate(placements_for(dims, src_dims)):
            region = regions_for(src_dims, index)
            start, size = ((0, 0, 0), src_dims) if region is None else region
            for k, g in zip(names, GUARDS):
                bufs[k].fill_(SENTINEL - 2 ** 32)
                bufs[k][g:g + count].copy_(dst_dev[k])
            rc_ = native.LIB.smx_tsdf_merge(0, nx, ny, nz, ptr["tsdf"], ptr["weight"], ptr["color"] if colour else None,
                                            sx, sy, sz, src["tsdf"].data_ptr(), src["weight"].data_ptr(),
                                            src["color"].data_ptr() if colour else None, *placement, *start, *size,
                                            native.TSDF_MERGE_MODES[mode], MAX_WEIGHT, stream)
            assert rc_ == 0, native.last_error()
            pending.append((placement, region, {k: b.clone() for k, b in bufs.items()}))
        torch.cuda.synchronize()
        for k in names:
            assert np.array_equal(src[k].cpu().numpy().view(np.uint32), src_state[k]), f"the source's {k} was written"
        for placement, region, outs in pending:
            want = mref.merge_ref(dst_state, src_state, placement, region, mode, MAX_WEIGHT)
            changed_calls += any(not np.array_equal(want[k], dst_state[k]) for k in names)
            for k, g in zip(names, GUARDS):
                got = outs[k].cpu().numpy().view(np.uint32)
                what = f"{k} of {mode} {src_dims} at {placement} region {region} into {dims}"
                assert (got[:g] == SENTINEL).all() and (got[g + count:] == SENTINEL).all(), f"{what}: guard band written"
                bad = np.argwhere(got[g:g + count].reshape(nz, ny, nx) != want[k])
                assert bad.size == 0, f"{what}: {len(bad)} words differ, first at (k, j, i) = {tuple(bad[0])}"
    # of five region kinds the 1-voxel region and the single column seldom meet a pair that changes; the others must
    assert changed_calls >= (5 if dims in LONGER else 40), f"only {changed_calls} calls changed the destination"


def test_a_region_outside_the_destination_writes_nothing(native):
    """The source overlaps the destination, the region does not: no word is written and the call returns 0."""
    rng = np.random.default_rng(7)
    dims, src_dims = (13, 7, 5), (5, 3, 2)
    dst_state, src_state = make_state(rng, dims, True, True), make_state(rng, src_dims, True, True)
    src_state["weight"][:] = WEIGHTS[2]                               # every source voxel is measured
    dst = {k: dev_words(v) for k, v in dst_state.items()}
    src = {k: dev_words(v) for k, v in src_state.items()}
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for placement, region in (((-2, 0, 0), ((0, 0, 0), (2, 3, 2))), ((10, 0, 0), ((3, 0, 0), (2, 3, 2))),
                              ((0, -1, 0), ((0, 0, 0), (5, 1, 2))), ((0, 0, 4), ((0, 0, 1), (5, 3, 1))),
                              ((0, 6, 0), ((2, 1, 0), (1, 2, 1))), ((-8192, 8192, 0), ((0, 0, 0), (5, 3, 2)))):
        for mode in (0, 1):
            rc_ = native.LIB.smx_tsdf_merge(0, *dims, dst["tsdf"].data_ptr(), dst["weight"].data_ptr(),
                                            dst["color"].data_ptr(), *src_dims, src["tsdf"].data_ptr(),
                                            src["weight"].data_ptr(), src["color"].data_ptr(), *placement, *region[0],
                                            *region[1], mode, MAX_WEIGHT, stream)
            assert rc_ == 0, native.last_error()
    torch.cuda.synchronize()
    for k in dst:
        assert np.array_equal(dst[k].cpu().numpy().view(np.uint32), dst_state[k]), k
    # the neighbouring region does write
    rc_ = native.LIB.smx_tsdf_merge(0, *dims, dst["tsdf"].data_ptr(), dst["weight"].data_ptr(), dst["color"].data_ptr(),
                                    *src_dims, src["tsdf"].data_ptr(), src["weight"].data_ptr(), src["color"].data_ptr(),
                                    -2, 0, 0, 2, 0, 0, 1, 3, 2, 0, MAX_WEIGHT, stream)
    assert rc_ == 0
    want = mref.merge_ref(dst_state, src_state, (-2, 0, 0), ((2, 0, 0), (1, 3, 2)), "fill", MAX_WEIGHT)
    assert not np.array_equal(want["weight"], dst_state["weight"])
    assert_state({k: v.cpu().numpy().view(np.uint32) for k, v in dst.items()}, want, "the region beside it")


# ---- TSDFVolume.merge -----------------------------------------------------------------------------------------------------

def test_merge_places_volumes_by_their_offsets_and_origins(cd):
    rng = np.random.default_rng(13)
    vs, origin = 0.125, (-1.0, 0.5, 2.0)
    for colour in (True, False):
        dst = cd.TSDFVolume((13, 7, 5), vs, origin, color=colour, truncation=0.5, max_weight=MAX_WEIGHT)
        dst_state = make_state(rng, (13, 7, 5), colour, False)
        load_state(dst, dst_state)
        dst.shift((2, -1, 1))                                         # a volume that has moved
        dst_state = wref.window_state(dst_state, (2, -1, 1), (13, 7, 5))
        big = cd.TSDFVolume((16, 7, 9), vs, origin, color=colour, truncation=0.5, max_weight=MAX_WEIGHT)
        big_state = make_state(rng, (16, 7, 9), colour, False)
        load_state(big, big_state)
        src = big.window((3, 1, -2), (8, 6, 7)).window((1, 0, 1), (6, 5, 5))     # a window of a window: offset (4, 1, -1)
        src_state = wref.window_state(big_state, (4, 1, -1), (6, 5, 5))
        assert src.offset == (4, 1, -1)
        for mode, region in (("average", None), ("fill", None), ("average", ((1, 0, 2), (4, 5, 2)))):
            before = volume_words(dst)
            assert_state(before, dst_state, "before the merge")
            dst.merge(src, **({} if (mode, region) == ("average", None) else dict(mode=mode, region=region)))
            dst_state = mref.merge_ref(dst_state, src_state, (2, 2, -2), region, mode, MAX_WEIGHT)
            assert_state(volume_words(dst), dst_state, f"merge {mode} {region} colour {colour}")
            assert_state(volume_words(src), src_state, "the source is untouched")
        assert dst.offset == (2, -1, 1)
        # two constructor origins a whole number of voxels apart
        apart = cd.TSDFVolume((6, 5, 5), vs, tuple(o + k * vs for o, k in zip(origin, (3, -2, 1))), color=colour,
                              truncation=0.5, max_weight=MAX_WEIGHT)
        load_state(apart, src_state)
        apart.shift((1, 0, 0))
        moved = wref.window_state(src_state, (1, 0, 0), (6, 5, 5))
        dst.merge(apart, mode="average")
        dst_state = mref.merge_ref(dst_state, moved, (3 + 1 - 2, -2 + 1, 1 - 1), None, "average", MAX_WEIGHT)
        assert_state(volume_words(dst), dst_state, "origins three, two and one voxels apart")


def test_merge_refusals_on_the_device(cd):
    vs, origin = 0.125, (0.0, 0.0, 0.0)
    a = cd.TSDFVolume((8, 6, 5), vs, origin, truncation=0.5)
    before = volume_words(a)
    with pytest.raises(RuntimeError, match="whole"):
        a.merge(cd.TSDFVolume((8, 6, 5), vs, (0.0625, 0.0, 0.0), truncation=0.5))
    with pytest.raises(RuntimeError, match="voxel_size"):
        a.merge(cd.TSDFVolume((8, 6, 5), 0.25, origin, truncation=0.5))
    with pytest.raises(RuntimeError, match="truncation"):
        a.merge(cd.TSDFVolume((8, 6, 5), vs, origin, truncation=0.75))
    with pytest.raises(RuntimeError, match="max_weight"):
        a.merge(cd.TSDFVolume((8, 6, 5), vs, origin, truncation=0.5, max_weight=8.0))
    with pytest.raises(RuntimeError, match="colour"):
        a.merge(cd.TSDFVolume((8, 6, 5), vs, origin, truncation=0.5, color=False))
    with pytest.raises(RuntimeError, match="itself"):
        a.merge(a)
    b = cd.TSDFVolume((4, 3, 2), vs, origin, truncation=0.5)
    with pytest.raises(RuntimeError, match="region"):
        a.merge(b, region=((0, 0, 0), (5, 3, 2)))
    with pytest.raises(RuntimeError, match="mode"):
        a.merge(b, mode="sum")
    torch.cuda.synchronize()
    assert_state(volume_words(a), before, "a refused merge")


# ---- two halves against the whole -----------------------------------------------------------------------------------------

def test_two_halves_merged_equal_the_whole(cd):
    """Even frames into A, odd frames into B, A.merge(B), against all frames into one volume.  The weights are sums of
    ones below the cap: equal bit for bit.  Each fusion step is 4 roundings of at most 2^-24 at |T| <= 1 and a weighted
    mean does not amplify an error, so either path is within 4 * steps * 2^-24 of the exact value: 8 steps one way, 4 and
    then the merge's one the other."""
    Q = fc.q_matrix(cd)
    poses, maps, images = fc.path_frames(8)
    vols = [cd.TSDFVolume(fc.BIG_DIMS, fc.VS, fc.BIG_ORIGIN, max_weight=64.0) for _ in range(3)]
    a, b, whole = vols
    for f, (pose, d, img) in enumerate(zip(poses, maps, images)):
        td, ti = torch.from_numpy(d).cuda(), torch.from_numpy(img).cuda()
        whole.integrate(td, Q, pose, image=ti, depth_range=fc.DEPTH_RANGE)
        (a, b)[f % 2].integrate(td, Q, pose, image=ti, depth_range=fc.DEPTH_RANGE)
    both = int(((a.weight > 0) & (b.weight > 0)).sum().item())
    assert both >= 2000, f"only {both} voxels were measured in both halves"
    b_before = volume_words(b)
    a.merge(b)
    assert torch.equal(a.weight.view(torch.int32), whole.weight.view(torch.int32)), "the weights differ"
    assert 4.0 <= float(whole.weight.max().item()) <= 8.0, "the cap must not bind"
    diff = float((a.tsdf.double() - whole.tsdf.double()).abs().max().item())
    bound = 4 * (8 + 5) * 2.0 ** -24
    print(f"max |dT| = {diff:.3e}, bound {bound:.3e}")
    assert diff <= bound
    assert float(whole.tsdf.abs().max().item()) <= 1.0
    assert_state(volume_words(b), b_before, "the merged-in half is untouched")


# ---- there and back through the store -------------------------------------------------------------------------------------

@pytest.mark.parametrize("margin", [0, 1, 2])
@pytest.mark.parametrize("steps", mref.OUT_AND_BACK)
def test_store_out_and_back(cd, steps, margin):
    rng = np.random.default_rng(5 + margin)
    for colour in (True, False):
        first = mref.plausible_state(rng, (13, 7, 5), colour)
        vol = cd.TSDFVolume((13, 7, 5), 0.125, (0.5, -1.0, 2.0), color=colour)
        load_state(vol, first)
        store = cd.TSDFSpillStore()
        held = merges = 0
        for d in mref.full_path(steps):
            boxes, restored = store.shift(vol, d, margin=margin)
            assert len(boxes) == sum(c != 0 for c in d) and all(isinstance(b, cd.TSDFVolume) for b in boxes)
            assert all(b.tsdf.is_cuda for b in store.volumes())
            held, merges = max(held, len(store)), merges + restored
        assert held >= 1 and merges >= 1
        assert vol.offset == (0, 0, 0) and vol.origin == (0.5, -1.0, 2.0)
        assert_state(volume_words(vol), first, f"{steps} margin {margin} colour {colour}")
        assert len(store) == 0 and store.bytes == 0 and store.evicted == 0


# ---- a returning camera against a fixed volume ----------------------------------------------------------------------------

def follow_the_path(cd, small, big, follow):
    """Both volumes over the frames of tests/tsdf_return_cases.py; follow(pose) moves the small one and returns
    (shift, len(store)).  Returns compare()'s inputs."""
    Q = fc.q_matrix(cd)
    poses, maps, images = rc.frames()
    offsets, changed, entries, shifts = [], [], [], []
    for pose, d, img in zip(poses, maps, images):
        shift, held = follow(pose)
        shifts.append(shift)
        offsets.append(small.offset)
        entries.append(held)
        td, ti = torch.from_numpy(d).cuda(), torch.from_numpy(img).cuda()
        before = [t.clone() for t in (big.tsdf, big.weight, big.color)]
        big.integrate(td, Q, pose, image=ti, depth_range=rc.DEPTH_RANGE)
        ch = (before[0].view(torch.int32) != big.tsdf.view(torch.int32)) | \
            (before[1].view(torch.int32) != big.weight.view(torch.int32)) | \
            (before[2].view(torch.int32)[..., 0] != big.color.view(torch.int32)[..., 0])
        changed.append(ch.cpu().numpy())
        small.integrate(td, Q, pose, image=ti, depth_range=rc.DEPTH_RANGE)
    return offsets, changed, volume_words(small), volume_words(big), entries, shifts


def test_a_returning_camera_finds_its_model(cd):
    big = cd.TSDFVolume(rc.BIG_DIMS, rc.VS, rc.BIG_ORIGIN)
    small = cd.TSDFVolume(rc.SMALL_DIMS, rc.VS, rc.SMALL_ORIGIN)
    store = cd.TSDFSpillStore()

    def follow(pose):
        d, boxes, restored = store.follow(small, pose)
        assert (restored > 0) <= (d != (0, 0, 0))
        return d, len(store)

    compared, returned = rc.compare(*follow_the_path(cd, small, big, follow))
    print(f"{compared} voxels compared, {returned} of them left the window, came back and are measured")
    assert len(store) == 0


# ---- graph capture --------------------------------------------------------------------------------------------------------

def test_graph_replay_of_one_launch(cd, native):
    rng = np.random.default_rng(31)
    dims, src_dims, placement = (67, 9, 6), (131, 4, 3), (-70, 2, 1)
    dst_state, src_state = make_state(rng, dims, True, False), make_state(rng, src_dims, True, False)
    src = {k: dev_words(v) for k, v in src_state.items()}
    eager = {k: dev_words(v) for k, v in dst_state.items()}
    replayed = {k: dev_words(v) for k, v in dst_state.items()}

    def launch(out, stream):
        rc_ = native.LIB.smx_tsdf_merge(0, *dims, out["tsdf"].data_ptr(), out["weight"].data_ptr(), out["color"].data_ptr(),
                                        *src_dims, src["tsdf"].data_ptr(), src["weight"].data_ptr(),
                                        src["color"].data_ptr(), *placement, 0, 0, 0, *src_dims, 1, MAX_WEIGHT,
                                        C.c_void_p(stream))
        assert rc_ == 0, native.last_error()

    s = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        launch(replayed, s.cuda_stream)
    torch.cuda.synchronize()
    want = dst_state
    for f in range(2):
        if f == 1:                                                    # new source values, the same graph
            src_state = make_state(rng, src_dims, True, False)
            for k in src:
                src[k].copy_(dev_words(src_state[k]))
        for k in replayed:                                            # capture ran nothing: the destination is as loaded
            assert np.array_equal(replayed[k].cpu().numpy().view(np.uint32), want[k]), f"before replay {f}: {k}"
        launch(eager, torch.cuda.current_stream().cuda_stream)
        graph.replay()
        torch.cuda.synchronize()
        want = mref.merge_ref(want, src_state, placement, None, "average", MAX_WEIGHT)
        for k in src:
            assert np.array_equal(replayed[k].cpu().numpy().view(np.uint32), want[k]), f"replay {f}: {k}"
            assert torch.equal(replayed[k], eager[k]), f"replay {f}: {k} against the eager call"


# ---- the pipeline ---------------------------------------------------------------------------------------------------------

def run_pipeline(cd, **keywords):
    from pipeline import DepthEstimationPipeline, DepthEstimationPipelineConfig
    poses, maps, images = rc.frames()
    cfg = DepthEstimationPipelineConfig(image_shape=(fc.FRAME_H, fc.FRAME_W), min_disparity=0, max_disparity=15,
                                        stereo_matching_backend="cuda")
    vol = cd.TSDFVolume(rc.SMALL_DIMS, rc.VS, rc.SMALL_ORIGIN)
    pipe = DepthEstimationPipeline(cfg, reprojection_matrix=fc.q_matrix(cd), tsdf_volume=vol,
                                   point_cloud_depth_range=rc.DEPTH_RANGE, follow_camera=True, **keywords)
    feed = iter([torch.from_numpy(m).cuda() for m in maps])
    pipe._stereo_matching.process = lambda left, right: next(feed)    # the maps are the sequence's, not matched
    results = [pipe.process(torch.from_numpy(img), torch.from_numpy(img), camera_pose=pose)
               for img, pose in zip(images, poses)]
    return results, vol


def manual_loop(cd, follow):
    """The volume after the frames with follow(volume, pose) before each, and what follow returned."""
    Q = fc.q_matrix(cd)
    poses, maps, images = rc.frames()
    vol = cd.TSDFVolume(rc.SMALL_DIMS, rc.VS, rc.SMALL_ORIGIN)
    returned = []
    for pose, d, img in zip(poses, maps, images):
        returned.append(follow(vol, pose))
        vol.integrate(torch.from_numpy(d).cuda(), Q, pose, image=torch.from_numpy(img).cuda(), depth_range=rc.DEPTH_RANGE)
    return returned, vol


def test_pipeline_follows_through_the_store(cd):
    store = cd.TSDFSpillStore()
    results, vol = run_pipeline(cd, spill_store=store)
    manual_store = cd.TSDFSpillStore()
    returned, manual = manual_loop(cd, lambda v, pose: manual_store.follow(v, pose))
    assert [r.volume_shift for r in results] == [d for d, _, _ in returned]
    assert [r.restored_boxes for r in results] == [n for _, _, n in returned]
    assert sum(r.restored_boxes for r in results) >= 2 and vol.offset == manual.offset == (0, 0, 0)
    assert all(r.spilled_volumes == [] for r in results)
    assert_state(volume_words(vol), volume_words(manual), "the pipeline's volume against the manual loop's")
    assert len(store) == len(manual_store) == 0
    kept, _ = run_pipeline(cd, spill_store=cd.TSDFSpillStore(), keep_spill=True)
    assert [len(r.spilled_volumes) for r in kept] == [sum(c != 0 for c in r.volume_shift) for r in kept]


def test_pipeline_without_a_store_is_unchanged(cd):
    results, vol = run_pipeline(cd)
    returned, manual = manual_loop(cd, lambda v, pose: v.follow(pose))
    assert [r.volume_shift for r in results] == [d for d, _ in returned]
    assert all(r.restored_boxes == 0 and r.spilled_volumes == [] for r in results)
    assert_state(volume_words(vol), volume_words(manual), "follow_camera without a store")
    with_store, _ = run_pipeline(cd, spill_store=cd.TSDFSpillStore())
    assert [r.volume_shift for r in with_store] == [r.volume_shift for r in results]
