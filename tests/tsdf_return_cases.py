"""A camera that goes out and comes home (tests/test_tsdf_merge_cpu.py, tests/test_tsdf_merge_gpu.py): the corridor of
tests/tsdf_follow_cases.py seen from a path that backs away from where it started and returns, a small volume that
follows it through a TSDFSpillStore and a large fixed one that holds the same world, and the comparison of the two.

The camera looks along +z and backs away, so what leaves the small volume on the way out is the measured space in front
of it.  The depth range ends 2.4 m from the camera: with the truncation band of 0.375 m that is less than the 3 m from
the volume's anchor to its front face, so while the camera backs away nothing outside the window is measured, and what
left is still what it was when the window comes back."""
import functools

import numpy as np

import tsdf_follow_cases as fc
import tsdf_ref as ref

VS, BIG_DIMS, BIG_ORIGIN, SMALL_DIMS = fc.VS, fc.BIG_DIMS, fc.BIG_ORIGIN, fc.SMALL_DIMS
SMALL_AT = (24, 0, 24)                                               # the small volume's first voxel in the large one
SMALL_ORIGIN = tuple(o + a * VS for o, a in zip(BIG_ORIGIN, SMALL_AT))
DEPTH_RANGE = (0.2, 2.4)
START, STEP, OUT = (0.0, 0.0, 6.0), (-0.15, 0.0, -0.3), 6            # six frames out, six frames home: 13 poses
FRAMES = 2 * OUT + 1


@functools.lru_cache(maxsize=None)
def frames(seed=31):
    """(poses [FRAMES, 4, 4] float64, exact disparity maps [FRAMES, H, W] f32, u8 RGB frames [FRAMES, 3, H, W])."""
    sc, rng = fc.scene(), np.random.default_rng(seed)
    poses, maps, images = [], [], []
    for f in range(FRAMES):
        k = min(f, FRAMES - 1 - f)
        pose = np.eye(4)
        pose[:3, 3] = [s + k * d for s, d in zip(START, STEP)]
        poses.append(pose)
        maps.append(sc.render(pose, fc.FRAME_H, fc.FRAME_W, fc.FX, fc.CX, fc.CY, fc.BASE))
        images.append(rng.integers(0, 256, (3, fc.FRAME_H, fc.FRAME_W)).astype(np.uint8))
    return np.stack(poses), np.stack(maps), np.stack(images)


def crop(words, offset):
    """The small volume's window at `offset` out of the large volume's words [nz, ny, nx]."""
    x0, y0, z0 = (a + b for a, b in zip(SMALL_AT, offset))
    nx, ny, nz = SMALL_DIMS
    assert x0 >= 0 and y0 >= 0 and z0 >= 0 and x0 + nx <= BIG_DIMS[0] and y0 + ny <= BIG_DIMS[1] and z0 + nz <= BIG_DIMS[2]
    return words[z0:z0 + nz, y0:y0 + ny, x0:x0 + nx]


def compare(offsets, changed, small, big, entries, shifts):
    """The comparison both tests make.  offsets[f]: the small volume's offset when frame f was integrated; changed[f]:
    [nz, ny, nx] bool over the large volume, the voxels whose words frame f changed there; small / big: the final
    {"tsdf", "weight", "color"} uint32 words; entries[f]: len(store) after frame f; shifts[f]: the shift before frame f.
    Asserts the conditions on the path and that the final window equals the large volume's crop, bit for bit, on the
    voxels that at every frame lay inside the live window or were not changed in the large volume by that frame.
    Returns (compared voxels, those among them that were outside the window at some frame and end measured)."""
    out = [s for s in shifts[:OUT + 1] if s != (0, 0, 0)]
    home = [s for s in shifts[OUT + 1:] if s != (0, 0, 0)]
    assert len(out) >= 2 and len(home) >= 2, f"need two shifts in each direction, got {shifts}"
    assert offsets[-1] == (0, 0, 0) and offsets[OUT] != (0, 0, 0)
    last = offsets[-1]
    nx, ny, nz = SMALL_DIMS
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    mask = np.ones((nz, ny, nx), bool)
    was_outside = np.zeros((nz, ny, nx), bool)
    for off, ch in zip(offsets, changed):
        inside = np.ones((nz, ny, nx), bool)
        for idx, n, a in ((i, nx, 0), (j, ny, 1), (k, nz, 2)):
            at = idx + last[a] - off[a]
            inside &= (at >= 0) & (at < n)
        mask &= inside | ~crop(ch, last)
        was_outside |= ~inside
    assert mask.mean() >= 0.25, f"only {mask.mean():.3f} of the window can be compared"
    for name in ("tsdf", "weight", "color"):
        bad = np.argwhere((small[name] != crop(big[name], last)) & mask)
        assert bad.size == 0, f"{name}: {len(bad)} voxels differ from the fixed volume, first at (k, j, i) = {tuple(bad[0])}"
    returned = int((mask & was_outside & (small["weight"] != 0)).sum())
    assert returned >= 500, f"only {returned} compared voxels left the window, came back and are measured"
    assert entries[-1] < entries[OUT], f"the store must shrink on the way home: {entries}"
    return int(mask.sum()), returned


def simulate(cd, with_store=True):
    """The whole comparison on the CPU with the twins: tsdf_ref.integrate_ref, and tsdf_merge_ref.NumpyVolume driven by
    cuda_depth.TSDFSpillStore (with_store=False: plain follow, which forgets what left).  Returns compare()'s inputs."""
    import tsdf_merge_ref as mref
    poses, maps, images = frames()
    Q = np.asarray(fc.q_matrix(cd), np.float32)
    P = ref.projection(Q)
    tau, wmax = 3.0 * VS, 64.0

    def to_ref(state):
        return {"tsdf": state["tsdf"].view(np.float32), "weight": state["weight"].view(np.float32),
                "color": np.ascontiguousarray(state["color"]).view(np.uint8).reshape(state["color"].shape + (4,))}

    def integrate(state, dims, origin, f):                           # state: uint32 words, updated in place
        ref.integrate_ref(to_ref(state), dims, origin, VS, tau, wmax, maps[f:f + 1], Q, P, ref.world_to_camera(poses[f]),
                          image=images[f:f + 1], depth_range=DEPTH_RANGE)

    def empty(dims):
        return {k: np.zeros(dims[::-1], np.uint32) for k in ("tsdf", "weight", "color")}

    big = empty(BIG_DIMS)
    small = mref.NumpyVolume(empty(SMALL_DIMS), VS, SMALL_ORIGIN, truncation=tau, max_weight=wmax)
    store = cd.TSDFSpillStore()
    offsets, changed, entries, shifts = [], [], [], []
    for f in range(FRAMES):
        if with_store:
            d, _, _ = store.follow(small, poses[f])
        else:
            d = cd.tsdf_follow_decision(small, poses[f])
            small.shift(d)
        shifts.append(d)
        offsets.append(small.offset)
        entries.append(len(store))
        before = {k: v.copy() for k, v in big.items()}
        integrate(big, BIG_DIMS, BIG_ORIGIN, f)
        changed.append(np.logical_or.reduce([before[k] != big[k] for k in big]))
        integrate(small.state, SMALL_DIMS, small.origin, f)
    return offsets, changed, small.state, big, entries, shifts
