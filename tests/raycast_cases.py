"""The volumes, cameras and parameter sweep that tests/test_raycast_march_cpu.py (the library's per-pixel rule compiled
for the host) and tests/test_raycast_gpu.py (the kernels) both hold against the dense NumPy twin (tests/raycast_ref.py).
The volume is test_tsdf_gpu.py's: 37 x 29 x 41 voxels of 0.05 m -- no multiple of the 8-voxel brick on any axis -- fused by
the TSDF twin from the same bumpy maps and poses.  Every twin result is computed once and shared."""
import functools

import numpy as np

import raycast_ref as rc
import tsdf_ref as ref

f32 = np.float32
DIMS, VS, ORIGIN = (37, 29, 41), 0.05, (-0.9, -0.6, 0.4)
SHAPE = (33, 45)                                                     # no multiple of the 8 x 8 pixel tile
DEPTH_RANGE = (0.0, 3.5)
STEPS = (0.5, 1.0, 2.5)                                              # in voxels
MIN_WEIGHTS = (1.0, 2.5)
QKINDS = ("kitti", "middlebury")


def reprojection(fx, cx, cy, b, fy=None, cx_right=None):
    """cuda_depth.reprojection_matrix, restated."""
    fy = fx if fy is None else fy
    cxr = cx if cx_right is None else cx_right
    return np.array([[1.0, 0.0, 0.0, -cx], [0.0, fx / fy, 0.0, -cy * fx / fy], [0.0, 0.0, 0.0, fx],
                     [0.0, 0.0, 1.0 / b, (cxr - cx) / b]], np.float64).astype(f32)


def q_of(kind, shape=SHAPE):
    H, W = shape
    if kind == "kitti":
        return reprojection(60.0, (W - 1) / 2.0 + 0.25, (H - 1) / 2.0 - 0.5, 0.2)
    if kind == "middlebury":                                         # fy != fx and cx_right; an integer principal point
        return reprojection(60.0, (W - 1) / 2.0, (H - 1) / 2.0, 0.2, fy=61.0, cx_right=(W - 1) / 2.0 + 4.5)
    return reprojection(60.0, (W - 1) / 2.0, (H - 1) / 2.0, 0.2)     # "centred": KITTI-style, integer principal point


def fusion_poses(n, rng):
    out = []
    for _ in range(n):
        eye = np.array([0.0, 0.0, -0.5]) + rng.uniform(-0.15, 0.15, 3)
        out.append(ref.look_at(eye, np.array([0.0, 0.1, 1.6]) + rng.uniform(-0.2, 0.2, 3)))
    return np.stack(out)


def fusion_maps(rng, n, H, W, zmean=1.5):
    """Disparities of a bumpy surface near depth zmean for f*B = 12, with invalid, NaN and outlier pixels."""
    v, u = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    d = np.empty((n, H, W), f32)
    for f in range(n):
        z = zmean + 0.3 * np.sin(u / 9.0 + f) * np.cos(v / 7.0) + rng.normal(0, 0.01, (H, W))
        d[f] = (12.0 / z).astype(f32)
    r = rng.random((n, H, W))
    d[r < 0.05] = -1.0
    d[(r >= 0.05) & (r < 0.06)] = np.nan
    d[(r >= 0.06) & (r < 0.07)] = rng.uniform(1.0, 40.0, int(((r >= 0.06) & (r < 0.07)).sum()))
    return d


@functools.lru_cache(maxsize=None)
def fused_state(colour=True, corner=False):
    """The twin-fused volume (read only: copy before changing it).  corner: only the upper left quarter of every map is
    valid, so the volume is measured in one corner and most of its bricks are empty."""
    rng = np.random.default_rng(11)
    H, W = 40, 56
    Q = reprojection(60.0, (W - 1) / 2.0 + 0.25, (H - 1) / 2.0 - 0.5, 0.2)
    state = ref.empty_state(DIMS, colour)
    for _ in range(2):
        d = fusion_maps(rng, 4, H, W)
        if corner:
            d[:, H // 2:, :] = -1.0
            d[:, :, W // 2:] = -1.0
        img = rng.integers(0, 256, (4, 3, H, W)).astype(np.uint8) if colour else None
        ref.integrate_ref(state, DIMS, ORIGIN, VS, 3 * VS, 64.0, d, Q, ref.projection(Q),
                          ref.world_to_camera(fusion_poses(4, rng)), image=img)
    for a in state.values():
        if a is not None:
            a.setflags(write=False)
    return state


@functools.lru_cache(maxsize=None)
def analytic_state():
    """A ball of radius 8 voxels in measured free space (tsdf exactly 1 beyond three voxels from its surface), with the
    low-x fifth of the volume unmeasured: bricks of all three kinds -- empty, mixed and free space."""
    nx, ny, nz = DIMS
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    dist = np.sqrt((i - 22.0) ** 2 + (j - 14.0) ** 2 + (k - 24.0) ** 2) - 8.0
    state = ref.empty_state(DIMS, True)
    state["tsdf"][:] = np.clip(dist / 3.0, -1.0, 1.0).astype(f32)
    state["weight"][:] = np.where(i < 8, 0.0, 2.0).astype(f32)
    state["color"][..., :3] = np.stack([i * 6, j * 8, k * 6], -1).astype(np.uint8)
    for a in state.values():
        a.setflags(write=False)
    return state


@functools.lru_cache(maxsize=None)
def expected_analytic(names, step_voxels):
    return rc.raycast_ref(analytic_state(), DIMS, ORIGIN, VS, q_of("kitti"), rc.view_pose(poses_of(names)), SHAPE,
                          min_weight=1.0, step=f32(VS) * f32(step_voxels), depth_range=DEPTH_RANGE)


def occupied_bricks(state, min_weight):
    """The fraction of the 8 x 8 x 8 bricks that hold a voxel of weight >= min_weight."""
    w = state["weight"] >= f32(min_weight)
    nz, ny, nx = w.shape
    pad = np.zeros(((nz + 7) // 8 * 8, (ny + 7) // 8 * 8, (nx + 7) // 8 * 8), bool)
    pad[:nz, :ny, :nx] = w
    return pad.reshape(pad.shape[0] // 8, 8, pad.shape[1] // 8, 8, pad.shape[2] // 8, 8).any(axis=(1, 3, 5)).mean()


VIEWS = {
    "outside": ref.look_at((0.1, -0.05, -0.5), (0.0, 0.1, 1.6)),
    "inside": ref.look_at((0.0, 0.1, 1.0), (0.05, 0.12, 1.9)),
    "behind": ref.look_at((0.0, 0.0, -0.3), (0.1, 0.0, -1.3)),       # looking away: every pixel invalid
    "oblique": ref.look_at((1.6, -0.9, 0.2), (0.0, 0.2, 1.5)),       # enters through a side face
}


def aligned_pose():
    """Looking exactly along +z from the centre of voxel (18, 14, 2): with an integer principal point the centre column
    and row have a zero direction component."""
    m = np.eye(4)
    m[:3, 3] = [ORIGIN[0] + 18.5 * VS, ORIGIN[1] + 14.5 * VS, ORIGIN[2] + 2.5 * VS]
    return m


def poses_of(names):
    return np.stack([aligned_pose() if k == "aligned" else VIEWS[k] for k in names])


@functools.lru_cache(maxsize=None)
def expected(names, qkind, step_voxels, min_weight, colour=True, corner=False, depth_range=DEPTH_RANGE):
    """The twin's outputs for the views `names` (a tuple) of fused_state(colour, corner)."""
    return rc.raycast_ref(fused_state(colour, corner), DIMS, ORIGIN, VS, q_of(qkind), rc.view_pose(poses_of(names)), SHAPE,
                          min_weight=min_weight, step=f32(VS) * f32(step_voxels), depth_range=depth_range)


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_same(got, want, what):
    """got / want: dicts of the five outputs; float planes compare by bit pattern (NaN depth included)."""
    for key in ("disparity", "depth", "normals", "weight"):
        if got.get(key) is None:
            continue
        g, e = bits(got[key]), bits(want[key])
        assert g.shape == e.shape, f"{what}: {key} shape {g.shape} != {e.shape}"
        bad = np.argwhere(g != e)
        assert bad.size == 0, f"{what}: {key}: {len(bad)} values differ, first at {tuple(bad[0])}"
    if got.get("colors") is not None:
        assert np.array_equal(got["colors"], want["colors"]), f"{what}: colors"
