"""smx_tsdf_extract_triangles on the device, bit for bit against the NumPy reference (tests/mesh_ref.py): volumes fused
on the device, directly filled states (sphere, random field, invalid voxels), rows of every width around the wave size,
flat volumes, a volume of 8 M voxels, a capacity below the total, the vertices against extract_point_cloud, determinism
and graph replay.  The table itself is checked in test_mesh_cpu.py."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import mesh_ref                                     # noqa: E402
import test_tsdf_gpu as tg                          # noqa: E402  (its volumes, maps and poses)
import tsdf_ref as ref                              # noqa: E402

SENTINEL = -77


@pytest.fixture(scope="module")
def cd():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import cuda_depth
    return cuda_depth


def device_triangles(tsdf, weight, min_weight, capacity, stream=None):
    """The raw call on device tensors [nz, ny, nx]: (triangles [capacity + 3, 3] prefilled with SENTINEL, count [1])."""
    import cuda_depth._native as native
    nz, ny, nx = tsdf.shape
    tris = torch.full((capacity + 3, 3), SENTINEL, dtype=torch.int32, device="cuda")
    count = torch.full((1,), SENTINEL, dtype=torch.int32, device="cuda")
    ws_bytes = native.LIB.smx_tsdf_extract_triangles_workspace_bytes(nx, ny, nz)
    assert ws_bytes > 0
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream if stream is None else stream.cuda_stream
    rc = native.LIB.smx_tsdf_extract_triangles(0, nx, ny, nz, tsdf.data_ptr(), weight.data_ptr(), min_weight, capacity,
                                               tris.data_ptr(), count.data_ptr(), ws.data_ptr(), ws_bytes, C.c_void_p(s))
    assert rc == 0, native.last_error()
    return tris, count, ws


def check_state(state, min_weight=1.0, what=""):
    """Runs the device on a host state with room for everything, and with a capacity below the total."""
    want, n, _ = mesh_ref.triangles_ref(state, min_weight)
    T, Wt = tg.dev(state["tsdf"]), tg.dev(state["weight"])
    tris, count, _ = device_triangles(T, Wt, min_weight, max(len(want), 1))
    torch.cuda.synchronize()
    got = tris.cpu().numpy()
    assert int(count.item()) == len(want), f"{what}: count {int(count.item())} != {len(want)}"
    bad = np.argwhere(got[:len(want)] != want)
    assert bad.size == 0, f"{what}: {len(bad)} indices differ, first at {tuple(bad[0])}"
    assert (got[len(want):] == SENTINEL).all(), f"{what}: written past the total"
    if len(want) > 3:
        cap = len(want) // 3
        tris, count, _ = device_triangles(T, Wt, min_weight, cap)
        torch.cuda.synchronize()
        got = tris.cpu().numpy()
        assert int(count.item()) == len(want), f"{what}: the count must be the total"
        assert np.array_equal(got[:cap], want[:cap]), f"{what}: prefix"
        assert (got[cap:] == SENTINEL).all(), f"{what}: written past the capacity"
    return want, n


def rough_state(dims, seed, holes=True):
    """A random field in (-0.9, 0.9) of weight 2, with (holes) voxels of weight 0, 0.5 and NaN and of T = 1, -1 and NaN
    sprinkled in."""
    nx, ny, nz = dims
    rng = np.random.default_rng(seed)
    T = rng.uniform(-0.9, 0.9, (nz, ny, nx)).astype(np.float32)
    Wt = np.full((nz, ny, nx), 2.0, np.float32)
    if holes:
        r = rng.random((nz, ny, nx))
        Wt[r < 0.04] = 0.0
        Wt[(r >= 0.04) & (r < 0.08)] = 0.5
        T[(r >= 0.08) & (r < 0.10)] = 1.0
        T[(r >= 0.10) & (r < 0.12)] = -1.0
        T[(r >= 0.12) & (r < 0.13)] = np.nan
        Wt[(r >= 0.13) & (r < 0.14)] = np.nan
    return {"tsdf": T, "weight": Wt, "color": None}


@pytest.mark.parametrize("min_weight", [1.0, 2.5])
def test_fused_volume(cd, min_weight):
    rng = np.random.default_rng(11)
    vol, state = tg.filled_volume(cd, rng)
    tg.assert_volume(vol, state, "fill")
    want, n, where = mesh_ref.triangles_ref(state, min_weight)
    assert len(want) > 100
    check_state(state, min_weight, f"fused {min_weight}")
    # the Python surface: the vertices are extract_point_cloud's, bit for bit, the triangles the reference's
    cloud = vol.extract_point_cloud(min_weight=min_weight)
    vol._capacity = 5                                               # too small: one retry with the exact counts
    mesh = vol.extract_triangle_mesh(min_weight=min_weight)
    assert isinstance(mesh, cd.TriangleMesh) and mesh.triangles.dtype == torch.int32
    assert mesh.vertices.shape == (n, 3) and vol._capacity == n
    assert torch.equal(mesh.vertices.view(torch.int32), cloud.points.view(torch.int32))
    assert torch.equal(mesh.normals.view(torch.int32), cloud.normals.view(torch.int32))
    assert torch.equal(mesh.colors, cloud.colors)
    assert np.array_equal(mesh.triangles.cpu().numpy(), want)
    assert vol.extract_triangle_mesh(min_weight=min_weight, normals=False).normals is None
    # every index names a vertex on an edge of the triangle's cell
    p = (mesh.vertices.cpu().numpy().astype(np.float64) - np.asarray(tg.ORIGIN)) / tg.VS - 0.5
    for m in range(3):
        u = p[want[:, m]] - where
        assert (u > -1e-3).all() and (u < 1 + 1e-3).all(), "a vertex outside its triangle's cell"
        on_lattice = (np.abs(u) < 1e-3) | (np.abs(u - 1) < 1e-3)
        assert (on_lattice.sum(axis=1) >= 2).all(), "a vertex off the edges of its triangle's cell"


def test_sphere_and_random_field(cd):
    st = mesh_ref.state_from_sdf(mesh_ref.spheres_sdf((33, 31, 35), [(15.3, 14.6, 17.1)], 9.0))
    want, _ = check_state(st, 1.0, "sphere")
    assert len(want) > 1000
    want, _ = check_state(mesh_ref.random_state((24, 25, 26), seed=7), 1.0, "random field")
    assert len(want) > 20000


@pytest.mark.parametrize("dims", [(1, 5, 4), (2, 5, 4), (63, 5, 4), (64, 4, 5), (65, 5, 3), (130, 4, 3), (128, 3, 3),
                                  (70, 2, 6), (70, 6, 2), (70, 2, 2), (70, 1, 5), (70, 5, 1), (257, 3, 2)])
def test_row_widths_and_flat_volumes(cd, dims):
    for seed, holes in ((1, False), (2, True)):
        st = rough_state(dims, seed + 10 * dims[0], holes)
        want, n = check_state(st, 1.0, f"{dims} holes={holes}")
        assert n > 0 or dims[0] == 1
        if min(dims) >= 2 and not holes:
            assert len(want) > 0
    if min(dims) >= 2:
        check_state(rough_state(dims, 5), 0.25, f"{dims} min_weight 0.25")


def test_no_valid_cell(cd):
    st = rough_state((70, 5, 4), 3, holes=False)
    st["weight"][:, :, ::2] = 0.0                                   # crossings along y and z remain, no cell is valid
    want, n = check_state(st, 1.0, "no valid cell")
    assert len(want) == 0 and n > 0
    st["weight"][:] = 0.0
    want, n = check_state(st, 1.0, "empty")
    assert len(want) == 0 and n == 0


def test_eight_million_voxels(cd):
    dims = (250, 181, 180)                                          # 8.1 M voxels, rows of three full chunks and 58
    assert dims[0] * dims[1] * dims[2] >= 8_000_000 and dims[0] % 64
    sdf = mesh_ref.spheres_sdf(dims, [(60.2, 70.4, 80.6), (180.7, 100.1, 60.3), (247.6, 90.3, 120.2)], 38.0)
    st = mesh_ref.state_from_sdf(sdf.astype(np.float32))
    st["weight"][60:90, :, :128] = 0.0                              # a slab without measurements cuts the first sphere
    want, n = check_state(st, 1.0, "8 M voxels")
    assert len(want) > 50000 and n > 25000


def test_determinism_and_graph_replay(cd):
    dims = (70, 21, 19)
    a, b = rough_state(dims, 41), rough_state(dims, 42, holes=False)
    T, Wt = tg.dev(a["tsdf"]), tg.dev(a["weight"])
    want, _ = mesh_ref.triangles_ref(a, 1.0)[:2]
    first, c1, _ = device_triangles(T, Wt, 1.0, len(want) + 50)
    second, c2, _ = device_triangles(T, Wt, 1.0, len(want) + 50)
    torch.cuda.synchronize()
    assert torch.equal(first, second) and torch.equal(c1, c2), "two calls differ"   # (the workspace has unwritten padding)
    cap = 5 * 69 * 20 * 18
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        tris, count, _ = device_triangles(T, Wt, 1.0, cap, stream=s)
    torch.cuda.synchronize()
    for f, st in enumerate((b, a)):
        T.copy_(tg.dev(st["tsdf"]))
        Wt.copy_(tg.dev(st["weight"]))
        tris.fill_(SENTINEL)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        want = mesh_ref.triangles_ref(st, 1.0)[0]
        got = tris.cpu().numpy()
        assert int(count.item()) == len(want), f"replay {f}"
        assert np.array_equal(got[:len(want)], want), f"replay {f}"
        assert (got[len(want):] == SENTINEL).all(), f"replay {f}: written past the total"


def test_batched_call_and_errors(cd):
    vol = cd.TSDFVolume((40, 12, 9), 0.05, (0.0, 0.0, 0.0), color=False)
    st = rough_state((40, 12, 9), 8)
    vol.tsdf.copy_(tg.dev(st["tsdf"]))
    vol.weight.copy_(tg.dev(st["weight"]))
    want, n, _ = mesh_ref.triangles_ref(st, 1.0)
    pts, nrm, col, count, tris, tcount = vol.extract_triangle_mesh_batched(n + 7, len(want) + 7, normals=False)
    torch.cuda.synchronize()
    assert nrm is None and col is None and int(count.item()) == n and int(tcount.item()) == len(want)
    assert tris.shape == (len(want) + 7, 3) and np.array_equal(tris[:len(want)].cpu().numpy(), want)
    ep, _, _ = ref.extract_ref(st, (40, 12, 9), (0.0, 0.0, 0.0), 0.05, 1.0)
    tg.assert_bitwise(pts[:n], ep, "vertices")
    with pytest.raises(RuntimeError, match="triangle_capacity"):
        vol.extract_triangle_mesh_batched(10, 0)
    vol.reset()
    mesh = vol.extract_triangle_mesh()
    assert mesh.vertices.shape == (0, 3) and mesh.triangles.shape == (0, 3) and mesh.colors is None
