"""Triangle meshes of TSDF volumes without a GPU: the generated marching-cubes table (cuda_depth/mc_table.py) against
its rule, the topology, orientation and position of the reference's meshes (tests/mesh_ref.py) on analytic volumes -- the
tests that catch a wrong table, which the bitwise GPU tests share and cannot -- the fused demo scene, PLY mesh files, the
C ABI's declaration, export and argument checks, and Python validation before the device is touched."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import mesh_ref
import tsdf_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "stereo_mi355x.h")
NEW_SYMBOLS = ("smx_tsdf_extract_triangles", "smx_tsdf_extract_triangles_workspace_bytes")
mc = mesh_ref.mc_table()


@pytest.fixture(scope="module")
def cd():
    import cuda_depth
    return cuda_depth


# ---- the table ------------------------------------------------------------------------------------------------------------

def crossed_edges(case):
    """The cube edges whose two corners differ in sign, from the numbering alone."""
    out = set()
    for e in range(12):
        b, a = mc.edge_base_axis(e)
        u = mc.corner_index(b)
        v = u + (1, 2, 4)[a]
        if ((case >> u) & 1) != ((case >> v) & 1):
            out.add(e)
    return out


def test_table_empty_cases_and_widest_row():
    counts, edges = mc.build_table()
    assert counts[0] == 0 and counts[255] == 0
    assert counts.max() == 5 and edges.shape == (256, 15)
    for case in range(256):
        assert (edges[case, :3 * counts[case]] < 12).all() and (edges[case, 3 * counts[case]:] == 255).all()
        assert (counts[case] == 0) == (case in (0, 255))


def test_table_segments_close_into_loops():
    for case in range(256):
        segs = mc.case_segments(case)
        want = crossed_edges(case)
        assert sorted(p for p, _ in segs) == sorted(want), case      # every crossed edge is left exactly once
        assert sorted(q for _, q in segs) == sorted(want), case      # and entered exactly once
        loops = mc.case_loops(case)
        assert sorted(e for l in loops for e in l) == sorted(want)
        assert all(l[0] == min(l) for l in loops) and [l[0] for l in loops] == sorted(l[0] for l in loops)
        assert len(mc.case_triangles(case)) == sum(len(l) - 2 for l in loops)
        for a, b, c in mc.case_triangles(case):
            assert len({a, b, c}) == 3


def test_table_face_rule():
    for case in range(256):
        for normal, ring in mc.FACES:
            inside = [(case >> c) & 1 for c in ring]
            segs = mc.face_segments(case, normal, ring)
            face_edges = {mc.edge_id(ring[m], ring[(m + 1) % 4]) for m in range(4)}
            crossed = face_edges & crossed_edges(case)
            assert {e for s in segs for e in s} == crossed
            if sum(inside) in (0, 4):
                assert segs == []
            elif len(crossed) == 2:
                assert len(segs) == 1
            else:                                                     # two diagonally opposite inside corners
                assert sum(inside) == 2 and len(crossed) == 4 and len(segs) == 2
                for p, q in segs:
                    ends = []
                    for e in (p, q):
                        b, a = mc.edge_base_axis(e)
                        u = mc.corner_index(b)
                        ends.append({u, u + (1, 2, 4)[a]})
                    (shared,) = ends[0] & ends[1]
                    assert (case >> shared) & 1, "a segment of an ambiguous face must cut off an inside corner"


def test_table_single_corner_and_complement():
    (tri,) = mc.case_triangles(1 << 0)
    p = [mc.edge_midpoint2(e).astype(np.float64) for e in tri]
    n = np.cross(p[1] - p[0], p[2] - p[0])
    assert (n > 0).all(), n
    for case in range(256):
        edges_of = lambda c: {e for t in mc.case_triangles(c) for e in t}  # noqa: E731
        assert edges_of(case) == edges_of(255 - case) == crossed_edges(case)


def test_committed_header_is_the_generated_text():
    path = os.path.join(ROOT, "stereo-depth_amd", "csrc", "k_mesh_table.h")
    assert open(path).read() == mc.header_text()
    assert os.path.samefile(path, mc.header_path())


# ---- topology through the reference ---------------------------------------------------------------------------------------

def closed_manifold(tris):
    keys, counts = mesh_ref.directed_edge_counts(tris)
    assert (counts == 1).all(), "a directed edge occurs more than once"
    assert np.array_equal(np.sort(mesh_ref.reverse_keys(keys)), keys), "an edge without its reverse"


SPHERE_DIMS, SPHERE_C, SPHERE_R = (33, 31, 35), (15.3, 14.6, 17.1), 9.0


@pytest.fixture(scope="module")
def sphere():
    st = mesh_ref.state_from_sdf(mesh_ref.spheres_sdf(SPHERE_DIMS, [SPHERE_C], SPHERE_R))
    tris, n, _ = mesh_ref.triangles_ref(st)
    pts, nrm, _ = ref.extract_ref(st, SPHERE_DIMS, (0.0, 0.0, 0.0), 1.0)
    assert len(pts) == n
    return st, tris, pts, nrm


def test_sphere_is_a_closed_surface_of_genus_0(sphere):
    _, tris, pts, _ = sphere
    assert len(tris) > 1000 and tris.dtype == np.int32
    assert tris.min() >= 0 and tris.max() < len(pts)
    closed_manifold(tris)
    assert mesh_ref.euler(tris) == 2
    assert len(np.unique(tris)) == len(pts), "on a fully valid volume every crossing is referenced"


def test_two_spheres_and_a_torus():
    st = mesh_ref.state_from_sdf(mesh_ref.spheres_sdf((50, 28, 27), [(12.3, 13.6, 13.2), (36.4, 13.1, 12.7)], 8.0))
    tris, n, _ = mesh_ref.triangles_ref(st)
    closed_manifold(tris)
    assert mesh_ref.euler(tris) == 4 and tris.max() < n
    st = mesh_ref.state_from_sdf(mesh_ref.torus_sdf((40, 41, 18), (19.3, 20.4, 8.6), 11.0, 4.5))
    tris, n, _ = mesh_ref.triangles_ref(st)
    closed_manifold(tris)
    assert mesh_ref.euler(tris) == 0 and tris.max() < n


def ambiguous_faces(inside):
    """Occurrences of the six ambiguous face configurations (three face planes x two diagonals)."""
    out = []
    for a, b in ((2, 1), (2, 0), (1, 0)):                             # the face's two in-plane array axes
        def sh(da, db):
            idx = [slice(None)] * 3
            idx[a] = slice(da, inside.shape[a] - 1 + da)
            idx[b] = slice(db, inside.shape[b] - 1 + db)
            return inside[tuple(idx)]
        s00, s10, s01, s11 = sh(0, 0), sh(1, 0), sh(0, 1), sh(1, 1)
        out.append(int((s00 & s11 & ~s10 & ~s01).sum()))
        out.append(int((~s00 & ~s11 & s10 & s01).sum()))
    return out


def test_random_field_is_closed_and_consistently_oriented():
    st = mesh_ref.random_state((24, 25, 26), seed=7)
    assert all(c > 0 for c in ambiguous_faces(st["tsdf"] < 0)), "an ambiguous face configuration does not occur"
    valid, case = mesh_ref.cells(st["tsdf"], st["weight"], 1.0)
    assert valid.all() and len(np.unique(case)) == 256
    tris, n, _ = mesh_ref.triangles_ref(st)
    assert tris.min() >= 0 and tris.max() < n
    keys, counts = mesh_ref.directed_edge_counts(tris)
    order = np.argsort(mesh_ref.reverse_keys(keys))
    assert np.array_equal(mesh_ref.reverse_keys(keys)[order], keys), "an edge without its reverse"
    assert np.array_equal(counts[order], counts), "an edge and its reverse occur a different number of times"


# ---- orientation and position ---------------------------------------------------------------------------------------------

def test_sphere_orientation_and_position(sphere):
    _, tris, pts, nrm = sphere
    p = pts.astype(np.float64)
    a, b, c = p[tris[:, 0]], p[tris[:, 1]], p[tris[:, 2]]
    g = np.cross(b - a, c - a)
    solid = np.linalg.norm(g, axis=1) > 1e-9
    assert solid.mean() > 0.9
    centroid = (a + b + c) / 3
    radial = centroid - (np.asarray(SPHERE_C) + 0.5)                  # voxel (i, j, k) is centred at index + 0.5
    assert (np.sum(g * radial, axis=1)[solid] > 0).all(), "a triangle faces inward"
    vn = nrm.astype(np.float64)
    nsum = vn[tris[:, 0]] + vn[tris[:, 1]] + vn[tris[:, 2]]
    assert (np.sum(g * nsum, axis=1)[solid] > 0).all(), "a triangle faces against its vertex normals"
    assert np.abs(np.linalg.norm(radial, axis=1) - SPHERE_R).max() < 0.5


# ---- the fused scene ------------------------------------------------------------------------------------------------------

SCENE_DIMS, SCENE_VS, SCENE_ORIGIN = (48, 23, 60), 0.1, (-2.4, -0.4, 4.0)
CAM = dict(H=96, W=128, fx=100.0, cx=63.5, cy=47.5, baseline=0.5)


@pytest.fixture(scope="module")
def fused(cd):
    scene, poses = ref.demo_scene(), ref.orbit_poses(6)
    Q = cd.reprojection_matrix(CAM["fx"], CAM["cx"], CAM["cy"], CAM["baseline"])
    d = np.stack([scene.render(p, CAM["H"], CAM["W"], CAM["fx"], CAM["cx"], CAM["cy"], CAM["baseline"]) for p in poses])
    st = ref.empty_state(SCENE_DIMS, False)
    ref.integrate_ref(st, SCENE_DIMS, SCENE_ORIGIN, SCENE_VS, 3 * SCENE_VS, 64.0, d, Q, ref.projection(Q),
                      ref.world_to_camera(poses))
    return st


def test_fused_scene_mesh(fused, tmp_path):
    from helpers.ply import read_mesh_ply, write_mesh_ply
    st = fused
    tris, n, where = mesh_ref.triangles_ref(st, 1.0)
    assert len(tris) > 2000 and tris.max() < n
    good = mesh_ref.usable(st["tsdf"], st["weight"], 1.0)
    bad_cell = ~np.ones(tuple(s - 1 for s in good.shape), bool)
    for g in mesh_ref.corner_views(good):
        bad_cell |= ~g
    assert bad_cell.any() and not bad_cell[where[:, 2], where[:, 1], where[:, 0]].any()
    flat = (where[:, 2] * SCENE_DIMS[1] + where[:, 1]) * SCENE_DIMS[0] + where[:, 0]
    assert (np.diff(flat) >= 0).all(), "cells out of order"
    seen = set(map(tuple, where))
    for min_weight in (2.0, 4.0):
        t2, n2, w2 = mesh_ref.triangles_ref(st, min_weight)
        assert len(t2) <= len(tris) and n2 <= n and set(map(tuple, w2)) <= seen
        seen, tris_count = set(map(tuple, w2)), len(t2)
    assert tris_count < len(tris)
    pts, nrm, _ = ref.extract_ref(st, SCENE_DIMS, SCENE_ORIGIN, SCENE_VS, 1.0)
    path = str(tmp_path / "scene.ply")
    write_mesh_ply(path, pts, tris, normals=nrm)
    v, t, c, nn = read_mesh_ply(path)
    assert c is None and t.dtype == np.int32
    assert np.array_equal(v.view(np.uint32), pts.view(np.uint32)) and np.array_equal(t, tris)
    assert np.array_equal(nn.view(np.uint32), nrm.view(np.uint32))


# ---- PLY ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("with_colors", [False, True])
@pytest.mark.parametrize("with_normals", [False, True])
def test_mesh_ply_round_trip(tmp_path, with_colors, with_normals):
    from helpers.ply import read_mesh_ply, read_ply, write_mesh_ply, write_ply
    rng = np.random.default_rng(3)
    pts = rng.normal(size=(11, 3)).astype(np.float32)
    tri = rng.integers(0, 11, (7, 3)).astype(np.int32)
    col = rng.integers(0, 256, (11, 3)).astype(np.uint8) if with_colors else None
    nrm = rng.normal(size=(11, 3)).astype(np.float32) if with_normals else None
    path = str(tmp_path / "m.ply")
    write_mesh_ply(path, pts, tri, colors=col, normals=nrm)
    data = open(path, "rb").read()
    head = data[:data.index(b"end_header\n")].decode("ascii")
    assert "element vertex 11" in head and "element face 7" in head
    assert "property list uchar int vertex_indices" in head and "format binary_little_endian 1.0" in head
    assert len(data) == len(head) + len("end_header\n") + 11 * (12 + 12 * with_normals + 3 * with_colors) + 7 * 13
    v, t, c, n = read_mesh_ply(path)
    assert np.array_equal(v, pts) and np.array_equal(t, tri) and t.dtype == np.int32
    assert (c is None) == (col is None) and (n is None) == (nrm is None)
    assert col is None or np.array_equal(c, col)
    assert nrm is None or np.array_equal(n, nrm)
    write_mesh_ply(path, pts, np.zeros((0, 3), np.int64))            # a mesh without faces
    v, t, _, _ = read_mesh_ply(path)
    assert t.shape == (0, 3) and np.array_equal(v, pts)
    write_ply(path, pts, col, nrm)                                    # the point-cloud functions are as they were
    assert np.array_equal(read_ply(path)[0], pts)
    with pytest.raises(ValueError, match="vertex and face"):
        read_mesh_ply(path)


def test_mesh_ply_rejects_bad_arguments(tmp_path):
    from helpers.ply import write_mesh_ply
    path = str(tmp_path / "bad.ply")
    pts = np.zeros((4, 3), np.float32)
    ok = np.array([[0, 1, 2]], np.int32)
    for tri in (np.array([[0, 1, 4]]), np.array([[0, -1, 2]]), np.zeros((2, 4), np.int32), np.zeros(3, np.int32),
                np.zeros((1, 3), np.float32)):
        with pytest.raises(ValueError, match="triangle"):
            write_mesh_ply(path, pts, tri)
    with pytest.raises(ValueError, match="vertices must be"):
        write_mesh_ply(path, np.zeros((4, 2), np.float32), ok)
    with pytest.raises(ValueError, match="colors must be"):
        write_mesh_ply(path, pts, ok, colors=np.zeros((4, 3), np.float32))
    with pytest.raises(ValueError, match="normals must be"):
        write_mesh_ply(path, pts, ok, normals=np.zeros((3, 3), np.float32))
    assert not os.path.exists(path)


# ---- the C ABI --------------------------------------------------------------------------------------------------------------

def test_c_abi_is_declared_and_exported():
    import cuda_depth._native as native
    text = open(HEADER).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\(", text), name
        assert name in native.EXPORTS, name
        assert getattr(native.LIB, name) is not None
        assert name in text.split("Conventions")[0], f"{name} is missing from the header's list of entry points"
    out = os.popen(f"nm -D --defined-only {native.LIB_PATH}").read()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bT " + name + r"\b", out), name
    assert native.LIB.smx_abi_version() == 4


def test_workspace_query():
    import cuda_depth._native as native
    q = native.LIB.smx_tsdf_extract_triangles_workspace_bytes
    for bad in ((0, 8, 8), (8, -1, 8), (8, 8, 4097), (4096, 4096, 65)):
        assert q(*bad) == 0, bad
    for nx, ny, nz in ((8, 8, 8), (1, 1, 1), (65, 3, 2), (512, 256, 512), (4096, 4096, 64), (1, 4096, 4096)):
        got = q(nx, ny, nz)
        # one byte per voxel; per row: a word per started chunk of 64 voxels (nx/16 + 4 bytes at most) and six ints,
        # with the scan's block sums and the alignment of the nine arrays under 64 bytes per row + 4 KiB
        assert nx * ny * nz <= got <= 4 * nx * ny * nz + 64 * ny * nz + 4096, (nx, ny, nz, got)
    # the benchmark volume: 1 byte per voxel + 4 per 64 voxels + 24 per row of 512, and the alignment
    assert q(512, 256, 512) <= (1 + 1 / 16 + 24 / 512) * 512 * 256 * 512 + 4096


def test_c_abi_rejects_bad_arguments_without_a_device():
    import cuda_depth._native as native
    lib, bad = native.LIB, native.SMX_OK - 1                          # SMX_ERR_INVALID_ARG = -1
    wsb = lib.smx_tsdf_extract_triangles_workspace_bytes(8, 8, 8)
    inf, nan = math.inf, math.nan

    def tt(**kw):
        a = dict(dev=0, nx=8, ny=8, nz=8, tsdf=C.c_void_p(0x2000000), weight=C.c_void_p(0x3000000), minw=1.0, cap=100,
                 tris=C.c_void_p(0x4000000), count=C.c_void_p(0x5000000), ws=C.c_void_p(0x100000000), wsb=wsb,
                 stream=None)
        a.update(kw)
        return lib.smx_tsdf_extract_triangles(*a.values())

    for kw in (dict(tsdf=None), dict(weight=None), dict(tris=None), dict(count=None), dict(ws=None), dict(nx=0),
               dict(ny=4097), dict(nz=-1), dict(nx=4096, ny=4096, nz=65), dict(minw=0.0), dict(minw=-1.0),
               dict(minw=nan), dict(minw=inf), dict(cap=0), dict(cap=-5), dict(cap=2 ** 30 + 1), dict(wsb=wsb - 1),
               dict(wsb=0), dict(tris=C.c_void_p(0x2000000 + 8)), dict(tris=C.c_void_p(0x3000000 + 2044)),
               dict(count=C.c_void_p(0x4000000 + 4)), dict(count=C.c_void_p(0x3000000)),
               dict(ws=C.c_void_p(0x2000000 + 16)), dict(ws=C.c_void_p(0x4000000 + 1196)),
               dict(ws=C.c_void_p(0x5000000 - 8)), dict(stream=native.STREAM_ENGINE)):
        assert tt(**kw) == bad, kw
        assert "smx_tsdf_extract_triangles" in native.last_error()
    assert tt(cap=2 ** 30 + 1) == bad and "capacity" in native.last_error()
    assert tt(ws=C.c_void_p(0x100000000 + 8)) == bad and "workspace must be 256-byte aligned" in native.last_error()
    assert tt(minw=nan) == bad and "min_weight" in native.last_error()
    assert tt(stream=native.STREAM_ENGINE) == bad and "stream" in native.last_error().lower()


# ---- Python ---------------------------------------------------------------------------------------------------------------

def test_python_validation_before_the_device(cd):
    import dataclasses
    import inspect
    vol = object.__new__(cd.TSDFVolume)                               # the checks run before any state is touched
    with pytest.raises(RuntimeError, match="triangle_capacity"):
        vol.extract_triangle_mesh_batched(10, 0)
    with pytest.raises(RuntimeError, match="triangle_capacity"):
        vol.extract_triangle_mesh_batched(10, 2 ** 30 + 1)
    with pytest.raises(TypeError):
        vol.extract_triangle_mesh_batched(10, 2.5)
    with pytest.raises(RuntimeError, match="capacity"):
        vol.extract_triangle_mesh_batched(0, 10)
    with pytest.raises(RuntimeError, match="min_weight"):
        vol.extract_triangle_mesh_batched(10, 10, min_weight=0.0)
    with pytest.raises(RuntimeError, match="min_weight"):
        vol.extract_triangle_mesh_batched(10, 10, min_weight=math.nan)
    sig = inspect.signature(cd.TSDFVolume.extract_triangle_mesh).parameters
    assert sig["min_weight"].default == 1.0 and sig["normals"].default is True
    sig = inspect.signature(cd.TSDFVolume.extract_triangle_mesh_batched).parameters
    assert [p for p in sig][1:3] == ["vertex_capacity", "triangle_capacity"]
    assert all(sig[p].kind is inspect.Parameter.KEYWORD_ONLY for p in ("min_weight", "normals", "colors"))
    assert [f.name for f in dataclasses.fields(cd.TriangleMesh)] == ["vertices", "triangles", "normals", "colors"]
