"""NumPy reference of smx_tsdf_extract_triangles (include/stereo_mi355x.h), vectorised over the cells: the vertex ranks
come from tsdf_ref.crossings (the emission rule of smx_tsdf_extract_points), the case table from cuda_depth/mc_table.py.
Also the analytic states (spheres, a torus, a random field) and the mesh bookkeeping that the CPU and GPU tests share."""
from __future__ import annotations

import functools
import importlib.util
import os

import numpy as np

import tsdf_ref

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def mc_table():
    """The generator module, loaded from its file so that the reference needs neither the package nor the library."""
    path = os.path.join(ROOT, "stereo-depth_amd", "cuda_depth", "mc_table.py")
    spec = importlib.util.spec_from_file_location("smx_mc_table", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def table():
    return mc_table().build_table()


def usable(tsdf, weight, min_weight):
    with np.errstate(invalid="ignore"):
        return (weight >= f32(min_weight)) & (np.abs(tsdf) < 1)


def corner_views(a):
    """The eight [nz-1, ny-1, nx-1] views of a [nz, ny, nx] array, corner c = cx + 2*cy + 4*cz."""
    nz, ny, nx = a.shape
    return [a[cz:nz - 1 + cz, cy:ny - 1 + cy, cx:nx - 1 + cx] for cz in (0, 1) for cy in (0, 1) for cx in (0, 1)]


def cells(tsdf, weight, min_weight):
    """(valid [nz-1, ny-1, nx-1] bool, case [same] uint8)."""
    good = usable(tsdf, weight, min_weight)
    inside = tsdf < 0
    valid = np.ones(tuple(n - 1 for n in tsdf.shape), bool)
    case = np.zeros(valid.shape, np.uint8)
    for c, (g, s) in enumerate(zip(corner_views(good), corner_views(inside))):
        valid &= g
        case |= (s.astype(np.uint8) << c).astype(np.uint8)
    return valid, case


def triangles_ref(state, min_weight=1.0):
    """(triangles [M, 3] int32, number of vertices N, cell of every triangle [M, 3] int as (i, j, k))."""
    T, Wt = state["tsdf"], state["weight"]
    nz, ny, nx = T.shape
    em = tsdf_ref.crossings(T, Wt, min_weight)
    n_vertices = int(em.sum())
    if min(nx, ny, nz) < 2:
        return np.zeros((0, 3), np.int32), n_vertices, np.zeros((0, 3), np.int64)
    rank = (np.cumsum(em.reshape(-1)) - 1).reshape(nz, ny, nx, 3)
    valid, case = cells(T, Wt, min_weight)
    kk, jj, ii = np.nonzero(valid)                                    # ascending (k*ny + j)*nx + i
    cs = case[kk, jj, ii]
    counts, edges = table()
    mc = mc_table()
    base = np.array([mc.edge_base_axis(e)[0] for e in range(12)])     # [12, 3] offsets (x, y, z)
    axis = np.array([mc.edge_base_axis(e)[1] for e in range(12)])
    e = edges[cs].astype(np.int64)                                    # [cells, 15]
    live = np.arange(15)[None, :] < 3 * counts[cs].astype(np.int64)[:, None]
    e = np.where(live, e, 0)
    v = rank[kk[:, None] + base[e, 2], jj[:, None] + base[e, 1], ii[:, None] + base[e, 0], axis[e]]
    assert em.reshape(nz, ny, nx, 3)[kk[:, None] + base[e, 2], jj[:, None] + base[e, 1], ii[:, None] + base[e, 0],
                                     axis[e]][live].all(), "a crossed edge of a valid cell is no emitted crossing"
    tri_live = live.reshape(-1, 5, 3)[:, :, 0]
    tris = v.reshape(-1, 5, 3)[tri_live]
    where = np.broadcast_to(np.stack([ii, jj, kk], axis=1)[:, None, :], (len(ii), 5, 3))[tri_live]
    return tris.astype(np.int32), n_vertices, where


# ---- states ---------------------------------------------------------------------------------------------------------------

def state_from_sdf(sdf_voxels, tau_voxels=3.0):
    """T = clip(sdf / tau, -1, 1), weight 1; sdf in voxels, [nz, ny, nx]."""
    T = np.clip(sdf_voxels / tau_voxels, -1.0, 1.0).astype(np.float32)
    return {"tsdf": T, "weight": np.ones_like(T), "color": None}


def grid(dims):
    nx, ny, nz = dims
    return np.meshgrid(np.arange(nz, dtype=np.float64), np.arange(ny, dtype=np.float64),
                       np.arange(nx, dtype=np.float64), indexing="ij")          # z, y, x in voxel units


def spheres_sdf(dims, centres, radius):
    z, y, x = grid(dims)
    d = np.full(z.shape, np.inf)
    for cx, cy, cz in centres:
        d = np.minimum(d, np.sqrt((x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2) - radius)
    return d


def torus_sdf(dims, centre, major, minor):
    z, y, x = grid(dims)
    q = np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2) - major
    return np.sqrt(q ** 2 + (z - centre[2]) ** 2) - minor


def random_state(dims, seed):
    """Uniform values in (-0.9, 0.9) inside a two-voxel shell of +0.5."""
    nx, ny, nz = dims
    rng = np.random.default_rng(seed)
    T = np.full((nz, ny, nx), 0.5, np.float32)
    T[2:-2, 2:-2, 2:-2] = rng.uniform(-0.9, 0.9, (nz - 4, ny - 4, nx - 4)).astype(np.float32)
    return {"tsdf": T, "weight": np.ones_like(T), "color": None}


# ---- bookkeeping ----------------------------------------------------------------------------------------------------------

def directed_edge_counts(tris):
    """(keys, counts) of the directed edges a -> b as a * 2^32 + b."""
    t = tris.astype(np.int64)
    a = np.concatenate([t[:, 0], t[:, 1], t[:, 2]])
    b = np.concatenate([t[:, 1], t[:, 2], t[:, 0]])
    return np.unique((a << 32) | b, return_counts=True)


def reverse_keys(keys):
    return ((keys & 0xffffffff) << 32) | (keys >> 32)


def euler(tris):
    """V_referenced - E + F."""
    keys, _ = directed_edge_counts(tris)
    und = np.unique(np.minimum(keys, reverse_keys(keys)))
    return len(np.unique(tris)) - len(und) + len(tris)
