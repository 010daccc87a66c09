"""Binary little-endian PLY files of point clouds and triangle meshes, without Open3D.

    write_ply(path, points, colors=None, normals=None)
                                             points [N, 3] float32-convertible, colors [N, 3] uint8 (optional),
                                             normals [N, 3] float32-convertible (optional)
    read_ply(path) -> (points [N, 3] float32, colors [N, 3] uint8 or None)
    read_ply(path, with_normals=True) -> (points, colors, normals [N, 3] float32 or None)

The header is exactly:

    ply
    format binary_little_endian 1.0
    element vertex <N>
    property float x
    property float y
    property float z
    [property float nx
    property float ny
    property float nz]
    [property uchar red
    property uchar green
    property uchar blue]
    end_header

followed by N records of 12 bytes, plus 12 with normals and 3 with colours.  Tensors on a GPU are copied to the host.

    write_mesh_ply(path, vertices, triangles, colors=None, normals=None)
                                             the same vertex element, then M faces: triangles [M, 3] int32-convertible
                                             indices into the vertices
    read_mesh_ply(path) -> (vertices [N, 3] float32, triangles [M, 3] int32, colors or None, normals or None)

A mesh file's header has, after the vertex properties,

    element face <M>
    property list uchar int vertex_indices

and after the vertex records M records of 13 bytes: the count 3 and three little-endian int32 indices.
"""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np

_XYZ = ["property float x", "property float y", "property float z"]
_RGB = ["property uchar red", "property uchar green", "property uchar blue"]
_NRM = ["property float nx", "property float ny", "property float nz"]


def _host(a) -> np.ndarray:
    if hasattr(a, "detach"):                                   # torch.Tensor, without importing torch here
        a = a.detach().cpu().numpy()
    return np.asarray(a)


def ply_header(count: int, with_colors: bool, with_normals: bool = False) -> bytes:
    lines = ["ply", "format binary_little_endian 1.0", f"element vertex {int(count)}"] + _XYZ
    if with_normals:
        lines += _NRM
    if with_colors:
        lines += _RGB
    return ("\n".join(lines + ["end_header"]) + "\n").encode("ascii")


def write_ply(path: str, points, colors=None, normals=None) -> None:
    pts = _host(points)
    if pts.ndim != 2 or pts.shape[1] != 3:
        raise ValueError(f"points must be [N, 3], got {pts.shape}")
    pts = pts.astype("<f4", copy=False)
    dtype = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    if normals is not None:
        nrm = _host(normals)
        if nrm.shape != pts.shape:
            raise ValueError(f"normals must be {pts.shape}, got {nrm.shape}")
        nrm = nrm.astype("<f4", copy=False)
        dtype += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
    if colors is not None:
        col = _host(colors)
        if col.shape != pts.shape or col.dtype != np.uint8:
            raise ValueError(f"colors must be uint8 {pts.shape}, got {col.dtype} {col.shape}")
        dtype += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    rec = np.empty(pts.shape[0], dtype=dtype)
    rec["x"], rec["y"], rec["z"] = pts[:, 0], pts[:, 1], pts[:, 2]
    if normals is not None:
        rec["nx"], rec["ny"], rec["nz"] = nrm[:, 0], nrm[:, 1], nrm[:, 2]
    if colors is not None:
        rec["red"], rec["green"], rec["blue"] = col[:, 0], col[:, 1], col[:, 2]
    with open(path, "wb") as f:
        f.write(ply_header(pts.shape[0], colors is not None, normals is not None))
        f.write(rec.tobytes())


def read_ply(path: str, *, with_normals: bool = False):
    """Reads what write_ply writes (binary little-endian, float x y z, optional float nx ny nz, optional uchar red green
    blue): (points, colors or None), and with with_normals=True (points, colors or None, normals or None)."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.find(b"end_header\n")
    if not data.startswith(b"ply\n") or end < 0:
        raise ValueError(f"{path}: not a PLY file")
    lines = data[:end].decode("ascii").splitlines()
    if "format binary_little_endian 1.0" not in lines:
        raise ValueError(f"{path}: only binary_little_endian 1.0 is supported")
    count = next(int(l.split()[2]) for l in lines if l.startswith("element vertex "))
    props = [l for l in lines if l.startswith("property ")]
    layouts = {(False, False): _XYZ, (False, True): _XYZ + _RGB, (True, False): _XYZ + _NRM,
               (True, True): _XYZ + _NRM + _RGB}
    found = [k for k, v in layouts.items() if v == props]
    if not found:
        raise ValueError(f"{path}: unsupported properties {props}")
    has_normals, with_colors = found[0]
    dtype = ([("x", "<f4"), ("y", "<f4"), ("z", "<f4")] + ([("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")] if has_normals
             else []) + ([("r", "u1"), ("g", "u1"), ("b", "u1")] if with_colors else []))
    rec = np.frombuffer(data, dtype=dtype, count=count, offset=end + len(b"end_header\n"))
    pts = np.stack([rec["x"], rec["y"], rec["z"]], axis=1).astype(np.float32)
    col = np.stack([rec["r"], rec["g"], rec["b"]], axis=1).astype(np.uint8) if with_colors else None
    if not with_normals:
        return pts, col
    nrm = np.stack([rec["nx"], rec["ny"], rec["nz"]], axis=1).astype(np.float32) if has_normals else None
    return pts, col, nrm


_FACE = "property list uchar int vertex_indices"
_FACE_DTYPE = [("n", "u1"), ("v", "<i4", (3,))]


def _vertex_records(points, colors, normals, what="points") -> np.ndarray:
    pts = _host(points)
    if pts.ndim != 2 or pts.shape[1] != 3:
        raise ValueError(f"{what} must be [N, 3], got {pts.shape}")
    pts = pts.astype("<f4", copy=False)
    dtype = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    if normals is not None:
        nrm = _host(normals)
        if nrm.shape != pts.shape:
            raise ValueError(f"normals must be {pts.shape}, got {nrm.shape}")
        nrm = nrm.astype("<f4", copy=False)
        dtype += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
    if colors is not None:
        col = _host(colors)
        if col.shape != pts.shape or col.dtype != np.uint8:
            raise ValueError(f"colors must be uint8 {pts.shape}, got {col.dtype} {col.shape}")
        dtype += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    rec = np.empty(pts.shape[0], dtype=dtype)
    rec["x"], rec["y"], rec["z"] = pts[:, 0], pts[:, 1], pts[:, 2]
    if normals is not None:
        rec["nx"], rec["ny"], rec["nz"] = nrm[:, 0], nrm[:, 1], nrm[:, 2]
    if colors is not None:
        rec["red"], rec["green"], rec["blue"] = col[:, 0], col[:, 1], col[:, 2]
    return rec


def write_mesh_ply(path: str, vertices, triangles, colors=None, normals=None) -> None:
    """Writes an indexed triangle mesh; every index must lie in [0, N)."""
    rec = _vertex_records(vertices, colors, normals, "vertices")
    tri = _host(triangles)
    if tri.ndim != 2 or tri.shape[1] != 3 or tri.dtype.kind not in "iu":
        raise ValueError(f"triangles must be integers [M, 3], got {tri.dtype} {tri.shape}")
    if tri.size and (int(tri.min()) < 0 or int(tri.max()) >= rec.shape[0]):
        raise ValueError(f"triangle indices must lie in [0, {rec.shape[0]}), got {int(tri.min())}..{int(tri.max())}")
    faces = np.empty(tri.shape[0], dtype=_FACE_DTYPE)
    faces["n"] = 3
    faces["v"] = tri
    header = ply_header(rec.shape[0], colors is not None, normals is not None)
    header = header[:-len(b"end_header\n")] + f"element face {tri.shape[0]}\n{_FACE}\nend_header\n".encode("ascii")
    with open(path, "wb") as f:
        f.write(header)
        f.write(rec.tobytes())
        f.write(faces.tobytes())


def read_mesh_ply(path: str):
    """Reads what write_mesh_ply writes: (vertices, triangles [M, 3] int32, colors or None, normals or None)."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.find(b"end_header\n")
    if not data.startswith(b"ply\n") or end < 0:
        raise ValueError(f"{path}: not a PLY file")
    lines = data[:end].decode("ascii").splitlines()
    if "format binary_little_endian 1.0" not in lines:
        raise ValueError(f"{path}: only binary_little_endian 1.0 is supported")
    elements = [l for l in lines if l.startswith("element ")]
    if len(elements) != 2 or not elements[0].startswith("element vertex ") or not elements[1].startswith("element face "):
        raise ValueError(f"{path}: need the elements vertex and face, got {elements}")
    count, faces = int(elements[0].split()[2]), int(elements[1].split()[2])
    at = lines.index(elements[1])
    props = [l for l in lines[:at] if l.startswith("property ")]
    if [l for l in lines[at:] if l.startswith("property ")] != [_FACE]:
        raise ValueError(f"{path}: the face element must be '{_FACE}'")
    layouts = {(False, False): _XYZ, (False, True): _XYZ + _RGB, (True, False): _XYZ + _NRM,
               (True, True): _XYZ + _NRM + _RGB}
    found = [k for k, v in layouts.items() if v == props]
    if not found:
        raise ValueError(f"{path}: unsupported properties {props}")
    has_normals, with_colors = found[0]
    dtype = ([("x", "<f4"), ("y", "<f4"), ("z", "<f4")] + ([("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")] if has_normals
             else []) + ([("r", "u1"), ("g", "u1"), ("b", "u1")] if with_colors else []))
    offset = end + len(b"end_header\n")
    rec = np.frombuffer(data, dtype=dtype, count=count, offset=offset)
    fr = np.frombuffer(data, dtype=_FACE_DTYPE, count=faces, offset=offset + rec.nbytes)
    if faces and not (fr["n"] == 3).all():
        raise ValueError(f"{path}: only triangles are supported")
    tri = fr["v"].astype(np.int32).reshape(-1, 3)
    if tri.size and (int(tri.min()) < 0 or int(tri.max()) >= count):
        raise ValueError(f"{path}: a triangle index lies outside [0, {count})")
    pts = np.stack([rec["x"], rec["y"], rec["z"]], axis=1).astype(np.float32)
    col = np.stack([rec["r"], rec["g"], rec["b"]], axis=1).astype(np.uint8) if with_colors else None
    nrm = np.stack([rec["nx"], rec["ny"], rec["nz"]], axis=1).astype(np.float32) if has_normals else None
    return pts, tri, col, nrm
