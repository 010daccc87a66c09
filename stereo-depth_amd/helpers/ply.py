"""Binary little-endian PLY files of point clouds, without Open3D.

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
