"""NumPy reference of smx_tsdf_integrate and smx_tsdf_extract_points (include/stereo_mi355x.h), in the header's float32
operation order: every arithmetic step is one float32 NumPy operation on float32 operands, vectorised over the voxels,
looping over the frames in order.  Also an analytic ray-cast renderer of planes and boxes (exact depth -> disparity
f*B/Z, rounded once to float32) and pose helpers for the tests and tools/tsdf_throughput.py."""
from __future__ import annotations

import numpy as np

f32 = np.float32


def colour_u8(v: np.ndarray) -> np.ndarray:
    """f32 -> u8: clamp(floorf(v + 0.5f), 0, 255), NaN -> 0."""
    if v.dtype == np.uint8:
        return v
    with np.errstate(invalid="ignore"):
        r = np.floor(v.astype(np.float32) + f32(0.5))
        return np.fmin(np.fmax(r, f32(0)), f32(255)).astype(np.uint8)


def empty_state(dims, color=True):
    nx, ny, nz = dims
    z = np.zeros((nz, ny, nx), np.float32)
    return {"tsdf": z.copy(), "weight": z.copy(), "color": np.zeros((nz, ny, nx, 4), np.uint8) if color else None}


def voxel_centres(dims, origin, s):
    nx, ny, nz = dims
    o = [f32(v) for v in origin]
    s = f32(s)
    gx = o[0] + (np.arange(nx, dtype=np.float32) + f32(0.5)) * s
    gy = o[1] + (np.arange(ny, dtype=np.float32) + f32(0.5)) * s
    gz = o[2] + (np.arange(nz, dtype=np.float32) + f32(0.5)) * s
    Z, Y, X = np.meshgrid(gz, gy, gx, indexing="ij")
    return X.reshape(-1), Y.reshape(-1), Z.reshape(-1)


def pixel_measurements(disp, Q, confidence=None, min_confidence=0.0, depth_range=(0.0, np.inf),
                       invalid_disparity=-1.0):
    """(Zm [n, H, W] with NaN where not accepted, w [n, H, W])."""
    d = np.asarray(disp, np.float32)
    n, H, W = d.shape
    q = np.asarray(Q, np.float32).reshape(4, 4)
    v, u = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    with np.errstate(all="ignore"):
        zw = ((q[2, 0] * u + q[2, 1] * v) + q[2, 2] * d) + q[2, 3]
        ww = ((q[3, 0] * u + q[3, 1] * v) + q[3, 2] * d) + q[3, 3]
        Zm = zw / ww
        ok = np.isfinite(d) & (d != f32(invalid_disparity)) & (ww > 0) & np.isfinite(Zm)
        ok &= (Zm >= f32(depth_range[0])) & (Zm <= f32(depth_range[1]))
        w = np.ones_like(d)
        if confidence is not None:
            c = np.asarray(confidence, np.float32)
            ok &= (c >= f32(min_confidence)) & (c > 0)
            w = c.copy()
    return np.where(ok, Zm, f32(np.nan)).astype(np.float32), w


def pixel_colours(image, n, H, W):
    """[n, H, W, 3] u8 from gray [n, H, W] / [n, 1, H, W] or RGB [n, 3, H, W], u8 or f32."""
    img = np.asarray(image)
    if img.ndim == 3:
        img = img[:, None]
    c = colour_u8(img)
    if c.shape[1] == 1:
        c = np.repeat(c, 3, axis=1)
    return np.moveaxis(c, 1, -1).reshape(n, H, W, 3)


def integrate_ref(state, dims, origin, voxel_size, truncation, max_weight, disp, Q, P, world_to_camera, *,
                  image=None, confidence=None, min_confidence=0.0, depth_range=(0.0, np.inf), invalid_disparity=-1.0):
    """Updates state (empty_state's dict, in place) with n maps [n, H, W] and poses world_to_camera [n, 3, 4] float32;
    returns the boolean [nz*ny*nx] mask of the voxels some frame measured."""
    disp = np.asarray(disp, np.float32)
    n, H, W = disp.shape
    Zm, wmap = pixel_measurements(disp, Q, confidence, min_confidence, depth_range, invalid_disparity)
    use_colour = state["color"] is not None
    pcol = pixel_colours(image, n, H, W) if use_colour else None
    gx, gy, gz = voxel_centres(dims, origin, voxel_size)
    T = state["tsdf"].reshape(-1)
    Wt = state["weight"].reshape(-1)
    Cs = state["color"].reshape(-1, 4) if use_colour else None
    P = np.asarray(P, np.float32).reshape(4, 4)
    M_all = np.asarray(world_to_camera, np.float32).reshape(n, 3, 4)
    tau, wmax = f32(truncation), f32(max_weight)
    touched = np.zeros(T.shape, bool)
    with np.errstate(all="ignore"):
        for f in range(n):
            M = M_all[f]
            c = [((M[r, 0] * gx + M[r, 1] * gy) + M[r, 2] * gz) + M[r, 3] for r in range(3)]
            p = {r: ((P[r, 0] * c[0] + P[r, 1] * c[1]) + P[r, 2] * c[2]) + P[r, 3] for r in (0, 1, 3)}
            fu = np.floor(p[0] / p[3] + f32(0.5))
            fv = np.floor(p[1] / p[3] + f32(0.5))
            m = (c[2] > 0) & (p[3] > 0) & (fu >= 0) & (fu <= f32(W - 1)) & (fv >= 0) & (fv <= f32(H - 1))
            idx = np.flatnonzero(m)
            iu, iv = fu[idx].astype(np.int64), fv[idx].astype(np.int64)
            zm = Zm[f, iv, iu]
            sdf = zm - c[2][idx]
            ok = sdf >= -tau                                          # NaN Zm (not accepted) fails
            idx, iu, iv, sdf = idx[ok], iu[ok], iv[ok], sdf[ok]
            w = wmap[f, iv, iu]
            t = np.fmin(sdf / tau, f32(1.0))
            T0, W0 = T[idx], Wt[idx]
            den = W0 + w
            T[idx] = ((T0 * W0) + (t * w)) / den
            Wt[idx] = np.fmin(den, wmax)
            if use_colour:
                C0 = Cs[idx, :3].astype(np.float32)
                I = pcol[f, iv, iu].astype(np.float32)
                Cn = ((C0 * W0[:, None]) + (I * w[:, None])) / den[:, None]
                Cs[idx, :3] = colour_u8(Cn)
                Cs[idx, 3] = 0
            touched[idx] = True
    return touched


def crossings(tsdf, weight, min_weight):
    """[nz*ny*nx, 3] bool: voxel v emits along axis a."""
    nz, ny, nx = tsdf.shape
    T = tsdf.astype(np.float32)
    with np.errstate(invalid="ignore"):
        good = (weight >= f32(min_weight)) & (np.abs(T) < 1)
    pos = T >= 0
    out = np.zeros((nz, ny, nx, 3), bool)
    out[:, :, :-1, 0] = good[:, :, :-1] & good[:, :, 1:] & (pos[:, :, :-1] != pos[:, :, 1:])
    out[:, :-1, :, 1] = good[:, :-1, :] & good[:, 1:, :] & (pos[:, :-1, :] != pos[:, 1:, :])
    out[:-1, :, :, 2] = good[:-1] & good[1:] & (pos[:-1] != pos[1:])
    return out.reshape(-1, 3)


def extract_ref(state, dims, origin, voxel_size, min_weight=1.0):
    """(points [N, 3] f32, normals [N, 3] f32, colors [N, 3] u8 or None) in (voxel, axis) order."""
    nx, ny, nz = dims
    T3, W3 = state["tsdf"], state["weight"]
    em = crossings(T3, W3, min_weight)
    vi, ax = np.nonzero(em)                                           # row-major: voxel ascending, then axis
    k, rem = np.divmod(vi, nx * ny)
    j, i = np.divmod(rem, nx)
    T = T3.reshape(-1)
    step = np.array([1, nx, nx * ny])
    nb = vi + step[ax]
    T0, T1 = T[vi], T[nb]
    s = f32(voxel_size)
    o = [f32(v) for v in origin]
    with np.errstate(all="ignore"):
        t = T0 / (T0 - T1)
        g = np.stack([o[0] + (i.astype(np.float32) + f32(0.5)) * s, o[1] + (j.astype(np.float32) + f32(0.5)) * s,
                      o[2] + (k.astype(np.float32) + f32(0.5)) * s], axis=1).astype(np.float32)
        r = np.arange(len(vi))
        g[r, ax] = g[r, ax] + t * s
        d = []
        for b, (c, lim) in enumerate(((i, nx), (j, ny), (k, nz))):
            up = np.where(c + 1 < lim, vi + step[b], vi)
            dn = np.where(c - 1 >= 0, vi - step[b], vi)
            d.append(T[up] - T[dn])
        ln = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
        zero = ln == 0
        nrm = np.stack([np.where(zero, f32(0), x / ln) for x in d], axis=1).astype(np.float32)
    cols = None
    if state["color"] is not None:
        Cs = state["color"].reshape(-1, 4)
        cols = Cs[np.where(t <= f32(0.5), vi, nb), :3].copy()
    return g, nrm, cols


# ---- poses ----------------------------------------------------------------------------------------------------------------

def look_at(eye, target, up=(0.0, -1.0, 0.0)) -> np.ndarray:
    """The float64 camera-to-world pose [4, 4] of a camera at eye looking at target (x right, y down, z forward), with
    `up` the world direction that appears up in the image."""
    eye, target, up = (np.asarray(v, np.float64) for v in (eye, target, up))
    z = target - eye
    z /= np.linalg.norm(z)
    x = np.cross(-up, z)                                          # x = y_down x z
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    m = np.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = x, y, z, eye
    return m


def world_to_camera(camera_to_world) -> np.ndarray:
    """[n, 3, 4] float32 from camera-to-world poses, inverted in float64 and rounded once (as TSDFVolume does)."""
    m = np.asarray(camera_to_world, np.float64)
    if m.ndim == 2:
        m = m[None]
    return np.ascontiguousarray(np.linalg.inv(m)[:, :3, :].astype(np.float32))


def projection(Q) -> np.ndarray:
    return np.linalg.inv(np.asarray(Q, np.float64)).astype(np.float32)


# ---- analytic scenes --------------------------------------------------------------------------------------------------------

class Scene:
    """A ground plane y = ground_y (y down: the ground is below the cameras at larger y) and axis-aligned boxes
    (lo, hi), in world coordinates."""

    def __init__(self, ground_y=None, boxes=()):
        self.ground_y = ground_y
        self.boxes = [(np.asarray(lo, np.float64), np.asarray(hi, np.float64)) for lo, hi in boxes]

    def ray_depth(self, origin, dirs):
        """Ray parameter of the first hit of rays origin + lam * dirs (dirs [N, 3] float64), inf for a miss."""
        lam = np.full(dirs.shape[0], np.inf)
        with np.errstate(divide="ignore", invalid="ignore"):
            if self.ground_y is not None:
                l = (self.ground_y - origin[1]) / dirs[:, 1]
                lam = np.where((l > 1e-9) & (l < lam), l, lam)
            for lo, hi in self.boxes:
                t1 = (lo - origin) / dirs
                t2 = (hi - origin) / dirs
                tn = np.nanmax(np.minimum(t1, t2), axis=1)
                tf = np.nanmin(np.maximum(t1, t2), axis=1)
                hit = (tn <= tf) & (tn > 1e-9)
                lam = np.where(hit & (tn < lam), tn, lam)
        return lam

    def distance(self, pts):
        """Unsigned distance of points [N, 3] to the nearest primitive's surface."""
        p = np.asarray(pts, np.float64)
        dist = np.full(p.shape[0], np.inf)
        if self.ground_y is not None:
            dist = np.minimum(dist, np.abs(p[:, 1] - self.ground_y))
        for lo, hi in self.boxes:
            c, h = (lo + hi) / 2, (hi - lo) / 2
            q = np.abs(p - c) - h
            outside = np.linalg.norm(np.maximum(q, 0.0), axis=1)
            inside = np.minimum(q.max(axis=1), 0.0)
            dist = np.minimum(dist, np.abs(outside + inside))
        return dist

    def face_normals(self, pts, margin):
        """(normals [N, 3], interior [N] bool): the outward normal of the surface nearest to each point, and whether the
        point lies on a face interior -- at least `margin` from the face's edges and from every other primitive."""
        p = np.asarray(pts, np.float64)
        cands = []                                                    # (distance, normal, interior) per primitive
        if self.ground_y is not None:
            n = np.zeros_like(p)
            n[:, 1] = -1.0
            cands.append((np.abs(p[:, 1] - self.ground_y), n, np.ones(len(p), bool)))
        for lo, hi in self.boxes:
            c, h = (lo + hi) / 2, (hi - lo) / 2
            q = np.abs(p - c) - h
            ax = q.argmax(axis=1)
            n = np.zeros_like(p)
            n[np.arange(len(p)), ax] = np.sign(p - c)[np.arange(len(p)), ax]
            qs = np.sort(q, axis=1)
            cands.append((self.__class__(boxes=[(lo, hi)]).distance(p), n, qs[:, 1] < -margin))
        d = np.stack([c[0] for c in cands])
        best = d.argmin(axis=0)
        r = np.arange(len(p))
        nrm = np.stack([c[1] for c in cands])[best, r]
        interior = np.stack([c[2] for c in cands])[best, r]
        ds = np.sort(d, axis=0)
        if len(cands) > 1:
            interior &= ds[1] > margin
        return nrm, interior

    def render(self, camera_to_world, H, W, fx, cx, cy, baseline):
        """Exact disparity [H, W] float32 (f*B/Z in float64, rounded once) of the pose, -1 where a ray hits nothing."""
        m = np.asarray(camera_to_world, np.float64)
        v, u = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
        dc = np.stack([(u - cx) / fx, (v - cy) / fx, np.ones_like(u)], axis=-1).reshape(-1, 3)   # z = 1: lam = Z
        dw = dc @ m[:3, :3].T
        Z = self.ray_depth(m[:3, 3], dw)
        d = np.where(np.isfinite(Z), fx * baseline / Z, -1.0)
        return d.reshape(H, W).astype(np.float32)


def demo_scene() -> Scene:
    """A ground plane 1.5 below the cameras and three boxes standing on it."""
    return Scene(ground_y=1.5, boxes=[((-1.6, 0.3, 5.0), (-0.4, 1.5, 6.2)), ((0.6, -0.2, 6.0), (1.8, 1.5, 7.0)),
                                      ((-0.5, 0.7, 8.0), (0.9, 1.5, 9.0))])


def orbit_poses(count, radius=0.8, centre=(0.0, 0.0, 1.0), target=(0.0, 0.8, 7.0)):
    """count camera-to-world poses on a small circle around centre, all looking at target."""
    poses = []
    for a in np.linspace(0.0, 2 * np.pi, count, endpoint=False):
        eye = np.asarray(centre) + radius * np.array([np.cos(a), 0.3 * np.sin(a), np.sin(a)])
        poses.append(look_at(eye, target))
    return np.stack(poses)
