"""`cuda_depth` -- drop-in for the reference's pybind11 torch extension of the same name
(/root/reference/src/csrc/depth/torch_extension_module.cc:6-27), implemented with ctypes
over the C ABI of libstereo_mi355x.so (hand-written HIP kernels for MI355X / gfx950).

Same two classes, same keyword names and defaults:

    cfg = cuda_depth.StereoMatchingConfiguration(height=375, width=1242, min_disparity=0, max_disparity=127)
    sm = cuda_depth.StereoMatching(cfg)
    disparity = sm.compute_disparity_map(left_chw_f32_cuda, right_chw_f32_cuda)   # [H, W] float32

On torch-ROCm `tensor.cuda()` is the HIP device, so the reference's
CudaStereoMatchingBackend body works unchanged.  Errors surface as RuntimeError, as
TORCH_CHECK failures do in the reference (stereo_matching.cc:13-15).
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import math
from typing import Optional, Tuple

import numpy as np
import torch

from . import _native
from ._native import LIB, SmxConfig, SmxDims, check

_U32_FIELDS = ("height", "width", "downscale_factor", "ncc_patch_radius", "sad_patch_radius", "threshold")
_I32_FIELDS = ("min_disparity", "max_disparity", "small_mbm_radius", "mid_mbm_radius", "large_mbm_radius")


class StereoMatchingConfiguration:
    """torch_extension_module.cc:7-20 -- 11 keyword arguments, identical names and defaults
    (including the pybind layer's width=1980, which differs from the struct's 1920)."""

    def __init__(self, height: int = 1080, width: int = 1980, downscale_factor: int = 2,
                 min_disparity: int = 75, max_disparity: int = 262, ncc_patch_radius: int = 1,
                 sad_patch_radius: int = 5, threshold: int = 5, small_mbm_radius: int = 1,
                 mid_mbm_radius: int = 4, large_mbm_radius: int = 10):
        values = dict(height=height, width=width, downscale_factor=downscale_factor,
                      min_disparity=min_disparity, max_disparity=max_disparity,
                      ncc_patch_radius=ncc_patch_radius, sad_patch_radius=sad_patch_radius,
                      threshold=threshold, small_mbm_radius=small_mbm_radius,
                      mid_mbm_radius=mid_mbm_radius, large_mbm_radius=large_mbm_radius)
        for name, v in values.items():
            # pybind11 rejects non-integers and negative values for uint32_t with TypeError
            if isinstance(v, bool) or not isinstance(v, int):
                raise TypeError(f"StereoMatchingConfiguration: '{name}' must be an int")
            if name in _U32_FIELDS and not (0 <= v < 2 ** 32):
                raise TypeError(f"StereoMatchingConfiguration: '{name}' must fit uint32_t")
            if name in _I32_FIELDS and not (-2 ** 31 <= v < 2 ** 31):
                raise TypeError(f"StereoMatchingConfiguration: '{name}' must fit int32_t")
        self._values = values

    def _as_struct(self, device_id: int, max_batch: int, match_mode: int) -> SmxConfig:
        c = SmxConfig()
        for name, v in self._values.items():
            setattr(c, name, v)
        c.device_id, c.max_batch, c.match_mode = device_id, max_batch, match_mode
        return c

    def __repr__(self) -> str:
        return "StereoMatchingConfiguration(" + ", ".join(f"{k}={v}" for k, v in self._values.items()) + ")"


def build_features() -> dict:
    """What libstereo_mi355x.so was built with (smx_build_features)."""
    f = LIB.smx_build_features()
    return {"experimental": bool(f & _native.FEATURE_EXPERIMENTAL)}


def _check_input(name: str, t: torch.Tensor) -> None:
    # stereo_matching.cc:13-15 CHECK_INPUT: same messages
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be a CUDA tensor")
    if not t.is_contiguous():
        raise RuntimeError(f"{name} must be contiguous")


def _check_like(name: str, t: torch.Tensor, dtype: torch.dtype, shape: tuple, device: torch.device) -> None:
    """An operand that must match a reference tensor's dtype, shape and device."""
    _check_input(name, t)
    if t.dtype != dtype or tuple(t.shape) != tuple(shape) or t.device != device:
        raise RuntimeError(f"{name} must be {str(dtype).removeprefix('torch.')} {tuple(shape)} on {device}")


def _int_arg(name: str, v) -> None:
    if isinstance(v, bool) or not isinstance(v, int):
        raise TypeError(f"{name} must be an int")


def _number_arg(name: str, v) -> None:
    if isinstance(v, bool) or not isinstance(v, (int, float)):
        raise TypeError(f"{name} must be a number")


def _stream(device_index: int) -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream(device_index).cuda_stream)


def _check_lr_scalars(max_diff, invalid_disparity) -> None:
    _number_arg("max_diff", max_diff)
    _number_arg("invalid_disparity", invalid_disparity)
    if not (math.isfinite(max_diff) and max_diff >= 0):
        raise RuntimeError(f"max_diff must be finite and >= 0, got {max_diff}")
    if not math.isfinite(invalid_disparity):
        raise RuntimeError(f"invalid_disparity must be finite (a NaN marker never compares equal), got {invalid_disparity}")


def left_right_check(left_disp: torch.Tensor, right_disp: torch.Tensor, *, max_diff: float = 1.0,
                     invalid_disparity: float = -1.0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Left-right consistency check of maps the caller already has (smx_lr_check): left_disp referenced to the left
    image, right_disp to the right image, both [H,W] or [n,H,W] float32 on one device.  Returns left_disp with every
    pixel whose match does not point back to it within max_diff replaced by invalid_disparity.  `out` may be left_disp."""
    _check_input("left_disp", left_disp)
    _check_input("right_disp", right_disp)
    if left_disp.dtype != torch.float32 or right_disp.dtype != torch.float32:
        raise RuntimeError("left_disp and right_disp must be torch.float32")
    if left_disp.dim() not in (2, 3) or tuple(right_disp.shape) != tuple(left_disp.shape):
        raise RuntimeError(f"left_disp and right_disp must both be [H,W] or [n,H,W] of one shape, got "
                           f"{tuple(left_disp.shape)} / {tuple(right_disp.shape)}")
    if right_disp.device != left_disp.device:
        raise RuntimeError("left_disp and right_disp must live on the same device")
    _check_lr_scalars(max_diff, invalid_disparity)
    if out is None:
        out = torch.empty_like(left_disp)
    else:
        _check_like("out", out, torch.float32, left_disp.shape, left_disp.device)
    n = 1 if left_disp.dim() == 2 else int(left_disp.shape[0])
    H, W = int(left_disp.shape[-2]), int(left_disp.shape[-1])
    if left_disp.numel() == 0:
        raise RuntimeError("left_disp is empty")
    dev = left_disp.device.index
    check(LIB.smx_lr_check(dev, n, H, W, left_disp.data_ptr(), right_disp.data_ptr(), out.data_ptr(), float(max_diff),
                           float(invalid_disparity), _stream(dev)))
    return out


def _postprocess_operands(disp: torch.Tensor, out: Optional[torch.Tensor]):
    """Shared checks of filter_speckles / fill_invalid: (out, n, H, W)."""
    _check_input("disp", disp)
    if disp.dtype != torch.float32:
        raise RuntimeError("disp must be torch.float32")
    if disp.dim() not in (2, 3) or disp.numel() == 0:
        raise RuntimeError(f"disp must be a non-empty [H,W] or [n,H,W] map, got {tuple(disp.shape)}")
    if out is None:
        out = torch.empty_like(disp)
    else:
        _check_like("out", out, torch.float32, disp.shape, disp.device)
    n = 1 if disp.dim() == 2 else int(disp.shape[0])
    return out, n, int(disp.shape[-2]), int(disp.shape[-1])


def _postprocess_workspace(n: int, H: int, W: int, device: torch.device) -> torch.Tensor:
    """Device scratch of smx_postprocess_workspace_bytes(n, H, W) bytes for smx_filter_speckles / smx_fill_invalid."""
    nbytes = int(LIB.smx_postprocess_workspace_bytes(n, H, W))
    if nbytes == 0:
        raise RuntimeError(f"post-processing: need 1 <= H, W <= 32768 (got {H} x {W})")
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def _launch_filter_speckles(disp, out, n, H, W, max_speckle_size, max_diff, invalid_disparity, workspace) -> None:
    dev = disp.device.index
    check(LIB.smx_filter_speckles(dev, n, H, W, disp.data_ptr(), out.data_ptr(), int(max_speckle_size), float(max_diff),
                                  float(invalid_disparity), workspace.data_ptr(), workspace.numel(), _stream(dev)))


def _launch_fill_invalid(disp, out, n, H, W, invalid_disparity, workspace) -> None:
    dev = disp.device.index
    check(LIB.smx_fill_invalid(dev, n, H, W, disp.data_ptr(), out.data_ptr(), float(invalid_disparity),
                               workspace.data_ptr(), workspace.numel(), _stream(dev)))


def _check_speckle_size(max_speckle_size) -> None:
    _int_arg("max_speckle_size", max_speckle_size)
    if not 0 <= max_speckle_size <= 2**31 - 1:
        raise RuntimeError(f"max_speckle_size must be in [0, 2**31 - 1], got {max_speckle_size}")


def filter_speckles(disp: torch.Tensor, *, max_speckle_size: int, max_diff: float = 1.0,
                    invalid_disparity: float = -1.0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Speckle filter (smx_filter_speckles) on the current stream: every connected region of valid pixels whose
    4-neighbours differ by at most max_diff, of max_speckle_size pixels or fewer, becomes invalid_disparity; every other
    pixel is copied.  disp: [H,W] or [n,H,W] float32 on a GPU (the n maps are independent).  `out` may be disp."""
    _check_speckle_size(max_speckle_size)
    _check_lr_scalars(max_diff, invalid_disparity)
    out, n, H, W = _postprocess_operands(disp, out)
    _launch_filter_speckles(disp, out, n, H, W, max_speckle_size, max_diff, invalid_disparity,
                            _postprocess_workspace(n, H, W, disp.device))
    return out


def fill_invalid(disp: torch.Tensor, *, invalid_disparity: float = -1.0,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Background hole fill (smx_fill_invalid) on the current stream: every non-valid pixel takes the smaller of the
    nearest valid values to its left and right in its row; rows without a valid pixel take the smaller of the nearest
    non-empty rows above and below.  disp: [H,W] or [n,H,W] float32 on a GPU.  `out` may be disp."""
    _check_lr_scalars(0.0, invalid_disparity)
    out, n, H, W = _postprocess_operands(disp, out)
    _launch_fill_invalid(disp, out, n, H, W, invalid_disparity, _postprocess_workspace(n, H, W, disp.device))
    return out


def _check_median_params(radius, sigma_color, sigma_space) -> None:
    _int_arg("radius", radius)
    if not 1 <= radius <= 15:
        raise RuntimeError(f"radius must be in 1..15, got {radius}")
    for name, v in (("sigma_color", sigma_color), ("sigma_space", sigma_space)):
        _number_arg(name, v)
        if not (math.isfinite(v) and v > 0):
            raise RuntimeError(f"{name} must be finite and > 0, got {v}")


def median_weight_tables(radius: int, sigma_color: float, sigma_space: float):
    """The integer weight tables of smx_weighted_median, in float64:
    range[k] = floor(1023 exp(-k^2 / (2 sigma_color^2)) + 0.5) for k in 0..255 and
    spatial[|dy| (radius+1) + |dx|] = floor(1023 exp(-(dx^2 + dy^2) / (2 sigma_space^2)) + 0.5).
    Returns (range uint16[256], spatial uint16[(radius+1)^2]) as numpy arrays."""
    import numpy as np
    _check_median_params(radius, sigma_color, sigma_space)
    sc2, ss2 = 2.0 * float(sigma_color) ** 2, 2.0 * float(sigma_space) ** 2
    rng = np.array([math.floor(1023.0 * math.exp(-(k * k) / sc2) + 0.5) for k in range(256)], np.uint16)
    spatial = np.array([math.floor(1023.0 * math.exp(-(dx * dx + dy * dy) / ss2) + 0.5)
                        for dy in range(radius + 1) for dx in range(radius + 1)], np.uint16)
    return rng, spatial


def _median_workspace(n: int, H: int, W: int, device: torch.device) -> Optional[torch.Tensor]:
    """Device scratch of smx_median_workspace_bytes(n, H, W) bytes, or None when the query is 0."""
    nbytes = int(LIB.smx_median_workspace_bytes(n, H, W))
    return torch.empty(nbytes, dtype=torch.uint8, device=device) if nbytes else None


def _launch_weighted_median(disp, holes, guide, out, n, H, W, radius, range_weight, spatial_weight, invalid_disparity,
                            workspace) -> None:
    """smx_weighted_median on the current stream; range_weight / spatial_weight: numpy uint16 host tables."""
    import numpy as np
    dev = disp.device.index
    rw = np.ascontiguousarray(range_weight, np.uint16)
    sw = np.ascontiguousarray(spatial_weight, np.uint16)
    if rw.shape != (256,) or sw.shape != ((radius + 1) ** 2,):
        raise RuntimeError(f"weight tables must be uint16[256] and uint16[{(radius + 1) ** 2}], got {rw.shape} and "
                           f"{sw.shape}")
    check(LIB.smx_weighted_median(dev, n, H, W, disp.data_ptr(), holes.data_ptr() if holes is not None else None,
                                  guide.data_ptr(), out.data_ptr(), int(radius), rw.ctypes.data, sw.ctypes.data,
                                  float(invalid_disparity), workspace.data_ptr() if workspace is not None else None,
                                  workspace.numel() if workspace is not None else 0, _stream(dev)))


def weighted_median(disp: torch.Tensor, guide: torch.Tensor, *, radius: int, sigma_color: float, sigma_space: float,
                    holes: Optional[torch.Tensor] = None, invalid_disparity: float = -1.0,
                    out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Image-guided weighted median (smx_weighted_median) on the current stream, with the tables of
    median_weight_tables(radius, sigma_color, sigma_space).  Each filtered pixel becomes the weighted median of the valid
    values of disp in its (2 radius + 1)^2 window, a sample weighing more the closer it lies and the closer its guide
    intensity is to the centre's.  holes=None filters every valid pixel of disp; otherwise only the pixels that are not
    valid in holes (the pre-fill map: the pixels the fill wrote), and every other pixel is copied.  disp, guide, holes,
    out: [H,W] or [n,H,W] float32 on one GPU.  out must not overlap disp or guide; it may be holes."""
    _check_median_params(radius, sigma_color, sigma_space)
    _check_lr_scalars(0.0, invalid_disparity)
    out, n, H, W = _postprocess_operands(disp, out)
    _check_like("guide", guide, torch.float32, disp.shape, disp.device)
    if holes is not None:
        _check_like("holes", holes, torch.float32, disp.shape, disp.device)
    rw, sw = median_weight_tables(radius, sigma_color, sigma_space)
    _launch_weighted_median(disp, holes, guide, out, n, H, W, radius, rw, sw, invalid_disparity,
                            _median_workspace(n, H, W, disp.device))
    return out


def _check_wls_params(lam, sigma_color, iterations, attenuation) -> None:
    _number_arg("lam", lam)
    if not (math.isfinite(lam) and 0 <= lam <= 2.0 ** 20):
        raise RuntimeError(f"lam must be finite in [0, 2**20], got {lam}")
    _number_arg("sigma_color", sigma_color)
    if not (math.isfinite(sigma_color) and sigma_color > 0):
        raise RuntimeError(f"sigma_color must be finite and > 0, got {sigma_color}")
    _int_arg("iterations", iterations)
    if not 1 <= iterations <= 8:
        raise RuntimeError(f"iterations must be in 1..8, got {iterations}")
    _number_arg("attenuation", attenuation)
    if not (math.isfinite(attenuation) and 0 < attenuation <= 1):
        raise RuntimeError(f"attenuation must be in (0, 1], got {attenuation}")


def wls_tables(lam: float, sigma_color: float, iterations: int = 3, attenuation: float = 0.25):
    """The float32 tables of smx_wls_filter, each computed in float64 and rounded once: lambdas[t] =
    lam * attenuation**t for t in 0..iterations-1 (the lambda schedule of the fast global smoother) and
    range_weight[k] = exp(-k / sigma_color) for k in 0..255.  Returns (lambdas float32[iterations],
    range_weight float32[256]) as numpy arrays."""
    import numpy as np
    _check_wls_params(lam, sigma_color, iterations, attenuation)
    lambdas = np.array([float(lam) * float(attenuation) ** t for t in range(iterations)], np.float64).astype(np.float32)
    rw = np.array([math.exp(-k / float(sigma_color)) for k in range(256)], np.float64).astype(np.float32)
    return lambdas, rw


def _wls_workspace(n: int, H: int, W: int, device: torch.device) -> torch.Tensor:
    """Device scratch of smx_wls_workspace_bytes(n, H, W) bytes for smx_wls_filter."""
    nbytes = int(LIB.smx_wls_workspace_bytes(n, H, W))
    if nbytes == 0:
        raise RuntimeError(f"wls_filter: need 1 <= H, W <= 32768 (got {H} x {W})")
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def _launch_wls(disp, confidence, guide, out, n, H, W, lambdas, range_weight, min_weight, invalid_disparity,
                workspace) -> None:
    """smx_wls_filter on the current stream; lambdas / range_weight: numpy float32 host tables."""
    import numpy as np
    dev = disp.device.index
    lam = np.ascontiguousarray(lambdas, np.float32)
    rw = np.ascontiguousarray(range_weight, np.float32)
    if lam.ndim != 1 or rw.shape != (256,):
        raise RuntimeError(f"tables must be float32[iterations] and float32[256], got {lam.shape} and {rw.shape}")
    check(LIB.smx_wls_filter(dev, n, H, W, disp.data_ptr(), confidence.data_ptr() if confidence is not None else None,
                             guide.data_ptr(), out.data_ptr(), int(lam.size), lam.ctypes.data, rw.ctypes.data,
                             float(min_weight), float(invalid_disparity), workspace.data_ptr(), workspace.numel(),
                             _stream(dev)))


def _check_min_weight(min_weight) -> None:
    _number_arg("min_weight", min_weight)
    if not (math.isfinite(min_weight) and min_weight >= 0):
        raise RuntimeError(f"min_weight must be finite and >= 0, got {min_weight}")


def wls_filter(disp: torch.Tensor, guide: torch.Tensor, *, lam: float = 8000.0, sigma_color: float = 1.5,
               iterations: int = 3, attenuation: float = 0.25, confidence: Optional[torch.Tensor] = None,
               min_weight: float = 1e-3, invalid_disparity: float = -1.0,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Image-guided weighted least squares filter (smx_wls_filter) on the current stream, with the tables of
    wls_tables(lam, sigma_color, iterations, attenuation).  Every pixel is rewritten: the confidence-weighted average of
    the valid pixels, spread along each row and column by `iterations` tridiagonal solves whose coupling across a guide
    step of k grey levels is lam * exp(-k / sigma_color).  The result is dense, smooth inside surfaces, with edges that
    follow the guide's; a pixel whose accumulated weight is at most min_weight (far from any valid pixel) becomes
    invalid_disparity.  confidence: None (every valid pixel weighs 1) or per-pixel weights, clamped to [0, 1].
    disp, guide, confidence, out: [H,W] or [n,H,W] float32 on one GPU (the n maps are independent); out may be disp.
    The defaults lam = 8000, sigma_color = 1.5 and min_weight = 1e-3 are judgement calls in the range OpenCV's
    DisparityWLSFilter users take, not the result of a measurement on this project's data."""
    _check_wls_params(lam, sigma_color, iterations, attenuation)
    _check_min_weight(min_weight)
    _check_lr_scalars(0.0, invalid_disparity)
    out, n, H, W = _postprocess_operands(disp, out)
    _check_like("guide", guide, torch.float32, disp.shape, disp.device)
    if confidence is not None:
        _check_like("confidence", confidence, torch.float32, disp.shape, disp.device)
    lambdas, rw = wls_tables(lam, sigma_color, iterations, attenuation)
    _launch_wls(disp, confidence, guide, out, n, H, W, lambdas, rw, min_weight, invalid_disparity,
                _wls_workspace(n, H, W, disp.device))
    return out


def _check_confidence_params(radius, lr_scale, texture_scale, invalid_disparity, radius_zero_ok: bool = False) -> None:
    """The scalar rules of smx_confidence_map, checked before the device is touched (radius 0: no texture term, where
    the caller allows it)."""
    _int_arg("radius", radius)
    if not ((radius_zero_ok and radius == 0) or 1 <= radius <= 15):
        raise RuntimeError(f"radius must be in {'0..15' if radius_zero_ok else '1..15'}, got {radius}")
    for name, v in (("lr_scale", lr_scale), ("texture_scale", texture_scale)):
        _number_arg(name, v)
        if not (math.isfinite(v) and v > 0):
            raise RuntimeError(f"{name} must be finite and > 0, got {v}")
    _number_arg("invalid_disparity", invalid_disparity)
    if not math.isfinite(invalid_disparity):
        raise RuntimeError(f"invalid_disparity must be finite (a NaN marker never compares equal), got {invalid_disparity}")


def _launch_confidence(disp, right_disp, guide, out, n, H, W, radius, lr_scale, texture_scale,
                       invalid_disparity) -> None:
    """smx_confidence_map on the current stream; right_disp / guide may be None."""
    dev = disp.device.index
    check(LIB.smx_confidence_map(dev, n, H, W, disp.data_ptr(), None if right_disp is None else right_disp.data_ptr(),
                                 None if guide is None else guide.data_ptr(), int(radius), float(lr_scale),
                                 float(texture_scale), float(invalid_disparity), out.data_ptr(), _stream(dev)))


def confidence_map(disp: torch.Tensor, right_disp: Optional[torch.Tensor] = None, guide: Optional[torch.Tensor] = None,
                   *, radius: int = 2, lr_scale: float = 1.0, texture_scale: float = 10.0,
                   invalid_disparity: float = -1.0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Per-pixel confidence in [0, 1] of a disparity map (smx_confidence_map; the rule is in include/stereo_mi355x.h), on
    the current stream: 0 on every non-valid pixel, otherwise c_lr * c_tex.  right_disp (the un-checked right-view map,
    e.g. compute_disparity_map_batch_lr's right_out or StereoSGM.compute's right_out): c_lr = max(0, 1 - |d - r| /
    lr_scale) with r the right-view value the pixel points at (0 where it points outside the image or at a non-valid
    value); None: c_lr = 1.  guide (e.g. the left gray plane): c_tex = min(1, (max - min) / texture_scale) over the
    (2 radius + 1)^2 window; None: c_tex = 1.  disp, right_disp, guide, out: [H,W] or [n,H,W] float32 on one GPU (the n
    maps are independent); out must not overlap the inputs.  The defaults lr_scale = 1 px, radius = 2 and
    texture_scale = 10 gray levels are starting points, not values tuned on this project's data."""
    _check_confidence_params(radius, lr_scale, texture_scale, invalid_disparity)
    out, n, H, W = _postprocess_operands(disp, out)
    if right_disp is not None:
        _check_like("right_disp", right_disp, torch.float32, disp.shape, disp.device)
    if guide is not None:
        _check_like("guide", guide, torch.float32, disp.shape, disp.device)
    _launch_confidence(disp, right_disp, guide, out, n, H, W, radius, lr_scale, texture_scale, invalid_disparity)
    return out


def _check_temporal_params(motion_radius, motion_threshold, decay, max_diff, max_weight, min_weight,
                           invalid_disparity) -> None:
    """The scalar rules of smx_temporal_filter, checked before the device is touched."""
    _int_arg("motion_radius", motion_radius)
    if not 0 <= motion_radius <= 7:
        raise RuntimeError(f"motion_radius must be in 0..7, got {motion_radius}")
    for name, v in (("motion_threshold", motion_threshold), ("decay", decay), ("max_diff", max_diff),
                    ("max_weight", max_weight), ("min_weight", min_weight), ("invalid_disparity", invalid_disparity)):
        _number_arg(name, v)
    for name, v in (("motion_threshold", motion_threshold), ("max_diff", max_diff), ("min_weight", min_weight)):
        if not (math.isfinite(v) and v >= 0):
            raise RuntimeError(f"{name} must be finite and >= 0, got {v}")
    if not 0 < decay <= 1:
        raise RuntimeError(f"decay must be in (0, 1], got {decay}")
    if not (math.isfinite(max_weight) and max_weight > 0):
        raise RuntimeError(f"max_weight must be finite and > 0, got {max_weight}")
    if not math.isfinite(invalid_disparity):
        raise RuntimeError(f"invalid_disparity must be finite (a NaN marker never compares equal), got {invalid_disparity}")


def _launch_temporal(disp, confidence, guide, prev_guide, state_disp, state_weight, guide_out, out, n, H, W,
                     motion_radius, motion_threshold, decay, max_diff, max_weight, min_weight,
                     invalid_disparity) -> None:
    """smx_temporal_filter on the current stream; confidence / guide_out may be None."""
    dev = disp.device.index
    check(LIB.smx_temporal_filter(dev, n, H, W, disp.data_ptr(), None if confidence is None else confidence.data_ptr(),
                                  guide.data_ptr(), prev_guide.data_ptr(), state_disp.data_ptr(),
                                  state_weight.data_ptr(), None if guide_out is None else guide_out.data_ptr(),
                                  out.data_ptr(), int(motion_radius), float(motion_threshold), float(decay),
                                  float(max_diff), float(max_weight), float(min_weight), float(invalid_disparity),
                                  _stream(dev)))


class TemporalFilter:
    """Motion-gated temporal filter of n independent disparity-map streams (smx_temporal_filter; the rule is in
    include/stereo_mi355x.h).  Where the guide (the left gray plane) has not changed around a pixel since the previous
    call (the mean |g - G| over the (2 motion_radius + 1)^2 window is at most motion_threshold), a valid measurement is
    blended with the pixel's history if they agree within max_diff, and an invalid one holds the history while its
    weight, decayed by `decay` per call, stays at least min_weight.  Everywhere else the measurement is taken as it is
    and the history restarts: without motion compensation the filter does little on a moving camera, but never smears.
    The history's weight is capped at max_weight.  The filter keeps the state (D, A) and the previous guide (two
    ping-pong buffers), so a caller only passes each frame's map and guide.  The defaults are starting points, not values
    tuned on this project's data."""

    def __init__(self, n: int, H: int, W: int, *, device=None, motion_radius: int = 1, motion_threshold: float = 4.0,
                 decay: float = 0.8, max_diff: float = 1.0, max_weight: float = 8.0, min_weight: float = 0.25,
                 invalid_disparity: float = -1.0):
        for name, v in (("n", n), ("H", H), ("W", W)):
            _int_arg(name, v)
        if not (n >= 1 and 1 <= H <= 32768 and 1 <= W <= 32768):
            raise RuntimeError(f"need n >= 1 and 1 <= H, W <= 32768 (got n {n}, H {H}, W {W})")
        _check_temporal_params(motion_radius, motion_threshold, decay, max_diff, max_weight, min_weight,
                               invalid_disparity)
        device = torch.device("cuda") if device is None else torch.device(device)
        if device.type != "cuda":
            raise RuntimeError(f"TemporalFilter needs a GPU device, got {device}")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.n, self.H, self.W, self.device = n, H, W, device
        self.motion_radius = motion_radius
        self.motion_threshold, self.decay, self.max_diff = float(motion_threshold), float(decay), float(max_diff)
        self.max_weight, self.min_weight = float(max_weight), float(min_weight)
        self.invalid_disparity = float(invalid_disparity)
        shape = (n, H, W)
        self._state_disp = torch.full(shape, self.invalid_disparity, dtype=torch.float32, device=device)
        self._state_weight = torch.zeros(shape, dtype=torch.float32, device=device)
        self._guides = torch.zeros((2,) + shape, dtype=torch.float32, device=device)
        self._prev = 0                                  # _guides[_prev] holds the previous call's guide

    @property
    def state(self):
        """(D, A): [n, H, W] views of the filtered map and its weight after the last call."""
        return self._state_disp, self._state_weight

    def reset(self, streams=None) -> None:
        """Forgets the history of every stream (None) or of the listed stream indices: their next call returns the
        measurement at the valid pixels and invalid_disparity elsewhere.  Runs on the current stream."""
        if streams is None:
            self._state_weight.zero_()
            self._state_disp.fill_(self.invalid_disparity)
            return
        idx = list(streams)
        for i in idx:
            _int_arg("stream index", i)
            if not 0 <= i < self.n:
                raise RuntimeError(f"stream index must be in 0..{self.n - 1}, got {i}")
        for i in idx:
            self._state_weight[i].zero_()
            self._state_disp[i].fill_(self.invalid_disparity)

    def apply(self, disp: torch.Tensor, guide: torch.Tensor, confidence: Optional[torch.Tensor] = None,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Filters one frame of every stream on the current stream and returns the filtered map(s).  disp, guide,
        confidence, out: float32 [n, H, W] on the filter's device ([H, W] also for n = 1).  confidence: None (every valid
        pixel weighs 1) or per-pixel weights, clamped to [0, 1], e.g. cuda_depth.confidence_map.  out=disp filters in
        place; out must not overlap guide or confidence."""
        _check_input("disp", disp)
        shape = (self.n, self.H, self.W)
        if not (tuple(disp.shape) == shape or (self.n == 1 and tuple(disp.shape) == shape[1:])):
            raise RuntimeError(f"disp must be float32 {shape} on {self.device}" +
                               (f" or {shape[1:]}" if self.n == 1 else "") + f", got {tuple(disp.shape)}")
        _check_like("disp", disp, torch.float32, disp.shape, self.device)
        _check_like("guide", guide, torch.float32, disp.shape, self.device)
        if confidence is not None:
            _check_like("confidence", confidence, torch.float32, disp.shape, self.device)
        if out is None:
            out = torch.empty_like(disp)
        else:
            _check_like("out", out, torch.float32, disp.shape, self.device)
        prev, nxt = self._guides[self._prev], self._guides[1 - self._prev]
        _launch_temporal(disp, confidence, guide, prev, self._state_disp, self._state_weight, nxt, out, self.n, self.H,
                         self.W, self.motion_radius, self.motion_threshold, self.decay, self.max_diff, self.max_weight,
                         self.min_weight, self.invalid_disparity)
        self._prev = 1 - self._prev
        return out


def _shape2(name: str, shape) -> tuple:
    try:
        h, w = (int(v) for v in shape)
    except (TypeError, ValueError):
        raise TypeError(f"{name} must be a (height, width) pair") from None
    if not (1 <= h <= 32768 and 1 <= w <= 32768):
        raise ValueError(f"{name} must lie in 1..32768, got {(h, w)}")
    return h, w


def rectification_map(K, dist, R, P, in_shape, out_shape):
    """The float64 rectification map of one camera, in the model and formula order of OpenCV's initUndistortRectifyMap:
    for each output pixel (u, v), X = inv(P[:, :3] @ R) @ [u, v, 1], x = X0 / X2, y = X1 / X2, then the radial
    (k1, k2, k3) and tangential (p1, p2) distortion of dist = (k1, k2, p1, p2[, k3]), then K.  A pixel with X2 <= 0 or a
    non-finite result is marked outside (NaN, which quantize_map sends outside the input).
    K: 3x3 raw intrinsics; R: 3x3 rectifying rotation; P: 3x3 or 3x4 rectified projection (only P[:, :3] is used).
    in_shape / out_shape: (height, width) of the raw and rectified images.  Returns (map_x, map_y), float64 [H_out, W_out]
    of raw-image pixel coordinates."""
    import numpy as np
    _shape2("in_shape", in_shape)
    Ho, Wo = _shape2("out_shape", out_shape)
    K = np.asarray(K, np.float64).reshape(3, 3)
    R = np.asarray(R, np.float64).reshape(3, 3)
    P = np.asarray(P, np.float64)
    if P.shape not in ((3, 3), (3, 4)):
        P = P.reshape(3, -1)
    d = np.zeros(5)
    dist = np.asarray(dist if dist is not None else [], np.float64).reshape(-1)
    if dist.size not in (0, 4, 5):
        raise ValueError(f"dist must hold 4 or 5 entries (k1, k2, p1, p2[, k3]), got {dist.size}")
    d[:dist.size] = dist
    k1, k2, p1, p2, k3 = d
    iR = np.linalg.inv(P[:, :3] @ R)
    v, u = np.meshgrid(np.arange(Ho, dtype=np.float64), np.arange(Wo, dtype=np.float64), indexing="ij")
    X0 = iR[0, 0] * u + iR[0, 1] * v + iR[0, 2]
    X1 = iR[1, 0] * u + iR[1, 1] * v + iR[1, 2]
    X2 = iR[2, 0] * u + iR[2, 1] * v + iR[2, 2]
    with np.errstate(all="ignore"):
        x, y = X0 / X2, X1 / X2
        x2, y2 = x * x, y * y
        r2 = x2 + y2
        xy2 = 2 * x * y
        kr = 1 + ((k3 * r2 + k2) * r2 + k1) * r2
        xd = x * kr + p1 * xy2 + p2 * (r2 + 2 * x2)
        yd = y * kr + p1 * (r2 + 2 * y2) + p2 * xy2
        map_x = K[0, 0] * xd + K[0, 1] * yd + K[0, 2]
        map_y = K[1, 1] * yd + K[1, 2]
    bad = ~(X2 > 0) | ~np.isfinite(map_x) | ~np.isfinite(map_y)
    map_x[bad] = np.nan
    map_y[bad] = np.nan
    return map_x, map_y


def quantize_map(map_x, map_y, in_shape):
    """float maps of raw-image pixel coordinates -> the int32 [H_out, W_out, 2] map of smx_remap_pairs, (x, y) in 1/32
    pixel: q = floor(m * 32 + 0.5), clamped to [-64, (W_in + 1) * 32] for x and [-64, (H_in + 1) * 32] for y (outside
    the input, every tap lies outside too); a non-finite entry becomes -64.  Takes any float map, e.g. one of OpenCV."""
    import numpy as np
    Hi, Wi = _shape2("in_shape", in_shape)
    mx, my = np.asarray(map_x, np.float64), np.asarray(map_y, np.float64)
    if mx.ndim != 2 or mx.shape != my.shape:
        raise ValueError(f"map_x and map_y must be 2-D of one shape, got {mx.shape} and {my.shape}")
    q = np.empty(mx.shape + (2,), np.int32)
    for k, (m, hi) in enumerate(((mx, (Wi + 1) * 32), (my, (Hi + 1) * 32))):
        with np.errstate(all="ignore"):
            f = np.floor(m * 32.0 + 0.5)
        f = np.where(np.isfinite(f), np.clip(f, -64, hi), -64)
        q[..., k] = f.astype(np.int32)
    return q


def _valid_taps(qmap, in_shape):
    """bool [H_out, W_out]: every tap of non-zero weight of the quantised map lies inside the input (a tap of weight 0
    is not read, so it does not count)."""
    import numpy as np
    Hi, Wi = in_shape
    q = np.asarray(qmap, np.int64)
    x0, y0, fx, fy = q[..., 0] >> 5, q[..., 1] >> 5, q[..., 0] & 31, q[..., 1] & 31
    x1 = np.where(fx > 0, x0 + 1, x0)
    y1 = np.where(fy > 0, y0 + 1, y0)
    return (x0 >= 0) & (x1 < Wi) & (y0 >= 0) & (y1 < Hi)


_BORDERS = {"constant": _native.BORDER_CONSTANT, "replicate": _native.BORDER_REPLICATE}


class StereoRectification:
    """Rectification of raw stereo frames on the GPU (smx_remap_pairs): both views of a batch in one launch, each
    through its own int32 map (quantize_map).  left_map / right_map: int32 [H_out, W_out, 2] (numpy or tensor);
    in_shape / out_shape: (height, width) of the raw and rectified frames; border_mode 'constant' (taps outside read
    border_value) or 'replicate' (taps clamped to the image).  left_valid: device bool [H_out, W_out], the output pixels
    whose left-view taps of non-zero weight all lie inside the raw image."""

    def __init__(self, left_map, right_map, in_shape, out_shape, *, border_mode: str = "constant",
                 border_value: float = 0.0, device=None):
        import numpy as np
        self.in_shape = _shape2("in_shape", in_shape)
        self.out_shape = _shape2("out_shape", out_shape)
        if border_mode not in _BORDERS:
            raise ValueError(f"border_mode must be 'constant' or 'replicate', got {border_mode!r}")
        _number_arg("border_value", border_value)
        if not math.isfinite(border_value):
            raise ValueError(f"border_value must be finite, got {border_value}")
        self.border_mode = border_mode
        self.border_value = float(border_value)
        device = torch.device("cuda" if device is None else device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = device
        maps = []
        for name, m in (("left_map", left_map), ("right_map", right_map)):
            m = m.cpu().numpy() if isinstance(m, torch.Tensor) else np.asarray(m)
            if m.dtype != np.int32 or m.shape != self.out_shape + (2,):
                raise ValueError(f"{name} must be int32 {self.out_shape + (2,)}, got {m.dtype} {m.shape}")
            maps.append(m)
        self.left_map = torch.from_numpy(np.ascontiguousarray(maps[0])).to(self.device)
        self.right_map = torch.from_numpy(np.ascontiguousarray(maps[1])).to(self.device)
        self.left_valid = torch.from_numpy(_valid_taps(maps[0], self.in_shape)).to(self.device)

    @classmethod
    def from_calibration(cls, left, right, in_shape, out_shape, **kwargs) -> "StereoRectification":
        """left / right: (K, dist, R, P) of each camera, as rectification_map takes them."""
        maps = [quantize_map(*rectification_map(*cam, in_shape, out_shape), in_shape) for cam in (left, right)]
        return cls(maps[0], maps[1], in_shape, out_shape, **kwargs)

    def _out(self, name, t, like, shape):
        if t is None:
            return torch.empty(shape, dtype=like.dtype, device=like.device)
        _check_like(name, t, like.dtype, shape, like.device)
        return t

    def rectify(self, left: torch.Tensor, right: Optional[torch.Tensor] = None, out=None):
        """Rectifies one pair ([C,H,W]) or a batch ([n,C,H,W]), uint8 or float32, C in 1..4, on the current stream.
        Returns (left_out, right_out) of the same dtype and rank, [.., C, H_out, W_out]; with right=None only the left
        frames are rectified and left_out alone is returned.  out: the output tensor(s) to write, in the same form."""
        _check_input("left", left)
        if left.dtype not in (torch.uint8, torch.float32):
            raise RuntimeError(f"frames must be uint8 or float32, got {left.dtype}")
        if left.dim() not in (3, 4) or not 1 <= int(left.shape[-3]) <= 4:
            raise RuntimeError(f"frames must be [C,H,W] or [n,C,H,W] with C in 1..4, got {tuple(left.shape)}")
        if tuple(left.shape[-2:]) != self.in_shape:
            raise RuntimeError(f"frames must be {self.in_shape[0]}x{self.in_shape[1]} (in_shape), got "
                               f"{tuple(left.shape[-2:])}")
        if left.device != self.device:
            raise RuntimeError(f"frames must live on {self.device}, got {left.device}")
        if left.numel() == 0:
            raise RuntimeError("left is empty")
        if right is not None:
            _check_like("right", right, left.dtype, left.shape, left.device)
        if left.dtype == torch.uint8 and not (0 <= self.border_value <= 255 and self.border_value.is_integer()):
            raise RuntimeError(f"a uint8 border_value must be an integer in 0..255, got {self.border_value}")
        shape = tuple(left.shape[:-2]) + self.out_shape
        if right is None:
            lo, ro = self._out("out", out, left, shape), None
        else:
            if out is not None and (not isinstance(out, (tuple, list)) or len(out) != 2):
                raise TypeError("out must be a (left_out, right_out) pair")
            lo = self._out("out[0]", None if out is None else out[0], left, shape)
            ro = self._out("out[1]", None if out is None else out[1], left, shape)
        n = 1 if left.dim() == 3 else int(left.shape[0])
        dt = _native.DTYPE_U8 if left.dtype == torch.uint8 else _native.DTYPE_F32
        dev = left.device.index
        check(LIB.smx_remap_pairs(dev, n, int(left.shape[-3]), dt, *self.in_shape, *self.out_shape, left.data_ptr(),
                                  None if right is None else right.data_ptr(), self.left_map.data_ptr(),
                                  None if right is None else self.right_map.data_ptr(), lo.data_ptr(),
                                  None if ro is None else ro.data_ptr(), _BORDERS[self.border_mode],
                                  self.border_value, _stream(dev)))
        return lo if right is None else (lo, ro)


def _launch_synthesis(probabilities, left, out, n, channels, D, h, w, scale) -> None:
    """smx_synthesize_right_view on the current stream."""
    dt = _native.DTYPE_U8 if left.dtype == torch.uint8 else _native.DTYPE_F32
    dev = left.device.index
    check(LIB.smx_synthesize_right_view(dev, n, channels, dt, D, h, w, int(scale), probabilities.data_ptr(),
                                        left.data_ptr(), out.data_ptr(), _stream(dev)))


def synthesize_right_view(probabilities: torch.Tensor, left: torch.Tensor, scale: int = 4,
                          out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The right view of `left` under a disparity probability volume (smx_synthesize_right_view; the rule is in
    include/stereo_mi355x.h), on the current stream: everything Deep3D does after the network's softmax -- bilinear
    upsampling by `scale`, the probability-weighted sum of the shifted left frames, `* 255 + 0.5` clamped to 0..255 --
    in one launch that stores neither the upsampled volume nor the shifted frames.  probabilities: [n, D, h, w] or
    [D, h, w] float32 on a GPU, D in 1..256; left: [n, C, H, W], [C, H, W] or [H, W] with C in (1, 3), H = h * scale,
    W = w * scale, float32 (values in 0..1) or uint8 (divided by 255); scale in 1..16.  Returns float32 in 0..255 in
    the shape of left; out: the tensor to write (it must not overlap the inputs).  TypeError for a dtype mistake,
    ValueError for a shape or device mismatch or a non-contiguous operand, before anything is launched."""
    for name, t in (("probabilities", probabilities), ("left", left)) + ((("out", out),) if out is not None else ()):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch.Tensor")
    _int_arg("scale", scale)
    if probabilities.dtype != torch.float32:
        raise TypeError(f"probabilities must be float32, got {probabilities.dtype}")
    if left.dtype not in (torch.uint8, torch.float32):
        raise TypeError(f"left must be uint8 or float32, got {left.dtype}")
    if out is not None and out.dtype != torch.float32:
        raise TypeError(f"out must be float32, got {out.dtype}")
    if not 1 <= scale <= 16:
        raise ValueError(f"scale must be in 1..16, got {scale}")
    if probabilities.dim() not in (3, 4) or probabilities.numel() == 0:
        raise ValueError(f"probabilities must be a non-empty [n, D, h, w] or [D, h, w], got {tuple(probabilities.shape)}")
    batched = probabilities.dim() == 4
    if left.dim() not in ((4,) if batched else (2, 3)):
        raise ValueError(f"left must be {'[n, C, H, W]' if batched else '[C, H, W] or [H, W]'} beside probabilities "
                         f"{tuple(probabilities.shape)}, got {tuple(left.shape)}")
    n = int(probabilities.shape[0]) if batched else 1
    D, h, w = (int(v) for v in probabilities.shape[-3:])
    channels = 1 if left.dim() == 2 else int(left.shape[-3])
    if channels not in (1, 3):
        raise ValueError(f"left must have 1 or 3 channels, got {channels}")
    if not 1 <= D <= 256:
        raise ValueError(f"probabilities must hold 1..256 disparity planes, got {D}")
    if tuple(left.shape[-2:]) != (h * scale, w * scale) or (batched and int(left.shape[0]) != n):
        raise ValueError(f"left must be {'%d frames of ' % n if batched else ''}{h * scale} x {w * scale} "
                         f"(probabilities {h} x {w}, scale {scale}), got {tuple(left.shape)}")
    if h * scale > 32768 or w * scale > 32768:
        raise ValueError(f"frames may be at most 32768 x 32768, got {h * scale} x {w * scale}")
    if out is not None and tuple(out.shape) != tuple(left.shape):
        raise ValueError(f"out must be {tuple(left.shape)} like left, got {tuple(out.shape)}")
    for name, t in (("probabilities", probabilities), ("left", left)) + ((("out", out),) if out is not None else ()):
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
    if not probabilities.is_cuda or left.device != probabilities.device:
        raise ValueError(f"probabilities and left must live on one GPU, got {probabilities.device} and {left.device}")
    if out is not None and out.device != left.device:
        raise ValueError(f"out must live on {left.device}, got {out.device}")
    if out is None:
        out = torch.empty(left.shape, dtype=torch.float32, device=left.device)
    _launch_synthesis(probabilities, left, out, n, channels, D, h, w, scale)
    return out


def _head_volume_geometry(probabilities: torch.Tensor, left: torch.Tensor, scale: int):
    """(n, channels, D, h, w) of synthesis_head's operands, or the TypeError / ValueError that names the mistake."""
    _int_arg("scale", scale)
    if probabilities.dtype != torch.float32:
        raise TypeError(f"probabilities must be float32, got {probabilities.dtype}")
    if left.dtype not in (torch.uint8, torch.float32):
        raise TypeError(f"left must be uint8 or float32, got {left.dtype}")
    if not 1 <= scale <= 16:
        raise ValueError(f"scale must be in 1..16, got {scale}")
    if probabilities.dim() not in (3, 4) or probabilities.numel() == 0:
        raise ValueError(f"probabilities must be a non-empty [n, D, h, w] or [D, h, w], got {tuple(probabilities.shape)}")
    batched = probabilities.dim() == 4
    if left.dim() not in ((4,) if batched else (2, 3)):
        raise ValueError(f"left must be {'[n, C, H, W]' if batched else '[C, H, W] or [H, W]'} beside probabilities "
                         f"{tuple(probabilities.shape)}, got {tuple(left.shape)}")
    n = int(probabilities.shape[0]) if batched else 1
    D, h, w = (int(v) for v in probabilities.shape[-3:])
    channels = 1 if left.dim() == 2 else int(left.shape[-3])
    if channels not in (1, 3):
        raise ValueError(f"left must have 1 or 3 channels, got {channels}")
    if not 1 <= D <= 256:
        raise ValueError(f"probabilities must hold 1..256 disparity planes, got {D}")
    if tuple(left.shape[-2:]) != (h * scale, w * scale) or (batched and int(left.shape[0]) != n):
        raise ValueError(f"left must be {'%d frames of ' % n if batched else ''}{h * scale} x {w * scale} "
                         f"(probabilities {h} x {w}, scale {scale}), got {tuple(left.shape)}")
    if h * scale > 32768 or w * scale > 32768:
        raise ValueError(f"frames may be at most 32768 x 32768, got {h * scale} x {w * scale}")
    if not left.is_contiguous():
        raise ValueError("left must be contiguous")
    if not probabilities.is_cuda or left.device != probabilities.device:
        raise ValueError(f"probabilities and left must live on one GPU, got {probabilities.device} and {left.device}")
    return n, channels, D, h, w


def synthesis_head_backward(grad_view: torch.Tensor, left: torch.Tensor, D: int, scale: int = 4,
                            out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The gradient of the probability volume from the gradient of synthesis_head's view (smx_synthesis_head_backward; the
    rule is in include/stereo_mi355x.h), on the current stream, in one launch that stores neither the upsampled gradient
    nor the shifted frames.  grad_view: [n, C, H, W], [C, H, W] or [H, W] float32 on a GPU; left: the frame the view was
    made from, in the shape of grad_view, float32 (0..1) or uint8; D in 1..256 planes; scale in 1..16 divides H and W.
    Returns float32 [n, D, H / scale, W / scale] ([D, h, w] for unbatched operands); out: the tensor to write (it must
    not overlap the inputs).  TypeError for a dtype mistake, ValueError for a shape or device mismatch or a
    non-contiguous operand, before anything is launched."""
    for name, t in (("grad_view", grad_view), ("left", left)) + ((("out", out),) if out is not None else ()):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch.Tensor")
    _int_arg("D", D)
    _int_arg("scale", scale)
    if grad_view.dtype != torch.float32:
        raise TypeError(f"grad_view must be float32, got {grad_view.dtype}")
    if left.dtype not in (torch.uint8, torch.float32):
        raise TypeError(f"left must be uint8 or float32, got {left.dtype}")
    if out is not None and out.dtype != torch.float32:
        raise TypeError(f"out must be float32, got {out.dtype}")
    if not 1 <= scale <= 16:
        raise ValueError(f"scale must be in 1..16, got {scale}")
    if not 1 <= D <= 256:
        raise ValueError(f"D must be in 1..256 disparity planes, got {D}")
    if grad_view.dim() not in (2, 3, 4) or grad_view.numel() == 0:
        raise ValueError(f"grad_view must be a non-empty [n, C, H, W], [C, H, W] or [H, W], got {tuple(grad_view.shape)}")
    if tuple(left.shape) != tuple(grad_view.shape):
        raise ValueError(f"left must be {tuple(grad_view.shape)} like grad_view, got {tuple(left.shape)}")
    n = int(grad_view.shape[0]) if grad_view.dim() == 4 else 1
    channels = 1 if grad_view.dim() == 2 else int(grad_view.shape[-3])
    H, W = (int(v) for v in grad_view.shape[-2:])
    if channels not in (1, 3):
        raise ValueError(f"grad_view must have 1 or 3 channels, got {channels}")
    if H % scale or W % scale:
        raise ValueError(f"scale {scale} must divide the frame's {H} x {W}")
    if H > 32768 or W > 32768:
        raise ValueError(f"frames may be at most 32768 x 32768, got {H} x {W}")
    h, w = H // scale, W // scale
    shape = ((n,) if grad_view.dim() == 4 else ()) + (D, h, w)
    if out is not None and tuple(out.shape) != shape:
        raise ValueError(f"out must be {shape}, got {tuple(out.shape)}")
    for name, t in (("grad_view", grad_view), ("left", left)) + ((("out", out),) if out is not None else ()):
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
    if not grad_view.is_cuda or left.device != grad_view.device:
        raise ValueError(f"grad_view and left must live on one GPU, got {grad_view.device} and {left.device}")
    if out is not None and out.device != left.device:
        raise ValueError(f"out must live on {left.device}, got {out.device}")
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=left.device)
    dt = _native.DTYPE_U8 if left.dtype == torch.uint8 else _native.DTYPE_F32
    dev = left.device.index
    check(LIB.smx_synthesis_head_backward(dev, n, channels, dt, D, h, w, int(scale), grad_view.data_ptr(),
                                          left.data_ptr(), out.data_ptr(), _stream(dev)))
    return out


class _SynthesisHead(torch.autograd.Function):
    """smx_synthesis_head_forward / _backward as one differentiable operation; only `left` is saved."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, probabilities, left, scale):
        n, channels, D, h, w = _head_volume_geometry(probabilities, left, scale)
        probabilities = probabilities.contiguous()
        view = torch.empty(left.shape, dtype=torch.float32, device=left.device)
        dt = _native.DTYPE_U8 if left.dtype == torch.uint8 else _native.DTYPE_F32
        dev = left.device.index
        check(LIB.smx_synthesis_head_forward(dev, n, channels, dt, D, h, w, int(scale), probabilities.data_ptr(),
                                             left.data_ptr(), view.data_ptr(), _stream(dev)))
        ctx.save_for_backward(left)
        ctx.D, ctx.scale = D, int(scale)
        return view

    @staticmethod
    @torch.autograd.function.once_differentiable
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, grad_view):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        (left,) = ctx.saved_tensors
        grad_view = grad_view.to(torch.float32).contiguous()
        return synthesis_head_backward(grad_view, left, ctx.D, ctx.scale), None, None


def synthesis_head(probabilities: torch.Tensor, left: torch.Tensor, scale: int = 4) -> torch.Tensor:
    """The training form of synthesize_right_view (smx_synthesis_head_forward): the same fused head without the rescale,
    so the view is float32 in 0..1 and unclamped, in the shape of left -- what Deep3D's L1 loss compares with the true
    right frame -- and it is differentiable with respect to probabilities (smx_synthesis_head_backward, one more
    launch).  Operands are synthesize_right_view's: probabilities [n, D, h, w] or [D, h, w] float32 on a GPU, left
    [n, C, H, W], [C, H, W] or [H, W], float32 in 0..1 or uint8.  left gets no gradient: one that requires grad is
    refused with a ValueError.  Only left is kept for the backward pass, never the volume or anything of its size
    times scale^2; the backward pass cannot be differentiated again.  Under autocast the head runs in float32."""
    for name, t in (("probabilities", probabilities), ("left", left)):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch.Tensor")
    _int_arg("scale", scale)
    if left.requires_grad:
        raise ValueError("left gets no gradient from synthesis_head: detach it")
    if not probabilities.is_floating_point():
        raise TypeError(f"probabilities must be float32, got {probabilities.dtype}")
    if not torch.is_autocast_enabled() or not probabilities.is_cuda:
        _head_volume_geometry(probabilities, left, scale)                # refuse before autograd records anything
    return _SynthesisHead.apply(probabilities, left, scale)


class StereoSGM:
    """Semi-global matching with a census 9x7 cost (smx_sgm; the rule is in include/stereo_mi355x.h), a second matcher
    beside StereoMatching.  Candidates are min_disparity..max_disparity (at most 256); paths 4 or 8; 0 <= P1 <= P2 <= 191;
    uniqueness in 0..99 percent (0: off); lr_max_diff None (no check) or a finite value >= 0: pixels whose right-view
    match does not point back within it become invalid_disparity; subpixel: parabola through the winner's neighbours."""

    def __init__(self, min_disparity: int = 0, max_disparity: int = 127, *, paths: int = 8, P1: int = 10,
                 P2: int = 120, uniqueness: int = 0, lr_max_diff: Optional[float] = None, subpixel: bool = True,
                 invalid_disparity: float = -1.0):
        for name, v in (("min_disparity", min_disparity), ("max_disparity", max_disparity), ("paths", paths),
                        ("P1", P1), ("P2", P2), ("uniqueness", uniqueness)):
            _int_arg(name, v)
        if not 0 <= min_disparity <= 32768:
            raise RuntimeError(f"min_disparity must be in 0..32768, got {min_disparity}")
        if not 1 <= max_disparity - min_disparity + 1 <= 256:
            raise RuntimeError(f"need 1 <= max_disparity - min_disparity + 1 <= 256, got {min_disparity}..{max_disparity}")
        if paths not in (4, 8):
            raise RuntimeError(f"paths must be 4 or 8, got {paths}")
        if not 0 <= P1 <= P2 <= 191:
            raise RuntimeError(f"need 0 <= P1 <= P2 <= 191, got P1 {P1}, P2 {P2}")
        if not 0 <= uniqueness <= 99:
            raise RuntimeError(f"uniqueness must be in 0..99 (percent, 0: off), got {uniqueness}")
        if lr_max_diff is not None:
            _number_arg("lr_max_diff", lr_max_diff)
            if not (math.isfinite(lr_max_diff) and lr_max_diff >= 0):
                raise RuntimeError(f"lr_max_diff must be None or finite and >= 0, got {lr_max_diff}")
        if not isinstance(subpixel, bool):
            raise TypeError("subpixel must be a bool")
        _number_arg("invalid_disparity", invalid_disparity)
        if not math.isfinite(invalid_disparity):
            raise RuntimeError(f"invalid_disparity must be finite (a NaN marker never compares equal), got "
                               f"{invalid_disparity}")
        self.min_disparity, self.max_disparity = min_disparity, max_disparity
        self.num_disparities = max_disparity - min_disparity + 1
        self.paths, self.P1, self.P2, self.uniqueness = paths, P1, P2, uniqueness
        self.lr_max_diff = None if lr_max_diff is None else float(lr_max_diff)
        self.subpixel = subpixel
        self.invalid_disparity = float(invalid_disparity)
        self._workspace: dict = {}                          # (device, n, H, W) -> uint8 tensor

    def workspace(self, n: int, H: int, W: int, device: torch.device) -> torch.Tensor:
        """The cached device workspace of smx_sgm for n pairs of H x W frames on `device`."""
        key = (device, n, H, W)
        ws = self._workspace.get(key)
        if ws is None:
            nbytes = int(LIB.smx_sgm_workspace_bytes(n, H, W, self.num_disparities, self.paths))
            if nbytes == 0:
                raise RuntimeError(f"StereoSGM: need 1 <= H, W <= 32768 and n * (H + W) <= 2**31 (got n {n}, {H} x {W})")
            ws = self._workspace[key] = torch.empty(nbytes, dtype=torch.uint8, device=device)
        return ws

    def compute(self, left: torch.Tensor, right: torch.Tensor, out: Optional[torch.Tensor] = None,
                gray_out: Optional[torch.Tensor] = None, right_out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """left, right: [C,H,W] or [n,C,H,W], uint8 or float32, C in {1, 3}, on one GPU.  Returns the float32 disparity
        map(s), [H,W] or [n,H,W], computed on the current stream.  out: the map tensor to write; gray_out: a float32
        tensor of the map's shape that receives the left frames' gray planes (the weighted median's guide); right_out: a
        float32 tensor of the map's shape that receives the right-view winner maps (smx_sgm_with_right_map: integer
        disparities, invalid_disparity where no candidate lies in the image), the right_disp of confidence_map."""
        _check_input("left", left)
        _check_input("right", right)
        if left.dtype not in (torch.uint8, torch.float32):
            raise RuntimeError(f"frames must be uint8 or float32, got {left.dtype}")
        if left.dim() not in (3, 4) or int(left.shape[-3]) not in (1, 3):
            raise RuntimeError(f"frames must be [C,H,W] or [n,C,H,W] with C in (1, 3), got {tuple(left.shape)}")
        if left.numel() == 0:
            raise RuntimeError("left is empty")
        _check_like("right", right, left.dtype, left.shape, left.device)
        shape = (tuple(left.shape[:1]) if left.dim() == 4 else ()) + tuple(left.shape[-2:])
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=left.device)
        else:
            _check_like("out", out, torch.float32, shape, left.device)
        if gray_out is not None:
            _check_like("gray_out", gray_out, torch.float32, shape, left.device)
        if right_out is not None:
            _check_like("right_out", right_out, torch.float32, shape, left.device)
        n = 1 if left.dim() == 3 else int(left.shape[0])
        H, W = int(left.shape[-2]), int(left.shape[-1])
        ws = self.workspace(n, H, W, left.device)
        dt = _native.DTYPE_U8 if left.dtype == torch.uint8 else _native.DTYPE_F32
        dev = left.device.index
        args = (dev, n, int(left.shape[-3]), dt, H, W, left.data_ptr(), right.data_ptr(), self.min_disparity,
                self.num_disparities, self.paths, self.P1, self.P2, self.uniqueness,
                -1.0 if self.lr_max_diff is None else self.lr_max_diff, int(self.subpixel), self.invalid_disparity,
                out.data_ptr(), None if gray_out is None else gray_out.data_ptr())
        if right_out is None:
            check(LIB.smx_sgm(*args, ws.data_ptr(), ws.numel(), _stream(dev)))
        else:
            check(LIB.smx_sgm_with_right_map(*args, right_out.data_ptr(), ws.data_ptr(), ws.numel(), _stream(dev)))
        return out


class StereoMatching:
    """torch_extension_module.cc:22-26.  `compute_disparity_map` is the reference method;
    the keyword-only constructor extras and the *_gray / *_batch methods are additions that
    expose the grayscale and batched entry points of the C ABI."""

    def __init__(self, configuration: Optional[StereoMatchingConfiguration] = None, *,
                 max_batch: int = 1, match_mode: str = "auto", device: Optional[int] = None,
                 overlap_min_pairs: int = 0, exact_filter: int = 0, fp_convention="source"):
        if configuration is None:
            configuration = StereoMatchingConfiguration()
        if not isinstance(configuration, StereoMatchingConfiguration):
            raise TypeError("configuration must be a cuda_depth.StereoMatchingConfiguration")
        if match_mode not in _native.MATCH_MODES:
            raise RuntimeError(f"match_mode must be one of {sorted(_native.MATCH_MODES)}")
        if isinstance(fp_convention, str):
            if fp_convention not in _native.FP_CONVENTIONS:
                raise RuntimeError(f"fp_convention must be one of {sorted(_native.FP_CONVENTIONS)} (or 0..5, or _native.fp_mixed)")
            fp_convention = _native.FP_CONVENTIONS[fp_convention]
        if not torch.cuda.is_available():
            raise RuntimeError("cuda_depth.StereoMatching needs a HIP device (no CPU fallback)")
        self._device = torch.cuda.current_device() if device is None else int(device)
        self._cfg = configuration._as_struct(self._device, int(max_batch), _native.MATCH_MODES[match_mode])
        self._cfg.overlap_min_pairs = int(overlap_min_pairs)      # 0: default threshold, -1: never use stream lanes
        self._cfg.exact_filter = int(exact_filter)                # RGB batches: 0 content-aware, 1 always filtered, -1 always dense
        # how a CUDA build of the reference may have fused step 1 and the parabola (include/stereo_mi355x.h:
        # smx_fp_convention); "source" = no contraction
        self._cfg.fp_convention = int(fp_convention)
        self._dims = SmxDims()
        check(LIB.smx_get_dims(C.byref(self._cfg), C.byref(self._dims)))
        self._handle = C.c_void_p()
        check(LIB.smx_create(C.byref(self._cfg), C.byref(self._handle)))
        self._max_batch = int(max_batch)
        d = self._dims
        dev = torch.device("cuda", self._device)
        # the reference returns an alias of its persistent output buffer (stereo_matching.cc:42)
        self._output = torch.zeros((d.H, d.W), dtype=torch.float32, device=dev)
        self._batch_output: Optional[torch.Tensor] = None
        self._lr_output: Optional[torch.Tensor] = None
        self._out_parity = 0

    # ------------------------------------------------------------------ lifetime
    def __del__(self):
        h = getattr(self, "_handle", None)
        if h is not None and h.value:
            try:
                LIB.smx_destroy(h)
            except Exception:      # interpreter shutdown: module globals may already be gone
                pass
            self._handle = None

    # ------------------------------------------------------------------ helpers
    @property
    def dims(self) -> SmxDims:
        return self._dims

    def _stream(self) -> C.c_void_p:
        return _stream(self._device)

    def _validate(self, name: str, t: torch.Tensor, shape, dtype=torch.float32) -> None:
        _check_input(name, t)
        if t.dtype != dtype:
            raise RuntimeError(f"{name} must be {dtype}, got {t.dtype}")
        if tuple(t.shape) != tuple(shape):
            raise RuntimeError(f"{name} must have shape {tuple(shape)}, got {tuple(t.shape)}")
        if t.device.index != self._device:
            raise RuntimeError(f"{name} must live on cuda:{self._device}")

    def _batch_out(self, n: int, engine_streams: bool = False) -> torch.Tensor:
        """Default output of a batch call: the engine's persistent batch buffer (valid until the next call, like the
        reference's single output, stereo_matching.cc:42).  Engine-stream calls small enough to alternate between the two
        stream lanes (2 n <= max_batch) alternate between the two halves of the buffer as well: two consecutive calls
        then write different memory and pipeline (the engine orders calls whose outputs overlap), and a result stays
        valid until the call after next."""
        d = self._dims
        if self._batch_output is None:
            self._batch_output = torch.zeros((self._max_batch, d.H, d.W), dtype=torch.float32,
                                             device=torch.device("cuda", self._device))
        if engine_streams and 2 * n <= self._max_batch:
            first = self._out_parity * (self._max_batch // 2)
            self._out_parity ^= 1
            return self._batch_output[first:first + n]
        return self._batch_output[:n]

    # ------------------------------------------------------------------ reference surface
    def compute_disparity_map(self, left_image: torch.Tensor, right_image: torch.Tensor) -> torch.Tensor:
        """stereo_matching.cc:22-43: [3,H,W] float32 CUDA tensors -> [H,W] float32 disparity
        (full-resolution pixels).  Returns the engine's persistent output tensor."""
        d = self._dims
        if isinstance(left_image, torch.Tensor) and left_image.dtype == torch.uint8:
            # addition: uint8 [3,H,W] straight from the image decoder; the cast is fused on the device
            self._validate("left_image", left_image, (3, d.H, d.W), torch.uint8)
            self._validate("right_image", right_image, (3, d.H, d.W), torch.uint8)
            check(LIB.smx_compute_rgb_u8(self._handle, left_image.data_ptr(), right_image.data_ptr(),
                                         self._output.data_ptr(), self._stream()))
            return self._output
        self._validate("left_image", left_image, (3, d.H, d.W))
        self._validate("right_image", right_image, (3, d.H, d.W))
        check(LIB.smx_compute_rgb(self._handle, left_image.data_ptr(), right_image.data_ptr(),
                                  self._output.data_ptr(), self._stream()))
        return self._output

    # ------------------------------------------------------------------ additions
    def compute_disparity_map_gray(self, left: torch.Tensor, right: torch.Tensor) -> torch.Tensor:
        """Grayscale entry ([H,W] float32 or uint8): skips reference step 1."""
        d = self._dims
        dtype = left.dtype if isinstance(left, torch.Tensor) and left.dtype == torch.uint8 else torch.float32
        self._validate("left_image", left, (d.H, d.W), dtype)
        self._validate("right_image", right, (d.H, d.W), dtype)
        fn = LIB.smx_compute_gray_u8 if dtype == torch.uint8 else LIB.smx_compute_gray
        check(fn(self._handle, left.data_ptr(), right.data_ptr(), self._output.data_ptr(), self._stream()))
        return self._output

    def compute_disparity_map_batch(self, left: torch.Tensor, right: torch.Tensor,
                                    out: Optional[torch.Tensor] = None, *, engine_streams: bool = False) -> torch.Tensor:
        """n independent pairs in one set of launches: [n,H,W] gray or [n,3,H,W] RGB, float32 or uint8.

        engine_streams=True submits on the engine's own streams (SMX_STREAM_ENGINE): the inputs must be
        complete (not merely enqueued) and `out` is defined only after join(); consecutive calls pipeline."""
        d = self._dims
        if not isinstance(left, torch.Tensor) or left.dim() not in (3, 4):
            raise RuntimeError("left_image must be [n,H,W] or [n,3,H,W]")
        n = int(left.shape[0])
        if not (1 <= n <= self._max_batch):
            raise RuntimeError(f"batch size {n} outside [1, max_batch={self._max_batch}]")
        gray = left.dim() == 3
        shape = (n, d.H, d.W) if gray else (n, 3, d.H, d.W)
        dtype = torch.uint8 if left.dtype == torch.uint8 else torch.float32
        self._validate("left_image", left, shape, dtype)
        self._validate("right_image", right, shape, dtype)
        if out is None:
            out = self._batch_out(n, engine_streams)
        else:
            self._validate("out", out, (n, d.H, d.W))
        if dtype == torch.uint8:
            fn = LIB.smx_compute_gray_u8_batch if gray else LIB.smx_compute_rgb_u8_batch
        else:
            fn = LIB.smx_compute_gray_batch if gray else LIB.smx_compute_rgb_batch
        check(fn(self._handle, n, left.data_ptr(), right.data_ptr(), out.data_ptr(),
                 _native.STREAM_ENGINE if engine_streams else self._stream()))
        return out

    def compute_disparity_map_batch_lr(self, left: torch.Tensor, right: torch.Tensor,
                                       out: Optional[torch.Tensor] = None, *, right_out: Optional[torch.Tensor] = None,
                                       max_diff: float = 1.0, invalid_disparity: float = -1.0) -> torch.Tensor:
        """Left-right checked disparity maps (smx_compute_lr_*_batch): same inputs as compute_disparity_map_batch, at most
        max_batch // 2 pairs (the right-view maps are computed in the same call, as n more pairs).  Pixels whose match
        in the right image does not point back to them within max_diff pixels become invalid_disparity.  right_out
        ([n,H,W] float32) receives the un-checked right-view maps.  The default `out` is a buffer of its own (valid
        until the next LR call), not the one of the plain batch method."""
        d = self._dims
        if not isinstance(left, torch.Tensor) or left.dim() not in (3, 4):
            raise RuntimeError("left_image must be [n,H,W] or [n,3,H,W]")
        n = int(left.shape[0])
        if not (1 <= n <= self._max_batch // 2):
            raise RuntimeError(f"LR batch size {n} outside [1, max_batch // 2 = {self._max_batch // 2}]: the right-view "
                               f"maps double the pairs of the call (create the engine with max_batch >= {2 * n})")
        gray = left.dim() == 3
        shape = (n, d.H, d.W) if gray else (n, 3, d.H, d.W)
        dtype = torch.uint8 if left.dtype == torch.uint8 else torch.float32
        self._validate("left_image", left, shape, dtype)
        self._validate("right_image", right, shape, dtype)
        _check_lr_scalars(max_diff, invalid_disparity)
        if out is None:
            if self._lr_output is None:
                self._lr_output = torch.zeros((self._max_batch // 2, d.H, d.W), dtype=torch.float32,
                                              device=torch.device("cuda", self._device))
            out = self._lr_output[:n]
        else:
            self._validate("out", out, (n, d.H, d.W))
        if right_out is not None:
            self._validate("right_out", right_out, (n, d.H, d.W))
        if dtype == torch.uint8:
            fn = LIB.smx_compute_lr_gray_u8_batch if gray else LIB.smx_compute_lr_rgb_u8_batch
        else:
            fn = LIB.smx_compute_lr_gray_batch if gray else LIB.smx_compute_lr_rgb_batch
        check(fn(self._handle, n, left.data_ptr(), right.data_ptr(), out.data_ptr(),
                 right_out.data_ptr() if right_out is not None else None, float(max_diff), float(invalid_disparity),
                 self._stream()))
        return out

    def join(self) -> None:
        """Orders the current stream behind every engine_streams=True call made so far (smx_join)."""
        check(LIB.smx_join(self._handle, self._stream()))

    def intermediate(self, stage: int, pair_index: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Copy of an intermediate of the last call (parity tests), on the current stream.  out: an existing
        contiguous buffer of the stage's size and dtype to copy into (e.g. a persistent guide image)."""
        d = self._dims
        nbytes = int(LIB.smx_stage_bytes(self._handle, stage))
        if nbytes == 0:
            raise RuntimeError(f"stage {stage} is not available for this configuration")
        dtype = torch.int32 if stage == _native.STAGE_GRID_FLAG else torch.float32
        if out is None:
            buf = torch.empty(nbytes // 4, dtype=dtype, device=torch.device("cuda", self._device))
        else:
            _check_input("out", out)
            if out.dtype != dtype or out.numel() * 4 != nbytes or out.device != torch.device("cuda", self._device):
                raise RuntimeError(f"out must be {dtype} of {nbytes // 4} elements on cuda:{self._device}")
            buf = out.view(-1)
        check(LIB.smx_get_intermediate(self._handle, stage, pair_index, buf.data_ptr(), nbytes, self._stream()))
        shapes = {
            _native.STAGE_GRAY_LEFT: (d.H, d.W), _native.STAGE_GRAY_RIGHT: (d.H, d.W),
            _native.STAGE_DOWN_LEFT: (d.h, d.w), _native.STAGE_DOWN_RIGHT: (d.h, d.w),
            _native.STAGE_WTA: (d.h, d.w), _native.STAGE_REFINED: (d.h, d.w),
            _native.STAGE_MBM_COSTS: (3, d.h, d.w), _native.STAGE_AGG_VOLUME: (d.h, d.w, d.Dd),
            _native.STAGE_GRID_FLAG: (1,),
        }
        return buf.view(shapes[stage])

    def profile_begin(self, max_calls: int) -> None:
        """Bracket every kernel of the next `max_calls` calls with HIP events on the current stream."""
        check(LIB.smx_profile_begin(self._handle, int(max_calls)))

    def profile_end(self) -> dict:
        """{kernel: (mean milliseconds per launch, launches)}; synchronises the recorded events."""
        ms = (C.c_float * len(_native.KERNEL_SLOTS))()
        cnt = (C.c_int * len(_native.KERNEL_SLOTS))()
        check(LIB.smx_profile_end(self._handle, ms, cnt))
        return {k: (float(ms[i]), int(cnt[i])) for i, k in enumerate(_native.KERNEL_SLOTS)}

    def match_geometry(self, n: int = 1) -> dict:
        """How the FAST_GRID aggregation kernel tiles a call of n pairs (smx_get_match_geometry)."""
        g = _native.SmxMatchGeometry()
        check(LIB.smx_get_match_geometry(self._handle, int(n), C.byref(g)))
        return {"kernel": _native.MATCH_KERNELS[g.kernel], "band_rows": g.band_rows, "rows_marched": g.rows_marched,
                "waves_per_workgroup": g.waves_per_workgroup, "workgroups": g.workgroups,
                "columns_per_wave": g.columns_per_wave, "useful_fraction": g.useful_fraction}

    def overlap_lanes(self, n: int) -> int:
        """Stream lanes (1 or 2) a batch call with n pairs runs on (smx_overlap_lanes)."""
        k = LIB.smx_overlap_lanes(self._handle, int(n))
        if k < 1:
            raise ValueError("smx_overlap_lanes: bad argument")
        return k

    def route_info(self) -> dict:
        """Launch-plan state that follows the content of earlier calls (smx_get_route_info)."""
        r = _native.SmxRouteInfo()
        check(LIB.smx_get_route_info(self._handle, C.byref(r)))
        return {k: getattr(r, k) for k, _ in r._fields_ if k != "reserved"}

    def last_match_mode(self) -> str:
        code = LIB.smx_last_match_mode(self._handle)
        return {v: k for k, v in _native.MATCH_MODES.items()}[code]


# ---- metric 3D point clouds ----------------------------------------------------------------------------------------------

@dataclasses.dataclass
class PointCloud:
    """One map's point cloud; a field is None where it does not apply.  points: [N, 3] float32 (X, Y, Z in the units of
    the reprojection matrix's baseline); colors: [N, 3] uint8 RGB (with an image); indices: [N] int32, the row-major pixel
    index y * W + x of each point (reproject_to_3d); counts: [N] int32, the points per voxel (voxel_downsample);
    xyz_map: [H, W, 3] float32, the organised cloud with NaN at the excluded pixels (reproject_to_3d(organized=True));
    normals: [N, 3] float32 unit normals (TSDFVolume.extract_point_cloud(normals=True))."""
    points: torch.Tensor
    colors: Optional[torch.Tensor] = None
    indices: Optional[torch.Tensor] = None
    counts: Optional[torch.Tensor] = None
    xyz_map: Optional[torch.Tensor] = None
    normals: Optional[torch.Tensor] = None


@dataclasses.dataclass
class TriangleMesh:
    """An indexed triangle mesh (TSDFVolume.extract_triangle_mesh).  vertices: [N, 3] float32; triangles: [M, 3] int32
    indices into the vertices, counter-clockwise seen from outside (from the cameras' side); normals: [N, 3] float32 unit
    vertex normals or None; colors: [N, 3] uint8 RGB or None.  Vertices that no triangle refers to are kept."""
    vertices: torch.Tensor
    triangles: torch.Tensor
    normals: Optional[torch.Tensor] = None
    colors: Optional[torch.Tensor] = None


@dataclasses.dataclass
class RenderedView:
    """What a TSDFVolume looks like from a camera (TSDFVolume.render): planes [H, W] for one pose [4, 4], [n, H, W] for
    poses [n, 4, 4].  disparity: float32, in the convention of every disparity map of this library, invalid_disparity
    where the ray hits no surface; depth: float32 camera depth of the hit, NaN without one; normals: [3, H, W] /
    [n, 3, H, W] float32 unit normals in the world frame, toward the cameras that measured the surface, 0 without a hit
    (None with normals=False); colors: [3, H, W] / [n, 3, H, W] uint8 RGB, 0 without a hit (None with colors=False or
    without a colour volume); weight: float32, the fusion weight of the voxel nearest to the hit, 0 without one."""
    disparity: torch.Tensor
    depth: torch.Tensor
    normals: Optional[torch.Tensor] = None
    colors: Optional[torch.Tensor] = None
    weight: Optional[torch.Tensor] = None


@dataclasses.dataclass
class TrackingResult:
    """What track_camera found, as device tensors (nothing is synchronised; one frame gives the shapes on the left, a
    batch of n the ones on the right).  pose: float32 [4, 4] / [n, 4, 4] camera-to-world, the initial pose's bits where
    lost; lost: bool [] / [n]; iterations, inliers, accepted: int32 [] / [n] -- the iterations that ran, and the inliers
    and the selected accepted pixels of the last one; rms: float32 [] / [n], the weighted point-to-plane residual of
    the last iteration (NaN if none ran); information: float64 [6, 6] / [n, 6, 6], the normal matrix of the last
    iteration over the twist (rotation, translation) in the world frame, which serves as the inverse covariance of the
    pose up to the residual's variance; normal_equations: float64 [30] / [n, 30], the sums it is made of.  With the
    photometric term (track_camera(image=...)): normal_equations has the joint system's thirty sums and then the three
    photometric ones ([33] / [n, 33]), information is the joint matrix, photometric_inliers: int32 [] / [n], the inliers
    that had a photometric term in the last iteration, and photometric_rms: float32 [] / [n], their weighted intensity
    residual (NaN without one); both are None without the term."""
    pose: torch.Tensor
    lost: torch.Tensor
    iterations: torch.Tensor
    inliers: torch.Tensor
    accepted: torch.Tensor
    rms: torch.Tensor
    information: torch.Tensor
    normal_equations: torch.Tensor
    photometric_inliers: Optional[torch.Tensor] = None
    photometric_rms: Optional[torch.Tensor] = None


def reprojection_matrix(fx: float, cx: float, cy: float, baseline: float, *, fy: Optional[float] = None,
                        cx_right: Optional[float] = None) -> np.ndarray:
    """The float32 4x4 Q of a rectified pair in OpenCV's reprojectImageTo3D convention, [X' Y' Z' W'] = Q [u v d 1]:
        [[1, 0,     0,     -cx        ],
         [0, fx/fy, 0,     -cy fx/fy  ],
         [0, 0,     0,      fx        ],
         [0, 0,     1/B,   (cx_right - cx)/B]]
    so Z = fx B / (d + cx_right - cx), X = (u - cx) Z / fx, Y = (v - cy) Z / fy.  fy defaults to fx, cx_right (the right
    camera's principal point) to cx; with Middlebury's doffs, cx_right = cx + doffs.  Units follow the baseline's.
    Computed in float64, rounded once to float32."""
    fy = fx if fy is None else fy
    cx_right = cx if cx_right is None else cx_right
    for name, v in (("fx", fx), ("fy", fy), ("cx", cx), ("cy", cy), ("baseline", baseline), ("cx_right", cx_right)):
        _number_arg(name, v)
        if not math.isfinite(v):
            raise RuntimeError(f"{name} must be finite, got {v}")
    if fx <= 0 or fy <= 0:
        raise RuntimeError(f"fx and fy must be > 0, got {fx}, {fy}")
    if baseline == 0:
        raise RuntimeError("baseline must not be 0")
    fx, fy, cx, cy, b, cxr = (float(v) for v in (fx, fy, cx, cy, baseline, cx_right))
    q = np.array([[1.0, 0.0, 0.0, -cx],
                  [0.0, fx / fy, 0.0, -cy * fx / fy],
                  [0.0, 0.0, 0.0, fx],
                  [0.0, 0.0, 1.0 / b, (cxr - cx) / b]], dtype=np.float64)
    return q.astype(np.float32)


def _check_q(Q) -> np.ndarray:
    q = np.asarray(Q.detach().cpu() if isinstance(Q, torch.Tensor) else Q)
    if q.shape != (4, 4) or not np.issubdtype(q.dtype, np.number):
        raise RuntimeError(f"Q must be a numeric 4x4 matrix, got shape {q.shape}")
    q = np.ascontiguousarray(q, dtype=np.float32)
    if not np.isfinite(q).all():
        raise RuntimeError("Q must be finite (in float32)")
    return q


def _check_reproject_params(min_confidence, depth_range, invalid_disparity) -> Tuple[float, float]:
    _number_arg("min_confidence", min_confidence)
    if not math.isfinite(min_confidence):
        raise RuntimeError(f"min_confidence must be finite, got {min_confidence}")
    _number_arg("invalid_disparity", invalid_disparity)
    if not math.isfinite(invalid_disparity):
        raise RuntimeError(f"invalid_disparity must be finite (a NaN marker never compares equal), got {invalid_disparity}")
    try:
        z_min, z_max = depth_range
    except (TypeError, ValueError):
        raise TypeError("depth_range must be a pair (z_min, z_max)") from None
    _number_arg("depth_range[0]", z_min)
    _number_arg("depth_range[1]", z_max)
    if math.isnan(z_min) or math.isnan(z_max) or z_min > z_max:
        raise RuntimeError(f"depth_range must satisfy z_min <= z_max, got {depth_range}")
    return float(z_min), float(z_max)


def _check_colour_image(image: torch.Tensor, n: int, H: int, W: int, batched: bool, device) -> int:
    """The number of channels (1 or 3) of a colour source for n maps of H x W."""
    _check_input("image", image)
    if image.dtype not in (torch.uint8, torch.float32):
        raise RuntimeError(f"image must be uint8 or float32, got {image.dtype}")
    if image.device != device:
        raise RuntimeError(f"image must be on {device}, got {image.device}")
    lead = (n,) if batched else ()
    shape = tuple(image.shape)
    for ch, want in ((1, lead + (H, W)), (1, lead + (1, H, W)), (3, lead + (3, H, W))):
        if shape == want:
            return ch
    raise RuntimeError(f"image must be {lead + (H, W)}, {lead + (1, H, W)} or {lead + (3, H, W)}, got {shape}")


def reproject_to_3d_batched(disp: torch.Tensor, Q, *, image: Optional[torch.Tensor] = None,
                            confidence: Optional[torch.Tensor] = None, min_confidence: float = 0.0,
                            depth_range=(0.0, math.inf), invalid_disparity: float = -1.0, organized: bool = False,
                            indices: bool = True):
    """reproject_to_3d of n maps [n, H, W] without synchronising (smx_reproject_points, on the current stream): returns
    (points [n H W, 3] f32, colors [n H W, 3] u8 or None, indices [n H W] int32 or None, offsets [n + 1] int32,
    xyz_map [n, H, W, 3] f32 or None), fresh tensors padded to the capacity n H W; the points of map i are rows
    offsets[i]..offsets[i+1] (device values) in row-major pixel order.  image: [n, H, W], [n, 1, H, W] (gray) or
    [n, 3, H, W] (RGB), uint8 or float32."""
    q = _check_q(Q)
    z_min, z_max = _check_reproject_params(min_confidence, depth_range, invalid_disparity)
    _check_input("disp", disp)
    if disp.dtype != torch.float32 or disp.dim() != 3:
        raise RuntimeError(f"disp must be float32 [n, H, W], got {disp.dtype} {tuple(disp.shape)}")
    n, H, W = disp.shape
    if not (n >= 1 and 1 <= H <= 32768 and 1 <= W <= 32768 and n * H * W <= 2 ** 30):
        raise RuntimeError(f"need n >= 1, 1 <= H, W <= 32768 and n * H * W <= 2^30, got {tuple(disp.shape)}")
    if confidence is not None:
        _check_like("confidence", confidence, torch.float32, disp.shape, disp.device)
    channels = 0 if image is None else _check_colour_image(image, n, H, W, True, disp.device)
    dev, cap = disp.device, n * H * W
    points = torch.empty((cap, 3), dtype=torch.float32, device=dev)
    colors = None if image is None else torch.empty((cap, 3), dtype=torch.uint8, device=dev)
    idx = torch.empty(cap, dtype=torch.int32, device=dev) if indices else None
    xyz = torch.empty((n, H, W, 3), dtype=torch.float32, device=dev) if organized else None
    offsets = torch.empty(n + 1, dtype=torch.int32, device=dev)
    ws_bytes = LIB.smx_reproject_workspace_bytes(n, H, W)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    qc = (C.c_float * 16)(*q.reshape(-1).tolist())
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    dtype = _native.DTYPE_F32 if image is not None and image.dtype == torch.float32 else _native.DTYPE_U8
    check(LIB.smx_reproject_points(dev.index, n, H, W, disp.data_ptr(), qc, ptr(confidence), float(min_confidence),
                                   z_min, z_max, float(invalid_disparity), ptr(image), channels, dtype,
                                   points.data_ptr(), ptr(colors), ptr(idx), ptr(xyz), offsets.data_ptr(),
                                   ws.data_ptr(), ws_bytes, _stream(dev.index)))
    return points, colors, idx, offsets, xyz


def reproject_to_3d(disp: torch.Tensor, Q, *, image: Optional[torch.Tensor] = None,
                    confidence: Optional[torch.Tensor] = None, min_confidence: float = 0.0,
                    depth_range=(0.0, math.inf), invalid_disparity: float = -1.0, organized: bool = False):
    """Metric 3D points of a disparity map [H, W] (-> PointCloud) or of n maps [n, H, W] (-> a list of n PointClouds),
    float32 on one GPU (smx_reproject_points; the rule is in include/stereo_mi355x.h).  Q: the 4x4 reprojection matrix
    (reprojection_matrix(), helpers.kitti_calibration.reprojection_matrix, MiddleBuryStereoCameraCalibration.
    reprojection_matrix()).  A pixel becomes a point where its disparity is finite and != invalid_disparity, W' > 0, the
    point is finite, depth_range[0] <= Z <= depth_range[1] and, with a confidence map, confidence >= min_confidence.
    image: the colour source, [H, W] / [1, H, W] (gray) or [3, H, W] (RGB) per map ([n, ...] for n maps), uint8 or float32
    (rounded and clamped to 0..255).  The points keep row-major pixel order; PointCloud.indices holds their pixel indices;
    organized=True adds PointCloud.xyz_map.  Runs on the current stream and SYNCHRONISES ONCE, to read the point counts;
    reproject_to_3d_batched is the asynchronous form.  Returns new tensors."""
    single = isinstance(disp, torch.Tensor) and disp.dim() == 2
    if isinstance(disp, torch.Tensor) and disp.dim() not in (2, 3):
        raise RuntimeError(f"disp must be [H, W] or [n, H, W], got {tuple(disp.shape)}")
    if single:
        _check_input("disp", disp)
        H, W = disp.shape
        if image is not None:
            _check_colour_image(image, 1, H, W, False, disp.device)
            image = image.unsqueeze(0)
        if confidence is not None:
            _check_like("confidence", confidence, torch.float32, disp.shape, disp.device)
            confidence = confidence.unsqueeze(0)
        disp = disp.unsqueeze(0)
    points, colors, idx, offsets, xyz = reproject_to_3d_batched(
        disp, Q, image=image, confidence=confidence, min_confidence=min_confidence, depth_range=depth_range,
        invalid_disparity=invalid_disparity, organized=organized)
    off = offsets.cpu().tolist()                                   # the one synchronisation
    clouds = [PointCloud(points=points[a:b], colors=None if colors is None else colors[a:b], indices=idx[a:b],
                         xyz_map=None if xyz is None else xyz[i])
              for i, (a, b) in enumerate(zip(off[:-1], off[1:]))]
    return clouds[0] if single else clouds


def _check_voxel_params(voxel_size, min_points) -> None:
    _number_arg("voxel_size", voxel_size)
    if not (math.isfinite(voxel_size) and voxel_size > 0):
        raise RuntimeError(f"voxel_size must be finite and > 0, got {voxel_size}")
    _int_arg("min_points", min_points)
    if min_points < 1:
        raise RuntimeError(f"min_points must be >= 1, got {min_points}")


def voxel_downsample_batched(points: torch.Tensor, offsets: torch.Tensor, voxel_size: float, *,
                             colors: Optional[torch.Tensor] = None, min_points: int = 1):
    """voxel_downsample of a compacted batch without synchronising (smx_voxel_downsample, on the current stream).
    points: [cap, 3] float32, colors: [cap, 3] uint8 or None, offsets: [n + 1] int32 on the same device (the points of
    map i are rows offsets[i]..offsets[i+1]), e.g. reproject_to_3d_batched's.  Returns (points [cap, 3], colors or None,
    counts [cap] int32, offsets [n + 1] int32, dropped [n] int32), fresh tensors padded to cap: map i's voxels are rows
    offsets[i]..offsets[i+1] in ascending voxel-index order; dropped[i] counts its points outside the index range or in
    voxels below min_points."""
    _check_voxel_params(voxel_size, min_points)
    _check_input("points", points)
    if points.dtype != torch.float32 or points.dim() != 2 or points.shape[1] != 3 or points.shape[0] < 1:
        raise RuntimeError(f"points must be float32 [cap >= 1, 3], got {points.dtype} {tuple(points.shape)}")
    cap, dev = points.shape[0], points.device
    if cap > 2 ** 30:
        raise RuntimeError(f"at most 2^30 points, got {cap}")
    _check_input("offsets", offsets)
    if offsets.dtype != torch.int32 or offsets.dim() != 1 or not 2 <= offsets.shape[0] <= 65537 or offsets.device != dev:
        raise RuntimeError(f"offsets must be int32 [n + 1] with 1 <= n <= 65536 on {dev}")
    if colors is not None:
        _check_like("colors", colors, torch.uint8, (cap, 3), dev)
    n = offsets.shape[0] - 1
    out_points = torch.empty((cap, 3), dtype=torch.float32, device=dev)
    out_colors = None if colors is None else torch.empty((cap, 3), dtype=torch.uint8, device=dev)
    counts = torch.empty(cap, dtype=torch.int32, device=dev)
    out_offsets = torch.empty(n + 1, dtype=torch.int32, device=dev)
    dropped = torch.empty(n, dtype=torch.int32, device=dev)
    ws_bytes = LIB.smx_voxel_workspace_bytes(n, cap)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    check(LIB.smx_voxel_downsample(dev.index, n, cap, points.data_ptr(), None if colors is None else colors.data_ptr(),
                                   offsets.data_ptr(), float(voxel_size), int(min_points), out_points.data_ptr(),
                                   None if out_colors is None else out_colors.data_ptr(), counts.data_ptr(),
                                   out_offsets.data_ptr(), dropped.data_ptr(), ws.data_ptr(), ws_bytes,
                                   _stream(dev.index)))
    return out_points, out_colors, counts, out_offsets, dropped


def voxel_downsample(cloud_or_list, voxel_size: float, *, min_points: int = 1):
    """One point per occupied voxel of a PointCloud (-> PointCloud) or of each cloud of a list (-> a list), on the
    current stream (smx_voxel_downsample; the rule is in include/stereo_mi355x.h): the centroid of the voxel's points,
    their mean colour (when every cloud has colours) and their number (PointCloud.counts), in ascending voxel-index
    order; the voxel index is floor(coord / voxel_size) per axis.  Voxels with fewer than min_points points are dropped,
    as are points whose index lies outside -2^20..2^20-1.  Deterministic: the same bits on every run and for a cloud
    alone or in a list.  SYNCHRONISES ONCE, to read the voxel counts; voxel_downsample_batched is the asynchronous form."""
    _check_voxel_params(voxel_size, min_points)
    single = isinstance(cloud_or_list, PointCloud)
    clouds = [cloud_or_list] if single else list(cloud_or_list)
    if not clouds or not all(isinstance(c, PointCloud) for c in clouds):
        raise TypeError("voxel_downsample takes a PointCloud or a non-empty list of PointClouds")
    dev = clouds[0].points.device
    for c in clouds:
        _check_input("points", c.points)
        if c.points.dtype != torch.float32 or c.points.dim() != 2 or c.points.shape[1] != 3 or c.points.device != dev:
            raise RuntimeError(f"every cloud's points must be float32 [N, 3] on {dev}")
    with_colors = all(c.colors is not None for c in clouds)
    sizes = [c.points.shape[0] for c in clouds]
    total = sum(sizes)
    pad = 1 if total == 0 else 0                                   # the device call needs room for one point
    points = torch.cat([c.points for c in clouds] + [torch.zeros((pad, 3), dtype=torch.float32, device=dev)])
    colors = None
    if with_colors:
        for c in clouds:
            _check_like("colors", c.colors, torch.uint8, (c.points.shape[0], 3), dev)
        colors = torch.cat([c.colors for c in clouds] + [torch.zeros((pad, 3), dtype=torch.uint8, device=dev)])
    offsets = torch.tensor(np.cumsum([0] + sizes), dtype=torch.int32).to(dev)
    out_points, out_colors, counts, out_offsets, _ = voxel_downsample_batched(points, offsets, voxel_size,
                                                                              colors=colors, min_points=min_points)
    off = out_offsets.cpu().tolist()                               # the one synchronisation
    result = [PointCloud(points=out_points[a:b], colors=None if out_colors is None else out_colors[a:b],
                         counts=counts[a:b]) for a, b in zip(off[:-1], off[1:])]
    return result[0] if single else result


# ---- TSDF fusion ---------------------------------------------------------------------------------------------------------

def _host_matrices(name: str, a, lead_ok: bool) -> np.ndarray:
    """A numeric [4, 4] or [n, 4, 4] array (numpy or tensor) as float64 [n, 4, 4]."""
    m = np.asarray(a.detach().cpu() if isinstance(a, torch.Tensor) else a)
    if not np.issubdtype(m.dtype, np.number):
        raise RuntimeError(f"{name} must be numeric")
    if m.shape == (4, 4):
        m = m[None]
    if m.ndim != 3 or m.shape[1:] != (4, 4) or m.shape[0] < 1 or (m.shape[0] > 1 and not lead_ok):
        raise RuntimeError(f"{name} must be [4, 4] or [n, 4, 4], got shape {m.shape}")
    return m.astype(np.float64)


def projection_matrix(Q) -> np.ndarray:
    """P = inv(Q) of a reprojection matrix, computed in float64 and rounded once to float32: [u' v' d' w'] = P [X Y Z 1]
    projects a camera-frame point to its pixel (u'/w', v'/w') and disparity.  A singular Q raises RuntimeError."""
    q = _check_q(Q).astype(np.float64)
    try:
        p = np.linalg.inv(q)
    except np.linalg.LinAlgError:
        raise RuntimeError("Q is singular: it has no projection") from None
    p32 = p.astype(np.float32)
    if not np.isfinite(p32).all() or np.linalg.matrix_rank(q) < 4:
        raise RuntimeError("Q is singular: it has no projection")
    return p32


def world_to_camera_poses(camera_to_world) -> np.ndarray:
    """[n, 3, 4] float32: the top rows of inv(pose) of camera-to-world poses [4, 4] / [n, 4, 4], inverted in float64 and
    rounded once.  A pose that is not finite, is singular or whose last row is not [0, 0, 0, 1] raises RuntimeError."""
    m = _host_matrices("camera_to_world", camera_to_world, True)
    if not np.isfinite(m).all():
        raise RuntimeError("camera_to_world must be finite")
    if not np.array_equal(m[:, 3, :], np.broadcast_to(np.array([0.0, 0.0, 0.0, 1.0]), (m.shape[0], 4))):
        raise RuntimeError("camera_to_world's last row must be [0, 0, 0, 1]")
    if (np.linalg.matrix_rank(m[:, :3, :3]) < 3).any():
        raise RuntimeError("camera_to_world is singular")
    inv = np.linalg.inv(m).astype(np.float32)
    if not np.isfinite(inv).all():
        raise RuntimeError("camera_to_world is singular")
    return np.ascontiguousarray(inv[:, :3, :])


def camera_to_world_poses(camera_to_world) -> np.ndarray:
    """[n, 3, 4] float32: the top rows of camera-to-world poses [4, 4] / [n, 4, 4], rounded once from float64 and not
    inverted (what TSDFVolume.render hands to smx_tsdf_raycast).  A pose that is not finite or whose last row is not
    [0, 0, 0, 1] raises RuntimeError."""
    m = _host_matrices("camera_to_world", camera_to_world, True)
    if not np.isfinite(m).all():
        raise RuntimeError("camera_to_world must be finite")
    if not np.array_equal(m[:, 3, :], np.broadcast_to(np.array([0.0, 0.0, 0.0, 1.0]), (m.shape[0], 4))):
        raise RuntimeError("camera_to_world's last row must be [0, 0, 0, 1]")
    m32 = m[:, :3, :].astype(np.float32)
    if not np.isfinite(m32).all():
        raise RuntimeError("camera_to_world must be finite (in float32)")
    return np.ascontiguousarray(m32)


# ---- point clouds back into camera views ---------------------------------------------------------------------------------

@dataclasses.dataclass
class ProjectedView:
    """A point cloud seen from a camera (project_points): planes [H, W].  disparity: float32, in the convention of every
    disparity map of this library, invalid_disparity where no point lands; index: int32, the row of the cloud's point
    that won the pixel's depth test, -1 where none (None with index=False) -- gather any per-point attribute with it;
    depth: float32 camera depth of that point, NaN where none (None with depth=False); colors: [3, H, W] uint8 RGB
    gathered from the cloud's colours, 0 where nothing landed (None without them)."""
    disparity: torch.Tensor
    index: Optional[torch.Tensor] = None
    depth: Optional[torch.Tensor] = None
    colors: Optional[torch.Tensor] = None


def _check_p(P) -> np.ndarray:
    p = np.asarray(P.detach().cpu() if isinstance(P, torch.Tensor) else P)
    if p.shape != (4, 4) or not np.issubdtype(p.dtype, np.number):
        raise RuntimeError(f"P must be a numeric 4x4 matrix, got shape {p.shape}")
    p = np.ascontiguousarray(p, dtype=np.float32)
    if not np.isfinite(p).all():
        raise RuntimeError("P must be finite (in float32)")
    return p


def _check_world_to_camera(world_to_camera) -> np.ndarray:
    m = np.asarray(world_to_camera.detach().cpu() if isinstance(world_to_camera, torch.Tensor) else world_to_camera)
    if m.ndim != 3 or m.shape[1:] != (3, 4) or m.shape[0] < 1 or not np.issubdtype(m.dtype, np.number):
        raise RuntimeError(f"world_to_camera must be a numeric [n, 3, 4] array, got shape {m.shape}")
    m = np.ascontiguousarray(m, dtype=np.float32)
    if not np.isfinite(m).all():
        raise RuntimeError("world_to_camera must be finite (in float32)")
    return m


def project_points_batched(points: torch.Tensor, offsets: torch.Tensor, Q, camera_to_world, shape, *, P=None,
                           radius: int = 0, depth_range=(0.0, math.inf), invalid_disparity: float = -1.0,
                           index: bool = True, depth: bool = False, world_to_camera=None):
    """n point clouds into n camera views of shape (H, W) as z-buffered disparity maps, without synchronising
    (smx_project_points, on the current stream; the rule is in include/stereo_mi355x.h): the inverse of
    reproject_to_3d_batched.  points: [cap, 3] float32, offsets: [n + 1] int32 on the same device (cloud f is rows
    offsets[f]..offsets[f+1]), e.g. reproject_to_3d_batched's or voxel_downsample_batched's.  camera_to_world: [n, 4, 4]
    (numpy or tensor), inverted in float64 as TSDFVolume.integrate does; world_to_camera=[n, 3, 4] float32 gives the
    matrices applied to the points as they are instead (then camera_to_world must be None; a CUDA tensor is used in place,
    which is the form to capture into a graph).  Q: the views' reprojection matrix, whose inverse projection_matrix(Q)
    takes camera points to (column, row, disparity); P=, a 4x4 with [u' v' d' w'] = P [X Y Z 1], replaces it (exactly
    one of Q and P).  A point counts where its camera depth c_2 is > 0
    and within depth_range, its rounded pixel lies within `radius` (0..8) of the image and its disparity is finite and
    != invalid_disparity; it covers the (2 radius + 1)^2 pixels around its pixel.  Every pixel keeps its nearest point
    (the lowest row among equally near ones).  Returns fresh tensors (disparity [n, H, W] float32 with
    invalid_disparity where nothing lands, index [n, H, W] int32 row within the cloud or -1 (None with index=False),
    depth [n, H, W] float32 c_2 or NaN (None with depth=False)); the same bits on every run."""
    if (Q is None) == (P is None):
        raise RuntimeError("exactly one of Q and P must be given")
    p = projection_matrix(Q) if P is None else _check_p(P)
    z_min, z_max = _check_reproject_params(0.0, depth_range, invalid_disparity)
    _int_arg("radius", radius)
    if not 0 <= radius <= 8:
        raise RuntimeError(f"radius must be in 0..8, got {radius}")
    for name, v in (("index", index), ("depth", depth)):
        if not isinstance(v, bool):
            raise TypeError(f"{name} must be a bool")
    if (camera_to_world is None) == (world_to_camera is None):
        raise RuntimeError("exactly one of camera_to_world and world_to_camera must be given")
    on_device = isinstance(world_to_camera, torch.Tensor) and world_to_camera.is_cuda
    if on_device:                                                       # used as it is: nothing is copied or read here
        _check_input("world_to_camera", world_to_camera)
        if world_to_camera.dtype != torch.float32 or world_to_camera.dim() != 3 or tuple(world_to_camera.shape[1:]) != (3, 4):
            raise RuntimeError(f"a device world_to_camera must be float32 [n, 3, 4], got {world_to_camera.dtype} "
                               f"{tuple(world_to_camera.shape)}")
        w2c = world_to_camera
    elif world_to_camera is None:
        w2c = world_to_camera_poses(camera_to_world)
    else:
        w2c = _check_world_to_camera(world_to_camera)
    H, W = _shape2("shape", shape)
    _check_input("points", points)
    if points.dtype != torch.float32 or points.dim() != 2 or points.shape[1] != 3 or points.shape[0] < 1:
        raise RuntimeError(f"points must be float32 [cap >= 1, 3], got {points.dtype} {tuple(points.shape)}")
    cap, dev = points.shape[0], points.device
    if cap > 2 ** 30:
        raise RuntimeError(f"at most 2^30 points, got {cap}")
    _check_input("offsets", offsets)
    if offsets.dtype != torch.int32 or offsets.dim() != 1 or not 2 <= offsets.shape[0] <= 65537 or offsets.device != dev:
        raise RuntimeError(f"offsets must be int32 [n + 1] with 1 <= n <= 65536 on {dev}")
    n = offsets.shape[0] - 1
    if w2c.shape[0] != n:
        raise RuntimeError(f"{n} cloud(s) need {n} pose(s), got {w2c.shape[0]}")
    if n * H * W > 2 ** 30:
        raise RuntimeError(f"need n * H * W <= 2^30, got {n} views of {(H, W)}")
    if on_device and w2c.device != dev:
        raise RuntimeError(f"world_to_camera must be on {dev}, got {w2c.device}")
    poses = w2c if on_device else torch.from_numpy(w2c).pin_memory().to(dev, non_blocking=True)
    disp = torch.empty((n, H, W), dtype=torch.float32, device=dev)
    idx = torch.empty((n, H, W), dtype=torch.int32, device=dev) if index else None
    dep = torch.empty((n, H, W), dtype=torch.float32, device=dev) if depth else None
    ws_bytes = LIB.smx_project_workspace_bytes(n, H, W)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    pc = (C.c_float * 16)(*p.reshape(-1).tolist())
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    check(LIB.smx_project_points(dev.index, n, cap, H, W, points.data_ptr(), offsets.data_ptr(), poses.data_ptr(), pc,
                                 int(radius), z_min, z_max, float(invalid_disparity), disp.data_ptr(), ptr(idx), ptr(dep),
                                 ws.data_ptr(), ws_bytes, _stream(dev.index)))
    return disp, idx, dep


def project_points(cloud, Q, camera_to_world=None, shape=None, **kwargs) -> ProjectedView:
    """One PointCloud, or an [N, 3] float32 tensor of points, seen from camera_to_world [4, 4] (the identity by default)
    through a camera with the reprojection matrix Q, as maps of shape (H, W): project_points_batched of one cloud, with
    its keywords (P, radius, depth_range, invalid_disparity, index, depth).  Returns a ProjectedView; colors is the
    cloud's colours gathered through the index plane (which is then computed even with index=False, and not
    returned).  An empty cloud gives an empty view."""
    if shape is None:
        raise TypeError("project_points needs shape=(H, W)")
    points, colors = (cloud.points, cloud.colors) if isinstance(cloud, PointCloud) else (cloud, None)
    if not isinstance(points, torch.Tensor):
        raise TypeError("project_points takes a PointCloud or an [N, 3] tensor")
    _check_input("points", points)
    if points.dtype != torch.float32 or points.dim() != 2 or points.shape[1] != 3:
        raise RuntimeError(f"points must be float32 [N, 3], got {points.dtype} {tuple(points.shape)}")
    N, dev = points.shape[0], points.device
    if colors is not None:
        _check_like("colors", colors, torch.uint8, (N, 3), dev)
    if camera_to_world is None and kwargs.get("world_to_camera") is None:
        camera_to_world = np.eye(4)
    elif camera_to_world is not None and (camera_to_world.dim() if isinstance(camera_to_world, torch.Tensor)
                                          else np.ndim(camera_to_world)) != 2:
        raise RuntimeError("project_points takes one pose [4, 4]")
    want_index = kwargs.pop("index", True)
    if not isinstance(want_index, bool):
        raise TypeError("index must be a bool")
    offsets = torch.tensor([0, N], dtype=torch.int32).to(dev)
    if N == 0:                                                         # the device call needs room for one point
        points = torch.zeros((1, 3), dtype=torch.float32, device=dev)
    disp, idx, dep = project_points_batched(points, offsets, Q, camera_to_world, shape,
                                            index=want_index or colors is not None, **kwargs)
    view_colors = None
    if colors is not None:
        if N == 0:
            view_colors = torch.zeros((3,) + tuple(disp.shape[1:]), dtype=torch.uint8, device=dev)
        else:
            hit = idx[0] >= 0
            gathered = colors[idx[0].clamp(min=0).long()]                  # [H, W, 3]
            view_colors = (gathered * hit.unsqueeze(-1)).permute(2, 0, 1).contiguous()
    return ProjectedView(disparity=disp[0], index=idx[0] if want_index else None,
                         depth=None if dep is None else dep[0], colors=view_colors)


def _check_tsdf_volume(dims, voxel_size, origin) -> Tuple[Tuple[int, int, int], float, Tuple[float, float, float]]:
    try:
        nx, ny, nz = dims
    except (TypeError, ValueError):
        raise TypeError("dims must be (nx, ny, nz)") from None
    for name, v in (("nx", nx), ("ny", ny), ("nz", nz)):
        _int_arg(name, v)
        if not 1 <= v <= 4096:
            raise RuntimeError(f"{name} must be in 1..4096, got {v}")
    if nx * ny * nz > 2 ** 30:
        raise RuntimeError(f"at most 2^30 voxels, got {nx} * {ny} * {nz}")
    _number_arg("voxel_size", voxel_size)
    if not (math.isfinite(voxel_size) and voxel_size > 0):
        raise RuntimeError(f"voxel_size must be finite and > 0, got {voxel_size}")
    try:
        o = tuple(origin)
    except TypeError:
        raise TypeError("origin must be (x, y, z)") from None
    if len(o) != 3:
        raise TypeError("origin must be (x, y, z)")
    for v in o:
        _number_arg("origin", v)
        if not math.isfinite(v):
            raise RuntimeError(f"origin must be finite, got {o}")
    return (nx, ny, nz), float(voxel_size), tuple(float(v) for v in o)


DEFAULT_TRACKING_SCHEDULE = ((4, 4), (2, 5), (1, 10))
_INFORMATION_INDEX = {}                                            # device -> int64 [6, 6]: the sum that holds A[i][j]


def _check_tracking_schedule(schedule) -> np.ndarray:
    try:
        pairs = [(int(s), int(k)) for s, k in schedule]
        if any(s != s0 or k != k0 for (s, k), (s0, k0) in zip(pairs, schedule)):
            raise ValueError
    except (TypeError, ValueError):
        raise TypeError("schedule must be a sequence of (stride, iterations) pairs of integers") from None
    if len(pairs) > 8 or any(s < 1 or s > 32768 or k < 0 for s, k in pairs) or sum(k for _, k in pairs) > 64:
        raise RuntimeError("schedule: at most 8 pairs with 1 <= stride <= 32768 and iterations >= 0, 64 iterations in "
                           f"all, got {tuple(pairs)}")
    return np.ascontiguousarray(np.array(pairs, np.int32).reshape(-1, 2))


def track_camera(disp: torch.Tensor, Q, pose, model: RenderedView, model_pose, *, model_Q=None,
                 confidence: Optional[torch.Tensor] = None, schedule=DEFAULT_TRACKING_SCHEDULE,
                 max_distance: float = 0.3, depth_range=(0.0, math.inf), min_inliers: int = 100,
                 min_confidence: float = 0.0, invalid_disparity: float = -1.0, min_pivot: float = 1e-3,
                 rot_eps: float = 0.0, trans_eps: float = 0.0, image: Optional[torch.Tensor] = None,
                 photometric_weight: float = 0.0, max_intensity_difference: float = 30.0,
                 model_intensity: Optional[torch.Tensor] = None, pyramid_levels: Optional[int] = None,
                 huber_delta: float = math.inf, schedule_levels=None) -> TrackingResult:
    """The camera-to-world pose of a frame from its disparity map, by projective point-to-plane ICP against a rendered
    view of the model (smx_track_camera; the rule, operation by operation, is in include/stereo_mi355x.h).  disp: float32
    [H, W] or [n, H, W] with the reprojection matrix Q; pose: the initial guess [4, 4] / [n, 4, 4] (numpy or tensor;
    rounded once to float32); model: the RenderedView (with normals) that TSDFVolume.render made from model_pose [4, 4]
    / [n, 4, 4] with the reprojection matrix model_Q (default Q) -- one view per frame; it need not have the frame's
    shape.  A pixel of the frame takes part where TSDFVolume.integrate would use it (depth_range, invalid_disparity,
    confidence >= min_confidence and > 0, which is then its weight) and where the model pixel it projects to has a
    surface within max_distance of it.  schedule: (stride, iterations) pairs, coarse to fine: an iteration of stride s
    uses every s-th pixel of every s-th row.  A frame is LOST -- its pose comes back unchanged -- when an iteration has
    fewer than min_inliers inliers or its 6 x 6 system has a pivot <= min_pivot (a frame that sees one plane only);
    rot_eps / trans_eps (radians, metres) stop a frame early once an update is smaller than both.  Runs on the current
    stream without synchronising and returns a TrackingResult of fresh device tensors.  Rotations are composed in
    float32: over a long sequence they drift from orthogonality, which this function does not repair; nor does it close
    loops or relocalise a lost camera.
    image with photometric_weight > 0 adds a photometric term to the same system (smx_track_camera_photometric), so that
    texture holds what geometry leaves free -- a frame that sees one plane is then tracked, not lost.  image: the frame
    the map was computed on, uint8 [3, H, W] RGB or [H, W] gray ([n, 3, H, W] / [n, H, W] batched), or a float32
    intensity plane [H, W] / [n, H, W]; the model's intensity comes from model.colors (render with colors=True) or from
    model_intensity, float32 like model.depth.  photometric_weight: metres per intensity unit (0..255 from uint8), about
    0.001 to 0.03; a term whose intensities differ by more than max_intensity_difference is left out.  The term's basin
    is a few model pixels.  Without an image, or with a weight of 0, the geometric entry runs as it always did.
    pyramid_levels = L (1..8) widens that basin (smx_track_camera_pyramid): the term is read from Gaussian pyramids of
    the two planes (intensity_pyramid; the model's masked by model.depth), a schedule pair of stride s from level
    min(L - 1, number of trailing zero bits of s) or from schedule_levels' entry for the pair (2^level must divide s),
    so the coarse strides see coarse texture; huber_delta (intensity units, default inf: off) caps the pull of a large
    residual at that of one of huber_delta.  The geometric term still reads the full-resolution view at every stride,
    and neither exposure nor gain is compensated.  With pyramid_levels=None the call is what it was."""
    for name, v, positive in (("photometric_weight", photometric_weight, False),
                              ("max_intensity_difference", max_intensity_difference, True),
                              ("max_distance", max_distance, True), ("min_pivot", min_pivot, False),
                              ("rot_eps", rot_eps, False), ("trans_eps", trans_eps, False)):
        _number_arg(name, v)
        if not (math.isfinite(v) and (v > 0 if positive else v >= 0)):
            raise RuntimeError(f"{name} must be finite and {'> 0' if positive else '>= 0'}, got {v}")
    if image is None and photometric_weight > 0:
        raise RuntimeError("photometric_weight > 0 needs the frame's image")
    photometric = image is not None and photometric_weight > 0
    if pyramid_levels is None:
        if schedule_levels is not None or huber_delta != math.inf:
            raise RuntimeError("schedule_levels and huber_delta need pyramid_levels")
    else:
        if not isinstance(pyramid_levels, int) or isinstance(pyramid_levels, bool) or not 1 <= pyramid_levels <= 8:
            raise RuntimeError(f"pyramid_levels must be an int in 1..8, got {pyramid_levels!r}")
        _number_arg("huber_delta", huber_delta)
        if not huber_delta > 0:
            raise RuntimeError(f"huber_delta must be > 0 (inf: no robust weights), got {huber_delta}")
    pyramid = photometric and pyramid_levels is not None
    q = _check_q(Q)
    qm = q if model_Q is None else _check_q(model_Q)
    if (qm[:3, 2] != 0).any() or qm[3, 0] != 0 or qm[3, 1] != 0 or qm[3, 2] == 0:
        raise RuntimeError("model_Q's ray must not depend on the disparity (what reprojection_matrix builds)")
    pm = projection_matrix(qm)
    z_min, z_max = _check_reproject_params(min_confidence, depth_range, invalid_disparity)
    sched = _check_tracking_schedule(schedule)
    if pyramid_levels is not None:
        levels = _check_schedule_levels(sched, pyramid_levels, schedule_levels)
    if not isinstance(min_inliers, int) or isinstance(min_inliers, bool) or not 1 <= min_inliers <= 2 ** 30:
        raise RuntimeError(f"min_inliers must be an int in 1..2^30, got {min_inliers!r}")
    _check_input("disp", disp)
    if disp.dtype != torch.float32 or disp.dim() not in (2, 3) or not disp.is_cuda:
        raise RuntimeError(f"disp must be float32 [H, W] or [n, H, W] on the GPU, got {disp.dtype} {tuple(disp.shape)} "
                           f"on {disp.device}")
    dev = disp.device
    batched = disp.dim() == 3
    n, H, W = disp.shape if batched else (1,) + tuple(disp.shape)
    if not (n >= 1 and 1 <= H <= 32768 and 1 <= W <= 32768 and n * H * W <= 2 ** 30):
        raise RuntimeError(f"need n >= 1, 1 <= H, W <= 32768 and n * H * W <= 2^30, got {tuple(disp.shape)}")
    if -(-W // 64) * -(-H // 4) > 32768:
        raise RuntimeError(f"need ceil(W / 64) * ceil(H / 4) <= 32768, got a frame of {(H, W)}")
    if confidence is not None:
        _check_like("confidence", confidence, torch.float32, disp.shape, dev)
    if not isinstance(model, RenderedView):
        raise TypeError("model must be a RenderedView (TSDFVolume.render)")
    if model.normals is None:
        raise RuntimeError("model has no normals: render it with normals=True")
    lead = (n,) if batched else ()
    Hm, Wm = model.depth.shape[-2:]
    _check_like("model.depth", model.depth, torch.float32, lead + (Hm, Wm), dev)
    _check_like("model.normals", model.normals, torch.float32, lead + (3, Hm, Wm), dev)
    pose_in = camera_to_world_poses(pose)
    c2w = camera_to_world_poses(model_pose)
    w2c = world_to_camera_poses(model_pose)
    if pose_in.shape[0] != n or c2w.shape[0] != n:
        raise RuntimeError(f"{n} frame(s) need {n} pose(s) and {n} model pose(s), got {pose_in.shape[0]} and {c2w.shape[0]}")
    poses = torch.from_numpy(np.stack([pose_in, c2w, w2c])).pin_memory().to(dev, non_blocking=True)
    pose_out = torch.empty((n, 3, 4), dtype=torch.float32, device=dev)
    info = torch.empty((n, 4), dtype=torch.int32, device=dev)
    rms = torch.empty((n,), dtype=torch.float32, device=dev)
    f16 = lambda m: (C.c_float * 16)(*m.reshape(-1).tolist())  # noqa: E731
    sc = (C.c_int32 * max(sched.size, 1))(*sched.reshape(-1).tolist())
    # the arguments both entries take first; then the term's operands, if any; then the outputs and the workspace
    args = (dev.index, n, H, W, disp.data_ptr(), None if confidence is None else confidence.data_ptr(), f16(q),
            float(min_confidence), z_min, z_max, float(invalid_disparity), Hm, Wm, model.depth.data_ptr(),
            model.normals.data_ptr(), f16(qm), f16(pm), poses[1].data_ptr(), poses[2].data_ptr(), poses[0].data_ptr(),
            sched.shape[0], sc, float(max_distance), min_inliers, float(min_pivot), float(rot_eps), float(trans_eps))
    pinfo = prms = None
    if photometric:
        frame_int = _intensity_plane("image", image, lead, H, W, dev)
        if model_intensity is None:
            if model.colors is None:
                raise RuntimeError("the photometric term needs model.colors (render with colors=True) or model_intensity")
            model_intensity = model.colors
        model_int = _intensity_plane("model_intensity", model_intensity, lead, Hm, Wm, dev)
        pinfo = torch.empty((n, 2), dtype=torch.int32, device=dev)
        prms = torch.empty((n,), dtype=torch.float32, device=dev)
        query = LIB.smx_track_camera_photometric_workspace_bytes
        if pyramid:
            frame_pyr = _pyramid_buffer(frame_int.reshape(n, H, W), pyramid_levels, None)
            model_pyr = _pyramid_buffer(model_int.reshape(n, Hm, Wm), pyramid_levels, model.depth)
            lv = (C.c_int32 * max(levels.size, 1))(*levels.tolist())
            args += (frame_pyr.data_ptr(), model_pyr.data_ptr(), pyramid_levels, lv, float(photometric_weight),
                     float(max_intensity_difference), float(huber_delta))
            entry = LIB.smx_track_camera_pyramid
        else:
            args += (frame_int.data_ptr(), model_int.data_ptr(), float(photometric_weight),
                     float(max_intensity_difference))
            entry = LIB.smx_track_camera_photometric
    else:
        entry, query = LIB.smx_track_camera, LIB.smx_track_camera_workspace_bytes
    sums = torch.empty((n, 33 if photometric else 30), dtype=torch.float64, device=dev)
    ws_bytes = query(n, H, W)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    args += (pose_out.data_ptr(), info.data_ptr(), rms.data_ptr(), sums.data_ptr())
    if photometric:
        args += (pinfo.data_ptr(), prms.data_ptr())
    check(entry(*args, ws.data_ptr(), ws_bytes, _stream(dev.index)))
    index = _INFORMATION_INDEX.get(dev)
    if index is None:
        host = np.zeros((6, 6), np.int64)
        for k, (i, j) in enumerate((i, j) for i in range(6) for j in range(i, 6)):
            host[i, j] = host[j, i] = k
        index = _INFORMATION_INDEX[dev] = torch.from_numpy(host).to(dev)
    pose4 = torch.zeros((n, 4, 4), dtype=torch.float32, device=dev)
    pose4[:, :3] = pose_out
    pose4[:, 3, 3] = 1.0
    out = (pose4, info[:, 0] != 0, info[:, 1], info[:, 2], info[:, 3], rms, sums[:, index], sums)
    if photometric:
        out += (pinfo[:, 0], prms)
    if not batched:
        out = tuple(t[0] for t in out)
    return TrackingResult(*out)


def intensity_planes(image: torch.Tensor) -> torch.Tensor:
    """uint8 frames [n, C, H, W], C = 1 or 3 (RGB), on the GPU to float32 intensity planes [n, H, W]
    (smx_intensity_planes): (77 R + 150 G + 29 B) / 256, or the gray value itself.  Runs on the current stream."""
    _check_input("image", image)
    if image.dtype != torch.uint8 or image.dim() != 4 or image.shape[1] not in (1, 3) or not image.is_cuda:
        raise RuntimeError(f"image must be uint8 [n, 1 or 3, H, W] on the GPU, got {image.dtype} {tuple(image.shape)} "
                           f"on {image.device}")
    n, c, H, W = image.shape
    if not (n >= 1 and 1 <= H <= 32768 and 1 <= W <= 32768 and n * H * W <= 2 ** 30):
        raise RuntimeError(f"need n >= 1, 1 <= H, W <= 32768 and n * H * W <= 2^30, got {tuple(image.shape)}")
    out = torch.empty((n, H, W), dtype=torch.float32, device=image.device)
    check(LIB.smx_intensity_planes(image.device.index, n, c, H, W, image.data_ptr(), out.data_ptr(),
                                   _stream(image.device.index)))
    return out


def _check_schedule_levels(sched: np.ndarray, pyramid_levels: int, schedule_levels) -> np.ndarray:
    """int32 [pairs]: the pyramid level of every pair of the checked schedule; by default the coarsest level whose grid
    holds the pair's stride."""
    strides = [int(s) for s in sched[:, 0]]
    if schedule_levels is None:
        lv = [min(pyramid_levels - 1, (s & -s).bit_length() - 1) for s in strides]
    else:
        try:
            lv = [int(v) for v in schedule_levels]
            if any(v != v0 for v, v0 in zip(lv, schedule_levels)):
                raise ValueError
        except (TypeError, ValueError):
            raise TypeError("schedule_levels must be a sequence of integers, one per schedule pair") from None
        if len(lv) != len(strides):
            raise RuntimeError(f"schedule_levels needs one level per schedule pair ({len(strides)}), got {len(lv)}")
    for s, v in zip(strides, lv):
        if not 0 <= v < pyramid_levels or s % (1 << v):
            raise RuntimeError(f"a schedule level must be in 0..{pyramid_levels - 1} and 2^level must divide the stride, "
                               f"got level {v} at stride {s}")
    return np.array(lv, np.int32)


def _pyramid_dims(H: int, W: int, levels: int):
    dims = [(H, W)]
    for _ in range(levels - 1):
        dims.append(((dims[-1][0] + 1) // 2, (dims[-1][1] + 1) // 2))
    return dims


def _pyramid_buffer(planes: torch.Tensor, levels: int, mask_depth: Optional[torch.Tensor]) -> torch.Tensor:
    """The pyramid of checked float32 planes [n, H, W] as one flat buffer (smx_intensity_pyramid's layout)."""
    n, H, W = planes.shape
    out = torch.empty((sum(n * h * w for h, w in _pyramid_dims(H, W, levels)),), dtype=torch.float32, device=planes.device)
    check(LIB.smx_intensity_pyramid(planes.device.index, n, H, W, levels, planes.data_ptr(),
                                    None if mask_depth is None else mask_depth.data_ptr(), out.data_ptr(),
                                    _stream(planes.device.index)))
    return out


def intensity_pyramid(planes: torch.Tensor, levels: int, mask_depth: Optional[torch.Tensor] = None):
    """The Gaussian pyramid of float32 intensity planes [n, H, W] (or one plane [H, W]) on the GPU
    (smx_intensity_pyramid): a list of `levels` tensors [n, H_l, W_l] ([H_l, W_l]), H_l = ceil(H / 2^l), views of one
    buffer in the layout smx_track_camera_pyramid reads.  Level 0 is the plane, NaN where mask_depth (float32, the
    planes' shape) is not finite and > 0; a level halves the one before it with the taps (1 4 6 4 1) / 16, and a pixel
    with a NaN in its footprint is a NaN.  Runs on the current stream."""
    _check_input("planes", planes)
    if planes.dtype != torch.float32 or planes.dim() not in (2, 3) or not planes.is_cuda:
        raise RuntimeError(f"planes must be float32 [H, W] or [n, H, W] on the GPU, got {planes.dtype} "
                           f"{tuple(planes.shape)} on {planes.device}")
    if not isinstance(levels, int) or isinstance(levels, bool) or not 1 <= levels <= 8:
        raise RuntimeError(f"levels must be an int in 1..8, got {levels!r}")
    batched = planes.dim() == 3
    n, H, W = planes.shape if batched else (1,) + tuple(planes.shape)
    if not (n >= 1 and 1 <= H <= 32768 and 1 <= W <= 32768 and n * H * W <= 2 ** 30):
        raise RuntimeError(f"need n >= 1, 1 <= H, W <= 32768 and n * H * W <= 2^30, got {tuple(planes.shape)}")
    if mask_depth is not None:
        _check_like("mask_depth", mask_depth, torch.float32, planes.shape, planes.device)
    buf = _pyramid_buffer(planes.reshape(n, H, W), levels, mask_depth)
    out, at = [], 0
    for h, w in _pyramid_dims(H, W, levels):
        level = buf[at:at + n * h * w].view(n, h, w)
        out.append(level if batched else level[0])
        at += n * h * w
    return out


def _intensity_plane(name: str, image: torch.Tensor, lead: tuple, H: int, W: int, dev) -> torch.Tensor:
    """The float32 plane(s) lead + (H, W) of a frame given as uint8 RGB lead + (3, H, W), uint8 gray or float32 intensity
    lead + (H, W)."""
    if not isinstance(image, torch.Tensor) or image.device != dev:
        raise RuntimeError(f"{name} must be a tensor on {dev}")
    shape = tuple(image.shape)
    if image.dtype == torch.float32 and shape == lead + (H, W):
        _check_input(name, image)
        return image
    if image.dtype == torch.uint8 and shape in (lead + (3, H, W), lead + (H, W)):
        c = 3 if shape == lead + (3, H, W) else 1
        return intensity_planes(image.contiguous().reshape(-1, c, H, W)).reshape(lead + (H, W))
    raise RuntimeError(f"{name} must be uint8 {lead + (3, H, W)} or {lead + (H, W)}, or float32 {lead + (H, W)}, got "
                       f"{image.dtype} {shape}")


WINDOW_START_MAX = 8192                                            # smx_tsdf_window: |x0|, |y0|, |z0|


def _int_triple(name: str, v, limit: Optional[int] = None) -> Tuple[int, int, int]:
    try:
        t = tuple(v)
    except TypeError:
        raise TypeError(f"{name} must be three ints") from None
    if len(t) != 3:
        raise TypeError(f"{name} must be three ints")
    for c in t:
        _int_arg(name, c)
        if limit is not None and abs(c) > limit:
            raise RuntimeError(f"{name}: at most {limit} voxels per axis, got {t}")
    return tuple(int(c) for c in t)


def tsdf_window_origin(origin, offset, voxel_size: float) -> Tuple[float, float, float]:
    """The world position of the corner of a volume that was built at `origin` and has moved by `offset` whole voxels:
    origin + offset * voxel_size per axis, one float64 product and sum from the two values that are kept, so that a
    volume's origin does not drift however many shifts made up the offset."""
    return tuple(float(o) if k == 0 else float(o) + k * float(voxel_size) for o, k in zip(origin, offset))


def tsdf_spill_boxes(dims, voxels, margin: int = 1):
    """What TSDFVolume.shift(voxels, spill=True) hands back, as [(start, dims), ...] windows of the volume before the
    shift: one box per axis with a non-zero component, in the order x, y, z.  A box covers the volume's whole
    cross-section in the other two axes; along its own axis a, with n = dims[a] and d = voxels[a], it covers the layers
    that leave -- [0, d) for d > 0, [n + d, n) for d < 0 -- extended by `margin` layers into the staying side and clipped
    to [0, n)."""
    dims, d = _int_triple("dims", dims), _int_triple("voxels", voxels)
    _int_arg("margin", margin)
    if margin < 0:
        raise RuntimeError(f"margin must be >= 0, got {margin}")
    boxes = []
    for a in range(3):
        n = dims[a]
        if d[a] == 0:
            continue
        lo, hi = (0, min(n, d[a] + margin)) if d[a] > 0 else (max(0, n + d[a] - margin), n)
        start, size = [0, 0, 0], list(dims)
        start[a], size[a] = lo, hi - lo
        boxes.append((tuple(start), tuple(size)))
    return boxes


def tsdf_follow_shift(position, origin, dims, voxel_size: float, anchor=(0.5, 0.5, 0.5)) -> Tuple[int, int, int]:
    """The whole-voxel shift that brings a volume's anchor point, origin + anchor * dims * voxel_size, to `position`: per
    axis (position - anchor point) / voxel_size in float64, rounded half away from zero."""
    out = []
    for p, o, n, a in zip(position, origin, dims, anchor):
        x = (float(p) - (float(o) + float(a) * n * float(voxel_size))) / float(voxel_size)
        if not math.isfinite(x):
            raise RuntimeError(f"the camera position {tuple(position)} is not finite in voxels")
        whole = math.floor(abs(x))
        if abs(x) - whole >= 0.5:                                   # an exact difference: floor(abs(x) + 0.5) is not
            whole += 1
        out.append(int(whole) if x >= 0 else -int(whole))
    return tuple(out)


def tsdf_spill_ownership(dims, voxels):
    """Parallel to tsdf_spill_boxes(dims, voxels, margin): the sub-box (start, dims) of the volume before the shift that
    each box OWNS, or None for a box that owns nothing.  Only voxels that leave are owned (margin layers stay with the
    volume), and each by one box: the x box owns its leaving layers over the whole cross-section, the y box its leaving
    layers over the x range that stays, the z box its leaving layers over the x and y ranges that stay.  So the corner
    that boxes share has one owner, and the owned boxes together are exactly the voxels that leave."""
    dims, d = _int_triple("dims", dims), _int_triple("voxels", voxels)
    leaving, staying = [], []
    for n, c in zip(dims, d):
        if c > 0:
            leaving.append((0, min(n, c)))
            staying.append((min(n, c), n))
        elif c < 0:
            leaving.append((max(0, n + c), n))
            staying.append((0, max(0, n + c)))
        else:
            leaving.append(None)
            staying.append((0, n))
    owned = []
    for a in range(3):
        if leaving[a] is None:
            continue
        ranges = [staying[b] if b < a else leaving[b] if b == a else (0, dims[b]) for b in range(3)]
        if any(hi <= lo for lo, hi in ranges):
            owned.append(None)
        else:
            owned.append((tuple(lo for lo, _ in ranges), tuple(hi - lo for lo, hi in ranges)))
    return owned


def tsdf_box_intersect(a, b):
    """The common part of two integer boxes (start, dims), or None."""
    lo = tuple(max(s, t) for s, t in zip(a[0], b[0]))
    hi = tuple(min(s + n, t + m) for s, n, t, m in zip(a[0], a[1], b[0], b[1]))
    if any(h <= l for l, h in zip(lo, hi)):
        return None
    return lo, tuple(h - l for l, h in zip(lo, hi))


def tsdf_box_subtract(a, b):
    """What is left of the integer box a = (start, dims) without box b, as at most 6 pairwise disjoint boxes: axis by
    axis, the slab of a below b and the slab above it are cut off, and what remains is narrowed to b's range."""
    if tsdf_box_intersect(a, b) is None:
        return [(tuple(a[0]), tuple(a[1]))]
    lo, hi = list(a[0]), [s + n for s, n in zip(a[0], a[1])]
    pieces = []
    for ax in range(3):
        b_lo, b_hi = b[0][ax], b[0][ax] + b[1][ax]
        for cut_lo, cut_hi in ((lo[ax], min(hi[ax], b_lo)), (max(lo[ax], b_hi), hi[ax])):
            if cut_hi > cut_lo:
                p_lo, p_hi = list(lo), list(hi)
                p_lo[ax], p_hi[ax] = cut_lo, cut_hi
                pieces.append((tuple(p_lo), tuple(h - l for l, h in zip(p_lo, p_hi))))
        lo[ax], hi[ax] = max(lo[ax], b_lo), min(hi[ax], b_hi)
    return pieces


def tsdf_follow_decision(volume, camera_to_world, threshold: Optional[int] = None, anchor=(0.5, 0.5, 0.5)):
    """The shift TSDFVolume.follow and TSDFSpillStore.follow make for a pose: tsdf_follow_shift of the camera position of
    camera_to_world [4, 4] (of the last pose of [n, 4, 4]) once max |d_a| >= threshold (a positive int, default
    max(1, min(dims) // 8)), else (0, 0, 0).  Needs the volume's .origin, .dims and .voxel_size only."""
    m = _host_matrices("camera_to_world", camera_to_world, True)
    if not np.isfinite(m).all():
        raise RuntimeError("camera_to_world must be finite")
    if threshold is None:
        threshold = max(1, min(volume.dims) // 8)
    _int_arg("threshold", threshold)
    if threshold < 1:
        raise RuntimeError(f"threshold must be a positive int, got {threshold}")
    try:
        anchor = tuple(anchor)
    except TypeError:
        raise TypeError("anchor must be three numbers") from None
    if len(anchor) != 3:
        raise TypeError("anchor must be three numbers")
    for v in anchor:
        _number_arg("anchor", v)
        if not math.isfinite(v):
            raise RuntimeError(f"anchor must be finite, got {anchor}")
    d = tsdf_follow_shift(m[-1, :3, 3].tolist(), volume.origin, volume.dims, volume.voxel_size, anchor)
    return d if max(abs(c) for c in d) >= threshold else (0, 0, 0)


class TSDFVolume:
    """A dense truncated-signed-distance volume that fuses posed disparity maps (smx_tsdf_integrate; the rules are in
    include/stereo_mi355x.h) and gives back its surface as points (smx_tsdf_extract_points), as a triangle mesh over
    those points (smx_tsdf_extract_triangles) or as disparity, normal and colour views from any pose (render:
    smx_tsdf_raycast).  The volume has
    dims = (nx, ny, nz) voxels of edge voxel_size, its corner at origin, in the caller's world frame; voxel (i, j, k) is
    centred at origin + (i + 0.5, j + 0.5, k + 0.5) * voxel_size.  It owns the state: .tsdf and .weight float32
    [nz, ny, nx], and with color=True .color uint8 [nz, ny, nx, 4] (R, G, B, 0).  truncation (default 3 * voxel_size,
    must exceed voxel_size) is the band around each surface that a measurement updates; the weight of a voxel is capped at
    max_weight, so older frames fade once it is reached.  Memory is fixed: 8 (12 with colour) bytes per voxel -- twice
    that from the first shift() until release_spare().

    The volume can follow the camera (shift, follow; window crops and grows): it moves in whole voxels, and .offset
    (ints) counts how far it has moved from where it was built.  .origin is always the constructor's origin +
    offset * voxel_size, computed in float64 from those two, so it does not drift; a volume that is never shifted
    behaves bit for bit as one without these methods.  Assigning .origin places the volume anew (offset 0)."""

    _offset = (0, 0, 0)                                              # whole voxels moved since construction
    _spare = None                                                    # shift's second set of state tensors

    @property
    def origin(self) -> Tuple[float, float, float]:
        return tsdf_window_origin(self._origin0, self._offset, self.voxel_size)

    @origin.setter
    def origin(self, value) -> None:
        self._origin0, self._offset = tuple(value), (0, 0, 0)

    @property
    def offset(self) -> Tuple[int, int, int]:
        return self._offset

    def __init__(self, dims, voxel_size: float, origin, *, truncation: Optional[float] = None, max_weight: float = 64.0,
                 color: bool = True, device=None):
        self.dims, self.voxel_size, self.origin = _check_tsdf_volume(dims, voxel_size, origin)
        truncation = 3.0 * self.voxel_size if truncation is None else truncation
        _number_arg("truncation", truncation)
        if not (math.isfinite(truncation) and np.float32(truncation) > np.float32(self.voxel_size)):
            raise RuntimeError(f"truncation must be finite and > voxel_size, got {truncation}")
        _number_arg("max_weight", max_weight)
        if not (math.isfinite(max_weight) and max_weight > 0):
            raise RuntimeError(f"max_weight must be finite and > 0, got {max_weight}")
        if not isinstance(color, bool):
            raise TypeError("color must be a bool")
        device = torch.device("cuda") if device is None else torch.device(device)
        if device.type != "cuda":
            raise RuntimeError(f"TSDFVolume needs a GPU device, got {device}")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.device, self.truncation, self.max_weight = device, float(truncation), float(max_weight)
        nx, ny, nz = self.dims
        self.tsdf = torch.zeros((nz, ny, nx), dtype=torch.float32, device=device)
        self.weight = torch.zeros((nz, ny, nx), dtype=torch.float32, device=device)
        self.color = torch.zeros((nz, ny, nx, 4), dtype=torch.uint8, device=device) if color else None
        self._capacity = min(3 * nx * ny * nz, 2 ** 30, max(4096, 2 * (nx * ny + ny * nz + nx * nz)))

    def reset(self) -> None:
        """Returns the volume to empty (every state value 0), on the current stream.  It stays where it is: .offset and
        .origin are kept."""
        self.tsdf.zero_()
        self.weight.zero_()
        if self.color is not None:
            self.color.zero_()

    def _origin(self):
        return (C.c_float * 3)(*self.origin)

    def _state_like(self, dims):
        """Uninitialised state tensors (tsdf, weight, color or None) for a volume of `dims` like this one."""
        nx, ny, nz = dims
        return (torch.empty((nz, ny, nx), dtype=torch.float32, device=self.device),
                torch.empty((nz, ny, nx), dtype=torch.float32, device=self.device),
                None if self.color is None else torch.empty((nz, ny, nx, 4), dtype=torch.uint8, device=self.device))

    def _window_into(self, start, dims, tsdf: torch.Tensor, weight: torch.Tensor, color: Optional[torch.Tensor]) -> None:
        nx, ny, nz = self.dims
        check(LIB.smx_tsdf_window(self.device.index, nx, ny, nz, self.tsdf.data_ptr(), self.weight.data_ptr(),
                                  None if self.color is None else self.color.data_ptr(), *start, *dims, tsdf.data_ptr(),
                                  weight.data_ptr(), None if color is None else color.data_ptr(),
                                  _stream(self.device.index)))

    def window(self, start, dims) -> "TSDFVolume":
        """A new volume that holds the window of this one that starts at voxel `start` = (x0, y0, z0), of any sign, and
        has `dims` voxels (smx_tsdf_window, on the current stream without synchronising): the part inside this volume is
        copied bit for bit, the rest is empty.  Same voxel_size, truncation, max_weight, colour-ness and device; its
        origin is this volume's moved by `start` voxels (it keeps the constructor's origin, and its .offset is this
        volume's plus start).  Crops with a window inside the volume, grows it with one around it."""
        start = _int_triple("start", start, WINDOW_START_MAX)
        dims, _, _ = _check_tsdf_volume(dims, self.voxel_size, self._origin0)
        out = object.__new__(TSDFVolume)
        out.dims, out.voxel_size, out.device = dims, self.voxel_size, self.device
        out._origin0, out._offset = self._origin0, tuple(a + b for a, b in zip(self._offset, start))
        out.truncation, out.max_weight = self.truncation, self.max_weight
        out.tsdf, out.weight, out.color = self._state_like(dims)
        nx, ny, nz = dims
        out._capacity = min(3 * nx * ny * nz, 2 ** 30, max(4096, 2 * (nx * ny + ny * nz + nx * nz)))
        self._window_into(start, dims, out.tsdf, out.weight, out.color)
        return out

    def shift(self, voxels, *, spill: bool = False, margin: int = 1) -> list:
        """Moves the volume's window in the world by voxels = (dx, dy, dz) whole voxels, on the current stream without
        synchronising: afterwards voxel (i, j, k) holds what (i + dx, j + dy, k + dz) held, the voxels that entered are
        empty, .offset has grown by voxels and .origin is the constructor's origin + offset * voxel_size.  (0, 0, 0)
        does nothing and launches nothing.

        The shift is one smx_tsdf_window into a SPARE set of state tensors, which then becomes the state: .tsdf, .weight
        and .color are different tensors after a shift (hold the volume, not its tensors), and the earlier ones are the
        next shift's spare.  The spare is allocated by the first shift and reused from then on, so a volume that shifts
        needs twice its state's memory until release_spare().

        spill=True returns what left as a list of TSDFVolumes -- ordinary volumes for extract_point_cloud,
        extract_triangle_mesh and render -- one box per axis with a non-zero component, in the order x, y, z
        (tsdf_spill_boxes): the whole cross-section of the volume before the shift in the other two axes and, along its
        own axis, the layers that leave plus `margin` layers of the staying side, clipped to the volume.  margin=1 keeps
        the crossings between a leaving voxel and a staying one, which neither the shifted volume nor a box without
        margin contains.  Surface elements can then appear twice: those wholly inside a margin layer (in the box and in
        the shifted volume) and those in the corner that two boxes share; voxel_downsample at voxel_size removes the
        duplicates from point clouds.  Without spill the list is empty and what left is gone.  shift itself does not
        fuse boxes back when the volume returns to a place it has left: a TSDFSpillStore, which drives shift, keeps the
        boxes and restores them with merge(mode="fill")."""
        d = _int_triple("voxels", voxels, WINDOW_START_MAX)
        if not isinstance(spill, bool):
            raise TypeError("spill must be a bool")
        boxes = tsdf_spill_boxes(self.dims, d, margin)
        if d == (0, 0, 0):
            return []
        spilled = [self.window(start, dims) for start, dims in boxes] if spill else []
        if self._spare is None:
            self._spare = self._state_like(self.dims)
        tsdf, weight, color = self._spare
        self._window_into(d, self.dims, tsdf, weight, color)
        self._spare = (self.tsdf, self.weight, self.color)
        self.tsdf, self.weight, self.color = tsdf, weight, color
        self._offset = tuple(a + b for a, b in zip(self._offset, d))
        return spilled

    def release_spare(self) -> None:
        """Frees shift's spare state tensors; the next shift allocates them again."""
        self._spare = None

    def follow(self, camera_to_world, *, threshold: Optional[int] = None, anchor=(0.5, 0.5, 0.5), spill: bool = False,
               margin: int = 1):
        """Keeps the camera at the volume's anchor point, origin + anchor * dims * voxel_size: with d the camera position
        of camera_to_world [4, 4] (of the last pose of [n, 4, 4]) minus that point, in voxels, rounded half away from
        zero (tsdf_follow_shift; host arithmetic in float64), shifts by d once max |d_a| >= threshold and returns
        (d, shift(d, spill=spill, margin=margin)); returns ((0, 0, 0), []) otherwise.  threshold: a positive int,
        default max(1, min(dims) // 8)."""
        d = tsdf_follow_decision(self, camera_to_world, threshold, anchor)
        if d == (0, 0, 0):
            return (0, 0, 0), []
        return d, self.shift(d, spill=spill, margin=margin)

    def merge(self, other: "TSDFVolume", *, mode: str = "average", region=None) -> None:
        """Merges another volume's state into this one, in place, on the current stream without synchronising
        (smx_tsdf_merge; the rule is in include/stereo_mi355x.h).  Where `other` has measured a voxel and this volume
        has not, the voxel takes other's state bit for bit; where both have, mode="average" (the default) makes it the
        weighted mean of the two in integrate's form, the weight capped at max_weight -- two volumes fused from disjoint
        sets of frames become, up to rounding, the volume fused from all of them -- and mode="fill" keeps this volume's
        state: what restores a spilled box when the volume returns to the place it left (TSDFSpillStore).  `other` is
        not changed.

        The volumes are placed by integers alone: other.offset - self.offset, plus the distance between the two
        constructor origins in voxels, which must be a whole number exactly (computed in float64).  Both must have the
        same voxel_size, truncation, max_weight, colour-ness and device, and other must not be this volume.
        region=(start, dims), in other's voxels, limits the merge to that box of other (default: all of it); the part of
        it that lies outside this volume is ignored."""
        if not isinstance(other, TSDFVolume):
            raise TypeError("other must be a TSDFVolume")
        if other is self:
            raise RuntimeError("a volume cannot be merged into itself")
        if mode not in _native.TSDF_MERGE_MODES:
            raise RuntimeError(f"mode must be 'average' or 'fill', got {mode!r}")
        for name in ("voxel_size", "truncation", "max_weight", "device"):
            if getattr(self, name) != getattr(other, name):
                raise RuntimeError(f"merge needs volumes of the same {name}, got {getattr(self, name)} and "
                                   f"{getattr(other, name)}")
        if (self.color is None) != (other.color is None):
            raise RuntimeError("merge needs two colour volumes or two without colour")
        placement = []
        for a, b, o0, o1 in zip(self._offset, other._offset, self._origin0, other._origin0):
            apart = (float(o1) - float(o0)) / float(self.voxel_size)
            if apart != math.floor(apart):
                raise RuntimeError(f"the volumes' origins {tuple(self._origin0)} and {tuple(other._origin0)} are not a whole "
                                   f"number of voxels apart ({apart} on one axis)")
            placement.append(b - a + int(apart))
        if region is None:
            start, dims = (0, 0, 0), other.dims
        else:
            try:
                start, dims = region
            except (TypeError, ValueError):
                raise TypeError("region must be (start, dims), three ints each") from None
            start, dims = _int_triple("region start", start), _int_triple("region dims", dims)
            if any(s < 0 or n < 1 or s + n > m for s, n, m in zip(start, dims, other.dims)):
                raise RuntimeError(f"region {start} + {dims} does not lie inside the other volume's {other.dims} voxels")
        if any(abs(p) > WINDOW_START_MAX for p in placement):
            raise RuntimeError(f"merge: the volumes are {tuple(placement)} voxels apart, at most {WINDOW_START_MAX} per axis")
        ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        check(LIB.smx_tsdf_merge(self.device.index, *self.dims, self.tsdf.data_ptr(), self.weight.data_ptr(),
                                 ptr(self.color), *other.dims, other.tsdf.data_ptr(), other.weight.data_ptr(),
                                 ptr(other.color), *placement, *start, *dims, _native.TSDF_MERGE_MODES[mode],
                                 self.max_weight, _stream(self.device.index)))

    def integrate(self, disp: torch.Tensor, Q, camera_to_world, *, image: Optional[torch.Tensor] = None,
                  confidence: Optional[torch.Tensor] = None, min_confidence: float = 0.0, depth_range=(0.0, math.inf),
                  invalid_disparity: float = -1.0) -> None:
        """Fuses n disparity maps float32 [H, W] or [n, H, W] (on the volume's device) taken with the cameras at
        camera_to_world [4, 4] / [n, 4, 4] (numpy or tensor; x right, y down, z forward, as reproject_to_3d), in order, on
        the current stream without synchronising.  Q: the maps' 4x4 reprojection matrix; its inverse, computed in float64,
        projects voxels to pixels.  A pixel counts where reproject_to_3d would make it a point (with depth_range,
        invalid_disparity and, given a confidence map [n, H, W], confidence >= min_confidence) and its confidence is
        > 0; its weight is its confidence, or 1.  image: the colour source, [H, W] / [1, H, W] (gray) or [3, H, W]
        (RGB) per map, uint8 or float32; required by a colour volume, ignored otherwise."""
        q = _check_q(Q)
        p = projection_matrix(q)
        z_min, z_max = _check_reproject_params(min_confidence, depth_range, invalid_disparity)
        w2c = world_to_camera_poses(camera_to_world)
        _check_input("disp", disp)
        if disp.dtype != torch.float32 or disp.dim() not in (2, 3) or disp.device != self.device:
            raise RuntimeError(f"disp must be float32 [H, W] or [n, H, W] on {self.device}, got {disp.dtype} "
                               f"{tuple(disp.shape)} on {disp.device}")
        batched = disp.dim() == 3
        n, H, W = disp.shape if batched else (1,) + tuple(disp.shape)
        if not (n >= 1 and 1 <= H <= 32768 and 1 <= W <= 32768 and n * H * W <= 2 ** 30):
            raise RuntimeError(f"need n >= 1, 1 <= H, W <= 32768 and n * H * W <= 2^30, got {tuple(disp.shape)}")
        if w2c.shape[0] != n:
            raise RuntimeError(f"{n} map(s) need {n} pose(s), got {w2c.shape[0]}")
        if confidence is not None:
            _check_like("confidence", confidence, torch.float32, disp.shape, self.device)
        channels = 0
        if self.color is not None:
            if image is None:
                raise RuntimeError("a colour volume needs image= (or build the volume with color=False)")
            channels = _check_colour_image(image, n, H, W, batched, self.device)
        else:
            image = None
        poses = torch.from_numpy(w2c).pin_memory().to(self.device, non_blocking=True)
        ws_bytes = LIB.smx_tsdf_integrate_workspace_bytes(n, H, W)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=self.device)
        qc = (C.c_float * 16)(*q.reshape(-1).tolist())
        pc = (C.c_float * 16)(*p.reshape(-1).tolist())
        ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        dtype = _native.DTYPE_F32 if image is not None and image.dtype == torch.float32 else _native.DTYPE_U8
        nx, ny, nz = self.dims
        check(LIB.smx_tsdf_integrate(self.device.index, nx, ny, nz, self._origin(), self.voxel_size, self.truncation,
                                     self.max_weight, self.tsdf.data_ptr(), self.weight.data_ptr(), ptr(self.color),
                                     n, H, W, disp.data_ptr(), qc, pc, poses.data_ptr(), ptr(confidence),
                                     float(min_confidence), z_min, z_max, float(invalid_disparity), ptr(image),
                                     channels, dtype, ws.data_ptr(), ws_bytes, _stream(self.device.index)))

    def integrate_points(self, cloud, Q, camera_to_world, shape, *, radius: int = 0, **integrate_kwargs) -> None:
        """Fuses a point cloud (a PointCloud or an [N, 3] tensor: a LiDAR scan, a spilled box's cloud, a downsampled
        cloud) as the measurement of a camera at camera_to_world [4, 4] with the reprojection matrix Q and (H, W) pixels.
        Composition only: integrate(project_points(cloud, Q, camera_to_world, shape, radius=radius, ...).disparity, Q,
        camera_to_world, image=the view's colours, ...); depth_range and invalid_disparity go to both, the other
        keywords to integrate.  A colour volume needs a cloud with colours (or image=)."""
        shared = {k: integrate_kwargs[k] for k in ("depth_range", "invalid_disparity") if k in integrate_kwargs}
        view = project_points(cloud, Q, camera_to_world, shape, radius=radius, index=False, **shared)
        integrate_kwargs.setdefault("image", view.colors)
        self.integrate(view.disparity, Q, camera_to_world, **integrate_kwargs)

    def _check_render_args(self, Q, camera_to_world, shape, min_weight, step, depth_range, normals, colors,
                           invalid_disparity):
        """render's arguments, before the device is touched: (q, poses [n, 3, 4] f32, batched, (H, W), step,
        (z_min, z_max))."""
        q = _check_q(Q)
        if (q[:3, 2] != 0).any() or q[3, 0] != 0 or q[3, 1] != 0 or q[3, 2] == 0:
            raise RuntimeError("Q's ray must not depend on the disparity: need Q[0..2, 2] = 0, Q[3, 0] = Q[3, 1] = 0 and "
                               "Q[3, 2] != 0 (what reprojection_matrix builds)")
        poses = camera_to_world_poses(camera_to_world)
        batched = (camera_to_world.dim() if isinstance(camera_to_world, torch.Tensor) else np.ndim(camera_to_world)) == 3
        H, W = _shape2("shape", shape)
        n = poses.shape[0]
        if n * H * W > 2 ** 30:
            raise RuntimeError(f"need n * H * W <= 2^30, got {n} views of {(H, W)}")
        _number_arg("min_weight", min_weight)
        if not (math.isfinite(min_weight) and min_weight > 0):
            raise RuntimeError(f"min_weight must be finite and > 0, got {min_weight}")
        step = self.voxel_size if step is None else step
        _number_arg("step", step)
        if not (math.isfinite(step) and step > 0):
            raise RuntimeError(f"step must be finite and > 0, got {step}")
        _number_arg("invalid_disparity", invalid_disparity)
        if not math.isfinite(invalid_disparity):
            raise RuntimeError(f"invalid_disparity must be finite, got {invalid_disparity}")
        for name, v in (("normals", normals), ("colors", colors)):
            if not isinstance(v, bool):
                raise TypeError(f"{name} must be a bool")
        if depth_range is None:                                         # no ray is longer than eye to farthest corner
            lo = np.asarray(self.origin, np.float64)
            hi = lo + np.asarray(self.dims, np.float64) * self.voxel_size
            corners = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])])
            eyes = poses[:, :, 3].astype(np.float64)
            depth_range = (0.0, float(np.linalg.norm(corners[None] - eyes[:, None], axis=2).max()))
        try:
            z_min, z_max = depth_range
        except (TypeError, ValueError):
            raise TypeError("depth_range must be a pair (z_min, z_max)") from None
        _number_arg("depth_range[0]", z_min)
        _number_arg("depth_range[1]", z_max)
        if not (math.isfinite(z_min) and math.isfinite(z_max) and 0 <= z_min <= z_max):
            raise RuntimeError(f"depth_range must be finite with 0 <= z_min <= z_max, got {depth_range}")
        samples = math.floor((np.float32(z_max) - np.float32(z_min)) / np.float32(step)) + 1
        if samples > 65536:
            raise RuntimeError(f"depth_range / step gives {samples} samples per ray, the limit is 65536")
        return q, poses, batched, (H, W), float(step), (float(z_min), float(z_max))

    def render(self, Q, camera_to_world, shape, *, min_weight: float = 1.0, step: Optional[float] = None,
               depth_range=None, normals: bool = True, colors: bool = True,
               invalid_disparity: float = -1.0) -> RenderedView:
        """The volume seen from camera_to_world [4, 4] / [n, 4, 4] (numpy or tensor; rounded once to float32, not
        inverted) through a camera with the reprojection matrix Q, as maps of shape (H, W): one ray per pixel, sampled
        every `step` (default voxel_size) of camera depth over depth_range (default 0 .. the distance from the eye to
        the volume's farthest corner, computed in float64 per call), hits the surface at the first change of the tsdf
        from [0, 1) to negative between two samples whose eight voxels all have weight >= min_weight
        (smx_tsdf_raycast; the rule is in include/stereo_mi355x.h).  Q's ray must not depend on the disparity, which
        holds for every reprojection_matrix.  Runs on the current stream without synchronising and returns a
        RenderedView of fresh tensors; a novel pose is as good as one that was fused."""
        q, poses, batched, (H, W), step, (z_min, z_max) = self._check_render_args(
            Q, camera_to_world, shape, min_weight, step, depth_range, normals, colors, invalid_disparity)
        dev, n = self.device, poses.shape[0]
        disp = torch.empty((n, H, W), dtype=torch.float32, device=dev)
        depth = torch.empty((n, H, W), dtype=torch.float32, device=dev)
        weight = torch.empty((n, H, W), dtype=torch.float32, device=dev)
        nrm = torch.empty((n, 3, H, W), dtype=torch.float32, device=dev) if normals else None
        col = torch.empty((n, 3, H, W), dtype=torch.uint8, device=dev) if colors and self.color is not None else None
        pose_dev = torch.from_numpy(poses).pin_memory().to(dev, non_blocking=True)
        nx, ny, nz = self.dims
        ws_bytes = LIB.smx_tsdf_raycast_workspace_bytes(nx, ny, nz)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        qc = (C.c_float * 16)(*q.reshape(-1).tolist())
        ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        check(LIB.smx_tsdf_raycast(dev.index, nx, ny, nz, self._origin(), self.voxel_size, self.tsdf.data_ptr(),
                                   self.weight.data_ptr(), ptr(self.color), float(min_weight), n, H, W, qc,
                                   pose_dev.data_ptr(), step, z_min, z_max, float(invalid_disparity), disp.data_ptr(),
                                   depth.data_ptr(), ptr(nrm), ptr(col), weight.data_ptr(), ws.data_ptr(), ws_bytes,
                                   _stream(dev.index)))
        if not batched:
            disp, depth, weight = disp[0], depth[0], weight[0]
            nrm, col = (None if t is None else t[0] for t in (nrm, col))
        return RenderedView(disparity=disp, depth=depth, normals=nrm, colors=col, weight=weight)

    def track(self, disp: torch.Tensor, Q, pose_guess, *, render_shape=None, min_weight: float = 1.0,
              step: Optional[float] = None, render_depth_range=None, **track_args) -> TrackingResult:
        """The pose of the frame(s) disp (float32 [H, W] / [n, H, W], reprojection matrix Q) against this volume: renders
        it from pose_guess [4, 4] / [n, 4, 4] (render, at render_shape -- default the frame's -- with min_weight, step
        and render_depth_range as its depth_range, depth and normals only) and tracks the frame against that view from
        the same pose (track_camera, which takes track_args).  Frame-to-model tracking: fuse the frame at the returned
        pose if it is not lost, and pass that pose as the next frame's guess.  With image= and a photometric_weight > 0
        among track_args the view is rendered with its colours, which then are the model's intensity; the volume must
        have been created with color=True."""
        if not isinstance(disp, torch.Tensor) or disp.dim() not in (2, 3):
            raise RuntimeError("disp must be a float32 tensor [H, W] or [n, H, W]")
        shape = tuple(disp.shape[-2:]) if render_shape is None else render_shape
        invalid = track_args.get("invalid_disparity", -1.0)
        weight = track_args.get("photometric_weight", 0.0)
        colors = (track_args.get("image") is not None and track_args.get("model_intensity") is None and
                  isinstance(weight, (int, float)) and weight > 0)
        if colors and self.color is None:
            raise RuntimeError("tracking with the photometric term needs a colour volume (TSDFVolume(..., color=True))")
        view = self.render(Q, pose_guess, shape, min_weight=min_weight, step=step, depth_range=render_depth_range,
                           normals=True, colors=colors, invalid_disparity=invalid)
        return track_camera(disp, Q, pose_guess, view, pose_guess, model_Q=Q, **track_args)

    def extract_point_cloud_batched(self, capacity: int, *, min_weight: float = 1.0, normals: bool = True,
                                    colors: bool = True):
        """The surface points without synchronising (smx_tsdf_extract_points, on the current stream): returns
        (points [capacity, 3] f32, normals [capacity, 3] f32 or None, colors [capacity, 3] u8 or None, count [1] int32),
        fresh tensors of which the first min(count, capacity) rows are written."""
        _int_arg("capacity", capacity)
        if not 1 <= capacity <= 2 ** 30:
            raise RuntimeError(f"capacity must be in 1..2^30, got {capacity}")
        _number_arg("min_weight", min_weight)
        if not (math.isfinite(min_weight) and min_weight > 0):
            raise RuntimeError(f"min_weight must be finite and > 0, got {min_weight}")
        dev = self.device
        pts = torch.empty((capacity, 3), dtype=torch.float32, device=dev)
        nrm = torch.empty((capacity, 3), dtype=torch.float32, device=dev) if normals else None
        col = torch.empty((capacity, 3), dtype=torch.uint8, device=dev) if colors and self.color is not None else None
        count = torch.empty(1, dtype=torch.int32, device=dev)
        nx, ny, nz = self.dims
        ws_bytes = LIB.smx_tsdf_extract_workspace_bytes(nx, ny, nz)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        check(LIB.smx_tsdf_extract_points(dev.index, nx, ny, nz, self._origin(), self.voxel_size, self.tsdf.data_ptr(),
                                          self.weight.data_ptr(), ptr(self.color), float(min_weight), capacity,
                                          pts.data_ptr(), ptr(nrm), ptr(col), count.data_ptr(), ws.data_ptr(),
                                          ws_bytes, _stream(dev.index)))
        return pts, nrm, col, count

    def extract_point_cloud(self, min_weight: float = 1.0, normals: bool = True) -> PointCloud:
        """The volume's surface as a PointCloud (points, unit normals toward the cameras with normals=True, colours of a
        colour volume): one point per zero crossing of the tsdf between two neighbouring voxels that both have weight
        >= min_weight and |tsdf| < 1, in ascending voxel order (the rule is in include/stereo_mi355x.h).  SYNCHRONISES
        to read the count; a first capacity that was too small is retried once with the exact count."""
        for attempt in range(2):
            pts, nrm, col, count = self.extract_point_cloud_batched(self._capacity, min_weight=min_weight,
                                                                    normals=normals)
            total = int(count.item())                                   # the synchronisation
            if total <= self._capacity or attempt == 1:
                break
            self._capacity = min(total, 2 ** 30)
        total = min(total, self._capacity)
        return PointCloud(points=pts[:total], colors=None if col is None else col[:total],
                          normals=None if nrm is None else nrm[:total])

    def extract_triangle_mesh_batched(self, vertex_capacity: int, triangle_capacity: int, *, min_weight: float = 1.0,
                                      normals: bool = True, colors: bool = True):
        """The surface as an indexed mesh without synchronising (smx_tsdf_extract_points, then
        smx_tsdf_extract_triangles, on the current stream): returns extract_point_cloud_batched(vertex_capacity)'s
        (points, normals, colors, count) followed by triangles [triangle_capacity, 3] int32, of which the first
        min(triangle_count, triangle_capacity) rows are written, and triangle_count [1] int32 (-1: the volume has more
        crossings than an int32 can index).  The indices refer to the complete vertex list, whatever vertex_capacity."""
        _int_arg("triangle_capacity", triangle_capacity)
        if not 1 <= triangle_capacity <= 2 ** 30:
            raise RuntimeError(f"triangle_capacity must be in 1..2^30, got {triangle_capacity}")
        pts, nrm, col, count = self.extract_point_cloud_batched(vertex_capacity, min_weight=min_weight, normals=normals,
                                                                colors=colors)
        dev = self.device
        tris = torch.empty((triangle_capacity, 3), dtype=torch.int32, device=dev)
        tcount = torch.empty(1, dtype=torch.int32, device=dev)
        nx, ny, nz = self.dims
        ws_bytes = LIB.smx_tsdf_extract_triangles_workspace_bytes(nx, ny, nz)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        check(LIB.smx_tsdf_extract_triangles(dev.index, nx, ny, nz, self.tsdf.data_ptr(), self.weight.data_ptr(),
                                             float(min_weight), triangle_capacity, tris.data_ptr(), tcount.data_ptr(),
                                             ws.data_ptr(), ws_bytes, _stream(dev.index)))
        return pts, nrm, col, count, tris, tcount

    def extract_triangle_mesh(self, min_weight: float = 1.0, normals: bool = True) -> TriangleMesh:
        """The volume's surface as a TriangleMesh: the vertices (normals, colours) are extract_point_cloud's points,
        unchanged and in the same order, and the triangles are marching cubes over the cells whose eight voxels all have
        weight >= min_weight and |tsdf| < 1 (the rule is in include/stereo_mi355x.h); a crossing next to a cell that is
        not valid stays as a vertex without a triangle.  SYNCHRONISES to read the counts; capacities that were too small
        are retried once with the exact counts."""
        tcap = min(2 * self._capacity, 2 ** 30)
        for attempt in range(2):
            pts, nrm, col, count, tris, tcount = self.extract_triangle_mesh_batched(
                self._capacity, tcap, min_weight=min_weight, normals=normals)
            total, ttotal = int(count.item()), int(tcount.item())          # the synchronisation
            if ttotal < 0:
                raise RuntimeError("the volume has more than 2^31 - 1 crossings: its vertices cannot be indexed")
            if (total <= self._capacity and ttotal <= tcap) or attempt == 1:
                break
            self._capacity = min(max(total, self._capacity), 2 ** 30)
            tcap = min(max(ttotal, 1), 2 ** 30)
        if total > self._capacity or ttotal > tcap:
            raise RuntimeError(f"the mesh has {total} vertices and {ttotal} triangles: more than 2^30")
        return TriangleMesh(vertices=pts[:total], triangles=tris[:ttotal], normals=None if nrm is None else nrm[:total],
                            colors=None if col is None else col[:total])


def _state_bytes(volume) -> int:
    nx, ny, nz = volume.dims
    return nx * ny * nz * (8 if volume.color is None else 12)


def _measured_flags(views) -> list:
    """Per array of weights (device tensors, or NumPy arrays of float32 or their uint32 words), whether a weight is > 0;
    the device's flags come back in ONE copy: the synchronisation of TSDFSpillStore.shift."""
    if not views:
        return []
    if isinstance(views[0], torch.Tensor):
        return torch.stack([(v > 0).any() for v in views]).tolist()
    return [bool((np.asarray(v).view(np.float32) > 0).any()) for v in views]


class TSDFSpillStore:
    """Keeps what left a volume that follows the camera and gives it back when the volume returns: the memory of a
    TSDFVolume beyond its window.  The store drives the volume -- call store.shift(volume, d) or store.follow(volume,
    pose) in place of the volume's own methods.  Each shift spills the leaving layers into boxes (TSDFVolume.shift with
    spill=True; the boxes stay on the device), records for each box the region it OWNS, and restores every owned region
    that lies inside the volume's new window with volume.merge(box, mode="fill", region=...): the voxels go back where
    the window is empty, bit for bit, and what the volume has measured there since stays.

    Ownership is kept in integer boxes of world voxels (offset space: voxel (0, 0, 0) is the first voxel of the volume
    as it was built).  Every world voxel that ever left is owned by exactly one holder, the live volume or one entry of
    the store (tsdf_spill_ownership splits what a shift cuts off among its boxes, margin layers excluded); a restored
    region passes from the entry back to the volume (tsdf_box_subtract), and an entry that owns nothing any more is
    dropped with its tensors.  A region in which nothing was measured is not kept either (a new box's, and what is left
    of a region restored in part): that is read back from the device, one flag per region in one copy, the ONE
    synchronisation of a shift through the store.

    max_bytes: a bound on the bytes of state the entries hold; beyond it the OLDEST entries are evicted -- that territory
    is forgotten, and .evicted counts them.  len(store) is the number of entries, .bytes their state's bytes, and
    volumes() the boxes themselves (ordinary volumes: extract, render or archive them).  One store serves one volume:
    it refuses a volume whose voxel_size, truncation, max_weight, colour-ness, device or constructor origin differ from
    the first one it saw.  Not done: offload of entries to the host or to disk, loop closure and relocalisation -- a
    returning camera finds its old model only as far as its pose estimate is consistent with the old one."""

    def __init__(self, max_bytes: Optional[int] = None):
        if max_bytes is not None:
            _int_arg("max_bytes", max_bytes)
            if max_bytes < 0:
                raise RuntimeError(f"max_bytes must be >= 0 or None, got {max_bytes}")
        self.max_bytes, self.evicted = max_bytes, 0
        self._entries = []                                           # oldest first: [box volume, [owned world boxes]]
        self._key = None

    def __len__(self) -> int:
        return len(self._entries)

    @property
    def bytes(self) -> int:
        return sum(_state_bytes(box) for box, _ in self._entries)

    def volumes(self) -> list:
        """The entries' boxes, oldest first."""
        return [box for box, _ in self._entries]

    def owned_regions(self) -> list:
        """Per entry, oldest first, the world-voxel boxes (start, dims) it still owns."""
        return [list(owned) for _, owned in self._entries]

    def _check_volume(self, volume) -> None:
        key = (volume.voxel_size, volume.truncation, volume.max_weight, volume.color is not None, volume.device,
               tuple(volume._origin0))
        if self._key is None:
            self._key = key
        elif key != self._key:
            raise RuntimeError("a TSDFSpillStore serves one volume: voxel_size, truncation, max_weight, colour-ness, device and "
                               f"constructor origin were {self._key}, got {key}")

    def shift(self, volume, voxels, *, margin: int = 1):
        """volume.shift(voxels, spill=True, margin=margin) through the store: returns (boxes, restored) -- the boxes that
        shift handed back (all of them, whether the store keeps them or not) and the number of merges launched to
        restore what the store held of the new window.  Everything runs on the current stream; a shift that spills
        synchronises once (see the class)."""
        self._check_volume(volume)
        d = _int_triple("voxels", voxels, WINDOW_START_MAX)
        before, dims = tuple(volume.offset), tuple(volume.dims)
        boxes = volume.shift(d, spill=True, margin=margin)
        if d == (0, 0, 0):
            return boxes, 0
        window = (tuple(volume.offset), dims)
        restored, unsure = 0, []                                     # unsure: (entry, region) that may hold nothing
        for entry in self._entries:
            box, owned = entry
            entry[1] = []
            for region in owned:
                part = tsdf_box_intersect(region, window)
                if part is None:
                    entry[1].append(region)
                    continue
                volume.merge(box, mode="fill", region=(tuple(s - o for s, o in zip(part[0], box.offset)), part[1]))
                restored += 1
                unsure.extend((entry, piece) for piece in tsdf_box_subtract(region, part))
        for box, own in zip(boxes, tsdf_spill_ownership(dims, d)):
            if own is not None:
                entry = [box, []]
                self._entries.append(entry)
                unsure.append((entry, (tuple(a + b for a, b in zip(before, own[0])), own[1])))
        views = []                                                   # the weights of each such region in its box
        for (box, _), (start, size) in unsure:
            x, y, z = (s - o for s, o in zip(start, box.offset))
            views.append(box.weight[z:z + size[2], y:y + size[1], x:x + size[0]])
        for (entry, region), measured in zip(unsure, _measured_flags(views)):
            if measured:
                entry[1].append(region)
        self._entries = [e for e in self._entries if e[1]]
        while self.max_bytes is not None and self._entries and self.bytes > self.max_bytes:
            self._entries.pop(0)
            self.evicted += 1
        return boxes, restored

    def follow(self, volume, camera_to_world, *, threshold: Optional[int] = None, anchor=(0.5, 0.5, 0.5), margin: int = 1):
        """TSDFVolume.follow through the store, with the same arithmetic (tsdf_follow_decision): returns
        (d, boxes, restored), ((0, 0, 0), [], 0) for a pose that does not move the volume."""
        self._check_volume(volume)
        d = tsdf_follow_decision(volume, camera_to_world, threshold, anchor)
        if d == (0, 0, 0):
            return (0, 0, 0), [], 0
        boxes, restored = self.shift(volume, d, margin=margin)
        return d, boxes, restored
