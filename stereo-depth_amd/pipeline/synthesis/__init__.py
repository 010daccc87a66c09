"""Right-view synthesis for single-camera depth: the counterpart of the reference's pipeline.synthesis.RightViewSynthesis
(right_view_synthesis.py:9-32), with the network left to the caller.

The reference runs a traced Deep3D: a VGG-based network that ends in a softmax over 65 disparity planes at a quarter of
the frame's resolution, followed by an upsampling, a "selection layer" (65 shifted copies of the left frame, weighted
and summed) and a rescale to 0..255.  Here the network is any callable the caller brings -- its convolutions are
MIOpen's business -- and everything after its last layer is one HIP kernel (cuda_depth.synthesize_right_view), which
never stores the upsampled volume or the shifted copies.  For training, the network, the loss, the optimiser and the
loop stay the caller's; the differentiable head is here: SelectionLayer (cuda_depth.synthesis_head), the same fused
kernel without the rescale and a hand-written HIP backward that gives the volume's gradient.  No network definition or
weights are part of this package."""
from __future__ import annotations

from typing import Callable, Optional, Tuple

import torch
import torch.nn.functional as F

import cuda_depth

__all__ = ["RightViewSynthesis", "DisparityOracleModel", "SelectionLayer"]


class SelectionLayer(torch.nn.Module):
    """The selection layer of Deep3D for training: forward(probabilities, left_full) -> the generated right view in
    0..1, [n, C, H, W] float32, differentiable with respect to probabilities (cuda_depth.synthesis_head).

    It takes the low-resolution volume [n, D, H / scale, W / scale] as the network's softmax leaves it, not the
    upsampled one: it is the drop-in for F.interpolate(volume, scale_factor=scale, mode="bilinear") followed by the
    reference's ViewSynthesisNetwork (shifted copies, product, sum), in two launches per step instead of a
    D x C x H x W stack held for autograd.  left_full is the frame in 0..1 (float32) or uint8; it gets no gradient.
    The layer has no parameters; the loss (the reference: L1 against the true right view) is the caller's."""

    def __init__(self, scale: int = 4):
        super().__init__()
        if isinstance(scale, bool) or not isinstance(scale, int):
            raise TypeError("scale must be an int")
        if not 1 <= scale <= 16:
            raise ValueError(f"scale must be in 1..16, got {scale}")
        self.scale = scale

    def forward(self, probabilities: torch.Tensor, left_full: torch.Tensor) -> torch.Tensor:
        return cuda_depth.synthesis_head(probabilities, left_full, self.scale)

    def extra_repr(self) -> str:
        return f"scale={self.scale}"


class DisparityOracleModel:
    """A weight-free stand-in for the network, for tests, tools and demos: the linear splat of a known low-resolution
    disparity map, P[d] = max(0, 1 - |d - disp|) for d = 0 .. D-1, in plain torch operations.  disp is clamped into
    0 .. D-1 first, so the planes are non-negative and sum to 1 at every pixel.  Through RightViewSynthesis it renders
    the right view of any frame from any disparity map (depth-image-based rendering): disparity_lowres is [h, w], in
    units of full-resolution pixels."""

    def __init__(self, disparity_lowres: torch.Tensor, D: int):
        if not isinstance(disparity_lowres, torch.Tensor) or disparity_lowres.dim() != 2:
            raise ValueError("disparity_lowres must be an [h, w] tensor")
        if isinstance(D, bool) or not isinstance(D, int) or not 1 <= D <= 256:
            raise ValueError(f"D must be an int in 1..256, got {D!r}")
        self.disparity_lowres = disparity_lowres.to(torch.float32)
        self.D = D

    def __call__(self, left_full: torch.Tensor, left_downscaled: torch.Tensor) -> torch.Tensor:
        disp = self.disparity_lowres.to(left_full.device).clamp(0.0, float(self.D - 1))
        planes = torch.arange(self.D, dtype=torch.float32, device=disp.device).view(self.D, 1, 1)
        return (1.0 - (planes - disp).abs()).clamp_min(0.0).unsqueeze(0).contiguous()


class RightViewSynthesis:
    """process(left_view) -> the generated right view, [3, H, W] float32 in 0..255, as the reference's class of this name.

    model: a callable (left_full [1, 3, H, W], left_downscaled [1, 3, H / scale, W / scale]), both float32 in 0..1 on the
    GPU, returning
      - model_output="probabilities": the soft-maxed volume [1, D, H / scale, W / scale] (D in 1..256), e.g. a
        torch.jit.load'ed trace of the network cut after its softmax; the head is cuda_depth.synthesize_right_view;
      - model_output="view": the generated view [1, 3, H, W] in 0..1, which is what the reference's own trace returns
        (it contains the upsampling and the selection layer); only the rescale `* 255 + 0.5`, clamped to 0..255, is
        applied (the same kernel with one plane of ones), so an existing trace works unchanged.
    full_resolution: the (H, W) every frame must have (the KITTI camera pads to 384 x 1280); a frame of another size is
    refused.  downscale: left_full -> left_downscaled; the default is F.interpolate(mode="bilinear",
    align_corners=False) -- it is a parameter because the weights decide which resampling they were trained with.
    Frames are uint8 or floating point in 0..255 and are divided by 255 (in float32), as the reference does.
    The result aliases a persistent buffer (like the engine's output buffer): clone it before the next call if it must
    survive."""

    def __init__(self, model: Callable[[torch.Tensor, torch.Tensor], torch.Tensor], *,
                 full_resolution: Tuple[int, int] = (384, 1280), scale: int = 4, model_output: str = "probabilities",
                 downscale: Optional[Callable[[torch.Tensor], torch.Tensor]] = None):
        if not callable(model):
            raise TypeError("model must be callable")
        if isinstance(scale, bool) or not isinstance(scale, int):
            raise TypeError("scale must be an int")
        if not 1 <= scale <= 16:
            raise ValueError(f"scale must be in 1..16, got {scale}")
        if model_output not in ("probabilities", "view"):
            raise ValueError(f"model_output must be 'probabilities' or 'view', got {model_output!r}")
        H, W = (int(v) for v in full_resolution)
        if H < scale or W < scale or H % scale or W % scale:
            raise ValueError(f"full_resolution {H} x {W} must be a positive multiple of scale {scale}")
        if downscale is not None and not callable(downscale):
            raise TypeError("downscale must be callable")
        self._model = model
        self._full_resolution = (H, W)
        self._downscaled_resolution = (H // scale, W // scale)
        self._scale = scale
        self._model_output = model_output
        self._downscale = downscale if downscale is not None else self._bilinear_downscale
        self._out: Optional[torch.Tensor] = None
        self._ones: Optional[torch.Tensor] = None             # model_output="view": the one probability plane

    def _bilinear_downscale(self, left_full: torch.Tensor) -> torch.Tensor:
        return F.interpolate(left_full, size=self._downscaled_resolution, mode="bilinear", align_corners=False)

    @torch.no_grad()
    def process(self, left_view: torch.Tensor) -> torch.Tensor:
        H, W = self._full_resolution
        if not isinstance(left_view, torch.Tensor):
            raise TypeError("left_view must be a torch.Tensor")
        if tuple(left_view.shape) != (3, H, W):
            raise ValueError(f"left_view must be [3, {H}, {W}] (full_resolution), got {tuple(left_view.shape)}")
        left_view = left_view.cuda().contiguous()
        left_full = (left_view.to(torch.float32) / 255.0).unsqueeze(0)
        # a uint8 frame goes to the kernel as it is (it divides by 255 in the same way); anything else as float32 in 0..1
        head_input = left_view if left_view.dtype == torch.uint8 else left_full[0]
        result = self._model(left_full, self._downscale(left_full))
        if self._out is None or self._out.device != left_view.device:
            self._out = torch.empty((3, H, W), dtype=torch.float32, device=left_view.device)
        if self._model_output == "view":
            if not isinstance(result, torch.Tensor) or tuple(result.shape) not in ((1, 3, H, W), (3, H, W)):
                raise ValueError(f"the model must return the view [1, 3, {H}, {W}], got "
                                 f"{tuple(getattr(result, 'shape', ()))}")
            if self._ones is None or self._ones.device != left_view.device:
                self._ones = torch.ones((1, H, W), dtype=torch.float32, device=left_view.device)
            view = result.to(torch.float32).reshape(3, H, W).contiguous()
            return cuda_depth.synthesize_right_view(self._ones, view, scale=1, out=self._out)
        h, w = self._downscaled_resolution
        if not isinstance(result, torch.Tensor) or result.dim() != 4 or \
                (int(result.shape[0]), int(result.shape[2]), int(result.shape[3])) != (1, h, w):
            raise ValueError(f"the model must return probabilities [1, D, {h}, {w}], got "
                             f"{tuple(getattr(result, 'shape', ()))}")
        return cuda_depth.synthesize_right_view(result[0].to(torch.float32).contiguous(), head_input,
                                                scale=self._scale, out=self._out)
