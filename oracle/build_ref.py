"""Recipe: builds the reference's own stereo path for the HOST into oracle/_ref/ (test infrastructure only).

The reference (dusanerdeljan/stereo-depth) is CUDA against libtorch-CUDA, but its stereo path uses a sliver of both:
eight small float32 kernels, torch::empty, size(), packed accessors, one dispatch macro, dim3, the built-in indices,
eight launches, and one kernel with dynamic shared memory and one barrier.  oracle/ref_host/ provides exactly that for
g++ (see ref_host.h), so the program that runs is the reference's text and not a reading of it.

The reference tree is read from $STEREO_REFERENCE_DIR (default /root/reference) and never copied into version
control: rewritten copies of the needed sources go to oracle/_ref/src/, the libraries to oracle/_ref/, and all of
oracle/_ref/ is git-ignored.  Two mechanical rewrites are applied, because g++ cannot parse the two constructs:

    kernel<scalar_t><<<grid, block[, shared]>>>(args)   ->  refhost::launch(refhost::launch_cfg(grid, block[, shared]), kernel<scalar_t>, args)
    extern __shared__ ... T name[];                     ->  T* name = static_cast<T*>(refhost::block_shared());

A rewrite that matches another number of places than listed below is an error: a silent miss would compile a launch
away.  libref_host.so is built with -ffp-contract=off (floating-point convention 0 of stereo_oracle.h); when the CPU
has FMA, libref_host_fma.so is built with -mfma -ffp-contract=fast as well, so that a real compiler's own choice of
contractions can be classified.

    python oracle/build_ref.py            # build (no-op when current)
"""
from __future__ import annotations

import hashlib
import os
import re
import shutil
import subprocess
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
HOST = os.path.join(_HERE, "ref_host")
OUT = os.path.join(_HERE, "_ref")
LIB = os.path.join(OUT, "libref_host.so")
LIB_FMA = os.path.join(OUT, "libref_host_fma.so")

# path under <reference>/src/csrc: (launches expected, extern __shared__ declarations expected); None = copied as is
SOURCES = {
    "depth/stereo_matching.cc": None,
    "depth/stereo_matching.hh": None,
    "depth/stereo_matching_configuration.hh": None,
    "depth/buffer/device_buffer.cc": None,
    "depth/buffer/device_buffer.hh": None,
    "depth/kernels/device_functions.cuh": None,
    "depth/kernels/ncc_matching_cost_volume_construction.hh": None,
    "depth/kernels/multi_block_matching_cost_aggregation.hh": None,
    "depth/kernels/wta_disparity_selection.hh": None,
    "depth/kernels/secondary_matching.hh": None,
    "depth/kernels/upscale_disparity_vertical_fill.hh": None,
    "depth/kernels/horizontal_disparity_fill.hh": None,
    "imageops/rgb_to_grayscale.hh": None,
    "imageops/mean_pool.hh": None,
    "imageops/kernels/rgb_to_grayscale.cu": (1, 0),
    "imageops/kernels/mean_pool.cu": (1, 0),
    "depth/kernels/ncc_matching_cost_volume_construction.cu": (1, 0),
    "depth/kernels/multi_block_matching_cost_aggregation.cu": (1, 1),
    "depth/kernels/wta_disparity_selection.cu": (1, 0),
    "depth/kernels/secondary_matching.cu": (1, 0),
    "depth/kernels/upscale_disparity_vertical_fill.cu": (1, 0),
    "depth/kernels/horizontal_disparity_fill.cu": (1, 0),
}
OWN = ("driver.cc", "runner.cc", "selfcheck.cc")
HEADERS = ("ref_host.h", "cuda.h", "cuda_runtime.h", os.path.join("torch", "extension.h"))

BASE_FLAGS = ["-std=c++17", "-fno-fast-math", "-fPIC", "-shared", "-Wall", "-Wno-unknown-pragmas", "-Wno-sign-compare"]
FLAGS = BASE_FLAGS + ["-O1", "-ffp-contract=off"]
# gcc forms fused multiply-adds in a pass that -O1 does not run: -O2, or the "FMA build" would hold none
FLAGS_FMA = BASE_FLAGS + ["-O2", "-mfma", "-ffp-contract=fast"]

_LAUNCH = re.compile(r"(\w+<scalar_t>)\s*<<<([^<>]*)>>>\s*\(")
_SHARED = re.compile(r"extern\s+__shared__\s+(?:__align__\([^;\[]*\)\s+)?([\w ]+?)\s+(\w+)\s*\[\s*\]\s*;")


def reference_dir() -> str:
    return os.environ.get("STEREO_REFERENCE_DIR", "/root/reference")


def available() -> bool:
    return os.path.isfile(os.path.join(reference_dir(), "src", "csrc", "depth", "stereo_matching.cc"))


def rewrite(text: str, launches: int, shared: int, name: str) -> str:
    text, n = _LAUNCH.subn(r"refhost::launch(refhost::launch_cfg(\2), \1, ", text)
    if n != launches or "<<<" in text or ">>>" in text:
        raise RuntimeError(f"build_ref: {name}: {n} kernel launches rewritten, {launches} expected (or one left over)")
    text, n = _SHARED.subn(r"\1* \2 = static_cast<\1*>(refhost::block_shared());", text)
    if n != shared or "__shared__" in text:
        raise RuntimeError(f"build_ref: {name}: {n} shared-memory declarations rewritten, {shared} expected (or one left over)")
    return text


def has_fma() -> bool:
    try:
        with open("/proc/cpuinfo") as f:
            return " fma " in f.read().replace("\n", " ")
    except OSError:
        return False


def _stamp(texts) -> str:
    h = hashlib.sha256()
    for rel in sorted(texts):
        h.update(rel.encode() + b"\0" + texts[rel].encode() + b"\0")
    for n in OWN + HEADERS:
        with open(os.path.join(HOST, n), "rb") as f:
            h.update(n.encode() + b"\0" + f.read() + b"\0")
    h.update(" ".join(FLAGS + FLAGS_FMA).encode())
    return h.hexdigest()


def build(force: bool = False) -> str:
    """Writes oracle/_ref/src and compiles oracle/_ref/libref_host.so (and _fma.so where the CPU has FMA).
    Returns the path of libref_host.so.  No-op when the inputs have not changed."""
    if not available():
        raise RuntimeError(f"build_ref: no reference tree at {reference_dir()} (set STEREO_REFERENCE_DIR)")
    root = os.path.join(reference_dir(), "src", "csrc")
    texts = {}
    for rel, counts in SOURCES.items():
        with open(os.path.join(root, rel)) as f:
            text = f.read()
        if counts is None:
            if "<<<" in text or "__shared__" in text:
                raise RuntimeError(f"build_ref: {rel}: holds a launch or a shared-memory declaration but is listed as plain")
            texts[rel] = text
        else:
            texts[rel] = rewrite(text, counts[0], counts[1], rel)
    stamp = _stamp(texts)
    stamp_file = os.path.join(OUT, "stamp")
    wanted = [LIB] + ([LIB_FMA] if has_fma() else [])
    if not force and all(os.path.exists(p) for p in wanted) and os.path.exists(stamp_file):
        with open(stamp_file) as f:
            if f.read().strip() == stamp:
                return LIB
    src = os.path.join(OUT, "src")
    shutil.rmtree(src, ignore_errors=True)
    for rel, text in texts.items():
        os.makedirs(os.path.dirname(os.path.join(src, rel)), exist_ok=True)
        with open(os.path.join(src, rel), "w") as f:
            f.write(text)
    units = [os.path.join(HOST, n) for n in OWN] + [os.path.join(src, rel) for rel in SOURCES if rel.endswith((".cc", ".cu"))]
    cxx = os.environ.get("CXX", "g++")
    for lib, flags in ((LIB, FLAGS), (LIB_FMA, FLAGS_FMA)):
        if lib not in wanted:
            continue
        cmd = [cxx] + flags + ["-I", HOST, "-I", src, "-o", lib + ".tmp", "-x", "c++"] + units
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode:
            raise RuntimeError("build_ref: " + " ".join(cmd) + "\n" + r.stdout + r.stderr)
        os.replace(lib + ".tmp", lib)
    with open(stamp_file, "w") as f:
        f.write(stamp + "\n")
    return LIB


class RefHost:
    """ctypes wrapper over a built oracle/_ref/libref_host*.so (never builds; `built()` says whether it is there)."""

    STAGES = ("out", "gray_left", "down_left", "wta", "refined", "agg_volume")

    def __init__(self, fma: bool = False):
        import ctypes as C
        self.C = C
        self.lib = C.CDLL(LIB_FMA if fma else LIB)
        fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
        self.fp = fp
        self.lib.ref_host_run.argtypes = [ip, fp, fp, C.c_int, C.c_float, C.c_int] + [fp] * 6
        self.lib.ref_host_run.restype = C.c_int
        self.lib.ref_host_dims.argtypes = [ip, ip]
        self.lib.ref_host_dims.restype = None
        self.lib.ref_host_selfcheck_barrier.argtypes = [C.c_int] * 5 + [C.c_float, C.c_int, fp]
        self.lib.ref_host_selfcheck_barrier.restype = C.c_int
        self.lib.ref_host_selfcheck_read.argtypes = [C.c_int, C.c_int, C.c_int32, C.c_int32, C.c_float]
        self.lib.ref_host_selfcheck_read.restype = C.c_float
        self.lib.ref_host_selfcheck_types.restype = C.c_int

    @staticmethod
    def built(fma: bool = False) -> bool:
        return os.path.exists(LIB_FMA if fma else LIB)

    # the reference's defaults of the six fields after max_disparity (stereo_matching_configuration.hh:11-16)
    DEFAULTS = (1, 5, 5, 1, 4, 10)

    def run(self, config, left, right, poison: float = 0.0, reverse: bool = False):
        """config = [H, W, K, min_disparity, max_disparity] (the reference's defaults for the rest) or all eleven fields
        in the order of stereo_matching_configuration.hh: ... ncc_patch_radius, sad_patch_radius, threshold,
        small_mbm_radius, mid_mbm_radius, large_mbm_radius.  left/right float32 [3,H,W] or [H,W].
        Returns a dict of the arrays named in STAGES."""
        import numpy as np
        C = self.C
        config = [int(v) for v in config]
        if len(config) == 5:
            config += self.DEFAULTS
        if len(config) != 11:
            raise RuntimeError(f"ref_host: a configuration has 5 or 11 entries, not {len(config)}")
        if min(config[5:]) < 0:
            raise RuntimeError(f"ref_host: negative radius or threshold in {config[5:]}")
        if config[8] > config[10] or config[9] > config[10]:
            # the aggregation tile is sized by the large radius: the reference's own text indexes past it (and crashes)
            raise RuntimeError(f"ref_host: small_mbm_radius {config[8]} / mid_mbm_radius {config[9]} above "
                               f"large_mbm_radius {config[10]}")
        cfg = np.ascontiguousarray(config, np.int32)
        H, W = int(cfg[0]), int(cfg[1])
        left = np.ascontiguousarray(left, np.float32)
        right = np.ascontiguousarray(right, np.float32)
        rgb = left.ndim == 3
        if left.shape != ((3, H, W) if rgb else (H, W)) or right.shape != left.shape:
            raise RuntimeError(f"ref_host: input shape {left.shape} / {right.shape} does not fit {H}x{W}")
        hwd = np.zeros(3, np.int32)
        ip = C.POINTER(C.c_int32)
        self.lib.ref_host_dims(cfg.ctypes.data_as(ip), hwd.ctypes.data_as(ip))
        h, w, Dd = (int(v) for v in hwd)
        shapes = dict(out=(H, W), gray_left=(H, W), down_left=(h, w), wta=(h, w), refined=(h, w), agg_volume=(h, w, Dd))
        got = {k: np.empty(shapes[k], np.float32) for k in self.STAGES}
        rc = self.lib.ref_host_run(cfg.ctypes.data_as(ip), left.ctypes.data_as(self.fp), right.ctypes.data_as(self.fp),
                                   int(rgb), float(poison), int(reverse), *[got[k].ctypes.data_as(self.fp) for k in self.STAGES])
        if rc:
            raise RuntimeError(f"ref_host: run failed (code {rc})")
        return got


if __name__ == "__main__":
    print(build(force="--force" in sys.argv))
