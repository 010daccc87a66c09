"""Merging TSDF volumes without a GPU: smx_tsdf_merge (include/stereo_mi355x.h) is declared and exported with its signature
and refuses every bad argument before a device is touched, in the documented order; the ownership of spill boxes and
the subtraction of boxes against boolean masks; cuda_depth.TSDFSpillStore driven on the NumPy volume of
tests/tsdf_merge_ref.py (out and back, a seeded walk, eviction); the Python-level errors of TSDFVolume.merge, of the
store and of the pipeline's keyword."""
import ctypes as C
import dataclasses
import inspect
import itertools
import math
import os
import re

import numpy as np
import pytest

import tsdf_merge_ref as mref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "stereo_mi355x.h")
NAME = "smx_tsdf_merge"


@pytest.fixture(scope="module")
def cd():
    import cuda_depth
    return cuda_depth


@pytest.fixture(scope="module")
def native():
    import cuda_depth._native as native
    return native


# ---- the C ABI --------------------------------------------------------------------------------------------------------------

def test_symbol_is_declared_and_exported(native):
    text = open(HEADER).read()
    assert re.search(r"\bint " + NAME + r"\(", text)
    assert NAME in text.split("Conventions")[0], "missing from the header's list of entry points"
    assert re.search(r"\bT " + NAME + r"\b", os.popen(f"nm -D --defined-only {native.LIB_PATH}").read())
    restype, argtypes = native.EXPORTS[NAME]
    p, i, f = C.c_void_p, C.c_int, C.c_float
    assert restype is C.c_int
    assert argtypes == [i, i, i, i, p, p, p, i, i, i, p, p, p, i, i, i, i, i, i, i, i, i, i, f, p]
    fn = getattr(native.LIB, NAME)
    assert fn.restype is C.c_int and list(fn.argtypes) == argtypes
    decl = re.search(r"\bint " + NAME + r"\((.*?)\);", text, flags=re.S).group(1)
    names = [re.sub(r".*[ *]", "", part.strip()) for part in decl.split(",")]
    assert names == ["device_id", "nx", "ny", "nz", "tsdf", "weight", "color", "sx", "sy", "sz", "src_tsdf", "src_weight",
                     "src_color", "x0", "y0", "z0", "rx", "ry", "rz", "cx", "cy", "cz", "mode", "max_weight", "stream"]
    assert re.search(r"#define SMX_TSDF_MERGE_FILL\s+0\b", text) and re.search(r"#define SMX_TSDF_MERGE_AVERAGE\s+1\b", text)
    assert native.TSDF_MERGE_MODES == {"fill": 0, "average": 1}
    assert native.LIB.smx_abi_version() == 4


def test_bad_arguments_are_refused_before_the_device(native):
    import torch
    lib, bad = native.LIB, -1                                         # SMX_ERR_INVALID_ARG

    def p(addr):
        return C.c_void_p(addr)

    # destination 16 x 12 x 10 (7680 bytes per array), source 8 x 6 x 5 (960 bytes per array); invented addresses
    def call(**kw):
        a = dict(dev=0, nx=16, ny=12, nz=10, tsdf=p(0x2000000), weight=p(0x3000000), color=p(0x4000000), sx=8, sy=6, sz=5,
                 src_tsdf=p(0x6000000), src_weight=p(0x7000000), src_color=p(0x8000000), x0=-3, y0=2, z0=7, rx=1, ry=0,
                 rz=2, cx=7, cy=6, cz=3, mode=1, max_weight=64.0, stream=None)
        a.update(kw)
        return lib.smx_tsdf_merge(*a.values())

    if not torch.cuda.is_available():            # a valid call stops at the device; with one it would run on these addresses
        assert call() == -3 and "cannot select HIP device" in native.last_error()
        assert call(color=None, src_color=None) == -3
        assert call(mode=0) == -3
        assert call(x0=8192, y0=-8192, z0=8192) == -3               # a region that misses the destination is valid
        assert call(rx=0, ry=0, rz=0, cx=8, cy=6, cz=5) == -3 and call(rx=7, ry=5, rz=4, cx=1, cy=1, cz=1) == -3
        assert call(nx=4096, ny=4096, nz=64, tsdf=p(1 << 40), weight=p(2 << 40), color=p(3 << 40)) == -3
        # operands just clear of each other
        assert call(src_tsdf=p(0x2000000 + 7680), src_weight=p(0x2000000 - 960), src_color=p(0x6000000 + 960)) == -3
    inf, nan = math.inf, math.nan
    broken = dict(
        null=[dict(tsdf=None), dict(weight=None), dict(src_tsdf=None), dict(src_weight=None)],
        colour=[dict(color=None), dict(src_color=None)],
        destination_dims=[dict(nx=0), dict(ny=4097), dict(nz=-1), dict(nx=4096, ny=4096, nz=65),
                          dict(nx=1025, ny=1024, nz=1024)],
        source_dims=[dict(sx=0), dict(sy=4097), dict(sz=-1), dict(sx=4096, sy=4096, sz=65), dict(sx=1024, sy=1025, sz=1024)],
        placement=[dict(x0=8193), dict(x0=-8193), dict(y0=8193), dict(y0=-8193), dict(z0=8193), dict(z0=-(2 ** 31))],
        region=[dict(rx=-1), dict(ry=-1), dict(rz=-1), dict(cx=0), dict(cy=0), dict(cz=-2), dict(rx=2), dict(ry=1),
                dict(rz=3), dict(cx=8), dict(cz=4), dict(rx=2 ** 31 - 1), dict(cx=2 ** 31 - 1)],
        mode=[dict(mode=2), dict(mode=-1)],
        max_weight=[dict(max_weight=0.0), dict(max_weight=-1.0), dict(max_weight=inf), dict(max_weight=nan),
                    dict(max_weight=0.0, mode=0), dict(max_weight=nan, mode=0)],
        overlaps=[dict(src_tsdf=p(0x2000000)), dict(src_tsdf=p(0x2000000 + 7676)), dict(src_weight=p(0x3000000 - 956)),
                  dict(src_color=p(0x4000000 + 100)), dict(src_weight=p(0x2000000 + 7679)),
                  dict(weight=p(0x2000000 + 7676)), dict(color=p(0x3000000 - 7679)), dict(color=p(0x2000000)),
                  dict(tsdf=p(0x6000000), src_tsdf=p(0x6000000))],
        stream=[dict(stream=native.STREAM_ENGINE)])
    for rule, cases in broken.items():
        for kw in cases:
            assert call(**kw) == bad, (rule, kw)
            assert NAME in native.last_error(), (rule, kw, native.last_error())
    for kw, word in ((dict(tsdf=None), "non-NULL"), (dict(src_color=None), "both"), (dict(nx=0), "nx, ny, nz"),
                     (dict(sz=0), "sx, sy, sz"), (dict(x0=9000), "x0"), (dict(y0=-9000), "y0"), (dict(z0=9000), "z0"),
                     (dict(rx=-1), "region"), (dict(mode=7), "mode"), (dict(max_weight=nan), "max_weight"),
                     (dict(src_tsdf=p(0x3000000)), "source array"), (dict(color=p(0x3000000 + 4)), "destination arrays"),
                     (dict(stream=native.STREAM_ENGINE), "stream")):
        assert call(**kw) == bad and word in native.last_error(), (kw, native.last_error())
    # the order of the rules: the earlier one answers a doubly wrong call
    assert call(weight=None, color=None) == bad and "non-NULL" in native.last_error()
    assert call(color=None, nx=0) == bad and "both" in native.last_error()
    assert call(nx=0, sx=0) == bad and "nx, ny, nz" in native.last_error()
    assert call(sx=0, x0=9000) == bad and "sx, sy, sz" in native.last_error()
    assert call(z0=9000, rx=-1) == bad and "z0" in native.last_error()
    assert call(cx=0, mode=5) == bad and "region" in native.last_error()
    assert call(mode=5, max_weight=0.0) == bad and "mode" in native.last_error()
    assert call(max_weight=0.0, src_tsdf=p(0x2000000)) == bad and "max_weight" in native.last_error()
    assert call(src_tsdf=p(0x2000000), stream=native.STREAM_ENGINE) == bad and "source array" in native.last_error()


# ---- boxes ------------------------------------------------------------------------------------------------------------------

def box_mask(shape_xyz, box, base=(0, 0, 0)):
    """[nz, ny, nx] mask of the integer box (start, dims) inside a grid whose first voxel is `base`."""
    nx, ny, nz = shape_xyz
    m = np.zeros((nz, ny, nx), bool)
    lo = [max(0, s - b) for s, b in zip(box[0], base)]
    hi = [min(n, s - b + d) for n, s, b, d in zip(shape_xyz, box[0], base, box[1])]
    if all(l < h for l, h in zip(lo, hi)):
        m[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]] = True
    return m


@pytest.mark.parametrize("d", [(0, 0, 2), (-3, 0, 0), (2, -1, 0), (1, 1, -1), (13, 0, -5), (-40, 3, 0), (12, -6, 4)])
@pytest.mark.parametrize("margin", [0, 1, 2, 9])
@pytest.mark.parametrize("dims", [(13, 7, 5), (24, 16, 20)])
def test_ownership_partitions_what_leaves(cd, dims, margin, d):
    boxes = cd.tsdf_spill_boxes(dims, d, margin)
    owned = cd.tsdf_spill_ownership(dims, d)
    assert len(owned) == len(boxes) == sum(c != 0 for c in d)
    nx, ny, nz = dims
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    stays = np.ones((nz, ny, nx), bool)
    for idx, n, c in ((i, nx, d[0]), (j, ny, d[1]), (k, nz, d[2])):
        stays &= (idx - c >= 0) & (idx - c < n)
    count = np.zeros((nz, ny, nx), int)
    for box, own in zip(boxes, owned):
        if own is None:
            continue
        assert all(n >= 1 for n in own[1])
        own_mask = box_mask(dims, own)
        assert own_mask.sum() == np.prod(own[1]), "the owned region must lie inside the volume"
        assert not (own_mask & ~box_mask(dims, box)).any(), "the owned region must lie inside its box"
        count += own_mask
    assert count.max() <= 1, "owned regions overlap"
    assert np.array_equal(count == 1, ~stays), "the owned regions are not exactly the voxels that leave"
    for box, own in zip(boxes, owned):
        if own is None:                                              # nothing of this box is left to own
            others = sum(box_mask(dims, o) for o in owned if o is not None)
            assert not (box_mask(dims, box) & ~stays & (others == 0)).any()


def test_ownership_arguments(cd):
    assert cd.tsdf_spill_ownership((8, 8, 8), (0, 0, 0)) == []
    assert cd.tsdf_spill_ownership((8, 8, 8), (3, 0, 0)) == [((0, 0, 0), (3, 8, 8))]
    assert cd.tsdf_spill_ownership((8, 8, 8), (2, -3, 0)) == [((0, 0, 0), (2, 8, 8)), ((2, 5, 0), (6, 3, 8))]
    assert cd.tsdf_spill_ownership((8, 8, 8), (8, 1, 0)) == [((0, 0, 0), (8, 8, 8)), None]
    with pytest.raises(TypeError):
        cd.tsdf_spill_ownership((8, 8, 8), (1.0, 0, 0))


SUBTRACT_CASES = [
    # (a, b)
    (((0, 0, 0), (6, 5, 4)), ((1, 1, 1), (3, 2, 2))),                # nested: six pieces
    (((0, 0, 0), (6, 5, 4)), ((0, 0, 0), (6, 5, 4))),                # equal: nothing left
    (((1, 1, 1), (3, 2, 2)), ((0, 0, 0), (6, 5, 4))),                # a inside b
    (((0, 0, 0), (3, 3, 3)), ((5, 5, 5), (2, 2, 2))),                # disjoint
    (((0, 0, 0), (3, 3, 3)), ((3, 0, 0), (2, 3, 3))),                # touching at a face
    (((0, 0, 0), (6, 5, 4)), ((4, -1, -1), (9, 9, 9))),              # cut by one plane
    (((0, 0, 0), (6, 5, 4)), ((-2, -2, -2), (5, 9, 9))),             # one plane, from the other side
    (((0, 0, 0), (6, 5, 4)), ((2, 3, -1), (9, 9, 9))),               # two planes
    (((0, 0, 0), (6, 5, 4)), ((2, 1, -5), (2, 3, 20))),              # a bar through it: four pieces
    (((0, 0, 0), (6, 5, 4)), ((3, 2, 1), (9, 9, 9))),                # three planes: a corner
    (((-4, 2, 7), (6, 5, 4)), ((-5, 3, 8), (4, 9, 2))),              # negative coordinates
]


@pytest.mark.parametrize("a,b", SUBTRACT_CASES)
def test_box_subtraction_against_masks(cd, a, b):
    base, shape = (-6, -3, -6), (22, 16, 24)
    pieces = cd.tsdf_box_subtract(a, b)
    assert len(pieces) <= 6
    total = np.zeros(shape[::-1], int)
    for piece in pieces:
        assert all(n >= 1 for n in piece[1])
        mask = box_mask(shape, piece, base)
        assert mask.sum() == np.prod(piece[1])
        total += mask
    assert total.max() <= 1, "pieces overlap"
    assert np.array_equal(total == 1, box_mask(shape, a, base) & ~box_mask(shape, b, base))
    inter = cd.tsdf_box_intersect(a, b)
    want = box_mask(shape, a, base) & box_mask(shape, b, base)
    assert (inter is None) == (not want.any())
    if inter is not None:
        assert np.array_equal(box_mask(shape, inter, base), want)


# ---- the store on the NumPy volume ----------------------------------------------------------------------------------------

DIMS = (13, 7, 5)


def plausible_state(rng, dims=DIMS, colour=True, measured=0.6):
    return mref.plausible_state(rng, dims, colour, measured)


def assert_same_state(got, want, what):
    for k in ("tsdf", "weight", "color"):
        if want[k] is None:
            assert got[k] is None
            continue
        bad = np.argwhere(got[k] != want[k])
        assert bad.size == 0, f"{what}: {k}: {len(bad)} words differ, first at (k, j, i) = {tuple(bad[0])}"


OUT_AND_BACK, full_path = mref.OUT_AND_BACK, mref.full_path


@pytest.mark.parametrize("margin", [0, 1, 2])
@pytest.mark.parametrize("steps", OUT_AND_BACK)
@pytest.mark.parametrize("colour", [True, False])
def test_store_out_and_back(cd, colour, steps, margin):
    rng = np.random.default_rng(5 + margin)
    first = plausible_state(rng, colour=colour)
    vol = mref.NumpyVolume(first)
    store = cd.TSDFSpillStore()
    held, restored = 0, 0
    for d in full_path(steps):
        boxes, n = store.shift(vol, d, margin=margin)
        assert len(boxes) == sum(c != 0 for c in d) and n == vol.merges - restored
        restored = vol.merges
        held = max(held, len(store))
    assert held >= 1 and restored >= 1
    assert vol.offset == (0, 0, 0)
    assert_same_state(vol.state, first, f"{steps} margin {margin}")
    assert len(store) == 0 and store.bytes == 0 and store.volumes() == [] and store.evicted == 0


def world_mask(region, base, shape):
    return box_mask(shape, region, base)


def test_store_seeded_walk(cd):
    rng = np.random.default_rng(41)
    first = plausible_state(rng)
    vol = mref.NumpyVolume(first)
    store = cd.TSDFSpillStore()
    base, shape = (-40, -40, -40), (93, 87, 85)                       # world voxels the walk can reach
    first_measured = box_mask(shape, ((0, 0, 0), DIMS), base)
    first_measured[first_measured] = (first["weight"].view(np.float32) > 0).reshape(-1)
    for step in range(200):
        d = tuple(int(c) for c in rng.integers(-4, 5, 3) * (rng.random(3) < 0.6))
        target = [o + c for o, c in zip(vol.offset, d)]
        d = tuple(c if abs(t) <= 24 else 0 for c, t in zip(d, target))   # stay inside the mask
        store.shift(vol, d, margin=int(rng.integers(0, 3)))
        live = box_mask(shape, (vol.offset, DIMS), base)
        count = np.zeros(shape[::-1], int)
        for box, regions in zip(store.volumes(), store.owned_regions()):
            assert regions, "an entry that owns nothing must be dropped"
            for region in regions:
                m = box_mask(shape, region, base)
                assert m.sum() == np.prod(region[1])
                assert not (m & ~box_mask(shape, (box.offset, box.dims), base)).any(), "owned outside its box"
                count += m
        assert count.max() <= 1, f"step {step}: owned regions overlap"
        assert not ((count > 0) & live).any(), f"step {step}: an owned region lies inside the live window"
        away = first_measured & ~live
        assert (count[away] == 1).all(), f"step {step}: a measured voxel that left is held by no entry"
        # what is inside the window of the first state is there bit for bit (nothing else was ever measured)
        here = first_measured & live
        got = np.zeros(shape[::-1], np.uint32)
        got[live] = vol.state["weight"].reshape(-1)
        want = np.zeros(shape[::-1], np.uint32)
        want[box_mask(shape, ((0, 0, 0), DIMS), base)] = first["weight"].reshape(-1)
        assert np.array_equal(got[here], want[here]), f"step {step}"
    assert len(store) >= 1
    store.shift(vol, tuple(-c for c in vol.offset))
    assert_same_state(vol.state, first, "the walk home")
    assert len(store) == 0 and store.bytes == 0


def test_store_eviction(cd):
    rng = np.random.default_rng(43)
    first = plausible_state(rng, measured=1.0)
    vol = mref.NumpyVolume(first)
    box_bytes = 2 * 7 * 5 * 12                                       # an x box of 1 leaving + 1 margin layer, with colour
    store = cd.TSDFSpillStore(max_bytes=2 * box_bytes)
    for k in range(2):
        store.shift(vol, (1, 0, 0))
        assert len(store) == k + 1 and store.bytes == (k + 1) * box_bytes and store.evicted == 0
    oldest = store.volumes()[0]
    store.shift(vol, (1, 0, 0))                                       # the third box does not fit: the oldest goes
    assert len(store) == 2 and store.bytes == 2 * box_bytes and store.evicted == 1
    assert oldest not in store.volumes() and [b.offset for b in store.volumes()] == [(1, 0, 0), (2, 0, 0)]
    _, restored = store.shift(vol, (-3, 0, 0))
    assert restored == 2 and len(store) == 0
    want = {k: v.copy() for k, v in first.items()}
    for v in want.values():
        v[:, :, 0] = 0                                                # the evicted layer is gone
    assert_same_state(vol.state, want, "after an eviction")
    tiny = cd.TSDFSpillStore(max_bytes=0)
    tiny.shift(vol, (2, 0, 0))
    assert len(tiny) == 0 and tiny.evicted == 1 and tiny.bytes == 0


def test_store_follow_uses_follows_arithmetic(cd):
    rng = np.random.default_rng(47)
    vol = mref.NumpyVolume(plausible_state(rng, (48, 32, 48)), voxel_size=0.125)
    store = cd.TSDFSpillStore()
    pose = np.eye(4)
    pose[:3, 3] = (3.0 + 3 * 0.125, 2.0, 3.0)                       # below the default threshold of 4
    assert store.follow(vol, pose) == ((0, 0, 0), [], 0) and vol.offset == (0, 0, 0)
    pose[:3, 3] = (3.0 + 4 * 0.125, 2.0 - 0.125, 3.0)
    d, boxes, restored = store.follow(vol, pose)
    assert d == (4, -1, 0) and len(boxes) == 2 and restored == 0 and vol.offset == (4, -1, 0) and len(store) == 2
    d, boxes, restored = store.follow(vol, pose, threshold=1)
    assert d == (0, 0, 0)
    pose[:3, 3] = (3.0, 2.0, 3.0)
    d, boxes, restored = store.follow(vol, pose, threshold=1, margin=0)
    assert d == (-4, 1, 0) and restored == 2 and len(store) == 0    # what entered on the way out was never measured
    for exc, kw in ((TypeError, dict(threshold=2.0)), (RuntimeError, dict(threshold=0)), (TypeError, dict(anchor=0.5))):
        with pytest.raises(exc):
            store.follow(vol, pose, **kw)


def test_returning_camera_path_on_the_twins(cd):
    """The path of the device test (tests/tsdf_return_cases.py) meets its conditions on the twins, and the comparison
    bites: without the store the voxels that left come back empty."""
    import tsdf_return_cases as rc
    compared, returned = rc.compare(*rc.simulate(cd))
    assert compared >= 0.25 * np.prod(rc.SMALL_DIMS) and returned >= 500
    with pytest.raises(AssertionError, match="differ from the fixed volume"):
        rc.compare(*rc.simulate(cd, with_store=False))


# ---- Python errors --------------------------------------------------------------------------------------------------------

def test_store_errors(cd):
    rng = np.random.default_rng(53)
    store = cd.TSDFSpillStore()
    vol = mref.NumpyVolume(plausible_state(rng))
    store.shift(vol, (1, 0, 0))
    for kw in (dict(voxel_size=0.25), dict(origin=(0.125, 0.0, 0.0)), dict(max_weight=8.0), dict(truncation=0.75),
               dict(device="elsewhere")):
        with pytest.raises(RuntimeError, match="one volume"):
            store.shift(mref.NumpyVolume(plausible_state(rng), **kw), (1, 0, 0))
    with pytest.raises(RuntimeError, match="one volume"):
        store.shift(mref.NumpyVolume(plausible_state(rng, colour=False)), (1, 0, 0))
    with pytest.raises(TypeError, match="voxels"):
        store.shift(vol, (1.0, 0, 0))
    with pytest.raises(RuntimeError, match="8192"):
        store.shift(vol, (9000, 0, 0))
    with pytest.raises(TypeError, match="max_bytes"):
        cd.TSDFSpillStore(max_bytes=1.5)
    with pytest.raises(RuntimeError, match="max_bytes"):
        cd.TSDFSpillStore(max_bytes=-1)
    assert store.shift(vol, (0, 0, 0)) == ([], 0)
    sig = inspect.signature(cd.TSDFSpillStore.shift)
    assert [(n, q.default) for n, q in sig.parameters.items() if q.kind is q.KEYWORD_ONLY] == [("margin", 1)]
    sig = inspect.signature(cd.TSDFSpillStore.follow)
    assert {n: q.default for n, q in sig.parameters.items() if q.kind is q.KEYWORD_ONLY} == dict(
        threshold=None, anchor=(0.5, 0.5, 0.5), margin=1)
    assert inspect.signature(cd.TSDFSpillStore.__init__).parameters["max_bytes"].default is None


def host_volume(cd, dims=(16, 12, 10), vs=0.125, origin=(0.0, 0.0, 0.0), colour=True, **kw):
    """TSDFVolume's host side alone: enough for merge's checks, which come before the device is touched."""
    vol = object.__new__(cd.TSDFVolume)
    vol.dims, vol.voxel_size, vol.origin = dims, vs, origin
    vol.truncation, vol.max_weight, vol.device = kw.get("truncation", 0.5), kw.get("max_weight", 64.0), kw.get("device", "cuda:0")
    vol.color = object() if colour else None
    vol.tsdf = vol.weight = None
    return vol


def test_merge_errors(cd):
    a = host_volume(cd)
    with pytest.raises(TypeError, match="TSDFVolume"):
        a.merge("volume")
    with pytest.raises(RuntimeError, match="itself"):
        a.merge(a)
    with pytest.raises(RuntimeError, match="mode"):
        a.merge(host_volume(cd), mode="max")
    for name, kw in (("voxel_size", dict(vs=0.25)), ("truncation", dict(truncation=0.75)),
                     ("max_weight", dict(max_weight=8.0)), ("device", dict(device="cuda:1"))):
        with pytest.raises(RuntimeError, match=name):
            a.merge(host_volume(cd, **kw))
    with pytest.raises(RuntimeError, match="colour"):
        a.merge(host_volume(cd, colour=False))
    with pytest.raises(RuntimeError, match="whole"):
        a.merge(host_volume(cd, origin=(0.0625, 0.0, 0.0)))
    with pytest.raises(RuntimeError, match="whole"):
        a.merge(host_volume(cd, origin=(0.0, 0.0, 1.0 + 2.0 ** -40)))
    b = host_volume(cd, dims=(8, 6, 5))
    for region in (7, ((0, 0, 0),), ((0, 0), (1, 1, 1)), ((0, 0, 0), (1.0, 1, 1))):
        with pytest.raises(TypeError, match="region"):
            a.merge(b, region=region)
    for region in (((-1, 0, 0), (1, 1, 1)), ((0, 0, 0), (0, 1, 1)), ((0, 0, 0), (9, 1, 1)), ((7, 5, 4), (1, 1, 2))):
        with pytest.raises(RuntimeError, match="region"):
            a.merge(b, region=region)
    far = host_volume(cd, origin=(0.125 * 9000, 0.0, 0.0))
    with pytest.raises(RuntimeError, match="8192"):
        a.merge(far)
    sig = inspect.signature(cd.TSDFVolume.merge)
    assert list(sig.parameters) == ["self", "other", "mode", "region"]
    assert {n: q.default for n, q in sig.parameters.items() if q.kind is q.KEYWORD_ONLY} == dict(mode="average", region=None)
    assert "TSDFSpillStore" in cd.TSDFVolume.shift.__doc__


def test_pipeline_keyword_and_result_field():
    import pipeline
    sig = inspect.signature(pipeline.DepthEstimationPipeline.__init__)
    assert sig.parameters["spill_store"].default is None
    fields = {f.name: f for f in dataclasses.fields(pipeline.DepthEstimationResult)}
    assert fields["restored_boxes"].kw_only and fields["restored_boxes"].default == 0
    names = list(fields)
    assert names[-1] == "confidence_map" and names.index("restored_boxes") == names.index("spilled_volumes") + 1
    import cuda_depth
    cfg = pipeline.DepthEstimationPipelineConfig(image_shape=(32, 48), min_disparity=0, max_disparity=15)
    with pytest.raises(ValueError, match="follow_camera"):
        pipeline.DepthEstimationPipeline(cfg, spill_store=cuda_depth.TSDFSpillStore())
    with pytest.raises(TypeError, match="spill_store"):
        pipeline.DepthEstimationPipeline(cfg, spill_store=[])


def test_twin_restates_the_rule():
    """The twin on hand-made pairs: the skip, the copy, FILL, and AVERAGE's arithmetic against exact rationals."""
    from fractions import Fraction
    f = lambda v: np.array([v], np.float32).view(np.uint32)[0]    # noqa: E731
    nan_w, nan_t = np.uint32(0x7FC00123), np.uint32(0xFFC00001)
    dst = (f(0.25), f(2.0), np.uint32(0x11223344))
    for mode in (mref.FILL, mref.AVERAGE):
        for w1 in (f(0.0), f(-0.0), f(-3.0), nan_w):                  # skipped: the destination's bits stay
            assert mref.merge_pair(*dst, nan_t, w1, np.uint32(0xFFFFFFFF), mode, 64.0) == dst
        for w0 in (f(0.0), f(-0.0), f(-1.0), nan_w):                  # copied bit for bit, the fourth byte included
            got = mref.merge_pair(nan_t, w0, np.uint32(5), nan_t, f(1e-30), np.uint32(0xAB000001), mode, 64.0)
            assert got == (nan_t, f(1e-30), np.uint32(0xAB000001))
    src = (f(-0.5), f(1.0), np.uint32(0xFF0A6400))
    assert mref.merge_pair(*dst, *src, mref.FILL, 64.0) == dst
    t, w, c = mref.merge_pair(*dst, *src, mref.AVERAGE, 2.5)
    assert w == f(2.5)                                               # the cap binds: 2 + 1 > 2.5
    assert t == f(float((Fraction(0.25) * 2 + Fraction(-0.5)) / 3))
    want = [math.floor((Fraction(a) * 2 + Fraction(b)) / 3 + Fraction(1, 2)) for a, b in ((0x44, 0x00), (0x33, 0x64), (0x22, 0x0A))]
    assert [int(c) & 255, (int(c) >> 8) & 255, (int(c) >> 16) & 255, int(c) >> 24] == want + [0]
    assert mref.merge_pair(*dst[:2], None, *src[:2], None, mref.AVERAGE, 64.0) == (t, f(3.0), None)
    # merge_ref, whole arrays at a time, against merge_pair pair by pair
    rng = np.random.default_rng(59)
    weights = np.array([0.0, -0.0, 1.0, 2.5, 3.0, -2.0, np.nan], np.float32).view(np.uint32)

    def state(dims):
        shape = dims[::-1]
        return {"tsdf": rng.uniform(-1, 1, shape).astype(np.float32).view(np.uint32), "weight": rng.choice(weights, shape),
                "color": rng.integers(0, 2 ** 24, shape).astype(np.uint32)}
    d, s = state((6, 5, 4)), state((5, 3, 4))
    for mode, placement, region in itertools.product((mref.FILL, mref.AVERAGE), ((0, 0, 0), (3, -1, 2), (-2, 3, -1)),
                                                     (None, ((1, 0, 1), (3, 2, 2)))):
        out = mref.merge_ref(d, s, placement, region, mode, 3.0)
        (rx, ry, rz), (cx, cy, cz) = region or ((0, 0, 0), (5, 3, 4))
        want = {k: v.copy() for k, v in d.items()}
        for k, j, i in itertools.product(range(rz, rz + cz), range(ry, ry + cy), range(rx, rx + cx)):
            x, y, z = i + placement[0], j + placement[1], k + placement[2]
            if 0 <= x < 6 and 0 <= y < 5 and 0 <= z < 4:
                want["tsdf"][z, y, x], want["weight"][z, y, x], want["color"][z, y, x] = mref.merge_pair(
                    d["tsdf"][z, y, x], d["weight"][z, y, x], d["color"][z, y, x], s["tsdf"][k, j, i],
                    s["weight"][k, j, i], s["color"][k, j, i], mode, 3.0)
        assert_same_state(out, want, f"mode {mode} at {placement} region {region}")
    # merge_ref: placement, region and clipping on a tiny case
    d = {"tsdf": np.zeros((1, 1, 4), np.uint32), "weight": np.zeros((1, 1, 4), np.uint32), "color": None}
    s = {"tsdf": np.full((1, 1, 3), f(0.5), np.uint32), "weight": np.full((1, 1, 3), f(1.0), np.uint32), "color": None}
    for placement, region, want in (((0, 0, 0), None, [1, 1, 1, 0]), ((2, 0, 0), None, [0, 0, 1, 1]),
                                    ((-2, 0, 0), None, [1, 0, 0, 0]), ((1, 0, 0), ((1, 0, 0), (1, 1, 1)), [0, 0, 1, 0]),
                                    ((4, 0, 0), None, [0, 0, 0, 0]), ((0, 1, 0), None, [0, 0, 0, 0])):
        out = mref.merge_ref(d, s, placement, region, "fill", 64.0)
        assert (out["weight"][0, 0] != 0).astype(int).tolist() == want, (placement, region)
        assert not d["weight"].any(), "merge_ref must not modify its inputs"
