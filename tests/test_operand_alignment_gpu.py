"""Operands that are aligned to their element type and no further (include/stereo_mi355x.h: conventions, Alignment).

A contiguous view into a larger buffer is an ordinary operand: frame k of a uint8 batch whose H*W is odd, a map cut out
of a ring buffer.  Several launchers pick a vector or a scalar form from the addresses they are given (tu_lr.hip,
tu_stages.hip, tu_remap.hip) and some kernels make 16-byte copies from 4-byte aligned addresses (k_prologue.h, k_fill.h);
the other map kernels make scalar accesses today, and their cases here are a tripwire for the day one is vectorised.

Every case runs a call on freshly allocated (256-byte aligned) operands, then again with operands moved to
offset_view(t, k): a view that starts k elements past a 256-byte boundary inside a sentinel-filled buffer.  Each output
must equal the aligned call's bit for bit (the entries' own tests tie that result to the references), and the guards
around every output view must still hold the sentinel: an aligned-group store that reaches before the first or past the
last element shows there.  Workspaces stay aligned: the contract requires it (tests/test_*_cpu.py check the rejection)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import raycast_cases as rc_cases                    # noqa: E402
import raycast_ref as rc                            # noqa: E402
import stereo_synthetic as syn                      # noqa: E402
import synthesis_ref                                # noqa: E402
import test_confidence_gpu as t_conf                # noqa: E402  (the generators of each entry's own tests)
import test_lr_check_gpu as t_lr                    # noqa: E402
import test_median_gpu as t_med                     # noqa: E402
import test_raycast_gpu as t_ray                    # noqa: E402
import test_sgm_gpu as t_sgm                        # noqa: E402
import test_synthesis_gpu as t_syn                  # noqa: E402
import test_temporal_gpu as t_temp                  # noqa: E402
import test_track_gpu as t_track                    # noqa: E402
import test_wls_gpu as t_wls                        # noqa: E402
import track_cases as tc                            # noqa: E402
from test_track_gpu import views, volume            # noqa: E402,F401  (the library's model views, tied to the twin's bits)

HERE = os.path.dirname(os.path.abspath(__file__))
SENTINEL_BITS = 0x7FD5A5A5                          # a quiet NaN with a payload: no kernel here produces it
SENTINEL_BYTE = 0xA5
GUARD_BYTES = 256                                   # of sentinel on each side of a view (at least 64 are required)
OFFSETS = (1, 2, 3)                                 # elements: floats, int32 words, doubles; bytes for uint8


@pytest.fixture(scope="module")
def cd():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import cuda_depth
    return cuda_depth


def _sentinel_flat(count, dtype):
    if dtype == torch.uint8:
        return torch.full((count,), SENTINEL_BYTE, dtype=torch.uint8, device="cuda")
    assert dtype in (torch.float32, torch.int32, torch.float64)
    words = torch.full((count * (2 if dtype == torch.float64 else 1),), SENTINEL_BITS, dtype=torch.int32, device="cuda")
    return words if dtype == torch.int32 else words.view(dtype)    # a double of two sentinel words is a NaN as well


def offset_view(t, k):
    """A contiguous view equal to t that starts k elements past a 256-byte boundary inside a larger sentinel-filled
    buffer, with GUARD_BYTES of sentinel (and never fewer than 64 bytes) before and after it."""
    es = t.element_size()
    front = GUARD_BYTES // es + k
    buf = _sentinel_flat(front + t.numel() + GUARD_BYTES // es, t.dtype)
    assert buf.data_ptr() % 256 == 0, "the allocator no longer returns 256-byte aligned blocks"
    view = buf[front:front + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 256 == k * es and front * es >= 64
    return view


def sentinel_view(shape, k, dtype=torch.float32):
    """An output operand at offset k that holds nothing but the sentinel."""
    return offset_view(_sentinel_flat(int(np.prod(shape)), dtype).view(shape), k)


def as_bits(t):
    """float32 as its words, float64 as its pairs of words (the last dimension doubles), everything else as it is."""
    return t.view(torch.int32) if t.dtype in (torch.float32, torch.float64) else t


def assert_guards(view, what):
    """Every element of the view's buffer outside the view still holds the sentinel."""
    base, off = view._base, view.storage_offset()
    assert base is not None and base.dim() == 1
    mark = SENTINEL_BYTE if view.dtype == torch.uint8 else SENTINEL_BITS
    b = as_bits(base)
    first, last = (i * view.element_size() // b.element_size() for i in (off, off + view.numel()))   # in b's elements
    before, after = b[:first] != mark, b[last:] != mark
    assert not bool(before.any()), f"{what}: {int(before.sum())} guard elements before the view were written"
    assert not bool(after.any()), f"{what}: {int(after.sum())} guard elements after the view were written"


def assert_same(got, want, what):
    g, w = as_bits(got).reshape(-1), as_bits(want).reshape(-1)
    assert g.shape == w.shape, f"{what}: {tuple(got.shape)} != {tuple(want.shape)}"
    if torch.equal(g, w):
        return
    bad = (g != w).nonzero().reshape(-1)
    i = int(bad[0])
    raise AssertionError(f"{what}: {bad.numel()} values differ from the aligned call's, first at flat index {i}: got "
                         f"{int(g[i]) & 0xFFFFFFFF:#x}, expected {int(w[i]) & 0xFFFFFFFF:#x}")


def check_output(view, want, what):
    assert_same(view, want, what)
    assert_guards(view, what)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- left_right_check ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", OFFSETS)
@pytest.mark.parametrize("n,H,W", [(2, 4, 64), (1, 2, 4112)])          # W % 4 == 0: the LDS form and the global form
def test_left_right_check(cd, n, H, W, k):
    dl, dr = t_lr._random_maps(np.random.default_rng(W + k), n, H, W)
    tl, tr = dev(dl), dev(dr)
    want = cd.left_right_check(tl, tr)
    for moved in ("left", "right", "out", "all"):
        a = offset_view(tl, k) if moved in ("left", "all") else tl
        b = offset_view(tr, k) if moved in ("right", "all") else tr
        out = sentinel_view((n, H, W), k if moved in ("out", "all") else 0)
        cd.left_right_check(a, b, out=out)
        check_output(out, want, f"{moved} at offset {k}")
        assert_same(a, tl, "left untouched")
        assert_same(b, tr, "right untouched")
    for right_k in (0, k):                                                # in place: out is left
        a = offset_view(tl, k)
        cd.left_right_check(a, offset_view(tr, right_k), out=a)
        check_output(a, want, f"in place at offset {k}, right at {right_k}")


# ---- the engine's plain and LR batch entries ---------------------------------------------------------------------------

GOLDEN = ["k4_48x96_d32", "k2_24x40_d16", "k1_20x31_d8"]                # K = 4 on the grid, K = 2, K = 1 with odd W
ENGINE_N = 3                                                              # inner planes of a batch start further off


def engine_inputs(kind, H, W, D, K):
    """(left, right) device batches of ENGINE_N pairs: integer-valued frames, so uint8 and float32 carry the same."""
    if kind.startswith("gray"):
        L, R = syn.make_batch(ENGINE_N, H, W, D, K, 70)
    else:
        pairs = [syn.random_rgb_pair(H, W, D, K, 80 + i) for i in range(ENGINE_N)]
        L, R = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
    L, R = np.ascontiguousarray(L, np.float32), np.ascontiguousarray(R, np.float32)
    assert np.array_equal(L, np.rint(L)) and L.min() >= 0 and L.max() <= 255
    tdt = torch.uint8 if kind.endswith("u8") else torch.float32
    return dev(L).to(tdt), dev(R).to(tdt)


@pytest.mark.parametrize("kind", ["gray_u8", "rgb_u8", "gray_f32", "rgb_f32"])
@pytest.mark.parametrize("golden", GOLDEN)
def test_engine_batch_entries(cd, golden, kind):
    H, W, K, dmin, dmax = (int(v) for v in np.load(os.path.join(HERE, "golden", golden + ".npz"))["config"])
    cfg = cd.StereoMatchingConfiguration(height=H, width=W, downscale_factor=K, min_disparity=dmin, max_disparity=dmax)
    sm = cd.StereoMatching(cfg, max_batch=2 * ENGINE_N)
    tl, tr = engine_inputs(kind, H, W, dmax + 1, K)
    shape = (ENGINE_N, H, W)
    want = sm.compute_disparity_map_batch(tl, tr, torch.empty(shape, device="cuda")).clone()
    want_r = torch.empty(shape, device="cuda")
    want_lr = sm.compute_disparity_map_batch_lr(tl, tr, torch.empty(shape, device="cuda"), right_out=want_r).clone()
    assert not torch.equal(want, want_lr), "the LR check invalidates some pixel"
    for k in OFFSETS:
        for moved in ("inputs", "outputs", "all"):
            a, b = (offset_view(tl, k), offset_view(tr, k)) if moved != "outputs" else (tl, tr)
            ko = k if moved != "inputs" else 0
            what = f"{golden} {kind}: {moved} at offset {k}"
            out = sentinel_view(shape, ko)
            sm.compute_disparity_map_batch(a, b, out)
            check_output(out, want, what + ", plain")
            out, right_out = sentinel_view(shape, ko), sentinel_view(shape, ko)
            sm.compute_disparity_map_batch_lr(a, b, out, right_out=right_out)
            check_output(out, want_lr, what + ", LR out")
            check_output(right_out, want_r, what + ", LR right_out")
            assert_same(a, tl, what + ", left untouched")
            assert_same(b, tr, what + ", right untouched")


# ---- SGM -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype,C", [("u8", 1), ("u8", 3), ("f32", 1), ("f32", 3)])
def test_sgm(cd, dtype, C):
    n, H, W, dmin, D = 2, 17, 24, 2, 12
    left, right = t_sgm.frames(n, C, H, W, dtype, 300 + C, specials=dtype == "f32")
    tl, tr = dev(left), dev(right)
    sgm = cd.StereoSGM(dmin, dmin + D - 1, uniqueness=10, lr_max_diff=1.0)
    shape = (n, H, W)
    want, want_g, want_r = (torch.empty(shape, device="cuda") for _ in range(3))
    sgm.compute(tl, tr, out=want, gray_out=want_g, right_out=want_r)
    for moved in ("frames", "outputs", "all"):
        a, b = (offset_view(tl, 1), offset_view(tr, 1)) if moved != "outputs" else (tl, tr)
        ko = 1 if moved != "frames" else 0
        out, gray, rout = sentinel_view(shape, ko), sentinel_view(shape, ko), sentinel_view(shape, ko)
        sgm.compute(a, b, out=out, gray_out=gray, right_out=rout)
        check_output(out, want, f"{moved}: out")
        check_output(gray, want_g, f"{moved}: gray_out")
        check_output(rout, want_r, f"{moved}: right_out")
        assert_same(a, tl, "left untouched")


# ---- every other map entry: all tensor operands at offset 1 ------------------------------------------------------------

MAPS = (2, 33, 96)


def run_confidence(cd, place):
    rng = np.random.default_rng(41)
    d, r, g = (dev(x) for x in (t_conf.random_map(rng, MAPS), t_conf.random_map(rng, MAPS), t_conf.random_guide(rng, MAPS)))
    out = place(None)
    cd.confidence_map(place(d), place(r), place(g), radius=2, out=out)
    return [out]


def run_temporal(cd, place):
    """Two frames through the C entry, so that the state planes and both guide planes are the caller's."""
    p = t_temp.PARAMS
    seq = t_temp.frames(np.random.default_rng(42), MAPS, 2)
    D = place(torch.full(MAPS, p["invalid_disparity"], device="cuda"))
    A, G = place(torch.zeros(MAPS, device="cuda")), place(torch.zeros(MAPS, device="cuda"))
    outs = []
    for d, c, g in seq:
        gout, out = place(None), place(None)
        t_temp.run(place(dev(d)), place(dev(c)), place(dev(g)), G, D, A, gout, out, p)
        outs += [out, gout]
        G = gout
    return outs + [D, A]


def run_median(cd, place):
    rng = np.random.default_rng(43)
    d, g = t_med.random_map(rng, MAPS), t_med.random_guide(rng, MAPS)
    h = t_med.holes_of(rng, d)
    out = place(None)
    cd.weighted_median(place(dev(d)), place(dev(g)), radius=2, sigma_color=10.0, sigma_space=2.0, holes=place(dev(h)),
                       out=out)
    return [out]


def run_wls(cd, place):
    rng = np.random.default_rng(44)
    d, g, c = t_wls.random_map(rng, MAPS), t_wls.random_guide(rng, MAPS, nan_frac=0.02), t_wls.random_conf(rng, MAPS)
    out = place(None)
    cd.wls_filter(place(dev(d)), place(dev(g)), lam=500.0, sigma_color=4.0, iterations=2, confidence=place(dev(c)),
                  out=out)
    return [out]


def _speckled(seed):
    rng = np.random.default_rng(seed)
    d = (rng.integers(0, 4, MAPS) * 3.0 + rng.uniform(-0.3, 0.3, MAPS)).astype(np.float32)
    d[rng.random(MAPS) < 0.2] = -1.0
    d[rng.random(MAPS) < 0.02] = np.nan
    return dev(d)


def run_speckles(cd, place):
    out = place(None)
    cd.filter_speckles(place(_speckled(45)), max_speckle_size=6, max_diff=1.0, out=out)
    return [out]


def run_fill(cd, place):
    out = place(None)
    cd.fill_invalid(place(_speckled(46)), out=out)
    return [out]


ENTRIES = dict(confidence_map=run_confidence, temporal_filter=run_temporal, weighted_median=run_median,
               wls_filter=run_wls, filter_speckles=run_speckles, fill_invalid=run_fill)


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_map_entry_with_every_operand_off_alignment(cd, entry):
    def aligned(t):
        return sentinel_view(MAPS, 0) if t is None else t

    def moved(t):
        return sentinel_view(MAPS, 1) if t is None else offset_view(t, 1)

    want = ENTRIES[entry](cd, aligned)
    got = ENTRIES[entry](cd, moved)
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.data_ptr() % 16 == 4, "the operand is not where the case wants it"
        check_output(g, w, f"{entry}: output {i}")


# ---- camera tracking, ray casting and right-view synthesis: inputs, outputs and both, one to three elements off ---------

PLACEMENTS = (("inputs", True, False), ("outputs", False, True), ("all", True, True))


def run_placed(ins, outs, k_in, k_out, launch):
    """launch(inputs, outputs) on the inputs moved to offset k_in and sentinel outputs of the shapes and types `outs` at
    offset k_out; returns the outputs after checking that the inputs are what they were."""
    a = {name: offset_view(t, k_in) if k_in else t for name, t in ins.items()}
    o = {name: sentinel_view(shape, k_out, dtype) for name, (shape, dtype) in outs.items()}
    launch(a, o)
    torch.cuda.synchronize()
    for name, t in ins.items():
        assert a[name].data_ptr() % 256 == k_in * t.element_size(), "the operand is not where the case wants it"
        assert_same(a[name], t, f"{name} untouched")
    return o


def check_placements(ins, outs, k, launch, what):
    """The aligned call's outputs after comparing every placement at offset k with them."""
    want = run_placed(ins, outs, 0, 0, launch)
    for moved, move_in, move_out in PLACEMENTS:
        got = run_placed(ins, outs, k if move_in else 0, k if move_out else 0, launch)
        for name in outs:
            assert got[name].data_ptr() % 256 == (k if move_out else 0) * got[name].element_size()
            check_output(got[name], want[name], f"{what}: {name} with {moved} at offset {k}")
    return want


@pytest.mark.parametrize("k", OFFSETS)
def test_track_camera(cd, views, k):
    """The C entry on two triples with confidence maps, strides 2 and 1; float64 sums and int32 info move by whole
    elements.  The workspace stays aligned."""
    d = t_track.Direct(cd, views, schedule=((2, 2), (1, 2)))
    conf = dev(np.stack([tc.frame(v, s, i, True)[3] for v, s, i, *_ in d.triples]))
    ins = dict(disp=d.disp, confidence=conf, depth=d.depth, normals=d.normals, c2w=d.c2w, w2c=d.w2c, pose_in=d.pose_in)
    outs = dict(pose_out=((d.n, 3, 4), torch.float32), info=((d.n, 4), torch.int32), rms=((d.n,), torch.float32),
                sums=((d.n, 30), torch.float64))

    def launch(a, o):
        assert d.call(min_confidence=0.1, **a, **o) == 0, d.native.last_error()

    got = check_placements(ins, outs, k, launch, "track_camera")
    for i, (v, s, j, *_) in enumerate(d.triples):                         # the aligned call is the twin's, confidence and all
        want = tc.expected(v, s, j, confidence=True, schedule=((2, 2), (1, 2)))
        assert want["info"][0] == 0 and want["info"][1] == 4
        tc.assert_same({"pose": got["pose_out"][i].cpu().numpy(), "info": got["info"][i].cpu().numpy(),
                        "rms": got["rms"][i].cpu().numpy(), "sums": got["sums"][i].cpu().numpy()}, want, f"triple {i}")


@pytest.mark.parametrize("k", OFFSETS)
def test_tsdf_raycast(cd, k):
    """The C entry with all five outputs.  The colour volume is one aligned 32-bit word per voxel (the header's state
    layout), so it moves by words; the colour output is uint8 and moves by bytes."""
    import types

    import cuda_depth._native as native
    vol = t_ray.upload(cd, rc_cases.fused_state())
    n, (H, W) = len(t_ray.THREE), rc_cases.SHAPE
    ins = dict(tsdf=vol.tsdf, weight=vol.weight, color=vol.color.view(torch.int32),
               poses=dev(rc.view_pose(rc_cases.poses_of(t_ray.THREE))))
    outs = dict(disparity=((n, H, W), torch.float32), depth=((n, H, W), torch.float32), normals=((n, 3, H, W), torch.float32),
                colors=((n, 3, H, W), torch.uint8), weight=((n, H, W), torch.float32))
    ws = torch.empty(native.LIB.smx_tsdf_raycast_workspace_bytes(*rc_cases.DIMS), dtype=torch.uint8, device="cuda")

    def launch(a, o):
        v = types.SimpleNamespace(dims=vol.dims, origin=vol.origin, voxel_size=vol.voxel_size, tsdf=a["tsdf"],
                                  weight=a["weight"], color=a["color"])
        t_ray.raycast_call(native, v, n, rc_cases.SHAPE, rc_cases.q_of("kitti"), a["poses"], t_ray.step_of(1.0),
                           rc_cases.DEPTH_RANGE, o["disparity"], o["depth"], o["normals"], o["colors"], o["weight"], ws,
                           torch.cuda.current_stream().cuda_stream)

    got = check_placements(ins, outs, k, launch, "tsdf_raycast")
    rc_cases.assert_same({name: t.cpu().numpy() for name, t in got.items()}, rc_cases.expected(t_ray.THREE, "kitti", 1.0, 1.0),
                         "the aligned call")


@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
@pytest.mark.parametrize("k", OFFSETS)
def test_synthesize_right_view(cd, k, u8):
    shape = n, C, D, h, w, S = synthesis_ref.SHAPES[1]                    # ragged tile rows and columns, two frames
    prob, left, want = t_syn.case(shape, u8)
    ins = dict(probabilities=dev(prob), left=dev(left))
    outs = dict(out=(left.shape, torch.float32))

    def launch(a, o):
        assert cd.synthesize_right_view(a["probabilities"], a["left"], scale=S, out=o["out"]) is o["out"]

    got = check_placements(ins, outs, k, launch, f"synthesize_right_view {'u8' if u8 else 'f32'}")
    t_syn.assert_bitwise(got["out"], want, "the aligned call")
