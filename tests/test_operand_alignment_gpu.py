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

import stereo_synthetic as syn                      # noqa: E402
import test_confidence_gpu as t_conf                # noqa: E402  (the generators of each entry's own tests)
import test_lr_check_gpu as t_lr                    # noqa: E402
import test_median_gpu as t_med                     # noqa: E402
import test_sgm_gpu as t_sgm                        # noqa: E402
import test_temporal_gpu as t_temp                  # noqa: E402
import test_wls_gpu as t_wls                        # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
SENTINEL_BITS = 0x7FD5A5A5                          # a quiet NaN with a payload: no kernel here produces it
SENTINEL_BYTE = 0xA5
GUARD_BYTES = 256                                   # of sentinel on each side of a view (at least 64 are required)
OFFSETS = (1, 2, 3)                                 # elements: floats for float32 operands, bytes for uint8


@pytest.fixture(scope="module")
def cd():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import cuda_depth
    return cuda_depth


def _sentinel_flat(count, dtype):
    if dtype == torch.uint8:
        return torch.full((count,), SENTINEL_BYTE, dtype=torch.uint8, device="cuda")
    assert dtype == torch.float32
    return torch.full((count,), SENTINEL_BITS, dtype=torch.int32, device="cuda").view(torch.float32)


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
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def assert_guards(view, what):
    """Every element of the view's buffer outside the view still holds the sentinel."""
    base, off = view._base, view.storage_offset()
    assert base is not None and base.dim() == 1
    mark = SENTINEL_BYTE if view.dtype == torch.uint8 else SENTINEL_BITS
    b = as_bits(base)
    before, after = b[:off] != mark, b[off + view.numel():] != mark
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
