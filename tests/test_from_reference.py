"""The pin: consumes the outputs of the REFERENCE ITSELF under tests/golden/from_reference/ (schema and provenance:
that directory's README.md -- the reference's own sources, built for the host), finds the floating-point convention the
binary that produced them follows, and pins the HIP path to them BITWISE under that convention.

Nothing of the reference is imported, copied or run here, and nothing under oracle/_ref/ is loaded: the committed
files are enough (tests/test_reference_host_cpu.py is where the host build itself runs).  The reference is
built by nvcc with its default --fmad=true (depth/setup.py:4-23 passes no flags), so its binary contracts the three sums
of products of the path (rgb_to_grayscale.cu:24-28, device_functions.cuh:39-40) and WHICH products it fuses is the
compiler's choice: the oracle and the engine both implement every possible choice (stereo_oracle.h SO_FP_* =
include/stereo_mi355x.h smx_fp_convention).  The CPU tests keep the machinery honest: they feed it "reference outputs"
produced by the oracle under each convention and expect it to name that convention."""
import glob
import os

import numpy as np
import pytest

import oracle_lib
import stereo_synthetic as syn
from oracle_lib import OracleConfig, FP_CONVENTIONS, FP_MIXED_CONVENTIONS, fp_name

DIR = os.path.join(os.path.dirname(__file__), "golden", "from_reference")
FILES = sorted(glob.glob(os.path.join(DIR, "*.npz")))
STAGES = ("gray_left", "down_left", "wta", "refined")
# a file's `config`: the first five fields (the rest at the reference's defaults, which are OracleConfig's) or all eleven,
# in the order of the reference's stereo_matching_configuration.hh
CONFIG_FIELDS = ("height", "width", "downscale_factor", "min_disparity", "max_disparity", "ncc_patch_radius",
                 "sad_patch_radius", "threshold", "small_mbm_radius", "mid_mbm_radius", "large_mbm_radius")


def oracle_config(config, conv=0):
    values = [int(v) for v in config]
    assert len(values) in (5, len(CONFIG_FIELDS)), f"a config of {len(values)} entries"
    return OracleConfig(fp_convention=conv, **dict(zip(CONFIG_FIELDS, values)))


def _all_fields(path):
    with np.load(path) as z:
        return z["config"].size == len(CONFIG_FIELDS)


ALL_FIELD_FILES = [p for p in FILES if _all_fields(p)]      # produced under non-default radii and threshold


def classify(z, orc):
    """Compares a reference-produced case with the oracle under every floating-point convention, inside the validity
    masks.  Returns (matching, report, cfg, masks): `matching` lists the conventions that reproduce every stored array
    bit for bit (several when the case is insensitive, e.g. integer gray with min_disparity = 0; none if the file agrees
    with no convention), report[name] the max |difference| per stage.  The six plain conventions (one pattern for step 1
    and the parabola alike) are tried first; only a file that none of them reproduces is tried against the mixed ones
    (a compiler chooses per expression: oracle_lib.FP_MIXED_CONVENTIONS)."""
    cfg = oracle_config(z["config"])
    md, mf = orc.masks(cfg)
    report, matching = {}, []
    for conv, name in list(FP_CONVENTIONS.items()) + list(FP_MIXED_CONVENTIONS.items()):
        if conv not in FP_CONVENTIONS and matching:
            break
        cfg.fp_convention = conv
        out, im = orc.run(cfg, z["left"], z["right"], intermediates=True)
        diffs = {"out": float(np.max(np.abs(out - z["out"])[mf])) if mf.any() else 0.0}
        exact = np.array_equal(out[mf], z["out"][mf])
        for st in STAGES:
            if st in z.files:
                m = mf if im[st].shape == mf.shape else md
                diffs[st] = float(np.max(np.abs(im[st] - z[st])[m])) if m.any() else 0.0
                exact = exact and np.array_equal(im[st][m], z[st][m])
        report[name] = diffs
        if exact:
            matching.append(conv)
    cfg.fp_convention = matching[0] if matching else 0
    return matching, report, cfg, (md, mf)


class _Case(dict):
    @property
    def files(self):
        return list(self)


def _fake_reference_case(orc, conv, rgb=True, dmin=0, H=40, W=64, D=16, noise=False):
    K = 2
    cfg = OracleConfig(height=H, width=W, downscale_factor=K, min_disparity=dmin, max_disparity=dmin + D - 1, fp_convention=conv)
    if noise:
        l, r = syn.make_noise_pair(H, W, 1)
    else:
        l, r = syn.random_rgb_pair(H, W, D, K, 4, dmin=dmin) if rgb else syn.make_pair(H, W, D, K, 4, dmin=dmin)[:2]
    out, im = orc.run(cfg, l, r, intermediates=True)
    z = _Case(left=l, right=r, out=out, config=np.array([H, W, K, dmin, dmin + D - 1], np.int32))
    z.update({k: im[k] for k in STAGES})
    return z


@pytest.mark.parametrize("conv", sorted(FP_CONVENTIONS))
def test_the_hook_names_the_convention_of_an_rgb_case(oracle, conv):
    matching, report, cfg, _ = classify(_fake_reference_case(oracle, conv), oracle)
    assert matching == [conv], report
    assert cfg.fp_convention == conv


def test_conventions_agree_on_integer_gray_and_part_on_the_parabola(oracle):
    """Integer-valued gray, min_disparity = 0 (the BASELINE style): products and sums up to the parabola are exact, and the
    parabola's sums are sums of small-integer multiples that rarely round differently -- the case may match several
    conventions.  With min_disparity > 0 the Q5 lookups (secondary_matching.cu:28-31) hand the parabola unrelated costs
    and the conventions separate in `refined`."""
    z = _fake_reference_case(oracle, 1, rgb=False)
    matching, report, _, _ = classify(z, oracle)
    assert 1 in matching
    for name in report:
        assert report[name]["down_left"] == 0.0 and report[name]["wta"] == 0.0, name
    z = _fake_reference_case(oracle, 1, rgb=False, dmin=20, H=64, W=96, D=32, noise=True)
    matching, report, _, _ = classify(z, oracle)
    assert 1 in matching and 0 not in matching, report
    assert report["source"]["refined"] > 1e-4, report      # NOT "within 1e-4 across conventions"


def test_a_file_that_matches_no_convention_is_reported(oracle):
    z = _fake_reference_case(oracle, 0)
    z["out"] = z["out"] + np.float32(0.25)
    matching, report, _, _ = classify(z, oracle)
    assert matching == [] and all(v["out"] > 0 for v in report.values())


def test_reference_files_follow_the_schema():
    for f in FILES:
        z = np.load(f)                      # allow_pickle stays False
        assert {"left", "right", "out", "config"} <= set(z.files), f
        H, W = int(z["config"][0]), int(z["config"][1])
        assert z["out"].shape == (H, W) and z["left"].shape in ((3, H, W), (H, W)), f


def _engine(cfg, **kwargs):
    """An engine with all eleven fields of cfg and its floating-point convention."""
    import cuda_depth
    return cuda_depth.StereoMatching(cuda_depth.StereoMatchingConfiguration(**{f: getattr(cfg, f) for f in CONFIG_FIELDS}),
                                     fp_convention=cfg.fp_convention, **kwargs)


def _hip_run(cfg, left, right, stages=()):
    import torch
    from cuda_depth import _native as N
    sm = _engine(cfg)
    l, r = torch.from_numpy(left).cuda(), torch.from_numpy(right).cuda()
    got = {"out": (sm.compute_disparity_map(l, r) if l.dim() == 3 else sm.compute_disparity_map_gray(l, r)).cpu().numpy()}
    ids = {"gray_left": N.STAGE_GRAY_LEFT, "down_left": N.STAGE_DOWN_LEFT, "wta": N.STAGE_WTA, "refined": N.STAGE_REFINED}
    for st in stages:
        if st == "gray_left" and left.ndim == 2:
            continue
        got[st] = sm.intermediate(ids[st]).cpu().numpy()
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("conv", [0, 1, 2])
def test_the_pin_works_end_to_end_on_a_stand_in(oracle, conv):
    """The machinery of the pin below on a stand-in file (oracle output under a convention): the hook names the convention,
    the engine created with it reproduces the file bitwise inside the masks."""
    pytest.importorskip("torch")
    z = _fake_reference_case(oracle, conv, dmin=8)
    matching, report, cfg, (md, mf) = classify(z, oracle)
    assert matching == [conv], report
    got = _hip_run(cfg, z["left"], z["right"], STAGES)
    for st in got:
        want = z["out"] if st == "out" else z[st]
        m = mf if want.shape == mf.shape else md
        assert np.array_equal(got[st][m], want[m]), st


@pytest.mark.gpu
def test_the_pin_works_end_to_end_on_a_mixed_convention(oracle):
    """Step 1 and the parabola contracted differently (SMX_FP_MIXED; what gcc does to the reference's text): no plain
    convention reproduces such a file, the hook names a mixed one, and the engine created with it is bitwise equal."""
    conv = oracle_lib.fp_mixed(3, 2)
    z = _fake_reference_case(oracle, conv, dmin=20, H=64, W=96, D=32)
    matching, report, cfg, (md, mf) = classify(z, oracle)
    assert conv in matching and not any(c in FP_CONVENTIONS for c in matching), report
    from cuda_depth import _native as N
    assert N.fp_mixed("fma_outer", "fma_second") == conv
    cfg.fp_convention = conv
    got = _hip_run(cfg, z["left"], z["right"], STAGES)
    for st in got:
        want = z["out"] if st == "out" else z[st]
        m = mf if want.shape == mf.shape else md
        assert np.array_equal(got[st][m], want[m]), st
    with pytest.raises(RuntimeError):                           # pattern 6 does not exist, alone or as a site
        cfg.fp_convention = 6 | (1 << 3)
        _hip_run(cfg, z["left"], z["right"])


@pytest.mark.gpu
@pytest.mark.parametrize("path", FILES or [None], ids=[os.path.basename(p) for p in FILES] or ["none"])
def test_hip_path_against_outputs_of_the_reference(path, oracle):
    """The pin: HIP path vs what the reference's own binary produced, BITWISE inside the validity mask, with the engine
    created under the floating-point convention the file follows."""
    if path is None:
        pytest.skip("no reference-produced outputs under tests/golden/from_reference/ (README.md there says how to add them)")
    pytest.importorskip("torch")
    z = np.load(path)
    matching, report, cfg, (md, mf) = classify(z, oracle)
    if not matching:
        pytest.fail(f"{path}: the reference's output matches no floating-point convention of the oracle: {report}")
    got = _hip_run(cfg, z["left"], z["right"], [s for s in STAGES if s in z.files])
    for st in got:
        want = z["out"] if st == "out" else z[st]
        m = mf if want.shape == mf.shape else md
        bad = int(np.count_nonzero(got[st][m] != want[m]))
        assert bad == 0, f"{path}: stage {st} differs from the reference in {bad} masked pixels under convention {fp_name(cfg.fp_convention)}"


# ---- files produced under non-default ncc / sad radii, threshold and aggregation radii --------------------------------
_CLASSIFIED = {}


def _classified(path, oracle):
    """(arrays of the file, cfg under the convention it follows, (mask_down, mask_full)), computed once per file."""
    if path not in _CLASSIFIED:
        with np.load(path) as f:
            z = _Case({k: f[k] for k in f.files})
        matching, report, cfg, masks = classify(z, oracle)
        assert matching, f"{path}: the reference's output matches no floating-point convention of the oracle: {report}"
        _CLASSIFIED[path] = (z, cfg, masks)
    return _CLASSIFIED[path]


_IDS = [os.path.basename(p)[:-4] for p in ALL_FIELD_FILES]


def test_the_files_under_non_default_fields_are_there():
    """Six of them, every one of the six fields away from its default somewhere, ncc_patch_radius on both sides of 2
    (stereo_oracle.h, safe rule S8), one integer-valued (the uint8 entry needs it)."""
    configs = [np.load(p)["config"] for p in ALL_FIELD_FILES]
    assert len(configs) == 6
    default = OracleConfig()
    for i, f in enumerate(CONFIG_FIELDS[5:], 5):
        assert any(int(c[i]) != getattr(default, f) for c in configs), f
    assert {int(c[5]) for c in configs} >= {0, 1, 2, 3}
    assert sum(_integer_valued(np.load(p)) for p in ALL_FIELD_FILES) == 1


def _integer_valued(z):
    return bool(np.all(z["left"] == np.rint(z["left"])) and np.all(z["right"] == np.rint(z["right"])))


def _other_pair(z, cfg, index):
    """A seeded float32 pair of the file's shape and kind (its neighbours in a batch)."""
    D = cfg.max_disparity + 1
    if z["left"].ndim == 3:
        l, r = syn.random_rgb_pair(cfg.height, cfg.width, D, cfg.downscale_factor, index, dmin=cfg.min_disparity)
    else:
        l, r = syn.make_pair(cfg.height, cfg.width, D, cfg.downscale_factor, index, dmin=cfg.min_disparity)[:2]
    return np.ascontiguousarray(l, np.float32), np.ascontiguousarray(r, np.float32)


@pytest.mark.gpu
@pytest.mark.parametrize("path", ALL_FIELD_FILES, ids=_IDS)
def test_batch_entry_against_outputs_of_the_reference(path, oracle):
    """The file's pair as the middle of a batch of three: its map equals the file bit for bit inside the mask, and the
    two seeded pairs around it come out as from single-pair calls, everywhere.  Non-default radii lie outside the fast
    kernel's envelope: every call reports exact_order."""
    torch = pytest.importorskip("torch")
    z, cfg, (_, mf) = _classified(path, oracle)
    pairs = [_other_pair(z, cfg, 401), (z["left"], z["right"]), _other_pair(z, cfg, 402)]
    sm = _engine(cfg, max_batch=3)
    left = torch.from_numpy(np.stack([p[0] for p in pairs])).cuda()
    right = torch.from_numpy(np.stack([p[1] for p in pairs])).cuda()
    got = sm.compute_disparity_map_batch(left, right).cpu().numpy()
    assert sm.last_match_mode() == "exact_order"
    bad = int(np.count_nonzero(got[1][mf] != z["out"][mf]))
    assert bad == 0, f"{path}: the middle pair of the batch differs from the reference in {bad} of {int(mf.sum())} masked pixels"
    single = sm.compute_disparity_map if left.dim() == 4 else sm.compute_disparity_map_gray
    for i in (0, 1, 2):
        alone = single(left[i], right[i]).cpu().numpy()
        assert sm.last_match_mode() == "exact_order"
        assert np.array_equal(got[i].view(np.uint32), alone.view(np.uint32)), f"{path}: pair {i} of the batch"


_INTEGER_FILES = [p for p in ALL_FIELD_FILES if _integer_valued(np.load(p))]


@pytest.mark.gpu
@pytest.mark.parametrize("path", _INTEGER_FILES, ids=[os.path.basename(p)[:-4] for p in _INTEGER_FILES])
def test_uint8_entry_against_outputs_of_the_reference(path, oracle):
    """The integer-valued file through the uint8 entries (single pair, and a batch of one): equal to the file bit for
    bit inside the mask."""
    torch = pytest.importorskip("torch")
    z, cfg, (_, mf) = _classified(path, oracle)
    sm = _engine(cfg)
    l, r = torch.from_numpy(z["left"]).to(torch.uint8).cuda(), torch.from_numpy(z["right"]).to(torch.uint8).cuda()
    assert np.array_equal(l.cpu().numpy().astype(np.float32), z["left"])
    single = sm.compute_disparity_map if l.dim() == 3 else sm.compute_disparity_map_gray
    got = single(l, r).cpu().numpy()
    assert sm.last_match_mode() == "exact_order"
    bad = int(np.count_nonzero(got[mf] != z["out"][mf]))
    assert bad == 0, f"{path}: the uint8 entry differs from the reference in {bad} of {int(mf.sum())} masked pixels"
    got = sm.compute_disparity_map_batch(l[None], r[None]).cpu().numpy()[0]
    assert sm.last_match_mode() == "exact_order"
    assert np.array_equal(got[mf], z["out"][mf])
