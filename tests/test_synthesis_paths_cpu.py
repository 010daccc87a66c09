"""Which instantiations and paths of the synthesis head's kernels the device tests reach (tests/synthesis_paths.py).

tests/synthesis_paths_harness.cpp prints what the real host code (k_synthesis_grad.h, k_synthesis.h, host-only) chooses for
a list of cases; the model's shape, chunk, LDS sizes and tile counts must equal it, so the model cannot drift from the
headers.  The case table of tests/test_synthesis_paths_gpu.py then has to reach, by the model: each of the 16 backward
instantiations with every path it can reach within the entries' 256 planes, each of the 8 forward instantiations with
both march forms and a second chunk, and every scale 1..16.  No GPU."""
import importlib.util
import itertools
import os
import re
import shutil
import subprocess

import pytest

import synthesis_paths as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "synthesis_paths_harness.cpp")
# beside the table: every scale and channel count at chunk lengths below, at and past one chunk
SWEEP = [sp.Case(1, C, "f32", D, h, w, S) for S, C, D, (h, w) in
         itertools.product(range(1, 17), (1, 3), (1, 2, 9, 65, 66, 256, 400), ((1, 1), (3, 18), (70, 45)))]


def _build_module():
    spec = importlib.util.spec_from_file_location("smx_build", os.path.join(ROOT, "stereo-depth_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    if not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")):
        pytest.skip("hipcc not found")
    b = _build_module()
    exe = str(tmp_path_factory.mktemp("synthesis_paths") / "synthesis_paths")
    cmd = [b.hipcc(), "-x", "hip", "--cuda-host-only", "-no-hip-rt"] + b.FLAGS + ["-I", b.INCLUDE, "-I", b.CSRC, "-o", exe, HARNESS]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, "harness did not compile:\n" + r.stdout + r.stderr
    return exe


def test_the_model_chooses_what_the_host_code_chooses(harness):
    cases = sp.CASES + SWEEP
    text = "".join("%d %d %d %d %d\n" % (c.C, c.D, c.h, c.w, c.S) for c in cases)
    r = subprocess.run([harness], input=text, capture_output=True, text=True, timeout=120)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and len(lines) == len(cases) + 1, r.stdout[-2000:] + r.stderr[-2000:]
    limits = re.fullmatch(r"limits (\d+) (\d+) cases (\d+)", lines[-1])
    assert limits and tuple(map(int, limits.groups())) == (sp.SYG_LDS_FLOATS, sp.SYN_LDS_FLOATS, len(cases)), lines[-1]
    for c, line in zip(cases, lines):
        b, f = sp.backward(c), sp.forward(c)
        mine = "grad %d %d %d %d %d %d %d %d %d %d %d  head %d %d %d %d" % (
            b["rows_log2"], b["tj_log2"], b["NT"], b["U"], b["ti"], b["tiles_i"], b["tiles_j"], b["dc"], b["rs"], b["lds"],
            b["threads"], f["dc"], f["lds"], f["tiles_x"], f["tiles_y"])
        assert line == mine, f"{tuple(c)}: the host code says\n{line}\nthe model\n{mine}"
        assert (b["NT"], b["U"]) == sp.FAMILIES[b["family"]][:2], tuple(c)


def test_the_dispatch_lines_are_the_ones_the_model_restates():
    """The instantiation is picked in tu_synthesis_grad.hip, which no host harness can include: its four lines as text."""
    text = open(os.path.join(ROOT, "stereo-depth_amd", "csrc", "tu_synthesis_grad.hip")).read()
    flat = re.sub(r"\s+", " ", text)
    for line in ("if (S == 4) launch_grad<10, 4, 4>(", "else if (sh.NT == 10) launch_grad<10, 4, 0>(",
                 "else if (sh.NT == 20) launch_grad<20, 2, 0>(", "else launch_grad<40, 1, 0>("):
        assert line in flat, line
    assert sorted(sp.FAMILIES.values()) == [(10, 4, 0), (10, 4, 4), (20, 2, 0), (40, 1, 0)]
    for fam, scales in sp.FAMILY_SCALES.items():
        for S in scales:
            assert sp.family_of(S) == fam and sp.syn_grad_shape(S)[2:] == sp.FAMILIES[fam][:2]
            assert sp.syn_grad_shape(S)[2] >= 2 * S + S // 2, "NT holds a border strip"


def test_every_staged_size_fits_the_lds():
    for c in sp.CASES + SWEEP:
        b, f = sp.backward(c), sp.forward(c)
        assert b["lds"] <= sp.SYG_LDS_FLOATS and f["lds"] <= sp.SYN_LDS_FLOATS, tuple(c)
        assert b["dc"] % b["U"] == 0 and b["dc"] >= b["U"] and 1 <= f["dc"] <= c.D, tuple(c)
        assert b["threads"] <= 256 and b["ti"] >= 2, tuple(c)


def test_the_table_reaches_every_backward_instantiation_with_every_path_it_can_reach():
    reached = {}
    for c in sp.CASES:
        b = sp.backward(c)
        assert b["flags"] <= set(sp.BACKWARD_FLAGS)
        reached.setdefault(b["instantiation"], set()).update(b["flags"])
    want = {(C, dtype, fam) for C in (1, 3) for dtype in ("f32", "u8") for fam in sp.FAMILIES}
    assert set(reached) == want and len(want) == 16
    for inst in sorted(want):
        missing = sp.reachable_flags(inst[2], inst[0]) - reached[inst]
        assert not missing, f"k_synthesis_grad<C={inst[0]}, {inst[1]}, {sp.FAMILIES[inst[2]]}> never reaches {sorted(missing)}"
    # what an instantiation cannot reach, it does not: one_round is fixed by S, U = 1 has no short step, and up to the
    # entries' 256 planes a gray frame is one chunk wherever the tile has 32 rows
    for c in sp.CASES + SWEEP:
        b = sp.backward(c)
        assert b["flags"] <= sp.family_flags(b["family"]), tuple(c)
        assert c.D > sp.MAX_PLANES or b["flags"] <= sp.reachable_flags(b["family"], c.C), tuple(c)
    assert {(C, fam) for C in (1, 3) for fam in sp.FAMILIES
            if "later_chunk_with_terms" not in sp.reachable_flags(fam, C)} == {(1, "sc4"), (1, "nt10"), (1, "nt20")}
    text = open(os.path.join(ROOT, "stereo-depth_amd", "csrc", "smx_maps.hip")).read()
    assert "if (D < 1 || D > %d) return 2;" % sp.MAX_PLANES in text, "the entries' limit on D"


def test_the_table_reaches_every_forward_instantiation_with_both_marches_and_a_second_chunk():
    reached, anywhere = {}, set()
    for c in sp.CASES:
        f = sp.forward(c)
        assert f["flags"] <= set(sp.FORWARD_FLAGS)
        anywhere |= f["flags"]
        for inst in f["instantiations"]:
            reached.setdefault(inst, set()).update(f["flags"])
    want = {(C, dtype, rescale) for C in (1, 3) for dtype in ("f32", "u8") for rescale in (True, False)}
    assert set(reached) == want and len(want) == 8
    for inst in sorted(want):
        missing = {"march_pairs", "march_rows", "two_chunks"} - reached[inst]
        assert not missing, f"k_synthesis<C={inst[0]}, {inst[1]}, RESCALE={inst[2]}> never reaches {sorted(missing)}"
    assert anywhere == set(sp.FORWARD_FLAGS), sorted(set(sp.FORWARD_FLAGS) - anywhere)


def test_every_scale_appears_and_every_case_has_two_frames():
    assert {c.S for c in sp.CASES} == set(range(1, 17))
    for fam in ("nt10", "nt20", "nt40"):
        assert any(c.S % 2 for c in sp.CASES if sp.family_of(c.S) == fam), f"an odd scale in {fam}"
    assert all(c.n == 2 and c.dtype in ("f32", "u8") and c.C in (1, 3) and 1 <= c.D <= sp.MAX_PLANES for c in sp.CASES)
    assert len(set(sp.CASES)) == len(sp.CASES)
    assert any(c.w * c.S < c.D for c in sp.CASES), "planes d >= W"


def test_the_model_on_the_shapes_worked_out_by_hand():
    """Figures read off the headers: D = 65 at S = 8, C = 3 is staged in chunks of 56 planes; a gray frame at S = 8 in
    chunks of 328, where w = 44 leaves the second chunk its terms in the first tile and none in the last; S = 16 at
    C = 3 holds 7 planes, and its tile j_lo = 2 of w = 6 is full; at S = 9 and w = 6 the full strip lasts while d <= 14."""
    assert sp.backward(sp.Case(2, 3, "f32", 65, 3, 18, 8))["dc"] == 56
    b = sp.backward(sp.Case(2, 1, "f32", 340, 1, 44, 8))
    assert b["dc"] == 328 and {"later_chunk_with_terms", "chunk_without_columns", "strip_full"} <= b["flags"]
    b = sp.backward(sp.Case(2, 3, "f32", 9, 2, 6, 16))
    assert b["dc"] == 7 and b["lds"] == 14210 and {"strip_full", "later_chunk_with_terms"} <= b["flags"]
    assert "strip_partial_in_full_tile" not in sp.backward(sp.Case(2, 3, "f32", 15, 1, 6, 9))["flags"]
    assert "strip_partial_in_full_tile" in sp.backward(sp.Case(2, 3, "f32", 16, 1, 6, 9))["flags"]
    # the shape tables of the older tests leave the FULL strip at NT = 20 unreached: w = 3 and w = 10
    assert "strip_full" not in sp.backward(sp.Case(1, 3, "f32", 65, 3, 10, 8))["flags"]
