"""The second pass of the stacked bands (k_match_fast.h: fast_stacked_tail) against the oracle, bit for bit.

Behind pass 1 a stacked wave fills one needed-set table per 24-row unit band and walks both at once: a disparity that both
unit bands need is marched once over the 70 staged tile rows (row mask of 48 bits), one that a single unit band needs over
that band's 46 rows, and fast_tail_leftover deals the odd ones out.  Every form gives the same bits, so each case compares
the final map, the WTA index and the three cost planes (AGG[arg], AGG[arg + 1], AGG[arg - 1]) of every distinct pair with
the oracle (multi_block_matching_cost_aggregation.cu:54-88, wta_disparity_selection.cu:22-30, secondary_matching.cu:28-31).

Harness as in tests/test_stacked_bands_gpu.py: the form forced (SMX_FAST_STACK=1), one engine-stream call of the smallest
batch that takes the throughput shape on this device, the eight contents of tests/stacked_tail_ref.py tiled over it
(idx = j % 8); smx_get_match_geometry must report 48-row bands.  Pooled shapes (stacked_tail_ref.CASES): 48 x 190 at 64
disparities (K = 2, box sums from prefix sums), 30 x 190 (six rows in the lower unit band), 24 x 190 (none), 54 x 190 (a
second band of six rows), 48 x 64 (one full and one partial window), 48 x 190 at 67 (the most a pitch-256 tile holds), 33
and 2 disparities, and at K = 4 (sliding sums).  Contents: a fronto-parallel plane, a disparity step on the seam row, one
row above and one row below it, a vertical ramp, planes at disparity 0 and Dd - 1, uniform noise.
tests/test_stacked_tail_cpu.py shows from the oracle alone that each case reaches every class of needed disparity, an odd
count in every queue, a row mask with bits from 32 on and both cyclic neighbours (or why its geometry cannot).

The report of the sparse form kept its meaning -- marches of a per-band second pass, per unit band -- and is checked apart,
for three of the cases: the value printed under SMX_DEBUG_HINTS=1 equals what tests/fast_density_ref.py predicts for 24-row
windows, |printed - model| <= 0.0005 + 1e-6 (the print's rounding plus float32 slack, as in tests/test_fast_density_gpu.py)."""
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import fast_density_ref as fd                       # noqa: E402
import stacked_tail_ref as st                       # noqa: E402
import test_gpu_parity as parity                    # noqa: E402

LINE = re.compile(r"\[smx\] fast kernel: second pass / first pass = ([0-9.]+) \(dense ([01])\)")   # smx_engine.hip: read_hints
TOL = 0.0005 + 1e-6


@pytest.fixture(scope="module")
def cd():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import cuda_depth
    return cuda_depth


@pytest.fixture(scope="module")
def cus(cd):
    cfg = cd.StereoMatchingConfiguration(height=64, width=96, min_disparity=0, max_disparity=15)
    return cd.StereoMatching(cfg).route_info()["compute_units"]


def _batch(runs, n, idx=None):
    idx = torch.arange(n, device="cuda") % len(runs) if idx is None else torch.tensor(idx, device="cuda")
    tl, tr = (torch.from_numpy(np.stack([r[k] for r in runs])).to(torch.uint8).cuda()[idx].contiguous() for k in (0, 1))
    return idx, tl, tr


@pytest.mark.parametrize("case", st.CASES, ids=[c["name"] for c in st.CASES])
def test_stacked_tail_against_the_oracle(cd, oracle_omp, monkeypatch, cus, case):
    from cuda_depth import _native as N
    K, h, w, Dd = case["K"], case["h"], case["w"], case["Dd"]
    n = st.throughput_pairs(h, w, cus)
    cfg, ocfg = parity._cfgs(cd, h * K, w * K, K, 0, Dd * K - 1)
    runs = st.oracle_runs(oracle_omp, ocfg, case)
    idx, tl, tr = _batch(runs, n)
    assert n >= 2 * len(runs), "every content at least twice in the batch"
    monkeypatch.setenv("SMX_FAST_STACK", "1")                       # read once, in smx_create
    sm = cd.StereoMatching(cfg, max_batch=n, overlap_min_pairs=-1)
    out = sm.compute_disparity_map_batch(tl, tr, engine_streams=True)
    sm.join()
    torch.cuda.synchronize()
    geo = sm.match_geometry(n)
    assert geo["kernel"] == "fast_window" and geo["band_rows"] == 48 and geo["rows_marched"] == 70, geo
    stages = {k: s for k, s in (("wta", N.STAGE_WTA), ("costs", N.STAGE_MBM_COSTS), ("refined", N.STAGE_REFINED),
                                ("down_left", N.STAGE_DOWN_LEFT), ("down_right", N.STAGE_DOWN_RIGHT))}
    for i, (_, _, ref_out, ref) in enumerate(runs):
        for j in (i, i + len(runs) * ((n - 1 - i) // len(runs))):   # the content's first and last copy in the batch
            assert int(idx[j]) == i
            got = {k: sm.intermediate(s, j).cpu().numpy() for k, s in stages.items()}
            got["out"] = out[j].cpu().numpy()
            parity._check(got, ref_out, ref, 0)


@pytest.mark.parametrize("name", st.REPORT_CASES)
def test_the_report_is_still_the_per_band_count(cd, oracle_omp, monkeypatch, capfd, cus, name):
    case = st.CASES_BY_NAME[name]
    K, h, w, Dd = case["K"], case["h"], case["w"], case["Dd"]
    n = st.throughput_pairs(h, w, cus)
    cfg, ocfg = parity._cfgs(cd, h * K, w * K, K, 0, Dd * K - 1)
    runs = st.oracle_runs(oracle_omp, ocfg, case)
    # Only every stride-th pair of a launch reports (fast_density_ref.sample_stride), and a stride that is a multiple of
    # eight would sample one content alone: the tiling advances by three more contents per stride and starts at the ramp,
    # so that the sampled pairs are ramp, noise, the step above the seam and the plane at 0 (four pairs at strides of 16).
    stride = fd.sample_stride(n)
    content = [(j + 4 + 3 * (j // stride)) % len(runs) for j in range(n)]
    assert len({content[j] for j in fd.sampled_pairs(n)}) >= min(3, len(fd.sampled_pairs(n))), "the sampled pairs differ in content"
    _, tl, tr = _batch(runs, n, content)
    monkeypatch.setenv("SMX_DEBUG_HINTS", "1")
    monkeypatch.setenv("SMX_FAST_STACK", "1")
    for k in ("SMX_FAST_DENSE", "SMX_FAST_DENSE_SMALL"):             # no forced form: a forced form does not report
        monkeypatch.delenv(k, raising=False)
    sm = cd.StereoMatching(cfg, max_batch=n, overlap_min_pairs=-1)  # a fresh engine is in the sparse form
    capfd.readouterr()
    out = sm.compute_disparity_map_batch(tl, tr, engine_streams=True)
    sm.join()
    torch.cuda.synchronize()
    sm.route_info()                                                  # read_hints: prints a fresh report
    reports = [(float(v), int(d)) for v, d in LINE.findall(capfd.readouterr().err)]
    geo = sm.match_geometry(n)
    assert geo["kernel"] == "fast_window" and geo["band_rows"] == 48, geo
    per_lane, model = fd.call_report(lambda j: runs[content[j]][3]["wta_index"], n, 1, Dd, fd.FA_TH, fd.tall_nd(Dd))
    print(f"{name}: n {n}: " + " + ".join(f"{m}/{win} = {float(r):.4f}" for m, win, r in per_lane) + f" -> {float(model):.4f}; printed {reports}")
    assert len(reports) == 1 and reports[0][1] == 0, reports
    assert abs(reports[0][0] - float(model)) <= TOL, (reports[0][0], float(model), per_lane)
    assert np.array_equal(out[0].cpu().numpy(), runs[content[0]][2]) and np.array_equal(out[n - 1].cpu().numpy(), runs[content[n - 1]][2])
