"""The density report of the sparse fast kernel (k_match_fast.h: fast_stats_report, fast_stacked_tail; k_fill.h:
fill_publish_fast_stats) against its model (tests/fast_density_ref.py).

The report is what ContentSwitch fast{0.10, 0.07} (smx_route.h) chooses the form of every later on-grid batch by, and no other
test reads its value: every form gives the same bits.  It is an exact function of the oracle's winner map and the launch
geometry, so each case pins it to the model to the last printed digit: an engine created with SMX_DEBUG_HINTS=1 prints every
fresh report it reads (`[smx] fast kernel: second pass / first pass = %.3f`, smx_engine.hip: read_hints) and route_info() reads.
Every case: a fresh engine (a report above 0.10 makes the next call dense, which reports nothing), no forced form,
match_geometry in the form the model assumes, exactly one report line, |printed - model| <= 0.0005 + 1e-6 (the print's
rounding plus float32 slack: the model has no other margin), and the first and the last map bit for bit against the oracle.

Inputs are uint8 gray, min_disparity 0, K = 2; the calls (fast_density_ref.CASES) are the smallest in the throughput shape
on the device at hand -- one workgroup of unit bands per CU on the stream lanes, 1.625 on a caller's stream
(match_fast_plan) -- and tile their distinct pairs with idx = j % len(pairs).  tests/test_fast_density_cpu.py shows from the
oracle alone that these inputs tell a wrong window height, a miscounted march and wrongly sampled pairs from the right ones.

Which height a plain case runs at is the plan's choice, asserted against its restatement (fast_density_ref.plain_band_rows):
24 rows at 96 x 190 (a 32-row tile of pitch 256 does not fit a CU three times, so 3 x 54 rows weighted by 1.3 lose to
4 x 46), 27 at 54 x 190, 32 at 30 x 190.  Plain and stacked therefore print the same value at 96 x 190; the pair of cases at
54 x 190 (plain_27_rows, stacked_where_plain_is_27) is where the stacked form's 24-row windows show against the plain plan's.
Measured on an MI355X (256 CUs), printed = model in every case: band / slant / noise at 96 x 190 0.041 / 0.308 / 0.933,
54 x 190 plain 0.566 against stacked 0.435, 30 x 190 plain 0.956, mixed 0.328, the latency frame 0.144 (69 / 15)."""
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import fast_density_ref as fd                       # noqa: E402
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


@pytest.fixture
def hints_env(monkeypatch):
    """SMX_DEBUG_HINTS on, no forced form (all read once, in smx_create)."""
    monkeypatch.setenv("SMX_DEBUG_HINTS", "1")
    for k in ("SMX_FAST_DENSE", "SMX_FAST_DENSE_SMALL", "SMX_FAST_STACK"):
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


_ORACLE = {}


def _oracle(oracle, ocfg, K, h, w, Dd, content, dmin=0):
    """(left, right, map, winner indices) of a named pair: the oracle runs once per distinct pair."""
    key = (K, h, w, Dd, content, dmin)
    if key not in _ORACLE:
        l, r = fd.make_content(content, h * K, w * K, Dd * K, K)
        out, im = oracle.run(ocfg, l, r, intermediates=True)
        _ORACLE[key] = (l, r, out, im["wta_index"].copy())
    return _ORACLE[key]


def _batch(pairs, n):
    idx = torch.arange(n, device="cuda") % len(pairs)
    return tuple(torch.from_numpy(np.stack([p[k] for p in pairs])).to(torch.uint8).cuda()[idx].contiguous() for k in (0, 1))


def _reports(capfd):
    return [(float(v), int(d)) for v, d in LINE.findall(capfd.readouterr().err)]


def _run(sm, tl, tr, streams, capfd):
    """One batch call, finished; the reports the engine printed from the call's start up to route_info()."""
    out = sm.compute_disparity_map_batch(tl, tr, engine_streams=streams)
    if streams:
        sm.join()
    torch.cuda.synchronize()
    info = sm.route_info()                           # read_hints: prints a fresh report
    return out, info, _reports(capfd)


@pytest.mark.parametrize("case", fd.CASES, ids=[c["name"] for c in fd.CASES])
def test_report_equals_the_model(cd, oracle_omp, hints_env, capfd, cus, case):
    K, h, w, Dd = case["K"], case["h"], case["w"], case["Dd"]
    n = fd.case_pairs(case, cus)
    cfg, ocfg = parity._cfgs(cd, h * K, w * K, K, 0, Dd * K - 1)
    pairs = [_oracle(oracle_omp, ocfg, K, h, w, Dd, c) for c in case["tiles"]]
    tl, tr = _batch(pairs, n)
    if case["stack"] is not None:
        hints_env.setenv("SMX_FAST_STACK", case["stack"])
    sm = cd.StereoMatching(cfg, max_batch=n, overlap_min_pairs=2 if case["lanes"] == 2 else -1)
    capfd.readouterr()
    out, info, reports = _run(sm, tl, tr, case["streams"], capfd)
    geo = sm.match_geometry(n)
    assert geo["kernel"] == "fast_window", geo
    if case["streams"]:
        assert sm.overlap_lanes(n) == case["lanes"]
    if case["rows"] is None:
        # (Dd = 140: no stacked instantiation, whatever is forced); the height the CPU test counts this case under
        assert geo["band_rows"] in fd.PLAIN_ROWS and geo["band_rows"] == fd.plain_band_rows(h, Dd), geo
    else:
        assert geo["band_rows"] == case["rows"] == fd.FA_STACK_TH and geo["rows_marched"] == 70, geo
    rows = fd.case_model_rows(case, geo["band_rows"])
    per_lane, model = fd.call_report(lambda j: pairs[j % len(pairs)][3], n, case["lanes"], Dd, rows, fd.tall_nd(Dd))
    print(f"{case['name']}: n {n}, band_rows {geo['band_rows']}, model R {rows}: " +
          " + ".join(f"{m}/{win} = {float(r):.4f}" for m, win, r in per_lane) + f" -> {float(model):.4f}; printed {reports}")
    if case["mixed"]:                                                # condition 3 of the CPU test, for this device's n
        pick_all = fd.call_report(lambda j: pairs[j % len(pairs)][3], n, case["lanes"], Dd, rows, fd.tall_nd(Dd),
                                  pick=lambda nl: list(range(nl)))[1]
        pick_next = fd.call_report(lambda j: pairs[j % len(pairs)][3], n, case["lanes"], Dd, rows, fd.tall_nd(Dd),
                                   pick=lambda nl: fd.sampled_pairs(nl, fd.sample_stride(nl) + 1))[1]
        assert abs(float(model) - float(pick_all)) > 0.005 and abs(float(model) - float(pick_next)) > 0.005, (model, pick_all, pick_next)
    assert len(reports) == 1, reports
    assert reports[0][1] == 0, "a fresh engine is in the sparse form"
    assert abs(reports[0][0] - float(model)) <= TOL, (reports[0][0], float(model), per_lane)
    assert info["fast_dense"] == (1 if float(model) > 0.10 else 0)   # ContentSwitch fast{0.10, 0.07}: hi
    for j in (0, n - 1):
        assert np.array_equal(out[j].cpu().numpy(), pairs[j % len(pairs)][2]), f"pair {j} of {n} differs from the oracle"


def test_latency_shape_at_12_row_bands(cd, oracle_omp, hints_env, capfd, cus):
    """One pair in the split kernel at 12-row bands (match_fast_plan: `wg_small > cus && wg_tall <= cus`): one window per
    workgroup, every 16th workgroup reports, its eight waves deal the needed disparities out pair by pair."""
    K, Dd = 2, fd.LATENCY_DD
    shape = fd.latency_shape(cus)
    if shape is None:
        pytest.skip(f"no size under pooled 200 x 640 takes 12-row bands for one pair at {cus} compute units")
    h, w = shape
    cfg, ocfg = parity._cfgs(cd, h * K, w * K, K, 0, Dd * K - 1)
    l, r, want, wta = _oracle(oracle_omp, ocfg, K, h, w, Dd, fd.LATENCY_CONTENT)
    tl, tr = (torch.from_numpy(x).to(torch.uint8).cuda() for x in (l, r))
    sm = cd.StereoMatching(cfg)
    capfd.readouterr()
    out = sm.compute_disparity_map_gray(tl, tr)
    torch.cuda.synchronize()
    geo = sm.match_geometry(1)
    assert geo["kernel"] == "fast_split" and geo["band_rows"] == fd.FA_TH_SMALL_TALL, geo
    sm.route_info()
    reports = _reports(capfd)
    m, win, model = fd.report([wta], Dd, fd.FA_TH_SMALL_TALL, fd.small_nd(Dd), [0], "latency")
    print(f"latency {h} x {w}: {m}/{win} = {float(model):.4f}; printed {reports}")
    assert win * ((Dd + 1) // 2) <= 900
    assert len(reports) == 1, reports
    assert abs(reports[0][0] - float(model)) <= TOL, (reports[0][0], float(model), m, win)
    assert np.array_equal(out.cpu().numpy(), want)


def _silent_call(cd, oracle_omp, capfd, cus, content, dmin=0):
    K, h, w, Dd = 2, 96, 190, 64
    n = fd.throughput_pairs(h, w, cus, False)
    cfg, ocfg = parity._cfgs(cd, h * K, w * K, K, dmin, dmin + Dd * K - 1)
    pair = _oracle(oracle_omp, ocfg, K, h, w, Dd, content, dmin)
    tl, tr = _batch([pair], n)
    sm = cd.StereoMatching(cfg, max_batch=n, overlap_min_pairs=-1)
    capfd.readouterr()
    return sm, tl, tr, pair, n


def test_forced_sparse_form_does_not_report(cd, oracle_omp, hints_env, capfd, cus):
    """SMX_FAST_DENSE=0: a forced form leaves the switch alone (plan_range: `f.opt.fast_dense < 0`)."""
    hints_env.setenv("SMX_FAST_DENSE", "0")
    sm, tl, tr, pair, n = _silent_call(cd, oracle_omp, capfd, cus, "noise")
    out, info, reports = _run(sm, tl, tr, False, capfd)
    assert sm.match_geometry(n)["kernel"] == "fast_window"
    assert reports == [] and info["fast_dense"] == 0, (reports, info)
    assert np.array_equal(out[0].cpu().numpy(), pair[2]) and np.array_equal(out[n - 1].cpu().numpy(), pair[2])


def test_min_disparity_above_zero_does_not_report(cd, oracle_omp, hints_env, capfd, cus):
    """min_disparity > 0: the fast kernel stops after the arg-max (pass1_only), there is no second pass to report."""
    sm, tl, tr, pair, n = _silent_call(cd, oracle_omp, capfd, cus, "noise", dmin=16)
    out, info, reports = _run(sm, tl, tr, False, capfd)
    assert sm.match_geometry(n)["kernel"] == "fast_window"
    assert reports == [] and info["fast_dense"] == 0, (reports, info)
    assert np.array_equal(out[0].cpu().numpy(), pair[2]) and np.array_equal(out[n - 1].cpu().numpy(), pair[2])


def test_dense_form_does_not_report(cd, oracle_omp, hints_env, capfd, cus):
    """The second noise call of an engine runs the dense form (the first one's report is above 0.10), which reports nothing."""
    sm, tl, tr, pair, n = _silent_call(cd, oracle_omp, capfd, cus, "noise")
    out, info, reports = _run(sm, tl, tr, False, capfd)
    assert len(reports) == 1 and reports[0][0] > 0.10 and info["fast_dense"] == 1, (reports, info)
    assert np.array_equal(out[n - 1].cpu().numpy(), pair[2])
    out, info, reports = _run(sm, tl, tr, False, capfd)
    assert reports == [] and info["fast_dense"] == 1, (reports, info)
    assert np.array_equal(out[0].cpu().numpy(), pair[2]) and np.array_equal(out[n - 1].cpu().numpy(), pair[2])
