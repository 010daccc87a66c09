"""Intensity pyramids and camera tracking that reads them on the device (include/stereo_mi355x.h: smx_intensity_pyramid,
smx_track_camera_pyramid), bit for bit against the NumPy twin (tests/track_pyramid_ref.py) on the cases of
tests/track_pyramid_cases.py.  The pyramid: planes from 1 x 1 to wider than two workgroup tiles, one and three planes, one
to eight levels, NaNs, an infinity and a mask.  The tracker: the triples of tests/track_photo_cases.py through three levels,
levels below a stride's own, every sum of one iteration at each level, batches with the middle triple lost, Huber's weight
and its threshold, the edges of the tap rule at level 1, the wall that the plain photometric term cannot track, the bits
of smx_track_camera_photometric at level 0, the entry's behaviour (repeatability, an aliased pose, optional outputs, graph
capture behind the pyramid kernels, the argument checks), and the Python layer and the pipeline."""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import raycast_cases as cases                       # noqa: E402
import raycast_ref as rc                            # noqa: E402
import track_cases as tc                            # noqa: E402
import track_photo_cases as pc                      # noqa: E402
import track_photo_ref as tp                        # noqa: E402
import track_pyramid_cases as yc                    # noqa: E402
import track_pyramid_ref as ty                      # noqa: E402
import track_ref as tr                              # noqa: E402

f32 = np.float32
SMX_ERR_INVALID_ARG = -1


@pytest.fixture(scope="module")
def cd():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import cuda_depth
    return cuda_depth


def dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).cuda()      # a copy: the shared cases are read-only


def pose4(m):
    m = np.asarray(m, np.float64)
    return m if m.shape == (4, 4) else np.vstack([m, [0.0, 0.0, 0.0, 1.0]])


def bits32(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def batch_pyramid(pyramids):
    """The flat buffer of n one-plane pyramids (lists of [Hl, Wl]) as one pyramid of n planes."""
    return np.concatenate([np.stack([p[l] for p in pyramids]).astype(f32).reshape(-1) for l in range(len(pyramids[0]))])


# ---- 1. the pyramid -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", yc.PYRAMID_SHAPES)
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("masked", [False, True])
def test_intensity_pyramid(cd, n, shape, masked):
    planes, mask = yc.pyramid_planes(n, shape, masked)
    p, m = dev(planes), dev(mask)
    for levels in (1, 2, 3, 4, 8):                                    # 8 levels take 128 pixels down to one
        got = cd.intensity_pyramid(p, levels, m)
        want = yc.pyramid_expected(n, shape, levels, masked)
        assert len(got) == levels
        for l, (g, w) in enumerate(zip(got, want)):
            assert g.dtype == torch.float32 and tuple(g.shape) == w.shape, (levels, l)
            assert yc.same_planes(g.cpu().numpy(), w), f"{levels} levels, level {l}"
        assert got[-1].data_ptr() == got[0].data_ptr() + 4 * sum(g.numel() for g in got[:-1])
    assert want[7].shape[1:] == ((shape[0] + 127) // 128, (shape[1] + 127) // 128)
    if shape[0] * shape[1] > 8:
        assert np.isnan(want[1]).any() and (np.isfinite(want[1]).any() or shape[0] < 8)
    assert torch.equal(p.isnan(), dev(planes).isnan())                # the operands are read only
    one = cd.intensity_pyramid(p[0], 2, None if m is None else m[0])
    assert [tuple(t.shape) for t in one] == [w.shape[1:] for w in want[:2]] and yc.same_planes(one[1].cpu().numpy(), want[1][0])


def test_more_planes_than_the_grid_has_layers(cd):
    """65,537 planes on a grid of 65,535 layers: two workgroups reduce a second plane, through the same LDS."""
    n, shape = 65537, (5, 9)
    rng = np.random.default_rng(31)
    planes = rng.uniform(0.0, 255.0, (n,) + shape).astype(f32)
    planes[0, 2, 4] = planes[65535, 1, 1] = planes[65536, 4, 8] = np.nan
    got = cd.intensity_pyramid(dev(planes), 3)
    for l, (g, w) in enumerate(zip(got, ty.intensity_pyramid_ref(planes, 3))):
        assert yc.same_planes(g.cpu().numpy(), w), f"level {l}"


def test_intensity_pyramid_refusals(cd):
    import cuda_depth._native as native
    lib = native.LIB
    plane = torch.zeros((2, 5, 7), device="cuda")
    out = torch.zeros(lib.smx_intensity_pyramid_bytes(2, 5, 7, 3) // 4, device="cuda")
    assert out.numel() == 2 * (35 + 12 + 4)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    P, M, O = plane.data_ptr(), plane.data_ptr(), out.data_ptr()
    assert lib.smx_intensity_pyramid(0, 2, 5, 7, 3, P, None, O, s) == 0, native.last_error()
    for args, text in (((2, 5, 7, 3, None, None, O, s), "non-NULL"), ((2, 5, 7, 3, P, None, None, s), "non-NULL"),
                       ((0, 5, 7, 3, P, None, O, s), "n >= 1"), ((2, 0, 7, 3, P, None, O, s), "H"),
                       ((2, 5, 40000, 3, P, None, O, s), "W"), ((2, 32768, 32768, 3, P, None, O, s), "2^30"),
                       ((2, 5, 7, 0, P, None, O, s), "levels"), ((2, 5, 7, 9, P, None, O, s), "levels"),
                       ((2, 5, 7, 3, O + 4 * 80, None, O, s), "overlap"), ((2, 5, 7, 3, P, O + 4 * 101, O, s), "overlap"),
                       ((2, 5, 7, 3, P, M, O, native.STREAM_ENGINE.value), "caller stream")):
        assert lib.smx_intensity_pyramid(0, *args) == SMX_ERR_INVALID_ARG, args[:4]
        assert text in native.last_error() and "smx_intensity_pyramid" in native.last_error(), native.last_error()
    q = lib.smx_intensity_pyramid_bytes
    assert q(0, 5, 7, 3) == 0 and q(2, 5, 7, 0) == 0 and q(2, 5, 7, 9) == 0 and q(2, 32768, 32768, 1) == 0
    assert q(1, 1, 1, 8) == 32 and q(3, 37, 70, 1) == 4 * 3 * 37 * 70
    with pytest.raises(RuntimeError, match="float32"):
        cd.intensity_pyramid(plane.to(torch.float64), 2)
    with pytest.raises(RuntimeError, match="levels"):
        cd.intensity_pyramid(plane, 0)
    with pytest.raises(RuntimeError, match="mask_depth"):
        cd.intensity_pyramid(plane, 2, plane[:1])
    torch.cuda.synchronize()


# ---- 2. the tracker -----------------------------------------------------------------------------------------------------------------

class Direct:
    """One direct call of smx_track_camera_pyramid (or, with photometric=True, smx_track_camera_photometric on the same
    operands and level 0 of the pyramids), every operand its own tensor.  models: one dict per triple sharing Qm and Pm,
    each with "pyramid"; frame_pyramids: one list of levels per triple."""

    def __init__(self, disp, Q, starts, models, frame_pyramids, weight, max_difference, schedule, schedule_levels,
                 huber_delta=math.inf, conf=None, **params):
        import cuda_depth._native as native
        self.native = native
        self.n, self.H, self.W = disp.shape
        self.Hm, self.Wm = models[0]["depth"].shape
        self.Q, self.Qm, self.Pm = Q, models[0]["Qm"], models[0]["Pm"]
        self.disp, self.conf = dev(np.asarray(disp, f32)), dev(conf)
        self.depth = dev(np.stack([m["depth"] for m in models]))
        self.normals = dev(np.stack([m["normals"] for m in models]))
        self.c2w = dev(np.stack([m["c2w"] for m in models]))
        self.w2c = dev(np.stack([m["w2c"] for m in models]))
        self.levels = len(frame_pyramids[0])
        self.fpyr = dev(batch_pyramid(frame_pyramids))
        self.mpyr = dev(batch_pyramid([m["pyramid"] for m in models]))
        self.pose_in = dev(np.asarray(starts, f32))
        n = self.n
        self.pose_out = torch.empty((n, 3, 4), device="cuda")
        self.info = torch.empty((n, 4), dtype=torch.int32, device="cuda")
        self.rms = torch.empty((n,), device="cuda")
        self.sums = torch.empty((n, 33), dtype=torch.float64, device="cuda")
        self.pinfo = torch.empty((n, 2), dtype=torch.int32, device="cuda")
        self.prms = torch.empty((n,), device="cuda")
        self.ws = torch.empty(native.LIB.smx_track_camera_photometric_workspace_bytes(n, self.H, self.W), dtype=torch.uint8,
                              device="cuda")
        self.schedule = np.asarray(schedule, np.int32).reshape(-1, 2)
        self.schedule_levels = tuple(schedule_levels)
        self.weight, self.max_difference, self.huber = weight, max_difference, huber_delta
        self.params = dict(min_confidence=0.0, rot_eps=0.0, trans_eps=0.0)
        self.params.update(params)

    @classmethod
    def of_triples(cls, triples, schedule=yc.SCHEDULE, schedule_levels=yc.SCHEDULE_LEVELS, levels=yc.LEVELS,
                   huber_delta=math.inf, weight=pc.WEIGHT, clean=False, **extra):
        kw = dict(tc.PARAMS)
        kw.update(extra)
        frames = [tc.frame(v, s, k, c) for v, s, k, c, _ in triples]
        conf = triples[0][3]
        if conf:
            kw.setdefault("min_confidence", 0.1)
        return cls(np.stack([fr[0] for fr in frames]), frames[0][1], np.stack([tc.start_pose(t[0]) for t in triples]),
                   [yc.model(v, m, levels, clean) for v, _, _, _, m in triples],
                   [yc.frame_pyramid(s, k, levels) for _, s, k, _, _ in triples], weight, pc.MAX_DIFFERENCE, schedule,
                   schedule_levels, huber_delta, conf=np.stack([fr[3] for fr in frames]) if conf else None, **kw)

    def call(self, stream=None, photometric=False, **over):
        """The status of the call with the named arguments replaced."""
        f16 = lambda m: (C.c_float * 16)(*np.asarray(m, f32).reshape(-1).tolist())  # noqa: E731
        ptr = lambda t: None if t is None else (t if isinstance(t, int) else t.data_ptr())  # noqa: E731
        p = self.params
        a = dict(n=self.n, H=self.H, W=self.W, disp=self.disp, confidence=self.conf, Q=self.Q,
                 min_confidence=p["min_confidence"], z_min=p["depth_range"][0], z_max=p["depth_range"][1], invalid=-1.0,
                 Hm=self.Hm, Wm=self.Wm, depth=self.depth, normals=self.normals, Qm=self.Qm, Pm=self.Pm, c2w=self.c2w,
                 w2c=self.w2c, pose_in=self.pose_in, schedule=self.schedule, max_distance=p["max_distance"],
                 min_inliers=p["min_inliers"], min_pivot=p["min_pivot"], rot_eps=p["rot_eps"], trans_eps=p["trans_eps"],
                 fpyr=self.fpyr, mpyr=self.mpyr, levels=self.levels, schedule_levels=self.schedule_levels,
                 weight=self.weight, max_difference=self.max_difference, huber=self.huber,
                 pose_out=self.pose_out, info=self.info, rms=self.rms, sums=self.sums, pinfo=self.pinfo, prms=self.prms,
                 ws=self.ws, ws_bytes=self.ws.numel(),
                 stream=torch.cuda.current_stream().cuda_stream if stream is None else stream)
        a.update(over)
        sched = None if a["schedule"] is None else np.asarray(a["schedule"], np.int32).reshape(-1)
        pairs = over.get("pairs", 0 if sched is None else sched.size // 2)
        sc = None if sched is None else (C.c_int32 * max(sched.size, 1))(*sched.tolist())
        lv = a["schedule_levels"]
        lv = None if lv is None else (C.c_int32 * max(len(lv), 1))(*lv)
        Q, Qm, Pm = (None if a[k] is None else f16(a[k]) for k in ("Q", "Qm", "Pm"))
        head = (0, a["n"], a["H"], a["W"], ptr(a["disp"]), ptr(a["confidence"]), Q, a["min_confidence"], a["z_min"],
                a["z_max"], a["invalid"], a["Hm"], a["Wm"], ptr(a["depth"]), ptr(a["normals"]), Qm, Pm, ptr(a["c2w"]),
                ptr(a["w2c"]), ptr(a["pose_in"]), pairs, sc, a["max_distance"], a["min_inliers"], a["min_pivot"],
                a["rot_eps"], a["trans_eps"])
        tail = (ptr(a["pose_out"]), ptr(a["info"]), ptr(a["rms"]), ptr(a["sums"]), ptr(a["pinfo"]), ptr(a["prms"]),
                ptr(a["ws"]), a["ws_bytes"], C.c_void_p(a["stream"]))
        if photometric:
            return self.native.LIB.smx_track_camera_photometric(*head, ptr(a["fpyr"]), ptr(a["mpyr"]), a["weight"],
                                                                a["max_difference"], *tail)
        return self.native.LIB.smx_track_camera_pyramid(*head, ptr(a["fpyr"]), ptr(a["mpyr"]), a["levels"], lv, a["weight"],
                                                        a["max_difference"], a["huber"], *tail)

    def run(self, **over):
        assert self.call(**over) == 0, self.native.last_error()
        return self.results()

    def results(self, pose=None):
        torch.cuda.synchronize()
        pose = (self.pose_out if pose is None else pose).cpu().numpy()
        return [{"pose": pose[i], "info": self.info[i].cpu().numpy(), "rms": self.rms[i].cpu().numpy(),
                 "sums": self.sums[i].cpu().numpy(), "pinfo": self.pinfo[i].cpu().numpy(), "prms": self.prms[i].cpu().numpy()}
                for i in range(self.n)]


@pytest.mark.parametrize("shape", tc.FRAME_SHAPES)
def test_the_schedule_through_three_levels(cd, shape):
    want = yc.expected("outside", shape)
    assert want["info"][0] == 0 and want["info"][1] == 7 and want["pinfo"][0] > 100
    got = Direct.of_triples([("outside", shape, 0, False, False)]).run()
    yc.assert_same(got[0], want, f"{shape}")


@pytest.mark.parametrize("schedule, schedule_levels", [(((4, 2),), (1,)), (((6, 2),), (1,)), (((4, 1), (1, 1)), (0, 0))])
def test_levels_below_the_strides_own(cd, schedule, schedule_levels):
    shape = tc.FRAME_SHAPES[0]
    want = yc.expected("left", shape, 1, schedule=schedule, schedule_levels=schedule_levels)
    assert want["pinfo"][0] > 0
    got = Direct.of_triples([("left", shape, 1, False, False)], schedule, schedule_levels).run()
    yc.assert_same(got[0], want, f"{schedule} at {schedule_levels}")


@pytest.mark.parametrize("shape", tc.FRAME_SHAPES)
@pytest.mark.parametrize("level", [0, 1, 2])
def test_every_sum_of_one_iteration_at_each_level(cd, level, shape):
    schedule = ((1 << level, 1),)
    want = yc.expected("left", shape, 1, schedule=schedule, schedule_levels=(level,), huber_delta=yc.HUBER, clean=True)
    assert np.count_nonzero(want["sums"]) == 33 and want["pinfo"][0] >= 12
    got = Direct.of_triples([("left", shape, 1, False, False)], schedule, (level,), huber_delta=yc.HUBER, clean=True).run()
    yc.assert_same(got[0], want, f"level {level} {shape}")


@pytest.mark.parametrize("confidence", [False, True])
@pytest.mark.parametrize("huber_delta", [math.inf, yc.HUBER])
def test_three_triples_with_the_middle_one_lost(cd, confidence, huber_delta):
    shape = tc.FRAME_SHAPES[0]
    triples = [("outside", shape, 0, confidence, False), ("left", shape, 1, confidence, True),
               ("left", shape, 2, confidence, False)]
    want = [yc.expected(v, s, k, c, m, huber_delta=huber_delta) for v, s, k, c, m in triples]
    assert [int(w["info"][0]) for w in want] == [0, 1, 0]
    got = Direct.of_triples(triples, huber_delta=huber_delta).run()
    for g, w, t in zip(got, want, triples):
        yc.assert_same(g, w, str(t))
    assert np.array_equal(bits32(got[1]["pose"]), bits32(tc.start_pose("left")))
    alone = Direct.of_triples(triples[2:], huber_delta=huber_delta).run()   # n = 1: the same bits
    yc.assert_same(alone[0], want[2], "n = 1")


@pytest.mark.parametrize("delta", [3.0, 2.0, math.inf])
def test_hubers_threshold(cd, delta):
    disp, Q, start, m, frame, weight, max_difference = yc.huber_case()
    got = Direct(disp[None], Q, start[None], [m], [frame], weight, max_difference, ((1, 1),), (0,), delta,
                 **pc.EDGE_PARAMS).run()[0]
    yc.assert_same(got, yc.huber_expected(delta), f"delta {delta}")
    assert got["pinfo"].tolist() == [1, 0]
    assert got["sums"][31] == (float(f32(2.0) / f32(3.0)) if delta == 2.0 else 1.0)     # |e| == delta weighs 1


@pytest.mark.parametrize("name", yc.EDGE_NAMES)
def test_the_edges_of_the_tap_rule_at_level_1(cd, name):
    disp, Q, start, m, frame, weight, max_difference = yc.edge_case(name)
    got = Direct(disp[None], Q, start[None], [m], [frame], weight, max_difference, ((2, 1),), (1,), **yc.EDGE_PARAMS).run()[0]
    yc.assert_same(got, yc.edge_expected(name), name)
    count = yc.EDGE_COUNTS[name]
    assert got["info"][2] == 1 and got["pinfo"].tolist() == [count, 1 - count]


def test_the_wall_from_eight_pixels_off(cd):
    d, Q, inten, pyr = yc.wall_frame()
    _, photo, want = yc.wall_expected()
    run = Direct(d[None], Q, yc.wall_start()[None], [yc.wall_model()], [pyr], yc.WALL_WEIGHT, yc.WALL_MAX_DIFFERENCE,
                 yc.WALL_SCHEDULE, yc.WALL_SCHEDULE_LEVELS, yc.WALL_HUBER, **yc.WALL_PARAMS)
    got = run.run()[0]
    yc.assert_same(got, want, "wall")
    true = yc.wall_true_pose()
    m0, d0 = tr.pose_error(yc.wall_start(), true)
    m1, d1 = tr.pose_error(got["pose"], true)
    # the joint entry on the same operands (level 0 of the pyramids; the wall has a surface at every pixel)
    assert run.call(photometric=True) == 0, run.native.last_error()
    plain = run.results()[0]
    pc.assert_same(plain, photo, "wall, photometric entry")
    m2, d2 = tr.pose_error(plain["pose"], true)
    print(f"wall: start {m0:.4f} m {d0:.2f} deg; pyramid {m1:.4f} m {d1:.2f} deg; photometric {m2:.4f} m {d2:.2f} deg")
    assert got["info"][0] == 0 and m1 < 0.1 * m0 and m2 > 0.5 * m0


@pytest.mark.parametrize("confidence", [False, True])
def test_level_0_without_huber_is_the_photometric_entry(cd, confidence):
    """Pyramids built on the device, the model's masked by its depth: smx_track_camera_photometric's bits on the planes."""
    shape = tc.FRAME_SHAPES[0]
    triples = [("outside", shape, 0, confidence, False), ("left", shape, 1, confidence, True),
               ("left", shape, 2, confidence, False)]
    d = Direct.of_triples(triples, tr.DEFAULT_SCHEDULE, (0, 0, 0))
    fint = dev(np.stack([pc.frame_intensity(s, k) for _, s, k, _, _ in triples]))
    mint = dev(np.stack([pc.model(v, m)["intensity"] for v, _, _, _, m in triples]))
    fl, ml = cd.intensity_pyramid(fint, yc.LEVELS), cd.intensity_pyramid(mint, yc.LEVELS, d.depth)
    got = d.run(fpyr=fl[0], mpyr=ml[0])
    for g, (v, s, k, c, m) in zip(got, triples):
        pc.assert_same(g, pc.expected(v, s, k, c, m), f"{v} {k} against the photometric twin")
    assert got[0]["pinfo"][0] > 0 and got[2]["pinfo"][0] > 0
    outs = [t.clone() for t in (d.pose_out, d.info, d.rms, d.sums, d.pinfo, d.prms)]
    for t in (d.pose_out, d.info, d.rms, d.sums, d.pinfo, d.prms):
        t.zero_()
    assert d.call(photometric=True, fpyr=fint, mpyr=mint) == 0, d.native.last_error()
    torch.cuda.synchronize()
    for a, b in zip(outs, (d.pose_out, d.info, d.rms, d.sums, d.pinfo, d.prms)):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


# ---- 3. the entry's behaviour -------------------------------------------------------------------------------------------------------

TWO = [("outside", tc.FRAME_SHAPES[0], 0, False, False), ("left", tc.FRAME_SHAPES[0], 1, False, False)]


def test_the_same_call_twice_an_aliased_pose_and_optional_outputs_left_out(cd):
    d = Direct.of_triples(TWO, huber_delta=yc.HUBER)
    want = [yc.expected(v, s, k, huber_delta=yc.HUBER) for v, s, k, *_ in TWO]
    first = d.run()
    for t in (d.pose_out, d.info, d.rms, d.sums, d.pinfo, d.prms):
        t.zero_()
    for a, b, w in zip(first, d.run(), want):
        yc.assert_same(a, w, "first call")
        yc.assert_same(b, a, "second call")
    pose = d.pose_in.clone()
    assert d.call(pose_in=pose, pose_out=pose, info=None, rms=None, sums=None, pinfo=None, prms=None) == 0, d.native.last_error()
    torch.cuda.synchronize()
    for i, w in enumerate(want):
        assert np.array_equal(bits32(pose[i].cpu().numpy()), bits32(w["pose"])), "aliased pose"
    for keep in ("pinfo", "prms"):                                     # each optional output on its own
        over = dict(info=None, rms=None, sums=None, pinfo=None, prms=None)
        del over[keep]
        for t in (d.pinfo, d.prms):
            t.zero_()
        assert d.call(**over) == 0, d.native.last_error()
        torch.cuda.synchronize()
        for i, w in enumerate(want):
            if keep == "pinfo":
                assert d.pinfo[i].tolist() == w["pinfo"].tolist()
            else:
                assert np.array_equal(bits32(d.prms[i].cpu().numpy()), bits32(w["prms"]))


def test_graph_capture_of_both_pyramids_then_track(cd):
    import cuda_depth._native as native
    lib = native.LIB
    d = Direct.of_triples(TWO, huber_delta=yc.HUBER)
    want = [yc.expected(v, s, k, huber_delta=yc.HUBER) for v, s, k, *_ in TWO]
    fint = dev(np.stack([pc.frame_intensity(s, k) for _, s, k, _, _ in TWO]))
    mint = dev(np.stack([pc.model(v)["intensity"] for v, *_ in TWO]))
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        sp = C.c_void_p(s.cuda_stream)
        assert lib.smx_intensity_pyramid(0, 2, d.H, d.W, yc.LEVELS, fint.data_ptr(), None, d.fpyr.data_ptr(), sp) == 0
        assert lib.smx_intensity_pyramid(0, 2, d.Hm, d.Wm, yc.LEVELS, mint.data_ptr(), d.depth.data_ptr(), d.mpyr.data_ptr(),
                                         sp) == 0, native.last_error()
        assert d.call(stream=s.cuda_stream) == 0, native.last_error()
    torch.cuda.synchronize()
    for replay in range(2):
        for t in (d.pose_out, d.info, d.rms, d.sums, d.pinfo, d.prms, d.fpyr, d.mpyr):
            t.zero_()
        torch.cuda.synchronize()
        graph.replay()
        for g, w in zip(d.results(), want):
            yc.assert_same(g, w, f"replay {replay}")


def test_argument_checks(cd):
    d = Direct.of_triples(TWO, schedule=((2, 1),), schedule_levels=(1,))
    lib, native = d.native.LIB, d.native
    assert d.call() == 0, native.last_error()
    H, W = d.H, d.W
    big = torch.empty(d.ws.numel() + 256, dtype=torch.uint8, device="cuda")
    level2 = 4 * 2 * (37 * 70 + 19 * 35)                              # where level 2 of the frame pyramid starts
    bad = [
        (dict(fpyr=None), "frame_pyramid"), (dict(mpyr=None), "model_pyramid"),
        (dict(disp=None), "disp"), (dict(Q=None), "non-NULL"), (dict(depth=None), "model_depth"),
        (dict(normals=None), "model_normals"), (dict(Qm=None), "Qm"), (dict(Pm=None), "Pm"), (dict(c2w=None), "non-NULL"),
        (dict(w2c=None), "non-NULL"), (dict(pose_in=None), "pose_in"), (dict(pose_out=None), "pose_out"),
        (dict(ws=None), "workspace"), (dict(n=0), "n >= 1"), (dict(H=0), "H"), (dict(W=40000), "W"),
        (dict(H=32768, W=32768, n=2), "2^30"), (dict(H=8192, W=8192, n=1), "tiles"), (dict(Hm=0), "Hm"),
        (dict(Wm=40000), "Wm"), (dict(Q=np.where(np.eye(4) > 0, np.nan, d.Q)), "Q["),
        (dict(Pm=np.full((4, 4), np.inf, f32)), "Pm["), (dict(Qm=np.eye(4, dtype=f32)), "Qm's ray"),
        (dict(z_min=2.0, z_max=1.0), "z_min"), (dict(min_confidence=math.inf), "min_confidence"),
        (dict(invalid=math.nan), "finite"), (dict(schedule=[[2, 1]] * 9, schedule_levels=(1,) * 9), "schedule_pairs"),
        (dict(schedule=None, pairs=1), "schedule"), (dict(schedule=[[0, 1]]), "stride"),
        (dict(schedule=[[2, -1]]), "iteration"), (dict(schedule=[[2, 33], [2, 32]], schedule_levels=(1, 1)), "in total"),
        (dict(max_distance=0.0), "max_distance"), (dict(min_inliers=0), "min_inliers"), (dict(min_pivot=-1.0), "min_pivot"),
        (dict(rot_eps=-1.0), "rot_eps"), (dict(trans_eps=math.nan), "trans_eps"),
        (dict(weight=-0.5), "photometric_weight"), (dict(weight=math.nan), "photometric_weight"),
        (dict(max_difference=0.0), "max_intensity_difference"), (dict(max_difference=math.nan), "max_intensity_difference"),
        (dict(levels=0), "levels"), (dict(levels=9), "levels"), (dict(schedule_levels=None), "schedule_levels"),
        (dict(schedule_levels=(3,)), "a schedule level"), (dict(schedule_levels=(-1,)), "a schedule level"),
        (dict(schedule_levels=(2,)), "divisible"), (dict(schedule=[[3, 1]]), "divisible"),
        (dict(schedule=[[4, 1], [1, 1]], schedule_levels=(2, 1)), "divisible"),
        (dict(huber=0.0), "huber_delta"), (dict(huber=-1.0), "huber_delta"), (dict(huber=math.nan), "huber_delta"),
        (dict(huber=-math.inf), "huber_delta"),
        (dict(ws_bytes=d.ws.numel() - 1), "workspace_bytes"),
        (dict(ws_bytes=lib.smx_track_camera_workspace_bytes(2, H, W)), "smx_track_camera_photometric_workspace_bytes"),
        (dict(ws=big.data_ptr() + 64), "aligned"),
        (dict(pose_out=d.pose_in.data_ptr() + 16), "overlaps an input"),
        (dict(pose_out=d.c2w), "overlaps an input"), (dict(info=d.disp), "overlaps an input"),
        (dict(pinfo=d.fpyr), "overlaps an input"), (dict(prms=d.mpyr), "overlaps an input"),
        (dict(pinfo=d.fpyr.data_ptr() + level2), "overlaps an input"),    # past level 0: the whole pyramid is an input
        (dict(rms=d.mpyr.data_ptr() + 4 * (d.mpyr.numel() - 1)), "overlaps an input"),
        (dict(rms=d.pose_out), "two outputs"), (dict(sums=d.ws), "two outputs"),
        (dict(pinfo=d.pose_out), "two outputs"), (dict(prms=d.pinfo), "two outputs"),
    ]
    for over, text in bad:
        rcode = d.call(**over)
        assert rcode == SMX_ERR_INVALID_ARG, (over.keys(), rcode)
        assert text in native.last_error(), (list(over), native.last_error())
        assert "smx_track_camera_pyramid" in native.last_error() or "invalid" in over, (list(over), native.last_error())
    assert d.call(huber=math.inf) == 0 and d.call(huber=1e-30) == 0, native.last_error()
    assert d.call(schedule=[], schedule_levels=None) == 0, native.last_error()      # no pairs: no levels to read
    assert d.call(schedule=[[4, 1], [6, 1], [2, 0]], schedule_levels=(2, 1, 0)) == 0, native.last_error()
    assert d.call(stream=native.STREAM_ENGINE.value) == SMX_ERR_INVALID_ARG and "caller stream" in native.last_error()
    torch.cuda.synchronize()


# ---- 4. the Python layer and the pipeline ---------------------------------------------------------------------------------------

def as_dict(res, i=None):
    """A TrackingResult (its triple i when batched) in the twin's form."""
    torch.cuda.synchronize()
    pick = (lambda t: t) if i is None else (lambda t: t[i])
    n = {k: pick(getattr(res, k)).cpu().numpy() for k in ("pose", "lost", "iterations", "inliers", "accepted", "rms",
                                                          "normal_equations", "photometric_inliers", "photometric_rms")}
    return {"pose": n["pose"][:3], "info": np.array([int(n["lost"]), n["iterations"], n["inliers"], n["accepted"]]),
            "rms": n["rms"], "sums": n["normal_equations"], "prms": n["photometric_rms"],
            "pinfo": np.array([n["photometric_inliers"], n["inliers"] - n["photometric_inliers"]])}


def test_track_camera_with_pyramid_levels(cd):
    shape, view = tc.FRAME_SHAPES[0], "outside"
    d, Q, _, _ = tc.frame(view, shape)
    m = yc.model(view)
    start, mpose = pose4(tc.start_pose(view)), tc.model_pose(view)
    rv = cd.RenderedView(disparity=dev(m["depth"]), depth=dev(m["depth"]), normals=dev(m["normals"]))
    kw = dict(model_Q=m["Qm"], model_intensity=dev(m["intensity"]), photometric_weight=pc.WEIGHT,
              max_intensity_difference=pc.MAX_DIFFERENCE, image=dev(pc.frame_intensity(shape, 0)), **tc.PARAMS)
    # the default levels of the default schedule: (2, 1, 0)
    res = cd.track_camera(dev(d), Q, start, rv, mpose, pyramid_levels=3, huber_delta=yc.HUBER, **kw)
    want = yc.expected(view, shape, schedule=tr.DEFAULT_SCHEDULE, huber_delta=yc.HUBER)
    assert want["info"][0] == 0 and want["pinfo"][0] > 100
    assert res.pose.shape == (4, 4) and res.normal_equations.shape == (33,)
    yc.assert_same(as_dict(res), want, "default levels")
    # two levels cap the stride-4 pair at level 1; given levels; batched
    res = cd.track_camera(dev(d), Q, start, rv, mpose, pyramid_levels=2, **kw)
    yc.assert_same(as_dict(res), yc.expected(view, shape, schedule=tr.DEFAULT_SCHEDULE, schedule_levels=(1, 1, 0), levels=2),
                   "two levels")
    rvb = cd.RenderedView(disparity=dev(m["depth"])[None], depth=dev(m["depth"])[None], normals=dev(m["normals"])[None])
    kwb = dict(kw, model_intensity=kw["model_intensity"][None], image=kw["image"][None])
    res = cd.track_camera(dev(d)[None], Q, start[None], rvb, mpose[None], pyramid_levels=3, schedule=yc.SCHEDULE,
                          schedule_levels=(1, 0, 0), **kwb)
    yc.assert_same(as_dict(res, 0), yc.expected(view, shape, schedule_levels=(1, 0, 0)), "given levels, batched")
    # one level, no robust weights: the photometric entry's bits; without pyramid_levels the call is what it was
    one = cd.track_camera(dev(d), Q, start, rv, mpose, pyramid_levels=1, **kw)
    old = cd.track_camera(dev(d), Q, start, rv, mpose, **kw)
    pc.assert_same(as_dict(one), pc.expected(view, shape), "one level")
    pc.assert_same(as_dict(old), pc.expected(view, shape), "pyramid_levels=None")
    # without an image the geometric entry runs, whatever the levels
    geo = cd.track_camera(dev(d), Q, start, rv, mpose, model_Q=m["Qm"], pyramid_levels=3, **tc.PARAMS)
    torch.cuda.synchronize()
    assert geo.photometric_inliers is None and geo.normal_equations.shape == (30,)
    assert np.array_equal(bits32(geo.pose.cpu().numpy()[:3]), bits32(tc.expected(view, shape)["pose"]))
    for bad, text in ((dict(pyramid_levels=0), "pyramid_levels"), (dict(pyramid_levels=9), "pyramid_levels"),
                      (dict(pyramid_levels=2.0), "pyramid_levels"), (dict(huber_delta=5.0), "need pyramid_levels"),
                      (dict(schedule_levels=(0, 0, 0)), "need pyramid_levels"),
                      (dict(pyramid_levels=3, huber_delta=0.0), "huber_delta"),
                      (dict(pyramid_levels=3, huber_delta=math.nan), "huber_delta"),
                      (dict(pyramid_levels=3, schedule_levels=(0, 0)), "one level per schedule pair"),
                      (dict(pyramid_levels=3, schedule_levels=(3, 1, 0)), "schedule level"),
                      (dict(pyramid_levels=3, schedule_levels=(2, 2, 0)), "schedule level")):
        with pytest.raises(RuntimeError, match=text):
            cd.track_camera(dev(d), Q, start, rv, mpose, **dict(kw, **bad))


@pytest.fixture(scope="module")
def volume(cd):
    state = cases.fused_state()
    vol = cd.TSDFVolume(cases.DIMS, cases.VS, cases.ORIGIN)
    vol.tsdf.copy_(dev(state["tsdf"]))
    vol.weight.copy_(dev(state["weight"]))
    vol.color.copy_(dev(state["color"]))
    return vol


def test_volume_track_with_pyramid_levels(cd, volume):
    shape = tc.FRAME_SHAPES[1]
    d, Q, _, _ = tc.frame("outside", shape)
    start = pose4(tc.start_pose("outside"))
    rgb = pc.frame_image(shape, 0)
    res = volume.track(dev(d), Q, start, render_depth_range=cases.DEPTH_RANGE, image=dev(rgb), photometric_weight=pc.WEIGHT,
                       max_intensity_difference=255.0, pyramid_levels=3, huber_delta=40.0, **tc.PARAMS)
    view = rc.raycast_ref(cases.fused_state(), cases.DIMS, cases.ORIGIN, cases.VS, Q, rc.view_pose(start), shape,
                          depth_range=cases.DEPTH_RANGE)
    m = tr.model_view(view["depth"][0], view["normals"][0], Q, start)
    m["pyramid"] = ty.intensity_pyramid_ref(tp.intensity_planes_ref(view["colors"], 3)[0], 3, m["depth"])
    frame = ty.intensity_pyramid_ref(tp.intensity_planes_ref(rgb[None], 3)[0], 3)
    want = ty.track_pyramid_ref(d, Q, start[:3], m, frame, pc.WEIGHT, huber_delta=40.0, max_difference=255.0, **tc.PARAMS)
    assert want["info"][0] == 0 and want["pinfo"][0] > 100
    yc.assert_same(as_dict(res), want, "TSDFVolume.track(pyramid_levels=3)")


def test_pipeline_passes_the_pyramid_arguments_to_the_tracker(cd):
    from pipeline import DepthEstimationPipeline, DepthEstimationPipelineConfig
    H, W = tc.SEQ_SHAPE
    Q, frames, poses = tc.sequence()
    order = (0, 1, 2)
    images = [torch.from_numpy(np.array(pc.frame_image((H, W), i))) for i in order]
    plain = dict(tc.SEQ_ARGS, photometric_weight=pc.WEIGHT, max_intensity_difference=255.0)
    targs = dict(plain, pyramid_levels=3, huber_delta=40.0)
    cfg = DepthEstimationPipelineConfig(image_shape=(H, W), min_disparity=0, max_disparity=15, stereo_matching_backend="cuda")
    vol = cd.TSDFVolume(cases.DIMS, cases.VS, cases.ORIGIN)
    pipe = DepthEstimationPipeline(cfg, reprojection_matrix=Q, tsdf_volume=vol, point_cloud_depth_range=tc.SEQ_RANGE,
                                   track_camera=True, initial_pose=poses[0], tracking_args=targs)
    maps = iter([dev(frames[i]) for i in order])
    pipe._stereo_matching.process = lambda left, right: next(maps)      # the frames' maps are the sequence's, not matched
    got = []
    for image in images:
        res = pipe.process(image, image)
        got.append((res.camera_pose, res.tracking_lost))
    # the same steps by hand, and the second frame without the pyramid arguments
    vol2, last = cd.TSDFVolume(cases.DIMS, cases.VS, cases.ORIGIN), None
    for i, image, (pose, lost) in zip(order, images, got):
        if last is None:
            last, found_lost = np.array(poses[0], np.float64), False
        else:
            found = vol2.track(dev(frames[i]), Q, last, depth_range=tc.SEQ_RANGE, image=image.cuda(), **targs)
            if i == 1:
                other = vol2.track(dev(frames[i]), Q, last, depth_range=tc.SEQ_RANGE, image=image.cuda(), **plain)
                assert not torch.equal(other.pose, found.pose), "the pyramid arguments took part"
            found_lost = bool(found.lost)
            assert int(found.photometric_inliers) > 100
            last = last if found_lost else found.pose.cpu().numpy().astype(np.float64)
        assert found_lost is lost and np.array_equal(last, pose), f"frame {i}"
        if not found_lost:
            vol2.integrate(dev(frames[i]), Q, last, image=image.cuda(), depth_range=tc.SEQ_RANGE)
    assert [lost for _, lost in got] == [False, False, False]
    assert torch.equal(vol2.tsdf, vol.tsdf) and torch.equal(vol2.weight, vol.weight) and torch.equal(vol2.color, vol.color)
