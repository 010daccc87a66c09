"""Camera tracking on the device (include/stereo_mi355x.h: smx_track_camera), bit for bit against the NumPy twin
(tests/track_ref.py) on the triples of tests/track_cases.py: the 37 x 29 x 41 volume, model views rendered by the library
at 33 x 45, noisy frames at 37 x 70 (wider than one 64-column tile, no multiple of it or of the 4 tile rows) and 33 x 45.
Strides 1, 2 and 3, one and three triples per call with the middle one lost, confidence maps with zeros and NaNs, an
aliased pose, an early stop, zero iterations, optional outputs left out, the thirty sums, repeatability, graph capture of
a render followed by a track, the argument checks, and the pipeline's track_camera."""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import raycast_cases as cases                       # noqa: E402
import raycast_ref as rc                            # noqa: E402
import track_cases as tc                            # noqa: E402
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
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def volume(cd):
    state = cases.fused_state()
    vol = cd.TSDFVolume(cases.DIMS, cases.VS, cases.ORIGIN)
    vol.tsdf.copy_(dev(state["tsdf"]))
    vol.weight.copy_(dev(state["weight"]))
    vol.color.copy_(dev(state["color"]))
    return vol


def pose4(m):
    m = np.asarray(m, np.float64)
    return m if m.shape == (4, 4) else np.vstack([m, [0.0, 0.0, 0.0, 1.0]])


@pytest.fixture(scope="module")
def views(cd, volume):
    """view name -> the library's rendering (depth, normals) at the model shape, which must have the twin's bits."""
    names = tc.MODEL_VIEWS
    got = volume.render(cases.q_of("kitti", tc.MODEL_SHAPE), np.stack([tc.model_pose(v) for v in names]), tc.MODEL_SHAPE,
                        depth_range=cases.DEPTH_RANGE, colors=False)
    torch.cuda.synchronize()
    out = {}
    for i, v in enumerate(names):
        want = tc.model(v)
        cases.assert_same({"depth": got.depth[i:i + 1].cpu().numpy(), "normals": got.normals[i:i + 1].cpu().numpy()},
                          {"depth": want["depth"][None], "normals": want["normals"][None]}, f"model view {v}")
        out[v] = (got.depth[i].clone(), got.normals[i].clone())
    return out


def track(cd, views, triples, schedule=tr.DEFAULT_SCHEDULE, batched=None, **extra):
    """triples: (view, shape, k, confidence, misses); returns (one dict per triple, the TrackingResult)."""
    kw = dict(tc.PARAMS)
    kw.update(extra)
    frames = [tc.frame(v, s, k, c) for v, s, k, c, _ in triples]
    conf = triples[0][3]
    if conf:
        kw.setdefault("min_confidence", 0.1)
    depth = torch.stack([torch.full_like(views[v][0], math.nan) if m else views[v][0] for v, _, _, _, m in triples])
    normals = torch.stack([torch.zeros_like(views[v][1]) if m else views[v][1] for v, _, _, _, m in triples])
    disp = dev(np.stack([fr[0] for fr in frames]))
    cmap = dev(np.stack([fr[3] for fr in frames])) if conf else None
    start = np.stack([pose4(tc.start_pose(t[0])) for t in triples])
    mposes = np.stack([tc.model_pose(t[0]) for t in triples])
    batched = len(triples) > 1 if batched is None else batched
    if not batched:
        disp, depth, normals, start, mposes = disp[0], depth[0], normals[0], start[0], mposes[0]
        cmap = None if cmap is None else cmap[0]
    model = cd.RenderedView(disparity=depth, depth=depth.contiguous(), normals=normals.contiguous())
    res = cd.track_camera(disp.contiguous(), frames[0][1], start, model, mposes, model_Q=cases.q_of("kitti", tc.MODEL_SHAPE),
                          confidence=cmap, schedule=schedule, **kw)
    torch.cuda.synchronize()
    lead = (lambda t: t) if batched else (lambda t: t[None])
    pose, lost, its = lead(res.pose).cpu().numpy(), lead(res.lost).cpu().numpy(), lead(res.iterations).cpu().numpy()
    inl, acc = lead(res.inliers).cpu().numpy(), lead(res.accepted).cpu().numpy()
    rms, sums, information = lead(res.rms).cpu().numpy(), lead(res.normal_equations).cpu().numpy(), lead(res.information)
    assert pose.shape == (len(triples), 4, 4) and np.array_equal(pose[:, 3], np.tile([0, 0, 0, 1], (len(triples), 1)))
    assert information.shape == (len(triples), 6, 6) and information.dtype == torch.float64
    out = []
    for i in range(len(triples)):
        assert np.array_equal(information[i].cpu().numpy(), tr.information(sums[i]))
        out.append({"pose": pose[i, :3], "info": np.array([int(lost[i]), its[i], inl[i], acc[i]]), "rms": rms[i],
                    "sums": sums[i]})
    return out, res


@pytest.mark.parametrize("shape", tc.FRAME_SHAPES)
@pytest.mark.parametrize("stride", [1, 2, 3])
def test_two_iterations_at_each_stride(cd, views, shape, stride):
    schedule = ((stride, 2),)
    want = tc.expected("outside", shape, schedule=schedule)
    assert want["info"][0] == 0 and 2 * want["info"][2] >= want["info"][3] > 0       # the twin tracks this case
    got, res = track(cd, views, [("outside", shape, 0, False, False)], schedule)
    assert res.pose.shape == (4, 4) and res.lost.shape == () and res.information.shape == (6, 6)
    tc.assert_same(got[0], want, f"{shape} stride {stride}")


@pytest.mark.parametrize("shape", tc.FRAME_SHAPES)
def test_the_thirty_sums_of_one_iteration_at_stride_1(cd, views, shape):
    got, _ = track(cd, views, [("left", shape, 1, False, False)], ((1, 1),))
    want = tc.expected("left", shape, 1, schedule=((1, 1),))
    assert want["sums"][29] > 500 and np.count_nonzero(want["sums"]) == 30
    tc.assert_same(got[0], want, f"one iteration {shape}")


@pytest.mark.parametrize("confidence", [False, True])
def test_three_triples_with_the_middle_one_lost(cd, views, confidence):
    shape = tc.FRAME_SHAPES[0]
    triples = [("outside", shape, 0, confidence, False), ("left", shape, 1, confidence, True),
               ("left", shape, 2, confidence, False)]
    want = [tc.expected(v, s, k, c, m) for v, s, k, c, m in triples]
    assert [int(w["info"][0]) for w in want] == [0, 1, 0]
    assert all(2 * w["info"][2] >= w["info"][3] > 0 for w in (want[0], want[2]))
    if confidence:
        conf = tc.frame("outside", shape, 0, True)[3]
        assert (conf == 0).any() and np.isnan(conf).any()
    got, res = track(cd, views, triples)
    assert res.pose.shape == (3, 4, 4) and res.lost.tolist() == [False, True, False]
    for g, w, t in zip(got, want, triples):
        tc.assert_same(g, w, str(t))
    assert np.array_equal(got[1]["pose"].view(np.uint32), tc.start_pose("left").view(np.uint32))
    alone, _ = track(cd, views, triples[:1], batched=True)                          # n = 1: the same bits
    tc.assert_same(alone[0], want[0], "n = 1")


def test_a_tolerance_stops_the_schedule_early_and_zero_iterations_are_the_identity(cd, views):
    shape = tc.FRAME_SHAPES[1]
    eps = dict(rot_eps=2e-3, trans_eps=2e-3)
    want = tc.expected("outside", shape, **eps)
    assert 1 <= want["info"][1] < 19 and want["info"][0] == 0
    got, _ = track(cd, views, [("outside", shape, 0, False, False)], **eps)
    tc.assert_same(got[0], want, "early stop")
    assert got[0]["info"][1] < 19
    got, _ = track(cd, views, [("outside", shape, 0, False, False)], ())
    tc.assert_same(got[0], tc.expected("outside", shape, schedule=()), "zero iterations")
    assert got[0]["info"].tolist() == [0, 0, 0, 0] and np.isnan(got[0]["rms"]) and not got[0]["sums"].any()
    assert np.array_equal(got[0]["pose"].view(np.uint32), tc.start_pose("outside").view(np.uint32))


def test_the_same_call_twice_gives_the_same_bits(cd, views):
    triples = [("outside", tc.FRAME_SHAPES[0], 0, True, False), ("left", tc.FRAME_SHAPES[0], 1, True, False)]
    a, _ = track(cd, views, triples)
    b, _ = track(cd, views, triples)
    for x, y in zip(a, b):
        tc.assert_same(x, y, "second call")


class Direct:
    """One direct call of the C entry on the triples (outside, left) at 37 x 70, every operand its own tensor."""

    def __init__(self, cd, views, schedule=tr.DEFAULT_SCHEDULE):
        import cuda_depth._native as native
        self.native = native
        self.shape, self.model_shape = tc.FRAME_SHAPES[0], tc.MODEL_SHAPE
        self.triples = [("outside", self.shape, 0, False, False), ("left", self.shape, 1, False, False)]
        self.n = 2
        frames = [tc.frame(v, s, k, c) for v, s, k, c, _ in self.triples]
        models = [tc.model(v) for v, *_ in self.triples]
        self.Q, self.Qm, self.Pm = frames[0][1], models[0]["Qm"], models[0]["Pm"]
        self.disp = dev(np.stack([fr[0] for fr in frames]))
        self.depth = torch.stack([views[v][0] for v, *_ in self.triples]).contiguous()
        self.normals = torch.stack([views[v][1] for v, *_ in self.triples]).contiguous()
        self.c2w = dev(np.stack([m["c2w"] for m in models]))
        self.w2c = dev(np.stack([m["w2c"] for m in models]))
        self.pose_in = dev(np.stack([tc.start_pose(v) for v, *_ in self.triples]))
        self.pose_out = torch.empty((2, 3, 4), device="cuda")
        self.info = torch.empty((2, 4), dtype=torch.int32, device="cuda")
        self.rms = torch.empty((2,), device="cuda")
        self.sums = torch.empty((2, 30), dtype=torch.float64, device="cuda")
        H, W = self.shape
        self.ws = torch.empty(native.LIB.smx_track_camera_workspace_bytes(2, H, W), dtype=torch.uint8, device="cuda")
        self.schedule = np.asarray(schedule, np.int32).reshape(-1, 2)
        self.want = [tc.expected(v, s, k, schedule=schedule) for v, s, k, *_ in self.triples]

    @classmethod
    def of(cls, n, shape, model_shape, Q, Qm, Pm, schedule, **operands):
        """A direct call on operands of the caller's: disp, depth, normals, c2w, w2c, pose_in, pose_out, info, rms, sums
        and ws, all device tensors."""
        import cuda_depth._native as native
        d = cls.__new__(cls)
        d.native, d.n, d.shape, d.model_shape, d.Q, d.Qm, d.Pm = native, n, shape, model_shape, Q, Qm, Pm
        d.schedule = np.asarray(schedule, np.int32).reshape(-1, 2)
        for name in ("disp", "depth", "normals", "c2w", "w2c", "pose_in", "pose_out", "info", "rms", "sums", "ws"):
            setattr(d, name, operands.pop(name))
        assert not operands, list(operands)
        return d

    def call(self, stream=None, **over):
        """The status of the call with the named arguments replaced."""
        H, W = self.shape
        f16 = lambda m: (C.c_float * 16)(*np.asarray(m, f32).reshape(-1).tolist())  # noqa: E731
        ptr = lambda t: None if t is None else (t if isinstance(t, int) else t.data_ptr())  # noqa: E731
        a = dict(n=self.n, H=H, W=W, disp=self.disp, confidence=None, Q=self.Q, min_confidence=0.0,
                 z_min=tc.DEPTH_RANGE[0], z_max=tc.DEPTH_RANGE[1], invalid=-1.0, Hm=self.model_shape[0], Wm=self.model_shape[1],
                 depth=self.depth, normals=self.normals, Qm=self.Qm, Pm=self.Pm, c2w=self.c2w, w2c=self.w2c,
                 pose_in=self.pose_in, schedule=self.schedule, max_distance=tc.MAX_DISTANCE, min_inliers=tc.MIN_INLIERS,
                 min_pivot=1e-3, rot_eps=0.0, trans_eps=0.0, pose_out=self.pose_out, info=self.info, rms=self.rms,
                 sums=self.sums, ws=self.ws, ws_bytes=self.ws.numel(),
                 stream=torch.cuda.current_stream().cuda_stream if stream is None else stream)
        a.update(over)
        sched = None if a["schedule"] is None else np.asarray(a["schedule"], np.int32).reshape(-1)
        pairs = over.get("pairs", 0 if sched is None else sched.size // 2)
        sc = None if sched is None else (C.c_int32 * max(sched.size, 1))(*sched.tolist())
        Q, Qm, Pm = (None if a[k] is None else f16(a[k]) for k in ("Q", "Qm", "Pm"))
        return self.native.LIB.smx_track_camera(
            0, a["n"], a["H"], a["W"], ptr(a["disp"]), ptr(a["confidence"]), Q, a["min_confidence"], a["z_min"], a["z_max"],
            a["invalid"], a["Hm"], a["Wm"], ptr(a["depth"]), ptr(a["normals"]), Qm, Pm, ptr(a["c2w"]), ptr(a["w2c"]),
            ptr(a["pose_in"]), pairs, sc, a["max_distance"], a["min_inliers"], a["min_pivot"], a["rot_eps"], a["trans_eps"],
            ptr(a["pose_out"]), ptr(a["info"]), ptr(a["rms"]), ptr(a["sums"]), ptr(a["ws"]), a["ws_bytes"],
            C.c_void_p(a["stream"]))

    def results(self, pose=None, full=True):
        torch.cuda.synchronize()
        pose = (self.pose_out if pose is None else pose).cpu().numpy()
        return [{"pose": pose[i], "info": self.info[i].cpu().numpy(), "rms": self.rms[i].cpu().numpy(),
                 "sums": self.sums[i].cpu().numpy()} if full else {"pose": pose[i]} for i in range(self.n)]


def test_direct_call_aliased_pose_and_optional_outputs_left_out(cd, views):
    d = Direct(cd, views)
    assert d.call() == 0, d.native.last_error()
    for g, w in zip(d.results(), d.want):
        tc.assert_same(g, w, "direct call")
    pose = d.pose_in.clone()
    assert d.call(pose_in=pose, pose_out=pose, info=None, rms=None, sums=None) == 0, d.native.last_error()
    torch.cuda.synchronize()
    for g, w in zip(d.results(pose, full=False), d.want):
        assert np.array_equal(g["pose"].view(np.uint32), w["pose"].view(np.uint32)), "aliased pose"


def test_graph_capture_of_render_then_track(cd, volume, views):
    import cuda_depth._native as native
    d = Direct(cd, views)
    Hm, Wm = tc.MODEL_SHAPE
    nx, ny, nz = cases.DIMS
    mdisp = torch.empty((2, Hm, Wm), device="cuda")
    d.depth, d.normals = torch.full((2, Hm, Wm), math.nan, device="cuda"), torch.zeros((2, 3, Hm, Wm), device="cuda")
    rws = torch.empty(native.LIB.smx_tsdf_raycast_workspace_bytes(nx, ny, nz), dtype=torch.uint8, device="cuda")
    M = rc.sample_count(cases.DEPTH_RANGE[0], cases.DEPTH_RANGE[1], f32(cases.VS))
    assert M > 1
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        rcode = native.LIB.smx_tsdf_raycast(0, nx, ny, nz, (C.c_float * 3)(*cases.ORIGIN), cases.VS, volume.tsdf.data_ptr(),
                                            volume.weight.data_ptr(), None, 1.0, 2, Hm, Wm,
                                            (C.c_float * 16)(*d.Qm.reshape(-1).tolist()), d.c2w.data_ptr(),
                                            float(f32(cases.VS)), cases.DEPTH_RANGE[0], cases.DEPTH_RANGE[1], -1.0,
                                            mdisp.data_ptr(), d.depth.data_ptr(), d.normals.data_ptr(), None, None,
                                            rws.data_ptr(), rws.numel(), C.c_void_p(s.cuda_stream))
        assert rcode == 0, native.last_error()
        assert d.call(stream=s.cuda_stream) == 0, native.last_error()
    torch.cuda.synchronize()
    for replay in range(2):
        for t in (d.pose_out, d.info, d.rms, d.sums, d.depth, d.normals):
            t.zero_()
        torch.cuda.synchronize()
        graph.replay()
        for g, w in zip(d.results(), d.want):
            tc.assert_same(g, w, f"replay {replay}")


def test_argument_checks(cd, views):
    d = Direct(cd, views, schedule=((2, 1),))
    lib, native = d.native.LIB, d.native
    assert d.call() == 0, native.last_error()
    H, W = d.shape
    big = torch.empty(d.ws.numel() + 256, dtype=torch.uint8, device="cuda")
    bad = [
        (dict(disp=None), "disp"), (dict(Q=None), "non-NULL"), (dict(depth=None), "model_depth"),
        (dict(normals=None), "model_normals"), (dict(Qm=None), "Qm"), (dict(Pm=None), "Pm"), (dict(c2w=None), "non-NULL"),
        (dict(w2c=None), "non-NULL"), (dict(pose_in=None), "pose_in"), (dict(pose_out=None), "pose_out"),
        (dict(ws=None), "workspace"), (dict(n=0), "n >= 1"), (dict(H=0), "H"), (dict(W=40000), "W"),
        (dict(H=32768, W=32768, n=2), "2^30"), (dict(H=8192, W=8192, n=1), "tiles"), (dict(Hm=0), "Hm"),
        (dict(Wm=40000), "Wm"), (dict(Q=np.where(np.eye(4) > 0, np.nan, d.Q)), "Q["),
        (dict(Pm=np.full((4, 4), np.inf, f32)), "Pm["), (dict(Qm=np.eye(4, dtype=f32)), "Qm's ray"),
        (dict(z_min=2.0, z_max=1.0), "z_min"), (dict(z_max=math.nan), "z_min"), (dict(min_confidence=math.inf), "min_confidence"),
        (dict(invalid=math.nan), "finite"), (dict(schedule=[[1, 1]] * 9), "schedule_pairs"),
        (dict(schedule=None, pairs=1), "schedule"), (dict(schedule=[[0, 1]]), "stride"),
        (dict(schedule=[[1, -1]]), "iteration"), (dict(schedule=[[1, 33], [1, 32]]), "in total"),
        (dict(max_distance=0.0), "max_distance"), (dict(max_distance=math.nan), "max_distance"),
        (dict(min_inliers=0), "min_inliers"), (dict(min_pivot=-1.0), "min_pivot"), (dict(rot_eps=-1.0), "rot_eps"),
        (dict(trans_eps=math.nan), "trans_eps"), (dict(ws_bytes=d.ws.numel() - 1), "workspace_bytes"),
        (dict(ws=big.data_ptr() + 64), "aligned"),
        (dict(pose_out=d.pose_in.data_ptr() + 16), "overlaps an input"),
        (dict(pose_out=d.c2w), "overlaps an input"), (dict(info=d.disp), "overlaps an input"),
        (dict(rms=d.pose_out), "two outputs"), (dict(sums=d.ws), "two outputs"),
    ]
    for over, text in bad:
        rcode = d.call(**over)
        assert rcode == SMX_ERR_INVALID_ARG, (over.keys(), rcode)
        assert text in native.last_error(), (list(over), native.last_error())
        assert "smx_track_camera" in native.last_error() or "invalid" in over, (list(over), native.last_error())
    assert d.call(stream=native.STREAM_ENGINE.value) == SMX_ERR_INVALID_ARG and "caller stream" in native.last_error()
    assert lib.smx_track_camera_workspace_bytes(0, H, W) == 0 and lib.smx_track_camera_workspace_bytes(1, 8192, 8192) == 0
    assert lib.smx_track_camera_workspace_bytes(2, H, W) == d.ws.numel() > 0
    # the Python layer's own checks
    depth, normals = views["outside"]
    disp, Q = dev(tc.frame("outside", d.shape)[0]), d.Q
    pose, view = pose4(tc.start_pose("outside")), cd.RenderedView(disparity=depth, depth=depth, normals=normals)
    with pytest.raises(RuntimeError, match="normals"):
        cd.track_camera(disp, Q, pose, cd.RenderedView(disparity=depth, depth=depth), pose, model_Q=d.Qm)
    with pytest.raises(TypeError, match="RenderedView"):
        cd.track_camera(disp, Q, pose, depth, pose, model_Q=d.Qm)
    with pytest.raises(RuntimeError, match="schedule"):
        cd.track_camera(disp, Q, pose, view, pose, model_Q=d.Qm, schedule=((1, 65),))
    with pytest.raises(TypeError, match="schedule"):
        cd.track_camera(disp, Q, pose, view, pose, model_Q=d.Qm, schedule=((1.5, 2),))
    with pytest.raises(RuntimeError, match="pose"):
        cd.track_camera(disp, Q, np.stack([pose, pose]), view, pose, model_Q=d.Qm)
    with pytest.raises(RuntimeError, match="min_inliers"):
        cd.track_camera(disp, Q, pose, view, pose, model_Q=d.Qm, min_inliers=0)
    with pytest.raises(RuntimeError, match="model.depth"):
        cd.track_camera(disp[None], Q, pose, view, pose, model_Q=d.Qm)


def test_volume_track_renders_then_tracks(cd, volume):
    shape = tc.FRAME_SHAPES[1]
    d, Q, true_pose, _ = tc.frame("outside", shape)
    start = pose4(tc.start_pose("outside"))
    res = volume.track(dev(d), Q, start, render_depth_range=cases.DEPTH_RANGE, **tc.PARAMS)
    torch.cuda.synchronize()
    view = rc.raycast_ref(cases.fused_state(), cases.DIMS, cases.ORIGIN, cases.VS, Q, rc.view_pose(start), shape,
                          depth_range=cases.DEPTH_RANGE)
    want = tr.track_ref(d, Q, start[:3], tr.model_view(view["depth"][0], view["normals"][0], Q, start), **tc.PARAMS)
    got = {"pose": res.pose.cpu().numpy()[:3], "rms": res.rms.cpu().numpy(), "sums": res.normal_equations.cpu().numpy(),
           "info": [int(res.lost), int(res.iterations), int(res.inliers), int(res.accepted)]}
    tc.assert_same(got, want, "TSDFVolume.track")
    assert want["info"][0] == 0 and tr.pose_error(want["pose"], true_pose)[0] < 0.5 * tr.pose_error(start, true_pose)[0]


def test_pipeline_tracks_its_own_poses(cd):
    from pipeline import DepthEstimationPipeline, DepthEstimationPipelineConfig
    H, W = tc.SEQ_SHAPE
    Q, frames, poses = tc.sequence()
    order = (0, 1, 2, 5, 3, 4)
    want, state = tc.sequence_expected(order)
    assert [lost for _, lost in want] == [False, False, False, True, False, False]
    cfg = DepthEstimationPipelineConfig(image_shape=(H, W), min_disparity=0, max_disparity=15, stereo_matching_backend="cuda")
    vol = cd.TSDFVolume(cases.DIMS, cases.VS, cases.ORIGIN, color=False)
    assert vol._check_render_args(Q, poses[1], (H, W), 1.0, None, None, True, False, -1.0)[-1] == tc.render_range(poses[1])
    pipe = DepthEstimationPipeline(cfg, reprojection_matrix=Q, tsdf_volume=vol, point_cloud_depth_range=tc.SEQ_RANGE,
                                   track_camera=True, initial_pose=poses[0], tracking_args=tc.SEQ_ARGS)
    maps = iter([dev(frames[i]) for i in order])
    pipe._stereo_matching.process = lambda left, right: next(maps)      # the frames' maps are the sequence's, not matched
    image = torch.zeros((3, H, W), dtype=torch.uint8)
    with pytest.raises(ValueError, match="camera_pose"):
        pipe.process(image, image, camera_pose=poses[0])
    for step, (pose, lost) in enumerate(want):
        before = (vol.tsdf.clone(), vol.weight.clone())
        res = pipe.process(image, image)
        torch.cuda.synchronize()
        assert res.tracking_lost is lost, f"frame {step}"
        assert res.camera_pose.shape == (4, 4) and np.array_equal(res.camera_pose, pose), f"frame {step}"
        if lost:
            assert torch.equal(vol.tsdf, before[0]) and torch.equal(vol.weight, before[1])
    assert np.array_equal(vol.tsdf.cpu().numpy().view(np.uint32), state["tsdf"].view(np.uint32))
    assert np.array_equal(vol.weight.cpu().numpy().view(np.uint32), state["weight"].view(np.uint32))
    assert (state["weight"] > 0).any()
    # the same steps by hand
    vol2, last = cd.TSDFVolume(cases.DIMS, cases.VS, cases.ORIGIN, color=False), None
    for i, (pose, lost) in zip(order, want):
        if last is None:
            last = np.array(poses[0], np.float64)
        else:
            found = vol2.track(dev(frames[i]), Q, last, depth_range=tc.SEQ_RANGE, **tc.SEQ_ARGS)
            assert bool(found.lost) is lost
            last = last if lost else found.pose.cpu().numpy().astype(np.float64)
        assert np.array_equal(last, pose)
        if not lost:
            vol2.integrate(dev(frames[i]), Q, last, depth_range=tc.SEQ_RANGE)
    assert torch.equal(vol2.tsdf, vol.tsdf) and torch.equal(vol2.weight, vol.weight)
    pipe.reset_tracking()
    maps = iter([dev(frames[0])])
    res = pipe.process(image, image)
    assert res.tracking_lost is False and np.array_equal(res.camera_pose, np.asarray(poses[0], np.float64))
    # every earlier argument combination behaves as before
    plain = DepthEstimationPipeline(cfg, reprojection_matrix=Q, tsdf_volume=cd.TSDFVolume(cases.DIMS, cases.VS, cases.ORIGIN))
    with pytest.raises(ValueError, match="camera_pose is required"):
        plain.process(image, image)
    with pytest.raises(ValueError, match="track_camera"):
        DepthEstimationPipeline(cfg, reprojection_matrix=Q, track_camera=True)
    with pytest.raises(ValueError, match="track_camera=True"):
        DepthEstimationPipeline(cfg, initial_pose=np.eye(4))
