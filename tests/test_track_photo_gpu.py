"""Camera tracking with the photometric term on the device (include/stereo_mi355x.h: smx_track_camera_photometric,
smx_intensity_planes), bit for bit against the NumPy twin (tests/track_photo_ref.py) on the cases of
tests/track_photo_cases.py: the triples of tests/track_cases.py with intensity planes at strides 1, 2 and 3, every sum of
one iteration, the default schedule, a weight of 0 against the geometric entry, batches with the middle triple lost, the
textured plane that the geometric entry loses, the edges of the tap rule, frames whose sums need the combine kernel's
chunk trees, the intensity planes, the entry's behaviour (repeatability, an aliased pose, optional outputs, graph capture,
the argument checks), and the Python layer and the pipeline."""
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


class Direct:
    """One direct call of smx_track_camera_photometric (or, with geometric=True, smx_track_camera on the same operands),
    every operand its own tensor.  models: one dict per triple sharing Qm and Pm."""

    def __init__(self, disp, Q, starts, models, intensity, weight, max_difference, schedule, conf=None, **params):
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
        self.fint = dev(np.asarray(intensity, f32))
        self.mint = dev(np.stack([np.asarray(m["intensity"], f32) for m in models]))
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
        self.weight, self.max_difference = weight, max_difference
        self.params = dict(min_confidence=0.0, rot_eps=0.0, trans_eps=0.0)
        self.params.update(params)

    @classmethod
    def of_triples(cls, triples, schedule=tr.DEFAULT_SCHEDULE, weight=pc.WEIGHT, **extra):
        kw = dict(tc.PARAMS)
        kw.update(extra)
        frames = [tc.frame(v, s, k, c) for v, s, k, c, _ in triples]
        conf = triples[0][3]
        if conf:
            kw.setdefault("min_confidence", 0.1)
        return cls(np.stack([fr[0] for fr in frames]), frames[0][1], np.stack([tc.start_pose(t[0]) for t in triples]),
                   [pc.model(v, m) for v, _, _, _, m in triples],
                   np.stack([pc.frame_intensity(s, k) for _, s, k, _, _ in triples]), weight, pc.MAX_DIFFERENCE, schedule,
                   conf=np.stack([fr[3] for fr in frames]) if conf else None, **kw)

    def call(self, stream=None, geometric=False, **over):
        """The status of the call with the named arguments replaced."""
        f16 = lambda m: (C.c_float * 16)(*np.asarray(m, f32).reshape(-1).tolist())  # noqa: E731
        ptr = lambda t: None if t is None else (t if isinstance(t, int) else t.data_ptr())  # noqa: E731
        p = self.params
        a = dict(n=self.n, H=self.H, W=self.W, disp=self.disp, confidence=self.conf, Q=self.Q,
                 min_confidence=p["min_confidence"], z_min=p["depth_range"][0], z_max=p["depth_range"][1], invalid=-1.0,
                 Hm=self.Hm, Wm=self.Wm, depth=self.depth, normals=self.normals, Qm=self.Qm, Pm=self.Pm, c2w=self.c2w,
                 w2c=self.w2c, pose_in=self.pose_in, schedule=self.schedule, max_distance=p["max_distance"],
                 min_inliers=p["min_inliers"], min_pivot=p["min_pivot"], rot_eps=p["rot_eps"], trans_eps=p["trans_eps"],
                 fint=self.fint, mint=self.mint, weight=self.weight, max_difference=self.max_difference,
                 pose_out=self.pose_out, info=self.info, rms=self.rms, sums=self.sums, pinfo=self.pinfo, prms=self.prms,
                 ws=self.ws, ws_bytes=self.ws.numel(),
                 stream=torch.cuda.current_stream().cuda_stream if stream is None else stream)
        a.update(over)
        sched = None if a["schedule"] is None else np.asarray(a["schedule"], np.int32).reshape(-1)
        pairs = over.get("pairs", 0 if sched is None else sched.size // 2)
        sc = None if sched is None else (C.c_int32 * max(sched.size, 1))(*sched.tolist())
        Q, Qm, Pm = (None if a[k] is None else f16(a[k]) for k in ("Q", "Qm", "Pm"))
        head = (0, a["n"], a["H"], a["W"], ptr(a["disp"]), ptr(a["confidence"]), Q, a["min_confidence"], a["z_min"],
                a["z_max"], a["invalid"], a["Hm"], a["Wm"], ptr(a["depth"]), ptr(a["normals"]), Qm, Pm, ptr(a["c2w"]),
                ptr(a["w2c"]), ptr(a["pose_in"]), pairs, sc, a["max_distance"], a["min_inliers"], a["min_pivot"],
                a["rot_eps"], a["trans_eps"])
        if geometric:
            return self.native.LIB.smx_track_camera(*head, ptr(a["pose_out"]), ptr(a["info"]), ptr(a["rms"]),
                                                    ptr(a["sums"]), ptr(a["ws"]), a["ws_bytes"], C.c_void_p(a["stream"]))
        return self.native.LIB.smx_track_camera_photometric(
            *head, ptr(a["fint"]), ptr(a["mint"]), a["weight"], a["max_difference"], ptr(a["pose_out"]), ptr(a["info"]),
            ptr(a["rms"]), ptr(a["sums"]), ptr(a["pinfo"]), ptr(a["prms"]), ptr(a["ws"]), a["ws_bytes"],
            C.c_void_p(a["stream"]))

    def run(self, **over):
        assert self.call(**over) == 0, self.native.last_error()
        return self.results()

    def results(self, pose=None):
        torch.cuda.synchronize()
        pose = (self.pose_out if pose is None else pose).cpu().numpy()
        return [{"pose": pose[i], "info": self.info[i].cpu().numpy(), "rms": self.rms[i].cpu().numpy(),
                 "sums": self.sums[i].cpu().numpy(), "pinfo": self.pinfo[i].cpu().numpy(), "prms": self.prms[i].cpu().numpy()}
                for i in range(self.n)]


# ---- 1. bits --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", tc.FRAME_SHAPES)
@pytest.mark.parametrize("stride", [1, 2, 3])
def test_two_iterations_at_each_stride(cd, shape, stride):
    schedule = ((stride, 2),)
    got = Direct.of_triples([("outside", shape, 0, False, False)], schedule).run()
    pc.assert_same(got[0], pc.expected("outside", shape, schedule=schedule), f"{shape} stride {stride}")


@pytest.mark.parametrize("shape", tc.FRAME_SHAPES)
def test_every_sum_of_one_iteration_at_stride_1(cd, shape):
    want = pc.expected("left", shape, 1, schedule=((1, 1),))
    assert np.count_nonzero(want["sums"]) == 33 and 4 * want["pinfo"][0] >= want["info"][2] > 0
    got = Direct.of_triples([("left", shape, 1, False, False)], ((1, 1),)).run()
    pc.assert_same(got[0], want, f"one iteration {shape}")


@pytest.mark.parametrize("shape", tc.FRAME_SHAPES)
def test_the_default_schedule(cd, shape):
    want = pc.expected("outside", shape)
    assert want["info"][1] == 19 and 4 * want["pinfo"][0] >= want["info"][2] > 0
    got = Direct.of_triples([("outside", shape, 0, False, False)]).run()
    pc.assert_same(got[0], want, f"default schedule {shape}")


# ---- 2. a weight of 0 is the geometric entry ----------------------------------------------------------------------------------

@pytest.mark.parametrize("confidence", [False, True])
def test_a_weight_of_zero_is_the_geometric_entry(cd, confidence):
    shape = tc.FRAME_SHAPES[0]
    triples = [("outside", shape, 0, confidence, False), ("left", shape, 1, confidence, True),
               ("left", shape, 2, confidence, False)]
    d = Direct.of_triples(triples, weight=0.0)
    got = d.run()
    for g, (v, s, k, c, m) in zip(got, triples):
        pc.assert_same(g, pc.expected(v, s, k, c, m, weight=0.0), f"{v} {k} weight 0")
        tc.assert_same(dict(g, sums=g["sums"][:30]), tc.expected(v, s, k, c, m), f"{v} {k} against the geometric twin")
    assert got[0]["pinfo"][0] > 0 and got[2]["pinfo"][0] > 0
    # and against the geometric entry itself, on the same operands
    sums30 = torch.empty((3, 30), dtype=torch.float64, device="cuda")
    ws = torch.empty(d.native.LIB.smx_track_camera_workspace_bytes(3, *shape), dtype=torch.uint8, device="cuda")
    pose = torch.empty_like(d.pose_out)
    info, rms = torch.empty_like(d.info), torch.empty_like(d.rms)
    assert d.call(geometric=True, pose_out=pose, info=info, rms=rms, sums=sums30, ws=ws, ws_bytes=ws.numel()) == 0
    torch.cuda.synchronize()
    assert torch.equal(pose.view(torch.int32), d.pose_out.view(torch.int32)) and torch.equal(info, d.info)
    assert torch.equal(rms.view(torch.int32), d.rms.view(torch.int32))
    assert torch.equal(sums30.view(torch.int64), d.sums[:, :30].contiguous().view(torch.int64))


# ---- 3. batches -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("confidence", [False, True])
def test_three_triples_with_the_middle_one_lost(cd, confidence):
    shape = tc.FRAME_SHAPES[0]
    triples = [("outside", shape, 0, confidence, False), ("left", shape, 1, confidence, True),
               ("left", shape, 2, confidence, False)]
    want = [pc.expected(v, s, k, c, m) for v, s, k, c, m in triples]
    assert [int(w["info"][0]) for w in want] == [0, 1, 0]
    got = Direct.of_triples(triples).run()
    for g, w, t in zip(got, want, triples):
        pc.assert_same(g, w, str(t))
    assert np.array_equal(bits32(got[1]["pose"]), bits32(tc.start_pose("left")))
    for i in (0, 2):                                                   # n = 1: the same bits
        alone = Direct.of_triples(triples[i:i + 1]).run()
        pc.assert_same(alone[0], want[i], f"n = 1, triple {i}")


# ---- 4. the plane ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", pc.PLANE_SHAPES)
def test_the_geometric_entry_loses_the_plane_and_the_photometric_one_tracks_it(cd, shape):
    disp, Q, inten = pc.plane_frame(shape)
    geo, want = pc.plane_expected(shape)
    d = Direct(disp[None], Q, pc.plane_start()[None], [pc.plane_model()], inten[None], pc.WEIGHT, 40.0, tr.DEFAULT_SCHEDULE,
               **pc.PLANE_PARAMS)
    sums30 = torch.empty((1, 30), dtype=torch.float64, device="cuda")
    ws = torch.empty(d.native.LIB.smx_track_camera_workspace_bytes(1, *shape), dtype=torch.uint8, device="cuda")
    assert d.call(geometric=True, sums=sums30, ws=ws, ws_bytes=ws.numel()) == 0, d.native.last_error()
    lost = d.results()[0]
    tc.assert_same(dict(lost, sums=sums30[0].cpu().numpy()), geo, f"plane {shape}, geometric")
    assert lost["info"][0] == 1 and np.array_equal(bits32(lost["pose"]), bits32(pc.plane_start()))
    got = d.run()[0]
    pc.assert_same(got, want, f"plane {shape}")
    m0, d0 = tr.pose_error(pc.plane_start(), pc.plane_true_pose())
    m1, d1 = tr.pose_error(got["pose"], pc.plane_true_pose())
    print(f"plane {shape}: {m0:.4f} m {d0:.3f} deg -> {m1:.5f} m {d1:.4f} deg")
    assert got["info"][0] == 0 and m1 <= 0.1 * m0 and d1 <= 0.1 * d0


# ---- 5. the edges of the tap rule -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", pc.EDGE_NAMES)
def test_the_edges_of_the_tap_rule(cd, name):
    disp, Q, start, m, inten, weight, max_difference, count = pc.edge_case(name)
    got = Direct(disp[None], Q, start[None], [m], inten[None], weight, max_difference, ((1, 1),), **pc.EDGE_PARAMS).run()[0]
    pc.assert_same(got, pc.edge_expected(name), name)
    assert got["info"][2] == 1 and got["pinfo"].tolist() == [count, 1 - count]


# ---- 6. the deep tree -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", pc.TREE_SHAPES)
def test_one_iteration_past_one_partial_per_chunk(cd, shape):
    want = pc.tree_expected(shape)
    assert pc.tree_len(shape) == dict(pc.TREE_CASES)[shape] and want["pinfo"][0] > 1000
    disp, Q = tc.scaled_frame(shape)
    d = Direct(disp[None], Q, tc.start_pose(tc.TREE_VIEW)[None], [pc.tree_model()], pc.tree_intensity(shape)[None], pc.WEIGHT,
               200.0, ((1, 1),), conf=tc.wide_confidence(shape)[None], **tc.PARAMS)
    pc.assert_same(d.run()[0], want, f"tree {shape}")


# ---- 7. intensity planes ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(1, 1), (5, 67), (33, 45)])
@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("n", [1, 3])
def test_intensity_planes(cd, n, channels, shape):
    rng = np.random.default_rng(n + 10 * channels + shape[1])
    img = rng.integers(0, 256, (n, channels) + shape).astype(np.uint8)
    img.reshape(-1)[0], img.reshape(-1)[-1] = 0, 255
    got = cd.intensity_planes(dev(img))
    assert got.shape == (n,) + shape and got.dtype == torch.float32
    assert np.array_equal(bits32(got.cpu().numpy()), bits32(tp.intensity_planes_ref(img, channels)))


def test_intensity_planes_refusals(cd):
    import cuda_depth._native as native
    lib = native.LIB
    img = torch.zeros((2, 3, 4, 5), dtype=torch.uint8, device="cuda")
    out = torch.zeros((2, 4, 5), device="cuda")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.smx_intensity_planes(0, 2, 3, 4, 5, img.data_ptr(), out.data_ptr(), s) == 0, native.last_error()
    both = torch.zeros(2 * 3 * 4 * 5 + 64, dtype=torch.uint8, device="cuda")
    for args, text in (((2, 3, 4, 5, None, out.data_ptr(), s), "non-NULL"), ((2, 3, 4, 5, img.data_ptr(), None, s), "non-NULL"),
                       ((0, 3, 4, 5, img.data_ptr(), out.data_ptr(), s), "n >= 1"),
                       ((2, 3, 0, 5, img.data_ptr(), out.data_ptr(), s), "H"),
                       ((2, 3, 4, 40000, img.data_ptr(), out.data_ptr(), s), "W"),
                       ((2, 3, 32768, 32768, img.data_ptr(), out.data_ptr(), s), "2^30"),
                       ((2, 2, 4, 5, img.data_ptr(), out.data_ptr(), s), "channels"),
                       ((2, 3, 4, 5, both.data_ptr(), both.data_ptr() + 64, s), "overlap"),
                       ((2, 3, 4, 5, img.data_ptr(), out.data_ptr(), native.STREAM_ENGINE.value), "caller stream")):
        assert lib.smx_intensity_planes(0, *args) == SMX_ERR_INVALID_ARG, args[:4]
        assert text in native.last_error() and "smx_intensity_planes" in native.last_error(), native.last_error()
    with pytest.raises(RuntimeError, match="uint8"):
        cd.intensity_planes(out)
    with pytest.raises(RuntimeError, match="uint8"):
        cd.intensity_planes(img[:, :2].contiguous())


# ---- 8. the entry's behaviour -------------------------------------------------------------------------------------------------------

TWO = [("outside", tc.FRAME_SHAPES[0], 0, False, False), ("left", tc.FRAME_SHAPES[0], 1, False, False)]


def test_the_same_call_twice_an_aliased_pose_and_optional_outputs_left_out(cd):
    d = Direct.of_triples(TWO)
    want = [pc.expected(v, s, k) for v, s, k, *_ in TWO]
    first = d.run()
    for t in (d.pose_out, d.info, d.rms, d.sums, d.pinfo, d.prms):
        t.zero_()
    for a, b, w in zip(first, d.run(), want):
        pc.assert_same(a, w, "first call")
        pc.assert_same(b, a, "second call")
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


@pytest.fixture(scope="module")
def volume(cd):
    state = cases.fused_state()
    vol = cd.TSDFVolume(cases.DIMS, cases.VS, cases.ORIGIN)
    vol.tsdf.copy_(dev(state["tsdf"]))
    vol.weight.copy_(dev(state["weight"]))
    vol.color.copy_(dev(state["color"]))
    return vol


def test_graph_capture_of_render_with_colours_then_intensity_planes_then_track(cd, volume):
    import cuda_depth._native as native
    lib = native.LIB
    shape = tc.FRAME_SHAPES[0]
    models = [pc.rendered_model(v) for v, *_ in TWO]
    images = np.stack([pc.frame_image(shape, k) for _, _, k, *_ in TWO])
    want = [pc.rendered_expected(v, shape, k) for v, _, k, *_ in TWO]
    assert all(w["info"][0] == 0 and w["pinfo"][0] > 100 for w in want)
    frames = [tc.frame(v, s, k, c) for v, s, k, c, _ in TWO]
    d = Direct(np.stack([fr[0] for fr in frames]), frames[0][1], np.stack([tc.start_pose(v) for v, *_ in TWO]), models,
               np.zeros((2,) + shape, f32), pc.WEIGHT, 255.0, tr.DEFAULT_SCHEDULE, **tc.PARAMS)
    Hm, Wm = tc.MODEL_SHAPE
    nx, ny, nz = cases.DIMS
    mdisp = torch.empty((2, Hm, Wm), device="cuda")
    colors = torch.zeros((2, 3, Hm, Wm), dtype=torch.uint8, device="cuda")
    image = dev(images)
    d.depth, d.normals = torch.full((2, Hm, Wm), math.nan, device="cuda"), torch.zeros((2, 3, Hm, Wm), device="cuda")
    rws = torch.empty(lib.smx_tsdf_raycast_workspace_bytes(nx, ny, nz), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        sp = C.c_void_p(s.cuda_stream)
        rcode = lib.smx_tsdf_raycast(0, nx, ny, nz, (C.c_float * 3)(*cases.ORIGIN), cases.VS, volume.tsdf.data_ptr(),
                                     volume.weight.data_ptr(), volume.color.data_ptr(), 1.0, 2, Hm, Wm,
                                     (C.c_float * 16)(*d.Qm.reshape(-1).tolist()), d.c2w.data_ptr(), float(f32(cases.VS)),
                                     cases.DEPTH_RANGE[0], cases.DEPTH_RANGE[1], -1.0, mdisp.data_ptr(), d.depth.data_ptr(),
                                     d.normals.data_ptr(), colors.data_ptr(), None, rws.data_ptr(), rws.numel(), sp)
        assert rcode == 0, native.last_error()
        assert lib.smx_intensity_planes(0, 2, 3, Hm, Wm, colors.data_ptr(), d.mint.data_ptr(), sp) == 0, native.last_error()
        assert lib.smx_intensity_planes(0, 2, 3, shape[0], shape[1], image.data_ptr(), d.fint.data_ptr(), sp) == 0
        assert d.call(stream=s.cuda_stream) == 0, native.last_error()
    torch.cuda.synchronize()
    for replay in range(2):
        for t in (d.pose_out, d.info, d.rms, d.sums, d.pinfo, d.prms, d.depth, d.normals, d.mint, d.fint, colors):
            t.zero_()
        torch.cuda.synchronize()
        graph.replay()
        for g, w in zip(d.results(), want):
            pc.assert_same(g, w, f"replay {replay}")
        assert np.array_equal(colors.cpu().numpy(), np.stack([m["colors"] for m in models]))


def test_argument_checks(cd):
    d = Direct.of_triples(TWO, schedule=((2, 1),))
    lib, native = d.native.LIB, d.native
    assert d.call() == 0, native.last_error()
    H, W = d.H, d.W
    big = torch.empty(d.ws.numel() + 256, dtype=torch.uint8, device="cuda")
    bad = [
        (dict(fint=None), "frame_intensity"), (dict(mint=None), "model_intensity"),
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
        (dict(trans_eps=math.nan), "trans_eps"),
        (dict(weight=-0.5), "photometric_weight"), (dict(weight=math.inf), "photometric_weight"),
        (dict(weight=math.nan), "photometric_weight"), (dict(max_difference=0.0), "max_intensity_difference"),
        (dict(max_difference=-1.0), "max_intensity_difference"), (dict(max_difference=math.nan), "max_intensity_difference"),
        (dict(ws_bytes=d.ws.numel() - 1), "workspace_bytes"),
        (dict(ws_bytes=lib.smx_track_camera_workspace_bytes(2, H, W)), "smx_track_camera_photometric_workspace_bytes"),
        (dict(ws=big.data_ptr() + 64), "aligned"),
        (dict(pose_out=d.pose_in.data_ptr() + 16), "overlaps an input"),
        (dict(pose_out=d.c2w), "overlaps an input"), (dict(info=d.disp), "overlaps an input"),
        (dict(pinfo=d.fint), "overlaps an input"), (dict(prms=d.mint), "overlaps an input"),
        (dict(pinfo=d.disp), "overlaps an input"), (dict(sums=d.fint), "overlaps an input"),
        (dict(rms=d.pose_out), "two outputs"), (dict(sums=d.ws), "two outputs"),
        (dict(pinfo=d.pose_out), "two outputs"), (dict(prms=d.pinfo), "two outputs"), (dict(prms=d.ws), "two outputs"),
        (dict(pinfo=d.sums.data_ptr() + 2 * 30 * 8), "two outputs"),  # past [n][30], inside the [n][33] sums
    ]
    for over, text in bad:
        rcode = d.call(**over)
        assert rcode == SMX_ERR_INVALID_ARG, (over.keys(), rcode)
        assert text in native.last_error(), (list(over), native.last_error())
        assert "smx_track_camera_photometric" in native.last_error() or "invalid" in over, (list(over), native.last_error())
    assert d.call(weight=0.0) == 0 and d.call(weight=3e38) == 0, native.last_error()
    assert d.call(stream=native.STREAM_ENGINE.value) == SMX_ERR_INVALID_ARG and "caller stream" in native.last_error()
    q = lib.smx_track_camera_photometric_workspace_bytes
    assert q(0, H, W) == 0 and q(1, 8192, 8192) == 0 and q(2, H, W) == d.ws.numel() > lib.smx_track_camera_workspace_bytes(2, H, W)
    torch.cuda.synchronize()


# ---- 9. the Python layer and the pipeline ---------------------------------------------------------------------------------------

def as_dict(res, i=None):
    """A TrackingResult (its triple i when batched) in the twin's form."""
    torch.cuda.synchronize()
    pick = (lambda t: t) if i is None else (lambda t: t[i])
    n = {k: pick(getattr(res, k)).cpu().numpy() for k in ("pose", "lost", "iterations", "inliers", "accepted", "rms",
                                                          "normal_equations", "photometric_inliers", "photometric_rms")}
    return {"pose": n["pose"][:3], "info": np.array([int(n["lost"]), n["iterations"], n["inliers"], n["accepted"]]),
            "rms": n["rms"], "sums": n["normal_equations"], "prms": n["photometric_rms"],
            "pinfo": np.array([n["photometric_inliers"], n["inliers"] - n["photometric_inliers"]])}


def test_track_camera_with_an_image(cd):
    shape, view = tc.FRAME_SHAPES[0], "outside"
    d, Q, _, _ = tc.frame(view, shape)
    m = pc.model(view)
    start, mpose = pose4(tc.start_pose(view)), tc.model_pose(view)
    rv = cd.RenderedView(disparity=dev(m["depth"]), depth=dev(m["depth"]), normals=dev(m["normals"]))
    kw = dict(model_Q=m["Qm"], model_intensity=dev(m["intensity"]), photometric_weight=pc.WEIGHT,
              max_intensity_difference=pc.MAX_DIFFERENCE, **tc.PARAMS)
    rgb = pc.frame_image(shape, 0)
    gray = rgb[1]
    for name, image, plane in (("float32", pc.frame_intensity(shape, 0), pc.frame_intensity(shape, 0)),
                               ("uint8 rgb", rgb, tp.intensity_planes_ref(rgb[None], 3)[0]),
                               ("uint8 gray", gray, gray.astype(f32))):
        res = cd.track_camera(dev(d), Q, start, rv, mpose, image=dev(image), **kw)
        want = tp.track_photo_ref(d, Q, start[:3], m, plane, pc.WEIGHT, max_difference=pc.MAX_DIFFERENCE, **tc.PARAMS)
        assert want["info"][0] == 0 and want["pinfo"][0] > 100, name
        assert res.pose.shape == (4, 4) and res.normal_equations.shape == (33,) and res.information.shape == (6, 6)
        pc.assert_same(as_dict(res), want, name)
        assert np.array_equal(res.information.cpu().numpy(), tr.information(want["sums"]))
    # batched, with uint8 model colours in place of model_intensity
    mc = pc.rendered_model(view)
    rvc = cd.RenderedView(disparity=dev(mc["depth"])[None], depth=dev(mc["depth"])[None], normals=dev(mc["normals"])[None],
                          colors=dev(mc["colors"])[None])
    res = cd.track_camera(dev(d)[None], Q, start[None], rvc, mpose[None], image=dev(rgb)[None], model_Q=mc["Qm"],
                          photometric_weight=pc.WEIGHT, max_intensity_difference=255.0, **tc.PARAMS)
    assert res.pose.shape == (1, 4, 4) and res.photometric_inliers.shape == (1,)
    pc.assert_same(as_dict(res, 0), pc.rendered_expected(view, shape, 0), "batched, model colours")
    # without an image, or with a weight of 0, the geometric entry runs
    old = cd.track_camera(dev(d), Q, start, rv, mpose, model_Q=m["Qm"], **tc.PARAMS)
    zero = cd.track_camera(dev(d), Q, start, rv, mpose, model_Q=m["Qm"], image=dev(rgb), photometric_weight=0.0, **tc.PARAMS)
    torch.cuda.synchronize()
    for r in (old, zero):
        assert r.photometric_inliers is None and r.photometric_rms is None and r.normal_equations.shape == (30,)
        assert np.array_equal(bits32(r.pose.cpu().numpy()[:3]), bits32(tc.expected(view, shape)["pose"]))
    with pytest.raises(RuntimeError, match="needs the frame's image"):
        cd.track_camera(dev(d), Q, start, rv, mpose, model_Q=m["Qm"], photometric_weight=0.01)
    with pytest.raises(RuntimeError, match="model.colors"):
        cd.track_camera(dev(d), Q, start, rv, mpose, model_Q=m["Qm"], image=dev(rgb), photometric_weight=0.01)
    with pytest.raises(RuntimeError, match="image must be"):
        cd.track_camera(dev(d), Q, start, rv, mpose, model_Q=m["Qm"], image=dev(rgb[:, :-1]), photometric_weight=0.01,
                        model_intensity=dev(m["intensity"]))
    with pytest.raises(RuntimeError, match="model_intensity must be"):
        cd.track_camera(dev(d), Q, start, rv, mpose, model_Q=m["Qm"], image=dev(rgb), photometric_weight=0.01,
                        model_intensity=dev(m["intensity"][:-1]))


def test_volume_track_with_an_image(cd, volume):
    shape = tc.FRAME_SHAPES[1]
    d, Q, _, _ = tc.frame("outside", shape)
    start = pose4(tc.start_pose("outside"))
    rgb = pc.frame_image(shape, 0)
    res = volume.track(dev(d), Q, start, render_depth_range=cases.DEPTH_RANGE, image=dev(rgb), photometric_weight=pc.WEIGHT,
                       max_intensity_difference=255.0, **tc.PARAMS)
    view = rc.raycast_ref(cases.fused_state(), cases.DIMS, cases.ORIGIN, cases.VS, Q, rc.view_pose(start), shape,
                          depth_range=cases.DEPTH_RANGE)
    m = tr.model_view(view["depth"][0], view["normals"][0], Q, start)
    m["intensity"] = tp.intensity_planes_ref(view["colors"], 3)[0]
    want = tp.track_photo_ref(d, Q, start[:3], m, tp.intensity_planes_ref(rgb[None], 3)[0], pc.WEIGHT, max_difference=255.0,
                              **tc.PARAMS)
    assert want["info"][0] == 0 and want["pinfo"][0] > 100
    pc.assert_same(as_dict(res), want, "TSDFVolume.track(image=)")
    plain = cd.TSDFVolume(cases.DIMS, cases.VS, cases.ORIGIN, color=False)
    with pytest.raises(RuntimeError, match="colour volume"):
        plain.track(dev(d), Q, start, image=dev(rgb), photometric_weight=pc.WEIGHT, **tc.PARAMS)


def test_pipeline_passes_the_left_frame_to_the_tracker(cd):
    from pipeline import DepthEstimationPipeline, DepthEstimationPipelineConfig
    H, W = tc.SEQ_SHAPE
    Q, frames, poses = tc.sequence()
    order = (0, 1, 2, 5, 3)
    images = [torch.from_numpy(np.array(pc.frame_image((H, W), i))) for i in order]
    targs = dict(tc.SEQ_ARGS, photometric_weight=pc.WEIGHT, max_intensity_difference=255.0)
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
    # the same steps by hand
    vol2, last, seen = cd.TSDFVolume(cases.DIMS, cases.VS, cases.ORIGIN), None, []
    for i, image, (pose, lost) in zip(order, images, got):
        if last is None:
            last, found_lost = np.array(poses[0], np.float64), False
        else:
            found = vol2.track(dev(frames[i]), Q, last, depth_range=tc.SEQ_RANGE, image=image.cuda(), **targs)
            found_lost = bool(found.lost)
            assert found.photometric_inliers is not None
            seen.append(int(found.photometric_inliers))
            last = last if found_lost else found.pose.cpu().numpy().astype(np.float64)
        assert found_lost is lost and np.array_equal(last, pose), f"frame {i}"
        if not found_lost:
            vol2.integrate(dev(frames[i]), Q, last, image=image.cuda(), depth_range=tc.SEQ_RANGE)
    assert [lost for _, lost in got] == [False, False, False, True, False] and max(seen) > 100
    assert torch.equal(vol2.tsdf, vol.tsdf) and torch.equal(vol2.weight, vol.weight) and torch.equal(vol2.color, vol.color)
    # the term took part: the geometric tracker ends elsewhere
    geo, _ = tc.sequence_expected()
    assert not np.array_equal(got[2][0], geo[2][0])
    with pytest.raises(RuntimeError, match="colour volume"):
        plain = DepthEstimationPipeline(cfg, reprojection_matrix=Q, point_cloud_depth_range=tc.SEQ_RANGE, track_camera=True,
                                        tsdf_volume=cd.TSDFVolume(cases.DIMS, cases.VS, cases.ORIGIN, color=False),
                                        initial_pose=poses[0], tracking_args=targs)
        maps = iter([dev(frames[0]), dev(frames[1])])
        plain._stereo_matching.process = lambda left, right: next(maps)
        plain.process(images[0], images[0])
        plain.process(images[1], images[1])
