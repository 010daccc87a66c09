"""Records how the engine-free entries of the C ABI (stereo-depth_amd/csrc/smx_maps.hip) refuse their arguments.

    python tools/record_map_entry_refusals.py [--lib PATH] [--out tests/golden/map_entry_refusals.json]

Run it on a machine WITHOUT a GPU against a library built from the commit whose behaviour is to be pinned.  Every check of
these entries runs before a device is selected, so there a refused call returns SMX_ERR_INVALID_ARG with its message and a
call that passes every check returns SMX_ERR_HIP ("cannot select HIP device 0") without touching a pointer: the pointers
below are invented integers.  tests/test_map_entry_refusals_cpu.py replays the file against the tree's library.

Per entry: one valid base call, one case per rule with that rule alone broken (a rule may have several variants), and one
case per adjacent pair of rules in the entry's order with both broken, which pins the order of the rules.  Per size query:
at least 8 calls, with the first rejected size on each side.

A record is {"entry", "args", "status", "message"} (queries: "value" in place of the last two).  In "args" a pointer is an
integer, a host table is {"t": "f32" | "u16", "n": length, "fill": value, "at": [[index, value], ...]}, NULL is null and a
non-finite float is the string "nan", "inf" or "-inf"; the C types come from cuda_depth._native.EXPORTS."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG, ERR_HIP = -1, -3
ENGINE_STREAM = 2 ** 64 - 1                       # SMX_STREAM_ENGINE
NAN, INF = "nan", "inf"
U8, F32 = 0, 1                                    # SMX_DTYPE_*


def A(k: int, off: int = 0) -> int:
    """The k-th invented operand: 4 GiB apart (no base call's operands touch), 256-byte aligned."""
    return 0x7000_0000_0000 + k * 0x1_0000_0000 + off


def table(t: str, n: int, fill, at=()):
    return {"t": t, "n": n, "fill": fill, "at": [list(p) for p in at]}


def is_operand(v) -> bool:
    return isinstance(v, int) and v >= A(0)


def slot(v: int) -> int:
    return (v - A(0)) >> 32


def plain(variant: dict) -> dict:
    return {k: x for k, x in variant.items() if not k.startswith("_")}


def norm(message: str) -> str:
    """A message without its numbers: two calls broke the same rule."""
    return re.sub(r"0x[0-9a-f]+|-?\d+(\.\d+)?(e[+-]?\d+)?|\bnan\b|\binf\b", "#", message)


def to_c(v, keep: list):
    """One recorded argument as ctypes accepts it (the same decoding as the replay test's)."""
    if isinstance(v, dict):
        arr = ({"f32": C.c_float, "u16": C.c_uint16}[v["t"]] * v["n"])(*([v["fill"]] * v["n"]))
        for k, x in v["at"]:
            arr[k] = float(x) if v["t"] == "f32" else x
        keep.append(arr)
        return arr
    return float(v) if isinstance(v, str) else v


IDENT = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1]


def mat(at=()):
    return {"t": "f32", "n": 16, "fill": 0, "at": [[i, v] for i, v in enumerate(IDENT) if v] + [list(p) for p in at]}


def entries(q):
    """name -> (argument names, base values, rules in the entry's order).  A rule is a list of variants; a variant is a
    dict of the arguments that break it; the first variants of two adjacent rules are merged into the pair case, and where
    both break through the same argument, or one break would undo the other, the later rule's variant carries the pair
    case as "_pair" and, as "_repaired", that case with the first rule mended: the recorder requires that the pair case gets
    the first rule's answer and that the mended one still gets the second's ("_no_pair": why no call breaks both).  q(name, *args) is the
    library's size query."""
    E = {}
    n, H, W = 2, 5, 37
    px4 = n * H * W * 4

    E["smx_lr_check"] = (
        "device_id n H W left right out max_diff invalid stream".split(),
        dict(device_id=0, n=n, H=H, W=W, left=A(1), right=A(2), out=A(3), max_diff=1.0, invalid=-1.0, stream=0),
        [[dict(max_diff=-1.0), dict(max_diff=NAN), dict(max_diff=INF)], [dict(invalid=NAN), dict(invalid=INF)],
         [dict(left=None), dict(right=None), dict(out=None)],
         [dict(n=0), dict(H=0), dict(W=0), dict(H=32769), dict(W=32769), dict(n=-1)],
         [dict(stream=ENGINE_STREAM)], [dict(out=A(2, 4)), dict(out=A(1, 4)), dict(out=A(2, px4 - 4))]])

    need = q("smx_postprocess_workspace_bytes", n, H, W)
    post_tail = [[dict(**{"in": None}), dict(out=None), dict(workspace=None)], [dict(n=0), dict(H=32769), dict(W=0), dict(W=32769), dict(H=0)],
                 [dict(workspace_bytes=need - 1), dict(workspace_bytes=0)],
                 [dict(out=A(1, 4))], [dict(workspace=A(1)), dict(workspace=A(2))], [dict(workspace=A(4, 4), _pair=dict(workspace=A(1, 4)))],
                 [dict(stream=ENGINE_STREAM)]]
    E["smx_filter_speckles"] = (
        "device_id n H W in out max_speckle_size max_diff invalid workspace workspace_bytes stream".split(),
        dict(device_id=0, n=n, H=H, W=W, **{"in": A(1)}, out=A(2), max_speckle_size=10, max_diff=1.0, invalid=-1.0,
             workspace=A(4), workspace_bytes=need, stream=0),
        [[dict(max_speckle_size=-1)], [dict(max_diff=NAN), dict(max_diff=-0.5)], [dict(invalid=INF)]] + post_tail)
    E["smx_fill_invalid"] = (
        "device_id n H W in out invalid workspace workspace_bytes stream".split(),
        dict(device_id=0, n=n, H=H, W=W, **{"in": A(1)}, out=A(2), invalid=-1.0, workspace=A(4), workspace_bytes=need,
             stream=0),
        [[dict(invalid=NAN)]] + post_tail)

    E["smx_weighted_median"] = (
        "device_id n H W in holes guide out radius range_weight spatial_weight invalid workspace workspace_bytes stream".split(),
        dict(device_id=0, n=n, H=H, W=W, **{"in": A(1)}, holes=A(2), guide=A(3), out=A(4), radius=2,
             range_weight=table("u16", 256, 7), spatial_weight=table("u16", 256, 9), invalid=-1.0, workspace=A(5),
             workspace_bytes=64, stream=0),
        [[dict(**{"in": None}), dict(guide=None), dict(out=None)], [dict(range_weight=None), dict(spatial_weight=None)],
         [dict(n=0), dict(W=32769), dict(H=0), dict(n=-3)], [dict(radius=0), dict(radius=16)],
         [dict(range_weight=table("u16", 256, 7, [(255, 1024)])), dict(range_weight=table("u16", 256, 7, [(3, 65535), (9, 2000)]))],
         [dict(spatial_weight=table("u16", 256, 9, [(8, 1024)]))], [dict(invalid=NAN)],
         # workspace_bytes below smx_median_workspace_bytes: the query is 0, so no size_t breaks this rule
         [dict(workspace=None, workspace_bytes=16)],
         [dict(out=A(1, 4)), dict(out=A(3, 8))], [dict(out=A(2, 4), _pair=dict(out=A(1, 4), holes=A(1, 8)),
                                                       _repaired={"in": A(9), "out": A(1, 4), "holes": A(1, 8)})],
         [dict(workspace=A(1)), dict(workspace=A(2, 256)), dict(workspace=A(3)), dict(workspace=A(4))],
         [dict(workspace=A(5, 4), _pair=dict(workspace=A(1, 4), workspace_bytes=64))], [dict(stream=ENGINE_STREAM)]])

    need = q("smx_wls_workspace_bytes", n, H, W)
    E["smx_wls_filter"] = (
        "device_id n H W in confidence guide out num_iterations lambdas range_weight min_weight invalid workspace workspace_bytes stream".split(),
        dict(device_id=0, n=n, H=H, W=W, **{"in": A(1)}, confidence=A(2), guide=A(3), out=A(4), num_iterations=2,
             lambdas=table("f32", 8, 100.0), range_weight=table("f32", 256, 0.5), min_weight=0.001, invalid=-1.0,
             workspace=A(5), workspace_bytes=need, stream=0),
        [[dict(**{"in": None}), dict(guide=None), dict(out=None)], [dict(lambdas=None), dict(range_weight=None)],
         [dict(n=0), dict(H=32769), dict(W=0), dict(W=32769)], [dict(num_iterations=0), dict(num_iterations=9)],
         [dict(lambdas=table("f32", 8, 100.0, [(1, -1.0)])), dict(lambdas=table("f32", 8, 100.0, [(0, NAN)])),
          dict(lambdas=table("f32", 8, 100.0, [(1, 1048577.0)]))],
         [dict(range_weight=table("f32", 256, 0.5, [(5, 2.0)])), dict(range_weight=table("f32", 256, 0.5, [(255, NAN)]))],
         [dict(min_weight=-1.0), dict(min_weight=INF)], [dict(invalid=NAN)],
         [dict(workspace_bytes=need - 1), dict(workspace=None)],
         [dict(out=A(2, 4)), dict(out=A(1, 4)), dict(out=A(3, 4))],
         [dict(workspace=A(3)), dict(workspace=A(1)), dict(workspace=A(2)), dict(workspace=A(4))],
         [dict(workspace=A(5, 8), _pair=dict(workspace=A(3, 8)))], [dict(stream=ENGINE_STREAM)]])

    E["smx_confidence_map"] = (
        "device_id n H W left_disp right_disp guide radius lr_scale texture_scale invalid out stream".split(),
        dict(device_id=0, n=n, H=H, W=W, left_disp=A(1), right_disp=A(2), guide=A(3), radius=2, lr_scale=1.0,
             texture_scale=4.0, invalid=-1.0, out=A(4), stream=0),
        [[dict(left_disp=None), dict(out=None)], [dict(n=0), dict(H=32769), dict(W=0), dict(H=0)], [dict(radius=0), dict(radius=16)],
         [dict(lr_scale=0.0), dict(lr_scale=NAN)], [dict(texture_scale=NAN), dict(texture_scale=-2.0)], [dict(invalid=INF)],
         [dict(out=A(3, 4)), dict(out=A(1, 4)), dict(out=A(2, 4))], [dict(stream=ENGINE_STREAM)]])

    E["smx_temporal_filter"] = (
        "device_id n H W disp confidence guide prev_guide state_disp state_weight guide_out out motion_radius motion_threshold decay max_diff max_weight min_weight invalid stream".split(),
        dict(device_id=0, n=n, H=H, W=W, disp=A(1), confidence=A(2), guide=A(3), prev_guide=A(4), state_disp=A(5),
             state_weight=A(6), guide_out=A(7), out=A(8), motion_radius=1, motion_threshold=8.0, decay=0.9, max_diff=2.0,
             max_weight=16.0, min_weight=0.05, invalid=-1.0, stream=0),
        [[dict(disp=None), dict(prev_guide=None), dict(state_weight=None), dict(out=None)], [dict(W=0), dict(n=0), dict(H=32769)],
         [dict(motion_radius=8), dict(motion_radius=-1)], [dict(motion_threshold=-1.0), dict(motion_threshold=NAN)],
         [dict(decay=0.0), dict(decay=1.5), dict(decay=NAN)], [dict(max_diff=-1.0)], [dict(max_weight=0.0), dict(max_weight=INF)],
         [dict(min_weight=-0.5)], [dict(invalid=NAN)], [dict(out=A(1, 4))],
         [dict(out=A(3, 4), _pair=dict(out=A(1, 4), confidence=A(1, 8)),
               _repaired=dict(disp=A(9), out=A(1, 4), confidence=A(1, 8))), dict(out=A(2, 4)), dict(out=A(5, 4)), dict(out=A(7, 4))],
         [dict(state_disp=A(3, 4)), dict(state_weight=A(1, 4)), dict(state_weight=A(4))],
         [dict(state_weight=A(5, 4), _pair=dict(state_disp=A(3, 4), state_weight=A(3, 8)),
               _repaired=dict(guide=A(9), state_disp=A(3, 4), state_weight=A(3, 8)))], [dict(guide_out=A(1, 4)), dict(guide_out=A(6, 4))], [dict(stream=ENGINE_STREAM)]])

    E["smx_remap_pairs"] = (
        "device_id n channels dtype H_in W_in H_out W_out left_in right_in left_map right_map left_out right_out border_mode border_value stream".split(),
        dict(device_id=0, n=2, channels=3, dtype=U8, H_in=6, W_in=9, H_out=5, W_out=7, left_in=A(1), right_in=A(2),
             left_map=A(3), right_map=A(4), left_out=A(5), right_out=A(6), border_mode=0, border_value=0.0, stream=0),
        [[dict(left_in=None), dict(left_map=None), dict(left_out=None)], [dict(right_map=None), dict(right_in=None, right_out=None)],
         [dict(n=0)], [dict(H_in=0), dict(W_out=32769), dict(W_in=32769), dict(H_out=0)], [dict(channels=5), dict(channels=0)], [dict(dtype=2)],
         [dict(border_mode=2)], [dict(border_value=INF)], [dict(border_value=0.5, _pair=dict(border_value=INF), _repaired="inf is neither finite nor an integer in 0..255"),
          dict(border_value=256.0)],
         [dict(n=2 ** 31 - 1, channels=4, dtype=F32, H_in=32768, W_in=32768,
               _no_pair="the uint8 border rule needs dtype U8, whose frames never reach 2^34 bytes")],
         [dict(left_out=A(1, 4)), dict(right_out=A(3, 8)), dict(left_out=A(4, 8)), dict(right_out=A(2))],
         [dict(right_out=A(5, 16), _pair=dict(left_out=A(1, 4), right_out=A(1, 8)),
               _repaired=dict(left_in=A(9), left_out=A(1, 4), right_out=A(1, 8)))], [dict(stream=ENGINE_STREAM)]])

    sn, sH, sW, sD = 2, 12, 40, 40
    need = q("smx_sgm_workspace_bytes", sn, sH, sW, sD, 8)
    sgm_names = ("device_id n channels dtype H W left right min_disparity num_disparities paths P1 P2 uniqueness "
                 "lr_max_diff subpixel invalid out gray_left_out").split()
    sgm_base = dict(device_id=0, n=sn, channels=1, dtype=U8, H=sH, W=sW, left=A(1), right=A(2), min_disparity=0,
                    num_disparities=sD, paths=8, P1=8, P2=32, uniqueness=10, lr_max_diff=1.0, subpixel=1, invalid=-1.0,
                    out=A(3), gray_left_out=A(4), right_out=A(5), workspace=A(6), workspace_bytes=need, stream=0)

    def sgm_rules(right):
        return ([[dict(left=None), dict(right=None), dict(out=None), dict(workspace=None)], [dict(H=32769), dict(n=0), dict(W=32769), dict(H=0)],
                 [dict(n=65537, W=32768), dict(n=65537, H=32768, W=32768)], [dict(channels=2), dict(channels=4), dict(channels=0)], [dict(dtype=3), dict(dtype=-1)],
                 [dict(min_disparity=-1), dict(min_disparity=32769)], [dict(num_disparities=0), dict(num_disparities=257)],
                 [dict(paths=5)], [dict(P1=40), dict(P1=-1), dict(P2=192)], [dict(uniqueness=100), dict(uniqueness=-1)],
                 [dict(lr_max_diff=NAN)], [dict(invalid=INF)], [dict(workspace_bytes=need - 1)],
                 [dict(out=A(1, 4)), dict(gray_left_out=A(2, 4)), dict(out=A(6, 256))] + ([dict(right_out=A(6, 512))] if right else []),
                 [dict(gray_left_out=A(3, 4), _pair=dict(out=A(1, 4), gray_left_out=A(1, 8)),
                       _repaired=dict(left=A(9), out=A(1, 4), gray_left_out=A(1, 8)))]] +
                ([[dict(right_out=A(3, 4)), dict(right_out=A(4, 4))]] if right else []) +
                [[dict(workspace=A(1)), dict(workspace=A(2))], [dict(workspace=A(6, 4), _pair=dict(workspace=A(1, 4)))], [dict(stream=ENGINE_STREAM)]])

    E["smx_sgm"] = (sgm_names + "workspace workspace_bytes stream".split(),
                    {k: v for k, v in sgm_base.items() if k != "right_out"}, sgm_rules(False))
    E["smx_sgm_with_right_map"] = (sgm_names + "right_out workspace workspace_bytes stream".split(), sgm_base,
                                   [[dict(right_out=None)]] + sgm_rules(True))

    E["smx_disparity_to_points"] = (
        "device_id disp H W bf invalid depth points count_dev workspace stream".split(),
        dict(device_id=0, disp=A(1), H=5, W=37, bf=100.0, invalid=-1.0, depth=A(2), points=A(3), count_dev=A(4),
             workspace=A(5), stream=0),
        [[dict(disp=None), dict(points=None), dict(count_dev=None), dict(workspace=None), dict(H=0), dict(W=0), dict(H=32769)]])
    E["smx_eval_metrics"] = (
        "device_id n est gt mask pixels max_disparity thresholds out_sums stream".split(),
        dict(device_id=0, n=2, est=A(1), gt=A(2), mask=A(3), pixels=185, max_disparity=64.0,
             thresholds=table("f32", 4, 1.0), out_sums=A(4), stream=0),
        [[dict(est=None), dict(gt=None), dict(out_sums=None), dict(thresholds=None), dict(n=0), dict(pixels=0)]])

    rn, rH, rW = 3, 5, 37
    need = q("smx_reproject_workspace_bytes", rn, rH, rW)
    reproj = [[dict(z_min=2.0, z_max=1.0), dict(z_min=NAN), dict(z_max=NAN)], [dict(min_confidence=NAN), dict(min_confidence=INF)],
              [dict(invalid_disparity=NAN)], [dict(image_channels=2), dict(image_channels=4)], [dict(image_dtype=2), dict(image_dtype=-1)]]
    E["smx_reproject_points"] = (
        "device_id n H W disp Q confidence min_confidence z_min z_max invalid_disparity image image_channels image_dtype points colors indices xyz_map offsets workspace workspace_bytes stream".split(),
        dict(device_id=0, n=rn, H=rH, W=rW, disp=A(1), Q=mat(), confidence=A(2), min_confidence=0.5, z_min=0.1, z_max=50.0,
             invalid_disparity=-1.0, image=A(3), image_channels=3, image_dtype=U8, points=A(4), colors=A(5), indices=A(6),
             xyz_map=A(7), offsets=A(8), workspace=A(9), workspace_bytes=need, stream=0),
        [[dict(disp=None), dict(Q=None), dict(points=None), dict(offsets=None), dict(workspace=None)], [dict(W=32769), dict(n=0), dict(H=32769)],
         [dict(n=32768, H=32768), dict(n=2, H=32768, W=32768)], [dict(Q=mat([(5, NAN)])), dict(Q=mat([(15, INF), (7, NAN)]))]] + reproj +
        [[dict(image=None, _no_pair="the image rules need an image, the colour rule needs none")], [dict(workspace_bytes=need - 1), dict(workspace_bytes=0)],
         [dict(points=A(1, 4)), dict(colors=A(3, 1)), dict(offsets=A(9, 8)), dict(xyz_map=A(2, 4))],
         [dict(indices=A(7, 4)), dict(indices=A(4, 4)), dict(offsets=A(7, 4)), dict(colors=A(6)),
          dict(colors=A(4, 6000), image=A(4, 7000))], [dict(workspace=A(9, 4))],
         [dict(stream=ENGINE_STREAM)]])

    vn, vcap = 2, 5000
    need = q("smx_voxel_workspace_bytes", vn, vcap)
    E["smx_voxel_downsample"] = (
        "device_id n capacity points colors offsets voxel_size min_points out_points out_colors out_counts out_offsets dropped workspace workspace_bytes stream".split(),
        dict(device_id=0, n=vn, capacity=vcap, points=A(1), colors=A(2), offsets=A(3), voxel_size=0.05, min_points=1,
             out_points=A(4), out_colors=A(5), out_counts=A(6), out_offsets=A(7), dropped=A(8), workspace=A(9),
             workspace_bytes=need, stream=0),
        [[dict(points=None), dict(offsets=None), dict(out_counts=None), dict(dropped=None), dict(workspace=None)],
         [dict(colors=None), dict(out_colors=None)],
         [dict(n=0), dict(n=65537), dict(capacity=0), dict(capacity=2 ** 30 + 1)],
         [dict(voxel_size=0.0), dict(voxel_size=NAN)], [dict(min_points=0), dict(min_points=-1)], [dict(workspace_bytes=need - 1)],
         [dict(out_points=A(1, 4)), dict(out_offsets=A(3, 4)), dict(dropped=A(9, 512)), dict(out_colors=A(2, 3))],
         [dict(dropped=A(7, 4)), dict(out_counts=A(4, 4)), dict(out_colors=A(4, 59000), colors=A(4, 70000))], [dict(workspace=A(9, 128))], [dict(stream=ENGINE_STREAM)]])

    tn, tH, tW = 2, 12, 20
    need = q("smx_tsdf_integrate_workspace_bytes", tn, tH, tW)
    origin = table("f32", 3, -1.0)
    volume = [[dict(nx=0), dict(ny=4097), dict(nx=1025, ny=1024, nz=1024)], [dict(voxel_size=0.0), dict(voxel_size=INF)],
              [dict(origin=table("f32", 3, -1.0, [(1, INF)])), dict(origin=table("f32", 3, -1.0, [(2, NAN), (0, NAN)]))]]
    E["smx_tsdf_integrate"] = (
        "device_id nx ny nz origin voxel_size truncation max_weight tsdf weight color n H W disp Q P world_to_camera confidence min_confidence z_min z_max invalid_disparity image image_channels image_dtype workspace workspace_bytes stream".split(),
        dict(device_id=0, nx=16, ny=12, nz=10, origin=origin, voxel_size=0.1, truncation=0.3, max_weight=64.0, tsdf=A(1),
             weight=A(2), color=A(3), n=tn, H=tH, W=tW, disp=A(4), Q=mat(), P=mat(), world_to_camera=A(5), confidence=A(6),
             min_confidence=0.5, z_min=0.1, z_max=50.0, invalid_disparity=-1.0, image=A(7), image_channels=3,
             image_dtype=U8, workspace=A(8), workspace_bytes=need, stream=0),
        [[dict(origin=None), dict(tsdf=None), dict(weight=None), dict(disp=None), dict(Q=None), dict(P=None),
          dict(world_to_camera=None), dict(workspace=None)]] + volume +
        [[dict(W=32769), dict(n=0)], [dict(n=32768, H=32768), dict(n=2, H=32768, W=32768)],
         [dict(truncation=0.1), dict(truncation=NAN), dict(truncation=0.05)], [dict(max_weight=0.0), dict(max_weight=NAN)],
         # Q[k] and P[k] are checked in one loop over k: the lower index wins, Q before P at the same index
         [dict(Q=mat([(5, NAN)])), dict(P=mat([(3, INF)])), dict(Q=mat([(5, NAN)]), P=mat([(3, NAN)])),
          dict(Q=mat([(3, NAN)]), P=mat([(3, NAN)])), dict(Q=mat([(2, INF)]), P=mat([(9, NAN)]))]] + reproj +
        [[dict(image=None, _no_pair="the image rules need an image, the colour rule needs none")], [dict(workspace_bytes=need - 1)],
         [dict(tsdf=A(4, 4)), dict(workspace=A(5)), dict(color=A(7)), dict(weight=A(6, 4))],
         [dict(color=A(2, 4)), dict(weight=A(1, 4)), dict(workspace=A(3)), dict(weight=A(1, 7000), disp=A(1, 10000))], [dict(workspace=A(8, 4))],
         [dict(stream=ENGINE_STREAM)]])

    need = q("smx_tsdf_extract_workspace_bytes", 16, 12, 10)
    E["smx_tsdf_extract_points"] = (
        "device_id nx ny nz origin voxel_size tsdf weight color min_weight capacity points normals colors count workspace workspace_bytes stream".split(),
        dict(device_id=0, nx=16, ny=12, nz=10, origin=origin, voxel_size=0.1, tsdf=A(1), weight=A(2), color=A(3),
             min_weight=0.5, capacity=1000, points=A(4), normals=A(5), colors=A(6), count=A(7), workspace=A(8),
             workspace_bytes=need, stream=0),
        [[dict(origin=None), dict(tsdf=None), dict(points=None), dict(count=None), dict(workspace=None)]] + volume +
        [[dict(min_weight=0.0), dict(min_weight=NAN)], [dict(capacity=0), dict(capacity=2 ** 30 + 1)], [dict(color=None)],
         [dict(workspace_bytes=need - 1)], [dict(points=A(1, 4)), dict(workspace=A(2)), dict(count=A(3, 4))],
         [dict(colors=A(5)), dict(count=A(8, 4)), dict(normals=A(4, 4)), dict(normals=A(4, 11000), tsdf=A(4, 20000))], [dict(workspace=A(8, 4))],
         [dict(stream=ENGINE_STREAM)]])

    need = q("smx_tsdf_extract_triangles_workspace_bytes", 70, 6, 5)
    E["smx_tsdf_extract_triangles"] = (
        "device_id nx ny nz tsdf weight min_weight capacity triangles count workspace workspace_bytes stream".split(),
        dict(device_id=0, nx=70, ny=6, nz=5, tsdf=A(1), weight=A(2), min_weight=0.5, capacity=1000, triangles=A(3),
             count=A(4), workspace=A(5), workspace_bytes=need, stream=0),
        [[dict(tsdf=None), dict(weight=None), dict(triangles=None), dict(count=None), dict(workspace=None)],
         [dict(nz=0), dict(nx=4097), dict(nx=1024, ny=1024, nz=1025)], [dict(min_weight=-1.0), dict(min_weight=INF)],
         [dict(capacity=0), dict(capacity=2 ** 30 + 1)], [dict(workspace_bytes=need - 1)],
         [dict(triangles=A(1, 4)), dict(workspace=A(2)), dict(count=A(2, 4))], [dict(workspace=A(4)), dict(count=A(3, 4)), dict(count=A(3, 11998), weight=A(3, 12000)),
          dict(workspace=A(2), count=A(3, 4))],
         [dict(workspace=A(5, 4), _pair=dict(count=A(5, 8), workspace=A(5, 4)), _repaired=dict(workspace=A(5, 4)))],
         [dict(stream=ENGINE_STREAM)]])
    return E


DIMS3 = [(1, 1, 1), (2, 5, 37), (3, 255, 257), (1, 1080, 1920), (0, 5, 37), (2, 0, 37), (2, 5, 0), (2, 32768, 32768),
         (2, 32769, 37), (2, 5, 32769), (-1, 5, 37)]
POINTS3 = DIMS3 + [(1, 32768, 32768), (1, 32768, 32767), (4, 16384, 16384), (4, 16384, 16385), (3, 32768, 16384)]
VOLS = [(1, 1, 1), (16, 12, 10), (70, 6, 5), (63, 64, 65), (4096, 4096, 64), (4096, 4096, 65), (1024, 1024, 1024),
        (1025, 1024, 1024), (0, 12, 10), (16, 0, 10), (16, 12, 0), (4097, 1, 1), (1, 4097, 1), (1, 1, 4097)]
QUERIES = {
    "smx_postprocess_workspace_bytes": DIMS3,
    "smx_median_workspace_bytes": DIMS3,
    "smx_wls_workspace_bytes": DIMS3,
    "smx_sgm_workspace_bytes": [(2, 12, 40, D, 8) for D in (0, 1, 40, 64, 65, 128, 129, 130, 256, 257)] +
                               [(2, 12, 40, 40, p) for p in (3, 4, 5, 7, 8, 9)] +
                               [(n, H, W, 40, 4) for n, H, W in DIMS3] +
                               [(32768, 32768, 32768, 1, 8), (32769, 32768, 32768, 1, 8), (65536, 16384, 16384, 64, 4),
                                (65537, 16384, 16384, 64, 4)],
    "smx_reproject_workspace_bytes": POINTS3,
    "smx_voxel_workspace_bytes": [(1, 1), (2, 5000), (1, 4095), (1, 4096), (1, 4097), (65536, 2 ** 30), (0, 5000),
                                  (65537, 5000), (2, 0), (2, 2 ** 30 + 1), (-1, 1), (2, -1)],
    "smx_tsdf_integrate_workspace_bytes": POINTS3,
    "smx_tsdf_extract_workspace_bytes": VOLS,
    "smx_tsdf_extract_triangles_workspace_bytes": VOLS,
}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None, help="library to record from (default: the tree's)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "map_entry_refusals.json"))
    opt = ap.parse_args()
    if opt.lib:
        os.environ["SMX_LIB_PATH"] = os.path.abspath(opt.lib)
    sys.path.insert(0, os.path.join(ROOT, "stereo-depth_amd"))
    from cuda_depth import _native
    lib = _native.LIB

    records, skipped = [], []
    for name, argsets in QUERIES.items():
        assert len(argsets) >= 8, name
        values = [int(getattr(lib, name)(*a)) for a in argsets]
        assert name == "smx_median_workspace_bytes" or (any(values) and not all(values)), (name, values)
        records += [{"entry": name, "args": list(a), "value": v} for a, v in zip(argsets, values)]

    def call(name, names, values):
        keep = []
        rc = getattr(lib, name)(*[to_c(values[k], keep) for k in names])
        return rc, _native.last_error()

    for name, (names, base, rules) in entries(lambda fn, *a: int(getattr(lib, fn)(*a))).items():
        assert sorted(names) == sorted(base) and len(names) == len(_native.EXPORTS[name][1]), name
        rc, msg = call(name, names, base)
        assert rc == ERR_HIP and msg == "cannot select HIP device 0", (name, rc, msg)
        records.append({"entry": name, "args": [base[k] for k in names], "status": rc, "message": msg})
        cases = [(f"rule {i}.{j}", plain(v)) for i, rule in enumerate(rules) for j, v in enumerate(rule)]
        pairs = []                                       # (what, both broken, first alone, second alone, first repaired)
        for i in range(len(rules) - 1):
            a, b = rules[i][0], rules[i + 1][0]
            what = f"rules {i}+{i + 1}"
            if "_no_pair" in b:
                skipped.append(f"{name}: rules {i} and {i + 1}: {b['_no_pair']}")
            elif "_pair" in b:
                pairs.append((what, b["_pair"], plain(a), plain(b), b.get("_repaired", plain(b))))
            else:
                assert not set(plain(a)) & set(plain(b)), f"{name} {what} break through the same argument: give a _pair"
                for first, second in ((plain(a), plain(b)), (plain(b), plain(a))):
                    for k in first:                      # neither break may lean on an address the other vacates
                        assert not any(is_operand(base[k]) and is_operand(v) and slot(v) == slot(base[k])
                                       for v in second.values()), f"{name} {what}: {k} moves away from under the other rule"
                pairs.append((what, {**plain(a), **plain(b)}, plain(a), plain(b), None))
        for what, change in cases + [(p[0], p[1]) for p in pairs]:
            assert set(change) <= set(names), (name, what)
            rc, msg = call(name, names, {**base, **change})
            assert rc == INVALID_ARG and msg, f"{name} {what}: status {rc}, '{msg}' -- every non-base case must be refused"
            records.append({"entry": name, "args": [{**base, **change}[k] for k in names], "status": rc, "message": msg})
        for what, both, first, second, repaired in pairs:
            text = {k: norm(call(name, names, {**base, **v})[1]) for k, v in (("both", both), ("first", first), ("second", second))}
            assert text["both"] == text["first"] != text["second"], f"{name} {what}: the first rule does not answer: {text}"
            if isinstance(repaired, dict):               # with the first rule mended the second must still be broken
                got = norm(call(name, names, {**base, **repaired})[1])
                assert got == text["second"], f"{name} {what}: the second rule is not broken in the pair case: '{got}'"
    with open(opt.out, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r, separators=(",", ":"), allow_nan=False) for r in records) + "\n]\n")
    n_entries = len({r["entry"] for r in records if "status" in r})
    print(f"{len(records)} records ({n_entries} entries, {len(QUERIES)} queries), {os.path.getsize(opt.out)} bytes -> {opt.out}")
    for s in skipped:
        print("no pair case:", s)
    assert n_entries == 17 and os.path.getsize(opt.out) < 221 * 1024
    return 0


if __name__ == "__main__":
    sys.exit(main())
