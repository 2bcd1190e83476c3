"""Developer tool (not a bench.py leg): one library call per odometry frame against the per-call plugin, in one process.

Two workloads, each through three paths:

  loop    the published configuration's loop (tools/batched_loop.py, tests/test_gpu_loop.py: CV initialisation, kd-tree
          frame-to-model, neighborhood sigma 0.2, <= 20 iterations with the live 1e-4 stop, 30 key frames, grid sample
          0.4 m) on 36 synthetic 64x2048 frames handed over as host arrays;
  plugin  the shape of bench.py's plugin leg: 64x2048 host arrays in (131 072 rows, no grid sample), 20 forced iterations
          against a fixed 100 000-point map (thresholds = inf: pose-only updates), pose and cloud out every frame.

  per_call          `MI355XICPFrameToModel` as it stands (`one_call_frame=False`; the loop behind the four device filters);
  one_call_plugin   the same plugin with `one_call_frame=True` (the filters of the loop stay in Python);
  one_call_library  `IcpContext.frame_launch` + `frame_end` alone — for the loop with the grid sample inside the call.

`--ab N`: N timed passes of every path, alternating (per_call, one_call_plugin, one_call_library, per_call, ...) inside
this process, after one untimed pass of each.  Prints one JSON line — frames/s and ms per frame of every pass, whether the
three trajectories are equal bit for bit — and appends it to profiles/frame_loop.jsonl (`--out`).

usage: python tools/frame_loop.py [--workload loop|plugin|both] [--ab 3] [--frames 36] [--steps 60]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "pylidar-slam_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from pylidar_slam_amd import odometry as our  # noqa: E402
from pylidar_slam_amd.engine import IcpContext  # noqa: E402
from pylidar_slam_amd.synthetic import SceneConfig, make_c2_workload, make_sequence  # noqa: E402

H, W = 64, 2048
PATHS = ("per_call", "one_call_plugin", "one_call_library")
INF = float("inf")


# ---- the published configuration's loop ---------------------------------------------------------------------------------
def loop_config(one_call):
    return our.MI355XICPConfig(max_num_alignments=20, threshold_delta_pose=1.0e-4, data_key="input_data",
                               local_map=dict(type="kdtree_local_map", local_map_size=30, num_neighbors_normals=10),
                               alignment=dict(mode="point_to_plane_gauss_newton",
                                              gauss_newton_config=dict(max_iters=1, scheme="neighborhood", sigma=0.2)),
                               one_call_frame=one_call)


def loop_filters(dev):
    """config/slam/preprocessing/grid_sample_mi355x.yaml with 0.4 m voxels and the padded grid sample; the de-skew writes
    to `deskewed` so that the plugin copies the registered rows out as `odometry_pc` (pose AND cloud out, on every path)."""
    return [our.ToDevice(our.ToDeviceConfig(device=str(dev)), device=dev),
            our.Distortion(our.DistortionConfig(pointcloud_key="pc_device", timestamps_key="timestamps_device",
                                                output_key="deskewed")),
            our.GridSample(our.GridSampleConfig(voxel_size=0.4, pointcloud_key="deskewed", padded=True)),
            our.ToTensor(our.ToTensorConfig(device=str(dev), keys={"sample_points": "input_data"}, dtype="float32"),
                         device=dev)]


def run_loop(path, scans, dev):
    if path == "one_call_library":
        ctx = IcpContext(height=H, width=W, max_num_alignments=20, threshold_delta_pose=1.0e-4, scheme="neighborhood",
                         sigma=0.2, local_map_size=30, num_neighbors_normals=10, device=dev.index or 0)
        ctx.use_torch_stream()
        ctx.odometry_init(voxel_size=0.4, threshold_trans=0.1, threshold_rot=0.3, constant_velocity=True, targets=1)
        rel, rows = [], 0
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for s in scans:
            ctx.frame_launch(s)
            r = ctx.frame_end()
            rel.append(r.pose)
            rows = 0 if r.points is None else r.points.shape[0]
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        ctx.close()
        return dt, np.stack(rel), rows
    odo = our.MI355XICPFrameToModel(loop_config(path == "one_call_plugin"), projector=our.SphericalProjector(H, W), device=dev)
    flt = loop_filters(dev)
    init = our.ConstantVelocityInitialization()
    odo.init()
    init.init()
    rows = 0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for f, s in enumerate(scans):
        d = {"numpy_pc": s}
        init.next_frame(d)
        for x in flt:
            x.filter(d)
        odo.process_next_frame(d)
        if f > 0:
            init.save_real_motion(d["odometry_pose"], d)
            rows = d["odometry_pc"].shape[0]
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    rel = odo.get_relative_poses()
    odo.ctx.close()
    return dt, rel, rows


# ---- the plugin leg's shape ---------------------------------------------------------------------------------------------
def run_plugin(path, workload, steps, dev):
    scans, _, model, order, start = workload
    if path == "one_call_library":
        ctx = IcpContext(height=H, width=W, max_num_alignments=20, threshold_delta_pose=0.0, scheme="geman_mcclure", sigma=0.3,
                         local_map_size=20, num_neighbors_normals=10, device=dev.index or 0)
        ctx.use_torch_stream()
        # (the caller holds the rows it hands over: no copy back, as the plugin makes `odometry_pc` from its host array)
        ctx.odometry_init(voxel_size=0.0, threshold_trans=INF, threshold_rot=INF, constant_velocity=True, targets=0,
                          copy_cloud=False)
        ctx.frame_launch(scans[start])
        ctx.frame_end()
        ctx.map_set(model)
        rel = []

        def frame(f):
            ctx.frame_launch(scans[f])
            r = ctx.frame_end()
            rel.append(r.pose)
            return scans[f].copy()  # (the cloud out: a fresh host array per frame, like the plugin's)
        close = ctx.close
    else:
        cfg = our.MI355XICPConfig(max_num_alignments=20, threshold_delta_pose=0.0, data_key="numpy_pc", threshold_trans=INF,
                                  threshold_rot=INF,
                                  local_map=dict(type="kdtree_local_map", local_map_size=20, num_neighbors_normals=10),
                                  alignment=dict(mode="point_to_plane_gauss_newton",
                                                 gauss_newton_config=dict(max_iters=1, scheme="geman_mcclure", sigma=0.3)),
                                  one_call_frame=path == "one_call_plugin")
        odo = our.MI355XICPFrameToModel(cfg, projector=our.SphericalProjector(H, W), device=dev)
        init = our.ConstantVelocityInitialization()
        odo.init()
        init.init()
        odo.process_next_frame({"numpy_pc": scans[start]})
        odo.local_map.set_map_pointcloud(model)
        rel = []

        def frame(f):
            d = {"numpy_pc": scans[f]}
            init.next_frame(d)
            odo.process_next_frame(d)
            init.save_real_motion(d["odometry_pose"], d)
            rel.append(d["odometry_pose"])
            return d["odometry_pc"]
        close = odo.ctx.close
    for k in range(5):  # (warm-up frames of this pass: allocations, the first grid build)
        frame(order[k % len(order)])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rows = 0
    for k in range(5, 5 + steps):
        rows = frame(order[k % len(order)]).shape[0]
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    close()
    return dt, np.stack(rel), rows


def ab(run, frames, passes):
    for path in PATHS:  # (untimed: kernels loaded, pinned buffers and streams made)
        run(path)
    fps = {p: [] for p in PATHS}
    rels, rows = {}, {}
    for _ in range(passes):
        for path in PATHS:
            dt, rels[path], rows[path] = run(path)
            fps[path].append(frames / dt)
    out = {}
    for path in PATHS:
        out[path + "_frames_per_s"] = [round(v, 1) for v in fps[path]]
        out[path + "_ms_per_frame"] = [round(1e3 / v, 4) for v in fps[path]]
        out[path + "_median_frames_per_s"] = round(float(np.median(fps[path])), 1)
        out[path + "_cloud_rows_out"] = int(rows[path])
    out["trajectories_equal"] = bool(all(np.array_equal(rels[PATHS[0]], rels[p]) for p in PATHS[1:]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", choices=["loop", "plugin", "both"], default="both")
    ap.add_argument("--ab", type=int, default=3, help="timed passes of every path, alternating inside this process")
    ap.add_argument("--frames", type=int, default=36, help="frames of the published configuration's loop")
    ap.add_argument("--steps", type=int, default=60, help="timed frames of the plugin leg's shape")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frame_loop.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    result = {"tool": "frame_loop", "ab": args.ab, "device": torch.cuda.get_device_name(0)}
    if args.workload in ("loop", "both"):
        scans = make_sequence(SceneConfig(height=H, width=W), args.frames)[0]
        result["loop"] = dict(frames=args.frames, **ab(lambda p: run_loop(p, scans, dev), args.frames, args.ab))
    if args.workload in ("plugin", "both"):
        workload = make_c2_workload(0, "pingpong", args.steps)
        result["plugin"] = dict(steps=args.steps, **ab(lambda p: run_plugin(p, workload, args.steps, dev), args.steps, args.ab))
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
