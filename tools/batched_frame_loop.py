"""Developer tool (not a bench.py leg): the frame loop of B drives behind two library calls against the per-call batched
plugin, in one process.

Workload: the published configuration's loop (tools/batched_loop.py, tests/test_gpu_loop.py: CV initialisation, kd-tree
frame-to-model, neighborhood sigma 0.2, <= 20 iterations with the live 1e-4 stop, 30 key frames, grid sample 0.4 m) on B
synthetic drives of 36 frames of 64x2048 each (different seeds and speeds), at B = 8 and B = 16, with the frames handed over
as host arrays (`host`) and as device tensors (`device`).  Pose and cloud out on every path.  Three paths:

  per_call          `MI355XPreprocessingBatch` + `MI355XICPFrameToModelBatch` as they stand (`one_call_frame=False`);
  one_call_plugin   the same two with `one_call_frame=True`: the step is icp_batch_frame_launch + icp_batch_frame_end, the
                    batched preprocessing stays in front;
  one_call_library  `IcpBatch.frame_launch` + `frame_end` alone, the grid sample inside the call.

NOT measured here: `one_call_plugin` keeps `MI355XPreprocessingBatch` in front on both inputs (its ToDevice uploads the host
arrays), so the flag is always timed on cuda tensors; the numpy route of the flagged plugin (the library's own single pinned
upload, no grid sample in front) has no leg of its own — of the three paths only `one_call_library` uses that upload.

`--ab N`: N timed passes of every path, alternating (per_call, one_call_plugin, one_call_library, per_call, ...) inside this
process, after one untimed pass of each.  ASSERTS that the three paths give every member the same trajectory, bit for bit.
Prints one JSON line per (B, input) — frames/s and ms per step of every pass, their range and median — and appends it to
profiles/batched_frame_loop.jsonl (`--out`).

usage: python tools/batched_frame_loop.py [--ab 3] [--batch 8 16] [--inputs host device] [--frames 36]"""
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
from pylidar_slam_amd.engine import IcpBatch, IcpContext  # noqa: E402
from pylidar_slam_amd.synthetic import SceneConfig, make_sequence  # noqa: E402

H, W = 64, 2048
PATHS = ("per_call", "one_call_plugin", "one_call_library")


def published_config(one_call):
    return our.MI355XICPConfig(max_num_alignments=20, threshold_delta_pose=1.0e-4, data_key="input_data",
                               local_map=dict(type="kdtree_local_map", local_map_size=30, num_neighbors_normals=10),
                               alignment=dict(mode="point_to_plane_gauss_newton",
                                              gauss_newton_config=dict(max_iters=1, scheme="neighborhood", sigma=0.2)),
                               one_call_frame=one_call)


def chain(dev):
    """config/slam/preprocessing/grid_sample_mi355x.yaml with 0.4 m voxels and the padded grid sample; the de-skew writes to
    `deskewed` so that the plugin copies the registered rows out as `odometry_pc` (pose AND cloud out, on every path)."""
    return {"0": {"filter_name": "to_device_mi355x", "device": str(dev),
                  "keys": {"numpy_pc": "pc_device", "numpy_pc_timestamps": "timestamps_device"}},
            "1": {"filter_name": "distortion_mi355x", "force": False, "activate": True, "pointcloud_key": "pc_device",
                  "timestamps_key": "timestamps_device", "output_key": "deskewed"},
            "2": {"filter_name": "grid_sample_mi355x", "voxel_size": 0.4, "pointcloud_key": "deskewed", "padded": True},
            "3": {"filter_name": "to_tensor_mi355x", "device": str(dev), "dtype": "float32",
                  "keys": {"sample_points": "input_data"}}}


def run(path, frames, dev):
    """frames[f][k]: frame f of drive k (host array or cuda tensor).  Returns (seconds, per-member relative poses, rows of
    the last cloud out)."""
    b = len(frames[0])
    rows = 0
    if path == "one_call_library":
        ctxs = [IcpContext(height=H, width=W, max_num_alignments=20, threshold_delta_pose=1.0e-4, scheme="neighborhood",
                           sigma=0.2, local_map_size=30, num_neighbors_normals=10, device=dev.index or 0) for _ in range(b)]
        batch = IcpBatch(ctxs)
        batch.use_torch_stream()
        batch.odometry_init(voxel_size=0.4, threshold_trans=0.1, threshold_rot=0.3, constant_velocity=True, targets=1)
        rel = [[] for _ in range(b)]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for step in frames:
            batch.frame_launch(step)
            for k, r in enumerate(batch.frame_end()):
                rel[k].append(r.pose)
                rows = 0 if r.points is None else r.points.shape[0]
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        batch.close()
        for c in ctxs:
            c.close()
        return dt, [np.stack(r) for r in rel], rows
    odo = our.MI355XICPFrameToModelBatch(published_config(path == "one_call_plugin"), b, projector=our.SphericalProjector(H, W),
                                         device=dev)
    pre = our.MI355XPreprocessingBatch(chain(dev), b, device=dev)
    init = [our.ConstantVelocityInitialization() for _ in range(b)]
    odo.init()
    for i in init:
        i.init()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for f, step in enumerate(frames):
        dicts = []
        for k in range(b):
            d = {"numpy_pc": step[k]}
            init[k].next_frame(d)
            dicts.append(d)
        pre.forward(dicts)
        odo.process_next_frames(dicts)
        if f > 0:
            for k, d in enumerate(dicts):
                init[k].save_real_motion(d["odometry_pose"], d)
            rows = dicts[-1]["odometry_pc"].shape[0]
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    rel = [odo.get_relative_poses(k)[:, :, :] for k in range(b)]
    odo.batch.close()
    pre.batch.close()
    for m in odo.members:
        m.ctx.close()
    return dt, rel, rows


def ab(frames, dev, passes):
    b, steps = len(frames[0]), len(frames)
    for path in PATHS:  # (untimed: kernels loaded, pinned buffers and streams made)
        run(path, frames, dev)
    fps = {p: [] for p in PATHS}
    rels, rows = {}, {}
    for _ in range(passes):
        for path in PATHS:
            dt, rels[path], rows[path] = run(path, frames, dev)
            fps[path].append(b * steps / dt)
    out = {}
    for path in PATHS:
        ms = [1e3 * b / v for v in fps[path]]
        out[path] = {"frames_per_s": [round(v, 1) for v in fps[path]], "ms_per_step": [round(v, 4) for v in ms],
                     "frames_per_s_range": [round(min(fps[path]), 1), round(max(fps[path]), 1)],
                     "frames_per_s_median": round(float(np.median(fps[path])), 1),
                     "ms_per_step_range": [round(min(ms), 4), round(max(ms), 4)],
                     "ms_per_step_median": round(float(np.median(ms)), 4), "cloud_rows_out": int(rows[path])}
    equal = all(np.array_equal(np.asarray(a).reshape(-1, 4, 4), np.asarray(w).reshape(-1, 4, 4))
                for p in PATHS[1:] for a, w in zip(rels[p], rels[PATHS[0]]))
    out["trajectories_equal"] = bool(equal)
    assert equal, "the three paths must give every member the same trajectory, bit for bit"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ab", type=int, default=3, help="timed passes of every path, alternating inside this process")
    ap.add_argument("--batch", type=int, nargs="+", default=[8, 16])
    ap.add_argument("--inputs", nargs="+", choices=["host", "device"], default=["host", "device"])
    ap.add_argument("--frames", type=int, default=36, help="frames per drive")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batched_frame_loop.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    seqs = [make_sequence(SceneConfig(height=H, width=W, seed=1234 + 1000 * k, step=0.3 + 0.05 * (k % 5)), args.frames)[0]
            for k in range(max(args.batch))]
    for b in args.batch:
        for kind in args.inputs:
            frames = [[seqs[k][f] for k in range(b)] for f in range(args.frames)]
            if kind == "device":
                frames = [[torch.from_numpy(s).to(dev) for s in step] for step in frames]
            result = {"tool": "batched_frame_loop", "ab": args.ab, "device": torch.cuda.get_device_name(0), "B": b,
                      "input": kind, "frames_per_member": args.frames, **ab(frames, dev, args.ab)}
            line = json.dumps(result)
            print(line, flush=True)
            if args.out:
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "a") as fh:
                    fh.write(line + "\n")


if __name__ == "__main__":
    main()
