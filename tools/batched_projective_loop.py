"""Developer tool (not a bench.py leg): the projective local map configuration (PF2M) through
`MI355XICPFrameToModelBatch`, B sequences per launch, against the single projective plugin.

PF2M (the reference's docs/results/KITTI/kitti_benchmark.md): 64x1024 vertex maps, projective_local_map with
local_map_size 20, point-to-plane with <= 15 alignments, neighborhood weighting (sigma 0.2), stop at 1e-4.  Synthetic
drives (different seeds and speeds), projected to vertex maps on the device before the timed loops.  For every B of
--batches: frames/s and ms per step of the batched loop, per-member ATE against ground truth; then the first --single
sequences through single `MI355XICPFrameToModel` plugins, one after the other: frames/s and ATE.  One JSON line per run.

usage: python tools/batched_projective_loop.py [--batches 1,4,8,16] [--frames 24] [--single 4] [--repeats 1]"""
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

from pylidar_slam_amd import eval as ev  # noqa: E402
from pylidar_slam_amd import odometry as our  # noqa: E402
from pylidar_slam_amd.engine import IcpContext  # noqa: E402
from pylidar_slam_amd.synthetic import SceneConfig, make_sequence  # noqa: E402

H, W = 64, 1024


def pf2m_config():
    return our.MI355XICPConfig(max_num_alignments=15, threshold_delta_pose=1.0e-4, data_key="vertex_map",
                               local_map=dict(type="projective_local_map", local_map_size=20),
                               alignment=dict(mode="point_to_plane_gauss_newton",
                                              gauss_newton_config=dict(max_iters=1, scheme="neighborhood", sigma=0.2)))


def drives(count, frames, dev):
    """(vertex maps on the device, ground-truth absolute poses) of `count` synthetic drives."""
    ctx = IcpContext(height=H, width=W, device=dev.index or 0)
    out = []
    for k in range(count):
        scans, gt = make_sequence(SceneConfig(height=H, width=W, seed=4321 + 1000 * k, step=0.3 + 0.05 * (k % 5),
                                              yaw_rate=0.004 * (1 + k % 3)), frames)
        out.append(([ctx.project(torch.from_numpy(np.ascontiguousarray(s, dtype=np.float32)).to(dev)).clone()
                     for s in scans], gt))
    torch.cuda.synchronize()
    ctx.close()
    return out


def ate(rel, gt_abs):
    gt_rel = ev.compute_relative_poses(gt_abs)
    gt_rel[0] = np.eye(4)
    return float(ev.compute_ate(np.asarray(rel, np.float64), gt_rel)[0])


def run_batched(seqs, dev):
    b = len(seqs)
    odo = our.MI355XICPFrameToModelBatch(pf2m_config(), b, projector=our.SphericalProjector(H, W), device=dev)
    init = [our.ConstantVelocityInitialization() for _ in range(b)]
    odo.init()
    for i in init:
        i.init()
    frames = len(seqs[0][0])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for f in range(frames):
        dicts = []
        for k in range(b):
            d = {"vertex_map": seqs[k][0][f]}
            init[k].next_frame(d)
            dicts.append(d)
        odo.process_next_frames(dicts)
        if f > 0:
            for k, d in enumerate(dicts):
                init[k].save_real_motion(d["odometry_pose"], d)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    rel = [odo.get_relative_poses(k) for k in range(b)]
    odo.batch.close()
    for m in odo.members:
        m.ctx.close()
    return dt, rel


def run_single(seqs, dev):
    dt, rel = 0.0, []
    for vmaps, _ in seqs:
        odo = our.MI355XICPFrameToModel(pf2m_config(), projector=our.SphericalProjector(H, W), device=dev)
        init = our.ConstantVelocityInitialization()
        odo.init()
        init.init()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for f, v in enumerate(vmaps):
            d = {"vertex_map": v}
            init.next_frame(d)
            odo.process_next_frame(d)
            if f > 0:
                init.save_real_motion(d["odometry_pose"], d)
        torch.cuda.synchronize()
        dt += time.perf_counter() - t0
        rel.append(odo.get_relative_poses())
        odo.ctx.close()
    return dt, rel


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,4,8,16")
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--single", type=int, default=4, help="sequences through the single plugin (0: none)")
    ap.add_argument("--repeats", type=int, default=1, help="timed passes of each loop (the best one is reported)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    batches = [int(b) for b in args.batches.split(",") if b]
    seqs = drives(max(batches + [args.single]), args.frames, dev)
    run_batched(seqs[:1], dev)  # (warm-up: kernels loaded, allocations made)
    for b in batches:
        best, rel = min((run_batched(seqs[:b], dev) for _ in range(args.repeats)), key=lambda r: r[0])
        print(json.dumps({"tool": "batched_projective_loop", "mode": "batched", "B": b, "frames_per_member": args.frames,
                          "frames_per_s": b * args.frames / best, "ms_per_step": 1e3 * best / args.frames,
                          "ate_m": [ate(r, g) for r, (_, g) in zip(rel, seqs)]}), flush=True)
    if args.single > 0:
        best, rel = min((run_single(seqs[:args.single], dev) for _ in range(args.repeats)), key=lambda r: r[0])
        print(json.dumps({"tool": "batched_projective_loop", "mode": "single", "sequences": args.single,
                          "frames_per_member": args.frames, "frames_per_s": args.single * args.frames / best,
                          "ms_per_frame": 1e3 * best / (args.single * args.frames),
                          "ate_m": [ate(r, g) for r, (_, g) in zip(rel, seqs)]}), flush=True)


if __name__ == "__main__":
    main()
