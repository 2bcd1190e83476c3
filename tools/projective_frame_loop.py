"""Developer tool (not a bench.py leg): the projective frame loop (PF2M) behind two library calls against the per-call
plugin, in one process.

Workload: the synthetic 64x1024 PF2M drive of tools/batched_projective_loop.py (vertex maps on the device, projective local
map of 20, point-to-plane with <= 15 alignments, neighborhood weighting sigma 0.2, live 1e-4 stop, CV initialisation), 24
frames: ONE sequence, then B = 8 and B = 16 drives (different seeds and speeds) a step.  Pose and cloud out on every path.
Three paths (for B drives: `MI355XICPFrameToModelBatch` and `IcpBatch.pmap_frame_launch` / `pmap_frame_end`):

  per_call          `MI355XICPFrameToModel` as it stands (`one_call_projective_frame=False`): icp_pmap_register polls the
                    host every four iterations, the transposition, the key-frame arithmetic and `odometry_pc` run in torch;
  one_call_plugin   the same plugin with `one_call_projective_frame=True`: a frame is icp_pmap_frame_launch +
                    icp_pmap_frame_end;
  one_call_library  `IcpContext.pmap_frame_launch` + `pmap_frame_end` alone, the constant-velocity guess kept by the library.

`--ab N`: N timed passes of every path, alternating (per_call, one_call_plugin, one_call_library, per_call, ...) inside this
process, after one untimed pass of each.  ASSERTS that the three paths give every sequence the same trajectory, bit for bit.
Prints one JSON line per size — frames/s and ms per frame (per step for B drives) of every pass, their range and median —
and appends it to profiles/projective_frame_loop.jsonl (`--out`).

usage: python tools/projective_frame_loop.py [--ab 3] [--frames 24] [--batch 8 16]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "pylidar-slam_amd"), ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from pylidar_slam_amd import odometry as our  # noqa: E402
from pylidar_slam_amd.engine import IcpBatch, IcpContext  # noqa: E402
from batched_projective_loop import H, W, drives, pf2m_config  # noqa: E402

PATHS = ("per_call", "one_call_plugin", "one_call_library")


def run(path, vmaps, dev):
    """Returns (seconds, relative poses [F,4,4], rows of the last cloud out)."""
    rows = 0
    if path == "one_call_library":
        ctx = IcpContext(height=H, width=W, max_num_alignments=15, threshold_delta_pose=1.0e-4, scheme="neighborhood",
                         sigma=0.2, local_map_size=20, device=dev.index or 0)
        ctx.use_torch_stream()
        ctx.pmap_odometry_init(threshold_trans=0.1, threshold_rot=0.3, constant_velocity=True, normals_kernel_size=5)
        rel = []
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for v in vmaps:
            ctx.pmap_frame_launch(v)
            r = ctx.pmap_frame_end()
            rel.append(r.pose)
            rows = 0 if r.points is None else r.points.shape[0]
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        ctx.close()
        return dt, np.stack(rel), rows
    cfg = pf2m_config()
    cfg.one_call_projective_frame = path == "one_call_plugin"
    odo = our.MI355XICPFrameToModel(cfg, projector=our.SphericalProjector(H, W), device=dev)
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
            rows = d["odometry_pc"].shape[0]
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    rel = odo.get_relative_poses()
    odo.ctx.close()
    return dt, rel, rows


def run_batch(path, seqs, dev):
    """seqs[k]: the vertex maps of drive k.  Returns (seconds, per-member relative poses, rows of the last cloud out)."""
    b, frames, rows = len(seqs), len(seqs[0]), 0
    if path == "one_call_library":
        ctxs = [IcpContext(height=H, width=W, max_num_alignments=15, threshold_delta_pose=1.0e-4, scheme="neighborhood",
                           sigma=0.2, local_map_size=20, device=dev.index or 0) for _ in range(b)]
        batch = IcpBatch(ctxs)
        batch.use_torch_stream()
        batch.pmap_odometry_init(threshold_trans=0.1, threshold_rot=0.3, constant_velocity=True, normals_kernel_size=5)
        rel = [[] for _ in range(b)]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for f in range(frames):
            batch.pmap_frame_launch([s[f] for s in seqs])
            for k, r in enumerate(batch.pmap_frame_end()):
                rel[k].append(r.pose)
                rows = 0 if r.points is None else r.points.shape[0]
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        batch.close()
        for c in ctxs:
            c.close()
        return dt, [np.stack(r) for r in rel], rows
    cfg = pf2m_config()
    cfg.one_call_projective_frame = path == "one_call_plugin"
    odo = our.MI355XICPFrameToModelBatch(cfg, b, projector=our.SphericalProjector(H, W), device=dev)
    init = [our.ConstantVelocityInitialization() for _ in range(b)]
    odo.init()
    for i in init:
        i.init()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for f in range(frames):
        dicts = []
        for k in range(b):
            d = {"vertex_map": seqs[k][f]}
            init[k].next_frame(d)
            dicts.append(d)
        odo.process_next_frames(dicts)
        if f > 0:
            for k, d in enumerate(dicts):
                init[k].save_real_motion(d["odometry_pose"], d)
            rows = dicts[-1]["odometry_pc"].shape[0]
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    rel = [odo.get_relative_poses(k) for k in range(b)]
    odo.batch.close()
    for m in odo.members:
        m.ctx.close()
    return dt, rel, rows


def ab(vmaps, dev, passes, batched=False):
    """vmaps: one drive's vertex maps, or (batched) a list of drives."""
    frames = len(vmaps[0]) if batched else len(vmaps)
    members = len(vmaps) if batched else 1
    runner = run_batch if batched else run
    for path in PATHS:  # (untimed: kernels loaded, pinned buffers and streams made)
        runner(path, vmaps, dev)
    fps = {p: [] for p in PATHS}
    rels, rows = {}, {}
    for _ in range(passes):
        for path in PATHS:
            dt, rels[path], rows[path] = runner(path, vmaps, dev)
            fps[path].append(members * frames / dt)
    out = {}
    for path in PATHS:
        ms = [1e3 * members / v for v in fps[path]]
        out[path] = {"frames_per_s": [round(v, 1) for v in fps[path]], "ms_per_frame": [round(v, 4) for v in ms],
                     "frames_per_s_range": [round(min(fps[path]), 1), round(max(fps[path]), 1)],
                     "frames_per_s_median": round(float(np.median(fps[path])), 1),
                     "ms_per_frame_range": [round(min(ms), 4), round(max(ms), 4)],
                     "ms_per_frame_median": round(float(np.median(ms)), 4), "cloud_rows_out": int(rows[path])}
    equal = all(np.array_equal(np.asarray(rels[p]).reshape(-1, 4, 4), np.asarray(rels[PATHS[0]]).reshape(-1, 4, 4))
                for p in PATHS[1:])
    out["trajectories_equal"] = bool(equal)
    assert equal, "the three paths must give the same trajectory, bit for bit"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ab", type=int, default=3, help="timed passes of every path, alternating inside this process")
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--batch", type=int, nargs="*", default=[8, 16], help="B drives a step, behind the single sequence")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "projective_frame_loop.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    seqs = [v for v, _ in drives(max([1] + args.batch), args.frames, dev)]
    for b in [1] + args.batch:
        body = ab(seqs[0], dev, args.ab) if b == 1 else ab(seqs[:b], dev, args.ab, batched=True)
        result = {"tool": "projective_frame_loop", "ab": args.ab, "device": torch.cuda.get_device_name(0), "sequences": b,
                  "frames": args.frames, "ms_per_frame_means": "ms per frame" if b == 1 else "ms per step of B frames", **body}
        line = json.dumps(result)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as fh:
                fh.write(line + "\n")


if __name__ == "__main__":
    main()
