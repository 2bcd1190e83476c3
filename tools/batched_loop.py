"""Developer tool (not a bench.py leg): B copies of the published configuration through `MI355XICPFrameToModelBatch`.

B synthetic drives (different seeds and speeds, 36 frames of 64x2048 each), preprocessed on the device as in
config/slam/preprocessing/grid_sample_mi355x.yaml with the padded grid sample (upload, de-skew, grid sample 0.4 m),
registered with one launch per ICP iteration for all B and updated with one map update for all B (key frames, evictions,
grid rebuilds, neighbourhood lists, eager normals).  `--preprocessing members`: the four single filters per member;
`batched`: one `MI355XPreprocessingBatch` call for all B.  `--timestamps`: every frame carries seeded, sorted synthetic
timestamps, so the de-skew runs (the drives have none otherwise).  The same frames then run through B single
`MI355XICPFrameToModel` plugins on the single-filter chain, one after the other, for comparison.  Prints one JSON line:
B, frames/s and ms per step of both, and the per-member ATE against ground truth of both.

usage: python tools/batched_loop.py --batch 8 [--frames 36] [--repeats 1] [--preprocessing members|batched] [--timestamps]"""
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
from pylidar_slam_amd.synthetic import SceneConfig, make_sequence  # noqa: E402

H, W = 64, 2048


def published_config():
    """docs/results/KITTI/kitti_benchmark.md:19 of the reference: <= 20 iterations, stop at 1e-4, 30 key frames."""
    return our.MI355XICPConfig(max_num_alignments=20, threshold_delta_pose=1.0e-4, data_key="input_data",
                               local_map=dict(type="kdtree_local_map", local_map_size=30, num_neighbors_normals=10),
                               alignment=dict(mode="point_to_plane_gauss_newton",
                                              gauss_newton_config=dict(max_iters=1, scheme="neighborhood", sigma=0.2)))


def chain(dev):
    """config/slam/preprocessing/grid_sample_mi355x.yaml with 0.4 m voxels and the padded grid sample."""
    return {"0": {"filter_name": "to_device_mi355x", "device": str(dev),
                  "keys": {"numpy_pc": "pc_device", "numpy_pc_timestamps": "timestamps_device"}},
            "1": {"filter_name": "distortion_mi355x", "force": False, "activate": True, "pointcloud_key": "pc_device",
                  "timestamps_key": "timestamps_device", "output_key": "distorted"},
            "2": {"filter_name": "grid_sample_mi355x", "voxel_size": 0.4, "pointcloud_key": "distorted", "padded": True},
            "3": {"filter_name": "to_tensor_mi355x", "device": str(dev), "dtype": "float32",
                  "keys": {"sample_points": "input_data"}}}


def filters(dev):
    c = chain(dev)
    return [our.ToDevice(our.ToDeviceConfig(**c["0"]), device=dev), our.Distortion(our.DistortionConfig(**c["1"])),
            our.GridSample(our.GridSampleConfig(**c["2"])), our.ToTensor(our.ToTensorConfig(**c["3"]), device=dev)]


def frame(seqs, k, f, stamps):
    """Frame f of drive k as the dataset hands it over (seeded sorted timestamps with --timestamps)."""
    s = seqs[k][0][f]
    d = {"numpy_pc": s}
    if stamps:
        d["numpy_pc_timestamps"] = np.sort(np.random.default_rng(100000 * k + f).uniform(0.0, 0.1, s.shape[0]))
    return d


def ate(rel, gt_abs):
    gt_rel = ev.compute_relative_poses(gt_abs)
    gt_rel[0] = np.eye(4)
    return float(ev.compute_ate(np.asarray(rel, np.float64), gt_rel)[0])


def run_batched(seqs, dev, preprocessing="members", stamps=False):
    b = len(seqs)
    odo = our.MI355XICPFrameToModelBatch(published_config(), b, projector=our.SphericalProjector(H, W), device=dev)
    pre = our.MI355XPreprocessingBatch(chain(dev), b, device=dev) if preprocessing == "batched" else None
    flt = [filters(dev) for _ in range(b)] if pre is None else None
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
            d = frame(seqs, k, f, stamps)
            init[k].next_frame(d)
            if pre is None:
                for x in flt[k]:
                    x.filter(d)
            dicts.append(d)
        if pre is not None:
            pre.forward(dicts)
        odo.process_next_frames(dicts)
        if f > 0:
            for k, d in enumerate(dicts):
                init[k].save_real_motion(d["odometry_pose"], d)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    rel = [odo.get_relative_poses(k) for k in range(b)]
    odo.batch.close()
    if pre is not None:
        pre.batch.close()
    return dt, rel


def run_single(seqs, dev, stamps=False):
    dt, rel = 0.0, []
    for k, (scans, _) in enumerate(seqs):
        odo = our.MI355XICPFrameToModel(published_config(), projector=our.SphericalProjector(H, W), device=dev)
        flt = filters(dev)
        init = our.ConstantVelocityInitialization()
        odo.init()
        init.init()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for f, s in enumerate(scans):
            d = frame(seqs, k, f, stamps)
            init.next_frame(d)
            for x in flt:
                x.filter(d)
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
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--frames", type=int, default=36)
    ap.add_argument("--repeats", type=int, default=1, help="timed passes of each loop (the best one is reported)")
    ap.add_argument("--no-single", action="store_true", help="skip the single-plugin comparison")
    ap.add_argument("--preprocessing", choices=["members", "batched"], default="members",
                    help="the single-filter chain per member, or one MI355XPreprocessingBatch call for all members")
    ap.add_argument("--timestamps", action="store_true", help="seeded sorted timestamps per frame: the de-skew runs")
    ap.add_argument("--ab", type=int, default=0,
                    help="instead: N timed passes of each preprocessing mode, alternating (members, batched, members, ...)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    seqs = [make_sequence(SceneConfig(height=H, width=W, seed=1234 + 1000 * k, step=0.3 + 0.05 * (k % 5)), args.frames)
            for k in range(args.batch)]
    frames = args.batch * args.frames
    if args.ab:
        for mode in ("members", "batched"):  # (warm-up of both)
            run_batched(seqs[:1], dev, mode, args.timestamps)
        runs = {"members": [], "batched": []}
        rels = {}
        for _ in range(args.ab):
            for mode in ("members", "batched"):
                dt, rels[mode] = run_batched(seqs, dev, mode, args.timestamps)
                runs[mode].append(frames / dt)
        print(json.dumps({"tool": "batched_loop", "ab": args.ab, "B": args.batch, "frames_per_member": args.frames,
                          "timestamps": bool(args.timestamps), "members_frames_per_s": runs["members"],
                          "batched_frames_per_s": runs["batched"],
                          "trajectories_equal": all(np.array_equal(a, b) for a, b in zip(rels["members"], rels["batched"]))}))
        return
    run_batched(seqs[:1], dev, args.preprocessing, args.timestamps)  # (warm-up: kernels loaded, allocations made)
    best_b, rel_b = min((run_batched(seqs, dev, args.preprocessing, args.timestamps) for _ in range(args.repeats)),
                        key=lambda r: r[0])
    out = {"tool": "batched_loop", "B": args.batch, "frames_per_member": args.frames,
           "preprocessing": args.preprocessing, "timestamps": bool(args.timestamps),
           "batched_frames_per_s": frames / best_b, "batched_ms_per_step": 1e3 * best_b / args.frames,
           "batched_ate_m": [ate(r, g) for r, (_, g) in zip(rel_b, seqs)]}
    if not args.no_single:
        best_s, rel_s = min((run_single(seqs, dev, args.timestamps) for _ in range(args.repeats)), key=lambda r: r[0])
        out.update({"single_frames_per_s": frames / best_s, "single_ms_per_frame": 1e3 * best_s / frames,
                    "single_ate_m": [ate(r, g) for r, (_, g) in zip(rel_s, seqs)],
                    "trajectories_equal": all(np.array_equal(a, b) for a, b in zip(rel_b, rel_s))})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
