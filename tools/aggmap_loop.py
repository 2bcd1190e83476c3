"""Developer tool (not a bench.py leg): what the aggregated world map (`MI355XICPConfig.aggregate_map_voxel`,
`IcpContext.aggregated_map`, icp_aggmap_*) costs and how fast it is, on a 36-frame synthetic drive of 64x2048 scans
(131 072 rows a frame, cuda tensors) at voxel 0.2 m.

Legs, alternated inside this process (`--ab N`: N timed passes of every leg, after one untimed pass of each):
  plugin_off   `MI355XICPFrameToModel` over the drive with the option at 0 — frames/s;
  plugin_on    the same with `aggregate_map_voxel` = 0.2: every frame's cloud goes into the map — frames/s;
  insert       bare `AggregatedMap.insert` of frames 1.. as device tensors with the poses of the plugin run, into a cleared
               map — inserts/s and rows/s;
  torch_unique baseline in torch-ROCm: the same float64 world points and voxel keys per frame (elementwise, so the same bits),
               concatenated, then `torch.unique` — rows/s.
A plugin pass times the 35 frames behind frame 0; an insert or baseline pass repeats the whole drive (a clear and 35 inserts; 35
key computations, one concatenation, one `torch.unique`) until at least `--min-window` seconds have passed.  Every window is
closed by a device synchronise.  Per leg: every pass, their median and range.

Before anything is timed the tool ASSERTS that the map of the plugin run and the map of the bare inserts hold exactly the
baseline's voxel set (the keys recomputed from the map's float64 points), that nothing was dropped or set aside, and that the
poses with the option on equal those with it off, bit for bit.

Appends one JSON line to profiles/aggmap_loop.jsonl (`--out`).

usage: python tools/aggmap_loop.py [--ab 3] [--frames 36] [--min-window 0.5]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "pylidar-slam_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

HEIGHT, WIDTH, VOXEL, CAPACITY = 64, 2048, 0.2, 2000000
OFFSET = 1 << 20


def torch_keys(torch, pts, pose, voxel):
    """int64 voxel keys of the rows of `pts` [n,3] float32 (cuda) moved by `pose`: the map's arithmetic, elementwise in float64"""
    p = pts.double()
    m = pose
    c = [torch.round((((m[i, 0] * p[:, 0] + m[i, 1] * p[:, 1]) + m[i, 2] * p[:, 2]) + m[i, 3]) / voxel).long() + OFFSET
         for i in range(3)]
    return c[0] | (c[1] << 21) | (c[2] << 42)


def numpy_keys(w, voxel):
    c = np.rint(w / np.float64(voxel)).astype(np.int64) + OFFSET
    return c[:, 0] | (c[:, 1] << 21) | (c[:, 2] << 42)


def run_plugin(torch, frames, voxel, sync):
    """the drive through the plugin; (plugin, seconds for the frames behind frame 0)"""
    from pylidar_slam_amd import odometry as our
    dev = torch.device("cuda:0")
    cfg = our.MI355XICPConfig(max_num_alignments=8, threshold_delta_pose=0.0, data_key="input_data",
                              aggregate_map_voxel=voxel, aggregate_map_capacity=CAPACITY)
    odo = our.MI355XICPFrameToModel(cfg, projector=our.SphericalProjector(HEIGHT, WIDTH), device=dev)
    odo.init()
    odo.process_next_frame({"input_data": frames[0]})
    sync()
    t0 = time.perf_counter()
    for f in frames[1:]:
        odo.process_next_frame({"input_data": f})
    sync()
    return odo, time.perf_counter() - t0


def repeated(call, sync, min_window):
    """calls per second of `call`, repeated until at least `min_window` seconds have passed, the window closed by a synchronise"""
    sync()
    t0 = time.perf_counter()
    reps = 0
    while True:
        call()
        reps += 1
        if time.perf_counter() - t0 >= min_window:
            break
    sync()
    return reps / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ab", type=int, default=3)
    ap.add_argument("--frames", type=int, default=36)
    ap.add_argument("--min-window", type=float, default=0.5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "aggmap_loop.jsonl"))
    args = ap.parse_args()

    import torch
    from pylidar_slam_amd.synthetic import SceneConfig, make_sequence
    assert torch.cuda.is_available(), "tools/aggmap_loop.py measures on the GPU: none is visible"
    sync = torch.cuda.synchronize
    scans, _ = make_sequence(SceneConfig(height=HEIGHT, width=WIDTH), args.frames)
    frames = [torch.from_numpy(np.ascontiguousarray(s, dtype=np.float32)).cuda() for s in scans]
    rows = sum(int(f.shape[0]) for f in frames[1:])

    # ---- the checked configuration (also the untimed pass of every leg) --------------------------------------------------
    off, _ = run_plugin(torch, frames, 0.0, sync)
    on, _ = run_plugin(torch, frames, VOXEL, sync)
    assert off.aggregated_map is None and on.aggregated_map is not None
    poses = np.stack(on.absolute_poses)
    assert np.array_equal(poses.view(np.uint64), np.stack(off.absolute_poses).view(np.uint64)), "the option changed a pose"
    poses_dev = [torch.from_numpy(p).cuda() for p in poses]

    def baseline():
        return torch.unique(torch.cat([torch_keys(torch, f, poses_dev[k + 1], VOXEL) for k, f in enumerate(frames[1:])]))

    want = np.sort(baseline().cpu().numpy())
    bare = on.ctx.aggregated_map(VOXEL, CAPACITY)

    def inserts():
        bare.clear()
        for k, f in enumerate(frames[1:]):
            bare.insert(f, poses[k + 1], k + 1)

    inserts()
    for name, m in (("plugin", on.aggregated_map), ("bare inserts", bare)):
        st = m.stats()
        assert st["dropped"] == st["out_of_range"] == st["nonfinite"] == st["error"] == 0 and st["inserts"] == len(frames) - 1, (name, st)
        got = np.sort(numpy_keys(m.points(dtype=np.float64), VOXEL))
        assert got.shape == want.shape and np.array_equal(got, want), f"{name}: the map is not the baseline's voxel set"
    size = bare.stats()["size"]
    del off, on

    # ---- timed passes ----------------------------------------------------------------------------------------------------
    passes = {"plugin_off": [], "plugin_on": [], "insert": [], "torch_unique": []}
    for _ in range(args.ab):
        passes["plugin_off"].append((len(frames) - 1) / run_plugin(torch, frames, 0.0, sync)[1])
        passes["plugin_on"].append((len(frames) - 1) / run_plugin(torch, frames, VOXEL, sync)[1])
        passes["insert"].append((len(frames) - 1) * repeated(inserts, sync, args.min_window))
        passes["torch_unique"].append(rows * repeated(baseline, sync, args.min_window))
    units = {"plugin_off": "frames/s", "plugin_on": "frames/s", "insert": "inserts/s", "torch_unique": "rows/s"}
    line = {"tool": "tools/aggmap_loop.py", "frames": len(frames), "rows_per_frame": int(frames[0].shape[0]), "voxel": VOXEL,
            "capacity": CAPACITY, "map_size": int(size), "ab": args.ab, "min_window_s": args.min_window, "device": torch.cuda.get_device_name(0),
            "checked_against_torch_unique": True, "legs": {}}
    for name, v in passes.items():
        line["legs"][name] = {"unit": units[name], "passes": [round(x, 1) for x in v], "median": round(statistics.median(v), 1),
                              "min": round(min(v), 1), "max": round(max(v), 1)}
    per_insert = rows / (len(frames) - 1)
    line["legs"]["insert"]["rows_per_s"] = {k: round(line["legs"]["insert"][k] * per_insert, 1) for k in ("median", "min", "max")}
    text = json.dumps(line)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
