"""Developer tool (not a bench.py leg): how fast the elevation image (`IcpContext.elevation_image`, icp_elevation_*) is, per
frame and per window, on a 36-frame synthetic drive of 64x2048 scans (131 072 float32 rows a frame, cuda tensors), image
400 x 400 at 0.4 m, z in [-2, 5] of the sensor frame.

Legs, alternated inside this process (`--ab N`: N timed passes of every leg, after one untimed pass of each):
  frame          `ElevationImage.build` of one frame's device tensor — images/s;
  frame_torch    baseline in torch-ROCm on the same rows: linear pixel ids, `scatter_reduce` amax of the clipped z, a second
                 amax of the row among the rows that hold it, then a gather of theta, points and colours — images/s;
  frame_numpy    the numpy model (tests/elevation_audit.py) on the host copy of the same rows — images/s, a CPU figure;
  window         `ElevationImage.build_from` over the aggregated map of the whole drive (voxel 0.2 m), full window — images/s;
  window_host    what stands there without it: `AggregatedMap.submap` to the host, then the numpy model — images/s (CPU).
A pass repeats its call until at least `--min-window` seconds have passed; every window is closed by a device synchronise.
Per leg: every pass, their median and range.

Before anything is timed the tool ASSERTS that the device image of the frame equals the numpy model on every array (the pixels on
which the torch baseline differs from it are counted and reported) and that every filled pixel of the window image holds `submap`'s row.

`--kernels`: no baselines and no timing — 50 builds of each kind, for a `rocprofv3 --kernel-trace --stats` run of its own.

Appends one JSON line to profiles/elevation_loop.jsonl (`--out`).

usage: python tools/elevation_loop.py [--ab 3] [--frames 36] [--min-window 0.5] [--kernels]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "pylidar-slam_amd"), os.path.join(ROOT, "tests"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

HEIGHT, WIDTH, VOXEL, CAPACITY = 64, 2048, 0.2, 2000000
IMAGE = dict(height=400, width=400, pixel_size=0.4, z_min=-2.0, z_max=5.0)


def torch_image(torch, pts, table, h, w, pixel, z_min, z_max):
    """(rgb, theta, points, index) of float32 rows `pts` [n,3] (cuda) by torch-ROCm operators: the same arithmetic, elementwise"""
    # (tensor divisors: torch turns a division by a Python scalar into a multiplication by its reciprocal)
    pixel = torch.tensor(pixel, dtype=torch.float32, device=pts.device)
    den = torch.tensor(float(z_max) - float(z_min), dtype=torch.float32, device=pts.device)
    fx = torch.round(pts[:, 0] / pixel + float(h // 2))
    fy = torch.round(pts[:, 1] / pixel + float(w // 2))
    ok = (fx >= 0) & (fx < h) & (fy >= 0) & (fy < w) & ~torch.isnan(pts[:, 2])
    rows = torch.nonzero(ok).reshape(-1)
    pix = (fx[rows].long() * w + fy[rows].long())
    zc = torch.clamp(pts[rows, 2], z_min, z_max) + 0.0
    best = torch.full((h * w,), -float("inf"), dtype=torch.float32, device=pts.device).scatter_reduce(0, pix, zc, "amax")
    holds = zc == best[pix]
    index = torch.full((h * w,), -1, dtype=torch.int64, device=pts.device).scatter_reduce(0, pix[holds], rows[holds], "amax")
    filled = index >= 0
    safe = index.clamp(min=0)
    theta = torch.where(filled, (best - z_min) / den, torch.full_like(best, z_min))
    points = torch.where(filled[:, None], pts[safe], torch.zeros((h * w, 3), dtype=torch.float32, device=pts.device))
    t = theta * 256.0
    t = torch.where(t == 256.0, torch.full_like(t, 255.0), t)
    k = torch.where(t < 0, torch.full_like(t, 256.0), torch.where(t >= 256.0, torch.full_like(t, 257.0), torch.trunc(t))).long()
    return table[k].reshape(h, w, 3), theta.reshape(h, w), points.reshape(h, w, 3), index.to(torch.int32).reshape(h, w)


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
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "elevation_loop.jsonl"))
    args = ap.parse_args()

    import torch
    import elevation_audit as model
    from pylidar_slam_amd.engine import IcpContext
    from pylidar_slam_amd.synthetic import SceneConfig, make_sequence
    assert torch.cuda.is_available(), "tools/elevation_loop.py measures on the GPU: none is visible"
    sync = torch.cuda.synchronize
    scans, poses = make_sequence(SceneConfig(height=HEIGHT, width=WIDTH), args.frames)
    poses = np.asarray(poses, np.float64).reshape(-1, 4, 4)
    frames = [torch.from_numpy(np.ascontiguousarray(s, dtype=np.float32)).cuda() for s in scans]
    frame, frame_host = frames[args.frames // 2], np.ascontiguousarray(scans[args.frames // 2], dtype=np.float32)
    spec = model.Spec(IMAGE["height"], IMAGE["width"], IMAGE["pixel_size"], IMAGE["z_min"], IMAGE["z_max"], False)
    table = model.random_table(0)
    table_dev = torch.from_numpy(table).cuda()

    ctx = IcpContext(height=HEIGHT, width=WIDTH)
    image = ctx.elevation_image(color_map=table, max_rows=int(frame.shape[0]), **IMAGE)
    window_image = ctx.elevation_image(color_map=table, max_rows=1, **IMAGE)
    world = ctx.aggregated_map(VOXEL, CAPACITY)
    for k, f in enumerate(frames):
        world.insert(f, poses[k], k)
    back = np.linalg.inv(poses[args.frames // 2])
    lo, hi = 0, args.frames

    def build_frame():
        image.build(frame)

    def build_torch():
        return torch_image(torch, frame, table_dev, spec.height, spec.width, spec.pixel_size, spec.z_min, spec.z_max)

    def build_numpy():
        return model.build(frame_host, spec, table)

    def build_window():
        window_image.build_from(world, lo, hi, back)

    def build_window_host():
        xyz, _ = world.submap(lo, hi, back)
        return model.build(xyz, spec, table)

    if args.kernels:
        for _ in range(50):
            build_frame()
            image.build(frame.double())
            build_window()
        sync()
        print(json.dumps({"tool": "tools/elevation_loop.py", "kernels": True, "builds_of_each_kind": 50}))
        return

    # ---- the checked configuration (also the untimed pass of every leg) --------------------------------------------------
    build_frame()
    want = build_numpy()
    assert image.stats() == want["stats"], (image.stats(), want["stats"])
    for name, got in (("rgb", image.rgb), ("theta", image.theta), ("points", image.points_3d), ("index", image.indices)):
        assert np.array_equal(got.view(np.uint8), want[name].view(np.uint8)), f"the device image differs from the model in {name}"
    rgb, theta, points, index = build_torch()  # (a baseline, not the product: its differences are reported, not refused)
    baseline_differs = {"index": int((index.cpu().numpy() != want["index"]).sum()),
                        "rgb": int((rgb.cpu().numpy() != want["rgb"]).any(axis=-1).sum()),
                        "points": int((points.cpu().numpy().view(np.uint32) != want["points"].view(np.uint32)).any(axis=-1).sum())}
    build_window()
    xyz, idx = world.submap(lo, hi, back)
    rows = np.full((len(world), 3), np.nan, np.float32)
    rows[idx] = xyz
    w_index, w_points = window_image.indices, window_image.points_3d
    assert np.array_equal(w_points[w_index >= 0].view(np.uint32), rows[w_index[w_index >= 0]].view(np.uint32)), "window image"
    window_stats, map_size = window_image.stats(), len(world)
    build_window_host()

    # ---- timed passes ----------------------------------------------------------------------------------------------------
    legs = {"frame": build_frame, "frame_torch": build_torch, "frame_numpy": build_numpy, "window": build_window,
            "window_host": build_window_host}
    passes = {name: [] for name in legs}
    for _ in range(args.ab):
        for name, call in legs.items():
            passes[name].append(repeated(call, sync, args.min_window))
    line = {"tool": "tools/elevation_loop.py", "frames": len(frames), "rows_per_frame": int(frame.shape[0]), "image": IMAGE,
            "frame_stats": want["stats"], "voxel": VOXEL, "map_size": int(map_size), "window_stats": window_stats, "ab": args.ab,
            "min_window_s": args.min_window, "device": torch.cuda.get_device_name(0), "checked_against_model": True, "torch_baseline_pixels_that_differ": baseline_differs,
            "cpu_legs": ["frame_numpy", "window_host"], "legs": {}}
    for name, v in passes.items():
        line["legs"][name] = {"unit": "images/s", "passes": [round(x, 1) for x in v], "median": round(statistics.median(v), 1),
                              "min": round(min(v), 1), "max": round(max(v), 1),
                              "us_per_image": {"median": round(1e6 / statistics.median(v), 1), "min": round(1e6 / max(v), 1),
                                               "max": round(1e6 / min(v), 1)}}
    text = json.dumps(line)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
