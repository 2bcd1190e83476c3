"""Developer tool (not a bench.py leg): how fast the cloud-to-cloud refinement (`IcpContext.cloud_refiner`, icp_refine_*) is on
the clouds the reference's loop closure hands to Open3D (slam/loop_closure.py:237-243): the `points_3D` of two elevation images.

A 36-frame synthetic drive of 64x2048 scans goes into an `AggregatedMap` (voxel 0.2 m); two overlapping windows of it (frames
0-23 and 12-35, each seen from its middle frame) become two `ElevationImage`s, at 400 x 400 / 0.4 m and at 1200 x 1200 / 0.1 m.
The candidate image is refined against the current one from the true relative pose disturbed by yaw 0.01 rad and (0.1, 0.05,
0) m, with the reference's settings (1.0 m, 30 iterations, 1e-6 / 1e-6).

Legs, alternated inside this process (`--ab N`: N timed passes of every leg, after one untimed pass of each), per image size:
  device   `CloudRefiner.refine(candidate image)` against the current image set as target once — refinements/s;
  torch    baseline in torch-ROCm on the same rows: chunked `torch.cdist` + `argmin`, `torch.linalg.svd`, the same loop in
           float32 distances and a float64 step — refinements/s;
  numpy    the numpy model's loop and step (tests/refine_audit.py) with `scipy.spatial.cKDTree(workers=16)` for the search on
           the host — refinements/s, a CPU figure.
A pass repeats its call until at least `--min-window` seconds have passed; every window is closed by a device synchronise.

Before anything is timed the tool ASSERTS the device result against the model (the numpy leg): equal iteration count and
`converged`, max|dT| below 1e-9; what the torch baseline differs by is reported, not refused.

`--kernels`: no baselines and no timing — 10 refinements of each size, for a `rocprofv3 --kernel-trace --stats` run of its own.

Appends one JSON line to profiles/refine_loop.jsonl (`--out`).

usage: python tools/refine_loop.py [--ab 3] [--frames 36] [--min-window 0.5] [--kernels]"""
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
IMAGES = {"400x400@0.4": dict(height=400, width=400, pixel_size=0.4, z_min=-2.0, z_max=5.0),
          "1200x1200@0.1": dict(height=1200, width=1200, pixel_size=0.1, z_min=-2.0, z_max=5.0)}
SETTINGS = dict(max_distance=1.0, max_iteration=30, relative_fitness=1e-6, relative_rmse=1e-6)


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


def torch_refine(torch, src, tgt, init, max_distance, max_iteration, relative_fitness, relative_rmse, chunk=2048):
    """(T, iterations, converged) by torch-ROCm operators: float32 cdist + argmin in chunks, the step by torch.linalg.svd in float64"""
    T = torch.from_numpy(init).cuda()
    src64, tgt64 = src.double(), tgt.double()
    prev = None
    it, converged = 0, False
    while True:
        p = src64 @ T[:3, :3].T + T[:3, 3]
        p32 = p.float()
        best_d, best_i = [], []
        for lo in range(0, len(p32), chunk):
            d, i = torch.cdist(p32[lo:lo + chunk], tgt).min(dim=1)
            best_d.append(d)
            best_i.append(i)
        d, i = torch.cat(best_d), torch.cat(best_i)
        hit = d < max_distance
        n = int(hit.sum())
        a, b = p[hit], tgt64[i[hit]]
        fitness = n / max(len(src), 1)
        rmse = float(torch.sqrt(((a - b) ** 2).sum(dim=1).mean())) if n else 0.0
        if prev is not None and abs(fitness - prev[0]) < relative_fitness and abs(rmse - prev[1]) < relative_rmse:
            converged = True
            break
        if it >= max_iteration:
            break
        prev = (fitness, rmse)
        up = torch.eye(4, dtype=torch.float64, device=T.device)
        if n:
            ma, mb = a.mean(dim=0), b.mean(dim=0)
            H = (b - mb).T @ (a - ma) / n
            U, _, Vt = torch.linalg.svd(H)
            s = torch.sign(torch.linalg.det(U) * torch.linalg.det(Vt))
            R = U @ torch.diag(torch.stack([torch.ones_like(s), torch.ones_like(s), s])) @ Vt
            up[:3, :3], up[:3, 3] = R, mb - R @ ma
        T = up @ T
        it += 1
    return T.cpu().numpy(), it, converged


def numpy_refine(model, src, tgt, init, max_distance, max_iteration, relative_fitness, relative_rmse):
    """the model's loop and step with a float64 cKDTree for the search (host)"""
    from scipy.spatial import cKDTree
    tree = cKDTree(tgt.astype(np.float64))
    T = np.array(init, np.float64)
    prev, it, converged = None, 0, False
    while True:
        P = model.move(T, src)
        d, i = tree.query(P, k=1, distance_upper_bound=max_distance, workers=16)
        hit = np.isfinite(d)
        n = int(hit.sum())
        fig = np.zeros(17)
        fig[0], fig[1] = n, float((d[hit] ** 2).sum())
        fitness, rmse = model.fitness_rmse(n, len(src), fig[1])
        if prev is not None and abs(fitness - prev[0]) < relative_fitness and abs(rmse - prev[1]) < relative_rmse:
            converged = True
            break
        if it >= max_iteration:
            break
        prev = (fitness, rmse)
        if n:
            p, q = P[hit], tgt[i[hit]].astype(np.float64)
            mp, mq = p.mean(axis=0), q.mean(axis=0)
            fig[2:5], fig[5:8], fig[8:] = mp, mq, ((q - mq).T @ (p - mp) / n).reshape(-1)
        T = model.mul44(model.step(fig), T)
        it += 1
    return T, it, converged


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ab", type=int, default=3)
    ap.add_argument("--frames", type=int, default=36)
    ap.add_argument("--min-window", type=float, default=0.5)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refine_loop.jsonl"))
    args = ap.parse_args()

    import torch
    import refine_audit as model
    from pylidar_slam_amd.engine import IcpContext
    from pylidar_slam_amd.synthetic import SceneConfig, make_sequence
    assert torch.cuda.is_available(), "tools/refine_loop.py measures on the GPU: none is visible"
    sync = torch.cuda.synchronize
    scans, poses = make_sequence(SceneConfig(height=HEIGHT, width=WIDTH), args.frames)
    poses = np.asarray(poses, np.float64).reshape(-1, 4, 4)
    ctx = IcpContext(height=HEIGHT, width=WIDTH)
    world = ctx.aggregated_map(VOXEL, CAPACITY)
    for k, s in enumerate(scans):
        world.insert(torch.from_numpy(np.ascontiguousarray(s, dtype=np.float32)).cuda(), poses[k], k)
    third = args.frames // 3
    windows = {"candidate": (0, 2 * third, third), "current": (third, args.frames, 2 * third)}  # (lo, hi, middle frame)
    truth = np.linalg.inv(poses[windows["current"][2]]) @ poses[windows["candidate"][2]]  # candidate frame into current frame
    init = model.rigid(0.01, (0.1, 0.05, 0.0)) @ truth
    table = np.zeros((259, 3), np.uint8)

    line = {"tool": "tools/refine_loop.py", "frames": len(scans), "voxel": VOXEL, "map_size": len(world), "settings": SETTINGS, "ab": args.ab,
            "min_window_s": args.min_window, "device": torch.cuda.get_device_name(0), "checked_against_model": True, "cpu_legs": ["numpy"],
            "images": {}}
    for name, geometry in IMAGES.items():
        pixels = geometry["height"] * geometry["width"]
        images = {}
        for which, (lo, hi, mid) in windows.items():
            images[which] = ctx.elevation_image(color_map=table, max_rows=1, **geometry)
            images[which].build_from(world, lo, hi, np.linalg.inv(poses[mid]))
        refiner = ctx.cloud_refiner(pixels, pixels, 1.0)
        refiner.set_target(images["current"])

        def run_device():
            return refiner.refine(images["candidate"], init=init, **SETTINGS)

        if args.kernels:
            for _ in range(10):
                refiner.set_target(images["current"])
                run_device()
            sync()
            continue
        rows = {}
        for which, img in images.items():
            pts = img.points_3d.reshape(-1, 3)
            rows[which] = np.ascontiguousarray(pts[~model.zero_rows(pts)])
        src_dev, tgt_dev = torch.from_numpy(rows["candidate"]).cuda(), torch.from_numpy(rows["current"]).cuda()

        def run_torch():
            return torch_refine(torch, src_dev, tgt_dev, init, **SETTINGS)

        def run_numpy():
            return numpy_refine(model, rows["candidate"], rows["current"], init, **SETTINGS)

        # ---- the checked configuration (also the untimed pass of every leg) ----------------------------------------------
        got = run_device()
        want_T, want_it, want_conv = run_numpy()
        dT = float(np.abs(got.transformation - want_T).max())
        assert got.iterations == want_it and got.converged == want_conv and dT < 1e-9, (name, got.iterations, want_it, dT)
        assert got.source_rows == len(rows["candidate"]) and got.target_rows == len(rows["current"])
        t_T, t_it, t_conv = run_torch()  # (a baseline, not the product: its differences are reported, not refused)
        legs = {"device": run_device, "torch": run_torch, "numpy": run_numpy}
        passes = {leg: [] for leg in legs}
        for _ in range(args.ab):
            for leg, call in legs.items():
                passes[leg].append(repeated(call, sync, args.min_window))
        entry = {"image": geometry, "source_rows": len(rows["candidate"]), "target_rows": len(rows["current"]), "iterations": got.iterations,
                 "converged": got.converged, "fitness": got.fitness, "inlier_rmse": got.inlier_rmse, "max_abs_dT_device_vs_model": dT,
                 "distance_of_result_from_truth": float(np.abs(got.transformation - truth).max()),
                 "torch_baseline": {"iterations": t_it, "converged": t_conv, "max_abs_dT_vs_model": float(np.abs(t_T - want_T).max())}, "legs": {}}
        for leg, v in passes.items():
            entry["legs"][leg] = {"unit": "refinements/s", "passes": [round(x, 3) for x in v], "median": round(statistics.median(v), 3),
                                  "ms_per_refinement": {"median": round(1e3 / statistics.median(v), 3), "min": round(1e3 / max(v), 3),
                                                        "max": round(1e3 / min(v), 3)}}
        line["images"][name] = entry
        refiner.close()
        for img in images.values():
            img.close()
    if args.kernels:
        print(json.dumps({"tool": "tools/refine_loop.py", "kernels": True, "refinements_of_each_size": 10}))
        return
    text = json.dumps(line)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
