"""Developer tool (not a bench.py leg): the rate of the k-NN query (`IcpContext.knn_query`, icp_knn_query) on the GPU, at the
bench's C2 shapes — the 131 072 points of one 64x2048 synthetic scan queried against the fixed 100 000-point map of
`pylidar_slam_amd.synthetic.make_c2_workload` — with device tensors in and out.

Legs, alternated inside this process (`--ab N`: N timed passes of every leg after every shape has been warmed):
  knn_k1, knn_k11, knn_k32   `knn_query(queries, k)` for k = 1, 11, 32;
  nn_search                  baseline (a): `nearest_neighbor_search(queries, with_normals=False, with_index=True)`, the 1-NN the
                             library had before, next to knn_k1;
  ckdtree_k1 / _k11 / _k32   baseline (b): `scipy.spatial.cKDTree(map).query(queries, k, workers=16)` on the HOST — a CPU
                             figure on 16 threads, the stand-in this project uses for pykdtree (tree built outside the window).
A timed window repeats the call until at least 0.5 s have passed and is closed by a device synchronise; the figure is queries
per second.  Per leg: every pass, their median and range.

Before anything is timed the tool ASSERTS, at this size, that the indices of every k agree with cKDTree on every row that is
not ambiguous (two consecutive truth distances among the first k + 1 closer than 1e-6 relative), that at most 1 % of the rows
are, and that k = 1 agrees with `nearest_neighbor_search` on every row: the timed configuration is a checked one.

Appends one JSON line to profiles/knn_query.jsonl (`--out`).  `--profile-pass`: one untimed pass of the GPU legs only, for a
`rocprofv3 --kernel-trace --stats` run of its own (-> profiles/knn_query_kernel_stats.csv).

usage: python tools/knn_loop.py [--ab 3] [--ks 1 11 32] [--min-window 0.5]"""
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

AMBIGUOUS_REL, AMBIGUOUS_MAX = 1.0e-6, 1.0e-2
CPU_THREADS = 16


def workload():
    """(map [100 000, 3], queries [131 072, 3]) of sequence 0 of the bench's C2 configuration"""
    from pylidar_slam_amd.synthetic import make_c2_workload
    scans, _, model, order, _ = make_c2_workload(0, "loop", 1)
    queries = np.ascontiguousarray(scans[order[0]], dtype=np.float32).reshape(-1, 3)
    queries = queries[np.isfinite(queries).all(axis=1)]
    return np.ascontiguousarray(model, dtype=np.float32), queries


def check_against_ckdtree(ctx, tree, map_pts, queries_dev, queries, ks):
    """the agreement the timed configuration is held to; returns the ambiguous share per k"""
    shares = {}
    kmax = max(ks)
    td, ti = tree.query(queries.astype(np.float64), k=kmax + 1, workers=CPU_THREADS)
    for k in ks:
        dist, index = ctx.knn_query(queries_dev, k=k)
        index, dist = index.cpu().numpy(), dist.cpu().numpy()
        t = td[:, :k + 1]
        amb = np.any((t[:, 1:] - t[:, :-1]) < AMBIGUOUS_REL * t[:, 1:], axis=1)
        shares[k] = float(amb.mean())
        assert shares[k] <= AMBIGUOUS_MAX, f"k = {k}: {shares[k]:.3%} of the rows are ambiguous"
        bad = np.flatnonzero(np.any(index != ti[:, :k], axis=1) & ~amb)
        assert bad.size == 0, f"k = {k}: {bad.size} unambiguous rows disagree with cKDTree, first {bad[:5].tolist()}"
        rel = np.abs(dist.astype(np.float64) - td[:, :k]) / np.maximum(td[:, :k], 1e-30)
        assert rel.max() <= 4 * 2.0 ** -23, f"k = {k}: a distance is {rel.max():.3e} (relative) from cKDTree's"
    _, _, nn = ctx.nearest_neighbor_search(queries_dev, with_normals=False, with_index=True)
    _, index = ctx.knn_query(queries_dev, k=1)
    assert bool((index[:, 0] == nn).all()), "k = 1 disagrees with nearest_neighbor_search"
    return shares


def timed(call, sync, n_queries, min_window):
    sync()
    t0 = time.perf_counter()
    reps = 0
    while True:
        call()
        reps += 1
        if time.perf_counter() - t0 >= min_window:  # (the host clock: the calls of a leg synchronise themselves)
            break
    sync()
    return reps * n_queries / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ab", type=int, default=3)
    ap.add_argument("--ks", type=int, nargs="+", default=[1, 11, 32])
    ap.add_argument("--min-window", type=float, default=0.5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_query.jsonl"))
    ap.add_argument("--profile-pass", action="store_true")
    args = ap.parse_args()

    import torch
    from scipy.spatial import cKDTree
    from pylidar_slam_amd.engine import IcpContext
    assert torch.cuda.is_available(), "tools/knn_loop.py measures on the GPU: none is visible"
    map_pts, queries = workload()
    n = int(queries.shape[0])
    ctx = IcpContext(height=64, width=2048)
    ctx.map_set(map_pts)
    q_dev = torch.from_numpy(queries).cuda()
    sync = torch.cuda.synchronize

    gpu_legs = {f"knn_k{k}": (lambda k=k: ctx.knn_query(q_dev, k=k)) for k in args.ks}
    gpu_legs["nn_search"] = lambda: ctx.nearest_neighbor_search(q_dev, with_normals=False, with_index=True)
    if args.profile_pass:
        for _ in range(3):
            for call in gpu_legs.values():
                call()
        sync()
        return

    tree = cKDTree(map_pts.astype(np.float64))
    q64 = queries.astype(np.float64)
    shares = check_against_ckdtree(ctx, tree, map_pts, q_dev, queries, args.ks)
    legs = dict(gpu_legs)
    for k in args.ks:
        legs[f"ckdtree_k{k}"] = lambda k=k: tree.query(q64, k=k, workers=CPU_THREADS)
    for call in legs.values():  # every shape warmed
        call()
    sync()
    passes = {name: [] for name in legs}
    for _ in range(args.ab):
        for name, call in legs.items():
            passes[name].append(timed(call, sync, n, args.min_window))
    line = {"tool": "tools/knn_loop.py", "map_points": int(map_pts.shape[0]), "queries": n, "ab": args.ab,
            "min_window_s": args.min_window, "unit": "queries/s", "device": torch.cuda.get_device_name(0),
            "checked_against_ckdtree": True, "ambiguous_share": {str(k): shares[k] for k in args.ks}, "legs": {}}
    for name, v in passes.items():
        line["legs"][name] = {"where": f"CPU, {CPU_THREADS} threads" if name.startswith("ckdtree") else "GPU",
                              "passes": [round(x, 1) for x in v], "median": round(statistics.median(v), 1),
                              "min": round(min(v), 1), "max": round(max(v), 1)}
    text = json.dumps(line)
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
