"""dev: where the HOST spends a frame of the published-configuration loop (bench.py::odometry_loop_leg with timers around every call)

usage: python tools/host_profile.py                      the single plugin
       python tools/host_profile.py --batch 8 [--preprocessing members|batched] [--timestamps]
                                                         one step of MI355XICPFrameToModelBatch, call by call"""
import argparse, os, sys, time, collections
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "pylidar-slam_amd")]
import numpy as np, torch
from pylidar_slam_amd.odometry import (ConstantVelocityInitialization, Distortion, DistortionConfig, GridSample, GridSampleConfig,
                                       MI355XICPConfig, MI355XICPFrameToModel, SphericalProjector, ToDevice, ToDeviceConfig, ToTensor, ToTensorConfig)
from pylidar_slam_amd.synthetic import SceneConfig, make_sequence
from pylidar_slam_amd import engine as E
ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=0)
ap.add_argument("--preprocessing", choices=["members", "batched"], default="members")
ap.add_argument("--timestamps", action="store_true")
args = ap.parse_args()
dev = torch.device("cuda", 0)
frames = 36
if args.batch:
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import batched_loop as BL
    from pylidar_slam_amd import odometry as our
    B = args.batch
    seqs = [make_sequence(SceneConfig(height=64, width=2048, seed=1234 + 1000 * k, step=0.3 + 0.05 * (k % 5)), frames)
            for k in range(B)]
    acc = collections.defaultdict(float); cnt = collections.Counter()
    def timed(obj, name, label):
        f = getattr(obj, name)
        def w(*a, **k):
            t = time.perf_counter(); r = f(*a, **k); acc[label] += time.perf_counter() - t; cnt[label] += 1; return r
        setattr(obj, name, w)
    # every call of a step, by class (the wrappers sit on the classes: the loop builds its objects per pass)
    for n in ("preprocess", "project_rows", "stage", "register_launch", "register_end", "map_update_staged", "use_torch_stream"):
        timed(E.IcpBatch, n, "IcpBatch." + n)
    for cls in (our.ToDevice, our.Distortion, our.GridSample, our.ToTensor):
        timed(cls, "filter", f"filter:{cls.__name__}")
    timed(our.MI355XPreprocessingBatch, "forward", "MI355XPreprocessingBatch.forward")
    for n in ("_read_input", "_rows_to_host", "sample_points", "_rows_event"):
        timed(our.MI355XICPFrameToModel, n, "member." + n)
    timed(our.MI355XICPFrameToModelBatch, "_process", "process_next_frames (odometry total)")
    BL.run_batched(seqs[:1], dev, args.preprocessing, args.timestamps)
    acc.clear(); cnt.clear()
    el, _ = BL.run_batched(seqs, dev, args.preprocessing, args.timestamps)
    print(f"B = {B}, preprocessing {args.preprocessing}, timestamps {args.timestamps}: step {el / frames * 1e6:.1f} us "
          f"(with the timers; {frames} steps)")
    for k, v in sorted(acc.items(), key=lambda kv: -kv[1]): print(f"  {k:45s} {v / frames * 1e6:8.1f} us/step  ({cnt[k]} calls)")
    sys.exit(0)
scans, _ = make_sequence(SceneConfig(height=64, width=2048), frames)
cfg = MI355XICPConfig(max_num_alignments=20, threshold_delta_pose=1.0e-4, data_key="input_data",
                      local_map=dict(type="kdtree_local_map", local_map_size=30, num_neighbors_normals=10),
                      alignment=dict(mode="point_to_plane_gauss_newton", gauss_newton_config=dict(max_iters=1, scheme="neighborhood", sigma=0.2)))
odo = MI355XICPFrameToModel(cfg, projector=SphericalProjector(64, 2048), device=dev)
filters = [ToDevice(ToDeviceConfig(device=str(dev)), device=dev),
           Distortion(DistortionConfig(pointcloud_key="pc_device", timestamps_key="timestamps_device", output_key="distorted")),
           GridSample(GridSampleConfig(voxel_size=0.4, pointcloud_key="distorted", padded=True)),
           ToTensor(ToTensorConfig(device=str(dev), keys={"sample_points": "input_data"}, dtype="float32"), device=dev)]
init = ConstantVelocityInitialization()
acc = collections.defaultdict(float); cnt = collections.Counter()
def timed(obj, name, label):
    f = getattr(obj, name)
    def w(*a, **k):
        t = time.perf_counter(); r = f(*a, **k); acc[label] += time.perf_counter() - t; cnt[label] += 1; return r
    setattr(obj, name, w)
ctx = odo.ctx
for n in ("register_launch", "register_end", "map_update_staged", "map_update", "stage_insert", "project", "project_rows", "grid_sample_padded", "use_torch_stream", "distort"):
    if hasattr(ctx, n): timed(ctx, n, "ctx." + n)
for i, f in enumerate(filters): timed(f, "filter", f"filter{i}:{type(f).__name__}")
timed(odo, "_read_input", "odo._read_input"); timed(odo, "_rows_to_host", "odo._rows_to_host")
timed(odo.local_map, "update", "local_map.update"); timed(odo.local_map, "stage", "local_map.stage")
def one_pass(record):
    odo.init(); init.init()
    if record: acc.clear(); cnt.clear()
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for f in range(frames):
        d = {"numpy_pc": scans[f]}
        init.next_frame(d)
        for flt in filters: flt.filter(d)
        t = time.perf_counter(); odo.process_next_frame(d); acc["process_next_frame (total)"] += time.perf_counter() - t
        if odo.relative_pose_key() in d: init.save_real_motion(d[odo.relative_pose_key()], d)
    torch.cuda.synchronize()
    return time.perf_counter() - t0
one_pass(False)
el = one_pass(True)
print(f"frame {el/ (frames-1)*1e6:.1f} us (with the timers)")
for k, v in sorted(acc.items(), key=lambda kv: -kv[1]): print(f"  {k:40s} {v/(frames-1)*1e6:8.1f} us/frame  ({cnt[k]} calls)")
