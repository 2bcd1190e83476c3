"""The drives of the one-call frame tests (tests/test_frame_host.py on the CPU, tests/test_gpu_frame.py on the MI355X):
scans, settings and key-frame thresholds, defined ONCE so that the CPU file can check on the numpy oracle what the GPU file
relies on — that no frame of a drive sits near a key-frame threshold.  TEST INFRASTRUCTURE, never imported by the package.

The synthetic drive moves 0.4 m and 0.57 degrees per frame.  With threshold_trans = 0.7 m and threshold_rot = 10 degrees
the motion since the last key frame alternates between 0.4 m (pose-only update) and 0.8 m (key frame): both kinds of
update occur, each about 40 % away from the threshold.

`python tests/frame_cases.py` re-records tests/golden/frame_keyframe.npz (the numpy / from_pose_matrix values of the
key-frame arithmetic on the poses of the `sampled` drive, which the stand-alone C++ check is held to)."""
import os
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

THRESHOLD_TRANS = 0.7   # metres
THRESHOLD_ROT = 10.0    # degrees
GOLDEN_KEYFRAME = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frame_keyframe.npz")


@dataclass
class Drive:
    name: str
    height: int
    width: int
    frames: int
    voxel_size: float            # 0: the rows as given
    targets: int                 # 0: rows (numpy frames), 1: pixels of the vertex map (tensor frames)
    max_num_alignments: int
    threshold_delta_pose: float
    timestamps: bool = False
    cost: str = "point_to_plane_gauss_newton"
    local_map_size: int = 3      # evictions within the drive
    scans: list = field(default_factory=list, repr=False)
    stamps: Optional[list] = field(default=None, repr=False)


_SCANS = {}


def _scans(height, width, frames):
    from pylidar_slam_amd.synthetic import SceneConfig, make_sequence
    key = (height, width)
    if key not in _SCANS or len(_SCANS[key]) < frames:
        _SCANS[key] = make_sequence(SceneConfig(height=height, width=width), frames)[0]
    return _SCANS[key][:frames]


def _timestamps(height, width, frame):
    """Per-point acquisition times of a spinning sensor: the azimuth column sets the time within the 0.1 s sweep."""
    sweep = np.tile(np.linspace(0.0, 0.1, width, endpoint=False), height)
    return (0.1 * frame + sweep).astype(np.float64)


def drive(name: str) -> Drive:
    kinds = {
        # GPU tests 1 and 6: grid sample 0.4 m, 8 forced iterations, targets = pixels
        "sampled": dict(height=32, width=1024, frames=10, voxel_size=0.4, targets=1, max_num_alignments=8,
                        threshold_delta_pose=0.0),
        # GPU test 2: the same with a live stop (chunked launches)
        "sampled_live": dict(height=32, width=1024, frames=10, voxel_size=0.4, targets=1, max_num_alignments=15,
                             threshold_delta_pose=1.0e-4),
        # GPU test 3: raw rows from host arrays, both costs
        "raw": dict(height=16, width=512, frames=6, voxel_size=0.0, targets=0, max_num_alignments=8,
                    threshold_delta_pose=0.0),
        "raw_p2p": dict(height=16, width=512, frames=6, voxel_size=0.0, targets=0, max_num_alignments=8,
                        threshold_delta_pose=0.0, cost="point_to_point_gauss_newton"),
        # GPU test 4: de-skew in front of the grid sample
        "deskew": dict(height=32, width=1024, frames=5, voxel_size=0.4, targets=1, max_num_alignments=8,
                       threshold_delta_pose=0.0, timestamps=True),
    }
    d = Drive(name=name, **kinds[name])
    d.scans = _scans(d.height, d.width, d.frames)
    if d.timestamps:
        d.stamps = [_timestamps(d.height, d.width, f) for f in range(d.frames)]
    return d


def plugin_config(d: Drive, **over):
    from pylidar_slam_amd.odometry import MI355XICPConfig
    kw = dict(max_num_alignments=d.max_num_alignments, threshold_delta_pose=d.threshold_delta_pose,
              threshold_trans=THRESHOLD_TRANS, threshold_rot=THRESHOLD_ROT,
              data_key="numpy_pc" if d.targets == 0 else "input_data",
              local_map=dict(type="kdtree_local_map", local_map_size=d.local_map_size, num_neighbors_normals=10),
              alignment=dict(mode=d.cost, gauss_newton_config=dict(max_iters=1)))
    kw.update(over)
    return MI355XICPConfig(**kw)


def key_frame_margins(rel_poses, threshold_trans=THRESHOLD_TRANS, threshold_rot=THRESHOLD_ROT):
    """`__update_map` (slam/odometry/icp_odometry.py:360-380) replayed with numpy on the relative poses of a run: per
    frame behind frame 0 (delta before, new delta, parameters, |t|, |r| in degrees, key frame?)."""
    from pylidar_slam_amd.odometry import from_pose_matrix
    delta = np.eye(4, dtype=np.float32)
    out = []
    for pose in rel_poses[1:]:
        pose = np.asarray(pose, np.float32).reshape(4, 4)
        new_delta = (delta @ pose).astype(np.float32)
        dp = from_pose_matrix(new_delta)
        trans = float(np.linalg.norm(dp[:3]))
        rot = float(np.linalg.norm(dp[3:])) * 180.0 / np.pi
        key = trans > threshold_trans or rot > threshold_rot
        out.append((delta.copy(), new_delta, dp, trans, rot, bool(key)))
        delta = np.eye(4, dtype=np.float32) if key else new_delta
    return out


def run_plugin_on_oracle(d: Drive):
    """The drive through `MI355XICPFrameToModel` with the numpy oracle standing in for the HIP context (the caller has
    monkeypatched `odometry.IcpContext`): the frame dicts and the plugin."""
    import torch
    import icp_oracle as O
    from pylidar_slam_amd import odometry as our
    odo = our.MI355XICPFrameToModel(plugin_config(d, device="cpu"), projector=our.SphericalProjector(d.height, d.width),
                                    device=torch.device("cpu"))
    init = our.ConstantVelocityInitialization()
    odo.init()
    init.init()
    dicts = []
    for f, scan in enumerate(d.scans):
        pts = scan
        if d.timestamps:
            pts = O.distort(scan, d.stamps[f], np.asarray(init.next_initial_pose(), np.float64))
        if d.voxel_size > 0:
            pts = O.grid_sample(pts, d.voxel_size)[0]
        pts = np.ascontiguousarray(pts, dtype=np.float32)
        data = {(("numpy_pc") if d.targets == 0 else "input_data"): pts if d.targets == 0 else torch.from_numpy(pts)}
        init.next_frame(data)
        odo.process_next_frame(data)
        if f > 0:
            init.save_real_motion(data["odometry_pose"], data)
        dicts.append(data)
    return dicts, odo


def record_keyframe_fixture(path=GOLDEN_KEYFRAME):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (os.path.join(root, "pylidar-slam_amd"), os.path.join(root, "oracle"), os.path.dirname(os.path.abspath(__file__))):
        if p not in sys.path:
            sys.path.insert(0, p)
    from oracle_context import OracleContext
    from pylidar_slam_amd import odometry as our
    our.IcpContext = OracleContext
    _, odo = run_plugin_on_oracle(drive("sampled"))
    rel = odo.get_relative_poses().astype(np.float32)
    rows = key_frame_margins(rel)
    np.savez(path, rel=rel, threshold_trans=np.float32(THRESHOLD_TRANS), threshold_rot=np.float32(THRESHOLD_ROT),
             delta=np.stack([r[0] for r in rows]), new_delta=np.stack([r[1] for r in rows]),
             params=np.stack([r[2] for r in rows]).astype(np.float32), trans=np.array([r[3] for r in rows]),
             rot_deg=np.array([r[4] for r in rows]), key_frame=np.array([r[5] for r in rows]))
    return path


if __name__ == "__main__":
    print("recorded", record_keyframe_fixture())
