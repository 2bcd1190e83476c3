"""The drives of the batched frame tests (tests/test_batch_frame_host.py on the CPU, tests/test_gpu_batch_frame.py on the
MI355X): three synthetic drives that differ in scene seed and speed, defined ONCE so that the CPU file can check on the
numpy oracle what the GPU file relies on.  TEST INFRASTRUCTURE, never imported by the package.

With threshold_trans = 0.7 m and threshold_rot = 10 degrees (tests/frame_cases.py) the members that move 0.4 m per frame
take a key frame at frames 2, 4, 6, 8, the member that moves 0.3 m per frame at frames 3, 6, 9: step 6 has every member
insert, the other steps mix insertions with pose-only updates.  The motion since the last key frame is 0.4 / 0.8 m or
0.3 / 0.6 / 0.9 m: at least 14 % away from 0.7 m (0.6 m), and the rotation never comes near 10 degrees."""
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

import frame_cases as FC

MEMBERS = ((1234, 0.4), (2234, 0.3), (3234, 0.4))  # (scene seed, metres per frame)
KEY_FRAMES = ([2, 4, 6, 8], [3, 6, 9], [2, 4, 6, 8])
FRAMES = 10


@dataclass
class BatchDrive:
    name: str
    height: int
    width: int
    frames: int
    voxel_size: float
    targets: int
    max_num_alignments: int
    threshold_delta_pose: float
    members: int = 3
    stamped: tuple = ()          # members whose frames carry timestamps
    local_map_size: int = 3      # evictions within the drive
    scans: list = field(default_factory=list, repr=False)    # [member][frame]
    stamps: Optional[list] = field(default=None, repr=False)  # [member][frame] or None


_SCANS = {}


def member_scans(member: int, height: int, width: int, frames: int):
    from pylidar_slam_amd.synthetic import SceneConfig, make_sequence
    seed, step = MEMBERS[member]
    key = (seed, step, height, width)
    if key not in _SCANS or len(_SCANS[key]) < frames:
        _SCANS[key] = make_sequence(SceneConfig(height=height, width=width, seed=seed, step=step), frames)[0]
    return _SCANS[key][:frames]


def drive(name: str, members: Optional[int] = None) -> BatchDrive:
    kinds = {
        # GPU tests 1, 5, 6, 8: grid sample 0.4 m, 8 forced iterations, targets = pixels
        "sampled": dict(height=32, width=1024, frames=FRAMES, voxel_size=0.4, targets=1, max_num_alignments=8,
                        threshold_delta_pose=0.0),
        # GPU test 2: the same with a live stop (chunked launches)
        "sampled_live": dict(height=32, width=1024, frames=FRAMES, voxel_size=0.4, targets=1, max_num_alignments=15,
                             threshold_delta_pose=1.0e-4),
        # GPU test 3: raw rows from host arrays
        "raw": dict(height=16, width=512, frames=6, voxel_size=0.0, targets=0, max_num_alignments=8,
                    threshold_delta_pose=0.0, members=2),
        # GPU test 8: the same rows, long enough for a proper step behind every group of refusals
        "raw_long": dict(height=16, width=512, frames=10, voxel_size=0.0, targets=0, max_num_alignments=8,
                         threshold_delta_pose=0.0),
        # GPU test 4: timestamps on members 0 and 2 only
        "deskew": dict(height=32, width=1024, frames=5, voxel_size=0.4, targets=1, max_num_alignments=8,
                       threshold_delta_pose=0.0, stamped=(0, 2)),
    }
    d = BatchDrive(name=name, **kinds[name])
    if members is not None:
        d.members = members
    d.scans = [member_scans(b, d.height, d.width, d.frames) for b in range(d.members)]
    if d.stamped:
        d.stamps = [[FC._timestamps(d.height, d.width, f) for f in range(d.frames)] if b in d.stamped else None
                    for b in range(d.members)]
    return d


def single_drive(d: BatchDrive, member: int) -> FC.Drive:
    """Member `member` of a batched drive as a drive of tests/frame_cases.py (the plugin on the oracle runs those)."""
    s = FC.Drive(name=f"{d.name}[{member}]", height=d.height, width=d.width, frames=d.frames, voxel_size=d.voxel_size,
                 targets=d.targets, max_num_alignments=d.max_num_alignments, threshold_delta_pose=d.threshold_delta_pose,
                 timestamps=bool(d.stamps and d.stamps[member] is not None), local_map_size=d.local_map_size)
    s.scans = d.scans[member]
    s.stamps = d.stamps[member] if d.stamps else None
    return s
