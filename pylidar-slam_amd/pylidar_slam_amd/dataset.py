"""Dataset side of the hot path: the `DatasetLoader` plugin surface, a synthetic-scan loader for
BASELINE.json's synthetic configurations, the KITTI odometry reader with the scan correction and the spherical
projection done on the MI355X, and the KITTI-360 reader of RAW (un-rectified) scans: correction and azimuth time stamps
from one upload, so that `Distortion` has something to de-skew by.

  reference                                                             here
  DatasetLoader            slam/dataset/configuration.py:31-119         DatasetLoader
  KITTIOdometrySequence    slam/dataset/kitti_dataset.py:93-279         KITTIOdometrySequence (correct_scan + projection on GPU)
  KITTIDatasetLoader       slam/dataset/kitti_dataset.py:311-400        KITTIDatasetLoader
  read_ground_truth_file / read_calib_file   kitti_dataset.py:40-91     same names
  (none: the reference ships no synthetic data)                         SyntheticSequence / SyntheticDatasetLoader
  get_sequence_poses       slam/dataset/kitti_360_dataset.py:61-96      kitti360_sequence_poses (numpy + scipy, no pandas)
  KITTI360Sequence         slam/dataset/kitti_360_dataset.py:99-185     KITTI360Sequence (one `kitti360_prepare` per item)
  KITTI360DatasetLoader    slam/dataset/kitti_360_dataset.py:214-277    KITTI360DatasetLoader

Items are the reference's data_dict: `numpy_pc` [N,3] float32 (host), `vertex_map` [3,H,W] float32 (device tensor),
`absolute_pose_gt` [4,4].  The GPU context lives in the main process: use these datasets with num_workers = 0.
"""
from abc import ABC, abstractmethod
from dataclasses import dataclass, field
from pathlib import Path
from typing import List, Optional

import numpy as np
import torch
from torch.utils.data import Dataset

from . import eval as _eval
from .engine import IcpContext
from .odometry import SphericalProjector, assert_debug
from .synthetic import SceneConfig, ray_directions, render_scan, trajectory

__all__ = ["DatasetLoader", "SyntheticDatasetConfig", "SyntheticSequence", "SyntheticDatasetLoader", "KITTIConfig",
           "KITTIOdometrySequence", "KITTIDatasetLoader", "read_ground_truth_file", "read_calib_file",
           "kitti_read_scan", "compute_relative_poses", "KITTI360Config", "KITTI360Sequence", "KITTI360DatasetLoader",
           "kitti360_sequence_poses", "kitti360_drive_foldername", "KITTI360_DRIVES"]


def compute_relative_poses(absolute: np.ndarray) -> np.ndarray:
    """relative[0] = I, relative[i] = inv(abs[i-1]) @ abs[i] (trajectory expressed from its first frame; the
    reference's `eval_odometry.compute_relative_poses` keeps abs[0] as the first entry — see `eval.py`)."""
    rel = np.zeros_like(absolute)
    rel[0] = np.eye(4)
    for i in range(1, absolute.shape[0]):
        rel[i] = np.linalg.inv(absolute[i - 1]) @ absolute[i]
    return rel


class DatasetLoader(ABC):
    """slam/dataset/configuration.py:31-119 (the part the odometry runner uses)."""

    @classmethod
    def max_num_workers(cls):
        return 0  # the GPU context is not shared with DataLoader worker processes

    @staticmethod
    def absolute_gt_key():
        return "absolute_pose_gt"

    @staticmethod
    def numpy_pc_key():
        return "numpy_pc"

    def __init__(self, config):
        self.config = config

    @abstractmethod
    def projector(self) -> SphericalProjector:
        raise NotImplementedError("")

    @abstractmethod
    def sequences(self):
        """((train datasets, names), (eval ...), (test ...), transform)"""
        raise NotImplementedError("")

    @abstractmethod
    def get_ground_truth(self, sequence_name):
        return None


# ----------------------------------------------------------------------------------------------------------------------
@dataclass
class SyntheticDatasetConfig:
    dataset: str = "synthetic"
    lidar_height: int = 64
    lidar_width: int = 1024
    up_fov: float = 3.0
    down_fov: float = -24.0
    num_frames: int = 10
    seed: int = 1234
    train_sequences: List[str] = field(default_factory=lambda: ["room_00"])
    lidar_key: str = "vertex_map"
    with_numpy_pc: bool = True
    device: str = "cuda:0"  # the GPU the scans are projected on
    # False (default): items are CPU tensors, so the reference runner's DataLoader(pin_memory=True) works unchanged
    # (slam/odometry/odometry_runner.py:51,149) and `_send_to_device` moves them; True: the vertex map stays on the
    # device (no D2H + H2D round trip) — needs `pin_memory=false`, a CUDA tensor cannot be pinned
    device_items: bool = False


def _device_index(device: str) -> int:
    d = torch.device(device)
    return 0 if d.index is None else int(d.index)


class SyntheticSequence(Dataset):
    def __init__(self, config: SyntheticDatasetConfig, ctx: IcpContext, name: str):
        self.config = config
        self.ctx = ctx
        offset = sum(ord(c) for c in name) % 97
        self.scene = SceneConfig(height=config.lidar_height, width=config.lidar_width, up_fov=config.up_fov,
                                 down_fov=config.down_fov, seed=config.seed + offset)
        self.dirs = ray_directions(self.scene)
        self.poses = trajectory(self.scene, config.num_frames)

    def __len__(self):
        return self.config.num_frames

    def __getitem__(self, idx) -> dict:
        assert_debug(0 <= idx < len(self))
        scan = render_scan(self.scene, self.poses[idx], idx, self.dirs)
        d = {}
        if self.config.with_numpy_pc:
            d["numpy_pc"] = scan
        vmap = self.ctx.project(torch.from_numpy(scan).to(self.ctx.device))
        d[self.config.lidar_key] = vmap if self.config.device_items else vmap.cpu()
        d[DatasetLoader.absolute_gt_key()] = torch.from_numpy(self.poses[idx])
        return d


class SyntheticDatasetLoader(DatasetLoader):
    def __init__(self, config: SyntheticDatasetConfig):
        super().__init__(config)
        self._ctx = IcpContext(height=config.lidar_height, width=config.lidar_width, up_fov=config.up_fov,
                               down_fov=config.down_fov, device=_device_index(config.device))
        self._sequences = {n: SyntheticSequence(config, self._ctx, n) for n in config.train_sequences}

    def projector(self) -> SphericalProjector:
        c = self.config
        return SphericalProjector(c.lidar_height, c.lidar_width, 3, c.up_fov, c.down_fov)

    def sequences(self):
        names = list(self._sequences)
        return ([self._sequences[n] for n in names], names), (None, None), (None, None), lambda x: x

    def get_ground_truth(self, sequence_name):
        if sequence_name not in self._sequences:
            return None
        return compute_relative_poses(self._sequences[sequence_name].poses)


# ----------------------------------------------------------------------------------------------------------------------
def kitti_read_scan(file_path: str) -> np.ndarray:
    """kitti_dataset.py:20-37: float32 records x, y, z, reflectance."""
    return np.fromfile(file_path, dtype=np.float32).reshape((-1, 4))


def read_calib_file(file_path: str) -> dict:
    """kitti_dataset.py:40-67."""
    calib = {}
    with open(file_path, "r") as f:
        for line in f.readlines():
            tokens = line.split(" ")
            if tokens[0] == "calib_time:" or len(tokens) < 2:
                continue
            calib[tokens[0][:-1]] = np.array([float(t) for t in tokens[1:]], dtype=np.float32)
    return calib


def read_ground_truth_file(file_path: str) -> np.ndarray:
    """kitti_dataset.py:70-91: [N,12] rows -> [N,4,4] (left-camera frame)."""
    poses = np.loadtxt(file_path, dtype=np.float64).reshape(-1, 12)
    n = poses.shape[0]
    poses = np.concatenate((poses, np.zeros((n, 3)), np.ones((n, 1))), axis=1)
    return poses.reshape((n, 4, 4))


@dataclass
class KITTIConfig:
    """kitti_dataset.py:283-302."""
    kitti_sequence_dir: str = ""
    dataset: str = "kitti"
    lidar_key: str = "vertex_map"
    absolute_gt_key: str = "absolute_pose_gt"
    lidar_height: int = 64
    lidar_width: int = 1024
    up_fov: float = 3.0
    down_fov: float = -24.0
    train_sequences: List[str] = field(default_factory=lambda: [f"{i:02}" for i in range(11)])
    eval_sequences: List[str] = field(default_factory=lambda: ["09", "10"])
    test_sequences: List[str] = field(default_factory=lambda: [f"{i:02}" for i in range(22)])
    with_numpy_pc: bool = True
    device: str = "cuda:0"       # the GPU scans are corrected and projected on
    device_items: bool = False   # see SyntheticDatasetConfig.device_items


class KITTIOdometrySequence(Dataset):
    """kitti_dataset.py:93-279 without the unrectified-raw branch: .bin read on the host, `correct_scan` and the
    spherical projection on the GPU (the reference burns DataLoader workers on both)."""

    def __init__(self, sequences_root_dir: str, sequence_id: str, ctx: IcpContext,
                 corrected_lidar_channel: str = "vertex_map", ground_truth_channel: Optional[str] = None,
                 with_numpy_pc: bool = False, device_items: bool = False):
        self._device_items = device_items
        self.sequence_dir = Path(sequences_root_dir)
        self.sequence_id = sequence_id
        self.ctx = ctx
        self.corrected_lidar_channel = corrected_lidar_channel
        self.ground_truth_channel = ground_truth_channel
        self._with_numpy_pc = with_numpy_pc
        self.velodyne_path = self.sequence_dir / "sequences" / sequence_id / "velodyne"
        assert_debug(self.velodyne_path.exists(), f"{self.velodyne_path} does not exist")
        self.size = len(sorted(self.velodyne_path.glob("*.bin")))
        calib_path = self.sequence_dir / "sequences" / sequence_id / "calib.txt"
        assert_debug(calib_path.exists() and calib_path.is_file())
        self.calibration_matrices = {}
        calib = read_calib_file(str(calib_path))
        if "Tr" in calib:
            self.calibration_matrices["Tr"] = np.concatenate(
                (calib["Tr"].reshape(3, 4), np.array([[0, 0, 0, 1]], dtype=np.float32)), axis=0)
        self.poses_gt = None
        if ground_truth_channel:
            gt_file = self.sequence_dir / "poses" / f"{sequence_id}.txt"
            if gt_file.exists() and gt_file.is_file():
                self.poses_gt = self._lidar_pose_gt(read_ground_truth_file(str(gt_file)))

    def _lidar_pose_gt(self, poses_gt: np.ndarray):  # :186-194
        if "Tr" in self.calibration_matrices:
            tr = self.calibration_matrices["Tr"].astype(np.float64)
            return np.einsum("...ij,...jk->...ik", np.einsum("...ij,...jk->...ik", np.linalg.inv(tr), poses_gt), tr)
        return poses_gt

    def __len__(self):
        return self.size

    def correct_scan(self, scan: np.ndarray) -> np.ndarray:
        """:202-231 on the GPU.  float32 out: the reference's numpy expression yields float32 under the numpy 1.x it
        was written for and float64 under numpy 2; the GPU kernel computes in float64 and this rounds once."""
        return self.ctx.kitti_correct_scan(scan).astype(np.float32)

    def __getitem__(self, idx) -> dict:
        assert_debug(idx < self.size)
        d = {}
        scan_path = self.velodyne_path / f"{idx:06}.bin"
        assert_debug(scan_path.exists() and scan_path.is_file(), f"The file {scan_path} does not exist")
        scan = self.correct_scan(kitti_read_scan(str(scan_path)))
        if self._with_numpy_pc:
            d["numpy_pc"] = scan
        vmap = self.ctx.project(torch.from_numpy(scan).to(self.ctx.device))
        d[self.corrected_lidar_channel] = vmap if self._device_items else vmap.cpu()
        if self.ground_truth_channel and self.poses_gt is not None:
            d[self.ground_truth_channel] = torch.from_numpy(self.poses_gt[idx])
        return d


class KITTIDatasetLoader(DatasetLoader):
    """kitti_dataset.py:311-400."""

    def __init__(self, config: KITTIConfig):
        super().__init__(config)
        self.odometry_sequence_dir = Path(config.kitti_sequence_dir)
        assert_debug(self.odometry_sequence_dir.exists())
        self._ctx = IcpContext(height=config.lidar_height, width=config.lidar_width, up_fov=config.up_fov,
                               down_fov=config.down_fov, device=_device_index(config.device))

    def projector(self) -> SphericalProjector:
        c = self.config
        return SphericalProjector(c.lidar_height, c.lidar_width, 3, c.up_fov, c.down_fov)

    def get_ground_truth(self, sequence_name):  # :333-347
        gt = self.odometry_sequence_dir / "poses" / f"{sequence_name}.txt"
        if not gt.exists():
            return None
        poses = read_ground_truth_file(str(gt)).astype(np.float64)
        calib = read_calib_file(str(self.odometry_sequence_dir / "sequences" / sequence_name / "calib.txt"))
        tr = np.eye(4, dtype=np.float64)
        tr[:3, :4] = calib["Tr"].reshape(3, 4)
        right = np.einsum("...ij,...jk->...ik", np.einsum("...ij,...jk->...ik", np.linalg.inv(tr), poses), tr)
        return _eval.compute_relative_poses(right)  # the reference's own convention: rel[0] = abs[0]

    def sequences(self):  # :349-400
        c = self.config

        def get(seqs):
            if not seqs:
                return None
            present = [s for s in seqs if (self.odometry_sequence_dir / "sequences" / s / "velodyne").exists()]
            return [KITTIOdometrySequence(str(self.odometry_sequence_dir), s, self._ctx, c.lidar_key, c.absolute_gt_key,
                                          with_numpy_pc=c.with_numpy_pc, device_items=c.device_items)
                    for s in present], present

        tr, ev, te = get(c.train_sequences), get(c.eval_sequences), get(c.test_sequences)
        return tr or (None, None), ev or (None, None), te or (None, None), lambda x: x


# ----------------------------------------------------------------------------------------------------------------------
# KITTI-360 (http://www.cvlibs.net/datasets/kitti-360/): raw HDL-64 scans, not motion-compensated — the one dataset of the
# reference that reaches its `Distortion` filter, through azimuth time stamps (slam/dataset/kitti_360_dataset.py:170-185)
KITTI360_DRIVES = {0: 11518, 2: 19240, 3: 1031, 4: 11587, 5: 6743, 6: 9699, 7: 3396, 9: 14056, 10: 3836}  # drive id: frames

# calib_cam_to_pose.txt (image_00) and calib_cam_to_velo.txt of the dataset's calibration folder
_KITTI360_CAM0_TO_POSE = np.array([[0.0371783278, -0.0986182135, 0.9944306009, 1.5752681039],
                                   [0.9992675562, -0.0053553387, -0.0378902567, 0.0043914093],
                                   [0.0090621821, 0.9951109327, 0.0983468786, -0.6500000000],
                                   [0.0, 0.0, 0.0, 1.0]], dtype=np.float64)
_KITTI360_CAM0_TO_VELO = np.array([[0.04307104361, -0.08829286498, 0.995162929, 0.8043914418],
                                   [-0.999004371, 0.007784614041, 0.04392796942, 0.2993489574],
                                   [-0.01162548558, -0.9960641394, -0.08786966659, -0.1770225824],
                                   [0.0, 0.0, 0.0, 1.0]], dtype=np.float64)


def kitti360_drive_foldername(drive_id: int) -> str:
    return f"2013_05_28_drive_{int(drive_id):04}_sync"


def _kitti360_velodyne_path(root_dir, drive_id: int) -> Path:
    return Path(root_dir) / "data_3d_raw" / kitti360_drive_foldername(drive_id) / "velodyne_points"


def kitti360_sequence_poses(root_dir, drive_id: int) -> Optional[np.ndarray]:
    """`get_sequence_poses` (kitti_360_dataset.py:61-96) on the host, without pandas: one lidar pose [F,4,4] float64 per
    frame, or None without a `data_poses/<drive>/poses.txt`.  The ground truth holds fewer poses than frames (rows `frame
    index, 12 pose entries`): rotations are interpolated by scipy's Slerp and translations linearly at the frame instants
    of `timestamps.txt` (nanoseconds; clipped to the first / last key instant), then taken to the lidar frame."""
    from scipy.interpolate import interp1d
    from scipy.spatial.transform import Rotation, Slerp

    assert_debug(int(drive_id) in KITTI360_DRIVES, f"KITTI-360 has no drive {drive_id}")
    gt_file = Path(root_dir) / "data_poses" / kitti360_drive_foldername(drive_id) / "poses.txt"
    if not gt_file.exists():
        return None
    rows = np.loadtxt(str(gt_file), dtype=np.float64, ndmin=2)  # [K, 13]
    key_frames = rows[:, 0].astype(np.int32)
    k = rows.shape[0]
    key_poses = np.concatenate((rows[:, 1:], np.zeros((k, 3)), np.ones((k, 1))), axis=1).reshape(k, 4, 4)
    with open(_kitti360_velodyne_path(root_dir, drive_id) / "timestamps.txt", "r") as f:
        stamps = [line.strip() for line in f if line.strip()]
    instants = np.array(stamps, dtype="datetime64[ns]").astype(np.int64).astype(np.float64)
    key_instants = instants[key_frames]
    instants = instants.clip(min=key_instants.min(), max=key_instants.max())
    poses = np.zeros((instants.shape[0], 4, 4), dtype=np.float64)
    poses[:, :3, :3] = Slerp(key_instants, Rotation.from_matrix(key_poses[:, :3, :3]))(instants).as_matrix()
    poses[:, :3, 3] = interp1d(key_instants, key_poses[:, :3, 3], axis=0)(instants)
    poses[:, 3, 3] = 1.0
    velo_to_pose = _KITTI360_CAM0_TO_POSE.dot(np.linalg.inv(_KITTI360_CAM0_TO_VELO))
    return np.einsum("nij,jk->nik", poses, velo_to_pose)


def _kitti360_from_first(poses: np.ndarray) -> np.ndarray:
    return np.einsum("ij,njk->nik", np.linalg.inv(poses[0]), poses)  # :133, :240


@dataclass
class KITTI360Config:
    """kitti_360_dataset.py:189-205."""
    root_dir: str = ""
    dataset: str = "kitti_360"
    lidar_height: int = 64
    lidar_width: int = 1024
    up_fov: float = 3.0
    down_fov: float = -24.0
    train_sequences: List[int] = field(default_factory=lambda: [0, 2, 3, 4, 5, 6, 7, 9, 10])
    test_sequences: List[int] = field(default_factory=lambda: [0, 2, 3, 4, 5, 6, 7])
    eval_sequences: List[int] = field(default_factory=lambda: [9, 10])
    device: str = "cuda:0"       # the GPU scans are corrected and timed on
    # False: `numpy_pc` / `numpy_pc_timestamps` are host arrays, as in the reference; True: both stay cuda tensors, so
    # `distortion_mi355x` -> `grid_sample_mi355x` -> the frame calls run without a round trip (see SyntheticDatasetConfig)
    device_items: bool = False


class KITTI360Sequence(Dataset):
    """kitti_360_dataset.py:99-185: the raw .bin is read on the host, then ONE `IcpContext.kitti360_prepare` corrects the
    scan and estimates its time stamps (clockwise, phi_0 = pi) — nothing is computed per point on the host.  `ctx`: an
    IcpContext, or a callable returning one (created when the first item is read)."""

    def __init__(self, kitti360_root_dir: str, drive_id: int, ctx, device_items: bool = False):
        self.root_dir = Path(kitti360_root_dir)
        self.drive_id = int(drive_id)
        assert_debug(self.drive_id in KITTI360_DRIVES, f"KITTI-360 has no drive {drive_id}")
        self.lidar_path = _kitti360_velodyne_path(self.root_dir, self.drive_id) / "data"
        assert_debug(self.lidar_path.exists(), f"The drive directory {self.lidar_path} does not exist")
        self.size = KITTI360_DRIVES[self.drive_id]
        self._ctx = ctx
        self._device_items = device_items
        self.gt_poses = kitti360_sequence_poses(self.root_dir, self.drive_id)
        if self.gt_poses is not None:
            self.gt_poses = _kitti360_from_first(self.gt_poses)

    @property
    def ctx(self) -> IcpContext:
        if not isinstance(self._ctx, IcpContext):
            self._ctx = self._ctx()
        return self._ctx

    def __len__(self):
        return self.size

    def __getitem__(self, idx) -> dict:
        assert_debug(0 <= idx < self.size)
        scan_path = self.lidar_path / f"{idx:010}.bin"
        assert_debug(scan_path.exists() and scan_path.is_file(), f"The file {scan_path} does not exist")
        scan = kitti_read_scan(str(scan_path))
        ctx = self.ctx
        d = {}
        if self._device_items:
            xyz, ts = ctx.kitti360_prepare(torch.from_numpy(scan).to(ctx.device))
            d["numpy_pc"] = xyz.to(torch.float32)  # rounded once, as KITTIOdometrySequence.correct_scan does
        else:
            xyz, ts = ctx.kitti360_prepare(scan)
            d["numpy_pc"] = xyz.astype(np.float32)
        d["numpy_reflectance"] = scan[:, 3:]
        d["numpy_pc_timestamps"] = ts
        if self.gt_poses is not None:
            d[DatasetLoader.absolute_gt_key()] = self.gt_poses[idx]
        return d


class KITTI360DatasetLoader(DatasetLoader):
    """kitti_360_dataset.py:214-277.  The GPU context is created with the first item read, so ground truth, projector and
    the sequence lists are available without a device."""

    def __init__(self, config: KITTI360Config):
        super().__init__(config)
        self.root_dir = Path(config.root_dir)
        assert_debug(self.root_dir.exists())
        self._context = None

    def _ctx(self) -> IcpContext:
        if self._context is None:
            c = self.config
            self._context = IcpContext(height=c.lidar_height, width=c.lidar_width, up_fov=c.up_fov, down_fov=c.down_fov,
                                       device=_device_index(c.device))
        return self._context

    def projector(self) -> SphericalProjector:
        c = self.config
        return SphericalProjector(c.lidar_height, c.lidar_width, 3, c.up_fov, c.down_fov)

    def get_ground_truth(self, drive_id):  # :236-241
        poses = kitti360_sequence_poses(self.root_dir, int(drive_id))
        if poses is None:
            return None
        return _eval.compute_relative_poses(_kitti360_from_first(poses))  # the reference's own convention: rel[0] = abs[0]

    def sequences(self):  # :243-277 (drives whose scans are absent are left out, as KITTIDatasetLoader does)
        c = self.config

        def get(drives):
            if not drives:
                return None
            present = [str(d) for d in drives if (_kitti360_velodyne_path(self.root_dir, int(d)) / "data").exists()]
            return [KITTI360Sequence(str(self.root_dir), int(d), self._ctx, c.device_items) for d in present], present

        tr, ev, te = get(c.train_sequences), get(c.eval_sequences), get(c.test_sequences)
        return tr or (None, None), ev or (None, None), te or (None, None), lambda x: x
