"""Host-side mirror of the reference's ICP odometry plugin surface, running on the MI355X through libicp_mi355x.so.

Same names, argument meaning and error behaviour as the reference classes they stand in for:

  reference (paths relative to the reference repo)                      here
  -------------------------------------------------------------------   -----------------------------------
  OdometryAlgorithm                slam/odometry/odometry.py:21-81      OdometryAlgorithm
  ICPFrameToModelConfig            slam/odometry/icp_odometry.py:29-64  MI355XICPConfig
  ICPFrameToModel                  slam/odometry/icp_odometry.py:72-381 MI355XICPFrameToModel
  KdTreeLocalMap                   slam/odometry/local_map.py:254-427   HashGridLocalMap
  ProjectiveLocalMap               slam/odometry/local_map.py:91-240    ProjectiveLocalMap
  GaussNewtonPointToPlaneAlignment slam/odometry/alignment.py:80-127    PointToPlaneAlignment
  SphericalProjector               slam/common/projection.py:426-508    SphericalProjector
  GridSample / grid_sample         slam/preprocessing.py:207-226        GridSample / grid_sample
  Distortion                       slam/preprocessing.py:144-191        Distortion
  ConstantVelocityInitialization   slam/initialization.py:103-119       ConstantVelocityInitialization

All array arithmetic over points happens in HIP kernels; this file only orchestrates (O(1) pose algebra per frame).
There is no CPU fallback: constructing any of these without the library / a GPU raises.
"""
import time
from abc import ABC, abstractmethod
from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional

import numpy as np
import torch

from .engine import IcpBatch, IcpContext, InvalidJacobianError, RegisterResult  # noqa: F401

__all__ = ["OdometryAlgorithm", "MI355XICPConfig", "MI355XICPFrameToModel", "HashGridLocalMap",
           "HashGridLocalMapConfig", "ProjectiveLocalMap", "ProjectiveLocalMapConfig", "PointToPlaneAlignment",
           "PointToPlaneAlignmentConfig", "PointToPointAlignment", "PointToPointAlignmentConfig", "SphericalProjector",
           "GridSample", "GridSampleConfig", "grid_sample", "Distortion", "DistortionConfig", "Voxelization",
           "VoxelizationConfig", "ToDevice", "ToDeviceConfig", "ConstantVelocityInitialization", "NeighborhoodResult",
           "MI355XICPFrameToModelBatch", "MI355XPreprocessingBatch",
           "build_pose_matrix", "from_pose_matrix"]


def assert_debug(condition: bool, message: str = ""):
    """reference slam/common/utils.py:30-38."""
    if not condition:
        raise AssertionError(message)


# ----------------------------------------------------------------------------------------------------------------------
# O(1) pose algebra on the host (euler xyz, R = Rz Ry Rx: slam/common/rotation.py:144-150,253-270; pose.py:120-207)
# ----------------------------------------------------------------------------------------------------------------------
def build_pose_matrix(params, dtype=np.float32) -> np.ndarray:
    p = np.asarray(params, dtype=dtype).reshape(6)
    cx, cy, cz = np.cos(p[3:])
    sx, sy, sz = np.sin(p[3:])
    t = np.eye(4, dtype=dtype)
    t[0, :3] = (cz * cy, cz * sy * sx - sz * cx, cz * sy * cx + sz * sx)
    t[1, :3] = (sz * cy, sz * sy * sx + cz * cx, sz * sy * cx - cz * sx)
    t[2, :3] = (-sy, cy * sx, cy * cx)
    t[:3, 3] = p[:3]
    return t


def from_pose_matrix(mat: np.ndarray, eps: float = 1.0e-6) -> np.ndarray:
    m = np.asarray(mat)
    sy = np.sqrt(m[0, 0] * m[0, 0] + m[1, 0] * m[1, 0])
    if not sy < eps:
        e = (np.arctan2(m[2, 1], m[2, 2]), np.arctan2(-m[2, 0], sy), np.arctan2(m[1, 0], m[0, 0]))
    else:
        e = (np.arctan2(-m[1, 2], m[1, 1]), np.arctan2(-m[2, 0], sy), 0.0)
    return np.array([m[0, 3], m[1, 3], m[2, 3], *e], dtype=m.dtype)


# ----------------------------------------------------------------------------------------------------------------------
class OdometryAlgorithm(ABC):
    """The plugin ABC of slam/odometry/odometry.py:21-81 (restated so the package is importable without the
    reference; `register.py` also registers the MI355X odometry in the reference's own ODOMETRY enum)."""

    def __init__(self, config, **kwargs):
        self.config = config
        self.elapsed: list = []

    @abstractmethod
    def init(self):
        self.elapsed = []

    def process_next_frame(self, data_dict: dict):
        beginning = time.time()
        self.do_process_next_frame(data_dict)
        self.elapsed.append(time.time() - beginning)

    @abstractmethod
    def do_process_next_frame(self, data_dict: dict):
        raise NotImplementedError("")

    def get_relative_poses(self) -> np.ndarray:
        raise NotImplementedError("")

    def get_elapsed(self) -> float:
        return sum(self.elapsed)

    @staticmethod
    def pointcloud_key() -> str:
        return "odometry_pc"

    @staticmethod
    def relative_pose_key() -> str:
        return "odometry_pose"


# ----------------------------------------------------------------------------------------------------------------------
@dataclass
class SphericalProjector:
    """Parameters of slam/common/projection.py:426-445; `build_projection_map` (:331-418) runs on the GPU."""
    height: int = 64
    width: int = 1024
    num_channels: int = 3
    up_fov: float = 3.0
    down_fov: float = -24.0
    _ctx: Optional[IcpContext] = field(default=None, repr=False, compare=False)

    def _context(self) -> IcpContext:
        if self._ctx is None:
            self._ctx = IcpContext(height=self.height, width=self.width, up_fov=self.up_fov, down_fov=self.down_fov)
        return self._ctx

    def build_projection_map(self, pointcloud, **kwargs):
        """[1, N, 3] (or [N, 3]) -> [1, 3, H, W]; torch cuda tensors stay on the device."""
        pts = pointcloud[0] if pointcloud.ndim == 3 else pointcloud
        vmap = self._context().project(pts)
        return vmap[None] if isinstance(vmap, np.ndarray) else vmap.unsqueeze(0)


# ----------------------------------------------------------------------------------------------------------------------
def grid_sample(pointcloud: np.ndarray, voxel_size: float, ctx: Optional[IcpContext] = None):
    """slam/common/pointcloud.py:182-195: (sample points, indices of the sampled points)."""
    ctx = ctx or _shared_context()
    if isinstance(pointcloud, np.ndarray) and pointcloud.dtype == np.float64:
        # e.g. the float64 output of `Distortion`: voxelised from the float64 values, like the reference
        return ctx.grid_sample_f64(pointcloud, voxel_size)
    pts, idx = ctx.grid_sample(pointcloud, voxel_size)
    if isinstance(pointcloud, np.ndarray) and pointcloud.dtype != np.float32:
        pts = pointcloud[idx]  # keep the caller's dtype, like `pointcloud[unique_indices]`
    return pts, idx


_SHARED: Dict[int, IcpContext] = {}


def _shared_context(device=None) -> IcpContext:
    """One utility context per GPU for the stateless filters (grid sampling, de-skew, voxel statistics)."""
    index = int(device.index) if device is not None and getattr(device, "index", None) is not None else 0
    if index not in _SHARED:
        _SHARED[index] = IcpContext(device=index)
    return _SHARED[index]


@dataclass
class VoxelizationConfig:
    """slam/preprocessing.py:43-59."""
    filter_name: str = "voxelization"
    input_channel: str = "numpy_pc"
    voxel_covariances_key: str = "voxel_covariances"
    voxel_means_key: str = "voxel_means"
    voxel_size_key: str = "voxel_sizes"
    voxel_indices_key: str = "voxel_indices"
    voxel_hashes_key: str = "voxel_hashes"
    voxel_coordinates_key: str = "voxel_coordinates"
    with_normal_distribution: bool = True
    voxel_size: float = 0.2


class Voxelization:
    """slam/preprocessing.py:63-98 (`Filter.filter(data_dict)` seam): voxel coordinates / hashes and the per-voxel
    point count, mean and covariance, computed on the GPU."""

    def __init__(self, config: VoxelizationConfig, ctx: Optional[IcpContext] = None, **kwargs):
        self.config = config
        self._ctx = ctx

    def filter(self, data_dict: dict):
        c = self.config
        assert_debug(c.input_channel in data_dict, f"The input channel {c.input_channel} was not in the input channel")
        pc = data_dict[c.input_channel]
        assert_debug(isinstance(pc, np.ndarray))
        assert_debug(pc.ndim == 2 and pc.shape[1] == 3, f"expected [N, 3], got {pc.shape}")
        out = (self._ctx or _shared_context()).voxel_statistics(pc, c.voxel_size, c.with_normal_distribution)
        data_dict[c.voxel_hashes_key] = out["voxel_hashes"]
        data_dict[c.voxel_coordinates_key] = out["voxel_coordinates"]
        if c.with_normal_distribution:
            data_dict[c.voxel_means_key] = out["voxel_means"]
            data_dict[c.voxel_covariances_key] = out["voxel_covariances"]
            data_dict[c.voxel_size_key] = out["voxel_sizes"]
            data_dict[c.voxel_indices_key] = out["voxel_indices"]


@dataclass
class GridSampleConfig:
    """slam/preprocessing.py:196-204."""
    filter_name: str = "grid_sample"
    voxel_size: float = 0.3
    pointcloud_key: str = "numpy_pc"
    output_indices_key: str = "sample_indices"
    output_sample_key: str = "sample_points"
    # MI355X-side: True = the device-resident pipeline's variant for cuda tensors — NO synchronisation: `sample_points` /
    # `sample_indices` keep the n rows of the input, the V samples first (same order), NaN rows / index -1 behind them, and
    # `sample_count` (a 0-dim int32 cuda tensor) holds V.  The MI355X odometry masks NaN rows, so a frame then synchronises
    # once, for its pose.  False (default): the reference's shapes — V rows, which costs the host a round trip for V
    padded: bool = False
    output_count_key: str = "sample_count"


def _is_device_tensor(a) -> bool:
    return isinstance(a, torch.Tensor) and a.is_cuda


class GridSample:
    """slam/preprocessing.py:207-226 (`Filter.filter(data_dict)` seam).  A numpy cloud gives numpy samples like the
    reference; a cuda tensor (float32, or the float64 output of `Distortion`) is sampled in place on the device and the
    samples / indices stay there — the device-resident hand-off towards the odometry."""

    def __init__(self, config: GridSampleConfig, ctx: Optional[IcpContext] = None, **kwargs):
        self.config = config
        self._ctx = ctx

    def filter(self, data_dict: dict):
        pc = data_dict[self.config.pointcloud_key]
        assert_debug(isinstance(pc, np.ndarray) or _is_device_tensor(pc), "Cannot Distort a non numpy frame")
        assert_debug(pc.ndim == 2 and pc.shape[1] == 3, f"expected [N, 3], got {pc.shape}")
        if _is_device_tensor(pc):
            ctx = self._ctx or _shared_context(pc.device)
            ctx.use_torch_stream()
            if bool(getattr(self.config, "padded", False)) and hasattr(ctx, "grid_sample_padded"):
                sample, indices, count = ctx.grid_sample_padded(pc, self.config.voxel_size)
                data_dict[getattr(self.config, "output_count_key", "sample_count")] = count
            else:
                sample, indices = ctx.grid_sample_f64(pc, self.config.voxel_size) if pc.dtype == torch.float64 else \
                    ctx.grid_sample(pc, self.config.voxel_size)
        else:
            sample, indices = grid_sample(pc, self.config.voxel_size, self._ctx)
        data_dict[self.config.output_sample_key] = sample
        data_dict[self.config.output_indices_key] = indices


@dataclass
class ToDeviceConfig:
    """Config of `ToDevice` (FILTER member `to_device_mi355x`)."""
    filter_name: str = "to_device_mi355x"
    device: str = "cuda:0"
    keys: Dict[str, str] = field(default_factory=lambda: {"numpy_pc": "pc_device",
                                                          "numpy_pc_timestamps": "timestamps_device"})
    # pageable arrays travel through a persistent pinned buffer on an upload stream of their own, into two alternating
    # device slots: the tensor a frame receives is overwritten TWO frames later — a consumer that keeps frames around
    # longer clones them, or sets this to False (torch's own blocking copy into a fresh tensor)
    pinned_staging: bool = True


class ToDevice:
    """Uploads the raw frame ONCE: every listed numpy array (or cpu tensor) present in the dict becomes a cuda tensor of
    the same dtype under the new key; the filters behind it (`Distortion`, `GridSample`) and the odometry then work on
    device memory only.  Keys that are absent are skipped (a dataset without timestamps has no `numpy_pc_timestamps`)."""

    def __init__(self, config: ToDeviceConfig, device=None, **kwargs):
        self.config = config
        dev = torch.device(device if device is not None and str(device) != "cpu" else config.device)
        self.device = dev if dev.type == "cuda" else torch.device(config.device)
        self._slots: Dict[str, Any] = {}
        self._stream = None

    def _upload(self, key: str, t: torch.Tensor) -> torch.Tensor:
        """Pageable host memory -> device the way the odometry uploads its frames (`MI355XICPFrameToModel._upload`): one host
        memcpy into a persistent pinned buffer, an asynchronous DMA on a stream of ITS OWN into one of two alternating
        device slots, the caller's stream made to wait for it — `tensor.to(device)` from pageable memory blocks the host
        for the whole transfer (165 us for a 131 072-point frame).  (The DMA enqueued on the caller's stream itself, behind
        the previous frame's map update, stalled later HIP calls of the frame for 2.4 ms each: measured in round 5.)"""
        if self.device.type != "cuda" or t.is_cuda or t.numel() == 0 or not getattr(self.config, "pinned_staging", True):
            return t.to(self.device, non_blocking=True)
        slot = self._slots.get(key)
        if slot is None or slot["pin"].numel() < t.numel() or slot["pin"].dtype != t.dtype:
            slot = self._slots[key] = {"pin": torch.empty(t.numel(), dtype=t.dtype, pin_memory=True), "free": None,
                                       "dev": [None, None], "which": 0, "used": [None, None]}
        if slot["free"] is not None:
            slot["free"].synchronize()  # the previous frame's DMA has left the staging buffer (long done in practice)
        stage = slot["pin"][:t.numel()].view(t.shape)
        # (numpy's memcpy: `stage.copy_(t)` goes through torch's intra-op thread pool for 1.5 MB — waking it cost 5 ms per
        # frame on the 256-thread host)
        stage.numpy()[...] = t.numpy()
        if self._stream is None:
            self._stream = torch.cuda.Stream(device=self.device)
        main = torch.cuda.current_stream(self.device)
        # the device slot handed out by the PREVIOUS call: whatever read it has been enqueued on the caller's stream by now —
        # an event there, which the DMA that overwrites that slot (the call after this one) waits for.  (the
        # upload stream never waited for the consumers; safe only behind the odometry's per-frame synchronisation.  The
        # wait is for work enqueued a whole frame ago, so the upload still overlaps the map update of the frame in between.)
        prev = slot["which"]
        if slot["dev"][prev] is not None:
            if slot["used"][prev] is None:
                slot["used"][prev] = torch.cuda.Event()
            slot["used"][prev].record(main)
        slot["which"] ^= 1
        dev = slot["dev"][slot["which"]]
        if dev is None or dev.numel() < t.numel() or dev.dtype != t.dtype:
            dev = slot["dev"][slot["which"]] = torch.empty(t.numel(), dtype=t.dtype, device=self.device)
        out = dev[:t.numel()].view(t.shape)
        with torch.cuda.stream(self._stream):
            if slot["used"][slot["which"]] is not None:
                self._stream.wait_event(slot["used"][slot["which"]])
            out.copy_(stage, non_blocking=True)
            slot["free"] = torch.cuda.Event()
            slot["free"].record(self._stream)
        main.wait_event(slot["free"])
        return out

    def filter(self, data_dict: dict):
        for old_key, new_key in dict(self.config.keys).items():
            if old_key not in data_dict:
                continue
            a = data_dict[old_key]
            t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
            assert_debug(isinstance(t, torch.Tensor), f"cannot upload `{old_key}` of type {type(a)}")
            data_dict[new_key] = self._upload(old_key, t)


@dataclass
class ToTensorConfig:
    """slam/preprocessing.py:101-107, plus an optional dtype for the renamed tensors."""
    filter_name: str = "to_tensor_mi355x"
    device: str = "cuda:0"
    keys: Dict[str, str] = field(default_factory=dict)
    dtype: str = ""  # e.g. "float32": what the odometry computes in (saves its own cast); "": keep the dtype


class ToTensor:
    """slam/preprocessing.py:110-126: numpy arrays -> tensors on the device under new keys; a tensor that already lives
    on the device is handed over as it is (zero-copy)."""

    def __init__(self, config: ToTensorConfig, device=None, **kwargs):
        self.config = config
        self.device = torch.device(device if device is not None else config.device)

    def filter(self, data_dict: dict):
        dtype = getattr(torch, self.config.dtype) if self.config.dtype else None
        for old_key, new_key in dict(self.config.keys).items():
            assert_debug(old_key in data_dict)
            a = data_dict[old_key]
            assert_debug(isinstance(a, (np.ndarray, torch.Tensor)))
            t = torch.from_numpy(a) if isinstance(a, np.ndarray) else a
            data_dict[new_key] = t.to(self.device, dtype) if dtype is not None else t.to(self.device)


# ----------------------------------------------------------------------------------------------------------------------
@dataclass
class DistortionConfig:
    """slam/preprocessing.py:130-141."""
    filter_name: str = "distortion"
    pointcloud_key: str = "numpy_pc"
    timestamps_key: str = "numpy_pc_timestamps"
    pose_key: str = "init_rpose"
    output_key: str = "input_data"
    force: bool = False
    activate: bool = True


class Distortion:
    """slam/preprocessing.py:144-191: de-skews a frame with the initial motion estimate (per-point slerp + linear
    translation by the normalised timestamp).  Pass-through (same array object) when deactivated, without timestamps or
    without an initial pose, exactly as the reference.  numpy in -> numpy out; cuda tensors in -> cuda tensor out."""

    def __init__(self, config: DistortionConfig, ctx: Optional[IcpContext] = None, **kwargs):
        self.config = config
        self._ctx = ctx

    def filter(self, data_dict: dict):
        c = self.config
        pc = data_dict[c.pointcloud_key]
        assert_debug(isinstance(pc, np.ndarray) or _is_device_tensor(pc), "Cannot Distort a non numpy frame")
        assert_debug(pc.ndim == 2 and pc.shape[1] == 3, f"expected [N, 3], got {pc.shape}")
        no_distortion = not c.activate or (c.timestamps_key not in data_dict)
        no_distortion = no_distortion or (data_dict[c.pose_key] is None if c.pose_key in data_dict else False)
        if no_distortion:
            data_dict[c.output_key] = pc
            return
        rpose = np.asarray(data_dict[c.pose_key])
        assert_debug(rpose.shape == (4, 4))
        timestamps = data_dict[c.timestamps_key]
        assert_debug(isinstance(timestamps, (np.ndarray, torch.Tensor)))
        timestamps = timestamps.reshape(-1)
        assert_debug(timestamps.shape[0] == pc.shape[0])
        ctx = self._ctx or _shared_context(pc.device if _is_device_tensor(pc) else None)
        if _is_device_tensor(pc):
            ctx.use_torch_stream()
        data_dict[c.output_key] = ctx.distort(pc, timestamps, rpose)


# ----------------------------------------------------------------------------------------------------------------------
class _PackedUpload:
    """`ToDevice._upload` for the B arrays of one key: one host copy each into ONE persistent pinned buffer, ONE DMA on an
    upload stream of its own into one of two alternating device slots, the caller's stream made to wait for it.  The
    tensors a call returns are views of that slot: overwritten TWO calls later (ToDevice's rule)."""

    def __init__(self, device):
        self.device = device
        self.pin = None
        self.free = None
        self.dev = [None, None]
        self.used = [None, None]
        self.which = 0
        self.stream = None

    def __call__(self, arrays):
        sizes = [int(a.size) for a in arrays]
        total = sum(sizes)
        if total == 0:
            return [torch.from_numpy(a).to(self.device) for a in arrays]
        tdtype = torch.from_numpy(arrays[0][:0]).dtype
        if self.pin is None or self.pin.numel() < total or self.pin.dtype != tdtype:
            self.pin = torch.empty(total, dtype=tdtype, pin_memory=True)
            self.free = None
        if self.free is not None:
            self.free.synchronize()  # the previous call's DMA has left the staging buffer (long done in practice)
        host = self.pin.numpy()
        off = 0
        for a, k in zip(arrays, sizes):
            host[off:off + k] = a.reshape(-1)
            off += k
        if self.stream is None:
            self.stream = torch.cuda.Stream(device=self.device)
        main = torch.cuda.current_stream(self.device)
        prev = self.which  # (the slot of the previous call: its readers are enqueued on `main` by now)
        if self.dev[prev] is not None:
            if self.used[prev] is None:
                self.used[prev] = torch.cuda.Event()
            self.used[prev].record(main)
        self.which ^= 1
        dev = self.dev[self.which]
        if dev is None or dev.numel() < total or dev.dtype != tdtype:
            dev = self.dev[self.which] = torch.empty(total, dtype=tdtype, device=self.device)
        with torch.cuda.stream(self.stream):
            if self.used[self.which] is not None:
                self.stream.wait_event(self.used[self.which])
            dev[:total].copy_(self.pin[:total], non_blocking=True)
            self.free = torch.cuda.Event()
            self.free.record(self.stream)
        main.wait_event(self.free)
        out, off = [], 0
        for a, k in zip(arrays, sizes):
            out.append(dev[off:off + k].view(a.shape))
            off += k
        return out


class MI355XPreprocessingBatch:
    """`Preprocessing.forward` (slam/preprocessing.py:269-290) for B frames at once, on the chain of
    config/slam/preprocessing/grid_sample_mi355x.yaml: to_device_mi355x -> distortion_mi355x -> grid_sample_mi355x ->
    to_tensor_mi355x.  `forward(dicts)` writes into every dict the keys, dtypes, shapes and values the four single filters
    (`ToDevice`, `Distortion`, `GridSample`, `ToTensor`) write, bit for bit, including Distortion's pass-through (no
    timestamps, `init_rpose` None or `activate: false`: `distorted` IS the uploaded float32 frame).

    One upload per key for all B frames (one pinned buffer, one DMA), then ONE library call (`IcpBatch.preprocess`): two
    launches de-skew the members with timestamps, four grid-sample all of them and write the float32 copy ToTensor makes.
    `padded: true`: nothing is read back; `padded: false` (the yaml's default): the B sample counts are read with ONE
    synchronisation and the dicts get V-row views (the exact-shape path's bits: same order of distinct voxel hashes).

    Lifetime: the uploaded frames (`pc_device`, `timestamps_device`) follow ToDevice's rule — views of a device slot that
    the call after next overwrites; clone them to keep them longer.  Every other tensor a call writes is a view of buffers
    allocated by that call (kept alive by the views) and stays valid for as long as the caller holds it."""

    CHAIN = ("to_device_mi355x", "distortion_mi355x", "grid_sample_mi355x", "to_tensor_mi355x")

    def __init__(self, filters_config, count: int, device=None, batch: Optional[IcpBatch] = None):
        cfg = filters_config
        if isinstance(cfg, dict) and "filters" in cfg:
            cfg = cfg["filters"]
        if isinstance(cfg, dict):
            cfg = [cfg[k] for k in sorted(cfg, key=lambda k: int(k))]
        cfg = [dict(c) for c in cfg]
        names = tuple(c.get("filter_name") for c in cfg)
        assert_debug(names == self.CHAIN, f"MI355XPreprocessingBatch batches the chain {' -> '.join(self.CHAIN)} "
                                          f"(config/slam/preprocessing/grid_sample_mi355x.yaml) only, got {' -> '.join(map(str, names))}")
        try:
            self.to_device = ToDeviceConfig(**cfg[0])
            self.distortion = DistortionConfig(**cfg[1])
            self.grid_sample = GridSampleConfig(**cfg[2])
            self.to_tensor = ToTensorConfig(**cfg[3])
        except TypeError as e:
            raise AssertionError(f"MI355XPreprocessingBatch: unknown filter option ({e})") from None
        dk = dict(self.to_device.keys)
        by_target = {v: k for k, v in dk.items()}
        c = self.distortion
        assert_debug(c.pointcloud_key in by_target and set(dk.values()) <= {c.pointcloud_key, c.timestamps_key},
                     "MI355XPreprocessingBatch: to_device_mi355x must upload exactly the frame (and its timestamps) "
                     "distortion_mi355x reads")
        assert_debug(self.grid_sample.pointcloud_key == c.output_key,
                     "MI355XPreprocessingBatch: grid_sample_mi355x must sample distortion_mi355x's output")
        assert_debug(dict(self.to_tensor.keys).keys() == {self.grid_sample.output_sample_key} and
                     self.to_tensor.dtype == "float32",
                     "MI355XPreprocessingBatch: to_tensor_mi355x must cast grid_sample_mi355x's samples to float32")
        self._pc_src = by_target[c.pointcloud_key]
        self._ts_src = by_target.get(c.timestamps_key)
        dev = torch.device(device if device is not None and str(device) != "cpu" else self.to_device.device)
        self.device = dev
        self.count = int(count)
        assert_debug(self.count >= 1, "a batch needs at least one frame")
        if batch is None:
            batch = IcpBatch([IcpContext(device=dev.index or 0) for _ in range(self.count)])
        assert_debug(len(batch) == self.count, f"a batch of {len(batch)} contexts for {self.count} frames")
        self.batch = batch
        self._uploads = {k: _PackedUpload(dev) for k in dk}

    def __len__(self):
        return self.count

    def forward(self, dicts):
        assert_debug(len(dicts) == self.count, f"expected {self.count} frames, got {len(dicts)}")
        c, gs = self.distortion, self.grid_sample
        dev = self.device
        # ---- ToDevice: every listed key present in the dicts, one DMA per key
        for src, dst in dict(self.to_device.keys).items():
            members = [k for k, d in enumerate(dicts) if src in d]
            host, passed = [], []
            for k in members:
                a = dicts[k][src]
                t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
                assert_debug(isinstance(t, torch.Tensor), f"cannot upload `{src}` of type {type(a)}")
                (passed if t.is_cuda else host).append((k, t))
            if host:
                dtypes = {t.dtype for _, t in host}
                assert_debug(len(dtypes) == 1, f"the `{src}` arrays of one batch must share a dtype, got {dtypes}")
                for (k, _), v in zip(host, self._uploads[src]([t.numpy() for _, t in host])):
                    dicts[k][dst] = v
            for k, t in passed:
                dicts[k][dst] = t.to(dev, non_blocking=True)
        # ---- Distortion's decisions, GridSample's inputs
        points, stamps, poses = [], [], []
        for k, d in enumerate(dicts):
            pc = d[c.pointcloud_key]
            assert_debug(_is_device_tensor(pc) and pc.dtype == torch.float32 and pc.ndim == 2 and pc.shape[1] == 3,
                         f"member {k}: expected a float32 [N, 3] frame, got {getattr(pc, 'dtype', type(pc))} "
                         f"{tuple(getattr(pc, 'shape', ()))}")
            no_distortion = not c.activate or (c.timestamps_key not in d)
            no_distortion = no_distortion or (d[c.pose_key] is None if c.pose_key in d else False)
            points.append(pc)
            if no_distortion:
                stamps.append(None)
                poses.append(None)
                continue
            rpose = np.asarray(d[c.pose_key])
            assert_debug(rpose.shape == (4, 4))
            ts = d[c.timestamps_key]
            assert_debug(isinstance(ts, torch.Tensor), f"member {k}: timestamps must be a tensor")
            ts = ts.reshape(-1)
            assert_debug(ts.shape[0] == pc.shape[0], f"member {k}: {ts.shape[0]} timestamps for {pc.shape[0]} points")
            stamps.append(ts.to(dev, torch.float64).contiguous())
            poses.append(rpose)
        # ---- the outputs of all members in four allocations
        ns = [int(p.shape[0]) for p in points]
        n64 = sum(n for n, t in zip(ns, stamps) if t is not None)
        buf64 = torch.empty(6 * n64, dtype=torch.float64, device=dev)
        buf32 = torch.empty(3 * sum(ns), dtype=torch.float32, device=dev)
        bufi = torch.empty(sum(ns), dtype=torch.int64, device=dev)
        counts = torch.empty(self.count, dtype=torch.int32, device=dev)
        outs, o64, o = [], 0, 0
        for k, (n, t) in enumerate(zip(ns, stamps)):
            f32 = buf32[3 * o:3 * (o + n)].view(n, 3)
            e = {"samples_f32": f32, "indices": bufi[o:o + n], "count": counts[k], "distorted": None, "samples": f32}
            if t is not None:
                e["distorted"] = buf64[3 * o64:3 * (o64 + n)].view(n, 3)
                e["samples"] = buf64[3 * (n64 + o64):3 * (n64 + o64 + n)].view(n, 3)
                o64 += n
            o += n
            outs.append(e)
        self.batch.preprocess(points, stamps, poses, gs.voxel_size, out=outs)
        padded = bool(getattr(gs, "padded", False))
        v = counts.cpu().tolist() if not padded else None  # (padded false: ONE synchronisation for the batch)
        (sample_src, sample_dst), = dict(self.to_tensor.keys).items()
        for k, (d, e) in enumerate(zip(dicts, outs)):
            d[c.output_key] = e["distorted"] if e["distorted"] is not None else points[k]
            if padded:
                d[gs.output_sample_key] = e["samples"]
                d[gs.output_indices_key] = e["indices"]
                d[getattr(gs, "output_count_key", "sample_count")] = e["count"]
                d[sample_dst] = e["samples_f32"]
            else:
                d[gs.output_sample_key] = e["samples"][:v[k]]
                d[gs.output_indices_key] = e["indices"][:v[k]]
                d[sample_dst] = e["samples_f32"][:v[k]] if e["samples"] is not e["samples_f32"] else d[gs.output_sample_key]
        return dicts

    __call__ = forward


# ----------------------------------------------------------------------------------------------------------------------
class ConstantVelocityInitialization:
    """slam/initialization.py:103-119: the initial guess is the last registered relative pose."""

    def __init__(self, *args, **kwargs):
        self.initial_estimate = None

    def init(self):
        self.initial_estimate = np.eye(4)

    @staticmethod
    def initial_pose_key():
        return "init_rpose"

    def next_initial_pose(self, **kwargs):
        return self.initial_estimate

    def next_frame(self, data_dict: dict, **kwargs):
        data_dict[self.initial_pose_key()] = self.next_initial_pose()

    def save_real_motion(self, relative_pose: np.ndarray, data_dict: Optional[dict] = None):
        self.initial_estimate = relative_pose


# ----------------------------------------------------------------------------------------------------------------------
@dataclass
class NeighborhoodResult:
    """LocalMap.NeighborhoodResult, slam/odometry/local_map.py:34-38."""
    neighbor_points: Any = None
    neighbor_normals: Any = None
    new_target_points: Any = None


def _is_context(obj) -> bool:
    return hasattr(obj, "map_init") and hasattr(obj, "register")


def _context_from(config, projector, device=None, **overrides) -> IcpContext:
    """An `IcpContext` for an inner-seam object built by one of the reference's registries (`LOCAL_MAP.load(config,
    pose=..., projector=...)`, `RIGID_ALIGNMENT.load(config, pose=...)`): the projector gives the image geometry."""
    kw = dict(height=int(getattr(projector, "height", 64)), width=int(getattr(projector, "width", 1024)),
              up_fov=float(getattr(projector, "up_fov", 3.0)), down_fov=float(getattr(projector, "down_fov", -24.0)))
    if device is not None and getattr(device, "index", None) is not None:
        kw["device"] = int(device.index)
    kw.update(overrides)
    return IcpContext(**kw)


def _like(reference, array: np.ndarray):
    """numpy result -> the kind (numpy / torch, device) of `reference`."""
    if isinstance(reference, torch.Tensor):
        return torch.from_numpy(np.ascontiguousarray(array)).to(reference.device)
    return array


@dataclass
class HashGridLocalMapConfig:
    """Registry config of `HashGridLocalMap` (LOCAL_MAP member `hashgrid_local_map_mi355x`); the fields of
    `KdTreeLocalMapConfig` (slam/odometry/local_map.py:243-251)."""
    type: str = "hashgrid_local_map_mi355x"
    pose: str = "euler"
    local_map_size: int = 20
    num_neighbors_normals: int = 10


class HashGridLocalMap:
    """Drop-in for `KdTreeLocalMap` (slam/odometry/local_map.py:254-427): a sliding window of the last
    `local_map_size` clouds, rebuilt (voxel-hash grid instead of a kd-tree) and with its lazy normal cache cleared on
    every update; exact 1-NN with no distance cap.  Built either around an existing context (`HashGridLocalMap(ctx)`,
    what `MI355XICPFrameToModel` does) or the way the reference's `LOCAL_MAP.load` builds a local map:
    `HashGridLocalMap(config, pose=..., projector=...)` (local_map.py:437-445, icp_odometry.py:93-94)."""

    def __init__(self, config_or_ctx=None, projector=None, pose=None, device=None, **kwargs):
        if _is_context(config_or_ctx):
            self.ctx, self.config = config_or_ctx, None
        else:
            self.config = config_or_ctx if config_or_ctx is not None else HashGridLocalMapConfig()
            self.ctx = _context_from(self.config, projector, device,
                                     local_map_size=int(_get(self.config, "local_map_size", 20)),
                                     num_neighbors_normals=int(_get(self.config, "num_neighbors_normals", 10)))
        self._last_count = 0

    def init(self):  # :279-288
        self.ctx.map_init()
        self._last_count = 0

    def set_map_pointcloud(self, pointcloud: np.ndarray, normals: Optional[np.ndarray] = None):  # :289-299
        assert_debug(isinstance(pointcloud, np.ndarray) and pointcloud.ndim == 2 and pointcloud.shape[1] == 3)
        assert_debug(normals is None, "externally supplied normals are not supported (the reference's own branch "
                                      "stores [M,3] where its cache expects [M,4], local_map.py:297-299,368,399)")
        self.ctx.map_set(pointcloud)

    def update(self, relative_pose, new_pc_data=None, new_vertex_map=None, **kwargs):  # :302-362
        if isinstance(relative_pose, torch.Tensor):
            assert_debug(tuple(relative_pose.shape) == (1, 4, 4))
            relative_pose = relative_pose[0].cpu().numpy()
        rel = np.asarray(relative_pose, dtype=np.float32)
        assert_debug(rel.shape == (4, 4))
        if kwargs.get("staged", False):  # the cloud handed to stage() before the registration
            self._last_count = self.ctx.map_update_staged(rel)
        elif new_pc_data is not None:
            pc = new_pc_data.reshape(-1, 3)
            self._last_count = self.ctx.map_update(rel, pc, skip_null=bool(kwargs.get("skip_null", False)))
        elif new_vertex_map is not None:
            vm = new_vertex_map
            assert_debug(vm.ndim == 4 and vm.shape[0] == 1 and vm.shape[1] == 3)
            self._last_count = self.ctx.map_update_vertex_map(rel, vm[0])
        else:
            self.ctx.map_update(rel, None)

    def stage(self, new_pc_data, skip_null: bool = False):
        """The cloud the next `update(..., staged=True)` inserts, handed over before the registration it follows: its rows
        are compacted and counted on the device while the host goes on (icp_map_stage_cloud) — same map as
        `update(pose, new_pc_data=...)`, one host synchronisation per frame less."""
        self.ctx.map_stage_cloud(new_pc_data.reshape(-1, 3), skip_null=skip_null)

    def nearest_neighbor_search(self, target_points, with_normals: bool = True, with_new_target_points: bool = True,
                                **kwargs) -> NeighborhoodResult:  # :372-395
        """Results live where the query lives: cuda tensors for a cuda tensor (zero-copy), cpu tensors for a cpu
        tensor (the reference returns tensors on the query's device, :389-394), numpy for numpy."""
        is_torch = isinstance(target_points, torch.Tensor)
        assert_debug(target_points.ndim == 2 and target_points.shape[1] == 3)
        nb, nm, _ = self.ctx.nearest_neighbor_search(target_points, with_normals=with_normals)
        res = NeighborhoodResult()
        if is_torch:
            res.neighbor_points = (nb if isinstance(nb, torch.Tensor) else _like(target_points, nb)).unsqueeze(0)
            if with_normals:
                res.neighbor_normals = (nm if isinstance(nm, torch.Tensor) else _like(target_points, nm)).unsqueeze(0)
            if with_new_target_points:
                res.new_target_points = target_points.reshape(1, -1, 3)
        else:
            res.neighbor_points = nb
            res.neighbor_normals = nm if with_normals else None
            res.new_target_points = target_points if with_new_target_points else None
        return res

    def get_last_frame(self) -> torch.Tensor:  # :424-427
        pts = self.ctx.map_points()
        return torch.from_numpy(pts[pts.shape[0] - self._last_count:])


@dataclass
class ProjectiveLocalMapConfig:
    """Registry config of `ProjectiveLocalMap` (LOCAL_MAP member `projective_local_map_mi355x`); the fields of the
    reference's `ProjectiveLocalMapConfig` (slam/odometry/local_map.py:82-88)."""
    type: str = "projective_local_map_mi355x"
    pose: str = "euler"
    local_map_size: int = 20
    normals_kernel_size: int = 5


class ProjectiveLocalMap:
    """Drop-in for `ProjectiveLocalMap` (slam/odometry/local_map.py:91-240), the reference's "GPU" local map: the last
    `local_map_size` vertex maps with box-filter normal maps, re-projected into the current frame on every update;
    neighbours by per-pixel association over the stored maps.  `ProjectiveLocalMap(ctx, normals_kernel_size)` or, the
    reference's registry form, `ProjectiveLocalMap(config, projector=..., pose=...)`."""

    def __init__(self, config_or_ctx=None, normals_kernel_size: Optional[int] = None, projector=None, pose=None,
                 device=None, **kwargs):
        if _is_context(config_or_ctx):
            self.ctx, self.config = config_or_ctx, None
            self.normals_kernel_size = 5 if normals_kernel_size is None else int(normals_kernel_size)
        else:
            self.config = config_or_ctx if config_or_ctx is not None else ProjectiveLocalMapConfig()
            self.ctx = _context_from(self.config, projector, device,
                                     local_map_size=int(_get(self.config, "local_map_size", 20)))
            self.normals_kernel_size = int(_get(self.config, "normals_kernel_size", 5))
        self._last_vmap = None

    def init(self):  # :113-119
        self.ctx.pmap_init()
        self._last_vmap = None

    def update(self, relative_pose, new_vertex_map=None, **kwargs):  # :122-174
        if isinstance(relative_pose, torch.Tensor):
            assert_debug(tuple(relative_pose.shape) == (1, 4, 4))
            relative_pose = relative_pose[0].cpu().numpy()
        rel = np.asarray(relative_pose, dtype=np.float32)
        assert_debug(rel.shape == (4, 4))
        if new_vertex_map is not None:
            assert_debug(new_vertex_map.ndim == 4 and new_vertex_map.shape[0] == 1 and new_vertex_map.shape[1] == 3)
            self.ctx.pmap_update(rel, new_vertex_map[0], self.normals_kernel_size)
            self._last_vmap = new_vertex_map[0]
        else:
            self.ctx.pmap_update(rel, None)

    def nearest_neighbor_search(self, target_points, with_normals: bool = True, with_new_target_points: bool = True,
                                **kwargs) -> NeighborhoodResult:  # :205-235
        assert_debug(target_points.ndim == 2 and target_points.shape[1] == 3)
        nb, nm, tg = self.ctx.pmap_nearest_neighbor_search(target_points)
        if isinstance(target_points, torch.Tensor):  # results on the query's device (cuda: straight from the kernel)
            wrap = lambda a: (a if isinstance(a, torch.Tensor) else _like(target_points, a)).unsqueeze(0)
        else:
            wrap = lambda a: a[None]
        res = NeighborhoodResult()
        res.neighbor_points = wrap(nb)
        if with_normals:
            res.neighbor_normals = wrap(nm)
        if with_new_target_points:
            res.new_target_points = wrap(tg)
        return res

    def get_last_frame(self):  # :238-240 — the points of the newest stored vertex map, [H*W, 3] (null pixels included)
        assert_debug(self._last_vmap is not None, "the local map is empty")
        vm = self._last_vmap
        if isinstance(vm, torch.Tensor):
            return vm.permute(1, 2, 0).reshape(-1, 3)
        return torch.from_numpy(np.ascontiguousarray(np.asarray(vm).transpose(1, 2, 0).reshape(-1, 3)))


@dataclass
class PointToPlaneAlignmentConfig:
    """Registry config of `PointToPlaneAlignment` (RIGID_ALIGNMENT member `point_to_plane_gauss_newton_mi355x`); the
    fields of `GaussNewtonPointToPlaneConfig` (slam/odometry/alignment.py:69-77)."""
    mode: str = "point_to_plane_gauss_newton_mi355x"
    pose: str = "euler"
    num_gn_iters: int = 1
    gauss_newton_config: Dict[str, Any] = field(default_factory=lambda: dict(max_iters=1))


@dataclass
class PointToPointAlignmentConfig:
    """Registry config of `PointToPointAlignment` (RIGID_ALIGNMENT member `point_to_point_gauss_newton_mi355x`); the
    fields of `GNPointToPointConfig` (slam/odometry/alignment.py:131-140)."""
    mode: str = "point_to_point_gauss_newton_mi355x"
    pose: str = "euler"
    num_gn_iters: int = 1
    initialize_with_svd: bool = False
    gauss_newton_config: Dict[str, Any] = field(default_factory=lambda: dict(max_iters=1))


def _alignment_context(config, device) -> IcpContext:
    gn = _get(config, "gauss_newton_config", {}) or {}
    assert_debug(int(_get(gn, "max_iters", 1)) == 1,
                 "the MI355X alignments run exactly one Gauss-Newton step per align() (gauss_newton_config.max_iters "
                 "= 1, the reference's default)")
    return _context_from(config, None, device, scheme=str(_get(gn, "scheme", "default")),
                         sigma=float(_get(gn, "sigma", 0.5)))


def _residuals_like(reference, residuals):
    """[n] residuals -> [1, n] on the device / of the kind of `reference`."""
    if isinstance(reference, torch.Tensor):
        r = residuals if isinstance(residuals, torch.Tensor) else torch.from_numpy(residuals)
        return r.to(reference.device).unsqueeze(0)
    return np.asarray(residuals)[None]


class PointToPlaneAlignment:
    """Drop-in for `GaussNewtonPointToPlaneAlignment.align` (slam/odometry/alignment.py:91-127): one Gauss-Newton
    point-to-plane step from x0 = 0 on given correspondences; returns (pose [1,4,4], params [1,6], residuals [1,N] =
    (w r)^2 per row) — torch tensors on the device of the inputs, like the reference (its caller multiplies the pose
    with a tensor on that device and sums the residuals, icp_odometry.py:284-297), numpy for numpy inputs.
    `PointToPlaneAlignment(ctx)` or, the reference's registry form, `PointToPlaneAlignment(config, pose=...)`."""

    def __init__(self, config_or_ctx=None, pose=None, device=None, **kwargs):
        if _is_context(config_or_ctx):
            self.ctx, self.config = config_or_ctx, None
        else:
            self.config = config_or_ctx if config_or_ctx is not None else PointToPlaneAlignmentConfig()
            self.ctx = _alignment_context(self.config, device)

    def align(self, ref_points, tgt_points, ref_normals=None, initial_estimate=None, mask=None, **kwargs):
        assert_debug(ref_normals is not None,
                     "The argument 'ref_normals' is required for a point to plane alignemnt")
        assert_debug(initial_estimate is None and mask is None,
                     "`initial_estimate` / `mask` are not supported by the MI355X point-to-plane alignment (the "
                     "frame-to-model loop passes neither, icp_odometry.py:284-287; the reference's own align raises on "
                     "a mask: optimization.py:393-394)")
        r = ref_points.reshape(-1, 3)
        t = tgt_points.reshape(-1, 3)
        n = ref_normals.reshape(-1, 3)
        pose, dx, _, _, res = self.ctx.align_point_to_plane(r, t, n, with_residuals=True)
        return _like(ref_points, pose[None]), _like(ref_points, dx[None]), _residuals_like(ref_points, res)


class PointToPointAlignment:
    """Drop-in for `GaussNewtonPointToPointAlignment.align` (slam/odometry/alignment.py:143-189): one Gauss-Newton
    point-to-point step on given correspondences, linearised at `initial_estimate` (zeros by default; the Procrustes
    solution when `initialize_with_svd`); returns (pose [1,4,4], params [1,6], residuals [1,N]) like the reference,
    on the device of the inputs."""

    def __init__(self, config_or_ctx=None, initialize_with_svd: Optional[bool] = None, pose=None, device=None, **kwargs):
        if _is_context(config_or_ctx):
            self.ctx, self.config = config_or_ctx, None
            self.initialize_with_svd = bool(initialize_with_svd)
        else:
            self.config = config_or_ctx if config_or_ctx is not None else PointToPointAlignmentConfig()
            self.ctx = _alignment_context(self.config, device)
            self.initialize_with_svd = bool(_get(self.config, "initialize_with_svd", False)) \
                if initialize_with_svd is None else bool(initialize_with_svd)

    def align(self, ref_points, tgt_points, initial_estimate=None, mask=None, **kwargs):
        assert_debug(mask is None, "`mask` is not supported by the MI355X point-to-point alignment")
        r = ref_points.reshape(-1, 3)
        t = tgt_points.reshape(-1, 3)
        x0 = None
        if self.initialize_with_svd:  # alignment.py:170-171, arguments in the reference's order
            x0 = from_pose_matrix(self.ctx.weighted_procrustes(r, t).astype(np.float32))
        elif initial_estimate is not None:
            est = initial_estimate.detach().cpu().numpy() if isinstance(initial_estimate, torch.Tensor) else \
                np.asarray(initial_estimate)
            x0 = from_pose_matrix(est.reshape(4, 4).astype(np.float32)) if est.size == 16 else \
                est.reshape(6).astype(np.float32)
        pose, params, _, _, res = self.ctx.align_point_to_point(r, t, x0, with_residuals=True)
        return _like(ref_points, pose[None]), _like(ref_points, params[None]), _residuals_like(ref_points, res)


# ----------------------------------------------------------------------------------------------------------------------
@dataclass
class MI355XICPConfig:
    """Mirrors `ICPFrameToModelConfig` (slam/odometry/icp_odometry.py:29-64) with the sub-configs flattened:
    `local_map` = KdTreeLocalMapConfig (local_map.py:243-251), `alignment` = GaussNewtonPointToPlaneConfig
    (alignment.py:69-77)."""
    algorithm: str = "icp_F2M_mi355x"
    device: str = "cuda:0"
    pose: str = "euler"
    max_num_alignments: int = 100
    threshold_delta_pose: float = 1.0e-4
    threshold_trans: float = 0.1
    threshold_rot: float = 0.3
    sigma: float = 0.1  # dead field in the reference too (icp_odometry.py:51)
    data_key: str = "vertex_map"
    local_map: Dict[str, Any] = field(default_factory=lambda: dict(type="kdtree_local_map", local_map_size=20,
                                                                   num_neighbors_normals=10))
    alignment: Dict[str, Any] = field(default_factory=lambda: dict(
        mode="point_to_plane_gauss_newton", gauss_newton_config=dict(max_iters=1)))
    initialization: Any = None
    viz_debug: bool = False
    # MI355X-side knobs
    cell_size: float = 0.0  # <= 0: auto-tuned
    max_rings: int = 2
    # frames of at most that many rows are compacted and counted in FRONT of their registration (icp_map_stage_cloud), so
    # that the map update after it needs no host round trip of its own: 6 106-row frames 0.64 -> 0.61 ms; a 131 072-row
    # frame pays more for the compaction on the registration's critical path than the round trip costs (0.516 -> 0.540 ms)
    stage_insert_max_rows: int = 32768
    # the non-null pixels of a sparse vertex map (a grid-sampled frame: 6 000 of 131 072) are compacted into consecutive
    # target rows in front of the registration (True: round 4's schedule), or the registration walks all H x W pixels and
    # masks the null ones inside its kernels (False: the valid queries stay spread over all 256 workgroups of a launch instead
    # of filling 12 — measured in round 5 on the published configuration: 0.52-0.55 vs 0.60 ms per frame)
    compact_sparse_vertex_map: bool = False
    # True: a frame is ONE pair of library calls (icp_frame_launch + icp_frame_end, include/icp_mi355x.h) instead of the ten
    # calls of do_process_next_frame below — the same poses, iterations, insertions and map, bit for bit.  numpy [N, 3] and
    # cuda [N, 3] frames against the kd-tree style map; anything else is refused with the reason, not routed elsewhere.
    # `MI355XICPFrameToModelBatch`: a step of all members is ONE pair of calls (icp_batch_frame_launch + icp_batch_frame_end),
    # and numpy [N, 3] frames are accepted on that route
    one_call_frame: bool = False
    # The same for the projective local map (PF2M): a frame is icp_pmap_frame_launch + icp_pmap_frame_end — the same poses,
    # iterations, key frames, clouds, window and model, bit for bit.  numpy [N, 3], cuda [N, 3] and cuda [3, H, W] /
    # [1, 3, H, W] vertex-map frames; anything else is refused with the reason, and so is the flag on a kd-tree style map
    one_call_projective_frame: bool = False
    # > 0: every frame's `odometry_pc` goes, with its float64 absolute pose and its frame index, into an aggregated world map on
    # the device (`IcpContext.aggregated_map`, icp_aggmap_*: one float64 point per voxel of that edge, in creation order) —
    # the concatenation the reference's loop closure starts from (slam/loop_closure.py:272-291), exposed as
    # `odo.aggregated_map`.  Three launches behind every frame; the poses are the same, bit for bit.  0 (the default): no
    # map is created and nothing is launched.  Frame 0 has no `odometry_pc` (the reference returns before it writes one,
    # icp_odometry.py:176-181) and is not inserted
    aggregate_map_voxel: float = 0.0
    aggregate_map_capacity: int = 2000000  # points; rows in voxels beyond it are counted as dropped


def _get(obj, key, default=None):
    if obj is None:
        return default
    if isinstance(obj, dict):
        return obj.get(key, default)
    return getattr(obj, key, default)


def key_frame_decision(delta: np.ndarray, pose: np.ndarray, threshold_trans: float, threshold_rot: float):
    """`__update_map`'s test (:360-380): (key frame?, delta @ pose in float32) — metres, and degrees of the Euler vector."""
    new_delta = (delta @ pose).astype(np.float32)
    dp = from_pose_matrix(new_delta)
    return bool(np.linalg.norm(dp[:3]) > threshold_trans or np.linalg.norm(dp[3:]) * 180 / np.pi > threshold_rot), new_delta


class _OneCallKdTree:
    """`one_call_frame`: what the one-call paths need to know of the kd-tree style map."""
    flag = "one_call_frame"
    vertex_maps = False  # (a vertex-map tensor goes through the per-call path)
    init, launch, end = "odometry_init", "frame_launch", "frame_end"  # on IcpContext and on IcpBatch
    refusal = ("one_call_frame covers numpy [N, 3] and cuda [N, 3] frames: a vertex-map tensor (or a cpu tensor) goes "
               "through the per-call path (one_call_frame=False), got ")
    refusal_batch = ("one_call_frame covers numpy [N, 3] and cuda [N, 3] frames (all members alike): a vertex-map tensor (or a "
                     "cpu tensor) goes through the per-call path (one_call_frame=False), got ")
    copy_points = True  # `odometry_pc` is a copy of the rows the end call hands out

    @staticmethod
    def init_extra(member, data_dicts) -> dict:
        # (a frame that comes padded from the device-resident grid sample is staged whatever its row count, as
        # do_process_next_frame does: `sample_count` says so at frame 0; the batched calls stage every frame whatever it says)
        return dict(stage_max_rows=0 if any(d.get("sample_count", None) is not None for d in data_dicts) else
                    int(_get(member.config, "stage_insert_max_rows", 32768)))

    @staticmethod
    def record_key_frame(member, res, frame, is_vmap):
        member.local_map._last_count = res.inserted


class _OneCallProjective:
    """`one_call_projective_frame`: the same of the projective local map."""
    flag = "one_call_projective_frame"
    vertex_maps = True
    init, launch, end = "pmap_odometry_init", "pmap_frame_launch", "pmap_frame_end"
    refusal = ("one_call_projective_frame covers numpy [N, 3], cuda [N, 3] and cuda [3, H, W] / [1, 3, H, W] frames: "
               "anything else (a cpu tensor) goes through the per-call path (one_call_projective_frame=False), got ")
    refusal_batch = ("one_call_projective_frame covers numpy [N, 3], cuda [N, 3] and cuda [3, H, W] / [1, 3, H, W] frames (all "
                     "members alike): anything else (a cpu tensor) goes through the per-call path, got ")
    copy_points = False  # (a view of the fresh array the end call filled: nobody else holds it)

    @staticmethod
    def init_extra(member, data_dicts) -> dict:
        return dict(normals_kernel_size=int(member.local_map.normals_kernel_size))

    @staticmethod
    def record_key_frame(member, res, frame, is_vmap):
        # (`get_last_frame`: a vertex map handed in is the newest stored map; for rows the library's projection is repeated
        # here — the same pixels — behind the frame, off its critical path)
        member.local_map._last_vmap = (frame[0] if frame.ndim == 4 else frame) if is_vmap else member.ctx.project(frame)


class MI355XICPFrameToModel(OdometryAlgorithm):
    """Drop-in for `ICPFrameToModel` (slam/odometry/icp_odometry.py:72-381) with the kd-tree local map and the
    Gauss-Newton point-to-plane alignment, every per-point stage on the MI355X."""

    def __init__(self, config: MI355XICPConfig, projector=None, pose=None, device=None, **kwargs):
        if not isinstance(config, MI355XICPConfig):
            known = {f for f in MI355XICPConfig.__dataclass_fields__}
            config = MI355XICPConfig(**{k: v for k, v in dict(config).items() if k in known})
        super().__init__(config)
        assert_debug(projector is not None)
        self.projector = projector
        lm = config.local_map
        lm_type = str(_get(lm, "type", "kdtree_local_map")).replace("_mi355x", "")
        self._projective = lm_type == "projective_local_map"
        assert_debug(self._projective or lm_type in ("kdtree_local_map", "hashgrid_local_map"),
                     f"unknown local map type {_get(lm, 'type')}")
        gn = _get(config.alignment, "gauss_newton_config", {}) or {}
        mode = str(_get(config.alignment, "mode", "point_to_plane_gauss_newton")).replace("_mi355x", "")
        assert_debug(mode in ("point_to_plane_gauss_newton", "point_to_point_gauss_newton"),
                     f"unknown alignment mode {mode} (RIGID_ALIGNMENT, slam/odometry/alignment.py:200-208)")
        # options the device loop does not implement are refused, not ignored
        assert_debug(int(_get(gn, "max_iters", 1)) == 1,
                     "gauss_newton_config.max_iters must be 1: every ICP iteration runs one Gauss-Newton step "
                     "(the reference's configurations, config/slam/odometry/alignment/*.yaml)")
        self._point_to_point = mode == "point_to_point_gauss_newton"
        assert_debug(not (self._point_to_point and self._projective),
                     "the point-to-point alignment runs against the kd-tree style local map only")
        assert_debug(not (self._point_to_point and bool(_get(config.alignment, "initialize_with_svd", False))),
                     "initialize_with_svd is available at the RigidAlignment seam (PointToPointAlignment), not inside "
                     "the device-resident loop")
        dev_index = 0
        if device is not None and getattr(device, "index", None) is not None:
            dev_index = device.index
        self.ctx = IcpContext(
            height=int(projector.height), width=int(projector.width), up_fov=float(projector.up_fov),
            down_fov=float(projector.down_fov), max_num_alignments=int(config.max_num_alignments),
            threshold_delta_pose=float(config.threshold_delta_pose), scheme=str(_get(gn, "scheme", "default")),
            sigma=float(_get(gn, "sigma", 0.5)), local_map_size=int(_get(lm, "local_map_size", 20)),
            num_neighbors_normals=int(_get(lm, "num_neighbors_normals", 10)), cell_size=float(config.cell_size),
            max_rings=int(config.max_rings), device=dev_index)
        self.device = self.ctx.device
        self.local_map = ProjectiveLocalMap(self.ctx, int(_get(lm, "normals_kernel_size", 5))) if self._projective \
            else HashGridLocalMap(self.ctx)
        if self._point_to_point:
            self.ctx.set_cost("point_to_point_gauss_newton")
            self.rigid_alignment = PointToPointAlignment(self.ctx)
        else:
            self.rigid_alignment = PointToPlaneAlignment(self.ctx)
        self.gn_max_iters = config.max_num_alignments
        self._sample_pointcloud = False
        self.relative_poses: List[np.ndarray] = []
        self.absolute_poses: List[np.ndarray] = []
        self.last_result: Optional[RegisterResult] = None
        self._iter = 0
        self._tgt_vmap = None
        self._tgt_rows = None
        self._tgt_pc = None
        self._delta_since_map_update = np.eye(4, dtype=np.float32)
        self._host_rows = None
        self._pin_in = self._pin_in_free = self._pin_out = self._copy_stream = self._upload_stream = None
        self._dev_in, self._dev_slot = [None, None], 0
        self._register_threshold_trans = config.threshold_trans
        self._register_threshold_rot = config.threshold_rot
        self._one_call = bool(_get(config, "one_call_frame", False))
        self._one_call_targets = None
        if self._one_call:
            assert_debug(not self._projective, "one_call_frame: the frame calls of the library run the kd-tree style local "
                                               "map, not the projective one")
            assert_debug(not bool(_get(config, "compact_sparse_vertex_map", False)),
                         "one_call_frame: compact_sparse_vertex_map is a schedule of the per-call path only")
            assert_debug(hasattr(self.ctx, "frame_launch"), "one_call_frame needs the library's frame calls")
        self.aggregated_map = None
        voxel = float(_get(config, "aggregate_map_voxel", 0.0) or 0.0)
        assert_debug(voxel >= 0.0, f"aggregate_map_voxel = {voxel} is negative")
        if voxel > 0.0:
            assert_debug(hasattr(self.ctx, "aggregated_map"), "aggregate_map_voxel needs the library's aggregated map")
            self.aggregated_map = self.ctx.aggregated_map(
                voxel, int(_get(config, "aggregate_map_capacity", 2000000)),
                max_insert_rows=max(262144, int(projector.height) * int(projector.width)))
        self._one_call_pmap = bool(_get(config, "one_call_projective_frame", False))
        if self._one_call_pmap:
            assert_debug(self._projective, "one_call_projective_frame: the projective frame calls of the library run the "
                                           "projective local map; the kd-tree style map has one_call_frame")
            assert_debug(not bool(_get(config, "compact_sparse_vertex_map", False)),
                         "one_call_projective_frame: compact_sparse_vertex_map is a schedule of the per-call path only")
            assert_debug(hasattr(self.ctx, "pmap_frame_launch"),
                         "one_call_projective_frame needs the library's projective frame calls")
        self._one_call_kind = _OneCallKdTree if self._one_call else _OneCallProjective if self._one_call_pmap else None

    def init(self):  # :128-145
        super().init()
        self._warn_handoff_fallbacks()  # (what the sequence before this one went through)
        self.relative_poses = []
        self.absolute_poses = []
        self.local_map.init()
        self._iter = 0
        self._delta_since_map_update = np.eye(4, dtype=np.float32)
        if self.aggregated_map is not None:
            self.aggregated_map.clear()

    def _aggregate(self, data_dict: dict, device_rows=None):
        """`aggregate_map_voxel` > 0: the frame's `odometry_pc` into the aggregated map, with the absolute pose just appended
        and the frame index.  `device_rows`: the frame's [N, 3] point rows where they are still on the device — inserted from
        there (the same rows as `odometry_pc`; a row with a NaN, which `odometry_pc` leaves out, is set aside by the map and
        counted as non-finite); otherwise the host rows of `odometry_pc` are inserted."""
        if self.aggregated_map is None:
            return
        rows = device_rows if device_rows is not None else data_dict[self.pointcloud_key()]
        if isinstance(rows, torch.Tensor) and not rows.is_cuda:
            rows = rows.numpy()
        self.aggregated_map.insert(rows, self.absolute_poses[-1], self._iter)

    def _warn_handoff_fallbacks(self):
        """Once per sequence (VERDICT r5 Weak #14): registrations whose pose hand-off inside a launch timed out were finished
        on per-iteration launches — same poses, but each one cost a 50 ms wall-clock timeout, and the context runs without
        lead launches from then on.  Silent in the library (`icp_handoff_fallbacks`); said aloud here."""
        ctx = getattr(self, "ctx", None)
        if ctx is None or not hasattr(ctx, "handoff_fallbacks"):
            return
        count = int(ctx.handoff_fallbacks())
        seen = getattr(self, "_handoff_fallbacks_seen", 0)
        if count > seen:
            import warnings
            warnings.warn(f"MI355XICPFrameToModel: {count - seen} registration(s) since the last check were finished on "
                          f"per-iteration launches behind a timed-out pose hand-off (icp_handoff_fallbacks = {count}): the GPU is "
                          "probably shared with other work; poses are unaffected, each such frame cost ~50 ms and the context "
                          "keeps to plain launches (set_option('lead_solve', 1) re-arms the hand-offs)", RuntimeWarning)
        self._handoff_fallbacks_seen = count

    @staticmethod
    def _initial_pose(data_dict: dict) -> np.ndarray:  # :147-154
        rpose = data_dict.get("init_rpose", None)
        if rpose is None:
            return np.eye(4, dtype=np.float32)
        if isinstance(rpose, torch.Tensor):
            # BASELINE configs[4]: a pose network's output (slam/initialization.py:222-283 writes a numpy array; a network
            # running on the device in bf16 hands over a tensor) — 16 numbers to the host, float32 from here on
            rpose = rpose.detach().to(torch.float32).cpu().numpy()
        return np.asarray(rpose).astype(np.float32).reshape(-1)[-16:].reshape(4, 4)

    # ------------------------------------------------------------------------------------------------------------------
    def _read_input(self, data_dict: dict, projected=None):  # :319-358
        """`projected`: (vertex map, rows or None) of this frame's [N, 3] device rows, already enqueued by the caller
        (`MI355XICPFrameToModelBatch`: one batched projection for all members) — the projection is not repeated here."""
        key = self.config.data_key
        assert_debug(key in data_dict, f"Could not find the key `{key}` in the input dictionary.\n"
                                       f"With keys : {data_dict.keys()}). Set the parameter "
                                       f"`slam.odometry.data_key` to the desired key")
        data = data_dict[key]
        self._tgt_vmap = None
        self._tgt_pc = None
        self._tgt_rows = None
        self._host_rows = None
        self._staged = False
        if isinstance(data, np.ndarray):
            assert_debug(data.ndim == 2 and data.shape[1] == 3, f"expected [N, 3], got {data.shape}")
            self._sample_pointcloud = True  # sticky (:330)
            self._host_rows = data if data.dtype == np.float32 and data.flags.c_contiguous else \
                np.ascontiguousarray(data, dtype=np.float32)
            pc = self._upload(self._host_rows)
            # the vertex map of a frame whose POINTS are registered and inserted (kd-tree style map) is not read before the
            # registration: projected behind its launch (do_process_next_frame), while the GPU iterates
            vmap = None if self._defer_projection() else self.ctx.project(pc)
        elif isinstance(data, torch.Tensor):
            if data.ndim in (3, 4):
                vmap = data.to(self.device, torch.float32)
                if data.ndim == 4:
                    assert_debug(data.shape[0] == 1, "Unexpected batched data format.")
                    vmap = vmap[0]
                assert_debug(vmap.shape[0] == 3)
                vmap = vmap.contiguous()
                # all H*W pixels; null / NaN pixels are masked inside the kernels (mask_not_null :343-344)
                pc = vmap.permute(1, 2, 0).reshape(-1, 3).contiguous()
            else:
                assert_debug(data.ndim == 2)
                pc = data.to(self.device, torch.float32).contiguous()
                if projected is not None:
                    vmap, self._tgt_rows = projected
                elif not self._sample_pointcloud and pc.is_cuda and hasattr(self.ctx, "project_rows"):
                    # the targets will be the pixels of this vertex map (sample_points): the projection writes them as
                    # rows too, instead of a transposing copy per frame
                    vmap, self._tgt_rows = self.ctx.project_rows(pc)
                else:
                    vmap = self.ctx.project(pc)
        else:
            raise RuntimeError(f"Could not interpret the data: {data} as a pointcloud tensor")
        # modify_nan_pmap (:356): a projected map never holds a NaN (NaN rows fail the pixel-validity test); a
        # caller-supplied vertex map keeps its NaN pixels, which every kernel masks exactly like null pixels
        self._tgt_vmap = vmap
        self._tgt_pc = pc
        self._pc_is_pixels = isinstance(data, torch.Tensor) and data.ndim in (3, 4)

    def _defer_projection(self) -> bool:
        return self._iter > 0 and not self._projective and self.device.type == "cuda"

    def sample_points(self):  # :301-308 — returns (device rows, skip_null)
        if not self._sample_pointcloud:
            h, w = self._tgt_vmap.shape[-2:]
            pixels = self._tgt_rows if self._tgt_rows is not None else \
                self._tgt_vmap.permute(1, 2, 0).reshape(h * w, 3).contiguous()
            # the non-null pixels (:303-305).  A vertex map projected from N points has at most N of them: when that is
            # well below H * W (a grid-sampled frame: 6 000 of 131 072) they are compacted on the device, in pixel order,
            # so the registration walks N rows — and estimates normals lazily for what N rows touch — instead of H * W
            n_in = self._tgt_pc.shape[0] if (self._tgt_pc is not None and not self._pc_is_pixels) else h * w
            if pixels.is_cuda and 2 * n_in <= h * w and hasattr(self.ctx, "compact_targets") and \
                    bool(_get(self.config, "compact_sparse_vertex_map", False)):
                return self.ctx.compact_targets(pixels, n_in, skip_null=True), True
            return pixels, True
        return self._tgt_pc, self._pc_is_pixels

    def register_new_frame(self, target_points, initial_estimate=None, skip_null: bool = False, **kwargs):  # :248-299
        if self._projective:
            res = self.ctx.pmap_register(target_points, initial_estimate, skip_null=skip_null)
        else:
            res = self.ctx.register(target_points, initial_estimate, skip_null=skip_null)
        self.last_result = res
        return res.params, res.pose, res.losses

    def do_process_next_frame(self, data_dict: dict):  # :157-246
        """One frame.  Against the kd-tree style map the registration is only ENQUEUED (`icp_register_launch`): while the
        GPU iterates, the host prepares the frame's `odometry_pc` (the host rows of a numpy frame, or an asynchronous
        device -> pinned copy of a tensor frame started before the registration was enqueued), then blocks on the
        registration alone (`icp_register_end`); the map update is enqueued from the pose without waiting for it, so it
        overlaps the caller's preparation of the next frame."""
        self.ctx.use_torch_stream()
        if self._one_call_kind is not None:
            return self._one_call_next_frame(data_dict)
        self._read_input(data_dict)
        if self._iter == 0:
            self.local_map.update(np.eye(4, dtype=np.float32), new_vertex_map=self._tgt_vmap.unsqueeze(0))  # :176
            return self._first_frame_done()
        initial_estimate = self._initial_pose(data_dict)
        targets, skip_null = self.sample_points()
        want_rows = "distorted" not in data_dict  # (:210-213: the de-skewed frame stands in for `_tgt_pc` when there is one)
        rows_ready = self._rows_event() if want_rows else None  # (recorded BEFORE the registration is enqueued)
        if self._projective:
            self.register_new_frame(targets, initial_estimate, skip_null=skip_null)
            tgt_np_pc = self._rows_to_host(rows_ready) if want_rows else data_dict["distorted"]
        else:
            # the frame goes into the map right after its registration (:229-231): its valid rows are compacted and counted
            # NOW, in front of the registration, so that the update finds the count on the host (one synchronisation less)
            # (rows in host memory would make the staging call wait for their upload: no round trip saved — except under
            # the CPU stand-in of tests/, which exercises this flow without a GPU)
            # (a frame that comes padded from the device-resident grid sample — a handful of valid rows among NaN rows —
            # is staged whatever its row count: the compaction walks flags, what it copies is the handful)
            self._staged = hasattr(self.local_map, "stage") and \
                (self._tgt_pc.is_cuda or self.device.type != "cuda") and \
                (int(self._tgt_pc.shape[0]) <= int(_get(self.config, "stage_insert_max_rows", 32768)) or
                 data_dict.get("sample_count", None) is not None)
            if self._staged:
                self.local_map.stage(self._tgt_pc, skip_null=self._pc_is_pixels)
            self.ctx.register_launch(targets, initial_estimate, skip_null=skip_null)
            if self._tgt_vmap is None:  # (deferred in _read_input: enqueued behind the registration, off its critical path)
                self._tgt_vmap = self.ctx.project(self._tgt_pc)
            tgt_np_pc = self._rows_to_host(rows_ready) if want_rows else data_dict["distorted"]  # GPU busy meanwhile
            self.last_result = self.ctx.register_end()  # raises before the map is touched (:286)
        self.__update_map(self.last_result.pose)
        self._frame_done(data_dict, self.last_result, tgt_np_pc,
                         self._tgt_pc if (want_rows and self._tgt_pc.is_cuda and not self._pc_is_pixels) else None)

    # ---- the ends of a frame every path shares ---------------------------------------------------------------------------
    def _first_frame_done(self):
        """Frame 0 is in the map (:176-181): the identity opens both pose chains; nothing is written to the dict."""
        self.relative_poses.append(np.eye(4, dtype=np.float32)[None])
        self.absolute_poses.append(np.eye(4, dtype=np.float64))
        self._iter += 1

    def _key_frame(self, pose: np.ndarray, decided=None) -> bool:
        """`__update_map`'s decision for `pose` (:360-380) — `decided`: the library has taken it — and what it leaves in
        `_delta_since_map_update`."""
        if decided is None:
            key_frame, new_delta = key_frame_decision(self._delta_since_map_update, pose, self._register_threshold_trans,
                                                      self._register_threshold_rot)
        else:
            key_frame = bool(decided)
            new_delta = None if key_frame else (self._delta_since_map_update @ pose).astype(np.float32)
        self._delta_since_map_update = np.eye(4, dtype=np.float32) if key_frame else new_delta
        return key_frame

    def _frame_done(self, data_dict: dict, res: RegisterResult, odometry_pc, device_rows=None):
        """A registered frame is in the map: the pose chains (:200-202), the dict's outputs (:243-244), the aggregated map."""
        self.last_result = res
        pose = res.pose
        self.relative_poses.append(pose[None].copy())
        self.absolute_poses.append(self.absolute_poses[-1].dot(build_pose_matrix(res.params.astype(np.float64), np.float64)))
        data_dict[self.pointcloud_key()] = odometry_pc
        data_dict[self.relative_pose_key()] = pose.reshape(4, 4).copy()
        self._aggregate(data_dict, device_rows)
        self._iter += 1

    def _one_call_next_frame(self, data_dict: dict):
        """`one_call_frame` / `one_call_projective_frame`: the frame through ONE pair of library calls (icp_frame_launch +
        icp_frame_end, or icp_pmap_frame_launch + icp_pmap_frame_end; `_OneCallKdTree` / `_OneCallProjective` say what differs).
        The library uploads a numpy frame, projects (or transposes a vertex map into target rows), stages, copies out
        `odometry_pc`, registers from `init_rpose`, applies the key-frame test of `__update_map` and updates the map; what
        stays here is the pose chain and the outputs written to the dict.  The initial guess stays the dict's `init_rpose`
        (the initialisation is a module of its own in the reference, slam/slam.py:126-140), handed over explicitly with every
        frame: the library's own constant-velocity mode (the guess read on the device) is for callers without such a module."""
        kind = self._one_call_kind
        key = self.config.data_key
        assert_debug(key in data_dict, f"Could not find the key `{key}` in the input dictionary.\n"
                                       f"With keys : {data_dict.keys()}). Set the parameter "
                                       f"`slam.odometry.data_key` to the desired key")
        data = data_dict[key]
        is_numpy = isinstance(data, np.ndarray)
        is_cuda = isinstance(data, torch.Tensor) and data.is_cuda
        is_vmap = kind.vertex_maps and is_cuda and data.ndim in (3, 4)
        assert_debug(is_numpy or is_vmap or (is_cuda and data.ndim == 2),
                     kind.refusal + f"{type(data).__name__} {tuple(getattr(data, 'shape', ()))}")
        if is_vmap:
            assert_debug(data.ndim == 3 or data.shape[0] == 1, "Unexpected batched data format.")
            assert_debug(data.shape[-3] == 3 and tuple(data.shape[-2:]) == (int(self.projector.height), int(self.projector.width)),
                         f"expected a [3, {self.projector.height}, {self.projector.width}] vertex map, got {tuple(data.shape)}")
        else:
            assert_debug(data.ndim == 2 and data.shape[1] == 3, f"expected [N, 3], got {tuple(data.shape)}")
        if is_numpy:
            self._sample_pointcloud = True  # sticky (:330)
        targets = 0 if self._sample_pointcloud else 1  # sample_points :301-308 (a vertex map's targets are its pixels anyway)
        want_rows = "distorted" not in data_dict  # (:210-213)
        # (`odometry_pc` of a numpy frame is made from the host rows the caller handed over, as on the per-call path: nothing
        # to copy back; a tensor frame's valid rows come back from the library, copied beside the registration)
        from_device = want_rows and not is_numpy
        first = self._iter == 0
        if first:
            getattr(self.ctx, kind.init)(voxel_size=0.0, threshold_trans=self._register_threshold_trans,
                                         threshold_rot=self._register_threshold_rot, constant_velocity=False, targets=targets,
                                         copy_cloud=from_device, **kind.init_extra(self, [data_dict]))
            self._one_call_targets = targets
        assert_debug(is_vmap or targets == self._one_call_targets,
                     f"{kind.flag}: numpy and tensor frames were mixed within one sequence (the targets of a "
                     "sequence are its rows or its pixels)")
        self._host_rows = None
        if is_numpy:
            self._host_rows = data if data.dtype == np.float32 and data.flags.c_contiguous else \
                np.ascontiguousarray(data, dtype=np.float32)
        frame = self._host_rows if is_numpy else data
        getattr(self.ctx, kind.launch)(frame, None, None if first else self._initial_pose(data_dict))
        host_pc = self._rows_to_host(None) if (want_rows and is_numpy and not first) else None  # GPU busy meanwhile
        res = getattr(self.ctx, kind.end)(with_points=from_device and not first)  # raises before the map is touched (:286)
        self._one_call_frame_done(kind, data_dict, res, frame, is_vmap, want_rows, host_pc)

    def _one_call_frame_done(self, kind, data_dict: dict, res, frame, is_vmap: bool, want_rows: bool, host_pc):
        """What a one-call frame leaves behind in the plugin (`MI355XICPFrameToModelBatch`: per member).  `frame`: what was
        launched; `host_pc`: `odometry_pc` where it was made from a numpy frame's own rows."""
        if res.key_frame:
            kind.record_key_frame(self, res, frame, is_vmap)
        if self._iter == 0:
            return self._first_frame_done()
        self._key_frame(res.register.pose, decided=res.key_frame)
        from_device = want_rows and not isinstance(frame, np.ndarray)
        if from_device:
            host_pc = res.points.copy() if kind.copy_points else res.points
        self._frame_done(data_dict, res.register, host_pc if want_rows else data_dict["distorted"],
                         frame if (from_device and frame.ndim == 2) else None)

    # ---- host <-> device traffic of a frame, kept off the critical path ----------------------------------------------
    def _upload(self, rows: np.ndarray) -> torch.Tensor:
        """[N,3] float32 host rows -> device tensor through a pinned staging buffer (a pageable source makes the
        runtime stage and block; pinned, the copy is one asynchronous DMA behind the previous frame's map update)."""
        n = int(rows.shape[0])
        if self.device.type != "cuda":  # (tensor placement only — the host logic is exercised without a GPU in tests/)
            return torch.from_numpy(rows).to(self.device)
        if self._pin_in is None or self._pin_in.shape[0] < n:
            self._pin_in = torch.empty((max(n, 1), 3), dtype=torch.float32, pin_memory=True)
            self._pin_in_free = None
        if self._pin_in_free is not None:
            self._pin_in_free.synchronize()  # the previous upload has left the staging buffer (long done in practice)
        stage = self._pin_in[:n]
        stage.numpy()[...] = rows
        # the DMA runs on a stream of its own, beside whatever the registration stream still has queued (the map update
        # and normal estimation enqueued behind the previous frame); the registration stream then waits for it
        if self._upload_stream is None:
            self._upload_stream = torch.cuda.Stream(device=self.device)
        main = torch.cuda.current_stream(self.device)
        # two persistent device slots, alternating: the DMA does not wait for the registration stream, so it must not
        # land in memory that work still queued there reads — the last reader of a slot is the map update enqueued two
        # frames ago, which finished before the previous registration did (and that one has been collected)
        self._dev_slot ^= 1
        slot = self._dev_in[self._dev_slot]
        if slot is None or slot.shape[0] < n:
            slot = self._dev_in[self._dev_slot] = torch.empty((max(n, 1), 3), dtype=torch.float32, device=self.device)
        dev = slot[:n]
        with torch.cuda.stream(self._upload_stream):
            dev.copy_(stage, non_blocking=True)
            self._pin_in_free = torch.cuda.Event()
            self._pin_in_free.record(self._upload_stream)
        main.wait_event(self._pin_in_free)
        return dev

    def _rows_event(self):
        """Marks, on the registration stream, the point from which the frame's device rows exist — so that their copy to
        the host can wait for THAT and not for the registration enqueued right after it."""
        if self._host_rows is not None or not self._tgt_pc.is_cuda:
            return None
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))
        return ev

    def _rows_to_host(self, ready) -> np.ndarray:
        """`odometry_pc` = the frame's points as a host array (`self._tgt_pc.cpu().numpy()`, :213; for a vertex-map frame
        its non-null pixels, :342-344; rows with a NaN removed, :357).  A numpy frame already is on the host.  A tensor
        frame is filtered on the device and copied into pinned memory on a side stream that waits for `ready` only: the
        host blocks in here while the GPU runs the registration (a numpy filter over 131 072 x 3 values took 2-3 ms per
        frame, on the critical path of the projective loop)."""
        if self._host_rows is not None:
            a = self._host_rows
            if not np.isnan(a).any():
                return a.copy()  # a fresh array per frame, like the reference's
            return a[~np.isnan(a).any(axis=1)]
        pc = self._tgt_pc
        if not pc.is_cuda:  # (tensor placement only — the host logic is exercised without a GPU in tests/)
            a = pc.numpy().reshape(-1, 3)
            keep = ~np.isnan(a).any(axis=1)
            if self._pc_is_pixels:
                keep &= np.abs(a).max(axis=1) > 0
            return a.copy() if keep.all() else a[keep]
        if self._copy_stream is None:
            self._copy_stream = torch.cuda.Stream(device=self.device)
        side = self._copy_stream
        side.wait_event(ready)
        with torch.cuda.stream(side):
            keep = ~torch.isnan(pc).any(dim=1)
            if self._pc_is_pixels:
                keep &= pc.abs().amax(dim=1) > 0
            rows = pc[keep]  # (synchronises the side stream only)
            n = int(rows.shape[0])
            if self._pin_out is None or self._pin_out.shape[0] < n:
                self._pin_out = torch.empty((max(n, 1), 3), dtype=torch.float32, pin_memory=True)
            self._pin_out[:n].copy_(rows, non_blocking=True)
            side.synchronize()
        return self._pin_out[:n].numpy().copy()

    def __update_map(self, new_rpose: np.ndarray):  # :360-380
        key_frame, new_delta = key_frame_decision(self._delta_since_map_update, new_rpose, self._register_threshold_trans,
                                                  self._register_threshold_rot)
        if key_frame:
            if self._projective:  # the projective map takes the vertex map (local_map.py:122-131)
                self.local_map.update(new_rpose, new_vertex_map=self._tgt_vmap.unsqueeze(0))
                self._delta_since_map_update = np.eye(4, dtype=np.float32)
                return
            # vertex-map input: `_tgt_pc` = the non-null pixels (:342-344) -> null rows are dropped inside the library
            if getattr(self, "_staged", False):
                self.local_map.update(new_rpose, staged=True)
            else:
                self.local_map.update(new_rpose, new_pc_data=self._tgt_pc, skip_null=self._pc_is_pixels)
            self._delta_since_map_update = np.eye(4, dtype=np.float32)
        else:
            self.local_map.update(new_rpose)
            self._delta_since_map_update = new_delta

    def get_relative_poses(self) -> Optional[np.ndarray]:  # :310-314
        self._warn_handoff_fallbacks()  # (the runner collects the trajectory at the end of a sequence)
        if len(self.relative_poses) == 0:
            return None
        return np.concatenate(self.relative_poses, axis=0)


# ----------------------------------------------------------------------------------------------------------------------
class MI355XICPFrameToModelBatch:
    """B independent sequences of `MI355XICPFrameToModel` (point-to-plane) advanced together: one call takes the next
    frame of every sequence, registers all of them together (`IcpBatch`) and updates all B local maps with one call.
    Per sequence the same poses, iteration counts, losses, steps and maps, bit for bit, as `MI355XICPFrameToModel` on the
    same frames (ICPFrameToModel.do_process_next_frame, slam/odometry/icp_odometry.py:157-246; __update_map :360-380).

    kd-tree style map (kdtree_local_map / hashgrid_local_map): one launch per ICP iteration for all B registrations and
    one `map_update_staged` — key-frame insertion, eviction, grid rebuild and eager normals; the frames' rows are staged by
    one `stage` call (two launches).  Per member still: the frame-0 insertion of the vertex map.

    Projective map (projective_local_map, local_map.py:91-240): frame 0 is one batched insertion; every later frame is one
    `pmap_register_launch` (three launches per ICP iteration for all B, every iteration enqueued) and one `pmap_update`
    (four launches: the vertex maps of the members that take a key frame, the model rebuild of every member).

    Both maps: [N,3] device frames are projected by ONE `project_rows` call (two launches) for all members; the rest of
    `_read_input` runs per member.  [3,H,W] / [1,3,H,W] vertex maps take `_read_input` per member.  `MI355XPreprocessingBatch`
    prepares the B frames in front of it in one call.

    Input: torch tensors (device-resident preprocessing, or [3,H,W] / [1,3,H,W] vertex maps).

    `MI355XICPConfig.one_call_frame=True` (kd-tree style map): the step goes through `IcpBatch.frame_launch` / `frame_end`
    instead (`_process_one_call`): numpy [N, 3] or cuda [N, 3] frames, the same poses, clouds and maps, bit for bit."""

    def __init__(self, config: MI355XICPConfig, count: int, projector=None, device=None, **kwargs):
        assert_debug(int(count) >= 1, "a batch needs at least one sequence")
        self.members = [MI355XICPFrameToModel(config, projector=projector, device=device, **kwargs) for _ in range(int(count))]
        m0 = self.members[0]
        self.config = m0.config
        assert_debug(not m0._point_to_point, "MI355XICPFrameToModelBatch batches the point-to-plane alignment only "
                                             "(point_to_plane_gauss_newton), not point-to-point")
        self.batch = IcpBatch([m.ctx for m in self.members])
        self.device = m0.device
        self._iter = 0
        self.elapsed: list = []
        # `one_call_frame`: a step is ONE pair of library calls for all members (icp_batch_frame_launch + icp_batch_frame_end)
        # instead of the calls of _process below.  The members were built with the flag, so each has already refused what the
        # frame calls do not cover (the projective map, compact_sparse_vertex_map); here they are only containers of the
        # sequences' outputs
        self._one_call = bool(_get(self.config, "one_call_frame", False))
        self._one_call_targets = None
        if self._one_call:
            assert_debug(hasattr(self.batch, "frame_launch"), "one_call_frame needs the library's batched frame calls")
        # `one_call_projective_frame`: the same for the projective map (icp_batch_pmap_frame_launch + icp_batch_pmap_frame_end);
        # the members were built with the flag and have refused a kd-tree style map
        self._one_call_pmap = bool(_get(self.config, "one_call_projective_frame", False))
        if self._one_call_pmap:
            assert_debug(hasattr(self.batch, "pmap_frame_launch"),
                         "one_call_projective_frame needs the library's batched projective frame calls")
        self._one_call_kind = m0._one_call_kind

    def __len__(self):
        return len(self.members)

    def init(self):
        for m in self.members:
            m.init()
        self._iter = 0
        self.elapsed = []

    def get_relative_poses(self, b: int) -> Optional[np.ndarray]:
        return self.members[b].get_relative_poses()

    def get_elapsed(self) -> float:
        return sum(self.elapsed)

    def process_next_frames(self, data_dicts):
        """`data_dicts[b]`: the next frame of sequence b (its preprocessed points under `config.data_key` as a torch tensor,
        its initial estimate under `init_rpose` as for the single plugin); fills `odometry_pose` and `odometry_pc` of every
        dict, as MI355XICPFrameToModel.process_next_frame does."""
        beginning = time.time()
        if self._one_call_kind is not None:
            self._process_one_call(data_dicts)
        else:
            self._process(data_dicts)
        self.elapsed.append(time.time() - beginning)

    def _process_one_call(self, data_dicts):
        """`one_call_frame` / `one_call_projective_frame`: the step through ONE pair of batched library calls
        (icp_batch_frame_launch + icp_batch_frame_end, or their icp_batch_pmap_ counterparts) — per member what
        `MI355XICPFrameToModel._one_call_next_frame` does with the single calls: the library uploads numpy frames (ONE pinned
        buffer and ONE copy for all members), projects, stages, registers from every dict's `init_rpose`, applies the key-frame
        tests and updates the maps; what stays here are the pose chains and the dicts' outputs.  numpy [N, 3] frames (not
        accepted on the per-call path), cuda [N, 3] frames and — projective map — cuda [3, H, W] / [1, 3, H, W] frames, all
        members alike.  A member whose registration fails raises `InvalidJacobianError` after the other members have completed
        their frame (their dicts and pose lists are filled)."""
        kind = self._one_call_kind
        members = self.members
        assert_debug(len(data_dicts) == len(members), f"expected {len(members)} frames, got {len(data_dicts)}")
        key = self.config.data_key
        for d in data_dicts:
            assert_debug(key in d, f"Could not find the key `{key}` in the input dictionary.")
        frames = [d[key] for d in data_dicts]
        is_numpy = all(isinstance(f, np.ndarray) for f in frames)
        is_cuda = all(isinstance(f, torch.Tensor) and f.is_cuda for f in frames)
        is_vmap = kind.vertex_maps and is_cuda and all(f.ndim in (3, 4) for f in frames)
        assert_debug(is_numpy or is_vmap or (is_cuda and all(f.ndim == 2 for f in frames)),
                     kind.refusal_batch + f"{[(type(f).__name__, tuple(getattr(f, 'shape', ()))) for f in frames]}")
        if not is_vmap:
            for f in frames:
                assert_debug(f.ndim == 2 and f.shape[1] == 3, f"expected [N, 3], got {tuple(f.shape)}")
        if is_numpy:
            for m in members:
                m._sample_pointcloud = True  # sticky (:330)
        targets = 0 if members[0]._sample_pointcloud else 1  # sample_points :301-308
        want = ["distorted" not in d for d in data_dicts]  # (:210-213)
        first = self._iter == 0
        if first:
            self.batch.use_torch_stream()
            getattr(self.batch, kind.init)(voxel_size=0.0, threshold_trans=members[0]._register_threshold_trans,
                                           threshold_rot=members[0]._register_threshold_rot, constant_velocity=False,
                                           targets=targets, copy_cloud=any(want) and not is_numpy,
                                           **kind.init_extra(members[0], data_dicts))
            self._one_call_targets = targets
        assert_debug(is_vmap or targets == self._one_call_targets,
                     f"{kind.flag}: numpy and tensor frames were mixed within one sequence (the targets of a "
                     "sequence are its rows or its pixels)")
        if is_numpy:
            frames = [f if f.dtype == np.float32 and f.flags.c_contiguous else np.ascontiguousarray(f, dtype=np.float32)
                      for f in frames]
        else:
            self.batch.use_torch_stream()
        getattr(self.batch, kind.launch)(frames, None,
                                         None if first else [m._initial_pose(d) for m, d in zip(members, data_dicts)])
        pcs = [None] * len(members)
        if is_numpy and not first:  # (`odometry_pc` of a numpy frame is made from the host rows: GPU busy meanwhile)
            for b, (m, f, w) in enumerate(zip(members, frames, want)):
                m._host_rows = f
                pcs[b] = m._rows_to_host(None) if w else None
        error = None
        try:
            results = getattr(self.batch, kind.end)(with_points=[w and not is_numpy and not first for w in want])
        except InvalidJacobianError as e:  # (raised behind the step: the healthy members have completed their frame)
            error, results = e, e.results
        for m, res, d, f, w, pc in zip(members, results, data_dicts, frames, want, pcs):
            if res is not None:
                m._one_call_frame_done(kind, d, res, f, is_vmap, w, pc)
        self._iter += 1
        if error is not None:
            raise error

    def _process(self, data_dicts):
        members = self.members
        assert_debug(len(data_dicts) == len(members), f"expected {len(members)} frames, got {len(data_dicts)}")
        key = self.config.data_key
        for d in data_dicts:
            assert_debug(key in d, f"Could not find the key `{key}` in the input dictionary.")
            assert_debug(isinstance(d[key], torch.Tensor),
                         "MI355XICPFrameToModelBatch takes torch tensors (device-resident preprocessing), not numpy input")
        self.batch.use_torch_stream()
        frames = [d[key] for d in data_dicts]
        if all(f.ndim == 2 and f.is_cuda for f in frames):
            # [N, 3] device frames: ONE projection call for all members (two launches), rows where a member's targets are
            # the pixels of its vertex map (sample_points), the rest of _read_input per member
            pcs = [f.to(self.device, torch.float32).contiguous() for f in frames]
            projected = self.batch.project_rows(pcs, rows=[not m._sample_pointcloud for m in members])
            for m, d, pr in zip(members, data_dicts, projected):
                m._read_input(d, projected=pr)
        else:
            for m, d in zip(members, data_dicts):
                m._read_input(d)  # vertex maps: as the single plugin
        if members[0]._projective:
            self._process_projective(data_dicts)
            return
        if self._iter == 0:
            for m in members:  # :176
                m.local_map.update(np.eye(4, dtype=np.float32), new_vertex_map=m._tgt_vmap.unsqueeze(0))
                m._first_frame_done()
            self._iter += 1
            return
        inits = [m._initial_pose(d) for m, d in zip(members, data_dicts)]
        sampled = [m.sample_points() for m in members]
        assert_debug(len({s for _, s in sampled}) == 1 and len({m._pc_is_pixels for m in members}) == 1,
                     "the frames of one batched call must be all point clouds or all vertex maps")
        # the frames go into the maps right after their registration (:229-231): compacted and counted in front of it
        self.batch.stage([m._tgt_pc.reshape(-1, 3) for m in members], skip_null=members[0]._pc_is_pixels)
        want = ["distorted" not in d for d in data_dicts]
        ready = [m._rows_event() if w else None for m, w in zip(members, want)]
        self.batch.register_launch([t for t, _ in sampled], inits, skip_null=sampled[0][1])
        pcs = [m._rows_to_host(r) if w else d["distorted"] for m, r, w, d in zip(members, ready, want, data_dicts)]
        results = self.batch.register_end()  # raises before a map is touched (:286)
        # the key-frame decisions, each with __update_map's own arithmetic (:360-380)
        insert = [m._key_frame(res.pose) for m, res in zip(members, results)]
        inserted = self.batch.map_update_staged(insert, [res.pose for res in results])
        for m, res, d, pc, ins, key_frame in zip(members, results, data_dicts, pcs, inserted, insert):
            if key_frame:
                m.local_map._last_count = ins
            m._frame_done(d, res, pc, m._tgt_pc if ("distorted" not in d and m._tgt_pc.is_cuda and not m._pc_is_pixels) else None)
        self._iter += 1

    def _process_projective(self, data_dicts):
        """The projective-map frame of every member (MI355XICPFrameToModel.do_process_next_frame with `_projective`)."""
        members = self.members
        ks = members[0].local_map.normals_kernel_size
        if self._iter == 0:  # :176 — every member's first vertex map, one batched insertion
            self.batch.pmap_update([np.eye(4, dtype=np.float32)] * len(members), [m._tgt_vmap for m in members], ks)
            for m in members:
                m.local_map._last_vmap = m._tgt_vmap
                m._first_frame_done()
            self._iter += 1
            return
        inits = [m._initial_pose(d) for m, d in zip(members, data_dicts)]
        sampled = [m.sample_points() for m in members]
        assert_debug(len({s for _, s in sampled}) == 1,
                     "the frames of one batched call must be all point clouds or all vertex maps")
        want = ["distorted" not in d for d in data_dicts]
        ready = [m._rows_event() if w else None for m, w in zip(members, want)]
        self.batch.pmap_register_launch([t for t, _ in sampled], inits, skip_null=sampled[0][1])
        pcs = [m._rows_to_host(r) if w else d["distorted"] for m, r, w, d in zip(members, ready, want, data_dicts)]
        results = self.batch.register_end()  # raises before a map is touched (:286)
        # the key-frame decisions, each with __update_map's own arithmetic (:360-380)
        vmaps = [m._tgt_vmap if m._key_frame(res.pose) else None for m, res in zip(members, results)]
        self.batch.pmap_update([res.pose for res in results], vmaps, ks)
        for m, res, d, pc, vm in zip(members, results, data_dicts, pcs, vmaps):
            if vm is not None:
                m.local_map._last_vmap = vm
            m._frame_done(d, res, pc, m._tgt_pc if ("distorted" not in d and m._tgt_pc.is_cuda and not m._pc_is_pixels) else None)
        self._iter += 1
