"""`IcpContext`: the Python handle on one `icp_ctx` of libicp_mi355x.so.

Accepts numpy arrays (host memory, staged by the library) and torch-ROCm tensors (device memory, zero-copy through
`tensor.data_ptr()`); returns numpy arrays or torch tensors accordingly.  torch is used for device memory and streams
only — every computation happens in the HIP kernels behind the C ABI.
"""
import ctypes as C
import weakref
from dataclasses import dataclass
from typing import Optional, Tuple, Union

import numpy as np
import torch

from . import _lib
from ._lib import (COSTS, FRAME_ROWS, FRAME_VERTEX_MAP, IcpBatchFrame, IcpConfig, IcpFrameConfig, IcpFrameResult,
                   IcpLibraryError, IcpPmapFrameConfig, IcpPreprocessFrame, IcpRegisterResult, MEM_DEVICE, MEM_HOST, SCHEMES,
                   STATUS_MESSAGES, TARGETS_ALL, TARGETS_SKIP_NULL)

Array = Union[np.ndarray, torch.Tensor]
_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None)  # (device index) -> raw hipStream_t of torch's current stream


class InvalidJacobianError(RuntimeError):
    """RuntimeError("Invalid Jacobian in Gauss Newton minimization") of slam/common/optimization.py:336.  Raised by a
    registration it carries `result`: the RegisterResult up to and including the failing iteration (the library fills the
    result block and the histories before it returns the status)."""
    result = None


class ExchangeTimeoutError(RuntimeError):
    """A peer rank did not deliver its normal equations within `exchange_timeout_ms` (in-library multi-GPU exchange)."""


@dataclass
class RegisterResult:
    pose: np.ndarray  # [4,4] f32
    params: np.ndarray  # [6] f32
    iterations: int
    converged: bool
    num_targets: int
    normals_computed: int
    losses: np.ndarray  # [iterations] f64
    dx: np.ndarray  # [iterations, 6] f32


@dataclass
class FrameResult:
    """One frame of `IcpContext.frame_launch` / `frame_end` (icp_frame_result)."""
    register: RegisterResult  # frame 0: the identity, 0 iterations
    frame_index: int
    key_frame: bool           # the frame went into the map (frame 0 always does)
    samples: int              # rows behind the grid sample (no grid sample: the rows given)
    inserted: int             # rows appended to the map (0: pose-only update)
    points: Optional[np.ndarray]  # `odometry_pc`: the frame's valid rows [rows, 3] f32 (None: frame 0, or not asked for)

    @property
    def pose(self) -> np.ndarray:
        return self.register.pose

    @property
    def params(self) -> np.ndarray:
        return self.register.params


def _ptr_mem(a: Optional[Array]) -> Tuple[Optional[int], int, object]:
    """(pointer, mem kind, keep-alive object) of an [.., 3]-float32 contiguous array / tensor."""
    if a is None:
        return None, MEM_HOST, None
    if isinstance(a, torch.Tensor):
        t = a
        if t.dtype != torch.float32 or not t.is_contiguous():
            t = t.to(torch.float32).contiguous()
        if t.is_cuda:
            return t.data_ptr(), MEM_DEVICE, t
        n = t.numpy()
        return n.ctypes.data, MEM_HOST, n
    n = np.ascontiguousarray(a, dtype=np.float32)
    return n.ctypes.data, MEM_HOST, n


def _on_device(*arrays) -> bool:
    return any(isinstance(a, torch.Tensor) and a.is_cuda for a in arrays)


_FRAME_CONFIG_FIELDS = {"voxel_size": float, "threshold_trans": float, "threshold_rot": float,
                        "constant_velocity": lambda v: int(bool(v)), "targets": int, "copy_cloud": lambda v: int(bool(v)),
                        "stage_max_rows": int}
_PMAP_FRAME_CONFIG_FIELDS = {k: v for k, v in _FRAME_CONFIG_FIELDS.items() if k != "stage_max_rows"}
_PMAP_FRAME_CONFIG_FIELDS["normals_kernel_size"] = int


def _fill_config(cfg, fields, who: str, kw):
    for k, v in kw.items():
        if k not in fields:
            raise TypeError(f"{who}() got an unexpected keyword argument {k!r}")
        setattr(cfg, k, fields[k](v))
    return cfg


def _frame_config(lib, **kw) -> IcpFrameConfig:
    """icp_default_frame_config with the given fields set (`IcpContext.odometry_init` and `IcpBatch.odometry_init`)."""
    cfg = IcpFrameConfig()
    lib.icp_default_frame_config(C.byref(cfg))
    return _fill_config(cfg, _FRAME_CONFIG_FIELDS, "odometry_init", kw)


def _pmap_frame_config(lib, **kw) -> IcpPmapFrameConfig:
    """icp_default_pmap_frame_config with the given fields set (the two `pmap_odometry_init`s)."""
    cfg = IcpPmapFrameConfig()
    lib.icp_default_pmap_frame_config(C.byref(cfg))
    return _fill_config(cfg, _PMAP_FRAME_CONFIG_FIELDS, "pmap_odometry_init", kw)


def _frame_arrays(data, timestamps=None, vertex_map: bool = False, who: str = "", rows_alt: str = ""):
    """One frame as the frame calls take it: [N,3] float32 rows on the host (numpy, cpu tensor) or on the device (cuda
    tensor) with optional [N] float64 timestamps where the rows live, or — `vertex_map` — a cuda [3,H,W] / [1,3,H,W]
    vertex map.  Returns (pointer, n, mem, layout, timestamp pointer, keep); `keep` holds what the pointers point into.
    `who` / `rows_alt`: the caller's words in the messages."""
    if vertex_map:
        vm = data[0] if data.ndim == 4 else data
        if (data.ndim == 4 and data.shape[0] != 1) or vm.shape[0] != 3:
            raise AssertionError(f"{who}expected a [3,H,W] vertex map, got {tuple(data.shape)}")
        vm = vm if vm.dtype == torch.float32 and vm.is_contiguous() else vm.to(torch.float32).contiguous()
        ts = None if timestamps is None else torch.as_tensor(timestamps).to(vm.device, torch.float64)
        return vm.data_ptr(), int(vm.shape[1] * vm.shape[2]), MEM_DEVICE, FRAME_VERTEX_MAP, \
            (ts.data_ptr() if ts is not None else None), (vm, ts)
    if isinstance(data, torch.Tensor) and data.is_cuda:
        pts = data if data.dtype == torch.float32 and data.is_contiguous() else data.to(torch.float32).contiguous()
        ts = None if timestamps is None else \
            torch.as_tensor(timestamps).to(pts.device, torch.float64).reshape(-1).contiguous()
        mem, p, tp = MEM_DEVICE, pts.data_ptr(), ts.data_ptr() if ts is not None else None
    else:
        pts = data.numpy() if isinstance(data, torch.Tensor) else data
        if not (isinstance(pts, np.ndarray) and pts.dtype == np.float32 and pts.flags.c_contiguous):
            pts = np.ascontiguousarray(pts, dtype=np.float32)
        ts = None if timestamps is None else np.ascontiguousarray(np.asarray(timestamps).reshape(-1), dtype=np.float64)
        mem, p, tp = MEM_HOST, pts.ctypes.data, ts.ctypes.data if ts is not None else None
    if pts.ndim != 2 or pts.shape[1] != 3 or (ts is not None and ts.shape[0] != pts.shape[0]):
        raise AssertionError(f"{who}expected [N,3] points (and [N] timestamps){rows_alt}, got {tuple(pts.shape)}")
    n = int(pts.shape[0])
    return (p if n else None), n, mem, FRAME_ROWS, (tp if n else None), (pts, ts)


def registering_contexts(device: int = 0) -> int:
    """Contexts of this process in a registration against the kd-tree style map, or holding an uncollected result of one, on
    `device` right now (`icp_registering_contexts`; -1 outside 0..63)."""
    return int(_lib.load_library().icp_registering_contexts(int(device)))


def _pose16(m) -> "C.Array":
    a = np.ascontiguousarray(np.asarray(m, dtype=np.float32).reshape(4, 4))
    return (C.c_float * 16)(*a.reshape(-1).tolist())


class IcpContext:
    def __init__(self, height: int = 64, width: int = 1024, up_fov: float = 3.0, down_fov: float = -24.0,
                 max_num_alignments: int = 100, threshold_delta_pose: float = 1.0e-4, scheme: str = "default",
                 sigma: float = 0.5, local_map_size: int = 20, num_neighbors_normals: int = 10,
                 cell_size: float = 0.0, max_rings: int = 2, device: int = 0, poll_every: int = 4):
        self._lib = _lib.load_library()
        cfg = IcpConfig()
        self._lib.icp_default_config(C.byref(cfg))
        if scheme not in SCHEMES:
            raise AssertionError(f"unknown weighting scheme {scheme}")
        cfg.height, cfg.width, cfg.up_fov, cfg.down_fov = int(height), int(width), float(up_fov), float(down_fov)
        cfg.max_num_alignments, cfg.threshold_delta_pose = int(max_num_alignments), float(threshold_delta_pose)
        cfg.scheme, cfg.sigma = SCHEMES[scheme], float(sigma)
        cfg.local_map_size, cfg.num_neighbors_normals = int(local_map_size), int(num_neighbors_normals)
        cfg.cell_size, cfg.max_rings, cfg.device, cfg.poll_every = float(cell_size), int(max_rings), int(device), \
            int(poll_every)
        self.config = cfg
        self.device = torch.device("cuda", int(device))
        self._device_index = int(device)
        handle = C.c_void_p()
        rc = self._lib.icp_create(C.byref(cfg), C.byref(handle))
        if rc != 0:
            raise IcpLibraryError(f"icp_create failed: {STATUS_MESSAGES.get(rc, rc)}")
        self._h = handle
        self._neq_tensor: Optional[torch.Tensor] = None

    # ------------------------------------------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            for m in list(getattr(self, "_cloud_refiners", ())) + list(getattr(self, "_elevation_images", ())) + \
                    list(getattr(self, "_aggregated_maps", ())):
                m.close()  # (a refiner, an image or a map is destroyed before its context)
            self._lib.icp_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int):
        if rc == 0:
            return
        msg = self._lib.icp_last_error(self._h).decode() or STATUS_MESSAGES.get(rc, str(rc))
        if rc == _lib.ICP_ERR_INVALID_JACOBIAN:
            raise InvalidJacobianError("Invalid Jacobian in Gauss Newton minimization")
        if rc == _lib.ICP_ERR_INVALID_ARGUMENT:
            raise AssertionError(msg)
        if rc == _lib.ICP_ERR_EXCHANGE:
            raise ExchangeTimeoutError(msg)
        raise RuntimeError(f"libicp_mi355x: {msg} ({rc})")

    def use_torch_stream(self):
        """Enqueue on torch's current HIP stream of this device (the library orders a switch of streams against the work
        it enqueued on the previous one)."""
        # (the raw handle straight from torch's bookkeeping where the build exposes it: the public query builds a Stream
        # object, 3-10 us a call — and every call that takes a device tensor asks)
        stream = _RAW_STREAM(self._device_index) if _RAW_STREAM is not None else \
            torch.cuda.current_stream(self.device).cuda_stream
        if stream != getattr(self, "_bound_stream", None):
            self._check(self._lib.icp_set_stream(self._h, C.c_void_p(stream)))
            self._bound_stream = stream

    def _bind(self, *arrays):
        """Device tensors come from (and results go to) torch's current stream: make sure the library enqueues there."""
        if _on_device(*arrays):
            self.use_torch_stream()

    def synchronize(self):
        self._check(self._lib.icp_synchronize(self._h))

    def set_cost(self, mode: str):
        """Alignment mode of the registration loop: a RIGID_ALIGNMENT member name of the reference
        ("point_to_plane_gauss_newton" | "point_to_point_gauss_newton")."""
        if mode not in COSTS:
            raise AssertionError(f"unknown alignment mode {mode}")
        self._check(self._lib.icp_set_cost(self._h, COSTS[mode]))

    def set_option(self, name: str, value: float):
        """MI355X-side tuning option (see `icp_set_option` in include/icp_mi355x.h); never changes a result."""
        self._check(self._lib.icp_set_option(self._h, name.encode(), float(value)))

    def set_alignment(self, scheme: str, sigma: float, max_num_alignments: int, threshold_delta_pose: float):
        self._check(self._lib.icp_set_alignment(self._h, SCHEMES[scheme], float(sigma), int(max_num_alignments),
                                                float(threshold_delta_pose)))
        self.config.scheme, self.config.sigma = SCHEMES[scheme], float(sigma)
        self.config.max_num_alignments = int(max_num_alignments)
        self.config.threshold_delta_pose = float(threshold_delta_pose)

    # ---- projection --------------------------------------------------------------------------------------------------
    def project(self, points: Array, with_index: bool = False, out: Optional[torch.Tensor] = None):
        """Vertex map [3, H, W] (same kind as the input: numpy in -> numpy out, cuda tensor in -> cuda tensor out)."""
        self._bind(points)
        p, mem, keep = _ptr_mem(points)
        n = int(keep.shape[0]) if keep is not None else 0
        h, w = self.config.height, self.config.width
        if mem == MEM_DEVICE:
            vmap = out if out is not None else torch.empty((3, h, w), dtype=torch.float32, device=keep.device)
            idx = torch.empty((h, w), dtype=torch.int32, device=keep.device) if with_index else None
            self._check(self._lib.icp_project(self._h, p, n, mem, vmap.data_ptr(),
                                              idx.data_ptr() if idx is not None else None, MEM_DEVICE))
        else:
            vmap = np.empty((3, h, w), dtype=np.float32)
            idx = np.empty((h, w), dtype=np.int32) if with_index else None
            self._check(self._lib.icp_project(self._h, p, n, mem, vmap.ctypes.data,
                                              idx.ctypes.data if idx is not None else None, MEM_HOST))
        return (vmap, idx) if with_index else vmap

    def project_rows(self, points: torch.Tensor):
        """Device-resident projection: (vertex map [3, H, W], the same pixels as rows [H * W, 3]) from one launch — the rows
        are `vmap.permute(1, 2, 0).reshape(-1, 3)` without the transposing copy."""
        self._bind(points)
        p, mem, keep = _ptr_mem(points)
        if mem != MEM_DEVICE:
            raise AssertionError("project_rows takes a device tensor")
        h, w = self.config.height, self.config.width
        vmap = torch.empty((3, h, w), dtype=torch.float32, device=keep.device)
        rows = torch.empty((h * w, 3), dtype=torch.float32, device=keep.device)
        self._check(self._lib.icp_project_rows(self._h, p, int(keep.shape[0]), vmap.data_ptr(), rows.data_ptr()))
        return vmap, rows

    def project_pixels(self, points: np.ndarray):
        p, mem, keep = _ptr_mem(points)
        n = int(keep.shape[0])
        rows, cols = np.empty(n, np.float32), np.empty(n, np.float32)
        self._check(self._lib.icp_project_pixels(self._h, p, n, mem, rows.ctypes.data, cols.ctypes.data, MEM_HOST))
        return rows, cols

    def kitti_correct_scan(self, scan: np.ndarray) -> np.ndarray:
        """`KITTIOdometrySequence.correct_scan`: [N,4] (or [N,3]) float32 -> corrected xyz [N,3] float64."""
        a = np.ascontiguousarray(scan, dtype=np.float32)
        if a.ndim != 2 or a.shape[1] < 3:
            raise AssertionError(f"expected [N, >=3] rows, got {a.shape}")
        out = np.empty((a.shape[0], 3), np.float64)
        self._check(self._lib.icp_kitti_correct_scan(self._h, a.ctypes.data, int(a.shape[0]), int(a.shape[1]), MEM_HOST,
                                                     out.ctypes.data, MEM_HOST))
        return out

    # ---- grid sampling -----------------------------------------------------------------------------------------------
    def voxel_hash(self, points: np.ndarray, voxel_size: float):
        p, mem, keep = _ptr_mem(points)
        n = int(keep.shape[0])
        vox, hashes = np.empty((n, 3), np.int64), np.empty(n, np.int64)
        self._check(self._lib.icp_voxel_hash(self._h, p, n, mem, float(voxel_size), vox.ctypes.data,
                                             hashes.ctypes.data, MEM_HOST))
        return vox, hashes

    def grid_sample(self, points: Array, voxel_size: float):
        """(sample points [V,3], indices [V] int64), ordered by ascending voxel hash."""
        self._bind(points)
        p, mem, keep = _ptr_mem(points)
        n = int(keep.shape[0])
        count = C.c_int64(0)
        if mem == MEM_DEVICE:
            idx = torch.empty(max(n, 1), dtype=torch.int64, device=keep.device)
            pts = torch.empty((max(n, 1), 3), dtype=torch.float32, device=keep.device)
            self._check(self._lib.icp_grid_sample(self._h, p, n, mem, float(voxel_size), idx.data_ptr(),
                                                  pts.data_ptr(), C.byref(count), MEM_DEVICE))
            return pts[:count.value], idx[:count.value]
        idx = np.empty(max(n, 1), np.int64)
        pts = np.empty((max(n, 1), 3), np.float32)
        self._check(self._lib.icp_grid_sample(self._h, p, n, mem, float(voxel_size), idx.ctypes.data,
                                              pts.ctypes.data, C.byref(count), MEM_HOST))
        return pts[:count.value].copy(), idx[:count.value].copy()

    def grid_sample_padded(self, points: "torch.Tensor", voxel_size: float):
        """The grid sample of the device-resident pipeline (`icp_grid_sample_padded[_f64]`): a cuda tensor in, and —
        without any synchronisation — (points [n,3] with the V samples first and NaN rows behind them, indices [n] int64
        with -1 behind the samples, V as a 0-dim int32 cuda tensor) out."""
        self._bind(points)
        if not (isinstance(points, torch.Tensor) and points.is_cuda):
            raise AssertionError("grid_sample_padded takes a cuda tensor (the device-resident pipeline)")
        f64 = points.dtype == torch.float64
        t = points.contiguous() if f64 else points.to(torch.float32).contiguous()
        n = int(t.shape[0])
        idx = torch.empty(max(n, 1), dtype=torch.int64, device=t.device)
        out = torch.empty((max(n, 1), 3), dtype=t.dtype, device=t.device)
        count = torch.empty((), dtype=torch.int32, device=t.device)
        fn = self._lib.icp_grid_sample_padded_f64 if f64 else self._lib.icp_grid_sample_padded
        self._check(fn(self._h, t.data_ptr(), n, float(voxel_size), idx.data_ptr(), out.data_ptr(), count.data_ptr()))
        return out[:n], idx[:n], count

    def voxel_statistics(self, points: np.ndarray, voxel_size: float, with_normal_distribution: bool = True):
        """`Voxelization.filter` (slam/preprocessing.py:63-98): dict with voxel_coordinates [n,3] i64, voxel_hashes [n]
        i64, voxel_indices [n] i64 and — with_normal_distribution — voxel_sizes [V] i64, voxel_means [V,3] f32,
        voxel_covariances [V,3,3] f32 (voxels by ascending hash)."""
        p, mem, keep = _ptr_mem(points)
        if mem != MEM_HOST:
            raise AssertionError("voxel_statistics takes a host array (the reference filter is numpy-only)")
        n = int(keep.shape[0])
        vox, hashes, ids = np.empty((n, 3), np.int64), np.empty(n, np.int64), np.empty(n, np.int64)
        nv = C.c_int64(0)
        sizes = means = covs = None
        if with_normal_distribution:
            sizes, means, covs = np.empty(n, np.int64), np.empty((n, 3), np.float32), np.empty((n, 3, 3), np.float32)
        self._check(self._lib.icp_voxel_statistics(
            self._h, p, n, mem, float(voxel_size), vox.ctypes.data, hashes.ctypes.data, ids.ctypes.data, C.byref(nv),
            sizes.ctypes.data if sizes is not None else None, means.ctypes.data if means is not None else None,
            covs.ctypes.data if covs is not None else None, MEM_HOST))
        out = {"voxel_coordinates": vox, "voxel_hashes": hashes, "voxel_indices": ids, "num_voxels": int(nv.value)}
        if with_normal_distribution:
            v = int(nv.value)
            out.update(voxel_sizes=sizes[:v].copy(), voxel_means=means[:v].copy(), voxel_covariances=covs[:v].copy())
        return out

    def grid_sample_f64(self, points: Array, voxel_size: float):
        """float64 cloud (the output of `distort`) -> (sample points [V,3] f64, indices [V] int64); a cuda tensor stays
        on the device (zero-copy in, device tensors out)."""
        self._bind(points)
        count = C.c_int64(0)
        if isinstance(points, torch.Tensor) and points.is_cuda:
            t = points.to(torch.float64).contiguous()
            n = int(t.shape[0])
            idx = torch.empty(max(n, 1), dtype=torch.int64, device=t.device)
            out = torch.empty((max(n, 1), 3), dtype=torch.float64, device=t.device)
            self._check(self._lib.icp_grid_sample_f64(self._h, t.data_ptr(), n, MEM_DEVICE, float(voxel_size),
                                                      idx.data_ptr(), out.data_ptr(), C.byref(count), MEM_DEVICE))
            return out[:count.value], idx[:count.value]
        pts64 = np.ascontiguousarray(points, dtype=np.float64)
        n = int(pts64.shape[0])
        idx = np.empty(max(n, 1), np.int64)
        out = np.empty((max(n, 1), 3), np.float64)
        self._check(self._lib.icp_grid_sample_f64(self._h, pts64.ctypes.data, n, MEM_HOST, float(voxel_size),
                                                  idx.ctypes.data, out.ctypes.data, C.byref(count), MEM_HOST))
        return out[:count.value].copy(), idx[:count.value].copy()

    # ---- de-skew -----------------------------------------------------------------------------------------------------
    def distort(self, points: Array, timestamps: Array, rel_pose):
        """`Distortion.filter`: [N,3] f32 points + [N] f64 timestamps + 4x4 initial motion -> [N,3] f64.  cuda tensors in
        -> cuda tensor out (nothing crosses PCIe but the 4x4 pose)."""
        self._bind(points)
        pose = np.ascontiguousarray(np.asarray(rel_pose, dtype=np.float64).reshape(4, 4))
        if isinstance(points, torch.Tensor) and points.is_cuda:
            pts = points.to(torch.float32).contiguous()
            ts = torch.as_tensor(timestamps).to(pts.device, torch.float64).reshape(-1).contiguous()
            if pts.ndim != 2 or pts.shape[1] != 3 or ts.shape[0] != pts.shape[0]:
                raise AssertionError(f"expected [N,3] points and [N] timestamps, got {tuple(pts.shape)} / {tuple(ts.shape)}")
            out = torch.empty((pts.shape[0], 3), dtype=torch.float64, device=pts.device)
            self._check(self._lib.icp_distort(self._h, pts.data_ptr(), ts.data_ptr(), int(pts.shape[0]), MEM_DEVICE,
                                              pose.ctypes.data, out.data_ptr(), MEM_DEVICE))
            return out
        pts = np.ascontiguousarray(points, dtype=np.float32)
        ts = np.ascontiguousarray(np.asarray(timestamps).reshape(-1), dtype=np.float64)
        if pts.ndim != 2 or pts.shape[1] != 3 or ts.shape[0] != pts.shape[0]:
            raise AssertionError(f"expected [N,3] points and [N] timestamps, got {pts.shape} / {ts.shape}")
        out = np.empty((pts.shape[0], 3), np.float64)
        self._check(self._lib.icp_distort(self._h, pts.ctypes.data, ts.ctypes.data, int(pts.shape[0]), MEM_HOST,
                                          pose.ctypes.data, out.ctypes.data, MEM_HOST))
        return out

    # ---- time stamps from the azimuth --------------------------------------------------------------------------------
    @staticmethod
    def _scan_rows(rows, what: str):
        """[N, 3] or [N, 4] float32 contiguous rows, numpy or cuda tensor (another dtype / layout is converted here)."""
        if isinstance(rows, torch.Tensor) and rows.is_cuda:
            a = rows if (rows.dtype == torch.float32 and rows.is_contiguous()) else rows.to(torch.float32).contiguous()
        else:
            a = np.ascontiguousarray(rows.detach().cpu().numpy() if isinstance(rows, torch.Tensor) else rows,
                                     dtype=np.float32)
        if a.ndim != 2 or a.shape[1] not in (3, 4):
            raise AssertionError(f"{what}: expected [N, 3] or [N, 4] rows, got {tuple(a.shape)}")
        return a

    def estimate_timestamps(self, rows: Array, clockwise: bool = True, phi_0: float = 0.0):
        """`estimate_timestamps` (slam/common/geometry.py:443-466): [N, 3] (or the [N, 4] records of a .bin scan) float32
        rows -> [N] float64 time stamps in [0, 1] from the azimuth.  numpy in -> numpy out; a cuda tensor in -> a cuda
        tensor out on torch's current stream, without a synchronisation: what `frame_launch(timestamps=...)`, `distort`
        and `IcpBatch.preprocess` take.  Arithmetic, seam and NaN cases: `icp_estimate_timestamps`, include/icp_mi355x.h."""
        self._bind(rows)
        a = self._scan_rows(rows, "estimate_timestamps")
        n, stride = int(a.shape[0]), int(a.shape[1])
        if isinstance(a, torch.Tensor):
            out = torch.empty(n, dtype=torch.float64, device=a.device)
            self._check(self._lib.icp_estimate_timestamps(self._h, a.data_ptr() if n else None, n, stride, MEM_DEVICE,
                                                          int(bool(clockwise)), float(phi_0), out.data_ptr(), MEM_DEVICE))
            return out
        out = np.empty(n, np.float64)
        self._check(self._lib.icp_estimate_timestamps(self._h, a.ctypes.data, n, stride, MEM_HOST, int(bool(clockwise)),
                                                      float(phi_0), out.ctypes.data, MEM_HOST))
        return out

    def kitti360_prepare(self, scan: Array, clockwise: bool = True, phi_0: float = np.pi):
        """`KITTI360Sequence.__getitem__` (slam/dataset/kitti_360_dataset.py:170-185) for one raw scan, from one upload and
        one read of it: (xyz [N, 3] float64 — the bits of `kitti_correct_scan` —, time stamps [N] float64 — the bits of
        `estimate_timestamps(scan, clockwise, phi_0)`).  numpy in -> numpy out, cuda tensor in -> cuda tensors out."""
        self._bind(scan)
        a = self._scan_rows(scan, "kitti360_prepare")
        n, stride = int(a.shape[0]), int(a.shape[1])
        if isinstance(a, torch.Tensor):
            xyz = torch.empty((n, 3), dtype=torch.float64, device=a.device)
            ts = torch.empty(n, dtype=torch.float64, device=a.device)
            self._check(self._lib.icp_kitti360_prepare(self._h, a.data_ptr() if n else None, n, stride, MEM_DEVICE,
                                                       int(bool(clockwise)), float(phi_0), xyz.data_ptr(), ts.data_ptr(),
                                                       MEM_DEVICE))
            return xyz, ts
        xyz, ts = np.empty((n, 3), np.float64), np.empty(n, np.float64)
        self._check(self._lib.icp_kitti360_prepare(self._h, a.ctypes.data, n, stride, MEM_HOST, int(bool(clockwise)),
                                                   float(phi_0), xyz.ctypes.data, ts.ctypes.data, MEM_HOST))
        return xyz, ts

    # ---- local map ---------------------------------------------------------------------------------------------------
    def map_init(self):
        self._check(self._lib.icp_map_init(self._h))

    def map_set(self, points: Array):
        self._bind(points)
        p, mem, keep = _ptr_mem(points)
        self._check(self._lib.icp_map_set(self._h, p, int(keep.shape[0]), mem))

    def map_update(self, rel_pose, new_points: Optional[Array] = None, skip_null: bool = False) -> int:
        self._bind(new_points)
        p, mem, keep = _ptr_mem(new_points)
        n = int(keep.shape[0]) if keep is not None else 0
        if keep is not None and n == 0:
            # an empty cloud still counts as a cloud in the reference's bookkeeping; give the library a valid pointer
            keep = np.zeros((1, 3), np.float32)
            p = keep.ctypes.data
            mem = MEM_HOST
        ins = C.c_int64(0)
        # rel_pose None: the device-resident pose of the last registration (no host round trip)
        self._check(self._lib.icp_map_update(self._h, _pose16(rel_pose) if rel_pose is not None else None, p, n, mem,
                                             TARGETS_SKIP_NULL if skip_null else TARGETS_ALL, C.byref(ins)))
        return int(ins.value)

    def map_stage_cloud(self, new_points: Array, skip_null: bool = False) -> None:
        """Prepares the cloud a later `map_update_staged` inserts (icp_map_stage_cloud): its valid rows are compacted on the
        device and their count is sent to the host without waiting — called before a registration, the update after it
        needs no host round trip of its own."""
        self._bind(new_points)
        p, mem, keep = _ptr_mem(new_points)
        n = int(keep.shape[0])
        self._check(self._lib.icp_map_stage_cloud(self._h, p if n else None, n, mem,
                                                  TARGETS_SKIP_NULL if skip_null else TARGETS_ALL))

    def map_update_staged(self, rel_pose) -> int:
        ins = C.c_int64(0)
        self._check(self._lib.icp_map_update_staged(self._h, _pose16(rel_pose) if rel_pose is not None else None,
                                                    C.byref(ins)))
        return int(ins.value)

    def map_update_vertex_map(self, rel_pose, vmap: Array) -> int:
        self._bind(vmap)
        p, mem, keep = _ptr_mem(vmap)
        ins = C.c_int64(0)
        self._check(self._lib.icp_map_update_vertex_map(self._h, _pose16(rel_pose), p, mem, C.byref(ins)))
        return int(ins.value)

    def map_size(self) -> int:
        return int(self._lib.icp_map_size(self._h))

    def map_num_clouds(self) -> int:
        return int(self._lib.icp_map_num_clouds(self._h))

    def handoff_fallbacks(self) -> int:
        """Registrations finished on per-iteration launches behind a timed-out hand-off (`icp_handoff_fallbacks`)."""
        return int(self._lib.icp_handoff_fallbacks(self._h))

    def lead_registrations(self) -> int:
        """Registrations of this context whose launches were latched onto lead launches when they began: no other context of
        the process was registering on the device at that moment (`icp_lead_registrations`)."""
        return int(self._lib.icp_lead_registrations(self._h))

    def first_build_launches(self) -> int:
        """Registrations whose first launch was the first-iteration build (`icp_first_build_launches`, option "first_build")."""
        return int(self._lib.icp_first_build_launches(self._h))

    def map_points(self) -> np.ndarray:
        out = np.empty((self.map_size(), 3), np.float32)
        if out.shape[0]:
            self._check(self._lib.icp_map_get(self._h, out.ctypes.data, MEM_HOST))
        return out

    def nearest_neighbor_search(self, points: Array, with_normals: bool = True, with_index: bool = False):
        self._bind(points)
        p, mem, keep = _ptr_mem(points)
        n = int(keep.shape[0])
        if mem == MEM_DEVICE:
            nb = torch.empty((n, 3), dtype=torch.float32, device=keep.device)
            nm = torch.empty((n, 3), dtype=torch.float32, device=keep.device) if with_normals else None
            ix = torch.empty(n, dtype=torch.int32, device=keep.device) if with_index else None
            self._check(self._lib.icp_nearest_neighbor_search(
                self._h, p, n, mem, nb.data_ptr(), nm.data_ptr() if nm is not None else None,
                ix.data_ptr() if ix is not None else None, MEM_DEVICE))
        else:
            nb = np.empty((n, 3), np.float32)
            nm = np.empty((n, 3), np.float32) if with_normals else None
            ix = np.empty(n, np.int32) if with_index else None
            self._check(self._lib.icp_nearest_neighbor_search(
                self._h, p, n, mem, nb.ctypes.data, nm.ctypes.data if nm is not None else None,
                ix.ctypes.data if ix is not None else None, MEM_HOST))
        return nb, nm, ix

    def knn_query(self, points: Array, k: int = 1, distance_upper_bound: Optional[float] = None, sqr_dists: bool = False):
        """`pykdtree.kdtree.KDTree(map).query(points, k)` (slam/odometry/local_map.py:369,385,405) against the map of this
        context: the exact k nearest map points of every row of `points` [n, 3] (`icp_knn_query`; k = 1..32).  Returns
        (dist [n, k] float32, index [n, k] int32): ascending by (distance, map index), indices in `map_points()` order;
        `sqr_dists` returns the squared distances.  `distance_upper_bound` = b keeps neighbours with d2 < b * b only.  Entries
        without a neighbour (fewer than k points within reach, a non-finite query row) are (+inf, `map_size()`).
        numpy in -> numpy out, cuda tensor in -> cuda tensors out."""
        self._bind(points)
        p, mem, keep = _ptr_mem(points)
        if keep.ndim != 2 or keep.shape[1] != 3:
            raise AssertionError(f"knn_query: expected [n, 3] points, got {tuple(keep.shape)}")
        n, k = int(keep.shape[0]), int(k)
        bound = 0.0 if distance_upper_bound is None else float(distance_upper_bound)
        if bound != bound or bound < 0.0:
            raise AssertionError(f"knn_query: distance_upper_bound = {distance_upper_bound} is not a distance")
        flags = _lib.KNN_SQR_DISTS if sqr_dists else 0
        cols = max(k, 0)  # (k < 1 is the library's to refuse: it looks at k first)
        # (one row at least: an empty array has no address, and the library tells an output from its absence by it)
        if mem == MEM_DEVICE:
            dist = torch.empty((max(n, 1), cols), dtype=torch.float32, device=keep.device)
            index = torch.empty((max(n, 1), cols), dtype=torch.int32, device=keep.device)
            dp, ip = dist.data_ptr(), index.data_ptr()
        else:
            dist, index = np.empty((max(n, 1), cols), np.float32), np.empty((max(n, 1), cols), np.int32)
            dp, ip = dist.ctypes.data, index.ctypes.data
        dist, index = dist[:n], index[:n]
        self._check(self._lib.icp_knn_query(self._h, p if n else None, n, mem, k, bound, flags, dp, ip, mem))
        return dist, index

    def last_neighbors(self, n: int):
        """(original map index per target, [3,4] pose) of the LAST iteration of the last registration, read back from the
        library's exact nearest-neighbour cache (test support: `icp_last_neighbors`)."""
        ix = np.empty(int(n), np.int32)  # n = the number of target rows of that registration
        pose = np.empty(12, np.float32)
        self._check(self._lib.icp_last_neighbors(self._h, ix.ctypes.data, pose.ctypes.data, MEM_HOST))
        return ix, pose.reshape(3, 4)

    def last_cache_entries(self, n: int, records: bool = False):
        """The NN-cache entry of every target of the last registration (test support: `icp_last_cache_entries`): a dict of
        `members` [n, 3] original map indices (the stored neighbour first, -1: none), `bound` [n] (L), `iteration` [n] (of
        the search, -1: no entry), `pose_hist` [last + 1, 3, 4], `last`, and with `records` the raw `records` [n, 8]."""
        last = C.c_int32(-1)
        self._check(self._lib.icp_last_cache_entries(self._h, None, None, None, None, None, C.byref(last), MEM_HOST))
        n = int(n)
        members, bound = np.empty((n, 3), np.int32), np.empty(n, np.float32)
        iteration, hist = np.empty(n, np.int32), np.empty((last.value + 1, 12), np.float32)
        rec = np.empty((n, 8), np.float32) if records else None
        self._check(self._lib.icp_last_cache_entries(self._h, members.ctypes.data, bound.ctypes.data, iteration.ctypes.data,
                                                     rec.ctypes.data if records else None, hist.ctypes.data, C.byref(last),
                                                     MEM_HOST))
        out = {"members": members, "bound": bound, "iteration": iteration, "pose_hist": hist.reshape(-1, 3, 4),
               "last": int(last.value)}
        if records:
            out["records"] = rec
        return out

    # ---- projective local map --------------------------------------------------------------------
    def _planar(self, vmap: Array):
        """[3,H,W] float32 contiguous -> (pointer, mem, keep-alive)."""
        h, w = self.config.height, self.config.width
        if isinstance(vmap, torch.Tensor):
            t = vmap.to(torch.float32).contiguous()
            if tuple(t.shape[-3:]) != (3, h, w):
                raise AssertionError(f"expected a [3,{h},{w}] vertex map, got {tuple(t.shape)}")
            if t.is_cuda:
                return t.data_ptr(), MEM_DEVICE, t
            a = t.numpy()
            return a.ctypes.data, MEM_HOST, a
        a = np.ascontiguousarray(vmap, dtype=np.float32)
        if a.shape[-3:] != (3, h, w):
            raise AssertionError(f"expected a [3,{h},{w}] vertex map, got {a.shape}")
        return a.ctypes.data, MEM_HOST, a

    def compute_normal_map(self, vmap: Array, kernel_size: int = 5):
        p, mem, keep = self._planar(vmap)
        h, w = self.config.height, self.config.width
        if mem == MEM_DEVICE:
            out = torch.empty((3, h, w), dtype=torch.float32, device=keep.device)
            self._check(self._lib.icp_compute_normal_map(self._h, p, mem, int(kernel_size), out.data_ptr(), MEM_DEVICE))
            return out
        out = np.empty((3, h, w), np.float32)
        self._check(self._lib.icp_compute_normal_map(self._h, p, mem, int(kernel_size), out.ctypes.data, MEM_HOST))
        return out

    def compute_neighbors(self, vm_target: np.ndarray, vm_reference: np.ndarray,
                          reference_fields: Optional[np.ndarray] = None):
        h, w = self.config.height, self.config.width
        t = np.ascontiguousarray(vm_target, dtype=np.float32).reshape(3, h, w)
        r = np.ascontiguousarray(vm_reference, dtype=np.float32).reshape(-1, 3, h, w)
        k = r.shape[0]
        f = fo = None
        c = 0
        if reference_fields is not None:
            f = np.ascontiguousarray(reference_fields, dtype=np.float32).reshape(k, -1, h, w)
            c = f.shape[1]
            fo = np.empty((c, h, w), np.float32)
        nb = np.empty((3, h, w), np.float32)
        self._check(self._lib.icp_compute_neighbors(self._h, t.ctypes.data, r.ctypes.data,
                                                    f.ctypes.data if f is not None else None, k, c, MEM_HOST,
                                                    nb.ctypes.data, fo.ctypes.data if fo is not None else None,
                                                    MEM_HOST))
        return nb, fo

    def pmap_init(self):
        self._check(self._lib.icp_pmap_init(self._h))

    def pmap_update(self, rel_pose, vmap: Optional[Array] = None, normals_kernel_size: int = 5):
        if vmap is None:
            self._check(self._lib.icp_pmap_update(self._h, _pose16(rel_pose), None, MEM_HOST, int(normals_kernel_size)))
            return
        p, mem, keep = self._planar(vmap)
        self._check(self._lib.icp_pmap_update(self._h, _pose16(rel_pose), p, mem, int(normals_kernel_size)))

    def pmap_num_maps(self) -> int:
        return int(self._lib.icp_pmap_num_maps(self._h))

    def pmap_model(self):
        """(`_model_vmap` [K,3,H,W], `_model_nmap` [K,3,H,W]) as numpy arrays."""
        k, h, w = self.pmap_num_maps(), self.config.height, self.config.width
        v4 = np.empty((k, h * w, 4), np.float32)
        n4 = np.empty((k, h * w, 4), np.float32)
        if k:
            self._check(self._lib.icp_pmap_get_model(self._h, v4.ctypes.data, n4.ctypes.data, MEM_HOST))
        to_maps = lambda a: np.ascontiguousarray(a[:, :, :3].reshape(k, h, w, 3).transpose(0, 3, 1, 2))
        return to_maps(v4), to_maps(n4)

    def pmap_nearest_neighbor_search(self, points: Array):
        """(neighbour points, neighbour normals, new target points), each [n,3], matched pixels in pixel order; cuda
        tensors for cuda points, numpy arrays otherwise."""
        self._bind(points)
        p, mem, keep = _ptr_mem(points)
        n = int(keep.shape[0])
        npix = self.config.height * self.config.width
        count = C.c_int64(0)
        if mem == MEM_DEVICE:
            rows = torch.empty((npix, 9), dtype=torch.float32, device=keep.device)
            self._check(self._lib.icp_pmap_nearest_neighbor_search(self._h, p, n, mem, rows.data_ptr(), C.byref(count),
                                                                   MEM_DEVICE))
            r = rows[:count.value]
            return r[:, 0:3].contiguous(), r[:, 3:6].contiguous(), r[:, 6:9].contiguous()
        rows = np.empty((npix, 9), np.float32)
        self._check(self._lib.icp_pmap_nearest_neighbor_search(self._h, p, n, mem, rows.ctypes.data, C.byref(count),
                                                               MEM_HOST))
        r = rows[:count.value]
        return r[:, 0:3].copy(), r[:, 3:6].copy(), r[:, 6:9].copy()

    def pmap_register(self, points: Array, init_pose=None, skip_null: bool = False) -> RegisterResult:
        self._bind(points)
        p, mem, keep = _ptr_mem(points)
        n = int(keep.shape[0])
        cap = max(1, int(self.config.max_num_alignments))
        losses = (C.c_double * cap)()
        dxs = (C.c_float * (6 * cap))()
        res = IcpRegisterResult()
        init = _pose16(init_pose if init_pose is not None else np.eye(4))
        self._check_registration(self._lib.icp_pmap_register(self._h, p, n, mem,
                                                             TARGETS_SKIP_NULL if skip_null else TARGETS_ALL, init,
                                                             C.byref(res), losses, dxs), res, losses, dxs)
        return self._result(res, losses, dxs)

    def pmap_register_launch(self, points: Array, init_pose=None, skip_null: bool = False):
        """`icp_pmap_register_launch`: `pmap_register` enqueued without waiting — every iteration on the stream, the stop
        decided on the device, no host polls; `register_end()` collects it (the same result, bit for bit)."""
        self._bind(points)
        p, mem, keep = _ptr_mem(points)
        self._keep_targets = [keep]
        init = _pose16(init_pose if init_pose is not None else np.eye(4))
        self._check(self._lib.icp_pmap_register_launch(self._h, p, int(keep.shape[0]), mem,
                                                       TARGETS_SKIP_NULL if skip_null else TARGETS_ALL, init))

    # ---- alignment ---------------------------------------------------------------------------------------------------
    def _residual_buffer(self, n: int, mem: int, like, with_residuals: bool):
        if not with_residuals:
            return None, None
        if mem == MEM_DEVICE:
            buf = torch.empty(n, dtype=torch.float32, device=like.device)
            return buf, buf.data_ptr()
        buf = np.empty(n, np.float32)
        return buf, buf.ctypes.data

    def _aligned(self, rc, pose, params, loss, neq, res, with_residuals):
        """The result tuple of an align call; an InvalidJacobianError carries it as `result` (the library writes every
        output before it returns that status: dx = 0, the loss and the sums of the rows, the residual vector)."""
        out = (np.array(pose, np.float32).reshape(4, 4), np.array(params, np.float32), float(loss.value),
               np.array(neq, np.float64))
        out = out + (res,) if with_residuals else out
        try:
            self._check(rc)
        except InvalidJacobianError as e:
            e.result = out
            raise
        return out

    def align_point_to_plane(self, ref_points: Array, tgt_points: Array, ref_normals: Array,
                             with_residuals: bool = False):
        """One Gauss-Newton point-to-plane step: (pose [4,4], dx [6], loss, normal equations [32] f64[, residuals [n]
        = (w r)^2 per row, numpy / cuda tensor like the inputs])."""
        self._bind(ref_points, tgt_points, ref_normals)
        r, mem_r, kr = _ptr_mem(ref_points)
        t, mem_t, kt = _ptr_mem(tgt_points)
        nn, mem_n, kn = _ptr_mem(ref_normals)
        if not (mem_r == mem_t == mem_n):
            raise AssertionError("ref / tgt / normals must live in the same memory space")
        n = int(kr.shape[0])
        if not (kt.shape[0] == n and kn.shape[0] == n):
            raise AssertionError("ref / tgt / normals must have the same number of rows")
        dx = (C.c_float * 6)()
        pose = (C.c_float * 16)()
        loss = C.c_double(0)
        neq = (C.c_double * 32)()
        res, res_ptr = self._residual_buffer(n, mem_r, kr, with_residuals)
        rc = self._lib.icp_align_point_to_plane(self._h, r, t, nn, n, mem_r, dx, pose, C.byref(loss), neq, res_ptr)
        return self._aligned(rc, pose, dx, loss, neq, res, with_residuals)

    def align_point_to_point(self, ref_points: Array, tgt_points: Array, x0=None, with_residuals: bool = False):
        """One Gauss-Newton point-to-point step linearised at x0 ([6] or None = zeros):
        (pose [4,4], params [6] = x0 + dx, loss, normal equations [32] f64[, residuals [n]])."""
        self._bind(ref_points, tgt_points)
        r, mem_r, kr = _ptr_mem(ref_points)
        t, mem_t, kt = _ptr_mem(tgt_points)
        if mem_r != mem_t:
            raise AssertionError("ref / tgt must live in the same memory space")
        n = int(kr.shape[0])
        if kt.shape[0] != n:
            raise AssertionError("ref / tgt must have the same number of rows")
        x = (C.c_float * 6)(*[float(v) for v in np.asarray(x0, np.float32).reshape(6)]) if x0 is not None else None
        params = (C.c_float * 6)()
        pose = (C.c_float * 16)()
        loss = C.c_double(0)
        neq = (C.c_double * 32)()
        res, res_ptr = self._residual_buffer(n, mem_r, kr, with_residuals)
        rc = self._lib.icp_align_point_to_point(self._h, r, t, n, mem_r, x, params, pose, C.byref(loss), neq, res_ptr)
        return self._aligned(rc, pose, params, loss, neq, res, with_residuals)

    def weighted_procrustes(self, tgt_points: Array, ref_points: Array, weights=None) -> np.ndarray:
        """`weighted_procrustes` (slam/common/registration.py:15-74): [4,4] float64 transform target -> reference."""
        t, mem_t, kt = _ptr_mem(tgt_points)
        r, mem_r, kr = _ptr_mem(ref_points)
        if mem_r != mem_t or kt.shape[0] != kr.shape[0]:
            raise AssertionError("target / reference must have the same shape and memory space")
        w, keep_w = None, None
        if weights is not None:
            if isinstance(weights, torch.Tensor):
                keep_w = weights.reshape(-1).to(torch.float32).contiguous()
                if (MEM_DEVICE if keep_w.is_cuda else MEM_HOST) != mem_t:
                    raise AssertionError("weights must live where the points live")
                w = keep_w.data_ptr()
            else:
                if mem_t != MEM_HOST:
                    raise AssertionError("weights must live where the points live")
                keep_w = np.ascontiguousarray(np.asarray(weights, np.float32).reshape(-1))
                w = keep_w.ctypes.data
            if keep_w.shape[0] != kt.shape[0]:
                raise AssertionError("one weight per point")
        out = (C.c_double * 16)()
        self._check(self._lib.icp_weighted_procrustes(self._h, t, r, w, int(kt.shape[0]), mem_t, out))
        return np.array(out, np.float64).reshape(4, 4)

    def compact_targets(self, rows: torch.Tensor, cap: int, skip_null: bool = True) -> torch.Tensor:
        """[cap,3] device tensor: the rows of `rows` [n,3] (a cuda tensor) that a registration with this masking would
        use, in order, at its head, null rows behind them — so registering it with skip_null walks `cap` rows instead of
        n.  `cap` must bound the number of passing rows (the caller's knowledge: a vertex map built from N points has at
        most N non-null pixels).  No host round trip."""
        if not (isinstance(rows, torch.Tensor) and rows.is_cuda):
            raise AssertionError("compact_targets works on device tensors")
        self._bind(rows)
        t = rows if rows.dtype == torch.float32 and rows.is_contiguous() else rows.to(torch.float32).contiguous()
        out = torch.empty((max(int(cap), 1), 3), dtype=torch.float32, device=t.device)
        self._check(self._lib.icp_compact_targets(self._h, t.data_ptr(), int(t.shape[0]),
                                                  TARGETS_SKIP_NULL if skip_null else TARGETS_ALL, out.data_ptr(),
                                                  int(cap)))
        return out[:int(cap)]

    # ---- registration ------------------------------------------------------------------------------------------------
    def _result(self, res: IcpRegisterResult, losses, dxs) -> RegisterResult:
        k = int(res.iterations)
        return RegisterResult(np.array(res.pose, np.float32).reshape(4, 4), np.array(res.params, np.float32), k,
                              bool(res.converged), int(res.num_targets), int(res.normals_computed),
                              np.array(losses[:k], np.float64), np.array(dxs, np.float32).reshape(-1, 6)[:k])

    def _check_registration(self, rc: int, res: IcpRegisterResult, losses, dxs):
        try:
            self._check(rc)
        except InvalidJacobianError as e:
            e.result = self._result(res, losses, dxs)
            raise

    def register(self, points: Array, init_pose=None, skip_null: bool = False) -> RegisterResult:
        self._bind(points)
        p, mem, keep = _ptr_mem(points)
        n = int(keep.shape[0])
        cap = max(1, int(self.config.max_num_alignments))
        losses = (C.c_double * cap)()
        dxs = (C.c_float * (6 * cap))()
        res = IcpRegisterResult()
        init = _pose16(init_pose if init_pose is not None else np.eye(4))
        self._check_registration(self._lib.icp_register(self._h, p, n, mem, TARGETS_SKIP_NULL if skip_null else TARGETS_ALL,
                                                        init, C.byref(res), losses, dxs), res, losses, dxs)
        return self._result(res, losses, dxs)

    # ---- multi-GPU: exchange of the normal equations inside the library ----------------------------------------------
    def exchange_create(self, rank: int, world: int) -> bytes:
        """Allocates this rank's inbox; returns its 64-byte IPC handle, to be all-gathered by the caller."""
        buf = C.create_string_buffer(64)
        self._check(self._lib.icp_exchange_create(self._h, int(rank), int(world), buf))
        return bytes(buf.raw)

    def exchange_connect(self, handles):
        """`handles`: the `world` handles in rank order.  From here on every registration on this context exchanges its
        normal equations with the peers inside the library (all ranks must issue the same registrations)."""
        blob = b"".join(bytes(h) for h in handles)
        self._check(self._lib.icp_exchange_connect(self._h, C.c_char_p(blob)))

    def exchange_destroy(self):
        self._check(self._lib.icp_exchange_destroy(self._h))

    # ---- multi-GPU: map-sharded normals ------------------------------------------------------------------------------
    def map_normals_owned(self, rank: int, world: int) -> torch.Tensor:
        """[M,4] float32 device tensor: (nx, ny, nz, 1) at the original index of every map point whose spatial bucket
        this rank owns, zeros elsewhere — to be summed over the ranks and handed to `map_normals_install`."""
        self.use_torch_stream()
        out = torch.empty((self.map_size(), 4), dtype=torch.float32, device=self.device)
        self._check(self._lib.icp_map_normals_owned(self._h, int(rank), int(world), out.data_ptr()))
        return out

    def map_normals_install(self, normals_by_index: torch.Tensor):
        self.use_torch_stream()
        t = normals_by_index.to(self.device, torch.float32).contiguous()
        if tuple(t.shape) != (self.map_size(), 4):
            raise AssertionError(f"expected [{self.map_size()}, 4] normals, got {tuple(t.shape)}")
        self._check(self._lib.icp_map_normals_install(self._h, t.data_ptr()))

    def map_normals_peek(self) -> np.ndarray:
        """The grid's normal cache as it stands (test support: `icp_map_normals_peek`): [M,4] float32 by original map index,
        (nx, ny, nz, 1) where the normal is there and zeros where it is not.  Estimates nothing and changes no flag."""
        out = np.zeros((self.map_size(), 4), np.float32)
        self._check(self._lib.icp_map_normals_peek(self._h, out.ctypes.data, MEM_HOST))
        return out

    # ---- multi-GPU seam ----------------------------------------------------------------------------------------------
    def normal_equations_tensor(self) -> torch.Tensor:
        """A torch-owned [32] f64 device vector installed as the context's normal-equation buffer, so that
        `torch.distributed.all_reduce` (RCCL) can sum it in place between accumulate() and solve()."""
        self.use_torch_stream()  # the collective that sums this vector is ordered on torch's stream
        if self._neq_tensor is None:
            self._neq_tensor = torch.zeros(32, dtype=torch.float64, device=self.device)
            self._check(self._lib.icp_set_normal_equations_buffer(self._h, self._neq_tensor.data_ptr()))
        return self._neq_tensor

    def register_begin(self, points: Array, init_pose=None, skip_null: bool = False):
        self._bind(points)
        p, mem, keep = _ptr_mem(points)
        self._keep_targets = [keep]
        init = _pose16(init_pose if init_pose is not None else np.eye(4))
        self._check(self._lib.icp_register_begin(self._h, p, int(keep.shape[0]), mem,
                                                 TARGETS_SKIP_NULL if skip_null else TARGETS_ALL, init))

    def register_launch(self, points: Array, init_pose=None, skip_null: bool = False):
        """Enqueue a whole registration without waiting; `register_end()` later blocks on it alone, so work enqueued in
        between (e.g. `map_update(None)`) overlaps the host's wait.  `init_pose="last"`: the initial guess is the pose of
        the previous registration, read on the device (constant-velocity initialisation without a host round trip) — with
        it up to two registrations may be in flight, `register_end()` returning them oldest first."""
        self._bind(points)
        p, mem, keep = _ptr_mem(points)
        self._keep_targets = (getattr(self, "_keep_targets", None) or [])[-1:] + [keep]
        mode = TARGETS_SKIP_NULL if skip_null else TARGETS_ALL
        if isinstance(init_pose, str):
            if init_pose != "last":
                raise AssertionError(f"unknown initial pose {init_pose!r}")
            self._check(self._lib.icp_register_launch_from_last(self._h, p, int(keep.shape[0]), mem, mode))
            return
        init = _pose16(init_pose if init_pose is not None else np.eye(4))
        self._check(self._lib.icp_register_launch(self._h, p, int(keep.shape[0]), mem, mode, init))

    def iteration_accumulate(self):
        self._check(self._lib.icp_iteration_accumulate(self._h))

    def iteration_solve(self):
        self._check(self._lib.icp_iteration_solve(self._h))

    def register_end(self) -> RegisterResult:
        cap = max(1, int(self.config.max_num_alignments))
        losses = (C.c_double * cap)()
        dxs = (C.c_float * (6 * cap))()
        res = IcpRegisterResult()
        self._check_registration(self._lib.icp_register_end(self._h, C.byref(res), losses, dxs), res, losses, dxs)
        return self._result(res, losses, dxs)

    # ---- one call per odometry frame ---------------------------------------------------------------------------------
    def odometry_init(self, voxel_size: float = 0.0, threshold_trans: float = 0.1, threshold_rot: float = 0.3,
                      constant_velocity: bool = True, targets: int = 0, copy_cloud: bool = True,
                      stage_max_rows: int = 32768):
        """`icp_odometry_init`: starts a sequence of `frame_launch` / `frame_end` on this context (empty map, frame 0).
        voxel_size > 0: the grid sample in front of every frame; targets 0: the frame's rows, 1: the pixels of its vertex
        map; constant_velocity: the initial guess of a frame is the last relative pose; copy_cloud: `frame_end` returns the
        frame's valid rows (`odometry_pc`), copied beside the registration; stage_max_rows: larger raw frames are not
        compacted in front of their registration (see icp_frame_config)."""
        cfg = _frame_config(self._lib, voxel_size=voxel_size, threshold_trans=threshold_trans, threshold_rot=threshold_rot,
                            constant_velocity=constant_velocity, targets=targets, copy_cloud=copy_cloud,
                            stage_max_rows=stage_max_rows)
        self._check(self._lib.icp_odometry_init(self._h, C.byref(cfg)))
        self._sequence_started(cfg)

    def _sequence_started(self, cfg: IcpFrameConfig):
        """A sequence of frame calls has been started on this context (by `odometry_init`, here or on a batch)."""
        self._frame_cfg = cfg
        self._frame_keep = None
        self._frame_rows = 0

    def frame_launch(self, points: Array, timestamps: Optional[Array] = None, init_pose=None):
        """`icp_frame_launch`: one frame — [N,3] float32 numpy rows (uploaded by the library through its pinned buffer) or a
        cuda tensor (used in place: keep it untouched until `frame_end`) — enqueued without waiting.  timestamps [N]
        float64 (where the points live): the frame is de-skewed by its initial guess.  init_pose: an explicit guess."""
        self._bind(points)
        p, n, mem, _, tp, keep = _frame_arrays(points, timestamps)
        self._check(self._lib.icp_frame_launch(self._h, p, n, mem, tp, _pose16(init_pose) if init_pose is not None else None))
        self._frame_launched(keep, n, mem)

    def _frame_launched(self, keep, n: int, mem: int):
        self._frame_keep = keep if mem == MEM_DEVICE else None  # (device data stays alive until the frame's end)
        self._frame_rows = n

    def frame_end(self, with_points: Optional[bool] = None, cap: Optional[int] = None) -> FrameResult:
        """`icp_frame_end`: waits for the frame's registration alone, applies the key-frame test and enqueues the map
        update; returns the pose, the per-iteration histories, the decision and — with_points (default: as `copy_cloud`
        of `odometry_init`) — the frame's valid rows.  An `Invalid Jacobian` raises before the map is touched."""
        return self._frame_end(self._lib.icp_frame_end, getattr(self, "_frame_cfg", None), with_points, cap)

    def _frame_end(self, fn, cfg, with_points, cap) -> FrameResult:
        """`frame_end` / `pmap_frame_end`: `fn` is the library's end call, `cfg` the sequence's configuration."""
        if with_points is None:
            with_points = bool(cfg is not None and cfg.copy_cloud)
        rows_cap = int(getattr(self, "_frame_rows", 0)) if cap is None else int(cap)
        hist = max(1, int(self.config.max_num_alignments))
        losses = (C.c_double * hist)()
        dxs = (C.c_float * (6 * hist))()
        res = IcpFrameResult()
        count = C.c_int64(0)
        out = np.empty((max(rows_cap, 1), 3), np.float32) if with_points else None
        rc = fn(self._h, C.byref(res), out.ctypes.data if out is not None else None, rows_cap,
                C.byref(count) if with_points else None, MEM_HOST, losses, dxs)
        self._frame_keep = None
        try:
            self._check_registration(rc, res.reg, losses, dxs)
        except AssertionError as e:  # (`cap` below the frame's rows: the frame is completed all the same)
            e.rows, e.result, e.register = int(count.value), res, self._result(res.reg, losses, dxs)
            raise
        first = int(res.frame_index) == 0
        points = out[:int(count.value)] if (out is not None and not first) else None
        return FrameResult(self._result(res.reg, losses, dxs), int(res.frame_index), bool(res.key_frame), int(res.samples),
                           int(res.inserted), points)

    # ---- one call per odometry frame, projective local map -----------------------------------------------------------
    def pmap_odometry_init(self, voxel_size: float = 0.0, threshold_trans: float = 0.1, threshold_rot: float = 0.3,
                           constant_velocity: bool = True, targets: int = 0, normals_kernel_size: int = 5,
                           copy_cloud: bool = True):
        """`icp_pmap_odometry_init`: starts a sequence of `pmap_frame_launch` / `pmap_frame_end` on this context (empty
        projective map, frame 0).  voxel_size > 0: the grid sample in front of every [N,3] frame; targets (for [N,3] frames)
        0: the frame's rows, 1: the pixels of its vertex map; normals_kernel_size: the window of the inserted maps' normals;
        the other settings as for `odometry_init`."""
        cfg = _pmap_frame_config(self._lib, voxel_size=voxel_size, threshold_trans=threshold_trans, threshold_rot=threshold_rot,
                                 constant_velocity=constant_velocity, targets=targets,
                                 normals_kernel_size=normals_kernel_size, copy_cloud=copy_cloud)
        self._check(self._lib.icp_pmap_odometry_init(self._h, C.byref(cfg)))
        self._pframe_cfg = cfg
        self._frame_keep = None
        self._frame_rows = 0

    def pmap_frame_launch(self, data: Array, timestamps: Optional[Array] = None, init_pose=None):
        """`icp_pmap_frame_launch`: one frame enqueued without waiting — [N,3] float32 rows (numpy: uploaded by the library;
        a cuda tensor: used in place) or a cuda [3,H,W] / [1,3,H,W] vertex map (its pixels are the targets).  Device data
        stays untouched until `pmap_frame_end`."""
        vmap = isinstance(data, torch.Tensor) and data.is_cuda and data.ndim in (3, 4)
        self._bind(data)
        if vmap and data.ndim == 4 and data.shape[0] != 1:
            raise AssertionError("Unexpected batched data format.")
        p, n, mem, layout, tp, keep = _frame_arrays(data, None if vmap else timestamps, vmap,
                                                    rows_alt=" or a [3,H,W] vertex map")
        if vmap and timestamps is not None:
            raise AssertionError("timestamps go with [N,3] rows, not with a vertex map")
        self._check(self._lib.icp_pmap_frame_launch(self._h, p, n, mem, layout, tp,
                                                    _pose16(init_pose) if init_pose is not None else None))
        self._frame_launched(keep, n, mem)

    def pmap_frame_end(self, with_points: Optional[bool] = None, cap: Optional[int] = None) -> FrameResult:
        """`icp_pmap_frame_end`: waits for the frame's registration alone, applies the key-frame test and enqueues the
        projective map's update; returns what `frame_end` returns (`inserted`: 1 when a vertex map was appended)."""
        return self._frame_end(self._lib.icp_pmap_frame_end, getattr(self, "_pframe_cfg", None), with_points, cap)

    # ---- aggregated world map -----------------------------------------------------------------------------------------
    def aggregated_map(self, voxel_size: float, capacity: int, max_insert_rows: int = 262144) -> "AggregatedMap":
        """A voxel-de-duplicated world map on this context's device (`icp_aggmap_*`): one float64 point per voxel of edge
        `voxel_size`, at most `capacity` points, fed by `insert` with at most `max_insert_rows` rows a call."""
        return AggregatedMap(self, voxel_size, capacity, max_insert_rows)

    def elevation_image(self, height: int = 400, width: int = 400, pixel_size: float = 0.4, z_min: float = 0.0,
                        z_max: float = 5.0, flip_z_axis: bool = False, color_map="jet", max_rows: int = 262144) -> "ElevationImage":
        """A top-down elevation image on this context's device (`icp_elevation_*`): `ElevationImageRegistration.build_image`
        of the reference with the settings of its constructor.  `color_map`: a matplotlib name, or a [259, 3] uint8 table."""
        return ElevationImage(self, height, width, pixel_size, z_min, z_max, flip_z_axis, color_map, max_rows)

    def cloud_refiner(self, max_target_rows: int, max_source_rows: int, cell_size: float = 1.0) -> "CloudRefiner":
        """A cloud-to-cloud point-to-point ICP on this context's device (`icp_refine_*`): the Open3D refinement of the
        reference's loop closure (slam/loop_closure.py:210-225), with a search grid of its own of `cell_size` metres."""
        return CloudRefiner(self, max_target_rows, max_source_rows, cell_size)

    def raise_for_status(self, rc: int):
        """Maps a status code of the C ABI to the exception the reference raises (public form of the internal check)."""
        self._check(rc)

    # ---- profiling ---------------------------------------------------------------------------------------------------
    def profile_enable(self, mask: int = 1):
        """bit mask of the kernels timed with HIP events: 1 search, 2 reduction, 4 normals (0 = off)."""
        self._check(self._lib.icp_profile_enable(self._h, int(mask)))

    def profile_read(self):
        s, n, r, m = C.c_double(0), C.c_int64(0), C.c_double(0), C.c_double(0)
        self._check(self._lib.icp_profile_read(self._h, C.byref(s), C.byref(n), C.byref(r), C.byref(m)))
        return {"search_ms": s.value, "search_launches": int(n.value), "reduce_ms": r.value, "normals_ms": m.value}

    def profile_read_iterations(self, cap: int = 64):
        """(ms, launches) of the search kernel by ICP iteration index (`icp_profile_read_iterations`)."""
        ms = np.zeros(cap, np.float64)
        n = np.zeros(cap, np.int64)
        self._check(self._lib.icp_profile_read_iterations(self._h, ms.ctypes.data, n.ctypes.data, int(cap)))
        return ms, n

    def profile_event_floor(self, samples: int = 200) -> float:
        """What an event pair adds (us, median) to the launch it brackets on this context's stream: measured around a kernel
        that spins for exactly 20 us, minus those 20 us (`icp_profile_event_floor`)."""
        v = C.c_double(0)
        self._check(self._lib.icp_profile_event_floor(self._h, int(samples), C.byref(v)))
        return float(v.value)


def _pose16_f64(m) -> "C.Array":
    a = np.ascontiguousarray(np.asarray(m, dtype=np.float64).reshape(4, 4))
    return (C.c_double * 16)(*a.reshape(-1).tolist())


class AggregatedMap:
    """The aggregated world map of a drive (`icp_aggmap_*`, include/icp_mi355x.h): the concatenation the reference's loop
    closure builds from its registered clouds (slam/loop_closure.py:272-291), kept on the device with one point per voxel.

    `insert(points, pose, frame_id)` moves the rows by the float64 absolute pose and is asynchronous; a voxel keeps the
    float64 world point of the first row that reached it, in creation order, with its `hits`, `first_frame` and
    `last_frame`.  Reads (`stats`, `points`, `hits`, ..., `submap`) synchronise.  Create it with
    `IcpContext.aggregated_map`."""

    def __init__(self, ctx: "IcpContext", voxel_size: float, capacity: int, max_insert_rows: int = 262144):
        self._ctx, self._lib = ctx, ctx._lib
        self.voxel_size, self.capacity, self.max_insert_rows = float(voxel_size), int(capacity), int(max_insert_rows)
        self._h = None
        h = C.c_void_p()
        ctx._check(self._lib.icp_aggmap_create(ctx._h, self.voxel_size, self.capacity, self.max_insert_rows, C.byref(h)))
        self._h = h
        if not hasattr(ctx, "_aggregated_maps"):
            ctx._aggregated_maps = weakref.WeakSet()
        ctx._aggregated_maps.add(self)

    def close(self):
        if getattr(self, "_h", None) and getattr(self._ctx, "_h", None):
            self._lib.icp_aggmap_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _handle(self):
        if not self._h:
            raise AssertionError("the aggregated map has been closed")
        return self._h

    def insert(self, points: Array, pose, frame_id: int) -> None:
        """The rows of `points` [n, 3] float32 (numpy: staged through pinned memory; cuda tensor: read in place) moved by
        `pose` [4, 4] float64 into the map, as frame `frame_id`."""
        h = self._handle()
        self._ctx._bind(points)
        p, mem, keep = _ptr_mem(points)
        if keep.ndim != 2 or keep.shape[1] != 3:
            raise AssertionError(f"AggregatedMap.insert: expected [n, 3] points, got {tuple(keep.shape)}")
        n = int(keep.shape[0])
        self._ctx._check(self._lib.icp_aggmap_insert(h, p if n else None, n, mem, C.byref(_pose16_f64(pose)), int(frame_id)))

    def stats(self) -> dict:
        """size, inserts, dropped, out_of_range, nonfinite and error of the map behind every insert so far (synchronises)."""
        c = _lib.IcpAggmapCounters()
        self._ctx._check(self._lib.icp_aggmap_stats(self._handle(), C.byref(c)))
        return {k: int(getattr(c, k)) for k, _ in c._fields_}

    def __len__(self) -> int:
        return self.stats()["size"]

    def _get(self, origin=None):
        h, size = self._handle(), len(self)
        xyz, hits = np.empty((size, 3), np.float32), np.empty(size, np.uint32)
        first, last = np.empty(size, np.int32), np.empty(size, np.int32)
        o = None if origin is None else C.byref((C.c_double * 3)(*np.asarray(origin, np.float64).reshape(3).tolist()))
        got = C.c_int64(0)
        self._ctx._check(self._lib.icp_aggmap_get(h, o, xyz.ctypes.data, hits.ctypes.data, first.ctypes.data, last.ctypes.data,
                                                  size, MEM_HOST, C.byref(got)))
        return xyz, hits, first, last

    def points(self, origin=None, dtype=np.float32) -> np.ndarray:
        """The stored points [size, 3] in creation order: float32(w - origin) (subtracted in float64, rounded once), or, with
        dtype=float64, the world points w themselves (no origin then)."""
        if np.dtype(dtype) == np.float64:
            if origin is not None:
                raise AssertionError("AggregatedMap.points: the float64 form returns the world points themselves (no origin)")
            size = len(self)
            xyz, got = np.empty((size, 3), np.float64), C.c_int64(0)
            self._ctx._check(self._lib.icp_aggmap_get_f64(self._handle(), xyz.ctypes.data, size, MEM_HOST, C.byref(got)))
            return xyz
        if np.dtype(dtype) != np.float32:
            raise AssertionError(f"AggregatedMap.points: float32 or float64, not {dtype}")
        return self._get(origin)[0]

    @property
    def hits(self) -> np.ndarray:
        """rows that fell into every stored voxel [size] uint32"""
        return self._get()[1]

    @property
    def first_frame(self) -> np.ndarray:
        """frame id of the insert that created every stored voxel [size] int32"""
        return self._get()[2]

    @property
    def last_frame(self) -> np.ndarray:
        """largest frame id among the rows of every stored voxel [size] int32"""
        return self._get()[3]

    def submap(self, lo: int, hi: int, pose):
        """(points [m, 3] float32, stored indices [m] int32) of the voxels with lo <= first_frame < hi, in storage order,
        moved by `pose` [4, 4] float64 — the window of slam/loop_closure.py:287-291 with the inverse of its middle pose."""
        h, size = self._handle(), len(self)
        xyz, index, got = np.empty((size, 3), np.float32), np.empty(size, np.int32), C.c_int64(0)
        self._ctx._check(self._lib.icp_aggmap_submap(h, int(lo), int(hi), C.byref(_pose16_f64(pose)), xyz.ctypes.data,
                                                     index.ctypes.data, size, MEM_HOST, C.byref(got)))
        m = int(got.value)
        return xyz[:m].copy(), index[:m].copy()

    def elevation(self, lo: int, hi: int, pose, image: "ElevationImage") -> "ElevationImage":
        """The elevation image of the window lo <= first_frame < hi moved by `pose`, built into `image` on the device without
        materialising the window (`ElevationImage.build_from`); returns `image`."""
        image.build_from(self, lo, hi, pose)
        return image

    def clear(self) -> None:
        """Empties the map; its memory stays."""
        self._ctx._check(self._lib.icp_aggmap_clear(self._handle()))

    def save_ply(self, path, origin=None, min_hits: int = 1) -> int:
        """Binary little-endian PLY of the stored points with hits >= min_hits: x y z float (relative to `origin`), hits uint.
        Returns the number of vertices written."""
        xyz, hits, _, _ = self._get(origin)
        return write_ply(path, xyz, hits, min_hits)


def write_ply(path, xyz: np.ndarray, hits: np.ndarray, min_hits: int = 1) -> int:
    """`AggregatedMap.save_ply` on arrays: plain Python and numpy."""
    keep = np.asarray(hits) >= int(min_hits)
    rows = np.empty(int(keep.sum()), dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("hits", "<u4")])
    kept = np.asarray(xyz, np.float32)[keep]
    rows["x"], rows["y"], rows["z"], rows["hits"] = kept[:, 0], kept[:, 1], kept[:, 2], np.asarray(hits, np.uint32)[keep]
    header = ("ply\nformat binary_little_endian 1.0\ncomment aggregated map, one point per voxel\n"
              f"element vertex {len(rows)}\nproperty float x\nproperty float y\nproperty float z\nproperty uint hits\n"
              "end_header\n")
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(rows.tobytes())
    return len(rows)


def colormap_table(color_map="jet") -> np.ndarray:
    """The [259, 3] uint8 table of a 256-colour matplotlib colour map (a name or a Colormap): its 256 colours, then its under,
    over and bad colour, each `uint8(rgba[:3] * 255.0)` — the conversion slam/common/registration.py:229-230 applies to every
    pixel.  matplotlib is imported here and nowhere else."""
    import matplotlib
    cmap = matplotlib.colormaps[color_map] if isinstance(color_map, str) else color_map
    if int(cmap.N) != 256:
        raise AssertionError(f"colormap_table: a colour map of 256 colours is needed, {cmap.name} has {cmap.N}")
    rgba = np.concatenate([np.asarray(cmap(np.arange(256)), np.float64).reshape(256, 4),
                           np.asarray([cmap.get_under(), cmap.get_over(), cmap.get_bad()], np.float64).reshape(3, 4)])
    return (rgba[:, :3] * 255.0).astype(np.uint8)


class ElevationImage:
    """`ElevationImageRegistration.build_image` of the reference (slam/common/registration.py:196-241) on the device
    (`icp_elevation_*`, include/icp_mi355x.h): the highest point per pixel of a top-down H x W image, as colour (`rgb`), `theta`,
    the float32 point behind every pixel (`points_3d`) and its row (`indices`, -1 where the pixel is empty).

    `build(points)` takes float32 or float64 rows (numpy: staged through pinned memory; cuda tensor: read in place);
    `build_from(map, lo, hi, pose)` rasterises a frame window of an `AggregatedMap`.  Both are asynchronous; the properties
    copy to the host and synchronise, `device(...)` returns cuda tensors without a host read.  Among rows of equal clipped z the
    highest row wins; a row whose z is NaN is set aside (`stats()["rows_nan_z"]`).  Create it with `IcpContext.elevation_image`."""

    def __init__(self, ctx: "IcpContext", height: int = 400, width: int = 400, pixel_size: float = 0.4, z_min: float = 0.0,
                 z_max: float = 5.0, flip_z_axis: bool = False, color_map="jet", max_rows: int = 262144):
        self._ctx, self._lib, self._h, self._keep = ctx, ctx._lib, None, None
        self.height, self.width, self.pixel_size = int(height), int(width), float(pixel_size)
        self.z_min, self.z_max, self.flip_z_axis, self.max_rows = float(z_min), float(z_max), bool(flip_z_axis), int(max_rows)
        table = color_map if isinstance(color_map, np.ndarray) else colormap_table(color_map)
        if table.dtype != np.uint8 or table.shape != (_lib.ELEVATION_LUT_ROWS, 3):
            raise AssertionError(f"ElevationImage: the colour table is [259, 3] uint8, not {table.dtype} {tuple(table.shape)}")
        self.table = np.ascontiguousarray(table)
        h = C.c_void_p()
        ctx._check(self._lib.icp_elevation_create(ctx._h, self.height, self.width, self.pixel_size, self.z_min, self.z_max,
                                                  int(self.flip_z_axis), self.table.ctypes.data, self.max_rows, C.byref(h)))
        self._h = h
        if not hasattr(ctx, "_elevation_images"):
            ctx._elevation_images = weakref.WeakSet()
        ctx._elevation_images.add(self)

    def close(self):
        if getattr(self, "_h", None) and getattr(self._ctx, "_h", None):
            self._lib.icp_elevation_destroy(self._h)
        self._h = self._keep = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _handle(self):
        if not self._h:
            raise AssertionError("the elevation image has been closed")
        return self._h

    def build(self, points: Array) -> None:
        """The image of the rows `points` [n, 3], float32 or float64 (any other type is converted to float32)."""
        h = self._handle()
        self._ctx._bind(points)
        if isinstance(points, torch.Tensor) and points.is_cuda:
            t = points if points.dtype in (torch.float32, torch.float64) else points.to(torch.float32)
            keep, mem, f64 = t.contiguous(), MEM_DEVICE, t.dtype == torch.float64
            ptr = keep.data_ptr()
        else:
            a = points.numpy() if isinstance(points, torch.Tensor) else np.asarray(points)
            keep = np.ascontiguousarray(a, dtype=np.float64 if a.dtype == np.float64 else np.float32)
            mem, f64, ptr = MEM_HOST, keep.dtype == np.float64, keep.ctypes.data
        if keep.ndim != 2 or keep.shape[1] != 3:
            raise AssertionError(f"ElevationImage.build: expected [n, 3] points, got {tuple(keep.shape)}")
        n = int(keep.shape[0])
        self._ctx._check(self._lib.icp_elevation_build(h, ptr if n else None, n, mem,
                                                       _lib.ELEVATION_F64 if f64 else _lib.ELEVATION_F32))
        self._keep = keep if mem == MEM_DEVICE else None  # (device rows are read in place, behind this call)

    def build_from(self, aggregated_map: "AggregatedMap", lo: int, hi: int, pose) -> None:
        """The image of the stored points of `aggregated_map` with lo <= first_frame < hi, moved by `pose` [4, 4] float64 as
        `AggregatedMap.submap` moves them; `indices` are stored indices."""
        self._ctx._check(self._lib.icp_elevation_build_aggmap(self._handle(), aggregated_map._handle(), int(lo), int(hi),
                                                              C.byref(_pose16_f64(pose))))
        self._keep = None

    def stats(self) -> dict:
        """rows_in_image, rows_outside, rows_nan_z and filled_pixels of the last build (synchronises)."""
        c = _lib.IcpElevationCounters()
        self._ctx._check(self._lib.icp_elevation_stats(self._handle(), C.byref(c)))
        return {k: int(getattr(c, k)) for k, _ in c._fields_}

    _OUTPUTS = {"rgb": (0, np.uint8, torch.uint8, 3), "theta": (1, np.float32, torch.float32, 0),
                "points_3d": (2, np.float32, torch.float32, 3), "indices": (3, np.int32, torch.int32, 0)}

    def _shape(self, last):
        return (self.height, self.width, last) if last else (self.height, self.width)

    def _host(self, name) -> np.ndarray:
        slot, dtype, _, last = self._OUTPUTS[name]
        out = np.empty(self._shape(last), dtype)
        args = [None] * 4
        args[slot] = out.ctypes.data
        self._ctx._check(self._lib.icp_elevation_get(self._handle(), *args, MEM_HOST))
        return out

    def device(self, *names) -> Tuple[torch.Tensor, ...]:
        """cuda tensors of the named outputs ("rgb", "theta", "points_3d", "indices"; none named: all four), copied on the
        device behind the build, on torch's current stream: no host read."""
        names = names or tuple(self._OUTPUTS)
        self._ctx.use_torch_stream()
        args, outs = [None] * 4, []
        for name in names:
            slot, _, dtype, last = self._OUTPUTS[name]
            outs.append(torch.empty(self._shape(last), dtype=dtype, device=self._ctx.device))
            args[slot] = outs[-1].data_ptr()
        self._ctx._check(self._lib.icp_elevation_get(self._handle(), *args, MEM_DEVICE))
        return tuple(outs)

    @property
    def rgb(self) -> np.ndarray:
        """the colour image [H, W, 3] uint8"""
        return self._host("rgb")

    @property
    def theta(self) -> np.ndarray:
        """(clipped z - z_min) / (z_max - z_min) of every pixel's point [H, W] float32; float32(z_min) where it is empty"""
        return self._host("theta")

    @property
    def points_3d(self) -> np.ndarray:
        """the point behind every pixel [H, W, 3] float32, zeros where it is empty (`points_3D`)"""
        return self._host("points_3d")

    @property
    def indices(self) -> np.ndarray:
        """the row behind every pixel [H, W] int32, -1 where it is empty (`pc_indices`)"""
        return self._host("indices")

    def build_image(self, pc: Array):
        """What the reference's `build_image` returns: (uint8 [H, W, 3], {"points_3D": float32 [H, W, 3], "pc_indices": int64
        [H, W]}), on the host."""
        self.build(pc)
        return self.rgb, {"points_3D": self.points_3d, "pc_indices": self.indices.astype(np.int64)}


class RefineResult:
    """What `CloudRefiner.end` returns (icp_refine_result): `transformation` [4, 4] float64 (source into target), `fitness`,
    `inlier_rmse`, `iterations`, `converged`, the counters `num_correspondences`, `source_rows`, `target_rows`,
    `source_rows_left_out`, `target_rows_left_out`, and `correspondences` [n] int32 (the target row of every source row at the
    last evaluation, -1 without one), copied from the device when first read."""

    def __init__(self, res: "_lib.IcpRefineResult", n: int, fetch):
        self.transformation = np.array(res.transformation, np.float64).reshape(4, 4)
        self.fitness, self.inlier_rmse = float(res.fitness), float(res.inlier_rmse)
        self.iterations, self.converged = int(res.iterations), bool(res.converged)
        self.num_correspondences, self.source_rows, self.target_rows = int(res.correspondences), int(res.source_rows), int(res.target_rows)
        self.source_rows_left_out, self.target_rows_left_out = int(res.source_rows_left_out), int(res.target_rows_left_out)
        self._n, self._fetch, self._corr = int(n), fetch, None

    @property
    def correspondences(self) -> np.ndarray:
        if self._corr is None:
            self._corr = self._fetch(self._n)
            self._fetch = None
        return self._corr


class CloudRefiner:
    """`ElevationImageLoopClosure._compute_transform` of the reference (slam/loop_closure.py:210-225) on the device
    (`icp_refine_*`, include/icp_mi355x.h): Open3D's point-to-point `registration_icp` of a source cloud against a target cloud.

    `set_target(rows)` builds the refiner's own search grid; `launch(rows, init, ...)` enqueues the whole loop and returns,
    `end()` waits and returns a `RefineResult`, `refine(...)` is both, `history()` the T and the 17 figures of every
    evaluation.  Rows are [n, 3] float32 (numpy: copied in; cuda tensor: read in place) or an `ElevationImage`, whose device
    `points_3D` is read in place (no copy: do not rebuild the image before `end`), the all-zero rows of empty pixels left out.  Nothing here touches the context's map or a
    registration in flight.  Create it with `IcpContext.cloud_refiner`."""

    def __init__(self, ctx: "IcpContext", max_target_rows: int, max_source_rows: int, cell_size: float = 1.0):
        self._ctx, self._lib, self._h = ctx, ctx._lib, None
        self.max_target_rows, self.max_source_rows, self.cell_size = int(max_target_rows), int(max_source_rows), float(cell_size)
        self._keep_target = self._keep_source = None
        self._n, self._last, self._corr_dev = 0, None, None
        h = C.c_void_p()
        ctx._check(self._lib.icp_refine_create(ctx._h, self.max_target_rows, self.max_source_rows, self.cell_size, C.byref(h)))
        self._h = h
        if not hasattr(ctx, "_cloud_refiners"):
            ctx._cloud_refiners = weakref.WeakSet()
        ctx._cloud_refiners.add(self)

    def close(self):
        if getattr(self, "_h", None) and getattr(self._ctx, "_h", None):
            self._lib.icp_refine_destroy(self._h)
        self._h = self._keep_target = self._keep_source = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _handle(self):
        if not self._h:
            raise AssertionError("the cloud refiner has been closed")
        return self._h

    def _rows(self, rows, drop_zero_rows: bool, who: str):
        """(pointer, n, mem, keep-alive, drop flag) of a cloud: an ElevationImage's device points_3D, or [n, 3] float32 rows"""
        if isinstance(rows, ElevationImage):
            if rows._ctx is not self._ctx:
                raise AssertionError(f"CloudRefiner.{who}: the elevation image belongs to another context")
            self._ctx.use_torch_stream()
            ptr, n = C.c_void_p(), C.c_int64(0)
            self._ctx._check(self._lib.icp_refine_image_rows(self._handle(), rows._handle(), C.byref(ptr), C.byref(n)))
            return ptr.value, int(n.value), MEM_DEVICE, rows, True  # (read in place: the image is kept alive, no copy is made)
        self._ctx._bind(rows)
        p, mem, keep = _ptr_mem(rows)
        if keep.ndim != 2 or keep.shape[1] != 3:
            raise AssertionError(f"CloudRefiner.{who}: expected [n, 3] points, got {tuple(keep.shape)}")
        n = int(keep.shape[0])
        return (p if n else None), n, mem, keep, bool(drop_zero_rows)

    def set_target(self, rows, drop_zero_rows: bool = False) -> None:
        """The target cloud (`target_pc` of the reference); asynchronous."""
        h = self._handle()
        p, n, mem, keep, drop = self._rows(rows, drop_zero_rows, "set_target")
        self._ctx._check(self._lib.icp_refine_set_target(h, p, n, mem, _lib.REFINE_DROP_ZERO_ROWS if drop else 0))
        self._keep_target = keep if mem == MEM_DEVICE else None

    def launch(self, rows, init=None, max_distance: float = 1.0, max_iteration: int = 30, relative_fitness: float = 1e-6,
               relative_rmse: float = 1e-6, drop_zero_rows: bool = False) -> None:
        """Enqueues the refinement of the source cloud `rows` (`candidate_pc`) from `init` [4, 4] (the identity by default) with
        the defaults of the reference's call; returns at once."""
        h = self._handle()
        p, n, mem, keep, drop = self._rows(rows, drop_zero_rows, "launch")
        prm = _lib.IcpRefineParams(float(max_distance), float(relative_fitness), float(relative_rmse), int(max_iteration),
                                   _lib.REFINE_DROP_ZERO_ROWS if drop else 0)
        t0 = _pose16_f64(np.eye(4) if init is None else init)
        self._ctx._check(self._lib.icp_refine_launch(h, p, n, mem, C.byref(t0), C.byref(prm)))
        self._keep_source, self._n = keep, n

    def end(self) -> RefineResult:
        """Waits for the refinement launched last and returns its `RefineResult`."""
        h = self._handle()
        res = _lib.IcpRefineResult()
        self._ctx.use_torch_stream()
        corr = torch.empty(max(self._n, 1), dtype=torch.int32, device=self._ctx.device)
        rc = self._lib.icp_refine_end(h, C.byref(res), corr.data_ptr() if self._n else None, MEM_DEVICE)
        self._keep_source = None
        self._ctx._check(rc)
        self._corr_dev = corr
        self._last = RefineResult(res, self._n, lambda n, c=corr: c[:n].cpu().numpy() if n else np.empty(0, np.int32))
        return self._last

    def correspondences_device(self) -> torch.Tensor:
        """the correspondences of the refinement collected last as an int32 cuda tensor [n]"""
        return self._corr_dev[:self._n]

    def refine(self, rows, **kw) -> RefineResult:
        """`launch(rows, **kw)` followed by `end()`."""
        self.launch(rows, **kw)
        return self.end()

    def history(self):
        """(transforms [iterations + 1, 4, 4], figures [iterations + 1, 17]) float64 of the refinement collected last: for every
        evaluation the T it ran with and count, sum d2, mu_p [3], mu_q [3], H [9]."""
        if self._last is None:
            raise AssertionError("CloudRefiner.history: no refinement has been collected")
        rows = self._last.iterations + 1
        t, s = np.empty((rows, 16), np.float64), np.empty((rows, _lib.REFINE_FIGURES), np.float64)
        self._ctx._check(self._lib.icp_refine_history(self._handle(), t.ctypes.data, s.ctypes.data, rows))
        return t.reshape(rows, 4, 4), s


class IcpBatch:
    """B independent sequences advanced by ONE launch per ICP iteration (`icp_batch_*`, include/icp_mi355x.h): B
    `IcpContext`s of one device — each with its own local map, scan and registration state, i.e. B instances of the
    reference's `ICPFrameToModel` (slam/odometry/icp_odometry.py:248-299 registers one sequence, one frame at a time) —
    whose registrations are enqueued together by one host thread.  Per sequence the same poses, bit for bit, as
    `IcpContext.register_launch` / `map_update(None)` / `register_end` on that context alone."""

    def __init__(self, contexts):
        self.contexts = list(contexts)
        if not self.contexts:
            raise AssertionError("a batch needs at least one context")
        self._lib = self.contexts[0]._lib
        arr = (C.c_void_p * len(self.contexts))(*[c._h for c in self.contexts])
        handle = C.c_void_p()
        rc = self._lib.icp_batch_create(arr, len(self.contexts), C.byref(handle))
        if rc != 0:
            raise AssertionError(f"icp_batch_create failed ({STATUS_MESSAGES.get(rc, rc)}): 1..{_lib.BATCH_MAX_SEQUENCES} distinct "
                                 "contexts of one device")
        self._h = handle
        self._keep = None

    def close(self):
        if getattr(self, "_h", None):
            self._lib.icp_batch_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        return len(self.contexts)

    def _check(self, rc: int):
        if rc == 0:
            return
        msg = self._lib.icp_batch_last_error(self._h).decode() or STATUS_MESSAGES.get(rc, str(rc))
        if rc == _lib.ICP_ERR_INVALID_JACOBIAN:
            raise InvalidJacobianError("Invalid Jacobian in Gauss Newton minimization")
        if rc == _lib.ICP_ERR_INVALID_ARGUMENT:
            raise AssertionError(msg)
        raise RuntimeError(f"libicp_mi355x: {msg} ({rc})")

    def use_torch_stream(self):
        """Every member enqueues on torch's current stream of the batch's device."""
        c0 = self.contexts[0]
        stream = _RAW_STREAM(c0._device_index) if _RAW_STREAM is not None else \
            torch.cuda.current_stream(c0.device).cuda_stream
        if stream != getattr(self, "_bound_stream", None) or any(getattr(c, "_bound_stream", None) != stream
                                                                 for c in self.contexts):
            self._check(self._lib.icp_batch_set_stream(self._h, C.c_void_p(stream)))
            self._bound_stream = stream
            for c in self.contexts:
                c._bound_stream = stream

    def register_launch(self, scans, init_poses=None, skip_null: bool = False):
        """`scans[b]`: member b's scan ([n_b, 3] float32; all cuda tensors or all host arrays).  `init_poses`: a list of
        4x4 matrices (None entries: identity), None (identity for all) or "last" (every member starts from the device-resident
        pose of its previous registration: constant-velocity initialisation without a host round trip)."""
        self._launch(self._lib.icp_batch_register_launch, scans, init_poses, skip_null)

    def pmap_register_launch(self, scans, init_poses=None, skip_null: bool = False):
        """`IcpContext.pmap_register` on every member against its projective map (icp_batch_pmap_register_launch): every
        iteration of all members enqueued, three launches per iteration; `register_end` collects the results.  `scans`,
        `init_poses` and `skip_null` as for `register_launch`."""
        self._launch(self._lib.icp_batch_pmap_register_launch, scans, init_poses, skip_null)

    def _launch(self, fn, scans, init_poses, skip_null):
        if len(scans) != len(self.contexts):
            raise AssertionError(f"expected {len(self.contexts)} scans, got {len(scans)}")
        if _on_device(*scans):
            self.use_torch_stream()
        ptrs, ns, keep, mems = [], [], [], set()
        for a in scans:
            p, mem, k = _ptr_mem(a)
            ptrs.append(p)
            ns.append(int(k.shape[0]))
            keep.append(k)
            mems.add(mem)
        if len(mems) != 1:
            raise AssertionError("the scans of a batch must live in one memory space")
        mem = mems.pop()
        self._keep = (getattr(self, "_keep", None) or [])[-1:] + [keep]
        xyz = (C.c_void_p * len(ptrs))(*ptrs)
        n = (C.c_int64 * len(ns))(*ns)
        mode = TARGETS_SKIP_NULL if skip_null else TARGETS_ALL
        if isinstance(init_poses, str):
            if init_poses != "last":
                raise AssertionError(f"unknown initial pose {init_poses!r}")
            self._check(fn(self._h, xyz, n, mem, mode, None, 1))
            return
        init = None
        if init_poses is not None:
            flat = np.stack([np.asarray(m if m is not None else np.eye(4), dtype=np.float32).reshape(16)
                             for m in init_poses])
            if flat.shape[0] != len(self.contexts):
                raise AssertionError("one initial pose per member")
            init = np.ascontiguousarray(flat)
        self._check(fn(self._h, xyz, n, mem, mode, init.ctypes.data if init is not None else None, 0))

    def project(self, scans, outs):
        """`IcpContext.project(scans[b], out=outs[b])` for every member in two launches (cuda tensors: [n_b, 3] float32 scans,
        [3, H, W] float32 vertex maps)."""
        if len(scans) != len(self.contexts) or len(outs) != len(self.contexts):
            raise AssertionError("one scan and one vertex map per member")
        self.use_torch_stream()
        keep = []
        for a, o in zip(scans, outs):
            p, mem, k = _ptr_mem(a)
            if mem != MEM_DEVICE or not (isinstance(o, torch.Tensor) and o.is_cuda and o.dtype == torch.float32
                                         and o.is_contiguous()):
                raise AssertionError("batched projection takes cuda tensors (float32, contiguous)")
            keep.append(k)
        xyz = (C.c_void_p * len(keep))(*[k.data_ptr() for k in keep])
        n = (C.c_int64 * len(keep))(*[int(k.shape[0]) for k in keep])
        vm = (C.c_void_p * len(outs))(*[o.data_ptr() for o in outs])
        self._check(self._lib.icp_batch_project(self._h, xyz, n, vm))
        return outs

    def map_update(self):
        """`map_update(None)` on every member: the pose-only update by the device-resident pose of its registration."""
        self._check(self._lib.icp_batch_map_update(self._h))

    def stage(self, clouds, skip_null: bool = False):
        """`IcpContext.map_stage_cloud(clouds[b])` on every member in ONE call, two launches (icp_batch_stage): the clouds
        ([n_b, 3] float32 cuda tensors) a later `map_update_staged` inserts."""
        b = len(self.contexts)
        if len(clouds) != b:
            raise AssertionError(f"expected {b} clouds, got {len(clouds)}")
        keep = [self._device_rows(pts, "batched staging") for pts in clouds]
        self.use_torch_stream()
        xyz = (C.c_void_p * b)(*[k.data_ptr() if k.shape[0] else None for k in keep])
        n = (C.c_int64 * b)(*[int(k.shape[0]) for k in keep])
        self._keep_staged = keep  # (read by the enqueued launches)
        self._check(self._lib.icp_batch_stage(self._h, xyz, n, TARGETS_SKIP_NULL if skip_null else TARGETS_ALL))

    @staticmethod
    def _device_rows(a, what: str) -> torch.Tensor:
        """[n, 3] float32 contiguous cuda rows (a float32 view of a cuda tensor of another dtype / layout is made here)."""
        if not (isinstance(a, torch.Tensor) and a.is_cuda):
            raise AssertionError(f"{what} takes cuda tensors (device pointers), got {type(a).__name__}"
                                 f"{'' if not isinstance(a, torch.Tensor) else ' on ' + str(a.device)}")
        t = a if (a.dtype == torch.float32 and a.is_contiguous()) else a.to(torch.float32).contiguous()
        if t.ndim != 2 or t.shape[1] != 3:
            raise AssertionError(f"{what}: expected [n, 3] rows, got {tuple(t.shape)}")
        return t

    def estimate_timestamps(self, rows_b, clockwise: bool = True, phi_0: float = 0.0):
        """`IcpContext.estimate_timestamps(rows_b[b], clockwise, phi_0)` for every member in two launches
        (icp_batch_estimate_timestamps): a list of [n_b] float64 cuda tensors.  rows_b[b]: [n_b, 3] or [n_b, 4] float32
        cuda rows, all of one width; None or an empty tensor: the member sits out (None in the result)."""
        b = len(self.contexts)
        if len(rows_b) != b:
            raise AssertionError(f"expected {b} scans, got {len(rows_b)}")
        keep = []
        for k, a in enumerate(rows_b):
            if a is None:
                keep.append(None)
                continue
            if not (isinstance(a, torch.Tensor) and a.is_cuda):
                raise AssertionError(f"batched time stamps, member {k}: the rows must be a cuda tensor (device pointers)")
            keep.append(IcpContext._scan_rows(a, f"batched time stamps, member {k}"))
        widths = {int(k.shape[1]) for k in keep if k is not None}
        if len(widths) > 1:
            raise AssertionError("batched time stamps: the members' rows must share one width (3 or 4)")
        stride = widths.pop() if widths else 3
        out = [torch.empty(int(k.shape[0]), dtype=torch.float64, device=k.device)
               if k is not None and k.shape[0] else None for k in keep]
        self.use_torch_stream()
        rows = (C.c_void_p * b)(*[k.data_ptr() if o is not None else None for k, o in zip(keep, out)])
        n = (C.c_int64 * b)(*[int(k.shape[0]) if o is not None else 0 for k, o in zip(keep, out)])
        ts = (C.c_void_p * b)(*[o.data_ptr() if o is not None else None for o in out])
        self._keep_timestamped = keep  # (read by the enqueued launches)
        self._check(self._lib.icp_batch_estimate_timestamps(self._h, rows, n, stride, int(bool(clockwise)), float(phi_0), ts))
        return out

    def project_rows(self, scans, rows=True):
        """`IcpContext.project_rows(scans[b])` for every member in two launches (icp_batch_project_rows): a list of
        (vertex map [3, H, W], rows [H * W, 3]) per member.  `rows`: False, or a list of flags — the members without rows
        get their vertex map only (None in place of the rows; the same launches as `project`)."""
        b = len(self.contexts)
        if len(scans) != b:
            raise AssertionError(f"expected {b} scans, got {len(scans)}")
        flags = [bool(rows)] * b if isinstance(rows, bool) else [bool(r) for r in rows]
        if len(flags) != b:
            raise AssertionError(f"expected {b} row flags, got {len(flags)}")
        keep = [self._device_rows(a, "batched projection") for a in scans]
        self.use_torch_stream()
        out = []
        for c, k, r in zip(self.contexts, keep, flags):
            h, w = c.config.height, c.config.width
            out.append((torch.empty((3, h, w), dtype=torch.float32, device=k.device),
                        torch.empty((h * w, 3), dtype=torch.float32, device=k.device) if r else None))
        xyz = (C.c_void_p * b)(*[k.data_ptr() if k.shape[0] else None for k in keep])
        n = (C.c_int64 * b)(*[int(k.shape[0]) for k in keep])
        vm = (C.c_void_p * b)(*[v.data_ptr() for v, _ in out])
        rw = (C.c_void_p * b)(*[r.data_ptr() if r is not None else None for _, r in out])
        self._keep_projected = keep
        self._check(self._lib.icp_batch_project_rows(self._h, xyz, n, vm, rw))
        return out

    def preprocess(self, points, timestamps, rel_poses, voxel_size: float, out=None):
        """`Distortion` -> `GridSample(padded)` -> `ToTensor(float32)` (slam/preprocessing.py:144-191, :207-226, :101-126)
        for every member in one call (icp_batch_preprocess): two launches de-skew, four sample, nothing is read back.

        points[b]: [n_b, 3] float32 cuda tensor; timestamps[b]: [n_b] float64 cuda tensor — the frame is de-skewed by
        rel_poses[b] (4x4) and sampled from its float64 rows — or None (Distortion's pass-through: sampled from its float32
        rows).  Returns `out` (allocated when None): one dict per member with `distorted` ([n, 3] float64, None without
        timestamps), `samples` ([n, 3] in the member's dtype), `samples_f32` ([n, 3] float32; for a float32 member the very
        same tensor as `samples`), `indices` ([n] int64) and `count` (0-dim int32 cuda tensor, V): the V samples by ascending
        voxel hash first, NaN rows / index -1 behind them — per member the bits of `IcpContext.distort` +
        `grid_sample_padded` + a float32 cast.  Entries of a given `out` may be None (`distorted` of a de-skewed member:
        the call is refused)."""
        b = len(self.contexts)
        if len(points) != b or len(timestamps) != b or len(rel_poses) != b:
            raise AssertionError(f"expected {b} frames, timestamps and relative poses, got "
                                 f"{len(points)} / {len(timestamps)} / {len(rel_poses)}")
        pts = []
        for k, a in enumerate(points):
            if not (isinstance(a, torch.Tensor) and a.is_cuda and a.dtype == torch.float32):
                raise AssertionError(f"batched preprocessing, member {k}: the points must be a float32 cuda tensor")
            pts.append(self._device_rows(a, f"batched preprocessing, member {k}"))
        ts = []
        for k, (t, p) in enumerate(zip(timestamps, pts)):
            if t is None:
                ts.append(None)
                continue
            if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64):
                raise AssertionError(f"batched preprocessing, member {k}: the timestamps must be a float64 cuda tensor")
            t = t.reshape(-1).contiguous()
            if t.shape[0] != p.shape[0]:
                raise AssertionError(f"batched preprocessing, member {k}: {t.shape[0]} timestamps for {p.shape[0]} points")
            ts.append(t)
        if out is None:
            out = []
            for p, t in zip(pts, ts):
                n, dev = int(p.shape[0]), p.device
                f32 = torch.empty((n, 3), dtype=torch.float32, device=dev)
                out.append({"distorted": torch.empty((n, 3), dtype=torch.float64, device=dev) if t is not None else None,
                            "samples": torch.empty((n, 3), dtype=torch.float64, device=dev) if t is not None else f32,
                            "samples_f32": f32, "indices": torch.empty(n, dtype=torch.int64, device=dev),
                            "count": torch.empty((), dtype=torch.int32, device=dev)})
        if len(out) != b:
            raise AssertionError(f"expected {b} output sets, got {len(out)}")
        for k, o in enumerate(out):
            for key in ("distorted", "samples", "samples_f32", "indices", "count"):
                v = o.get(key)
                if v is not None and not (isinstance(v, torch.Tensor) and v.is_cuda and v.is_contiguous()):
                    raise AssertionError(f"batched preprocessing, member {k}: `{key}` must be a contiguous cuda tensor")
        frames = (IcpPreprocessFrame * b)()
        rel_off = IcpPreprocessFrame.rel_pose.offset
        poses = []
        for k, (p, t, o) in enumerate(zip(pts, ts, out)):
            f = frames[k]
            n = int(p.shape[0])
            f.xyz = p.data_ptr() if n else None
            f.n = n
            if t is not None:
                f.timestamps = t.data_ptr() if n else None
                pose = np.ascontiguousarray(np.asarray(rel_poses[k], dtype=np.float64).reshape(16))
                poses.append(pose)
                C.memmove(C.addressof(f) + rel_off, pose.ctypes.data, 128)

            def ptr(key, dtype=None):
                v = o.get(key)
                if v is None or n == 0 and key != "count":
                    return None
                if dtype is not None and v.dtype != dtype:
                    raise AssertionError(f"batched preprocessing, member {k}: `{key}` must be {dtype}")
                return v.data_ptr()
            f.distorted_out = ptr("distorted", torch.float64)
            smp = o.get("samples")
            f.samples_out = None if (smp is None or smp is o.get("samples_f32")) else \
                ptr("samples", torch.float64 if t is not None else torch.float32)
            f.samples_f32_out = ptr("samples_f32", torch.float32)
            f.indices_out = ptr("indices", torch.int64)
            f.count_out = ptr("count", torch.int32)
        self.use_torch_stream()
        self._keep_preprocessed = (pts, ts)  # (read by the enqueued launches)
        self._check(self._lib.icp_batch_preprocess(self._h, frames, float(voxel_size)))
        return out

    def map_update_staged(self, insert, rel_poses=None):
        """`ICPFrameToModel.__update_map` for every member (icp_batch_map_update_staged): member b inserts the cloud it
        staged (`stage`) if `insert[b]`, and is updated by its pose only otherwise.  `rel_poses`: B 4x4 matrices, or None
        (every member's device-resident pose of its last registration).  Returns the rows inserted per member."""
        b = len(self.contexts)
        if len(insert) != b:
            raise AssertionError(f"expected {b} insert flags, got {len(insert)}")
        flags = (C.c_int32 * b)(*[1 if f else 0 for f in insert])
        rel = None
        if rel_poses is not None:
            rel = np.ascontiguousarray(np.stack([np.asarray(m, dtype=np.float32).reshape(16) for m in rel_poses]))
            if rel.shape[0] != b:
                raise AssertionError("one relative pose per member")
        ins = (C.c_int64 * b)()
        self._check(self._lib.icp_batch_map_update_staged(self._h, rel.ctypes.data if rel is not None else None, flags, ins))
        return [int(v) for v in ins]

    def pmap_update(self, rel_poses, vmaps, normals_kernel_size: int = 5):
        """`IcpContext.pmap_update(rel_poses[b], vmaps[b], normals_kernel_size)` on every member in four launches
        (icp_batch_pmap_update): `vmaps[b]` a [3,H,W] vertex map (all cuda tensors or all host arrays) to insert, or None for
        a pose-only update; `vmaps` None: pose-only for every member."""
        b = len(self.contexts)
        if len(rel_poses) != b or (vmaps is not None and len(vmaps) != b):
            raise AssertionError(f"expected {b} relative poses and vertex maps")
        rel = np.ascontiguousarray(np.stack([np.asarray(m, dtype=np.float32).reshape(16) for m in rel_poses]))
        ptrs, keep, mems = [None] * b, [], set()
        for i, (c, v) in enumerate(zip(self.contexts, vmaps if vmaps is not None else [None] * b)):
            if v is None:
                continue
            p, mem, k = c._planar(v)
            ptrs[i] = p
            keep.append(k)
            mems.add(mem)
        if len(mems) > 1:
            raise AssertionError("the vertex maps of a batch must live in one memory space")
        mem = mems.pop() if mems else MEM_DEVICE
        if mem == MEM_DEVICE:
            self.use_torch_stream()
        vm = (C.c_void_p * b)(*ptrs)
        self._keep_vmaps = keep  # (alive until the next update: the copies _planar made are read by the enqueued launches)
        self._check(self._lib.icp_batch_pmap_update(self._h, rel.ctypes.data, vm, mem, int(normals_kernel_size)))

    # ---- one call per odometry frame, B sequences per call -------------------------------------------------------------
    def odometry_init(self, **kw):
        """`icp_batch_odometry_init`: `IcpContext.odometry_init(**kw)` on every member (the sequence state is the member's
        own: a member may also be stepped, or restarted, alone)."""
        cfg = _frame_config(self._lib, **kw)
        self._check(self._lib.icp_batch_odometry_init(self._h, C.byref(cfg)))
        for c in self.contexts:
            mine = IcpFrameConfig()
            C.memmove(C.byref(mine), C.byref(cfg), C.sizeof(cfg))
            c._sequence_started(mine)
        self._frame_step = None

    def frame_launch(self, scans, timestamps=None, init_poses=None, skip=None):
        self._launch_frames(scans, timestamps, init_poses, skip, False)

    def pmap_frame_launch(self, frames, timestamps=None, init_poses=None, skip=None):
        """`icp_batch_pmap_frame_launch`: as `frame_launch`, against the members' projective maps; `frames[b]`: [N,3] rows (all
        numpy or all cuda) or — all members alike — cuda [3,H,W] / [1,3,H,W] vertex maps."""
        self._launch_frames(frames, timestamps, init_poses, skip, True)

    def _launch_frames(self, scans, timestamps, init_poses, skip, pmap):
        """`icp_batch_frame_launch`: `scans[b]` = member b's next frame ([N,3] float32; all numpy arrays — uploaded by the
        library through ONE pinned buffer — or all cuda tensors, used in place until `frame_end`); `timestamps[b]` ([N]
        float64 where the points live) or None; `init_poses[b]` (4x4) or None; `skip[b]`: the member sits this step out
        (its scan may be None)."""
        b = len(self.contexts)
        skip = [False] * b if skip is None else [bool(v) for v in skip]
        timestamps = [None] * b if timestamps is None else list(timestamps)
        init_poses = [None] * b if init_poses is None else list(init_poses)
        if len(scans) != b or len(skip) != b or len(timestamps) != b or len(init_poses) != b:
            raise AssertionError(f"expected {b} scans, timestamps, initial poses and skip flags")
        active = [a for a, sk in zip(scans, skip) if not sk]
        on_device = bool(active) and all(isinstance(a, torch.Tensor) and a.is_cuda for a in active)
        if not on_device and _on_device(*active):
            raise AssertionError("the frames of a batched step must live in one memory space")
        if on_device:
            self.use_torch_stream()
        vmaps = pmap and on_device and all(a.ndim in (3, 4) for a in active)
        if pmap and not vmaps and any(isinstance(a, torch.Tensor) and a.ndim in (3, 4) for a in active):
            raise AssertionError("the frames of a batched step are all rows or all cuda vertex maps")
        frames = (IcpBatchFrame * b)()
        keep, rows = [], [0] * b
        for i, (a, t, g, sk) in enumerate(zip(scans, timestamps, init_poses, skip)):
            f = frames[i]
            f.skip = 1 if sk else 0
            if sk:
                continue
            f.xyz, f.n, _, _, f.timestamps, arrays = _frame_arrays(a, t, vmaps, who=f"member {i}: ")
            pose = _pose16(g) if g is not None else None
            f.init_pose = C.cast(pose, C.c_void_p) if pose is not None else None
            keep.append((*arrays, pose))
            rows[i] = int(f.n)
        mem = MEM_DEVICE if on_device else MEM_HOST
        if pmap:
            self._check(self._lib.icp_batch_pmap_frame_launch(self._h, frames, mem, FRAME_VERTEX_MAP if vmaps else FRAME_ROWS))
        else:
            self._check(self._lib.icp_batch_frame_launch(self._h, frames, mem))
        self._frame_step = (keep if on_device else None, rows, skip)

    def pmap_odometry_init(self, **kw):
        """`icp_batch_pmap_odometry_init`: `IcpContext.pmap_odometry_init` on every member (the same keywords), every member
        checked before any is restarted."""
        cfg = _pmap_frame_config(self._lib, **kw)
        self._check(self._lib.icp_batch_pmap_odometry_init(self._h, C.byref(cfg)))
        for c in self.contexts:
            c._pframe_cfg = cfg
            c._frame_keep, c._frame_rows = None, 0

    def pmap_frame_end(self, with_points=None, cap=None):
        """`icp_batch_pmap_frame_end`: as `frame_end`, with ONE batched update of the projective maps."""
        return self.frame_end(with_points, cap, _pmap=True)

    def frame_end(self, with_points=None, cap=None, _pmap=False):
        """`icp_batch_frame_end`: one wait for all registrations, the key-frame tests, one batched map update.  A list with
        one `FrameResult` per member (None: the member sat the step out).  with_points: a flag or one per member (default:
        each member's `copy_cloud`).  A member whose registration failed raises `InvalidJacobianError` AFTER the step has
        completed for the others — `.results` (None at the failed positions) and `.failed`, as `register_end`; a `cap[b]`
        below the member's rows raises AssertionError with `.results` (that member's `points` None) and `.rows`."""
        b = len(self.contexts)
        step = getattr(self, "_frame_step", None)
        rows = step[1] if step else [0] * b
        skip = step[2] if step else [False] * b
        if with_points is None:
            attr = "_pframe_cfg" if _pmap else "_frame_cfg"
            want = [bool(getattr(c, attr, None) is not None and getattr(c, attr).copy_cloud) for c in self.contexts]
        elif isinstance(with_points, (list, tuple)):
            want = [bool(v) for v in with_points]
        else:
            want = [bool(with_points)] * b
        caps = [int(r) for r in rows] if cap is None else [int(v) for v in cap]
        hist = max(1, int(self.contexts[0].config.max_num_alignments))
        res = (IcpFrameResult * b)()
        losses = (C.c_double * (hist * b))()
        dxs = (C.c_float * (6 * hist * b))()
        outs = [np.empty((max(c, 1), 3), np.float32) if (w and not sk) else None for c, w, sk in zip(caps, want, skip)]
        out_ptrs = (C.c_void_p * b)(*[o.ctypes.data if o is not None else None for o in outs])
        cap_arr = (C.c_int64 * b)(*caps)
        counts = (C.c_int64 * b)()
        end = self._lib.icp_batch_pmap_frame_end if _pmap else self._lib.icp_batch_frame_end
        rc = end(self._h, res, out_ptrs, cap_arr, counts, MEM_HOST, losses, dxs)
        if rc == _lib.ICP_ERR_INVALID_ARGUMENT and \
                self._lib.icp_batch_last_error(self._h).decode().endswith("(nothing was changed)"):
            self._check(rc)  # refused: the step (if any) still awaits its end
        self._frame_step = None
        la = np.array(losses, np.float64).reshape(b, hist)
        da = np.array(dxs, np.float32).reshape(b, hist, 6)
        out, failed = [], []
        for i in range(b):
            r = res[i]
            if int(r.frame_index) < 0:
                out.append(None)
                continue
            if int(r.reg.status) != 0:
                failed.append(i)
                out.append(None)
                continue
            k = int(r.reg.iterations)
            reg = RegisterResult(np.array(r.reg.pose, np.float32).reshape(4, 4), np.array(r.reg.params, np.float32), k,
                                 bool(r.reg.converged), int(r.reg.num_targets), int(r.reg.normals_computed),
                                 la[i, :k].copy(), da[i, :k].copy())
            first = int(r.frame_index) == 0
            n = int(counts[i])
            pts = outs[i][:n] if (outs[i] is not None and not first and n <= caps[i]) else None
            out.append(FrameResult(reg, int(r.frame_index), bool(r.key_frame), int(r.samples), int(r.inserted), pts))
        if rc != 0:
            try:
                self._check(rc)
            except Exception as err:
                err.results, err.failed, err.rows = out, failed, [int(v) for v in counts]
                if failed:  # (what the registration reached, as IcpContext.frame_end hands it over)
                    i = failed[0]
                    k = int(res[i].reg.iterations)
                    err.result = RegisterResult(np.array(res[i].reg.pose, np.float32).reshape(4, 4),
                                                np.array(res[i].reg.params, np.float32), k, bool(res[i].reg.converged),
                                                int(res[i].reg.num_targets), int(res[i].reg.normals_computed),
                                                la[i, :k].copy(), da[i, :k].copy())
                raise
        return out

    def register_end(self):
        """One wait for all members; a list of `RegisterResult`s.  Raises what the first failing member would raise; the
        library has collected every member all the same, so the exception carries `.results` (the list, None at the
        failing positions) and `.failed` (their indices): a neighbour's singular system costs the healthy members
        nothing."""
        b = len(self.contexts)
        cap = max(1, int(self.contexts[0].config.max_num_alignments))
        res = (IcpRegisterResult * b)()
        for r in res:
            r.status = _lib.ICP_ERR_INVALID_ARGUMENT  # (a slot the library never reached is no result)
        losses = (C.c_double * (cap * b))()
        dxs = (C.c_float * (6 * cap * b))()
        rc = self._lib.icp_batch_register_end(self._h, res, losses, dxs)
        la = np.array(losses, np.float64).reshape(b, cap)
        da = np.array(dxs, np.float32).reshape(b, cap, 6)
        out = []
        for i in range(b):
            if rc != 0 and int(res[i].status) != 0:
                out.append(None)
                continue
            k = int(res[i].iterations)
            out.append(RegisterResult(np.array(res[i].pose, np.float32).reshape(4, 4), np.array(res[i].params, np.float32), k,
                                      bool(res[i].converged), int(res[i].num_targets), int(res[i].normals_computed),
                                      la[i, :k].copy(), da[i, :k].copy()))
        if rc != 0:
            try:
                self._check(rc)
            except Exception as err:
                err.results = out
                err.failed = [i for i, r in enumerate(out) if r is None]
                raise
        return out
