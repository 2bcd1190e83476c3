"""Registers the MI355X plugins inside an importable pyLiDAR-SLAM checkout, without editing it.

The reference resolves its plugins through enums of `(class, config dataclass)` pairs:
  ODOMETRY         selector `algorithm`    slam/odometry/__init__.py:23-32   (loader slam/common/utils.py:266-302)
  DATASET          selector `dataset`      slam/dataset/__init__.py:15-38
  FILTER           selector `filter_name`  slam/preprocessing.py:230-252
  LOCAL_MAP        selector `type`         slam/odometry/local_map.py:437-445   (inner seam of ICPFrameToModel)
  RIGID_ALIGNMENT  selector `mode`         slam/odometry/alignment.py:200-208   (inner seam of ICPFrameToModel)
and hydra's ConfigStore (slam/odometry/icp_odometry.py:67-68).  An Enum cannot be extended in place, so
`register_with_reference()` builds new enums with the same members plus the MI355X ones and swaps them in wherever
the reference imported them.  A maintainer would instead add the lines shown in INTEGRATION.md to those modules.
"""
import sys
from enum import Enum

ALGORITHM_NAME = "icp_F2M_mi355x"
DATASET_NAMES = ("synthetic_mi355x", "kitti_mi355x", "kitti_360_mi355x")
FILTER_NAMES = ("grid_sample_mi355x", "distortion_mi355x", "voxelization_mi355x", "to_device_mi355x", "to_tensor_mi355x")
LOCAL_MAP_NAMES = ("hashgrid_local_map_mi355x", "projective_local_map_mi355x")
ALIGNMENT_NAMES = ("point_to_plane_gauss_newton_mi355x", "point_to_point_gauss_newton_mi355x")


def _swap_enum(owner, attr: str, extra: dict, mixins: tuple, namespace: dict):
    """New enum = members of `owner.attr` + `extra`, installed in every loaded slam.* module that holds the old one."""
    current = getattr(owner, attr)
    if all(name in current.__members__ for name in extra):
        return current
    members = {m.name: m.value for m in current}
    members.update(extra)
    base = type(f"_{attr}Base", mixins, dict(namespace)) if (mixins or namespace) else None
    patched = Enum(attr, members, type=base) if base is not None else Enum(attr, members)
    patched.__doc__ = current.__doc__
    for name, mod in list(sys.modules.items()):
        if name.startswith("slam") and getattr(mod, attr, None) is current:
            setattr(mod, attr, patched)
    return patched


def register_with_reference():
    """Call once, before `SLAM.init()` / `run.py`'s hydra main builds the pipeline. Returns the patched ODOMETRY enum
    (`icp_F2M_mi355x`); DATASET gains `synthetic_mi355x` / `kitti_mi355x` / `kitti_360_mi355x`, FILTER gains `grid_sample_mi355x` /
    `distortion_mi355x` / `voxelization_mi355x` / `to_device_mi355x` / `to_tensor_mi355x`, LOCAL_MAP gains
    `hashgrid_local_map_mi355x` / `projective_local_map_mi355x` and RIGID_ALIGNMENT gains
    `point_to_plane_gauss_newton_mi355x` / `point_to_point_gauss_newton_mi355x` (so the reference's OWN
    `ICPFrameToModel` can run on the MI355X local map / alignment through its inner seams)."""
    import slam.dataset as ref_dataset
    import slam.odometry as ref_odometry
    import slam.preprocessing as ref_pre
    from slam.common.utils import ObjectLoaderEnum

    from .dataset import (KITTI360Config, KITTI360DatasetLoader, KITTIConfig, KITTIDatasetLoader, SyntheticDatasetConfig,
                          SyntheticDatasetLoader)
    import slam.odometry.alignment as ref_alignment
    import slam.odometry.local_map as ref_local_map
    from .odometry import (Distortion, DistortionConfig, GridSample, GridSampleConfig, HashGridLocalMap,
                           HashGridLocalMapConfig, MI355XICPConfig, MI355XICPFrameToModel, PointToPlaneAlignment,
                           PointToPlaneAlignmentConfig, PointToPointAlignment, PointToPointAlignmentConfig,
                           ProjectiveLocalMap, ProjectiveLocalMapConfig, ToDevice, ToDeviceConfig, ToTensor,
                           ToTensorConfig, Voxelization, VoxelizationConfig)

    odometry = _swap_enum(ref_odometry, "ODOMETRY", {ALGORITHM_NAME: (MI355XICPFrameToModel, MI355XICPConfig)},
                          (ObjectLoaderEnum,), {"type_name": classmethod(lambda cls: "algorithm")})
    _swap_enum(ref_dataset, "DATASET", {DATASET_NAMES[0]: (SyntheticDatasetLoader, SyntheticDatasetConfig),
                                         DATASET_NAMES[1]: (KITTIDatasetLoader, KITTIConfig),
                                         DATASET_NAMES[2]: (KITTI360DatasetLoader, KITTI360Config)},
               (ObjectLoaderEnum,), {"type_name": classmethod(lambda cls: "dataset")})

    def _load_filter(config, **kwargs):  # slam/preprocessing.py:243-252, against the patched enum
        name = config.filter_name
        flt = ref_pre.FILTER
        assert name in flt.__members__, f"unknown filter {name}"
        _class, _config = flt[name].value
        return _class(_config(**config), **kwargs)

    _swap_enum(ref_pre, "FILTER", {FILTER_NAMES[0]: (GridSample, GridSampleConfig),
                                   FILTER_NAMES[1]: (Distortion, DistortionConfig),
                                   FILTER_NAMES[2]: (Voxelization, VoxelizationConfig),
                                   FILTER_NAMES[3]: (ToDevice, ToDeviceConfig),
                                   FILTER_NAMES[4]: (ToTensor, ToTensorConfig)},
               (), {"load": staticmethod(_load_filter)})
    _swap_enum(ref_local_map, "LOCAL_MAP", {LOCAL_MAP_NAMES[0]: (HashGridLocalMap, HashGridLocalMapConfig),
                                            LOCAL_MAP_NAMES[1]: (ProjectiveLocalMap, ProjectiveLocalMapConfig)},
               (ObjectLoaderEnum,), {"type_name": classmethod(lambda cls: "type")})
    _swap_enum(ref_alignment, "RIGID_ALIGNMENT",
               {ALIGNMENT_NAMES[0]: (PointToPlaneAlignment, PointToPlaneAlignmentConfig),
                ALIGNMENT_NAMES[1]: (PointToPointAlignment, PointToPointAlignmentConfig)},
               (ObjectLoaderEnum,), {"type_name": classmethod(lambda cls: "mode")})
    try:  # hydra group entries, so `slam/odometry=icp_odometry_mi355x` / `dataset=synthetic_mi355x` resolve
        from hydra.core.config_store import ConfigStore
        cs = ConfigStore.instance()
        cs.store(name="icp_odometry_mi355x", group="slam/odometry", node=MI355XICPConfig)
        cs.store(name=DATASET_NAMES[0], group="dataset", node=SyntheticDatasetConfig)
        cs.store(name=DATASET_NAMES[1], group="dataset", node=KITTIConfig)
        cs.store(name=DATASET_NAMES[2], group="dataset", node=KITTI360Config)
        cs.store(name="hashgrid_mi355x", group="slam/odometry/local_map", node=HashGridLocalMapConfig)
        cs.store(name="projective_mi355x", group="slam/odometry/local_map", node=ProjectiveLocalMapConfig)
        cs.store(name="point_to_plane_GN_mi355x", group="slam/odometry/alignment", node=PointToPlaneAlignmentConfig)
        cs.store(name="point_to_point_GN_mi355x", group="slam/odometry/alignment", node=PointToPointAlignmentConfig)
    except Exception:  # hydra absent: the enum patches are all the loaders need
        pass
    return odometry


def install_kdtree():
    """Places `pylidar_slam_amd.kdtree` at `sys.modules["pykdtree.kdtree"]` (under a parent package `pykdtree`), so that
    `from pykdtree.kdtree import KDTree` — slam/odometry/local_map.py:12 — resolves to the MI355X search and the reference's
    unmodified `KdTreeLocalMap` runs its queries (:385, :405) on the device.  A slam.* module that was imported before and
    holds another `KDTree` is handed this one.  Returns the installed module."""
    import types

    from . import kdtree
    parent = types.ModuleType("pykdtree")
    parent.__path__ = []  # a package: `import pykdtree.kdtree` resolves through sys.modules
    parent.kdtree = kdtree
    sys.modules["pykdtree"] = parent
    sys.modules["pykdtree.kdtree"] = kdtree
    for name, mod in list(sys.modules.items()):
        held = getattr(mod, "KDTree", None) if name.startswith("slam") else None
        if held is not None and held is not kdtree.KDTree and getattr(held, "__module__", "").startswith("pykdtree"):
            setattr(mod, "KDTree", kdtree.KDTree)
    return kdtree


class _DeviceElevationBuilder:
    """The default builder of `install_elevation_image`: an `ElevationImage` with the settings of one reference object, on a
    context shared by all of them, recreated with more room when a cloud has more rows than it takes."""
    _ctx = None

    def __init__(self, owner):
        self.owner, self.image = owner, None

    def build_image(self, pc):
        from .engine import IcpContext, colormap_table
        rows = int(pc.shape[0])
        if self.image is None or rows > self.image.max_rows:
            if _DeviceElevationBuilder._ctx is None:
                _DeviceElevationBuilder._ctx = IcpContext()
            if self.image is not None:
                self.image.close()
            o = self.owner
            room = 1 << max(17, (rows - 1).bit_length())
            self.image = _DeviceElevationBuilder._ctx.elevation_image(o.H, o.W, o.pixel_size, o.z_min, o.z_max, o.flip_axis,
                                                                      colormap_table(o.color_map), room)
        return self.image.build_image(pc)


def install_elevation_image(factory=None):
    """Assigns the reference's `ElevationImageRegistration` (slam/common/registration.py:179-241; the class exists only where
    `cv2` does) a `build_image` that routes through a per-instance builder on the MI355X, so that its callers — the loop
    closure, slam/loop_closure.py:294, and `ElevationImageInitialization`, slam/initialization.py:176 — rasterise on the device.
    `factory(instance)` returns an object with `build_image(pc)`; the default builds an `engine.ElevationImage` from the
    instance's H, W, pixel_size, z_min, z_max, flip_axis and color_map.  A builder is made again when one of those settings
    changes.  Returns the patched class, or None where the reference does not define it."""
    try:
        import slam.common.registration as ref_registration
    except ImportError:
        return None
    cls = getattr(ref_registration, "ElevationImageRegistration", None)
    if cls is None:
        return None
    make = factory or _DeviceElevationBuilder

    def build_image(self, pc):
        key = (self.H, self.W, self.pixel_size, self.z_min, self.z_max, bool(self.flip_axis), id(self.color_map))
        held = self.__dict__.get("_mi355x_elevation")
        if held is None or held[0] != key:
            held = (key, make(self))
            self.__dict__["_mi355x_elevation"] = held
        return held[1].build_image(pc)

    build_image.__doc__ = "Builds an elevation image (on the MI355X: pylidar_slam_amd.register.install_elevation_image)"
    cls.build_image = build_image
    return cls


class _DeviceCloudRefiner:
    """The default refiner of `install_loop_closure_refinement`: a `CloudRefiner` on a context shared by all of them, recreated
    with more room when a cloud has more rows than it takes."""
    _ctx = None

    def __init__(self, owner=None):
        self.owner, self.refiner = owner, None

    def refine(self, candidate_pc, target_pc, initial_transform, max_distance):
        from .engine import IcpContext
        rows_t, rows_s = int(target_pc.shape[0]), int(candidate_pc.shape[0])
        r = self.refiner
        if r is None or rows_t > r.max_target_rows or rows_s > r.max_source_rows:
            if _DeviceCloudRefiner._ctx is None:
                _DeviceCloudRefiner._ctx = IcpContext()
            if r is not None:
                r.close()
            room = 1 << max(17, (max(rows_t, rows_s, 1) - 1).bit_length())
            r = self.refiner = _DeviceCloudRefiner._ctx.cloud_refiner(room, room, 1.0)
        r.set_target(target_pc)
        return r.refine(candidate_pc, init=initial_transform, max_distance=max_distance)


def compute_transform(self, initial_transform, candidate_pc, target_pc, factory=None):
    """`ElevationImageLoopClosure._compute_transform` (slam/loop_closure.py:210-225) on the MI355X: the point-to-point ICP of
    `candidate_pc` against `target_pc` from `initial_transform`, bound `self.config.icp_distance_threshold` (1.0 where `self`
    has no such setting), 30 iterations, 1e-6 / 1e-6; returns `(np.linalg.inv(T), candidate_pc, target_pc)` as the reference
    does, the inverse taken on the host in float64.  `self` keeps its refiner (made by `factory(self)`, by default a
    `CloudRefiner` on a shared context); any object that takes attributes will do."""
    import numpy as np
    held = getattr(self, "_mi355x_refiner", None)
    if held is None:
        held = (factory or _DeviceCloudRefiner)(self)
        self._mi355x_refiner = held
    bound = float(getattr(getattr(self, "config", None), "icp_distance_threshold", 1.0))
    result = held.refine(np.ascontiguousarray(candidate_pc, dtype=np.float32), np.ascontiguousarray(target_pc, dtype=np.float32),
                         np.asarray(initial_transform, dtype=np.float64), bound)
    return np.linalg.inv(result.transformation), candidate_pc, target_pc


def install_loop_closure_refinement(factory=None):
    """Assigns the reference's `ElevationImageLoopClosure` (slam/loop_closure.py:122-; the class exists only where `cv2` does)
    the `_compute_transform` above, and switches the module's Open3D guard (`_with_o3d`, tested at :237) on.  The config field
    `EILoopClosureConfig.with_icp_refinement` took its default from that guard when the class was defined: without Open3D it is
    False and has to be set to True by the user for the refinement to run.  `factory(instance)` returns an object with `refine(candidate_pc, target_pc, initial_transform,
    max_distance)` whose result has a `transformation`.  Returns the patched class, or None where the reference does not define
    it."""
    try:
        import slam.loop_closure as ref_loop_closure
    except ImportError:
        return None
    cls = getattr(ref_loop_closure, "ElevationImageLoopClosure", None)
    if cls is None:
        return None

    def _compute_transform(self, initial_transform, candidate_pc, target_pc):
        return compute_transform(self, initial_transform, candidate_pc, target_pc, factory)

    _compute_transform.__doc__ = "Refines the 2-D alignment (on the MI355X: pylidar_slam_amd.register.install_loop_closure_refinement)"
    cls._compute_transform = _compute_transform
    ref_loop_closure._with_o3d = True
    return cls
