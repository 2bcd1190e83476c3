"""The four one-call plugin paths (`one_call_frame` / `one_call_projective_frame`, single and batched) against a recording
stand-in for `IcpContext` / `IcpBatch`: which methods the plugin calls, in which order and with what, and what it makes of
the `FrameResult`s it gets back — the call log, the dict outputs, the pose chains, `_iter` and what a key frame records
(`local_map._last_vmap`; `local_map._last_count`, asserted on the batched kd-tree path), all against literals.  Three numpy
frames of 8 rows per sequence (frame 1 has a NaN row, frame 2 arrives as float64), scripted results: frame 0, a pose-only
frame, a key frame; once with and once without `distorted` in the dict.  No GPU, no library: the cuda-tensor branches assert
`is_cuda` and stay with the GPU tests."""
import inspect

import numpy as np
import pytest
import torch

import pylidar_slam_amd.odometry as odo_mod
from pylidar_slam_amd.engine import FrameResult, RegisterResult

H, W = 4, 8
PROJECTIVE = dict(type="projective_local_map", local_map_size=3)
# scripted poses: pure translations by binary fractions (exact in float32 and float64)
T1, T2 = (0.0625, 0.0, 0.0), (0.5, 0.25, 0.0)


def _pose(t):
    m = np.eye(4, dtype=np.float32)
    m[:3, 3] = t
    return m


def _register(t, iterations):
    return RegisterResult(_pose(t), np.array([*t, 0, 0, 0], np.float32), iterations, True, 8, 0,
                          np.zeros(iterations), np.zeros((iterations, 6), np.float32))


def _scripted(k, member=0):
    """The result of frame k: frame 0 (the identity, in the map), a pose-only frame, a key frame."""
    if k == 0:
        return FrameResult(_register((0.0, 0.0, 0.0), 0), 0, True, 8, 8, None)
    if k == 1:
        return FrameResult(_register(T1, 3), 1, False, 8, 0, None)
    return FrameResult(_register(T2, 5), 2, True, 8, 7 - member, None)


def _describe(v):
    if isinstance(v, np.ndarray):
        return ("ndarray", v.shape, v.dtype.name)
    if isinstance(v, torch.Tensor):
        return ("tensor", tuple(v.shape), str(v.dtype))
    if isinstance(v, (list, tuple)):
        return [_describe(x) for x in v]
    if isinstance(v, (np.floating, np.integer, np.bool_)):
        return v.item()
    return v


class _Recorder:
    """Logs `(who.method, {parameter: description})` with the arguments bound to the method's own parameter names, so that
    a positional and a keyword call read the same."""
    LOG = None
    COUNT = 0

    def _log(self, name, values):
        values = {k: _describe(v) for k, v in values.items() if k != "self"}
        _Recorder.LOG.append((f"{self.who}.{name}", values))


def _recorded(fn):
    sig = inspect.signature(fn)

    def wrapper(self, *a, **k):
        bound = sig.bind(self, *a, **k)
        bound.apply_defaults()
        args = dict(bound.arguments)
        for name, p in sig.parameters.items():
            if p.kind is inspect.Parameter.VAR_KEYWORD:
                args.update(args.pop(name))
        self._log(fn.__name__, args)
        return fn(self, *a, **k)

    return wrapper


class RecordingContext(_Recorder):
    def __init__(self, height=64, width=1024, device=0, **kw):
        self.who = f"ctx{_Recorder.COUNT}"
        _Recorder.COUNT += 1
        self.device = torch.device("cpu")
        self.frame = 0
        self.projected = []

    def register(self, *a, **k):  # (what makes a context a context for the local maps; never called on these paths)
        raise RuntimeError("must not be reached")

    @_recorded
    def use_torch_stream(self):
        pass

    @_recorded
    def map_init(self):
        pass

    @_recorded
    def pmap_init(self):
        pass

    @_recorded
    def odometry_init(self, voxel_size=0.0, threshold_trans=0.1, threshold_rot=0.3, constant_velocity=True, targets=0,
                      copy_cloud=True, stage_max_rows=32768):
        self.frame = 0

    @_recorded
    def pmap_odometry_init(self, voxel_size=0.0, threshold_trans=0.1, threshold_rot=0.3, constant_velocity=True, targets=0,
                           normals_kernel_size=5, copy_cloud=True):
        self.frame = 0

    @_recorded
    def frame_launch(self, points, timestamps=None, init_pose=None):
        pass

    @_recorded
    def pmap_frame_launch(self, data, timestamps=None, init_pose=None):
        pass

    def _end(self):
        self.frame += 1
        return _scripted(self.frame - 1)

    @_recorded
    def frame_end(self, with_points=None, cap=None):
        return self._end()

    @_recorded
    def pmap_frame_end(self, with_points=None, cap=None):
        return self._end()

    @_recorded
    def project(self, points, with_index=False, out=None):
        self.projected.append(np.full((3, H, W), float(len(self.projected)), np.float32))
        return self.projected[-1]


class RecordingBatch(_Recorder):
    def __init__(self, contexts):
        self.who = "batch"
        self.contexts = list(contexts)
        self.frame = 0

    @_recorded
    def use_torch_stream(self):
        pass

    @_recorded
    def odometry_init(self, **kw):
        self.frame = 0

    @_recorded
    def pmap_odometry_init(self, **kw):
        self.frame = 0

    @_recorded
    def frame_launch(self, scans, timestamps=None, init_poses=None, skip=None):
        pass

    @_recorded
    def pmap_frame_launch(self, frames, timestamps=None, init_poses=None, skip=None):
        pass

    def _end(self):
        self.frame += 1
        return [_scripted(self.frame - 1, b) for b in range(len(self.contexts))]

    @_recorded
    def frame_end(self, with_points=None, cap=None):
        return self._end()

    @_recorded
    def pmap_frame_end(self, with_points=None, cap=None):
        return self._end()


@pytest.fixture
def recording(monkeypatch):
    monkeypatch.setattr(odo_mod, "IcpContext", RecordingContext)
    monkeypatch.setattr(odo_mod, "IcpBatch", RecordingBatch)
    _Recorder.LOG, _Recorder.COUNT = [], 0
    yield _Recorder.LOG
    _Recorder.LOG = None


def _frames(seed):
    rng = np.random.default_rng(seed)
    f = [rng.normal(size=(8, 3)).astype(np.float32) * 10 for _ in range(3)]
    f[1][5, 1] = np.nan
    f[2] = f[2].astype(np.float64)
    return f


ROWS32, POSE44 = ("ndarray", (8, 3), "float32"), ("ndarray", (4, 4), "float32")
KD_INIT = dict(voxel_size=0.0, threshold_trans=0.1, threshold_rot=0.3, constant_velocity=False, targets=0, copy_cloud=False,
               stage_max_rows=32768)
PMAP_INIT = dict(voxel_size=0.0, threshold_trans=0.1, threshold_rot=0.3, constant_velocity=False, targets=0,
                 normals_kernel_size=5, copy_cloud=False)
# the chain of absolute poses: float64 products of the scripted translations
ABS = [np.eye(4), np.eye(4), np.eye(4)]
ABS[1][:3, 3] = (0.0625, 0.0, 0.0)
ABS[2][:3, 3] = (0.5625, 0.25, 0.0)


def _check_outputs(odo, dicts, frames, distorted, tokens):
    """What the plugin made of the three scripted results of one sequence."""
    assert odo._iter == 3
    assert len(odo.relative_poses) == 3 and all(p.shape == (1, 4, 4) and p.dtype == np.float32 for p in odo.relative_poses)
    rel = np.concatenate(odo.relative_poses)
    assert np.array_equal(rel[0], np.eye(4)) and np.array_equal(rel[1], _pose(T1)) and np.array_equal(rel[2], _pose(T2))
    assert len(odo.absolute_poses) == 3 and all(p.dtype == np.float64 for p in odo.absolute_poses)
    for got, want in zip(odo.absolute_poses, ABS):
        assert np.array_equal(got, want)
    # frame 0 writes nothing into its dict (the reference returns before it does, icp_odometry.py:176-181)
    assert "odometry_pc" not in dicts[0] and "odometry_pose" not in dicts[0]
    for k, t in ((1, T1), (2, T2)):
        d = dicts[k]
        assert d["odometry_pose"].shape == (4, 4) and np.array_equal(d["odometry_pose"], _pose(t))
        assert d["odometry_pose"] is not odo.relative_poses[k]
        if distorted:
            assert d["odometry_pc"] is tokens[k]  # the de-skewed frame stands in, as it is
        else:
            want = np.ascontiguousarray(frames[k], np.float32)
            want = want[~np.isnan(want).any(axis=1)]
            assert d["odometry_pc"].dtype == np.float32 and d["odometry_pc"].shape == ((7, 3) if k == 1 else (8, 3))
            assert np.array_equal(d["odometry_pc"], want)
            assert not np.shares_memory(d["odometry_pc"], frames[k])  # a fresh array per frame
    assert odo.last_result.iterations == 5 and odo._sample_pointcloud is True


def _dicts(frames, distorted):
    tokens = [np.zeros((2, 3), np.float32) for _ in frames]
    dicts = [{"numpy_pc": f, **({"distorted": t} if distorted else {})} for f, t in zip(frames, tokens)]
    return dicts, tokens


@pytest.mark.parametrize("distorted", [False, True])
def test_single_kdtree_one_call_path(recording, distorted):
    odo = odo_mod.MI355XICPFrameToModel(odo_mod.MI355XICPConfig(one_call_frame=True, data_key="numpy_pc"),
                                        projector=odo_mod.SphericalProjector(H, W), device=torch.device("cpu"))
    odo.init()
    frames = _frames(1)
    dicts, tokens = _dicts(frames, distorted)
    for d in dicts:
        odo.process_next_frame(d)
    assert recording == [
        ("ctx0.map_init", {}),
        ("ctx0.use_torch_stream", {}),
        ("ctx0.odometry_init", KD_INIT),
        ("ctx0.frame_launch", dict(points=ROWS32, timestamps=None, init_pose=None)),
        ("ctx0.frame_end", dict(with_points=False, cap=None)),
        ("ctx0.use_torch_stream", {}),
        ("ctx0.frame_launch", dict(points=ROWS32, timestamps=None, init_pose=POSE44)),
        ("ctx0.frame_end", dict(with_points=False, cap=None)),
        ("ctx0.use_torch_stream", {}),
        ("ctx0.frame_launch", dict(points=ROWS32, timestamps=None, init_pose=POSE44)),
        ("ctx0.frame_end", dict(with_points=False, cap=None)),
    ]
    _check_outputs(odo, dicts, frames, distorted, tokens)
    assert len(odo.elapsed) == 3


@pytest.mark.parametrize("distorted", [False, True])
def test_single_projective_one_call_path(recording, distorted):
    odo = odo_mod.MI355XICPFrameToModel(
        odo_mod.MI355XICPConfig(one_call_projective_frame=True, data_key="numpy_pc", local_map=PROJECTIVE),
        projector=odo_mod.SphericalProjector(H, W), device=torch.device("cpu"))
    odo.init()
    frames = _frames(2)
    dicts, tokens = _dicts(frames, distorted)
    for d in dicts:
        odo.process_next_frame(d)
    project = ("ctx0.project", dict(points=ROWS32, with_index=False, out=None))
    assert recording == [
        ("ctx0.pmap_init", {}),
        ("ctx0.use_torch_stream", {}),
        ("ctx0.pmap_odometry_init", PMAP_INIT),
        ("ctx0.pmap_frame_launch", dict(data=ROWS32, timestamps=None, init_pose=None)),
        ("ctx0.pmap_frame_end", dict(with_points=False, cap=None)),
        project,  # frame 0 is a key frame: `_last_vmap` is recorded before the early return
        ("ctx0.use_torch_stream", {}),
        ("ctx0.pmap_frame_launch", dict(data=ROWS32, timestamps=None, init_pose=POSE44)),
        ("ctx0.pmap_frame_end", dict(with_points=False, cap=None)),
        ("ctx0.use_torch_stream", {}),
        ("ctx0.pmap_frame_launch", dict(data=ROWS32, timestamps=None, init_pose=POSE44)),
        ("ctx0.pmap_frame_end", dict(with_points=False, cap=None)),
        project,
    ]
    _check_outputs(odo, dicts, frames, distorted, tokens)
    assert len(odo.ctx.projected) == 2 and odo.local_map._last_vmap is odo.ctx.projected[1]


def _batch_log(prefix, init, frames_name, n_members, projects):
    """The call log of three batched steps of `n_members` sequences; `projects`: the steps behind which every member's
    context projects its frame (the projective key frames)."""
    rows, poses = [ROWS32] * n_members, [POSE44] * n_members
    log = [(f"ctx{b}.{'pmap_init' if prefix else 'map_init'}", {}) for b in range(n_members)]
    for step in range(3):
        if step == 0:
            log += [("batch.use_torch_stream", {}), (f"batch.{prefix}odometry_init", init)]
        log += [(f"batch.{prefix}frame_launch", {frames_name: rows, "timestamps": None,
                                                   "init_poses": None if step == 0 else poses, "skip": None}),
                (f"batch.{prefix}frame_end", dict(with_points=[False] * n_members, cap=None))]
        if step in projects:
            log += [(f"ctx{b}.project", dict(points=ROWS32, with_index=False, out=None)) for b in range(n_members)]
    return log


@pytest.mark.parametrize("distorted", [False, True])
def test_batched_kdtree_one_call_path(recording, distorted):
    odo = odo_mod.MI355XICPFrameToModelBatch(odo_mod.MI355XICPConfig(one_call_frame=True, data_key="numpy_pc"), 2,
                                             projector=odo_mod.SphericalProjector(H, W), device=torch.device("cpu"))
    odo.init()
    frames = [_frames(3), _frames(4)]
    made = [_dicts(f, distorted) for f in frames]
    for k in range(3):
        odo.process_next_frames([made[b][0][k] for b in range(2)])
    assert recording == _batch_log("", KD_INIT, "scans", 2, ())
    assert odo._iter == 3 and len(odo.elapsed) == 3
    for b, m in enumerate(odo.members):
        _check_outputs(m, made[b][0], frames[b], distorted, made[b][1])
        assert m.local_map._last_count == 7 - b  # what the key frame (frame 2) inserted; the pose-only frame left it alone


@pytest.mark.parametrize("distorted", [False, True])
def test_batched_projective_one_call_path(recording, distorted):
    odo = odo_mod.MI355XICPFrameToModelBatch(
        odo_mod.MI355XICPConfig(one_call_projective_frame=True, data_key="numpy_pc", local_map=PROJECTIVE), 2,
        projector=odo_mod.SphericalProjector(H, W), device=torch.device("cpu"))
    odo.init()
    frames = [_frames(5), _frames(6)]
    made = [_dicts(f, distorted) for f in frames]
    for k in range(3):
        odo.process_next_frames([made[b][0][k] for b in range(2)])
    assert recording == _batch_log("pmap_", PMAP_INIT, "frames", 2, (0, 2))
    assert odo._iter == 3 and len(odo.elapsed) == 3
    for b, m in enumerate(odo.members):
        _check_outputs(m, made[b][0], frames[b], distorted, made[b][1])
        assert len(m.ctx.projected) == 2 and m.local_map._last_vmap is m.ctx.projected[1]


# ---- the map bookkeeping every one-call path keeps (on the commit before the paths were folded the single kd-tree path kept
# ---- none of it, and no kd-tree path recorded frame 0's insertion) --------------------------------------------------------------
@pytest.mark.parametrize("flag,local_map", [("one_call_frame", None), ("one_call_projective_frame", PROJECTIVE)])
@pytest.mark.parametrize("batched", [False, True])
def test_one_call_paths_keep_delta_and_last_count(recording, flag, local_map, batched):
    """`_delta_since_map_update` after every frame (the identity behind a key frame, delta @ pose behind a pose-only frame) and,
    kd-tree map, `local_map._last_count` = what the last key frame inserted, frame 0 included (`get_last_frame` reads it)."""
    kw = dict(data_key="numpy_pc", **{flag: True}, **({"local_map": local_map} if local_map else {}))
    cfg, proj, cpu = odo_mod.MI355XICPConfig(**kw), odo_mod.SphericalProjector(H, W), torch.device("cpu")
    if batched:
        odo = odo_mod.MI355XICPFrameToModelBatch(cfg, 2, projector=proj, device=cpu)
        members, step = odo.members, lambda k: odo.process_next_frames([{"numpy_pc": f[k]} for f in frames])
    else:
        odo = odo_mod.MI355XICPFrameToModel(cfg, projector=proj, device=cpu)
        members, step = [odo], lambda k: odo.process_next_frame({"numpy_pc": frames[0][k]})
    odo.init()
    frames = [_frames(7 + b) for b in range(len(members))]
    want_delta = [np.eye(4, dtype=np.float32), _pose(T1), np.eye(4, dtype=np.float32)]
    for k in range(3):
        step(k)
        for b, m in enumerate(members):
            assert m._delta_since_map_update.dtype == np.float32 and np.array_equal(m._delta_since_map_update, want_delta[k])
            if local_map is None:
                assert m.local_map._last_count == [8, 8, 7 - b][k]
