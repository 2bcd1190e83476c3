"""GPU side of the audit of calls beside work in flight: the library run through the scenario runner of tests/inflight_audit.py,
one test per table row and in-flight state.  Every class was derived from the source first (the table); a run here confirms a
cell, it is not used to find out what an unpredictable call does.

Each cell runs the scenario twice on fresh contexts — under test with "chunked_launch" 1, the twin with 0 — and compares, bit
for bit, pose, parameters, losses, steps, iteration count, convergence and num_targets of every registration or frame, the map,
its cloud count and normal cache afterwards, the next registration on the same context, and the call's own output (see
inflight_audit.run_cell for the twin of each class).  ORDERED rows whose call can change a registration also run the control: the
call made BEFORE the launch must change it.  The `held` cells assert that the twin's jump ran at least k1 + 3 iterations, so
iterations WERE held back when the call was made.

Shapes: 16 x 512 scans, a fixed map of 10 000 points, max_num_alignments 20, geman_mcclure / 0.3, local_map_size 3: the
smallest at which chunking exists (inflight_audit.kd_fixture; tests/test_inflight_audit.py asserts the hold-back on the CPU).

Every scenario closes on `registering_contexts() == 0` once its contexts are closed (GpuRig.close): whatever the call under test
did, refusals and error exits included, nothing of it stays in the device's count of registering contexts
(tests/neighbour_audit.py holds that count call by call).

THE OVERLAPPED STATE is one fixed sequence, run once: a pass shows no race on that run and proves no absence of one.
"""
import ctypes as C
import os
import sys
import time
from types import SimpleNamespace

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import inflight_audit as A  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (no CPU fallback exists for the product path)")
    return torch


@pytest.fixture(scope="module")
def env(torch_cuda):
    """The scene, its device copies and the arguments of every recipe, built once."""
    torch = torch_cuda
    from pylidar_slam_amd.engine import IcpContext
    fx = A.kd_fixture()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    e = SimpleNamespace(torch=torch, fx=fx, cache={}, started=time.perf_counter(), cells=0, controls=0)
    e.scans = [dev(s) for s in fx["scans"]]
    e.map, e.map2 = dev(fx["map"]), dev(fx["map2"])
    e.short, e.jump, e.second, e.next = (e.scans[i] for i in (A.SHORT_FRAME, A.JUMP_FRAME, A.SECOND_FRAME, A.NEXT_FRAME))
    rng = np.random.default_rng(31)
    cloud = fx["scans"][5].copy()
    cloud[rng.integers(0, len(cloud), 150)] = np.nan
    cloud[rng.integers(0, len(cloud), 150)] = 0.0
    e.cloud_np, e.cloud = cloud, dev(cloud)
    e.shift = np.eye(4, dtype=np.float32)
    e.shift[:3, 3] = (0.3, -0.2, 0.05)
    nrm = rng.normal(size=(4 * A.HEIGHT * A.WIDTH, 4)).astype(np.float32)  # (at least any map of these cells)
    nrm[:, :3] /= np.linalg.norm(nrm[:, :3], axis=1, keepdims=True)
    nrm[:, 3] = 1.0
    e.normals = dev(nrm)
    e.host_rows = np.ascontiguousarray(fx["scans"][8][1000:5000])
    e.host_rows2 = np.ascontiguousarray(fx["scans"][9][1000:5000])
    e.dev_rows = dev(e.host_rows)
    e.records = np.ascontiguousarray(np.concatenate([e.host_rows, np.ones((len(e.host_rows), 1), np.float32)], axis=1))
    e.stamps = np.linspace(0.0, 0.1, len(e.host_rows))
    e.motion = np.eye(4)
    e.motion[:3, 3] = (0.4, 0.01, 0.0)
    # what depends on the image size: vertex maps for the recipes, and the projective drive of the 17 x 33 states
    from pylidar_slam_amd.synthetic import SceneConfig, make_sequence, pose_matrix
    e.geo = {}
    for h, w in ((A.HEIGHT, A.WIDTH), (17, 33)):
        scratch = IcpContext(height=h, width=w)
        g = SimpleNamespace(height=h, width=w)
        g.vmap_np, g.vmap2_np = (np.ascontiguousarray(scratch.project(fx["scans"][k])) for k in (8, 9))  # (numpy in, numpy out)
        g.vmap = dev(g.vmap_np)
        drive, _ = make_sequence(SceneConfig(height=h, width=w), 6)
        g.vmaps = [scratch.project(dev(sc)).clone() for sc in drive]
        g.rows = [v.permute(1, 2, 0).reshape(-1, 3).contiguous() for v in g.vmaps]
        g.step = pose_matrix(np.array([0.4, 0.0, 0.0, 0.0, 0.0, 0.01])).astype(np.float32)
        torch.cuda.synchronize()
        scratch.close()
        e.geo[(h, w)] = g
    e.side = torch.cuda.Stream()
    e.lut = rng.integers(0, 256, (259, 3)).astype(np.uint8)
    yield e
    torch.cuda.synchronize()
    print(f"\ninflight audit: {e.cells} cells, {e.controls} with a control, {time.perf_counter() - e.started:.1f} s")


def _bits(x):
    """Anything a call returns -> hashable bits."""
    if x is None or isinstance(x, (int, float, str, bool, bytes)):
        return x
    if isinstance(x, np.ndarray):
        return (x.dtype.str, x.shape, x.tobytes())
    if hasattr(x, "detach"):
        return _bits(x.detach().cpu().numpy())
    if isinstance(x, dict):
        return tuple((k, _bits(v)) for k, v in sorted(x.items()))
    if isinstance(x, (tuple, list)):
        return tuple(_bits(v) for v in x)
    raise TypeError(type(x))


def _reg(r):
    return A.Result((_bits(r.pose), _bits(r.params), _bits(r.losses), _bits(r.dx), int(r.iterations), bool(r.converged),
                     int(r.num_targets)), int(r.iterations))


def _frame(f):
    return A.Result(_reg(f.register).bits + (int(f.frame_index), bool(f.key_frame), int(f.samples), int(f.inserted), _bits(f.points)),
                    int(f.register.iterations))


# ---- the recipes: arguments chosen to have teeth where the call can have any -----------------------------------------------------
def _r_set_stream(rig):
    with rig.env.torch.cuda.stream(rig.env.side):
        rig.ctx.use_torch_stream()  # (icp_set_stream to a side stream; the next call with a device tensor switches back)


def _r_neq_buffer(rig):
    t = rig.env.torch.full((32,), -7.0, dtype=rig.env.torch.float64, device="cuda")
    rig.keep.append(t)
    rig.ctx._check(rig.ctx._lib.icp_set_normal_equations_buffer(rig.ctx._h, C.c_void_p(t.data_ptr())))
    # (no iteration of the registration in flight may write it: read right behind that registration's end)
    rig.probes.append(lambda: _bits(t))


def _r_stage(rig):
    rig.ctx.map_stage_cloud(rig.env.cloud, skip_null=True)
    rig.staged_by_x = True


def _r_launch(rig, init):
    rig.ctx.register_launch(rig.env.second, init)
    rig.pending += 1


def _r_pmap_search(rig):
    if rig.ctx.pmap_num_maps() == 0:  # (a kd-tree context: the search needs a projective map — icp_pmap_update is INDEPENDENT there)
        rig.ctx.pmap_update(np.eye(4, dtype=np.float32), rig.g.vmap_np)
    return rig.ctx.pmap_nearest_neighbor_search(rig.env.host_rows2)  # host rows: staged through ctx->targets


def _r_objects(rig):
    """An aggregated map, an elevation image and a refiner, created, fed, read through EVERY entry point of theirs and closed:
    icp_aggmap_insert / _stats / _get / _get_f64 / _submap / _clear, icp_elevation_build / _build_aggmap / _get / _stats,
    icp_refine_set_target / _image_rows / _launch / _end / _history."""
    e, c = rig.env, rig.ctx
    m = c.aggregated_map(0.5, 20000, 8192)
    m.insert(e.host_rows, np.eye(4), 0)
    m.insert(e.dev_rows, e.motion, 1)
    out = [m.points(), m.points(dtype=np.float64), m.stats(), m.submap(0, 2, np.eye(4))]
    img = c.elevation_image(64, 64, 0.5, -3.0, 3.0, color_map=e.lut, max_rows=8192)
    img.build(e.dev_rows)
    out += [img.theta, img.indices, img.stats()]
    img2 = c.elevation_image(64, 64, 0.5, -3.0, 3.0, color_map=e.lut, max_rows=8192)
    img2.build_from(m, 0, 2, np.eye(4))
    out += [img2.theta, img2.stats()]
    r = c.cloud_refiner(8192, 8192)
    r.set_target(img)                     # (icp_refine_image_rows: the image's device points in place)
    res = r.refine(img2, max_iteration=2)
    out += [res.transformation, res.fitness, res.iterations]
    r.set_target(e.host_rows)
    res = r.refine(e.dev_rows, max_iteration=3)
    out += [res.transformation, res.fitness, res.inlier_rmse, res.iterations, res.correspondences, r.history()]
    m.clear()
    out.append(m.stats())
    for o in (r, img2, img, m):
        o.close()
    return out


# ---- the batched forms: member 0 is the context in the state, two idle members (a map, one collected registration) beside it
def _b3(x):
    return [x] * BATCH


def _r_batch_stage(rig):
    rig.bx().stage(_b3(rig.env.cloud), skip_null=True)
    rig.staged_by_x = True


def _r_batch_launch(rig):
    rig.bx().register_launch([rig.env.second, rig.env.short, rig.env.short])
    rig.pending += 1
    rig.batch_pending = True


def _r_batch_set_stream(rig):
    with rig.env.torch.cuda.stream(rig.env.side):
        rig.bx().use_torch_stream()


def _r_batch_project(rig):
    g = rig.g
    outs = [rig.env.torch.empty((3, g.height, g.width), dtype=rig.env.torch.float32, device="cuda") for _ in range(BATCH)]
    return rig.bx().project(_b3(rig.env.dev_rows), outs)


def _r_exchange_connect(rig):
    rig.ctx._check(rig.ctx._lib.icp_exchange_connect(rig.ctx._h, C.c_char_p(b"\0" * 64)))


EYE = np.eye(4, dtype=np.float32)
RECIPES = {
    # ---- ICP_HELD_FIRST, then the change
    "icp_set_stream": _r_set_stream,
    "icp_set_option": lambda r: r.ctx.set_option("prune_guard", 0.004),
    "icp_set_cost": lambda r: r.ctx.set_cost("point_to_point_gauss_newton"),
    "icp_set_alignment": lambda r: r.ctx.set_alignment("huber", 0.5, A.MAX_ITERATIONS, r.threshold),
    "icp_set_normal_equations_buffer": _r_neq_buffer,
    "icp_map_init": lambda r: r.ctx.map_init(),
    "icp_map_set": lambda r: r.ctx.map_set(r.env.map2),
    "icp_map_update": lambda r: r.ctx.map_update(r.env.shift, r.env.cloud, skip_null=True),
    "icp_map_update_vertex_map": lambda r: r.ctx.map_update_vertex_map(r.env.shift, r.g.vmap),
    "icp_map_stage_cloud": _r_stage,
    "icp_map_update_staged": lambda r: r.ctx.map_update_staged(r.env.shift),
    "icp_map_normals_owned": lambda r: r.ctx.map_normals_owned(0, 1),
    "icp_map_normals_install": lambda r: r.ctx.map_normals_install(r.env.normals[:r.ctx.map_size()]),
    "icp_register_launch": lambda r: _r_launch(r, None),
    "icp_register_launch_from_last": lambda r: _r_launch(r, "last"),
    "icp_odometry_init": lambda r: r.ctx.odometry_init(),
    # ---- refused
    "icp_estimate_timestamps": lambda r: r.ctx.estimate_timestamps(r.env.dev_rows),
    "icp_kitti360_prepare": lambda r: r.ctx.kitti360_prepare(r.env.records),
    "icp_align_point_to_plane": lambda r: r.ctx.align_point_to_plane(r.env.host_rows, r.env.host_rows2, r.env.host_rows),
    "icp_align_point_to_point": lambda r: r.ctx.align_point_to_point(r.env.host_rows, r.env.host_rows2),
    "icp_weighted_procrustes": lambda r: r.ctx.weighted_procrustes(r.env.host_rows2, r.env.host_rows),
    "icp_nearest_neighbor_search": lambda r: r.ctx.nearest_neighbor_search(r.env.host_rows),
    "icp_knn_query": lambda r: r.ctx.knn_query(r.env.host_rows, k=3),
    "icp_map_normals_peek": lambda r: r.ctx.map_normals_peek(),
    "icp_last_neighbors": lambda r: r.ctx.last_neighbors(A.HEIGHT * A.WIDTH),
    "icp_last_cache_entries": lambda r: r.ctx.last_cache_entries(A.HEIGHT * A.WIDTH),
    "icp_register": lambda r: r.ctx.register(r.env.second),
    "icp_register_begin": lambda r: r.ctx.register_begin(r.env.second),
    "icp_pmap_register": lambda r: r.ctx.pmap_register(r.env.second),
    "icp_pmap_register_launch": lambda r: r.ctx.pmap_register_launch(r.env.second),
    "icp_iteration_accumulate": lambda r: r.ctx.iteration_accumulate(),
    "icp_iteration_solve": lambda r: r.ctx.iteration_solve(),
    "icp_frame_launch": lambda r: r.ctx.frame_launch(r.env.second),
    "icp_frame_end": lambda r: r.ctx.frame_end(with_points=False),
    "icp_pmap_frame_launch": lambda r: r.ctx.pmap_frame_launch(r.env.second),
    "icp_pmap_frame_end": lambda r: r.ctx.pmap_frame_end(with_points=False),
    "icp_pmap_odometry_init": lambda r: r.ctx.pmap_odometry_init(),
    "icp_exchange_create": lambda r: r.ctx.exchange_create(0, 1),
    "icp_exchange_connect": _r_exchange_connect,
    "icp_exchange_destroy": lambda r: r.ctx.exchange_destroy(),
    "icp_register_end": lambda r: _reg(r.ctx.register_end()),
    "icp_pmap_init": lambda r: r.ctx.pmap_init(),
    "icp_pmap_update": lambda r: r.ctx.pmap_update(r.g.step, r.g.vmap_np),
    "icp_pmap_get_model": lambda r: r.ctx.pmap_model(),
    # ---- independent: host inputs where the entry point stages (stage_in, ctx->targets), device inputs otherwise
    "icp_project": lambda r: (r.ctx.project(r.env.host_rows), r.ctx.project(r.env.dev_rows, with_index=True)),
    "icp_project_rows": lambda r: r.ctx.project_rows(r.env.dev_rows),
    "icp_project_pixels": lambda r: r.ctx.project_pixels(r.env.host_rows),
    "icp_kitti_correct_scan": lambda r: r.ctx.kitti_correct_scan(r.env.records),
    "icp_voxel_hash": lambda r: r.ctx.voxel_hash(r.env.host_rows, 0.3),
    "icp_grid_sample": lambda r: (r.ctx.grid_sample(r.env.host_rows, 0.3), r.ctx.grid_sample(r.env.dev_rows, 0.3)),
    "icp_grid_sample_f64": lambda r: r.ctx.grid_sample_f64(r.env.host_rows.astype(np.float64), 0.3),
    "icp_grid_sample_padded": lambda r: r.ctx.grid_sample_padded(r.env.dev_rows, 0.3),
    "icp_voxel_statistics": lambda r: r.ctx.voxel_statistics(r.env.host_rows, 0.3),
    "icp_distort": lambda r: r.ctx.distort(r.env.host_rows, r.env.stamps, r.env.motion),
    "icp_compact_targets": lambda r: r.ctx.compact_targets(r.env.cloud, 8192, skip_null=True),
    "icp_synchronize": lambda r: r.ctx.synchronize(),
    "icp_map_get": lambda r: r.ctx.map_points(),
    "icp_compute_normal_map": lambda r: r.ctx.compute_normal_map(r.g.vmap_np),
    "icp_compute_neighbors": lambda r: r.ctx.compute_neighbors(r.g.vmap_np, np.stack([r.g.vmap2_np, r.g.vmap_np])),
    "icp_pmap_nearest_neighbor_search": _r_pmap_search,
    "icp_profile_read": lambda r: (r.ctx.profile_read(), None)[1],
    "icp_grid_sample_padded_f64": lambda r: r.ctx.grid_sample_padded(r.env.dev_rows.double(), 0.3),
    "icp_profile_enable": lambda r: r.ctx.profile_enable(1),
    "icp_profile_read_iterations": lambda r: (r.ctx.profile_read_iterations(8), None)[1],
    "icp_profile_event_floor": lambda r: (r.ctx.profile_event_floor(4), None)[1],
    # ---- the batched forms
    "icp_batch_stage": _r_batch_stage,
    "icp_batch_map_update": lambda r: r.bx().map_update(),
    "icp_batch_map_update_staged": lambda r: r.bx().map_update_staged([1, 0, 0], _b3(r.env.shift)),
    "icp_batch_register_launch": _r_batch_launch,
    "icp_batch_register_end": lambda r: [_reg(x) for x in r.bx().register_end()],
    "icp_batch_set_stream": _r_batch_set_stream,
    "icp_batch_project": _r_batch_project,
    "icp_batch_project_rows": lambda r: r.bx().project_rows(_b3(r.env.dev_rows)),
    "icp_batch_preprocess": lambda r: r.bx().preprocess(_b3(r.env.dev_rows), _b3(None), _b3(None), 0.3),
    "icp_batch_estimate_timestamps": lambda r: r.bx().estimate_timestamps(_b3(r.env.dev_rows)),
    "icp_batch_odometry_init": lambda r: r.bx().odometry_init(),
    "icp_batch_pmap_odometry_init": lambda r: r.bx().pmap_odometry_init(),
    "icp_batch_frame_launch": lambda r: r.bx().frame_launch(_b3(r.env.second)),
    "icp_batch_frame_end": lambda r: r.bx().frame_end(),
    "icp_batch_pmap_frame_launch": lambda r: r.bx().pmap_frame_launch(_b3(r.env.second)),
    "icp_batch_pmap_frame_end": lambda r: r.bx().pmap_frame_end(),
    "icp_batch_pmap_register_launch": lambda r: r.bx().pmap_register_launch(_b3(r.env.second)),
    "icp_batch_pmap_update": lambda r: r.bx().pmap_update(_b3(EYE), None),
}
# the objects of a context: one composite recipe under the name of every entry point it goes through
OBJECT_SYMBOLS = ("icp_aggmap_insert", "icp_aggmap_stats", "icp_aggmap_get", "icp_aggmap_get_f64", "icp_aggmap_submap", "icp_aggmap_clear",
                  "icp_elevation_build", "icp_elevation_build_aggmap", "icp_elevation_get", "icp_elevation_stats",
                  "icp_refine_set_target", "icp_refine_image_rows", "icp_refine_launch", "icp_refine_end", "icp_refine_history")
RECIPES.update({s: _r_objects for s in OBJECT_SYMBOLS})
BATCH_SYMBOLS = sorted(s for s in RECIPES if s.startswith("icp_batch_"))

LIVE_STATES = ("held", "two_pending", "begun", "frame", "pframe", "pmap_launched", "batch_hold")
PROJECTIVE_STATES = ("pframe", "pmap_launched")
BEGUN_PAIRS = 12  # accumulate + solve pairs of the begun state (behind the stop they return at once)
BATCH = 3         # members of the batch_hold state


def _stop_on_a_device_error(what, e):
    """A HIP error (ICP_ERR_HIP, or torch's own) is a finding to be read, not a state to go on testing in: the session ends here
    and starts nothing more on the device."""
    text = str(e)
    if text.rstrip().endswith("(-2)") or "HIP error" in text or "illegal memory access" in text:  # (-2: ICP_ERR_HIP)
        pytest.exit(f"device error in {what}: {text} — nothing more is started on the GPU", returncode=3)


class GpuRig:
    """The runner's rig over an IcpContext (see inflight_audit.run_scenario).  The projective states run on 17 x 33 contexts,
    batch_hold on three 16 x 512 contexts of which member 0 takes the call under test."""

    def __init__(self, env, chunked, state, variant, pre_stage=False, with_sequence=False):
        from pylidar_slam_amd.engine import IcpBatch, IcpContext
        self.env, self.state, self.variant, self.pre_stage, self.with_sequence = env, state, variant, pre_stage, with_sequence
        self.chunked, self.extras, self.batch_pending, self.refusal = chunked, [], False, None
        self.threshold = A.THRESHOLD if state in LIVE_STATES else 0.0
        self.g = env.geo[(17, 33) if state in PROJECTIVE_STATES else (A.HEIGHT, A.WIDTH)]
        kw = dict(height=self.g.height, width=self.g.width, max_num_alignments=A.MAX_ITERATIONS,
                  threshold_delta_pose=self.threshold, scheme=A.SCHEME, sigma=A.SIGMA, local_map_size=A.LOCAL_MAP_SIZE)
        self.kw = kw
        by_batch = state == "batch_hold" or variant == "batch"
        self.members = [self._record(IcpContext(**kw)) for _ in range(BATCH if by_batch else 1)]
        for c in self.members:
            c.set_option("chunked_launch", chunked)
        self.ctx = self.members[0]
        self.batch = self._record(IcpBatch(self.members), True) if by_batch else None
        self.results, self.keep, self.probes, self.probe_bits = [], [], [], ()
        self.hold = {"held": (0, 1), "batch_hold": (0, BATCH)}.get(state)
        self.pending, self.staged_by_x = 0, False

    def _record(self, obj, batch=False):
        """The status and the message of the library's own refusals, taken where the binding receives them: an AssertionError
        of a guard of the Python layer passes through no _check and is no refusal of the library."""
        check = obj._check
        last_error = obj._lib.icp_batch_last_error if batch else obj._lib.icp_last_error

        def recording(rc):
            if rc != 0:
                self.refusal = (int(rc), last_error(obj._h).decode())
            return check(rc)
        obj._check = recording
        return obj

    def bx(self):
        """The batch the batched forms are called on: the state's own, or member 0 with two idle members made now."""
        from pylidar_slam_amd.engine import IcpBatch, IcpContext
        if self.batch is None:
            for _ in range(BATCH - 1):
                m = self._record(IcpContext(**self.kw))
                m.set_option("chunked_launch", self.chunked)
                if self.with_sequence:
                    m.odometry_init()
                m.map_set(self.env.map)
                m.register(self.env.short)
                self.extras.append(m)
            self.batch = self._record(IcpBatch([self.ctx] + self.extras), True)
        return self.batch

    def _do(self, what, fn, *a, **kw):
        try:
            return fn(*a, **kw)
        except AssertionError as e:
            raise A.RigError(f"{what}: {type(e).__name__}: {e}")
        except RuntimeError as e:
            _stop_on_a_device_error(what, e)
            raise A.RigError(f"{what}: {type(e).__name__}: {e}")

    # -- the steps
    def prepare(self):
        c, e, g, s = self.ctx, self.env, self.g, self.state
        key = self.variant != "nonkey"
        if s == "frame" and self.variant == "batch":
            self._do("batch odometry_init", self.batch.odometry_init)
            for f in A.FRAME_PROLOGUE:
                self._do("batch frame_launch", self.batch.frame_launch, [e.scans[f], e.scans[f + 1], e.scans[f + 2]])
                self.results += [_frame(r) for r in self._do("batch frame_end", self.batch.frame_end)]
        elif s == "frame":
            self._do("odometry_init", c.odometry_init, threshold_trans=0.1 if key else 100.0, threshold_rot=0.3 if key else 180.0)
            for f in A.FRAME_PROLOGUE:
                self._do("frame_launch", c.frame_launch, e.scans[f])
                self.results.append(_frame(self._do("frame_end", c.frame_end)))
        elif s == "pframe":
            self._do("pmap_odometry_init", c.pmap_odometry_init, threshold_trans=0.1 if key else 100.0,
                     threshold_rot=0.3 if key else 180.0)
            for f in A.FRAME_PROLOGUE:
                self._do("pmap_frame_launch", c.pmap_frame_launch, g.vmaps[f])
                self.results.append(_frame(self._do("pmap_frame_end", c.pmap_frame_end)))
        elif s == "pmap_launched":
            self._do("pmap_init", c.pmap_init)
            self._do("pmap_update", c.pmap_update, EYE, g.vmaps[0])
            self._do("pmap_update", c.pmap_update, g.step, g.vmaps[1])
            self.results.append(_reg(self._do("pmap_register", c.pmap_register, g.rows[1], None, True)))
        else:
            for m in self.members:
                if self.with_sequence:
                    self._do("odometry_init", m.odometry_init)
                self._do("map_set", m.map_set, e.map)
            if self.pre_stage:
                self._do("stage", c.map_stage_cloud, e.cloud, skip_null=True)
            for m in self.members:
                self.results.append(_reg(self._do("register", m.register, e.short)))

    def enter(self):
        c, e, g, s = self.ctx, self.env, self.g, self.state
        if s in ("held", "pending"):
            self._do("launch", c.register_launch, e.jump, None)
            self.pending = 1
        elif s == "two_pending":
            self._do("launch", c.register_launch, e.jump, None)
            if self.variant == "one_at_a_time":
                self.results.append(_reg(self._do("register_end", c.register_end)))
            else:
                self.pending = 1
            self._do("launch from last", c.register_launch, e.second, "last")
            self.pending += 1
        elif s == "begun":
            self._do("begin", c.register_begin, e.jump)
            for _ in range(2):
                self._do("accumulate", c.iteration_accumulate)
                self._do("solve", c.iteration_solve)
        elif s == "frame" and self.variant == "batch":
            k = A.FRAME_JUMP
            self._do("batch frame_launch", self.batch.frame_launch, [e.scans[k], e.scans[k + 1], e.scans[k + 2]])
        elif s == "frame":
            self._do("frame_launch", c.frame_launch, e.scans[A.FRAME_JUMP])
        elif s == "pframe":
            self._do("pmap_frame_launch", c.pmap_frame_launch, g.vmaps[3])
        elif s == "pmap_launched":
            self._do("pmap_register_launch", c.pmap_register_launch, g.rows[3], None, True)
            self.pending = 1
        elif s == "batch_hold":
            self._do("batch launch", self.batch.register_launch, [e.jump, e.scans[A.JUMP_FRAME - 1], e.second])
        else:
            raise A.RigError(f"no prologue for {s}")

    def call(self, symbol):
        self.refusal = None
        try:
            return A.Outcome(0, "", _bits(RECIPES[symbol](self)))
        except AssertionError as e:
            if self.refusal is None:  # (a guard of the Python layer: the library was never asked)
                return A.Outcome(-99, "", f"raised by the binding, not by the library: {e}")
            return A.Outcome(self.refusal[0], self.refusal[1], str(e))
        except RuntimeError as e:
            _stop_on_a_device_error(symbol, e)
            return A.Outcome(self.refusal[0] if self.refusal else -2, str(e), None)

    def finish(self):
        c, s = self.ctx, self.state
        if s == "frame" and self.variant == "batch":
            self.results += [_frame(r) for r in self._do("batch frame_end", self.batch.frame_end)]
        elif s in ("frame", "pframe"):
            self.results.append(_frame(self._do("frame_end", c.frame_end if s == "frame" else c.pmap_frame_end)))
            while self.pending:  # (a registration the call under test launched beside the frame: collected behind it)
                self.results.append(_reg(self._do("register_end", c.register_end)))
                self.pending -= 1
        elif s == "batch_hold":
            self.results += [_reg(r) for r in self._do("batch end", self.batch.register_end)]
        else:
            if s == "begun":
                for _ in range(BEGUN_PAIRS - 2):
                    self._do("accumulate", c.iteration_accumulate)
                    self._do("solve", c.iteration_solve)
                self.pending = 1
            if self.batch_pending:  # (a batched launch of the call under test: its batch collects member 0's OLDEST result)
                rs = self._do("batch end", self.batch.register_end)
                self.results.append(_reg(rs[0]))
                self.pending -= 1
            while self.pending:
                self.results.append(_reg(self._do("register_end", c.register_end)))
                self.pending -= 1
        self.probe_bits = tuple(p() for p in self.probes)

    def follow(self):
        c, e, g, s = self.ctx, self.env, self.g, self.state
        if self.staged_by_x:  # (what an ORDERED icp_map_stage_cloud leaves behind the registration: its cloud, inserted now)
            self._do("update_staged", c.map_update_staged, e.shift)
        if s == "frame" and self.variant == "batch":
            k = A.FRAME_NEXT
            self._do("batch frame_launch", self.batch.frame_launch, [e.scans[k], e.scans[k + 1], e.scans[k + 2]])
            self.results += [_frame(r) for r in self._do("batch frame_end", self.batch.frame_end)]
        elif s == "frame":
            self._do("frame_launch", c.frame_launch, e.scans[A.FRAME_NEXT])
            self.results.append(_frame(self._do("frame_end", c.frame_end)))
        elif s == "pframe":
            self._do("pmap_frame_launch", c.pmap_frame_launch, g.vmaps[4])
            self.results.append(_frame(self._do("pmap_frame_end", c.pmap_frame_end)))
        elif s == "pmap_launched":
            if c.pmap_num_maps() == 0:  # (behind icp_pmap_init)
                self._do("pmap_update", c.pmap_update, EYE, g.vmaps[0])
            self.results.append(_reg(self._do("pmap_register", c.pmap_register, g.rows[4], None, True)))
        else:
            if c.map_size() == 0:  # (behind icp_map_init / icp_odometry_init: a registration needs a map)
                self._do("map_set", c.map_set, e.map2)
            self.results.append(_reg(self._do("register", c.register, e.next)))

    def snapshot(self):
        out = [self.probe_bits]
        for c in self.members:
            if c.map_size() > 0:
                out += [_bits(self._do("map_points", c.map_points)), c.map_num_clouds(),
                        _bits(self._do("normals_peek", c.map_normals_peek))]
            if c.pmap_num_maps() > 0:
                out += [c.pmap_num_maps(), _bits(self._do("pmap_model", c.pmap_model))]
        return tuple(out)

    def close(self):
        if self.batch is not None:
            self.batch.close()
        for c in self.members + self.extras:
            c.close()
        self.keep.clear()
        # (whatever the scenario did, error exits included: no context of it is left in the device's count of registering contexts)
        from pylidar_slam_amd.engine import registering_contexts
        assert registering_contexts(0) == 0, f"{self.state}: the count of registering contexts is left at {registering_contexts(0)}"


# ---- the cells: every row with a recipe in the kd-tree states and the key frame; the frame that is no key frame and the projective
# states take the rows whose class, message or buffers differ there ----------------------------------------------------------------
_SINGLE = sorted(s for s in RECIPES if s not in OBJECT_SYMBOLS[1:] and not s.startswith("icp_batch_"))
PER_STATE = {
    ("held", None): sorted(RECIPES),
    ("pending", None): _SINGLE + ["icp_batch_stage", "icp_batch_map_update", "icp_batch_project_rows", "icp_batch_estimate_timestamps"],
    ("two_pending", None): _SINGLE + ["icp_batch_register_launch", "icp_batch_stage"],
    ("begun", None): _SINGLE + BATCH_SYMBOLS,
    ("batch_hold", None): _SINGLE + [s for s in BATCH_SYMBOLS if s not in ("icp_batch_register_launch", "icp_batch_register_end")],
    ("frame", "key"): _SINGLE + BATCH_SYMBOLS,
    # a frame launched by icp_batch_frame_launch: the single calls on a member refuse as between the member's own frame calls
    ("frame", "batch"): ["icp_register_end", "icp_map_stage_cloud", "icp_map_update_staged", "icp_pmap_init", "icp_pmap_update",
                         "icp_map_normals_peek", "icp_estimate_timestamps", "icp_project", "icp_grid_sample"],
    ("frame", "nonkey"): ["icp_register_end", "icp_map_stage_cloud", "icp_map_update_staged", "icp_map_update", "icp_set_alignment",
                          "icp_project", "icp_frame_end"],
    ("pframe", "key"): ["icp_register_end", "icp_pmap_init", "icp_pmap_update", "icp_map_stage_cloud", "icp_map_update_staged",
                        "icp_set_option", "icp_set_stream", "icp_pmap_register", "icp_pmap_register_launch", "icp_pmap_frame_launch",
                        "icp_odometry_init", "icp_estimate_timestamps", "icp_register", "icp_project", "icp_grid_sample",
                        "icp_pmap_nearest_neighbor_search", "icp_pmap_get_model", "icp_compute_normal_map", "icp_pmap_frame_end"],
    ("pframe", "nonkey"): ["icp_register_end", "icp_pmap_init", "icp_pmap_update", "icp_project", "icp_pmap_frame_end"],
    ("pmap_launched", None): ["icp_pmap_update", "icp_pmap_init", "icp_set_option", "icp_set_stream", "icp_map_set", "icp_pmap_register",
                              "icp_pmap_register_launch", "icp_register", "icp_knn_query", "icp_estimate_timestamps",
                              "icp_align_point_to_plane", "icp_map_normals_peek", "icp_odometry_init", "icp_project", "icp_grid_sample",
                              "icp_pmap_nearest_neighbor_search", "icp_pmap_get_model", "icp_compute_normal_map", "icp_register_end"],
}
# (symbol, state): why the cell is not run
SKIPPED = {
    ("icp_odometry_init", "frame"): "COLLECTS by dropping the frame: the twin's frame has no result to compare",
    ("icp_pmap_nearest_neighbor_search", "frame"): "its recipe first gives the context a projective map: icp_pmap_update is REFUSED there",
    ("icp_profile_enable", "frame"): "the next icp_frame_launch refuses a context with profiling on: no follow-up frame to compare",
    ("icp_profile_enable", "batch_hold"): "a batched launch refuses a member with profiling on: the twin that enables it first has no state",
    ("icp_batch_register_end", "held"): "COLLECTS member 0 only through a batch whose idle members have nothing to collect",
    ("icp_batch_register_end", "begun"): "as under held",
    ("icp_batch_register_launch", "frame"): "a second registration beside the frame: ORDERED as icp_register_launch, no batched collection of it here",
    ("icp_batch_odometry_init", "frame"): "COLLECTS by dropping the frame, as icp_odometry_init",
    ("icp_batch_pmap_odometry_init", "batch_hold"): "as icp_batch_odometry_init there",
}
CELLS = [(state, variant, symbol) for (state, variant), symbols in PER_STATE.items() for symbol in symbols
         if A.TABLE[symbol].cells[state].kind != "N/A" and (symbol, state) not in SKIPPED]


def test_the_cells_cover_every_recipe_and_every_recipe_is_a_table_row():
    assert set(RECIPES) <= set(A.TABLE)
    assert {c[2] for c in CELLS if c[0] == "held"} == set(RECIPES) - {s for s, st in SKIPPED if st == "held"}
    # every row of the table that is not a constructor, a destructor, a default or an accessor has a recipe
    assert {s for s, r in A.TABLE.items() if any(c.kind != "N/A" for c in r.cells.values())} == set(RECIPES)
    kinds = {}
    for state, _, symbol in CELLS:
        k = A.TABLE[symbol].cells[state].kind
        kinds[k] = kinds.get(k, 0) + 1
    print("cells run on the GPU:", len(CELLS), kinds, "entry points:", len(RECIPES))
    # (the COLLECTS cells are the finishing call of the state itself, chunked against unchunked: counted apart)
    assert kinds["ORDERED"] >= 90 and kinds["REFUSED"] >= 250 and kinds["INDEPENDENT"] >= 150 and kinds["COLLECTS"] <= 12


@pytest.mark.parametrize("state,variant,symbol", CELLS, ids=[f"{s}{'-' + v if v else ''}-{x}" for s, v, x in CELLS])
def test_cell(env, state, variant, symbol):
    row = A.TABLE[symbol]
    cell = row.cells[state]
    # (icp_map_update_staged finds a staged cloud of the caller's wherever a caller can have staged one: its class is then read
    # off the in-flight checks, not off "no staged cloud")
    pre_stage = symbol in ("icp_map_update_staged", "icp_batch_map_update_staged") and state not in ("frame",) + PROJECTIVE_STATES
    with_sequence = symbol == "icp_batch_frame_launch" and state != "frame"  # (members with a sequence: the refusal is the state's)
    factory = lambda chunked, st, var: GpuRig(env, chunked, st, var, pre_stage, with_sequence)
    # (the twins that never make the call are shared by the REFUSED cells of a state)
    cache = env.cache if not (pre_stage or with_sequence) else {}
    # (the control belongs to the kd-tree registration: a kd-tree map call changes no projective one)
    control = row.control if state not in PROJECTIVE_STATES else "no kd-tree registration in flight"
    fails = A.run_cell(factory, state, symbol, cell, control, variant, cache)
    env.cells += 1
    env.controls += control is True and cell.kind == "ORDERED"
    assert fails == [], f"{symbol} beside `{state}` is {cell.kind}({cell.text}) in the table; failed checks: {fails}"


def test_the_frame_state_holds_iterations_back(env):
    """What the `frame` cells stand on: the jump frame's registration runs more iterations than its first chunk (the last
    frame's count + 1), so iterations are held back between icp_frame_launch and icp_frame_end.  Printed and asserted once."""
    trace, _ = A.run_scenario(lambda c, s, v: GpuRig(env, c, s, v), "frame", "icp_frame_end", 0, "never", "key")
    assert trace.error is None, trace.error
    last, jump = trace.results[len(A.FRAME_PROLOGUE) - 1].iterations, trace.results[len(A.FRAME_PROLOGUE)].iterations
    print("frame state: the last prologue frame ran", last, "iterations, the jump frame", jump)
    assert jump > last + 1


def _overlapped_run(env, overlap):
    """The fixed sequence of the overlapped state: a staged insertion into a full 3-cloud window on the map stream, and beside it
    every entry point that does NOT join that stream (DeviceGuard(ctx, false)) — projection, the grid-sample family, the
    de-skew, icp_compact_targets, icp_register_end behind a pose-only update, and the frame calls, whose end enqueues the update
    the next frame's preprocessing runs beside."""
    from pylidar_slam_amd.engine import IcpContext
    e, g = env, env.geo[(A.HEIGHT, A.WIDTH)]
    kw = dict(height=A.HEIGHT, width=A.WIDTH, max_num_alignments=A.MAX_ITERATIONS, threshold_delta_pose=A.THRESHOLD, scheme=A.SCHEME,
              sigma=A.SIGMA, local_map_size=A.LOCAL_MAP_SIZE)
    out = []
    ctx = IcpContext(**kw)
    ctx.set_option("overlap_map_update", overlap)
    ctx.map_init()
    for k in (0, 1, 2):  # the window is full: the staged insertion below evicts
        ctx.map_update(e.shift, e.scans[k])
    out.append(_reg(ctx.register(e.scans[3])))
    ctx.map_stage_cloud(e.cloud, skip_null=True)
    out.append(ctx.map_update_staged(e.shift))  # on the map stream with overlap 1
    out.append(_bits(ctx.project(e.dev_rows, with_index=True)))
    out.append(_bits(ctx.project_rows(e.dev_rows)))
    out.append(_bits(ctx.grid_sample(e.dev_rows, 0.3)))
    out.append(_bits(ctx.grid_sample_padded(e.dev_rows, 0.3)))
    out.append(_bits(ctx.grid_sample_padded(e.dev_rows.double(), 0.3)))
    out.append(_bits(ctx.voxel_hash(e.host_rows, 0.3)))
    out.append(_bits(ctx.distort(e.dev_rows, env.torch.from_numpy(e.stamps).cuda(), e.motion)))
    out.append(_bits(ctx.compact_targets(e.cloud, 8192, skip_null=True)))
    out.append(_bits(ctx.estimate_timestamps(e.dev_rows)))
    ctx.register_launch(e.scans[4], None)  # (joins the map stream)
    ctx.map_update(None)                   # pose-only, by the device-resident pose: on the map stream again
    out.append(_reg(ctx.register_end()))   # does not join: the pose arrives while the update runs
    out.append(_bits(ctx.project(e.dev_rows)))
    out.append(_reg(ctx.register(e.scans[5])))
    out += [_bits(ctx.map_points()), ctx.map_num_clouds(), _bits(ctx.map_normals_peek())]
    ctx.close()
    # the frame calls: every end leaves its update on the map stream, the next launch preprocesses (grid sample, projection) beside it
    ctx = IcpContext(**kw)
    ctx.set_option("overlap_map_update", overlap)
    ctx.odometry_init(voxel_size=0.3, targets=1)
    for k in range(5):
        ctx.frame_launch(e.scans[k])
        out.append(_frame(ctx.frame_end()))
    out += [_bits(ctx.map_points()), ctx.map_num_clouds(), _bits(ctx.map_normals_peek())]
    ctx.close()
    return out


def test_overlapped_calls_equal_the_joined_twin_on_one_run(env):
    """The `overlapped` state: "overlap_map_update" 1 against 0, every output of the fixed sequence bit for bit.  Run ONCE: a pass
    shows no race on this run and proves no absence of one."""
    under, twin = _overlapped_run(env, 1), _overlapped_run(env, 0)
    assert len(under) == len(twin)
    for k, (a, b) in enumerate(zip(under, twin)):
        assert a == b, f"output {k} of the overlapped sequence differs from the joined twin"
