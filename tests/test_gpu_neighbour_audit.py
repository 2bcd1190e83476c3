"""GPU side of the audit of contexts beside each other: the library run through the runner of tests/neighbour_audit.py — a context A
in an in-flight state, a neighbour B (a context or a batch of three) running a job beside it on the same device, each with its own
map, scans and stream, one host thread driving both, finished in both orders — then the benchmark's two arrangements, small
(batches on streams of their own; host threads), and the life cycle of the shared count.

Every comparison is bit equality against a SOLO TWIN (the same calls on a fresh context with nobody beside it) or an exact
integer (`lead_registrations()`, `registering_contexts()`, `handoff_fallbacks()`): there is no tolerance here.

Shapes, the smallest at which every path is still taken: 16 x 256 scans (4096 rows: 32 workgroups of the 128-query shape; one job
with 1 row, one with 4097), fixed maps of 8192 points, 8 forced iterations, the live-threshold registrations configured as
test_two_contexts_with_chunked_launches_on_one_device (15 iterations, 1e-6, geman_mcclure / 0.3), projective contexts at 17 x 33.
At these sizes every launch of both contexts is co-resident on the device: nothing here contends for CUs, and no hand-off may
time out (`handoff_fallbacks() == 0` is asserted, "lead_timeout_ms" is never set).
"""
import os
import sys
import threading
import time
from types import SimpleNamespace

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import neighbour_audit as N  # noqa: E402
import test_gpu_batch as TB  # noqa: E402  (its sequences, its single-context run and its comparison)
import test_gpu_inflight_audit as I  # noqa: E402  (its _bits / _reg / _frame: every returned bit, hashable)

pytestmark = pytest.mark.gpu

H, W, MAP_POINTS = 16, 256, 8192
SCHEME, SIGMA, LOCAL_MAP_SIZE = "geman_mcclure", 0.3, 3
LIVE_THRESHOLD = 1.0e-6
SCAN_FRAMES = {"short": 3, "jump": 10, "jump_b": 9, "second": 11, "next": 4}
EYE = np.eye(4, dtype=np.float32)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (no CPU fallback exists for the product path)")
    return torch


@pytest.fixture(scope="module")
def env(torch_cuda):
    torch = torch_cuda
    from pylidar_slam_amd.engine import IcpContext
    from pylidar_slam_amd.synthetic import SceneConfig, make_fixed_map, make_sequence, pose_matrix
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    cfg = SceneConfig(height=H, width=W)
    scans, poses = make_sequence(cfg, 12)
    e = SimpleNamespace(torch=torch, cache={}, tally=[0, 0], cells=0, started=time.perf_counter())
    e.frames = [dev(s) for s in scans]
    e.map = dev(make_fixed_map(cfg, scans[:4], poses[:4], ref_frame=3, num_points=MAP_POINTS))
    e.scan = {name: e.frames[k] for name, k in SCAN_FRAMES.items()}
    jump = scans[SCAN_FRAMES["jump"]]
    hit = int(np.flatnonzero(np.linalg.norm(jump, axis=1) > 1.0)[W * 8])  # a return in the middle of the image
    e.scan["one_row"] = dev(jump[hit:hit + 1])
    e.scan["odd_rows"] = dev(np.concatenate([jump, scans[SCAN_FRAMES["jump_b"]][hit:hit + 1]]))
    assert e.scan["one_row"].shape[0] == 1 and e.scan["odd_rows"].shape[0] == H * W + 1
    rng = np.random.default_rng(31)
    cloud = scans[5].copy()
    cloud[rng.integers(0, len(cloud), 50)] = np.nan
    cloud[rng.integers(0, len(cloud), 50)] = 0.0
    e.cloud = dev(cloud)
    e.shift = EYE.copy()
    e.shift[:3, 3] = (0.3, -0.2, 0.05)
    e.rows = dev(scans[8][1000:3000])
    # the projective drive of the 17 x 33 states, as the inflight audit builds it
    scratch = IcpContext(height=17, width=33)
    drive, _ = make_sequence(SceneConfig(height=17, width=33), 6)
    e.vmaps = [scratch.project(dev(sc)).clone() for sc in drive]
    e.prows = [v.permute(1, 2, 0).reshape(-1, 3).contiguous() for v in e.vmaps]
    e.step = pose_matrix(np.array([0.4, 0.0, 0.0, 0.0, 0.0, 0.01])).astype(np.float32)
    torch.cuda.synchronize()  # (every party enqueues on a stream of its own from here on)
    scratch.close()
    yield e
    torch.cuda.synchronize()
    print(f"\nneighbour audit: {e.cells} cells, {e.tally[0]} registrations latched lead and {e.tally[1]} plain in them, "
          f"{time.perf_counter() - e.started:.1f} s")


# ---- the drivers of neighbour_audit's protocol over the library ------------------------------------------------------------------------
class GpuContext:
    def __init__(self, world, live, projective=False, overlap=False):
        from pylidar_slam_amd.engine import IcpContext
        self.w, self.e = world, world.env
        self.stream = self.e.torch.cuda.Stream()
        h, w = (17, 33) if projective else (H, W)
        self.ctx = IcpContext(height=h, width=w, max_num_alignments=N.LIVE_MAX if live else N.FORCED,
                              threshold_delta_pose=LIVE_THRESHOLD if live else 0.0, scheme=SCHEME, sigma=SIGMA,
                              local_map_size=LOCAL_MAP_SIZE)
        self.ctx.set_option("chunked_launch", 1)
        if overlap:
            self.ctx.set_option("overlap_map_update", 1)
        self.frame_index = 0

    def _do(self, fn, *a, conv=None, **kw):
        from pylidar_slam_amd.engine import InvalidJacobianError
        try:
            with self.e.torch.cuda.stream(self.stream):
                try:
                    out = fn(*a, **kw)
                    out = conv(out) if conv else out
                except InvalidJacobianError as err:  # (the result up to the failing iteration: compared like any other)
                    r = I._reg(err.result)
                    out = N.Result(r.bits + ("Invalid Jacobian",), r.iterations)
        except AssertionError as err:
            raise N.RigError(f"{getattr(fn, '__name__', fn)}: {err}")
        except RuntimeError as err:
            I._stop_on_a_device_error(getattr(fn, "__name__", str(fn)), err)
            raise N.RigError(f"{getattr(fn, '__name__', fn)}: {err}")
        self.w.tick()
        return out

    def map_set(self):
        self._do(self.ctx.map_set, self.e.map)

    def register(self, scan):
        return self._do(self.ctx.register, self.e.scan[scan], conv=I._reg)

    def launch(self, scan, last=False):
        self._do(self.ctx.register_launch, self.e.scan[scan], "last" if last else None)

    def end(self):
        return self._do(self.ctx.register_end, conv=I._reg)

    def begin(self, scan):
        self._do(self.ctx.register_begin, self.e.scan[scan])

    def pair(self):
        self._do(self.ctx.iteration_accumulate)
        self._do(self.ctx.iteration_solve)

    # -- the frame calls (thresholds of the key-frame test as the inflight audit sets them)
    def odometry_init(self, key):
        self._do(self.ctx.odometry_init, threshold_trans=0.1 if key else 100.0, threshold_rot=0.3 if key else 180.0)
        self.frame_index = 0

    def frame_launch(self, k):
        self._do(self.ctx.frame_launch, self.e.frames[k])

    def frame_end(self):
        out = self._do(self.ctx.frame_end, conv=I._frame)
        self.frame_index += 1
        return out

    def pmap_odometry_init(self, key):
        self._do(self.ctx.pmap_odometry_init, threshold_trans=0.1 if key else 100.0, threshold_rot=0.3 if key else 180.0)
        self.frame_index = 0

    def pframe_launch(self, k):
        self._do(self.ctx.pmap_frame_launch, self.e.vmaps[k])

    def pframe_end(self):
        out = self._do(self.ctx.pmap_frame_end, conv=I._frame)
        self.frame_index += 1
        return out

    def pmap_setup(self):
        self._do(self.ctx.pmap_init)
        self._do(self.ctx.pmap_update, EYE, self.e.vmaps[0])
        self._do(self.ctx.pmap_update, self.e.step, self.e.vmaps[1])

    def pmap_register(self, k):
        return self._do(self.ctx.pmap_register, self.e.prows[k], None, True, conv=I._reg)

    def pmap_launch(self, k):
        self._do(self.ctx.pmap_register_launch, self.e.prows[k], None, True)

    # -- calls that register nothing
    def nns(self):
        return self._do(self.ctx.nearest_neighbor_search, self.e.rows, conv=I._bits)

    def knn(self):
        return self._do(self.ctx.knn_query, self.e.rows, k=3, conv=I._bits)

    def map_update_cloud(self):
        return self._do(self.ctx.map_update, self.e.shift, self.e.cloud, skip_null=True, conv=I._bits)

    def leads(self):
        return self.ctx.lead_registrations()

    def fallbacks(self):
        return self.ctx.handoff_fallbacks()

    def snapshot(self):
        c, out = self.ctx, []
        with self.e.torch.cuda.stream(self.stream):
            if c.map_size() > 0:
                out += [I._bits(c.map_points()), c.map_num_clouds(), I._bits(c.map_normals_peek())]
            if c.pmap_num_maps() > 0:
                out += [c.pmap_num_maps(), I._bits(c.pmap_model())]
        return tuple(out)

    def close(self):
        self.ctx.close()


class GpuBatch:
    def __init__(self, world, members):
        from pylidar_slam_amd.engine import IcpBatch
        self.w, self.e, self.members = world, world.env, members
        self.stream = members[0].stream
        for m in members:  # (a batch enqueues on ONE stream)
            m.stream = self.stream
        self.b = IcpBatch([m.ctx for m in members])
        self._do = lambda fn, *a, **kw: GpuContext._do(self, fn, *a, **kw)

    def launch(self, scans, last=False):
        self._do(self.b.register_launch, [self.e.scan[s] for s in scans], "last" if last else None)

    def map_update(self):
        self._do(self.b.map_update)

    def end(self):
        return self._do(self.b.register_end, conv=lambda rs: [I._reg(r) for r in rs])

    def close(self):
        self.b.close()


class GpuWorld:
    def __init__(self, env):
        self.env, self.tick = env, lambda: None

    def context(self, live, projective=False, overlap=False):
        return GpuContext(self, live, projective, overlap)

    def batch(self, contexts):
        return GpuBatch(self, contexts)

    def count(self):
        from pylidar_slam_amd.engine import registering_contexts
        return registering_contexts(0)

    def close(self):
        pass

    # -- every way a registration can end (neighbour_audit.ENDINGS)
    def ending(self, name, expect):
        torch = self.env.torch

        def ready(n=1):
            cs = [self.context(False) for _ in range(n)]
            for c in cs:
                c.map_set()
            return cs

        def refused(fn, *a, **kw):
            try:
                fn(*a, **kw)
            except N.RigError:
                return
            raise N.RigError("the call was to be refused")
        if name == "collected":
            c, = ready()
            c.launch("short")
            expect(1)
            c.end()
            expect(0)
            c.close()
        elif name == "invalid_jacobian":  # an exact plane: every row has the same normal (test_gpu_batch_direct._plane)
            xs, ys = np.meshgrid(np.arange(40, dtype=np.float32) * 0.1, np.arange(40, dtype=np.float32) * 0.1)
            plane = np.stack([xs.ravel(), ys.ravel(), np.zeros(xs.size, np.float32)], axis=1)
            above = np.ascontiguousarray(plane[::3] + np.array([0.013, 0.007, 0.05], np.float32))
            c = self.context(False)
            c._do(c.ctx.map_set, torch.from_numpy(plane).cuda())
            c._do(c.ctx.register_launch, torch.from_numpy(above).cuda(), None)
            expect(1)
            res = c.end()
            if res.bits[-1] != "Invalid Jacobian":
                raise N.RigError("the plane over a plane was to raise Invalid Jacobian")
            expect(0)
            c.close()
        elif name == "launch_refused_empty_map":
            c = self.context(False)
            try:
                c.launch("short")
                raise N.RigError("an empty map was to refuse the launch")
            except N.RigError as err:
                if "empty" not in str(err):
                    raise
            expect(0)
            c.close()
        elif name in ("batch_fails_at_last_member", "batch_option_mismatch"):
            cs = ready(3)
            # a member off the fused path is found out BEHIND its register_begin (two members are counted by then); an option the
            # members must share is found out in front of every begin
            cs[2].ctx.set_option(*(("fuse_iteration", 0) if name == "batch_fails_at_last_member" else ("wide_until", 7)))
            b = self.batch(cs)
            refused(b.launch, ["short", "jump", "second"])
            expect(0)
            b.close()
            for c in cs:
                c.close()
        elif name == "batch_closed_pending":
            cs = ready(3)
            b = self.batch(cs)
            b.launch(["short", "jump", "second"])
            expect(3)
            b.close()
            expect(3)  # (the members' results stand: each member collects its own)
            for k, c in enumerate(cs):
                c.end()
                expect(2 - k)
            for c in cs:
                c.close()
        elif name in ("closed_one_pending", "closed_two_pending"):
            c, = ready()
            c.launch("short")
            if name == "closed_two_pending":
                c.launch("jump", last=True)
            expect(1)
            c.close()
        elif name == "frame_dropped":
            c = self.context(False)
            c.odometry_init(True)
            c.frame_launch(0)
            c.frame_end()
            c.frame_launch(1)
            expect(1)
            c.odometry_init(True)  # (icp_odometry_init drops the launched frame: frame_drop_pending collects its registration)
            expect(0)
            c.close()
        elif name == "begun_destroyed":
            c, = ready()
            c.begin("short")
            expect(1)
            c.close()
        else:
            raise N.RigError(name)


def _world(env):
    return lambda: GpuWorld(env)


# ---- the matrix ------------------------------------------------------------------------------------------------------------------------
def test_the_matrix_is_the_table():
    assert len(N.CELLS) == len(N.STATES) * (sum(2 if j.spans else 1 for j in N.JOBS.values()))
    assert [s for s, spec in N.STATES.items() if spec.counted == 0] == ["pframe", "pmap_launched"]
    print("cells:", len(N.CELLS), "skipped:", len(N.SKIPPED))


@pytest.mark.parametrize("state,job,order", N.CELLS, ids=["-".join(c) for c in N.CELLS])
def test_cell(env, state, job, order):
    fails = N.run_cell(_world(env), state, job, order, env.cache, env.tally)
    env.cells += 1
    assert fails == [], f"A in `{state}` beside B running `{job}` ({order}): failed check {fails}"


def test_a_context_alternates_lead_and_plain_on_one_mailbox(env):
    """Six registrations of one context, each from "last", latched lead, plain, plain, lead, plain, lead as a neighbour comes and
    goes (two results of the context pending beside it in between): the pattern read back through lead_registrations(), every
    result and the map bit-equal to the same six run alone."""
    assert N.run_alternation(_world(env)) == []


@pytest.mark.parametrize("ending", N.ENDINGS)
def test_the_count_is_left_however_a_registration_ends(env, ending):
    """registering_contexts() is 0 behind every ending, and a fresh context's next registration is lead."""
    assert N.run_ending(_world(env), ending) == []


# ---- the benchmark's own loop, small ---------------------------------------------------------------------------------------------------
BENCH_KW = dict(height=H, width=W, max_num_alignments=N.FORCED, threshold_delta_pose=0.0, scheme=SCHEME, sigma=SIGMA)
STEPS = 5


@pytest.fixture(scope="module")
def drives(torch_cuda):
    """Eight independent sequences and what each gives on a context of its own (computed once)."""
    seqs = TB._sequences(8, H, W, MAP_POINTS, 6, seed0=4321)
    options = dict(TB.BENCH_OPTIONS)
    return seqs, {frames: [TB._run_single(BENCH_KW, options, s, frames, "pose", torch_cuda) for s in seqs] for frames in (STEPS, 6)}


@pytest.mark.parametrize("groups,members", [(2, 3), (4, 2)], ids=["2x3", "4x2"])
def test_batches_on_streams_of_their_own(torch_cuda, drives, groups, members):
    """bench.py::batched_leg's loop: G batches, each on a stream of its own, one thread; per step project / register_launch /
    map_update for EVERY batch, then register_end for every batch, the launch order rotated each step.  Per member every step's
    result and the final map equal the single-context run; the batch launched first in a step is lead, those behind it plain;
    the count is the number of members in flight and 0 behind each step."""
    from pylidar_slam_amd.engine import IcpBatch, IcpContext, registering_contexts
    torch = torch_cuda
    seqs, solo = drives
    parts = [list(range(g * members, (g + 1) * members)) for g in range(groups)]
    ctxs = {}
    for s in range(groups * members):
        c = IcpContext(**BENCH_KW)
        for k, v in TB.BENCH_OPTIONS.items():
            c.set_option(k, v)
        c.map_set(torch.from_numpy(seqs[s][1]).cuda())
        ctxs[s] = c
    scans = {s: [torch.from_numpy(x).cuda() for x in seqs[s][0][:STEPS]] for s in ctxs}
    vmaps = {s: torch.empty((3, H, W), dtype=torch.float32, device="cuda") for s in ctxs}
    torch.cuda.synchronize()
    batches = [IcpBatch([ctxs[s] for s in part]) for part in parts]
    streams = [torch.cuda.Stream() for _ in parts]
    out, last = {s: [] for s in ctxs}, {s: None for s in ctxs}
    assert registering_contexts(0) == 0
    for step in range(STEPS):
        order = [(g + step) % groups for g in range(groups)]
        for rank, g in enumerate(order):
            before = [ctxs[s].lead_registrations() for s in parts[g]]
            with torch.cuda.stream(streams[g]):
                batches[g].project([scans[s][step] for s in parts[g]], [vmaps[s] for s in parts[g]])
                batches[g].register_launch([scans[s][step] for s in parts[g]], [last[s] for s in parts[g]])
                batches[g].map_update()
            got = [ctxs[s].lead_registrations() - b for s, b in zip(parts[g], before)]
            assert got == [1 if rank == 0 else 0] * members, (step, g, rank, got)
            assert registering_contexts(0) == (rank + 1) * members
        for rank, g in enumerate(order):
            for s, r in zip(parts[g], batches[g].register_end()):
                out[s].append(r)
                last[s] = r.pose
            assert registering_contexts(0) == (groups - rank - 1) * members
    maps = {s: c.map_points() for s, c in ctxs.items()}
    fallbacks = {s: c.handoff_fallbacks() for s, c in ctxs.items()}
    for b in batches:
        b.close()
    for c in ctxs.values():
        c.close()
    assert registering_contexts(0) == 0
    for s in ctxs:
        TB._assert_same(solo[STEPS][s], (out[s], maps[s], fallbacks[s]), ("batches on streams", groups, members, s))


def test_four_host_threads_on_one_run(torch_cuda, drives):
    """The 4-thread arrangement: four host threads, each with a context and a stream of its own, six frames each.  Every sequence
    equals its solo run bit for bit.  Which registrations are lead depends on how the threads interleave, so only two things are
    asserted of the decision: lead + plain = the registrations run (0 <= lead <= 6 per context), and the count is 0 after the
    joins.  ONE run: a pass shows no race on that run and proves no absence of one."""
    from pylidar_slam_amd.engine import IcpContext, registering_contexts
    torch = torch_cuda
    seqs, solo = drives
    frames, threads_n = 6, 4
    got, errors = {}, []

    def work(s):
        try:
            with torch.cuda.stream(torch.cuda.Stream()):
                c = IcpContext(**BENCH_KW)
                for k, v in TB.BENCH_OPTIONS.items():
                    c.set_option(k, v)
                c.map_set(torch.from_numpy(seqs[s][1]).cuda())
                rs, init = [], None
                for f in range(frames):
                    c.register_launch(torch.from_numpy(seqs[s][0][f]).cuda(), init)
                    c.map_update(None, None)
                    rs.append(c.register_end())
                    init = rs[-1].pose
                got[s] = (rs, c.map_points(), c.handoff_fallbacks(), c.lead_registrations())
                c.close()
        except Exception as err:  # noqa: BLE001  (reported by the asserting thread)
            errors.append((s, repr(err)))
    assert registering_contexts(0) == 0
    threads = [threading.Thread(target=work, args=(s,), daemon=True) for s in range(threads_n)]
    deadline = time.monotonic() + 60.0
    for t in threads:
        t.start()
    for t in threads:
        t.join(max(0.0, deadline - time.monotonic()))
    assert not any(t.is_alive() for t in threads), "a host thread did not finish within 60 s"
    assert not errors, errors
    assert registering_contexts(0) == 0
    leads = [got[s][3] for s in range(threads_n)]
    print("lead registrations per thread (of 6):", leads)
    for s in range(threads_n):
        assert 0 <= got[s][3] <= frames
        TB._assert_same(solo[frames][s], got[s][:3], ("host threads", s))
