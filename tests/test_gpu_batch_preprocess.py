"""`-m gpu`: the batched preprocessing stage — `icp_batch_preprocess` / `IcpBatch.preprocess`, `MI355XPreprocessingBatch`,
`icp_batch_project_rows` / `IcpBatch.project_rows` and `icp_batch_stage` / `IcpBatch.stage`.

The reference's `Preprocessing` chain (slam/preprocessing.py:269-290: Distortion :144-191 -> GridSample :207-226 ->
ToTensor :101-126) for B frames at once, and the projection / staging in front of a batched registration.  Per member
everything must be what the single filters / the single context compute on the same frame, bit for bit."""
import copy
import ctypes as C
import os

import numpy as np
import pytest

from test_gpu_batch_loop import _assert_same_run, _record, _scans
from test_loop_reference import golden_loop, loop_scans, published_config  # noqa: F401 (fixtures)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
H, W = 64, 2048


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (no CPU fallback exists for the product path)")
    return torch


def _yaml_chain(**grid):
    """config/slam/preprocessing/grid_sample_mi355x.yaml, grid_sample_mi355x's options overridden by `grid`."""
    import yaml
    with open(os.path.join(ROOT, "config", "slam", "preprocessing", "grid_sample_mi355x.yaml")) as f:
        cfg = yaml.safe_load(f)["filters"]
    cfg = copy.deepcopy(cfg)
    cfg["2"].update(grid)
    return cfg


def _single_filters(cfg, dev):
    """The four single filters of the same chain (what Preprocessing builds from the yaml, one per frame)."""
    from pylidar_slam_amd import odometry as our
    c = [dict(cfg[k]) for k in sorted(cfg, key=int)]
    return [our.ToDevice(our.ToDeviceConfig(**c[0]), device=dev), our.Distortion(our.DistortionConfig(**c[1])),
            our.GridSample(our.GridSampleConfig(**c[2])), our.ToTensor(our.ToTensorConfig(**c[3]), device=dev)]


def _timestamps(seed, n):
    """Seeded, sorted synthetic timestamps of one sweep (float64 seconds)."""
    return np.sort(np.random.default_rng(seed).uniform(0.0, 0.1, n)).astype(np.float64)


def _motion(seed):
    """A small relative motion (a few degrees about a tilted axis, a few centimetres)."""
    from pylidar_slam_amd.odometry import build_pose_matrix
    rng = np.random.default_rng(seed)
    return build_pose_matrix(np.concatenate([rng.uniform(-0.3, 0.3, 3), rng.uniform(-0.05, 0.05, 3)]), np.float32)


def _same(a, b, label):
    """Same type, dtype and shape; bit-equal where finite, NaN in the same places."""
    import torch
    assert type(a) is type(b), (label, type(a), type(b))
    if not isinstance(a, torch.Tensor):
        assert np.array_equal(np.asarray(a), np.asarray(b)), label
        return
    assert a.dtype == b.dtype and tuple(a.shape) == tuple(b.shape) and a.device == b.device, \
        (label, a.dtype, b.dtype, tuple(a.shape), tuple(b.shape))
    x, y = a.cpu().numpy(), b.cpu().numpy()
    if x.dtype.kind == "f":
        nx, ny = np.isnan(x), np.isnan(y)
        assert np.array_equal(nx, ny), (label, "NaN rows")
        assert np.array_equal(x[~nx], y[~ny]), (label, "values")
    else:
        assert np.array_equal(x, y), label


def _assert_same_dicts(single, batched, label):
    assert single.keys() == batched.keys(), (label, sorted(single.keys()), sorted(batched.keys()))
    for key in single:
        _same(single[key], batched[key], f"{label}: {key}")
    # Distortion's pass-through hands over the uploaded frame itself, ToTensor a float32 tensor itself
    assert (single["distorted"] is single["pc_device"]) == (batched["distorted"] is batched["pc_device"]), label
    assert (single["input_data"] is single["sample_points"]) == (batched["input_data"] is batched["sample_points"]), label


def _run_chains(torch, cfg, frames):
    """`frames`: B input dicts.  Returns (single chain per member, one MI355XPreprocessingBatch call) outputs."""
    from pylidar_slam_amd.odometry import MI355XPreprocessingBatch
    dev = torch.device("cuda:0")
    singles = []
    for f in frames:
        d = dict(f)
        for flt in _single_filters(cfg, dev):
            flt.filter(d)
        singles.append(d)
    pre = MI355XPreprocessingBatch(cfg, len(frames), device=dev)
    batched = [dict(f) for f in frames]
    pre.forward(batched)
    torch.cuda.synchronize()
    return singles, batched, pre


# ---- 1. the reference's outputs --------------------------------------------------------------------------------------
def test_reference_pin(torch_cuda):
    """tests/golden/distortion.npz (the reference's Distortion + GridSample outputs) as four members of one batch, plus a
    fifth with constant timestamps: every de-skewed frame within 1e-11 of the reference's and bit-equal to `distort` on
    its own; every sample index list equal to the reference's."""
    torch = torch_cuda
    from pylidar_slam_amd.engine import IcpBatch, IcpContext
    g = np.load(os.path.join(GOLDEN, "distortion.npz"))
    names = ("small", "large", "identity", "pure_translation", "constant")
    ctxs = [IcpContext() for _ in names]
    batch = IcpBatch(ctxs)
    pc = torch.from_numpy(g["pc"]).cuda()
    ts = torch.from_numpy(g["timestamps"]).cuda()
    const = torch.full_like(ts, 3.0)
    poses = [g[f"{n}_rpose"] for n in names[:4]] + [g["small_rpose"]]
    out = batch.preprocess([pc] * 5, [ts] * 4 + [const], poses, 0.3)
    torch.cuda.synchronize()
    single = IcpContext()
    for k, name in enumerate(names):
        o = out[k]
        dist = o["distorted"].cpu().numpy()
        alone = single.distort(pc, ts if k < 4 else const, poses[k]).cpu().numpy()
        assert np.array_equal(dist, alone), name
        v = int(o["count"])
        idx = o["indices"].cpu().numpy()
        if k < 4:
            np.testing.assert_allclose(dist, g[f"{name}_distorted"], atol=1e-11)
            np.testing.assert_array_equal(idx[:v], g[f"{name}_sample_indices"])
        else:
            np.testing.assert_allclose(dist, g["constant_ts_distorted"], atol=1e-12)
            p, i, c = single.grid_sample_padded(o["distorted"], 0.3)
            assert int(c) == v and np.array_equal(i.cpu().numpy(), idx)
        assert (idx[v:] == -1).all()
        smp = o["samples"].cpu().numpy()
        assert smp.dtype == np.float64 and np.array_equal(smp[:v], dist[idx[:v]]) and np.isnan(smp[v:]).all()
        assert np.array_equal(o["samples_f32"].cpu().numpy()[:v], smp[:v].astype(np.float32))
    batch.close()
    for c in ctxs + [single]:
        c.close()


# ---- 2. batched equals single, filter by filter ------------------------------------------------------------------------
def _ragged_frames(torch):
    """Seven frames of ragged sizes: de-skewed; without timestamps; init_rpose None; empty (n = 0); > 262 144 points (the
    single path inside the call); a skewed frame whose voxel keys overflow one bucket slice (thousands of voxels in a
    small box plus one point far away); a plain de-skewed one at benchmark size."""
    scans = _scans(11234, 0.3, 3)
    rng = np.random.default_rng(7)
    big = rng.uniform(-60.0, 60.0, (300_000, 3)).astype(np.float32)
    g = np.stack(np.meshgrid(*[np.arange(24) * 0.3] * 3, indexing="ij"), -1).reshape(-1, 3)
    box = np.concatenate([g + rng.uniform(-0.05, 0.05, g.shape), [[4.0e3, -3.5e3, 900.0]]]).astype(np.float32)
    frames = [
        {"numpy_pc": scans[0][::2].copy(), "numpy_pc_timestamps": _timestamps(1, scans[0][::2].shape[0]), "init_rpose": _motion(1)},
        {"numpy_pc": scans[1][1::3].copy(), "init_rpose": _motion(2)},
        {"numpy_pc": scans[2][::5].copy(), "numpy_pc_timestamps": _timestamps(3, scans[2][::5].shape[0]), "init_rpose": None},
        {"numpy_pc": np.zeros((0, 3), np.float32), "numpy_pc_timestamps": np.zeros(0, np.float64), "init_rpose": _motion(4)},
        {"numpy_pc": big, "numpy_pc_timestamps": _timestamps(5, big.shape[0]), "init_rpose": _motion(5)},
        {"numpy_pc": box, "numpy_pc_timestamps": _timestamps(6, box.shape[0]), "init_rpose": _motion(6)},
        {"numpy_pc": scans[2].copy(), "numpy_pc_timestamps": _timestamps(8, scans[2].shape[0]), "init_rpose": _motion(8)},
    ]
    assert box.shape[0] > 4096 + 1 and big.shape[0] > 262_144
    return frames


@pytest.mark.parametrize("padded", [True, False])
def test_batched_equals_single_filter_by_filter(torch_cuda, padded):
    torch = torch_cuda
    frames = _ragged_frames(torch)
    cfg = _yaml_chain(padded=padded)
    singles, batched, pre = _run_chains(torch, cfg, frames)
    for k, (s, b) in enumerate(zip(singles, batched)):
        _assert_same_dicts(s, b, f"member {k}")
    # the cases are what they claim to be
    assert batched[0]["distorted"].dtype == torch.float64 and batched[1]["distorted"] is batched[1]["pc_device"]
    assert batched[2]["distorted"] is batched[2]["pc_device"] and batched[3]["sample_points"].shape[0] == 0
    pre.batch.close()


def test_deactivated_distortion_passes_through(torch_cuda):
    """`activate: false` (distortion_mi355x): every frame's `distorted` is its uploaded float32 frame, timestamps or not."""
    torch = torch_cuda
    cfg = _yaml_chain(padded=True)
    cfg["1"]["activate"] = False
    scans = _scans(12234, 0.3, 2)
    frames = [{"numpy_pc": s, "numpy_pc_timestamps": _timestamps(k, s.shape[0]), "init_rpose": _motion(k)}
              for k, s in enumerate(scans)]
    singles, batched, pre = _run_chains(torch, cfg, frames)
    for k, (s, b) in enumerate(zip(singles, batched)):
        _assert_same_dicts(s, b, f"member {k}")
        assert b["distorted"] is b["pc_device"]
    pre.batch.close()


def test_benchmark_size(torch_cuda):
    """B = 8 frames of 64 x 2048 with timestamps, one call: equal to the single chain member by member."""
    torch = torch_cuda
    cfg = _yaml_chain(padded=True, voxel_size=0.4)
    frames = []
    for k in range(8):
        s = _scans(1234 + 1000 * k, 0.3, 1)[0]
        frames.append({"numpy_pc": s, "numpy_pc_timestamps": _timestamps(100 + k, s.shape[0]), "init_rpose": _motion(k)})
    singles, batched, pre = _run_chains(torch, cfg, frames)
    for k, (s, b) in enumerate(zip(singles, batched)):
        _assert_same_dicts(s, b, f"member {k}")
        assert s["pc_device"].shape[0] > 100_000
    pre.batch.close()


# ---- 3. projection and staging -----------------------------------------------------------------------------------------
def test_project_rows_and_stage(torch_cuda):
    """`IcpBatch.project_rows` equals `IcpContext.project_rows` per member on padded inputs (NaN rows behind the samples);
    `IcpBatch.stage` then `map_update_staged` equals per-member staging: same maps and windows."""
    torch = torch_cuda
    from pylidar_slam_amd.engine import IcpBatch, IcpContext
    drives = [_scans(13234 + 1000 * b, 0.3 + 0.05 * b, 3, with_motion=True) for b in range(3)]
    util = IcpContext(height=H, width=W)
    clouds = [[util.grid_sample_padded(torch.from_numpy(s).cuda(), 0.4)[0] for s in scans] for scans, _ in drives]
    clouds[2][2] = clouds[2][2][:0]  # an empty cloud
    torch.cuda.synchronize()

    def contexts():
        return [IcpContext(height=H, width=W, max_num_alignments=20, threshold_delta_pose=1e-4, scheme="neighborhood",
                           sigma=0.2, local_map_size=30, num_neighbors_normals=10) for _ in range(3)]

    runs = []
    for batched in (False, True):
        ctxs = contexts()
        batch = IcpBatch(ctxs)
        batch.use_torch_stream()
        if batched:
            projected = batch.project_rows([cl[1] for cl in clouds])
        else:
            projected = [c.project_rows(cl[1]) for c, cl in zip(ctxs, clouds)]
        for b in range(3):
            ctxs[b].map_update(np.eye(4, dtype=np.float32), clouds[b][0])
        for step in (1, 2):
            if batched:
                batch.stage([cl[step] for cl in clouds], skip_null=False)
            else:
                for c, cl in zip(ctxs, clouds):
                    c.map_stage_cloud(cl[step], skip_null=False)
            inserted = batch.map_update_staged([1, 1, 1], [drives[b][1][step] for b in range(3)])
        torch.cuda.synchronize()
        runs.append(([(v.cpu().numpy(), r.cpu().numpy()) for v, r in projected], inserted,
                     [(c.map_points(), c.map_num_clouds()) for c in ctxs]))
        batch.close()
        for c in ctxs:
            c.close()
    (proj_a, ins_a, maps_a), (proj_b, ins_b, maps_b) = runs
    for (va, ra), (vb, rb) in zip(proj_a, proj_b):
        assert np.array_equal(va, vb) and np.array_equal(ra, rb)
    assert ins_a == ins_b and ins_a[2] == 0
    for (ma, na), (mb, nb) in zip(maps_a, maps_b):
        assert na == nb and np.array_equal(ma, mb)
    util.close()


# ---- 4. the loop ------------------------------------------------------------------------------------------------------
def _drive_frames(scans, seed):
    return [{"numpy_pc": s, "numpy_pc_timestamps": _timestamps(seed + f, s.shape[0])} for f, s in enumerate(scans)]


def _run_single_chain(torch, frames, cfg, chain, hw):
    """One drive through the padded single-filter chain and MI355XICPFrameToModel: what _run_single of
    test_gpu_batch_loop returns."""
    from pylidar_slam_amd import odometry as our
    dev = torch.device("cuda:0")
    odo = our.MI355XICPFrameToModel(cfg, projector=our.SphericalProjector(*hw), device=dev)
    filters = _single_filters(chain, dev)
    init = our.ConstantVelocityInitialization()
    odo.init()
    init.init()
    out = []
    for f, frame in enumerate(frames):
        d = dict(frame)
        init.next_frame(d)
        for flt in filters:
            flt.filter(d)
        odo.process_next_frame(d)
        if f > 0:
            init.save_real_motion(d["odometry_pose"], d)
            out.append(_record(odo.last_result))
    maps = odo.ctx.map_points() if not odo._projective else odo.ctx.pmap_model()[0]
    clouds = odo.ctx.map_num_clouds() if not odo._projective else odo.ctx.pmap_num_maps()
    result = (out, maps, clouds, odo.get_relative_poses())
    odo.ctx.close()
    return result


def _run_batched_chain(torch, drives, cfg, chain, hw):
    """The same drives through MI355XPreprocessingBatch + MI355XICPFrameToModelBatch."""
    from pylidar_slam_amd import odometry as our
    dev = torch.device("cuda:0")
    count = len(drives)
    odo = our.MI355XICPFrameToModelBatch(cfg, count, projector=our.SphericalProjector(*hw), device=dev)
    pre = our.MI355XPreprocessingBatch(chain, count, device=dev)
    inits = [our.ConstantVelocityInitialization() for _ in range(count)]
    odo.init()
    for i in inits:
        i.init()
    out = [[] for _ in range(count)]
    for f in range(len(drives[0])):
        dicts = [dict(drives[b][f]) for b in range(count)]
        for b in range(count):
            inits[b].next_frame(dicts[b])
        pre.forward(dicts)
        odo.process_next_frames(dicts)
        if f == 0:
            continue
        for b, d in enumerate(dicts):
            inits[b].save_real_motion(d["odometry_pose"], d)
            out[b].append(_record(odo.members[b].last_result))
    result = []
    for b, m in enumerate(odo.members):
        maps = m.ctx.map_points() if not m._projective else m.ctx.pmap_model()[0]
        clouds = m.ctx.map_num_clouds() if not m._projective else m.ctx.pmap_num_maps()
        result.append((out[b], maps, clouds, odo.get_relative_poses(b)))
    odo.batch.close()
    pre.batch.close()
    return result


def test_published_loop_with_batched_preprocessing(torch_cuda, loop_scans):
    """Four 36-frame drives of the published configuration with timestamps (the golden loop's scans and three other
    seeds) through MI355XPreprocessingBatch + MI355XICPFrameToModelBatch: every frame, the final map, the window and the
    trajectory equal to four single plugins on the padded single-filter chain."""
    torch = torch_cuda
    scans0, _ = loop_scans
    seqs = [scans0, _scans(2234, 0.3, 36), _scans(3234, 0.5, 36), _scans(4234, 0.25, 36)]
    drives = [_drive_frames(s, 1000 * k) for k, s in enumerate(seqs)]
    cfg = published_config()
    chain = _yaml_chain(padded=True, voxel_size=0.4)
    batched = _run_batched_chain(torch, drives, cfg, chain, (H, W))
    for b, frames in enumerate(drives):
        single = _run_single_chain(torch, frames, cfg, chain, (H, W))
        _assert_same_run(single, batched[b], f"member {b}")
        assert single[2] == 30


def test_projective_loop_with_batched_preprocessing(torch_cuda):
    """The projective map (64 x 1024) on the same batched stage: equal to the single plugins."""
    torch = torch_cuda
    from pylidar_slam_amd.synthetic import SceneConfig, make_sequence
    from pylidar_slam_amd.odometry import MI355XICPConfig
    cfg = MI355XICPConfig(max_num_alignments=20, threshold_delta_pose=1e-4, data_key="input_data",
                          local_map=dict(type="projective_local_map", local_map_size=10),
                          alignment=dict(mode="point_to_plane_gauss_newton",
                                         gauss_newton_config=dict(max_iters=1, scheme="neighborhood", sigma=0.2)))
    seqs = [make_sequence(SceneConfig(height=64, width=1024, seed=5234 + 1000 * k, step=0.3 + 0.05 * k), 12)[0]
            for k in range(3)]
    drives = [_drive_frames(s, 500 * k) for k, s in enumerate(seqs)]
    chain = _yaml_chain(padded=True, voxel_size=0.4)
    batched = _run_batched_chain(torch, drives, cfg, chain, (64, 1024))
    for b, frames in enumerate(drives):
        _assert_same_run(_run_single_chain(torch, frames, cfg, chain, (64, 1024)), batched[b], f"member {b}")


# ---- 6. refusals and layout --------------------------------------------------------------------------------------------
def test_refused_calls_change_nothing(torch_cuda):
    """Every refusal — list lengths != B, a CPU tensor where a device pointer is required, a timestamps length != n,
    `distorted_out` missing for a de-skewing member, a call while a member is inside a registration — leaves every output
    buffer and member untouched; the next accepted call gives what a fresh batch gives."""
    torch = torch_cuda
    from pylidar_slam_amd.engine import IcpBatch, IcpContext
    scans = _scans(14234, 0.3, 2)
    pcs = [torch.from_numpy(s).cuda() for s in scans]
    tss = [torch.from_numpy(_timestamps(k, s.shape[0])).cuda() for k, s in enumerate(scans)]
    poses = [_motion(0), _motion(1)]
    ctxs = [IcpContext(height=H, width=W) for _ in range(2)]
    batch = IcpBatch(ctxs)
    batch.use_torch_stream()

    def fresh_out():
        out = []
        for p in pcs:
            n = p.shape[0]
            f32 = torch.full((n, 3), 7.0, dtype=torch.float32, device=p.device)
            out.append({"distorted": torch.full((n, 3), 7.0, dtype=torch.float64, device=p.device),
                        "samples": torch.full((n, 3), 7.0, dtype=torch.float64, device=p.device), "samples_f32": f32,
                        "indices": torch.full((n,), 7, dtype=torch.int64, device=p.device),
                        "count": torch.full((), 7, dtype=torch.int32, device=p.device)})
        return out

    out = fresh_out()

    def untouched():
        torch.cuda.synchronize()
        for o in out:
            for v in o.values():
                assert bool((v == 7).all()), "an output buffer was written by a refused call"

    with pytest.raises(AssertionError, match="expected 2"):
        batch.preprocess(pcs[:1], tss[:1], poses[:1], 0.4, out=out)
    untouched()
    with pytest.raises(AssertionError, match="cuda"):
        batch.preprocess([pcs[0], scans[1]], tss, poses, 0.4, out=out)
    untouched()
    with pytest.raises(AssertionError, match="cuda"):
        batch.preprocess(pcs, [tss[0], tss[1].cpu()], poses, 0.4, out=out)
    untouched()
    with pytest.raises(AssertionError, match="timestamps for"):
        batch.preprocess(pcs, [tss[0], tss[1][:-1]], poses, 0.4, out=out)
    untouched()
    missing = [dict(o) for o in out]
    missing[1]["distorted"] = None
    with pytest.raises(AssertionError, match="distorted_out"):
        batch.preprocess(pcs, tss, poses, 0.4, out=missing)
    untouched()
    with pytest.raises(AssertionError, match="cuda"):
        batch.stage([pcs[0], scans[1]])
    with pytest.raises(AssertionError, match="expected 2"):
        batch.project_rows(pcs[:1])
    # a member inside a registration (icp_register_begin .. icp_register_end)
    ctxs[0].map_update(np.eye(4, dtype=np.float32), pcs[0])
    ctxs[0].register_begin(pcs[1], poses[1])
    for call in (lambda: batch.preprocess(pcs, tss, poses, 0.4, out=out), lambda: batch.stage(pcs),
                 lambda: batch.project_rows(pcs)):
        with pytest.raises(AssertionError, match="registration in progress"):
            call()
    untouched()
    ctxs[0].register_end()
    got = batch.preprocess(pcs, tss, poses, 0.4, out=out)
    ref_ctxs = [IcpContext(height=H, width=W) for _ in range(2)]
    ref = IcpBatch(ref_ctxs).preprocess(pcs, tss, poses, 0.4)
    torch.cuda.synchronize()
    for a, b in zip(got, ref):
        for key in ("distorted", "samples", "samples_f32", "indices", "count"):
            _same(a[key], b[key], key)
    batch.close()
    for c in ctxs + ref_ctxs:
        c.close()


def test_frame_struct_layout_and_chain_refusal(torch_cuda):
    """ctypes.sizeof(IcpPreprocessFrame) is the header's struct; a chain other than the mi355x grid-sample chain is
    refused by MI355XPreprocessingBatch with a clear message."""
    from pylidar_slam_amd import _lib
    from pylidar_slam_amd.odometry import MI355XPreprocessingBatch
    # xyz, n, timestamps, rel_pose[16] (float64), distorted_out, samples_out, samples_f32_out, indices_out, count_out
    assert C.sizeof(_lib.IcpPreprocessFrame) == 8 * 3 + 16 * 8 + 8 * 5
    assert _lib.IcpPreprocessFrame.rel_pose.offset == 24 and _lib.IcpPreprocessFrame.count_out.offset == 184
    cfg = _yaml_chain()
    other = {"0": cfg["0"], "1": cfg["2"], "2": cfg["3"]}  # no distortion filter
    with pytest.raises(AssertionError, match="batches the chain"):
        MI355XPreprocessingBatch(other, 2)
    voxelized = copy.deepcopy(cfg)
    voxelized["2"]["filter_name"] = "voxelization"
    with pytest.raises(AssertionError, match="batches the chain"):
        MI355XPreprocessingBatch(voxelized, 2)
