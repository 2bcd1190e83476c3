"""Every iteration of the fused hash-grid registration against a float64 Gauss-Newton step (tests/iteration_audit.py).

The rest of the suite pins this path on itself (about 60 schedules give the bits of "default") and on final poses at
1e-4 m / 1e-4 rad with per-iteration losses at 2e-3 — bars a self-correcting loop meets with 0.2 % of its rows missing.
Here runs of k = 1 .. K iterations (threshold 0: each a prefix of the next, asserted to the bit) expose EVERY iteration:
`icp_last_neighbors` gives the neighbour of every target and the pose of the last iteration of a run, a search of the map
points themselves gives the library's own (possibly carried) normals, and the step is recomputed on the host from exactly
those — float32 rows operation by operation, exact sums — and held to dx atol 2e-7 / rtol 2e-5, loss 1e-5, the row count
exactly; the neighbours to the kd-tree (mismatches: squared-distance ties within 2e-6, at most 0.1 % of the rows), the
normals to O.knn_normals, the next pose to the oracle's float32 pose algebra at 1e-6.  Single contexts and default options
unless a case says otherwise; `handoff_fallbacks() == 0` in every audited context (truncated_runs).

tests/test_iteration_audit.py shows on the CPU that each of the four checks fails the wrong copy meant for it.
The worst figures of every family are printed and quoted in the docstrings below (measured on an MI355X).
"""
import numpy as np
import pytest

import iteration_audit as A

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (no CPU fallback exists for the product path)")
    return torch


def _maker(model, scheme="geman_mcclure", sigma=0.3, h=32, w=1024, opts=None, cost=None, **kw):
    from pylidar_slam_amd.engine import IcpContext

    def make(k):
        ctx = IcpContext(height=h, width=w, max_num_alignments=k, threshold_delta_pose=0.0, scheme=scheme, sigma=sigma, **kw)
        for name, value in (opts or {}).items():
            ctx.set_option(name, value)
        if cost == "point_to_point":
            ctx.set_cost("point_to_point_gauss_newton")
        ctx.map_set(model)
        return ctx
    return make


def _audit(name, worst, model, targets, K, scheme="geman_mcclure", sigma=0.3, init=None, skip_null=False,
           cost="point_to_plane", observable=True, duplicates=False, **maker):
    """truncated_runs + audit_run of one case; returns (records, (status, result) of run K)."""
    init = np.eye(4, dtype=F32) if init is None else np.asarray(init, F32)
    records, mp, nm, last = A.truncated_runs(_maker(model, scheme, sigma, cost=cost, **maker), targets, init, K, skip_null)
    assert np.array_equal(mp, np.asarray(model, F32)), name  # map_set: the map as given, in its order
    if observable:
        assert all(r.ix is not None for r in records), f"{name}: the neighbours of the iterations were not observable"
    A.audit_run(name, records, targets, mp, nm, scheme, sigma, cost, skip_null, init, worst, duplicates=duplicates,
                k_normals=maker.get("num_neighbors_normals", 10))
    return records, last


# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", A.SIZES)
def test_sizes(torch_cuda, n):
    """geman_mcclure 0.3, K = 6, n rows of a 32 x 1024 scan against a 30 000-point map; n < 6 and any n the oracle finds
    singular report the oracle's status.
    Measured: 92 iterations audited, dx equal to the oracle's in every float32 bit (|ddx| 0), dloss <= 3.6e-16, no
    neighbour differs from the kd-tree's, pose chain <= 9.4e-8; n = 1 and 2 are an Invalid Jacobian at iteration 1 on both
    sides, n = 6 and 7 solve on both sides (reference spread <= 2e-11: no case widened)."""
    scan, model = A.small_scene()
    worst = A.Worst(f"sizes n={n}")
    records, (rc, res) = _audit(f"n={n}", worst, model, A.subset(scan, n), 6)
    print(worst)
    if n < 6:
        assert rc == A.ICP_ERR_INVALID_JACOBIAN and res.iterations == 1
    else:
        assert len(records) == res.iterations


@pytest.mark.parametrize("n", [130_560, 131_071, 131_072])
def test_full_size(torch_cuda, n):
    """64 x 2048 against the 100 000-point map of the C2 tests, K = 20: 255 super-rows, one row short of 256, and 256 (the
    `ns == 256` branch of sum_partials_vt).
    Measured, over the 3 x 20 iterations: |ddx| <= 1.4e-17, dloss <= 4.1e-16, no neighbour mismatch among 131 072 rows,
    min |dot| 0.9999999, pose chain <= 1.9e-9."""
    scan, model = A.c2_inputs()
    worst = A.Worst(f"full size n={n}")
    records, (rc, res) = _audit(f"full n={n}", worst, model, np.ascontiguousarray(scan[:n]), 20, h=64, w=2048)
    print(worst)
    assert rc == 0 and res.iterations == 20 and len(records) == 20


@pytest.mark.parametrize("case", ["rows_131073", "rows_196608", "no_carry", "bench_options"])
def test_full_size_variants(torch_cuda, case):
    """More rows than pixels as a plain [N,3] cloud (131 073 and 196 608: 257 and 384 super-rows), one run with
    carry_normals 0, and the option set of the benchmark's batched leg (wide_until 0, cell_lists 1).
    `icp_register` accepts more rows than the image has pixels (every buffer is sized by the row count), and
    `icp_last_neighbors` serves the bench option set.  Measured, 4 x 20 iterations: |ddx| 0, dloss <= 5.9e-16, no
    mismatch, pose chain <= 1.9e-9."""
    from test_gpu_batch import BENCH_OPTIONS
    worst = A.Worst(f"full size {case}")
    targets, model, opts = A.full_size_variant(case)
    assert case != "bench_options" or opts == BENCH_OPTIONS
    records, (rc, res) = _audit(case, worst, model, targets, 20, h=64, w=2048, opts=opts)
    print(worst)
    assert rc == 0 and res.iterations == 20 and res.num_targets == targets.shape[0]


@pytest.mark.parametrize("scheme", A.SCHEMES)
def test_schemes(torch_cuda, scheme):
    """All eight weight schemes at 32 x 1024, K = 8, sigma per scheme so that both branches occur (A.SCHEME_SIGMA; the CPU
    suite takes the census).
    Measured, 8 x 8 iterations: |ddx| <= 1.9e-9 (exp; 0 for the schemes without expf / logf), dloss <= 4.0e-8 (cauchy:
    logf against numpy's log), no mismatch, pose chain <= 1.9e-9."""
    scan, model = A.small_scene()
    worst = A.Worst(f"scheme {scheme}")
    _, (rc, res) = _audit(scheme, worst, model, scan, 8, scheme, A.SCHEME_SIGMA[scheme], skip_null=True)
    print(worst)
    assert rc == 0 and res.iterations == 8


@pytest.mark.parametrize("scheme,sigma", A.P2P_CASES)
def test_point_to_point_cost(torch_cuda, scheme, sigma):
    """The point-to-point cost (`set_cost`) runs unfused: `icp_last_neighbors` does not serve it.  Rows and solve are
    audited with the kd-tree's neighbours at the pose the chain gives (the initial pose, then the pose the previous run
    returned); there is no neighbour or normal check in this mode.
    Measured, 3 x 8 iterations: |ddx| <= 3.7e-9, dloss <= 4.3e-9, pose chain <= 6.0e-8."""
    scan, model = A.small_scene()
    worst = A.Worst(f"point to point {scheme}")
    records, (rc, res) = _audit(f"p2p {scheme}", worst, model, scan, 8, scheme, sigma, skip_null=True, cost="point_to_point",
                                observable=False)
    print(worst)
    assert rc == 0 and res.iterations == 8 and all(r.ix is None for r in records)


@pytest.mark.parametrize("case", ["blocks", "one_left", "all_masked"])
def test_masks(torch_cuda, case):
    """NaN and null rows under skip_null that empty whole 128-row and 512-row blocks, straddle their borders and leave
    exactly one valid row in a block.  An all-masked scan sums no row: ||r|| = 0 < 1e-7 is the residual guard of the
    reference's GaussNewton at the first iteration — one iteration, converged, dx = 0, loss 0, the initial pose returned
    (the audit holds the record to exactly that).
    Measured: |ddx| 0, dloss <= 2.3e-16, no mismatch, masked rows -1 and no others, pose chain <= 1.9e-9."""
    scan, model = A.small_scene()
    targets = A.mask_cases(scan)[case]
    worst = A.Worst(f"masks {case}")
    init = A.O.build_pose_matrix(np.array([0.05, -0.02, 0.01, 0.001, -0.002, 0.004], F32))
    records, (rc, res) = _audit(case, worst, model, targets, 6, init=init, skip_null=True)
    print(worst)
    if case == "all_masked":
        assert rc == 0 and res.iterations == 1 and res.num_targets == 0 and res.converged and len(records) == 1
        assert np.array_equal(res.pose, init) and res.losses[0] == 0.0 and not res.dx.any()
        assert (records[0].ix == -1).all()
    else:
        assert rc == 0 and res.iterations == 6 and res.num_targets == int(A.valid_rows(targets, True).sum())


def test_far_targets(torch_cuda):
    """The recipe of test_targets_far_from_the_map_in_the_fused_kernel — coarse rings and the exhaustive scan — audited at
    every iteration, not only the last.
    Measured, 4 iterations: |ddx| 0, dloss <= 3.8e-16, no mismatch (the 59 far rows included), pose chain <= 9.3e-10."""
    frame, model = A.far_targets()
    worst = A.Worst("far targets")
    _, (rc, res) = _audit("far", worst, model, frame, 4, h=64, w=2048)
    print(worst)
    assert rc == 0 and res.iterations == 4 and res.num_targets == 6000


@pytest.mark.parametrize("case", A.MAP_CASES)
def test_maps(torch_cuda, case):
    """Maps of 5 and 11 points (5: fewer than k + 1, the reference has no neighbourhood of k and the library's normals are
    held to unit norm; 11 = k + 1: every other point is a neighbour, compared with O.knn_normals), a map with exact duplicates (the tie goes to the lowest index, the rows are unaffected), and map, scan and
    initial pose moved together by 1 km and 10 km (float32 cancellation, faithful to the reference: the oracle sees the same
    float32; these are the cases the tolerance rule may widen — printed per iteration).
    Measured: |ddx| 0 and dloss <= 2.4e-16 everywhere but at 10 km; 5 points: Invalid Jacobian at iteration 4 on both
    sides; duplicates: every neighbour the lowest index of its equal points; pose chain <= 6.1e-8.  WIDENED by the tolerance
    rule (max(2e-7, 4 x |inv(H) g - Cholesky solve| in float64)), 10 km only: iteration 1 reference spread 4.93e-7 -> dx
    atol 1.97e-6, measured |ddx| 5.96e-7; iteration 2 spread 6.0e-8 -> atol 2.4e-7, measured 1.19e-7; iterations 3-6 at
    the project bar (|ddx| <= 3.0e-8).  1 km: spread <= 3.4e-12, not widened."""
    worst = A.Worst(f"maps {case}")
    model, targets, init = A.map_case(case)
    _audit(case, worst, model, targets, 6, init=init, duplicates=case == "duplicates")
    print(worst)


@pytest.mark.parametrize("case", list(A.POSE_CASES))
def test_initial_poses(torch_cuda, case):
    """An initial yaw of 3 rad, an initial pitch of exactly float32(pi / 2) (the `sy < 1e-6` branch of wave_from_pose_f32)
    and a far-off initial pose (0.5 m / 0.05 rad: the early iterations take the search paths, the late ones the cache).
    Measured, 3 x 8 iterations: |ddx| <= 5.6e-17, dloss <= 3.5e-16, no mismatch, pose chain <= 6.0e-8 (yaw 3 rad),
    1.58e-7 (pitch pi / 2: the gimbal branch at the first update), 9.3e-10 (far off)."""
    _, model = A.small_scene()
    worst = A.Worst(f"initial pose {case}")
    targets, init = A.pose_case(case)
    _, (rc, res) = _audit(case, worst, model, targets, 8, init=init)
    print(worst)
    assert rc == 0 and res.iterations == 8


def test_guards(torch_cuda):
    """A scan that is an exact subset of the map with an identity initial pose stops after one iteration, converged,
    dx = 0, loss = sum r^2, pose untouched; a plane over a plane is an Invalid Jacobian at the audited iteration.
    Measured: both exactly as the oracle has them (loss 0.0 for the subset; det H = 0 by LU and by Cholesky for the plane)."""
    scan, model = A.small_scene()
    worst = A.Worst("guards")
    records, (rc, res) = _audit("subset", worst, model, np.ascontiguousarray(model[::3]), 3)
    assert rc == 0 and res.iterations == 1 and res.converged and not res.dx.any() and res.losses[0] == 0.0
    assert np.array_equal(res.pose, np.eye(4, dtype=F32)) and len(records) == 1
    pmap, over = A.plane_case()
    records, (rc, res) = _audit("plane", worst, pmap, over, 3)
    assert rc == A.ICP_ERR_INVALID_JACOBIAN and res.iterations == 1 and not res.converged and len(records) == 1
    print(worst)


def test_chained_frames(torch_cuda):
    """Three frames with register_launch / map_update(None, None) / register_end and init = "last": every iteration of
    every frame against the map as re-expressed (`map_points()`) — the carried normals (rotated with the pose-only update,
    held to the same |dot| > 1 - 1e-5 against fresh estimates as any other) and the frame seeds included.
    Measured, 3 x 6 iterations: |ddx| 0, dloss <= 2.3e-16, no mismatch, carried normals |dot| >= 0.9999997 against fresh
    estimates, the first pose of frames 1 and 2 bit-equal to the pose of the frame before, pose chain <= 1.9e-9."""
    from pylidar_slam_amd.engine import IcpContext
    scans, model = A.small_sequence()
    K, scheme, sigma = 6, "geman_mcclure", 0.3
    worst = A.Worst("chained frames")
    poses = []
    for f in range(3):
        def make(k, f=f):
            ctx = IcpContext(height=32, width=1024, max_num_alignments=K, threshold_delta_pose=0.0, scheme=scheme, sigma=sigma)
            ctx.map_set(model)
            for g in range(f):
                ctx.register_launch(scans[g], "last" if g else None, skip_null=True)
                ctx.map_update(None, None)
                ctx.register_end()
            ctx.set_alignment(scheme, sigma, k, 0.0)
            return ctx

        def register(ctx, targets, init, skip_null, f=f):
            ctx.register_launch(targets, "last" if f else None, skip_null=skip_null)
            return A.raw_register_end(ctx)

        init = poses[-1] if f else np.eye(4, dtype=F32)
        records, mp, nm, (rc, res) = A.truncated_runs(make, scans[f], init, K, True, register)
        assert rc == 0 and res.iterations == K and all(r.ix is not None for r in records)
        assert f == 0 or not np.array_equal(mp, model)  # the map was re-expressed
        A.audit_run(f"frame {f}", records, scans[f], mp, nm, scheme, sigma, "point_to_plane", True, init, worst)
        poses.append(res.pose)
    print(worst)


@pytest.mark.parametrize("threshold", [1e-4, 1e-3])
def test_live_threshold(torch_cuda, threshold):
    """threshold_delta_pose live: `iterations` is the first k with ||dx_k||_2 < threshold, computed in float32 from the
    returned steps, and the last iteration passes the full audit (its pose is the returned one: the loop breaks before the
    update).
    Measured: 5 iterations at 1e-4 (||dx|| 3.6e-1, 3.9e-2, 3.7e-3, 3.2e-4, 2.8e-5), 4 at 1e-3; the last one |ddx| 0."""
    from pylidar_slam_amd.engine import IcpContext
    scan, model = A.small_scene()
    ctx = IcpContext(height=32, width=1024, max_num_alignments=40, threshold_delta_pose=threshold, scheme="geman_mcclure",
                     sigma=0.3)
    ctx.map_set(model)
    rc, res = A.raw_register(ctx, scan, None, True)
    rec, mp, nm = A.observe(ctx, rc, res, scan.shape[0])
    assert ctx.handoff_fallbacks() == 0
    ctx.close()
    norms = np.array([np.sqrt((d.astype(F32) ** 2).sum(dtype=F32)) for d in res.dx])
    below = np.nonzero(norms < F32(threshold))[0]
    print(f"threshold {threshold}: {res.iterations} iterations, ||dx|| {norms}")
    assert rc == 0 and len(below) and res.iterations == below[0] + 1 and res.converged
    assert rec is not None and rec.ix is not None and rec.k == res.iterations
    worst = A.Worst(f"live threshold {threshold}")
    A.audit_run(f"threshold {threshold}", [rec], scan, mp, nm, "geman_mcclure", 0.3, "point_to_plane", True, None, worst)
    assert np.array_equal(res.pose[:3], rec.pose12)
    print(worst)
