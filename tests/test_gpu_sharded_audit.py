"""The scan-sharded registration on the device, shard by shard, against float64 (tests/sharded_audit.py).

The multi-GPU seam (icp_register_begin / icp_iteration_accumulate / icp_normal_equations_ptr /
icp_set_normal_equations_buffer / icp_iteration_solve) has never run on two physical GPUs; what ONE GPU can show is the rank
arithmetic.  A `SimulatedWorld` holds W contexts with the same map in this process, gives each its slice and sums the 32
doubles itself in rank order; runs of k = 1 .. K = 6 forced iterations are bit-for-bit prefixes of each other, so every
iteration is held on its own: A every rank's vector to the model of its shard (row count exact, 29 sums within
2 n 2^-53 sum |a_i b_i|, an empty shard exact zeros, the pad 0.0), B the rank-order total to what one context accumulates
from the whole scan at the same pose, C every rank's step to the float64 solve of the total the test wrote (half a float32
ulp + 4 x the spread of three float64 solves; the loss bit-equal to element 27), D all ranks bit-equal, E one rank no
special case, F no row without a unique float32 neighbour (tests/test_sharded_audit.py asserts that for these clouds on the
CPU, and that every check fails the wrong copy meant for it).

Scans of at most 4 097 rows against maps of 7 500 - 11 600 points; contexts are created once per module and option set.
The worst figure of every check is printed by each test and quoted in its docstring (measured on an MI355X).

More than 256 partial rows in one launch: the default (512-query) shape of launch_iterate_fused writes ceil(n / 512)
super-rows, so the 257th appears at n = 131 073 — far above the sizes of this file; tests/test_gpu_iteration_audit.py
(test_full_size: 131 071 / 131 072, test_full_size_variants: 131 073) holds those launches to the same row model.
"""
import numpy as np
import pytest

import iteration_audit as IA
import sharded_audit as S

pytestmark = pytest.mark.gpu
F32 = np.float32
K = 6
SCHEME, SIGMA = "geman_mcclure", 0.3
_POOL, _NORMALS = {}, {}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (no CPU fallback exists for the product path)")
    yield torch
    for ctxs in _POOL.values():
        for c in ctxs:
            c.close()
    _POOL.clear()
    _NORMALS.clear()


def _new_context(model, opts, cost):
    from pylidar_slam_amd.engine import IcpContext
    ctx = IcpContext(height=32, width=1024, max_num_alignments=K, threshold_delta_pose=0.0, scheme=SCHEME, sigma=SIGMA)
    for name, value in opts:
        ctx.set_option(name, value)
    if cost == "point_to_point":
        ctx.set_cost("point_to_point_gauss_newton")
    ctx.map_set(model)
    return ctx


def _contexts(map_name, model, rank_opts, cost="point_to_plane"):
    """One pooled context per entry of `rank_opts` (a dict of options each), all holding `model`."""
    used, out = {}, []
    for opts in rank_opts:
        key = (map_name, tuple(sorted((opts or {}).items())), cost)
        pool = _POOL.setdefault(key, [])
        i = used.get(key, 0)
        used[key] = i + 1
        if i == len(pool):
            pool.append(_new_context(model, key[1], cost))
        out.append(pool[i])
    return out


def _normals(map_name, model):
    """The library's own normal of every map point (eager estimation, default options), read once per map."""
    if map_name not in _NORMALS:
        ctx = _new_context(model, (), "point_to_plane")
        _NORMALS[map_name] = IA.kernel_normals(ctx, model)
        assert np.array_equal(ctx.map_points(), np.asarray(model, F32))
        ctx.close()
    return _NORMALS[map_name]


def _world(ranks, scheme, sigma, threshold=0.0):
    def make(k):
        for c in ranks:
            c.set_alignment(scheme, sigma, k, threshold)
        return S.SimulatedWorld(ranks)
    return make


def _audit(name, worst, map_name, model, shards, scheme=SCHEME, sigma=SIGMA, opts=None, cost="point_to_plane",
           skip_null=False, init=None, squares32=False, iterations=K, checks="ABCDF"):
    """audit_world of one case on pooled contexts: W ranks + one more context of rank 0's options for the whole scan."""
    rank_opts = opts if isinstance(opts, list) else [opts] * len(shards)
    ctxs = _contexts(map_name, model, rank_opts + [rank_opts[0]], cost)
    ranks, whole = ctxs[:-1], ctxs[-1]
    whole.set_alignment(scheme, sigma, iterations, 0.0)
    normals = _normals(map_name, model) if cost == "point_to_plane" else None
    last, _ = S.audit_world(name, _world(ranks, scheme, sigma), whole, model, normals, shards, init, iterations, scheme,
                            sigma, cost, skip_null, squares32, worst, checks)
    return last, ranks


# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,world", S.BOUNDS_CUTS)
def test_cuts_of_shard_bounds(torch_cuda, n, world):
    """Every cut distributed.shard_bounds makes at the sizes where the kernels take another path: one row, a world larger
    than the scan (n = 1 of 2 and 5 of 8: empty ranks, which contribute exact zeros), 3 + 3 + 1, 257 + 256, 257 x 3 + 254,
    1 366 x 2 + 1 364 and 513 x 7 + 506.  n = 1 and 5 are an Invalid Jacobian at iteration 1 on every rank alike.
    Measured, 33 iterations and 131 shard vectors: A the worst sum at 0.268 of its bound (n = 7: three rows a shard; <=
    0.008 from 513 rows on), B the total at 0.143 (n = 7; <= 0.002), C |ddx| at <= 0.983 of a bar of 1.49e-8 — half a
    float32 ulp of the step, which the rounding of the returned float32 alone uses up; the spread of the float64 solves
    is <= 2.1e-15 —, every loss bit-equal to element 27, every empty rank exact zeros, F 0 rows, pose chain <= 1.9e-9."""
    model = S.scene()[1]
    worst = S.Worst(f"shard_bounds n={n} W={world}")
    last, _ = _audit(f"n={n} W={world}", worst, "scene", model, S.bounds_cut(S.cloud(n), world))
    print(worst)
    rc, res = last.results[0]
    if n < 6:
        assert rc == IA.ICP_ERR_INVALID_JACOBIAN and res.iterations == 1
    assert res.num_targets == n


@pytest.mark.parametrize("name", list(S.ABI_CUTS) + ["nan_shard", "null_shard"])
def test_cuts_the_abi_allows(torch_cuda, name):
    """Cuts shard_bounds never makes: 1 + 4 095, 4 095 + 1, 0 + 4 096, 2 048 + 0 + 2 048, a rank of 300 NaN rows between
    513 and 512 rows, and a rank of 300 null rows under skip_null.  An empty or all-invalid rank contributes exact zeros
    in every iteration.
    Measured, 6 x 6 iterations: A <= 0.002 of the bound, B <= 0.001, C <= 0.994 of 1.49e-8, zeros exact, F 0 rows."""
    model = S.scene()[1]
    if name in S.ABI_CUTS:
        shards, skip = S.cut(S.cloud(sum(S.ABI_CUTS[name])), S.ABI_CUTS[name]), False
    else:
        shards = S.cut(S.cloud(1025), (513, 512))
        shards.insert(1, S.nan_shard(300) if name == "nan_shard" else S.null_shard(300))
        skip = name == "null_shard"
    worst = S.Worst(f"ABI cut {name}")
    last, _ = _audit(name, worst, "scene", model, shards, skip_null=skip)
    print(worst)
    assert last.results[0][0] == 0 and last.results[0][1].iterations == K
    for part in last.parts:
        for rank, rows in enumerate(shards):
            if not IA.valid_rows(rows, skip).any():
                assert not part[rank].any()


def test_ranks_of_different_workgroup_widths(torch_cuda):
    """Rank 0 with `wide_until` 0 (512-thread workgroups from the first iteration), rank 1 with the default (1 024-thread
    workgroups in the early iterations), on shards of 511 and 1 025 rows.
    Measured: A 0.002, B 0.001, C 0.991 of 1.49e-8, pose chain 4.7e-10."""
    model = S.scene()[1]
    worst = S.Worst("widths")
    last, _ = _audit("widths", worst, "scene", model, S.cut(S.cloud(1536), (511, 1025)), opts=[{"wide_until": 0}, {}])
    print(worst)
    assert last.results[0][0] == 0 and last.results[0][1].iterations == K


@pytest.mark.parametrize("scheme", IA.SCHEMES)
def test_schemes(torch_cuda, scheme):
    """All eight weight schemes at n = 1 025, W = 4, the sigmas of iteration_audit.SCHEME_SIGMA.
    Measured, 8 x 6 iterations: A <= 0.008 of the bound without expf / logf, 0.055 (exp), 0.034 (neighborhood), 0.033
    (cauchy) of the bound with alignment_audit.TRANSCENDENTAL_BOUND; B <= 0.002; C <= 0.989 of its bar; F 0 rows."""
    model = S.scene()[1]
    worst = S.Worst(f"scheme {scheme}")
    last, _ = _audit(scheme, worst, "scene", model, S.bounds_cut(S.cloud(1025), 4), scheme, IA.SCHEME_SIGMA[scheme])
    print(worst)
    assert last.results[0][0] == 0 and last.results[0][1].iterations == K


PATHS = {"fused": ({}, "point_to_plane", False),
         "unfused": ({"fuse_iteration": 0}, "point_to_plane", True),
         "point_to_point": ({}, "point_to_point", True),
         "lazy_fused": ({"eager_normals_limit": 0, "lazy_fused": 2}, "point_to_plane", False),
         "lazy_unfused": ({"eager_normals_limit": 0, "lazy_fused": 0}, "point_to_plane", True)}


@pytest.mark.parametrize("path", list(PATHS))
def test_every_path_behind_accumulate(torch_cuda, path):
    """n = 1 025, W = 3 on the fused kernel, with `fuse_iteration` 0, with the point-to-point cost, and with the normals
    estimated on demand (`eager_normals_limit` 0) inside the fused kernel (`lazy_fused` 2) and in front of the unfused
    reduction (`lazy_fused` 0): there every rank estimates another subset of the normals, and the vectors are still those
    of the model with the eagerly estimated normals.  The unfused and point-to-point rows add the float32 squares in
    elements 27 and 28 (RowAcc::add_row), the fused kernels the float64 products: the model follows each.
    Measured, 5 x 6 iterations: A <= 0.006, B 0.001, C <= 0.958 of 1.49e-8 (point-to-point: 0.997 of 5.96e-8), pose chain
    <= 9.3e-10 (point-to-point 6.0e-8); a fresh context with the lazy options estimates fewer than a quarter of the map's
    normals for one shard."""
    opts, cost, squares32 = PATHS[path]
    model = S.scene()[1]
    worst = S.Worst(f"path {path}")
    last, ranks = _audit(path, worst, "scene", model, S.bounds_cut(S.cloud(1025), 3), opts=opts, cost=cost,
                         squares32=squares32)
    print(worst)
    assert last.results[0][0] == 0 and last.results[0][1].iterations == K
    if path.startswith("lazy"):  # (the pooled contexts hold their normals by now: a fresh one shows the schedule of the options)
        fresh = _new_context(model, tuple(sorted(opts.items())), cost)
        computed = fresh.register(S.bounds_cut(S.cloud(1025), 3)[0]).normals_computed
        fresh.close()
        assert 0 < computed < len(model) // 4, computed


def test_live_stop_second_registration_and_driver(torch_cuda):
    """Live thresholds halfway between consecutive float32 step norms of a forced run: every rank stops at the iteration
    the norms name with the pose held, and the driver's remaining accumulate / sum / solve calls — behind the stop
    k_sum_partials writes nothing, the world goes on summing the stale vectors W-fold per call — change no bit of any
    result.  A second registration on the same contexts, with an empty rank among them, passes A-D from its first
    iteration; and `distributed.sharded_register` on one context without a process group is the world's rank 0 at W = 1,
    bit for bit.
    Measured: five thresholds, stops at iterations 2, 3, 4, 5 and 6 of 6; behind a stop the count element of the totals
    grew 4-, 16-, 64-, 256-fold and no result bit changed; the second registrations (256 + 0 + 1 + 256 rows): A 0.007,
    B 0.002, C 0.907, the empty rank exact zeros; the driver equal to the world in every bit."""
    from pylidar_slam_amd.distributed import sharded_register
    model = S.scene()[1]
    shards = S.bounds_cut(S.cloud(1025), 4)
    ranks = _contexts("scene", model, [{}] * 4)
    forced = _world(ranks, SCHEME, SIGMA)(K).run(shards, None, K)
    assert not S.check_ranks_agree(forced.results)
    norms = [S.norm32(d) for d in forced.results[0][1].dx]
    cases = S.thresholds_between(norms)
    assert len(cases) >= 3, norms
    fails = []
    for thr, stop in cases:
        live = _world(ranks, SCHEME, SIGMA, thr)(K).run(shards, None, K)
        exact = _world(ranks, SCHEME, SIGMA, thr)(K).run(shards, None, stop)
        held = np.eye(4, dtype=F32) if stop == 1 else \
            _world(ranks, SCHEME, SIGMA)(stop - 1).run(shards, None, stop - 1).results[0][1].pose
        fails += S.check_stop(live.results, stop, held, exact.results) + S.check_ranks_agree(live.results)
        for k in range(1, stop + 1):
            fails += S.check_solve(k, live.totals[k - 1], live.results, thr, K)[0]
        growth = [float(live.totals[k][29] / live.totals[stop - 1][29]) for k in range(stop, K)]
        print(f"  threshold {thr:.3e}: stop at iteration {stop} of {K}; the count element of the totals behind it grew "
              f"{growth}-fold")
        # (stale contents behind the stop are what the NEXT registration must not see)
        second = S.Worst(f"second registration behind the stop at {stop}")
        _audit(f"second after stop {stop}", second, "scene", model, S.cut(S.cloud(513), (256, 0, 1, 256)), iterations=3)
        print(second)
    assert not fails, fails
    # the driver itself, no process group: the world at W = 1
    ctx = ranks[0]
    rows = S.cloud(1025)
    ctx.set_alignment(SCHEME, SIGMA, K, 0.0)
    seam = S.SimulatedWorld([ctx]).run([rows], None, K).results[0]
    driver = S.ended(lambda: sharded_register(ctx, rows, None, K))
    assert not S.check_one_rank(seam, driver, "sharded_register")


@pytest.mark.parametrize("n", [1, 7, 513, 4097])
def test_one_rank_is_no_special_case(torch_cuda, n):
    """W = 1 through the seam is `register` on the same rows and the in-library exchange at world 1, bit for bit.
    Measured: equal at n = 1 (Invalid Jacobian at iteration 1), 7 (Invalid Jacobian at iteration 6), 513 and 4 097."""
    model = S.scene()[1]
    rows = S.cloud(n)
    ctx, plain, solo = _contexts("scene", model, [{}] * 3)
    for c in (ctx, plain, solo):
        c.set_alignment(SCHEME, SIGMA, K, 0.0)
    seam = S.SimulatedWorld([ctx]).run([rows], None, K).results[0]
    fails = S.check_one_rank(seam, IA.raw_register(plain, rows), "register")
    solo.exchange_connect([solo.exchange_create(0, 1)])
    try:
        fails += S.check_one_rank(seam, IA.raw_register(solo, rows), "the in-library exchange at world 1")
    finally:
        solo.exchange_destroy()
    assert not fails, fails
    print(f"  n={n}: status {seam[0]}, {seam[1].iterations} iterations, the three results equal in every bit")


def test_guards_on_the_summed_system(torch_cuda):
    """A shard of rows on a single plane (iteration_audit.plane_case: singular alone) beside a regular shard: no rank
    fails and the totals pass A-D.  Both shards on that plane: every rank reports Invalid Jacobian at iteration 1 with the
    same result handed over.  Targets 1-6 m and hundreds of metres from the map (iteration_audit.far_targets) on one rank
    only.
    Measured, 13 iterations: A 0.003, B 0.001, C 0.988 of 1.49e-8 (spread 7.2e-16); the plane shard's own 6 x 6 system is
    singular by LU and by Cholesky; 60 far rows."""
    gmap, plane, regular = S.guard_scene()
    worst = S.Worst("guards")
    last, _ = _audit("plane + regular", worst, "guard", gmap, [plane, regular])
    assert last.results[0][0] == 0 and last.results[0][1].iterations == K
    alone = S.solve_total(last.parts[0][0])
    assert alone["invalid"] and not alone["undetermined"], alone["det"]  # (the plane shard IS singular on its own)
    last, _ = _audit("plane + plane", worst, "guard", gmap, S.bounds_cut(plane, 2))
    assert all(rc == IA.ICP_ERR_INVALID_JACOBIAN and res.iterations == 1 and not res.converged for rc, res in last.results)
    with_far, near, fmap, count = S.far_scene()
    assert count >= 40
    last, _ = _audit("far + near", worst, "far", fmap, [with_far, near])
    print(worst)
    assert last.results[0][0] == 0 and last.results[0][1].iterations == K


@pytest.mark.parametrize("family", ["yaw_3rad", "offset_10km"])
def test_poses_and_maps(torch_cuda, family):
    """iteration_audit.pose_case("yaw_3rad") and map_case("offset_10km") at W = 2, 4 097 rows.  At 10 km from the origin
    the 6 x 6 system is ill-conditioned: the bar of C is the spread of the model's own float64 solves there.
    Measured: yaw 3 rad A 0.001, B 0.000, C 0.975 of 1.49e-8; 10 km A 0.000, B 0.001, C 0.457 of a bar of 1.49e-6 (the
    three float64 solves of the total are 2.5e-7 apart), F 0 rows."""
    model, rows, init = S.device_cloud(family)
    worst = S.Worst(family)
    last, _ = _audit(family, worst, family if family == "offset_10km" else "scene", model, S.bounds_cut(rows, 2), init=init)
    print(worst)
    assert last.results[0][1].iterations >= 1
