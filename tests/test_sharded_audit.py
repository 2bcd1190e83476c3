"""The accounting of tests/sharded_audit.py on the CPU: `SimulatedWorld` and checks A-F on engines that answer from the
model itself (ModelEngine: test_distributed_gloo.OracleEngine with the row model, guards, stop and `done` of the library),
on the cuts and the clouds tests/test_gpu_sharded_audit.py runs on the device — and deliberately wrong copies, each of which
must be reported by the check meant for it, by name."""
import numpy as np
import pytest
import torch
from scipy.spatial import cKDTree

import iteration_audit as IA
import sharded_audit as S

F32, F64 = np.float32, np.float64
K = 6
SCHEME, SIGMA = "geman_mcclure", 0.3


@pytest.fixture(scope="module")
def engine_class():
    return S.model_engine_class()


@pytest.fixture(scope="module")
def scene_normals():
    return IA.oracle_normals(S.scene()[1])


def _world_maker(engine_class, model, normals, W, wrong=None, world_class=S.SimulatedWorld, threshold=0.0, **kw):
    """make_world(k): W fresh engines of k iterations; `wrong` = {rank: name of the wrong copy}."""
    def make(k):
        return world_class([engine_class(model, normals, SCHEME, SIGMA, iterations=k, threshold=threshold,
                                         wrong=(wrong or {}).get(r), **kw) for r in range(W)])
    return make


def _audit(engine_class, model, normals, shards, wrong=None, world_class=S.SimulatedWorld, iterations=K, init=None,
           skip_null=False, **kw):
    whole = engine_class(model, normals, SCHEME, SIGMA, **kw)
    return S.audit_world("cpu", _world_maker(engine_class, model, normals, len(shards), wrong, world_class, **kw), whole,
                         model, normals, shards, init, iterations, SCHEME, SIGMA, skip_null=skip_null,
                         squares32=kw.get("squares32", False), cost=kw.get("cost", "point_to_plane"))


# ----------------------------------------------------------------------------------------------------------------------
def test_module_imports_without_a_gpu_and_cuts_tile():
    from pylidar_slam_amd.distributed import shard_bounds
    for n, w in S.BOUNDS_CUTS:
        sizes = [len(s) for s in S.bounds_cut(np.zeros((n, 3), F32), w)]
        assert sum(sizes) == n and sizes == [shard_bounds(n, w, r)[1] - shard_bounds(n, w, r)[0] for r in range(w)]
    assert [len(s) for s in S.bounds_cut(np.zeros((5, 3), F32), 8)] == [1, 1, 1, 1, 1, 0, 0, 0]
    assert [len(s) for s in S.bounds_cut(np.zeros((1025, 3), F32), 4)] == [257, 257, 257, 254]
    assert [len(s) for s in S.bounds_cut(np.zeros((4097, 3), F32), 8)] == [513] * 7 + [506]
    for sizes in S.ABI_CUTS.values():
        assert [len(s) for s in S.cut(np.zeros((sum(sizes), 3), F32), sizes)] == list(sizes)


def test_nn_f32_is_the_brute_force():
    """The candidate form of the float32 neighbour search gives the indices of iteration_audit.brute_force_nn_f32."""
    scan, model = S.scene()
    q = S.cloud(1025)
    ix, flagged = S.nn_f32(q, model, cKDTree(model.astype(F64)))
    assert np.array_equal(ix, IA.brute_force_nn_f32(q, model)) and not flagged.any()
    dup = np.concatenate([model[:50], model])  # exact duplicates: the lowest index, and every such row flagged
    ix, flagged = S.nn_f32(model[:50], dup, cKDTree(dup.astype(F64)))
    assert np.array_equal(ix, np.arange(50)) and flagged.all()


@pytest.mark.parametrize("n,world", S.BOUNDS_CUTS)
def test_bounds_cuts_on_the_model(engine_class, scene_normals, n, world):
    """The cuts of shard_bounds: the world's totals, steps and results pass A-F on the model's own engines (n < 6 is an
    Invalid Jacobian at iteration 1 on every rank alike)."""
    model = S.scene()[1]
    last, _ = _audit(engine_class, model, scene_normals, S.bounds_cut(S.cloud(n), world))
    rc, res = last.results[0]
    assert (rc == IA.ICP_ERR_INVALID_JACOBIAN and res.iterations == 1) if n < 6 else res.iterations >= 1
    assert res.num_targets == n


@pytest.mark.parametrize("name", list(S.ABI_CUTS) + ["nan_shard", "null_shard"])
def test_abi_cuts_on_the_model(engine_class, scene_normals, name):
    model = S.scene()[1]
    if name in S.ABI_CUTS:
        shards, skip = S.cut(S.cloud(sum(S.ABI_CUTS[name])), S.ABI_CUTS[name]), False
    else:
        shards = S.cut(S.cloud(1025), (513, 512))
        shards.insert(1, S.nan_shard(300) if name == "nan_shard" else S.null_shard(300))
        skip = name == "null_shard"
    last, _ = _audit(engine_class, model, scene_normals, shards, skip_null=skip, iterations=3)
    assert last.results[0][1].iterations == 3
    for part in last.parts:  # the empty / all-invalid rank contributed exact zeros
        for rank, rows in enumerate(shards):
            if not IA.valid_rows(rows, skip).any():
                assert not part[rank].any()


@pytest.mark.parametrize("kw", [dict(cost="point_to_point", squares32=True), dict(squares32=True)], ids=["p2p", "row_acc"])
def test_other_paths_on_the_model(engine_class, scene_normals, kw):
    _audit(engine_class, S.scene()[1], scene_normals, S.bounds_cut(S.cloud(1025), 3), iterations=3, **kw)


@pytest.mark.parametrize("name", S.DEVICE_CLOUDS)
def test_no_cloud_of_the_device_tests_is_flagged(engine_class, name):
    """F is a condition on the case: on every cloud the device tests register the model flags no row — no float32
    neighbour within TIE_RTOL / TIE_ABS of the nearest — at any pose of the model's own chain of K iterations."""
    model, rows, init = S.device_cloud(name)
    assert len(rows) <= 4097 and len(model) <= 12000
    normals = IA.oracle_normals(model)
    tree = cKDTree(model.astype(F64))
    eng = engine_class(model, normals, SCHEME, SIGMA, iterations=K)
    eng.register_begin(rows, init)
    for k in range(K):
        assert S.shard_model(model, normals, tree, rows, False, eng.pose[:3], SCHEME, SIGMA)["flagged"] == 0, (name, k)
        eng.iteration_accumulate()
        eng.iteration_solve()
        if eng.done:
            break


# ----------------------------------------------------------------------------------------------------------------------
# E, the stop, the exchange order
# ----------------------------------------------------------------------------------------------------------------------
def test_one_rank_and_the_driver(engine_class, scene_normals):
    """W = 1 through the world = the plain registration = distributed.sharded_register without a process group."""
    from pylidar_slam_amd.distributed import sharded_register
    model, rows = S.scene()[1], S.cloud(513)
    seam = S.SimulatedWorld([engine_class(model, scene_normals, SCHEME, SIGMA, iterations=K)]).run([rows], None, K).results[0]
    plain = S.ended(lambda: engine_class(model, scene_normals, SCHEME, SIGMA, iterations=K).register(rows))
    assert not S.check_one_rank(seam, plain, "register")
    driver = S.ended(lambda: sharded_register(engine_class(model, scene_normals, SCHEME, SIGMA, iterations=K), rows, None, K))
    assert not S.check_one_rank(seam, driver, "sharded_register")
    other = S.ended(lambda: engine_class(model, scene_normals, SCHEME, SIGMA, iterations=K).register(rows[:-1]))
    assert [c for c, _ in S.check_one_rank(seam, other, "register")] == ["E one rank"]


def _stop_case(engine_class, normals, wrong=None):
    model, shards = S.scene()[1], S.bounds_cut(S.cloud(1025), 4)
    forced = _world_maker(engine_class, model, normals, 4)(K).run(shards, None, K)
    norms = [S.norm32(d) for d in forced.results[0][1].dx]
    cases = S.thresholds_between(norms)
    assert len(cases) >= 3 and {s for _, s in cases} >= {2, 3, 4}
    fails = []
    for thr, stop in cases:
        live = _world_maker(engine_class, model, normals, 4, wrong, threshold=thr)(K).run(shards, None, K)
        exact = _world_maker(engine_class, model, normals, 4, threshold=thr)(K).run(shards, None, stop)
        held = np.eye(4, dtype=F32) if stop == 1 else \
            _world_maker(engine_class, model, normals, 4)(stop - 1).run(shards, None, stop - 1).results[0][1].pose
        fails += S.check_stop(live.results, stop, held, exact.results) + S.check_ranks_agree(live.results)
        for k in range(1, stop + 1):
            fails += S.check_solve(k, live.totals[k - 1], live.results, thr, K)[0]
    return fails


def test_live_stop(engine_class, scene_normals):
    assert not _stop_case(engine_class, scene_normals)


def test_exchange_order_is_not_seen_by_b_but_by_the_bit_comparison(engine_class, scene_normals):
    """The total summed in reverse rank order passes A-D — any order of W additions is within B's bound — and is caught by
    the comparison with the rank-order world, which is what the in-library exchange is held to on the device."""
    class Reversed(S.SimulatedWorld):
        def total(self, parts):
            return super().total(parts[::-1])
    model, shards = S.scene()[1], S.bounds_cut(S.cloud(4097), 8)
    rev, _ = _audit(engine_class, model, scene_normals, shards, world_class=Reversed, iterations=4)
    fwd = _world_maker(engine_class, model, scene_normals, 8)(4).run(shards, None, 4)
    assert [c for c, _ in S.check_exchange_order(fwd.results[0], rev.results[0])] == ["exchange order"]
    assert not S.check_exchange_order(fwd.results[0], fwd.results[1])


# ----------------------------------------------------------------------------------------------------------------------
# wrong copies
# ----------------------------------------------------------------------------------------------------------------------
def _checks_of(call):
    with pytest.raises(IA.AuditFailure) as e:
        call()
    print(" ", str(e.value)[:400])
    return set(e.value.checks)


def test_wrong_last_row_dropped(engine_class, scene_normals):
    shards = S.bounds_cut(S.cloud(1025), 4)
    assert "A row count" in _checks_of(lambda: _audit(engine_class, S.scene()[1], scene_normals, shards,
                                                      wrong={2: "last_row_dropped"}, iterations=2))


def test_wrong_shards_overlap_by_one_row(engine_class, scene_normals):
    """The wrong cut reaches engines and model alike: every shard is what it says (A passes), the total is not the scan's."""
    rows = S.cloud(1025)
    model = S.scene()[1]
    shards = [rows[:513], rows[512:]]
    whole = engine_class(model, scene_normals, SCHEME, SIGMA)
    make = _world_maker(engine_class, model, scene_normals, 2)
    run = make(1).run(shards, None, 1)
    tree = cKDTree(model.astype(F64))
    eye = np.eye(4, dtype=F32)
    models = [S.shard_model(model, scene_normals, tree, s, False, eye[:3], SCHEME, SIGMA) for s in shards]
    assert not any(S.check_shard(1, r, run.parts[0][r], models[r])[0] for r in range(2))
    scan_models = [S.shard_model(model, scene_normals, tree, rows, False, eye[:3], SCHEME, SIGMA)]
    fails, _ = S.check_additivity(1, run.totals[0], S.whole_vector(whole, rows, eye, False), scan_models, SCHEME)
    assert [c for c, _ in fails] == ["B count"]


def test_wrong_total_in_float32(engine_class, scene_normals):
    class Float32Total(S.SimulatedWorld):
        def total(self, parts):
            s = torch.zeros(S.NEQ, dtype=torch.float32)
            for p in parts:
                s += p.to(torch.float32)
            return s.to(torch.float64)
    shards = S.bounds_cut(S.cloud(1025), 4)
    got = _checks_of(lambda: _audit(engine_class, S.scene()[1], scene_normals, shards, world_class=Float32Total, iterations=2))
    assert "B additivity" in got and not got & {"A sums", "A row count", "C step", "C loss", "D ranks agree"}


def test_wrong_count_not_summed(engine_class, scene_normals):
    class CountOfRankZero(S.SimulatedWorld):
        def total(self, parts):
            s = super().total(parts)
            s[29] = parts[0][29]
            return s
    shards = S.bounds_cut(S.cloud(1025), 4)
    got = _checks_of(lambda: _audit(engine_class, S.scene()[1], scene_normals, shards, world_class=CountOfRankZero, iterations=2))
    assert "B count" in got and "A row count" not in got


def test_wrong_rank_solves_its_local_sums(engine_class, scene_normals):
    shards = S.bounds_cut(S.cloud(1025), 4)
    got = _checks_of(lambda: _audit(engine_class, S.scene()[1], scene_normals, shards, wrong={1: "solves_local_sums"},
                                    iterations=2))
    assert {"C step", "C loss", "D ranks agree"} <= got


def test_wrong_rank_accumulates_at_the_previous_pose(engine_class, scene_normals):
    shards = S.bounds_cut(S.cloud(1025), 4)
    got = _checks_of(lambda: _audit(engine_class, S.scene()[1], scene_normals, shards, wrong={3: "previous_pose"}, iterations=3))
    assert "A sums" in got and "A row count" not in got


def test_wrong_empty_shard_returns_stale_sums(engine_class, scene_normals):
    """An empty rank that writes nothing holds the total of the previous iteration (the world wrote it there)."""
    shards = S.cut(S.cloud(4096), S.ABI_CUTS["2048+0+2048"])
    got = _checks_of(lambda: _audit(engine_class, S.scene()[1], scene_normals, shards, wrong={1: "stale_empty_shard"},
                                    iterations=2))
    assert "A row count" in got or "A empty shard" in got
    part = np.zeros(S.NEQ)
    part[3] = -0.0
    empty = dict(n=0, flagged=0)
    assert [c for c, _ in S.check_shard(1, 0, part, empty)[0]] == ["A empty shard"]  # (exact zeros: not even -0.0)
    part[3], part[30] = 0.0, 1.0
    assert [c for c, _ in S.check_shard(1, 0, part, empty)[0]] == ["A pad"]


def test_wrong_stop_from_a_rank_local_step(engine_class, scene_normals):
    got = {c for c, _ in _stop_case(engine_class, scene_normals, wrong={2: "local_stop"})}
    assert "D ranks agree" in got and "stop" in got


def test_wrong_accumulation_behind_done(engine_class, scene_normals):
    """A rank that goes on accumulating and solving behind `done`: it solves the W-fold sums the driver leaves there."""
    got = {c for c, _ in _stop_case(engine_class, scene_normals, wrong={0: "runs_behind_done"})}
    assert "stop" in got
