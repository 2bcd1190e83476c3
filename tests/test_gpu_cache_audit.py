"""The NN cache's certificates read back and held to the map (tests/cache_audit.py; `icp_last_cache_entries`).

From its second iteration on a registration answers most queries from the cache without searching, on the strength of a
bound L nothing else in the suite ever sees: `last_neighbors` reports the winner only, and a bound that is a little too
large shows only if a later pose carries a query toward the one point the bound forgot.  Here every entry — candidate set,
L, iteration of the search — is read out with the pose history and checked against the whole map in float64: A the bound is
sound at the pose it was formed at (no tolerance), B the set's nearest member is the model's neighbour at every pose the
entry served, C every iteration that kept the entry was entitled to by the hit test restated, with the age rule, D the hit
records.  Clouds that put the runner-up where the bound has to come from a pruned cell's gap, a losing lane's best or a
set of three; the first iteration under the 20 observable option sets; six iterations under the cache option sets, the
lazy-normals build and the records; runs of 26 .. 160 iterations through the 24-pose window and the 7-bit iteration field;
one `IcpBatch`; the three-frame chain with its frame seeds.

tests/test_cache_audit.py shows on the CPU that each check fails the wrong copy meant for it.
"""
import numpy as np
import pytest

import cache_audit as CA
import search_audit as S
import test_gpu_search_audit as G

pytestmark = pytest.mark.gpu
F32 = np.float32
SHIFT = G.SHIFT
IDENTITY = np.eye(4, dtype=F32)[:3]

FIRST_OPTION_SETS = {k: v for k, v in G.OPTION_SETS.items() if k not in G.UNOBSERVABLE}
ITER_OPTION_SETS = dict(G.CACHE_OPTION_SETS, lazy_normals={"eager_normals_limit": 0, "lazy_fused": 2},
                        hit_records={"hit_records": 1}, late_from_1={"hit_records": 1, "late_from": 1})
LONG_OPTION_SETS = {"defaults": {}, "tail_from_1": {"resident_tail": 1, "wide_until": 0}}
LONG_RUNS = (26, 50, 130, 160)
assert len(FIRST_OPTION_SETS) == 20


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (no CPU fallback exists for the product path)")
    return torch


def _records(opts):
    return bool(opts.get("hit_records"))


@pytest.mark.parametrize("name", list(CA.FINE_CLOUDS) + list(CA.REUSED))
def test_first_iteration(torch_cuda, name):
    """One iteration from the identity (the transform is exact: the clouds stay sharp) under the 20 observable option sets:
    every entry a search leaves — ball lanes 1 / 2 / 8, ball_max, ball_empty, far lanes, the wave search, narrow and wide, flat
    rows, the record builds, the late kernel — passes A and B.  The coarse, far and exhaustive rows: L == 0 or sound."""
    cloud, mm = CA.cloud(name), CA.map_model(name)
    fine = name in CA.FINE_CLOUDS
    worst = np.inf
    for label, opts in FIRST_OPTION_SETS.items():
        ctx = G._context(cloud, 2, 1, opts)
        _, rep = CA.run_and_audit(ctx, mm, cloud.queries, 1, f"{name}, {label}", _records(opts), fine)
        assert rep.rows + rep.flagged == cloud.queries.shape[0], (name, label)
        worst = min(worst, rep.min_slack)
    own = np.asarray(sorted(r for rows in cloud.kinds.values() for r in rows))
    print(f"{name}: {own.size} constructed rows of {cloud.queries.shape[0]}, smallest slack of A over all sets {worst:.3g}")


@pytest.mark.parametrize("name", CA.ITERATED + ("faces h=0.3 small", "faces h=0.7 small"))
def test_across_iterations(torch_cuda, name):
    """Six iterations at threshold 0 from the scan displaced by SHIFT: A - D from ONE read-out, at every pose of the history.
    The four cache option sets (the resident tail among them), the lazy-normals instantiation, the records and the late kernel."""
    cloud, mm = CA.cloud(name), CA.map_model(name)
    scan = np.ascontiguousarray(cloud.queries + SHIFT)
    for label, opts in ITER_OPTION_SETS.items():
        ctx = G._context(cloud, 2, 6, opts)
        _, rep = CA.run_and_audit(ctx, mm, scan, 6, f"{name}, {label}", _records(opts))
        assert rep.positive > 0 and rep.aged > 0, (name, label)


@pytest.mark.parametrize("label", list(LONG_OPTION_SETS))
def test_long_runs(torch_cuda, label):
    """26, 50, 130 and 160 iterations at threshold 0: past the 24 poses the workgroups keep (slot = iteration % 24, which the
    resident tail overwrites trip by trip) and past the 7 bits of the stored iteration.  A - C with the age rule: no entry is
    older than 24 although the loop is — the 25th launch behind a search searches again.  Losses and steps of every run are a
    prefix of the longest run's to the bit."""
    name = "face quads h=0.3"
    cloud, mm = CA.cloud(name), CA.map_model(name)
    scan = np.ascontiguousarray(cloud.queries + SHIFT)
    runs = []
    for k in LONG_RUNS:
        ctx = G._context(cloud, 2, k, LONG_OPTION_SETS[label])
        res, rep = CA.run_and_audit(ctx, mm, scan, k, f"{name}, {label}, {k} iterations")
        assert rep.positive > 0 and rep.aged > 0 and rep.max_age <= CA.CACHE_HIST
        runs.append(res)
    for k, res in zip(LONG_RUNS, runs):
        assert np.array_equal(res.losses, runs[-1].losses[:k]) and np.array_equal(res.dx, runs[-1].dx[:k]), \
            f"{label}: the run of {k} iterations is no prefix of the run of {LONG_RUNS[-1]}"


@pytest.mark.parametrize("k", (6, 27))
def test_batched(torch_cuda, k):
    """One `IcpBatch` of three contexts with three clouds and cell sizes (k_iterate_batch carries a copy of the hit test of its
    own): A - C per member."""
    from pylidar_slam_amd.engine import IcpBatch
    names = ("face quads h=0.3", "lane split h=0.7", "ties h=0.5 small")
    clouds = [CA.cloud(n) for n in names]
    scans = [np.ascontiguousarray(c.queries + SHIFT) for c in clouds]
    ctxs = [G._context(c, 2, k) for c in clouds]
    batch = IcpBatch(ctxs)
    batch.register_launch(scans)
    results = iter(batch.register_end())
    for name, ctx, scan in zip(names, ctxs, scans):
        _, rep = CA.run_and_audit(ctx, CA.map_model(name), scan, k, f"batch of {k}, {name}", register=lambda _: next(results),
                                   close=False)
        assert rep.positive > 0 and rep.aged > 0
    batch.close()
    for ctx in ctxs:
        ctx.close()


def test_frame_seeds(torch_cuda):
    """The three-frame chain of test_gpu_search_audit: register_launch / map_update(None, None) / register_end, init "last".
    The first iteration of frames 1 and 2 starts every search from a frame seed (k_cache_to_seed): a seed that loses must reach
    the bound.  A - C against `map_points()` as each frame saw them."""
    cloud = S.small("faces h=0.3 small")
    for f in range(3):
        ctx = G._context(cloud, 2, 4)
        for g in range(f):
            ctx.register_launch(np.ascontiguousarray(cloud.queries + SHIFT * F32(g + 1)), "last" if g else None, skip_null=False)
            ctx.map_update(None, None)
            ctx.register_end()
        scan = np.ascontiguousarray(cloud.queries + SHIFT * F32(f + 1))
        mm = CA.MapModel(ctx.map_points())

        def register(c):
            c.register_launch(scan, "last" if f else None, skip_null=False)
            return c.register_end()

        _, rep = CA.run_and_audit(ctx, mm, scan, 4, f"chain, frame {f}", register=register)
        assert rep.positive > 0 and rep.aged > 0


def test_refusals(torch_cuda):
    """The read-out refuses where `last_neighbors` does, in words of its own, and the records where none are kept."""
    cloud = CA.cloud("lane split h=0.3")
    n = cloud.queries.shape[0]
    ctx = G._context(cloud, 2, 2)
    with pytest.raises(AssertionError, match="icp_last_cache_entries: no fused registration"):
        ctx.last_cache_entries(n)
    ctx.register(cloud.queries, None, False)
    out = ctx.last_cache_entries(n)
    assert out["last"] == 1 and out["members"].shape == (n, 3) and np.array_equal(out["pose_hist"][0], IDENTITY)
    with pytest.raises(AssertionError, match="icp_last_cache_entries: no hit records"):
        ctx.last_cache_entries(n, records=True)
    ctx.map_set(cloud.map)                       # the map changed: the entries describe another grid
    with pytest.raises(AssertionError, match="icp_last_cache_entries: no fused registration"):
        ctx.last_cache_entries(n)
    ctx.close()
    ctx = G._context(cloud, 2, 2, {"fuse_iteration": 0})
    ctx.register(cloud.queries, None, False)
    with pytest.raises(AssertionError, match="icp_last_cache_entries: no fused registration"):
        ctx.last_cache_entries(n)
    ctx.close()
