"""The NN-cache certificate audit on the CPU (tests/cache_audit.py): what the new clouds are built to contain, the kd-tree
shortcut of the model against the brute force, the loop of the GPU tests clean on a context that answers from the model —
and each check failing the wrong copy meant for it."""
import numpy as np
import pytest

import cache_audit as CA
import knn_audit as K
import search_audit as S

F32 = np.float32
SHIFT = np.array([1.0e-4, -1.0e-4, 1.0e-4], F32)
MOVE = np.array([0.02, -0.01, 0.015], F32)       # far enough that entries run out of slack: rows on both sides of the test
IDENTITY = np.eye(4, dtype=F32)[:3]


@pytest.mark.parametrize("name", list(CA.NEW_CLOUDS))
def test_model_shortcut_flags_and_intent(name):
    """On the new clouds the model through the kd-tree's candidates is the brute-force model to the bit, at most FLAGGED_MAX of
    the rows are flagged, and every constructed row has the neighbour its construction means (W) by the model."""
    cloud = CA.cloud(name)
    _, got = CA.model_at(CA.map_model(name), cloud.queries, IDENTITY)
    ref = S.model_nn(cloud.map, cloud.queries)
    assert np.array_equal(got.index, ref.index) and np.array_equal(got.dist.view(np.uint32), ref.dist.view(np.uint32))
    assert np.array_equal(got.flagged, ref.flagged) and ref.flagged.sum() <= K.FLAGGED_MAX * cloud.queries.shape[0]
    assert cloud.queries.shape[0] - cloud.first_adv >= 36 and cloud.first_adv == S.SMALL_FILLER
    for row, index in cloud.expect.items():
        assert int(ref.index[row, 0]) == index and not ref.flagged[row], (name, row)


def test_model_shortcut_at_a_pose():
    """... and at a pose that is not the identity, on a cloud of exact ties"""
    cloud = CA.cloud("ties h=0.5 small")
    pose = CA.converging_poses(3, MOVE)[2]
    pose[0, 1], pose[1, 0] = F32(1.0e-3), F32(-1.0e-3)
    _, got = CA.model_at(CA.map_model(cloud.name), cloud.queries, pose)
    ref = S.model_nn(cloud.map, cloud.queries, pose)
    assert np.array_equal(got.index, ref.index) and np.array_equal(got.flagged, ref.flagged)


@pytest.mark.parametrize("h", (0.3, 0.7, 0.5))
def test_face_quads_are_what_they_claim(h):
    """Of the INPUT: W shares the query's cell, B lies in another cell, nearer than the gap to that cell as computed (not at the
    control h = 0.5, where no such point exists), d(B) - d(W) spans 1e-6 .. 1e-3 m and more, and on some rows the SLACKENED gap
    exceeds d(W): B's cell is pruned and only its gap speaks for B.  h = 0.3 has such face points at positive coordinates
    only (floorf is not symmetric: test_search_audit), h = 0.7 on both sides."""
    cloud = CA.cloud(f"face quads h={h}")
    what = CA.classify_quads(cloud)
    rows = list(what.values())
    assert all(r.w_own and r.b_other and not r.own_empty and r.gap > 0 for r in rows)
    if h == S.CONTROL_H:
        assert len(cloud.kinds["control"]) >= 36 and not any(r.below_gap for r in rows)
    else:
        assert all(r.below_gap for r in rows)
        assert len(cloud.kinds["face"]) >= 24 and len(cloud.kinds["edge"]) >= 6 and len(cloud.kinds["corner"]) >= 6
        q = cloud.queries[cloud.kinds["face"]]
        moved = np.abs(q - F32(S.LANE0)) > 1.0        # (the axis a face row runs along leaves the lane coordinate)
        assert moved.any(axis=0).all() and (q.max() > 1.0) and (h == 0.3 or q.min() < -1.0)
    gaps = np.array([r.gap for r in rows])
    assert gaps.min() < 3.0e-6 and gaps.max() > 3.0e-4 and sum(r.pruned for r in rows) >= 6, (gaps.min(), gaps.max())
    assert sum(r.pruned for r in rows) < len(rows)      # ... and rows whose B is SEEN: both ways into `second`


@pytest.mark.parametrize("h", (0.3, 0.7))
def test_lane_split_is_what_it_claims(h):
    cloud = CA.cloud(f"lane split h={h}")
    rows = list(CA.classify_quads(cloud).values())
    assert len(rows) >= 30 and all(r.own_empty and r.b_other and r.two_axes and r.gap > 0 for r in rows)
    own_empty, _, _ = S.classify(cloud.map, cloud.queries[cloud.kinds["split"]], h)
    assert own_empty.all()
    gaps = np.array([r.gap for r in rows])
    assert gaps.min() < 3.0e-6 and gaps.max() > 3.0e-3


def test_sets_of_three_are_what_they_claim():
    cloud = CA.cloud("sets of three h=0.3")
    mm = CA.map_model(cloud.name)
    for kind, cells in (("own", 1), ("across", 4)):
        rows = np.asarray(cloud.kinds[kind])
        d, idx = mm.candidates(cloud.queries[rows], 5)
        assert ((d[:, 2] - d[:, 0] >= 0.99e-4) & (d[:, 2] - d[:, 0] <= 1.01e-3)).all()
        assert ((d[:, 3] - d[:, 2] >= 0.99e-4) & (d[:, 3] - d[:, 2] <= 1.01e-3)).all() and (d[:, 4] - d[:, 3] > 0.05).all()
        own = S.cell_coord(cloud.queries[rows], cloud.h)
        for r in range(rows.size):
            other = {tuple(c) for c in S.cell_coord(cloud.map[idx[r, :4]], cloud.h).tolist()} - {tuple(own[r].tolist())}
            assert len(other) == (0 if cells == 1 else 4), (kind, r, other)


# ---- the loop of the GPU tests on a context that answers from the model ---------------------------------------------------
@pytest.mark.parametrize("name", list(CA.FINE_CLOUDS) + list(CA.REUSED))
def test_loop_runs_clean_on_the_model(name):
    """One iteration from the identity and six from the displaced scan, records on: A - D hold, nothing is vacuous, the flagged
    share stays under its cap (`audit` asserts all of it)."""
    cloud, mm = CA.cloud(name), CA.map_model(name)
    ctx = CA.FakeContext(cloud.map, [IDENTITY], mm=mm)
    _, rep = CA.run_and_audit(ctx, mm, cloud.queries, 1, f"{name}, identity")
    assert rep.rows + rep.flagged == cloud.queries.shape[0] and rep.positive > 0
    scan = np.ascontiguousarray(cloud.queries + SHIFT)
    ctx = CA.FakeContext(cloud.map, CA.converging_poses(6, SHIFT), records=True, mm=mm)
    _, rep = CA.run_and_audit(ctx, mm, scan, 6, f"{name}, six iterations", records=True)
    assert rep.aged > 0 and rep.record_rows > 0 and rep.min_slack > 0


def _moved_run(count, wrong=None, records=False, name="sets of three h=0.3"):
    cloud, mm = CA.cloud(name), CA.map_model(name)
    scan = np.ascontiguousarray(cloud.queries + MOVE)
    ctx = CA.FakeContext(cloud.map, CA.converging_poses(count, MOVE, 0.6), records=records, wrong=wrong, mm=mm)
    ctx.register(scan)
    return mm, scan, ctx.last_cache_entries(scan.shape[0], records)


@pytest.mark.parametrize("count", (8, 26, 30))
def test_long_moved_runs_are_clean_and_expire(count):
    """With a motion that uses entries up — rows on both sides of the test in every iteration — the restated cache passes, and
    past 24 iterations its oldest entry is exactly 24 old: the 25th launch behind a search misses."""
    mm, scan, out = _moved_run(count)
    rep = CA.audit(mm, scan, out, f"moved, {count} iterations")
    assert 0 < rep.aged < rep.rows and rep.max_age == min(count - 1, CA.CACHE_HIST)
    assert 0.0 < rep.kept_share[-1] < 1.0


# ---- each check fails the wrong copy meant for it ---------------------------------------------------------------------------
def _ring_rows(name, kinds):
    cloud = CA.cloud(name)
    return cloud, CA.map_model(name), np.concatenate([np.asarray(cloud.kinds[k], np.int64) for k in kinds])


def test_ring_entry_restates_the_search():
    """`ring_entry` without switches is search_audit.ring_search: the same neighbour, L = sqrtf(second) * 0.999999f"""
    for name, kinds in (("face quads h=0.3", ("face", "edge", "corner")), ("lane split h=0.7", ("split",))):
        cloud, _, rows = _ring_rows(name, kinds)
        grid = S.Grid(cloud.map, cloud.h)
        for r in rows[::3]:
            _, i, exact, second = S.ring_search(grid, cloud.queries[r], 2)
            for lanes in (1, 4):
                j, L = CA.ring_entry(grid, cloud.queries[r], lanes=lanes)
                assert exact and i == j and L == np.sqrt(second) * CA.C_DOWN, (name, r, lanes)


A_WRONG = [("face quads h=0.3", ("face", "edge", "corner"), "second_strict", 1), ("face quads h=0.7", ("face", "edge", "corner"), "second_strict", 1),
           ("face quads h=0.3", ("face", "edge", "corner"), "seen_only", 4), ("face quads h=0.7", ("face",), "seen_only", 1),
           ("lane split h=0.3", ("split",), "lose_lanes", 4), ("lane split h=0.7", ("split",), "lose_lanes", 4),
           ("lane split h=0.3", ("split",), "seed_unfolded", 1), ("lane split h=0.7", ("split",), "seed_unfolded", 1)]


@pytest.mark.parametrize("name,kinds,wrong,lanes", A_WRONG)
def test_check_a_fails_its_wrong_copies(name, kinds, wrong, lanes):
    """A bound from the gap as computed, a bound from the seen points alone, a reduce that forgets the losing lanes' bests, a
    seed that loses and is forgotten: the restated search passes check A on the rows built for it, each wrong copy does not.
    The seed is the runner-up B, handed over as the previous frame would."""
    cloud, mm, rows = _ring_rows(name, kinds)
    seeds = {}
    if wrong == "seed_unfolded":
        seeds = {"seed_of": {int(r): (K.model_d2(cloud.map[cloud.expect[int(r)] + 1][None], cloud.queries[r][None])[0][0, 0],
                                      cloud.expect[int(r)] + 1) for r in rows}}
    rep = CA.audit(mm, cloud.queries, CA.entries_of(cloud, rows, lanes=lanes, **seeds), f"{name}, restated")
    assert rep.rows == rows.size and rep.positive == rows.size
    with pytest.raises(AssertionError, match="check A: .* is not in the set of row"):
        CA.audit(mm, cloud.queries, CA.entries_of(cloud, rows, lanes=lanes, wrong=wrong, **seeds), f"{name}, {wrong}")


def test_age_rule_fails_its_wrong_copy():
    """`<=` for `<` at age 25: an entry survives its 25th launch"""
    mm, scan, out = _moved_run(30, "age_le")
    with pytest.raises(AssertionError, match="check age: .* entry of age 25 > 24"):
        CA.audit(mm, scan, out, "age 25 passes")


@pytest.mark.parametrize("count", (130, 160))
def test_iteration_field_wrap(count):
    """Past iteration 128 the stored field has wrapped.  Resolved against the running iteration the cache goes on as before;
    taken as it stands (the kernel before this audit) every entry written from iteration 128 on is 128 launches old at once —
    sound, and never a hit again: at 160 iterations no row has aged, which `audit` refuses as vacuous."""
    mm, scan, out = _moved_run(count)
    rep = CA.audit(mm, scan, out, f"moved, {count} iterations")
    assert rep.aged > 0.5 * rep.rows and rep.max_age <= CA.CACHE_HIST
    mm, scan, out = _moved_run(count, "field_plain")
    if count == 160:
        with pytest.raises(AssertionError, match="check vacuous: .* no audited row has aged"):
            CA.audit(mm, scan, out, "the field as it stands")
    else:
        plain = CA.audit(mm, scan, out, "the field as it stands")
        assert plain.aged < rep.aged


@pytest.mark.parametrize("wrong", ("slot_next", "no_delta"))
def test_check_c_fails_its_wrong_copies(wrong):
    """a displacement measured from the pose of j + 1, and none at all"""
    mm, scan, out = _moved_run(8, wrong)
    with pytest.raises(AssertionError, match="check C: .* kept at iteration . without the right to"):
        CA.audit(mm, scan, out, wrong)


def test_check_b_fails_its_wrong_copy():
    """a member replaced by the true runner-up: on sets of two and three the set's nearest is then another point at some pose"""
    mm, scan, out = _moved_run(8)
    CA.audit(mm, scan, out, "untouched")
    p, _ = CA.model_at(mm, scan, out["pose_hist"][-1])
    members = out["members"].astype(np.int64)
    _, runner = CA.nearest_outside(mm, p, members)
    rows = np.flatnonzero(out["iteration"] >= 0)[::7]
    wrong = dict(out, members=out["members"].copy())
    wrong["members"][rows, 0] = runner[rows]
    with pytest.raises(AssertionError, match="check B: .* the nearest member of row"):
        CA.audit(mm, scan, wrong, "runner-up for a member")


def test_check_d_fails_its_wrong_copy():
    """a record's bound taken from the points outside the set alone: the set's other members are nearer than it says"""
    mm, scan, out = _moved_run(8, None, True)
    rep = CA.audit(mm, scan, out, "records")
    assert rep.record_rows > 0
    mm, scan, out = _moved_run(8, "record_no_members", True)
    with pytest.raises(AssertionError, match="^check D: .* < the bound"):
        CA.audit(mm, scan, out, "record bound without the members")
