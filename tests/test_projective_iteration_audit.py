"""The projective iteration audit (tests/projective_iteration_audit.py) on the CPU: the accounting passes on the oracle's own
loop for every case of the device tests, no non-guard case is left with an undetermined step, every deliberately wrong copy of
a run is reported by the check meant for it, and the cases exercise what they are built for.

Measured here (the stand-in of the device: oracle statements, matrix-product sums, the step rounded to float32), worst per
family: shapes |ddx| 1.5e-9 / sums at 2.3e-2 of their bound; schemes 2.4e-9 / 1.9e-2; targets 4.4e-9 / 2.3e-2; windows 2.3e-8 /
3.5e-2 — against bars of 9.3e-10 .. 3.0e-8 (half a float32 ulp of the step + 4 x a model spread of at most 4.0e-15) for the
five IEEE schemes; exp / neighborhood / cauchy add |inv(H)| (|dg| + |dH| |dx|) TRANSCENDENTAL_BOUND, which STEP_ATOL cuts in
21 of their 84 iterations.  The equal-range pair won by the lowest index moves dx by 8.8e-8 — inside the 2e-7 the path was
held at before — and every sum by more than 1e6 times its bound."""
import numpy as np
import pytest

import projection_audit as PA
import projective_cases as PC
import projective_iteration_audit as P

F32 = np.float32
CASES = P.cases()


def _inputs(case):
    mv, mn = P.cached_cpu_window(case.window, case.h, case.w)
    init = case.init_pose()
    return mv, mn, P.make_targets(case.targets, case.h, case.w, mv, init), init


def _standin(case, wrong=None, threshold=0.0):
    mv, mn, targets, init = _inputs(case)
    return P.standin_records(mv, mn, targets, case.skip_null, init, case.K, case.scheme, case.sigma, threshold, wrong)


def _audit(case, records, threshold=0.0, worst=None):
    mv, mn, targets, init = _inputs(case)
    return P.audit_run(case.name, records, mv, mn, targets, case.skip_null, case.scheme, case.sigma, init, threshold,
                       case.guard, worst, quiet=True)


def test_shapes_sit_at_the_edges_of_the_summing_loop():
    """blocks = ceil(H W / 256) partial rows, S = ceil(blocks / 4) super-rows (sum_partials_vt, quad = 1)."""
    want = {(3, 3): (1, 1), (1, 300): (2, 1), (17, 33): (3, 1), (4, 256): (4, 1), (5, 256): (5, 2), (16, 2048): (128, 32),
            (128, 257): (129, 33), (64, 1024): (256, 64), (112, 2048): (896, 224), (112, 2049): (897, 225),
            (128, 2048): (1024, 256), (128, 2049): (1025, 257)}
    assert {s: P.blocks_of(*s) for s in P.SHAPES} == want
    assert 17 * 33 - 2 * 256 == 49


@pytest.mark.parametrize("family", sorted({c.family for c in CASES}))
def test_accounting_passes_on_the_oracles_loop(family):
    """Every case of the family within its bars; outside the guard cases no undetermined step (`audit_run` raises the
    "undetermined" check), no bar above STEP_ATOL, and the run makes its K iterations."""
    worst = P.Worst(family)
    for case in (c for c in CASES if c.family == family):
        records = _standin(case)
        models = _audit(case, records, worst=worst)
        if not case.guard:
            assert len(records) == case.K, case.name
            assert all(float(m["dx_bar"].max()) <= P.STEP_ATOL for m in models), case.name
            assert all(max(m["ref"]["spread"], m["ref"]["order_spread"]) <= 1.0e-12 for m in models), case.name
    print(worst)
    assert worst.n > 0 and worst.undetermined == []


def test_guard_cases_end_on_their_guards():
    by = {c.name: _standin(c) for c in CASES if c.guard}
    assert [r.status for r in by["shape 3x3"]] == [P.ICP_ERR_INVALID_JACOBIAN]
    for name in ("n=1 17x33", "n=5 17x33"):
        assert [r.status for r in by[name]] == [P.ICP_ERR_INVALID_JACOBIAN], name
    for name in ("n=0 17x33", "off image 17x33", "on model 17x33"):
        r = by[name]
        assert len(r) == 1 and r[0].status == P.ICP_OK and r[0].converged and not np.any(r[0].dx), name
    assert by["n=0 17x33"][0].num_targets == 0 and by["off image 17x33"][0].num_targets == 0
    assert by["on model 17x33"][0].num_targets >= 6 and by["on model 17x33"][0].neq[28] == 0.0


# (the wrong copy, the case it is shown on, the checks that may report it)
WRONG_ON = {
    "stale_zbuffer": ("shape 17x33", {"row count", "normal equations"}),
    "previous_pose": ("shape 17x33", {"row count", "normal equations"}),
    "farther_wins": ("contested 17x33", {"row count", "normal equations"}),
    "tie_lowest_index": ("ties 17x33", {"normal equations"}),
    "higher_layer": ("window twice 17x33", {"normal equations"}),
    "unset_not_skipped": ("window recycled near origin 17x33", {"row count"}),
    "skip_null_ignored": ("shape 17x33", {"row count", "normal equations"}),
    "last_block_dropped": ("shape 17x33", {"row count"}),
    "quarter_row_dropped": ("shape 5x256", {"row count"}),
    "float32_sums": ("shape 64x1024", {"normal equations"}),
    "wrong_huber_branch": ("shape 17x33", {"normal equations"}),
    "pose_advanced_on_guard": ("shape 3x3", {"pose chain"}),
}


@pytest.mark.parametrize("wrong", P.WRONG)
def test_wrong_copy_is_reported(wrong):
    name, allowed = WRONG_ON[wrong]
    case = P.case_by_name(name)
    _audit(case, _standin(case))  # (the right copy passes)
    with pytest.raises(P.AuditFailure) as e:
        _audit(case, _standin(case, wrong))
    got = set(e.value.checks)
    print(f"{wrong} on {name}: {sorted(got)}: {str(e.value)[:300]}")
    # (a run that has gone wrong once goes on from another pose: later iterations may fail the step check as well)
    assert got & allowed and got <= allowed | {"step", "pose chain"}, (wrong, got)
    first = e.value.failures[0]
    assert first[0] in allowed, first


def test_a_single_wrong_winner_or_layer_is_orders_beyond_the_bound():
    """One pixel with the other winner of an equal-range pair (iteration 1 of the tie case): the sums move by more than 1e6
    times their bound — what "a single pixel exceeds this bound by many orders of magnitude" rests on."""
    case = P.case_by_name("ties 17x33")
    mv, mn, targets, init = _inputs(case)
    rec = _standin(case, "tie_lowest_index")[0]
    model = P.model_iteration(mv, mn, targets, case.skip_null, rec.pose12, case.scheme, case.sigma)
    assert rec.num_targets == model["n"]
    ratio = np.abs(rec.neq[:29] - model["sums"][:29]) / model["sum_tol"][:29]
    assert ratio.max() > 1.0e6, ratio.max()
    # the case holds the tie: the two rows of each pair land in one pixel with equal range bits, and the model takes the higher
    moved = PC.transform_fma(targets, init)
    bit = PA.model(moved, case.h, case.w, PC.UP_FOV, PC.DOWN_FOV)
    assert not bit.flagged.any()
    n = len(targets)
    pairs = [(i, n - 16 - 4 + i) for i in range(4)]
    for lo, hi in pairs:
        assert bit.pixel[lo] == bit.pixel[hi] >= 0 and bit.r[lo].view(np.uint32) == bit.r[hi].view(np.uint32)
        assert not np.array_equal(targets[lo], targets[hi])
    won = set(model["target_rows"].tolist())
    assert sum(hi in won for _, hi in pairs) >= 1 and not any(lo in won for lo, _ in pairs)


def test_model_agrees_with_the_association_model():
    """model_rows against projective_cases.expected_association over projection_audit.model's z-buffer: the same rows, bit
    for bit (two formulations of the winner and of the layer)."""
    for name in ("shape 17x33", "contested 5x256", "window recycled 5x256", "window twice 17x33", "planted 17x33"):
        case = P.case_by_name(name)
        mv, mn, targets, init = _inputs(case)
        q, p, n, pix, rows_of, flagged = P.model_rows(mv, mn, targets, case.skip_null, init[:3])
        src = P.valid_source_rows(targets, case.skip_null)
        moved = PC.transform_fma(np.asarray(targets, F32)[src], init)
        bit = PA.model(moved, case.h, case.w, PC.UP_FOV, PC.DOWN_FOV)
        enb, enn, etg, epix, eidx = PC.expected_association(mv, mn, moved, bit.index)
        assert flagged == 0 and len(q) > 0
        assert np.array_equal(pix, epix) and np.array_equal(rows_of, src[eidx]), name
        for a, b in ((q, enb), (n, enn), (p, etg)):
            assert np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32)), name


def test_census_of_branches():
    """Per scheme at 17 x 33 and 64 x 1024 the rows of the run hold both Huber-style branches (|r| below and above sigma) and
    clamped rows (0 < |r| < 1e-4); the planted cases add r == 0 rows; contested pixels, unset layers and layer ties occur
    where the cases claim them."""
    for case in (c for c in CASES if c.family == "schemes" or c.name in ("shape 17x33", "shape 64x1024")):
        got = P.census(_audit(case, _standin(case)), case.sigma)
        print(case.name, got)
        assert got["quadratic"] > 0 and got["linear"] > 0 and got["clamped"] > 0, (case.name, got)
    for name in ("planted 17x33", "planted 5x256"):
        case = P.case_by_name(name)
        assert P.census(_audit(case, _standin(case)), case.sigma)["zero"] > 0
    # contested pixels: more valid rows than winners
    case = P.case_by_name("contested 17x33")
    mv, mn, targets, init = _inputs(case)
    src = P.valid_source_rows(targets, True)
    bit = PA.model(PC.transform_fma(targets[src], init), case.h, case.w, PC.UP_FOV, PC.DOWN_FOV)
    assert (bit.pixel >= 0).sum() > 1.2 * (bit.index >= 0).sum()
    # unset layers under occupied pixels; layers that tie
    mv, mn, _, _ = _inputs(P.case_by_name("window recycled 17x33"))
    is_set = np.abs(mv).max(axis=1) > 0
    assert (is_set.any(axis=0) & ~is_set.all(axis=0)).sum() > 10
    mv, mn, _, _ = _inputs(P.case_by_name("window twice 17x33"))
    assert mv.shape[0] == 2 and np.array_equal(mv[0], mv[1]) and not np.array_equal(mn[0], mn[1])
    # NaN rows, null rows
    for name, skip in (("nan 17x33", False), ("shape 17x33", True)):
        t = _inputs(P.case_by_name(name))[2]
        assert len(P.valid_source_rows(t, skip)) < len(t), name


@pytest.mark.parametrize("name", ["shape 17x33", "shape 64x1024"])
def test_live_threshold_stops_where_the_history_says(name):
    """Thresholds halfway, geometrically, between consecutive |dx_k| of the forced run: the run under each stops at the
    iteration the float32 norms name, converged, with the pose it held before that iteration, a bit-prefix of the forced run."""
    case = P.case_by_name(name)
    forced = _standin(case)
    stops = P.thresholds_between(forced)
    assert len(stops) >= 2, [P.norm32(r.dx) for r in forced]
    for threshold, stop_at in stops:
        live = _standin(case, threshold=threshold)
        assert len(live) == stop_at and live[-1].converged and live[-1].iterations == stop_at
        assert np.array_equal(live[-1].pose_after[:3], forced[stop_at - 1].pose12)
        for a, b in zip(live, forced):
            assert a.loss == b.loss and np.array_equal(a.dx, b.dx)
        _audit(case, live, threshold)
        # the accounting holds the stop decision: a run that went on regardless is reported
        with pytest.raises(P.AuditFailure) as e:
            _audit(case, forced[:stop_at], threshold)
        assert "status" in e.value.checks
