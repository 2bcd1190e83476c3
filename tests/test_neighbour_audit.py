"""CPU: the table, the runner and the toy model of tests/neighbour_audit.py (contexts beside each other on one device).  The runner
passes over the toy, and each deliberately wrong copy of the toy is reported by the check meant for it and by no other; the GPU
file (tests/test_gpu_neighbour_audit.py) runs the library through the same runner."""
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import inflight_audit as A  # noqa: E402
import neighbour_audit as N  # noqa: E402


def test_the_table_records_the_uncounted_states_as_they_are():
    assert set(N.STATES) == {"held", "pending", "two_pending", "begun", "frame", "batch_hold", "pframe", "pmap_launched"}
    assert {s for s, spec in N.STATES.items() if spec.counted == 0} == {"pframe", "pmap_launched"}
    assert set(N.STATES) <= set(A.STATES)  # (the in-flight states of the inflight audit: `overlapped` has nothing in flight)
    assert N.STATES["batch_hold"].counted == 3 and all(N.STATES[s].counted == 1 for s in ("held", "pending", "two_pending", "begun", "frame"))
    # every job of a span runs in both finishing orders, the others once; a cell is skipped only with a reason
    assert len(N.CELLS) == len(N.STATES) * sum(2 if j.spans else 1 for j in N.JOBS.values())
    assert all(reason for reason in N.SKIPPED.values())
    assert set(N.MEANT) == set(N.FAULTS) and set(N.MEANT.values()) <= set(N.CHECKS)


def test_the_two_diagnostics_are_declared_rows_of_the_inflight_table():
    declared = A.declared_symbols()
    for name in ("icp_lead_registrations", "icp_registering_contexts"):
        assert name in declared and A.TABLE[name].cells["held"].kind == "N/A"


def test_every_cell_passes_over_the_toy():
    cache, tally = {}, [0, 0]
    failed = {c: f for c in N.CELLS for f in [N.run_cell(N.toy_world(), *c, cache=cache, tally=tally)] if f}
    assert failed == {}
    assert tally[0] > 0 and tally[1] > 0  # (both answers were given)
    print("toy:", len(N.CELLS), "cells,", tally[0], "registrations lead,", tally[1], "plain")


def test_the_toy_holds_chunks_back_where_the_cells_say_so():
    """What `latched` stands on: the held registrations of the toy run at least k1 + 3 iterations."""
    assert N.NEED["jump"] >= N.NEED["short"] + 3 and min(N.NEED["jump"], N.NEED["jump_b"], N.NEED["second"]) >= N.NEED["short"] + 3
    assert N.LIVE_MAX >= N.NEED["jump"]


def test_the_alternation_and_the_endings_pass_over_the_toy():
    assert N.run_alternation(N.toy_world()) == []
    assert {e: N.run_ending(N.toy_world(), e) for e in N.ENDINGS} == {e: [] for e in N.ENDINGS}


def _reports(fault):
    """{check: how often} over the matrix, the alternation and the endings of the toy with `fault`."""
    seen, cache = {}, {}
    runs = [N.run_cell(N.toy_world(fault), *c, cache=cache) for c in N.CELLS]
    runs.append(N.run_alternation(N.toy_world(fault)))
    runs += [N.run_ending(N.toy_world(fault), e) for e in N.ENDINGS]
    for fails in runs:
        for f in fails:
            seen[f] = seen.get(f, 0) + 1
    return seen


@pytest.mark.parametrize("fault", N.FAULTS)
def test_a_wrong_copy_is_reported_by_its_own_check_and_by_no_other(fault):
    seen = _reports(fault)
    assert set(seen) == {N.MEANT[fault]}, (fault, seen)


def test_the_oracle_context_has_the_two_accessors():
    from oracle_context import OracleContext
    ctx = OracleContext(height=8, width=16)
    assert ctx.lead_registrations() == 0 and ctx.registering_contexts() == 0
