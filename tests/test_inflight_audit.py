"""CPU side of the audit of calls beside work in flight (tests/inflight_audit.py): the table covers the header, agrees with the
header's own contract paragraph, the fixtures guarantee a hold-back before a GPU is involved, the scenario runner passes on the
toy state machine for every cell — and reports each deliberately wrong copy of that machine by the check meant for it."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, os.path.join(ROOT, "pylidar-slam_amd"), os.path.join(ROOT, "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import inflight_audit as A  # noqa: E402


# ---- completeness ------------------------------------------------------------------------------------------------------------
def test_the_table_has_one_row_per_declared_symbol_and_a_class_for_every_state():
    declared = A.declared_symbols()
    assert len(declared) >= 115
    assert sorted(A.TABLE) == declared, (sorted(set(declared) - set(A.TABLE)), sorted(set(A.TABLE) - set(declared)))
    for symbol, row in A.TABLE.items():
        assert tuple(row.cells) == A.STATES, symbol
        for state, cell in row.cells.items():
            assert cell.kind in A.KINDS, (symbol, state)
            if cell.kind == "INDEPENDENT":
                assert len(cell.text) > 10, f"{symbol} / {state}: the reason names the buffers"
            if cell.kind == "REFUSED":  # (the reason itself: the name of the function in front of it says nothing)
                assert len(cell.text.split(": ")[-1]) >= 10, f"{symbol} / {state}: a refusal names its reason"
        assert row.control is True or (isinstance(row.control, str) and row.control), symbol


def test_the_header_and_the_table_name_the_same_ordered_and_refused_calls():
    """The contract paragraph at icp_register_launch lists the single-context entry points that enqueue held-back iterations
    first, and those that are refused: exactly the ORDERED / REFUSED rows of the `held` state."""
    lists = A.header_lists()
    single = [s for s in A.TABLE if not s.startswith("icp_batch_")]
    for kind in ("ORDERED", "REFUSED"):
        table = sorted(s for s in single if A.TABLE[s].cells["held"].kind == kind)
        assert lists[kind], f"the header's {kind} list was not found"
        assert lists[kind] == table, (kind, sorted(set(lists[kind]) ^ set(table)))
    collects = sorted(s for s in single if A.TABLE[s].cells["held"].kind == "COLLECTS")
    assert collects == ["icp_register_end"]
    # the frame paragraph: what is refused between the two frame calls although it is ordered (or collects) beside a registration
    raw = open(A.HEADER).read()
    frame_only = sorted(s for s in single if A.TABLE[s].cells["frame"] == A.REFUSED(A.FRM) and A.TABLE[s].cells["held"].kind != "REFUSED")
    assert frame_only == ["icp_map_stage_cloud", "icp_map_update_staged", "icp_pmap_init", "icp_pmap_update", "icp_register_end"]
    paragraph = raw[raw.index("CALLS BETWEEN icp_frame_launch AND icp_frame_end"):]
    paragraph = paragraph[:paragraph.index("One frame at a time per context")]
    for s in frame_only:
        assert s in paragraph, s


def test_census_of_the_table():
    census = {k: 0 for k in A.KINDS}
    for row in A.TABLE.values():
        for cell in row.cells.values():
            census[cell.kind] += 1
    assert sum(census.values()) == len(A.TABLE) * len(A.STATES)
    print("cells:", census)


# ---- fixtures ----------------------------------------------------------------------------------------------------------------
def test_the_fixtures_hold_iterations_back():
    """The `held` precondition on the audit's inputs, by the float64-accumulating oracle: the short frame stops after k1
    iterations, the jump needs at least k1 + 3 — a first chunk of k1 + 1 (csrc/register_plan.h) leaves iterations held back."""
    import icp_oracle as O
    F = A
    fx = F.kd_fixture()
    counts = {}
    for name in ("short", "jump"):
        oc = O.ICPOracleConfig(max_num_alignments=F.MAX_ITERATIONS, threshold_delta_pose=F.THRESHOLD, scheme=F.SCHEME, sigma=F.SIGMA,
                               height=F.HEIGHT, width=F.WIDTH)
        o = O.ICPFrameToModelOracle(oc)
        o.local_map.set_map_pointcloud(fx["map"])
        o.register_new_frame(fx[name], np.eye(4, dtype=np.float32))
        counts[name] = len(o.traces[-1].dx)
    print("oracle iterations:", counts)
    assert counts["short"] == F.K1_ORACLE
    assert counts["jump"] >= counts["short"] + 3 and counts["jump"] < F.MAX_ITERATIONS
    # one iteration of slack either way for the float32 device: still a hold-back of at least one chunk
    assert counts["jump"] - 1 >= (counts["short"] + 1) + 3


# ---- the runner on the toy ---------------------------------------------------------------------------------------------------
def _variants(state):
    return ("key", "nonkey") if state in ("frame", "pframe") else (None,)


@pytest.mark.parametrize("state", A.STATES)
def test_the_runner_passes_on_the_toy_for_every_cell(state):
    cache = {}
    ran = 0
    for symbol, row in sorted(A.TABLE.items()):
        for variant in _variants(state):
            fails = A.run_cell(A.toy_factory(), state, symbol, row.cells[state], row.control, variant, cache)
            assert fails == [], (symbol, state, variant, fails)
            ran += row.cells[state].kind != "N/A"
    assert ran > 80


def test_the_toy_holds_iterations_back_in_the_held_state():
    rig = A.ToyRig(1, "held")
    rig.prepare()
    rig.enter()
    reg = rig.ctx.pending[-1]
    assert reg["enq"] == A.NEED["short"] + 1 < A.NEED["jump"]  # the first chunk: iterations of the last registration + 1
    rig.finish()
    assert rig.results[1].iterations == A.NEED["jump"] >= rig.results[0].iterations + 3


# (fault, state, variant, symbol, the cell the runner is given — None: the table's — and the check that must report it)
WRONG_COPIES = [
    ("no_flush", "held", None, "icp_map_set", None, "registration"),
    ("no_flush", "held", None, "icp_set_cost", None, "registration"),
    ("one_chunk", "held", None, "icp_map_update", None, "registration"),
    ("flush_after", "held", None, "icp_set_alignment", None, "registration"),
    ("flush_after", "frame", "key", "icp_map_normals_install", None, "registration"),
    ("refusal_mutates", "frame", "key", "icp_map_stage_cloud", None, "refusal-changed-nothing"),
    ("refusal_in_registration", "held", None, "icp_knn_query", None, "context-after-refusal"),
    ("refusal_in_registration", "pending", None, "icp_align_point_to_plane", None, "context-after-refusal"),
    ("register_end_takes_frame", "frame", "key", "icp_register_end", None, "refusal-status"),
    ("stage_replaces_frame_rows", "frame", "key", "icp_map_stage_cloud", None, "refusal-status"),
    ("update_staged_consumes", "frame", "key", "icp_map_update_staged", None, "refusal-status"),
    # ... and what the runner says had the table called the old behaviour harmless
    ("register_end_takes_frame", "frame", "key", "icp_register_end", A.INDEPENDENT("as if it were harmless"), "frame-end"),
    ("stage_replaces_frame_rows", "frame", "key", "icp_map_stage_cloud", A.INDEPENDENT("as if it were harmless"), "map"),
    ("update_staged_consumes", "frame", "key", "icp_map_update_staged", A.INDEPENDENT("as if it were harmless"), "frame-end"),
    ("independent_rewrites_targets", "held", None, "icp_pmap_nearest_neighbor_search", None, "registration"),
    ("independent_rewrites_targets", "held", None, "icp_compute_neighbors", None, "registration"),
    ("newest_first", "two_pending", None, "icp_register_end", None, "collect-order"),
    ("newest_first", "two_pending", None, "icp_set_option", None, "collect-order"),
]


@pytest.mark.parametrize("fault,state,variant,symbol,cell,check", WRONG_COPIES,
                         ids=[f"{w[0]}-{w[1]}-{w[3]}-{'table' if w[4] is None else 'as-independent'}" for w in WRONG_COPIES])
def test_each_wrong_copy_is_reported_by_its_check_and_by_no_other(fault, state, variant, symbol, cell, check):
    assert fault in A.FAULTS and check in A.CHECKS
    row = A.TABLE[symbol]
    given = cell or row.cells[state]
    fails = A.run_cell(A.toy_factory(fault), state, symbol, given, row.control, variant)
    assert fails == [check], (fault, symbol, state, fails)
    # the same cell on the sound toy passes (with the table's own class)
    assert A.run_cell(A.toy_factory(), state, symbol, row.cells[state], row.control, variant) == []


def test_every_fault_of_the_toy_has_a_wrong_copy():
    assert sorted({w[0] for w in WRONG_COPIES}) == sorted(A.FAULTS)


def test_a_control_without_teeth_is_reported():
    """A row that claims a control (the call made before the launch changes the registration) is held to it: a call whose
    effect no iteration reads fails the cell."""
    row = A.TABLE["icp_set_stream"]
    assert A.run_cell(A.toy_factory(), "held", "icp_set_stream", row.cells["held"], True) == ["control"]
    assert A.run_cell(A.toy_factory(), "held", "icp_map_set", A.TABLE["icp_map_set"].cells["held"], True) == []


def test_a_fixture_without_a_hold_back_is_reported(monkeypatch):
    monkeypatch.setitem(A.NEED, "jump", A.NEED["short"] + 2)
    assert A.run_cell(A.toy_factory(), "held", "icp_map_set", A.ORDERED, True) == ["precondition-held"]
