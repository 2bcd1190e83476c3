"""Calls beside work in flight: the table of what every entry point of include/icp_mi355x.h does when its context still has a
registration or a frame on the stream, the scenario runner that holds an implementation to a cell of that table, and a toy
model of the host-side state machine (csrc/register.hip, frame.hip, api.hip) the runner is tried on.  TEST INFRASTRUCTURE:
standard library only, importable without a GPU, never imported by the package.  tests/test_inflight_audit.py holds the table
and the runner on the CPU, tests/test_gpu_inflight_audit.py runs the library through the same runner.

THE STATES (a fixed prologue on a fresh context each):
  held           icp_register_launch with a live stop threshold and "chunked_launch" 1: the last collected registration ran k1
                 iterations, this one needs at least k1 + 3, so k1 + 1 are on the stream and the rest is HELD BACK
  pending        the same with a forced iteration count: everything enqueued, nothing collected
  two_pending    icp_register_launch + icp_register_launch_from_last, neither collected
  begun          between icp_register_begin and icp_register_end (in_registration)
  frame          between icp_frame_launch and icp_frame_end of a later, staged frame (a key frame and one that is not)
  pframe         the same for icp_pmap_frame_launch
  pmap_launched  behind icp_pmap_register_launch
  batch_hold     a member of an icp_batch whose chunked batched registration holds iterations back
  overlapped     a staged or pose-only map update running on the context's map stream ("overlap_map_update" 1)

THE CLASSES, every one derived by reading the entry point (the GPU run confirms; it discovers nothing):
  ORDERED        iterations held back are enqueued first (ICP_HELD_FIRST / continue_launch(ctx, -1)), then the call takes
                 effect: the registration equals its twin, the call's effect lies behind it
  REFUSED(text)  ICP_ERR_INVALID_ARGUMENT, icp_last_error holds `text`, nothing changed, the context goes on like its twin
  INDEPENDENT(r) the call touches nothing the work in flight reads or writes; r names the buffers
  COLLECTS       the call that ends the state
  N/A            constructors, destructors, defaults, pure accessors of host fields

WHAT THE READING FOUND (the place of each fix is in the row's note):
  * icp_register_end / icp_map_stage_cloud / icp_map_update_staged between the two frame calls took the frame's result,
    replaced its staged rows, consumed them: now REFUSED ("a frame is launched and awaits its end").
  * icp_pmap_init / icp_pmap_update between the two frame calls emptied or moved the window the frame's end appends to: REFUSED.
  * icp_pmap_register with a result pending handed that OLDER result out as its own and left the context "in registration":
    REFUSED now (the header used to list it among the calls that enqueue held-back iterations first).
  * icp_set_normal_equations_buffer let held-back iterations sum into the NEW vector: ICP_HELD_FIRST now.
  * icp_exchange_connect switched the exchange on under enqueued or held-back iterations: REFUSED like icp_exchange_create.
  * icp_set_alignment and the map calls between icp_register_begin and icp_register_end re-allocated the state or rebuilt the
    grid under the caller's next icp_iteration_accumulate: REFUSED like icp_set_option.
  * icp_iteration_accumulate / _solve / icp_register_end with nothing to act on returned the bare status: they name it now.
  * the batched forms asked nothing of a member whose OWN frame is launched or which is between icp_register_begin and
    icp_register_end: icp_batch_register_end collected the member's frame registration (the frame could never end),
    icp_batch_stage replaced and icp_batch_map_update_staged consumed its staged rows, icp_batch_map_update moved its map, and
    an icp_batch_register_launch that failed on the begun member ABANDONED the caller's registration (batch_abandon).  All
    REFUSED now, before any member changes (batch.hip: batch_members_free).
  * REFUTED: icp_pmap_nearest_neighbor_search, icp_compute_neighbors and the alignment seams write ctx->targets — which only the
    packing launch reads, and that launch is on the stream before icp_register_launch returns (first_pack_flush); the
    iterations read tgt4.  icp_compact_targets uses scan_tmp and counter, which no iteration reads.  icp_last_neighbors and
    icp_last_cache_entries do check (in_registration || result_pending()).  icp_map_get reads map_xyz, which no iteration writes.
"""
import os
import re
from collections import namedtuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "icp_mi355x.h")

STATES = ("held", "pending", "two_pending", "begun", "frame", "pframe", "pmap_launched", "batch_hold", "overlapped")
ICP_ERR_INVALID_ARGUMENT = -1


def declared_symbols():
    """The entry points include/icp_mi355x.h declares (as tests/test_cabi.py::_declared_symbols)."""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(icp_[a-z_0-9]+)\s*\(", text)))


def header_lists():
    """The lists of the contract paragraph at icp_register_launch: {"ORDERED": [...], "REFUSED": [...]}.  The paragraph writes
    them as `ORDERED (enqueues them first): a, b, c.` and `REFUSED (...): a, b.`; `icp_x_a / _b` stands for icp_x_a, icp_x_b."""
    raw = open(HEADER).read()
    out = {}
    for key, pattern in (("ORDERED", r"ORDERED \(enqueues them first\):(.*?)\.\n"), ("REFUSED", r"REFUSED \(while[^)]*\):(.*?)\.\n")):
        m = re.search(pattern, raw, flags=re.S)
        if not m:
            out[key] = []
            continue
        names = []
        for tok in re.findall(r"icp_[a-z_0-9]+(?:\s*/\s*_[a-z_0-9]+)*", m.group(1)):
            parts = [p.strip() for p in tok.split("/")]
            names.append(parts[0])
            for suffix in parts[1:]:
                names.append(parts[0][:parts[0].rfind("_")] + suffix)
        out[key] = sorted(set(names))
    return out


# ---- the classes -------------------------------------------------------------------------------------------------------------
Cell = namedtuple("Cell", "kind text")
ORDERED = Cell("ORDERED", "")
COLLECTS = Cell("COLLECTS", "")
NA = Cell("N/A", "")


def REFUSED(fragment):
    return Cell("REFUSED", fragment)


def INDEPENDENT(reason):
    return Cell("INDEPENDENT", reason)


KINDS = ("ORDERED", "REFUSED", "INDEPENDENT", "COLLECTS", "N/A")

# control: True — applied BEFORE the launch the call changes the registration (the runner demands it);
#          a string — why no control exists
Row = namedtuple("Row", "symbol cells control note")

RIP = "registration in progress"
FRM = "a frame is launched and awaits its end"
BH = "still holds iterations back"
PEND = "collect the pending result first"
AWAIT = "awaits icp_register_end"
TWO = "two results are already pending"
NOREG = "no registration in progress"
TUNING = "a tuning option never changes a result"
NOTEETH = "the call changes nothing a registration reads"

TABLE = {}


def _row(symbol, held, pending, two_pending, begun, frame, pframe, pmap_launched, batch_hold, overlapped, control=NOTEETH, note=""):
    assert symbol not in TABLE, symbol
    cells = dict(zip(STATES, (held, pending, two_pending, begun, frame, pframe, pmap_launched, batch_hold, overlapped)))
    TABLE[symbol] = Row(symbol, cells, control, note)


def _all(symbol, cell, control=NOTEETH, note="", **override):
    cells = {s: cell for s in STATES}
    cells.update(override)
    _row(symbol, *[cells[s] for s in STATES], control=control, note=note)


# ---- N/A: constructors, destructors, defaults, accessors of host fields
for _s in ("icp_default_config", "icp_create", "icp_destroy", "icp_last_error", "icp_version", "icp_default_frame_config",
           "icp_default_pmap_frame_config", "icp_default_refine_params", "icp_map_size", "icp_map_num_clouds",
           "icp_handoff_fallbacks", "icp_first_build_launches", "icp_lead_registrations", "icp_registering_contexts", "icp_pmap_num_maps", "icp_normal_equations_ptr",
           "icp_batch_create", "icp_batch_destroy", "icp_batch_last_error", "icp_aggmap_create", "icp_aggmap_destroy",
           "icp_elevation_create", "icp_elevation_destroy", "icp_refine_create", "icp_refine_destroy"):
    _all(_s, NA)

# ---- scratch only: api.hip stages through stage_in / stage_out / stage_out2 / vox_out, the samplers through scan_a / scan_b /
# keys_* / vals_* / sort_tmp / counter, the projection through zbuf.  search.hip and gauss_newton.hip (the iterations) name none
# of them: a kd-tree iteration reads tgt4, the grid, the normals, the NN cache, the state, partials and the mailbox.  The
# projective iterations do use zbuf (projective.hip: pmap_iterate) — every one of them is on the stream when
# icp_pmap_register_launch returns, so a later projection follows them in stream order.
_SCRATCH = INDEPENDENT("stage_in / stage_out / stage_out2 / zbuf / scan_* / keys_* / counter: no iteration reads them; "
                       "projective iterations (zbuf) are all enqueued, stream order")
for _s in ("icp_project", "icp_project_rows", "icp_project_pixels", "icp_kitti_correct_scan", "icp_voxel_hash",
           "icp_grid_sample", "icp_grid_sample_f64", "icp_voxel_statistics", "icp_distort"):
    _all(_s, _SCRATCH)
for _s in ("icp_grid_sample_padded", "icp_grid_sample_padded_f64"):
    _all(_s, _SCRATCH, begun=REFUSED(RIP))
_all("icp_compact_targets", INDEPENDENT("scan_tmp and counter (compact_valid_rows) and the caller's output: no iteration reads them"))
_all("icp_synchronize", INDEPENDENT("waits for the stream (joined with the map stream); writes nothing"))
_all("icp_profile_enable", INDEPENDENT("host fields of the profile; held-back launches are then bracketed by events, same bits"),
     control=TUNING)
for _s in ("icp_profile_read", "icp_profile_read_iterations"):
    _all(_s, INDEPENDENT("synchronises the stream and reads the profile's host totals"))
_all("icp_profile_event_floor", INDEPENDENT("spin kernels without memory arguments, two events of its own"))
_MAPREAD = INDEPENDENT("copies map_xyz[map_cur] / pm_mv, pm_mn to the caller: iterations never write them")
_all("icp_map_get", _MAPREAD, overlapped=ORDERED, note="issue item 5: refuted, correct by stream order")
_all("icp_pmap_get_model", _MAPREAD, overlapped=ORDERED)
_PM = INDEPENDENT("stage_in / stage_out / pm_tmp / flags / counter and ctx->targets, which only the packing launch reads — "
                  "on the stream before a launch returns (first_pack_flush); iterations read tgt4")
_all("icp_compute_normal_map", _PM, overlapped=ORDERED, note="issue item 5: refuted")
_all("icp_compute_neighbors", _PM, overlapped=ORDERED, note="issue item 5: refuted (writes ctx->targets, read by the packing launch alone)")
_all("icp_pmap_nearest_neighbor_search", _PM, overlapped=ORDERED, note="issue item 4: refuted (ctx->targets is read by the packing launch alone)")
_PMW = INDEPENDENT("the projective window (pm_slots, pm_poses, pm_v / pm_n / pm_mv / pm_mn): kd-tree iterations read none of it")
_all("icp_pmap_init", _PMW, frame=REFUSED(FRM), pframe=REFUSED(FRM), pmap_launched=ORDERED, overlapped=ORDERED,
     note="fixed (api.hip icp_pmap_init): emptied the window icp_pmap_frame_end re-expresses")
_all("icp_pmap_update", _PMW, frame=REFUSED(FRM), pframe=REFUSED(FRM), pmap_launched=ORDERED, overlapped=ORDERED,
     note="fixed (api.hip icp_pmap_update): moved the window under a launched frame")
_OWN = "buffers, table and pinned rows of the object itself (aggmap.hip / elevation.hip / refine.hip), none of the context's"
for _s in ("icp_aggmap_insert", "icp_aggmap_stats", "icp_aggmap_get", "icp_aggmap_get_f64", "icp_aggmap_submap", "icp_aggmap_clear",
           "icp_elevation_build", "icp_elevation_build_aggmap", "icp_elevation_get", "icp_elevation_stats", "icp_refine_set_target",
           "icp_refine_launch", "icp_refine_end", "icp_refine_image_rows", "icp_refine_history"):
    _all(_s, INDEPENDENT(_OWN))

# ---- ICP_HELD_FIRST, then the change
_all("icp_set_stream", ORDERED, batch_hold=REFUSED(BH), control="a stream changes no result")
_all("icp_set_option", ORDERED, begun=REFUSED(RIP), batch_hold=REFUSED(BH), control=TUNING)
_all("icp_set_cost", ORDERED, begun=REFUSED(RIP), batch_hold=REFUSED(BH), control=True)
_all("icp_set_alignment", ORDERED, begun=REFUSED(RIP), batch_hold=REFUSED(BH), control=True,
     note="fixed (api.hip): refused between icp_register_begin and icp_register_end (ensure_state re-allocated the state)")
_all("icp_set_normal_equations_buffer", ORDERED, batch_hold=REFUSED(BH), control="every iteration overwrites the vector: same bits",
     note="fixed (api.hip): ICP_HELD_FIRST — held-back iterations summed into the new vector")
_MAPFIX = "fixed (api.hip): refused between icp_register_begin and icp_register_end"
_all("icp_map_init", ORDERED, begun=REFUSED(RIP), batch_hold=REFUSED(BH), control="an empty map refuses the launch", note=_MAPFIX)
_all("icp_map_set", ORDERED, begun=REFUSED(RIP), batch_hold=REFUSED(BH), control=True, note=_MAPFIX)
_all("icp_map_update", ORDERED, begun=REFUSED(RIP), batch_hold=REFUSED(BH), control=True,
     note=_MAPFIX + "; rel_pose = NULL with a cloud is refused while a result is pending")
_all("icp_map_update_vertex_map", ORDERED, begun=REFUSED(RIP), batch_hold=REFUSED(BH), control=True, note=_MAPFIX)
_all("icp_map_stage_cloud", ORDERED, begun=REFUSED(RIP), frame=REFUSED(FRM), pframe=REFUSED(FRM), batch_hold=REFUSED(BH),
     control="staging alone changes no registration (icp_map_update_staged has the teeth)",
     note="issue item 2: confirmed by reading, fixed (api.hip icp_map_stage_cloud)")
_all("icp_map_update_staged", ORDERED, begun=REFUSED(RIP), frame=REFUSED(FRM), pframe=REFUSED(FRM), batch_hold=REFUSED(BH),
     control=True, note="issue item 3: confirmed by reading, fixed (api.hip icp_map_update_staged)")
_all("icp_map_normals_owned", ORDERED, begun=REFUSED(RIP), batch_hold=REFUSED(BH), control="re-estimates the same normals")
_all("icp_map_normals_install", ORDERED, begun=REFUSED(RIP), batch_hold=REFUSED(BH), control=True)
_all("icp_register_launch", ORDERED, two_pending=REFUSED(TWO), begun=REFUSED(RIP), batch_hold=REFUSED(BH),
     control="the next registration: it has no effect on the one in flight")
_all("icp_register_launch_from_last", ORDERED, two_pending=REFUSED(TWO), begun=REFUSED(RIP), batch_hold=REFUSED(BH),
     control="the next registration: it has no effect on the one in flight")
_all("icp_odometry_init", ORDERED, begun=REFUSED(RIP), frame=COLLECTS, pframe=REFUSED("holds a projective map"),
     pmap_launched=REFUSED("holds a projective map"), batch_hold=REFUSED("held by a batched registration"),
     control="an empty map refuses the launch", note="icp_map_init behind frame_drop_pending")

# ---- refused while a registration is enqueued or uncollected (shared buffers: targets, partial rows, normal equations, scratch)
for _s in ("icp_estimate_timestamps", "icp_kitti360_prepare"):
    _all(_s, REFUSED(RIP), overlapped=_SCRATCH)
for _s in ("icp_align_point_to_plane", "icp_align_point_to_point", "icp_weighted_procrustes", "icp_nearest_neighbor_search",
           "icp_exchange_create", "icp_exchange_destroy"):
    _all(_s, REFUSED(RIP), overlapped=ORDERED)
_all("icp_exchange_connect", REFUSED(RIP), overlapped=ORDERED,
     note="fixed (api.hip icp_exchange_connect): switched exchange_on under enqueued and held-back iterations")
_all("icp_knn_query", REFUSED("icp_knn_query: " + RIP), batch_hold=REFUSED(BH), overlapped=ORDERED,
     note="held: the held-back iterations are enqueued first, then the refusal")
_all("icp_map_normals_peek", REFUSED("icp_map_normals_peek: " + RIP), overlapped=ORDERED)
for _s in ("icp_last_neighbors", "icp_last_cache_entries"):
    _all(_s, REFUSED(RIP), overlapped=REFUSED("no fused registration against the current map"),
         note="issue item 5: refuted, both check in_registration || result_pending()")
_all("icp_register", REFUSED(PEND), begun=REFUSED(RIP), overlapped=ORDERED)
_all("icp_register_begin", REFUSED(PEND), begun=REFUSED(RIP), overlapped=ORDERED)
_all("icp_pmap_register", REFUSED(AWAIT), overlapped=ORDERED,
     note="fixed (register.hip icp_pmap_register): returned the older pending result as its own")
_all("icp_pmap_register_launch", REFUSED(AWAIT), overlapped=ORDERED)
for _s in ("icp_iteration_accumulate", "icp_iteration_solve"):
    _all(_s, REFUSED(NOREG), begun=NA, note="begun: the state's own driver; the refusal names its reason now (register.hip)")
# (the frame calls on a context without a sequence of that kind — every state but its own — say so first; with a sequence
# icp_frame_launch says "a registration of this context is in progress or awaits icp_register_end")
NOSEQ, NOFRAME = "no sequence", "no frame launched"
_all("icp_frame_launch", REFUSED("icp_frame_launch: " + NOSEQ), frame=REFUSED("a frame is already launched"), overlapped=ORDERED)
_all("icp_pmap_frame_launch", REFUSED("icp_pmap_frame_launch: " + NOSEQ), pframe=REFUSED("a frame is already launched"),
     overlapped=ORDERED)
_all("icp_frame_end", REFUSED("icp_frame_end: " + NOFRAME), frame=COLLECTS)
_all("icp_pmap_frame_end", REFUSED("icp_pmap_frame_end: " + NOFRAME), pframe=COLLECTS)
_all("icp_pmap_odometry_init", REFUSED(AWAIT), frame=REFUSED("a kd-tree sequence"), pframe=COLLECTS,
     batch_hold=REFUSED("held by a batched registration"), overlapped=ORDERED)

# ---- the call that ends the state
_all("icp_register_end", COLLECTS, frame=REFUSED(FRM), pframe=REFUSED(FRM), batch_hold=REFUSED("icp_batch_register_end"),
     overlapped=REFUSED("no registration to collect"),
     note="issue item 1: confirmed by reading, fixed (register.hip: icp_register_end refuses, the frame calls use register_collect)")

# ---- the batched forms, called on a batch ONE member of which (member 0) is in the state.  batch.hip: front_batch_check refuses
# a member in registration, front_batch_flush enqueues what the batch and every member hold back (batch_flush +
# continue_launch), pmap_batch_check refuses a member with anything pending, batch_members_free refuses a begun member and a
# member whose own frame is launched.  The batched frame calls (batch_frame_plan.h) ask every member for a sequence first.
OWN = "a frame is launched and awaits its end"
STILL = "a registration is still pending"
MEMBER_REG = "a registration of the member's own is in progress or awaits its end"
for _s in ("icp_batch_preprocess", "icp_batch_project_rows"):
    _all(_s, ORDERED, begun=REFUSED(RIP), overlapped=INDEPENDENT("as the single calls"))
_all("icp_batch_project", INDEPENDENT("no check and no flush of the members, the buffers of icp_project"))
_all("icp_batch_stage", ORDERED, begun=REFUSED(RIP), frame=REFUSED(OWN), pframe=REFUSED(OWN),
     note="fixed (batch.hip): replaced the rows a member's own launched frame staged")
_all("icp_batch_estimate_timestamps", REFUSED(RIP), overlapped=INDEPENDENT("as icp_estimate_timestamps"))
_all("icp_batch_set_stream", ORDERED, batch_hold=REFUSED(BH), control="a stream changes no result")
_all("icp_batch_register_launch", ORDERED, two_pending=REFUSED(TWO), begun=REFUSED(RIP), control="the next registration",
     note="fixed (batch.hip): a launch that failed on a begun member abandoned the caller's registration")
_all("icp_batch_map_update", ORDERED, begun=REFUSED(RIP), frame=REFUSED(OWN), pframe=REFUSED(OWN), control=True,
     note="fixed (batch.hip): no check of a begun member or of a member's own frame")
_all("icp_batch_map_update_staged", ORDERED, begun=REFUSED(RIP), frame=REFUSED(OWN), pframe=REFUSED(OWN), control=True,
     note="fixed (batch.hip): consumed the rows a member's own launched frame staged")
_all("icp_batch_pmap_register_launch", REFUSED(STILL), overlapped=ORDERED)
_all("icp_batch_pmap_update", REFUSED(STILL), overlapped=ORDERED)
_all("icp_batch_register_end", COLLECTS, frame=REFUSED(OWN), pframe=REFUSED(OWN), overlapped=REFUSED("no registration to collect"),
     note="fixed (batch.hip): collected a member's own frame registration; collects through register_collect")
_all("icp_batch_odometry_init", ORDERED, begun=REFUSED(RIP), frame=COLLECTS, pframe=REFUSED("holds a projective map"),
     pmap_launched=REFUSED("holds a projective map"), batch_hold=REFUSED("held by a batched registration"),
     control="an empty map refuses the launch")
_all("icp_batch_pmap_odometry_init", REFUSED(AWAIT), frame=REFUSED("a kd-tree sequence"), pframe=COLLECTS,
     batch_hold=REFUSED("held by a batched registration"), overlapped=ORDERED)
_all("icp_batch_frame_launch", REFUSED(MEMBER_REG), pframe=REFUSED(NOSEQ), pmap_launched=REFUSED(NOSEQ), overlapped=ORDERED,
     note="members with a kd-tree sequence; without one: no sequence")
_all("icp_batch_pmap_frame_launch", REFUSED(NOSEQ), frame=REFUSED("a kd-tree sequence"), pframe=REFUSED(MEMBER_REG), overlapped=ORDERED)
_all("icp_batch_frame_end", REFUSED("no step launched"),
     note="frame: a frame the member launched itself is ended by the member")
_all("icp_batch_pmap_frame_end", REFUSED("no step launched"))


# ---- the scenario runner -----------------------------------------------------------------------------------------------------
class RigError(Exception):
    """A step of a scenario other than the call under test failed."""


Outcome = namedtuple("Outcome", "status message output")       # of the call under test; message = icp_last_error
Result = namedtuple("Result", "bits iterations")               # of a registration or a frame: every returned bit, hashable
Trace = namedtuple("Trace", "results x snapshot error")        # error: (step, text) of the RigError that ended the scenario

CHECKS = ("precondition-held", "scenario-error", "x-status", "refusal-status", "refusal-message", "registration", "collect-order",
          "frame-end", "refusal-changed-nothing", "context-after-refusal", "map", "next-registration", "x-output", "control")


def run_scenario(factory, state, symbol, chunked, x_when, variant=None):
    """One run.  `factory(chunked, state, variant)` returns a rig on a fresh context with the methods
         prepare()            the map and the SHORT registration, collected (results += 1)
         enter()              the launches that produce the state
         call(symbol)         the call under test by its recipe -> Outcome
         finish()             the COLLECTS calls of the state (results += the registrations / the frame in flight)
         follow()             the next registration on the same context (results += 1)
         snapshot()           (map points, number of clouds, normal cache) as hashable bits
         close()
       and the fields results (list of Result) and hold (index of the short and of the held registration in results, or None).
       x_when: "inflight" (between enter and finish), "before" (in front of enter: an idle context), "never"."""
    rig = factory(chunked, state, variant)
    x = snap = error = None
    step = "prepare"
    try:
        rig.prepare()
        if x_when == "before":
            step = "call"
            x = rig.call(symbol)
        step = "enter"
        rig.enter()
        if x_when == "inflight":
            step = "call"
            x = rig.call(symbol)
        step = "finish"
        rig.finish()
        step = "follow"
        rig.follow()
        step = "snapshot"
        snap = rig.snapshot()
    except RigError as e:
        error = (step, str(e))
    finally:
        results = list(rig.results)
        hold = rig.hold
        rig.close()
    return Trace(results, x, snap, error), hold


def run_cell(factory, state, symbol, cell, control=NOTEETH, variant=None, cache=None):
    """Holds one cell: the run under test ("chunked_launch" 1) against its twin ("chunked_launch" 0).  Returns the names of the
    checks that failed (CHECKS), [] for a cell that holds.
      ORDERED       twin: the same calls.  registration / map / next-registration / x-output equal; with a control, the call made
                    BEFORE the launch must change the registrations (control).  Between the two frame calls too: an explicit
                    icp_map_update in front of icp_frame_end and the same update behind it give different maps (the end moves
                    the map and appends the frame's rows), so "the frame ends first" is no twin of an ORDERED call — the frame's
                    own result still is the one of the same calls without chunking
      INDEPENDENT   twin: the call on the idle context in front of the launch (X's own output on an idle twin), the work in flight
                    untouched by it.  In the frame states this stands for "the twin ends the frame first": X made afterwards
                    would read a map the frame's end has already moved
      REFUSED       twin: never makes the call.  status, message, then nothing changed and the context usable
      COLLECTS      twin: the same.  registration, and for two results: oldest first (collect-order)"""
    kind = cell.kind
    if kind == "N/A":
        return []
    cache = {} if cache is None else cache

    # (two results pending: the twin launches and collects ONE AT A TIME — the order the two slots must be handed out in
    # cannot be read off a twin that uses the same two slots)
    twin_variant = "one_at_a_time" if state == "two_pending" else variant

    def twin_of(x_when, sym):
        key = (state, twin_variant, x_when, sym if x_when != "never" else None)
        if key not in cache:
            cache[key] = run_scenario(factory, state, sym, 0, x_when, twin_variant)
        return cache[key]

    x_when = {"ORDERED": "inflight", "INDEPENDENT": "inflight", "REFUSED": "inflight", "COLLECTS": "never"}[kind]
    under, hold = run_scenario(factory, state, symbol, 1, x_when, variant)
    twin, _ = twin_of({"ORDERED": "inflight", "INDEPENDENT": "before", "REFUSED": "never", "COLLECTS": "never"}[kind], symbol)
    fails = []
    if twin.error:
        return ["scenario-error"]
    if hold is not None:  # iterations were in fact held back when the call was made
        short, held = twin.results[hold[0]].iterations, twin.results[hold[1]].iterations
        if held < short + 3:
            return ["precondition-held"]
    if kind == "REFUSED":
        if under.x is None:
            return ["scenario-error"]
        if under.x.status != ICP_ERR_INVALID_ARGUMENT:
            return ["refusal-status"]
        if cell.text not in (under.x.message or "") or not under.x.message:
            fails.append("refusal-message")
        if under.error:
            return fails + ["context-after-refusal"]
    else:
        if under.error:
            return ["frame-end" if under.error[0] == "finish" and state in ("frame", "pframe") else "scenario-error"]
        if kind != "COLLECTS" and (under.x is None or under.x.status != 0):
            return ["x-status"]
    n = min(len(under.results), len(twin.results)) - 1  # the registrations in front of the follow-up
    if under.results[:n] != twin.results[:n] or len(under.results) != len(twin.results):
        swapped = state == "two_pending" and n >= 2 and under.results[n - 2:n] == twin.results[n - 2:n][::-1] and \
            under.results[:n - 2] == twin.results[:n - 2]
        fails.append("collect-order" if swapped else "registration")
    changed = []
    if under.snapshot != twin.snapshot:
        changed.append("map")
    if under.results[n:] != twin.results[n:]:
        changed.append("next-registration")
    if kind == "REFUSED":
        if changed:
            fails.append("refusal-changed-nothing")
    else:
        fails += changed
        if kind != "COLLECTS" and under.x.output != twin.x.output:
            fails.append("x-output")
    if kind == "ORDERED" and control is True and not fails and state != "overlapped":  # (overlapped: no registration in flight)
        ctl, _ = run_scenario(factory, state, symbol, 0, "before", twin_variant)
        if ctl.error is None and ctl.results[:n] == twin.results[:n]:
            fails.append("control")
    return fails


# ---- the fixtures of the GPU audit (numpy and the package's synthetic scene: imported on demand, no GPU) ----------------------
# The smallest shapes at which chunking exists: 16 x 512 scans (8 192 rows) against a fixed map of 10 000 points in the frame
# of scan 3.  SHORT = scan 3 itself (the oracle stops after K1_ORACLE = 3 iterations), JUMP = scan 10 from the identity (9
# iterations: 2.8 m away), so a first chunk of k1 + 1 = 4 leaves five iterations held back — more than the chunk of four
# icp_register_end adds at a time.  tests/test_inflight_audit.py asserts those counts on the CPU.
HEIGHT, WIDTH, MAP_POINTS = 16, 512, 10_000
THRESHOLD, SCHEME, SIGMA, LOCAL_MAP_SIZE = 1.0e-4, "geman_mcclure", 0.3, 3
K1_ORACLE = 3
SHORT_FRAME, JUMP_FRAME, SECOND_FRAME, NEXT_FRAME = 3, 10, 11, 4
# the frame states: frames 0, 1, 2 in order, then a jump to frame 6 (the constant-velocity guess is one step, the motion four),
# then frame 7
FRAME_PROLOGUE, FRAME_JUMP, FRAME_NEXT = (0, 1, 2), 6, 7
_FIXTURE = {}


def kd_fixture():
    """{"scans": 12 scans [8192, 3] float32, "poses", "map" [10000, 3], "map2" (another map of the same scene), "short", "jump",
    "second", "next"} — computed once."""
    if not _FIXTURE:
        from pylidar_slam_amd.synthetic import SceneConfig, make_fixed_map, make_sequence
        cfg = SceneConfig(height=HEIGHT, width=WIDTH)
        scans, poses = make_sequence(cfg, 12)
        _FIXTURE.update(scans=scans, poses=poses,
                        map=make_fixed_map(cfg, scans[:4], poses[:4], ref_frame=3, num_points=MAP_POINTS),
                        map2=make_fixed_map(cfg, scans[2:6], poses[2:6], ref_frame=1, num_points=MAP_POINTS - 1000, seed=11),
                        short=scans[SHORT_FRAME], jump=scans[JUMP_FRAME], second=scans[SECOND_FRAME], next=scans[NEXT_FRAME])
    return _FIXTURE


# ---- the toy: a deterministic model of the host-side state machine -------------------------------------------------------------
# Iteration k of a registration is worth hash((k, map version, configuration version, normals version, packed targets)) at the
# moment it is ENQUEUED; a registration of scan s needs NEED[s] iterations (what the stop threshold decides on the device), so
# its result is the first NEED[s] of the outcomes enqueued for it — whoever lets a held-back iteration see a change, or collects
# the wrong slot, changes a bit.
MAX_ITERATIONS = 20
NEED = {"short": 3, "jump": 9, "next": 4, "second": 5}
FAULTS = ("no_flush", "one_chunk", "flush_after", "refusal_mutates", "refusal_in_registration", "register_end_takes_frame",
          "stage_replaces_frame_rows", "update_staged_consumes", "independent_rewrites_targets", "newest_first")

# what a call changes once it takes effect (toy): the rest only touches scratch
EFFECT = {"icp_map_init": "map", "icp_map_set": "map", "icp_map_update": "map", "icp_map_update_vertex_map": "map",
          "icp_map_stage_cloud": "stage", "icp_map_update_staged": "update_staged", "icp_set_option": "config",
          "icp_set_cost": "config", "icp_set_alignment": "config", "icp_map_normals_install": "normals",
          "icp_map_normals_owned": "normals_same", "icp_set_stream": "stream", "icp_map_get": "read_map",
          "icp_register_launch": "launch", "icp_register_launch_from_last": "launch", "icp_odometry_init": "map",
          "icp_pmap_init": "pmap", "icp_pmap_update": "pmap",
          "icp_batch_map_update": "map", "icp_batch_map_update_staged": "update_staged", "icp_batch_stage": "stage",
          "icp_batch_set_stream": "stream", "icp_batch_odometry_init": "map", "icp_batch_register_launch": "launch",
          "icp_batch_pmap_update": "pmap"}


class ToyContext:
    def __init__(self, chunked=1, live=True, fault=None, table=None):
        self.chunked, self.live, self.fault, self.table = chunked, live, fault, table or TABLE
        self.map, self.map_version, self.cfg_version, self.normals, self.pmap, self.stream, self.scratch = ("m0",), 0, 0, 0, 0, 0, 0
        self.last_iterations = 0
        self.pending = []            # registrations launched and not collected, oldest first (two result slots)
        self.in_registration = False
        self.begun = None
        self.staged = None
        self.frame = None            # {"key": bool, "rows": id} while a frame is launched
        self.batch_hold = False
        self.error = ""

    # -- the machine
    def _enqueue(self, reg, count):
        for _ in range(max(0, min(count, MAX_ITERATIONS - reg["enq"]))):
            reg["out"].append(hash((reg["enq"], self.map_version, self.cfg_version, self.normals, reg["packed"])))
            reg["enq"] += 1

    def _flush(self):
        if not self.pending or self.fault == "no_flush":
            return
        reg = self.pending[-1]
        self._enqueue(reg, 4 if self.fault == "one_chunk" else MAX_ITERATIONS)

    def _fail(self, text):
        self.error = text
        return ICP_ERR_INVALID_ARGUMENT

    def launch(self, scan):
        if self.in_registration:
            return self._fail(RIP)
        if len(self.pending) >= 2:
            return self._fail(TWO)
        if self.batch_hold:
            return self._fail(BH)
        self._flush()
        reg = {"scan": scan, "packed": scan, "enq": 0, "out": []}
        first = self.last_iterations + 1 if (self.chunked and self.live) else MAX_ITERATIONS
        self._enqueue(reg, first)
        self.pending.append(reg)
        return 0

    def begin(self, scan):
        if self.pending:
            return self._fail(PEND)
        if self.in_registration:
            return self._fail(RIP)
        self.in_registration = True
        self.begun = {"scan": scan, "packed": scan, "enq": 0, "out": []}
        return 0

    def accumulate_solve(self):
        if not self.in_registration or self.begun is None:
            return self._fail(NOREG)
        self._enqueue(self.begun, 1)
        return 0

    def _collect(self):
        """-> (status, Result)"""
        if self.begun is not None and not self.pending:
            reg, self.begun, self.in_registration = self.begun, None, False
        elif self.pending:
            reg = self.pending.pop(-1 if self.fault == "newest_first" else 0)
            if not self.pending:  # (only the newest registration may still hold iterations back)
                while reg["enq"] < min(NEED[reg["scan"]], MAX_ITERATIONS):
                    self._enqueue(reg, 4)
        else:
            return self._fail("no registration to collect"), None
        need = min(NEED[reg["scan"]], reg["enq"])
        self.last_iterations = need
        return 0, Result(tuple(reg["out"][:need]), need)

    def register_end(self):
        if self.frame is not None and self.fault != "register_end_takes_frame":
            return self._fail("icp_register_end: " + FRM), None
        if self.batch_hold:
            return self._fail("collect it with icp_batch_register_end"), None
        return self._collect()

    def frame_launch(self, scan, key):
        if self.frame is not None or self.pending or self.in_registration:
            return self._fail("icp_frame_launch: ")
        self.staged = "rows-" + scan
        rc = self.launch(scan)
        if rc == 0:
            self.frame = {"key": key}
        return rc

    def frame_end(self):
        if self.frame is None:
            return self._fail("icp_frame_end: no frame launched"), None
        rc, res = self._collect()
        if rc:
            return rc, None
        frame, self.frame = self.frame, None
        self._flush()
        if frame["key"]:
            if self.staged is None:
                return self._fail("no staged cloud (icp_map_stage_cloud)"), None
            self.map, self.staged = self.map + (self.staged,), None
        self.map_version += 1
        return 0, Result(res.bits + (frame["key"],), res.iterations)

    # -- the call under test, by the table
    def _apply(self, symbol):
        effect = EFFECT.get(symbol, "scratch")
        if effect == "map":
            self.map, self.map_version = ("x-" + symbol,), self.map_version + 1
        elif effect == "config":
            self.cfg_version += 1
        elif effect == "normals":
            self.normals += 1
        elif effect == "pmap":
            self.pmap += 1
        elif effect == "stream":
            self.stream += 1
        elif effect == "stage":
            self.staged = "rows-x"
        elif effect == "update_staged":
            if self.staged is None:
                return self._fail("no staged cloud (icp_map_stage_cloud)"), None
            self.map, self.staged, self.map_version = self.map + (self.staged,), None, self.map_version + 1
            return 0, len(self.map)
        elif effect == "read_map":
            return 0, self.map
        elif effect == "launch":
            if symbol.startswith("icp_batch_"):
                self.batch_hold = False  # (batch_flush: what the batch held back is enqueued by _flush below)
            return self.launch("second"), None
        else:
            self.scratch += 1
        return 0, None

    def call(self, symbol, state):
        cell = self.table[symbol].cells[state]
        # the three frame cells as the library was before the audit: the call goes through
        if self.frame is not None and (symbol, self.fault) in (("icp_register_end", "register_end_takes_frame"),
                                                               ("icp_map_stage_cloud", "stage_replaces_frame_rows"),
                                                               ("icp_map_update_staged", "update_staged_consumes")):
            if symbol == "icp_register_end":
                rc, res = self._collect()
                return Outcome(rc, self.error if rc else "", res)
            rc, out = self._apply(symbol)
            return Outcome(rc, self.error if rc else "", out)
        if cell.kind == "REFUSED":
            if self.fault == "refusal_mutates":
                self._apply(symbol)
            if self.fault == "refusal_in_registration":
                self.in_registration = True
            if symbol == "icp_knn_query":
                self._flush()  # (ICP_HELD_FIRST stands in front of its refusal)
            return Outcome(self._fail(symbol + ": " + cell.text), self.error, None)
        if cell.kind == "ORDERED":
            if self.batch_hold and not symbol.startswith("icp_batch_"):  # (the batch's own calls flush what it holds)
                return Outcome(self._fail(BH), self.error, None)
            if self.fault == "flush_after":
                rc, out = self._apply(symbol)
                self._flush()
            else:
                self._flush()
                rc, out = self._apply(symbol)
            return Outcome(rc, self.error if rc else "", out)
        if cell.kind == "INDEPENDENT":
            if self.fault == "independent_rewrites_targets" and self.pending:
                self.pending[-1]["packed"] = "x"
            effect = EFFECT.get(symbol, "scratch")
            if effect == "read_map":
                return Outcome(0, "", self.map)
            if effect == "pmap":
                self.pmap += 1
            else:
                self.scratch += 1
            return Outcome(0, "", None)
        raise RigError(f"the toy has no call for a {cell.kind} cell ({symbol}, {state})")


class ToyRig:
    """The runner's rig over a ToyContext.  The projective and batched states reuse the kd-tree machine: pframe is a frame whose
    iterations are all enqueued, pmap_launched a pending registration, batch_hold a held one that refuses the single calls,
    overlapped an idle context (the toy has one stream)."""

    def __init__(self, chunked, state, variant=None, fault=None, table=None):
        live = state in ("held", "frame", "batch_hold")
        self.state, self.variant = state, variant
        self.ctx = ToyContext(chunked, live, fault, table)
        self.results = []
        self.hold = (0, 1) if state in ("held", "batch_hold") else None

    def _ok(self, rc, what):
        if rc:
            raise RigError(f"{what}: {self.ctx.error}")

    def _collect(self, fn, what):
        rc, res = fn()
        self._ok(rc, what)
        self.results.append(res)

    def prepare(self):
        self._ok(self.ctx.launch("short"), "launch short")
        self._collect(self.ctx.register_end, "end short")

    def enter(self):
        c, s = self.ctx, self.state
        if s in ("held", "pending", "pmap_launched", "batch_hold"):
            self._ok(c.launch("jump"), "launch")
            c.batch_hold = s == "batch_hold"
        elif s == "two_pending":
            self._ok(c.launch("jump"), "launch")
            if self.variant == "one_at_a_time":
                self._collect(c.register_end, "register end")
            self._ok(c.launch("second"), "launch from last")
        elif s == "begun":
            self._ok(c.begin("jump"), "begin")
            self._ok(c.accumulate_solve(), "accumulate")
        elif s in ("frame", "pframe"):
            c.staged = "rows-own"  # (what an ORDERED icp_map_update_staged of the caller would consume: never the frame's)
            self._ok(c.frame_launch("jump", self.variant != "nonkey"), "frame launch")

    def call(self, symbol):
        if self.state not in ("frame", "pframe") and EFFECT.get(symbol) == "update_staged" and self.ctx.staged is None:
            self.ctx.staged = "rows-own"
        return self.ctx.call(symbol, self.state)

    def finish(self):
        c, s = self.ctx, self.state
        if s in ("frame", "pframe"):
            self._collect(c.frame_end, "frame end")
            return
        if s == "begun":
            for _ in range(NEED["jump"] - 1):
                self._ok(c.accumulate_solve(), "accumulate")
        if s == "batch_hold":
            c.batch_hold = False  # (icp_batch_register_end)
        while c.pending or c.begun is not None:
            self._collect(c.register_end, "register end")

    def follow(self):
        self._ok(self.ctx.launch("next"), "launch next")
        self._collect(self.ctx.register_end, "end next")

    def snapshot(self):
        c = self.ctx
        return (c.map, c.map_version, c.normals, c.cfg_version)

    def close(self):
        pass


def toy_factory(fault=None, table=None):
    return lambda chunked, state, variant=None: ToyRig(chunked, state, variant, fault, table)
