"""Contexts beside each other on one device: the table of what a context A in an in-flight state and a job of a neighbour B do to
each other, the runner that holds an implementation to a cell of that table, and a toy model of the host state every context of
a process shares (csrc/api.hip: g_registering, registering_enter / _leave; register.hip: register_begin's lead_latched,
RegisteringGuard; batch.hip: the batched decision, BatchUnwind).  TEST INFRASTRUCTURE: standard library only, importable without
a GPU, never imported by the package.  tests/test_neighbour_audit.py holds the runner on the toy and on deliberately wrong copies
of it, tests/test_gpu_neighbour_audit.py runs the library through the same runner.

WHAT IS SHARED.  Lead launches make the workgroups of a launch wait for one another (the pose mailbox), which is only safe while
no other launch of the process competes for the device.  So every registration against the kd-tree style map ENTERS a count per
device when it begins and LEAVES it when its context has neither a registration in progress nor a result pending; a registration
that finds another context counted is latched onto per-iteration launches ("plain") for all its chunks.  A batch answers once
for all its members and counts them out.  Projective registrations never enter the count.  Lead and plain launches compute the
same bits: a wrong answer shows as a lost speed-up (decision), a stale mailbox pose (latched, bits) or a leaked count that
turns every later registration of the process plain (count).

THE DRIVERS.  The parties below are written once, against a small protocol a `world` offers:
  world.context(live, projective=False) -> a context driver: map_set() register(s) launch(s, last=False) end() begin(s) pair()
        odometry_init(key) frame_launch(k) frame_end() pmap_setup() pmap_register(k) pmap_launch(k) pmap_odometry_init(key)
        pframe_launch(k) pframe_end() nns() knn() map_update_cloud() leads() fallbacks() snapshot() close()
  world.batch(contexts) -> launch(scans, last=False) map_update() end() close()
  world.count() -> the device's count            world.tick() -> called by a driver behind EVERY library call it makes
Scans are named ("short", "jump", "second", "next", "one_row", "odd_rows"), frames numbered; a registration or a frame returns a
hashable Result of every returned bit.  ToyWorld is one implementation, the GPU test file holds the other.

THE CHECKS (run_cell returns the FIRST that fails: what follows a wrong count is derived from it):
  scenario-error     a step failed, or a step began another number of registrations than the table says
  count              world.count() == the number of contexts in registration or with a result pending, behind every call; 0 at the end
  decision           a step raises lead_registrations() by the registrations it began if no OTHER party is counted, else by zero
  timeouts           handoff_fallbacks() == 0 everywhere
  precondition-held  the chunked registration ran at least k1 + 3 iterations: chunks were in fact held back
  latched            a chunked registration equals its solo twin whatever began or ended between its chunks
  bits               every other result, the maps and normals afterwards, and the next registration equal the solo twin
"""
from collections import namedtuple

Result = namedtuple("Result", "bits iterations")
CHECKS = ("scenario-error", "count", "decision", "timeouts", "precondition-held", "latched", "bits")

# ---- the table -----------------------------------------------------------------------------------------------------------------
# counted: contexts of A in the count while A is in the state; begins: kd-tree registrations its `enter` begins; live: a live
# stop threshold (chunks); hold: index pair (short, held) into A's results where the state holds iterations back
State = namedtuple("State", "counted begins live hold note")
STATES = {
    "held": State(1, 1, True, (0, 1), "icp_register_launch, chunks held back"),
    "pending": State(1, 1, False, None, "icp_register_launch, forced count, uncollected"),
    "two_pending": State(1, 2, False, None, "icp_register_launch + _from_last, neither collected"),
    "begun": State(1, 1, False, None, "between icp_register_begin and icp_register_end"),
    "frame": State(1, 1, True, None, "between icp_frame_launch and icp_frame_end"),
    "batch_hold": State(3, 3, True, (0, 3), "three members of a batch whose chunked registration holds iterations back"),
    "pframe": State(0, 0, False, None, "NOT counted: projective registrations never enter the count"),
    "pmap_launched": State(0, 0, False, None, "NOT counted: behind icp_pmap_register_launch"),
}
# spans: the job has a launching and a collecting call (two finishing orders exist); counted / begins as above, while it spans
Job = namedtuple("Job", "spans counted begins live hold note")
JOBS = {
    "register": Job(False, 0, 1, False, None, "icp_register"),
    "launch_forced": Job(True, 1, 1, False, None, "icp_register_launch + icp_register_end, forced iterations"),
    "launch_one_row": Job(True, 1, 1, False, None, "the same, a scan of 1 row"),
    "launch_odd_rows": Job(True, 1, 1, False, None, "the same, a scan of 4097 rows"),
    "launch_live": Job(True, 1, 1, True, (0, 1), "the same with a live threshold: chunked"),
    "two_last": Job(True, 1, 2, False, None, "two launches, the second from \"last\", collected one by one"),
    "frame_key": Job(True, 1, 1, False, None, "icp_frame_launch + icp_frame_end, a key frame"),
    "frame_none": Job(True, 1, 1, False, None, "the same, a frame that is no key frame"),
    "pmap_register": Job(False, 0, 0, False, None, "icp_pmap_register"),
    "pmap_frame": Job(True, 0, 0, False, None, "icp_pmap_frame_launch + icp_pmap_frame_end"),
    "batch3": Job(True, 3, 3, False, None, "a batch of three: register_launch + map_update + register_end"),
    "batch_two": Job(True, 3, 6, False, None, "a batch of three launched twice back to back, the second from \"last\""),
    "sharded": Job(True, 1, 1, False, None, "icp_register_begin, icp_iteration_accumulate / _solve, icp_register_end"),
    "nns": Job(False, 0, 0, False, None, "icp_nearest_neighbor_search"),
    "knn": Job(False, 0, 0, False, None, "icp_knn_query"),
    "map_update": Job(False, 0, 0, False, None, "icp_map_update with a cloud under \"overlap_map_update\" 1"),
}
ORDERS = {
    "b_first": (("a", "prepare"), ("b", "prepare"), ("a", "enter"), ("b", "begin"), ("b", "end"), ("a", "finish"),
                ("a", "follow"), ("b", "follow")),
    "a_first": (("a", "prepare"), ("b", "prepare"), ("a", "enter"), ("b", "begin"), ("a", "finish"), ("b", "end"),
                ("a", "follow"), ("b", "follow")),
}
# (state, job, order): why the cell cannot exist
SKIPPED = {(s, j, "a_first"): "the job returns collected: nothing of B is in flight when A ends, one finishing order"
           for s in STATES for j, job in JOBS.items() if not job.spans}
SKIPPED[("batch_hold", "member_of_that_batch", "*")] = "B as a member of the batch that holds A: the batch's own call, " \
    "held to its class by the inflight audit (icp_batch_* beside batch_hold)"
SKIPPED[("begun", "same_context", "*")] = "B on A's own context: the inflight audit's REFUSED cells"
CELLS = [(s, j, o) for s in STATES for j in JOBS for o in ORDERS if (s, j, o) not in SKIPPED]

BEGUN_PAIRS = 8       # accumulate + solve pairs of a registration driven through the sharded seam (the forced count)
FRAME_PROLOGUE, FRAME_JUMP, FRAME_NEXT = (0, 1, 2), 6, 7   # A's frame states, as the inflight audit's
JOB_FRAMES = (0, 1, 2), 3, 4                              # B's frame jobs: consecutive frames


class RigError(Exception):
    """A step of a scenario failed in the driver."""


class _Failed(Exception):
    pass


# ---- the parties: written once, run on the toy and on the device ------------------------------------------------------------------
class _Party:
    def __init__(self, world):
        self.world, self.results, self.counted, self.ctxs, self.batch, self.hold = world, [], 0, [], None, None

    def leads(self):
        return sum(c.leads() for c in self.ctxs)

    def fallbacks(self):
        return sum(c.fallbacks() for c in self.ctxs)

    def snapshot(self):
        return tuple(c.snapshot() for c in self.ctxs)

    def close(self):
        if self.batch is not None:
            self.batch.close()
        for c in self.ctxs:
            c.close()
        self.counted = 0

    def run(self, step):
        """-> the kd-tree registrations the step began"""
        return getattr(self, step)() or 0

    # (self.counted is set BEFORE the call that changes it: the driver ticks behind the call; icp_register enters and leaves
    # inside one call)
    def _sync_register(self, c, scan):
        self.results.append(c.register(scan))

    def _frames(self, c, frames, launch, end, kd):
        begun = 0
        for k in frames:
            registers = kd and c.frame_index > 0
            self.counted += registers
            launch(k)
            self.counted -= registers  # (the frame's end collects its registration: the context leaves inside the call)
            self.results.append(end())
            begun += registers
        return begun


class PartyA(_Party):
    """A context (three for batch_hold) brought into `state` by the recipe of the inflight audit."""

    def __init__(self, world, state):
        super().__init__(world)
        self.state, spec = state, STATES[state]
        projective = state in ("pframe", "pmap_launched")
        self.ctxs = [world.context(spec.live, projective) for _ in range(3 if state == "batch_hold" else 1)]
        self.c = self.ctxs[0]
        self.batch = world.batch(self.ctxs) if state == "batch_hold" else None
        self.hold = spec.hold

    def prepare(self):
        c, s = self.c, self.state
        if s == "frame":
            c.odometry_init(True)
            return self._frames(c, FRAME_PROLOGUE, c.frame_launch, c.frame_end, True)
        if s == "pframe":
            c.pmap_odometry_init(True)
            return self._frames(c, FRAME_PROLOGUE, c.pframe_launch, c.pframe_end, False)
        if s == "pmap_launched":
            c.pmap_setup()
            self.results.append(c.pmap_register(1))
            return 0
        for m in self.ctxs:
            m.map_set()
        for m in self.ctxs:
            self._sync_register(m, "short")
        return len(self.ctxs)

    def enter(self):
        c, s = self.c, self.state
        self.counted = STATES[s].counted
        if s in ("held", "pending"):
            c.launch("jump")
        elif s == "two_pending":
            c.launch("jump")
            c.launch("second", last=True)
        elif s == "begun":
            c.begin("jump")
            for _ in range(2):
                c.pair()
        elif s == "frame":
            c.frame_launch(FRAME_JUMP)
        elif s == "pframe":
            c.pframe_launch(3)
        elif s == "pmap_launched":
            c.pmap_launch(3)
        elif s == "batch_hold":
            self.batch.launch(["jump", "jump_b", "second"])
        return STATES[s].begins

    def finish(self):
        c, s = self.c, self.state
        if s == "begun":
            for _ in range(BEGUN_PAIRS - 2):
                c.pair()
        if s == "two_pending":
            self.results.append(c.end())  # (the older one: the context stays counted for the newer)
        self.counted = 0
        if s == "frame":
            self.results.append(c.frame_end())
        elif s == "pframe":
            self.results.append(c.pframe_end())
        elif s == "batch_hold":
            self.results += self.batch.end()
        else:
            self.results.append(c.end())

    def follow(self):
        c, s = self.c, self.state
        if s == "frame":
            return self._frames(c, (FRAME_NEXT,), c.frame_launch, c.frame_end, True)
        if s == "pframe":
            return self._frames(c, (4,), c.pframe_launch, c.pframe_end, False)
        if s == "pmap_launched":
            self.results.append(c.pmap_register(4))
            return 0
        self._sync_register(c, "next")
        return 1


class PartyB(_Party):
    """The neighbour: a context (three for the batched jobs) of its own that runs `job` between `begin` and `end`."""

    def __init__(self, world, job):
        super().__init__(world)
        self.job, spec = job, JOBS[job]
        projective = job in ("pmap_register", "pmap_frame")
        self.ctxs = [world.context(spec.live, projective, overlap=job == "map_update")
                     for _ in range(3 if job in ("batch3", "batch_two") else 1)]
        self.c = self.ctxs[0]
        self.batch = world.batch(self.ctxs) if len(self.ctxs) == 3 else None
        self.hold = spec.hold

    def prepare(self):
        c, j = self.c, self.job
        if j in ("frame_key", "frame_none"):
            c.odometry_init(j == "frame_key")
            return self._frames(c, JOB_FRAMES[0], c.frame_launch, c.frame_end, True)
        if j == "pmap_frame":
            c.pmap_odometry_init(True)
            return self._frames(c, JOB_FRAMES[0], c.pframe_launch, c.pframe_end, False)
        if j == "pmap_register":
            c.pmap_setup()
            self.results.append(c.pmap_register(1))
            return 0
        for m in self.ctxs:
            m.map_set()
        for m in self.ctxs:
            self._sync_register(m, "short")
        return len(self.ctxs)

    def begin(self):
        c, j = self.c, self.job
        spec = JOBS[j]
        if not spec.spans:
            if j == "register":
                self._sync_register(c, "jump")
            elif j == "pmap_register":
                self.results.append(c.pmap_register(3))
            else:
                self.results.append(Result(getattr(c, {"nns": "nns", "knn": "knn", "map_update": "map_update_cloud"}[j])(), 0))
            return spec.begins
        self.counted = spec.counted
        if j in ("launch_forced", "launch_live"):
            c.launch("jump")
        elif j == "launch_one_row":
            c.launch("one_row")
        elif j == "launch_odd_rows":
            c.launch("odd_rows")
        elif j == "two_last":
            c.launch("jump")
            c.launch("second", last=True)
        elif j in ("frame_key", "frame_none"):
            c.frame_launch(JOB_FRAMES[1])
        elif j == "pmap_frame":
            c.pframe_launch(JOB_FRAMES[1])
        elif j == "batch3":
            self.batch.launch(["jump", "jump_b", "second"])
            self.batch.map_update()
        elif j == "batch_two":
            self.batch.launch(["jump", "jump_b", "second"])
            self.batch.launch(["second", "jump", "jump_b"], last=True)
        elif j == "sharded":
            c.begin("jump")
            for _ in range(2):
                c.pair()
        return spec.begins

    def end(self):
        c, j = self.c, self.job
        if not JOBS[j].spans:
            return 0
        if j == "sharded":
            for _ in range(BEGUN_PAIRS - 2):
                c.pair()
        if j == "two_last":
            self.results.append(c.end())
        if j == "batch_two":
            self.results += self.batch.end()
        self.counted = 0
        if j in ("frame_key", "frame_none"):
            self.results.append(c.frame_end())
        elif j == "pmap_frame":
            self.results.append(c.pframe_end())
        elif self.batch is not None:
            self.results += self.batch.end()
        else:
            self.results.append(c.end())

    def follow(self):
        c, j = self.c, self.job
        if j in ("frame_key", "frame_none"):
            return self._frames(c, (JOB_FRAMES[2],), c.frame_launch, c.frame_end, True)
        if j == "pmap_frame":
            return self._frames(c, (JOB_FRAMES[2],), c.pframe_launch, c.pframe_end, False)
        if j == "pmap_register":
            self.results.append(c.pmap_register(4))
            return 0
        self._sync_register(c, "next")
        return 1


# ---- the runner -------------------------------------------------------------------------------------------------------------------
Solo = namedtuple("Solo", "results snapshot fail")
Tally = namedtuple("Tally", "lead plain")   # registrations of the cell under test that were latched lead / plain


def _close(world, parties):
    for p in parties:
        try:
            p.close()
        except Exception:
            pass
    world.close()


def _drive(world, parties, script, expect_begins, tally):
    """Runs `script` ((who, step), ...) over `parties` {who: party}; raises _Failed(check) at the first check that fails."""
    def tick():
        if world.count() != sum(p.counted for p in parties.values()):
            raise _Failed("count")
    world.tick = tick
    for who, step in script:
        me = parties[who]
        others = [p for k, p in parties.items() if k != who]
        alone = all(p.counted == 0 for p in others)
        before, others_before = me.leads(), [p.leads() for p in others]
        try:
            begun = me.run(step)
        except RigError:
            raise _Failed("scenario-error")
        tick()
        if (who, step) in expect_begins and begun != expect_begins[(who, step)]:
            raise _Failed("scenario-error")
        got = me.leads() - before
        tally[0] += got
        tally[1] += begun - got
        if got != (begun if alone else 0) or [p.leads() for p in others] != others_before:
            raise _Failed("decision")
    if any(p.fallbacks() for p in parties.values()):
        raise _Failed("timeouts")


def _held_ok(party):
    if party.hold is None:
        return True
    short, held = party.hold
    return party.results[held].iterations >= party.results[short].iterations + 3


def run_solo(make_world, kind, name, cache):
    """The solo twin: the party's own steps on a fresh world with nobody beside it, held to the same checks."""
    key = (kind, name)
    if key not in cache:
        world = make_world()
        party = PartyA(world, name) if kind == "a" else PartyB(world, name)
        steps = ("prepare", "enter", "finish", "follow") if kind == "a" else ("prepare", "begin", "end", "follow")
        fail = results = snap = None
        try:
            _drive(world, {kind: party}, [(kind, s) for s in steps], {}, [0, 0])
            results, snap = list(party.results), party.snapshot()
            if not _held_ok(party):
                fail = "precondition-held"
        except _Failed as e:
            fail = str(e)
        finally:
            _close(world, [party])
        if fail is None and world.count() != 0:
            fail = "count"
        cache[key] = Solo(results, snap, fail)
    return cache[key]


def run_cell(make_world, state, job, order, cache=None, tally=None):
    """Holds one cell: A in `state`, B running `job` beside it, finished in `order`.  Returns [] or [the first check that failed]."""
    cache = {} if cache is None else cache
    tally = [0, 0] if tally is None else tally
    twins = {"a": run_solo(make_world, "a", state, cache), "b": run_solo(make_world, "b", job, cache)}
    for t in twins.values():
        if t.fail:
            return [t.fail]
    world = make_world()
    parties = {"a": PartyA(world, state), "b": PartyB(world, job)}
    expect = {("a", "enter"): STATES[state].begins, ("b", "begin"): JOBS[job].begins}
    fail, got = None, {}
    try:
        _drive(world, parties, ORDERS[order], expect, tally)
        got = {k: (list(p.results), p.snapshot()) for k, p in parties.items()}
    except _Failed as e:
        fail = str(e)
    finally:
        _close(world, list(parties.values()))
    if fail:
        return [fail]
    if world.count() != 0:
        return ["count"]
    for who, party in parties.items():
        results, snap = got[who]
        twin = twins[who]
        held = party.hold[1] if party.hold else None
        if held is not None and results[held].iterations < results[party.hold[0]].iterations + 3:
            return ["precondition-held"]
        if held is not None and results[held] != twin.results[held]:
            return ["latched"]
        if results != twin.results or snap != twin.snapshot:
            return ["bits"]
    return []


# ---- one sequence outside the matrix: lead, plain, plain, lead, plain, lead on one mailbox ---------------------------------------------
ALTERNATION = (True, False, False, True, False, True)
ALT_SCANS = ("short", "jump", "second", "next", "jump_b", "short")


def run_alternation(make_world):
    """One context X registers six scans, each from "last" behind the first, while a neighbour N is begun and collected so that X's
    registrations are latched lead, plain, plain, lead, plain, lead — with two results of X pending beside N in between.  Returns
    [] or the first failing check: decision (the pattern read back through leads()), count, bits (against the same six alone)."""
    def sequence(with_neighbour):
        world = make_world()
        x, n = world.context(False), (world.context(False) if with_neighbour else None)
        out, pattern, fail = [], [], None
        state = {"x": 0, "n": 0}

        def tick():
            if world.count() != state["x"] + state["n"]:
                raise _Failed("count")
        world.tick = tick

        def launch(k):
            before = x.leads()
            state["x"] = 1
            x.launch(ALT_SCANS[k], last=k > 0)
            pattern.append(x.leads() - before == 1)

        def end(last_of_x):
            if last_of_x:
                state["x"] = 0
            out.append(x.end())

        def n_launch():
            if n is not None:
                state["n"] = 1
                n.launch("jump")

        def n_end():
            if n is not None:
                state["n"] = 0
                n.end()
        try:
            x.map_set()
            if n is not None:
                n.map_set()
            launch(0)            # lead: alone
            n_launch()
            launch(1)            # plain: N is pending (X holds two results beside it)
            end(False)
            launch(2)            # plain
            end(False)
            n_end()
            end(True)
            launch(3)            # lead: N has left
            end(True)
            n_launch()
            launch(4)            # plain
            n_end()
            end(True)
            launch(5)            # lead
            end(True)
            snap = x.snapshot()
            if x.fallbacks() or (n is not None and n.fallbacks()):
                fail = "timeouts"
        except _Failed as e:
            fail, snap = str(e), None
        except RigError:
            fail, snap = "scenario-error", None
        finally:
            _close(world, [c for c in (x, n) if c is not None])
        if fail is None and world.count() != 0:
            fail = "count"
        return out, snap, pattern, fail
    alone, beside = sequence(False), sequence(True)
    for run in (alone, beside):
        if run[3]:
            return [run[3]]
    if alone[2] != [True] * 6 or beside[2] != list(ALTERNATION):
        return ["decision"]
    if alone[:2] != beside[:2]:
        return ["bits"]
    return []


# ---- the life cycle of the count: every way a registration can end ----------------------------------------------------------------------
ENDINGS = ("collected", "invalid_jacobian", "launch_refused_empty_map", "batch_fails_at_last_member", "batch_option_mismatch",
           "batch_closed_pending", "closed_one_pending", "closed_two_pending", "frame_dropped", "begun_destroyed")


def run_ending(make_world, ending):
    """`world.ending(name, expect)` makes the registration end that way (expect(n): the count the rule gives at that point);
    afterwards the count is 0 and a fresh context's next registration is lead.  Returns [] or the first failing check."""
    world = make_world()
    fresh = None

    def expect(n):
        if world.count() != n:
            raise _Failed("count")
    try:
        world.ending(ending, expect)
        expect(0)
        fresh = world.context(False)
        fresh.map_set()
        before = fresh.leads()
        fresh.launch("short")
        expect(1)
        fresh.end()
        expect(0)
        if fresh.leads() - before != 1:
            raise _Failed("decision")
    except _Failed as e:
        return [str(e)]
    except RigError:
        return ["scenario-error"]
    finally:
        _close(world, [fresh] if fresh is not None else [])
    return [] if world.count() == 0 else ["count"]


# ---- the toy: the count and the two decisions, restated -------------------------------------------------------------------------------
# A registration's iteration k is worth hash((scan, k, the pose it started from, map version)); a chunk that runs on lead launches
# takes its first pose from the MAILBOX and publishes every pose there, a plain chunk takes it from the state and publishes none:
# whoever re-takes the decision between two chunks reads a stale pose.
NEED = {"short": 3, "jump": 9, "jump_b": 8, "second": 7, "next": 5, "one_row": 4, "odd_rows": 6}
FORCED, LIVE_MAX = 8, 15
FAULTS = ("per_chunk", "leak_on_error", "left_at_destroy", "leave_while_pending", "batch_strangers", "batch_ignores_older",
          "decision_before_enter", "projective_counted")
# the check each wrong copy is meant for
MEANT = {"per_chunk": "latched", "leak_on_error": "count", "left_at_destroy": "count", "leave_while_pending": "count",
         "batch_strangers": "decision", "batch_ignores_older": "decision", "decision_before_enter": "decision",
         "projective_counted": "count"}


class _Reg:
    def __init__(self, scan, cap, need, pose):
        self.scan, self.cap, self.need, self.pose, self.enq, self.out, self.lead = scan, cap, min(need, cap), pose, 0, [], False
        self.chunks = False  # enqueued by icp_register_launch: in chunks, each of which asks lead_latched

    def final(self):
        return self.out[self.need - 1]


class ToyContext:
    def __init__(self, world, live, projective=False, overlap=False):
        self.w, self.live, self.projective = world, live, projective
        self.in_registration, self.pending, self.counted, self.lead_count = False, [], False, 0
        self.last_iterations, self.map_version, self.mailbox, self.last_reg = 0, 0, None, None
        self.begun, self.frame_index, self.frame_key, self.frame, self.batch_hold, self.closed = None, 0, True, False, False, False

    # -- the count
    def _enter(self):
        if not self.counted:
            self.w.g_registering += 1
            self.counted = True

    def _leave(self):
        if self.counted:
            self.w.g_registering -= 1
            self.counted = False

    def _guard(self):
        """RegisteringGuard: on the way out of an entry point"""
        pending = self.pending and self.w.fault != "leave_while_pending"
        if not self.in_registration and not pending:
            self._leave()

    def _shared(self):
        return self.w.g_registering > (1 if self.counted else 0)

    # -- a registration
    def _begin(self, scan, last=False, kd=True, own_answer=True):
        cap = LIVE_MAX if self.live else FORCED
        need = NEED[scan] if self.live else cap
        # ("last": the device-resident pose at the end of the registration before — all of it is enqueued, the callers flush first)
        pose = self.last_reg.final() if last else "identity"
        reg = _Reg(scan, cap, need, pose)
        self.last_reg = reg
        self.mailbox = pose
        if kd or self.w.fault == "projective_counted":
            if self.w.fault == "decision_before_enter":
                shared = self.w.g_registering > 1  # (written as if this context were counted already)
                self._enter()
            else:
                self._enter()
                shared = self._shared()
            if kd and own_answer:
                reg.lead = not shared
                self.lead_count += reg.lead
        self.in_registration = True
        return reg

    def _enqueue(self, reg, count, lead=None):
        lead = reg.lead if lead is None else lead
        if reg.chunks and self.w.fault == "per_chunk":
            lead = not self._shared()
        pose = self.mailbox if lead else reg.pose
        for _ in range(count):
            if reg.enq >= reg.cap:
                break
            pose = hash((reg.scan, reg.enq, pose, self.map_version))
            reg.out.append(pose)
            reg.enq += 1
        reg.pose = pose
        if lead:
            self.mailbox = pose

    def _flush(self):
        if self.pending:
            self._enqueue(self.pending[-1], LIVE_MAX)

    def _result(self, reg):
        self.last_iterations = reg.need
        return Result(tuple(reg.out[:reg.need]), reg.need)

    def _hand_over(self, reg, first):
        self._enqueue(reg, first)
        self.pending.append(reg)
        self.in_registration = False

    def _tick(self):
        self.w.tick()

    def map_set(self):
        self.map_version = 1
        self._tick()

    def register(self, scan):
        reg = self._begin(scan)
        self._enqueue(reg, reg.cap, lead=False)  # (the host polls: no lead launches)
        self.in_registration = False
        self._guard()
        self._tick()
        return self._result(reg)

    def launch(self, scan, last=False, kd=True):
        try:
            if len(self.pending) >= 2:
                raise RigError("two results are already pending")
            if self.map_version == 0:
                raise RigError("the local map is empty")
            self._flush()
            reg = self._begin(scan, last, kd)
            reg.chunks = kd
            self._hand_over(reg, self.last_iterations + 1 if (self.live and kd) else reg.cap)
        finally:
            self._guard()
            self._tick()

    def end(self):
        try:
            if self.begun is not None and not self.pending:
                reg, self.begun, self.in_registration = self.begun, None, False
            elif self.pending:
                reg = self.pending[0]
                if len(self.pending) == 1:
                    while reg.enq < reg.need:
                        self._enqueue(reg, 4)
                self.pending.pop(0)
            else:
                raise RigError("no registration to collect")
            return self._result(reg)
        finally:
            self._guard()
            self._tick()

    def begin(self, scan):
        self.begun = self._begin(scan)
        self._tick()

    def pair(self):
        self._enqueue(self.begun, 1, lead=False)
        self._tick()
        self._tick()

    # -- frames (the kd-tree pair counts, the projective pair does not)
    def odometry_init(self, key):
        self.frame_index, self.frame_key, self.map_version = 0, key, 0
        self._tick()

    pmap_odometry_init = odometry_init

    def _frame_launch(self, k, kd):
        if self.frame_index > 0:
            self.launch("jump" if k in (FRAME_JUMP, JOB_FRAMES[1]) else "next", kd=kd)
        else:
            self._tick()
        self.frame = True

    def _frame_end(self, kd):
        res = Result((), 0)
        if self.frame_index > 0:
            res = self.end()
        else:
            self._tick()
        self.frame = False
        self.map_version = hash((self.map_version, self.frame_key, res.bits[-1:] if res.bits else None))
        self.frame_index += 1
        return Result(res.bits + (self.frame_key,), res.iterations)

    def frame_launch(self, k):
        self._frame_launch(k, True)

    def frame_end(self):
        return self._frame_end(True)

    def pframe_launch(self, k):
        self._frame_launch(k, False)

    def pframe_end(self):
        return self._frame_end(False)

    def pmap_setup(self):
        self.map_version = 1
        self._tick()

    def pmap_register(self, k):
        self.launch("next" if k != 3 else "jump", kd=False)
        return self.end()

    def pmap_launch(self, k):
        self.launch("jump", kd=False)

    # -- calls that register nothing
    def nns(self):
        self._tick()
        return hash((self.map_version, "nns"))

    def knn(self):
        self._tick()
        return hash((self.map_version, "knn"))

    def map_update_cloud(self):
        self.map_version = hash((self.map_version, "cloud"))
        self._tick()
        return self.map_version

    def leads(self):
        return self.lead_count

    def fallbacks(self):
        return 0

    def snapshot(self):
        return self.map_version

    def close(self):
        if not self.closed and self.w.fault != "left_at_destroy":
            self._leave()
        self.closed = True


class ToyBatch:
    def __init__(self, world, members):
        self.w, self.members, self.regs, self.lead = world, members, [], False

    def _flush(self):
        for m, reg in self.regs:
            m._enqueue(reg, LIVE_MAX, lead=self.lead)
            m.batch_hold = False

    def launch(self, scans, last=False, bad_member=None):
        self._flush()
        entered, regs = 0, []
        for i, (m, scan) in enumerate(zip(self.members, scans)):
            if len(m.pending) >= 2:
                raise RigError("two results are already pending")
            was = m.counted
            regs.append((m, m._begin(scan, last, own_answer=False)))
            entered += not was
            if bad_member == i:  # (an error exit behind the members' begins: BatchUnwind)
                for x in self.members:
                    x.in_registration = False
                    if not x.pending and self.w.fault != "leak_on_error":
                        x._leave()
                self.w.tick()
                raise RigError("batched registration: refused at its last member")
        counted = sum(m.counted for m in self.members)
        if self.w.fault == "batch_ignores_older":
            counted = entered
        self.lead = self.w.g_registering <= (1 if self.w.fault == "batch_strangers" else counted)
        live = self.members[0].live
        first = max(m.last_iterations for m in self.members) + 1 if live else FORCED
        for m, reg in regs:
            reg.lead = self.lead
            m.lead_count += self.lead
            m._enqueue(reg, first, lead=self.lead)
            m.pending.append(reg)
            m.in_registration = False
            m.batch_hold = live
        self.regs = regs
        self.w.tick()

    def map_update(self):
        self._flush()
        for m, reg in self.regs:
            m.map_version = hash((m.map_version, reg.final()))
        self.w.tick()

    def end(self):
        out = []
        for m in self.members:
            reg = m.pending[0]
            if len(m.pending) == 1:
                while reg.enq < reg.need:
                    m._enqueue(reg, 4, lead=self.lead)
            m.pending.pop(0)
            m.batch_hold = False
            out.append(m._result(reg))
            m._guard()
        self.regs = [(m, r) for m, r in self.regs if r in m.pending]
        self.w.tick()
        return out

    def close(self):
        for m in self.members:
            m.batch_hold = False


class ToyWorld:
    def __init__(self, fault=None):
        self.fault, self.g_registering, self.tick = fault, 0, lambda: None

    def context(self, live, projective=False, overlap=False):
        return ToyContext(self, live, projective, overlap)

    def batch(self, contexts):
        return ToyBatch(self, contexts)

    def count(self):
        return self.g_registering

    def close(self):
        pass

    def ending(self, name, expect):
        def ready(n=1):
            cs = [self.context(False) for _ in range(n)]
            for c in cs:
                c.map_set()
            return cs
        if name in ("collected", "invalid_jacobian"):
            c, = ready()
            c.launch("short")
            expect(1)
            c.end()
            c.close()
        elif name == "launch_refused_empty_map":
            c = self.context(False)
            try:
                c.launch("short")
            except RigError:
                pass
            expect(0)
            c.close()
        elif name in ("batch_fails_at_last_member", "batch_option_mismatch"):
            cs = ready(3)
            b = self.batch(cs)
            try:
                b.launch(["short"] * 3, bad_member=2)
            except RigError:
                pass
            expect(0)
            b.close()
            for c in cs:
                c.close()
        elif name == "batch_closed_pending":
            cs = ready(3)
            b = self.batch(cs)
            b.launch(["short"] * 3)
            expect(3)
            b.close()
            expect(3)  # (the members' results stand: collected one by one)
            for k, c in enumerate(cs):
                c.end()
                expect(2 - k)
            for c in cs:
                c.close()
        elif name in ("closed_one_pending", "closed_two_pending"):
            c, = ready()
            c.launch("short")
            if name == "closed_two_pending":
                c.launch("jump", last=True)
            expect(1)
            c.close()
        elif name == "frame_dropped":
            c = self.context(False)
            c.odometry_init(True)
            c.frame_launch(0)
            c.frame_end()
            c.frame_launch(1)
            expect(1)
            c.end()               # (icp_odometry_init drops the launched frame: it collects the registration)
            c.odometry_init(True)
            expect(0)
            c.close()
        elif name == "begun_destroyed":
            c, = ready()
            c.begin("short")
            expect(1)
            c.close()
        else:
            raise RigError(name)


def toy_world(fault=None):
    return lambda: ToyWorld(fault)
