"""CPU (`-m "not gpu"`): the bit model of the kd-tree local map (tests/map_lifecycle.py) on its own.  The evidence that the
device tests of tests/test_gpu_map_lifecycle.py bite:

  * the model has the bits of the reference's own KdTreeLocalMap after EVERY operation of the recorded scripts
    (tests/golden/map_lifecycle.npz, oracle/make_golden_map_lifecycle.py) and of `mu_final` (components.npz), counts
    included — no pose of the scripts had to be replaced: float64 Gauss-Jordan and np.linalg.inv round to the same float32
    inverse on all of them;
  * it stays inside the derived float64 bound on every script (worst ratio measured: 0.63 of 5 x 2^-24 per move);
  * each deliberately wrong copy of it — or of a recorded state — fails the check meant for it, and the fma-contracted
    move fails the bits ONLY: it passes the float64 bound, which is the point of a bit check;
  * the loop of the device tests itself — every operation through its entry point, check_state, check_search,
    check_registration — runs clean on a context that answers from the oracle, and stops at a wrong copy of the update;
  * the maps of the scripts let the search and the normals be judged: ties among the probes stay below the mismatch cap and
    more than half of the neighbourhoods are determined, by the model's values alone.
"""
import os

import numpy as np
import pytest

import iteration_audit as A
import map_lifecycle as L
from conftest import GOLDEN

F32, F64 = np.float32, np.float64


@pytest.fixture(scope="module")
def recording():
    return np.load(os.path.join(GOLDEN, "map_lifecycle.npz"))


class StateContext:
    """What check_state reads of an IcpContext, answered by a model (a wrong one) or by a recorded state."""

    def __init__(self, points, counts):
        self.points, self.counts = np.asarray(points, F32), list(counts)

    def map_size(self):
        return len(self.points)

    def map_num_clouds(self):
        return len(self.counts)

    def map_points(self):
        return self.points.copy()


def _failures(name, mutant, ops=None):
    """The script through the model and a wrong copy of it side by side: [(operation, failed check)] of check_state."""
    s = L.script(name)
    good, bad = L.MapModel(s.local_map_size), L.MapModel(s.local_map_size, mutant)
    out = []
    for i, op in enumerate(ops or s.ops):
        L.apply(good, op)
        ins = L.apply(bad, op)
        try:
            L.check_state(StateContext(bad.map, bad.counts), good, f"{name} op {i}", ins)
        except AssertionError as e:
            msg = str(e)
            print(msg[:300])
            out.append((i, msg[1:msg.index("]")]))
    return out


# ----------------------------------------------------------------------------------------------------------------------
def test_model_equals_mu_final(golden_components):
    g = golden_components
    m = L.MapModel(2)
    c, rel = g["mu_clouds"], g["mu_rel"]
    m.update(np.eye(4), c[0])
    m.update(rel, c[1])
    m.update(rel)
    m.update(rel, c[2])
    m.update(rel, c[3])
    assert m.counts == list(g["mu_counts"])
    assert L.first_difference(m.map, g["mu_final"]) is None, L.first_difference(m.map, g["mu_final"])


@pytest.mark.parametrize("name", L.RECORDED)
def test_model_equals_the_recording(recording, name):
    """Bit for bit after every operation, counts too; the recording passes check_state as a device would."""
    s = L.script(name)
    m = L.MapModel(s.local_map_size)
    for i, op in enumerate(s.ops):
        L.apply(m, op)
        ctx = StateContext(recording[f"{name}_map_{i}"], recording[f"{name}_counts_{i}"])
        assert m.counts == ctx.counts, (name, i, m.counts, ctx.counts)
        L.check_state(ctx, m, f"{name} op {i} ({op.note})")
    assert i == len(s.ops) - 1 and f"{name}_map_{i + 1}" not in recording.files


def test_scripts_hold_what_they_claim():
    w = L.script("window")
    sizes = [len(op.cloud) for op in w.ops if op.cloud is not None]
    assert len(w.ops) == 14 and {0, 1, 255, 256, 257, 1639} <= set(sizes)
    st = L.states("window")
    assert [c for _, c, _ in st][4] == [1, 255, 256] and st[5][1] == [255, 256, 0] and st[8][1] == [256, 0, 0]
    assert st[8][2] == 0 and st[9][2] == 576 and st[10][2] == 560  # all NaN; 24 NaN rows; 24 NaN and 16 null rows
    assert (st[9][0] == 0).all(axis=1).sum() == 16 and np.signbit(st[9][0]).any(axis=1)[(st[9][0] == 0).all(axis=1)].any()
    assert not np.array_equal(w.ops[0].rel, np.eye(4, dtype=F32))
    one = L.states("window_one")
    assert [len(m) for m, _, _ in one] == [600, 513, 513, 0, 0, 400, 400, 257] and all(len(c) == 1 for _, c, _ in one)
    su = L.states("set_then_update")
    assert [len(m) for m, _, _ in su] == [3000, 3400, 3656, 3756, 0, 600, 900] and su[0][1] == [] and su[3][1] == [256, 500]
    fixed = L.script("set_then_update").ops[0].cloud
    assert L.first_difference(su[1][0][:3000], L.move(L.invert4(L.script("set_then_update").ops[1].rel), fixed)) is None
    d = L.script("drift")
    assert sum(op.cloud is None for op in d.ops) == 40 and d.ops[-1].register == 3
    assert max(len(m) for n in L.SCRIPTS for m, _, _ in L.states(n)) <= 6000


@pytest.mark.parametrize("name", L.SCRIPTS)
def test_model_inside_its_float64_bound(name):
    """Measured worst ratios: window 0.61, window_one 0.53, set_then_update 0.63, drift 0.54 (of 5 x 2^-24 per move)."""
    s = L.script(name)
    m = L.MapModel(s.local_map_size)
    worst = 0.0
    for op in s.ops:
        L.apply(m, op)
        worst = max(worst, m.check_against_float64())
    print(f"{name}: worst |model - float64 shadow| / bound {worst:.3f}")
    assert 0.0 < worst <= 1.0


def test_per_move_error_and_inverse_on_random_poses():
    """200 random poses: Gauss-Jordan and np.linalg.inv of the float32 matrix round to the same float32 inverse; one move
    stays inside 5 x 2^-24 (|R^-1||p| + |t^-1|); the fma-contracted move differs in bits on every pose and stays inside too."""
    rng = np.random.default_rng(11)
    pts = (rng.normal(size=(2000, 3)) * [20, 15, 3]).astype(F32)
    worst, share = 0.0, []
    for _ in range(200):
        rel = A.O.build_pose_matrix(np.concatenate([rng.normal(0, 0.5, 3), rng.uniform(-0.3, 0.3, 3)]).astype(F32)).astype(F32)
        inv = L.invert4(rel)
        assert np.array_equal(inv.view(np.uint32), np.linalg.inv(rel).view(np.uint32))
        i64 = np.linalg.inv(rel.astype(F64))
        exact = pts.astype(F64) @ i64[:3, :3].T + i64[:3, 3]
        bound = 5.0 * 2.0 ** -24 * (np.abs(pts.astype(F64)) @ np.abs(i64[:3, :3]).T + np.abs(i64[:3, 3]))
        a, b = L.move(inv, pts), L.move_fma(inv, pts)
        worst = max(worst, float((np.abs(a - exact) / bound).max()), float((np.abs(b - exact) / bound).max()))
        share.append(float((a.view(np.uint32) != b.view(np.uint32)).mean()))
    print(f"worst per-move error {worst * 5:.2f} x 2^-24; fma differs in {min(share) * 100:.1f} .. {max(share) * 100:.1f} % of "
          f"the coordinates")
    assert worst <= 1.0 and min(share) > 0.05


def test_singular_pose_is_refused_by_the_model():
    rel = np.eye(4, dtype=F32)
    rel[2] = 0
    assert L.invert4(rel) is None
    m = L.MapModel(3)
    m.update(np.eye(4), np.ones((4, 3), F32))
    before = m.map.copy()
    assert m.update(rel, np.ones((2, 3), F32)) is None and np.array_equal(m.map, before) and m.counts == [4]


# ---- each check fails the wrong copy meant for it ---------------------------------------------------------------------
def test_eviction_from_the_back_fails_the_bits():
    f = _failures("window", "evict_back")
    assert f[0] == (4, "map bits")  # the first eviction: the same size, other rows


def test_popping_the_new_count_fails_the_size():
    f = _failures("window", "pop_new_count")
    assert f[0] == (4, "map size")


def test_uncounted_zero_row_cloud_fails_num_clouds_then_the_map():
    """In `window` the 0-row cloud fills the window, so the size gives it away at once; in a window that is not yet full
    only num_clouds does — and the map one update later."""
    assert _failures("window", "zero_cloud_uncounted")[0] == (5, "map size")
    w = L.script("window").ops
    f = _failures("window", "zero_cloud_uncounted", ops=[w[0], w[1], w[5], w[3]])
    assert f == [(2, "num clouds"), (3, "map size")]


def test_counted_map_set_fails_the_size():
    """num_clouds gives it away at once; the size within three updates: counted, the 3000 `map_set` points leave as one
    cloud at the second insertion — as the reference has it, 400 of them leave at the third."""
    f = _failures("set_then_update", "set_counted")
    assert f[:2] == [(0, "num clouds"), (1, "num clouds")] and (2, "map size") in f and (3, "map size") in f


def test_moved_first_cloud_fails_the_bits():
    assert _failures("window", "first_cloud_moved")[0] == (0, "map bits")


def test_uninverted_pose_fails_the_bits():
    assert _failures("window", "rel_not_inverted")[0] == (1, "map bits")


def test_transposed_rotation_fails_bits_and_bound():
    assert _failures("window", "rotation_transposed")[0] == (1, "map bits")
    s = L.script("window")
    bad = L.MapModel(3, "rotation_transposed")
    with pytest.raises(AssertionError, match="float64 shadow"):
        for op in s.ops:
            L.apply(bad, op)
            bad.check_against_float64()


def test_fma_contracted_move_fails_the_bits_only():
    for name in L.SCRIPTS:
        f = _failures(name, "fma_move")
        assert f and {c for _, c in f} == {"map bits"}, (name, f[:3])
        s = L.script(name)
        bad = L.MapModel(s.local_map_size, "fma_move")
        worst = 0.0
        for op in s.ops:
            L.apply(bad, op)
            worst = max(worst, bad.check_against_float64())  # PASSES: a tolerance would not notice
        print(f"{name}: fma-contracted move at {worst:.3f} of the float64 bound, first bit difference at op {f[0][0]}")
        assert worst <= 1.0


def test_kept_nan_row_fails_the_size():
    assert _failures("window", "nan_row_kept")[0] == (8, "map size")


def test_kept_null_row_fails_the_size():
    assert _failures("window", "null_row_kept")[0] == (10, "map size")


def test_vertex_map_threshold():
    """A pixel of norm exactly float32(0.01) is dropped (`>`), 0.0101 kept, 0.0099 and NaN dropped."""
    v = np.zeros((3, L.H, L.W), F32)
    v[0, 3, 5] = F32(0.01)  # sqrt(fl(x x)) == x
    v[1, 4, 6] = F32(0.0101)
    v[2, 5, 7] = F32(0.0099)
    v[:, 6, 8] = (1.0, np.nan, 2.0)
    v[:, 2, 9] = (3.0, 4.0, 5.0)
    assert np.sqrt(v[0, 3, 5] * v[0, 3, 5]) == L.VMAP_THRESHOLD
    good, bad = L.MapModel(3), L.MapModel(3, "vmap_threshold_ge")
    assert good.update_vertex_map(np.eye(4), v) == 2 and bad.update_vertex_map(np.eye(4), v) == 3
    assert np.array_equal(good.map, np.array([[3, 4, 5], [0, 0.0101, 0]], F32))  # row-major pixel order
    with pytest.raises(AssertionError, match=r"\[map size\]"):
        L.check_state(StateContext(bad.map, bad.counts), good, "vertex map", 3)


def _recorded_search(recording, step):
    """(map of the MODEL at the step, probes, recorded neighbour index, recorded normals, NormalReference)."""
    first_row = dict(L.RECORDED_SEARCH)[step]
    m = L.states("window")[step][0]
    probes = L.displaced_probes(m, seed=step, first_row=first_row)
    return m, probes, recording[f"window_search_ix_{step}"], recording[f"window_search_normals_{step}"], A.NormalReference(m)


def test_recorded_search_passes(recording):
    for step, _ in L.RECORDED_SEARCH:
        m, probes, ix, nm, nref = _recorded_search(recording, step)
        fig = L.verify_search(f"window op {step}", m, probes, m[ix], nm, ix, nref)
        print(step, {k: v for k, v in fig.items()})
        assert fig["mismatches"] == 0 and fig["clear"] > fig["used"] // 2


def test_shifted_neighbour_index_fails_the_search(recording):
    """One index left at its value from before the eviction (index, not index - evicted)."""
    m, probes, ix, nm, nref = _recorded_search(recording, 4)
    evicted = 1639
    stale = ix.copy()
    stale[7] += evicted
    with pytest.raises(AssertionError, match="outside the map"):
        L.verify_search("stale", m, probes, None, nm, stale, nref)
    wrapped = ix.copy()
    wrapped[7] = (ix[7] + evicted) % len(m)
    with pytest.raises(AssertionError, match="not the nearest map point"):
        L.verify_search("wrapped", m, probes, None, nm, wrapped, nref)
    with pytest.raises(AssertionError, match="neighbor_points are not the model's points"):
        L.verify_search("points", m, probes, m[ix], nm, wrapped, nref)


def test_normal_from_before_the_update_fails_the_normals(recording):
    """The normals the reference held BEFORE the first eviction left in place for the rows that survived it (old index =
    index + evicted): the map turned with the pose, they did not."""
    m, probes, ix, nm, nref = _recorded_search(recording, 4)
    ix_before, nm_before = recording["window_search_ix_3"], recording["window_search_normals_3"]
    before = {int(i): n for i, n in zip(ix_before, nm_before)}
    stale, swapped = nm.copy(), 0
    for r, i in enumerate(ix):
        old = int(i) + 1639
        if i < 256 and old in before:
            stale[r] = before[old]
            swapped += 1
    print(f"{swapped} of {len(ix)} probes take the normal of before the update")
    assert swapped >= 100
    with pytest.raises(AssertionError, match="determined normals beyond"):
        L.verify_search("stale normals", m, probes, None, stale, ix, nref)


# ---- census: conditions on the inputs, from the model alone ----------------------------------------------------------------
@pytest.mark.parametrize("name", L.SCRIPTS)
def test_census(name):
    """Behind every operation at which the device test searches: the share of probes whose two nearest float64 distances
    tie within TIE_RTOL stays below MISMATCH_CAP (measured: at most 9.2e-4, one probe), and NormalReference determines more
    than half of the neighbourhoods (measured: at least 97 %)."""
    worst_tie, least_clear = 0.0, 1.0
    for i, (m, counts, _) in enumerate(L.states(name)):
        if not L.searched(name, i) or not len(m):
            continue
        nref = A.NormalReference(m)
        tie = L.tie_census(m, L.search_probes(m, i), nref.tree)
        used = np.unique(A.lowest_index_of_equal_points(m))
        nref.need(used)
        clear = float(nref.clear[used].mean())
        worst_tie, least_clear = max(worst_tie, tie), min(least_clear, clear)
        assert tie < A.MISMATCH_CAP, (name, i, tie)
        assert clear > 0.5, (name, i, clear)
    print(f"{name}: tie share <= {worst_tie:.2e}, determined neighbourhoods >= {least_clear * 100:.1f} %")


def test_census_of_the_plane_map():
    """The plane map of the refusal test, under the seeds of its two searches."""
    rel, clouds = L.plane_inputs()
    m = L.MapModel(3)
    for c in clouds:
        m.update(rel, c)
    assert not m.map[:, 2].any() and len(m) == 4096
    nref = A.NormalReference(m.map)
    nref.need(np.arange(len(m)))
    assert nref.clear.mean() > 0.5
    for seed in L.PLANE_SEEDS:
        assert L.tie_census(m.map, L.search_probes(m.map, seed), nref.tree) < A.MISMATCH_CAP


# ---- the device harness itself, on a context that answers from the oracle ------------------------------------------------
class OracleMapContext:
    """The map calls of `IcpContext` the device tests make, answered on the CPU: the update by a MapModel of its own (or a
    wrong copy), the search by a kd-tree with the lowest index of equal points, the normals by O.knn_normals."""

    def __init__(self, local_map_size, k=10, mutant=None):
        from types import SimpleNamespace
        self.m, self.staged = L.MapModel(local_map_size, mutant), None
        self.pose = self.pending = self.done = self.last = None
        self.alignment = (L.SCHEME, L.SIGMA, L.K_REG)
        self.config = SimpleNamespace(num_neighbors_normals=k)

    def set_option(self, name, value):
        pass

    def map_init(self):
        self.m.init()

    def map_set(self, points):
        self.m.set(points)

    def _update(self, rel, cloud, skip_null):
        if rel is None:
            if self.pose is None and self.pending is None:
                raise AssertionError("rel_pose = NULL needs a previous registration on this context")
            if self.pending is not None and cloud is not None:
                raise AssertionError("rel_pose = NULL with a new cloud: collect the pending registration first")
            if self.pending is not None:  # enqueued behind the registration: it reads the pose that registration ends with
                self.pose = self._registration(*self.pending).pose
            rel = self.pose
        ins = self.m.update(rel, cloud, skip_null)
        if ins is None:
            raise AssertionError("singular relative pose")
        return ins

    def map_update(self, rel, cloud=None, skip_null=False):
        return self._update(rel, cloud, skip_null)

    # ---- registration: the oracle's own loop on the map as it stands (iteration_audit.oracle_records)
    def set_alignment(self, scheme, sigma, max_num_alignments, threshold_delta_pose):
        assert threshold_delta_pose == 0.0
        self.alignment = (scheme, sigma, int(max_num_alignments))

    def _registration(self, points, init, skip_null):
        from types import SimpleNamespace
        if self.done is None:
            scheme, sigma, k = self.alignment
            m = self.m.map
            recs = A.oracle_records(points, m, A.oracle_normals(m, self.config.num_neighbors_normals),
                                    np.eye(4, dtype=F32) if init is None else init, k, scheme, sigma, skip_null=skip_null)
            assert all(r.status == A.ICP_OK for r in recs)
            self.last = recs[-1]
            self.done = SimpleNamespace(iterations=len(recs), losses=np.array([r.loss for r in recs]),
                                        dx=np.stack([r.dx for r in recs]), num_targets=recs[-1].num_targets,
                                        converged=recs[-1].converged, pose=recs[-1].pose_after.copy())
        return self.done

    def register(self, points, init_pose=None, skip_null=False):
        self.done = None
        res = self._registration(points, init_pose, skip_null)
        self.pose = res.pose
        return res

    def register_launch(self, points, init_pose=None, skip_null=False):
        self.pending, self.done = (points, init_pose, skip_null), None

    def register_end(self):
        res = self._registration(*self.pending)
        self.pending, self.pose = None, res.pose
        return res

    def last_neighbors(self, n):
        assert len(self.last.ix) == n
        return self.last.ix.astype(np.int32), self.last.pose12.copy()

    def map_stage_cloud(self, cloud, skip_null=False):
        self.staged = (np.array(cloud, F32), skip_null)

    def map_update_staged(self, rel):
        if self.staged is None:
            raise AssertionError("no staged cloud")
        ins = self._update(rel, *self.staged)
        self.staged = None
        return ins

    def map_update_vertex_map(self, rel, vmap):
        return self.m.update_vertex_map(rel, vmap)

    def project(self, points):
        return A.O.build_projection_map(np.asarray(points, F32), L.H, L.W, 3.0, -24.0)

    def map_size(self):
        return len(self.m)

    def map_num_clouds(self):
        return len(self.m.counts)

    def map_points(self):
        return self.m.map.copy()

    def handoff_fallbacks(self):
        return 0

    def close(self):
        pass

    def nearest_neighbor_search(self, points, with_normals=True, with_index=False):
        if not len(self.m):
            raise RuntimeError("the local map is empty")
        self.pose = None  # (as the library: the search re-initialises the state a pose-only update would read)
        m, k = self.m.map, self.config.num_neighbors_normals
        tree = A.cKDTree(m.astype(F64))
        ix = A.lowest_index_of_equal_points(m)[tree.query(np.asarray(points, F64))[1]]
        used = np.unique(ix)
        nm = A.O.knn_normals(m, tree, used, k)[np.searchsorted(used, ix)]
        return m[ix], nm, ix.astype(np.int32)


HARNESS = [(n, e) for e in ("host", "staged", "vertex_map") for n in L.SCRIPTS] + \
          [(n, "device_pose") for n in ("window", "set_then_update")]


@pytest.mark.parametrize("name,entry", HARNESS)
def test_device_harness_on_the_oracle(monkeypatch, name, entry):
    """The loop of tests/test_gpu_map_lifecycle.py (every operation through its entry point, check_state, check_search,
    check_registration at the marks; rel_pose None with its launch / end pair and its refused insertion) runs clean on a
    context that answers from the oracle — and stops at the first operation a wrong copy of the update gets wrong."""
    import test_gpu_map_lifecycle as T
    monkeypatch.setattr(A, "registered", lambda call: (A.ICP_OK, call()))  # (no Invalid Jacobian here: nothing to catch)
    monkeypatch.setattr(T, "_ctx", lambda size, options=(), **kw: OracleMapContext(size, kw.get("num_neighbors_normals", 10)))
    worst = A.Worst(f"{name}/{entry} on the oracle")
    figs = T._run(None, name, entry, worst=worst)
    print(worst)
    assert figs["mismatches"] == 0 and figs["searched"] >= 4
    assert figs["registered"] == sum(op.register is not None for op in L.script(name).ops) >= 1 and worst.n == figs["registered"]
    monkeypatch.setattr(T, "_ctx", lambda size, options=(), **kw: OracleMapContext(size, mutant="fma_move"))
    with pytest.raises(AssertionError, match=r"\[map bits\]"):
        T._run(None, name, entry)
