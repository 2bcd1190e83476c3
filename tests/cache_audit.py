"""What the NN cache's certificates are held to (csrc/search.hip: the cache test of iterate_body and of k_iterate_batch, the
six producers of L), the clouds that aim at the bound, a host restatement of the cache whose switches are the wrong copies
the CPU suite turns on, and the loop the GPU tests run.  TEST INFRASTRUCTURE, never imported by the package.

An entry, as `icp_last_cache_entries` hands it out: a candidate set S of up to three ORIGINAL map indices (the stored
neighbour first), L, and the iteration j of the search.  L is a lower bound on the distance from p_j — the query under the
pose of iteration j, as `transform_point` computes it (search_audit.transform_f32) — to every map point that is not a member
of S.  A later iteration t keeps the entry when
    sqrt(d2_winner) * 1.000001 < L - (|p_t - p_j| * 1.000001 + 1e-7) - margin
and its age t - j is 1 .. CACHE_HIST.  An entry found with iteration j after iteration `last` was kept by every t in (j, last].

The checks (`audit`), on every valid row whose model is certain (unflagged) at every pose it is evaluated at:
  A  sound bound.   L is finite and >= 0, and the nearest map point outside S lies at float64 distance >= L from p_j (float32
                    coordinates; differences, squares and the root in float64).  NO tolerance: L is a float32 distance scaled
                    by 0.999999 (16 * 2^-24), the roundings above it are below 3 * 2^-24.
  B  exact set.     The nearest member of S by the key (bits of d2, index) is the model's neighbour at p_j and at every p_t,
                    t in (j, last]; members are < map size and distinct.
  C  kept => entitled.  For t in (j, last], in float64: d = |winner - p_t|, delta = |p_t - p_j|, c = float32(1.000001):
                    d * c < L - (delta * c + 1e-7) + band, band = 8 * 2^-24 * (d + L + delta) — the device's left side errs by
                    under 4 * 2^-24 * d (three roundings of d2, a 1-ulp root, one product), its right side by under
                    4 * 2^-24 * delta + 2 * 2^-24 * L; the band doubles the sum.  Without refresh_margin: the necessary
                    condition under every option set.  (Under "hit_records" a hit may have been decided from the record: its
                    bound at p_r is at most L - delta(r, j) and its test subtracts delta(t, r) >= delta(t, j) - delta(r, j),
                    with 1e-7 twice — the same necessary condition.)  And last - j <= CACHE_HIST.  (Read from the kernel: a
                    record of age <= CACHE_HIST is tried before its entry and can carry an entry PAST that age; no registration
                    with records runs that long here, and the rule is asserted as it stands.)
  D  records.       The recorded winner has the bits of the model's neighbour at the record's iteration r, every OTHER map point
                    is at float64 distance >= the record's bound from p_r, and last - r <= CACHE_HIST.
The model at a pose is search_audit.model_nn's, evaluated on the candidates a float64 kd-tree names (`model_at`): the float32
d2 of a pair is within 5 * 2^-24 of its float64 square, so the minimum key is among the points whose float64 distance is within
1e-6 of the least; rows where the tree's list does not prove that go to the brute force.
"""
import types

import numpy as np

import knn_audit as K
import search_audit as S

F32 = np.float32
U = 2.0 ** -24
C_UP = F32(1.000001)
C_DOWN = F32(0.999999)
EPS_DELTA = F32(1e-7)
CACHE_HIST = 24
ITER_WRAP = 128
BAND = 8.0 * U
SET_SPREAD = F32(2.0e-3)     # the model producer takes a second and third member within that of the nearest
_TREE_K = 8


# ---- the model at a pose ---------------------------------------------------------------------------------------------
class MapModel:
    """a map with its float64 kd-tree; models and outside distances are kept per pose (option sets share their poses)"""

    def __init__(self, map_pts):
        from scipy.spatial import cKDTree
        self.map = np.ascontiguousarray(map_pts, F32)
        self.m64 = self.map.astype(np.float64)
        self.tree = cKDTree(self.m64)
        self._kept = {}

    def candidates(self, p32, k):
        """(float64 distances [n, k] ascending, indices) of the k float64-nearest map points, the distances recomputed plainly"""
        k = min(k, self.map.shape[0])
        _, idx = self.tree.query(p32.astype(np.float64), k=k)
        idx = idx.reshape(p32.shape[0], k)
        d = np.sqrt(((self.m64[idx] - p32.astype(np.float64)[:, None, :]) ** 2).sum(axis=2))
        order = np.argsort(d, axis=1, kind="stable")
        return np.take_along_axis(d, order, axis=1), np.take_along_axis(idx, order, axis=1)


def pair_d2(pts, p):
    """float32 d2 of `consider`, elementwise: pts [n, k, 3] against p [n, 3]; (d2, unsure)"""
    dx, dy, dz = (pts[..., a] - p[:, None, a] for a in range(3))
    s, f1 = K._fma_sq(dy, dx * dx)
    d2, f2 = K._fma_sq(dz, s)
    return d2, f1 | f2


def _key(d2, idx):
    return (np.ascontiguousarray(d2, F32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | idx.astype(np.uint64)


def model_points(mm, p32):
    """the model's neighbour of already transformed points: K.Knn (dist = sqrt(d2), index, flagged), plus the candidates' keys
    sorted (d2 [n, k], index [n, k]) for the producer of the fake context"""
    n = p32.shape[0]
    d64, idx = mm.candidates(p32, _TREE_K)
    d2, unsure = pair_d2(mm.map[idx], p32)
    order = np.argsort(_key(d2, idx), axis=1)
    d2s, idxs = np.take_along_axis(d2, order, axis=1), np.take_along_axis(idx, order, axis=1)
    best = d2s[:, 0]
    limit = np.nextafter(best, F32(np.inf))
    flagged = np.any(unsure & (d2 <= limit[:, None]), axis=1)
    # a point outside the list lies at >= d64[:, -1]: its float32 d2 is above best when that square, 1e-6 off, still is
    proven = (d64[:, -1] ** 2) * (1.0 - 1.0e-6) > best.astype(np.float64)
    index = idxs[:, 0].astype(np.int32)
    rest = np.flatnonzero(~proven)
    if rest.size:
        w = K.model_knn(mm.map, np.ascontiguousarray(p32[rest]), 1, sqr=True)
        best = best.copy()
        best[rest], index[rest], flagged[rest] = w.dist[:, 0], w.index[:, 0], w.flagged
    with np.errstate(invalid="ignore"):
        return K.Knn(np.sqrt(best)[:, None], index[:, None], flagged), (d2s, idxs, proven)


def model_at(mm, scan, pose12):
    """(p_t [n, 3] float32, K.Knn of the model at that pose), kept per (scan, pose)"""
    scan = np.ascontiguousarray(scan, F32)
    key = ("model", scan.ctypes.data, scan.shape[0], np.ascontiguousarray(pose12, F32).tobytes())
    if key not in mm._kept:
        p, unsure = S.transform_f32(pose12, scan)
        got, _ = model_points(mm, p)
        got.flagged |= unsure
        mm._kept[key] = (scan, p, got)     # (the scan is kept alive: its address is part of the key)
    return mm._kept[key][1:]


def nearest_outside(mm, p32, members):
    """float64 distance [n] from p to the nearest map point that is NOT one of `members` [n, s] (-1: none), and its index"""
    d, idx = mm.candidates(p32, members.shape[1] + 3)
    inside = (idx[:, :, None] == members[:, None, :]).any(axis=2)
    d = np.where(inside, np.inf, d)
    at = np.argmin(d, axis=1)
    r = np.arange(p32.shape[0])
    return d[r, at], idx[r, at]


def nearest_member(mm, p32, members):
    """(index [n] of the nearest member by the key, its float32 d2, the float32 d2 of the nearest OTHER member or inf)"""
    safe = np.clip(members, 0, mm.map.shape[0] - 1)
    d2, _ = pair_d2(mm.map[safe], p32)
    d2 = np.where(members >= 0, d2, F32(np.inf)).astype(F32)
    key = np.where(members >= 0, _key(d2, safe), np.uint64(0xFFFFFFFFFFFFFFFF))
    at = np.argmin(key, axis=1)
    r = np.arange(p32.shape[0])
    others = d2.copy()
    others[r, at] = np.inf
    return members[r, at], d2[r, at], others.min(axis=1)


# ---- the audit -----------------------------------------------------------------------------------------------------------
class Report:
    def __init__(self, what):
        self.what, self.failures = what, []
        self.rows = self.flagged = self.positive = self.aged = self.record_rows = 0
        self.min_slack, self.worst_c, self.kept_share, self.max_age = np.inf, np.inf, [], 0

    def fail(self, check, text):
        self.failures.append(f"check {check}: {self.what}: {text}")

    def line(self):
        share = " ".join(f"{s:.2f}" for s in self.kept_share)
        return (f"{self.what}: {self.rows} rows ({self.flagged} flagged), L > 0 on {self.positive}, aged {self.aged} (oldest "
                f"{self.max_age}), smallest slack of A {self.min_slack:.3g}, C nearest its band {self.worst_c:.3g} bands, "
                f"{self.record_rows} records, kept since before iteration t [{share}]")


def audit(mm, scan, out, what, fine_level=True, raise_on_failure=True):
    """Checks A - D (D where `out` has records) on one read-out against the map of `mm`; returns the Report.  `out`: what
    IcpContext.last_cache_entries returns.  fine_level: no audited row with L > 0 is a failure."""
    rep = Report(what)
    scan = np.ascontiguousarray(scan, F32)
    n, m = scan.shape[0], mm.map.shape[0]
    members = np.asarray(out["members"]).reshape(n, 3).astype(np.int64)
    L32 = np.asarray(out["bound"], F32).reshape(n)
    it = np.asarray(out["iteration"]).reshape(n).astype(np.int64)
    hist, last = np.asarray(out["pose_hist"], F32), int(out["last"])
    assert hist.shape == (last + 1, 3, 4), (what, hist.shape, last)
    L = L32.astype(np.float64)
    valid = it >= 0
    if ((it > last) | (it < -1)).any():
        rep.fail("age", f"an iteration outside -1 .. {last}")
    if (members[~valid] != -1).any() or (L32[~valid] != 0).any():
        rep.fail("B", "a row without an entry has members or a bound")
    # members: the stored neighbour present, every index below the map size, no index twice
    mv = members[valid]
    bad = (mv[:, 0] < 0) | (mv >= m).any(axis=1) | (mv < -1).any(axis=1)
    for a, b in ((0, 1), (0, 2), (1, 2)):
        bad |= (mv[:, a] == mv[:, b]) & (mv[:, a] >= 0)
    if bad.any():
        rep.fail("B", f"{int(bad.sum())} entries with a member out of range or twice, first row {np.flatnonzero(valid)[bad][0]}")
        valid = valid & ~np.isin(np.arange(n), np.flatnonzero(valid)[bad])
    if not (np.isfinite(L32[valid]) & (L32[valid] >= 0)).all():
        rep.fail("A", "L is not finite or negative")
    age = np.where(valid, last - it, 0)
    if (age > CACHE_HIST).any():
        r = int(np.argmax(age))
        rep.fail("age", f"row {r} carries an entry of age {int(age[r])} > {CACHE_HIST}")
    first = int(it[valid].min()) if valid.any() else last
    first = max(first, last - CACHE_HIST - 8)       # (entries beyond the window have failed above; their poses are not needed)
    # the record's iteration
    rec = rr = None
    if "records" in out:
        rec = np.ascontiguousarray(out["records"], F32).reshape(n, 8)
        rr = rec[:, 7].copy().view(np.int32).astype(np.int64)
        rr[~valid] = -1
        if ((rr > last) | ((rr >= 0) & (rr <= it))).any():
            rep.fail("D", "a record that is not younger than its entry, or from the future")
        if (last - rr[rr >= 0] > CACHE_HIST).any():
            rep.fail("D", f"a record of age {int((last - rr[rr >= 0]).max())} > {CACHE_HIST}")
        first = min(first, max(int(rr[rr >= 0].min()), last - CACHE_HIST - 8)) if (rr >= 0).any() else first
    flagged = np.zeros(n, bool)
    P, models = {}, {}
    for t in range(max(first, 0), last + 1):
        P[t], models[t] = model_at(mm, scan, hist[t])
        flagged |= valid & (np.clip(it, 0, None) <= t) & models[t].flagged
    use = valid & ~flagged & (it >= first)
    rep.rows, rep.flagged = int(use.sum()), int((valid & flagged).sum())
    pj = np.zeros((n, 3), F32)
    for t in P:
        pj[it == t] = P[t][it == t]
    rows = np.flatnonzero(use)
    # A: the nearest map point outside S, at the pose of the search
    if rows.size:
        d_out, i_out = nearest_outside(mm, pj[rows], members[rows])
        viol = d_out < L[rows]
        if viol.any():
            r = np.flatnonzero(viol)[0]
            rep.fail("A", f"{int(viol.sum())} of {rows.size} rows: map point {int(i_out[r])} is not in the set of row {int(rows[r])} "
                          f"and lies at {d_out[r]!r} < L = {L[rows][r]!r} (iteration {int(it[rows][r])})")
        pos = L[rows] > 0
        rep.positive = int(pos.sum())
        if pos.any():
            rep.min_slack = float(((d_out[pos] - L[rows][pos]) / d_out[pos]).min())
    rep.aged = int((age[rows] >= 1).sum())
    rep.max_age = int(age[rows].max()) if rows.size else 0
    c = float(C_UP)
    for t in sorted(P):
        at = np.flatnonzero(use & (it <= t))
        rep.kept_share.append(float((use & (it < t)).sum()) / max(rep.rows, 1))
        if not at.size:
            continue
        win, _, _ = nearest_member(mm, P[t][at], members[at])
        want = models[t].index[at, 0]
        diff = win != want
        if diff.any():
            r = np.flatnonzero(diff)[0]
            rep.fail("B", f"{int(diff.sum())} rows at iteration {t}: the nearest member of row {int(at[r])} is {int(win[r])}, the "
                          f"model's neighbour {int(want[r])} (entry of iteration {int(it[at][r])}, members {members[at][r].tolist()})")
        older = it[at] < t
        if older.any():
            ao, wo = at[older], win[older]
            p64 = P[t][ao].astype(np.float64)
            d = np.sqrt(((mm.m64[wo] - p64) ** 2).sum(axis=1))
            delta = np.sqrt(((p64 - pj[ao].astype(np.float64)) ** 2).sum(axis=1))
            room = L[ao] - (delta * c + float(EPS_DELTA)) - d * c
            band = BAND * (d + L[ao] + delta)
            with np.errstate(divide="ignore", invalid="ignore"):
                rep.worst_c = min(rep.worst_c, float(np.where(band > 0, room / band, np.inf).min()))
            viol = ~(d * c < L[ao] - (delta * c + float(EPS_DELTA)) + band)
            if viol.any():
                r = np.flatnonzero(viol)[0]
                rep.fail("C", f"{int(viol.sum())} rows kept at iteration {t} without the right to: row {int(ao[r])}, entry of "
                              f"iteration {int(it[ao][r])}, d {d[r]!r}, L {L[ao][r]!r}, delta {delta[r]!r}, band {band[r]!r}")
    # D: the records
    if rec is not None:
        at = np.flatnonzero(use & (rr >= max(first, 0)))
        rep.record_rows = int(at.size)
        if at.size:
            pr = np.stack([P[int(t)][r] for r, t in zip(at, rr[at])])
            want = np.array([models[int(t)].index[r, 0] for r, t in zip(at, rr[at])], np.int64)
            okf = np.array([not models[int(t)].flagged[r] for r, t in zip(at, rr[at])])
            got = np.ascontiguousarray(rec[at, :3]).view(np.uint32)
            ref = np.ascontiguousarray(mm.map[want]).view(np.uint32)
            diff = (got != ref).any(axis=1) & okf
            if diff.any():
                rep.fail("D", f"{int(diff.sum())} records whose winner has not the bits of the model's neighbour, first row "
                              f"{int(at[np.flatnonzero(diff)[0]])}")
            bound = rec[at, 3].astype(np.float64)
            d_out, i_out = nearest_outside(mm, pr, want[:, None])
            viol = ~(np.isfinite(bound)) | ((d_out < bound) & okf)
            if viol.any():
                r = np.flatnonzero(viol)[0]
                rep.fail("D", f"{int(viol.sum())} records: map point {int(i_out[r])} lies at {d_out[r]!r} < the bound {bound[r]!r} of "
                              f"row {int(at[r])} (record of iteration {int(rr[at][r])})")
    if fine_level and rep.rows and rep.positive == 0:
        rep.fail("vacuous", "no audited row has L > 0")
    if last + 1 >= 6 and rep.rows and rep.aged == 0:
        rep.fail("vacuous", f"{last + 1} iterations and no audited row has aged")
    if rep.flagged > K.FLAGGED_MAX * (rep.rows + rep.flagged) + 1:
        rep.fail("flagged", f"{rep.flagged} of {rep.rows + rep.flagged} rows flagged")
    print(rep.line())
    if raise_on_failure and rep.failures:
        raise AssertionError("\n".join(rep.failures))
    return rep


def run_and_audit(ctx, mm, scan, iterations, what, records=False, fine_level=True, register=None, close=True):
    """The loop of the GPU tests on a context (closed here unless `close` is off): one registration of `iterations` iterations (`register`: a callable
    that runs it instead and returns the result), ONE read-out, `last_neighbors` beside it, checks A - D.  (result, Report)"""
    n = scan.shape[0]
    res = register(ctx) if register else ctx.register(scan, None, False)
    out = ctx.last_cache_entries(n, records=records)
    ix, pose = ctx.last_neighbors(n)
    again = ctx.last_cache_entries(n)                 # the read-out reads: a second one finds what the first found
    fallbacks = ctx.handoff_fallbacks()
    if close:
        ctx.close()
    assert res.iterations == iterations and fallbacks == 0, (what, res.iterations, fallbacks)
    assert out["last"] == iterations - 1 and np.array_equal(out["pose_hist"][-1], np.asarray(pose, F32).reshape(3, 4)), what
    for k in ("members", "bound", "iteration", "pose_hist"):
        assert np.array_equal(np.asarray(out[k]).view(np.uint32), np.asarray(again[k]).view(np.uint32)), (what, k)
    rep = audit(mm, scan, out, what, fine_level)
    # the two read-outs agree: `last_neighbors` is the nearest member at the last pose
    p_last, _ = model_at(mm, scan, out["pose_hist"][-1])
    has = out["iteration"] >= 0
    win, _, _ = nearest_member(mm, p_last[has], out["members"][has].astype(np.int64))
    assert np.array_equal(win, np.asarray(ix)[has]) and (np.asarray(ix)[~has] == -1).all(), f"{what}: last_neighbors differs"
    return res, rep


# ---- the cache restated: the fake context of the CPU suite -------------------------------------------------------------
def _sqrt32(x):
    with np.errstate(invalid="ignore"):
        return np.sqrt(np.asarray(x, F32)).astype(F32)


def _dist32(a, b):
    m = (a - b).astype(F32)
    s, _ = K._fma_sq(m[:, 1], m[:, 0] * m[:, 0])
    d2, _ = K._fma_sq(m[:, 2], s)
    return d2


class FakeContext:
    """The NN cache on the host, answering from the model: every search leaves the model's neighbour, the members within
    SET_SPREAD of it and L = sqrtf(d2 of the nearest non-member) * 0.999999f; every later iteration applies the cache test in
    float32 (the root correctly rounded: the device's is within an ulp).  `poses`: [3, 4] per iteration, instead of a solve.
    wrong: "age_le" (age 25 passes), "slot_next" (the displacement from the pose of j + 1), "no_delta" (no displacement),
    "record_no_members" (a record's bound from `outside` alone), "field_plain" (the age taken from the stored 7-bit iteration
    field as it stands — the cache test before this audit: from iteration 128 on every entry looks 128 launches old)."""

    def __init__(self, map_pts, poses, records=False, wrong=None, mm=None):
        self.mm = mm or MapModel(map_pts)
        self.poses = [np.asarray(p, F32).reshape(3, 4) for p in poses]
        self.records, self.wrong = records, wrong
        self.out = None

    def _search(self, p, rows, t):
        _, (d2s, idxs, proven) = model_points(self.mm, p[rows])
        assert proven.all()
        near = _sqrt32(d2s)
        take = (near[:, 1:3] - near[:, :1]) < SET_SPREAD
        take[:, 1] &= take[:, 0]
        self.members[rows, 0] = idxs[:, 0]
        self.members[rows, 1] = np.where(take[:, 0], idxs[:, 1], -1)
        self.members[rows, 2] = np.where(take[:, 1], idxs[:, 2], -1)
        nxt = 1 + take.sum(axis=1)
        self.L[rows] = near[np.arange(rows.size), nxt] * C_DOWN
        self.it[rows] = t
        self.rec[rows] = 0
        self.rec_it[rows] = -1

    def register(self, scan, *_):
        scan = np.ascontiguousarray(scan, F32)
        n, mm = scan.shape[0], self.mm
        self.members, self.L, self.it = np.full((n, 3), -1, np.int64), np.zeros(n, F32), np.full(n, -1, np.int64)
        self.rec, self.rec_it = np.zeros((n, 8), F32), np.full(n, -1, np.int64)
        P = []
        max_age = CACHE_HIST + 1 if self.wrong == "age_le" else CACHE_HIST
        for t, pose in enumerate(self.poses):
            p, _ = S.transform_f32(pose, scan)
            P.append(p)
            hit = np.zeros(n, bool)
            if t:
                if self.records:
                    hr = np.flatnonzero((self.rec_it >= 0) & (t - self.rec_it <= max_age))
                    pr = np.stack([P[int(k)][r] for r, k in zip(hr, self.rec_it[hr])]) if hr.size else np.zeros((0, 3), F32)
                    delta = _sqrt32(_dist32(p[hr], pr)) * C_UP + EPS_DELTA
                    hit[hr] = _sqrt32(_dist32(self.rec[hr, :3], p[hr])) * C_UP < self.rec[hr, 3] - delta
                stored = (self.it & (ITER_WRAP - 1)) if self.wrong == "field_plain" else self.it
                he = np.flatnonzero(~hit & (t - stored <= max_age))
                src = np.minimum(self.it[he] + 1, t) if self.wrong == "slot_next" else self.it[he]
                pj = np.stack([P[int(k)][r] for r, k in zip(he, src)]) if he.size else np.zeros((0, 3), F32)
                delta = _sqrt32(_dist32(p[he], pj)) * C_UP + EPS_DELTA
                if self.wrong == "no_delta":
                    delta = np.zeros_like(delta)
                win, d2w, others2 = nearest_member(mm, p[he], self.members[he])
                outside = (self.L[he] - delta).astype(F32)
                ok = _sqrt32(d2w) * C_UP < outside
                hit[he] = ok
                if self.records:
                    bound = outside if self.wrong == "record_no_members" else np.minimum(outside, _sqrt32(others2) * C_DOWN)
                    rows = he[ok]
                    self.rec[rows, :3], self.rec[rows, 3], self.rec_it[rows] = mm.map[win[ok]], bound[ok], t
            self._search(p, np.flatnonzero(~hit), t)
        last = len(self.poses) - 1
        rec = self.rec.copy()
        rec[:, 7] = self.rec_it.astype(np.int32).view(F32)
        self.out = {"members": self.members.astype(np.int32), "bound": self.L.copy(), "iteration": self.it.astype(np.int32),
                    "pose_hist": np.stack(self.poses), "last": last, "records": rec}
        self._p_last = P[-1]
        return types.SimpleNamespace(iterations=len(self.poses))

    def last_cache_entries(self, n, records=False):
        assert not records or self.records, "no hit records"
        return {k: v for k, v in self.out.items() if k != "records" or records}

    def last_neighbors(self, n):
        win, _, _ = nearest_member(self.mm, self._p_last, self.members)
        return win.astype(np.int32), self.poses[-1]

    def handoff_fallbacks(self):
        return 0

    def close(self):
        pass


def converging_poses(count, shift, rate=0.5):
    """poses that take a scan displaced by `shift` back, the rest of the way shrinking by `rate` per iteration"""
    out = []
    for t in range(count):
        pose = np.eye(4, dtype=F32)[:3].copy()
        pose[:, 3] = (-np.asarray(shift, np.float64) * (1.0 - rate ** t)).astype(F32)
        out.append(pose)
    return out


# ---- one ring search that leaves an entry, with the wrong copies of check A ------------------------------------------------
def ring_entry(grid, q, max_rings=2, lanes=1, seed=None, wrong=None):
    """`nearest_in_level` as search_audit.ring_search restates it (slackened gaps), with what the cache keeps: (index, L).
    lanes: the visited cells are dealt round-robin to that many lanes, each with a best and a `second` of its own, reduced at
    the end (the row path's quad); seed: (d2, index) of a candidate known beforehand, the best of lane 0 at the start.
    wrong: "second_strict" (a pruned cell's gap as computed, not the slackened one the prune used), "seen_only" (pruned cells
    not folded), "lose_lanes" (the reduce takes the winning lane's `second` and the other lanes' seconds, not their bests),
    "seed_unfolded" (a seed that loses is forgotten)."""
    q = np.asarray(q, F32)
    h = grid.h
    c = S.cell_coord(q, h)
    off, strict_off = S.cell_off(q, c, h, True), S.cell_off(q, c, h, False)
    edge = F32(min(np.minimum(off[0], off[1])))
    INF, NONE = F32(np.inf), 0x7fffffff
    best, bidx, second = [INF] * lanes, [NONE] * lanes, [INF] * lanes
    if seed is not None:
        best[0], bidx[0] = F32(seed[0]), int(seed[1])
    pruned = INF
    dealt = 0

    def scan(cell):
        nonlocal dealt
        idx = grid.cells.get(cell)
        if not idx:
            return
        ln = dealt % lanes
        dealt += 1
        for d2, i in zip(S._d2(grid, idx, q), idx):
            if i == bidx[ln]:
                continue
            if d2 < best[ln] or (d2 == best[ln] and i < bidx[ln]):
                loser_is_seed = seed is not None and bidx[ln] == int(seed[1])
                if not (wrong == "seed_unfolded" and loser_is_seed):
                    second[ln] = min(second[ln], best[ln])
                best[ln], bidx[ln] = d2, i
            else:
                second[ln] = min(second[ln], d2)

    def shell(r, sl):
        o = np.arange(-r, r + 1)
        use = off if sl else strict_off
        gx, gy, gz = (S.axis_gap(o, (use[0][a], use[1][a]), h, sl) for a in range(3))
        n = o.size
        s2, _ = K._fma_sq(np.broadcast_to(gy[None, :], (n, n)).copy(), np.broadcast_to((gz * gz)[:, None], (n, n)).copy())
        g2, _ = K._fma_sq(np.broadcast_to(gx[None, None, :], (n, n, n)).copy(), np.broadcast_to(s2[:, :, None], (n, n, n)).copy())
        return o, g2

    def reduce():
        w = min(range(lanes), key=lambda k: (best[k], bidx[k]))
        sec = min(second)
        if wrong != "lose_lanes":
            for k in range(lanes):
                if k != w and bidx[k] != bidx[w]:
                    sec = min(sec, best[k])
        if wrong != "seen_only":
            sec = min(sec, pruned)
        return best[w], bidx[w], sec

    scan(tuple(c.tolist()))
    for r in range(1, max_rings + 1):
        o, g2s = shell(r, True)
        g2b = shell(r, False)[1] if wrong == "second_strict" else g2s
        on_shell = np.abs(o)[:, None, None] == r
        on_shell = on_shell | (np.abs(o)[None, :, None] == r) | (np.abs(o)[None, None, :] == r)
        for iz, iy, ix in np.argwhere(on_shell):
            if g2s[iz, iy, ix] > min(best):
                pruned = min(pruned, g2b[iz, iy, ix])
                continue
            scan((int(c[0]) + int(o[ix]), int(c[1]) + int(o[iy]), int(c[2]) + int(o[iz])))
        bound = S.ring_bound(r, h, edge, True)
        b2 = bound * bound * S.EXIT_FACTOR
        b, i, sec = reduce()
        if b <= b2:
            return i, _sqrt32(min(sec, b2)) * C_DOWN
    return reduce()[1], F32(0.0)


def entries_of(cloud, rows, **kw):
    """a read-out of one iteration from the identity whose entries `ring_entry` made for `rows` (the other rows: no entry)"""
    grid = S.Grid(cloud.map, cloud.h)
    n = cloud.queries.shape[0]
    members, bound, it = np.full((n, 3), -1, np.int32), np.zeros(n, F32), np.full(n, -1, np.int32)
    for r in rows:
        seed = kw.get("seed_of", {}).get(int(r)) if "seed_of" in kw else None
        i, L = ring_entry(grid, cloud.queries[r], seed=seed, **{k: v for k, v in kw.items() if k != "seed_of"})
        members[r, 0], bound[r], it[r] = i, L, 0
    return {"members": members, "bound": bound, "iteration": it, "pose_hist": np.eye(4, dtype=F32)[None, :3], "last": 0}


# ---- the clouds that aim at the bound ------------------------------------------------------------------------------------
GAPS = np.logspace(-6, -2, 9)                 # d(B) - d(W), metres
QUAD_OFFSETS = (3.0e-4, 3.0e-3, 2.5e-2)       # the query's distance from the face


def face_quads(h, per_line=12):
    """Face quadruples: W in the query's own cell, B in the neighbouring cell of one axis on a point of search_audit.face_table
    (below (float)k * h although in cell k: d(B) < the gap as computed), C in the own cell farther out, d(B) - d(W) graded
    over GAPS; and the same across an edge and a corner of the cell (gap2 a sum of two or three squares).  h = 0.5 (control):
    B on the face or 8 ulp off it.  kinds: "face", "edge", "corner" (adversarial: d(B) < the strict gap), "control"."""
    def make():
        am, aq, kinds, expect = [], [], {"face": [], "edge": [], "corner": [], "control": []}, {}
        lane, g_at = 0, 0

        def add(kind, Q, B, axis0):
            nonlocal g_at
            dB = np.sqrt(((B.astype(np.float64) - Q) ** 2).sum())
            sgn = F32(np.sign(B[axis0] - Q[axis0]))
            cq = S.cell_coord(Q, h)
            for _ in range(GAPS.size):      # the next grade this place can hold (an ulp of a 300 m coordinate is 3e-5 m)
                g = GAPS[g_at % GAPS.size]
                g_at += 1
                W, Cp = Q.copy(), Q.copy()
                W[axis0] = F32(Q[axis0] - sgn * F32(dB - g))
                Cp[axis0] = F32(Q[axis0] - sgn * F32(1.5 * dB + 1.0e-3))
                d2 = K.model_d2(np.stack((W, B, Cp)), Q[None])[0][0]
                if g < 0.8 * dB and (S.cell_coord(W, h) == cq).all() and (S.cell_coord(Cp, h) == cq).all() and d2[0] < d2[1] < d2[2]:
                    break
            else:
                return False
            expect[len(aq)] = len(am)
            am.extend((W, B, Cp))
            kinds[kind].append(len(aq))
            aq.append(Q)
            return True

        for axis in range(3):
            for sign in (1, -1):
                table = S.face_table(h, sign, QUAD_OFFSETS)
                picks = S._spread([t for t in table if t[4]], per_line) if h != S.CONTROL_H else \
                    S._spread([t for t in table if not t[4]], per_line)
                for k, a, q, _, adv in picks:
                    add("face" if adv else "control", S._point(axis, q, lane), S._point(axis, a, lane), axis)
                lane += 1
        if h != S.CONTROL_H:
            for naxes, kind in ((2, "edge"), (3, "corner")):
                for k, a, q, _, _ in S._spread([t for s in (1, -1) for t in S.face_table(h, s, QUAD_OFFSETS) if t[4]], 4 * per_line):
                    if len(kinds[kind]) >= per_line:
                        break
                    A, Q = S._point(0, a, 40 + naxes), S._point(0, q, 40 + naxes)
                    A[:naxes], Q[:naxes] = a, q
                    cq, ca = S.cell_coord(Q, h), S.cell_coord(A, h)
                    g2 = (S.axis_gap(ca - cq, S.cell_off(Q, cq, h, False), h, False).astype(np.float64) ** 2).sum()
                    if g2 > K.model_d2(A[None], Q[None])[0][0, 0]:
                        add(kind, Q, A, 0)
        return S._assemble(f"face quads h={h}", h, "W in the own cell, B on a skewed face point across it, C beyond", am, aq,
                           kinds, expect, S.SMALL_FILLER)
    return S._cached(("face_quads", h, per_line), make)


def lane_split(h, per_axis=12):
    """The own cell is empty; W across the face of one axis, B across the face of ANOTHER axis, d(B) - d(W) graded over GAPS:
    two cells of ring 1 — two lanes of a split search, and the loser's best is the runner-up."""
    def make():
        am, aq, kinds, expect = [], [], {"split": []}, {}
        hh = F32(h)
        g_at = 0
        for axis in range(3):
            other = (axis + 1) % 3
            n = 0
            table = [t for s in (1, -1) for t in S.face_table(h, s, QUAD_OFFSETS)]
            for k, a, q, _, _ in S._spread(table, 8 * per_axis):
                if n >= per_axis:
                    break
                dW = abs(float(a) - float(q))
                g = GAPS[g_at % GAPS.size]
                g_at += 1
                base = S._ulps(F32(abs(k) + 3) * hh, 16)
                W, Q, B = S._point(axis, a, 60), S._point(axis, q, 60), S._point(axis, q, 60)
                W[other] = Q[other] = base
                B[other] = F32(base - F32(dW + g))
                d2 = K.model_d2(np.stack((W, B)), Q[None])[0][0]
                if len({tuple(S.cell_coord(p, h)) for p in (W, Q, B)}) != 3 or not d2[0] < d2[1]:
                    continue
                expect[len(aq)] = len(am)
                am.extend((W, B))
                kinds["split"].append(len(aq))
                aq.append(Q)
                n += 1
        return S._assemble(f"lane split h={h}", h, "own cell empty, winner and runner-up across faces of two axes", am, aq, kinds,
                           expect, S.SMALL_FILLER)
    return S._cached(("lane_split", h, per_axis), make)


def sets_of_three(h=0.3, count=48):
    """Three candidates within 1e-4 .. 1e-3 m of each other in distance and a fourth 1e-4 .. 1e-3 m beyond them, around a query
    in the middle of its cell: at 0.1 m (all four in the own cell) and at 0.2 m (across four faces)."""
    def make():
        rng = np.random.default_rng(23)
        am, aq, kinds, expect = [], [], {"own": [], "across": []}, {}
        dirs = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0]], np.float64)
        for i in range(count):
            kind, d0 = ("own", 0.1) if i % 2 == 0 else ("across", 0.2)
            cell = np.array([203 + 7 * i, 205, 207 + (i % 5)], np.float64)
            Q = ((cell + 0.5) * h).astype(F32)
            e = np.sort(10.0 ** rng.uniform(-4, -3, 2))
            dist = np.array([d0, d0 + e[0] * 0.5, d0 + e[1], d0 + e[1] + 10.0 ** rng.uniform(-4, -3)])   # (spread e[1])
            pts = (Q.astype(np.float64)[None] + dirs[rng.permutation(4)] * dist[:, None]).astype(F32)
            expect[len(aq)] = len(am)
            am.extend(pts)
            kinds[kind].append(len(aq))
            aq.append(Q)
        return S._assemble(f"sets of three h={h}", h, "three near-equal candidates and a fourth just beyond", am, aq, kinds, expect,
                           S.SMALL_FILLER)
    return S._cached(("sets_of_three", h, count), make)


def classify_quads(cloud):
    """Of the INPUT, per adversarial row of a face-quad or lane-split cloud (rows of kinds face / edge / corner / control /
    split): (own cell of W, B in another cell, d(B) below the gap to B's cell as computed, d(B) - d(W) float64, whether the
    SLACKENED gap of B's cell exceeds d(W): the cell is pruned once W is the best)"""
    out = {}
    h = cloud.h
    for kind, rows in cloud.kinds.items():
        for r in rows:
            Q = cloud.queries[r]
            w = cloud.expect[int(r)]
            W, B = cloud.map[w], cloud.map[w + 1]
            cq, cw, cb = S.cell_coord(Q, h), S.cell_coord(W, h), S.cell_coord(B, h)
            gs = S.axis_gap(cb - cq, S.cell_off(Q, cq, h, False), h, False).astype(np.float64)
            gl = S.axis_gap(cb - cq, S.cell_off(Q, cq, h, True), h, True).astype(np.float64)
            dW = np.sqrt(((W.astype(np.float64) - Q) ** 2).sum())
            dB = np.sqrt(((B.astype(np.float64) - Q) ** 2).sum())
            out[int(r)] = types.SimpleNamespace(kind=kind, w_own=bool((cw == cq).all()), b_other=bool((cb != cq).any()),
                                                below_gap=bool(dB * dB < (gs ** 2).sum()), gap=dB - dW,
                                                pruned=bool((gl ** 2).sum() > dW * dW), own_empty=bool((cw != cq).any()),
                                                two_axes=bool(((cw != cq) & (cb == cq)).any() and ((cb != cq) & (cw == cq)).any()))
    return out


NEW_CLOUDS = {"face quads h=0.3": lambda: face_quads(0.3), "face quads h=0.7": lambda: face_quads(0.7),
              "face quads h=0.5": lambda: face_quads(0.5), "lane split h=0.3": lambda: lane_split(0.3),
              "lane split h=0.7": lambda: lane_split(0.7), "sets of three h=0.3": lambda: sets_of_three(0.3)}
FINE_CLOUDS = dict(NEW_CLOUDS, **S.SMALL)                       # a fine-level answer for (nearly) every row: L > 0 expected
REUSED = ("exits h=0.3", "coarse h=0.3", "far cells h=0.05")    # L == 0 or sound, never NaN
ITERATED = ("face quads h=0.3", "face quads h=0.7", "lane split h=0.3", "sets of three h=0.3", "skew ties h=0.3 small",
            "ties h=0.5 small")


def cloud(name):
    c = FINE_CLOUDS[name]() if name in FINE_CLOUDS else S.cloud(name)
    assert c.name == name, (c.name, name)
    return c


_MODELS = {}


def map_model(name, map_pts=None):
    """the MapModel of a cloud's map (or of `map_pts` under that name), made once"""
    if name not in _MODELS:
        _MODELS[name] = MapModel(cloud(name).map if map_pts is None else map_pts)
    return _MODELS[name]
