"""Audit of single iterations of the fused hash-grid registration (tests/test_iteration_audit.py on the CPU,
tests/test_gpu_iteration_audit.py on the device).  TEST INFRASTRUCTURE: numpy + scipy + oracle/icp_oracle.py, importable
without a GPU, never imported by the package.

ICP corrects itself: an iteration that drops a workgroup's rows or matches a few targets to a stale neighbour still ends at
the same pose within 1e-4.  So every iteration is held on its own: a run of k iterations with threshold 0 is a prefix of a
run of K (`truncated_runs` asserts it to the bit), `icp_last_neighbors` returns the neighbour of every target and the pose
of the LAST iteration of a run, and `audit_iteration` makes four independent checks of that iteration:

  rows / row count   the step and loss recomputed from the kernel's OWN neighbours and normals (float32 rows, exact sums:
                     O.gauss_newton_step with float64 accumulation) at the bars of projective_cases.assert_step;
  neighbours         the kernel's neighbours against a kd-tree at the pose the iteration ran with;
  normals            the kernel's normals against O.knn_normals of the map as currently expressed;
  pose chain         the next pose from this iteration's step in the oracle's float32 algebra.

The accounting takes the record of an iteration as plain arrays, so the CPU suite hands it the oracle's own loop
(`oracle_records`) — and deliberately wrong copies of it.
"""
from dataclasses import dataclass, replace
from typing import Optional

import numpy as np
from scipy.spatial import cKDTree

import icp_oracle as O
from projective_cases import F32, F64, ROW_SIGMA, SCHEMES, assert_step, fma32, transform_fma  # noqa: F401 (shared)

ICP_OK, ICP_ERR_INVALID_JACOBIAN = 0, -3
STEP_ATOL = 2.0e-7  # projective_cases.assert_step: dx atol 2e-7 / rtol 2e-5, loss 1e-5
MISMATCH_CAP = 1.0e-3  # share of valid rows whose neighbour may differ from the kd-tree's (the `> 0.999` of the C2 tests)
TIE_RTOL = 2.0e-6  # ... each of them a squared-distance tie within this (the `rtol=2e-6` of the C2 tests)
TIE_ABS = 1.0e-12  # ... or closer than this in absolute squared distance (m^2: coincident points)
NORMAL_DOT, NORMAL_UNIT = 1.0e-5, 1.0e-5
POSE_ATOL = 1.0e-6  # test_register_masks_nan_and_null_rows
COSTS = ("point_to_plane", "point_to_point")


class AuditFailure(AssertionError):
    """`checks`: the names of the checks that failed ("rows", "row count", "neighbours", "normals", "pose chain")."""

    def __init__(self, failures):
        self.failures = failures
        self.checks = tuple(name for name, _ in failures)
        super().__init__("; ".join(f"[{name}] {why}" for name, why in failures))


@dataclass
class IterationRecord:
    k: int  # 1-based iteration
    pose12: np.ndarray  # [3,4] f32: the pose the iteration ran with
    ix: Optional[np.ndarray]  # [n] neighbour (original map index) of every target row, -1: masked; None: not observable
    loss: float
    dx: np.ndarray  # [6] f32
    num_targets: int
    status: int  # ICP_OK | ICP_ERR_INVALID_JACOBIAN at this iteration
    iterations: int  # of the run that ended with this iteration
    converged: bool
    pose_after: np.ndarray  # [4,4] f32: the pose the run returned


# ----------------------------------------------------------------------------------------------------------------------
# restated arithmetic
# ----------------------------------------------------------------------------------------------------------------------
def pose44(pose12):
    t = np.eye(4, dtype=F32)
    t[:3, :] = np.asarray(pose12, F32).reshape(3, 4)
    return t


def valid_rows(targets, skip_null):
    """target_valid of search_device.h: no NaN; under skip_null not (0, 0, 0)."""
    t = np.asarray(targets, F32).reshape(-1, 3)
    ok = ~np.isnan(t).any(axis=1)
    if skip_null:
        ok &= ~(t == 0).all(axis=1)
    return ok


def chain_pose(dx, pose):
    """register_new_frame (icp_odometry.py:296-297) in the oracle's float32 algebra."""
    return O.build_pose_matrix(O.from_pose_matrix((O.build_pose_matrix(np.asarray(dx, F32)) @ pose44(pose[:3])).astype(F32)))


def brute_force_nn_f32(queries, model, chunk=1024):
    """Nearest map point in FLOAT32 arithmetic, d2 = (dx dx + dy dy) + dz dz, the lowest index of equal distances."""
    q, m = np.asarray(queries, F32), np.asarray(model, F32)
    idx = np.empty(q.shape[0], np.int64)
    for s in range(0, q.shape[0], chunk):
        d = q[s:s + chunk, None, :] - m[None, :, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        idx[s:s + chunk] = d2.argmin(axis=1)
    return idx


def weighted_rows(p, q, n, scheme, sigma, cost):
    """(weighted residuals [m] f32, weighted Jacobian [m,6] f32, sum r^2 in float64) as O.gauss_newton_step /
    O.point_to_point_step form them at x0 = 0."""
    p, q = np.asarray(p, F32), np.asarray(q, F32)
    if cost == "point_to_plane":
        res, jac = O.point_to_plane_rows(p, q, np.asarray(n, F32))
    else:
        d = (p - q).astype(F32)
        res = np.sqrt((d * d).sum(axis=-1, dtype=F32))
        dr = O.euler_jacobian(np.zeros(3, F32))
        jac = np.concatenate([d, np.stack([((p @ dr[k].T).astype(F32) * d).sum(axis=-1, dtype=F32) for k in range(3)], 1)],
                             axis=1).astype(F32)
    raw = float((res.astype(F64) ** 2).sum())
    w = O.ls_weights(scheme, sigma, res, p, q)
    return (res * w).astype(F32), (jac * w.reshape(-1, 1)).astype(F32), raw


def reference_step(p, q, n, scheme, sigma, cost):
    """The float64 Gauss-Newton step of the rows, two algebraically equal ways.  Returns dict(status, stopped, dx [6] f32,
    loss, count, spread = max |inv(H) g - cholesky solve| (float64), det = (LU, Cholesky))."""
    count = int(np.asarray(p).shape[0])
    out = dict(status=ICP_OK, stopped=False, dx=np.zeros(6, F32), loss=0.0, count=count, spread=0.0, det=(0.0, 0.0))
    if count == 0:
        out.update(stopped=True)
        return out
    res, jac, raw = weighted_rows(p, q, n, scheme, sigma, cost)
    if np.sqrt(raw) < 1.0e-7:  # optimization.py:323-327
        out.update(stopped=True, loss=raw)
        return out
    ja, ra = jac.astype(F64), res.astype(F64)
    H, g = ja.T @ ja, ja.T @ ra
    out["loss"] = float((ra * ra).sum())
    det_lu = float(np.linalg.det(H))
    try:
        L = np.linalg.cholesky(H)
        det_ch = float(np.prod(np.diag(L) ** 2))
    except np.linalg.LinAlgError:
        L, det_ch = None, 0.0
    out["det"] = (det_lu, det_ch)
    if abs(det_lu) < 1.0e-7:  # :334-336
        out["status"] = ICP_ERR_INVALID_JACOBIAN
    try:
        dx_inv = -(np.linalg.inv(H) @ g)
        other = np.linalg.solve(L.T, np.linalg.solve(L, g)) if L is not None else np.linalg.solve(H, g)
    except np.linalg.LinAlgError:
        return out
    out["dx"] = dx_inv.astype(F32)
    out["spread"] = float(np.abs(dx_inv + other).max())
    return out


# ----------------------------------------------------------------------------------------------------------------------
# the four checks
# ----------------------------------------------------------------------------------------------------------------------
def check_rows(rec, targets, map_points, normals, scheme, sigma, cost, skip_null, ix=None):
    """Rows and solve.  Returns (failures, figures)."""
    t = np.asarray(targets, F32).reshape(-1, 3)
    ok = valid_rows(t, skip_null)
    p = transform_fma(t[ok], pose44(rec.pose12))
    ix = np.asarray(rec.ix if ix is None else ix)[ok]
    fails, fig = [], dict(rows=int(ok.sum()), ddx=0.0, dloss=0.0, spread=0.0, atol=STEP_ATOL, widened=False)
    if rec.num_targets != int(ok.sum()):
        fails.append(("row count", f"iteration {rec.k}: {rec.num_targets} rows summed, {int(ok.sum())} valid"))
    if ok.any() and ((ix < 0).any() or (ix >= len(map_points)).any()):
        fails.append(("rows", f"iteration {rec.k}: a valid row without a neighbour"))
        return fails, fig
    q = np.asarray(map_points, F32)[ix]
    n = np.asarray(normals, F32)[ix] if cost == "point_to_plane" else None
    ref = reference_step(p, q, n, scheme, sigma, cost)
    fig.update(spread=ref["spread"], det=ref["det"], ref_status=ref["status"], stopped=ref["stopped"])
    # a determinant the two float64 formulations (LU, Cholesky) put on either side of the 1e-7 guard is undetermined by the
    # reference itself: either status is accepted there
    undetermined = (abs(ref["det"][0]) < 1.0e-7) != (abs(ref["det"][1]) < 1.0e-7) and not ref["stopped"]
    fig["status_undetermined"] = undetermined
    invalid = rec.status == ICP_ERR_INVALID_JACOBIAN if undetermined else ref["status"] == ICP_ERR_INVALID_JACOBIAN
    if invalid != (rec.status == ICP_ERR_INVALID_JACOBIAN) or rec.status not in (ICP_OK, ICP_ERR_INVALID_JACOBIAN):
        fails.append(("rows", f"iteration {rec.k}: status {rec.status}, the oracle's {ref['status']} (det {ref['det'][0]:.3e} "
                              f"by LU, {ref['det'][1]:.3e} by Cholesky)"))
        return fails, fig
    if invalid:  # dx = 0, the loss of the rows, the loop ends there, not converged
        if np.any(rec.dx != 0) or rec.iterations != rec.k or rec.converged:
            fails.append(("rows", f"iteration {rec.k}: Invalid Jacobian with dx {rec.dx}, iterations {rec.iterations}, "
                                  f"converged {rec.converged}"))
        if abs(rec.loss - ref["loss"]) > 1e-5 * abs(ref["loss"]):
            fails.append(("rows", f"iteration {rec.k}: loss {rec.loss} vs {ref['loss']} at the Invalid Jacobian"))
        return fails, fig
    if ref["stopped"]:  # ||r|| < 1e-7: x unchanged, loss = sum r^2, the loop ends converged
        if np.any(rec.dx != 0) or not rec.converged or rec.iterations != rec.k:
            fails.append(("rows", f"iteration {rec.k}: residual guard, but dx {rec.dx} converged {rec.converged} "
                                  f"iterations {rec.iterations}"))
        if abs(rec.loss - ref["loss"]) > 1e-5 * abs(ref["loss"]) + 1e-300:
            fails.append(("rows", f"iteration {rec.k}: loss {rec.loss} vs sum r^2 {ref['loss']}"))
        return fails, fig
    fig["ddx"] = float(np.abs(rec.dx.astype(F64) - ref["dx"].astype(F64)).max())
    fig["dloss"] = abs(rec.loss - ref["loss"]) / abs(ref["loss"]) if ref["loss"] else abs(rec.loss)
    atol = max(STEP_ATOL, 4.0 * ref["spread"])  # the tolerance rule: from the reference's own spread, never the kernel's
    fig.update(atol=atol, widened=atol > STEP_ATOL)
    try:
        if atol > STEP_ATOL:
            np.testing.assert_allclose(rec.dx, ref["dx"], atol=atol, rtol=2e-5)
            assert abs(rec.loss - ref["loss"]) <= 1e-5 * abs(ref["loss"]), (rec.loss, ref["loss"])
        else:
            assert_step(rec.dx, rec.loss, ref["count"], (ref["dx"], ref["loss"], ref["count"]))
    except AssertionError as e:
        fails.append(("rows", f"iteration {rec.k}: |ddx| {fig['ddx']:.2e} dloss {fig['dloss']:.2e} (atol {atol:.1e}): "
                              + " ".join(str(e).split())[:300]))
    return fails, fig


def check_neighbours(rec, targets, map_points, skip_null, tree=None, low=None):
    """The kernel's neighbours against the kd-tree at the pose the iteration ran with."""
    t = np.asarray(targets, F32).reshape(-1, 3)
    ok = valid_rows(t, skip_null)
    ix = np.asarray(rec.ix)
    fails, fig = [], dict(mismatches=0, share=0.0, worst_tie=0.0)
    if (ix[~ok] != -1).any() or (ix[ok] < 0).any():
        fails.append(("neighbours", f"iteration {rec.k}: {(ix[~ok] != -1).sum()} masked rows with a neighbour, "
                                    f"{(ix[ok] < 0).sum()} valid rows without"))
        return fails, fig
    if not ok.any():
        return fails, fig
    if (ix[ok] >= len(map_points)).any():
        fails.append(("neighbours", f"iteration {rec.k}: index beyond the map"))
        return fails, fig
    m = np.asarray(map_points, F32).astype(F64)
    p = transform_fma(t[ok], pose44(rec.pose12)).astype(F64)
    bd, bi = (tree if tree is not None else cKDTree(m)).query(p, workers=-1)
    used = ((p - m[ix[ok]]) ** 2).sum(axis=1)
    if low is None:
        differ = ix[ok] != bi
    else:  # (the tree returns ANY of equal points: compare the lowest index of each; check_duplicates holds the kernel to it)
        differ = low[ix[ok]] != low[bi]
    fig["mismatches"] = int(differ.sum())
    fig["share"] = float(differ.mean())
    if differ.any():
        rel = np.abs(used[differ] - bd[differ] ** 2) / np.maximum(bd[differ] ** 2, 1e-300)
        rel = np.where(np.abs(used[differ] - bd[differ] ** 2) <= TIE_ABS, 0.0, rel)
        fig["worst_tie"] = float(rel.max())
        if (rel > TIE_RTOL).any():
            fails.append(("neighbours", f"iteration {rec.k}: {(rel > TIE_RTOL).sum()} of {differ.sum()} mismatches are no "
                                        f"distance ties (worst {rel.max():.2e} relative)"))
    if differ.mean() > MISMATCH_CAP:
        fails.append(("neighbours", f"iteration {rec.k}: {differ.sum()} of {ok.sum()} neighbours differ from the kd-tree's"))
    return fails, fig


def lowest_index_of_equal_points(map_points):
    """For every map point the lowest index holding the same coordinates (itself where it is unique)."""
    m = np.ascontiguousarray(np.asarray(map_points, F32) + F32(0.0))  # (-0.0 == 0.0)
    _, first, inv = np.unique(m.view(np.dtype((np.void, 12))).reshape(-1), return_index=True, return_inverse=True)
    lowest = np.full(len(first), len(m), np.int64)
    np.minimum.at(lowest, inv.reshape(-1), np.arange(len(m)))
    return lowest[inv.reshape(-1)]


def check_duplicates(rec, low):
    """Exact duplicates in the map (`low` = lowest_index_of_equal_points): the tie goes to the lowest index."""
    ix = np.asarray(rec.ix)
    used = ix[ix >= 0]
    bad = used != low[used]
    return [("neighbours", f"iteration {rec.k}: {bad.sum()} neighbours are not the lowest index of equal points")] \
        if bad.any() else []


class NormalReference:
    """O.knn_normals of the map points a registration used, computed once per map, and which of them are DETERMINED by
    the oracle's own values (the criterion of test_knn_normals_on_stress_clouds): the two smallest eigenvalues of the
    neighbourhood covariance apart by more than 1e-3 of the largest, no tie on the k-th distance."""

    def __init__(self, map_points, k=10):
        self.m = np.asarray(map_points, F32)
        self.k = k
        self.tree = cKDTree(self.m.astype(F64))
        self.ref = np.full((len(self.m), 3), np.nan, F32)
        self.clear = np.zeros(len(self.m), bool)
        self.done = np.zeros(len(self.m), bool)

    def need(self, idx):
        idx = np.unique(np.asarray(idx))
        idx = idx[~self.done[idx]]
        k = self.k
        if not len(idx) or len(self.m) < k + 1:  # fewer than k + 1 points: the reference has no neighbourhood of k
            return
        self.ref[idx] = O.knn_normals(self.m, self.tree, idx, k=k)
        d, nb = self.tree.query(self.m[idx].astype(F64), k=min(k + 2, len(self.m)), workers=-1)
        c = (self.m[nb[:, 1:k + 1].reshape(-1)].reshape(-1, k, 3) - self.m[idx][:, None, :]).astype(F64)
        ev = np.linalg.eigvalsh((c[:, :, :, None] * c[:, :, None, :]).mean(axis=1))
        self.clear[idx] = ev[:, 1] - ev[:, 0] > 1e-3 * ev[:, 2]
        if d.shape[1] == k + 2:  # (exactly k + 1 points: every other point is a neighbour, no k-th distance to tie on)
            self.clear[idx] &= d[:, -1] - d[:, -2] > 1e-6 * d[:, -1]
        self.done[idx] = True


def check_normals(rec, normals, nref):
    """Every normal used: finite and of unit norm to 1e-5.  Over the neighbourhoods the oracle determines: |dot| > 1 - 1e-5
    against O.knn_normals on the map as currently expressed — normals carried through a pose-only update included, at the
    same bar.  `used` / `clear` (how many were compared) are reported per iteration."""
    ix = np.asarray(rec.ix)
    used = np.unique(ix[ix >= 0])
    fails, fig = [], dict(used=int(len(used)), clear=0, min_dot=1.0)
    if not len(used):
        return fails, fig
    n = np.asarray(normals, F32)[used]
    if not np.isfinite(n).all():
        fails.append(("normals", f"iteration {rec.k}: non-finite normals"))
        return fails, fig
    length = np.linalg.norm(n.astype(F64), axis=1)
    if (np.abs(length - 1.0) > NORMAL_UNIT).any():
        fails.append(("normals", f"iteration {rec.k}: |n| off 1 by {np.abs(length - 1).max():.2e}"))
    nref.need(used)
    clear = nref.clear[used]
    fig["clear"] = int(clear.sum())
    if clear.any():
        dots = np.abs((n[clear].astype(F64) * nref.ref[used][clear].astype(F64)).sum(axis=1))
        fig["min_dot"] = float(dots.min())
        if not fig["min_dot"] > 1 - NORMAL_DOT:
            fails.append(("normals", f"iteration {rec.k}: min |dot| {fig['min_dot']:.7f}, {(dots <= 1 - NORMAL_DOT).sum()} of "
                                     f"{clear.sum()} determined normals beyond 1e-5"))
    if len(used) >= 100 and clear.mean() <= 0.5:
        fails.append(("normals", f"iteration {rec.k}: only {clear.mean() * 100:.1f} % of the used neighbourhoods are determined"))
    return fails, fig


def check_pose_chain(rec, pose_next):
    """pose_{k+1} (the pose iteration k + 1 ran with, or the pose the run returned) from pose_k and dx_k."""
    fails, fig = [], dict(drot=0.0, dtrans=0.0)
    moved = rec.status == ICP_OK and not rec.converged  # (a guard, a live threshold or an error: the loop breaks first)
    expect = chain_pose(rec.dx, rec.pose12) if moved else pose44(rec.pose12)
    got = np.asarray(pose_next, F32).reshape(-1, 4)[:3]
    fig["drot"] = float(np.abs(got[:, :3].astype(F64) - expect[:3, :3]).max())
    scale = max(1.0, float(np.abs(expect[:3, 3]).max()))
    fig["dtrans"] = float(np.abs(got[:, 3].astype(F64) - expect[:3, 3]).max()) / scale
    if not moved and not np.array_equal(got, expect[:3]):
        fails.append(("pose chain", f"iteration {rec.k}: the pose moved behind a guard / an error"))
    elif fig["drot"] > POSE_ATOL or fig["dtrans"] > POSE_ATOL:
        fails.append(("pose chain", f"iteration {rec.k}: rotation off by {fig['drot']:.2e}, translation by "
                                    f"{fig['dtrans']:.2e} x max(1, |t|)"))
    return fails, fig


def audit_iteration(rec, targets, map_points, normals, scheme, sigma, cost="point_to_plane", skip_null=False,
                    pose_next=None, nref=None, tree=None, low=None):
    """The four checks of one iteration; raises AuditFailure naming those that failed, returns the figures.  `rec.ix` None
    (the neighbours of the iteration are not observable: the point-to-point cost runs unfused): rows and solve from the
    kd-tree's neighbours, no neighbour / normal check."""
    fails, fig = [], {}
    if rec.ix is None:
        t = np.asarray(targets, F32).reshape(-1, 3)
        ok = valid_rows(t, skip_null)
        kd = np.full(len(t), -1, np.int64)
        if ok.any():
            m = np.asarray(map_points, F32).astype(F64)
            kd[ok] = (tree if tree is not None else cKDTree(m)).query(
                transform_fma(t[ok], pose44(rec.pose12)).astype(F64), workers=-1)[1]
        f, g = check_rows(rec, targets, map_points, normals, scheme, sigma, cost, skip_null, ix=kd)
        fails += f
        fig.update(g)
    else:
        f, g = check_rows(rec, targets, map_points, normals, scheme, sigma, cost, skip_null)
        fails += f
        fig.update(g)
        f, g = check_neighbours(rec, targets, map_points, skip_null, tree, low)
        fails += f
        fig.update(g)
        if low is not None:
            fails += check_duplicates(rec, low)
        if cost == "point_to_plane" and nref is not None:
            f, g = check_normals(rec, normals, nref)
            fails += f
            fig.update(g)
    if pose_next is not None:
        f, g = check_pose_chain(rec, pose_next)
        fails += f
        fig.update(g)
    if fails:
        raise AuditFailure(fails)
    return fig


class Worst:
    """The worst figures of a case family, printed by the tests and quoted in their docstrings."""

    def __init__(self, name):
        self.name, self.n = name, 0
        self.f = dict(ddx=0.0, dloss=0.0, share=0.0, mismatches=0, worst_tie=0.0, drot=0.0, dtrans=0.0, min_dot=1.0,
                      atol=STEP_ATOL, spread=0.0)
        self.widened = []
        self.undetermined = []  # iterations whose status the reference itself leaves open

    def add(self, fig, label=""):
        self.n += 1
        for k in self.f:
            if k in fig and np.isfinite(fig[k]):
                self.f[k] = min(self.f[k], fig[k]) if k == "min_dot" else max(self.f[k], fig[k])
        if fig.get("widened"):
            self.widened.append((label, fig["spread"], fig["atol"]))

    def __str__(self):
        f = self.f
        s = (f"{self.name}: {self.n} iterations audited; worst |ddx| {f['ddx']:.2e}, dloss {f['dloss']:.2e}, mismatch share "
             f"{f['share']:.2e} ({f['mismatches']} rows at most, worst tie {f['worst_tie']:.1e}), pose chain "
             f"{max(f['drot'], f['dtrans']):.2e}, min |dot| {f['min_dot']:.7f}")
        for label, spread, atol in self.widened[:6]:
            s += f"\n  widened {label}: reference spread {spread:.2e} -> dx atol {atol:.2e}"
        for label in self.undetermined:
            s += f"\n  status undetermined by the reference, the kernel's accepted: {label}"
        if len(self.widened) > 6:
            s += f"\n  ... and {len(self.widened) - 6} more widened iterations"
        return s


# ----------------------------------------------------------------------------------------------------------------------
# runs on the device
# ----------------------------------------------------------------------------------------------------------------------
def registered(call):
    """(status, RegisterResult) of a registration call: an InvalidJacobianError carries the result up to the failing
    iteration (`result`)."""
    from pylidar_slam_amd.engine import InvalidJacobianError
    try:
        return ICP_OK, call()
    except InvalidJacobianError as e:
        assert e.result is not None
        return ICP_ERR_INVALID_JACOBIAN, e.result


def raw_register(ctx, points, init_pose=None, skip_null=False):
    return registered(lambda: ctx.register(points, init_pose, skip_null))


def raw_register_end(ctx):
    return registered(ctx.register_end)


def kernel_normals(ctx, map_points):
    """The library's own normal of every map point by original index, read from its normal cache through a search of the
    map points themselves (carried normals included: `map_normals_owned` would estimate them afresh).  A point that is an
    exact duplicate of a lower index is never a neighbour and keeps NaN."""
    m = np.asarray(map_points, F32)
    out = np.full((len(m), 3), np.nan, F32)
    if len(m):
        _, nm, ix = ctx.nearest_neighbor_search(m, with_normals=True, with_index=True)
        out[ix] = nm
    return out


def observe(ctx, rc, res, n, with_normals=True):
    """What a finished run leaves to look at: last_neighbors FIRST (later calls may touch the cache), then
    the map and the normals.  Returns (record of its last iteration or None when it ran none, map points, normals)."""
    rec = None
    if res.iterations > 0:
        try:
            ix, pose12 = ctx.last_neighbors(n)
        except AssertionError as e:  # the point-to-point cost runs unfused: nothing to read from
            if "no fused registration" not in str(e):
                raise
            ix, pose12 = None, None
        it = res.iterations
        rec = IterationRecord(it, pose12, ix, float(res.losses[it - 1]), res.dx[it - 1].copy(), res.num_targets, rc, it,
                              res.converged, res.pose.copy())
    mp = ctx.map_points()
    nm = kernel_normals(ctx, mp) if with_normals and ctx.config.num_neighbors_normals and rec is not None and \
        rec.ix is not None else None
    return rec, mp, nm


def truncated_runs(make_ctx, targets, init, K, skip_null, register=None):
    """Runs of k = 1 .. K iterations (threshold 0) on fresh contexts `make_ctx(k)` — the map set, max_num_alignments = k —
    each observed through `observe`.  Asserts the prefix property bit for bit (losses[:k] and dx[:k] of run k are those of
    run K) and `handoff_fallbacks() == 0`; returns (records, map points, normals, (status, result) of run K): one record per iteration run K made; the map and
    the normals every run held are asserted equal to run K's.
    `register(ctx, targets, init, skip_null)` -> (status, result): raw_register by default."""
    register = register or raw_register
    n = int(np.asarray(targets).shape[0])
    runs = []
    for k in range(1, K + 1):
        ctx = make_ctx(k)
        assert ctx.config.max_num_alignments == k and ctx.config.threshold_delta_pose == 0.0
        rc, res = register(ctx, targets, init, skip_null)
        rec, mp, nm = observe(ctx, rc, res, n)
        assert ctx.handoff_fallbacks() == 0, k
        ctx.close()
        runs.append((rc, res, rec, mp, nm))
    rcK, resK = runs[-1][0], runs[-1][1]
    records = []
    for k, (rc, res, rec, mp, nm) in enumerate(runs, start=1):
        j = min(k, resK.iterations)
        assert res.iterations == j, (k, res.iterations, resK.iterations)
        assert np.array_equal(res.losses, resK.losses[:j]) and np.array_equal(res.dx, resK.dx[:j]), \
            f"a run of {k} iterations is no prefix of the run of {K}"
        assert np.array_equal(mp, runs[-1][3]), k
        assert (nm is None) == (runs[-1][4] is None) and (nm is None or np.array_equal(nm, runs[-1][4], equal_nan=True)), \
            f"the normals run {k} held are not those of run {K}"
        if k <= resK.iterations:
            assert rec is not None and rec.k == k
            assert (rc == ICP_OK) or k == resK.iterations, (k, rc)
            records.append(rec)
        else:  # a guard or an error ended the loop before k: the same result as run K
            assert rc == rcK and np.array_equal(res.pose, resK.pose) and res.converged == resK.converged, k
    if resK.iterations == 0:
        assert rcK == ICP_OK and resK.num_targets == 0
    return records, runs[-1][3], runs[-1][4], (rcK, resK)


def complete_poses(records, init):
    """Records whose pose is not observable (ix None) take it from the chain: the initial pose, then the pose the previous
    run returned (with threshold 0 that IS the pose the next iteration runs with)."""
    out = []
    for r in records:
        if r.pose12 is None:
            prev = np.asarray(init if r.k == 1 else out[-1].pose_after, F32).reshape(4, 4)
            r = replace(r, pose12=prev[:3].copy())
        out.append(r)
    return out


def audit_run(name, records, targets, map_points, normals, scheme, sigma, cost="point_to_plane", skip_null=False,
              init=None, worst=None, duplicates=False, k_normals=10):
    """Every record of a run through audit_iteration, the pose chain between consecutive iterations and into the returned
    pose; prints the figures per iteration, collects every failure and raises them together."""
    records = complete_poses(records, np.eye(4, dtype=F32) if init is None else init)
    m = np.asarray(map_points, F32)
    tree = cKDTree(m.astype(F64)) if len(m) else None
    nref = NormalReference(m, k_normals) if cost == "point_to_plane" and normals is not None and len(m) else None
    low = lowest_index_of_equal_points(m) if duplicates else None
    failures = []
    for i, rec in enumerate(records):
        if i == 0 and init is not None and not np.array_equal(rec.pose12, np.asarray(init, F32).reshape(4, 4)[:3]):
            failures.append(("pose chain", f"{name}: the first iteration ran with another pose than the initial one"))
        nxt = records[i + 1].pose12 if i + 1 < len(records) else rec.pose_after
        if i + 1 < len(records) and not np.array_equal(records[i + 1].pose12, rec.pose_after[:3]):
            failures.append(("pose chain", f"{name}: run {rec.k} returned another pose than iteration {rec.k + 1} ran with"))
        try:
            fig = audit_iteration(rec, targets, m, normals, scheme, sigma, cost, skip_null, nxt, nref, tree, low)
        except AuditFailure as e:
            failures += [(c, f"{name}: {w}") for c, w in e.failures]
            continue
        if worst is not None:
            worst.add(fig, f"{name} it {rec.k}")
        print(f"  {name} it {rec.k}: rows {fig.get('rows')}, |ddx| {fig.get('ddx', 0):.2e} (atol {fig.get('atol', 0):.1e}, "
              f"reference spread {fig.get('spread', 0):.1e}), dloss {fig.get('dloss', 0):.2e}, ties excluded "
              f"{fig.get('mismatches', 0)} ({fig.get('share', 0) * 100:.4f} %), normals used {fig.get('used', 0)} / compared "
              f"{fig.get('clear', 0)}: min |dot| {fig.get('min_dot', 1):.7f}, "
              f"pose chain {max(fig.get('drot', 0), fig.get('dtrans', 0)):.2e}"
              + (", neighbours from the kd-tree" if rec.ix is None else "")
              + (f", STATUS UNDETERMINED by the reference (det {fig['det'][0]:.3e} by LU, {fig['det'][1]:.3e} by Cholesky): "
                 f"the kernel's {rec.status} accepted" if fig.get("status_undetermined") else ""))
        if worst is not None and fig.get("status_undetermined"):
            worst.undetermined.append(f"{name} it {rec.k}")
    if failures:
        raise AuditFailure(failures)


# ----------------------------------------------------------------------------------------------------------------------
# the oracle's own loop (the stand-in for the device in the CPU suite)
# ----------------------------------------------------------------------------------------------------------------------
def oracle_normals(map_points, k=10):
    m = np.asarray(map_points, F32)
    return O.knn_normals(m, cKDTree(m.astype(F64)), np.arange(len(m)), k)


def oracle_records(targets, map_points, normals, init, K, scheme, sigma, cost="point_to_plane", skip_null=False):
    """K forced iterations of register_new_frame on the kd-tree map with the transform of the kernels (transform_fma),
    float64 sums: the records `truncated_runs` would return."""
    t = np.asarray(targets, F32).reshape(-1, 3)
    ok = valid_rows(t, skip_null)
    m = np.asarray(map_points, F32)
    tree = cKDTree(m.astype(F64))
    pose = np.asarray(init, F32).reshape(4, 4).copy()
    records = []
    for k in range(1, K + 1):
        p = transform_fma(t[ok], pose)
        ix = np.full(len(t), -1, np.int64)
        ix[ok] = tree.query(p.astype(F64))[1]
        ref = reference_step(p, m[ix[ok]], normals[ix[ok]] if cost == "point_to_plane" else None, scheme, sigma, cost)
        nxt = pose if (ref["status"] != ICP_OK or ref["stopped"]) else chain_pose(ref["dx"], pose)
        records.append(IterationRecord(k, pose[:3].copy(), ix, ref["loss"], ref["dx"], int(ok.sum()), ref["status"], k,
                                       ref["stopped"], nxt.copy()))
        if ref["status"] != ICP_OK or ref["stopped"]:
            break
        pose = nxt
    return records


# ----------------------------------------------------------------------------------------------------------------------
# case inputs (shared by the CPU census and the device tests)
# ----------------------------------------------------------------------------------------------------------------------
SIZES = (1, 2, 6, 7, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1023, 4097, 32767, 32768)
# sigma per scheme: residuals of the small scene spread over ~1e-3 .. 1e-1 m (ROW_SIGMA: both Huber branches occur)
SCHEME_SIGMA = {"default": 0.5, "least_square": 0.5, "huber": ROW_SIGMA, "exp": 0.1, "neighborhood": 0.3,
                "geman_mcclure": 0.3, "square_geman_mcclure": 0.3, "cauchy": 0.1}
P2P_CASES = (("least_square", 0.5), ("huber", 0.1), ("neighborhood", 0.3))  # test_point_to_point_cost
_CACHE = {}


def small_scene():
    """(scan [32768,3], map [30000,3]) of the size tests: a 32 x 1024 scan against a map of four OTHER scans."""
    if "small" not in _CACHE:
        from pylidar_slam_amd.synthetic import SceneConfig, make_fixed_map, make_sequence
        cfg = SceneConfig(height=32, width=1024)
        scans, poses = make_sequence(cfg, 7)
        _CACHE["small"] = (scans[4], make_fixed_map(cfg, scans[:4], poses[:4], ref_frame=3, num_points=30_000), scans)
    return _CACHE["small"][:2]


def small_sequence():
    """The three scans that follow the map of small_scene (chained frames) and that map."""
    small_scene()
    return [_CACHE["small"][2][f] for f in (4, 5, 6)], _CACHE["small"][1]


def tiny_scene():
    """(scan [4096,3], map) of the CPU suite: 16 x 256."""
    if "tiny" not in _CACHE:
        from pylidar_slam_amd.synthetic import SceneConfig, make_fixed_map, make_sequence
        cfg = SceneConfig(height=16, width=256)
        scans, poses = make_sequence(cfg, 4)
        _CACHE["tiny"] = (scans[3], make_fixed_map(cfg, scans[:3], poses[:3], ref_frame=2, num_points=6_000))
    return _CACHE["tiny"]


def subset(scan, n):
    """n rows of the scan: strided over the whole image where n divides into it, the first n otherwise."""
    s = np.asarray(scan, F32)
    valid = s[valid_rows(s, True)]
    step = len(valid) // n
    out = valid[::step][:n] if step >= 1 and n <= 4097 else valid[:n]
    assert out.shape[0] == n, (n, out.shape)
    return np.ascontiguousarray(out)


def mask_cases(scan):
    """Targets with NaN and (0,0,0) rows (skip_null) that empty whole 128-row and 512-row blocks, straddle their borders,
    leave exactly one valid row in a block, and mask everything.  name -> [n,3]."""
    s = np.asarray(scan, F32)
    out = {}
    a = s.copy()
    a[128:256] = np.nan  # a whole 128-row block
    a[1024:1536] = 0.0  # a whole 512-row block (null rows)
    a[2000:2100] = np.nan  # across the 2048 border
    a[2500:2570] = 0.0  # across the 2560 border
    out["blocks"] = a
    b = s.copy()
    b[3072:3584] = np.nan
    b[3072 + 77] = s[3072 + 77]  # one valid row in a 512-row block
    b[4096:4224] = 0.0
    b[4096 + 127] = s[4096 + 127]  # one valid row, the last of a 128-row block
    b[::2][5000:5100] = np.nan
    out["one_left"] = b
    c = np.full_like(s, np.nan)
    c[1::2] = 0.0
    out["all_masked"] = c
    return out


def c2_inputs():
    """Scan / map pair of the C2 parity tests (the inputs oracle/make_golden_c2.py ran the reference on)."""
    if "c2" not in _CACHE:
        from pylidar_slam_amd.synthetic import SceneConfig, make_fixed_map, make_sequence
        cfg = SceneConfig(height=64, width=2048)
        scans, poses = make_sequence(cfg, 9)
        _CACHE["c2"] = (scans[8], make_fixed_map(cfg, scans[:8], poses[:8], ref_frame=7, num_points=100_000))
    return _CACHE["c2"]


def bench_workload():
    """bench.py's headline workload (`make_workload(0, "pingpong")`): tracked scans the map has never seen, the map the
    voxel-subsampled union of eight OTHER scans — restated here so that the tests do not import the benchmark."""
    if "bench" not in _CACHE:
        from pylidar_slam_amd.synthetic import SceneConfig, make_fixed_map, make_sequence
        cfg = SceneConfig(height=64, width=2048, seed=1234, step=0.2, yaw_rate=0.005)
        scans, poses = make_sequence(cfg, 16)
        even = list(range(0, 16, 2))
        model = make_fixed_map(cfg, [scans[f] for f in even], poses[even], ref_frame=0, num_points=100_000)
        rel = np.linalg.inv(poses[1]) @ poses[0]
        model = (model.astype(F64) @ rel[:3, :3].T + rel[:3, 3]).astype(F32)
        _CACHE["bench"] = ({f: scans[f] for f in (3, 5, 7)}, poses, model)
    return _CACHE["bench"]


def full_size_variant(case):
    """(targets, map, options) of test_full_size_variants: more rows than pixels as a plain cloud, carry_normals 0, the
    option set of the benchmark's batched leg."""
    if case.startswith("rows_"):
        scan, model = c2_inputs()
        n = int(case.split("_")[1])
        extra = scan[: n - scan.shape[0]] + F32(0.01)  # (other points than the first ones: no equal rows)
        return np.ascontiguousarray(np.concatenate([scan, extra])), model, {}
    scans, _, model = bench_workload()
    return scans[3], model, ({"carry_normals": 0} if case == "no_carry" else {"wide_until": 0, "cell_lists": 1})


def far_targets():
    """The recipe of test_targets_far_from_the_map_in_the_fused_kernel: a sparse frame with targets 1-6 m and hundreds of
    metres from every map point.  (frame [131072,3], map)."""
    if "far" not in _CACHE:
        scans, _, model = bench_workload()
        rng = np.random.default_rng(3)
        frame = np.full((131072, 3), np.nan, F32)
        keep = rng.choice(131072, 6000, replace=False)
        frame[keep] = scans[3][keep]
        far = rng.choice(keep, 60, replace=False)
        frame[far[:40], 2] += rng.uniform(1.5, 6.0, 40).astype(F32)
        frame[far[40:52]] += F32(40.0)
        frame[far[52:]] = (rng.normal(size=(8, 3)) * 50 + 400).astype(F32)
        _CACHE["far"] = (frame, model)
    return _CACHE["far"]


MAP_CASES = ("five_points", "eleven_points", "duplicates", "offset_1km", "offset_10km")
POSE_CASES = {"yaw_3rad": [0, 0, 0, 0, 0, 3.0], "pitch_half_pi": [0, 0, 0, 0, float(F32(np.pi / 2)), 0],
              "far_off": [0.5, 0, 0, 0, 0, 0.05]}


def map_case(case):
    """(map, targets, initial pose) of test_maps."""
    scan, model = small_scene()
    rng = np.random.default_rng(5)
    init, targets = np.eye(4, dtype=F32), subset(scan, 4097)
    if case in ("five_points", "eleven_points"):
        m = 5 if case == "five_points" else 11
        model = np.ascontiguousarray(model[rng.choice(len(model), m, replace=False)])
        targets = subset(scan, 512)
    elif case == "duplicates":
        rep = np.repeat(model[:500], rng.integers(2, 6, 500), axis=0)  # 500 points held two to five times, anywhere
        model = np.ascontiguousarray(np.concatenate([model[500:], rep])[rng.permutation(len(rep) + len(model) - 500)])
    else:
        shift = np.array([1000.0, -1000.0, 100.0] if case == "offset_1km" else [10000.0, -10000.0, 100.0], F64)
        g = np.eye(4)
        g[:3, 3] = shift
        small = O.build_pose_matrix(np.array([0.1, -0.05, 0.02, 0.002, -0.003, 0.01], F64), F64)
        init = (g @ small @ np.linalg.inv(g)).astype(F32)
        model = (model.astype(F64) + shift).astype(F32)
        targets = (targets.astype(F64) + shift).astype(F32)
    return model, targets, init


def pose_case(case):
    """(targets, initial pose) of test_initial_poses: the scan turned the other way, so that the initial pose brings it
    back onto the map (the far-off pose: the scan as it is)."""
    scan, _ = small_scene()
    params = POSE_CASES[case]
    targets = scan[valid_rows(scan, True)]
    if case != "far_off":
        back = np.linalg.inv(O.build_pose_matrix(np.array(params, F64), F64))
        targets = (targets.astype(F64) @ back[:3, :3].T).astype(F32)
    return np.ascontiguousarray(targets), O.build_pose_matrix(np.array(params, F32))


def plane_case(side=64):
    """(map, targets) of the Invalid-Jacobian guard: a jittered grid on z = 0 and every fifth point of it lifted."""
    ax = np.arange(side, dtype=F32) * F32(0.25)
    plane = np.stack(np.meshgrid(ax, ax, indexing="ij"), axis=-1).reshape(-1, 2)
    plane = plane + np.random.default_rng(9).uniform(-0.05, 0.05, plane.shape).astype(F32)  # (no lattice ties)
    pmap = np.ascontiguousarray(np.concatenate([plane, np.zeros((len(plane), 1), F32)], axis=1).astype(F32))
    return pmap, np.ascontiguousarray(pmap[::5] + np.array([0.06, -0.04, 0.125], F32))


def census(targets, map_points, init, scheme, sigma, skip_null=True, cost="point_to_plane"):
    """What the first iteration of a case exercises, by the oracle's own values: the residual_census of projective_cases
    plus far rows (> 1 m from the map) and 128- / 512-row blocks without a valid row."""
    from projective_cases import residual_census
    t = np.asarray(targets, F32).reshape(-1, 3)
    ok = valid_rows(t, skip_null)
    m = np.asarray(map_points, F32)
    out = dict(valid=int(ok.sum()), quadratic=0, linear=0, clamped=0, zero=0, far=0)
    for b in (128, 512):
        pad = np.concatenate([ok, np.zeros((-len(ok)) % b, bool)]).reshape(-1, b)
        out[f"empty_{b}"] = int((~pad.any(axis=1)).sum())
        out[f"single_{b}"] = int((pad.sum(axis=1) == 1).sum())
    if ok.any():
        p = transform_fma(t[ok], np.asarray(init, F32).reshape(4, 4))
        tree = cKDTree(m.astype(F64))
        d, ix = tree.query(p.astype(F64), workers=-1)
        nrm = O.knn_normals(m, tree, np.unique(ix), 10)
        nn = nrm[np.searchsorted(np.unique(ix), ix)]
        if cost == "point_to_plane":
            out.update(residual_census((m[ix], nn, p), sigma))
        else:  # the point-to-point residual is the distance itself
            a = np.linalg.norm((p - m[ix]).astype(F32), axis=1)
            out.update(quadratic=int((a < F32(sigma)).sum()), linear=int((a >= F32(sigma)).sum()),
                       clamped=int(((a < F32(1.0e-4)) & (a > 0)).sum()), zero=int((a == 0).sum()))
        out["far"] = int((d > 1.0).sum())
    return out
