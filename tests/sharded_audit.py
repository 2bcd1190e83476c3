"""Audit of the scan-sharded registration, shard by shard (tests/test_sharded_audit.py on the CPU,
tests/test_gpu_sharded_audit.py on the device).  TEST INFRASTRUCTURE: numpy + scipy + torch tensors + the other audit
modules of tests/, importable without a GPU, never imported by the package.

The multi-GPU seam — icp_register_begin / icp_iteration_accumulate / icp_normal_equations_ptr /
icp_set_normal_equations_buffer / icp_iteration_solve, driven by `distributed.sharded_register` and reproduced by
k_sum_exchange_solve — needs no second GPU to be held to a model: `SimulatedWorld` holds W contexts with the same map in
ONE process, gives each its slice of the scan and does the all-reduce itself, in float64 and in rank order (`s = 0.0;
s += neq_r`, the order k_sum_exchange_solve documents).  Runs of k = 1 .. K forced iterations are bit-for-bit prefixes of
each other (`audit_world` asserts it), so run k - 1 returns the pose iteration k ran with, and `shard_model` recomputes the
30 sums of every shard at that pose from the map, the library's own normals and the shard's rows alone — the row model is
iteration_audit.weighted_rows, nothing is restated here.  Every check is a function of its own and fails by its name:

  A  per shard      "A row count" exact; "A sums": each of the 29 sums within 2 n 2^-53 sum |a_i b_i| (n the shard's valid
                    rows; + alignment_audit.TRANSCENDENTAL_BOUND for exp / neighborhood / cauchy: the bound of the
                    projective audit); "A empty shard": a shard without valid rows gives exact zeros in elements 0 .. 29;
                    "A pad": elements 30 and 31 are 0.0 (include/icp_mi355x.h);
  B  additivity     "B count" / "B additivity": the rank-order total against the vector ONE context accumulates from the
                    whole scan at the same pose, the same bound with n the whole scan's valid rows, the count exactly;
  C  the solve      "C step": dx of every rank within half a float32 ulp + MARGIN x the spread of three float64 solves
                    (inv(H) g, Cholesky, LU) of the total the test itself wrote; "C loss": the loss bit-equal to element 27
                    of that total (28 behind the residual guard); "C status": status, guards, stop and `iterations` exact;
  D  ranks agree    "D ranks agree": pose, params, losses, dx, iterations, converged, status of all W results bit-equal;
  E  one rank       "E one rank": W = 1 through the seam bit-equal to `register` / to the in-library exchange at world 1;
  F  neighbours     "F neighbours": rows whose float32 nearest neighbour is not unique within iteration_audit.TIE_RTOL /
                    TIE_ABS are flagged — the sums of a shard that holds one are not determined by the model, and A / B
                    are not applied to it; their share is capped at iteration_audit.MISMATCH_CAP (a condition on the
                    case: the clouds of the device tests flag none, which the CPU suite asserts).

Elements 27 (sum (w r)^2) and 28 (sum r^2) are defined by the kernel that forms the rows: the fused iteration kernels add
the float64 product of the two float32 operands (gn_device.h::neq_operands), RowAcc::add_row of the unfused and the
point-to-point path adds the FLOAT32 squares (gauss_newton.hip) — `squares32` says which; the two differ by the rounding
of each square, 1e-8 relative, far outside the summation bound.
"""
import math
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np
import torch
from scipy.spatial import cKDTree

import iteration_audit as IA
from alignment_audit import MARGIN, TRANSCENDENTAL_BOUND, TRI, U
from iteration_audit import ICP_ERR_INVALID_JACOBIAN, ICP_OK, AuditFailure, pose44
from projective_cases import transform_fma
from projective_iteration_audit import norm32

F32, F64 = np.float32, np.float64
NEQ, NEQ_USED = 32, 30
RESULT_FIELDS = ("pose", "params", "losses", "dx", "iterations", "converged")
# the cuts distributed.shard_bounds makes: (n, world)
BOUNDS_CUTS = ((1, 1), (1, 2), (5, 8), (7, 3), (513, 2), (1025, 4), (4096, 3), (4097, 8))
# ... and cuts it never makes but the C ABI allows: shard sizes
ABI_CUTS = {"1+4095": (1, 4095), "4095+1": (4095, 1), "0+4096": (0, 4096), "2048+0+2048": (2048, 0, 2048)}


# ----------------------------------------------------------------------------------------------------------------------
# the simulated world
# ----------------------------------------------------------------------------------------------------------------------
@dataclass
class WorldRun:
    parts: List[np.ndarray]  # per driver iteration [W, 32] f64: every rank's vector behind its accumulate
    totals: List[np.ndarray]  # per driver iteration [32] f64: what the world wrote into every rank's vector
    results: list  # W x (status, result)


def ended(call):
    """(status, result) of a `register_end`: an Invalid Jacobian is raised with the result up to the failing iteration."""
    try:
        return ICP_OK, call()
    except RuntimeError as e:
        if getattr(e, "result", None) is None:
            raise
        return ICP_ERR_INVALID_JACOBIAN, e.result


class SimulatedWorld:
    """W engines (IcpContext, or anything with register_begin / iteration_accumulate / normal_equations_tensor /
    iteration_solve / register_end) holding the same map, each bound to torch's current stream as in `sharded_register`;
    the all-reduce is torch arithmetic on that stream."""

    def __init__(self, contexts):
        self.contexts = list(contexts)
        for c in self.contexts:
            if hasattr(c, "use_torch_stream"):
                c.use_torch_stream()
        self.neq = [c.normal_equations_tensor() for c in self.contexts]

    def total(self, parts):
        """The all-reduce: float64, rank order."""
        s = torch.zeros_like(parts[0])
        for p in parts:
            s += p
        return s

    def run(self, shards, init, iterations, skip_null=False) -> WorldRun:
        assert len(shards) == len(self.contexts)
        for c, rows in zip(self.contexts, shards):
            c.register_begin(rows, init, skip_null=skip_null)
        rec_parts, rec_totals = [], []
        for _ in range(iterations):
            for c in self.contexts:
                c.iteration_accumulate()
            parts = [t.clone() for t in self.neq]
            total = self.total(parts)
            for t in self.neq:
                t.copy_(total)
            for c in self.contexts:
                c.iteration_solve()
            rec_parts.append(torch.stack(parts))
            rec_totals.append(total.clone())
        results = [ended(c.register_end) for c in self.contexts]
        return WorldRun([p.cpu().numpy() for p in rec_parts], [t.cpu().numpy() for t in rec_totals], results)


def cut(rows, sizes):
    """Contiguous shards of the given sizes."""
    rows = np.asarray(rows, F32).reshape(-1, 3)
    assert sum(sizes) == len(rows), (sizes, len(rows))
    edges = np.concatenate([[0], np.cumsum(sizes)])
    return [np.ascontiguousarray(rows[edges[r]:edges[r + 1]]) for r in range(len(sizes))]


def bounds_cut(rows, world):
    from pylidar_slam_amd.distributed import shard_bounds
    rows = np.asarray(rows, F32).reshape(-1, 3)
    return [np.ascontiguousarray(rows[slice(*shard_bounds(len(rows), world, r))]) for r in range(world)]


# ----------------------------------------------------------------------------------------------------------------------
# the model of one shard at one pose
# ----------------------------------------------------------------------------------------------------------------------
def nn_f32(queries, model, tree, k=8):
    """iteration_audit.brute_force_nn_f32 without its n x m table: the float32 squared distances d2 = (dx dx + dy dy) +
    dz dz of the k nearest points by the kd-tree, the lowest index of the smallest (the CPU suite asserts the same
    indices as the brute force); and which rows have a second candidate within TIE_RTOL / TIE_ABS of it (`flagged`)."""
    q, m = np.asarray(queries, F32), np.asarray(model, F32)
    if not len(q):
        return np.zeros(0, np.int64), np.zeros(0, bool)
    k = min(k, len(m))
    _, cand = tree.query(q.astype(F64), k=k, workers=-1)
    cand = np.sort(cand.reshape(len(q), k), axis=1)  # ascending index: argmin takes the lowest of equal distances
    d = q[:, None, :] - m[cand]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    best = d2.argmin(axis=1)
    rows = np.arange(len(q))
    b = d2[rows, best].astype(F64)
    flagged = np.zeros(len(q), bool)
    if k > 1:
        rest = d2.astype(F64)
        rest[rows, best] = np.inf
        second = rest.min(axis=1)
        flagged = (second - b <= IA.TIE_ABS) | (second - b <= IA.TIE_RTOL * b)
    return cand[rows, best], flagged


def shard_model(map_points, normals, tree, rows, skip_null, pose12, scheme, sigma, cost="point_to_plane", squares32=False):
    """dict(sums [30] f64, asum [30] = sum |terms|, tol [30], n, flagged) of one shard at one pose."""
    t = np.asarray(rows, F32).reshape(-1, 3)
    ok = IA.valid_rows(t, skip_null)
    n = int(ok.sum())
    sums, asum = np.zeros(NEQ_USED), np.zeros(NEQ_USED)
    flagged = 0
    if n:
        p = transform_fma(t[ok], pose44(pose12))
        ix, tie = nn_f32(p, map_points, tree)
        flagged = int(tie.sum())
        m = np.asarray(map_points, F32)
        nrm = np.asarray(normals, F32)[ix] if cost == "point_to_plane" else None
        rw, jw, raw = IA.weighted_rows(p, m[ix], nrm, scheme, sigma, cost)
        ja, ra = jw.astype(F64), rw.astype(F64)
        terms = [ja[:, a] * ja[:, b] for a, b in TRI] + [ja[:, a] * ra for a in range(6)]
        terms.append((rw * rw).astype(F64) if squares32 else ra * ra)
        with np.errstate(all="ignore"):
            for e, term in enumerate(terms):
                sums[e] = math.fsum(term) if np.isfinite(term).all() else term.sum()
                asum[e] = math.fsum(np.abs(term)) if np.isfinite(term).all() else np.abs(term).sum()
        if squares32:  # sum r^2 of the float32 squares: the unweighted residual is the weighted one of `least_square`
            r = IA.weighted_rows(p, m[ix], nrm, "least_square", sigma, cost)[0]
            sums[28] = asum[28] = math.fsum((r * r).astype(F64))
        else:
            sums[28] = asum[28] = raw
        sums[29] = asum[29] = n
    tol = 2.0 * n * U * asum
    if scheme in TRANSCENDENTAL_BOUND:
        tol[:28] += TRANSCENDENTAL_BOUND[scheme] * asum[:28]
    tol[29] = 0.0
    return dict(sums=sums, asum=asum, tol=tol, n=n, flagged=flagged)


def _ratio(diff, tol):
    with np.errstate(all="ignore"):
        r = np.where(diff == 0, 0.0, diff / np.where(tol > 0, tol, np.inf))
        return float(np.nanmax(np.where((diff > 0) & (tol == 0), np.inf, r)))


# ----------------------------------------------------------------------------------------------------------------------
# the checks: each returns (failures [(check, why)], figures)
# ----------------------------------------------------------------------------------------------------------------------
def check_shard(k, rank, vec, model):
    """A: one rank's vector behind its accumulate against the model of its shard."""
    vec = np.asarray(vec, F64)
    fails, fig = [], dict(a_ratio=0.0)
    who = f"iteration {k} rank {rank}"
    if not (np.isfinite(vec[30:]).all() and (vec[30:] == 0).all()):
        fails.append(("A pad", f"{who}: elements 30, 31 are {vec[30:]!r}, not 0.0"))
    if vec[29] != model["n"]:
        return fails + [("A row count", f"{who}: {vec[29]!r} rows summed, {model['n']} valid")], fig
    if model["n"] == 0:
        if (vec[:NEQ_USED] != 0).any() or np.signbit(vec[:NEQ_USED]).any():
            fails.append(("A empty shard", f"{who}: a shard without valid rows left {vec[:NEQ_USED][vec[:NEQ_USED] != 0]!r}"))
        return fails, fig
    if model["flagged"]:  # (not determined by the model: check F holds the case to account)
        return fails, fig
    with np.errstate(all="ignore"):
        diff = np.abs(vec[:29] - model["sums"][:29])
        bad = ~(diff <= model["tol"][:29])
    fig["a_ratio"] = _ratio(diff, model["tol"][:29])
    if bad.any():
        e = int(np.argmax(bad))
        fails.append(("A sums", f"{who}: {bad.sum()} of 29 sums beyond their bound, first element {e}: {vec[e]!r} vs "
                                f"{model['sums'][e]!r} (bound {model['tol'][e]:.3e})"))
    return fails, fig


def check_additivity(k, total, whole, models, scheme):
    """B: the rank-order total against the vector one context accumulated from the whole scan at the same pose."""
    total, whole = np.asarray(total, F64), np.asarray(whole, F64)
    n = sum(m["n"] for m in models)
    fails, fig = [], dict(b_ratio=0.0)
    if total[29] != whole[29] or total[29] != n:
        return [("B count", f"iteration {k}: the total counts {total[29]!r} rows, the whole scan {whole[29]!r}, the model "
                            f"{n}")], fig
    if any(m["flagged"] for m in models):
        return fails, fig
    asum = np.sum([m["asum"] for m in models], axis=0) * (1.0 + TRANSCENDENTAL_BOUND.get(scheme, 0.0))
    tol = 2.0 * n * U * asum[:29]
    with np.errstate(all="ignore"):
        diff = np.abs(total[:29] - whole[:29])
        bad = ~(diff <= tol)
    fig["b_ratio"] = _ratio(diff, tol)
    if bad.any():
        e = int(np.argmax(bad))
        fails.append(("B additivity", f"iteration {k}: {bad.sum()} of 29 sums of the total beyond their bound of the whole "
                                      f"scan's, first element {e}: {total[e]!r} vs {whole[e]!r} (bound {tol[e]:.3e})"))
    return fails, fig


def solve_total(total):
    """The float64 step of a 32-vector three ways.  dict(stopped, invalid, undetermined, dx64 [6], bar [6], spread, det)."""
    v = np.asarray(total, F64)
    out = dict(stopped=False, invalid=False, undetermined=False, dx64=np.zeros(6), bar=np.zeros(6), spread=0.0,
               det=(0.0, 0.0))
    if np.sqrt(v[28]) < 1.0e-7:  # (gauss_newton_from_neq: the residual guard comes first, whatever the count)
        out["stopped"] = True
        return out
    H = np.zeros((6, 6))
    for e, (a, b) in enumerate(TRI):
        H[a, b] = H[b, a] = v[e]
    g = v[21:27]
    if not np.isfinite(H).all():
        out.update(invalid=True, det=(np.nan, np.nan))
        return out
    det_lu = float(np.linalg.det(H))
    try:
        L = np.linalg.cholesky(H)
        det_ch = float(np.prod(np.diag(L) ** 2))
    except np.linalg.LinAlgError:
        L, det_ch = None, 0.0
    out["det"] = (det_lu, det_ch)
    out["invalid"] = abs(det_lu) < 1.0e-7
    out["undetermined"] = (abs(det_lu) < 1.0e-7) != (abs(det_ch) < 1.0e-7)
    if out["invalid"] and not out["undetermined"]:
        return out
    try:
        ways = [-(np.linalg.inv(H) @ g), -np.linalg.solve(H, g)]
        if L is not None:
            ways.append(-np.linalg.solve(L.T, np.linalg.solve(L, g)))
    except np.linalg.LinAlgError:
        out["invalid"] = True
        return out
    out["dx64"] = ways[0]
    out["spread"] = float(max(np.abs(a - b).max() for a in ways for b in ways))
    out["bar"] = 0.5 * np.spacing(np.abs(ways[0]).astype(F32)).astype(F64) + MARGIN * out["spread"]
    return out


def check_solve(k, total, results, threshold=0.0, max_iterations=None):
    """C: iteration k of every rank against the float64 solve of the total the world wrote."""
    v = np.asarray(total, F64)
    sol = solve_total(v)
    fails, fig = [], dict(c_ratio=0.0, spread=sol["spread"], c_bar=float(sol["bar"].max()))
    for rank, (rc, res) in enumerate(results):
        who = f"iteration {k} rank {rank}"
        if res.iterations < k:
            fails.append(("C status", f"{who}: the run ended at iteration {res.iterations}"))
            continue
        dx, loss = np.asarray(res.dx[k - 1], F32), float(res.losses[k - 1])
        invalid_out = rc == ICP_ERR_INVALID_JACOBIAN and res.iterations == k
        invalid = invalid_out if sol["undetermined"] else sol["invalid"]
        if invalid != invalid_out or rc not in (ICP_OK, ICP_ERR_INVALID_JACOBIAN):
            fails.append(("C status", f"{who}: status {rc} at iteration {res.iterations}, the total's determinant "
                                      f"{sol['det'][0]:.3e} by LU, {sol['det'][1]:.3e} by Cholesky"))
            continue
        if invalid or sol["stopped"]:
            what, e = ("Invalid Jacobian", 27) if invalid else ("residual guard", 28)
            if np.any(dx != 0) or res.iterations != k or bool(res.converged) != (not invalid):
                fails.append(("C status", f"{who}: {what} with dx {dx}, iterations {res.iterations}, converged "
                                          f"{res.converged}"))
            if loss != v[e]:
                fails.append(("C loss", f"{who}: {what}: the loss {loss!r} is not element {e} of the total, {v[e]!r}"))
            if res.num_targets != int(v[29]):
                fails.append(("C status", f"{who}: num_targets {res.num_targets}, the total counts {v[29]!r}"))
            continue
        d = np.abs(dx.astype(F64) - sol["dx64"])
        fig["c_ratio"] = max(fig["c_ratio"], _ratio(d, sol["bar"]))
        if not (d <= sol["bar"]).all():
            a = int(np.argmax(d - sol["bar"]))
            fails.append(("C step", f"{who}: |ddx| {d[a]:.3e} in component {a}, bar {sol['bar'][a]:.3e}: dx {dx} vs "
                                    f"{sol['dx64']}"))
        if loss != v[27]:
            fails.append(("C loss", f"{who}: the loss {loss!r} is not element 27 of the total, {v[27]!r}"))
        stop = norm32(dx) < float(F32(threshold))
        last = stop or (max_iterations is not None and k >= max_iterations)
        if (last and (res.iterations != k or bool(res.converged) != stop)) or (not last and res.iterations <= k):
            fails.append(("C status", f"{who}: |dx| {norm32(dx):.3e} against the threshold {threshold:.3e}, but converged "
                                      f"{res.converged}, iterations {res.iterations}"))
        if res.iterations == k and res.num_targets != int(v[29]):
            fails.append(("C status", f"{who}: num_targets {res.num_targets}, the total counts {v[29]!r}"))
    return fails, fig


def same_bits(a, b):
    """The fields of two (status, result) that differ in any bit."""
    out = [] if a[0] == b[0] else ["status"]
    for f in RESULT_FIELDS:
        x, y = np.asarray(getattr(a[1], f)), np.asarray(getattr(b[1], f))
        if x.shape != y.shape or x.dtype != y.dtype or x.tobytes() != y.tobytes():
            out.append(f)
    return out


def check_ranks_agree(results, what=""):
    """D."""
    fails = []
    for rank in range(1, len(results)):
        diff = same_bits(results[0], results[rank])
        if diff:
            fails.append(("D ranks agree", f"{what}rank {rank} differs from rank 0 in {', '.join(diff)}: iterations "
                                           f"{results[rank][1].iterations} / {results[0][1].iterations}, status "
                                           f"{results[rank][0]} / {results[0][0]}"))
    return fails


def check_one_rank(seam, other, what):
    """E: W = 1 through the seam against `register` / the in-library exchange at world 1 on the same rows."""
    diff = same_bits(seam, other)
    return [("E one rank", f"the seam at W = 1 differs from {what} in {', '.join(diff)}")] if diff else []


def check_exchange_order(world_result, exchange_result, what="the exchange"):
    """The rank-order sum is the contract of k_sum_exchange_solve: its result against the world's rank 0, bit for bit.
    (B cannot see the order of the W additions: any order is within its bound.)"""
    diff = same_bits(world_result, exchange_result)
    return [("exchange order", f"{what} differs from the simulated world in {', '.join(diff)}")] if diff else []


def check_neighbours(k, models):
    """F."""
    n, flagged = sum(m["n"] for m in models), sum(m["flagged"] for m in models)
    fig = dict(flagged=flagged, share=flagged / n if n else 0.0)
    if n and flagged / n > IA.MISMATCH_CAP:
        return [("F neighbours", f"iteration {k}: {flagged} of {n} rows have no unique float32 neighbour")], fig
    return [], fig


def check_prefix(runs):
    """Run k is a bit-for-bit prefix of run K: vectors, totals, losses, dx; a run that ended early (a guard, an error)
    returns what every longer run returns."""
    fails = []
    last = runs[-1]
    itK = last.results[0][1].iterations
    for k, run in enumerate(runs, start=1):
        j = min(k, itK)
        for rank, (rc, res) in enumerate(run.results):
            rcK, resK = last.results[rank]
            if res.iterations != min(k, resK.iterations) or np.asarray(res.losses).tobytes() != \
                    np.asarray(resK.losses[:res.iterations]).tobytes() or \
                    np.asarray(res.dx).tobytes() != np.asarray(resK.dx[:res.iterations]).tobytes():
                fails.append(("prefix", f"rank {rank}: a run of {k} iterations is no prefix of the run of {len(runs)}"))
            elif k > resK.iterations and same_bits((rc, res), (rcK, resK)):
                fails.append(("prefix", f"rank {rank}: run {k} behind the end of the loop differs from run {len(runs)}"))
        for i in range(j):
            if run.parts[i].tobytes() != last.parts[i].tobytes() or run.totals[i].tobytes() != last.totals[i].tobytes():
                fails.append(("prefix", f"run {k}: the vectors of iteration {i + 1} are not those of run {len(runs)}"))
    return fails


class Worst:
    """The worst figure of every check over a family of cases, printed by the tests and quoted in their docstrings."""

    def __init__(self, name):
        self.name, self.n, self.shards = name, 0, 0
        self.f = dict(a_ratio=0.0, b_ratio=0.0, c_ratio=0.0, c_bar=0.0, spread=0.0, flagged=0, share=0.0, chain=0.0)

    def add(self, fig):
        for key, v in fig.items():
            if key in self.f and np.isfinite(v):
                self.f[key] = max(self.f[key], v)

    def __str__(self):
        f = self.f
        return (f"{self.name}: {self.n} iterations, {self.shards} shard vectors audited; A sums at {f['a_ratio']:.3f} of "
                f"their bound, B total at {f['b_ratio']:.3f} of its bound, C |ddx| at {f['c_ratio']:.3f} of its bar (largest "
                f"bar {f['c_bar']:.2e}, largest spread {f['spread']:.2e}), F {f['flagged']} rows flagged (share "
                f"{f['share']:.2e}), pose chain {f['chain']:.2e}")


def whole_vector(engine, rows, pose, skip_null):
    """What ONE engine accumulates from the whole scan at `pose` (no solve; the registration is ended at once)."""
    neq = engine.normal_equations_tensor()
    engine.register_begin(rows, pose, skip_null=skip_null)
    engine.iteration_accumulate()
    out = neq.clone().cpu().numpy()
    ended(engine.register_end)
    return out


def audit_world(name, make_world, whole, map_points, normals, shards, init, K, scheme, sigma, cost="point_to_plane",
                skip_null=False, squares32=False, worst=None, checks="ABCDF", raise_failures=True):
    """Runs of k = 1 .. K forced iterations on `make_world(k)` (a SimulatedWorld whose engines run k iterations at most,
    threshold 0), the prefix property, then checks A, B (against `whole`, an engine holding the same map; None: not
    applied), C, D, F and the pose chain on every iteration run K made.  Returns (run K, failures); raises them unless
    told otherwise."""
    init = np.eye(4, dtype=F32) if init is None else np.asarray(init, F32).reshape(4, 4)
    m = np.asarray(map_points, F32)
    tree = cKDTree(m.astype(F64))
    runs = [make_world(k).run(shards, init, k, skip_null) for k in range(1, K + 1)]
    fails = check_prefix(runs)
    last = runs[-1]
    made = last.results[0][1].iterations
    scan = np.concatenate([np.asarray(s, F32).reshape(-1, 3) for s in shards]) if len(shards) else np.zeros((0, 3), F32)
    for k in range(1, min(made, K) + 1):
        pose = init if k == 1 else np.asarray(runs[k - 2].results[0][1].pose, F32).reshape(4, 4)
        fig = {}
        models = [shard_model(m, normals, tree, rows, skip_null, pose[:3], scheme, sigma, cost, squares32)
                  for rows in shards]
        if "A" in checks:
            for rank, model in enumerate(models):
                f, g = check_shard(k, rank, last.parts[k - 1][rank], model)
                fails += f
                fig["a_ratio"] = max(fig.get("a_ratio", 0.0), g["a_ratio"])
        if "B" in checks and whole is not None:
            f, g = check_additivity(k, last.totals[k - 1], whole_vector(whole, scan, pose, skip_null), models, scheme)
            fails += f
            fig.update(g)
        if "C" in checks:
            f, g = check_solve(k, last.totals[k - 1], runs[k - 1].results, 0.0, k)
            fails += f
            fig.update(g)
            rc, res = runs[k - 1].results[0]
            if res.iterations >= k:
                rec = IA.IterationRecord(k, pose[:3].copy(), None, float(res.losses[k - 1]), np.asarray(res.dx[k - 1], F32),
                                         res.num_targets, rc, res.iterations, bool(res.converged), np.asarray(res.pose, F32))
                f, g = IA.check_pose_chain(rec, res.pose)
                fails += f
                fig["chain"] = max(g["drot"], g["dtrans"])
        if "D" in checks:
            fails += check_ranks_agree(runs[k - 1].results, f"run {k}: ")
        if "F" in checks:
            f, g = check_neighbours(k, models)
            fails += f
            fig.update(g)
        print(f"  {name} it {k}: rows {[mm['n'] for mm in models]}, A {fig.get('a_ratio', 0):.3f}, B {fig.get('b_ratio', 0):.3f}, "
              f"C {fig.get('c_ratio', 0):.3f} of bar {fig.get('c_bar', 0):.2e} (spread {fig.get('spread', 0):.1e}), flagged "
              f"{fig.get('flagged', 0)}, pose chain {fig.get('chain', 0):.2e}")
        if worst is not None:
            worst.add(fig)
            worst.n += 1
            worst.shards += len(shards)
    if "D" in checks:
        for k in range(made + 1, K + 1):
            fails += check_ranks_agree(runs[k - 1].results, f"run {k}: ")
    if fails and raise_failures:
        raise AuditFailure(fails)
    return last, fails


# ----------------------------------------------------------------------------------------------------------------------
# the stand-in engine of the CPU suite: the model behind the engine protocol
# ----------------------------------------------------------------------------------------------------------------------
class ModelInvalidJacobian(RuntimeError):
    result = None


@dataclass
class ModelResult:
    pose: np.ndarray
    params: np.ndarray
    iterations: int
    converged: bool
    num_targets: int
    losses: np.ndarray
    dx: np.ndarray
    normals_computed: int = 0


def _oracle_engine():
    from test_distributed_gloo import OracleEngine
    return OracleEngine


class _Config:
    max_num_alignments = 1
    threshold_delta_pose = 0.0


def model_engine_class():
    """ModelEngine: tests/test_distributed_gloo.py::OracleEngine (the engine protocol on the oracle) with the row model of
    this audit, the guards, the stop threshold, `done` and the histories of the library.  `wrong`: a deliberately wrong
    copy (tests/test_sharded_audit.py)."""
    base = _oracle_engine()

    class ModelEngine(base):
        def __init__(self, map_points, normals, scheme="geman_mcclure", sigma=0.3, cost="point_to_plane", iterations=1,
                     threshold=0.0, squares32=False, wrong=None):
            self.map = np.asarray(map_points, F32)
            self.normals = np.asarray(normals, F32)
            self.tree = cKDTree(self.map.astype(F64))
            self.scheme, self.sigma, self.cost, self.squares32, self.wrong = scheme, sigma, cost, squares32, wrong
            self.neq = torch.zeros(NEQ, dtype=torch.float64)
            self.config = _Config()
            self.set_alignment(scheme, sigma, iterations, threshold)

        def set_alignment(self, scheme, sigma, max_num_alignments, threshold_delta_pose):
            self.scheme, self.sigma = scheme, sigma
            self.config.max_num_alignments = int(max_num_alignments)
            self.config.threshold_delta_pose = float(F32(threshold_delta_pose))

        def register_begin(self, pts, init_pose=None, skip_null=False):
            self.pts = np.asarray(pts, F32).reshape(-1, 3)
            if self.wrong == "last_row_dropped":
                self.pts = self.pts[:-1]
            self.skip_null = skip_null
            self.pose = np.eye(4, dtype=F32) if init_pose is None else np.asarray(init_pose, F32).reshape(4, 4).copy()
            self.prev_pose = self.pose.copy()
            self.params = np.zeros(6, F32)
            self.losses, self.dxs = [], []
            self.done, self.converged, self.status, self.iter, self.n_targets = False, False, ICP_OK, 0, 0

        def _local(self, pose):
            s = shard_model(self.map, self.normals, self.tree, self.pts, self.skip_null, pose[:3], self.scheme, self.sigma,
                            self.cost, self.squares32)
            return s["sums"]

        def iteration_accumulate(self):
            if self.done and self.wrong != "runs_behind_done":  # (k_sum_partials(check_done = 1): nothing is written)
                return
            if self.wrong == "stale_empty_shard" and not IA.valid_rows(self.pts, self.skip_null).any():
                return  # the vector keeps what it held: the total of the previous iteration
            pose = self.prev_pose if self.wrong == "previous_pose" else self.pose
            v = np.zeros(NEQ)
            v[:NEQ_USED] = self._local(pose)
            self.local = v
            self.neq.copy_(torch.from_numpy(v))

        def iteration_solve(self):
            if self.done and self.wrong != "runs_behind_done":
                return
            v = self.neq.numpy().copy()
            if self.wrong == "solves_local_sums":
                v = self.local.copy()
            sol = solve_total(v)
            stop_by = solve_total(self.local) if self.wrong == "local_stop" else sol
            dx = np.zeros(6, F32) if (sol["invalid"] or sol["stopped"]) else sol["dx64"].astype(F32)
            self.losses.append(float(v[28] if sol["stopped"] else v[27]))
            self.dxs.append(dx)
            self.n_targets = int(v[29])
            self.iter += 1
            if sol["invalid"] and not sol["stopped"]:
                self.status, self.done = ICP_ERR_INVALID_JACOBIAN, True
                return
            dx_stop = dx if stop_by is sol else stop_by["dx64"].astype(F32)
            if sol["stopped"] or norm32(dx_stop) < self.config.threshold_delta_pose:
                self.done = self.converged = True
                return
            self.prev_pose = self.pose
            self.pose = IA.chain_pose(dx, self.pose[:3])
            if self.iter >= self.config.max_num_alignments:
                self.done = True

        def register_end(self):
            k = len(self.losses)
            res = ModelResult(self.pose.copy(), np.asarray(self.params, F32), self.iter, self.converged, self.n_targets,
                              np.array(self.losses, F64), np.array(self.dxs, F32).reshape(k, 6))
            if self.status == ICP_ERR_INVALID_JACOBIAN:
                e = ModelInvalidJacobian("Invalid Jacobian in Gauss Newton minimization")
                e.result = res
                raise e
            return res

        def register(self, pts, init_pose=None, skip_null=False):
            """The single-process registration: the same loop without the seam."""
            self.register_begin(pts, init_pose, skip_null)
            for _ in range(self.config.max_num_alignments):
                self.iteration_accumulate()
                self.iteration_solve()
            return self.register_end()

    return ModelEngine


# ----------------------------------------------------------------------------------------------------------------------
# clouds (shared by the CPU suite and the device tests)
# ----------------------------------------------------------------------------------------------------------------------
_CACHE = {}
MAP_STRIDE = 4  # every fourth point of iteration_audit's 30 000-point maps: 7 500 points


def scene():
    """(scan [32768,3], map [7500,3]): iteration_audit.small_scene with every fourth map point."""
    if "scene" not in _CACHE:
        scan, model = IA.small_scene()
        _CACHE["scene"] = (scan, np.ascontiguousarray(model[::MAP_STRIDE]))
    return _CACHE["scene"]


def cloud(n):
    """n valid rows of the scan, strided over the whole image."""
    return IA.subset(scene()[0], n)


def nan_shard(rows):
    return np.full((rows, 3), np.nan, F32)


def null_shard(rows):
    return np.zeros((rows, 3), F32)


def guard_scene(shift=(300.0, 300.0, 0.0)):
    """(map, plane targets, regular targets): iteration_audit.plane_case moved `shift` away from the scene and appended to
    its map, so that one map serves a shard that is singular alone (rows on the plane z = 0: J = [n, p x n] with n = +-z
    spans three dimensions) and a regular one."""
    if "guard" not in _CACHE:
        pmap, ptargets = IA.plane_case()
        s = np.asarray(shift, F32)
        _CACHE["guard"] = (np.ascontiguousarray(np.concatenate([scene()[1], pmap + s])), np.ascontiguousarray(ptargets + s),
                           cloud(1025))
    return _CACHE["guard"]


def far_scene():
    """(rows with the far targets [<= 2049,3], regular rows, map): iteration_audit.far_targets — a sparse frame with targets
    1-6 m and hundreds of metres from every map point — cut down to the sizes of this audit: every twelfth map point, the
    far rows and their neighbours in the frame on one rank, rows without a far target on the other."""
    if "far" not in _CACHE:
        frame, model = IA.far_targets()
        model = np.ascontiguousarray(model[::12])
        rows = frame[IA.valid_rows(frame, False)]
        d, _ = cKDTree(model.astype(F64)).query(rows.astype(F64), workers=-1)
        far = d > 1.0
        near = np.flatnonzero(~far)
        with_far = np.concatenate([rows[far], rows[near[:1024]]])
        _CACHE["far"] = (np.ascontiguousarray(with_far), np.ascontiguousarray(rows[near[1024:1024 + 1500]]), model,
                         int(far.sum()))
    return _CACHE["far"]


def pose_family(case):
    """(map, targets [4097,3], init) of iteration_audit.pose_case at the sizes of this audit."""
    targets, init = IA.pose_case(case)
    return scene()[1], IA.subset(targets, 4097), init


def map_family(case):
    """(map, targets [4097,3], init) of iteration_audit.map_case at the sizes of this audit."""
    model, targets, init = IA.map_case(case)
    return np.ascontiguousarray(model[::MAP_STRIDE]), targets, init


DEVICE_CLOUDS = ("rows_1", "rows_5", "rows_7", "rows_513", "rows_1025", "rows_1536", "rows_4096", "rows_4097", "guard", "far",
                 "yaw_3rad", "offset_10km")


def device_cloud(name):
    """(map, rows, initial pose) of every cloud tests/test_gpu_sharded_audit.py registers, by name."""
    eye = np.eye(4, dtype=F32)
    if name.startswith("rows_"):
        return scene()[1], cloud(int(name.split("_")[1])), eye
    if name == "guard":
        gmap, plane, regular = guard_scene()
        return gmap, np.concatenate([plane, regular]), eye
    if name == "far":
        with_far, regular, model, _ = far_scene()
        return model, np.concatenate([with_far, regular]), eye
    if name == "yaw_3rad":
        return pose_family(name)
    return map_family(name)


def thresholds_between(norms):
    """Live thresholds halfway between consecutive float32 step norms of a forced run: (threshold, the iteration the run
    must stop at) — the first iteration whose norm is below the threshold."""
    out = []
    for a, b in zip(norms[:-1], norms[1:]):
        if a == b:
            continue
        thr = float(F32(0.5 * (float(a) + float(b))))
        stop = next((i + 1 for i, v in enumerate(norms) if v < thr), None)
        if stop is not None and thr not in [t for t, _ in out]:
            out.append((thr, stop))
    return out


def check_stop(results, stop, held_pose, reference_results):
    """The live stop: every rank stops at iteration `stop`, converged, with the pose iteration `stop` ran with, and the
    driver's remaining calls changed no bit — `reference_results`: the same world driven for exactly `stop` iterations."""
    fails = []
    for rank, (rc, res) in enumerate(results):
        if rc != ICP_OK or res.iterations != stop or not res.converged:
            fails.append(("stop", f"rank {rank}: status {rc}, iterations {res.iterations}, converged {res.converged}; the "
                                  f"step norms name iteration {stop}"))
        elif np.asarray(res.pose, F32).tobytes() != np.asarray(held_pose, F32).reshape(4, 4).tobytes():
            fails.append(("stop", f"rank {rank}: the pose moved behind the stop"))
        diff = same_bits((rc, res), reference_results[rank])
        if diff:
            fails.append(("stop", f"rank {rank}: the calls behind the stop changed {', '.join(diff)}"))
    return fails
