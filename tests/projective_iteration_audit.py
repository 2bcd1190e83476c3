"""Audit of single iterations of the projective registration — k_pm_project_targets, k_pm_iterate and k_sum_solve of
csrc/projective.hip / gauss_newton.hip behind `pmap_register` — (tests/test_projective_iteration_audit.py on the CPU,
tests/test_gpu_projective_iteration_audit.py on the device).  TEST INFRASTRUCTURE: numpy + oracle/icp_oracle.py + the other
audit modules of tests/, importable without a GPU, never imported by the package.

A run of k forced iterations (threshold 0) is a bit-for-bit prefix of a run of K (`truncated_runs` asserts it), the pose run
k - 1 returned is the pose iteration k ran with, and the 30 sums of iteration k are what `normal_equations_tensor()` holds
after run k (`launch_sum_solve` hands ctx->neq to k_sum_solve on this path too: gauss_newton.hip).  `model_iteration`
recomputes the iteration from `pmap_model()`, the target rows, the target mode and that pose alone:

  NaN rows dropped, (0,0,0) rows dropped under skip_null; every row moved by the fma chain (projective_cases.transform_fma);
  its pixel by the bit model of pixel_of (projection_audit.model); per pixel the smallest (float32 range bits, ~row index);
  a moved point that is all zero skipped; the layer the first smallest sqrtf((dx dx + dy dy) + dz dz) over the set layers;
  an all-zero neighbour skipped; rows, float64 sums and step by alignment_audit.seam_step("point_to_plane", q, p, n, ...) —
  but elements 27 (sum (w r)^2) and 28 (sum r^2) as the iteration kernels define them, float64 products of the float32
  operands (neq_operands), not the float32 squares RowAcc::add_row of the alignment seams adds: see model_iteration.

`check_iteration` holds a record to it, every check by its name:

  row count          neq[29] and num_targets, exact;
  normal equations   each of the 29 sums within seam_step's sum_tol (2 n 2^-53 sum |a_i b_i|, + TRANSCENDENTAL_BOUND for
                     exp / neighborhood / cauchy);
  status             Invalid Jacobian and the residual guard as alignment_audit.check_seam treats them;
  step               dx against -(inv(H) g) of the model's sums in float64 within: half a float32 ulp of the model's
                     component + MARGIN x the larger of the model's spreads (inv(H) g against the Cholesky solve; the rows
                     added in the opposite order) + — exp / neighborhood / cauchy — |inv(H)| (|dg| + |dH| |dx|) for sums
                     moved by their TRANSCENDENTAL_BOUND (first order, from the model's own 6x6 system); never above
                     STEP_ATOL.  The loss bit-equal to neq[27] and within sum_tol[27] of the model's;
  pose chain         the pose after against iteration_audit.chain_pose at POSE_ATOL; unchanged, bit for bit, behind a guard;
  undetermined       (a condition on the case, not on the device) a model spread above STEP_CAP outside a guard case.
"""
from dataclasses import dataclass
from typing import Callable, Optional

import numpy as np

import alignment_audit as AA
import icp_oracle as O
import iteration_audit as IA
import projection_audit as PA
import projective_cases as PC
from alignment_audit import MARGIN, STEP_CAP, TRANSCENDENTAL_BOUND
from iteration_audit import ICP_ERR_INVALID_JACOBIAN, ICP_OK, POSE_ATOL, SCHEME_SIGMA, STEP_ATOL, AuditFailure, chain_pose, pose44

F32, F64 = np.float32, np.float64
PM_THREADS = 256  # pixels per workgroup of k_pm_iterate: one partial row each
WRONG = ("stale_zbuffer", "previous_pose", "farther_wins", "tie_lowest_index", "higher_layer", "unset_not_skipped",
         "skip_null_ignored", "last_block_dropped", "quarter_row_dropped", "float32_sums", "wrong_huber_branch",
         "pose_advanced_on_guard")


def blocks_of(h, w):
    """(partial rows, super-rows of sum_partials_vt with quad = 1)."""
    b = -(-h * w // PM_THREADS)
    return b, -(-b // 4)


@dataclass
class Record:
    k: int  # 1-based iteration
    pose12: np.ndarray  # [3,4] f32: the pose the iteration ran with
    neq: Optional[np.ndarray]  # [>= 30] f64: the sums of the iteration; None: not observable
    loss: float
    dx: np.ndarray  # [6] f32
    num_targets: int
    status: int
    iterations: int  # of the run that ended with this iteration
    converged: bool
    pose_after: np.ndarray  # [4,4] f32: the pose the run returned


# ----------------------------------------------------------------------------------------------------------------------
# the model of one iteration
# ----------------------------------------------------------------------------------------------------------------------
def valid_source_rows(targets, skip_null):
    return np.flatnonzero(IA.valid_rows(targets, skip_null))


def model_rows(mv, mn, targets, skip_null, pose12):
    """(q, p, n [m,3] float32 in pixel order, pixels [m], target row of each [m], rows the projection model flags)."""
    mv, mn = np.asarray(mv, F32), np.asarray(mn, F32)
    k, _, h, w = mv.shape
    t = np.asarray(targets, F32).reshape(-1, 3)
    src = valid_source_rows(t, skip_null)
    moved = PC.transform_fma(t[src], pose44(pose12))
    bit = PA.model(moved, h, w, PC.UP_FOV, PC.DOWN_FOV)  # (its pixel, range and flags alone: the winner is taken below)
    cand = np.flatnonzero(bit.pixel >= 0)
    # smallest (range bits << 32 | ~index): the nearest, of equal ranges the HIGHEST row index
    cand = cand[np.lexsort((-src[cand], bit.r[cand].view(np.uint32), bit.pixel[cand]))]
    first = np.ones(len(cand), bool)
    first[1:] = bit.pixel[cand][1:] != bit.pixel[cand][:-1]
    win = cand[first]
    pix = bit.pixel[win]
    p = moved[win]
    lv, ln = mv.reshape(k, 3, -1)[:, :, pix], mn.reshape(k, 3, -1)[:, :, pix]  # [K,3,m]
    is_set = np.abs(lv).max(axis=1) > 0  # (q.w == 1: pmap_build writes a vertex only where a point with r > 0 landed)
    with np.errstate(all="ignore"):
        d = p.T[None] - lv
        dist = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).astype(F32)
    dist = np.where(is_set, dist, F32(np.inf))
    best = dist.argmin(axis=0)  # the first of equal distances
    m = np.arange(len(pix))
    q, n = lv[best, :, m].reshape(-1, 3), ln[best, :, m].reshape(-1, 3)
    ok = is_set.any(axis=0) & (np.abs(p).max(axis=1) > 0) & (np.abs(q).max(axis=1) > 0)
    return q[ok], p[ok], n[ok], pix[ok], src[win][ok], int(bit.flagged.sum())


def _system(sums):
    H = np.zeros((6, 6))
    for e, (a, b) in enumerate(AA.TRI):
        H[a, b] = H[b, a] = sums[e]
    return H, np.array(sums[21:27], F64)


def model_iteration(mv, mn, targets, skip_null, pose12, scheme, sigma):
    """alignment_audit.seam_step of the model's rows + `dx64` (the step before its rounding to float32), `dx_bar` [6] (the
    bar of the step check), `capped` (the derived bar exceeded STEP_ATOL and was cut to it), `flagged`, `pix`."""
    q, p, n, pix, rows_of, flagged = model_rows(mv, mn, targets, skip_null, pose12)
    model = AA.seam_step("point_to_plane", q, p, n, None, scheme, sigma)
    # Elements 27 and 28.  seam_step restates RowAcc::add_row of the alignment seams, which adds the FLOAT32 squares of w r and
    # r.  The iteration kernels (k_pm_iterate here, the fused kd-tree kernel) form every element e as the float64 product of
    # the two float32 operands neq_operands(e) names — 27: (w r)(w r), 28: r r — which is what iteration_audit.reference_step
    # already holds the fused path to (`loss = (ra * ra).sum()`).  The two differ by the rounding of each square (1e-8
    # relative), far outside the summation bound: the model follows the kernel's definition, the bound stays the derived one.
    rows = model["rows"]
    for e, key in ((27, "rw"), (28, "r")):
        sq = rows[key].astype(F64) ** 2
        model["sums"][e] = model["asum"][e] = float(sq.sum())
        model["sum_tol"][e] = 2.0 * model["n"] * AA.U * model["asum"][e] + \
            (TRANSCENDENTAL_BOUND[scheme] * model["asum"][e] if e == 27 and scheme in TRANSCENDENTAL_BOUND else 0.0)
    ref = dict(AA.solve_sums(model["sums"]), order_spread=model["ref"]["order_spread"])
    model["ref"] = ref
    dx64, bar, half_ulp = np.zeros(6), np.zeros(6), np.zeros(6)
    if ref["status"] == ICP_OK and not ref["stopped"] and np.isfinite(model["sums"]).all():
        H, g = _system(model["sums"])
        try:
            hinv = np.linalg.inv(H)
            dx64 = -(hinv @ g)
            half_ulp = 0.5 * np.spacing(np.abs(dx64).astype(F32)).astype(F64)
            bar = half_ulp + MARGIN * max(ref["spread"], ref["order_spread"])
            if scheme in TRANSCENDENTAL_BOUND:
                dH, dg = _system(model["asum"])
                bar = bar + TRANSCENDENTAL_BOUND[scheme] * (np.abs(hinv) @ (dg + dH @ np.abs(dx64)))
        except np.linalg.LinAlgError:
            bar = np.full(6, np.inf)
    # STEP_ATOL caps the bar; the rounding of the returned float32 itself is no tolerance and stays (it exceeds the cap only
    # for a step of more than 2 m / 2 rad: `rounding_beyond_cap`, which the CPU suite allows in the guard cases alone)
    capped = bool((bar > STEP_ATOL).any())
    model.update(dx64=dx64, dx_bar=np.maximum(np.minimum(bar, STEP_ATOL), half_ulp), derived_bar=bar, capped=capped,
                 rounding_beyond_cap=bool((half_ulp > STEP_ATOL).any()), flagged=flagged, pix=pix, target_rows=rows_of, q=q,
                 p=p, normals=n)
    return model


def norm32(dx):
    """sqrtf of the float32 sum of squares, in order (solve_core)."""
    s = F32(0)
    for v in np.asarray(dx, F32):
        s = F32(s + F32(v * v))
    return float(np.sqrt(s))


# ----------------------------------------------------------------------------------------------------------------------
# the checks
# ----------------------------------------------------------------------------------------------------------------------
def check_iteration(rec, model, threshold=0.0, guard_case=False):
    """Returns (failures [(check, why)], figures).  A wrong row count ends the check: nothing else is comparable."""
    ref, n, k = model["ref"], model["n"], rec.k
    fig = dict(rows=n, ddx=0.0, dloss=0.0, sum_ratio=0.0, bar=float(model["dx_bar"].max()), capped=model["capped"],
               spread=max(ref["spread"], ref.get("order_spread", 0.0)), drot=0.0, dtrans=0.0, status_undetermined=False,
               guard=False)
    fails = []
    if model["flagged"]:
        fails.append(("undetermined", f"iteration {k}: the projection model flags {model['flagged']} rows"))
    neq = None if rec.neq is None else np.asarray(rec.neq, F64)
    if (neq is not None and neq[29] != n) or rec.num_targets != n:
        return fails + [("row count", f"iteration {k}: {None if neq is None else neq[29]} rows summed, num_targets "
                                      f"{rec.num_targets}, the model's {n}")], fig
    # the 29 float sums
    if neq is not None:
        with np.errstate(all="ignore"):
            diff = np.abs(neq[:29] - model["sums"][:29])
            tol = model["sum_tol"][:29]
            bad = ~(diff <= tol)
            ratio = np.where(diff == 0, 0.0, diff / np.where(tol > 0, tol, np.inf))
            ratio = np.where((diff > 0) & (tol == 0), np.inf, ratio)
        fig["sum_ratio"] = float(np.nanmax(ratio))
        if bad.any():
            e = int(np.argmax(bad))
            fails.append(("normal equations", f"iteration {k}: {bad.sum()} of 29 sums beyond their bound, first element {e}: "
                                              f"{neq[e]!r} vs {model['sums'][e]!r} (bound {tol[e]:.3e})"))
    # status and guards
    invalid_out = rec.status == ICP_ERR_INVALID_JACOBIAN
    undetermined = (abs(ref["det"][0]) < 1.0e-7) != (abs(ref["det"][1]) < 1.0e-7) and not ref["stopped"]
    fig["status_undetermined"] = bool(undetermined)
    invalid = invalid_out if undetermined else ref["status"] == ICP_ERR_INVALID_JACOBIAN
    moved = False
    if invalid != invalid_out or rec.status not in (ICP_OK, ICP_ERR_INVALID_JACOBIAN):
        fails.append(("status", f"iteration {k}: status {rec.status}, the model's {ref['status']} (det {ref['det'][0]:.3e} by "
                                f"LU, {ref['det'][1]:.3e} by Cholesky)"))
    elif invalid or ref["stopped"]:
        fig["guard"] = True
        what = "Invalid Jacobian" if invalid else "residual guard"
        e = 27 if invalid else 28
        if np.any(rec.dx != 0) or rec.iterations != k or bool(rec.converged) != (not invalid):
            fails.append(("status", f"iteration {k}: {what} with dx {rec.dx}, iterations {rec.iterations}, converged "
                                    f"{rec.converged}"))
        if not abs(rec.loss - model["sums"][e]) <= model["sum_tol"][e]:
            fails.append(("step", f"iteration {k}: {what}: loss {rec.loss!r} vs {model['sums'][e]!r}"))
        if neq is not None and rec.loss != neq[e]:
            fails.append(("step", f"iteration {k}: {what}: the loss {rec.loss!r} is not the sum the iteration formed"))
    else:
        if not guard_case and max(ref["spread"], ref["order_spread"]) > STEP_CAP:
            fails.append(("undetermined", f"iteration {k}: the model's own float64 solves are {ref['spread']:.2e} / "
                                          f"{ref['order_spread']:.2e} apart"))
        if not guard_case and model["rounding_beyond_cap"]:
            fails.append(("undetermined", f"iteration {k}: a step of {np.abs(model['dx64']).max():.1f}: half a float32 ulp of "
                                          f"it is above STEP_ATOL"))
        d =np.abs(rec.dx.astype(F64) - model["dx64"])
        fig["ddx"] = float(d.max())
        fig["dloss"] = abs(rec.loss - model["sums"][27]) / abs(model["sums"][27]) if model["sums"][27] else abs(rec.loss)
        if not (d <= model["dx_bar"]).all():
            a = int(np.argmax(d - model["dx_bar"]))
            fails.append(("step", f"iteration {k}: |ddx| {d[a]:.3e} in component {a}, bar {model['dx_bar'][a]:.3e}: dx {rec.dx} "
                                  f"vs {model['dx64']}"))
        if not abs(rec.loss - model["sums"][27]) <= model["sum_tol"][27]:
            fails.append(("step", f"iteration {k}: loss {rec.loss!r} vs {model['sums'][27]!r} (bound {model['sum_tol'][27]:.3e})"))
        if neq is not None and rec.loss != neq[27]:
            fails.append(("step", f"iteration {k}: the loss {rec.loss!r} is not the sum (w r)^2 the iteration formed, {neq[27]!r}"))
        stop = norm32(rec.dx) < threshold
        moved = not stop
        if bool(rec.converged) != stop or (stop and rec.iterations != k):
            fails.append(("status", f"iteration {k}: |dx| {norm32(rec.dx):.3e} against the threshold {threshold:.3e}, but "
                                    f"converged {rec.converged}, iterations {rec.iterations}"))
    # the pose chain
    got = np.asarray(rec.pose_after, F32).reshape(-1, 4)[:3]
    if not moved:
        if not np.array_equal(got.view(np.uint32), np.asarray(rec.pose12, F32).reshape(3, 4).view(np.uint32)):
            fails.append(("pose chain", f"iteration {k}: the pose moved behind a guard / a stop"))
    else:
        expect = chain_pose(rec.dx, rec.pose12)
        fig["drot"] = float(np.abs(got[:, :3].astype(F64) - expect[:3, :3]).max())
        fig["dtrans"] = float(np.abs(got[:, 3].astype(F64) - expect[:3, 3]).max()) / max(1.0, float(np.abs(expect[:3, 3]).max()))
        if not (fig["drot"] <= POSE_ATOL and fig["dtrans"] <= POSE_ATOL):
            fails.append(("pose chain", f"iteration {k}: rotation off by {fig['drot']:.2e}, translation by {fig['dtrans']:.2e} "
                                        f"x max(1, |t|)"))
    return fails, fig


class Worst:
    """The worst figures of a case family, printed by the tests and quoted in their docstrings."""

    def __init__(self, name):
        self.name, self.n, self.guards, self.capped = name, 0, 0, 0
        self.f = dict(ddx=0.0, dloss=0.0, sum_ratio=0.0, bar=0.0, spread=0.0, drot=0.0, dtrans=0.0)
        self.undetermined = []

    def add(self, fig, label=""):
        self.n += 1
        self.guards += bool(fig["guard"])
        self.capped += bool(fig["capped"])
        for k in self.f:
            if np.isfinite(fig[k]):
                self.f[k] = max(self.f[k], fig[k])
        if fig["status_undetermined"]:
            self.undetermined.append(label)

    def __str__(self):
        f = self.f
        s = (f"{self.name}: {self.n} iterations audited ({self.guards} behind a guard); worst |ddx| {f['ddx']:.2e} (largest bar "
             f"{f['bar']:.2e}, {self.capped} cut to STEP_ATOL; largest model spread {f['spread']:.2e}), dloss {f['dloss']:.2e}, "
             f"worst sum at {f['sum_ratio']:.2e} of its bound, pose chain {max(f['drot'], f['dtrans']):.2e}")
        for label in self.undetermined:
            s += f"\n  status undetermined by the model, the run's accepted: {label}"
        return s


def audit_run(name, records, mv, mn, targets, skip_null, scheme, sigma, init, threshold=0.0, guard_case=False, worst=None,
              quiet=False):
    """Every record through check_iteration, the chain between consecutive records; collects every failure and raises them
    together (AuditFailure.checks names the checks).  Returns the models."""
    failures, models = [], []
    for i, rec in enumerate(records):
        if i == 0 and not np.array_equal(np.asarray(rec.pose12, F32), np.asarray(init, F32).reshape(4, 4)[:3]):
            failures.append(("pose chain", f"{name}: the first iteration ran with another pose than the initial one"))
        if i + 1 < len(records) and not np.array_equal(records[i + 1].pose12, np.asarray(rec.pose_after, F32)[:3]):
            failures.append(("pose chain", f"{name}: run {rec.k} returned another pose than iteration {rec.k + 1} ran with"))
        model = model_iteration(mv, mn, targets, skip_null, rec.pose12, scheme, sigma)
        models.append(model)
        fails, fig = check_iteration(rec, model, threshold, guard_case)
        failures += [(c, f"{name}: {why}") for c, why in fails]
        if fails:
            continue
        if worst is not None:
            worst.add(fig, f"{name} it {rec.k}")
        if not quiet:
            print(f"  {name} it {rec.k}: rows {fig['rows']}, |ddx| {fig['ddx']:.2e} (bar {fig['bar']:.1e}, model spread "
                  f"{fig['spread']:.1e}), dloss {fig['dloss']:.2e}, sums at {fig['sum_ratio']:.2e} of their bound, pose chain "
                  f"{max(fig['drot'], fig['dtrans']):.2e}" + (", guard" if fig["guard"] else ""))
    if failures:
        raise AuditFailure(failures)
    return models


# ----------------------------------------------------------------------------------------------------------------------
# the stand-in for the device in the CPU suite, and its deliberately wrong copies
# ----------------------------------------------------------------------------------------------------------------------
def _standin_rows(mv, mn, moved, index, higher_layer=False, unset_as_point=False):
    """k_pm_iterate's loop, layer by layer with a running best (another formulation than model_rows' argmin); `index`
    [H*W]: the winner of every pixel as a row of `moved`.  Returns (q, p, n, pixels)."""
    k = mv.shape[0]
    lv, ln = np.asarray(mv, F32).reshape(k, 3, -1), np.asarray(mn, F32).reshape(k, 3, -1)
    pix = np.flatnonzero(index >= 0)
    p = moved[index[pix]]
    best = np.full(len(pix), np.inf, F32)
    bk = np.full(len(pix), -1, np.int64)
    for layer in range(k):
        q = lv[layer][:, pix].T
        with np.errstate(all="ignore"):
            e = p - q
            d = np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]).astype(F32)
        usable = np.ones(len(pix), bool) if unset_as_point else np.abs(q).max(axis=1) > 0
        take = usable & ((d <= best) if higher_layer else (d < best))
        best, bk = np.where(take, d, best), np.where(take, layer, bk)
    safe = np.maximum(bk, 0)
    q, n = lv[safe, :, pix].reshape(-1, 3), ln[safe, :, pix].reshape(-1, 3)
    ok = (bk >= 0) & (np.abs(p).max(axis=1) > 0) & (np.abs(q).max(axis=1) > 0)
    return q[ok], p[ok], n[ok], pix[ok]


def _fused_loss_sums(out, rw, r):
    """Elements 27 and 28 as the iteration kernels form them (float64 products of the float32 w r and r), and the loss."""
    neq = out["neq"]
    neq[27], neq[28] = float((np.asarray(rw, F32).astype(F64) ** 2).sum()), float((np.asarray(r, F32).astype(F64) ** 2).sum())
    if out["status"] == ICP_OK and np.sqrt(neq[28]) < 1.0e-7:
        out["loss"] = float(neq[28])
    else:
        out["loss"] = float(neq[27])


def standin_records(mv, mn, targets, skip_null, init, K, scheme, sigma, threshold=0.0, wrong=None):
    """K iterations of pmap_register from the ORACLE's statements (alignment_audit.oracle_seam: O.point_to_plane_rows,
    O.ls_weights, matrix products for the sums, inv(H)), the z-buffer by projection_audit.model's scatter, the layers by
    _standin_rows: the records `truncated_runs` returns on the device.  `wrong`: one of WRONG."""
    assert wrong is None or wrong in WRONG, wrong
    mv = np.asarray(mv, F32)
    _, _, h, w = mv.shape
    t = np.asarray(targets, F32).reshape(-1, 3)
    src = valid_source_rows(t, skip_null and wrong != "skip_null_ignored")
    pose = np.asarray(init, F32).reshape(4, 4).copy()
    prev_pose, keys, records = pose, None, []
    blocks, supers = blocks_of(h, w)
    for k in range(1, K + 1):
        assoc_pose = prev_pose if wrong == "previous_pose" else pose
        moved = PC.transform_fma(t[src], assoc_pose)
        bit = PA.model(moved, h, w, PC.UP_FOV, PC.DOWN_FOV, wrong=wrong if wrong in ("farther_wins", "tie_lowest_index") else None,
                       keys=keys if wrong == "stale_zbuffer" else None)
        keys = bit.keys
        q, p, n, pix = _standin_rows(mv, mn, moved, bit.index.reshape(-1), higher_layer=wrong == "higher_layer",
                                     unset_as_point=wrong == "unset_not_skipped")
        if wrong == "last_block_dropped":
            keep = pix // PM_THREADS != blocks - 1
            q, p, n = q[keep], p[keep], n[keep]
        if wrong == "quarter_row_dropped":  # base row s + S of super-row s = 0
            keep = pix // PM_THREADS != min(supers, blocks - 1)
            q, p, n = q[keep], p[keep], n[keep]
        if wrong in ("float32_sums", "wrong_huber_branch"):
            rows = AA.seam_rows("point_to_plane", q, p, n, None, scheme, sigma)
            if wrong == "wrong_huber_branch":
                assert scheme == "huber"
                plain = AA.seam_rows("point_to_plane", q, p, n, None, "least_square", sigma)
                j = int(np.argmax(np.abs(rows["r"])))  # a row of the linear branch, weighed as a quadratic one
                assert abs(rows["r"][j]) >= F32(sigma)
                for key in rows:
                    rows[key] = rows[key].copy()
                    rows[key][j] = plain[key][j]
            out = AA.output_from_rows(rows, dtype=F32 if wrong == "float32_sums" else F64)
            if wrong != "float32_sums":
                _fused_loss_sums(out, rows["rw"], rows["r"])
        elif len(q):
            out = AA.oracle_seam("point_to_plane", q, p, n, None, scheme, sigma, with_residuals=False)
            _fused_loss_sums(out, IA.weighted_rows(p, q, n, scheme, sigma, "point_to_plane")[0], O.point_to_plane_rows(p, q, n)[0])
        else:
            out = AA.seam_output(ICP_OK, np.eye(4), np.zeros(6), 0.0, np.zeros(32))
        neq, dx = out["neq"], out["params"]
        guard = out["status"] != ICP_OK or np.sqrt(neq[28]) < 1.0e-7
        stop = guard or norm32(dx) < threshold
        nxt = pose if stop else chain_pose(dx, pose)
        if wrong == "pose_advanced_on_guard" and guard:
            nxt = chain_pose(np.array([1e-3, 0, 0, 0, 0, 1e-4], F32), pose)
        records.append(Record(k, pose[:3].copy(), neq.copy(), out["loss"], dx.copy(), int(neq[29]), out["status"], k,
                              bool(stop and out["status"] == ICP_OK), nxt.copy()))
        if stop:
            break
        prev_pose, pose = pose, nxt
    return records


# ----------------------------------------------------------------------------------------------------------------------
# windows and cases (shared by the CPU suite and the device tests)
# ----------------------------------------------------------------------------------------------------------------------
SHAPES = ((3, 3), (1, 300), (17, 33), (4, 256), (5, 256), (16, 2048), (128, 257), (64, 1024), (112, 2048), (112, 2049),
          (128, 2048), (128, 2049))
LARGE = SHAPES[-4:]  # K = 2, one scheme
SCHEME_SHAPES = ((17, 33), (64, 1024))
K_FULL, K_LARGE = 6, 2
_CACHE = {}


def iteration_inputs(h, w):
    """PC.iteration_case(h, w, "scan"), once per shape: (update calls, scan rows with the null rows, initial poses)."""
    if ("case", h, w) not in _CACHE:
        _CACHE[("case", h, w)] = PC.iteration_case(h, w, "scan")
    return _CACHE[("case", h, w)]


def window_calls(kind, h, w):
    """(update calls [(rel_pose, vmap or None, kernel size)], local_map_size) of a window family member."""
    calls, _, _ = iteration_inputs(h, w)
    if kind in ("lms4", "lms2", "lms1"):
        return [(p, v, 5) for p, v in calls], int(kind[3:])
    if kind == "ks3":
        return [(p, v, 3) for p, v in calls], 4
    if kind == "recycled":  # every slot recycled twice, sparse maps with holes into recycled slots: layers unset at pixels
        return [(p, v, 5) for p, v in PC.window_sequence(h, w, 2)], 2
    if kind == "twice":  # the same vertex map under the identity, its normals at kernel sizes 3 and 5: the layers tie
        v = calls[0][1]
        return [(np.eye(4, dtype=F32), v, 3), (np.eye(4, dtype=F32), v, 5)], 4
    raise AssertionError(kind)


def cpu_window(h, w, calls, lms):
    """(mv, mn) [K,3,H,W] of the window the update calls leave, on the CPU: PC.LibraryWindowOracle for the window and its
    poses, PC.emulate_model for the model layers."""
    ks_now = [5]
    orc = PC.LibraryWindowOracle(h, w, PC.UP_FOV, PC.DOWN_FOV, local_map_size=lms, normals_dtype=F64,
                                 nmap_of=lambda v: O.compute_normal_map(v, ks_now[0], F64))
    orc.build_model = lambda: None  # (the oracle's float32 re-projection is not what the iteration is held to)
    for pose, v, ks in calls:
        ks_now[0] = ks
        orc.update(pose, v)
    return PC.emulate_model(orc.vmaps, orc.nmaps, orc.poses, h, w)


def cached_cpu_window(kind, h, w):
    if ("window", kind, h, w) not in _CACHE:
        calls, lms = window_calls(kind, h, w)
        _CACHE[("window", kind, h, w)] = cpu_window(h, w, calls, lms)
    return _CACHE[("window", kind, h, w)]


def _scan(h, w):
    return np.ascontiguousarray(iteration_inputs(h, w)[1], F32)


def make_targets(kind, h, w, mv, init):
    """name -> target rows.  `mv`: the model of the window (the planted kinds search it)."""
    scan = _scan(h, w)
    valid = scan[np.abs(scan).max(axis=1) > 0]
    rng = np.random.default_rng(17)
    if kind == "scan":  # the scan's H*W rows with their null rows (the synthetic scene leaves few: every 41st row is made one)
        out = scan.copy()
        out[5::41] = 0.0
        return out
    if kind == "contested":  # 1.5 x H*W rows: the scan and a jittered copy of half of it
        half = scan[: len(scan) // 2]
        jit = (half + rng.normal(0.0, 0.02, half.shape).astype(F32)) * (np.abs(half).max(axis=1, keepdims=True) > 0)
        return np.ascontiguousarray(np.concatenate([scan, jit.astype(F32)]))
    if kind == "ties":  # pairs (a, a + e, z), (a + e, a, z): equal range bits, one pixel (azimuth 45 degrees: column 0.375 W),
        a = np.array([1.5, 2.0, 2.5, 3.0], F32)  # nearer than the scan there; under the identity pose
        z = (a * (np.sqrt(2.0) * np.tan(np.deg2rad([-5.0, -10.0, -15.0, -20.0])))).astype(F32)  # (four rows of the image)
        b = a + F32(1.0e-3)
        plus, minus = np.stack([a, b, z], 1), np.stack([b, a, z], 1)
        copies = valid[:16].copy()  # exact copies of rows at a higher index: the same sums either way
        return np.ascontiguousarray(np.concatenate([plus, valid, minus, copies]).astype(F32))
    if kind[0] == "n" and kind[1:].isdigit():  # n0, n1, n5, n6, n7
        n = int(kind[1:])
        step = max(1, len(valid) // max(n, 1))
        return np.ascontiguousarray(valid[::step][:n].reshape(-1, 3))
    if kind == "nan":
        out = scan.copy()
        out[::7, 1] = np.nan
        out[3::11] = np.nan
        return out
    if kind == "off_image":  # above and below the field of view
        up = valid[: max(8, len(valid) // 4)].copy()
        up[:, 2] = np.abs(up[:, :2]).max(axis=1) * F32(3.0) + F32(1.0)
        return np.ascontiguousarray(np.concatenate([up, up * np.array([1, 1, -1], F32)]))
    if kind == "planted":  # r == 0 rows, 0 < |r| < 1e-4 rows, a NaN and a null row, the scan
        return PC.iteration_targets(mv, init, scan, True)[0]
    if kind == "on_model":  # every target exactly on a model point: the residual guard
        exact, _, _ = PC.plant_targets(mv, init, count=64)
        assert len(exact) >= 6
        return exact
    if kind == "near_origin":  # a few targets nearer to the origin than to the model: an unset layer taken for a point wins
        out = valid.copy()
        out[::9] *= F32(0.01)
        return out
    raise AssertionError(kind)


@dataclass
class Case:
    name: str
    h: int
    w: int
    window: str = "lms4"
    targets: str = "scan"
    skip_null: bool = True
    init: int = 1  # index into the initial poses of iteration_case: 0 the identity
    scheme: str = "huber"
    K: int = K_FULL
    guard: bool = False  # built for a guard: an undetermined status is accepted, the spreads are not held to STEP_CAP
    family: str = "shapes"

    @property
    def sigma(self):
        return SCHEME_SIGMA[self.scheme]

    def init_pose(self):
        return iteration_inputs(self.h, self.w)[2][self.init]


def cases():
    out = []
    for h, w in SHAPES:
        out.append(Case(f"shape {h}x{w}", h, w, K=K_LARGE if (h, w) in LARGE else K_FULL, guard=(h, w) == (3, 3)))
    for h, w in SCHEME_SHAPES:
        for i, s in enumerate(PC.SCHEMES):
            if s != "huber":
                out.append(Case(f"scheme {s} {h}x{w}", h, w, scheme=s, skip_null=bool(i % 2), family="schemes"))
    for h, w in ((17, 33), (5, 256)):
        out.append(Case(f"all rows {h}x{w}", h, w, skip_null=False, family="targets"))
        out.append(Case(f"contested {h}x{w}", h, w, targets="contested", family="targets"))
        out.append(Case(f"ties {h}x{w}", h, w, targets="ties", init=0, family="targets"))
        out.append(Case(f"nan {h}x{w}", h, w, targets="nan", skip_null=False, family="targets"))
        out.append(Case(f"planted {h}x{w}", h, w, targets="planted", family="targets"))
        out.append(Case(f"identity {h}x{w}", h, w, init=0, family="targets"))
    for n in (0, 1, 5, 6, 7):
        out.append(Case(f"n={n} 17x33", 17, 33, targets=f"n{n}", guard=True, family="guards"))
    out.append(Case("off image 17x33", 17, 33, targets="off_image", guard=True, family="guards"))
    out.append(Case("on model 17x33", 17, 33, targets="on_model", guard=True, family="guards"))
    for kind in ("lms1", "lms2", "ks3", "recycled", "twice"):
        out.append(Case(f"window {kind} 17x33", 17, 33, window=kind, init=0 if kind == "twice" else 1, family="windows"))
    out.append(Case("window recycled near origin 17x33", 17, 33, window="recycled", targets="near_origin", family="windows"))
    out.append(Case("window recycled 5x256", 5, 256, window="recycled", family="windows"))
    return out


def case_by_name(name):
    return next(c for c in cases() if c.name == name)


def thresholds_between(records):
    """[(threshold, iteration it must stop at)]: halfway, geometrically, between consecutive float32 norms of the audited
    history — the decision is never marginal.  Only where the norms fall."""
    norms = [norm32(r.dx) for r in records]
    out = []
    for k in range(1, len(norms)):
        if norms[k] < norms[k - 1] and norms[k] > 0 and all(v > np.sqrt(norms[k] * norms[k - 1]) for v in norms[:k]):
            out.append((float(np.sqrt(norms[k] * norms[k - 1])), k + 1))
    return out


def census(models, sigma):
    """Which branches the model's rows of a run exercise (projective_cases.residual_census), summed over its iterations."""
    out = dict(quadratic=0, linear=0, clamped=0, zero=0)
    for m in models:
        if m["n"]:
            for key, v in PC.residual_census((m["q"], m["normals"], m["p"]), sigma).items():
                out[key] += v
    return out


# ----------------------------------------------------------------------------------------------------------------------
# runs on the device
# ----------------------------------------------------------------------------------------------------------------------
def device_context(case, max_num_alignments, threshold=0.0):
    """A context holding the case's window (the update calls made), the normal-equation buffer installed."""
    from pylidar_slam_amd.engine import IcpContext
    calls, lms = window_calls(case.window, case.h, case.w)
    ctx = IcpContext(height=case.h, width=case.w, local_map_size=lms, max_num_alignments=max_num_alignments,
                     threshold_delta_pose=threshold, scheme=case.scheme, sigma=case.sigma)
    ctx.pmap_init()
    for pose, v, ks in calls:
        ctx.pmap_update(pose, v, ks)
    ctx.normal_equations_tensor()
    return ctx


def per_call(ctx, targets, init, skip_null):
    return IA.registered(lambda: ctx.pmap_register(targets, init, skip_null=skip_null))


def launched(ctx, targets, init, skip_null):
    ctx.pmap_register_launch(targets, init, skip_null=skip_null)
    return IA.registered(ctx.register_end)


def truncated_runs(ctx, case, targets, init, register: Callable = per_call):
    """Runs of k = 1 .. K forced iterations on the case's context (threshold 0, max_num_alignments = k), the 30 sums read from
    its normal-equation buffer after each synchronous call.  Asserts the prefix property bit for bit; returns (records,
    (status, result) of run K).  The K runs share ONE context (`set_alignment` between them) rather than K contexts given the
    same update calls: what a registration leaves behind — target keys in the z-buffer, the state, the sums — is then in
    front of the next run, and the prefix property would show it."""
    K, skip_null = case.K, case.skip_null
    runs = []
    for k in range(1, K + 1):
        ctx.set_alignment(case.scheme, case.sigma, k, 0.0)
        rc, res = register(ctx, targets, init, skip_null)
        runs.append((rc, res, ctx.normal_equations_tensor().cpu().numpy().copy()))
    rcK, resK, _ = runs[-1]
    records = []
    for k, (rc, res, neq) in enumerate(runs, start=1):
        j = min(k, resK.iterations)
        assert res.iterations == j, (k, res.iterations, resK.iterations)
        assert np.array_equal(res.losses, resK.losses[:j]) and np.array_equal(res.dx, resK.dx[:j]), \
            f"a run of {k} iterations is no prefix of the run of {K}"
        if k <= resK.iterations:
            assert rc == ICP_OK or k == resK.iterations, (k, rc)
            pose_in = np.asarray(init, F32).reshape(4, 4) if k == 1 else runs[k - 2][1].pose
            records.append(Record(k, pose_in[:3].copy(), neq, float(res.losses[k - 1]), res.dx[k - 1].copy(), res.num_targets,
                                  rc, res.iterations, res.converged, res.pose.copy()))
        else:  # a guard ended the loop before k: the same result as run K
            assert rc == rcK and np.array_equal(res.pose, resK.pose) and res.converged == resK.converged, k
    return records, (rcK, resK)


def same_result(a, b, what):
    """(status, RegisterResult) pairs: bit for bit."""
    assert a[0] == b[0], f"{what}: status {a[0]} vs {b[0]}"
    ra, rb = a[1], b[1]
    assert ra.iterations == rb.iterations and ra.converged == rb.converged and ra.num_targets == rb.num_targets, \
        f"{what}: iterations {ra.iterations} / {rb.iterations}, converged {ra.converged} / {rb.converged}, rows " \
        f"{ra.num_targets} / {rb.num_targets}"
    for name in ("pose", "losses", "dx"):
        x, y = np.ascontiguousarray(getattr(ra, name)), np.ascontiguousarray(getattr(rb, name))
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), f"{what}: {name}"
