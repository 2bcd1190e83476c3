"""Audit of the three stand-alone alignment seams — icp_align_point_to_plane, icp_align_point_to_point and
icp_weighted_procrustes — (tests/test_alignment_audit.py on the CPU, tests/test_gpu_alignment_audit.py on the device).
TEST INFRASTRUCTURE: numpy + oracle/icp_oracle.py + tests/iteration_audit.py, importable without a GPU, never imported by
the package.

The seams hand back more than a registration does: the 30 float64 sums of the normal equations, the residual vector
(w r)^2 per row, params = x0 + dx.  The model restates the float32 rows exactly as the kernels form them (operation by
operation, no contraction), so that

  row count          neq[29] is exact;
  status             follows the rule of iteration_audit.check_rows (LU and Cholesky determinant on opposite sides of 1e-7:
                     either status); dx = 0 and params = x0 behind both guards;
  step               dx and loss at STEP_ATOL 2e-7 / rtol 2e-5 / loss 1e-5, the absolute bar widened to 4 x the spread of
                     the float64 solves — inv(H) g, the Cholesky solve, and the solve of the same rows added in the opposite
                     order — never from the kernel's output; a bar beyond STEP_CAP: the step is undetermined;
  normal equations   every sum within 2 n 2^-53 sum |a_i b_i| of the model's: the bound of ANY order of n float64
                     additions of exact products (Higham, Accuracy and Stability, eq. 4.4: (n - 1) u / (1 - (n - 1) u),
                     u = 2^-53, doubled for the two sides);
  residual vector    bit for bit for the schemes whose rows use IEEE + - * / sqrt alone.

`exp`, `neighborhood` and `cauchy` call expf / logf and a linearisation point x0 != 0 calls cosf / sinf, none of which
has a single answer: there the bars are 4 x the spread between two CPU evaluations of the model (the function in float32,
and in float64 rounded to float32), the margin the project uses for C_SOLVE (projective_cases.py).
"""
import numpy as np

import icp_oracle as O
import iteration_audit as A
from iteration_audit import F32, F64, ICP_ERR_INVALID_JACOBIAN, ICP_OK, STEP_ATOL, AuditFailure  # noqa: F401

COSTS = A.COSTS
SCHEMES = A.SCHEMES
IEEE_SCHEMES = ("default", "least_square", "huber", "geman_mcclure", "square_geman_mcclure")
U = 2.0 ** -53
POSE_ATOL = A.POSE_ATOL  # pose = build_pose_matrix(params): the device's cosf / sinf against numpy's
MARGIN = 4.0  # x a CPU-side spread (the margin of C_SOLVE)
# A step whose derived bar exceeds the project's pose bar (1e-4 m / 1e-4 rad, BASELINE.json) is UNDETERMINED by the reference
# (the rule of projective_cases.NORMAL_TOL_CAP): at pitch = pi / 2 two columns of J coincide to 1e-8 (gimbal lock), det H
# stays above 1e-7 by its sheer scale and the float64 solves of the same rows differ by 1e4 rad.  The CPU suite asserts
# that this happens in the pitch_half_pi cases alone.
STEP_CAP = 1.0e-4

# Largest relative difference of (w r)^2 between the two evaluations of the transcendental (float32 / float64 rounded),
# over every row of every case of the device tests, as test_alignment_audit.py::test_tolerance_constants re-measures it;
# TRANSCENDENTAL_BOUND = MARGIN x the spread is the per-row relative bar of these schemes, and — every term of the 28
# weighted sums carries two factors w, (w r)^2 carries the same two — the relative widening of their sums.
TRANSCENDENTAL_SPREAD = {"exp": 6.0e-7, "neighborhood": 6.0e-7, "cauchy": 6.0e-7}  # measured 5.61e-7, 5.70e-7, 5.51e-7
TRANSCENDENTAL_BOUND = {k: MARGIN * v for k, v in TRANSCENDENTAL_SPREAD.items()}


# ----------------------------------------------------------------------------------------------------------------------
# rows
# ----------------------------------------------------------------------------------------------------------------------
def _fn(name, x, mode):
    """expf / logf of a float32 array: in float32, or in float64 rounded to float32."""
    f = getattr(np, name)
    with np.errstate(all="ignore"):
        return f(x.astype(F32)) if mode == "f32" else f(x.astype(F64)).astype(F32)


def robust_weights(scheme, sigma, res, d2, transcendental="f32", clamp=True):
    """robust_weight of csrc/gn_device.h = O.ls_weights (optimization.py:45-50) on the residuals `res` and — `neighborhood`
    — the squared distance `d2` of the pair it weighs by; every operation rounded to float32.  `clamp` False: the wrong
    copy without the 1e-4 clamp."""
    res = np.asarray(res, F32)
    if scheme in ("default", "least_square"):
        return np.ones(res.shape, F32)
    s = F32(sigma)
    a = np.abs(res)
    r2 = res * res
    with np.errstate(all="ignore"):
        if scheme == "huber":
            cost = np.where(a < s, r2, F32(2) * s * a - s * s)
        elif scheme == "exp":
            cost = r2 * _fn("exp", -r2 / (s * s), transcendental)
        elif scheme == "neighborhood":
            nrm = np.sqrt(np.asarray(d2, F32))
            cost = r2 * _fn("exp", -(nrm * nrm) / (s * s), transcendental)
        elif scheme == "geman_mcclure":
            cost = s * r2 / (s + r2)
        elif scheme == "square_geman_mcclure":
            q = s / (s + r2)
            cost = r2 * (q * q)
        elif scheme == "cauchy":
            q = res / s
            cost = _fn("log", F32(1) + q * q, transcendental)
        else:
            raise AssertionError(scheme)
        den = np.maximum(a, F32(1.0e-4)) if clamp else a
        return (np.sqrt(cost.astype(F32)) / den).astype(F32)


def _mat3(a, b):
    """mat3_mul of gauss_newton.hip: s = ((0 + a0 b0) + a1 b1) + a2 b2 in float32, no contraction."""
    c = np.zeros((3, 3), F32)
    for i in range(3):
        for j in range(3):
            s = F32(0)
            for k in range(3):
                s = F32(s + F32(a[i, k] * b[k, j]))
            c[i, j] = s
    return c


def linearisation(x0, trig="f32"):
    """(R0 [3,3], dR [3,3,3]) of linearise_euler: O.euler_to_mat / O.euler_jacobian (rotation.py:144-187) with the products
    spelt out.  `trig`: cos / sin in float32 | in float64 rounded to float32 | "oracle": the oracle's own matrices (numpy
    matmul, whose float32 kernels may fuse a multiply-add)."""
    e = np.asarray(x0, F32)[3:]
    if trig == "oracle":
        return O.euler_to_mat(e), O.euler_jacobian(e)
    c, s = (np.cos(e), np.sin(e)) if trig == "f32" else (np.cos(e.astype(F64)).astype(F32), np.sin(e.astype(F64)).astype(F32))
    z, o = F32(0), F32(1)
    rx = np.array([[o, z, z], [z, c[0], -s[0]], [z, s[0], c[0]]], F32)
    ry = np.array([[c[1], z, s[1]], [z, o, z], [-s[1], z, c[1]]], F32)
    rz = np.array([[c[2], -s[2], z], [s[2], c[2], z], [z, z, o]], F32)
    jx = np.array([[z, z, z], [z, -s[0], -c[0]], [z, c[0], -s[0]]], F32)
    jy = np.array([[-s[1], z, c[1]], [z, z, z], [-c[1], z, -s[1]]], F32)
    jz = np.array([[-s[2], -c[2], z], [c[2], -s[2], z], [z, z, z]], F32)
    zy = _mat3(rz, ry)
    return _mat3(zy, rx), np.stack([_mat3(zy, jx), _mat3(_mat3(rz, jy), rx), _mat3(_mat3(jz, ry), rx)])


def _dot3(m, p):
    """(m0 px + m1 py) + m2 pz per row, float32."""
    return (m[0] * p[:, 0] + m[1] * p[:, 1]) + m[2] * p[:, 2]


def seam_rows(cost, ref, tgt, normals, x0, scheme, sigma, trig="f32", transcendental="f32", clamp=True,
              neighborhood_on="raw", use_x0=True):
    """The float32 rows of k_reduce_given / k_reduce_p2p: dict(jw [n,6] weighted Jacobian, rw [n] weighted residual,
    r [n] raw residual, rw2 [n] = (w r)^2, r2 [n] = r r), all float32.  For point-to-plane and for point-to-point at x0 = 0
    these are iteration_audit.weighted_rows (asserted by the CPU suite); for x0 != 0 O.point_to_point_step's rows with the
    sums spelt out.  `neighborhood` weighs by the RAW target (alignment.py:183).  `clamp`, `neighborhood_on="moved"` and
    `use_x0=False` build wrong copies."""
    q, p = np.asarray(ref, F32).reshape(-1, 3), np.asarray(tgt, F32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        e = p - q
        d2raw = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
        if cost == "point_to_plane":
            n = np.asarray(normals, F32).reshape(-1, 3)
            r = (e[:, 0] * n[:, 0] + e[:, 1] * n[:, 1]) + e[:, 2] * n[:, 2]
            jac = np.stack([n[:, 0], n[:, 1], n[:, 2], p[:, 1] * n[:, 2] - p[:, 2] * n[:, 1],
                            p[:, 2] * n[:, 0] - p[:, 0] * n[:, 2], p[:, 0] * n[:, 1] - p[:, 1] * n[:, 0]], axis=1)
            d2 = d2raw
        else:
            x = np.zeros(6, F32) if (x0 is None or not use_x0) else np.asarray(x0, F32).reshape(6)
            r0, dr = linearisation(x, trig)
            d = np.stack([(_dot3(r0[a], p) + x[a]) - q[:, a] for a in range(3)], axis=1)
            r = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
            cols = [d[:, 0], d[:, 1], d[:, 2]]
            for k in range(3):
                s = np.zeros(len(p), F32)
                for a in range(3):
                    s = s + _dot3(dr[k, a], p) * d[:, a]
                cols.append(s)
            jac = np.stack(cols, axis=1)
            d2 = d2raw if neighborhood_on == "raw" else (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        w = robust_weights(scheme, sigma, r, d2, transcendental, clamp)
        rw = (r * w).astype(F32)
        jw = (jac * w.reshape(-1, 1)).astype(F32)
        return dict(jw=jw, rw=rw, r=r.astype(F32), rw2=(rw * rw).astype(F32), r2=(r * r).astype(F32))


TRI = [(a, b) for a in range(6) for b in range(a, 6)]


def row_sums(rows, dtype=F64):
    """(sums [30], absolute sums [30]) of the rows as RowAcc::add_row accumulates them: 21 upper-triangle elements of H
    (exact float64 products of float32 factors), 6 of g, sum (w r)^2 and sum r^2 of the float32 squares, the row count.
    `dtype` float32: the wrong copy that sums in float32."""
    jw, rw = rows["jw"].astype(dtype), rows["rw"].astype(dtype)
    terms = [jw[:, a] * jw[:, b] for a, b in TRI] + [jw[:, a] * rw for a in range(6)] + \
            [rows["rw2"].astype(dtype), rows["r2"].astype(dtype), np.ones(len(rw), dtype)]
    with np.errstate(all="ignore"):
        if dtype == F32:  # (a running float32 sum, as a float32 accumulator would hold it)
            return np.array([np.cumsum(t, dtype=F32)[-1] if len(t) else 0.0 for t in terms], F64), None
        return np.array([t.sum() for t in terms], F64), np.array([np.abs(t).sum() for t in terms], F64)


def solve_sums(sums):
    """iteration_audit.reference_step from the 30 sums (the same statements; the CPU suite asserts the same results)."""
    count = int(sums[29])
    out = dict(status=ICP_OK, stopped=False, dx=np.zeros(6, F32), loss=0.0, count=count, spread=0.0, det=(0.0, 0.0))
    if count == 0:
        out.update(stopped=True)
        return out
    if np.sqrt(sums[28]) < 1.0e-7:
        out.update(stopped=True, loss=float(sums[28]))
        return out
    H = np.zeros((6, 6))
    for k, (a, b) in enumerate(TRI):
        H[a, b] = H[b, a] = sums[k]
    g = sums[21:27].copy()
    out["loss"] = float(sums[27])
    if not np.isfinite(H).all():  # a NaN row: every sum is NaN; the library reports an Invalid Jacobian (its documented
        out.update(status=ICP_ERR_INVALID_JACOBIAN, det=(np.nan, np.nan))  # deviation: `abs(det) < 1e-7` is False for NaN)
        return out
    det_lu = float(np.linalg.det(H))
    try:
        L = np.linalg.cholesky(H)
        det_ch = float(np.prod(np.diag(L) ** 2))
    except np.linalg.LinAlgError:
        L, det_ch = None, 0.0
    out["det"] = (det_lu, det_ch)
    if abs(det_lu) < 1.0e-7:
        out["status"] = ICP_ERR_INVALID_JACOBIAN
    try:
        dx_inv = -(np.linalg.inv(H) @ g)
        other = np.linalg.solve(L.T, np.linalg.solve(L, g)) if L is not None else np.linalg.solve(H, g)
    except np.linalg.LinAlgError:
        return out
    out["dx"] = dx_inv.astype(F32)
    out["spread"] = float(np.abs(dx_inv + other).max())
    return out


def seam_step(cost, ref, tgt, normals, x0, scheme, sigma):
    """The model of one seam call: the rows, their 30 float64 sums, the float64 step two ways, params = float32(x0 + dx),
    pose = O.build_pose_matrix(params), and the bars every check uses:
      sum_tol [30]   2 n 2^-53 sum |a_i b_i| per element, + TRANSCENDENTAL_BOUND x sum |a_i b_i| for exp / neighborhood /
                     cauchy (elements 0 .. 27: the weighted ones), + MARGIN x the spread of the sums over the evaluations
                     of cos / sin at x0 != 0;
      row_tol        None: the residual vector bit for bit; else the bar per row, TRANSCENDENTAL_BOUND x |(w r)^2| and
                     MARGIN x the largest difference of a row over the evaluations of cos / sin;
      dx_spread      the largest difference of dx over those evaluations (0 where they agree to the bit)."""
    n = int(np.asarray(ref).reshape(-1, 3).shape[0])
    x = np.zeros(6, F32) if x0 is None else np.asarray(x0, F32).reshape(6)
    rows = seam_rows(cost, ref, tgt, normals, x, scheme, sigma)
    sums, asum = row_sums(rows)
    ref_step = solve_sums(sums)
    sum_tol = 2.0 * n * U * asum
    row_tol, dx_spread, trig_exact = None, 0.0, True
    if scheme not in IEEE_SCHEMES:
        sum_tol[:28] += TRANSCENDENTAL_BOUND[scheme] * asum[:28]
        row_tol = TRANSCENDENTAL_BOUND[scheme] * np.abs(rows["rw2"].astype(F64))
    if cost == "point_to_point" and np.any(x[3:] != 0):
        base = linearisation(x, "f32")
        for trig in ("f64", "oracle"):
            other = linearisation(x, trig)
            if all(np.array_equal(u, v) for u, v in zip(base, other)):
                continue
            trig_exact = False
            alt = seam_rows(cost, ref, tgt, normals, x, scheme, sigma, trig=trig)
            alt_sums, _ = row_sums(alt)
            with np.errstate(all="ignore"):
                sum_tol = sum_tol + MARGIN * np.abs(alt_sums - sums)
                worst_row = float(np.nanmax(np.abs(alt["rw2"].astype(F64) - rows["rw2"].astype(F64)))) if n else 0.0
            row_tol = (0.0 if row_tol is None else row_tol) + np.full(n, MARGIN * worst_row)
            dx_spread = max(dx_spread, float(np.abs(solve_sums(alt_sums)["dx"].astype(F64) - ref_step["dx"].astype(F64)).max()))
    moved = ref_step["status"] == ICP_OK and not ref_step["stopped"]
    params = (x + ref_step["dx"]).astype(F32) if moved else x.copy()
    # a third float64 solve: the same rows added in the opposite order (the spread of inv(H) g against the Cholesky solve of
    # the SAME sums says nothing about what the order of 10^5 additions does to an ill-conditioned solve)
    order_spread = float(np.abs(solve_sums(row_sums(take_rows(rows, slice(None, None, -1)))[0])["dx"].astype(F64)
                                - ref_step["dx"].astype(F64)).max()) if n else 0.0
    ref_step["order_spread"] = order_spread
    return dict(cost=cost, scheme=scheme, n=n, x0=x, rows=rows, sums=sums, asum=asum, ref=ref_step, sum_tol=sum_tol,
                row_tol=row_tol, dx_spread=dx_spread, trig_exact=trig_exact, params=params,
                pose=O.build_pose_matrix(params))


# ----------------------------------------------------------------------------------------------------------------------
# what a seam call returned, and the check
# ----------------------------------------------------------------------------------------------------------------------
def seam_output(status, pose, params, loss, neq, residuals=None):
    return dict(status=int(status), pose=np.asarray(pose, F32).reshape(4, 4), params=np.asarray(params, F32).reshape(6),
                loss=float(loss), neq=np.asarray(neq, F64).reshape(-1),
                residuals=None if residuals is None else np.asarray(residuals, F32).reshape(-1))


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, F32).view(np.uint32), np.asarray(b, F32).view(np.uint32))


def check_seam(out, model):
    """Returns (failures [(kind, why)], figures).  Kinds: "row count", "status", "step", "params", "pose",
    "normal equations", "residual vector".  A wrong row count ends the check: nothing else is comparable."""
    fails, ref, n = [], model["ref"], model["n"]
    fig = dict(rows=n, ddx=0.0, dloss=0.0, sum_ratio=0.0, bit_rows=0, tol_rows=0, row_ratio=0.0, spread=ref["spread"],
               atol=STEP_ATOL, widened=False, det=ref["det"], status_undetermined=False, step_undetermined=False)
    neq = out["neq"]
    if not (neq[29] == n):
        return [("row count", f"{neq[29]} rows summed, {n} given")], fig
    x0 = model["x0"]
    dx = (out["params"].astype(F64) - x0.astype(F64))
    invalid_out = out["status"] == ICP_ERR_INVALID_JACOBIAN
    undetermined = (abs(ref["det"][0]) < 1.0e-7) != (abs(ref["det"][1]) < 1.0e-7) and not ref["stopped"]
    fig["status_undetermined"] = bool(undetermined)
    invalid = invalid_out if undetermined else ref["status"] == ICP_ERR_INVALID_JACOBIAN
    if invalid != invalid_out or out["status"] not in (ICP_OK, ICP_ERR_INVALID_JACOBIAN):
        fails.append(("status", f"status {out['status']}, the model's {ref['status']} (det {ref['det'][0]:.3e} by LU, "
                                f"{ref['det'][1]:.3e} by Cholesky)"))
    elif invalid or ref["stopped"]:
        what = "Invalid Jacobian" if invalid else "residual guard"
        if not _same_bits(out["params"], x0):
            fails.append(("params", f"{what}: params {out['params']} are not x0 {x0}"))
        want = ref["loss"] if invalid else float(model["sums"][28])
        if np.isnan(want) != np.isnan(out["loss"]) or (not np.isnan(want) and abs(out["loss"] - want) > 1e-5 * abs(want) + 1e-300):
            fails.append(("step", f"{what}: loss {out['loss']} vs {want}"))
        if not (out["loss"] == (neq[27] if invalid else neq[28]) or (np.isnan(out["loss"]) and np.isnan(neq[27]))):
            fails.append(("step", f"{what}: the loss {out['loss']} is not the sum the call returned"))
    else:
        step = ref["dx"].astype(F64)
        # params = float32(x0 + dx): dx read back from params carries half an ulp of params
        back = 0.5 * np.spacing(np.maximum(np.abs(out["params"]), np.abs(x0)).astype(F32)).astype(F64) * (x0 != 0)
        atol = max(STEP_ATOL, MARGIN * ref["spread"], MARGIN * ref["order_spread"], MARGIN * model["dx_spread"])
        fig["step_undetermined"] = bool(atol > STEP_CAP)
        if atol > STEP_CAP:  # the reference's own float64 solves are further apart than the project's pose bar: no step to
            atol = np.inf  # hold the call to (the sums, the residual vector and the loss still are)
        fig.update(ddx=float(np.abs(dx - step).max()), atol=atol, widened=atol > STEP_ATOL,
                   dloss=abs(out["loss"] - ref["loss"]) / abs(ref["loss"]) if ref["loss"] else abs(out["loss"]))
        bar = atol + 2e-5 * np.abs(step) + back
        if not np.isfinite(out["params"]).all():
            fails.append(("step", f"params {out['params']}"))
        elif (np.abs(dx - step) > bar).any():
            bare = bool(np.any(x0 != 0) and (np.abs(out["params"].astype(F64) - step) <= bar).all())  # params = dx alone
            fails.append(("params" if bare else "step",
                          f"|ddx| {fig['ddx']:.2e} (atol {atol:.1e}): params {out['params']}, the model's "
                          f"{model['params']}" + (" — dx without x0" if bare else "")))
        if not abs(out["loss"] - ref["loss"]) <= 1e-5 * abs(ref["loss"]):
            fails.append(("step", f"loss {out['loss']} vs {ref['loss']}"))
        if out["loss"] != neq[27]:
            fails.append(("step", f"the loss {out['loss']} is not the sum (w r)^2 the call returned, {neq[27]}"))
    # pose = build_pose_matrix(params) of the call's own params
    want_pose = O.build_pose_matrix(out["params"])
    if not (np.array_equal(out["pose"][:3, 3], out["params"][:3]) and np.array_equal(out["pose"][3], [0, 0, 0, 1])
            and np.abs(out["pose"][:3, :3].astype(F64) - want_pose[:3, :3]).max() <= POSE_ATOL):
        fails.append(("pose", f"the pose is not build_pose_matrix(params): {out['pose']} vs {want_pose}"))
    # the 29 float sums
    with np.errstate(all="ignore"):
        diff = np.abs(neq[:29] - model["sums"][:29])
        tol = model["sum_tol"][:29]
        both_nan = np.isnan(neq[:29]) & np.isnan(model["sums"][:29])
        bad = ~both_nan & ~(diff <= tol)
        ratio = np.where(both_nan | (diff == 0), 0.0, diff / np.where(tol > 0, tol, np.inf))
        ratio = np.where(~both_nan & (diff > 0) & (tol == 0), np.inf, ratio)
    fig["sum_ratio"] = float(np.nanmax(ratio)) if len(ratio) else 0.0
    if bad.any():
        e = int(np.argmax(bad))
        fails.append(("normal equations", f"{bad.sum()} of 29 sums beyond their bound, first element {e}: {neq[e]!r} vs "
                                          f"{model['sums'][e]!r} (bound {tol[e]:.3e})"))
    # the residual vector
    if out["residuals"] is not None:
        got, want = out["residuals"], model["rows"]["rw2"]
        if got.shape != want.shape:
            fails.append(("residual vector", f"shape {got.shape}, {want.shape} rows"))
        elif model["row_tol"] is None:
            same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
            fig["bit_rows"] = int(len(want))
            if not same.all():
                i = int(np.argmin(same))
                fails.append(("residual vector", f"{(~same).sum()} of {len(want)} rows differ in their bits, first row {i}: "
                                                 f"{got[i]!r} vs {want[i]!r}"))
        else:
            with np.errstate(all="ignore"):
                d = np.abs(got.astype(F64) - want.astype(F64))
                nan_ok = np.isnan(got) == np.isnan(want)
                bad = ~nan_ok | (~np.isnan(want) & ~(d <= model["row_tol"]))
                r = np.where((d > 0) & ~np.isnan(d), d / np.where(model["row_tol"] > 0, model["row_tol"], np.inf), 0.0)
            fig.update(tol_rows=int(len(want)), row_ratio=float(r.max()) if len(r) else 0.0)
            if bad.any():
                i = int(np.argmax(bad))
                fails.append(("residual vector", f"{bad.sum()} of {len(want)} rows beyond their bar, first row {i}: "
                                                 f"{got[i]!r} vs {want[i]!r} (bar {model['row_tol'][i]:.3e})"))
    return fails, fig


def assert_seam(out, model, label=""):
    fails, fig = check_seam(out, model)
    if fails:
        raise AuditFailure([(k, f"{label}: {w}") for k, w in fails])
    return fig


class SeamWorst:
    """The worst figures of a family of seam calls, printed by the tests and quoted in their docstrings."""

    def __init__(self, name):
        self.name, self.n = name, 0
        self.f = dict(ddx=0.0, dloss=0.0, sum_ratio=0.0, row_ratio=0.0, bit_rows=0, tol_rows=0)
        self.widened, self.undetermined = [], []

    def add(self, fig, label=""):
        self.n += 1
        for k in ("ddx", "dloss", "sum_ratio", "row_ratio"):
            if np.isfinite(fig[k]):
                self.f[k] = max(self.f[k], fig[k])
        self.f["bit_rows"] += fig["bit_rows"]
        self.f["tol_rows"] += fig["tol_rows"]
        if fig["widened"]:
            self.widened.append((label, fig["atol"]))
        if fig["status_undetermined"]:
            self.undetermined.append(label)
        if fig["step_undetermined"]:
            self.undetermined.append(label + " (step)")

    def __str__(self):
        f = self.f
        s = (f"{self.name}: {self.n} calls checked; worst |ddx| {f['ddx']:.2e}, dloss {f['dloss']:.2e}, worst sum at "
             f"{f['sum_ratio']:.2e} of its bound, {f['bit_rows']} residual rows bit-compared, {f['tol_rows']} held to a bar "
             f"(worst at {f['row_ratio']:.2e} of it)")
        for label, atol in self.widened[:6]:
            s += f"\n  widened {label}: dx atol {atol:.2e}"
        for label in self.undetermined:
            s += f"\n  status undetermined by the model, the call's accepted: {label}"
        return s


def oracle_seam(cost, ref, tgt, normals, x0, scheme, sigma, with_residuals=True):
    """The stand-in for the device in the CPU suite: the seam call from the ORACLE's statements — O.point_to_plane_rows /
    the row expressions of O.point_to_point_step, O.ls_weights, matrix products for the sums (another order of addition
    than row_sums), inv(H) for the step."""
    q, p = np.asarray(ref, F32).reshape(-1, 3), np.asarray(tgt, F32).reshape(-1, 3)
    x = np.zeros(6, F32) if x0 is None else np.asarray(x0, F32).reshape(6)
    with np.errstate(all="ignore"):
        if cost == "point_to_plane":
            res, jac = O.point_to_plane_rows(p, q, np.asarray(normals, F32).reshape(-1, 3))
        else:
            r0, dr = linearisation(x, "f32")
            d = np.stack([(_dot3(r0[a], p) + x[a]) - q[:, a] for a in range(3)], axis=1).astype(F32)
            res = np.sqrt((d * d).sum(axis=-1, dtype=F32))
            rot = [np.stack([_dot3(dr[k, a], p) for a in range(3)], axis=1) for k in range(3)]
            jac = np.concatenate([d, np.stack([(rot[k] * d).sum(axis=-1, dtype=F32) for k in range(3)], 1)], axis=1).astype(F32)
        w = O.ls_weights(scheme, sigma, res, p, q)
        rw = (res * w).astype(F32)
        jw = (jac * w.reshape(-1, 1)).astype(F32)
        ja, ra = jw.astype(F64), rw.astype(F64)
        H, g = ja.T @ ja, ja.T @ ra
        neq = np.zeros(32)
        neq[:21] = [H[a, b] for a, b in TRI]
        neq[21:27] = g
        neq[27] = (rw * rw).astype(F32).astype(F64).sum()
        neq[28] = (res * res).astype(F32).astype(F64).sum()
        neq[29] = len(p)
        status, dx, loss = ICP_OK, np.zeros(6, F32), neq[27]
        if np.sqrt(neq[28]) < 1.0e-7:
            loss = neq[28]
        elif not (abs(np.linalg.det(H)) >= 1.0e-7):
            status = ICP_ERR_INVALID_JACOBIAN
        else:
            dx = (-(np.linalg.inv(H) @ g)).astype(F32)
    params = (x + dx).astype(F32)
    return seam_output(status, O.build_pose_matrix(params), params, loss, neq, (rw * rw).astype(F32) if with_residuals else None)


def output_from_rows(rows, x0=None, dtype=F64, add_x0=True, count=None, residuals=None):
    """A seam output computed from `rows` (the CPU suite builds its wrong copies with it): the sums in `dtype`, the step of
    solve_sums, params = x0 + dx (`add_x0` False: dx alone), the residual vector of the rows (or `residuals`); `count`
    overrides the row count."""
    x = np.zeros(6, F32) if x0 is None else np.asarray(x0, F32).reshape(6)
    sums, _ = row_sums(rows, dtype)
    if count is not None:
        sums[29] = count
    st = solve_sums(sums)
    neq = np.zeros(32)
    neq[:30] = sums
    params = (x + st["dx"]).astype(F32) if add_x0 else st["dx"].copy()
    return seam_output(st["status"], O.build_pose_matrix(params), params, st["loss"], neq,
                       rows["rw2"].copy() if residuals is None else residuals)


def take_rows(rows, keep):
    return {k: v[keep] for k, v in rows.items()}


# ----------------------------------------------------------------------------------------------------------------------
# Procrustes
# ----------------------------------------------------------------------------------------------------------------------
DETERMINED_GAP = 1.0e-6  # s[1] - s[2] > DETERMINED_GAP s[0]: the rotation is a function of the cross-covariance


def _horn(C):
    """Horn 1987: the rotation maximising tr(R^T C) is the unit quaternion of the largest eigenvalue of the symmetric 4x4
    matrix of the cross-covariance's elements (M = C^T in Horn's notation: target -> reference)."""
    S = C.T
    n = np.array([[S[0, 0] + S[1, 1] + S[2, 2], S[1, 2] - S[2, 1], S[2, 0] - S[0, 2], S[0, 1] - S[1, 0]],
                  [S[1, 2] - S[2, 1], S[0, 0] - S[1, 1] - S[2, 2], S[0, 1] + S[1, 0], S[2, 0] + S[0, 2]],
                  [S[2, 0] - S[0, 2], S[0, 1] + S[1, 0], -S[0, 0] + S[1, 1] - S[2, 2], S[1, 2] + S[2, 1]],
                  [S[0, 1] - S[1, 0], S[2, 0] + S[0, 2], S[1, 2] + S[2, 1], -S[0, 0] - S[1, 1] + S[2, 2]]])
    _, v = np.linalg.eigh(n)
    w, x, y, z = v[:, -1]
    return np.array([[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (y * x + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
                     [2 * (z * x - w * y), 2 * (z * y + w * x), w * w - x * x - y * y + z * z]])


def procrustes_model(tgt, ref, weights=None, reflection_fix=True, weighted_cov=False, mean_dtype=F32):
    """O.weighted_procrustes (registration.py:15-74) as the kernels form it: the weighted means accumulated in float64 and
    rounded to float32, the centred differences in float32, their cross-covariance in float64 WITHOUT the weights.  Also the
    singular values, Horn's quaternion solution of the same cross-covariance and the bars of check_procrustes.
    `reflection_fix`, `weighted_cov`, `mean_dtype` build wrong copies."""
    t, r = np.asarray(tgt, F32).reshape(-1, 3), np.asarray(ref, F32).reshape(-1, 3)
    n = len(t)
    w = np.ones(n, F64) if weights is None else np.asarray(weights, F32).reshape(-1).astype(F64)
    sw = w.sum()
    if not sw != 0.0:
        return dict(refused=True, n=n)
    mu_t = ((w[:, None] * t.astype(F64)).sum(axis=0) / sw).astype(mean_dtype)
    mu_r = ((w[:, None] * r.astype(F64)).sum(axis=0) / sw).astype(mean_dtype)
    dt = (t - mu_t.astype(F32)).astype(F32).astype(F64) if mean_dtype == F32 else t.astype(F64) - mu_t
    dr = (r - mu_r.astype(F32)).astype(F32).astype(F64) if mean_dtype == F32 else r.astype(F64) - mu_r
    C = (dr * w[:, None]).T @ dt if weighted_cov else dr.T @ dt
    c_bound = 2.0 * n * U * (np.abs(dr).T @ np.abs(dt))  # any order of n float64 additions of exact products
    Um, s, Vt = np.linalg.svd(C)
    S = np.eye(3)
    d = 1.0
    if np.linalg.det(Um) * np.linalg.det(Vt) < 0:
        d = -1.0
        if reflection_fix:
            S[2, 2] = -1.0
    R = Um @ S @ Vt
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = mu_r.astype(F64) - R @ mu_t.astype(F64)
    determined = bool(s[1] - s[2] > DETERMINED_GAP * s[0]) and s[0] > 0
    R2 = _horn(C)
    spread = float(np.abs(R - R2).max()) if determined else np.inf
    # |dR| <= 2 |dC|_F / (s1 + d s2) for a perturbation dC of the cross-covariance (the polar factor's first-order bound,
    # Higham, Functions of Matrices, thm 8.9 applied to the 3x3 problem with the sign d of the reflection fix), + 64 ulp for
    # the float64 products U S V^T of either side
    gap = s[1] + d * s[2]
    rot_tol = MARGIN * spread + (2.0 * np.linalg.norm(c_bound) / gap if determined and gap > 0 else np.inf) + 64 * 2.0 ** -52
    ulp_t, ulp_r = np.spacing(np.abs(mu_t.astype(F32))).astype(F64), np.spacing(np.abs(mu_r.astype(F32))).astype(F64)
    cost0 = float((dt * dt).sum() + (dr * dr).sum())
    err = float((((dt @ R.T) - dr) ** 2).sum())
    return dict(refused=False, n=n, pose=T, R=R, R2=R2, s=s, d=d, C=C, c_bound=c_bound, determined=determined, spread=spread,
                rot_tol=rot_tol, mu_t=mu_t, mu_r=mu_r, ulp_t=ulp_t, ulp_r=ulp_r, dt=dt, dr=dr, err=err,
                # tr(R^T C) of the call's rotation is the optimum of ITS cross-covariance, within c_bound of this one:
                err_slack=4.0 * float(c_bound.sum()) + 64 * 2.0 ** -52 * cost0)


def oracle_procrustes(model):
    """The stand-in for the device in the CPU suite: the model's SECOND formulation (Horn's quaternion) where the rotation
    is determined, the SVD's elsewhere; t = mu_ref - R mu_tgt.  (O.weighted_procrustes itself accumulates its means in
    float32: |d mu| up to n 2^-24 |mu|, far outside one ulp — test_alignment_audit.py holds the model to the reference's
    recorded results at the bars of the existing tests instead.)"""
    T = np.eye(4)
    T[:3, :3] = model["R2"] if model["determined"] else model["R"]
    T[:3, 3] = model["mu_r"].astype(F64) - T[:3, :3] @ model["mu_t"].astype(F64)
    return T


def check_procrustes(pose, model):
    """Returns (failures [(kind, why)], figures).  Kinds: "rotation" (orthonormal, det 1), "centroid"
    (R mu_tgt + t = mu_ref), "pose" (the determined rotation and translation), "optimum" (the alignment error)."""
    T = np.asarray(pose, F64).reshape(4, 4)
    R, t = T[:3, :3], T[:3, 3]
    fails = []
    fig = dict(determined=model["determined"], drot=0.0, dtrans=0.0, rot_tol=model["rot_tol"], spread=model["spread"])
    if not np.array_equal(T[3], [0, 0, 0, 1]):
        fails.append(("rotation", f"last row {T[3]}"))
    orth = float(np.abs(R @ R.T - np.eye(3)).max())
    det = float(np.linalg.det(R))
    if not (orth <= 1e-12 and abs(det - 1.0) <= 1e-12):
        fails.append(("rotation", f"|R R^T - I| {orth:.2e}, det {det:.15f}"))
        return fails, fig
    mu_t, mu_r = model["mu_t"].astype(F64), model["mu_r"].astype(F64)
    # one float32 ulp of either mean (the float64-accumulated mean may round to the neighbouring float32), the target's
    # carried through R, + the float64 rounding of the three products
    cen_tol = model["ulp_r"] + np.abs(R) @ model["ulp_t"] + 8 * 2.0 ** -52 * (np.abs(mu_r) + np.abs(R) @ np.abs(mu_t))
    cen = np.abs(R @ mu_t + t - mu_r)
    if (cen > cen_tol).any():
        fails.append(("centroid", f"R mu_tgt + t - mu_ref = {cen} (bar {cen_tol})"))
    if model["determined"]:
        fig["drot"] = float(np.abs(R - model["R"]).max())
        fig["dtrans"] = float(np.abs(t - model["pose"][:3, 3]).max())
        trans_tol = cen_tol + model["rot_tol"] * np.abs(mu_t).sum()
        if fig["drot"] > model["rot_tol"] or (np.abs(t - model["pose"][:3, 3]) > trans_tol).any():
            fails.append(("pose", f"rotation off by {fig['drot']:.2e} (bar {model['rot_tol']:.2e}: spread "
                                  f"{model['spread']:.2e}), translation by {fig['dtrans']:.2e} (bar {trans_tol})"))
    err = float((((model["dt"] @ R.T) - model["dr"]) ** 2).sum())
    fig["excess"] = err - model["err"]
    if not err <= model["err"] + model["err_slack"]:
        fails.append(("optimum", f"alignment error {err!r} above the model's optimum {model['err']!r} "
                                 f"(slack {model['err_slack']:.3e})"))
    return fails, fig


def assert_procrustes(pose, model, label=""):
    fails, fig = check_procrustes(pose, model)
    if fails:
        raise AuditFailure([(k, f"{label}: {w}") for k, w in fails])
    return fig


# ----------------------------------------------------------------------------------------------------------------------
# case inputs (shared by the CPU suite and the device tests)
# ----------------------------------------------------------------------------------------------------------------------
STRIDE = 65_536  # reduce_grid: 256 workgroups of 256 threads — rows from here on take the stride's second turn
GUARD_SIZES = (1, 2, 5)  # fewer than six rows: singular by both formulations
SWEEP_SIZES = GUARD_SIZES + (6, 7, 63, 64, 65, 255, 256, 257, 511, 513, STRIDE - 1, STRIDE, STRIDE + 1, STRIDE + 257,
                             3 * STRIDE + 100)
SWEEP_SCHEMES = ("default", "huber", "cauchy")
ALL_SCHEME_SIZES = (257, STRIDE + 1)
SIGMA = dict(A.SCHEME_SIGMA)  # huber 0.05: the residuals below spread over 1e-3 .. 1e-1 m, both branches occur
OFFSET = np.array([0.1, -0.07, 0.05, 0.01, -0.006, 0.008])  # 0.1 m / 0.01 rad
# the point-to-point offsets of the small sizes, scaled until both float64 determinants clear [1e-8, 1e-6] (asserted by the
# CPU suite for every case): det H grows with the 12th power of the residuals' scale
P2P_SCALE = {6: 8.0, 7: 8.0}
_CACHE = {}


def cloud(n, seed=11, box=40.0):
    """(ref [n,3] float32, unit normals [n,3] float32, unit noise [n,3]): n seeded points of a `box` m box."""
    key = ("cloud", n, seed, box)
    if key not in _CACHE:
        rng = np.random.default_rng(seed + n)
        ref = rng.uniform(-box / 2, box / 2, (n, 3))
        nrm = rng.normal(size=(n, 3))
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        _CACHE[key] = (ref.astype(F32), nrm.astype(F32), rng.normal(size=(n, 3)))
    ref, nrm, noise = _CACHE[key]
    return ref, nrm, noise


def moved(ref, noise, scale=1.0, noise_m=0.005):
    T = O.build_pose_matrix(OFFSET * scale, F64)
    back = np.linalg.inv(T)
    return (ref.astype(F64) @ back[:3, :3].T + back[:3, 3] + noise_m * scale * noise).astype(F32)


def sweep_case(cost, n):
    """(ref, tgt, normals or None, x0 None) of the size sweep."""
    ref, nrm, noise = cloud(n)
    scale = P2P_SCALE.get(n, 1.0) if cost == "point_to_point" else 1.0
    return ref, moved(ref, noise, scale), (nrm if cost == "point_to_plane" else None)


def sweep_sigma(scheme, n):
    """SIGMA, but cauchy at the guard sizes with sigma 1: at 0.1 its weights are about 1 / sigma = 10, H of five rows has
    eigenvalues of 1e4 and more, and the rounding noise of a float64 determinant of that rank-5 matrix (about 1e-16 x their
    product) is 1e2 .. 1e3, not below 1e-7: the status of those cases would be undetermined on every side."""
    return 1.0 if scheme == "cauchy" and n in GUARD_SIZES else SIGMA[scheme]


def sweep_cases():
    """(cost, scheme, n) of the size sweep: default / huber / cauchy at every size, all eight schemes at 257 and 65 537."""
    out = [(c, s, n) for c in COSTS for s in SWEEP_SCHEMES for n in SWEEP_SIZES]
    out += [(c, s, n) for c in COSTS for s in SCHEMES if s not in SWEEP_SCHEMES for n in ALL_SCHEME_SIZES]
    return out


def content_case(cost, n=STRIDE + 1, shift=None):
    """Rows of every kind at one seam: r == 0 rows, rows with 0 < |r| < 1e-4, both Huber branches; point-to-point: coincident
    p == q rows (r = 0, J = 0, the weight 0 / 1e-4); point-to-plane: non-unit and zero normals, taken as given.  `shift`: the
    whole scene moved by that offset (1 km, 10 km) before the rounding to float32."""
    ref, nrm, noise = cloud(n, seed=23)
    ref64 = ref.astype(F64) + (0.0 if shift is None else np.asarray(shift, F64))
    ref = ref64.astype(F32)
    T = np.linalg.inv(O.build_pose_matrix(OFFSET, F64))
    if shift is not None:  # the small motion about the scene's own origin
        g = np.eye(4)
        g[:3, 3] = shift
        T = g @ T @ np.linalg.inv(g)
    tgt = (ref.astype(F64) @ T[:3, :3].T + T[:3, 3] + 0.005 * noise).astype(F32)
    nrm = nrm.copy()
    k = np.arange(n)
    tgt[k % 17 == 3] = ref[k % 17 == 3]  # p == q: r = 0 at both seams
    near = k % 17 == 5  # a few ulp off the reference: 0 < |r| < 1e-4
    tgt[near] = np.nextafter(ref[near], F32(np.inf)) if shift is None else ref[near] + np.spacing(np.abs(ref[near]))
    if cost == "point_to_plane":
        nrm[k % 17 == 7] *= F32(2.5)  # non-unit normals
        nrm[k % 17 == 9] *= F32(0.01)
        nrm[k % 17 == 11] = 0.0  # zero normals: r = 0, J = 0
    return ref, tgt, (nrm if cost == "point_to_plane" else None)


def row_census(cost, ref, tgt, normals, scheme="huber", sigma=None):
    """Which rows a case holds, by the model's own residuals (the census of projective_cases.residual_census + the kinds of
    this seam)."""
    sigma = SIGMA["huber"] if sigma is None else sigma
    rows = seam_rows(cost, ref, tgt, normals, None, "least_square", sigma)
    a = np.abs(rows["r"])
    out = dict(quadratic=int((a < F32(sigma)).sum()), linear=int((a >= F32(sigma)).sum()),
               clamped=int(((a < F32(1.0e-4)) & (a > 0)).sum()), zero=int((a == 0).sum()),
               coincident=int((np.asarray(ref, F32) == np.asarray(tgt, F32)).all(axis=1).sum()))
    if normals is not None:
        ln = np.linalg.norm(np.asarray(normals, F64), axis=1)
        out.update(zero_normals=int((ln == 0).sum()), non_unit_normals=int(((np.abs(ln - 1) > 1e-3) & (ln > 0)).sum()))
    return out


X0_CASES = {"zero": [0, 0, 0, 0, 0, 0], "small": [0.1, -0.05, 0.02, 0.002, -0.003, 0.01], "yaw_3rad": [0, 0, 0, 0, 0, 3.0],
            "pitch_half_pi": [0, 0, 0, 0, float(F32(np.pi / 2)), 0], "translation": [1.5, -2.0, 0.25, 0, 0, 0]}
# (neighborhood weighs by the RAW target, tens of metres from its reference under a large x0: sigma 30 m, or every weight
# underflows to 0 and the case is an Invalid Jacobian on both sides)
X0_SCHEMES = (("least_square", 0.5), ("huber", 0.1), ("neighborhood", 30.0))
X0_SIZES = (257, STRIDE + 1)


def x0_case(name, n, aligned=False):
    """(ref, tgt, x0) at the linearisation point `name`: the targets are the references taken back by T(x0) and by OFFSET,
    so that T(x0) brings them within 0.1 m / 0.01 rad.  `aligned`: tgt exactly on T(x0)^-1 ref in the model's own float32
    arithmetic where that is possible — see x0_guard_case."""
    ref, _, noise = cloud(n, seed=31)
    x0 = np.array(X0_CASES[name], F32)
    back = np.linalg.inv(O.build_pose_matrix(x0.astype(F64), F64))
    mid = moved(ref, noise).astype(F64)
    return ref, (mid @ back[:3, :3].T + back[:3, 3]).astype(F32), x0


def x0_guard_case(n=257):
    """Targets ALREADY aligned under x0, every residual exactly 0: a translation-only x0 of powers of two and coordinates
    on a 2^-10 grid, so that (1 p + t) - q is exact in float32.  (ref, tgt, x0)."""
    rng = np.random.default_rng(41)
    tgt = (rng.integers(-20_000, 20_000, (n, 3)) / 1024.0).astype(F32)
    x0 = np.array([0.5, -2.0, 0.25, 0, 0, 0], F32)
    return (tgt + x0[:3]).astype(F32), tgt, x0


PROCRUSTES_SIZES = (1, 2, 3, 255, 256, 257, STRIDE + 1, 3 * STRIDE + 100)
WEIGHT_KINDS = ("none", "uniform", "random", "one_nonzero", "negative", "zero_sum")
SHAPE_KINDS = ("collinear", "coplanar", "all_equal", "mirrored", "half_turn", "offset_1km")


def procrustes_cloud(n, seed=51):
    ref, _, noise = cloud(n, seed=seed)
    T = O.build_pose_matrix(np.array([0.4, -0.3, 0.2, 0.03, -0.02, 0.3]), F64)
    return (ref.astype(F64) @ T[:3, :3].T + T[:3, 3] + 0.01 * noise).astype(F32), ref  # (tgt, ref)


def procrustes_weights(kind, n, seed=61):
    rng = np.random.default_rng(seed + n)
    if kind == "none":
        return None
    if kind == "uniform":
        return np.full(n, 0.25, F32)
    if kind == "random":
        return rng.uniform(0.1, 2.0, n).astype(F32)
    if kind == "one_nonzero":
        w = np.zeros(n, F32)
        w[n // 2] = 3.0
        return w
    if kind == "negative":
        w = rng.uniform(0.5, 1.5, n).astype(F32)
        w[::3] = -0.25
        return w
    w = np.ones(n, F32)  # zero_sum: exactly 0 in float64 (the kernel's accumulator) for every order of addition
    w[: n // 2] = -1.0
    if n % 2:
        w[-1] = 0.0
    return w


def procrustes_shape(kind, n=257):
    """(tgt, ref) of the cloud shapes."""
    tgt, ref = procrustes_cloud(n, seed=71)
    if kind == "collinear":
        s = np.linspace(-10, 10, n)[:, None]
        ref = (s * np.array([[1.0, 2.0, -0.5]]) + [3.0, 1.0, 2.0]).astype(F32)
        tgt = (s * np.array([[2.0, -1.0, 0.5]]) + [-1.0, 0.5, 0.0]).astype(F32)
    elif kind == "coplanar":
        import os
        g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "alignment.npz"))
        tgt, ref = g["flat_tgt"], g["flat_ref"]
    elif kind == "all_equal":
        tgt = np.tile(np.array([[1.0, 2.0, 3.0]], F32), (n, 1))
        ref = tgt + F32(0.5)
    elif kind == "mirrored":
        tgt = (ref * np.array([1, 1, -1], F32)).astype(F32)
    elif kind == "half_turn":
        tgt = (ref * np.array([-1, -1, 1], F32) + np.array([0.5, 0.25, -1.0], F32)).astype(F32)
    elif kind == "offset_1km":
        shift = np.array([1000.0, -1000.0, 100.0])
        tgt, ref = (tgt.astype(F64) + shift).astype(F32), (ref.astype(F64) + shift).astype(F32)
    else:
        raise AssertionError(kind)
    return np.ascontiguousarray(tgt), np.ascontiguousarray(ref)


CONTENT_SCHEMES = ("huber", "square_geman_mcclure", "neighborhood")
OFFSETS = {"offset_1km": (1000.0, -1000.0, 100.0), "offset_10km": (10000.0, -10000.0, 100.0)}
NAN_SIZES = (257, STRIDE + 1)


def nan_case(cost, n, where):
    """The sweep's case of n rows with a NaN target row at the first, a middle or the last position."""
    ref, tgt, nrm = sweep_case(cost, n)
    tgt = tgt.copy()
    row = {"first": 0, "middle": n // 2, "last": n - 1}[where]
    tgt[row, 1] = np.nan
    return ref, tgt, nrm, row


def seam_cases(families=("sweep", "content", "offsets", "nan", "x0")):
    """Every seam case of the device tests: (label, cost, scheme, sigma, ref, tgt, normals, x0), generated one at a time."""
    if "sweep" in families:
        for cost, scheme, n in sweep_cases():
            yield (f"sweep {cost} {scheme} n={n}", cost, scheme, sweep_sigma(scheme, n)) + sweep_case(cost, n) + (None,)
    if "content" in families:
        for cost in COSTS:
            for scheme in CONTENT_SCHEMES:
                yield (f"content {cost} {scheme}", cost, scheme, SIGMA[scheme]) + content_case(cost) + (None,)
    if "offsets" in families:
        for cost in COSTS:
            for name, shift in OFFSETS.items():
                for scheme in ("default", "huber"):
                    yield (f"{name} {cost} {scheme}", cost, scheme, SIGMA[scheme]) + content_case(cost, 4097, shift) + (None,)
    if "nan" in families:
        for cost in COSTS:
            for n in NAN_SIZES:
                for where in ("first", "middle", "last"):
                    yield (f"nan {cost} n={n} {where}", cost, "huber", SIGMA["huber"]) + nan_case(cost, n, where)[:3] + (None,)
    if "x0" in families:
        for name in X0_CASES:
            for n in X0_SIZES:
                for scheme, sigma in X0_SCHEMES:
                    ref, tgt, x0 = x0_case(name, n)
                    yield (f"x0 {name} {scheme} n={n}", "point_to_point", scheme, sigma, ref, tgt, None, x0)
        ref, tgt, x0 = x0_guard_case()
        yield ("x0 residual guard", "point_to_point", "huber", 0.1, ref, tgt, None, x0)


def procrustes_cases():
    """Every Procrustes case of the device tests: (label, tgt, ref, weights)."""
    for n in PROCRUSTES_SIZES:
        tgt, ref = procrustes_cloud(n)
        for kind in WEIGHT_KINDS:
            if n > 257 and kind not in ("none", "random", "zero_sum"):
                continue
            yield f"n={n} weights {kind}", tgt, ref, procrustes_weights(kind, n)
    for kind in SHAPE_KINDS:
        tgt, ref = procrustes_shape(kind)
        for wk in ("none", "random"):
            yield f"{kind} weights {wk}", tgt, ref, procrustes_weights(wk, len(tgt))
