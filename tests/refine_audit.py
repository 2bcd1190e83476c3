"""Float64 numpy model of the cloud-to-cloud refiner (icp_refine_*, include/icp_mi355x.h), operation by operation, with a
brute-force search — and the clouds its tests share.  `wrong=` selects one deliberately wrong reading of the specification.

Measured on the convergent clouds of `convergent_cases()` (tests/test_refine_audit.py asserts both):
  summation spread   max|dT| of the free-running result under reversed summation order: 8.9e-16 (cube), 1.05e-14 (lattice);
                     SPREAD = 1.1e-14 is the unit of the free-running bar;
  the model's step   numpy.linalg.svd against Horn's quaternion through eigh on the same H, max|dR| in units of
                     u * 2 |H|_F / (sigma_2 + s sigma_3), u = 2^-53, over every evaluation of those runs: worst 3.6
                     (3.514); STEP_UNITS = 3.6 is the unit of the step bar, which is 4 x 3.6 = 14.4.
The lattice trap: on the 0.4 m lattice a cloud moved by 0.3 m or more locks onto the neighbouring site (it stops by its own
test 0.39 m from the truth); `trap_case()` creeps for all 30 iterations and is the case for converged == 0."""
import functools

import numpy as np

U = 2.0 ** -53
SPREAD = 1.1e-14      # the unit of the free-running bar
STEP_UNITS = 3.6      # the unit of the step bar: the measured worst of the model's two routes
WRONG = ("inclusive", "ties_high", "d2_float32", "incremental", "no_reflection", "H_transposed", "means_kept",
         "zero_rows_counted", "fitness_only")


def zero_rows(rows):
    """the reference's `norm > 0` filter in float32: True where (x*x + y*y) + z*z is not > 0"""
    r = np.asarray(rows, np.float32)
    with np.errstate(all="ignore"):
        s = (r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2]
        return ~(s > np.float32(0))


def move(T, rows):
    """p'_a = ((T_a0 x + T_a1 y) + T_a2 z) + T_a3 on the float32 rows converted to float64"""
    r = np.asarray(rows, np.float32).astype(np.float64)
    x, y, z = r[:, 0], r[:, 1], r[:, 2]
    with np.errstate(all="ignore"):
        return np.stack([((T[a, 0] * x + T[a, 1] * y) + T[a, 2] * z) + T[a, 3] for a in range(3)], axis=1)


def correspond(P, target, usable, max_distance, wrong=None, chunk=512):
    """(row or -1, d2) of every moved point against the usable target rows: the smallest (d2, row) with d2 < max_distance^2"""
    r2 = np.float64(max_distance) * np.float64(max_distance)
    rows = np.flatnonzero(usable)
    Q = np.asarray(target, np.float32)[rows].astype(np.float64)
    out, out_d2 = np.full(len(P), -1, np.int64), np.zeros(len(P))
    if len(rows) == 0:
        return out, out_d2
    for lo in range(0, len(P), chunk):
        p = P[lo:lo + chunk]
        with np.errstate(all="ignore"):
            if wrong == "d2_float32":
                pf, qf = p.astype(np.float32), Q.astype(np.float32)
                dx, dy, dz = (pf[:, None, a] - qf[None, :, a] for a in range(3))
                d2 = ((dx * dx + dy * dy) + dz * dz).astype(np.float64)
            else:
                dx, dy, dz = (p[:, None, a] - Q[None, :, a] for a in range(3))
                d2 = (dx * dx + dy * dy) + dz * dz
            ok = (d2 <= r2) if wrong == "inclusive" else (d2 < r2)
        d2 = np.where(ok, d2, np.inf)
        if wrong == "ties_high":
            best = d2.shape[1] - 1 - np.argmin(d2[:, ::-1], axis=1)
        else:
            best = np.argmin(d2, axis=1)  # (the first minimum: the lowest row)
        dmin = d2[np.arange(len(p)), best]
        found = np.isfinite(dmin)
        out[lo:lo + chunk] = np.where(found, rows[best], -1)
        out_d2[lo:lo + chunk] = np.where(found, dmin, 0.0)
    return out, out_d2


def _sum(v, reverse):
    v = np.asarray(v, np.float64)
    return np.sum(v[::-1] if reverse else v, axis=0)


class Evaluation:
    pass


def evaluate(T, source, target, max_distance, drop_source=False, drop_target=False, wrong=None, reverse=False, P=None):
    """One evaluation at T: correspondences, counts, fitness, rmse and the 17 figures (count, sum d2, mu_p, mu_q, H)."""
    source, target = np.asarray(source, np.float32).reshape(-1, 3), np.asarray(target, np.float32).reshape(-1, 3)
    e = Evaluation()
    src_out = zero_rows(source) if drop_source else np.zeros(len(source), bool)
    tgt_out = zero_rows(target) if drop_target else np.zeros(len(target), bool)
    usable = ~tgt_out & np.isfinite(target.astype(np.float64)).all(axis=1)
    P = move(T, source) if P is None else P
    ask = ~src_out & np.isfinite(P).all(axis=1)
    corr, d2 = np.full(len(source), -1, np.int64), np.zeros(len(source))
    corr[ask], d2[ask] = correspond(P[ask], target, usable, max_distance, wrong)
    e.P, e.corr, e.d2 = P, corr, d2
    e.source_left_out, e.target_left_out = int(src_out.sum()), int(tgt_out.sum())
    e.counted = len(source) if wrong == "zero_rows_counted" else len(source) - e.source_left_out
    hit = corr >= 0
    e.count = int(hit.sum())
    e.sum_d2 = float(_sum(d2[hit], reverse)) if e.count else 0.0
    e.fitness, e.rmse = fitness_rmse(e.count, e.counted, e.sum_d2)
    e.fig = np.zeros(17)
    e.fig[0], e.fig[1] = e.count, e.sum_d2
    if e.count:
        p, q = P[hit], target[corr[hit]].astype(np.float64)
        mp, mq = _sum(p, reverse) / e.count, _sum(q, reverse) / e.count
        a, b = (p, q) if wrong == "means_kept" else (p - mp, q - mq)
        H = _sum(b[:, :, None] * a[:, None, :], reverse) / e.count
        e.fig[2:5], e.fig[5:8], e.fig[8:] = mp, mq, (H.T if wrong == "H_transposed" else H).reshape(-1)
    return e


def fitness_rmse(count, counted, sum_d2):
    if count <= 0:
        return 0.0, 0.0
    return float(np.float64(count) / np.float64(counted)), float(np.sqrt(np.float64(sum_d2) / np.float64(count)))


def pivot(target, drop_target=False):
    """the centre of the bounding box of the target rows in the grid: what the kernels take their sums about"""
    t = np.asarray(target, np.float32).reshape(-1, 3)
    keep = np.isfinite(t.astype(np.float64)).all(axis=1) & ~(zero_rows(t) if drop_target else np.zeros(len(t), bool))
    if not keep.any():
        return np.zeros(3)
    k = t[keep].astype(np.float64)
    return 0.5 * (k.min(axis=0) + k.max(axis=0))


def figures_exact(e, target, c):
    """the 17 figures of an evaluation in extended precision, and the bound gamma_n * sum|terms| (+ the rounding of the last
    operations) of a float64 summation about the pivot c in ANY order: (figures, bounds)"""
    L = np.longdouble
    fig, tol = np.zeros(17), np.zeros(17)
    hit = e.corr >= 0
    n = int(hit.sum())
    fig[0] = n
    if n == 0:
        return fig, tol
    g = (n + 8) * U / (1 - (n + 8) * U)
    p, q = e.P[hit].astype(L), np.asarray(target, np.float32)[e.corr[hit]].astype(L)
    d2 = e.d2[hit].astype(L)
    fig[1], tol[1] = float(d2.sum()), g * float(np.abs(d2).sum())
    a, b = p - c.astype(L), q - c.astype(L)
    ma, mb = a.sum(axis=0) / n, b.sum(axis=0) / n
    ta, tb = g * (np.abs(a).sum(axis=0) / n).astype(np.float64), g * (np.abs(b).sum(axis=0) / n).astype(np.float64)
    fig[2:5], fig[5:8] = (c + ma).astype(np.float64), (c + mb).astype(np.float64)
    tol[2:5], tol[5:8] = ta + 4 * U * (np.abs(c) + np.abs(fig[2:5])), tb + 4 * U * (np.abs(c) + np.abs(fig[5:8]))
    M = (b[:, :, None] * a[:, None, :]).sum(axis=0) / n
    Mabs = (np.abs(b)[:, :, None] * np.abs(a)[:, None, :]).sum(axis=0) / n
    H = M - mb[:, None] * ma[None, :]
    am, bm = np.abs(ma).astype(np.float64), np.abs(mb).astype(np.float64)
    tH = g * Mabs.astype(np.float64) + bm[:, None] * ta[None, :] + tb[:, None] * am[None, :] + 4 * U * (np.abs(M).astype(np.float64) + bm[:, None] * am[None, :])
    fig[8:], tol[8:] = H.astype(np.float64).reshape(-1), tH.reshape(-1)
    return fig, tol


def rotation_svd(H, wrong=None):
    Um, S, Vt = np.linalg.svd(H)
    s = 1.0 if wrong == "no_reflection" else (1.0 if np.linalg.det(Um) * np.linalg.det(Vt) >= 0 else -1.0)
    return Um @ np.diag([1.0, 1.0, s]) @ Vt


def rotation_horn(H):
    S = H.T  # S_ab = sum p'_a q_b
    N = np.array([[S[0, 0] + S[1, 1] + S[2, 2], S[1, 2] - S[2, 1], S[2, 0] - S[0, 2], S[0, 1] - S[1, 0]],
                  [S[1, 2] - S[2, 1], S[0, 0] - S[1, 1] - S[2, 2], S[0, 1] + S[1, 0], S[2, 0] + S[0, 2]],
                  [S[2, 0] - S[0, 2], S[0, 1] + S[1, 0], S[1, 1] - S[0, 0] - S[2, 2], S[1, 2] + S[2, 1]],
                  [S[0, 1] - S[1, 0], S[2, 0] + S[0, 2], S[1, 2] + S[2, 1], S[2, 2] - S[0, 0] - S[1, 1]]])
    w, x, y, z = np.linalg.eigh(N)[1][:, -1]
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def condition_unit(H):
    """u * 2 |H|_F / (sigma_2 + s sigma_3): the condition number of the polar factor (inf where it is not unique)"""
    Um, S, Vt = np.linalg.svd(H)
    s = 1.0 if np.linalg.det(Um) * np.linalg.det(Vt) >= 0 else -1.0
    den = S[1] + s * S[2]
    return np.inf if not den > 0 else U * 2 * np.linalg.norm(H) / den


def step(fig, wrong=None, route="svd"):
    """update [4,4] from the 17 figures: R, t = mu_q - R mu_p; the identity without a correspondence"""
    up = np.eye(4)
    if not fig[0] > 0:
        return up
    H = fig[8:].reshape(3, 3)
    R = rotation_horn(H) if route == "horn" else rotation_svd(H, wrong)
    up[:3, :3], up[:3, 3] = R, fig[5:8] - R @ fig[2:5]
    return up


def mul44(a, b):
    return np.array([[((a[i, 0] * b[0, j] + a[i, 1] * b[1, j]) + a[i, 2] * b[2, j]) + a[i, 3] * b[3, j] for j in range(4)] for i in range(4)])


def run(source, target, init=None, max_distance=1.0, max_iteration=30, relative_fitness=1e-6, relative_rmse=1e-6, drop_source=False,
        drop_target=False, wrong=None, reverse=False):
    """The loop: evaluate at init; up to max_iteration times step, evaluate, stop test.  Returns a dict."""
    T = np.eye(4) if init is None else np.array(init, np.float64).reshape(4, 4)
    source = np.asarray(source, np.float32).reshape(-1, 3)
    limit = max_iteration if len(source) else 0
    P = move(T, source) if wrong == "incremental" else None
    e = evaluate(T, source, target, max_distance, drop_source, drop_target, wrong, reverse, P)
    hist_T, hist_e, it, converged = [T], [e], 0, False
    while it < limit:
        up = step(e.fig, wrong)
        T = mul44(up, T)
        if wrong == "incremental":  # Open3D's way: the moved copy is moved again, rounded to float32 rows here to show it
            P = move(up, P.astype(np.float32))
        it += 1
        prev, e = e, evaluate(T, source, target, max_distance, drop_source, drop_target, wrong, reverse, P)
        hist_T.append(T)
        hist_e.append(e)
        if abs(e.fitness - prev.fitness) < relative_fitness and (wrong == "fitness_only" or abs(e.rmse - prev.rmse) < relative_rmse):
            converged = True
            break
    return {"T": T, "fitness": e.fitness, "rmse": e.rmse, "iterations": it, "converged": converged, "corr": e.corr,
            "history_T": np.array(hist_T), "evaluations": hist_e}


# ---- clouds ------------------------------------------------------------------------------------------------------------
def rigid(yaw, t):
    c, s = np.cos(yaw), np.sin(yaw)
    M = np.eye(4)
    M[:3, :3] = [[c, -s, 0], [s, c, 0], [0, 0, 1]]
    M[:3, 3] = t
    return M


def _moved(rows, M):
    return (rows.astype(np.float64) @ M[:3, :3].T + M[:3, 3]).astype(np.float32)


def cube_case(n_target=5000, n_source=3000, seed=0, offset=(0.0, 0.0, 0.0)):
    """n_source rows of a uniform random cloud in a 20 m cube; the source is the target moved by the INVERSE of `truth`"""
    rng = np.random.default_rng(seed)
    target = (rng.uniform(-10, 10, (n_target, 3)) + np.asarray(offset)).astype(np.float32)
    truth = rigid(0.05, (0.2, -0.1, 0.1))
    centre = np.eye(4)
    centre[:3, 3] = offset
    truth = centre @ truth @ np.linalg.inv(centre)  # (the motion about the cloud's own centre)
    source = _moved(target[rng.permutation(n_target)[:n_source]], np.linalg.inv(truth))
    return source, target, truth


def lattice_case(shift=(0.1, 0.05, 0.0), yaw=0.01, n=100, pitch=0.4, n_source=6000, seed=1):
    """a subset of an n x n lattice at `pitch` with relief, moved by yaw and shift"""
    rng = np.random.default_rng(seed)
    i, j = np.meshgrid(np.arange(n) - n / 2, np.arange(n) - n / 2, indexing="ij")
    x, y = i.reshape(-1) * pitch, j.reshape(-1) * pitch
    z = 1.5 + np.sin(x * 0.31) * np.cos(y * 0.23) + 0.4 * np.sin(x * 1.3 + y * 0.7)
    target = np.stack([x, y, z], axis=1).astype(np.float32)
    truth = rigid(yaw, shift)
    source = _moved(target[rng.permutation(len(target))[:n_source]], np.linalg.inv(truth))
    return source, target, truth


@functools.lru_cache(maxsize=None)
def convergent_cases():
    return {"cube": cube_case(), "lattice": lattice_case()}


@functools.lru_cache(maxsize=None)
def free_run(name, reverse=False):
    """the free-running model on a named cloud, computed once a process"""
    s, t, _ = trap_case() if name == "trap" else convergent_cases()[name]
    return run(s, t, reverse=reverse)


def trap_case():
    """the lattice trap: yaw 0.1 rad and (0.3, 0.1, 0) m on a 0.4 m lattice: 30 iterations, never stopped by its own test"""
    return lattice_case(shift=(0.3, 0.1, 0.0), yaw=0.1, n=50, n_source=1500)


def small_case(n_target, n_source, seed=0, spread=3.0):
    """a small random pair a fraction of a metre apart: most source rows have a correspondence within 1 m"""
    rng = np.random.default_rng(1000 + seed)
    target = rng.uniform(-spread, spread, (n_target, 3)).astype(np.float32)
    pick = rng.integers(0, n_target, n_source)
    source = (target[pick].astype(np.float64) + rng.normal(0, 0.15, (n_source, 3))).astype(np.float32)
    return _moved(source, rigid(0.03, (0.1, -0.05, 0.02))), target
