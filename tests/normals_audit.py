"""The model the kNN map normals are held to (csrc/search.hip: k_normals, k_normals_all, k_normals_hood, k_normals_hood2 and
its batch form, k_normals_tail, k_normals_tail16, k_normals_owned, k_normals_generic, the lazy estimation inside k_iterate_*),
the clouds they are audited on and the comparison helpers.  TEST INFRASTRUCTURE, never imported by the package.

The model restates the source operation by operation in float32 (the library builds with -ffp-contract=off: a fused
multiply-add appears only where the source says fmaf):

  neighbour set   the k + 1 smallest keys (bits of d2, original index) of the map against the point, d2 =
                  fmaf(dz, dz, fmaf(dy, dy, dx * dx)) (knn_device.h: point_key; knn_audit.model_knn_multi), the first key
                  dropped (the point itself, or a duplicate of it with a lower index), entries beyond the map empty:
                  used = min(k, M - 1).
  covariance      centred on the POINT (not on the mean).  k = 5, 10, 20 (`CovSums`): d = q - p in float32, every float32
                  product through (float64(v) + 6144.0) - 6144.0, the six sums in float64, float32(sum) * (1 / float32(used)).
                  The sums are taken in ascending and in descending key order; a point whose two sums differ (or whose terms
                  leave the range in which float64 adds them exactly and whose exact sum is not what either order gave) is
                  ORDER-DEPENDENT: the kernels reach the neighbours in different orders, the model cannot say which bits come out.
                  Every other k (`k_normals_generic`): sequential float32 sums in ascending key order, then * invk.
  eigenvector     `smallest_eigenvector`: unit-trace scaling, at most 8 cyclic Jacobi sweeps in the order (0,1), (0,2), (1,2),
                  the `off <= 1e-9f` stop, the `apq == 0` skip, the three update loops (A <- A J, A <- J^T A, V <- V J), two
                  rounds of selection (ties to the LAST axis), 1 / sqrtf of the squared norm.  fmaf(x, x, 1) is emulated as
                  knn_audit._fma_sq does, its uncertain sums settled exactly (fma_sq1); a point whose emulation stays
                  uncertain, in the key or in the sweep, is flagged.

Flagged and order-dependent points are left out of bit comparisons and counted; the suites assert a cap (knn_audit.FLAGGED_MAX)
and the clouds here are chosen so that the count is zero.

Degenerate outputs follow from the same code: M = 1 gives a zero covariance, no rotation, three equal eigenvalues and, ties to
the last axis, (0, 0, 1); so does a map of equal points.  M = 2 gives a rank-1 matrix d d^T and what the sweeps leave of it.

The float64 truth (`truth_normals`): float64 k-NN, numpy.linalg.eigh of the float64 covariance, and the gap
(l1 - l0) / l2 that scales the bar: sin(angle) <= BAR * 2^-24 / gap wherever gap > GAP_MIN.  The first-order perturbation of
an eigenvector by an error E of the matrix is |E| / (l1 - l0); the unit-trace matrix carries float32 roundings of its entries
(|E| of a few 2^-24 relative to l2), hence the form of the bar.  BAR is four times the worst ratio MEASURED over the audit's
own clouds (the margin the other audits here take over a CPU-measured spread):
    the model against float64:      worst ratio 3.14 (the offset cloud at k = 32, a generic k with plain float32 sums;
                                    2.63 at worst for k = 5, 10, 20: the offset cloud at k = 20)
    the reference's float32 SVD:    worst ratio 2.40 (`icp_oracle.knn_normals`, local_map.py:397-422, same cloud and k)
so BAR = 12.56.  tests/test_normals_audit.py re-measures both and fails if the figure here is not the one the clouds give.
"""
import os
import re

import numpy as np

import knn_audit as KA

F32 = np.float32
GRID_KS = (5, 10, 20)          # the neighbourhood sizes with kernels of their own (CovSums); every other k is generic
GENERIC_KS = (1, 2, 3, 7, 12, 32, 64)
GAP_MIN = 1.0e-6
MEASURED_WORST = 3.14          # the model's worst ratio against float64 over clouds() x (GRID_KS + GENERIC_KS); see above
BAR = 4.0 * MEASURED_WORST
U24 = 2.0 ** -24
FLAGGED_MAX = KA.FLAGGED_MAX
_C = 6144.0                    # CovSums::grid: 1.5 * 2^12, ulp 2^-40
_EXACT_BELOW = 2.0 ** 13       # sums of multiples of 2^-40 below it are exact in float64 whatever their order


# ---- what the source says about its launches -----------------------------------------------------------------------------
def _source(name="search.hip"):
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, "..", "pylidar-slam_amd", "csrc", name)) as f:
        return f.read()


def launch_shapes():
    """points per workgroup of every kernel family and the block caps, read from csrc/search.hip"""
    src = _source()

    def const(name):
        m = re.search(r"static constexpr int %s = (\d+);" % name, src)
        assert m, name
        return int(m.group(1))

    nrm, nrm2, tail16 = const("NRM_THREADS"), const("NRM2_THREADS"), const("TAIL16_THREADS")
    cap = re.search(r"static int worklist_blocks\(.*?if \(blocks > (\d+)\) blocks = \1;", src, re.S)
    generic = re.search(r"__launch_bounds__\((\d+)\) void k_normals_generic", src)
    kmax = re.search(r"k_normals_generic.*?constexpr int KMAX = (\d+);", src, re.S)
    assert cap and generic and kmax
    return {"four_lanes": nrm // 4, "two_lanes": nrm // 2, "pair": nrm2 // 2, "tail16_rows": tail16 // 16,
            "generic_threads": int(generic.group(1)), "worklist_blocks_max": int(cap.group(1)), "generic_kmax": int(kmax.group(1))}


# ---- the model -----------------------------------------------------------------------------------------------------------
class Normals:
    """normals [M, 3] float32, neighbours [M, k] int32 (M = empty), cov [M, 6] float32, used [M], flagged [M] bool (an
    uncertain fmaf emulation in the key or the sweep), order_dependent [M] bool, sweeps [M] (rotating sweeps taken),
    keys [M, k + 1] int32: the whole list, the dropped first key included (what a k-NN query for k + 1 returns).  `rows`: the
    map points modelled where they are not all of them (every array then has one entry per row of `rows`)."""

    def __init__(self, k, normals, neighbours, cov, used, flagged, order_dependent, sweeps, keys=None, rows=None):
        self.k, self.normals, self.neighbours, self.cov, self.used = k, normals, neighbours, cov, used
        self.flagged, self.order_dependent, self.sweeps, self.keys, self.rows = flagged, order_dependent, sweeps, keys, rows

    @property
    def left_out(self):
        return self.flagged | self.order_dependent


def neighbour_lists(cloud, ks, extra=0, higher_index_ties=False, rows=None):
    """{k: (lists [M, k + 1 + extra] int32 with M for an empty entry, flagged [M])}: the k + 1 (+ extra) smallest keys of every
    map point, from ONE evaluation of the distances.  `higher_index_ties`: the wrong copy whose ties go to the higher index (the
    right one on the reversed cloud).  `rows`: the lists of these map points only."""
    cloud = np.ascontiguousarray(cloud, F32)
    m = cloud.shape[0]
    assert rows is None or not higher_index_ties
    src = np.ascontiguousarray(cloud[::-1]) if higher_index_ties else cloud
    queries = src if rows is None else np.ascontiguousarray(cloud[rows])
    got = KA.model_knn_multi(src, queries, tuple(sorted({k + 1 + extra for k in ks})))
    out = {}
    for k in ks:
        r = got[k + 1 + extra]
        idx, flagged = r.index, r.flagged
        if higher_index_ties:
            idx = np.where(idx < m, m - 1 - idx, m)[::-1]
            flagged = flagged[::-1]
        out[k] = (np.ascontiguousarray(idx, np.int32), np.ascontiguousarray(flagged))
    return out


def _deltas(cloud, nb, centre_on_mean=False, rows=None):
    m = cloud.shape[0]
    valid = nb < m
    q = cloud[np.minimum(nb, m - 1)]
    centre = (cloud if rows is None else cloud[rows])[:, None, :]
    if centre_on_mean:
        cnt = np.maximum(valid.sum(axis=1), 1).astype(F32)
        centre = (np.where(valid[:, :, None], q, F32(0)).sum(axis=1, dtype=F32) / cnt[:, None])[:, None, :]
    with np.errstate(invalid="ignore", over="ignore"):
        d = q - centre
    return d, valid


_PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


def cov_grid(cloud, nb, divisor=None, centre_on_mean=False, rows=None):
    """(cov [M, 6] float32, used [M], order_dependent [M]) as CovSums computes it over the neighbours `nb` [M, k] (M = empty)"""
    d, valid = _deltas(cloud, nb, centre_on_mean, rows)
    used = valid.sum(axis=1).astype(np.int32)
    n, k = nb.shape
    cov = np.zeros((n, 6), F32)
    dependent = np.zeros(n, bool)
    div = used if divisor is None else np.full(n, divisor, np.int32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        invk = np.where(div > 0, F32(1.0) / div.astype(F32), F32(0.0)).astype(F32)
        for c, (a, b) in enumerate(_PAIRS):
            prod = d[:, :, a] * d[:, :, b]                                    # float32 products
            g = np.where(valid, (prod.astype(np.float64) + _C) - _C, 0.0)
            fwd, rev = np.zeros(n), np.zeros(n)
            for j in range(k):
                fwd = fwd + g[:, j]
                rev = rev + g[:, k - 1 - j]
            dependent |= ~((fwd == rev) | (np.isnan(fwd) & np.isnan(rev)))
            # beyond the range of the grid the partial sums of SOME order may round: exact integers of 2^-40 decide
            wide = np.flatnonzero((np.abs(g).sum(axis=1) >= _EXACT_BELOW) & np.isfinite(fwd))
            for r in wide:
                exact = sum(int(v * 2.0 ** 40) for v in g[r])
                if float(exact) * 2.0 ** -40 != fwd[r] or int(fwd[r] * 2.0 ** 40) != exact:
                    dependent[r] = True
            cov[:, c] = fwd.astype(F32) * invk
    return cov, used, dependent


def cov_plain(cloud, nb, divisor=None, rows=None):
    """(cov, used) as k_normals_generic computes it: sequential float32 sums in ascending key order, then * invk"""
    d, valid = _deltas(cloud, nb, rows=rows)
    used = valid.sum(axis=1).astype(np.int32)
    n, k = nb.shape
    cov = np.zeros((n, 6), F32)
    div = used if divisor is None else np.full(n, divisor, np.int32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        invk = np.where(div > 0, F32(1.0) / div.astype(F32), F32(0.0)).astype(F32)
        for c, (a, b) in enumerate(_PAIRS):
            s = np.zeros(n, F32)
            for j in range(k):
                s = np.where(valid[:, j], s + d[:, j, a] * d[:, j, b], s)
            cov[:, c] = s * invk
    return cov, used


def fma_sq1(a32):
    """fmaf(a, a, 1.0f) of a float32 array, and the entries that stay uncertain.  knn_audit._fma_sq leaves the sums that land
    on the middle between two float32 values open (a rotation angle theta with a short mantissa and theta^2 >> 1 does: the
    float64 sum drops the 1 that decides); those few are settled with exact rationals, rounded to nearest even as fmaf does."""
    from fractions import Fraction
    r, unsure = KA._fma_sq(a32, np.ones_like(a32))
    for i in np.flatnonzero(unsure):
        exact = Fraction(float(a32[i])) ** 2 + 1
        near = F32(float(exact))                       # (within one float32 step of the answer)
        best = None
        for c in (np.nextafter(near, F32(-np.inf)), near, np.nextafter(near, F32(np.inf))):
            if not np.isfinite(c):
                break
            err = abs(Fraction(float(c)) - exact)
            even = (int(np.asarray(c, F32).view(np.uint32)) & 1) == 0
            if best is None or err < best[0] or (err == best[0] and even):
                best = (err, c)
        else:
            r[i] = best[1]
            unsure[i] = False
    return r, unsure


def smallest_eigenvector(cov, sweeps=8, ties_first=False):
    """(normals [n, 3] float32, unsure [n], rotating sweeps [n]) of cov [n, 6] = {c00, c01, c02, c11, c12, c22}: the function
    of csrc/search.hip from `const float tr = ...` to its end.  `sweeps`, `ties_first`: the wrong copies."""
    cov = np.asarray(cov, F32)
    n = cov.shape[0]
    one, zero = F32(1.0), F32(0.0)
    a00, a01, a02, a11, a12, a22 = (cov[:, i] for i in range(6))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        tr = (a00 + a11) + a22
        sc = np.where(tr > 0, one / tr, one).astype(F32)
        A = [[a00 * sc, a01 * sc, a02 * sc], [a01 * sc, a11 * sc, a12 * sc], [a02 * sc, a12 * sc, a22 * sc]]
        V = [[np.full(n, one if i == j else zero, F32) for j in range(3)] for i in range(3)]
        active = np.ones(n, bool)
        unsure = np.zeros(n, bool)
        taken = np.zeros(n, np.int32)
        for _ in range(sweeps):
            off = (np.abs(A[0][1]) + np.abs(A[0][2])) + np.abs(A[1][2])
            active &= ~(off <= F32(1e-9))
            if not active.any():
                break
            taken += active
            for p, q in ((0, 1), (0, 2), (1, 2)):
                apq = A[p][q]
                do = active & (apq != zero)
                if not do.any():
                    continue
                theta = (A[q][q] - A[p][p]) / (F32(2.0) * apq)
                r1, u1 = fma_sq1(theta)
                t = np.where(theta >= 0, one, -one).astype(F32) / (np.abs(theta) + np.sqrt(r1))
                r2, u2 = fma_sq1(t)
                c = one / np.sqrt(r2)
                s = t * c
                unsure |= do & (u1 | u2)
                for k in range(3):      # A <- A J
                    akp, akq = A[k][p], A[k][q]
                    A[k][p] = np.where(do, c * akp - s * akq, akp)
                    A[k][q] = np.where(do, s * akp + c * akq, akq)
                for k in range(3):      # A <- J^T A
                    apk, aqk = A[p][k], A[q][k]
                    A[p][k] = np.where(do, c * apk - s * aqk, apk)
                    A[q][k] = np.where(do, s * apk + c * aqk, aqk)
                for k in range(3):
                    vkp, vkq = V[k][p], V[k][q]
                    V[k][p] = np.where(do, c * vkp - s * vkq, vkp)
                    V[k][q] = np.where(do, s * vkp + c * vkq, vkq)
        c1 = (A[1][1] <= A[2][2]) if ties_first else (A[1][1] < A[2][2])
        lam = np.where(c1, A[1][1], A[2][2])
        x, y, z = (np.where(c1, V[i][1], V[i][2]) for i in range(3))
        c0 = (A[0][0] <= lam) if ties_first else (A[0][0] < lam)
        x, y, z = np.where(c0, V[0][0], x), np.where(c0, V[1][0], y), np.where(c0, V[2][0], z)
        inv = one / np.sqrt((x * x + y * y) + z * z)
        out = np.stack((x * inv, y * inv, z * inv), axis=1).astype(F32)
    return out, unsure, taken


WRONG_COPIES = ("kth_is_next", "first_kept", "ties_higher", "mean_centred", "other_sums", "divisor_k", "seven_sweeps",
                "ties_first_axis")


def model_normals_multi(cloud, ks, wrong=None, lists=None, rows=None):
    """{k: Normals} of every map point.  `wrong`: one of WRONG_COPIES, the copies the audit must tell from the model.
    `lists`: neighbour_lists(cloud, ks, extra=1) computed before (the distances are most of the model's time).  `rows`: these
    map points only (the model's time is in proportion)."""
    assert wrong is None or wrong in WRONG_COPIES, wrong
    cloud = np.ascontiguousarray(cloud, F32)
    assert cloud.ndim == 2 and cloud.shape[1] == 3
    m = cloud.shape[0]
    if rows is not None:
        rows = np.asarray(rows, np.int64)
        m = rows.shape[0]
    if wrong == "ties_higher":
        lists = neighbour_lists(cloud, ks, higher_index_ties=True)
    elif lists is None:
        lists = neighbour_lists(cloud, ks, extra=1 if wrong == "kth_is_next" else 0, rows=rows)
    out = {}
    for k in ks:
        full, flagged = lists[k]
        assert full.shape[1] >= k + (2 if wrong == "kth_is_next" else 1)
        if wrong == "kth_is_next":
            nb = np.concatenate((full[:, 1:k], full[:, k + 1:k + 2]), axis=1)
        elif wrong == "first_kept":
            nb = full[:, :k]
        else:
            nb = full[:, 1:k + 1]
        grid = (k in GRID_KS) != (wrong == "other_sums")
        divisor = k if wrong == "divisor_k" else None
        if grid:
            cov, used, dependent = cov_grid(cloud, nb, divisor, centre_on_mean=wrong == "mean_centred", rows=rows)
        else:
            assert wrong != "mean_centred" or k in GRID_KS
            cov, used = cov_plain(cloud, nb, divisor, rows=rows)
            dependent = np.zeros(m, bool)
        normals, unsure, sweeps = smallest_eigenvector(cov, sweeps=7 if wrong == "seven_sweeps" else 8,
                                                       ties_first=wrong == "ties_first_axis")
        out[k] = Normals(k, normals, np.ascontiguousarray(nb), cov, used, flagged | unsure, dependent, sweeps,
                         np.ascontiguousarray(full[:, :k + 1]), rows)
    return out


def model_normals(cloud, k, wrong=None, rows=None):
    return model_normals_multi(cloud, (k,), wrong, rows=rows)[k]


# ---- the float64 truth ---------------------------------------------------------------------------------------------------
def eig_truth(nb_points64, centre64):
    """(normal [n, 3], gap [n]) of float64 neighbourhoods [n, k, 3] around centres [n, 3]"""
    c = nb_points64 - centre64[:, None, :]
    cov = (c[:, :, :, None] * c[:, :, None, :]).mean(axis=1)
    w, v = np.linalg.eigh(cov)
    with np.errstate(invalid="ignore", divide="ignore"):
        gap = np.where(w[:, 2] > 0, (w[:, 1] - w[:, 0]) / w[:, 2], 0.0)
    return v[:, :, 0], gap


def truth_normals(cloud, k):
    """(normal [M, 3] float64, gap [M], determined [M]) — float64 k-NN (k + 1, the first dropped), eigh of the float64
    covariance; `determined`: M > k + 1, gap > GAP_MIN and a neighbour set no tie or near tie leaves to the tie order (the
    k + 1-th and k + 2-th distances apart by more than knn_audit.AMBIGUOUS_REL, and the point its own nearest neighbour)."""
    m = cloud.shape[0]
    if m < k + 2:
        return np.zeros((m, 3)), np.zeros(m), np.zeros(m, bool)
    dist, idx = KA.truth_knn(cloud, cloud, k + 2)
    c64 = cloud.astype(np.float64)
    normal, gap = eig_truth(c64[idx[:, 1:k + 1]], c64)
    with np.errstate(invalid="ignore"):
        apart = (dist[:, k + 1] - dist[:, k]) > KA.AMBIGUOUS_REL * dist[:, k + 1]
        own = (idx[:, 0] == np.arange(m)) & (dist[:, 1] > 0)
    return normal, gap, apart & own & (gap > GAP_MIN)


def sin_angle(a, b):
    """sin of the angle between the LINES of a and b (a normal's sign is free)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    cr = np.cross(a, b)
    na, nb = np.linalg.norm(a, axis=1), np.linalg.norm(b, axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.linalg.norm(cr, axis=1) / (na * nb)


def truth_ratio(normals, truth, rows=None):
    """worst sin(angle) * gap / 2^-24 of `normals` against truth_normals' tuple over its determined rows (of `rows`), and
    how many rows that were"""
    normal, gap, determined = truth
    use = determined.copy()
    if rows is not None:
        sel = np.zeros_like(use)
        sel[rows] = True
        use &= sel
    if not use.any():
        return 0.0, 0
    ratio = sin_angle(np.asarray(normals)[use], normal[use]) * gap[use] / U24
    assert np.isfinite(ratio).all()
    return float(ratio.max()), int(use.sum())


# ---- comparison helpers --------------------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def differing(normals, want, rows=None):
    """the compared map points (of `rows`) whose normal differs from the model's in any bit"""
    normals = np.asarray(normals)
    if want.rows is not None:   # (a model of some rows: `normals` is by map index, `rows` counts within the model's)
        normals = normals[want.rows]
    assert normals.dtype == np.float32 and normals.shape == want.normals.shape, (normals.dtype, normals.shape, want.normals.shape)
    use = ~want.left_out
    if rows is not None:
        sel = np.zeros_like(use)
        sel[rows] = True
        use &= sel
    return np.flatnonzero(np.any(_bits(normals) != _bits(want.normals), axis=1) & use), int(use.sum())


def check_bits(normals, want, rows=None, what=""):
    """`normals` [M, 3] float32 (by original index) against the model, bit for bit on every map point (of `rows`) the model
    does not leave out; the first differing point is reported with its neighbour list, covariance and both normals.  Returns
    the number of points compared."""
    bad, compared = differing(normals, want, rows)
    if bad.size:
        s = int(bad[0])
        at = s if want.rows is None else int(want.rows[s])
        raise AssertionError(
            f"{what}: the normals of {bad.size} of {compared} map points differ from the model (k = {want.k}), first point {at}: "
            f"{np.asarray(normals)[at].tolist()} against {want.normals[s].tolist()}; neighbours {want.neighbours[s].tolist()}, "
            f"used {int(want.used[s])}, covariance {want.cov[s].tolist()}, {int(want.sweeps[s])} sweeps")
    return compared


def check_caps(want, what=""):
    """at most FLAGGED_MAX of the map points flagged, and as many order-dependent; returns both counts"""
    m = max(1, want.normals.shape[0])
    f, d = int(want.flagged.sum()), int(want.order_dependent.sum())
    assert f <= FLAGGED_MAX * m and d <= FLAGGED_MAX * m, (what, want.k, f, d, m)
    return f, d


# ---- clouds --------------------------------------------------------------------------------------------------------------
_CACHE = {}
EDGE_SIZES = (63, 64, 65, 127, 128, 129, 1023, 1024, 1025)   # the workgroup edges of every kernel (launch_shapes())
PAIR_EXPECTED = (0.35856858, 0.71713716, -0.5976144)         # M = 2: the pair (0, 0, 0), (1, 2, 3)


def lidar():
    """about 8 192 points: a 16-row synthetic scene (four scans in one frame): dense ring-1 hits, stragglers, the coarse level"""
    if "lidar" not in _CACHE:
        from pylidar_slam_amd.synthetic import SceneConfig, make_fixed_map, make_sequence
        cfg = SceneConfig(height=16, width=512)
        scans, poses = make_sequence(cfg, 4)
        c = np.ascontiguousarray(make_fixed_map(cfg, scans, poses, ref_frame=3, num_points=8192), F32)
        c.setflags(write=False)
        _CACHE["lidar"] = c
    return _CACHE["lidar"]


def clouds():
    """{name: cloud}: the stress clouds of the audit (the tiny and the workgroup-edge maps come from tiny_maps / edge_maps)"""
    if "clouds" not in _CACHE:
        rng = np.random.default_rng(21)
        out = {"lidar": lidar()}
        ax = np.arange(24, dtype=F32) * F32(0.25)
        out["lattice"] = np.stack(np.meshgrid(ax, ax, ax[:12], indexing="ij"), axis=-1).reshape(-1, 3)
        base = (rng.normal(size=(1500, 3)) * np.array([10.0, 10.0, 1.0])).astype(F32)
        out["duplicates"] = np.repeat(base[:400], rng.integers(1, 24, size=400), axis=0)
        out["isolated"] = np.concatenate([base[:800], (rng.normal(size=(40, 3)) * 300 + 500).astype(F32)])
        out["offset"] = (base[:1000].repeat(2, axis=0) * np.array([1.0, 1.0, 0.5]) + rng.normal(size=(2000, 3)) * 0.5
                         + np.array([10000.0, -10000.0, 50.0])).astype(F32)
        t = np.sort(rng.random(300))
        out["line"] = (np.outer(t, [30.0, 12.0, 3.0]) + np.array([-4.0, 2.0, 0.5])).astype(F32)
        plane = (rng.random((500, 3)) * np.array([20.0, 20.0, 0.0])).astype(F32)
        out["plane"] = plane
        for c in out.values():
            c.setflags(write=False)
        _CACHE["clouds"] = {k: np.ascontiguousarray(v) for k, v in out.items()}
    return _CACHE["clouds"]


def tiny_maps(k):
    """maps of M = 1, 2, k, k + 1, k + 2 points (the head of the LiDAR cloud thinned so that they are not one scan row; the
    pair is PAIR_EXPECTED's)"""
    c = lidar()[::37]
    out = {"m1": c[:1], "m2": np.array([[0, 0, 0], [1, 2, 3]], F32)}
    for m in (k, k + 1, k + 2):
        if m > 2:
            out[f"m{m}"] = c[:m]
    return {n: np.ascontiguousarray(v) for n, v in out.items()}


def edge_maps():
    return {f"edge{m}": np.ascontiguousarray(lidar()[:m]) for m in EDGE_SIZES}


def tiled_lattice(copies):
    """(cloud, copy of every point): the lattice `copies` times, 64 m apart on a grid of eight columns.  Every coordinate and
    every difference within a copy stays exact in float32 and no other copy comes near a point's k + 1 <= 21 nearest, so the
    normal of point i of every copy is the model's normal of point i of the lattice: a map larger than any launch's grid
    without a brute force over it."""
    base = clouds()["lattice"]
    j = np.arange(copies)
    shift = np.stack((64.0 * (j % 8), 64.0 * (j // 8), np.zeros(copies)), axis=1).astype(F32)
    cloud = (base[None, :, :] + shift[:, None, :]).reshape(-1, 3)
    assert np.array_equal((cloud.reshape(copies, -1, 3) - shift[:, None, :]), np.broadcast_to(base, (copies,) + base.shape))
    return np.ascontiguousarray(cloud, F32), np.repeat(j, base.shape[0])


def model(name, cloud, k):
    """the model of a named cloud, computed once (all k of a cloud from one evaluation of the distances)"""
    key = ("model", name)
    if key not in _CACHE:
        _CACHE[key] = {}
    have = _CACHE[key]
    if k not in have:
        want = [x for x in (GRID_KS + GENERIC_KS if cloud.shape[0] > 2048 else (k,)) if x not in have]
        have.update(model_normals_multi(cloud, tuple(want)))
    return have[k]


def truth(name, cloud, k):
    key = ("truth", name, k)
    if key not in _CACHE:
        _CACHE[key] = truth_normals(cloud, k)
    return _CACHE[key]
