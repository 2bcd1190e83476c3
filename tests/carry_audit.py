"""The bit model of the CARRIED map normals (csrc/hash_grid.hip: carry_normal, grid_scatter_part; csrc/api.hip: map_update_body),
its checks, poses and clouds.  TEST INFRASTRUCTURE: numpy + tests/map_lifecycle.py + tests/normals_audit.py, importable without
a GPU, never imported by the package.  tests/test_carry_audit.py holds it on the CPU, tests/test_gpu_carry_audit.py holds the
library to it through `IcpContext.map_normals_peek()` (`icp_map_normals_peek`: the normal cache as it stands, by original index,
(nx, ny, nz, 1) where the point's flag is 1 and zeros elsewhere — it estimates nothing).

With option "carry_normals" (the default) a pose-only map update rotates the normals the old grid holds into the new frame
instead of clearing them.  What the model states, operation by operation:

  which updates carry   map_update_body: carry_normals, no cloud, nothing evicted, keep > 0, a valid grid, the point-to-plane
                        cost (`carries`).  Every other update clears the cache.
  T                     map_lifecycle.invert4 of the float32 pose (float64 Gauss-Jordan, the source's pivot rule, no fma,
                        rounded to float32); the identity behind a registration that failed (status != ICP_OK).
  the rotation          x = fl(fl(fl(T0 nx) + fl(T1 ny)) + fl(T2 nz)), likewise y (T4 T5 T6) and z (T8 T9 T10); the translation
                        column is not read.
  n2                    fl(fl(fl(x x) + fl(y y)) + fl(z z))
  the branch            fabsf(fl(n2 - 1)) > float32(4e-7) ? rsqrtf(n2) : 1  (a NaN n2 compares false: sc = 1)
  the result            fl(x sc), fl(y sc), fl(z sc)
  the guards            flagged iff the old flag was 1, n2 > 0, sc < inf AND the result is finite and not all zero
  the filing            the row of cell-sorted position i goes to o = bits(old_pts[i].w), 0 <= o < carry_m: by ORIGINAL index
  the scatter           nflag = (w == 1); the rows of points without a carried normal are four zeros

THE ARITHMETIC AS COMPILED.  Read from the gfx950 assembly (hipcc -S, the flags of csrc/Makefile, which include
-ffp-contract=off) of every kernel that inlines carry_normal — k_grid_clear, k_grid_insert2_ride and k_grid_clear_batch;
k_grid_insert2_batch passes no InsertRide and holds no copy of it (its carry runs in k_grid_clear_batch).  All three are the SAME
sequence: nine v_mul_f32 and six v_add_f32 for the rotation in the order above, three v_mul_f32 and two v_add_f32 for n2,
v_add_f32 -1.0, v_cmp_gt_f32 |.| against 0x34d6bf95, three v_mul_f32 for the result — no v_fma / v_fmac anywhere in it.  rsqrtf
is v_rsq_f32 with the denormal guard of the device library around it (n2 < 2^-126 is multiplied by 2^24 first and the result by
2^12: both exact).  The source now says so with __fmul_rn / __fadd_rn, as move_point does; the assembly of the carry shows the
same multiply / add sequence before and after (the guards behind it are new, see below).  So the three paths are one
arithmetic, and `other_contraction` below is what a build WITHOUT -ffp-contract=off would have made of the old plain-C source.

rsqrtf IS NOT CORRECTLY ROUNDED.  HIP's device math table is not shipped with the toolchain here; the ISA's figure for
V_RSQ_F32 is 1 ulp.  The admissible scale factors are therefore the float32 values within RSQ_ULPS = 1 + 1 steps of
float32(1 / sqrt(float64(n2))) — five candidates (the further step also covers the double rounding of that float64
expression).  A renormalised row of the device must be fl(x sc), fl(y sc), fl(z sc) for ONE candidate sc; `check_bits` records
which one matched (the census).  Rows that do not renormalise have no latitude at all.

THE FIX THIS AUDIT MADE.  The source used to flag a row whenever n2 > 0 and sc < inf: a normal whose n2 overflows (2e19 u: n2 =
+inf, rsqrtf = 0) came out as a FLAGGED ZERO normal — against the comment "a zero normal stays unestimated", and a flagged row is
never estimated again: every point-to-plane row built on it is zero.  Under a pose without a zero in its rotation an infinite
component came out as a flagged NaN row the same way (inf * 0).  carry_normal now tests the RESULT; the old rule is the wrong
copy `zero_flagged`.

(C) LENGTH.  Let u = 2^-24.  The float32 n2 of the rotated (x, y, z) is the exact sum of squares times (1 + t), |t| <= (1 + u)^3
- 1 (three rounded products of positive terms, two rounded sums); below 2^-100 the products lose relative accuracy and the row
is left out.  A row that did NOT renormalise has |n2 - 1| <= 4e-7 in float32 (n2 - 1 is exact there), so its exact squared
length is within LENGTH_KEPT = (1 + 4e-7)(1 + 3u + ...) - 1 = 5.8e-7 of 1.  A row that did has sc = (1 + e) / sqrt(n2), |e| <= u
(correct rounding) + RSQ_ULPS * 2u (the steps), every component rounded once more (|d| <= u): its exact squared length is (1 +
e)^2 (1 + t')(1 + d)^2, within LENGTH_RENORMALISED = (1 + 5u)^2 (1 + 3u + ...)(1 + u)^2 - 1 = 8.9e-7 of 1.  `check_length` holds
every flagged row to the bound of its branch.

(D) DIRECTION.  One carry moves the direction of a unit normal off the exact rotation by at most c u radians, to first order:
    T          every entry of the float32 inverse is off the float64 one by <= u |T_ij| (the float64 elimination itself adds
               1e-16): the rotated vector moves by <= u sqrt(sum_i (sum_j |T_ij| |n_j|)^2) <= sqrt(3) u
    products   three per component, each <= u |T_ij n_j|: per component <= u |T_i| |n| <= u, the vector <= sqrt(3) u
    sums       fl(p1 + p2) <= u (|p1| + |p2|) <= u per component, sqrt(3) u for the vector; the second sum <= u |x_i|, the
               vector <= u
    scaling    a common factor turns nothing; the three products with sc round once each: <= u |n|  (zero where sc = 1)
c = 3 sqrt(3) + 2 = 7.196; C_DIRECTION = 7.25 takes in the second-order terms, lengths off 1 by 1e-6 and float32 poses that
are orthogonal to 1e-7 only.  After K carries the angle to (R_K ... R_1)^-1 n0 — the inverses in float64 of the float32 poses —
is at most K C_DIRECTION u: a DERIVED bound.  The model's own drift under the alternating 0.1 degree pose is reported by
tests/test_carry_audit.py as a ratio to it.

Each check raises with its own name in front: "[flag census]", "[carry bits]", "[length]", "[direction]", "[never carried]".
"""
import math

import numpy as np

import map_lifecycle as L
import normals_audit as NA

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
THRESHOLD = F32(4e-7)
RSQ_ULPS = 2                      # the ISA's 1 ulp for V_RSQ_F32 and one further step
RSQ_STEPS = (0, -1, 1, -2, 2)     # the order in which check_bits tries the candidates
N2_MIN = 2.0 ** -100              # below it the length bound does not hold (products near the subnormal range)
_SUMS = 1.0 / (1.0 - ((1.0 + U) ** 3 - 1.0)) - 1.0
LENGTH_KEPT = (1.0 + float(THRESHOLD)) * (1.0 + _SUMS) - 1.0
LENGTH_RENORMALISED = (1.0 + (1 + 2 * RSQ_ULPS) * U) ** 2 * (1.0 + _SUMS) * (1.0 + U) ** 2 - 1.0
C_DIRECTION = 7.25                # 3 sqrt(3) + 2 = 7.196 and the second-order terms (docstring)
assert 3.0 * math.sqrt(3.0) + 2.0 < C_DIRECTION
WRONG = ("pose_not_inverted", "block_transposed", "translation_added", "other_contraction", "always_renormalised",
         "never_renormalised", "threshold_on_norm", "zero_flagged", "filed_by_position", "carried_twice",
         "carried_across_insertion", "carried_under_point_to_point")
SIZES = (1, 2, 11, 63, 64, 65, 255, 256, 257, 1023, 1025, 4097, 8192)
OPTION_SIZES = (257, 8192)
CHAIN_M, CHAIN_STEPS, CHAIN_MARKS = 600, 1000, (10, 40, 200, 1000)
FAR = (10000.0, -10000.0, 50.0)


# ---- poses and clouds ------------------------------------------------------------------------------------------------------
def pose(yaw=0.0, pitch=0.0, translation=(0.0, 0.0, 0.0)):
    """float32 4x4 of [tx, ty, tz, 0, pitch, yaw] (radians), as the oracle's build_pose_matrix forms it in float32"""
    return L.A.O.build_pose_matrix(np.array([*translation, 0.0, pitch, yaw], F32)).astype(F32)


def poses():
    """{name: float32 pose}: identity, the 0.1 degree yaw + 0.033 degree pitch of straight driving, the synthetic drive's 0.57
    degrees, yaw 3 rad, pitch pi / 2 — and each with a (10 km, -10 km, 50 m) translation"""
    base = {"identity": (0.0, 0.0), "small": (math.radians(0.1), math.radians(0.033)), "drive": (math.radians(0.57), 0.0),
            "yaw_3rad": (3.0, 0.0), "pitch_half_pi": (0.0, float(F32(np.pi / 2)))}
    out = {}
    for name, (yaw, pitch) in base.items():
        out[name] = pose(yaw, pitch)
        out[name + "+far"] = pose(yaw, pitch, FAR)
    return out


def cloud(kind, m):
    """the first m points of the 8 192-point LiDAR map / of the lattice of tests/normals_audit.py"""
    c = NA.lidar() if kind == "lidar" else NA.clouds()["lattice"]
    assert m <= len(c), (kind, m)
    return np.ascontiguousarray(c[:m], F32)


def scans():
    """six 16 x 512 scans of the scene the LiDAR map was merged from (the map is expressed in the frame of scans()[3])"""
    if "scans" not in _EST:
        from pylidar_slam_amd.synthetic import SceneConfig, make_sequence
        _EST["scans"] = [np.ascontiguousarray(s, F32) for s in make_sequence(SceneConfig(height=16, width=512), 6)[0]]
    return _EST["scans"]


CHAIN_FIRST = 4000


def chain_cloud():
    """the CHAIN_M points of the LiDAR map from CHAIN_FIRST on: the cut on which both branches of the carry occur at every step
    of the chain from the second on (tests/test_carry_audit.py: condition (ii), and what other cuts give)"""
    return np.ascontiguousarray(NA.lidar()[CHAIN_FIRST:CHAIN_FIRST + CHAIN_M], F32)


def chain_poses(steps):
    """the 0.1 degree pose and its transpose in alternation"""
    small = poses()["small"]
    back = np.ascontiguousarray(small.T)
    return [small if i % 2 == 0 else back for i in range(steps)]


_EST = {}


def estimated4(points, k=10):
    """[M,4]: normals_audit.model_normals of every point of the cloud, flagged — what a search of every map point leaves in the
    cache of a map without duplicates (computed once per cloud)"""
    key = (np.ascontiguousarray(points, F32).tobytes(), int(k))
    if key not in _EST:
        want = NA.model_normals(points, int(k))
        out = np.ones((len(points), 4), F32)
        out[:, :3] = want.normals
        out.setflags(write=False)
        _EST[key] = (out, want)
    return _EST[key][0]


def estimated_model(points, k=10):
    estimated4(points, k)
    return _EST[(np.ascontiguousarray(points, F32).tobytes(), int(k))][1]


def planted_rows():
    """(names, [P,4] rows for map_normals_install): lengths 1 +- j 2^-24 (j = 0 .. 8) along a skew unit direction, the exact
    axes, a zero row, a row whose n2 underflows to 0, 1e-20 u (subnormal n2), 1e19 u, 2e19 u (n2 = +inf), one with a NaN and
    one with an infinite component"""
    d = np.array([0.36, 0.48, 0.8], F64)
    names, rows = [], []
    for j in range(-8, 9):
        names.append(f"length 1{j:+d} ulp")
        rows.append(d * (1.0 + j * U))
    for a in range(3):
        for s in (1.0, -1.0):
            names.append(f"axis {'+' if s > 0 else '-'}{'xyz'[a]}")
            rows.append(s * np.eye(3)[a])
    for name, v in (("zero", d * 0.0), ("n2 underflows", d * 1e-30), ("subnormal n2", d * 1e-20), ("1e19 u", d * 1e19),
                    ("2e19 u: n2 overflows", d * 2e19), ("NaN component", np.array([0.6, np.nan, 0.8])),
                    ("infinite component", np.array([0.6, np.inf, 0.8]))):
        names.append(name)
        rows.append(v)
    out = np.ones((len(rows), 4), F32)
    with np.errstate(over="ignore"):
        out[:, :3] = np.asarray(rows, F64).astype(F32)
    return names, out


# ---- the arithmetic --------------------------------------------------------------------------------------------------------
def transform_of(rel32, ok=True, wrong=None):
    """T of map_move_prepare: invert4 of the float32 pose; the identity behind a failed registration"""
    if not ok:
        return np.eye(4, dtype=F32)
    rel32 = np.asarray(rel32, F32).reshape(4, 4)
    if wrong == "pose_not_inverted":
        return rel32.copy()
    T = L.invert4(rel32)
    assert T is not None, "singular pose"
    if wrong == "block_transposed":
        T = T.copy()
        T[:3, :3] = T[:3, :3].T.copy()
    return T


def _fma(a, b, c):
    """fmaf emulated through float64: the product of two float32 is exact there (the second rounding is the wrong copy's)"""
    return (np.asarray(a, F64) * np.asarray(b, F64) + np.asarray(c, F64)).astype(F32)


def rotate(T, n3, wrong=None):
    T = np.asarray(T, F32).reshape(4, 4)
    n3 = np.asarray(n3, F32)
    nx, ny, nz = n3[:, 0], n3[:, 1], n3[:, 2]
    out = []
    with np.errstate(all="ignore"):
        for i in range(3):
            if wrong == "other_contraction":
                v = _fma(T[i, 2], nz, _fma(T[i, 1], ny, T[i, 0] * nx))
            else:
                v = (T[i, 0] * nx + T[i, 1] * ny) + T[i, 2] * nz
            if wrong == "translation_added":
                v = v + T[i, 3]
            out.append(np.asarray(v, F32))
    return out


def squared_length(x, y, z, wrong=None):
    with np.errstate(all="ignore"):
        if wrong == "other_contraction":
            return _fma(z, z, _fma(y, y, x * x))
        return np.asarray((x * x + y * y) + z * z, F32)


def renormalises(n2, wrong=None):
    with np.errstate(all="ignore"):
        if wrong == "always_renormalised":
            return np.ones(n2.shape, bool)
        if wrong == "never_renormalised":
            return np.zeros(n2.shape, bool)
        if wrong == "threshold_on_norm":
            return np.abs(np.sqrt(n2) - F32(1.0)) > THRESHOLD
        return np.abs(n2 - F32(1.0)) > THRESHOLD


def rsqrt_candidate(n2, step=0):
    """float32(1 / sqrt(float64(n2))) moved by `step` float32 values (0 and inf stay: rsqrtf(inf) = 0, rsqrtf(0) = inf)"""
    with np.errstate(all="ignore"):
        r = (1.0 / np.sqrt(np.asarray(n2, F64))).astype(F32)
        movable = np.isfinite(r) & (r > 0)
        to = F32(np.inf) if step > 0 else F32(0.0)
        for _ in range(abs(step)):
            r = np.where(movable, np.nextafter(r, to), r).astype(F32)
    return r


def carry_rows(T, before4, step=0, wrong=None):
    """carry_normal over [M,4] rows by original index: (the rows behind the carry, which flagged rows renormalised)"""
    b = np.asarray(before4, F32).reshape(-1, 4)
    flagged = b[:, 3] == 1
    x, y, z = rotate(T, b[:, :3], wrong)
    n2 = squared_length(x, y, z, wrong)
    ren = renormalises(n2, wrong)
    with np.errstate(all="ignore"):
        sc = np.where(ren, rsqrt_candidate(n2, step), F32(1.0)).astype(F32)
        o = np.stack((x * sc, y * sc, z * sc), axis=1).astype(F32)
        ok = flagged & (n2 > 0) & (sc < np.inf)
        if wrong != "zero_flagged":
            ok &= (o != 0).any(axis=1) & (np.abs(o) < np.inf).all(axis=1)
    out = np.zeros_like(b)
    out[ok, :3] = o[ok]
    out[ok, 3] = 1.0
    return out, ren & flagged


def carries(carry_normals=1, has_cloud=False, evicted=0, keep=1, grid_valid=True, cost="point_to_plane", wrong=None):
    """whether map_update_body carries the normals over this update"""
    return bool(carry_normals and (not has_cloud or wrong == "carried_across_insertion") and evicted == 0 and keep > 0 and
                grid_valid and (cost == "point_to_plane" or wrong == "carried_under_point_to_point"))


def update(before4, rel32, ok=True, step=0, wrong=None, orig_of_pos=None, inserted=0, evicted=0, **rule):
    """The normal cache [M',4] behind one map update (M' = M - evicted + inserted).  `orig_of_pos`: the original index at every
    cell-sorted position of the old grid (only the wrong copy `filed_by_position` reads it).  `rule`: carries()' arguments."""
    b = np.asarray(before4, F32).reshape(-1, 4)
    keep = len(b) - evicted
    out = np.zeros((keep + inserted, 4), F32)
    has_cloud = bool(rule.pop("has_cloud", False)) or inserted > 0  # (a cloud of zero rows is a cloud)
    if not carries(has_cloud=has_cloud, evicted=evicted, keep=keep, wrong=wrong, **rule):
        return out
    T = transform_of(rel32, ok, wrong)
    rows, _ = carry_rows(T, b[evicted:], step, wrong)
    if wrong == "carried_twice":
        rows, _ = carry_rows(T, rows, step, wrong)
    if wrong == "filed_by_position":
        rows = rows[np.asarray(orig_of_pos)]  # (carry[i] instead of carry[o]: point o receives what position o held)
    out[:keep] = rows
    return out


def free_run(n0_4, rels, step=0, wrong=None, marks=()):
    """the model applied along a chain of poses; returns ({mark: rows after `mark` updates}, renormalised share per update)"""
    rows, share, at = np.asarray(n0_4, F32).copy(), [], {}
    for k, rel in enumerate(rels, 1):
        T = transform_of(rel, wrong=wrong)
        rows, ren = carry_rows(T, rows, step, wrong)
        share.append(float(ren.sum()) / max(1, int((rows[:, 3] == 1).sum())))
        if k in marks:
            at[k] = rows.copy()
    return at, share


# ---- the checks ------------------------------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _candidates(before4, T):
    return {s: carry_rows(T, before4, s) for s in RSQ_STEPS}


def check_flags(tag, before4, after4, T):
    """(A) flagged after <=> flagged before and a finite non-zero result; every unflagged row four zeros, w is 0 or 1.  Returns
    (flagged before, flagged after)."""
    b, a = np.asarray(before4, F32).reshape(-1, 4), np.asarray(after4, F32).reshape(-1, 4)
    assert a.shape == b.shape, f"[flag census] {tag}: {a.shape} rows behind {b.shape}"
    w = _bits(a[:, 3])
    assert np.isin(w, _bits(np.array([0.0, 1.0], F32))).all(), f"[flag census] {tag}: a flag column that is neither 0 nor 1"
    got = a[:, 3] == 1
    cands = _candidates(b, T)
    may = np.any([c[:, 3] == 1 for c, _ in cands.values()], axis=0)
    must = np.all([c[:, 3] == 1 for c, _ in cands.values()], axis=0)
    appeared, lost = got & ~may, must & ~got
    assert not appeared.any(), \
        (f"[flag census] {tag}: {appeared.sum()} rows are flagged that the model leaves unestimated, the first row "
         f"{int(np.flatnonzero(appeared)[0])}: {a[np.flatnonzero(appeared)[0]]!r} from {b[np.flatnonzero(appeared)[0]]!r}")
    assert not lost.any(), \
        (f"[flag census] {tag}: {lost.sum()} of {must.sum()} normals the model carries are gone, the first row "
         f"{int(np.flatnonzero(lost)[0])}: from {b[np.flatnonzero(lost)[0]]!r}")
    dirty = ~got & _bits(a).any(axis=1)
    assert not dirty.any(), f"[flag census] {tag}: {dirty.sum()} unflagged rows are not zeros, the first {a[np.flatnonzero(dirty)[0]]!r}"
    return int((b[:, 3] == 1).sum()), int(got.sum())


def check_bits(tag, before4, after4, T):
    """(B) every flagged row behind the carry from the rows before it: bit-equal to the model for one rsqrtf candidate (rows
    that do not renormalise: no latitude).  Returns (census {step: rows matched} over the renormalised rows, renormalised rows,
    flagged rows)."""
    b, a = np.asarray(before4, F32).reshape(-1, 4), np.asarray(after4, F32).reshape(-1, 4)
    assert a.shape == b.shape, f"[carry bits] {tag}: {a.shape} rows behind {b.shape}"
    cands = _candidates(b, T)
    ren = cands[0][1]
    matched = np.zeros(len(a), bool)
    census = {}
    for s in RSQ_STEPS:
        same = ~matched & ~(_bits(a) != _bits(cands[s][0])).any(axis=1)
        census[s] = int((same & ren).sum())
        matched |= same
    if not matched.all():
        r = int(np.flatnonzero(~matched)[0])
        raise AssertionError(
            f"[carry bits] {tag}: {(~matched).sum()} of {len(a)} rows are not the model's for any rsqrtf candidate, the first row "
            f"{r} ({'renormalised' if ren[r] else 'kept'}): {a[r]!r} ({_bits(a[r])}) against {cands[0][0][r]!r} "
            f"({_bits(cands[0][0][r])}) from {b[r]!r}")
    return census, int(ren.sum()), int((a[:, 3] == 1).sum())


def check_length(tag, after4, renormalised=None):
    """(C) | |n|^2 - 1 | in float64 of every flagged row inside the bound of its branch (`renormalised`: which rows took the
    rsqrtf branch; None: the larger bound for all).  Returns the worst ratio to the bound."""
    a = np.asarray(after4, F32).reshape(-1, 4)
    use = a[:, 3] == 1
    if not use.any():
        return 0.0
    n2 = (a[:, :3].astype(F64) ** 2).sum(axis=1)
    bound = np.full(len(a), max(LENGTH_KEPT, LENGTH_RENORMALISED))
    if renormalised is not None:
        bound = np.where(renormalised, LENGTH_RENORMALISED, LENGTH_KEPT)
    with np.errstate(invalid="ignore"):
        ratio = np.where(use, np.abs(n2 - 1.0) / bound, 0.0)
    bad = use & ~(ratio <= 1.0)
    assert not bad.any(), \
        (f"[length] {tag}: {bad.sum()} of {use.sum()} carried normals are off unit length by more than the branch rule allows, "
         f"the worst |n|^2 - 1 = {np.nanmax(np.abs(n2[use] - 1.0)):.3e} (bounds {LENGTH_KEPT:.3e} kept, "
         f"{LENGTH_RENORMALISED:.3e} renormalised)")
    return float(ratio.max())


def check_step(tag, before4, after4, T):
    """(A), (B) and (C) of one carry from the rows before it.  Returns a dict of figures."""
    fb, fa = check_flags(tag, before4, after4, T)
    census, ren, flagged = check_bits(tag, before4, after4, T)
    a = np.asarray(after4, F32).reshape(-1, 4)
    x, y, z = rotate(T, np.asarray(before4, F32).reshape(-1, 4)[:, :3])
    with np.errstate(all="ignore"):
        in_range = squared_length(x, y, z).astype(F64) >= N2_MIN
    masked = a.copy()
    masked[~in_range] = 0.0
    length = check_length(tag, masked, _candidates(before4, T)[0][1])
    return dict(before=fb, after=fa, census=census, renormalised=ren, flagged=flagged, length_ratio=length)


def exact_rotation(rels):
    """(R_K ... R_1)^-1 = R_K^-1 ... applied in order: the product of the float64 inverses of the float32 poses, 3x3"""
    m = np.eye(3)
    for rel in rels:
        m = np.linalg.inv(np.asarray(rel, F32).reshape(4, 4).astype(F64))[:3, :3] @ m
    return m


def check_direction(tag, n0_4, nk_4, rels):
    """(D) the angle between every flagged row after the K = len(rels) carries and the exact rotation of the row it started
    from: at most K C_DIRECTION 2^-24.  Returns (worst angle, worst ratio to the bound)."""
    a, b = np.asarray(nk_4, F32).reshape(-1, 4), np.asarray(n0_4, F32).reshape(-1, 4)
    use = (a[:, 3] == 1) & (b[:, 3] == 1)
    if not use.any():
        return 0.0, 0.0
    want = b[use, :3].astype(F64) @ exact_rotation(rels).T
    got = a[use, :3].astype(F64)
    cr = np.linalg.norm(np.cross(got, want), axis=1)
    angle = np.arctan2(cr, (got * want).sum(axis=1))
    bound = len(rels) * C_DIRECTION * U
    worst = float(angle.max())
    assert worst <= bound, \
        (f"[direction] {tag}: after {len(rels)} carries a normal is {worst:.3e} rad off the exact rotation of where it started, "
         f"the derived bound is {bound:.3e} ({(angle > bound).sum()} of {use.sum()} rows beyond it)")
    return worst, worst / bound


def check_estimated(tag, after4, map_points, k=10, rows=None):
    """every row (of `rows`) flagged and bit-equal to normals_audit.model_normals on `map_points` — the cache behind an eager
    estimation of the whole map.  Returns the number of rows compared."""
    a = np.asarray(after4, F32).reshape(-1, 4)
    sel = np.arange(len(a)) if rows is None else np.asarray(rows)
    assert (a[sel, 3] == 1).all(), f"[flag census] {tag}: {(a[sel, 3] != 1).sum()} of {len(sel)} rows are not estimated"
    want = NA.model_normals(np.ascontiguousarray(map_points, F32), int(k), rows=sel)
    NA.check_caps(want, tag)
    return NA.check_bits(np.ascontiguousarray(a[:, :3]), want, what=f"[normal bits] {tag}")


def check_never_carried(tag, before4, after4, T, map_points=None, k=10):
    """Behind an update that must not carry: every row is zeros, or (flagged) the estimator's bits on `map_points` — and no
    flagged row is the rotation of an old normal.  Returns the number of flagged rows."""
    a = np.asarray(after4, F32).reshape(-1, 4)
    got = np.flatnonzero(a[:, 3] == 1)
    dirty = (a[:, 3] != 1) & _bits(a).any(axis=1)
    assert not dirty.any(), f"[never carried] {tag}: {dirty.sum()} unflagged rows are not zeros"
    if got.size and map_points is None:
        raise AssertionError(f"[never carried] {tag}: {got.size} of {len(a)} normals are there behind an update that clears them, "
                             f"the first row {int(got[0])}: {a[got[0]]!r}")
    if got.size:
        b = np.asarray(before4, F32).reshape(-1, 4)
        n = min(len(a), len(b))
        rot, _ = carry_rows(T, b[:n])
        same = (rot[:, 3] == 1) & (a[:n, 3] == 1) & ~(_bits(a[:n]) != _bits(rot)).any(axis=1)
        est = estimated_or_none(map_points, k, got)
        fresh = np.zeros(len(a), bool)
        fresh[got] = ~(_bits(a[got, :3]) != _bits(est)).any(axis=1)
        stale = same[:n] & ~fresh[:n]
        assert not stale.any(), f"[never carried] {tag}: {stale.sum()} rows are the rotated old normals, the first row {int(np.flatnonzero(stale)[0])}"
        check_estimated(tag, a, map_points, k, rows=got)
    return int(got.size)


def estimated_or_none(map_points, k, rows):
    return NA.model_normals(np.ascontiguousarray(map_points, F32), int(k), rows=np.asarray(rows)).normals


def old_bar_passes(moved_map, normals3, k=10):
    """whether tests/iteration_audit.check_normals — the only bar carried normals were held to — passes these normals on the map
    as moved; returns (passes, min |dot|)"""
    from types import SimpleNamespace
    nref = L.A.NormalReference(moved_map, k)
    fails, fig = L.A.check_normals(SimpleNamespace(k="old bar", ix=np.arange(len(moved_map))), normals3, nref)
    return not fails, fig["min_dot"]
