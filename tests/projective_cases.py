"""Inputs and per-pixel accounting for the projective local map tests (tests/test_projective_cases.py on the CPU,
tests/test_gpu_projective_edges.py on the device).  TEST INFRASTRUCTURE: plain numpy + oracle/icp_oracle.py, importable
without a GPU, never imported by the package.

The accounting helpers take the OUTPUT of the code under test (a normal map, a model, association rows) as plain arrays,
so the CPU suite can hand them the oracle's own output — and deliberately wrong copies of it — and see what they report.
Every pixel is classified from the oracle's values, never from the output under test.
"""
import os

import numpy as np

import icp_oracle as O

F32, F64 = np.float32, np.float64
UP_FOV, DOWN_FOV = 3.0, -24.0
EPS64 = float(np.finfo(F64).eps)
ULP32 = float(np.finfo(F32).eps)  # spacing of float32 at 1.0
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ----------------------------------------------------------------------------------------------------------------------
# inputs
# ----------------------------------------------------------------------------------------------------------------------
def scan_vmap(h, w, seed=4242, frame=0, step=0.4, yaw_rate=0.01):
    """[3,H,W] vertex map of frame `frame` of a seeded synthetic drive, through the oracle's projection."""
    from pylidar_slam_amd.synthetic import SceneConfig, make_sequence
    scans, _ = make_sequence(SceneConfig(height=h, width=w, seed=seed, step=step, yaw_rate=yaw_rate), frame + 1)
    return O.build_projection_map(scans[frame], h, w, UP_FOV, DOWN_FOV)


def golden_vmap(frame=0):
    return np.load(os.path.join(GOLDEN, "projective.npz"))["vmaps"][frame].copy()


def damage(vmap, content, seed=7):
    """A copy of `vmap` damaged on purpose.  `content`:
    dense | holes (every sixth row, columns 0, W/3 and W-1, a rectangle, a top band: what a real sensor's FoV and dropouts
    leave) | mild (one null row, one null column) | salt50 (keep 50 %) | far10 (coordinates x 3, keep 10 %) | null |
    single (one non-null pixel) | corners (one non-null pixel in each corner)."""
    v = np.array(vmap, dtype=F32, copy=True)
    _, h, w = v.shape
    rng = np.random.default_rng(seed)
    if content == "dense":
        return v
    if content == "holes":
        v[:, 4::6, :] = 0.0
        v[:, :, [0, w // 3, w - 1]] = 0.0
        v[:, h // 2:h // 2 + max(1, h // 8), w // 2:w // 2 + max(1, w // 8)] = 0.0
        v[:, :max(1, h // 16), :] = 0.0
        return v
    if content == "mild":
        if h > 2:
            v[:, h // 2, :] = 0.0
        v[:, :, w // 2] = 0.0
        return v
    if content == "salt50":
        v[:, rng.random((h, w)) >= 0.5] = 0.0
        return v
    if content == "far10":
        v *= F32(3.0)
        v[:, rng.random((h, w)) >= 0.1] = 0.0
        return v
    keep = np.zeros((h, w), bool)
    if content == "single":
        keep[h // 2, w // 3] = True
    elif content == "corners":
        keep[[0, 0, h - 1, h - 1], [0, w - 1, 0, w - 1]] = True
    elif content != "null":
        raise AssertionError(f"unknown content {content}")
    if content != "null" and not (np.abs(v).max(axis=0) > 0)[keep].all():  # (the kept pixels must hold a point)
        v[:, keep] = np.array([[4.0], [1.0], [-0.5]], F32)
    v[:, ~keep] = 0.0
    return v


# (name, H, W, content, kernel size, accounted).  `accounted`: the undetermined pixels are capped at 1 % of the non-null
# ones and every other pixel is held to its derived tolerance.  The others are the cases whose whole point is rank
# deficiency — kernel size 1 (one point per window), single / corner pixels, the sparse far map, the all-null map, and the
# one-row image at kernel sizes 3 and 5 (every window a short, nearly collinear run of points: a third of them has a
# condition number that puts the tolerance above 1e-4) — and assert only the null / zero-or-unit / finite rules.
NORMAL_CASES = (
    [("golden", 32, 256, "dense", ks, ks > 1) for ks in (1, 3, 5, 7, 15)]
    + [("golden", 32, 256, "holes", ks, True) for ks in (3, 5, 7, 15)]
    + [("golden", 32, 256, "salt50", 7, True)]
    + [("scan", 64, 1024, "dense", 5, True), ("scan", 64, 1024, "holes", 3, True), ("scan", 64, 1024, "holes", 7, True),
       ("scan", 64, 1024, "salt50", 5, True), ("scan", 64, 1024, "salt50", 1, False),
       ("scan", 64, 1024, "far10", 5, False)]
    + [("scan", 17, 33, "mild", 3, True), ("scan", 17, 33, "holes", 5, True), ("scan", 17, 33, "dense", 15, True),
       ("scan", 5, 7, "dense", 3, True), ("scan", 5, 7, "mild", 7, True), ("scan", 5, 7, "dense", 15, True),
       ("scan", 1, 300, "dense", 3, False), ("scan", 1, 300, "mild", 5, False), ("scan", 1, 300, "dense", 15, True),
       ("scan", 3, 3, "dense", 3, True), ("scan", 3, 3, "dense", 5, True), ("scan", 3, 3, "dense", 15, True)]
    + [("golden", 32, 256, c, 5, False) for c in ("null", "single", "corners")]
    + [("scan", 17, 33, c, 3, False) for c in ("null", "single", "corners")]
)


def normal_case_input(source, h, w, content):
    base = golden_vmap(0) if source == "golden" else scan_vmap(h, w)
    assert base.shape == (3, h, w)
    return damage(base, content)


def case_id(case):
    return "-".join(str(x) for x in case[:5])


# ----------------------------------------------------------------------------------------------------------------------
# A. normal maps
# ----------------------------------------------------------------------------------------------------------------------
# tolerance on sin(angle) of a determined pixel: 2 float32 ulp (the kernel rounds a float64 unit vector to float32 once:
# <= 0.5 ulp per component, sqrt(3) / 2 ulp on the vector; 2 ulp with margin for the comparison's own arithmetic) plus
# C_SOLVE * eps64 * cond(A) for the float64 3x3 solve.  C_SOLVE = 4 x the largest spread, in units of eps64 * cond(A),
# between two float64 formulations of the oracle over every accounted case of NORMAL_CASES: the adjugate as written
# (O.compute_normal_map) and np.linalg.solve.  Measured (tests/test_projective_cases.py::test_solve_spread_backs_the_
# tolerance re-measures and asserts it): largest spread 3012 eps64 cond(A) (the 64 x 1024 map with holes at kernel size 3;
# the adjugate is not backward stable, its error grows like cond(A)^2) -> 4 x -> C_SOLVE = 12048.
C_SOLVE = 12048.0
NORMAL_TOL_CAP = 1.0e-4  # a pixel whose derived tolerance exceeds the existing `max < 1e-4` bar is "undetermined"
DET_THRESHOLD = 1.0e-6  # geometry.py:272-273


def window_sums(vmap, ks):
    """float64 window sums of the oracle: S [H,W,3], A [H,W,3,3] and the number of non-null points per window.
    (The kernel adds the same float64 products in the same order — rows, then columns of the window — so A and S are
    also what it holds, bit for bit; the classification below does not rely on that.)"""
    v = np.asarray(vmap, dtype=F64)
    _, h, w = v.shape
    cov = (v[None] * v[:, None]).reshape(9, h, w)
    s = O._box_sum(v, ks)
    a = O._box_sum(cov, ks).reshape(3, 3, h, w)
    cnt = O._box_sum((np.abs(v).max(axis=0) > 0)[None].astype(F64), ks)[0]
    return np.moveaxis(s, 0, 2), np.moveaxis(a, (0, 1), (2, 3)), cnt


def solve_normals(S, A, ok):
    """The second float64 formulation: np.linalg.solve(A, S), normalised; zero where `ok` is False."""
    n = np.zeros_like(S)
    sol = np.linalg.solve(A[ok], S[ok][..., None])[..., 0]
    nrm = np.linalg.norm(sol, axis=-1, keepdims=True)
    n[ok] = sol / np.where(nrm > 0, nrm, 1.0)
    return n


class NormalReference:
    """The oracle's float64 normal map of `vmap` at kernel size `ks` and the class of every pixel:
    null | determined (with `tol`, the bound on sin(angle), and `expect_zero`) | undetermined."""

    def __init__(self, vmap, ks):
        self.vmap, self.ks = np.asarray(vmap, F32), ks
        S, A, cnt = window_sums(vmap, ks)
        self.exact = O.compute_normal_map(vmap, ks, dtype=F64)  # [3,H,W] float64
        self.null = np.abs(self.vmap).max(axis=0) == 0
        tr = np.trace(A, axis1=-2, axis2=-1)
        det = np.linalg.det(A)
        # |det computed by ANY float64 formulation of six triple products - det of A| <= 16 eps (tr A)^3: the entries of
        # the positive semi-definite A are bounded by tr A, the six products by (tr A)^3 / 27 each, a handful of roundings
        self.det_bound = 16.0 * EPS64 * tr ** 3
        few = cnt < 3  # exact determinant 0: whatever a float64 formulation returns is rounding noise
        straddles = np.abs(np.abs(det) - DET_THRESHOLD) <= self.det_bound
        self.expect_zero = ~few & ~straddles & (np.abs(det) <= DET_THRESHOLD)
        solvable = ~few & ~straddles & ~self.expect_zero & ~self.null
        self.cond = np.full(det.shape, np.inf)
        self.cond[solvable] = np.linalg.cond(A[solvable])
        self.tol = 2.0 * ULP32 + C_SOLVE * EPS64 * self.cond
        loose = solvable & (self.tol > NORMAL_TOL_CAP)
        self.undetermined = ~self.null & (few | straddles | loose)
        self.determined = ~self.null & ~self.undetermined
        self.S, self.A = S, A
        self.why = dict(few=int((few & ~self.null).sum()), straddles=int((straddles & ~few & ~self.null).sum()),
                        loose=int(loose.sum()))

    def spread(self):
        """max over the determined non-zero pixels of sin(angle between the two float64 formulations) / (eps64 cond(A))."""
        ok = self.determined & ~self.expect_zero
        if not ok.any():
            return 0.0
        alt = solve_normals(self.S, self.A, ok)
        ex = np.moveaxis(self.exact, 0, 2)
        s = np.linalg.norm(np.cross(alt[ok], ex[ok]), axis=-1)
        return float((s / (EPS64 * self.cond[ok])).max())

    def account(self, nmap):
        """Holds a normal map [3,H,W] float32 to the rules; returns the counts and the unexplained pixels [[row, col]]."""
        n = np.asarray(nmap)
        assert n.shape == self.exact.shape
        n64 = n.astype(F64)
        length = np.linalg.norm(n64, axis=0)
        zero = np.abs(n).max(axis=0) == 0
        finite = np.isfinite(n).all(axis=0)
        bad = ~finite
        bad |= self.null & ~zero
        unit = np.abs(length - 1.0) <= 1.0e-6
        bad |= self.undetermined & ~(zero | unit)
        ex_zero = np.abs(self.exact).max(axis=0) == 0
        sin = np.linalg.norm(np.cross(n64, self.exact, axis=0), axis=0)
        det_nz = self.determined & ~self.expect_zero
        bad |= self.determined & (zero != ex_zero)
        bad |= det_nz & ~zero & ~unit
        with np.errstate(invalid="ignore"):
            bad |= det_nz & ~(sin <= self.tol)
        worst = float(sin[det_nz & finite].max()) if (det_nz & finite).any() else 0.0
        at = np.unravel_index(np.argmax(np.where(det_nz & finite, sin, -1.0)), sin.shape)
        return dict(null=int(self.null.sum()), determined=int(self.determined.sum()),
                    undetermined=int(self.undetermined.sum()), non_null=int((~self.null).sum()),
                    noise_normals=int((self.undetermined & ~zero).sum()), worst_sin=worst, worst_tol=float(self.tol[at]),
                    unexplained=np.argwhere(bad))


# ----------------------------------------------------------------------------------------------------------------------
# float32 arithmetic of the kernels, restated
# ----------------------------------------------------------------------------------------------------------------------
def fma32(a, b, c):
    """fmaf(a, b, c) on float32 arrays: the product of two float32 is exact in float64; the sum is rounded to odd at 53
    bits (Boldo & Melquiond 2008) and then once to float32 — the correctly rounded a * b + c."""
    p = np.asarray(a, F32).astype(F64) * np.asarray(b, F32).astype(F64)
    c = np.broadcast_to(np.asarray(c, F32).astype(F64), p.shape)
    s = np.asarray(p + c)
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    even = (s.view(np.int64) & 1) == 0
    s = np.where((e != 0.0) & even, np.nextafter(s, np.where(e > 0.0, np.inf, -np.inf)), s)
    return s.astype(F32)


def transform_fma(points, pose, translate=True):
    """p' = fma(z, T2, fma(y, T1, x * T0)) + T3 per row of T (pm_project_body / pm_resolve_body / pm_iterate_body in
    projective.hip); `translate` False: the rotation alone (the model normals)."""
    p = np.asarray(points, F32).reshape(-1, 3)
    t = np.asarray(pose, F32).reshape(4, 4)
    out = np.empty_like(p)
    for k in range(3):
        acc = (p[:, 0].astype(F64) * F64(t[k, 0])).astype(F32)
        acc = fma32(p[:, 1], t[k, 1], acc)
        acc = fma32(p[:, 2], t[k, 2], acc)
        out[:, k] = acc + t[k, 3] if translate else acc
    return out


def range32(p):
    """sqrtf((x * x + y * y) + z * z), every operation rounded to float32 (pixel_of, k_project)."""
    p = np.asarray(p, F32)
    return np.sqrt((p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2])


def invert4(m):
    """`invert4` of csrc/map_move_device.h (host build): Gauss-Jordan with partial pivoting in float64, no fused
    operations, the result rounded to float32."""
    a = [[float(m[r][c]) for c in range(4)] + [1.0 if r == c else 0.0 for c in range(4)] for r in range(4)]
    for c in range(4):
        piv = c
        for r in range(c + 1, 4):
            if abs(a[r][c]) > abs(a[piv][c]):
                piv = r
        assert a[piv][c] != 0.0
        a[c], a[piv] = a[piv], a[c]
        inv = 1.0 / a[c][c]
        a[c] = [x * inv for x in a[c]]
        for r in range(4):
            if r != c:
                f = a[r][c]
                a[r] = [x - f * y for x, y in zip(a[r], a[c])]
    return np.array([row[4:] for row in a], F64).astype(F32)


class LibraryWindowOracle(O.ProjectiveLocalMapOracle):
    """`ProjectiveLocalMapOracle` whose window poses are composed as the library composes them, so that both sides
    transform by bit-identical poses.  Mirrors `pmap_window_step` of csrc/api.hip: the first map takes the relative pose
    as it is; afterwards `inv = invert4(rel_pose)` (float64 Gauss-Jordan rounded to float32), every kept pose becomes
    sum_k (double) inv[r][k] * (double) pose[k][c], k ascending from 0.0, rounded once to float32; a new map enters with
    the identity; the oldest leaves beyond local_map_size.  (The stock oracle multiplies np.linalg.inv(rel_pose) in
    float32.)  `nmap_of`: the normal map to store with a vertex map — the device's own for the bit-exact normal check."""

    def __init__(self, *args, nmap_of=None, **kwargs):
        self.nmap_of = nmap_of
        super().__init__(*args, **kwargs)

    def update(self, rel_pose, new_vertex_map=None):
        rel_pose = np.asarray(rel_pose, dtype=F32).reshape(4, 4)
        if new_vertex_map is not None:
            v = np.asarray(new_vertex_map, dtype=F32).reshape(3, self.h, self.w)
            nm = (self.nmap_of(v) if self.nmap_of is not None else
                  O.compute_normal_map(v, self.ks, self.normals_dtype)).astype(F32)
            mask = np.abs(v).max(axis=0) > 0
        if not self.vmaps:
            self.vmaps, self.nmaps, self.masks, self.poses = [v], [nm], [mask], [rel_pose.copy()]
        else:
            inv = invert4(rel_pose).astype(F64)
            moved = []
            for p in self.poses:
                p = p.astype(F64)
                acc = np.zeros((4, 4))
                for k in range(4):
                    acc = acc + inv[:, k:k + 1] * p[k:k + 1, :]
                moved.append(acc.astype(F32))
            self.poses = moved
            if new_vertex_map is not None:
                self.poses.append(np.eye(4, dtype=F32))
                self.vmaps.append(v)
                self.nmaps.append(nm)
                self.masks.append(mask)
            if len(self.poses) > self.size:
                self.vmaps, self.nmaps, self.masks, self.poses = self.vmaps[1:], self.nmaps[1:], self.masks[1:], \
                    self.poses[1:]
        self.build_model()


def pose_drift_bound(updates, scale):
    """Bound on |library pose - stock oracle pose| per entry after `updates` window steps: each step rounds the inverse
    and the product to float32 on either side (2 x 2 roundings of entries no larger than `scale`, the largest entry of the
    window's poses) and carries the previous difference through a rotation: 4 ulp(scale) per update."""
    return 4.0 * float(np.spacing(F32(scale))) * max(1, updates)


# ----------------------------------------------------------------------------------------------------------------------
# C. window and model
# ----------------------------------------------------------------------------------------------------------------------
def toss_band(h, w):
    """The coin-toss band of tests/test_gpu_parity.py::test_projection: 4 ulp of the largest coordinate, and no tighter than
    1.5 x what the reference's own code paths differ by (tests/golden/projection_spread.npz)."""
    spread = np.load(os.path.join(GOLDEN, "projection_spread.npz"))
    own = max(float(spread[k]) for k in spread.files if k.endswith("max_pixel_difference"))
    return max(4 * float(np.spacing(F32(max(h, w)))), 1.5 * own)


def transform_tolerance(points, pose):
    """Per point, the bound on |fma chain - O.apply_transformation| per coordinate: either side makes at most four float32
    roundings (three products / fused steps and the translation) of partial sums no larger than M = |x| + |y| + |z| + max|t|
    (|R_ij| <= 1), half an ulp each: 4 ulp(M) for the two together."""
    p = np.asarray(points, F32).reshape(-1, 3)
    m = np.abs(p).sum(axis=1) + np.abs(np.asarray(pose, F32)[:3, 3]).max()
    return 4.0 * np.spacing(m.astype(F32)).astype(F64)


def _near_half(x, band):
    return np.abs(x - np.floor(x) - 0.5) <= band


def coin_toss(points, h, w, slack=None):
    """Is the reference row / column of each point within the band of a half-integer?  `slack` [n]: a displacement (metres)
    the point may carry (the transform rounding), which moves its column by slack / rho * W / (2 pi) and its row by
    slack / range * H / fov pixels; the band is widened by that amount."""
    p = np.asarray(points, F32).reshape(-1, 3)
    rows, cols, r = O.spherical_projection(p, h, w, UP_FOV, DOWN_FOV)
    band = toss_band(h, w)
    br = bc = np.full(p.shape[0], band)
    if slack is not None:
        fov = (abs(UP_FOV) + abs(DOWN_FOV)) / 180.0 * np.pi
        rho = np.sqrt(p[:, 0].astype(F64) ** 2 + p[:, 1].astype(F64) ** 2)
        with np.errstate(divide="ignore", invalid="ignore"):
            br = band + np.where(r > 0, slack / r * h / fov, 0.0)
            bc = band + np.where(rho > 0, slack / rho * w / (2 * np.pi), np.inf)
    return (_near_half(rows.astype(F64), br) | _near_half(cols.astype(F64), bc)) & (r > 0)


def pixel_index(points, h, w):
    """The oracle's pixel of each point (-1: outside the image or null), as build_projection_map rounds it."""
    rows, cols, r = O.spherical_projection(np.asarray(points, F32).reshape(-1, 3), h, w, UP_FOV, DOWN_FOV)
    pr, pc = np.round(rows), np.round(cols)
    ok = (pr >= 0) & (pr <= h - 1) & (pc >= 0) & (pc <= w - 1) & (r > 0)
    return np.where(ok, pr.astype(np.int64) * w + pc.astype(np.int64), -1)


def _row_keys(a):
    a = np.ascontiguousarray(np.asarray(a, F32).reshape(-1, 3))
    return a.view(np.dtype((np.void, 12))).reshape(-1)


def match_rows(rows, table):
    """Index into `table` [m,3] of every row of `rows` [n,3] by bit pattern (-1: absent).  `table` rows must be unique
    where they are matched (the first of equal rows is returned)."""
    tk, rk = _row_keys(table), _row_keys(rows)
    order = np.argsort(tk, kind="stable")
    pos = np.searchsorted(tk[order], rk)
    pos = np.minimum(pos, len(order) - 1) if len(order) else pos
    if not len(order):
        return np.full(len(rk), -1, np.int64)
    hit = tk[order][pos] == rk
    return np.where(hit, order[pos], -1)


def bit_model_unequal(rows, points, h, w):
    """`rows` [H*W,3] (the pixels of a vertex map as rows) against the bit model of the projection applied to `points` [n,3]
    (NaN rows: no point): (the pixels whose three floats are not the bits of the model's winner — zeros where it has none —,
    the number of pixels compared, the number of rows the model flags)."""
    import projection_audit as PA
    bit = PA.model(np.ascontiguousarray(points, F32), h, w, UP_FOV, DOWN_FOV)
    skip = PA.excluded_pixels(bit)
    got = np.ascontiguousarray(np.asarray(rows, F32).reshape(-1, 3))
    differ = (got.view(np.uint32) != bit.rows.view(np.uint32)).any(axis=1) & ~skip
    return np.flatnonzero(differ), int((~skip).sum()), int(bit.flagged.sum())


def account_model(mv, mn, vmaps, nmaps, poses, h, w):
    """Every pixel of every layer of a model (`mv`, `mn` [K,3,H,W]) against the oracle's build_model of the same window
    (`vmaps`, `nmaps` [3,H,W] per layer and the bit-identical `poses`).  A pixel is
      equal       same winning source pixel as the oracle's, vertex within transform_tolerance of the oracle's, and vertex
                  and normal bit-equal to the fma chain of that source pixel's vertex and (stored) normal;
      explained   another winner than the oracle's (or a winner on one side only), where (i) one of the two source points
                  has its reference row / column in the coin-toss band, or (ii) both land here with ranges within 2 float32
                  ulp of each other; the device's winner must still be bit-equal to the fma chain of a source pixel;
      unexplained anything else.
    Beside it the stricter accounting against the BIT MODEL of the projection (tests/projection_audit.py), which knows no coin
    toss: `model_unequal` counts the pixels whose vertex is not, bit for bit, the winner of that model applied to the fma chain
    of the layer's valid source pixels (pixel_of's validity, the lowest key) — zeros where the model has no winner;
    `model_compared` the pixels compared (all but those a flagged row of the model can enter: `model_flagged` rows)."""
    mv, mn = np.asarray(mv, F32), np.asarray(mn, F32)
    npix = h * w
    out = dict(occupied=0, equal=0, explained=0, worst_dv=0.0, worst_tol=0.0, unexplained=[], explained_pixels=set(),
               model_unequal=0, model_compared=0, model_flagged=0, model_first=[])
    assert mv.shape == (len(vmaps), 3, h, w) and mn.shape == mv.shape, (mv.shape, len(vmaps))
    for k, (v, nm, pose) in enumerate(zip(vmaps, nmaps, poses)):
        src = O.vertex_map_to_points(np.asarray(v, F32))
        src_n = O.vertex_map_to_points(np.asarray(nm, F32))
        valid = np.abs(src).max(axis=1) > 0
        dev_pts = transform_fma(src, pose)
        dev_nrm = transform_fma(src_n, pose, translate=False)
        ora_pts = O.apply_transformation(src, pose) * valid[:, None].astype(F32)
        _, oidx = O.build_projection_map(ora_pts, h, w, UP_FOV, DOWN_FOV, return_index=True)
        oidx = oidx.reshape(-1)
        tol = transform_tolerance(src, pose)
        toss = coin_toss(ora_pts, h, w, slack=tol) & valid
        opix = pixel_index(ora_pts, h, w)
        rng_o = range32(ora_pts)
        lv, ln = O.vertex_map_to_points(mv[k]), O.vertex_map_to_points(mn[k])
        occ = np.abs(lv).max(axis=1) > 0
        # the device's winner per occupied pixel, recovered by bit pattern from the fma chain of the valid source pixels
        table = np.where(valid[:, None], dev_pts, np.nan).astype(F32)
        didx = np.full(npix, -1, np.int64)
        didx[occ] = match_rows(lv[occ], table)
        out["occupied"] += int((occ | (oidx >= 0)).sum())
        unequal, compared, flagged = bit_model_unequal(lv, table, h, w)
        out["model_unequal"] += int(unequal.size)
        out["model_compared"] += compared
        out["model_flagged"] += flagged
        out["model_first"] += [(k, int(p // w), int(p % w)) for p in unequal[:4]]
        # the common case in one sweep: the oracle's winner, the bits of its fma chain, within the transform tolerance
        safe = np.maximum(didx, 0)
        dv = np.abs(lv.astype(F64) - ora_pts[safe].astype(F64)).max(axis=1)
        same = occ & (didx >= 0) & (didx == oidx) & (ln == dev_nrm[safe]).all(axis=1)
        if same.any():
            worst = int(np.argmax(np.where(same, dv - tol[safe], -np.inf)))
            if dv[worst] - tol[didx[worst]] > out["worst_dv"] - out["worst_tol"] or out["worst_tol"] == 0.0:
                out["worst_dv"], out["worst_tol"] = float(dv[worst]), float(tol[didx[worst]])
        fine = same & (dv <= tol[safe])
        out["equal"] += int(fine.sum())
        for p in np.nonzero((occ | (oidx >= 0) | (np.abs(ln).max(axis=1) > 0)) & ~fine)[0]:
            a, b = int(didx[p]), int(oidx[p])
            where = (k, int(p // w), int(p % w))
            if occ[p] and a < 0:
                out["unexplained"].append(where + ("vertex is no transformed source pixel of this layer",))
                continue
            if not occ[p] and np.abs(ln[p]).max() > 0:
                out["unexplained"].append(where + ("normal without a vertex",))
                continue
            if occ[p] and not np.array_equal(ln[p], dev_nrm[a]):
                out["unexplained"].append(where + ("normal is not the rotated normal of the winning source pixel",))
                continue
            if a == b:
                out["unexplained"].append(where + (f"vertex {dv[p]:.2e} from the oracle's, tolerance {tol[b]:.2e}",))
                continue
            ok = True
            if a >= 0:  # the device's winner must belong here by the reference's arithmetic, or be a coin toss
                ok &= bool(opix[a] == p or toss[a])
            why = (a >= 0 and bool(toss[a])) or (b >= 0 and bool(toss[b]))
            if a >= 0 and b >= 0 and not why:
                why = abs(float(rng_o[a]) - float(rng_o[b])) <= 2.0 * float(np.spacing(max(rng_o[a], rng_o[b])))
            if ok and why:
                out["explained"] += 1
                out["explained_pixels"].add(int(p))
            else:
                out["unexplained"].append(where + (f"winner {a} here, {b} in the oracle: neither a coin toss nor a tie",))
    return out


def account_recorded(recorded_mv, vmaps, poses, h, w, drift):
    """A model RECORDED from the reference's own run (`ls_model_vmap` of tests/golden/projective.npz) against the oracle's
    build_model of the window (`vmaps`, `poses`) the same updates leave.  The reference composed its poses in its own
    float32 arithmetic: `drift` is the bound on the difference per pose entry (pose_drift_bound), which moves a point by up
    to drift (|x| + |y| + |z| + 1).  Per layer and pixel: equal (both null, or both the same source pixel within that
    displacement + transform_tolerance), or explained (the oracle's winner or the recorded vertex's source pixel is a coin
    toss under that slack, or the two have ranges within 2 float32 ulp + the slack), or unexplained."""
    from scipy.spatial import cKDTree
    rec = np.asarray(recorded_mv, F32)
    out = dict(occupied=0, equal=0, explained=0, unexplained=[], same_winner=[])
    assert rec.shape == (len(vmaps), 3, h, w), rec.shape
    for k, (v, pose) in enumerate(zip(vmaps, poses)):
        src = O.vertex_map_to_points(np.asarray(v, F32))
        valid = np.abs(src).max(axis=1) > 0
        ora = O.apply_transformation(src, pose) * valid[:, None].astype(F32)
        _, oidx = O.build_projection_map(ora, h, w, UP_FOV, DOWN_FOV, return_index=True)
        oidx = oidx.reshape(-1)
        slack = transform_tolerance(src, pose) + drift * (np.abs(src).sum(axis=1).astype(F64) + 1.0)
        toss = coin_toss(ora, h, w, slack=slack) & valid
        rng_o = range32(ora).astype(F64)
        lv = O.vertex_map_to_points(rec[k])
        occ = np.abs(lv).max(axis=1) > 0
        vi = np.nonzero(valid)[0]
        dist, near = cKDTree(ora[vi].astype(F64)).query(lv.astype(F64))
        ridx = np.where(occ, vi[near], -1)  # the source pixel of the recorded vertex
        close = np.abs(lv.astype(F64) - ora[np.maximum(ridx, 0)].astype(F64)).max(axis=1) <= slack[np.maximum(ridx, 0)]
        out["occupied"] += int((occ | (oidx >= 0)).sum())
        fine = (~occ & (oidx < 0)) | (occ & close & (ridx == oidx))
        out["equal"] += int((fine & occ).sum())
        out["same_winner"].append((fine & occ).reshape(h, w))
        for p in np.nonzero(~fine)[0]:
            a, b = int(ridx[p]), int(oidx[p])
            where = (k, int(p // w), int(p % w))
            if occ[p] and not close[p]:
                out["unexplained"].append(where + ("recorded vertex is no transformed source pixel of this layer",))
                continue
            why = (a >= 0 and bool(toss[a])) or (b >= 0 and bool(toss[b]))
            if a >= 0 and b >= 0 and not why:
                why = abs(rng_o[a] - rng_o[b]) <= 2.0 * float(np.spacing(F32(max(rng_o[a], rng_o[b])))) + slack[a] + slack[b]
            if why:
                out["explained"] += 1
            else:
                out["unexplained"].append(where + (f"winner {a} recorded, {b} in the oracle",))
    return out


def recorded_run_updates(golden):
    """The update calls the reference's `ls` run made (tests/golden/projective.npz): its relative poses `ls_rel` under the
    key-frame rule of ICPFrameToModel as ICPProjectiveOracle.process_next_frame applies it (thresholds 0.1 m / 0.3 deg)."""
    cfg = O.ICPOracleConfig()
    calls = [(np.eye(4, dtype=F32), golden["vmaps"][0])]
    delta = np.eye(4, dtype=F32)
    for f in range(1, len(golden["vmaps"])):
        pose = golden["ls_rel"][f].astype(F32)
        new_delta = (delta @ pose).astype(F32)
        dp = O.from_pose_matrix(new_delta)
        if np.linalg.norm(dp[:3]) > cfg.threshold_trans or np.linalg.norm(dp[3:]) * 180 / np.pi > cfg.threshold_rot:
            calls.append((pose, golden["vmaps"][f]))
            delta = np.eye(4, dtype=F32)
        else:
            calls.append((pose, None))
            delta = new_delta
    return calls


def emulate_model(vmaps, nmaps, poses, h, w, keep_farther=False):
    """What pmap_build computes, on the CPU: the fma chain of every valid source pixel, a FLOAT64 spherical projection of
    the float32 result, the z-buffer keyed by (float32 range, highest index wins a tie).  The stand-in for the device in the
    CPU suite: it differs from the float32 oracle exactly where a float32 coordinate rounds to the other side of a
    half-integer.  `keep_farther`: a deliberately wrong z-buffer."""
    fov_up, fov_down = UP_FOV / 180.0 * np.pi, DOWN_FOV / 180.0 * np.pi
    fov = abs(fov_down) + abs(fov_up)
    mv = np.zeros((len(vmaps), 3, h * w), F32)
    mn = np.zeros_like(mv)
    for k, (v, nm, pose) in enumerate(zip(vmaps, nmaps, poses)):
        src, src_n = O.vertex_map_to_points(np.asarray(v, F32)), O.vertex_map_to_points(np.asarray(nm, F32))
        pts, nrm = transform_fma(src, pose), transform_fma(src_n, pose, translate=False)
        r = range32(pts)
        ok = (np.abs(src).max(axis=1) > 0) & (r > 0)
        x, y, z, r64 = (a.astype(F64) for a in (pts[:, 0], pts[:, 1], pts[:, 2], np.where(ok, r, 1)))
        row = np.rint((1.0 - (np.arcsin(np.clip(z / r64, -1, 1)) + abs(fov_down)) / fov) * h)
        col = np.rint(0.5 * (-np.arctan2(y, x) / np.pi + 1.0) * w)
        ok &= (row >= 0) & (row <= h - 1) & (col >= 0) & (col <= w - 1)
        idx = np.nonzero(ok)[0]
        pix = (row[idx] * w + col[idx]).astype(np.int64)
        # ascending write order, last write wins: descending range, then ascending index
        order = np.lexsort((idx, r[idx] if keep_farther else -r[idx]))
        win = np.full(h * w, -1, np.int64)
        win[pix[order]] = idx[order]
        hit = win >= 0
        mv[k][:, hit] = pts[win[hit]].T
        mn[k][:, hit] = nrm[win[hit]].T
    return mv.reshape(len(vmaps), 3, h, w), mn.reshape(len(vmaps), 3, h, w)


def window_poses(count, yaw=0.25, step=1.0, seed=3):
    """Relative poses with steps large enough that many points cross the azimuth seam and leave the vertical FoV: yaw of a
    few tenths of a radian, about a metre of translation, a little pitch / roll / heave."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        sign = -1.0 if k % 3 == 2 else 1.0
        out.append(O.build_pose_matrix(np.array(
            [step * (0.8 + 0.4 * rng.random()), 0.3 * rng.normal(), 0.05 * rng.normal(), 0.02 * rng.normal(),
             0.02 * rng.normal(), sign * yaw * (0.6 + 0.8 * rng.random())], F32)))
    return out


def window_sequence(h, w, local_map_size, source="scan"):
    """The update calls of part C: [(rel_pose, vmap or None)], at least 2 (local_map_size + 1) + 1 insertions so that every
    storage slot is recycled twice, a non-identity first pose, pose-only updates interleaved, and — the decisive step — a
    mostly-null map with structured holes inserted into the slot a dense one has just been evicted from."""
    inserts = 2 * (local_map_size + 1) + 2
    poses = window_poses(inserts + inserts // 3 + 1)
    calls, pi = [], 0
    for k in range(inserts):
        v = golden_vmap(k % 6) if source == "golden" else scan_vmap(h, w, frame=k % 4, step=0.6)
        if k >= local_map_size + 1 and k % 2 == 1:  # into a recycled slot: sparse, with holes
            v = damage(damage(v, "holes"), "salt50", seed=k)
        calls.append((poses[pi], v))
        pi += 1
        if k % 3 == 1:
            calls.append((poses[pi], None))
            pi += 1
    return calls


# ----------------------------------------------------------------------------------------------------------------------
# D. association
# ----------------------------------------------------------------------------------------------------------------------
def expected_association(mv, mn, points, index_map):
    """The rows pmap_nearest_neighbor_search must return, bit for bit, from the model it searches (`mv`, `mn` [K,3,H,W]), the
    target points [n,3] and the pixel every target won (`index_map` [H,W], -1 empty): per occupied target pixel, in pixel
    order, the layer a float32 argmin of sqrt((dx dx + dy dy) + dz dz) over the non-null layers selects (first minimum),
    no row where every layer is null.  Returns (neighbours, normals, targets, pixels, target indices)."""
    k, _, h, w = mv.shape
    lv = np.asarray(mv, F32).reshape(k, 3, -1)
    ln = np.asarray(mn, F32).reshape(k, 3, -1)
    idx = np.asarray(index_map).reshape(-1)
    pix = np.nonzero(idx >= 0)[0]
    t = np.asarray(points, F32).reshape(-1, 3)[idx[pix]]  # [m,3]
    q = lv[:, :, pix]  # [K,3,m]
    d = t.T[None] - q
    dist = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    dist = np.where(np.abs(q).max(axis=1) > 0, dist, np.inf)
    best = dist.argmin(axis=0)
    ok = np.isfinite(dist.min(axis=0)) & (np.abs(t).max(axis=1) > 0)
    m = np.arange(len(pix))
    nb, nn = q[best, :, m], ln[:, :, pix][best, :, m]
    return nb[ok], nn[ok], t[ok], pix[ok], idx[pix][ok]


def account_association(rows, mv, mn, points, index_map, oracle_rows=None, model_explained=frozenset()):
    """`rows` = (neighbours, normals, targets) as returned.  Exact part: equal to expected_association, row by row.  Against
    the oracle's (`oracle_rows`, from `nearest_neighbor_search` of a LibraryWindowOracle): the sets of matched targets are
    equal apart from targets whose pixel — or one of its eight neighbours, columns wrapping — holds the reference pixel of
    a target in the coin-toss band, or is an explained pixel of the model accounting.
    Beside it, stricter: `model_unequal` counts the pixels of `index_map` whose winner is not the winner of the bit model of the
    projection (tests/projection_audit.py) applied to `points`, and — the targets the search itself projected — the returned
    target rows that are not, in pixel order, that model's winners at the pixels some layer of the model occupies."""
    import projection_audit as PA
    nb, nn, tg = (np.asarray(a, F32).reshape(-1, 3) for a in rows)
    _, _, h, w = mv.shape
    pts = np.asarray(points, F32).reshape(-1, 3)
    enb, enn, etg, epix, eidx = expected_association(mv, mn, pts, index_map)
    out = dict(rows=int(tg.shape[0]), expected_rows=int(etg.shape[0]), explained=0, unexplained=[])
    bit = PA.model(np.ascontiguousarray(pts), h, w, UP_FOV, DOWN_FOV)
    skip = PA.excluded_pixels(bit)
    out["model_unequal"] = int(((np.asarray(index_map).reshape(-1) != bit.index.reshape(-1)) & ~skip).sum())
    out["model_flagged"] = int(bit.flagged.sum())
    if not skip.any():
        mtg = expected_association(mv, mn, pts, bit.index)[2]
        if mtg.shape != tg.shape:
            out["model_unequal"] += abs(int(mtg.shape[0]) - int(tg.shape[0])) or 1
        else:
            out["model_unequal"] += int((mtg.view(np.uint32) != np.ascontiguousarray(tg).view(np.uint32)).any(axis=1).sum())
    if tg.shape != etg.shape or not np.array_equal(tg, etg):
        out["unexplained"].append(("targets", "the matched targets / their order differ from the device's own pixels"))
        return out
    for name, got, exp in (("neighbour", nb, enb), ("normal", nn, enn)):
        diff = np.nonzero((got != exp).any(axis=1))[0]
        for r in diff[:8]:
            out["unexplained"].append((name, int(epix[r] // w), int(epix[r] % w), "not the argmin layer of the model"))
    if oracle_rows is not None:
        otg = np.asarray(oracle_rows[2], F32).reshape(-1, 3)
        finite = np.where(np.isfinite(pts).all(axis=1)[:, None], pts, 0).astype(F32)
        oi = match_rows(otg, finite)
        assert (oi >= 0).all()
        mine, theirs = set(match_rows(etg, finite).tolist()), set(oi.tolist())  # (equal rows count as one target)
        opix = pixel_index(finite, h, w)
        toss = coin_toss(finite, h, w)
        touched = np.zeros((h, w), bool)
        for p in list(opix[toss & (opix >= 0)]) + list(model_explained):
            r0, c0 = divmod(int(p), w)
            for dr in (-1, 0, 1):
                for dc in (-1, 0, 1):
                    if 0 <= r0 + dr < h:
                        touched[r0 + dr, (c0 + dc) % w] = True
        touched = touched.reshape(-1)
        for i in sorted(mine ^ theirs):
            if opix[i] >= 0 and touched[opix[i]] or toss[i]:
                out["explained"] += 1
            else:
                out["unexplained"].append(("target", int(i), "matched on one side only, no coin toss near its pixel"))
    return out


def association_targets(h, w, pose, frame=3, source="golden", extra_edges=True):
    """Unique target points of a scan moved by `pose` (float32 oracle transform), null pixels dropped; with `extra_edges`
    also rows outside the FoV, a NaN row, a (0,0,0) row and two nearer points in the pixel of the first one."""
    v = golden_vmap(frame) if source == "golden" else scan_vmap(h, w, frame=frame)
    pts = O.apply_transformation(O.vertex_map_to_points(v), np.asarray(pose, F32))
    pts = pts[np.abs(O.vertex_map_to_points(v)).max(axis=1) > 0]
    if extra_edges and pts.shape[0] > 4:
        first = pts[0].copy()
        edges = np.array([[1.0, 0.0, 5.0], [2.0, 0.5, -6.0], [np.nan, 1.0, 1.0], [0.0, 0.0, 0.0],
                          first * F32(0.5), first * F32(0.25)], F32)
        # (first * 0.5 and first * 0.25 share first's pixel: the nearest of the three must win it)
        pts = np.concatenate([pts, edges]).astype(F32)
    _, first_of = np.unique(_row_keys(np.where(np.isfinite(pts), pts, 0).astype(F32)), return_index=True)
    keep = np.zeros(pts.shape[0], bool)
    keep[first_of] = True
    keep |= ~np.isfinite(pts).all(axis=1)
    return np.ascontiguousarray(pts[keep])


# ----------------------------------------------------------------------------------------------------------------------
# E. one iteration's rows
# ----------------------------------------------------------------------------------------------------------------------
SCHEMES = ("default", "least_square", "huber", "exp", "neighborhood", "geman_mcclure", "square_geman_mcclure", "cauchy")
ROW_SIGMA = 0.05  # residuals of the E inputs spread over ~1e-3 .. 1e-1 m: both Huber branches occur


def plant_targets(mv, pose, count=24):
    """Targets t with fma-chain(pose, t) EXACTLY on a model point (r == 0 rows) and, from the same search, some a few ulp
    off it (0 < |r| < 1e-4: the clamp of robust_weight).  Candidates: t0 = R^T (q - trans) rounded to float32 and its 26
    one-ulp neighbours; a candidate that reproduces q bit for bit is an exact hit.  Returns (exact [a,3], near [b,3],
    pixels of the exact ones)."""
    k, _, h, w = mv.shape
    pose = np.asarray(pose, F32)
    lv = np.asarray(mv[0], F32).reshape(3, -1).T
    pix = np.nonzero(np.abs(lv).max(axis=1) > 0)[0]
    pix = pix[np.linspace(0, len(pix) - 1, min(len(pix), 40 * count)).astype(int)] if len(pix) else pix
    q = lv[pix]
    t0 = ((q.astype(F64) - pose[:3, 3].astype(F64)) @ pose[:3, :3].astype(F64)).astype(F32)
    exact, near, where = [], [], []
    steps = [(a, b, c) for a in (0, -1, 1) for b in (0, -1, 1) for c in (0, -1, 1)]
    for j in range(len(pix)):
        cand = np.stack([t0[j] + np.array(s, F32) * np.spacing(np.abs(t0[j])) for s in steps]).astype(F32)
        got = transform_fma(cand, pose)
        hit = np.nonzero((got == q[j]).all(axis=1))[0]
        if len(hit) and len(exact) < count:
            exact.append(cand[hit[0]])
            where.append(int(pix[j]))
        elif len(near) < count and not len(hit):
            near.append(cand[0])
    return (np.array(exact, F32).reshape(-1, 3), np.array(near, F32).reshape(-1, 3), np.array(where, np.int64))


def iteration_targets(mv, pose, scan_points, skip_null):
    """The target cloud of one E case: the scan's points, the planted ones in front (a planted target must win its pixel: the
    scan's points whose moved position falls into a planted pixel are dropped), a NaN row and a (0,0,0) row."""
    _, _, h, w = mv.shape
    exact, near, where = plant_targets(mv, pose)
    pts = np.asarray(scan_points, F32).reshape(-1, 3)
    moved = transform_fma(pts, pose)
    taken = set(where.tolist()) | set(pixel_index(transform_fma(near, pose), h, w).tolist())
    pts = pts[~np.isin(pixel_index(moved, h, w), list(taken))]
    odd = np.array([[np.nan, 0.0, 1.0], [0.0, 0.0, 0.0]], F32)
    return np.ascontiguousarray(np.concatenate([exact, near, odd, pts]).astype(F32)), len(exact)


def moved_targets(points, pose, skip_null):
    """What the iteration kernel associates: NaN rows dropped, null rows dropped under skip_null, the rest through the fma
    chain (a (0,0,0) row kept under TARGETS_ALL becomes the translation: a valid point unless the pose is the identity)."""
    p = np.asarray(points, F32).reshape(-1, 3)
    p = p[np.isfinite(p).all(axis=1)]
    if skip_null:
        p = p[np.abs(p).max(axis=1) > 0]
    return transform_fma(p, pose)


def host_step(rows, scheme, sigma):
    """dx, loss, row count of one Gauss-Newton step from association rows (neighbours, normals, targets): float32 rows,
    float64 normal equations (O.gauss_newton_step)."""
    nb, nn, tg = rows
    st = O.gauss_newton_step(tg, nb, nn, scheme, sigma, accumulate=F64)
    return st.dx, st.loss, int(np.asarray(tg).shape[0])


def residual_census(rows, sigma):
    """Which branches the rows exercise, by the oracle's own residuals."""
    nb, nn, tg = rows
    res, _ = O.point_to_plane_rows(tg, nb, nn)
    a = np.abs(res)
    return dict(quadratic=int((a < F32(sigma)).sum()), linear=int((a >= F32(sigma)).sum()),
                clamped=int(((a < F32(1.0e-4)) & (a > 0)).sum()), zero=int((a == 0).sum()))


def assert_step(dx, loss, count, ref):
    """The bars of test_gauss_newton_step against the float64 oracle."""
    rdx, rloss, rcount = ref
    assert count == rcount, (count, rcount)
    np.testing.assert_allclose(dx, rdx, atol=2e-7, rtol=2e-5)
    assert abs(loss - rloss) <= 1e-5 * abs(rloss), (loss, rloss)


def oracle_registration(orc, targets, init, iters, scheme, sigma):
    """`iters` forced iterations of ICPProjectiveOracle.process_next_frame's loop against the map `orc` (float64 normal
    equations); the final pose."""
    pose = np.asarray(init, F32).copy()
    for _ in range(iters):
        p = O.apply_transformation(targets, pose)
        q, n, t = orc.nearest_neighbor_search(p)
        step = O.gauss_newton_step(t, q, n, scheme, sigma, F64)
        pose = O.build_pose_matrix(O.from_pose_matrix((O.build_pose_matrix(step.dx) @ pose).astype(F32)))
    return pose


def iteration_case(h, w, source):
    """The map and the scan of one E case: (update calls, scan rows [H*W,3] with its null rows, initial poses).  Three maps
    in a window of four — the second with structured holes — then the next frame as the scan."""
    frames = [golden_vmap(k) if source == "golden" else scan_vmap(h, w, frame=k) for k in range(4)]
    rel = O.build_pose_matrix(np.array([0.4, 0.01, -0.01, 0.002, -0.001, 0.01], F32))
    calls = [(window_poses(1)[0], frames[0]), (rel, damage(frames[1], "holes")), (rel, None), (rel, frames[2])]
    inits = [np.eye(4, dtype=F32), O.build_pose_matrix(np.array([0.35, 0.03, -0.02, 0.004, -0.003, 0.02], F32))]
    return calls, O.vertex_map_to_points(frames[3]), inits
