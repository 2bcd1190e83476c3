"""The model the azimuth time stamps are held to (csrc/timestamps.hip; icp_estimate_timestamps, icp_kitti360_prepare,
icp_batch_estimate_timestamps), the clouds they are audited on and the comparison helpers.  TEST INFRASTRUCTURE, never
imported by the package.

The reference (`estimate_timestamps`, slam/common/geometry.py:443-466) stays in float32 for float32 rows, and numpy's
float32 arctan2 is not correctly rounded: no kernel can match it bit for bit.  The kernels evaluate atan2 in float64 and
round once to float32; every later step is the reference's, in float32, operation by operation.  `model` restates exactly
that in numpy, so the kernels are held to it BIT FOR BIT — except where the float64 arctan2 lies so close to the middle of
two float32 values that a float64 routine one or two ulp away from numpy's rounds to the other neighbour: `model` flags
those rows (`flagged`), and the clouds used here are chosen to have none.

Against the reference itself the bar is 4 x its own spread — max |reference(float32 rows) - reference(the same rows as
float64)| — measured by tests/test_timestamps_audit.py and recorded in tests/golden/timestamps_reference.npz: a float32
arctan2 that may be off by one ulp on either side allows 2 x the spread, rounding in the two float32 steps behind it takes
the rest (factor 4 is also the factor the de-skew audit uses over its reference's float64-against-long-double difference).

Seam: a row whose azimuth is within about 1.5e-7 rad of a = phi_0 (mod 2 pi), but not on it, gets time 0 or 1 depending
on the last bit of arctan2, and the reference's own float32 and float64 evaluations disagree there.  The clouds keep
every row at least 1e-5 rad from the seam of every (direction, phi_0) audited, or exactly on it (y = +-0, x < 0).
"""
import numpy as np

F32 = np.float32
PHI_0S = (0.0, float(np.pi), 1.0, -2.5)
DIRECTIONS = (True, False)
SEAM_MARGIN = 1.0e-5  # rad
FLAGGED_MAX = 1.0e-5  # share of a case's rows the model may flag


class Model:
    """phi [n] float32 (what k_azimuth writes), lo / hi (its min / max with NaN dropped, as fminf / fmaxf do), t [n] float64
    (what k_azimuth_normalise writes: the float32 quotient widened), flagged [n] bool."""

    def __init__(self, phi, lo, hi, t, flagged):
        self.phi, self.lo, self.hi, self.t, self.flagged = phi, lo, hi, t, flagged


def _wrap(a32, clockwise, phi_0):
    phi = a32 * F32(-1.0 if clockwise else 1.0)
    phi = phi - F32(phi_0)
    neg = phi < F32(0.0)
    phi[neg] = phi[neg] + F32(2.0 * np.pi)
    return phi


def normalise(phi, lo, hi):
    with np.errstate(invalid="ignore", divide="ignore"):
        return ((phi - lo) / (hi - lo)).astype(np.float64)


def near_rounding_boundary(a64):
    """a float64 arctan2 that, moved by two float64 ulp either way, would round to another float32: only there may the
    device's float64 atan2 legitimately pick the other neighbour"""
    a64 = np.asarray(a64, np.float64)
    a32 = a64.astype(F32)
    up = np.nextafter(np.nextafter(a64, np.inf), np.inf)
    down = np.nextafter(np.nextafter(a64, -np.inf), -np.inf)
    with np.errstate(invalid="ignore"):
        flagged = (up.astype(F32) != a32) | (down.astype(F32) != a32)
    return flagged & ~np.isnan(a64)


def model(rows, clockwise=True, phi_0=0.0, minmax_rows=None):
    """`rows`: [n, >= 3] float32.  `minmax_rows` (the wrong copy): min / max over that many leading rows only."""
    rows = np.asarray(rows)
    assert rows.dtype == np.float32 and rows.ndim == 2 and rows.shape[1] >= 3
    a64 = np.arctan2(rows[:, 1].astype(np.float64), rows[:, 0].astype(np.float64))
    a32 = a64.astype(F32)
    flagged = near_rounding_boundary(a64)
    phi = _wrap(a32, clockwise, phi_0)
    part = phi if minmax_rows is None else phi[:minmax_rows]
    with np.errstate(invalid="ignore"):
        lo, hi = np.fmin.reduce(part, initial=F32(np.inf)), np.fmax.reduce(part, initial=F32(-np.inf))
    return Model(phi, F32(lo), F32(hi), normalise(phi, F32(lo), F32(hi)), flagged)


# ---- clouds ----------------------------------------------------------------------------------------------------------
def seam_distance(rows, clockwise, phi_0):
    """|a - phi_0| mod 2 pi per row (a = -+atan2, float64): 0 on the seam of that (direction, phi_0)."""
    a = np.arctan2(rows[:, 1].astype(np.float64), rows[:, 0].astype(np.float64)) * (-1.0 if clockwise else 1.0)
    d = np.mod(a - phi_0, 2.0 * np.pi)
    return np.minimum(d, 2.0 * np.pi - d)


def seam_safe(rows):
    """every row at least SEAM_MARGIN from the seam of every audited (direction, phi_0), or exactly on it (y = +-0, x < 0)"""
    on = (rows[:, 1] == 0) & (rows[:, 0] < 0)
    ok = np.ones(rows.shape[0], bool)
    for cw in DIRECTIONS:
        for p in PHI_0S:
            ok &= seam_distance(rows, cw, p) >= SEAM_MARGIN
    return bool(np.all(ok | on))


def make_scan(seed, n, stride=4, seam_rows=0):
    """[n, stride] float32 rows of a spinning sensor: azimuths uniform over the turn, seam-safe; the last `seam_rows` rows
    lie exactly on the seam of (clockwise, phi_0 = pi): y = +0 / -0 alternating, x < 0."""
    rng = np.random.default_rng(seed)
    rows = np.empty((0, stride), F32)
    while rows.shape[0] < n - seam_rows:
        m = 2 * n + 16
        theta = rng.uniform(-np.pi, np.pi, m)
        r = rng.uniform(2.0, 80.0, m)
        cand = np.empty((m, stride), F32)
        cand[:, 0] = (r * np.cos(theta)).astype(F32)
        cand[:, 1] = (r * np.sin(theta)).astype(F32)
        cand[:, 2] = rng.uniform(-3.0, 3.0, m).astype(F32)
        if stride == 4:
            cand[:, 3] = rng.uniform(0.0, 1.0, m).astype(F32)
        ok = np.ones(m, bool)
        for cw in DIRECTIONS:
            for p in PHI_0S:
                ok &= seam_distance(cand, cw, p) >= SEAM_MARGIN
        ok &= seam_distance(cand, True, np.pi) >= SEAM_MARGIN  # (|theta| = pi, whatever float64 makes of PHI_0S[1])
        rows = np.concatenate((rows, cand[ok]))
    rows = rows[:n - seam_rows]
    if seam_rows:
        seam = np.zeros((seam_rows, stride), F32)
        seam[:, 0] = -rng.uniform(2.0, 80.0, seam_rows).astype(F32)
        seam[:, 1] = np.where(np.arange(seam_rows) % 2 == 0, F32(0.0), F32(-0.0))
        seam[:, 2] = rng.uniform(-3.0, 3.0, seam_rows).astype(F32)
        rows = np.concatenate((rows, seam))
    return np.ascontiguousarray(rows)


def place_extremes(rows, lo_at, hi_at, clockwise, phi_0):
    """a copy of `rows` with the row of the smallest phi moved to index lo_at and that of the largest to hi_at"""
    rows = rows.copy()
    m = model(rows, clockwise, phi_0)
    for at, pick in ((lo_at, np.nanargmin), (hi_at, np.nanargmax)):
        k = int(pick(model(rows, clockwise, phi_0).phi))
        rows[[at, k]] = rows[[k, at]]
    after = model(rows, clockwise, phi_0)
    assert after.lo == m.lo and after.hi == m.hi
    assert after.phi[lo_at] == m.lo and after.phi[hi_at] == m.hi
    return rows


# ---- comparison helpers ------------------------------------------------------------------------------------------------
def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_bits(a, b):
    """equal bit for bit, except that any NaN equals any NaN"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    nan = np.isnan(a) & np.isnan(b)
    return bool(np.all((_bits(a) == _bits(b)) | nan))


def check_bits(got, want, what=""):
    """`got` [n] float64 time stamps against the model's, bit for bit; the message names the first rows that differ"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float64 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    if not same_bits(got, want):
        nan = np.isnan(got) & np.isnan(want)
        bad = np.flatnonzero((_bits(got) != _bits(want)) & ~nan)
        raise AssertionError(f"{what}: {bad.size} of {got.size} rows differ from the model, first at {bad[:5].tolist()}: "
                             f"{got[bad[:5]].tolist()} against {want[bad[:5]].tolist()}")


def worst_difference(got, ref):
    """max |got - ref| over the rows (a NaN on one side only: inf)"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape
    if got.size == 0:
        return 0.0
    d = np.abs(got - ref)
    d[np.isnan(got) & np.isnan(ref)] = 0.0
    d[np.isnan(d)] = np.inf
    return float(d.max())


def check_within(got, ref, bound, what=""):
    """every row within `bound` of the reference; returns the worst difference"""
    worst = worst_difference(got, ref)
    assert worst <= bound, f"{what}: {worst:.3e} from the reference, the bar is {bound:.3e}"
    return worst


def check_seam(t, seam_index, what=""):
    """the exact-seam rows are exactly 0.0"""
    v = np.asarray(t)[seam_index]
    assert np.all(v == 0.0), f"{what}: seam rows at {v[v != 0.0][:5].tolist()}, expected exactly 0"


# ---- a KITTI-360 tree small enough for a test ---------------------------------------------------------------------------
def write_kitti360_tree(root, frames=3, rows=2000, drive=0, seed=77):
    """`frames` raw scans of `rows` records, `timestamps.txt` (one instant per frame, 0.1 s apart, nanosecond digits) and a
    `poses.txt` with two key poses — the first and the last frame, as the ground truth holds fewer poses than frames —
    under `root`, in the dataset's layout.  Returns the scans."""
    import os
    folder = f"2013_05_28_drive_{drive:04}_sync"
    velo = os.path.join(str(root), "data_3d_raw", folder, "velodyne_points")
    os.makedirs(os.path.join(velo, "data"))
    os.makedirs(os.path.join(str(root), "data_poses", folder))
    scans = []
    for i in range(frames):
        scan = make_scan(seed + i, rows, 4)
        scan.tofile(os.path.join(velo, "data", f"{i:010}.bin"))
        scans.append(scan)
    with open(os.path.join(velo, "timestamps.txt"), "w") as f:
        for i in range(frames):
            f.write(f"2013-05-28 08:46:{2 + i // 10:02}.{(i % 10) * 100000000 + 904295108 % 100000000:09}\n")

    def key_pose(yaw, pitch, t):
        cy, sy, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
        rot = np.array([[cy, -sy, 0.0], [sy, cy, 0.0], [0.0, 0.0, 1.0]]) @ np.array([[cp, 0.0, sp], [0.0, 1.0, 0.0], [-sp, 0.0, cp]])
        return np.concatenate((rot, np.asarray(t, np.float64).reshape(3, 1)), axis=1).reshape(-1)

    keys = {0: key_pose(0.3, 0.02, (845.1, 3725.4, 116.2)), frames - 1: key_pose(0.34, 0.015, (846.3, 3725.9, 116.25))}
    with open(os.path.join(str(root), "data_poses", folder, "poses.txt"), "w") as f:
        for k, p in keys.items():
            f.write(" ".join([str(k)] + [f"{v:.10f}" for v in p]) + "\n")
    return scans
