"""The model the spherical projection and its z-buffer are held to (csrc/projection.hip, csrc/projection_device.h:
icp_project, icp_project_rows, icp_project_pixels, icp_batch_project, icp_batch_project_rows and frame 0 of the frame calls),
the clouds they are audited on and the comparison helpers.  TEST INFRASTRUCTURE, never imported by the package.

The reference (`torch__spherical_projection`, slam/common/projection.py:11-73, and `Projector.build_projection_map`,
:331-418) evaluates atan2 and asin in float32, and its own code paths disagree in their last bit: no kernel can match it bit
for bit.  The kernels decide the pixel from the angles evaluated in float64 and rounded once to float32 wherever the fast
float32 coordinate lies within 2e-3 pixel of a half-integer, and claim that elsewhere the fast path cannot change the pixel.
`model` restates the exact path everywhere, operation by operation in float32, so a kernel that equals it BIT FOR BIT has
both the exact path and that claim right — except where the float64 angle lies so close to the middle of two float32
values that a float64 routine one or two ulp from numpy's rounds to the other neighbour: `model` flags those rows
(`flagged`), and the clouds used here, seeded, have none.

Two edges are settled as the reference settles them: x*x + y*y + z*z follows IEEE gradual underflow (a point of 1e-20 m has
a subnormal sum of squares, a range > 0 and is kept; at 1e-23 m the squares are 0 and the row is masked by `r == 0`,
projection.py:55-57), and a range that overflows to +inf keeps its point (inf > 0, :409).
"""
import numpy as np

from timestamps_audit import near_rounding_boundary

F32 = np.float32
F64 = np.float64
BAND = F32(2.0e-3)  # near_half of csrc/projection_device.h
FOVS = ((3.0, -24.0), (15.0, -15.0), (2.0, -2.0), (0.0, -90.0))
WRONG = ("farther_wins", "tie_lowest_index", "half_away", "less_than_at_edge", "column_band_only", "no_refinement",
         "fused_range", "fov_float32", "stale_zbuffer")


class Model:
    """row, col, r [n] float32 (what k_project_pixels writes, and the range of the key); pixel [n] int64 (-1: dropped);
    index [H, W] int32 (-1: empty); vmap [3, H, W] and rows [H * W, 3] float32 (zeros where empty); keys [H * W] uint64 (the
    z-buffer after the scatter, all ones where empty); flagged [n] bool."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def fov_params(up_fov, down_fov, wrong=None):
    """(fov_down_abs, fov) as `proj_params` forms them: degrees held in float32, radians in float64, one cast each"""
    up = F64(F32(up_fov)) / 180.0 * np.pi
    down = F64(F32(down_fov)) / 180.0 * np.pi
    if wrong == "fov_float32":
        return F32(abs(down)), F32(abs(down)) + F32(abs(up))
    return F32(abs(down)), F32(abs(down) + abs(up))


def _range(x, y, z, wrong=None):
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        if wrong == "fused_range":
            from projective_cases import fma32
            return np.sqrt(fma32(z, z, fma32(y, y, x * x)))
        return np.sqrt((x * x + y * y) + z * z)


def near_half(v):
    with np.errstate(invalid="ignore"):
        return np.abs(v - np.floor(v) - F32(0.5)) < BAND


def coordinates(pts, h, w, up_fov, down_fov, exact=True, wrong=None):
    """(row, col, r, flagged): float32 operations in the order of `spherical_rowcol`; `exact` False: the angles by numpy's
    float32 arctan2 / arcsin (a stand-in for a fast path; never what the kernels are held to)"""
    pts = np.asarray(pts)
    assert pts.dtype == np.float32 and pts.ndim == 2 and pts.shape[1] == 3, (pts.dtype, pts.shape)
    x, y, z = (np.ascontiguousarray(pts[:, k]) for k in range(3))
    fda, fov = fov_params(up_fov, down_fov, wrong)
    r = _range(x, y, z, wrong)
    with np.errstate(all="ignore"):
        q = z / r
        if exact:
            a64, s64 = np.arctan2(y.astype(F64), x.astype(F64)), np.arcsin(q.astype(F64))
            flagged = (near_rounding_boundary(a64) | near_rounding_boundary(s64)) & (r != 0)
            theta, phi = -(a64.astype(F32)), s64.astype(F32)
        else:
            flagged = np.zeros(x.shape, bool)
            theta, phi = -np.arctan2(y, x), np.arcsin(q)
        pc = F32(0.5) * (theta / F32(np.pi) + F32(1.0))
        pr = F32(1.0) - (phi + fda) / fov
        col, row = pc * F32(w), pr * F32(h)
    null = r == 0
    row, col = np.where(null, F32(-1.0), row).astype(F32), np.where(null, F32(-1.0), col).astype(F32)
    return row, col, r.astype(F32), flagged


def _round(v, wrong=None):
    with np.errstate(invalid="ignore"):
        if wrong == "half_away":
            return np.where(np.isnan(v), v, np.sign(v) * np.floor(np.abs(v) + F32(0.5))).astype(F32)
        return np.rint(v)


def empty_keys(h, w):
    return np.full(h * w, ~np.uint64(0), np.uint64)


def model(pts, h, w, up_fov=3.0, down_fov=-24.0, wrong=None, keys=None):
    """`wrong`: one of WRONG, a deliberately wrong copy.  `keys`: the z-buffer the scatter starts from (only the
    "stale_zbuffer" copy passes anything but a clean one)."""
    pts = np.ascontiguousarray(pts, F32).reshape(-1, 3)
    n = pts.shape[0]
    assert wrong is None or wrong in WRONG, wrong
    row, col, r, flagged = coordinates(pts, h, w, up_fov, down_fov, True, wrong)
    prow_src, pcol_src = row, col
    if wrong in ("column_band_only", "no_refinement"):
        frow, fcol, _, _ = coordinates(pts, h, w, up_fov, down_fov, False)
        refine = near_half(fcol) if wrong == "column_band_only" else np.zeros(n, bool)
        prow_src, pcol_src = np.where(refine, row, frow), np.where(refine, col, fcol)
    prow, pcol = _round(prow_src, wrong), _round(pcol_src, wrong)
    with np.errstate(invalid="ignore"):
        if wrong == "less_than_at_edge":
            valid = (prow >= 0) & (prow < h - 1) & (pcol >= 0) & (pcol < w - 1) & (r > 0)
        else:
            valid = (prow >= 0) & (prow <= h - 1) & (pcol >= 0) & (pcol <= w - 1) & (r > 0)
    pixel = np.full(n, -1, np.int64)
    pixel[valid] = prow[valid].astype(np.int64) * w + pcol[valid].astype(np.int64)
    rbits = r.view(np.uint32).astype(np.uint64)
    low = np.arange(n, dtype=np.uint32)
    if wrong == "farther_wins":
        rbits = np.uint64(0xffffffff) - rbits
    if wrong != "tie_lowest_index":
        low = ~low
    key = (rbits << np.uint64(32)) | low.astype(np.uint64)
    zbuf = empty_keys(h, w) if keys is None else np.array(keys, np.uint64)
    v = np.flatnonzero(valid)
    np.minimum.at(zbuf, pixel[v], key[v])
    index = np.full(h * w, -1, np.int32)
    won = zbuf != ~np.uint64(0)
    low_won = (zbuf[won] & np.uint64(0xffffffff)).astype(np.uint32)
    index[won] = (low_won if wrong == "tie_lowest_index" else ~low_won).astype(np.int32)
    rows = np.zeros((h * w, 3), F32)
    inside = won & (index >= 0) & (index < n)  # (a stale key may name a row this cloud does not have)
    rows[inside] = pts[index[inside]]
    return Model(row=row, col=col, r=r, pixel=pixel, valid=valid, flagged=flagged, keys=zbuf, index=index.reshape(h, w),
                 rows=rows, vmap=np.ascontiguousarray(rows.T).reshape(3, h, w), n=n, h=h, w=w)


def excluded_pixels(m):
    """[H * W] bool: the (at most two) pixels each flagged row can enter.  All False on every cloud of this file."""
    out = np.zeros(m.h * m.w, bool)
    for i in np.flatnonzero(m.flagged):
        for dr in (-2, 0, 2):
            for dc in (-2, 0, 2):
                pr = np.rint(m.row[i] + dr * np.spacing(np.abs(m.row[i])))
                pc = np.rint(m.col[i] + dc * np.spacing(np.abs(m.col[i])))
                if 0 <= pr <= m.h - 1 and 0 <= pc <= m.w - 1:
                    out[int(pr) * m.w + int(pc)] = True
    return out


# ---- clouds ----------------------------------------------------------------------------------------------------------
def _radians(up_fov, down_fov):
    return abs(up_fov) / 180.0 * np.pi, abs(down_fov) / 180.0 * np.pi


def _points(az, el, rng_m):
    az, el, rng_m = (np.asarray(v, F64) for v in (az, el, rng_m))
    return np.stack((rng_m * np.cos(el) * np.cos(az), rng_m * np.cos(el) * np.sin(az), rng_m * np.sin(el)), axis=1).astype(F32)


def _az_of(col, w):
    return -np.pi * (2.0 * np.asarray(col, F64) / w - 1.0)


def _el_of(row, h, up_fov, down_fov):
    a_up, a_down = _radians(up_fov, down_fov)
    return (1.0 - np.asarray(row, F64) / h) * (a_up + a_down) - a_down


def at_columns(rng, cols, h, w, up_fov, down_fov):
    """points whose float64 column is `cols`, at a random row inside the image and a random range"""
    cols = np.asarray(cols, F64)
    return _points(_az_of(cols, w), _el_of(rng.uniform(0.0, h - 1.0, cols.shape), h, up_fov, down_fov),
                   rng.uniform(1.0, 80.0, cols.shape))


def at_rows(rng, rows, h, w, up_fov, down_fov):
    """points whose float64 row is `rows`, at a random column inside the image and a random range"""
    rows = np.asarray(rows, F64)
    return _points(_az_of(rng.uniform(0.0, w - 1.0, rows.shape), w), _el_of(rows, h, up_fov, down_fov),
                   rng.uniform(1.0, 80.0, rows.shape))


def _move_ulps(a, s):
    toward = F32(np.inf if s > 0 else -np.inf)
    for _ in range(abs(s)):
        a = np.nextafter(a, toward)
    return a


def lidar(seed, n, h, w, up_fov=3.0, down_fov=-24.0):
    """azimuth uniform, elevation over the field of view and 2 degrees either side, ranges 1 .. 80 m"""
    rng = np.random.default_rng(seed)
    a_up, a_down = _radians(up_fov, down_fov)
    margin = 2.0 / 180.0 * np.pi
    el = np.clip(rng.uniform(-a_down - margin, a_up + margin, n), -np.pi / 2, np.pi / 2)
    return _points(rng.uniform(-np.pi, np.pi, n), el, rng.uniform(1.0, 80.0, n))


def _boundaries(h, w, per):
    return np.repeat(np.arange(w) + 0.5, per), np.repeat(np.arange(-1, h) + 0.5, per)


def boundary(seed, h, w, up_fov=3.0, down_fov=-24.0, per=4, ulps=(1, 2, 3)):
    """`per` points on every column boundary k + 0.5 and every row boundary j + 0.5 (j = -1: the image's upper edge), and
    copies with y and z moved by 1, 2, 3 float32 ulp either way"""
    rng = np.random.default_rng(seed)
    cols, rows = _boundaries(h, w, per)
    base = np.concatenate((at_columns(rng, cols, h, w, up_fov, down_fov), at_rows(rng, rows, h, w, up_fov, down_fov)))
    out = [base]
    for s in ulps:
        for sign in (1, -1):
            c = base.copy()
            c[:, 1], c[:, 2] = _move_ulps(c[:, 1], sign * s), _move_ulps(c[:, 2], sign * s)
            out.append(c)
    return np.ascontiguousarray(np.concatenate(out))


def band_edge(seed, h, w, up_fov=3.0, down_fov=-24.0, per=4):
    """the same boundaries, every point 1e-4 .. 1e-2 pixel (log-uniform) off its boundary on either side: rows just inside
    and just outside the refinement band"""
    rng = np.random.default_rng(seed)
    cols, rows = _boundaries(h, w, per)

    def off(a):
        return a + rng.choice((-1.0, 1.0), a.shape) * 10.0 ** rng.uniform(-4.0, -2.0, a.shape)
    return np.ascontiguousarray(np.concatenate((at_columns(rng, off(cols), h, w, up_fov, down_fov),
                                                at_rows(rng, off(rows), h, w, up_fov, down_fov))))


def image_edge(seed, h, w, up_fov=3.0, down_fov=-24.0):
    """rows around -0.5, 0.5, H - 1.5, H - 0.5; columns around 0, 0.5, W - 0.5, W; the +-pi seam (x < 0, y = +-0 and y one
    ulp — subnormal, smallest normal, 1e-30 — either side; y = -0 gives col = W, dropped); the z axis (x = y = +-0, all four
    sign pairs, phi = +-pi / 2); |q| = 1 after rounding"""
    rng = np.random.default_rng(seed)
    offs = np.array([0.0, 1e-7, -1e-7, 1e-6, -1e-6, 1e-5, -1e-5, 1e-4, -1e-4, 1e-3, -1e-3, 1.9e-3, -1.9e-3, 2.1e-3, -2.1e-3,
                     3e-3, -3e-3, 0.4, -0.4])
    rows = (np.array([-0.5, 0.5, h - 1.5, h - 0.5])[:, None] + offs[None, :]).reshape(-1)
    cols = (np.array([0.0, 0.5, w - 0.5, float(w)])[:, None] + offs[None, :]).reshape(-1)
    parts = [at_rows(rng, np.tile(rows, 2), h, w, up_fov, down_fov), at_columns(rng, np.tile(cols, 2), h, w, up_fov, down_fov)]
    tiny = np.array([0.0, -0.0, 1.4e-45, -1.4e-45, 1.17549435e-38, -1.17549435e-38, 1e-30, -1e-30, 1e-9, -1e-9], F32)
    seam = np.zeros((tiny.size * 3, 3), F32)
    seam[:, 0] = -np.repeat(np.array([1.0, 17.3, 80.0], F32), tiny.size)
    seam[:, 1] = np.tile(tiny, 3)
    seam[:, 2] = np.tan(_el_of(h / 2.0, h, up_fov, down_fov)) * -seam[:, 0]
    parts.append(seam)
    axis = np.array([[sx, sy, sz] for sx in (0.0, -0.0) for sy in (0.0, -0.0) for sz in (5.0, -5.0)], F32)
    parts.append(axis)
    parts.append(np.array([[1e-4, 1e-4, 50.0], [1e-4, -1e-4, -50.0], [1e-3, 0.0, 70.0], [-1e-5, 1e-6, 33.0],
                           [3e-4, 0.0, -1.0], [60.0, 1e-4, 1e-5]], F32))
    return np.ascontiguousarray(np.concatenate(parts))


SPECIAL_KINDS = ("zero", "nan", "inf", "overflow", "subnormal_squares", "underflow", "negative_zero", "plain")


def special(h, w, up_fov=3.0, down_fov=-24.0):
    """(points, kind per row): all-zero rows; a NaN in each coordinate; +-inf rows; rows of 1e20 (the squares overflow, r = inf),
    two of them bit-equal and a third in the same pixel; rows of 1e-19 .. 1e-22 (subnormal squares) and 1e-23 .. 1e-25 (the
    squares underflow to 0); rows of -0.0; four plain points"""
    el = np.tan(_el_of(h / 2.0, h, up_fov, down_fov))
    pts, kind = [], []

    def add(k, *rows):
        for r in rows:
            pts.append(r)
            kind.append(SPECIAL_KINDS.index(k))

    def mid(x, y):  # at the middle row of the image
        return [x, y, el * np.hypot(x, y)]
    add("zero", [0, 0, 0], [0, 0, 0], [0, 0, 0])
    nan, inf = np.nan, np.inf
    add("nan", [nan, 1, 1], [1, nan, 1], [1, 1, nan], [nan, nan, nan], [nan, 0, 0])
    add("inf", [inf, 1, 1], [1, -inf, 1], [1, 1, inf], [inf, inf, inf], [-inf, 1, -inf], [1, 1, -inf], [-inf, -1, 0])
    add("overflow", mid(1e20, 1e18), mid(1e20, 1e18), mid(2e20, 2e18), mid(-1e20, 3e19))
    for e in (19, 20, 21, 22):
        s = 10.0 ** -e
        add("subnormal_squares", mid(s, 0.3 * s), mid(-0.5 * s, s))
    for e in (23, 24, 25):
        s = 10.0 ** -e
        add("underflow", mid(s, 0.3 * s), mid(-0.5 * s, s))
    add("negative_zero", [-0.0, -0.0, -0.0], [-0.0, 0.0, 0.0], [0.0, 0.0, -0.0])
    add("plain", mid(10, 0.1), mid(10, 0.1), mid(-20, 5), mid(3, -3))
    with np.errstate(over="ignore", under="ignore"):
        return np.array(pts, F64).astype(F32), np.array(kind)


def in_pixel(rng, j, k, m, h, w, up_fov, down_fov, rng_m=None):
    """m points inside pixel (j, k), at least 0.1 pixel from its edges; `rng_m`: one range for all of them (the float32
    ranges of the rounded points then take a handful of values: equal-range ties), else 1 .. 80 m"""
    return _points(_az_of(k + rng.uniform(-0.4, 0.4, m), w), _el_of(j + rng.uniform(-0.4, 0.4, m), h, up_fov, down_fov),
                   np.full(m, rng_m) if rng_m is not None else rng.uniform(1.0, 80.0, m))


def ties(seed, h, w, up_fov=3.0, down_fov=-24.0):
    """pixels that receive 2 (bit-equal duplicates), 257 and 4 096 points of (nearly) one range; a pixel astride y = 0 with
    (x, y, z) / (x, -y, z) pairs — equal ranges, different points; a pixel with three clearly different ranges; shuffled"""
    rng = np.random.default_rng(seed)
    j = [min(h - 1, v) for v in (0, h // 3, h // 2, h - 1)]
    k = [min(w - 1, v) for v in (1, w // 3, w - 2)]
    two = in_pixel(rng, j[1], k[0], 1, h, w, up_fov, down_fov)
    pairs = in_pixel(rng, j[2], w // 2, 8, h, w, up_fov, down_fov, 12.0)
    mirrored = pairs * np.array([1, -1, 1], F32)
    parts = [two, two, in_pixel(rng, j[0], k[1], 257, h, w, up_fov, down_fov, 10.0),
             in_pixel(rng, j[3], k[2], 4096, h, w, up_fov, down_fov, 7.0), pairs, mirrored, pairs[:3],
             in_pixel(rng, j[1], k[2], 1, h, w, up_fov, down_fov, 5.0), in_pixel(rng, j[1], k[2], 1, h, w, up_fov, down_fov, 10.0),
             in_pixel(rng, j[1], k[2], 1, h, w, up_fov, down_fov, 20.0)]
    out = np.concatenate(parts)
    return np.ascontiguousarray(out[rng.permutation(out.shape[0])])


def one_pixel(seed, h, w, up_fov=3.0, down_fov=-24.0, m=1000):
    """every point in one pixel; the nearest one three times over"""
    rng = np.random.default_rng(seed)
    pts = in_pixel(rng, h // 2, w // 2 - 1 if w > 1 else 0, m, h, w, up_fov, down_fov)
    near = pts[np.argmin(_range(pts[:, 0], pts[:, 1], pts[:, 2]))]
    pts[[m // 7, m // 2, m - 3]] = near
    return np.ascontiguousarray(pts)


def padded(cloud, v):
    """the first `v` rows of `cloud`, NaN rows behind them: what the padded grid sample hands over"""
    out = np.array(cloud, F32)
    out[v:] = np.nan
    return out


def padded_cases(cloud):
    n = cloud.shape[0]
    return {f"padded_V{v}": padded(cloud, v) for v in (0, 1, n - 1, n)}


SEEDS = dict(lidar=101, boundary=202, band_edge=303, image_edge=404, ties=505, one_pixel=606)


def clouds(h, w, up_fov=3.0, down_fov=-24.0, n_lidar=4099, per=None, which=None):
    """name -> [n, 3] float32: every cloud of the audit on one image (seeds fixed).  `per`: points per boundary of the boundary
    cloud (default: 4 up to 256 columns, else 2), four times as many for the band-edge cloud — at 64 x 2048: 29 582 boundary
    rows, 16 904 band-edge rows."""
    per = per if per is not None else (4 if w <= 256 else 2)
    make = dict(lidar=lambda: lidar(SEEDS["lidar"], n_lidar, h, w, up_fov, down_fov),
                boundary=lambda: boundary(SEEDS["boundary"], h, w, up_fov, down_fov, per),
                band_edge=lambda: band_edge(SEEDS["band_edge"], h, w, up_fov, down_fov, 4 * per),
                image_edge=lambda: image_edge(SEEDS["image_edge"], h, w, up_fov, down_fov),
                special=lambda: special(h, w, up_fov, down_fov)[0],
                ties=lambda: ties(SEEDS["ties"], h, w, up_fov, down_fov),
                one_pixel=lambda: one_pixel(SEEDS["one_pixel"], h, w, up_fov, down_fov))
    return {name: make[name]() for name in (which or make)}


# ---- the cases of tests/test_gpu_projection_audit.py, listed once: tests/test_projection_audit.py asserts on the CPU that
# the model flags no row of any of them -------------------------------------------------------------------------------
IMAGES = ((16, 128), (64, 2048))
SMALL_IMAGES = ((1, 1), (1, 300), (3, 3), (5, 7), (255, 1), (256, 1), (257, 1))
LARGE_IMAGES = ((128, 4096), (128, 8192), (128, 16384))
PIXEL_COUNTS = (1, 255, 256, 257, 65537)
STATE_IMAGE = (16, 512)
_CACHE = {}


def _frozen(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
        for a in _CACHE[key].values():
            a.setflags(write=False)
    return _CACHE[key]


def pixel_cases(h, w, up_fov, down_fov):
    """every cloud on one image and field of view, and LiDAR-like clouds of the lengths at the launch grid's edges"""
    def make():
        out = clouds(h, w, up_fov, down_fov)
        out.update({f"lidar_n{n}": lidar(SEEDS["lidar"] + n, n, h, w, up_fov, down_fov) for n in PIXEL_COUNTS})
        return out
    return _frozen(("pixels", h, w, up_fov, down_fov), make)


def map_cases(h, w, up_fov=3.0, down_fov=-24.0):
    """the clouds `project` / `project_rows` are held on: all of them at 16 x 128, the three boundary clouds at 64 x 2048, and
    on the small images (where a tie pixel cannot be placed) everything but the tie clouds, with 300 LiDAR-like rows"""
    def make():
        if (h, w) == IMAGES[0]:
            return clouds(h, w, up_fov, down_fov)
        if (h, w) == IMAGES[1]:
            return clouds(h, w, up_fov, down_fov, which=("boundary", "band_edge", "image_edge"))
        return clouds(h, w, up_fov, down_fov, n_lidar=300, which=("lidar", "boundary", "band_edge", "image_edge", "special"))
    return _frozen(("map", h, w, up_fov, down_fov), make)


def large_cases(h, w):
    """8 points per boundary: the boundary cloud (with its 1-ulp copies) and the band-edge cloud"""
    return _frozen(("large", h, w), lambda: dict(boundary=boundary(SEEDS["boundary"], h, w, per=8, ulps=(1,)),
                                                band_edge=band_edge(SEEDS["band_edge"], h, w, per=8)))


def batch_members(count):
    """the clouds of a batch of `count` members at 16 x 128: member 0 empty and member 1 NaN rows only (count >= 3), clouds of
    different lengths between them, the longest last"""
    def make():
        h, w = IMAGES[0]
        if count == 1:
            return {"0": lidar(SEEDS["lidar"], 1500, h, w)}
        named = clouds(h, w)
        pool = [named[k] for k in ("ties", "image_edge", "special", "band_edge", "boundary", "one_pixel")]
        out = {"0": np.zeros((0, 3), F32), "1": np.full((300, 3), np.nan, F32)}
        for b in range(2, count - 1):
            out[str(b)] = pool[b - 2] if b - 2 < len(pool) else lidar(SEEDS["lidar"] + b, 100 + 37 * b, h, w)
        out[str(count - 1)] = lidar(SEEDS["lidar"] + count, 5003, h, w)
        return out
    return [v for _, v in sorted(_frozen(("batch", count), make).items(), key=lambda kv: int(kv[0]))]


def state_clouds():
    """the clouds of the z-buffer sequence at STATE_IMAGE: three scans of the synthetic drive (dense), a 10-point cloud and
    every 7th row of a scan moved 1.5 times as far (sparse: it wins no pixel against keys left behind)"""
    def make():
        from pylidar_slam_amd.synthetic import SceneConfig, make_sequence
        h, w = STATE_IMAGE
        scans = make_sequence(SceneConfig(height=h, width=w), 3)[0]
        out = {f"scan{i}": np.ascontiguousarray(s, F32) for i, s in enumerate(scans)}
        out["ten"] = lidar(SEEDS["lidar"] + 7, 10, h, w)
        out["sparse"] = np.ascontiguousarray(out["scan2"][::7] * F32(1.5))
        return out
    return _frozen(("state",), make)


def yaw_pose(angle=0.25):
    c, s = np.cos(angle), np.sin(angle)
    return np.array([[c, -s, 0, 0], [s, c, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], F64).astype(F32)


def planted(h=16, w=128, angle=0.25):
    """The boundary cloud for the projective kernels, which transform before they project: `rows` (the cloud), `turned` (the
    cloud turned by the yaw in float64 and rounded, so that the inverse yaw puts it back within an ulp or two of its
    boundaries), `back` (turned the other way), and the first H * W rows of `rows` and `turned` as [3, H, W] vertex maps."""
    def make():
        rows = boundary(SEEDS["boundary"], h, w)
        yaw = yaw_pose(angle).astype(F64)[:3, :3]
        turned = (rows.astype(F64) @ yaw.T).astype(F32)
        back = (rows.astype(F64) @ yaw).astype(F32)
        as_map = lambda a: np.ascontiguousarray(a[:h * w].T).reshape(3, h, w)
        return dict(rows=rows, turned=turned, back=back, vmap=as_map(rows), vmap_turned=as_map(turned))
    return _frozen(("planted", h, w, angle), make)


def every_gpu_case():
    """(what, h, w, up_fov, down_fov, cloud) of every cloud the GPU file projects"""
    for h, w in IMAGES:
        for fov in FOVS:
            for name, c in pixel_cases(h, w, *fov).items():
                yield f"pixels {h}x{w} {fov} {name}", h, w, fov[0], fov[1], c
    for h, w in IMAGES + SMALL_IMAGES:
        for name, c in map_cases(h, w).items():
            yield f"map {h}x{w} {name}", h, w, 3.0, -24.0, c
    for h, w in LARGE_IMAGES:
        for name, c in large_cases(h, w).items():
            yield f"large {h}x{w} {name}", h, w, 3.0, -24.0, c
    for count in (1, 3, 32):
        for b, c in enumerate(batch_members(count)):
            yield f"batch of {count}, member {b}", IMAGES[0][0], IMAGES[0][1], 3.0, -24.0, c
    for name, c in state_clouds().items():
        yield f"state {name}", STATE_IMAGE[0], STATE_IMAGE[1], 3.0, -24.0, c


# ---- comparison helpers ------------------------------------------------------------------------------------------------
def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def differing(got, want):
    """flat indices where `got` and `want` differ in their bits (any NaN equals any NaN)"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    bad = _bits(got) != _bits(want)
    if got.dtype.kind == "f":
        bad &= ~(np.isnan(got) & np.isnan(want))
    return np.flatnonzero(bad.reshape(-1))


def check_bits(got, want, what="", skip=None):
    """bit for bit; `skip`: a mask (shape of `want`) of entries left out; returns how many were compared.  The message names
    the first entries that differ."""
    bad = differing(got, want)
    if skip is not None:
        bad = bad[~np.broadcast_to(skip, np.shape(want)).reshape(-1)[bad]]
    if bad.size:
        g, w_ = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
        at = [tuple(int(v) for v in np.unravel_index(b, np.shape(want))) for b in bad[:5]]
        raise AssertionError(f"{what}: {bad.size} of {g.size} entries differ from the model, first at {at}: "
                             f"{g[bad[:5]].tolist()} against {w_[bad[:5]].tolist()}")
    return int(np.size(want) - (0 if skip is None else np.count_nonzero(np.broadcast_to(skip, np.shape(want)))))


def account(index, m, pts, limit=8):
    """for every pixel whose winner differs from the model's: both winners, their ranges and their float coordinates"""
    index = np.asarray(index).reshape(-1)
    want = m.index.reshape(-1)
    lines = []
    for p in np.flatnonzero(index != want)[:limit]:
        def who(i):
            if i < 0 or i >= m.n:
                return f"{int(i)}"
            return (f"{int(i)} {pts[i].tolist()} r {float(m.r[i])!r} row {float(m.row[i])!r} col {float(m.col[i])!r} -> "
                    f"pixel {int(m.pixel[i])}")
        lines.append(f"pixel ({int(p // m.w)}, {int(p % m.w)}) = {int(p)}: got {who(index[p])}; the model has {who(want[p])}")
    return int((index != want).sum()), lines


def check_map(index, vmap, rows, m, pts, what=""):
    """index map, vertex map and rows (each may be None) against the model, bit for bit, outside the pixels of flagged rows;
    returns the number of pixels compared"""
    skip = excluded_pixels(m)
    if index is not None:
        index = np.asarray(index)
        assert index.dtype == np.int32 and index.shape == (m.h, m.w), (what, index.dtype, index.shape)
        bad = (index.reshape(-1) != m.index.reshape(-1)) & ~skip
        if bad.any():
            count, lines = account(np.where(skip, m.index.reshape(-1), index.reshape(-1)), m, pts)
            raise AssertionError(f"{what}: {count} of {m.h * m.w} pixels have another winner than the model\n" + "\n".join(lines))
    if vmap is not None:
        check_bits(np.asarray(vmap), m.vmap, what + ", vertex map", skip.reshape(1, m.h, m.w))
    if rows is not None:
        check_bits(np.asarray(rows), m.rows, what + ", rows", skip[:, None])
    return int((~skip).sum())
