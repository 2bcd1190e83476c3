"""Bit model of the elevation image (`icp_elevation_*`, include/icp_mi355x.h; csrc/elevation.hip), in numpy: vectorised,
operation by operation in the type of the rows, so that the device's arrays can be compared with it bit for bit.

    row = rint(x / pixel + H // 2), column = rint(y / pixel + W // 2)      half to even, float32 or float64 like the rows
    kept iff 0 <= row < H and 0 <= column < W; a kept row with a NaN z is set aside (the one deliberate deviation)
    clipped z = clip(z, z_min, z_max), -0.0 made +0.0; the greatest wins the pixel (flip: the smallest), ties: the highest row
    theta = (clipped z - z_min) / T(z_max - z_min), stored as float32; empty pixels hold float32(z_min)
    colour = table[row of matplotlib's rule on a float32 image]

`build(points, spec, table, variant=...)`: `variant` names one deliberately WRONG reading of the specification (WRONG_VARIANTS);
the CPU tests show that each is caught on a named cloud.  No deliberately wrong kernel exists.

`python tests/elevation_audit.py --record` writes, where the reference checkout is present, the reference's own `build_image`
outputs on the edge clouds to tests/golden/elevation_reference.npz."""
import os
import sys
from dataclasses import dataclass

import numpy as np

WRONG_VARIANTS = ("lowest_index_ties", "half_away", "float64_arith", "raw_z_order", "f32_order", "swap_hw", "le_last_row",
                  "empty_zero", "colour_round", "no_256", "neg_zero_below")
LUT_ROWS, UNDER, OVER, BAD = 259, 256, 257, 258
REF = "/root/reference"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "elevation_reference.npz")


@dataclass(frozen=True)
class Spec:
    height: int = 400
    width: int = 400
    pixel_size: float = 0.4
    z_min: float = 0.0
    z_max: float = 5.0
    flip: bool = False


def colour_rows(theta, variant=None):
    """row of the [259, 3] table for every float32 theta: matplotlib's Colormap.__call__ on a float32 image, N = 256"""
    theta = np.asarray(theta, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        t = theta * np.float32(256)
        if variant != "no_256":
            t = np.where(t == np.float32(256), np.float32(255), t)
        k = (np.rint(t) if variant == "colour_round" else np.trunc(t))
        k = np.where(np.isfinite(k), k, 0).astype(np.int64)
    k = np.where(t < 0, UNDER, np.where(t >= 256, OVER, k))
    return np.where(np.isnan(t), BAD, k)


def random_table(seed=0):
    return np.random.default_rng(seed).integers(0, 256, (LUT_ROWS, 3), dtype=np.uint8)


def _cells(v, pixel, half, dt, variant):
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        q = v / dt(pixel) + dt(half)
        if variant == "half_away":
            return np.where(q >= 0, np.floor(q + dt(0.5)), np.ceil(q - dt(0.5)))
        return np.rint(q)


def build(points, spec, table, keep=None, variant=None):
    """{"rgb" uint8 [H,W,3], "theta" float32 [H,W], "points" float32 [H,W,3], "index" int32 [H,W], "stats" dict} of `points`
    [n,3] float32 or float64 (any other type: float32).  keep: bool [n], rows that exist at all (a frame window)."""
    assert variant is None or variant in WRONG_VARIANTS, variant
    p = np.asarray(points)
    if p.dtype != np.float64:
        p = p.astype(np.float32)
    p = p.reshape(-1, 3)
    stored = p
    dt = p.dtype.type
    if variant == "float64_arith":
        p, dt = p.astype(np.float64), np.float64
    h, w = int(spec.height), int(spec.width)
    table = np.asarray(table, np.uint8).reshape(LUT_ROWS, 3)
    half_h, half_w = (w // 2, h // 2) if variant == "swap_hw" else (h // 2, w // 2)
    fx = _cells(p[:, 0], spec.pixel_size, half_h, dt, variant).astype(np.float64)
    fy = _cells(p[:, 1], spec.pixel_size, half_w, dt, variant).astype(np.float64)
    with np.errstate(invalid="ignore"):
        inside = (fx >= 0) & ((fx <= h) if variant == "le_last_row" else (fx < h)) & (fy >= 0) & (fy < w)
    exists = np.ones(len(p), bool) if keep is None else np.asarray(keep, bool)
    nan_z = np.isnan(p[:, 2])
    ok = exists & inside & ~nan_z
    stats = {"rows_in_image": int(ok.sum()), "rows_outside": int((exists & ~inside).sum()),
             "rows_nan_z": int((exists & inside & nan_z).sum())}
    rows = np.flatnonzero(ok)
    lo, hi = dt(spec.z_min), dt(spec.z_max)
    den = dt(np.float64(spec.z_max) - np.float64(spec.z_min))
    pix = (fx[rows].astype(np.int64) % h) * w + fy[rows].astype(np.int64)
    zc = np.clip(p[rows, 2], lo, hi)
    if variant != "neg_zero_below":
        zc = zc + dt(0)  # -0.0 + 0.0 = +0.0
    rank = p[rows, 2] if variant == "raw_z_order" else zc.astype(np.float32) if variant == "f32_order" else zc
    rank = rank if spec.flip else -rank
    minus = np.signbit(zc) if variant == "neg_zero_below" else np.zeros(len(rows), bool)
    minus = ~minus if spec.flip else minus
    by_row = rows if variant == "lowest_index_ties" else -rows
    order = np.lexsort((by_row, minus, rank, pix))  # pixel, then the winning z first, then the winning row first
    _, first = np.unique(pix[order], return_index=True)
    win = order[first]
    theta = np.full(h * w, 0.0 if variant == "empty_zero" else np.float32(spec.z_min), np.float32)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        theta[pix[win]] = ((zc[win] - lo) / den).astype(np.float32)
    xyz = np.zeros((h * w, 3), np.float32)
    with np.errstate(over="ignore"):
        xyz[pix[win]] = stored[rows[win]].astype(np.float32)
    index = np.full(h * w, -1, np.int32)
    index[pix[win]] = rows[win]
    stats["filled_pixels"] = int(len(win))
    return {"rgb": table[colour_rows(theta, variant)].reshape(h, w, 3), "theta": theta.reshape(h, w), "points": xyz.reshape(h, w, 3),
            "index": index.reshape(h, w), "stats": stats}


def clipped_z(points, spec):
    """the clipped height of every row, in the rows' type (what a tie is decided on)"""
    p = np.asarray(points)
    dt = np.float64 if p.dtype == np.float64 else np.float32
    return np.clip(p.reshape(-1, 3).astype(dt)[:, 2], dt(spec.z_min), dt(spec.z_max)) + dt(0)


class ModelImage:
    """Stands in for `pylidar_slam_amd.engine.ElevationImage` on the CPU (the hook's injected builder)."""

    def __init__(self, spec, table):
        self.spec, self.table, self.out = spec, np.asarray(table, np.uint8), None

    def build(self, points):
        self.out = build(points, self.spec, self.table)

    def build_image(self, points):
        self.build(points)
        return self.out["rgb"], {"points_3D": self.out["points"], "pc_indices": self.out["index"].astype(np.int64)}


# ---- clouds ----------------------------------------------------------------------------------------------------------------
def gaussian_cloud(n, seed, dtype=np.float32, spread=40.0):
    """x and y normal; the heights a shuffled ramp: all distinct and strictly inside (0, 5)"""
    rng = np.random.default_rng(seed)
    p = rng.standard_normal((n, 3)) * spread
    p[:, 2] = rng.permutation(np.linspace(0.01, 4.99, n))
    return p.astype(dtype)


def tied_cloud(n, seed, dtype=np.float32):
    """a third of the rows below z_min = 0, a tenth above z_max = 5: clipped ties in most pixels"""
    rng = np.random.default_rng(seed)
    p = rng.standard_normal((n, 3)) * np.array([30.0, 30.0, 3.0]) + np.array([0.0, 0.0, 1.2])
    return p.astype(dtype)


def boundary_cloud(spec, dtype, ulps=(0, 1, 2, 3)):
    """points on every pixel boundary k + 0.5 of both axes (and a margin beyond the image), with copies 1, 2 and 3 ulp either
    side; z grows with the row so that nothing ties"""
    dt = np.dtype(dtype).type
    out = []
    for extent, half, axis in ((spec.height, spec.height // 2, 0), (spec.width, spec.width // 2, 1)):
        k = np.arange(-2, min(extent, 64) + 2, dtype=np.float64) if extent > 70 else np.arange(-2, extent + 2, dtype=np.float64)
        if extent > 70:
            k = np.concatenate([k, np.arange(extent - 4, extent + 2, dtype=np.float64)])
        v = ((k + 0.5 - half) * spec.pixel_size).astype(dt)
        for u in ulps:
            for side in ((-1, 1) if u else (1,)):
                c = v.copy()
                for _ in range(u):
                    c = np.nextafter(c, dt(side * np.inf))
                pts = np.zeros((len(c), 3), dt)
                pts[:, axis] = c
                out.append(pts)
    p = np.concatenate(out)
    p[:, 2] = np.linspace(0.5, 4.5, len(p)).astype(dt)
    return p


def edge_clouds(dtype=np.float32):
    """name -> (points, Spec): the clouds the wrong readings are caught on and the reference's outputs are recorded for"""
    dt = np.dtype(dtype).type
    odd = Spec(5, 7, 0.4, 0.0, 5.0, False)
    clouds = {}
    clouds["ties"] = (np.array([[0.0, 0.0, 7.0], [0.0, 0.0, 6.0], [0.0, 0.0, 5.0], [0.1, 0.0, 9.0], [0.4, 0.4, -3.0], [0.4, 0.4, -1.0],
                                [0.4, 0.4, 0.0]], dt), odd)
    clouds["boundaries"] = (boundary_cloud(odd, dtype), odd)
    p = np.zeros((10, 3), dt)  # cells -0 (kept), 0, 2, 2, 4, 4, 6, 4, 5 = H and -1
    p[:, 0] = (np.array([-2.5, -1.5, -0.5, 0.5, 1.5, 2.5, 3.5, 2.49, 3.0, -3.0]) * 0.4).astype(dt)
    p[:, 2] = np.linspace(1.0, 4.0, 10).astype(dt)
    clouds["image_edges"] = (p, odd)
    clouds["raw_order"] = (np.array([[0.0, 0.0, 9.0], [0.0, 0.0, 7.0], [0.4, 0.0, -4.0], [0.4, 0.0, -2.0]], dt),
                           Spec(5, 7, 0.4, 0.0, 5.0, False))
    clouds["zeros"] = (np.array([[0.0, 0.0, 0.0], [0.0, 0.0, -0.0], [0.4, 0.0, -0.0], [0.4, 0.0, 0.0]], dt), Spec(5, 7, 0.4, -2.0, 5.0, False))
    clouds["zeros_flipped"] = (clouds["zeros"][0], Spec(5, 7, 0.4, -2.0, 5.0, True))
    clouds["empty_mid"] = (np.array([[0.0, 0.0, 1.0]], dt), Spec(5, 7, 0.4, 0.5, 5.0, False))
    z = np.array([5.0, 6.0, 2.4990234375, 2.5, 2.5009765625, 0.009765625, 4.990234375], dt)  # theta * 256 = 256, .., 127.95, 128, 128.05, 0.5, 255.5
    p = np.zeros((len(z), 3), dt)
    p[:, 1] = ((np.arange(len(z)) - 3) * 0.4).astype(dt)
    p[:, 2] = z
    clouds["colour_steps"] = (p, odd)
    if np.dtype(dtype) == np.float64:
        base = 2.0
        clouds["below_float32"] = (np.array([[0.0, 0.0, base + 3e-9], [0.0, 0.0, base + 2e-9], [0.0, 0.0, base + 1e-9], [0.4, 0.0, base],
                                             [0.4, 0.0, base + 1e-12], [0.4, 0.0, base + 1e-13]], dt), odd)
    else:
        # x / float32(0.4) rounds to a half-way case in float32 that float64 arithmetic does not see
        v = (np.arange(1, 4000, dtype=np.float64) * 0.1).astype(np.float32)
        q32 = v / np.float32(0.4) + np.float32(1000)
        q64 = v.astype(np.float64) / 0.4 + 1000
        pick = np.flatnonzero(np.rint(q32).astype(np.int64) != np.rint(q64).astype(np.int64))
        p = np.zeros((len(pick), 3), dt)
        p[:, 1] = v[pick]
        p[:, 2] = np.linspace(1.0, 4.0, len(pick)).astype(dt)
        clouds["float32_quotients"] = (p, Spec(5, 2001, 0.4, 0.0, 5.0, False))
    return clouds


# ---- the reference's own build_image -----------------------------------------------------------------------------------------
def reference_builder(spec, color_map="jet"):
    """The reference's ElevationImageRegistration (slam/common/registration.py:179-241) with `spec`, built without its
    constructor (cm.get_cmap is gone from matplotlib 3.10) behind a throw-away cv2 module.  Needs the reference checkout and
    oracle/shims on sys.path."""
    import types

    import matplotlib
    names = ("cv2", "slam.common.modules", "slam.common.registration")
    saved = {k: sys.modules.pop(k, None) for k in names}
    sys.modules["cv2"] = types.ModuleType("cv2")
    try:  # fresh copies of the two modules that look at cv2; whatever the process held before is put back
        import slam.common.registration as registration
        cls = registration.ElevationImageRegistration
    finally:
        import slam.common as package
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
                if k != "cv2":
                    setattr(package, k.rsplit(".", 1)[1], v)
    obj = object.__new__(cls)
    obj.H, obj.W, obj.pixel_size = int(spec.height), int(spec.width), spec.pixel_size
    obj.z_min, obj.z_max, obj.flip_axis = spec.z_min, spec.z_max, bool(spec.flip)
    obj.color_map = matplotlib.colormaps[color_map] if isinstance(color_map, str) else color_map
    return obj


def record(path=GOLDEN):
    sys.path[:0] = [os.path.join(ROOT, "oracle", "shims"), REF, os.path.join(ROOT, "pylidar-slam_amd")]
    out = {}
    for dtype in (np.float32, np.float64):
        tag = np.dtype(dtype).name
        for name, (points, spec) in edge_clouds(dtype).items():
            if name == "float32_quotients":
                continue  # (its image is 5 x 2001: reproducible from the model's own arithmetic, too wide for a fixture)
            image, extra = reference_builder(spec).build_image(points.copy())
            key = f"{tag}/{name}"
            out[key + "/points"] = points
            out[key + "/spec"] = np.array([spec.height, spec.width, spec.pixel_size, spec.z_min, spec.z_max, float(spec.flip)])
            out[key + "/rgb"] = image
            out[key + "/points_3D"] = extra["points_3D"]
            out[key + "/pc_indices"] = extra["pc_indices"]
    # the deliberate deviation: a NaN z wins its pixel in the reference and paints it with the bad colour
    spec = Spec(5, 7, 0.4, 0.0, 5.0, False)
    points = np.array([[0.0, 0.0, 4.0], [0.0, 0.0, np.nan], [0.4, 0.0, 1.0]], np.float32)
    image, extra = reference_builder(spec).build_image(points.copy())
    out["nan_z/points"], out["nan_z/rgb"], out["nan_z/pc_indices"] = points, image, extra["pc_indices"]
    np.savez_compressed(path, **out)
    return path


if __name__ == "__main__":
    if "--record" in sys.argv:
        if not os.path.isdir(os.path.join(REF, "slam")):
            sys.exit("the reference checkout is not present")
        print("wrote", record())
