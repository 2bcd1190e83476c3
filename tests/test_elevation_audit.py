"""CPU: the bit model the elevation image is held to (tests/elevation_audit.py) against the reference's own `build_image`
(slam/common/registration.py:196-241, imported from /root/reference through oracle/shims behind a throw-away cv2 module; those
tests are skipped where that checkout is absent, the GPU box), against matplotlib's colour rule, against the reference's
recorded outputs (tests/golden/elevation_reference.npz), against eleven deliberately wrong readings of the specification —
each caught on a named cloud — and the hook that hands the reference's class a device-backed `build_image`."""
import os
import sys
import types

import numpy as np
import pytest

import elevation_audit as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_reference = pytest.mark.skipif(not os.path.isdir(os.path.join(A.REF, "slam")), reason="reference checkout not present")
DTYPES = [np.float32, np.float64]
SHAPES = [(400, 400), (5, 7), (1, 300)]


@pytest.fixture()
def reference_on_path():
    import logging
    logging.disable(logging.WARNING)
    added = [os.path.join(ROOT, "oracle", "shims"), A.REF]
    sys.path[:0] = added
    yield
    for p in added:
        sys.path.remove(p)
    logging.disable(logging.NOTSET)


@pytest.fixture(scope="module")
def jet():
    pytest.importorskip("matplotlib")
    from pylidar_slam_amd.engine import colormap_table
    return colormap_table("jet")


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _spec(shape, **kw):
    pixel = {(400, 400): 0.4, (5, 7): 20.0, (1, 300): 0.4}[shape]
    return A.Spec(shape[0], shape[1], pixel, kw.get("z_min", 0.0), kw.get("z_max", 5.0), kw.get("flip", False))


# ---- the model against the reference's own function ------------------------------------------------------------------------
@needs_reference
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("flip", [False, True])
def test_model_equals_the_reference_where_no_height_ties(reference_on_path, jet, shape, dtype, flip):
    """all z distinct and strictly inside the clip range: colour, points_3D and pc_indices on every pixel"""
    cloud = A.gaussian_cloud(60000, 7, dtype)
    z = cloud[:, 2]
    assert len(np.unique(z)) == len(z) and z.min() > 0.0 and z.max() < 5.0
    spec = _spec(shape, flip=flip)
    image, extra = A.reference_builder(spec).build_image(cloud.copy())
    want = A.build(cloud, spec, jet)
    assert image.dtype == np.uint8 and np.array_equal(image, want["rgb"])
    assert extra["pc_indices"].dtype == np.int64 and np.array_equal(extra["pc_indices"], want["index"])
    assert extra["points_3D"].dtype == np.float32 and np.array_equal(_bits(extra["points_3D"]), _bits(want["points"]))
    filled = want["stats"]["filled_pixels"]
    assert filled == int((want["index"] >= 0).sum()) and (filled >= 100 or filled == shape[0] * shape[1])


@needs_reference
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("z_min", [-2.0, 0.0, 0.5])
@pytest.mark.parametrize("flip", [False, True])
def test_model_equals_the_reference_up_to_the_winner_of_a_tie(reference_on_path, jet, z_min, dtype, flip):
    """clipped ties: the colour image is equal on EVERY pixel; where the index differs the two rows have the same clipped z"""
    cloud = A.tied_cloud(200000, 11, dtype)
    spec = A.Spec(400, 400, 0.4, z_min, 5.0, flip)
    image, extra = A.reference_builder(spec).build_image(cloud.copy())
    want = A.build(cloud, spec, jet)
    assert np.array_equal(image, want["rgb"])
    ref_index = extra["pc_indices"]
    assert np.array_equal(ref_index >= 0, want["index"] >= 0)
    differ = np.flatnonzero((ref_index != want["index"]).reshape(-1))
    zc = A.clipped_z(cloud, spec)
    mine, theirs = want["index"].reshape(-1)[differ], ref_index.reshape(-1)[differ]
    assert np.array_equal(_bits(zc[mine]), _bits(zc[theirs]))
    assert np.all(mine > theirs)  # the model's winner is the highest row of the tie
    same = np.flatnonzero((ref_index == want["index"]).reshape(-1))
    assert np.array_equal(_bits(extra["points_3D"].reshape(-1, 3)[same]), _bits(want["points"].reshape(-1, 3)[same]))
    ties = int(((zc == np.float32(z_min)) | (zc == 5.0)).sum())
    assert ties > 10000 and len(differ) > 100


@needs_reference
def test_recorded_reference_outputs_are_what_the_reference_gives_and_what_the_model_gives(reference_on_path, jet):
    """tests/golden/elevation_reference.npz (written by `elevation_audit.py --record`): still the reference's outputs; the
    model's wherever no tie decides; and the deliberate deviation: a NaN z wins its pixel there and is set aside here"""
    gold = np.load(A.GOLDEN)
    seen = 0
    for dtype in DTYPES:
        tag = np.dtype(dtype).name
        for name, (points, spec) in A.edge_clouds(dtype).items():
            key = f"{tag}/{name}"
            if key + "/rgb" not in gold.files:
                continue
            seen += 1
            assert np.array_equal(_bits(gold[key + "/points"]), _bits(points)), key
            image, extra = A.reference_builder(spec).build_image(points.copy())
            assert np.array_equal(image, gold[key + "/rgb"]) and np.array_equal(_bits(extra["points_3D"]), _bits(gold[key + "/points_3D"])), key
            want = A.build(points, spec, jet)
            assert np.array_equal(gold[key + "/rgb"], want["rgb"]), key
            if name not in ("ties", "raw_order", "zeros", "zeros_flipped", "colour_steps"):  # (clouds with ties: the winner is the model's rule)
                assert np.array_equal(gold[key + "/pc_indices"], want["index"]), key
                assert np.array_equal(_bits(gold[key + "/points_3D"]), _bits(want["points"])), key
    assert seen >= 16
    points = gold["nan_z/points"]
    assert gold["nan_z/pc_indices"][2, 3] == 1 and tuple(gold["nan_z/rgb"][2, 3]) == tuple(jet[A.BAD])
    want = A.build(points, A.Spec(5, 7, 0.4, 0.0, 5.0, False), jet)
    assert want["index"][2, 3] == 0 and want["stats"]["rows_nan_z"] == 1 and want["stats"]["rows_in_image"] == 2


def test_recorded_fixture_agrees_with_the_model_without_the_reference(jet):
    """the same fixture on a machine without the checkout: colour everywhere, the rows wherever no tie decides"""
    gold = np.load(A.GOLDEN)
    for key in sorted(k[:-4] for k in gold.files if k.endswith("/rgb") and k.count("/") == 2):
        h, w, pixel, lo, hi, flip = gold[key + "/spec"]
        spec = A.Spec(int(h), int(w), float(pixel), float(lo), float(hi), bool(flip))
        want = A.build(gold[key + "/points"], spec, jet)
        assert np.array_equal(gold[key + "/rgb"], want["rgb"]), key
        differ = np.flatnonzero((gold[key + "/pc_indices"] != want["index"]).reshape(-1))
        zc = A.clipped_z(gold[key + "/points"], spec)
        assert np.array_equal(zc[want["index"].reshape(-1)[differ]], zc[gold[key + "/pc_indices"].reshape(-1)[differ]]), key


# ---- colour ----------------------------------------------------------------------------------------------------------------
def test_colour_rule_against_matplotlib_on_jet_and_on_random_bytes():
    matplotlib = pytest.importorskip("matplotlib")
    from matplotlib.colors import ListedColormap
    from pylidar_slam_amd.engine import colormap_table
    rng = np.random.default_rng(2)
    one = np.float32(1)
    theta = np.concatenate([rng.uniform(-0.5, 1.5, 20000).astype(np.float32), np.linspace(0, 1, 4097, dtype=np.float32),
                            np.array([0.0, -0.0, 1.0, np.nextafter(one, np.float32(0)), np.nextafter(one, np.float32(2)), np.nan, np.inf,
                                      -np.inf, 1e38, 3e38, -1e-45, 1e-45, 0.5, -2.0], np.float32)]).reshape(-1, 3)
    noise = ListedColormap(rng.integers(0, 256, (256, 3)) / 255.0, name="noise")
    noise.set_under((0.2, 0.4, 0.6))
    noise.set_over((0.9, 0.1, 0.3))
    noise.set_bad((0.5, 0.7, 0.1))
    for cmap in (matplotlib.colormaps["jet"], noise):
        table = colormap_table(cmap)
        with np.errstate(invalid="ignore", over="ignore"):
            theirs = (cmap(theta.copy())[:, :, :3] * 255.0).astype(np.uint8)  # slam/common/registration.py:229-230
        assert np.array_equal(table[A.colour_rows(theta)], theirs), cmap.name
    rows = A.colour_rows(theta)
    assert {A.UNDER, A.OVER, A.BAD, 0, 255}.issubset(set(rows.reshape(-1).tolist()))
    table = colormap_table(noise)
    assert len({tuple(table[A.UNDER]), tuple(table[A.OVER]), tuple(table[A.BAD]), tuple(table[255]), tuple(table[0])}) == 5
    jet = colormap_table("jet")
    assert tuple(jet[A.OVER]) == tuple(jet[255])  # why jet alone would hide an over / no-256 mistake


# ---- deliberately wrong copies ---------------------------------------------------------------------------------------------
CAUGHT_ON = {"lowest_index_ties": ("ties", "index"), "half_away": ("boundaries", "index"), "float64_arith": ("float32_quotients", "index"),
             "raw_z_order": ("raw_order", "index"), "f32_order": ("below_float32", "index"), "swap_hw": ("boundaries", "index"),
             "le_last_row": ("image_edges", "index"), "empty_zero": ("empty_mid", "rgb"), "colour_round": ("colour_steps", "rgb"),
             "no_256": ("colour_steps", "rgb"), "neg_zero_below": ("zeros", "index")}


@pytest.mark.parametrize("variant", A.WRONG_VARIANTS)
def test_every_wrong_reading_is_caught_on_its_cloud(variant):
    name, array = CAUGHT_ON[variant]
    dtype = np.float64 if name == "below_float32" else np.float32
    points, spec = A.edge_clouds(dtype)[name]
    table = A.random_table(1)
    right, wrong = A.build(points, spec, table), A.build(points, spec, table, variant=variant)
    assert not np.array_equal(right[array], wrong[array]), (variant, name)
    if variant == "neg_zero_below":
        flipped = A.edge_clouds(dtype)["zeros_flipped"]
        assert not np.array_equal(A.build(*flipped, table)["index"], A.build(*flipped, table, variant=variant)["index"])
    if variant == "float64_arith":
        assert len(points) >= 1
    # and is no other reading of a cloud well inside the image, without ties: the variants differ only where they are meant to
    calm = A.gaussian_cloud(3000, 5, dtype, spread=4.0)
    calm_spec = A.Spec(64, 64, 1.0, 0.0, 5.0, False)
    if variant not in ("half_away", "float64_arith", "swap_hw", "colour_round", "f32_order"):
        assert all(np.array_equal(a, b) for a, b in zip(list(A.build(calm, calm_spec, table).values())[:4],
                                                         list(A.build(calm, calm_spec, table, variant=variant).values())[:4])), variant


def test_catalogue_of_wrong_readings_is_complete():
    assert set(CAUGHT_ON) == set(A.WRONG_VARIANTS) and len(A.WRONG_VARIANTS) == 11
    for dtype in DTYPES:
        for name, (points, spec) in A.edge_clouds(dtype).items():
            assert points.dtype == dtype and points.ndim == 2 and points.shape[1] == 3 and len(points) >= 1, name


# ---- the hook --------------------------------------------------------------------------------------------------------------
def test_install_elevation_image_routes_build_image_through_a_per_instance_builder(monkeypatch):
    from pylidar_slam_amd import register
    made = []

    class ElevationImageRegistration:  # the stubbed class: the attributes the reference's constructor sets (:185-194)
        def __init__(self, h, w, flip=False):
            self.H, self.W, self.pixel_size, self.z_min, self.z_max, self.flip_axis, self.color_map = h, w, 0.4, 0.0, 5.0, flip, "noise"

        def build_image(self, pc):
            raise AssertionError("the reference's own build_image ran")

    def factory(owner):
        made.append(owner)
        return A.ModelImage(A.Spec(owner.H, owner.W, owner.pixel_size, owner.z_min, owner.z_max, owner.flip_axis), A.random_table(4))

    slam, common = types.ModuleType("slam"), types.ModuleType("slam.common")
    registration = types.ModuleType("slam.common.registration")
    slam.common, common.registration = common, registration
    slam.__path__, common.__path__ = [], []
    for name, mod in (("slam", slam), ("slam.common", common), ("slam.common.registration", registration)):
        monkeypatch.setitem(sys.modules, name, mod)
    assert register.install_elevation_image(factory) is None  # no cv2: the reference does not define the class
    registration.ElevationImageRegistration = ElevationImageRegistration
    assert register.install_elevation_image(factory) is ElevationImageRegistration
    a, b = ElevationImageRegistration(5, 7), ElevationImageRegistration(40, 30, flip=True)
    cloud = A.tied_cloud(500, 3)
    cloud[:, :2] *= 0.05
    for obj in (a, b, a):
        image, extra = obj.build_image(cloud)
        want = A.build(cloud, A.Spec(obj.H, obj.W, 0.4, 0.0, 5.0, obj.flip_axis), A.random_table(4))
        assert np.array_equal(image, want["rgb"]) and np.array_equal(extra["pc_indices"], want["index"]) and extra["pc_indices"].dtype == np.int64
        assert np.array_equal(_bits(extra["points_3D"]), _bits(want["points"]))
    assert made == [a, b]  # one builder per instance, kept
    a.z_max = 4.0  # a setting changes: the builder is made again
    image, _ = a.build_image(cloud)
    assert made == [a, b, a] and np.array_equal(image, A.build(cloud, A.Spec(5, 7, 0.4, 0.0, 4.0, False), A.random_table(4))["rgb"])
