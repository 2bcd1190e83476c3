"""The model of the kNN map normals (tests/normals_audit.py) held to float64 and to the reference's own arithmetic, the wrong
copies it must tell apart, and the oracle-backed context held to it.  CPU only.

Measured here (numpy, the clouds of normals_audit.clouds(), k = 5, 10, 20, 1, 2, 3, 7, 12, 32, 64), ratio = sin(angle) * gap /
2^-24 over the determined points (gap > 1e-6, an unambiguous neighbour set):
    the model against float64 eigh:                   worst 3.14 (offset cloud, k = 32: the generic float32 sums), 2.63 for
                                                      k = 5, 10, 20 (offset cloud, k = 20)
    the reference's float32 SVD against float64:      worst 2.40 (offset cloud, k = 32)
    the model against the reference's float32 SVD:    worst 2.83 (offset cloud, k = 20)
    flagged / order-dependent points:                 0 / 0 on every cloud and k
BAR = 4 x 3.14 (normals_audit.MEASURED_WORST).

The wrong copies, points moved (of the compared ones) at k = 10 / 7 / 1 — a copy that moves no point of a cloud computes the
model's own normals there, so there is nothing to catch; every copy is caught on at least one cloud:
                        LiDAR 8 192           lattice 6 912        duplicates 4 889    why a zero
    kth_is_next         8192 / 8192 / 8192    6872 / 6692 / 554    227 / 90 / 34
    first_kept          8192 / 8192 / 8192    6872 / 6472 / 12     752 / 366 / 11
    ties_higher            0 /    0 /    0    2024 / 2064 / 24       0 /  0 /  0       no two distances of the LiDAR map tie in the
                                                                                       k + 1-th place; twins tie whole lists
    mean_centred        8192 (k = 10)         2072 (k = 10)        1005 (k = 10)
    other_sums          6422 / 6082 / 749        0 /    0 /   0     263 / 51 /  0      the lattice's products and sums are exact
                                                                                       in float32 as on the grid
    seven_sweeps           0 /    0 /   65       0 /    0 /   0      22 /  0 /  0      no such neighbourhood still rotates in its
                                                                                       8th sweep (at most 4 are taken)
    ties_first_axis        0 /    0 /   56    4840 /    0 / 6912   3964 / 4422 / 4878  no two eigenvalues are equal
    divisor_k           a 10-point map at k = 10: all 10 points; a 4-point map: 3 / 4 / 0 at k = 10 / 7 / 1; 0 on every map of
                        k + 1 points or more.  The stop does NOT move (the sweeps taken are the same): float32(sum) * (1 / k) and
                        * (1 / used) round differently, and the unit-trace scaling, itself rounded, does not undo it.
"""
import numpy as np
import pytest

import knn_audit as KA
import normals_audit as N

ALL_KS = N.GRID_KS + N.GENERIC_KS


@pytest.fixture(scope="module")
def O():
    import icp_oracle
    return icp_oracle


def test_launch_shapes_come_from_the_source():
    s = N.launch_shapes()
    assert s["four_lanes"] == 64 and s["pair"] == 64 and s["two_lanes"] == 128 and s["tail16_rows"] == 16
    assert s["generic_threads"] == 128 and s["worklist_blocks_max"] == 4096 and s["generic_kmax"] == max(ALL_KS) + 1
    for edge in (s["four_lanes"], s["two_lanes"], s["pair"], 1024):
        assert {edge - 1, edge, edge + 1} <= set(N.EDGE_SIZES)


@pytest.mark.parametrize("name", list(N.clouds()))
def test_model_against_float64_and_the_reference(O, name):
    """On every determined point the model stays within BAR * 2^-24 / gap of float64 eigh, and so does the reference's float32
    SVD on the same neighbourhoods; the two within the same bar of each other.  Caps: nothing flagged beyond FLAGGED_MAX.  Every
    normal finite and of unit length to float32 rounding."""
    from scipy.spatial import cKDTree
    cloud = N.clouds()[name]
    tree = cKDTree(cloud.astype(np.float64))
    worst = [0.0, 0.0, 0.0]
    for k in ALL_KS:
        want = N.model(name, cloud, k)
        f, d = N.check_caps(want, name)
        assert np.isfinite(want.normals).all(), (name, k)
        assert np.abs(np.linalg.norm(want.normals.astype(np.float64), axis=1) - 1.0).max() < 3 * N.U24 * 2, (name, k)
        assert np.array_equal(want.used, np.full(cloud.shape[0], min(k, cloud.shape[0] - 1)))
        truth = N.truth(name, cloud, k)
        rows = np.flatnonzero(truth[2] & ~want.left_out)
        r_model, count = N.truth_ratio(want.normals, truth, rows)
        r_ref = r_both = 0.0
        if count:
            ref = O.knn_normals(cloud, tree, rows, k=k)
            full = np.zeros_like(want.normals)
            full[rows] = ref
            r_ref, _ = N.truth_ratio(full, truth, rows)
            r_both = float((N.sin_angle(want.normals[rows], ref) * truth[1][rows] / N.U24).max())
        print(f"{name} k {k}: {count} of {cloud.shape[0]} determined, flagged {f}, order-dependent {d}, ratio to float64: model "
              f"{r_model:.2f}, reference {r_ref:.2f}; model to reference {r_both:.2f}")
        assert f == 0 and d == 0, (name, k, f, d)   # (measured; the cap itself is check_caps')
        assert r_model <= N.BAR and r_ref <= N.BAR and r_both <= N.BAR, (name, k, r_model, r_ref, r_both)
        worst = [max(a, b) for a, b in zip(worst, (r_model, r_ref, r_both))]
    # BAR is four times a MEASURED spread: the figure in normals_audit must be the one these clouds give
    assert worst[0] <= N.MEASURED_WORST, (name, worst)
    if name == "plane":
        assert worst[0] == 0.0   # z = 0 exactly: every product with dz is 0, the normal is (0, 0, +-1) in every arithmetic
    if name == "offset":
        assert worst[0] > N.MEASURED_WORST - 0.01, worst   # (the cloud that sets the figure)


def test_degenerate_maps_have_their_expected_normals():
    """M = 1: zero covariance, (0, 0, 1).  All points equal: the same.  M = 2: the rank-1 matrix of the pair.  A line: finite
    unit normals orthogonal to it (the model alone defines WHICH).  The values are the same for every k."""
    for k in (5, 10, 20, 3, 64):
        one = N.model_normals(np.array([[3.0, -2.0, 7.0]], N.F32), k)
        assert one.normals.tolist() == [[0.0, 0.0, 1.0]] and one.used.tolist() == [0] and not one.cov.any()
        same = N.model_normals(np.tile(np.array([[3.0, -2.0, 7.0]], N.F32), (30, 1)), k)
        assert np.array_equal(same.normals, np.tile(np.array([[0, 0, 1]], N.F32), (30, 1))) and not same.cov.any()
        assert same.neighbours[0, 0] == 1 and same.neighbours[5, 0] == 1 and same.neighbours[1, 0] == 1  # (index 0 is dropped, by everyone)
        pair = N.model_normals(N.tiny_maps(k)["m2"], k)
        assert pair.used.tolist() == [1, 1]
        assert np.array_equal(pair.normals[0], np.array(N.PAIR_EXPECTED, N.F32)), pair.normals[0].tolist()
        assert np.array_equal(pair.normals[1], pair.normals[0])   # (d and -d: the same matrix)
        line = N.clouds()["line"]
        got = N.model("line", line, k)
        assert np.isfinite(got.normals).all()
        # the stored points are off the line by half a float32 step per coordinate (|p| < 32: e = sqrt(3) * 2^-20 per point, twice
        # that on a difference); the direction of largest spread of k such differences, the farthest of length r, is within
        # sqrt(k) * 2 e / r of the line, and the normal is orthogonal to it up to the sweep's own rounding
        along = np.array([30.0, 12.0, 3.0]) / np.linalg.norm([30.0, 12.0, 3.0])
        kk = min(k, line.shape[0] - 1)
        r = np.linalg.norm(line[got.neighbours[:, kk - 1]].astype(np.float64) - line, axis=1)
        tol = np.sqrt(kk) * 2 * np.sqrt(3.0) * 2.0 ** -20 / r + 8 * N.U24
        assert (np.abs(got.normals.astype(np.float64) @ along) <= tol).all()


def test_fma_emulation_settles_the_middles():
    """theta with a short mantissa and theta^2 >> 1: theta^2 is exactly the middle between two float32 values, the 1 decides
    (upwards), and float64 drops it.  fma_sq1 settles it; what is left uncertain is nothing."""
    a = np.array([762490900000.0, -7.872503e16, 538574850.0, 3.0, 0.0, 2.0 ** -12, np.inf], N.F32)
    r, unsure = N.fma_sq1(a)
    assert not unsure.any()
    from fractions import Fraction
    for x, got in zip(a[:6], r[:6]):
        exact = Fraction(float(x)) ** 2 + 1
        lo, hi = np.nextafter(got, N.F32(-np.inf)), np.nextafter(got, N.F32(np.inf))
        assert abs(Fraction(float(got)) - exact) <= min(abs(Fraction(float(lo)) - exact), abs(Fraction(float(hi)) - exact))
    assert r[0] > N.F32(float(a[0]) ** 2) and np.isinf(r[6])   # (the naive float64 route rounds the first one to even: down)


# the table of the module docstring: {copy: {cloud: {k: points moved}}}
_MOVED = {
    "kth_is_next": {"lidar": {10: 8192, 7: 8192, 1: 8192}, "lattice": {10: 6872, 7: 6692, 1: 554}, "duplicates": {10: 227, 7: 90, 1: 34}},
    "first_kept": {"lidar": {10: 8192, 7: 8192, 1: 8192}, "lattice": {10: 6872, 7: 6472, 1: 12}, "duplicates": {10: 752, 7: 366, 1: 11}},
    "ties_higher": {"lidar": {10: 0, 7: 0, 1: 0}, "lattice": {10: 2024, 7: 2064, 1: 24}, "duplicates": {10: 0, 7: 0, 1: 0}},
    "mean_centred": {"lidar": {10: 8192}, "lattice": {10: 2072}, "duplicates": {10: 1005}},
    "other_sums": {"lidar": {10: 6422, 7: 6082, 1: 749}, "lattice": {10: 0, 7: 0, 1: 0}, "duplicates": {10: 263, 7: 51, 1: 0}},
    "seven_sweeps": {"lidar": {10: 0, 7: 0, 1: 65}, "lattice": {10: 0, 7: 0, 1: 0}, "duplicates": {10: 22, 7: 0, 1: 0}},
    "ties_first_axis": {"lidar": {10: 0, 7: 0, 1: 56}, "lattice": {10: 4840, 7: 0, 1: 6912}, "duplicates": {10: 3964, 7: 4422, 1: 4878}},
}
_LISTS = {}


def _lists(name, cloud, ks):
    if name not in _LISTS:
        _LISTS[name] = N.neighbour_lists(cloud, ks, extra=1)
    return _LISTS[name]


@pytest.mark.parametrize("copy", list(_MOVED))
def test_wrong_copies_are_caught(copy):
    """Each wrong copy of the model is caught by check_bits on every cloud on which it moves a point, the LiDAR cloud or the
    lattice among them, and moves exactly the recorded number of points."""
    ks = (10, 7, 1)
    caught = set()
    for name, per_k in _MOVED[copy].items():
        cloud = N.clouds()[name]
        lists = _lists(name, cloud, ks)
        got = N.model_normals_multi(cloud, tuple(per_k), copy, lists=lists)
        for k, moved in per_k.items():
            right = N.model(name, cloud, k)
            bad, compared = N.differing(got[k].normals, right)
            print(f"{copy} on {name}, k {k}: moves {bad.size} of {compared} points")
            assert bad.size == moved, (copy, name, k, bad.size, moved)
            if moved:
                with pytest.raises(AssertionError, match="differ from the model"):
                    N.check_bits(got[k].normals, right, what=f"{copy} {name}")
                caught.add(name)
            else:
                assert N.check_bits(got[k].normals, right) == compared
    assert caught & {"lidar", "lattice"}, (copy, caught)


def test_wrong_divisor_is_caught_on_a_map_smaller_than_k_plus_1():
    """`k` where `used` belongs: the same matrix up to a factor — and other bits, because float32(sum) * (1 / 10) and
    * (1 / 9) round differently and the rounded unit-trace scaling does not undo that.  The 1e-9 stop does not move: the sweeps
    taken are the same.  On a map of k + 1 points or more the copy IS the model."""
    for name, ks, moved in (("m10", (10, 7, 1), (10, 0, 0)), ("m4", (10, 7, 1), (3, 4, 0))):
        cloud = N.tiny_maps(10)[name] if name == "m10" else np.ascontiguousarray(N.lidar()[::37][:4])
        right = N.model_normals_multi(cloud, ks)
        wrong = N.model_normals_multi(cloud, ks, "divisor_k")
        for k, want in zip(ks, moved):
            bad, compared = N.differing(wrong[k].normals, right[k])
            print(f"divisor_k on {name}, k {k}: moves {bad.size} of {compared} points")
            assert bad.size == want and np.array_equal(wrong[k].sweeps, right[k].sweeps), (name, k, bad.size)
            if want:
                with pytest.raises(AssertionError, match="differ from the model"):
                    N.check_bits(wrong[k].normals, right[k])
                # the same line to float32 rounding: the divisor cancels in the eigenvector
                assert N.sin_angle(wrong[k].normals, right[k].normals).max() < 1e-5
    cloud = N.tiny_maps(10)["m11"]
    assert np.array_equal(N.model_normals(cloud, 10, "divisor_k").normals, N.model_normals(cloud, 10).normals)


def test_check_bits_reports_the_point_and_respects_rows():
    cloud = N.clouds()["isolated"]
    want = N.model("isolated", cloud, 10)
    got = want.normals.copy()
    got[17, 1] = np.nextafter(got[17, 1], N.F32(2.0))
    with pytest.raises(AssertionError, match=r"first point 17: .* neighbours \[.*covariance \["):
        N.check_bits(got, want, what="one ulp")
    assert N.check_bits(got, want, rows=np.array([3, 16, 18])) == 3
    assert N.check_bits(-want.normals, want, rows=np.zeros(0, np.int64)) == 0
    with pytest.raises(AssertionError):
        N.check_bits(-want.normals, want)            # (the sign is part of the bits)


@pytest.mark.parametrize("k", [5, 10, 20])
def test_oracle_context_normals_stand_on_the_model(k):
    """tests/oracle_context.py keeps its own normals (the oracle's restatement of the reference: float64 kd-tree, float32 SVD);
    on every determined point they lie within the float64 bar of the truth and of the model — the CPU loop tests and the GPU
    stand on one answer."""
    from oracle_context import OracleContext
    cloud = np.ascontiguousarray(N.lidar()[:2048])
    ctx = OracleContext(num_neighbors_normals=k)
    ctx.map_set(cloud)
    _, normals, ix = ctx.nearest_neighbor_search(cloud, with_index=True)
    assert np.array_equal(ix, np.arange(cloud.shape[0]))
    want = N.model("edge2048", cloud, k)
    truth = N.truth("edge2048", cloud, k)
    rows = np.flatnonzero(truth[2] & ~want.left_out)
    assert rows.size > 0.99 * cloud.shape[0]
    r_truth, _ = N.truth_ratio(normals, truth, rows)
    r_model = float((N.sin_angle(normals[rows], want.normals[rows]) * truth[1][rows] / N.U24).max())
    print(f"oracle context, k {k}: {rows.size} points, ratio to float64 {r_truth:.2f}, to the model {r_model:.2f}")
    assert r_truth <= N.BAR and r_model <= N.BAR, (r_truth, r_model)


def test_edge_maps_stay_unflagged():
    """the maps at the workgroup edges and the tiny maps the GPU audit uses: nothing flagged, every normal finite"""
    for name, cloud in N.edge_maps().items():
        if cloud.shape[0] > 129:
            continue                                  # (the larger ones are modelled by the GPU audit alone: seconds each)
        for k in (5, 10, 20, 7, 64):
            want = N.model(name, cloud, k)
            assert N.check_caps(want, name) == (0, 0) and np.isfinite(want.normals).all()
    for k in ALL_KS:
        for name, cloud in N.tiny_maps(k).items():
            want = N.model_normals(cloud, k)
            assert N.check_caps(want, name) == (0, 0) and np.isfinite(want.normals).all(), (name, k)
            assert np.array_equal(want.used, np.full(cloud.shape[0], min(k, cloud.shape[0] - 1)))
    assert KA.FLAGGED_MAX == N.FLAGGED_MAX == 1.0e-3
