"""CPU side of the preprocessing audit (tests/preprocess_audit.py): the model equals the oracle on every case, the committed
recordings of the reference (components.npz, voxelization.npz, distortion.npz and preprocess_edges.npz, the reference's own
answer on the edge cases), every case is what it claims to be, and each deliberately wrong copy of the model fails by its
own named check and no other.  No GPU, no torch.  tests/test_gpu_preprocess_audit.py runs the same cases on the device."""
import hashlib
import os

import numpy as np
import pytest

import icp_oracle as O
import preprocess_audit as P
from conftest import GOLDEN

F32, F64, I64 = np.float32, np.float64, np.int64


@pytest.fixture(scope="module")
def small():
    return P.small_cases()


@pytest.fixture(scope="module")
def large():
    """The cases of 32 768 rows and more, built once."""
    out = [P.bucket_full_case()] + P.exact_switch_cases()
    for kind in ("clustered", "full"):
        out.append(P.repeated_case(P.PADDED_BUCKET_MAX_N, 9000, kind))
        out.extend(P.repeated_case(P.PADDED_BUCKET_MAX_N + 1, v, kind) for v in P.SORT_EMIT_V + (9000,))
    return out


@pytest.fixture(scope="module")
def edges():
    return np.load(os.path.join(GOLDEN, "preprocess_edges.npz"))


def _exact_out(model, indices=None):
    idx = model.indices if indices is None else np.asarray(indices, I64)
    return {"indices": idx, "points": model.points[idx]}


def _padded_out(model):
    pts, idx, count = model.padded()
    return {"indices": idx, "points": pts, "count": count}


# ----------------------------------------------------------------------------------------------------------------------
# the model against the oracle and the recordings
# ----------------------------------------------------------------------------------------------------------------------
def test_model_equals_the_oracle_on_every_case(small, large):
    for c in small + large:
        m = c.model
        assert np.array_equal(O.voxelise(c.points, c.voxel), m.voxels), c
        assert np.array_equal(O.voxel_hashing(m.voxels), m.hashes), c
        pts, idx = O.grid_sample(c.points, c.voxel)
        assert np.array_equal(idx, m.indices) and P.same_bits(pts, c.points[m.indices]), c
        assert P.check_sample(_exact_out(m), m) == [] and P.check_sample(_padded_out(m), m) == [], c
        assert P.check_hash({"voxels": m.voxels, "hashes": m.hashes}, m) == [], c


def test_statistics_model_against_the_oracle(small):
    """The oracle sums pairwise (numpy.sum), the model one member after the other like the kernel: integers exactly, the
    float32 sums at the bars of test_voxelization_filter."""
    for c in small:
        if c.f64:
            continue
        m = c.model
        sizes, means, covs = P.voxel_stats_model(c.points, m)
        osz, omeans, ocovs, oids = O.voxel_normal_distribution(c.points, m.hashes)
        assert np.array_equal(osz, sizes) and np.array_equal(oids, m.ids), c
        np.testing.assert_allclose(means, omeans, rtol=1e-6, atol=1e-5, err_msg=c.name)
        np.testing.assert_allclose(covs, ocovs, rtol=1e-4, atol=1e-5, err_msg=c.name)
        assert P.check_stats({"ids": m.ids, "count": m.count, "sizes": sizes, "means": means, "covs": covs}, m,
                             (sizes, means, covs)) == []


def test_model_equals_the_existing_goldens(golden_components):
    g = golden_components
    m = P.SampleModel(g["gs_pc"], float(g["gs_voxel"]))
    assert np.array_equal(m.voxels, g["gs_voxels"]) and np.array_equal(m.hashes, g["gs_hashes"])
    assert np.array_equal(m.indices, g["gs_indices"])
    v = np.load(os.path.join(GOLDEN, "voxelization.npz"))
    for name in ("v02", "v10"):
        m = P.SampleModel(v["pc"], float(v[f"{name}_size"]))
        sizes, means, covs = P.voxel_stats_model(v["pc"], m)
        assert np.array_equal(m.voxels, v[f"{name}_voxel_coordinates"]) and np.array_equal(m.hashes, v[f"{name}_voxel_hashes"])
        assert np.array_equal(m.ids, v[f"{name}_voxel_indices"]) and np.array_equal(sizes, v[f"{name}_voxel_sizes"])
        np.testing.assert_allclose(means, v[f"{name}_voxel_means"], rtol=1e-6, atol=1e-5)
        np.testing.assert_allclose(covs, v[f"{name}_voxel_covariances"], rtol=1e-4, atol=1e-5)
    d = np.load(os.path.join(GOLDEN, "distortion.npz"))
    for name in ("small", "large", "identity", "pure_translation"):
        out = P.deskew_model(d["pc"], d["timestamps"], d[f"{name}_rpose"])
        np.testing.assert_allclose(out, d[f"{name}_distorted"], rtol=0, atol=1e-11)
        assert np.array_equal(P.SampleModel(out, 0.3).indices, d[f"{name}_sample_indices"])
    np.testing.assert_allclose(P.deskew_model(d["pc"], np.full(d["pc"].shape[0], 3.0), d["small_rpose"]),
                               d["constant_ts_distorted"], rtol=0, atol=1e-11)


def _sha(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()


def test_model_equals_the_reference_on_the_edge_cases(edges):
    """tests/golden/preprocess_edges.npz: the reference's own voxelise / voxel_hashing / sample_from_hashes /
    voxel_normal_distribution on the ties, the collisions, the sentinel voxel and the wrapping hashes — integers exactly, the
    statistics at the bars of test_voxelization_filter (the reference's argsort is not stable)."""
    cases = {c.name: c for c in P.tie_cases() + [P.collision_case()] + P.sentinel_cases() + [P.wrap_case()]}
    assert sorted(cases) == sorted(str(n) for n in edges["grid_cases"])
    for name, c in cases.items():
        assert _sha(c.points) == str(edges[f"{name}_sha"]), f"{name}: the builder no longer gives the recorded input"
        m = c.model
        assert np.array_equal(m.voxels, edges[f"{name}_voxels"]) and np.array_equal(m.hashes, edges[f"{name}_hashes"]), name
        assert np.array_equal(m.indices, edges[f"{name}_indices"]), name
        if c.f64:
            continue
        sizes, means, covs = P.voxel_stats_model(c.points, m)
        assert np.array_equal(sizes, edges[f"{name}_sizes"]) and np.array_equal(m.ids, edges[f"{name}_ids"]), name
        assert edges[f"{name}_means"].dtype == F32 and edges[f"{name}_covs"].dtype == F32
        np.testing.assert_allclose(means, edges[f"{name}_means"], rtol=1e-6, atol=1e-5, err_msg=name)
        np.testing.assert_allclose(covs, edges[f"{name}_covs"], rtol=1e-4, atol=1e-5, err_msg=name)


def test_deskew_model_equals_the_reference_on_every_motion(edges):
    """Distortion.filter itself on the nineteen motions (0 .. pi - 1e-6 rad, float64 and float32-rounded poses) at n = 4000:
    the model, the written-out construction and the oracle's O.distort at 1e-11 m (measured: 1.5e-13 m and less)."""
    n, stride = 4000, int(edges["deskew_stride"])
    pc, ts = P.deskew_points(n), P.deskew_timestamps(n, "epoch")
    assert _sha(pc) + _sha(ts) == str(edges["deskew_sha"])
    worst = 0.0
    for name, rpose in P.deskew_motions().items():
        assert P.same_bits(np.asarray(edges[f"deskew_{name}_rpose"]), np.asarray(rpose))
        want = edges[f"deskew_{name}"]
        for out in (P.deskew_model(pc, ts, rpose), P.deskew_generic(pc, ts, rpose), O.distort(pc, ts, rpose)):
            worst = max(worst, float(np.abs(out[::stride] - want).max()))
            np.testing.assert_allclose(out[::stride], want, rtol=0, atol=1e-11, err_msg=name)
    print(f"de-skew, model / construction / oracle against the recording: worst {worst:.2e} m")


# ----------------------------------------------------------------------------------------------------------------------
# the cases are what they claim to be
# ----------------------------------------------------------------------------------------------------------------------
def test_case_claims(small, large):
    assert P.hash_of(P.COLLISION_OFFSET) == 0 and P.hash_of(P.SENTINEL_VOXEL) == -1
    assert P.hash_of((5, 6, 7)) == P.hash_of(tuple(a + b for a, b in zip((5, 6, 7), P.COLLISION_OFFSET)))
    by = {c.name: c for c in small + large}
    # ties: exact halves, rounded to even
    for c in P.tie_cases():
        k = c.facts["ties"]
        q = c.points[:k].astype(F64) / c.voxel
        assert np.all(np.abs(q - np.floor(q)) == 0.5) and np.all(c.model.voxels[:k] % 2 == 0)
    # collisions collide: one sample, one voxel id per pair
    m = by["collision"].model
    for far, near in by["collision"].facts["pairs"]:
        both = np.concatenate([far, near])
        assert len({int(h) for h in m.hashes[both]}) == 1 and len({int(i) for i in m.ids[both]}) == 1
        assert len({tuple(v) for v in m.voxels[both]}) == 2 and int(far[0]) in m.indices.tolist()
    # the sentinel voxel hashes to -1 and sorts between the negative and the non-negative hashes
    for name, k in (("sentinel-one", 1), ("sentinel-several", 7), ("sentinel-none", 0)):
        m = by[name].model
        assert int((m.hashes == -1).sum()) == k and int((m.uniq == -1).sum()) == min(k, 1)
    # the bucket sort: occupancy 4096 (the LDS list's last size) and 4097 (its first overflow) of slice 0
    assert by["bucket-slice-4096"].model.slice_occupancy().max() == P.BUCKET_CAP
    assert by["bucket-slice-4097"].model.slice_occupancy().max() == P.BUCKET_CAP + 1
    occ = by["bucket-full-262144"].model.slice_occupancy()
    assert (occ > P.BUCKET_CAP).any() and ((occ > 0) & (occ <= P.BUCKET_CAP)).any()
    # full key range: 64 differing bits, eight radix passes
    P.assert_full_range(by["wrap-V300"].model)
    for v in P.SORT_EMIT_V:
        full, clustered = (by[f"repeat-{k}-n262145-V{v}"].model for k in ("full", "clustered"))
        assert full.count == clustered.count == v and clustered.radix_passes() <= 5
        if v >= 63:
            assert full.radix_passes() == 8
    assert [P.sort_emit_form(v) for v in (8191, 8192, 8193, 20000)] == ["registers", "registers", "loop", "loop"]
    assert by["exact-switch-V32768"].model.count == P.EXACT_BUCKET_MAX_V
    assert by["exact-switch-V32769"].model.count == P.EXACT_BUCKET_MAX_V + 1
    # the de-skew cases: every size, every kind, the extremes where they are said to be
    cases = P.deskew_cases()
    assert {c[1] for c in cases} == set(P.DESKEW_SIZES) and {c[2] for c in cases} == set(P.TS_KINDS)
    assert any(c[3] == 16384 for c in cases) and any(c[4] == 16384 for c in cases)
    for c in cases:
        if c[3] is not None:
            ts = P.deskew_timestamps(c[1], c[2], c[3], c[4])
            assert int(np.argmin(ts)) == c[3] % c[1] and int(np.argmax(ts)) == c[4] % c[1]
    ts = P.deskew_timestamps(1000, "epoch")
    assert ts.min() > 1.5e9 and ts.max() - ts.min() <= 0.1
    assert len(set(P.deskew_timestamps(1000, "two_valued").tolist())) == 2
    assert P.deskew_timestamps(1000, "negative").max() < 0


# ----------------------------------------------------------------------------------------------------------------------
# deliberately wrong copies: each fails by its own check and no other
# ----------------------------------------------------------------------------------------------------------------------
def test_wrong_copies_of_the_sample_fail_by_their_own_check(small):
    by = {c.name: c for c in small}
    # the last index of a voxel instead of the first
    m = by["dedupe-spread-n1025"].model
    ends = np.append(m.starts[1:], m.n) - 1
    assert P.check_sample(_exact_out(m, m.order[ends]), m) == ["samples"]
    m = by["collision"].model
    assert P.check_sample(_exact_out(m, m.order[np.append(m.starts[1:], m.n) - 1]), m) == ["samples"]
    # the samples in unsigned hash order
    m = by["sentinel-one"].model
    unsigned = m.indices[np.argsort(m.uniq.view(np.uint64), kind="stable")]
    assert not np.array_equal(unsigned, m.indices) and P.check_sample(_exact_out(m, unsigned), m) == ["order"]
    # a collision left as two samples: one sample per distinct VOXEL
    m = by["collision"].model
    _, first = np.unique(m.voxels, axis=0, return_index=True)
    two = first[np.lexsort((first, m.hashes[first]))]
    assert two.shape[0] == m.count + 3 and P.check_sample(_exact_out(m, two), m) == ["samples"]
    # the sentinel voxel dropped
    for name in ("sentinel-one", "sentinel-several"):
        m = by[name].model
        assert P.check_sample(_exact_out(m, m.indices[m.uniq != -1]), m) == ["samples"]
    m = by["sentinel-several"].model  # ... or its side cell won by another than the smallest index
    other = m.indices.copy()
    other[m.uniq == -1] = max(by["sentinel-several"].facts["where"])
    assert P.check_sample(_exact_out(m, other), m) == ["samples"]
    # the count off by one; zero padding instead of NaN / -1
    m = by["wrap-V300"].model
    for delta in (1, -1):
        out = _padded_out(m)
        out["count"] = m.count + delta
        assert P.check_sample(out, m) == ["count"]
    out = _padded_out(m)
    out["points"][m.count:] = 0.0
    out["indices"][m.count:] = 0
    assert P.check_sample(out, m) == ["padding"]
    out = _padded_out(m)
    out["indices"][-1] = 0
    assert P.check_sample(out, m) == ["padding"]


def test_wrong_copies_of_voxels_and_statistics_fail_by_their_own_check(small):
    by = {c.name: c for c in small}
    # round half away from zero
    for c in P.tie_cases():
        m = c.model
        away = P.voxel_coords(c.points, c.voxel, half_away=True)
        assert not np.array_equal(away, m.voxels)
        assert P.check_hash({"voxels": away, "hashes": P.voxel_hashes(away)}, m) == ["voxels"]
        assert P.check_hash({"voxels": m.voxels, "hashes": m.hashes + 1}, m) == ["hashes"]
    # the sums of ONE crafted voxel in reversed order: fifty points whose float32 sums depend on the order
    rng = np.random.default_rng(11)
    pts = np.concatenate([by["collision"].points, rng.uniform(-0.45, 0.45, (50, 3)).astype(F32) + F32(20.0)])
    m = P.SampleModel(pts, 1.0)
    vid = int(m.ids[-1])
    assert m.sizes[vid] == 50
    right = P.voxel_stats_model(pts, m)
    wrong = P.voxel_stats_model(pts, m, reverse_in=vid)
    assert not (P.same_bits(right[1], wrong[1]) and P.same_bits(right[2], wrong[2])), "the crafted voxel does not tell the order"
    others = np.arange(m.count) != vid
    assert P.same_bits(right[1][others], wrong[1][others]) and P.same_bits(right[2][others], wrong[2][others])
    np.testing.assert_allclose(wrong[1], right[1], rtol=1e-6, atol=1e-5)   # (the bars in force until now let it through)
    np.testing.assert_allclose(wrong[2], right[2], rtol=1e-4, atol=1e-5)
    out = {"ids": m.ids, "count": m.count}
    assert P.check_stats(dict(out, sizes=wrong[0], means=wrong[1], covs=wrong[2]), m, right) == ["stats"]
    # the covariance divided by the count
    norm = P.voxel_stats_model(pts, m, normalise=True)
    assert P.check_stats(dict(out, sizes=norm[0], means=norm[1], covs=norm[2]), m, right) == ["stats"]
    assert P.check_stats(dict(out, sizes=right[0], means=right[1], covs=right[2]), m, right) == []
    ids = m.ids.copy()
    ids[-1] += 1
    assert P.check_stats(dict(out, ids=ids), m, right) == ["ids"]


def test_wrong_copies_of_the_deskew_fail_by_their_own_check():
    motions = P.deskew_motions()
    # the minimum taken over the first 16 384 timestamps only
    n = 16385
    p, ts, pose = P.deskew_points(n), P.deskew_timestamps(n, "unsorted", lo_at=16384, hi_at=0), motions["theta0.3-f64"]
    want = P.deskew_model(p, ts, pose)
    assert P.check_deskew(want, want, p, pose) == [] and P.check_deskew(P.deskew_generic(p, ts, pose), want, p, pose) == []
    assert P.check_deskew(P.deskew_generic(p, ts, pose, alpha=P.deskew_alpha(ts, limit=16384)), want, p, pose) == ["deskew"]
    ts = P.deskew_timestamps(n, "epoch", lo_at=0, hi_at=16384)
    want = P.deskew_model(p, ts, pose)
    assert P.check_deskew(P.deskew_generic(p, ts, pose, alpha=P.deskew_alpha(ts, limit=16384)), want, p, pose) == ["deskew"]
    # one member's range applied to another
    mine, theirs = P.deskew_timestamps(257, "unsorted"), P.deskew_timestamps(300, "negative", seed=1)
    p = P.deskew_points(257)
    want = P.deskew_model(p, mine, pose)
    leaked = (mine - theirs.min()) / (theirs.max() - theirs.min())
    assert P.check_deskew(P.deskew_generic(p, mine, pose, alpha=leaked), want, p, pose) == ["deskew"]
    # the raw-matrix log map (the library before this audit) on a float32 pose: fails from theta = 1e-4 on, at 0.05 by 2e-10
    # of the range; on the exact float64 poses it passes
    p, ts = P.deskew_points(4000), P.deskew_timestamps(4000, "epoch")
    for th in (0.05, 0.3, 1.0, 3.0):
        pose = motions[f"theta{th:g}-f32"]
        assert P.check_deskew(P.deskew_raw_log(p, ts, pose), P.deskew_model(p, ts, pose), p, pose) == ["deskew"], th
        pose = motions[f"theta{th:g}-f64"]
        assert P.check_deskew(P.deskew_raw_log(p, ts, pose), P.deskew_model(p, ts, pose), p, pose) == []
    assert P.check_deskew(np.zeros((4000, 3), F32), P.deskew_model(p, ts, pose), p, pose) == ["deskew"]


# ----------------------------------------------------------------------------------------------------------------------
# the de-skew bar
# ----------------------------------------------------------------------------------------------------------------------
def test_deskew_bar_is_the_measured_one():
    """DESKEW_SPREAD is the worst difference, per row and relative to |p| + |t|, between the model in float64 (scipy) and in
    np.longdouble over every de-skew case (measured 1.88e-15; the exact float64 poses alone: 8.3e-16), the bar 4 x it and
    tighter than the project's 1e-11 m at 120 m; the written-out construction agrees with scipy to the same rounding, and
    the oracle's O.distort — the kernel's arithmetic in numpy — meets the bar on every case, float32 poses included."""
    if np.finfo(P.LD).eps >= np.finfo(F64).eps:
        pytest.fail("np.longdouble is no wider than float64 here: the bar cannot be re-measured")
    worst, worst_f64, worst_oracle = 0.0, 0.0, 0.0
    for case in P.deskew_cases():
        p, ts, pose = P.build_deskew_case(case)
        model = P.deskew_model(p, ts, pose)
        e = P.deskew_error(model, P.deskew_generic(p, ts, pose, P.LD), p, pose)
        worst = max(worst, e)
        if not case[5].endswith("f32"):
            worst_f64 = max(worst_f64, e)
        eo = P.deskew_error(O.distort(p, ts, pose), model, p, pose)
        worst_oracle = max(worst_oracle, eo)
        assert eo <= P.DESKEW_BAR, (case[0], case[5], eo)
    print(f"de-skew model, float64 against longdouble: worst {worst:.2e} (float64 poses alone {worst_f64:.2e}) of |p| + |t|; "
          f"bar {P.DESKEW_BAR:.2e}; O.distort against the model: worst {worst_oracle:.2e}")
    assert P.DESKEW_SPREAD / 1.5 <= worst <= P.DESKEW_SPREAD, worst
    assert P.DESKEW_BAR == 4 * P.DESKEW_SPREAD and P.DESKEW_BAR * (120.0 + np.linalg.norm(P.DESKEW_T)) <= 1e-11
