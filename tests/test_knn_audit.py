"""CPU: the float32 model of the k-NN query (tests/knn_audit.py) against a float64 truth, its ties, the wrong copies its
comparison has to catch — and `pylidar_slam_amd.kdtree.KDTree` / `register.install_kdtree()` on a stand-in context whose
`knn_query` is that model, down to the reference's own `ICPFrameToModel` running its `KdTreeLocalMap` through it."""
import os
import sys

import numpy as np
import pytest

import knn_audit as A
from oracle_context import OracleContext

REF = "/root/reference"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class ModelContext(OracleContext):
    """The stand-in: `map_set` keeps the points, `knn_query` is the model."""

    def map_set(self, points):
        self.knn_map = np.ascontiguousarray(self._np(points).reshape(-1, 3), dtype=np.float32)

    def knn_query(self, points, k=1, distance_upper_bound=None, sqr_dists=False):
        r = A.model_knn(self.knn_map, np.ascontiguousarray(points, dtype=np.float32), int(k), distance_upper_bound, sqr_dists)
        assert not r.flagged.any()
        return r.dist, r.index


# ---- the model against the truth ---------------------------------------------------------------------------------------
def _audit(map_pts, queries, ks, what):
    """distances within the derived bar, indices equal on every unambiguous row; returns the worst error in ulps"""
    models = A.model_knn_multi(map_pts, queries, ks)
    td, ti = A.truth_knn(map_pts, queries, max(ks) + 1)
    worst = 0.0
    for k in ks:
        r = models[k]
        flagged = float(r.flagged.mean())
        assert flagged <= A.FLAGGED_MAX, (what, k, flagged)
        amb = A.ambiguous_rows(td[:, :k + 1])
        assert float(amb.mean()) <= A.AMBIGUOUS_MAX, (what, k, float(amb.mean()))
        err = A.ulp_error(r.dist, td[:, :k])
        worst = max(worst, float(err.max()))
        print(f"{what} k = {k}: worst distance error {err.max():.3f} ulp (bar {A.DIST_BAR_ULP}), flagged {flagged:.4%}, "
              f"ambiguous {amb.mean():.4%}")
        assert err.max() <= A.DIST_BAR_ULP, (what, k, float(err.max()))
        ok = ~amb & ~r.flagged
        bad = np.flatnonzero(np.any(r.index != ti[:, :k], axis=1) & ok)
        assert bad.size == 0, (what, k, bad[:5].tolist())
    return worst


def test_model_against_float64_truth_on_the_scene():
    map_pts, queries, sampled = A.scene()
    _audit(map_pts, queries, A.KS, "24 576-point map")
    _audit(sampled, queries[:1024], (1, 3, 11, 17, 32), "6 471-point map")


def test_model_squared_distances_and_small_maps():
    map_pts, queries, sampled = A.scene()
    q = queries[:256]
    r = A.model_knn(sampled, q, 11, sqr=True)
    td, _ = A.truth_knn(sampled, q, 11)
    err = A.ulp_error(r.dist, td * td)
    print(f"squared distances: worst {err.max():.3f} ulp (bar {A.SQR_BAR_ULP})")
    assert err.max() <= A.SQR_BAR_ULP
    for k in (4, 11, 32):
        for m in sorted({1, 2, k - 1, k, k + 1}):
            small = np.ascontiguousarray(sampled[::97][:m])
            r = A.model_knn(small, q, k)
            td, ti = A.truth_knn(small, q, k)
            c = min(k, m)
            assert np.all(np.isinf(r.dist[:, c:])) and np.all(r.index[:, c:] == m) and np.all(np.isfinite(r.dist[:, :c]))
            assert A.ulp_error(r.dist, td).max() <= A.DIST_BAR_ULP
            ok = ~A.ambiguous_rows(td[:, :c]) & ~r.flagged
            assert np.array_equal(r.index[ok], ti[ok])


def test_bits_of_the_midpoint_test():
    """the mantissa-bit test of knn_audit._near_f32_midpoint: within one float64 ulp of the middle between two float32 values"""
    rng = np.random.default_rng(5)
    mid = (np.float32(1.0) + np.arange(1, 2000, dtype=np.float32) * np.float32(2.0 ** -23)).astype(np.float64) + 2.0 ** -24
    s = np.concatenate((rng.uniform(1e-3, 500.0, 100000), mid, np.nextafter(mid, 0), np.nextafter(mid, 9), mid + 2.0 ** -40,
                        np.array([0.0, 272.49957275390625])))
    s32 = s.astype(np.float32)
    up = (s32.astype(np.float64) + np.nextafter(s32, np.float32(np.inf)).astype(np.float64)) / 2      # the middles on either
    down = (s32.astype(np.float64) + np.nextafter(s32, np.float32(-np.inf)).astype(np.float64)) / 2  # side, exact in float64
    want = (np.abs(s - up) <= np.spacing(s)) | (np.abs(s - down) <= np.spacing(s))
    assert np.array_equal(A._near_f32_midpoint(s), want) and want.sum() >= 3 * mid.size and not want[-2:].any()


def test_lattice_and_duplicates_order_by_distance_then_index():
    for name, (map_pts, queries) in (("lattice", A.lattice()), ("duplicated", A.duplicated())):
        for k in (1, 8, 11, 32):
            r = A.model_knn(map_pts, queries, k)
            assert not r.flagged.any(), name
            A.check_key_order(map_pts, queries, r, name)
    map_pts, queries = A.lattice()
    r = A.model_knn(map_pts, queries[343:], 8)          # a cell centre: its eight corners, all at sqrt(0.75), ascending index
    assert np.all(r.dist == np.float32(np.sqrt(np.float32(0.75)))) and np.all(np.diff(r.index, axis=1) > 0)
    map_pts, queries = A.duplicated()
    r = A.model_knn(map_pts, queries, 2)
    pairs = r.dist[:, 0] == r.dist[:, 1]                 # a point and its copy: the lower index first
    assert pairs.all() and np.all(r.index[:, 1] == r.index[:, 0] + 1) and np.all(r.index[:, 0] % 2 == 0)


def test_the_comparison_catches_wrong_copies():
    map_pts, queries, sampled = A.scene()
    q = queries[:128]
    want = A.model_knn(sampled, q, 11)
    A.check_bits(want.dist.copy(), want.index.copy(), want)
    # a swapped neighbour pair
    idx = want.index.copy()
    idx[7, [3, 4]] = idx[7, [4, 3]]
    with pytest.raises(AssertionError, match="indices"):
        A.check_bits(want.dist, idx, want)
    # a distance two ulp off
    dist = want.dist.copy()
    dist[9, 10] = np.nextafter(np.nextafter(dist[9, 10], np.float32(np.inf)), np.float32(np.inf))
    with pytest.raises(AssertionError, match="distances"):
        A.check_bits(dist, want.index, want)
    # ... which the truth comparison has to catch from the other side as well: the bar is not loose enough to hide six ulp
    td, _ = A.truth_knn(sampled, q, 11)
    off = want.dist.copy()
    for _ in range(6):
        off = np.nextafter(off, np.float32(np.inf))
    assert A.ulp_error(off, td).max() > A.DIST_BAR_ULP
    # index M - 1 in place of M for a missing entry
    small = np.ascontiguousarray(sampled[:5])
    short = A.model_knn(small, q, 8)
    assert np.all(short.index[:, 5:] == 5) and np.all(np.isinf(short.dist[:, 5:]))
    idx = short.index.copy()
    idx[:, 5:] = 4
    with pytest.raises(AssertionError, match="indices"):
        A.check_bits(short.dist, idx, short)
    # a bound applied with <=: the lattice has points exactly at distance 1
    lat, lq = A.lattice()
    strict = A.model_knn(lat, lq[:343], 11, bound=1.0)
    loose = A.model_knn(lat, lq[:343], 11, bound=1.0, inclusive_bound=True)
    assert np.all(strict.index[:, 1:] == 343) and np.all(strict.index[:, 0] == np.arange(343))
    with pytest.raises(AssertionError):
        A.check_bits(loose.dist, loose.index, strict)
    # non-finite rows have no neighbours
    bad = q[:4].copy()
    bad[0, 0], bad[1, 1], bad[2, 2] = np.nan, np.inf, -np.inf
    r = A.model_knn(sampled, bad, 3)
    assert np.all(np.isinf(r.dist[:3])) and np.all(r.index[:3] == sampled.shape[0]) and np.all(np.isfinite(r.dist[3]))


# ---- KDTree on the stand-in -----------------------------------------------------------------------------------------------
def test_kdtree_shapes_dtypes_and_refusals():
    from pylidar_slam_amd.kdtree import KDTree
    map_pts, queries, sampled = A.scene()
    q = queries[:64]
    tree = KDTree(sampled, leafsize=10, context=ModelContext())
    assert (tree.n, tree.ndim) == (6471, 3) and tree.data_pts.dtype == np.float32 and np.array_equal(tree.data_pts, sampled)
    d1, i1 = tree.query(q)
    assert d1.shape == (64,) and i1.shape == (64,) and d1.dtype == np.float32 and i1.dtype == np.uint32
    d, i = tree.query(q.astype(np.float64), k=11)
    assert d.shape == (64, 11) and i.shape == (64, 11) and d.dtype == np.float32 and i.dtype == np.uint32
    want = A.model_knn(sampled, q, 11)
    A.check_bits(d, i.astype(np.int32), want)
    assert np.array_equal(d1, d[:, 0]) and np.array_equal(i1, i[:, 0])
    ds, _ = tree.query(q, k=2, sqr_dists=True)
    assert np.array_equal(ds, A.model_knn(sampled, q, 2, sqr=True).dist)
    db, ib = tree.query(q, k=3, distance_upper_bound=0.3)
    assert np.all(ib[np.isinf(db)] == 6471) and np.isinf(db).any() and np.isfinite(db).any() and np.all(db[np.isfinite(db)] < 0.3)
    with pytest.raises(ValueError, match="eps"):
        tree.query(q, eps=0.1)
    with pytest.raises(ValueError, match="mask"):
        tree.query(q, mask=np.zeros(6471, bool))
    with pytest.raises(ValueError, match="ndim"):
        KDTree(np.zeros((10, 2), np.float32), context=ModelContext())
    with pytest.raises(ValueError, match="query_pts"):
        tree.query(np.zeros((4, 2), np.float32))
    for k in (0, 33):
        with pytest.raises(ValueError, match="outside 1..32"):
            tree.query(q, k=k)


def test_private_contexts_come_from_the_factory_and_are_reused(monkeypatch):
    import gc
    from pylidar_slam_amd import kdtree
    made = []

    def factory():
        made.append(ModelContext())
        return made[-1]

    monkeypatch.setattr(kdtree, "context_factory", factory)
    monkeypatch.setattr(kdtree, "_idle_contexts", [])
    _, queries, sampled = A.scene()
    tree = kdtree.KDTree(sampled[:100])
    other = kdtree.KDTree(sampled[100:300])
    assert len(made) == 2 and tree._ctx is made[0] and other._ctx is made[1]
    _, i = other.query(queries[:8])
    assert np.array_equal(i.astype(np.int32), A.model_knn(sampled[100:300], queries[:8], 1).index[:, 0])
    del tree
    gc.collect()
    again = kdtree.KDTree(sampled[:50])
    assert len(made) == 2 and again._ctx is made[0]       # the context of the tree that is gone, with its new map
    _, i = again.query(queries[:8])
    assert np.array_equal(i.astype(np.int32), A.model_knn(sampled[:50], queries[:8], 1).index[:, 0])


# ---- the reference's own ICPFrameToModel through install_kdtree() ------------------------------------------------------------
@pytest.fixture()
def reference_on_path():
    added = [os.path.join(ROOT, "oracle", "shims"), REF]
    sys.path[:0] = added
    yield
    for p in added:
        sys.path.remove(p)


def _run_reference(scans, tree_class, log):
    import torch
    import slam.odometry.local_map as ref_local_map
    from slam.common.pose import Pose
    from slam.common.projection import SphericalProjector
    from slam.odometry.alignment import GaussNewtonPointToPlaneConfig
    from slam.odometry.icp_odometry import ICPFrameToModel, ICPFrameToModelConfig
    from slam.odometry.local_map import KdTreeLocalMapConfig
    import icp_oracle as O

    class Logged(tree_class):
        def query(self, query_pts, k=1, **kw):
            d, i = super().query(query_pts, k=k, **kw)
            log.append((np.asarray(self.data_pts if hasattr(self, "data_pts") else self.data, np.float32).copy(),
                        np.asarray(query_pts, np.float32).copy(), int(k), np.asarray(i).astype(np.int64).reshape(len(query_pts), -1)))
            return d, i

    held = ref_local_map.KDTree
    ref_local_map.KDTree = Logged
    try:
        cfg = ICPFrameToModelConfig(
            max_num_alignments=4, threshold_delta_pose=1.0e-4, data_key="sample_points",
            local_map=KdTreeLocalMapConfig(local_map_size=3),
            alignment=GaussNewtonPointToPlaneConfig(gauss_newton_config=dict(max_iters=1, scheme="neighborhood", sigma=0.5)))
        odo = ICPFrameToModel(cfg, projector=SphericalProjector(32, 256, 3, 3.0, -24.0), pose=Pose("euler"),
                              device=torch.device("cpu"))
        odo.init()
        poses = []
        for s in scans:
            d = {"sample_points": O.grid_sample(s, 0.8)[0]}
            odo.process_next_frame(d)
            poses.append(np.asarray(d["odometry_pose"]).copy() if "odometry_pose" in d else np.eye(4, dtype=np.float32))
        return np.stack(poses), np.stack(odo.absolute_poses)
    finally:
        ref_local_map.KDTree = held


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "slam")), reason="reference checkout not present")
def test_reference_kdtree_local_map_runs_through_install_kdtree(reference_on_path, monkeypatch):
    """The reference's `ICPFrameToModel` with its `KdTreeLocalMap`, once on the cKDTree stand-in of oracle/shims and once on
    `pylidar_slam_amd.kdtree` (installed by `install_kdtree()`, backed by the model): every query returns the same indices —
    on a run none of whose rows is ambiguous — and the poses are bit-equal."""
    import logging
    logging.disable(logging.WARNING)
    from pylidar_slam_amd.synthetic import SceneConfig, make_sequence
    import slam.odometry.local_map as ref_local_map
    shim_tree = ref_local_map.KDTree
    assert shim_tree.__module__ == "pykdtree.kdtree" and "shims" in sys.modules["pykdtree.kdtree"].__file__
    # (seed 1: none of the 24 137 query rows of the run is ambiguous — of seeds 1234, 1, 2, ... the first that is so)
    scans, _ = make_sequence(SceneConfig(height=32, width=256, seed=1), 4)
    shim_log, our_log = [], []
    shim_modules = {name: sys.modules.get(name) for name in ("pykdtree", "pykdtree.kdtree")}
    try:
        shim_poses = _run_reference(scans, shim_tree, shim_log)

        from pylidar_slam_amd import kdtree as our_kdtree
        from pylidar_slam_amd.register import install_kdtree
        monkeypatch.setattr(our_kdtree, "context_factory", ModelContext)
        monkeypatch.setattr(our_kdtree, "_idle_contexts", [])
        assert install_kdtree() is our_kdtree
        import pykdtree.kdtree as resolved
        assert resolved is our_kdtree and sys.modules["pykdtree"].kdtree is our_kdtree
        assert ref_local_map.KDTree is our_kdtree.KDTree    # the module imported before the call is handed the new class
        our_poses = _run_reference(scans, our_kdtree.KDTree, our_log)
    finally:
        ref_local_map.KDTree = shim_tree
        for name, mod in shim_modules.items():
            if mod is not None:
                sys.modules[name] = mod

    assert len(shim_log) == len(our_log) and len(shim_log) >= 6 and {k for _, _, k, _ in shim_log} == {1, 11}
    from scipy.spatial import cKDTree
    rows = 0
    for (m0, q0, k0, i0), (m1, q1, k1, i1) in zip(shim_log, our_log):
        assert k0 == k1 and np.array_equal(m0, m1) and np.array_equal(q0, q1)
        td, _ = cKDTree(m0.astype(np.float64)).query(q0.astype(np.float64), k=k0 + 1)
        assert not A.ambiguous_rows(td).any(), "choose another seed: a row of this run is ambiguous"
        assert np.array_equal(i0, i1)
        rows += q0.shape[0]
    assert rows > 1000
    for a, b in zip(shim_poses, our_poses):
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))
