"""`pykdtree.kdtree.KDTree` on the MI355X: the class the reference builds over its local map and queries for the nearest
neighbour of every target and the k + 1 neighbours of every map point whose normal is due (slam/odometry/local_map.py:369,
385, 405), answered by the exact k-NN search of the library (`IcpContext.knn_query`, `icp_knn_query`).

    tree = KDTree(map_points)                 # [M, 3]
    dist, idx = tree.query(points)            # [n] float32, [n] uint32
    dist, idx = tree.query(points, k=11)      # [n, 11], [n, 11]

`register.install_kdtree()` places this module at `sys.modules["pykdtree.kdtree"]`, so that the reference's unmodified
`KdTreeLocalMap` imports it.  The search is exact: neighbours ascend by (distance, index), exact ties go to the lower index,
distances are float32 (pykdtree computes float32 data in float32 as well).  Entries without a neighbour are (+inf, n), the
convention pykdtree documents.  What the library does not do is refused, not ignored: `eps != 0`, `mask`, data that is not
[M, 3], k > 32."""
import numpy as np

from ._lib import KNN_MAX_K

# Builds the private context of a tree made without one; None: `IcpContext()`.  (Tests put a CPU stand-in here.)
context_factory = None
# private contexts of trees that are gone: the reference builds a tree per map update (local_map.py:369) and drops the one
# before — the next tree takes over its context, with the device buffers it has already grown
_idle_contexts = []


def _private_context():
    if _idle_contexts:
        return _idle_contexts.pop()
    if context_factory is not None:
        return context_factory()
    from .engine import IcpContext
    return IcpContext()


class KDTree:
    def __init__(self, data_pts, leafsize=16, context=None):
        """data_pts [M, 3]; `leafsize` is accepted and unused (there are no leaves: a voxel hash grid, searched exactly either
        way).  context: an `IcpContext` — or a stand-in with `map_set` / `knn_query` — to hold the points; None creates a
        private one."""
        pts = np.asarray(data_pts)
        if pts.ndim != 2:
            raise ValueError(f"KDTree: data_pts must be [n, ndim], got an array of shape {pts.shape}")
        self.n, self.ndim = int(pts.shape[0]), int(pts.shape[1])
        if self.ndim != 3:
            raise ValueError(f"KDTree: the MI355X search is built for ndim = 3, got ndim = {self.ndim}")
        if self.n < 1:
            raise ValueError("KDTree: data_pts is empty")
        self.data_pts = np.ascontiguousarray(pts, dtype=np.float32)
        self.leafsize = int(leafsize)
        self._private = context is None
        self._ctx = _private_context() if context is None else context
        self._ctx.map_set(self.data_pts)

    def __del__(self):
        if getattr(self, "_private", False) and getattr(self, "_ctx", None) is not None and _idle_contexts is not None:
            _idle_contexts.append(self._ctx)
            self._ctx = None

    def query(self, query_pts, k=1, eps=0, distance_upper_bound=None, sqr_dists=False, mask=None):
        """(dist float32, idx uint32), [n] for k = 1 and [n, k] otherwise: the k nearest data points of every row of
        query_pts [n, 3], nearest first."""
        if eps != 0:
            raise ValueError(f"KDTree.query: eps = {eps}: the search is exact, an approximate one is not built")
        if mask is not None:
            raise ValueError("KDTree.query: mask is not supported")
        q = np.asarray(query_pts)
        if q.ndim != 2 or q.shape[1] != self.ndim:
            raise ValueError(f"KDTree.query: query_pts must be [n, {self.ndim}], got an array of shape {q.shape}")
        k = int(k)
        if not 1 <= k <= KNN_MAX_K:
            raise ValueError(f"KDTree.query: k = {k} is outside 1..{KNN_MAX_K}")
        dist, idx = self._ctx.knn_query(np.ascontiguousarray(q, dtype=np.float32), k=k,
                                        distance_upper_bound=distance_upper_bound, sqr_dists=bool(sqr_dists))
        dist = np.asarray(dist, dtype=np.float32).reshape(-1, k)
        idx = np.asarray(idx).reshape(-1, k).astype(np.uint32)
        if k == 1:
            return dist[:, 0], idx[:, 0]
        return dist, idx
