"""Generates tests/golden/map_lifecycle.npz by running the REFERENCE's own KdTreeLocalMap (unmodified, imported from
/root/reference through the stubs in oracle/shims, as oracle/make_golden.py does for `mu_*`) through the `window`,
`window_one` and `set_then_update` scripts of tests/map_lifecycle.py (map_lifecycle.RECORDED).  TEST INFRASTRUCTURE.  Run in the build container only:

    python oracle/make_golden_map_lifecycle.py

Recorded after EVERY operation: `_local_map` (float32) and `_local_map_num_elements`; at the two operations of
map_lifecycle.RECORDED_SEARCH (before and directly behind the first eviction) the neighbour index and the normal the
reference gives each of the 512 displaced probes.  The scripts' inputs are regenerated from the seeded generator by the
tests, not stored: the fixture holds recorded results only.
"""
import logging
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "oracle", "shims"), "/root/reference", os.path.join(ROOT, "pylidar-slam_amd"),
                os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")]
logging.disable(logging.WARNING)

import numpy as np  # noqa: E402
import torch  # noqa: E402

torch.set_num_threads(1)

from slam.odometry.local_map import KdTreeLocalMap, KdTreeLocalMapConfig  # noqa: E402

import map_lifecycle as L  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "map_lifecycle.npz")


def run(name):
    s = L.script(name)
    lm = KdTreeLocalMap(KdTreeLocalMapConfig(local_map_size=s.local_map_size))
    lm.init()
    out = {}
    for i, op in enumerate(s.ops):
        if op.kind == "init":
            lm.init()
        elif op.kind == "set":
            lm.set_map_pointcloud(op.cloud.copy())
        else:
            cloud = op.cloud
            if cloud is not None and op.skip_null:  # the caller's side of skip_null: the reference is handed the kept rows
                cloud = cloud[~((cloud == 0).all(axis=1))]
            lm.update(op.rel.copy(), new_pc_data=None if cloud is None else cloud.copy())
        m = lm._local_map if lm._local_map is not None else np.zeros((0, 3), np.float32)
        assert m.dtype == np.float32, (name, i, m.dtype)
        out[f"{name}_map_{i}"] = np.ascontiguousarray(m)
        out[f"{name}_counts_{i}"] = np.array(lm._local_map_num_elements, np.int64)
        for step, first_row in (L.RECORDED_SEARCH if name == "window" else ()):
            if step == i:
                probes = L.displaced_probes(m, seed=step, first_row=first_row)
                res = lm.nearest_neighbor_search(probes)
                _, ix = lm._model_kdtree.query(probes)
                assert np.array_equal(res.neighbor_points, m[ix])
                out[f"{name}_search_ix_{i}"] = ix.astype(np.int32)
                out[f"{name}_search_normals_{i}"] = np.asarray(res.neighbor_normals, np.float32)
    return out


if __name__ == "__main__":
    out = {}
    for name in L.RECORDED:
        out.update(run(name))
    np.savez_compressed(OUT, **out)
    print(os.path.basename(OUT), os.path.getsize(OUT) // 1024, "KiB;", "components.npz",
          os.path.getsize(os.path.join(os.path.dirname(OUT), "components.npz")) // 1024, "KiB")
