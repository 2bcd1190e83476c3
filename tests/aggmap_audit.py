"""Bit model of the aggregated world map (`icp_aggmap_*`, include/icp_mi355x.h; csrc/aggmap.hip), in numpy: vectorised, float64
operation by operation, so that the device's arrays can be compared with it bit for bit.

    w = ((r0 x + r1 y) + r2 z) + t     float64, every product and sum rounded once
    c = rint(w / v)                    half to even
    key = the three coordinates, biased by 2^20, 21 bits each (x lowest): exact
    slot = mix(key) & mask             x ^= x >> 33; x *= 0xff51afd7ed558ccd; x ^= x >> 33

`AggMapModel(v, C, R, variant=...)`: `variant` names one deliberately WRONG reading of the specification (WRONG_VARIANTS); the
CPU tests show that each is caught on a named cloud.  No deliberately wrong kernel exists."""
from fractions import Fraction

import numpy as np

OFFSET = 1 << 20
MIX = np.uint64(0xff51afd7ed558ccd)
WRONG_VARIANTS = ("last_row_wins", "highest_in_wave", "truncate", "float32_transform", "fma", "hash_merge", "unordered_emit",
                  "capacity_by_key", "no_creator_hits", "submap_le")


def world_points(points, pose, variant=None):
    """[n,3] float64: the rows of `points` (float32) moved by `pose` [4,4] float64"""
    p = np.asarray(points, np.float32).reshape(-1, 3)
    pose = np.asarray(pose, np.float64).reshape(4, 4)
    if variant == "float32_transform":
        q, m = p, pose.astype(np.float32)
    else:
        q, m = p.astype(np.float64), pose
    w = np.empty(q.shape, q.dtype)
    with np.errstate(over="ignore", invalid="ignore"):
        for i in range(3):
            if variant == "fma":  # what a contracting compiler makes of the expression: the two later products are fused
                w[:, i] = [float(Fraction(float(m[i, 2])) * Fraction(float(z)) +
                                 Fraction(float(Fraction(float(m[i, 1])) * Fraction(float(y)) + Fraction(float(m[i, 0] * x))))) + m[i, 3]
                           for x, y, z in q]
            else:
                w[:, i] = ((m[i, 0] * q[:, 0] + m[i, 1] * q[:, 1]) + m[i, 2] * q[:, 2]) + m[i, 3]
    return w.astype(np.float64)


def voxel_coords_real(w, voxel, variant=None):
    """rint(w / v), still float64 (the range is tested before any conversion)"""
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        q = np.asarray(w, np.float64) / np.float64(voxel)
        return np.trunc(q) if variant == "truncate" else np.rint(q)


def in_range(c):
    return np.all((c >= -float(OFFSET)) & (c < float(OFFSET)), axis=-1)


def pack_keys(c):
    """uint64 keys of int64 voxel coordinates [n,3] in [-2^20, 2^20)"""
    b = (np.asarray(c, np.int64) + OFFSET).astype(np.uint64)
    return b[:, 0] | (b[:, 1] << np.uint64(21)) | (b[:, 2] << np.uint64(42))


def unpack_keys(keys):
    k = np.asarray(keys, np.uint64)
    m = np.uint64(0x1FFFFF)
    return np.stack([k & m, (k >> np.uint64(21)) & m, (k >> np.uint64(42)) & m], axis=-1).astype(np.int64) - OFFSET


def slot_count(capacity, max_rows):
    need, s = 2 * (int(capacity) + int(max_rows)), 2
    while s < need:
        s <<= 1
    return s


def slot_of_keys(keys, slots):
    """first slot of every key's probe chain in a table of `slots` slots"""
    x = np.asarray(keys, np.uint64).copy()
    x ^= x >> np.uint64(33)
    with np.errstate(over="ignore"):
        x *= MIX
    x ^= x >> np.uint64(33)
    return (x & np.uint64(slots - 1)).astype(np.int64)


def grid_hash(c):
    """the grid sample's colliding hash (wrapping int64), which the map does NOT use"""
    c = np.asarray(c, np.int64).astype(np.uint64)
    with np.errstate(over="ignore"):
        return np.uint64(73856093) * c[:, 0] + np.uint64(19349669) * c[:, 1] + np.uint64(83492791) * c[:, 2]


class AggMapModel:
    def __init__(self, voxel_size, capacity, max_insert_rows=262144, variant=None):
        assert variant is None or variant in WRONG_VARIANTS, variant
        assert voxel_size > 0 and np.isfinite(voxel_size) and capacity >= 1 and max_insert_rows >= 1
        self.voxel, self.capacity, self.max_rows, self.variant = float(voxel_size), int(capacity), int(max_insert_rows), variant
        self.slots = slot_count(capacity, max_insert_rows)
        self.clear()

    def clear(self):
        self.w = np.empty((0, 3), np.float64)
        self.hits = np.empty(0, np.uint32)
        self.first_frame = np.empty(0, np.int32)
        self.last_frame = np.empty(0, np.int32)
        self.keys = np.empty(0, np.uint64)          # key of every stored point
        self.unstored = np.empty(0, np.uint64)      # keys claimed beyond the capacity
        self.inserts = self.dropped = self.out_of_range = self.nonfinite = 0
        self.error = 0

    @property
    def size(self):
        return len(self.w)

    def stats(self):
        return {"size": self.size, "inserts": self.inserts, "dropped": self.dropped, "out_of_range": self.out_of_range,
                "nonfinite": self.nonfinite, "error": self.error}

    def _keys_of(self, c):
        if self.variant == "hash_merge":
            return grid_hash(c)
        return pack_keys(c)

    def insert(self, points, pose, frame_id):
        p = np.asarray(points, np.float32).reshape(-1, 3)
        pose = np.asarray(pose, np.float64).reshape(4, 4)
        assert len(p) <= self.max_rows and np.all(np.isfinite(pose))
        self.inserts += 1
        if len(p) == 0:
            return
        w = world_points(p, pose, self.variant)
        finite = np.all(np.isfinite(w), axis=1)
        c = voxel_coords_real(w, self.voxel, self.variant)
        ok = finite & in_range(c)
        self.nonfinite += int((~finite).sum())
        self.out_of_range += int((finite & ~ok).sum())
        rows = np.flatnonzero(ok)
        if len(rows) == 0:
            return
        keys = self._keys_of(c[rows].astype(np.int64))
        uniq, first, inverse, counts = np.unique(keys, return_index=True, return_inverse=True, return_counts=True)
        winner = rows[first]  # smallest row of the insert in every voxel
        if self.variant == "last_row_wins":
            last = np.zeros(len(uniq), np.int64)
            np.maximum.at(last, inverse, rows)
            winner = last
        elif self.variant == "highest_in_wave":  # the highest lane of every wave group leads it; the lowest leader wins
            wave = rows // 64
            pair, pinv = np.unique(np.stack([inverse, wave], 1), axis=0, return_inverse=True)
            top = np.zeros(len(pair), np.int64)
            np.maximum.at(top, pinv.reshape(-1), rows)
            winner = np.full(len(uniq), np.iinfo(np.int64).max)
            np.minimum.at(winner, pair[:, 0], top)
        # where every voxel of the insert stands: stored index, -2 unstored, -1 unknown
        state = np.full(len(uniq), -1, np.int64)
        if self.size:
            order = np.argsort(self.keys, kind="stable")
            pos = np.searchsorted(self.keys[order], uniq)
            hit = (pos < self.size) & (self.keys[order][np.minimum(pos, self.size - 1)] == uniq)
            state[hit] = order[pos[hit]]
        if len(self.unstored):
            state[np.isin(uniq, self.unstored)] = -2
        stored = state >= 0
        self.hits[state[stored]] += counts[stored].astype(np.uint32)
        self.last_frame[state[stored]] = np.maximum(self.last_frame[state[stored]], np.int32(frame_id))
        self.dropped += int(counts[state == -2].sum())
        new = np.flatnonzero(state == -1)
        room = self.capacity - self.size
        if room <= 0:  # a full map creates nothing
            self.dropped += int(counts[new].sum())
            return
        if self.variant == "capacity_by_key":
            cut = new[:room], new[room:]
            kept = cut[0][np.argsort(winner[cut[0]], kind="stable")]
            lost = cut[1]
        else:
            by_row = new[np.argsort(winner[new], kind="stable")]  # creation order: ascending winning row
            kept, lost = by_row[:room], by_row[room:]
        if self.variant == "unordered_emit":
            kept = np.sort(kept)  # by key
        self.w = np.concatenate([self.w, w[winner[kept]]])
        self.hits = np.concatenate([self.hits, (np.zeros(len(kept)) if self.variant == "no_creator_hits" else counts[kept]).astype(np.uint32)])
        self.first_frame = np.concatenate([self.first_frame, np.full(len(kept), frame_id, np.int32)])
        self.last_frame = np.concatenate([self.last_frame, np.full(len(kept), frame_id, np.int32)])
        self.keys = np.concatenate([self.keys, uniq[kept]])
        self.unstored = np.concatenate([self.unstored, uniq[lost]])
        self.dropped += int(counts[lost].sum())

    def points(self, origin=None, dtype=np.float32):
        if np.dtype(dtype) == np.float64:
            return self.w.copy()
        o = np.zeros(3) if origin is None else np.asarray(origin, np.float64).reshape(3)
        return (self.w - o[None, :]).astype(np.float32)

    def submap(self, lo, hi, pose):
        keep = (self.first_frame >= lo) & ((self.first_frame <= hi) if self.variant == "submap_le" else (self.first_frame < hi))
        idx = np.flatnonzero(keep).astype(np.int32)
        m = np.asarray(pose, np.float64).reshape(4, 4)
        q = self.w[idx]
        out = np.empty((len(idx), 3), np.float64)
        for i in range(3):
            out[:, i] = ((m[i, 0] * q[:, 0] + m[i, 1] * q[:, 1]) + m[i, 2] * q[:, 2]) + m[i, 3]
        return out.astype(np.float32), idx


def sequential_model(voxel, capacity, inserts):
    """The same semantics as a plain dictionary loop, row by row (the second formulation the model is held to).
    inserts: [(points, pose, frame_id)].  Returns (w, hits, first_frame, last_frame, stats)."""
    table, w, hits, first, last = {}, [], [], [], []
    st = {"size": 0, "inserts": 0, "dropped": 0, "out_of_range": 0, "nonfinite": 0, "error": 0}
    v = np.float64(voxel)
    for points, pose, frame in inserts:
        st["inserts"] += 1
        m = np.asarray(pose, np.float64).reshape(4, 4)
        for row in np.asarray(points, np.float32).reshape(-1, 3):
            x, y, z = (np.float64(a) for a in row)
            with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
                wr = [((m[i, 0] * x + m[i, 1] * y) + m[i, 2] * z) + m[i, 3] for i in range(3)]
                if not all(np.isfinite(a) for a in wr):
                    st["nonfinite"] += 1
                    continue
                c = [np.rint(a / v) for a in wr]
            if not all(-float(OFFSET) <= a < float(OFFSET) for a in c):
                st["out_of_range"] += 1
                continue
            key = tuple(int(a) for a in c)
            i = table.get(key)
            if i is None:
                if len(w) >= capacity:
                    st["dropped"] += 1
                    continue
                table[key] = len(w)
                w.append(wr)
                hits.append(1)
                first.append(frame)
                last.append(frame)
            else:
                hits[i] += 1
                last[i] = max(last[i], frame)
    st["size"] = len(w)
    return (np.array(w, np.float64).reshape(-1, 3), np.array(hits, np.uint64).astype(np.uint32), np.array(first, np.int32),
            np.array(last, np.int32), st)


def colliding_keys(slots, target_slot, count, rng=None, avoid=()):
    """`count` distinct in-range voxel coordinates [count,3] whose keys all start their probe chain at `target_slot`"""
    rng = rng or np.random.default_rng(7)
    found, seen = [], set(map(tuple, np.asarray(avoid, np.int64).reshape(-1, 3)))
    while len(found) < count:
        c = rng.integers(-2000, 2000, size=(200000, 3))
        good = c[slot_of_keys(pack_keys(c), slots) == target_slot]
        for row in good:
            if tuple(row) not in seen:
                seen.add(tuple(row))
                found.append(row)
    return np.array(found[:count], np.int64)


def voxel_centres(c, voxel):
    """float32 points in the middle of the given voxels (exactly representable for power-of-two voxel sizes and small coordinates)"""
    return (np.asarray(c, np.float64) * voxel).astype(np.float32)
