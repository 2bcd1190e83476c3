"""Audit of frame preprocessing — csrc/grid_sample.hip: voxel hash, grid sample (hash-table dedupe + three sorts), voxel
statistics and the de-skew, single and batched — (tests/test_preprocess_audit.py on the CPU,
tests/test_gpu_preprocess_audit.py on the device).  TEST INFRASTRUCTURE: numpy + scipy only, no torch, no GPU, never
imported by the package.

The model, stated without the oracle's `np.unique`:

  voxel coordinates  np.round(float64(p) / float64(voxel)) as int64 (round half to even), defined for |p / voxel| < 2^62:
                     every case stays inside that and asserts it;
  hash               73856093 x + 19349669 y + 83492791 z in wrapping uint64, viewed as int64;
  sample             per distinct hash the smallest input index, the samples by ascending SIGNED hash; padded outputs hold
                     the V samples, then NaN rows / index -1; the count is exact; the float64 paths gather the float64 rows
                     and the batch's float32 copy is (float32) of those rows;
  statistics         voxel id = rank of the hash; per voxel the members in ascending input index, float32 sums one member
                     after the other, mean = sum / float32(count), covariance from separate float32 subtract, multiply and
                     add in the element order of k_voxel_stats: bit for bit;
  de-skew            alpha per frame as Distortion.filter forms it, rotation = scipy Slerp between the identity and
                     Rotation.from_matrix(float64(R)) exactly as the reference constructs it, translation alpha t, float64
                     einsum.  The kernel differs from it by its sincos and the Rodrigues form of the same rotation, so the
                     bar is DESKEW_BAR = 4 x the worst difference between this model in float64 and in np.longdouble, per
                     row, relative to |p| + |t| (test_preprocess_audit.py re-measures it).

NaN timestamps are outside this audit: numpy's min / max propagate a NaN and the device's fmin / fmax drop it; no case
holds one.

Every check returns the list of the names of what failed — `samples`, `order`, `padding`, `count`, `voxels`, `hashes`,
`ids`, `stats`, `deskew` — so that a wrong copy can be shown to fail by its own check and no other.
"""
import numpy as np

F32, F64, I64, U64 = np.float32, np.float64, np.int64, np.uint64
LD = np.longdouble
HASH_MUL = (73856093, 19349669, 83492791)
COLLISION_OFFSET = (4681, -3002, -3445)   # 73856093 * 4681 - 19349669 * 3002 - 83492791 * 3445 = 0
SENTINEL_VOXEL = (-3326, -5281, 4166)     # hashes to -1 = DEDUPE_EMPTY of csrc/grid_sample.hip (the side cell)
BUCKET_BLOCKS, BUCKET_CAP = 64, 4096      # csrc/grid_sample.hip
EXACT_BUCKET_MAX_V = 32768                # exact path: bucket sort up to V, rocPRIM above
PADDED_BUCKET_MAX_N = 262144              # padded path: bucket sort up to n, k_sort_emit above
SORT_WAVES, REG_TILES = 16, 8             # k_sort_emit: tiles per wave <= REG_TILES (V <= 8192) stay in registers
STATS_MAX_ROWS = 20000

# The worst per-row difference between the de-skew model in float64 and in np.longdouble, relative to |p| + |t|, over
# deskew_cases(): measured 1.88e-15 — on the float32 poses, whose orthogonal factor scipy takes from a float64 SVD; the exact
# float64 poses alone give 8.3e-16 — (test_preprocess_audit.py::test_deskew_bar_is_the_measured_one re-measures both), and
# the bar the kernel is held to: 4 x it.  At 120 m range that is 9.2e-13 m, inside the project's 1e-11.
DESKEW_SPREAD = 1.9e-15
DESKEW_BAR = 4.0 * DESKEW_SPREAD


# ----------------------------------------------------------------------------------------------------------------------
# the model: voxels, hashes, sample, statistics
# ----------------------------------------------------------------------------------------------------------------------
def voxel_coords(points, voxel, half_away=False):
    q = np.asarray(points).astype(F64) / F64(voxel)
    assert q.size == 0 or np.abs(q).max() < 2.0 ** 62, "outside the defined range of the int64 conversion"
    if half_away:  # the wrong copy: C's round()
        return (np.sign(q) * np.floor(np.abs(q) + 0.5)).astype(I64)
    return np.round(q).astype(I64)


def voxel_hashes(voxels):
    v = np.asarray(voxels, I64).view(U64).reshape(-1, 3)
    with np.errstate(over="ignore"):
        h = U64(HASH_MUL[0]) * v[:, 0] + U64(HASH_MUL[1]) * v[:, 1] + U64(HASH_MUL[2]) * v[:, 2]
    return h.view(I64)


def hash_of(voxel):
    """The hash of one voxel in Python integers (no numpy): what the case claims are checked with."""
    h = sum(m * int(c) for m, c in zip(HASH_MUL, voxel)) % (1 << 64)
    return h - (1 << 64) if h >= (1 << 63) else h


class SampleModel:
    """voxels [n,3], hashes [n], indices [V] (smallest index per distinct hash, by ascending signed hash), ids [n] (rank of
    the point's hash), uniq [V] (the distinct hashes, ascending), order (stable argsort of the hashes), starts [V]."""

    def __init__(self, points, voxel):
        self.points = np.ascontiguousarray(points)
        self.voxel = float(voxel)
        self.n = int(self.points.shape[0])
        self.voxels = voxel_coords(self.points, voxel).reshape(-1, 3)
        self.hashes = voxel_hashes(self.voxels)
        self.order = np.argsort(self.hashes, kind="stable")
        hs = self.hashes[self.order]
        head = np.ones(self.n, bool)
        head[1:] = hs[1:] != hs[:-1]
        self.starts = np.flatnonzero(head)
        self.indices = self.order[self.starts].astype(I64)
        self.uniq = hs[self.starts]
        self.count = int(self.starts.shape[0])
        ids_sorted = np.cumsum(head) - 1
        self.ids = np.empty(self.n, I64)
        self.ids[self.order] = ids_sorted
        self.sizes = np.diff(np.append(self.starts, self.n)).astype(I64)

    # what the sorts see: the keys are hash ^ sign bit, compared unsigned
    def keys(self):
        return self.uniq.view(U64) ^ U64(1 << 63)

    def key_bits(self):
        k = self.keys()
        return int(int(k.max()) - int(k.min())).bit_length() if k.size else 0

    def radix_passes(self):
        return (self.key_bits() + 7) // 8

    def slice_occupancy(self):
        """Pairs per slice of the bucket sort, by the rule above bucket_sort_emit_body: slice = (key - min) >> shift with
        shift = bits(max - min) - 6 (0 when fewer than 7 bits differ)."""
        k = self.keys()
        bits = self.key_bits()
        shift = max(bits - 6, 0)
        rel = (k - k.min()) >> U64(shift)
        assert int(rel.max()) < BUCKET_BLOCKS
        return np.bincount(rel.astype(np.int64), minlength=BUCKET_BLOCKS)

    def padded(self, dtype=None):
        """(points [n,3], indices [n], count) of the padded entry points."""
        src = self.points if dtype is None else self.points.astype(dtype)
        pts = np.full((self.n, 3), np.nan, src.dtype)
        idx = np.full(self.n, -1, I64)
        pts[:self.count] = src[self.indices]
        idx[:self.count] = self.indices
        return pts, idx, self.count


def voxel_stats_model(points, model, reverse_in=None, normalise=False):
    """sizes [V], means [V,3] f32, covs [V,3,3] f32 in the operation order of k_voxel_stats: every voxel's members in
    ascending input index, one float32 addition per member and component (member k of every voxel at once: the same
    sequential sums, vectorised ACROSS voxels, never inside one).  `reverse_in` (a voxel id) / `normalise`: the wrong copies."""
    p = np.ascontiguousarray(points, F32)
    V = model.count
    members = model.order.copy()
    starts, sizes = model.starts, model.sizes
    if reverse_in is not None:
        b, e = starts[reverse_in], starts[reverse_in] + sizes[reverse_in]
        members[b:e] = members[b:e][::-1]
    s = np.zeros((V, 3), F32)
    for k in range(int(sizes.max()) if V else 0):
        live = np.flatnonzero(sizes > k)
        s[live] = s[live] + p[members[starts[live] + k]]
    means = (s / sizes.astype(F32)[:, None]).astype(F32)
    c = np.zeros((V, 6), F32)
    pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
    for k in range(int(sizes.max()) if V else 0):
        live = np.flatnonzero(sizes > k)
        d = p[members[starts[live] + k]] - means[live]
        for j, (a, b) in enumerate(pairs):
            c[live, j] = c[live, j] + d[:, a] * d[:, b]
    covs = np.empty((V, 3, 3), F32)
    for j, (a, b) in enumerate(pairs):
        covs[:, a, b] = c[:, j]
        covs[:, b, a] = c[:, j]
    if normalise:
        covs = (covs / sizes.astype(F32)[:, None, None]).astype(F32)
    return sizes.copy(), means, covs


# ----------------------------------------------------------------------------------------------------------------------
# the checks
# ----------------------------------------------------------------------------------------------------------------------
def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def check_hash(out, model):
    """out: voxels [n,3], hashes [n] (icp_voxel_hash, and the same fields of icp_voxel_statistics).  `voxels`: equal to the
    model's; `hashes`: the hash of the voxels HANDED BACK (so that a wrong voxel is named once)."""
    bad = []
    v, h = np.asarray(out["voxels"]), np.asarray(out["hashes"])
    if v.dtype != I64 or not np.array_equal(v, model.voxels):
        bad.append("voxels")
    if h.dtype != I64 or h.shape != (model.n,) or v.shape != (model.n, 3) or not np.array_equal(h, voxel_hashes(v)):
        bad.append("hashes")
    return bad


def check_sample(out, model, source=None):
    """out: indices, points, and — the padded entry points — count; indices / points then hold n rows.  `source`: the rows
    the samples are gathered from (default: the model's points; the batch's float32 copy: their float32 cast).
      count     the count handed back is V;
      samples   the rows in front of the padding are the model's SET of indices, each with the bits of its source row;
      order     their hashes ascend (signed);
      padding   every row behind the count (and behind V, so that a wrong count is named once) is NaN / -1."""
    src = model.points if source is None else source
    idx, pts = np.asarray(out["indices"]), np.asarray(out["points"])
    bad = []
    if "count" in out:
        c = int(out["count"])
        if c != model.count:
            bad.append("count")
        if idx.shape != (model.n,) or pts.shape != (model.n, 3):
            return bad + ["padding"]
        tail_i, tail_p = idx[max(c, model.count):], pts[max(c, model.count):]
        if not (np.all(tail_i == -1) and np.all(np.isnan(tail_p))):
            bad.append("padding")
        m = min(max(c, 0), model.count)
        idx, pts, want = idx[:m], pts[:m], model.indices[:m]
    else:
        want = model.indices
    valid = idx.dtype == I64 and pts.dtype == src.dtype and pts.shape == (idx.shape[0], 3) and \
        (idx.size == 0 or (idx.min() >= 0 and idx.max() < model.n))
    if not valid or not np.array_equal(np.sort(idx), np.sort(want)) or not same_bits(pts, src[idx]):
        bad.append("samples")
    if valid and idx.size > 1:
        h = model.hashes[idx]
        if np.any(h[1:] < h[:-1]):
            bad.append("order")
    return bad


def check_stats(out, model, stats):
    """out: ids [n], count, and — with the normal distribution — sizes, means, covs.  `ids`: the rank of every point's hash;
    `count`: V; `stats`: sizes exactly, means and covariances bit for bit."""
    bad = []
    if not np.array_equal(np.asarray(out["ids"]), model.ids):
        bad.append("ids")
    if int(out["count"]) != model.count:
        bad.append("count")
    if out.get("sizes") is not None:
        sizes, means, covs = stats
        if not (np.array_equal(out["sizes"], sizes) and same_bits(out["means"], means) and same_bits(out["covs"], covs)):
            bad.append("stats")
    return bad


# ----------------------------------------------------------------------------------------------------------------------
# cases: grid sample and voxels
# ----------------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, name, points, voxel, **facts):
        self.name, self.points, self.voxel, self.facts = name, np.ascontiguousarray(points), float(voxel), facts
        self._model = None

    @property
    def n(self):
        return int(self.points.shape[0])

    @property
    def f64(self):
        return self.points.dtype == F64

    @property
    def model(self):
        if self._model is None:
            self._model = SampleModel(self.points, self.voxel)
        return self._model

    def __repr__(self):
        return self.name


def tie_cases():
    """a. p / voxel exactly k + 0.5, k in -3 .. 3 on every axis (0.5 -> 0, 1.5 -> 2, -0.5 -> -0, -1.5 -> -2 among them), then
    the same points one ulp up and one ulp down; float32 and float64 rows, voxel 1.0 and 0.5."""
    out = []
    for dtype in (F32, F64):
        for voxel in (1.0, 0.5):
            k = np.arange(-3, 4)
            g = np.stack(np.meshgrid(k, k, k, indexing="ij"), axis=-1).reshape(-1, 3)
            ties = ((g + 0.5) * voxel).astype(dtype)
            q = ties.astype(F64) / voxel
            assert np.array_equal(q, g + 0.5), "the ties are not exact halves"
            up = np.nextafter(ties, dtype(np.inf))
            down = np.nextafter(ties, dtype(-np.inf))
            pts = np.concatenate([ties, up, down])
            want = np.where(g % 2 == 0, g, g + 1)  # half to even
            assert np.array_equal(voxel_coords(ties, voxel), want)
            assert np.array_equal(voxel_coords(up, voxel), g + 1) and np.array_equal(voxel_coords(down, voxel), g)
            for a, b in ((0.5, 0), (1.5, 2), (-0.5, 0), (-1.5, -2)):
                assert voxel_coords(np.array([[a * voxel] * 3], dtype), voxel)[0, 0] == b
            out.append(Case(f"ties-{np.dtype(dtype).name}-v{voxel}", pts, voxel, ties=ties.shape[0]))
    return out


def _filler(rng, n_voxels, per_voxel, spread=40):
    """per_voxel points in each of n_voxels small-integer voxels (voxel size 1.0), offsets in quarters: exact in float32."""
    v = rng.integers(-spread, spread + 1, (n_voxels, 3))
    pts = np.repeat(v, per_voxel, axis=0) + rng.integers(-1, 2, (n_voxels * per_voxel, 3)) * 0.25
    return pts[rng.permutation(pts.shape[0])].astype(F32)


def collision_case():
    """b. three pairs of voxels v, v + COLLISION_OFFSET with one hash; the partner that comes first in space (v) sits at the
    LATER indices, so that the sample is the far partner's point.  Several points per partner: the statistics merge them."""
    rng = np.random.default_rng(101)
    fill = _filler(rng, 200, 6)
    bases = np.array([[1, 2, 3], [-4, 5, -6], [7, -8, 9]])
    off = np.array(COLLISION_OFFSET)
    assert hash_of(COLLISION_OFFSET) == 0
    n = fill.shape[0] + 24
    pts = np.empty((n, 3), F32)
    slots = rng.permutation(n)
    pair_rows = []
    k = 0
    taken = []
    for j, b in enumerate(bases):
        rows = np.sort(slots[k:k + 8])
        k += 8
        far, near = rows[:4], rows[4:]          # the far partner first in index, the near one (first in space) later
        jit = rng.integers(-1, 2, (8, 3)) * 0.25
        pts[far] = (b + off + jit[:4]).astype(F32)
        pts[near] = (b + jit[4:]).astype(F32)
        pair_rows.append((far, near))
        taken.extend(rows)
    rest = np.setdiff1d(np.arange(n), np.array(taken))
    pts[rest] = fill
    case = Case("collision", pts, 1.0, pairs=pair_rows)
    m = case.model
    for far, near in pair_rows:
        assert len(set(m.hashes[np.concatenate([far, near])].tolist())) == 1, "the partners do not collide"
        assert not np.array_equal(m.voxels[far[0]], m.voxels[near[0]])
        assert far.max() < near.min() and m.voxels[near[0], 0] < m.voxels[far[0], 0]
        assert far[0] in m.indices and not set(near.tolist()) & set(m.indices.tolist())
        assert len(set(m.ids[np.concatenate([far, near])].tolist())) == 1
    return case


def sentinel_cases():
    """c. the voxel whose hash is -1 (the dedupe table's empty key: it rides in a side cell): one such point, several at
    scattered indices (the smallest index has to win the side cell's atomicMin), none."""
    assert hash_of(SENTINEL_VOXEL) == -1
    out = []
    for name, where in (("one", [700]), ("several", [1290, 64, 1023, 65, 511, 300, 1291]), ("none", [])):
        rng = np.random.default_rng(202)
        pts = _filler(rng, 260, 5)
        for w in where:
            pts[w] = (np.array(SENTINEL_VOXEL) + rng.integers(-1, 2, 3) * 0.25).astype(F32)
        case = Case(f"sentinel-{name}", pts, 1.0, where=where)
        m = case.model
        got = np.flatnonzero(m.hashes == -1)
        assert np.array_equal(got, np.sort(where)), "the sentinel voxel is not where the case says"
        assert (m.uniq < -1).any() and (m.uniq >= 0).any()
        if where:
            r = int(np.flatnonzero(m.uniq == -1)[0])
            assert m.uniq[r - 1] < -1 and m.uniq[r + 1] >= 0 and m.indices[r] == min(where)
        out.append(case)
    return out


def wrap_points(v_count, n, seed=303):
    """d. float64 rows with |voxel| up to 1e11 (voxel size 1.0: the coordinates are exact integers): the hashes wrap and
    span more than 2^63, so the sorts see 64 differing bits (eight radix passes, shift 58 in the bucket sort)."""
    rng = np.random.default_rng(seed)
    vox = rng.integers(-10 ** 11, 10 ** 11, (v_count, 3))
    pts = vox[np.arange(n) % v_count].astype(F64)
    return pts[rng.permutation(n)] if n > v_count else pts


def assert_full_range(model):
    assert int(model.uniq.min()) < -(1 << 62) and int(model.uniq.max()) > (1 << 62), "the hashes do not span 2^63"
    assert model.key_bits() == 64 and model.radix_passes() == 8


def wrap_case():
    case = Case("wrap-V300", wrap_points(300, 900), 1.0)
    m = case.model
    assert m.count == 300
    assert_full_range(m)
    exact = (m.voxels.astype(object) * np.array(HASH_MUL, dtype=object)).sum(axis=1)   # Python integers: no wrap
    wrapped = sum(1 for e, h in zip(exact, m.hashes) if e != int(h))
    assert wrapped > m.n // 20 and all(hash_of(v) == int(h) for v, h in zip(m.voxels[:50], m.hashes[:50])), "the sums do not wrap"
    return case


DEDUPE_SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)


def dedupe_cases():
    """e. wave and workgroup edges of k_hash_dedupe: every size with all points in one voxel, with every point its own
    voxel, and with the lanes of a wave alternating between two voxels that come back five waves later — the first
    occurrence of a voxel in another wave and, from 320 rows on, another workgroup than the rest."""
    out = []
    for n in DEDUPE_SIZES:
        i = np.arange(n)
        for kind, ids in (("one", np.zeros(n, int)), ("own", i), ("spread", 2 * ((i // 64) % 5) + (i & 1))):
            vox = np.stack([ids - 3, 2 - ids, 2 * ids - 5], axis=1)
            jit = np.stack([(i % 3) - 1, ((i // 3) % 3) - 1, ((i // 9) % 3) - 1], axis=1) * 0.25
            case = Case(f"dedupe-{kind}-n{n}", (vox + jit).astype(F32), 1.0)
            assert case.model.count == len(set(ids.tolist()))
            out.append(case)
    return out


def bucket_slice_case(v_line):
    """f. v_line voxels on the x axis (the hash is monotone in x there) and one far outlier at x = 300 000 that stretches
    the key range so that the whole line falls into slice 0: its occupancy is v_line."""
    rng = np.random.default_rng(404)
    x = np.concatenate([np.arange(v_line), np.arange(500), [300000]])  # 500 voxels twice: the dedupe has work
    pts = np.zeros((x.shape[0], 3), F32)
    pts[:, 0] = x
    case = Case(f"bucket-slice-{v_line}", pts[rng.permutation(x.shape[0])], 1.0)
    occ = case.model.slice_occupancy()
    assert case.model.count == v_line + 1 and occ[0] == v_line and occ.sum() == v_line + 1 and occ.max() == v_line
    return case


def grid_points(nx, ny, nz, extra=0):
    """nx ny nz (+ extra) points, every one its own voxel (small integers, voxel 1.0)."""
    i = np.arange(nx * ny * nz)
    pts = np.stack([i % nx, (i // nx) % ny, i // (nx * ny)], axis=1).astype(F32)
    if extra:
        pts = np.concatenate([pts, np.stack([np.full(extra, nx + 1.0), np.arange(extra), np.zeros(extra)], axis=1).astype(F32)])
    return pts


def bucket_full_case():
    """f. the padded bucket sort at its largest V: n = V = 262 144, every point its own voxel on the x axis — slices inside
    the LDS list and a slice beyond it (ranked against all V keys) in ONE launch.  The keys span 45 bits, so a slice is
    2^39 / 73856093 = 7443.66 voxels wide: slices 0 .. 62 hold 4090 voxels each (every 1.82nd x), slice 63 the other 4474
    (every 1.6th).  One overflowing slice, and no larger, because that branch costs members x V key reads of ONE workgroup:
    2.3 million per thread here, seconds at the 8 600 members a uniform cloud of this size puts into every other slice."""
    width = 2.0 ** 39 / HASH_MUL[0]
    xs = [int(np.ceil(s * width)) + np.floor(np.arange(4090) * 1.82).astype(np.int64) for s in range(63)]
    xs.append(int(np.ceil(63 * width)) + np.floor(np.arange(PADDED_BUCKET_MAX_N - 63 * 4090) * 1.6).astype(np.int64))
    x = np.concatenate(xs)
    assert x.shape[0] == PADDED_BUCKET_MAX_N and np.all(np.diff(x) > 0) and x[-1] < 2 ** 24
    rng = np.random.default_rng(405)
    pts = np.zeros((x.shape[0], 3), F32)
    pts[:, 0] = x
    case = Case("bucket-full-262144", pts[rng.permutation(pts.shape[0])], 1.0)
    m = case.model
    occ = m.slice_occupancy()
    assert m.count == m.n == PADDED_BUCKET_MAX_N and m.key_bits() == 45
    assert np.array_equal(occ[:63], np.full(63, 4090)) and occ[63] == 4474 > BUCKET_CAP, "not both kinds of slice"
    return case


def exact_switch_cases():
    """g. V = 32 768 (the last bucket sort of the exact path) and V = 32 769 (the first rocPRIM sort), n = V."""
    out = []
    for extra in (0, 1):
        rng = np.random.default_rng(506 + extra)
        pts = grid_points(32, 32, 32, extra)
        case = Case(f"exact-switch-V{pts.shape[0]}", pts[rng.permutation(pts.shape[0])], 1.0)
        assert case.model.count == case.n == EXACT_BUCKET_MAX_V + extra
        out.append(case)
    return out


SORT_EMIT_V = (1, 63, 64, 65, 1023, 1024, 1025, 8191, 8192, 8193, 20000)


def clustered_voxels(v_count):
    """v_count distinct LiDAR-like voxels: a 40 x 40 x 13 block of small integers (few key bits differ)."""
    assert v_count <= 40 * 40 * 13
    i = (np.arange(v_count) * 7919) % (40 * 40 * 13)   # 7919 is prime to 20 800: distinct
    return np.stack([i % 40 - 20, (i // 40) % 40 - 20, i // 1600 - 6], axis=1)


def repeated_case(n, v_count, kind):
    """h. n rows over v_count voxels, built by repeating rows (row i sits in voxel i mod V: the first V rows are the
    samples).  kind `clustered`: float32, few radix passes; `full`: the float64 full-range keys of (d), eight passes."""
    if kind == "clustered":
        base = clustered_voxels(v_count).astype(F32)
    else:
        base = wrap_points(v_count, v_count, seed=707)
    pts = base[np.arange(n) % v_count]
    case = Case(f"repeat-{kind}-n{n}-V{v_count}", pts, 1.0, kind=kind)
    m = case.model
    assert m.count == v_count and np.array_equal(np.sort(m.indices), np.arange(v_count))
    if kind == "full" and v_count >= 63:
        assert_full_range(m)
    return case


def sort_emit_form(v_count):
    """`registers` / `loop`: which form of k_sort_emit a count of V pairs takes."""
    tiles = (v_count + 63) // 64
    return "registers" if (tiles + SORT_WAVES - 1) // SORT_WAVES <= REG_TILES else "loop"


def small_cases():
    """The cases of at most a few thousand rows, in a fixed order."""
    return tie_cases() + [collision_case()] + sentinel_cases() + [wrap_case()] + dedupe_cases() + \
        [bucket_slice_case(4096), bucket_slice_case(4097)]


# ----------------------------------------------------------------------------------------------------------------------
# the de-skew
# ----------------------------------------------------------------------------------------------------------------------
def deskew_alpha(timestamps, limit=None):
    """preprocessing.py:177-185.  `limit`: the wrong copy whose minimum / maximum see the first `limit` values only."""
    ts = np.asarray(timestamps, F64).reshape(-1)
    seen = ts if limit is None else ts[:limit]
    diff = np.max(seen) - np.min(seen)
    return ts * 0 if diff == 0.0 else (ts - np.min(seen)) / (np.max(seen) - np.min(seen))


def deskew_model(points, timestamps, rpose, alpha=None):
    """Distortion.filter as the reference constructs it: scipy's from_matrix, Slerp, as_matrix and a float64 einsum."""
    from scipy.spatial.transform import Rotation, Slerp
    rpose = np.asarray(rpose)
    alpha = deskew_alpha(timestamps) if alpha is None else alpha
    rot_times = Rotation.from_matrix(np.array([np.eye(3, dtype=F64), rpose[:3, :3].astype(F64)]))
    rots = Slerp(np.array([0.0, 1.0]), rot_times)(alpha).as_matrix()
    tr = alpha.reshape(-1, 1) * rpose[:3, 3].astype(F64).reshape(1, 3)
    return np.einsum("nij,nj->ni", rots, np.asarray(points).astype(F64)) + tr


def _inverse3(m):
    """The inverse of a 3x3 matrix by cofactors, in the matrix's own dtype (np.linalg has no longdouble)."""
    c = np.empty_like(m)
    for i in range(3):
        for j in range(3):
            a, b, d, e = (m[(i + 1) % 3, (j + 1) % 3], m[(i + 1) % 3, (j + 2) % 3],
                          m[(i + 2) % 3, (j + 1) % 3], m[(i + 2) % 3, (j + 2) % 3])
            c[j, i] = a * e - b * d
    return c / (m[0, 0] * c[0, 0] + m[0, 1] * c[1, 0] + m[0, 2] * c[2, 0])


def is_orthogonal(m):
    """The test scipy 1.15's Rotation.from_matrix applies before it orthogonalises (found by probing it with G (I + eps S)
    and diag(1 + eps, 1, 1) G: np.isclose(M M^T, I, atol=1e-12) at numpy's default rtol 1e-5)."""
    m = np.asarray(m, F64)
    return bool(np.all(np.isclose(m @ m.T, np.eye(3), atol=1e-12)))


def polar_rotation(m, dtype=F64):
    """The orthogonal factor of m — U V^T of its SVD, the solution of the orthogonal Procrustes problem scipy takes — by
    Newton's iteration X <- (X + X^-T) / 2 (Higham, Functions of Matrices, ch. 8), which needs no LAPACK and runs in any
    dtype; quadratic: a float32 pose (6e-8 from a rotation) is at rounding after two turns."""
    x = np.asarray(m).astype(dtype)
    for _ in range(30):
        nxt = (x + _inverse3(x).T) / 2
        done = np.abs(nxt - x).max() <= 4 * np.finfo(dtype).eps
        x = nxt
        if done:
            break
    return x


def matrix_to_quaternion(m, dtype=F64):
    """Rotation.from_matrix of the scipy this project is pinned on: a matrix that fails is_orthogonal is replaced by its
    orthogonal factor, then Markley's "Unit quaternion from rotation matrix" (2008): the largest of the trace and the three
    diagonal entries picks the formula, the result is normalised.  (x, y, z, w), w >= 0."""
    m = np.asarray(m).astype(dtype) if is_orthogonal(m) else polar_rotation(m, dtype)
    dec = [m[0, 0], m[1, 1], m[2, 2], m[0, 0] + m[1, 1] + m[2, 2]]
    c = int(np.argmax(dec))
    q = np.zeros(4, dtype)
    if c != 3:
        i, j, k = c, (c + 1) % 3, (c + 2) % 3
        q[i] = 1 - dec[3] + 2 * m[i, i]
        q[j] = m[j, i] + m[i, j]
        q[k] = m[k, i] + m[i, k]
        q[3] = m[k, j] - m[j, k]
    else:
        q[0], q[1], q[2] = m[2, 1] - m[1, 2], m[0, 2] - m[2, 0], m[1, 0] - m[0, 1]
        q[3] = 1 + dec[3]
    q = q / np.sqrt((q * q).sum())
    return -q if q[3] < 0 else q


def axis_angle(m, dtype=F64):
    """(axis, theta) of the rotation from_matrix yields for m: what distort_arg hands the kernel."""
    q = matrix_to_quaternion(m, dtype)
    nv = np.sqrt((q[:3] * q[:3]).sum())
    theta = 2 * np.arctan2(nv, q[3])
    return (q[:3] / nv if nv > 0 else np.zeros(3, dtype)), theta


def deskew_generic(points, timestamps, rpose, dtype=F64, alpha=None):
    """The same construction written out (from_matrix -> rotation vector -> alpha x it -> quaternion -> matrix -> sum), in
    `dtype`: float64 agrees with scipy to rounding, np.longdouble gives the model's own error.  alpha is the reference's
    float64 alpha in both: it is data to the rotation.  A given `alpha` may leave [0, 1] (the wrong copies: scipy's Slerp
    refuses those)."""
    alpha = (deskew_alpha(timestamps) if alpha is None else np.asarray(alpha, F64)).astype(dtype)
    rpose = np.asarray(rpose)
    axis, theta = axis_angle(rpose[:3, :3], dtype)
    half = alpha * theta / 2
    w, s = np.cos(half), np.sin(half)
    x, y, z = (axis[k] * s for k in range(3))
    p = np.asarray(points).astype(dtype)
    r = np.empty((alpha.shape[0], 3, 3), dtype)
    r[:, 0, 0], r[:, 0, 1], r[:, 0, 2] = 1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)
    r[:, 1, 0], r[:, 1, 1], r[:, 1, 2] = 2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)
    r[:, 2, 0], r[:, 2, 1], r[:, 2, 2] = 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)
    t = rpose[:3, 3].astype(dtype)
    return (r * p[:, None, :]).sum(axis=2) + alpha[:, None] * t[None, :]


def deskew_raw_log(points, timestamps, rpose, alpha=None):
    """The wrong copy that was the library until this audit: axis and angle from (R - R^T) / 2 and the trace of the RAW
    matrix — right for an exact rotation, off by the pose's rounding for a float32 one."""
    alpha = deskew_alpha(timestamps) if alpha is None else alpha
    rot = np.asarray(rpose)[:3, :3].astype(F64)
    v = 0.5 * np.array([rot[2, 1] - rot[1, 2], rot[0, 2] - rot[2, 0], rot[1, 0] - rot[0, 1]])
    nv = np.linalg.norm(v)
    theta = np.arctan2(nv, 0.5 * (np.trace(rot) - 1.0))
    axis = v / nv if nv > 0 else np.zeros(3)
    phi = alpha * theta
    p = np.asarray(points).astype(F64)
    c, s = np.cos(phi)[:, None], np.sin(phi)[:, None]
    rotated = p * c + np.cross(axis[None, :], p) * s + axis[None, :] * (p @ axis)[:, None] * (1.0 - c)
    return rotated + alpha[:, None] * np.asarray(rpose)[:3, 3].astype(F64)[None, :]


def deskew_error(out, want, points, rpose):
    """Worst per-row |out - want| relative to |p| + |t| (a row with p = 0 and t = 0: absolute)."""
    out, want = np.asarray(out, LD), np.asarray(want, LD)
    if out.shape != want.shape:
        return np.inf
    if out.shape[0] == 0:
        return 0.0
    scale = np.linalg.norm(np.asarray(points).astype(F64), axis=1) + np.linalg.norm(np.asarray(rpose)[:3, 3].astype(F64))
    err = np.sqrt(((out - want) ** 2).sum(axis=1)).astype(F64)
    if not np.all(np.isfinite(err)):
        return np.inf
    return float(np.max(err / np.where(scale > 0, scale, 1.0)))


def check_deskew(out, want, points, rpose, bar=DESKEW_BAR):
    out = np.asarray(out)
    return [] if out.dtype == F64 and deskew_error(out, want, points, rpose) <= bar else ["deskew"]


DESKEW_SIZES = (1, 2, 255, 256, 257, 16383, 16384, 16385, 40000)
DESKEW_THETAS = (0.0, 1e-8, 1e-4, 0.05, 0.3, 1.0)
DESKEW_WIDE_THETAS = (3.0, np.pi - 1e-3, np.pi - 1e-6)   # towards pi, where the raw-matrix log map lost its axis
DESKEW_AXIS = np.array([0.3, -0.5, 0.81])           # a skew axis (normalised below)
DESKEW_T = np.array([1.5, -0.3, 0.2])
TS_KINDS = ("unsorted", "negative", "epoch", "two_valued", "all_equal")
EXTREME_SLOTS = (0, -1, 255, 256, 16384)            # 16 384: the first element of the reduction's second turn


def rotation_about(axis, theta):
    from scipy.spatial.transform import Rotation
    a = np.asarray(axis, F64)
    return Rotation.from_rotvec(a / np.linalg.norm(a) * theta).as_matrix()


def deskew_motions():
    """name -> 4x4 pose: theta about the skew axis with a translation, as the exact float64 matrix (`f64`) and rounded to
    float32 (`f32`: what the frame loop's constant-velocity guess is), and a pure translation."""
    out = {}
    for th in DESKEW_THETAS + DESKEW_WIDE_THETAS:
        m = np.eye(4)
        m[:3, :3] = rotation_about(DESKEW_AXIS, th)
        m[:3, 3] = DESKEW_T
        out[f"theta{th:.8g}-f64"] = m
        out[f"theta{th:.8g}-f32"] = m.astype(F32)
    t = np.eye(4)
    t[:3, 3] = [0.7, 0.1, 0.0]
    out["translation"] = t
    return out


def deskew_points(n, seed=0):
    rng = np.random.default_rng(900 + seed)
    return np.clip(rng.normal(size=(n, 3)) * 40.0, -69.0, 69.0).astype(F32)   # |p| < 120 m


def deskew_timestamps(n, kind, lo_at=None, hi_at=None, seed=0):
    """n float64 timestamps of one kind; the frame's minimum / maximum planted at lo_at / hi_at when given."""
    rng = np.random.default_rng(1000 + seed)
    if kind == "unsorted":
        ts = rng.uniform(0.0, 0.1, n)
    elif kind == "negative":
        ts = -5.0 - rng.uniform(0.0, 0.1, n)
    elif kind == "epoch":
        ts = 1.6e9 + rng.uniform(0.0, 0.1, n)
    elif kind == "two_valued":
        ts = np.where(rng.random(n) < 0.5, 3.0, 3.1)
    elif kind == "all_equal":
        return np.full(n, 7.25)
    else:
        raise AssertionError(kind)
    if lo_at is not None and hi_at is not None and n > 1:
        lo_at, hi_at = lo_at % n, hi_at % n
        if lo_at != hi_at:
            span = ts.max() - ts.min()
            ts[lo_at] = ts.min() - 0.25 * span - 1e-3
            ts[hi_at] = ts.max() + 0.25 * span + 1e-3
            assert int(np.argmin(ts)) == lo_at and int(np.argmax(ts)) == hi_at
    return ts


def deskew_cases():
    """(label, points, timestamps, motion name): every size with every timestamp kind, the motions cycling; every motion at
    257 and 16 385 rows; the minimum and the maximum at every pair of distinct EXTREME_SLOTS the size has."""
    names = list(deskew_motions())
    out, k = [], 0
    for n in DESKEW_SIZES:
        for kind in TS_KINDS:
            out.append((f"n{n}-{kind}", n, kind, None, None, names[k % len(names)]))
            k += 1
    for n in (257, 16385):
        for name in names:
            out.append((f"n{n}-motion", n, "unsorted", None, None, name))
    for n in (257, 16385, 40000):
        slots = [s for s in EXTREME_SLOTS if s < n]
        for lo in slots:
            for hi in slots:
                if lo % n != hi % n:
                    out.append((f"n{n}-min@{lo}-max@{hi}", n, "epoch" if (lo + hi) % 2 else "unsorted", lo, hi,
                                names[k % len(names)]))
                    k += 1
    return out


def build_deskew_case(case, seed=0):
    label, n, kind, lo, hi, name = case
    return deskew_points(n, seed), deskew_timestamps(n, kind, lo, hi, seed), deskew_motions()[name]
