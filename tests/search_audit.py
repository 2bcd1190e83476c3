"""The model the exact 1-NN search is held to (csrc/search.hip, search_device.h; the ring loops of knn_device.h / knn.hip),
the clouds that put points at the faces of its own cells, and a host restatement of the ring search whose switches are the
wrong copies the CPU suite turns on.  TEST INFRASTRUCTURE, never imported by the package.

The model.  The nearest neighbour of a query is the minimum of the 64-bit key (bits of d2, original index) over the WHOLE
map, d2 = fma(dz, dz, fma(dy, dy, dx * dx)) of the float32 differences (`consider`, search_device.h) — knn_audit.model_d2
with its fma emulation and its flags, k = 1.  It knows no cells, rings, guards or caches: whatever the schedule, the cell
size and max_rings, the kernel answers this index.  Queries a registration transforms go through `transform_f32`, the
float32 restatement of `transform_point` (fma emulated and flagged the same way); at the identity pose the transform is
exact (fmaf(z, 0, fmaf(y, 0, x * 1)) + 0 = x).

The cells.  A point belongs to the cell floorf(p * inv_h), inv_h = 1.0f / h (`cell_coord`), clamped to +-(2^20 - 8); the
search takes the box of cell c to start at (float)c * h and measures its face gaps from f = p - (float)c * h (`axis_gap`).
For an h that is no power of two the two disagree by a few ulp of the coordinate: a map point can sit in cell k while
lying below (float)k * h, so that the gap to "its" box exceeds its true distance.  `ring_search` restates one level of the
search operation by operation (slack, the library's: every gap short by GAP_SLACK * (|p| + (|o| + 1) * h), DESIGN.md
section 4; slack=False: the gap as computed, compared with `>` — the search before this audit) and the clouds below are
built by SEARCHING, per cell face, for configurations in which the strict copy answers the wrong point.

The clouds.  Functions returning a `Cloud`: (map, queries, h, note) plus the rows of each kind.  The adversarial rows are
embedded in knn_audit.scene()'s sampled map and a share of its queries, so that a registration of the queries against the
map is well conditioned.  One-axis configurations share the other two coordinates (d2 = dx * dx: no fma at all).

The classifier (`classify`) describes the INPUT, not the kernel: whether the query's own cell is empty, how many
candidates the cells hold that a ball of the model's best distance reaches, and whether that ball leaves the 2 x 2 x 2
block of cells nearest the query.  Which tier of the kernel took a query cannot be read from outside.
"""
import numpy as np

import knn_audit as K

F32 = np.float32
CELL_CLAMP = (1 << 20) - 8
COARSE_FACTOR = 4.0
COARSE_RINGS = 6
EXIT_FACTOR = F32(0.999999)
SLACK_MULTIPLE = 16          # every gap is short by SLACK_MULTIPLE * 2^-24 * (|p| + (|o| + 1) * h), DESIGN.md section 4
AUDITED_H = (0.3, 0.37, 0.7, 1.1)
CONTROL_H = 0.5
LANE0 = 60.125               # the adversarial lines run at other-axis coordinates LANE0 + 20 * lane: clear of the scene
FILLER = 2048                # scene queries that keep a registration well conditioned


class Cloud:
    def __init__(self, name, map_pts, queries, h, note, kinds=None, expect=None, first_adv=0, scene_rows=None):
        self.name, self.h, self.note = name, float(h), note
        self.map = np.ascontiguousarray(map_pts, F32)
        self.queries = np.ascontiguousarray(queries, F32)
        self.kinds = kinds or {}          # kind -> rows of `queries`
        self.expect = expect or {}        # query row -> the map index the construction means to be nearest
        self.first_adv = first_adv        # adversarial rows start here (the filler comes first)
        # per query row its row in knn_audit.scene()'s queries, or -1; the map then begins with the sampled scene map
        self.scene_rows = None if scene_rows is None else np.asarray(scene_rows, np.int64)
        assert self.map.shape[0] <= 8192 and self.queries.shape[0] <= 4096, (name, self.map.shape, self.queries.shape)
        self.map.setflags(write=False)
        self.queries.setflags(write=False)


# ---- float32 restatements ----------------------------------------------------------------------------------------------
def inv_of(h):
    return F32(1.0) / F32(h)


def cell_coord(p, h):
    """floorf(p * inv_h) clamped, per coordinate (icp_internal.h: cell_coord); float32 throughout"""
    c = np.floor(np.asarray(p, F32) * inv_of(h))
    return np.clip(c, -CELL_CLAMP, CELL_CLAMP).astype(np.int64)


def cell_coord_f64(p, h):
    """the WRONG membership: floor(p / h) in float64"""
    return np.floor(np.asarray(p, np.float64) / float(F32(h))).astype(np.int64)


def _fma(a32, b32, c32):
    """fmaf(a, b, c) for float32 arrays and where double rounding cannot be excluded (knn_audit._fma_sq for a general
    product: a * b of two float32 is exact in float64)"""
    p64 = np.asarray(a32, F32).astype(np.float64) * np.asarray(b32, F32).astype(np.float64)
    c64 = np.asarray(c32, F32).astype(np.float64)
    s64 = p64 + c64
    unsure = K._near_f32_midpoint(np.abs(s64)) & np.isfinite(s64)
    v = s64 - p64
    exact = ((p64 - (s64 - v)) + (c64 - v)) == 0.0
    with np.errstate(over="ignore"):
        return s64.astype(F32), unsure & ~exact


def transform_f32(pose, pts):
    """p' = p R^T + t as transform_point computes it; returns (points [n, 3] float32, unsure [n])"""
    T = np.asarray(pose, F32).reshape(-1)[:12]
    pts = np.asarray(pts, F32)
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    out = np.empty_like(pts)
    unsure = np.zeros(pts.shape[0], bool)
    for r in range(3):
        a, u1 = _fma(y, np.full_like(y, T[4 * r + 1]), x * T[4 * r])
        b, u2 = _fma(z, np.full_like(z, T[4 * r + 2]), a)
        out[:, r] = b + T[4 * r + 3]
        unsure |= u1 | u2
    return out, unsure


def model_nn(map_pts, queries, pose=None, tie_high=False):
    """Knn (k = 1) of the model; `pose`: the queries are transformed first (rows whose transform is unsure are flagged);
    non-finite query rows have no neighbour.  tie_high: the WRONG copy that gives an exact tie to the higher index."""
    q = np.asarray(queries, F32)
    extra = np.zeros(q.shape[0], bool)
    if pose is not None:
        q, extra = transform_f32(pose, q)
    if tie_high:
        m = np.asarray(map_pts, F32)
        got = K.model_knn(np.ascontiguousarray(m[::-1]), q, 1)
        got.index = np.where(got.index < m.shape[0], m.shape[0] - 1 - got.index, m.shape[0]).astype(np.int32)
    else:
        got = K.model_knn(map_pts, q, 1)
    got.flagged |= extra
    return got


def truth_nn(map_pts, queries):
    """float64 brute force: (d2 [n] float64 of the nearest, its index, d2 of the runner-up)"""
    m64, q64 = np.asarray(map_pts, np.float64), np.asarray(queries, np.float64)
    best = np.empty(q64.shape[0])
    idx = np.empty(q64.shape[0], np.int64)
    second = np.empty(q64.shape[0])
    for lo in range(0, q64.shape[0], 256):
        d = ((m64[None] - q64[lo:lo + 256, None]) ** 2).sum(axis=2)
        i = np.argmin(d, axis=1)
        idx[lo:lo + 256] = i
        best[lo:lo + 256] = d[np.arange(d.shape[0]), i]
        d[np.arange(d.shape[0]), i] = np.inf
        second[lo:lo + 256] = d.min(axis=1)
    return best, idx, second


# ---- the ring search of one level, restated ------------------------------------------------------------------------------
GAP_SLACK = F32(SLACK_MULTIPLE * 2.0 ** -24)


def slack_h(h):
    """search_device.h: slack_h — what every further cell adds to a slackened gap"""
    return F32(h) - GAP_SLACK * F32(h)


def cell_off(p, c, h, slack=True):
    """search_device.h: cell_off — (lo, hi): the distances of p to the lower and the upper face of the box of its cell c,
    short by GAP_SLACK * (|p| + 2 h) (slack False: as the search computed them before the audit, f and h - f)"""
    p, h = np.asarray(p, F32), F32(h)
    f = np.minimum(np.maximum(p - np.asarray(c).astype(F32) * h, F32(0.0)), h)
    s = GAP_SLACK * (np.abs(p) + F32(2.0) * h) if slack else F32(0.0)
    return (f - s).astype(F32), ((h - f) - s).astype(F32)


def axis_gap(o, off, h, slack=True):
    """search_device.h: axis_gap, operation by operation, from `off` = cell_off(..., slack): the distance to the box of the
    cell at offset o on one axis, in all short by GAP_SLACK * (|p| + (|o| + 1) * h) and clamped at 0; scalars or arrays"""
    o = np.asarray(o)
    lo, hi = off
    hs = slack_h(h) if slack else F32(h)
    g = np.where(o < 0, lo + (-o - 1).astype(F32) * hs, hi + (o - 1).astype(F32) * hs).astype(F32)
    g = np.where(o == 0, F32(0.0), np.maximum(g, F32(0.0))).astype(F32)
    return g if g.ndim else F32(g)


def ring_bound(r, h, edge, slack=True):
    """search_device.h: ring_bound — nothing outside the block of rings <= r is closer"""
    return np.maximum(F32(r) * (slack_h(h) if slack else F32(h)) + F32(edge), F32(0.0)).astype(F32)


class Grid:
    """the cells of a map at cell size h: {(cx, cy, cz): map indices ascending}"""

    def __init__(self, map_pts, h, membership=cell_coord):
        self.map, self.h = np.asarray(map_pts, F32), F32(h)
        cells = membership(self.map, h)
        self.cells = {}
        for i, c in enumerate(map(tuple, cells.tolist())):
            self.cells.setdefault(c, []).append(i)


def _d2(grid, idx, q):
    d2, _ = K.model_d2(grid.map[idx], np.asarray(q, F32)[None])
    return d2[0]


def ring_search(grid, q, max_rings, slack=True, prune_ge=False, tie_high=False, exit_factor=True, second_strict=False):
    """`nearest_in_level` for one query: (d2, index, exact, second).  `second` is the lower bound the NN cache would keep on
    every other point: the minimum of the other candidates seen and of the gaps of the pruned cells (taken from the gap the
    prune used: the slackened one under `slack`; second_strict: from the gap as computed, the wrong copy that certifies a hit
    which is none).  The other switches are wrong copies as well."""
    q = np.asarray(q, F32)
    h = grid.h
    c = cell_coord(q, h)
    off = cell_off(q, c, h, slack)
    strict_off = cell_off(q, c, h, False)
    edge = F32(min(np.minimum(off[0], off[1])))
    best, bidx, second = F32(np.inf), 0x7fffffff, F32(np.inf)

    def scan(cell):
        nonlocal best, bidx, second
        idx = grid.cells.get(cell)
        if not idx:
            return
        for d2, i in zip(_d2(grid, idx, q), idx):
            wins = d2 < best or (d2 == best and ((i > bidx) if tie_high else (i < bidx)))
            if bidx == 0x7fffffff or wins:
                second, best, bidx = min(second, best), d2, i
            else:
                second = min(second, d2)

    def shell(r, sl):
        """gap2 = fma(gx, gx, fma(gy, gy, gz * gz)) [oz, oy, ox] over the cube of offsets -r .. r"""
        o = np.arange(-r, r + 1)
        use = off if sl else strict_off
        gx, gy, gz = (axis_gap(o, (use[0][a], use[1][a]), h, sl) for a in range(3))
        n = o.size
        s2, _ = K._fma_sq(np.broadcast_to(gy[None, :], (n, n)).copy(), np.broadcast_to((gz * gz)[:, None], (n, n)).copy())
        g2, _ = K._fma_sq(np.broadcast_to(gx[None, None, :], (n, n, n)).copy(), np.broadcast_to(s2[:, :, None], (n, n, n)).copy())
        return o, g2

    scan(tuple(c.tolist()))
    for r in range(1, max_rings + 1):
        o, g2s = shell(r, slack)
        g2b = shell(r, False)[1] if second_strict else g2s
        on_shell = np.abs(o)[:, None, None] == r
        on_shell = on_shell | (np.abs(o)[None, :, None] == r) | (np.abs(o)[None, None, :] == r)
        # the best only shrinks: what is pruned against the best at the ring's start stays pruned
        gone = on_shell & ((g2s >= best) if prune_ge else (g2s > best))
        if gone.any():
            second = min(second, F32(g2b[gone].min()))
        for iz, iy, ix in np.argwhere(on_shell & ~gone):      # (C order: oz, oy, ox ascending — nearest_in_level's)
            g2 = g2s[iz, iy, ix]
            if g2 >= best if prune_ge else g2 > best:
                second = min(second, g2b[iz, iy, ix])
                continue
            scan((int(c[0]) + int(o[ix]), int(c[1]) + int(o[iy]), int(c[2]) + int(o[iz])))
        bound = ring_bound(r, h, edge, slack)
        b2 = bound * bound * EXIT_FACTOR if exit_factor else bound * bound
        if best <= b2:
            return best, bidx, True, min(second, b2)
    return best, bidx, False, F32(0.0)


def search(cloud_map, q, h, max_rings=2, grids=None, coarse=True, **kw):
    """`nearest_in_grid`: fine rings, coarse rings, exhaustive scan; returns (index, second).  grids: (fine, coarse) made once"""
    fine, crs = grids if grids else (Grid(cloud_map, h, kw.pop("membership", cell_coord)), None)
    kw.pop("membership", None)
    d2, i, exact, second = ring_search(fine, q, max_rings, **kw)
    if exact or not coarse:
        return i, second
    crs = crs or Grid(cloud_map, F32(h) * F32(COARSE_FACTOR))
    d2, i, exact, second = ring_search(crs, q, COARSE_RINGS, **kw)
    if exact:
        return i, F32(0.0)
    d2 = K.model_d2(np.asarray(cloud_map, F32), np.asarray(q, F32)[None])[0][0]           # the exhaustive scan
    at = np.flatnonzero(d2 == d2.min())
    return int(at[-1] if kw.get("tie_high", False) else at[0]), F32(0.0)


def grids_of(map_pts, h, membership=cell_coord):
    return Grid(map_pts, h, membership), Grid(map_pts, F32(h) * F32(COARSE_FACTOR), membership)


# ---- the classifier ------------------------------------------------------------------------------------------------------
def classify(map_pts, queries, h):
    """Describes the INPUT (not the kernel): per query row
         own_empty   no map point shares the query's cell
         candidates  map points in the cells of the 27-neighbourhood whose box (by the computed gaps) a ball of the model's
                     best distance reaches, the own cell included
         leaves      that ball reaches past the 2 x 2 x 2 block of cells nearest the query (past a FARTHER face on some axis,
                     or the best lies beyond ring 1)
    Non-finite rows: own_empty, 0 candidates, leaves."""
    map_pts, q = np.asarray(map_pts, F32), np.asarray(queries, F32)
    hh = F32(h)

    def key(c):
        c = c + (1 << 20)
        return (c[..., 0] << 42) | (c[..., 1] << 21) | c[..., 2]

    cells, counts = np.unique(key(cell_coord(map_pts, h)), return_counts=True)
    ok = np.isfinite(q).all(axis=1)
    qq = np.where(ok[:, None], q, F32(0))
    best = np.full(q.shape[0], np.inf, F32)
    best[ok] = K.model_knn(map_pts, q[ok], 1, sqr=True).dist[:, 0]
    qc = cell_coord(qq, h)
    f, hf = cell_off(qq, qc, h, False)        # the offsets as computed, no slack: this describes the input

    def count_of(c):
        k = key(c)
        at = np.minimum(np.searchsorted(cells, k), cells.shape[0] - 1)
        return np.where(cells[at] == k, counts[at], 0)

    own_empty = (count_of(qc) == 0) | ~ok
    leaves = (np.sqrt(best)[:, None] > np.maximum(f, hf)).any(axis=1) | ~ok
    cand = np.zeros(q.shape[0], np.int64)
    gaps = {-1: f.astype(np.float64), 0: np.zeros(f.shape), 1: hf.astype(np.float64)}   # axis_gap at o = -1, 0, +1
    for oz in (-1, 0, 1):
        for oy in (-1, 0, 1):
            for ox in (-1, 0, 1):
                g2 = gaps[ox][:, 0] ** 2 + gaps[oy][:, 1] ** 2 + gaps[oz][:, 2] ** 2
                cand += np.where(g2 <= best, count_of(qc + np.array([ox, oy, oz])), 0)
    cand[~ok] = 0
    return own_empty, cand, leaves


def per_block(mask, block):
    """how many rows of every `block` consecutive rows have `mask`"""
    n = mask.shape[0]
    pad = (-n) % block
    return np.concatenate((mask, np.zeros(pad, bool))).reshape(-1, block).sum(axis=1)


# ---- construction helpers ------------------------------------------------------------------------------------------------
def _ulps(x, j):
    x = F32(x)
    for _ in range(abs(j)):
        x = np.nextafter(x, F32(np.inf) if j > 0 else F32(-np.inf))
    return x


def _point(axis, v, lane):
    p = np.full(3, F32(LANE0 + 20.0 * lane), F32)
    p[axis] = v
    return p


_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def face_table(h, sign=1, offsets=(2.0e-4, 3.5e-4, 6.0e-4), reach=300.0):
    """Every one-axis triple (k, A, q, C, adversarial) at the faces k = 2 .. reach / h (times `sign`) between cells k - 1 and k:
    A within 8 ulp of float32(k) * h on either side, q a fraction of a millimetre from the face in the neighbouring cell of
    A's, C in q's own cell on the far side of q.  adversarial: d2(A) < d2(C) < gap^2 in float32 — a strict prune of A's cell
    answers C; the others (A on the face or 8 ulp off it, a gap that does not exceed the distance) are controls.
    Vectorised over the faces; the same arithmetic as `cell_coord` and `axis_gap`."""
    def make():
        hh = F32(h)
        ks = sign * np.arange(2, min(int(reach / h), 1000) + 1)
        face = ks.astype(F32) * hh
        steps = [face]
        for _ in range(8):
            steps.append(np.nextafter(steps[-1], F32(np.inf)))
        down = [face]
        for _ in range(8):
            down.append(np.nextafter(down[-1], F32(-np.inf)))
        a = np.stack(down[:0:-1] + steps, axis=1)[:, :, None, None]                      # [k, j = -8 .. 8, 1, 1]
        off = (np.array(offsets, F32)[:, None] * np.array([-1.0, 1.0], F32)[None, :])[None, None]
        q = (face[:, None, None, None] + off).astype(F32)                                 # [k, 1, offset, side]
        ca, cq = cell_coord(a, h), cell_coord(q, h)
        da = a - q
        ok = (np.abs(ca - cq) == 1) & (da * (ca - cq).astype(F32) > 0)
        g = axis_gap(ca - cq, cell_off(q, cq, h, False), h, False)                        # the gap as computed, no slack
        d2a, g2 = da * da, g * g
        adv = ok & (g2 > d2a)
        out = []
        for ki, ji, oi, si in np.argwhere(adv):
            av, qv, d, gg = a[ki, ji, 0, 0], q[ki, 0, oi, si], d2a[ki, ji, oi, si], g2[ki, ji, oi, si]
            for t in (0.5, 0.25, 0.75):
                dc = F32(np.sqrt(np.float64(d) + t * (np.float64(gg) - np.float64(d))))
                cpt = F32(qv - F32(np.sign(av - qv)) * dc)
                dcc = cpt - qv
                if int(cell_coord(cpt, h)) == int(cq[ki, 0, oi, si]) and d < dcc * dcc < gg:
                    out.append((int(ks[ki]), av, qv, cpt, True))
                    break
        ctl = ok & ~adv
        ctl[:, 1:8] = False
        ctl[:, 9:16] = False                                                               # j = -8, 0, 8 only
        for ki, ji, oi, si in np.argwhere(ctl)[::97]:
            av, qv = a[ki, ji, 0, 0], q[ki, 0, oi, si]
            cpt = F32(qv - F32(1.5) * (av - qv))
            if int(cell_coord(cpt, h)) == int(cq[ki, 0, oi, si]):
                out.append((int(ks[ki]), av, qv, cpt, False))
        return out
    return _cached(("face_table", h, sign, offsets, reach), make)


def _spread(items, n):
    """n of `items`, evenly spaced, at most one per face k"""
    seen, uniq = set(), []
    for it in items:
        if it[0] not in seen:
            seen.add(it[0])
            uniq.append(it)
    if len(uniq) <= n:
        return uniq
    return [uniq[i] for i in np.unique(np.linspace(0, len(uniq) - 1, n).round().astype(int))]


def _assemble(name, h, note, adv_map, adv_q, kinds, expect, filler=None):
    """the sampled scene map + the adversarial map rows; `filler` scene queries, then the adversarial queries"""
    _, sq, sampled = K.scene()
    filler = FILLER if filler is None else filler
    step = max(1, sq.shape[0] // filler) if filler else 1
    fill_rows = np.arange(sq.shape[0])[::step][:filler] if filler else np.zeros(0, np.int64)
    fill = sq[fill_rows]
    m0, q0 = sampled.shape[0], fill.shape[0]
    map_pts = np.concatenate((sampled, np.asarray(adv_map, F32).reshape(-1, 3)))
    queries = np.concatenate((fill, np.asarray(adv_q, F32).reshape(-1, 3)))
    kinds = {k: np.asarray(v, np.int64) + q0 for k, v in kinds.items()}
    expect = {r + q0: i + m0 for r, i in expect.items()}
    rows = np.concatenate((fill_rows, np.full(queries.shape[0] - q0, -1, np.int64)))
    return Cloud(name, map_pts, queries, h, note, kinds, expect, first_adv=q0, scene_rows=rows)


# ---- the clouds ----------------------------------------------------------------------------------------------------------
def _adversarial(h, sign=1):
    return [t for t in face_table(h, sign) if t[4]]


def faces(h, per_line=16, filler=None):
    """Face triples on each axis and both signs of the coordinate, |coordinate| 1 .. 300 m, A 0 .. 8 ulp on either side of
    float32(k) * h.  kinds: "adversarial" (a strict-gap prune answers C), "control" (A at the face or 8 ulp off it, no
    disagreement), "bound" (the triple with C at half A's distance: the answer is C and A's cell is rightly pruned, but a
    lower bound on the other points taken from the gap as computed exceeds d2(A)).  In the triples A has the HIGHER original
    index: a scan that meets C first and prunes A's cell keeps C."""
    def make():
        am, aq, kinds, expect = [], [], {"adversarial": [], "control": [], "bound": []}, {}
        lane = 0
        for axis in range(3):
            for sign in (1, -1):
                table = face_table(h, sign)
                picks = _spread([t for t in table if t[4]], per_line) + _spread([t for t in table if not t[4]], 4)
                for k, a, q, cpt, adv in picks:
                    expect[len(aq)] = len(am) + 1
                    am += [_point(axis, cpt, lane), _point(axis, a, lane)]
                    kinds["adversarial" if adv else "control"].append(len(aq))
                    aq.append(_point(axis, q, lane))
                    if adv:   # "bound": C at half A's distance — the answer is C, A's cell is rightly pruned, and the bound
                        expect[len(aq)] = len(am)                     # kept on every other point must not exceed d2(A)
                        am += [_point(axis, F32(q - F32(0.5) * (a - q)), lane + 20), _point(axis, a, lane + 20)]
                        kinds["bound"].append(len(aq))
                        aq.append(_point(axis, q, lane + 20))
                lane += 1
        return _assemble(f"faces h={h}" + _SMALL * (filler is not None), h, "one-axis face triples, three axes, both signs", am,
                         aq, kinds, expect, filler)
    return _cached(("faces", h, per_line, filler), make)


def _strict_answers_first(trial, q, h, max_rings=2):
    """the strict restatement answers trial[0] although the model answers trial[1]"""
    if int(K.model_knn(trial, np.asarray(q, F32)[None], 1).index[0, 0]) != 1:
        return False
    return search(trial, q, h, max_rings, slack=False)[0] == 0


def corners(h, per_kind=24):
    """Two and three axes at a face at once: A across an edge or a corner of the query's cell (gap2 is a sum of two or three
    squares), C in the own cell along the first axis.  Kept where the strict restatement answers C."""
    def make():
        am, aq, kinds, expect = [], [], {"edge": [], "corner": []}, {}
        hh = F32(h)
        for naxes, kind in ((2, "edge"), (3, "corner")):
            for k, a, q, _, _ in _spread(_adversarial(h) + _adversarial(h, -1), 4 * per_kind):
                if len(kinds[kind]) >= per_kind:
                    break
                A, Q = _point(0, a, 40 + naxes), _point(0, q, 40 + naxes)
                A[:naxes], Q[:naxes] = a, q   # the same face on every axis: an edge (2) or a corner (3) of the cell
                d2a = K.model_d2(A[None], Q[None])[0][0, 0]
                cq, ca = cell_coord(Q, h), cell_coord(A, h)
                g2 = (axis_gap(ca - cq, cell_off(Q, cq, h, False), h, False).astype(np.float64) ** 2).sum()
                if not g2 > d2a:
                    continue
                Cp = Q.copy()
                Cp[0] = F32(Q[0] - F32(np.sign(a - q)) * F32(np.sqrt(0.5 * (np.float64(d2a) + g2))))
                if not (cell_coord(Cp, h) == cq).all() or not _strict_answers_first(np.stack((Cp, A)), Q, h):
                    continue
                expect[len(aq)] = len(am) + 1
                am += [Cp, A]
                kinds[kind].append(len(aq))
                aq.append(Q)
        return _assemble(f"corners h={h}", h, "edges and corners: two and three axes at a face", am, aq, kinds, expect)
    return _cached(("corners", h, per_kind), make)


def ties(filler=None):
    """Exact ties across a face.  h = 0.5 (a power of two: boxes and membership agree, every value dyadic): A exactly ON the
    face k (so in cell k), q = face - d in cell k - 1, C = q - d: d2(A) = d2(C) = gap^2 to the bit — pruning with `>=` loses A.
    Every configuration twice: the lower original index across the face ("far_low", the answer is A) and in the own cell
    ("own_low", the answer is C).  "exit_tie": q = face - e, P inside the ring-1 block and B on the box of the first cell ring 1
    does not visit, both exactly 0.5 + e away = the exit bound, B with the lower index: an early exit WITHOUT its 0.999999f
    factor stops at ring 1 with P."""
    def make():
        am, aq, kinds, expect = [], [], {"far_low": [], "own_low": [], "exit_tie": []}, {}
        lane = 50
        for axis in range(3):
            for sign in (1, -1):
                for k in (3, 17, 101, 399):
                    face = F32(sign * k) * F32(0.5)
                    for d in (F32(2.0 ** -12), F32(3 * 2.0 ** -13)):
                        q = F32(face - d)
                        cpt = F32(q - d)
                        for far_low in (True, False):
                            A, Cp = _point(axis, face, lane), _point(axis, cpt, lane)
                            expect[len(aq)] = len(am)
                            am += [A, Cp] if far_low else [Cp, A]
                            kinds["far_low" if far_low else "own_low"].append(len(aq))
                            aq.append(_point(axis, q, lane))
                            lane += 1
        for axis in range(3):                                         # "exit_tie": see the docstring
            for k in (5, 33, 257):
                for e in (F32(2.0 ** -10), F32(3 * 2.0 ** -11)):
                    q = F32(F32(k) * F32(0.5) - e)
                    B, P = _point(axis, F32(k + 1) * F32(0.5), lane), _point(axis, F32(q - (F32(0.5) + e)), lane)
                    expect[len(aq)] = len(am)
                    am += [B, P]
                    kinds["exit_tie"].append(len(aq))
                    aq.append(_point(axis, q, lane))
                    lane += 1
        return _assemble("ties h=0.5" + _SMALL * (filler is not None), 0.5, "exact ties across a face", am, aq, kinds, expect,
                         filler)
    return _cached(("ties", filler), make)


def skew_ties(h=0.3, per_axis=16, filler=None):
    """Ties at a skewed face: A an adversarial face point (in cell k, below float32(k) * h), q = A - d and C = q - d with d 16 ulp
    of A, so that d2(A) and d2(C) have equal bits and gap^2 exceeds them; A has the LOWER original index and is the answer —
    a strict prune keeps C."""
    def make():
        am, aq, kinds, expect = [], [], {"skew": []}, {}
        for axis in range(3):
            n = 0
            for k, a, _, _, _ in _spread([t for t in _adversarial(h) if t[1] > t[2]], 8 * per_axis):
                if n >= per_axis:
                    break
                d = F32(np.spacing(a) * 16)
                q = F32(a - d)
                cpt = F32(q - d)
                cq = int(cell_coord(q, h))
                if int(cell_coord(a, h)) != cq + 1 or int(cell_coord(cpt, h)) != cq or (a - q) != (q - cpt):
                    continue
                g = axis_gap(1, cell_off(q, cq, h, False), h, False)
                if not g * g > d * d:
                    continue
                expect[len(aq)] = len(am)
                am += [_point(axis, a, 56), _point(axis, cpt, 56)]
                kinds["skew"].append(len(aq))
                aq.append(_point(axis, q, 56))
                n += 1
        return _assemble(f"skew ties h={h}" + _SMALL * (filler is not None), h,
                         "ties at a skewed face, the lower index across it", am, aq, kinds, expect, filler)
    return _cached(("skew_tie", h, per_axis, filler), make)


def own_empty(h, per_axis=16):
    """The query's cell holds nothing: q a fraction of a millimetre inside an edge of its cell, A across the face of one axis (an
    adversarial face point), C across the face of another axis, d2(A) < d2(C) < gap^2: three different cells.  Kept where the
    strict restatement answers C."""
    def make():
        am, aq, kinds, expect = [], [], {"adversarial": []}, {}
        hh = F32(h)
        for axis in range(3):
            other = (axis + 1) % 3
            n = 0
            for k, a, q, cpt, _ in _spread(_adversarial(h) + _adversarial(h, -1), 8 * per_axis):
                if n >= per_axis:
                    break
                dc = abs(F32(cpt - q))
                k2 = abs(k) + 3
                base = _ulps(F32(k2) * hh, 16)                    # the other axis: q just above the face of cell k2 ...
                cy = F32(base - dc)                                # ... and C below it, dc from q
                A, Q, Cp = _point(axis, a, 60), _point(axis, q, 60), _point(axis, q, 60)
                A[other] = Q[other] = base
                Cp[other] = cy
                cells = {tuple(cell_coord(p, h)) for p in (A, Q, Cp)}
                if len(cells) != 3 or not _strict_answers_first(np.stack((Cp, A)), Q, h):
                    continue
                expect[len(aq)] = len(am) + 1
                am += [Cp, A]
                kinds["adversarial"].append(len(aq))
                aq.append(Q)
                n += 1
        return _assemble(f"own cell empty h={h}", h, "own cell empty, A and C across faces of two axes", am, aq, kinds, expect)
    return _cached(("own_empty", h, per_axis), make)


def exits(h=0.3, coord=200.0):
    """Ring r and the early exit (r * h + edge)^2 * 0.999999f at a 200 m coordinate, where an ulp (1.5e-5 m) outweighs the 1e-6
    margin.  Per r = 1, 2, 4: q 0.2 mm below a face of the x axis; B in the cell r + 1 across it, an ulp below that cell's
    box (ring r does not visit it), and P in the visited block along y (a small coordinate: a fine lattice) with
    d2(B) < d2(P) <= the bound: an exit at ring r answers P ("adversarial", kept where the strict restatement with
    max_rings = r does).  And P alone, the first 1 .. 8 representable distances BEYOND the bound ("beyond": no exit at ring r)."""
    def make():
        am, aq, kinds, expect = [], [], {"adversarial": [], "beyond": []}, {}
        hh = F32(h)
        slot = 0

        def place(x):
            nonlocal slot
            p = np.array([x, 2.125 + 8.0 * (slot % 6) + h / 2, 2.125 + 8.0 * (slot // 6)], F32)
            slot += 1
            return p

        for r in (1, 2, 4):
            found = 0
            for k in range(int(coord / h), int(coord / h) + 400, 7):
                if found >= 6:
                    break
                b = _ulps(F32(k + r) * hh, -1)
                q = F32(F32(k) * hh - F32(2.0e-4))
                if int(cell_coord(b, h)) != k + r or int(cell_coord(q, h)) != k - 1:
                    continue
                Q = place(q)
                B = Q.copy()
                B[0] = b
                fq = np.minimum(np.maximum(Q - cell_coord(Q, h).astype(F32) * hh, F32(0)), hh)
                bound = F32(r) * hh + F32(min(np.minimum(fq, hh - fq)))
                b2 = bound * bound * EXIT_FACTOR
                db = b - q
                P = Q.copy()
                P[1] = F32(Q[1] - F32(np.sqrt(0.5 * (np.float64(db * db) + np.float64(b2)))))
                if not _strict_answers_first(np.stack((P, B)), Q, h, r):
                    slot -= 1
                    continue
                expect[len(aq)] = len(am) + 1
                am += [P, B]
                kinds["adversarial"].append(len(aq))
                aq.append(Q)
                found += 1
            for j in range(1, 9):                                     # P alone, beyond the bound
                Q = place(F32(F32(int(coord / h) + 500 + 40 * j + r) * hh - F32(2.0e-4)))
                fq = np.minimum(np.maximum(Q - cell_coord(Q, h).astype(F32) * hh, F32(0)), hh)
                bound = F32(r) * hh + F32(min(np.minimum(fq, hh - fq)))
                b2 = bound * bound * EXIT_FACTOR
                P = Q.copy()
                P[1] = F32(Q[1] - bound)
                beyond = 0
                for _ in range(256):
                    dy = P[1] - Q[1]
                    if dy * dy > b2:
                        beyond += 1
                        if beyond == j:
                            break
                    P[1] = _ulps(P[1], -1)
                expect[len(aq)] = len(am)
                am.append(P)
                kinds["beyond"].append(len(aq))
                aq.append(Q)
        return _assemble(f"exits h={h}", h, "the early exit at rings 1, 2 and 4, 200 m", am, aq, kinds, expect)
    return _cached(("exits", h, coord), make)


def coarse(h=0.3):
    """The coarse level (4 h, six rings): face triples on the COARSE cells with the query 1.5 .. 6 m from every map point (no
    fine ring reaches one), and rows beyond every coarse ring (the exhaustive scan)."""
    def make():
        am, aq, kinds, expect = [], [], {"adversarial": [], "control": [], "beyond": []}, {}
        ch = F32(h) * F32(COARSE_FACTOR)
        lane = 100
        for dist in (1.5, 2.5, 4.0, 6.0):
            found = 0
            for k in range(int(40 / ch), int(40 / ch) + 4000):
                if found >= 6:
                    break
                face = F32(k) * ch
                for j in range(1, 9):
                    a = _ulps(face, -j)
                    if int(cell_coord(a, ch)) != k:
                        continue
                    q = F32(a - F32(dist))
                    cq = int(cell_coord(q, ch))
                    g = axis_gap(k - cq, cell_off(q, cq, ch, False), ch, False)
                    da = a - q
                    if not g * g > da * da:
                        continue
                    dc = F32(np.sqrt(0.5 * (np.float64(da * da) + np.float64(g * g))))
                    cpt = F32(q - dc)
                    dcc = cpt - q
                    if not da * da < dcc * dcc < g * g:
                        continue
                    expect[len(aq)] = len(am) + 1
                    am += [_point(1, cpt, lane), _point(1, a, lane)]
                    kinds["adversarial"].append(len(aq))
                    aq.append(_point(1, q, lane))
                    lane += 2
                    found += 1
                    break
        for i, dist in enumerate((1.0, 3.0, 6.0)):                  # controls: a lone point at 1 .. 6 m
            expect[len(aq)] = len(am)
            am.append(_point(2, F32(50.0 + 0.1 * i), lane))
            kinds["control"].append(len(aq))
            aq.append(_point(2, F32(50.0 + 0.1 * i + dist), lane))
            lane += 2
        for i in range(8):                                           # beyond every ring: kilometres from the map
            kinds["beyond"].append(len(aq))
            aq.append(np.array([3000.0 + 10.0 * i, -2500.0, 1000.0 + i], F32))
        return _assemble(f"coarse h={h}", h, "coarse-cell face triples, lone points, the exhaustive scan", am, aq, kinds, expect)
    return _cached(("coarse", h), make)


def far_cells(h=0.05):
    """Coordinates beyond the +-(2^20 - 8) cell clamp at h = 0.05 (52 428 m): map points and queries on both sides of the clamp,
    every axis and sign; all values multiples of 1/4 m (exact differences)."""
    def make():
        rng = np.random.default_rng(5)
        am, aq = [], []
        lim = CELL_CLAMP * 0.05
        for axis in range(3):
            for sign in (1.0, -1.0):
                for base in (lim - 8.0, lim + 40.0, 60000.0):
                    ctr = np.full(3, 16.0 * (1 + axis), np.float64)
                    ctr[axis] = sign * base
                    am.append(ctr + np.round(rng.uniform(-6, 6, (6, 3)) * 4) / 4)
                    aq.append(ctr + np.round(rng.uniform(-8, 8, (6, 3)) * 4) / 4)
        am, aq = np.concatenate(am).astype(F32), np.concatenate(aq).astype(F32)
        return _assemble(f"far cells h={h}", h, "beyond the cell clamp", am, aq, {"far": np.arange(aq.shape[0])}, {})
    return _cached(("far_cells", h), make)


def dense(h=0.3, count=300):
    """One cell with 300 points (more than ball_max 256) on a 2^-10 m lattice; queries inside it and across its six faces."""
    def make():
        rng = np.random.default_rng(11)
        c = np.array([401, 405, 409])
        lo = (c.astype(np.float64) * h)
        steps = int(h * 1024) - 8
        pts = np.unique(rng.integers(4, steps, (count * 2, 3)), axis=0)
        pts = pts[rng.permutation(pts.shape[0])[:count]]
        am = (np.ceil(lo * 1024)[None] + pts) / 1024.0
        am = am.astype(F32)
        assert (cell_coord(am, h) == c[None]).all() and am.shape[0] == count
        qs = (np.ceil(lo * 1024)[None] + rng.integers(-steps, 2 * steps, (192, 3))) / 1024.0 + 2.0 ** -11
        return _assemble(f"dense h={h}", h, "a cell of 300 points", am, qs.astype(F32), {"dense": np.arange(192)}, {})
    return _cached(("dense", h, count), make)


LAYOUT_H = 0.37
LAYOUT_COUNTS = {128: (16, 17, 48, 49, 64, 65, 128, 0), 512: (16, 17, 48, 49, 64, 65, 128, 129), 5120: (256, 257)}


def layout(block):
    """Rows ordered so that block i of `block` consecutive queries (128 or 512; 5120: two blocks of 512) holds exactly
    LAYOUT_COUNTS[block][i] rows whose own cell is empty: the far_min 16, wave_misses 48, ball_lanes 64 / 128 / 256 and
    far_max 128 thresholds of icp_set_option, at and one above.  With "xcd_sectors" 0 the row order is the block order.
    h = 0.37.  The own-cell-empty rows are the adversarial rows of own_empty(0.37) (its map is the map here), spread over the
    blocks, then scene queries whose cell is empty; the rest are scene queries whose cell is occupied."""
    def make():
        h = LAYOUT_H
        src = own_empty(h)
        _, sq, _ = K.scene()
        size = 512 if block == 5120 else block
        empty = _cached(("scene empty", h), lambda: classify(src.map, sq, h)[0])
        adv = src.queries[src.kinds["adversarial"]]
        assert classify(src.map, adv, h)[0].all()
        e_rows, f_rows = list(np.flatnonzero(empty)[::-1]), list(np.flatnonzero(~empty)[::-1])
        adv_rows = list(range(adv.shape[0]))
        rows, srow = [], []
        for n in LAYOUT_COUNTS[block]:
            for _ in range(min(4, n, len(adv_rows))):
                rows.append(adv[adv_rows.pop()])
                srow.append(-1)
            for i in range(size - (len(rows) % size or size) if len(rows) % size else size):
                r = e_rows.pop() if (len(rows) % size) < n else f_rows.pop()
                rows.append(sq[r])
                srow.append(r)
        cl = Cloud(f"layout {block}", src.map, np.stack(rows), h, "own-cell-empty rows counted per workgroup", scene_rows=srow)
        cl.block, cl.counts = size, LAYOUT_COUNTS[block]
        return cl
    return _cached(("layout", block), make)


_SMALL = " small"
SMALL_FILLER = 768
SMALL = {"faces h=0.3 small": lambda: faces(0.3, filler=SMALL_FILLER), "faces h=0.7 small": lambda: faces(0.7, filler=SMALL_FILLER),
         "ties h=0.5 small": lambda: ties(filler=SMALL_FILLER), "skew ties h=0.3 small": lambda: skew_ties(0.3, filler=SMALL_FILLER)}


def small(name):
    """the face and tie clouds with 768 filler rows: the clouds of the tests that evaluate the model at many poses"""
    return SMALL[name]()


def _registry():
    reg = {}
    for h in AUDITED_H + (CONTROL_H,):
        reg[f"faces h={h}"] = lambda h=h: faces(h)
    for h in AUDITED_H:
        reg[f"corners h={h}"] = lambda h=h: corners(h)
        reg[f"own cell empty h={h}"] = lambda h=h: own_empty(h)
    reg["ties h=0.5"] = ties
    for h in (0.3, 0.7):
        reg[f"skew ties h={h}"] = lambda h=h: skew_ties(h)
        reg[f"exits h={h}"] = lambda h=h: exits(h)
        reg[f"coarse h={h}"] = lambda h=h: coarse(h)
    reg["far cells h=0.05"] = far_cells
    reg["dense h=0.3"] = dense
    for block in LAYOUT_COUNTS:
        reg[f"layout {block}"] = lambda block=block: layout(block)
    return reg


CLOUDS = _registry()          # name -> builder; a cloud is built on first use and kept


def cloud(name):
    c = CLOUDS[name]()
    assert c.name == name, (c.name, name)
    return c


def _scene_model():
    """the model of every scene query against the sampled scene map, squared distances — the part every cloud shares"""
    def make():
        _, sq, sampled = K.scene()
        return K.model_knn(sampled, sq, 1, sqr=True)
    return _cached("scene model", make)


def model_of(cloud):
    """The model's answer on a cloud at the identity pose, computed once.  Rows taken from the scene's queries reuse their
    model against the sampled scene map (the head of every cloud's map) and add the cloud's own map rows: the minimum of
    the (d2, index) keys of the two parts, flagged where either part is."""
    def make():
        if cloud.scene_rows is None:
            return model_nn(cloud.map, cloud.queries)
        m0 = K.scene()[2].shape[0]
        assert np.array_equal(cloud.map[:m0], K.scene()[2])
        n, m = cloud.queries.shape[0], cloud.map.shape[0]
        out = K.Knn(np.empty((n, 1), F32), np.empty((n, 1), np.int32), np.zeros(n, bool))
        own = np.flatnonzero(cloud.scene_rows < 0)
        if own.size:
            w = K.model_knn(cloud.map, cloud.queries[own], 1, sqr=True)
            out.dist[own], out.index[own], out.flagged[own] = w.dist, w.index, w.flagged
        sc = np.flatnonzero(cloud.scene_rows >= 0)
        if sc.size:
            base = _scene_model()
            r = cloud.scene_rows[sc]
            d, i, fl = base.dist[r, 0], base.index[r, 0], base.flagged[r].copy()
            if m > m0:
                w = K.model_knn(cloud.map[m0:], cloud.queries[sc], 1, sqr=True)
                wins = w.dist[:, 0] < d                          # (a tie stays with the lower index: the scene's)
                d, i = np.where(wins, w.dist[:, 0], d), np.where(wins, w.index[:, 0] + m0, i)
                fl |= w.flagged
            out.dist[sc, 0], out.index[sc, 0], out.flagged[sc] = d, i, fl
        with np.errstate(invalid="ignore"):
            out.dist = np.sqrt(out.dist)
        return out
    return _cached(("model", cloud.name), make)


def check_indices(index, want, what, neighbours=None, map_pts=None):
    """`index` [n] against the model on every unflagged row; `neighbours` [n, 3] must have the bits of map[index]"""
    index = np.asarray(index).reshape(-1)
    use = ~want.flagged
    bad = np.flatnonzero((index != want.index[:, 0]) & use)
    assert bad.size == 0, (f"{what}: {bad.size} of {int(use.sum())} rows differ from the model, first row {bad[0]}: "
                           f"{int(index[bad[0]])} against {int(want.index[bad[0], 0])}")
    if neighbours is not None:
        got = np.ascontiguousarray(neighbours, F32).view(np.uint32)
        ref = np.ascontiguousarray(np.asarray(map_pts, F32)[index]).view(np.uint32)
        assert np.array_equal(got, ref), f"{what}: a returned neighbour has not the bits of map[index]"
    return int(use.sum()), int((~use).sum())
