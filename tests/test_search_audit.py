"""The search audit on the CPU (tests/search_audit.py): the model against a float64 brute force, the flag caps, what every
cloud is built to contain, the block layouts, the slackened gap swept over every cell face — and each check failing the wrong
copy meant for it on a named cloud."""
import numpy as np
import pytest

import knn_audit as K
import search_audit as S

F32 = np.float32


@pytest.mark.parametrize("name", list(S.CLOUDS))
def test_model_against_float64(name):
    """The model's squared distance is within SQR_BAR_ULP of the float64 truth on every row, and where the model's index is
    not the truth's the two candidates are closer than the model can tell: each is within the bar of its own truth, so
    their true squared distances differ by at most 2 x SQR_BAR_ULP ulp."""
    cloud = S.cloud(name)
    want = S.model_of(cloud)
    best, idx, _ = S.truth_nn(cloud.map, cloud.queries)
    d2 = want.dist[:, 0].astype(np.float64) ** 2   # (the model keeps the distance; squaring it back costs an ulp)
    err = K.ulp_error(d2, best)
    assert err.max() <= K.SQR_BAR_ULP + 1.5, (name, err.max())
    other = np.flatnonzero(want.index[:, 0] != idx)
    if other.size:
        picked = ((cloud.map[want.index[other, 0]].astype(np.float64) - cloud.queries[other].astype(np.float64)) ** 2).sum(axis=1)
        assert K.ulp_error(picked, best[other]).max() <= 2 * K.SQR_BAR_ULP, (name, other[:5])
    assert other.size <= K.AMBIGUOUS_MAX * cloud.queries.shape[0], (name, other.size)


@pytest.mark.parametrize("name", list(S.CLOUDS) + list(S.SMALL))
def test_flag_cap_and_intent(name):
    """At most FLAGGED_MAX of a cloud's rows are flagged, and every constructed row has the neighbour its construction
    means it to have (A for a triple, the lower index for a tie ...) by the MODEL, which knows no cells."""
    cloud = S.cloud(name) if name in S.CLOUDS else S.small(name)
    want = S.model_of(cloud) if name in S.CLOUDS else S.model_nn(cloud.map, cloud.queries)
    assert want.flagged.sum() <= K.FLAGGED_MAX * cloud.queries.shape[0], (name, int(want.flagged.sum()))
    for row, index in cloud.expect.items():
        assert int(want.index[row, 0]) == index and not want.flagged[row], (name, row, int(want.index[row, 0]), index)


def test_adversarial_rows_exist():
    """Every audited cell size has face triples a strict prune gets wrong, on several axes and signs; the power of two has none."""
    for h in S.AUDITED_H:
        cloud = S.cloud(f"faces h={h}")
        assert len(cloud.kinds["adversarial"]) >= 6 and len(cloud.kinds["control"]) >= 12, (h, cloud.kinds)
        assert len(S.cloud(f"corners h={h}").kinds["edge"]) >= 2 and len(S.cloud(f"corners h={h}").kinds["corner"]) >= 2
        assert len(S.cloud(f"own cell empty h={h}").kinds["adversarial"]) >= 3
    assert len(S.cloud("faces h=0.5").kinds["adversarial"]) == 0 and not S._adversarial(0.5) and not S._adversarial(0.5, -1)
    # (found: positive coordinates at h = 0.3, 0.37 and 0.7, negative ones at 0.7 and 1.1 — floorf is not symmetric)
    rows = np.concatenate([S.cloud(f"faces h={h}").queries[S.cloud(f"faces h={h}").kinds["adversarial"]] for h in S.AUDITED_H])
    assert (rows.min(axis=0) < -1).all() and (rows.max(axis=0) > 1).all()
    assert all(S._adversarial(h) for h in (0.3, 0.37, 0.7)) and all(S._adversarial(h, -1) for h in (0.7, 1.1))
    for h in (0.3, 0.7):
        assert len(S.cloud(f"exits h={h}").kinds["adversarial"]) >= 12 and len(S.cloud(f"skew ties h={h}").kinds["skew"]) >= 12
        assert len(S.cloud(f"coarse h={h}").kinds["adversarial"]) >= 12


@pytest.mark.parametrize("block", list(S.LAYOUT_COUNTS))
def test_layout_counts(block):
    """Every workgroup's rows of a layout cloud hold exactly the intended number of own-cell-empty queries (the classifier
    describes the input), the adversarial own-cell-empty rows among them."""
    cloud = S.cloud(f"layout {block}")
    empty, cand, leaves = S.classify(cloud.map, cloud.queries, cloud.h)
    assert tuple(S.per_block(empty, cloud.block)) == cloud.counts
    assert (cloud.scene_rows < 0).sum() >= min(8, sum(cloud.counts)) and empty[cloud.scene_rows < 0].all()
    assert cand.max() <= 256 and leaves.any() and not leaves.all()


def test_classifier_on_known_rows():
    cloud = S.cloud("own cell empty h=0.3")
    rows = cloud.kinds["adversarial"]
    empty, cand, leaves = S.classify(cloud.map, cloud.queries[rows], cloud.h)
    assert empty.all() and (cand >= 1).all()
    dense = S.cloud("dense h=0.3")
    _, cand, _ = S.classify(dense.map, dense.queries[dense.kinds["dense"]], dense.h)
    assert cand.max() >= 300   # more than ball_max 256 candidates in reach
    far = S.cloud("coarse h=0.3")
    _, _, leaves = S.classify(far.map, far.queries[far.kinds["beyond"]], far.h)
    assert leaves.all()


# ---- the restatement: right and wrong copies -----------------------------------------------------------------------------
def _answers(cloud, rows, max_rings=2, membership=S.cell_coord, **kw):
    grids = S.grids_of(cloud.map, cloud.h, membership)
    out = [S.search(cloud.map, cloud.queries[r], cloud.h, max_rings, grids=grids, **kw) for r in rows]
    return np.array([o[0] for o in out]), np.array([o[1] for o in out], F32)


def _rows(cloud, *kinds):
    return np.concatenate([np.asarray(cloud.kinds[k], np.int64) for k in kinds])


RIGHT_COPY = [("faces h=0.3", ("adversarial", "control", "bound")), ("faces h=0.37", ("adversarial",)),
              ("faces h=1.1", ("adversarial", "control")), ("corners h=0.7", ("edge", "corner")),
              ("ties h=0.5", ("far_low", "own_low", "exit_tie")), ("skew ties h=0.3", ("skew",)),
              ("own cell empty h=0.37", ("adversarial",)), ("exits h=0.3", ("adversarial", "beyond")),
              ("coarse h=0.7", ("adversarial", "control", "beyond")), ("far cells h=0.05", ("far",))]


@pytest.mark.parametrize("name,kinds", RIGHT_COPY)
def test_slackened_search_is_the_model(name, kinds):
    """The ring search with slackened gaps answers the model's index on every constructed row, at max_rings 1, 2 and 4, and
    the bound it would hand the NN cache never exceeds the squared distance of the runner-up."""
    cloud = S.cloud(name)
    rows = _rows(cloud, *kinds)[::2]
    want = S.model_of(cloud).index[rows, 0]
    second = K.model_knn(cloud.map, cloud.queries[rows], 2, sqr=True).dist[:, 1]
    for max_rings in (1, 2, 4):
        got, bound = _answers(cloud, rows, max_rings)
        assert np.array_equal(got, want), (name, max_rings, rows[got != want][:5])
        assert (bound <= second).all(), (name, max_rings)


def test_wrong_copy_strict_gap():
    """the gap as computed, compared strictly: answers C on every face triple, edge, corner and empty-cell row"""
    for name, kinds in (("faces h=0.3", ("adversarial",)), ("faces h=1.1", ("adversarial",)), ("corners h=0.37", ("edge", "corner")),
                        ("own cell empty h=0.7", ("adversarial",)), ("skew ties h=0.7", ("skew",))):
        cloud = S.cloud(name)
        rows = _rows(cloud, *kinds)
        got, _ = _answers(cloud, rows, slack=False)
        want = S.model_of(cloud)
        assert (got != want.index[rows, 0]).all(), name
        full = want.index[:, 0].copy()
        full[rows] = got
        with pytest.raises(AssertionError, match="differ from the model"):
            S.check_indices(full, want, name)
    cloud = S.cloud("faces h=0.3")      # the controls are no trouble to it
    rows = _rows(cloud, "control")
    assert np.array_equal(_answers(cloud, rows, slack=False)[0], S.model_of(cloud).index[rows, 0])


def test_wrong_copy_prune_at_equality():
    """`>=` for `>` on the ties at h = 0.5, where the gap is exact: loses A where A has the lower index"""
    cloud = S.cloud("ties h=0.5")
    want = S.model_of(cloud).index[:, 0]
    rows = _rows(cloud, "far_low")
    assert np.array_equal(_answers(cloud, rows, slack=False)[0], want[rows])          # (strict is right at a power of two)
    got, _ = _answers(cloud, rows, slack=False, prune_ge=True)
    assert (got != want[rows]).all()
    own = _rows(cloud, "own_low")
    assert np.array_equal(_answers(cloud, own, slack=False, prune_ge=True)[0], want[own])


def test_wrong_copy_ties_to_the_higher_index():
    cloud = S.cloud("ties h=0.5")
    want = S.model_of(cloud)
    rows = _rows(cloud, "far_low", "own_low", "exit_tie")
    wrong = S.model_nn(cloud.map, cloud.queries, tie_high=True)
    assert (wrong.index[rows, 0] != want.index[rows, 0]).all()
    with pytest.raises(AssertionError, match="differ from the model"):
        S.check_indices(wrong.index[:, 0], want, "ties to the higher index")
    got, _ = _answers(cloud, rows, tie_high=True)
    assert (got != want.index[rows, 0]).all()


def test_wrong_copy_float64_membership():
    """Membership by floor(p / h) in float64 puts A — below float32(k) * h — into the QUERY's cell: the own-cell scan meets
    it, the strict copy is right by accident and not one triple is adversarial any more.  The clouds are built on
    floorf(p * inv_h), the library's membership, and the face table finds nothing without it."""
    cloud = S.cloud("faces h=0.3")
    rows = _rows(cloud, "adversarial")
    got, _ = _answers(cloud, rows, slack=False, membership=S.cell_coord_f64)
    assert np.array_equal(got, S.model_of(cloud).index[rows, 0])
    a = cloud.map[[cloud.expect[r] for r in rows]]
    q = cloud.queries[rows]
    assert (S.cell_coord(a, 0.3) != S.cell_coord(q, 0.3)).any(axis=1).all()
    assert (S.cell_coord_f64(a, 0.3) == S.cell_coord_f64(q, 0.3)).all()


def test_wrong_copy_exit_without_factor():
    """the early exit at `<= bound * bound`: stops at ring 1 with P although B, as far to the bit, has the lower index"""
    cloud = S.cloud("ties h=0.5")
    rows = _rows(cloud, "exit_tie")
    want = S.model_of(cloud).index[rows, 0]
    assert np.array_equal(_answers(cloud, rows, slack=False)[0], want)
    got, _ = _answers(cloud, rows, slack=False, exit_factor=False)
    assert (got != want).all()


def test_wrong_copy_no_coarse_level():
    cloud = S.cloud("coarse h=0.3")
    rows = _rows(cloud, "adversarial", "control", "beyond")
    got, _ = _answers(cloud, rows, coarse=False)
    assert (got != S.model_of(cloud).index[rows, 0]).all()


def test_wrong_copy_stale_cache():
    """the neighbours of the previous pose: a shift of 3e-4 m towards C moves every query of a triple past the middle between
    A and C (they are 4e-4 m apart)"""
    cloud = S.small("faces h=0.3 small")
    pose = np.eye(4, dtype=F32)[:3].copy()
    pose[:, 3] = [-3.0e-4, -3.0e-4, -3.0e-4]
    want = S.model_nn(cloud.map, cloud.queries, pose)
    stale = S.model_nn(cloud.map, cloud.queries)
    rows = _rows(cloud, "adversarial")
    assert (stale.index[rows, 0] != want.index[rows, 0]).sum() >= len(rows) // 4
    with pytest.raises(AssertionError, match="differ from the model"):
        S.check_indices(stale.index[:, 0], want, "stale")


def test_wrong_copy_bound_from_the_unslackened_gap():
    """a lower bound on the other points taken from the gap as computed certifies a hit that is none: on the "bound" rows it
    exceeds d2(A)"""
    cloud = S.cloud("faces h=0.3")
    rows = _rows(cloud, "bound")
    second = K.model_knn(cloud.map, cloud.queries[rows], 2, sqr=True).dist[:, 1]
    got, bound = _answers(cloud, rows)
    assert np.array_equal(got, S.model_of(cloud).index[rows, 0]) and (bound <= second).all()
    got, bound = _answers(cloud, rows, second_strict=True)
    assert np.array_equal(got, S.model_of(cloud).index[rows, 0]) and (bound > second).all()


def test_transform_restatement():
    """the identity is exact; a general pose agrees with float64 to a few ulp of the largest term and is seldom unsure"""
    cloud = S.cloud("faces h=0.3")
    same, unsure = S.transform_f32(np.eye(4, dtype=F32), cloud.queries)
    assert np.array_equal(same.view(np.uint32), cloud.queries.view(np.uint32)) and not unsure.any()
    import icp_oracle as O
    pose = O.build_pose_matrix(np.array([0.05, -0.02, 0.01, 0.001, -0.002, 0.004], F32)).astype(F32)
    got, unsure = S.transform_f32(pose, cloud.queries)
    ref = cloud.queries.astype(np.float64) @ pose[:3, :3].astype(np.float64).T + pose[:3, 3].astype(np.float64)
    assert np.abs(got - ref).max() <= 4 * np.spacing(F32(np.abs(cloud.queries).max())) and unsure.mean() < 1.0e-3


# ---- the slack ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h", S.AUDITED_H + (S.CONTROL_H, 0.05))
def test_slackened_gap_never_exceeds_a_distance(h):
    """Every face k = -400 .. 400, a map point within 8 ulp of float32(k) * h on either side, queries from an ulp to four cells
    off the face on both sides: the slackened gap from the query to the cell `cell_coord` gives the point never exceeds
    their distance as `consider` computes it — squared, in float32, as the prune compares them — so the slackened test prunes
    no cell that holds a nearer point; and the slackened ring bound never exceeds the distance to a point outside the block.
    The gap as computed (no slack) does exceed it at some faces of every h that is no power of two — and, for any h, in the
    cells at the origin, where |q| is far below h and f = q - c * h drops q's low bits."""
    hh = F32(h)
    ks = np.arange(-400, 401)
    face = ks.astype(F32) * hh
    pts = [face]
    for _ in range(8):
        pts.append(np.nextafter(pts[-1], F32(np.inf)))
    for _ in range(8):
        pts.insert(0, np.nextafter(pts[0], F32(-np.inf)))
    a = np.stack(pts, axis=1)[:, :, None]                                             # [k, 17, 1]
    offs = np.array([0.0, 2.0e-4, 3.5e-4, 1.0e-3, 0.25 * h, 0.5 * h, 0.99 * h, h, 1.5 * h, 2.25 * h, 3.0 * h, 3.999 * h], F32)
    q = np.concatenate([face[:, None] + offs[None], face[:, None] - offs[None],
                        np.nextafter(face, F32(np.inf))[:, None], np.nextafter(face, F32(-np.inf))[:, None]], axis=1)[:, None, :]
    ca, cq = S.cell_coord(a, h), S.cell_coord(q, h)
    o = ca - cq
    d = a - q
    d2 = d * d
    worst = 0.0
    for slack in (True, False):
        g = S.axis_gap(o, S.cell_off(q, cq, h, slack), h, slack)
        over = (g * g > d2) & (o != 0)
        if slack:
            assert not over.any(), (h, np.argwhere(over)[:3])
            # the bound of ring r = |o| - 1: the point lies outside the block of rings <= r
            lo, hi = S.cell_off(q, cq, h, True)
            r = np.abs(o) - 1
            bound = np.maximum(r.astype(F32) * S.slack_h(h) + np.minimum(lo, hi), F32(0))
            assert not ((bound * bound * S.EXIT_FACTOR > d2) & (o != 0)).any(), h
        else:
            worst = float(np.max(np.where(over, g - np.abs(d), 0)))
            # (a power of two: only at the origin, where f = q - c * h rounds at the scale of h, not of q)
            assert over[np.abs(ks) > 1].any() == (h != 0.5) and over.any(), (h, int(over.sum()))
    print(f"h = {h}: the gap as computed exceeds the distance by up to {worst:.3g} m")
