"""CPU: the bit model of the carried map normals (tests/carry_audit.py) against float64, against deliberately wrong copies of
itself and against the bar carried normals were held to before it existed; and the two conditions tests/test_gpu_carry_audit.py
relies on, on the clouds that file uses.

Measured here (numpy, no GPU):
  direction (D)   the model under the alternating 0.1 degree pose on the chain cloud: 5.2e-7 / 2.1e-6 / 1.0e-5 / 3.9e-5 rad after
                  10 / 40 / 200 / 1 000 carries — 0.121 / 0.121 / 0.116 / 0.090 of the derived bound K 7.25 2^-24 (0.88 - 0.65 x
                  2^-24 rad per carry); with every rsqrtf candidate two steps low or high: 0.092 / 0.086 of it after 1 000.
  length (C)      worst | |n|^2 - 1 | over the chain 0.45 - 0.50 of the bound of its branch (0.65 with every candidate two steps low).
  wrong copies    twelve, each reported by the check named for it; with the sums contracted to fma 36.5 % of the carried normals
                  differ in some bit; the threshold on |n| instead of n2 is reported at 39 of the first 40 steps.
  condition (i)   every estimated normal of the 8 192-point LiDAR map, the 4 097-point lattice and the chain cloud has
                  |n2 - 1| <= 2.4e-7 in float32 (two steps of float32 above 1; the branch's threshold is 4e-7) and no -0.0
                  component: the identity carry is bit-exact, the sentence in csrc/hash_grid.hip holds.
  condition (ii)  on the chain cloud both branches occur at every step from the second on: 1.0 % of the rows renormalise at the
                  second step (6 of 600), 2.2 - 19 % from the third on.  This is a property of the CLOUD: of the sixteen 600-point
                  cuts of the LiDAR map at multiples of 500 only the two at 4 000 and 6 500 reach 1 % at the second step (0 - 0.8 %
                  elsewhere), and cuts that are mostly walls (normals with z = 0, which the yaw leaves in their plane) have later
                  steps without a renormalised row at all — the 3.5 - 10 % of a sketch with random unit vectors is not what
                  estimated normals give.  The chain cloud is the cut on which the condition holds.
  the old bar     at the 0.1 degree pose iteration_audit.check_normals passes the carry by the pose instead of its inverse (min
                  |dot| 0.9999931) and the transposed block (0.9999932; the right carry: 0.9999999): the reason this audit exists."""
import numpy as np
import pytest

import carry_audit as C
import map_lifecycle as L

F32 = np.float32


@pytest.fixture(scope="module")
def chain():
    """the chain cloud, its estimated normals, the alternating poses, the model's state after 3 and 4 carries"""
    pts = C.chain_cloud()
    n0 = C.estimated4(pts)
    rels = C.chain_poses(C.CHAIN_STEPS)
    at, share = C.free_run(n0, rels, marks=(3, 4) + C.CHAIN_MARKS)
    perm = np.random.default_rng(3).permutation(len(pts))  # the original index at every cell-sorted position of some grid
    return dict(pts=pts, n0=n0, rels=rels, at=at, share=share, perm=perm)


# ---- the model against float64 ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("steps", C.CHAIN_MARKS)
def test_direction_against_float64(chain, steps):
    worst, ratio = C.check_direction(f"chain of {steps}", chain["n0"], chain["at"][steps], chain["rels"][:steps])
    length = C.check_length(f"chain of {steps}", chain["at"][steps])
    print(f"chain of {steps}: worst angle {worst:.3e} rad = {ratio:.3f} of the derived bound "
          f"({worst / steps / C.U:.2f} x 2^-24 per carry); | |n|^2 - 1 | {length:.3f} of its bound")
    assert 0.0 < ratio <= 1.0 and 0.0 < length <= 1.0


@pytest.mark.parametrize("step", [-C.RSQ_ULPS, C.RSQ_ULPS])
def test_every_rsqrt_candidate_stays_inside_the_bounds(chain, step):
    at, _ = C.free_run(chain["n0"], chain["rels"], step=step, marks=(C.CHAIN_STEPS,))
    worst, ratio = C.check_direction(f"candidates {step:+d}", chain["n0"], at[C.CHAIN_STEPS], chain["rels"])
    length = C.check_length(f"candidates {step:+d}", at[C.CHAIN_STEPS])
    print(f"rsqrtf {step:+d} steps off: direction {ratio:.3f}, length {length:.3f} of the bounds")
    assert ratio <= 1.0 and length <= 1.0


def test_candidates_are_five_neighbouring_floats():
    n2 = np.array([0.9999990, 1.0000010, 1e-40, 1e38, 0.0, np.inf], F32)
    c = np.stack([C.rsqrt_candidate(n2, s) for s in (-2, -1, 0, 1, 2)])
    step = np.diff(c[:, :4].view(np.int32).astype(np.int64), axis=0)
    assert (step == 1).all()
    assert (c[:, 4] == np.inf).all() and (c[:, 5] == 0).all()
    exact = 1.0 / np.sqrt(n2[:4].astype(np.float64))
    assert (np.abs(c[2, :4].astype(np.float64) - exact) <= 0.5 * np.spacing(c[2, :4]).astype(np.float64) * (1 + 1e-9)).all()


def test_bounds_are_what_the_docstring_derives():
    assert 5.7e-7 < C.LENGTH_KEPT < 5.9e-7 and 8.9e-7 < C.LENGTH_RENORMALISED < 9.0e-7
    assert float(C.THRESHOLD) == float(np.array([0x34d6bf95], np.uint32).view(F32)[0])  # the constant in the compiled kernels


# ---- every wrong copy is reported by the check meant for it ----------------------------------------------------------------
def _step_case(chain, pose_name, start):
    before = chain["n0"] if start == 0 else chain["at"][start]
    rel = C.poses()[pose_name]
    return before, rel, C.transform_of(rel)


@pytest.mark.parametrize("wrong,pose_name,start", [
    ("pose_not_inverted", "small", 0), ("pose_not_inverted", "drive", 0), ("block_transposed", "small", 0),
    ("block_transposed", "pitch_half_pi", 3), ("translation_added", "small+far", 0), ("other_contraction", "small", 0),
    ("always_renormalised", "small", 0), ("never_renormalised", "small", 3), ("filed_by_position", "small", 3),
    ("carried_twice", "small", 3)])
def test_wrong_copies_fail_the_bit_check(chain, wrong, pose_name, start):
    before, rel, T = _step_case(chain, pose_name, start)
    right = C.update(before, rel)
    C.check_step(f"{pose_name} from step {start}", before, right, T)
    got = C.update(before, rel, wrong=wrong, orig_of_pos=chain["perm"])
    with pytest.raises(AssertionError, match=r"\[carry bits\]"):
        C.check_bits(f"{wrong} at {pose_name} from step {start}", before, got, T)


def test_other_contraction_moves_a_quarter_of_the_rows(chain):
    before, rel, T = _step_case(chain, "small", 0)
    a, b = C.update(before, rel), C.update(before, rel, wrong="other_contraction")
    share = float((a.view(np.uint32) != b.view(np.uint32)).any(axis=1).mean())
    print(f"with the sums contracted to fma {share * 100:.1f} % of the carried normals differ in some bit")
    assert share > 0.1


def test_threshold_on_the_norm_fails_the_bit_check_within_forty_steps(chain):
    """|sqrt(n2) - 1| > 4e-7 instead of |n2 - 1| > 4e-7 keeps rows the source renormalises (n2 - 1 between 4e-7 and 8e-7)"""
    rows, caught = chain["n0"], []
    for k, rel in enumerate(chain["rels"][:40], 1):
        T = C.transform_of(rel)
        got = C.update(rows, rel, wrong="threshold_on_norm")
        try:
            C.check_bits(f"threshold_on_norm, step {k}", rows, got, T)
        except AssertionError as e:
            assert "[carry bits]" in str(e)
            caught.append(k)
        rows = C.update(rows, rel)
    print(f"threshold on the norm: reported at {len(caught)} of 40 steps, the first at step {caught[:1]}")
    assert caught


def test_never_renormalised_leaves_the_length_bound(chain):
    at, _ = C.free_run(chain["n0"], chain["rels"], wrong="never_renormalised", marks=(C.CHAIN_STEPS,))
    with pytest.raises(AssertionError, match=r"\[length\]"):
        C.check_length("never renormalised, 1 000 steps", at[C.CHAIN_STEPS], np.zeros(len(chain["n0"]), bool))


@pytest.mark.parametrize("wrong", ["pose_not_inverted", "block_transposed"])
def test_wrong_rotations_leave_the_direction_bound(chain, wrong):
    # (alternating a pose and its transpose undoes itself every second step: an odd number of steps shows the mistake)
    at, _ = C.free_run(chain["n0"], chain["rels"][:9], wrong=wrong, marks=(9,))
    with pytest.raises(AssertionError, match=r"\[direction\]"):
        C.check_direction(f"{wrong}, 9 steps", chain["n0"], at[9], chain["rels"][:9])


def test_a_flagged_zero_normal_fails_the_flag_census():
    """the guard as it was (n2 > 0 && sc < inf): 2e19 u comes out as a FLAGGED zero row (n2 = +inf, rsqrtf = 0) and, under a
    pose with no zero in its rotation, an infinite component as a flagged NaN row (inf * 0); under the identity 0 * inf makes
    n2 NaN, which either rule leaves unestimated, as it does a NaN component"""
    names, rows = C.planted_rows()
    for pose_name in ("identity", "small"):
        rel = C.poses()[pose_name]
        T = C.transform_of(rel)
        right = C.update(rows, rel)
        C.check_flags(f"planted rows at {pose_name}", rows, right, T)
        C.check_bits(f"planted rows at {pose_name}", rows, right, T)
        kept = {n for n, r in zip(names, right) if r[3] == 1}
        assert kept == {n for n in names if n.startswith(("length", "axis"))} | {"subnormal n2", "1e19 u"}, kept
        assert np.isfinite(right).all() and (right[right[:, 3] == 1, :3] != 0).any(axis=1).all()
        got = C.update(rows, rel, wrong="zero_flagged")
        bad = {n for n, r in zip(names, got) if r[3] == 1 and (not np.isfinite(r).all() or not r[:3].any())}
        assert bad == {"2e19 u: n2 overflows"} | ({"infinite component"} if pose_name == "small" else set()), bad
        with pytest.raises(AssertionError, match=r"\[flag census\]"):
            C.check_flags(f"zero_flagged at {pose_name}", rows, got, T)


def test_planted_lengths_straddle_the_threshold():
    names, rows = C.planted_rows()
    _, ren = C.carry_rows(np.eye(4, dtype=F32), rows)
    lengths = [r for n, r in zip(names, ren) if n.startswith("length")]
    assert any(lengths) and not all(lengths) and lengths[0] and lengths[-1] and not lengths[8]  # both ends renormalise, 1 does not


def test_a_dropped_normal_and_a_partial_cache(chain):
    before, rel, T = _step_case(chain, "small", 3)
    before = before.copy()
    before[::3] = 0.0                                   # a third of the rows without a normal
    right = C.update(before, rel)
    fb, fa = C.check_flags("partial", before, right, T)
    assert fb == fa == int((before[:, 3] == 1).sum())
    lost = right.copy()
    lost[1] = 0.0
    with pytest.raises(AssertionError, match=r"\[flag census\].*gone"):
        C.check_flags("one normal dropped", before, lost, T)
    appeared = right.copy()
    appeared[0] = (0.0, 0.0, 1.0, 1.0)
    with pytest.raises(AssertionError, match=r"\[flag census\].*unestimated"):
        C.check_flags("one normal out of nowhere", before, appeared, T)
    with pytest.raises(AssertionError, match=r"\[flag census\]"):
        C.check_flags("filed by position", before, C.update(before, rel, wrong="filed_by_position", orig_of_pos=chain["perm"]), T)


@pytest.mark.parametrize("wrong,rule", [("carried_across_insertion", dict(inserted=5)),
                                        ("carried_across_insertion", dict(has_cloud=True)),
                                        ("carried_under_point_to_point", dict(cost="point_to_point"))])
def test_updates_that_must_not_carry(chain, wrong, rule):
    before, rel, T = _step_case(chain, "small", 0)
    right = C.update(before, rel, **dict(rule))
    assert not right.any() and len(right) == len(before) + rule.get("inserted", 0)
    assert C.check_never_carried("cleared", before, right, T) == 0
    with pytest.raises(AssertionError, match=r"\[never carried\]"):
        C.check_never_carried(wrong, before, C.update(before, rel, wrong=wrong, **dict(rule)), T)
    moved = L.move(T, chain["pts"])
    rows = np.arange(0, len(moved), 7)
    with pytest.raises(AssertionError, match=r"\[never carried\].*rotated old normals"):
        some = np.where(np.isin(np.arange(len(before)), rows)[:, None], C.update(before, rel, wrong=wrong, **dict(rule))[:len(before)],
                        F32(0.0))  # (a seventh of the rows still there, as if the rest had been cleared)
        C.check_never_carried(wrong, before, some, T, map_points=moved)


def test_the_rule_of_map_update_body():
    assert C.carries()
    for rule in (dict(carry_normals=0), dict(has_cloud=True), dict(evicted=3), dict(keep=0), dict(grid_valid=False),
                 dict(cost="point_to_point")):
        assert not C.carries(**rule), rule
    before = C.planted_rows()[1]
    assert not C.update(before, np.eye(4, dtype=F32), evicted=2).any() and len(C.update(before, np.eye(4, dtype=F32), evicted=2)) == len(before) - 2
    # a failed registration: the identity whatever pose it left
    assert np.array_equal(C.transform_of(C.poses()["yaw_3rad"], ok=False), np.eye(4, dtype=F32))


# ---- the reason this audit exists ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wrong", ["pose_not_inverted", "block_transposed"])
def test_the_old_bar_passes_a_wrong_rotation_at_small_motion(chain, wrong):
    before, rel, T = _step_case(chain, "small", 0)
    moved = L.move(T, chain["pts"])
    ok_right, dot_right = C.old_bar_passes(moved, C.update(before, rel)[:, :3])
    ok_wrong, dot_wrong = C.old_bar_passes(moved, C.update(before, rel, wrong=wrong)[:, :3])
    print(f"{wrong} at the 0.1 degree pose: check_normals passes it with min |dot| {dot_wrong:.7f} (the right carry: {dot_right:.7f})")
    assert ok_right and ok_wrong and dot_wrong < dot_right
    with pytest.raises(AssertionError, match=r"\[carry bits\]"):
        C.check_bits(wrong, before, C.update(before, rel, wrong=wrong), T)


# ---- the conditions the device file relies on ------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,m", [("lidar", 8192), ("lattice", 4097), ("chain", C.CHAIN_M)])
def test_condition_i_estimated_normals_survive_the_identity(kind, m):
    pts = C.chain_cloud() if kind == "chain" else C.cloud(kind, m)
    est = C.estimated4(pts)
    x, y, z = est[:, 0], est[:, 1], est[:, 2]
    n2 = (x * x + y * y) + z * z
    worst = float(np.abs(n2 - F32(1.0)).max())
    print(f"{kind} {m}: worst |n2 - 1| of an estimated normal {worst:.3e} (threshold {float(C.THRESHOLD):.3e})")
    assert worst <= float(C.THRESHOLD)
    assert not (np.signbit(est[:, :3]) & (est[:, :3] == 0)).any()  # (-0.0 + 0.0 is +0.0: such a component would lose its sign)
    same, ren = C.carry_rows(np.eye(4, dtype=F32), est)
    assert not ren.any() and not (same.view(np.uint32) != est.view(np.uint32)).any()


def test_condition_ii_both_branches_at_every_step_of_the_chain(chain):
    share = np.array(chain["share"])
    print(f"renormalised share per step: first {share[0]:.4f}, second {share[1]:.4f}, from the third on {share[2:].min():.4f} - "
          f"{share[2:].max():.4f}")
    assert share[0] == 0.0                    # the first carry of estimated normals never renormalises (condition (i))
    assert (share[1:] >= 0.01).all() and (share[1:] < 1.0).all()
