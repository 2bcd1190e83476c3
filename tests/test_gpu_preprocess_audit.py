"""Frame preprocessing on the device — icp_voxel_hash, icp_grid_sample[_f64], icp_grid_sample_padded[_f64],
icp_voxel_statistics, icp_distort and icp_batch_preprocess (csrc/grid_sample.hip) — against the model of
tests/preprocess_audit.py, on cases that force every code path: exact rounding ties, colliding voxels, the voxel whose hash
is the dedupe table's empty key (the side cell), wrapping hashes over the full 64-bit key range, every wave / workgroup edge
of the dedupe, the bucket sort's LDS list at 4096 and 4097 pairs, the exact path's switch to rocPRIM at V = 32 769, the
padded path's switch to k_sort_emit at n = 262 145 with that kernel's register form (V <= 8192), its loop form and five and
eight radix passes; the de-skew at every edge of its min / max reduction, with float64 and float32 poses.

Integers — voxels, hashes, indices, order, counts, padding, voxel ids — are compared exactly, the voxel statistics bit for
bit, the de-skew at preprocess_audit.DESKEW_BAR (7.6e-15 of |p| + |t|: 4 x the model's own float64-against-longdouble
difference).  Which path a case takes is a property of the case the CPU suite asserts from the model
(tests/test_preprocess_audit.py::test_case_claims), not something read out of the library.  Every test prints its worst
figures."""
import numpy as np
import pytest

import preprocess_audit as P

pytestmark = pytest.mark.gpu
F32, F64, I64 = np.float32, np.float64, np.int64


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (no CPU fallback exists for the product path)")
    return torch


@pytest.fixture(scope="module")
def ctx(torch_cuda):
    """One context for the whole module: every test also shows that a context that has served other sizes before — a larger
    table, a used side cell — gives the model's answer."""
    from pylidar_slam_amd.engine import IcpContext
    c = IcpContext()
    yield c
    c.close()


@pytest.fixture(scope="module")
def families():
    small = P.small_cases()
    fam = {"ties": [c for c in small if c.name.startswith("ties")],
           "collision": [c for c in small if c.name == "collision"],
           "sentinel": [c for c in small if c.name.startswith("sentinel")],
           "wrap": [c for c in small if c.name.startswith("wrap")],
           "dedupe": [c for c in small if c.name.startswith("dedupe")],
           "bucket-slice": [c for c in small if c.name.startswith("bucket-slice")]}
    assert sum(len(v) for v in fam.values()) == len(small)
    return fam


@pytest.fixture(scope="module")
def large():
    """name -> case, built once (tests/test_preprocess_audit.py asserts their claims)."""
    out = [P.bucket_full_case()] + P.exact_switch_cases()
    for kind in ("clustered", "full"):
        out.append(P.repeated_case(P.PADDED_BUCKET_MAX_N, 9000, kind))
        out.extend(P.repeated_case(P.PADDED_BUCKET_MAX_N + 1, v, kind) for v in P.SORT_EMIT_V + (9000,))
    return {c.name: c for c in out}


def _np(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def _entry_points(ctx, torch, case, rows=("f32", "f64")):
    """Every entry point that accepts the case -> name: output dict (numpy), each held to the model.  float32 rows also go
    through the float64 entry points as their exact float64 copy (the same voxels).  `rows`: the float32 entry points,
    the float64 ones, or both."""
    m = case.model
    p64 = np.ascontiguousarray(case.points.astype(F64))
    out = {}

    def held(name, bad):
        assert bad == [], f"{case.name}: {name} fails {bad} (n {m.n}, V {m.count})"

    def exact(name, res, src):
        out[name] = {"indices": _np(res[1]), "points": _np(res[0])}
        held(name, P.check_sample(out[name], m, src))

    def padded(name, res, src):
        out[name] = {"indices": _np(res[1]), "points": _np(res[0]), "count": int(res[2])}
        held(name, P.check_sample(out[name], m, src))

    if not case.f64 and "f32" in rows:
        vox, hashes = ctx.voxel_hash(case.points, case.voxel)
        out["voxel_hash"] = {"voxels": vox, "hashes": hashes}
        held("voxel_hash", P.check_hash(out["voxel_hash"], m))
        dev = torch.from_numpy(case.points).cuda()
        exact("grid_sample host", ctx.grid_sample(case.points, case.voxel), case.points)
        exact("grid_sample cuda", ctx.grid_sample(dev, case.voxel), case.points)
        padded("grid_sample_padded f32", ctx.grid_sample_padded(dev, case.voxel), case.points)
        if m.n <= P.STATS_MAX_ROWS:
            s = ctx.voxel_statistics(case.points, case.voxel)
            out["voxel_statistics"] = {"voxels": s["voxel_coordinates"], "hashes": s["voxel_hashes"], "ids": s["voxel_indices"],
                                       "count": s["num_voxels"], "sizes": s["voxel_sizes"], "means": s["voxel_means"],
                                       "covs": s["voxel_covariances"]}
            held("voxel_statistics", P.check_hash(out["voxel_statistics"], m) +
                 P.check_stats(out["voxel_statistics"], m, P.voxel_stats_model(case.points, m)))
            bare = ctx.voxel_statistics(case.points, case.voxel, with_normal_distribution=False)
            held("voxel_statistics, no distribution",
                 P.check_stats({"ids": bare["voxel_indices"], "count": bare["num_voxels"]}, m, None))
    if "f64" not in rows:
        return out
    dev64 = torch.from_numpy(p64).cuda()
    exact("grid_sample_f64 host", ctx.grid_sample_f64(p64, case.voxel), p64)
    exact("grid_sample_f64 cuda", ctx.grid_sample_f64(dev64, case.voxel), p64)
    padded("grid_sample_padded f64", ctx.grid_sample_padded(dev64, case.voxel), p64)
    return out


def _same_outputs(a, b):
    if a.keys() != b.keys():
        return False
    for name in a:
        for key in a[name]:
            x, y = a[name][key], b[name][key]
            if not (x == y if isinstance(x, int) else P.same_bits(x, y)):
                return False
    return True


# ----------------------------------------------------------------------------------------------------------------------
# grid sample, voxel hash, voxel statistics
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["ties", "collision", "sentinel", "wrap", "dedupe", "bucket-slice"])
def test_small_cases_through_every_entry_point(torch_cuda, ctx, families, family):
    """a-f of the audit: ties (half to even, one ulp either side, float32 and float64 rows), three colliding pairs (one
    sample, one merged voxel, one voxel id per pair), the hash -1 in the side cell (one point, seven scattered ones, none),
    hashes that wrap and span 2^63 (`bits` = 64: shift 58 in the bucket sort), the dedupe at 1 .. 1025 rows, and slice 0 of
    the bucket sort at 4096 pairs (the LDS list's last size) and 4097 (ranked against all keys)."""
    rows = calls = 0
    for case in families[family]:
        out = _entry_points(ctx, torch_cuda, case)
        rows += case.n * len(out)
        calls += len(out)
        extra = ""
        if family == "bucket-slice":
            extra = f", slice occupancy {int(case.model.slice_occupancy().max())} (list {P.BUCKET_CAP})"
        if family in ("wrap", "sentinel"):
            extra = f", key bits {case.model.key_bits()}, side cell used: {bool((case.model.hashes == -1).any())}"
        print(f"{case.name}: n {case.n}, V {case.model.count}, {len(out)} entry points{extra}")
    print(f"{family}: {len(families[family])} cases, {calls} calls, {rows} rows compared, every integer exact, statistics bit-equal")


@pytest.mark.parametrize("rows", ["f32", "f64"])
def test_bucket_sort_at_its_largest(torch_cuda, ctx, large, rows):
    """f. n = V = 262 144 through the padded bucket sort: 63 slices inside the LDS list and one of 4474 pairs ranked against
    all keys in one launch (that one workgroup's 2.3 million key reads per thread are this test's seconds); the exact entry
    points hand the same V to rocPRIM.  The float32 and the float64 entry points are two tests: one padded call each."""
    case = large["bucket-full-262144"]
    occ = case.model.slice_occupancy()
    out = _entry_points(ctx, torch_cuda, case, rows=(rows,))
    print(f"{case.name} {rows}: V {case.model.count}, slices over the list {int((occ > P.BUCKET_CAP).sum())} (largest "
          f"{int(occ.max())}), inside {int(((occ > 0) & (occ <= P.BUCKET_CAP)).sum())}; {len(out)} entry points exact")


@pytest.mark.parametrize("v", [P.EXACT_BUCKET_MAX_V, P.EXACT_BUCKET_MAX_V + 1])
def test_exact_path_switch_to_rocprim(torch_cuda, ctx, large, v):
    """g. V = 32 768: the exact entry points' last bucket sort; V = 32 769: their first rocPRIM sort."""
    case = large[f"exact-switch-V{v}"]
    out = _entry_points(ctx, torch_cuda, case)
    print(f"{case.name}: n {case.n}, V {case.model.count} -> {'bucket sort' if v <= P.EXACT_BUCKET_MAX_V else 'rocPRIM'}; "
          f"{len(out)} entry points exact")


@pytest.mark.parametrize("kind", ["clustered", "full"])
def test_padded_path_switch_and_sort_emit(torch_cuda, ctx, large, kind):
    """h. n = 262 144 (the padded path's last bucket sort) and n = 262 145 (k_sort_emit) over the same 9000 voxels; at
    n = 262 145 every V of SORT_EMIT_V: one pair, the tile edges, the 8192 / 8193 switch between the register and the loop
    form, 20 000, and the 9000 of the other side of the switch.  `clustered`: LiDAR-like keys, five radix passes; `full`: keys over the whole 64-bit range, eight."""
    for n, vs in ((P.PADDED_BUCKET_MAX_N, (9000,)), (P.PADDED_BUCKET_MAX_N + 1, P.SORT_EMIT_V + (9000,))):
        for v in vs:
            case = large[f"repeat-{kind}-n{n}-V{v}"]
            out = _entry_points(ctx, torch_cuda, case)
            route = "bucket sort" if n <= P.PADDED_BUCKET_MAX_N else f"k_sort_emit, {P.sort_emit_form(v)} form"
            print(f"{case.name}: padded -> {route}, {case.model.radix_passes()} passes over {case.model.key_bits()} key bits; "
                  f"{len(out)} entry points exact")


def test_one_context_through_all_cases_equals_fresh_contexts(torch_cuda, ctx, families, large):
    """i. One context through the cases in an order that alternates large and small — a table sized for 262 145 rows in
    front of a one-row frame, a used side cell in front of a frame without the sentinel voxel — then every case on a
    context of its own: bit-equal.  (Every case but bucket-full-262144, whose one overflowing slice takes seconds a call:
    test_bucket_sort_at_its_largest runs it on the module's used context.)"""
    from pylidar_slam_amd.engine import IcpContext
    small = [c for f in ("sentinel", "dedupe", "collision", "wrap", "ties", "bucket-slice") for c in families[f]]
    big = [large[k] for k in ("repeat-full-n262145-V8193", "repeat-clustered-n262144-V9000", "exact-switch-V32769",
                              "repeat-clustered-n262145-V20000", "repeat-full-n262145-V64", "exact-switch-V32768")]
    order = []
    step = max(1, len(small) // len(big))
    for k, c in enumerate(small):
        if k % step == 0 and k // step < len(big):
            order.append(big[k // step])
        order.append(c)
    assert all(b in order for b in big)
    shared = IcpContext()
    first = [_entry_points(shared, torch_cuda, c) for c in order]
    shared.close()
    for c, was in zip(order, first):
        own = IcpContext()
        assert _same_outputs(was, _entry_points(own, torch_cuda, c)), f"{c.name}: a used context answers differently"
        own.close()
    print(f"{len(order)} cases on one context, then each on its own: bit-equal")


def _batch_check(torch, batch, singles, members, stamped, label):
    """One IcpBatch.preprocess of three float32 members (stamped: with all-equal timestamps and a motion — alpha = 0, the
    de-skewed rows are the exact float64 copy of the input, sampled by the float64 path) against the model and the single
    entry points."""
    pose = P.deskew_motions()["theta0.3-f32"]
    pts = [torch.from_numpy(c.points).cuda() for c in members]
    ts = [torch.full((c.n,), 7.25, dtype=torch.float64, device="cuda") if stamped else None for c in members]
    out = batch.preprocess(pts, ts, [pose] * len(members), 1.0)
    torch.cuda.synchronize()
    for c, o, single, p in zip(members, out, singles, pts):
        m = c.model
        src = c.points.astype(F64) if stamped else c.points
        if stamped:
            assert P.same_bits(_np(o["distorted"]), src), f"{label} {c.name}: alpha = 0 moved a point"
        else:
            assert o["distorted"] is None and o["samples"] is o["samples_f32"]
        got = {"indices": _np(o["indices"]), "points": _np(o["samples"]), "count": int(o["count"])}
        bad = P.check_sample(got, m, src)
        got32 = dict(got, points=_np(o["samples_f32"]))
        bad += P.check_sample(got32, m, c.points)
        assert bad == [], f"{label} {c.name}: the batch member fails {bad}"
        alone = single.grid_sample_padded(torch.from_numpy(src).cuda(), 1.0)
        assert P.same_bits(_np(alone[0]), got["points"]) and P.same_bits(_np(alone[1]), got["indices"]) and \
            int(alone[2]) == got["count"], f"{label} {c.name}: the batch member differs from the single call"


@pytest.mark.parametrize("stamped", [False, True], ids=["float32-rows", "deskewed-float64-rows"])
def test_batch_members_equal_the_model_and_the_single_calls(torch_cuda, families, large, stamped):
    """IcpBatch.preprocess with B = 3 members drawn from different cases (voxel 1.0 throughout): every float32 small case
    (the 4096- and 4097-pair slices among them: the batch kernel's LDS list and its overflow branch), a 262 144-row member
    inside the batch launch and a 262 145-row member that leaves the batch for the single path (k_sort_emit, then the
    float32 copy)."""
    from pylidar_slam_amd.engine import IcpBatch, IcpContext
    pool = [c for f in ("collision", "sentinel", "dedupe", "bucket-slice", "ties") for c in families[f]
            if not c.f64 and c.voxel == 1.0]
    pool += [large["repeat-clustered-n262144-V9000"], large["repeat-clustered-n262145-V8193"], large["exact-switch-V32769"]]
    third = (len(pool) + 2) // 3
    ctxs = [IcpContext() for _ in range(3)]
    singles = [IcpContext() for _ in range(3)]
    batch = IcpBatch(ctxs)
    groups = 0
    for k in range(third):
        members = [pool[k], pool[(k + third) % len(pool)], pool[(k + 2 * third) % len(pool)]]
        assert len({c.name.split("-n")[0] for c in members}) > 1 or len({c.n for c in members}) > 1
        _batch_check(torch_cuda, batch, singles, members, stamped, f"group {k}")
        groups += 1
    batch.close()
    for c in ctxs + singles:
        c.close()
    print(f"{groups} batches of 3 over {len(pool)} cases ({'with' if stamped else 'without'} timestamps): members equal the "
          f"model and the single calls")


# ----------------------------------------------------------------------------------------------------------------------
# the de-skew
# ----------------------------------------------------------------------------------------------------------------------
def _deskew_groups():
    cases = P.deskew_cases()
    return {"sizes-and-kinds": [c for c in cases if c[3] is None and not c[0].endswith("motion")],
            "motions": [c for c in cases if c[0].endswith("motion")],
            "extremes": [c for c in cases if c[3] is not None]}


@pytest.mark.parametrize("group", ["sizes-and-kinds", "motions", "extremes"])
def test_deskew_single(torch_cuda, ctx, group):
    """icp_distort against scipy's Slerp (preprocess_audit.deskew_model) at 1 .. 40 000 rows — both sides of the min / max
    reduction's second turn at 16 384 — with unsorted, negative, epoch-sized, two-valued and all-equal timestamps, the
    frame's minimum and maximum at rows 0, n - 1, 255, 256 and 16 384, and rotations of 0 .. 1 rad, 3 rad, pi - 1e-3 and
    pi - 1e-6 about a skew axis as exact float64 matrices and rounded to float32 (the constant-velocity guess of the
    frame loop).

    Bar: DESKEW_BAR = 7.6e-15 of |p| + |t| per row = 4 x 1.9e-15; measured 1.88e-15: the worst difference between the
    model in float64 and in np.longdouble over these cases (the float64 poses alone: 8.3e-16); the kernel's arithmetic in
    numpy (O.distort) differs from the model by 1.14e-15.  Measured on an MI355X: worst 1.96e-15 (sizes and kinds),
    1.80e-15 (motions), 1.56e-15 (extremes), each on a float32 pose; 1.96e-15 in the batches of four."""
    worst, worst32, rows = 0.0, 0.0, 0
    for case in _deskew_groups()[group]:
        p, ts, pose = P.build_deskew_case(case)
        want = P.deskew_model(p, ts, pose)
        host = ctx.distort(p, ts, pose)
        e = P.deskew_error(host, want, p, pose)
        worst = max(worst, e)
        if case[5].endswith("f32"):
            worst32 = max(worst32, e)
        assert P.check_deskew(host, want, p, pose) == [], (case[0], case[5], e, P.DESKEW_BAR)
        dev = ctx.distort(torch_cuda.from_numpy(p).cuda(), torch_cuda.from_numpy(ts).cuda(), pose)
        assert P.same_bits(_np(dev), host), (case[0], "device tensors differ from host arrays")
        rows += p.shape[0]
    print(f"de-skew {group}: {len(_deskew_groups()[group])} cases, {rows} rows, worst {worst:.2e} of |p| + |t| "
          f"(float32 poses {worst32:.2e}) against the bar {P.DESKEW_BAR:.2e}")


def test_deskew_batch_members_keep_their_own_range(torch_cuda):
    """IcpBatch.preprocess with B = 4 de-skewed members of different sizes and timestamp ranges (a reduction that leaked
    across members would apply one member's range to another): every member at DESKEW_BAR of the model, bit-equal to the
    single icp_distort, and its samples the model's sample of the de-skewed rows."""
    from pylidar_slam_amd.engine import IcpBatch, IcpContext
    torch = torch_cuda
    cases = P.deskew_cases()
    quarter = len(cases) // 4
    ctxs = [IcpContext() for _ in range(4)]
    single = IcpContext()
    batch = IcpBatch(ctxs)
    worst, groups = 0.0, 0
    for g in range(0, quarter, 2):
        members = [cases[g + k * quarter] for k in range(4)]
        built = [P.build_deskew_case(c, seed=k) for k, c in enumerate(members)]
        assert len({b[0].shape[0] for b in built}) > 1 and len({(b[1].min(), b[1].max()) for b in built}) > 1
        out = batch.preprocess([torch.from_numpy(b[0]).cuda() for b in built], [torch.from_numpy(b[1]).cuda() for b in built],
                               [b[2] for b in built], 0.5)
        torch.cuda.synchronize()
        for c, (p, ts, pose), o in zip(members, built, out):
            got = _np(o["distorted"])
            want = P.deskew_model(p, ts, pose)
            worst = max(worst, P.deskew_error(got, want, p, pose))
            assert P.check_deskew(got, want, p, pose) == [], (c[0], c[5], P.deskew_error(got, want, p, pose))
            assert P.same_bits(single.distort(p, ts, pose), got), (c[0], "the batch member differs from icp_distort")
            m = P.SampleModel(got, 0.5)
            sample = {"indices": _np(o["indices"]), "points": _np(o["samples"]), "count": int(o["count"])}
            bad = P.check_sample(sample, m) + P.check_sample(dict(sample, points=_np(o["samples_f32"])), m, got.astype(F32))
            assert bad == [], (c[0], bad)
        groups += 1
    batch.close()
    for c in ctxs + [single]:
        c.close()
    print(f"de-skew batch: {groups} batches of 4, worst {worst:.2e} of |p| + |t| against the bar {P.DESKEW_BAR:.2e}")
