"""The kd-tree local map of the library against the bit model of tests/map_lifecycle.py after EVERY update.

The rest of the suite takes the map from the library itself (`map_points()`) or compares its final state once, at 1e-5.
Here scripted lives of the map — evictions of full, one-row and zero-row clouds, all-NaN clouds, NaN and null rows with and
without skip_null, a window of one, `map_set` followed by updates, `map_init`, 40 pose-only moves in a row — run through
every insertion entry point, and behind every operation the library must hold the model's map BIT FOR BIT (the model has
the bits of the reference's own KdTreeLocalMap: tests/test_map_lifecycle.py), answer a search of every map point, 512
displaced points and 64 far points with the model's nearest neighbours (ties within TIE_RTOL, at most MISMATCH_CAP of the
probes), and give normals that pass iteration_audit.check_normals on the model's map.  Behind the operations a script marks
— the first eviction, the eviction of a zero-row cloud, `set_then_update`'s third insertion, a pose-only update — the next
scan is registered and its last iteration audited against the map the MODEL says is there.

tests/test_map_lifecycle.py shows on the CPU that each of these checks fails the wrong copy meant for it, and runs the loop
below (`_run`) on a context that answers from the oracle.  The worst figures of every test are printed and quoted in the
docstrings below (measured on an MI355X; the 23 cases take 24 s together, the slowest 2 s).  No map differed from the
model anywhere: neither the library nor the model had to be changed.
"""
import numpy as np
import pytest

import carry_audit as C
import iteration_audit as A
import map_lifecycle as L

pytestmark = pytest.mark.gpu
F32 = np.float32
ENTRIES = ("host", "device", "staged", "vertex_map", "device_pose")
# what each entry point can express: a registration needs a map (window_one empties it), drift is 40 poses of its own
EXPRESSES = {"host": L.SCRIPTS, "device": L.SCRIPTS, "staged": L.SCRIPTS, "vertex_map": L.SCRIPTS,
             "device_pose": ("window", "set_then_update")}
OPTIONS = (("insert_by_cell", 0), ("carry_normals", 0), ("cell_lists", 1), ("overlap_map_update", 1), ("hoods", 0),
           ("frame_seed", 0), ("num_neighbors_normals", 5))


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (no CPU fallback exists for the product path)")
    return torch


def _ctx(local_map_size, options=(), **kw):
    from pylidar_slam_amd.engine import IcpContext
    ctx = IcpContext(height=L.H, width=L.W, max_num_alignments=L.K_REG, threshold_delta_pose=0.0, scheme=L.SCHEME,
                     sigma=L.SIGMA, local_map_size=local_map_size, **kw)
    for name, value in options:
        ctx.set_option(name, value)
    return ctx


def _valid(cloud, skip_null):
    return cloud[A.valid_rows(cloud, skip_null)]


def _vertex_map(ctx, cloud):
    """The cloud as a 16 x 256 vertex map (`ctx.project` of its valid rows) with a NaN pixel and pixels of norm 0.0099,
    exactly float32(0.01) and 0.0101 — only the last of them enters the map; a cloud without rows: all zeros."""
    rows = _valid(cloud, True)
    if not len(rows):
        return np.zeros((3, L.H, L.W), F32)
    v = np.ascontiguousarray(ctx.project(np.ascontiguousarray(rows)), F32)
    v[:, 0, 0] = (1.0, np.nan, 2.0)
    v[:, 0, 1] = (0.0099, 0.0, 0.0)
    v[:, 0, 2] = (0.0, 0.0101, 0.0)
    v[:, 0, 3] = (0.0, 0.0, 0.01)
    return v


def _apply(torch, ctx, model, op, entry, i, state):
    """One operation through an entry point, on the library and on the model; returns the library's `inserted`."""
    if op.kind == "init":
        ctx.map_init()
        model.init()
        return None
    if op.kind == "set":
        ctx.map_set(torch.from_numpy(op.cloud).cuda() if entry == "device" else op.cloud)
        model.set(op.cloud)
        return None
    rel, cloud = op.rel, op.cloud
    if entry == "device_pose" and len(model):  # (a first cloud has no map to register against: its pose comes from the host)
        return _apply_device_pose(ctx, model, op, i, state)
    if cloud is None:
        ins = ctx.map_update(rel, None)
        model.update(rel, None)
    elif entry in ("host", "device_pose"):
        ins = ctx.map_update(rel, cloud, op.skip_null)
        model.update(rel, cloud, op.skip_null)
    elif entry == "device":
        ins = ctx.map_update(rel, torch.from_numpy(cloud).cuda(), op.skip_null)
        model.update(rel, cloud, op.skip_null)
    elif entry == "staged":
        if i == 3:  # a staged cloud replaced before use: only the second may appear
            ctx.map_stage_cloud(np.ascontiguousarray(cloud[::-1] + F32(1.0)), False)
        ctx.map_stage_cloud(cloud, op.skip_null)
        ins = ctx.map_update_staged(rel)
        model.update(rel, cloud, op.skip_null)
    else:
        vmap = _vertex_map(ctx, cloud)
        ins = ctx.map_update_vertex_map(rel, vmap)
        model.update_vertex_map(rel, vmap)
    return ins


def _apply_device_pose(ctx, model, op, i, state):
    """rel_pose None: the scan of the operation's frame is registered first, the update reads the pose on the device and the
    model takes `res.pose`.  Operation 6 (pose only) runs between register_launch and register_end — where an inserting
    update is refused with the map untouched; operation 3 (inserting) behind a register_launch / register_end pair."""
    scans = state["scans"]
    frame = op.frame if op.frame is not None else state["frame"]
    init = op.rel if op.frame is not None else np.eye(4, dtype=F32)
    state["frame"] = frame
    ctx.set_alignment(L.SCHEME, L.SIGMA, L.K_REG, 0.0)
    if op.cloud is None and i == 6:
        ctx.register_launch(scans[frame], init, skip_null=True)
        with pytest.raises(AssertionError, match="collect the pending registration"):
            ctx.map_update(None, scans[frame][:100])
        ins = ctx.map_update(None, None)  # (the check_state behind this operation shows that the refused cloud left nothing)
        rc, res = A.raw_register_end(ctx)
    elif i == 3:
        ctx.register_launch(scans[frame], init, skip_null=True)
        rc, res = A.raw_register_end(ctx)
        ins = ctx.map_update(None, op.cloud, op.skip_null)
    else:
        rc, res = A.raw_register(ctx, scans[frame], init, True)
        if state.get("before") is not None:
            state["before"] = ctx.map_normals_peek()  # (the cache the update carries: behind the registration, not in front of it)
        ins = ctx.map_update(None, op.cloud, op.skip_null)
    assert rc == A.ICP_OK and res.iterations == L.K_REG, (i, rc, res.iterations)
    state["rel"] = res.pose
    model.update(res.pose, op.cloud, op.skip_null)
    return ins


def _run(torch, name, entry, options=(), worst=None, normals_out=None, **kw):
    s = L.script(name)
    ctx, model = _ctx(s.local_map_size, options, **kw), L.MapModel(s.local_map_size)
    state = dict(scans=s.scans, frame=0)
    figs = dict(share=0.0, mismatches=0, worst_tie=0.0, min_dot=1.0, ratio=0.0, searched=0, registered=0, normal_bits=0,
                carried_bits=0)
    from pylidar_slam_amd.engine import IcpContext
    for i, op in enumerate(s.ops):
        tag = f"{name}/{entry} op {i} ({op.note or op.kind})"
        # a pose-only update of a map with points CARRIES the normals the grid holds (unless "carry_normals" is 0): the cache
        # read back behind it is held to the bit model of tests/carry_audit.py, applied to the cache read back in front of it
        carried = isinstance(ctx, IcpContext) and op.kind == "update" and op.cloud is None and len(model) > 0 and \
            ("carry_normals", 0) not in tuple(options)
        state["before"] = ctx.map_normals_peek() if carried else None
        state["rel"] = op.rel
        ins = _apply(torch, ctx, model, op, entry, i, state)
        if carried:
            fig = C.check_step(tag, state["before"], ctx.map_normals_peek(), C.transform_of(state["rel"]))
            figs["carried_bits"] += fig["flagged"]
        L.check_state(ctx, model, tag, ins)
        figs["ratio"] = max(figs["ratio"], model.check_against_float64())
        if op.register is not None:
            L.check_registration(ctx, model, s.scans[op.register], op.init, tag, worst)
            figs["registered"] += 1
            L.check_state(ctx, model, tag + " behind the registration")
        if L.searched(name, i):
            # behind a "set" or an inserting update the grid was rebuilt and every normal is estimated anew (so it is behind every
            # operation with "carry_normals" 0): those are held to the bit model too; behind a pose-only update they are carried
            # (the oracle-backed context of tests/test_map_lifecycle.py estimates every time, in the reference's arithmetic: the
            # model's float64 bar instead of its bits)
            library = isinstance(ctx, IcpContext)
            estimated = not library or op.cloud is not None or ("carry_normals", 0) in tuple(options)
            fig, _, normals = L.check_search(ctx, model, tag, seed=i, estimated=estimated, bits=library)
            if normals_out is not None:
                normals_out.append(normals)
            if fig is not None:
                figs["searched"] += 1
                for k in ("share", "mismatches", "worst_tie"):
                    figs[k] = max(figs[k], fig[k])
                figs["min_dot"] = min(figs["min_dot"], fig["min_dot"])
                figs["normal_bits"] += fig["normal_bits"]
    assert ctx.handoff_fallbacks() == 0
    ctx.close()
    print(f"{name}/{entry}{' ' + str(options) if options else ''}: {len(s.ops)} operations with the model's bits; "
          f"{figs['searched']} searches, mismatch share <= {figs['share']:.2e} ({figs['mismatches']} probes at most, worst tie "
          f"{figs['worst_tie']:.1e}), min |dot| {figs['min_dot']:.7f}; {figs['registered']} registrations audited; "
          f"float64 ratio {figs['ratio']:.3f}; {figs['normal_bits']} estimated and {figs['carried_bits']} carried normals bit-equal "
          f"to their models")
    return figs


# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,entry", [(n, e) for e in ENTRIES for n in EXPRESSES[e] if n != "drift"])  # (drift: test_drift)
def test_script(torch_cuda, name, entry):
    """Every script through every entry point that can express it: `map_update` with host arrays and with CUDA tensors,
    `map_stage_cloud` + `map_update_staged` (operation 3: a staged cloud replaced before use), `map_update_vertex_map`
    (the clouds projected, a NaN pixel and pixels of norm 0.0099 / float32(0.01) / 0.0101 added) and rel_pose None (the
    device-resident pose of a registration of the frame's scan; the model takes `res.pose`).
    Measured, 11 script x entry cases, 137 operations: the model's bits, counts and `inserted` behind every one of them; 124
    searches without a single neighbour that differs from the model's float64 nearest (of up to 4 332 probes each), min
    |dot| 0.9999999 over the determined neighbourhoods; 24 registrations audited: |ddx| <= 5.6e-17, dloss <= 2.3e-16, no
    neighbour mismatch, pose chain <= 1.9e-9; float64 ratio <= 0.635 of the bound; handoff_fallbacks 0."""
    worst = A.Worst(f"{name}/{entry}")
    _run(torch_cuda, name, entry, worst=worst)
    print(worst)


_DEFAULT = {}


def _default_normals(torch):
    if "window" not in _DEFAULT:
        out = []
        _run(torch, "window", "host", normals_out=out)
        _DEFAULT["window"] = out
    return _DEFAULT["window"]


@pytest.mark.parametrize("option,value", OPTIONS)
def test_options_change_nothing(torch_cuda, option, value):
    """The `window` script under each option that touches the map update or the structures built behind it: the map bits
    and the neighbour indices are the model's; the normals are bit-equal to the default run's for every option that leaves
    their arithmetic alone (all but carry_normals and num_neighbors_normals, which pass check_normals like any others).
    Measured, 7 options x 14 operations: the model's bits everywhere, no neighbour mismatch, the normals of insert_by_cell 0,
    cell_lists 1, overlap_map_update 1, hoods 0 and frame_seed 0 bit-equal to the default run's behind every operation;
    carry_normals 0 and num_neighbors_normals 5: min |dot| 0.9999999; 3 registrations audited each, |ddx| 0."""
    default = _default_normals(torch_cuda)
    got = []
    if option == "num_neighbors_normals":
        _run(torch_cuda, "window", "host", normals_out=got, num_neighbors_normals=value)
    else:
        _run(torch_cuda, "window", "host", options=((option, value),), normals_out=got)
    if option not in ("carry_normals", "num_neighbors_normals"):
        for i, (a, b) in enumerate(zip(got, default)):
            assert (a is None) == (b is None)
            if a is not None:
                both = ~np.isnan(a).any(axis=1) & ~np.isnan(b).any(axis=1)
                assert np.array_equal(np.isnan(a), np.isnan(b)), f"{option}: op {i}"
                why = L.first_difference(a[both], b[both])
                assert why is None, f"{option} = {value}, op {i}: the normals are not those of the default run: {why}"


def test_drift(torch_cuda):
    """A full window, then 40 pose-only moves with alternating poses — a third more than the longest chain a point lives
    through in the published window of 30 key frames: the model's bits behind each move, search and registration behind the
    last, and the distance to the float64 shadow inside the derived bound.
    Measured: the model's bits behind all 43 operations; worst |map - float64 shadow| 0.544 of the bound after 40 moves; the
    search behind the last move without a mismatch, its registration |ddx| 0, dloss 3.5e-16, pose chain 9.3e-10."""
    worst = A.Worst("drift")
    figs = _run(torch_cuda, "drift", "host", worst=worst)
    print(worst)
    print(f"drift: worst |map - float64 shadow| / bound {figs['ratio']:.3f}")
    assert 0.0 < figs["ratio"] <= 1.0 and figs["registered"] == 1


def test_refusals_leave_the_map_alone(torch_cuda):
    """A singular pose, rel_pose None on a context that never registered, `map_update_staged` without a staged cloud, and a
    registration that ends in Invalid Jacobian followed by `map_update(None, None)` (collected first, and enqueued between
    launch and end): each returns its error and the map keeps the model's bits, counts and search structure.
    Measured: every call refused (or, behind the Invalid Jacobian, answered with 0 rows and nothing moved) as stated, bits
    and counts unchanged after each, three searches without a mismatch."""
    from pylidar_slam_amd.engine import InvalidJacobianError
    s = L.script("window")
    ctx, model = _ctx(3), L.MapModel(3)
    for i, op in enumerate(s.ops[:5]):
        assert ctx.map_update(op.rel, op.cloud, op.skip_null) == L.apply(model, op)
    L.check_state(ctx, model, "before the refusals")
    singular = np.eye(4, dtype=F32)
    singular[1] = 0.0
    cloud = s.ops[1].cloud
    for what, call in (("singular pose, a cloud", lambda: ctx.map_update(singular, s.ops[3].cloud)),
                       ("singular pose, pose only", lambda: ctx.map_update(singular, None)),
                       ("rel None, never registered", lambda: ctx.map_update(None, None)),
                       ("rel None with a cloud, never registered", lambda: ctx.map_update(None, cloud)),
                       ("nothing staged", lambda: ctx.map_update_staged(s.ops[5].rel))):
        with pytest.raises(AssertionError):
            call()
        L.check_state(ctx, model, what)
    ctx.map_stage_cloud(cloud)
    with pytest.raises(AssertionError):
        ctx.map_update_staged(singular)
    L.check_state(ctx, model, "singular pose, staged")
    L.check_search(ctx, model, "behind the refusals", seed=4)  # (operation 4 of `window`: its seed)
    ctx.close()

    rel, clouds = L.plane_inputs()  # a jittered grid on z = 0; a move in the plane keeps it there exactly
    ctx, model = _ctx(3), L.MapModel(3)
    for c in clouds:
        assert ctx.map_update(rel, c) == model.update(rel, c)
    assert not model.map[:, 2].any()
    L.check_state(ctx, model, "plane")
    L.check_search(ctx, model, "plane", seed=L.PLANE_SEEDS[0])
    targets = np.ascontiguousarray(model.map[::5] + np.array([0.06, -0.04, 0.125], F32))  # every fifth point lifted
    with pytest.raises(InvalidJacobianError):
        ctx.register(targets)
    assert ctx.map_update(None, None) == 0  # the failed registration moves nothing
    L.check_state(ctx, model, "map_update(None, None) behind an Invalid Jacobian")
    ctx.register_launch(targets)
    assert ctx.map_update(None, None) == 0
    with pytest.raises(InvalidJacobianError):
        ctx.register_end()
    L.check_state(ctx, model, "map_update(None, None) between the launch and the end of an Invalid Jacobian")
    L.check_search(ctx, model, "behind the Invalid Jacobian", seed=L.PLANE_SEEDS[1])
    assert ctx.map_update(rel, None) == 0 and model.update(rel, None) == 0
    L.check_state(ctx, model, "the next update")
    ctx.close()
