"""`-m gpu`: every iteration of the projective registration (k_pm_project_targets, k_pm_iterate, k_sum_solve behind
`pmap_register`) held to the float64 model of tests/projective_iteration_audit.py — row count, the 29 sums, status, step,
loss and pose chain, iteration by iteration (its accounting is shown to bite on the CPU in
tests/test_projective_iteration_audit.py) — then the live threshold and the other builds of the same registration
(`pmap_register_launch`, `IcpBatch.pmap_register_launch` twice in a row) bit for bit against the audited run.  Every case
is a valid call; nothing here provokes a fault.  The 30 sums of an iteration are read from `normal_equations_tensor()`:
`launch_sum_solve` hands ctx->neq to k_sum_solve on the projective path as on the kd-tree path (gauss_newton.hip)."""
import numpy as np
import pytest

import projective_iteration_audit as P

pytestmark = pytest.mark.gpu
F32 = np.float32
CASES = P.cases()
_AUDITED = {}  # case name -> what `_audited` returned
_WORST = {}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (no CPU fallback exists for the product path)")
    return torch


def _audited(case):
    """The case's forced run, audited once per session: (records, (status, result) of run K, targets, initial pose)."""
    if case.name not in _AUDITED:
        ctx = P.device_context(case, case.K)
        mv, mn = ctx.pmap_model()
        init = case.init_pose()
        targets = P.make_targets(case.targets, case.h, case.w, mv, init)
        records, last = P.truncated_runs(ctx, case, targets, init)
        ctx.close()
        worst = _WORST.setdefault(case.family, P.Worst(case.family))
        P.audit_run(case.name, records, mv, mn, targets, case.skip_null, case.scheme, case.sigma, init, 0.0, case.guard, worst)
        _AUDITED[case.name] = (records, last, targets, init)
    return _AUDITED[case.name]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name.replace(" ", "_"))
def test_every_iteration(torch_cuda, case):
    """The case's runs of k = 1 .. K forced iterations, every iteration through projective_iteration_audit.check_iteration.
    Measured on the MI355X, worst per family (|ddx| under its largest bar / relative dloss / worst sum as a share of its
    bound / pose chain), row counts, status and guards exact everywhere:
      shapes   (12 cases, 51 iterations, 3 x 3 an Invalid Jacobian on both sides): 9.8e-10 under 1.9e-9 / 4.2e-16 / 9.7e-3 / 6.0e-8;
      schemes  (14, 84): 3.4e-9 (21 iterations of exp / neighborhood / cauchy with the bar cut to STEP_ATOL) / 4.1e-8
               (cauchy: logf, inside TRANSCENDENTAL_BOUND; 4.2e-16 for the IEEE schemes) / 1.8e-2 / 7.5e-9;
      targets  (12, 72): 4.4e-9 under 7.5e-9 / 3.8e-16 / 4.0e-3 / 1.9e-9;
      windows  (7, 42): 1.5e-8 under 3.0e-8 / 3.3e-16 / 5.2e-3 / 3.9e-8;
      guards   (7, 13, seven of them behind a guard; n = 7 diverges with steps of more than 8 m: half a float32 ulp of the step, 9.5e-7,
               is the bar): 5.8e-7 / 1.1e-16 / 0.17 (six rows) / 6.0e-8.
    The model's own float64 solves are at most 2.2e-15 apart outside the guard family.  No kernel bug found."""
    records, (rc, res), _, _ = _audited(case)
    if not case.guard:
        assert len(records) == case.K == res.iterations and rc == P.ICP_OK
    print(_WORST[case.family])


@pytest.mark.parametrize("name", ["shape 17x33", "shape 5x256"])
def test_fresh_contexts_give_the_audited_runs(torch_cuda, name):
    """The audited runs share one context; K fresh contexts given the same update calls (max_num_alignments = k from the
    start) return the same runs, bit for bit, with the same sums."""
    case = P.case_by_name(name)
    records, _, targets, init = _audited(case)
    for rec in records:
        ctx = P.device_context(case, rec.k)
        rc, res = P.per_call(ctx, targets, init, case.skip_null)
        neq = ctx.normal_equations_tensor().cpu().numpy().copy()
        ctx.close()
        assert rc == rec.status and res.iterations == rec.k and res.num_targets == rec.num_targets
        assert float(res.losses[-1]) == rec.loss and np.array_equal(res.dx[-1], rec.dx) and np.array_equal(res.pose, rec.pose_after)
        assert np.array_equal(neq[:30], rec.neq[:30]), rec.k


@pytest.mark.parametrize("register", [P.per_call, P.launched], ids=["per_call", "launched"])
@pytest.mark.parametrize("name", ["shape 17x33", "shape 64x1024"])
def test_live_threshold(torch_cuda, name, register):
    """Thresholds halfway, geometrically, between consecutive |dx_k| of the audited forced run: per call (the host polls) and
    launched (the device decides) the run stops at the iteration the float32 norms name, converged, with the pose it held
    before that iteration, a bit-prefix of the forced run — and passes the audit with its threshold.  Measured on the MI355X:
    17 x 33 stops at iterations 2, 5 and 6 (thresholds 2.0e-2, 5.0e-3, 3.2e-3; the norms rise once in between), 64 x 1024 at
    2, 3, 4, 5 and 6 (2.5e-2 .. 4.6e-4), both ways; |ddx| of the stopping iteration 8.1e-12 .. 2.3e-10, each within its bar."""
    case = P.case_by_name(name)
    forced, _, targets, init = _audited(case)
    stops = P.thresholds_between(forced)
    assert len(stops) >= 2, [P.norm32(r.dx) for r in forced]
    ctx = P.device_context(case, case.K)
    mv, mn = ctx.pmap_model()
    for threshold, stop_at in stops:
        ctx.set_alignment(case.scheme, case.sigma, case.K, threshold)
        rc, res = register(ctx, targets, init, case.skip_null)
        neq = ctx.normal_equations_tensor().cpu().numpy().copy()
        assert rc == P.ICP_OK and res.iterations == stop_at and res.converged, (threshold, stop_at, res.iterations)
        assert np.array_equal(res.pose[:3].view(np.uint32), forced[stop_at - 1].pose12.view(np.uint32))
        for k in range(stop_at):
            assert float(res.losses[k]) == forced[k].loss and np.array_equal(res.dx[k], forced[k].dx), (threshold, k)
        last = P.Record(stop_at, forced[stop_at - 1].pose12, neq, float(res.losses[-1]), res.dx[-1].copy(), res.num_targets,
                        rc, res.iterations, res.converged, res.pose.copy())
        P.audit_run(f"{name} threshold {threshold:.2e}", [last], mv, mn, targets, case.skip_null, case.scheme, case.sigma,
                    np.vstack([last.pose12, [[0, 0, 0, 1]]]).astype(F32), threshold)
    ctx.close()


def _batch_results(batch):
    from pylidar_slam_amd.engine import InvalidJacobianError
    try:
        return batch.register_end(), []
    except InvalidJacobianError as e:
        return e.results, e.failed


@pytest.mark.parametrize("shape", P.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_other_builds_return_the_audited_run(torch_cuda, shape):
    """At every shape: `pmap_register_launch` + `register_end`, `IcpBatch.pmap_register_launch` with three members of
    different content (the audited targets; every third row of them from the identity; targets that all fall off the image:
    that member ends at its first iteration on the residual guard) and a second batched registration straight after the
    first (the clear-on-read z-buffer must be clean) return the audited run's result bit for bit — the members beside it
    that of their own per-call run."""
    from pylidar_slam_amd.engine import IcpBatch
    case = next(c for c in CASES if c.family == "shapes" and (c.h, c.w) == shape)
    _, audited, targets, init = _audited(case)
    off = P.make_targets("off_image", case.h, case.w, None, init)
    scans = [targets, np.ascontiguousarray(targets[::3]), off]
    inits = [init, np.eye(4, dtype=F32), init]
    ctx = P.device_context(case, case.K)
    singles = [audited] + [P.per_call(ctx, s, i, case.skip_null) for s, i in zip(scans[1:], inits[1:])]
    P.same_result(P.per_call(ctx, targets, init, case.skip_null), audited, "the audited run again, after two others")
    P.same_result(P.launched(ctx, targets, init, case.skip_null), audited, "pmap_register_launch + register_end")
    ctx.close()
    assert singles[2][0] == P.ICP_OK and singles[2][1].iterations == 1 and singles[2][1].converged and \
        singles[2][1].num_targets == 0
    members = [P.device_context(case, case.K) for _ in scans]
    batch = IcpBatch(members)
    for turn in ("first", "second"):
        batch.pmap_register_launch(scans, inits, skip_null=case.skip_null)
        results, failed = _batch_results(batch)
        for b, (rc, res) in enumerate(singles):
            if rc != P.ICP_OK:  # (a member with a singular system: the batch reports it and delivers no result for it)
                assert b in failed, (turn, b)
                continue
            assert b not in failed and results[b] is not None, (turn, b, failed)
            P.same_result((P.ICP_OK, results[b]), (rc, res), f"{turn} batched registration, member {b}")
    batch.close()
    for m in members:
        m.close()
