"""CPU side of the cloud-to-cloud refiner (icp_refine_*, include/icp_mi355x.h):

* every call is declared with the signature written down here, cites the reference lines it stands for, is exported, bound,
  and reachable as `IcpContext.cloud_refiner` / `CloudRefiner` / `register.install_loop_closure_refinement`;
* the kernel unit and its headers are part of the build;
* what needs no device (csrc/refine_plan.h: every refusal, table and grid sizes, the ring count, the footprint — and
  csrc/refine_device.h: the zero-row filter, the box bound of a cell, the rigid step of the solve kernel) as a stand-alone
  program under -fsanitize=address,undefined, against the rules written down here and the numpy model (tests/refine_audit.py)."""
import ctypes
import inspect
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import refine_audit as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "icp_mi355x.h")
CSRC = os.path.join(ROOT, "pylidar-slam_amd", "csrc")
MAX_INDEX = 2 ** 31 - 1
CITATION = "slam/loop_closure.py:210-225"

SIGNATURES = {
    "icp_default_refine_params": ("void", ["icp_refine_params* params"]),
    "icp_refine_create": ("int", ["icp_ctx* ctx", "int64_t max_target_rows", "int64_t max_source_rows", "double cell_size", "icp_refine** out"]),
    "icp_refine_destroy": ("void", ["icp_refine* refiner"]),
    "icp_refine_set_target": ("int", ["icp_refine* refiner", "const float* xyz", "int64_t n", "int mem", "int32_t flags"]),
    "icp_refine_launch": ("int", ["icp_refine* refiner", "const float* xyz", "int64_t n", "int mem", "const double init[16]",
                                  "const icp_refine_params* params"]),
    "icp_refine_end": ("int", ["icp_refine* refiner", "icp_refine_result* result", "int32_t* correspondence_out", "int out_mem"]),
    "icp_refine_image_rows": ("int", ["icp_refine* refiner", "icp_elevation* image", "const float** xyz_out", "int64_t* n_out"]),
    "icp_refine_history": ("int", ["icp_refine* refiner", "double* transforms_out", "double* sums_out", "int32_t cap"]),
}


def test_every_call_is_declared_cited_exported_and_bound():
    from pylidar_slam_amd import _lib, engine, register
    doc = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", doc, flags=re.S)
    lib = ctypes.CDLL(_lib.library_path())
    for name, (ret, want) in SIGNATURES.items():
        m = re.search(r"(\w+)\s+%s\s*\(([^;]*)\)\s*;" % name, text)
        assert m, f"{name} is not declared"
        args = [re.sub(r"\s+", " ", a).strip() for a in m.group(2).split(",")]
        assert m.group(1) == ret and args == want, (name, m.group(1), args)
        at = doc.index(m.group(0).split("(")[0].strip() + "(")
        comment = doc[doc.rindex("/*", 0, at):at]
        assert CITATION in comment, name  # the comment right in front of the declaration
        assert hasattr(lib, name), f"{name} is not exported"
        restype, argtypes = _lib.EXPORTED_SYMBOLS[name]
        assert len(argtypes) == len(want) and restype is (None if ret == "void" else ctypes.c_int), name
    assert sorted(n for n in _lib.EXPORTED_SYMBOLS if "refine" in n) == sorted(SIGNATURES)
    # the structs: field by field as the header has them, sizes pinned
    params = re.search(r"typedef struct \{([^}]*)\} icp_refine_params;", text).group(1)
    assert re.findall(r"(double|int32_t) (\w+);", params) == [("double", "max_distance"), ("double", "relative_fitness"), ("double", "relative_rmse"),
                                                              ("int32_t", "max_iteration"), ("int32_t", "flags")]
    assert [f for f, _ in _lib.IcpRefineParams._fields_] == [n for _, n in re.findall(r"(double|int32_t) (\w+);", params)]
    assert ctypes.sizeof(_lib.IcpRefineParams) == 3 * 8 + 2 * 4
    result = re.search(r"typedef struct \{([^}]*)\} icp_refine_result;", text).group(1)
    names = [n.strip().split("[")[0] for decl in re.findall(r"(?:double|int64_t|int32_t) ([^;]*);", result) for n in decl.split(",")]
    assert names == [f for f, _ in _lib.IcpRefineResult._fields_] == \
        ["transformation", "fitness", "inlier_rmse", "correspondences", "source_rows", "target_rows", "source_rows_left_out",
         "target_rows_left_out", "iterations", "converged"]
    assert ctypes.sizeof(_lib.IcpRefineResult) == 16 * 8 + 2 * 8 + 5 * 8 + 2 * 4
    assert re.search(r"#define ICP_REFINE_DROP_ZERO_ROWS 1\b", text) and _lib.REFINE_DROP_ZERO_ROWS == 1 and _lib.REFINE_FIGURES == 17
    section = doc[doc.index("---- cloud-to-cloud refinement"):doc.index("typedef struct icp_refine icp_refine;")]
    for word in (CITATION, ":237-243", "deviations", "incrementally", "ties", "strict", "bit-equal"):
        assert word in section, word
    # the defaults are the reference's call
    p = _lib.IcpRefineParams()
    lib.icp_default_refine_params.argtypes = [ctypes.POINTER(_lib.IcpRefineParams)]
    lib.icp_default_refine_params.restype = None
    lib.icp_default_refine_params(ctypes.byref(p))
    assert (p.max_distance, p.max_iteration, p.relative_fitness, p.relative_rmse, p.flags) == (1.0, 30, 1e-6, 1e-6, 0)
    # the Python surface
    assert callable(engine.IcpContext.cloud_refiner)
    for method in ("set_target", "launch", "end", "refine", "history", "close"):
        assert callable(getattr(engine.CloudRefiner, method)), method
    sig = inspect.signature(engine.CloudRefiner.launch)
    assert [(k, v.default) for k, v in sig.parameters.items()][2:] == [("init", None), ("max_distance", 1.0), ("max_iteration", 30),
                                                                       ("relative_fitness", 1e-6), ("relative_rmse", 1e-6),
                                                                       ("drop_zero_rows", False)]
    assert inspect.signature(engine.IcpContext.cloud_refiner).parameters["cell_size"].default == 1.0
    assert isinstance(engine.RefineResult.correspondences, property)
    assert callable(register.install_loop_closure_refinement) and callable(register.compute_transform)


def test_kernel_unit_is_built_and_keeps_to_vector_stores_and_plain_cpp():
    make = open(os.path.join(CSRC, "Makefile")).read()
    srcs = re.search(r"^SRCS\s*:=\s*(.*)$", make, flags=re.M).group(1).split()
    assert "refine.hip" in srcs
    rule = re.search(r"^\$\(OBJDIR\)/%\.o:(.*)$", make, flags=re.M).group(1).split()
    assert "refine_plan.h" in rule and "refine_device.h" in rule
    unit = open(os.path.join(CSRC, "refine.hip")).read()
    assert '#include "refine_plan.h"' in unit and '#include "refine_device.h"' in unit
    for name in ("refine_plan.h", "refine_device.h"):
        plan = open(os.path.join(CSRC, name)).read()
        assert "hip/" not in plan and "__global__" not in plan  # free of HIP: they build with the host compiler alone
    assert "asm" not in unit and "__builtin_amdgcn" not in unit
    assert not re.search(r"while\s*\(|for\s*\(\s*;\s*;\s*\)", unit)  # no loop without its bound in its head: nothing polls or spins
    code = re.sub(r"//[^\n]*", "", unit)
    assert "atomicAdd(" in code and not re.search(r"atomicAdd\(\s*&?\w+(->|\.)?\w*\s*,\s*[^)]*(double|float|\d\.\d)", code)  # integer atomics only
    assert "build_grid" not in code and "RegState" not in code  # its grid is its own


def test_the_drop_in_runs_on_any_refiner_and_returns_the_inverse():
    from pylidar_slam_amd import register
    seen = {}

    class Result:
        transformation = A.rigid(0.3, (1.0, -2.0, 0.5))

    class Fake:
        def __init__(self, owner):
            seen["owner"] = owner

        def refine(self, candidate_pc, target_pc, initial_transform, max_distance):
            seen.update(candidate=candidate_pc, target=target_pc, init=initial_transform, bound=max_distance)
            return Result()

    class Config:
        icp_distance_threshold = 0.75

    class Owner:
        config = Config()

    owner, cand, tgt = Owner(), np.zeros((5, 3)), np.ones((7, 3), np.float32)
    inv, a, b = register.compute_transform(owner, np.eye(4, dtype=np.float32), cand, tgt, factory=Fake)
    assert a is cand and b is tgt and seen["owner"] is owner and seen["bound"] == 0.75
    assert seen["candidate"].dtype == np.float32 and seen["init"].dtype == np.float64
    assert np.array_equal(inv, np.linalg.inv(Result.transformation))
    held = owner._mi355x_refiner
    register.compute_transform(owner, np.eye(4), cand, tgt, factory=Fake)
    assert owner._mi355x_refiner is held  # one refiner per instance
    # where the reference does not define the class (it needs cv2), nothing is patched
    try:
        import slam.loop_closure as ref
        has = hasattr(ref, "ElevationImageLoopClosure")
    except ImportError:
        has = False
    patched = register.install_loop_closure_refinement(Fake)
    assert (patched is not None) == has


# ---- the plan header under the host sanitizers ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plan_program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    exe = tmp_path_factory.mktemp("refine_plan") / "refine_plan_check"
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(cxx).startswith("g++") else []
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-ffp-contract=off", *static, "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "native", "refine_plan_check.cpp"), "-o", str(exe)], check=True)
    return str(exe)


def _run(program, tmp_path, lines):
    cases = tmp_path / "cases.txt"
    cases.write_text("\n".join(lines) + "\n")
    r = subprocess.run([program, str(cases)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-2000:]
    out = r.stdout.splitlines()
    assert len(out) == len(lines)
    return out


def _bits(v):
    return "%016x" % struct.unpack("<Q", struct.pack("<d", v))[0]


def _bits32(v):
    return "%08x" % struct.unpack("<I", struct.pack("<f", v))[0]


def _check(lines_out, wants, prefix, cases):
    kinds = set()
    for line, want, case in zip(lines_out, wants, cases):
        w = line.split()
        kinds.add(w[0])
        if want is None:
            assert w == ["ok"], (line, case)
        else:
            assert w[0] == "refused" and int(w[1]) == -1 and want in line and line.split(None, 2)[2].startswith(prefix), (line, case, want)
    assert kinds == {"ok", "refused"}


def _rows_model(n, cap, mem, flags, xyz=1):
    if n < 0:
        return "negative"
    if n > cap:
        return "exceeds the capacity"
    if mem not in (0, 1):
        return "host or device memory"
    if flags & ~1:
        return "unknown flag"
    if n > 0 and not xyz:
        return "xyz is NULL"
    return None


def _launch_model(n, cap, mem, kind, which, value, have_p, dist, iters, rf, rr, flags, have_t, flying, xyz=1):
    if not have_p:
        return "params is NULL"
    rows = _rows_model(n, cap, mem, flags, xyz)
    if rows:
        return rows
    with np.errstate(over="ignore"):
        if not dist > 0 or not np.isfinite(dist) or not np.isfinite(np.float64(dist) * np.float64(dist)):
            return "max_distance"
    if not 0 <= iters <= 1000:
        return "max_iteration"
    if not rf >= 0 or not rr >= 0:
        return "threshold"
    if kind == 0 or (kind == 2 and 0 <= which < 16 and not np.isfinite(value)):
        return "non-finite"
    if not have_t:
        return "no target"
    if flying:
        return "in flight"
    return None


def test_every_refusal_under_sanitizers(plan_program, tmp_path):
    inf, nan = float("inf"), float("nan")
    create = [(1, 1, 1.0, 1), (MAX_INDEX, MAX_INDEX, 5e-324, 1), (262144, 1440000, 0.4, 1)]
    create += [(1000, 1000, c, 1) for c in (0.0, -0.0, -1.0, inf, -inf, nan)]
    create += [(0, 5, 1.0, 1), (5, 0, 1.0, 1), (-1, -1, 1.0, 1), (MAX_INDEX + 1, 5, 1.0, 1), (5, MAX_INDEX + 1, 1.0, 1), (2 ** 62, 2 ** 62, 1.0, 1),
               (0, 0, nan, 1), (1000, 1000, 1.0, 0), (0, 0, nan, 0)]

    def create_model(t, s, c, out):
        if not out:
            return "out is NULL"
        if not c > 0 or not np.isfinite(c):
            return "cell size"
        if t < 1 or s < 1:
            return "below 1"
        if t > MAX_INDEX or s > MAX_INDEX:
            return "capacity exceeds"
        return None
    out = _run(plan_program, tmp_path, [f"C {t} {s} {_bits(c)} {o}" for t, s, c, o in create])
    _check(out, [create_model(*c) for c in create], "icp_refine_create: ", create)

    target = [(0, 64, 0, 0, 0), (64, 64, 1, 1, 0), (65, 64, 0, 0, 0), (-1, 64, 0, 0, 0), (-2 ** 40, 64, 1, 1, 0), (MAX_INDEX, MAX_INDEX, 1, 0, 0),
              (5, 64, 2, 0, 0), (5, 64, -1, 1, 0), (5, 64, 0, 2, 0), (5, 64, 0, 3, 0), (5, 64, 1, -1, 0), (5, 64, 0, 0, 1), (65, 64, 7, 7, 1)]
    target = [t + (1,) for t in target] + [(0, 64, 0, 0, 0, 0), (5, 64, 0, 0, 0, 0), (5, 64, 1, 1, 1, 0), (65, 64, 0, 0, 0, 0)]
    out = _run(plan_program, tmp_path, [f"S {n} {cap} {mem} {fl} {fly} {x}" for n, cap, mem, fl, fly, x in target])
    _check(out, [_rows_model(n, cap, mem, fl, x) or ("in flight" if fly else None) for n, cap, mem, fl, fly, x in target], "icp_refine_set_target: ", target)

    ok = dict(n=100, cap=100, mem=0, kind=1, which=0, value=0.0, have_p=1, dist=1.0, iters=30, rf=1e-6, rr=1e-6, flags=0, have_t=1, flying=0, xyz=1)
    launch = [dict(ok), dict(ok, n=0), dict(ok, iters=0), dict(ok, iters=1000), dict(ok, rf=0.0, rr=0.0), dict(ok, flags=1, mem=1), dict(ok, dist=5e-324 ** 0.5 * 4),
              dict(ok, dist=1e154)]
    launch += [dict(ok, n=-1), dict(ok, n=101), dict(ok, n=2 ** 40), dict(ok, mem=2), dict(ok, mem=-1), dict(ok, flags=2), dict(ok, flags=-1), dict(ok, have_p=0),
               dict(ok, have_p=0, n=-1), dict(ok, kind=0), dict(ok, have_t=0), dict(ok, flying=1), dict(ok, have_t=0, flying=1)]
    launch += [dict(ok, xyz=0), dict(ok, xyz=0, n=0), dict(ok, xyz=0, dist=0.0)]
    launch += [dict(ok, dist=d) for d in (0.0, -0.0, -1.0, inf, -inf, nan, 1e155, 1e308)]
    launch += [dict(ok, iters=i) for i in (-1, 1001, 2 ** 31 - 1, -2 ** 31)]
    launch += [dict(ok, rf=v) for v in (-1e-300, -1.0, nan, -inf)] + [dict(ok, rr=v) for v in (-5e-324, nan)] + [dict(ok, rf=inf, rr=inf)]
    launch += [dict(ok, kind=2, which=k, value=v) for k in range(16) for v in (nan, inf, -inf, 1e308, -0.0)]
    lines = [f"L {c['n']} {c['cap']} {c['mem']} {c['kind']} {c['which']} {_bits(c['value'])} {c['have_p']} {_bits(c['dist'])} {c['iters']} "
             f"{_bits(c['rf'])} {_bits(c['rr'])} {c['flags']} {c['have_t']} {c['flying']} {c['xyz']}" for c in launch]
    out = _run(plan_program, tmp_path, lines)
    _check(out, [_launch_model(**c) for c in launch], "icp_refine_launch: ", launch)

    out = _run(plan_program, tmp_path, ["E 1 0", "E 1 1", "E 0 0", "E 0 7", "E 1 2", "E 1 -1"])
    assert out[0] == out[1] == "ok" and all("nothing has been launched" in o for o in out[2:4]) and all("host or device memory" in o for o in out[4:])
    assert all(o.startswith("refused -1 icp_refine_end: ") for o in out[2:])
    out = _run(plan_program, tmp_path, ["I 1 1 1 1", "I 0 1 1 1", "I 1 0 1 1", "I 1 1 0 1", "I 1 1 1 0", "I 0 0 0 0"])
    assert out[0] == "ok" and "image is NULL" in out[1] and "another context" in out[2] and "output is NULL" in out[3] and "output is NULL" in out[4]
    assert all(o.startswith("refused -1 icp_refine_image_rows: ") for o in out[1:])
    out = _run(plan_program, tmp_path, ["Y 1 0 1", "Y 1 30 31", "Y 1 30 1001", "Y 0 0 100", "Y 1 30 30", "Y 1 0 0", "Y 1 5 -1"])
    assert out[:3] == ["ok"] * 3 and "no refinement has been collected" in out[3] and all("is below" in o for o in out[4:])
    assert all(o.startswith("refused -1 icp_refine_history: ") for o in out[3:])


def test_table_sizes_grids_rings_and_footprint_under_sanitizers(plan_program, tmp_path):
    sizes = [1, 2, 3, 31, 32, 33, 2 ** 10, 2 ** 10 + 1, 2 ** 17, 2 ** 17 + 1, 2 ** 20 - 1, 1440000, 2 ** 30, 2 ** 30 + 1, MAX_INDEX]
    cases = [(t, 1000, 0, 0, t) for t in sizes] + [(1000, s, 1, 1, s) for s in (1, 255, 256, 257, 2048 * 256, 2048 * 256 + 1, MAX_INDEX)]
    cases += [(0, 5, 0, 0, 0), (5, 0, 0, 0, -3), (MAX_INDEX + 1, 5, 1, 1, 1)]
    out = _run(plan_program, tmp_path, [f"T {t} {s} {ht} {hs} {n}" for t, s, ht, hs, n in cases])
    for line, (t, s, ht, hs, n) in zip(out, cases):
        slots, foot, blocks, iterate = (int(v) for v in line.split())
        assert slots & (slots - 1) == 0 and slots >= 64 and slots >= 2 * t and (slots == 64 or slots < 4 * t), (t, slots)
        valid = 1 <= t <= MAX_INDEX and 1 <= s <= MAX_INDEX
        want = t * 24 + slots * 16 + s * 4 + 2048 * 160 + 1001 * 33 * 8 + 512 + (t * 12 if ht else 0) + (s * 12 if hs else 0)
        assert foot == (want if valid else 0), (t, s)
        assert blocks == (0 if n < 1 else -(-n // 256)) and iterate == min(max(blocks, 1), 2048), n
    # rings: ceil(bound / cell) + 1 — the widening for the rounded cell coordinate —, 0 (exhaustive) above 7 cells
    one_up = float(np.nextafter(1.0, 2.0))
    ratios = [(0.25, 1.0, 2), (1.0, 1.0, 2), (one_up, 1.0, 3), (3.7, 1.0, 5), (0.1, 0.4, 2), (1.0, 0.4, 4), (1.0, 0.1, 0), (7.0, 1.0, 8),
              (float(np.nextafter(7.0, 8.0)), 1.0, 0), (1e300, 1.0, 0), (1.0, 5e-324, 0), (5e-324, 1.0, 2), (0.7, 0.1, 8), (3.0, 1.0, 4)]
    out = _run(plan_program, tmp_path, [f"R {_bits(d)} {_bits(c)}" for d, c, _ in ratios])
    assert [int(o) for o in out] == [w for _, _, w in ratios]


def test_zero_row_filter_and_cell_boxes_under_sanitizers(plan_program, tmp_path):
    rows = np.array([[0, 0, 0], [-0.0, 0, 0], [1e-30, 1e-30, 1e-30], [1e-20, 0, 0], [1e-23, 1e-23, 0], [1, 0, 0], [0, 0, -1e-10], [np.nan, 0, 0],
                     [np.inf, 0, 0], [0, -np.inf, 1], [1e30, 1e30, 0], [1e-45, 0, 0], [2e-23, 3e-23, 0]], np.float32)
    out = _run(plan_program, tmp_path, [f"Z {_bits32(x)} {_bits32(y)} {_bits32(z)}" for x, y, z in rows])
    assert [int(o) for o in out] == [int(v) for v in A.zero_rows(rows)]
    assert [int(o) for o in out][:6] == [1, 1, 1, 0, 1, 0]
    # the box of a cell bounds every coordinate whose computed cell it is: the gap is 0 for them, and never above the true distance
    rng = np.random.default_rng(5)
    lines, checks = [], []
    for cell in (1.0, 0.4, 0.1, 3.7):
        inv = 1.0 / cell
        q = np.concatenate([rng.uniform(-50, 50, 200), np.arange(-20, 21) * cell, np.nextafter(np.arange(-20, 21) * cell, np.inf),
                            np.nextafter(np.arange(-20, 21) * cell, -np.inf), [1e5 * cell, -1e5 * cell, (2 ** 20 - 1) * cell]])
        k = np.floor(q * inv).astype(np.int64)
        v = q + rng.uniform(-3, 3, len(q)) * cell
        for qq, kk, vv in zip(q, k, v):
            lines += [f"G {_bits(qq)} {kk} {_bits(cell)}", f"G {_bits(vv)} {kk} {_bits(cell)}"]
            checks.append((qq, vv))
    out = _run(plan_program, tmp_path, lines)
    gaps = [struct.unpack("<d", struct.pack("<Q", int(o, 16)))[0] for o in out]
    for (qq, vv), own, other in zip(checks, gaps[0::2], gaps[1::2]):
        assert own == 0.0 and 0.0 <= other <= abs(vv - qq), (qq, vv, own, other)
    assert sum(g > 0 for g in gaps[1::2]) > 300


def test_the_step_of_the_solve_kernel_against_the_model_under_sanitizers(plan_program, tmp_path):
    """refine_step on the figures of the model's own runs, on random and on degenerate H: within 4 x the recorded worst of the
    model's two routes, in condition units, where the rotation is unique; a proper rotation with t = mu_q - R mu_p everywhere"""
    rng = np.random.default_rng(11)
    figs = [e.fig for name in ("cube", "lattice", "trap") for e in A.free_run(name)["evaluations"]]
    for _ in range(40):
        H = rng.normal(0, 1, (3, 3)) * 10.0 ** rng.integers(-3, 4)
        figs.append(np.concatenate([[100.0, 3.0], rng.normal(0, 100, 6), H.reshape(-1)]))
    figs.append(np.concatenate([[10.0, 1.0], np.zeros(6), np.diag([3.0, 2.0, -1.0]).reshape(-1)]))  # a reflection to be fixed
    degenerate = [np.zeros((3, 3)), np.outer([1.0, 2.0, 3.0], [0.5, -1.0, 2.0]), np.diag([1.0, 1.0, -1.0]), np.diag([2.0, 0.0, 0.0]), np.diag([1.0, 1.0, 0.0]) * 1e-140]
    figs += [np.concatenate([[2.0, 1.0], rng.normal(0, 10, 6), H.reshape(-1)]) for H in degenerate]
    figs.append(np.concatenate([[0.0, 0.0], rng.normal(0, 10, 6), rng.normal(0, 1, 9)]))  # no correspondence: the identity
    out = _run(plan_program, tmp_path, ["P " + " ".join(_bits(v) for v in f) for f in figs])
    worst, unique = 0.0, 0
    for line, fig in zip(out, figs):
        up = np.array([struct.unpack("<d", struct.pack("<Q", int(w, 16)))[0] for w in line.split()]).reshape(4, 4)
        assert np.array_equal(up[3], [0, 0, 0, 1])
        if fig[0] == 0:
            assert np.array_equal(up, np.eye(4))
            continue
        R, t = up[:3, :3], up[:3, 3]
        assert np.abs(R.T @ R - np.eye(3)).max() <= 16 * A.U and np.linalg.det(R) > 0
        assert np.abs(t - (fig[5:8] - R @ fig[2:5])).max() <= 8 * A.U * (np.abs(fig[5:8]).max() + np.abs(R) @ np.abs(fig[2:5])).max()
        unit = A.condition_unit(fig[8:].reshape(3, 3))
        if np.isfinite(unit) and unit < 1e-6:
            unique += 1
            err = np.abs(R - A.step(fig)[:3, :3]).max() / unit
            worst = max(worst, err)
            assert err <= 4 * A.STEP_UNITS, (err, fig)
    print("worst step error in condition units:", worst)
    assert unique > 40
