"""CPU side of the aggregated world map (icp_aggmap_*, include/icp_mi355x.h):

* every call is declared with the signature written down here, cites the reference lines it stands for, is exported, bound,
  and reachable as `IcpContext.aggregated_map` / `AggregatedMap` and through the plugin's `aggregate_map_voxel`;
* the kernel unit is part of the build;
* what needs no device (csrc/aggmap_plan.h: every refusal, the slot count and its overflow edge, the footprint, the key
  packing at the coordinate limits, the slot function) as a stand-alone program under -fsanitize=address,undefined, against
  the rules written down here and the model's own packing and slot function (tests/aggmap_audit.py)."""
import ctypes
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import aggmap_audit as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "icp_mi355x.h")
CSRC = os.path.join(ROOT, "pylidar-slam_amd", "csrc")
MAX_ROWS = 1 << 30

SIGNATURES = {
    "icp_aggmap_create": ("int", ["icp_ctx* ctx", "double voxel_size", "int64_t capacity", "int64_t max_insert_rows", "icp_aggmap** out"]),
    "icp_aggmap_destroy": ("void", ["icp_aggmap* map"]),
    "icp_aggmap_insert": ("int", ["icp_aggmap* map", "const float* xyz", "int64_t n", "int mem", "const double pose[16]", "int32_t frame_id"]),
    "icp_aggmap_stats": ("int", ["icp_aggmap* map", "icp_aggmap_counters* out"]),
    "icp_aggmap_get": ("int", ["icp_aggmap* map", "const double origin[3]", "float* xyz_out", "uint32_t* hits_out",
                               "int32_t* first_frame_out", "int32_t* last_frame_out", "int64_t cap", "int out_mem", "int64_t* size_out"]),
    "icp_aggmap_get_f64": ("int", ["icp_aggmap* map", "double* xyz_out", "int64_t cap", "int out_mem", "int64_t* size_out"]),
    "icp_aggmap_submap": ("int", ["icp_aggmap* map", "int32_t frame_lo", "int32_t frame_hi", "const double pose[16]", "float* xyz_out",
                                  "int32_t* index_out", "int64_t cap", "int out_mem", "int64_t* count_out"]),
    "icp_aggmap_clear": ("int", ["icp_aggmap* map"]),
}


def test_every_call_is_declared_cited_exported_and_bound():
    from pylidar_slam_amd import _lib, engine, odometry
    doc = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", doc, flags=re.S)
    lib = ctypes.CDLL(_lib.library_path())
    for name, (ret, want) in SIGNATURES.items():
        m = re.search(r"(\w+)\s+%s\s*\(([^;]*)\)\s*;" % name, text)
        assert m, f"{name} is not declared"
        args = [re.sub(r"\s+", " ", a).strip() for a in m.group(2).split(",")]
        assert m.group(1) == ret and args == want, (name, m.group(1), args)
        # the comment right in front of the declaration cites both reference locations
        at = doc.index(m.group(0).split("(")[0].strip() + "(")
        comment = doc[doc.rindex("/*", 0, at):at]
        assert "slam/loop_closure.py:272-291" in comment and "slam/common/pose.py:40-49" in comment, name
        assert hasattr(lib, name), f"{name} is not exported"
        restype, argtypes = _lib.EXPORTED_SYMBOLS[name]
        assert len(argtypes) == len(want) and restype is (None if ret == "void" else ctypes.c_int), name
    assert ctypes.sizeof(_lib.IcpAggmapCounters) == 6 * 8
    fields = re.search(r"typedef struct \{([^}]*)\} icp_aggmap_counters;", text).group(1)
    assert re.findall(r"int64_t (\w+);", fields) == [f for f, _ in _lib.IcpAggmapCounters._fields_] == \
        ["size", "inserts", "dropped", "out_of_range", "nonfinite", "error"]
    assert callable(engine.IcpContext.aggregated_map)
    for method in ("insert", "stats", "points", "submap", "clear", "save_ply"):
        assert callable(getattr(engine.AggregatedMap, method)), method
    for prop in ("hits", "first_frame", "last_frame"):
        assert isinstance(getattr(engine.AggregatedMap, prop), property), prop
    cfg = odometry.MI355XICPConfig()
    assert cfg.aggregate_map_voxel == 0.0 and isinstance(cfg.aggregate_map_capacity, int) and cfg.aggregate_map_capacity >= 1


def test_kernel_unit_is_built_and_shares_the_grid_samples_rounding():
    make = open(os.path.join(CSRC, "Makefile")).read()
    srcs = re.search(r"^SRCS\s*:=\s*(.*)$", make, flags=re.M).group(1).split()
    assert "aggmap.hip" in srcs and "grid_sample.hip" in srcs
    rule = re.search(r"^\$\(OBJDIR\)/%\.o:(.*)$", make, flags=re.M).group(1).split()
    assert "aggmap_plan.h" in rule and "voxel_device.h" in rule
    unit = open(os.path.join(CSRC, "aggmap.hip")).read()
    sample = open(os.path.join(CSRC, "grid_sample.hip")).read()
    shared = open(os.path.join(CSRC, "voxel_device.h")).read()
    assert '#include "voxel_device.h"' in unit and '#include "voxel_device.h"' in sample and '#include "aggmap_plan.h"' in unit
    assert len(re.findall(r"long long voxel_coord\(", shared)) == 1
    assert not re.search(r"long long voxel_coord\(T", unit) and not re.search(r"long long voxel_coord\(T", sample)
    plan = open(os.path.join(CSRC, "aggmap_plan.h")).read()
    assert "hip/" not in plan and "__global__" not in plan  # free of HIP: it builds with the host compiler alone
    # no unbounded spin: every loop of the unit has its bound in its head
    assert not re.search(r"while\s*\(\s*(true|1)\s*\)|for\s*\(\s*;\s*;\s*\)", unit)


# ---- the plan header under the host sanitizers ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plan_program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    exe = tmp_path_factory.mktemp("aggmap_plan") / "aggmap_plan_check"
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(cxx).startswith("g++") else []
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", *static, "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "native", "aggmap_plan_check.cpp"), "-o", str(exe)], check=True)
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


def _create_model(v, c, r):
    if not (v > 0) or not np.isfinite(v):
        return "voxel size"
    if c < 1:
        return "capacity"
    if r < 1:
        return "max_insert_rows"
    if c > MAX_ROWS or r > MAX_ROWS or c + r > MAX_ROWS:
        return "exceeds"
    return None


def _pose_ok(kind, which, value):
    return kind == 1 or (kind == 2 and (not 0 <= which < 16 or np.isfinite(value)))


def _insert_model(n, rows, mem, kind, which, value):
    if n < 0:
        return "negative"
    if n > rows:
        return "exceeds max_insert_rows"
    if not _pose_ok(kind, which, value):
        return "non-finite"
    if mem not in (0, 1):
        return "host or device memory"
    return None


def _submap_model(lo, hi, mem, kind, which, value):
    if lo > hi:
        return "frame_lo"
    if not _pose_ok(kind, which, value):
        return "non-finite"
    if mem not in (0, 1):
        return "host or device memory"
    return None


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


def test_every_refusal_under_sanitizers(plan_program, tmp_path):
    inf, nan = float("inf"), float("nan")
    create = [(0.2, 100, 64), (0.0, 100, 64), (-0.0, 100, 64), (-1.0, 100, 64), (inf, 100, 64), (-inf, 100, 64), (nan, 100, 64),
              (5e-324, 1, 1), (0.2, 0, 64), (0.2, -5, 64), (0.2, 100, 0), (0.2, 100, -1), (0.2, MAX_ROWS - 64, 64),
              (0.2, MAX_ROWS - 63, 64), (0.2, MAX_ROWS, 1), (0.2, 1, MAX_ROWS), (0.2, MAX_ROWS + 1, 1), (0.2, 2 ** 62, 2 ** 62),
              (0.2, 2 ** 63 - 1, 2 ** 63 - 1), (nan, 0, 0), (0.2, 0, 0)]
    out = _run(plan_program, tmp_path, [f"C {_bits(v)} {c} {r}" for v, c, r in create])
    _check(out, [_create_model(*c) for c in create], "icp_aggmap_create: ", create)
    insert = [(0, 64, 0, 1, 0, 0.0), (64, 64, 1, 1, 0, 0.0), (65, 64, 0, 1, 0, 0.0), (-1, 64, 0, 1, 0, 0.0), (-2 ** 40, 64, 0, 1, 0, 0.0),
              (2 ** 40, 64, 0, 1, 0, 0.0), (5, 64, 2, 1, 0, 0.0), (5, 64, -1, 1, 0, 0.0), (5, 64, 0, 0, 0, 0.0), (-1, 64, 7, 0, 0, 0.0),
              (65, 64, 7, 0, 0, 0.0)]
    insert += [(5, 64, 0, 2, k, v) for k in range(16) for v in (nan, inf, -inf, 1.0e308, -0.0)]
    out = _run(plan_program, tmp_path, [f"I {n} {r} {mem} {k} {w} {_bits(v)}" for n, r, mem, k, w, v in insert])
    _check(out, [_insert_model(*c) for c in insert], "icp_aggmap_insert: ", insert)
    submap = [(0, 0, 0, 1, 0, 0.0), (-5, 7, 1, 1, 0, 0.0), (3, 2, 0, 1, 0, 0.0), (2 ** 31 - 1, -2 ** 31, 0, 1, 0, 0.0),
              (-2 ** 31, 2 ** 31 - 1, 0, 1, 0, 0.0), (0, 1, 2, 1, 0, 0.0), (0, 1, 0, 0, 0, 0.0), (3, 2, 9, 0, 0, 0.0)]
    submap += [(0, 1, 1, 2, k, v) for k in (0, 3, 11, 15) for v in (nan, inf, 2.5)]
    out = _run(plan_program, tmp_path, [f"S {lo} {hi} {mem} {k} {w} {_bits(v)}" for lo, hi, mem, k, w, v in submap])
    _check(out, [_submap_model(*c) for c in submap], "icp_aggmap_submap: ", submap)
    out = _run(plan_program, tmp_path, ["G 0", "G 1", "G 2", "G -1"])
    assert out[0] == out[1] == "ok" and all(o.startswith("refused -1 icp_aggmap_get: host or device memory") for o in out[2:])


def test_slot_counts_footprint_and_the_overflow_edge_under_sanitizers(plan_program, tmp_path):
    # the sum C + R alone (1 is below what a map can have — both are at least 1 — and still has its slot count)
    totals = [1, 2] + [v for k in (2, 3, 5, 10, 17, 29, 30) for v in (2 ** k - 1, 2 ** k, 2 ** k + 1)] + [0, 2 ** 40, 2 ** 64 - 1]
    for line, total in zip(_run(plan_program, tmp_path, [f"P {t}" for t in totals]), totals):
        want = 0
        if 1 <= total <= MAX_ROWS:
            want = 2
            while want < 2 * total:
                want *= 2
        assert int(line) == want, total
        assert want == 0 or (want >= 2 * total and (want == 2 or want // 2 < 2 * total))
    cases = [(1, 1)]
    for k in (2, 3, 5, 10, 17, 29):
        for total in (2 ** k - 1, 2 ** k, 2 ** k + 1):
            for rows in (1, total // 3 + 1, total - 1):
                cases.append((total - rows, rows))
    cases += [(MAX_ROWS - 1, 1), (MAX_ROWS - 262144, 262144)]
    bad = [(MAX_ROWS, 1), (1, MAX_ROWS), (2 ** 62, 2 ** 62), (2 ** 63 - 1, 2 ** 63 - 1), (0, 5), (5, 0), (-1, -1)]
    out = _run(plan_program, tmp_path, [f"T {c} {r}" for c, r in cases + bad])
    for line, (c, r) in zip(out, cases):
        slots, bytes_, per_block = (int(v) for v in line.split())
        assert slots == A.slot_count(c, r) and slots >= 2 * (c + r) and slots & (slots - 1) == 0 and (slots == 2 or slots // 2 < 2 * (c + r)), (c, r, slots)
        assert bytes_ == slots * 24 + c * 32 + r * 16 + 1025 * 4 + 64, (c, r)
        assert per_block % 256 == 0 and per_block >= 256 and -(-r // per_block) <= 1024 and (per_block == 256 or -(-r // (per_block - 256)) > 1024), (r, per_block)
    assert int(out[len(cases) - 2].split()[0]) == 2 ** 31  # the largest table
    for line, case in zip(out[len(cases):], bad):
        assert line.split()[:2] == ["0", "0"], case


def test_packing_round_trip_and_slots_against_the_model_under_sanitizers(plan_program, tmp_path):
    lim = (-(1 << 20), (1 << 20) - 1)
    coords = [(x, y, z) for x in lim for y in lim for z in lim] + [(0, 0, 0), (-1, -1, -1), (1, 2, 3), (-1000, 999, 5)]
    rng = np.random.default_rng(5)
    coords += [tuple(int(v) for v in row) for row in rng.integers(lim[0], lim[1] + 1, (200, 3))]
    masks = [1, 255, (1 << 20) - 1, (1 << 31) - 1]
    lines = [f"K {x} {y} {z} {masks[i % 4]:x}" for i, (x, y, z) in enumerate(coords)]
    out = _run(plan_program, tmp_path, lines)
    keys = A.pack_keys(np.array(coords, np.int64))
    assert len(set(int(k) for k in keys)) == len(set(coords)) and np.array_equal(A.unpack_keys(keys), np.array(coords, np.int64))
    for i, (line, c) in enumerate(zip(out, coords)):
        w = line.split()
        assert int(w[0], 16) == int(keys[i]) and int(w[0], 16) < 2 ** 63, c
        assert tuple(int(v) for v in w[1:4]) == c, c
        assert int(w[4]) == int(A.slot_of_keys(keys[i:i + 1], masks[i % 4] + 1)[0]), c
    e = float(1 << 20)
    reals = [(-e, 1), (e - 1, 1), (e, 0), (-e - 1, 0), (0.0, 1), (-0.0, 1), (np.nextafter(-e, -np.inf), 0), (np.nextafter(e, 0), 1),
             (float("inf"), 0), (float("-inf"), 0), (float("nan"), 0), (1.0e300, 0)]
    out = _run(plan_program, tmp_path, [f"R {_bits(v)}" for v, _ in reals])
    assert [int(o) for o in out] == [w for _, w in reals]


# ---- the plugin's option, on the numpy stand-in of the context -------------------------------------------------------------
def test_plugin_option_inserts_every_odometry_pc_with_its_absolute_pose(monkeypatch):
    """per-call path, host logic only (tests/oracle_context.py stands in for the HIP context): at 0 no map is asked for; above 0
    every frame behind frame 0 is inserted — the rows of its `odometry_pc`, `absolute_poses[frame]`, the frame index — and
    `init()` clears the map; a context without the aggregated map is refused"""
    import torch
    import pylidar_slam_amd.odometry as odo_mod
    from oracle_context import OracleContext
    from pylidar_slam_amd.synthetic import SceneConfig, make_sequence
    created, calls = [], []

    class Recorder(A.AggMapModel):
        def insert(self, points, pose, frame_id):
            points = points.numpy() if isinstance(points, torch.Tensor) else points
            calls.append((np.array(points, np.float32), np.array(pose, np.float64), int(frame_id)))
            super().insert(points, pose, frame_id)

    class WithMap(OracleContext):
        def aggregated_map(self, voxel_size, capacity, max_insert_rows=262144):
            created.append(Recorder(voxel_size, capacity, max_insert_rows))
            return created[-1]

    scans, _ = make_sequence(SceneConfig(height=16, width=128), 4)
    proj = odo_mod.SphericalProjector(16, 128)
    kw = dict(max_num_alignments=3, threshold_delta_pose=0.0, data_key="numpy_pc", device="cpu")
    monkeypatch.setattr(odo_mod, "IcpContext", OracleContext)
    with pytest.raises(AssertionError, match="aggregated map"):
        odo_mod.MI355XICPFrameToModel(odo_mod.MI355XICPConfig(aggregate_map_voxel=0.25, **kw), projector=proj, device=torch.device("cpu"))
    with pytest.raises(AssertionError, match="negative"):
        odo_mod.MI355XICPFrameToModel(odo_mod.MI355XICPConfig(aggregate_map_voxel=-1.0, **kw), projector=proj, device=torch.device("cpu"))
    monkeypatch.setattr(odo_mod, "IcpContext", WithMap)
    runs = {}
    for voxel in (0.0, 0.25):
        odo = odo_mod.MI355XICPFrameToModel(odo_mod.MI355XICPConfig(aggregate_map_voxel=voxel, aggregate_map_capacity=5000, **kw),
                                            projector=proj, device=torch.device("cpu"))
        odo.init()
        dicts = []
        for s in scans:
            dicts.append({"numpy_pc": s})
            odo.process_next_frame(dicts[-1])
        runs[voxel] = (odo, dicts)
    off, on = runs[0.0][0], runs[0.25][0]
    assert off.aggregated_map is None and len(created) == 1 and on.aggregated_map is created[0]
    assert (created[0].voxel, created[0].capacity, created[0].max_rows) == (0.25, 5000, 262144)
    assert np.array_equal(np.stack(off.absolute_poses), np.stack(on.absolute_poses))
    assert [c[2] for c in calls] == [1, 2, 3]
    for rows, pose, frame in calls:
        assert np.array_equal(rows, runs[0.25][1][frame]["odometry_pc"]) and np.array_equal(pose, on.absolute_poses[frame])
    assert "odometry_pc" not in runs[0.25][1][0] and created[0].stats()["inserts"] == 3 and created[0].size > 128
    on.init()
    assert created[0].size == 0 and created[0].stats()["inserts"] == 0
