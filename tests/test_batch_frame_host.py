"""CPU side of the batched frame calls (icp_batch_odometry_init / icp_batch_frame_launch / icp_batch_frame_end,
include/icp_mi355x.h):

* the three calls and `icp_batch_frame` are declared behind the single-frame block, exported and bound with the header's
  layout; the single-frame structs keep theirs;
* the drives of tests/test_gpu_batch_frame.py take their key frames where tests/batch_frame_cases.py says and keep every
  frame's key-frame quantities at least 10 % away from the thresholds, on the plugin driven by the numpy oracle (where the
  yardstick of a GPU comparison decides with numpy — the plugin's flag — a rounding difference cannot flip a decision);
* the member partition and the refusals (csrc/batch_frame_plan.h) as a stand-alone program under
  -fsanitize=address,undefined, against a model of the rules written here;
* the batched plugin's `one_call_frame` flag: what it refuses, on the oracle-backed context."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import batch_frame_cases as BC
import frame_cases as FC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "icp_mi355x.h")
CSRC = os.path.join(ROOT, "pylidar-slam_amd", "csrc")
NAMES = ("icp_batch_odometry_init", "icp_batch_frame_launch", "icp_batch_frame_end")


# ---- header and binding --------------------------------------------------------------------------------------------
def test_batched_frame_calls_are_declared_and_bound():
    from pylidar_slam_amd import _lib
    doc = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", doc, flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} is not declared in include/icp_mi355x.h"
        assert name in _lib.EXPORTED_SYMBOLS, f"{name} is not bound in _lib.EXPORTED_SYMBOLS"
    assert "typedef struct icp_batch_frame {" in text
    # behind the single-frame block, which no longer says that the batched form does not exist
    assert text.index("typedef struct icp_batch_frame {") > text.index("int icp_frame_end(")
    assert "does not exist" not in doc[doc.index("one call per odometry frame"):doc.index("typedef struct icp_frame_config")]
    lib = ctypes.CDLL(_lib.library_path())
    for name in NAMES:
        assert hasattr(lib, name), f"{name} is not exported by the library"
    assert _lib.EXPORTED_SYMBOLS["icp_batch_frame_end"][1][1] == ctypes.POINTER(_lib.IcpFrameResult)
    assert _lib.EXPORTED_SYMBOLS["icp_batch_frame_launch"][1][1] == ctypes.POINTER(_lib.IcpBatchFrame)


def test_batch_frame_layout_matches_the_header(tmp_path):
    """sizeof / offsetof of icp_batch_frame as the C compiler lays the header out, against the ctypes structure; the
    single-frame structs keep their layout."""
    from pylidar_slam_amd import _lib
    cc = shutil.which("gcc") or shutil.which("cc") or shutil.which("clang")
    assert cc, "no C compiler"
    structs = {"icp_batch_frame": _lib.IcpBatchFrame, "icp_frame_config": _lib.IcpFrameConfig,
               "icp_frame_result": _lib.IcpFrameResult}
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "icp_mi355x.h"', 'int main(void) {']
    for s, cls in structs.items():
        src.append(f'  printf("{s} %zu\\n", sizeof({s}));')
        for n, _ in cls._fields_:
            src.append(f'  printf("{s}.{n} %zu\\n", offsetof({s}, {n}));')
    src += ['  return 0;', '}']
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.run([cc, "-std=c99", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    out = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for s, cls in structs.items():
        assert ctypes.sizeof(cls) == int(out[s]), s
        for n, _ in cls._fields_:
            assert getattr(cls, n).offset == int(out[f"{s}.{n}"]), (s, n)
    assert ctypes.sizeof(_lib.IcpBatchFrame) == 5 * 8  # three pointers, an int64, an int32 and its padding
    assert ctypes.sizeof(_lib.IcpFrameConfig) == 8 + 6 * 4
    assert ctypes.sizeof(_lib.IcpFrameResult) == ctypes.sizeof(_lib.IcpRegisterResult) + 2 * 4 + 2 * 8


def test_engine_batch_has_the_frame_methods():
    from pylidar_slam_amd.engine import IcpBatch
    for name in ("odometry_init", "frame_launch", "frame_end"):
        assert callable(getattr(IcpBatch, name, None)), name


# ---- the fixture condition of the GPU tests -------------------------------------------------------------------------------
def test_batched_drives_keep_clear_of_the_key_frame_thresholds_and_mix_decisions(monkeypatch):
    """Every member of the `sampled` drive on the plugin driven by the numpy oracle: no frame's |t| or |r| 180 / pi comes
    within 10 % of its threshold, the key frames fall where tests/batch_frame_cases.py says — and with THOSE decisions one
    step has every member insert while others mix insertions with pose-only updates."""
    import pylidar_slam_amd.odometry as odo_mod
    from oracle_context import OracleContext
    monkeypatch.setattr(odo_mod, "IcpContext", OracleContext)
    d = BC.drive("sampled")
    keys = []
    for member in range(d.members):
        _, odo = FC.run_plugin_on_oracle(BC.single_drive(d, member))
        rows = FC.key_frame_margins(odo.get_relative_poses())
        assert len(rows) == d.frames - 1
        for f, (_, _, _, trans, rot, _) in enumerate(rows, start=1):
            assert abs(trans - FC.THRESHOLD_TRANS) >= 0.10 * FC.THRESHOLD_TRANS, (member, f, trans)
            assert abs(rot - FC.THRESHOLD_ROT) >= 0.10 * FC.THRESHOLD_ROT, (member, f, rot)
        keys.append({f for f, r in enumerate(rows, start=1) if r[5]})
        assert sorted(keys[-1]) == BC.KEY_FRAMES[member], (member, sorted(keys[-1]))
    mixed = [f for f in range(1, d.frames) if 0 < sum(f in k for k in keys) < len(keys)]
    together = [f for f in range(1, d.frames) if all(f in k for k in keys)]
    assert mixed and together == [6], (mixed, together)


# ---- the member partition and the refusals under the host sanitizers ----------------------------------------------------
@pytest.fixture(scope="module")
def plan_program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    exe = tmp_path_factory.mktemp("plan") / "batch_frame_plan_check"
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(cxx).startswith("g++") else []
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", *static, "-I", CSRC,
                    os.path.join(ROOT, "tests", "native", "batch_frame_plan_check.cpp"), "-o", str(exe)], check=True)
    return str(exe)


FIELDS = ("skip", "has_sequence", "frame_index", "voxel_size", "targets", "point_to_point", "projective_map", "exchange",
          "profiling", "registering", "frame_launched", "stream")


def _member(**kw):
    m = dict(skip=0, has_sequence=1, frame_index=3, voxel_size=0.4, targets=1, point_to_point=0, projective_map=0,
             exchange=0, profiling=0, registering=0, frame_launched=0, stream=7)
    m.update(kw)
    return m


def _model(members, pending):
    """The rules of the issue, written down independently: ("ok", skipped, first, registering) or ("refused", member, word)."""
    if not 1 <= len(members) <= 32:
        return ("refused", -1, "members are required")
    if pending:
        return ("refused", -1, "already launched")
    lead = None
    for b, m in enumerate(members):
        if m["skip"]:
            continue
        for key, word in (("has_sequence", "no sequence"), ("point_to_point", "point-to-point"),
                          ("projective_map", "projective map"), ("exchange", "exchange"), ("profiling", "profiling"),
                          ("registering", "registration of the member's own"), ("frame_launched", "frame of the member's own")):
            if bool(m[key]) != (key == "has_sequence"):
                return ("refused", b, word)
        if lead is None:
            lead = m
            continue
        if (m["voxel_size"] > 0 or lead["voxel_size"] > 0) and m["voxel_size"] != lead["voxel_size"]:
            return ("refused", b, "voxel_size")
        if m["targets"] != lead["targets"]:
            return ("refused", b, "targets")
        if m["stream"] != lead["stream"]:
            return ("refused", b, "one stream")
    if lead is None:
        return ("refused", -1, "every member is skipped")
    idx = range(len(members))
    return ("ok", [b for b in idx if members[b]["skip"]],
            [b for b in idx if not members[b]["skip"] and members[b]["frame_index"] == 0],
            [b for b in idx if not members[b]["skip"] and members[b]["frame_index"] >= 1])


def _run(program, tmp_path, lines):
    cases = tmp_path / "cases.txt"
    cases.write_text("\n".join(lines) + "\n")
    r = subprocess.run([program, str(cases)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-2000:]
    return r.stdout.splitlines()


def _plan_line(members, pending):
    return "P %d %d " % (len(members), int(pending)) + " ".join(" ".join(repr(m[k]) for k in FIELDS) for m in members)


def _check_plan(line, members, pending):
    want = _model(members, pending)
    w = line.split()
    if want[0] == "refused":
        assert w[0] == "refused" and int(w[1]) == want[1] and want[2] in line, (line, want)
        return
    assert w[0] == "ok", (line, want)
    s, f, r, m = w.index("S"), w.index("F"), w.index("R"), w.index("M")
    got = ([int(v) for v in w[s + 1:f]], [int(v) for v in w[f + 1:r]], [int(v) for v in w[r + 1:m]])
    assert got == (want[1], want[2], want[3]), (line, want)
    assert int(w[m + 1]) == sum(1 << b for b in want[3])


def test_member_partition_and_refusals_under_sanitizers(plan_program, tmp_path):
    """Every refusal of the issue by name, the partitions of the GPU tests (a skipped member, a late starter beside
    registering members, all first, B = 1, B = 32), and 400 random member tables against the model above."""
    cases = [
        ([_member(), _member(), _member()], False),
        ([_member(frame_index=0)] * 3, False),
        ([_member(), _member(skip=1, has_sequence=0, registering=1), _member()], False),      # nothing of a skipped member is read
        ([_member(), _member(), _member(frame_index=0)], False),                               # a late starter
        ([_member()], False),
        ([_member(frame_index=b % 3) for b in range(32)], False),
        ([_member(voxel_size=0.0, targets=0), _member(voxel_size=-1.0, targets=0)], False),    # no grid sample either way
        ([_member(), _member(has_sequence=0)], False),
        ([_member(), _member()], True),
        ([_member(skip=1), _member(skip=1)], False),
        ([_member(), _member(point_to_point=1)], False),
        ([_member(projective_map=1), _member()], False),
        ([_member(), _member(exchange=1)], False),
        ([_member(), _member(profiling=1)], False),
        ([_member(), _member(), _member(registering=1)], False),
        ([_member(), _member(frame_launched=1)], False),
        ([_member(), _member(voxel_size=0.3)], False),
        ([_member(), _member(skip=1, voxel_size=0.3), _member(targets=0)], False),
        ([_member(), _member(stream=8)], False),
    ]
    rng = np.random.default_rng(11)
    for _ in range(400):
        n = int(rng.integers(1, 33))
        members = []
        for _b in range(n):
            flags = {k: int(rng.random() < 0.03) for k in ("point_to_point", "projective_map", "exchange", "profiling",
                                                            "registering", "frame_launched")}
            members.append(_member(skip=int(rng.random() < 0.3), has_sequence=int(rng.random() > 0.03),
                                   frame_index=int(rng.integers(0, 4)), voxel_size=0.4 if rng.random() > 0.04 else 0.0,
                                   targets=int(rng.random() > 0.04), stream=7 if rng.random() > 0.03 else 9, **flags))
        cases.append((members, bool(rng.random() < 0.05)))
    out = _run(plan_program, tmp_path, [_plan_line(m, p) for m, p in cases])
    assert len(out) == len(cases)
    kinds = set()
    for line, (members, pending) in zip(out, cases):
        _check_plan(line, members, pending)
        kinds.add(line.split()[0])
    assert kinds == {"ok", "refused"}
    # an empty table and one beyond ICP_BATCH_MAX_SEQUENCES are refused without a member being read
    out = _run(plan_program, tmp_path, ["P 0 0", _plan_line([_member()] * 33, False)])
    assert all(line.startswith("refused -1") for line in out) and len(out) == 2


def test_update_members_and_end_refusal_under_sanitizers(plan_program, tmp_path):
    """The map update runs over the members whose registration succeeded, in order; the call's status is the first failure's;
    an end with nothing launched is refused."""
    out = _run(plan_program, tmp_path, ["U 3 0 0 1 -3 2 0", "U 3 4 -3 5 -2 9 0", "U 1 0 0", "U 0", "U 2 1 -3 2 -3", "E 0", "E 1"])
    assert out == ["update 0 2 first -3", "update 9 first -3", "update 0 first 0", "update first 0", "update first -3",
                   "refused no step launched (icp_batch_frame_launch first)", "ok"]


# ---- the batched plugin's flag ------------------------------------------------------------------------------------------
def test_batched_one_call_frame_refusals(monkeypatch):
    import torch
    import pylidar_slam_amd.odometry as odo_mod
    from oracle_context import OracleContext

    class FakeBatch:
        def __init__(self, contexts):
            self.contexts = contexts

        def use_torch_stream(self):
            pass

        def odometry_init(self, **kw):
            raise RuntimeError("must not be reached")

        frame_launch = frame_end = odometry_init

    class WithFrameCalls(OracleContext):
        def frame_launch(self, *a, **k):
            raise RuntimeError("must not be reached")

    assert odo_mod.MI355XICPConfig().one_call_frame is False
    monkeypatch.setattr(odo_mod, "IcpContext", WithFrameCalls)
    monkeypatch.setattr(odo_mod, "IcpBatch", FakeBatch)
    proj = odo_mod.SphericalProjector(16, 256)
    cpu = torch.device("cpu")
    with pytest.raises(AssertionError, match="projective"):
        odo_mod.MI355XICPFrameToModelBatch(odo_mod.MI355XICPConfig(
            one_call_frame=True, local_map=dict(type="projective_local_map", local_map_size=3)), 2, projector=proj, device=cpu)
    with pytest.raises(AssertionError, match="compact_sparse_vertex_map"):
        odo_mod.MI355XICPFrameToModelBatch(odo_mod.MI355XICPConfig(one_call_frame=True, compact_sparse_vertex_map=True), 2,
                                           projector=proj, device=cpu)
    odo = odo_mod.MI355XICPFrameToModelBatch(odo_mod.MI355XICPConfig(one_call_frame=True, data_key="vertex_map"), 2,
                                             projector=proj, device=cpu)
    assert odo._one_call is True
    odo.init()
    with pytest.raises(AssertionError, match="vertex-map tensor"):
        odo.process_next_frames([{"vertex_map": torch.zeros(1, 3, 16, 256)}, {"vertex_map": torch.zeros(1, 3, 16, 256)}])
    with pytest.raises(AssertionError, match="Could not find the key"):
        odo.process_next_frames([{"other": None}, {"other": None}])
    with pytest.raises(AssertionError, match="expected 2 frames"):
        odo.process_next_frames([{"vertex_map": np.zeros((4, 3), np.float32)}])
    # the default path is untouched by the field: numpy frames stay refused there
    plain = odo_mod.MI355XICPFrameToModelBatch(odo_mod.MI355XICPConfig(data_key="vertex_map"), 2, projector=proj, device=cpu)
    assert plain._one_call is False
    plain.init()
    with pytest.raises(AssertionError, match="not numpy input"):
        plain.process_next_frames([{"vertex_map": np.zeros((4, 3), np.float32)}] * 2)
