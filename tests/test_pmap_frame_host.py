"""CPU side of the projective one-call frame (icp_pmap_odometry_init / icp_pmap_frame_launch / icp_pmap_frame_end /
icp_pmap_register_launch, include/icp_mi355x.h):

* the calls and the config struct are declared, exported and bound with the header's layout and defaults;
* the drives of tests/test_gpu_pmap_frame.py (tests/pmap_frame_cases.py) keep every frame's key-frame quantities at least
  10 % away from both thresholds on the numpy oracle `ICPProjectiveOracle` — a condition on the INPUTS of the bit-for-bit GPU
  comparisons — with both kinds of map update and the evictions the drives are built for;
* the plugin's `one_call_projective_frame` field: default, yaml, and the refusals that name their reason."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import frame_cases as FC
import pmap_frame_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "icp_mi355x.h")
CALLS = ("icp_default_pmap_frame_config", "icp_pmap_odometry_init", "icp_pmap_frame_launch", "icp_pmap_frame_end",
         "icp_pmap_register_launch")


# ---- header and binding --------------------------------------------------------------------------------------------
def test_pmap_frame_calls_are_declared_exported_and_bound():
    from pylidar_slam_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.library_path())
    for name in CALLS:
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} is not declared in include/icp_mi355x.h"
        assert name in _lib.EXPORTED_SYMBOLS, f"{name} is not bound in _lib.EXPORTED_SYMBOLS"
        assert hasattr(lib, name), f"{name} is not exported by the library"
    assert "typedef struct icp_pmap_frame_config" in text
    assert re.search(r"ICP_FRAME_ROWS\s*=\s*0\s*,\s*ICP_FRAME_VERTEX_MAP\s*=\s*1", text)
    assert (_lib.FRAME_ROWS, _lib.FRAME_VERTEX_MAP) == (0, 1)
    # the block that documents the calls cites the reference lines they replace
    doc = open(HEADER).read()
    block = doc[doc.index("one call per odometry frame against the projective local map"):
                doc.index("typedef struct icp_pmap_frame_config")]
    for cite in ("icp_odometry.py:157-246", "local_map.py:113-235", ":248-299", "local_map.py:205-235", ":128-145", ":319-358",
                 ":301-308", ":360-380", "local_map.py:122-174", ":176", ":286"):
        assert cite in block, cite
    # the kd-tree frame config did not grow
    assert ctypes.sizeof(_lib.IcpFrameConfig) == 8 + 6 * 4


def test_pmap_frame_config_layout_matches_the_header(tmp_path):
    """sizeof / offsetof of icp_pmap_frame_config as the C compiler lays the header out, against the ctypes structure."""
    from pylidar_slam_amd import _lib
    cc = shutil.which("gcc") or shutil.which("cc") or shutil.which("clang")
    assert cc, "no C compiler"
    names = [f[0] for f in _lib.IcpPmapFrameConfig._fields_]
    assert names == ["voxel_size", "threshold_trans", "threshold_rot", "constant_velocity", "targets", "normals_kernel_size",
                     "copy_cloud"]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "icp_mi355x.h"', 'int main(void) {',
           '  printf("size %zu\\n", sizeof(icp_pmap_frame_config));']
    src += [f'  printf("{n} %zu\\n", offsetof(icp_pmap_frame_config, {n}));' for n in names]
    src += ['  return 0;', '}']
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.run([cc, "-std=c99", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    out = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert ctypes.sizeof(_lib.IcpPmapFrameConfig) == int(out["size"]) == 8 + 6 * 4
    for n in names:
        assert getattr(_lib.IcpPmapFrameConfig, n).offset == int(out[n]), n


def test_default_pmap_frame_config():
    from pylidar_slam_amd import _lib
    lib = _lib.load_library()
    cfg = _lib.IcpPmapFrameConfig()
    lib.icp_default_pmap_frame_config(ctypes.byref(cfg))
    assert cfg.voxel_size == 0.0 and cfg.constant_velocity == 1 and cfg.targets == 0 and cfg.copy_cloud == 1
    assert cfg.normals_kernel_size == 5
    assert abs(cfg.threshold_trans - 0.1) < 1e-7 and abs(cfg.threshold_rot - 0.3) < 1e-7  # icp_odometry.py:29-64


# ---- the fixture condition of the GPU drives ---------------------------------------------------------------------------
_ORACLE_RUNS = {}


def _oracle_run(name):
    if name not in _ORACLE_RUNS:
        d = PC.drive(name)
        # (the configuration the GPU file drives the flagged plugin with: the drive's own settings and thresholds)
        cfg = PC.plugin_config(d, one_call_projective_frame=True)
        assert cfg.one_call_projective_frame is True and cfg.threshold_trans == PC.THRESHOLD_TRANS
        assert cfg.local_map["local_map_size"] == d.local_map_size and cfg.max_num_alignments == d.max_num_alignments
        _ORACLE_RUNS[name] = PC.run_on_oracle(d)
    return _ORACLE_RUNS[name]


@pytest.mark.parametrize("name", PC.NAMES)
def test_drive_keeps_clear_of_the_key_frame_thresholds_on_the_projective_oracle(name):
    """Every frame's |t| and |r| 180 / pi at least 10 % from its threshold on `ICPProjectiveOracle`, both kinds of update in
    every drive (the GPU poses agree with the oracle's to 1e-4 m / 1e-4 rad: the margins are 0.07 m and 8 degrees at the
    least)."""
    d = PC.drive(name)
    rel, windows = _oracle_run(name)
    rows = FC.key_frame_margins(rel)
    assert len(rows) == d.frames - 1
    for f, (_, _, _, trans, rot, _) in enumerate(rows, start=1):
        assert abs(trans - PC.THRESHOLD_TRANS) >= 0.10 * PC.THRESHOLD_TRANS, (name, f, trans)
        assert abs(rot - PC.THRESHOLD_ROT) >= 0.10 * PC.THRESHOLD_ROT, (name, f, rot)
    keys = sum(1 for r in rows if r[5])
    assert keys >= 1 and len(rows) - keys >= 1, (name, keys)
    assert max(windows) <= d.local_map_size and windows[0] == 1


def test_the_drives_evict_where_they_are_built_to():
    """`vmap`: a window of 2, key frames at 2 and 4 — the one at frame 4 evicts; `rows_pixels`: a window of 3, key frames at
    2, 4, 6, 8 — those at 6 and 8 evict."""
    for name, key_frames, evicting in (("vmap", [2, 4], [4]), ("rows_pixels", [2, 4, 6, 8], [6, 8])):
        d = PC.drive(name)
        rel, windows = _oracle_run(name)
        rows = FC.key_frame_margins(rel)
        assert [f for f, r in enumerate(rows, start=1) if r[5]] == key_frames, name
        # a key frame that leaves the window size where it was has pushed the oldest map out
        assert [f for f in key_frames if windows[f] == windows[f - 1] == d.local_map_size] == evicting, (name, windows)


# ---- the plugin's flag ---------------------------------------------------------------------------------------------------
PROJECTIVE = dict(type="projective_local_map", local_map_size=3)


def test_one_call_projective_frame_field_and_refusals(monkeypatch):
    import torch
    import pylidar_slam_amd.odometry as odo_mod
    from oracle_context import OracleContext
    assert odo_mod.MI355XICPConfig().one_call_projective_frame is False
    yaml = open(os.path.join(ROOT, "config", "slam", "odometry", "icp_odometry_mi355x.yaml")).read()
    assert re.search(r"^one_call_projective_frame:\s*false\s*$", yaml, flags=re.M)
    monkeypatch.setattr(odo_mod, "IcpContext", OracleContext)
    proj = odo_mod.SphericalProjector(16, 256)
    cpu = torch.device("cpu")
    # a context without the library's projective frame calls (the numpy stand-in): refused, not routed to the per-call path
    with pytest.raises(AssertionError, match="projective frame calls"):
        odo_mod.MI355XICPFrameToModel(odo_mod.MI355XICPConfig(one_call_projective_frame=True, local_map=PROJECTIVE),
                                      projector=proj, device=cpu)

    class WithFrameCalls(OracleContext):
        def pmap_init(self):
            pass

        def pmap_frame_launch(self, *a, **k):
            raise RuntimeError("must not be reached")

        pmap_odometry_init = pmap_frame_launch

    monkeypatch.setattr(odo_mod, "IcpContext", WithFrameCalls)
    # the kd-tree style map has one_call_frame
    with pytest.raises(AssertionError, match="kd-tree style map"):
        odo_mod.MI355XICPFrameToModel(odo_mod.MI355XICPConfig(one_call_projective_frame=True), projector=proj, device=cpu)
    odo = odo_mod.MI355XICPFrameToModel(odo_mod.MI355XICPConfig(one_call_projective_frame=True, data_key="vertex_map",
                                                                local_map=PROJECTIVE), projector=proj, device=cpu)
    odo.init()
    with pytest.raises(AssertionError, match="a cpu tensor"):
        odo.process_next_frame({"vertex_map": torch.zeros(1, 3, 16, 256)})
    with pytest.raises(AssertionError, match="a cpu tensor"):
        odo.process_next_frame({"vertex_map": torch.zeros(100, 3)})
    with pytest.raises(AssertionError, match=r"expected \[N, 3\]"):
        odo.process_next_frame({"vertex_map": np.zeros((100, 4), np.float32)})
    with pytest.raises(AssertionError, match="Could not find the key"):
        odo.process_next_frame({"other": None})
    # the default path is untouched by the field
    plain = odo_mod.MI355XICPFrameToModel(odo_mod.MI355XICPConfig(data_key="vertex_map", local_map=PROJECTIVE),
                                          projector=proj, device=cpu)
    assert plain._one_call_pmap is False and plain._one_call is False


# ---- the batched calls: binding, and the plan header under the host sanitizers --------------------------------------------
CSRC = os.path.join(ROOT, "pylidar-slam_amd", "csrc")
BATCH_CALLS = ("icp_batch_pmap_odometry_init", "icp_batch_pmap_frame_launch", "icp_batch_pmap_frame_end")
PLAN_FIELDS = ("skip", "has_sequence", "kd_sequence", "frame_index", "voxel_size", "targets", "normals_kernel_size",
               "point_to_point", "exchange", "profiling", "registering", "frame_launched", "has_timestamps", "n", "pixels",
               "stream")


def test_batched_pmap_frame_calls_are_declared_exported_and_bound():
    from pylidar_slam_amd import _lib
    from pylidar_slam_amd.engine import IcpBatch
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.library_path())
    for name in BATCH_CALLS:
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} is not declared in include/icp_mi355x.h"
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
    for name in ("pmap_odometry_init", "pmap_frame_launch", "pmap_frame_end"):
        assert callable(getattr(IcpBatch, name))
    # the kd-tree plan header is as it was: the projective plan has a header of its own, without a HIP dependency
    plan = open(os.path.join(CSRC, "batch_pmap_frame_plan.h")).read()
    assert "#include <hip" not in plan and "icp_internal.h" not in plan and "batch_pmap_frame_plan(" in plan


@pytest.fixture(scope="module")
def pmap_plan_program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    exe = tmp_path_factory.mktemp("pmap_plan") / "batch_pmap_frame_plan_check"
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(cxx).startswith("g++") else []
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", *static, "-I", CSRC,
                    os.path.join(ROOT, "tests", "native", "batch_pmap_frame_plan_check.cpp"), "-o", str(exe)], check=True)
    return str(exe)


def _pm(**kw):
    m = dict(skip=0, has_sequence=1, kd_sequence=0, frame_index=3, voxel_size=0.0, targets=1, normals_kernel_size=5,
             point_to_point=0, exchange=0, profiling=0, registering=0, frame_launched=0, has_timestamps=0, n=8192, pixels=8192,
             stream=7)
    m.update(kw)
    return m


def _plan_line(members, pending=False, vmap=False, host=False):
    words = ["P", str(len(members)), str(int(pending)), str(int(vmap)), str(int(host))]
    for m in members:
        words += [repr(float(m[k])) if k == "voxel_size" else str(int(m[k])) for k in PLAN_FIELDS]
    return " ".join(words)


def _plan_model(members, pending, vmap, host):
    """The plan as the header documents it: ('ok', skipped, first, registering) or ('refused', member, word of the reason)."""
    if not 1 <= len(members) <= 32:
        return ("refused", -1, "1 to 32 members")
    if pending:
        return ("refused", -1, "already launched")
    if vmap and host:
        return ("refused", -1, "device memory")
    lead = None
    for b, m in enumerate(members):
        if m["skip"]:
            continue
        checks = [(m["kd_sequence"], "kd-tree sequence"), (not m["has_sequence"], "no sequence"), (m["frame_index"] < 0, "frame index"),
                  (m["point_to_point"], "point-to-point"), (m["exchange"], "exchange"), (m["profiling"], "profiling"),
                  (m["registering"], "registration of the member's own"), (m["frame_launched"], "awaits icp_pmap_frame_end"),
                  (m["n"] < 0 or m["n"] > 2 ** 31 - 1, "row count"), (vmap and m["n"] != m["pixels"], "H*W"),
                  (vmap and (m["has_timestamps"] or m["voxel_size"] > 0), "go with rows")]
        for bad, word in checks:
            if bad:
                return ("refused", b, word)
        if lead is None:
            lead = m
            continue
        checks = [(m["voxel_size"] != lead["voxel_size"] and not (m["voxel_size"] <= 0 and lead["voxel_size"] <= 0), "voxel_size differs"),
                  (not vmap and m["targets"] != lead["targets"], "targets differs"),
                  (m["normals_kernel_size"] != lead["normals_kernel_size"], "normals_kernel_size differs"),
                  (m["pixels"] != lead["pixels"], "height and width"), (m["stream"] != lead["stream"], "one stream")]
        for bad, word in checks:
            if bad:
                return ("refused", b, word)
    if lead is None:
        return ("refused", -1, "every member is skipped")
    idx = range(len(members))
    return ("ok", [b for b in idx if members[b]["skip"]], [b for b in idx if not members[b]["skip"] and members[b]["frame_index"] == 0],
            [b for b in idx if not members[b]["skip"] and members[b]["frame_index"] > 0])


def _check_plan_line(line, members, pending, vmap, host):
    body, same = line.rsplit(" | ", 1)
    assert same == "same", line  # no member changes, refused or not
    want = _plan_model(members, pending, vmap, host)
    w = body.split()
    if want[0] == "refused":
        assert w[0] == "refused" and int(w[1]) == want[1] and want[2] in body, (line, want)
        return want[2]
    assert w[0] == "ok", (line, want)
    s, f, r, v = w.index("S"), w.index("F"), w.index("R"), w.index("V")
    assert [int(x) for x in w[s + 1:f]] == want[1] and [int(x) for x in w[f + 1:r]] == want[2]
    assert [int(x) for x in w[r + 1:v]] == want[3] and int(w[v + 1]) == int(vmap)
    return "ok"


def _run_plan(program, tmp_path, lines):
    cases = tmp_path / "cases.txt"
    cases.write_text("\n".join(lines) + "\n")
    r = subprocess.run([program, str(cases)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-2000:]
    return r.stdout.splitlines()


def test_pmap_member_partition_and_refusals_under_sanitizers(pmap_plan_program, tmp_path):
    """Every refusal by name, the partitions of the GPU tests (a skipped member, a late starter beside registering members,
    all first, B = 1, B = 32, both layouts), and 3000 random member tables against the model above; no member changes."""
    hand = [
        ([_pm(), _pm(), _pm()], False, False, False),
        ([_pm(), _pm(), _pm()], False, True, False),
        ([_pm(frame_index=0)] * 3, False, True, False),
        ([_pm(), _pm(skip=1, has_sequence=0, registering=1, kd_sequence=1), _pm()], False, False, False),  # nothing of a skipped member is read
        ([_pm(), _pm(), _pm(frame_index=0)], False, False, True),                                       # a late starter, host rows
        ([_pm()], False, True, False),
        ([_pm(frame_index=b % 3) for b in range(32)], False, False, False),
        ([_pm(targets=0), _pm(targets=1)], False, True, False),                                         # vertex maps: targets unread
        ([_pm(voxel_size=0.4, n=100), _pm(voxel_size=0.4, n=0, has_timestamps=1)], False, False, True),
        ([_pm(), _pm()], True, False, False),
        ([_pm(), _pm()], False, True, True),
        ([_pm(skip=1), _pm(skip=1)], False, False, False),
        ([_pm(), _pm(kd_sequence=1)], False, False, False),
        ([_pm(), _pm(has_sequence=0)], False, False, False),
        ([_pm(), _pm(frame_index=-1)], False, False, False),
        ([_pm(point_to_point=1), _pm()], False, False, False),
        ([_pm(), _pm(exchange=1)], False, False, False),
        ([_pm(), _pm(profiling=1)], False, False, False),
        ([_pm(), _pm(registering=1)], False, False, False),
        ([_pm(), _pm(frame_launched=1)], False, False, False),
        ([_pm(), _pm(n=-1)], False, False, False),
        ([_pm(), _pm(n=4096)], False, True, False),
        ([_pm(), _pm(has_timestamps=1)], False, True, False),
        ([_pm(voxel_size=0.4), _pm(voxel_size=0.4)], False, True, False),
        ([_pm(voxel_size=0.4), _pm(voxel_size=0.2)], False, False, False),
        ([_pm(targets=0), _pm(targets=1)], False, False, False),
        ([_pm(), _pm(normals_kernel_size=3)], False, False, False),
        ([_pm(), _pm(pixels=4096, n=4096)], False, True, False),
        ([_pm(), _pm(stream=8)], False, False, False),
    ]
    rng = np.random.default_rng(20261019)
    rare = lambda p: int(rng.random() < p)
    cases = list(hand)
    for _ in range(3000):
        count = int(rng.integers(1, 7))
        vmap = bool(rare(0.4))
        members = [_pm(skip=rare(0.2), has_sequence=1 - rare(0.03), kd_sequence=rare(0.03), frame_index=int(rng.integers(-1, 4)) if rare(0.5) else 2,
                       voxel_size=float(rng.choice([0.0, 0.0, 0.0, 0.4])) if not vmap or rare(0.1) else 0.0, targets=1 - rare(0.1),
                       normals_kernel_size=5 if not rare(0.05) else 3, point_to_point=rare(0.03), exchange=rare(0.03), profiling=rare(0.03),
                       registering=rare(0.03), frame_launched=rare(0.03), has_timestamps=rare(0.05), n=8192 if not rare(0.05) else 100,
                       pixels=8192 if not rare(0.03) else 4096, stream=7 if not rare(0.05) else 9) for _ in range(count)]
        cases.append((members, bool(rare(0.03)), vmap, bool(rare(0.1))))
    out = _run_plan(pmap_plan_program, tmp_path, [_plan_line(*c) for c in cases])
    assert len(out) == len(cases)
    seen = {_check_plan_line(line, *c) for line, c in zip(out, cases)}
    every = {"ok", "1 to 32 members", "already launched", "device memory", "kd-tree sequence", "no sequence", "frame index",
             "point-to-point", "exchange", "profiling", "registration of the member's own", "awaits icp_pmap_frame_end", "row count",
             "H*W", "go with rows", "voxel_size differs", "targets differs", "normals_kernel_size differs", "height and width",
             "one stream", "every member is skipped"}
    out2 = _run_plan(pmap_plan_program, tmp_path, ["P 0 0 0 0", _plan_line([_pm()] * 33), "E 0", "E 1"])
    assert out2[0].startswith("refused -1 1 to 32") and out2[1].startswith("refused -1 1 to 32")
    assert out2[2] == "refused no step launched (icp_batch_pmap_frame_launch first)" and out2[3] == "ok"
    assert seen | {"1 to 32 members"} == every, every - seen


def test_batched_one_call_projective_frame_refusals(monkeypatch):
    """The batch plugin with the flag: refused without the library's batched calls and on cpu tensors, before any call."""
    import torch
    import pylidar_slam_amd.odometry as odo_mod
    from oracle_context import OracleContext

    class Ctx(OracleContext):
        def pmap_init(self):
            pass

        def pmap_frame_launch(self, *a, **k):
            raise RuntimeError("must not be reached")

    class NoCalls:
        def __init__(self, contexts):
            self.contexts = contexts

    class WithCalls(NoCalls):
        def pmap_frame_launch(self, *a, **k):
            raise RuntimeError("must not be reached")

        pmap_odometry_init = use_torch_stream = pmap_frame_launch

    monkeypatch.setattr(odo_mod, "IcpContext", Ctx)
    proj = odo_mod.SphericalProjector(16, 256)
    cfg = odo_mod.MI355XICPConfig(one_call_projective_frame=True, data_key="vertex_map", local_map=PROJECTIVE)
    monkeypatch.setattr(odo_mod, "IcpBatch", NoCalls)
    with pytest.raises(AssertionError, match="batched projective frame calls"):
        odo_mod.MI355XICPFrameToModelBatch(cfg, 2, projector=proj, device=torch.device("cpu"))
    monkeypatch.setattr(odo_mod, "IcpBatch", WithCalls)
    odo = odo_mod.MI355XICPFrameToModelBatch(cfg, 2, projector=proj, device=torch.device("cpu"))
    odo.init()
    with pytest.raises(AssertionError, match="a cpu tensor"):
        odo.process_next_frames([{"vertex_map": torch.zeros(3, 16, 256)}] * 2)
    with pytest.raises(AssertionError, match="expected 2 frames"):
        odo.process_next_frames([{"vertex_map": torch.zeros(3, 16, 256)}])
    with pytest.raises(AssertionError, match="kd-tree style map"):
        odo_mod.MI355XICPFrameToModelBatch(odo_mod.MI355XICPConfig(one_call_projective_frame=True), 2, projector=proj,
                                           device=torch.device("cpu"))
