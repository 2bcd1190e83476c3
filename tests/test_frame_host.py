"""CPU side of the one-call frame (icp_odometry_init / icp_frame_launch / icp_frame_end, include/icp_mi355x.h):

* the three calls and the two structs are declared, exported and bound with the header's layout;
* the drives of tests/test_gpu_frame.py keep every frame's key-frame quantities away from the thresholds (a condition on
  the INPUTS of the bit-for-bit GPU comparisons: a one-ulp difference between numpy's 4x4 float32 product and the
  library's cannot flip a decision there), checked on the plugin driven by the numpy oracle;
* the key-frame arithmetic of icp_frame_end (csrc/frame_keyframe.h) as a stand-alone program under
  -fsanitize=address,undefined, against numpy / from_pose_matrix values recorded in tests/golden/frame_keyframe.npz;
* the plugin's `one_call_frame` field: default, yaml, and the refusals that name their reason."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import frame_cases as FC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "icp_mi355x.h")
CSRC = os.path.join(ROOT, "pylidar-slam_amd", "csrc")
U = 2.0 ** -24  # unit roundoff of float32


# ---- header and binding --------------------------------------------------------------------------------------------
def test_frame_calls_are_declared_and_bound():
    from pylidar_slam_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in ("icp_odometry_init", "icp_frame_launch", "icp_frame_end", "icp_default_frame_config"):
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} is not declared in include/icp_mi355x.h"
        assert name in _lib.EXPORTED_SYMBOLS, f"{name} is not bound in _lib.EXPORTED_SYMBOLS"
    assert "typedef struct icp_frame_config" in text and "typedef struct icp_frame_result" in text
    # the block that documents the calls cites the reference lines they replace
    doc = open(HEADER).read()
    block = doc[doc.index("one call per odometry frame"):doc.index("typedef struct icp_frame_config")]
    for cite in ("icp_odometry.py:157-246", "319-358", "360-380", "slam/preprocessing.py:144-191", ":207-226", ":101-126",
                 "slam/initialization.py:103-119"):
        assert cite in block, cite


def test_frame_struct_layouts_match_the_header(tmp_path):
    """sizeof / offsetof of the two structs as the C compiler lays the header out, against the ctypes structures."""
    from pylidar_slam_amd import _lib
    cc = shutil.which("gcc") or shutil.which("cc") or shutil.which("clang")
    assert cc, "no C compiler"
    fields = {"icp_frame_config": [f[0] for f in _lib.IcpFrameConfig._fields_],
              "icp_frame_result": [f[0] for f in _lib.IcpFrameResult._fields_]}
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "icp_mi355x.h"', 'int main(void) {']
    for s, names in fields.items():
        src.append(f'  printf("{s} %zu\\n", sizeof({s}));')
        for n in names:
            src.append(f'  printf("{s}.{n} %zu\\n", offsetof({s}, {n}));')
    src += ['  return 0;', '}']
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.run([cc, "-std=c99", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    out = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for s, cls in (("icp_frame_config", _lib.IcpFrameConfig), ("icp_frame_result", _lib.IcpFrameResult)):
        assert ctypes.sizeof(cls) == int(out[s]), s
        for n in fields[s]:
            assert getattr(cls, n).offset == int(out[f"{s}.{n}"]), (s, n)
    assert ctypes.sizeof(_lib.IcpFrameConfig) == 8 + 6 * 4
    assert ctypes.sizeof(_lib.IcpFrameResult) == ctypes.sizeof(_lib.IcpRegisterResult) + 2 * 4 + 2 * 8


def test_default_frame_config():
    from pylidar_slam_amd import _lib
    lib = _lib.load_library()
    cfg = _lib.IcpFrameConfig()
    lib.icp_default_frame_config(ctypes.byref(cfg))
    assert cfg.voxel_size == 0.0 and cfg.constant_velocity == 1 and cfg.targets == 0 and cfg.copy_cloud == 1
    assert abs(cfg.threshold_trans - 0.1) < 1e-7 and abs(cfg.threshold_rot - 0.3) < 1e-7  # icp_odometry.py:29-64


# ---- the fixture condition of GPU tests 1-4 --------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sampled", "sampled_live", "raw", "raw_p2p", "deskew"])
def test_drive_keeps_clear_of_the_key_frame_thresholds(monkeypatch, name):
    """No frame's |t| or |r| 180 / pi within a relative 1e-3 of its threshold, on the plugin driven by the numpy oracle
    (the GPU poses agree with the oracle's to 1e-4 m / 1e-4 rad, BASELINE.json: the margins found here are 0.09 m and
    8 degrees at the least)."""
    import pylidar_slam_amd.odometry as odo_mod
    from oracle_context import OracleContext
    monkeypatch.setattr(odo_mod, "IcpContext", OracleContext)
    d = FC.drive(name)
    _, odo = FC.run_plugin_on_oracle(d)
    rows = FC.key_frame_margins(odo.get_relative_poses())
    assert len(rows) == d.frames - 1
    for f, (_, _, _, trans, rot, _) in enumerate(rows, start=1):
        assert abs(trans - FC.THRESHOLD_TRANS) > 1e-3 * FC.THRESHOLD_TRANS, (name, f, trans)
        assert abs(rot - FC.THRESHOLD_ROT) > 1e-3 * FC.THRESHOLD_ROT, (name, f, rot)
    keys = sum(1 for r in rows if r[5])
    if d.frames >= 10:  # (GPU tests 1, 2 and 6 assert at least two updates of each kind)
        assert keys >= 2 and len(rows) - keys >= 2, (name, keys)
    else:
        assert keys >= 1 and len(rows) - keys >= 1, (name, keys)
    # the oracle's map saw what the decisions say: an insertion per key frame, a move per other frame
    calls = odo.ctx.calls
    assert calls.count("insert_staged") == keys and calls.count("move") == len(rows) - keys


# ---- the key-frame arithmetic under the host sanitizers ----------------------------------------------------------------
def _bits(a):
    return " ".join("%08x" % v for v in np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32))


def _from_bits(words):
    return np.array([int(w, 16) for w in words], np.uint32).view(np.float32)


@pytest.fixture(scope="module")
def keyframe_program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    exe = tmp_path_factory.mktemp("keyframe") / "keyframe_check"
    # (the sanitizer runtimes linked statically — clang's default — so that the program stands alone whatever the environment
    # preloads)
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(cxx).startswith("g++") else []
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", *static, "-I", CSRC,
                    os.path.join(ROOT, "tests", "native", "keyframe_check.cpp"), "-o", str(exe)], check=True)
    return str(exe)


def _run_cases(program, tmp_path, deltas, poses, thr_trans, thr_rot):
    cases = tmp_path / "cases.txt"
    lines = ["%d %s" % (len(poses), _bits([thr_trans, thr_rot]))]
    lines += [_bits(d) + " " + _bits(p) for d, p in zip(deltas, poses)]
    cases.write_text("\n".join(lines) + "\n")
    r = subprocess.run([program, str(cases)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-2000:]
    out = []
    for line in r.stdout.splitlines():
        w = line.split()
        out.append((int(w[0]), _from_bits(w[1:17]).reshape(4, 4), _from_bits(w[17:23]), float(w[23]), float(w[24])))
    assert len(out) == len(poses)
    return out


def test_key_frame_arithmetic_under_sanitizers(keyframe_program, tmp_path):
    """Per frame of the `sampled` drive (delta and pose as numpy had them): the decision equal; every element of delta x pose
    within 8 u sum_k |delta_ik| |pose_kj| of numpy's (two float32 evaluations of a four-term dot product, in whatever order
    and with or without fused multiply-adds, each lie within gamma_4 <= 4.000001 u of the exact one); |t| and |r| within what
    that moves them by plus 8 ulp for sqrtf / atan2f: 2e-6 m, 2e-6 rad = 1.2e-4 degrees (the margins to the thresholds are
    0.09 m and 8 degrees)."""
    g = np.load(FC.GOLDEN_KEYFRAME)
    assert np.array_equal(g["key_frame"], [r[5] for r in FC.key_frame_margins(g["rel"])])  # the fixture is the replay of its poses
    out = _run_cases(keyframe_program, tmp_path, g["delta"], g["rel"][1:], float(g["threshold_trans"]), float(g["threshold_rot"]))
    assert g["key_frame"].sum() >= 2 and (~g["key_frame"]).sum() >= 2
    for f, (key, new_delta, params, trans, rot) in enumerate(out):
        assert key == int(g["key_frame"][f]), f
        bound = 8 * U * (np.abs(g["delta"][f].astype(np.float64)) @ np.abs(g["rel"][f + 1].astype(np.float64)))
        assert (np.abs(new_delta.astype(np.float64) - g["new_delta"][f]) <= bound).all(), (f, new_delta - g["new_delta"][f])
        assert np.abs(params[:3] - g["params"][f][:3]).max() <= 2e-6 and np.abs(params[3:] - g["params"][f][3:]).max() <= 2e-6
        assert abs(trans - g["trans"][f]) <= 2e-6 and abs(rot - g["rot_deg"][f]) <= 1.2e-4, (f, trans, rot)


def test_key_frame_arithmetic_edges_under_sanitizers(keyframe_program, tmp_path):
    """Identity, a motion exactly at neither threshold, and the gimbal-lock branch of from_pose_matrix (pitch = pi / 2),
    against `from_pose_matrix` of this package."""
    from pylidar_slam_amd.odometry import build_pose_matrix, from_pose_matrix
    eye = np.eye(4, dtype=np.float32)
    poses = [eye, build_pose_matrix([0.05, 0.0, 0.0, 0.0, 0.0, 0.001]), build_pose_matrix([1.0, 2.0, 3.0, 0.3, np.pi / 2, 0.0]),
             build_pose_matrix([0.0, 0.0, 0.0, 0.0, 0.0, 0.02])]
    deltas = [eye, build_pose_matrix([0.04, 0.0, 0.0, 0.0, 0.0, 0.0]), eye, eye]
    out = _run_cases(keyframe_program, tmp_path, deltas, poses, 0.1, 0.3)
    want_keys = [0, 0, 1, 1]  # nothing; 9 cm and 0.06 degrees; metres; 1.15 degrees of yaw alone
    for (key, new_delta, params, trans, rot), d, p, want in zip(out, deltas, poses, want_keys):
        ref = (d @ p).astype(np.float32)
        dp = from_pose_matrix(ref)
        assert key == want
        np.testing.assert_allclose(new_delta, ref, atol=1e-6)
        np.testing.assert_allclose(params, dp, atol=2e-6)
        assert abs(trans - np.linalg.norm(dp[:3])) <= 4e-6 and abs(rot - np.linalg.norm(dp[3:]) * 180 / np.pi) <= 2e-4
    assert out[0][3] == 0.0 and out[0][4] == 0.0 and np.array_equal(out[0][1], eye)
    assert out[2][2][5] == 0.0  # the gimbal-lock branch sets the yaw to zero


# ---- the plugin's flag ---------------------------------------------------------------------------------------------------
def test_one_call_frame_field_and_refusals(monkeypatch):
    import torch
    import pylidar_slam_amd.odometry as odo_mod
    from oracle_context import OracleContext
    assert odo_mod.MI355XICPConfig().one_call_frame is False
    yaml = open(os.path.join(ROOT, "config", "slam", "odometry", "icp_odometry_mi355x.yaml")).read()
    assert re.search(r"^one_call_frame:\s*false\s*$", yaml, flags=re.M)
    monkeypatch.setattr(odo_mod, "IcpContext", OracleContext)
    proj = odo_mod.SphericalProjector(16, 256)
    cpu = torch.device("cpu")
    # a context without the library's frame calls (the numpy stand-in): refused, not routed to the per-call path
    with pytest.raises(AssertionError, match="frame calls"):
        odo_mod.MI355XICPFrameToModel(odo_mod.MI355XICPConfig(one_call_frame=True), projector=proj, device=cpu)

    class WithFrameCalls(OracleContext):
        def frame_launch(self, *a, **k):
            raise RuntimeError("must not be reached")

    monkeypatch.setattr(odo_mod, "IcpContext", WithFrameCalls)
    with pytest.raises(AssertionError, match="projective"):
        odo_mod.MI355XICPFrameToModel(odo_mod.MI355XICPConfig(
            one_call_frame=True, local_map=dict(type="projective_local_map", local_map_size=3)), projector=proj, device=cpu)
    odo = odo_mod.MI355XICPFrameToModel(odo_mod.MI355XICPConfig(one_call_frame=True, data_key="vertex_map"),
                                        projector=proj, device=cpu)
    odo.init()
    with pytest.raises(AssertionError, match="vertex-map tensor"):
        odo.process_next_frame({"vertex_map": torch.zeros(1, 3, 16, 256)})
    with pytest.raises(AssertionError, match="Could not find the key"):
        odo.process_next_frame({"other": None})
    # the default path is untouched by the field
    plain = odo_mod.MI355XICPFrameToModel(odo_mod.MI355XICPConfig(data_key="vertex_map"), projector=proj, device=cpu)
    assert plain._one_call is False
