"""CPU side of the registration and batch units of the C ABI (csrc/register.hip, batch.hip, search_stats.hip):

* csrc/register_plan.h — how many iterations the first chunk of a launched registration holds, and where the descriptor
  tables of the batched kd-tree and projective registrations lie in their slot — as a stand-alone program under
  -fsanitize=address,undefined, against the expressions the launch paths used to spell out themselves, written down here;
* the three units are built, hold host code only, and `icp_set_option` stays where tests/test_cabi.py reads it."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pylidar-slam_amd", "csrc")
UNITS = ("register.hip", "batch.hip", "search_stats.hip")


@pytest.fixture(scope="module")
def plan_program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    exe = tmp_path_factory.mktemp("plan") / "register_plan_check"
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(cxx).startswith("g++") else []
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", *static, "-I", CSRC,
                    os.path.join(ROOT, "tests", "native", "register_plan_check.cpp"), "-o", str(exe)], check=True)
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


# ---- the first chunk -----------------------------------------------------------------------------------------------------
def _first_chunk(iters, threshold, chunked, tail, last):
    """The rule as register_launch and icp_batch_register_launch each spelled it out: every iteration unless a live threshold
    meets "chunked_launch" (and no resident tail is planned); then the most any member ran last time (3 without a collected
    registration) plus one, at most all."""
    if not (threshold > 0 and chunked and not tail):
        return iters
    return min(iters, max(v if v > 0 else 3 for v in last) + 1)


def _chunk_line(iters, threshold, chunked, tail, last):
    return "C %d %r %d %d %d %s" % (iters, threshold, chunked, tail, len(last), " ".join(str(v) for v in last))


def test_first_chunk_rule_under_sanitizers(plan_program, tmp_path):
    named = [
        ((100, 0.0, 1, 0, [7]), 100),      # threshold 0: a forced count, all of them
        ((100, -1.0, 1, 0, [7]), 100),
        ((100, 1e-4, 0, 0, [7]), 100),     # "chunked_launch" 0: all
        ((100, 1e-4, 1, 0, [0]), 4),       # no history: 3 + 1
        ((5, 1e-4, 1, 0, [7]), 5),         # history 7, cap 5
        ((100, 1e-4, 1, 0, [2, 9, 0]), 10),
        ((100, 1e-4, 1, 0, [2, 0]), 4),    # (the member without history counts as 3, beside one that ran fewer)
        ((100, 1e-4, 1, 1, [7]), 100),     # a resident tail is planned: all
        ((100, 1e-4, 1, 0, [99]), 100),
        ((1, 1e-4, 1, 0, [0]), 1),
    ]
    rng = np.random.default_rng(5)
    cases = [c for c, _ in named]
    for _ in range(300):
        count = int(rng.integers(1, 33))
        cases.append((int(rng.integers(1, 120)), float(rng.choice([0.0, -1.0, 1e-4, 0.5])), int(rng.random() < 0.8),
                      int(rng.random() < 0.1), [int(v) for v in rng.integers(0, 120, count) * (rng.random(count) < 0.8)]))
    out = _run(plan_program, tmp_path, [_chunk_line(*c) for c in cases])
    for (case, want), got in zip(named, out):
        assert int(got) == want == _first_chunk(*case), (case, got, want)
    for case, got in zip(cases, out):
        assert int(got) == _first_chunk(*case), (case, got)


# ---- the slot layouts ------------------------------------------------------------------------------------------------------
def _pad(v):
    return (v + 255) // 256 * 256


SIZES = [(48, 200, 136), (40, 1, 7), (256, 512, 256), (1, 1, 1), (104, 333, 72)]
COUNTS = (1, 2, 32)


def test_batched_kd_tree_layout_under_sanitizers(plan_program, tmp_path):
    """[packs | iterate and sum + solve tables of the chunk's iterations]: the packing table is padded to 256 bytes, the tables
    behind it are `count` descriptors each, and `need` has room for a solving launch behind every iteration."""
    cases = [(p, i, s, c, k) for p, i, s in SIZES for c in COUNTS for k in (1, 4, 100)]
    out = _run(plan_program, tmp_path, ["K %d %d %d %d %d" % c for c in cases])
    for (p, i, s, c, k), line in zip(cases, out):
        first, it_bytes, ss_bytes, need = (int(v) for v in line.split())
        assert first == ((p * c + 255) // 256) * 256 and first % 256 == 0 and first >= p * c
        assert (it_bytes, ss_bytes) == (i * c, s * c)
        assert need == first + k * (i * c + s * c)


def test_batched_projective_layout_under_sanitizers(plan_program, tmp_path):
    """[packs | registrations | sum + solve | sum + solve of the last iteration], every table on a 256-byte boundary."""
    cases = [(p, r, s, c) for p, r, s in SIZES for c in COUNTS]
    out = _run(plan_program, tmp_path, ["P %d %d %d %d" % c for c in cases])
    for (p, r, s, c), line in zip(cases, out):
        regs, ss, ss_last, need = (int(v) for v in line.split())
        pack_bytes, reg_bytes, ss_bytes = _pad(p * c), _pad(r * c), _pad(s * c)
        assert (regs, ss, ss_last) == (pack_bytes, pack_bytes + reg_bytes, pack_bytes + reg_bytes + ss_bytes)
        assert all(v % 256 == 0 for v in (regs, ss, ss_last, need))
        assert need == pack_bytes + reg_bytes + 2 * ss_bytes


# ---- the units, as text -----------------------------------------------------------------------------------------------------
def test_units_are_built_and_hold_host_code_only():
    make = open(os.path.join(CSRC, "Makefile")).read()
    srcs = next(line for line in make.splitlines() if line.startswith("SRCS")).split()
    for unit in UNITS:
        assert unit in srcs, f"{unit} is not in SRCS"
        text = open(os.path.join(CSRC, unit)).read()
        for word in ("__global__", "<<<", "hipLaunchKernelGGL"):
            assert word not in text, f"{unit} holds {word}: kernels and their launches live in the kernel-bearing units"
    assert "register_plan.h" in make
    api = open(os.path.join(CSRC, "api.hip")).read()
    assert "\nint icp_set_option(" in api and api.index("\nint icp_set_option(") < api.index("\nint icp_set_cost(")
    for text, unit in ((open(os.path.join(CSRC, u)).read(), u) for u in ("register.hip", "batch.hip")):
        assert "first_chunk_iterations(" in text and '#include "register_plan.h"' in text, unit
