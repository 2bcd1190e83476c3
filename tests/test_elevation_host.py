"""CPU side of the elevation image (icp_elevation_*, include/icp_mi355x.h):

* every call is declared with the signature written down here, cites the reference lines it stands for, is exported, bound,
  and reachable as `IcpContext.elevation_image` / `ElevationImage` / `AggregatedMap.elevation` / `register.install_elevation_image`;
* the kernel unit and its headers are part of the build;
* what needs no device (csrc/elevation_plan.h: every refusal, the grids, the footprint — and the arithmetic of one row and one
  pixel that the kernels call: cell, clip, z-buffer word, theta, colour row) as a stand-alone program under
  -fsanitize=address,undefined, against the rules written down here and the numpy model (tests/elevation_audit.py)."""
import ctypes
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import elevation_audit as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "icp_mi355x.h")
CSRC = os.path.join(ROOT, "pylidar-slam_amd", "csrc")
MAX_INDEX = 2 ** 31 - 1

SIGNATURES = {
    "icp_elevation_create": ("int", ["icp_ctx* ctx", "int64_t height", "int64_t width", "double pixel_size", "double z_min", "double z_max",
                                     "int flip", "const uint8_t* lut", "int64_t max_rows", "icp_elevation** out"]),
    "icp_elevation_destroy": ("void", ["icp_elevation* img"]),
    "icp_elevation_build": ("int", ["icp_elevation* img", "const void* xyz", "int64_t n", "int mem", "int dtype"]),
    "icp_elevation_build_aggmap": ("int", ["icp_elevation* img", "icp_aggmap* map", "int32_t frame_lo", "int32_t frame_hi",
                                           "const double pose[16]"]),
    "icp_elevation_get": ("int", ["icp_elevation* img", "uint8_t* rgb_out", "float* theta_out", "float* points_out", "int32_t* index_out",
                                  "int out_mem"]),
    "icp_elevation_stats": ("int", ["icp_elevation* img", "icp_elevation_counters* out"]),
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
        assert "slam/common/registration.py:196-241" in comment, name  # the comment right in front of the declaration
        assert hasattr(lib, name), f"{name} is not exported"
        restype, argtypes = _lib.EXPORTED_SYMBOLS[name]
        assert len(argtypes) == len(want) and restype is (None if ret == "void" else ctypes.c_int), name
    assert sorted(n for n in _lib.EXPORTED_SYMBOLS if n.startswith("icp_elevation_")) == sorted(SIGNATURES)
    assert ctypes.sizeof(_lib.IcpElevationCounters) == 4 * 8
    fields = re.search(r"typedef struct \{([^}]*)\} icp_elevation_counters;", text).group(1)
    assert re.findall(r"int64_t (\w+);", fields) == [f for f, _ in _lib.IcpElevationCounters._fields_] == \
        ["rows_in_image", "rows_outside", "rows_nan_z", "filled_pixels"]
    assert re.search(r"ICP_ELEVATION_F32 = 0, ICP_ELEVATION_F64 = 1", text) and (_lib.ELEVATION_F32, _lib.ELEVATION_F64) == (0, 1)
    section = doc[doc.index("---- elevation image"):doc.index("typedef struct icp_elevation icp_elevation;")]
    assert "slam/loop_closure.py:294" in section and "slam/initialization.py:176" in section and "deviation" in section
    assert callable(engine.IcpContext.elevation_image) and callable(engine.AggregatedMap.elevation) and callable(engine.colormap_table)
    for method in ("build", "build_from", "stats", "build_image", "device", "close"):
        assert callable(getattr(engine.ElevationImage, method)), method
    for prop in ("rgb", "theta", "points_3d", "indices"):
        assert isinstance(getattr(engine.ElevationImage, prop), property), prop
    assert callable(register.install_elevation_image)


def test_kernel_unit_is_built_and_keeps_to_vector_stores_and_plain_cpp():
    make = open(os.path.join(CSRC, "Makefile")).read()
    srcs = re.search(r"^SRCS\s*:=\s*(.*)$", make, flags=re.M).group(1).split()
    assert "elevation.hip" in srcs and "aggmap.hip" in srcs
    rule = re.search(r"^\$\(OBJDIR\)/%\.o:(.*)$", make, flags=re.M).group(1).split()
    assert "elevation_plan.h" in rule and "aggmap_device.h" in rule and "aggmap_plan.h" in rule
    unit = open(os.path.join(CSRC, "elevation.hip")).read()
    agg = open(os.path.join(CSRC, "aggmap.hip")).read()
    shared = open(os.path.join(CSRC, "aggmap_device.h")).read()
    assert '#include "elevation_plan.h"' in unit and '#include "aggmap_device.h"' in unit and '#include "aggmap_device.h"' in agg
    # the window is moved by the one agg_world the submap uses
    assert len(re.findall(r"double agg_world\(", shared)) == 1 and "double agg_world(" not in agg and "double agg_world(" not in unit
    assert "agg_world(pose, 0" in unit
    plan = open(os.path.join(CSRC, "elevation_plan.h")).read()
    assert "hip/" not in plan and "__global__" not in plan  # free of HIP: it builds with the host compiler alone
    assert "asm" not in unit and "__builtin_amdgcn" not in unit
    assert not re.search(r"while\s*\(|for\s*\(\s*;\s*;\s*\)", unit)  # no loop without its bound in its head


def test_colormap_table_is_matplotlibs_lookup_table():
    matplotlib = pytest.importorskip("matplotlib")
    from pylidar_slam_amd.engine import colormap_table
    for name in ("jet", "viridis"):
        cmap = matplotlib.colormaps[name]
        table = colormap_table(name)
        assert table.dtype == np.uint8 and table.shape == (259, 3)
        cmap(0.5)  # (fills the private table)
        assert np.array_equal(table, (cmap._lut[:, :3] * 255.0).astype(np.uint8))
    assert np.array_equal(colormap_table(matplotlib.colormaps["jet"]), colormap_table("jet"))
    with pytest.raises(AssertionError, match="256 colours"):
        colormap_table(matplotlib.colormaps["tab10"])


# ---- the plan header under the host sanitizers ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plan_program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no C++ compiler"
    exe = tmp_path_factory.mktemp("elevation_plan") / "elevation_plan_check"
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(cxx).startswith("g++") else []
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-ffp-contract=off", *static, "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "native", "elevation_plan_check.cpp"), "-o", str(exe)], check=True)
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


def _create_model(h, w, pixel, lo, hi, table, rows):
    if not (pixel > 0) or not np.isfinite(pixel):
        return "pixel size"
    if not (np.isfinite(lo) and np.isfinite(hi)):
        return "not finite"
    if not lo < hi:
        return "is not below"
    with np.errstate(over="ignore"):
        if not np.isfinite(hi - lo) or not np.float32(lo) < np.float32(hi) or not np.isfinite(np.float32(lo)) or not np.isfinite(np.float32(hi)):
            return "float32"
    if h < 1 or w < 1:
        return "below 1"
    if h * w > MAX_INDEX:
        return "pixels"
    if rows < 1:
        return "max_rows"
    if rows > MAX_INDEX:
        return "max_rows exceeds"
    if not table:
        return "colour table"
    return None


def _build_model(n, rows, mem, dtype):
    if n < 0:
        return "negative"
    if n > MAX_INDEX:
        return "int32"
    if n > rows:
        return "exceeds max_rows"
    if mem not in (0, 1):
        return "host or device memory"
    if dtype not in (0, 1):
        return "float32 or float64"
    return None


def _window_model(same, lo, hi, kind, which, value):
    if same != 1:
        return "another context"
    if lo > hi:
        return "frame_lo"
    if not (kind == 1 or (kind == 2 and (not 0 <= which < 16 or np.isfinite(value)))):
        return "non-finite"
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
    ok = (400, 400, 0.4, 0.0, 5.0, 1, 262144)
    create = [ok, (1, 1, 5e-324, -1e300, 1e30, 1, 1), (46340, 46340, 0.4, 0.0, 5.0, 1, MAX_INDEX), (MAX_INDEX, 1, 0.4, 0.0, 5.0, 1, 1),
              (1, MAX_INDEX, 0.4, 0.0, 5.0, 1, 1)]
    for pixel in (0.0, -0.0, -0.4, inf, -inf, nan):
        create.append((400, 400, pixel, 0.0, 5.0, 1, 262144))
    for lo, hi in ((5.0, 5.0), (5.0, 0.0), (nan, 5.0), (0.0, nan), (-inf, 5.0), (0.0, inf), (1.0, 1.0 + 1e-12), (-1e308, 1e308),
                   (1e39, 1e40), (-0.0, 0.0)):
        create.append((400, 400, 0.4, lo, hi, 1, 262144))
    for h, w in ((0, 400), (400, 0), (-1, -1), (46341, 46341), (65536, 32768), (MAX_INDEX, 2), (2 ** 40, 2 ** 40), (2 ** 62, 4), (2 ** 63 - 1, 2 ** 63 - 1)):
        create.append((h, w, 0.4, 0.0, 5.0, 1, 262144))
    for rows in (0, -1, MAX_INDEX + 1, 2 ** 62):
        create.append((400, 400, 0.4, 0.0, 5.0, 1, rows))
    create += [(400, 400, 0.4, 0.0, 5.0, 0, 262144), (0, 0, nan, nan, nan, 0, 0)]
    out = _run(plan_program, tmp_path, [f"C {h} {w} {_bits(p)} {_bits(lo)} {_bits(hi)} {t} {r}" for h, w, p, lo, hi, t, r in create])
    _check(out, [_create_model(*c) for c in create], "icp_elevation_create: ", create)
    build = [(0, 64, 0, 0), (64, 64, 1, 1), (65, 64, 0, 0), (-1, 64, 0, 0), (-2 ** 40, 64, 0, 0), (2 ** 40, 2 ** 41, 0, 0), (MAX_INDEX, MAX_INDEX, 1, 1),
             (MAX_INDEX + 1, 2 ** 40, 0, 0), (5, 64, 2, 0), (5, 64, -1, 1), (5, 64, 0, 2), (5, 64, 1, -1), (65, 64, 7, 7), (-1, 64, 7, 7)]
    out = _run(plan_program, tmp_path, [f"B {n} {r} {mem} {dt}" for n, r, mem, dt in build])
    _check(out, [_build_model(*c) for c in build], "icp_elevation_build: ", build)
    window = [(1, 0, 0, 1, 0, 0.0), (1, -5, 7, 1, 0, 0.0), (0, 0, 1, 1, 0, 0.0), (2, 0, 1, 1, 0, 0.0), (1, 3, 2, 1, 0, 0.0),
              (1, 2 ** 31 - 1, -2 ** 31, 1, 0, 0.0), (1, -2 ** 31, 2 ** 31 - 1, 1, 0, 0.0), (1, 0, 1, 0, 0, 0.0), (0, 3, 2, 0, 0, 0.0)]
    window += [(1, 0, 1, 2, k, v) for k in range(16) for v in (nan, inf, -inf, 1.0e308, -0.0)]
    out = _run(plan_program, tmp_path, [f"W {s} {lo} {hi} {k} {w} {_bits(v)}" for s, lo, hi, k, w, v in window])
    _check(out, [_window_model(*c) for c in window], "icp_elevation_build_aggmap: ", window)
    out = _run(plan_program, tmp_path, ["G 0", "G 1", "G 2", "G -1"])
    assert out[0] == out[1] == "ok" and all(o.startswith("refused -1 icp_elevation_get: host or device memory") for o in out[2:])


def test_grids_and_footprint_under_sanitizers(plan_program, tmp_path):
    cases = [(400, 400, 262144, 0, 131072, 2000000), (400, 400, 262144, 1, 0, 1), (1, 1, 1, 0, 1, 255), (5, 7, 64, 1, 255, 256), (255, 1, 64, 0, 256, 257),
             (1, 300, 64, 0, 257, 1048576), (46340, 46340, MAX_INDEX, 1, MAX_INDEX, 2 ** 30), (1, 1, 1, 0, -5, 1048577), (0, 5, 5, 0, 65537, 4096 * 256 - 1),
             (65536, 32768, 5, 0, 1, 1), (5, 5, 0, 0, 1, 1), (2 ** 62, 4, 5, 0, 1, 1)]
    out = _run(plan_program, tmp_path, [f"T {h} {w} {r} {host} {n} {cap}" for h, w, r, host, n, cap in cases])
    for line, (h, w, r, host, n, cap) in zip(out, cases):
        foot, blocks, window = (int(v) for v in line.split())
        valid = h >= 1 and w >= 1 and h * w <= MAX_INDEX and 1 <= r <= MAX_INDEX
        assert foot == (h * w * 35 + 259 * 3 + 64 * 128 + (r * 24 if host else 0) if valid else 0), (h, w, r, host)
        assert blocks == (0 if n < 1 else -(-n // 256)) and blocks * 256 >= n, n
        assert window == min(-(-cap // 256), 4096) and window >= 1, cap


def test_cells_against_the_model_under_sanitizers(plan_program, tmp_path):
    """the kernels' own cell function on every pixel boundary and 1, 2, 3 ulp either side, both types, odd and even extents, and
    on the values no image holds"""
    lines, want = [], []
    for dtype, tag, bits in ((np.float32, "f", _bits32), (np.float64, "d", _bits)):
        for spec in (A.Spec(5, 7, 0.4), A.Spec(6, 300, 0.5), A.Spec(400, 401, 0.4)):
            cloud = A.boundary_cloud(spec, dtype)
            special = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, -0.0, 0.0, 3e9 * spec.pixel_size, 1e19], dtype)
            for axis, extent in ((0, spec.height), (1, spec.width)):
                v = np.concatenate([cloud[:, axis], special])
                cells = A._cells(v, spec.pixel_size, extent // 2, np.dtype(dtype).type, None).astype(np.float64)
                with np.errstate(invalid="ignore"):
                    inside = (cells >= 0) & (cells < extent)
                for value, cell, ok in zip(v, cells, inside):
                    lines.append(f"X {tag} {bits(value)} {bits(np.dtype(dtype).type(spec.pixel_size))} {extent // 2} {extent}")
                    want.append(f"1 {int(cell)}" if ok else "0 -1")
    out = _run(plan_program, tmp_path, lines)
    assert len(lines) > 4000 and sum(w != "0 -1" for w in want) > 2000 and sum(w == "0 -1" for w in want) > 100
    assert out == want, [(a, b, c) for a, b, c in zip(lines, out, want) if b != c][:5]
    big = _run(plan_program, tmp_path, [f"X d {_bits(2.0 ** 31 - 1.0)} {_bits(1.0)} 0 {MAX_INDEX}", f"X d {_bits(2.0 ** 31 - 2.0)} {_bits(1.0)} 0 {MAX_INDEX}",
                                       f"X f {_bits32(2.0 ** 31)} {_bits32(1.0)} 0 {MAX_INDEX}"])
    assert big == ["0 -1", f"1 {MAX_INDEX - 1}", "0 -1"]


def test_clip_word_theta_and_colour_row_against_the_model_under_sanitizers(plan_program, tmp_path):
    rng = np.random.default_rng(3)
    lines, want, words = [], [], {}
    for dtype, tag, bits in ((np.float32, "f", _bits32), (np.float64, "d", _bits)):
        dt = np.dtype(dtype).type
        for z_min, z_max in ((0.0, 5.0), (-2.0, 5.0), (0.5, 5.0), (-3.0, -1.0)):
            lo, hi, den = dt(z_min), dt(z_max), dt(np.float64(z_max) - np.float64(z_min))
            z = np.concatenate([rng.uniform(z_min - 1, z_max + 1, 300).astype(dtype),
                                np.array([lo, hi, np.nextafter(lo, dt(np.inf)), np.nextafter(lo, dt(-np.inf)), np.nextafter(hi, dt(np.inf)),
                                          np.nextafter(hi, dt(-np.inf)), np.inf, -np.inf, 0.0, -0.0, 1e30, -1e30], dtype)])
            zc = np.clip(z, lo, hi) + dt(0)
            theta = ((zc - lo) / den).astype(np.float32)
            rows = A.colour_rows(theta)
            for flip in (0, 1):
                for k, (a, c, t, r) in enumerate(zip(z, zc, theta, rows)):
                    lines.append(f"Z {tag} {bits(a)} {bits(lo)} {bits(hi)} {bits(den)} {flip} {k}")
                    want.append((bits(c).lstrip("0") or "0", _bits32(t).lstrip("0") or "0", int(r)))
                    words[len(lines) - 1] = (tag, flip, float(c), k, z_min)
    out = _run(plan_program, tmp_path, lines)
    got = [o.split() for o in out]
    assert [(g[0], g[2], int(g[3])) for g in got] == want
    # the z-buffer word orders like (clipped z, row) — flipped: like (-clipped z, row) —, equal zeros give equal words, none is 0
    for tag in ("f", "d"):
        for flip in (0, 1):
            for z_min in (0.0, -2.0, 0.5, -3.0):
                mine = [(int(got[i][1], 16), c, k) for i, (t, f, c, k, zm) in words.items() if (t, f, zm) == (tag, flip, z_min)]
                assert all(w > 0 for w, _, _ in mine)
                by_word = sorted(mine)
                keyed = sorted(mine, key=lambda m: ((-m[1] if flip else m[1]), m[2])) if tag == "f" else sorted(mine, key=lambda m: (-m[1] if flip else m[1]))
                assert [m[1] for m in by_word] == [m[1] for m in keyed]
                if tag == "f":
                    assert [m[2] for m in by_word] == [m[2] for m in keyed] and all(w & 0xffffffff == k for w, _, k in mine)
                else:
                    zero = {w for w, c, _ in mine if c == 0.0}
                    assert len(zero) <= 1


def test_colour_rows_of_every_kind_of_theta_under_sanitizers(plan_program, tmp_path):
    """under, over, bad, 256 -> 255, truncation, the two zeros, the subnormals, overflow of theta * 256 — and every row of the
    table from a theta of its own"""
    one = np.float32(1)
    theta = np.array([0.0, -0.0, 1.0, np.nextafter(one, np.float32(0)), np.nextafter(one, np.float32(2)), 0.5, 0.998046875, 0.99609375,
                      255.5 / 256, 1e-45, -1e-45, -0.5, -2.0, 2.0, 1e38, 3e38, np.inf, -np.inf, np.nan, 0.00390625, 0.003906249], np.float32)
    theta = np.concatenate([theta, (np.arange(256, dtype=np.float32) + np.float32(0.5)) / np.float32(256)])
    out = _run(plan_program, tmp_path, [f"K {_bits32(t)}" for t in theta])
    want = A.colour_rows(theta)
    assert [int(o) for o in out] == [int(w) for w in want]
    assert set(range(259)) == set(int(w) for w in want) and int(want[2]) == 255 and int(want[0]) == int(want[1]) == 0
