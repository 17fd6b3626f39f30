"""CPU: the Winograd forward / data-gradient route header (gif_amd/csrc/wino_route.h) against its recorded table, and the library's size
queries against the numbers recorded before the header existed.

tests/host/wino_route_dump.cpp includes only the header.  It is built here with the compiler the library build needs (host only, C++17)
under AddressSanitizer and UBSan, run as a stand-alone program, and its output compared line by line with
tests/golden/wino_route_table.txt: one line per (geometry, mode, guarded) with everything the launch code takes from the route — the
input transform's kernel, lanes and workgroups, the GEMM's kernel, template arguments, tiles, grid, block size and LDS bytes, the twin,
padded dims, sizes, partial-sum rows, profiling family, or the 32-bit limit the call fails — over a grid that puts every predicate of the
header on both sides of its threshold, then per knob value (as the raw environment string) the cases that value changes.
tests/golden/wino_queries_golden.json (tests/golden/make_wino_queries_golden.py) holds what gif_winograd_pack_dims / _pack_dims_x3 /
_workspace_floats / _weight_f32h2_bytes returned for the table's geometries at the commit before the header: the library must still
return them, and the table must report them."""
import ctypes
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GOLDEN)
import make_wino_queries_golden as rec  # noqa: E402  (the geometry keys and the library queries of the recording)


@pytest.fixture(scope="module")
def dump_lines(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("wino_route") / "wino_route_dump")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    # (sanitizers on the host code only: each flag right after -Xarch_host)
    flags = "-x c++ -std=c++17 -O1 -g -Wall -Werror -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined"
    cmd = [hipcc] + flags.split() + ["-I", os.path.join(ROOT, "gif_amd", "csrc"), os.path.join(ROOT, "tests", "host", "wino_route_dump.cpp"),
                                     "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert built.returncode == 0, built.stderr[-4000:]
    ran = subprocess.run([exe], capture_output=True, text=True, timeout=300)  # (either sanitizer ends the program with an error status)
    assert ran.returncode == 0, (ran.returncode, ran.stderr[-4000:])
    return ran.stdout.splitlines()


def test_route_table_matches_the_recorded_one(dump_lines):
    with open(os.path.join(GOLDEN, "wino_route_table.txt")) as f:
        want = f.read().splitlines()
    for i, (a, b) in enumerate(zip(dump_lines, want)):
        assert a == b, f"line {i + 1}:\n got  {a}\n want {b}"
    assert len(dump_lines) == len(want)
    assert len(want) > 300 and sum("differ from the default" in l for l in want) == 15
    # every kernel of the launch ladder, every transform and every limit is named somewhere in the table
    text = "\n".join(want)
    for name in ("mfma<2>", "mfma<4>", "x3<128,128>", "x3<256,64>", "h2<128,128,3>", "h2<128,128,4>", "h2<128,128,5>", "rows<4>", "rows<8>",
                 "rows<16>", "-> tile ", "-> gy ", "error V", "error y", "error x", "error U"):
        assert name in text, name


def _golden():
    with open(os.path.join(GOLDEN, "wino_queries_golden.json")) as f:
        return json.load(f)


def test_library_size_queries_match_the_recorded_ones():
    from gif_amd import _lib
    lib = _lib.load()
    golden = _golden()
    assert list(golden) == rec.geometries(), "the recorded geometries are not the route table's"
    bad = [(k, rec.query(lib, k), want) for k, want in golden.items() if rec.query(lib, k) != want]
    assert not bad, f"{len(bad)} of {len(golden)} geometries; first: {bad[0]}"
    # degenerate arguments keep their answers
    rp = ctypes.c_int()
    assert lib.gif_winograd_pack_dims(0, 8, ctypes.byref(rp), ctypes.byref(rp)) == -1
    assert lib.gif_winograd_pack_dims_x3(8, 8, None, ctypes.byref(rp)) == -1
    assert lib.gif_winograd_workspace_floats(0, 8, 8, 64) == 0 and lib.gif_winograd_workspace_floats(1, 8, 8, 0) == 0
    assert lib.gif_winograd_workspace_floats(1, 1, 8, 64) == 0  # (no 2x2 tile)
    assert lib.gif_winograd_weight_f32h2_bytes(0, 32) == 0 and lib.gif_winograd_weight_f32h2_bytes(128, 0) == 0


def test_route_table_reports_the_recorded_sizes(dump_lines):
    golden = _golden()
    line = re.compile(r"^(.*?) \| (native|bf16x3|f16x2) \| [ug] -> .* ; ntiles\d+ pad\d+ RP(\d+) CP(\d+) vfloats(\d+) u2bytes(\d+)( sums\d+x\d+ fam\d+)?$")
    seen = set()
    for l in dump_lines:
        if l.startswith("GIF_") or l.startswith("gy "):  # (knobs are not set in the recording; gy lines carry no size of their own)
            continue
        m = line.match(l)
        assert m, l
        key, mode = m.group(1), m.group(2)
        rp, cp, vfloats, u2bytes = (int(v) for v in m.groups()[2:6])
        want = golden[key]
        seen.add(key)
        assert vfloats == want["workspace_floats"], l
        if mode == "native":
            assert [rp, cp] == want["pack_dims"] and u2bytes == 0, l
        else:
            assert [rp, cp] == want["pack_dims_x3"] and u2bytes == want["weight_f32h2_bytes"], l
    assert seen == set(golden)
