"""CPU: the weight-gradient route header (gif_amd/csrc/wgrad_route.h) against its recorded table, and the library's size queries against
the numbers recorded before the header existed.

tests/host/wgrad_route_dump.cpp includes only the header.  It is built here with the compiler the library build needs (host only, C++17)
under AddressSanitizer and UBSan, run as a stand-alone program, and its output compared line by line with
tests/golden/wgrad_route_table.txt: one line per (geometry, mode, modulated, split count) with everything the launch code takes from the
route — kernel, template arguments, block size, workgroups per split, twin, workspace dims, scale-table rows, chunk, profiling family —
over a grid that puts every predicate of the header on both sides of its threshold, then per knob the cases that knob changes.
tests/golden/wgrad_splits_golden.json (tests/golden/make_wgrad_splits_golden.py) holds what gif_conv2d_wgrad_splits / _splits_f16 /
_dims / _dims_f16 and gif_conv3x3_winograd_wgrad_splits returned for the table's geometries in the three contraction modes at the commit
before the header: the library must still return them, and the table must report them."""
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
import make_wgrad_splits_golden as rec  # noqa: E402  (the geometry keys and the library queries of the recording)

MODES = ("native", "bf16x3", "f16x2")


@pytest.fixture(scope="module")
def dump_lines(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("wgrad_route") / "wgrad_route_dump")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    # (sanitizers on the host code only: each flag right after -Xarch_host)
    flags = "-x c++ -std=c++17 -O1 -g -Wall -Werror -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined"
    cmd = [hipcc] + flags.split() + ["-I", os.path.join(ROOT, "gif_amd", "csrc"), os.path.join(ROOT, "tests", "host", "wgrad_route_dump.cpp"),
                                     "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert built.returncode == 0, built.stderr[-4000:]
    ran = subprocess.run([exe], capture_output=True, text=True, timeout=300)  # (either sanitizer ends the program with an error status)
    assert ran.returncode == 0, (ran.returncode, ran.stderr[-4000:])
    return ran.stdout.splitlines()


def test_route_table_matches_the_recorded_one(dump_lines):
    with open(os.path.join(GOLDEN, "wgrad_route_table.txt")) as f:
        want = f.read().splitlines()
    for i, (a, b) in enumerate(zip(dump_lines, want)):
        assert a == b, f"line {i + 1}:\n got  {a}\n want {b}"
    assert len(dump_lines) == len(want)
    assert len(want) > 300 and sum("differ from the default" in l for l in want) == 14


def _golden():
    with open(os.path.join(GOLDEN, "wgrad_splits_golden.json")) as f:
        return json.load(f)


def test_library_size_queries_match_the_recorded_ones():
    from gif_amd import _lib
    lib = _lib.load()
    golden = _golden()
    assert list(golden) == rec.geometries(), "the recorded geometries are not the route table's"
    before = lib.gif_get_fp32_mfma_mode()
    bad = [(k, rec.query(lib, k), want) for k, want in golden.items() if rec.query(lib, k) != want]
    assert lib.gif_get_fp32_mfma_mode() == before
    assert not bad, f"{len(bad)} of {len(golden)} geometries; first: {bad[0]}"
    # degenerate arguments keep their answers
    assert lib.gif_conv2d_wgrad_splits(None) == 1 and lib.gif_conv2d_wgrad_splits_f16(None) == 1
    assert lib.gif_conv3x3_winograd_wgrad_splits(0, 8, 8, 64, 64) == 1 and lib.gif_conv3x3_winograd_wgrad_splits(1, 1, 8, 64, 64) == 1
    rp = ctypes.c_int()
    assert lib.gif_conv2d_wgrad_dims(0, 8, ctypes.byref(rp), ctypes.byref(rp)) == -1
    assert lib.gif_conv2d_wgrad_dims_f16(8, 8, None, ctypes.byref(rp)) == -1


def test_route_table_reports_the_recorded_split_counts(dump_lines):
    golden = _golden()
    line = re.compile(r"^(.*?) \| (native|bf16x3|f16x2|f16) \| [us] \| n\d+ -> .* ; RP(\d+) CP(\d+) .* splits (\d+)$")
    seen = set()
    for l in dump_lines:
        if l.startswith("GIF_"):  # (the per-knob part: knobs are not set in the recording)
            continue
        m = line.match(l)
        assert m, l
        key, mode, rp, cp, splits = m.group(1), m.group(2), int(m.group(3)), int(m.group(4)), int(m.group(5))
        want = golden[key]
        seen.add(key)
        if key.startswith("planes"):
            assert splits == want["winograd_splits"][MODES.index(mode)], l
        elif mode == "f16":
            assert [splits] * 3 == want["splits_f16"] and [rp, cp] == want["dims_f16"], l
        else:
            assert splits == want["splits"][MODES.index(mode)] and [rp, cp] == want["dims"], l
    assert seen == set(golden)
