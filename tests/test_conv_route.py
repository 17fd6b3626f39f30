"""CPU: the forward / data-gradient route header (gif_amd/csrc/conv_route.h) against its recorded table, the tile, split and merge claims
of tests/test_gpu_conv_routes.ROWS against that table, and the library's packing / eligibility queries against the answers recorded before
the header existed.

tests/host/conv_route_dump.cpp includes only the header.  It is built here with the compiler the library build needs (host only, C++17)
under AddressSanitizer and UBSan, run as a stand-alone program, and its output compared line by line with
tests/golden/conv_route_table.txt: one line per case with everything the launch code takes from the route — per launch the kernel, its
template arguments, row range, phases, tiles, grid, block size, dynamic LDS bytes, scale-table geometry and partial-sum rows; per op the
packing, profiling family, zero fill, merged flag, partial rows x tile rows and the guarded twin's route — first for the library calls
gif_amd/ops.py makes for the fwd / dgrad rows of ROWS (tests/golden/conv_route_cases.txt, written by make_conv_route_cases.py), then over
a grid that puts every predicate of the header on both sides of its threshold, then per knob the cases that knob changes.
CLAIMS restates, as data, what the comments of ROWS say about tile, launches, bulk rows and merged phases; the table must say the same.
tests/golden/conv_queries_golden.json (make_conv_queries_golden.py) holds what gif_conv2d_pack_dims / _x3 / _f16, gif_conv2d_x3_eligible
and gif_conv2d_f16_halo_eligible returned for the table's geometries at the commit before the header: the library must still return
them, and the table's RP / CP / halo columns must agree.
tests/golden/conv_plan_table.txt (make_conv_plan_golden.py) holds what gif_amd/ops.py decided before it called the library (Winograd or
direct route, contraction mode, tap-dense K order) at the commit before ops.conv_plan existed, over a grid that puts every rule and
knob of that decision on both sides: conv_plan must still decide the same."""
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GOLDEN)
import make_conv_queries_golden as rec  # noqa: E402  (the geometry keys and the library queries of the recording)
import make_conv_plan_golden as plans  # noqa: E402
import make_conv_route_cases as cases  # noqa: E402


@pytest.fixture(scope="module")
def dump_lines(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("conv_route") / "conv_route_dump")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    # (sanitizers on the host code only: each flag right after -Xarch_host)
    flags = "-x c++ -std=c++17 -O1 -g -Wall -Werror -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined"
    cmd = [hipcc] + flags.split() + ["-I", os.path.join(ROOT, "gif_amd", "csrc"), os.path.join(ROOT, "tests", "host", "conv_route_dump.cpp"),
                                     "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert built.returncode == 0, built.stderr[-4000:]
    ran = subprocess.run([exe, os.path.join(GOLDEN, "conv_route_cases.txt")], capture_output=True, text=True, timeout=300)
    assert ran.returncode == 0, (ran.returncode, ran.stderr[-4000:])  # (either sanitizer ends the program with an error status)
    return ran.stdout.splitlines()


def test_route_table_matches_the_recorded_one(dump_lines):
    with open(os.path.join(GOLDEN, "conv_route_table.txt")) as f:
        want = f.read().splitlines()
    for i, (a, b) in enumerate(zip(dump_lines, want)):
        assert a == b, f"line {i + 1}:\n got  {a}\n want {b}"
    assert len(dump_lines) == len(want)
    assert 300 < len(want) < 500 and sum("differ from the default" in l for l in want) == 11


def test_case_file_is_current():
    with open(os.path.join(GOLDEN, "conv_route_cases.txt")) as f:
        assert f.read().splitlines() == cases.case_lines(), "run tests/golden/make_conv_route_cases.py"


def test_conv_plan_decides_what_the_recorded_table_says():
    with open(os.path.join(GOLDEN, "conv_plan_table.txt")) as f:
        want = f.read().splitlines()
    got = plans.table_lines()
    for i, (a, b) in enumerate(zip(got, want)):
        assert a == b, f"line {i + 1}:\n got  {a}\n want {b}"
    assert len(got) == len(want) > 1000
    # both sides of every answer are in the table, for each op
    for op in ("fwd", "dgrad", "wgrad"):
        ends = {l.split(" -> ")[1] for l in want if " -> " in l and l.split()[1] == op}
        assert {"winograd native 0", "winograd bf16x3 0", "winograd f16x2 0", "direct native 0", "direct bf16x3 0", "direct f16x2 0", "direct f16 0"} <= ends, (op, ends)
        assert (op == "wgrad") != ({"direct bf16x3 1", "direct f16x2 1"} <= ends), (op, ends)


# ---- the claims of the ROWS comments ---------------------------------------------------------------------------------------------
def parse(line):
    """One default-knob table line -> dict(name, mode, zero, merged, launches=[(kernel, tile, m_begin, M)], halo)."""
    head, rest = line.split(" -> ", 1)
    name, op, mode = head.split(" | ")[:3]
    main = rest.split(" + twin ")[0]
    out = {"name": name, "op": op, "mode": mode, "zero": " zero1" in main, "error": " error " in main, "launches": [],
           "halo": {" halo1": True, " halo0": False}.get(main[main.index(" zero") + 6:][:6]), "dot": " t1 |" in head, "merged": " merged1" in main}
    if not out["error"]:
        body = main.split(" :", 1)[1].strip()
        for text in (body.split(" ; ") if body else []):
            tile, mm = re.search(r" (\d+x\d+)x\d+ w", text), re.search(r" m\[(\d+),(\d+)\)", text)
            out["launches"].append((text.split()[0], tile.group(1) if tile else None, int(mm.group(1)) if mm else 0, int(mm.group(2)) if mm else None))
    return out


def one(kernel, tile=None):
    return dict(kernel=kernel, tile=tile, n=1, bulk=None, merged=False)


def split(tile, bulk):
    return dict(kernel="glds", tile=tile, n=2, bulk=bulk, merged=False)


def merged(tile):
    return dict(kernel="multi", tile=tile, n=1, bulk=None, merged=True)


def phases(n=None):
    """one launch (or bulk + remainder) per phase; n: their number where the comment gives it"""
    return dict(kernel=None, tile=None, n=n, bulk=None, merged=False)


S, N, F = ("f16x2", "bf16x3"), ("native",), ("f16",)
A = S + N
# row -> [(modes, claim)]: the tile of the first launch, the number of launches, the rows of a bulk launch (its 64x64 remainder launch
# starts there) and the merged flag, as the row's comment in test_gpu_conv_routes.py states them
CLAIMS = {
    "t128_383": [(S, one("glds", "128x64")), (N, one("glds", "64x64"))],
    "t128_384": [(A, one("glds", "128x128"))],
    "t128_383_dgrad": [(S, one("glds", "128x64")), (N, one("glds", "64x64"))],
    "t128_384_dgrad": [(A, one("glds", "128x128"))],
    "t64_127": [(A, one("glds", "64x64"))],
    "t64_128": [(S, one("glds", "128x64")), (N, one("glds", "64x64"))],
    "t256_511": [(A, one("glds", "128x128"))],
    "t256_512": [(S, one("glds", "256x128")), (N, one("glds", "128x128"))],
    "split_rem128": [(S, split("256x128", 131072)), (N, split("128x128", 131072))],
    "split_rem129": [(S, one("glds", "256x128")), (N, one("glds", "128x128"))],
    "split_rem128_dgrad": [(S, split("256x128", 131072)), (N, split("128x128", 131072))],
    "split_tn2": [(S, split("256x128", 65536)), (N, split("128x128", 65536))],
    "split_tn3": [(S, one("glds", "256x128")), (N, one("glds", "128x128"))],
    "thin_w32": [(("f16x2",), one("rows_thin")), (("bf16x3",) + N, one("glds", "256x32"))],
    "thin_w64": [(("f16x2",), one("rows_thin")), (("bf16x3",) + N, one("glds", "256x32"))],
    "thin_w256": [(("f16x2",), one("rows_thin")), (("bf16x3",) + N, one("glds", "256x32"))],
    "thin_w512": [(("f16x2",), one("rows_thin")), (("bf16x3",) + N, one("glds", "256x32"))],
    "thin_w48": [(A, one("glds", "256x32"))],
    "thin_w16": [(A, one("glds", "256x32"))],
    "thin_m320": [(A, one("glds", "256x32"))],
    "thin_dgrad_w64": [(("f16x2",), one("rows_thin")), (("bf16x3",) + N, one("glds", "256x32"))],
    "tconv_small_all": [(A, merged("64x64"))],
    "tconv_not_small": [(A, phases(4))],
    "tconv_big_all": [(S, merged("256x128")), (N, phases())],
    "tconv_not_big": [(A, phases())],
    "halo_16": [(F, one("halo"))],
    "halo_15": [(F, one("glds", "128x64"))],
    "halo_c40_o32": [(F, one("halo"))],
    "halo_c40_o40": [(F, one("glds", "128x64"))],
    "halo_o72": [(F, one("glds", "64x64"))],
    "halo_s2": [(F, one("glds", "256x32"))],
    "halo_dot_h24": [(F, one("glds", "256x32"))],
    "halo_dot_512": [(F, one("halo"))],
    "halo_dot_496": [(F, one("halo"))],
    "f16_t256_512": [(F, one("glds", "256x256"))],
    "f16_t256_511": [(F, one("glds", "128x128"))],
    "f16_t128_383": [(F, one("glds", "64x64"))],
    "f16_t128_384": [(F, one("glds", "128x128"))],
    "f16_tconv_small": [(F, merged("64x64"))],
    "f16_tconv_not_small": [(F, phases(4))],
    # the tap-dense rows (and their native register-staged counterparts): 2640 / 2046 / 1073 / 264 rows are far below 384 tiles of 128, so the
    # 128-wide ones run 64x64 tiles (wino_cin28, 32768 rows: 128x64) and the <= 32-channel ones 256x32 — never the 8-wave 256x128 tile
    "dense_c12": [(S, one("glds", "256x32")), (N, one("simple", "256x32"))],
    "dense_c24_o36": [(S, one("glds", "64x64")), (N, one("simple", "128x128"))],
    "dense_c9_o17": [(S, one("glds", "256x32")), (N, one("simple", "256x32"))],
    "dense_c28_o33": [(S, one("glds", "64x64")), (N, one("simple", "128x128"))],
    "dense_dgrad": [(S, one("glds", "64x64")), (N, one("simple", "128x128"))],
    "wino_cin28": [(S, one("glds", "128x64")), (N, one("simple", "128x128"))],
    "c17_o33_s2": [(S, one("glds", "64x64")), (N, one("simple", "128x128"))],
    "c33_o9_dgrad_1x1_s2": [(A, dict(kernel="glds", tile="256x32", n=1, bulk=None, merged=False, zero=True))],
}
DENSE_ROWS = ("dense_c12", "dense_c24_o36", "dense_c9_o17", "dense_c28_o33", "dense_dgrad", "wino_cin28", "c17_o33_s2")


def test_table_holds_the_claims_of_the_route_rows(dump_lines):
    import test_gpu_conv_routes as routes
    table = {}
    for l in dump_lines:
        if not l.startswith(("g_", "GIF_")):
            table[l.split(" | ")[0]] = parse(l)
    prefixes = ("t128_", "t64_", "t256_", "split_", "thin_", "tconv_", "f16_t", "f16_tconv_", "halo_")
    for row in routes.ROWS:
        if row.name.startswith(prefixes):
            assert row.name in CLAIMS, f"{row.name}: the row's tile / split / merge claim is not restated in CLAIMS"
    checked = 0
    for name, claims in CLAIMS.items():
        row = next(r for r in routes.ROWS if r.name == name)
        assert sorted(m for modes, _ in claims for m in modes) == sorted(row.fams), f"{name}: a claim for every mode the row runs in"
        for modes, c in claims:
            for mode in modes:
                t = table[f"{name}-{mode}"]
                what = f"{name}-{mode}: {t}"
                assert not t["error"] and t["merged"] == c["merged"] and t["zero"] == c.get("zero", False), what
                assert len(t["launches"]) == c["n"] if c["n"] else len(t["launches"]) >= 4, what
                kernel, tile, m_begin, M = t["launches"][0]
                if c["kernel"]:
                    assert kernel == c["kernel"] and tile == c["tile"] and m_begin == 0, what
                if c["bulk"]:
                    assert M == c["bulk"] and t["launches"][1][:3] == ("glds", "64x64", c["bulk"]), what
                checked += 1
    # the dense rows of CLAIMS are calls of the tap-dense entry points; where a plain layer runs 256x128 tiles (the grid's g_dense_big,
    # 65536 rows x 256 channels) a tap-dense one runs 128x128
    for name in DENSE_ROWS:
        for mode in S:
            assert " d1 " in next(l for l in dump_lines if l.startswith(f"{name}-{mode} |")), name
    big = [parse(l) for l in dump_lines if l.startswith("g_dense_big |")]
    assert len(big) == 2 and all(t["launches"][0][:2] == ("glds", "128x128") and len(t["launches"]) == 1 for t in big), big
    assert checked >= 110


# ---- the library's queries -------------------------------------------------------------------------------------------------------
def _golden():
    with open(os.path.join(GOLDEN, "conv_queries_golden.json")) as f:
        return json.load(f)


def test_library_queries_match_the_recorded_ones():
    from gif_amd import _lib
    lib = _lib.load()
    golden = _golden()
    assert list(golden) == rec.geometries(), "the recorded geometries are not the route table's"
    bad = [(k, rec.query(lib, k), want) for k, want in golden.items() if rec.query(lib, k) != want]
    assert not bad, f"{len(bad)} of {len(golden)} geometries; first: {bad[0]}"
    # degenerate arguments keep their answers
    import ctypes
    rp = ctypes.c_int()
    assert lib.gif_conv2d_pack_dims(0, 8, ctypes.byref(rp), ctypes.byref(rp)) == -1
    assert lib.gif_conv2d_pack_dims_x3(8, 8, None, ctypes.byref(rp)) == -1
    assert lib.gif_conv2d_pack_dims_f16(8, 0, ctypes.byref(rp), ctypes.byref(rp)) == -1
    assert lib.gif_conv2d_x3_eligible(0, 32) == 0 and lib.gif_conv2d_x3_eligible(8, 26) == 0
    assert lib.gif_conv2d_f16_halo_eligible(0, 8, 3, 3, 1, 16, 16) == 0 and lib.gif_conv2d_f16_halo_eligible(8, 8, 3, 3, 1, 0, 16) == 0


def test_route_table_reports_the_recorded_packing_and_halo_answers(dump_lines):
    golden = _golden()
    cols = re.compile(r"-> RP(\d+) CP(\d+) ")
    seen = set()
    for l in dump_lines:
        if l.startswith("GIF_"):  # (the per-knob part: knobs are not set in the recording)
            continue
        m, c = rec.GEOM.search(l), cols.search(l)
        assert m and c, l
        key = f"{m.group(1)} {m.group(2)}"
        want, t = golden[key], parse(l)
        seen.add(key)
        dims = {"native": "dims", "bf16x3": "dims_x3", "f16x2": "dims_x3", "f16": "dims_f16"}[t["mode"]]
        assert [int(c.group(1)), int(c.group(2))] == want[dims], l
        if t["mode"] == "f16" and t["op"] == "fwd" and not t["dot"] and not t["error"]:
            assert t["halo"] == bool(want["halo"]) == (t["launches"][0][0] == "halo"), l
        if t["mode"] in S and not t["error"] and " d1 " not in l:  # the direct bf16x3 / f16x2 kernels run what gif_conv2d_x3_eligible accepts
            assert want["x3_eligible"] == 1, l
    assert seen == set(golden)
