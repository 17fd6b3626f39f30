"""CPU: the FIR / reduction / pointwise-grid header (gif_amd/csrc/ew_route.h) against its recorded table, against what the comments of
the GPU route tests claim, against the scratch its callers allocate, and the library's size queries against the numbers recorded before
the header existed.

tests/host/ew_route_dump.cpp includes only the header.  It is built here with the compiler the library build needs (host only, C++17)
under AddressSanitizer and UBSan, run as a stand-alone program, and its output compared line by line with
tests/golden/ew_route_table.txt: one line per case with everything the launch code takes from the header — an upfirdn2d call's kernel,
template arguments, grid, block size and work items, with the fused column sum its partial rows and every stage of their reduction; the
stages and scratch rows of reduce_plan; the block counts of the column-sum, per-sample-product and texture-loss launches; the scratch
sizes callers allocate by — over every row of test_gpu_conv_routes.FIR_ROWS and a grid that puts each predicate on both sides of its
threshold, then what GIF_FIR_BLOCK (as the raw environment string) changes.
tests/golden/ew_queries_golden.json (tests/golden/make_ew_queries_golden.py) holds what the six size queries returned over the table's
shapes at the commit before the header: the library must still return them, and the table must report them."""
import json
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GOLDEN)
import make_ew_queries_golden as rec  # noqa: E402  (the query keys and the library queries of the recording)


@pytest.fixture(scope="module")
def dump_lines(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ew_route") / "ew_route_dump")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    # (sanitizers on the host code only: each flag right after -Xarch_host)
    flags = "-x c++ -std=c++17 -O1 -g -Wall -Werror -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined"
    cmd = [hipcc] + flags.split() + ["-I", os.path.join(ROOT, "gif_amd", "csrc"), os.path.join(ROOT, "tests", "host", "ew_route_dump.cpp"),
                                     "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert built.returncode == 0, built.stderr[-4000:]
    ran = subprocess.run([exe], capture_output=True, text=True, timeout=300)  # (either sanitizer ends the program with an error status)
    assert ran.returncode == 0, (ran.returncode, ran.stderr[-4000:])
    return ran.stdout.splitlines()


FIR = re.compile(r"^fir (\S+) \| B(\d+) C(\d+) Ho(\d+) Wo(\d+) up(\d) down(\d) px(\d) py(\d) k(\d)x(\d) \| cs([01]) -> (\S+) grid(\d+)x(\d+) thr256 "
                 r"items(\d+)(?: ; partial(\d+) ; (.*) ; ws_rows(\d+))?$")
PLAN = re.compile(r"^(\d) stages:(.*) ; tmp(\d+)$")
STAGE = re.compile(r"^([pt])\+(\d+) per(\d+) x(\d+) > ([to])\+(\d+)$")


def parse_plan(text):
    """(stages, tmp rows): a stage is (source, first row, rows per group, groups, destination, first row)."""
    m = PLAN.match(text)
    assert m, text
    stages = [STAGE.match(s.strip()) for s in m.group(2).split("|") if s.strip()]
    assert all(stages) and len(stages) == int(m.group(1)), text
    return [tuple(v if v in "pto" else int(v) for v in s.groups()) for s in stages], int(m.group(3))


def fir_cases(lines):
    """name -> {colsum flag -> match} of the default-knob fir lines."""
    out = {}
    for l in lines:
        if l.startswith("fir "):
            m = FIR.match(l)
            assert m, l
            out.setdefault(m.group(1), {})[int(m.group(12))] = m
    return out


def test_route_table_matches_the_recorded_one(dump_lines):
    with open(os.path.join(GOLDEN, "ew_route_table.txt")) as f:
        want = f.read().splitlines()
    for i, (a, b) in enumerate(zip(dump_lines, want)):
        assert a == b, f"line {i + 1}:\n got  {a}\n want {b}"
    assert len(dump_lines) == len(want)
    assert len(want) > 280 and sum("differ from the default" in l for l in want) == 8
    # every kernel, every kind of plan and every cap is named somewhere in the table
    text = "\n".join(want)
    for name in ("blur_rows<16,4>", "blur_tiled<2,4>", "up2_block", "resample<1,2>", "resample<2,1>", "generic", "0 stages", "1 stages", "2 stages",
                 "3 stages", "grid4096x1", "grid64x4", "blocks512 rpb257", "chunks64 rpb129", "tex_pair n262145 -> 1024", "grid ew n0 -> 1"):
        assert name in text, name


def test_table_covers_the_gpu_route_rows(dump_lines):
    """Every row of test_gpu_conv_routes.FIR_ROWS is in the table under its name with its shape, without and with the column sum."""
    import test_gpu_conv_routes as routes  # (pytest puts this directory on sys.path)
    cases = fir_cases(dump_lines)
    for r in routes.FIR_ROWS:
        assert set(cases[r.name]) == {0, 1}, r.name
        for m in cases[r.name].values():
            got = tuple(int(v) for v in m.groups()[1:11])
            assert got == (r.B, r.C, r.out[0], r.out[1], r.up, r.down, r.pad0, r.pad0, 4, 4), r.name
        assert (cases[r.name][1].group(17) is not None) == (r.up == 1 and r.down == 1), r.name  # the blur rows alone fuse a column sum


# What the comments of FIR_ROWS state about each row, as data: kernel, grid (x, y) and, for the rows that fuse a column sum, the
# reduction of the grid's partial rows as (rows per group, full groups, rows of the tail group or 0); None: one stage.
# (blur_tiled_131008: 512 * 2047 = 1048064 tiles are 4094 workgroups, not 4096: 63 groups of 64 and a tail of 62.)
CLAIMS = {
    "up2_even": ("up2_block", (1, 3 * 38), None),
    "up2_odd": ("up2_block", (1, 3 * 37), None),
    "up2_even_bra": ("up2_block", (1, 3 * 38), None),
    "up2_odd_bra": ("up2_block", (1, 2 * 33), None),
    "up2_bho_65535": ("up2_block", (1, 3 * 10923), None),
    "up2_bho_65536": ("generic", (3072, 1), None),
    "up2_bho_65532_bra": ("up2_block", (1, 4 * 8192), None),
    "down2": ("resample<1,2>", (1, 36), None),
    "down2_pad2": ("resample<1,2>", (1, 51), None),
    "down2_generic": ("generic", (1025, 1), None),
    "blur_tiled_small": ("blur_tiled<2,4>", (4, 1), None),
    "blur_tiled_tail": ("blur_tiled<2,4>", (520, 1), (9, 57, 7)),
    "blur_tiled_131008": ("blur_tiled<2,4>", (4094, 1), (64, 63, 62)),
    "blur_rows_131072": ("blur_rows<16,4>", (512, 1), None),
    "blur_rows_513": ("blur_rows<16,4>", (513, 1), (9, 57, 0)),
    "blur_rows_tail": ("blur_rows<16,4>", (520, 1), (9, 57, 7)),
    "blur_plain_c24": ("blur_tiled<2,4>", (3, 1), None),
}


def test_table_agrees_with_the_claims_of_the_gpu_rows(dump_lines):
    import test_gpu_conv_routes as routes
    assert set(CLAIMS) == {r.name for r in routes.FIR_ROWS}
    cases = fir_cases(dump_lines)
    for name, (kernel, grid, groups) in CLAIMS.items():
        for cs, m in cases[name].items():
            assert m.group(13) == kernel and (int(m.group(14)), int(m.group(15))) == grid, (name, m.group(0))
        m = cases[name][1]
        if m.group(17) is None:
            assert groups is None, name
            continue
        nblk = int(m.group(17))
        assert nblk == grid[0] * grid[1], name
        stages, tmp = parse_plan(m.group(18))
        if groups is None:
            assert stages == [("p", 0, nblk, 1, "o", 0)] and tmp == 0, (name, stages)
            continue
        per, full, tail = groups
        want = [("p", 0, per, full, "t", 0)] + ([("p", full * per, tail, 1, "t", full)] if tail else [])
        want.append(("t", 0, full + (1 if tail else 0), 1, "o", 0))
        assert stages == want and tmp == full + (1 if tail else 0) and full * per + tail == nblk, (name, stages)


def test_plans_sum_every_row_once_within_the_callers_scratch(dump_lines):
    """Every plan of the table reads each of its Y * nblk partial rows exactly once, writes each scratch row before the final stage reads
    it, and writes no more scratch than the bound each caller sizes by: reduce_tmp_rows_single (Y == 1: FLAME, the FIR column sums),
    reduce_tmp_rows(Y) (shading), epilogue_tmp_rows (convolutions); a FIR launch's partial rows and scratch fit the rows of its red_ws."""
    line = re.compile(r"^plan Y(\d+) nblk(\d+) -> (.*) ; bounds single(\d+) samples(\d+) epilogue(\d+)$")
    plans = []
    for l in dump_lines:
        if l.startswith("plan "):
            m = line.match(l)
            assert m, l
            Y, nblk, single, samples, epilogue = (int(m.group(i)) for i in (1, 2, 4, 5, 6))
            plans.append((Y, nblk, m.group(3), single, samples, epilogue, None))
    y1_bounds = next(p[3:6] for p in plans if p[0] == 1)  # (the bounds of a Y == 1 plan do not depend on nblk)
    for by_cs in fir_cases(dump_lines).values():
        m = by_cs[1]
        if m.group(17) is not None:
            plans.append((1, int(m.group(17)), m.group(18)) + y1_bounds + (int(m.group(19)),))
    assert len(plans) > 100
    seen = set()
    for Y, nblk, text, single, samples, epilogue, ws_rows in plans:
        stages, tmp = parse_plan(text)
        seen.add((Y > 1, len(stages)))
        if Y <= 0 or nblk <= 0:
            assert not stages and tmp == 0
            continue
        read_p, written_t, read_t, written_o = [], [], [], []
        for src, r0, per, groups, dst, w0 in stages:
            (read_p if src == "p" else read_t).extend(range(r0, r0 + per * groups))
            if src == "t":  # the final stage: everything it reads has been written
                assert sorted(written_t) == list(range(per * groups)) == sorted(read_t), text
            (written_t if dst == "t" else written_o).extend(range(w0, w0 + groups))
        assert sorted(read_p) == list(range(Y * nblk)), text
        assert sorted(written_o) == list(range(Y)) and len(written_t) == tmp, text
        assert tmp <= samples and tmp <= epilogue and (Y > 1 or tmp <= single), (Y, nblk, tmp)
        if ws_rows is not None:
            assert nblk + tmp <= nblk + single <= ws_rows and nblk + single <= epilogue, (nblk, tmp, ws_rows)
    assert seen == {(False, 0), (False, 1), (False, 2), (False, 3), (True, 1), (True, 2)}


def _golden():
    with open(os.path.join(GOLDEN, "ew_queries_golden.json")) as f:
        return json.load(f)


def test_library_size_queries_match_the_recorded_ones():
    from gif_amd import _lib
    lib = _lib.load()
    golden = _golden()
    assert list(golden) == rec.keys(), "the recorded queries are not the route table's"
    bad = [(k, rec.query(lib, k), want) for k, want in golden.items() if rec.query(lib, k) != want]
    assert not bad, f"{len(bad)} of {len(golden)} queries; first: {bad[0]}"
    # degenerate arguments keep their answers
    assert lib.gif_conv_epilogue_ws_floats(0, 8) == 0 and lib.gif_conv_epilogue_ws_floats(8, 0) == 0
    assert lib.gif_colsum_partial_floats(100, 6) == 0 and lib.gif_colsum_partial_floats(100, 1028) == 0 and lib.gif_colsum_partial_floats(100, 0) == 0
    assert lib.gif_shade_sh_bwd_workspace_bytes(0, 16, 16) == 0 and lib.gif_flame_skin_bwd_workspace_bytes(0, 64, 36, 5) == 0


def test_route_table_reports_the_recorded_sizes(dump_lines):
    golden = dict(_golden())
    single = None
    for l in dump_lines:
        if l.startswith("GIF_"):  # (knobs are not set in the recording)
            continue
        m = FIR.match(l)
        if m and m.group(19) is not None:
            B, C, Ho, Wo = (int(v) for v in m.groups()[1:5])
            assert golden.pop(f"epilogue rows{B * Ho * Wo} C{C}", None) in (None, int(m.group(19)) * C), l  # (None: a shape seen before)
            continue
        m = re.match(r"^epilogue rows(\d+) -> cap\d+ ws_rows(\d+)$", l)
        if m:
            assert golden.pop(f"epilogue rows{m.group(1)} C{rec.ODD_COUT}") == int(m.group(2)) * 8, l
        m = re.match(r"^grid colsum nrows(\d+) C(\d+) -> blocks(\d+) rpb\d+$", l)
        if m:
            assert golden.pop(f"colsum nrows{m.group(1)} C{m.group(2)}") == int(m.group(3)) * int(m.group(2)), l
        m = re.match(r"^grid mul_reduce HW(\d+) -> chunks(\d+) rpb\d+$", l)
        if m:
            assert golden.pop(f"mul_reduce HW{m.group(1)}") == int(m.group(2)), l
        m = re.match(r"^grid tex_pair n(\d+) -> (\d+)$", l)
        if m:
            assert golden.pop(f"tex_pair n{m.group(1)}") == int(m.group(2)), l
        m = re.match(r"^tmp_rows Y(\d+) -> (\d+)$", l)
        if m:  # one backward block per sample: B partial rows + the scratch, 27 floats each
            B = int(m.group(1))
            assert golden.pop(f"shade B{B} H{rec.SHADE_HW[0]} W{rec.SHADE_HW[1]}") == (B + int(m.group(2))) * 27 * 4, l
        m = re.match(r"^plan .* bounds single(\d+) ", l)
        if m:
            single = int(m.group(1))
    for B, V, KP, J in rec.FLAME_SHAPES:  # per region: one partial row per 32 / 64 vertices + the scratch of a Y == 1 reduction
        want = ((-(-V // 32) + single) * B * KP + (-(-V // 64) + single) * B * J * 12) * 4
        assert golden.pop(f"flame B{B} V{V} KP{KP} J{J}") == want
    assert not golden, list(golden)
