"""GPU: gif::split_pair_h2 (gif_amd/csrc/common.h), the fp32 -> (hi, lo) f16 split inside every f16x2 kernel, bit for bit.

tests/host/h2_split_check.hip includes the header and calls the function from small kernels of its own.  It is built here with the flags of
gif_amd/csrc/Makefile and run ONCE; the tests read its output.
  * sweep: all 2^32 patterns of a0 (a1 a bijection of the pattern) under the scales 2^e, e in SCALES, against the restatement kept in that
    source — multiply, convert, subtract, convert, one pinned operation each.  hi is compared for every finite a, lo wherever the reference
    hi is finite; the program prints how many elements that rule left out, and for e = -126 and -113 (|a| * 2^e < 2^15) it must be none.
    The same again with each split between two MFMAs at two workgroups per CU: the condition under which packed fp32 forms went wrong
    (profiles/r5_pk_opsel_probe.txt).
  * table: edge values under the scales 1 and 2^13 against numpy, a reference no GPU code has a part in:
    hi = float16(float32(a * sc)), lo = float16(float32(a * sc) - float32(hi))."""
import os
import shutil
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALES = (-126, -113, -30, -1, 0, 13, 30, 126)


def _f32(bits):
    return np.array([bits], np.uint32).view(np.float32)[0]


def edge_values():
    """fp32 values at the edges of the two roundings (each also negated)."""
    pos = [
        np.float32(0.0),
        _f32(0x00000001), _f32(0x007FFFFF),                                        # smallest and largest fp32 subnormal
        np.float32(2.0 ** -24 * (1 - 2.0 ** -11)), np.float32(2.0 ** -24 * (1 + 2.0 ** -11)),  # around the smallest f16 subnormal
        np.float32(65472.0), np.float32(65504.0), np.float32(65519.99),            # rescale limit, f16 maximum, just below the overflow threshold
        np.float32(1 + 2.0 ** -11), np.float32(1 + 3 * 2.0 ** -11),                # ties of the hi rounding: down to even, up to even
        np.float32(1 + 2.0 ** -12 + 2.0 ** -23), np.float32(1 + 2.0 ** -12 + 3 * 2.0 ** -23),  # ties of the lo rounding (hi = 1)
    ]
    return np.array(pos + [-v for v in pos], np.float32)


def edge_cases():
    """(a0, a1, sc) triples: every edge value in both halves of the pair, under both scales."""
    v = edge_values()
    a0 = np.concatenate([v, v])
    a1 = np.concatenate([np.roll(v, 5), np.roll(v, 5)])
    sc = np.concatenate([np.full(len(v), 1.0, np.float32), np.full(len(v), 2.0 ** 13, np.float32)])
    return a0, a1, sc


def numpy_split(a, sc):
    with np.errstate(over="ignore", invalid="ignore"):
        x = (a * sc).astype(np.float32)
        hi = x.astype(np.float16)
        lo = (x - hi.astype(np.float32)).astype(np.float32).astype(np.float16)
    return hi.view(np.uint16).astype(np.uint32), lo.view(np.uint16).astype(np.uint32)


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if shutil.which(hipcc) is None:
        pytest.skip("no hipcc")
    d = tmp_path_factory.mktemp("h2_split")
    exe = str(d / "h2_split_check")
    cmd = [hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-Wall", "-Wno-unused-function", "-I", os.path.join(ROOT, "include"), "-I",
           os.path.join(ROOT, "gif_amd", "csrc"), os.path.join(ROOT, "tests", "host", "h2_split_check.hip"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert built.returncode == 0, built.stderr[-4000:]
    a0, a1, sc = edge_cases()
    cases = str(d / "cases.txt")
    with open(cases, "w") as f:
        for t in zip(a0.view(np.uint32), a1.view(np.uint32), sc.view(np.uint32)):
            f.write("%08x %08x %08x\n" % t)
    ran = subprocess.run([exe, cases], capture_output=True, text=True, timeout=120)
    assert ran.returncode == 0, (ran.returncode, ran.stdout[-2000:], ran.stderr[-2000:])
    sweep, table = {}, []
    for line in ran.stdout.splitlines():
        w = line.split()
        if w[0] == "sweep":
            sweep[(w[1], int(w[3]))] = {w[i]: int(w[i + 1]) for i in range(4, len(w), 2)}
        elif w[0] == "table":
            table.append((int(w[1], 16), int(w[2], 16)))
    return sweep, table


@pytest.mark.parametrize("setting", ["bare", "mfma"])
def test_every_pattern_splits_as_the_restated_arithmetic(report, setting):
    sweep, _ = report
    for e in SCALES:
        c = sweep[(setting, e)]
        print(setting, e, c)
        # both elements of a pair run through all 2^32 patterns; 2^24 of them are infinities and NaNs
        assert c["nonfinite"] == 2 * 2 ** 24 and c["hi_cmp"] == 2 * (2 ** 32 - 2 ** 24), (e, c)
        assert c["lo_cmp"] + c["excluded"] == c["hi_cmp"], (e, c)
        assert c["hi_bad"] == 0 and c["lo_bad"] == 0, (e, c)
        if e in (-126, -113):
            assert c["excluded"] == 0, (e, c)
    assert sweep[(setting, 0)]["excluded"] > 0  # (the rule is exercised: |a| >= 65520 overflows hi under the scale 1)


def test_edge_values_split_as_numpy_says(report):
    _, table = report
    a0, a1, sc = edge_cases()
    h0, l0 = numpy_split(a0, sc)
    h1, l1 = numpy_split(a1, sc)
    assert len(table) == len(a0) == 48
    for i, (hi, lo) in enumerate(table):
        want = (int(h0[i] | (h1[i] << 16)), int(l0[i] | (l1[i] << 16)))
        assert (hi, lo) == want, "a0 %r a1 %r sc %r: got %08x %08x, want %08x %08x" % (a0[i], a1[i], sc[i], hi, lo, *want)


def test_the_numpy_table_holds_the_edges_it_names():
    """The reference side alone (no GPU result enters): the table's expected dwords at the values the docstring promises."""
    one = np.float32(1.0)
    def split(a, sc=one):
        h, l = numpy_split(np.array([a], np.float32), np.array([sc], np.float32))
        return int(h[0]), int(l[0])
    assert split(np.float32(-0.0)) == (0x8000, 0x0000)                   # hi keeps the sign, x - hi = +0
    assert split(_f32(0x80000001)) == (0x8000, 0x8000)                   # a negative fp32 subnormal: both terms -0
    assert split(np.float32(2.0 ** -24 * (1 + 2.0 ** -11))) == (0x0001, 0x0000)   # lo 2^-35 is below half the f16 quantum
    assert split(np.float32(2.0 ** -24 * (1 - 2.0 ** -11))) == (0x0001, 0x8000)
    assert split(np.float32(65504.0)) == (0x7BFF, 0x0000)
    assert split(np.float32(65472.0)) == (0x7BFE, 0x0000)                # 65504 - 32: an f16 number
    assert split(np.float32(65519.99)) == (0x7BFF, 0x4BFE)               # fp32 65519.98828125 = 65504 + (16 - 3/256): a tie, to even 16 - 2/128
    assert split(np.float32(65504.0), np.float32(2.0 ** 13)) == (0x7C00, 0xFC00)  # overflow: hi = inf, lo = -inf
    assert split(np.float32(1 + 2.0 ** -11)) == (0x3C00, 0x1000)         # tie to even: down, lo = +2^-11
    assert split(np.float32(1 + 3 * 2.0 ** -11)) == (0x3C02, 0x9000)     # tie to even: up, lo = -2^-11
    assert split(np.float32(1 + 2.0 ** -12 + 2.0 ** -23)) == (0x3C00, 0x0C00)      # lo tie: 2^-12 (1 + 2^-11) -> 2^-12
    assert split(np.float32(1 + 2.0 ** -12 + 3 * 2.0 ** -23)) == (0x3C00, 0x0C02)  # lo tie: 2^-12 (1 + 3 * 2^-11) -> 2^-12 (1 + 2^-9)
