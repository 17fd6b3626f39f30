"""CPU: the f16x2 row arithmetic every f16x2 kernel and both weight packers share (gif_amd/csrc/h2_row.h: exponent choice, the grow
decision in its wave-uniform and private forms, the window test, the weight rows' exponent and flag) against tests/h2_row_ref.py.

tests/host/h2_row_check.cpp includes only that header.  It is built here with the compiler the library build needs (host only, C++17)
under AddressSanitizer and UBSan, run as a stand-alone program, and every line it prints is recomputed from the line's inputs by the
reference; the properties the kernels rely on are asserted on top."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import h2_row_ref as ref  # noqa: E402


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("h2_row") / "h2_row_check")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    # (sanitizers on the host code only: each flag right after -Xarch_host)
    flags = "-x c++ -std=c++17 -O1 -g -Wall -Werror -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined"
    cmd = [hipcc] + flags.split() + ["-I", os.path.join(ROOT, "gif_amd", "csrc"), os.path.join(ROOT, "tests", "host", "h2_row_check.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert built.returncode == 0, built.stderr[-4000:]
    ran = subprocess.run([exe], capture_output=True, text=True, timeout=300)  # (either sanitizer ends the program with an error status)
    assert ran.returncode == 0, (ran.returncode, ran.stderr[-4000:])
    return ran.stdout.splitlines()


def _of(lines, kind):
    return [l for l in lines if l.startswith(kind + " ")]


def _f(hexbits):
    return ref.f32(int(hexbits, 16))


def test_exponent_for_a_row_maximum(lines):
    got = _of(lines, "exp")
    assert len(got) == 2 * 256 * 3
    seen = set()
    for l in got:
        t, m, e = re.match(r"exp t=(\d+) m=([0-9a-f]{8}) -> e=(-?\d+)$", l).groups()
        t, e, m = int(t), int(e), _f(m)
        seen.add((t, ref.field(m), ref.bits_of(m) & 0x7FFFFF))
        assert e == ref.exp_for(m, t), l
        assert -126 <= e <= 126, l
        if 1 <= ref.field(m) <= 254:  # a finite normal value
            if abs(t - (ref.field(m) - 127)) <= 126:  # not clamped: the scaled maximum lands in the target binade
                assert 2.0 ** t <= float(np.ldexp(np.float64(m), e)) < 2.0 ** (t + 1), l
            else:
                assert abs(e) == 126, l
    assert seen == {(t, f, mt) for t in (13, 14) for f in range(256) for mt in (0, 1, 0x7FFFFF)}
    # the clamp sets in exactly where the exponent would leave [-126, 126]
    assert ref.exp_for(ref.f32(14 << 23), 13) == 126 and ref.exp_for(ref.f32(15 << 23), 13) == 125
    assert ref.exp_for(ref.f32(15 << 23), 14) == 126 and ref.exp_for(ref.f32(16 << 23), 14) == 125


STATE = r"ex=(-?\d+) dl=(-?\d+) sc=([0-9a-f]{8}) lim=([0-9a-f]{8}) max=([0-9a-f]{8}) gmin=([0-9a-f]{8}) wide=([01])"


def _check_step(l, row, old_ex, m, state):
    ex, dl = int(state[0]), int(state[1])
    sc, lim = _f(state[2]), _f(state[3])
    assert float(sc) == 2.0 ** ex, l
    with np.errstate(over="ignore"):
        assert lim == np.float32(np.ldexp(np.float64(65472.0), -ex)), l
    assert dl == ex - old_ex and ex <= old_ex, l  # (the exponent never goes back up)
    if ex > -126:
        assert float(m) * 2.0 ** ex <= 65472.0, l
    assert l.split(" -> ")[1].startswith(row.text()), (l, row.text())


def test_tracker_sequences_in_both_forms(lines):
    rows, names = {}, set()
    lane, priv = _of(lines, "lane"), _of(lines, "priv")
    assert len(lane) == len(priv) >= 40
    for l in lane:
        name, step, m, *state = re.match(r"lane (\w+) (\d+) m=([0-9a-f]{8}) -> " + STATE + "$", l).groups()
        row = rows.setdefault(("lane", name), ref.Row())
        names.add(name)
        old, m = row.ex, _f(m)
        row.observe([m])
        _check_step(l, row, old, m, state)
    for l in priv:
        name, step, m0, m1, *state, grew = re.match(r"priv (\w+) (\d+) m0=([0-9a-f]{8}) m1=([0-9a-f]{8}) -> " + STATE + r" grew=([01])$", l).groups()
        row = rows.setdefault(("priv", name), ref.Row())
        old, m0, m1 = row.ex, _f(m0), _f(m1)
        assert int(grew) == int(row.observe([m0, m1])), l
        _check_step(l, row, old, max(m0, m1), state)
    assert names >= {"first", "headroom_in", "headroom_out", "at_lim", "ties", "zeros_between", "tiny", "huge", "tiny_then_huge", "shrinking",
                     "all_zero"}
    # both forms end every sequence in the same exponent, and the cases are what their names say
    for name in names:
        assert rows[("lane", name)].ex == rows[("priv", name)].ex, name
    by = {(re.split(" ", l)[1], int(re.split(" ", l)[2])): re.search(STATE, l).groups() for l in lane}
    assert by[("first", 0)][:2] == ("13", "-113")  # from the initial exponent 126 to the one of 1.0
    assert [by[("headroom_in", k)][1] for k in range(4)] == ["-113", "0", "0", "0"]
    assert [by[("headroom_out", k)][0] for k in range(4)] == ["13", "10", "7", "-6"]
    assert [by[("at_lim", k)][1] for k in range(4)] == ["-113", "0", "-2", "0"]  # m == lim keeps the exponent, the next float up does not
    assert [by[("ties", k)][1] for k in range(5)] == ["-114", "0", "0", "-3", "0"]
    assert [by[("all_zero", k)][0] for k in range(3)] == ["126"] * 3 and by[("all_zero", 2)][5] == "ffffffff"
    assert [by[("shrinking", k)][0] for k in range(7)] == ["4"] * 7
    assert by[("tiny", 0)][0] == "126" and by[("huge", 3)][0] == str(13 - 126)  # clamped at the top; 1e38 lies in binade 126, 3e38 within its 4x


def test_window_of_a_row(lines):
    got = {}
    for l in _of(lines, "wide"):
        name, groups, wide = re.match(r"wide (\w+) g=([0-9a-f,]+) -> wide=([01])$", l).groups()
        row = ref.Row()
        for g in groups.split(","):
            row.observe([_f(g)])
        assert int(wide) == int(row.wide()), l
        got[name] = int(wide)
    for tail in ("", "_mant", "_first"):
        assert [got["below_%d%s" % (d, tail)] for d in (13, 14, 15)] == [0, 0, 1], tail
    assert got["only_zero"] == 0 and got["zeros_one_value"] == 0 and got["zeros_one_tiny"] == 0 and got["denormal_group"] == 1


def test_weight_row_exponent_and_flag(lines):
    wrow = _of(lines, "wrow")
    assert len(wrow) == 10
    for l in wrow:
        rm, e = re.match(r"wrow rowmax=([0-9a-f]{8}) -> e=(-?\d+)$", l).groups()
        assert int(e) == ref.weight_exp(_f(rm)), l
    assert "wrow rowmax=3f800000 -> e=14" in wrow
    got = {}
    for l in _of(lines, "wnar"):
        rm, gm, narrow = re.match(r"wnar rowmax=([0-9a-f]{8}) gm=([0-9a-f]{8}) -> narrow=([01])$", l).groups()
        assert int(narrow) == int(ref.weight_narrow(_f(rm), _f(gm))), l
        if int(gm, 16) == 0:
            assert narrow == "0", l  # an all-zero group never flags its row
        got[(rm, gm)] = int(narrow)
    assert len(got) >= 30
    one = "3f800000"
    assert [got[(one, "%08x" % ref.bits_of(np.ldexp(np.float32(1.0), -d)))] for d in (15, 16, 17)] == [0, 0, 1]
    assert "wnar_kept -> narrow=1" in lines
