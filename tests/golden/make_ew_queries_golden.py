"""Generates tests/golden/ew_queries_golden.json: what the six size queries behind the pointwise launches and the reductions of
libgif_hip.so return (no GPU needed) over the shapes of tests/golden/ew_route_table.txt: gif_conv_epilogue_ws_floats for the output rows
and channels of every fused FIR line and for the rows of every `epilogue` line, gif_colsum_partial_floats / gif_mul_reduce_chunks /
gif_texture_pair_loss_partials for every `grid` line of theirs, gif_shade_sh_bwd_workspace_bytes for the sample counts of the `tmp_rows`
lines and gif_flame_skin_bwd_workspace_bytes for FLAME_SHAPES.  Recorded ONCE from the commit before csrc/ew_route.h existed (its library
given as the first argument); tests/test_ew_route.py holds the library and the route table to these answers.
Run: python tests/golden/make_ew_queries_golden.py [path/to/libgif_hip.so]"""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from gif_amd import _lib  # noqa: E402

ODD_COUT = 6  # channel count of the `epilogue` lines' queries: not a multiple of 4 (the query rounds it up)
SHADE_HW = (16, 16)  # image of the shade queries: one backward block per sample
FLAME_SHAPES = [(1, 5023, 400, 5), (2, 33, 36, 5), (4, 64, 0, 1), (3, 20000, 100, 8), (8, 1, 63, 8)]  # B, V, KP, J

PATTERNS = [
    (re.compile(r"^fir \S+ \| B(\d+) C(\d+) Ho(\d+) Wo(\d+) .* ; ws_rows\d+$"), lambda B, C, Ho, Wo: f"epilogue rows{B * Ho * Wo} C{C}"),
    (re.compile(r"^epilogue rows(\d+) ->"), lambda rows: f"epilogue rows{rows} C{ODD_COUT}"),
    (re.compile(r"^grid colsum nrows(\d+) C(\d+) ->"), lambda n, C: f"colsum nrows{n} C{C}"),
    (re.compile(r"^grid mul_reduce HW(\d+) ->"), lambda HW: f"mul_reduce HW{HW}"),
    (re.compile(r"^grid tex_pair n(\d+) ->"), lambda n: f"tex_pair n{n}"),
    (re.compile(r"^tmp_rows Y(\d+) ->"), lambda Y: f"shade B{Y} H{SHADE_HW[0]} W{SHADE_HW[1]}"),
]


def keys():
    """Query keys of the default-knob part of the route table in order of first appearance, then the FLAME shapes."""
    out = []
    with open(os.path.join(HERE, "ew_route_table.txt")) as f:
        for line in f:
            for pat, key in PATTERNS:
                m = pat.match(line.rstrip("\n"))
                if m and key(*(int(v) for v in m.groups())) not in out:
                    out.append(key(*(int(v) for v in m.groups())))
    return out + [f"flame B{B} V{V} KP{KP} J{J}" for B, V, KP, J in FLAME_SHAPES]


def query(lib, key):
    kind = key.split(" ", 1)[0]
    a = [int(v) for v in re.findall(r"\d+", key)]
    fn = {"epilogue": lib.gif_conv_epilogue_ws_floats, "colsum": lib.gif_colsum_partial_floats, "mul_reduce": lib.gif_mul_reduce_chunks,
          "tex_pair": lib.gif_texture_pair_loss_partials, "shade": lib.gif_shade_sh_bwd_workspace_bytes,
          "flame": lib.gif_flame_skin_bwd_workspace_bytes}[kind]
    return int(fn(*a))


def main():
    if len(sys.argv) > 1:
        _lib.LIB_PATH = os.path.abspath(sys.argv[1])
    lib = _lib.load()
    out = {k: query(lib, k) for k in keys()}
    with open(os.path.join(HERE, "ew_queries_golden.json"), "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in out.items()) + "\n}\n")
    print(f"{len(out)} queries recorded from {_lib.LIB_PATH}")


if __name__ == "__main__":
    main()
