"""Generates tests/golden/conv_queries_golden.json: what the packing and eligibility queries of libgif_hip.so return (no GPU needed) for
every geometry of tests/golden/conv_route_table.txt: gif_conv2d_pack_dims / _x3 / _f16 and gif_conv2d_x3_eligible for the op's (output,
contraction) channel counts and, for forward convolutions, gif_conv2d_f16_halo_eligible.  Recorded ONCE from the commit before
csrc/conv_route.h existed (its library given as the first argument); tests/test_conv_route.py holds the library and the route table to
these answers.
Run: python tests/golden/make_conv_queries_golden.py [path/to/libgif_hip.so]"""
import ctypes
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from gif_amd import _lib  # noqa: E402

GEOM = re.compile(r"\| (fwd|dgrad) \| \w+ \| d\d s\d t\d \| (B(\d+) Ci(\d+) Co(\d+) k(\d) s(\d) p(\d) (\d+)x(\d+)) ->")


def geometries():
    """Geometry keys ("op B.. Ci.. Co.. k. s. p. HxW") of the default-knob part of the route table, in order of first appearance."""
    keys = []
    with open(os.path.join(HERE, "conv_route_table.txt")) as f:
        for line in f:
            m = GEOM.search(line)
            if m and not line.startswith("GIF_") and f"{m.group(1)} {m.group(2)}" not in keys:
                keys.append(f"{m.group(1)} {m.group(2)}")
    return keys


def query(lib, key):
    op, rest = key.split(" ", 1)
    B, Ci, Co, K, s, p, H, W = (int(v) for v in re.match(r"B(\d+) Ci(\d+) Co(\d+) k(\d) s(\d) p(\d) (\d+)x(\d+)$", rest).groups())
    cout, cin = (Co, Ci) if op == "fwd" else (Ci, Co)  # the op's output / contraction channels
    rp, cp = ctypes.c_int(), ctypes.c_int()
    out = {}
    for name, fn in (("dims", lib.gif_conv2d_pack_dims), ("dims_x3", lib.gif_conv2d_pack_dims_x3), ("dims_f16", lib.gif_conv2d_pack_dims_f16)):
        assert fn(cout, cin, ctypes.byref(rp), ctypes.byref(cp)) == 0
        out[name] = [rp.value, cp.value]
    out["x3_eligible"] = lib.gif_conv2d_x3_eligible(cout, cin)
    if op == "fwd":
        Hs, Ws = (H + 2 * p - K) // s + 1, (W + 2 * p - K) // s + 1
        out["halo"] = lib.gif_conv2d_f16_halo_eligible(Ci, Co, K, K, s, Hs, Ws)
    return out


def main():
    if len(sys.argv) > 1:
        _lib.LIB_PATH = os.path.abspath(sys.argv[1])
    lib = _lib.load()
    out = {k: query(lib, k) for k in geometries()}
    with open(os.path.join(HERE, "conv_queries_golden.json"), "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in out.items()) + "\n}\n")
    print(f"{len(out)} geometries recorded from {_lib.LIB_PATH}")


if __name__ == "__main__":
    main()
