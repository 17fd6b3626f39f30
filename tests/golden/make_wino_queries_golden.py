"""Generates tests/golden/wino_queries_golden.json: what the Winograd size queries of libgif_hip.so return (no GPU needed) for every
geometry of tests/golden/wino_route_table.txt: gif_winograd_pack_dims, gif_winograd_pack_dims_x3, gif_winograd_workspace_floats and
gif_winograd_weight_f32h2_bytes (of the _x3 dims).  Recorded ONCE from the commit before csrc/wino_route.h existed (its library given as
the first argument); tests/test_wino_route.py holds the library and the route table to these numbers.
Run: python tests/golden/make_wino_queries_golden.py [path/to/libgif_hip.so]"""
import ctypes
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from gif_amd import _lib  # noqa: E402

GEOM = re.compile(r"^B(\d+) H(\d+) W(\d+) C(\d+) Co(\d+) \|")


def geometries():
    """Geometry keys of the default-knob part of the route table, in order of first appearance."""
    keys = []
    with open(os.path.join(HERE, "wino_route_table.txt")) as f:
        for line in f:
            m = GEOM.match(line)
            if m and line[:m.end() - 2] not in keys:
                keys.append(line[:m.end() - 2])
    return keys


def query(lib, key):
    """The library's answers for one geometry key."""
    B, H, W, C, Co = (int(v) for v in GEOM.match(key + " |").groups())
    rp, cp = ctypes.c_int(), ctypes.c_int()
    out = {}
    assert lib.gif_winograd_pack_dims(Co, C, ctypes.byref(rp), ctypes.byref(cp)) == 0
    out["pack_dims"] = [rp.value, cp.value]
    assert lib.gif_winograd_pack_dims_x3(Co, C, ctypes.byref(rp), ctypes.byref(cp)) == 0
    out["pack_dims_x3"] = [rp.value, cp.value]
    out["workspace_floats"] = lib.gif_winograd_workspace_floats(B, H, W, C)
    out["weight_f32h2_bytes"] = lib.gif_winograd_weight_f32h2_bytes(rp.value, cp.value)
    return out


def main():
    if len(sys.argv) > 1:
        _lib.LIB_PATH = os.path.abspath(sys.argv[1])
    lib = _lib.load()
    out = {k: query(lib, k) for k in geometries()}
    with open(os.path.join(HERE, "wino_queries_golden.json"), "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in out.items()) + "\n}\n")
    print(f"{len(out)} geometries recorded from {_lib.LIB_PATH}")


if __name__ == "__main__":
    main()
