"""Generates tests/golden/wgrad_splits_golden.json: what the weight-gradient size queries of libgif_hip.so return (no GPU needed) for
every geometry of tests/golden/wgrad_route_table.txt, in each of the three fp32 contraction modes: gif_conv2d_wgrad_dims / _dims_f16,
gif_conv2d_wgrad_splits / _splits_f16 and, for the Winograd plane GEMMs, gif_conv3x3_winograd_wgrad_splits.  Recorded ONCE from the
commit before csrc/wgrad_route.h existed (its library given as the first argument); tests/test_wgrad_route.py holds the library and the
route table to these numbers.
Run: python tests/golden/make_wgrad_splits_golden.py [path/to/libgif_hip.so]"""
import ctypes
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from gif_amd import _lib  # noqa: E402

CONV = re.compile(r"^B(\d+) Hs(\d+) Ws(\d+) Cs(\d+) Cb(\d+) k(\d) s(\d) p(\d) \|")
PLANES = re.compile(r"^planes tiles(\d+) Cs(\d+) Cb(\d+) \|")


def geometries():
    """Geometry keys of the default-knob part of the route table, in order of first appearance."""
    keys = []
    with open(os.path.join(HERE, "wgrad_route_table.txt")) as f:
        for line in f:
            m = CONV.match(line) or PLANES.match(line)
            if m and line[:m.end() - 2] not in keys:
                keys.append(line[:m.end() - 2])
    return keys


def query(lib, key):
    """The library's answers for one geometry key, in the three contraction modes (the mode is restored)."""
    rp, cp = ctypes.c_int(), ctypes.c_int()
    before = lib.gif_get_fp32_mfma_mode()
    out = {}
    try:
        m = PLANES.match(key + " |")
        if m:
            ntiles, cs, cb = (int(v) for v in m.groups())
            out["winograd_splits"] = []
            for mode in (0, 1, 2):
                assert lib.gif_set_fp32_mfma_mode(mode) == 0
                out["winograd_splits"].append(lib.gif_conv3x3_winograd_wgrad_splits(1, 2, 2 * ntiles, cs, cb))
            return out
        B, Hs, Ws, Cs, Cb, K, s, p = (int(v) for v in CONV.match(key + " |").groups())
        g = _lib.ConvGeom(B, (Hs - 1) * s + K - 2 * p, (Ws - 1) * s + K - 2 * p, Cb, Hs, Ws, Cs, K, K, s, p)
        assert lib.gif_conv2d_wgrad_dims(Cs, Cb, ctypes.byref(rp), ctypes.byref(cp)) == 0
        out["dims"] = [rp.value, cp.value]
        assert lib.gif_conv2d_wgrad_dims_f16(Cs, Cb, ctypes.byref(rp), ctypes.byref(cp)) == 0
        out["dims_f16"] = [rp.value, cp.value]
        out["splits"], out["splits_f16"] = [], []
        for mode in (0, 1, 2):
            assert lib.gif_set_fp32_mfma_mode(mode) == 0
            out["splits"].append(lib.gif_conv2d_wgrad_splits(ctypes.byref(g)))
            out["splits_f16"].append(lib.gif_conv2d_wgrad_splits_f16(ctypes.byref(g)))
        return out
    finally:
        lib.gif_set_fp32_mfma_mode(before)


def main():
    if len(sys.argv) > 1:
        _lib.LIB_PATH = os.path.abspath(sys.argv[1])
    lib = _lib.load()
    out = {k: query(lib, k) for k in geometries()}
    with open(os.path.join(HERE, "wgrad_splits_golden.json"), "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in out.items()) + "\n}\n")
    print(f"{len(out)} geometries recorded from {_lib.LIB_PATH}")


if __name__ == "__main__":
    main()
