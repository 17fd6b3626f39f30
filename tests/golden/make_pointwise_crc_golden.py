"""Generates tests/golden/pointwise_crc_golden.json: the CRC-32 of every result of every case of tests/test_gpu_pointwise_bits.py, on the
GPU, from the library this checkout built — or from another build of it (the commit the bits are to be compared with), given as the
first argument.  Runs every case twice and refuses to write a case whose two runs differ.
Run: python tests/golden/make_pointwise_crc_golden.py [path/to/libgif_hip.so] [output.json]"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
from gif_amd import _lib  # noqa: E402


def main():
    if len(sys.argv) > 1 and sys.argv[1]:
        _lib.LIB_PATH = os.path.abspath(sys.argv[1])
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, "pointwise_crc_golden.json")
    import test_gpu_pointwise_bits as bits
    out, unstable = {}, []
    for c in bits.CASES:
        a, b = bits.pointwise_crcs(*c), bits.pointwise_crcs(*c)
        if a == b:
            out[bits.case_id(*c)] = a
        else:
            unstable.append(bits.case_id(*c))
    with open(out_path, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(out)} cases recorded from {_lib.LIB_PATH}; not reproducible: {unstable}")
    return 1 if unstable else 0


if __name__ == "__main__":
    sys.exit(main())
