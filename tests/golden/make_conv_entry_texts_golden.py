"""Generates tests/golden/conv_entry_texts_golden.json: what libgif_hip.so answers (no GPU needed) to every row of
tests/test_conv_entry_texts_cpu.py — the return code and gif_last_error() text of a refused call, or the value of a size query.
Recorded ONCE from the commit before the host bodies of the packing, weight-gradient and fused-sum entry points were merged (its
library given as the first argument); the test holds the library to these answers.
Run: python tests/golden/make_conv_entry_texts_golden.py [path/to/libgif_hip.so]"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
from gif_amd import _lib  # noqa: E402
import test_conv_entry_texts_cpu as rows  # noqa: E402


def main():
    if len(sys.argv) > 1:
        _lib.LIB_PATH = os.path.abspath(sys.argv[1])
    lib = _lib.load()
    out = {rid: rows.answer(lib, kind, entry, args) for rid, kind, entry, args in rows.ROWS}
    with open(rows.GOLDEN, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in out.items()) + "\n}\n")
    print(f"{len(out)} rows recorded from {_lib.LIB_PATH}")


if __name__ == "__main__":
    main()
