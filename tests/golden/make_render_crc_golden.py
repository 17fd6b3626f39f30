"""Generates tests/golden/render_crc_golden.json: the CRC-32s of every case of tests/test_gpu_render_bits.py (each forward result
and each gradient asked for, the albedo gradient excepted), on the GPU, from this checkout's gif_amd package — or from another
checkout's (the commit the bits are to be compared with: its root, with its library built, given as the first argument; the test
module drives public API only, so this checkout's copy of it runs against either).  Runs every case twice and refuses to write a
case whose two results differ.  Cases left out because two runs disagreed: none — the first recording refused `texture_map` for its
gradient to the source image (CRCs 202435531 and 1985661101): gif_texture_map_bwd_f32 scatters with float atomics, as
include/gif_hip.h says, so the test module launches that gradient and hashes the case's forward results only.
One case cannot run at the commit the file was recorded from: raster-none-f2-va (rasterize_attributes over a mesh without faces)
raised "face_gather_bwd: null pointer" in its backward there, the empty face gradient's address being 0; only
antialias._AntialiasFn special-cased F == 0.  Its record is the definition instead — no face, so exact zeros: the image, the mask
and both gradients, in the shapes and dtypes test_no_faces_give_exact_zeros asserts.
Run: python tests/golden/make_render_crc_golden.py [path/to/other/checkout] [output.json]"""
import json
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1] else os.path.dirname(os.path.dirname(HERE)))
import gif_amd  # noqa: E402


def no_faces_definition(bits):
    zeros = lambda dtype, *shape: zlib.crc32(np.zeros(shape, dtype).tobytes())
    V = bits.aref.edge_mesh(bits.B, bits.H)[0].shape[1]
    return {"img": zeros(np.float32, bits.B, 3, bits.H, bits.W), "mask": zeros(np.bool_, bits.B, 1, bits.H, bits.W),
            "g_v": zeros(np.float64, bits.B, V, 3), "g_a": zeros(np.float32, bits.B, V, 3)}


def main():
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, "render_crc_golden.json")
    import test_gpu_render_bits as bits
    out, unstable, by_definition = {}, [], []
    for name in bits.CASES:
        try:
            a, b = bits.render_crcs(name), bits.render_crcs(name)
        except gif_amd._lib.GifHipError as e:
            if name != "raster-none-f2-va":
                raise
            print(f"{name}: {e}: recorded by definition", flush=True)
            a = b = no_faces_definition(bits)
            by_definition.append(name)
        if a == b:
            out[name] = a
        else:
            unstable.append(name)
        print(name, a, "" if a == b else f"!= {b}", flush=True)
    with open(out_path, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(out)} cases recorded from {os.path.dirname(gif_amd.__file__)}; not reproducible: {unstable}; "
          f"by definition: {by_definition}")
    return 1 if unstable else 0


if __name__ == "__main__":
    sys.exit(main())
