"""Generates tests/golden/conv_route_cases.txt: for every fwd / dgrad row of tests/test_gpu_conv_routes.ROWS in every mode it lists, the
library call gif_amd/ops.py makes for it when the call ends in csrc/conv_igemm.hip (rows that take the Winograd route are left out), one
line per case:
    <row>-<mode>  fwd|dgrad  native|bf16x3|f16x2|f16  dense scaled dot  B Cin Cout K stride pad H W
(the forward convolution, channel counts as the activations carry them; dense / scaled / dot: tap-dense entry point, per-sample input
scales, dot fusion).  The decisions are ops.winograd_eligible, x3_conv, x3_tapdense and h2_conv, which are pure Python: no GPU and no
library is needed.  tests/host/conv_route_dump.cpp reads the file; tests/test_conv_route.py checks that it is current.
Run: python tests/golden/make_conv_route_cases.py"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))


def case_lines():
    import torch
    from gif_amd import ops
    import test_gpu_conv_routes as routes
    lines = []
    real_mode = ops.get_fp32_mfma_mode
    try:
        for row in routes.ROWS:
            if row.op == "wgrad":
                continue
            B, Ci, Co, K, s, p, H, W = row.shape
            spec = ops.ConvSpec(K, K, s, p)
            Hs, Ws = (H + 2 * p - K) // s + 1, (W + 2 * p - K) // s + 1
            for mode in row.fams:
                f16 = mode == "f16"
                dt = torch.float16 if f16 else torch.float32
                ops.get_fp32_mfma_mode = (lambda m: lambda: m)("native" if f16 else mode)
                saved = [(k, getattr(ops, k)) for k, _ in row.patch]
                for k, v in row.patch:
                    setattr(ops, k, v)
                try:
                    cb, cs = routes.cpad(Ci, f16), routes.cpad(Co, f16)
                    epi = {"in_scale": True} if row.epi in ("full", "scale") else {}
                    if row.op == "fwd":
                        wino = ops.winograd_eligible(spec, B, H, W, cb, cs, dtype=dt)
                        cin, cout, hw_out = cb, cs, Hs * Ws
                    else:
                        wino = (H, W) == (Hs, Ws) and ops.winograd_eligible(spec, B, Hs, Ws, cs, cb, dtype=dt)
                        cin, cout, hw_out = cs, cb, H * W
                    if wino:
                        continue
                    x3 = ops.x3_conv(dt, cin)
                    dense = ops.x3_tapdense(dt, cin, spec, row.op == "dgrad", epi, cout)
                    lib_mode = "f16" if f16 else "f16x2" if ops.h2_conv(x3, dense) else "bf16x3" if (x3 or dense) else "native"
                    dot = row.epi == "fuse" and hw_out % 256 == 0
                    lines.append(f"{row.name}-{mode} {row.op} {lib_mode} {int(dense)} {int(bool(epi))} {int(dot)} {B} {cb} {cs} {K} {s} {p} {H} {W}")
                finally:
                    for k, v in saved:
                        setattr(ops, k, v)
    finally:
        ops.get_fp32_mfma_mode = real_mode
    return lines


if __name__ == "__main__":
    out = case_lines()
    with open(os.path.join(HERE, "conv_route_cases.txt"), "w") as f:
        f.write("\n".join(out) + "\n")
    print(f"{len(out)} cases written")
