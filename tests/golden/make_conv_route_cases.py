"""Generates tests/golden/conv_route_cases.txt: for every fwd / dgrad row of tests/test_gpu_conv_routes.ROWS in every mode it lists, the
library call gif_amd/ops.py makes for it when the call ends in csrc/conv_igemm.hip (rows that take the Winograd route are left out), one
line per case:
    <row>-<mode>  fwd|dgrad  native|bf16x3|f16x2|f16  dense scaled dot  B Cin Cout K stride pad H W
(the forward convolution, channel counts as the activations carry them; dense / scaled / dot: tap-dense entry point, per-sample input
scales, dot fusion).  The decision is ops.conv_plan, the function conv_fwd and conv_bwd_data ask themselves; it is pure Python: no GPU and
no library is needed.  tests/host/conv_route_dump.cpp reads the file; tests/test_conv_route.py checks that it is current.
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
                    cin, cout, hw_out = (cb, cs, Hs * Ws) if row.op == "fwd" else (cs, cb, H * W)
                    plan = ops.conv_plan(row.op, dt, B, spec, (H, W), (Hs, Ws), cin, cout, epi)
                    if plan.route == "winograd":
                        continue
                    dot = row.epi == "fuse" and hw_out % 256 == 0
                    lines.append(f"{row.name}-{mode} {row.op} {plan.mode} {int(plan.dense)} {int(bool(epi))} {int(dot)} {B} {cb} {cs} {K} {s} {p} {H} {W}")
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
