"""Shaded condition timing on one idle MI355X: gif_amd.shading (sh_shade on gif_shade_sh_f32 / gif_shade_sh_bwd_f32) next to the
float32 torch restatement of the shading step (tests/shading_ref.py) in its place, on the same device and the same inputs.  The
rasteriser passes, the FLAME layer and the texture decode are the same launches in both arms.
  (a) render_shaded_condition forward, nothing requires a gradient
  (b) ShadedFlameConditionRenderer forward + backward to the labels [B,236] (straight_through=True; this asks for g_albedo)
  (c) the same two with the restatement in sh_shade's place
Each figure is the median over `--calls` eager calls (after `--warmup`) of the time between two HIP events around one call, so it
includes the gaps the host leaves between the launches of a call — what a caller sees.  No speed-up is promised; the condition to
hold is (a) <= (c) forward and (b) <= (c) forward + backward.
  --kernels N   instead: N calls each of sh_shade alone, forward + backward, in three configurations (no albedo gradient;
                per-sample albedo with its gradient; shared albedo with its gradient) on the renderer's own UV and normal images.
                Meant to run under `rocprofv3 --kernel-trace --stats`; `--trace FILE` then reads the kernel trace (.csv) back and
                prints the two kernels' times per configuration with algorithmic bytes / time.
Usage (GPU): python tools/shade_bench.py [--batch 32] [--size 256] [--tex 256] [--out profiles/shaded_render.txt]
"""
import argparse
import csv
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

CONFIGS = ("no albedo gradient (per-sample albedo)", "per-sample albedo with g_albedo", "shared albedo with g_albedo")


def mesh(V):
    """The golden body mesh scaled to a head's size, cut to its first V vertices and the faces among them."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "body_mesh.npz"))
    v, f = g["vertices"].astype(np.float64) * 0.1, g["faces"].astype(np.int64)
    V = min(V, v.shape[0])
    return v[:V], f[(f < V).all(1)]


def median_ms(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(calls)]
    for e0, e1 in ev:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    t = sorted(e0.elapsed_time(e1) for e0, e1 in ev)
    return statistics.median(t), t[len(t) // 10], t[-1 - len(t) // 10]


def read_trace(path, n, B, S, T, coverage):
    """Per configuration, the median duration of the two kernels over its n dispatches, in dispatch order."""
    rows = []
    with open(path, newline="") as fh:
        for r in csv.DictReader(fh):
            name = r.get("Kernel_Name", "")
            if "shade_sh" in name:
                rows.append((int(r["Start_Timestamp"]), "bwd" if "shade_sh_bwd" in name else "fwd",
                             (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
    rows.sort()
    lines = []
    for kind in ("fwd", "bwd"):
        t = [d for _, k, d in rows if k == kind]
        if len(t) < 3 * n:
            lines.append(f"{kind}: {len(t)} dispatches in the trace, {3 * n} expected: not measured")
            continue
        t = t[-3 * n:]  # (the agreement check in front of the timed calls dispatches first)
        for c, cfg in enumerate(CONFIGS):
            us = statistics.median(t[c * n:(c + 1) * n])
            px = B * S * S
            if kind == "fwd":
                by = px * 33
                lines.append(f"forward   {cfg:42s} {us:8.1f} us   {by / us / 1e6:6.2f} TB/s of 33 B/pixel (8 TB/s HBM)")
            else:
                by = px * 57  # reads uv 8, normal 12, mask 1, g_out 12; writes g_uv 12, g_nrm 12
                add = px * coverage * 48 if c else 0      # four taps x three channels x 4 bytes per covered pixel
                extra = f"; g_albedo adds {add / us / 1e6:5.2f} TB/s of ~1.3 TB/s atomic rate" if c else ""
                lines.append(f"backward  {cfg:42s} {us:8.1f} us   {by / us / 1e6:6.2f} TB/s of 57 B/pixel{extra}")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--tex", type=int, default=256)
    ap.add_argument("--vertices", type=int, default=5023)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--kernels", type=int, default=0)
    ap.add_argument("--trace", type=str, default=None)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "shade_bench needs an MI355X"
    import shading_ref
    from gif_amd import flame as fl
    from gif_amd import render
    from gif_amd import shading as sd
    from gif_amd.data import synthetic_flame_labels
    B, S, T = a.batch, a.size, a.tex
    v, f = mesh(a.vertices)
    layer = fl.FlameLayer(fl.synthetic_flame_model(v)).cuda()
    faces = torch.from_numpy(f).cuda()
    uvs = sd.synthetic_face_uvs(v, f).cuda()
    model = sd.synthetic_texture_model(T, 50)
    fb = synthetic_flame_labels(B, "cuda", torch.Generator("cuda").manual_seed(0), n_labels=236)
    fb[:, 156] = 8.0
    fb[:, 157:159] = torch.tensor([0.01, -0.01], device="cuda")
    fb[:, 209:236] *= 0.3
    fb[:, 209:212] += 2.5
    rnd = sd.ShadedFlameConditionRenderer(layer, faces, uvs, model, S, S, straight_through=True)
    with torch.no_grad():
        _, v_ndc, _ = rnd.vertices(fb)
        albedo, sh = rnd.appearance(fb)
        normal_img, mask = render.rasterize_attributes(v_ndc, faces, render.vertex_normals(v_ndc, faces) * 0.5 + 0.5, S, S)
        uv_img, _ = sd.rasterize_face_attributes(v_ndc, faces, torch.cat((uvs, uvs.new_zeros(uvs.shape[0], 3, 1)), 2), S, S)
    coverage = mask.float().mean().item()
    head = f"shaded condition, B = {B}, {S} x {S}, T = {T}, V = {v.shape[0]}, F = {f.shape[0]}, coverage {coverage:.2f}; " \
           f"{torch.cuda.get_device_name(0)}"

    if a.kernels or a.trace:
        n = a.kernels
        if a.trace:
            text = "\n".join([head, f"kernel times: median of {n} dispatches per configuration from a rocprofv3 kernel trace"]
                             + read_trace(a.trace, n, B, S, T, coverage))
        else:
            up = torch.randn(B, 3, S, S, device="cuda", generator=torch.Generator("cuda").manual_seed(1))
            for c in range(3):
                alb = (albedo[:1] if c == 2 else albedo).clone().requires_grad_(c > 0)
                x = [uv_img.clone().requires_grad_(True), normal_img.clone().requires_grad_(True), alb, sh.clone().requires_grad_(True)]
                for _ in range(n):
                    y = sd.sh_shade(x[0], x[1], mask, x[2], x[3], 2.0, -1.0)
                    torch.autograd.grad(y, [t for t in x if t.requires_grad], up)
                torch.cuda.synchronize()
            text = head + f"\n{n} sh_shade forward + backward calls per configuration done: " + "; ".join(CONFIGS)
    else:
        leaves = fb.clone().requires_grad_(True)
        up = torch.randn(B, 6, S, S, device="cuda", generator=torch.Generator("cuda").manual_seed(1))
        hip, ref32 = sd.sh_shade, shading_ref.sh_shade

        def fwd():
            with torch.no_grad():
                return sd.render_shaded_condition(v_ndc, faces, uvs, albedo, sh, S, S)

        def fwd_bwd():
            return torch.autograd.grad(torch.cat(rnd(leaves), 1), leaves, up)[0]

        def arm(fn, shade):
            def run():
                sd.sh_shade = shade
                try:
                    return fn()
                finally:
                    sd.sh_shade = hip
            return run

        arms = [("(a) render_shaded_condition forward, no grad", arm(fwd, hip)),
                ("(c) forward with the torch restatement", arm(fwd, ref32)),
                ("(b) labels -> condition forward + backward", arm(fwd_bwd, hip)),
                ("(c) forward + backward with the restatement", arm(fwd_bwd, ref32))]
        # same function: the arms agree before they are timed
        diff_img = (arms[0][1]() != arms[1][1]()).float().mean().item()
        ga, gc = arms[2][1](), arms[3][1]()
        diff_g = ((ga - gc).norm() / gc.norm()).item()
        res = {}
        for _ in range(2):  # two alternating passes; the second is reported (clocks and caches settled)
            for name, fn in arms:
                res[name] = median_ms(fn, a.calls, a.warmup)
        lines = [head, f"median of {a.calls} eager calls after {a.warmup} warm-up calls, HIP events around each call (10th .. 90th percentile)",
                 f"arms agree: {diff_img:.2e} of the quantised condition's values differ; label gradients differ by {diff_g:.2e} (relative)"]
        for name, _ in arms:
            m, lo, hi = res[name]
            lines.append(f"{name:46s} {m * 1e3:9.1f} us  ({lo * 1e3:.1f} .. {hi * 1e3:.1f})")
        fa, fc = res[arms[0][0]][0], res[arms[1][0]][0]
        ba, bc = res[arms[2][0]][0], res[arms[3][0]][0]
        lines.append(f"forward: restatement / sh_shade = {fc / fa:.2f}x   forward + backward: restatement / sh_shade = {bc / ba:.2f}x")
        lines.append(f"condition (a) <= (c) forward: {'holds' if fa <= fc else 'FAILS'}; (b) <= (c) forward + backward: "
                     f"{'holds' if ba <= bc else 'FAILS'}")
        text = "\n".join(lines)
    print(text, flush=True)
    if a.out:
        with open(a.out, "a" if a.trace else "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
