"""FLAME layer timing on one idle MI355X: gif_amd.flame.FlameLayer next to the float32 torch restatement of the same algorithm
(tests/flame_ref.py) on the same device and the same inputs.
  (a) FlameLayer forward, nothing requires a gradient      two launches: gif_flame_joints_f32, gif_flame_skin_f32
  (b) FlameLayer forward + backward to shape, expression and pose
  (c) the torch restatement, forward and forward + backward
Each figure is the median over `--calls` eager calls (after `--warmup`) of the time between two HIP events around one call, so
it includes the gaps the host leaves between the launches of a call — what a caller sees.  No speed-up is promised; the
condition to hold is (a) <= (c) forward and (b) <= (c) forward + backward.
Usage (GPU): python tools/flame_bench.py [--batch 32] [--vertices 5023] [--out profiles/flame_layer.txt]
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def template(V, seed=0):
    """The golden body mesh scaled to a head's size; more vertices than it has are drawn around it."""
    v = np.load(os.path.join(ROOT, "tests", "golden", "body_mesh.npz"))["vertices"].astype(np.float64) * 0.1
    if V > v.shape[0]:
        rng = np.random.RandomState(seed)
        v = np.concatenate([v, v[rng.randint(0, v.shape[0], V - v.shape[0])] + rng.randn(V - v.shape[0], 3) * 1e-3])
    return v[:V]


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--vertices", type=int, default=5023)
    ap.add_argument("--n-shape", type=int, default=100)
    ap.add_argument("--n-exp", type=int, default=50)
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "flame_bench needs an MI355X"
    import flame_ref
    from gif_amd import flame as fl
    B, V, ns, ne = a.batch, a.vertices, a.n_shape, a.n_exp
    model = fl.synthetic_flame_model(template(V), ns, ne)
    layer = fl.FlameLayer(model, ns, ne).cuda()
    c32 = flame_ref.constants(model, ns, ne, torch.float32, "cuda")
    g = torch.Generator("cuda").manual_seed(0)
    r = lambda n, s: torch.randn(B, n, device="cuda", generator=g) * s
    shape, exp, pose = r(ns, 1.0), r(ne, 1.0), r(6, 0.15)
    zero3, zero6 = torch.zeros(B, 3, device="cuda"), torch.zeros(B, 6, device="cuda")
    up = torch.randn(B, V, 3, device="cuda", generator=g)
    leaves = [t.clone().requires_grad_(True) for t in (shape, exp, pose)]

    def layer_fwd():
        with torch.no_grad():
            return layer(shape, exp, pose)[0]

    def layer_fwd_bwd():
        return torch.autograd.grad(layer(*leaves)[0], leaves, up)

    def torch_fwd():
        with torch.no_grad():
            return flame_ref.flame_vertices(c32, shape, exp, pose, zero3, zero6)

    def torch_fwd_bwd():
        return torch.autograd.grad(flame_ref.flame_vertices(c32, *leaves, zero3, zero6), leaves, up)

    # same function: the arms agree before they are timed
    ref = flame_ref.flame_vertices(flame_ref.constants(model, ns, ne, torch.float64, "cuda"), shape.double(), exp.double(),
                                   pose.double(), zero3.double(), zero6.double())
    err = lambda y: ((y.double() - ref).abs().max() / ref.abs().max()).item()
    e_layer, e_torch = err(layer_fwd()), err(torch_fwd())
    gl, gt = layer_fwd_bwd(), torch_fwd_bwd()
    g_diff = max(((x - y).norm() / y.norm()).item() for x, y in zip(gl, gt))
    arms = [("(a) FlameLayer forward, no grad", layer_fwd), ("(c) torch float32 forward, no grad", torch_fwd),
            ("(b) FlameLayer forward + backward", layer_fwd_bwd), ("(c) torch float32 forward + backward", torch_fwd_bwd)]
    res = {}
    for _ in range(2):  # two alternating passes; the second is reported (clocks and caches settled)
        for name, fn in arms:
            res[name] = median_ms(fn, a.calls, a.warmup)
    kp = layer.dirs.shape[0]
    lines = [f"FLAME layer, B = {B}, V = {V}, K = {ns + ne}, KP = {kp}, J = {len(layer.parents)}; {torch.cuda.get_device_name(0)}",
             f"median of {a.calls} eager calls after {a.warmup} warm-up calls, HIP events around each call (10th .. 90th percentile)",
             f"forward error vs float64: FlameLayer {e_layer:.2e}, torch float32 {e_torch:.2e}; gradients, layer vs torch: {g_diff:.2e}"]
    for name, _ in arms:
        m, lo, hi = res[name]
        lines.append(f"{name:40s} {m * 1e3:9.1f} us  ({lo * 1e3:.1f} .. {hi * 1e3:.1f})")
    fa, fc = res[arms[0][0]][0], res[arms[1][0]][0]
    ba, bc = res[arms[2][0]][0], res[arms[3][0]][0]
    lines.append(f"forward: torch / FlameLayer = {fc / fa:.2f}x   forward + backward: torch / FlameLayer = {bc / ba:.2f}x")
    lines.append(f"condition (a) <= (c) forward: {'holds' if fa <= fc else 'FAILS'}; (b) <= (c) forward + backward: "
                 f"{'holds' if ba <= bc else 'FAILS'}")
    text = "\n".join(lines)
    print(text, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
