"""FLAME landmark-fit timing on one idle MI355X: the layers with and without the fused pose chain, and one iteration of
the fitter.  The loss of arms (a) - (d) is the sum of squares of landmarks2d; forward + backward to shape, expression and pose.
  (a) FlameLandmarkLayer(fused_chain=False) fwd + bwd     the path before fused_chain existed, unchanged
  (b) FlameLandmarkLayer(fused_chain=True)  fwd + bwd
  (c) FlameLayer(landmarks, fused_chain=False) fwd + bwd
  (d) FlameLayer(landmarks, fused_chain=True)  fwd + bwd
  (e) one FlameLandmarkFitter iteration (all groups moving): fused layer, gif_landmark_loss_f32, Adam
  (f) the same iteration with the unfused layer, project_landmarks and torch ops for the loss, the same Adam
Each figure is the median over `--calls` eager calls (after `--warmup`) of the time between two HIP events around one call, so it
includes the gaps the host leaves between the launches of a call; the arms alternate in one process and the second pass is
reported.  Conditions: (b) <= (a), (d) <= (c), (e) <= (f), (b) < (d).
Usage (GPU): python tools/fit_bench.py [--batch 32] [--vertices 5023] [--out profiles/flame_fit.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from flame_bench import median_ms, template  # noqa: E402


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
    assert torch.cuda.is_available(), "fit_bench needs an MI355X"
    from gif_amd import fitting, flame as fl
    B, V, ns, ne = a.batch, a.vertices, a.n_shape, a.n_exp
    model = fl.synthetic_flame_model(template(V), ns, ne)
    faces = np.load(os.path.join(ROOT, "tests", "golden", "body_mesh.npz"))["faces"].astype(np.int64)
    emb = fl.synthetic_landmark_embedding(faces[(faces < V).all(1)])
    layers = {(lean, fused): (fl.FlameLandmarkLayer(model, emb, ns, ne, fused_chain=fused) if lean else
                              fl.FlameLayer(model, ns, ne, landmarks=emb, fused_chain=fused)).cuda()
              for lean in (True, False) for fused in (False, True)}
    g = torch.Generator("cuda").manual_seed(0)
    r = lambda n, s: torch.randn(B, n, device="cuda", generator=g) * s
    shape, exp, pose = r(ns, 1.0), r(ne, 1.0), r(6, 0.3)
    leaves = [t.clone().requires_grad_(True) for t in (shape, exp, pose)]
    loss = lambda l2d: (l2d * l2d).sum()

    def layer_arm(lean, fused):
        layer, pick = layers[(lean, fused)], 0 if lean else 1
        return lambda: torch.autograd.grad(loss(layer(*leaves)[pick]), leaves)

    # the fitter: targets from the drawn parameters under a camera, the iteration timed away from the start
    fitter = fitting.FlameLandmarkFitter(model, emb, ns, ne, s0=4.0)
    cam = torch.tensor([[5.0, 0.01, -0.02]], device="cuda").repeat(B, 1)
    with torch.no_grad():
        target = fl.project_landmarks(layers[(True, False)](shape, exp, pose)[0], cam)[:, :, :2].contiguous()
    unfused = layers[(True, False)]

    def torch_loss(x, target2d, weight, rigid):
        l2d = unfused(x["shape"], x["expression"], x["pose"], x["neck_pose"], x["eye_pose"].detach())[0]
        p = fl.project_landmarks(l2d, x["cam"])[:, :, :2]
        per = ((p - target2d) ** 2).sum(2).sum(1)
        return per + fitter.reg_shape * (x["shape"] * x["shape"]).sum(1) + fitter.reg_exp * (x["expression"] * x["expression"]).sum(1)

    def fit_arm(loss_fn):
        x = fitter._start(B, None)
        opt = torch.optim.Adam([x[name] for name in fitter.GROUPS], lr=fitter.lr)
        return lambda: fitter.iterate(x, opt, target, None, False, None, loss_fn)

    arms = [("(a) FlameLandmarkLayer unfused fwd + bwd", layer_arm(True, False)), ("(b) FlameLandmarkLayer fused fwd + bwd", layer_arm(True, True)),
            ("(c) FlameLayer unfused fwd + bwd", layer_arm(False, False)), ("(d) FlameLayer fused fwd + bwd", layer_arm(False, True)),
            ("(e) fitter iteration", fit_arm(None)), ("(f) iteration, unfused layer + torch loss", fit_arm(torch_loss))]
    # same function: the fused arms' gradients against the unfused ones before anything is timed
    gd = [fn() for _, fn in arms[:4]]
    rel = lambda x, y: max(((p - q).norm() / q.norm()).item() for p, q in zip(x, y))
    g_diff = (rel(gd[1], gd[0]), rel(gd[3], gd[2]))
    res = {}
    for _ in range(2):  # two alternating passes; the second is reported (clocks and caches settled)
        for name, fn in arms:
            res[name] = median_ms(fn, a.calls, a.warmup)
    lines = [f"FLAME landmark fit, B = {B}, V = {V}, K = {ns + ne}, J = {len(unfused.parents)}, {len(emb.vertex_ids())} vertices named by "
             f"the tables; {torch.cuda.get_device_name(0)}",
             f"median of {a.calls} eager calls after {a.warmup} warm-up calls, HIP events around each call (10th .. 90th percentile)",
             f"gradients, fused against unfused: FlameLandmarkLayer {g_diff[0]:.2e}, FlameLayer {g_diff[1]:.2e}"]
    for name, _ in arms:
        m, lo, hi = res[name]
        lines.append(f"{name:46s} {m * 1e3:9.1f} us  ({lo * 1e3:.1f} .. {hi * 1e3:.1f})")
    ma, mb, mc, md, me, mf = (res[name][0] for name, _ in arms)
    lines.append(f"(a) / (b) = {ma / mb:.2f}x   (c) / (d) = {mc / md:.2f}x   (f) / (e) = {mf / me:.2f}x   (d) / (b) = {md / mb:.2f}x")
    ok = lambda c: "holds" if c else "FAILS"
    lines.append(f"condition (b) <= (a): {ok(mb <= ma)}; (d) <= (c): {ok(md <= mc)}; (e) <= (f): {ok(me <= mf)}; (b) < (d): {ok(mb < md)}")
    text = "\n".join(lines)
    print(text, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
