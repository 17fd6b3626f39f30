"""FLAME landmark timing on one idle MI355X: the landmark outputs of gif_amd.flame next to the float32 torch restatement of the
same definition (tests/flame_landmarks_ref.py over tests/flame_ref.py) on the same device and the same inputs.  The loss of every
arm is the sum of squares of landmarks2d; forward + backward to shape, expression and pose.
  (a) FlameLayer(landmarks=...)      all V vertices skinned, the landmark kernels on top
  (b) FlameLandmarkLayer             only the vertices the tables name are skinned
  (c) the torch restatement
  (d) the landmark step alone on given vertices and transforms, forward + backward to the vertices: the two kernels against their
      torch restatement (atan2, round, two index_selects, two gathers)
Each figure is the median over `--calls` eager calls (after `--warmup`) of the time between two HIP events around one call, so
it includes the gaps the host leaves between the launches of a call.  Conditions: (b) <= (a), (a) <= (c), (d) kernels <= restatement.
Usage (GPU): python tools/landmark_bench.py [--batch 32] [--vertices 5023] [--out profiles/flame_landmarks.txt]
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
    assert torch.cuda.is_available(), "landmark_bench needs an MI355X"
    import flame_landmarks_ref as lref
    import flame_ref
    from gif_amd import flame as fl
    B, V, ns, ne = a.batch, a.vertices, a.n_shape, a.n_exp
    model = fl.synthetic_flame_model(template(V), ns, ne)
    faces = np.load(os.path.join(ROOT, "tests", "golden", "body_mesh.npz"))["faces"].astype(np.int64)
    emb = fl.synthetic_landmark_embedding(faces[(faces < V).all(1)])
    full = fl.FlameLayer(model, ns, ne, landmarks=emb).cuda()
    lean = fl.FlameLandmarkLayer(model, emb, ns, ne).cuda()
    c32, t32 = flame_ref.constants(model, ns, ne, torch.float32, "cuda"), lref.tables(emb, torch.float32, "cuda")
    g = torch.Generator("cuda").manual_seed(0)
    r = lambda n, s: torch.randn(B, n, device="cuda", generator=g) * s
    shape, exp, pose = r(ns, 1.0), r(ne, 1.0), r(6, 0.3)
    zero3, zero6 = torch.zeros(B, 3, device="cuda"), torch.zeros(B, 6, device="cuda")
    leaves = [t.clone().requires_grad_(True) for t in (shape, exp, pose)]
    loss = lambda l2d: (l2d * l2d).sum()

    def layer_arm(layer, pick):
        return lambda: torch.autograd.grad(loss(layer(*leaves)[pick]), leaves)

    def torch_arm():
        return torch.autograd.grad(loss(lref.flame_landmarks(c32, t32, *leaves, zero3, zero6)[1]), leaves)

    # (d): vertices and transforms as the layer produces them, landmark step alone
    with torch.no_grad():
        verts0, A0 = full._forward_nograd(B, [shape, exp, pose, None, None])
    verts_leaf = verts0.clone().requires_grad_(True)
    yaw_joint, R, Ld, Ls, Lf = full._lmk
    tabs = (full.lmk_dyn_vid, full.lmk_dyn_bary, full.lmk_st_vid, full.lmk_st_bary)

    def step_kernels():
        lmk = fl._FlameLandmarksFn.apply(verts_leaf, A0, yaw_joint, R, Ld, Ls + Lf, *tabs)[0]
        return torch.autograd.grad(loss(lmk[:, :Ld + Ls]), verts_leaf)

    def step_torch():
        Rw = A0.view(B, -1, 3, 4)[:, yaw_joint, :, :3]
        return torch.autograd.grad(loss(lref.landmarks_of(t32, verts_leaf, Rw)[0]), verts_leaf)

    # same function: the arms agree before they are timed
    c64, t64 = flame_ref.constants(model, ns, ne, torch.float64, "cuda"), lref.tables(emb, torch.float64, "cuda")
    ref = lref.flame_landmarks(c64, t64, shape.double(), exp.double(), pose.double(), zero3.double(), zero6.double())
    err = lambda y: ((y.double() - ref[1]).abs().max() / ref[1].abs().max()).item()
    with torch.no_grad():
        e_full, e_lean = err(full(shape, exp, pose)[1]), err(lean(shape, exp, pose)[0])
        e_torch = err(lref.flame_landmarks(c32, t32, shape, exp, pose, zero3, zero6)[1])
    arms = [("(a) FlameLayer(landmarks) fwd + bwd", layer_arm(full, 1)), ("(b) FlameLandmarkLayer fwd + bwd", layer_arm(lean, 0)),
            ("(c) torch float32 fwd + bwd", torch_arm), ("(d) landmark kernels fwd + bwd", step_kernels),
            ("(d) torch float32 landmark step", step_torch)]
    gd = [fn() for _, fn in arms]
    rel = lambda x, y: max(((p - q).norm() / q.norm()).item() for p, q in zip(x, y))
    g_diff = (rel(gd[0], gd[2]), rel(gd[1], gd[2]), rel(gd[3], gd[4]))
    res = {}
    for _ in range(2):  # two alternating passes; the second is reported (clocks and caches settled)
        for name, fn in arms:
            res[name] = median_ms(fn, a.calls, a.warmup)
    lines = [f"FLAME landmarks, B = {B}, V = {V}, K = {ns + ne}, J = {len(full.parents)}, R = {R}, Ld = {Ld}, Ls = {Ls}, Lf = {Lf}, "
             f"{len(emb.vertex_ids())} vertices named by the tables; {torch.cuda.get_device_name(0)}",
             f"median of {a.calls} eager calls after {a.warmup} warm-up calls, HIP events around each call (10th .. 90th percentile)",
             f"landmarks2d error vs float64: FlameLayer {e_full:.2e}, FlameLandmarkLayer {e_lean:.2e}, torch float32 {e_torch:.2e}; "
             f"gradients vs torch: (a) {g_diff[0]:.2e}, (b) {g_diff[1]:.2e}, (d) {g_diff[2]:.2e}"]
    for name, _ in arms:
        m, lo, hi = res[name]
        lines.append(f"{name:40s} {m * 1e3:9.1f} us  ({lo * 1e3:.1f} .. {hi * 1e3:.1f})")
    ma, mb, mc, mdk, mdt = (res[name][0] for name, _ in arms)
    lines.append(f"(a) / (b) = {ma / mb:.2f}x   (c) / (a) = {mc / ma:.2f}x   (d) torch / kernels = {mdt / mdk:.2f}x")
    ok = lambda c: "holds" if c else "FAILS"
    lines.append(f"condition (b) <= (a): {ok(mb <= ma)}; (a) <= (c): {ok(ma <= mc)}; (d) kernels <= restatement: {ok(mdk <= mdt)}")
    text = "\n".join(lines)
    print(text, flush=True)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
