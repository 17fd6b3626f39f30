"""The FLAME layer's kernels (gif_flame_joints_f32, gif_flame_skin_f32, gif_flame_skin_bwd_f32) against the float64 restatement
of the algorithm in tests/flame_ref.py, at the sizes where they can go wrong:
  V in {1, 33, 257, 5023}   a partial vertex tile (16 / 32 / 64 vertices per workgroup), one workgroup vs many in the reductions
  B in {1, 3, 33}           33 crosses the 32-sample chunk and leaves a chunk with one busy wave
  (n_shape, n_exp)          (7, 5): KP = 48 / 30; (100, 50): KP = 186 / 168, three 64-column passes; (300, 100): KP = 436, seven
  J = 5 (FLAME's parents) and J = 3 as the chain [-1, 0, 1]; neck and eye poses non-zero; one sample with an all-zero pose
  (Rodrigues at its 1e-8 guard).  The ends of the chain lengths the kernels take: J = 1 (no pose feature, KP == K, an empty
  R[:, 1:]), J = 2 (the neck is the last joint) and J = 8 (kMaxJ; joints past the fifth do not rotate).

Bound, forward and backward alike:  err <= M * err32 + 2^-23,  err32 = the same metric for the float32 restatement on the CPU
with the same inputs (forward: max|got - ref| / max|ref|; backward: Frobenius, per parameter group).  M = 4.  It started at 8
(a kernel adding up to 436 terms one after the other, against torch's blocked sums: a random-walk estimate of 2-3x the
restatement's error, with a factor of about 3 on top) and the first measurement of that kernel gave up to 4.7x at KP = 436; the
kernel now sums each 64-column pass on its own (blocked, like the restatement), every case measures below 2, and M is 4.
MEASURED err / err32 on an MI355X (`pytest -s` prints them; forward: no-grad path / grad path; backward: worst parameter group):
  case             forward        backward
  v1_b1            0.57 / 0.14    1.03 (shape)
  v33_b3_chain     0.70 / 0.70    1.27 (shape)
  v33_b33_k400     0.76 / 0.79    1.01 (expression)
  v257_b3          1.00 / 1.00    0.57 (shape)
  v257_b33_chain   0.89 / 0.88    0.77 (shape)
  v5023_b1         0.53 / 0.52    0.23 (neck)
  v5023_b33        0.73 / 0.73    0.65 (shape)
  v33_b3_j1        1.00 / 1.00    1.39 (expression)
  v33_b33_j2       0.92 / 0.93    1.29 (shape)
  v257_b3_j8       0.81 / 1.22    0.47 (shape)
err32 itself: 1.5e-7 .. 4.3e-7 forward; 8.6e-8 .. 1.1e-6 for shape / expression and 4.1e-7 .. 1.7e-5 for the poses backward (the
largest at V = 1, where one vertex carries the whole cancellation).
"""
import os

import numpy as np
import pytest
import torch

import flame_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M = 4
FLOOR = 2.0 ** -23
GROUPS = ("shape_params", "expression_params", "pose_params", "neck_pose", "eye_pose")
# (V, B, (n_shape, n_exp), parents)
FLAME, CHAIN = (-1, 0, 1, 1, 1), (-1, 0, 1)
CASES = {
    "v1_b1": (1, 1, (7, 5), FLAME),
    "v33_b3_chain": (33, 3, (7, 5), CHAIN),
    "v33_b33_k400": (33, 33, (300, 100), FLAME),
    "v257_b3": (257, 3, (7, 5), FLAME),
    "v257_b33_chain": (257, 33, (100, 50), CHAIN),
    "v5023_b1": (5023, 1, (7, 5), FLAME),
    "v5023_b33": (5023, 33, (100, 50), FLAME),
    # the ends of the chain lengths the kernels take (J in 1..8; joints past the fifth do not rotate)
    "v33_b3_j1": (33, 3, (7, 5), (-1,)),              # no pose feature (KP == K), an empty R[:, 1:]
    "v33_b33_j2": (33, 33, (7, 5), (-1, 0)),          # the neck is the last joint
    "v257_b3_j8": (257, 3, (7, 5), (-1, 0, 1, 1, 1, 0, 5, 2)),  # kMaxJ: three joints that do not rotate, 96 floats of A per sample
}


def body():
    g = np.load(os.path.join(ROOT, "tests", "golden", "body_mesh.npz"))
    return g["vertices"].astype(np.float64) * 0.1, g["faces"].astype(np.int64)


def rel_max(got, ref):
    return ((got.double().cpu() - ref).abs().max() / ref.abs().max()).item()


def times(e, e32):
    return e / max(e32, 1e-30)


def rel_fro(got, ref):
    return ((got.double().cpu() - ref).norm() / ref.norm()).item()


_cache = {}


def case(name):
    """Model, inputs, upstream gradient and the CPU results (float64 reference, float32 yardstick) of a case: computed once,
    shared by the tests, never modified."""
    if name in _cache:
        return _cache[name]
    from gif_amd import flame as fl
    V, B, (ns, ne), parents = CASES[name]
    model = fl.synthetic_flame_model(body()[0][:V], ns, ne, seed=V + B, parents=parents)
    g = torch.Generator().manual_seed(1000 + V + B)
    r = lambda n, s: torch.randn(B, n, generator=g) * s
    inputs = [r(ns, 1.0), r(ne, 1.0), r(6, 0.15), r(3, 0.15), r(6, 0.15)]
    if B > 1:
        for t in inputs[2:]:
            t[1] = 0  # one sample with an all-zero pose
    up = torch.randn(B, V, 3, generator=g)
    out = {"model": model, "layer_args": (ns, ne), "inputs": inputs, "up": up}
    for dt in (torch.float64, torch.float32):
        c = flame_ref.constants(model, ns, ne, dt)
        x = [t.to(dt, copy=True).requires_grad_(True) for t in inputs]  # (a copy: the shared inputs stay plain tensors)
        v = flame_ref.flame_vertices(c, *x)
        grads = torch.autograd.grad(v, x, up.to(dt))
        out[dt] = (v.detach(), [t.detach() for t in grads])
    ref, ref_g = out[torch.float64]
    y32, y32_g = out[torch.float32]
    out["err32"] = rel_max(y32, ref)
    out["err32_g"] = [rel_fro(a, b) for a, b in zip(y32_g, ref_g)]
    _cache[name] = out
    return out


def layer_of(c):
    from gif_amd import flame as fl
    return fl.FlameLayer(c["model"], *c["layer_args"]).cuda()


def run_grad(layer, inputs, up, which=range(5)):
    x = [t.cuda().requires_grad_(i in which) for i, t in enumerate(inputs)]
    v = layer(*x)[0]
    grads = torch.autograd.grad(v, [x[i] for i in which], up.cuda())
    return v.detach(), dict(zip(which, grads))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_forward_matches_float64_reference(name):
    c = case(name)
    layer = layer_of(c)
    ref = c[torch.float64][0]
    bound = M * c["err32"] + FLOOR
    with torch.no_grad():
        fast = layer(*[t.cuda() for t in c["inputs"]])[0]  # joints kernel + skin kernel
    slow = run_grad(layer, c["inputs"], c["up"])[0]         # torch joints + skin kernel
    e_fast, e_slow, e_pair = rel_max(fast, ref), rel_max(slow, ref), rel_max(fast, slow.double().cpu())
    print(f"\n[flame fwd] {name}: err32 {c['err32']:.2e}  no-grad path {e_fast:.2e} (x{times(e_fast, c['err32']):.2f})  "
          f"grad path {e_slow:.2e} (x{times(e_slow, c['err32']):.2f})  between the paths {e_pair:.2e}")
    assert fast.shape == ref.shape and torch.isfinite(fast).all()
    assert e_fast <= bound, f"no-grad path: {e_fast:.3e} > {bound:.3e}"
    assert e_slow <= bound, f"grad path: {e_slow:.3e} > {bound:.3e}"
    assert e_pair <= bound, f"the two paths differ by {e_pair:.3e} > {bound:.3e}"


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_backward_matches_float64_autograd(name):
    c = case(name)
    grads = run_grad(layer_of(c), c["inputs"], c["up"])[1]
    ref_g = c[torch.float64][1]
    msgs, bad = [], []
    for i, group in enumerate(GROUPS):
        if ref_g[i].norm().item() == 0:  # (the eye poses of a 3-joint chain move nothing)
            assert grads[i].abs().max().item() == 0
            continue
        e, e32 = rel_fro(grads[i], ref_g[i]), c["err32_g"][i]
        msgs.append(f"{group} {e:.2e} (err32 {e32:.2e}, x{times(e, e32):.2f})")
        if not e <= M * e32 + FLOOR:
            bad.append(f"{group}: {e:.3e} > {M * e32 + FLOOR:.3e}")
    print(f"\n[flame bwd] {name}: " + "  ".join(msgs))
    assert not bad, "; ".join(bad)


@pytest.mark.gpu
def test_two_runs_give_identical_bits():
    c = case("v5023_b33")
    layer = layer_of(c)
    runs = []
    for _ in range(2):
        with torch.no_grad():
            fast = layer(*[t.cuda() for t in c["inputs"]])[0]
        slow, grads = run_grad(layer, c["inputs"], c["up"])
        runs.append([fast, slow] + [grads[i] for i in range(5)])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["v33_b3_chain", "v5023_b33"])
def test_optional_outputs(name):
    """A subset of the inputs requiring a gradient gives the same values as all of them; at the entry point, either output
    pointer of the backward may be null, and so may the forward's v_posed."""
    from gif_amd import flame as fl
    c = case(name)
    layer = layer_of(c)
    verts, full = run_grad(layer, c["inputs"], c["up"])
    for which in ((2,), (0,)):  # pose_params alone, shape_params alone
        v, part = run_grad(layer, c["inputs"], c["up"], which)
        assert torch.equal(v, verts)
        assert torch.equal(part[which[0]], full[which[0]])
    # the autograd Function directly: g_coef alone (g_A = NULL), g_A alone (g_coef = NULL), neither (v_posed = NULL)
    B, (V, J), KP = c["up"].shape[0], layer.lbs_weights.shape, layer.dirs.shape[0]
    g = torch.Generator().manual_seed(5)
    coef = (torch.randn(B, KP, generator=g) * 0.1).cuda()
    A = (torch.eye(3, 4).reshape(1, 1, 12) + 0.1 * torch.randn(B, J, 12, generator=g)).cuda()
    consts = (layer.v_template, layer.dirs, layer.lbs_weights)
    up = c["up"].cuda()

    def run(need_c, need_a):
        x, y = coef.clone().requires_grad_(need_c), A.clone().requires_grad_(need_a)
        v = fl._FlameSkinFn.apply(x, y, *consts)
        if need_c or need_a:
            v.backward(up)
        return v.detach(), x.grad, y.grad

    v_both, gc, ga = run(True, True)
    v_c, gc_only, none_a = run(True, False)
    v_a, none_c, ga_only = run(False, True)
    v_none, _, _ = run(False, False)
    assert none_a is None and none_c is None
    assert torch.equal(gc, gc_only) and torch.equal(ga, ga_only)
    assert torch.equal(v_both, v_c) and torch.equal(v_both, v_a) and torch.equal(v_both, v_none)
    # and those gradients are the right ones: the skinning alone, in float64
    cd, Ad = coef.double().cpu().requires_grad_(True), A.double().cpu().requires_grad_(True)
    vp = (layer.v_template.double().cpu() + cd @ layer.dirs.double().cpu()).view(B, V, 3)
    T = torch.einsum("vj,bjrc->bvrc", layer.lbs_weights.double().cpu(), Ad.view(B, J, 3, 4))
    ref = torch.einsum("bvrc,bvc->bvr", T, torch.cat([vp, vp.new_ones(B, V, 1)], 2))
    rc, ra = torch.autograd.grad(ref, (cd, Ad), c["up"].double())
    # fp32 sums of up to 3 V = 15069 terms in blocks of 96 / 64 and then over the blocks: sqrt(n) 2^-24 ~ 7e-6 at the very worst
    assert rel_max(v_both, ref.detach()) <= 1e-5 and rel_fro(gc, rc) <= 1e-5 and rel_fro(ga, ra) <= 1e-5


@pytest.mark.gpu
def test_flame_layer_drives_the_condition_renderer():
    """flame_batch [N,159] -> condition with no stand-in: finite, covers pixels, and with straight_through=True every slice of the
    labels (shape, expression, pose, camera) receives a finite non-zero gradient; none with the default floor quantisation."""
    from gif_amd import flame as fl
    from gif_amd import render
    from gif_amd.data import synthetic_flame_labels
    v, f = body()
    layer = fl.FlameLayer(fl.synthetic_flame_model(v)).cuda()
    ft = torch.from_numpy(f).cuda()
    tex = torch.rand(v.shape[0], 3, device="cuda", generator=torch.Generator("cuda").manual_seed(0))
    fb = synthetic_flame_labels(2, "cuda", torch.Generator("cuda").manual_seed(1))
    fb[:, 156] = 8.0  # camera scale: the 0.1-sized template fills most of the image ...
    fb[:, 157:159] = torch.tensor([0.01, -0.01], device="cuda")  # ... around its centre (the labels' shift suits a unit-sized head)
    fb.requires_grad_(True)
    rend, nrm = render.FlameConditionRenderer(layer, ft, tex, 64, 64, straight_through=True)(fb)
    assert rend.shape == (2, 3, 64, 64) and nrm.shape == (2, 3, 64, 64)
    assert torch.isfinite(rend).all() and torch.isfinite(nrm).all()
    assert (nrm != -1).any(1).float().mean().item() > 0.05  # covered pixels (the background renders as -1)
    up = torch.randn(rend.shape, device="cuda", generator=torch.Generator("cuda").manual_seed(2))
    ((rend + nrm) * up).sum().backward()
    assert torch.isfinite(fb.grad).all()
    for lo, hi in ((0, 100), (100, 150), (150, 156), (156, 159)):
        assert fb.grad[:, lo:hi].abs().sum().item() > 0, (lo, hi)
    fb.grad = None
    rend, nrm = render.FlameConditionRenderer(layer, ft, tex, 64, 64)(fb)  # default: floor quantisation, zero gradient
    ((rend + nrm) * up).sum().backward()
    assert torch.all(fb.grad == 0)
    with torch.no_grad():  # the no-grad path (two launches) renders the same condition
        rend2, _ = render.FlameConditionRenderer(layer, ft, tex, 64, 64)(fb.detach())
    assert (rend2 != rend).float().mean().item() < 0.01  # (a vertex moving by an ulp may flip a pixel's quantisation step)
