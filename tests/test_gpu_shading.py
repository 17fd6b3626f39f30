"""The shaded condition's kernels (gif_shade_sh_f32, gif_shade_sh_bwd_f32 behind gif_amd.shading.sh_shade) and the pipeline around
them against the float64 restatement in tests/shading_ref.py.  Cases (B, Ba, H, W, T), inputs from shading_ref.make_case:
  one_pixel        (1,1,1,1,1)       the smallest possible shape
  5x7_t2           (1,1,5,7,2)       a non-square image, T = 2
  shared_33x65_t3  (3,1,33,65,3)     one albedo accumulating over the batch; partial workgroups (forward 256, backward 1024 pixels)
  64x64_t257       (3,3,64,64,257)   T not a power of two; four backward workgroups per sample
  16x300_t16       (2,2,16,300,16)   a row longer than a workgroup; H * W no multiple of 256

Bound, the rule of tests/test_gpu_flame.py:  err <= 4 * err32 + 2^-23,  err32 = the same metric for the float32 restatement on the
CPU with the same inputs (forward: max|got - ref| / max|ref|; each of the four gradients: relative Frobenius).
MEASURED err / err32 on an MI355X (`pytest -s` prints them; profiles/shaded_render.txt has the run):
  case             forward   g_uv   g_normal   g_albedo   g_sh
  one_pixel        1.00      1.00   0.58       1.00       1.00
  5x7_t2           0.75      0.90   1.17       0.74       0.65
  shared_33x65_t3  0.90      1.00   0.97       1.22       0.37    (g_albedo: 1.29 in a second run — float atomics)
  64x64_t257       1.00      1.00   1.00       1.00       0.95
  16x300_t16       1.00      1.00   0.99       1.02       0.31
  edges (forward)  0.81
  pipeline         images 0 / 0 (no value differs in any of the three runs); g_vertices 0.96; g_albedo 1.00; g_sh 0.52
err32 itself: forward 4.0e-8 .. 1.2e-5 (it grows with T: the texel position costs T 2^-24), gradients 2.0e-8 .. 1.3e-5.  Every case
measures below 2.
"""
import os

import numpy as np
import pytest
import torch

import shading_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M = 4
FLOOR = 2.0 ** -23
GROUPS = ("uv", "normal", "albedo", "sh")


def rel_max(got, ref):
    return ((got.double().cpu() - ref).abs().max() / ref.abs().max()).item()


def rel_fro(got, ref):
    return ((got.double().cpu() - ref).norm() / ref.norm()).item()


def times(e, e32):
    return e / max(e32, 1e-30)


_cache = {}


def case(name):
    """Inputs, upstream gradient and the CPU results (float64 reference, float32 yardstick) of a case: computed once, shared by
    the tests, never modified."""
    if name in _cache:
        return _cache[name]
    uv, nrm, mask, albedo, sh, up, _ = shading_ref.make_case(*shading_ref.CASES[name])
    out = {"inputs": (uv, nrm, mask, albedo, sh), "up": up}
    for dt in (torch.float64, torch.float32):
        x = [t.to(dt, copy=True).requires_grad_(True) for t in (uv, nrm, albedo, sh)]
        y = shading_ref.sh_shade(x[0], x[1], mask, x[2], x[3])
        out[dt] = (y.detach(), [g.detach() for g in torch.autograd.grad(y, x, up.to(dt))])
    ref, ref_g = out[torch.float64]
    out["err32"] = rel_max(out[torch.float32][0], ref)
    out["err32_g"] = [rel_fro(a, b) for a, b in zip(out[torch.float32][1], ref_g)]
    _cache[name] = out
    return out


def run(inputs, up, which=(0, 1, 2, 3), scale=(1.0, 0.0)):
    """sh_shade on the device with the operands in `which` (of uv, normal, albedo, sh) requiring a gradient."""
    from gif_amd import shading as sd
    uv, nrm, mask, albedo, sh = [t.cuda() for t in inputs]
    x = [t.requires_grad_(i in which) for i, t in enumerate((uv, nrm, albedo, sh))]
    y = sd.sh_shade(x[0], x[1], mask, x[2], x[3], *scale)
    grads = torch.autograd.grad(y, [x[i] for i in which], up.cuda()) if which else ()
    return y.detach(), dict(zip(which, grads))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(shading_ref.CASES))
def test_forward_and_gradients_match_float64(name):
    c = case(name)
    ref, ref_g = c[torch.float64]
    y, grads = run(c["inputs"], c["up"])
    e = rel_max(y, ref)
    msgs, bad = [f"forward {e:.2e} (err32 {c['err32']:.2e}, x{times(e, c['err32']):.2f})"], []
    assert y.shape == ref.shape and torch.isfinite(y).all()
    if not e <= M * c["err32"] + FLOOR:
        bad.append(f"forward: {e:.3e} > {M * c['err32'] + FLOOR:.3e}")
    for i, group in enumerate(GROUPS):
        assert grads[i].shape == ref_g[i].shape and grads[i].dtype == torch.float32
        if ref_g[i].norm().item() == 0:
            assert grads[i].abs().max().item() == 0
            continue
        e, e32 = rel_fro(grads[i], ref_g[i]), c["err32_g"][i]
        msgs.append(f"g_{group} {e:.2e} (err32 {e32:.2e}, x{times(e, e32):.2f})")
        if not e <= M * e32 + FLOOR:
            bad.append(f"g_{group}: {e:.3e} > {M * e32 + FLOOR:.3e}")
    print(f"\n[shade] {name}: " + "  ".join(msgs))
    assert grads[0][:, 2].abs().max().item() == 0  # channel 2 of g_uv is written 0
    assert not bad, "; ".join(bad)


@pytest.mark.gpu
def test_forward_at_the_edges():
    """Values only (the function is continuous there): grid coordinates exactly -1 and +1, on texel centres, and beyond
    +-(1 + 2/T), where the output is exactly 0 — as it is for a coordinate that is not finite.  T = 8: every coordinate and texel
    position is exact in float32 and float64 alike."""
    from gif_amd import shading as sd
    T = 8
    inside = [-1.0, 1.0] + [(2 * i + 1) / T - 1 for i in range(T)] + [-1 - 0.5 / T, 1 + 0.5 / T, 0.25]
    beyond = [-(1 + 2.0 / T), 1 + 2.0 / T, -3.0, 3.0]
    g = torch.Generator().manual_seed(3)
    albedo = torch.rand(1, 3, T, T, generator=g)
    sh = torch.randn(1, 9, 3, generator=g)
    sh[:, 0] += 2.5

    def grid(coords):
        n = len(coords)
        c = torch.tensor(coords, dtype=torch.float32)
        uv = torch.stack([c[None, :].expand(n, n), c[:, None].expand(n, n), torch.zeros(n, n)])[None]
        d = torch.randn(1, 3, n, n, generator=g)
        return uv, d / d.norm(dim=1, keepdim=True), torch.ones(1, 1, n, n, dtype=torch.bool)

    uv, nrm, mask = grid(inside + beyond)
    ref = shading_ref.sh_shade(uv.double(), nrm.double(), mask, albedo.double(), sh.double())
    e32 = rel_max(shading_ref.sh_shade(uv, nrm, mask, albedo, sh), ref)
    got = sd.sh_shade(uv.cuda(), nrm.cuda(), mask.cuda(), albedo.cuda(), sh.cuda())
    e = rel_max(got, ref)
    print(f"\n[shade] edges: forward {e:.2e} (err32 {e32:.2e}, x{times(e, e32):.2f})")
    assert e <= M * e32 + FLOOR
    k = len(inside)
    assert (ref[:, :, :k, :k] != 0).all()  # (every tap of those cells carries weight somewhere)
    assert torch.all(got[:, :, k:, :] == 0) and torch.all(got[:, :, :, k:] == 0)
    uv, nrm, mask = grid(inside + [float("nan"), float("inf"), -float("inf"), 1e30, -1e30])
    got = sd.sh_shade(uv.cuda(), nrm.cuda(), mask.cuda(), albedo.cuda(), sh.cuda())
    assert torch.all(got[:, :, k:, :] == 0) and torch.all(got[:, :, :, k:] == 0) and torch.isfinite(got).all()


@pytest.mark.gpu
def test_normal_scale_and_offset():
    """nrm_mul / nrm_add = (2, -1) on the [0,1]-mapped normal image against (1, 0) on the mapped-back one: 2 x is exact, so both
    round 2 x - 1 once — the same bits forward; the normal's gradient carries the factor 2."""
    c = case("16x300_t16")
    uv, nrm, mask, albedo, sh = c["inputs"]
    n01 = nrm * 0.5 + 0.5
    y1, g1 = run((uv, 2 * n01 - 1, mask, albedo, sh), c["up"], which=(1,))
    y2, g2 = run((uv, n01, mask, albedo, sh), c["up"], which=(1,), scale=(2.0, -1.0))
    assert torch.equal(y1, y2)
    assert torch.equal(g2[1], 2 * g1[1])


@pytest.mark.gpu
def test_all_background_gives_exact_zeros():
    c = case("shared_33x65_t3")
    uv, nrm, mask, albedo, sh = c["inputs"]
    y, grads = run((uv, nrm, torch.zeros_like(mask), albedo, sh), c["up"])
    assert torch.all(y == 0)
    for i in range(4):
        assert torch.all(grads[i] == 0), GROUPS[i]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["shared_33x65_t3", "16x300_t16"])
def test_optional_outputs_and_determinism(name):
    """Every single-output backward gives the bits of the all-outputs backward for g_uv, g_nrm, g_sh (g_albedo, summed with float
    atomics, stays within the bound of the float64 reference in both); two runs give identical out, g_uv, g_nrm, g_sh; the no-grad
    forward equals the grad-path forward."""
    c = case(name)
    ref_alb, e32_alb = c[torch.float64][1][2], c["err32_g"][2]
    y, full = run(c["inputs"], c["up"])
    y2, again = run(c["inputs"], c["up"])
    assert torch.equal(y, y2)
    for i in (0, 1, 3):
        assert torch.equal(full[i], again[i]), GROUPS[i]
        yi, part = run(c["inputs"], c["up"], which=(i,))
        assert torch.equal(yi, y) and torch.equal(part[i], full[i]), GROUPS[i]
    _, alone = run(c["inputs"], c["up"], which=(2,))
    for g in (full[2], again[2], alone[2]):
        assert rel_fro(g, ref_alb) <= M * e32_alb + FLOOR
    with torch.no_grad():
        y0, _ = run(c["inputs"], c["up"], which=())
    assert torch.equal(y0, y)


def body():
    g = np.load(os.path.join(ROOT, "tests", "golden", "body_mesh.npz"))
    return g["vertices"].astype(np.float64) * 0.1, g["faces"].astype(np.int64)


def two_views(v):
    """The body mesh filling most of the image (y flipped like the renderer's), and a second view turned about y and shifted."""
    base = torch.from_numpy(v * 8.0 * np.array([1.0, -1.0, 1.0])).float()
    a = 0.3
    rot = torch.tensor([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]], dtype=torch.float32)
    return torch.stack([base, base @ rot.T + torch.tensor([0.02, -0.03, 0.0])]).cuda()


@pytest.mark.gpu
def test_rasterize_face_attributes_against_the_per_vertex_rasteriser():
    """Per-face-corner attributes gathered from per-vertex ones render the bits rasterize_attributes renders and send the same
    bits back to the vertices; their own gradient is the per-corner one (its sum over a vertex's corners is the per-vertex
    gradient), and attributes shared by the batch [F,3,3] receive the sum over the samples."""
    from gif_amd import render
    from gif_amd import shading as sd
    v, f = body()
    verts, faces = two_views(v), torch.from_numpy(f).cuda()
    g = torch.Generator().manual_seed(5)
    attr = torch.rand(2, v.shape[0], 3, generator=g).cuda()
    up = torch.randn(2, 3, 64, 64, generator=g).cuda()

    def grads(fn, a):
        x, a = verts.clone().requires_grad_(True), a.clone().requires_grad_(True)
        img, mask = fn(x, faces, a, 64, 64)
        return (img.detach(), mask) + torch.autograd.grad(img, (x, a), up)

    img0, m0, gv0, ga0 = grads(render.rasterize_attributes, attr)
    img1, m1, gv1, gf1 = grads(sd.rasterize_face_attributes, attr[:, faces])
    assert m0.any() and torch.equal(img0, img1) and torch.equal(m0, m1) and torch.equal(gv0, gv1)
    assert gf1.shape == (2, f.shape[0], 3, 3)
    back = torch.zeros(2, v.shape[0], 3, dtype=torch.float64, device="cuda").index_add_(
        1, faces.reshape(-1), gf1.double().reshape(2, -1, 3))
    assert ((back - ga0.double()).norm() / ga0.double().norm()).item() <= 1e-6  # (fp32 sums over a vertex's ~6 corners)
    shared = attr[0][faces]
    img2, _, gv2, gf2 = grads(sd.rasterize_face_attributes, shared)
    img3, _, gv3, gf3 = grads(sd.rasterize_face_attributes, shared[None].expand(2, -1, -1, -1))
    assert gf2.shape == (f.shape[0], 3, 3)
    assert torch.equal(img2, img3) and torch.equal(gv2, gv3) and torch.equal(gf2, gf3.sum(0))
    with pytest.raises(ValueError, match="face_attributes"):
        sd.rasterize_face_attributes(verts, faces, attr, 64, 64)


@pytest.mark.gpu
def test_pipeline_matches_the_restatement_in_its_place(monkeypatch):
    """render_shaded_condition(straight_through=True) three times: with sh_shade, with the float32 restatement on the device in
    its place, and with the float64 restatement in its place (casts around it).  The HIP rasteriser and its backward are the
    same in all three, so the float64 run is the reference and the float32 run the yardstick (err32) for the images and for the
    gradients to vertices_ndc, albedo and sh_coeff.  The albedo is affine in the texel coordinates: its bilinear derivative is
    continuous across cells."""
    from gif_amd import shading as sd
    v, f = body()
    B, T, S = 2, 64, 64
    g = torch.Generator().manual_seed(11)
    verts = two_views(v)
    faces = torch.from_numpy(f).cuda()
    uvs = sd.synthetic_face_uvs(v, f, seed=1).cuda()
    yy, xx = torch.meshgrid(torch.linspace(0, 1, T), torch.linspace(0, 1, T), indexing="ij")
    coef = torch.rand(B, 3, 3, generator=g)
    albedo = (0.3 + 0.2 * coef[:, :, 0, None, None] + 0.25 * coef[:, :, 1, None, None] * xx
              + 0.2 * coef[:, :, 2, None, None] * yy).cuda()
    sh = torch.randn(B, 9, 3, generator=g) * 0.3
    sh[:, 0] += 2.5
    sh = sh.cuda()
    up = torch.randn(B, 6, S, S, generator=g).cuda()

    def render_with(fn):
        if fn is not None:
            monkeypatch.setattr(sd, "sh_shade", fn)
        x = [t.clone().requires_grad_(True) for t in (verts, albedo, sh)]
        cond = sd.render_shaded_condition(x[0], faces, uvs, x[1], x[2], S, S, straight_through=True)
        return [cond.detach()] + list(torch.autograd.grad(cond, x, up))

    hip = render_with(None)
    f32 = render_with(shading_ref.sh_shade_in(torch.float32))
    f64 = render_with(shading_ref.sh_shade_in(torch.float64))
    assert hip[0].shape == (B, 6, S, S) and (hip[0][:, 3:] != -1).any(1).float().mean().item() > 0.05
    assert torch.equal(hip[0][:, 3:], f64[0][:, 3:])  # the normal render does not pass through the shading
    msgs, bad = [], []
    for name, got, y32, ref, metric in zip(("images", "g_vertices", "g_albedo", "g_sh"), hip, f32, f64,
                                           (rel_max, rel_fro, rel_fro, rel_fro)):
        ref = ref.double().cpu()
        assert ref.abs().max().item() > 0, name
        e, e32 = metric(got, ref), metric(y32, ref)
        msgs.append(f"{name} {e:.2e} (err32 {e32:.2e}, x{times(e, e32):.2f})")
        if not e <= M * e32 + FLOOR:
            bad.append(f"{name}: {e:.3e} > {M * e32 + FLOOR:.3e}")
    print("\n[shade] pipeline: " + "  ".join(msgs))
    assert not bad, "; ".join(bad)


@pytest.mark.gpu
def test_flame_layer_drives_the_shaded_renderer():
    """flame_batch [N,236] -> GIF's condition with no stand-in: finite, covers pixels, and with straight_through=True every slice
    of the labels (shape, expression, pose, camera, texture code, light code) receives a finite non-zero gradient; none with the
    default floor quantisation."""
    from gif_amd import flame as fl
    from gif_amd import shading as sd
    from gif_amd.data import synthetic_flame_labels
    v, f = body()
    layer = fl.FlameLayer(fl.synthetic_flame_model(v)).cuda()
    ft = torch.from_numpy(f).cuda()
    uvs = sd.synthetic_face_uvs(v, f).cuda()
    model = sd.synthetic_texture_model(64, 50, seed=0)
    fb = synthetic_flame_labels(2, "cuda", torch.Generator("cuda").manual_seed(1), n_labels=236)
    fb[:, 156] = 8.0  # camera scale: the 0.1-sized template fills most of the image ...
    fb[:, 157:159] = torch.tensor([0.01, -0.01], device="cuda")  # ... around its centre
    fb[:, 209:236] *= 0.3
    fb[:, 209:212] += 2.5  # a light that leaves most of the render inside (0, 1)
    fb.requires_grad_(True)
    rend, nrm = sd.ShadedFlameConditionRenderer(layer, ft, uvs, model, 64, 64, straight_through=True)(fb)
    assert rend.shape == (2, 3, 64, 64) and nrm.shape == (2, 3, 64, 64)
    assert torch.isfinite(rend).all() and torch.isfinite(nrm).all()
    assert (nrm != -1).any(1).float().mean().item() > 0.05  # covered pixels (the background renders as -1)
    assert (rend != -1).any(1).float().mean().item() > 0.05
    up = torch.randn(rend.shape, device="cuda", generator=torch.Generator("cuda").manual_seed(2))
    ((rend + nrm) * up).sum().backward()
    assert torch.isfinite(fb.grad).all()
    for lo, hi in ((0, 100), (100, 150), (150, 156), (156, 159), (159, 209), (209, 236)):
        assert fb.grad[:, lo:hi].abs().sum().item() > 0, (lo, hi)
    fb.grad = None
    rend, nrm = sd.ShadedFlameConditionRenderer(layer, ft, uvs, model, 64, 64)(fb)  # default: floor quantisation, zero gradient
    ((rend + nrm) * up).sum().backward()
    assert torch.all(fb.grad == 0)
    shared = sd.ShadedFlameConditionRenderer(layer, ft, uvs, model, 64, 64, shared_appearance=True)
    with torch.no_grad():
        r0, _ = shared(fb.detach())
        same_look = fb.detach().clone()
        same_look[1, 159:236] = same_look[0, 159:236]
        r1, _ = sd.ShadedFlameConditionRenderer(layer, ft, uvs, model, 64, 64)(same_look)
    # one albedo for the batch (Ba = 1) renders what two equal ones do (a one-row decode may round differently from a two-row one,
    # and an ulp may flip a pixel's quantisation step)
    assert (r0 != r1).float().mean().item() < 0.01
