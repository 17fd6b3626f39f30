"""Analytic edge antialiasing on the GPU (gif_antialias_f32, gif_antialias_bwd_f32 through gif_amd.antialias; -m gpu): forward
and both gradients against the float64 restatement tests/antialias_ref.py fed with the GPU's own tri and depth buffers,
determinism, the exact a = 0.5 case, the unchanged existing outputs, and a camera fit through the soft silhouette.

Cases (tests/antialias_ref.CASES): the 10 x 12 sphere, three posed copies at 70 x 90 (crosses the 64-pixel tile and band edge in
both axes) and one at 64 x 64; test_gpu_render_grad's edge_mesh at 70 x 70 (faces behind faces, boundary edges, a face that wins
no pixel, a degenerate face); one triangle in a 1 x 9 and in a 9 x 1 image (no vertical / no horizontal pairs); a quad whose
outline runs along row 0, row H-1, column 0 and column W-1; C = 1, 3, 4 and 7 over them.

Marginal pairs (t or a within 1e-4 of 0 or 1, a within 1e-4 of 0.5: float32 may classify them differently) are excluded by
zeroing the upstream gradient at their two pixels, which are left out of the forward comparison as well; their share of the
blended pairs is asserted <= 1 % and printed (measured on the oracle's buffers: 0 in every case but the edge mesh, 2 of 590).

Tolerances are not fixed in advance: every case measures the float32 run of the restatement against its float64 run — the
error of the definition itself in the kernels' number format — and allows the kernels 4 x that (the kernels make the same
operations in another reduction order, nothing else differs).  Metrics: largest absolute difference for the output and the image
gradient; row_err and fro_err of test_gpu_render_grad for the vertex gradient.  Measured on an MI355X, kernels / float32
restatement (the bound is 4 x the second figure; every figure is printed before it is asserted):
  case              forward              d image              d vertices row_err    d vertices fro_err
  sphere_70x90_b3   2.94e-6 / 2.94e-6    8.09e-6 / 8.09e-6    1.97e-7 / 1.57e-7     9.34e-8 / 6.60e-8
  sphere_64x64_b1   1.40e-6 / 1.40e-6    2.90e-6 / 2.90e-6    8.59e-8 / 9.31e-8     5.32e-8 / 4.36e-8
  edges_70x70_b2    2.56e-6 / 2.56e-6    9.12e-6 / 9.18e-6    1.23e-7 / 1.10e-7     7.50e-8 / 7.91e-8
  triangle_1x9      7.20e-8 / 7.20e-8    3.22e-7 / 3.22e-7    3.10e-8 / 4.45e-8     4.89e-8 / 6.91e-8
  triangle_9x1      7.20e-8 / 7.20e-8    3.22e-7 / 3.22e-7    3.85e-8 / 4.45e-8     5.95e-8 / 6.84e-8
  border_11x13      4.13e-7 / 4.13e-7    7.98e-7 / 7.98e-7    7.00e-8 / 3.12e-8     1.02e-7 / 5.30e-8
The forward figure has the size of the format: a is a difference of two pixel coordinates, and one unit in the last place of a
coordinate between 64 and 128 is 7.6e-6.  Camera fit: loss 270.9 -> 2.41, camera within (0.0005, 0.0076, 0.0025) of the target.
"""
import numpy as np
import pytest
import torch

import antialias_ref as aref

MAX_MARGINAL = 0.01
SLACK = 4.0  # kernels vs float64 may be this many times the float32 restatement's own error


def fro_err(got, ref):
    got, ref = got.double().cpu(), ref.double().cpu()
    return ((got - ref).norm() / ref.norm().clamp_min(1e-30)).item()


def row_err(got, ref):
    got, ref = got.double().cpu(), ref.double().cpu()
    rn = ref.norm(dim=-1)
    scale = rn.pow(2).mean().sqrt().clamp_min(1e-30)
    return ((got - ref).norm(dim=-1) / (rn + scale)).max().item()


def max_err(got, ref, keep=None):
    d = (got.double().cpu() - ref.double().cpu()).abs()
    return (d * keep if keep is not None else d).max().item()


def gpu_buffers(v_ndc, faces, h, w):
    """(pixel-space vertices, tri, depth) of the launch rasterize_attributes makes for these NDC vertices."""
    from gif_amd import standard_rasterize as sr
    B = v_ndc.shape[0]
    vi = sr.to_image_space(v_ndc.float(), h, w)
    fv = sr.face_vertices(vi, faces[None].expand(B, -1, -1))
    depth, tri, img = sr.new_buffers(B, h, w, v_ndc.device)
    sr.standard_rasterize_colors(fv, torch.zeros_like(fv), depth, tri, img, h, w)
    return vi, tri, depth


_RUNS = {}


def run_case(name):
    """One forward and backward of the kernels and of the float64 and float32 restatements per case, shared by the tests."""
    if name in _RUNS:
        return _RUNS[name]
    from gif_amd import antialias as AA
    v, f, h, w, C = aref.CASES[name]()
    B = v.shape[0]
    vt, ft = torch.from_numpy(v).cuda().requires_grad_(True), torch.from_numpy(f).cuda()
    vi, tri, depth = gpu_buffers(vt.detach(), ft, h, w)
    gen = torch.Generator().manual_seed(11)
    image_cpu = torch.rand((B, C, h, w), generator=gen)
    G_cpu = torch.randn((B, C, h, w), generator=gen)
    adj = aref.edge_adjacency_ref(f)
    assert torch.equal(AA.edge_adjacency(ft).cpu().long(), torch.from_numpy(adj))

    def ref(dtype):
        v_ = vt.detach().cpu().to(dtype).requires_grad_(True)
        im_ = image_cpu.to(dtype, copy=True).requires_grad_(True)
        out, stats = aref.antialias_ref(im_, tri.cpu(), depth.cpu(), aref.face_vertices_ref(v_, vi.cpu(), f, h, w), adj)
        return v_, im_, out, stats

    v64, im64, out64, stats = ref(torch.float64)
    v32, im32, out32, stats32 = ref(torch.float32)
    keep = (~stats["marginal_pixels"])[:, None].double()
    G = G_cpu.double() * keep
    (out64 * G).sum().backward()
    (out32 * G.float()).sum().backward()
    image = image_cpu.cuda().requires_grad_(True)
    out = AA.antialias(image, tri, depth, vt, ft)
    out.backward(G.float().cuda())
    torch.cuda.synchronize()
    _RUNS[name] = dict(stats=stats, stats32=stats32, keep=keep, out=(out.detach(), out32.detach(), out64.detach()),
                       gi=(image.grad, im32.grad, im64.grad), gv=(vt.grad, v32.grad, v64.grad), tri=tri, image=image_cpu, C=C)
    return _RUNS[name]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(aref.CASES))
def test_forward_and_gradients_vs_fp64(name):
    r = run_case(name)
    s = r["stats"]
    share = s["marginal"] / max(s["blended"], 1)
    print(f"{name}: C = {r['C']}, {s['pairs']} pairs, {s['blended']} blended, {s['marginal']} marginal ({100 * share:.2f} %)")
    assert s["blended"] > 0 and share <= MAX_MARGINAL
    assert (s["pairs"], s["blended"]) == (r["stats32"]["pairs"], r["stats32"]["blended"])
    out, out32, out64 = r["out"]
    gi, gi32, gi64 = r["gi"]
    gv, gv32, gv64 = r["gv"]
    figures = {
        "forward": (max_err(out, out64, r["keep"]), max_err(out32, out64, r["keep"])),
        "d image": (max_err(gi, gi64), max_err(gi32, gi64)),
        "d vertices row_err": (row_err(gv, gv64), row_err(gv32, gv64)),
        "d vertices fro_err": (fro_err(gv, gv64), fro_err(gv32, gv64)),
    }
    for what, (got, f32) in figures.items():
        print(f"  {what}: kernels {got:.2e}, float32 restatement {f32:.2e}, bound {SLACK * f32:.2e}")
    assert torch.all(gv[..., 2] == 0)  # depth only chooses the front pixel
    assert gv64.abs().sum() > 0 and (out64.detach() - r["image"].double()).abs().sum() > 0
    # pixels without a pair keep the input's bits
    tri = r["tri"].cpu()
    lone = torch.ones_like(tri, dtype=torch.bool)
    lone[:, :, 1:] &= tri[:, :, 1:] == tri[:, :, :-1]
    lone[:, :, :-1] &= tri[:, :, 1:] == tri[:, :, :-1]
    lone[:, 1:] &= tri[:, 1:] == tri[:, :-1]
    lone[:, :-1] &= tri[:, 1:] == tri[:, :-1]
    lone = lone[:, None].expand_as(r["image"])
    assert torch.equal(out.cpu()[lone], r["image"][lone])
    for what, (got, f32) in figures.items():
        assert got <= SLACK * f32, (name, what, got, f32)


@pytest.mark.gpu
def test_backward_deterministic():
    from gif_amd import antialias as AA
    v, f, h, w, C = aref.CASES["sphere_70x90_b3"]()
    ft = torch.from_numpy(f).cuda()
    gen = torch.Generator().manual_seed(5)
    image0, G = torch.rand((3, C, h, w), generator=gen).cuda(), torch.randn((3, C, h, w), generator=gen).cuda()
    grads = []
    for _ in range(2):
        vt, image = torch.from_numpy(v).cuda().requires_grad_(True), image0.clone().requires_grad_(True)
        _, tri, depth = gpu_buffers(vt.detach(), ft, h, w)
        AA.antialias(image, tri, depth, vt, ft).backward(G)
        grads.append((vt.grad.clone(), image.grad.clone()))
    assert torch.equal(grads[0][0].view(torch.int32), grads[1][0].view(torch.int32))
    assert torch.equal(grads[0][1].view(torch.int32), grads[1][1].view(torch.int32))
    assert grads[0][0].abs().sum() > 0 and (grads[0][1] != G).any()


@pytest.mark.gpu
def test_only_requested_gradients():
    """Either gradient alone equals its value when both are asked for."""
    from gif_amd import antialias as AA
    v, f, h, w, C = aref.CASES["edges_70x70_b2"]()
    ft = torch.from_numpy(f).cuda()
    gen = torch.Generator().manual_seed(6)
    image0, G = torch.rand((2, C, h, w), generator=gen).cuda(), torch.randn((2, C, h, w), generator=gen).cuda()
    _, tri, depth = gpu_buffers(torch.from_numpy(v).cuda(), ft, h, w)
    got = {}
    for need_i, need_v in ((True, True), (True, False), (False, True)):
        vt, image = torch.from_numpy(v).cuda().requires_grad_(need_v), image0.clone().requires_grad_(need_i)
        AA.antialias(image, tri, depth, vt, ft).backward(G)
        got[need_i, need_v] = (image.grad, vt.grad)
    assert got[True, False][1] is None and got[False, True][0] is None
    assert torch.equal(got[True, True][0], got[True, False][0]) and torch.equal(got[True, True][1], got[False, True][1])


@pytest.mark.gpu
def test_half_pixel_edges_return_the_rasterisers_bits():
    """An axis-aligned rectangle with its edges at half-integer coordinates (exact in float32 through the NDC transform at
    16 x 16): every pair has a = 0.5 exactly, weight 0 — the image and the mask come back bit for bit."""
    from gif_amd import antialias as AA, render
    h = w = 16
    v, f = aref.pixel_mesh([(3.5, 2.5), (9.5, 2.5), (9.5, 7.5), (3.5, 7.5)], [(0, 1, 2), (0, 2, 3)], h, w)
    vt, ft = torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda()
    attr = torch.rand(1, 4, 3, generator=torch.Generator().manual_seed(3)).cuda()
    img, mask = render.rasterize_attributes(vt, ft, attr, h, w)
    assert mask.sum().item() == 6 * 5
    img_aa, cov_aa = AA.rasterize_attributes_aa(vt, ft, attr, h, w)
    assert torch.equal(img_aa.contiguous().view(torch.int32), img.view(torch.int32))
    assert torch.equal(cov_aa, mask.float())
    # the same rectangle a quarter pixel to the right does blend
    v2 = v.copy()
    v2[..., 0] += 0.25 * 2 / w
    img2, cov2 = AA.rasterize_attributes_aa(torch.from_numpy(v2).cuda(), ft, attr, h, w)
    assert not torch.equal(cov2, mask.float())
    # left edge at x = 3.75: column 4 is covered to 3/4; right edge at x = 9.75: column 10 to 1/4.  (Row 7 of the right edge is
    # left out: its front pixel (9, 7) lies in the lower-left triangle, which does not own that edge — §3o, "what it does not do".)
    assert torch.equal(cov2[0, 0, 3:8, 4], torch.full((5,), 0.75, device="cuda"))
    assert torch.equal(cov2[0, 0, 3:7, 10], torch.full((4,), 0.25, device="cuda"))


@pytest.mark.gpu
def test_existing_outputs_unchanged():
    """rasterize_attributes and render_condition still return what the reference-shaped launches give, bit for bit; the mask of
    rasterize_attributes still has no gradient; rasterize_attributes_aa rasterises the same image under its blend."""
    from gif_amd import antialias as AA, render
    from gif_amd import standard_rasterize as sr
    v, f, h, w, _ = aref.CASES["edges_70x70_b2"]()
    B = v.shape[0]
    vt, ft = torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda()
    attr = torch.rand(v.shape, generator=torch.Generator().manual_seed(4)).cuda()

    def by_hand(a):
        faces_b = ft[None].expand(B, -1, -1)
        fv = sr.face_vertices(sr.to_image_space(vt, h, w), faces_b)
        depth, tri, img = sr.new_buffers(B, h, w, "cuda")
        sr.standard_rasterize_colors(fv, sr.face_vertices(a.contiguous(), faces_b), depth, tri, img, h, w)
        return img.permute(0, 3, 1, 2).contiguous(), tri, depth

    img0, tri0, depth0 = by_hand(attr)
    vg, ag = vt.clone().requires_grad_(True), attr.clone().requires_grad_(True)
    img, mask = render.rasterize_attributes(vg, ft, ag, h, w)
    assert torch.equal(img.detach().view(torch.int32), img0.view(torch.int32)) and torch.equal(mask[:, 0], tri0 >= 0)
    assert mask.requires_grad is False and render.rasterize_attributes(vg, ft, ag, h, w)[1].requires_grad is False
    normals = render.vertex_normals(vt, ft)
    cond0 = torch.cat((render.quantize_8bit(img0) * 2 - 1, render.quantize_8bit(by_hand(normals * 0.5 + 0.5)[0]) * 2 - 1), 1)
    assert torch.equal(render.render_condition(vt, ft, attr, h, w).view(torch.int32), cond0.view(torch.int32))
    # the opt-in path rasterises the same buffers: where no pair touches a pixel the bits are the rasteriser's
    img_aa, cov_aa = AA.rasterize_attributes_aa(vt, ft, attr, h, w)
    ref = AA.antialias(torch.cat((img0, (tri0 >= 0)[:, None].float()), 1), tri0, depth0, vt, ft)
    assert torch.equal(torch.cat((img_aa, cov_aa), 1), ref)
    assert img_aa.shape == (B, 3, h, w) and cov_aa.shape == (B, 1, h, w) and not torch.equal(img_aa, img0)
    sil = AA.soft_silhouette(vt, ft, h, w)
    assert torch.equal(sil, cov_aa)


@pytest.mark.gpu
def test_coverage_alone_reaches_the_vertices():
    from gif_amd import antialias as AA
    v, f, h, w, _ = aref.CASES["sphere_64x64_b1"]()
    ft = torch.from_numpy(f).cuda()
    attr = torch.rand(v.shape, generator=torch.Generator().manual_seed(8)).cuda().requires_grad_(True)
    vt = torch.from_numpy(v).cuda().requires_grad_(True)
    img_aa, cov_aa = AA.rasterize_attributes_aa(vt, ft, attr, h, w)
    assert img_aa.requires_grad and cov_aa.requires_grad
    cov_aa.sum().backward()
    assert torch.isfinite(vt.grad).all() and vt.grad[..., :2].abs().sum() > 0 and torch.all(vt.grad[..., 2] == 0)
    assert torch.all(attr.grad == 0)  # the mask does not depend on the attributes
    vt.grad = None
    img_aa, _ = AA.rasterize_attributes_aa(vt, ft, attr, h, w)
    img_aa.sum().backward()
    assert attr.grad.abs().sum() > 0 and vt.grad.abs().sum() > 0
    vs = torch.from_numpy(v).cuda().requires_grad_(True)
    AA.soft_silhouette(vs, ft, h, w).sum().backward()
    assert vs.grad.abs().sum() > 0


@pytest.mark.gpu
def test_camera_fit_through_the_soft_silhouette():
    """Adam on the summed squared difference of soft silhouettes moves an orthographic camera (s, tx, ty) onto its target: a mask
    loss alone, through batch_orth_proj.  Conditions with slack, not measurements: the loss falls below 10 % of its start and
    every component ends within 0.03 of the target."""
    from gif_amd import antialias as AA, render
    verts, f = aref.small_sphere()
    X = torch.from_numpy(verts.astype(np.float32))[None].cuda()
    ft = torch.from_numpy(f).cuda()
    h = w = 48
    target_cam = torch.tensor([[0.6, 0.15, -0.1]], device="cuda")
    with torch.no_grad():
        target = AA.soft_silhouette(render.batch_orth_proj(X, target_cam), ft, h, w)
    cam = torch.tensor([[0.45, -0.05, 0.08]], device="cuda", requires_grad=True)
    opt = torch.optim.Adam([cam], lr=0.02)
    losses = []
    for _ in range(60):
        opt.zero_grad()
        loss = ((AA.soft_silhouette(render.batch_orth_proj(X, cam), ft, h, w) - target) ** 2).sum()
        loss.backward()
        opt.step()
        losses.append(loss.item())
    with torch.no_grad():
        last = ((AA.soft_silhouette(render.batch_orth_proj(X, cam), ft, h, w) - target) ** 2).sum().item()
    err = (cam.detach() - target_cam).abs()[0].tolist()
    print(f"camera fit: loss {losses[0]:.1f} -> {last:.2f}, camera error {err}")
    assert last < 0.1 * losses[0] and max(err) <= 0.03, (losses[0], last, err)


@pytest.mark.gpu
def test_refusals():
    """CPU tensors raise GifHipError (no fallback); a double backward raises; two topologies in one batch are refused."""
    from gif_amd import _lib
    from gif_amd import antialias as AA
    v, f, h, w, C = aref.CASES["border_11x13"]()
    vt, ft = torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda()
    _, tri, depth = gpu_buffers(vt, ft, h, w)
    image = torch.rand(1, C, h, w).cuda()
    for args in ((image.cpu(), tri, depth, vt, ft), (image, tri.cpu(), depth, vt, ft), (image, tri, depth, vt.cpu(), ft),
                 (image, tri, depth, vt, ft.cpu())):
        with pytest.raises(_lib.GifHipError, match="device tensors"):
            AA.antialias(*args)
    with pytest.raises(_lib.GifHipError, match="device tensors"):
        AA.soft_silhouette(vt.cpu(), ft.cpu(), h, w)
    vg = vt.clone().requires_grad_(True)
    out = AA.antialias(image, tri, depth, vg, ft)
    (g,) = torch.autograd.grad(out.sum() * 0.5 + (out * out).sum(), vg, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable|differentiated twice|does not require grad"):
        g.sum().backward()
    two = torch.stack([ft, ft.flip(0)])
    v2 = vt.expand(2, -1, -1).contiguous()
    _, tri2, depth2 = gpu_buffers(v2, ft, h, w)
    with pytest.raises(_lib.GifHipError, match="needs one face topology for the whole batch"):
        AA.antialias(image.expand(2, -1, -1, -1).contiguous(), tri2, depth2, v2, two)
