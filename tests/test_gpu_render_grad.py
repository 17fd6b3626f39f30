"""Differentiable condition rendering: the backward passes of vertex_normals, rasterize_attributes and render_condition
(gif_vertex_normals_bwd_f32, gif_rasterize_colors_bwd_f32, gif_face_gather_bwd_f32) against fp64 autograd of torch
restatements written here, plus determinism and no-change-of-forward checks (-m gpu).

The restatements take the forward's face-index buffer `tri` as given (the gradient lives inside the winning face only) and
rebuild each covered pixel as sum_k w_k c_k with the reference's barycentric formula at integer pixel centres, inverDeno = 0
giving w = (1, 0, 0).  The two CPU tests tie that restatement to the true derivative by central differences in fp64, with the
vertices moved so little that the oracle rasteriser's `tri` does not change.

Ill-conditioned pixels: on a grazing (nearly edge-on) or sliver face the reference's fp32 barycentric formula itself departs
from its fp64 value (up to hundreds, on the rotated sphere's silhouette), and so does any derivative of it.  `conditioned`
keeps the covered pixels where the fp32 forward image and the fp64 restatement agree to FWD_TOL; the upstream gradient is zeroed
elsewhere, and the excluded share of the covered pixels is asserted small (MAX_EXCLUDED) and printed.

Error metrics (`row_err`, `fro_err`): per vertex row, |got - ref|_2 / (|ref|_2 + rms of all rows of ref): relative for every vertex that
carries a gradient, and a vertex whose true gradient is ~0 is held to the tensor's typical scale rather than to zero; and
|got - ref|_F / |ref|_F over the whole tensor.
"""
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-4
# vertex gradients, worst vertex row: ~3x the worst measured on an MI355X (7.1e-4, sphere B=4 through render_condition).  The
# per-pixel chain rule through the barycentric formula cancels in fp32 (p0 gets -(dv0 + dv1 + dv2)); a float32 emulation of the
# kernel's arithmetic on the body mesh gives 1.9e-4 on its worst row and 3.3e-5 on the whole tensor, float64 3e-14.  The whole
# tensor (fro_err) is held to TOL.
TOL_ROW_V = 2e-3
EPS = 1e-6  # F.normalize eps of the reference's vertex_normals
FWD_TOL = 1e-5  # fp32 forward vs fp64 restatement, per pixel, attributes in [0, 1]
MAX_EXCLUDED = 0.01


# ------------------------------------------------------------------------------------------------ meshes (NDC vertices)
def body_mesh(B):
    """tests/golden/body_mesh.npz scaled into the image, B rotated / scaled copies."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "body_mesh.npz"))
    v, f = g["vertices"] * np.float32(0.8), g["faces"].astype(np.int64)
    rng = np.random.RandomState(0)
    vs = []
    for i in range(B):
        a = rng.uniform(-0.6, 0.6) if i else 0.0
        R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]], np.float32)
        vs.append((v @ R.T * np.float32(1.0 + 0.1 * i)).astype(np.float32))
    return np.stack(vs), f


def sphere_mesh(B):
    """FLAME-sized synthetic mesh: V = 5023, F = 9976.  A lat-long sphere (70 x 70 quads + pole fans: 4972 vertices,
    9940 faces), 51 unused vertices, and 36 faces repeated from the front half (exact depth ties: the lower index wins)."""
    nlat, nlon = 72, 70
    verts = [(0.0, -1.0, 0.0)]
    for i in range(1, nlat):
        t = np.pi * i / nlat - np.pi / 2
        for j in range(nlon):
            p = 2 * np.pi * j / nlon
            verts.append((np.cos(t) * np.sin(p), np.sin(t), np.cos(t) * np.cos(p)))
    verts.append((0.0, 1.0, 0.0))
    verts = np.array(verts)
    top = len(verts) - 1
    ring = lambda i, j: 1 + (i - 1) * nlon + j % nlon
    faces = []
    for j in range(nlon):
        faces.append((0, ring(1, j + 1), ring(1, j)))
        faces.append((top, ring(nlat - 1, j), ring(nlat - 1, j + 1)))
    for i in range(1, nlat - 1):
        for j in range(nlon):
            a, b, c, d = ring(i, j), ring(i, j + 1), ring(i + 1, j), ring(i + 1, j + 1)
            faces.append((a, b, d))
            faces.append((a, d, c))
    faces = np.array(faces, np.int64)
    faces = np.concatenate([faces, faces[2 * nlon + 10:2 * nlon + 46]])
    rng = np.random.RandomState(1)
    verts = np.concatenate([verts, rng.uniform(-0.5, 0.5, (51, 3))])
    assert verts.shape == (5023, 3) and faces.shape == (9976, 3)
    vs = []
    for i in range(B):
        a = 0.3 * i
        R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        vs.append(verts @ R.T * 0.85)
    vs = np.stack(vs)
    vs[..., 2] *= -1  # +z away from the camera: the z-buffer keeps the near (-z) half, whose faces wind front-facing
    return vs.astype(np.float32), faces


def edge_mesh(B, h):
    """Two screen-filling faces behind a few medium ones, a face that covers no pixel centre, a degenerate (zero-area)
    face and an unused vertex."""
    rng = np.random.RandomState(2)
    px = 2.0 / h  # one pixel in NDC
    v = [(-1.6, -1.55, 0.9), (1.63, -1.6, 0.9), (1.57, 1.6, 0.9), (-1.6, 1.62, 0.9)]  # screen-filling quad, far; its
    # diagonal is skewed off the pixel grid
    f = [(0, 2, 1), (0, 3, 2)]
    for _ in range(6):  # medium triangles in front
        c = rng.uniform(-0.6, 0.6, 2)
        k = len(v)
        for a in (0.0, 2.1, 4.2):
            r = rng.uniform(0.15, 0.35)
            v.append((c[0] + r * np.cos(a), c[1] + r * np.sin(a), rng.uniform(0.0, 0.5)))
        f.append((k, k + 2, k + 1))
    # no pixel centre: a tiny triangle strictly between pixel centres (pixel centre (i, j) sits at NDC -1 + 2 i / h)
    x0, y0 = -1 + px * 10.2, -1 + px * 20.2
    k = len(v)
    v += [(x0, y0, 0.1), (x0 + px * 0.5, y0, 0.1), (x0, y0 + px * 0.5, 0.1)]
    f.append((k, k + 1, k + 2))
    f.append((k, k + 2, k + 1))  # (either winding)
    # degenerate: a repeated vertex
    k = len(v)
    v += [(0.1, 0.1, 0.0), (0.4, 0.2, 0.0)]
    f.append((k, k, k + 1))
    v.append((0.0, 0.0, 0.0))  # unused
    f = np.array(f, np.int64)
    v = np.array(v, np.float64)
    vs = np.stack([v + np.array([3 * px * i, -2 * px * i, 0.0]) for i in range(B)])  # whole pixels: coverage classes kept
    return vs.astype(np.float32), f


# ------------------------------------------------------------------------------------------------ fp64 restatements
def to_pixels(v, h, w):
    """x, y of standard_rasterize.to_image_space (z only orders the faces)."""
    return torch.stack([v[..., 0] * w / 2 + w / 2, v[..., 1] * h / 2 + h / 2], -1)


def interp_ref(pix, attr, faces, tri):
    """pix [B,V,2], attr [B,V,3] (float64, differentiable), faces [F,3] int64, tri [B,H,W] int -> images [B,3,H,W]."""
    B, H, W = tri.shape
    bi, yi, xi = torch.nonzero(tri >= 0, as_tuple=True)
    fi = tri[bi, yi, xi].long()
    corner = faces[fi]  # [N,3] vertex ids
    p = pix[bi[:, None], corner]  # [N,3,2]
    c = attr[bi[:, None], corner]  # [N,3,3]
    v0, v1, v2 = p[:, 2] - p[:, 0], p[:, 1] - p[:, 0], torch.stack([xi, yi], -1).to(pix) - p[:, 0]
    d00, d01, d11 = (v0 * v0).sum(-1), (v0 * v1).sum(-1), (v1 * v1).sum(-1)
    d02, d12 = (v0 * v2).sum(-1), (v1 * v2).sum(-1)
    den = d00 * d11 - d01 * d01
    degen = den == 0
    inv = torch.where(degen, torch.zeros_like(den), 1 / torch.where(degen, torch.ones_like(den), den))
    u = (d11 * d02 - d01 * d12) * inv
    vv = (d00 * d12 - d01 * d02) * inv
    wts = torch.stack([1 - u - vv, vv, u], -1)  # [N,3]
    val = (wts[..., None] * c).sum(1)  # [N,3]
    img = torch.zeros((B, H, W, 3), dtype=pix.dtype).index_put((bi, yi, xi), val)
    return img.permute(0, 3, 1, 2)


def normals_ref(v, faces):
    """oracle/mesh_ref.vertex_normals in differentiable torch: index_add of the corner cross products, F.normalize."""
    B, V, _ = v.shape
    vf = v[:, faces]  # [B,F,3,3]
    n = torch.zeros_like(v)
    n = n.index_add(1, faces[:, 1], torch.cross(vf[:, :, 2] - vf[:, :, 1], vf[:, :, 0] - vf[:, :, 1], dim=-1))
    n = n.index_add(1, faces[:, 2], torch.cross(vf[:, :, 0] - vf[:, :, 2], vf[:, :, 1] - vf[:, :, 2], dim=-1))
    n = n.index_add(1, faces[:, 0], torch.cross(vf[:, :, 1] - vf[:, :, 0], vf[:, :, 2] - vf[:, :, 0], dim=-1))
    return n / n.norm(dim=2, keepdim=True).clamp_min(EPS)


def condition_ref(pix, v, tex, faces, tri):
    """render_condition(straight_through=True) without the quantisation (its gradient is the identity)."""
    n = normals_ref(v, faces)
    return torch.cat([interp_ref(pix, tex, faces, tri) * 2 - 1, interp_ref(pix, n * 0.5 + 0.5, faces, tri) * 2 - 1], 1)


def conditioned(gpu_imgs, ref_imgs, tri):
    """[B,1,H,W] float mask of the covered pixels where every fp32 forward image agrees with its fp64 restatement."""
    ok = tri.cpu()[:, None] >= 0
    for a, b in zip(gpu_imgs, ref_imgs):
        ok &= ((a.detach().cpu().double() - b.detach()).abs() <= FWD_TOL).all(1, keepdim=True)
    covered = (tri >= 0).sum().item()
    excluded = 1 - ok.sum().item() / max(covered, 1)
    assert excluded < MAX_EXCLUDED, f"{excluded:.4f} of the covered pixels are ill-conditioned"
    return ok.double(), excluded


def fro_err(got, ref):
    got, ref = got.double().cpu(), ref.double().cpu()
    return ((got - ref).norm() / ref.norm().clamp_min(1e-30)).item()


def row_err(got, ref):
    got, ref = got.double().cpu(), ref.double().cpu()
    rn = ref.norm(dim=-1)
    scale = rn.pow(2).mean().sqrt().clamp_min(1e-30)
    return ((got - ref).norm(dim=-1) / (rn + scale)).max().item()


# ------------------------------------------------------------------------------------------------ GPU helpers
def gpu_tri(v_ndc, faces, h, w):
    """The forward's face-index buffer for these NDC vertices (the same launch rasterize_attributes makes)."""
    from gif_amd import standard_rasterize as sr
    B = v_ndc.shape[0]
    vi = sr.to_image_space(v_ndc.float(), h, w)
    fv = sr.face_vertices(vi, faces[None].expand(B, -1, -1))
    depth, tri, img = sr.new_buffers(B, h, w, v_ndc.device)
    sr.standard_rasterize_colors(fv, torch.zeros_like(fv), depth, tri, img, h, w)
    return vi, tri


def ref_pixels(v64, vi32, h, w):
    """fp64 pixel coordinates carrying exactly the fp32 values the kernel sees, with the exact NDC -> pixel derivative."""
    p = to_pixels(v64, h, w)
    return vi32[..., :2].double().cpu() + (p - p.detach())


MESHES = {
    "body_b1": lambda: body_mesh(1),
    "body_b4": lambda: body_mesh(4),
    "sphere_b1": lambda: sphere_mesh(1),
    "sphere_b4": lambda: sphere_mesh(4),
    "edges_b1": lambda: edge_mesh(1, 256),
    "edges_b4": lambda: edge_mesh(4, 256),
}


def _cuda(v, f, seed):
    torch.manual_seed(seed)
    vt = torch.from_numpy(v).cuda()
    ft = torch.from_numpy(f).cuda()
    tex = torch.rand(v.shape, device="cuda")
    return vt, ft, tex


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(MESHES))
def test_rasterize_attributes_backward_vs_fp64(name):
    from gif_amd import render
    h = w = 256
    v, f = MESHES[name]()
    vt, ft, tex = _cuda(v, f, 0)
    vt.requires_grad_(True)
    tex.requires_grad_(True)
    img, mask = render.rasterize_attributes(vt, ft, tex, h, w)
    vi, tri = gpu_tri(vt.detach(), ft, h, w)
    assert torch.equal(mask[:, 0], tri >= 0)
    cover = (tri >= 0).float().mean().item()
    assert cover > 0.05, f"{name}: mesh covers {cover:.3f} of the image"
    v64 = vt.detach().cpu().double().requires_grad_(True)
    t64 = tex.detach().cpu().double().requires_grad_(True)
    ref = interp_ref(ref_pixels(v64, vi, h, w), t64, torch.from_numpy(f), tri.cpu())
    keep, excluded = conditioned([img], [ref], tri)
    g = torch.randn_like(img) * keep.float().cuda()
    img.backward(g)
    (ref * g.cpu().double()).sum().backward()
    assert torch.all(vt.grad[..., 2] == 0)  # depth only selects the winner
    ev, fv, et = row_err(vt.grad, v64.grad), fro_err(vt.grad, v64.grad), row_err(tex.grad, t64.grad)
    print(f"{name}: cover {cover:.3f}  excluded {excluded:.1e}  d vertices {ev:.2e} (tensor {fv:.2e})  d attributes {et:.2e}")
    assert ev < TOL_ROW_V and fv < TOL and et < TOL, (name, ev, fv, et)
    if name.startswith("edges"):
        # the no-pixel, degenerate and unused vertices get exactly zero
        assert torch.all(vt.grad[:, -6:] == 0) and torch.all(tex.grad[:, -6:] == 0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["sphere_b1", "sphere_b4", "body_b4"])
def test_vertex_normals_backward_vs_fp64(name):
    """Including three vertices whose only face is degenerate (exactly collinear, exact dyadic coordinates): their sums are
    exactly 0 in fp32 and fp64, so F.normalize's clamped branch g / eps is taken."""
    from gif_amd import render
    v, f = MESHES[name]()
    B, V = v.shape[:2]
    iso = np.array([[0.25, 0.5, 0.125], [0.75, 0.25, 0.375], [0.5, 0.375, 0.25]], np.float32)  # iso[2] = midpoint
    v = np.concatenate([v, np.repeat(iso[None], B, 0)], 1)
    f = np.concatenate([f, [[V + 2, V, V + 1]]])
    vt, ft, _ = _cuda(v, f, 1)
    vt.requires_grad_(True)
    n = render.vertex_normals(vt, ft)
    g = torch.randn_like(n)
    n.backward(g)
    v64 = vt.detach().cpu().double().requires_grad_(True)
    ref = normals_ref(v64, torch.from_numpy(f))
    assert (ref.float() - n.detach().cpu()).abs().max().item() < 1e-5
    assert torch.all(n[:, -3:] == 0)  # clamped branch in the forward too
    (ref * g.cpu().double()).sum().backward()
    err = row_err(vt.grad, v64.grad)
    print(f"{name}: d vertices {err:.2e} (tensor {fro_err(vt.grad, v64.grad):.2e})")
    assert err < TOL, (name, err)
    assert v64.grad[:, -3:].abs().max() > 1e4  # the eps branch carried g / eps into the degenerate face


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["body_b4", "sphere_b4"])
def test_render_condition_straight_through_vs_fp64(name):
    from gif_amd import render
    h = w = 256
    v, f = MESHES[name]()
    vt, ft, tex = _cuda(v, f, 2)
    vt.requires_grad_(True)
    tex.requires_grad_(True)
    cond = render.render_condition(vt, ft, tex, h, w, straight_through=True)
    vi, tri = gpu_tri(vt.detach(), ft, h, w)
    v64 = vt.detach().cpu().double().requires_grad_(True)
    t64 = tex.detach().cpu().double().requires_grad_(True)
    pix, faces = ref_pixels(v64, vi, h, w), torch.from_numpy(f)
    with torch.no_grad():
        imgs = [render.rasterize_attributes(vt, ft, tex, h, w)[0],
                render.rasterize_attributes(vt, ft, render.vertex_normals(vt, ft) * 0.5 + 0.5, h, w)[0]]
        refs = [interp_ref(pix, t64, faces, tri.cpu()), interp_ref(pix, normals_ref(v64, faces) * 0.5 + 0.5, faces, tri.cpu())]
    keep, excluded = conditioned(imgs, refs, tri)
    G = torch.randn_like(cond) * keep.float().cuda()
    cond.backward(G)
    ref = condition_ref(pix, v64, t64, faces, tri.cpu())
    (ref * G.cpu().double()).sum().backward()
    ev, fv, et = row_err(vt.grad, v64.grad), fro_err(vt.grad, v64.grad), row_err(tex.grad, t64.grad)
    print(f"{name}: excluded {excluded:.1e}  d vertices {ev:.2e} (tensor {fv:.2e})  d texture {et:.2e}")
    assert ev < TOL_ROW_V and fv < TOL and et < TOL, (name, ev, fv, et)


@pytest.mark.gpu
def test_backward_deterministic():
    from gif_amd import render
    v, f = sphere_mesh(4)
    grads = []
    for _ in range(2):
        vt, ft, tex = _cuda(v, f, 3)
        vt.requires_grad_(True)
        tex.requires_grad_(True)
        cond = render.render_condition(vt, ft, tex, 256, 256, straight_through=True)
        cond.backward(torch.ones_like(cond) * torch.linspace(-1, 1, 256, device="cuda"))
        grads.append((vt.grad.clone(), tex.grad.clone()))
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])
    assert grads[0][0].abs().sum() > 0 and grads[0][1].abs().sum() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["body_b4", "edges_b4"])
def test_forward_unchanged_by_grad(name):
    """Values are bit-identical with and without grad-requiring inputs; no history without them; the default quantisation
    has a zero gradient."""
    from gif_amd import render
    v, f = MESHES[name]()
    vt, ft, tex = _cuda(v, f, 4)
    with torch.no_grad():
        c0 = render.render_condition(vt, ft, tex)
        i0, m0 = render.rasterize_attributes(vt, ft, tex, 256, 256)
        n0 = render.vertex_normals(vt, ft)
    c1 = render.render_condition(vt, ft, tex)
    assert c1.grad_fn is None and render.rasterize_attributes(vt, ft, tex, 256, 256)[0].grad_fn is None
    assert render.vertex_normals(vt, ft).grad_fn is None
    vg, tg = vt.clone().requires_grad_(True), tex.clone().requires_grad_(True)
    c2 = render.render_condition(vg, ft, tg)
    c3 = render.render_condition(vg, ft, tg, straight_through=True)
    i2, m2 = render.rasterize_attributes(vg, ft, tg, 256, 256)
    n2 = render.vertex_normals(vg, ft)
    assert c2.grad_fn is not None and c3.grad_fn is not None and i2.grad_fn is not None and n2.grad_fn is not None
    for a, b in ((c0, c1), (c0, c2), (c0, c3), (i0, i2), (m0, m2), (n0, n2)):
        assert torch.equal(a, b.detach())
    assert not m2.requires_grad
    c2.backward(torch.randn_like(c2))
    assert torch.all(vg.grad == 0) and torch.all(tg.grad == 0)


@pytest.mark.gpu
def test_flame_renderer_passes_straight_through():
    """FlameConditionRenderer(straight_through=True): the FLAME parameters (here the camera) receive a gradient."""
    from gif_amd import render
    from gif_amd.data import SyntheticFlame
    v, f = sphere_mesh(1)
    flame = SyntheticFlame(v[0] * 0.1, "cuda")
    ft = torch.from_numpy(f).cuda()
    tex = torch.rand(v.shape[1], 3, device="cuda")
    fb = torch.zeros(2, 159, device="cuda")
    fb[:, 156] = 8.0  # camera scale: the 0.1-sized template fills most of the image
    fb.requires_grad_(True)
    rend, nrm = render.FlameConditionRenderer(flame, ft, tex, 64, 64, straight_through=True)(fb)
    (rend * torch.randn_like(rend)).sum().backward()
    assert torch.isfinite(fb.grad).all() and fb.grad[:, 156:159].abs().sum() > 0
    fb.grad = None
    rend, nrm = render.FlameConditionRenderer(flame, ft, tex, 64, 64)(fb)  # default: floor quantisation, zero gradient
    (rend * torch.randn_like(rend)).sum().backward()
    assert torch.all(fb.grad == 0)


# ------------------------------------------------------------------------------------------------ CPU: restatement vs FD
def _oracle_tri(v, f, h, w):
    """tri of the oracle rasteriser; float64 vertices take its float64 path (to_image_space in float64 as well)."""
    from oracle import rasterize_oracle as ro
    B = v.shape[0]
    if v.dtype == np.float64:
        vi = v.copy()
        vi[..., 0] = v[..., 0] * w / 2 + w / 2
        vi[..., 1] = v[..., 1] * h / 2 + h / 2
        vi[..., 2] = v[..., 2] - v[..., 2].min() + 1
    else:
        vi = ro.to_image_space(v, h, w)
    fv = np.ascontiguousarray(ro.face_vertices(vi, np.repeat(f[None], B, 0).astype(np.int32)))
    d, t, b = ro.new_buffers(B, h, w)
    if v.dtype == np.float64:
        d, b = d.astype(np.float64), b.astype(np.float64)
    ro.standard_rasterize(fv, d, t, b, h, w)
    return vi, t


@pytest.mark.parametrize("which", ["interp", "condition"])
def test_restatement_matches_finite_differences(which):
    """The analytic gradient of the fp64 restatement equals its central difference, with perturbations so small that the
    oracle's tri buffer is unchanged (checked): the formula is the true derivative of the rendered pixels."""
    h = w = 48
    v, f = edge_mesh(2, h)
    v = v.astype(np.float32)
    rng = np.random.RandomState(5)
    tex = rng.uniform(0, 1, v.shape)
    G = torch.from_numpy(rng.standard_normal((2, 6 if which == "condition" else 3, h, w)))
    ft = torch.from_numpy(f)
    _, tri0 = _oracle_tri(v, f, h, w)
    assert np.array_equal(_oracle_tri(v.astype(np.float64), f, h, w)[1], tri0)
    tri = torch.from_numpy(tri0)

    def loss(vv, tt):
        pix = to_pixels(vv, h, w)
        out = condition_ref(pix, vv, tt, ft, tri) if which == "condition" else interp_ref(pix, tt, ft, tri)
        return (out * G).sum()

    v64 = torch.from_numpy(v.astype(np.float64)).requires_grad_(True)
    t64 = torch.from_numpy(tex).requires_grad_(True)
    loss(v64, t64).backward()
    delta = 1e-7
    for k in range(4):
        dv = torch.from_numpy(rng.standard_normal(v.shape))
        dv[..., 2] = 0 if which == "interp" else dv[..., 2]
        dt = torch.from_numpy(rng.standard_normal(tex.shape))
        for s in (1, -1):  # tri stays fixed under the perturbation (the oracle's float64 path)
            _, t_s = _oracle_tri(v.astype(np.float64) + s * delta * dv.numpy(), f, h, w)
            assert np.array_equal(t_s, tri0)
        with torch.no_grad():
            fd = (loss(v64 + delta * dv, t64 + delta * dt) - loss(v64 - delta * dv, t64 - delta * dt)) / (2 * delta)
        an = (v64.grad * dv).sum() + (t64.grad * dt).sum()
        assert abs(fd.item() - an.item()) <= 1e-6 * max(abs(an.item()), 1.0), (k, fd.item(), an.item())
