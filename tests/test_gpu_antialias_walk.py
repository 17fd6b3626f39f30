"""Walking edge antialiasing on the GPU (gif_antialias_walk_f32, gif_antialias_walk_bwd_f32 through gif_amd.antialias with
max_hops > 0; -m gpu): forward and both gradients against the float64 restatement tests/antialias_walk_ref.py fed
with the GPU's own tri and depth buffers, the pixels walking adds, the unchanged bits of everything that existed, determinism,
an exact edge through a face that does not own it, and a camera fit on a mesh that is fine for its image.

Cases (tests/antialias_walk_ref.WALK_CASES; mesh, image, C, max_hops): the 10 x 12 sphere, three posed copies at 70 x 90 (B > 1,
tile and band edges) and one at 64 x 64, 4 hops; the 24 x 30 sphere at 70 x 90, 16 hops (deepest hit at hop 15); the 40 x 48 sphere
at 70 x 90, 8 hops (the cap cuts walks short: kernel and restatement must stop at the same hop); test_gpu_render_grad's edge_mesh
(boundary edges only: walking adds nothing); the strip mesh and its transpose at 12 x 12 (faces narrower than a pixel behind the
outline); the border quad as a 9 x 9 grid at 11 x 13 (grown boxes clamped at all four image borders); C = 1, 3, 4, 7 over them.

Pattern, metrics and marginal handling are tests/test_gpu_antialias.py's: marginal pairs (some edge tested along the walk has t or
a within 1e-4 of 0 or 1, or the hit's a lies within 1e-4 of 0.5) get no upstream gradient at their two pixels, which are left out
of the forward comparison; their share of the blended pairs is asserted <= 1 % (none where fewer than 100 blend).  Tolerances are
not fixed in advance: every case measures the float32 run of the restatement against its float64 run and allows the kernels 4 x
that (the same operations in another summation order).  Measured on an MI355X, kernels / float32 restatement (the bound is 4 x the
second figure; every figure is printed before it is asserted):
  case               blended (0 hops)  forward              d image              d vertices row_err    d vertices fro_err
  sphere_70x90_b3    637 (335)         2.94e-6 / 2.94e-6    8.09e-6 / 8.09e-6    3.45e-7 / 2.57e-7     8.34e-8 / 9.73e-8
  sphere_64x64_b1    170 (79)          1.40e-6 / 1.40e-6    7.06e-6 / 7.12e-6    1.08e-7 / 8.61e-8     8.53e-8 / 6.55e-8
  sphere24x30_70x90  178 (23)          2.71e-6 / 2.71e-6    7.86e-6 / 7.86e-6    2.29e-7 / 1.55e-7     4.69e-8 / 6.27e-8
  sphere40x48_70x90  158 (8)           3.06e-6 / 3.06e-6    8.10e-6 / 8.10e-6    2.58e-7 / 2.08e-7     6.36e-8 / 6.39e-8
  edges_70x70_b2     590 (590)         2.56e-6 / 2.56e-6    9.12e-6 / 9.18e-6    1.85e-7 / 1.10e-7     1.15e-7 / 7.91e-8
  strip_12x12        24 (10)           1.32e-7 / 1.32e-7    2.93e-7 / 2.93e-7    9.07e-8 / 6.07e-8     9.40e-8 / 3.90e-8
  strip_12x12_t      24 (10)           1.85e-7 / 1.85e-7    4.53e-7 / 4.53e-7    1.13e-7 / 1.17e-7     1.44e-7 / 1.27e-7
  border_grid_11x13  40 (11)           3.83e-7 / 3.83e-7    7.52e-7 / 7.52e-7    2.65e-7 / 2.65e-7     7.33e-8 / 7.33e-8
Marginal pairs: 1 on the 40 x 48 sphere (not among the blended), 2 on the edge mesh (as at zero hops), none elsewhere.  Walking
changes 71 pixels of the 64 x 64 sphere's soft silhouette.  Camera fit (24 x 30 sphere at 48 x 48, 60 Adam steps): with 16 hops loss
264.7 -> 5.03, camera within (0.0002, 0.0037, 0.0044) of the target; with zero hops 275.7 -> 0.34, within (0.0009, 0.0006, 0.0024).
"""
import numpy as np
import pytest
import torch

import antialias_ref as aref
import antialias_walk_ref as wref
from test_gpu_antialias import SLACK, fro_err, gpu_buffers, max_err, row_err

MAX_MARGINAL = 0.01

_RUNS = {}


def run_case(name):
    """One forward and backward of the kernels and of the float64 and float32 restatements per case, shared by the tests."""
    if name in _RUNS:
        return _RUNS[name]
    from gif_amd import antialias as AA
    v, f, h, w, C, hops = wref.WALK_CASES[name]()
    B = v.shape[0]
    vt, ft = torch.from_numpy(v).cuda().requires_grad_(True), torch.from_numpy(f).cuda()
    vi, tri, depth = gpu_buffers(vt.detach(), ft, h, w)
    gen = torch.Generator().manual_seed(11)
    image_cpu = torch.rand((B, C, h, w), generator=gen)
    G_cpu = torch.randn((B, C, h, w), generator=gen)
    adj = aref.edge_adjacency_ref(f)
    assert torch.equal(AA.edge_adjacency(ft).cpu().long(), torch.from_numpy(adj))

    def ref(dtype, max_hops=hops):
        v_ = vt.detach().cpu().to(dtype).requires_grad_(True)
        im_ = image_cpu.to(dtype, copy=True).requires_grad_(True)
        out, stats = wref.antialias_walk_ref(im_, tri.cpu(), depth.cpu(), aref.face_vertices_ref(v_, vi.cpu(), f, h, w), adj, max_hops)
        return v_, im_, out, stats

    v64, im64, out64, stats = ref(torch.float64)
    v32, im32, out32, stats32 = ref(torch.float32)
    stats0 = ref(torch.float64, 0)[3]
    keep = (~stats["marginal_pixels"])[:, None].double()
    G = G_cpu.double() * keep
    (out64 * G).sum().backward()
    (out32 * G.float()).sum().backward()
    image = image_cpu.cuda().requires_grad_(True)
    out = AA.antialias(image, tri, depth, vt, ft, max_hops=hops)
    out.backward(G.float().cuda())
    torch.cuda.synchronize()
    _RUNS[name] = dict(stats=stats, stats32=stats32, stats0=stats0, keep=keep, out=(out.detach(), out32.detach(), out64.detach()),
                       gi=(image.grad, im32.grad, im64.grad), gv=(vt.grad, v32.grad, v64.grad), tri=tri, depth=depth, image=image_cpu,
                       G=G.float().cuda(), C=C, hops=hops, v=v, f=f, hw=(h, w))
    return _RUNS[name]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(wref.WALK_CASES))
def test_forward_and_gradients_vs_fp64(name):
    r = run_case(name)
    s, s0 = r["stats"], r["stats0"]
    share = s["marginal"] / max(s["blended"], 1)
    print(f"{name}: C = {r['C']}, {r['hops']} hops, {s['pairs']} pairs ({s['outline_pairs']} outline), {s['blended']} blended "
          f"({s0['blended']} at zero hops), per hop {s['hits_per_hop']}, {s['marginal']} marginal ({100 * share:.2f} %)")
    assert s["blended"] > 0 and share <= MAX_MARGINAL and (s["blended"] >= 100 or s["marginal"] == 0)
    assert (sum(s["hits_per_hop"][1:]) > 0) == (name != "edges_70x70_b2")  # the edge mesh has boundary edges only
    assert s["pairs"] == r["stats32"]["pairs"] and torch.equal(s["hits"], r["stats32"]["hits"])
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
def test_walking_changes_the_pixels_the_restatement_names():
    """Fails without the feature: on the 64 x 64 sphere soft_silhouette(max_hops=4) differs from max_hops=0 at exactly the pixels
    at which the float64 restatement's two runs differ (91 more pairs blend; no pair of this case is marginal)."""
    from gif_amd import antialias as AA
    v, f, h, w, _ = aref.CASES["sphere_64x64_b1"]()
    vt, ft = torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda()
    sil0, sil4 = AA.soft_silhouette(vt, ft, h, w), AA.soft_silhouette(vt, ft, h, w, max_hops=4)
    vi, tri, depth = gpu_buffers(vt, ft, h, w)
    cov = (tri >= 0)[:, None].double().cpu()
    fv = aref.face_vertices_ref(vt.cpu().double(), vi.cpu(), f, h, w)
    adj = aref.edge_adjacency_ref(f)
    ref0, s0 = wref.antialias_walk_ref(cov, tri.cpu(), depth.cpu(), fv, adj, 0)
    ref4, s4 = wref.antialias_walk_ref(cov, tri.cpu(), depth.cpu(), fv, adj, 4)
    assert s4["marginal"] == 0 and (s0["blended"], s4["blended"]) == (79, 170)
    changed, named = (sil4 != sil0).cpu(), ref4 != ref0
    print(f"pixels changed by walking: kernels {int(changed.sum())}, restatement {int(named.sum())}")
    assert int(named.sum()) > 0 and int(changed.sum()) == int(named.sum()) and torch.equal(changed, named)


@pytest.mark.gpu
def test_zero_hops_keeps_the_existing_bits():
    """antialias(..., max_hops=0) is the call without the keyword, output and both gradients; the new entry points called with
    max_hops = 0 give the old entry points' forward and image-gradient bits."""
    from gif_amd import _lib
    from gif_amd import antialias as AA
    from gif_amd import standard_rasterize as sr
    lib, stream = _lib.load(), torch.cuda.current_stream().cuda_stream
    for name in ("sphere_70x90_b3", "edges_70x70_b2"):
        v, f, h, w, C = aref.CASES[name]()
        B, F = v.shape[0], len(f)
        ft = torch.from_numpy(f).cuda()
        gen = torch.Generator().manual_seed(12)
        image0, G = torch.rand((B, C, h, w), generator=gen).cuda(), torch.randn((B, C, h, w), generator=gen).cuda()
        vi, tri, depth = gpu_buffers(torch.from_numpy(v).cuda(), ft, h, w)
        got = []
        for kw in ({}, {"max_hops": 0}):
            vt, image = torch.from_numpy(v).cuda().requires_grad_(True), image0.clone().requires_grad_(True)
            out = AA.antialias(image, tri, depth, vt, ft, **kw)
            out.backward(G)
            got.append((out.detach(), image.grad, vt.grad))
        for a, b in zip(*got):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        assert not torch.equal(got[0][0], image0) and got[0][2].abs().sum() > 0
        # the entry points themselves
        fv = sr.face_vertices(vi, ft[None].expand(B, -1, -1)).contiguous()
        adj = AA.edge_adjacency(ft)
        outs = [torch.empty_like(image0) for _ in range(4)]
        ptr = lambda t: t.data_ptr()
        common = (ptr(tri), ptr(depth), ptr(fv), ptr(adj))
        _lib.check(lib.gif_antialias_f32(ptr(image0), *common, ptr(outs[0]), B, C, F, h, w, stream), "aa")
        _lib.check(lib.gif_antialias_walk_f32(ptr(image0), *common, ptr(outs[1]), B, C, F, h, w, 0, stream), "aa walk")
        _lib.check(lib.gif_antialias_bwd_f32(None, *common, ptr(G), ptr(outs[2]), None, B, C, F, h, w, None, stream), "aa bwd")
        _lib.check(lib.gif_antialias_walk_bwd_f32(None, *common, ptr(G), ptr(outs[3]), None, B, C, F, h, w, 0, None, stream), "aa walk bwd")
        torch.cuda.synchronize()
        assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)) and torch.equal(outs[0], got[0][0])
        assert torch.equal(outs[2].view(torch.int32), outs[3].view(torch.int32)) and torch.equal(outs[2], got[0][1])


@pytest.mark.gpu
def test_walking_adds_nothing_on_boundary_edges():
    """The edge mesh has boundary edges only: max_hops = 4 gives the zero-hop forward and image-gradient bits (its vertex gradient
    is summed in another order and is compared in test_forward_and_gradients_vs_fp64)."""
    from gif_amd import antialias as AA
    r = run_case("edges_70x70_b2")
    ft = torch.from_numpy(r["f"]).cuda()
    vt, image = torch.from_numpy(r["v"]).cuda(), r["image"].cuda().requires_grad_(True)
    out0 = AA.antialias(image, r["tri"], r["depth"], vt, ft)
    out0.backward(r["G"])
    assert torch.equal(out0.detach().view(torch.int32), r["out"][0].view(torch.int32))
    assert torch.equal(image.grad.view(torch.int32), r["gi"][0].view(torch.int32))


@pytest.mark.gpu
def test_backward_deterministic_and_only_requested_gradients():
    """Two runs of forward plus backward on the 24 x 30 sphere with 16 hops give the same bits of both gradients; either gradient
    alone equals its value when both are asked for."""
    from gif_amd import antialias as AA
    v, f, h, w, C, hops = wref.WALK_CASES["sphere24x30_70x90"]()
    ft = torch.from_numpy(f).cuda()
    gen = torch.Generator().manual_seed(5)
    image0, G = torch.rand((1, C, h, w), generator=gen).cuda(), torch.randn((1, C, h, w), generator=gen).cuda()
    _, tri, depth = gpu_buffers(torch.from_numpy(v).cuda(), ft, h, w)
    got = []
    for need_i, need_v in ((True, True), (True, True), (True, False), (False, True)):
        vt, image = torch.from_numpy(v).cuda().requires_grad_(need_v), image0.clone().requires_grad_(need_i)
        AA.antialias(image, tri, depth, vt, ft, max_hops=hops).backward(G)
        got.append((image.grad, vt.grad))
    assert torch.equal(got[0][0].view(torch.int32), got[1][0].view(torch.int32))
    assert torch.equal(got[0][1].view(torch.int32), got[1][1].view(torch.int32))
    assert got[0][1].abs().sum() > 0 and (got[0][0] != G).any()
    assert got[2][1] is None and got[3][0] is None
    assert torch.equal(got[0][0], got[2][0]) and torch.equal(got[0][1], got[3][1])


@pytest.mark.gpu
def test_rectangle_edge_through_a_face_that_does_not_own_it():
    """test_half_pixel_edges_return_the_rasterisers_bits' rectangle a quarter pixel to the right: with one hop the right edge's
    lowest row (front pixel in the lower-left triangle, which does not own that edge) reads 0.25 like the four above it."""
    from gif_amd import antialias as AA
    h = w = 16
    v, f = wref.quarter_rectangle()
    vt, ft = torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda()
    attr = torch.rand(1, 4, 3, generator=torch.Generator().manual_seed(3)).cuda()
    _, cov0 = AA.rasterize_attributes_aa(vt, ft, attr, h, w)
    _, cov1 = AA.rasterize_attributes_aa(vt, ft, attr, h, w, max_hops=1)
    assert cov0[0, 0, 7, 10].item() == 0
    assert torch.equal(cov1[0, 0, 3:8, 10], torch.full((5,), 0.25, device="cuda"))
    assert torch.equal(cov1[0, 0, 3:8, 4], torch.full((5,), 0.75, device="cuda"))
    assert torch.equal(AA.soft_silhouette(vt, ft, h, w, max_hops=1), cov1)


def _camera_fit(max_hops):
    from gif_amd import antialias as AA, render
    verts, f = wref.sphere(24, 30)
    X = torch.from_numpy(verts.astype(np.float32))[None].cuda()
    ft = torch.from_numpy(f).cuda()
    h = w = 48
    target_cam = torch.tensor([[0.6, 0.15, -0.1]], device="cuda")
    sil = lambda c: AA.soft_silhouette(render.batch_orth_proj(X, c), ft, h, w, max_hops=max_hops)
    with torch.no_grad():
        target = sil(target_cam)
    cam = torch.tensor([[0.45, -0.05, 0.08]], device="cuda", requires_grad=True)
    opt = torch.optim.Adam([cam], lr=0.02)
    losses = []
    for _ in range(60):
        opt.zero_grad()
        loss = ((sil(cam) - target) ** 2).sum()
        loss.backward()
        opt.step()
        losses.append(loss.item())
    with torch.no_grad():
        last = ((sil(cam) - target) ** 2).sum().item()
    return losses[0], last, (cam.detach() - target_cam).abs()[0].tolist()


@pytest.mark.gpu
def test_camera_fit_on_a_mesh_that_is_fine_for_its_image():
    """test_camera_fit_through_the_soft_silhouette's cameras, optimiser, 60 steps and conditions (conditions with slack, not
    measurements: final loss below 10 % of the start, every component within 0.03 of the target) on the 24 x 30 sphere at 48 x 48,
    whose faces next to the outline are narrower than a pixel, with max_hops = 16.  The same fit with zero hops is printed beside
    it and nothing is asserted about it."""
    first, last, err = _camera_fit(16)
    first0, last0, err0 = _camera_fit(0)
    print(f"camera fit, 16 hops: loss {first:.1f} -> {last:.2f}, camera error {err}")
    print(f"camera fit,  0 hops: loss {first0:.1f} -> {last0:.2f}, camera error {err0}")
    assert last < 0.1 * first and max(err) <= 0.03, (first, last, err)


@pytest.mark.gpu
def test_refusals():
    """max_hops of -1, 65 and 1.5 raise GifHipError; a double backward raises."""
    from gif_amd import _lib
    from gif_amd import antialias as AA
    v, f, h, w, C, hops = wref.WALK_CASES["border_grid_11x13"]()
    vt, ft = torch.from_numpy(v).cuda(), torch.from_numpy(f).cuda()
    _, tri, depth = gpu_buffers(vt, ft, h, w)
    image = torch.rand(1, C, h, w).cuda()
    for bad in (-1, 65, 1.5):
        with pytest.raises(_lib.GifHipError, match="max_hops"):
            AA.antialias(image, tri, depth, vt, ft, max_hops=bad)
        with pytest.raises(_lib.GifHipError, match="max_hops"):
            AA.soft_silhouette(vt, ft, h, w, max_hops=bad)
        with pytest.raises(_lib.GifHipError, match="max_hops"):
            AA.rasterize_attributes_aa(vt, ft, torch.zeros_like(vt), h, w, max_hops=bad)
    vg = vt.clone().requires_grad_(True)
    out = AA.antialias(image, tri, depth, vg, ft, max_hops=hops)
    (g,) = torch.autograd.grad(out.sum() * 0.5 + (out * out).sum(), vg, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable|differentiated twice|does not require grad"):
        g.sum().backward()
