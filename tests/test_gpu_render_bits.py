"""-m gpu: every output and gradient of the mesh and render bindings (gif_amd.render, antialias, shading, texture_space, flame) is
bit-identical to the recorded one.

These bindings launch deterministic kernels (no float atomics, fixed reduction orders), so a change of the host side around the
launches — who marshals the arguments, which autograd Function owns a launch, where the mesh plumbing lives — must keep every bit.
Only public API is driven, so this file runs unchanged at any commit.  tests/golden/render_crc_golden.json holds the CRC-32 of each
result's bytes (the dtype is part of the bytes: a gradient that came back in another dtype does not match), written by
tests/golden/make_render_crc_golden.py from the commit before the bindings were gathered behind _lib.launch (two runs agreed on
every case).  Never hashed: the two gradients the library accumulates with float atomics (include/gif_hip.h names both) — the one
to `albedo` (gif_shade_sh_bwd_f32; tests/test_gpu_shading.py compares it in fp64) and the one to the texture map's source image
(gif_texture_map_bwd_f32: two runs of the recorded commit gave CRCs 202435531 and 1985661101; tests/test_gpu_kernels.py and
tests/test_gpu_render_edges.py compare it with the reference's).  Both are asked for, so that their launches are exercised.

Shapes: B = 2, images of 48 x 64 (h != w: a swapped pair shows in the [w/2, h/2, 0] scaling and in the kernel arguments); the
216-face sphere and the 11-face edge mesh of tests/antialias_ref.py; a 16 x 16 albedo; flame.synthetic_flame_model over the
sphere's 110 vertices with 3 shape and 2 expression columns; the texture map's fixed T = 256 from a 24 x 32 source image.
SIDE_STREAM: one case of each module runs again on a side stream and must give the default stream's CRCs (a launch that read the
stream outside its device guard, or not at all, would race the inputs' producers or give other bits).
The F == 0 cases are asserted directly as well (exact zeros of the right shape and dtype): see test_no_faces_give_exact_zeros.
"""
import itertools
import json
import os
import zlib

import numpy as np
import pytest
import torch

import antialias_ref as aref  # (pytest puts this directory on sys.path)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "render_crc_golden.json")
B, H, W, T_ALB = 2, 48, 64, 16


def _crc(t):
    return zlib.crc32(t.detach().contiguous().cpu().numpy().tobytes())


def _rand(seed, *shape, lo=0.0, hi=1.0):
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed)) * (hi - lo) + lo


def _mesh(kind, faces_dim=2, dtype=torch.float32):
    """(vertices_ndc [B,V,3] on the device, faces [F,3] or [B,F,3] int64 on the device)"""
    v, f = aref.sphere_case(B) if kind == "sphere" else aref.edge_mesh(B, H)
    f = torch.from_numpy(f)
    if kind == "none":
        f = f[:0]
    if faces_dim == 3:
        f = f[None].expand(B, -1, -1).contiguous()
    return torch.from_numpy(v).to(dtype).cuda(), f.cuda()


def _grads(outs_and_ups, inputs):
    """{name: gradient} of sum_i (out_i * up_i) for the inputs {name: leaf} (one backward pass)."""
    names = list(inputs)
    gs = torch.autograd.grad([o for o, _ in outs_and_ups], [inputs[n] for n in names], [u for _, u in outs_and_ups])
    return {"g_" + n: g for n, g in zip(names, gs)}


def _up(seed, like):
    return torch.randn(like.shape, generator=torch.Generator().manual_seed(seed)).to(like.dtype).cuda()


# --------------------------------------------------------------------------------------------------------------------- render
def c_raster(mesh, faces_dim, need):
    from gif_amd import render
    v, f = _mesh(mesh, faces_dim, torch.float64)  # float64 in: the vertex gradient must come back float64
    a = _rand(1, *v.shape).cuda()
    leaves = {k: t.requires_grad_(True) for k, t in (("v", v), ("a", a)) if k in need}
    img, mask = render.rasterize_attributes(v, f, a, H, W)
    out = {"img": img, "mask": mask, **_grads([(img, _up(2, img))], leaves)}
    assert out.get("g_v", v).dtype == torch.float64 and out.get("g_a", a).dtype == torch.float32
    return out


def c_normals(mesh, faces_dim):
    from gif_amd import render
    v, f = _mesh(mesh, faces_dim, torch.float64)
    v.requires_grad_(True)
    n = render.vertex_normals(v, f)
    out = {"normals": n, **_grads([(n, _up(3, n))], {"v": v})}
    assert out["g_v"].dtype == torch.float64
    return out


def c_condition():
    from gif_amd import render
    v, f = _mesh("sphere")
    tex = _rand(4, *v.shape).cuda()
    v.requires_grad_(True), tex.requires_grad_(True)
    cond = render.render_condition(v, f, tex, H, W, straight_through=True)
    return {"cond": cond, **_grads([(cond, _up(5, cond))], {"v": v, "tex": tex})}


# -------------------------------------------------------------------------------------------------------------------- shading
def c_face_attributes(shared):
    from gif_amd import shading
    v, f = _mesh("sphere", dtype=torch.float64)
    fa = _rand(6, *((() if shared else (B,)) + (f.shape[0], 3, 3))).cuda()
    v.requires_grad_(True), fa.requires_grad_(True)
    img, mask = shading.rasterize_face_attributes(v, f, fa, H, W)
    out = {"img": img, "mask": mask, **_grads([(img, _up(7, img))], {"v": v, "fa": fa})}
    assert out["g_v"].dtype == torch.float64 and out["g_fa"].shape == fa.shape
    return out


SH_INPUTS = ("uv", "nrm", "alb", "sh")


def c_sh_shade(Ba):
    """the forward, then the backward for every non-empty subset of the four differentiable inputs"""
    from gif_amd import shading
    base = {"uv": _rand(8, B, 3, H, W, lo=-1.1, hi=1.1), "nrm": _rand(9, B, 3, H, W), "alb": _rand(10, Ba, 3, T_ALB, T_ALB),
            "sh": _rand(11, B, 9, 3, lo=-1.0)}
    mask = (_rand(12, B, 1, H, W) > 0.3).cuda()
    out = {}
    for n in range(1, 5):
        for need in itertools.combinations(SH_INPUTS, n):
            x = {k: t.clone().cuda().requires_grad_(k in need) for k, t in base.items()}
            y = shading.sh_shade(x["uv"], x["nrm"], mask, x["alb"], x["sh"], nrm_mul=2.0, nrm_add=-1.0)
            out.setdefault("shaded", y)
            for k, g in _grads([(y, _up(13, y))], {k: x[k] for k in need}).items():
                if k != "g_alb":  # float atomics: not reproducible
                    out[f"{k}@{'+'.join(need)}"] = g
    return out


def c_shaded_condition():
    from gif_amd import shading
    v, f = _mesh("sphere")
    uvs = shading.synthetic_face_uvs(aref.small_sphere()[0], aref.small_sphere()[1], seed=1).cuda()
    alb, sh = _rand(14, 1, 3, T_ALB, T_ALB).cuda(), _rand(15, B, 9, 3, lo=-1.0).cuda()
    leaves = {"v": v, "uvs": uvs, "alb": alb, "sh": sh}
    for t in leaves.values():
        t.requires_grad_(True)
    cond = shading.render_shaded_condition(v, f, uvs, alb, sh, H, W, straight_through=True)
    g = _grads([(cond, _up(16, cond))], leaves)
    del g["g_alb"]  # float atomics: not reproducible
    return {"cond": cond, **g}


# ------------------------------------------------------------------------------------------------------------------ antialias
def _buffers(v, f):
    """tri and depth as the rasteriser leaves them, through the drop-in module's public calls"""
    from gif_amd import standard_rasterize as sr
    fb = f[None].expand(B, -1, -1) if f.ndimension() == 2 else f
    fv = sr.face_vertices(sr.to_image_space(v.float(), H, W), fb)
    depth, tri, bary = sr.new_buffers(B, H, W, v.device)
    sr.standard_rasterize(fv, depth, tri, bary, H, W)
    return tri, depth


def c_antialias(mesh, hops, need):
    from gif_amd import antialias as AA
    v, f = _mesh(mesh, dtype=torch.float64)
    tri, depth = _buffers(v, f)
    image = _rand(17, B, 4, H, W).double().cuda()
    leaves = {k: t.requires_grad_(True) for k, t in (("image", image), ("v", v)) if k == need}
    y = AA.antialias(image, tri, depth, v, f, max_hops=hops)
    out = {"out": y, **_grads([(y, _up(18, y))], leaves)}
    assert all(g.dtype == torch.float64 for g in out.values())
    return out


def c_raster_aa(hops, need):
    from gif_amd import antialias as AA
    v, f = _mesh("sphere", dtype=torch.float64)
    a = _rand(19, *v.shape).cuda()
    leaves = {k: t.requires_grad_(True) for k, t in (("a", a), ("v", v)) if k == need}
    img, cov = AA.rasterize_attributes_aa(v, f, a, H, W, max_hops=hops)
    return {"img": img, "cov": cov, **_grads([(img, _up(20, img)), (cov, _up(21, cov))], leaves)}


def c_silhouette(mesh, hops):
    from gif_amd import antialias as AA
    v, f = _mesh(mesh, dtype=torch.float64)
    v.requires_grad_(True)
    cov = AA.soft_silhouette(v, f, H, W, max_hops=hops)
    return {"cov": cov, **_grads([(cov, _up(22, cov))], {"v": v})}


# -------------------------------------------------------------------------------------------------------------- texture_space
def c_texture_map():
    from gif_amd.texture_space import FlameTextureSpace
    from test_oracle_texture import load_fixture
    g, td, verts, normals = load_fixture()
    fts = FlameTextureSpace(td, None).cuda()
    img = _rand(23, 2, 3, 24, 32, lo=-1.0).cuda().requires_grad_(True)
    tex, mask = fts.compute_texture_map(img, verts.cuda(), normals.cuda(), camera_params=torch.from_numpy(g["cam"]).cuda())
    _grads([(tex, _up(24, tex))], {"img": img})  # launched, not hashed: float atomics, like the albedo gradient
    return {"tex": tex, "mask": mask}


# ---------------------------------------------------------------------------------------------------------------------- flame
def c_flame(landmarks, grad):
    from gif_amd import flame as fl
    tmpl, faces = aref.small_sphere()
    emb = fl.synthetic_landmark_embedding(faces, n_dynamic=3, n_static=5, n_full=4, n_rows=5) if landmarks else None
    layer = fl.FlameLayer(fl.synthetic_flame_model(tmpl, 3, 2), 3, 2, landmarks=emb).cuda()
    x = {k: (_rand(25 + i, B, n, lo=-1.0) * s).cuda().requires_grad_(grad)
         for i, (k, n, s) in enumerate((("shape", 3, 1.0), ("exp", 2, 1.0), ("pose", 6, 0.2), ("neck", 3, 0.2), ("eye", 6, 0.2)))}
    with torch.set_grad_enabled(grad):
        outs = layer(*x.values())
    out = {k: t for k, t in zip(("verts", "lmk2d", "lmk3d"), outs) if t is not None}
    assert len(out) == (3 if landmarks else 1)
    if grad:
        out.update(_grads([(t, _up(30 + i, t)) for i, t in enumerate(out.values())], x))
    return out


CASES = {}
for _fd, _need in itertools.product((2, 3), ("v", "a", "va")):
    CASES[f"raster-sphere-f{_fd}-{_need}"] = (c_raster, "sphere", _fd, _need)
CASES["raster-edges-f2-va"] = (c_raster, "edges", 2, "va")
CASES["raster-none-f2-va"] = (c_raster, "none", 2, "va")
for _fd in (2, 3):
    CASES[f"normals-sphere-f{_fd}"] = (c_normals, "sphere", _fd)
CASES["normals-edges-f2"] = (c_normals, "edges", 2)
CASES["condition"] = (c_condition,)
CASES["face_attributes-shared"] = (c_face_attributes, True)
CASES["face_attributes-per_sample"] = (c_face_attributes, False)
CASES["sh_shade-ba1"] = (c_sh_shade, 1)
CASES[f"sh_shade-ba{B}"] = (c_sh_shade, B)
CASES["shaded_condition"] = (c_shaded_condition,)
for _hops, _need in itertools.product((0, 3), ("image", "v")):
    CASES[f"antialias-sphere-h{_hops}-{_need}"] = (c_antialias, "sphere", _hops, _need)
    CASES[f"raster_aa-h{_hops}-{'a' if _need == 'image' else 'v'}"] = (c_raster_aa, _hops, "a" if _need == "image" else "v")
for _hops in (0, 3):
    CASES[f"antialias-edges-h{_hops}-v"] = (c_antialias, "edges", _hops, "v")
    CASES[f"silhouette-sphere-h{_hops}"] = (c_silhouette, "sphere", _hops)
    CASES[f"antialias-none-h{_hops}-v"] = (c_antialias, "none", _hops, "v")
    CASES[f"silhouette-none-h{_hops}"] = (c_silhouette, "none", _hops)
CASES["texture_map"] = (c_texture_map,)
for _lmk, _grad in itertools.product((False, True), (False, True)):
    CASES[f"flame-{'lmk' if _lmk else 'plain'}-{'grad' if _grad else 'nograd'}"] = (c_flame, _lmk, _grad)

# one case of render, antialias, shading, texture_space and flame each (the flame no-grad case: its two launches share one stream)
SIDE_STREAM = ["raster-sphere-f2-va", "antialias-sphere-h3-v", "sh_shade-ba1", "texture_map", "flame-lmk-nograd", "flame-lmk-grad"]
NO_FACES = [n for n in CASES if "-none-" in n]


def run_case(name, side_stream=False):
    """{result name: tensor} of one case, on the default stream or on a fresh side stream (synchronised before and after)"""
    fn, *args = CASES[name]
    torch.cuda.synchronize()
    if side_stream:
        with torch.cuda.stream(torch.cuda.Stream()):
            out = fn(*args)
    else:
        out = fn(*args)
    torch.cuda.synchronize()
    return out


def render_crcs(name, side_stream=False):
    return {k: _crc(t) for k, t in run_case(name, side_stream).items()}


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_render_bits_match_the_recorded_ones(name):
    golden = _golden()
    assert name in golden, f"{name}: no recorded CRCs (tests/golden/make_render_crc_golden.py)"
    got = render_crcs(name)
    assert got == golden[name], f"{name}: CRCs {got}, recorded {golden[name]}: the bindings' bits changed"


@pytest.mark.gpu
@pytest.mark.parametrize("name", SIDE_STREAM)
def test_side_stream_gives_the_default_streams_bits(name):
    got = render_crcs(name, side_stream=True)
    assert got == _golden()[name], f"{name} on a side stream: CRCs {got}, recorded {_golden()[name]}"


@pytest.mark.gpu
@pytest.mark.parametrize("name", NO_FACES)
def test_no_faces_give_exact_zeros(name):
    """F == 0: nothing is covered and no gradient reaches a vertex or an attribute — exact zeros [B,V,3] in the input's dtype"""
    out = run_case(name)
    V = aref.edge_mesh(B, H)[0].shape[1]
    for k, dtype in (("g_v", torch.float64), ("g_a", torch.float32)):
        if k in out:
            assert out[k].shape == (B, V, 3) and out[k].dtype == dtype and not out[k].any(), (name, k)
    if "img" in out:
        assert not out["img"].any() and not out["mask"].any()
    if "cov" in out:
        assert out["cov"].shape == (B, 1, H, W) and not out["cov"].any()


def test_every_case_is_recorded():
    golden = _golden()
    assert sorted(golden) == sorted(CASES)
    assert set(SIDE_STREAM) <= set(CASES) and len(NO_FACES) == 5
    assert not any("alb" in k.split("@")[0] for rec in golden.values() for k in rec), "the albedo gradient is never hashed"
    zeros = zlib.crc32(np.zeros((B, aref.edge_mesh(B, H)[0].shape[1], 3), np.float64).tobytes())
    assert all(golden[n]["g_v"] == zeros for n in NO_FACES)
