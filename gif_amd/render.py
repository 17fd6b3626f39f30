"""Condition-render pipeline around the rasteriser: projected mesh -> 6-channel condition image.

Mirrors the pieces of the reference that exist in-tree:
  vertex_normals / batch_orth_proj       model/mesh_and_3d_helpers.py:5-50
  NDC -> pixel transform, buffer init    my_utils/standard_rasterize_cuda/visibility.py:38-44
  8-bit quantisation of the renders      my_utils/visualize_flame_overlay.py:29-31  (floor(clamp*255)/255)
  [-1,1] scaling and channel order       plots/generate_random_samples.py:22-30, :188-189  (cat(texture, normal))
The FLAME layer lives in the reference's absent `photometric_optimization` submodule; its algorithm is public and is built
here as gif_amd.flame.FlameLayer (HIP forward and backward) — only the licensed model file stays outside.  The
per-vertex "texture" attribute is an INPUT here; the condition GIF actually uses — the FLAME albedo texture lit by spherical
harmonics — is gif_amd.shading.render_shaded_condition, built on the same rasteriser passes.
Kernels: gif_vertex_normals_f32 (gather, deterministic) and gif_rasterize_colors_f32, both behind the C ABI.
Backward (differentiable condition rendering): gif_vertex_normals_bwd_f32, gif_rasterize_colors_bwd_f32 and
gif_face_gather_bwd_f32, all deterministic (no float atomics).
"""
import numpy as np
import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _lib
from . import standard_rasterize as sr


def _topology_csr(faces_cpu: np.ndarray):
    """vertex -> (face, corner) entries ordered like the reference's index_add_ passes: corner 1, 2, 0; faces ascending."""
    F = faces_cpu.shape[0]
    V = int(faces_cpu.max()) + 1 if F else 0
    ents, verts = [], []
    for rank, corner in enumerate((1, 2, 0)):
        ents.append(np.arange(F, dtype=np.int64) * 4 + corner)
        verts.append(faces_cpu[:, corner].astype(np.int64))
    ents, verts = np.concatenate(ents), np.concatenate(verts)
    order = np.argsort(verts, kind="stable")  # stable: keeps (pass, face) order inside a vertex
    counts = np.bincount(verts, minlength=V)
    return ents[order].astype(np.int32), counts


def _topology(faces, V, device):
    """(faces [F,3] int32, CSR offsets [V+1], CSR entries [3F]) on `device` for faces [F,3] or [B,F,3] (the topology of
    sample 0, shared by the batch).  Cached ON the faces tensor (attribute), validated by its in-place version counter: no
    global cache keyed by an address that could be recycled."""
    cached = getattr(faces, "_gif_csr", None)
    if cached is None or cached[0] != (faces._version, V, str(device)):
        f2 = faces[0] if faces.ndimension() == 3 else faces
        f_cpu = f2.detach().cpu().numpy().astype(np.int64)
        if f_cpu.size and (f_cpu.min() < 0 or f_cpu.max() >= V):
            raise _lib.GifHipError(f"face index out of range [0,{V})")
        ent, counts = _topology_csr(f_cpu)
        off = np.zeros(V + 1, np.int32)
        off[1:len(counts) + 1] = np.cumsum(counts)[:V]
        off[len(counts) + 1:] = off[len(counts)]
        cached = ((faces._version, V, str(device)),
                  (f2.to(device=device, dtype=torch.int32).contiguous(), torch.from_numpy(off).to(device),
                   torch.from_numpy(ent).to(device)))
        faces._gif_csr = cached
    return cached[1]


def _face_gather_bwd(gface, off, ent, V):
    """d face_vertices(x, faces) [B,F,3,3] -> d x [B,V,3]: per-vertex gather over the CSR (deterministic, no atomics)."""
    B, F = gface.shape[:2]
    gface = gface.contiguous()
    out = torch.empty((B, V, 3), device=gface.device, dtype=torch.float32)
    _lib.check(_lib.load().gif_face_gather_bwd_f32(gface.data_ptr(), off.data_ptr(), ent.data_ptr(), out.data_ptr(), B, V, F,
                                                    torch.cuda.current_stream().cuda_stream), "face_gather_bwd")
    return out


class _VertexNormalsFn(Function):
    @staticmethod
    def forward(ctx, vertices, f32, off, ent):
        B, V, _ = vertices.shape
        verts = vertices.contiguous().float()
        out = torch.empty_like(verts)
        lib = _lib.load()
        with torch.cuda.device(verts.device):  # launch on the operands' device and its current stream
            _lib.check(lib.gif_vertex_normals_f32(verts.data_ptr(), f32.data_ptr(), off.data_ptr(), ent.data_ptr(),
                                                  out.data_ptr(), B, V, f32.shape[0],
                                                  torch.cuda.current_stream().cuda_stream), "vertex_normals")
        ctx.save_for_backward(verts, f32, off, ent)
        ctx.in_dtype = vertices.dtype
        return out

    @staticmethod
    @once_differentiable  # raw kernel launch: a double backward must fail loudly, not return a history-free gradient
    def backward(ctx, gout):
        verts, f32, off, ent = ctx.saved_tensors
        B, V, _ = verts.shape
        gout = gout.contiguous().float()
        work = torch.empty_like(verts)
        gv = torch.empty_like(verts)
        with torch.cuda.device(verts.device):
            _lib.check(_lib.load().gif_vertex_normals_bwd_f32(verts.data_ptr(), f32.data_ptr(), off.data_ptr(),
                                                              ent.data_ptr(), gout.data_ptr(), work.data_ptr(), gv.data_ptr(),
                                                              B, V, f32.shape[0], torch.cuda.current_stream().cuda_stream),
                       "vertex_normals_bwd")
        return gv.to(ctx.in_dtype), None, None, None


def vertex_normals(vertices, faces):
    """[B,V,3] float32, faces [F,3] or [B,F,3] (same topology for every sample) -> unit normals [B,V,3].
    Differentiable with respect to `vertices` (gif_vertex_normals_bwd_f32)."""
    assert vertices.ndimension() == 3 and vertices.shape[2] == 3
    if not vertices.is_cuda:
        raise _lib.GifHipError("vertex_normals needs device tensors (no CPU fallback)")
    f32, off, ent = _topology(faces, vertices.shape[1], vertices.device)
    return _VertexNormalsFn.apply(vertices, f32, off, ent)


def batch_orth_proj(X, camera):
    """Orthographic camera [s, tx, ty]: s * (X.xy + t), z scaled by s  (mesh_and_3d_helpers.py:40-50)."""
    camera = camera.clone().view(-1, 1, 3)
    X_trans = torch.cat([X[:, :, :2] + camera[:, :, 1:], X[:, :, 2:]], 2)
    return camera[:, :, 0:1] * X_trans


def _rasterize_colors(vertices_ndc, faces, face_colors_of, h, w, with_depth=False):
    """The forward both attribute rasterisers share: (fv, fc, tri, image [B,3,h,w], mask [B,1,h,w]); `face_colors_of(faces_b)`
    gives the per-face-corner attributes [B,F,3,3].  with_depth=True appends the depth buffer [B,h,w] (gif_amd.antialias)."""
    B = vertices_ndc.shape[0]
    faces_b = faces[None].expand(B, -1, -1) if faces.ndimension() == 2 else faces
    v = sr.to_image_space(vertices_ndc.float(), h, w)
    fv = sr.face_vertices(v, faces_b)
    fc = face_colors_of(faces_b)
    depth, tri, img = sr.new_buffers(B, h, w, vertices_ndc.device)
    sr.standard_rasterize_colors(fv, fc, depth, tri, img, h, w)
    out = (fv, fc, tri, img.permute(0, 3, 1, 2).contiguous(), (tri >= 0)[:, None])
    return out + (depth,) if with_depth else out


def _rasterize_colors_bwd(fv, fc, tri, gimg, faces, V, vdtype, h, w, need_v, need_c, what):
    """d image -> (d vertices_ndc [B,V,3] in `vdtype` or None, d face colours [B,F,3,3] or None): gif_rasterize_colors_bwd_f32,
    then for the vertices the face gather's transpose and the NDC -> pixel scaling."""
    B, F = fv.shape[:2]
    if faces.ndimension() == 3 and B > 1 and faces.stride(0) != 0 and not torch.equal(faces, faces[:1].expand_as(faces)):
        raise _lib.GifHipError(f"{what} backward needs one face topology for the whole batch")
    dev = fv.device
    lib = _lib.load()
    g = gimg.float().permute(0, 2, 3, 1).contiguous()  # [B,H,W,3]: the forward's image buffer layout
    gfv = torch.empty_like(fv) if need_v else None
    gfc = torch.empty_like(fc) if need_c else None
    ws = torch.empty((max(lib.gif_rasterize_colors_bwd_workspace_bytes(B, F, h, w) // 4, 1),), device=dev,
                     dtype=torch.float32)
    gv = None
    with torch.cuda.device(dev):
        _lib.check(lib.gif_rasterize_colors_bwd_f32(fv.data_ptr(), fc.data_ptr(), tri.data_ptr(), g.data_ptr(),
                                                    gfv.data_ptr() if need_v else None,
                                                    gfc.data_ptr() if need_c else None, B, F, h, w, ws.data_ptr(),
                                                    torch.cuda.current_stream().cuda_stream), "rasterize_colors_bwd")
        if need_v:
            _, off, ent = _topology(faces, V, dev)
            gv = _face_gather_bwd(gfv, off, ent, V)
            # to_image_space: x * w/2 + w/2, y * h/2 + h/2; z only orders the faces (no gradient)
            gv *= torch.tensor([w / 2, h / 2, 0.0], device=dev, dtype=torch.float32)
            gv = gv.to(vdtype)
    return gv, gfc


class _RasterizeAttributesFn(Function):
    @staticmethod
    def forward(ctx, vertices_ndc, attributes, faces, h, w):
        fv, fc, tri, img, mask = _rasterize_colors(
            vertices_ndc, faces, lambda faces_b: sr.face_vertices(attributes.float().contiguous(), faces_b), h, w)
        ctx.mark_non_differentiable(mask)
        ctx.save_for_backward(fv, fc, tri)
        ctx.faces, ctx.hw = faces, (h, w)
        ctx.dtypes = (vertices_ndc.dtype, attributes.dtype)
        ctx.V = (vertices_ndc.shape[1], attributes.shape[1])
        return img, mask

    @staticmethod
    @once_differentiable  # raw kernel launch: a double backward must fail loudly, not return a history-free gradient
    def backward(ctx, gimg, _gmask):
        fv, fc, tri = ctx.saved_tensors
        faces, (h, w) = ctx.faces, ctx.hw
        need_v, need_a = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        gv, gfc = _rasterize_colors_bwd(fv, fc, tri, gimg, faces, ctx.V[0], ctx.dtypes[0], h, w, need_v, need_a,
                                        "rasterize_attributes")
        ga = None
        if need_a:
            with torch.cuda.device(fv.device):
                _, off, ent = _topology(faces, ctx.V[1], fv.device)
                ga = _face_gather_bwd(gfc, off, ent, ctx.V[1]).to(ctx.dtypes[1])
        return gv, ga, None, None, None


def rasterize_attributes(vertices_ndc, faces, attributes, h, w):
    """Barycentric interpolation of per-vertex attributes [B,V,3] over the z-buffered mesh -> images [B,3,h,w], plus
    the coverage mask [B,1,h,w].  vertices_ndc: x,y in [-1,1], any z (visibility.py:38-44 conventions).
    Differentiable with respect to vertices_ndc (x, y) and attributes inside each pixel's winning face
    (gif_rasterize_colors_bwd_f32); no silhouette, occlusion-boundary or depth gradient.  The mask has no gradient.
    gif_amd.antialias.rasterize_attributes_aa is the opt-in variant whose outline carries a gradient."""
    return _RasterizeAttributesFn.apply(vertices_ndc, attributes, faces, h, w)


def quantize_8bit(img01):
    """floor(clamp(x,0,1)*255)/255 — the reference's render post-processing (visualize_flame_overlay.py:29-31)."""
    return torch.floor(img01.clamp(0, 1) * 255) / 255.0


def _quantize_straight_through(img01):
    """quantize_8bit's values, identity gradient: q + (x - x) is exactly q, and its derivative with respect to x is 1."""
    return quantize_8bit(img01.detach()) + (img01 - img01.detach())


def render_condition(vertices_ndc, faces, vertex_texture, h=256, w=256, straight_through=False):
    """6-channel generator condition: cat(texture render, normal render) in [-1,1] (generate_random_samples.py:22-30,
    :188-189).  Normals are mapped to [0,1] as n*0.5+0.5 before the 8-bit quantisation (normal-map convention).
    Differentiable with respect to vertices_ndc and vertex_texture; the floor quantisation has a zero gradient, so
    straight_through=True passes gradients through it unchanged (forward values are the same either way)."""
    quant = _quantize_straight_through if straight_through else quantize_8bit
    normals = vertex_normals(vertices_ndc, faces)
    normal_img, _ = rasterize_attributes(vertices_ndc, faces, normals * 0.5 + 0.5, h, w)
    tex_img, _ = rasterize_attributes(vertices_ndc, faces, vertex_texture, h, w)
    normal_img = quant(normal_img) * 2 - 1
    tex_img = quant(tex_img) * 2 - 1
    return torch.cat((tex_img, normal_img), dim=1)


class FlameConditionRenderer:
    """callable flame_batch [N, >=159] -> (rend_flm, norma_map_img), both [N,3,h,w] in [-1,1]: the role
    OverLayViz.get_rendered_mesh + the [-1,1] scaling play in InterpolatedTextureLoss.get_image_and_textures
    (loss_functions/losses.py:184-215).  `flame` is the FLAME layer: gif_amd.flame.FlameLayer over a converted model file or
    over flame.synthetic_flame_model (differentiable with respect to shape, expression and pose), any callable with its
    signature, or gif_amd.data.SyntheticFlame, the benchmark's fixed stand-in.  `vertex_texture` [V,3] in [0,1] is a fixed per-vertex
    colour in place of the SH-lit albedo render; gif_amd.shading.ShadedFlameConditionRenderer renders that one from columns
    159:236 of the labels."""

    def __init__(self, flame, faces, vertex_texture, h=256, w=256, straight_through=False):
        self.flame, self.faces, self.vertex_texture, self.h, self.w = flame, faces, vertex_texture, h, w
        self.straight_through = straight_through  # render_condition's: gradients through the 8-bit quantisation

    def vertices(self, flame_batch):
        """(FLAME vertices, vertices in NDC with the y flip of stg2_generator.py:368, camera)."""
        shape, exp = flame_batch[:, 0:100], flame_batch[:, 100:150]
        pose, cam = flame_batch[:, 150:156], flame_batch[:, 156:159]
        verts, _, _ = self.flame(shape_params=shape, expression_params=exp, pose_params=pose)
        trans = batch_orth_proj(verts, cam)
        return verts, torch.cat([trans[:, :, :1], -trans[:, :, 1:]], 2), cam

    def __call__(self, flame_batch):
        _, v_ndc, _ = self.vertices(flame_batch)
        tex = self.vertex_texture[None].expand(v_ndc.shape[0], -1, -1)
        cond = render_condition(v_ndc, self.faces, tex, self.h, self.w, straight_through=self.straight_through)
        return cond[:, :3], cond[:, 3:]
