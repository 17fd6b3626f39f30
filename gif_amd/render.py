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
    sample 0, shared by the batch).  Cached ON the faces tensor (attribute: no global cache keyed by an address that could be
    recycled) and validated like the packed weights (ops._cached_weight_op): by the in-place version counter AND the address and
    geometry of the data — `faces.data = other` keeps the counter, copy.deepcopy copies the attribute to a tensor with a counter of
    its own.  A write through `.data` into the same storage bumps no counter and moves no address: that one is the caller's to
    announce, with `del faces._gif_csr`."""
    key = (faces._version, faces.data_ptr(), tuple(faces.shape), tuple(faces.stride()), V, str(device))
    cached = getattr(faces, "_gif_csr", None)
    if cached is None or cached[0] != key:
        f2 = faces[0] if faces.ndimension() == 3 else faces
        f_cpu = f2.detach().cpu().numpy().astype(np.int64)
        if f_cpu.size and (f_cpu.min() < 0 or f_cpu.max() >= V):
            raise _lib.GifHipError(f"face index out of range [0,{V})")
        ent, counts = _topology_csr(f_cpu)
        off = np.zeros(V + 1, np.int32)
        off[1:len(counts) + 1] = np.cumsum(counts)[:V]
        off[len(counts) + 1:] = off[len(counts)]
        cached = (key,
                  (f2.to(device=device, dtype=torch.int32).contiguous(), torch.from_numpy(off).to(device),
                   torch.from_numpy(ent).to(device)))
        faces._gif_csr = cached
    return cached[1]


def _face_gather_bwd(gface, off, ent, V):
    """d face_vertices(x, faces) [B,F,3,3] -> d x [B,V,3]: per-vertex gather over the CSR (deterministic, no atomics); no face, no
    launch: exact zeros."""
    B, F = gface.shape[:2]
    if F == 0:
        return torch.zeros((B, V, 3), device=gface.device, dtype=torch.float32)
    out = torch.empty((B, V, 3), device=gface.device, dtype=torch.float32)
    _lib.launch("gif_face_gather_bwd_f32", gface.device, gface.contiguous(), off, ent, out, B, V, F)
    return out


def _batched_faces(faces, B):
    """faces [F,3] (a view, no copy) or [B,F,3] -> [B,F,3]"""
    return faces[None].expand(B, -1, -1) if faces.ndimension() == 2 else faces


def _projected_face_vertices(vertices_ndc, faces, h, w):
    """pixel-space face vertices [B,F,3,3] float32 of vertices_ndc [B,V,3]: what every rasteriser and antialias launch reads"""
    return sr.face_vertices(sr.to_image_space(vertices_ndc.float(), h, w), _batched_faces(faces, vertices_ndc.shape[0]))


def _one_topology(faces, B, what):
    if faces.ndimension() == 3 and B > 1 and faces.stride(0) != 0 and not torch.equal(faces, faces[:1].expand_as(faces)):
        raise _lib.GifHipError(f"{what} needs one face topology for the whole batch")


def _ndc_vertex_grad(gfv, faces, V, h, w, dtype):
    """d pixel-space face vertices [B,F,3,3] -> d vertices_ndc [B,V,3] in `dtype`: the face gather's transpose, then to_image_space's
    x * w/2 + w/2, y * h/2 + h/2; z only orders the faces (no gradient)."""
    _, off, ent = _topology(faces, V, gfv.device)
    gv = _face_gather_bwd(gfv, off, ent, V)
    gv *= torch.tensor([w / 2, h / 2, 0.0], device=gfv.device, dtype=torch.float32)
    return gv.to(dtype)


class _VertexNormalsFn(Function):
    @staticmethod
    def forward(ctx, vertices, f32, off, ent):
        B, V, _ = vertices.shape
        verts = vertices.contiguous().float()
        out = torch.empty_like(verts)
        _lib.launch("gif_vertex_normals_f32", verts.device, verts, f32, off, ent, out, B, V, f32.shape[0])
        ctx.save_for_backward(verts, f32, off, ent)
        ctx.in_dtype = vertices.dtype
        return out

    @staticmethod
    @once_differentiable  # raw kernel launch: a double backward must fail loudly, not return a history-free gradient
    def backward(ctx, gout):
        verts, f32, off, ent = ctx.saved_tensors
        B, V, _ = verts.shape
        work = torch.empty_like(verts)
        gv = torch.empty_like(verts)
        _lib.launch("gif_vertex_normals_bwd_f32", verts.device, verts, f32, off, ent, gout.contiguous().float(), work, gv, B, V,
                    f32.shape[0])
        return gv.to(ctx.in_dtype), None, None, None


def vertex_normals(vertices, faces):
    """[B,V,3] float32, faces [F,3] or [B,F,3] (same topology for every sample) -> unit normals [B,V,3].
    Differentiable with respect to `vertices` (gif_vertex_normals_bwd_f32)."""
    assert vertices.ndimension() == 3 and vertices.shape[2] == 3
    _lib.require_device("vertex_normals", vertices=vertices)
    f32, off, ent = _topology(faces, vertices.shape[1], vertices.device)
    return _VertexNormalsFn.apply(vertices, f32, off, ent)


def batch_orth_proj(X, camera):
    """Orthographic camera [s, tx, ty]: s * (X.xy + t), z scaled by s  (mesh_and_3d_helpers.py:40-50)."""
    camera = camera.clone().view(-1, 1, 3)
    X_trans = torch.cat([X[:, :, :2] + camera[:, :, 1:], X[:, :, 2:]], 2)
    return camera[:, :, 0:1] * X_trans


class _RasterizeColorsFn(Function):
    """The one owner of gif_rasterize_colors_f32 and gif_rasterize_colors_bwd_f32: (image [B,3,h,w], mask [B,1,h,w], tri [B,h,w],
    depth [B,h,w]), the last three without a gradient.  per_vertex: `attributes` [B,Va,3] are gathered through `faces`; else they
    are given per face corner, [F,3,3] (shared by the batch) or [B,F,3,3].  `what` names the caller in a refusal."""

    @staticmethod
    def forward(ctx, vertices_ndc, attributes, faces, h, w, per_vertex, what):
        B = vertices_ndc.shape[0]
        fv = _projected_face_vertices(vertices_ndc, faces, h, w)
        fc = attributes.float()
        if per_vertex:
            fc = sr.face_vertices(fc.contiguous(), _batched_faces(faces, B))
        else:
            fc = (fc[None].expand(B, -1, -1, -1) if fc.ndimension() == 3 else fc).contiguous()
        depth, tri, img = sr.new_buffers(B, h, w, vertices_ndc.device)
        sr.standard_rasterize_colors(fv, fc, depth, tri, img, h, w)
        mask = (tri >= 0)[:, None]
        ctx.mark_non_differentiable(mask, tri, depth)
        ctx.set_materialize_grads(False)  # no zero tensors (a fill launch each) for the three outputs that carry no gradient
        ctx.save_for_backward(fv, fc, tri)
        ctx.faces, ctx.hw, ctx.per_vertex, ctx.what = faces, (h, w), per_vertex, what
        ctx.dtypes = (vertices_ndc.dtype, attributes.dtype)
        ctx.V, ctx.attr_shape = vertices_ndc.shape[1], attributes.shape
        return img.permute(0, 3, 1, 2).contiguous(), mask, tri, depth

    @staticmethod
    @once_differentiable  # raw kernel launch: a double backward must fail loudly, not return a history-free gradient
    def backward(ctx, gimg, _gmask, _gtri, _gdepth):
        fv, fc, tri = ctx.saved_tensors
        faces, (h, w) = ctx.faces, ctx.hw
        need_v, need_a = ctx.needs_input_grad[:2]
        B, F = fv.shape[:2]
        _one_topology(faces, B, ctx.what + " backward")
        g = gimg.float().permute(0, 2, 3, 1).contiguous()  # [B,H,W,3]: the forward's image buffer layout
        gfv = torch.empty_like(fv) if need_v else None
        gfc = torch.empty_like(fc) if need_a else None
        ws = _lib.workspace(_lib.load().gif_rasterize_colors_bwd_workspace_bytes(B, F, h, w), fv.device)
        _lib.launch("gif_rasterize_colors_bwd_f32", fv.device, fv, fc, tri, g, gfv, gfc, B, F, h, w, ws)
        gv = _ndc_vertex_grad(gfv, faces, ctx.V, h, w, ctx.dtypes[0]) if need_v else None
        ga = None
        if need_a and ctx.per_vertex:
            Va = ctx.attr_shape[1]
            ga = _face_gather_bwd(gfc, *_topology(faces, Va, fv.device)[1:], Va).to(ctx.dtypes[1])
        elif need_a:
            ga = (gfc.sum(0) if len(ctx.attr_shape) == 3 else gfc).to(ctx.dtypes[1])
        return gv, ga, None, None, None, None, None


def rasterize_attributes(vertices_ndc, faces, attributes, h, w):
    """Barycentric interpolation of per-vertex attributes [B,V,3] over the z-buffered mesh -> images [B,3,h,w], plus
    the coverage mask [B,1,h,w].  vertices_ndc: x,y in [-1,1], any z (visibility.py:38-44 conventions).
    Differentiable with respect to vertices_ndc (x, y) and attributes inside each pixel's winning face
    (gif_rasterize_colors_bwd_f32); no silhouette, occlusion-boundary or depth gradient.  The mask has no gradient.
    gif_amd.antialias.rasterize_attributes_aa is the opt-in variant whose outline carries a gradient."""
    return _RasterizeColorsFn.apply(vertices_ndc, attributes, faces, h, w, True, "rasterize_attributes")[:2]


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
