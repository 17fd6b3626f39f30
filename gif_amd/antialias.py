"""Silhouette gradients: analytic edge antialiasing over the rasteriser's output (definition in include/gif_hip.h).

The rasteriser's gradient lives inside each pixel's winning face: the outline of the mesh cannot move under an
image loss, and the coverage mask has no gradient at all.  This post-pass finds the pixel pairs that straddle a silhouette edge
and blends them by the edge's sub-pixel position, a smooth function of the edge's two vertices — the blend carries the
gradient.  Opt-in: rasterize_attributes and render_condition are unchanged (GIF's condition is floor-quantised to 8 bits and is
the parity surface).
Kernels: gif_antialias_f32, gif_antialias_bwd_f32 (gfx950, deterministic, no float atomics) behind the C ABI; no CPU fallback.

max_hops > 0 lets a pair walk from the front pixel's face across non-silhouette edges to the face that owns the
outline edge, through gif_antialias_walk_f32 and gif_antialias_walk_bwd_f32: on a mesh whose faces next to the outline are
narrower than a pixel most of the outline blends only this way.  The default 0 takes the entry points above.
"""
import numpy as np
import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _lib, render
from . import standard_rasterize as sr


def _edge_adjacency_host(faces_cpu: np.ndarray) -> np.ndarray:
    """[F,3] int64 -> [F,3] int32: edge k of face f joins corners (k+1)%3 and (k+2)%3; the entry is the one OTHER face with the
    same undirected vertex pair, -1 if there is none or more than one (boundary and non-manifold edges are silhouette edges)."""
    F = faces_cpu.shape[0]
    adj = np.full((F, 3), -1, np.int32)
    if F == 0:
        return adj
    a = faces_cpu[:, [1, 2, 0]].reshape(-1)  # corner (k+1)%3 of entry f*3 + k
    b = faces_cpu[:, [2, 0, 1]].reshape(-1)
    key = np.minimum(a, b) * (int(faces_cpu.max()) + 1) + np.maximum(a, b)
    order = np.argsort(key, kind="stable")
    ks = key[order]
    start = np.flatnonzero(np.r_[True, ks[1:] != ks[:-1]])
    count = np.diff(np.r_[start, len(ks)])
    first = order[start[count == 2]]
    second = order[start[count == 2] + 1]
    two = first // 3 != second // 3  # (a face that names one vertex twice meets only itself)
    first, second = first[two], second[two]
    flat = adj.reshape(-1)
    flat[first] = second // 3
    flat[second] = first // 3
    return adj


def edge_adjacency(faces):
    """faces [F,3] or [B,F,3] (the topology of sample 0, shared by the batch) -> edge_adj [F,3] int32 on the faces' device.
    Built on the host once per topology and cached ON the faces tensor, validated by its in-place version counter (like
    render._topology)."""
    cached = getattr(faces, "_gif_edge_adj", None)
    if cached is None or cached[0] != (faces._version, str(faces.device)):
        f2 = faces[0] if faces.ndimension() == 3 else faces
        f_cpu = f2.detach().cpu().numpy().astype(np.int64)
        if f_cpu.size and f_cpu.min() < 0:
            raise _lib.GifHipError("negative face index")
        cached = ((faces._version, str(faces.device)), torch.from_numpy(_edge_adjacency_host(f_cpu)).to(faces.device))
        faces._gif_edge_adj = cached
    return cached[1]


MAX_HOPS = 64


def _check_hops(max_hops, what):
    if isinstance(max_hops, bool) or not isinstance(max_hops, (int, np.integer)) or not 0 <= max_hops <= MAX_HOPS:
        raise _lib.GifHipError(f"{what}: max_hops must be an integer in 0 .. {MAX_HOPS}, got {max_hops!r}")
    return int(max_hops)


def _one_topology(faces, B, what):
    if faces.ndimension() == 3 and B > 1 and faces.stride(0) != 0 and not torch.equal(faces, faces[:1].expand_as(faces)):
        raise _lib.GifHipError(f"{what} needs one face topology for the whole batch")


class _AntialiasFn(Function):
    @staticmethod
    def forward(ctx, image, vertices_ndc, tri, depth, faces, max_hops):
        B, C, h, w = image.shape
        _one_topology(faces, B, "antialias")
        faces_b = faces[None].expand(B, -1, -1) if faces.ndimension() == 2 else faces
        fv = sr.face_vertices(sr.to_image_space(vertices_ndc.float(), h, w), faces_b)
        F = fv.shape[1]
        adj = edge_adjacency(faces)
        img = image.float().contiguous()
        tri, depth = tri.contiguous(), depth.float().contiguous()
        out = torch.empty_like(img)
        with torch.cuda.device(img.device):  # launch on the operands' device and its current stream
            args = (img.data_ptr(), tri.data_ptr(), depth.data_ptr(), fv.data_ptr(), adj.data_ptr(), out.data_ptr(), B, C, F, h, w)
            stream = torch.cuda.current_stream().cuda_stream
            if max_hops == 0:
                _lib.check(_lib.load().gif_antialias_f32(*args, stream), "antialias")
            else:
                _lib.check(_lib.load().gif_antialias_walk_f32(*args, max_hops, stream), "antialias_walk")
        ctx.save_for_backward(img, tri, depth, fv, adj)
        ctx.faces, ctx.V, ctx.max_hops = faces, vertices_ndc.shape[1], max_hops
        ctx.dtypes = (image.dtype, vertices_ndc.dtype)
        return out.to(image.dtype)

    @staticmethod
    @once_differentiable  # raw kernel launch: a double backward must fail loudly, not return a history-free gradient
    def backward(ctx, gout):
        img, tri, depth, fv, adj = ctx.saved_tensors
        B, C, h, w = img.shape
        F = fv.shape[1]
        need_i, need_v = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_i or need_v):
            return None, None, None, None, None, None
        dev = img.device
        lib = _lib.load()
        g = gout.float().contiguous()
        gi = torch.empty_like(img) if need_i else None
        gfv = torch.empty_like(fv) if need_v else None
        ws = torch.empty((max(lib.gif_antialias_bwd_workspace_bytes(B, F, h, w) // 4, 1) if need_v else 1,), device=dev,
                         dtype=torch.float32)
        gv = None
        with torch.cuda.device(dev):
            args = (img.data_ptr(), tri.data_ptr(), depth.data_ptr(), fv.data_ptr(), adj.data_ptr(), g.data_ptr(),
                    gi.data_ptr() if need_i else None, gfv.data_ptr() if need_v else None, B, C, F, h, w)
            stream = torch.cuda.current_stream().cuda_stream
            if ctx.max_hops == 0:
                _lib.check(lib.gif_antialias_bwd_f32(*args, ws.data_ptr(), stream), "antialias_bwd")
            else:
                _lib.check(lib.gif_antialias_walk_bwd_f32(*args, ctx.max_hops, ws.data_ptr(), stream), "antialias_walk_bwd")
            if need_v:
                if F == 0:
                    gv = torch.zeros((B, ctx.V, 3), device=dev, dtype=ctx.dtypes[1])
                else:
                    _, off, ent = render._topology(ctx.faces, ctx.V, dev)
                    gv = render._face_gather_bwd(gfv, off, ent, ctx.V)
                    # to_image_space: x * w/2 + w/2, y * h/2 + h/2; z only orders the faces (no gradient)
                    gv *= torch.tensor([w / 2, h / 2, 0.0], device=dev, dtype=torch.float32)
                    gv = gv.to(ctx.dtypes[1])
        return (gi.to(ctx.dtypes[0]) if need_i else None), gv, None, None, None, None


def antialias(image, tri, depth, vertices_ndc, faces, max_hops=0):
    """image [B,C,h,w] (any C >= 1) with the rasteriser's tri [B,h,w] int32 and depth [B,h,w] for vertices_ndc [B,V,3] and faces
    [F,3] or [B,F,3] (one topology) -> [B,C,h,w]: pixel pairs that straddle a silhouette edge blended by the edge's sub-pixel
    position (definition: include/gif_hip.h).  Differentiable with respect to image and to x, y of
    vertices_ndc; not twice.  max_hops (0 .. 64) > 0: a pair whose front face does not own the outline edge walks on across up to
    that many non-silhouette edges to the face that does; 0 is §3o's definition and its kernels."""
    max_hops = _check_hops(max_hops, "antialias")
    for name, t in (("image", image), ("tri", tri), ("depth", depth), ("vertices_ndc", vertices_ndc), ("faces", faces)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise _lib.GifHipError(f"antialias needs device tensors (no CPU fallback): {name}")
    if image.ndimension() != 4 or image.shape[1] < 1 or tri.shape != (image.shape[0],) + image.shape[2:] or tri.shape != depth.shape:
        raise _lib.GifHipError("antialias: image [B,C,h,w] with C >= 1, tri and depth [B,h,w]")
    if tri.dtype != torch.int32:
        raise _lib.GifHipError(f"tri must be int32, got {tri.dtype}")
    if vertices_ndc.ndimension() != 3 or vertices_ndc.shape[0] != image.shape[0] or vertices_ndc.shape[2] != 3:
        raise _lib.GifHipError("antialias: vertices_ndc [B,V,3]")
    return _AntialiasFn.apply(image, vertices_ndc, tri, depth, faces, max_hops)


class _RasterizeBuffersFn(Function):
    """render._RasterizeAttributesFn's launches and backward, handing the face-index and depth buffers back as well."""

    @staticmethod
    def forward(ctx, vertices_ndc, attributes, faces, h, w):
        fv, fc, tri, img, mask, depth = render._rasterize_colors(
            vertices_ndc, faces, lambda faces_b: sr.face_vertices(attributes.float().contiguous(), faces_b), h, w, with_depth=True)
        ctx.mark_non_differentiable(mask, tri, depth)
        ctx.save_for_backward(fv, fc, tri)
        ctx.faces, ctx.hw = faces, (h, w)
        ctx.dtypes = (vertices_ndc.dtype, attributes.dtype)
        ctx.V = (vertices_ndc.shape[1], attributes.shape[1])
        return img, mask, tri, depth

    @staticmethod
    @once_differentiable
    def backward(ctx, gimg, _gmask, _gtri, _gdepth):
        fv, fc, tri = ctx.saved_tensors
        faces, (h, w) = ctx.faces, ctx.hw
        need_v, need_a = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        gv, gfc = render._rasterize_colors_bwd(fv, fc, tri, gimg, faces, ctx.V[0], ctx.dtypes[0], h, w, need_v, need_a,
                                               "rasterize_attributes_aa")
        ga = None
        if need_a:
            with torch.cuda.device(fv.device):
                _, off, ent = render._topology(faces, ctx.V[1], fv.device)
                ga = render._face_gather_bwd(gfc, off, ent, ctx.V[1]).to(ctx.dtypes[1])
        return gv, ga, None, None, None


def rasterize_attributes_aa(vertices_ndc, faces, attributes, h, w, max_hops=0):
    """render.rasterize_attributes with an antialiased outline: (image_aa [B,3,h,w], coverage_aa [B,1,h,w]).  The rasteriser's
    launches, then `antialias` over the three attribute channels and the 0 / 1 mask as a fourth.  Both outputs are differentiable:
    inside the faces as rasterize_attributes is, and at silhouette edges through the blend — a loss on coverage_aa alone reaches
    the vertices.  max_hops: as in `antialias`."""
    max_hops = _check_hops(max_hops, "rasterize_attributes_aa")
    if not vertices_ndc.is_cuda:
        raise _lib.GifHipError("rasterize_attributes_aa needs device tensors (no CPU fallback)")
    img, mask, tri, depth = _RasterizeBuffersFn.apply(vertices_ndc, attributes, faces, h, w)
    out = antialias(torch.cat((img, mask.to(img.dtype)), dim=1), tri, depth, vertices_ndc, faces, max_hops)
    return out[:, :3], out[:, 3:]


def soft_silhouette(vertices_ndc, faces, h, w, max_hops=0):
    """coverage_aa [B,1,h,w] alone: one rasteriser pass for the face-index and depth buffers (no attribute gather), then `antialias`
    over the 0 / 1 mask.  Differentiable with respect to x, y of vertices_ndc.  max_hops: as in `antialias`."""
    max_hops = _check_hops(max_hops, "soft_silhouette")
    if not vertices_ndc.is_cuda:
        raise _lib.GifHipError("soft_silhouette needs device tensors (no CPU fallback)")
    B = vertices_ndc.shape[0]
    with torch.no_grad():
        faces_b = faces[None].expand(B, -1, -1) if faces.ndimension() == 2 else faces
        fv = sr.face_vertices(sr.to_image_space(vertices_ndc.float(), h, w), faces_b)
        depth, tri, bary = sr.new_buffers(B, h, w, vertices_ndc.device)
        sr.standard_rasterize(fv, depth, tri, bary, h, w)
        mask = (tri >= 0)[:, None].float()
    return antialias(mask, tri, depth, vertices_ndc, faces, max_hops)
