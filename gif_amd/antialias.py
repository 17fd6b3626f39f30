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
    Built on the host once per topology and cached ON the faces tensor, validated like render._topology: by the in-place version
    counter AND the address and geometry of the data (`faces.data = other` keeps the counter).  A write through `.data` into the same
    storage bumps no counter and moves no address: that one is the caller's to announce, with `del faces._gif_edge_adj`."""
    key = (faces._version, faces.data_ptr(), tuple(faces.shape), tuple(faces.stride()), str(faces.device))
    cached = getattr(faces, "_gif_edge_adj", None)
    if cached is None or cached[0] != key:
        f2 = faces[0] if faces.ndimension() == 3 else faces
        f_cpu = f2.detach().cpu().numpy().astype(np.int64)
        if f_cpu.size and f_cpu.min() < 0:
            raise _lib.GifHipError("negative face index")
        cached = (key, torch.from_numpy(_edge_adjacency_host(f_cpu)).to(faces.device))
        faces._gif_edge_adj = cached
    return cached[1]


MAX_HOPS = 64


def _check_hops(max_hops, what):
    if isinstance(max_hops, bool) or not isinstance(max_hops, (int, np.integer)) or not 0 <= max_hops <= MAX_HOPS:
        raise _lib.GifHipError(f"{what}: max_hops must be an integer in 0 .. {MAX_HOPS}, got {max_hops!r}")
    return int(max_hops)


class _AntialiasFn(Function):
    @staticmethod
    def forward(ctx, image, vertices_ndc, tri, depth, faces, max_hops):
        B, C, h, w = image.shape
        render._one_topology(faces, B, "antialias")
        fv = render._projected_face_vertices(vertices_ndc, faces, h, w)
        adj = edge_adjacency(faces)
        img = image.float().contiguous()
        tri, depth = tri.contiguous(), depth.float().contiguous()
        out = torch.empty_like(img)
        walk = ("gif_antialias_walk_f32", max_hops) if max_hops else ("gif_antialias_f32",)
        if C:  # (no channel: nothing to blend, and the entry points take C >= 1)
            _lib.launch(walk[0], img.device, img, tri, depth, fv, adj, out, B, C, fv.shape[1], h, w, *walk[1:])
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
        need_i, need_v = ctx.needs_input_grad[:2]
        if not (need_i or need_v):
            return None, None, None, None, None, None
        gi = torch.empty_like(img) if need_i else None
        if C == 0:  # no channel carries a gradient to a vertex
            gv = torch.zeros((B, ctx.V, 3), device=img.device, dtype=ctx.dtypes[1]) if need_v else None
            return (gi.to(ctx.dtypes[0]) if need_i else None), gv, None, None, None, None
        gfv = torch.empty_like(fv) if need_v else None
        # (the workspace serves the vertex gradient alone: one element without it)
        ws = _lib.workspace(_lib.load().gif_antialias_bwd_workspace_bytes(B, F, h, w) if need_v else 0, img.device)
        walk = ("gif_antialias_walk_bwd_f32", ctx.max_hops) if ctx.max_hops else ("gif_antialias_bwd_f32",)
        _lib.launch(walk[0], img.device, img, tri, depth, fv, adj, gout.float().contiguous(), gi, gfv, B, C, F, h, w, *walk[1:], ws)
        gv = render._ndc_vertex_grad(gfv, ctx.faces, ctx.V, h, w, ctx.dtypes[1]) if need_v else None
        return (gi.to(ctx.dtypes[0]) if need_i else None), gv, None, None, None, None


def antialias(image, tri, depth, vertices_ndc, faces, max_hops=0):
    """image [B,C,h,w] (any C; C = 0 gives the empty image back) with the rasteriser's tri [B,h,w] int32 and depth [B,h,w] for
    vertices_ndc [B,V,3] and faces [F,3] or [B,F,3] (one topology) -> [B,C,h,w]: pixel pairs that straddle a silhouette edge
    blended by the edge's sub-pixel position (definition: include/gif_hip.h).  Differentiable with respect to image
    and to x, y of vertices_ndc; not twice.  max_hops (0 .. 64) > 0: a pair whose front face does not own the outline edge walks on
    across up to that many non-silhouette edges to the face that does; 0 is §3o's definition and its kernels."""
    max_hops = _check_hops(max_hops, "antialias")
    _lib.require_device("antialias", image=image, tri=tri, depth=depth, vertices_ndc=vertices_ndc, faces=faces)
    if image.ndimension() != 4 or tri.shape != (image.shape[0],) + image.shape[2:] or tri.shape != depth.shape:
        raise _lib.GifHipError("antialias: image [B,C,h,w], tri and depth [B,h,w]")
    if tri.dtype != torch.int32:
        raise _lib.GifHipError(f"tri must be int32, got {tri.dtype}")
    if vertices_ndc.ndimension() != 3 or vertices_ndc.shape[0] != image.shape[0] or vertices_ndc.shape[2] != 3:
        raise _lib.GifHipError("antialias: vertices_ndc [B,V,3]")
    return _AntialiasFn.apply(image, vertices_ndc, tri, depth, faces, max_hops)


def rasterize_attributes_aa(vertices_ndc, faces, attributes, h, w, max_hops=0):
    """render.rasterize_attributes with an antialiased outline: (image_aa [B,3,h,w], coverage_aa [B,1,h,w]).  The rasteriser's
    launches, then `antialias` over the three attribute channels and the 0 / 1 mask as a fourth.  Both outputs are differentiable:
    inside the faces as rasterize_attributes is, and at silhouette edges through the blend — a loss on coverage_aa alone reaches
    the vertices.  max_hops: as in `antialias`."""
    max_hops = _check_hops(max_hops, "rasterize_attributes_aa")
    _lib.require_device("rasterize_attributes_aa", vertices_ndc=vertices_ndc)
    img, mask, tri, depth = render._RasterizeColorsFn.apply(vertices_ndc, attributes, faces, h, w, True, "rasterize_attributes_aa")
    out = antialias(torch.cat((img, mask.to(img.dtype)), dim=1), tri, depth, vertices_ndc, faces, max_hops)
    return out[:, :3], out[:, 3:]


def soft_silhouette(vertices_ndc, faces, h, w, max_hops=0):
    """coverage_aa [B,1,h,w] alone: one rasteriser pass for the face-index and depth buffers (no attribute gather), then `antialias`
    over the 0 / 1 mask.  Differentiable with respect to x, y of vertices_ndc.  max_hops: as in `antialias`."""
    max_hops = _check_hops(max_hops, "soft_silhouette")
    _lib.require_device("soft_silhouette", vertices_ndc=vertices_ndc)
    B = vertices_ndc.shape[0]
    with torch.no_grad():
        fv = render._projected_face_vertices(vertices_ndc, faces, h, w)
        depth, tri, bary = sr.new_buffers(B, h, w, vertices_ndc.device)
        sr.standard_rasterize(fv, depth, tri, bary, h, w)
        mask = (tri >= 0)[:, None].float()
    return antialias(mask, tri, depth, vertices_ndc, faces, max_hops)

