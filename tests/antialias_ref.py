"""Torch restatement of the analytic edge antialiasing of gif_amd.antialias (definition: include/gif_hip.h).

Dtype-generic: float64 is the yardstick, a float32 run of the same code sizes the tolerances.  `tri` and `depth` are taken as
given; every discrete choice (pairs, front pixel, silhouette classification, candidate, receiver) is made on detached values
and frozen, so autograd differentiates through the crossing position a and the blended values only — the gradients the
definition names.  Each call reports the number of pairs, of blended pairs, and of MARGINAL pairs: pairs for which some
silhouette edge of the front face has t or a within MARGIN of 0 or 1 while neither lies further than MARGIN outside [0, 1] (the
candidate test could go either way), or whose chosen a lies within MARGIN of 0.5 (the receiver could).  `marginal_pixels` marks
both pixels of those pairs.
The second half holds the meshes and CASES that tests/test_antialias_cpu.py and tests/test_gpu_antialias.py share.
"""
import numpy as np
import torch

MARGIN = 1e-4


def edge_adjacency_ref(faces):
    """[F,3] ints -> [F,3] int64 by the definition, face by face (a dictionary; independent of the library's sort)."""
    faces = np.asarray(faces).astype(np.int64)
    users = {}
    for f, tri in enumerate(faces):
        for k in range(3):
            a, b = int(tri[(k + 1) % 3]), int(tri[(k + 2) % 3])
            users.setdefault((min(a, b), max(a, b)), []).append((f, k))
    adj = np.full(faces.shape, -1, np.int64)
    for ent in users.values():
        if len(ent) == 2 and ent[0][0] != ent[1][0]:
            (f0, k0), (f1, k1) = ent
            adj[f0, k0], adj[f1, k1] = f1, f0
    return adj


def _front_facing(fv):
    """The rasteriser's front-face test on [...,3,3] face vertices."""
    x, y = fv[..., 0], fv[..., 1]
    return (y[..., 2] - y[..., 0]) * (x[..., 1] - x[..., 0]) < (y[..., 1] - y[..., 0]) * (x[..., 2] - x[..., 0])


def antialias_ref(image, tri, depth, face_vertices, edge_adj):
    """image [B,C,H,W], face_vertices [B,F,3,3] (pixel units) in one floating dtype; tri [B,H,W] integer, depth [B,H,W],
    edge_adj [F,3] integer.  Returns (out [B,C,H,W], stats) with stats = {"pairs", "blended", "marginal", "marginal_pixels"
    ([B,H,W] bool)}."""
    B, C, H, W = image.shape
    dt = image.dtype
    tri = tri.long()
    depth = depth.to(dt)
    edge_adj = torch.as_tensor(edge_adj).long()
    fv = face_vertices
    flat = image.permute(0, 2, 3, 1).reshape(B * H * W, C)
    out = flat
    stats = {"pairs": 0, "blended": 0, "marginal": 0, "marginal_pixels": torch.zeros((B, H, W), dtype=torch.bool)}
    for axis in (0, 1):  # 0: p and its right neighbour; 1: p and its lower neighbour
        if (W if axis == 0 else H) < 2:
            continue
        tp = tri[:, :, :-1] if axis == 0 else tri[:, :-1]
        tq = tri[:, :, 1:] if axis == 0 else tri[:, 1:]
        b, py, px = torch.nonzero(tp != tq, as_tuple=True)
        if b.numel() == 0:
            continue
        qy, qx = (py, px + 1) if axis == 0 else (py + 1, px)
        tpp, tqq = tri[b, py, px], tri[b, qy, qx]
        a_is_p = (tqq < 0) | ((tpp >= 0) & (depth[b, py, px] <= depth[b, qy, qx]))
        ay, ax = torch.where(a_is_p, py, qy), torch.where(a_is_p, px, qx)
        by, bx = torch.where(a_is_p, qy, py), torch.where(a_is_p, qx, px)
        f = tri[b, ay, ax]
        face = fv[b, f]  # [N,3,3]
        u, v = axis, 1 - axis
        Au, Av = (ax if axis == 0 else ay).to(dt), (ay if axis == 0 else ax).to(dt)
        s = ((bx - ax) if axis == 0 else (by - ay)).to(dt)
        hit = torch.zeros_like(a_is_p)
        marginal = torch.zeros_like(a_is_p)
        best = torch.zeros(b.shape, dtype=dt)
        for k in range(3):
            P, Q = face[:, (k + 1) % 3], face[:, (k + 2) % 3]
            den = Q[:, v] - P[:, v]
            ok = den.detach() != 0
            t = (Av - P[:, v]) / torch.where(ok, den, torch.ones_like(den))
            a = (P[:, u] + t * (Q[:, u] - P[:, u]) - Au) * s
            n = edge_adj[f, k]
            sil = (n < 0) | ~_front_facing(fv[b, n.clamp_min(0)].detach())
            td, ad = t.detach(), a.detach()
            cand = ok & sil & (td >= 0) & (td <= 1) & (ad >= 0) & (ad <= 1)
            near = lambda z: (z.abs() <= MARGIN) | ((z - 1).abs() <= MARGIN)
            within = (td >= -MARGIN) & (td <= 1 + MARGIN) & (ad >= -MARGIN) & (ad <= 1 + MARGIN)
            marginal |= ok & sil & within & (near(td) | near(ad))
            better = cand & (~hit | (ad < best.detach()))  # strict: the lowest k keeps a tie
            best = torch.where(better, a, best)
            hit |= cand
        marginal |= hit & ((best.detach() - 0.5).abs() <= MARGIN)
        stats["pairs"] += int(b.numel())
        stats["blended"] += int(hit.sum())
        stats["marginal"] += int(marginal.sum())
        mp = stats["marginal_pixels"]
        mp[b[marginal], py[marginal], px[marginal]] = True
        mp[b[marginal], qy[marginal], qx[marginal]] = True
        recv_a = best.detach() < 0.5
        wgt = torch.where(recv_a, 0.5 - best, best - 0.5)
        ia, ib = (b * H + ay) * W + ax, (b * H + by) * W + bx
        r, d = torch.where(recv_a, ia, ib)[hit], torch.where(recv_a, ib, ia)[hit]
        out = out.index_add(0, r, wgt[hit][:, None] * (flat[d] - flat[r]))  # reads from the input image only
    return out.reshape(B, H, W, C).permute(0, 3, 1, 2), stats


def face_vertices_ref(v_ndc, vi32, faces, h, w, base=None):
    """[B,F,3,3] pixel-space face vertices in v_ndc's dtype that carry exactly the float32 values `vi32` [B,V,3] the kernels see
    (standard_rasterize.to_image_space), with the exact NDC -> pixel derivative for x and y and none for z.  `base`: the NDC
    vertices vi32 belongs to, where v_ndc is a perturbation of them (finite differences); default v_ndc itself."""
    to_px = lambda v: torch.stack([v[..., 0] * w / 2 + w / 2, v[..., 1] * h / 2 + h / 2, torch.zeros_like(v[..., 2])], -1)
    p = to_px(v_ndc)
    pix = torch.as_tensor(vi32).to(v_ndc.dtype) + (p - (p.detach() if base is None else to_px(base.detach())))
    return pix[:, torch.as_tensor(faces).long()]


# ------------------------------------------------------------------------------------------ cases of the CPU and GPU tests
def small_sphere():
    """10 x 12 lat-long sphere: V = 110, F = 216, unit radius, z flipped as in test_gpu_render_grad.sphere_mesh."""
    nlat, nlon = 10, 12
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
    verts[:, 2] *= -1  # +z away from the camera: the near half winds front-facing
    assert verts.shape == (110, 3) and len(faces) == 216
    return verts, np.array(faces, np.int64)


def sphere_case(B):
    """B rotated, scaled and shifted copies of the small sphere (NDC)."""
    v, f = small_sphere()
    vs = []
    for i in range(B):
        a, c = 0.37 + 0.45 * i, 0.23 - 0.31 * i
        Ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        Rx = np.array([[1, 0, 0], [0, np.cos(c), -np.sin(c)], [0, np.sin(c), np.cos(c)]])
        vs.append(v @ (Rx @ Ry).T * (0.55 + 0.13 * i) + np.array([0.21 - 0.17 * i, -0.12 + 0.11 * i, 0.0]))
    return np.stack(vs).astype(np.float32), f


def edge_mesh(B, h):
    """test_gpu_render_grad.edge_mesh: two screen-filling faces behind a few medium ones (faces behind faces, boundary edges), a
    face that covers no pixel centre, a degenerate (zero-area) face and an unused vertex."""
    rng = np.random.RandomState(2)
    px = 2.0 / h  # one pixel in NDC
    v = [(-1.6, -1.55, 0.9), (1.63, -1.6, 0.9), (1.57, 1.6, 0.9), (-1.6, 1.62, 0.9)]
    f = [(0, 2, 1), (0, 3, 2)]
    for _ in range(6):  # medium triangles in front
        c = rng.uniform(-0.6, 0.6, 2)
        k = len(v)
        for a in (0.0, 2.1, 4.2):
            r = rng.uniform(0.15, 0.35)
            v.append((c[0] + r * np.cos(a), c[1] + r * np.sin(a), rng.uniform(0.0, 0.5)))
        f.append((k, k + 2, k + 1))
    x0, y0 = -1 + px * 10.2, -1 + px * 20.2  # no pixel centre: a tiny triangle strictly between pixel centres
    k = len(v)
    v += [(x0, y0, 0.1), (x0 + px * 0.5, y0, 0.1), (x0, y0 + px * 0.5, 0.1)]
    f.append((k, k + 1, k + 2))
    f.append((k, k + 2, k + 1))  # (either winding)
    k = len(v)
    v += [(0.1, 0.1, 0.0), (0.4, 0.2, 0.0)]  # degenerate: a repeated vertex
    f.append((k, k, k + 1))
    v.append((0.0, 0.0, 0.0))  # unused
    f = np.array(f, np.int64)
    v = np.array(v, np.float64)
    vs = np.stack([v + np.array([3 * px * i, -2 * px * i, 0.0]) for i in range(B)])
    return vs.astype(np.float32), f


def pixel_mesh(corners_px, faces, h, w):
    """One image of a mesh given in PIXEL coordinates [(x, y)], at depth 0.5 -> NDC vertices [1,V,3]; faces are rewound where
    needed so that each passes the rasteriser's front-face test."""
    p = np.array(corners_px, np.float64)
    out = []
    for a, b, c in faces:
        front = (p[c, 1] - p[a, 1]) * (p[b, 0] - p[a, 0]) < (p[b, 1] - p[a, 1]) * (p[c, 0] - p[a, 0])
        out.append((a, b, c) if front else (a, c, b))
    v = np.stack([(p[:, 0] - w / 2) / (w / 2), (p[:, 1] - h / 2) / (h / 2), np.full(len(p), 0.5)], -1)
    return v[None].astype(np.float32), np.array(out, np.int64)


def border_case(h, w):
    """A quad whose four (slightly skewed) silhouette edges run between row 0 and row 1, row h-2 and row h-1, column 0 and
    column 1, column w-2 and column w-1: every pair on them has a pixel on the image border."""
    return pixel_mesh([(0.3, 0.4), (w - 1.35, 0.25), (w - 1.3, h - 1.45), (0.45, h - 1.3)], [(0, 1, 2), (0, 2, 3)], h, w)


# name -> (vertices_ndc [B,V,3] float32, faces [F,3], h, w, C)
CASES = {
    "sphere_70x90_b3": lambda: sphere_case(3) + (70, 90, 3),
    "sphere_64x64_b1": lambda: (sphere_case(2)[0][1:], sphere_case(2)[1], 64, 64, 1),
    "edges_70x70_b2": lambda: edge_mesh(2, 70) + (70, 70, 4),
    "triangle_1x9": lambda: pixel_mesh([(2.3, -3.0), (6.6, -2.0), (4.0, 5.0)], [(0, 1, 2)], 1, 9) + (1, 9, 7),
    "triangle_9x1": lambda: pixel_mesh([(-3.0, 2.3), (-2.0, 6.6), (5.0, 4.0)], [(0, 1, 2)], 9, 1) + (9, 1, 7),
    "border_11x13": lambda: border_case(11, 13) + (11, 13, 3),
}
