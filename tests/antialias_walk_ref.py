"""Torch restatement of the walking edge antialiasing, gif_amd.antialias with max_hops (definition: include/gif_hip.h, DESIGN.md
§3p): tests/antialias_ref.py's definition with one parameter more.  A pair whose front face owns no silhouette edge that crosses
the segment A -> B leaves that face through the crossing edge nearest to A and asks the neighbour, up to max_hops times.

Dtype-generic like antialias_ref: float64 is the yardstick, a float32 run sizes the tolerances.  Every discrete choice (pairs,
front pixel, classification, candidates, the route of the walk, receiver) is made on detached values and frozen; autograd sees
the crossing position a of the hit edge and the blended values only.  With max_hops = 0 every operation is antialias_ref's, in
its order: the output and the counts are the same bits.

MARGINAL pairs: some edge TESTED along the walk has t or a within MARGIN of 0 or 1 while neither lies further than MARGIN outside
[0, 1] (the candidate test could go either way), or the hit's a lies within MARGIN of 0.5.  Tested are the silhouette edges of
every face the walk visits and, in a face the walk may still leave (hop < max_hops), its other edges too — at hop = max_hops a
non-silhouette edge decides nothing.  The edge a walk came in through is not tested.
The second half adds the lat x long sphere, the strip and grid meshes and the cases of tests/test_antialias_walk_cpu.py and
tests/test_gpu_antialias_walk.py.
"""
import numpy as np
import torch

import antialias_ref as aref
from antialias_ref import MARGIN, _front_facing


def antialias_walk_ref(image, tri, depth, face_vertices, edge_adj, max_hops):
    """antialias_ref's arguments and max_hops >= 0.  Returns (out [B,C,H,W], stats): antialias_ref's keys "pairs", "blended",
    "marginal", "marginal_pixels", and
      "hits_per_hop"      [max_hops + 1] ints: blended pairs by the hop their hit edge was found at
      "marginal_blended"  the marginal pairs among the blended ones
      "hits"              [n,8] int64, one row per blended pair in the order they are added: axis, b, py, px (the pair's first
                          pixel), face and edge k of the hit, hop, 1 if exactly one pixel of the pair is covered (an OUTLINE pair)
      "hit_a"             [n] the crossing positions a of those rows (detached)
      "outline_pairs"     the number of outline pairs."""
    B, C, H, W = image.shape
    dt = image.dtype
    tri = tri.long()
    depth = depth.to(dt)
    edge_adj = torch.as_tensor(edge_adj).long()
    fv = face_vertices
    flat = image.permute(0, 2, 3, 1).reshape(B * H * W, C)
    out = flat
    stats = {"pairs": 0, "blended": 0, "marginal": 0, "marginal_pixels": torch.zeros((B, H, W), dtype=torch.bool),
             "hits_per_hop": [0] * (max_hops + 1), "marginal_blended": 0, "outline_pairs": 0}
    rows, hit_as = [], []
    near = lambda z: (z.abs() <= MARGIN) | ((z - 1).abs() <= MARGIN)
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
        t_b = tri[b, by, bx]
        u, v = axis, 1 - axis
        Au, Av = (ax if axis == 0 else ay).to(dt), (ay if axis == 0 else ax).to(dt)
        s = ((bx - ax) if axis == 0 else (by - ay)).to(dt)
        cur = tri[b, ay, ax]
        prev = torch.full_like(cur, -1)
        walking = torch.ones_like(a_is_p)
        hit = torch.zeros_like(a_is_p)
        marginal = torch.zeros_like(a_is_p)
        best = torch.zeros(b.shape, dtype=dt)
        hit_f, hit_k, hit_hop = torch.zeros_like(cur), torch.zeros_like(cur), torch.zeros_like(cur)
        for hop in range(max_hops + 1):
            face = fv[b, cur]  # [N,3,3]
            found = torch.zeros_like(a_is_p)  # a silhouette candidate in this face
            leaves = torch.zeros_like(a_is_p)  # any other candidate
            lbest = torch.zeros(b.shape, dtype=dt)
            lnext = torch.zeros_like(cur)
            for k in range(3):
                P, Q = face[:, (k + 1) % 3], face[:, (k + 2) % 3]
                den = Q[:, v] - P[:, v]
                n = edge_adj[cur, k]
                ok = walking & (den.detach() != 0)
                if hop > 0:
                    ok = ok & (n != prev)  # the edge the walk came in through
                t = (Av - P[:, v]) / torch.where(den.detach() != 0, den, torch.ones_like(den))
                a = (P[:, u] + t * (Q[:, u] - P[:, u]) - Au) * s
                sil = (n < 0) | ~_front_facing(fv[b, n.clamp_min(0)].detach())
                td, ad = t.detach(), a.detach()
                inside = ok & (td >= 0) & (td <= 1) & (ad >= 0) & (ad <= 1)
                within = (td >= -MARGIN) & (td <= 1 + MARGIN) & (ad >= -MARGIN) & (ad <= 1 + MARGIN)
                tested = ok & (sil if hop == max_hops else torch.ones_like(sil))
                marginal |= tested & within & (near(td) | near(ad))
                cand = inside & sil
                better = cand & (~found | (ad < best.detach()))  # strict: the lowest k keeps a tie
                best = torch.where(better, a, best)
                hit_k = torch.where(better, torch.full_like(hit_k, k), hit_k)
                found |= cand
                other = inside & ~sil
                lbetter = other & (~leaves | (ad < lbest))
                lbest = torch.where(lbetter, ad, lbest)
                lnext = torch.where(lbetter, n, lnext)
                leaves |= other
            hit_f = torch.where(found, cur, hit_f)
            hit_hop = torch.where(found, torch.full_like(hit_hop, hop), hit_hop)
            hit |= found
            walking = walking & ~found & leaves & (lnext != t_b)
            if hop == max_hops or not walking.any():
                break
            prev = torch.where(walking, cur, prev)
            cur = torch.where(walking, lnext, cur)
        marginal |= hit & ((best.detach() - 0.5).abs() <= MARGIN)
        outline = (tpp < 0) != (tqq < 0)
        stats["pairs"] += int(b.numel())
        stats["blended"] += int(hit.sum())
        stats["marginal"] += int(marginal.sum())
        stats["marginal_blended"] += int((marginal & hit).sum())
        stats["outline_pairs"] += int(outline.sum())
        for hop in range(max_hops + 1):
            stats["hits_per_hop"][hop] += int((hit & (hit_hop == hop)).sum())
        mp = stats["marginal_pixels"]
        mp[b[marginal], py[marginal], px[marginal]] = True
        mp[b[marginal], qy[marginal], qx[marginal]] = True
        rows.append(torch.stack([torch.full_like(b, axis), b, py, px, hit_f, hit_k, hit_hop, outline.long()], 1)[hit])
        hit_as.append(best.detach()[hit])
        recv_a = best.detach() < 0.5
        wgt = torch.where(recv_a, 0.5 - best, best - 0.5)
        ia, ib = (b * H + ay) * W + ax, (b * H + by) * W + bx
        r, d = torch.where(recv_a, ia, ib)[hit], torch.where(recv_a, ib, ia)[hit]
        out = out.index_add(0, r, wgt[hit][:, None] * (flat[d] - flat[r]))  # reads from the input image only
    stats["hits"] = torch.cat(rows) if rows else torch.zeros((0, 8), dtype=torch.long)
    stats["hit_a"] = torch.cat(hit_as) if hit_as else torch.zeros((0,), dtype=dt)
    return out.reshape(B, H, W, C).permute(0, 3, 1, 2), stats


# ------------------------------------------------------------------------------------------ meshes and cases
def sphere(nlat, nlon):
    """nlat x nlon lat-long sphere, antialias_ref.small_sphere generalised: V = (nlat - 1) nlon + 2, F = 2 nlon (nlat - 1)."""
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
    return verts, np.array(faces, np.int64)


def posed(verts, a=0.37, c=0.23, scale=0.55, shift=(0.21, -0.12)):
    """One image [1,V,3] float32 of `verts` posed like antialias_ref.sphere_case's image 0."""
    Ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    Rx = np.array([[1, 0, 0], [0, np.cos(c), -np.sin(c)], [0, np.sin(c), np.cos(c)]])
    return (verts @ (Rx @ Ry).T * scale + np.array([shift[0], shift[1], 0.0]))[None].astype(np.float32)


def grid_mesh(xs, ys, h, w, transpose=False):
    """Pixel-space vertices xs[j][i], ys[j][i] (row j, column i) -> pixel_mesh of the cells, each split (a,b,d), (a,d,c) with
    a, b the cell's upper and c, d its lower corners.  transpose: x and y swapped (the image is then w x h as given)."""
    nr, nc = len(xs), len(xs[0])
    pts = [((ys[j][i], xs[j][i]) if transpose else (xs[j][i], ys[j][i])) for j in range(nr) for i in range(nc)]
    faces = []
    for j in range(nr - 1):
        for i in range(nc - 1):
            a, b, c, d = j * nc + i, j * nc + i + 1, (j + 1) * nc + i, (j + 1) * nc + i + 1
            faces += [(a, b, d), (a, d, c)]
    return aref.pixel_mesh(pts, faces, h, w)


STRIP_COLS, STRIP_ROWS, STRIP_SKEW = (1.4, 4.6, 5.1), (-2.5, 3.3, 7.7, 13.5), 0.03


def strip_edge(E, j, skew=STRIP_SKEW):
    """x of the strip mesh's outer edge on vertex row j."""
    return E + skew * j


def strip_mesh(E, transpose=False, skew=STRIP_SKEW):
    """12 x 12: three columns of cells, the last two narrower than a pixel, behind the outline at x = E (+ skew per vertex row):
    the outermost covered pixel of a row lies in a face that does not own the outline edge beside it."""
    cols = STRIP_COLS + (E,)
    xs = [[x + skew * j for x in cols] for j in range(len(STRIP_ROWS))]
    ys = [[y] * len(cols) for y in STRIP_ROWS]
    return grid_mesh(xs, ys, 12, 12, transpose)


def border_grid(h, w, n=9):
    """antialias_ref.border_case's quad as an n x n bilinear grid of cells (F = 2 n n): the outline runs along rows 0 and h-1 and
    columns 0 and w-1, through faces narrower than a pixel or not owning it."""
    c = np.array([(0.3, 0.4), (w - 1.35, 0.25), (w - 1.3, h - 1.45), (0.45, h - 1.3)])  # corners 0 1 / 3 2
    xs, ys = [], []
    for j in range(n + 1):
        left, right = c[0] + (c[3] - c[0]) * j / n, c[1] + (c[2] - c[1]) * j / n
        row = [left + (right - left) * i / n for i in range(n + 1)]
        xs.append([p[0] for p in row])
        ys.append([p[1] for p in row])
    return grid_mesh(xs, ys, h, w)


def quarter_rectangle():
    """The rectangle of test_half_pixel_edges_return_the_rasterisers_bits a quarter pixel to the right, at 16 x 16: edges at
    x = 3.75 and 9.75 (exact in float32)."""
    v, f = aref.pixel_mesh([(3.5, 2.5), (9.5, 2.5), (9.5, 7.5), (3.5, 7.5)], [(0, 1, 2), (0, 2, 3)], 16, 16)
    v = v.copy()
    v[..., 0] += 0.25 * 2 / 16
    return v, f


def _sphere_case(nlat, nlon, h, w, C, hops):
    verts, f = sphere(nlat, nlon)
    return posed(verts), f, h, w, C, hops


# name -> (vertices_ndc [B,V,3] float32, faces [F,3], h, w, C, max_hops)
WALK_CASES = {
    "sphere_70x90_b3": lambda: aref.sphere_case(3) + (70, 90, 3, 4),
    "sphere_64x64_b1": lambda: aref.CASES["sphere_64x64_b1"]() + (4,),
    "sphere24x30_70x90": lambda: _sphere_case(24, 30, 70, 90, 3, 16),
    "sphere40x48_70x90": lambda: _sphere_case(40, 48, 70, 90, 4, 8),  # the cap cuts walks short
    "edges_70x70_b2": lambda: aref.edge_mesh(2, 70) + (70, 70, 4, 4),
    "strip_12x12": lambda: strip_mesh(5.3) + (12, 12, 7, 4),
    "strip_12x12_t": lambda: strip_mesh(5.3, transpose=True) + (12, 12, 7, 4),
    "border_grid_11x13": lambda: border_grid(11, 13) + (11, 13, 3, 2),
}
