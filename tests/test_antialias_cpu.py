"""CPU-side checks of the analytic edge antialiasing: the float64 restatement tests/antialias_ref.py against hand
-computed edge positions and against central differences, the edge adjacency of gif_amd.antialias on closed, open and
non-manifold meshes, the entry points' argument validation (before any launch), and the share of marginal pairs in every case
of tests/test_gpu_antialias.py — all on the oracle rasteriser's tri and depth buffers."""
import numpy as np
import pytest
import torch

import antialias_ref as aref
from gif_amd import _lib
from gif_amd import antialias as AA
from oracle import rasterize_oracle as ro

MAX_MARGINAL = 0.01  # of the blended pairs


def oracle_buffers(v, f, h, w):
    """(vi [B,V,3] float32 pixel-space vertices, tri, depth) of the oracle rasteriser for NDC vertices v [B,V,3]."""
    B = v.shape[0]
    vi = ro.to_image_space(v, h, w)
    fv = ro.face_vertices(vi, np.repeat(f[None], B, 0).astype(np.int32))
    d, t, b = ro.new_buffers(B, h, w)
    ro.standard_rasterize(fv, d, t, b, h, w)
    return vi, t, d


def run_ref(v, f, h, w, image=None, dtype=torch.float64):
    vi, t, d = oracle_buffers(v, f, h, w)
    tri = torch.from_numpy(t)
    if image is None:
        image = (tri >= 0)[:, None].to(dtype)  # coverage as the image
    fv = aref.face_vertices_ref(torch.from_numpy(v).to(dtype), vi, f, h, w)
    out, stats = aref.antialias_ref(image.to(dtype), tri, torch.from_numpy(d), fv, aref.edge_adjacency_ref(f))
    return out, stats, tri


@pytest.mark.parametrize("axis", [0, 1])
@pytest.mark.parametrize("edge,inner,outer", [(5.3, 0.8, 0.0), (5.7, 1.0, 0.2)])
def test_analytic_edge(axis, edge, inner, outer):
    """One large triangle with a straight edge at coordinate `edge` over a zero background, coverage as the image: the pixel
    inside the edge (5) and the pixel outside it (6) take the covered share of their pixel, 5.5 - edge and edge - 5.5."""
    h, w = (9, 12) if axis == 0 else (12, 9)
    px = [(edge, -20.0), (edge, 30.0), (-30.0, 4.0)]
    if axis == 1:
        px = [(y, x) for x, y in px]
    v, f = aref.pixel_mesh(px, [(0, 1, 2)], h, w)
    out, stats, tri = run_ref(v, f, h, w)
    line = out[0, 0] if axis == 0 else out[0, 0].T  # [9 lines, 12 pixels across the edge]
    assert tuple(line.shape) == (9, 12) and stats["blended"] == 9 and stats["pairs"] == 9 and stats["marginal"] == 0
    assert (line[:, :5] == 1).all() and (line[:, 7:] == 0).all()
    assert (line[:, 5] - inner).abs().max() <= 1e-6 and (line[:, 6] - outer).abs().max() <= 1e-6, line[:, 4:8]


def test_shared_edge_of_coplanar_triangles_blends_nothing():
    h, w = 10, 12
    v, f = aref.pixel_mesh([(2.4, 1.6), (9.3, 2.2), (8.7, 7.5), (1.8, 6.9)], [(0, 1, 2), (0, 2, 3)], h, w)
    _, tri0, _ = oracle_buffers(v, f, h, w)
    image = torch.from_numpy(tri0 + 2.0)[:, None]  # a different value on either side of the shared edge
    out, stats, tri = run_ref(v, f, h, w, image)
    assert set(np.unique(tri0)) == {-1, 0, 1}
    cov = (tri >= 0)
    pad = torch.nn.functional.pad(cov, (1, 1, 1, 1), value=True)
    inner = cov & pad[:, 1:-1, :-2] & pad[:, 1:-1, 2:] & pad[:, :-2, 1:-1] & pad[:, 2:, 1:-1]  # no background neighbour
    crossing = (tri[:, :, 1:] != tri[:, :, :-1]) & inner[:, :, 1:] & inner[:, :, :-1]
    assert crossing.any(), "no pair straddles the shared edge away from the outline"
    assert torch.equal(out[:, 0][inner], image[:, 0][inner])  # the shared edge is no silhouette edge
    assert stats["blended"] > 0 and not torch.equal(out, image)  # the outer edges are


def test_edge_adjacency_closed_open_and_non_manifold():
    _, f = aref.small_sphere()
    adj = AA._edge_adjacency_host(f)
    assert adj.dtype == np.int32 and adj.shape == f.shape and (adj >= 0).all()  # closed: every edge has its one neighbour
    assert np.array_equal(adj, aref.edge_adjacency_ref(f))
    for fi in range(len(f)):  # the neighbour holds the same vertex pair
        for k in range(3):
            assert {f[fi, (k + 1) % 3], f[fi, (k + 2) % 3]} <= set(f[adj[fi, k]])
    # open strip of three triangles 0-1-2, 1-3-2, 2-3-4: interior edges (1,2) and (2,3); the other five edges are boundary
    strip = np.array([(0, 1, 2), (1, 3, 2), (2, 3, 4)], np.int64)
    assert AA._edge_adjacency_host(strip).tolist() == [[1, -1, -1], [2, 0, -1], [-1, -1, 1]]
    # fan of three faces on the edge (0, 1), plus a face that shares (1, 2) with the first: -1 exactly on the triple edge and
    # on the boundary
    fan = np.array([(0, 1, 2), (1, 0, 3), (0, 1, 4), (2, 1, 5)], np.int64)
    got = AA._edge_adjacency_host(fan)
    assert got.tolist() == [[3, -1, -1], [-1, -1, -1], [-1, -1, -1], [-1, -1, 0]]
    assert np.array_equal(got, aref.edge_adjacency_ref(fan))
    # a face that names one vertex twice does not become its own neighbour; no faces: an empty table
    assert AA._edge_adjacency_host(np.array([(0, 0, 1)], np.int64)).tolist() == [[-1, -1, -1]]
    assert AA._edge_adjacency_host(np.zeros((0, 3), np.int64)).shape == (0, 3)
    # the tensor front end: int32 on the faces' device, cached on the tensor until it changes in place
    ft = torch.from_numpy(fan)
    a0 = AA.edge_adjacency(ft)
    assert a0.dtype == torch.int32 and a0.tolist() == got.tolist() and AA.edge_adjacency(ft) is a0
    ft[3] = torch.tensor([2, 5, 6])
    assert AA.edge_adjacency(ft).tolist() == [[-1, -1, -1]] * 4
    assert AA.edge_adjacency(torch.from_numpy(strip)[None].expand(2, -1, -1)).tolist() == AA._edge_adjacency_host(strip).tolist()


def test_reference_gradient_matches_central_differences():
    """The restatement's analytic gradient against float64 central differences (step 1e-6 in NDC, tri and depth unchanged),
    one direction per face for a few faces of the sphere case that carry a silhouette gradient.  Marginal pairs carry no upstream
    gradient.  Bound 1e-6 relative: round-off of the difference quotient is ~1e-16 * |loss| / step ~ 1e-9 and the truncation
    term step^2 * f''' stays below it for edges longer than a pixel; the measured worst (6.8e-9) is printed."""
    v, f = aref.sphere_case(3)
    h, w = 70, 90
    vi, t, d = oracle_buffers(v, f, h, w)
    tri, depth, adj = torch.from_numpy(t), torch.from_numpy(d), aref.edge_adjacency_ref(f)
    rng = np.random.RandomState(7)
    image = torch.from_numpy(rng.uniform(0, 1, (3, 3, h, w)))
    G = torch.from_numpy(rng.standard_normal((3, 3, h, w)))

    v64 = torch.from_numpy(v.astype(np.float64)).requires_grad_(True)

    def loss(vv, g):
        out, stats = aref.antialias_ref(image, tri, depth, aref.face_vertices_ref(vv, vi, f, h, w, base=v64), adj)
        return (out * g).sum(), stats

    _, stats = loss(v64, G)
    G = G * (~stats["marginal_pixels"])[:, None]
    loss(v64, G)[0].backward()
    assert torch.all(v64.grad[..., 2] == 0)
    moved = torch.nonzero(v64.grad.abs().sum(-1) > 0)
    assert len(moved) > 30
    worst = 0.0
    step = 1e-6
    for b, vid in moved[rng.permutation(len(moved))[:6]].tolist():
        faces_of = np.flatnonzero((f == vid).any(1))[:2]
        dv = torch.zeros_like(v64)
        dv[b, np.unique(f[faces_of])] = torch.from_numpy(rng.standard_normal((len(np.unique(f[faces_of])), 3)))
        with torch.no_grad():
            (lp, sp), (lm, sm) = loss(v64 + step * dv, G), loss(v64 - step * dv, G)
        assert sp["blended"] == stats["blended"] == sm["blended"]
        fd, an = ((lp - lm) / (2 * step)).item(), (v64.grad * dv).sum().item()
        worst = max(worst, abs(fd - an) / max(abs(an), 1.0))
        assert abs(fd - an) <= 1e-6 * max(abs(an), 1.0), (b, vid, fd, an)
    print(f"restatement vs central differences: worst relative difference {worst:.2e}")


@pytest.mark.parametrize("name", list(aref.CASES))
def test_marginal_share_of_gpu_cases(name):
    """Every case of tests/test_gpu_antialias.py blends something, and at most 1 % of its blended pairs are marginal."""
    v, f, h, w, C = aref.CASES[name]()
    _, stats, _ = run_ref(v, f, h, w)
    share = stats["marginal"] / max(stats["blended"], 1)
    print(f"{name}: {stats['pairs']} pairs, {stats['blended']} blended, {stats['marginal']} marginal ({100 * share:.2f} %)")
    assert stats["blended"] > 0 and share <= MAX_MARGINAL, stats


def test_float32_run_classifies_like_float64():
    """The float32 run of the restatement (the tolerance yardstick of the GPU tests) blends the same pairs as the float64 run."""
    v, f, h, w, _ = aref.CASES["sphere_70x90_b3"]()
    s64 = run_ref(v, f, h, w)[1]
    s32 = run_ref(v, f, h, w, dtype=torch.float32)[1]
    assert (s64["pairs"], s64["blended"]) == (s32["pairs"], s32["blended"])


def test_argument_validation_without_gpu():
    lib = _lib.load()
    stream = None
    assert lib.gif_antialias_f32(None, None, None, None, None, None, 0, 3, 10, 8, 8, stream) == 0  # B = 0
    assert lib.gif_antialias_f32(None, None, None, None, None, None, 2, 3, 0, 8, 8, stream) == 0  # F = 0
    assert lib.gif_antialias_bwd_f32(None, None, None, None, None, None, None, None, 0, 3, 10, 8, 8, None, stream) == 0
    assert lib.gif_antialias_bwd_f32(None, None, None, None, None, None, None, None, 2, 3, 0, 8, 8, None, stream) == 0
    for dims in ((1, 0, 4, 8, 8), (1, -1, 4, 8, 8), (-1, 3, 4, 8, 8), (1, 3, -4, 8, 8), (1, 3, 4, 0, 8), (1, 3, 4, 8, -8)):
        assert lib.gif_antialias_f32(None, None, None, None, None, None, *dims, stream) == -1, dims
        assert b"bad dims" in lib.gif_last_error()
        assert lib.gif_antialias_bwd_f32(None, None, None, None, None, None, None, None, *dims, None, stream) == -1, dims
    assert lib.gif_antialias_f32(None, None, None, None, None, None, 1, 3, 4, 8, 8, stream) == -1
    assert b"null pointer" in lib.gif_last_error()
    # per (image, face, 64-row band): 8 floats, like the rasteriser's backward (16)
    assert lib.gif_antialias_bwd_workspace_bytes(3, 216, 70, 90) == 3 * 216 * 2 * 8 * 4
    assert lib.gif_antialias_bwd_workspace_bytes(3, 216, 70, 90) * 2 == lib.gif_rasterize_colors_bwd_workspace_bytes(3, 216, 70, 90)
    assert lib.gif_antialias_bwd_workspace_bytes(0, 216, 70, 90) == 8


def test_cpu_tensors_are_refused():
    v, f, h, w, _ = aref.CASES["border_11x13"]()
    vt, ft = torch.from_numpy(v), torch.from_numpy(f)
    tri, depth = torch.zeros(1, h, w, dtype=torch.int32), torch.zeros(1, h, w)
    with pytest.raises(_lib.GifHipError, match="device tensors"):
        AA.antialias(torch.zeros(1, 3, h, w), tri, depth, vt, ft)
    with pytest.raises(_lib.GifHipError, match="device tensors"):
        AA.rasterize_attributes_aa(vt, ft, torch.zeros_like(vt), h, w)
    with pytest.raises(_lib.GifHipError, match="device tensors"):
        AA.soft_silhouette(vt, ft, h, w)
