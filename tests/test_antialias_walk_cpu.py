"""CPU-side checks of the walking edge antialiasing: the restatement tests/antialias_walk_ref.py against
antialias_ref at zero hops (bit for bit), against hand-computed edges that the front pixel's face does not own, and against
central differences at vertices reached by walking only; the blend counts of the prototype the definition was drawn up with;
the marginal share of every case of tests/test_gpu_antialias_walk.py; and the new entry points' argument validation (before
any launch) — all on the oracle rasteriser's tri and depth buffers."""
import numpy as np
import pytest
import torch

import antialias_ref as aref
import antialias_walk_ref as wref
from gif_amd import _lib
from gif_amd import antialias as AA
from oracle import rasterize_oracle as ro

MAX_MARGINAL = 0.01  # of the blended pairs; a case with fewer than 100 blended pairs may have none

# case -> (blended pairs at the case's max_hops, blended pairs at zero hops, the deepest hop with a hit); all outline pairs but
# the edge mesh's, whose pairs lie between faces and on which walking adds nothing (it has boundary edges only)
EXPECTED = {
    "sphere_70x90_b3": (170 + 213 + 254, 86 + 97 + 152, 4),
    "sphere_64x64_b1": (170, 79, 4),
    "sphere24x30_70x90": (178, 23, 15),
    "sphere40x48_70x90": (158, 8, 8),
    "edges_70x70_b2": (590, 590, 0),
    "strip_12x12": (24, 10, 3),
    "strip_12x12_t": (24, 10, 3),
    "border_grid_11x13": (40, 11, 1),
}


def oracle_buffers(v, f, h, w):
    """(vi [B,V,3] float32 pixel-space vertices, tri, depth) of the oracle rasteriser for NDC vertices v [B,V,3]."""
    B = v.shape[0]
    vi = ro.to_image_space(v, h, w)
    fv = ro.face_vertices(vi, np.repeat(f[None], B, 0).astype(np.int32))
    d, t, b = ro.new_buffers(B, h, w)
    ro.standard_rasterize(fv, d, t, b, h, w)
    return vi, t, d


def run_walk(v, f, h, w, max_hops, image=None, dtype=torch.float64):
    vi, t, d = oracle_buffers(v, f, h, w)
    tri = torch.from_numpy(t)
    if image is None:
        image = (tri >= 0)[:, None].to(dtype)  # coverage as the image
    fv = aref.face_vertices_ref(torch.from_numpy(v).to(dtype), vi, f, h, w)
    out, stats = wref.antialias_walk_ref(image.to(dtype), tri, torch.from_numpy(d), fv, aref.edge_adjacency_ref(f), max_hops)
    return out, stats, tri


def test_sphere_generalises_small_sphere():
    v, f = wref.sphere(10, 12)
    v0, f0 = aref.small_sphere()
    assert np.array_equal(v, v0) and np.array_equal(f, f0)
    v, f = wref.sphere(24, 30)
    assert v.shape == (23 * 30 + 2, 3) and len(f) == 1380 and (aref.edge_adjacency_ref(f) >= 0).all()


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("name", list(aref.CASES))
def test_zero_hops_is_the_existing_restatement_bit_for_bit(name, dtype):
    v, f, h, w, C = aref.CASES[name]()
    vi, t, d = oracle_buffers(v, f, h, w)
    tri, depth, adj = torch.from_numpy(t), torch.from_numpy(d), aref.edge_adjacency_ref(f)
    image = torch.rand((v.shape[0], C, h, w), generator=torch.Generator().manual_seed(1), dtype=torch.float64).to(dtype)
    fv = aref.face_vertices_ref(torch.from_numpy(v).to(dtype), vi, f, h, w)
    out0, s0 = aref.antialias_ref(image, tri, depth, fv, adj)
    out1, s1 = wref.antialias_walk_ref(image, tri, depth, fv, adj, 0)
    assert out0.dtype == out1.dtype == dtype and torch.equal(out0, out1)
    assert (s0["pairs"], s0["blended"], s0["marginal"]) == (s1["pairs"], s1["blended"], s1["marginal"])
    assert torch.equal(s0["marginal_pixels"], s1["marginal_pixels"]) and s1["hits_per_hop"] == [s0["blended"]]


def test_walking_only_adds_blends():
    """64 x 64 sphere, hops 0, 1, 2, 4: the set of blended pairs only grows, a pair blended at fewer hops keeps its hit and its a,
    and the outline pairs that blend are the prototype's 79, 112, 160, 170 of 170."""
    v, f, h, w, _ = aref.CASES["sphere_64x64_b1"]()
    before, counts = {}, []
    for hops in (0, 1, 2, 4):
        _, s, _ = run_walk(v, f, h, w, hops)
        assert s["outline_pairs"] == 170 and sum(s["hits_per_hop"]) == s["blended"] == len(s["hits"])
        now = {tuple(r[:4]): (tuple(r[4:]), a) for r, a in zip(s["hits"].tolist(), s["hit_a"].tolist())}
        assert len(now) == s["blended"]
        for key, val in before.items():
            assert now.get(key) == val, (hops, key)  # same face, edge, hop and the same bits of a
        assert all(hit[2] <= hops for hit, _ in now.values())
        before = now
        counts.append(int(s["hits"][:, 7].sum()))
    assert counts == [79, 112, 160, 170]


def test_rectangle_edge_through_a_face_that_does_not_own_it():
    """The rectangle of test_half_pixel_edges_return_the_rasterisers_bits a quarter pixel to the right: the front pixel (9, 7) of
    the right edge's lowest row lies in the lower-left triangle, which does not own that edge.  One hop finds it."""
    v, f = wref.quarter_rectangle()
    out0, s0, _ = run_walk(v, f, 16, 16, 0)
    out1, s1, _ = run_walk(v, f, 16, 16, 1)
    assert torch.equal(out0[0, 0, 3:7, 10], torch.full((4,), 0.25, dtype=torch.float64)) and out0[0, 0, 7, 10] == 0
    assert torch.equal(out1[0, 0, 3:8, 10], torch.full((5,), 0.25, dtype=torch.float64))
    assert torch.equal(out1[0, 0, 3:8, 4], torch.full((5,), 0.75, dtype=torch.float64))
    assert s1["blended"] > s0["blended"] and s1["hits_per_hop"][1] > 0


@pytest.mark.parametrize("transpose", [False, True], ids=["rows", "columns"])
@pytest.mark.parametrize("edge", [5.3, 5.7])
def test_strip_edge_through_faces_narrower_than_a_pixel(edge, transpose):
    """The strip mesh: the outline at x = E + 0.03 j on vertex row j lies behind two columns of cells narrower than a pixel, so most
    front pixels lie in faces that do not own it.  Four hops blend all 24 outline pairs (zero hops: 10; deepest hit at hop 3), and
    on each row pixel 5 and pixel 6 take the covered share of their area for that row's edge position."""
    v, f = wref.strip_mesh(edge, transpose)
    out0, s0, _ = run_walk(v, f, 12, 12, 0)
    out, s, _ = run_walk(v, f, 12, 12, 4)
    assert s["outline_pairs"] == 24 and s0["blended"] == 10 and s["blended"] == 24 and s["marginal"] == 0
    assert s["hits_per_hop"][3] > 0 and s["hits_per_hop"][4] == 0
    line = out[0, 0].T if transpose else out[0, 0]  # [12 lines, 12 pixels across the edge]
    rows = wref.STRIP_ROWS
    for y in range(12):
        j = max(i for i in range(len(rows) - 1) if rows[i] <= y)
        x_e = wref.strip_edge(edge, j + (y - rows[j]) / (rows[j + 1] - rows[j]))
        assert abs(line[y, 5].item() - min(1.0, x_e - 4.5)) <= 1e-6 and abs(line[y, 6].item() - max(0.0, x_e - 5.5)) <= 1e-6, (y, line[y])
        assert (line[y, 2:5] == 1).all() and (line[y, 7:] == 0).all()
    # no skew: the edge of the definition's example, 0.8 / 0.0 and 1.0 / 0.2
    v, f = wref.strip_mesh(edge, transpose, skew=0.0)
    out, s, _ = run_walk(v, f, 12, 12, 4)
    line = out[0, 0].T if transpose else out[0, 0]
    assert (line[:, 5] - min(1.0, edge - 4.5)).abs().max() <= 1e-6 and (line[:, 6] - max(0.0, edge - 5.5)).abs().max() <= 1e-6


def test_reference_gradient_matches_central_differences_after_a_walk():
    """test_antialias_cpu's check (float64 central differences, step 1e-6 in NDC, bound 1e-6 relative, tri and depth unchanged;
    marginal pairs carry no upstream gradient) with max_hops = 8, at vertices whose whole gradient comes from hits at hop >= 1:
    endpoints of such hit edges that are endpoints of no hit edge at hop 0.  The bound's argument holds as there: the edges of the
    10 x 12 sphere at 70 x 90 are longer than a pixel.  Eight such vertices carry a gradient; the worst relative difference measured is 8.2e-10
    (printed)."""
    v, f = aref.sphere_case(3)
    h, w, hops = 70, 90, 8
    vi, t, d = oracle_buffers(v, f, h, w)
    tri, depth, adj = torch.from_numpy(t), torch.from_numpy(d), aref.edge_adjacency_ref(f)
    rng = np.random.RandomState(7)
    image = torch.from_numpy(rng.uniform(0, 1, (3, 3, h, w)))
    G = torch.from_numpy(rng.standard_normal((3, 3, h, w)))
    v64 = torch.from_numpy(v.astype(np.float64)).requires_grad_(True)

    def loss(vv, g):
        out, stats = wref.antialias_walk_ref(image, tri, depth, aref.face_vertices_ref(vv, vi, f, h, w, base=v64), adj, hops)
        return (out * g).sum(), stats

    _, stats = loss(v64, G)
    G = G * (~stats["marginal_pixels"])[:, None]
    loss(v64, G)[0].backward()
    assert torch.all(v64.grad[..., 2] == 0)
    ends = {0: set(), 1: set()}  # (image, vertex) endpoints of hit edges found at hop 0 / later
    for _, b, _, _, face, k, hop, _ in stats["hits"].tolist():
        ends[min(hop, 1)] |= {(b, int(f[face, (k + 1) % 3])), (b, int(f[face, (k + 2) % 3]))}
    walked = sorted(p for p in ends[1] - ends[0] if v64.grad[p].abs().sum() > 0)
    assert len(walked) > 0
    worst = 0.0
    step = 1e-6
    for i in rng.permutation(len(walked))[:6]:
        dv = torch.zeros_like(v64)
        dv[walked[i]] = torch.from_numpy(rng.standard_normal(3))
        with torch.no_grad():
            (lp, sp), (lm, sm) = loss(v64 + step * dv, G), loss(v64 - step * dv, G)
        assert torch.equal(sp["hits"], stats["hits"]) and torch.equal(sm["hits"], stats["hits"])
        fd, an = ((lp - lm) / (2 * step)).item(), (v64.grad * dv).sum().item()
        worst = max(worst, abs(fd - an) / max(abs(an), 1.0))
        assert abs(fd - an) <= 1e-6 * max(abs(an), 1.0), (walked[i], fd, an)
    print(f"walking restatement vs central differences: {len(walked)} walked-only vertices, worst relative difference {worst:.2e}")


@pytest.mark.parametrize("name", list(wref.WALK_CASES))
def test_gpu_cases_blend_by_walking_alike_in_both_formats(name):
    """Every case of tests/test_gpu_antialias_walk.py: the blend counts are the prototype's, something blends at a hop >= 1 (but on
    the edge mesh, where nothing may), the float32 and float64 runs blend the same pairs with the same hit edges at the same hops,
    and at most 1 % of the blended pairs are marginal (none where fewer than 100 blend)."""
    v, f, h, w, C, hops = wref.WALK_CASES[name]()
    _, s, _ = run_walk(v, f, h, w, hops)
    _, s32, _ = run_walk(v, f, h, w, hops, dtype=torch.float32)
    _, s0, _ = run_walk(v, f, h, w, 0)
    share = s["marginal"] / max(s["blended"], 1)
    print(f"{name}: {s['pairs']} pairs ({s['outline_pairs']} outline), {s['blended']} blended ({s0['blended']} at zero hops), per hop "
          f"{s['hits_per_hop']}, {s['marginal']} marginal ({100 * share:.2f} %), {s['marginal_blended']} of them blended")
    blended, at_zero, deepest = EXPECTED[name]
    assert (s["blended"], s0["blended"]) == (blended, at_zero)
    assert max(i for i, n in enumerate(s["hits_per_hop"]) if n) == deepest
    assert (sum(s["hits_per_hop"][1:]) > 0) == (name != "edges_70x70_b2")
    assert torch.equal(s["hits"], s32["hits"]) and s["pairs"] == s32["pairs"]
    assert share <= MAX_MARGINAL and (s["blended"] >= 100 or s["marginal"] == 0), s
    if name == "sphere40x48_70x90":  # the cap cuts walks short here: kernel and restatement must stop at the same hop
        assert run_walk(v, f, h, w, 16)[1]["blended"] == 172


def test_argument_validation_without_gpu():
    lib = _lib.load()
    stream = None
    fwd = lambda *dims: lib.gif_antialias_walk_f32(None, None, None, None, None, None, *dims, stream)
    bwd = lambda *dims: lib.gif_antialias_walk_bwd_f32(None, None, None, None, None, None, None, None, *dims, None, stream)
    for fn in (fwd, bwd):
        assert fn(0, 3, 10, 8, 8, 2) == 0  # B = 0
        assert fn(2, 3, 0, 8, 8, 2) == 0  # F = 0
        for dims in ((1, 0, 4, 8, 8), (1, -1, 4, 8, 8), (-1, 3, 4, 8, 8), (1, 3, -4, 8, 8), (1, 3, 4, 0, 8), (1, 3, 4, 8, -8)):
            assert fn(*dims, 2) == -1, dims
            assert b"bad dims" in lib.gif_last_error()
        for hops in (-1, 65):
            for dims in ((1, 3, 4, 8, 8), (0, 3, 10, 8, 8), (2, 3, 0, 8, 8)):  # refused before the empty-work rules as well
                assert fn(*dims, hops) == -1, (dims, hops)
                assert b"max_hops" in lib.gif_last_error()
        for hops in (0, 64):
            assert fn(1, 3, 4, 8, 8, hops) == -1
            assert b"null pointer" in lib.gif_last_error()


def test_cpu_tensors_are_refused_with_hops():
    v, f, h, w, _ = aref.CASES["border_11x13"]()
    vt, ft = torch.from_numpy(v), torch.from_numpy(f)
    tri, depth = torch.zeros(1, h, w, dtype=torch.int32), torch.zeros(1, h, w)
    with pytest.raises(_lib.GifHipError, match="device tensors"):
        AA.antialias(torch.zeros(1, 3, h, w), tri, depth, vt, ft, max_hops=2)
    with pytest.raises(_lib.GifHipError, match="device tensors"):
        AA.rasterize_attributes_aa(vt, ft, torch.zeros_like(vt), h, w, max_hops=2)
    with pytest.raises(_lib.GifHipError, match="device tensors"):
        AA.soft_silhouette(vt, ft, h, w, max_hops=2)
    for bad in (-1, 65, 1.5, True, "2"):
        with pytest.raises(_lib.GifHipError, match="max_hops"):
            AA.soft_silhouette(vt, ft, h, w, max_hops=bad)
