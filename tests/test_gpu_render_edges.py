"""-m gpu: the resize, texture-map and vertex-normal kernels (csrc/resize.hip, csrc/mesh.hip) at the edges of their index arithmetic,
against an fp64 reference of the same operation.

Each row of the tables is a shape or an input placed on one predicate or piece of index arithmetic: make_taps' `src < 0` clamp, its
`i0 > nin - 1` clamp and the bicubic index clamp on both sides (resize.hip), the 256 * 64 workgroup cap of the resize launch, the
four x0ok / x1ok / y0ok / y1ok zeroings of bilinear_setup, the `t < TT` tail and the per-workgroup pre-sum of the invalid texels in
texture_map_bwd_kernel, `i >= B * V`, `off[v] == off[v + 1]`, the three corner branches of vertex_sum and fmaxf(len, 1e-6f)
(mesh.hip), and the offset fill and version check of render._topology.  Each row's comment names the predicate and the side.

Reference: torch.float64 on the CPU over exactly the fp32 operands the kernel reads: F.interpolate(align_corners=False),
F.grid_sample(bilinear, zeros, align_corners=False) on a grid built in fp64 from the barycentric point and the camera, the three
index_add_ passes + x / max(|x|, 1e-6) for the normals, and fp64 autograd of the same for the two backward passes.  Bound, per
element:

    |got - ref| <= TOL[family] * R + COORD[family] * S + TINY

R is the same operation on absolute values (bicubic: the absolute tap weights; normals: the first-order sensitivity of
x / max(|x|, eps) applied to the sum of the |cross-product terms|, plus |n| for the square root and the division).  S carries the one
error no operand magnitude does: the sample coordinate is formed in fp32.  S = |d value / d coordinate| x the coordinate's magnitude
(the sum of the absolute terms it is formed from), forward; |g| x |d weight / d coordinate| x that magnitude per scattered weight,
backward.  Values are continuous in the coordinate (zero padding included), but a derivative is not where a tap index flips: S is the
larger of the two one-sided values, evaluated at the coordinate moved by -/+ SHIFT x its magnitude.  A row whose coordinates are exact
in fp32 (a power-of-two scale; dyadic vertices, barycentric weights and cameras) passes no S at all: it is held to TOL * R alone.

Bicubic, a finding of the first measurement: against R alone the bicubic rows reached 9.4e-6 (rs_9x12) where the coordinate term explains
1e-7.  The cause is not the kernel's indexing: make_taps evaluates the cubic-convolution weights in Horner form in fp32
(cubic2(t) = ((A t - 5A) t + 8A) t - 4A: terms of size 4 .. 12 cancel to a weight below 0.1), so a weight carries an absolute
rounding of a few 2^-24 x the size of those terms, whatever its own size, and a tap with a near-zero weight on a large pixel is not
covered by |w| |x|.  ATen's own fp32 kernel shows the same figure against the fp64 one (9.2e-6 on the same row).  Like the coordinate,
this is an error of the weight that no operand magnitude carries, so it joins S: per tap, the same Horner polynomial on absolute
values (_cubic_weights) in place of |d w / d coordinate| x magnitude.  At the dyadic fractions of a power-of-two scale every product
of the polynomial is exact, so the exact rows still pass no S.  Bilinear weights (1 - l, l) round relative to themselves: nothing added.

The restatements written here (taps, grids, scatter, Jacobian) are tied to ATen's float64 results without a GPU in
tests/test_cpu_wiring.py (test_render_edges_*).

Observed on the MI355X (all rows of this module; the larger of three runs, the atomic backward passes differ between runs) and the
constants chosen from it.  tol: worst |got - ref| / R over the rows without S.  coord: worst (|got - ref| - tol * R) / S over the
rows with S, tol being the observed value of the same family.
  family         tol (row)                          TOL             coord (row)                          COORD
  bilinear       1.96e-7 (rs_gridcap)               9e-7   (4.6 x)  5.66e-8 (rs_9x12)                    2.5e-7 (4.4 x)
  bilinear_bwd   2.89e-7 (rs_gridcap)               1.3e-6 (4.5 x)  4.21e-8 (rs_down_16)                 2e-7   (4.7 x)
  bicubic        2.60e-7 (rs_gridcap)               1.2e-6 (4.6 x)  1.48e-8 (rs_down_16)                 7e-8   (4.7 x)
  bicubic_bwd    5.59e-7 (rs_gridcap)               2.5e-6 (4.5 x)  3.34e-8 (rs_down_16)                 1.5e-7 (4.5 x)
  texmap         1.14e-7 (tx_t32_5x12_c4)           5e-7   (4.4 x)  1.07e-7 (tx_t32_12x5_c1_rand)        5e-7   (4.7 x)
  texmap_bwd     1.63e-7 (tx_t21_5x12_b3 all)       7.5e-7 (4.6 x)  6.14e-8 (tx_t32_12x5_c1_rand all)    2.8e-7 (4.6 x)
  normals        1.03e-7 (vn_v255)                  4.5e-7 (4.4 x)  -
The bicubic coord figures are small because their S is dominated by the polynomial on absolute values, a worst-case magnitude (up
to 20 per weight); against R alone the same rows stand at 9.4e-6 (forward, rs_9x12) and 1.8e-5 (backward, rs_down_16).
Every case prints its ratios ("[route ratio]" lines with -s) so that a re-measurement is one run of this module."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

NAN = float("nan")
U32 = 2.0 ** -24  # unit round-off of fp32
SHIFT = 16 * U32  # relative coordinate shift at which the one-sided derivatives of S are taken
EPS = 1e-6  # F.normalize eps of the reference's vertex_normals
TINY = 1e-30

# per-element tolerances (see the module docstring for the measurements behind them)
TOL = {"bilinear": 9e-7, "bicubic": 1.2e-6, "bilinear_bwd": 1.3e-6, "bicubic_bwd": 2.5e-6, "texmap": 5e-7, "texmap_bwd": 7.5e-7,
       "normals": 4.5e-7}
COORD = {"bilinear": 2.5e-7, "bicubic": 7e-8, "bilinear_bwd": 2e-7, "bicubic_bwd": 1.5e-7, "texmap": 5e-7, "texmap_bwd": 2.8e-7}
WORST = {}  # (family, "tol" | "coord") -> (worst ratio so far, case)


def _note(fam, what, r_tol, r_coord):
    line = f"\n[route ratio] {fam} {what}:"
    for kind, r in (("tol", r_tol), ("coord", r_coord)):
        if r is None:
            continue
        key = (fam, kind)
        if key not in WORST or r > WORST[key][0]:
            WORST[key] = (r, what)
        line += f" {kind} {r:.3e} (module worst so far {WORST[key][0]:.3e} at {WORST[key][1]})"
    print(line)


def _check(got, ref, R, fam, what, extra=None):
    """|got - ref| <= TOL * R + COORD * extra + TINY element-wise.  got: any tensor (moved to CPU fp64); ref, R: fp64 CPU; extra: the
    coordinate sensitivity S (fp64 CPU) or None for a row whose coordinates are exact in fp32."""
    got = got.detach().double().cpu()
    assert got.shape == ref.shape == R.shape, (what, got.shape, ref.shape, R.shape)
    assert torch.isfinite(got).all(), f"{what}: {int((~torch.isfinite(got)).sum())} non-finite elements"
    err = (got - ref).abs()
    if extra is None:
        ex = torch.zeros_like(R)
        r_coord = None
    else:
        assert extra.shape == R.shape, (what, extra.shape, R.shape)
        ex = COORD[fam] * extra
        r_coord = ((err - TOL[fam] * R).clamp_min(0) / (extra + TINY)).max().item() if err.numel() else 0.0
    r_tol = ((err - ex).clamp_min(0) / (R + TINY)).max().item() if err.numel() else 0.0
    _note(fam, what, r_tol, r_coord)
    bad = err > TOL[fam] * R + ex + TINY
    if bad.any():
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{what} [{fam}]: {int(bad.sum())} of {bad.numel()} elements out of bound; first at {i}: got "
                             f"{got[i].item():.9e} ref {ref[i].item():.9e} R {R[i].item():.3e} S {ex[i].item():.3e}; worst ratio "
                             f"{r_tol:.3e} > {TOL[fam]:.1e}")


def _rng(seed):
    return torch.Generator().manual_seed(seed)


def _poison(*numels):
    """Leave NaN-filled blocks of these sizes in the caching allocator, so that an output the kernel never writes reads NaN."""
    ts = [torch.full((n,), NAN, device="cuda") for n in numels for _ in range(4)]
    del ts


# ---------------------------------------------------------------------------------------------------------------------------------
# a. resize (csrc/resize.hip: make_taps, resize_fwd_kernel, resize_bwd_kernel) through data.fast_image_reshape
# ---------------------------------------------------------------------------------------------------------------------------------
CUBIC_A = -0.75


def _cubic_weights(x):
    """Cubic-convolution weights of the taps i0 - 1 .. i0 + 2 at fraction x (fp64), their derivatives in x, and the same Horner
    polynomials on absolute values (the magnitude their fp32 evaluation rounds at): [..., 4] each."""
    A = CUBIC_A

    def c1(t):
        return ((A + 2) * t - (A + 3)) * t * t + 1, (3 * (A + 2) * t - 2 * (A + 3)) * t, ((A + 2) * t + (A + 3)) * t * t + 1

    def c2(t):
        return ((A * t - 5 * A) * t + 8 * A) * t - 4 * A, (3 * A * t - 10 * A) * t + 8 * A, ((-A * t - 5 * A) * t - 8 * A) * t - 4 * A

    (w0, d0, r0), (w1, d1, r1), (w2, d2, r2), (w3, d3, r3) = c2(x + 1), c1(x), c1(1 - x), c2(2 - x)
    return torch.stack([w0, w1, w2, w3], -1), torch.stack([d0, d1, -d2, -d3], -1), torch.stack([r0, r1, r2, r3], -1)


def _is_pow2(nin, nout):
    r = nin / nout
    return r > 0 and np.frexp(r)[0] == 0.5 and float(np.float32(r)) == r


def _taps(nin, nout, mode, shift=0.0):
    """fp64 taps of one axis: indices [nout, K], weights [nout, K], their derivatives in the source coordinate [nout, K], the
    coordinate's magnitude [nout], and the magnitude the weight itself rounds at, where that is no multiple of the weight (bicubic:
    the Horner polynomial on absolute values) [nout, K].  Both magnitudes are zero on an axis with a power-of-two scale: the fp32
    coordinate is exact, and the fraction is a multiple of 1/8, at which every product of the polynomial is exact as well.
    shift: relative move of the coordinate."""
    scale = nin / nout
    d = torch.arange(nout, dtype=torch.float64)
    inexact = 0.0 if _is_pow2(nin, nout) else 1.0
    assert inexact or scale >= 0.25
    mag = inexact * (scale * (d + 0.5) + 0.5)
    s = scale * (d + 0.5) - 0.5 + shift * mag
    if mode == "bilinear":
        free = (s >= 0).double()  # src < 0 is clamped to 0: the value no longer depends on the coordinate
        s = s.clamp_min(0)
        i0 = s.floor().long().clamp_max(nin - 1)
        i1 = i0 + (i0 < nin - 1).long()
        lam = s - i0
        return torch.stack([i0, i1], 1), torch.stack([1 - lam, lam], 1), torch.stack([-free, free], 1), mag, torch.zeros(nout, 2).double()
    fl = s.floor()
    w, dw, wr = _cubic_weights(s - fl)
    idx = (fl.long()[:, None] + torch.arange(-1, 3)).clamp(0, nin - 1)
    return idx, w, dw, mag, inexact * wr


def _scatter(idx, w, nin):
    return torch.zeros(idx.shape[0], nin, dtype=torch.float64).scatter_add_(1, idx, w)


def _axis(nin, nout, mode):
    """Dense [nout, nin] matrices of one axis: M (signed weights), Ma (absolute weights), Ds (the signed derivative on either side
    of a tap flip), Da (absolute derivatives, element-wise larger side), Mr (rounding magnitudes of the weights), and the
    coordinate magnitude."""
    idx, w, _, mag, wr = _taps(nin, nout, mode)
    Ds, Da = [], torch.zeros(nout, nin, dtype=torch.float64)
    for sh in (-SHIFT, SHIFT):
        i2, _, dw2, _, _ = _taps(nin, nout, mode, sh)
        Ds.append(_scatter(i2, dw2, nin))
        Da = torch.maximum(Da, _scatter(i2, dw2.abs(), nin))
    return dict(M=_scatter(idx, w, nin), Ma=_scatter(idx, w.abs(), nin), Ds=Ds, Da=Da, Mr=_scatter(idx, wr, nin), mag=mag)


def _sep(My, x, Mx):
    """rows first, then columns: y[.., o, p] = sum_ij My[o, i] x[.., i, j] Mx[p, j]"""
    return My @ x @ Mx.T


RS_ROWS = [
    # name, layout, (Hi, Wi), (Ho, Wo)      layout: N x C planes; "view" = a non-contiguous NCHW view of an NHWC buffer
    ("rs_1x1", (1, 3), (1, 1), (5, 7)),          # nin 1: bilinear i0 = i1 = 0; all four bicubic taps clamp to 0, on both sides at once
    ("rs_1x9_h4", (1, 3), (1, 9), (4, 9)),       # a 1-pixel axis next to an identity axis; H scale 0.25: src < 0 on outputs 0, 1
    ("rs_2x3", (1, 3), (2, 3), (9, 11)),         # nin <= 3: bicubic taps clamped below and above in one tap set; src < 0 on 0..1
    ("rs_3x3_up16", (1, 3), (3, 3), (16, 16)),   # scale 3/16: src < 0 on outputs 0 .. 2 and src > nin - 1 on 13 .. 15 (i0 clamp)
    ("rs_identity", (1, 3), (7, 5), (7, 5)),     # scale 1: src = dst, every fraction 0
    ("rs_down_16", (1, 3), (16, 16), (5, 3)),    # non-integer down-scale 3.2 / 5.33: taps skip source pixels
    ("rs_9x12", (1, 3), (9, 12), (31, 17)),      # different scales on the two axes, planes > 1
    ("rs_33x31", (1, 3), (33, 31), (8, 64)),     # one axis down (4.125), the other up (0.484); Wo 64 > one wave per row
    ("rs_exact_4x6", (1, 3), (4, 6), (8, 3)),    # scales 0.5 and 2: every fp32 coordinate exact (no S term)
    ("rs_planes1", (1, 1), (5, 4), (3, 9)),      # planes 1: pl = 0 only
    ("rs_view_2x3", (2, 3), (6, 7), (11, 4)),    # planes 2 * 3 from a non-contiguous view: the wrapper's contiguous() copy
    # total 5 * 1024 * 1024 = 5 242 880 > 256 * 64 * 256 = 4 194 304: lanes of the first 4096 workgroups take a second trip, which
    # lands in plane 4.  Scale 0.5: every coordinate exact.
    ("rs_gridcap", (1, 5), (512, 512), (1024, 1024)),
]
RS_VIEW = {"rs_view_2x3"}
RS_MODES = ["bilinear", "bicubic"]


@functools.lru_cache(maxsize=2)
def _resize_case(name, mode):
    """Operands, fp64 restatement and bounds of one row (shared by the GPU test and the CPU check; nothing in it is modified)."""
    _, (N, C), (Hi, Wi), (Ho, Wo) = next(r for r in RS_ROWS if r[0] == name)
    g = _rng(20 + [r[0] for r in RS_ROWS].index(name))
    if name in RS_VIEW:
        x = torch.randn(N, Hi, Wi, C, generator=g).permute(0, 3, 1, 2)
        gy = torch.randn(N, Ho, Wo, C, generator=g).permute(0, 3, 1, 2)
    else:
        x, gy = torch.randn(N, C, Hi, Wi, generator=g), torch.randn(N, C, Ho, Wo, generator=g)
    ay, ax = _axis(Hi, Ho, mode), _axis(Wi, Wo, mode)
    xd, gd = x.double(), gy.double()
    exact = not (ay["mag"].any() or ax["mag"].any())
    c = dict(x=x, gy=gy, exact=exact, fwd=_sep(ay["M"], xd, ax["M"]), R=_sep(ay["Ma"], xd.abs(), ax["Ma"]),
             bwd=_sep(ay["M"].T, gd, ax["M"].T), Rb=_sep(ay["Ma"].T, gd.abs(), ax["Ma"].T), S=None, Sb=None)
    if not exact:
        sy = torch.stack([_sep(D, xd, ax["M"]).abs() for D in ay["Ds"]]).amax(0) * ay["mag"][:, None]
        sx = torch.stack([_sep(ay["M"], xd, D).abs() for D in ax["Ds"]]).amax(0) * ax["mag"][None, :]
        c["S"] = sy + sx + _sep(ay["Mr"], xd.abs(), ax["Ma"]) + _sep(ay["Ma"], xd.abs(), ax["Mr"])
        c["Sb"] = (_sep((ay["Da"] * ay["mag"][:, None] + ay["Mr"]).T, gd.abs(), ax["Ma"].T)
                   + _sep(ay["Ma"].T, gd.abs(), (ax["Da"] * ax["mag"][:, None] + ax["Mr"]).T))
    return c


def _interp64(x, size, mode):
    return F.interpolate(x, size=size, mode=mode, align_corners=False)


@pytest.mark.parametrize("mode", RS_MODES)
@pytest.mark.parametrize("row", RS_ROWS, ids=[r[0] for r in RS_ROWS])
def test_resize(row, mode):
    from gif_amd.data import fast_image_reshape
    name, (N, C), (Hi, Wi), (Ho, Wo) = row
    c = _resize_case(name, mode)
    x = c["x"].cuda().requires_grad_(True)
    gy = c["gy"].cuda()
    assert x.is_contiguous() == (name not in RS_VIEW) and gy.is_contiguous() == (name not in RS_VIEW)
    _poison(N * C * Ho * Wo)
    y = fast_image_reshape(x, Wo, Ho, mode=mode)  # (the wrapper returns width_out rows)
    assert y.shape == (N, C, Ho, Wo)
    xd = c["x"].double().requires_grad_(True)
    ref = _interp64(xd, (Ho, Wo), mode)
    _check(y, ref.detach(), c["R"], mode, f"{name} {mode}", extra=c["S"])
    _poison(N * C * Hi * Wi)
    y.backward(gy)
    (gref,) = torch.autograd.grad(ref, xd, c["gy"].double())
    _check(x.grad, gref, c["Rb"], f"{mode}_bwd", f"{name} {mode} bwd", extra=c["Sb"])
    if name == "rs_identity" and mode == "bilinear":
        assert torch.equal(y.detach().cpu(), c["x"]) and torch.equal(x.grad.cpu(), c["gy"])  # weights (1, 0): exact


# ---------------------------------------------------------------------------------------------------------------------------------
# b. texture map (csrc/mesh.hip: texel_grid, bilinear_setup, texture_map_kernel, texture_map_bwd_kernel) through _TextureMapFn
# ---------------------------------------------------------------------------------------------------------------------------------
# Named texels of the exact rows: grid coordinates (gx, gy) for the camera (1, 0, 0).  Pixel ix = ((gx + 1) * W - 1) / 2:
# gx = -1.0625 gives ix in (-1, 0) (x0 outside, x1 = 0 inside) and gx = 0.9375 gives ix in (W - 1, W) (x0 = W - 1 inside, x1 outside)
# for every W used here; likewise gy.
TX_NAMED = [
    # name, gx, gy, taps inside the image (for H, W >= 2)
    ("inside", 0.1875, -0.3125, 4),        # all of x0ok, x1ok, y0ok, y1ok
    ("left", -1.0625, 0.25, 2),            # x0ok false alone
    ("right", 0.9375, -0.25, 2),           # x1ok false alone
    ("top", 0.25, -1.0625, 2),             # y0ok false alone
    ("bottom", -0.25, 0.9375, 2),          # y1ok false alone
    ("top_left", -1.0625, -1.0625, 1),     # x0ok and y0ok false: only (y1, x1) left
    ("top_right", 0.9375, -1.0625, 1),     # x1ok and y0ok false
    ("bottom_left", -1.0625, 0.9375, 1),   # x0ok and y1ok false
    ("bottom_right", 0.9375, 0.9375, 1),   # x1ok and y1ok false
    ("out_right", 3.0, 0.5, 0),            # wholly outside: every weight zero
    ("out_top", -0.5, -1.75, 0),
    ("out_corner", 1.75, 1.75, 0),
    ("centre", 0.0, 0.0, None),            # grid (0, 0) exactly: shares its taps with the invalid texels
]
TX_CAMS_EXACT = [(1.0, 0.0, 0.0), (0.5, 0.25, -0.5), (1.25, -0.125, 0.0625)]
TX_V = 16

TX_ROWS = [
    # name, T, (H, W), C, B, map, exact
    #   map "wg2_invalid": T 21, TT 441 = 256 + 185: workgroup 1 of the backward is the tail (185 live lanes, 71 with t >= TT) and
    #   holds invalid texels only; workgroup 0 mixes both.  "all": T 16, TT 256 = one workgroup, no invalid texel (s == 0: the
    #   centre contribution is skipped).  "interleaved": T 32, four workgroups, every third texel invalid inside every wave.
    ("tx_t21_8x8", 21, (8, 8), 3, 1, "wg2_invalid", True),
    ("tx_t21_8x8_rand", 21, (8, 8), 3, 1, "wg2_invalid", False),    # the same with coordinates that round in fp32
    ("tx_t16_8x8", 16, (8, 8), 3, 1, "all", True),
    ("tx_t16_1x1_c4", 16, (1, 1), 4, 1, "all", True),               # H = W = 1: every sample has at least two taps outside
    ("tx_t32_5x12_c4", 32, (5, 12), 4, 1, "interleaved", True),     # H < W, H odd: the centre row is an integer coordinate
    ("tx_t32_12x5_c1_rand", 32, (12, 5), 1, 1, "interleaved", False),  # H > W, C 1
    ("tx_t21_12x5_c1", 21, (12, 5), 1, 1, "wg2_invalid", True),
    ("tx_t21_5x12_b3", 21, (5, 12), 3, 3, "wg2_invalid", True),     # B 3: one mesh, three cameras (blockIdx.y, the b * TT offsets)
    ("tx_t32_8x8_c4_b3_rand", 32, (8, 8), 4, 3, "interleaved", False),
    ("tx_t16_1x1_c1_rand", 16, (1, 1), 1, 1, "all", False),
]


def _tex_mesh(g):
    """16 vertices.  0..2 and 3..5: the two halves of the square [-4, 4]^2 (dyadic corners), normals z < 0 and > 0; 6..14: three
    random triangles (normal z of one sign inside a triangle, |z| >= 0.1, so that |interpolated nz| >= 0.1); 15 unused."""
    v = torch.empty(TX_V, 3)
    v[:6, :2] = torch.tensor([[-4.0, -4.0], [4.0, -4.0], [-4.0, 4.0], [4.0, 4.0], [-4.0, 4.0], [4.0, -4.0]])
    v[6:, :2] = torch.rand(10, 2, generator=g) * 2.6 - 1.3
    v[:, 2] = torch.randn(TX_V, generator=g)
    nrm = torch.randn(TX_V, 3, generator=g)
    sign = torch.tensor([-1.0] * 3 + [1.0] * 3 + [-1.0] * 3 + [1.0] * 3 + [-1.0] * 4)
    nrm[:, 2] = sign * (0.1 + torch.rand(TX_V, generator=g))
    return v, nrm


def _tex_valid(T, kind):
    t = torch.arange(T * T)
    if kind == "all":
        return torch.ones(T * T, dtype=torch.bool)
    if kind == "interleaved":
        return t % 3 != 0
    assert kind == "wg2_invalid" and T * T > 256
    return (t < 256) & (t % 7 != 3)


@functools.lru_cache(maxsize=None)
def _tex_case(name):
    """Operands of one row (fp32 / int32 CPU tensors, as the kernel reads them)."""
    _, T, (H, W), C, B, kind, exact = next(r for r in TX_ROWS if r[0] == name)
    g = _rng(40 + [r[0] for r in TX_ROWS].index(name))
    verts, normals = _tex_mesh(g)
    valid = _tex_valid(T, kind)
    N = int(valid.sum())
    if exact:
        # targets on the lattice k / 16, |k| <= 24 (ix exact; +-1 and integer pixel coordinates among them), the named ones first
        tgt = torch.randint(-24, 25, (N, 2), generator=g).double() / 16
        tgt[:len(TX_NAMED)] = torch.tensor([[gx, gy] for _, gx, gy, _ in TX_NAMED])
        px, py = tgt[:, 0], -tgt[:, 1]  # camera (1, 0, 0): gx = px, gy = -py
        lower = px + py <= 0  # triangle (0, 1, 2): p = v0 + 8 b1 ex + 8 b2 ey; otherwise (3, 4, 5): p = v3 - 8 b1 ex - 8 b2 ey
        b1 = torch.where(lower, (px + 4) / 8, (4 - px) / 8)
        b2 = torch.where(lower, (py + 4) / 8, (4 - py) / 8)
        tbc = torch.stack([1 - b1 - b2, b1, b2], 1).float()
        assert torch.equal(tbc.double().sum(1), torch.ones(N, dtype=torch.float64)) and (tbc >= 0).all()
        tfaces = torch.where(lower[:, None], torch.tensor([0, 1, 2]), torch.tensor([3, 4, 5])).int()
        cam = torch.tensor(TX_CAMS_EXACT[:B])
    else:
        tri = torch.randint(0, 3, (N,), generator=g)
        tfaces = (6 + 3 * tri[:, None] + torch.arange(3)).int()
        e = -torch.rand(N, 3, generator=g).clamp_min(1e-6).log()
        tbc = (e / e.sum(1, keepdim=True)).float()  # Dirichlet(1, 1, 1)
        cam = torch.stack([0.8 + 0.7 * torch.rand(B, generator=g), 0.6 * torch.rand(B, generator=g) - 0.3,
                           0.6 * torch.rand(B, generator=g) - 0.3], 1)
    tmap = torch.full((T * T,), -1, dtype=torch.int32)
    tmap[valid] = torch.randperm(N, generator=g).int()  # (not monotone in t: map[t] is an index, not a rank)
    return dict(T=T, H=H, W=W, C=C, B=B, exact=exact, img=torch.randn(B, C, H, W, generator=g),
                verts=verts[None].repeat(B, 1, 1), normals=normals[None].repeat(B, 1, 1), cam=cam, tmap=tmap, tfaces=tfaces,
                tbc=tbc, gtex=torch.randn(B, C, T, T, generator=g))


def _tex_grid(c):
    """fp64 grid of texel_grid over the fp32 operands: (grid [B,T,T,2], interpolated normal z [B,TT], valid [TT], magnitude of gx and
    gy [B,TT] = the sum of the absolute terms they are formed from)."""
    T, B = c["T"], c["B"]
    v, nz, bc, cam = c["verts"].double(), c["normals"].double()[..., 2], c["tbc"].double(), c["cam"].double()
    valid = c["tmap"] >= 0
    n = c["tmap"].long().clamp_min(0)
    f, b = c["tfaces"].long()[n], bc[n]  # [TT,3]
    terms = v[:, f, :2] * b[None, :, :, None]  # [B,TT,3,2]
    p, pa = terms.sum(2), terms.abs().sum(2)
    s, tx, ty = cam[:, 0:1], cam[:, 1:2], cam[:, 2:3]
    gx, gy = s * (p[..., 0] + tx), -(s * (p[..., 1] + ty))
    mx, my = s.abs() * (pa[..., 0] + tx.abs()), s.abs() * (pa[..., 1] + ty.abs())
    zero = torch.zeros_like(gx)
    gx, gy, mx, my = (torch.where(valid[None], t, zero) for t in (gx, gy, mx, my))  # invalid texels sample (0, 0), exactly
    nzi = torch.where(valid[None], (nz[:, f] * b[None]).sum(2), zero)
    return torch.stack([gx, gy], -1).view(B, T, T, 2), nzi, valid, torch.stack([mx, my], -1)


def _bilinear_taps(ix, iy, H, W):
    """The four taps of bilinear_setup in fp64: flat index [4, ...] (clamped into the image), weight, d weight / d ix,
    d weight / d iy (all zero for a tap outside the image)."""
    x0, y0 = ix.floor(), iy.floor()
    ax, ay = ix - x0, iy - y0
    out = []
    for dy, dx, w, wx, wy in ((0, 0, (1 - ax) * (1 - ay), -(1 - ay), -(1 - ax)), (0, 1, ax * (1 - ay), 1 - ay, -ax),
                              (1, 0, (1 - ax) * ay, -ay, 1 - ax), (1, 1, ax * ay, ay, ax)):
        xi, yi = x0.long() + dx, y0.long() + dy
        ok = ((xi >= 0) & (xi < W) & (yi >= 0) & (yi < H)).double()
        out.append((yi.clamp(0, H - 1) * W + xi.clamp(0, W - 1), ok * w, ok * wx, ok * wy, ok))
    return [torch.stack(t) for t in zip(*out)]


def _tex_restated(c, gtex):
    """Hand-written fp64 forward, backward and bounds: dict(fwd, R, S, bwd, Rb, Sb, ntaps) for the gradient gtex [B,C,T,T] (fp64)."""
    T, H, W, C, B = c["T"], c["H"], c["W"], c["C"], c["B"]
    grid, _, valid, gmag = _tex_grid(c)
    TT = T * T
    gx, gy = grid[..., 0].reshape(B, TT), grid[..., 1].reshape(B, TT)
    ix, iy = ((gx + 1) * W - 1) / 2, ((gy + 1) * H - 1) / 2
    v = valid[None].double()
    magx, magy = v * (0.5 * W * (gmag[..., 0] + 1) + 0.5), v * (0.5 * H * (gmag[..., 1] + 1) + 0.5)
    img = c["img"].double().reshape(B, C, H * W)
    g = gtex.reshape(B, C, TT)

    def gather(idx, wt, src):  # sum over taps of wt [4,B,TT] * src[b, c, idx [4,B,TT]] -> [B,C,TT]
        return sum(wt[k][:, None] * src.gather(2, idx[k][:, None].expand(B, C, TT)) for k in range(4))

    def scatter(idx, wt, src):  # [B,C,HW] += wt [4,B,TT] * src [B,C,TT] at idx
        out = torch.zeros(B, C, H * W, dtype=torch.float64)
        for k in range(4):
            out.scatter_add_(2, idx[k][:, None].expand(B, C, TT), wt[k][:, None] * src)
        return out

    idx, w, _, _, ok = _bilinear_taps(ix, iy, H, W)
    r = dict(fwd=gather(idx, w, img), R=gather(idx, w, img.abs()), bwd=scatter(idx, w, g), Rb=scatter(idx, w, g.abs()),
             ntaps=ok.sum(0))
    S, Sb = torch.zeros(B, C, TT, dtype=torch.float64), torch.zeros(B, C, H * W, dtype=torch.float64)
    for sx in (-SHIFT, SHIFT):
        for sy in (-SHIFT, SHIFT):
            i2, _, wx, wy, _ = _bilinear_taps(ix + sx * magx, iy + sy * magy, H, W)
            S = torch.maximum(S, gather(i2, wx, img).abs() * magx[:, None] + gather(i2, wy, img).abs() * magy[:, None])
            Sb = torch.maximum(Sb, scatter(i2, wx.abs() * magx + wy.abs() * magy, g.abs()))
    shape = lambda t: t.view(B, C, T, T) if t.shape[2] == TT else t.view(B, C, H, W)  # noqa: E731
    r.update(S=S, Sb=Sb)
    return {k: (shape(t) if k != "ntaps" else t) for k, t in r.items()}


def _tex_reference(c, gtex):
    """ATen float64: texture, mask, image gradient for gtex, and the same gradient for |gtex| (the weights are >= 0)."""
    grid, nzi, valid, _ = _tex_grid(c)
    img = c["img"].double().requires_grad_(True)
    tex = F.grid_sample(img, grid, mode="bilinear", padding_mode="zeros", align_corners=False)
    (gimg,) = torch.autograd.grad(tex, img, gtex, retain_graph=True)
    (gabs,) = torch.autograd.grad(tex, img, gtex.abs())
    assert (nzi[:, valid].abs() >= 1e-3).all(), "a valid texel's interpolated normal z is too close to the mask's threshold"
    mask = (valid[None] & (nzi < 0)).view(c["B"], 1, c["T"], c["T"])
    return tex.detach(), mask, gimg, gabs


def _tex_named_ok(c, ntaps):
    """The named texels of an exact row land where their names say (sample 0; the tap counts need H, W >= 2)."""
    assert c["exact"] and _tex_grid(c)[0].abs().max() <= 4
    where = {int(n): t for t, n in enumerate(c["tmap"].tolist()) if 0 <= n < len(TX_NAMED)}
    for n, (name, gx, gy, taps) in enumerate(TX_NAMED):
        got = _tex_grid(c)[0].view(c["B"], -1, 2)[0, where[n]]
        assert got[0].item() == gx and got[1].item() == gy, (name, got)
        if taps is not None and c["H"] >= 2 and c["W"] >= 2:
            assert int(ntaps[0, where[n]]) == taps, (name, int(ntaps[0, where[n]]), taps)


@pytest.mark.parametrize("row", TX_ROWS, ids=[r[0] for r in TX_ROWS])
def test_texture_map(row):
    from gif_amd.texture_space import _TextureMapFn
    name, T, (H, W), C, B, kind, exact = row
    c = _tex_case(name)
    valid = c["tmap"] >= 0
    gtexs = [("all", c["gtex"].double())]
    if not valid.all():  # the whole gradient is the pre-summed centre contribution of the invalid texels
        gtexs.append(("invalid_only", c["gtex"].double() * (~valid).view(1, 1, T, T)))
    img = c["img"].cuda().requires_grad_(True)
    dev = [c[k].cuda() for k in ("verts", "normals", "cam", "tmap", "tfaces", "tbc")]
    _poison(B * C * T * T)
    tex, mask = _TextureMapFn.apply(img, *dev, T)
    assert tex.shape == (B, C, T, T) and mask.shape == (B, 1, T, T) and mask.dtype == torch.bool
    for gi, (gname, gtex) in enumerate(gtexs):
        ref, mref, gref, gabs = _tex_reference(c, gtex)
        r = _tex_restated(c, gtex)
        if gi == 0:
            if exact:
                _tex_named_ok(c, r["ntaps"])
            assert mref.any() and not mref[:, :, valid.view(T, T)].all(), f"{name}: the mask has one value only"
            assert torch.equal(mask.cpu(), mref), f"{name}: {int((mask.cpu() != mref).sum())} mask texels differ"
            _check(tex, ref, r["R"], "texmap", name, extra=None if exact else r["S"])
            assert (tex.detach().cpu()[r["ntaps"].view(B, 1, T, T).expand(B, C, T, T) == 0] == 0).all()  # wholly outside: exactly 0
        _poison(B * C * H * W)
        (gimg,) = torch.autograd.grad(tex, img, gtex.float().cuda(), retain_graph=True)
        _check(gimg, gref, gabs, "texmap_bwd", f"{name} bwd {gname}", extra=None if exact else r["Sb"])
        if gname == "invalid_only":
            assert (gimg.cpu()[(gabs == 0)] == 0).all() and int((gabs != 0).sum()) <= 4 * B * C  # the centre taps only


# ---------------------------------------------------------------------------------------------------------------------------------
# c. vertex normals (csrc/mesh.hip: vertex_sum, vertex_normals_kernel; render._topology) through render.vertex_normals
# ---------------------------------------------------------------------------------------------------------------------------------
# vertex roles of every mesh (V >= 64)
VN_FAN, VN_FAN_N = 0, 13            # vertex 0: corner 0 of 13 faces around the ring 1 .. 13 (high valence, one branch only)
VN_TRI = 14                         # corner 0, 1 and 2 of three faces (with 15 .. 20): all three vertex_sum branches in one sum
VN_ONE = (21, 22, 23)               # one face only: valence 1 (as corner 0, 1 and 2 respectively)
VN_TINY = (24, 25, 26)              # one face with edges of 2^-12: |sum| = 2^-24 = 6e-8 < eps, not zero: the clamped branch
VN_NOFACE = (27, 28)                # no face, in the middle of the range: off[v] == off[v + 1]
VN_FIRST_FREE = 29                  # 29 .. V - 3: random faces; V - 2, V - 1: no face and beyond faces.max()

VN_ROWS = [
    # name, V, B, faces given as      (one thread per (b, v); 256 per workgroup)
    ("vn_v255", 255, 1, "FK"),      # B * V = 255: one workgroup, lane 255 idle (i >= B * V)
    ("vn_v256", 256, 1, "BFK"),     # B * V = 256: exactly one workgroup
    ("vn_v257", 257, 1, "FK"),      # B * V = 257: one live lane in workgroup 1
    ("vn_v85_b3", 85, 3, "BFK"),    # B * V = 255 with b = i / V in {0, 1, 2}
    ("vn_v86_b3", 86, 3, "FK"),     # B * V = 258: sample 2's last two vertices in workgroup 1
]


@functools.lru_cache(maxsize=None)
def _vn_case(name):
    _, V, B, _ = next(r for r in VN_ROWS if r[0] == name)
    g = _rng(60 + [r[0] for r in VN_ROWS].index(name))
    verts = torch.randn(B, V, 3, generator=g)
    a, b_, c_ = VN_TINY
    h = 2.0 ** -12
    verts[:, b_] = verts[:, a] + torch.tensor([h, 0.0, 0.0])
    verts[:, c_] = verts[:, a] + torch.tensor([0.0, h, 0.0])
    faces = [(VN_FAN, 1 + k, 1 + (k + 1) % VN_FAN_N) for k in range(VN_FAN_N)]
    t = VN_TRI
    faces += [(t, t + 1, t + 2), (t + 3, t, t + 4), (t + 5, t + 6, t)]
    faces += [VN_ONE, VN_TINY]
    lo, hi = VN_FIRST_FREE, V - 2  # random faces over [lo, hi), three distinct corners each, every vertex used
    pool = torch.arange(lo, hi)
    for _ in range(4):
        perm = pool[torch.randperm(hi - lo, generator=g)]
        perm = torch.cat([perm, perm[:(-len(perm)) % 3]])
        faces += [tuple(int(i) for i in f) for f in perm.view(-1, 3)]
    faces = torch.tensor(faces, dtype=torch.int64)
    assert all(len(set(f)) == 3 for f in faces.tolist()) and int(faces.max()) == V - 3
    return dict(V=V, B=B, verts=verts, faces=faces)


def _vn_restated(verts, faces):
    """fp64 restatement of the reference's vertex_normals over fp32 vertices [B,V,3]: (normals, R).  Three index_add_ passes
    (corner 1, 2, 0), x / max(|x|, eps).  R = sum_j |J_ij| Rx_j + |n_i| with J the Jacobian of x / max(|x|, eps) and Rx the same sum
    over the absolute terms of the cross products."""
    v = verts.double()
    vf = v[:, faces]  # [B,F,3,3]
    x, Rx = torch.zeros_like(v), torch.zeros_like(v)
    for corner, (p, q) in ((1, (2, 0)), (2, (0, 1)), (0, (1, 2))):
        ea, eb = vf[:, :, p] - vf[:, :, corner], vf[:, :, q] - vf[:, :, corner]
        x = x.index_add(1, faces[:, corner], torch.cross(ea, eb, dim=-1))
        ab = lambda i, j: (ea[..., i] * eb[..., j]).abs() + (ea[..., j] * eb[..., i]).abs()  # noqa: E731
        Rx = Rx.index_add(1, faces[:, corner], torch.stack([ab(1, 2), ab(2, 0), ab(0, 1)], -1))
    return (x, Rx) + _normalize_bound(x, Rx)


def _normalize_jacobian(x):
    """d (x / max(|x|, eps)) / d x, [..., 3, 3]"""
    ln = x.norm(dim=-1, keepdim=True)
    eye = torch.eye(3, dtype=torch.float64)
    n = x / ln.clamp_min(TINY)
    free = (eye - n[..., :, None] * n[..., None, :]) / ln.clamp_min(TINY)[..., None]
    return torch.where((ln >= EPS)[..., None], free, eye / EPS)


def _normalize_bound(x, Rx):
    n = x / x.norm(dim=-1, keepdim=True).clamp_min(EPS)
    return n, (_normalize_jacobian(x).abs() * Rx[..., None, :]).sum(-1) + n.abs()


def _vn_check(name, got, verts, faces, what):
    x, _, ref, R = _vn_restated(verts, faces)
    _check(got, ref, R, "normals", f"{name} {what}")
    count = torch.bincount(faces.reshape(-1), minlength=verts.shape[1])
    assert (got.cpu()[:, count == 0] == 0).all(), f"{name}: a vertex without a face must be exactly 0"
    return x, count


@pytest.mark.parametrize("row", VN_ROWS, ids=[r[0] for r in VN_ROWS])
def test_vertex_normals(row):
    from gif_amd import render
    name, V, B, layout = row
    c = _vn_case(name)
    faces = c["faces"]
    fdev = faces.cuda() if layout == "FK" else faces[None].repeat(B, 1, 1).cuda()
    vdev = c["verts"].cuda()
    _poison(B * V * 3)
    n1 = render.vertex_normals(vdev, fdev)
    x, count = _vn_check(name, n1, c["verts"], faces, layout)
    # the rows are what their comments say
    ln = x.norm(dim=-1)
    assert count[VN_FAN] == VN_FAN_N and count[VN_TRI] == 3 and all(count[i] == 1 for i in VN_ONE + VN_TINY)
    assert all(count[i] == 0 for i in VN_NOFACE + (V - 2, V - 1))
    assert ((ln[:, list(VN_TINY)] > 1e-8) & (ln[:, list(VN_TINY)] < 0.2 * EPS)).all()
    assert (ln[:, count > 0][:, 3:] > 0).all() and ((ln < 0.5 * EPS) | (ln > 2 * EPS)).all()  # nothing sits on the clamp's threshold
    # a second call returns the same bits (cached CSR); an in-place edit of faces must re-derive it (_topology's version check)
    n2 = render.vertex_normals(vdev, fdev)
    assert torch.equal(n1.view(torch.int32), n2.view(torch.int32))
    f2 = faces.clone()
    f2[0] = torch.tensor([VN_NOFACE[0], V - 1, VN_ONE[0]])  # vertex 27 and the last vertex gain a face, the fan loses one
    f2[VN_FAN_N + 1] = f2[VN_FAN_N + 1].flip(0)             # the face (17, 14, 18) is turned over
    if layout == "FK":
        fdev.copy_(f2)
    else:
        fdev[0].copy_(f2)  # (the topology of sample 0 is the batch's)
    n3 = render.vertex_normals(vdev, fdev)
    _vn_check(name, n3, c["verts"], f2, f"{layout} edited")
    assert not torch.equal(n1[:, V - 1], n3[:, V - 1])
