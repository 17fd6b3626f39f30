"""-m gpu: the mesh rasteriser and its backward (csrc/rasterize.hip: raster_bin, raster_tiles, raster_colors_bwd_band,
raster_colors_bwd_reduce) and the face gather (csrc/mesh.hip: face_gather_bwd_kernel) at the edges of their own index arithmetic.

The whole-mesh and random-triangle tests hit the common paths; here every row is a few faces written by hand and placed on one
predicate of the kernels.  Each row's comment names the predicate and the side the row sits on; `claim` restates that side as data
(tile count, per-tile list lengths, clipped box areas, band ranges, band pixel counts, covered pixels) and tests/test_cpu_wiring.py
(test_raster_edges_*) recomputes it on the CPU from a numpy restatement of front_facing / face_bbox / the tile and band arithmetic
(geometry, bands below) and from the C oracle alone.  The copies of the kernels' constants (K) are read back from rasterize.hip there.

A. Forward (FROWS; gif_rasterize_f32 / _colors_f32 / _f64 / _colors_f64 through gif_amd.standard_rasterize): bit equality with
   oracle.rasterize_oracle.standard_rasterize[_colors] on the same numpy arrays from the same caller buffers: tri equal, depth bits equal,
   payload bits equal, no tolerance.  Every row runs in all four variants.  The caller buffers are sentinels (tri -7, a finite payload
   pattern, a per-pixel depth pattern of 1e5 .. 1e5 + 4 unless the row seeds its own), so a pixel the kernel should not have written is
   caught.  The GPU runs twice on the same buffers (idempotent: a face ties with its own depth and wins again) and once on fresh ones:
   the list order inside a tile is not deterministic, so an order dependence would show as a difference between the calls.
   Inputs stay inside what the oracle and the kernel define alike: |x|, |y| < 2^31, no face with z of mixed sign or zero, no caller
   depth of -0.0 (checked on the CPU); every coordinate is exact in fp32, so the float32 and float64 variants read the same numbers.
   Refusals, no-ops and the workspace contract (cached, unregistered and 0xFF-filled, registration on and off) have tests of their own.
   A finding of the first run: bin_f255 failed in its colours variant.  No predicate of the kernels was wrong: ops._raster_workspace
   sized the cached workspace as bytes // 8 int64 words, and gif_rasterize_workspace_bytes is a multiple of 4 only (1028 for one tile
   and 255 faces), so the last list entry was written 4 bytes behind a 1024-byte allocation, into the face colours allocated next.
   Fixed there (rounded up); _cached_workspaces_are_whole states it for every workspace the rows leave in the cache.
B. Backward of the colour interpolation (BROWS; gif_rasterize_colors_bwd_f32 through ctypes as render.py calls it, per-face inputs
   [B, F, 3, 3], tri from the GPU forward and asserted equal to the oracle's, outputs and workspace pre-filled with NaN).
   Reference: bwd_ref, an fp64 restatement in torch on the CPU with autograd: the formula of bary_at (test_gpu_render_grad.interp_ref
   on per-face inputs) over the fp32 values widened to fp64, summed over the pixels tri assigns to each face.  Bound, per element, with
   no element excluded:

       |got - ref| <= TOL[family] * R + TINY
       colour: R = sum_pix |w_k| |g_ch|          vertex: R = sum_pix sum_k (sum_ch |g_ch| |c_k,ch|) |d w_k / d p_j|   (fp64 Jacobian)

   Condition on the faces: the fp32 chain through the dot products loses accuracy as 1 / sin^2 of the angle at p0 (conditioning, not
   indexing), so every face of these rows that wins a pixel has den / (dot00 dot11) >= 1/4 and every altitude >= 2 pixels (asserted on
   the CPU).  The one rounding-degenerate face (bw_degen) is held to exact statements instead.  The kernel is deterministic (no float
   atomics): two calls must agree in bits, and a null output must not change the bits of the other.
C. Face gather (GROWS; gif_face_gather_bwd_f32 through render._face_gather_bwd with render._topology): the face gradient holds small
   integers, every sum is exact: equality with an int64 scatter-add on the CPU, from an output left NaN in the allocator.

Observed on the MI355X (all rows of BROWS, one run; the kernel is deterministic) and the constants chosen from it: worst
|got - ref| / R over the family.
  family    worst (row)                 TOL              factor
  colour    2.44e-7 (bw_h192)           1.1e-6           4.5 x
  vertex    6.43e-7 (bw_n)              2.9e-6           4.5 x
Every case prints its ratios ("[raster ratio]" lines with -s), so a re-measurement is one run of this module."""
import collections
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# the kernels' constants (rasterize.hip); tests/test_cpu_wiring.py reads them back from the source
K = dict(kTile=64, kSmallArea=16, kBinThreads=256, kMaxLdsTiles=1024, kTileThreads=512, kBwdWaves=4, kBand=64)
TILE = K["kTile"]
NAN = float("nan")
INF = float("inf")
TINY = 1e-30
GIF_EINVAL = -1
VARIANTS = ("f32", "c32", "f64", "c64")  # plain / colours x float32 / float64

TOL = {"colour": 1.1e-6, "vertex": 2.9e-6}  # see the module docstring for the measurement behind them
WORST = {}


# ---------------------------------------------------------------------------------------------------------------------------------
# faces
# ---------------------------------------------------------------------------------------------------------------------------------
def rt(x, y, s, z=1.0):
    """Front-facing right triangle, right angle (p0) at (x, y), legs s along +y (p1) and +x (p2).  For integer x, y, s it covers the
    pixels (x + i, y + j), i, j >= 0, i + j < s: the two legs are inclusive, the hypotenuse (w[0] > 0) is not."""
    z0, z1, z2 = z if isinstance(z, tuple) else (z, z, z)
    return [[x, y, z0], [x, y + s, z1], [x + s, y, z2]]


def bx(x0, y0, bw, bh, z=1.0):
    """Front-facing right triangle whose bounding box is exactly the pixel columns x0 .. x0 + bw - 1 and rows y0 .. y0 + bh - 1
    (vertices 1/8 before the first and 1/4 behind the last pixel centre); it always covers (x0, y0)."""
    z0, z1, z2 = z if isinstance(z, tuple) else (z, z, z)
    return [[x0 - 0.125, y0 - 0.125, z0], [x0 - 0.125, y0 + bh - 0.75, z1], [x0 + bw - 0.75, y0 - 0.125, z2]]


def flip(face):
    """the other winding"""
    return [face[0], face[2], face[1]]


def cells(n, bw=2, bh=2, pitch=2, per_row=32, x0=0, y0=0):
    """n tiny faces, face i on its own grid cell with its own depth 1 + i / 1024"""
    return [bx(x0 + (i % per_row) * pitch, y0 + (i // per_row) * pitch, bw, bh, 1 + i / 1024) for i in range(n)]


Row = collections.namedtuple("Row", "name H W faces depth claim", defaults=(None, None))


# seeded caller depth buffers: functions of (row, typed face vertices, colours or None) -> depth [B, H, W] of the same dtype
def _first_pass(row, fv):
    """(tri, zp) of an oracle run from an all +inf depth buffer"""
    from oracle import rasterize_oracle as ro
    B = fv.shape[0]
    d = np.full((B, row.H, row.W), INF, fv.dtype)
    t = np.full((B, row.H, row.W), -1, np.int32)
    ro.standard_rasterize(fv, d, t, np.zeros((B, row.H, row.W, 3), fv.dtype), row.H, row.W)
    return t, d


SEED_SPLIT_X, SEED_TIE_Y = 14, 13


def seed_pos(row, fv):
    """+inf; on the face's pixels with x < SEED_SPLIT_X a nearer caller depth (the caller wins: tri and payload untouched); on its pixels
    of row SEED_TIE_Y with x >= SEED_SPLIT_X exactly the face's zp (the face wins the tie with the caller)"""
    t, zp = _first_pass(row, fv)
    d = np.full(t.shape, INF, fv.dtype)
    x = np.arange(row.W)[None, None, :]
    y = np.arange(row.H)[None, :, None]
    d[(t >= 0) & (x < SEED_SPLIT_X)] = 0.25
    tie = (t >= 0) & (x >= SEED_SPLIT_X) & (y == SEED_TIE_Y)
    d[tie] = zp[tie]
    return d


def seed_neg(row, fv):
    """negative caller depths: -2.25 on even columns (between the faces' depths -3 .. -1.5), -1 on odd columns (behind every face)"""
    d = np.full((fv.shape[0], row.H, row.W), -1.0, fv.dtype)
    d[:, :, 0::2] = -2.25
    return d


def _bin_tail(F):
    """F faces: 0 a large far face (when F > 1), 1 .. F - 2 tiny ones on rows >= 8, and the LAST one the only face that is nearest at (5, 5)"""
    faces = ([rt(0, 0, 40, 5.0)] if F > 1 else []) + cells(max(F - 2, 0), pitch=3, per_row=20, x0=2, y0=8)
    return [faces + [rt(4, 4, 3, 0.5)]]


def _ties(n):
    """n faces: three identical ones at indices 7, 2 and n - 1, tiny ones elsewhere (rows >= 24)"""
    faces = cells(n, per_row=30, x0=2, y0=24)
    for i in (7, 2, n - 1):
        faces[i] = rt(3, 3, 16, (2.0, 3.0, 5.0))
    return [faces]


DEGEN = [[0.0, 0.0, 1.0], [4096.0, 1.0, 2.0], [4096.0, 0.0, 3.0]]  # front-facing; its fp32 den rounds to 0: w = (1, 0, -0) on the whole box

FROWS = [
    # ---- A.1 raster_bin ---------------------------------------------------------------------------------------------------------
    # `fi < F` of the 256-lane workgroup: F = 1 / 255 (one workgroup, idle lanes), 256 (exactly one), 257 (lane 0 of workgroup 1 is the
    # only live one, and its face is the only one nearest at (5, 5): a dropped tail face changes the image)
    Row("bin_f1", 64, 64, _bin_tail(1), claim=dict(F=1, groups=1, tri={(0, 5, 5): 0})),
    Row("bin_f255", 64, 64, _bin_tail(255), claim=dict(F=255, groups=1, tri={(0, 5, 5): 254})),
    Row("bin_f256", 64, 64, _bin_tail(256), claim=dict(F=256, groups=1, tri={(0, 5, 5): 255})),
    Row("bin_f257", 64, 64, _bin_tail(257), claim=dict(F=257, groups=2, tri={(0, 5, 5): 256})),
    # `tx1 = x_max >> 6`: a box that ends at x = 63.0 exactly is listed in tile 0 alone, one that ends at 64.0 in tiles 0 and 1
    Row("tile_x63", 64, 128, [[[[58, 10, 1], [58, 16, 1], [63.0, 10, 1]]]], claim=dict(nt=2, lists={(0, 0): 1, (0, 1): 0})),
    Row("tile_x64", 64, 128, [[[[58, 10, 1], [58, 16, 1], [64.0, 10, 1]]]], claim=dict(nt=2, lists={(0, 0): 1, (0, 1): 1})),
    # `ty1 = y_max >> 6`: the same pair in y
    Row("tile_y63", 128, 64, [[[[10, 58, 1], [10, 63.0, 1], [16, 58, 1]]]], claim=dict(nt=2, lists={(0, 0): 1, (0, 1): 0})),
    Row("tile_y64", 128, 64, [[[[10, 58, 1], [10, 64.0, 1], [16, 58, 1]]]], claim=dict(nt=2, lists={(0, 0): 1, (0, 1): 1})),
    # inside(): `w[2] >= 0 && w[1] >= 0 && w[0] > 0` on integer vertices: two inclusive edges, one exclusive: 36 pixels, x and y in
    # 60 .. 67, across the 63 | 64 seam of four tiles
    Row("incl_int", 128, 128, [[rt(60, 60, 8, (1.0, 2.0, 3.0))]], claim=dict(nt=4, lists={(0, t): 1 for t in range(4)}, cover=36)),
    # `if (front_facing(f))` false: the other winding of the same triangle is never listed
    Row("none_back", 128, 128, [[flip(rt(60, 60, 8))]], claim=dict(lists={(0, t): 0 for t in range(4)}, cover=0)),
    # front_facing of an exactly collinear face (a repeated vertex): 0 < 0 is false
    Row("none_collinear", 64, 64, [[[[10, 10, 1], [10, 10, 1], [30, 20, 1]]]], claim=dict(lists={(0, 0): 0}, cover=0)),
    # `x_min <= x_max && y_min <= y_max` false: front-facing, strictly between pixel centres (ceil(min) > floor(max))
    Row("none_empty_box", 64, 64, [[[[10.25, 10.25, 1], [10.25, 10.75, 1], [10.75, 10.25, 1]]]], claim=dict(lists={(0, 0): 0}, cover=0)),
    # the same predicate through the clamps: one face wholly beyond each of the four borders (x_max < 0, x_min > W - 1, likewise y)
    Row("none_offscreen", 64, 64, [[rt(-30, 10, 8), rt(70, 10, 8), rt(10, -30, 8), rt(10, 70, 8)]], claim=dict(lists={(0, 0): 0}, cover=0)),
    # face_bbox's clamps to 0, W - 1, H - 1: faces that hang over every border, negative coordinates and coordinates >= W, >= H
    Row("clamp_borders", 64, 64, [[rt(-5, -5, 12, 1.0), rt(58, 20, 12, 2.0), rt(20, 58, 12, 3.0), rt(60, 60, 10, 4.0), rt(-6, 30, 10, 5.0),
                                   rt(30, -6, 10, 6.0)]],
        claim=dict(lists={(0, 0): 6}, tri={(0, 0, 0): 0, (0, 20, 63): 1, (0, 63, 20): 2, (0, 63, 63): 3, (0, 30, 0): 4, (0, 0, 30): 5})),
    # the tx / ty loops over more than one tile: one face over all 3 x 3 tiles of a 192 x 192 image, a small nearer one in the middle tile
    Row("large_3x3", 192, 192, [[rt(-10, -10, 420, (7.0, 8.0, 9.0)), bx(100, 100, 5, 5, 1.0)]],
        claim=dict(nt=9, lists={**{(0, t): 1 for t in range(9)}, (0, 4): 2}, cover=192 * 192)),
    # `base[t] = atomicAdd(cb + t, c)`: 600 faces in tile 0: three bin workgroups add to one counter, their offsets must not overlap
    Row("list_600", 64, 128, [cells(600) + [bx(70, 5, 3, 3, 1.0), bx(90, 40, 5, 5, 2.0)]], claim=dict(groups=3, lists={(0, 0): 600, (0, 1): 2})),
    # `lds = nt <= kMaxLdsTiles` true at exactly 1024 tiles: counting stays in LDS.  One face reaches the last column, one is 60 wide
    Row("nt1024", 2, 65536, [[rt(65530, 0, 8, 1.0), [[10, -1, 2], [10, 3, 2], [69.5, -1, 2]]]],
        claim=dict(nt=1024, lists={(0, 1023): 1, (0, 0): 1, (0, 1): 1, (0, 2): 0}, tri={(0, 0, 65535): 0, (0, 1, 20): 1})),
    # the same predicate false at 1025 tiles: every entry is one global atomic.  B = 2: the per-image offsets of count and list with nt
    # odd (pad2 rounds the counters up to 2050 words)
    Row("nt1025", 2, 65537, [[rt(65530, 0, 8, 1.0), [[10, -1, 2], [10, 3, 2], [69.5, -1, 2]]],
                             [[[200, -1, 2], [200, 3, 2], [259.5, -1, 2]], rt(65531, 0, 8, 1.0)]],
        claim=dict(nt=1025, lists={(0, 1024): 1, (0, 1023): 1, (0, 0): 1, (0, 1): 1, (1, 3): 1, (1, 4): 1, (1, 0): 0, (1, 1024): 1},
                   tri={(0, 0, 65536): 0, (0, 1, 20): 1, (1, 0, 65536): 1, (1, 1, 210): 0})),
    # ---- A.2 raster_tiles -------------------------------------------------------------------------------------------------------
    # `area <= kSmallArea` true at exactly 16 pixels (the lane walks the box), in the four shapes of 16
    Row("cls_4x4", 64, 64, [[bx(20, 20, 4, 4)]], claim=dict(areas={(0, 0): 16})),
    Row("cls_2x8", 64, 64, [[bx(20, 20, 2, 8)]], claim=dict(areas={(0, 0): 16})),
    Row("cls_1x16", 64, 64, [[bx(20, 20, 1, 16)]], claim=dict(areas={(0, 0): 16})),
    Row("cls_16x1", 64, 64, [[bx(20, 20, 16, 1)]], claim=dict(areas={(0, 0): 16})),
    # the same predicate false at 17 and 18 pixels (`__ballot(area > kSmallArea)`: the wave walks the box)
    Row("cls_1x17", 64, 64, [[bx(20, 20, 1, 17)]], claim=dict(areas={(0, 0): 17})),
    Row("cls_2x9", 64, 64, [[bx(20, 20, 2, 9)]], claim=dict(areas={(0, 0): 18})),
    # the class follows the box CLIPPED to the tile (x_min = max(x_min, tx0) ...): a 10 x 10 box is wave class in tile 0 (8 x 8), lane
    # class with exactly 16 pixels in tiles 1 and 2 (2 x 8, 8 x 2) and lane class in tile 3, which it overlaps by 2 x 2 pixels only
    # (a vertex at (65.25, 65.25): it covers (64, 64) and (65, 65) there)
    Row("cls_clipped", 128, 128, [[[[55.875, 60, 1], [65.25, 65.25, 2], [60, 55.875, 3]]]],
        claim=dict(areas={(0, 0): 64, (0, 1): 16, (0, 2): 16, (0, 3): 4}, tri={(0, 64, 64): 0, (0, 65, 65): 0, (0, 60, 60): 0})),
    # the wave walk `for (y0 ..; y0 += 8) for (x0 ..; x0 += 8)`, `x <= gx1 && y <= gy1`: one step exactly, a partial second step in
    # both axes, the whole tile (64 steps), one row of 8 steps with 7 of 8 lane rows idle
    Row("walk_8x8", 64, 64, [[bx(20, 20, 8, 8)]], claim=dict(areas={(0, 0): 64})),
    Row("walk_9x9", 64, 64, [[bx(20, 20, 9, 9)]], claim=dict(areas={(0, 0): 81})),
    Row("walk_64x64", 64, 64, [[bx(0, 0, 64, 64, (1.0, 2.0, 3.0))]], claim=dict(areas={(0, 0): 4096})),
    Row("walk_64x1", 64, 64, [[bx(0, 31, 64, 1)]], claim=dict(areas={(0, 0): 64})),
    # `for (j0 = 0; j0 < n; j0 += kTileThreads)`: 511 (one round, lane 63 of wave 7 idle), 512 (exactly one), 513 (entry 512 alone in a
    # second round: the cand[j] path), 1025 (a third round).  Tile 1 holds 3 faces.  F >= 512 here: `j_first < F` is true for every lane;
    # every row with F < 512 (all the others) is on its false side for the lanes beyond F.
    Row("list_511", 64, 128, [cells(511) + cells(3, x0=70, y0=9, pitch=5)], claim=dict(lists={(0, 0): 511, (0, 1): 3})),
    Row("list_512", 64, 128, [cells(512) + cells(3, x0=70, y0=9, pitch=5)], claim=dict(lists={(0, 0): 512, (0, 1): 3})),
    Row("list_513", 64, 128, [cells(513) + cells(3, x0=70, y0=9, pitch=5)], claim=dict(lists={(0, 0): 513, (0, 1): 3})),
    # (64 x 64 / 4 = 1024 cells: face 1024 sits across four cells, nearer than all)
    Row("list_1025", 64, 128, [cells(1024) + [bx(31, 31, 2, 2, 0.5)] + cells(3, x0=70, y0=9, pitch=5)], claim=dict(lists={(0, 0): 1025, (0, 1): 3})),
    # the same 513 with 5 x 5 boxes: all wave class, so the ballot of round 0 has bit 63 set (lane 63 of wave 0 holds entry 504) and
    # `__ffsll` / `todo &= todo - 1` run over all 64 bits
    Row("list_513_wave", 64, 64, [cells(513, bw=5, bh=5, per_row=30)], claim=dict(lists={(0, 0): 513}, areas={(504, 0): 25, (512, 0): 25})),
    # partial tiles: `tx1 = min(tx0 + kTile, W) - 1`, `x <= tx1 && y <= ty1` in seed and resolve.  A far face over everything, a nearer
    # one over the last row and column
    Row("part_1x1", 1, 1, [[rt(-3, -3, 40, 9.0), rt(-2, -2, 10, (1.0, 2.0, 3.0))]], claim=dict(nt=1, cover=1, tri={(0, 0, 0): 1})),
    Row("part_63x65", 63, 65, [[rt(-3, -3, 400, 9.0), rt(61, 59, 10, (1.0, 2.0, 3.0))]],  # the last tile is one column wide
        claim=dict(nt=2, cover=63 * 65, tri={(0, 62, 64): 1}, areas={(1, 1): 4})),
    Row("part_65x63", 65, 63, [[rt(-3, -3, 400, 9.0), rt(59, 61, 10, (1.0, 2.0, 3.0))]],  # the last tile is one row high
        claim=dict(nt=2, cover=63 * 65, tri={(0, 64, 62): 1}, areas={(1, 1): 4})),
    Row("part_64x128", 64, 128, [[rt(-3, -3, 400, 9.0), rt(124, 60, 10, (1.0, 2.0, 3.0))]], claim=dict(nt=2, cover=64 * 128, tri={(0, 63, 127): 1})),
    # `n_sh = count[blockIdx.x]` = 0: 2 x 2 tiles, faces in three of them: tile 3 keeps the sentinels exactly
    Row("empty_tile", 128, 128, [[bx(10, 10, 9, 9, 1.0), bx(80, 20, 4, 4, 2.0), bx(20, 90, 20, 3, 3.0)]],
        claim=dict(nt=4, lists={(0, 0): 1, (0, 1): 1, (0, 2): 1, (0, 3): 0})),
    # the seed `key[p] = ordered_bits(depth_in[p]) << 32 | kNoFace`, positive depths: a nearer caller keeps its pixel, an equal one
    # loses it to the face (fidx < kNoFace in the low word), +inf elsewhere
    Row("seed_pos", 64, 64, [[rt(10, 10, 12, (1.0, 2.0, 3.0))]], depth=seed_pos, claim=dict(seed="pos")),
    # the `u & 0x80000000` branch of ordered_bits: all-negative z, against the far sentinel and against negative caller depths
    Row("neg_z", 64, 64, [[rt(20, 20, 8, (-2.0, -2.0, -3.0)), rt(20, 20, 8, (-3.0, -1.5, -2.0))]], claim=dict(split=True)),
    Row("seed_neg", 64, 64, [[rt(20, 20, 8, (-2.0, -2.0, -3.0)), rt(20, 20, 8, (-3.0, -1.5, -2.0))]], depth=seed_neg, claim=dict(seed="neg")),
    # `if (zp == zp)`: a face with a NaN z in front (lower index) of a finite one never wins and no NaN is written
    Row("nan_z", 64, 64, [[rt(10, 10, 16, (NAN, 1.0, 1.0)), rt(10, 10, 16, (2.0, 3.0, 4.0))]], claim=dict(cover=136, only_face=1)),
    # the face index in the low word of the key (float32) and the fkey pass (float64): three identical faces at 7, 2, 300 of 301: the
    # lowest index wins every pixel
    Row("tie_3of301", 64, 64, _ties(301), claim=dict(F=301, tie_winner=2, tie_losers=(7, 300))),
    # two different coplanar faces (constant z = 2, integer vertices: every zp is exactly 2) that share their hypotenuse, inclusive in
    # both: the shared pixels go to the lower index
    Row("tie_coplanar", 64, 64, [[[[20, 28, 2], [28, 20, 2], [20, 20, 2]], [[28, 20, 2], [20, 28, 2], [28, 28, 2]]]], claim=dict(shared=7)),
    # `c.inv = (den == 0) ? 0 : 1 / den`: front-facing but den rounds to 0 in fp32: w = (1, 0, -0), the face fills its whole clamped
    # box (400 pixels, rows 0 and 1); in float64 it is a proper sliver (200 pixels, row 0).  Each against its own oracle, -0.0 included
    Row("degen_round", 4, 200, [[DEGEN]], claim=dict(cover={"f32": 400, "f64": 200})),
    # `b = blockIdx.x / nt` and the b offsets of fv, count, list and the image: three images with different faces; image 1 has all
    # faces back-facing (its tiles' lists are empty)
    Row("batch3", 64, 128, [[bx(5, 5, 9, 9, 1.0), bx(70, 5, 3, 3, 2.0), rt(60, 30, 8, 3.0)],
                            [flip(bx(5, 5, 9, 9, 1.0)), flip(bx(70, 5, 3, 3, 2.0)), flip(rt(60, 30, 8, 3.0))],
                            [rt(100, 40, 20, 1.0), bx(60, 60, 8, 4, 2.0), bx(0, 0, 1, 1, 3.0)]],
        claim=dict(lists={(0, 0): 2, (0, 1): 2, (1, 0): 0, (1, 1): 0, (2, 0): 2, (2, 1): 2})),
]
FROW = {r.name: r for r in FROWS}


def face_array(faces, dtype=np.float64):
    """[B][F] lists of 3 x (x, y, z) -> [B, F, 3, 3]"""
    return np.ascontiguousarray(np.array(faces, dtype=np.float64).astype(dtype))


def colours(fv):
    """per-vertex colours that are not symmetric in the three vertices (dyadic: exact in both types)"""
    idx = np.arange(fv.size, dtype=np.int64).reshape(fv.shape)
    k = np.arange(3)[None, None, :, None]
    return np.ascontiguousarray((0.125 + (idx * 37 % 64) / 64.0 + 0.5 * k * k).astype(fv.dtype))


def caller_buffers(row, fv):
    """sentinel caller buffers (numpy): depth, tri, payload"""
    B, H, W = fv.shape[0], row.H, row.W
    if row.depth is None:
        depth = (1e5 + np.arange(B * H * W, dtype=np.int64) % 5).reshape(B, H, W).astype(fv.dtype)
    else:
        depth = row.depth(row, fv)
    tri = np.full((B, H, W), -7, np.int32)
    pay = (-3.0 - (np.arange(B * H * W * 3, dtype=np.int64) % 13) * 0.125).reshape(B, H, W, 3).astype(fv.dtype)
    return depth, tri, pay


def oracle_run(row, fv, fc, bufs):
    """the C oracle on copies of the caller buffers"""
    from oracle import rasterize_oracle as ro
    d, t, p = (a.copy() for a in bufs)
    if fc is None:
        ro.standard_rasterize(fv, d, t, p, row.H, row.W)
    else:
        ro.standard_rasterize_colors(fv, fc, d, t, p, row.H, row.W)
    return d, t, p


@functools.lru_cache(maxsize=None)
def forward_case(name, variant):
    """(fv, fc or None, caller buffers, oracle result) of one row in one variant; nothing in it is modified afterwards"""
    row = FROW[name]
    fv = face_array(row.faces, np.float64 if variant.endswith("64") else np.float32)
    fc = colours(fv) if variant[0] == "c" else None
    bufs = caller_buffers(row, fv)
    return fv, fc, bufs, oracle_run(row, fv, fc, bufs)


def geometry(fv, H, W):
    """numpy restatement of front_facing, face_bbox and raster_bin's tile arithmetic in fv's own dtype: dict(listed [B, F], box [B, F, 4]
    (x_min, x_max, y_min, y_max), tiles_x, tiles_y, nt, lists [B, nt], area(b, f, t): the face's box clipped to tile t)"""
    x, y = fv[..., 0], fv[..., 1]
    front = (y[..., 2] - y[..., 0]) * (x[..., 1] - x[..., 0]) < (y[..., 1] - y[..., 0]) * (x[..., 2] - x[..., 0])
    box = np.stack([np.maximum(np.ceil(x.min(-1)).astype(np.int64), 0), np.minimum(np.floor(x.max(-1)).astype(np.int64), W - 1),
                    np.maximum(np.ceil(y.min(-1)).astype(np.int64), 0), np.minimum(np.floor(y.max(-1)).astype(np.int64), H - 1)], -1)
    listed = front & (box[..., 0] <= box[..., 1]) & (box[..., 2] <= box[..., 3])
    tiles_x, tiles_y = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    nt = tiles_x * tiles_y
    lists = np.zeros((fv.shape[0], nt), np.int64)
    for b, f in zip(*np.nonzero(listed)):
        x0, x1, y0, y1 = box[b, f]
        for ty in range(y0 >> 6, (y1 >> 6) + 1):
            lists[b, ty * tiles_x + (x0 >> 6):ty * tiles_x + (x1 >> 6) + 1] += 1

    def area(b, f, t):
        if not listed[b, f]:
            return 0
        tx0, ty0 = (t % tiles_x) * TILE, (t // tiles_x) * TILE
        x0, x1 = max(box[b, f, 0], tx0), min(box[b, f, 1], min(tx0 + TILE, W) - 1)
        y0, y1 = max(box[b, f, 2], ty0), min(box[b, f, 3], min(ty0 + TILE, H) - 1)
        return int((x1 - x0 + 1) * (y1 - y0 + 1)) if x1 >= x0 and y1 >= y0 else 0

    return dict(listed=listed, box=box, tiles_x=tiles_x, tiles_y=tiles_y, nt=nt, lists=lists, area=area)


def _same_bits(a, b):
    ints = {4: np.int32, 8: np.int64}[a.dtype.itemsize]
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(ints), b.view(ints))


def _assert_equal(what, got, ref):
    for name, g, r in zip(("depth", "tri", "payload"), got, ref):
        if not _same_bits(g, r):
            ints = {4: np.int32, 8: np.int64}[g.dtype.itemsize]
            bad = np.argwhere(g.view(ints) != r.view(ints))
            i = tuple(int(v) for v in bad[0])
            raise AssertionError(f"{what}: {name} differs from the oracle in {len(bad)} elements; first at {i}: got {g[i]!r} ref {r[i]!r}")


def _gpu_forward(row, fv, fc, bufs, calls=1):
    """standard_rasterize[_colors] on device copies of the caller buffers, `calls` times on the same buffers -> numpy results"""
    from gif_amd import standard_rasterize as sr
    dev = [torch.from_numpy(a.copy()).cuda() for a in bufs]
    fvd = torch.from_numpy(fv).cuda()
    fcd = None if fc is None else torch.from_numpy(fc).cuda()
    for _ in range(calls):
        if fc is None:
            out = sr.standard_rasterize(fvd, dev[0], dev[1], dev[2], row.H, row.W)
        else:
            out = sr.standard_rasterize_colors(fvd, fcd, dev[0], dev[1], dev[2], row.H, row.W)
        assert all(o is d for o, d in zip(out, dev))  # in place, returned
    return [d.cpu().numpy() for d in dev]


def _cached_workspaces_are_whole():
    """every workspace ops.rasterize keeps holds all of gif_rasterize_workspace_bytes (a multiple of 4, not of 8: bin_f255 needs 1028)"""
    from gif_amd import _lib, ops
    lib = _lib.load()
    assert ops._raster_ws
    for (_, _, B, F, h, w), ws in ops._raster_ws.items():
        need = lib.gif_rasterize_workspace_bytes(B, F, h, w)
        assert ws.numel() * ws.element_size() >= need, f"cached workspace of {(B, F, h, w)}: {ws.numel() * ws.element_size()} bytes < {need}"


@pytest.mark.parametrize("row", FROWS, ids=[r.name for r in FROWS])
def test_forward(row):
    for variant in VARIANTS:
        fv, fc, bufs, ref = forward_case(row.name, variant)
        once = _gpu_forward(row, fv, fc, bufs)
        _assert_equal(f"{row.name} {variant}", once, ref)
        twice = _gpu_forward(row, fv, fc, bufs, calls=2)  # fresh buffers again, two calls on them
        _assert_equal(f"{row.name} {variant} second call on the same buffers", twice, ref)
    _cached_workspaces_are_whole()


# ---------------------------------------------------------------------------------------------------------------------------------
# A.3 refusals and no-ops, A.4 the workspace contract
# ---------------------------------------------------------------------------------------------------------------------------------
def _stream():
    return torch.cuda.current_stream().cuda_stream


def _abi_forward(lib, fv, fc, dev, H, W, ws_ptr, B=None, F=None):
    """straight through the C ABI on device tensors dev = (depth, tri, payload)"""
    B = fv.shape[0] if B is None else B
    F = fv.shape[1] if F is None else F
    f64 = fv.dtype == torch.float64
    if fc is None:
        fn = lib.gif_rasterize_f64 if f64 else lib.gif_rasterize_f32
        rc = fn(fv.data_ptr(), dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), B, F, H, W, ws_ptr, _stream())
    else:
        fn = lib.gif_rasterize_colors_f64 if f64 else lib.gif_rasterize_colors_f32
        rc = fn(fv.data_ptr(), fc.data_ptr(), dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), B, F, H, W, ws_ptr, _stream())
    torch.cuda.synchronize()
    return rc


def test_wrapper_refusals():
    from gif_amd import _lib
    from gif_amd import standard_rasterize as sr
    row = FROW["cls_4x4"]
    fv, fc, bufs, _ = forward_case(row.name, "c32")
    fvd, fcd = torch.from_numpy(fv).cuda(), torch.from_numpy(fc).cuda()
    d, t, p = (torch.from_numpy(a.copy()).cuda() for a in bufs)
    wide = torch.zeros(1, 64, 128, device="cuda")
    with pytest.raises(RuntimeError, match="contiguous"):  # a non-contiguous tensor
        sr.standard_rasterize(fvd, wide[:, :, ::2], t, p, 64, 64)
    with pytest.raises(_lib.GifHipError, match="depth_buffer must be"):  # a wrong dtype
        sr.standard_rasterize(fvd, d.double(), t, p, 64, 64)
    with pytest.raises(_lib.GifHipError, match="triangle_buffer must be"):
        sr.standard_rasterize(fvd, d, t.long(), p, 64, 64)
    with pytest.raises(_lib.GifHipError, match="float32 or float64"):
        sr.standard_rasterize(fvd.half(), d, t, p, 64, 64)
    with pytest.raises(_lib.GifHipError, match="shape of face_vertices"):  # a colour shape mismatch
        sr.standard_rasterize_colors(fvd, torch.cat([fcd, fcd], 1), d, t, p, 64, 64)
    for got, ref in zip((d, t, p), bufs):  # nothing was launched
        assert _same_bits(got.cpu().numpy(), ref)


def test_abi_refusals_and_noops():
    from gif_amd import _lib
    lib = _lib.load()
    row = FROW["cls_4x4"]
    fv, fc, bufs, _ = forward_case(row.name, "c32")
    fvd, fcd = torch.from_numpy(fv).cuda(), torch.from_numpy(fc).cuda()
    dev = [torch.from_numpy(a.copy()).cuda() for a in bufs]
    ws = torch.zeros(64, dtype=torch.int64, device="cuda")

    def err():
        return lib.gif_last_error().decode()

    assert _abi_forward(lib, fvd, None, dev, 64, 64, ws.data_ptr() + 4) == GIF_EINVAL and "workspace" in err()  # `workspace & 7`
    assert _abi_forward(lib, fvd, fcd, dev, 64, 64, ws.data_ptr() + 4) == GIF_EINVAL and "workspace" in err()
    assert _abi_forward(lib, fvd, None, dev, 0, 64, ws.data_ptr()) == GIF_EINVAL and "H=0" in err()               # `H > 0`
    assert _abi_forward(lib, fvd, None, dev, 64, 64, ws.data_ptr(), B=65536) == GIF_EINVAL and "images" in err()  # `B <= 65535`
    assert _abi_forward(lib, fvd, None, dev, 64, 64, ws.data_ptr(), F=0) == 0                                     # `F == 0`
    assert _abi_forward(lib, fvd, fcd, dev, 64, 64, ws.data_ptr(), F=0) == 0
    assert _abi_forward(lib, fvd, None, dev, 64, 64, ws.data_ptr(), B=0) == 0                                     # `B * H * W == 0`
    assert _abi_forward(lib, fvd, fcd, dev, 64, 64, ws.data_ptr(), B=0) == 0
    for got, ref in zip(dev, bufs):  # refused or a no-op: the buffers are exactly as they were
        assert _same_bits(got.cpu().numpy(), ref)
    assert not ws.any()


# two face sets of one (B, F, H, W) = (1, 3, 128, 128): X fills tiles 0, 1 and 2 (lists 2, 1, 1), Y tiles 1 and 3 (lists 1, 3):
# other lengths, and tiles 0 and 2 are empty under Y
WS_X = Row("ws_x", 128, 128, [[bx(5, 5, 9, 9, 1.0), bx(60, 20, 8, 8, 2.0), bx(20, 90, 6, 6, 3.0)]], claim=dict(lists={(0, 0): 2, (0, 1): 1, (0, 2): 1, (0, 3): 0}))
WS_Y = Row("ws_y", 128, 128, [[bx(70, 80, 9, 9, 1.0), bx(100, 60, 8, 8, 2.0), bx(90, 100, 20, 3, 3.0)]], claim=dict(lists={(0, 0): 0, (0, 1): 1, (0, 2): 0, (0, 3): 3}))
WS_600 = Row("ws_600", 64, 128, FROW["list_600"].faces, claim=dict(lists={(0, 0): 600, (0, 1): 2}))
WS_ROWS = [WS_X, WS_Y, WS_600]


def _ws_case(row, variant="f32"):
    fv = face_array(row.faces, np.float64 if variant.endswith("64") else np.float32)
    fc = colours(fv) if variant[0] == "c" else None
    bufs = caller_buffers(row, fv)
    return fv, fc, bufs, oracle_run(row, fv, fc, bufs)


def test_cached_workspace_hands_its_counters_back_zero():
    """through ops.rasterize, which caches and registers the workspace: X, then Y with the same (B, F, H, W); a counter that was not
    handed back zero would lengthen one of Y's lists with X's stale entries or shift its offsets"""
    for variant in VARIANTS:
        for row in (WS_X, WS_Y, WS_X, WS_Y):
            fv, fc, bufs, ref = _ws_case(row, variant)
            _assert_equal(f"{row.name} {variant} (cached workspace)", _gpu_forward(row, fv, fc, bufs), ref)


@pytest.mark.parametrize("row", [WS_X, WS_600], ids=["f3", "f600"])
def test_unregistered_workspace_needs_no_initialisation(row):
    """a workspace of the test's own, exactly gif_rasterize_workspace_bytes long, every byte 0xFF, never registered: the library's memset
    of the counters and the pre_idx clamp (`min(cand[j_first], F - 1)` of a stale entry 0xFFFFFFFF) must make it equal to the oracle, and
    the sentinel words before and behind it must stay"""
    from gif_amd import _lib
    lib = _lib.load()
    GUARD = 64  # words
    for variant in ("f32", "c64"):
        fv, fc, bufs, ref = _ws_case(row, variant)
        B, F = fv.shape[:2]
        nbytes = lib.gif_rasterize_workspace_bytes(B, F, row.H, row.W)
        nt = geometry(fv, row.H, row.W)["nt"]
        assert nbytes == 4 * ((B * nt + 1) // 2 * 2 + B * nt * F)
        words = nbytes // 4
        block = torch.full((words + 2 * GUARD,), -1, dtype=torch.int32, device="cuda")  # 0xFF bytes
        block[:GUARD] = 0x5A5A5A5A
        block[GUARD + words:] = 0x5A5A5A5A
        ws_ptr = block.data_ptr() + 4 * GUARD
        assert ws_ptr % 8 == 0
        dev = [torch.from_numpy(a.copy()).cuda() for a in bufs]
        fvd = torch.from_numpy(fv).cuda()
        fcd = None if fc is None else torch.from_numpy(fc).cuda()
        for call in range(2):
            block[GUARD:GUARD + words] = -1
            assert _abi_forward(lib, fvd, fcd, dev, row.H, row.W, ws_ptr) == 0
            _assert_equal(f"{row.name} {variant} (0xFF workspace, call {call})", [d.cpu().numpy() for d in dev], ref)
            assert (block[:GUARD] == 0x5A5A5A5A).all() and (block[GUARD + words:] == 0x5A5A5A5A).all()
            assert not block[GUARD:GUARD + B * nt].any()  # the counters come back zero


def test_workspace_registration_on_and_off():
    from gif_amd import _lib
    lib = _lib.load()
    fvx, _, bufx, refx = _ws_case(WS_X)
    fvy, _, bufy, refy = _ws_case(WS_Y)
    nbytes = lib.gif_rasterize_workspace_bytes(1, 3, 128, 128)
    ws = torch.zeros(nbytes // 8 + 1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()

    def run(fv, bufs):
        dev = [torch.from_numpy(a.copy()).cuda() for a in bufs]
        assert _abi_forward(lib, torch.from_numpy(fv).cuda(), None, dev, 128, 128, ws.data_ptr()) == 0
        return [d.cpu().numpy() for d in dev]

    assert lib.gif_rasterize_assume_clean_workspace(ws.data_ptr(), 1) == 0
    try:
        _assert_equal("registered, X", run(fvx, bufx), refx)
        _assert_equal("registered, Y", run(fvy, bufy), refy)
    finally:
        assert lib.gif_rasterize_assume_clean_workspace(ws.data_ptr(), 0) == 0
    ws.view(torch.uint8).fill_(0xFF)
    _assert_equal("unregistered again, 0xFF, X", run(fvx, bufx), refx)
    assert lib.gif_rasterize_assume_clean_workspace(None, 1) == GIF_EINVAL


# ---------------------------------------------------------------------------------------------------------------------------------
# B. backward of the colour interpolation
# ---------------------------------------------------------------------------------------------------------------------------------
def wt(x, y, a, b, z=1.0):
    """Well-shaped front-facing triangle: p0 = (x, y), p1 = p0 + (b / 4, b), p2 = p0 + (a, a / 8): sin^2 of the angle at p0 is 0.87"""
    return [[x, y, z], [x + 0.25 * b, y + b, z], [x + a, y + 0.125 * a, z]]


BRow = collections.namedtuple("BRow", "name H W faces claim")


def _bw_tail(F):
    """F faces on their own cells of a 32 x 32 image; each wins pixels, the last included"""
    return [[wt(1.3 + 10 * (i % 3), 1.2 + 10 * (i // 3), 7.5, 7.0, 1 + i / 8) for i in range(F)]]


# claims: bands {face: (b0, b1)} of image 0 (b1 < b0: the face shades nothing); n {(face, band): pixels of the band's part of the box};
# wins {face: True / False}: whether the face owns a pixel of the oracle's tri
BROWS = [
    # `if (fi >= F) return` of the 4-wave workgroup: F = 1 (three waves leave), 4 (none), 5 (workgroup 1 keeps one), 7
    BRow("bw_f1", 32, 32, _bw_tail(1), dict(wins={0: True})),
    BRow("bw_f4", 32, 32, _bw_tail(4), dict(wins={3: True})),
    BRow("bw_f5", 32, 32, _bw_tail(5), dict(wins={4: True})),
    BRow("bw_f7", 32, 32, _bw_tail(7), dict(wins={6: True})),
    # bands = (H + 63) / 64 = 1: `band < b0 || band > b1` never true; face 1 is clamped at the top border (y < 0), face 2 at the bottom
    BRow("bw_h64", 64, 32, [[wt(2.3, 3.2, 20.0, 40.0, 2.0), wt(4.3, -6.8, 18.0, 20.0, 1.0), wt(6.3, 50.2, 20.0, 30.0, 1.0)]],
         dict(bands={0: (0, 0), 1: (0, 0), 2: (0, 0)}, wins={0: True, 1: True, 2: True})),
    # two bands, the second one row: face 0 has the box rows 63 .. 64 (r1 = min(y_max, 63) in band 0, r0 = max(y_min, 64) in band 1),
    # face 1 stays in band 0, face 2 is clamped at the bottom border: its part of band 1 is the single row 64
    BRow("bw_h65", 65, 48, [[[[3.3, 62.125, 1], [5.3, 64.875, 1], [30.3, 62.25, 1]], wt(2.3, 3.2, 20.0, 40.0, 2.0), wt(20.3, 40.2, 20.0, 40.0, 3.0)]],
         dict(bands={0: (0, 1), 1: (0, 0), 2: (0, 1)}, n={(0, 0): 27, (0, 1): 27, (2, 1): 20}, wins={0: True, 1: True, 2: True})),
    # three bands: 0 inside band 0; 1 rows 63 .. 64; 2 rows 64 .. 127 exactly (b0 = b1 = 1); 3 over all three bands; 4 clamped at the top
    # border; 5 clamped at the bottom border (y > H - 1)
    BRow("bw_h192", 192, 64, [[wt(1.3, 2.2, 14.0, 30.0, 1.0),
                               [[20.3, 62.125, 1], [22.3, 64.875, 1], [47.3, 62.25, 1]],
                               [[5.3, 64.0, 2], [12.3, 127.0, 2], [40.6, 66.0, 2]],
                               [[30.3, 40.2, 5], [40.3, 170.7, 5], [62.6, 50.2, 5]],
                               wt(40.3, -9.8, 20.0, 24.0, 1.0),
                               wt(3.3, 150.2, 25.0, 60.0, 1.0)]],
         dict(bands={0: (0, 0), 1: (0, 1), 2: (1, 1), 3: (0, 2), 4: (0, 0), 5: (2, 2)}, wins={i: True for i in range(6)})),
    # `for (p = lane; p < n; p += 64)`: n = 63 (lane 63 idle), 64 (the exact wave), 65 (one lane takes a second trip), 200 (the stride loop)
    BRow("bw_n", 64, 64, [[bx(2, 2, 3, 21, 1.0), bx(10, 2, 8, 8, 1.0), bx(22, 2, 5, 13, 1.0), bx(30, 2, 10, 20, 1.0)]],
         dict(n={(0, 0): 63, (1, 0): 64, (2, 0): 65, (3, 0): 200}, wins={i: True for i in range(4)})),
    # `if (tri[gp] != fi) continue`: face 1 is wholly hidden behind face 0 (both outputs exactly 0), face 2 half hidden (only its own
    # pixels count); `!front_facing` (3), an empty box (4) and a collinear face (5): b1 < b0, zeros written by the reduce pass
    BRow("bw_hidden", 48, 48, [[wt(2.3, 2.2, 30.0, 30.0, 1.0), wt(6.3, 6.2, 12.0, 12.0, 2.0), wt(14.3, 1.2, 30.0, 26.0, 3.0),
                                flip(wt(20.3, 30.2, 12.0, 12.0, 0.5)), [[40.25, 40.25, 0.5], [40.25, 40.75, 0.5], [40.75, 40.25, 0.5]],
                                [[30, 40, 0.5], [30, 40, 0.5], [44, 46, 0.5]]]],
         dict(bands={3: (0, -1), 4: (0, -1), 5: (0, -1)}, wins={0: True, 1: False, 2: True, 3: False, 4: False, 5: False})),
    # `if (c.inv == 0.f) continue`: the rounding-degenerate face of A.2: no vertex gradient, w = (1, 0, -0)
    BRow("bw_degen", 4, 200, [[DEGEN]], dict(n={(0, 0): 400}, wins={0: True})),
    # `b = blockIdx.z`, `fo = b * F + fi`, `img = b * H * W`: two images with different faces and tri
    BRow("bw_b2", 65, 32, [[wt(2.3, 3.2, 20.0, 40.0, 2.0), wt(4.3, 50.2, 18.0, 20.0, 1.0), wt(6.3, 10.2, 12.0, 12.0, 1.0)],
                           [wt(5.3, 30.2, 22.0, 33.0, 1.0), flip(wt(4.3, 50.2, 18.0, 20.0, 1.0)), wt(1.3, 1.2, 25.0, 20.0, 3.0)]],
         dict(wins={0: True, 1: True, 2: True})),
]
BROW = {r.name: r for r in BROWS}
B_DEGENERATE = {"bw_degen"}


def bands(fv, H, W):
    """numpy restatement of bwd_bands on float32 faces [B, F, 3, 3]: (b0, b1 [B, F], n(b, f, band))"""
    g = geometry(fv, H, W)
    box, listed = g["box"], g["listed"]
    b0 = np.where(listed, box[..., 2] // K["kBand"], 0)
    b1 = np.where(listed, box[..., 3] // K["kBand"], -1)

    def n(b, f, band):
        if not listed[b, f] or band < b0[b, f] or band > b1[b, f]:
            return 0
        r0, r1 = max(box[b, f, 2], band * K["kBand"]), min(box[b, f, 3], band * K["kBand"] + K["kBand"] - 1)
        return int((r1 - r0 + 1) * (box[b, f, 1] - box[b, f, 0] + 1))

    return b0, b1, n


def bary64(P, xy):
    """bary_at in torch: P [N, 3, 2] face vertices, xy [N, 2] pixel centres -> (w [N, 3], den [N]); den == 0 gives w = (1, 0, 0)"""
    v0, v1, v2 = P[:, 2] - P[:, 0], P[:, 1] - P[:, 0], xy - P[:, 0]
    d00, d01, d11 = (v0 * v0).sum(-1), (v0 * v1).sum(-1), (v1 * v1).sum(-1)
    d02, d12 = (v0 * v2).sum(-1), (v1 * v2).sum(-1)
    den = d00 * d11 - d01 * d01
    degen = den == 0
    inv = torch.where(degen, torch.zeros_like(den), 1 / torch.where(degen, torch.ones_like(den), den))
    u = (d11 * d02 - d01 * d12) * inv
    v = (d00 * d12 - d01 * d02) * inv
    return torch.stack([1 - u - v, v, u], -1), den


def bwd_ref(fv, fc, tri, g):
    """fp64 restatement of the backward with autograd.  fv, fc [B, F, 3, 3], tri [B, H, W] int, g [B, H, W, 3] (any float tensors, widened
    to fp64) -> dict(gfv, gfc [B, F, 3, 3], Rv, Rc the bounds' magnitudes, npix [B, F])."""
    B, F = fv.shape[:2]
    fv, fc, g = fv.double(), fc.double(), g.double()
    bi, yi, xi = torch.nonzero(tri >= 0, as_tuple=True)
    fo = bi * F + tri[bi, yi, xi].long()
    P = fv.reshape(B * F, 3, 3)[fo][:, :, :2].clone().requires_grad_(True)  # per pixel: the winning face's vertices
    C = fc.reshape(B * F, 3, 3)[fo].clone().requires_grad_(True)
    gp = g[bi, yi, xi]  # [N, 3]
    w, _ = bary64(P, torch.stack([xi, yi], -1).double())
    loss = ((w[..., None] * C).sum(1) * gp).sum()
    gP, gC = torch.autograd.grad(loss, (P, C), retain_graph=True)
    # R: colour |w_k| |g_ch|; vertex sum_k (sum_ch |g_ch| |c_k,ch|) |d w_k / d p_j|
    Rc_pix = w.detach().abs()[:, :, None] * gp.abs()[:, None, :]
    Rv_pix = torch.zeros_like(gP)
    for k in range(3):
        (J,) = torch.autograd.grad(w[:, k].sum(), P, retain_graph=True)  # [N, 3, 2]: d w_k / d p_j of each pixel
        Rv_pix += (gp.abs() * C.detach()[:, k].abs()).sum(-1)[:, None, None] * J.abs()

    def per_face(t):
        return torch.zeros((B * F,) + t.shape[1:], dtype=torch.float64).index_add_(0, fo, t).reshape((B, F) + t.shape[1:])

    z = torch.zeros(B, F, 3, 1, dtype=torch.float64)
    return dict(gfv=torch.cat([per_face(gP), z], -1), gfc=per_face(gC), Rv=torch.cat([per_face(Rv_pix), z], -1), Rc=per_face(Rc_pix),
                npix=torch.zeros(B * F, dtype=torch.int64).index_add_(0, fo, torch.ones_like(fo)).reshape(B, F))


@functools.lru_cache(maxsize=None)
def backward_case(name):
    """float32 operands of one row (CPU tensors), the oracle's tri, the upstream gradient and the fp64 reference"""
    from oracle import rasterize_oracle as ro
    row = BROW[name]
    fv = face_array(row.faces, np.float32)
    fc = colours(fv)
    B = fv.shape[0]
    d, t, img = ro.new_buffers(B, row.H, row.W)
    ro.standard_rasterize_colors(fv, fc, d, t, img, row.H, row.W)
    gen = torch.Generator().manual_seed(100 + [r.name for r in BROWS].index(name))
    g = torch.randn(B, row.H, row.W, 3, generator=gen)
    fvt, fct, tri = torch.from_numpy(fv), torch.from_numpy(fc), torch.from_numpy(t)
    return dict(fv=fvt, fc=fct, tri=tri, g=g, ref=bwd_ref(fvt, fct, tri, g))


def _note(fam, what, ratio):
    if fam not in WORST or ratio > WORST[fam][0]:
        WORST[fam] = (ratio, what)
    print(f"\n[raster ratio] {fam} {what}: {ratio:.3e} (module worst so far {WORST[fam][0]:.3e} at {WORST[fam][1]})")


def _check(got, ref, R, fam, what):
    got = got.detach().double().cpu()
    assert got.shape == ref.shape == R.shape, (what, got.shape, ref.shape, R.shape)
    assert torch.isfinite(got).all(), f"{what}: {int((~torch.isfinite(got)).sum())} non-finite elements"
    err = (got - ref).abs()
    ratio = (err / (R + TINY)).max().item()
    _note(fam, what, ratio)
    bad = err > TOL[fam] * R + TINY
    if bad.any():
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{what} [{fam}]: {int(bad.sum())} of {bad.numel()} elements out of bound; first at {i}: got {got[i].item():.9e} "
                             f"ref {ref[i].item():.9e} R {R[i].item():.3e}; worst ratio {ratio:.3e} > {TOL[fam]:.1e}")


def _abi_backward(lib, fv, fc, tri, g, H, W, want_v=True, want_c=True):
    """gif_rasterize_colors_bwd_f32 as render.py calls it; outputs and workspace pre-filled with NaN -> (rc, gfv, gfc)"""
    B, F = fv.shape[:2]
    gfv = torch.full_like(fv, NAN) if want_v else None
    gfc = torch.full_like(fc, NAN) if want_c else None
    ws = torch.full((max(lib.gif_rasterize_colors_bwd_workspace_bytes(B, F, H, W) // 4, 1),), NAN, device="cuda")
    rc = lib.gif_rasterize_colors_bwd_f32(fv.data_ptr(), fc.data_ptr(), tri.data_ptr(), g.data_ptr(), gfv.data_ptr() if want_v else None,
                                          gfc.data_ptr() if want_c else None, B, F, H, W, ws.data_ptr(), _stream())
    torch.cuda.synchronize()
    return rc, gfv, gfc


def _bits(t):
    return t.view(torch.int32)


@pytest.mark.parametrize("row", BROWS, ids=[r.name for r in BROWS])
def test_backward(row):
    from gif_amd import _lib
    from gif_amd import standard_rasterize as sr
    lib = _lib.load()
    c = backward_case(row.name)
    H, W = row.H, row.W
    fv, fc, g = c["fv"].cuda(), c["fc"].cuda(), c["g"].cuda()
    B, F = fv.shape[:2]
    depth, tri, img = sr.new_buffers(B, H, W, "cuda")
    sr.standard_rasterize_colors(fv, fc, depth, tri, img, H, W)
    assert torch.equal(tri.cpu(), c["tri"]), f"{row.name}: the forward's tri differs from the oracle's"
    rc, gfv, gfc = _abi_backward(lib, fv, fc, tri, g, H, W)
    assert rc == 0
    ref = c["ref"]
    assert not torch.isnan(gfv).any() and not torch.isnan(gfc).any(), f"{row.name}: an output element was left unwritten"
    assert (gfv[..., 2] == 0).all()  # depth only selects the winner
    if row.name in B_DEGENERATE:
        # den rounds to 0 in fp32 (not in the fp64 restatement): exact statements instead of the vertex bound
        assert (gfv == 0).all()
        assert (gfc[:, :, 1:] == 0).all()  # w[1] = 0, w[2] = -0: +-0 times g
        own = (c["tri"] == 0)[..., None].double()
        plain = (c["g"].double() * own).sum((1, 2))  # [B, 3]: w[0] = 1 on every pixel
        _check(gfc[:, 0, 0], plain, (c["g"].double().abs() * own).sum((1, 2)), "colour", f"{row.name} vertex 0")
    else:
        _check(gfc, ref["gfc"], ref["Rc"], "colour", row.name)
        _check(gfv, ref["gfv"], ref["Rv"], "vertex", row.name)
    lost = ref["npix"] == 0  # a face that won no pixel: both outputs exactly 0, written
    assert (gfv.cpu()[lost] == 0).all() and (gfc.cpu()[lost] == 0).all()
    for f, wins in row.claim.get("wins", {}).items():
        assert bool(ref["npix"][0, f] > 0) == wins, (row.name, f)
    # deterministic: a second call gives the same bits; a null output does not change the other
    rc2, gfv2, gfc2 = _abi_backward(lib, fv, fc, tri, g, H, W)
    assert rc2 == 0 and torch.equal(_bits(gfv), _bits(gfv2)) and torch.equal(_bits(gfc), _bits(gfc2))
    rc3, none_v, gfc3 = _abi_backward(lib, fv, fc, tri, g, H, W, want_v=False)
    assert rc3 == 0 and none_v is None and torch.equal(_bits(gfc), _bits(gfc3))
    rc4, gfv4, none_c = _abi_backward(lib, fv, fc, tri, g, H, W, want_c=False)
    assert rc4 == 0 and none_c is None and torch.equal(_bits(gfv), _bits(gfv4))
    rc5, _, _ = _abi_backward(lib, fv, fc, tri, g, H, W, want_v=False, want_c=False)
    assert rc5 == GIF_EINVAL and "no output" in lib.gif_last_error().decode()


# ---------------------------------------------------------------------------------------------------------------------------------
# C. gif_face_gather_bwd_f32 (mesh.hip: face_gather_bwd_kernel) through render._face_gather_bwd and render._topology
# ---------------------------------------------------------------------------------------------------------------------------------
GA_FAN, GA_FAN_N = 0, 40   # vertex 0: corner 0 of 40 faces around the ring 1 .. 40 (`for (e = off[v]; e < off[v + 1]; ++e)`, 40 trips)
GA_TRI = 41                # corner 0, 1 and 2 of three different faces (with 42 .. 47): `ent[e] & 3` takes all three values, `>> 2` three faces
GA_NOFACE = 50             # no face, in the middle of the range: off[v] == off[v + 1]: exactly 0 from a NaN output
GA_FIRST_FREE = 51         # 51 .. V - 2: a strip of faces (i, i + 1, i + 2); V - 1, the last vertex: no face

GROWS = [
    # name, B, V           one thread per (b, v), 256 per workgroup
    ("ga_v255", 1, 255),   # `i >= B * V`: B * V = 255: lane 255 idle
    ("ga_v256", 1, 256),   # B * V = 256: exactly one workgroup
    ("ga_v257", 1, 257),   # B * V = 257: one live lane in workgroup 1 (the last vertex, which has no face)
    ("ga_v85_b3", 3, 85),  # `gf = gface + b * F * 9`: B * V = 255 with b = i / V in {0, 1, 2}
    ("ga_v86_b3", 3, 86),  # B * V = 258: sample 2's last two vertices in workgroup 1
    ("ga_f1", 2, 8),       # F = 1: faces [(3, 1, 2)]; vertices 0 and 4 .. 7 have no face
]


def gather_faces(name, V):
    if name == "ga_f1":
        return torch.tensor([[3, 1, 2]], dtype=torch.int64)
    faces = [(GA_FAN, 1 + k, 1 + (k + 1) % GA_FAN_N) for k in range(GA_FAN_N)]
    t = GA_TRI
    faces += [(t, t + 1, t + 2), (t + 3, t, t + 4), (t + 5, t + 6, t)]
    faces += [(i, i + 1, i + 2) for i in range(GA_FIRST_FREE, V - 3)]
    return torch.tensor(faces, dtype=torch.int64)


def gather_ref(gface, faces, V):
    """int64 scatter-add: out[b, faces[f, c]] += gface[b, f, c]"""
    B = gface.shape[0]
    out = torch.zeros(B, V, 3, dtype=torch.int64)
    return out.index_add_(1, faces.reshape(-1), gface.long().reshape(B, -1, 3))


def _poison(*numels):
    """Leave NaN-filled blocks of these sizes in the caching allocator, so that an output the kernel never writes reads NaN."""
    ts = [torch.full((n,), NAN, device="cuda") for n in numels for _ in range(4)]
    del ts


@pytest.mark.parametrize("row", GROWS, ids=[r[0] for r in GROWS])
def test_face_gather(row):
    from gif_amd import render
    name, B, V = row
    faces = gather_faces(name, V)
    F = faces.shape[0]
    gen = torch.Generator().manual_seed(7 + [r[0] for r in GROWS].index(name))
    gface = torch.randint(-8, 9, (B, F, 3, 3), generator=gen).float()
    ref = gather_ref(gface, faces, V)
    _, off, ent = render._topology(faces.cuda(), V, torch.device("cuda", torch.cuda.current_device()))
    _poison(B * V * 3)
    got = render._face_gather_bwd(gface.cuda(), off, ent, V).cpu()
    assert got.shape == (B, V, 3) and got.dtype == torch.float32
    assert not torch.isnan(got).any(), f"{name}: {int(torch.isnan(got).any(-1).sum())} vertices were left unwritten"
    assert torch.equal(got.double(), ref.double()), f"{name}: {int((got.double() != ref.double()).any(-1).sum())} vertices differ"
    count = torch.bincount(faces.reshape(-1), minlength=V)
    assert (got[:, count == 0] == 0).all() and count[V - 1] == 0
    if name != "ga_f1":
        assert count[GA_FAN] == GA_FAN_N and count[GA_TRI] == 3 and count[GA_NOFACE] == 0
        assert sorted(int((faces[:, c] == GA_TRI).sum()) for c in range(3)) == [1, 1, 1]
