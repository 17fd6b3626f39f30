"""-m gpu: the Winograd kernels (csrc/conv_winograd.hip: wino_input_transform_rows<8>, wino_gy_transform, the weight transforms,
wino_gemm_mfma<2> / <4>, wino_gemm_x3<128,128>, wino_gemm_h2<128,128,3>; the plane mode of csrc/conv_wgrad.hip and
wino_unpack_wgrad_kernel) at the edges of their own index arithmetic, against an fp64 reference.

tests/test_gpu_conv_routes.py puts rows on the eligibility predicates of ops.py; here ops.conv3x3_winograd and
ops.conv3x3_winograd_wgrad are called directly (they only need R <= cout_act, C % 4 == 0 and even H / W), so that a row can sit on an
edge INSIDE the kernels: tile rows per lane of the input transform (TYB = 8), channel padding (C..CP), the transform's grid cap
(256 * 32 workgroups of 256 lanes = 2 097 152 lanes per trip of the grid-stride loop), the row padding of V / Mg (ntiles..ntiles_pad,
WPAD = 256: two 128-row M blocks), ragged M / N / K blocks of the three GEMMs, xcd_remap with a grid that is no multiple of 8, the
`wide` predicate of the native GEMM, the tile pairs, the 256-row tile and the split chunks of the plane GEMMs.  Each row's comment names
the edge and the side; rows are seeded from their own description.  Every row runs in the three contraction modes
(ops.set_fp32_mfma_mode); which GEMM a mode runs is part of the row: with cout_act % 128 != 0 the split modes run the native GEMM
(family 2), else wino_gemm_x3 (10) / wino_gemm_h2 (14); the plane GEMMs run bf16x3 (11) / f16x2 (16) only on 128 x 128 tiles, else the
native kernel (3).  The family is asserted through ops.prof_read; tile sizes, `wide` and the split chunks are not observable from
Python: the row's `claim` is checked on the CPU against the constants of the sources (tests/test_cpu_wiring.py:
test_winograd_edges_*).  A grid of 9 workgroups cannot occur — tiles_m = ntiles_pad / 128 is even because WPAD = 2 * WBM — so the
xcd_remap rows have 2, 6 and 10 workgroups.

Reference: torch.float64 on the CPU over the operands the kernels read.  Bound, per element and with no element excluded
(test_gpu_conv_routes._check):

    |got - ref| <= TOL[family] * R + TINY[family]

R is the direct operation (conv2d / conv_transpose2d / the weight gradient) on absolute values carried through the epilogue, as in
test_gpu_conv_routes, and the tolerances are that module's families native / bf16x3 / f16x2 unchanged: no Winograd row exceeds them
(below), so no Winograd-specific family with a wider R was needed.  The fused column sums and dot products are held against the
sums of R.  V (keep_v=True) is held to B^T d B * s in fp64 with TOL["wino_v"] = 5 * 2^-24: four additions and one multiplication,
each rounding at most 2^-24 of |B^T| |d| |B| |s| (from the number format, not from a measurement).

Observed worst |got - ref| / R on the MI355X (all rows of this module, one run; fused column sums and dot products in brackets)
against the tolerance it is held to:
  native  3.8e-7 (wide_512 out)      [4.0e-9]  ->  TOL 2e-6    (5.3 x; the family's own worst is 4.4e-7)
  bf16x3  3.4e-7 (w32x32_t31 dW)     [4.4e-9]  ->  TOL 2e-6    (5.9 x)
  f16x2   3.4e-7 (w32x32_t31 dW)     [4.0e-9]  ->  TOL 1.5e-6  (4.4 x)
  wino_v  1.4e-7 (c36_scaled V)                ->  TOL 3.0e-7  (5 * 2^-24)
(w32x32_t31 runs the native 32 x 32 plane GEMM in every mode.)  Every case prints its ratio ("[route ratio]" lines with -s) so that
a re-measurement is one run of this module.

Poisoned workspaces (section f): the library's C entry points are called as ops.py calls them, on V / Mg / ws / y buffers with
sentinels behind the size the library asks for, pre-filled with zeros, quiet NaN, 3e38 and (f16x2) a row pattern with a 16-channel
group 2^-24 below the others: results bit-equal between the fills, finite, sentinels untouched, and the f16x2 gate unmoved — against
weights whose packed rows carry the narrow flag, with a control that puts the same group into a real row of x.

Out of scope: RUNNING the knob-only A/B kernels (GIF_WINO_XFORM, GIF_WINO_WN, GIF_WINO_X3_TILE, GIF_WINO_H2_STAGES are read once per
process).  Which kernel, tile and ring depth each value of the four selects is covered on the CPU: csrc/wino_route.h parses them, and
tests/golden/wino_route_table.txt (tests/test_wino_route.py) records the route of every value.
"""
import ctypes
import math
import zlib
from typing import NamedTuple

import pytest
import torch
import torch.nn.functional as F

from test_gpu_conv_routes import TINY, TOL, _check

pytestmark = pytest.mark.gpu

CL = torch.channels_last
MODES = ("native", "bf16x3", "f16x2")
SQRT2 = 2 ** 0.5

TOL.update({"wino_v": 5 * 2.0 ** -24})
TINY.update({"wino_v": 1e-30})

# The constants of csrc/wino_route.h this module's rows are computed from (tests/test_cpu_wiring.py holds them to the header's)
K = dict(WBM=128, WBN=64, WBK=32, WPAD=256, TYB=8, CAP_WG=256 * 32, WIDE_MIN=512)
CAP_LANES = K["CAP_WG"] * 256  # 2 097 152 lanes per trip of the transforms' grid-stride loop

# the input transform of F(2x2, 3x3), Y = A^T [(G g G^T) .* (B^T d B)] A
BT = torch.tensor([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=torch.float64)


def _rng(*desc):
    return torch.Generator().manual_seed(zlib.crc32(repr(desc).encode()))


def _cl(t):
    return t.cuda().contiguous(memory_format=CL)


def geometry(B, C, Co, H, W, mode="native", k=K):
    """What the host code of conv_winograd.hip computes for a forward / data-gradient call (C = contraction channels, Co = cout_act)."""
    TH, TW = H // 2, W // 2
    ntiles = B * TH * TW
    pad = -(-ntiles // k["WPAD"]) * k["WPAD"]
    CP = -(-C // k["WBK"]) * k["WBK"]
    split = mode != "native" and Co % 128 == 0
    RP = -(-Co // 128) * 128 if split else -(-Co // k["WBN"]) * k["WBN"]
    tiles_m = pad // k["WBM"]
    wide = (not split) and Co % 128 == 0 and tiles_m * (RP // 128) >= k["WIDE_MIN"]
    bn = 128 if (split or wide) else k["WBN"]
    lanes = B * -(-TH // k["TYB"]) * TW * (CP // 4)
    return dict(TH=TH, TW=TW, ntiles=ntiles, ntiles_pad=pad, CP=CP, RP=RP, tiles_m=tiles_m, tiles_n=RP // bn, nwg=tiles_m * (RP // bn),
                wide=wide, lanes=lanes, trips=-(-lanes // (k["CAP_WG"] * 256)), yblocks=-(-TH // k["TYB"]), last_block=TH - (-(-TH // k["TYB"]) - 1) * k["TYB"],
                gemm=("h2" if mode == "f16x2" else "x3") if split else ("mfma4" if wide else "mfma2"), pad_blocks=(pad - ntiles) // k["WBM"])


# ---------------------------------------------------------------------------------------------------------------------------------
# fp64 references
# ---------------------------------------------------------------------------------------------------------------------------------
def wino_v64(x, absolute=False):
    """V[16][B * TH * TW][C] = B^T d B over the 4x4 patches of the padded x (stride 2), in fp64."""
    m = (lambda t: t.abs()) if absolute else (lambda t: t)
    B, C, H, W = x.shape
    TH, TW = H // 2, W // 2
    xp = F.pad(m(x), (1, 1, 1, 1))
    out = x.new_zeros(4, 4, B, C, TH, TW)
    for r in range(4):
        for s in range(4):
            d = xp[:, :, r:r + 2 * TH - 1:2, s:s + 2 * TW - 1:2]
            out += m(BT)[:, r].view(4, 1, 1, 1, 1, 1) * m(BT)[:, s].view(1, 4, 1, 1, 1, 1) * d
    return out.permute(0, 1, 2, 4, 5, 3).reshape(16, B * TH * TW, C)


def wgrad64(gy, x):
    with torch.enable_grad():
        ww = torch.zeros(gy.shape[1], x.shape[1], 3, 3, dtype=torch.float64, requires_grad=True)
        (gw,) = torch.autograd.grad(F.conv2d(x, ww, padding=1), ww, gy)
    return gw


# ---------------------------------------------------------------------------------------------------------------------------------
# a-d. forward / data gradient: input transform, the three GEMMs with the fused output transform, the epilogue
# ---------------------------------------------------------------------------------------------------------------------------------
class FRow(NamedTuple):
    name: str
    shape: tuple          # (B, C, Co, H, W): C = channels of the op's input (the contraction), Co = cout_act
    claim: dict           # the edge the comment names, as values of geometry() (native mode unless the key says otherwise)
    op: str = "fwd"       # fwd | dgrad (rows_are_out=False: flipped taps, swapped channels)
    epi: str = ""         # "" | in (per-sample in_scale) | full (in / out scales, residual, bias, act) | fuse (mask + colsum) | fusedot
    v: bool = False       # also check V from keep_v=True
    wview: bool = False   # weights as a non-contiguous view
    modes: tuple = MODES


FROWS = [
    # ---- a. input transform wino_input_transform_rows<8>: one lane walks up to 8 tiles down a tile column of one sample
    FRow("th1_tw1", (3, 32, 64, 2, 2), dict(ntiles=3, TH=1, TW=1, yblocks=1, last_block=1), epi="in"),   # every patch touches all four borders
    FRow("th7", (2, 32, 64, 14, 6), dict(TH=7, yblocks=1, last_block=7)),     # one short block: ty1 = min(8, 7); sample 1 starts at tile row 7
    FRow("th8", (2, 32, 64, 16, 6), dict(TH=8, yblocks=1, last_block=8)),     # one full block
    FRow("th9", (2, 32, 64, 18, 6), dict(TH=9, yblocks=2, last_block=1)),     # a second block of one tile
    FRow("th17", (2, 32, 64, 34, 6), dict(TH=17, yblocks=3, last_block=1)),
    FRow("c36_scaled", (3, 36, 64, 18, 6), dict(CP=64, TH=9), epi="in", v=True),   # CP 64: 28 pad channels write zeros and must not read
                                                                                    #   in_scale; per-sample scale, sample index in every block
    FRow("c60", (2, 60, 64, 14, 6), dict(CP=64, TH=7), epi="in", v=True),          # one pad quad
    FRow("cap_exact", (16, 2048, 4, 2, 512), dict(ntiles=4096, lanes=CAP_LANES, trips=1)),       # 4096 tiles x 512 lanes: exactly the cap
    FRow("cap_over", (17, 2048, 4, 2, 482), dict(ntiles=4097, lanes=CAP_LANES + 512, trips=2)),  # second trip: the last tile of the last sample
    # ---- b. native GEMM wino_gemm_mfma<2> (128 x 64 blocks) in every mode (Co % 128 != 0): tile counts around the M block and WPAD
    FRow("t127", (1, 32, 64, 2, 254), dict(ntiles=127, ntiles_pad=256, tiles_m=2, pad_blocks=1, nwg=2)),   # one row short of an M block;
                                                                                                            #   2 workgroups: nwg < 8
    FRow("t128", (1, 32, 64, 2, 256), dict(ntiles=128, ntiles_pad=256, tiles_m=2, pad_blocks=1)),   # a whole M block of padding rows
    FRow("t129", (3, 32, 64, 2, 86), dict(ntiles=129, ntiles_pad=256, tiles_m=2, pad_blocks=0)),    # one real row in the second block
    FRow("t255", (3, 32, 64, 10, 34), dict(ntiles=255, ntiles_pad=256, pad_blocks=0)),
    FRow("t256", (1, 32, 64, 32, 32), dict(ntiles=256, ntiles_pad=256, pad_blocks=0)),              # no padding row at all
    FRow("t257", (1, 32, 64, 2, 514), dict(ntiles=257, ntiles_pad=512, tiles_m=4, pad_blocks=1)),   # block 2 holds one row, block 3 none
    FRow("co4", (3, 32, 4, 2, 86), dict(RP=64, tiles_n=1)),                    # one float4 of real columns
    FRow("co60", (3, 32, 60, 2, 86), dict(RP=64, tiles_n=1)),                  # the last float4 of the N block is padding
    FRow("co68", (3, 32, 68, 2, 86), dict(RP=128, tiles_n=2, nwg=4)),          # the second N block holds four real columns
    FRow("co124", (3, 32, 124, 2, 86), dict(RP=128, tiles_n=2)),
    FRow("c36", (3, 36, 64, 2, 86), dict(CP=64)),                              # two K chunks, the second with 4 real channels
    FRow("nwg6", (3, 32, 132, 2, 86), dict(RP=192, nwg=6)),                    # xcd_remap: nwg < 8 with three N blocks
    FRow("nwg10", (3, 32, 260, 2, 86), dict(RP=320, nwg=10)),                  # xcd_remap: nwg % 8 == 2 (tiles_m is even: 9 cannot occur)
    FRow("wide_512", (1, 4, 128, 512, 512), dict(tiles_m=512, wide=True, gemm="mfma4"), modes=("native",)),   # 8-wave 128 x 128 kernel
    FRow("wide_510", (1, 4, 128, 510, 512), dict(tiles_m=510, wide=False, gemm="mfma2"), modes=("native",)),  # 4-wave kernel
    # ---- c. wino_gemm_x3<128,128> (bf16x3) / wino_gemm_h2<128,128,3> (f16x2): Co % 128 == 0; native runs wino_gemm_mfma<2>
    FRow("s_t127", (1, 32, 128, 2, 254), dict(ntiles=127, **{"gemm:bf16x3": "x3", "gemm:f16x2": "h2", "gemm": "mfma2"})),
    FRow("s_t129", (3, 32, 128, 2, 86), dict(ntiles=129, **{"gemm:bf16x3": "x3", "gemm:f16x2": "h2"})),
    FRow("s_t257_co256", (1, 32, 256, 2, 514), dict(ntiles=257, ntiles_pad=512, **{"tiles_n:bf16x3": 2, "nwg:f16x2": 8})),
    FRow("s_c36", (3, 36, 128, 2, 86), dict(CP=64, **{"gemm:f16x2": "h2"})),
    FRow("s_dgrad", (3, 32, 128, 2, 86), dict(ntiles=129), op="dgrad"),        # flipped taps, swapped channel strides
    FRow("s_wview", (3, 36, 128, 2, 86), dict(ntiles=129), wview=True),        # a permuted slice of a larger tensor
    FRow("s_wview_dgrad", (3, 36, 68, 2, 86), dict(ntiles=129), op="dgrad", wview=True),
    # ---- d. epilogue on a ragged tile count (129) and ragged Co (68: native GEMM; 128: split GEMMs)
    FRow("e_full_68", (3, 32, 68, 2, 86), dict(ntiles=129, RP=128), epi="full"),
    FRow("e_full_128", (3, 32, 128, 2, 86), dict(ntiles=129, **{"gemm:f16x2": "h2"}), epi="full"),
    FRow("e_fuse_68", (3, 32, 68, 2, 86), dict(ntiles=129), op="dgrad", epi="fuse"),
    FRow("e_fuse_128", (3, 32, 128, 2, 86), dict(ntiles=129), op="dgrad", epi="fuse"),
    FRow("e_dot_68", (3, 32, 68, 16, 32), dict(ntiles=384, ntiles_pad=512, pad_blocks=1), op="dgrad", epi="fusedot"),  # 128 tiles per sample
    FRow("e_dot_128", (3, 32, 128, 16, 32), dict(ntiles=384, pad_blocks=1), op="dgrad", epi="fusedot"),
]
F_CASES = [pytest.param(r, m, id=f"{r.name}-{m}") for r in FROWS for m in r.modes]
_FREF = {}


@pytest.fixture(autouse=True)
def _restore():
    from gif_amd import ops
    before, guard = ops.get_fp32_mfma_mode(), ops.H2_GUARD
    ops.h2_fallback_stats(reset=True)
    yield
    ops.prof_enable(False)
    ops.set_fp32_mfma_mode(before)
    ops.H2_GUARD = guard
    ops.h2_fallback_stats(reset=True)


def _wview(row, store):
    """the canonical [O, I, 3, 3] view of a row's stored weights (CPU or device: a sliced view does not keep its strides across .cuda())"""
    if not row.wview:
        return store
    B, C, Co, H, W = row.shape
    O, I = (Co, C) if row.op == "fwd" else (C, Co)
    return store[:, :, 2:2 + I, 1:1 + O].permute(3, 2, 0, 1)


def _f_operands(row):
    """CPU fp32 operands.  w is the canonical forward-conv weight [O, I, 3, 3]: fwd: O = Co, I = C; dgrad: O = C (the op's input), I = Co."""
    B, C, Co, H, W = row.shape
    g = _rng(row.name, row.shape, row.op, row.epi)
    O, I = (Co, C) if row.op == "fwd" else (C, Co)
    if row.wview:  # stored [3, 3, I + 5, O + 3]: every stride differs from the contiguous layout's
        store = torch.randn(3, 3, I + 5, O + 3, generator=g) / math.sqrt(9 * C)
    else:
        store = torch.randn(O, I, 3, 3, generator=g) / math.sqrt(9 * C)
    o = {"w_store": store, "w": _wview(row, store), "x": torch.randn(B, C, H, W, generator=g)}
    if row.epi in ("in", "full"):
        o["in_scale"] = torch.rand(B, C, generator=g) + 0.5
    if row.epi == "full":
        o["out_scale"] = torch.rand(B, Co, generator=g) + 0.5
        o["bias"] = torch.randn(Co, generator=g)
        o["residual"] = torch.randn(B, Co, H, W, generator=g)
    if row.epi in ("fuse", "fusedot"):
        o["mask_src"] = torch.randn(B, Co, H, W, generator=g)
    if row.epi == "fusedot":
        o["dot_src"] = torch.randn(B, Co, H, W, generator=g)
    return o


def _f_reference(row):
    """name -> (ref, R), shared by the modes"""
    key = (row.name, row.shape, row.op, row.epi)
    if key in _FREF:
        return _FREF[key]
    o = {k: v.double() for k, v in _f_operands(row).items() if k != "w_store"}
    x, w = o["x"], o["w"]
    if "in_scale" in o:
        x = x * o["in_scale"][:, :, None, None]
    g = w if row.op == "fwd" else w.flip(2, 3).transpose(0, 1)  # the data gradient as a forward conv
    z, R = F.conv2d(x, g, padding=1), F.conv2d(x.abs(), g.abs(), padding=1)
    out = {}
    if row.v:
        s = o["in_scale"].repeat_interleave((row.shape[3] // 2) * (row.shape[4] // 2), 0)[None] if "in_scale" in o else 1.0
        out["v"] = (wino_v64(o["x"]) * s, wino_v64(o["x"], absolute=True) * s)
    if "dot_src" in o:  # taken before out_scale
        out["dot"] = ((z * o["dot_src"]).sum((2, 3)), (R * o["dot_src"].abs()).sum((2, 3)))
    if "out_scale" in o:
        z, R = z * o["out_scale"][:, :, None, None], R * o["out_scale"][:, :, None, None]
    if "residual" in o:  # (epi "full": residual, bias and the leaky ReLU come together)
        z, R = z + o["residual"] + o["bias"][None, :, None, None], R + o["residual"].abs() + o["bias"].abs()[None, :, None, None]
        z, R = SQRT2 * F.leaky_relu(z, 0.2), SQRT2 * R
    if "mask_src" in o:
        f = SQRT2 * torch.where(o["mask_src"] > 0, 1.0, 0.2).double()
        z, R = z * f, R * f
        out["colsum"] = (z.sum((0, 2, 3)), R.sum((0, 2, 3)))
    out["y"] = (z, R)
    _FREF[key] = out
    if row.name.startswith("wide_"):  # 0.8 GB of fp64, used by one case: not kept
        _FREF.pop(key)
    return out


def _f_run(row, o, w_dev, keep_v=False):
    from gif_amd import ops
    B, C, Co, H, W = row.shape
    epi = {}
    for k in ("in_scale", "out_scale", "bias"):
        if k in o:
            epi[k] = o[k].cuda().contiguous()
    if "residual" in o:
        epi["residual"] = _cl(o["residual"])
        epi["act"] = True
    fuse = None
    if "mask_src" in o:
        fuse = ops.GradFuse(mask_src=_cl(o["mask_src"]), mask_slope=0.2, mask_gain=SQRT2, want_colsum=True,
                            dot_src=_cl(o["dot_src"]) if "dot_src" in o else None)
        epi["fuse"] = fuse
    out = ops.conv3x3_winograd(o["x_dev"], w_dev, row.op == "fwd", Co, keep_v=keep_v, **epi)
    return (*out, fuse) if keep_v else (out, None, fuse)


def _prof_begin():
    from gif_amd import ops
    ops.prof_enable(True)
    for f in range(18):
        ops.prof_read(f)  # (reading clears a family's records)


def _ran():
    from gif_amd import ops
    torch.cuda.synchronize()
    ran = {f: ops.prof_read(f)[2] for f in range(18)}
    ops.prof_enable(False)
    return {f: n for f, n in ran.items() if n and f != 4}  # (4: the transforms, recorded beside the GEMM)


@pytest.mark.parametrize("row,mode", F_CASES)
def test_winograd_forward_edges(row, mode):
    from gif_amd import ops
    B, C, Co, H, W = row.shape
    geo = geometry(*row.shape, mode)
    ops.set_fp32_mfma_mode(mode)
    o = _f_operands(row)
    ref = _f_reference(row)
    o["x_dev"] = _cl(o["x"])
    w_dev = _wview(row, o["w_store"].cuda())
    assert w_dev.stride() == o["w"].stride() and w_dev.is_contiguous() != row.wview
    _prof_begin()
    y, V, fuse = _f_run(row, o, w_dev, keep_v=row.v)
    fam = {"mfma2": 2, "mfma4": 2, "x3": 10, "h2": 14}[geo["gemm"]]
    assert _ran() == {fam: 1}, f"{row.name} [{mode}]: expected one op in family {fam} ({geo['gemm']})"
    if mode == "f16x2":
        assert ops.h2_fallback_stats() == 0, f"{row.name}: well-scaled operands took the guarded bf16x3 fallback"
    assert y.shape == (B, Co, H, W) and y.dtype == torch.float32 and y.is_contiguous(memory_format=CL)
    got = y.double().cpu()
    y2, _, fuse2 = _f_run(row, o, w_dev)
    assert torch.equal(y, y2), f"{row.name} [{mode}]: a second call gave different bits"
    del y, y2
    assert torch.isfinite(got).all(), f"{row.name}: NaN / Inf"
    _check(got, *ref["y"], mode, f"{row.name} out")
    if fuse is not None:
        assert torch.equal(fuse.colsum, fuse2.colsum), f"{row.name}: the fused column sums changed between two calls"
        _check(fuse.colsum.double().cpu(), *ref["colsum"], mode, f"{row.name} colsum")
        if "dot" in ref:
            assert torch.equal(fuse.dot, fuse2.dot)
            _check(fuse.dot.double().cpu(), *ref["dot"], mode, f"{row.name} dot")
    if row.v:
        Vd = V.view(16, geo["ntiles_pad"], geo["CP"])[:, :geo["ntiles"]]
        assert torch.count_nonzero(Vd[:, :, C:].contiguous().view(torch.int32)).item() == 0, f"{row.name}: channel padding of V is not +0"
        vref, vR = ref["v"]
        _check(Vd[:, :, :C].double().cpu(), vref, vR, "wino_v", f"{row.name} V")


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("Co", [68, 128])
def test_winograd_dot_fusion_refused_at_48_tiles_per_sample(Co, mode):
    """per_sample = 4 * 12 = 48 is no multiple of the 128-row M block: the call fails before the GEMM and leaves y as it was."""
    from gif_amd import _lib, ops
    ops.set_fp32_mfma_mode(mode)
    B, C, H, W = 3, 32, 8, 24
    g = _rng("dot48", Co)
    x, w = _cl(torch.randn(B, C, H, W, generator=g)), torch.randn(C, Co, 3, 3, generator=g).cuda()
    src = _cl(torch.randn(B, Co, H, W, generator=g))
    with pytest.raises(_lib.GifHipError, match="dot fusion"):
        ops.conv3x3_winograd(x, w, False, Co, fuse=ops.GradFuse(dot_src=src))
    y = torch.full((B * H * W * Co + 256,), -7.25, device="cuda")
    fuse = ops.GradFuse(dot_src=src, want_colsum=True)
    e = ops._epilogue(out_bchw=(B, Co, H, W), fuse=fuse)
    V = torch.zeros((_lib.load().gif_winograd_workspace_floats(B, H, W, C) + 256,), device="cuda")
    rc = _c_conv(mode, x, w, Co, False, V, y, e)
    assert rc != 0 and b"dot fusion" in _lib.load().gif_last_error()
    torch.cuda.synchronize()
    assert (y == -7.25).all(), "the refused call wrote to y"


# ---------------------------------------------------------------------------------------------------------------------------------
# e. weight gradient: wino_gy_transform, wino_input_transform_rows<8>, the 16 plane GEMMs (conv_wgrad.hip), wino_unpack_wgrad_kernel
# ---------------------------------------------------------------------------------------------------------------------------------
class WRow(NamedTuple):
    name: str
    shape: tuple          # (B, Cs, Cb, H, W, O, I): small = output gradient [B, Cs, H, W], big = input [B, Cb, H, W], dW [O, I, 3, 3]
    claim: dict           # ntiles; tile = (BP, BQ) of the native launch; x3: the split modes run their own 128 x 128 kernels; nsplit, chunk
    opt: str = ""         # "" | wscale | scales (per-sample small_scale / big_scale) | keepv (big_v from the forward pass)
    modes: tuple = MODES


WROWS = [
    # ---- plane-GEMM tile pairs: tile_of(CsP) x tile_of(CbP) with CsP / CbP the 32-padded channels (32 -> 32; 36, 64 -> 64 -> 128)
    WRow("w32x32_t31", (1, 32, 32, 2, 62, 32, 32), dict(ntiles=31, tile=(32, 32), x3=False, nsplit=1, chunk=32)),       # one stage, one row short
    WRow("w32x128_t33", (3, 32, 36, 2, 22, 32, 35), dict(ntiles=33, tile=(32, 128), x3=False, nsplit=1, chunk=64)),     # second stage of one tile;
                                                                                                                         #   I 35 of 36
    WRow("w128x32_t75", (3, 36, 32, 10, 10, 36, 32), dict(ntiles=75, tile=(128, 32), x3=False, nsplit=1, chunk=96)),
    WRow("w128x128_t129", (3, 64, 64, 2, 86, 64, 64), dict(ntiles=129, tile=(128, 128), x3=True, nsplit=2, chunk=96)),  # two splits, the last 33
    WRow("w_splits8", (1, 64, 64, 20, 200, 64, 64), dict(ntiles=1000, tile=(128, 128), x3=True, nsplit=8, chunk=128)),  # last split 104 of 128
    WRow("w_o66_i35", (3, 68, 36, 10, 10, 66, 35), dict(ntiles=75, tile=(128, 128), x3=True, nsplit=1, chunk=96)),      # O < Cs, I < Cb: unpack
    WRow("w_wscale", (3, 36, 64, 2, 86, 36, 64), dict(ntiles=129, tile=(128, 128), x3=True, nsplit=2), opt="wscale"),
    WRow("w_scales", (3, 64, 36, 10, 10, 64, 36), dict(ntiles=75, tile=(128, 128), x3=True), opt="scales"),
    WRow("w_keepv", (3, 64, 36, 18, 6, 64, 33), dict(ntiles=81, tile=(128, 128), x3=True), opt="keepv"),
    # ---- 256 x 128 tiles, native only: CsP 160 -> RP 256, from 16 384 tiles
    WRow("w_big_16384", (1, 132, 64, 256, 256, 132, 64), dict(ntiles=16384, tile=(256, 128), big=True, nsplit=64, chunk=256), modes=("native",)),
    WRow("w_big_16128", (1, 132, 64, 252, 256, 132, 64), dict(ntiles=16128, tile=(128, 128), big=False, nsplit=32, chunk=512), modes=("native",)),
]
W_CASES = [pytest.param(r, m, id=f"{r.name}-{m}") for r in WROWS for m in r.modes]
_WREF = {}


def _w_operands(row):
    B, Cs, Cb, H, W, O, I = row.shape
    g = _rng(row.name, row.shape, row.opt)
    o = {"small": torch.randn(B, Cs, H, W, generator=g), "big": torch.randn(B, Cb, H, W, generator=g), "wscale": 1.0}
    if row.opt == "wscale":
        o["wscale"] = -0.37
    if row.opt in ("scales", "keepv"):
        o["big_scale"] = torch.rand(B, Cb, generator=g) + 0.5
    if row.opt == "scales":
        o["small_scale"] = torch.rand(B, Cs, generator=g) + 0.5
    return o


def _w_reference(row):
    key = (row.name, row.shape, row.opt)
    if key not in _WREF:
        o = _w_operands(row)
        O, I = row.shape[5:]
        gy, x = o["small"].double(), o["big"].double()
        if "small_scale" in o:
            gy = gy * o["small_scale"].double()[:, :, None, None]
        if "big_scale" in o:
            x = x * o["big_scale"].double()[:, :, None, None]
        s = o["wscale"]
        _WREF[key] = (s * wgrad64(gy, x)[:O, :I], abs(s) * wgrad64(gy.abs(), x.abs())[:O, :I])
    return _WREF[key]


@pytest.mark.parametrize("row,mode", W_CASES)
def test_winograd_wgrad_edges(row, mode):
    from gif_amd import ops
    B, Cs, Cb, H, W, O, I = row.shape
    ops.set_fp32_mfma_mode(mode)
    o = _w_operands(row)
    ref, R = _w_reference(row)
    small, big = _cl(o["small"]), _cl(o["big"])
    ss = o["small_scale"].cuda() if "small_scale" in o else None
    bs = o["big_scale"].cuda() if "big_scale" in o else None
    _prof_begin()
    dw = ops.conv3x3_winograd_wgrad(small, big, O, I, o["wscale"], ss, bs)
    fam = 3 if (mode == "native" or not row.claim.get("x3")) else (11 if mode == "bf16x3" else 16)
    assert _ran() == {fam: 1}, f"{row.name} [{mode}]: expected one op in family {fam}"
    if mode == "f16x2":
        assert ops.h2_fallback_stats() == 0, f"{row.name}: well-scaled operands took the guarded bf16x3 fallback"
    assert dw.shape == (O, I, 3, 3) and dw.dtype == torch.float32
    dw2 = ops.conv3x3_winograd_wgrad(small, big, O, I, o["wscale"], ss, bs)
    assert torch.equal(dw, dw2), f"{row.name} [{mode}]: a second call gave different bits"
    if row.opt == "keepv":  # V kept from the forward pass over the same (big, big_scale)
        w = torch.randn(Cs, Cb, 3, 3, generator=_rng(row.name, "w")).cuda()
        _, V = ops.conv3x3_winograd(big, w, True, Cs, keep_v=True, in_scale=bs)
        dw3 = ops.conv3x3_winograd_wgrad(small, big, O, I, o["wscale"], ss, bs, big_v=V)
        assert torch.equal(dw, dw3), f"{row.name} [{mode}]: the forward pass's V gives other bits than the recomputed one"
    got = dw.double().cpu()
    assert torch.isfinite(got).all()
    _check(got, ref, R, mode, f"{row.name} dW")


# ---------------------------------------------------------------------------------------------------------------------------------
# f. poisoned workspaces, through the C API as ops.py calls it
# ---------------------------------------------------------------------------------------------------------------------------------
GUARD = 256  # sentinel floats behind the size the library asks for


def _c_conv(mode, x, w, Co, rows_are_out, V, y, e):
    """ops.conv3x3_winograd's calls on caller-owned V and y (flat fp32 buffers); returns the launch's status."""
    from gif_amd import _lib, ops
    lib = _lib.load()
    B, C, H, W = x.shape
    assert x.is_contiguous(memory_format=CL)
    x3 = mode != "native" and Co % 128 == 0
    h2 = x3 and mode == "f16x2"
    RP, CP = ctypes.c_int(), ctypes.c_int()
    _lib.check((lib.gif_winograd_pack_dims_x3 if x3 else lib.gif_winograd_pack_dims)(Co, C, ctypes.byref(RP), ctypes.byref(CP)), "pack_dims")
    O, I = w.shape[:2]
    so, si, sky, skx = w.stride()
    R, Cc, sr, sc = (O, I, so, si) if rows_are_out else (I, O, si, so)
    tail = (R, Cc, RP.value, CP.value, sr, sc, sky, skx, 0 if rows_are_out else 1, 1.0, ops._stream())
    dims = (B, H, W, C, Co, ctypes.byref(e), ops._stream())
    if h2:
        U2 = torch.empty((lib.gif_winograd_weight_f32h2_bytes(RP.value, CP.value),), device=x.device, dtype=torch.uint8)
        U3 = torch.empty((16, 3, RP.value, CP.value), device=x.device, dtype=torch.bfloat16)
        _lib.check(lib.gif_winograd_weight_f32h2(w.data_ptr(), U2.data_ptr(), U3.data_ptr(), *tail), "winograd_weight_f32h2")
        return lib.gif_conv3x3_winograd_f32h2(x.data_ptr(), U2.data_ptr(), U3.data_ptr(), y.data_ptr(), V.data_ptr(), *dims)
    if x3:
        U = torch.empty((16, 3, RP.value, CP.value), device=x.device, dtype=torch.bfloat16)
        _lib.check(lib.gif_winograd_weight_f32x3(w.data_ptr(), U.data_ptr(), *tail), "winograd_weight_f32x3")
        return lib.gif_conv3x3_winograd_f32x3(x.data_ptr(), U.data_ptr(), y.data_ptr(), V.data_ptr(), *dims)
    U = torch.empty((16, RP.value, CP.value), device=x.device, dtype=torch.float32)
    _lib.check(lib.gif_winograd_weight_f32(w.data_ptr(), U.data_ptr(), *tail), "winograd_weight_f32")
    return lib.gif_conv3x3_winograd_f32(x.data_ptr(), U.data_ptr(), y.data_ptr(), V.data_ptr(), *dims)


def _poison(buf, n, kind, cols=None):
    """Fill the first n floats of `buf` (the size the library asks for); the sentinels behind them get a pattern of their own."""
    if kind == "zero":
        buf[:n] = 0.0
    elif kind == "nan":
        buf[:n] = float("nan")
    elif kind == "3e38":
        buf[:n] = 3e38
    else:  # "window": rows of ones with channels 32..47 (one 16-element K group) 2^-24 below them
        v = buf[:n].view(-1, cols)
        v[:] = 1.0
        v[:, 32:48] = 2.0 ** -24
    buf[n:] = torch.arange(buf.numel() - n, device=buf.device, dtype=torch.float32) + 0.5


def _sentinels_ok(buf, n):
    return torch.equal(buf[n:], torch.arange(buf.numel() - n, device=buf.device, dtype=torch.float32) + 0.5)


def _bits(t):
    return t.contiguous().view(torch.int32)


FILLS = {"native": ("nan", "3e38"), "bf16x3": ("nan", "3e38"), "f16x2": ("nan", "3e38", "window")}


def _window_weights(O, I, g):
    """the "window" weights of test_f16x2_winograd_adversarial: 16 input channels 2^24 above the others -> every packed row is flagged"""
    w = torch.randn(O, I, 3, 3, generator=g) / 34
    w[:, 32:48] *= 2.0 ** 24
    return w


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", [(3, 64, 128, 2, 86), (3, 64, 68, 2, 86), (3, 64, 128, 16, 32)], ids=["t129_co128", "t129_co68", "t384_dot"])
def test_winograd_forward_ignores_workspace_padding(shape, mode):
    """"the row padding (ntiles..ntiles_pad) is never written and never matters"; "rows >= ntiles are padding and may hold anything"."""
    from gif_amd import _lib, ops
    lib = _lib.load()
    B, C, Co, H, W = shape
    geo = geometry(*shape, mode)
    assert geo["ntiles_pad"] > geo["ntiles"]
    ops.set_fp32_mfma_mode(mode)
    g = _rng("poison fwd", shape)
    x = torch.randn(B, C, H, W, generator=g)
    w = _window_weights(Co, C, g).cuda()
    dot = (H // 2) * (W // 2) % 128 == 0
    n_y, n_v = B * H * W * Co, lib.gif_winograd_workspace_floats(B, H, W, C)
    assert n_v == 16 * geo["ntiles_pad"] * geo["CP"]
    # mask / dot sources and y carry one more sample of room: a row index one past ntiles would land there, not outside
    src = torch.randn(2, (B + 1) * H * W * Co, generator=g).cuda()
    as_nhwc = lambda t: t[:n_y].view(B, H, W, Co).permute(0, 3, 1, 2)

    def run(xd, kind):
        V = torch.empty((n_v + GUARD,), device="cuda")
        y = torch.empty((n_y + H * W * Co,), device="cuda")
        _poison(V, n_v, kind, geo["CP"])
        _poison(y, n_y, "zero")
        fuse = ops.GradFuse(mask_src=as_nhwc(src[0]), mask_slope=0.2, mask_gain=SQRT2, want_colsum=True, dot_src=as_nhwc(src[1]) if dot else None)
        e = ops._epilogue(out_bchw=(B, Co, H, W), fuse=fuse)
        before = ops.h2_fallback_stats()
        _lib.check(_c_conv(mode, xd, w, Co, True, V, y, e), "conv3x3_winograd")
        moved = ops.h2_fallback_stats() - before
        assert _sentinels_ok(V, n_v) and _sentinels_ok(y, n_y), f"{kind}: sentinels behind V / y were written"
        return y[:n_y], fuse.colsum, fuse.dot, moved

    xd = _cl(x)
    y0, cs0, dot0, moved0 = run(xd, "zero")
    assert moved0 == 0 and torch.isfinite(y0).all() and torch.isfinite(cs0).all() and (dot0 is None or torch.isfinite(dot0).all())
    for kind in FILLS[mode]:
        y1, cs1, dot1, moved = run(xd, kind)
        assert moved == 0, f"{kind}: padding rows raised the f16x2 gate"
        assert torch.equal(_bits(y0), _bits(y1)), f"{kind}: y depends on the workspace's padding"
        assert torch.equal(_bits(cs0), _bits(cs1)), f"{kind}: the column sums depend on the workspace's padding"
        assert dot0 is None or torch.equal(_bits(dot0), _bits(dot1)), f"{kind}: the dots depend on the workspace's padding"
    if geo["gemm"] == "h2":  # the control: the same group in a real row raises the gate once (so the check above can fail)
        xb = x.clone()
        xb[:, 32:48] *= 2.0 ** -24
        _, _, _, moved = run(_cl(xb), "zero")
        assert moved == 1, "an out-of-window group in real rows must take the guarded fallback"


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", [(3, 64, 64, 10, 10), (3, 64, 64, 2, 86)], ids=["t75", "t129"])
def test_winograd_wgrad_ignores_workspace_padding(shape, mode):
    """"row padding untouched: the wgrad GEMM bounds K itself": the plane GEMMs never read a tile row >= ntiles of V or Mg."""
    from gif_amd import _lib, ops
    lib = _lib.load()
    B, Cs, Cb, H, W = shape
    ops.set_fp32_mfma_mode(mode)
    g = _rng("poison wgrad", shape)
    small, big = _cl(torch.randn(B, Cs, H, W, generator=g)), _cl(torch.randn(B, Cb, H, W, generator=g))
    RP, CP = ctypes.c_int(), ctypes.c_int()
    _lib.check(lib.gif_conv2d_wgrad_dims(ops.pad32(Cs), ops.pad32(Cb), ctypes.byref(RP), ctypes.byref(CP)), "wgrad_dims")
    nsplit = lib.gif_conv3x3_winograd_wgrad_splits(B, H, W, Cs, Cb)
    n_v, n_mg = lib.gif_winograd_workspace_floats(B, H, W, Cb), lib.gif_winograd_workspace_floats(B, H, W, Cs)
    n_ws = nsplit * 16 * RP.value * CP.value
    fn = {"native": lib.gif_conv3x3_winograd_wgrad_f32, "bf16x3": lib.gif_conv3x3_winograd_wgrad_f32x3, "f16x2": lib.gif_conv3x3_winograd_wgrad_f32h2}[mode]

    def run(kind):
        V, Mg, ws = (torch.empty((n + GUARD,), device="cuda") for n in (n_v, n_mg, n_ws))
        dw = torch.empty((Cs * Cb * 9 + GUARD,), device="cuda")
        _poison(V, n_v, kind, ops.pad32(Cb))
        _poison(Mg, n_mg, kind, ops.pad32(Cs))
        _poison(ws, n_ws, kind, CP.value)
        _poison(dw, Cs * Cb * 9, "zero")
        before = ops.h2_fallback_stats()
        _lib.check(fn(big.data_ptr(), small.data_ptr(), V.data_ptr(), Mg.data_ptr(), ws.data_ptr(), None, None, B, H, W, Cs, Cb, nsplit,
                      ops._stream()), "conv3x3_winograd_wgrad")
        _lib.check(lib.gif_winograd_unpack_wgrad_f32(ws.data_ptr(), dw.data_ptr(), nsplit, Cs, Cb, RP.value, CP.value, Cb * 9, 9, 3, 1, 1.0,
                                                     ops._stream()), "winograd_unpack_wgrad")
        moved = ops.h2_fallback_stats() - before
        assert all(_sentinels_ok(t, n) for t, n in ((V, n_v), (Mg, n_mg), (ws, n_ws), (dw, Cs * Cb * 9))), f"{kind}: sentinels were written"
        return dw[:Cs * Cb * 9], moved

    dw0, moved0 = run("zero")
    assert moved0 == 0 and torch.isfinite(dw0).all()
    for kind in FILLS[mode]:
        dw1, moved = run(kind)
        assert moved == 0, f"{kind}: padding raised the f16x2 gate"
        assert torch.equal(_bits(dw0), _bits(dw1)), f"{kind}: dW depends on the workspaces' padding"
    ref = wgrad64(small.double().cpu(), big.double().cpu())
    R = wgrad64(small.double().cpu().abs(), big.double().cpu().abs())
    _check(dw0.view(Cs, Cb, 3, 3).double().cpu(), ref, R, mode, f"poison wgrad {shape}")
