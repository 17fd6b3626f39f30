"""-m gpu: every f16 store that raises the device's overflow flag (csrc/common.h store4_flag: "unless every |v| <= 65504, NaN
included"), at its threshold, through gif_amd.ops.  The flag is the only thing between a clamped activation gradient and a training
step on wrong gradients, and a spurious flag halves the loss scale: both directions are checked at every site.

SITES (csrc/, nine calls of store4_flag):
  conv_igemm.hip conv_epilogue            every forward / data-gradient convolution kernel shares it: the gather kernels
                                          (conv_gather_mfma_glds: 256x32, 128x64, 64x64, 128x128, 256x256 tiles), the merged transposed
                                          phases (conv_gather_mfma_glds_multi), conv_halo_f16<BN, CP>; plain and fused (GradFuse) row loop
  elementwise.hip upfirdn2d_kernel        tests/test_gpu_pointwise_edges.py (test_f16_flag_threshold_generic_fir)
                  fir4x4_resample<1, 2>   FIR_SITES down2
                  fir4x4_up2_block        FIR_SITES up2_even / up2_odd (both pad parities)
                  blur4x4_tiled           FIR_SITES tiled / tiled_fuse
                  blur4x4_rows            FIR_SITES rows / rows_fuse
                  colsum_stage1<1>        bias_act_bwd, with and without gbias
                  colsum_stage1<2>        mul_reduce(scale=, want_scaled=True)
                  pack_nhwc_kernel        tests/test_gpu_pointwise_edges.py (test_f16_flag_threshold_pack_nhwc)
NOT reached: fir4x4_resample<2, 1>, the one-pixel up-by-2 kernel.  upfirdn2d_impl takes it only with GIF_FIR_BLOCK=0, which is read once per
process (a static) and honoured under GIF_EXPERIMENTAL=1 only, so it would take a child process per case; its store is the line
fir4x4_resample<1, 2> runs, and tests/test_gpu_round6.py holds its f16 output to the block kernel's bits (in children).

conv_halo_f16 instantiations: conv_route.h push_halo takes BN = 32 | 64 from the packed output rows and CP = 32 | 64 from the packed
contraction channels, under halo_weight_bytes = taps * BN * CP * 2 <= 36 864.  All four are reachable: <32,32> (halo_o29, fuse_halo_*),
<64,32> (halo_16), <32,64> (halo_c40_o32) with nine taps; <64,64> with at most four taps (73 728 B at nine): the 1x1 row halo_1x1 here, and
the 2x2 / 2x1 / 1x2 / 1x1 output-parity phases of a stride-2 data gradient (tconv_halo_phases runs <32,32> on them).  None is unreachable.

CONSTRUCTION.  Zero background, one non-zero operand entry per operand (a weight tensor with one tap of 2.0 and one hot input element; a
4x4 FIR kernel with one tap of 2.0; gain 2, slope 0.5, scale 2 at the elementwise sites), so exactly ONE output element is non-zero,
every product is exact and the expected output is a bit pattern: clamp(reference, +-65504) cast to half, NaN kept.  The reference is the
fp64 operation (F.conv2d / F.conv_transpose2d / test_gpu_conv_routes.fir64 / the elementwise formula) on the unit hot element, times the
hot value (one exact product: linear), plus the residual; each case asserts that the reference has its single non-zero where the case
says.  Value classes of the hot element (the operands are halfs: 32752 * 2 = 65504, 32768 * 2 = 65536):
  max  65504 exactly                      no flag, stored 65504              (and -65504)
  next 65504 + 2^-8 (residual 2^-8)       the next float32: flag, stored 65504 (and mirrored)
  pow2 65536                              flag, stored 65504                 (and mirrored)
  +inf / -inf / nan through the residual  flag; stored +-65504 / NaN         (elementwise sites: through the operand, which has no
                                                                             residual; they have no `next`: a half times 1 or 2 is a half)
Fused rows: the mask multiplies after the contraction, so the hot operand is halved where the mask factor is 2 (16376 * 2 * 2 = 65504) —
the flag follows the stored value, not the accumulator; the fused column sums are the sums BEFORE the clamp (65536 stays 65536) and the dot
is the contraction before residual and mask.
Per case: the flag; the whole output bit-equal; the same launch with watching off raises nothing; a raised flag survives a clean launch
until it is cleared.

RANDOM BACKGROUND (test_random_background_*): one row per conv family and FIR kernel at odd sizes; fp64 reference from the half-rounded
operands, operands rescaled by powers of two (asserted exact and finite in half) until max |ref| <= 0.97 * 65504 (flag 0) and until
max |ref| >= 1.03 * 65504 (flag 1; output = clamped reference within TOL["f16"] / TOL["fir16"] of test_gpu_conv_routes.py).  The 3 % margins
are asserted on the reference alone; fp32 accumulation over K <= 2304 terms is orders of magnitude below them."""
import math
import zlib
from typing import NamedTuple

import pytest
import torch
import torch.nn.functional as F

from gpu_util import Flag
from test_gpu_conv_routes import _check, cpad, fir64

pytestmark = pytest.mark.gpu

H16 = torch.float16
CL = torch.channels_last
LIM = 65504.0
INF, NAN = math.inf, math.nan
F16_FAMILY = 6  # gif_prof_read: the f16 forward / data-gradient kernels


class Cls(NamedTuple):
    name: str
    hot: float       # the hot operand; the site's one product doubles it
    res: float       # added at the hot output element (residual), 0: none
    flag: float
    stored: float


CLASSES = [Cls("max", 32752.0, 0.0, 0.0, LIM), Cls("next", 32752.0, 2.0 ** -8, 1.0, LIM), Cls("pow2", 32768.0, 0.0, 1.0, LIM),
           Cls("-max", -32752.0, 0.0, 0.0, -LIM), Cls("-next", -32752.0, -2.0 ** -8, 1.0, -LIM), Cls("-pow2", -32768.0, 0.0, 1.0, -LIM),
           Cls("+inf", 1.0, INF, 1.0, LIM), Cls("-inf", 1.0, -INF, 1.0, -LIM), Cls("nan", 1.0, NAN, 1.0, NAN)]
# sites without a residual: the non-finite value is the operand itself; no `next`
EW_CLASSES = [c for c in CLASSES if c.res == 0.0] + [Cls("+inf", INF, 0.0, 1.0, LIM), Cls("-inf", -INF, 0.0, 1.0, -LIM), Cls("nan", NAN, 0.0, 1.0, NAN)]


def test_the_threshold_constants():
    """The classes are what the docstring says they are, in float32 and in half."""
    nxt = torch.tensor(LIM).nextafter(torch.tensor(INF)).item()
    assert nxt == LIM + 2.0 ** -8 and torch.tensor(32752.0 * 2 + 2.0 ** -8, dtype=torch.float32).item() == nxt
    for v in (32752.0, 32768.0, 16376.0, 16384.0, 2.0 ** -8, LIM):
        assert torch.tensor(v).to(H16).item() == v
    assert torch.tensor(65536.0).to(H16).isinf() and torch.finfo(H16).max == LIM


def _bits(t):
    """int16 view of a half tensor in NCHW order, -0 as +0 and NaN as one pattern"""
    t = torch.where(t.isnan(), torch.full_like(t, NAN), t + 0.0)
    return t.contiguous().view(torch.int16)


def _assert_stored(y, ref, what):
    """y (device half) is clamp(ref, +-65504) as halfs, bit for bit; ref: fp64 on the device, before the clamp"""
    assert y.dtype == H16 and y.shape == ref.shape, (what, y.dtype, y.shape, ref.shape)
    want = ref.clamp(-LIM, LIM).to(H16)  # (clamp keeps NaN)
    bad = _bits(y) != _bits(want)
    if bad.any():
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ; first at {i}: stored {y[i].item()} expected {want[i].item()}")


def _same(a, b):
    return bool(((a == b) | (a.isnan() & b.isnan())).all())


def _want_flag(ref):
    return 0.0 if bool((ref.abs() <= LIM).all()) else 1.0  # (false for a NaN, like the kernel's comparison)


def _run_classes(fl, classes, launch, expect, what, check_aux=None):
    """launch(cls) -> (y, aux); expect(cls) -> fp64 reference before the clamp (device).  The four assertions of the module docstring."""
    clean = flagged = None
    for c in classes:
        ref = expect(c)
        assert _want_flag(ref) == c.flag, f"{what} {c.name}: the construction does not give the class (max |ref| {ref.abs().max().item()})"
        clamped = ref.clamp(-LIM, LIM)
        assert bool(clamped.isnan().any()) if math.isnan(c.stored) else bool((clamped == c.stored).any()), f"{what} {c.name}: no element stores {c.stored}"
        found, (y, aux) = fl.after(lambda: launch(c))
        print(f"\n[flag site] {what} {c.name}: flag {found}")
        assert found == c.flag, f"{what} {c.name}: flag {found}, expected {c.flag}"
        _assert_stored(y, ref, f"{what} {c.name}")
        if check_aux is not None:
            check_aux(c, aux, ref)
        found, (y2, _) = fl.after(lambda: launch(c), watch=False)
        assert found == 0.0, f"{what} {c.name}: flagged with watching off"
        _assert_stored(y2, ref, f"{what} {c.name} (watching off)")
        if c.flag and flagged is None:
            flagged = c
        if not c.flag and clean is None:
            clean = c
    fl.clear()
    launch(flagged)
    launch(clean)
    assert fl.read() == 1.0, f"{what}: a clean launch after the {flagged.name} launch lowered the flag"
    found, _ = fl.after(lambda: launch(clean))
    assert found == 0.0, f"{what}: the flag was not cleared"


def _hot_at(ref, pos, what):
    nz = ref.nonzero()
    assert nz.shape[0] == 1 and tuple(int(v) for v in nz[0]) == tuple(pos), f"{what}: the unit reference is non-zero at {nz.tolist()}, not only at {pos}"


def _positions(B, C, Cr, H, W, big=False, parity=False):
    """Hot output elements (b, c, y, x) of a [B, C, H, W] output with Cr real channels: the first element, the last valid one (the tail of a
    partial tile / patch / strip / block, the last real channel), the four lanes of a channel quad (first: lane 0; lane1..3 at a middle
    pixel), parity: a pixel of the (odd, odd) output phase of a stride-2 data gradient."""
    q = 4 if Cr >= 8 else 0
    my, mx = (H // 2) | 1, (W // 2) & ~1
    out = [("first", (0, 0, 0, 0)), ("last", (B - 1, Cr - 1, H - 1, W - 1)), ("lane1", (B - 1, q + 1, min(my, H - 1), mx))]
    if not big:
        out += [("lane2", (0, q + 2, min(my, H - 1), mx)), ("lane3", (B - 1, q + 3, 0, W - 1))]
    if parity:
        out.append(("odd_odd", (0, Cr - 1, (H - 2) | 1, (W - 2) | 1)))
    return [(n, p) for n, p in out if p[1] < Cr]


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. convolutions.  Shapes: test_gpu_conv_routes.ROWS of the f16 mode by name (their tile / merge claims are asserted on the CPU by
# tests/test_conv_route.py), and the rows added here with the conv_route.h rule that places them.
# ---------------------------------------------------------------------------------------------------------------------------------
class ConvSite(NamedTuple):
    name: str
    op: str             # fwd | dgrad
    shape: tuple        # the FORWARD conv (B, Cin, Cout, K, stride, pad, H, W), as in test_gpu_conv_routes.Row
    halo: object = None  # what gif_conv2d_f16_halo_eligible says about the op's contraction / output channels and output grid (None: not asked)
    fuse: str = ""      # "" | mask (GradFuse mask_src + colsum) | dot (+ dot_src)
    big: bool = False   # three positions instead of five: the reference convolution is the cost


CONV_SITES = [
    # ---- gather kernels (route_phase): every tile of the f16 ladder
    ConvSite("halo_15", "fwd", (2, 32, 64, 3, 1, 1, 15, 17), halo=False),            # ROWS: Hp 15 < 16 -> gather, BN 64: 128x64 tiles, M 510
    ConvSite("halo_15_dgrad", "dgrad", (2, 32, 64, 3, 1, 1, 15, 17), halo=False),    # its data gradient: 32 outputs -> 256x32 tiles, M % 256 = 254
    ConvSite("gather_o29", "fwd", (2, 32, 29, 3, 1, 1, 15, 17), halo=False),         # halo_15 with 29 outputs (RP 32: 256x32 tiles): last real channel 28
    ConvSite("f16_t128_383", "fwd", (1, 72, 72, 1, 1, 0, 127, 386), big=True),       # ROWS: 64x64 tiles (M 49022 = 765 * 64 + 62)
    ConvSite("f16_t128_384", "fwd", (1, 72, 72, 1, 1, 0, 127, 387), big=True),       # ROWS: 128x128 tiles (M 49149 % 128 = 125)
    ConvSite("f16_t256_512", "fwd", (1, 72, 256, 1, 1, 0, 255, 514), big=True),      # ROWS: 256x256 tiles on 8 waves (M 131070 % 256 = 254)
    # ---- conv_halo_f16<BN, CP>
    ConvSite("halo_16", "fwd", (2, 32, 64, 3, 1, 1, 16, 16), halo=True),             # ROWS: <64, 32>, whole patches
    ConvSite("halo_c40_o32", "fwd", (1, 40, 32, 3, 1, 1, 17, 20), halo=True),        # ROWS: <32, 64>, 17 x 20: patches overhang on both axes
    ConvSite("halo_o29", "fwd", (1, 32, 29, 3, 1, 1, 17, 20), halo=True),            # 32 -> 29 (RP 32, CP 32): <32, 32>, last real channel 28 of 32
    ConvSite("halo_1x1", "fwd", (1, 40, 40, 1, 1, 0, 17, 20), halo=True),            # CP 64, RP 64, one tap: 8192 B <= 36 864 -> <64, 64>
    ConvSite("halo_16_dgrad", "dgrad", (2, 64, 32, 3, 1, 1, 16, 16), halo=True),     # data gradient on the halo kernel (taps run backwards: ddy -1)
    # ---- transposed stride-2 data gradients
    ConvSite("f16_tconv_small", "dgrad", (1, 72, 33, 3, 2, 0, 311, 627), big=True),      # ROWS: four phases merged into one launch
    ConvSite("f16_tconv_not_small", "dgrad", (1, 72, 33, 3, 2, 0, 311, 629), big=True),  # ROWS: one launch per phase
    ConvSite("tconv_halo_phases", "dgrad", (2, 29, 32, 3, 2, 0, 33, 35)),            # 29 outputs (RP 32: not `wide`, never merged), phases of 17 x 18
                                                                                      #   .. 16 x 17 pixels with 2x2 .. 1x1 taps -> four halo launches
    # ---- the fused (GradFuse) row loop of conv_epilogue; stride-1 data gradients, the op that carries the fusions in functional.py
    ConvSite("fuse_gather_mask", "dgrad", (2, 32, 64, 3, 1, 1, 15, 17), halo=False, fuse="mask"),  # 256x32 tiles, 255 pixels: no dot
    ConvSite("fuse_gather_dot", "dgrad", (1, 72, 32, 3, 1, 1, 32, 32), halo=False, fuse="dot"),    # 72 outputs (RP 128 > 64), M 1024: 64x64 tiles
    ConvSite("fuse_halo_mask", "dgrad", (1, 29, 32, 3, 1, 1, 17, 20), halo=True, fuse="mask"),     # partial sums of overhanging patches
    ConvSite("fuse_halo_dot", "dgrad", (2, 24, 16, 3, 1, 1, 32, 32), halo=True, fuse="dot"),       # H * W = 1024, Hp % 16 == 0: the halo kernel's dot
]


def _conv_geometry(site):
    """(contraction channels, output channels, input grid, output grid) of the op"""
    B, Ci, Co, K, s, p, H, W = site.shape
    small = ((H + 2 * p - K) // s + 1, (W + 2 * p - K) // s + 1)
    return (Ci, Co, (H, W), small) if site.op == "fwd" else (Co, Ci, small, (H, W))


def _conv64(site, x, w):
    B, Ci, Co, K, s, p, H, W = site.shape
    if site.op == "fwd":
        return F.conv2d(x, w, stride=s, padding=p)
    Hs, Ws = x.shape[2:]
    opad = (H - ((Hs - 1) * s + K - 2 * p), W - ((Ws - 1) * s + K - 2 * p))
    return F.conv_transpose2d(x, w, stride=s, padding=p, output_padding=opad)


def _conv_source(site, oy, ox):
    """A tap (ky, kx) and the input pixel that reach output pixel (oy, ox) through it; the corner taps first."""
    B, Ci, Co, K, s, p, H, W = site.shape
    _, _, (Hi, Wi), _ = _conv_geometry(site)
    order = [K - 1, 0] + list(range(1, K - 1)) if K > 1 else [0]

    def axis(o, n_in, rev):
        for k in (order[::-1] if rev else order):
            if site.op == "fwd":
                i = o * s - p + k
            else:
                if (o + p - k) % s:
                    continue
                i = (o + p - k) // s
            if 0 <= i < n_in:
                return k, i
        raise AssertionError((site.name, o))

    ky, iy = axis(oy, Hi, False)
    kx, ix = axis(ox, Wi, True)
    return ky, kx, iy, ix


def _assert_conv_route(site, run):
    """One op in the f16 family, and the halo predicate (test_gpu_conv_routes.test_conv_route_vs_fp64's assertions)."""
    from gif_amd import _lib, ops
    B, Ci, Co, K, s, p, H, W = site.shape
    cin, cout, _, (Ho, Wo) = _conv_geometry(site)
    try:
        ops.prof_enable(True)
        for fam in range(18):
            ops.prof_read(fam)
        run()
        torch.cuda.synchronize()
        ran = {fam: n for fam in range(18) for n in [ops.prof_read(fam)[2]] if n}
    finally:
        ops.prof_enable(False)
    assert ran == {F16_FAMILY: 1}, f"{site.name}: expected one op in family {F16_FAMILY}, got {ran}"
    if site.halo is not None:
        # stride-1 ops: the data gradient is a unit-stride gather over the same tap grid with the channel roles swapped
        assert s == 1
        ok = bool(_lib.load().gif_conv2d_f16_halo_eligible(cpad(cin, True), cpad(cout, True), K, K, 1, Ho, Wo))
        if site.fuse == "dot":
            ok = ok and Ho % 16 == 0 and Wo % 16 == 0  # conv_route.h halo_eligible: the dot needs whole patches
        assert ok == site.halo, site.name


CONV_CASES = [pytest.param(site, pn, pos, id=f"{site.name}-{pn}") for site in CONV_SITES
              for pn, pos in _positions(site.shape[0], cpad(_conv_geometry(site)[1], True), _conv_geometry(site)[1], *_conv_geometry(site)[3],
                                        big=site.big, parity=site.shape[4] == 2)]
CONV_CASES += [pytest.param(site, "neg_mask", (site.shape[0] - 1, 2, 3, 5), id=f"{site.name}-neg_mask") for site in CONV_SITES if site.fuse]


@pytest.mark.parametrize("site,pname,pos", CONV_CASES)
def test_conv_store_at_the_threshold(site, pname, pos):
    from gif_amd import ops
    B, Ci, Co, K, s, p, H, W = site.shape
    cin, cout, (Hi, Wi), (Ho, Wo) = _conv_geometry(site)
    cin_p, cout_p = cpad(cin, True), cpad(cout, True)
    b, c, oy, ox = pos
    ky, kx, iy, ix = _conv_source(site, oy, ox)
    ci = (cin - 1) if pname == "last" else (c * 5 + 3) % cin  # the contraction channel of the hot product (last: the channel tail)
    w = torch.zeros(Co, Ci, K, K)
    w[(c, ci) if site.op == "fwd" else (ci, c)][ky, kx] = 2.0
    spec = ops.ConvSpec(K, K, s, p)
    # mask factor at the hot element: gain 2 where mask_src > 0, gain * slope = 1 elsewhere
    g = torch.Generator().manual_seed(zlib.crc32(repr((site.name, pname)).encode()))
    mask = dot_src = None
    factor = 1.0
    if site.fuse:
        mask = torch.where(torch.rand(B, cout_p, Ho, Wo, generator=g) < 0.5, -1.0, 1.0)
        mask[pos] = -1.0 if pname == "neg_mask" else 1.0
        factor = 1.0 if pname == "neg_mask" else 2.0
        if site.fuse == "dot":
            dot_src = torch.randint(1, 4, (B, cout_p, Ho, Wo), generator=g).float() * torch.where(torch.rand(B, cout_p, Ho, Wo, generator=g) < 0.5, -1.0, 1.0)
    # the unit reference: fp64 convolution of the one-hot operands
    x1 = torch.zeros(B, cin, Hi, Wi, dtype=torch.float64)
    x1[b, ci, iy, ix] = 1.0
    unit = F.pad(_conv64(site, x1, w.double()), (0, 0, 0, 0, 0, cout_p - cout))
    _hot_at(unit, pos, site.name)
    assert unit[pos].item() == 2.0
    unit = unit.cuda()
    wd = w.cuda()
    maskd = None if mask is None else mask.to(H16).cuda().contiguous(memory_format=CL)
    dotd = None if dot_src is None else dot_src.to(H16).cuda().contiguous(memory_format=CL)
    fd = None if mask is None else (2.0 * torch.where(mask > 0, 1.0, 0.5)).double().cuda()

    xd = torch.zeros(B, cin_p, Hi, Wi, dtype=H16, device="cuda").contiguous(memory_format=CL)
    resd = torch.zeros(B, cout_p, Ho, Wo, dtype=H16, device="cuda").contiguous(memory_format=CL)

    def launch(c_):
        hot = c_.hot / factor
        assert torch.tensor(hot).to(H16).item() == hot
        xd[b, ci, iy, ix] = hot
        resd[pos] = c_.res
        epi = {} if c_.res == 0.0 else {"residual": resd}  # (no residual operand where the class has none: the plain epilogue)
        fuse = None
        if site.fuse:
            fuse = ops.GradFuse(mask_src=maskd, mask_slope=0.5, mask_gain=2.0, want_colsum=True, dot_src=dotd)
            epi["fuse"] = fuse
        y = ops.conv_fwd(xd, wd, spec, **epi) if site.op == "fwd" else ops.conv_bwd_data(xd, wd, spec, (H, W), **epi)
        return y, fuse

    def expect(c_):
        ref = unit * (c_.hot / factor)
        if c_.res != 0.0:
            ref[pos] += c_.res
        return ref if fd is None else ref * fd

    def check_aux(c_, fuse, ref):
        if fuse is None:
            return
        # the column sums are taken BEFORE the clamp (one non-zero term: exact)
        assert _same(fuse.colsum.double(), ref.sum((0, 2, 3))), f"{site.name} {c_.name}: colsum {fuse.colsum[c].item()} vs {ref.sum((0, 2, 3))[c].item()}"
        if dotd is not None:  # contraction * dot_src, before residual and mask
            want = (unit * (c_.hot / factor) * dotd.double()).sum((2, 3))
            assert _same(fuse.dot.double(), want), f"{site.name} {c_.name}: dot {fuse.dot[b, c].item()} vs {want[b, c].item()}"

    fl = Flag()
    try:
        _assert_conv_route(site, lambda: launch(CLASSES[0]))
        _run_classes(fl, CLASSES, launch, expect, f"{site.name} {pname}", check_aux)
    finally:
        fl.restore()


OUT_F32 = [("halo", (2, 8, 4, 1, 1, 0, 32, 32), True), ("gather", (2, 8, 4, 1, 1, 0, 15, 17), False)]


@pytest.mark.parametrize("name,shape,halo", OUT_F32, ids=[r[0] for r in OUT_F32])
def test_out_f32_is_the_negative_control(name, shape, halo):
    """ToRGB's form (1x1, out_f32=True): a result of 102 400 is stored exactly as fp32 and raises nothing, on either kernel; the same launch
    with a half output raises the flag and stores 65504."""
    from gif_amd import _lib, ops
    B, Ci, Co, K, s, p, H, W = shape
    assert bool(_lib.load().gif_conv2d_f16_halo_eligible(cpad(Ci, True), cpad(Co, True), K, K, s, H, W)) == halo
    x = torch.zeros(B, Ci, H, W, dtype=H16)
    w = torch.zeros(Co, Ci, K, K)
    for b, c, ci, y_, x_ in ((0, 0, 0, 0, 0), (B - 1, Co - 1, Ci - 1, H - 1, W - 1)):
        x[b, ci, y_, x_] = 51200.0
        w[c, ci, 0, 0] = 2.0
    ref = F.pad(F.conv2d(x.double(), w.double()), (0, 0, 0, 0, 0, cpad(Co, True) - Co)).cuda()
    assert ref.max().item() == 102400.0 and (ref != 0).sum().item() == 2
    xd, wd, spec = x.cuda().contiguous(memory_format=CL), w.cuda(), ops.ConvSpec(K, K, s, p)
    fl = Flag()
    try:
        found, y = fl.after(lambda: ops.conv_fwd(xd, wd, spec, out_f32=True))
        assert found == 0.0, "an fp32 store raised the f16 flag"
        assert y.dtype == torch.float32 and torch.equal(y.double(), ref)
        found, y = fl.after(lambda: ops.conv_fwd(xd, wd, spec))
        assert found == 1.0
        _assert_stored(y, ref, f"out_f32 {name}: the half output")
    finally:
        fl.restore()


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. FIR kernels (csrc/elementwise.hip upfirdn2d_impl)
# ---------------------------------------------------------------------------------------------------------------------------------
class FirSite(NamedTuple):
    name: str
    kernel: str     # what upfirdn2d_impl launches (fir_kernel restates its thresholds)
    dims: tuple     # B, C, H, W, up, down, pad0, (Ho, Wo): test_gpu_conv_routes.FirRow's fields
    fuse: bool = False
    big: bool = False


FIR_SITES = [
    FirSite("tiled", "blur4x4_tiled", (2, 8, 38, 42, 1, 1, 1, (37, 41))),               # FIR_ROWS blur_tiled_small: 2 x 4 tiles, Ho odd, Wo % 4 = 1
    FirSite("tiled_fuse", "blur4x4_tiled", (2, 8, 38, 42, 1, 1, 1, (37, 41)), fuse=True),
    # rows kernel: B * cdiv(Ho, 16) * cdiv(Wo, 4) * C / 4 = 2 * 16 * 64 * 64 = 131072 with C % 8 == 0 (the FIR_ROWS rows kernel shapes have 4
    # channels: fp32 only); Ho % 16 = 15, Wo % 4 = 3: the last strip is partial on both axes
    FirSite("rows", "blur4x4_rows", (2, 256, 256, 256, 1, 1, 1, (255, 255)), big=True),
    FirSite("rows_fuse", "blur4x4_rows", (2, 256, 256, 256, 1, 1, 1, (255, 255)), fuse=True, big=True),
    FirSite("down2", "fir4x4_resample<1,2>", (2, 8, 37, 41, 1, 2, 1, (18, 20))),        # FIR_ROWS down2
    FirSite("up2_even", "fir4x4_up2_block", (3, 8, 37, 29, 2, 1, 2, (74, 58))),         # FIR_ROWS up2_even: pad0 2
    FirSite("up2_odd", "fir4x4_up2_block", (3, 8, 37, 29, 2, 1, 1, (73, 57))),          # FIR_ROWS up2_odd: the other block parity, odd Ho / Wo
]


def fir_kernel(B, C, H, W, up, down, pad0, out, KH=4, KW=4):
    """upfirdn2d_impl's choice, restated"""
    Ho, Wo = out
    cdiv = lambda a, b: (a + b - 1) // b
    if up == 1 and down == 1 and (KH, KW) == (4, 4):
        return "blur4x4_rows" if B * cdiv(Ho, 16) * cdiv(Wo, 4) * (C // 4) >= 256 * 256 * 2 else "blur4x4_tiled"
    if (KH, KW) == (4, 4) and B * Ho <= 65535 and (up, down) in ((1, 2), (2, 1)):
        return "fir4x4_up2_block" if up == 2 else "fir4x4_resample<1,2>"  # (up 2: the block kernel unless GIF_FIR_BLOCK=0)
    return "upfirdn2d_kernel"


def _fir_source(dims, oy, ox):
    """A tap (a, b) of the flipped kernel and the input pixel it reads for output (oy, ox): u = o * down + a - pad0 = up * i"""
    B, C, H, W, up, down, pad0, _ = dims

    def axis(o, n, order):
        for a in order:
            u = o * down + a - pad0
            if u >= 0 and u % up == 0 and u // up < n:
                return a, u // up
        raise AssertionError((dims, o))

    a, iy = axis(oy, H, (3, 0, 1, 2))
    b_, ix = axis(ox, W, (0, 3, 2, 1))
    return a, b_, iy, ix


FIR_CASES = [pytest.param(site, pn, pos, id=f"{site.name}-{pn}") for site in FIR_SITES
             for pn, pos in _positions(site.dims[0], site.dims[1], site.dims[1], *site.dims[7], big=site.big)]
FIR_CASES += [pytest.param(site, "neg_mask", (site.dims[0] - 1, 2, 3, 5), id=f"{site.name}-neg_mask") for site in FIR_SITES if site.fuse]


@pytest.mark.parametrize("site,pname,pos", FIR_CASES)
def test_fir_store_at_the_threshold(site, pname, pos):
    from gif_amd import _lib, ops
    B, C, H, W, up, down, pad0, (Ho, Wo) = site.dims
    assert fir_kernel(*site.dims) == site.kernel and C % 8 == 0
    assert _lib.knob("GIF_FIR_BLOCK", "1") != "0", "this process runs the A/B kernel for up 2"
    assert not site.fuse or ops.fir_fusable(C, up, down, (4, 4), H16)
    b, c, oy, ox = pos
    a, b_, iy, ix = _fir_source(site.dims, oy, ox)
    k = torch.zeros(4, 4)
    k[3 - a, 3 - b_] = 2.0  # (flip=True: the kernel reads k[3 - a][3 - b] at tap (a, b))
    # the unit reference, fp64 on the device (the rows kernel's shape has 33 M elements; fir64 is slices and adds, no kernel of this project)
    x1 = torch.zeros(B, C, H, W, dtype=torch.float64, device="cuda")
    x1[b, c, iy, ix] = 1.0
    unit = fir64(x1, k.double().cuda(), up, down, pad0, (Ho, Wo))
    del x1
    _hot_at(unit, pos, site.name)
    assert unit[pos].item() == 2.0
    g = torch.Generator().manual_seed(zlib.crc32(repr((site.name, pname)).encode()))
    maskd = fd = None
    factor = 1.0
    if site.fuse:
        mask = torch.where(torch.rand(B, C, Ho, Wo, generator=g) < 0.5, -1.0, 1.0)
        mask[pos] = -1.0 if pname == "neg_mask" else 1.0
        factor = 1.0 if pname == "neg_mask" else 2.0
        maskd = mask.to(H16).cuda().contiguous(memory_format=CL)
        fd = 2.0 * torch.where(maskd > 0, 1.0, 0.5).double()
    kd = k.cuda()
    xd = torch.zeros(B, C, H, W, dtype=H16, device="cuda").contiguous(memory_format=CL)
    resd = torch.zeros(B, C, Ho, Wo, dtype=H16, device="cuda").contiguous(memory_format=CL)

    def launch(c_):
        xd[b, c, iy, ix] = c_.hot / factor
        resd[pos] = c_.res
        kw = {} if c_.res == 0.0 else {"residual": resd}
        fuse = None
        if site.fuse:
            fuse = ops.GradFuse(mask_src=maskd, mask_slope=0.5, mask_gain=2.0, want_colsum=True)
            kw["fuse"] = fuse
        return ops.upfirdn2d(xd, kd, up, down, pad0, (Ho, Wo), **kw), fuse

    def expect(c_):
        ref = unit * (c_.hot / factor)
        if c_.res != 0.0:
            ref[pos] += c_.res
        return ref if fd is None else ref * fd

    def check_aux(c_, fuse, ref):
        if fuse is not None:  # the sums before the clamp; one non-zero term: exact
            assert _same(fuse.colsum.double(), ref.sum((0, 2, 3))), f"{site.name} {c_.name}: colsum {fuse.colsum[c].item()}"

    fl = Flag()
    try:
        _run_classes(fl, CLASSES, launch, expect, f"{site.name} {pname}", check_aux)
    finally:
        fl.restore()


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the colsum_stage1 sites: bias_act_bwd (MODE 1) and mul_reduce's scaled output (MODE 2).  [2, 24, 37, 37]: C4 = 6 leaves 4 of the 256
# lanes without a row (R = 42), bias_act_bwd runs 5 blocks of 548 rows (the last one 546), mul_reduce 11 chunks of 125 rows (the last 119)
# per sample; [2, 8, 37, 37]: C4 = 2, two blocks.  last = the last row of the last block of the last sample.
# ---------------------------------------------------------------------------------------------------------------------------------
EW_SHAPES = [(2, 24, 37, 37), (2, 8, 37, 37)]
EW_CASES = [pytest.param(shape, pn, pos, id=f"c{shape[1]}-{pn}") for shape in EW_SHAPES for pn, pos in _positions(*shape[:2], shape[1], *shape[2:])]


@pytest.mark.parametrize("want_gbias", [True, False], ids=["gbias", "no_gbias"])
@pytest.mark.parametrize("neg", [False, True], ids=["y_pos", "y_neg"])
@pytest.mark.parametrize("shape,pname,pos", EW_CASES)
def test_bias_act_bwd_store_at_the_threshold(shape, pname, pos, neg, want_gbias):
    """gx = gy * gain * (y > 0 ? 1 : slope) with gain 2, slope 0.5: the factor is 2 where y > 0 and 1 elsewhere.  y_neg: gy itself is the
    stored value there, and 65536 is no half: that side has max and the non-finite classes only."""
    from gif_amd import ops
    B, C, H, W = shape
    g = torch.Generator().manual_seed(zlib.crc32(repr((shape, pname, neg)).encode()))
    y = torch.where(torch.rand(B, C, H, W, generator=g) < 0.5, -1.0, 1.0)
    y[pos] = -1.0 if neg else 1.0
    factor = 1.0 if neg else 2.0
    yd = y.to(H16).cuda().contiguous(memory_format=CL)
    fd = 2.0 * torch.where(yd > 0, 1.0, 0.5).double()
    gyd = torch.zeros(B, C, H, W, dtype=H16, device="cuda").contiguous(memory_format=CL)
    # y_neg: the operand is the stored value; 65536 cannot be a half operand, so pow2 leaves (inf covers "above the limit")
    classes = [c_ for c_ in EW_CLASSES if not (neg and abs(c_.hot) == 32768.0)]

    def hot(c_):
        return c_.hot * 2.0 / factor

    def launch(c_):
        assert not math.isfinite(hot(c_)) or torch.tensor(hot(c_)).to(H16).item() == hot(c_)
        gyd[pos] = hot(c_)
        return ops.bias_act_bwd(gyd, yd, want_gbias, slope=0.5, gain=2.0)

    def expect(c_):
        ref = torch.zeros(B, C, H, W, dtype=torch.float64, device="cuda")
        ref[pos] = hot(c_)
        return ref * fd

    def check_aux(c_, gbias, ref):
        assert (gbias is not None) == want_gbias
        if want_gbias:  # the bias gradient sums the values before the clamp
            assert _same(gbias.double(), ref.sum((0, 2, 3))), f"bias_act_bwd {c_.name}: gbias {gbias[pos[1]].item()}"

    fl = Flag()
    try:
        _run_classes(fl, classes, launch, expect, f"bias_act_bwd {shape} {pname}", check_aux)
    finally:
        fl.restore()


@pytest.mark.parametrize("shape,pname,pos", EW_CASES)
def test_mul_reduce_scaled_store_at_the_threshold(shape, pname, pos):
    """scaled = scale[b, c] * a with power-of-two scales (2 at the hot sample and channel); out = sum_hw a * b is fp32 and not clamped."""
    from gif_amd import ops
    B, C, H, W = shape
    g = torch.Generator().manual_seed(zlib.crc32(repr((shape, pname)).encode()))
    scale = 2.0 ** torch.randint(-2, 2, (B, C), generator=g).float()
    scale[pos[0], pos[1]] = 2.0
    bt = torch.randint(1, 4, (B, C, H, W), generator=g).float()
    sd, bd = scale.cuda(), bt.to(H16).cuda().contiguous(memory_format=CL)
    ad = torch.zeros(B, C, H, W, dtype=H16, device="cuda").contiguous(memory_format=CL)

    def launch(c_):
        ad[pos] = c_.hot
        out, scaled = ops.mul_reduce(ad, bd, scale=sd, want_scaled=True)
        return scaled, out

    def expect(c_):
        ref = torch.zeros(B, C, H, W, dtype=torch.float64, device="cuda")
        ref[pos] = c_.hot
        return ref * sd.double()[:, :, None, None]

    def check_aux(c_, out, ref):
        want = torch.zeros(B, C, dtype=torch.float64, device="cuda")
        want[pos[0], pos[1]] = c_.hot * bt[pos].item()
        assert _same(out.double(), want), f"mul_reduce {c_.name}: out {out[pos[0], pos[1]].item()}"

    fl = Flag()
    try:
        _run_classes(fl, EW_CLASSES, launch, expect, f"mul_reduce {shape} {pname}", check_aux)
    finally:
        fl.restore()


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. random background: no false positive below the limit, no miss above it, anywhere in the tensor
# ---------------------------------------------------------------------------------------------------------------------------------
def _r16(t):
    return t.to(H16).float()


def _pow2_scales(peak):
    """(k_under, k_over): the largest power of two with peak * 2^k <= 0.97 * 65504 and the smallest with peak * 2^k >= 1.03 * 65504"""
    ku = math.floor(math.log2(0.97 * LIM / peak))
    ko = math.ceil(math.log2(1.03 * LIM / peak))
    assert peak * 2.0 ** ku <= 0.97 * LIM and peak * 2.0 ** ko >= 1.03 * LIM and ko > ku
    return ku, ko


def _scaled16(t, k, what):
    """t * 2^k, exactly, as finite halfs (t: half-representable fp32)"""
    s = t * 2.0 ** k
    h = s.to(H16)
    assert torch.isfinite(h).all() and torch.equal(h.float(), s), f"{what}: scaling by 2^{k} leaves the half format"
    return h


RANDOM_CONV = [
    ConvSite("rand_gather", "fwd", (2, 32, 64, 3, 1, 1, 15, 17), halo=False),              # K = 288, 128x64 tiles
    ConvSite("rand_gather_c256", "dgrad", (1, 29, 256, 3, 1, 1, 15, 17), halo=False),      # K = 2304 (256 contraction channels), 29 real outputs
    ConvSite("rand_halo", "fwd", (1, 40, 29, 3, 1, 1, 17, 20), halo=True),                 # <32, 64>, overhanging patches, 29 real channels
    ConvSite("rand_tconv_merged", "dgrad", (2, 72, 33, 3, 2, 0, 33, 35)),                  # 72 outputs (wide), every phase small: merged 64x64
    ConvSite("rand_tconv_halo_phases", "dgrad", (2, 29, 32, 3, 2, 0, 33, 35)),             # one halo launch per output-parity phase
    ConvSite("rand_fuse_mask", "dgrad", (2, 32, 64, 3, 1, 1, 15, 17), halo=False, fuse="mask"),
]


@pytest.mark.parametrize("site", RANDOM_CONV, ids=[s.name for s in RANDOM_CONV])
def test_random_background_conv(site):
    from gif_amd import ops
    B, Ci, Co, K, s, p, H, W = site.shape
    cin, cout, (Hi, Wi), (Ho, Wo) = _conv_geometry(site)
    cin_p, cout_p = cpad(cin, True), cpad(cout, True)
    g = torch.Generator().manual_seed(zlib.crc32(site.name.encode()))
    x = _r16(torch.randn(B, cin, Hi, Wi, generator=g))
    w = _r16(torch.randn(Co, Ci, K, K, generator=g) / math.sqrt(cin * K * K))
    spec = ops.ConvSpec(K, K, s, p)
    f = mask = None
    if site.fuse:
        mask = _r16(torch.randn(B, cout_p, Ho, Wo, generator=g))
        f = 2 ** 0.5 * torch.where(mask > 0, 1.0, 0.2).double()
        maskd = mask.to(H16).cuda().contiguous(memory_format=CL)

    def reference(xs, ws):
        z, R = _conv64(site, xs.double(), ws.double()), _conv64(site, xs.double().abs(), ws.double().abs())
        z, R = F.pad(z, (0, 0, 0, 0, 0, cout_p - cout)), F.pad(R, (0, 0, 0, 0, 0, cout_p - cout))
        return (z, R) if f is None else (z * f, R * f)

    peak = reference(x, w)[0].abs().max().item()
    ku, ko = _pow2_scales(peak)
    fl = Flag()
    try:
        routed = False
        for k, want in ((ku, 0.0), (ko, 1.0)):
            # the power of two goes to both operands; the packed weights are halfs as well
            xs, ws = _scaled16(x, k - k // 2, "x"), _scaled16(w, k // 2, "w")
            ref, R = reference(xs.float(), ws.float())
            m = ref.abs().max().item()
            assert (m <= 0.97 * LIM) if want == 0.0 else (m >= 1.03 * LIM), (k, m)
            xd = F.pad(xs, (0, 0, 0, 0, 0, cin_p - cin)).cuda().contiguous(memory_format=CL)
            wd = ws.float().cuda()

            def run():
                epi = {}
                if site.fuse:
                    epi["fuse"] = ops.GradFuse(mask_src=maskd, mask_slope=0.2, mask_gain=2 ** 0.5, want_colsum=True)
                return ops.conv_fwd(xd, wd, spec, **epi) if site.op == "fwd" else ops.conv_bwd_data(xd, wd, spec, (H, W), **epi)

            if not routed:
                _assert_conv_route(site, run)
                routed = True
            found, y = fl.after(run)
            n_over = int((ref.abs() > LIM).sum())
            print(f"\n[flag random] {site.name} 2^{k}: max |ref| {m:.1f} ({n_over} elements over), flag {found}")
            assert found == want, f"{site.name} at 2^{k}: flag {found} with max |ref| = {m:.1f}"
            got = y.double().cpu()
            assert torch.isfinite(got).all() and got.abs().max().item() <= LIM
            _check(got, ref.clamp(-LIM, LIM), R, "f16", f"{site.name} 2^{k}")
            found, _ = fl.after(run, watch=False)
            assert found == 0.0
    finally:
        fl.restore()


RANDOM_FIR = [
    FirSite("rand_tiled", "blur4x4_tiled", (2, 8, 38, 42, 1, 1, 1, (37, 41))),
    FirSite("rand_tiled_fuse", "blur4x4_tiled", (2, 8, 38, 42, 1, 1, 1, (37, 41)), fuse=True),
    FirSite("rand_rows", "blur4x4_rows", (2, 256, 256, 256, 1, 1, 1, (255, 255)), big=True),
    FirSite("rand_down2", "fir4x4_resample<1,2>", (2, 8, 37, 41, 1, 2, 1, (18, 20))),
    FirSite("rand_up2_even", "fir4x4_up2_block", (3, 8, 37, 29, 2, 1, 2, (75, 59))),   # odd Ho / Wo on the even pad as well
    FirSite("rand_up2_odd", "fir4x4_up2_block", (3, 8, 37, 29, 2, 1, 1, (73, 57))),
]


@pytest.mark.parametrize("site", RANDOM_FIR, ids=[s.name for s in RANDOM_FIR])
def test_random_background_fir(site):
    from gif_amd import ops
    B, C, H, W, up, down, pad0, (Ho, Wo) = site.dims
    assert fir_kernel(*site.dims) == site.kernel
    g = torch.Generator(device="cuda").manual_seed(zlib.crc32(site.name.encode()))
    x = _r16(torch.randn(B, C, H, W, generator=g, device="cuda"))
    k = torch.rand(4, 4, generator=g, device="cuda") + 0.25  # asymmetric: fp32, as the kernels read it
    k = k / k.sum() * up ** 2
    f = maskd = None
    if site.fuse:
        maskd = torch.randn(B, C, Ho, Wo, generator=g, device="cuda").to(H16).contiguous(memory_format=CL)
        f = 2 ** 0.5 * torch.where(maskd > 0, 1.0, 0.2).double()

    def reference(xs, ks):  # fp64 on the device: slices and adds (fir64)
        z, R = fir64(xs.double(), ks.double(), up, down, pad0, (Ho, Wo)), fir64(xs.double().abs(), ks.double(), up, down, pad0, (Ho, Wo))
        return (z, R) if f is None else (z * f, R * f)

    peak = reference(x, k)[0].abs().max().item()
    ku, ko = _pow2_scales(peak)
    fl = Flag()
    try:
        for kk, want in ((ku, 0.0), (ko, 1.0)):
            # a blur lowers the peak: 2^kk on x alone would leave the half range, so the fp32 kernel takes half of the exponent
            xs, ks = _scaled16(x, kk - kk // 2, "x"), k * 2.0 ** (kk // 2)
            ref, R = reference(xs.float(), ks)
            m = ref.abs().max().item()
            assert (m <= 0.97 * LIM) if want == 0.0 else (m >= 1.03 * LIM), (kk, m)
            xd = xs.contiguous(memory_format=CL)

            def run():
                kw = {"fuse": ops.GradFuse(mask_src=maskd, mask_slope=0.2, mask_gain=2 ** 0.5, want_colsum=True)} if site.fuse else {}
                return ops.upfirdn2d(xd, ks, up, down, pad0, (Ho, Wo), **kw)

            found, y = fl.after(run)
            print(f"\n[flag random] {site.name} 2^{kk}: max |ref| {m:.1f} ({int((ref.abs() > LIM).sum())} elements over), flag {found}")
            assert found == want, f"{site.name} at 2^{kk}: flag {found} with max |ref| = {m:.1f}"
            got = y.double()
            assert torch.isfinite(got).all() and got.abs().max().item() <= LIM
            _check(got, ref.clamp(-LIM, LIM), R, "fir16", f"{site.name} 2^{kk}")  # (on the device: 33 M elements in the rows shape)
            found, _ = fl.after(run, watch=False)
            assert found == 0.0
    finally:
        fl.restore()
