"""-m gpu: the pointwise, packing, pyramid and texture-loss kernels of csrc/elementwise.hip (bias_act_kernel, pack_nhwc_kernel,
unpack_nhwc_kernel, bilinear_down_kernel / _bwd_kernel, tex_pair_loss_stage1 / stage2 / bwd_kernel, the generic upfirdn2d_kernel)
and the f16 saturation flag of common.h (store4_flag) at the edges of their index arithmetic, against an fp64 reference.

Each row of the tables sits on one side of an edge: a single float4, a channel-quad count that is no power of two (`i % C4`), the
grid caps (ew_grid: 4096 workgroups x 256 lanes = 1 048 576 work items per trip of a grid-stride loop; tex_pair_blocks: 1024
workgroups = 262 144 items), a workgroup that spans a channel boundary (`i % HW`), source strides, kernel shapes, pads and output
sizes that read outside the input.  Each row's comment names the edge.  Rows are seeded from their own description.

Reference: torch.float64 on the CPU over the operands the kernel reads (f16 rows: the half-rounded operands).  Bound, per element
and with no element excluded (test_gpu_conv_routes._check):

    |got - ref| <= TOL[family] * R + TINY[family]

R is the same operation on absolute values carried through the epilogue.  Two places where that sentence needs a decision:
  * texture-loss gradient g * f * s * (1 - s) * 2d with s = sigmoid(d^2): the kernel forms 1 - s from the ROUNDED s (as autograd's
    sigmoid backward does), so the complement carries the absolute rounding of s: R uses (1 + s) for it, the subtraction on absolute
    values.  d = a - b is one rounding of the exact difference: R uses |d|, not |a| + |b|.  Where s rounds to 1 (|d| >= ~4.2) the
    gradient is exactly 0; the true value is below 2|d| exp(-d^2), and the rows with |d| = 10 and 1e3 assert |gradient| < 1e-30.
  * exact operations are asserted bit-equal instead: pack / unpack, the f = 1 pyramid copy, zeros outside a FIR's support and off the
    pyramid's taps, the gradient on masked texels, the clamp to +-65504, act(bias + residual) where a FIR reads nothing.

Observed worst |got - ref| / R on the MI355X (all rows of this module, one run) and the tolerance chosen from it:
  bias32  1.6e-7 (cap_first)                        ->  TOL 8e-7    (5.0 x)
  bias16  4.9e-4 (cap_first_c8)                     ->  TOL 7e-4    (the f16 store alone rounds by up to 2^-11 = 4.9e-4 of |ref| <= R)
  down32  1.1e-7 (fwd_cap forward)                  ->  TOL 5e-7    (4.4 x)
  tex32   6.7e-8 (n1 loss)                          ->  TOL 3.5e-7  (5.2 x)
  texg32  7.9e-8 (cap_first gradient, gloss 0.37)   ->  TOL 4e-7    (5.1 x)
  gfir32  1.6e-7 (k4_noflip_blur)                   ->  TOL 8e-7    (5.1 x)
  gfir16  4.8e-4 (k3_up3)                           ->  TOL 7e-4    (2^-11 again: the sums themselves are exact to fp32)
  firg32  1.2e-7 (autograd up 2, pad (2, 1))        ->  TOL 6e-7    (5.1 x)
  firg16  4.7e-4 (autograd down 2, pad (1, 1))      ->  TOL 7e-4    (2^-11)
Every case prints its ratio ("[route ratio]" lines with -s) so that a re-measurement is one run of this module.

bilinear_down against ATen's float32 CPU kernel (the comment in elementwise.hip claims its operation order): NOT equal
in general.  The kernel computes 0.5 * (0.5 a + 0.5 b) + 0.5 * (0.5 c + 0.5 d) — multiplications by 0.5 are exact, so this is
((a + b) + (c + d)) / 4 with three roundings — and ATen's CPU kernel adds the four weighted taps in another order: 3 of the 13 rows
agree bit for bit (the others differ by one or two units in the last place), so bit equality is printed ("[aten bits]") and not
asserted; the fp64 bound is the check."""
import math
import zlib

import pytest
import torch
import torch.nn.functional as F

from gpu_util import Flag as _Flag  # (moved there: tests/test_gpu_f16_flag_sites.py and test_gpu_f16_overflow_chain.py share it)
from test_gpu_conv_routes import TINY, TOL, _check, fir64

H16 = torch.float16
F32 = torch.float32
CL = torch.channels_last
SQRT2 = 2 ** 0.5
CAP = 4096 * 256      # ew_grid: work items of one trip
TEX_CAP = 1024 * 256  # tex_pair_blocks

# this module's tolerance families, added to the tables that test_gpu_conv_routes._check reads
TOL.update({"bias32": 8e-7, "bias16": 7e-4, "down32": 5e-7, "tex32": 3.5e-7, "texg32": 4e-7, "gfir32": 8e-7, "gfir16": 7e-4,
            "firg32": 6e-7, "firg16": 7e-4})
TINY.update({"bias32": 1e-30, "bias16": 2.0 ** -24, "down32": 1e-30, "tex32": 1e-30, "texg32": 1e-30, "gfir32": 1e-30,
             "gfir16": 2.0 ** -24, "firg32": 1e-30, "firg16": 2.0 ** -24})


def _rng(*desc):
    return torch.Generator().manual_seed(zlib.crc32(repr(desc).encode()))


def _r16(t):
    return t.to(H16).float()


def _id(dt):
    return "f16" if dt == H16 else "f32"


def _cl(t, dt=None):
    return (t if dt is None else t.to(dt)).cuda().contiguous(memory_format=CL)


def _contract(y, y2, shape, dt, what):
    """shape, dtype, layout, finiteness, and the same bits from a second call"""
    assert tuple(y.shape) == tuple(shape) and y.dtype == dt, (what, y.shape, y.dtype)
    assert y.is_contiguous(memory_format=CL), f"{what}: not NHWC"
    assert torch.isfinite(y).all(), f"{what}: NaN / Inf"
    assert torch.equal(y, y2), f"{what}: a second call gave different bits"


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == H16 else torch.int32)


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. bias_act forward: y = gain * lrelu(x + residual + bias[c], slope); one lane = one float4, bias quad = i % C4
# ---------------------------------------------------------------------------------------------------------------------------------
BA_ROWS = [
    # name, B, C, H, W, bias, residual, slope, gain          (f16 runs the rows with C % 8 == 0)
    ("px1_c4", 1, 4, 1, 1, True, True, 0.2, SQRT2),          # n4 = 1: a single float4
    ("px1_c8", 1, 8, 1, 1, True, True, 0.2, SQRT2),          # the f16 twin: two float4
    ("c12", 2, 12, 5, 7, True, True, 0.2, SQRT2),            # C4 = 3: i % C4 with 256 % C4 != 0, more than one workgroup
    ("c24", 2, 24, 9, 7, True, True, 0.2, SQRT2),            # C4 = 6 (f16 too)
    ("c36", 1, 36, 3, 5, True, True, 0.2, SQRT2),            # C4 = 9
    ("c1024", 1, 1024, 2, 3, True, True, 0.2, SQRT2),        # C4 = 256 = the workgroup: the backward's limit, not the forward's
    ("c1028", 1, 1028, 1, 3, True, True, 0.2, SQRT2),        # C4 = 257 > 256: the forward has no limit
    ("c1032", 1, 1032, 1, 3, True, True, 0.2, SQRT2),        # C4 = 258 (f16 too)
    ("bias_only", 2, 24, 5, 7, True, False, 0.2, SQRT2),
    ("res_only", 2, 24, 5, 7, False, True, 0.2, SQRT2),
    ("neither", 2, 24, 5, 7, False, False, 0.2, SQRT2),
    ("identity", 2, 24, 5, 7, True, True, 1.0, 1.0),         # slope 1, gain 1: the bias-only epilogue of the condition-noise conv
    ("slope_01_gain3", 2, 24, 5, 7, True, True, 0.01, 3.0),
    ("relu_gain_half", 2, 12, 5, 7, True, False, 0.0, 0.5),  # slope 0
    ("cap_last", 1, 4, 1024, 1024, True, False, 0.2, SQRT2),     # n4 = 1 048 576: the last size with a single trip
    ("cap_first", 1, 4, 1, CAP + 1, True, True, 0.2, SQRT2),     # n4 = 1 048 577: the first with a second trip
    ("cap_mid_c12", 1, 12, 1, 349600, True, False, 0.2, SQRT2),  # C4 = 3, n4 = 1 048 800: 1 048 576 % 3 == 1, the second trip
                                                                  #   starts in the middle of a pixel
    ("cap_last_c8", 1, 8, 512, 1024, True, False, 0.2, SQRT2),   # f16 twins: n4 = 1 048 576,
    ("cap_first_c8", 1, 8, 1, CAP // 2 + 1, True, True, 0.2, SQRT2),  # 1 048 578 (the first even count past the cap),
    ("cap_mid_c24", 1, 24, 1, 174800, True, False, 0.2, SQRT2),  # C4 = 6, n4 = 1 048 800: 1 048 576 % 6 == 4
    ("zeros_c12", 1, 12, 4, 8, True, False, 0.2, SQRT2),     # rows of +0.0, -0.0 and x == -bias: lrelu's branch at exactly 0
    ("zeros_c24", 1, 24, 4, 8, True, False, 0.2, SQRT2),
]
BA_CASES = [pytest.param(r, dt, id=f"{r[0]}-{_id(dt)}") for r in BA_ROWS for dt in (F32, H16) if not (dt == H16 and r[2] % 8)]


def bias_act64(x, bias, res, slope, gain):
    """(reference, R) in fp64 from CPU operands (bias / res may be None)"""
    pre, R = x.double(), x.double().abs()
    if res is not None:
        pre, R = pre + res.double(), R + res.double().abs()
    if bias is not None:
        pre, R = pre + bias.double()[None, :, None, None], R + bias.double().abs()[None, :, None, None]
    return gain * F.leaky_relu(pre, slope), gain * max(1.0, abs(slope)) * R


@pytest.mark.gpu
@pytest.mark.parametrize("row,dt", BA_CASES)
def test_bias_act_forward(row, dt):
    from gif_amd import ops
    name, B, C, H, W, has_b, has_r, slope, gain = row
    g = _rng(row)
    rd = _r16 if dt == H16 else (lambda t: t)
    x = rd(torch.randn(B, C, H, W, generator=g))
    bias = torch.randn(C, generator=g) if has_b else None
    res = rd(torch.randn(B, C, H, W, generator=g)) if has_r else None
    zeros = name.startswith("zeros")
    if zeros:
        bias = rd(bias)  # so that -bias is an activation value in f16 as well
        bias[::2] = 0.0  # every second channel: x = +-0 gives a pre-activation of exactly +-0
        x[:, :, 0], x[:, :, 1], x[:, :, 2] = 0.0, -0.0, -bias[None, :, None]
    xd = _cl(x, dt)
    kw = dict(bias=None if bias is None else bias.cuda(), residual=None if res is None else _cl(res, dt), slope=slope, gain=gain)
    y = ops.bias_act(xd, **kw)
    _contract(y, ops.bias_act(xd, **kw), (B, C, H, W), dt, name)
    ref, R = bias_act64(x, bias, res, slope, gain)
    got = y.double().cpu()
    _check(got, ref, R, "bias16" if dt == H16 else "bias32", f"{name} bias_act")
    if zeros:
        at0 = (x.double() + bias.double()[None, :, None, None]) == 0
        assert at0[:, ::2, :3].all() and at0[:, :, 2].all() and at0.sum().item() == B * W * (C + 2 * (C // 2))
        assert torch.count_nonzero(ref[at0]).item() == 0 and torch.count_nonzero(got[at0]).item() == 0, f"{name}: lrelu(0) is not 0"
        want = F.leaky_relu(x + bias[None, :, None, None], slope) * torch.tensor(gain)
        assert torch.equal(got[:, :, :3].float(), want[:, :, :3].to(dt).float()), f"{name}: differs from F.leaky_relu around 0"


@pytest.mark.gpu
def test_bias_act_f16_forward_store_clamps():
    """The forward store (store4, no flag) clamps: a result beyond the half range is +-65504, never Inf; 65504 itself is kept."""
    from gif_amd import ops
    v = torch.tensor([60000., -60000., 65504., -65504., 32752., -32752., 32768., -32768., 100., -100., 0., 1., 40000., -40000.,
                      32736., -7.])
    x = v.view(1, 16, 1, 1).repeat(1, 1, 2, 3)
    assert torch.equal(_r16(x), x)
    y = ops.bias_act(_cl(x, H16), None, None, 1.0, 2.0)
    want = torch.clamp(2.0 * x, -65504.0, 65504.0)
    assert torch.equal(_r16(want), want) and (want.abs() == 65504).sum() >= 8
    assert torch.isfinite(y).all() and torch.equal(y.float().cpu(), want)
    # through bias, residual and the negative branch: 2 * 0.5 * (x - 60000 - 60000) <= -54496 (kept, at x = 65504), else -65504
    b = torch.full((16,), -60000.0)
    y = ops.bias_act(_cl(x, H16), b.cuda(), _cl(torch.full_like(x, -60000.0), H16), 0.5, 2.0)
    ref, _ = bias_act64(x, b, torch.full_like(x, -60000.0), 0.5, 2.0)
    assert torch.equal(y.float().cpu(), torch.clamp(ref, -65504.0, 65504.0).to(H16).float())
    assert y.min().item() == -65504.0 and y.max().item() == -54496.0


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. pack_nhwc / unpack_nhwc: one lane = one pixel, any source strides; exact
# ---------------------------------------------------------------------------------------------------------------------------------
def pack_ref(a, b, off0, off1, cp):
    """F.pad(torch.cat(...)): a at [off0, off0 + C0), b (or None) at [off1, off1 + C1), zeros in front, between and behind"""
    parts, end = [a], off0 + a.shape[1]
    if b is not None:
        parts += [a.new_zeros(a.shape[0], off1 - end, *a.shape[2:]), b]
        end = off1 + b.shape[1]
    return F.pad(torch.cat(parts, 1), (0, 0, 0, 0, off0, cp - end))


PK_ROWS = [
    # name, B, H, W, C0, off0, C1 (0: one source), off1, Cp, view of source 0, view of source 1
    ("px1", 1, 1, 1, 3, 0, 0, 0, 4, "nchw", ""),                 # H = W = 1, one source, Cp = 4
    ("row_1xw", 2, 1, 9, 3, 0, 6, 3, 16, "nchw", "nchw"),        # 1 x W image; the discriminator's 3 + 6 -> 16 (9 live channels)
    ("col_hx1", 2, 9, 1, 3, 0, 6, 3, 16, "nchw", "cl"),          # H x 1 image
    ("off0_1", 2, 5, 7, 3, 1, 0, 0, 4, "nchw", ""),              # off0 > 0: a zero channel in front (what UnpackNhwcFn.backward packs)
    ("gap", 2, 5, 7, 2, 1, 3, 5, 12, "cl", "nchw"),              # zeros in front, a gap (channels 3, 4) and padding behind (8 .. 11)
    ("tight", 3, 4, 6, 4, 0, 4, 4, 8, "nchw", "nchw"),           # no padding at all
    ("cslice", 2, 5, 7, 3, 0, 6, 3, 16, "cslice", "cslice"),     # channel-sliced channels_last views
    ("sslice", 2, 5, 7, 3, 0, 6, 3, 12, "sslice", "nchw"),       # x[:, :, 1:-1, 2:]
    ("expand", 3, 5, 7, 3, 0, 6, 3, 12, "nchw", "expand"),       # batch stride 0
    ("expand0", 3, 5, 7, 3, 0, 0, 0, 4, "expand", ""),           # batch stride 0 on source 0
    ("hw_t", 2, 5, 7, 3, 0, 6, 3, 12, "hw_t", "hw_t"),           # transposed in H and W
    ("multi_wg", 2, 17, 19, 1, 0, 2, 1, 4, "nchw", "cl"),        # 646 pixels: three workgroups
    ("cap_last", 1, 1024, 1024, 1, 0, 0, 0, 4, "nchw", ""),      # npix = 1 048 576: the last single trip
    ("cap_first", 1, 1, CAP + 1, 1, 0, 0, 0, 4, "nchw", ""),     # npix = 1 048 577: the first second trip
]


def _src(kind, B, C, H, W, g):
    """(values as a contiguous CPU tensor, device view with the strides `kind` names)"""
    shape, view = {
        "nchw": ((B, C, H, W), lambda t: t),
        "cl": ((B, C, H, W), lambda t: t.contiguous(memory_format=CL)),
        "cslice": ((B, C + 3, H, W), lambda t: t.contiguous(memory_format=CL)[:, 1:1 + C]),
        "sslice": ((B, C, H + 2, W + 2), lambda t: t[:, :, 1:-1, 2:]),
        "expand": ((1, C, H, W), lambda t: t.expand(B, C, H, W)),
        "hw_t": ((B, C, W, H), lambda t: t.transpose(2, 3)),
    }[kind]
    base = torch.randn(shape, generator=g)
    return view(base).contiguous(), view(base.cuda())


def _pack_case(row):
    name, B, H, W, C0, off0, C1, off1, cp, v0, v1 = row
    g = _rng(row)
    a, ad = _src(v0, B, C0, H, W, g)
    b, bd = _src(v1, B, C1, H, W, g) if C1 else (None, None)
    return a, ad, b, bd


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [F32, H16], ids=_id)
@pytest.mark.parametrize("row", PK_ROWS, ids=[r[0] for r in PK_ROWS])
def test_pack_nhwc(row, dt):
    from gif_amd import ops
    name, B, H, W, C0, off0, C1, off1, cp, v0, v1 = row
    a, ad, b, bd = _pack_case(row)
    if v0 in ("expand", "hw_t", "sslice", "cslice"):
        assert not ad.is_contiguous() and (v0 != "expand" or ad.stride(0) == 0)
    y = ops.pack_nhwc(ad, off0, bd, off1, cp, dt)
    _contract(y, ops.pack_nhwc(ad, off0, bd, off1, cp, dt), (B, cp, H, W), dt, name)
    want = pack_ref(a, b, off0, off1, cp).to(dt)
    assert torch.equal(_bits(y.cpu().contiguous()), _bits(want)), f"{name}: pack_nhwc is not bit-equal to F.pad(cat).to({dt})"
    if dt == H16:
        return
    # the adjoint per source, and <pack(a, b), g> = <a, unpack(g, off0, C0)> + <b, unpack(g, off1, C1)>
    gy = torch.randn(B, cp, H, W, generator=_rng(row, "g"))
    gd = _cl(gy)
    lhs = (y.double().cpu() * gy.double()).sum().item()
    rhs, mag = 0.0, 0.0
    for s, off, C in ((a, off0, C0), (b, off1, C1)):
        if s is None:
            continue
        u = ops.unpack_nhwc(gd, off, C)
        _contract(u, ops.unpack_nhwc(gd, off, C), (B, C, H, W), F32, f"{name} unpack")
        assert torch.equal(u.cpu(), gy[:, off:off + C]), f"{name}: unpack_nhwc({off}, {C}) is not the channel slice"
        rhs += (s.double() * u.double().cpu()).sum().item()
        mag += (s.double().abs() * gy[:, off:off + C].double().abs()).sum().item()
    assert abs(lhs - rhs) <= 1e-12 * mag, f"{name}: adjointness {lhs} vs {rhs}"  # exact maps: only the fp64 sums round


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [F32, H16], ids=_id)
def test_unpack_nhwc_offsets(dt):
    """c_off = 0, 1, 3 and Cp - C with C = 1, 3, 6 out of Cp = 16: the slice, cast to float (one lane copies C scalars)"""
    from gif_amd import ops
    B, cp, H, W = 2, 16, 5, 7
    gy = torch.randn(B, cp, H, W, generator=_rng("unpack", cp)).to(dt)
    gd = _cl(gy)
    for C in (1, 3, 6):
        for off in (0, 1, 3, cp - C):
            u = ops.unpack_nhwc(gd, off, C)
            _contract(u, ops.unpack_nhwc(gd, off, C), (B, C, H, W), F32, f"unpack {off} {C}")
            assert torch.equal(u.cpu(), gy[:, off:off + C].float()), (off, C)
    big = torch.randn(1, 4, 1, CAP + 1, generator=_rng("unpack cap")).to(dt)  # npix = 1 048 577 (f16: Cp 8)
    if dt == H16:
        big = torch.cat([big, big.flip(1)], 1)
    u = ops.unpack_nhwc(_cl(big), 1, 2)
    assert torch.equal(u.cpu(), big[:, 1:3].float())


@pytest.mark.gpu
def test_pack_nhwc_refusals():
    from gif_amd import _lib, ops
    a, b = torch.randn(2, 3, 4, 5, device="cuda"), torch.randn(2, 6, 4, 5, device="cuda")
    with pytest.raises(_lib.GifHipError, match="source 1 must follow source 0"):
        ops.pack_nhwc(a, 6, b, 0, 12, F32)          # source 1 in front of source 0
    with pytest.raises(_lib.GifHipError, match="source 1 must follow source 0"):
        ops.pack_nhwc(a, 0, b, 2, 12, F32)          # overlapping
    with pytest.raises(_lib.GifHipError, match=r"source 0 channels \[2, 5\) outside \[0, 4\)"):
        ops.pack_nhwc(a, 2, None, 0, 4, F32)        # off0 + C0 > Cp
    with pytest.raises(_lib.GifHipError, match="source 1 must follow source 0 inside Cp"):
        ops.pack_nhwc(a, 0, b, 3, 8, F32)           # off1 + C1 > Cp
    with pytest.raises(_lib.GifHipError, match=r"bad arguments \(Cp=10\)"):
        ops.pack_nhwc(a, 0, b, 3, 10, F32)          # Cp % 4 != 0
    with pytest.raises(_lib.GifHipError, match="no CPU fallback"):
        ops.pack_nhwc(a.cpu(), 0, None, 0, 4, F32)
    with pytest.raises(_lib.GifHipError, match="unpack_nhwc: bad arguments"):
        ops.unpack_nhwc(_cl(torch.zeros(1, 8, 2, 2)), 6, 3)  # c_off + C > Cp


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the f16 saturation flag at its threshold (common.h store4_flag: raised unless every |v| <= 65504, NaN included).  The nan case
# failed before this module: the flag tested the fmaxf of the four magnitudes, which drops a NaN beside a finite value, and sat_f16's
# fminf / fmaxf stored the NaN as -65504 — an f16 gradient NaN reached the loss scaler neither as a flag nor as a value.
# ---------------------------------------------------------------------------------------------------------------------------------
FLAG_VALUES = [("next", float(torch.tensor(65504.0).nextafter(torch.tensor(math.inf)))), ("pinf", math.inf), ("ninf", -math.inf),
               ("nan", math.nan)]


@pytest.mark.gpu
@pytest.mark.parametrize("vname,val", FLAG_VALUES, ids=[v[0] for v in FLAG_VALUES])
def test_f16_flag_threshold_pack_nhwc(vname, val):
    from gif_amd import ops
    assert torch.tensor(val).isnan() or abs(val) > 65504.0
    fl = _Flag()
    try:
        for npix, spots in ((300, (0, 299)), (CAP + 300, (CAP + 17,))):  # first pixel, last pixel; a pixel of the second trip only
            g = _rng("flag", npix)
            base = (torch.rand(1, 1, 1, npix, generator=g) * 2 - 1) * 65504.0
            base[0, 0, 0, 5], base[0, 0, 0, 7] = 65504.0, -65504.0  # the largest magnitude is exactly the limit
            assert base.abs().max().item() == 65504.0
            bd = base.cuda()
            found, y = fl.after(lambda: ops.pack_nhwc(bd, 0, None, 0, 4, H16))
            assert found == 0.0, "a tensor whose largest magnitude is 65504 raised the flag"
            assert torch.equal(_bits(y.cpu()), _bits(pack_ref(base, None, 0, 0, 4).to(H16)))
            for spot in spots:
                t = base.clone()
                t[0, 0, 0, spot] = val
                td = t.cuda()
                found, y = fl.after(lambda: ops.pack_nhwc(td, 0, None, 0, 4, H16))
                assert found == 1.0, f"{vname} at pixel {spot} of {npix} did not raise the flag"
                got = y[0, 0, 0, spot].item()
                print(f"\n[flag] {vname} at {spot}: stored {got}")
                want = t.clamp(-65504.0, 65504.0)  # (clamp keeps NaN)
                assert (math.isnan(got) if math.isnan(val) else got == math.copysign(65504.0, val)), f"{vname}: stored {got}"
                keep = torch.ones(npix, dtype=torch.bool)
                keep[spot] = not math.isnan(val)
                assert torch.equal(y.cpu()[0, 0, 0][keep], want.to(H16)[0, 0, 0][keep]) and not y.cpu()[0, 1:].any()
                found, _ = fl.after(lambda: ops.pack_nhwc(td, 0, None, 0, 4, H16), watch=False)
                assert found == 0.0, "flagged with watching off"
            # the flag survives a clean launch until it is cleared
            fl.clear()
            ops.pack_nhwc(td, 0, None, 0, 4, H16)
            ops.pack_nhwc(bd, 0, None, 0, 4, H16)
            assert fl.read() == 1.0
            found, _ = fl.after(lambda: ops.pack_nhwc(bd, 0, None, 0, 4, H16))
            assert found == 0.0
    finally:
        fl.restore()


@pytest.mark.gpu
def test_f16_flag_threshold_generic_fir():
    """The same threshold through upfirdn2d_kernel's store: a 1 x 1 kernel of value 1 stores its input."""
    from gif_amd import ops
    fl = _Flag()
    try:
        x = _r16((torch.rand(1, 8, 3, 5, generator=_rng("firflag")) * 2 - 1) * 65504.0)
        x[0, 0, 0, 0], x[0, 7, 2, 4] = 65504.0, -65504.0
        k = torch.ones(1, 1, device="cuda")
        xd = _cl(x, H16)
        found, y = fl.after(lambda: ops.upfirdn2d(xd, k, 1, 1, 0, (3, 5)))
        assert found == 0.0 and torch.equal(y, xd)
        # 65504 + 2^-8 is the next float32: over the limit in the accumulator, stored as 65504
        bias = torch.zeros(8)
        bias[0] = 2.0 ** -8
        found, y = fl.after(lambda: ops.upfirdn2d(xd, k, 1, 1, 0, (3, 5), bias=bias.cuda()))
        assert found == 1.0 and y[0, 0, 0, 0].item() == 65504.0 and torch.isfinite(y).all()
        found, _ = fl.after(lambda: ops.upfirdn2d(xd, k, 1, 1, 0, (3, 5), bias=bias.cuda()), watch=False)
        assert found == 0.0
        for val in (math.inf, -math.inf):
            t = x.clone()
            t[0, 3, 1, 2] = val
            td = _cl(t, H16)
            found, y = fl.after(lambda: ops.upfirdn2d(td, k, 1, 1, 0, (3, 5)))
            assert found == 1.0 and y[0, 3, 1, 2].item() == math.copysign(65504.0, val)
    finally:
        fl.restore()


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. bilinear_down forward / backward: taps f*d + f/2 - 1 and f*d + f/2 per axis, weight 0.5 each; f == 1 copies
# ---------------------------------------------------------------------------------------------------------------------------------
BD_ROWS = [
    # name, B, C, R, S
    ("f2_s1", 1, 4, 2, 1),          # one output pixel, one float4
    ("f4_s1", 3, 8, 4, 1),
    ("f2_s2", 1, 12, 4, 2),         # C4 = 3: idx % C4
    ("f4_s2", 3, 20, 8, 2),         # C4 = 5
    ("f2_s3", 1, 20, 6, 3),         # (6, 3): odd S
    ("f6_s2", 3, 12, 12, 2),        # f = 6: o0 = 2
    ("f6_s3", 1, 8, 18, 3),
    ("f64_s1", 1, 4, 64, 1),        # f = 64: taps 31, 32 of 64
    ("f1_s5", 3, 12, 5, 5),         # f = 1: a copy
    ("f4_s5", 1, 20, 20, 5),        # backward 2000 items: several workgroups
    ("fwd_cap", 61681, 68, 2, 1),   # forward B*S*S*C/4 = 61681 * 17 = 1 048 577: the first second trip (C4 = 17)
    ("bwd_cap", 61681, 68, 1, 1),   # backward B*R*R*C/4 = 1 048 577 (2^20 + 1 = 17 * 61681 has no square factor: R = 1, the copy)
    ("bwd_cap_f2", 1, 4, 1026, 513),  # backward 1 052 676 items with f = 2: taps on the second trip
]
ATEN_BITS = {}  # row -> the forward equals ATen's float32 CPU kernel bit for bit


def down_tap_mask(R, S):
    """[R, R] bool: the source pixels that are one of the four taps of their f x f cell (f even)"""
    f = R // S
    on = torch.tensor([(i % f) in (f // 2 - 1, f // 2) for i in range(R)])
    return on[:, None] & on[None, :]


@pytest.mark.gpu
@pytest.mark.parametrize("row", BD_ROWS, ids=[r[0] for r in BD_ROWS])
def test_bilinear_down(row):
    from gif_amd import ops
    name, B, C, R, S = row
    g = _rng(row)
    x = torch.randn(B, C, R, R, generator=g)
    gy = torch.randn(B, C, S, S, generator=g)
    xd, gd = _cl(x), _cl(gy)
    y = ops.bilinear_down(xd, S)
    _contract(y, ops.bilinear_down(xd, S), (B, C, S, S), F32, name)
    gx = ops.bilinear_down(gd, S, backward_to=R)
    _contract(gx, ops.bilinear_down(gd, S, backward_to=R), (B, C, R, R), F32, f"{name} bwd")
    x64 = x.double().requires_grad_(True)
    ref = F.interpolate(x64, (S, S), mode="bilinear", align_corners=False)
    (gref,) = torch.autograd.grad(ref, x64, gy.double())
    Rf = F.interpolate(x.double().abs(), (S, S), mode="bilinear", align_corners=False)
    xa = x.double().requires_grad_(True)
    (Rb,) = torch.autograd.grad(F.interpolate(xa, (S, S), mode="bilinear", align_corners=False), xa, gy.double().abs())
    got, gotb = y.double().cpu(), gx.double().cpu()
    _check(got, ref.detach(), Rf, "down32", f"{name} fwd")
    _check(gotb, gref, Rb, "down32", f"{name} bwd")
    aten = F.interpolate(x, (S, S), mode="bilinear", align_corners=False)
    ATEN_BITS[name] = torch.equal(_bits(y.cpu().contiguous()), _bits(aten.contiguous()))
    print(f"\n[aten bits] {name}: {ATEN_BITS[name]}; so far {sum(ATEN_BITS.values())} of {len(ATEN_BITS)} rows equal")
    if R == S:
        assert torch.equal(y, xd) and torch.equal(gx, gd), f"{name}: f = 1 is a copy"
    else:
        off = ~down_tap_mask(R, S)
        assert torch.count_nonzero(gx.cpu()[:, :, off]).item() == 0, f"{name}: gradient off the four taps"
        assert torch.equal(gx.cpu()[:, :, ~off].view(B, C, S, 2, S, 2), (0.25 * gy)[:, :, :, None, :, None].expand(B, C, S, 2, S, 2))
    lhs, rhs = (got * gy.double()).sum().item(), (x.double() * gotb).sum().item()
    assert abs(lhs - rhs) <= TOL["down32"] * (Rf * gy.double().abs()).sum().item(), f"{name}: adjointness {lhs} vs {rhs}"


@pytest.mark.gpu
def test_bilinear_down_refusals():
    from gif_amd import _lib, ops
    with pytest.raises(_lib.GifHipError, match=r"R/S must be 1 or an even integer \(got 6/2\)"):
        ops.bilinear_down(_cl(torch.zeros(1, 4, 6, 6)), 2)            # R / S = 3
    with pytest.raises(_lib.GifHipError, match=r"R/S must be 1 or an even integer \(got 5/2\)"):
        ops.bilinear_down(_cl(torch.zeros(1, 4, 5, 5)), 2)            # R % S != 0
    with pytest.raises(_lib.GifHipError, match=r"R/S must be 1 or an even integer \(got 6/2\)"):
        ops.bilinear_down(_cl(torch.zeros(1, 4, 2, 2)), 2, backward_to=6)
    with pytest.raises(_lib.GifHipError, match="bilinear_down: bad arguments"):
        ops.bilinear_down(_cl(torch.zeros(1, 6, 4, 4)), 2)            # C = 6
    with pytest.raises(_lib.GifHipError, match="fp32 only"):
        ops.bilinear_down(_cl(torch.zeros(1, 8, 4, 4), H16), 2)


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. texture_pair_loss: mean(sigmoid(((a - b) ma mb)^2) f) over [C, H, W]; one lane = one element, mask / f index = i % HW
# ---------------------------------------------------------------------------------------------------------------------------------
TX_ROWS = [
    # name, C, H, W, masks (none | a | b | ab | all), f (pos | zeros | neg | ones), d ("" | sat)
    ("n1", 1, 1, 1, "none", "pos", ""),
    ("n255", 3, 5, 17, "ab", "neg", ""),           # one workgroup less a lane; HW 85: it spans three channels
    ("n256", 4, 8, 8, "a", "pos", ""),             # exactly one workgroup
    ("n257", 1, 1, 257, "b", "zeros", ""),         # one lane into the second workgroup
    ("hw77_c3", 3, 7, 11, "ab", "pos", ""),        # HW 77, non-square: i % HW
    ("hw300_c3", 3, 12, 25, "b", "neg", ""),       # HW 300 > 256 and no multiple of it: workgroups 1 and 2 span a channel boundary
    ("hw300_c4_none", 4, 25, 12, "none", "zeros", ""),
    ("cap_last", 4, 256, 256, "ab", "pos", ""),    # n = 262 144 = 1024 workgroups: the last single trip
    ("cap_first", 1, 5, 52429, "ab", "neg", ""),   # n = 262 145: the first second trip
    ("cap_c3", 3, 2, 43691, "b", "pos", ""),       # n = 262 146, C = 3: the second trip lands in channel 2
    ("all_masked", 3, 7, 11, "all", "neg", ""),    # loss = 0.5 mean(f), gradient exactly 0
    ("all_masked_ones", 4, 8, 8, "all", "ones", ""),  # ... and exactly 0.5: 256 x 0.5 / 256
    ("sat", 4, 8, 8, "a", "neg", "sat"),           # |a - b| = 0, 1e-4, 3, 10, 1e3: the sigmoid saturates
]
SAT_D = (0.0, 1e-4, 3.0, 10.0, 1e3)


def tex_loss64(a, b, ma, mb, f):
    """(loss, R of the loss, d, s) in fp64; ma / mb [H, W] 0 / 1 or None, f [H, W]"""
    d = a.double() - b.double()
    for m in (ma, mb):
        if m is not None:
            d = d * m.double()
    s = torch.sigmoid(d * d)
    return (s * f.double()).mean(), (s * f.double().abs()).mean(), d, s


def tex_grad_R(d, s, f, gloss):
    """R of d loss / d a = gloss / n * f * s * (1 - s) * 2 d: (1 + s) for the complement of the rounded s (module docstring)"""
    return abs(gloss) / d.numel() * f.double().abs() * s * (1 + s) * 2 * d.abs()


def _tex_case(row):
    name, C, H, W, masks, fk, dk = row
    g = _rng(row)
    a, b = torch.rand(C, H, W, generator=g) * 2 - 1, torch.rand(C, H, W, generator=g) * 2 - 1
    if dk == "sat":
        sgn = torch.where(torch.rand(C, H, W, generator=g) > 0.5, 1.0, -1.0)
        a = b + sgn * torch.tensor(SAT_D)[torch.arange(C * H * W) % len(SAT_D)].view(C, H, W)
    ma = (torch.rand(H, W, generator=g) > 0.3).float() if masks in ("a", "ab") else None
    mb = (torch.rand(H, W, generator=g) > 0.3).float() if masks in ("b", "ab") else None
    if masks == "all":
        ma, mb = (torch.rand(H, W, generator=g) > 0.5).float(), None
        mb = 1 - ma
    f = {"pos": lambda: torch.rand(H, W, generator=g), "neg": lambda: torch.randn(H, W, generator=g), "ones": lambda: torch.ones(H, W),
         "zeros": lambda: torch.rand(H, W, generator=g) * (torch.rand(H, W, generator=g) > 0.4)}[fk]()
    return a, b, ma, mb, f


@pytest.mark.gpu
@pytest.mark.parametrize("row", TX_ROWS, ids=[r[0] for r in TX_ROWS])
def test_texture_pair_loss(row):
    from gif_amd import losses, ops
    name, C, H, W, masks, fk, dk = row
    a, b, ma, mb, f = _tex_case(row)
    dev = lambda t: None if t is None else t.cuda()
    ad, bd, mad, mbd, fd = (dev(t) for t in (a, b, ma, mb, f))
    loss = ops.texture_pair_loss(ad, bd, mad, mbd, fd)
    assert loss.shape == () and loss.dtype == F32 and torch.isfinite(loss).item()
    assert torch.equal(loss, ops.texture_pair_loss(ad, bd, mad, mbd, fd)), f"{name}: a second call gave different bits"
    a64 = a.double().requires_grad_(True)
    ref, Rl, d, s = tex_loss64(a64, b, ma, mb, f)
    (gref,) = torch.autograd.grad(ref, a64)
    d, s = d.detach(), s.detach()
    _check(loss.double().cpu().view(1), ref.detach().view(1), Rl.detach().view(1), "tex32", f"{name} loss")
    vis = torch.ones(H, W) if ma is None else ma
    vis = vis if mb is None else vis * mb
    for gl in (0.37, 1.0):
        gd = torch.tensor(gl, device="cuda")
        ga = ops.texture_pair_loss(ad, bd, mad, mbd, fd, gloss=gd)
        assert ga.shape == (C, H, W) and ga.dtype == F32 and ga.is_contiguous() and torch.isfinite(ga).all()
        assert torch.equal(ga, ops.texture_pair_loss(ad, bd, mad, mbd, fd, gloss=gd))
        _check(ga.double().cpu(), gl * gref, tex_grad_R(d, s, f, gl), "texg32", f"{name} grad gloss {gl}")
        assert torch.count_nonzero(ga.cpu()[:, vis == 0]).item() == 0, f"{name}: gradient on a masked texel"
        if dk == "sat":
            big = (a - b).abs() >= 9.5
            assert big.sum() >= 2 * C * H * W // 5 - 1 and (ga.cpu()[big].abs() < 1e-30).all(), "gradient where the sigmoid is saturated"
    # the autograd function: the same loss bits, b's gradient the exact negative of a's, gloss scales
    ar, br = ad.clone().requires_grad_(True), bd.clone().requires_grad_(True)
    lf = losses._TexPairLossFn.apply(ar, br, mad, mbd, fd)
    assert torch.equal(lf.detach(), loss)
    (lf * 0.37).backward()
    assert torch.equal(br.grad, -ar.grad)
    assert torch.equal(ar.grad, ops.texture_pair_loss(ad, bd, mad, mbd, fd, gloss=torch.tensor(0.37, device="cuda")))
    if masks == "all":
        assert ref.item() == 0.5 * f.double().mean().item() and torch.count_nonzero(ar.grad).item() == 0
        if fk == "ones":
            assert loss.item() == 0.5


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. the generic upfirdn2d_kernel (KH * KW <= 16, not 4 x 4) and flip = 0 through every 4 x 4 route
# ---------------------------------------------------------------------------------------------------------------------------------
GF_ROWS = [
    # name, B, C, H, W, KH, KW, up, down, pad0, (Ho, Wo), flip, epilogue ("" | bra)
    ("k4_noflip_blur", 2, 8, 9, 7, 4, 4, 1, 1, 1, (8, 6), False, ""),      # flip = 0 on the tiled blur kernel
    ("k4_noflip_up2", 2, 8, 9, 7, 4, 4, 2, 1, 2, (18, 14), False, ""),     # ... the up-by-2 block kernel
    ("k4_noflip_up2_odd", 2, 8, 9, 7, 4, 4, 2, 1, 1, (17, 13), False, "bra"),
    ("k4_noflip_down2", 2, 8, 9, 8, 4, 4, 1, 2, 1, (4, 4), False, ""),     # ... the down-by-2 resample kernel
    ("k4_noflip_up2_down2", 2, 8, 9, 7, 4, 4, 2, 2, 2, (9, 7), False, ""),  # 4 x 4 on the generic kernel, flip = 0
    ("k1", 1, 8, 5, 6, 1, 1, 1, 1, 0, (5, 6), True, ""),                   # one tap, pad0 = 0: a scaled copy
    ("k2", 2, 8, 5, 6, 2, 2, 1, 1, 1, (6, 7), True, ""),
    ("k2_noflip", 2, 8, 5, 6, 2, 2, 1, 1, 1, (6, 7), False, ""),
    ("k3", 2, 8, 7, 5, 3, 3, 1, 1, 1, (7, 5), True, ""),
    ("k3_noflip", 2, 8, 7, 5, 3, 3, 1, 1, 1, (7, 5), False, ""),
    ("k1x4", 2, 8, 7, 5, 1, 4, 1, 1, 1, (8, 4), True, ""),                 # KH != KW: a * KW + b
    ("k4x1_noflip", 2, 8, 7, 5, 4, 1, 1, 1, 1, (6, 7), False, ""),
    ("k3x5", 2, 8, 7, 9, 3, 5, 1, 1, 2, (9, 9), True, ""),                 # 15 taps
    ("k3x5_noflip_bra", 2, 16, 7, 9, 3, 5, 1, 1, 2, (9, 9), False, "bra"),  # bias + residual + leaky ReLU on a non-4 x 4 kernel
    ("k5x3_up2", 1, 8, 5, 4, 5, 3, 2, 1, 2, (10, 9), True, ""),
    ("k3_up2_down2", 2, 8, 7, 5, 3, 3, 2, 2, 1, (7, 5), True, ""),         # up = 2 with down = 2
    ("k3_up3", 2, 8, 7, 5, 3, 3, 3, 1, 1, (21, 15), False, ""),            # up = 3: u / up, iy * up != u
    ("k2_down3", 2, 8, 10, 11, 2, 2, 1, 3, 1, (4, 4), True, ""),           # down = 3
    ("k3_pad0_0", 2, 8, 7, 5, 3, 3, 1, 1, 0, (5, 3), True, ""),            # pad0 = 0: the valid region only
    ("k2_pad0_5", 2, 8, 7, 5, 2, 2, 1, 1, 5, (12, 10), True, ""),          # pad0 = 5 > the kernel: rows / columns 0 .. 3 read nothing
    ("k3_past", 2, 8, 5, 4, 3, 3, 1, 1, 1, (10, 9), False, ""),            # rows >= 6, columns >= 5 read entirely outside: exactly 0
    ("k3_past_bra", 2, 8, 5, 4, 3, 3, 1, 1, 1, (10, 9), True, "bra"),      # ... act(bias + residual) with an epilogue
    ("k3_up2_past", 1, 8, 3, 4, 3, 3, 2, 1, 1, (11, 12), True, ""),
    ("multi_wg", 3, 24, 9, 11, 3, 3, 1, 1, 1, (9, 11), False, ""),         # 1782 items, C4 = 6
]
GF_CASES = [pytest.param(r, dt, id=f"{r[0]}-{_id(dt)}") for r in GF_ROWS for dt in (F32, H16)]


def _fir_case(row, f16):
    name, B, C, H, W, KH, KW, up, down, pad0, out, flip, epi = row
    g = _rng(row)
    rd = _r16 if f16 else (lambda t: t)
    x = rd(torch.randn(B, C, H, W, generator=g))
    k = torch.rand(KH, KW, generator=g) + 0.25  # asymmetric and positive: R is the same FIR on |x|
    k = k / k.sum() * up ** 2
    bias = torch.randn(C, generator=g) if epi else None
    res = rd(torch.randn(B, C, *out, generator=g)) if epi else None
    return x, k, bias, res


def fir_support(row):
    """[Ho, Wo] bool: the outputs that read at least one input sample"""
    name, B, C, H, W, KH, KW, up, down, pad0, out, flip, epi = row
    return fir64(torch.ones(1, 1, H, W, dtype=torch.float64), torch.ones(KH, KW, dtype=torch.float64), up, down, pad0, out)[0, 0] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("row,dt", GF_CASES)
def test_generic_upfirdn2d(row, dt):
    from gif_amd import ops
    name, B, C, H, W, KH, KW, up, down, pad0, out, flip, epi = row
    x, k, bias, res = _fir_case(row, dt == H16)
    ref = fir64(x.double(), k.double(), up, down, pad0, out, flip)
    R = fir64(x.double().abs(), k.double(), up, down, pad0, out, flip)
    kw = {}
    if epi:
        kw = dict(bias=bias.cuda(), residual=_cl(res, dt), act=True, slope=0.3, gain=1.25)
        ref = 1.25 * F.leaky_relu(ref + res.double() + bias.double()[None, :, None, None], 0.3)
        R = 1.25 * (R + res.double().abs() + bias.double().abs()[None, :, None, None])
    xd, kd = _cl(x, dt), k.cuda()
    y = ops.upfirdn2d(xd, kd, up, down, pad0, out, flip, **kw)
    _contract(y, ops.upfirdn2d(xd, kd, up, down, pad0, out, flip, **kw), (B, C, *out), dt, name)
    _check(y.double().cpu(), ref, R, "gfir16" if dt == H16 else "gfir32", f"{name} out")
    outside = ~fir_support(row)
    if "past" in name or "pad0_5" in name:
        assert outside.sum() >= out[0] + out[1]
    got_out = y.cpu()[:, :, outside]
    if not epi:
        assert torch.count_nonzero(got_out).item() == 0, f"{name}: outputs that read nothing are not 0"
    else:  # the kernel's own fp32 operations on an empty sum: (0 + residual) + bias, the branch, * slope, * gain
        v = res + bias[None, :, None, None]
        want = (torch.where(v > 0, v, v * torch.tensor(0.3)) * torch.tensor(1.25)).to(dt)
        assert torch.equal(got_out, want[:, :, outside]), f"{name}: outputs that read nothing are not act(bias + residual)"


@pytest.mark.gpu
def test_upfirdn2d_refuses_17_taps():
    from gif_amd import _lib, ops
    x = _cl(torch.zeros(1, 4, 4, 20))
    with pytest.raises(_lib.GifHipError, match="bad up/down/kernel"):
        ops.upfirdn2d(x, torch.ones(1, 17, device="cuda"), 1, 1, 0, (4, 4))
    assert ops.upfirdn2d(x, torch.ones(1, 16, device="cuda"), 1, 1, 0, (4, 5)).shape == (1, 4, 4, 5)


# autograd through GF.upfirdn2d: the backward calls the forward with swapped up / down, pad0' = K - 1 - pad0 and `not flip`, so
# with an asymmetric kernel a wrong tap order at flip = 0 shows
GA_ROWS = [(1, 1, (2, 1)), (2, 1, (2, 1)), (1, 2, (1, 1)), (1, 1, (-1, 2))]


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [F32, H16], ids=_id)
@pytest.mark.parametrize("up,down,pad", GA_ROWS, ids=[f"up{u}_down{d}_pad{p[0]}_{p[1]}" for u, d, p in GA_ROWS])
def test_upfirdn2d_autograd_asymmetric_kernel(up, down, pad, dt):
    from gif_amd import functional as GF
    from oracle import stylegan2_ref as R
    g = _rng("fir autograd", up, down, pad)
    rd = _r16 if dt == H16 else (lambda t: t)
    B, C, H, W = 2, 8, 9, 7
    x = rd(torch.randn(B, C, H, W, generator=g))
    k = torch.rand(4, 4, generator=g) + 0.25
    k = k / k.sum() * up ** 2
    x64 = x.double().requires_grad_(True)
    ref = R.upfirdn2d(x64, k.double(), up, down, pad)
    gy = rd(torch.randn(ref.shape, generator=g))
    (gref,) = torch.autograd.grad(ref, x64, gy.double())
    xa = x.double().requires_grad_(True)
    (Rg,) = torch.autograd.grad(R.upfirdn2d(xa, k.double(), up, down, pad), xa, gy.double().abs())
    Rf = R.upfirdn2d(x.double().abs(), k.double(), up, down, pad)
    grads = []
    for _ in range(2):
        xd = _cl(x, dt).requires_grad_(True)
        y = GF.upfirdn2d(xd, k.cuda(), up, down, pad)
        y.backward(_cl(gy, dt))
        grads.append(xd.grad)
    _contract(grads[0], grads[1], (B, C, H, W), dt, "fir autograd")
    assert y.shape == ref.shape and y.dtype == dt
    _check(y.detach().double().cpu(), ref.detach(), Rf, "gfir16" if dt == H16 else "gfir32", f"fir autograd {up} {down} {pad} fwd")
    _check(grads[0].double().cpu(), gref, Rg, "firg16" if dt == H16 else "firg32", f"fir autograd {up} {down} {pad} grad")
