"""-m gpu: the skinny GEMMs, the style path, the modulation bank, the column sums, the per-sample kernels and the fused Adam + EMA
at every tile, chunk and grid boundary of their index arithmetic, against an fp64 reference of the same operation.

Each row of the tables is a shape computed from one predicate or piece of index arithmetic (csrc/linear.hip: the 8-float K
chunks of skinny_nt_body split over 16 waves x 4 in flight, the 32 x 32 tiles and the four tiles per workgroup of skinny_tn_body,
the float4 A loads of skinny_nn_kernel, the bank's segment table; csrc/elementwise.hip: colsum_blocks, colsum_stage2,
mul_reduce_chunks, R = 256 / C4, the per-sample kernels; csrc/optim.hip: the 4096-float chunks and the vec check of
adam_ema_kernel): the last shape on one side of the boundary or the first on the other.  Each row's comment names the predicate
and the side.

Reference: torch.float64 on the CPU over exactly the operands the kernel reads (f16 rows: the half-rounded operands).  Bound, per
element:

    |got - ref| <= TOL[family] * R + EXTRA + TINY

where R is the same fp64 operation on absolute values (through nonlinear epilogues: the first-order sensitivity, e.g.
R_d = 0.5 |d|^3 R_v for d = rsqrt(v + eps)) and EXTRA is the absolute rounding of an epilogue that no operand magnitude carries
(the fp32 ulp of rsqrt's result, the store of a half).  An element whose reference pre-activation lies within TOL * R of zero may
take either branch of a leaky ReLU.

Observed worst |got - ref| / R on the MI355X (all rows of this module, one run) and the tolerance chosen from it:
  gemm    2.3e-7 (tn_t15_m65)                      ->  TOL 1e-6    (4.3 x)
  style   2.7e-7 (st_b65 style_demod_bwd_w)         ->  TOL 1.2e-6  (4.4 x)
  bank    2.9e-7 (bank_m33 seg1 gw)                 ->  TOL 1.2e-6  (4.1 x)
  sum32   2.7e-7 (cs_c1020 act_inv_mul_reduce)      ->  TOL 1.2e-6  (4.4 x)
  sum16   2.4e-7 (cs_c1016 f16 act_inv_mul_reduce)  ->  TOL 1e-6    (4.1 x; the f16 rows sum in fp32 as well)
  ew16    4.9e-4 (f16 mul_reduce scaled)            ->  TOL 7e-4    (the f16 store alone rounds by up to 2^-11 = 4.9e-4 of |ref| <= R)
  sample  1.0e-7 (bilinear_down f2)                 ->  TOL 5e-7    (5 x)
  adam    1.5e-7 (adam_scalar_ema v)                ->  TOL 1e-6    (6.5 x)
  route   9.0e-7 (modc_nobank12 g_w)                ->  TOL 4e-6    (4.4 x; the convolution routes run in the default fp32 mode)
Every case prints its ratio ("[route ratio]" lines with -s) so that a re-measurement is one run of this module."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import adam_ref

pytestmark = pytest.mark.gpu

H16 = torch.float16
CL = torch.channels_last
NAN = float("nan")
U32 = 2.0 ** -24  # unit round-off of fp32

# per-element tolerances (see the module docstring for the measurements behind them)
TOL = {"gemm": 1e-6, "style": 1.2e-6, "bank": 1.2e-6, "sum32": 1.2e-6, "sum16": 1e-6, "ew16": 7e-4, "sample": 5e-7, "adam": adam_ref.TOL_ADAM,
       "route": 4e-6}
TINY = 1e-30
WORST = {}  # family -> (worst ratio so far, case)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _note(fam, what, ratio):
    if fam not in WORST or ratio > WORST[fam][0]:
        WORST[fam] = (ratio, what)
    print(f"\n[route ratio] {fam} {what}: {ratio:.3e} (module worst so far {WORST[fam][0]:.3e} at {WORST[fam][1]})")


def _check(got, ref, R, fam, what, extra=None, alt=None):
    """|got - ref| <= TOL * R + extra + TINY element-wise.  got: any tensor (moved to CPU fp64); ref, R, extra, alt: fp64 CPU.
    alt: a second admissible reference (the other leaky-ReLU branch), used only where the pre-activation is ambiguous (NaN elsewhere)."""
    got = got.detach().double().cpu()
    assert got.shape == ref.shape == R.shape, (what, got.shape, ref.shape, R.shape)
    assert torch.isfinite(got).all(), f"{what}: {int((~torch.isfinite(got)).sum())} non-finite elements"
    err = (got - ref).abs()
    if alt is not None:
        err = torch.where(torch.isnan(alt), err, torch.minimum(err, (got - alt).abs()))
    ex = torch.zeros_like(R) if extra is None else extra
    ratio = ((err - ex).clamp_min(0) / (R + TINY)).max().item() if err.numel() else 0.0
    _note(fam, what, ratio)
    bad = err > TOL[fam] * R + ex + TINY
    if bad.any():
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{what} [{fam}]: {int(bad.sum())} of {bad.numel()} elements out of bound; first at {i}: got "
                             f"{got[i].item():.9e} ref {ref[i].item():.9e} R {R[i].item():.3e}; worst ratio {ratio:.3e} > {TOL[fam]:.1e}")


def _rng(seed):
    return torch.Generator().manual_seed(seed)


def _strided(x, extra, fill=NAN):
    """x [rows, w] -> device view of the same values inside a [rows, w + extra] buffer whose other columns hold `fill`."""
    buf = torch.full((x.shape[0], x.shape[1] + extra), fill, dtype=torch.float32)
    buf[:, :x.shape[1]] = x
    return buf.cuda()[:, :x.shape[1]]


def _poison(*numels):
    """Leave NaN-filled blocks of these sizes in the caching allocator, so that an output the kernel never writes reads NaN."""
    ts = [torch.full((n,), NAN, device="cuda") for n in numels for _ in range(16)]
    del ts


def _lrelu(v, slope, gain):
    return torch.where(v > 0, v, v * slope) * gain


def _pad4(c):
    return (c + 3) // 4 * 4


# ---------------------------------------------------------------------------------------------------------------------------------
# a. skinny GEMMs (csrc/linear.hip)
# ---------------------------------------------------------------------------------------------------------------------------------
# NT: C[M][N] = act(scale * A[M][K] . B[N][K]^T + bias).  nchunks = cdiv(K, 8); wave w takes chunks 4w .. 4w+3, then + 64.
NT_ROWS = [
    # name, M, N, K, cpad
    ("nt_k4", 33, 31, 4, 32),          # K % 8 == 4: one half chunk (lane half 1 idle); N 31 < one tile, cpad 32 = the tile
    ("nt_k12", 1, 32, 12, 33),         # K % 8 == 4 after one full chunk; M 1; cpad 33 > N crosses into a second column tile
    ("nt_k508", 31, 33, 508, 64),      # K 508: last of round 1 is a half chunk (63.5 chunks); N 33 = one column into tile 2
    ("nt_k512", 32, 64, 512, 64),      # K 512 = 16 waves x 4 chunks x 8: exactly one round; M 32 = one row tile
    ("nt_k516", 64, 65, 516, 96),      # K 516: a half chunk in round 2 (wave 0 only); cpad 96 > N 65: a whole padding tile
    ("nt_k520", 65, 40, 520, 40),      # K 520: one full chunk in round 2; M 65 = one row into row tile 3
    ("nt_k8192", 65, 33, 8192, 36),    # K 8192: 16 full rounds, none partial
    ("nt_k8196", 65, 520, 8196, 520),  # K 8196: a half chunk at the start of round 17 (the module's largest GEMM)
    ("nt_m512", 512, 32, 516, 32),     # M 512 = the skinny route's row limit: 16 row tiles
]


@pytest.mark.parametrize("row", NT_ROWS, ids=[r[0] for r in NT_ROWS])
def test_linear_nt(row):
    from gif_amd import ops
    name, M, N, K, cp = row
    g = _rng(1)
    A, B = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g)
    bias = torch.randn(N, generator=g)
    scale, slope, gain = 1 / math.sqrt(K), 0.2, math.sqrt(2)
    a, b = _strided(A, 8), _strided(B, 12)  # lda = K + 8, ldb = K + 12: the stride gaps hold NaN
    bd = bias.cuda()
    for act in (False, True):
        y1 = ops.linear_nt(a, b, bd, scale, act=act, slope=slope, gain=gain, n_pad=cp)
        y2 = ops.linear_nt(a, b, bd, scale, act=act, slope=slope, gain=gain, n_pad=cp)
        torch.cuda.synchronize()
        assert torch.equal(y1.view(torch.int32), y2.view(torch.int32)), f"{name}: second call differs"
        assert (y1[:, N:] == 0).all() and not torch.signbit(y1[:, N:]).any(), f"{name}: padding columns not +0"
        pre = scale * (A.double() @ B.double().T) + bias.double()
        Rp = scale * (A.double().abs() @ B.double().abs().T) + bias.double().abs()
        if act:
            ref, R = _lrelu(pre, slope, gain), Rp * gain
            amb = pre.abs() <= TOL["gemm"] * Rp
            alt = torch.where(amb, torch.where(pre > 0, pre * slope, pre) * gain, torch.full_like(pre, NAN))
            _check(y1[:, :N], ref, R, "gemm", f"{name} act", alt=alt)
        else:
            _check(y1[:, :N], pre, Rp, "gemm", f"{name}")


# NN: C[M][K] = scale * A[M][N] . B[N][K]; A read as float4 over [n, n+4) with only n < N checked, B zero for n + t >= N.
NN_ROWS = [
    # name, M, N, K (output columns), kpad
    ("nn_n9", 33, 9, 31, 32),       # N % 8 == 1: chunk 2 holds one valid column; K 31 < one tile
    ("nn_n12", 1, 12, 32, 33),      # N % 8 == 4: the last chunk's upper half absent; kpad 33 crosses into tile 2
    ("nn_n13", 32, 13, 33, 64),     # N % 8 == 5, N % 4 == 1: A columns 13..15 inside the float4 are outside the operand
    ("nn_n517", 65, 517, 65, 96),   # N % 8 == 5 past one 512-column round; kpad 96: a whole padding tile
    ("nn_n1023", 64, 1023, 40, 40), # N % 4 == 3: three NaN-filled columns in the last float4; two rounds of 64 chunks
    ("nn_m512", 512, 20, 36, 36),   # M 512 = the row limit; N % 8 == 4
]


@pytest.mark.parametrize("row", NN_ROWS, ids=[r[0] for r in NN_ROWS])
def test_linear_nn(row):
    """Columns [N, lda) of A — including [N, pad4(N)), which the float4 loads read — and every stride gap hold NaN: the header
    promises C = scale * A[M][N] . B[N][K], so none of it may reach C."""
    from gif_amd import ops
    name, M, N, K, kp = row
    g = _rng(2)
    A, B = torch.randn(M, N, generator=g), torch.randn(N, K, generator=g)
    scale = 1 / math.sqrt(N)
    a = _strided(A, _pad4(N) - N + 8)  # lda = pad4(N) + 8
    b = _strided(B, 4 + (-K) % 4)
    y1 = ops.linear_nn(a, b, scale, k_pad=kp)
    y2 = ops.linear_nn(a, b, scale, k_pad=kp)
    torch.cuda.synchronize()
    assert torch.equal(y1.view(torch.int32), y2.view(torch.int32)), f"{name}: second call differs"
    assert (y1[:, K:] == 0).all(), f"{name}: padding columns not zero"
    _check(y1[:, :K], scale * (A.double() @ B.double()), scale * (A.double().abs() @ B.double().abs()), "gemm", name)


# TN: C[N][K] = scale * A[M][N]^T . B[M][K]; 32 x 32 tiles, 4 per workgroup (a wave past N returns), 16 rows per iteration.
TN_ROWS = [
    # name, M, N, K             tiles = cdiv(N, 32) * cdiv(K, 32)
    ("tn_t1_m15", 15, 32, 32),    # 1 tile (== 1 mod 4): three idle waves; M 15 < one 16-row step
    ("tn_t2_m16", 16, 33, 32),    # 2 tiles (== 2 mod 4); M 16 = one step exactly
    ("tn_t3_m17", 17, 65, 31),    # 3 tiles (== 3 mod 4); M 17 = one row into step 2; K 31 < one tile
    ("tn_t9_m1", 1, 65, 65),      # 9 tiles (== 1 mod 4): workgroup 3 holds one live wave; M 1
    ("tn_t6_m33", 33, 40, 96),    # 6 tiles (== 2 mod 4), M 33
    ("tn_t15_m65", 65, 161, 96),  # 15 tiles (== 3 mod 4), M 65
    ("tn_t16_m512", 512, 64, 256),  # 16 tiles (== 0 mod 4), M 512: 32 steps
]


@pytest.mark.parametrize("row", TN_ROWS, ids=[r[0] for r in TN_ROWS])
def test_linear_tn(row):
    from gif_amd import ops
    name, M, N, K = row
    g = _rng(3)
    A, B = torch.randn(M, N, generator=g), torch.randn(M, K, generator=g)
    a, b = _strided(A, 4 + (-N) % 4), _strided(B, 8 + (-K) % 4)
    y1 = ops.linear_tn(a, b, 0.5)
    y2 = ops.linear_tn(a, b, 0.5)
    torch.cuda.synchronize()
    assert torch.equal(y1.view(torch.int32), y2.view(torch.int32)), f"{name}: second call differs"
    _check(y1, 0.5 * (A.double().T @ B.double()), 0.5 * (A.double().abs().T @ B.double().abs()), "gemm", name)


# ---------------------------------------------------------------------------------------------------------------------------------
# b. style path (ModulatedConv2d's demodulation: weight_sq_sum, style_demod, style_demod_bwd_s / _w, demod_wgrad)
# ---------------------------------------------------------------------------------------------------------------------------------
STYLE_ROWS = [
    # name, B, cout, cin, taps      (cout_pad = cout rounded up to 8, cin_pad = cin + 4)
    ("st_b1", 1, 31, 32, 9),       # B 1; cout 31 < one tile; cout * cin * taps = 8928, not a multiple of 256
    ("st_b31", 31, 32, 36, 1),     # B 31; cout 32 = one tile; cin 36: a half K chunk; taps 1
    ("st_b32", 32, 33, 64, 9),     # B 32 = one row tile; cout 33 crosses into tile 2
    ("st_b33", 33, 65, 68, 9),     # B 33: a second row tile; cin 68 crosses into a third 32-wide tile of bwd_s
    ("st_b65", 65, 64, 100, 1),    # B 65: three row tiles; cin 100 (% 8 == 4)
]


@pytest.mark.parametrize("row", STYLE_ROWS, ids=[r[0] for r in STYLE_ROWS])
def test_style_path(row):
    from gif_amd import ops
    name, B, cout, cin, taps = row
    g = _rng(4)
    kk = int(math.isqrt(taps))
    W = torch.randn(cout, cin, kk, kk, generator=g)
    S = torch.randn(B, cin, generator=g) + 1.0
    cout_pad, cin_pad = (cout + 7) // 8 * 8, cin + 4
    scale2, eps = 1.0 / (cin * taps), 1e-8
    Wd = W.double()
    # weight_sq_sum
    wsq = ops.weight_sq_sum(W.cuda())
    wsq_ref = Wd.pow(2).sum(dim=(2, 3))
    _check(wsq, wsq_ref, wsq_ref, "style", f"{name} weight_sq_sum")
    Wsq = wsq.cpu()  # the operand the following kernels read
    Wq = Wsq.double()
    # style_demod: s pad columns [cin, cin_pad) hold NaN (only [0, cin) is the operand)
    s_dev = _strided(S, cin_pad - cin)
    d = ops.style_demod(s_dev, wsq, scale2, eps, cout_pad)
    Sd = S.double()
    v = scale2 * (Sd.pow(2) @ Wq.T) + eps
    d_ref = v.rsqrt()
    R_d = 0.5 * d_ref.pow(3) * v
    _check(d[:, :cout], d_ref, R_d, "style", f"{name} style_demod", extra=2 * U32 * d_ref)
    assert (d[:, cout:] == 1).all(), f"{name}: d padding columns must be 1"
    D = d.cpu()
    # backward: gd [B, cout_pad], its padding columns hold NaN (the header: only [:, :Cout] is the operand)
    GD = torch.randn(B, cout_pad, generator=g)
    GD[:, cout:] = NAN
    gd = GD.cuda()
    gacc = GD[:, :cout].double() * (-0.5 * scale2) * D[:, :cout].double().pow(3)
    Racc = GD[:, :cout].double().abs() * (0.5 * scale2) * D[:, :cout].double().pow(3)
    s_full = torch.zeros(B, cin_pad)
    s_full[:, :cin] = S
    GSIN = torch.randn(B, cin_pad, generator=g)
    for gs_in in (None, GSIN):
        gs = ops.style_demod_bwd_s(gd, d, wsq, s_full.cuda(), None if gs_in is None else gs_in.cuda(), scale2)
        ref = 2 * Sd * (gacc @ Wq)
        R = 2 * Sd.abs() * (Racc @ Wq)
        if gs_in is not None:
            ref, R = ref + gs_in[:, :cin].double(), R + gs_in[:, :cin].double().abs()
        _check(gs[:, :cin], ref, R, "style", f"{name} style_demod_bwd_s{'' if gs_in is None else ' gs_in'}")
        assert (gs[:, cin:] == 0).all(), f"{name}: gs padding columns must be 0"
    gw = ops.style_demod_bwd_w(gd, d, s_dev, cout, cin, scale2)
    _check(gw, gacc.T @ Sd.pow(2), Racc.T @ Sd.pow(2), "style", f"{name} style_demod_bwd_w")
    GW = torch.randn(cout, cin, generator=g)
    gW = ops.demod_wgrad(W.cuda(), GW.cuda())
    ref = 2 * Wd * GW.double()[:, :, None, None]
    _check(gW, ref, ref.abs(), "style", f"{name} demod_wgrad")


# ---------------------------------------------------------------------------------------------------------------------------------
# c. modulation bank (linear_bank_fwd / linear_bank_bwd)
# ---------------------------------------------------------------------------------------------------------------------------------
BANK_ROWS = [
    # name, M, K, ldx extra, x_cols, widths
    # 40 segments (BANK_MAX): widths 8 / 16 / 24 share one 32-wide bank_find window; chunks 8+...: see the assertion below
    ("bank40_m1", 1, 36, 4, 40, [8, 16, 24, 40, 8, 16, 24, 520] * 5),
    ("bank_m33", 33, 512, 8, 520, [8, 520, 16, 24, 40]),   # K 512: 16 k tiles in the weight gradient (bias from tk == 0)
    ("bank_m65", 65, 32, 4, 36, [24, 8, 40, 16]),          # K 32: one k tile; x_cols 36 > K: padding columns of gx
    ("bank_m65_k68", 65, 68, 12, 72, [16, 8, 8, 520, 24]), # K 68: three k tiles, the last 4 wide; a half K chunk forward
]


@pytest.mark.parametrize("row", BANK_ROWS, ids=[r[0] for r in BANK_ROWS])
def test_linear_bank(row):
    from gif_amd import ops
    name, M, K, ldx_extra, x_cols, widths = row
    assert sum(widths) // 8 % 64 != 0, "the total chunk count must not be a multiple of 64"
    g = _rng(5)
    X = torch.randn(M, K, generator=g)
    Ws = [torch.randn(n, K, generator=g) for n in widths]
    Bs = [torch.randn(n, generator=g) if i % 3 else None for i, n in enumerate(widths)]
    GS = [torch.randn(M, n, generator=g) for n in widths]
    scale = 1 / math.sqrt(K)
    x = _strided(X, ldx_extra)  # ldx > K, gap NaN
    ws = [w.cuda() for w in Ws]
    bs = [None if b is None else b.cuda() for b in Bs]
    gss = [t.cuda() for t in GS]
    assert ops.linear_bank_ok(x, ws)
    outs = ops.linear_bank_fwd(x, ws, bs, scale)
    _poison(*widths, M * x_cols)
    gx, gws, gbs = ops.linear_bank_bwd(x, ws, gss, scale, True, True, True, x_cols=x_cols)
    torch.cuda.synchronize()
    Xd = X.double()
    gx_ref = torch.zeros(M, K, dtype=torch.float64)
    gx_R = torch.zeros(M, K, dtype=torch.float64)
    for i, (W, b, GSi) in enumerate(zip(Ws, Bs, GS)):
        what = f"{name} seg{i} n{W.shape[0]}"
        ref = scale * (Xd @ W.double().T) + (0 if b is None else b.double())
        R = scale * (Xd.abs() @ W.double().abs().T) + (0 if b is None else b.double().abs())
        _check(outs[i], ref, R, "bank", f"{what} fwd")
        # same body and order as linear_nt / linear_tn on the one segment: identical bits
        alone = ops.linear_nt(x, ws[i], bs[i], scale)
        assert torch.equal(outs[i].view(torch.int32), alone.view(torch.int32)), f"{what}: forward differs from linear_nt"
        _check(gws[i], scale * (GSi.double().T @ Xd), scale * (GSi.double().abs().T @ Xd.abs()), "bank", f"{what} gw")
        alone = ops.linear_tn(gss[i], x, scale)
        assert torch.equal(gws[i].view(torch.int32), alone.view(torch.int32)), f"{what}: weight gradient differs from linear_tn"
        _check(gbs[i], GSi.double().sum(0), GSi.double().abs().sum(0), "bank", f"{what} gbias")
        gx_ref += scale * (GSi.double() @ W.double())
        gx_R += scale * (GSi.double().abs() @ W.double().abs())
    _check(gx[:, :K], gx_ref, gx_R, "bank", f"{name} gx")
    assert (gx[:, K:] == 0).all(), f"{name}: gx padding columns must be zero"


def test_linear_bank_refuses_41_segments():
    from gif_amd import _lib, ops
    x = torch.randn(2, 8, device="cuda")
    ws = [torch.randn(8, 8, device="cuda") for _ in range(41)]
    assert ops.linear_bank_ok(x, ws[:40]) and not ops.linear_bank_ok(x, ws)
    with pytest.raises(_lib.GifHipError, match="segments"):
        ops.linear_bank_fwd(x, ws, [None] * 41, 1.0)
    with pytest.raises(_lib.GifHipError, match="segments"):
        ops.linear_bank_bwd(x, ws, [torch.zeros(2, 8, device="cuda")] * 41, 1.0, True, True, True)


# ---------------------------------------------------------------------------------------------------------------------------------
# d. routes in Python: EqualLinear, ModulatedConv2d.scales (fast style path), modulation_bank
# ---------------------------------------------------------------------------------------------------------------------------------
def _prof_begin():
    from gif_amd import ops
    ops.prof_enable(True)
    for fam in range(18):
        ops.prof_read(fam)  # (reading clears a family's records)


def _prof_conv_launches():
    from gif_amd import ops
    torch.cuda.synchronize()
    n = sum(ops.prof_read(fam)[2] for fam in range(18))
    ops.prof_enable(False)
    return n


EQL_ROWS = [
    # name, rows, in_dim, out_dim, skinny, bias + activation
    #   predicate: in_dim % 4 == 0 and rows <= _SKINNY_MAX_ROWS and pad4(out_dim) <= 1024
    ("eql_rows512", 512, 64, 40, True, True),      # rows 512 = _SKINNY_MAX_ROWS: skinny
    ("eql_rows513", 513, 64, 40, False, True),     # rows 513: the 1x1 convolution
    ("eql_in36", 8, 36, 33, True, True),           # in_dim % 4 == 0: skinny
    ("eql_in34", 8, 34, 33, False, True),          # in_dim % 4 == 2: convolution (input padded to 36)
    ("eql_out1024", 4, 32, 1024, True, True),      # pad4(out_dim) 1024: skinny
    # pad4(out_dim) 1028 > 1024: convolution.  Without bias and activation: the bias / activation backward of the convolution route
    # (bias_act_bwd) is limited to 1024 channels, which no layer of the model reaches
    ("eql_out1025", 4, 32, 1025, False, False),
]


@pytest.mark.parametrize("row", EQL_ROWS, ids=[r[0] for r in EQL_ROWS])
def test_equal_linear_route(row):
    from gif_amd import layers
    name, rows, ind, outd, skinny, epi = row
    assert layers._SKINNY_MAX_ROWS == 512
    torch.manual_seed(6)
    lin = layers.EqualLinear(ind, outd, bias=epi, bias_init=0.1, activation="fused_lrelu" if epi else None,
                             apply_sqrt2_fac_in_eq_lin=True)
    if epi:
        with torch.no_grad():
            lin.bias.normal_()
    lin = lin.cuda()
    g = _rng(6)
    X, GY = torch.randn(rows, ind, generator=g), torch.randn(rows, outd, generator=g)
    x = X.cuda().requires_grad_(True)
    _prof_begin()
    y = lin(x)
    y.backward(GY.cuda())
    n_conv = _prof_conv_launches()
    assert (n_conv > 0) == (not skinny), f"{name}: {n_conv} conv-family ops, expected the {'skinny' if skinny else 'conv'} route"
    W = lin.weight.detach().cpu().double()
    b = lin.bias.detach().cpu().double() if epi else torch.zeros(outd, dtype=torch.float64)
    Xd, sc = X.double(), lin.scale
    gain, slope = (math.sqrt(2), 0.2) if epi else (1.0, 1.0)
    pre = sc * (Xd @ W.T) + b
    Rp = sc * (Xd.abs() @ W.abs().T) + b.abs()
    amb = (pre.abs() <= TOL["route"] * Rp) & epi
    alt = torch.where(amb, torch.where(pre > 0, pre * slope, pre) * gain, torch.full_like(pre, NAN))
    _check(y, _lrelu(pre, slope, gain), Rp * gain, "route", f"{name} fwd", alt=alt)
    # gradients: an element whose branch is ambiguous contributes either slope: its whole magnitude is admitted as EXTRA
    gp = GY.double() * gain * torch.where(pre > 0, 1.0, slope) * ~amb
    gpR = GY.double().abs() * gain * ~amb
    gpA = GY.double().abs() * gain * amb
    _check(x.grad, sc * gp @ W, sc * gpR @ W.abs(), "route", f"{name} gx", extra=sc * gpA @ W.abs())
    if epi:
        _check(lin.bias.grad, gp.sum(0), gpR.sum(0), "route", f"{name} gbias", extra=gpA.sum(0))
    _check(lin.weight.grad, sc * gp.T @ Xd, sc * gpR.T @ Xd.abs(), "route", f"{name} gw", extra=sc * gpA.T @ Xd.abs())


def _style_ref(style, Wm, bm, scm, W, scale, eps, GS, GD, cin, cout):
    """fp64 s, d and the first-order gradients of <s, GS> + <d, GD> w.r.t. style, Wm, bm, W — signed values and their R."""
    s = scm * (style @ Wm.T) + bm
    sR = scm * (style.abs() @ Wm.abs().T) + bm.abs()
    wsq = W.pow(2).sum(dim=(2, 3))
    v = scale ** 2 * (s.pow(2) @ wsq.T) + eps
    d = v.rsqrt()
    dR = 0.5 * d.pow(3) * (scale ** 2 * ((s.abs() * sR * 2) @ wsq.T) + scale ** 2 * (s.pow(2) @ wsq.T))
    gacc = GD * (-0.5) * d.pow(3)
    gaR = GD.abs() * 0.5 * d.pow(3)
    gs = GS + 2 * s * (scale ** 2 * gacc @ wsq)
    gsR = GS.abs() + 2 * s.abs() * (scale ** 2 * gaR @ wsq)
    gwsq = scale ** 2 * gacc.T @ s.pow(2)
    gW = 2 * W * gwsq[:, :, None, None]
    gWR = 2 * W.abs() * (scale ** 2 * gaR.T @ s.pow(2))[:, :, None, None]
    return dict(s=(s, sR), d=(d, dR), style=(scm * gs @ Wm, scm * gsR @ Wm.abs()), Wm=(scm * gs.T @ style, scm * gsR.T @ style.abs()),
                bm=(gs.sum(0), gsR.sum(0)), W=(gW, gWR))


STYLE_ROUTE_ROWS = [
    # name, rows, cin, cout, bank     fast: rows <= 512 and cin % 4 == 0 (and in_act <= 1024); bank: >= 2 layers, n % 8 == 0 ...
    ("modc_fast", 8, 16, 24, False),      # fast style path (skinny GEMM + GF.demodulation), no bank
    ("modc_rows513", 513, 16, 24, False),  # rows 513 > _SKINNY_MAX_ROWS: EqualLinear on the convolution + torch demodulation
    ("modc_cin18", 8, 18, 24, False),     # cin % 4 == 2: not fast
    ("modc_bank", 8, 16, 24, True),       # two layers of width 16 / 24: the bank takes both
    ("modc_nobank12", 8, 12, 24, True),   # width 12 (% 8 == 4): linear_bank_ok refuses, each layer fast on its own
]


@pytest.mark.parametrize("row", STYLE_ROUTE_ROWS, ids=[r[0] for r in STYLE_ROUTE_ROWS])
def test_modulated_conv_style_route(row):
    from gif_amd import layers
    name, rows, cin, cout, bank = row
    torch.manual_seed(7)
    sdim = 32
    convs = [layers.ModulatedConv2d(cin, cout, 3, sdim).cuda()]
    if bank:
        convs.append(layers.ModulatedConv2d(24, cout, 3, sdim).cuda())
    for c in convs:
        with torch.no_grad():
            c.modulation.bias.normal_(1.0, 0.3)
    g = _rng(7)
    ST = torch.randn(rows, sdim, generator=g)
    style = ST.cuda().requires_grad_(True)
    _prof_begin()
    if bank:
        layers.modulation_bank(convs, style)
        took = [c._banked is not None for c in convs]
        assert all(took) == (cin % 8 == 0), f"{name}: bank taken {took}"
    outs = [c.scales(style) for c in convs]
    GSs = [torch.randn(rows, c.in_channel, generator=g) for c in convs]
    GDs = [torch.randn(rows, c.out_channel, generator=g) for c in convs]
    loss = sum((s[:, :c.in_channel] * G.cuda()).sum() + (d[:, :c.out_channel] * H.cuda()).sum()
               for c, (s, d), G, H in zip(convs, outs, GSs, GDs))
    loss.backward()
    n_conv = _prof_conv_launches()
    fast = rows <= 512 and cin % 4 == 0
    assert (n_conv > 0) == (not fast), f"{name}: {n_conv} conv-family ops with fast = {fast}"
    gst_ref = torch.zeros(rows, sdim, dtype=torch.float64)
    gst_R = torch.zeros(rows, sdim, dtype=torch.float64)
    for i, (c, (s, d), G, H) in enumerate(zip(convs, outs, GSs, GDs)):
        m = c.modulation
        ref = _style_ref(ST.double(), m.weight.detach().cpu().double(), m.bias.detach().cpu().double(), m.scale,
                         c.weight.detach().cpu().double().squeeze(0), c.scale, c.eps, G.double(), H.double(), c.in_channel,
                         c.out_channel)
        _check(s[:, :c.in_channel], *ref["s"], "route", f"{name} l{i} s")
        _check(d[:, :c.out_channel], *ref["d"], "route", f"{name} l{i} d", extra=2 * U32 * ref["d"][0])
        _check(m.weight.grad, *ref["Wm"], "route", f"{name} l{i} g_modw")
        _check(m.bias.grad, *ref["bm"], "route", f"{name} l{i} g_modb")
        _check(c.weight.grad.squeeze(0), *ref["W"], "route", f"{name} l{i} g_w")
        gst_ref += ref["style"][0]
        gst_R += ref["style"][1]
    _check(style.grad, gst_ref, gst_R, "route", f"{name} g_style")


# ---------------------------------------------------------------------------------------------------------------------------------
# e. column sums (colsum, bias_act_bwd, mul_reduce, act_inv_mul_reduce), fp32 and f16
# ---------------------------------------------------------------------------------------------------------------------------------
def _blocks(npix, C):
    R = 256 // (C // 4)
    return min(max(-(-npix // (R * 16)), 1), 512)


def _npix(nblk, C):
    return nblk * (256 // (C // 4)) * 16


COLSUM_ROWS = [
    # name, B, C, H, W       (npix = B*H*W; colsum_blocks = min(cdiv(npix, R*16), 512), R = 256 / (C/4))
    ("cs_blk511", 1, 64, 1, _npix(511, 64)),        # 511 workgroups
    ("cs_blk512", 1, 64, 1, _npix(512, 64)),        # 512 = the cap exactly
    ("cs_blk513", 1, 64, 1, _npix(512, 64) + 1),    # 513 wanted: capped at 512, rows_per_block grows to 17 per row lane
    ("cs_nblk31", 2, 36, 1, _npix(31, 36) // 2),    # stage 2 nblk 31: the unrolled loop never runs (k + 28 < 31 fails for rl 3)
    ("cs_nblk32", 1, 1024, 1, _npix(32, 1024)),     # nblk 32 = one unrolled pass; C 1024: R = 1
    ("cs_nblk33", 3, 12, 1, _npix(33, 12) // 3),    # nblk 33: one pass + a tail row; C4 3 does not divide 256 (R 85, 1 idle thread)
    ("cs_nblk33_c24", 1, 24, 1, _npix(33, 24)),     # nblk 33 again with C % 8 == 0 (f16 too); C4 6 does not divide 256 (R 42)
    ("cs_nblk36", 1, 24, 1, _npix(36, 24)),         # nblk 36: tail of 4
    ("cs_c4", 2, 4, 5, 7),                          # C 4: R 256; one block, fewer rows than row lanes
    ("cs_c1020", 4, 1020, 3, 5),                    # C4 255: R 1, one idle thread
    ("cs_c1016", 2, 1016, 3, 5),                    # C4 254: R 1, two idle threads (C % 8 == 0: f16 too)
]


def _nhwc(x, dtype=torch.float32):
    return x.to(dtype).cuda().contiguous(memory_format=CL)


# f16 activations carry a multiple of 8 channels (ops.cpad): the f16 rows are the ones with C % 8 == 0
COLSUM_CASES = [pytest.param(r, d, id=f"{r[0]}-{n}") for r in COLSUM_ROWS for d, n in ((torch.float32, "f32"), (H16, "f16"))
                if d == torch.float32 or r[2] % 8 == 0]


@pytest.mark.parametrize("row,dtype", COLSUM_CASES)
def test_column_sums(row, dtype):
    from gif_amd import ops
    name, B, C, H, W = row
    f16 = dtype == H16
    fam = "sum16" if f16 else "sum32"
    tag = f"{name} {'f16' if f16 else 'f32'}"
    g = _rng(8)
    X = torch.randn(B, C, H, W, generator=g).to(dtype)  # (f16: the half-rounded operands are the reference's)
    Y = torch.randn(B, C, H, W, generator=g).to(dtype)
    Xd, Yd = X.double(), Y.double()
    x, y = _nhwc(X, dtype), _nhwc(Y, dtype)
    # colsum
    _poison(C)
    _check(ops.colsum(x), Xd.sum(dim=(0, 2, 3)), Xd.abs().sum(dim=(0, 2, 3)), fam, f"{tag} colsum")
    # bias_act_bwd: gx = gy * gain * (y > 0 ? 1 : slope) (stored in the activation dtype), gbias = its column sums
    for slope, gain in ((0.2, math.sqrt(2)), (1.0, 1.0)):
        _poison(C)
        gx, gb = ops.bias_act_bwd(x, y, True, slope, gain)
        ref = Xd * gain * torch.where(Yd > 0, 1.0, slope)
        if f16:
            _check(gx, ref, ref.abs(), "ew16", f"{tag} bias_act_bwd gx s{slope}", extra=torch.full_like(ref, 2.0 ** -25))
        else:
            _check(gx, ref, ref.abs(), fam, f"{tag} bias_act_bwd gx s{slope}")
        _check(gb, ref.sum(dim=(0, 2, 3)), ref.abs().sum(dim=(0, 2, 3)), fam, f"{tag} bias_act_bwd gbias s{slope}")
    # mul_reduce with the scaled output
    SC = torch.randn(B, C, generator=g)
    _poison(B * C)
    out, scaled = ops.mul_reduce(x, y, SC.cuda(), want_scaled=True)
    _check(out, (Xd * Yd).sum(dim=(2, 3)), (Xd * Yd).abs().sum(dim=(2, 3)), fam, f"{tag} mul_reduce")
    ref = SC.double()[:, :, None, None] * Xd
    if f16:
        _check(scaled, ref, ref.abs(), "ew16", f"{tag} mul_reduce scaled", extra=torch.full_like(ref, 2.0 ** -25))
    else:
        _check(scaled, ref, ref.abs(), fam, f"{tag} mul_reduce scaled")
    # act_inv_mul_reduce: out[b, c] = sum_hw g * (act^-1(y) - residual - bias[c])
    RES = torch.randn(B, C, H, W, generator=g).to(dtype)
    BIAS = torch.randn(C, generator=g)
    for res, bias, slope, gain in ((None, None, 0.2, math.sqrt(2)), (RES, None, 0.5, 1.0), (None, BIAS, 0.2, 2.0),
                                   (RES, BIAS, 1.0, math.sqrt(2))):
        _poison(B * C)
        out = ops.act_inv_mul_reduce(x, y, None if res is None else _nhwc(res, dtype), None if bias is None else bias.cuda(),
                                     slope, gain)
        inv = Yd * torch.where(Yd > 0, 1.0 / gain, 1.0 / (gain * slope))
        e, eR = inv, inv.abs()
        if res is not None:
            e, eR = e - res.double(), eR + res.double().abs()
        if bias is not None:
            e, eR = e - bias.double()[None, :, None, None], eR + bias.double().abs()[None, :, None, None]
        _check(out, (Xd * e).sum(dim=(2, 3)), (Xd.abs() * eR).sum(dim=(2, 3)), fam,
               f"{tag} act_inv_mul_reduce res{res is not None} bias{bias is not None} s{slope} g{gain:.3f}")


@pytest.mark.parametrize("HW", [8192, 8193])
def test_mul_reduce_chunk_cap(HW):
    """mul_reduce_chunks = min(colsum_blocks(HW, 32), 64): HW 8192 -> exactly 64 chunks, 8193 -> capped (65 wanted)."""
    from gif_amd import _lib, ops
    assert _lib.load().gif_mul_reduce_chunks(HW) == 64
    g = _rng(9)
    B, C = 2, 36
    X, Y = torch.randn(B, C, 1, HW, generator=g), torch.randn(B, C, 1, HW, generator=g)
    Xd, Yd = X.double(), Y.double()
    x, y = _nhwc(X), _nhwc(Y)
    out, _ = ops.mul_reduce(x, y)
    _check(out, (Xd * Yd).sum(dim=(2, 3)), (Xd * Yd).abs().sum(dim=(2, 3)), "sum32", f"mul_reduce HW{HW}")
    out = ops.act_inv_mul_reduce(x, y, None, None, 0.2, math.sqrt(2))
    inv = Yd * torch.where(Yd > 0, 1 / math.sqrt(2), 1 / (0.2 * math.sqrt(2)))
    _check(out, (Xd * inv).sum(dim=(2, 3)), (Xd * inv).abs().sum(dim=(2, 3)), "sum32", f"act_inv_mul_reduce HW{HW}")


def test_column_sums_empty():
    """npix = 0 / B = 0: nothing out of range; a column sum over no rows is zero (bias gradient included)."""
    from gif_amd import ops
    C = 12
    x = torch.zeros(0, C, 4, 4, device="cuda").contiguous(memory_format=CL)
    _poison(C)
    assert torch.equal(ops.colsum(x).cpu(), torch.zeros(C))
    _poison(C)
    gx, gb = ops.bias_act_bwd(x, x, True)
    assert gx.shape == x.shape and torch.equal(gb.cpu(), torch.zeros(C))
    out, scaled = ops.mul_reduce(x, x, torch.zeros(0, C, device="cuda"), want_scaled=True)
    assert out.shape == (0, C) and scaled.shape == x.shape
    assert ops.act_inv_mul_reduce(x, x, None, None, 0.2, 1.0).shape == (0, C)


# ---------------------------------------------------------------------------------------------------------------------------------
# f. per-sample kernels: sqnorm, minibatch stddev, bilinear_down, texture pair loss
# ---------------------------------------------------------------------------------------------------------------------------------
SQNORM_ROWS = [
    # name, B, n        (1024 threads x float4 = 4096 floats per pass; rows start 16-byte aligned iff n % 4 == 0)
    ("sq_n4096", 3, 4096),    # n % 4 == 0: float4 loop, exactly one pass
    ("sq_n4097", 3, 4097),    # n % 4 == 1: rows 1, 2 misaligned -> scalar loop; n > 4096
    ("sq_n4094", 4, 4094),    # n % 4 == 2
    ("sq_n4095", 3, 4095),    # n % 4 == 3, just below one pass
    ("sq_n4100", 3, 4100),    # n % 4 == 0, one float4 into pass 2
    ("sq_n1001", 5, 1001),    # n % 4 == 1, fewer elements than threads
    ("sq_n10003", 3, 10003),  # n % 4 == 3, three passes
]


def _hash_input(B, n):
    """Deterministic fp32 values without a random generator: multiples of 1/256 in [-2, 2)."""
    i = np.arange(B * n, dtype=np.int64)
    return torch.from_numpy((((i * 2654435761) % 1021) - 510).astype(np.float32) / 256.0).reshape(B, n)


@pytest.mark.parametrize("row", SQNORM_ROWS, ids=[r[0] for r in SQNORM_ROWS])
def test_sqnorm_per_sample(row):
    from gif_amd import ops
    name, B, n = row
    G = torch.randn(B, n, generator=_rng(10))
    out = ops.sqnorm_per_sample(G.cuda())
    ref = G.double().pow(2).sum(1)
    _check(out, ref, ref, "sample", name)


def test_sqnorm_aligned_bits_unchanged():
    """n % 4 == 0 keeps the float4 loop and its summation order: the bits equal those the kernel produced before the alignment
    check was added (tests/golden/sqnorm_aligned_bits.npy, computed on an MI355X from these hashed inputs)."""
    from gif_amd import ops
    want = np.load(os.path.join(GOLDEN, "sqnorm_aligned_bits.npy"))
    got = []
    for B, n in ((3, 4096), (3, 4100), (2, 65536)):
        got.append(ops.sqnorm_per_sample(_hash_input(B, n).cuda()).cpu().view(torch.int32).numpy())
    assert np.array_equal(np.concatenate(got), want.view(np.int32))


MBSTD_ROWS = [
    # name, B, G, C, Cy, H, W      (M = B / G groups; y[..., C] = stat, y[..., C+1:] = 0)
    ("mb_g1", 3, 1, 8, 12, 4, 4),      # G 1: variance 0, sd = 1e-4
    ("mb_g2", 6, 2, 12, 16, 4, 4),     # G 2, M 3
    ("mb_g4", 8, 4, 16, 24, 15, 20),   # G 4, M 2; H*W 300: every thread loops (n = 4800 > 256); Cy = C + 8
    ("mb_g8", 16, 8, 8, 12, 4, 4),     # G 8 = the size of xv[8]; M 2
    ("mb_g8_hw300", 8, 8, 4, 8, 15, 20),  # G 8, M 1, H*W 300
]


@pytest.mark.parametrize("row", MBSTD_ROWS, ids=[r[0] for r in MBSTD_ROWS])
def test_minibatch_stddev_kernels(row):
    from gif_amd import ops
    name, B, G, C, Cy, H, W = row
    M = B // G
    g = _rng(11)
    X = torch.randn(B, C, H, W, generator=g) * 0.7 + 0.3
    GY = torch.randn(B, Cy, H, W, generator=g)
    y, stat = ops.mbstd_fwd(_nhwc(X), G, Cy)
    Xd = X.double()
    xg = Xd.reshape(G, M, C, H, W)
    mean = xg.mean(0)
    dev_ = xg - mean
    var = dev_.pow(2).mean(0)
    sd = (var + 1e-8).sqrt()
    n = C * H * W
    stat_ref = sd.mean(dim=(1, 2, 3))
    varR = (xg.abs() + mean.abs()).pow(2).mean(0)
    sdR = 0.5 * varR / sd + sd
    _check(stat, stat_ref, sdR.mean(dim=(1, 2, 3)), "sample", f"{name} stat")
    yc = y.cpu()
    assert torch.equal(yc[:, :C], X), f"{name}: y[:, :C] must be a copy of x"
    stat_b = stat_ref[torch.arange(B) % M]
    _check(yc[:, C], stat_b[:, None, None].expand(B, H, W), sdR.mean(dim=(1, 2, 3))[torch.arange(B) % M][:, None, None].expand(B, H, W),
           "sample", f"{name} y stat channel")
    assert (yc[:, C + 1:] == 0).all(), f"{name}: channels past C + 1 must be zero"
    # backward
    gx = ops.mbstd_bwd(_nhwc(X), _nhwc(GY), G)
    GYd = GY.double()
    gstat = GYd[:, C].reshape(G, M, H, W).sum(dim=(0, 2, 3))  # [M]
    gstatR = GYd[:, C].abs().reshape(G, M, H, W).sum(dim=(0, 2, 3))
    k = (gstat / n)[None, :, None, None, None] / (G * sd)[None]
    kR = (gstatR / n)[None, :, None, None, None] / (G * sd)[None] * (1 + sdR[None] / sd[None])
    ref = GYd[:, :C].reshape(G, M, C, H, W) + k * dev_
    R = GYd[:, :C].abs().reshape(G, M, C, H, W) + kR * (xg.abs() + mean.abs())
    _check(gx, ref.reshape(B, C, H, W), R.reshape(B, C, H, W), "sample", f"{name} bwd")


def test_minibatch_stddev_rejects_unaligned_channels():
    """mbstd_write_kernel loads x[pix * C + c] as float4: C % 4 != 0 is refused before any launch."""
    from gif_amd import _lib, ops
    x = torch.zeros(4, 6, 4, 4, device="cuda").contiguous(memory_format=CL)
    with pytest.raises(_lib.GifHipError, match="multiple"):
        ops.mbstd_fwd(x, 2, 8)
    with pytest.raises(_lib.GifHipError, match="multiple"):
        ops.mbstd_bwd(x, torch.zeros(4, 8, 4, 4, device="cuda").contiguous(memory_format=CL), 2)


@pytest.mark.parametrize("f", [1, 2, 4, 8])
def test_bilinear_down(f):
    from gif_amd import ops
    B, C, S = 3, 12, 5
    R = S * f
    g = _rng(12)
    X = torch.randn(B, C, R, R, generator=g)
    Xd = X.double().requires_grad_(True)
    ref = F.interpolate(Xd, size=(S, S), mode="bilinear", align_corners=False)
    Rr = F.interpolate(X.double().abs(), size=(S, S), mode="bilinear", align_corners=False)
    y = ops.bilinear_down(_nhwc(X), S)
    _check(y, ref.detach(), Rr, "sample", f"bilinear_down f{f}")
    GY = torch.randn(B, C, S, S, generator=g)
    (gref,) = torch.autograd.grad(ref, Xd, GY.double())
    Xa = X.double().requires_grad_(True)
    (gR,) = torch.autograd.grad(F.interpolate(Xa, size=(S, S), mode="bilinear", align_corners=False), Xa, GY.double().abs())
    gx = ops.bilinear_down(_nhwc(GY), S, backward_to=R)
    _check(gx, gref, gR, "sample", f"bilinear_down_bwd f{f}")


TEX_ROWS = [
    # name, C, H, W        (n = C*H*W; stage 1 blocks = min(cdiv(n, 256), 1024))
    ("tex_small", 3, 17, 17),      # n 867: 4 blocks; HW 289 not a multiple of 256
    ("tex_1024", 4, 256, 256),     # n 262144 = 1024 x 256: the cap exactly, no striding
    ("tex_stride", 3, 300, 300),   # n 270000 > 262144: the grid strides; HW 90000 not a multiple of 256
]


@pytest.mark.parametrize("masks", ["none", "a", "ab"])
@pytest.mark.parametrize("row", TEX_ROWS, ids=[r[0] for r in TEX_ROWS])
def test_texture_pair_loss(row, masks):
    from gif_amd import ops
    name, C, H, W = row
    g = _rng(13)
    A, Bt = torch.rand(C, H, W, generator=g) * 2 - 1, torch.rand(C, H, W, generator=g) * 2 - 1
    Fm = torch.rand(H, W, generator=g)
    ma = torch.rand(H, W, generator=g) > 0.3 if "a" in masks else None
    mb = torch.rand(H, W, generator=g) > 0.3 if "b" in masks else None
    dev = lambda t: None if t is None else t.cuda()  # noqa: E731
    loss = ops.texture_pair_loss(A.cuda(), Bt.cuda(), dev(ma), dev(mb), Fm.cuda())
    vis = torch.ones(H, W, dtype=torch.bool)
    for m in (ma, mb):
        if m is not None:
            vis &= m
    d = (A.double() - Bt.double()) * vis
    s = torch.sigmoid(d * d)
    Fd = Fm.double()
    n = C * H * W
    ref = (s * Fd).sum() / n
    Rl = ((s + 2 * d * d * s * (1 - s)) * Fd).sum() / n
    _check(loss, ref, Rl, "sample", f"{name} {masks} loss")
    gl = torch.tensor(1.7)
    ga = ops.texture_pair_loss(A.cuda(), Bt.cuda(), dev(ma), dev(mb), Fm.cuda(), gloss=gl.cuda())
    gref = 1.7 / n * Fd * s * (1 - s) * 2 * d
    gR = 1.7 / n * Fd * 2 * d.abs() * s * (1 - s) * (1 + 2 * d * d)
    extra = 1.7 / n * Fd * 2 * d.abs() * s * 4 * U32  # (1 - s) computed in fp32 from s: absolute rounding of a few ulp of 1
    _check(ga, gref, gR, "sample", f"{name} {masks} grad", extra=extra)


# ---------------------------------------------------------------------------------------------------------------------------------
# g. fused Adam + EMA (FlatAdam.step) against torch's single-tensor Adam restated in fp64
# ---------------------------------------------------------------------------------------------------------------------------------
ADAM_ROWS = [
    # name, parameter sizes, misaligned index or None, ema
    ("adam_tails_ema", [5, 4097, 8190, 3, 4096], None, True),   # n % 4 in {1, 1, 2, 3, 0}; 4097 / 8190: two 4096-float chunks
    ("adam_tails", [7, 12289, 2], None, False),                 # EMA off; 12289: three full chunks + 1 element
    ("adam_scalar_ema", [6, 4101], 1, True),                    # parameter 1 starts 4 bytes past a 16-byte boundary: scalar branch
]


_f32, _adam_ref = adam_ref.f32, adam_ref.adam_ref  # (shared with test_gpu_resume)


@pytest.mark.parametrize("row", ADAM_ROWS, ids=[r[0] for r in ADAM_ROWS])
def test_flat_adam(row):
    from gif_amd.optim import FlatAdam
    from gif_amd.train_step import FlatGradBucket
    name, sizes, mis, ema_on = row
    g = _rng(14)
    params, bases = [], []
    for i, n in enumerate(sizes):
        if i == mis:
            base = torch.randn(n + 4, generator=g).cuda()
            bases.append(base)
            p = torch.nn.Parameter(base[1:1 + n])
            assert p.is_contiguous() and p.data_ptr() % 16 == 4
        else:
            p = torch.nn.Parameter(torch.randn(n, generator=g).cuda())
        params.append(p)
    emas = [torch.nn.Parameter(p.detach().clone() + 0.01) for p in params]
    lr, b1, b2, eps, decay = 2e-3, 0.5, 0.99, 1e-8, 0.9
    bucket = FlatGradBucket(params)
    opt = FlatAdam(params, lr=lr, betas=(b1, b2), eps=eps, bucket=bucket, ema_params=emas if ema_on else None)
    inv = torch.tensor(0.25, device="cuda")
    found = torch.zeros((), device="cuda")
    t = 0
    for step in range(4):
        grads = [torch.randn(n, generator=g) * (4.0 if step >= 2 else 1.0) for n in sizes]
        for view, gr in zip(bucket.views, grads):
            view.copy_(gr.view_as(view))
        before = [(p.detach().cpu().double(), opt.state[p]["exp_avg"].cpu().double(), opt.state[p]["exp_avg_sq"].cpu().double(),
                   e.detach().cpu().double()) for p, e in zip(params, emas)]
        bits = [x.detach().clone() for p, e in zip(params, emas) for x in (p, opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"], e)]
        scaled = step >= 2  # steps 2, 3: loss-scaled (inv_grad_scale 0.25); step 3 overflowed (found_inf 1)
        if step == 3:
            found.fill_(1.0)
        opt.step(ema_decay=decay if ema_on else None, inv_grad_scale=inv if scaled else None, found_inf=found if scaled else None)
        torch.cuda.synchronize()
        if step == 3:
            after = [x for p, e in zip(params, emas) for x in (p, opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"], e)]
            for a, b in zip(bits, after):
                assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{name}: a found_inf step changed a buffer"
            continue
        t += 1
        for i, (p, e, gr, (p0, m0, v0, e0)) in enumerate(zip(params, emas, grads, before)):
            gd = gr.double() * (0.25 if scaled else 1.0)
            pr, mr, vr, upd = _adam_ref(p0, gd, m0, v0, t, lr, b1, b2, eps, scaled)
            what = f"{name} step{step} p{i} n{sizes[i]}"
            Rm, Rv, Rp = adam_ref.adam_bounds(p0, gd, m0, vr, upd)  # |m0| + |g|, |v|, |p0| + 4 |upd|
            _check(opt.state[p]["exp_avg"], mr, Rm, "adam", f"{what} m")
            _check(opt.state[p]["exp_avg_sq"], vr, Rv, "adam", f"{what} v")
            _check(p, pr, Rp, "adam", f"{what} p")
            if ema_on:
                df = _f32(decay)
                er = e0 * df + (1 - df) * p.detach().cpu().double()  # (the kernel blends its own new p)
                _check(e, er, e0.abs() * df + (1 - df) * p.detach().cpu().double().abs(), "adam", f"{what} ema")
            else:
                assert torch.equal(e.detach().cpu().double(), e0), f"{what}: EMA written with EMA off"
    del bases
