"""-m gpu: the FIR outputs, column sums, per-sample products and texture losses of the route rows are bit-identical to the recorded ones.

Every kernel behind these ops sums in a fixed order, so a change of the host-side dispatch (csrc/ew_route.h, the launch code of
csrc/elementwise.hip) that keeps every kernel, grid and reduction stage must keep every bit.  Cases: each row of
test_gpu_conv_routes.FIR_ROWS in each dtype it runs (the output and, where the row fuses one, the column sum), colsum / bias_act_bwd /
mul_reduce / act_inv_mul_reduce over each row and dtype of test_gpu_linear_reduce_routes.COLSUM_ROWS, and the loss and gradient of each
row of its TEX_ROWS per mask set — on those tests' operands (same seeds, same draws), without their fp64 references.
tests/golden/pointwise_crc_golden.json holds the CRC-32 of each result's bytes, written by tests/golden/make_pointwise_crc_golden.py from
the commit before the route header (two runs agreed on every case)."""
import json
import math
import os
import zlib

import pytest
import torch

import test_gpu_conv_routes as routes  # (pytest puts this directory on sys.path)
import test_gpu_linear_reduce_routes as sums

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pointwise_crc_golden.json")
H16, CL = routes.H16, routes.CL
DT = {"f32": torch.float32, "f16": H16}
MASKS = ("none", "a", "ab")

# (kind, row name, dtype name or mask set) and the results each case checks
CASES = ([("fir", r.name, dt) for r in routes.FIR_ROWS for dt in DT if not (dt == "f16" and r.C % 8)] +
         [("sum", r[0], dt) for r in sums.COLSUM_ROWS for dt in DT if dt == "f32" or r[2] % 8 == 0] +
         [("tex", r[0], m) for r in sums.TEX_ROWS for m in MASKS])
OUTPUTS = {"sum": ("colsum", "bias_act_bwd_gx", "bias_act_bwd_gbias", "mul_reduce", "mul_reduce_scaled", "act_inv_mul_reduce"),
           "tex": ("loss", "grad")}


def case_id(kind, name, variant):
    return f"{kind}-{name}-{variant}"


def outputs(kind, name, variant):
    if kind == "fir":
        row = next(r for r in routes.FIR_ROWS if r.name == name)
        return ("out", "colsum") if row.epi == "fuse" else ("out",)
    return OUTPUTS[kind]


def _crc(t):
    torch.cuda.synchronize()
    return zlib.crc32(t.detach().contiguous().cpu().numpy().tobytes())


def _fir(name, dtname):
    """The operands of test_gpu_conv_routes.test_fir_route_vs_fp64 (same generator, same order of draws)."""
    from gif_amd import ops
    row = next(r for r in routes.FIR_ROWS if r.name == name)
    dt = DT[dtname]
    g = torch.Generator().manual_seed(zlib.crc32(repr(row).encode()))
    r16 = (lambda t: t.to(H16).float()) if dt == H16 else (lambda t: t)
    x = r16(torch.randn(row.B, row.C, row.H, row.W, generator=g))
    k = torch.rand(4, 4, generator=g) + 0.25
    k = k / k.sum() * row.up ** 2
    Ho, Wo = row.out
    kw, fuse = {}, None
    if row.epi == "bra":
        bias = torch.randn(row.C, generator=g)
        res = r16(torch.randn(row.B, row.C, Ho, Wo, generator=g))
        kw = dict(bias=bias.cuda(), residual=res.to(dt).cuda().contiguous(memory_format=CL), act=True)
    if row.epi == "fuse":
        m = r16(torch.randn(row.B, row.C, Ho, Wo, generator=g))
        fuse = ops.GradFuse(mask_src=m.to(dt).cuda().contiguous(memory_format=CL), mask_slope=0.2, mask_gain=2 ** 0.5, want_colsum=True)
        kw = dict(fuse=fuse)
    y = ops.upfirdn2d(x.to(dt).cuda().contiguous(memory_format=CL), k.cuda(), row.up, row.down, row.pad0, (Ho, Wo), **kw)
    assert y.shape == (row.B, row.C, Ho, Wo) and y.dtype == dt
    out = {"out": _crc(y)}
    if fuse is not None:
        assert fuse.colsum.shape == (row.C,) and fuse.colsum.dtype == torch.float32
        out["colsum"] = _crc(fuse.colsum)
    return out


def _sum(name, dtname):
    """The operands of test_gpu_linear_reduce_routes.test_column_sums; each op once (its first activation, residual and bias given)."""
    from gif_amd import ops
    _, B, C, H, W = next(r for r in sums.COLSUM_ROWS if r[0] == name)
    dtype = DT[dtname]
    g = sums._rng(8)
    X = torch.randn(B, C, H, W, generator=g).to(dtype)
    Y = torch.randn(B, C, H, W, generator=g).to(dtype)
    x, y = sums._nhwc(X, dtype), sums._nhwc(Y, dtype)
    out = {"colsum": _crc(ops.colsum(x))}
    gx, gb = ops.bias_act_bwd(x, y, True, 0.2, math.sqrt(2))
    out["bias_act_bwd_gx"], out["bias_act_bwd_gbias"] = _crc(gx), _crc(gb)
    SC = torch.randn(B, C, generator=g)
    red, scaled = ops.mul_reduce(x, y, SC.cuda(), want_scaled=True)
    out["mul_reduce"], out["mul_reduce_scaled"] = _crc(red), _crc(scaled)
    RES = torch.randn(B, C, H, W, generator=g).to(dtype)
    BIAS = torch.randn(C, generator=g)
    out["act_inv_mul_reduce"] = _crc(ops.act_inv_mul_reduce(x, y, sums._nhwc(RES, dtype), BIAS.cuda(), 0.2, math.sqrt(2)))
    return out


def _tex(name, masks):
    """The operands of test_gpu_linear_reduce_routes.test_texture_pair_loss."""
    from gif_amd import ops
    _, C, H, W = next(r for r in sums.TEX_ROWS if r[0] == name)
    g = sums._rng(13)
    A, Bt = torch.rand(C, H, W, generator=g) * 2 - 1, torch.rand(C, H, W, generator=g) * 2 - 1
    Fm = torch.rand(H, W, generator=g)
    ma = torch.rand(H, W, generator=g) > 0.3 if "a" in masks else None
    mb = torch.rand(H, W, generator=g) > 0.3 if "b" in masks else None
    dev = lambda t: None if t is None else t.cuda()  # noqa: E731
    loss = ops.texture_pair_loss(A.cuda(), Bt.cuda(), dev(ma), dev(mb), Fm.cuda())
    ga = ops.texture_pair_loss(A.cuda(), Bt.cuda(), dev(ma), dev(mb), Fm.cuda(), gloss=torch.tensor(1.7).cuda())
    assert ga.shape == (C, H, W)
    return {"loss": _crc(loss), "grad": _crc(ga)}


def pointwise_crcs(kind, name, variant):
    """result name -> CRC-32 of its bytes, for one case."""
    got = {"fir": _fir, "sum": _sum, "tex": _tex}[kind](name, variant)
    assert tuple(got) == outputs(kind, name, variant)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("kind,name,variant", CASES, ids=[case_id(*c) for c in CASES])
def test_pointwise_bits_match_the_recorded_ones(kind, name, variant):
    with open(GOLDEN) as f:
        golden = json.load(f)
    cid = case_id(kind, name, variant)
    assert cid in golden, f"{cid}: no recorded CRCs (tests/golden/make_pointwise_crc_golden.py)"
    got = pointwise_crcs(kind, name, variant)
    bad = {k: (f"{v:#010x}", f"{golden[cid][k]:#010x}") for k, v in got.items() if v != golden[cid][k]}
    assert not bad, f"{cid}: (CRC, recorded) {bad}: the bits changed"


def test_every_case_is_recorded():
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert sorted(golden) == sorted(case_id(*c) for c in CASES)
    for c in CASES:
        assert sorted(golden[case_id(*c)]) == sorted(outputs(*c)), c
