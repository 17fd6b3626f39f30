"""-m gpu: the weight gradients of the route table are bit-identical to the recorded ones.

With the split count fixed every weight-gradient kernel reduces in a fixed order, so a change of the host-side dispatch (csrc/wgrad_route.h,
the launch code of csrc/conv_wgrad.hip) that keeps every route must keep every bit.  Cases: each `wgrad` row of test_gpu_conv_routes.ROWS in
each mode it lists, on that module's operands, plus one modulated call per mode (per-sample scales on both sides of the wg_x3 geometry:
Hs*Ws = 272 is a multiple of 16 but not of 32, the 16-pixel-stage scale-table kernels).  tests/golden/wgrad_crc_golden.json holds the CRC-32
of each result's bytes, written by tests/golden/make_wgrad_crc_golden.py from the commit before the route header (two runs agreed on every
case)."""
import json
import os
import zlib

import pytest
import torch

import test_gpu_conv_routes as routes  # (pytest puts this directory on sys.path)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wgrad_crc_golden.json")
MODES = ("f16x2", "bf16x3", "native", "f16")
SCALED_ROW = "wg_x3"
CASES = [(r.name, m, False) for r in routes.ROWS if r.op == "wgrad" for m in r.fams] + [(SCALED_ROW, m, True) for m in MODES]


def case_id(name, mode, scaled):
    return f"{name}{'_scaled' if scaled else ''}-{mode}"


def wgrad_crc(name, mode, scaled):
    """CRC-32 of ops.conv_wgrad's result for one case (the contraction mode is restored afterwards)."""
    from gif_amd import ops
    row = next(r for r in routes.ROWS if r.name == name)
    B, Ci, Co, K, s, p, H, W = row.shape
    f16 = mode == "f16"
    dt = torch.float16 if f16 else torch.float32
    saved = ops.get_fp32_mfma_mode()
    try:
        if not f16:
            ops.set_fp32_mfma_mode(mode)
        o = routes._operands(row, f16)
        cs, cb = routes.cpad(Co, f16), routes.cpad(Ci, f16)
        kw = {}
        if scaled:
            g = torch.Generator().manual_seed(zlib.crc32(repr((row.shape, "scales")).encode()))
            kw = dict(small_scale=(torch.rand(B, cs, generator=g) + 0.5).cuda(), big_scale=(torch.rand(B, cb, generator=g) + 0.5).cuda())
        y = ops.conv_wgrad(routes._dev(o["small"], cs, dt), routes._dev(o["big"], cb, dt), ops.ConvSpec(K, K, s, p), Co, Ci, **kw)
        torch.cuda.synchronize()
        assert y.shape == (Co, Ci, K, K) and y.dtype == torch.float32
        return zlib.crc32(y.contiguous().cpu().numpy().tobytes())
    finally:
        ops.set_fp32_mfma_mode(saved)


@pytest.mark.gpu
@pytest.mark.parametrize("name,mode,scaled", CASES, ids=[case_id(*c) for c in CASES])
def test_wgrad_bits_match_the_recorded_ones(name, mode, scaled):
    with open(GOLDEN) as f:
        golden = json.load(f)
    cid = case_id(name, mode, scaled)
    assert cid in golden, f"{cid}: no recorded CRC (tests/golden/make_wgrad_crc_golden.py)"
    got = wgrad_crc(name, mode, scaled)
    assert got == golden[cid], f"{cid}: CRC {got:#010x}, recorded {golden[cid]:#010x}: the weight gradient's bits changed"


def test_every_case_is_recorded():
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert sorted(golden) == sorted(case_id(*c) for c in CASES)
