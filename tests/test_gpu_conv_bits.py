"""-m gpu: the forward convolutions and data gradients of the route table are bit-identical to the recorded ones.

These ops have no split-K and reduce their per-tile partial sums in a fixed order, so a change of the host-side dispatch (csrc/conv_route.h,
the launch code of csrc/conv_igemm.hip) that keeps every route must keep every bit.  Cases: each `fwd` / `dgrad` row of
test_gpu_conv_routes.ROWS in each mode it lists, on that module's operands and through its _run (the Winograd rows included).
tests/golden/conv_crc_golden.json holds the CRC-32 of each output's bytes and, where the row fuses them, of the column sums and the dot
products, written by tests/golden/make_conv_crc_golden.py from the commit before the route header (two runs agreed on every case)."""
import json
import os
import zlib

import pytest
import torch

import test_gpu_conv_routes as routes  # (pytest puts this directory on sys.path)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_crc_golden.json")
CASES = [(r.name, m) for r in routes.ROWS if r.op in ("fwd", "dgrad") for m in r.fams]


def case_id(name, mode):
    return f"{name}-{mode}"


def _crc(t):
    return zlib.crc32(t.contiguous().cpu().numpy().tobytes())


def conv_crcs(name, mode):
    """CRC-32s of one case's results: {"y": ..} plus "colsum" / "dot" where the row fuses them (mode and patches are restored afterwards)."""
    from gif_amd import ops
    row = next(r for r in routes.ROWS if r.name == name)
    f16 = mode == "f16"
    saved_mode = ops.get_fp32_mfma_mode()
    saved = [(k, getattr(ops, k)) for k, _ in row.patch]
    try:
        for k, v in row.patch:
            setattr(ops, k, v)
        if not f16:
            ops.set_fp32_mfma_mode(mode)
        y, fuse = routes._run(row, mode, routes._operands(row, f16))
        torch.cuda.synchronize()
        out = {"y": _crc(y)}
        if fuse is not None:
            out["colsum"] = _crc(fuse.colsum)
            if fuse.dot is not None:
                out["dot"] = _crc(fuse.dot)
        return out
    finally:
        ops.set_fp32_mfma_mode(saved_mode)
        for k, v in saved:
            setattr(ops, k, v)


@pytest.mark.gpu
@pytest.mark.parametrize("name,mode", CASES, ids=[case_id(*c) for c in CASES])
def test_conv_bits_match_the_recorded_ones(name, mode):
    with open(GOLDEN) as f:
        golden = json.load(f)
    cid = case_id(name, mode)
    assert cid in golden, f"{cid}: no recorded CRCs (tests/golden/make_conv_crc_golden.py)"
    got = conv_crcs(name, mode)
    assert got == golden[cid], f"{cid}: CRCs {got}, recorded {golden[cid]}: the convolution's bits changed"


def test_every_case_is_recorded():
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert sorted(golden) == sorted(case_id(*c) for c in CASES)
