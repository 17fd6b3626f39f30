"""-m gpu: the Winograd forward convolutions and data gradients of tests/test_gpu_winograd_edges.py are bit-identical to the recorded ones.

These ops have no split-K and reduce their per-tile partial sums in a fixed order, so a change of the host-side dispatch (csrc/wino_route.h,
the launch code of csrc/conv_winograd.hip) that keeps every route must keep every bit.  Cases: each row of test_gpu_winograd_edges.FROWS
in each mode it lists, on that module's operands and through its _f_run — which covers wino_gemm_mfma<2> and <4>, wino_gemm_x3<128,128>
and wino_gemm_h2<128,128,3> behind wino_input_transform_rows<8>.  tests/golden/wino_crc_golden.json holds the CRC-32 of each output's
bytes, of the real rows of V where the row checks V, and of the fused column sums / dot products where the row has them, written by
tests/golden/make_wino_crc_golden.py from the commit before the route header (two runs agreed on every case).  A result of more than
2^26 elements would be hashed over its first and last 2^22 elements only (no row is that large: the largest, wide_512, has 2^25)."""
import json
import os
import zlib

import pytest
import torch

import test_gpu_winograd_edges as edges  # (pytest puts this directory on sys.path)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wino_crc_golden.json")
CASES = [(r.name, m) for r in edges.FROWS for m in r.modes]
WHOLE_MAX, ENDS = 2 ** 26, 2 ** 22


def case_id(name, mode):
    return f"{name}-{mode}"


def hashed_in_part(row):
    """the results of `row` that are hashed over their two ends only"""
    B, C, Co, H, W = row.shape
    geo = edges.geometry(*row.shape)
    sizes = {"y": B * Co * H * W, "v": 16 * geo["ntiles"] * geo["CP"] if row.v else 0}
    return [k for k, n in sizes.items() if n > WHOLE_MAX]


def _crc(t):
    flat = t.contiguous().view(-1)
    if flat.numel() > WHOLE_MAX:
        flat = torch.cat([flat[:ENDS], flat[-ENDS:]])
    return zlib.crc32(flat.cpu().numpy().tobytes())


def wino_crcs(name, mode):
    """CRC-32s of one case's results: {"y": ..} plus "v" where the row checks V and "colsum" / "dot" where it fuses them (the mode is
    restored afterwards)."""
    from gif_amd import ops
    row = next(r for r in edges.FROWS if r.name == name)
    geo = edges.geometry(*row.shape, mode)
    saved_mode = ops.get_fp32_mfma_mode()
    try:
        ops.set_fp32_mfma_mode(mode)
        o = edges._f_operands(row)
        o["x_dev"] = edges._cl(o["x"])
        y, V, fuse = edges._f_run(row, o, edges._wview(row, o["w_store"].cuda()), keep_v=row.v)
        torch.cuda.synchronize()
        out = {"y": _crc(y)}
        if row.v:  # (the row padding ntiles..ntiles_pad is never written)
            out["v"] = _crc(V.view(16, geo["ntiles_pad"], geo["CP"])[:, :geo["ntiles"]])
        if fuse is not None:
            out["colsum"] = _crc(fuse.colsum)
            if fuse.dot is not None:
                out["dot"] = _crc(fuse.dot)
        return out
    finally:
        ops.set_fp32_mfma_mode(saved_mode)


@pytest.mark.gpu
@pytest.mark.parametrize("name,mode", CASES, ids=[case_id(*c) for c in CASES])
def test_winograd_bits_match_the_recorded_ones(name, mode):
    with open(GOLDEN) as f:
        golden = json.load(f)
    cid = case_id(name, mode)
    assert cid in golden, f"{cid}: no recorded CRCs (tests/golden/make_wino_crc_golden.py)"
    got = wino_crcs(name, mode)
    assert got == golden[cid], f"{cid}: CRCs {got}, recorded {golden[cid]}: the convolution's bits changed"


def test_every_case_is_recorded():
    with open(GOLDEN) as f:
        golden = json.load(f)
    assert sorted(golden) == sorted(case_id(*c) for c in CASES)
    for row in edges.FROWS:
        want = {"y"} | ({"v"} if row.v else set()) | ({"colsum"} if row.epi in ("fuse", "fusedot") else set()) | ({"dot"} if row.epi == "fusedot" else set())
        assert all(set(golden[case_id(row.name, m)]) == want for m in row.modes), row.name
        assert not hashed_in_part(row), row.name
