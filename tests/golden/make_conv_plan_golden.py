"""Generates tests/golden/conv_plan_table.txt: what gif_amd/ops.py decides before it calls the library, one line per case:
    <knobs>  fwd|dgrad|wgrad  f32|f16  <fp32 MFMA mode>  B Cin Cout K stride pad Hb Wb Hs Ws  scaled in_bytes -> route mode dense
(Cin / Cout: the op's contraction / output channel counts as the activations carry them, for wgrad Cb / Cs; Hb Wb / Hs Ws: the big and the
small side of the forward convolution; scaled: per-sample input scales; <knobs>: "default" or the one knob set differently), then
    <knobs>  wino  fwd|wgrad  <fp32 MFMA mode>  Cout -> mode
for the Winograd functions called on their own.  First the default knobs; then each of eight knobs flipped and the two channel thresholds at
0 and 256, one at a time over a thinned grid, of which only the cases are listed whose line differs from the default one (and how many did).  The lines come from ops.conv_plan and ops.winograd_mode alone, which are pure Python: no GPU
and no library is needed.  The first version of the file was recorded at the commit before conv_plan existed, from the predicates composed as
conv_fwd, conv_bwd_data, conv_wgrad, conv3x3_winograd and conv3x3_winograd_wgrad composed them then; tests/test_conv_route.py checks that
conv_plan still gives every line.
Run: python tests/golden/make_conv_plan_golden.py"""
import os
import sys
from typing import NamedTuple

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

CHANNELS = (4, 8, 12, 24, 28, 32, 48, 64, 128, 252, 256)
SPECS = ((3, 3, 1, 1), (3, 3, 2, 0), (1, 1, 1, 0), (3, 3, 1, 0))
# every count as contraction side against an output side below / above the Winograd and tap-dense output rules, and every count as output
# side against a contraction side below / above the bf16x3 and Winograd input rules
PAIRS = sorted({(ci, co) for ci in CHANNELS for co in (48, 256)} | {(ci, co) for ci in (24, 128) for co in CHANNELS})
THIN = ((12, 24), (24, 128), (32, 48), (128, 128), (256, 256))
BASE = (8, 64, 64)  # 8192 2x2 tiles: exactly WINOGRAD_MIN_TILES
# (B, Hb, Wb): 7936 tiles (below WINOGRAD_MIN_TILES, above WINOGRAD_WGRAD_MIN_TILES), odd H, odd W, 2048 tiles (exactly the weight
# gradient's threshold) and 1984
SHAPES = ((8, 64, 62), (8, 63, 64), (8, 64, 63), (2, 64, 64), (2, 64, 62))
F32 = (("f32", "native"), ("f32", "bf16x3"), ("f32", "f16x2"))
F16 = (("f16", "native"), ("f16", "f16x2"))  # (f16 activations keep their kernels whatever the process-wide fp32 mode is)
OPS = ("fwd", "dgrad", "wgrad")
FLIPS = ("WINOGRAD", "WINOGRAD_WGRAD", "WINOGRAD_X3", "X3_TAPDENSE", "H2_CONV", "H2_WGRAD", "H2_WINO", "H2_DENSE")
WINO_COUTS = (48, 128, 252, 256)  # the Winograd GEMM's bf16x3 / f16x2 forms want full 128-wide N tiles
MIN_C = tuple((k, v) for k in ("WINOGRAD_MIN_C", "WINOGRAD_WGRAD_MIN_C") for v in (0, 256))


class Case(NamedTuple):
    op: str
    dtype: str
    mfma: str
    B: int
    cin: int
    cout: int
    spec: tuple
    big_hw: tuple
    small_hw: tuple
    scaled: bool = False
    in_bytes: int = 0


def _case(op, mode, pair, spec, shape=BASE, small_hw=None, **kw):
    K, _, s, p = spec
    B, H, W = shape
    return Case(op, mode[0], mode[1], B, pair[0], pair[1], spec, (H, W), small_hw or ((H + 2 * p - K) // s + 1, (W + 2 * p - K) // s + 1), **kw)


def _modes(pair, f16=F16):
    return F32 + (() if pair[0] % 8 or pair[1] % 8 else f16)


def default_cases(max_bytes):
    for pair in PAIRS:  # the channel rules, at the Winograd spec and size
        for mode in _modes(pair, F16[:1]):
            for op in OPS:
                yield _case(op, mode, pair, SPECS[0])
    for pair in THIN:
        for mode in _modes(pair):
            for op in OPS:
                for spec in SPECS[1:]:
                    yield _case(op, mode, pair, spec)
                if pair[0] >= 32 and mode[0] == "f32":  # the size rules of the Winograd route
                    for shape in SHAPES:
                        yield _case(op, mode, pair, SPECS[0], shape)
                    if op != "fwd":  # a data / weight gradient whose two sides differ in size (enough tiles, even sizes, the Winograd spec)
                        yield _case(op, mode, pair, SPECS[0], (8, 66, 66), small_hw=(64, 64))
                # per-sample scales and the 4 GiB rule: they touch fwd / dgrad of fp32 activations; one pair shows that they touch nothing else
                if pair[1] != 256 and (pair == (24, 128) or (op != "wgrad" and mode[0] == "f32")) and mode != F16[0]:
                    for spec in SPECS[:3]:
                        yield _case(op, mode, pair, spec, scaled=True)
                        yield _case(op, mode, pair, spec, in_bytes=max_bytes)
                        yield _case(op, mode, pair, spec, in_bytes=max_bytes + 4)


def knob_cases():
    for pair in THIN:
        for mode in _modes(pair, F16[1:]):
            for spec in (SPECS[0], SPECS[3]):
                for op in OPS:
                    yield _case(op, mode, pair, spec)


def table_lines():
    import torch
    from gif_amd import ops
    real_mode = ops.get_fp32_mfma_mode

    def run(cases):
        out = []
        for c in cases:
            ops.get_fp32_mfma_mode = (lambda m: lambda: m)(c.mfma)
            plan = ops.conv_plan(c.op, torch.float16 if c.dtype == "f16" else torch.float32, c.B, ops.ConvSpec(*c.spec), c.big_hw, c.small_hw,
                                 c.cin, c.cout, {"in_scale": True} if c.scaled else {}, c.in_bytes)
            K, _, s, p = c.spec
            out.append(f"{c.op} {c.dtype} {c.mfma} {c.B} {c.cin} {c.cout} {K} {s} {p} {c.big_hw[0]} {c.big_hw[1]} {c.small_hw[0]} "
                       f"{c.small_hw[1]} {int(c.scaled)} {c.in_bytes} -> {plan.route} {plan.mode} {int(plan.dense)}")
        for mfma in ("native", "bf16x3", "f16x2"):
            ops.get_fp32_mfma_mode = (lambda m: lambda: m)(mfma)
            for op in ("fwd", "wgrad"):
                for cout in WINO_COUTS:
                    out.append(f"wino {op} {mfma} {cout} -> {ops.winograd_mode(op, cout)}")
        return out

    try:
        lines = ["default " + l for l in run(default_cases(ops.X3_MAX_INPUT_BYTES))]
        base = run(knob_cases())
        for knob, value in [(k, not getattr(ops, k)) for k in FLIPS] + list(MIN_C):
            saved = getattr(ops, knob)
            setattr(ops, knob, value)
            try:
                differ = [l for l, b in zip(run(knob_cases()), base) if l != b]
            finally:
                setattr(ops, knob, saved)
            lines.append(f"{knob}={int(value)}: {len(differ)} of {len(base)} cases differ from the default")
            lines += [f"{knob}={int(value)} {l}" for l in differ]
    finally:
        ops.get_fp32_mfma_mode = real_mode
    return lines


if __name__ == "__main__":
    out = table_lines()
    with open(os.path.join(HERE, "conv_plan_table.txt"), "w") as f:
        f.write("\n".join(out) + "\n")
    print(f"{len(out)} lines written")
