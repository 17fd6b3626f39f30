"""TEST INFRASTRUCTURE ONLY — small autograd graphs over gif_amd.functional, each written twice, and the ways a graph may legally be
used (tests/test_graph_wiring_cpu.py on the ATen contracts of tests/cpu_ops.py, tests/test_gpu_graph_wiring.py on the kernels).

Every graph G1..G7 has
  * build(L, o, tap): the graph out of gif_amd.functional calls on the leaves L (a dict of tensors; an absent leaf is None),
  * ref(L, o, tap, rec): the same function in plain, dtype-generic torch (F.conv2d, F.conv_transpose2d, F.leaky_relu, broadcasting,
    the FIR filter as a depthwise F.conv2d), written from the formulas in the docstrings of functional.py and oracle/stylegan2_ref.py:
        conv2d_bias_act      y = gain * lrelu(conv2d(x, w * wscale) + bias)
        modulated_conv2d_act y = gain * lrelu(d[b,co] * conv2d(s[b,ci] * x, w * wscale) + residual + bias)
        modulated_conv2d     y = d * conv2d(s * x, w * wscale), transposed: d * conv_transpose2d(s * x, w * wscale, stride) (d may be None)
        upfirdn2d            y = (zero-pad(x) * flip(k))[::down]    blur_bias_act  y = gain * lrelu(upfirdn2d(x) + residual + bias)
        demodulation         d = rsqrt(scale^2 * s^2 @ (sum_taps w^2)^T + eps)
    It never looks at the Functions' backward code: torch's own autograd differentiates it, in float64 for the reference and in fp32
    for err32, the error the same arithmetic has in the kernels' number format.
`tap(name, y)` is called on every activation a test may want to look at (retain_grad, hooks, autograd.grad w.r.t. it) BEFORE its
consumers are built; `rec(name, z, R, slope, gain)` receives every pre-activation z with R, the same operation on absolute values (as
tests/test_gpu_conv_routes.py defines R).  A draw is ADMISSIBLE when every element of every real activation has |z| >= 4 * TOL * R: no
kernel within TOL of the reference can then put an element on the other side of the leaky ReLU, and no comparison needs an allowance
for sign flips.  CASES carries, per graph, the first admissible seed from its base (find_seed; TOL = 2e-6, the fp32 conv tolerance
of test_gpu_conv_routes.py); the tests assert admissibility and search nothing."""
import functools
from types import MappingProxyType
from typing import NamedTuple

import torch
import torch.nn.functional as F

TOL32 = 2e-6  # test_gpu_conv_routes.TOL of the fp32 contraction modes
TOL16 = 7e-4  # ... and of f16 activations
SQ2 = 2 ** 0.5
_K1 = torch.tensor([1.0, 3.0, 3.0, 1.0])
FIR = (_K1[None, :] * _K1[:, None]) / 64.0  # layers.make_kernel([1, 3, 3, 1])


# ---------------------------------------------------------------------------------------------------------------------------------
# plain-torch pieces of the restatement
# ---------------------------------------------------------------------------------------------------------------------------------
def _bc(v):
    return v[None, :, None, None] if v.dim() == 1 else v[:, :, None, None]


def _fir(x, k, down=1, pad=(0, 0)):
    C = x.shape[1]
    z = F.pad(x, (pad[0], pad[1], pad[0], pad[1]))
    kf = torch.flip(k.to(x.dtype), [0, 1])[None, None].expand(C, 1, -1, -1)
    return F.conv2d(z, kf, groups=C)[:, :, ::down, ::down]


class _Round(torch.autograd.Function):
    """Where an f16 kernel stores a tensor: the value (fwd) and / or the gradient that comes back through this point (bwd) is rounded to
    half; identity otherwise.  (First order only.)"""

    @staticmethod
    def forward(ctx, x, fwd, bwd):
        ctx.bwd = bwd
        return x.half().to(x.dtype) if fwd else x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return (g.half().to(g.dtype) if ctx.bwd else g), None, None


def _act(rec, name, z, R, slope, gain, h=False):
    """h (f16 activations): the masked gradient the consumer's data-gradient kernel stores, and the activation this layer stores, are halfs."""
    rec(name, z.detach(), R, slope, gain)
    if not h:
        return gain * F.leaky_relu(z, slope)
    return _Round.apply(gain * F.leaky_relu(_Round.apply(z, False, True), slope), True, False)


def _conv(x, w, ws, stride, pad, transposed=False, h=False):
    w = _Round.apply(w * ws, True, False) if h else w * ws  # (h: the f16 kernels contract with the scaled weight packed as halfs)
    return F.conv_transpose2d(x, w, stride=stride, padding=pad) if transposed else F.conv2d(x, w, stride=stride, padding=pad)


def _cba(rec, name, x, w, b, stride, pad, ws, slope=0.2, gain=SQ2):
    z = _conv(x, w, ws, stride, pad)
    with torch.no_grad():
        R = _conv(x.abs(), w.abs(), ws, stride, pad)
        if b is not None:
            R = R + _bc(b).abs()
    if b is not None:
        z = z + _bc(b)
    return _act(rec, name, z, R, slope, gain)


class _OutScale16(torch.autograd.Function):
    """y = z * d in the fp32 epilogue of an f16 kernel; its adjoint enters the data- and weight-gradient kernels as the input scale: d as a
    half, times the half gradient, as a half."""

    @staticmethod
    def forward(ctx, z, d):
        ctx.save_for_backward(z, d)
        return z * _bc(d)

    @staticmethod
    def backward(ctx, g):
        z, d = ctx.saved_tensors
        gz = (g.half().to(g.dtype) * _bc(d.half().to(d.dtype))).half().to(g.dtype)
        return gz, (g * z).sum(dim=(2, 3))


def _modconv(x, w, s, d, ws, stride, pad, transposed=False, h=False):
    if not h:
        z = _conv(x * _bc(s), w, ws, stride, pad, transposed)
        return z if d is None else z * _bc(d)
    # f16 kernels (conv_igemm.hip): the modulation is cast to half and multiplied into the half operand fragments, as halfs
    z = _conv(_Round.apply(x * _bc(_Round.apply(s, True, False)), True, False), w, ws, stride, pad, transposed, True)
    return z if d is None else _OutScale16.apply(z, d)


def _mca(rec, name, x, w, s, d, r, b, pad, ws, slope=0.2, gain=SQ2, h=False):
    z = _modconv(x, w, s, d, ws, 1, pad, h=h)
    with torch.no_grad():
        R = _modconv(x.abs(), w.abs(), s.abs(), d.abs(), ws, 1, pad)
    for t in (r, None if b is None else _bc(b)):
        if t is not None:
            z = z + t
            R = R + t.detach().abs()
    return _act(rec, name, z, R, slope, gain, h)


def _demod(s, w, ws, eps=1e-8):
    return torch.rsqrt(ws ** 2 * (s.pow(2) @ w.pow(2).sum(dim=(2, 3)).t()) + eps)


def _ws(w):
    return 1.0 / (w.shape[1] * w.shape[2] * w.shape[3]) ** 0.5


# ---------------------------------------------------------------------------------------------------------------------------------
# the graphs: build = gif_amd.functional, ref = plain torch
# ---------------------------------------------------------------------------------------------------------------------------------
def g1_build(L, o, tap):
    from gif_amd import functional as GF
    y1 = tap("y1", GF.conv2d_bias_act(L["x"], L["w1"], L["b1"], 1, 1, _ws(L["w1"]), o.get("slope1", 0.2), o.get("gain1", SQ2)))
    return [GF.conv2d_bias_act(y1, L["w2"], L["b2"], 1, 1, _ws(L["w2"]))]


def g1_ref(L, o, tap, rec):
    y1 = tap("y1", _cba(rec, "y1", L["x"], L["w1"], L["b1"], 1, 1, _ws(L["w1"]), o.get("slope1", 0.2), o.get("gain1", SQ2)))
    return [_cba(rec, "y2", y1, L["w2"], L["b2"], 1, 1, _ws(L["w2"]))]


def g2_build(L, o, tap):
    from gif_amd import functional as GF
    y = tap("y1", GF.conv2d_bias_act(L["x"], L["w1"], L["b1"], 1, 1, _ws(L["w1"])))
    return [GF.conv2d_bias_act(y, L["w2"], L["b2"], 1, 1, _ws(L["w2"])), GF.conv2d_bias_act(y, L["w3"], L["b3"], 1, 1, _ws(L["w3"])), y.sin()]


def g2_ref(L, o, tap, rec):
    y = tap("y1", _cba(rec, "y1", L["x"], L["w1"], L["b1"], 1, 1, _ws(L["w1"])))
    return [_cba(rec, "ya", y, L["w2"], L["b2"], 1, 1, _ws(L["w2"])), _cba(rec, "yb", y, L["w3"], L["b3"], 1, 1, _ws(L["w3"])), y.sin()]


def g3_build(L, o, tap):
    """A from-RGB ConvLayer, then discriminator.ResBlock as layers.py wires it: conv1 with passthrough, Blur(pad 2, 2) -> stride-2 conv2 with
    1/sqrt(2) in its gain, the skip = FIR with down 2 (pad 1, 1) -> 1x1 conv with 1/sqrt(2) in its weight scale and conv2's output as residual."""
    from gif_amd import functional as GF
    k, r = FIR.to(L["x"].device), 1 / SQ2
    y0 = tap("y0", GF.conv2d_bias_act(L["x"], L["w0"], L["b0"], 1, 1, _ws(L["w0"])))
    out, alias = GF.conv2d_bias_act(y0, L["w1"], L["b1"], 1, 1, _ws(L["w1"]), passthrough=True)
    out = tap("y1", out)
    out = GF.conv2d_bias_act(GF.upfirdn2d(out, k, pad=(2, 2)), L["w2"], L["b2"], 2, 0, _ws(L["w2"]), 0.2, SQ2 * r)
    return [GF.conv2d(GF.upfirdn2d(alias, k, up=1, down=2, pad=(1, 1)), L["w3"], 1, 0, wscale=_ws(L["w3"]) * r, residual=out)]


def g3_ref(L, o, tap, rec):
    k, r = FIR, 1 / SQ2
    y0 = tap("y0", _cba(rec, "y0", L["x"], L["w0"], L["b0"], 1, 1, _ws(L["w0"])))
    out = tap("y1", _cba(rec, "y1", y0, L["w1"], L["b1"], 1, 1, _ws(L["w1"])))
    out = _cba(rec, "y2", _fir(out, k, 1, (2, 2)), L["w2"], L["b2"], 2, 0, _ws(L["w2"]), 0.2, SQ2 * r)
    return [_conv(_fir(y0, k, 2, (1, 1)), L["w3"], _ws(L["w3"]) * r, 1, 0) + out]


def _scales_build(L, o, i):
    from gif_amd import functional as GF
    w = L[f"w{i}"]
    if o.get("demod"):
        return L[f"s{i}"], GF.demodulation(L[f"s{i}"], w, _ws(w), 1e-8, w.shape[0])
    return L[f"s{i}"], L[f"d{i}"]


def _scales_ref(L, o, i):
    w = L[f"w{i}"]
    return L[f"s{i}"], (_demod(L[f"s{i}"], w, _ws(w)) if o.get("demod") else L[f"d{i}"])


def g4_build(L, o, tap):
    """The last condition-noise conv (conv + bias, identity activation) as `residual` of a StyledConv, a second StyledConv on top."""
    from gif_amd import functional as GF
    r = tap("r", GF.conv2d_bias_act(L["c"], L["wr"], L["br"], 1, 1, _ws(L["wr"]), 1.0, 1.0))
    (s1, d1), (s2, d2) = _scales_build(L, o, 1), _scales_build(L, o, 2)
    y1 = tap("y1", GF.modulated_conv2d_act(L["x"], L["w1"], s1, d1, r, L["b1"], 1, _ws(L["w1"])))
    return [GF.modulated_conv2d_act(y1, L["w2"], s2, d2, None, L["b2"], 1, _ws(L["w2"]))]


def g4_ref(L, o, tap, rec):
    r = tap("r", _cba(rec, "r", L["c"], L["wr"], L["br"], 1, 1, _ws(L["wr"]), 1.0, 1.0))
    (s1, d1), (s2, d2) = _scales_ref(L, o, 1), _scales_ref(L, o, 2)
    y1 = tap("y1", _mca(rec, "y1", L["x"], L["w1"], s1, d1, r, L["b1"], 1, _ws(L["w1"])))
    return [_mca(rec, "y2", y1, L["w2"], s2, d2, None, L["b2"], 1, _ws(L["w2"]))]


def g5_build(L, o, tap):
    """layers.ModulatedConv2d.forward_fused_act, up-sampling branch: conv_transpose2d (stride 2, canonical forward weight = the transposed
    view) to 2H + 1, then Blur(pad 1, 1; kernel * 4) with the condition-noise residual, the bias and the leaky ReLU in the FIR epilogue.
    There is deliberately no stand-alone upfirdn2d between the two: layers.py fuses the blur into blur_bias_act, and that wiring is what is
    copied.  (Upfirdn2dFn's port route runs in the ResBlock graph.)"""
    from gif_amd import functional as GF
    H, W = L["x"].shape[2:]
    y1 = tap("y1", GF.modulated_conv2d_act(L["x"], L["w1"], L["s1"], L["d1"], None, L["b1"], 1, _ws(L["w1"])))
    r = tap("r", GF.conv2d_bias_act(L["c"], L["wr"], L["br"], 1, 1, _ws(L["wr"]), 1.0, 1.0))
    wt = L["w2"].transpose(0, 1)  # the layer's weight is [Cout, Cin, k, k]
    up = GF.modulated_conv2d(y1, wt, L["s2"], L["d2"], stride=2, pad=0, transposed=True, out_hw=(2 * H + 1, 2 * W + 1), wscale=_ws(L["w2"]))
    return [GF.blur_bias_act(up, (FIR * 4).to(up.device), (1, 1), r, L["b2"])]


def g5_ref(L, o, tap, rec):
    y1 = tap("y1", _mca(rec, "y1", L["x"], L["w1"], L["s1"], L["d1"], None, L["b1"], 1, _ws(L["w1"])))
    r = tap("r", _cba(rec, "r", L["c"], L["wr"], L["br"], 1, 1, _ws(L["wr"]), 1.0, 1.0))
    wt, ws = L["w2"].transpose(0, 1), _ws(L["w2"])
    up = _modconv(y1, wt, L["s2"], L["d2"], ws, 2, 0, True)
    z = _fir(up, FIR * 4, 1, (1, 1)) + r + _bc(L["b2"])
    with torch.no_grad():
        R = _fir(_modconv(y1.abs(), wt.abs(), L["s2"].abs(), L["d2"].abs(), ws, 2, 0, True), FIR * 4, 1, (1, 1)) + r.abs() + _bc(L["b2"]).abs()
    return [_act(rec, "y2", z, R, 0.2, SQ2)]


def g6_build(L, o, tap):
    from gif_amd import functional as GF
    y1 = tap("y1", GF.modulated_conv2d_act(L["x"], L["w1"], L["s1"], L["d1"], None, L["b1"], 1, _ws(L["w1"])))
    return [GF.modulated_conv2d(y1, L["w2"], L["s2"], None, stride=1, pad=0, wscale=_ws(L["w2"]), out_f32=bool(o.get("f16")))]


def g6_ref(L, o, tap, rec):
    """f16: x, y1 and the gradients stored on them are halfs, the scaled weights are packed as halfs, the RGB output is fp32 (out_f32) and
    its fp32 gradient re-enters the f16 kernels rounded to half.  All sums are fp32 in the kernels: nothing else rounds."""
    h = bool(o.get("f16"))
    x = _Round.apply(L["x"], False, True) if h else L["x"]
    y1 = tap("y1", _mca(rec, "y1", x, L["w1"], L["s1"], L["d1"], None, L["b1"], 1, _ws(L["w1"]), h=h))
    rgb = _modconv(y1, L["w2"], L["s2"], None, _ws(L["w2"]), 1, 0, h=h)
    return [_Round.apply(rgb, False, True) if h else rgb]


# ---------------------------------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------------------------------
class Case(NamedTuple):
    name: str
    build: object
    ref: object
    leaves: tuple        # (name, kind, shape): kind x (activation input) | w | b | s | d
    seed: int            # first admissible seed from the base (find_seed), asserted by the tests
    opts: object = MappingProxyType({})
    absent: tuple = ()   # leaves passed as None
    frozen: tuple = ()   # leaves with requires_grad off in every use
    masks: int = 0       # GradFuse(mask_src=...) launches one full first-order backward must build, ports on (port-carrying edges)
    route: str = ""      # "dot": the modulation gradient rides in the data-gradient epilogue, "mul_reduce": the stand-alone pass
    down: str = "w2"     # U3: a downstream leaf (its layer's data gradient still runs, the layers below are pruned) and an upstream one
    up: str = "b1"
    second: tuple = ("x",)  # U5: leaves the inner gradient is taken of
    tol: float = TOL32   # the conv tolerance admissibility is stated with
    grad_inputs: object = MappingProxyType({})  # U4, ports on: what autograd.grad(inputs=[tap]) sees: none | full | partial (see functional.ActPort)


def _conv_leaves(B, C, H, W, n):
    out = [("x", "x", (B, C, H, W))]
    for i in range(1, n + 1):
        out += [(f"w{i}", "w", (C, C, 3, 3)), (f"b{i}", "b", (C,))]
    return tuple(out)


def _styled_leaves(B, Cin, C, H, W, demod=False, cond_hw=None, w2=(3, 3), c2=None):
    c2 = C if c2 is None else c2
    out = [("x", "x", (B, Cin, H, W)), ("c", "x", (B, 4) + (cond_hw or (H, W))), ("wr", "w", (C, 4, 3, 3)), ("br", "b", (C,)),
           ("w1", "w", (C, Cin, 3, 3)), ("b1", "b", (C,)), ("s1", "s", (B, Cin)), ("w2", "w", (c2, C) + w2), ("b2", "b", (c2,)), ("s2", "s", (B, C))]
    if not demod:
        out += [("d1", "d", (B, C)), ("d2", "d", (B, c2))]
    return tuple(out)


_G3 = (("x", "x", (2, 8, 32, 32)), ("w0", "w", (8, 8, 3, 3)), ("b0", "b", (8,)), ("w1", "w", (8, 8, 3, 3)), ("b1", "b", (8,)),
       ("w2", "w", (12, 8, 3, 3)), ("b2", "b", (12,)), ("w3", "w", (12, 8, 1, 1)))
_G6 = tuple(l for l in _styled_leaves(2, 8, 8, 32, 32, w2=(1, 1), c2=4) if l[0] not in ("c", "wr", "br", "d2", "b2"))
_NONE = {"y1": "none"}
_SX = ("x", "s1")

CASES = [
    Case("cba_chain", g1_build, g1_ref, _conv_leaves(2, 8, 32, 32, 2), 1003, masks=1, grad_inputs=_NONE),
    Case("cba_chain_b1_none", g1_build, g1_ref, _conv_leaves(2, 8, 32, 32, 2), 1000, absent=("b1",), masks=1, up="w1", grad_inputs=_NONE),
    Case("cba_chain_b1_frozen", g1_build, g1_ref, _conv_leaves(2, 8, 32, 32, 2), 1003, frozen=("b1",), masks=1, up="w1", grad_inputs=_NONE),
    Case("cba_chain_ident", g1_build, g1_ref, _conv_leaves(2, 8, 32, 32, 2), 1000, opts={"slope1": 1.0, "gain1": 1.0}, grad_inputs={"y1": "full"}),
    Case("cba_fan_out", g2_build, g2_ref, _conv_leaves(2, 8, 32, 32, 3), 2003, masks=2, grad_inputs={"y1": "partial"}),
    Case("resblock", g3_build, g3_ref, _G3, 3000, masks=2, down="w1", up="b0", grad_inputs={"y0": "none", "y1": "none"}),
    Case("styled_pair_32", g4_build, g4_ref, _styled_leaves(2, 8, 8, 32, 32), 4006, masks=1, route="dot", second=_SX, up="br",
         grad_inputs={"y1": "none", "r": "none"}),
    Case("styled_pair_16", g4_build, g4_ref, _styled_leaves(2, 8, 8, 16, 16), 4100, route="mul_reduce", second=_SX, up="br",
         grad_inputs={"y1": "none", "r": "none"}),
    Case("styled_pair_c36", g4_build, g4_ref, _styled_leaves(2, 36, 8, 32, 32), 4206, masks=1, route="dot", second=_SX, up="br",
         grad_inputs={"y1": "none", "r": "none"}),
    Case("styled_up", g5_build, g5_ref, _styled_leaves(2, 8, 8, 32, 32, cond_hw=(64, 64)), 5040, masks=1, route="dot", second=_SX, up="br",
         grad_inputs={"y1": "none", "r": "none"}),
    Case("to_rgb", g6_build, g6_ref, _G6, 6001, masks=1, route="dot", second=_SX, grad_inputs=_NONE),
    # f16 activations, fp32 RGB output (out_f32): the fp32 gradient re-enters the f16 kernels as f16.  Admissibility at TOL 7e-4 asks |z| >=
    # 2.8e-3 * R of every element: with biases of +-0.5 no draw of 16k elements has it (about 1 % of the elements fail), and at the 100-odd
    # elements where one would, the fused dot (1024 | H * W) is out of reach.  So b1 = +-5 + 0.5 * randn instead: the pre-activations sit
    # around +-5 (std 3.8; both slopes: the sign is mostly per channel, some tens of elements cross), the factor 4 and 32x32 stay.
    # First order only: the recorded backward of an out_f32 layer is not part of what this variant is about.  Device tier only.
    Case("to_rgb_f16", g6_build, g6_ref, _G6, 6106, opts=MappingProxyType({"f16": True, "bias": 5.0}), masks=1, route="dot", second=(),
         grad_inputs=_NONE, tol=TOL16),
    Case("demod_closed", g4_build, g4_ref, _styled_leaves(2, 8, 8, 32, 32, demod=True), 7000, opts={"demod": True}, masks=1, route="dot",
         second=_SX, up="br", grad_inputs={"y1": "none", "r": "none"}),
]
BY_NAME = {c.name: c for c in CASES}
CPU_CASES = [c for c in CASES if not c.opts.get("f16")]  # (the ATen contracts of the CPU tier are fp32)
GROUPS = {"wb": ("w", "b"), "x": ("x",), "sd": ("s", "d")}  # U2: kinds frozen together


def frozen_by_group(case, group):
    return tuple(n for n, k, _ in case.leaves if k in GROUPS[group])


def u2_pairs(cases=None):
    """(case name, group) for every group the case has a leaf of."""
    return [(c.name, g) for c in (CASES if cases is None else cases) for g in GROUPS if frozen_by_group(c, g)]


def make_leaves(case, conv=None, frozen=(), seed=None, ref=False):
    """fp32 CPU draws of the case's seed, passed through conv(kind, tensor) (dtype / device), then made leaves: weights and biases are
    nn.Parameters (functional.inputs_only_backward skips exactly those)."""
    g = torch.Generator().manual_seed(case.seed if seed is None else seed)
    L = {}
    for name, kind, shape in case.leaves:
        t = torch.randn(*shape, generator=g)
        if kind == "b":
            t = 0.5 * t + (case.opts.get("bias", 0.0) * torch.sign(t) if name == "b1" else 0.0)
        elif kind == "s":
            t = 1.0 + 0.3 * t
        elif kind == "d":
            t = 0.5 + t.abs()
        if name in case.absent:
            L[name] = None
            continue
        t = t if conv is None else conv(kind, t)
        if case.opts.get("f16") and kind == "x":  # f16 activations; the restatement starts from the same, rounded, values
            t = t.half().to(t.dtype) if ref else t.half()
        need = name not in case.frozen and name not in frozen
        L[name] = torch.nn.Parameter(t, requires_grad=need) if kind in "wb" else t.requires_grad_(need)
    return L


class Graph:
    """One forward of a case: .L leaves, .names (leaves that require a gradient), .outs, .loss = sum of squares of the outputs, .taps."""

    def __init__(self, case, conv=None, frozen=(), tap=None, ref=False, seed=None):
        self.case, self.taps, self.acts = case, {}, []
        self.L = make_leaves(case, conv, frozen, seed, ref)
        self.names = [n for n, t in self.L.items() if t is not None and t.requires_grad]

        def _tap(name, y):
            self.taps[name] = y
            if tap is not None:
                tap(name, y)
            return y

        if ref:
            self.outs = case.ref(self.L, case.opts, _tap, lambda *a: self.acts.append(a))
        else:
            self.outs = case.build(self.L, case.opts, _tap)
        self.loss = sum((o.float() if o.dtype == torch.float16 else o).pow(2).sum() for o in self.outs)

    def grads(self, names=None, of=None, **kw):
        """{leaf name: gradient} of .loss (or of `of`) w.r.t. the named leaves (default: all that require one)."""
        names = self.names if names is None else names
        out = torch.autograd.grad(self.loss if of is None else of, [self.L[n] for n in names], **kw)
        return dict(zip(names, out))


def cpu(g):
    return {k: (None if v is None else v.detach().cpu()) for k, v in g.items()}


def admissible(acts, tol):
    """Every element of every real activation is at least 4 * tol * R away from the kink."""
    return all(bool((z.abs() >= 4 * tol * R).all()) for _, z, R, slope, gain in acts if not (slope == 1.0 and gain == 1.0))


def find_seed(case, base, tries=200):
    """First seed in base, base + 1, ... whose float64 forward is admissible (how the seeds of CASES were chosen)."""
    for seed in range(base, base + tries):
        with torch.no_grad():
            if admissible(Graph(case, lambda k, t: t.double(), ref=True, seed=seed).acts, case.tol):
                return seed
    raise AssertionError(f"{case.name}: no admissible seed in {tries} tries from {base}")


@functools.lru_cache(maxsize=None)
def reference(name, dtype=torch.float64):
    """Gradients of the plain-torch restatement in `dtype` on the CPU: u1 {leaf: grad}; taps {tap: d loss / d tap}; partial {tap: the part
    of it that reaches the tap from consumers outside the port protocol}; per U5 target t: g[t] the inner gradient, u5[t] {leaf: grad of
    (g ** 2).sum()}; acts for admissible().  Computed once per case and dtype, never modified."""
    case = BY_NAME[name]
    G = Graph(case, lambda k, t: t.to(dtype), ref=True)
    out = {"acts": G.acts, "names": G.names, "u1": cpu(G.grads(retain_graph=True))}
    taps = list(G.taps)
    out["taps"] = dict(zip(taps, [t.detach() for t in torch.autograd.grad(G.loss, [G.taps[t] for t in taps], retain_graph=True)]))
    out["partial"] = {}
    if case.name == "cba_fan_out":
        (out["partial"]["y1"],) = torch.autograd.grad(G.outs[2].pow(2).sum(), [G.taps["y1"]], retain_graph=True)
    out["g"], out["u5"] = {}, {}
    for t in case.second:
        (g,) = torch.autograd.grad(G.loss, [G.L[t]], create_graph=True)
        out["g"][t] = g.detach()
        out["u5"][t] = cpu(G.grads(of=g.pow(2).sum(), retain_graph=True, allow_unused=True))
    return out


def rel_err(got, ref):
    """max |got - ref| / max |ref| over one tensor, in float64."""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float((got - ref).abs().max() / ref.abs().max())


# ---------------------------------------------------------------------------------------------------------------------------------
# the uses.  conv(kind, tensor) places a leaf (dtype / device); every result comes back as CPU tensors.
# ---------------------------------------------------------------------------------------------------------------------------------
def u1(case, conv=None, frozen=()):
    """U1 / U2: one full first-order pass on a fresh graph (frozen: leaves with requires_grad off before the forward)."""
    return cpu(Graph(case, conv, frozen).grads())


def u3(case, conv, how):
    """U3: a legal other use of the graph first, then the full pass on the SAME graph.  how: down | up (a partial pass aimed at one
    leaf) | twice (the full pass) | backward2 (loss.backward twice: returns .grad / 2, exact in binary floating point)."""
    G = Graph(case, conv)
    if how == "backward2":
        G.loss.backward(retain_graph=True)
        G.loss.backward(retain_graph=True)
        return cpu({n: G.L[n].grad / 2 for n in G.names})
    G.grads(G.names if how == "twice" else [case.down if how == "down" else case.up], retain_graph=True)
    return cpu(G.grads())


def u4(case, conv, how):
    """U4: look at the gradient of every tapped activation.  how: retain_before | hook_before (set when the tap is produced, before its
    consumers are built) | retain_after | hook_after (set after the forward) | grad_inputs (autograd.grad w.r.t. the taps).
    Returns ({tap: gradient seen, None if none was}, {leaf: gradient} of the same pass)."""
    seen = {}

    def watch(name, y):
        if how.startswith("retain"):
            y.retain_grad()
        else:
            def hook(g, name=name):
                assert name not in seen, f"{name}: hook called twice"
                seen[name] = g
            y.register_hook(hook)

    G = Graph(case, conv, tap=watch if how.endswith("before") else None)
    if how == "grad_inputs":
        taps = list(G.taps)
        out = torch.autograd.grad(G.loss, [G.taps[t] for t in taps] + [G.L[n] for n in G.names], allow_unused=True)
        return cpu(dict(zip(taps, out))), cpu(dict(zip(G.names, out[len(taps):])))
    if how.endswith("after"):
        for name, y in G.taps.items():
            watch(name, y)
    G.loss.backward()
    if how.startswith("retain"):
        seen = {name: y.grad for name, y in G.taps.items()}
    return cpu({t: seen.get(t) for t in G.taps}), cpu({n: G.L[n].grad for n in G.names})


def u5(case, conv, target, inputs_only=False, then_full=False):
    """U5: g = d loss / d target with create_graph, then the gradients of (g ** 2).sum() w.r.t. all leaves (the R1 / path-length shape).
    inputs_only: the inner call runs inside functional.inputs_only_backward().  then_full (U6): return the plain full pass on the same
    graph instead of the second-order gradients.  Returns (g, {leaf: gradient}, conv_wgrad calls of the inner pass)."""
    import contextlib
    from gif_amd import functional as GF, ops
    G = Graph(case, conv)
    calls, real = [0], ops.conv_wgrad

    def counted(*a, **k):
        calls[0] += 1
        return real(*a, **k)

    ops.conv_wgrad = counted
    try:
        with GF.inputs_only_backward() if inputs_only else contextlib.nullcontext():
            (g,) = torch.autograd.grad(G.loss, [G.L[target]], create_graph=True)
    finally:
        ops.conv_wgrad = real
    if then_full:
        return g.detach().cpu(), cpu(G.grads()), calls[0]
    return g.detach().cpu(), cpu(G.grads(of=g.pow(2).sum(), allow_unused=True)), calls[0]
