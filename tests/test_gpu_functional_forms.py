"""-m gpu: the conv-side bindings (gif_amd/functional.py over gif_amd/ops.py: conv, FIR, bias / activation, reductions, minibatch stddev, the style
path) fed their operands in other FORMS than dense, 16-byte-aligned tensors at storage offset 0 on the current stream.  tests/ops_forms.py has the
forms (nchw, wide, permuted, expanded, batch_offset, offset4, side_stream) and the two hooks; every run in this module happens under
recorded_launches(before=checked(stream)) or (before=forbidden()): a pointer that is not 16-byte aligned, a launch on another stream than the
current one, or any launch where the binding had to refuse stops as an AssertionError BEFORE the call reaches the library.

  1. every graph of graph_cases.CASES in every form: outputs, every tapped activation and every leaf gradient bit-equal (same shape, same dtype) to
     the plain run of the same case — the kernels sum in a fixed order (tests/test_gpu_graph_wiring.py relies on it), so no tolerance and no element
     left out.  `expanded` compares with its materialised batch.  The plain run is checked too, and its first forward convolution is handed the
     leaf's own address: a dense aligned input costs no copy.
  2. the recorded backward (graph_cases.u5: R1 and the path-length regulariser) of every case's `second` targets in nchw, wide and side_stream.
  3. the ops whose interesting operand is never a leaf of a graph, that operand in every form, the rest plain: blur_bias_act (residual, bias),
     bias_act (residual, bias), conv2d(residual=), conv_transpose2d, upfirdn2d up 2 / down 2, bilinear_down, minibatch_stddev, linear_bias_act (bias).
  4. refusals, under forbidden(): wrong dtype, device, length or shape raises GifHipError naming the operand, launches nothing, caches nothing.

Findings, parent -> now.  Only the first was run on the device against the parent's functional.py (once, in bounds: the residual has the output's
element count); the others are read from the parent's code — under the hooks they stop before the call, which shows nothing the reading does not.
  * blur_bias_act with an NCHW-contiguous residual: BlurBiasActFn handed it to the FIR epilogue untouched and it was read as NHWC, no error;
    [blur_bias_act-residual-nchw] failed with "grad x: 4624 of 4624 elements differ from the plain run (0 NaN)" (y and the other gradients as
    well) -> ops.upfirdn2d converts with nhwc(), ops._epilogue refuses a residual that is not an aligned NHWC tensor of the output's shape.
  * bias / in_scale / out_scale / FIR taps and the scales of conv_wgrad went in as data_ptr() of whatever they were: a stride-2 bias was read
    across its NaN gap, float64, CPU and unpadded-length vectors were launched -> ops._vec: fp32, device, exact length, dense, aligned, or refused.
  * a float64, half or CPU weight was packed as if it were fp32 device memory -> refused before the cache is looked at.  The epilogue is now
    assembled BEFORE the weights are packed: at the parent a refusal-to-be came after the pack launch.
  * a dense NHWC view one float into a buffer (data_ptr() % 16 == 4) passed ops.nhwc() unchanged -> copied to an aligned tensor.
  * streams: every call site passes the current stream, on autograd's thread as well; nothing to fix.
  * beyond the issue's list: ops._mat's own alignment guard fell through to t.contiguous(), which returns a dense matrix at an odd offset
    unchanged — [demod_closed-offset4] stopped "gif_style_demod_f32: argument 0 ... is not 16-byte aligned" on this tree before the fix -> a copy.
    act_inv_mul_reduce took residual and bias raw (its one caller converts first) -> nhwc() and _vec there too.
"""
import contextlib

import pytest
import torch

import graph_cases as G
import ops_forms as OF
from gpu_util import dev
from test_gpu_input_forms import recorded_launches

pytestmark = pytest.mark.gpu
CASES = [c.name for c in G.CASES]


@pytest.fixture(autouse=True)
def _restore():
    from gif_amd import ops
    before, fuse = ops.get_fp32_mfma_mode(), ops.FUSE_GRAD
    yield
    ops.set_fp32_mfma_mode(before)
    ops.FUSE_GRAD = fuse


@contextlib.contextmanager
def watched(formname):
    """Everything inside runs under checked(the stream it must run on); side_stream: inside torch.cuda.stream(a fresh stream), ordered after the
    current stream's work before and ahead of it after, and at least one launch must have been recorded."""
    cur = torch.cuda.current_stream()
    if formname != "side_stream":
        with recorded_launches(before=OF.checked(cur.cuda_stream)) as rec:
            yield rec
        return
    fresh = torch.cuda.Stream()
    assert fresh.cuda_stream != cur.cuda_stream
    fresh.wait_stream(cur)
    with recorded_launches(before=OF.checked(fresh.cuda_stream)) as rec, torch.cuda.stream(fresh):
        yield rec
    cur.wait_stream(fresh)
    assert rec.streams(), "no launch of the library was recorded"
    assert all(s == fresh.cuda_stream for _, s in rec.streams())


def same_bits(got, want, what):
    assert got.keys() == want.keys(), (what, sorted(got), sorted(want))
    for k, a in got.items():
        b = want[k]
        if a is None or b is None:
            assert a is None and b is None, f"{what}: {k}: one of the two runs has no result"
            continue
        assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: {k}: {tuple(a.shape)} {a.dtype} against {tuple(b.shape)} {b.dtype}"
        assert torch.equal(a, b), f"{what}: {k}: {int((a != b).sum())} of {a.numel()} elements differ from the plain run ({int(torch.isnan(a).sum())} NaN)"


# ---------------------------------------------------------------------------------------------------------------------------- 1. graphs
def graph_run(case, formname, conv):
    with watched(formname) as rec:
        g = G.Graph(case, conv)
        grads = g.grads()
    torch.cuda.synchronize()
    res = {f"out{i}": o.detach() for i, o in enumerate(g.outs)}
    res.update({f"tap {k}": y.detach() for k, y in g.taps.items()})
    for k, v in grads.items():
        leaf = g.L[k]
        assert v.shape == leaf.shape and v.dtype == leaf.dtype and v.device == leaf.device, (k, tuple(v.shape), v.dtype)
        res[f"grad {k}"] = v
    return res, rec, g.L


_plain = {}


def plain_graph(name, partner="plain"):
    """The plain run of a case (or of the expanded form's materialised batch), once; under `checked` like every other run."""
    if (name, partner) not in _plain:
        case = G.BY_NAME[name]
        res, rec, L = graph_run(case, "plain", OF.form(partner))
        assert all(bool(torch.isfinite(v.float()).all()) for v in res.values()), f"{name}: the plain run is not finite"
        if partner == "plain":
            # a dense aligned input costs no copy: the forward convolutions read the activation leaves at their own addresses
            fwd = [a[0] for n, a in rec.calls if n.startswith(("gif_conv2d_fwd", "gif_conv3x3_winograd_f"))]
            xs = {k: L[k].data_ptr() for k, kind, _ in case.leaves if kind == "x"}
            assert fwd and fwd[0] in xs.values(), f"{name}: the first forward convolution reads {fwd[:1]}, the activation leaves are at {xs}"
            assert all(p in fwd for p in xs.values()), f"{name}: an activation leaf was copied before its convolution: {xs}, read {fwd}"
        _plain[name, partner] = res
    return _plain[name, partner]


@pytest.mark.parametrize("formname", OF.FORMS)
@pytest.mark.parametrize("name", CASES)
def test_graph_in_a_form_gives_the_plain_bits(name, formname):
    want = plain_graph(name, OF.PARTNER.get(formname, "plain"))
    got, rec, _ = graph_run(G.BY_NAME[name], formname, OF.form(formname))
    same_bits(got, want, f"{name} {formname}")


# ---------------------------------------------------------------------------------------------------------------------- 2. second order
_plain_u5 = {}


def u5_run(name, target, formname):
    with watched(formname):
        g, grads, _ = G.u5(G.BY_NAME[name], OF.form(formname), target)
    return dict({f"grad {k}": v for k, v in grads.items()}, g=g)


@pytest.mark.parametrize("formname", ["nchw", "wide", "side_stream"])
@pytest.mark.parametrize("name,target", [(c.name, t) for c in G.CASES for t in c.second])
def test_recorded_backward_in_a_form_gives_the_plain_bits(name, target, formname):
    if (name, target) not in _plain_u5:
        _plain_u5[name, target] = u5_run(name, target, "plain")
    same_bits(u5_run(name, target, formname), _plain_u5[name, target], f"{name} u5({target}) {formname}")


# ------------------------------------------------------------------------------------- 3. operands that are never the leaf of a graph
def _k(scale=1.0):
    return (G.FIR * scale).cuda()


def _blur(L):
    from gif_amd import functional as GF
    return GF.blur_bias_act(L["x"], _k(4), (1, 1), L["residual"], L["bias"])


def _bias_act(L):
    from gif_amd import functional as GF
    return GF.bias_act(L["x"], L["bias"], L["residual"])


def _conv_res(L):
    from gif_amd import functional as GF
    return GF.conv2d(L["x"], L["w"], 1, 1, wscale=0.1, residual=L["residual"])


def _conv_t(L):
    from gif_amd import functional as GF
    return GF.conv_transpose2d(L["x"], L["w"], 2, 0, (33, 33), wscale=0.1)


def _fir_up(L):
    from gif_amd import functional as GF
    return GF.upfirdn2d(L["x"], _k(4), up=2, down=1, pad=(2, 1))


def _fir_down(L):
    from gif_amd import functional as GF
    return GF.upfirdn2d(L["x"], _k(), up=1, down=2, pad=(1, 1))


def _bil(L):
    from gif_amd import functional as GF
    return GF.bilinear_down(L["x"], 8)


def _mbstd(L):
    from gif_amd import functional as GF
    return GF.minibatch_stddev(L["x"], 2, 12)


def _linear(L):
    from gif_amd import functional as GF
    return GF.linear_bias_act(L["x"], L["w"], L["bias"], 0.3, True, 0.2, 2 ** 0.5, 8)


_X = ("x", "x", (2, 8, 16, 16))
_R = ("residual", "x", (2, 8, 16, 16))
_B = ("bias", "b", (8,))
_W = ("w", "w", (8, 8, 3, 3))
# op: (leaves (name, kind, shape), the call, its output's spatial size, the operands taken through the forms)
OPS = {
    "blur_bias_act": ((("x", "x", (2, 8, 17, 17)), _R, _B), _blur, (16, 16), ("residual", "bias")),
    "bias_act": ((_X, _B, _R), _bias_act, (16, 16), ("residual", "bias")),
    "conv2d_residual": ((_X, _W, _R), _conv_res, (16, 16), ("residual", "x", "w")),
    "conv_transpose2d": ((_X, _W), _conv_t, (33, 33), ("x", "w")),
    "upfirdn2d_up2": ((_X,), _fir_up, (32, 32), ("x",)),
    "upfirdn2d_down2": ((_X,), _fir_down, (8, 8), ("x",)),
    "bilinear_down": ((_X,), _bil, (8, 8), ("x",)),
    "minibatch_stddev": ((("x", "x", (4, 8, 4, 4)),), _mbstd, (4, 4), ("x",)),
    "linear_bias_act": ((("x", "s", (2, 8)), ("w", "s", (8, 8)), _B), _linear, None, ("bias",)),
}
OP_TABLE = [(op, operand, f) for op, (leaves, _, _, varied) in OPS.items() for operand in varied for f in OF.FORMS
            if {n: k for n, k, _ in leaves}[operand] in OF.APPLIES[f]]


def op_run(opname, operand, formname, place):
    leaves, fn, hw, _ = OPS[opname]
    gen, plain = torch.Generator().manual_seed(11), OF.form("plain")
    L = {n: (place if n == operand else plain)(k, torch.randn(*shape, generator=gen)).requires_grad_(True) for n, k, shape in leaves}
    with watched(formname):
        y = fn(L)
        assert hw is None or tuple(y.shape[2:]) == hw, (opname, tuple(y.shape))
        grads = torch.autograd.grad(y.pow(2).sum(), list(L.values()))
    torch.cuda.synchronize()
    for (n, t), g in zip(L.items(), grads):
        assert g.shape == t.shape and g.dtype == t.dtype, (opname, n, tuple(g.shape), g.dtype)
    return dict({f"grad {n}": g for n, g in zip(L, grads)}, y=y.detach())


@pytest.mark.parametrize("opname,operand,formname", OP_TABLE, ids=[f"{o}-{a}-{f}" for o, a, f in OP_TABLE])
def test_op_operand_in_a_form_gives_the_plain_bits(opname, operand, formname):
    want = op_run(opname, operand, "plain", OF.partner(formname))
    assert all(bool(torch.isfinite(v).all()) for v in want.values()), f"{opname}: the plain run is not finite"
    same_bits(op_run(opname, operand, formname, OF.form(formname)), want, f"{opname} {operand} {formname}")


def test_every_operand_the_forms_apply_to_is_in_the_table():
    assert len(OP_TABLE) == sum(len([f for f in OF.FORMS if {n: k for n, k, _ in lv}[a] in OF.APPLIES[f]]) for lv, _, _, var in OPS.values() for a in var)
    assert ("blur_bias_act", "residual", "nchw") in OP_TABLE and ("linear_bias_act", "bias", "offset4") in OP_TABLE
    assert set(OF.APPLIES) == set(OF.FORMS) and len(CASES) * len(OF.FORMS) == 91


# ------------------------------------------------------------------------------------------------------------------------- 4. refusals
def _refusal_operands():
    """6 logical channels in activations of 8: the unpadded count is the wrong length for every per-channel and per-sample vector"""
    g = torch.Generator().manual_seed(5)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    return dict(x=dev(r(2, 6, 16, 16)), w=r(6, 6, 3, 3).cuda(), b=r(8).cuda(), s=(1 + 0.1 * r(2, 8)).cuda(), d=(1 + 0.1 * r(2, 8)).cuda(),
                k=_k(), res=dev(r(2, 6, 16, 16)))


def _refusals():
    from gif_amd import functional as GF
    mc = lambda o, **kw: GF.modulated_conv2d_act(o["x"], o["w"], kw.get("s", o["s"]), kw.get("d", o["d"]), None, kw.get("b", o["b"]), 1)  # noqa: E731
    return {
        "float64 weight": ("weight", lambda o: GF.conv2d(o["x"], o["w"].double(), 1, 1)),
        "half weight": ("weight", lambda o: GF.conv2d(o["x"], o["w"].half(), 1, 1)),
        "cpu weight": ("weight", lambda o: GF.conv2d(o["x"], o["w"].cpu(), 1, 1)),
        "cpu weight, transposed": ("weight", lambda o: GF.conv_transpose2d(o["x"], o["w"].cpu(), 2, 0, (33, 33))),
        "float64 bias": ("bias", lambda o: GF.conv2d_bias_act(o["x"], o["w"], o["b"].double(), 1, 1)),
        "float64 bias, bias_act": ("bias", lambda o: GF.bias_act(o["x"], o["b"].double())),
        "float64 bias, blur": ("bias", lambda o: GF.blur_bias_act(o["x"], o["k"], (2, 1), None, o["b"].double())),
        "float64 s": ("in_scale", lambda o: mc(o, s=o["s"].double())),
        "float64 d": ("out_scale", lambda o: mc(o, d=o["d"].double())),
        "float64 k": (r"k \(FIR taps\)", lambda o: GF.upfirdn2d(o["x"], o["k"].double(), pad=(2, 1))),
        "short bias": ("bias", lambda o: GF.conv2d_bias_act(o["x"], o["w"], o["b"][:6].contiguous(), 1, 1)),
        "short bias, bias_act": ("bias", lambda o: GF.bias_act(o["x"], o["b"][:6].contiguous())),
        "short s": ("in_scale", lambda o: mc(o, s=o["s"][:, :6].contiguous())),
        "short d": ("out_scale", lambda o: mc(o, d=o["d"][:, :6].contiguous())),
        "short s, modulated_conv2d": ("in_scale", lambda o: GF.modulated_conv2d(o["x"], o["w"], o["s"][:, :6].contiguous(), None, pad=1)),
        "cpu bias": ("bias", lambda o: GF.conv2d_bias_act(o["x"], o["w"], o["b"].cpu(), 1, 1)),
        "cpu bias, bias_act": ("bias", lambda o: GF.bias_act(o["x"], o["b"].cpu())),
        "cpu k": (r"k \(FIR taps\)", lambda o: GF.upfirdn2d(o["x"], o["k"].cpu(), pad=(2, 1))),
        "residual of another shape": ("residual", lambda o: GF.conv2d(o["x"], o["w"], 1, 1, residual=o["res"][:, :, :8, :8])),
        "residual of another shape, blur": ("residual", lambda o: GF.blur_bias_act(o["x"], o["k"], (2, 1), o["res"][:, :, :8], o["b"])),
        "residual of another shape, bias_act": ("residual", lambda o: GF.bias_act(o["x"], o["b"], o["res"][:, :4])),
        "residual of another shape, modulated": ("residual", lambda o: GF.modulated_conv2d_act(o["x"], o["w"], o["s"], o["d"], o["res"][:1], o["b"], 1)),
    }


REFUSALS = ["float64 weight", "half weight", "cpu weight", "cpu weight, transposed", "float64 bias", "float64 bias, bias_act", "float64 bias, blur",
            "float64 s", "float64 d", "float64 k", "short bias", "short bias, bias_act", "short s", "short d", "short s, modulated_conv2d", "cpu bias",
            "cpu bias, bias_act", "cpu k", "residual of another shape", "residual of another shape, blur", "residual of another shape, bias_act",
            "residual of another shape, modulated"]


@pytest.mark.parametrize("what", REFUSALS)
def test_refusal_names_the_operand_and_launches_nothing(what):
    from gif_amd import _lib, ops
    table = _refusals()
    assert list(table) == REFUSALS
    operand, call = table[what]
    o = _refusal_operands()
    torch.cuda.synchronize()
    ops.clear_weight_cache()
    with recorded_launches(before=OF.forbidden()) as rec:
        with pytest.raises(_lib.GifHipError, match=operand) as err:
            call(o)
    print(f"\n[refusal] {what}: {err.value}")
    assert rec.streams() == [], f"{what}: launched {rec.streams()}"
    assert not ops._weight_cache, f"{what}: cached {list(ops._weight_cache)}"


def test_the_refusal_operands_are_accepted_as_they_are():
    """the same calls with the operands of _refusal_operands unchanged run (so every refusal above is about the one operand it changes)"""
    from gif_amd import functional as GF
    o = _refusal_operands()
    with watched("plain") as rec:
        ys = [GF.conv2d(o["x"], o["w"], 1, 1, residual=o["res"]), GF.conv2d_bias_act(o["x"], o["w"], o["b"], 1, 1), GF.bias_act(o["x"], o["b"], o["res"]),
              GF.modulated_conv2d_act(o["x"], o["w"], o["s"], o["d"], o["res"], o["b"], 1), GF.upfirdn2d(o["x"], o["k"], pad=(2, 1)),
              GF.blur_bias_act(o["x"], o["k"], (2, 1), o["res"], o["b"]), GF.modulated_conv2d(o["x"], o["w"], o["s"], None, pad=1)]
    torch.cuda.synchronize()
    assert rec.streams() and all(bool(torch.isfinite(y).all()) and tuple(y.shape) == (2, 8, 16, 16) for y in ys)
