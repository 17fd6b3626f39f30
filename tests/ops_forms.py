"""TEST INFRASTRUCTURE ONLY — what the conv-side bindings of gif_amd/ops.py (conv, FIR, bias / activation, reductions, minibatch stddev, the
style path: some sixty direct ctypes calls, each taking t.data_ptr() and the current stream by hand) are fed in tests/test_gpu_functional_forms.py,
and the two hooks that look at every call BEFORE it reaches the library (recorded_launches(before=...), tests/test_gpu_input_forms.py).

The forms.  form(name, device) is a conv(kind, tensor) callable for graph_cases.make_leaves: it places the fp32 CPU draw `tensor` of kind x
(activation, logical [B,C,H,W]) | w ([O,I,KH,KW]) | b ([C]) | s | d ([B,C]) on `device` in the named form.  Every form asserts that it is what
it claims to be, and wherever a form leaves a gap in its buffer the gap holds NaN: one stray read poisons the result.
  plain          x: channels zero-padded to a multiple of 4, dense NHWC at storage offset 0 (gpu_util.dev); the rest dense (.cuda())
  nchw           x: channel-padded and NCHW-contiguous — the layout any torch user's tensor has
  wide           x = [:, :C] of an NHWC tensor with C + 4 channels; w = [:O, :I] of [O+2, I+4, KH, KW]; b = [::2] of [2C]; s, d = [:, :C] of [B, C+4]
  permuted       x stored with H and W swapped, transposed back; w stored [KH, KW, I, O], permuted back; s, d stored [C, B], .t()
  expanded       sample 0 of x, s, d expanded over the batch with stride 0        plain partner: expanded_plain, that batch materialised
  batch_offset   x, s, d = rows 1 : 1 + B of a tensor with B + 2 rows: a storage offset that stays 16-byte aligned
  offset4        x, b, s, d dense in their own layout, one float into a larger buffer: data_ptr() % 16 == 4.  (w stays plain: UNALIGNED_OK
                 exempts every reader of a source weight, and a kernel is never handed a misaligned pointer on purpose.)
  side_stream    plain tensors; the test runs forward and backward inside torch.cuda.stream(a fresh stream)
to_rgb_f16 casts its activation to half after the form was applied (graph_cases.make_leaves): a dense form keeps its strides through the cast,
`wide` and `offset4` come out of it as a dense aligned copy.

The hooks.
  pointer_args(name, args)  [(where, address)] of the non-null addresses a call hands over, found from _lib.PROTOTYPES[name]: where = the argument
                            index, or (index, field) for the pointers inside a byref(ConvEpilogue) / (index, segment, field) inside a
                            LinearBankSeg array; the trailing stream is left out.  Host pointers (geometry structs, int out-parameters) are not device
                            addresses and are not listed.
  checked(stream)           raises AssertionError (entry and argument named) when a launch is handed another stream than `stream`, or any call a
                            pointer that is not 16-byte aligned and not listed in UNALIGNED_OK
  forbidden()               raises on any launch; size and eligibility queries pass
Both raise before the call is forwarded: a misaligned, host or wrongly typed pointer never reaches the GPU, a missing check in the bindings shows up
as a test failure."""
import ctypes

import torch
import torch.nn.functional as F

NAN = float("nan")
EPILOGUE_FIELDS = ("in_scale", "out_scale", "bias", "residual", "mask_src", "dot_src", "dot", "colsum", "red_ws")
BANK_FIELDS = ("w", "bias", "s", "gs", "gw", "gbias")

# Operands a kernel reads element by element through a base address and runtime element strides: a 4-byte-aligned float address is all they
# need.  Every row is the SOURCE weight w (argument 0) of a packing / transform entry point; the line is where the kernel reads it:
#   v = scale * w[r * sr + c * sc + ky * sky + kx * skx]    (one float per thread; sr, sc, sky, skx are kernel arguments, nothing to vectorise)
_W = "source weight, read one float at a time through runtime element strides: "
UNALIGNED_OK = {
    "gif_pack_weight_f32": {0: _W + "csrc/weight_pack.hip:21 (pack_weight_kernel)"},
    "gif_pack_weight_f16": {0: _W + "csrc/weight_pack.hip:21 (pack_weight_kernel, T = f16)"},
    "gif_pack_weight_f32x3": {0: _W + "csrc/weight_pack.hip:37 (pack_weight_x3_kernel)"},
    "gif_pack_weight_f32x3_tapdense": {0: _W + "csrc/weight_pack.hip:60 (pack_weight_x3_dense_kernel)"},
    "gif_pack_weight_f32h2": {0: _W + "csrc/conv_wgrad.hip:973 (pack_h2)"},
    "gif_pack_weight_f32h2x3": {0: _W + "csrc/conv_wgrad.hip:973 (pack_h2)"},
    "gif_pack_weight_f32h2x3_tapdense": {0: _W + "csrc/conv_wgrad.hip:973 (pack_h2)"},
    "gif_winograd_weight_f32": {0: _W + "csrc/conv_winograd.hip:213"},
    "gif_winograd_weight_f32x3": {0: _W + "csrc/conv_winograd.hip:1133"},
    "gif_winograd_weight_f32h2": {0: _W + "csrc/conv_winograd.hip:1053 (wino_weight_transform_h2)"},
}


# ----------------------------------------------------------------------------------------------------------------------------- the hooks
def _protos():
    from gif_amd import _lib
    return _lib


def has_stream(name):
    """the entry's last parameter is the stream"""
    L = _protos()
    res, argtypes = L.PROTOTYPES[name]
    return res is L.c_int and bool(argtypes) and argtypes[-1] is L.P


def is_launch(name):
    """as recorded_launches.streams() defines a launch"""
    return has_stream(name) and not name.startswith("gif_f16_overflow")


def _addr(v):
    if v is None:
        return 0
    if isinstance(v, ctypes.c_void_p):
        return v.value or 0
    return int(v)


def pointer_args(name, args):
    L = _protos()
    _, argtypes = L.PROTOTYPES[name]
    assert len(args) == len(argtypes), f"{name}: {len(args)} arguments for {len(argtypes)} parameters"
    n = len(argtypes) - 1 if has_stream(name) else len(argtypes)
    out = []
    for i in range(n):
        ty, a = argtypes[i], args[i]
        if ty is L.P:
            if _addr(a):
                out.append((i, _addr(a)))
        elif ty is L.EP and a is not None:
            e = a._obj if hasattr(a, "_obj") else a.contents if hasattr(a, "contents") else a  # byref(e) | pointer(e) | e
            out += [((i, f), _addr(getattr(e, f))) for f in EPILOGUE_FIELDS if _addr(getattr(e, f))]
        elif ty is ctypes.POINTER(L.LinearBankSeg) and a is not None:
            for j, seg in enumerate(a):
                out += [((i, j, f), _addr(getattr(seg, f))) for f in BANK_FIELDS if _addr(getattr(seg, f))]
    return out


def checked(stream, unaligned_ok=None):
    ok = UNALIGNED_OK if unaligned_ok is None else unaligned_ok

    def before(name, args):
        if is_launch(name):
            assert _addr(args[-1]) == _addr(stream), \
                f"{name}: argument {len(args) - 1} (the stream) is {_addr(args[-1]):#x}, the current stream is {_addr(stream):#x}"
        for where, addr in pointer_args(name, args):
            exempt = ok.get(name, {})
            if addr % 16 and where not in exempt:
                raise AssertionError(f"{name}: argument {where} = {addr:#x} is not 16-byte aligned (address % 16 = {addr % 16})")
    return before


def forbidden():
    def before(name, args):
        assert not is_launch(name), f"{name}: a launch where the binding had to refuse its operands (arguments {args})"
    return before


# ----------------------------------------------------------------------------------------------------------------------------- the forms
def _padc(t):
    c = t.shape[1]
    return t if c % 4 == 0 else F.pad(t, (0, 0, 0, 0, 0, (c + 3) // 4 * 4 - c))


def _nhwc_in(buf, B, H, W, C):
    """logical [B,C,H,W] over a physical [B,H,W,C] buffer"""
    return buf.view(B, H, W, C).permute(0, 3, 1, 2)


class Forms:
    def __init__(self, device="cuda"):
        self.device = torch.device(device)

    def to(self, t):
        return t.to(self.device)

    # every method: (kind, fp32 CPU tensor) -> the tensor the op is given
    def plain(self, kind, t):
        if kind != "x":
            return self.to(t.contiguous())
        y = self.to(_padc(t)).contiguous(memory_format=torch.channels_last)
        assert y.storage_offset() == 0 and y.data_ptr() % 16 == 0
        return y

    side_stream = plain

    def nchw(self, kind, t):
        if kind != "x":
            return self.plain(kind, t)
        y = self.to(_padc(t).contiguous())
        assert y.is_contiguous() and not y.is_contiguous(memory_format=torch.channels_last)
        return y

    def wide(self, kind, t):
        if kind == "x":
            t = _padc(t)
            B, C, H, W = t.shape
            buf = torch.full((B, H, W, C + 4), NAN)
            buf[..., :C] = t.permute(0, 2, 3, 1)
            v = self.to(buf).permute(0, 3, 1, 2)[:, :C]
            assert v.stride() == ((C + 4) * H * W, 1, (C + 4) * W, C + 4) and not v.is_contiguous(memory_format=torch.channels_last)
        elif kind == "w":
            O, I, KH, KW = t.shape
            buf = torch.full((O + 2, I + 4, KH, KW), NAN)
            buf[:O, :I] = t
            v = self.to(buf)[:O, :I]
            assert v.stride(0) == (I + 4) * KH * KW
        elif kind == "b":
            buf = torch.full((2 * t.shape[0],), NAN)
            buf[::2] = t
            v = self.to(buf)[::2]
            assert v.stride() == (2,)
        else:
            B, C = t.shape
            buf = torch.full((B, C + 4), NAN)
            buf[:, :C] = t
            v = self.to(buf)[:, :C]
            assert v.stride() == (C + 4, 1)
        assert not v.is_contiguous() and v.shape == (_padc(t).shape if kind == "x" else t.shape)
        return v

    def permuted(self, kind, t):
        if kind == "x":
            t = _padc(t)
            v = self.to(t.transpose(2, 3).contiguous(memory_format=torch.channels_last)).transpose(2, 3)
            assert v.shape == t.shape and not v.is_contiguous(memory_format=torch.channels_last) and not v.is_contiguous()
        elif kind == "w":
            v = self.to(t.permute(2, 3, 1, 0).contiguous()).permute(3, 2, 0, 1)
            assert v.shape == t.shape and v.stride(0) == 1 and not v.is_contiguous()
        elif kind in "sd":
            v = self.to(t.t().contiguous()).t()
            assert v.shape == t.shape and v.stride() == (1, t.shape[0]) and not v.is_contiguous()
        else:
            return self.plain(kind, t)
        return v

    def expanded(self, kind, t):
        if kind not in "xsd":
            return self.plain(kind, t)
        v = self.plain(kind, t[:1].clone()).expand(t.shape[0], *[-1] * (t.dim() - 1))
        assert v.stride(0) == 0 and v.shape[0] == t.shape[0]
        return v

    def expanded_plain(self, kind, t):
        if kind not in "xsd":
            return self.plain(kind, t)
        return self.plain(kind, t[:1].expand(t.shape[0], *[-1] * (t.dim() - 1)).contiguous())

    def batch_offset(self, kind, t):
        if kind not in "xsd":
            return self.plain(kind, t)
        t = _padc(t) if kind == "x" else t
        B = t.shape[0]
        buf = torch.full((B + 2,) + tuple(t.shape[1:]), NAN)
        buf[1:1 + B] = t
        buf = self.to(buf.contiguous(memory_format=torch.channels_last) if kind == "x" else buf)
        v = buf[1:1 + B]
        assert v.storage_offset() == t[0].numel() and v.data_ptr() % 16 == 0 and v.data_ptr() != buf.data_ptr()
        assert v.is_contiguous(memory_format=torch.channels_last) if kind == "x" else v.is_contiguous()
        return v

    def offset4(self, kind, t):
        if kind == "w":
            assert all(0 in UNALIGNED_OK[n] for n in UNALIGNED_OK), "a reader of w is not exempt: give w the offset as well"
            return self.plain(kind, t)
        t = _padc(t) if kind == "x" else t
        n = t.numel()
        buf = torch.full((n + 4,), NAN)
        buf[1:1 + n] = (t.permute(0, 2, 3, 1) if kind == "x" else t).reshape(-1)
        buf = self.to(buf)
        if kind == "x":
            B, C, H, W = t.shape
            v = _nhwc_in(buf[1:1 + n], B, H, W, C)
            assert v.is_contiguous(memory_format=torch.channels_last)
        else:
            v = buf[1:1 + n].view(t.shape)
            assert v.is_contiguous()
        assert buf.data_ptr() % 16 == 0 and v.data_ptr() % 16 == 4 and v.storage_offset() == 1
        return v


FORMS = ("nchw", "wide", "permuted", "expanded", "batch_offset", "offset4", "side_stream")
PARTNER = {"expanded": "expanded_plain"}  # the plain run a form is compared with (default: plain)
APPLIES = {"nchw": "x", "wide": "xwbsd", "permuted": "xwsd", "expanded": "xsd", "batch_offset": "xsd", "offset4": "xbsd",
           "side_stream": "xwbsd"}  # kinds a form changes (the others it leaves plain)


def form(name, device="cuda"):
    return getattr(Forms(device), name)


def partner(name, device="cuda"):
    return form(PARTNER.get(name, "plain"), device)


def values(name, kind, t):
    """the dense fp32 CPU tensor a form stands for"""
    t = _padc(t) if kind == "x" else t
    if (name in PARTNER or name in PARTNER.values()) and kind in "xsd":
        t = t[:1].expand(t.shape[0], *[-1] * (t.dim() - 1)).contiguous()
    return t
