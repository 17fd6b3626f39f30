"""The tools of tests/ops_forms.py would catch what they exist to catch — checked without a GPU and without the library: the forms on CPU tensors,
the hooks against a fake library object that records whether an entry point was reached."""
import ctypes

import pytest
import torch

import ops_forms as OF
from test_gpu_input_forms import recorded_launches

SHAPES = {"x": (2, 6, 5, 7), "w": (5, 6, 3, 3), "b": (8,), "s": (2, 8), "d": (2, 8)}  # (6 channels: padded to 8 like gpu_util.dev)
GAP = {"wide": "xwbsd", "batch_offset": "xsd", "offset4": "xbsd"}  # kinds whose buffer is larger than the view


def _storage(v):
    return torch.empty(0, dtype=v.dtype).set_(v.untyped_storage())


@pytest.mark.parametrize("kind", list(SHAPES))
@pytest.mark.parametrize("name", ("plain", "expanded_plain") + OF.FORMS)
def test_form_has_the_plain_values_and_its_strides_offset_and_gap(name, kind):
    t = torch.randn(*SHAPES[kind], generator=torch.Generator().manual_seed(3))
    v = OF.form(name, "cpu")(kind, t)  # (asserts its own strides and offset)
    want = OF.values(name, kind, t)
    assert v.dtype == torch.float32 and v.shape == want.shape and torch.equal(v, want), (name, kind)
    if kind == "x" and name != "expanded":
        assert torch.equal(v[:, 6:], torch.zeros_like(v[:, 6:])), "the padding channels are zero"
    store = _storage(v)
    nans = int(torch.isnan(store).sum())
    if kind in GAP.get(name, ""):
        assert nans == store.numel() - v.numel() > 0, (name, kind, nans, store.numel(), v.numel())
    else:
        assert nans == 0 and store.numel() == (v[:1].numel() if name == "expanded" and kind in "xsd" else v.numel())
    # the claims, stated once more from outside
    cl = torch.channels_last
    if name == "offset4" and kind != "w":
        assert v.data_ptr() % 16 == 4
    if name == "batch_offset" and kind in "xsd":
        assert v.storage_offset() > 0 and v.data_ptr() % 16 == 0
    if name == "expanded" and kind in "xsd":
        assert v.stride(0) == 0
    if name in ("wide", "permuted") and kind != "b" or (name, kind) == ("wide", "b"):
        assert not v.is_contiguous() and not (v.dim() == 4 and v.is_contiguous(memory_format=cl))
    if name == "nchw" and kind == "x":
        assert v.is_contiguous() and not v.is_contiguous(memory_format=cl)
    if name in ("plain", "side_stream"):
        assert v.storage_offset() == 0 and (v.is_contiguous(memory_format=cl) if kind == "x" else v.is_contiguous())


# --------------------------------------------------------------------------------------------------------------------------- the hooks
class FakeLib:
    """Stands where _lib.load() keeps the loaded library: four real prototypes, every call counted, nothing launched."""
    NAMES = ("gif_bias_act_f32", "gif_conv2d_fwd_f32", "gif_conv2d_pack_dims", "gif_pack_weight_f32", "gif_linear_bank_fwd_f32")

    def __init__(self):
        self.reached = []

    def __getattr__(self, name):
        if name not in FakeLib.NAMES:
            raise AttributeError(name)
        return lambda *args: self.reached.append(name) or 0


@pytest.fixture
def fake():
    from gif_amd import _lib
    saved, lib = _lib._lib, FakeLib()
    _lib._lib = lib
    yield lib
    _lib._lib = saved


def _conv_args(stream, **fields):
    from gif_amd import _lib
    g, e = _lib.ConvGeom(1, 4, 4, 4, 4, 4, 4, 3, 3, 1, 1), _lib.ConvEpilogue()
    for k, v in fields.items():
        setattr(e, k, v)
    return (0x1000, 0x2000, 0x3000, ctypes.byref(g), ctypes.byref(e), stream)


BIAS_ACT = (0x1000, None, 0x2000, 0x3000, 64, 8, 0.2, 1.0, 0x77)  # x, bias = NULL, residual, y, rows, C, slope, gain, stream


def test_pointer_args():
    from gif_amd import _lib
    assert OF.pointer_args("gif_bias_act_f32", BIAS_ACT) == [(0, 0x1000), (2, 0x2000), (3, 0x3000)]  # no NULL, no stream
    got = OF.pointer_args("gif_conv2d_fwd_f32", _conv_args(0x77, bias=0x4004, residual=0x5000, red_ws=0x6000, act=1))
    assert got == [(0, 0x1000), (1, 0x2000), (2, 0x3000), ((4, "bias"), 0x4004), ((4, "residual"), 0x5000), ((4, "red_ws"), 0x6000)]
    assert OF.pointer_args("gif_conv2d_pack_dims", (8, 8, ctypes.byref(ctypes.c_int()), ctypes.byref(ctypes.c_int()))) == []
    segs = (_lib.LinearBankSeg * 2)()
    segs[0].w, segs[1].w, segs[1].bias, segs[1].n = 0x1000, 0x2000, 0x2104, 8
    assert OF.pointer_args("gif_linear_bank_fwd_f32", (0x9000, 2, 8, 8, segs, 2, 1.0, 0x77)) == \
        [(0, 0x9000), ((4, 0, "w"), 0x1000), ((4, 1, "w"), 0x2000), ((4, 1, "bias"), 0x2104)]
    assert OF.is_launch("gif_bias_act_f32") and not OF.is_launch("gif_conv2d_pack_dims") and not OF.is_launch("gif_conv_epilogue_ws_floats")
    assert set(OF.EPILOGUE_FIELDS) == {n for n, t in _lib.ConvEpilogue._fields_ if t is _lib.P}
    assert set(OF.BANK_FIELDS) == {n for n, t in _lib.LinearBankSeg._fields_ if t is _lib.P}
    assert all(n in _lib.PROTOTYPES and _lib.PROTOTYPES[n][1][i] is _lib.P for n, row in OF.UNALIGNED_OK.items() for i in row)


def test_checked_stops_a_misaligned_pointer_and_a_foreign_stream_before_the_call(fake):
    from gif_amd import _lib
    with recorded_launches(before=OF.checked(0x77)) as rec:
        lib = _lib.load()
        assert lib.gif_bias_act_f32(*BIAS_ACT) == 0 and lib.gif_conv2d_fwd_f32(*_conv_args(0x77, bias=0x4000)) == 0
        assert fake.reached == ["gif_bias_act_f32", "gif_conv2d_fwd_f32"] and len(rec.calls) == 2
        with pytest.raises(AssertionError, match=r"gif_conv2d_fwd_f32: argument \(4, 'bias'\).*not 16-byte aligned"):
            lib.gif_conv2d_fwd_f32(*_conv_args(0x77, bias=0x4004))
        with pytest.raises(AssertionError, match=r"gif_bias_act_f32: argument 2 .*not 16-byte aligned"):
            lib.gif_bias_act_f32(*(BIAS_ACT[:2] + (0x2008,) + BIAS_ACT[3:]))
        with pytest.raises(AssertionError, match=r"gif_bias_act_f32: argument 8 \(the stream\)"):
            lib.gif_bias_act_f32(*(BIAS_ACT[:-1] + (0x88,)))
        with pytest.raises(AssertionError, match="the stream"):
            lib.gif_bias_act_f32(*(BIAS_ACT[:-1] + (None,)))  # (the default stream is another stream than 0x77)
        # the exemption covers the listed argument of the listed entry and nothing else
        pack = (0x1004, 0x2000, 8, 8, 3, 3, 32, 32, 72, 9, 3, 1, 1.0, 0x77)
        assert lib.gif_pack_weight_f32(*pack) == 0
        with pytest.raises(AssertionError, match=r"gif_pack_weight_f32: argument 1 "):
            lib.gif_pack_weight_f32(*((0x1000, 0x2004) + pack[2:]))
        assert fake.reached == ["gif_bias_act_f32", "gif_conv2d_fwd_f32", "gif_pack_weight_f32"] and len(rec.calls) == 3, "a refused call went through"
        assert rec.streams() == [("gif_bias_act_f32", 0x77), ("gif_conv2d_fwd_f32", 0x77), ("gif_pack_weight_f32", 0x77)]
    with recorded_launches(before=OF.checked(0x77, unaligned_ok={})):
        with pytest.raises(AssertionError, match=r"gif_pack_weight_f32: argument 0 "):
            _lib.load().gif_pack_weight_f32(*pack)
    with recorded_launches(before=OF.checked(None)):  # the default stream: NULL and 0 are the same stream
        assert _lib.load().gif_bias_act_f32(*(BIAS_ACT[:-1] + (0,))) == 0
    assert len(fake.reached) == 4


def test_forbidden_stops_every_launch_and_lets_queries_through(fake):
    from gif_amd import _lib
    with recorded_launches(before=OF.forbidden()) as rec:
        lib = _lib.load()
        assert lib.gif_conv2d_pack_dims(8, 8, ctypes.byref(ctypes.c_int()), ctypes.byref(ctypes.c_int())) == 0
        for name, args in (("gif_bias_act_f32", BIAS_ACT), ("gif_conv2d_fwd_f32", _conv_args(0x77))):
            with pytest.raises(AssertionError, match=name):
                getattr(lib, name)(*args)
    assert fake.reached == ["gif_conv2d_pack_dims"] and [n for n, _ in rec.calls] == ["gif_conv2d_pack_dims"] and rec.streams() == []


def test_the_hook_is_optional(fake):
    from gif_amd import _lib
    with recorded_launches() as rec:
        assert _lib.load().gif_bias_act_f32(*(BIAS_ACT[:2] + (0x2008,) + BIAS_ACT[3:])) == 0
    assert fake.reached == ["gif_bias_act_f32"] and len(rec.calls) == 1 and _lib._lib is fake
