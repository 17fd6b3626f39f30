"""Raw (non-autograd) launches of the gfx950 kernels on torch device tensors.

Conventions: activations are torch tensors of LOGICAL shape [B,C,H,W] whose memory is NHWC
(torch.channels_last); fp32 (the reference dtype) with C % 4 == 0, or float16 (BASELINE config 5: f16 activations,
fp32 everything else) with C % 8 == 0 — the kernel family is chosen by the activation's dtype.  Weights, biases, per-sample
scales, FIR taps and every reduction result are fp32 in both cases.  Everything runs on torch's current HIP stream.
torch is used for device memory and streams only — all arithmetic is in libgif_hip.so.
"""
import ctypes
import functools
import os
import weakref
from typing import NamedTuple, Optional

import torch

from . import _lib

CL = torch.channels_last


def _stream():
    # current stream of the CURRENT device; _device_guard makes that the operands' device
    return torch.cuda.current_stream().cuda_stream


def _device_guard(fn):
    """Run `fn` with the operands' device current (launch + stream + per-device kernel state all follow it) and refuse
    operands that span devices.  One process per GPU never takes the slow branch."""
    @functools.wraps(fn)
    def wrapped(*args, **kw):
        dev = None
        for a in args + tuple(kw.values()):
            if isinstance(a, torch.Tensor) and a.is_cuda:
                if dev is None:
                    dev = a.device
                elif a.device != dev:
                    raise _lib.GifHipError(f"{fn.__name__}: operands on different devices ({dev} and {a.device})")
        if dev is None or dev.index == torch.cuda.current_device():
            return fn(*args, **kw)
        with torch.cuda.device(dev):
            return fn(*args, **kw)
    return wrapped


def _p(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def pad4(c: int) -> int:
    return (c + 3) // 4 * 4


def cpad(c: int, dtype=torch.float32) -> int:
    """Channel count of an activation holding c logical channels: multiple of 4 (fp32: 16-byte lanes) or 8 (f16)."""
    q = 8 if dtype == torch.float16 else 4
    return (c + q - 1) // q * q


def _sfx(dtype) -> str:
    return "_f16" if dtype == torch.float16 else "_f32"


def _fn(name: str, dtype):
    """C entry point of the kernel family matching the activation dtype (gif_<name>_f32 / gif_<name>_f16)."""
    return getattr(_lib.load(), "gif_" + name + _sfx(dtype))


def nhwc(x: torch.Tensor) -> torch.Tensor:
    """fp32 or f16, device-resident, NHWC memory.  Fails loudly on CPU tensors: there is no CPU path."""
    if not x.is_cuda:
        raise _lib.GifHipError("gif_amd kernels need device tensors (no CPU fallback); got a CPU tensor")
    if x.dtype not in (torch.float32, torch.float16):
        raise _lib.GifHipError(f"gif_amd kernels take fp32 or f16 activations; got {x.dtype}")
    if x.dim() != 4:
        raise _lib.GifHipError(f"expected a 4-D activation, got shape {tuple(x.shape)}")
    if x.dtype == torch.float16 and x.shape[1] % 8:
        raise _lib.GifHipError(f"f16 activations need a channel count that is a multiple of 8, got {x.shape[1]}")
    return _aligned(x.contiguous(memory_format=CL))


def _aligned(t: torch.Tensor) -> torch.Tensor:
    """`t` (dense in its own layout) at a 16-byte-aligned address: the kernels read operands as 16-byte lanes.  A dense view that starts
    an odd number of elements into a larger buffer is copied; fresh allocations never are."""
    return t if t.data_ptr() % 16 == 0 else t.clone(memory_format=torch.preserve_format)


def _vec(t: Optional[torch.Tensor], what: str, shape, device) -> Optional[torch.Tensor]:
    """A per-channel ([C]) or per-sample ([B,C]) operand, FIR taps included, as the kernels index it: fp32, on `device`, exactly `shape`
    (the ACTIVATION's channel count: layers._pad_vec), dense and 16-byte aligned (any other strides or offset: a copy of a few hundred
    floats).  Another dtype is refused, not converted: a cast inside a Function would hand autograd a gradient of the wrong dtype."""
    if t is None:
        return None
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_cuda or t.device != device or tuple(t.shape) != tuple(shape):
        got = f"{tuple(t.shape)} {t.dtype} on {t.device}" if isinstance(t, torch.Tensor) else type(t).__name__
        raise _lib.GifHipError(f"{what}: expected an fp32 tensor of shape {tuple(shape)} on {device}, got {got}")
    return _aligned(t.contiguous())


def _weight_check(w, device, what: str):
    """A convolution weight is a 4-D fp32 tensor (any strides) on the activations' device: the packing kernels read it as floats through
    its address and element strides."""
    if (not isinstance(w, torch.Tensor) or w.dim() != 4 or w.dtype != torch.float32 or not w.is_cuda
            or (device is not None and w.device != device)):
        got = f"{tuple(w.shape)} {w.dtype} on {w.device}" if isinstance(w, torch.Tensor) else type(w).__name__
        raise _lib.GifHipError(f"{what}: weight: expected a 4-D fp32 tensor on {device or 'the device'} (no CPU fallback, no conversion), "
                               f"got {got}")


def _same_dtype(a, b, what):
    if a.dtype != b.dtype:
        raise _lib.GifHipError(f"{what}: operands of different dtypes ({a.dtype} and {b.dtype})")


def empty_nhwc(B, C, H, W, device, dtype=torch.float32):
    return torch.empty((B, C, H, W), device=device, dtype=dtype, memory_format=CL)


class ConvSpec(NamedTuple):
    """The underlying FORWARD convolution (see include/gif_hip.h)."""
    KH: int
    KW: int
    stride: int
    pad: int

    def small_hw(self, Hb, Wb):
        return ((Hb + 2 * self.pad - self.KH) // self.stride + 1, (Wb + 2 * self.pad - self.KW) // self.stride + 1)

    def big_hw(self, Hs, Ws):
        return ((Hs - 1) * self.stride + self.KH - 2 * self.pad, (Ws - 1) * self.stride + self.KW - 2 * self.pad)


def _geom(B, Hb, Wb, Cb, Hs, Ws, Cs, spec: ConvSpec):
    return _lib.ConvGeom(B, Hb, Wb, Cb, Hs, Ws, Cs, spec.KH, spec.KW, spec.stride, spec.pad)


# Gradient-producer fusions (gif_conv_epilogue ABI 2).  GIF_FUSE_GRAD=0 keeps every backward on the stand-alone passes (A/B).
FUSE_GRAD = _lib.knob("GIF_FUSE_GRAD", "1") != "0"


class GradFuse:
    """Work a gradient-producing launch does in its epilogue instead of leaving it to stand-alone passes (include/gif_hip.h,
    gif_conv_epilogue ABI 2):
      mask_src (+ slope, gain): the op's output is the gradient w.r.t. a tensor that a fused leaky ReLU produced — multiply by
                                gain * (mask_src > 0 ? 1 : slope), i.e. FusedLeakyReLU's backward (stylegan2_common_layers.py:22-39);
      want_colsum             : .colsum [C] = sum over all pixels of the masked output as computed in fp32, before an f16 store rounds or
                                clamps it (the bias gradient of that layer);
      dot_src                 : .dot [B,C] = sum_hw contraction * dot_src, taken BEFORE out_scale (the modulation gradient of
                                ModulatedConv2d, :311-320).
    After the launch the results are in .colsum / .dot (fp32)."""

    def __init__(self, mask_src=None, mask_slope=1.0, mask_gain=1.0, want_colsum=False, dot_src=None):
        self.mask_src, self.mask_slope, self.mask_gain = mask_src, float(mask_slope), float(mask_gain)
        self.want_colsum, self.dot_src = bool(want_colsum), dot_src
        self.colsum = self.dot = self._ws = None


def dot_fusable(H, W, dtype=torch.float32):
    """The modulation-gradient dot product can ride in a convolution epilogue: every tile (<= 256 rows; Winograd: 256 2x2
    tiles) stays inside one sample.  fp32 and f16 activations alike (the sums are fp32 and taken before the store rounds)."""
    return FUSE_GRAD and dtype in (torch.float32, torch.float16) and (H * W) % 1024 == 0


def _epilogue(in_scale=None, out_scale=None, bias=None, residual=None, act=False, slope=0.2, gain=2 ** 0.5, fuse=None,
              out_bchw=None, dtype=torch.float32, out_f32=False, in_c=None, device=None):
    """The gif_conv_epilogue of a launch that writes an activation of shape out_bchw and element type `dtype` on `device` (in_c: channel
    count of the activation it reads).  in_scale [B,in_c], out_scale [B,C] and bias [C] go through _vec; residual, mask_src and dot_src must
    be NHWC tensors of the output's shape and dtype at a 16-byte-aligned address (ops.nhwc gives one).  The dense copies _vec made stay
    alive on the returned struct until the caller has launched."""
    B, C, H, W = out_bchw
    if device is None:  # (a caller that names none: the device of the first operand there is)
        given = [t for t in (residual, in_scale, out_scale, bias, *((fuse.mask_src, fuse.dot_src) if fuse is not None else ()))
                 if isinstance(t, torch.Tensor)]
        device = given[0].device if given else None
    in_scale = _vec(in_scale, "conv epilogue: in_scale", (B, C if in_c is None else in_c), device)
    out_scale = _vec(out_scale, "conv epilogue: out_scale", (B, C), device)
    bias = _vec(bias, "conv epilogue: bias", (C,), device)
    for t, what, dt in ((residual, "conv epilogue: residual", dtype), (None if fuse is None else fuse.mask_src, "GradFuse.mask_src", dtype),
                        (None if fuse is None else fuse.dot_src, "GradFuse.dot_src", dtype)):
        if t is not None and (tuple(t.shape) != (B, C, H, W) or t.dtype != dt or t.device != device or not t.is_contiguous(memory_format=CL)
                              or t.data_ptr() % 16):
            raise _lib.GifHipError(f"{what}: expected a 16-byte-aligned NHWC {dt} tensor of shape {(B, C, H, W)} on {device}, got "
                                   f"{tuple(t.shape)} {t.dtype} on {t.device}, strides {tuple(t.stride())}")
    e = _lib.ConvEpilogue(_p(in_scale), _p(out_scale), _p(bias), _p(residual), 1 if act else 0, slope, gain)
    e._keep = (in_scale, out_scale, bias)
    e.out_f32 = 1 if out_f32 else 0
    if fuse is not None:
        e.mask_src, e.mask_slope, e.mask_gain = _p(fuse.mask_src), fuse.mask_slope, fuse.mask_gain
        e.dot_src = _p(fuse.dot_src)
        if fuse.mask_src is None and fuse.dot_src is None:
            raise _lib.GifHipError("GradFuse: nothing to fuse (the plain column sum of a gradient is ops.colsum)")
        if fuse.dot_src is not None:
            fuse.dot = torch.empty((B, C), device=device, dtype=torch.float32)
            e.dot = fuse.dot.data_ptr()
        if fuse.want_colsum:
            fuse.colsum = torch.empty((C,), device=device, dtype=torch.float32)
            e.colsum = fuse.colsum.data_ptr()
        if fuse.dot is not None or fuse.colsum is not None:
            fuse._ws = torch.empty((_lib.load().gif_conv_epilogue_ws_floats(B * H * W, C),), device=device, dtype=torch.float32)
            e.red_ws = fuse._ws.data_ptr()
    return e


# Packed / transformed weights are a pure function of (the parameter's current contents, view geometry, layout arguments):
# the same weights are packed 2-3 times per training iteration (D runs three forwards, every backward re-packs for the data
# gradient), so the results are kept until the parameter changes.  An entry is keyed on the identity of the BASE tensor (a
# weak reference proves it is still the same object), its data pointer and in-place version counter (optimisers, copy_,
# load_state_dict and FlatAdam all bump it) and the view geometry — never on an address alone.
WEIGHT_CACHE = _lib.knob("GIF_WEIGHT_CACHE", "1") != "0"
_weight_cache = {}
_WEIGHT_CACHE_MAX = 512


def clear_weight_cache():
    """Forget every packed / transformed weight (call after writing parameters through .data, which bumps no version counter)."""
    _weight_cache.clear()


def _cached_weight_op(w, tag, build):
    if not WEIGHT_CACHE:
        return build()
    base = w._base if w._base is not None else w
    key = (id(base), tag, w.storage_offset(), tuple(w.shape), tuple(w.stride()))
    state = (base.data_ptr(), base._version)
    hit = _weight_cache.get(key)
    if hit is not None and hit[0]() is base and hit[1] == state:
        return hit[2]
    out = build()
    if len(_weight_cache) >= _WEIGHT_CACHE_MAX:
        for k in [k for k, v in _weight_cache.items() if v[0]() is None]:
            del _weight_cache[k]
        if len(_weight_cache) >= _WEIGHT_CACHE_MAX:
            _weight_cache.clear()
    _weight_cache[key] = (weakref.ref(base), state, out)
    return out


X3_TAPDENSE = _lib.knob("GIF_X3_TAPDENSE", "1") != "0"  # tap-dense K order for 3x3 layers with 8..28 contraction channels (A/B)
X3_MIN_CIN = int(_lib.knob("GIF_X3_MIN_CIN", "24"))  # gif_conv2d_x3_eligible: >= 24 (one zero-padded 32-float K chunk)
# The bf16x3 / f16 kernels address their input through 32-bit buffer offsets (conv_igemm.hip): launches the buffer-addressed DMA does
# not take (>= 4 GiB of input) stay on the native fp32 kernel.  conv_plan applies the rule.
X3_MAX_INPUT_BYTES = (1 << 32) - (1 << 26)


def x3_conv(dtype, cin_act: int, src=None, spec=None) -> bool:
    """fp32 conv fwd/dgrad with `cin_act` contraction channels runs on the bf16x3 kernels (mode + eligibility; src and spec are not
    looked at: the size of the input is conv_plan's question)."""
    return dtype == torch.float32 and cin_act >= X3_MIN_CIN and split_mode()


def split_mode() -> bool:
    """The fp32 contractions run on the 16-bit matrix cores (bf16x3, or f16x2 with bf16x3 for the layers f16x2 does not take)."""
    return get_fp32_mfma_mode() in ("bf16x3", "f16x2")


H2_CONV = _lib.knob("GIF_H2_CONV", "1") != "0"    # f16x2 mode: direct fwd / dgrad kernels (A/B knobs per kernel family)
H2_WGRAD = _lib.knob("GIF_H2_WGRAD", "1") != "0"  # f16x2 mode: weight-gradient kernels (direct and Winograd plane GEMMs)
H2_WINO = _lib.knob("GIF_H2_WINO", "1") != "0"    # f16x2 mode: Winograd fwd / dgrad GEMM
H2_GUARD = True  # False: f16x2 launches run without their guarded bf16x3 twin (tests only: shows what the guard protects against)


# f16x2 mode: the tap-dense launches (3x3 layers with 8..28 contraction channels) stay on the bf16x3 tap-dense kernel by default — the f16x2 form
# (gif_conv2d_*_f32h2_tapdense, tests/test_gpu_f16x2.py) measured SLOWER in the step: 200.0 vs 198.5 ms in one call (24 -> 128 at 256^2: 7.9 vs
# 6.7 ms per step; these launches are bound by their per-lane tap gathers, not by the matrix pipe, and the row tracking adds VALU work)
H2_DENSE = _lib.knob("GIF_H2_DENSE", "0") != "0"


def h2_conv(x3: bool, dense: bool) -> bool:
    """This bf16x3-eligible direct launch runs the f16x2 kernels (three f16 products under per-row scales, guarded bf16x3 fallback)."""
    return (bool(x3) or bool(dense)) and (H2_DENSE or not dense) and H2_CONV and get_fp32_mfma_mode() == "f16x2"


def x3_tapdense(dtype, cin_act: int, spec, transposed: bool, epi, cout_act: int = 64) -> bool:
    """3x3 fp32 conv with 8 <= cin_act < 32 contraction channels runs the bf16x3 kernel in its tap-dense K order (include/gif_hip.h:
    the condition-noise convs and the 24 -> C layers; no per-tap padding of K).  Not for strided data gradients (tap subsets per
    output phase) and not for modulated launches.  Measured per shape at 256^2, batch 32 (profiles/r3_conv_shapes.md vs the run
    before the mode existed): 24 -> 128 3.62 vs 4.08 ms per step, 12 -> 24 0.88 vs 1.15 (native kernel); but 8 -> 12 0.76 vs 0.66
    (native) and 24 -> 12 0.79 vs 0.67 (padded bf16x3): with <= 32 output channels the launch is bound by its gathers, which the
    dense order scatters over two pixels per 128-byte row — those two keep their old kernels."""
    if not (X3_TAPDENSE and dtype == torch.float32 and split_mode() and 8 <= cin_act < 32 and cin_act % 4 == 0
            and (spec.KH, spec.KW) == (3, 3) and not (transposed and spec.stride != 1) and epi.get("in_scale") is None):
        return False
    return cin_act >= 12 and (cout_act > 32 or cin_act < X3_MIN_CIN)


def _weight_view(w, rows_are_out: bool, cout_act: int, cin_act: int):
    """(R, C, sr, sc, sky, skx): rows, columns and element strides of the operand a canonical weight view w[O,I,KH,KW] (any strides) packs
    into.  rows_are_out=True: rows = O, cols = I (forward); False: rows = I, cols = O (data gradient)."""
    O, I = w.shape[:2]
    so, si, sky, skx = w.stride()
    R, C, sr, sc = (O, I, so, si) if rows_are_out else (I, O, si, so)
    assert R <= cout_act and C <= cin_act, (R, cout_act, C, cin_act)
    return R, C, sr, sc, sky, skx


def _dims(query, rows: int, cols: int, what: str):
    """(RP, CP) of one of the library's padded-dimension queries."""
    RP, CP = ctypes.c_int(), ctypes.c_int()
    _lib.check(query(rows, cols, ctypes.byref(RP), ctypes.byref(CP)), what)
    return RP.value, CP.value


def _pack(w, rows_are_out, cout_act, cin_act, scale, dtype, form, tapdense, device=None):
    """pack_weight / pack_weight_h2x3: `form` is the family of gif_pack_weight_<form>[_tapdense] ("f32h2x3": both operands of an f16x2 launch).
    device: the activations' (None: a device weight on its own)."""
    _weight_check(w, device, "pack_weight")
    lib = _lib.load()
    KH, KW = w.shape[2:]
    R, C, sr, sc, sky, skx = _weight_view(w, rows_are_out, cout_act, cin_act)

    def build():
        RP, CP = _dims(getattr(lib, "gif_conv2d_pack_dims" + {"f32": "", "f16": "_f16"}.get(form, "_x3")), cout_act, cin_act, "pack_dims")
        T, CPk = (lib.gif_conv2d_x3_tapdense_steps(cin_act, KH, KW), 32) if tapdense else (KH * KW, CP)
        geo = (R, C, cin_act, KH, KW, RP) if tapdense else (R, C, KH, KW, RP, CP)
        shapes = []
        if "h2" in form:  # [row exponents + flag][tap][2][RP][CP] f16, an opaque byte buffer
            nbytes = lib.gif_pack_weight_f32h2_tapdense_bytes(cin_act, KH, KW, RP) if tapdense else lib.gif_pack_weight_f32h2_bytes(KH, KW, RP, CP)
            shapes.append(((nbytes,), torch.uint8))
        if "x3" in form:
            shapes.append(((T, 3, RP, CPk), torch.bfloat16))
        wp = [torch.empty(s, device=w.device, dtype=t) for s, t in shapes or [((T, RP, CP), dtype)]]
        name = "pack_weight_" + form + ("_tapdense" if tapdense else "")
        _lib.check(getattr(lib, "gif_" + name)(w.data_ptr(), *[p.data_ptr() for p in wp], *geo, sr, sc, sky, skx, float(scale), _stream()), name)
        return tuple(wp) if form == "f32h2x3" else wp[0]

    return _cached_weight_op(w, ("pack", rows_are_out, cout_act, cin_act, float(scale), dtype, form, bool(tapdense)), build)


def pack_weight(w: torch.Tensor, rows_are_out: bool, cout_act: int, cin_act: int, scale: float = 1.0, dtype=torch.float32, x3=False,
                tapdense=False, h2=False, device=None):
    """Pack a canonical forward-conv weight view w[O,I,KH,KW] (any strides) into [T][RP][CP] of `dtype` (fp32 or f16), or
    (x3=True) into the pre-split bf16x3 operand [T][3][RP][CP] (bf16) of the gif_conv2d_*_f32x3 entry points, (tapdense=True) into that
    operand in the tap-dense K order [steps][3][RP][32], or (h2=True) into the f16x2 operand.

    rows_are_out=True : rows = O, cols = I (operand of gif_conv2d_fwd)
    rows_are_out=False: rows = I, cols = O (operand of gif_conv2d_bwd_data)
    cout_act / cin_act are the channel counts of the op's output / input ACTIVATIONS (>= canonical counts).
    """
    form = "f32x3" if tapdense else "f32h2" if h2 else "f32x3" if x3 else "f16" if dtype == torch.float16 else "f32"
    return _pack(w, rows_are_out, cout_act, cin_act, scale, dtype, form, tapdense, device)


def pack_weight_h2x3(w: torch.Tensor, rows_are_out: bool, cout_act: int, cin_act: int, scale: float = 1.0, tapdense=False, device=None):
    """(wp2, wp3): the f16x2 packing and the bf16x3 packing (the guarded fallback's operand) of the same weight view, ONE launch."""
    return _pack(w, rows_are_out, cout_act, cin_act, scale, torch.float32, "f32h2x3", tapdense, device)


# Winograd F(2x2,3x3) dispatch for stride-1 / pad-1 3x3 convs (conv_winograd.hip).  GIF_WINOGRAD=0 forces the direct
# implicit-GEMM kernels; below GIF_WINOGRAD_MIN_TILES 2x2 tiles the launch cannot fill the chip and the direct path wins.
WINOGRAD = _lib.knob("GIF_WINOGRAD", "1") != "0"
WINOGRAD_MIN_TILES = int(_lib.knob("GIF_WINOGRAD_MIN_TILES", "8192"))
WINOGRAD_WGRAD = _lib.knob("GIF_WINOGRAD_WGRAD", "1") != "0"
WINOGRAD_X3 = _lib.knob("GIF_WINO_X3", "1") != "0"  # bf16x3 mode: Winograd fwd/dgrad GEMMs on the bf16x3 kernel too
WINOGRAD_WGRAD_MIN_TILES = int(_lib.knob("GIF_WINOGRAD_WGRAD_MIN_TILES", "2048"))  # split-K fills the chip earlier
# Per-channel-count rule (round 6, profiles/r6_dispatch_ab.md): the smaller of the two channel counts must reach these for the
# Winograd route — forward / data gradient and weight gradient separately (the weight gradient re-uses the forward's V when both
# take the route, otherwise it runs its own input transform).  Under f16x2 the direct kernels beat the Winograd route on the
# 128-channel layers (one A/B call, alternating arms, ms per step: 184.8 / 184.4 with 0 / 0; 187.0 / 186.0 with 256 / 0; 186.4 / 185.4
# with 0 / 256; 182.5 / 182.8 with 256 / 256; 188.3 with 512 / 512; 204.3 without Winograd) — the two halves only pay together: a
# direct forward leaves the weight gradient without a V to re-use.
# (The rule belongs to the f16x2 mode: with six bf16 products or the fp32-input MFMA per product the direct kernels are 1.4-2.3 x slower than
# the Winograd route at 128 channels as well — those modes keep 0 / 0.  None = by mode; an int (tests, GIF_WINOGRAD_MIN_C /
# GIF_WINOGRAD_WGRAD_MIN_C under GIF_EXPERIMENTAL=1) overrides.)
_k = _lib.knob("GIF_WINOGRAD_MIN_C", "")
WINOGRAD_MIN_C = int(_k) if _k != "" else None
_k = _lib.knob("GIF_WINOGRAD_WGRAD_MIN_C", "")
WINOGRAD_WGRAD_MIN_C = int(_k) if _k != "" else None
del _k
WINOGRAD_MIN_C_F16X2 = 256


def _winograd_min_c(override):
    if override is not None:
        return override
    return WINOGRAD_MIN_C_F16X2 if get_fp32_mfma_mode() == "f16x2" else 0


_winograd_calls = 0


def prof_winograd_calls():
    """Number of Winograd launches so far (tests use it to prove the path under test actually ran)."""
    return _winograd_calls


def winograd_eligible(spec: ConvSpec, B, H, W, cin_act, cout_act=64, min_tiles=None, dtype=torch.float32, min_c=None):
    # cout < 48 wastes over a quarter of the GEMM's 64-wide N tile; the direct 256x32 kernel is faster there (measured)
    min_tiles = WINOGRAD_MIN_TILES if min_tiles is None else min_tiles
    min_c = _winograd_min_c(WINOGRAD_MIN_C) if min_c is None else min_c
    return (WINOGRAD and dtype == torch.float32 and tuple(spec) == (3, 3, 1, 1) and H % 2 == 0 and W % 2 == 0 and cin_act >= 32 and cout_act >= 48
            and min(cin_act, cout_act) >= min_c and B * (H // 2) * (W // 2) >= min_tiles)


class ConvPlan(NamedTuple):
    """What one convolution runs, decided before the library is called (conv_plan)."""
    route: str   # "winograd" | "direct"
    mode: str    # "native" | "bf16x3" | "f16x2" | "f16": the entry-point family of the library call (FAMILY)
    dense: bool  # direct route only: the tap-dense entry point


def _fp32_mode(x3, h2) -> str:
    """Contraction mode of an fp32 launch that has a bf16x3 form (x3) and an f16x2 form (h2: its A/B knob): f16x2, else split, else native."""
    if not (x3 and split_mode()):
        return "native"
    return "f16x2" if h2 and get_fp32_mfma_mode() == "f16x2" else "bf16x3"


def winograd_mode(op: str, cout_act: int) -> str:
    """Contraction mode of the Winograd route's GEMMs (op "wgrad": the plane GEMMs of the weight gradient; else fwd / dgrad).
    fwd / dgrad: the split GEMM's 128-wide N tile wants full tiles; other channel counts stay on the native GEMM (GIF_WINO_X3=0: A/B)."""
    if op == "wgrad":
        return _fp32_mode(True, H2_WGRAD)
    return _fp32_mode(WINOGRAD_X3 and cout_act % 128 == 0, H2_WINO)


def conv_plan(op: str, dtype, B, spec: ConvSpec, big_hw, small_hw, cin_act: int, cout_act: int, epi=None, in_bytes: int = 0) -> ConvPlan:
    """Route, contraction mode and K order of one convolution: everything conv_fwd, conv_bwd_data and conv_wgrad decide before they call the
    library.  Pure: reads its arguments, the knobs above and get_fp32_mfma_mode(); tests/golden/conv_plan_table.txt records its answers.

    op: "fwd" | "dgrad" | "wgrad".  big_hw / small_hw: the two sides of the forward convolution, (H, W) tuples.  cin_act / cout_act: contraction and output
    channel counts of THIS op as the activations carry them (fwd: Cb, Cs; dgrad: Cs, Cb; wgrad: Cb, Cs).  epi: the epilogue arguments
    (x3_tapdense looks for in_scale).  in_bytes: size of the fwd / dgrad input; past X3_MAX_INPUT_BYTES a direct launch stays native."""
    wgrad, f16 = op == "wgrad", dtype == torch.float16
    # the weight gradient has thresholds of its own (None: winograd_eligible's); the two sides of a forward 3x3 / stride 1 / pad 1 are one size
    min_tiles, min_c = (min(WINOGRAD_MIN_TILES, WINOGRAD_WGRAD_MIN_TILES), _winograd_min_c(WINOGRAD_WGRAD_MIN_C)) if wgrad else (None, None)
    if (big_hw == small_hw and (not wgrad or (WINOGRAD_WGRAD and cin_act >= 64 and cout_act >= 64))
            and winograd_eligible(spec, B, *small_hw, cin_act, cout_act, min_tiles, dtype, min_c)):
        return ConvPlan("winograd", winograd_mode(op, cout_act), False)
    if wgrad:
        return ConvPlan("direct", "f16" if f16 else _fp32_mode(True, H2_WGRAD), False)
    x3 = x3_conv(dtype, cin_act)
    dense = x3_tapdense(dtype, cin_act, spec, op == "dgrad", {} if epi is None else epi, cout_act)
    if in_bytes > X3_MAX_INPUT_BYTES:
        x3 = dense = False
    return ConvPlan("direct", "f16x2" if h2_conv(x3, dense) else "bf16x3" if (x3 or dense) else "f16" if f16 else "native", bool(dense))


# Entry-point family of each contraction mode: gif_<op>_<family>[_tapdense]
FAMILY = {"native": "f32", "bf16x3": "f32x3", "f16x2": "f32h2", "f16": "f16"}


def _call(op: str, mode: str, *args, dense=False):
    """Call gif_<op>_<family of mode>[_tapdense](*args) and check its status."""
    name = f"{op}_{FAMILY[mode]}" + ("_tapdense" if dense else "")
    _lib.check(getattr(_lib.load(), "gif_" + name)(*args), name)


def _weight_ptrs(wp):
    """Pointer arguments of packed weights: one operand, or the f16x2 pair (the guarded bf16x3 twin's operand second: None with H2_GUARD off)."""
    if isinstance(wp, torch.Tensor):
        return (wp.data_ptr(),)
    return (wp[0].data_ptr(), wp[1].data_ptr() if H2_GUARD else None)


def conv3x3_winograd(x, w, rows_are_out: bool, cout_act: int, wscale=1.0, keep_v=False, **epi):
    """act(out_scale * conv3x3_s1_p1(in_scale * x, w) + residual + bias) via Winograd F(2x2,3x3).

    rows_are_out=True : forward conv with w[O,I,3,3];  False: its data gradient (taps rotated, channels swapped).
    keep_v=True returns (y, V): V = the transformed (in_scale * x), reusable by conv3x3_winograd_wgrad(big=x)."""
    global _winograd_calls
    _winograd_calls += 1
    lib = _lib.load()
    x = nhwc(x)
    _weight_check(w, x.device, "conv3x3_winograd")
    B, C, H, W = x.shape
    R, Cc, sr, sc, sky, skx = _weight_view(w, rows_are_out, cout_act, C)
    mode = winograd_mode("fwd", cout_act)
    e = _epilogue(out_bchw=(B, cout_act, H, W), in_c=C, device=x.device, **epi)  # (before anything is launched or cached: it refuses)

    def build():  # f16x2: its transform and the bf16x3 transform (the operand of the GEMM's guarded bf16x3 twin) in one launch
        RP, CP = _dims(lib.gif_winograd_pack_dims if mode == "native" else lib.gif_winograd_pack_dims_x3, cout_act, C, "winograd_pack_dims")
        U = [torch.empty((lib.gif_winograd_weight_f32h2_bytes(RP, CP),), device=x.device, dtype=torch.uint8)] if mode == "f16x2" else []
        U.append(torch.empty((16, RP, CP), device=x.device, dtype=torch.float32) if mode == "native" else
                 torch.empty((16, 3, RP, CP), device=x.device, dtype=torch.bfloat16))
        _call("winograd_weight", mode, w.data_ptr(), *[u.data_ptr() for u in U], R, Cc, RP, CP, sr, sc, sky, skx, 0 if rows_are_out else 1,
              float(wscale), _stream())
        return tuple(U) if mode == "f16x2" else U[0]

    U = _cached_weight_op(w, ("wino", rows_are_out, cout_act, C, float(wscale), mode), build)
    V = torch.empty((lib.gif_winograd_workspace_floats(B, H, W, C),), device=x.device, dtype=torch.float32)
    out = empty_nhwc(B, cout_act, H, W, x.device)
    _call("conv3x3_winograd", mode, x.data_ptr(), *_weight_ptrs(U), out.data_ptr(), V.data_ptr(), B, H, W, C, cout_act, ctypes.byref(e), _stream())
    return (out, V) if keep_v else out


def _epi_check(x, epi):
    r = epi.get("residual")
    if r is not None:
        _same_dtype(x, r, "conv epilogue residual")


def _conv_direct(plan: ConvPlan, op: str, src, w, out_bchw, g, wscale, epi):
    """The direct-kernel launch of conv_fwd (op "conv2d_fwd") / conv_bwd_data ("conv2d_bwd_data") as `plan` says: weights packed for the
    plan's mode (an f16x2 launch takes the bf16x3 packing for its guarded fallback too), then the one entry point."""
    fwd, dt = op == "conv2d_fwd", src.dtype
    e = _epilogue(out_bchw=out_bchw, dtype=dt, in_c=src.shape[1], device=src.device, **epi)  # (before anything is launched or cached: it refuses)
    if plan.mode == "f16x2":
        wp = pack_weight_h2x3(w, fwd, out_bchw[1], src.shape[1], wscale, tapdense=plan.dense, device=src.device)
    else:
        wp = pack_weight(w, fwd, out_bchw[1], src.shape[1], wscale, dt, x3=plan.mode == "bf16x3", tapdense=plan.dense, device=src.device)
    # out_f32 (f16 activations only): fp32 result, e.g. the RGB image of ToRGB
    out = empty_nhwc(*out_bchw, src.device, torch.float32 if epi.get("out_f32") else dt)
    _call(op, plan.mode, src.data_ptr(), *_weight_ptrs(wp), out.data_ptr(), ctypes.byref(g), ctypes.byref(e), _stream(), dense=plan.dense)
    return out


def conv_fwd(big, w, spec: ConvSpec, wscale=1.0, keep_v=False, **epi):
    """small = conv2d(big, w[O,I,KH,KW]) ; returns [B, cpad(O), Hs, Ws] in big's dtype.

    keep_v=True returns (small, V) where V is the Winograd-transformed (in_scale * big) if that path ran, else None;
    pass it to conv_wgrad(big_v=V) for the weight gradient of the same (big, in_scale)."""
    big = nhwc(big)
    _weight_check(w, big.device, "conv_fwd")
    dt = big.dtype
    B, Cb, Hb, Wb = big.shape
    Cs = cpad(w.shape[0], dt)
    Hs, Ws = spec.small_hw(Hb, Wb)
    _epi_check(big, epi)
    if dt != torch.float16:
        epi.pop("out_f32", None)  # (fp32 activations: the result is fp32 anyway)
    plan = conv_plan("fwd", dt, B, spec, (Hb, Wb), (Hs, Ws), Cb, Cs, epi, big.numel() * big.element_size())
    if plan.route == "winograd":
        return conv3x3_winograd(big, w, True, Cs, wscale, keep_v=keep_v, **epi)
    out = _conv_direct(plan, "conv2d_fwd", big, w, (B, Cs, Hs, Ws), _geom(B, Hb, Wb, Cb, Hs, Ws, Cs, spec), wscale, epi)
    return (out, None) if keep_v else out


def conv_bwd_data(small, w, spec: ConvSpec, big_hw, wscale=1.0, **epi):
    """big = conv_transpose2d(small, w[O,I,KH,KW]) ; returns [B, cpad(I), Hb, Wb] in small's dtype."""
    small = nhwc(small)
    _weight_check(w, small.device, "conv_bwd_data")
    dt = small.dtype
    B, Cs, Hs, Ws = small.shape
    Cb = cpad(w.shape[1], dt)
    Hb, Wb = big_hw
    _epi_check(small, epi)
    plan = conv_plan("dgrad", dt, B, spec, (Hb, Wb), (Hs, Ws), Cs, Cb, epi, small.numel() * small.element_size())
    if plan.route == "winograd":
        return conv3x3_winograd(small, w, False, Cb, wscale, **epi)
    return _conv_direct(plan, "conv2d_bwd_data", small, w, (B, Cb, Hb, Wb), _geom(B, Hb, Wb, Cb, Hs, Ws, Cs, spec), wscale, epi)


def pad32(c: int) -> int:
    return (c + 31) // 32 * 32


def conv3x3_winograd_wgrad(small, big, O, I, wscale=1.0, small_scale=None, big_scale=None, big_v=None):
    """dW[O,I,3,3] of the stride-1 / pad-1 3x3 conv via Winograd F(3x3,2x2) (transforms + 16 plane GEMMs + unpack).
    big_v: the V kept from the forward pass over the same (big, big_scale) — skips the input transform."""
    global _winograd_calls
    _winograd_calls += 1
    lib = _lib.load()
    small, big = nhwc(small), nhwc(big)
    B, Cs, H, W = small.shape
    Cb = big.shape[1]
    assert big.shape == (B, Cb, H, W) and O <= Cs and I <= Cb
    small_scale = _vec(small_scale, "conv3x3_winograd_wgrad: small_scale", (B, Cs), small.device)
    big_scale = _vec(big_scale, "conv3x3_winograd_wgrad: big_scale", (B, Cb), small.device)
    RP, CP = _dims(lib.gif_conv2d_wgrad_dims, pad32(Cs), pad32(Cb), "wgrad_dims")
    nsplit = lib.gif_conv3x3_winograd_wgrad_splits(B, H, W, Cs, Cb)
    dev = small.device
    nv = lib.gif_winograd_workspace_floats(B, H, W, Cb)
    if big_v is not None and big_v.numel() != nv:
        raise _lib.GifHipError(f"conv3x3_winograd_wgrad: cached V has {big_v.numel()} floats, expected {nv}")
    V = big_v if big_v is not None else torch.empty((nv,), device=dev, dtype=torch.float32)
    Mg = torch.empty((lib.gif_winograd_workspace_floats(B, H, W, Cs),), device=dev, dtype=torch.float32)
    ws = torch.empty((nsplit, 16, RP, CP), device=dev, dtype=torch.float32)
    _call("conv3x3_winograd_wgrad", winograd_mode("wgrad", Cs), None if big_v is not None else big.data_ptr(), small.data_ptr(), V.data_ptr(),
          Mg.data_ptr(), ws.data_ptr(), _p(small_scale), _p(big_scale), B, H, W, Cs, Cb, nsplit, _stream())
    dw = torch.empty((O, I, 3, 3), device=dev, dtype=torch.float32)
    so, si, sky, skx = dw.stride()
    _lib.check(lib.gif_winograd_unpack_wgrad_f32(ws.data_ptr(), dw.data_ptr(), nsplit, O, I, RP, CP, so, si, sky, skx, float(wscale),
                                                 _stream()), "winograd_unpack_wgrad")
    return dw


def conv_wgrad(small, big, spec: ConvSpec, O, I, wscale=1.0, small_scale=None, big_scale=None, big_v=None):
    """dW[O,I,KH,KW] = wscale * sum small (x) big  (contiguous canonical layout, fp32 for fp32 AND f16 operands).
    big_v: optional Winograd V of (big_scale * big) kept from conv_fwd(keep_v=True)."""
    lib = _lib.load()
    small, big = nhwc(small), nhwc(big)
    _same_dtype(small, big, "conv_wgrad")
    B, Cs, Hs, Ws = small.shape
    _, Cb, Hb, Wb = big.shape
    assert O <= Cs and I <= Cb
    small_scale = _vec(small_scale, "conv_wgrad: small_scale", (B, Cs), small.device)
    big_scale = _vec(big_scale, "conv_wgrad: big_scale", (B, Cb), small.device)
    plan = conv_plan("wgrad", small.dtype, B, spec, (Hb, Wb), (Hs, Ws), Cb, Cs)
    if plan.route == "winograd":
        return conv3x3_winograd_wgrad(small, big, O, I, wscale, small_scale, big_scale, big_v)
    g = _geom(B, Hb, Wb, Cb, Hs, Ws, Cs, spec)
    f16 = "_f16" if plan.mode == "f16" else ""
    RP, CP = _dims(getattr(lib, "gif_conv2d_wgrad_dims" + f16), Cs, Cb, "wgrad_dims")
    nsplit = getattr(lib, "gif_conv2d_wgrad_splits" + f16)(ctypes.byref(g))
    ws = torch.empty((nsplit, spec.KH * spec.KW, RP, CP), device=small.device, dtype=torch.float32)
    _call("conv2d_wgrad", plan.mode, small.data_ptr(), big.data_ptr(), ws.data_ptr(), _p(small_scale), _p(big_scale), ctypes.byref(g), nsplit,
          _stream())
    dw = torch.empty((O, I, spec.KH, spec.KW), device=small.device, dtype=torch.float32)
    so, si, sky, skx = dw.stride()
    _lib.check(lib.gif_unpack_wgrad_f32(ws.data_ptr(), dw.data_ptr(), nsplit, O, I, spec.KH, spec.KW, RP, CP, so, si, sky, skx, float(wscale),
                                        _stream()), "unpack_wgrad")
    return dw


def fir_fusable(C, up, down, kshape, dtype=torch.float32):
    """The blur kernels (4x4 FIR, up = down = 1) take the mask / column-sum fusions for power-of-two channel counts."""
    return (FUSE_GRAD and dtype in (torch.float32, torch.float16) and up == 1 and down == 1 and tuple(kshape) == (4, 4)
            and C & (C - 1) == 0 and C <= 1024)


def upfirdn2d(x, k, up, down, pad0, out_hw, flip=True, bias=None, residual=None, act=False, slope=0.2, gain=2 ** 0.5, fuse=None):
    x = nhwc(x)
    B, C, Hi, Wi = x.shape
    Ho, Wo = out_hw
    if not isinstance(k, torch.Tensor) or k.dim() != 2:
        raise _lib.GifHipError(f"upfirdn2d: k: expected 2-D FIR taps, got {tuple(k.shape) if isinstance(k, torch.Tensor) else type(k).__name__}")
    KH, KW = k.shape
    k = _vec(k, "upfirdn2d: k (FIR taps)", (KH, KW), x.device)
    if residual is not None:
        residual = nhwc(residual)  # (any layout a caller has: an NCHW tensor of the right shape is not NHWC memory)
        _same_dtype(x, residual, "upfirdn2d residual")
    e = _epilogue(bias=bias, residual=residual, act=act, slope=slope, gain=gain, fuse=fuse, out_bchw=(B, C, Ho, Wo), dtype=x.dtype,
                  device=x.device)
    y = empty_nhwc(B, C, Ho, Wo, x.device, x.dtype)
    _lib.check(_fn("upfirdn2d", x.dtype)(x.data_ptr(), k.data_ptr(), y.data_ptr(), B, Hi, Wi, C, Ho, Wo, up, down, pad0, pad0,
                                         KH, KW, 1 if flip else 0, ctypes.byref(e), _stream()), "upfirdn2d")
    return y


def bias_act(x, bias=None, residual=None, slope=0.2, gain=2 ** 0.5):
    x = nhwc(x)
    B, C, H, W = x.shape
    if residual is not None:
        residual = nhwc(residual)
        if residual.shape != x.shape or residual.device != x.device:
            raise _lib.GifHipError(f"bias_act: residual: expected shape {tuple(x.shape)} on {x.device}, got {tuple(residual.shape)} on {residual.device}")
        _same_dtype(x, residual, "bias_act residual")
    bias = _vec(bias, "bias_act: bias", (C,), x.device)
    y = empty_nhwc(B, C, H, W, x.device, x.dtype)
    _lib.check(_fn("bias_act", x.dtype)(x.data_ptr(), _p(bias), _p(residual), y.data_ptr(), B * H * W, C, slope, gain,
                                        _stream()), "bias_act")
    return y


def bias_act_bwd(gy, y, want_gbias, slope=0.2, gain=2 ** 0.5):
    lib = _lib.load()
    gy, y = nhwc(gy), nhwc(y)
    _same_dtype(gy, y, "bias_act_bwd")
    B, C, H, W = y.shape
    npix = B * H * W
    gx = empty_nhwc(B, C, H, W, y.device, y.dtype)
    gbias = partial = None
    if npix == 0:  # nothing to launch: the bias gradient of an empty batch is zero
        return gx, (torch.zeros((C,), device=y.device, dtype=torch.float32) if want_gbias else None)
    if want_gbias:
        gbias = torch.empty((C,), device=y.device, dtype=torch.float32)
        partial = torch.empty((lib.gif_colsum_partial_floats(npix, C),), device=y.device, dtype=torch.float32)
    _lib.check(_fn("bias_act_bwd", y.dtype)(gy.data_ptr(), y.data_ptr(), gx.data_ptr(), _p(gbias), _p(partial), npix, C, slope,
                                            gain, _stream()), "bias_act_bwd")
    return gx, gbias


def colsum(x):
    """[B,C,H,W] (NHWC) -> [C] sum over B,H,W (fp32)."""
    lib = _lib.load()
    x = nhwc(x)
    B, C, H, W = x.shape
    npix = B * H * W
    if npix == 0:  # nothing to launch: a sum over no rows
        return torch.zeros((C,), device=x.device, dtype=torch.float32)
    out = torch.empty((C,), device=x.device, dtype=torch.float32)
    partial = torch.empty((lib.gif_colsum_partial_floats(npix, C),), device=x.device, dtype=torch.float32)
    _lib.check(_fn("colsum", x.dtype)(x.data_ptr(), out.data_ptr(), partial.data_ptr(), npix, C, _stream()), "colsum")
    return out


def mul_reduce(a, b, scale=None, want_scaled=False):
    """out[b,c] = sum_hw a*b (fp32) ; optionally scaled = scale[b,c]*a (activation dtype)."""
    lib = _lib.load()
    a, b = nhwc(a), nhwc(b)
    _same_dtype(a, b, "mul_reduce")
    B, C, H, W = a.shape
    assert b.shape == a.shape
    if B * H * W == 0:  # nothing to launch
        return torch.zeros((B, C), device=a.device, dtype=torch.float32), (empty_nhwc(B, C, H, W, a.device, a.dtype) if want_scaled else None)
    nchunk = lib.gif_mul_reduce_chunks(H * W)
    out = torch.empty((B, C), device=a.device, dtype=torch.float32)
    partial = torch.empty((B * nchunk * C,), device=a.device, dtype=torch.float32)
    scaled = empty_nhwc(B, C, H, W, a.device, a.dtype) if want_scaled else None
    scale = _vec(scale, "mul_reduce: scale", (B, C), a.device)
    _lib.check(_fn("mul_reduce", a.dtype)(a.data_ptr(), b.data_ptr(), _p(scale), _p(scaled), out.data_ptr(), partial.data_ptr(),
                                          B, H * W, C, _stream()), "mul_reduce")
    return out, scaled


def bilinear_down(x, S, backward_to=None):
    """Forward: x [B,C,R,R] -> [B,C,S,S].  backward_to=R: x is the gradient of a level, returns the gradient [B,C,R,R]."""
    lib = _lib.load()
    x = nhwc(x)
    if x.dtype != torch.float32:
        raise _lib.GifHipError("bilinear_down is fp32 only (the condition pyramid is built in fp32 and cast per level)")
    B, C = x.shape[:2]
    if backward_to is None:
        R = x.shape[2]
        y = empty_nhwc(B, C, S, S, x.device)
        _lib.check(lib.gif_bilinear_down_f32(x.data_ptr(), y.data_ptr(), B, R, S, C, 0, _stream()), "bilinear_down")
    else:
        R = backward_to
        y = empty_nhwc(B, C, R, R, x.device)
        _lib.check(lib.gif_bilinear_down_f32(x.data_ptr(), y.data_ptr(), B, R, S, C, 1, _stream()), "bilinear_down_bwd")
    return y


def _i64x4(t):
    return (ctypes.c_int64 * 4)(*t.stride())


@_device_guard
def pack_nhwc(src0, off0, src1, off1, cp, dtype):
    """[B,cp,H,W] NHWC tensor of `dtype` (fp32 / f16) with channels [off0, off0 + C0) = src0, [off1, off1 + C1) = src1 (or None),
    zeros elsewhere — torch.cat + channel padding + conversion + layout change in one pass (include/gif_hip.h).  Sources: fp32,
    logical [B,C,H,W], any strides."""
    lib = _lib.load()
    for t in (src0, src1):
        if t is not None and (not t.is_cuda or t.dtype != torch.float32 or t.dim() != 4):
            raise _lib.GifHipError("pack_nhwc needs 4-D fp32 device tensors (no CPU fallback)")
    B, C0, H, W = src0.shape
    if src1 is not None and (src1.shape[0], src1.shape[2], src1.shape[3]) != (B, H, W):
        raise _lib.GifHipError(f"pack_nhwc: sources disagree: {tuple(src0.shape)} vs {tuple(src1.shape)}")
    out = empty_nhwc(B, cp, H, W, src0.device, dtype)
    _lib.check(_fn("pack_nhwc", dtype)(src0.data_ptr(), C0, off0, _i64x4(src0), _p(src1), 0 if src1 is None else src1.shape[1], off1,
                                       None if src1 is None else _i64x4(src1), out.data_ptr(), B, H, W, cp, _stream()), "pack_nhwc")
    return out


@_device_guard
def unpack_nhwc(g, c_off, C):
    """Adjoint of pack_nhwc w.r.t. one source: channels [c_off, c_off + C) of the NHWC tensor g -> fp32 [B,C,H,W] (channels_last)."""
    g = nhwc(g)
    B, cp, H, W = g.shape
    out = torch.empty((B, C, H, W), device=g.device, dtype=torch.float32, memory_format=CL)
    _lib.check(_fn("unpack_nhwc", g.dtype)(g.data_ptr(), out.data_ptr(), B, H, W, cp, c_off, C, _stream()), "unpack_nhwc")
    return out


def act_inv_mul_reduce(g, y, residual, bias, slope, gain):
    """out[b,c] = sum_hw g * (act^-1(y) - residual - bias[c])  (see gif_hip.h)."""
    lib = _lib.load()
    g, y = nhwc(g), nhwc(y)
    _same_dtype(g, y, "act_inv_mul_reduce")
    B, C, H, W = y.shape
    bias = _vec(bias, "act_inv_mul_reduce: bias", (C,), y.device)
    if residual is not None:
        residual = nhwc(residual)
        if residual.shape != y.shape or residual.device != y.device:
            raise _lib.GifHipError(f"act_inv_mul_reduce: residual: expected shape {tuple(y.shape)} on {y.device}, got {tuple(residual.shape)}")
        _same_dtype(y, residual, "act_inv_mul_reduce residual")
    if B * H * W == 0:  # nothing to launch
        return torch.zeros((B, C), device=y.device, dtype=torch.float32)
    nchunk = lib.gif_mul_reduce_chunks(H * W)
    out = torch.empty((B, C), device=y.device, dtype=torch.float32)
    partial = torch.empty((B * nchunk * C,), device=y.device, dtype=torch.float32)
    _lib.check(_fn("act_inv_mul_reduce", y.dtype)(g.data_ptr(), y.data_ptr(), _p(residual), _p(bias), out.data_ptr(),
                                                  partial.data_ptr(), B, H * W, C, slope, gain, _stream()),
               "act_inv_mul_reduce")
    return out


def mbstd_fwd(x, G, Cy):
    lib = _lib.load()
    x = nhwc(x)
    if x.dtype != torch.float32:
        raise _lib.GifHipError("minibatch stddev is fp32 only (functional.minibatch_stddev casts the 4x4 tensor)")
    B, C, H, W = x.shape
    y = empty_nhwc(B, Cy, H, W, x.device)
    stat = torch.empty((B // G,), device=x.device, dtype=torch.float32)
    _lib.check(lib.gif_mbstd_fwd_f32(x.data_ptr(), y.data_ptr(), stat.data_ptr(), B, H, W, C, Cy, G, _stream()), "mbstd_fwd")
    return y, stat


def mbstd_bwd(x, gy, G):
    lib = _lib.load()
    x, gy = nhwc(x), nhwc(gy)
    B, C, H, W = x.shape
    Cy = gy.shape[1]
    gx = empty_nhwc(B, C, H, W, x.device)
    _lib.check(lib.gif_mbstd_bwd_f32(x.data_ptr(), gy.data_ptr(), gx.data_ptr(), B, H, W, C, Cy, G, _stream()), "mbstd_bwd")
    return gx


def sqnorm_per_sample(g):
    lib = _lib.load()
    if not g.is_cuda or g.dtype != torch.float32:
        raise _lib.GifHipError("sqnorm_per_sample needs an fp32 device tensor")
    g = g if g.is_contiguous() or g.is_contiguous(memory_format=CL) else g.contiguous()
    B = g.shape[0]
    out = torch.empty((B,), device=g.device, dtype=torch.float32)
    _lib.check(lib.gif_sqnorm_per_sample_f32(g.data_ptr(), out.data_ptr(), B, g.numel() // max(B, 1), _stream()), "sqnorm")
    return out


# One zero-initialised rasteriser workspace per (device, stream, problem size), kept across calls: the tile kernel hands the
# counters back zeroed, so the per-call memset node is switched off for exactly these pointers
# (gif_rasterize_assume_clean_workspace(ws, 1)).  A failed call drops its entry (the counters may be dirty).
_raster_ws = {}
_RASTER_WS_MAX = 8


def _raster_ws_drop(lib, key):
    ws = _raster_ws.pop(key, None)
    if ws is not None:
        lib.gif_rasterize_assume_clean_workspace(ws.data_ptr(), 0)  # before the memory can be handed to somebody else


def _raster_workspace(lib, dev, B, F, h, w):
    key = (dev.index, torch.cuda.current_stream().cuda_stream, B, F, h, w)
    ws = _raster_ws.get(key)
    if ws is None:
        if len(_raster_ws) >= _RASTER_WS_MAX:
            _raster_ws_drop(lib, next(iter(_raster_ws)))
        # (the byte count is a multiple of 4, not of 8: B * tiles * F odd leaves half a word, which must not be cut off)
        ws = torch.zeros((max((lib.gif_rasterize_workspace_bytes(B, F, h, w) + 7) // 8, 1),), device=dev, dtype=torch.int64)
        _raster_ws[key] = ws
        _lib.check(lib.gif_rasterize_assume_clean_workspace(ws.data_ptr(), 1), "rasterize_assume_clean_workspace")
    return key, ws


def rasterize(face_vertices, depth, tri, out3, h, w, face_colors=None):
    """float32 or float64 buffers (all floating tensors of one dtype, like the reference's AT_DISPATCH_FLOATING_TYPES)."""
    lib = _lib.load()
    B, F = face_vertices.shape[:2]
    f64 = face_vertices.dtype == torch.float64
    key, ws = _raster_workspace(lib, face_vertices.device, B, F, h, w)
    plain, colors = (lib.gif_rasterize_f64, lib.gif_rasterize_colors_f64) if f64 else (lib.gif_rasterize_f32,
                                                                                        lib.gif_rasterize_colors_f32)
    if face_colors is None:
        rc = plain(face_vertices.data_ptr(), depth.data_ptr(), tri.data_ptr(), out3.data_ptr(), B, F, h, w, ws.data_ptr(),
                   _stream())
    else:
        rc = colors(face_vertices.data_ptr(), face_colors.data_ptr(), depth.data_ptr(), tri.data_ptr(), out3.data_ptr(), B, F,
                    h, w, ws.data_ptr(), _stream())
    if rc != 0:
        _raster_ws_drop(lib, key)  # (the library already forgot the pointer: its counters may be dirty)
    _lib.check(rc, "rasterize")


def _mask_u8(m, hw):
    if m is None:
        return None
    m = m.reshape(-1)
    if m.numel() != hw:
        raise _lib.GifHipError(f"texture_pair_loss: visibility mask has {m.numel()} elements, expected {hw}")
    return (m != 0).to(torch.uint8).contiguous()


def texture_pair_loss(a, b, ma, mb, f, gloss=None):
    """mean(sigmoid(((a-b)*ma*mb)^2) * f) over [C,H,W]; with gloss (device scalar) returns d/da instead (d/db = -d/da)."""
    lib = _lib.load()
    if not (a.is_cuda and b.is_cuda and f.is_cuda) or a.dtype != torch.float32 or a.dim() != 3 or a.shape != b.shape:
        raise _lib.GifHipError("texture_pair_loss: need two fp32 device textures [C,H,W] of the same shape (no CPU fallback)")
    a, b = a.contiguous(), b.contiguous()
    C, H, W = a.shape
    HW = H * W
    f = f.to(torch.float32).reshape(-1).contiguous()
    if f.numel() != HW:
        raise _lib.GifHipError(f"texture_pair_loss: face mask has {f.numel()} elements, expected {HW}")
    ma, mb = _mask_u8(ma, HW), _mask_u8(mb, HW)
    if gloss is None:
        partial = torch.empty((lib.gif_texture_pair_loss_partials(C * HW),), device=a.device, dtype=torch.float32)
        loss = torch.empty((), device=a.device, dtype=torch.float32)
        _lib.check(lib.gif_texture_pair_loss_f32(a.data_ptr(), b.data_ptr(), _p(ma), _p(mb), f.data_ptr(), partial.data_ptr(),
                                                 loss.data_ptr(), C, HW, _stream()), "texture_pair_loss")
        return loss
    ga = torch.empty_like(a)
    gloss = gloss.to(torch.float32).contiguous()
    _lib.check(lib.gif_texture_pair_loss_bwd_f32(a.data_ptr(), b.data_ptr(), _p(ma), _p(mb), f.data_ptr(), gloss.data_ptr(),
                                                 ga.data_ptr(), C, HW, _stream()), "texture_pair_loss_bwd")
    return ga


def resize(x, out_hw, mode: str, backward_to=None):
    """NCHW fp32 resize (bilinear / bicubic, align_corners=False).  backward_to=(Hi, Wi): apply the adjoint to x instead."""
    lib = _lib.load()
    if not x.is_cuda or x.dtype != torch.float32 or x.dim() != 4:
        raise _lib.GifHipError("resize: need a 4-D fp32 device tensor (no CPU fallback)")
    if mode not in ("bilinear", "bicubic"):
        raise _lib.GifHipError(f"resize: mode {mode!r} not supported (bilinear | bicubic)")
    x = x.contiguous()
    B, C, H, W = x.shape
    m = 0 if mode == "bilinear" else 1
    if backward_to is None:
        Ho, Wo = out_hw
        y = torch.empty((B, C, Ho, Wo), device=x.device, dtype=torch.float32)
        _lib.check(lib.gif_resize_f32(x.data_ptr(), y.data_ptr(), B * C, H, W, Ho, Wo, m, _stream()), "resize")
        return y
    Hi, Wi = backward_to
    gx = torch.empty((B, C, Hi, Wi), device=x.device, dtype=torch.float32)
    _lib.check(lib.gif_resize_bwd_f32(x.data_ptr(), gx.data_ptr(), B * C, Hi, Wi, H, W, m, _stream()), "resize_bwd")
    return gx


for _name in ("pack_weight", "conv3x3_winograd", "conv_fwd", "conv_bwd_data", "conv3x3_winograd_wgrad", "conv_wgrad", "upfirdn2d",
              "bias_act", "bias_act_bwd", "colsum", "mul_reduce", "bilinear_down", "act_inv_mul_reduce", "mbstd_fwd", "mbstd_bwd",
              "sqnorm_per_sample", "rasterize", "texture_pair_loss", "resize"):
    globals()[_name] = _device_guard(globals()[_name])
del _name


def _mat(t, what):
    if not t.is_cuda or t.dtype != torch.float32 or t.dim() != 2:
        raise _lib.GifHipError(f"{what}: need a 2-D fp32 device tensor (no CPU fallback), got {tuple(t.shape)} {t.dtype} on {t.device}")
    if t.stride(1) == 1 and t.stride(0) >= t.shape[1] and t.data_ptr() % 16 == 0 and t.stride(0) % 4 == 0:
        return t
    return _aligned(t.contiguous())  # (.contiguous() alone hands a dense matrix at an odd offset back as it is)


def linear_nt(a, b, bias=None, scale=1.0, act=False, slope=0.2, gain=1.0, n_pad=None):
    """[M, n_pad] = act(scale * a[M,K] @ b[N,K]^T + bias[n_pad]); columns N..n_pad are zero.  K % 4 == 0."""
    lib = _lib.load()
    a, b = _mat(a, "linear_nt"), _mat(b, "linear_nt")
    M = a.shape[0]
    N, K = b.shape
    assert a.shape[1] >= K, (a.shape, b.shape)  # `a` may carry padding columns beyond K
    n_pad = N if n_pad is None else n_pad
    # (the kernel reads bias[n] for n < N only: the logical width is taken as well as the padded one EqualLinear passes)
    bias = _vec(bias, "linear_nt: bias", (N,) if bias is not None and tuple(bias.shape) == (N,) else (n_pad,), a.device)
    c = torch.empty((M, n_pad), device=a.device, dtype=torch.float32)
    _lib.check(lib.gif_linear_nt_f32(a.data_ptr(), b.data_ptr(), _p(bias), c.data_ptr(), M, N, K, a.stride(0), b.stride(0), n_pad,
                                     n_pad, float(scale), 1 if act else 0, float(slope), float(gain), _stream()), "linear_nt")
    return c


LINEAR_BANK_MAX = 40  # segments per launch (kernel-argument table, csrc/linear.hip)


def linear_bank_ok(x, weights):
    """The modulation bank takes fp32 [n, K] weights with n % 8 == 0 over one [M, K'] input (K % 4 == 0)."""
    K = weights[0].shape[1]
    return (0 < len(weights) <= LINEAR_BANK_MAX and x.dtype == torch.float32 and x.dim() == 2 and x.shape[1] >= K and K % 4 == 0
            and all(w.dim() == 2 and w.shape[1] == K and w.shape[0] % 8 == 0 and w.dtype == torch.float32 for w in weights))


def _bank_segs(weights):
    segs = (_lib.LinearBankSeg * len(weights))()
    keep = []
    for g, w in zip(segs, weights):
        w = _mat(w, "linear_bank")
        assert w.stride(0) == w.shape[1], "linear_bank: weight rows must be contiguous"
        keep.append(w)
        g.w, g.n = w.data_ptr(), w.shape[0]
    return segs, keep


def linear_bank_fwd(x, weights, biases, scale):
    """[scale * x @ w_l^T + b_l for l]: ONE launch for all layers (gif_linear_bank_fwd_f32)."""
    lib = _lib.load()
    x = _mat(x, "linear_bank_fwd")
    M, K = x.shape[0], weights[0].shape[1]
    segs, keep = _bank_segs(weights)
    outs = []
    for g, w, b in zip(segs, weights, biases):
        o = torch.empty((M, w.shape[0]), device=x.device, dtype=torch.float32)
        if b is not None:
            assert b.dtype == torch.float32 and b.numel() == w.shape[0] and b.is_contiguous()
            g.bias = b.data_ptr()
        g.s = o.data_ptr()
        outs.append(o)
    _lib.check(lib.gif_linear_bank_fwd_f32(x.data_ptr(), M, K, x.stride(0), segs, len(weights), float(scale), _stream()), "linear_bank_fwd")
    return outs


def linear_bank_bwd(x, weights, grads, scale, want_x, want_w, want_b, x_cols=None):
    """(gx [M, x_cols] or None, [gw_l] or None, [gb_l] or None) of linear_bank_fwd for the per-layer output gradients `grads`:
    one launch for all weight / bias gradients, one for gx (gif_linear_bank_bwd_f32)."""
    lib = _lib.load()
    x = _mat(x, "linear_bank_bwd")
    M, K = x.shape[0], weights[0].shape[1]
    segs, keep = _bank_segs(weights)
    gws = gbs = None
    new = torch.zeros_like if M == 0 else torch.empty_like  # (an empty batch launches nothing: the gradients are zeros, not garbage)
    if want_w:
        gws = [new(w, memory_format=torch.contiguous_format) for w in weights]
    if want_b:
        gbs = [(torch.zeros if M == 0 else torch.empty)((w.shape[0],), device=x.device, dtype=torch.float32) for w in weights]
    if want_b and not want_w:  # the column sums ride on the weight-gradient launch
        gws = [new(w, memory_format=torch.contiguous_format) for w in weights]
    for i, (g, w, gs) in enumerate(zip(segs, weights, grads)):
        gs = gs.contiguous()
        assert gs.shape == (M, w.shape[0]) and gs.dtype == torch.float32, (gs.shape, gs.dtype)
        keep.append(gs)
        g.gs = gs.data_ptr()
        if gws is not None:
            g.gw = gws[i].data_ptr()
        if gbs is not None:
            g.gbias = gbs[i].data_ptr()
    gx = None
    x_cols = K if x_cols is None else x_cols
    if want_x:
        gx = torch.empty((M, x_cols), device=x.device, dtype=torch.float32)
    _lib.check(lib.gif_linear_bank_bwd_f32(x.data_ptr(), M, K, x.stride(0), segs, len(weights), float(scale), _p(gx),
                                           x_cols, x_cols, _stream()), "linear_bank_bwd")
    return gx, (gws if want_w else None), gbs


def linear_nn(a, b, scale=1.0, n_valid=None, k_pad=None):
    """[M, k_pad] = scale * a[M, :n_valid] @ b[n_valid, K]; columns K..k_pad are zero."""
    lib = _lib.load()
    a, b = _mat(a, "linear_nn"), _mat(b, "linear_nn")
    M = a.shape[0]
    N, K = b.shape
    assert a.shape[1] >= N
    k_pad = K if k_pad is None else k_pad
    c = torch.empty((M, k_pad), device=a.device, dtype=torch.float32)
    _lib.check(lib.gif_linear_nn_f32(a.data_ptr(), b.data_ptr(), c.data_ptr(), M, N, K, a.stride(0), b.stride(0), k_pad, k_pad,
                                     float(scale), _stream()), "linear_nn")
    return c


def linear_tn(a, b, scale=1.0, n_valid=None, k_valid=None):
    """[n_valid, k_valid] = scale * a[M, :n_valid]^T @ b[M, :k_valid]."""
    lib = _lib.load()
    a, b = _mat(a, "linear_tn"), _mat(b, "linear_tn")
    M = a.shape[0]
    assert b.shape[0] == M
    N = a.shape[1] if n_valid is None else n_valid
    K = b.shape[1] if k_valid is None else k_valid
    c = torch.empty((N, K), device=a.device, dtype=torch.float32)
    _lib.check(lib.gif_linear_tn_f32(a.data_ptr(), b.data_ptr(), c.data_ptr(), M, N, K, a.stride(0), b.stride(0), K, float(scale),
                                     _stream()), "linear_tn")
    return c


# ---- style path of ModulatedConv2d (csrc/linear.hip; include/gif_hip.h "Style path") ----
def weight_sq_sum(w):
    """wsq [Cout, Cin] = sum_taps w[Cout, Cin, kh, kw]^2, cached per parameter version like the packed weights."""
    lib = _lib.load()
    if not w.is_cuda or w.dtype != torch.float32 or w.dim() != 4:
        raise _lib.GifHipError("weight_sq_sum: need a 4-D fp32 device weight (no CPU fallback)")

    def build():
        wc = w.contiguous()
        O, I, KH, KW = wc.shape
        out = torch.empty((O, I), device=w.device, dtype=torch.float32)
        _lib.check(lib.gif_weight_sq_sum_f32(wc.data_ptr(), out.data_ptr(), O, I, KH * KW, _stream()), "weight_sq_sum")
        return out
    return _cached_weight_op(w, ("wsq",), build)


def style_demod(s, wsq, scale2, eps, cout_pad):
    """d [B, cout_pad] = rsqrt(scale2 * s[:, :Cin]^2 @ wsq^T + eps); padding columns 1."""
    lib = _lib.load()
    s, wsq = _mat(s, "style_demod"), _mat(wsq, "style_demod")
    B = s.shape[0]
    cout, cin = wsq.shape
    d = torch.empty((B, cout_pad), device=s.device, dtype=torch.float32)
    _lib.check(lib.gif_style_demod_f32(s.data_ptr(), wsq.data_ptr(), d.data_ptr(), B, cout, cin, s.stride(0), wsq.stride(0), cout_pad,
                                       cout_pad, float(scale2), float(eps), _stream()), "style_demod")
    return d


def style_demod_bwd_s(gd, d, wsq, s, gs_in, scale2):
    """gs_total [B, cin_pad] = gs_in + 2 * s * ((gd * (-scale2/2) * d^3)[:, :Cout] @ wsq); cin_pad = s.shape[1]."""
    lib = _lib.load()
    gd, d, wsq, s = _mat(gd, "style_demod_bwd_s"), _mat(d, "style_demod_bwd_s"), _mat(wsq, "style_demod_bwd_s"), _mat(s, "style_demod_bwd_s")
    B, cin_pad = s.shape
    cout, cin = wsq.shape
    if gd.shape != d.shape or gd.stride(0) != d.stride(0):
        gd, d = gd.contiguous(), d.contiguous()
    if gs_in is not None:
        gs_in = gs_in.contiguous()
        assert gs_in.shape == s.shape
    s = s.contiguous()
    out = torch.empty((B, cin_pad), device=s.device, dtype=torch.float32)
    _lib.check(lib.gif_style_demod_bwd_s_f32(gd.data_ptr(), d.data_ptr(), wsq.data_ptr(), s.data_ptr(), _p(gs_in), out.data_ptr(), B, cout,
                                             cin, gd.stride(0), wsq.stride(0), cin_pad, cin_pad, float(scale2), _stream()),
               "style_demod_bwd_s")
    return out


def style_demod_bwd_w(gd, d, s, cout, cin, scale2):
    """g_wsq [Cout, Cin] = (gd * (-scale2/2) * d^3)[:, :Cout]^T @ s[:, :Cin]^2."""
    lib = _lib.load()
    gd, d, s = _mat(gd, "style_demod_bwd_w"), _mat(d, "style_demod_bwd_w"), _mat(s, "style_demod_bwd_w")
    if gd.stride(0) != d.stride(0):
        gd, d = gd.contiguous(), d.contiguous()
    B = s.shape[0]
    out = torch.empty((cout, cin), device=s.device, dtype=torch.float32)
    _lib.check(lib.gif_style_demod_bwd_w_f32(gd.data_ptr(), d.data_ptr(), s.data_ptr(), out.data_ptr(), B, cout, cin, gd.stride(0),
                                             s.stride(0), float(scale2), _stream()), "style_demod_bwd_w")
    return out


def demod_wgrad(w, g_wsq):
    """gW [Cout, Cin, kh, kw] = 2 * w * g_wsq[:, :, None, None]."""
    lib = _lib.load()
    wc = w.contiguous()
    O, I, KH, KW = wc.shape
    g_wsq = g_wsq.contiguous()
    out = torch.empty_like(wc)
    _lib.check(lib.gif_demod_wgrad_f32(wc.data_ptr(), g_wsq.data_ptr(), out.data_ptr(), O, I, KH * KW, _stream()), "demod_wgrad")
    return out


for _name in ("linear_nt", "linear_nn", "linear_tn", "weight_sq_sum", "style_demod", "style_demod_bwd_s", "style_demod_bwd_w", "demod_wgrad"):
    globals()[_name] = _device_guard(globals()[_name])
del _name


FP32_MFMA_MODES = {"native": 0, "bf16x3": 1, "f16x2": 2}


def set_fp32_mfma_mode(mode):
    """How fp32 convolution contractions reach the matrix cores (process-wide, see include/gif_hip.h): "native" fp32 MFMA
    or "bf16x3" (exact three-way bf16 split of every fp32 operand, six bf16 MFMA products, fp32 accumulation).  Tensors
    are fp32 in HBM either way."""
    global _fp32_mode_cache
    _lib.check(_lib.load().gif_set_fp32_mfma_mode(FP32_MFMA_MODES[mode] if isinstance(mode, str) else int(mode)), "set_fp32_mfma_mode")
    _fp32_mode_cache = None


_fp32_mode_cache = None


def get_fp32_mfma_mode() -> str:
    global _fp32_mode_cache
    if _fp32_mode_cache is None:
        m = _lib.load().gif_get_fp32_mfma_mode()
        _fp32_mode_cache = {v: k for k, v in FP32_MFMA_MODES.items()}[m]
    return _fp32_mode_cache


def h2_fallback_stats(reset=False):
    """(guarded f16x2 launches that took the bf16x3 fallback,) on the current device since the last reset.  Synchronises."""
    out = (ctypes.c_uint64 * 2)()
    _lib.check(_lib.load().gif_h2_fallback_stats(out, 1 if reset else 0), "h2_fallback_stats")
    return int(out[0])


def prof_enable(on: bool):
    _lib.load().gif_prof_enable(1 if on else 0)


def prof_read(family: int):
    ms, fl, n = ctypes.c_double(), ctypes.c_double(), ctypes.c_int64()
    _lib.load().gif_prof_read(family, ctypes.byref(ms), ctypes.byref(fl), ctypes.byref(n))
    return ms.value, fl.value, n.value
