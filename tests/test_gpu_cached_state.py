"""-m gpu: what the library remembers between calls (DESIGN.md "Remembered state"), through the kernels that consume it.

tests/test_cache_keys_cpu.py drives the three host caches with a counting `build`.  Here the same changes of the source reach the
device: a packed / transformed weight (ops._cached_weight_op), the topology tables on a faces tensor (render._topology,
antialias.edge_adjacency), FlatAdam's chunk table of raw addresses, the version bump after FlatAdam's raw-pointer writes, and the
WEIGHT_CACHE switch around the side-stream generator forward of GifTrainer.d_step.  A stale entry raises nothing: the convolution
runs with last step's weights and returns a plausible image.

CONSUMERS (one small shape per packed form; the weight is a Parameter [1,O,I,K,K] handed over as `p.squeeze(0)`, a fresh view of
the base each call, as layers.ModulatedConv2d does; shapes are test_gpu_conv_routes rows or the smallest its predicates admit, the
kernel family asserted with ops.prof_read):
  direct_fwd / direct_dgrad  33 -> 48, 3x3, 9 x 7    native f32 (family 0), bf16x3 f32x3 (8), f16x2 f32h2x3 (13)
  thin_b1_c4_o9              register-staged (5)     f32
  dense_c9_o17               tap-dense (12)          f32x3_tapdense
  f16_halo_16, f16_gather_s2 f16 activations (6)     f16
  wino_fwd / wino_dgrad      WINOGRAD_MIN_TILES 16, 8 x 8: native 32 -> 48 (2), bf16x3 32 -> 128 (10), f16x2 256 -> 256 (14)
  style                      weight_sq_sum at [48,33,3,3] -> style_demod (which takes cin % 4 == 0 only and refuses 33 columns: it
                             reads the cached sums with three zero columns appended, the same value)
  direct_fwd_h2_only         pack_weight(h2=True) f32h2, consumed by gif_conv2d_fwd_f32h2 without the guarded twin (13)
ROUTES a .. l: see ROUTES, test_route_e_flat_adam and the tests named route_i .. route_l.  Per cell: (1) the result after the change
is bit-equal to the same call after ops.clear_weight_cache(); (2) it differs from the result on the old weight; (3) it meets its
family's bound against fp64 on the new weight (test_gpu_conv_routes._check / TOL / TINY; the style rule of
test_gpu_linear_reduce_routes.test_style_path) — no tolerance is introduced here; (4) launches of gif_pack_weight*,
gif_winograd_weight* and gif_weight_sq_sum_f32, counted with recorded_launches: a repeated call records 0, the first call after a
change exactly 1.

Observed pack-launch counts on the MI355X (one run of this module, "[cached state]" lines with -s), as (first call, repeat, first
call after the route, repeat, after clear_weight_cache()):
  routes a, b, c_slice, c_detach, d, f, g, h   each of the 18 consumers: 1, 0, 1, 0, 1
  route e (FlatAdam + EMA)                     each of the 18 consumers, parameter and EMA twin alike: 1, 0, 1, 0, 1; after the
                                               found_inf = 1 step 1 and 1 (the version counters rose again), with unchanged bits
  route i (mode cycle on one weight)           direct and Winograd: native 1, bf16x3 1, f16x2 1, native again 0 (the mode is part of
                                               the layout tag: the first entry is still valid); after an in-place change 1, then 0,
                                               in every mode
  route j (forward / data gradient)            four modes / routes: fwd 1, dgrad 1, fwd 0, dgrad 0; after the change the same
  route k (513 1x1 weights)                    1 each; the 513th insertion empties the full cache, so the first weight again: 1,
                                               the 513th again: 0; len(_weight_cache) <= 512 throughout
  route l (WEIGHT_CACHE = False)               every call 1, nothing stored

FINDINGS, parent commit -> now:
  1. `faces.data = other` (same or another face count): render._topology and antialias.edge_adjacency answered with the tables of
     the OLD faces (the key held the version counter, which `.data =` keeps, and neither address nor shape) -> both keys hold
     (version, data_ptr, shape, stride, ...): rebuilt.  Found and fixed on the host (tests/test_cache_keys_cpu.py); the GPU rows
     here run only the equal-size swap, and only with the fix in place.
  2. copy.deepcopy(faces) copies the attribute to a tensor with a version counter of its own: once the copy's counter reached the
     cached one, an edited copy answered with the original's tables -> the address in the key tells them apart (host row).
  3. Weight cache, FlatAdam table, version bumps, two-stream block: no stale hit, no race and no difference found; ops.py, optim.py
     and train_step.py are the parent commit's, and every cell above passes on them.
  4. style_demod refuses a [48,33] operand (cin % 4): not a defect, the model pads; see the `style` consumer.

Wall time of the module on the MI355X: 202 tests in 6.3 s (8 s with start-up); the slowest are the first call of the process
(1.7 s: it loads the library) and the two GifTrainer runs (1.1 s together).
"""
import contextlib
import math
import zlib

import pytest
import torch
import torch.nn.functional as F

import test_gpu_empty_sizes as E
from test_gpu_conv_routes import TINY, TOL, _check, _dev, cpad
from test_gpu_input_forms import recorded_launches
from test_gpu_linear_reduce_routes import ADAM_ROWS, U32, _adam_ref
from test_gpu_linear_reduce_routes import _check as _check_lr

pytestmark = pytest.mark.gpu

H16 = torch.float16
FP32_MODES = ("native", "bf16x3", "f16x2")
WINO_FAMS = (2, 10, 14)
PACK_PREFIXES = ("gif_pack_weight", "gif_winograd_weight", "gif_weight_sq_sum_f32")
assert all(k in TOL and k in TINY for k in FP32_MODES + ("f16",))


def pack_launches(rec):
    """launches (not size queries) of the packing, Winograd weight transform and squared-sum kernels among the recorded calls"""
    return sum(1 for name, _ in rec.calls if name.startswith(PACK_PREFIXES) and not name.endswith("_bytes"))


def counted(c, w):
    with recorded_launches() as rec:
        outs = c.run(w)
    return outs, pack_launches(rec)


def same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and x.dtype == y.dtype and torch.equal(x, y) for x, y in zip(a, b))


@contextlib.contextmanager
def session(mode=None, patch=()):
    """the fp32 contraction mode and ops attributes of a cell, an empty weight cache switched on; everything restored after"""
    from gif_amd import ops
    saved_mode, cache_was = ops.get_fp32_mfma_mode(), ops.WEIGHT_CACHE
    saved = [(k, getattr(ops, k)) for k, _ in patch]
    try:
        for k, v in patch:
            setattr(ops, k, v)
        if mode in FP32_MODES:
            ops.set_fp32_mfma_mode(mode)
        ops.WEIGHT_CACHE = True
        ops.clear_weight_cache()
        yield ops
    finally:
        ops.prof_enable(False)
        ops.set_fp32_mfma_mode(saved_mode)
        for k, v in saved:
            setattr(ops, k, v)
        ops.WEIGHT_CACHE = cache_was
        ops.clear_weight_cache()


def families(fn):
    """(fn(), {kernel family: ops recorded}) — family 4, the Winograd transforms recorded beside the GEMM, left out"""
    from gif_amd import ops
    ops.prof_enable(True)
    for fam in range(18):
        ops.prof_read(fam)  # (reading clears a family's records)
    out = fn()
    torch.cuda.synchronize()
    ran = {fam: ops.prof_read(fam)[2] for fam in range(18)}
    ops.prof_enable(False)
    return out, {f: n for f, n in ran.items() if n and f != 4}


# ------------------------------------------------------------------------------------------------------------------- consumers
class Conv:
    """One convolution of test_gpu_conv_routes' Row shape (B, Cin, Cout, K, stride, pad, H, W) of the FORWARD conv, no epilogue."""

    def __init__(self, name, op, shape, mode, fam, patch=(), halo=None):
        self.name, self.op, self.shape, self.mode, self.fam, self.patch, self.halo = name, op, shape, mode, fam, patch, halo
        B, Ci, Co, K, s, p, H, W = shape
        self.wshape = (Co, Ci, K, K)
        self.f16 = mode == "f16"
        self.hs = ((H + 2 * p - K) // s + 1, (W + 2 * p - K) // s + 1)

    def weights(self, salt):
        Co, Ci, K, _ = self.wshape
        g = torch.Generator().manual_seed(zlib.crc32(f"{self.name} w{salt}".encode()))
        return torch.randn(Co, Ci, K, K, generator=g) / math.sqrt(Ci * K * K)

    def setup(self):
        B, Ci, Co, K, s, p, H, W = self.shape
        g = torch.Generator().manual_seed(zlib.crc32(f"{self.name} x".encode()))
        cin_o, hw = (Ci, (H, W)) if self.op == "fwd" else (Co, self.hs)
        x = torch.randn(B, cin_o, *hw, generator=g)
        self.x = x.to(H16).float() if self.f16 else x
        self.dt = H16 if self.f16 else torch.float32
        self.xd = _dev(self.x, cpad(cin_o, self.f16), self.dt)
        if self.halo is not None:
            from gif_amd import _lib
            assert bool(_lib.load().gif_conv2d_f16_halo_eligible(cpad(Ci, True), cpad(Co, True), K, K, s, *self.hs)) == self.halo

    def run(self, w):
        from gif_amd import ops
        B, Ci, Co, K, s, p, H, W = self.shape
        spec = ops.ConvSpec(K, K, s, p)
        if self.op == "fwd":
            return (ops.conv_fwd(self.xd, w, spec),)
        return (ops.conv_bwd_data(self.xd, w, spec, (H, W)),)

    def check(self, outs, W1, what):
        """the fp64 bound of test_gpu_conv_routes over the operands the kernel reads (f16: the half-rounded weights)"""
        B, Ci, Co, K, s, p, H, W = self.shape
        (y,) = outs
        w = (W1.to(H16) if self.f16 else W1).double()
        x = self.x.double()
        if self.op == "fwd":
            conv = lambda a, b: F.conv2d(a, b, stride=s, padding=p)
            c_out, hw = Co, self.hs
        else:
            op_ = (H - ((self.hs[0] - 1) * s + K - 2 * p), W - ((self.hs[1] - 1) * s + K - 2 * p))
            conv = lambda a, b: F.conv_transpose2d(a, b, stride=s, padding=p, output_padding=op_)
            c_out, hw = Ci, (H, W)
        assert y.shape == (B, cpad(c_out, self.f16), *hw) and y.dtype == self.dt, (y.shape, y.dtype)
        assert torch.count_nonzero(y[:, c_out:]).item() == 0, f"{what}: padded output channels are not zero"
        got = y[:, :c_out].double().cpu()
        assert torch.isfinite(got).all(), f"{what}: NaN / Inf"
        _check(got, conv(x, w), conv(x.abs(), w.abs()), self.mode, what)


class Style:
    """weight_sq_sum feeding style_demod at [48,33,3,3]: (wsq, d)"""
    name, mode, fam, patch, wshape = "style", None, None, (), (48, 33, 3, 3)
    B, cin_pad, cout_pad, eps = 3, 36, 48, 1e-8
    scale2 = 1.0 / (33 * 9)

    def weights(self, salt):
        return torch.randn(*self.wshape, generator=torch.Generator().manual_seed(40 + salt))

    def setup(self):
        self.S = torch.randn(self.B, 33, generator=torch.Generator().manual_seed(4)) + 1.0
        s = torch.zeros(self.B, self.cin_pad)
        s[:, :33] = self.S
        self.sd = s.cuda()

    def run(self, w):
        from gif_amd import ops
        wsq = ops.weight_sq_sum(w)  # [48,33]: the cached result, at the odd channel count
        # style_demod takes cin % 4 == 0 and 4-float row strides (it refuses [48,33]): the same sums with three zero columns, under
        # zero columns of s — exactly the demodulation of the 33-channel weight
        return wsq, ops.style_demod(self.sd, F.pad(wsq, (0, self.cin_pad - 33)), self.scale2, self.eps, self.cout_pad)

    def check(self, outs, W1, what):
        wsq, d = outs
        wsq_ref = W1.double().pow(2).sum(dim=(2, 3))
        _check_lr(wsq, wsq_ref, wsq_ref, "style", f"{what} weight_sq_sum")
        v = self.scale2 * (self.S.double().pow(2) @ wsq.cpu().double().T) + self.eps  # (the operand style_demod read)
        d_ref = v.rsqrt()
        _check_lr(d[:, :48], d_ref, 0.5 * d_ref.pow(3) * v, "style", f"{what} style_demod", extra=2 * U32 * d_ref)


class ConvH2Only(Conv):
    """pack_weight(h2=True), the f16x2 operand alone, consumed by gif_conv2d_fwd_f32h2 without its guarded bf16x3 twin (what
    _conv_direct hands over with ops.H2_GUARD off): the one packed form no default route reaches"""

    def run(self, w):
        import ctypes
        from gif_amd import ops
        B, Ci, Co, K, s, p, H, W = self.shape
        spec, Cb, Cs = ops.ConvSpec(K, K, s, p), self.xd.shape[1], cpad(Co, False)
        wp = ops.pack_weight(w, True, Cs, Cb, h2=True)
        out = ops.empty_nhwc(B, Cs, *self.hs, self.xd.device)
        g = ops._geom(B, H, W, Cb, *self.hs, Cs, spec)
        e = ops._epilogue(out_bchw=(B, Cs, *self.hs))
        ops._call("conv2d_fwd", "f16x2", self.xd.data_ptr(), wp.data_ptr(), None, out.data_ptr(), ctypes.byref(g), ctypes.byref(e),
                  ops._stream())
        return (out,)


DIRECT_FAM = {"f16x2": 13, "bf16x3": 8, "native": 0}
WINO = (("WINOGRAD_MIN_TILES", 16),)
CONSUMERS = (
    [Conv(f"direct_fwd-{m}", "fwd", (1, 33, 48, 3, 1, 1, 9, 7), m, DIRECT_FAM[m]) for m in FP32_MODES]
    + [Conv(f"direct_dgrad-{m}", "dgrad", (1, 48, 33, 3, 1, 1, 9, 7), m, DIRECT_FAM[m]) for m in FP32_MODES]
    + [Conv("thin_b1_c4_o9", "fwd", (1, 4, 9, 3, 1, 1, 7, 5), "native", 5),
       Conv("dense_c9_o17", "fwd", (1, 9, 17, 3, 1, 1, 37, 29), "bf16x3", 12),
       Conv("f16_halo_16", "fwd", (2, 32, 64, 3, 1, 1, 16, 16), "f16", 6, halo=True),
       Conv("f16_gather_s2", "fwd", (2, 32, 32, 3, 2, 0, 33, 35), "f16", 6, halo=False),
       Conv("wino_fwd-native", "fwd", (1, 32, 48, 3, 1, 1, 8, 8), "native", 2, WINO),
       Conv("wino_dgrad-native", "dgrad", (1, 48, 32, 3, 1, 1, 8, 8), "native", 2, WINO),      # contraction 32, output 48
       Conv("wino_fwd-bf16x3", "fwd", (1, 32, 128, 3, 1, 1, 8, 8), "bf16x3", 10, WINO),
       Conv("wino_dgrad-bf16x3", "dgrad", (1, 128, 32, 3, 1, 1, 8, 8), "bf16x3", 10, WINO),   # contraction 32, output 128
       Conv("wino_fwd-f16x2", "fwd", (1, 256, 256, 3, 1, 1, 8, 8), "f16x2", 14, WINO),
       Conv("wino_dgrad-f16x2", "dgrad", (1, 256, 256, 3, 1, 1, 8, 8), "f16x2", 14, WINO),
       ConvH2Only("direct_fwd_h2_only-f16x2", "fwd", (1, 33, 48, 3, 1, 1, 9, 7), "f16x2", 13),
       Style()])
BY_NAME = {c.name: c for c in CONSUMERS}


def assert_family(c, ran, wino_calls):
    if c.fam is None:
        return
    assert ran == {c.fam: 1}, f"{c.name}: expected one op in family {c.fam}, got {ran}"
    assert wino_calls == (1 if c.fam in WINO_FAMS else 0), f"{c.name}: Winograd route {'not ' if c.fam in WINO_FAMS else ''}taken"


def param_of(W):
    return torch.nn.Parameter(W.cuda()[None].contiguous())  # [1,O,I,K,K], as ModulatedConv2d keeps it


def warm(c, p):
    """first call (family asserted, 1 pack launch) and a repeat (0 launches, the same bits) on the parameter's current contents"""
    from gif_amd import ops
    n_wino = ops.prof_winograd_calls()
    (y, n), ran = families(lambda: counted(c, p.squeeze(0)))
    assert_family(c, ran, ops.prof_winograd_calls() - n_wino)
    assert n == 1, f"{c.name}: the first call recorded {n} pack launches"
    y2, n2 = counted(c, p.squeeze(0))
    assert n2 == 0 and same(y, y2), f"{c.name}: the repeated call recorded {n2} pack launches / changed bits"
    return y


def first_calls(c, p):
    """the first call after a change and its repeat, each with its pack-launch count (no cache is cleared here)"""
    return counted(c, p.squeeze(0)) + counted(c, p.squeeze(0))


def after_change(c, p, y_old, W_old, what, first=1, calls=None):
    """assertions 1 .. 4 of a cell on the parameter's NEW contents; returns the result.  calls: first_calls(c, p), where the caller
    had to make them earlier (before this function clears the cache)"""
    from gif_amd import ops
    y1, n1, y1b, n1b = first_calls(c, p) if calls is None else calls
    W1 = p.detach()[0].cpu()
    assert not torch.equal(W1, W_old), f"{what}: the route did not change the weight"
    ops.clear_weight_cache()
    y1c, n1c = counted(c, p.squeeze(0))
    print(f"\n[cached state] {what}: pack launches after the route {n1}, repeat {n1b}, after clear {n1c}")
    assert n1c == 1
    assert same(y1, y1c), f"{what}: not the bits of the same call on an empty cache: a stale entry answered"
    assert not same(y1, y_old), f"{what}: the result did not follow the weight"
    c.check(y1, W1, what)
    assert n1 == first, f"{what}: the first call after the change recorded {n1} pack launches, expected {first}"
    assert n1b == 0 and same(y1, y1b), f"{what}: the repeated call recorded {n1b} pack launches / changed bits"
    return y1


# ---------------------------------------------------------------------------------------------------------------------- routes
def _a(p, new):
    with torch.no_grad():
        p.mul_(0.5)


def _b(p, new):
    with torch.no_grad():
        p.copy_(new)


def _c_slice(p, new):
    with torch.no_grad():
        p[0, 1:3] = new[0, 1:3]


def _c_detach(p, new):
    p.detach().mul_(-1.25)


def _d(p, new):
    p.grad = torch.sign(new)
    torch.optim.Adam([p], lr=0.05).step()
    p.grad = None


def _f(p, new):
    m = torch.nn.Module()
    m.weight = p
    m.load_state_dict({"weight": new})


def _g(p, new):
    p.data = new


def _h(p, new):
    from gif_amd import ops
    p.data.copy_(new)  # no version bump, the same address: the caller's to announce
    ops.clear_weight_cache()


ROUTES = {"a_no_grad_inplace": _a, "b_copy_": _b, "c_slice_write": _c_slice, "c_detach_write": _c_detach, "d_torch_adam": _d,
          "f_load_state_dict": _f, "g_data_swap": _g, "h_data_copy_then_clear": _h}


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("name", list(BY_NAME))
def test_route(name, route):
    c = BY_NAME[name]
    with session(c.mode, c.patch):
        c.setup()
        W0 = c.weights(0)
        p = param_of(W0)
        y0 = warm(c, p)
        ROUTES[route](p, c.weights(1).cuda()[None].contiguous())
        after_change(c, p, y0, W0, f"{route} {name}")


@pytest.mark.parametrize("name", list(BY_NAME))
def test_route_e_flat_adam(name):
    """FlatAdam.step writes the parameter and its EMA twin through raw pointers; only the version bump that follows stands between a
    consumer and last step's weights.  Both entries are warm before the step and nothing clears the cache until both were consumed
    again.  A found_inf = 1 step changes no bit of either result."""
    from gif_amd.optim import FlatAdam
    from gif_amd.train_step import FlatGradBucket
    c = BY_NAME[name]
    with session(c.mode, c.patch):
        c.setup()
        W0, E0 = c.weights(0), c.weights(2)
        p, e = param_of(W0), param_of(E0)
        bucket = FlatGradBucket([p])
        opt = FlatAdam([p], lr=0.05, betas=(0.5, 0.99), bucket=bucket, ema_params=[e])
        yp, ye = warm(c, p), warm(c, e)
        versions = (p._version, e._version)
        bucket.views[0].copy_(torch.sign(c.weights(1)).cuda()[None])
        opt.step(ema_decay=0.5)
        assert p._version > versions[0] and e._version > versions[1]
        calls_p, calls_e = first_calls(c, p), first_calls(c, e)
        yp1 = after_change(c, p, yp, W0, f"e_flat_adam {name} parameter", calls=calls_p)
        ye1 = after_change(c, e, ye, E0, f"e_flat_adam {name} ema", calls=calls_e)
        # a skipped step (found_inf = 1), both entries warm again
        assert same(yp1, c.run(p.squeeze(0))) and same(ye1, c.run(e.squeeze(0)))
        before = (p.detach().clone(), e.detach().clone())
        found, inv = torch.ones((), device="cuda"), torch.ones((), device="cuda")
        opt.step(ema_decay=0.5, inv_grad_scale=inv, found_inf=found)
        torch.cuda.synchronize()
        assert torch.equal(before[0], p.detach()) and torch.equal(before[1], e.detach()), f"{name}: a found_inf step wrote"
        (yp2, np2), (ye2, ne2) = counted(c, p.squeeze(0)), counted(c, e.squeeze(0))
        print(f"\n[cached state] e_flat_adam {name}: pack launches after the found_inf step {np2}, {ne2}")
        assert same(yp1, yp2) and same(ye1, ye2), f"{name}: a found_inf = 1 step changed a result"
        assert np2 <= 1 and ne2 <= 1


@pytest.mark.parametrize("name", ["direct_fwd", "wino_fwd"])
def test_route_i_mode_cycle_on_one_weight(name):
    """set_fp32_mfma_mode native -> bf16x3 -> f16x2 -> native on ONE weight: the mode is part of the layout tag, so each mode packs
    once and the return to native finds its entry still valid; after an in-place change every mode packs anew"""
    from gif_amd import ops
    cs = {m: BY_NAME[f"{name}-{m}"] for m in FP32_MODES}
    if name == "wino_fwd":  # one weight for the three modes: 256 -> 256 takes the Winograd route in all of them
        cs = {m: Conv(f"wino_fwd_256-{m}", "fwd", (1, 256, 256, 3, 1, 1, 8, 8), m, f, WINO) for m, f in zip(FP32_MODES, WINO_FAMS)}
    base = cs["native"]
    with session("native", base.patch):
        base.setup()
        for c in cs.values():
            c.x, c.xd, c.dt = base.x, base.xd, base.dt
        W0 = base.weights(0)
        p = param_of(W0)
        y, counts = {}, []
        for step, m in enumerate(FP32_MODES + ("native",)):
            ops.set_fp32_mfma_mode(m)
            n_wino = ops.prof_winograd_calls()
            (out, n), ran = families(lambda: counted(cs[m], p.squeeze(0)))
            assert_family(cs[m], ran, ops.prof_winograd_calls() - n_wino)
            counts.append(n)
            if step == 3:
                assert same(out, y["native"]), "native after the cycle: other bits than before it"
            y[m] = out
            cs[m].check(out, W0, f"i {name} {m}")
        print(f"\n[cached state] i_mode_cycle {name}: pack launches {counts}")
        assert counts == [1, 1, 1, 0], counts
        with torch.no_grad():
            p.mul_(0.5)
        W1 = p.detach()[0].cpu()
        for m in FP32_MODES:
            ops.set_fp32_mfma_mode(m)
            out, n = counted(cs[m], p.squeeze(0))
            out2, n2 = counted(cs[m], p.squeeze(0))
            assert (n, n2) == (1, 0) and same(out, out2), (m, n, n2)
            assert not same(out, y[m])
            cs[m].check(out, W1, f"i {name} {m} after the change")
            y[m] = out
        ops.clear_weight_cache()
        for m in FP32_MODES:
            ops.set_fp32_mfma_mode(m)
            assert same(y[m], cs[m].run(p.squeeze(0))), f"{m}: not the bits of an empty cache"


@pytest.mark.parametrize("mode,wshape,fams,patch", [("native", (48, 33), (0, 0), ()), ("bf16x3", (48, 33), (8, 8), ()),
                                                     ("f16x2", (48, 33), (13, 13), ()), ("native", (64, 64), (2, 2), WINO)],
                         ids=["direct-native", "direct-bf16x3", "direct-f16x2", "wino-native"])
def test_route_j_forward_and_data_gradient_alternate(mode, wshape, fams, patch):
    """one weight [O,I,3,3] as the forward operand and as the data-gradient operand in alternation: two entries of one base, neither
    answers for the other, both are rebuilt after a change"""
    from gif_amd import ops
    O, I = wshape
    H, W = (8, 8) if patch else (9, 7)
    fwd = Conv(f"j_fwd_{O}_{I}-{mode}", "fwd", (1, I, O, 3, 1, 1, H, W), mode, fams[0], patch)
    dg = Conv(f"j_dgrad_{O}_{I}-{mode}", "dgrad", (1, I, O, 3, 1, 1, H, W), mode, fams[1], patch)
    with session(mode, patch):
        fwd.setup()
        dg.setup()
        W0 = fwd.weights(0)
        p = param_of(W0)
        seq = [fwd, dg, fwd, dg]
        for rnd, Wn in enumerate((W0, None)):
            if Wn is None:
                with torch.no_grad():
                    p.add_(fwd.weights(1).cuda()[None])
                Wn = p.detach()[0].cpu()
            outs, counts = [], []
            for c in seq:
                n_wino = ops.prof_winograd_calls()
                (out, n), ran = families(lambda: counted(c, p.squeeze(0)))
                assert_family(c, ran, ops.prof_winograd_calls() - n_wino)
                outs.append(out)
                counts.append(n)
            print(f"\n[cached state] j {mode} {wshape} round {rnd}: pack launches {counts}")
            assert counts == [1, 1, 0, 0], counts
            assert same(outs[0], outs[2]) and same(outs[1], outs[3])
            fwd.check(outs[0], Wn, f"j fwd {mode} round {rnd}")
            dg.check(outs[1], Wn, f"j dgrad {mode} round {rnd}")
            if rnd:
                assert not same(outs[0], first[0]) and not same(outs[1], first[1])
                ops.clear_weight_cache()
                assert same(outs[0], fwd.run(p.squeeze(0))) and same(outs[1], dg.run(p.squeeze(0))), "a stale entry answered"
            first = outs


def test_route_k_513_weights_then_the_first_again():
    """513 distinct 4 -> 4 1x1 weights fill the cache past its 512 entries; every result is its own weight's, the cache never holds
    more than 512 entries, and the first weight again is packed anew (the insertion that found the cache full emptied it)"""
    g = torch.Generator().manual_seed(13)
    N = 513
    Ws = torch.randn(N, 4, 4, 1, 1, generator=g) * 0.5
    x = torch.randn(1, 4, 5, 5, generator=g)
    ref = torch.einsum("noi,bihw->nbohw", Ws[:, :, :, 0, 0].double(), x.double())
    R = torch.einsum("noi,bihw->nbohw", Ws[:, :, :, 0, 0].double().abs(), x.double().abs())
    with session("native") as ops:
        assert ops._WEIGHT_CACHE_MAX == 512
        spec = ops.ConvSpec(1, 1, 1, 0)
        xd = _dev(x, 4, torch.float32)
        ws = [Ws[i].cuda() for i in range(N)]  # all alive: no entry dies
        ys, counts, sizes = [], [], []
        with recorded_launches() as rec:
            for w in ws:
                before = len(rec.calls)
                ys.append(ops.conv_fwd(xd, w, spec))
                counts.append(sum(1 for n, _ in rec.calls[before:] if n.startswith(PACK_PREFIXES) and not n.endswith("_bytes")))
                sizes.append(len(ops._weight_cache))
        assert counts == [1] * N
        assert max(sizes) == 512 and sizes[511] == 512 and sizes[512] == 1, (max(sizes), sizes[510:])

        class Pointwise:
            @staticmethod
            def run(w):
                return (ops.conv_fwd(xd, w, spec),)

        y_first, n_first = counted(Pointwise, ws[0])
        y_last, n_last = counted(Pointwise, ws[N - 1])
        print(f"\n[cached state] k: pack launches of the first weight again {n_first}, of the 513th again {n_last}")
        assert (n_first, n_last) == (1, 0)
        assert torch.equal(y_first[0], ys[0]) and torch.equal(y_last[0], ys[N - 1])
        got = torch.stack([y.double().cpu() for y in ys])
        _check(got, ref, R, "native", "k 513 weights")
        assert len(ops._weight_cache) <= 512


@pytest.mark.parametrize("name", list(BY_NAME))
def test_route_l_cache_switched_off(name):
    """WEIGHT_CACHE = False: every call packs, nothing is stored, and the bits are those of the cached path"""
    c = BY_NAME[name]
    with session(c.mode, c.patch) as ops:
        c.setup()
        W0 = c.weights(0)
        p = param_of(W0)
        y_cached = warm(c, p)
        ops.clear_weight_cache()
        ops.WEIGHT_CACHE = False
        (y0, n0), (y0b, n0b) = counted(c, p.squeeze(0)), counted(c, p.squeeze(0))
        assert (n0, n0b) == (1, 1) and len(ops._weight_cache) == 0
        assert same(y0, y_cached) and same(y0b, y_cached)
        p.data.copy_(c.weights(1).cuda()[None])  # even the write no counter sees: nothing is remembered
        y1, n1 = counted(c, p.squeeze(0))
        assert n1 == 1 and len(ops._weight_cache) == 0 and not same(y1, y0)
        c.check(y1, p.detach()[0].cpu(), f"l {name}")
        ops.WEIGHT_CACHE = True
        assert same(y1, c.run(p.squeeze(0))), f"{name}: cache on and off give different bits"


# -------------------------------------------------------------------------------------------------------------------- topology
TOPOLOGY_OPS = ("vertex_normals", "rasterize_attributes", "antialias-h0", "soft_silhouette-h0")


def _row_edit(f):
    f[3] = torch.tensor([0, 1, 4], device=f.device)  # face 3 turned over: other corner order, other edge slots, a flipped normal


def _winding_flip(f):
    f.copy_(f[:, [0, 2, 1]])


def _data_swap(f):
    # the same F and V (never another face count on the device): the fan's faces in another order, one of them turned over
    f.data = torch.tensor([[0, 2, 3], [0, 3, 4], [0, 1, 4], [0, 1, 2]], device=f.device)


TOPOLOGY_ROUTES = {"row_edit": _row_edit, "winding_flip": _winding_flip, "data_swap_same_F_V": _data_swap}


def _topology_call(op, d, x, faces, aux):
    leaves = E.leaves_on(x, "cuda", torch.float32)
    leaves["f"] = faces
    outs = op.gpu(d, leaves, aux)
    grads = E.backward(outs, leaves, {k: u.cuda() for k, u in aux["ups"].items()}) if op.grad else {}
    torch.cuda.synchronize()
    return {**outs, **grads}, set(grads)


def _topology_flow(op, d, x, faces, what):
    """the op on `faces` (a device tensor that may carry cached tables) for the mesh x (x["f"]: the same faces on the CPU): results
    bit-equal to those on a fresh clone, and under the op's own rule against its float64 reference (err <= 4 * err32 + 2^-23)"""
    x = {k: t.detach().clone() for k, t in x.items()}  # (E.leaves_on marks a float32 CPU input itself as a leaf: a fresh set per flow)
    aux = {}
    if op.prepass is not None:
        aux.update(op.prepass(d, x))
    ref = op.reference(d, x, aux)
    got, grads = _topology_call(op, d, x, faces, aux)
    fresh, _ = _topology_call(op, d, x, faces.clone(), aux)
    assert sorted(got) == sorted(fresh) == sorted(ref[torch.float64])
    for k in got:
        assert torch.equal(got[k], fresh[k]), f"{what} {k}: not the bits of a fresh clone of the faces: stale tables"
        E.compare(f"{what} {k}", got[k], ref[torch.float64][k], ref[torch.float32][k], False, gradient=k in grads)
    return got


def _tables(faces, V):
    from gif_amd import antialias, render
    return [t.clone() for t in render._topology(faces, V, faces.device)] + [antialias.edge_adjacency(faces).clone()]


@pytest.mark.parametrize("route", list(TOPOLOGY_ROUTES))
@pytest.mark.parametrize("name", TOPOLOGY_OPS)
def test_topology_follows_the_faces(name, route):
    """vertex_normals forward and backward, the face gather behind rasterize_attributes' vertex gradient, antialias and
    soft_silhouette on test_gpu_empty_sizes' 5-vertex, 4-face mesh at 8 x 8: the faces tensor carries warm tables, then changes"""
    op, d = E.OPS[name], E.dims_of({})
    assert (d["V"], d["F"], d["H"], d["W"]) == (5, 4, 8, 8)
    x = op.inputs(d)
    faces = x["f"].cuda()
    _topology_flow(op, d, x, faces, f"{name} warm")
    assert hasattr(faces, "_gif_csr") or hasattr(faces, "_gif_edge_adj"), f"{name} left no table on the faces: nothing is tested"
    old = _tables(faces, d["V"])
    TOPOLOGY_ROUTES[route](faces)
    assert faces.shape == (4, 3) and int(faces.max()) < d["V"] and int(faces.min()) >= 0  # (the same F and V, always)
    new, want = _tables(faces, d["V"]), _tables(faces.clone(), d["V"])
    assert all(torch.equal(a, b) for a, b in zip(new, want)), f"{name} {route}: stale tables"
    assert any(not torch.equal(a, b) for a, b in zip(new, old)), f"{route} changed no table: nothing is tested"
    _topology_flow(op, d, dict(x, f=faces.detach().cpu().clone()), faces, f"{name} {route}")


def test_vertex_normals_follow_every_route_in_turn():
    """the three changes one after the other on ONE faces tensor, the normals differing after each"""
    from gif_amd import render
    d = E.dims_of({})
    v, f = E.mesh(d)
    vd, faces = v.cuda(), f.cuda()
    last = render.vertex_normals(vd, faces)
    for route, change in TOPOLOGY_ROUTES.items():
        change(faces)
        got = render.vertex_normals(vd, faces)
        assert torch.equal(got, render.vertex_normals(vd, faces.clone())), f"{route}: stale tables"
        assert not torch.equal(got, last), f"{route}: the normals did not follow the faces"
        ref64, ref32 = (E.rg.normals_ref(v.to(dt), faces.cpu()) for dt in (torch.float64, torch.float32))
        E.compare(f"normals {route}", got, ref64, ref32, False)
        last = got


# ------------------------------------------------------------------------------------------------------------- FlatAdam's table
def test_flat_adam_table_follows_moved_storage():
    """step, move one parameter and one EMA tensor to fresh storage (p.data = p.data.clone()), step again: the kernel writes the NEW
    storage (fp64 Adam within TOL["adam"]), the old storage keeps its bits, every version counter rises on each applied step"""
    from gif_amd.optim import FlatAdam
    from gif_amd.train_step import FlatGradBucket
    sizes = [5, 4097, 3]
    assert all(n in ADAM_ROWS[0][1] for n in sizes)
    g = torch.Generator().manual_seed(14)
    params = [torch.nn.Parameter(torch.randn(n, generator=g).cuda()) for n in sizes]
    emas = [torch.nn.Parameter(p.detach().clone() + 0.01) for p in params]
    lr, b1, b2, eps, decay = 2e-3, 0.5, 0.99, 1e-8, 0.9
    bucket = FlatGradBucket(params)
    opt = FlatAdam(params, lr=lr, betas=(b1, b2), eps=eps, bucket=bucket, ema_params=emas)
    held = {}
    for t in (1, 2):
        grads = [torch.randn(n, generator=g) for n in sizes]
        for view, gr in zip(bucket.views, grads):
            view.copy_(gr)
        if t == 2:  # parameter 1 (two chunks) and EMA 0 move; the old storage stays alive, so a write to it would be seen, not a fault
            for what, tens in (("p1", params[1]), ("e0", emas[0])):
                old = tens.data
                tens.data = tens.data.clone()
                assert tens.data_ptr() != old.data_ptr()
                held[what] = (old, old.clone())
            key_before = opt._table_key
        before = [(p.detach().cpu().double(), opt.state[p]["exp_avg"].cpu().double(), opt.state[p]["exp_avg_sq"].cpu().double(),
                   e.detach().cpu().double()) for p, e in zip(params, emas)]
        versions = [x._version for x in params + emas]
        opt.step(ema_decay=decay)
        torch.cuda.synchronize()
        assert all(x._version > v for x, v in zip(params + emas, versions)), f"step {t}: a version counter did not rise"
        if t == 2:
            assert opt._table_key != key_before and opt._table_key[1] == params[1].data_ptr()
            for what, (old, bits) in held.items():
                assert torch.equal(old.view(torch.int32), bits.view(torch.int32)), f"{what}: the step wrote the storage it had left"
        for i, (p, e, gr, (p0, m0, v0, e0)) in enumerate(zip(params, emas, grads, before)):
            pr, mr, vr, upd = _adam_ref(p0, gr.double(), m0, v0, t, lr, b1, b2, eps, False)
            what = f"table step{t} p{i} n{sizes[i]}"
            _check_lr(p, pr, p0.abs() + 4 * upd.abs(), "adam", f"{what} p")
            df = float(torch.tensor(decay, dtype=torch.float32))
            pn = p.detach().cpu().double()
            _check_lr(e, e0 * df + (1 - df) * pn, e0.abs() * df + (1 - df) * pn.abs(), "adam", f"{what} ema")
            assert not torch.equal(p.detach().cpu().double(), p0) and not torch.equal(e.detach().cpu().double(), e0)


# ------------------------------------------------------------------------------------------------------------ two-stream block
def _trainer(two_streams):
    from gif_amd.train_step import GifTrainer
    from test_gpu_models import _build_d, _build_g
    torch.manual_seed(0)
    G, G_ema, D = _build_g(16).cuda(), _build_g(16).cuda(), _build_d(32).cuda()
    G_ema.load_state_dict(G.state_dict())
    tr = GifTrainer(G, D, G_ema, step=3, fuse_d_passes=False)
    tr.two_streams = two_streams  # (the attribute, not the environment knob)
    return tr


def _batch(gen):
    real = torch.rand(4, 3, 32, 32, device="cuda", generator=gen) * 2 - 1
    cond = torch.rand(4, 6, 32, 32, device="cuda", generator=gen) * 2 - 1
    return real, cond, torch.randint(0, 16, (4,), device="cuda", generator=gen)


def test_two_stream_block_changes_nothing_and_stores_nothing():
    """GifTrainer.d_step with two_streams: the generator forward on the side stream runs with the weight cache off.  Two iterations
    (a plain and an R1 one) give the bits of the one-stream schedule in every loss and every G, D and G_ema parameter; the cache does
    not grow inside the block; the switch is back after a generator forward that raises."""
    from gif_amd import ops
    res, inside = {}, []
    with session():
        for two in (False, True):
            ops.clear_weight_cache()
            tr = _trainer(two)
            main, forward = torch.cuda.current_stream(), tr.G.forward

            def watched(*a, _forward=forward, _main=main, **kw):
                if torch.cuda.current_stream() == _main:
                    return _forward(*a, **kw)
                n = len(ops._weight_cache)
                assert ops.WEIGHT_CACHE is False, "the side-stream forward ran with the weight cache on"
                out = _forward(*a, **kw)
                inside.append((n, len(ops._weight_cache)))
                return out

            tr.G.forward = watched
            gen = torch.Generator(device="cuda").manual_seed(1)
            losses = [[t.item() for t in tr.step(i, *_batch(gen))] for i in (14, 15)]
            tr.flush()
            torch.cuda.synchronize()
            res[two] = (losses, [p.detach().clone() for m in (tr.G, tr.D, tr.G_ema) for p in m.parameters()])
            assert ops.WEIGHT_CACHE is True
            if two:
                def raising(*a, _forward=forward, _main=main, **kw):
                    if torch.cuda.current_stream() == _main:
                        return _forward(*a, **kw)
                    raise RuntimeError("generator forward on the side stream")

                tr.G.forward = raising
                for prior in (True, False):
                    ops.WEIGHT_CACHE = prior
                    with pytest.raises(RuntimeError, match="side stream"):
                        tr.d_step(16, *_batch(gen))
                    assert ops.WEIGHT_CACHE is prior, f"WEIGHT_CACHE {prior} before the block, {ops.WEIGHT_CACHE} after it raised"
                    assert torch.cuda.current_stream() == main
                ops.WEIGHT_CACHE = True
            torch.cuda.synchronize()
    assert len(inside) == 2 and all(a == b for a, b in inside), f"the weight cache grew inside the block: {inside}"
    assert res[False][0] == res[True][0], (res[False][0], res[True][0])
    assert len(res[False][1]) == len(res[True][1])
    bad = [i for i, (a, b) in enumerate(zip(res[False][1], res[True][1])) if not torch.equal(a, b)]
    assert not bad, f"{len(bad)} of {len(res[True][1])} parameters differ between the one-stream and the two-stream schedule"
