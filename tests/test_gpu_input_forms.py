"""-m gpu: the public mesh, shading, antialias, FLAME, texture-space and resize ops fed their inputs in other FORMS than dense float32
on the current stream — what the bindings' `.float()`, `.contiguous()`, `ctx.dtypes` and stream plumbing are for, and what only one
test touched so far (a FLAME label slice, held to "fewer than 1 % of the pixels differ").

The ops, shapes and inputs are those of tests/test_gpu_empty_sizes.py at the base row (B = 2, V = 5, F = 4, 8 x 8, T = 4, C = 3,
(n_shape, n_exp) = (3, 2), (Ld, Ls, Lf) = (1, 2, 2)).  Each form wraps every floating input (and, for the layout forms, the integer
and bool ones: faces, tri, mask) and is compared with the PLAIN call: the same values as dense float32 tensors on the current stream.
  f64          float64 inputs                                       plain: x.float()
  f16          float16 inputs                                       plain: x.half().float()
  transposed   last two axes swapped, copied, swapped back          (same values, permuted strides)
  sliced       the leading columns of a wider tensor                (same values, a longer row stride)
  expanded     sample 0 expanded over the batch, stride 0           plain: that batch, materialised
  side_stream  the call inside torch.cuda.stream(a fresh stream); every launch of the library is recorded (`recorded_launches`)
               and must have been handed that stream, and there must be at least one
Outputs must be bit-equal to the plain call's (after the cast to the output's dtype).  Gradients are taken at the LEAF behind the
form (the float64 / float16 tensor, the wide tensor, the one sample): they must have the leaf's shape and dtype — autograd refuses
another shape and casts another dtype itself, so this is asserted for completeness — and be bit-equal to the plain call's
gradient at the same leaf in dense float32, cast.  No form may reach _lib.marshal's refusal of a non-contiguous tensor.
Three results are accumulated with float atomics and have no bits to keep: the albedo gradient of sh_shade (and of
render_shaded_condition, where it is the same launch), the texture map's image gradient, and the adjoint of the resize
(gif_resize_bwd_f32: resize_image's gradient and _ResizeBwdFn's output; include/gif_hip.h and resize.hip say so: two calls on the
same dense input differ by an ulp in a few elements).  They are held to test_gpu_shading's rule against float64 instead,
err <= 4 * err32 + 2^-23 in the Frobenius norm, in every form.

FlameLayer's no-grad path hands gif_flame_joints_f32 raw addresses and row strides; its forms are listed in FLAME_FORMS: column
slices of one [B,159] label tensor, the same at B = 1, a stride-0 expanded row, a pose with column stride 2, and every one of the
32 subsets of the five parameter groups as None against explicit zeros.  Each is bit-equal to the dense call, and the grad path
agrees with it under test_gpu_flame's rule (err <= 4 * err32 + 2^-23, max metric).  What the entry point was handed is recorded as
well: a view with unit column stride goes in as its own address and row stride (no copy), the pose with column stride 2 as the
address of a dense copy with row stride 6 (the copy branch).
"""
import itertools

import pytest
import torch

import shading_ref
import test_gpu_empty_sizes as E

M_RULE, FLOOR = 4, 2.0 ** -23
ATOMIC = {"g_alb", "g_img"}  # (gradient names, wherever they occur)
ATOMIC_RESIZE = {"resize_image": "g_x", "_ResizeBwdFn": "gx"}  # (op family: the result gif_resize_bwd_f32 accumulates)


def is_atomic(opname, key):
    return key in ATOMIC or ATOMIC_RESIZE.get(opname.split("-")[0]) == key


# --------------------------------------------------------------------------------------------------------------------- the forms
class Form:
    """leaf(t): the tensor the caller owns for the dense float32 CPU tensor t (on the device); view(leaf): what goes into the op.
    floats_only: the form is a dtype and leaves integer and bool inputs alone."""
    floats_only = False

    def leaf(self, t):
        return t.cuda()

    def view(self, leaf, batched):
        return leaf


class Dtype(Form):
    floats_only = True

    def __init__(self, dtype):
        self.dtype = dtype

    def leaf(self, t):
        return t.cuda().to(self.dtype)


class Transposed(Form):
    def view(self, leaf, batched):
        if leaf.ndimension() < 2:
            return leaf
        v = leaf.transpose(-1, -2).contiguous().transpose(-1, -2)
        assert min(leaf.shape[-2:]) < 2 or not v.is_contiguous()
        return v


class Sliced(Form):
    def leaf(self, t):
        pad = torch.full(t.shape[:-1] + (3,), 7, dtype=t.dtype)
        return torch.cat([t, pad], -1).cuda()

    def view(self, leaf, batched):
        v = leaf[..., :leaf.shape[-1] - 3]
        assert not v.is_contiguous()
        return v


class Expanded(Form):
    def leaf(self, t):
        return t.cuda()

    def view(self, leaf, batched):
        if not batched:
            return leaf
        v = leaf[:1].expand(leaf.shape[0], *[-1] * (leaf.ndimension() - 1))
        assert v.stride(0) == 0
        return v


FORMS = {"f64": Dtype(torch.float64), "f16": Dtype(torch.float16), "transposed": Transposed(), "sliced": Sliced(), "expanded": Expanded(),
         "side_stream": Form()}
BATCHED = {"v", "a", "tex", "image", "uv", "nrm", "mask", "sh", "img", "verts", "normals", "cam", "x", "gy", "shape", "exp", "pose", "neck",
           "eye"}  # inputs with a leading batch axis ("fa" and "alb" may be shared: left alone by `expanded`)


def build(form, x, dense):
    """(leaves {name: device tensor, floating ones requiring a gradient}, inputs {name: what the op gets}).  dense: the plain
    call — the same leaves in float32, their views made contiguous."""
    leaves, inputs = {}, {}
    for k, t in x.items():
        if form.floats_only and not t.is_floating_point():
            leaf = t.cuda()
            leaves[k], inputs[k] = leaf, leaf
            continue
        leaf = form.leaf(t)
        if dense and leaf.is_floating_point():
            leaf = leaf.float()
        leaf.requires_grad_(leaf.is_floating_point())
        view = form.view(leaf, k in BATCHED)
        leaves[k], inputs[k] = leaf, (view.contiguous() if dense else view)
    return leaves, inputs


class recorded_launches:
    """Context: every call of a gif_* symbol through _lib.load() is recorded as (name, arguments) in .calls.  The bindings fetch the
    library with _lib.load() at every call, so swapping the loaded handle for a forwarding proxy sees all of them.
    before(name, args), if given, is called BEFORE the call is recorded and forwarded: a hook that raises keeps the arguments from ever
    reaching the library (tests/ops_forms.py: `checked`, `forbidden`)."""

    def __init__(self, before=None):
        self.before = before

    def __enter__(self):
        from gif_amd import _lib
        real, calls, before = _lib.load(), [], self.before

        class Proxy:
            def __getattr__(self, name):
                fn = getattr(real, name)
                if not name.startswith("gif_"):
                    return fn

                def call(*args):
                    if before is not None:
                        before(name, args)
                    calls.append((name, args))
                    return fn(*args)
                return call

        self._lib, self.real, self.calls = _lib, real, calls
        _lib._lib = Proxy()
        return self

    def __exit__(self, *exc):
        self._lib._lib = self.real

    def streams(self):
        """[(entry, the stream it was handed)] of the recorded launches: the entries whose last parameter is the stream"""
        from gif_amd import _lib
        out = []
        for name, args in self.calls:
            res, argtypes = _lib.PROTOTYPES[name]
            if res is _lib.c_int and argtypes and argtypes[-1] is _lib.P and not name.startswith("gif_f16_overflow"):
                out.append((name, args[-1]))
        return out


def run(op, d, form, x, aux, dense, stream=None):
    from gif_amd import _lib
    leaves, inputs = build(form, x, dense)
    torch.cuda.synchronize()
    try:
        if stream is not None:
            with recorded_launches() as rec, torch.cuda.stream(stream):
                outs = op.gpu(d, inputs, aux)
                grads = E.backward(outs, leaves, {k: u.cuda() for k, u in aux["ups"].items()}) if op.grad else {}
            handed = rec.streams()
            assert handed, "no launch of the library was recorded"
            wrong = [(n, s) for n, s in handed if s != stream.cuda_stream]
            assert not wrong, f"launched on another stream than the current one ({stream.cuda_stream}): {wrong}"
        else:
            outs = op.gpu(d, inputs, aux)
            grads = E.backward(outs, leaves, {k: u.cuda() for k, u in aux["ups"].items()}) if op.grad else {}
    except _lib.GifHipError as e:
        assert "not contiguous" not in str(e), f"_lib.marshal's refusal reached from a public op: {e}"
        raise
    torch.cuda.synchronize()
    return leaves, inputs, outs, grads


def values_of(form, x):
    """the dense float32 CPU tensors a form stands for (the reference's and the rasteriser pre-pass's inputs)"""
    _, inputs = build(form, x, dense=True)
    return {k: t.detach().cpu() for k, t in inputs.items()}


def atomic_bound(op, d, xv, aux, key):
    """(float64 gradient, err32) of one of the two atomically accumulated gradients, by the restatement"""
    if op.name == "render_shaded_condition":
        return shaded_condition_albedo(d, xv, aux)
    ref = op.reference(d, xv, dict(aux))
    r64, r32 = ref[torch.float64][key], ref[torch.float32][key]
    return r64, E.rel_fro(r32, r64)


def shaded_condition_albedo(d, xv, aux):
    """d cond / d albedo of render_shaded_condition in float64: the library's own pieces up to sh_shade's inputs and the upstream
    gradient that reaches the shaded image, then shading_ref's backward (the one launch that uses atomics)."""
    from gif_amd import render, shading
    x = E.leaves_on(xv, "cuda", torch.float32)
    n = render.vertex_normals(x["v"], x["f"])
    nimg, mask = render.rasterize_attributes(x["v"], x["f"], n * 0.5 + 0.5, d["H"], d["W"])
    fa = torch.cat((x["uvs"], torch.zeros_like(x["uvs"][..., :1])), 2)
    uv, _ = shading.rasterize_face_attributes(x["v"], x["f"], fa, d["H"], d["W"])
    shaded = shading.sh_shade(uv, nimg, mask, x["alb"], x["sh"], nrm_mul=2.0, nrm_add=-1.0)
    cond = render._quantize_straight_through(shaded.clamp(0, 1)) * 2 - 1
    g_shaded, = torch.autograd.grad(cond, shaded, aux["ups"]["cond"][:, :3].cuda())
    res = []
    for dt in (torch.float64, torch.float32):
        alb = xv["alb"].to(dt).requires_grad_(True)
        y = shading_ref.sh_shade(uv.detach().cpu().to(dt), nimg.detach().cpu().to(dt), mask.cpu(), alb, xv["sh"].to(dt), 2.0, -1.0)
        res.append(torch.autograd.grad(y, alb, g_shaded.cpu().to(dt))[0])
    return res[0], E.rel_fro(res[1], res[0])


TABLE = [(op, form) for op in E.OPS for form in FORMS]


@pytest.mark.gpu
@pytest.mark.parametrize("opname,formname", TABLE, ids=[f"{o}-{f}" for o, f in TABLE])
def test_form_gives_the_plain_calls_bits(opname, formname):
    op, form, d = E.OPS[opname], FORMS[formname], E.dims_of({})
    x = op.inputs(d)
    xv = values_of(form, x)
    aux = dict(op.prepass(d, xv)) if op.prepass is not None and not isinstance(op, E.Composed) else {}
    if isinstance(op, E.Composed):
        aux["ups"] = {k: torch.randn(d["B"], c, d["H"], d["W"], generator=E.gen(d, 77)) for k, c in op.channels.items()}
    else:
        op.reference(d, xv, aux)  # (sets the upstream gradients, and antialias's marginal-pixel mask)
    if formname == "f16":  # (a float16 output takes its upstream gradient in float16: give both calls one that float16 holds)
        aux["ups"] = {k: u.half().float() for k, u in aux["ups"].items()}
    leaves_p, _, outs_p, grads_p = run(op, d, form, x, aux, dense=True)
    stream = torch.cuda.Stream() if formname == "side_stream" else None
    leaves, inputs, outs, grads = run(op, d, form, x, aux, dense=False, stream=stream)
    if formname in ("transposed", "sliced", "expanded"):
        assert any(not t.is_contiguous() for t in inputs.values()), "the form left every input dense"
    report = []
    for k, o in outs.items():
        assert o.shape == outs_p[k].shape and o.is_cuda
        if is_atomic(opname, k):  # (_ResizeBwdFn's output IS the resize's accumulated adjoint)
            ref, e32 = atomic_bound(op, d, xv, aux, k)
            e = E.rel_fro(o.detach().float().cpu(), ref)
            report.append(f"{k} {e:.1e}/{e32:.1e}")
            assert e <= M_RULE * e32 + FLOOR, f"{opname} {formname} {k}: err {e:.3e} > {M_RULE} * {e32:.3e} + 2^-23"
            continue
        assert torch.equal(o, outs_p[k].to(o.dtype)), f"{opname} {formname} {k}: {int((o != outs_p[k].to(o.dtype)).sum())} elements differ"
    for k, g in grads.items():
        leaf = leaves[k[2:]]
        assert g.shape == leaf.shape and g.dtype == leaf.dtype and g.device == leaf.device, (k, g.shape, g.dtype)
        if is_atomic(opname, k):
            ref, e32 = atomic_bound(op, d, xv, aux, k)
            # the leaf may be wider than the input (sliced) or one sample (expanded): compare where the input lives
            got = g.detach().float().cpu()
            got = got[..., :ref.shape[-1]] if formname == "sliced" else got
            if formname == "expanded" and k[2:] in BATCHED:  # (the leaf's sample 0 collects the batch, the others nothing)
                assert not got[1:].any()
                got, ref = got[:1], ref.sum(0, keepdim=True)
            e = E.rel_fro(got, ref)
            report.append(f"{k} {e:.1e}/{e32:.1e}")
            slack = 2.0 ** -11 if formname == "f16" else 0.0  # (the gradient itself is rounded to float16: half an ulp of 2^-10)
            assert e <= M_RULE * e32 + FLOOR + slack, f"{opname} {formname} {k}: err {e:.3e} > {M_RULE} * {e32:.3e} + 2^-23"
            continue
        want = grads_p[k].to(g.dtype)
        assert torch.equal(g, want), f"{opname} {formname} {k}: {int((g != want).sum())} of {g.numel()} elements differ"
    print(f"\n[input forms] {opname} {formname}: {len(outs) + len(grads) - len(report)} of {len(outs) + len(grads)} results bit-equal  "
          + "  ".join(report))


# ------------------------------------------------------------------------------------------------------- FlameLayer, no-grad path
def _labels(B):
    g = torch.Generator().manual_seed(5)
    lbl = torch.randn(B, 159, generator=g)
    for lo, hi, s in ((150, 156, 0.1), (120, 126, 0.1), (140, 143, 0.05), (20, 32, 0.1)):  # the columns used as poses: small rotations
        lbl[:, lo:hi] *= s
    lbl[:, 141] += torch.tensor([-0.5, 0.5]).repeat(B)[:B]  # (neck, about y: yaw +28 / -28 degrees, far from the row thresholds)
    return lbl.cuda()


def _layer():
    from gif_amd import flame as fl
    d = E.dims_of({})
    model, _, emb = E.flame_parts(d, True)
    return fl.FlameLayer(model, d["NS"], d["NE"], landmarks=emb).cuda(), model, emb, d


def _call(layer, args, grad=False):
    if grad:
        args = [None if a is None else a.detach().requires_grad_(True) for a in args]  # (still the views they were)
    with torch.set_grad_enabled(grad):
        return [t.detach() for t in layer(*args)]


def _slices(lbl):
    return [lbl[:, 0:3], lbl[:, 100:102], lbl[:, 150:156], lbl[:, 140:143], lbl[:, 120:126]]


def _f_slices(B):
    lbl = _labels(B)
    args = _slices(lbl)
    assert all(a.stride(0) == 159 for a in args)
    return args


def _f_expanded(B):
    row = _labels(1)
    args = [a.expand(B, -1) for a in _slices(row)]
    assert all(a.stride(0) == 0 for a in args)
    return args


def _f_pose_stride2(B):
    lbl = _labels(B)
    args = _slices(lbl)
    args[2] = lbl[:, 20:32:2]
    assert args[2].shape == (B, 6) and args[2].stride(1) == 2
    return args


FLAME_FORMS = {"label_slices": lambda: _f_slices(2), "label_slices_b1": lambda: _f_slices(1), "expanded_row": lambda: _f_expanded(2),
               "pose_column_stride_2": lambda: _f_pose_stride2(2)}


def _flame_bound(model, emb, d, args):
    """4 * err32 + 2^-23 of test_gpu_flame for these parameters (max metric over vertices and landmarks together)"""
    import flame_landmarks_ref as lref
    import flame_ref
    res = {}
    for dt in (torch.float64, torch.float32):
        x = [a.detach().cpu().to(dt) for a in args]
        c, t = flame_ref.constants(model, d["NS"], d["NE"], dt), lref.tables(emb, dt)
        v, l2d, l3d, _ = lref.flame_landmarks(c, t, *x)
        res[dt] = torch.cat([v, l2d, l3d], 1)
    return res[torch.float64], M_RULE * E.rel_max(res[torch.float32], res[torch.float64]) + FLOOR


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(FLAME_FORMS))
def test_flame_nograd_path_takes_views_as_they_are(name):
    layer, model, emb, d = _layer()
    args = FLAME_FORMS[name]()
    dense = [a.contiguous() for a in args]
    assert all(a.is_contiguous() and a.stride(-1) == 1 for a in dense)
    want = _call(layer, dense)
    with recorded_launches() as rec:
        got = _call(layer, args)
    assert all(torch.equal(a, b) for a, b in zip(got, want)), name
    # what gif_flame_joints_f32 was handed: (address, row stride) of shape, expression, pose, neck, eye
    (joints,) = [a for n, a in rec.calls if n == "gif_flame_joints_f32"]
    for view, at in zip(args, (3, 6, 9, 11, 13)):
        ptr, ld = joints[at], joints[at + 1]
        if view.stride(1) == 1:
            assert (ptr, ld) == (view.data_ptr(), view.stride(0)), (name, at, "a view with unit column stride goes in as it is")
        else:
            assert ptr != view.data_ptr() and ld == view.shape[1], (name, at, "the copy branch: a dense copy, row stride = columns")
    assert (name == "pose_column_stride_2") == any(v.stride(1) != 1 for v in args)
    ref, bound = _flame_bound(model, emb, d, dense)
    slow = torch.cat(_call(layer, args, grad=True), 1)
    e_ref, e_pair = E.rel_max(torch.cat(got, 1).cpu(), ref), E.rel_max(slow.cpu(), torch.cat(got, 1).double().cpu())
    print(f"\n[input forms] FlameLayer {name}: no-grad path bit-equal to the dense call; err {e_ref:.2e}, grad path vs no-grad path "
          f"{e_pair:.2e}, bound {bound:.2e}")
    assert e_ref <= bound and e_pair <= bound


@pytest.mark.gpu
def test_flame_none_is_explicit_zeros_for_every_subset():
    """each of the 32 subsets of (shape, expression, pose, neck, eye) given as None: the bits of explicit zeros, both paths"""
    layer, model, emb, d = _layer()
    full = _f_slices(2)
    for grad in (False, True):
        for subset in itertools.product((False, True), repeat=5):
            if all(subset):
                continue  # (no argument at all: the layer then makes a batch of one)
            args = [None if drop else a for a, drop in zip(full, subset)]
            zeros = [torch.zeros_like(a) if drop else a for a, drop in zip(full, subset)]
            got, want = _call(layer, args, grad), _call(layer, zeros, grad)
            assert all(torch.equal(a, b) for a, b in zip(got, want)), (grad, subset)
    got = _call(layer, [None] * 5)
    want = _call(layer, [torch.zeros(1, n, device="cuda") for n in (d["NS"], d["NE"], 6, 3, 6)])
    assert got[0].shape[0] == 1 and all(torch.equal(a, b) for a, b in zip(got, want))


@pytest.mark.gpu
def test_flame_nograd_path_casts_other_dtypes():
    layer, model, emb, d = _layer()
    dense = [a.contiguous().half().float() for a in _f_slices(2)]
    want = _call(layer, dense)
    for dt in (torch.float64, torch.float16):
        got = _call(layer, [a.to(dt) for a in dense])
        assert all(torch.equal(a, b) and a.dtype == torch.float32 for a, b in zip(got, want)), dt


def test_every_op_of_the_empty_size_table_has_every_form():
    assert len(TABLE) == len(E.OPS) * 6 and set(ATOMIC) == {"g_alb", "g_img"}
    assert is_atomic("resize_image-bicubic", "g_x") and is_atomic("_ResizeBwdFn-bilinear", "gx")
    assert not is_atomic("_ResizeBwdFn-bilinear", "g_gy")
