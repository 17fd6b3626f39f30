"""-m gpu: the public mesh, shading, antialias, FLAME, texture-space and resize ops at EMPTY sizes and at sizes of one, forward and
backward, through the Python bindings — the boundary the kernel-level tables do not cover.

One table.  Every op has one base shape (B = 2, V = 5, F = 4, an 8 x 8 image, T = 4, C = 3, (n_shape, n_exp) = (3, 2),
(Ld, Ls, Lf) = (1, 2, 2), R = 3 rows, a 5 x 7 resize target); a row sets one of the op's dimensions to 0, or to 1, or is one of the
combinations B == 0 and F == 0, V == 0 and F == 0, B == 0 with one shared albedo.  V == 0 alone is not a row of an op that takes faces:
a face would name a vertex that does not exist (render._topology refuses it by name); with FLAME it is `vertex_ids=[]`
(flame.synthetic_flame_model needs a template, on the host).  Ba == 0 exists only together with B == 0.

Expected value of a row, outputs and the gradient to every input that can require one:
  * plain ops (vertex_normals, rasterize_attributes, rasterize_face_attributes, sh_shade, antialias, the FLAME layers,
    compute_texture_map, resize_image and _ResizeBwdFn): the float64 restatement the project has, on the CPU at the row's shape —
    test_gpu_render_grad's normals_ref and interp_ref (imported), shading_ref, antialias_ref
    and antialias_walk_ref (these three read the rasteriser's own face-index and depth buffers, as their modules do), flame_ref,
    flame_landmarks_ref, F.grid_sample and F.interpolate.  Where torch refuses the shape (grid_sample at T == 0, interpolate at
    C == 0) the expectation is written out: every tap lies outside, exact zeros; no plane, an empty tensor.
  * composed ops (render_condition, render_shaded_condition, rasterize_attributes_aa, soft_silhouette): the same public pieces
    called one by one, bit for bit; and in a row with an empty dimension the written-out definition — the background value of
    every channel (-1 after the [-1, 1] scaling of the conditions, 0 for a coverage) and zero gradients.
  Every result is compared by shape, dtype and device, and then by class: where the float32 run of the restatement reproduces the
  float64 run exactly (zeros, copies, empty tensors — every tensor of a row with an empty mesh, batch or image) the library must
  give those bits, torch.equal, no tolerance; elsewhere (rows of size one, the pose gradients of a layer without blend shapes)
  the rule of test_gpu_flame and test_gpu_shading holds, per tensor: err <= 4 * err32 + 2^-23, with their metrics — max|got - ref|
  / max|ref| for an output, Frobenius for a gradient — and err32 the float32 restatement's own err for that tensor.
  A row with a 0 among EXACT_DIMS must fall into the first class entirely.

Uninitialised memory must not pass by luck: before every call the caching allocator is POISONED.  The outputs, gradients and
scratch an op of this module allocates are a few KiB, so every one of its requests is served from the free blocks of the small
pool of the stream it runs on.  `poison` releases the cached segments nothing lives in, puts 1 MiB of room on the free list, and
then takes every free block of that stream off the list — requests of 1 MiB down to 512 bytes, each size until the allocator has
to reserve new memory — fills each to its end with NaN and frees them all: whatever block a later torch.empty is cut from, and
however it is split, it holds NaN throughout.  This relies on one thing, that a request the free list can serve reserves nothing
new; test_poison_reaches_torch_empty checks the outcome in a pool fragmented on purpose, allocating in the mixed order the
bindings do, and that nothing was served from memory the poison never saw.

The contract: no row may end in an error that says "null pointer" (the message for a caller's bug, not for an empty tensor);
rows with B == 0, F == 0, V == 0, C == 0, no landmarks or no blend shapes compute; a row may refuse — GifHipError or ValueError
naming the dimension — only where an image or texture extent is 0 and the C entry point documents "bad dims" for it.  Those rows
are REFUSES, and nothing else is.

FINDINGS, per row (at the parent commit -> now):
  vertex_normals           F0: "vertex_normals: null pointer"; V0_F0: "vertex_normals: bad dims" -> computed, exact zeros (mesh.hip:
                           B * V == 0 returns, F == 0 fills zeros, before the pointer checks); B0, B0_F0, ones: computed.
  rasterize_attributes,    B0, B0_F0, V0_F0: torch's "min(): Expected reduction dim" from standard_rasterize.to_image_space (an
  rasterize_face_attributes, empty z column has no minimum) -> computed; F0: computed (fixed one pull request ago); H0, W0: REFUSED
  render_condition,        by the rasteriser ("bad dims ... H=0"); the two conditions' F0 died in vertex_normals as above, and
  render_shaded_condition  B0_Ba1 in to_image_space.
  sh_shade                 H0, W0 with sh_coeff requiring a gradient: g_sh came back uninitialised (54 NaN of 54 under the poison)
                           -> exact zeros (shade.hip: memset when there is no pixel); T0: computed, exact zeros; B0 (Ba = 0 and 1),
                           Ba1, ones: computed.
  antialias, rasterize_attributes_aa, soft_silhouette (max_hops 0 and 2)
                           B0, V0_F0: to_image_space as above -> computed; C0 (antialias): refused "C >= 1" -> computed (an empty
                           image back, zero vertex gradient, no launch); F0: computed; H0, W0: REFUSED ("bad dims").
  FlameLayer, FlameLandmarkLayer
                           NS0_NE0 (no blend shapes at all), all six variants: numpy's "cannot reshape array of size 0 into shape
                           (0,newaxis)" from flame.joint_basis -> computed (the reshape names both extents).  Every other row
                           computed at the parent commit as well (B0, V0 through vertex_ids=[], one kind of blend shape or of
                           landmark missing, no landmark at all).
  compute_texture_map      C0: "texture_map: bad dims" -> computed (the mask alone); F0 (no valid texel): "texture_map: null
                           pointer"; V0_F0: "texture_map: bad dims" -> computed (mesh.hip: an empty texel list may be null, V may
                           be 0); B0: computed; H0, W0, T0: REFUSED ("bad dims", which now names the extents).
  resize_image, _ResizeBwdFn (bilinear and bicubic)
                           B0, C0: "resize: bad arguments" / "resize_bwd: bad arguments" -> computed (resize.hip: planes == 0
                           returns before the pointer test); H0, W0, HO0, WO0: REFUSED ("bad dims", which now names the extents).
Measured on an MI355X: the 293 rows take 4 s together, the slowest row 1.2 s (the first one: it loads the library).
"""
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import antialias_ref as aref
import antialias_walk_ref as wref
import flame_landmarks_ref as lref
import flame_ref
import shading_ref
import test_gpu_render_grad as rg  # (its float64 restatements of the normals and of the interpolation)

M_RULE, FLOOR = 4, 2.0 ** -23
SMALL_MAX = 1 << 20  # the caching allocator's largest small-pool request, in bytes
POISON_ROOM = SMALL_MAX  # bytes of free room made before each call; an op of this module allocates a few KiB
BASE = {"B": 2, "V": 5, "F": 4, "H": 8, "W": 8, "T": 4, "C": 3, "Ba": None, "NS": 3, "NE": 2, "Ld": 1, "Ls": 2, "Lf": 2, "HO": 5,
        "WO": 7}
IMAGE_EXTENTS = ("H", "W", "T", "HO", "WO")

VERTS = np.array([[0.05, -0.1, 0.2], [-0.7, -0.6, 0.5], [0.73, -0.65, 0.6], [0.7, 0.8, 0.4], [-0.8, 0.7, 0.7]])
FACES = np.array([[0, 1, 2], [0, 2, 3], [0, 3, 4], [0, 4, 1]], np.int64)


def rows_of(dims, extra=()):
    """{row name: {dimension: value}}: each dimension at 0 and at 1, the combinations, and the op's own extra rows"""
    rows = {}
    for k in dims:
        if k == "Ba":
            rows["Ba1"] = {"Ba": 1}
            continue
        if not (k == "V" and "F" in dims):  # (V == 0 alone: faces would name vertices that do not exist)
            rows[k + "0"] = {k: 0}
        rows[k + "1"] = {k: 1}
    if "B" in dims and "F" in dims:
        rows["B0_F0"] = {"B": 0, "F": 0}
    if "V" in dims and "F" in dims:
        rows["V0_F0"] = {"V": 0, "F": 0}
    if "Ba" in dims:
        rows["B0_Ba1"] = {"B": 0, "Ba": 1}
    if "NS" in dims:
        rows["NS0_NE0"] = {"NS": 0, "NE": 0}
        rows["NS1_NE0"] = {"NS": 1, "NE": 0}
    if "Ld" in dims:
        rows["Ld0_Ls0_Lf0"] = {"Ld": 0, "Ls": 0, "Lf": 0}
    rows.update(extra)
    return rows


def dims_of(row):
    d = dict(BASE, **row)
    if d["Ba"] is None:
        d["Ba"] = d["B"]
    return d


def gen(d, salt):
    return torch.Generator().manual_seed(1000 * salt + sum((i + 1) * v for i, v in enumerate(d.values())))


def mesh(d):
    """(vertices_ndc [B,V,3] float32, faces [F,3] int64): a fan of four faces around vertex 0, cut to F faces and V vertices (a face
    index past V wraps, so V = 1 gives degenerate faces), every sample shifted by a fraction of a pixel; no vertex on a pixel centre"""
    B, V, Fn = d["B"], d["V"], d["F"]
    v = np.stack([VERTS[:V] + b * np.array([0.11, -0.07, 0.0]) for b in range(B)]) if B else np.zeros((0, V, 3))
    f = FACES[:Fn] % max(V, 1)
    assert V > 0 or Fn == 0
    return torch.from_numpy(v.astype(np.float32)), torch.from_numpy(f.reshape(Fn, 3))


# ------------------------------------------------------------------------------------------------------------------ the harness
def poison(shapes):
    """NaN into EVERY free byte a request of the op's can be served from, on the current stream; returns the bytes filled.
    The op's requests are small (asserted: `shapes`, the outputs, gradients and scratch it will allocate, stay far below the room
    made here), so the caching allocator serves them from the free blocks it holds for this stream in its small pool, whichever it
    picks and however it splits them.  After the cached segments nothing lives in have been released and 1 MiB of room has been put
    on the free list, those blocks are taken off the list one by one: requests of 1 MiB, then 512 KiB, ... down to 512 bytes (the
    allocator's granule), each size repeated until a request makes the allocator reserve new memory — the sign that no free block
    of that size is left; that new segment is given back at once.  Every block taken is filled to its end and held until the list
    is empty, then all are freed.  Nothing here depends on which block the allocator picks or in which order."""
    need = sum(-(-4 * int(np.prod(t)) // 512) * 512 for t in shapes)
    assert need <= POISON_ROOM // 4, f"the op asks for {need} bytes: more room is needed than the poison makes"
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    room = torch.empty(POISON_ROOM // 4, device="cuda", dtype=torch.float32)  # (a small-pool request: at most 1 MiB)
    del room
    held, size = [], SMALL_MAX
    while size >= 512:
        before = torch.cuda.memory_reserved()
        t = torch.empty(size // 4, device="cuda", dtype=torch.float32)
        if torch.cuda.memory_reserved() != before:  # served from a new segment: the free list has no block of this size left
            del t
            torch.cuda.empty_cache()
            size //= 2
            continue
        held.append(t.fill_(float("nan")))
    filled = sum(4 * t.numel() for t in held)
    del held
    return filled


def leaves_on(x, device, dtype):
    return {k: t.to(device=device, dtype=dtype if t.is_floating_point() else None).requires_grad_(t.is_floating_point())
            for k, t in x.items()}


def backward(outs, leaves, ups):
    """{g_name: gradient} of sum_i <out_i, up_i> to every floating leaf; an output that carries no history gives zeros"""
    names = [k for k, t in leaves.items() if t.requires_grad]
    live = [(o, ups[k].to(o)) for k, o in outs.items() if o.is_floating_point() and o.requires_grad]
    if not live or not names:
        return {"g_" + k: torch.zeros_like(leaves[k]) for k in names}
    gs = torch.autograd.grad([o for o, _ in live], [leaves[k] for k in names], [u for _, u in live], allow_unused=True)
    return {"g_" + k: (torch.zeros_like(leaves[k]) if g is None else g) for k, g in zip(names, gs)}


def rel_max(got, ref):
    if ref.numel() == 0:
        return 0.0
    return ((got.double() - ref.double()).abs().max() / ref.double().abs().max().clamp_min(1e-300)).item()


def rel_fro(got, ref):
    return ((got.double() - ref.double()).norm() / ref.double().norm().clamp_min(1e-300)).item()


def compare(what, got, ref64, ref32, must_be_exact, gradient=False):
    """shape, dtype, device, then the value by its class (module docstring); returns 'exact' or the err / err32 figures.
    gradient: the Frobenius metric instead of the max metric."""
    assert got.is_cuda, f"{what}: on {got.device}"
    assert tuple(got.shape) == tuple(ref64.shape), f"{what}: shape {list(got.shape)}, expected {list(ref64.shape)}"
    want_dtype = torch.float32 if ref64.is_floating_point() else ref64.dtype
    assert got.dtype == want_dtype, f"{what}: dtype {got.dtype}, expected {want_dtype}"
    g = got.detach().cpu()
    if not ref64.is_floating_point():
        assert torch.equal(ref32, ref64), f"{what}: the restatement's own float32 and float64 runs disagree (a marginal input)"
        assert torch.equal(g, ref64), f"{what}: {int((g != ref64).sum())} of {g.numel()} elements differ"
        return "exact"
    nan = int(torch.isnan(g).sum())
    assert nan == 0, f"{what}: {nan} NaN of {g.numel()} elements (uninitialised memory under the poison)"
    if torch.equal(ref32.double(), ref64.double()):
        assert torch.equal(g.double(), ref64.double()), \
            f"{what}: expected exactly the reference's bits, max |diff| {(g.double() - ref64.double()).abs().max().item():.3e}"
        return "exact"
    assert not must_be_exact, f"{what}: a row with an empty dimension must give zeros, copies or empty tensors"
    metric = rel_fro if gradient else rel_max
    e, e32 = metric(g, ref64), metric(ref32, ref64)
    assert e <= M_RULE * e32 + FLOOR, f"{what}: err {e:.3e} > {M_RULE} * {e32:.3e} + 2^-23"
    return f"{e:.1e}/{e32:.1e}"


def call_gpu(op, d, x, aux):
    """the op on the device: (outs, grads); a "null pointer" anywhere fails the row"""
    try:
        leaves = leaves_on(x, "cuda", torch.float32)
        outs = op.gpu(d, leaves, aux)
        ups = {k: t for k, t in aux["ups"].items()}
        grads = backward(outs, leaves, {k: u.cuda() for k, u in ups.items()}) if op.grad else {}
        torch.cuda.synchronize()
        return outs, grads
    except Exception as e:  # noqa: BLE001 (every kind: the text decides)
        assert "null pointer" not in str(e), f"'null pointer' is for a caller's bug, not for an empty tensor: {e}"
        raise


def run_row(op, name):
    from gif_amd import _lib
    d = dims_of(op.rows[name])
    x = op.inputs(d)
    if (op.family, name) in REFUSES:
        zero = [k for k in IMAGE_EXTENTS if d[k] == 0]
        assert zero, "only an empty image or texture may be refused"
        with pytest.raises((_lib.GifHipError, ValueError)) as info:
            call_gpu(op, d, x, {"ups": {}, **op.refused_aux(d)})
        msg = str(info.value)
        assert "null pointer" not in msg and "bad dims" in msg, msg
        field = {"HO": "Ho", "WO": "Wo", "H": "H", "W": "W", "T": "T"}[zero[0]]
        assert any(f"{field}{suffix}=0" in msg for suffix in ("", "i")), f"the refusal does not name {field} = 0: {msg}"
        print(f"\n[empty sizes] {op.name} {name}: refused ({msg.split(': ', 1)[-1]})")
        return
    aux = {}
    if op.prepass is not None:
        aux.update(op.prepass(d, x))
    ref = op.reference(d, x, aux)
    torch.cuda.synchronize()
    poison([t.shape for t in ref[torch.float64].values()] + [t.shape for t in x.values()] + list(op.scratch(d)))
    outs, grads = call_gpu(op, d, x, aux)
    got = {**outs, **grads}
    assert sorted(got) == sorted(ref[torch.float64]), (sorted(got), sorted(ref[torch.float64]))
    exact_row = any(d[k] == 0 for k in EXACT_DIMS) and name not in op.inexact
    r64, r32 = ref[torch.float64], ref[torch.float32]
    report = [f"{k} {compare(f'{op.name} {name} {k}', got[k], r64[k], r32[k], exact_row, gradient=k in grads)}" for k in got]
    print(f"\n[empty sizes] {op.name} {name}: computed  " + "  ".join(report))


EXACT_DIMS = ("B", "V", "F", "H", "W", "T", "C")  # a 0 here leaves zeros, copies or empty tensors, nothing to round


class Op:
    """name; dims it has; inputs(d) -> {name: CPU float32 (differentiable) or integer tensor}; gpu(d, leaves, aux) and
    ref(d, leaves, dtype, aux) -> {name: output}; prepass(d, x) -> aux entries computed on the device (the rasteriser's buffers);
    scratch(d): shapes of the intermediates the binding allocates with torch.empty, for the poison."""
    grad, prepass, family = True, None, None
    inexact = ()  # rows with an empty dimension whose results are still rounded values

    def __init__(self, name, dims, extra_rows=(), **kw):
        self.name, self.dims = name, dims
        self.rows = rows_of(dims, dict(extra_rows))
        self.__dict__.update(kw)

    def scratch(self, d):
        return [(d["B"], d["F"], 3, 3), (d["B"], d["V"], 3), (d["B"], 3, d["H"], d["W"]), (d["B"], d["H"], d["W"], 3)]

    def refused_aux(self, d):
        return {}

    def reference(self, d, x, aux):
        """{float64: results, float32: results} of the restatement on the CPU (outputs and gradients); sets aux["ups"]"""
        ref = {}
        for dt in (torch.float64, torch.float32):
            leaves = leaves_on(x, "cpu", dt)
            outs = self.ref(d, leaves, dt, aux)
            if dt == torch.float64:
                aux.setdefault("ups", upstream(d, outs))  # (a caller may bring its own upstream gradients)
            grads = backward(outs, leaves, aux["ups"]) if self.grad else {}
            ref[dt] = {k: t.detach() for k, t in {**outs, **grads}.items()}
        return ref


def upstream(d, outs):
    g = gen(d, 77)
    return {k: torch.randn(tuple(o.shape), generator=g) for k, o in outs.items() if o.is_floating_point()}


class Composed(Op):
    """An op that is a composition of public pieces.  `call(d, leaves)` is the op and `pieces(d, leaves)` the same pieces one by one,
    both on the device.  The expectation is the pieces' result, bit for bit; over an empty mesh, batch or image it is the written-out
    definition instead: every channel of `channels` at the background `value`, and no gradient."""

    def reference(self, d, x, aux):
        if any(d[k] == 0 for k in ("B", "V", "F", "H", "W")):
            outs = {k: torch.full((d["B"], c, d["H"], d["W"]), self.value) for k, c in self.channels.items()}
            aux["ups"] = upstream(d, outs)
            res = {**outs, **{"g_" + k: torch.zeros_like(t) for k, t in x.items() if t.is_floating_point()}}
        else:
            leaves = leaves_on(x, "cuda", torch.float32)
            outs = self.pieces(d, leaves)
            aux["ups"] = upstream(d, outs)
            grads = backward(outs, leaves, {k: u.cuda() for k, u in aux["ups"].items()})
            res = {k: t.detach().cpu() for k, t in {**outs, **grads}.items()}
        return {torch.float64: res, torch.float32: res}

    def gpu(self, d, x, aux):
        return self.call(d, x)


# ---------------------------------------------------------------------------------------------------------------- render pieces
def raster_buffers(v32, f, h, w):
    """(pixel-space vertices [B,V,3] float32, tri, depth) on the CPU: what the library's rasteriser leaves for these vertices, through
    the drop-in module's public calls"""
    from gif_amd import standard_rasterize as sr
    v, f = v32.cuda(), f.cuda()
    B = v.shape[0]
    vi = sr.to_image_space(v, h, w)
    fv = sr.face_vertices(vi, f[None].expand(B, -1, -1))
    depth, tri, bary = sr.new_buffers(B, h, w, v.device)
    sr.standard_rasterize(fv, depth, tri, bary, h, w)
    return {"vi": vi.cpu(), "tri": tri.cpu(), "depth": depth.cpu()}


def pixels_ref(v, vi32, h, w):
    """pixel x, y [B,V,2] in v's dtype that carry exactly the float32 values the kernels see, with the exact derivative"""
    p = torch.stack([v[..., 0] * w / 2 + w / 2, v[..., 1] * h / 2 + h / 2], -1)
    return vi32[..., :2].to(v.dtype) + (p - p.detach())


def interp_ref(pix, corner_attr, faces, tri):
    """test_gpu_render_grad.interp_ref (barycentric interpolation inside each pixel's winning face -> [B,3,H,W]) for attributes given
    per face corner [B,F,3,3]: every face gets three vertices of its own, which carry its corners' positions and attributes"""
    B, Fn = pix.shape[0], faces.shape[0]
    own = torch.arange(3 * Fn).view(Fn, 3)
    return rg.interp_ref(pix[:, faces].reshape(B, 3 * Fn, 2), corner_attr.reshape(B, 3 * Fn, 3), own, tri)


def mesh_inputs(d, **more):
    v, f = mesh(d)
    return {"v": v, "f": f, **more}


def mesh_prepass(d, x):
    return raster_buffers(x["v"], x["f"], d["H"], d["W"])


def _normals():
    from gif_amd import render
    return Op("vertex_normals", ("B", "V", "F"), inputs=mesh_inputs,
              gpu=lambda d, x, aux: {"normals": render.vertex_normals(x["v"], x["f"])},
              ref=lambda d, x, dt, aux: {"normals": rg.normals_ref(x["v"], x["f"])})


def _raster():
    from gif_amd import render

    def inputs(d):
        return mesh_inputs(d, a=torch.rand(d["B"], d["V"], 3, generator=gen(d, 1)))

    def gpu(d, x, aux):
        img, mask = render.rasterize_attributes(x["v"], x["f"], x["a"], d["H"], d["W"])
        return {"img": img, "mask": mask}

    def ref(d, x, dt, aux):
        img = interp_ref(pixels_ref(x["v"], aux["vi"], d["H"], d["W"]), x["a"][:, x["f"]], x["f"], aux["tri"])
        return {"img": img, "mask": (aux["tri"] >= 0)[:, None]}

    return Op("rasterize_attributes", ("B", "V", "F", "H", "W"), inputs=inputs, gpu=gpu, ref=ref, prepass=mesh_prepass, family="raster")


def _face_attributes(per_sample):
    from gif_amd import shading

    def inputs(d):
        lead = (d["B"],) if per_sample else ()
        return mesh_inputs(d, fa=torch.rand(*lead, d["F"], 3, 3, generator=gen(d, 2)))

    def gpu(d, x, aux):
        img, mask = shading.rasterize_face_attributes(x["v"], x["f"], x["fa"], d["H"], d["W"])
        return {"img": img, "mask": mask}

    def ref(d, x, dt, aux):
        fa = x["fa"] if per_sample else x["fa"][None].expand(d["B"], -1, -1, -1)
        return {"img": interp_ref(pixels_ref(x["v"], aux["vi"], d["H"], d["W"]), fa, x["f"], aux["tri"]),
                "mask": (aux["tri"] >= 0)[:, None]}

    return Op("rasterize_face_attributes" + ("-per_sample" if per_sample else "-shared"), ("B", "V", "F", "H", "W"), inputs=inputs,
              gpu=gpu, ref=ref, prepass=mesh_prepass, family="raster")


def composed(name, dims, inputs, call, pieces, channels, value, family="raster"):
    return Composed(name, dims, inputs=inputs, call=call, pieces=pieces, channels=channels, value=value, family=family)


def _condition():
    from gif_amd import render

    def inputs(d):
        return mesh_inputs(d, tex=torch.rand(d["B"], d["V"], 3, generator=gen(d, 3)))

    def call(d, x):
        return {"cond": render.render_condition(x["v"], x["f"], x["tex"], d["H"], d["W"], straight_through=True)}

    def pieces(d, x):
        q = render._quantize_straight_through
        n = render.vertex_normals(x["v"], x["f"])
        nimg, _ = render.rasterize_attributes(x["v"], x["f"], n * 0.5 + 0.5, d["H"], d["W"])
        timg, _ = render.rasterize_attributes(x["v"], x["f"], x["tex"], d["H"], d["W"])
        return {"cond": torch.cat((q(timg) * 2 - 1, q(nimg) * 2 - 1), 1)}

    return composed("render_condition", ("B", "V", "F", "H", "W"), inputs, call, pieces, {"cond": 6}, -1.0)


def _shaded_condition():
    from gif_amd import render, shading

    def inputs(d):
        g = gen(d, 4)
        return mesh_inputs(d, uvs=torch.rand(d["F"], 3, 2, generator=g) * 1.6 - 0.8, alb=torch.rand(d["Ba"], 3, d["T"], d["T"], generator=g),
                           sh=torch.randn(d["B"], 9, 3, generator=g))

    def call(d, x):
        return {"cond": shading.render_shaded_condition(x["v"], x["f"], x["uvs"], x["alb"], x["sh"], d["H"], d["W"],
                                                        straight_through=True)}

    def pieces(d, x):
        q = render._quantize_straight_through
        n = render.vertex_normals(x["v"], x["f"])
        nimg, mask = render.rasterize_attributes(x["v"], x["f"], n * 0.5 + 0.5, d["H"], d["W"])
        fa = torch.cat((x["uvs"], torch.zeros_like(x["uvs"][..., :1])), 2)
        uv, _ = shading.rasterize_face_attributes(x["v"], x["f"], fa, d["H"], d["W"])
        shaded = shading.sh_shade(uv, nimg, mask, x["alb"], x["sh"], nrm_mul=2.0, nrm_add=-1.0)
        return {"cond": torch.cat((q(shaded.clamp(0, 1)) * 2 - 1, q(nimg) * 2 - 1), 1)}

    # (T0: an empty texture leaves the normal render as it is, so that row is compared with the pieces)
    return composed("render_shaded_condition", ("B", "V", "F", "H", "W", "T", "Ba"), inputs, call, pieces, {"cond": 6}, -1.0)


# --------------------------------------------------------------------------------------------------------------------- shading
def _sh_shade():
    from gif_amd import shading

    def inputs(d):
        B, Ba, H, W, T = d["B"], d["Ba"], d["H"], d["W"], d["T"]
        g = gen(d, 5)
        Tc = max(T, 1)  # texel position = an integer in [-1, T - 1] plus a fraction in [0.05, 0.95], as shading_ref.make_case does
        pos = torch.randint(-1, Tc, (B, 2, H, W), generator=g).double() + 0.05 + 0.9 * torch.rand(B, 2, H, W, generator=g, dtype=torch.float64)
        uv = torch.cat([((2 * pos + 1) / Tc - 1).float(), torch.zeros(B, 1, H, W)], 1)
        n = torch.randn(B, 3, H, W, generator=g, dtype=torch.float64)
        nrm = (n / n.norm(dim=1, keepdim=True) * (0.8 + 0.4 * torch.rand(B, 1, H, W, generator=g, dtype=torch.float64))).float()
        mask = torch.rand(B, 1, H, W, generator=g) < 0.7
        if mask.numel():
            mask[:, :, 0, 0] = True
        sh = torch.randn(B, 9, 3, generator=g)
        sh[:, 0] += 2.5
        return {"uv": uv, "nrm": nrm, "alb": torch.rand(Ba, 3, T, T, generator=g), "sh": sh, "mask": mask}

    def gpu(d, x, aux):
        return {"shaded": shading.sh_shade(x["uv"], x["nrm"], x["mask"], x["alb"], x["sh"])}

    def ref(d, x, dt, aux):
        if d["T"] == 0:  # grid_sample refuses an empty texture; every tap lies outside: exact zeros, and nothing to differentiate
            return {"shaded": torch.zeros(d["B"], 3, d["H"], d["W"], dtype=dt)}
        return {"shaded": shading_ref.sh_shade(x["uv"], x["nrm"], x["mask"], x["alb"], x["sh"])}

    return Op("sh_shade", ("B", "H", "W", "T", "Ba"), inputs=inputs, gpu=gpu, ref=ref, family="shade",
              scratch=lambda d: [(d["B"], 9, 3), (d["Ba"], 3, d["T"], d["T"]), (d["B"], 3, d["H"], d["W"])])


# ------------------------------------------------------------------------------------------------------------------- antialias
def _antialias(hops):
    from gif_amd import antialias as AA

    def inputs(d):
        return mesh_inputs(d, image=torch.rand(d["B"], d["C"], d["H"], d["W"], generator=gen(d, 6)))

    def restate(d, x, aux):
        fv = aref.face_vertices_ref(x["v"], aux["vi"], x["f"].numpy(), d["H"], d["W"])
        adj = aref.edge_adjacency_ref(x["f"].numpy())
        if hops:
            return wref.antialias_walk_ref(x["image"], aux["tri"], aux["depth"], fv, adj, hops)
        return aref.antialias_ref(x["image"], aux["tri"], aux["depth"], fv, adj)

    def ref(d, x, dt, aux):
        out, stats = restate(d, x, aux)
        if dt == torch.float64:  # pixels of marginal pairs (float32 may classify them differently) are left out, as in test_gpu_antialias
            aux["keep"] = (~stats["marginal_pixels"])[:, None]
            aux["blended"] = stats["blended"]
        else:
            assert stats["blended"] == aux["blended"]
        return {"out": out * aux["keep"].to(dt)}

    def gpu(d, x, aux):
        out = AA.antialias(x["image"], aux["tri"].cuda(), aux["depth"].cuda(), x["v"], x["f"], max_hops=hops)
        assert AA.edge_adjacency(x["f"]).cpu().long().tolist() == aref.edge_adjacency_ref(x["f"].cpu().numpy()).tolist()
        return {"out": out * aux["keep"].cuda().float()}

    def refused_aux(d):  # (the rasteriser refuses an empty image before it could leave buffers: empty ones of the right shape)
        hw = (d["B"], d["H"], d["W"])
        return {"tri": torch.full(hw, -1, dtype=torch.int32), "depth": torch.zeros(hw), "keep": torch.ones(hw, dtype=torch.bool)[:, None]}

    return Op(f"antialias-h{hops}", ("B", "V", "F", "H", "W", "C"), inputs=inputs, gpu=gpu, ref=ref, prepass=mesh_prepass,
              family="antialias", refused_aux=refused_aux,
              scratch=lambda d: [(d["B"], d["C"], d["H"], d["W"]), (d["B"], d["F"], 3, 3), (d["B"], d["V"], 3)])


def _raster_aa(hops):
    from gif_amd import antialias as AA
    from gif_amd import render

    def inputs(d):
        return mesh_inputs(d, a=torch.rand(d["B"], d["V"], 3, generator=gen(d, 7)))

    def call(d, x):
        img, cov = AA.rasterize_attributes_aa(x["v"], x["f"], x["a"], d["H"], d["W"], max_hops=hops)
        return {"img": img, "cov": cov}

    def pieces(d, x):
        img, mask, tri, depth = render._RasterizeColorsFn.apply(x["v"], x["a"], x["f"], d["H"], d["W"], True, "pieces")
        out = AA.antialias(torch.cat((img, mask.float()), 1), tri, depth, x["v"], x["f"], max_hops=hops)
        return {"img": out[:, :3], "cov": out[:, 3:]}

    return composed(f"rasterize_attributes_aa-h{hops}", ("B", "V", "F", "H", "W"), inputs, call, pieces, {"img": 3, "cov": 1}, 0.0,
                    family="antialias")


def _silhouette(hops):
    from gif_amd import antialias as AA

    def call(d, x):
        return {"cov": AA.soft_silhouette(x["v"], x["f"], d["H"], d["W"], max_hops=hops)}

    def pieces(d, x):
        b = raster_buffers(x["v"].detach().cpu(), x["f"].cpu(), d["H"], d["W"])
        tri, depth = b["tri"].cuda(), b["depth"].cuda()
        return {"cov": AA.antialias((tri >= 0)[:, None].float(), tri, depth, x["v"], x["f"], max_hops=hops)}

    return composed(f"soft_silhouette-h{hops}", ("B", "V", "F", "H", "W"), mesh_inputs, call, pieces, {"cov": 1}, 0.0, family="antialias")


# ----------------------------------------------------------------------------------------------------------------------- flame
def flame_parts(d, with_emb):
    """(model over the 5-vertex template, or the 1-vertex one; vertex_ids or None; embedding or None)"""
    from gif_amd import flame as fl
    V = d["V"]
    model = fl.synthetic_flame_model(VERTS[:max(V, 1)] * 0.1 if V == 1 else VERTS * 0.1, d["NS"], d["NE"], seed=3)
    ids = np.zeros(0, np.int64) if V == 0 else None
    emb = None
    if with_emb:
        faces = FACES % model.v_template.shape[0]
        L = (0, 0, 0) if V == 0 else (d["Ld"], d["Ls"], d["Lf"])  # (no vertex: no landmark can name one)
        emb = fl.synthetic_landmark_embedding(faces, L[0], L[1], L[2], 3, seed=5)
    return model, ids, emb


def flame_inputs(d):
    B = d["B"]
    g = gen(d, 8)
    r = lambda n, s: torch.randn(B, n, generator=g) * s
    neck = r(3, 0.05)
    if B:
        neck[:, 1] += torch.tensor([-0.5, 0.5]).repeat(B)[:B]  # yaw +28 / -28 degrees: far from the row thresholds (M = 1)
    return {"shape": r(d["NS"], 1.0), "exp": r(d["NE"], 1.0), "pose": r(6, 0.1), "neck": neck, "eye": r(6, 0.1)}


def flame_reference(d, x, dt, with_emb, only_landmarks):
    model, ids, emb = flame_parts(d, with_emb)
    c = flame_ref.constants(model, d["NS"], d["NE"], dt)
    verts = flame_ref.flame_vertices(c, *x.values())
    out = {} if only_landmarks else {"verts": verts if ids is None else verts[:, torch.from_numpy(ids)]}
    if emb is not None:
        t = lref.tables(emb, dt)
        Rw = lref.neck_rotation(c, x["pose"], x["neck"], x["eye"], t["yaw_joint"])
        if dt == torch.float64 and d["B"] and emb.dynamic_vid.shape[1]:
            y = torch.clamp(lref.yaw_degrees(Rw).detach(), max=1.0)
            assert ((y - 0.5) - torch.round(y - 0.5)).abs().min().item() >= 0.01, y  # the rows are decided (test_gpu_flame_landmarks)
        out["lmk2d"], out["lmk3d"], _ = lref.landmarks_of(t, verts, Rw)
    return out


def _flame(with_emb, grad):
    from gif_amd import flame as fl

    def gpu(d, x, aux):
        model, ids, emb = flame_parts(d, with_emb)
        layer = fl.FlameLayer(model, d["NS"], d["NE"], landmarks=emb, vertex_ids=ids).cuda()
        with torch.set_grad_enabled(grad):
            outs = layer(*x.values())
        return {k: t for k, t in zip(("verts", "lmk2d", "lmk3d"), outs) if t is not None}

    dims = ("B", "V", "NS", "NE") + (("Ld", "Ls", "Lf") if with_emb else ())
    return Op(f"FlameLayer-{'lmk' if with_emb else 'plain'}-{'grad' if grad else 'nograd'}", dims, inputs=flame_inputs, gpu=gpu,
              ref=lambda d, x, dt, aux: flame_reference(d, x, dt, with_emb, False), grad=grad, family="flame",
              scratch=flame_scratch)


def flame_scratch(d):
    KP = d["NS"] + d["NE"] + 36
    return [(d["B"], KP), (d["B"], 5, 12), (d["B"], d["V"], 3), (d["B"], d["Ld"] + d["Ls"] + d["Lf"], 3), (d["B"],)]


def _landmark_layer(grad):
    from gif_amd import flame as fl

    def gpu(d, x, aux):
        model, _, emb = flame_parts(d, True)
        layer = fl.FlameLandmarkLayer(model, emb, d["NS"], d["NE"]).cuda()
        with torch.set_grad_enabled(grad):
            l2d, l3d = layer(*x.values())
        return {"lmk2d": l2d, "lmk3d": l3d}

    return Op(f"FlameLandmarkLayer-{'grad' if grad else 'nograd'}", ("B", "NS", "NE", "Ld", "Ls", "Lf"), inputs=flame_inputs, gpu=gpu,
              ref=lambda d, x, dt, aux: flame_reference(d, x, dt, True, True), grad=grad, family="flame", scratch=flame_scratch)


# --------------------------------------------------------------------------------------------------------------- texture space
def texture_data(d):
    """every second texel of the T x T grid is valid (none without a face), on face t mod F with fixed barycentric weights"""
    T, Fn = d["T"], d["F"]
    _, faces = mesh(d)
    ys, xs = np.meshgrid(np.arange(T), np.arange(T), indexing="ij")
    valid = np.arange(0, T * T, 2) if Fn else np.zeros(0, np.int64)
    rng = np.random.RandomState(11)
    bc = rng.dirichlet([1, 1, 1], len(valid)).astype(np.float32).reshape(len(valid), 3)
    return {"x_coords": xs.reshape(-1), "y_coords": ys.reshape(-1), "valid_pixel_ids": valid,
            "valid_pixel_3d_faces": faces.numpy()[valid % max(Fn, 1)].reshape(len(valid), 3), "valid_pixel_b_coords": bc}


def _texture_map():
    from gif_amd.texture_space import FlameTextureSpace

    def inputs(d):
        g = gen(d, 9)
        v, _ = mesh(d)
        cam = torch.tensor([[0.9, 0.05, -0.03]]).repeat(d["B"], 1)
        return {"img": torch.rand(d["B"], d["C"], d["H"], d["W"], generator=g), "verts": v,
                "normals": torch.randn(d["B"], d["V"], 3, generator=g), "cam": cam}

    def gpu(d, x, aux):
        space = type("TextureSpace", (FlameTextureSpace,), {"TEX": d["T"]})(texture_data(d), None).cuda()
        # (the source image alone is differentiable: the mesh is data here)
        tex, mask = space.compute_texture_map(x["img"], x["verts"].detach(), x["normals"].detach(), camera_params=x["cam"].detach())
        return {"tex": tex, "mask": mask}

    def ref(d, x, dt, aux):
        """oracle/texture_ref.compute_texture_map, dtype-generic"""
        B, C, T = d["B"], d["C"], d["T"]
        td = texture_data(d)
        ids = td["valid_pixel_ids"]
        ty, tx = torch.from_numpy(td["y_coords"][ids]), torch.from_numpy(td["x_coords"][ids])
        f, bc = torch.from_numpy(td["valid_pixel_3d_faces"]).long(), torch.from_numpy(td["valid_pixel_b_coords"]).to(dt)
        verts, normals, cam = x["verts"].detach(), x["normals"].detach(), x["cam"].detach().view(-1, 1, 3)
        p3 = sum(verts[:, f[:, k], :] * bc[:, k][None, :, None] for k in range(3)) if len(ids) else verts.new_zeros(B, 0, 3)
        proj = cam[:, :, 0:1] * (p3[:, :, :2] + cam[:, :, 1:])
        grid = torch.zeros((B, T, T, 2), dtype=dt)
        grid[:, ty, tx, 0], grid[:, ty, tx, 1] = proj[:, :, 0], -proj[:, :, 1]
        n3 = sum(normals[:, f[:, k], 2] * bc[:, k][None] for k in range(3)) if len(ids) else normals.new_zeros(B, 0)
        mask = torch.zeros((B, 1, T, T), dtype=torch.bool)
        mask[:, 0, ty, tx] = n3 < 0
        if C == 0:  # (torch's backward of grid_sample is not defined without a plane)
            return {"tex": x["img"].new_zeros(B, 0, T, T) + x["img"].sum(), "mask": mask}
        return {"tex": F.grid_sample(x["img"], grid, mode="bilinear", padding_mode="zeros", align_corners=False), "mask": mask}

    # (no valid texel: every texel samples the image centre, as the reference's zero grid does — values, not zeros)
    return Op("compute_texture_map", ("B", "V", "F", "C", "H", "W", "T"), inputs=inputs, gpu=gpu, ref=ref, family="texture",
              inexact=("F0", "V0_F0"),
              scratch=lambda d: [(d["B"], d["C"], d["T"], d["T"]), (d["B"], d["C"], d["H"], d["W"])])


# ---------------------------------------------------------------------------------------------------------------------- resize
def _interpolate(x, size, mode):
    if x.shape[1] == 0:  # F.interpolate refuses a tensor without planes: the result has none either
        return x.new_zeros(x.shape[0], 0, *size) + x.sum()
    return F.interpolate(x, size=size, mode=mode, align_corners=False)


def _resize(mode):
    from gif_amd import data

    def inputs(d):
        return {"x": torch.rand(d["B"], d["C"], d["H"], d["W"], generator=gen(d, 10))}

    return Op(f"resize_image-{mode}", ("B", "C", "H", "W", "HO", "WO"), inputs=inputs, family="resize",
              gpu=lambda d, x, aux: {"y": data.resize_image(x["x"], (d["HO"], d["WO"]), mode)},
              ref=lambda d, x, dt, aux: {"y": _interpolate(x["x"], (d["HO"], d["WO"]), mode)},
              scratch=lambda d: [(d["B"], d["C"], d["HO"], d["WO"])])


def _resize_bwd(mode):
    from gif_amd import data

    def inputs(d):
        return {"gy": torch.randn(d["B"], d["C"], d["HO"], d["WO"], generator=gen(d, 11))}

    def ref(d, x, dt, aux):
        x0 = torch.zeros(d["B"], d["C"], d["H"], d["W"], dtype=dt, requires_grad=True)
        gx, = torch.autograd.grad(_interpolate(x0, (d["HO"], d["WO"]), mode), x0, x["gy"], create_graph=True)
        return {"gx": gx}

    return Op(f"_ResizeBwdFn-{mode}", ("B", "C", "H", "W", "HO", "WO"), inputs=inputs, ref=ref, family="resize",
              gpu=lambda d, x, aux: {"gx": data._ResizeBwdFn.apply(x["gy"], (d["H"], d["W"]), (d["HO"], d["WO"]), mode)},
              scratch=lambda d: [(d["B"], d["C"], d["H"], d["W"])])


def _ops():
    ops = [_normals(), _raster(), _face_attributes(False), _face_attributes(True), _condition(), _sh_shade(), _shaded_condition()]
    for hops in (0, 2):
        ops += [_antialias(hops), _raster_aa(hops), _silhouette(hops)]
    ops += [_flame(e, g) for e, g in itertools.product((False, True), (False, True))]
    ops += [_landmark_layer(False), _landmark_layer(True), _texture_map()]
    ops += [f(m) for f, m in itertools.product((_resize, _resize_bwd), ("bilinear", "bicubic"))]
    return {op.name: op for op in ops}


# {(op family, row): the entry point's documented refusal}: an image or texture extent of 0, nothing else
REFUSES = {
    ("raster", "H0"): "rasterize_colors: bad dims (H > 0)", ("raster", "W0"): "rasterize_colors: bad dims (W > 0)",
    ("antialias", "H0"): "rasterize / antialias: bad dims (H > 0)", ("antialias", "W0"): "rasterize / antialias: bad dims (W > 0)",
    ("texture", "H0"): "texture_map: bad dims (H > 0: there is no image to sample)", ("texture", "W0"): "texture_map: bad dims (W > 0)",
    ("texture", "T0"): "texture_map: bad dims (T > 0)",
    ("resize", "H0"): "resize: bad dims (Hi > 0)", ("resize", "W0"): "resize: bad dims (Wi > 0)",
    ("resize", "HO0"): "resize: bad dims (Ho > 0)", ("resize", "WO0"): "resize: bad dims (Wo > 0)",
}

OPS = _ops()  # (built at import: the bindings are plain Python until a call loads the library)
TABLE = [(name, row) for name, op in OPS.items() for row in op.rows]


@pytest.mark.gpu
@pytest.mark.parametrize("op,row", TABLE, ids=[f"{o}-{r}" for o, r in TABLE])
def test_row(op, row):
    run_row(OPS[op], row)


@pytest.mark.gpu
def test_poison_reaches_torch_empty():
    """The self-check of the poison, in a pool made dirty on purpose: a torch.empty of any small size, in the mixed order the bindings
    allocate in, reads NaN throughout and is served from the poisoned blocks (nothing new is reserved) — on the default stream and
    on a side stream."""
    shapes = [(2, 3, 8, 8), (2, 1, 8, 8), (2, 5, 3), (2, 4, 3, 3), (2, 9, 3), (1, 3, 4, 4), (3,), (2, 8, 8, 3), (2, 41), (2, 5, 12)]
    for stream in (torch.cuda.current_stream(), torch.cuda.Stream()):
        with torch.cuda.stream(stream):
            # fragment the pool: blocks of many sizes, every other one freed, the rest alive around the holes
            junk = [torch.zeros(128 * (1 + (7 * i) % 13), device="cuda") for i in range(64)]
            junk = junk[::2]
            filled = poison(shapes)
            assert filled >= POISON_ROOM
            reserved = torch.cuda.memory_reserved()
            fresh = [torch.empty(s, device="cuda") for _ in range(3) for s in shapes] + [torch.empty(s, device="cuda") for s in shapes[::-1]]
            torch.cuda.synchronize()
            assert all(torch.isnan(t).all() for t in fresh), str([int(torch.isnan(t).sum()) for t in fresh])
            assert torch.cuda.memory_reserved() == reserved, "served from memory the poison never saw"
            del fresh, junk


def test_refuses_holds_only_empty_images():
    """REFUSES names image and texture extents alone, every row of the table exists, and every op of the issue's list is there."""
    families = {"raster", "antialias", "texture", "resize", "shade", "flame", None}
    for (family, row), why in REFUSES.items():
        assert family in families and row[:-1] in IMAGE_EXTENTS and row.endswith("0") and "bad dims" in why
    assert len(TABLE) == len(set(TABLE)) == 293 and len(OPS) == 24
    assert not any(r in ("V0", "Ba0") for o, r in TABLE if "F" in OPS[o].dims or "Ba" in OPS[o].dims)
