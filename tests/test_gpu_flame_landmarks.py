"""The FLAME landmark kernels (gif_flame_landmarks_f32, gif_flame_landmarks_bwd_f32) and the layers on top of them against the
float64 restatement in tests/flame_landmarks_ref.py, on the same fp32-rounded constants and inputs.

The landmark step on given fp32 vertices and transforms (STEP):
  V in {3, 33, 257}; B in {1, 3, 33}; (R, Ld) in {(1, 0), (1, 1), (3, 1), (79, 17)}; Ls in {0, 1, 119}; Ld + Ls = 300 (more landmarks
  than a workgroup has lanes); every landmark on one face (V = 3: all contributions collide on three vertices); J = 5 and the
  chain (-1, 0, 1), yaw_joint = 1.  Two sizes beyond that list, for the backward's own thresholds: V = 2049 (three vertex ranges
  of 1024 per sample, the last one a single vertex) and Ld + Ls = 400 (1200 contributions: two staged tiles of 1024, five passes
  of 256 lanes).  Two chain lengths beyond J = 5 and 3: J = 1 (the yaw joint is the root, yaw_joint = 0) and J = 8 (kMaxJ).
  row      equal to the reference's;
  forward  per component |got - ref| <= 4 * 2^-24 * sum_i |bary_i v_i|           (three products, two adds, each rounded once);
  backward per element   |got - ref| <= (n + 1) * 2^-24 * sum |terms|, n = the number of contributions to the vertex (one product
           each, n - 1 adds); elements no landmark touches are exactly 0; two runs give identical bits.
Poses: the yaws of tests/test_flame_landmarks_cpu.py as global + neck rotations about y, then seeded general rotations.  For every
sample the test first asserts in float64 that min(yaw_deg, M) is at least 0.01 degrees from every half-integer (a precondition
on the inputs: the fp32 error of A is ~1e-5 degrees, so the float64 reference alone fixes the row).

The whole layer, parameters -> landmarks (LAYER), FlameLayer(landmarks=...) and FlameLandmarkLayer, no-grad and grad path, forward
and backward to the five parameter groups, with the rule of tests/test_gpu_flame.py:  err <= 4 * err32 + 2^-23,  err32 = the same
metric for the float32 restatement on the CPU (forward: max|got - ref| / max|ref| over both landmark outputs; backward: Frobenius,
per parameter group).
MEASURED err / err32 on an MI355X (`pytest -s` prints them; forward: no-grad path / grad path, FlameLayer then FlameLandmarkLayer;
backward: worst parameter group, FlameLayer then FlameLandmarkLayer):
  case             forward                      backward                             the two layers
  v33_b3_chain     0.75 / 0.75, 0.75 / 0.75     0.92 (neck), 1.02 (neck)             landmarks bit-equal, gradients not
  v257_b3_r1       0.85 / 0.85, 0.85 / 0.85     0.46 (eye), 0.43 (expression)        landmarks bit-equal, gradients not
  v257_b33_flame   0.68 / 0.70, 0.68 / 0.70     0.83 (expression), 0.79 (expression) landmarks bit-equal, gradients not
  v257_b3_j8       0.74 / 0.74, 0.74 / 0.74     0.46 (shape), 0.54 (shape)           landmarks bit-equal, gradients not
err32 itself: 8.5e-8 .. 2.8e-7 forward; 1.9e-7 .. 5.7e-7 for shape / expression and 8.3e-7 .. 3.1e-6 for the poses backward.
The landmark step: forward worst |err| / bound 0.56, backward 0.58 (0.01 with 136 contributions on one vertex); the J = 1 and J = 8
rows: forward 0.45 and 0.45, backward 0.40 and 0.46.
"""
import math
import os

import numpy as np
import pytest
import torch

import flame_landmarks_ref as lref
import flame_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
M_RULE, FLOOR = 4, 2.0 ** -23
GROUPS = ("shape_params", "expression_params", "pose_params", "neck_pose", "eye_pose")
FLAME, CHAIN = (-1, 0, 1, 1, 1), (-1, 0, 1)
ROOT_ONLY, EIGHT = (-1,), (-1, 0, 1, 1, 1, 0, 5, 2)  # the ends of the chain lengths the kernels take (J in 1..8)
YAWS = (0.0, -0.2, 12.3, 38.7, 45.0, -1.0, -12.3, -38.7, -45.0)
ROWS39 = (0, 0, 12, 39, 39, 40, 51, 78, 78)

# name: (V, B, R, Ld, Ls, parents)
STEP = {
    "v3_b1_r1_ld0_ls1": (3, 1, 1, 0, 1, FLAME),
    "v3_b3_r1_ld1_ls0": (3, 3, 1, 1, 0, CHAIN),
    "v33_b3_r3_ld1_ls119": (33, 3, 3, 1, 119, CHAIN),
    "v33_b33_r3_ld1_ls1": (33, 33, 3, 1, 1, FLAME),
    "v257_b33_r79_ld17_ls119": (257, 33, 79, 17, 119, FLAME),
    "v257_b3_r79_ld17_ls0": (257, 3, 79, 17, 0, CHAIN),
    "v257_b3_r79_ld17_ls283": (257, 3, 79, 17, 283, FLAME),      # Ld + Ls = 300
    "v3_b33_r79_ld17_ls119_one_face": (3, 33, 79, 17, 119, FLAME),  # every landmark on the same face
    "v2049_b3_r3_ld1_ls399": (2049, 3, 3, 1, 399, FLAME),         # three vertex ranges, two contribution tiles
    "v33_b3_r3_ld1_ls1_j1": (33, 3, 3, 1, 1, ROOT_ONLY),          # J = 1: the yaw joint is the root (yaw_joint = 0)
    "v257_b3_r79_ld17_ls119_j8": (257, 3, 79, 17, 119, EIGHT),    # J = 8: 96 floats of A per sample
}
# name: (V, B, (n_shape, n_exp), parents, (R, Ld, Ls, Lf))
LAYER = {
    "v33_b3_chain": (33, 3, (7, 5), CHAIN, (3, 1, 1, 2)),
    "v257_b3_r1": (257, 3, (7, 5), FLAME, (1, 1, 119, 0)),
    "v257_b33_flame": (257, 33, (7, 5), FLAME, (79, 17, 51, 68)),
    "v257_b3_j8": (257, 3, (7, 5), EIGHT, (79, 17, 51, 68)),
}


# seeds of the general rotations, picked so that the precondition on the yaws holds (24 random yaws all 0.01 degrees away from a
# half-integer: most seeds do, these keep 0.05 degrees)
POSE_SEED = {"v257_b33_r79_ld17_ls119": 7, "v3_b33_r79_ld17_ls119_one_face": 7, "v257_b33_flame": 7}


def faces_of(V, seed):
    if V == 3:
        return np.array([[0, 1, 2]])
    return np.random.RandomState(seed).randint(0, V, (2 * V, 3))


def pose_rows(B, seed, offset=0):
    """(global, neck) axis-angle [B,3] each: the prescribed yaws (from `offset` on) split 0.6 / 0.4 between two rotations about
    y (a rotation about y by -t has yaw t), then general rotations."""
    g = torch.Generator().manual_seed(seed)
    glob, neck = torch.zeros(B, 3, dtype=torch.float64), torch.zeros(B, 3, dtype=torch.float64)
    n = min(B, len(YAWS))
    yaws = [YAWS[(offset + i) % len(YAWS)] for i in range(n)]
    for i, t in enumerate(yaws):
        glob[i, 1], neck[i, 1] = -0.6 * math.radians(t), -0.4 * math.radians(t)
    if B > n:
        glob[n:] = torch.randn(B - n, 3, generator=g, dtype=torch.float64) * 0.4
        neck[n:] = torch.randn(B - n, 3, generator=g, dtype=torch.float64) * 0.4
    return glob, neck, yaws


def assert_rows_are_decided(yaw_deg, M):
    """The precondition: min(yaw_deg, M) is at least 0.01 degrees from every half-integer, for every sample."""
    y = torch.clamp(yaw_deg, max=float(M))
    dist = ((y - 0.5) - torch.round(y - 0.5)).abs()  # distance of y to the nearest k + 0.5
    assert torch.isfinite(yaw_deg).all() and dist.min().item() >= 0.01, (yaw_deg.tolist(), dist.min().item())


_cache = {}


def step_case(name):
    """Inputs and float64 results of a landmark-step case: computed once, shared, never modified."""
    if name in _cache:
        return _cache[name]
    from gif_amd import flame as fl
    V, B, R, Ld, Ls, parents = STEP[name]
    seed = 100 + V + B + R + Ls
    emb = fl.synthetic_landmark_embedding(faces_of(V, seed), n_dynamic=Ld, n_static=Ls, n_full=0, n_rows=R, seed=seed)
    emb.check_vertices(V)
    t = lref.tables(emb, torch.float64)
    J, M = len(parents), (R - 1) // 2
    yj = min(1, J - 1)  # the yaw joint: the neck, or the root of a one-joint chain (which then carries the whole prescribed yaw)
    g = torch.Generator().manual_seed(seed)
    verts = torch.randn(B, V, 3, generator=g)  # fp32: the kernel's input
    up = torch.randn(B, Ld + Ls, 3, generator=g)
    glob, neck, yaws = pose_rows(B, POSE_SEED.get(name, 0), offset=V + B)
    # A [B,J,12] in fp32: world rotations of the chain (global, neck, then seeded rotations) beside arbitrary translations
    rot = torch.randn(B, J, 3, generator=g, dtype=torch.float64) * 0.3
    rot[:, 0] = glob + neck if J == 1 else glob  # (both rotate about y: the sum is their product)
    if J > 1:
        rot[:, 1] = neck
    Rl = flame_ref.rodrigues(rot.reshape(B * J, 3)).view(B, J, 3, 3)
    GR = torch.stack([lref.world_rotation(Rl, parents, j) for j in range(J)], 1)
    A = torch.cat([GR, torch.randn(B, J, 3, 1, generator=g, dtype=torch.float64)], 3).reshape(B, J, 12).float()
    # float64 reference on the fp32 inputs
    Rw = A.double().view(B, J, 3, 4)[:, yj, :, :3]
    yaw = lref.yaw_degrees(Rw)
    assert_rows_are_decided(yaw, M)
    l2d, _, row = lref.landmarks_of(t, verts.double(), Rw)
    if M == 39:
        assert row[:len(yaws)].tolist() == [ROWS39[YAWS.index(y)] for y in yaws]
    # per-sample (vid, bary) [B,L,3] of the chosen rows, the forward's magnitudes and the backward's sums
    vid = torch.cat([t["dynamic_vid"][row], t["static_vid"][None].expand(B, -1, -1)], 1)
    bary = torch.cat([t["dynamic_bary"][row], t["static_bary"][None].expand(B, -1, -1)], 1)
    bi = torch.arange(B)[:, None, None]
    mag = (verts.double()[bi, vid] * bary[..., None]).abs().sum(2)            # [B,L,3]: sum_i |bary_i v_i|
    terms = bary[..., None] * up.double()[:, :, None, :]                        # [B,L,3 corners,3]
    idx = (bi.expand_as(vid), vid)
    zeros = lambda: torch.zeros(B, V, 3, dtype=torch.float64)
    g_ref = zeros().index_put_(idx, terms, accumulate=True)
    g_abs = zeros().index_put_(idx, terms.abs(), accumulate=True)
    count = zeros().index_put_(idx, torch.ones_like(terms), accumulate=True)
    out = {"tables": t, "verts": verts, "A": A, "up": up, "dims": (V, B, R, Ld, Ls, J), "yaw_joint": yj, "row": row, "lmk": l2d,
           "mag": mag, "g_ref": g_ref, "g_abs": g_abs, "count": count}
    _cache[name] = out
    return out


def run_step(c, need_grad=True):
    from gif_amd import flame as fl
    V, B, R, Ld, Ls, J = c["dims"]
    t = c["tables"]
    dev = lambda a, dt: a.to(device="cuda", dtype=dt).contiguous() if a.numel() else None
    verts = c["verts"].cuda().requires_grad_(need_grad)
    lmk, row = fl._FlameLandmarksFn.apply(verts, c["A"].cuda(), c["yaw_joint"], R, Ld, Ls, dev(t["dynamic_vid"], torch.int32),
                                          dev(t["dynamic_bary"], torch.float32), dev(t["static_vid"], torch.int32),
                                          dev(t["static_bary"], torch.float32))
    return verts, lmk, row


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(STEP))
def test_step_forward_and_row(name):
    c = step_case(name)
    _, lmk, row = run_step(c, need_grad=False)
    assert row.dtype == torch.int32 and row.cpu().long().tolist() == c["row"].tolist()
    assert lmk.shape == c["lmk"].shape
    err = (lmk.double().cpu() - c["lmk"]).abs()
    bound = 4 * U * c["mag"]
    worst = (err / bound.clamp_min(1e-300)).max().item()
    print(f"\n[landmarks fwd] {name}: max |err| {err.max().item():.2e}, worst err / bound {worst:.2f}")
    assert (err <= bound).all(), f"worst err / bound {worst:.3f}"


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(STEP))
def test_step_backward(name):
    c = step_case(name)
    runs = []
    for _ in range(2):
        verts, lmk, _ = run_step(c)
        runs.append(torch.autograd.grad(lmk, verts, c["up"].cuda())[0])
    got = runs[0].double().cpu()
    assert got.shape == c["g_ref"].shape
    err = (got - c["g_ref"]).abs()
    bound = (c["count"] + 1) * U * c["g_abs"]
    worst = (err / bound.clamp_min(1e-300))[c["count"] > 0].max().item()
    print(f"\n[landmarks bwd] {name}: up to {int(c['count'].max().item())} contributions to a vertex, max |err| "
          f"{err.max().item():.2e}, worst err / bound {worst:.2f}, untouched elements {(c['count'] == 0).float().mean().item():.2f}")
    assert (err <= bound).all(), f"worst err / bound {worst:.3f}"
    assert (runs[0].cpu()[c["count"] == 0] == 0).all()  # untouched: exact zeros
    assert torch.equal(runs[0], runs[1])


@pytest.mark.gpu
def test_no_landmarks_is_empty_and_backward_is_zero():
    from gif_amd import _lib
    from gif_amd import flame as fl
    lib = _lib.load()
    g = torch.full((2, 5, 3), 7.0, device="cuda")
    with torch.cuda.device(g.device):
        _lib.check(lib.gif_flame_landmarks_bwd_f32(None, None, None, None, None, None, g.data_ptr(), 2, 5, 1, 0, 0,
                                                   torch.cuda.current_stream().cuda_stream), "flame_landmarks_bwd")
    assert (g == 0).all()
    v = faces_of(33, 0)
    model = fl.synthetic_flame_model(body()[:33], 3, 2)
    empty = fl.synthetic_landmark_embedding(v, 0, 0, 0, 1)
    out = fl.FlameLayer(model, 3, 2, landmarks=empty).cuda()(torch.zeros(2, 3, device="cuda"))
    assert out[1].shape == (2, 0, 3) and out[2].shape == (2, 0, 3)


# ------------------------------------------------------------------------------------------------------------- whole layer
def body():
    return np.load(os.path.join(ROOT, "tests", "golden", "body_mesh.npz"))["vertices"].astype(np.float64) * 0.1


def rel_max(got, ref):
    return ((got.double().cpu() - ref).abs().max() / ref.abs().max()).item()


def rel_fro(got, ref):
    return ((got.double().cpu() - ref).norm() / ref.norm()).item()


def times(e, e32):
    return e / max(e32, 1e-30)


def layer_case(name):
    if name in _cache:
        return _cache[name]
    from gif_amd import flame as fl
    V, B, (ns, ne), parents, (R, Ld, Ls, Lf) = LAYER[name]
    seed = 200 + V + B
    model = fl.synthetic_flame_model(body()[:V], ns, ne, seed=seed, parents=parents)
    emb = fl.synthetic_landmark_embedding(faces_of(V, seed), Ld, Ls, Lf, R, seed=seed)
    g = torch.Generator().manual_seed(seed)
    r = lambda n, s: torch.randn(B, n, generator=g) * s
    glob, neck, _ = pose_rows(B, POSE_SEED.get(name, 0), offset=B)
    pose = torch.cat([glob.float(), r(3, 0.15)], 1)
    inputs = [r(ns, 1.0), r(ne, 1.0), pose, neck.float(), r(6, 0.15)]
    ups = (torch.randn(B, Ld + Ls, 3, generator=g), torch.randn(B, Lf, 3, generator=g))
    out = {"model": model, "emb": emb, "layer_args": (ns, ne), "inputs": inputs, "ups": ups}
    for dt in (torch.float64, torch.float32):
        c, t = flame_ref.constants(model, ns, ne, dt), lref.tables(emb, dt)
        x = [a.to(dt, copy=True).requires_grad_(True) for a in inputs]
        _, l2d, l3d, row = lref.flame_landmarks(c, t, *x)
        if dt == torch.float64:
            assert_rows_are_decided(lref.yaw_degrees(lref.neck_rotation(c, x[2], x[3], x[4], 1)).detach(), (R - 1) // 2)
        grads = torch.autograd.grad([l2d, l3d], x, [u.to(dt) for u in ups], allow_unused=True)
        out[dt] = (torch.cat([l2d, l3d], 1).detach(), [torch.zeros_like(a) if gr is None else gr.detach() for a, gr in zip(x, grads)], row)
    ref, ref_g, row = out[torch.float64]
    y32, y32_g, row32 = out[torch.float32]
    assert torch.equal(row, row32)
    out["err32"] = rel_max(y32, ref)
    out["err32_g"] = [rel_fro(a, b) if b.norm().item() else 0.0 for a, b in zip(y32_g, ref_g)]
    _cache[name] = out
    return out


def layers_of(c):
    from gif_amd import flame as fl
    return (fl.FlameLayer(c["model"], *c["layer_args"], landmarks=c["emb"]).cuda(),
            fl.FlameLandmarkLayer(c["model"], c["emb"], *c["layer_args"]).cuda())


def run_layer(layer, c, grad):
    x = [t.cuda().requires_grad_(grad) for t in c["inputs"]]
    if not grad:
        with torch.no_grad():
            out = layer(*x)
        return torch.cat(out[-2:], 1), None
    out = layer(*x)
    grads = torch.autograd.grad(list(out[-2:]), x, [u.cuda() for u in c["ups"]], allow_unused=True)
    return torch.cat(out[-2:], 1).detach(), grads


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(LAYER))
def test_layer_forward_matches_float64_reference(name):
    c = layer_case(name)
    ref = c[torch.float64][0]
    bound = M_RULE * c["err32"] + FLOOR
    outs, msgs = [], []
    for layer, label in zip(layers_of(c), ("FlameLayer", "FlameLandmarkLayer")):
        fast, slow = run_layer(layer, c, False)[0], run_layer(layer, c, True)[0]
        assert fast.shape == ref.shape and torch.isfinite(fast).all()
        e_fast, e_slow = rel_max(fast, ref), rel_max(slow, ref)
        msgs.append(f"{label}: no-grad path {e_fast:.2e} (x{times(e_fast, c['err32']):.2f}) grad path {e_slow:.2e} "
                    f"(x{times(e_slow, c['err32']):.2f})")
        assert e_fast <= bound, f"{label}, no-grad path: {e_fast:.3e} > {bound:.3e}"
        assert e_slow <= bound, f"{label}, grad path: {e_slow:.3e} > {bound:.3e}"
        outs.append((fast, slow))
    e_pair = max(rel_max(a, b.double().cpu()) for a, b in zip(*outs))
    equal = all(torch.equal(a, b) for a, b in zip(*outs))
    print(f"\n[landmarks layer fwd] {name}: err32 {c['err32']:.2e}  " + "  ".join(msgs) +
          f"  between the two layers {e_pair:.2e} ({'bit-equal' if equal else 'not bit-equal'})")
    assert e_pair <= bound, f"the two layers differ by {e_pair:.3e} > {bound:.3e}"


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(LAYER))
def test_layer_backward_matches_float64_autograd(name):
    c = layer_case(name)
    ref_g = c[torch.float64][1]
    msgs, bad, both = [], [], []
    for layer, label in zip(layers_of(c), ("FlameLayer", "FlameLandmarkLayer")):
        grads = run_layer(layer, c, True)[1]
        both.append(grads)
        for i, group in enumerate(GROUPS):
            if ref_g[i].norm().item() == 0:  # (the eye poses of a 3-joint chain move nothing)
                assert grads[i] is None or grads[i].abs().max().item() == 0
                continue
            e, e32 = rel_fro(grads[i], ref_g[i]), c["err32_g"][i]
            msgs.append(f"{label} {group} {e:.2e} (err32 {e32:.2e}, x{times(e, e32):.2f})")
            if not e <= M_RULE * e32 + FLOOR:
                bad.append(f"{label} {group}: {e:.3e} > {M_RULE * e32 + FLOOR:.3e}")
    equal = all(torch.equal(a, b) for a, b in zip(*both) if a is not None and b is not None)
    print(f"\n[landmarks layer bwd] {name}: " + "  ".join(msgs) + f"  the two layers' gradients: {'bit-equal' if equal else 'not bit-equal'}")
    assert not bad, "; ".join(bad)


# ------------------------------------------------------------------------------------------------------------------ wiring
@pytest.mark.gpu
def test_gradient_goes_to_verts_only_and_only_when_asked(monkeypatch):
    from gif_amd import flame as fl
    c = step_case("v33_b3_r3_ld1_ls119")
    V, B, R, Ld, Ls, J = c["dims"]
    t = c["tables"]
    tabs = [t["dynamic_vid"].int().cuda(), t["dynamic_bary"].float().cuda(), t["static_vid"].int().cuda(), t["static_bary"].float().cuda()]
    launches = []
    real = fl._launch_landmarks_bwd
    monkeypatch.setattr(fl, "_launch_landmarks_bwd", lambda *a: (launches.append(1), real(*a))[1])
    up = c["up"].cuda()
    # verts and A both require a gradient: one backward launch, A receives none
    verts, A = c["verts"].cuda().requires_grad_(True), c["A"].cuda().requires_grad_(True)
    lmk, row = fl._FlameLandmarksFn.apply(verts, A, 1, R, Ld, Ls, *tabs)
    assert lmk.requires_grad and not row.requires_grad
    lmk.backward(up)
    assert len(launches) == 1 and verts.grad is not None and A.grad is None
    # only A requires one: no backward launch, no gradient
    verts2 = c["verts"].cuda()
    lmk2, _ = fl._FlameLandmarksFn.apply(verts2, A, 1, R, Ld, Ls, *tabs)
    lmk2.backward(up)
    assert len(launches) == 1 and verts2.grad is None and A.grad is None
    assert torch.equal(lmk2, lmk)
    # a double backward raises
    verts3 = c["verts"].cuda().requires_grad_(True)
    lmk3, _ = fl._FlameLandmarksFn.apply(verts3, A, 1, R, Ld, Ls, *tabs)
    g, = torch.autograd.grad(lmk3, verts3, up.clone().requires_grad_(True), create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()


@pytest.mark.gpu
def test_layer_without_landmarks_is_unchanged_and_views_go_in():
    from gif_amd import flame as fl
    c = layer_case("v257_b33_flame")
    ns, ne = c["layer_args"]
    plain = fl.FlameLayer(c["model"], ns, ne).cuda()
    with_lmk, lmk_only = layers_of(c)
    x = [t.cuda() for t in c["inputs"]]
    for grad in (False, True):
        xs = [t.clone().requires_grad_(grad) for t in x]
        with torch.set_grad_enabled(grad):
            v, a, b = plain(*xs)
            v2, l2d, l3d = with_lmk(*xs)
        assert a is None and b is None
        assert torch.equal(v, v2)
        assert l2d.shape == (33, 68, 3) and l3d.shape == (33, 68, 3)
    # slices of one label tensor go in as they are, both layers
    fb = torch.cat(x[:3], 1)
    with torch.no_grad():
        want = with_lmk(*x[:3])
        got = with_lmk(fb[:, :ns], fb[:, ns:ns + ne], fb[:, ns + ne:])
        assert all(torch.equal(p, q) for p, q in zip(got, want))
        got = lmk_only(fb[:, :ns], fb[:, ns:ns + ne], fb[:, ns + ne:])
        assert len(got) == 2 and all(torch.equal(p, q) for p, q in zip(got, lmk_only(*x[:3])))


@pytest.mark.gpu
def test_project_landmarks_equals_the_reference_lines():
    from gif_amd import flame as fl
    g = torch.Generator().manual_seed(0)
    lmk = torch.randn(3, 68, 3, generator=g, dtype=torch.float64).cuda()
    cam = torch.randn(3, 3, generator=g, dtype=torch.float64).cuda()
    cam0 = cam.clone()
    # batch_orth_proj (model/mesh_and_3d_helpers.py:40-50), then the flip of plots/voca/generate_voca_gt.py:68-69
    c = cam.view(-1, 1, 3)
    want = c[:, :, 0:1] * torch.cat([lmk[:, :, :2] + c[:, :, 1:], lmk[:, :, 2:]], 2)
    want[:, :, 1:] *= -1
    got = fl.project_landmarks(lmk, cam)
    assert torch.equal(got, want) and torch.equal(cam, cam0)
