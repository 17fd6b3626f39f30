"""The autograd bindings of gif_amd/functional.py on the small graphs of tests/graph_cases.py, under every legal use of a graph, with
the real kernels on the device, against the float64 plain-torch restatement of the same graph on the CPU (the CPU tier runs the same
table over the ATen contracts: tests/test_graph_wiring_cpu.py).

Sign flips cannot loosen the bound: every case runs the seed written into graph_cases.CASES, whose float64 forward keeps every element
of every pre-activation at least 4 * TOL * R away from the kink of its leaky ReLU (TOL = 2e-6, the conv tolerance of
test_gpu_conv_routes.py; R = the operation on absolute values).  The tests assert that, search nothing, and leave no element and no
tensor out of any comparison.

Bound, per returned tensor, first and second order:   err = max|got - ref| / max|ref| <= M * err32 + 2^-23
with err32 the same metric for the fp32 run of the restatement on the CPU.  `pytest -s` prints err / err32 for every (graph, use,
tensor) as `[graph ...]` lines.  Pairs the table declares equal (U2 vs U1, U3 vs U1, U6 vs U1, inside vs outside
inputs_only_backward, a use run twice) must be bit-equal: the kernels sum in a fixed order.

MEASURED worst err / err32 per graph on an MI355X (f16x2, the default contraction mode; ports on / off do not differ in the worst):
  graph                first order (tensor, use: err / err32)         second order, U5 (tensor: err / err32)
  cba_chain             2.29 (b2, U1: 1.0e-07 / 4.4e-08)     1.30 (b1: 1.7e-07 / 1.3e-07)
  cba_chain_b1_none    14.76 (b2, U1: 4.6e-07 / 3.1e-08)     2.24 (b2: 2.7e-07 / 1.2e-07)
  cba_chain_b1_frozen   2.29 (b2, U1: 1.0e-07 / 4.4e-08)     1.00 (b2: 1.2e-07 / 1.2e-07)
  cba_chain_ident       3.51 (b1, U1: 2.7e-07 / 7.8e-08)     3.37 (b1: 3.6e-07 / 1.1e-07)
  cba_fan_out           2.32 (b2, U1: 1.3e-07 / 5.7e-08)     2.03 (b2: 3.2e-07 / 1.6e-07)
  resblock              2.44 (b1, U1: 2.1e-07 / 8.5e-08)     8.78 (b1: 2.9e-07 / 3.3e-08)
  styled_pair_32        5.31 (d2, U1: 1.3e-07 / 2.5e-08)     3.77 (s1: 2.6e-07 / 6.9e-08)
  styled_pair_16        3.50 (b2, U1: 1.8e-07 / 5.1e-08)     2.67 (b2: 2.4e-07 / 8.8e-08)
  styled_pair_c36       6.17 (br, U1: 1.2e-07 / 2.0e-08)     5.01 (br: 1.4e-07 / 2.9e-08)
  styled_up             3.49 (b1, U1: 2.6e-07 / 7.6e-08)     2.81 (s1: 2.9e-07 / 1.1e-07)
  to_rgb                1.78 (d1, U1: 1.7e-07 / 9.6e-08)     2.23 (b1: 1.3e-07 / 5.8e-08)
  demod_closed          2.28 (s1, U1: 1.2e-06 / 5.3e-07)     2.19 (b1: 1.5e-06 / 6.9e-07)
(styled_pair_* in bf16x3 and native: the same figures to the digit but for styled_pair_c36's second order, 4.83 in bf16x3 — at 8
contraction channels every mode runs the thin fp32 kernels, only the 36-channel forward of styled_pair_c36 changes family.)
M1 = 60 and M2 = 36: four times the worst ratio of each order.  The two ratios above 8 are bias gradients of 8 values whose fp32
restatement happens to land below half an ulp (err32 3.1e-8 and 3.3e-8 < 2^-24), so the ratio is mostly its denominator: the errors
themselves are 4.6e-7 and 2.9e-7, under 4 * 2^-23.  They are what the column-sum kernel must be expected to give: at 8 channels
colsum_stage1 (gif_amd/csrc/elementwise.hip) runs 128 row lanes that add 16 rows each and then folds the 128 lane sums in ONE sequential
chain (143 dependent additions, a random-walk error of about sqrt(143) * 2^-24 = 7e-7 of the partial sums) where torch adds in
a vectorised pairwise order.  Every tensor that is not a bias gradient measures below 5.4 (d2 of styled_pair_32); weights and
activations, whose err32 is 2e-7 .. 1e-6, measure below 1.9.

to_rgb_f16 (f16 activations, fp32 RGB output whose fp32 gradient re-enters the f16 kernels as f16; first order, 32x32, fused dot) is
measured against a restatement that rounds to half where gif_amd/csrc/conv_igemm.hip does: x, y1 and the gradients stored on them, the
scaled weights as packed, the modulation cast to half and multiplied into the half operand as a half (forward: s; adjoint: d), the
re-entering RGB gradient.  MEASURED worst err / err32 per tensor (err / err32):
  x 3.00 (1.2e-03 / 3.9e-04)   y1 18.7 (1.3e-03 / 6.8e-05)   w1 41.4 (2.9e-04 / 7.0e-06)   s1 105 (3.8e-04 / 3.6e-06)
  b1 113 (3.3e-05 / 3.0e-07)   d1 360 (5.8e-04 / 1.6e-06)    w2 785 (1.5e-04 / 1.9e-07)    s2 1143 (1.3e-04 / 1.1e-07)
MF16 = 4600, four times the worst.  The ratios are this large because err32 is not a yardstick of half arithmetic: the fp32 and the float64
restatement round the same values at the same places, so they differ only where a value sits within 1e-7 of a rounding boundary (a few
elements flip by one half ulp: 4e-4 on x, nothing on an 8-value sum), while the kernels differ from either by what the restatement does
not model — d1's gradient is taken from the stored, rounded y1 (act_inv_mul_reduce), the fused epilogues round in another order —
which is a half ulp per element everywhere, averaged down in the sums.  With M * err32 alone the bound on x and y1 would exceed 1, so
the case is ALSO held to the precision of the format: err <= 8 * 2^-11 = 3.9e-3, one unit roundoff of half for each of the at most eight
roundings between the loss and a leaf (RGB gradient, modulated operand, weights, stored gradient — per layer, two layers).  Measured
worst: 2.6 * 2^-11 (y1).
"""
import pytest
import torch

import graph_cases as G
from gpu_util import dev

pytestmark = pytest.mark.gpu

M1 = 60   # first order
M2 = 36   # second order (U5)
MF16 = 4600  # to_rgb_f16 (first order), against the restatement that rounds to half
FLOOR = 2.0 ** -23
HALF_CAP = 8 * 2.0 ** -11  # to_rgb_f16 only, on top of MF16 (see the docstring)
NAMES = [c.name for c in G.CASES]
MODES = [(n, "f16x2") for n in NAMES] + [(n, m) for n in NAMES if n.startswith("styled_pair") for m in ("bf16x3", "native")]
DIRECT = {"f16x2": 13, "bf16x3": 8, "native": 0}  # kernel families of test_gpu_conv_routes.py: LDS-DMA direct kernels; 5: the thin ones
THIN = 5


def conv(kind, t):
    return dev(t) if kind == "x" else t.cuda()


@pytest.fixture(autouse=True)
def _restore():
    from gif_amd import ops
    before, fuse = ops.get_fp32_mfma_mode(), ops.FUSE_GRAD
    yield
    ops.set_fp32_mfma_mode(before)
    ops.FUSE_GRAD = fuse
    ops.prof_enable(False)


@pytest.fixture(params=[True, False], ids=["ports_on", "ports_off"])
def fuse(request):
    """U7: every test runs with the activation ports on and off."""
    from gif_amd import ops
    ops.FUSE_GRAD = request.param
    return request.param


_err32, _u1 = {}, {}


def err32(name):
    """{use key: {tensor: err32}}: the fp32 restatement against the float64 one, once per graph."""
    if name not in _err32:
        r64, r32 = G.reference(name), G.reference(name, torch.float32)
        assert G.admissible(r64["acts"], G.BY_NAME[name].tol), f"{name}: the table's seed is not admissible"
        e = {"u1": {k: G.rel_err(r32["u1"][k], v) for k, v in r64["u1"].items()},
             "taps": {k: G.rel_err(r32["taps"][k], v) for k, v in r64["taps"].items()},
             "partial": {k: G.rel_err(r32["partial"][k], v) for k, v in r64["partial"].items()}}
        for t in r64["g"]:
            e["g", t] = {t: G.rel_err(r32["g"][t], r64["g"][t])}
            e["u5", t] = {k: G.rel_err(r32["u5"][t][k], v) for k, v in r64["u5"][t].items() if v is not None}
        _err32[name] = e
    return _err32[name]


def check(got, ref, e32, m, what):
    for k, r in ref.items():
        g = got[k]
        if r is None or r.abs().max() == 0:
            assert g is None or g.abs().max() == 0, f"{what}: {k} must have no gradient"
            continue
        assert g is not None, f"{what}: {k} has no gradient"
        assert torch.isfinite(g).all(), f"{what}: {k} NaN / Inf"
        e = G.rel_err(g, r)
        print(f"[graph {what}] {k}: err {e:.3e} err32 {e32[k]:.3e} ratio {e / max(e32[k], 1e-30):.2f}")
        assert e <= m * e32[k] + FLOOR, f"{what}: {k} err {e:.3e} > {m} * {e32[k]:.3e} + 2^-23"
        assert m != MF16 or e <= HALF_CAP, f"{what}: {k} err {e:.3e} > 8 * 2^-11"


def m1(name):
    return MF16 if G.BY_NAME[name].opts.get("f16") else M1


def same_bits(a, b, what):
    assert a.keys() == b.keys(), (what, sorted(a), sorted(b))
    for k in a:
        assert (a[k] is None) == (b[k] is None) and (a[k] is None or torch.equal(a[k], b[k])), \
            f"{what}: {k} differs" + ("" if a[k] is None or b[k] is None else f" (rel {G.rel_err(a[k], b[k]):.3e})")


def fresh_u1(name, fuse, mode="f16x2"):
    """U1 on a fresh graph, once per (graph, ports, mode): what the other uses must reproduce to the bit."""
    from gif_amd import ops
    key = (name, fuse, mode)
    if key not in _u1:
        assert ops.get_fp32_mfma_mode() == mode and ops.FUSE_GRAD == fuse
        _u1[key] = G.u1(G.BY_NAME[name], conv)
    return _u1[key]


# ---- U1 (+ the routes), in the default mode and, for the StyledConv pair, in bf16x3 and native ---------------------------------------
@pytest.mark.parametrize("name,mode", MODES)
def test_u1_full_pass_and_its_routes(name, mode, fuse, monkeypatch):
    from gif_amd import ops
    case = G.BY_NAME[name]
    ops.set_fp32_mfma_mode(mode)
    c = {"mask": 0, "dot": 0, "mul_reduce_scaled": 0}
    real_fuse, real_mr = ops.GradFuse, ops.mul_reduce

    class CountingFuse(real_fuse):
        def __init__(self, **kw):
            super().__init__(**kw)
            c["mask"] += self.mask_src is not None
            c["dot"] += self.dot_src is not None

    def mul_reduce(a, b, scale=None, want_scaled=False):
        c["mul_reduce_scaled"] += bool(want_scaled)
        return real_mr(a, b, scale=scale, want_scaled=want_scaled)

    monkeypatch.setattr(ops, "GradFuse", CountingFuse)
    monkeypatch.setattr(ops, "mul_reduce", mul_reduce)
    ops.prof_enable(True)
    for fam in range(18):
        ops.prof_read(fam)  # (reading clears a family's records)
    got = G.u1(case, conv)
    torch.cuda.synchronize()
    ran = {fam: n for fam in range(18) for n in [ops.prof_read(fam)[2]] if n}
    ops.prof_enable(False)
    monkeypatch.undo()
    print(f"[graph {name} {mode} {'on' if fuse else 'off'}] families {ran} counts {c}")
    check(got, G.reference(name)["u1"], err32(name)["u1"], m1(name), f"{name} U1 {mode}")
    # the routes: the real dot_fusable (1024 | H * W) decides between the fused data gradient and mul_reduce
    if not fuse:
        assert c["mask"] == 0 and c["dot"] == 0 and c["mul_reduce_scaled"] == (2 if case.route else 0), c
    else:
        assert c["mask"] >= case.masks and (case.masks > 0 or c["mask"] == 0), (c, case.masks)
        if case.route == "dot":
            assert c["dot"] == 2 and c["mul_reduce_scaled"] == 0, c
        if case.route == "mul_reduce":
            assert c["dot"] == 0 and c["mul_reduce_scaled"] == 2, c
    if name.startswith("styled_pair"):
        # 36 input channels: the first layer's forward (contraction 36 >= 24 / 32) leaves the thin, register-staged kernels for the LDS-DMA
        # kernel of the mode; everything else contracts over 8 channels and stays thin (family 1: the direct weight gradient)
        assert ran.get(THIN, 0) > 0 and ran.get(1, 0) == 3, ran
        assert ran.get(DIRECT[mode], 0) == (1 if name == "styled_pair_c36" else 0), (mode, ran)
    same_bits(G.u1(case, conv), got, f"{name} {mode}: the same pass on a second fresh graph")
    _u1.setdefault((name, fuse, mode), got)


# ---- U2 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,group", G.u2_pairs())
def test_u2_frozen_groups_leave_the_other_gradients_unchanged(name, group, fuse):
    case = G.BY_NAME[name]
    frozen = G.frozen_by_group(case, group)
    full = fresh_u1(name, fuse)
    got = G.u1(case, conv, frozen=frozen)
    assert got.keys() == full.keys() - set(frozen) and got
    same_bits(got, {k: full[k] for k in got}, f"{name} U2 {group} frozen vs U1")


# ---- U3 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["down", "up", "twice", "backward2"])
@pytest.mark.parametrize("name", NAMES)
def test_u3_an_earlier_pass_on_the_graph_leaves_nothing_behind(name, how, fuse):
    same_bits(G.u3(G.BY_NAME[name], conv, how), fresh_u1(name, fuse), f"{name} U3 {how} vs U1 on a fresh graph")


# ---- U4 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["retain_before", "hook_before", "retain_after", "hook_after"])
@pytest.mark.parametrize("name", NAMES)
def test_u4_a_watched_activation_sees_its_whole_gradient(name, how, fuse):
    case, ref, e = G.BY_NAME[name], G.reference(name), err32(name)
    seen, leaves = G.u4(case, conv, how)
    assert seen.keys() == ref["taps"].keys()
    check(seen, ref["taps"], e["taps"], m1(name), f"{name} U4 {how}")
    check(leaves, ref["u1"], e["u1"], m1(name), f"{name} U4 {how} leaves")


@pytest.mark.parametrize("name", NAMES)
def test_u4_autograd_grad_wrt_a_tagged_activation(name, fuse):
    """The documented limitation (functional.ActPort): ports on, autograd.grad(inputs=[y]) finds only what consumers outside the
    protocol sent to y (None under allow_unused where there are none); ports off, the whole gradient."""
    case, ref, e = G.BY_NAME[name], G.reference(name), err32(name)
    seen, leaves = G.u4(case, conv, "grad_inputs")
    same_bits(leaves, fresh_u1(name, fuse), f"{name} U4 grad_inputs leaves vs U1")
    for tap, kind in case.grad_inputs.items():
        kind = kind if fuse else "full"
        if kind == "none":
            assert seen[tap] is None, f"{name}: {tap} received a gradient outside its port"
        else:
            key = "taps" if kind == "full" else "partial"
            check({tap: seen[tap]}, {tap: ref[key][tap]}, e[key], m1(name), f"{name} U4 grad_inputs ({kind})")


# ---- U5, U6 ------------------------------------------------------------------------------------------------------------------------
def _targets():
    return [(c.name, t, "f16x2") for c in G.CASES for t in c.second] + \
           [(c.name, t, m) for c in G.CASES if c.name.startswith("styled_pair") for t in c.second for m in ("bf16x3", "native")]


@pytest.mark.parametrize("name,target,mode", _targets())
def test_u5_recorded_backward(name, target, mode, fuse):
    from gif_amd import ops
    case, ref, e = G.BY_NAME[name], G.reference(name), err32(name)
    ops.set_fp32_mfma_mode(mode)
    g0, got0, w0 = G.u5(case, conv, target, False)
    g1, got1, w1 = G.u5(case, conv, target, True)
    assert w0 > 0 and w1 == 0, (w0, w1)
    check({target: g0}, {target: ref["g"][target]}, e["g", target], M1, f"{name} U5 {mode} inner gradient")
    check(got0, ref["u5"][target], e["u5", target], M2, f"{name} U5 {mode} d|g|^2, g = dloss/d{target}")
    same_bits({target: g1}, {target: g0}, f"{name} U5: inner gradient inside vs outside inputs_only_backward")
    same_bits(got1, got0, f"{name} U5: second order inside vs outside inputs_only_backward")


@pytest.mark.parametrize("name,target", [(c.name, t) for c in G.CASES for t in c.second])
def test_u6_first_order_after_a_recorded_pass(name, target, fuse):
    _, got, _ = G.u5(G.BY_NAME[name], conv, target, then_full=True)
    same_bits(got, fresh_u1(name, fuse), f"{name} U6 vs U1 on a fresh graph")
