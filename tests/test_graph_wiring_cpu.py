"""CPU tier: the autograd bindings of gif_amd/functional.py on the small graphs of tests/graph_cases.py, under every legal use of a
graph, against the float64 plain-torch restatement of the same graph.  Every HIP launch is replaced by its ATen contract
(tests/cpu_ops.py), so both sides are ATen and every gradient is held to max|got - ref| <= 1e-5 * max|ref| (the bound
test_cpu_wiring.py uses for the forward); results the table declares equal must be bit-equal.

The whole-model tests exercise one use of a graph: a single full backward.  The activation ports keep state outside autograd (the
`parts` lists, gradients delivered on an alias of y), which other legal uses can break:
  U1 full pass            U2 requires_grad off on groups of leaves       U3 a partial / repeated pass on a retained graph first
  U4 retain_grad / hooks / autograd.grad on a tagged activation          U5 create_graph (R1, path length), in and out of
  inputs_only_backward    U6 a first-order pass after a recorded one     U7 all of it with the ports off (ops.FUSE_GRAD = False).
Against functional.py as it was before the fixes that came with this file, 58 of the 446 tests here fail, with the ports on only:
  U3 [*-down], 9 graphs (chain, fan-out, ResBlock, every StyledConv graph): the producer's bias gradient exactly doubled, e.g.
      "cba_chain U3 down: b1 rel err 1.000e+00 > 1e-05", "styled_up U3 down: br rel err 1.000e+00 > 1e-05" (stale `parts`);
  U4 retain / hook, before and after, 44 cases: "to_rgb U4 hook_after: y1 has no gradient", "styled_pair_c36 U4 retain_before: r has no
      gradient" (the gradient went to the alias only);
  U2 [*-sd], 5 StyledConv graphs: "GradFuse: nothing to fuse" — with s and d frozen and the input a leaf, the modulated data gradient
      built a GradFuse with neither mask nor dot product, which ops refuses (cpu_ops.py now refuses it the same way)."""
import pytest
import torch

import cpu_ops
import graph_cases as G
from oracle import stylegan2_ref as R

NAMES = [c.name for c in G.CPU_CASES]  # (all but the f16 variant of ToRGB: the contracts are fp32; its seed and restatement are checked here)
TOL = 1e-5


@pytest.fixture(params=[True, False], ids=["ports_on", "ports_off"])
def fuse(request, monkeypatch):
    """U7: every test runs with the activation ports on and off."""
    from gif_amd import ops
    cpu_ops.install(monkeypatch)
    monkeypatch.setattr(ops, "FUSE_GRAD", request.param)
    return request.param


@pytest.fixture
def counts(monkeypatch, fuse):
    from gif_amd import ops
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
    return c


def check(got, ref, what):
    """Every tensor of got within TOL of the float64 reference; a leaf the reference gives no (or a zero) gradient gets none or zero."""
    assert got.keys() == ref.keys(), (what, sorted(got), sorted(ref))
    for k, r in ref.items():
        g = got[k]
        if r is None or r.abs().max() == 0:
            assert g is None or g.abs().max() == 0, f"{what}: {k} must have no gradient"
            continue
        assert g is not None, f"{what}: {k} has no gradient"
        e = G.rel_err(g, r)
        assert e <= TOL, f"{what}: {k} rel err {e:.3e} > {TOL:.0e}"


def same_bits(a, b, what):
    assert a.keys() == b.keys(), (what, sorted(a), sorted(b))
    for k in a:
        assert (a[k] is None) == (b[k] is None) and (a[k] is None or torch.equal(a[k], b[k])), \
            f"{what}: {k} differs" + ("" if a[k] is None or b[k] is None else f" (rel {G.rel_err(a[k], b[k]):.3e})")


# ---- the restatement and the table themselves ------------------------------------------------------------------------------------
def test_fir_restatement_is_the_oracles_upfirdn2d():
    x = torch.randn(2, 3, 9, 10, dtype=torch.float64, generator=torch.Generator().manual_seed(0))
    for down, pad in ((1, (2, 2)), (2, (1, 1)), (1, (1, 1)), (2, (2, 1))):
        assert torch.equal(G._fir(x, G.FIR.double(), down, pad), R.upfirdn2d(x, G.FIR.double(), 1, down, pad))


@pytest.mark.parametrize("name", [c.name for c in G.CASES])
def test_table_seed_is_the_first_admissible_one(name):
    case = G.BY_NAME[name]
    assert G.find_seed(case, case.seed // 100 * 100) == case.seed
    ref = G.reference(name)
    assert G.admissible(ref["acts"], case.tol) and len(ref["acts"]) >= 1
    assert all(v is not None and v.abs().max() > 0 for v in ref["u1"].values()), "every leaf reaches the loss"


@pytest.mark.parametrize("name", NAMES)
def test_forward_matches_the_restatement(name, fuse):
    case = G.BY_NAME[name]
    got, ref = G.Graph(case), G.Graph(case, lambda k, t: t.double(), ref=True)
    for a, b in zip(got.outs, ref.outs):
        assert G.rel_err(a, b) <= TOL
    assert got.taps.keys() == ref.taps.keys() == case.grad_inputs.keys()


# ---- U1 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_u1_full_pass_and_its_routes(name, fuse, counts):
    case = G.BY_NAME[name]
    got = G.u1(case)
    check(got, G.reference(name)["u1"], f"{name} U1")
    if not fuse:
        assert counts["mask"] == 0 and counts["dot"] == 0, counts
        assert counts["mul_reduce_scaled"] == (2 if case.route else 0), counts
    else:
        assert counts["mask"] >= case.masks and (case.masks > 0 or counts["mask"] == 0), (counts, case.masks)
        if case.route == "dot":
            assert counts["dot"] == 2 and counts["mul_reduce_scaled"] == 0, counts
        if case.route == "mul_reduce":
            assert counts["dot"] == 0 and counts["mul_reduce_scaled"] == 2, counts
    same_bits(G.u1(case), got, f"{name}: the same pass on a second fresh graph")


def test_ports_on_and_off_agree_to_the_bit_where_the_routes_coincide(monkeypatch):
    """On this tier the epilogue fusions and the stand-alone passes are the same ATen expressions in the same order, except where a
    gradient that autograd would add from two tensors is added inside a launch instead (fan-out: three consumers summed in another order;
    ResBlock: the skip gradient as the data gradient's residual), so every other graph must not differ by a bit."""
    from gif_amd import ops
    cpu_ops.install(monkeypatch)
    for case in G.CPU_CASES:
        if case.name in ("cba_fan_out", "resblock"):
            continue
        out = {}
        for on in (True, False):
            monkeypatch.setattr(ops, "FUSE_GRAD", on)
            out[on] = G.u1(case)
        same_bits(out[True], out[False], f"{case.name}: ports on vs off")


# ---- U2 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,group", G.u2_pairs(G.CPU_CASES))
def test_u2_frozen_groups_leave_the_other_gradients_unchanged(name, group, fuse):
    case = G.BY_NAME[name]
    frozen = G.frozen_by_group(case, group)
    full = G.u1(case)
    got = G.u1(case, frozen=frozen)
    assert got.keys() == full.keys() - set(frozen) and got
    same_bits(got, {k: full[k] for k in got}, f"{name} U2 {group} frozen vs U1")
    check(got, {k: G.reference(name)["u1"][k] for k in got}, f"{name} U2 {group}")


# ---- U3 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["down", "up", "twice", "backward2"])
@pytest.mark.parametrize("name", NAMES)
def test_u3_an_earlier_pass_on_the_graph_leaves_nothing_behind(name, how, fuse):
    case = G.BY_NAME[name]
    got = G.u3(case, None, how)
    check(got, G.reference(name)["u1"], f"{name} U3 {how}")
    same_bits(got, G.u1(case), f"{name} U3 {how} vs U1 on a fresh graph")


# ---- U4 ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["retain_before", "hook_before", "retain_after", "hook_after"])
@pytest.mark.parametrize("name", NAMES)
def test_u4_a_watched_activation_sees_its_whole_gradient(name, how, fuse):
    """retain_grad() or a hook, set before the consumers are built (they decline the port) or after (they check again when their
    backward runs): the gradient seen is the float64 one, and the leaves' gradients are those of U1."""
    case, ref = G.BY_NAME[name], G.reference(name)
    seen, leaves = G.u4(case, None, how)
    check(seen, ref["taps"], f"{name} U4 {how}")
    check(leaves, ref["u1"], f"{name} U4 {how} leaves")


@pytest.mark.parametrize("name", NAMES)
def test_u4_autograd_grad_wrt_a_tagged_activation(name, fuse):
    """The documented limitation (functional.ActPort): with the ports on, autograd.grad(inputs=[y]) finds only what consumers outside the
    protocol sent to y — nothing (None under allow_unused) where there are none; with the ports off, the whole gradient."""
    case, ref = G.BY_NAME[name], G.reference(name)
    seen, leaves = G.u4(case, None, "grad_inputs")
    check(leaves, ref["u1"], f"{name} U4 grad_inputs leaves")
    for tap, kind in case.grad_inputs.items():
        kind = kind if fuse else "full"
        if kind == "none":
            assert seen[tap] is None, f"{name}: {tap} received a gradient outside its port"
        else:
            check({tap: seen[tap]}, {tap: ref["taps" if kind == "full" else "partial"][tap]}, f"{name} U4 grad_inputs ({kind})")


# ---- U5, U6 ------------------------------------------------------------------------------------------------------------------------
def _targets():
    return [(c.name, t) for c in G.CPU_CASES for t in c.second]


@pytest.mark.parametrize("inputs_only", [False, True], ids=["all_inputs", "inputs_only"])
@pytest.mark.parametrize("name,target", _targets())
def test_u5_recorded_backward(name, target, inputs_only, fuse):
    case, ref = G.BY_NAME[name], G.reference(name)
    g, got, wgrads = G.u5(case, None, target, inputs_only)
    check({target: g}, {target: ref["g"][target]}, f"{name} U5 inner gradient")
    check(got, ref["u5"][target], f"{name} U5 d |g|^2 / d leaves, g = d loss / d {target}")
    assert (wgrads == 0) if inputs_only else (wgrads > 0), wgrads
    if inputs_only:
        g0, got0, _ = G.u5(case, None, target, False)
        same_bits({target: g}, {target: g0}, f"{name} U5: inner gradient inside vs outside inputs_only_backward")
        same_bits(got, got0, f"{name} U5: second order inside vs outside inputs_only_backward")


@pytest.mark.parametrize("name,target", _targets())
def test_u6_first_order_after_a_recorded_pass(name, target, fuse):
    case = G.BY_NAME[name]
    _, got, _ = G.u5(case, None, target, then_full=True)
    check(got, G.reference(name)["u1"], f"{name} U6")
    same_bits(got, G.u1(case), f"{name} U6 vs U1 on a fresh graph")
