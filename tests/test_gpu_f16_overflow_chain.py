"""-m gpu: the chain behind the f16 overflow flag, end to end: flagged stores inside a real autograd graph -> DeviceLossScaler's
begin_step / watching / end_backward / update -> the bucket's flag slot -> FlatAdam.step(found_inf=) -> a trainer iteration that is skipped.
(The stores themselves: tests/test_gpu_f16_flag_sites.py; the scaler's policy: tests/test_loss_scaler_cpu.py.)"""
import contextlib
import io
import math

import pytest
import torch

import graph_cases as G
from gpu_util import Flag
from test_gpu_graph_wiring import MF16, check, conv, err32

pytestmark = pytest.mark.gpu

H16 = torch.float16
LIM = 65504.0


def _restore_flag():
    Flag().restore()  # word zero, watching off: the state outside a backward pass


# ---------------------------------------------------------------------------------------------------------------------------------
# (a) a real autograd graph: graph_cases to_rgb_f16 (StyledConv -> ToRGB with an fp32 image), the project's one f16 graph
# ---------------------------------------------------------------------------------------------------------------------------------
def _loss_scales():
    """(S_lo, S_hi), powers of two chosen from the float64 restatement alone.  The f16 tensors that carry a gradient in this graph: the
    masked gradient stored on y1 (gain * lrelu'(z1) * dL/dy1, by the ToRGB data gradient's fused epilogue or mul_reduce + the mask pass),
    dL/dx (the first layer's data gradient) — both flagged stores — and the fp32 image gradient that re-enters the f16 kernels through a
    cast (no clamp: it overflows to inf, which the next flagged store reports).  S_lo puts the largest of the three at or below half of
    65504; S_hi puts the larger of the two flagged stores at or above twice 65504."""
    name = "to_rgb_f16"
    ref = G.reference(name)
    (act,) = [a for a in ref["acts"] if a[0] == "y1"]
    _, z, _, slope, gain = act
    stored_y1 = (gain * torch.where(z > 0, 1.0, slope) * ref["taps"]["y1"]).abs().max().item()
    stored_x = ref["u1"]["x"].abs().max().item()
    g64 = G.Graph(G.BY_NAME[name], lambda k, t: t.double(), ref=True)
    image_grad = (2 * g64.outs[0]).abs().max().item()  # d sum(rgb^2) / d rgb
    flagged, every = max(stored_y1, stored_x), max(stored_y1, stored_x, image_grad)
    s_lo = 2.0 ** math.floor(math.log2(0.5 * LIM / every))
    s_hi = 2.0 ** math.ceil(math.log2(2.0 * LIM / flagged))
    assert every * s_lo <= 0.5 * LIM and flagged * s_hi >= 2.0 * LIM
    print(f"\n[overflow chain] stored y1 {stored_y1:.3e} x {stored_x:.3e} image {image_grad:.3e}: S_lo 2^{math.log2(s_lo):.0f} S_hi 2^{math.log2(s_hi):.0f}")
    return s_lo, s_hi


def _scaled_backward(scale):
    """One backward of the graph under a DeviceLossScaler at `scale`, the way GifTrainer brackets it.  Returns (scaler, {leaf: grad / scale})."""
    from gif_amd.train_step import DeviceLossScaler, FlatGradBucket
    gr = G.Graph(G.BY_NAME["to_rgb_f16"], conv)
    fp32 = [n for n in gr.names if gr.L[n].dtype == torch.float32]  # (x is a half leaf: its gradient stays outside the fp32 bucket)
    assert set(gr.names) - set(fp32) == {"x"}
    bucket = FlatGradBucket([gr.L[n] for n in fp32])
    sc = DeviceLossScaler(torch.device("cuda"), init_scale=scale, growth_interval=1000, max_scale=2.0 ** 40)
    bucket.zero()
    sc.begin_step()
    with sc.watching():
        (gr.loss * sc.scale).backward()
    sc.end_backward(bucket)
    bucket.all_reduce_mean()  # (no process group: gathers the gradients into the bucket)
    sc.update(bucket.flat)
    torch.cuda.synchronize()
    grads = {n: gr.L[n].grad.detach().float().cpu() / scale for n in gr.names}
    return sc, bucket, grads


def test_graph_backward_under_the_scaler_below_and_above_the_limit():
    s_lo, s_hi = _loss_scales()
    try:
        sc, bucket, grads = _scaled_backward(s_lo)
        assert sc.found_inf.item() == 0.0 and sc.skipped.item() == 0.0 and sc.scale.item() == s_lo, "a spurious overflow at S_lo"
        assert bucket.flag_slot.item() == 0.0 and sc.inv_scale.item() == 1.0 / s_lo
        # the bound tests/test_gpu_graph_wiring.py holds this case to (MF16 * err32 + 2^-23, and 8 * 2^-11)
        check(grads, G.reference("to_rgb_f16")["u1"], err32("to_rgb_f16")["u1"], MF16, f"to_rgb_f16 at loss scale {s_lo}")
        sc, bucket, _ = _scaled_backward(s_hi)
        assert sc.found_inf.item() == 1.0, "a gradient store above the half range did not reach the scaler"
        assert sc.scale.item() == s_hi / 2 and sc.skipped.item() == 1.0 and sc.inv_scale.item() == 1.0 / s_hi
        assert sc.sat.item() > 0 and math.isinf(bucket.flag_slot.item()), "the overflow was seen, but not through the flag word"
    finally:
        _restore_flag()


# ---------------------------------------------------------------------------------------------------------------------------------
# (b) a trainer whose first steps overflow
# ---------------------------------------------------------------------------------------------------------------------------------
def _build(res, vocab=16):
    from gif_amd.discriminator import Discriminator
    from gif_amd.generator import StyledGenerator
    with contextlib.redirect_stdout(io.StringIO()):
        g = StyledGenerator(embedding_vocab_size=vocab, rendered_flame_ascondition=True, normal_maps_as_cond=True)
        d = Discriminator(size=res, num_color_chnls=9)
    return g, d


def _flat(tensors):
    return torch.cat([t.detach().reshape(-1) for t in tensors])


def _applied(optim):
    st = optim.state_dict()["state"]
    return float(next(iter(st.values()))["step"]) if st else 0.0


def test_trainer_skips_overflowing_steps_and_recovers():
    """GifTrainer at 32x32 with loss_scale 2^30 (test_gpu_f16.test_f16_gradients_and_training_iteration's trainer otherwise): iteration 0
    overflows in both networks and must leave every tensor of the optimisation untouched; the scales halve from clamp(2^29) = 2^20 until a
    step applies.  When that happens is whatever the halving gives; the test only holds the books: skipped + applied = iterations."""
    from gif_amd.train_step import GifTrainer
    torch.manual_seed(1)
    Gn, Dn = _build(32)
    G_ema, _ = _build(32)
    G_ema.load_state_dict(Gn.state_dict())
    tr = GifTrainer(Gn.cuda(), Dn.cuda(), G_ema.cuda(), step=3, r1_every=2, act_dtype=H16, loss_scale=2.0 ** 30)
    gen = torch.Generator(device="cuda").manual_seed(7)
    nets = {"G": list(Gn.parameters()), "D": list(Dn.parameters()), "G_ema": list(G_ema.parameters())}
    in_bucket = set(id(p) for p in tr.g_bucket.params)
    nets["G outside the bucket"] = [p for p in Gn.parameters() if id(p) not in in_bucket]
    assert nets["G outside the bucket"], "step = 3 leaves the blocks above 32x32 without a gradient"
    moments = {"G": [tr.g_optim._m, tr.g_optim._v], "D": [tr.d_optim._m, tr.d_optim._v]}
    for k, opt in (("G", tr.g_optim), ("D", tr.d_optim)):  # the flat buffers are the exp_avg / exp_avg_sq of every parameter
        st = opt.state[opt.bucket.params[0]]
        assert st["exp_avg"].data_ptr() == moments[k][0].data_ptr() and st["exp_avg_sq"].data_ptr() == moments[k][1].data_ptr()

    def snapshot():
        tr.flush()
        s = {k: _flat(v) for k, v in nets.items()}
        s.update({k + " moments": _flat(v) for k, v in moments.items()})
        return s

    def batch():
        real = torch.rand(4, 3, 32, 32, device="cuda", generator=gen) * 2 - 1
        c = torch.rand(4, 6, 32, 32, device="cuda", generator=gen) * 2 - 1
        return real, c, torch.randint(0, 16, (4,), device="cuda", generator=gen)

    try:
        before = snapshot()
        scales = {"G": tr.g_scaler, "D": tr.d_scaler}
        for sc in scales.values():
            assert sc.scale.item() == 2.0 ** 30
        # ---- iteration 0: both networks overflow
        tr.step(0, *batch())
        after = snapshot()
        for k, sc in scales.items():
            assert sc.skipped.item() == 1.0, f"{k}: the step at loss scale 2^30 was not skipped"
            assert sc.scale.item() == min(max(2.0 ** 30 / 2, 1.0), sc.max_scale) == 2.0 ** 20
        for k in before:
            assert torch.equal(before[k], after[k]), f"a skipped step changed {k}"
        assert _applied(tr.g_optim) == 0.0 and _applied(tr.d_optim) == 0.0
        # ---- go on until both networks have applied steps
        first = {"G": None, "D": None}
        for i in range(1, 24):
            applied0 = {"G": _applied(tr.g_optim), "D": _applied(tr.d_optim)}
            scale0 = {k: sc.scale.item() for k, sc in scales.items()}
            d_loss, g_loss = tr.step(i, *batch())
            now = snapshot()
            applied = {"G": _applied(tr.g_optim), "D": _applied(tr.d_optim)}
            for k, sc in scales.items():
                did = applied[k] - applied0[k]
                assert did in (0.0, 1.0) and sc.skipped.item() + applied[k] == i + 1, (k, i, sc.skipped.item(), applied[k])
                assert sc.scale.item() == (scale0[k] if did else max(scale0[k] / 2, 1.0)), (k, i)
                moved = not torch.equal(after[k], now[k])
                assert moved == bool(did), f"{k}, iteration {i}: the weights {'moved on a skipped' if moved else 'did not move on an applied'} step"
                assert torch.equal(after[k + " moments"], now[k + " moments"]) != bool(did), f"{k}, iteration {i}: Adam moments"
                if did and first[k] is None:
                    first[k] = i
            assert (not torch.equal(after["G_ema"], now["G_ema"])) == bool(applied["G"] - applied0["G"]), f"iteration {i}: G_ema moves with G's steps only"
            assert torch.equal(after["G outside the bucket"], now["G outside the bucket"])
            if first["G"] is not None or first["D"] is not None:
                assert math.isfinite(d_loss.item()) and math.isfinite(g_loss.item()), (i, d_loss.item(), g_loss.item())
            after = now
            if all(v is not None and i >= v + 2 for v in first.values()):
                break
        print(f"\n[overflow chain] first applied step: {first}; scales G {tr.g_scaler.scale.item()} D {tr.d_scaler.scale.item()}; "
              f"skipped G {tr.g_scaler.skipped.item()} D {tr.d_scaler.skipped.item()} of {i + 1} iterations")
        assert first["G"] is not None and first["D"] is not None, f"no step applied in {i + 1} iterations: {first}"
    finally:
        _restore_flag()
