"""CPU tier: the autograd WIRING of gif_amd (functional.py Functions, layers, generator, discriminator, losses, GifTrainer)
against the oracle, with every HIP launch replaced by its ATen contract (tests/cpu_ops.py).  Catches, without a GPU, what a
kernel test cannot: a backward that calls the wrong op / operand / scale, a gradient that silently loses its history under
create_graph (round-1 advisor finding), the data-parallel trainer's synchronisation.  The kernels behind the same entry points
are checked against the same oracle in the -m gpu tier."""
import contextlib
import io
import os
import socket

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cpu_ops
from gpu_util import assert_close, assert_grads_close
from oracle import stylegan2_ref as R


@pytest.fixture
def cpu(monkeypatch):
    cpu_ops.install(monkeypatch)


def _build_g(vocab=16):
    from gif_amd.generator import StyledGenerator
    with contextlib.redirect_stdout(io.StringIO()):
        return StyledGenerator(embedding_vocab_size=vocab, rendered_flame_ascondition=True, normal_maps_as_cond=True)


def _build_d(size):
    from gif_amd.discriminator import Discriminator
    return Discriminator(size=size, num_color_chnls=9)


def _leaves(sd):
    return {k: (v.clone().requires_grad_(True) if (not k.endswith('kernel') and 'embd_weight' not in k) else v.clone())
            for k, v in sd.items()}


def _seeded(model, seed):
    sd = R.seeded_state_dict(model.state_dict(), seed)
    model.load_state_dict(sd, strict=True)
    for p in model.parameters():
        p.requires_grad_(True)
    return sd


def test_generator_and_discriminator_first_order_vs_oracle(cpu):
    torch.manual_seed(0)
    g, d = _build_g(), _build_d(16)
    gsd, dsd = _seeded(g, 1), _seeded(d, 101)
    gen = torch.Generator().manual_seed(201)  # a draw without activation sign flips (see gpu_util.assert_grads_close)
    cond = torch.rand(4, 6, 16, 16, generator=gen) * 2 - 1
    idx = torch.tensor([1, 5, 9, 13])
    gl, dl = _leaves(gsd), _leaves(dsd)
    fake_r = R.generator_forward(gl, cond, 2, idx)
    loss_r = F.softplus(-R.discriminator_forward(dl, fake_r, cond, 16)).mean()
    fake = g(cond, None, step=2, alpha=1, input_indices=idx)
    assert_close(fake[0], fake_r, 1e-5, "G forward")
    loss = F.softplus(-d(fake, condition=cond)[0]).mean()
    assert abs(loss.item() - loss_r.item()) < 1e-5
    gk = [k for k, v in gl.items() if v.requires_grad]
    ref = torch.autograd.grad(loss_r, [gl[k] for k in gk], allow_unused=True)
    named = dict(g.named_parameters())
    got = torch.autograd.grad(loss, [named[k] for k in gk], allow_unused=True)
    assert_grads_close(got, ref, gk, tight=1e-4, max_outlier_frac=0.0, what="G grads through D")


def test_gradient_epilogue_fusions_equal_the_standalone_passes(cpu, monkeypatch):
    """The activation ports (leaky-ReLU backward + bias gradient + modulation gradient delivered by the kernel that produces
    the gradient, functional.ActPort / ops.GradFuse) against the same model with GIF_FUSE_GRAD off: same parameter gradients
    of G through D, and the fused routes were really taken (the dot-product fusion is forced on: at 16x16 the kernels' tile
    constraint would route it to the stand-alone pass, the contract restatement has no such constraint)."""
    from gif_amd import ops
    torch.manual_seed(0)
    g, d = _build_g(), _build_d(16)
    _seeded(g, 1), _seeded(d, 101)
    gen = torch.Generator().manual_seed(11)
    cond = torch.rand(4, 6, 16, 16, generator=gen) * 2 - 1
    idx = torch.tensor([1, 5, 9, 13])
    params = list(g.parameters()) + list(d.parameters())
    calls = {"mask": 0, "dot": 0, "colsum": 0, "bias_act_bwd": 0, "mul_reduce": 0, "colsum_op": 0}
    real_fuse = ops.GradFuse

    class CountingFuse(real_fuse):
        def __init__(self, **kw):
            super().__init__(**kw)
            calls["mask"] += self.mask_src is not None
            calls["dot"] += self.dot_src is not None
            calls["colsum"] += self.want_colsum

    def counted(name):
        fn = getattr(ops, name)

        def wrapped(*a, **k):
            calls[name] += 1
            return fn(*a, **k)
        return wrapped

    monkeypatch.setattr(ops, "GradFuse", CountingFuse)
    monkeypatch.setattr(ops, "bias_act_bwd", counted("bias_act_bwd"))
    monkeypatch.setattr(ops, "mul_reduce", counted("mul_reduce"))
    plain_colsum = ops.colsum

    def colsum_counted(x):
        calls["colsum_op"] += 1
        return plain_colsum(x)
    monkeypatch.setattr(ops, "colsum", colsum_counted)

    def grads(fused):
        monkeypatch.setattr(ops, "FUSE_GRAD", fused)
        monkeypatch.setattr(ops, "dot_fusable", (lambda H, W, dtype=torch.float32: True) if fused else (lambda H, W, dtype=torch.float32: False))
        for k in calls:
            calls[k] = 0
        fake = g(cond, None, step=2, alpha=1, input_indices=idx)
        loss = F.softplus(-d(fake, condition=cond)[0]).mean()
        out = torch.autograd.grad(loss, params, allow_unused=True)
        return out, dict(calls)

    ref, c0 = grads(False)
    got, c1 = grads(True)
    assert c0["mask"] == 0 and c0["dot"] == 0 and c0["bias_act_bwd"] > 10 and c0["mul_reduce"] > 8
    assert c1["mask"] > 10 and c1["dot"] >= 8 and c1["colsum"] > 5, c1
    assert c1["bias_act_bwd"] < c0["bias_act_bwd"] // 2, (c0, c1)
    # the last condition-noise conv of every StyledConv (conv + bias, no activation) gets its bias gradient from the layer it feeds
    assert c0["colsum_op"] - c1["colsum_op"] >= 5, (c0, c1)  # five StyledConvs at step 2
    n = 0
    for a, b, (k, _) in zip(got, ref, list(g.named_parameters()) + list(d.named_parameters())):
        assert (a is None) == (b is None), k
        if b is not None:
            assert_close(a, b, 2e-5, k)
            n += 1
    assert n > 80


def test_activation_ports_do_not_leak_the_graph(cpu):
    """The port protocol hangs Python attributes on activation tensors; a reference cycle through them would keep every
    iteration's activations alive (found on the GPU as an out-of-memory after a few steps).  The number of live tensors must
    not grow from one iteration to the next — with the cyclic garbage collector off."""
    import gc
    torch.manual_seed(0)
    g, d = _build_g(), _build_d(16)
    cond = torch.rand(2, 6, 16, 16) * 2 - 1
    idx = torch.tensor([1, 5])

    def live():
        return sum(1 for o in gc.get_objects() if isinstance(o, torch.Tensor))

    gc.collect()
    gc.disable()
    try:
        counts = []
        for _ in range(3):
            fake = g(cond, None, step=2, alpha=1, input_indices=idx)
            F.softplus(-d(fake, condition=cond)[0]).mean().backward()
            del fake
            counts.append(live())
    finally:
        gc.enable()
    assert counts[1] == counts[2], counts


def test_r1_double_backward_vs_oracle(cpu):
    from gif_amd import losses
    torch.manual_seed(0)
    d = _build_d(16)
    dsd = _seeded(d, 4)
    gen = torch.Generator().manual_seed(5)
    img = torch.rand(4, 3, 16, 16, generator=gen) * 2 - 1
    cond = torch.rand(4, 6, 16, 16, generator=gen) * 2 - 1
    dl = _leaves(dsd)
    ir = img.clone().requires_grad_(True)
    sr = R.discriminator_forward(dl, ir, cond, 16)
    pen_r = R.grad_penalty_loss([ir], sr)
    keys = [k for k, v in dl.items() if v.requires_grad]
    ref = torch.autograd.grad(F.softplus(-sr).mean() + pen_r.mean(), [dl[k] for k in keys])
    ih = img.clone().requires_grad_(True)
    sh, _ = d([ih], condition=cond)
    # the inner gradient (d scores / d image, create_graph) must not compute D's weight gradients (functional.inputs_only_backward)
    from gif_amd import ops
    n_wgrad = [0]
    real_wgrad = ops.conv_wgrad

    def counted_wgrad(*a, **k):
        n_wgrad[0] += 1
        return real_wgrad(*a, **k)
    ops.conv_wgrad = counted_wgrad
    try:
        pen = losses.grad_penalty_loss([ih], sh, step=None)
        assert n_wgrad[0] == 0, "the R1 inner pass computed weight gradients"
    finally:
        ops.conv_wgrad = real_wgrad
    assert_close(pen, pen_r.detach(), 1e-4, "R1 penalty")
    named = dict(d.named_parameters())
    got = torch.autograd.grad(F.softplus(-sh).mean() + pen.mean(), [named[k] for k in keys])
    assert_grads_close(got, ref, keys, tight=1e-4, what="D grads through the R1 double backward")


def test_generator_recorded_backward_path_length_and_direct_grad(cpu, monkeypatch):
    """The generator's fused ops switch to a recorded (any-order) backward under create_graph: StyleGAN2-form path-length
    penalty and DIRECT_GRAD_REG (train.py:203-215), values AND parameter gradients vs the oracle's autograd."""
    from gif_amd import losses
    torch.manual_seed(0)
    g = _build_g()
    gsd = _seeded(g, 6)
    gen = torch.Generator().manual_seed(7)
    B = 2
    cond = torch.rand(B, 6, 16, 16, generator=gen) * 2 - 1
    style = torch.randn(B, 512, generator=gen)
    noise = torch.randn(B, 3, 16, 16, generator=gen)
    gl = _leaves(gsd)
    z = style.clone().requires_grad_(True)
    fake_r = R.generator_forward(gl, cond, 2, z)
    (pg_r,) = torch.autograd.grad((fake_r * noise / np.sqrt(16 * 16)).sum(), z, create_graph=True)
    len_r = torch.sqrt(pg_r.pow(2).sum(1))
    mean_r = 0.01 * len_r.mean().detach()
    pen_r = (len_r - mean_r).pow(2).mean()
    keys = [k for k, v in gl.items() if v.requires_grad and not any(f".{i}." in k for i in (3, 4, 5, 6, 7, 8))]
    ref = torch.autograd.grad(pen_r, [gl[k] for k in keys], allow_unused=True)
    draws = [style, noise]

    def replay(*a, **k):
        t = draws.pop(0)
        return t.clone().requires_grad_(k.get("requires_grad", False))

    monkeypatch.setattr(torch, "randn", replay)
    reg = losses.PathLengthRegularizor(reference_semantics=False)
    pen = reg.path_length_reg(g, step=2, alpha=1.0, input_indices=torch.zeros(B, dtype=torch.long), cond=cond)
    monkeypatch.undo()
    cpu_ops.install(monkeypatch)
    assert pen.requires_grad
    assert abs(pen.item() - pen_r.item()) < 2e-2 * abs(pen_r.item()), (pen.item(), pen_r.item())
    named = dict(g.named_parameters())
    got = torch.autograd.grad(pen, [named[k] for k in keys], allow_unused=True)
    assert sum(1 for b in ref if b is not None and b.abs().max() > 0) > 40
    assert_grads_close(got, ref, keys, tight=2e-4, what="d PL penalty / d parameters (recorded backward of G)")
    # DIRECT_GRAD_REG
    gl = _leaves(gsd)
    idx = torch.tensor([3, 11])
    c_r = cond.clone().requires_grad_(True)
    pen_r = R.grad_penalty_loss([c_r], R.generator_forward(gl, c_r, 2, idx).pow(2)).mean()
    ref = torch.autograd.grad(pen_r, [gl[k] for k in keys], allow_unused=True)
    c_h = cond.clone().requires_grad_(True)
    fake = g(c_h, None, step=2, alpha=1, input_indices=idx)
    pen = losses.grad_penalty_loss([c_h], torch.pow(fake[-1], 2), step=None).mean()
    assert abs(pen.item() - pen_r.item()) < 2e-2 * abs(pen_r.item())
    got = torch.autograd.grad(pen, [named[k] for k in keys], allow_unused=True)
    assert_grads_close(got, ref, keys, tight=2e-4, what="d direct-grad penalty / d parameters")


def test_trainer_trajectory_vs_oracle_trainer_on_cpu(cpu):
    """GifTrainer (torch Adam on CPU) vs oracle/train_ref.py: two iterations incl. an R1 one — losses, weights, EMA."""
    from gif_amd.train_step import GifTrainer
    from oracle.train_ref import RefTrainer
    torch.manual_seed(0)
    G, G_ema, D = _build_g(), _build_g(), _build_d(16)
    g_sd = R.seeded_state_dict(G.state_dict(), 61)
    d_sd = R.seeded_state_dict(D.state_dict(), 62)
    G.load_state_dict(g_sd)
    G_ema.load_state_dict(g_sd)
    D.load_state_dict(d_sd)
    ref = RefTrainer(g_sd, d_sd, res_step=2, size=16, r1_every=2)
    tr = GifTrainer(G, D, G_ema, step=2, r1_every=2, fused_adam=False)
    gen = torch.Generator().manual_seed(63)
    for i in range(2):
        real = torch.rand(4, 3, 16, 16, generator=gen) * 2 - 1
        cond = torch.rand(4, 6, 16, 16, generator=gen) * 2 - 1
        idx = torch.randint(0, 16, (4,), generator=gen)
        d_ref, g_ref = ref.step(i, real, cond, idx)
        d_got, g_got = tr.step(i, real, cond, idx)
        assert abs(d_got.item() - d_ref.item()) < 1e-3 * max(1.0, abs(d_ref.item())), (i, d_got.item(), d_ref.item())
        assert abs(g_got.item() - g_ref.item()) < 1e-3 * max(1.0, abs(g_ref.item())), (i, g_got.item(), g_ref.item())
    # parameters above the current resolution never receive a gradient: like in the reference, Adam holds no state for them
    dead = G.generator.progression[5].st_cv1.conv.weight
    assert dead.grad is None and len(tr.g_optim.state.get(dead, {})) == 0


# ---- the REAL trainer in two data-parallel processes (gloo, CPU) -------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _dp_worker(rank, world, port, q):
    try:
        import copy
        import hashlib
        import torch.distributed as dist
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
        dist.init_process_group("gloo", rank=rank, world_size=world)
        torch.set_num_threads(2)
        cpu_ops.install()
        from gif_amd.train_step import GifTrainer
        torch.manual_seed(1000 + rank)  # different initial weights and embedding buffers per rank
        G, G_ema, D = _build_g(), _build_g(), _build_d(16)
        G_ema.load_state_dict(G.state_dict())
        w_before = G.generator.progression[1].st_cv2.conv.weight.detach().clone()
        tr = GifTrainer(G, D, G_ema, step=2, r1_every=2, fused_adam=False)  # broadcasts rank 0's state
        w_synced = G.generator.progression[1].st_cv2.conv.weight.detach().clone()
        emb = G.image_embedding.embd_weight.detach().clone()
        gen = torch.Generator().manual_seed(9)  # the GLOBAL batch of 8, identical in both processes
        real = torch.rand(2, 8, 3, 16, 16, generator=gen) * 2 - 1
        cond = torch.rand(2, 8, 6, 16, 16, generator=gen) * 2 - 1
        idx = torch.randint(0, 16, (2, 8), generator=gen)
        sl = slice(rank * 4, rank * 4 + 4)
        halves = []
        for h in range(world):  # the two halves' D gradients WITHOUT data parallelism, on copies of the synced models
            G2, D2 = copy.deepcopy(G), copy.deepcopy(D)
            hs = slice(h * 4, h * 4 + 4)
            rs, _ = D2([real[0, hs]], condition=cond[0, hs])
            with torch.no_grad():
                fk = G2(cond[0, hs], None, step=2, alpha=1.0, input_indices=idx[0, hs])[0]
            fs, _ = D2([fk], condition=cond[0, hs])
            gs = torch.autograd.grad(F.softplus(-rs).mean() + F.softplus(fs).mean(), list(D2.parameters()))
            halves.append(torch.cat([g.reshape(-1) for g in gs]))
        mean_halves = (halves[0] + halves[1]) / 2
        assert tr.overlap_comm
        tr.d_step(0, real[0, sl], cond[0, sl], idx[0, sl])
        tr.d_bucket.wait()
        exchanged = torch.cat([p.grad.reshape(-1) for p in D.parameters()]).clone()
        tr.g_step(cond[0, sl], idx[0, sl])
        l1 = tr.step(1, real[1, sl], cond[1, sl], idx[1, sl])  # R1 iteration
        tr.flush()
        err = ((exchanged - mean_halves).abs().max() / mean_halves.abs().max()).item()

        def digest(m):
            return hashlib.sha1(torch.cat([p.detach().reshape(-1) for p in m.parameters()]).numpy().tobytes()).hexdigest()

        q.put((rank, "ok", hashlib.sha1(w_before.numpy().tobytes()).hexdigest(), hashlib.sha1(w_synced.numpy().tobytes()).hexdigest(),
               hashlib.sha1(emb.numpy().tobytes()).hexdigest(), err, digest(G), digest(D), digest(G_ema), [t.item() for t in l1]))
        dist.destroy_process_group()
    except Exception:
        import traceback
        q.put((rank, "error", traceback.format_exc()))
        raise


def test_real_trainer_two_gloo_processes_on_cpu():
    """GifTrainer itself (not a stand-in model) in two gloo processes: construction-time broadcast from different per-rank
    seeds, exchanged D gradients == mean of the halves' single-process gradients, replicas bit-identical after two iterations."""
    import torch.multiprocessing as mp
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_dp_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=900) for _ in range(world)], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=120)
    for r in res:
        assert r[1] == "ok", r[2]
    (_, _, b0, s0, e0, err0, g0, d0, m0, l0), (_, _, b1, s1, e1, err1, g1, d1, m1, l1) = res
    assert b0 != b1, "ranks started from different weights"
    assert s0 == s1 == b0, "construction broadcast rank 0's parameters"
    assert e0 == e1, "construction broadcast rank 0's embedding BUFFER"
    assert err0 < 1e-5 and err1 < 1e-5, (err0, err1)
    assert g0 == g1 and d0 == d1 and m0 == m1, "replicas bit-identical after 2 iterations"
    assert all(np.isfinite(l0)) and all(np.isfinite(l1))


def test_fused_discriminator_passes_equal_the_two_calls(cpu):
    """GifTrainer.d_step runs D once on [real; fake] (minibatch-stddev per half) where train.py:142 / :169 call it twice: same
    loss, same gradients (every D parameter receives one gradient instead of two that autograd adds), R1 iterations unchanged."""
    import copy
    from gif_amd.train_step import GifTrainer
    torch.manual_seed(0)
    G, G_ema, D = _build_g(), _build_g(), _build_d(16)
    G_ema.load_state_dict(G.state_dict())
    gen = torch.Generator().manual_seed(5)
    real = torch.rand(8, 3, 16, 16, generator=gen) * 2 - 1
    cond = torch.rand(8, 6, 16, 16, generator=gen) * 2 - 1
    idx = torch.randint(0, 16, (8,), generator=gen)
    out = {}
    for fuse in (True, False):
        g, ge, d = copy.deepcopy(G), copy.deepcopy(G_ema), copy.deepcopy(D)
        tr = GifTrainer(g, d, ge, step=2, r1_every=2, fused_adam=False, fuse_d_passes=fuse)
        calls = []
        orig = d.forward
        d.forward = lambda *a, _o=orig, **k: (calls.append(a[0][0].shape[0]), _o(*a, **k))[1]
        loss0 = tr.d_step(0, real, cond, idx)
        grads = [p.grad.clone() for p in d.parameters()]
        n_plain = len(calls)
        loss1 = tr.d_step(1, real, cond, idx)  # R1 iteration: separate calls in both modes
        out[fuse] = (loss0.item(), grads, n_plain, len(calls) - n_plain, calls[:n_plain], loss1.item())
    assert out[True][2] == 1 and out[True][4] == [16], "one D call over 2 x 8 samples"
    assert out[False][2] == 2 and out[False][4] == [8, 8]
    assert out[True][3] == 2 and out[False][3] == 2, "R1 iterations keep the two calls"
    assert abs(out[True][0] - out[False][0]) < 1e-6 * max(1.0, abs(out[False][0]))
    assert abs(out[True][5] - out[False][5]) < 1e-4 * max(1.0, abs(out[False][5]))
    for a, b in zip(out[True][1], out[False][1]):
        assert_close(a, b, 2e-5, "D gradients: fused pass vs two calls")


def test_modulation_bank_is_one_call_and_equals_the_per_layer_linears(cpu, monkeypatch):
    """Generator.forward hands every ModulatedConv2d the same w (len(style) < 2): their EqualLinears run as ONE LinearBankFn call
    (reference: one call per layer, stylegan2_common_layers.py:311-313) — same image, same parameter gradients; two styles
    (mixing) fall back to the per-layer path."""
    from gif_amd import functional as GF, layers
    torch.manual_seed(0)
    g = _build_g()
    _seeded(g, 9)
    gen = torch.Generator().manual_seed(3)
    cond = torch.rand(2, 6, 16, 16, generator=gen) * 2 - 1
    idx = torch.tensor([1, 7])
    calls = []
    orig = GF.ops.linear_bank_fwd
    monkeypatch.setattr(GF.ops, "linear_bank_fwd", lambda x, ws, bs, sc: (calls.append(len(ws)), orig(x, ws, bs, sc))[1])
    out = {}
    for bank in (True, False):
        monkeypatch.setattr(layers, "_STYLE_BANK", bank)
        g.zero_grad(set_to_none=True)
        img = g(cond, None, step=2, alpha=1, input_indices=idx)[-1]
        img.pow(2).mean().backward()
        out[bank] = (img.detach().clone(), {k: p.grad.clone() for k, p in g.named_parameters() if p.grad is not None})
    assert calls == [8], calls  # 4x4: conv + ToRGB, 8x8 and 16x16: two convs + ToRGB each
    assert_close(out[True][0], out[False][0], 1e-6, "image: bank vs per-layer modulation")
    assert out[True][1].keys() == out[False][1].keys()
    for k in out[False][1]:
        assert_close(out[True][1][k], out[False][1][k], 2e-5, f"grad {k}: bank vs per-layer modulation")
    assert all(c.conv._banked is None for c in g.generator.to_rgb), "every banked s was consumed"
    # two styles: no bank
    monkeypatch.setattr(layers, "_STYLE_BANK", True)
    calls.clear()
    styles = [torch.randn(2, 512, generator=gen), torch.randn(2, 512, generator=gen)]
    noise = g._condition_pyramid(cond, 2) if hasattr(g, "_condition_pyramid") else None
    if noise is not None:
        g.generator(styles, None, noise, step=2, alpha=1)
        assert calls == []


def test_interpolate_flame_labels_and_synthetic_flame_fixtures():
    """Host logic of the texture-interpolation hook (train.py:224-227): neighbouring labels blended with one weight, light /
    texture codes of the first sample kept; the synthetic FLAME stand-in and texture-space fixture have the reference's shapes."""
    import numpy as np
    from gif_amd import data, losses
    lbl = torch.arange(4 * 236, dtype=torch.float32).view(4, 236)
    out = losses.interpolate_flame_labels(lbl, t=0.25)
    assert out.shape == (3, 236)
    assert torch.allclose(out[:, :159], lbl[:-1, :159] + 0.25 * (lbl[1:, :159] - lbl[:-1, :159]))
    assert torch.equal(out[:, 159:], lbl[:-1, 159:])
    np.random.seed(3)
    t = np.random.uniform(0, 1)
    np.random.seed(3)
    assert torch.allclose(losses.interpolate_flame_labels(lbl), losses.interpolate_flame_labels(lbl, t))
    tmpl = np.random.RandomState(0).randn(50, 3).astype(np.float32)
    flame = data.SyntheticFlame(tmpl, "cpu", seed=1)
    lab = data.synthetic_flame_labels(3, "cpu", torch.Generator().manual_seed(2))
    v, a, b = flame(shape_params=lab[:, :100], expression_params=lab[:, 100:150], pose_params=lab[:, 150:156])
    assert v.shape == (3, 50, 3) and a is None and b is None
    v0, _, _ = flame(torch.zeros(1, 100), torch.zeros(1, 50), torch.zeros(1, 6))
    assert torch.allclose(v0[0], torch.from_numpy(tmpl), atol=1e-6)  # zero parameters = the template
    R = data._rodrigues(torch.tensor([[0.0, 0.0, np.pi / 2]]))
    assert torch.allclose(R[0] @ torch.tensor([1.0, 0.0, 0.0]), torch.tensor([0.0, 1.0, 0.0]), atol=1e-6)
    faces = np.random.RandomState(1).randint(0, 50, (80, 3))
    td = data.synthetic_texture_data(faces, T=64, fill=0.5)
    n = len(td["valid_pixel_ids"])
    assert td["valid_pixel_3d_faces"].shape == (n, 3) and td["valid_pixel_b_coords"].shape == (n, 3)
    assert abs(n / 64 ** 2 - 0.5) < 0.05 and np.allclose(td["valid_pixel_b_coords"].sum(1), 1, atol=1e-5)


# ---------------------------------------------------------------------------------------------------------------------------------
# tests/test_gpu_render_edges.py: every hand-written fp64 restatement it bounds the kernels with agrees with ATen's float64 result
# (F.interpolate, F.grid_sample, F.normalize) or with fp64 autograd, at every row of its tables — a wrong restatement cannot bless a
# wrong kernel.  No GPU.
# ---------------------------------------------------------------------------------------------------------------------------------
def _agree12(a, b, what):
    assert a.shape == b.shape, (what, a.shape, b.shape)
    d = (a - b).abs().max().item() if a.numel() else 0.0
    assert d <= 1e-12, f"{what}: restatement and ATen float64 differ by {d:.3e}"


def _edges():
    import test_gpu_render_edges as E
    return E


@pytest.mark.parametrize("mode", ["bilinear", "bicubic"])
@pytest.mark.parametrize("name", ["rs_1x1", "rs_1x9_h4", "rs_2x3", "rs_3x3_up16", "rs_identity", "rs_down_16", "rs_9x12", "rs_33x31",
                                  "rs_exact_4x6", "rs_planes1", "rs_view_2x3", "rs_gridcap"])
def test_render_edges_resize_restatement(name, mode):
    E = _edges()
    assert name in [r[0] for r in E.RS_ROWS] and len(E.RS_ROWS) == 12 and E.RS_MODES == ["bilinear", "bicubic"]
    _, _, (Hi, Wi), (Ho, Wo) = next(r for r in E.RS_ROWS if r[0] == name)
    c = E._resize_case(name, mode)
    x = c["x"].double().requires_grad_(True)
    ref = E._interp64(x, (Ho, Wo), mode)
    (gref,) = torch.autograd.grad(ref, x, c["gy"].double())
    _agree12(c["fwd"], ref.detach(), f"{name} {mode} forward")
    _agree12(c["bwd"], gref, f"{name} {mode} backward")
    assert (c["R"] >= ref.detach().abs() - 1e-12).all() and (c["Rb"] >= gref.abs() - 1e-12).all()
    if mode == "bilinear":  # weights >= 0: R is the operation itself on |x|
        _agree12(c["R"], E._interp64(c["x"].double().abs(), (Ho, Wo), mode), f"{name} R")
    assert c["exact"] == (E._is_pow2(Hi, Ho) and E._is_pow2(Wi, Wo)) == (name in ("rs_1x9_h4", "rs_identity", "rs_exact_4x6", "rs_gridcap"))
    if not c["exact"]:
        assert torch.isfinite(c["S"]).all() and (c["S"] >= 0).all() and (c["Sb"] >= 0).all() and c["Sb"].shape == gref.shape


@pytest.mark.parametrize("mode", ["bilinear", "bicubic"])
def test_render_edges_tap_derivatives(mode):
    """d weight / d coordinate of _taps (what S is built from) against a central difference, wherever no tap index flips."""
    E = _edges()
    for nin, nout in ((2, 9), (3, 16), (16, 5), (9, 31), (33, 8), (31, 64)):
        idx, w, dw, mag, wr = E._taps(nin, nout, mode)
        h = 1e-6
        (ip, wp, _, _, _), (im, wm, _, _, _) = E._taps(nin, nout, mode, h), E._taps(nin, nout, mode, -h)
        same = ((ip == im).all(1) & (ip == idx).all(1))
        if mode == "bilinear":
            same &= (nin / nout * (torch.arange(nout) + 0.5) - 0.5 - 2 * h * mag) > 0  # past the src < 0 clamp
        assert same.sum() >= nout // 2
        fd = (wp - wm) / (2 * h * mag[:, None])
        assert ((fd - dw).abs()[same] < 1e-6).all(), (nin, nout, (fd - dw).abs()[same].max())
        assert (w.sum(1) - 1).abs().max() < 1e-12 and dw.sum(1).abs().max() < 1e-12  # a partition of unity
        assert (wr >= w.abs()).all() if mode == "bicubic" else not wr.any()  # the polynomial on absolute values bounds the weight


@pytest.mark.parametrize("name", ["tx_t21_8x8", "tx_t21_8x8_rand", "tx_t16_8x8", "tx_t16_1x1_c4", "tx_t32_5x12_c4", "tx_t32_12x5_c1_rand",
                                  "tx_t21_12x5_c1", "tx_t21_5x12_b3", "tx_t32_8x8_c4_b3_rand", "tx_t16_1x1_c1_rand"])
def test_render_edges_texture_restatement(name):
    E = _edges()
    assert name in [r[0] for r in E.TX_ROWS] and len(E.TX_ROWS) == 10
    c = E._tex_case(name)
    valid = c["tmap"] >= 0
    assert c["verts"].shape[1] <= 16 and E._tex_grid(c)[0].abs().max() <= 4
    if c["B"] > 1:  # one mesh, different cameras
        assert torch.equal(c["verts"][0], c["verts"][1]) and not torch.equal(c["cam"][0], c["cam"][1])
    for gtex in (c["gtex"].double(), c["gtex"].double() * (~valid).view(1, 1, c["T"], c["T"])):
        ref, mask, gref, gabs = E._tex_reference(c, gtex)
        r = E._tex_restated(c, gtex)
        _agree12(r["fwd"], ref, f"{name} forward")
        _agree12(r["bwd"], gref, f"{name} backward")
        _agree12(r["Rb"], gabs, f"{name} backward R")
        assert (r["R"] >= ref.abs() - 1e-12).all() and (r["S"] >= 0).all() and (r["Sb"] >= 0).all()
    if c["exact"]:
        E._tex_named_ok(c, r["ntaps"])
    # the map is what the row's comment says: 256-texel workgroups all valid / all invalid / mixed
    wg = [valid[i:i + 256] for i in range(0, len(valid), 256)]
    kind = next(r_[5] for r_ in E.TX_ROWS if r_[0] == name)
    if kind == "wg2_invalid":
        assert len(wg) == 2 and len(wg[1]) == 185 and not wg[1].any() and wg[0].any() and not wg[0].all()
    elif kind == "all":
        assert len(wg) == 1 and wg[0].all()
    else:
        assert len(wg) == 4 and all(w.view(4, 64).any(1).all() and not w.view(4, 64).all(1).any() for w in wg)


@pytest.mark.parametrize("name", ["vn_v255", "vn_v256", "vn_v257", "vn_v85_b3", "vn_v86_b3"])
def test_render_edges_normals_restatement(name):
    """The three-pass corner sum equals the sum of the face normals cross(p1 - p0, p2 - p0) over a vertex's faces (each corner's
    cross product is that normal), accumulated face by face in numpy; x / max(|x|, eps) is F.normalize; the Jacobian behind R is
    fp64 autograd's."""
    E = _edges()
    assert name in [r[0] for r in E.VN_ROWS] and len(E.VN_ROWS) == 5
    c = E._vn_case(name)
    x, Rx, n, R = E._vn_restated(c["verts"], c["faces"])
    v = c["verts"].double().numpy()
    want = np.zeros_like(v)
    for f in c["faces"].numpy():
        nf = np.cross(v[:, f[1]] - v[:, f[0]], v[:, f[2]] - v[:, f[0]])
        for k in f:
            want[:, k] += nf
    _agree12(x, torch.from_numpy(want), f"{name} corner sums")
    _agree12(n, F.normalize(x, eps=E.EPS, dim=-1), f"{name} normalize")
    assert (Rx >= x.abs() - 1e-12).all() and (R >= n.abs()).all()
    pick = torch.tensor([E.VN_FAN, E.VN_TRI, E.VN_ONE[0], E.VN_TINY[0], E.VN_NOFACE[0], c["V"] - 1])
    xs = x[0, pick]
    J = torch.autograd.functional.jacobian(lambda t: F.normalize(t, eps=E.EPS, dim=-1), xs)  # [6,3,6,3]
    J = torch.stack([J[i, :, i, :] for i in range(len(pick))])
    got = E._normalize_jacobian(xs)
    assert ((got - J).abs() <= 1e-12 * J.abs().amax(dim=(1, 2), keepdim=True).clamp_min(1)).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# The fp64 restatements of tests/test_gpu_pointwise_edges.py, tied to ATen float64 / the oracle within 1e-12.  No GPU.
# ---------------------------------------------------------------------------------------------------------------------------------
def _pointwise():
    import test_gpu_pointwise_edges as P
    return P


def test_pointwise_edges_pack_reference():
    """pack_ref is a zero tensor with the two sources written at their offsets, and its adjoint per source is the channel slice."""
    P = _pointwise()
    for row in P.PK_ROWS:
        name, B, H, W, C0, off0, C1, off1, cp, v0, v1 = row
        if B * H * W > 4096:
            continue
        g = P._rng(row)
        a = torch.randn(B, C0, H, W, generator=g, dtype=torch.float64)
        b = torch.randn(B, C1, H, W, generator=g, dtype=torch.float64) if C1 else None
        want = torch.zeros(B, cp, H, W, dtype=torch.float64)
        want[:, off0:off0 + C0] = a
        if b is not None:
            want[:, off1:off1 + C1] = b
        got = P.pack_ref(a, b, off0, off1, cp)
        _agree12(got, want, f"{name} pack_ref")
        gy = torch.randn(B, cp, H, W, generator=g, dtype=torch.float64)
        rhs = (a * gy[:, off0:off0 + C0]).sum() + (0 if b is None else (b * gy[:, off1:off1 + C1]).sum())
        assert abs((got * gy).sum() - rhs) <= 1e-12 * (got.abs() * gy.abs()).sum()


def test_pointwise_edges_texture_loss_restatement():
    """tex_loss64 is the oracle's pairwise_texture_loss on the textures times the common visibility mask; tex_grad_R bounds the
    autograd gradient and keeps (1 + s) where the gradient has (1 - s)."""
    from oracle import texture_loss_ref as TL
    P = _pointwise()
    for row in P.TX_ROWS:
        name, C, H, W = row[:4]
        if C * H * W > 4096:
            continue
        a, b, ma, mb, f = P._tex_case(row)
        a64 = a.double().requires_grad_(True)
        loss, Rl, d, s = P.tex_loss64(a64, b, ma, mb, f)
        m = torch.ones(H, W, dtype=torch.float64)
        for t in (ma, mb):
            m = m if t is None else m * t.double()
        want = TL.pairwise_texture_loss(f.double()[None], a.double() * m, b.double() * m)
        assert abs(loss.item() - want.item()) <= 1e-12 and Rl.item() >= abs(loss.item()) - 1e-12
        (gr,) = torch.autograd.grad(loss, a64)
        s_, d_ = s.detach(), d.detach()
        _agree12(gr, f.double() * s_ * (1 - s_) * 2 * d_ * m / d_.numel(), f"{name} gradient formula")
        assert (P.tex_grad_R(d_, s_, f, 0.37) >= 0.37 * gr.abs() - 1e-300).all()
        if row[6] == "sat":
            assert sorted(set((a - b).abs().round().flatten().tolist())) == [0.0, 3.0, 10.0, 1000.0]


def test_pointwise_edges_pyramid_tap_rule():
    """down_tap_mask marks exactly the source pixels with a non-zero weight in fp64 autograd of F.interpolate, each weight 0.25."""
    P = _pointwise()
    for name, B, C, R, S in P.BD_ROWS:
        if R == S or R > 64:
            continue
        x = torch.zeros(1, 1, R, R, dtype=torch.float64, requires_grad=True)
        y = F.interpolate(x, (S, S), mode="bilinear", align_corners=False)
        (w,) = torch.autograd.grad(y, x, torch.ones_like(y))
        mask = P.down_tap_mask(R, S)
        assert torch.equal(w[0, 0] != 0, mask) and mask.sum().item() == 4 * S * S, name
        _agree12(w[0, 0], 0.25 * mask.double(), f"{name} tap weights")


def test_pointwise_edges_fir_rows_match_the_oracle():
    """fir64 on every (kernel shape, up, down, pad0, output size, flip) of the generic-kernel rows — non-square kernels, flip = 0,
    pad0 = 0 and beyond the kernel, outputs past the input: none of which test_fir64_matches_the_oracle covers — is the oracle's
    upfirdn2d (flip = 0: the oracle given the flipped kernel), cropped to the row's output size; fir_support marks its non-zero
    outputs for a positive input."""
    P = _pointwise()
    for row in P.GF_ROWS:
        name, B, C, H, W, KH, KW, up, down, pad0, (Ho, Wo), flip, epi = row
        x, k, _, _ = P._fir_case(row, False)
        x, k = x.double(), k.double()
        p1 = max((Ho - 1) * down + KH - (H * up + pad0), (Wo - 1) * down + KW - (W * up + pad0))
        want = R.upfirdn2d(x, k if flip else torch.flip(k, [0, 1]), up, down, (pad0, p1))[:, :, :Ho, :Wo]
        got = P.fir64(x, k, up, down, pad0, (Ho, Wo), flip)
        _agree12(got, want, f"{name} fir64")
        pos = R.upfirdn2d(torch.ones_like(x), k, up, down, (pad0, p1))[0, 0, :Ho, :Wo]
        assert torch.equal(pos > 0, P.fir_support(row)), name
        if flip is False and KH * KW > 1:
            assert (got - P.fir64(x, k, up, down, pad0, (Ho, Wo), True)).abs().max() > 1e-3, f"{name}: the kernel is symmetric"


# ---------------------------------------------------------------------------------------------------------------------------------
# tests/test_gpu_winograd_edges.py: the edge each row claims, held against csrc/wino_route.h (through tests/host/wino_route_dump.cpp) and
# csrc/wgrad_route.h (through tests/host/wgrad_route_dump.cpp), and its fp64 restatements tied to ATen float64.  No GPU.
# ---------------------------------------------------------------------------------------------------------------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _winograd():
    import test_gpu_winograd_edges as WE
    return WE


def test_winograd_edges_constants_are_the_sources():
    """A constant or a decision changed in csrc/wino_route.h fails here; it does not silently move a row off its edge: K is the header's
    constants, and geometry() — written from the host code before the header existed — is what the header reports (through
    tests/host/wino_route_dump.cpp, a stand-alone program under ASan + UBSan) for every row in every mode."""
    import re
    import subprocess
    import tempfile
    from gif_amd import ops
    WE = _winograd()
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    flags = "-x c++ -std=c++17 -O1 -g -Wall -Werror -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined"
    cases, args = [], ["K"]
    before = ops.get_fp32_mfma_mode()
    try:
        for row in WE.FROWS:
            for mode in WE.MODES:  # (every mode, also those the GPU test of the row does not run)
                ops.set_fp32_mfma_mode(mode)
                entry = ops.winograd_mode("fwd", row.shape[2])  # the entry point ops.conv3x3_winograd calls
                B, C, Co, H, W = row.shape
                cases.append((row, mode, entry))
                args += ["fwd"] + [str(v) for v in (B, H, W, C, Co, WE.MODES.index(entry), 1)]
    finally:
        ops.set_fp32_mfma_mode(before)
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "wino_route_dump")
        built = subprocess.run([hipcc] + flags.split() + ["-I", os.path.join(ROOT, "gif_amd", "csrc"),
                                                          os.path.join(ROOT, "tests", "host", "wino_route_dump.cpp"), "-o", exe],
                               capture_output=True, text=True, timeout=600)
        assert built.returncode == 0, built.stderr[-4000:]
        ran = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300)
    assert ran.returncode == 0, (ran.returncode, ran.stderr[-4000:])
    lines = ran.stdout.splitlines()
    assert len(lines) == len(cases) + 1
    assert {k: int(v) for k, v in (f.split("=") for f in lines[0].split())} == dict(WE.K, WNSTAGE=3)
    pat = re.compile(r"-> rows<8> lanes(\d+) blocks(\d+) thr256 trips(\d+) fam4 ; (mfma<2>|mfma<4>|x3<128,128>|h2<128,128,3>) bm(\d+) bn(\d+) tm(\d+) tn(\d+) "
                     r"grid(\d+) thr(\d+) lds\d+(?: \+ twin x3<128,128> bm128 bn128 tm(\d+) tn(\d+) grid(\d+) thr512 lds\d+)? ; "
                     r"ntiles(\d+) pad(\d+) RP(\d+) CP(\d+) ")
    names = {"mfma<2>": "mfma2", "mfma<4>": "mfma4", "x3<128,128>": "x3", "h2<128,128,3>": "h2"}
    seen = set()
    for (row, mode, entry), l in zip(cases, lines[1:]):
        geo = WE.geometry(*row.shape, mode)
        m = pat.search(l)
        assert m, l
        lanes, blocks, trips, gemm, bm, bn, tm, tn, grid, thr = m.groups()[:10]
        ntiles, pad, rp, cp = (int(v) for v in m.groups()[13:])
        got = dict(ntiles=ntiles, ntiles_pad=pad, CP=cp, RP=rp, tiles_m=int(tm), tiles_n=int(tn), nwg=int(grid), wide=gemm == "mfma<4>",
                   gemm=names[gemm], lanes=int(lanes), trips=int(trips))
        assert got == {k: geo[k] for k in got}, (row.name, mode, l)
        assert (int(bm), int(bn)) == (geo["ntiles_pad"] // geo["tiles_m"], geo["RP"] // geo["tiles_n"]), (row.name, mode, l)
        assert int(blocks) == min(-(-geo["lanes"] // 256), WE.K["CAP_WG"]) and int(thr) == (256 if gemm == "mfma<2>" else 512), (row.name, mode, l)
        assert (entry == "f16x2") == (m.group(11) is not None) and (m.group(11) is None or m.groups()[10:13] == (tm, tn, grid)), (row.name, mode, l)
        seen.add(got["gemm"])
    assert seen == {"mfma2", "mfma4", "x3", "h2"}
    assert WE.CAP_LANES == 2097152 == 32 * 16 * 128 * 32  # the benchmark's own shape: batch 32, 256^2, 128 channels


def test_winograd_edges_forward_rows_sit_on_their_edges():
    from gif_amd import _lib
    import ctypes
    WE = _winograd()
    lib = _lib.load()
    names = [r.name for r in WE.FROWS]
    assert len(set(names)) == len(names)
    seen = set()
    for row in WE.FROWS:
        B, C, Co, H, W = row.shape
        assert H % 2 == 0 and W % 2 == 0 and C % 4 == 0 and Co % 4 == 0 and row.claim
        for mode in WE.MODES:
            geo = WE.geometry(*row.shape, mode)
            rp, cp = ctypes.c_int(), ctypes.c_int()
            dims = lib.gif_winograd_pack_dims_x3 if geo["gemm"] in ("x3", "h2") else lib.gif_winograd_pack_dims
            assert dims(Co, C, ctypes.byref(rp), ctypes.byref(cp)) == 0 and (rp.value, cp.value) == (geo["RP"], geo["CP"]), row.name
            assert lib.gif_winograd_workspace_floats(B, H, W, C) == 16 * geo["ntiles_pad"] * geo["CP"], row.name
            assert geo["ntiles_pad"] * geo["CP"] < 2 ** 31 and B * H * W * max(C, Co) < 2 ** 31, row.name  # the library's own limits
            for key, want in row.claim.items():
                k, _, m = key.partition(":")
                if (m or "native") == mode:
                    assert geo[k] == want, (row.name, mode, k, geo[k], want)
                    seen.add(k)
        if row.epi == "fusedot":
            assert (H // 2) * (W // 2) % 128 == 0
    assert seen >= {"ntiles", "ntiles_pad", "lanes", "trips", "tiles_m", "wide", "RP", "CP", "nwg", "gemm", "yblocks", "last_block", "pad_blocks"}
    by = {r.name: WE.geometry(*r.shape) for r in WE.FROWS}
    assert by["cap_exact"]["lanes"] == WE.CAP_LANES and by["cap_over"]["lanes"] - WE.CAP_LANES == by["cap_over"]["CP"] // 4  # exactly one tile
    assert {by[n]["ntiles"] for n in ("t127", "t128", "t129", "t255", "t256", "t257")} == {127, 128, 129, 255, 256, 257}
    assert all(g["tiles_m"] % 2 == 0 for g in by.values())  # WPAD = 2 * WBM: an odd workgroup count such as 9 cannot occur
    assert {by[n]["nwg"] % 8 for n in ("t127", "nwg6", "nwg10")} == {2, 6} and by["nwg10"]["nwg"] > 8


def test_winograd_edges_wgrad_rows_sit_on_their_edges(tmp_path):
    """Tile pair, 256-row tile, bf16x3 / f16x2 eligibility, split count and chunk of every weight-gradient row, from wgrad_route.h."""
    import re
    import subprocess
    from gif_amd import _lib
    WE = _winograd()
    lib = _lib.load()
    exe = str(tmp_path / "wgrad_route_dump")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    flags = "-x c++ -std=c++17 -O1 -g -Wall -Werror -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined"
    built = subprocess.run([hipcc] + flags.split() + ["-I", os.path.join(ROOT, "gif_amd", "csrc"),
                                                      os.path.join(ROOT, "tests", "host", "wgrad_route_dump.cpp"), "-o", exe],
                           capture_output=True, text=True, timeout=600)
    assert built.returncode == 0, built.stderr[-4000:]
    pad32 = lambda c: (c + 31) // 32 * 32
    cases, args = [], []
    for row in WE.WROWS:
        B, Cs, Cb, H, W, O, I = row.shape
        assert O <= Cs and I <= Cb and Cs % 4 == 0 and Cb % 4 == 0 and H % 2 == 0 and W % 2 == 0
        ntiles = B * (H // 2) * (W // 2)
        assert ntiles == row.claim["ntiles"]
        nsplit = lib.gif_conv3x3_winograd_wgrad_splits(B, H, W, Cs, Cb)
        for mode in row.modes:
            cases.append((row, mode, nsplit))
            args += ["planes", str(ntiles), str(pad32(Cs)), str(pad32(Cb)), str(WE.MODES.index(mode)), str(nsplit)]
    ran = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300)
    assert ran.returncode == 0, (ran.returncode, ran.stderr[-4000:])
    lines = ran.stdout.splitlines()
    assert len(lines) == len(cases)
    pat = re.compile(r"-> (?:mfma f32 (\d+)x(\d+) \S+ \S+ bkp(\d+) tab0 x3=(\d)|h2v2 tab1) thr256|-> mfma f32 32x32 w1x1 glds1 bkp32 tab0 x3=0 thr64")
    seen_tiles, multi_short = set(), False
    for (row, mode, nsplit), l in zip(cases, lines):
        c = row.claim
        chunk, fam, splits = (int(re.search(p, l).group(1)) for p in (r" chunk(\d+) ", r" fam(\d+) ", r" splits (\d+)$"))
        assert splits == nsplit == c.get("nsplit", nsplit), (row.name, l)  # the header's count is the library's
        assert chunk == c.get("chunk", chunk) and chunk % 32 == 0 and (nsplit - 1) * chunk < c["ntiles"] <= nsplit * chunk, (row.name, l)
        multi_short |= nsplit > 1 and nsplit * chunk > c["ntiles"]
        native_tile = re.search(r"mfma f32 (\d+)x(\d+) ", l)
        x3 = mode != "native" and bool(c.get("x3"))
        assert fam == (3 if not x3 else 11 if mode == "bf16x3" else 16), (row.name, mode, l)
        if mode == "native":
            assert (int(native_tile.group(1)), int(native_tile.group(2))) == c["tile"], (row.name, l)
            assert ("256x128" in l) == bool(c.get("big")), (row.name, l)
            seen_tiles.add(c["tile"])
        elif x3:
            assert c["tile"] == (128, 128) and ("x3=1" in l) and (mode == "bf16x3" or l.split("->")[1].lstrip().startswith("h2v2")), (row.name, l)
        else:
            assert "x3=0" in l and "twin" not in l, (row.name, l)
    assert seen_tiles == {(32, 32), (32, 128), (128, 32), (128, 128), (256, 128)} and multi_short
    assert {r.claim["ntiles"] for r in WE.WROWS} >= {31, 33, 75, 129, 16384, 16128}


def test_winograd_edges_restatements():
    """wino_v64, the V reference: folded with G g G^T through A^T . A (F(2x2, 3x3)) it is the convolution in ATen float64, which ties
    its position and tile order to the operation; the data gradient as a forward conv with flipped taps and swapped channels."""
    WE = _winograd()
    G = torch.tensor([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], dtype=torch.float64)
    AT = torch.tensor([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=torch.float64)
    g = torch.Generator().manual_seed(11)
    for B, C, O, H, W in ((2, 5, 3, 2, 2), (1, 4, 6, 6, 4), (3, 3, 2, 4, 10)):
        x = torch.randn(B, C, H, W, generator=g, dtype=torch.float64)
        w = torch.randn(O, C, 3, 3, generator=g, dtype=torch.float64)
        gy = torch.randn(B, O, H, W, generator=g, dtype=torch.float64)
        V = WE.wino_v64(x).view(4, 4, B, H // 2, W // 2, C)
        U = torch.einsum("xk,ockl,yl->ocxy", G, w, G)
        y = torch.einsum("ax,by,ocxy,xynhwc->nohawb", AT, AT, U, V).reshape(B, O, H, W)
        _agree12(y, F.conv2d(x, w, padding=1), "wino_v64")
        assert (WE.wino_v64(x, absolute=True) >= WE.wino_v64(x).abs() - 1e-12).all()
        _agree12(F.conv2d(gy, w.flip(2, 3).transpose(0, 1), padding=1), F.conv_transpose2d(gy, w, padding=1), "dgrad as a forward conv")
        ww = w.clone().requires_grad_(True)
        (gw,) = torch.autograd.grad(F.conv2d(x, ww, padding=1), ww, gy)
        _agree12(WE.wgrad64(gy, x), gw, "wgrad64")


# ---------------------------------------------------------------------------------------------------------------------------------
# tests/test_gpu_wgrad_edges.py: what each row claims about its launch (kernel, tile, stage depth, scale table, grouped taps, twin,
# chunk, table rows, empty splits, family), held against csrc/wgrad_route.h through tests/host/wgrad_route_dump.cpp (a stand-alone
# host program under AddressSanitizer and UBSan), and its fp64 reference tied to ATen float64.  No GPU.
# ---------------------------------------------------------------------------------------------------------------------------------
def _wgrad_edges():
    import test_gpu_wgrad_edges as GE
    return GE


def test_wgrad_edges_rows_sit_on_their_edges(tmp_path):
    import re
    import subprocess
    GE = _wgrad_edges()
    exe = str(tmp_path / "wgrad_route_dump")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    flags = "-x c++ -std=c++17 -O1 -g -Wall -Werror -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined"
    built = subprocess.run([hipcc] + flags.split() + ["-I", os.path.join(ROOT, "gif_amd", "csrc"),
                                                      os.path.join(ROOT, "tests", "host", "wgrad_route_dump.cpp"), "-o", exe],
                           capture_output=True, text=True, timeout=600)
    assert built.returncode == 0, built.stderr[-4000:]
    names = [r.name for r in GE.ROWS]
    assert len(set(names)) == len(names)
    cases = [(r, m) for r in GE.ROWS for m in r.modes]
    assert set(GE.CLAIMS) == {(r.name, m) for r, m in cases}, "CLAIMS must cover every (row, mode) and nothing else"
    args = [a for r, m in cases for a in GE.dump_args(r, m)]
    ran = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300)
    assert ran.returncode == 0, (ran.returncode, ran.stderr[-4000:])
    lines = ran.stdout.splitlines()
    assert len(lines) == len(cases)
    for (r, m), l in zip(cases, lines):
        B, Hs, Ws, Cs, Cb, KH, KW, s, p = GE.geom_of(r, m)
        assert Cs % (8 if m == "f16" else 4) == 0 and Cb % (8 if m == "f16" else 4) == 0 and 1 <= KH <= 3 and 1 <= KW <= 3 and s in (1, 2), r.name
        assert min(GE.big_hw(GE.geom_of(r, m))) >= 1, r.name
        assert GE.claim_of_line(l, r, m) == GE.CLAIMS[r.name, m], (r.name, m, l)
    C = GE.CLAIMS
    by = {r.name: r for r in GE.ROWS}
    # ---- the facts the row comments name
    for route in ("thin", "sq", "tiny"):
        for m in GE.ALL:
            assert C[f"ch_{route}_n16", m][1:4] == (32, 1, 0) and C[f"ch_{route}_n33_1", m][1] == 64 and C[f"ch_{route}_n33_2", m][1] == 32
            assert C[f"ch_{route}_n130_5", m][1:4:2] == (32, 0) and C[f"ch_{route}_n130_6", m][1:4:2] == (32, 1) and C[f"ch_{route}_b3_n2", m][1] == 64
    for m in GE.FP32_MODES:
        assert C["sm_256x257", m] == ("small", 320, 0, 50, 1) and C["sm_1x65537", m] == ("small", 320, 0, 51, 1)
        assert C["sm_not_255x257", m][0].startswith("mfma f32 32x32 ") and C["tb_65", m][0] == "mfma f32 128x128 w2x2 glds0 bkp32 tab0 x3=0"
        assert C["tb_65", m][2] == 65 and C["tb_45", m][2] == 45 and " tab1 " in C["tb_45", m][0]
    assert 65537 - 204 * 320 == 257 and 205 * 320 >= 65537  # sm_1x65537: the last non-empty split
    assert C["sm_not_255x257", "native"][1:4:2] == (608, 5) and C["hl_511", "f16"][1:4:2] == (576, 2)  # empty splits with the library's own count
    assert C["tb_f16_17", "f16"][:3] == ("mfma f16 128x128 w2x2 glds1 bkp32 tab1 x3=0", 4096, 17)
    assert C["tb_f16_9", "f16"][:3] == ("mfma f16 256x256 w2x4 glds1 bkp32 tab1 x3=0", 2048, 9)
    assert C["tb_b4_n3", "native"][1:3] == (64, 3) and C["tb_b_past", "native"][1:3] == (64, 3)
    taps = {"tp_cb4": (9, 1), "tp_cb12": (9, 1), "tp_cb16": (8, 2), "tp_cb20": (6, 2), "tp_cb24": (5, 2), "tp_cb28": (4, 3), "tp_cb32": (4, 3),
            "tp_cb24_2x2": (4, 1), "tp_cb24_1x3": (3, 1), "tp_cb24_rows2": (5, 2)}
    for n, (tpt, tg) in taps.items():
        assert C[n, "f16x2"][0].startswith(f"h2v2 tab0 taps tpt{tpt} tg{tg} + mfma f32 128x32 w2x1 "), n
        T, Cb = by[n].geom[5] * by[n].geom[6], by[n].geom[4]
        assert tpt == min(128 // Cb, T) and tg == -(-T // tpt)
    assert {T - (tg - 1) * tpt for T, (tpt, tg) in ((9, taps[n]) for n in ("tp_cb16", "tp_cb28", "tp_cb32"))} == {1}  # a last group of ONE tap
    assert C["tp_cb24_1x1", "f16x2"][0].startswith("mfma f32 128x32 w2x1 glds1 bkp32 tab0 x3=2 + ")
    assert {C[n, "f16"][0] for n in by if n.startswith("hl_") and n != "hl_511"} == {"halo tr1"} and C["hl_511", "f16"][0].startswith("mfma f16 32x32 ")
    patches = {n: by[n].geom[0] * -(-by[n].geom[1] // 16) * -(-by[n].geom[2] // 16) for n in by if n.startswith("hl_")}
    assert (patches["hl_513"], patches["hl_1025"], patches["hl_511"], patches["hl_xsample_sc"]) == (513, 1025, 511, 578)
    for n in by:
        if n.startswith("cu16_") or n in ("lad_tab16", "tb_b4_n3", "tb_45"):
            assert all(" bkp16 " in C[n, m][0] for m in by[n].modes), n
        if n.startswith("cu_") and n.endswith(("_sc", "_sc_s2")) and n != "cu_b3_1x32_sc":
            assert " glds0 " in C[n, "native"][0], n
    gg = GE.GUARD_GEOM
    assert gg[0] * gg[1] * gg[2] == 160 and -(-160 // GE.GUARD_NSPLIT) <= 32 and (GE.GUARD_NSPLIT - 1) * 32 >= 160  # the last split is empty
    # ---- section 5 names every launch of the default-knob route table (conv geometries); small and halo have sections of their own
    def sig(launch):
        return re.sub(r" tpt\d+ tg\d+", "", launch)
    ladder = {sig(C[r.name, m][0]) for r in GE.ROWS if r.ladder for m in r.modes}
    with open(os.path.join(ROOT, "tests", "golden", "wgrad_route_table.txt")) as f:
        table = set()
        for l in f.read().splitlines():
            if l.startswith(("GIF_", "planes")):
                continue
            launch = re.search(r" -> (.*?) ; RP", l).group(1)
            table.add(sig(re.sub(r" thr\d+ wgs\d+", "", launch).replace(" + twin ", " + ")))
    assert {"small", "halo tr1"} <= table and {"small", "halo tr1"} <= {c[0] for c in C.values()}
    assert table - {"small", "halo tr1"} <= ladder, sorted(table - ladder)
    assert len(ladder) >= 25, sorted(ladder)


def test_wgrad_edges_reference_is_the_weight_gradient():
    """wgrad64 against autograd of F.conv2d in ATen float64: non-square kernels, stride 2, padding, per-sample scales, wscale."""
    GE = _wgrad_edges()
    g = torch.Generator().manual_seed(12)
    for B, Hs, Ws, Cs, Cb, KH, KW, s, p in ((2, 5, 7, 3, 4, 3, 3, 1, 1), (2, 5, 7, 3, 4, 3, 3, 2, 0), (3, 4, 6, 2, 5, 1, 3, 1, 0),
                                            (1, 5, 6, 4, 3, 3, 1, 1, 1), (2, 4, 4, 3, 3, 2, 2, 1, 1), (2, 3, 5, 2, 2, 2, 3, 1, 0),
                                            (2, 1, 9, 3, 2, 3, 3, 1, 1), (1, 6, 5, 2, 3, 1, 1, 1, 0), (2, 3, 4, 3, 2, 2, 3, 2, 0)):
        Hb, Wb = GE.big_hw((B, Hs, Ws, Cs, Cb, KH, KW, s, p))
        x = torch.randn(B, Cb, Hb, Wb, generator=g, dtype=torch.float64)
        gy = torch.randn(B, Cs, Hs, Ws, generator=g, dtype=torch.float64)
        ss, bs = torch.rand(B, Cs, generator=g, dtype=torch.float64) + 0.5, torch.rand(B, Cb, generator=g, dtype=torch.float64) + 0.5
        for sa, sb, wscale in ((None, None, 1.0), (ss, bs, -0.37), (ss, None, 1.0)):
            w = torch.zeros(Cs, Cb, KH, KW, dtype=torch.float64, requires_grad=True)
            xs = x if sb is None else x * sb[:, :, None, None]
            gs = gy if sa is None else gy * sa[:, :, None, None]
            y = F.conv2d(xs, w, stride=s, padding=p)
            assert y.shape[2:] == (Hs, Ws)
            (gw,) = torch.autograd.grad(y, w, gs)
            _agree12(GE.wgrad64(gy, x, KH, KW, s, p, sa, sb, wscale), wscale * gw, "wgrad64")
            R = GE.wgrad64(gy, x, KH, KW, s, p, sa, sb, wscale, absolute=True)
            assert (R >= GE.wgrad64(gy, x, KH, KW, s, p, sa, sb, wscale).abs() - 1e-12).all()
    # a one-row map: the ky != 1 taps of a padded 3x3 only ever read padding
    R = GE.wgrad64(torch.ones(1, 2, 1, 9), torch.ones(1, 2, 1, 9), 3, 3, 1, 1, absolute=True)
    assert (R[:, :, 0] == 0).all() and (R[:, :, 2] == 0).all() and (R[:, :, 1] > 0).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# tests/test_gpu_raster_edges.py: the edge each row claims, recomputed from the constants of csrc/rasterize.hip by a numpy restatement
# of front_facing / face_bbox / the tile and band arithmetic, the C oracle's behaviour the rows rely on, and the backward's fp64
# restatement tied to central differences.  No GPU.
# ---------------------------------------------------------------------------------------------------------------------------------
def _raster_edges():
    import test_gpu_raster_edges as RE
    return RE


def test_raster_edges_constants_are_the_sources():
    """A constant changed in rasterize.hip fails here; it does not silently move a row off its edge."""
    import re
    RE = _raster_edges()
    with open(os.path.join(ROOT, "gif_amd", "csrc", "rasterize.hip")) as f:
        src = f.read()

    def one(pattern):
        m = re.findall(pattern, src)
        assert len(m) == 1, (pattern, m)
        return m[0]

    got = {name: int(one(r"constexpr int %s = (\d+);" % name))
           for name in ("kTile", "kSmallArea", "kBinThreads", "kMaxLdsTiles", "kTileThreads", "kBwdWaves")}
    # the band height of the backward is the tile edge
    one(r"b0 = y_min / kTile; b1 = y_max / kTile;")
    one(r"const int r0 = max\(y_min, band \* kTile\), r1 = min\(y_max, band \* kTile \+ kTile - 1\);")
    one(r"int bwd_bands_per_image\(int H\) \{ return \(H \+ kTile - 1\) / kTile; \}")
    got["kBand"] = got["kTile"]
    assert got == RE.K
    # the expressions geometry() and bands() restate, and the predicates the rows name
    assert got["kTile"] == 1 << 6
    one(r"tx0 = x_min >> 6; tx1 = x_max >> 6; ty0 = y_min >> 6; ty1 = y_max >> 6;")
    one(r"const bool lds = nt <= kMaxLdsTiles;")
    one(r"if \(area > 0 && area <= kSmallArea\)")
    one(r"__ballot\(area > kSmallArea\)")
    one(r"for \(int j0 = 0; j0 < n; j0 \+= kThreads\)")
    one(r"const uint32_t pre_idx = j_first < F \? min\(cand\[j_first\], \(uint32_t\)\(F - 1\)\) : 0u;")
    assert len(re.findall(r"raster_tiles<T, (?:true|false), kTileThreads><<<grid, kTileThreads, 0, s>>>", src)) == 2
    one(r"raster_bin<T><<<dim3\(\(unsigned\)gif::cdiv\(F, kBinThreads\), \(unsigned\)B\), kBinThreads, 0, s>>>")
    one(r"const int fi = blockIdx\.x \* kBwdWaves \+ \(threadIdx\.x >> 6\), band = blockIdx\.y, b = blockIdx\.z;")
    one(r"inline long pad2\(long n\) \{ return \(n \+ 1\) / 2 \* 2; \}")
    one(r"for \(int p = lane; p < n; p \+= 64\)")


def _raster_rows(RE):
    return list(RE.FROWS) + list(RE.WS_ROWS)


def test_raster_edges_forward_rows_sit_on_their_edges():
    RE = _raster_edges()
    rows = _raster_rows(RE)
    assert len({r.name for r in rows}) == len(rows)
    seen = set()
    for row in rows:
        fv64, fv32 = RE.face_array(row.faces, np.float64), RE.face_array(row.faces, np.float32)
        B, F = fv64.shape[:2]
        assert fv64.shape == (B, F, 3, 3), row.name
        # the input constraints: exact in fp32, |x|, |y| < 2^31 and finite, no face with z of mixed sign or zero (a NaN z aside), no
        # caller depth of -0.0
        assert np.array_equal(fv32.astype(np.float64), fv64, equal_nan=True), row.name
        assert np.isfinite(fv64[..., :2]).all() and (np.abs(fv64[..., :2]) < 2.0 ** 31).all(), row.name
        z = fv64[..., 2]
        zs = np.where(np.isnan(z), np.nanmax(z, -1, keepdims=True), z)
        assert ((zs > 0).all(-1) | (zs < 0).all(-1)).all(), row.name
        for fv in (fv32, fv64):
            depth = RE.caller_buffers(row, fv)[0]
            assert depth.dtype == fv.dtype and not (np.signbit(depth) & (depth == 0)).any() and not np.isnan(depth).any(), row.name
        g32, g64 = RE.geometry(fv32, row.H, row.W), RE.geometry(fv64, row.H, row.W)
        assert np.array_equal(g32["lists"], g64["lists"]) and np.array_equal(g32["box"], g64["box"]), row.name
        g = g32
        assert g["lists"].max() <= F and B <= 65535 and row.H * row.W <= 270000, row.name
        claim = row.claim or {}
        assert claim, row.name
        for key, want in claim.items():
            seen.add(key)
            if key == "F":
                assert F == want, (row.name, F)
            elif key == "groups":
                assert -(-F // RE.K["kBinThreads"]) == want, (row.name, F)
            elif key == "nt":
                assert g["nt"] == want, (row.name, g["nt"])
            elif key == "lists":
                for (b, t), n in want.items():
                    assert g["lists"][b, t] == n, (row.name, b, t, int(g["lists"][b, t]), n)
            elif key == "areas":
                for (f, t), a in want.items():
                    assert g["area"](0, f, t) == a, (row.name, f, t, g["area"](0, f, t), a)
            else:
                assert key in ("cover", "tri", "seed", "split", "only_face", "tie_winner", "tie_losers", "shared"), (row.name, key)
    assert seen >= {"F", "groups", "nt", "lists", "areas", "cover", "tri"}
    by = {r.name: r for r in rows}
    geo = lambda n: RE.geometry(RE.face_array(by[n].faces, np.float32), by[n].H, by[n].W)  # noqa: E731
    # both sides of every predicate of the table
    assert geo("nt1024")["nt"] == RE.K["kMaxLdsTiles"] and geo("nt1025")["nt"] == RE.K["kMaxLdsTiles"] + 1
    assert [int(geo(f"list_{n}")["lists"][0, 0]) for n in (511, 512, 513, 1025)] == [511, 512, 513, 1025]
    assert 2 * RE.K["kTileThreads"] < 1025 and RE.K["kTileThreads"] == 512
    assert [geo(n)["area"](0, 0, 0) for n in ("cls_4x4", "cls_2x8", "cls_1x16", "cls_16x1")] == [RE.K["kSmallArea"]] * 4
    assert [geo(n)["area"](0, 0, 0) for n in ("cls_1x17", "cls_2x9")] == [RE.K["kSmallArea"] + 1, RE.K["kSmallArea"] + 2]
    g = geo("list_513_wave")
    assert all(g["area"](0, f, 0) > RE.K["kSmallArea"] for f in range(513))  # every ballot bit of round 0, bit 63 included
    g = geo("list_513")
    assert all(0 < g["area"](0, f, 0) <= RE.K["kSmallArea"] for f in range(513))
    assert [by[n].faces[0].__len__() for n in ("bin_f1", "bin_f255", "bin_f256", "bin_f257")] == [1, 255, 256, 257]
    assert geo("ws_x")["lists"].tolist() != geo("ws_y")["lists"].tolist()
    assert RE.face_array(RE.WS_X.faces).shape == RE.face_array(RE.WS_Y.faces).shape and (RE.WS_X.H, RE.WS_X.W) == (RE.WS_Y.H, RE.WS_Y.W)


def test_raster_edges_the_oracle_behaves_as_the_rows_assume():
    RE = _raster_edges()
    by = {r.name: r for r in RE.FROWS}

    def run(name, variant="f32"):
        fv, fc, bufs, (d, t, p) = RE.forward_case(name, variant)
        return fv, bufs, d, t, p

    for row in RE.FROWS:
        claim = row.claim
        for variant in RE.VARIANTS:
            fv, bufs, d, t, p = run(row.name, variant)
            covered = t >= 0
            assert ((t == -7) | covered).all() and t.max() < fv.shape[1], row.name
            # an untouched pixel keeps all three caller values
            assert np.array_equal(d[~covered], bufs[0][~covered]) and np.array_equal(p[~covered], bufs[2][~covered]), row.name
            assert not np.isnan(d).any() and not np.isnan(p).any(), row.name
            want = claim.get("cover")
            if isinstance(want, dict):
                want = want[variant[1:] == "64" and "f64" or "f32"]
            if want is not None:
                assert int(covered.sum()) == want, (row.name, variant, int(covered.sum()))
            if want != 0:
                assert covered.any(), (row.name, variant)  # every row that claims coverage has some
            for (b, y, x), f in claim.get("tri", {}).items():
                assert t[b, y, x] == f, (row.name, variant, (b, y, x), int(t[b, y, x]))
            if "only_face" in claim:
                assert set(np.unique(t[covered])) == {claim["only_face"]}
            if "tie_winner" in claim:
                a, b_, c_ = sorted((claim["tie_winner"],) + claim["tie_losers"])
                assert np.array_equal(fv[0, a], fv[0, b_]) and np.array_equal(fv[0, a], fv[0, c_])
                own = t[0] == claim["tie_winner"]
                assert own.sum() == 136 and not np.isin(t, claim["tie_losers"]).any()  # rt(3, 3, 16): the lowest index wins every pixel
    # the tail face of the bin rows: without it (5, 5) belongs to another face or to nobody
    for name in ("bin_f255", "bin_f256", "bin_f257"):
        _, _, _, t, _ = run(name)
        assert (t == 0).sum() > 100 and len(np.unique(t)) == len(by[name].faces[0]) + 1  # every face wins a pixel (and -7 is left)
    # list rows: every tiny face wins a pixel, so a face dropped from a round changes the image
    for name, F in (("list_511", 514), ("list_512", 515), ("list_513", 516), ("list_1025", 1028), ("list_513_wave", 513), ("list_600", 602)):
        _, _, _, t, _ = run(name)
        assert len(np.unique(t[t >= 0])) == F, name
    # coplanar tie: the shared pixels (the hypotenuse x + y = 48) go to face 0 whichever face comes first
    for variant in ("f32", "f64"):
        fv, bufs, d, t, p = run("tie_coplanar", variant)
        swapped = RE.oracle_run(by["tie_coplanar"], np.ascontiguousarray(fv[:, ::-1]), None, bufs)[1]
        shared = (t[0] == 0) & (swapped[0] == 0)
        ys, xs = np.nonzero(shared)
        assert shared.sum() == by["tie_coplanar"].claim["shared"] and (xs + ys == 48).all(), (variant, int(shared.sum()))
        assert (d[0][t[0] >= 0] == 2).all()
    # seeded depth, positive z
    for variant in RE.VARIANTS:
        fv, bufs, d, t, p = run("seed_pos", variant)
        first_t, zp = RE._first_pass(by["seed_pos"], fv)
        x = np.arange(64)[None, None, :]
        y = np.arange(64)[None, :, None]
        cov = first_t >= 0
        caller, tie = cov & (x < RE.SEED_SPLIT_X), cov & (x >= RE.SEED_SPLIT_X) & (y == RE.SEED_TIE_Y)
        assert caller.sum() >= 10 and tie.sum() >= 4 and (cov & ~caller & ~tie).sum() >= 10
        assert (t[caller] == -7).all() and (d[caller] == 0.25).all() and np.array_equal(p[caller], bufs[2][caller])  # the caller wins
        assert (t[tie] == 0).all() and np.array_equal(d[tie], zp[tie]) and np.array_equal(bufs[0][tie], zp[tie])  # the face wins the tie
        assert (t[cov & ~caller] == 0).all() and np.isinf(d[~cov]).all()
    # negative z: the two faces split the 36 pixels; against negative caller depths only the pixels nearer than the caller change
    for variant in ("f32", "f64"):
        _, _, d, t, _ = run("neg_z", variant)
        assert sorted(((t == 0).sum(), (t == 1).sum())) == [10, 26] and (d[t >= 0] < 0).all()
        _, bufs, d2, t2, _ = run("seed_neg", variant)
        won = t2 >= 0
        assert 0 < won.sum() < 36 and (d2[won] <= bufs[0][won]).all() and np.array_equal(d2[won], d[won]) and np.array_equal(t2[won], t[won])
        lost = (t >= 0) & ~won
        assert (d[lost] > bufs[0][lost]).all() and (bufs[0][lost] == -2.25).all() and (bufs[0][won] == -2.25).any() and (bufs[0][won] == -1).any()
    # the rounding-degenerate face: its fp32 den is exactly 0 and it writes -0.0 barycentrics
    _, _, _, t, p = run("degen_round", "f32")
    assert (t[0, :2] == 0).all() and (t[0, 2:] == -7).all()
    assert (p[0, :2, :, 0] == 1).all() and (p[0, :2, :, 1:] == 0).all() and np.signbit(p[0, :2, :, 1:]).any()
    _, _, _, t, _ = run("degen_round", "f64")
    assert (t[0, 0] == 0).all() and (t[0, 1:] == -7).all()


def test_raster_edges_backward_rows_sit_on_their_edges():
    RE = _raster_edges()
    assert len({r.name for r in RE.BROWS}) == len(RE.BROWS)
    seen = set()
    for row in RE.BROWS:
        c = RE.backward_case(row.name)
        fv = c["fv"].numpy()
        B, F = fv.shape[:2]
        assert 16 <= row.W <= 64 or row.name in RE.B_DEGENERATE
        b0, b1, n = RE.bands(fv, row.H, row.W)
        npix = c["ref"]["npix"]
        for key, want in row.claim.items():
            seen.add(key)
            for k, v in want.items():
                if key == "bands":
                    assert (b0[0, k], b1[0, k]) == v, (row.name, k, (int(b0[0, k]), int(b1[0, k])))
                elif key == "n":
                    assert n(0, k[0], k[1]) == v, (row.name, k, n(0, *k))
                else:
                    assert key == "wins" and bool(npix[0, k] > 0) == v, (row.name, k, int(npix[0, k]))
        assert b1.max() < -(-row.H // RE.K["kBand"])
        # a face owns pixels only inside its own bands
        for b, f in zip(*np.nonzero(npix.numpy() > 0)):
            ys = np.nonzero((c["tri"][b].numpy() == f).any(1))[0]
            assert b0[b, f] <= ys.min() // 64 and ys.max() // 64 <= b1[b, f], (row.name, b, f)
        # the accuracy condition: every face that wins a pixel is well shaped
        if row.name in RE.B_DEGENERATE:
            p = fv[0, 0, :, :2]  # its fp32 den is exactly zero
            v0, v1 = p[2] - p[0], p[1] - p[0]
            d00, d01, d11 = v0 @ v0, v0 @ v1, v1 @ v1
            assert np.float32(d00 * d11) - np.float32(d01 * d01) == 0 and d00.dtype == np.float32
            continue
        p = fv[..., :2].astype(np.float64)
        v0, v1, v2 = p[:, :, 2] - p[:, :, 0], p[:, :, 1] - p[:, :, 0], p[:, :, 2] - p[:, :, 1]
        d00, d01, d11 = (v0 * v0).sum(-1), (v0 * v1).sum(-1), (v1 * v1).sum(-1)
        den = d00 * d11 - d01 * d01  # (twice the area) squared
        longest = np.sqrt(np.maximum(np.maximum(d00, d11), (v2 * v2).sum(-1)))
        win = npix.numpy() > 0
        assert (den[win] / (d00 * d11)[win] >= 0.25).all(), row.name
        assert (np.sqrt(den[win]) / longest[win] >= 2).all(), row.name  # the smallest altitude
        assert (npix.numpy()[win] >= 10).all(), row.name
    assert seen == {"bands", "n", "wins"}
    ns = RE.BROW["bw_n"].claim["n"]
    assert sorted(ns.values()) == [63, 64, 65, 200]
    assert [len(RE.BROW[f"bw_f{k}"].faces[0]) for k in (1, 4, 5, 7)] == [1, 4, 5, 7] and RE.K["kBwdWaves"] == 4
    assert [-(-RE.BROW[n].H // 64) for n in ("bw_h64", "bw_h65", "bw_h192")] == [1, 2, 3]


@pytest.mark.parametrize("name", ["bw_f4", "bw_hidden"])
def test_raster_edges_backward_restatement_is_the_derivative(name):
    """The autograd gradient of bwd_ref equals a central difference of the interpolated image in fp64, tri held fixed."""
    RE = _raster_edges()
    c = RE.backward_case(name)
    fv, fc, tri, g = c["fv"].double(), c["fc"].double(), c["tri"], c["g"].double()
    B, F = fv.shape[:2]
    bi, yi, xi = torch.nonzero(tri >= 0, as_tuple=True)
    fo = bi * F + tri[bi, yi, xi].long()

    def loss(v, a):
        w, _ = RE.bary64(v.reshape(B * F, 3, 3)[fo][:, :, :2], torch.stack([xi, yi], -1).double())
        return ((w[..., None] * a.reshape(B * F, 3, 3)[fo]).sum(1) * g[bi, yi, xi]).sum()

    gen = torch.Generator().manual_seed(3)
    delta = 1e-6
    for k in range(4):
        dv = torch.randn(fv.shape, generator=gen, dtype=torch.float64)
        da = torch.randn(fc.shape, generator=gen, dtype=torch.float64)
        fd = (loss(fv + delta * dv, fc + delta * da) - loss(fv - delta * dv, fc - delta * da)) / (2 * delta)
        an = (c["ref"]["gfv"] * dv).sum() + (c["ref"]["gfc"] * da).sum()
        assert abs(fd.item() - an.item()) <= 1e-6 * max(abs(an.item()), 1.0), (k, fd.item(), an.item())
    assert (c["ref"]["gfv"][..., 2] == 0).all() and (c["ref"]["Rv"] >= c["ref"]["gfv"].abs() - 1e-12).all()
    assert (c["ref"]["Rc"] >= c["ref"]["gfc"].abs() - 1e-12).all()


def test_raster_edges_gather_reference_is_the_gradient_of_face_vertices():
    RE = _raster_edges()
    for name, B, V in RE.GROWS:
        faces = RE.gather_faces(name, V)
        assert int(faces.max()) < V - 1 and B * V in (255, 256, 257, 258, 16)
        gface = torch.randint(-8, 9, (B, faces.shape[0], 3, 3), generator=torch.Generator().manual_seed(1)).double()
        x = torch.zeros(B, V, 3, dtype=torch.float64, requires_grad=True)
        (gx,) = torch.autograd.grad(x[:, faces], x, gface)
        assert torch.equal(gx, RE.gather_ref(gface, faces, V).double())
        assert gface.abs().max() * faces.shape[0] * 3 < 2 ** 24  # every fp32 sum is exact
