"""-m gpu: optimiser state that outlives a process — FlatAdam's state_dict() handed to torch.optim.Adam and
back, parameters that join a live optimiser (progressive growing), and a GifTrainer continued from its own checkpoint.

  a. FlatAdam -> torch.optim.Adam, directly and through torch.save / torch.load: no `step` tensor is shared, with another
     parameter's or with the donor's, every count advances by one per step, and both optimisers go on in step.
  b. torch.optim.Adam -> FlatAdam with unequal counts (`late` got its first gradient at the third step): every parameter is
     corrected by its own count, and the counts come back out of state_dict().
  c. Growth: a second FlatAdam over a larger bucket loads the first one's state; `late` starts at count 0 like in torch.  The same
     again under loss scaling with one skipped step.
  d. The predicate that decides what the generator's bucket holds against what autograd really leaves without a gradient.
  e. A trainer saved after two iterations and continued by a fresh one equals the uninterrupted run bit for bit.
  f. A checkpoint of the fused trainer continued with torch.optim.Adam (what the reference's train.py:392-394 would do).

Reference of every FlatAdam step: adam_ref.adam_ref, fp64 over the optimiser's own operands read before the step, with the bounds
and the tolerance of test_gpu_linear_reduce_routes.test_flat_adam (TOL 1e-6 against |m0| + |g|, |v| and |p0| + 4 |upd|).  An
optimiser whose parameters carry unequal counts forms its bias corrections on the device from the fp32 betas, like a loss-scaled
step (device_step=True in the reference).  Two fp32 optimisers are compared at 2e-6 (test_gpu_round2's bound for the same pair)."""
import contextlib
import io

import pytest
import torch

import adam_ref
from gpu_util import assert_close

pytestmark = pytest.mark.gpu

BETAS = [(0.0, 0.99 ** 0.8), (0.9, 0.999)]
BETA_IDS = ["trainer_betas", "default_betas"]
LR, EPS = 2e-3, 1e-8
# 4097 and 8190: two 4096-float chunks each (the count offset is per chunk); `late` is one of them.  The last one stays outside
# the bucket in (a) and (b).  Chunk and alignment edges proper: test_gpu_linear_reduce_routes.test_flat_adam.
SIZES = [5, 4097, 3, 8190, 64, 7]
LATE, OUT = 3, 5


def _rng(seed):
    return torch.Generator().manual_seed(seed)


def _bag(seed):
    g = _rng(seed)
    return [torch.nn.Parameter(torch.randn(n, generator=g).cuda()) for n in SIZES]


def _grads(g, idxs, gain=1.0):
    return {i: torch.randn(SIZES[i], generator=g) * gain * (10.0 ** (i % 3 - 1)) for i in idxs}


def _feed(bucket, params, grads):
    """Write the gradients into the bucket's views, the way test_flat_adam does."""
    where = {id(p): v for p, v in zip(bucket.params, bucket.views)}
    for i, gr in grads.items():
        where[id(params[i])].copy_(gr)


def _counts(opt, params):
    """{index in params: step} of an optimiser's state_dict()."""
    sd = opt.state_dict()
    order = sd["param_groups"][0]["params"]
    assert len(order) == len(params)
    return {i: float(sd["state"][k]["step"]) for i, k in enumerate(order) if k in sd["state"]}


def _checked_step(opt, bucket, params, grads, counts, betas, what, device_step, emas=None, decay=None, inv=None, found=None,
                  grad_scale=1.0):
    """One FlatAdam step, every parameter checked against adam_ref with ITS count counts[i] (the count after this step)."""
    _feed(bucket, params, grads)
    before = {i: (params[i].detach().cpu().double(), opt.state[params[i]]["exp_avg"].cpu().double(),
                  opt.state[params[i]]["exp_avg_sq"].cpu().double(), None if emas is None else emas[i].detach().cpu().double())
              for i in grads}
    opt.step(ema_decay=decay, inv_grad_scale=inv, found_inf=found)
    torch.cuda.synchronize()
    for i, gr in grads.items():
        p0, m0, v0, e0 = before[i]
        gd = gr.double() * grad_scale
        pr, mr, vr, upd = adam_ref.adam_ref(p0, gd, m0, v0, counts[i], LR, betas[0], betas[1], EPS, device_step)
        Rm, Rv, Rp = adam_ref.adam_bounds(p0, gd, m0, vr, upd)
        w = f"{what} p{i} n{SIZES[i]} t{counts[i]}"
        adam_ref.check(opt.state[params[i]]["exp_avg"], mr, Rm, f"{w} m")
        adam_ref.check(opt.state[params[i]]["exp_avg_sq"], vr, Rv, f"{w} v")
        adam_ref.check(params[i], pr, Rp, f"{w} p")
        if emas is not None and decay is not None:
            df = adam_ref.f32(decay)
            pn = params[i].detach().cpu().double()  # (the kernel blends its own new p)
            adam_ref.check(emas[i], e0 * df + (1 - df) * pn, e0.abs() * df + (1 - df) * pn.abs(), f"{w} ema")


# ---------------------------------------------------------------------------------------------------------------------------------
# a. FlatAdam -> torch.optim.Adam
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["direct", "pickle"])
@pytest.mark.parametrize("betas", BETAS, ids=BETA_IDS)
def test_handover_flat_adam_to_torch_adam(betas, route):
    from gif_amd.optim import FlatAdam
    from gif_amd.train_step import FlatGradBucket
    params = _bag(1)
    inb = [i for i in range(len(SIZES)) if i != OUT]
    bucket = FlatGradBucket(params, active=lambda p: p is not params[OUT])
    opt = FlatAdam(params, lr=LR, betas=betas, eps=EPS, bucket=bucket)
    g = _rng(2)
    for _ in range(3):
        _feed(bucket, params, _grads(g, inb))
        opt.step()
    sd = opt.state_dict()
    if route == "pickle":  # what checkpoint.save_checkpoint / load_checkpoint do
        buf = io.BytesIO()
        torch.save(sd, buf)
        buf.seek(0)
        sd = torch.load(buf, weights_only=False)
    clones = [torch.nn.Parameter(p.detach().clone()) for p in params]
    opt_t = torch.optim.Adam(clones, lr=LR, betas=betas, eps=EPS)
    opt_t.load_state_dict(sd)
    assert clones[OUT] not in opt_t.state or not opt_t.state[clones[OUT]], "state for a parameter that never had a gradient"
    steps = [opt_t.state[clones[i]]["step"] for i in inb]
    assert all(float(s) == 3.0 for s in steps), [float(s) for s in steps]
    ptrs = [s.untyped_storage().data_ptr() for s in steps]
    assert len(set(ptrs)) == len(ptrs), "two parameters of the loaded optimiser share one `step` tensor"
    donor = set(st["step"].untyped_storage().data_ptr() for st in opt.state.values() if st)
    assert not donor & set(ptrs), "the loaded optimiser holds the donor's own `step` tensor"
    for j in (1, 2):
        grads = _grads(g, inb)
        for i, c in enumerate(clones):
            c.grad = grads[i].cuda() if i in grads else None
        opt_t.step()
        assert all(float(opt_t.state[clones[i]]["step"]) == 3.0 + j for i in inb), \
            (j, [float(opt_t.state[clones[i]]["step"]) for i in inb])
        assert _counts(opt, params) == {i: 2.0 + j for i in inb}, "the loaded optimiser's step moved the donor's count"
        _feed(bucket, params, grads)
        opt.step()
        assert _counts(opt, params) == {i: 3.0 + j for i in inb}
    for i in inb:
        assert_close(params[i], clones[i], 2e-6, f"parameter {i} two steps after the hand-over ({route})")
        # (1 - beta2 is formed in fp32 by the kernel and in double by torch: test_gpu_round2 holds exp_avg_sq of the pair to 5e-5)
        assert_close(opt.state[params[i]]["exp_avg_sq"], opt_t.state[clones[i]]["exp_avg_sq"], 5e-5, f"exp_avg_sq {i} ({route})")
    assert torch.equal(params[OUT], clones[OUT])


# ---------------------------------------------------------------------------------------------------------------------------------
# b. torch.optim.Adam -> FlatAdam, unequal counts
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("betas", BETAS, ids=BETA_IDS)
def test_handover_torch_adam_to_flat_adam_keeps_each_count(betas):
    from gif_amd.optim import FlatAdam
    from gif_amd.train_step import FlatGradBucket
    params = _bag(3)
    clones = [torch.nn.Parameter(p.detach().clone()) for p in params]
    opt_t = torch.optim.Adam(clones, lr=LR, betas=betas, eps=EPS)
    inb = [i for i in range(len(SIZES)) if i != OUT]
    g = _rng(4)
    for it in range(5):
        grads = _grads(g, [i for i in inb if i != LATE or it >= 2])
        for i, c in enumerate(clones):
            c.grad = grads[i].cuda() if i in grads else None
        opt_t.step()
    assert [float(opt_t.state[clones[i]]["step"]) for i in inb] == [3.0 if i == LATE else 5.0 for i in inb]
    with torch.no_grad():
        for p, c in zip(params, clones):
            p.copy_(c)
    bucket = FlatGradBucket(params, active=lambda p: p is not params[OUT])
    opt = FlatAdam(params, lr=LR, betas=betas, eps=EPS, bucket=bucket)
    opt.load_state_dict(opt_t.state_dict())
    assert _counts(opt, params) == {i: (3.0 if i == LATE else 5.0) for i in inb}
    for j in (1, 2, 3):
        grads = _grads(g, inb)
        for i, c in enumerate(clones):
            c.grad = grads[i].cuda() if i in grads else None
        opt_t.step()
        counts = {i: (3 if i == LATE else 5) + j for i in inb}
        _checked_step(opt, bucket, params, grads, counts, betas, f"torch->flat step{j}", device_step=True)
    assert _counts(opt, params) == {i: (6.0 if i == LATE else 8.0) for i in inb}, "a parameter without state must have no entry"
    for i in inb:
        assert_close(params[i], clones[i], 2e-6, f"parameter {i} three steps after the hand-over")
    assert torch.equal(params[OUT], clones[OUT]) and params[OUT].grad is None


# ---------------------------------------------------------------------------------------------------------------------------------
# c. growth: `late` joins with a new bucket and a new optimiser
# ---------------------------------------------------------------------------------------------------------------------------------
def test_growth_late_parameter_starts_at_count_zero():
    from gif_amd.optim import FlatAdam
    from gif_amd.train_step import FlatGradBucket
    betas, decay = BETAS[0], 0.75  # (0.75 and 0.25 are exact in fp32: the EMA reference of the torch path below has no rounding of its own)
    params = _bag(5)
    emas = [torch.nn.Parameter(p.detach().clone() + 0.01) for p in params]
    every = list(range(len(SIZES)))
    early = [i for i in every if i != LATE]
    bucket1 = FlatGradBucket(params, active=lambda p: p is not params[LATE])
    opt1 = FlatAdam(params, lr=LR, betas=betas, eps=EPS, bucket=bucket1, ema_params=emas)
    g = _rng(6)
    late0 = params[LATE].detach().clone()
    for t in (1, 2, 3, 4):
        e0 = emas[LATE].detach().cpu().double()
        _checked_step(opt1, bucket1, params, _grads(g, early), {i: t for i in early}, betas, f"phase1 step{t}", device_step=False,
                      emas=emas, decay=decay)
        pl = params[LATE].detach().cpu().double()
        adam_ref.check(emas[LATE], e0 * decay + (1 - decay) * pl, e0.abs() * decay + (1 - decay) * pl.abs(), f"phase1 step{t} late ema")
    assert torch.equal(params[LATE], late0) and params[LATE].grad is None
    sd1 = opt1.state_dict()
    assert _counts(opt1, params) == {i: 4.0 for i in early}, "`late` never had a gradient: no entry, as in torch"
    snap = [(p.detach().clone(), e.detach().clone()) for p, e in zip(params, emas)]

    def second_phase(scaled):
        with torch.no_grad():
            for (p, e), (p0, e0) in zip(zip(params, emas), snap):
                p.copy_(p0)
                e.copy_(e0)
        bucket2 = FlatGradBucket(params)
        opt2 = FlatAdam(params, lr=LR, betas=betas, eps=EPS, bucket=bucket2, ema_params=emas)
        opt2.load_state_dict(sd1)
        assert _counts(opt2, params) == {i: (0.0 if i == LATE else 4.0) for i in every}
        assert not opt2.state[params[LATE]]["exp_avg"].any() and not opt2.state[params[LATE]]["exp_avg_sq"].any()
        inv = torch.tensor(0.25, device="cuda") if scaled else None
        found = torch.zeros((), device="cuda") if scaled else None
        gg = _rng(7)
        applied = 0
        for launch in range(4 if scaled else 3):
            grads = _grads(gg, every, gain=4.0 if scaled else 1.0)
            what = f"phase2 {'scaled ' if scaled else ''}launch{launch}"
            if scaled and launch == 1:  # an overflowed step: nothing moves, no count advances
                found.fill_(1.0)
                _feed(bucket2, params, grads)
                tensors = lambda: [x for p, e in zip(params, emas)  # noqa: E731
                                   for x in (p, opt2.state[p]["exp_avg"], opt2.state[p]["exp_avg_sq"], e)]
                bits = [x.detach().clone() for x in tensors()]
                opt2.step(ema_decay=decay, inv_grad_scale=inv, found_inf=found)
                torch.cuda.synchronize()
                for a, b in zip(bits, tensors()):
                    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{what}: a found_inf step changed a buffer"
                found.zero_()
                assert _counts(opt2, params) == {i: float(applied + (0 if i == LATE else 4)) for i in every}
                continue
            applied += 1
            counts = {i: applied + (0 if i == LATE else 4) for i in every}
            _checked_step(opt2, bucket2, params, grads, counts, betas, what, device_step=True, emas=emas, decay=decay, inv=inv,
                          found=found, grad_scale=0.25 if scaled else 1.0)
            assert _counts(opt2, params) == {i: float(c) for i, c in counts.items()}
        assert _counts(opt2, params) == {i: (3.0 if i == LATE else 7.0) for i in every}

    second_phase(False)
    second_phase(True)


# ---------------------------------------------------------------------------------------------------------------------------------
# d. the bucket's predicate against autograd
# ---------------------------------------------------------------------------------------------------------------------------------
def _nets(vocab=8, size=16):
    from gif_amd.discriminator import Discriminator
    from gif_amd.generator import StyledGenerator
    with contextlib.redirect_stdout(io.StringIO()):
        kw = dict(embedding_vocab_size=vocab, rendered_flame_ascondition=True, normal_maps_as_cond=True)
        return StyledGenerator(**kw), StyledGenerator(**kw), Discriminator(size=size, num_color_chnls=9)


@pytest.mark.parametrize("step", [2, 3])
def test_g_param_active_is_what_autograd_reaches(step):
    from gif_amd.train_step import FlatGradBucket, _g_param_active
    torch.manual_seed(0)
    G = _nets()[0].cuda()
    res = 4 * 2 ** step
    gen = torch.Generator(device="cuda").manual_seed(1)
    cond = torch.rand(2, 6, res, res, device="cuda", generator=gen) * 2 - 1
    idx = torch.randint(0, 8, (2,), device="cuda", generator=gen)
    img = G(cond, None, step=step, alpha=1, input_indices=idx)[0]
    assert img.shape == (2, 3, res, res)
    img.pow(2).mean().backward()
    active = _g_param_active(G, step)
    named = list(G.named_parameters())
    no_grad = [n for n, p in named if p.grad is None]
    rejected = [n for n, p in named if not active(p)]
    assert no_grad == rejected, (sorted(set(no_grad) - set(rejected)), sorted(set(rejected) - set(no_grad)))
    assert rejected and len(rejected) < len(named)
    bucket = FlatGradBucket(G.parameters(), active=active)  # what Adam never sees is decided from that predicate
    assert [id(p) for p in bucket.params] == [id(p) for _, p in named if active(p)]
    assert [id(p) for p in bucket.inactive] == [id(p) for _, p in named if not active(p)]


# ---------------------------------------------------------------------------------------------------------------------------------
# e. / f. trainer resume
# ---------------------------------------------------------------------------------------------------------------------------------
def _batches(n, res=16, vocab=8):
    gen = torch.Generator(device="cuda").manual_seed(11)
    return [(torch.rand(4, 3, res, res, device="cuda", generator=gen) * 2 - 1, torch.rand(4, 6, res, res, device="cuda", generator=gen) * 2 - 1,
             torch.randint(0, vocab, (4,), device="cuda", generator=gen)) for _ in range(n)]


def _trainer(seed, **kw):
    from gif_amd.train_step import GifTrainer
    torch.manual_seed(seed)
    g, ge, d = _nets()
    ge.load_state_dict(g.state_dict())
    return GifTrainer(g.cuda(), d.cuda(), ge.cuda(), step=2, r1_every=2, gen_reg_type='None', **kw)


def _state(tr, losses):
    tr.flush()
    torch.cuda.synchronize()
    s = {}
    for nm, net in (("G", tr.G), ("D", tr.D), ("G_ema", tr.G_ema)):
        for k, v in net.state_dict().items():
            s[f"{nm}.{k}"] = v.detach().clone()
    for nm, opt in (("g_optim", tr.g_optim), ("d_optim", tr.d_optim)):
        s[f"{nm}.exp_avg"], s[f"{nm}.exp_avg_sq"] = opt._m.clone(), opt._v.clone()
    s["losses"] = torch.tensor(losses, dtype=torch.float64)
    return s


@pytest.mark.parametrize("act", [None, torch.float16], ids=["fp32", "f16"])
def test_trainer_resumed_from_its_checkpoint_equals_the_uninterrupted_run(act, tmp_path):
    """Four iterations (1 and 3 are R1 iterations) in one trainer, against two iterations, save_checkpoint, a fresh trainer on freshly
    drawn networks, load_checkpoint, two iterations.  torch.equal on everything: a difference is state that is neither saved nor rebuilt.
    f16: the checkpoint holds no scaler state, so the comparison needs both runs at the initial scale (no skipped step) — asserted."""
    from gif_amd import checkpoint as C
    kw = {} if act is None else {"act_dtype": act}
    batches = _batches(4)
    scalers = []

    def run(tr, its):
        out = []
        for i in its:
            d_loss, g_loss = tr.step(i, *batches[i])
            out += [d_loss.item(), g_loss.item()]
        scalers.extend(s for s in (tr.g_scaler, tr.d_scaler) if s is not None)
        return out

    tr_a = _trainer(0, **kw)
    a = _state(tr_a, run(tr_a, range(4))[4:])
    tr_b = _trainer(0, **kw)
    run(tr_b, range(2))
    path = str(tmp_path / "ck" / "000002_1.model")
    C.save_checkpoint(tr_b, path, step=2, used_samples=8)
    tr_c = _trainer(5, **kw)
    assert not torch.equal(tr_c.G.generator.const_input.input, tr_b.G.generator.const_input.input)
    assert C.load_checkpoint(tr_c, path) == (2, 8)
    b = _state(tr_c, run(tr_c, range(2, 4)))
    if act is not None:
        assert len(scalers) == 6
        for s in scalers:
            assert s.skipped.item() == 0.0 and s.scale.item() == 2.0 ** 12, "precondition: no skipped step, both runs at the initial scale"
    assert a.keys() == b.keys()
    differ = [k for k in a if not torch.equal(a[k], b[k])]
    assert not differ, f"{len(differ)} of {len(a)} tensors differ after the resume, first: {differ[:8]}; losses {a['losses'].tolist()} vs {b['losses'].tolist()}"
    assert _applied_counts(tr_c) == _applied_counts(tr_a) == (4.0, 4.0)


def _applied_counts(tr):
    out = []
    for opt in (tr.g_optim, tr.d_optim):
        steps = set(float(st["step"]) for st in opt.state_dict()["state"].values())
        assert len(steps) == 1, steps
        out.append(steps.pop())
    return tuple(out)


def test_fused_trainer_checkpoint_continues_with_torch_adam(tmp_path):
    from gif_amd import checkpoint as C
    batches = _batches(3)
    tr = _trainer(0)
    for i in range(2):
        tr.step(i, *batches[i])
    path = str(tmp_path / "ck" / "000002_1.model")
    C.save_checkpoint(tr, path, step=2, used_samples=8)
    tr2 = _trainer(5, fused_adam=False)
    assert type(tr2.g_optim) is torch.optim.Adam and type(tr2.d_optim) is torch.optim.Adam
    C.load_checkpoint(tr2, path)
    d_loss, g_loss = tr2.step(2, *batches[2])
    assert torch.isfinite(d_loss).item() and torch.isfinite(g_loss).item()
    for nm, opt in (("g_optim", tr2.g_optim), ("d_optim", tr2.d_optim)):
        steps = [float(st["step"]) for st in opt.state.values() if st]
        assert steps and all(s == 3.0 for s in steps), f"{nm}: counts after one step on a checkpoint of two: {sorted(set(steps))}"
    assert len([1 for st in tr2.g_optim.state.values() if st]) == len(tr.g_bucket.params)
    path2 = str(tmp_path / "ck" / "000003_1.model")
    C.save_checkpoint(tr2, path2, step=2, used_samples=12)
    ck = torch.load(path2, weights_only=False)
    for key in ("g_optimizer", "d_optimizer_flm"):
        steps = [float(st["step"]) for st in ck[key]["state"].values()]
        assert steps and all(s == 3.0 for s in steps), f"{key} in the next checkpoint: {sorted(set(steps))}"
    for net in (tr2.G, tr2.D, tr2.G_ema):
        for k, v in net.state_dict().items():
            assert torch.isfinite(v).all(), k
