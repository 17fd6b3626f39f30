"""Pins oracle/stylegan2_ref.py against golden vectors produced by the real reference: model-level forward and gradients
(tests/golden/make_stylegan2_golden.py) and forward parity of models and layers (tests/golden/make_reference_parity_golden.py)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from golden import make_reference_parity_golden as P  # noqa: E402
from oracle import stylegan2_ref as R  # noqa: E402

GOLD = os.path.join(os.path.dirname(__file__), "golden", "stylegan2_golden.pt")
PARITY = os.path.join(os.path.dirname(__file__), "golden", "reference_parity_golden.pt")


def _gold():
    return torch.load(GOLD, weights_only=True)


def _template(shapes, kernels):
    t = {k: torch.zeros(s) for k, s in shapes.items()}
    t.update(kernels)
    return t


def g_state(gold, seed):
    return R.seeded_state_dict(_template(gold["g_template"], gold["g_kernels"]), seed)


def d_state(gold, seed):
    return R.seeded_state_dict(_template(gold["d_template"], gold["d_kernels"]), seed)


def test_generator_matches_reference_golden():
    gold = _gold()
    c = gold["g32"]
    sd = {k: v.requires_grad_(True) if v.is_floating_point() and not k.endswith("kernel") and "embd" not in k else v
          for k, v in g_state(gold, c["seed"]).items()}
    out = R.generator_forward(sd, c["cond"], 3, c["idx"])
    assert torch.equal(out.detach(), c["out"]) or (out.detach() - c["out"]).abs().max() < 1e-5
    loss = (out * torch.linspace(-1, 1, out.numel()).view_as(out)).sum()
    loss.backward()
    pairs = [("generator.const_input.input", c["grad_const"], slice(None)),
             ("generator.progression.2.st_cv1.conv.modulation.bias", c["grad_mod_b_16"], slice(None)),
             ("generator.to_rgb.3.conv.weight", c["grad_rgb_w_32"], slice(None)),
             ("z_to_w.8.bias", c["grad_z_to_w_8_b"], slice(None))]
    for key, ref, sl in pairs:
        got = sd[key].grad[sl]
        assert (got - ref).abs().max() <= 1e-4 * ref.abs().max() + 1e-6, key
    assert (sd["generator.progression.0.st_cv1.conv.weight"].grad[0, :2] - c["grad_w_4x4"]).abs().max() < 1e-4
    assert (sd["generator.progression.3.st_cv2.noise.noise_conv.4.weight"].grad[:8] - c["grad_noise_w_32"]).abs().max() \
        <= 1e-4 * c["grad_noise_w_32"].abs().max()


def test_generator_config1_shape_golden():
    gold = _gold()
    c = gold["g64"]
    with torch.no_grad():
        out = R.generator_forward(g_state(gold, c["seed"]), torch.zeros(4, 6, 64, 64), 4, c["z"])
    assert out.shape == (4, 3, 64, 64)
    assert (out - c["out"]).abs().max() < 1e-5


def test_discriminator_r1_matches_reference_golden():
    gold = _gold()
    c = gold["d32"]
    sd = {k: (v.requires_grad_(True) if not k.endswith("kernel") else v) for k, v in d_state(gold, c["seed"]).items()}
    img = c["img"].clone().requires_grad_(True)
    scores = R.discriminator_forward(sd, img, c["cond"], 32)
    assert (scores.detach() - c["scores"]).abs().max() < 1e-6
    pen = R.grad_penalty_loss([img], scores)
    assert (pen.detach() - c["r1"]).abs().max() <= 1e-5 * c["r1"].abs().max()
    (torch.nn.functional.softplus(-scores).mean() + pen.mean()).backward()
    assert (sd["convs.0.0.weight"].grad - c["grad_first_w"]).abs().max() <= 1e-4 * c["grad_first_w"].abs().max()
    assert (sd["final_linear.1.weight"].grad - c["grad_lin1_w"]).abs().max() <= 1e-4 * c["grad_lin1_w"].abs().max()
    assert (img.grad - c["grad_img"]).abs().max() <= 1e-4 * c["grad_img"].abs().max()
    with torch.no_grad():
        s8 = R.discriminator_forward(d_state(gold, c["seed"]), gold["d32_b8"]["img"], gold["d32_b8"]["cond"], 32)
    assert (s8 - gold["d32_b8"]["scores"]).abs().max() < 1e-6


def test_upfirdn2d_shapes_and_edge_cases():
    k = R.make_kernel([1, 3, 3, 1])
    x = torch.randn(2, 3, 8, 8)
    assert R.upfirdn2d(x, k * 4, up=2, pad=(2, 1)).shape == (2, 3, 16, 16)   # Upsample
    assert R.upfirdn2d(x, k, pad=(2, 2)).shape == (2, 3, 9, 9)               # D blur before stride-2 3x3
    assert R.upfirdn2d(x, k, pad=(1, 1)).shape == (2, 3, 7, 7)               # D blur before stride-2 1x1
    assert R.upfirdn2d(x, k, down=2, pad=(1, 1)).shape == (2, 3, 4, 4)       # Downsample
    assert R.upfirdn2d(x, k, pad=(-1, 2)).shape == (2, 3, 6, 6)              # negative pad = crop
    # DC gain 1 for the normalised kernel in the interior
    ones = torch.ones(1, 1, 8, 8)
    assert torch.allclose(R.upfirdn2d(ones, k, pad=(2, 2))[0, 0, 3:6, 3:6], torch.ones(3, 3), atol=1e-6)


def _parity():
    """Outputs of the real reference modules and the inputs they were computed on (tests/golden/make_reference_parity_golden.py)."""
    gold = torch.load(PARITY, weights_only=True)
    x = P.inputs()
    assert P.checksums(x) == gold["input_checksums"], "regenerated inputs differ from the ones the stored outputs were computed on"
    return gold, x


def test_oracle_equals_imported_reference():
    gold, x = _parity()
    gold = gold["stylegan2"]
    sd = R.seeded_state_dict(P.template_sd(gold["g_template"]), P.G_SEED)
    with torch.no_grad():  # stored outputs of another CPU (other ATen conv kernels): a few ulps of the |out| <= 3.2 image,
        for idx, ref in zip((torch.tensor([1, 19]), x["z"]), gold["g_out"]):  # the bound of test_generator_config1_shape_golden
            assert (R.generator_forward(sd, x["cond"], 4, idx) - ref).abs().max() < 1e-5
    sdd = R.seeded_state_dict(P.template_sd(gold["d_template"]), P.D_SEED)
    with torch.no_grad():
        assert (R.discriminator_forward(sdd, x["img"], x["d_cond"], 64) - gold["d_scores"]).abs().max() < 1e-6
    # layer-level: upfirdn2d incl. negative pads, FusedLeakyReLU
    k = R.make_kernel([1, 3, 3, 1])
    assert torch.equal(k, gold["fir_kernel"])
    for (up, down, pad), ref in zip(P.UPFIRDN_CASES, gold["fir_out"]):
        assert torch.equal(R.upfirdn2d(x["fir_x"], k, up, down, pad), ref)


def test_oracle_layer_variants_equal_imported_reference():
    """Less-travelled layer options: down-sampling modulated conv, no-demod 1x1 (ToRGB), up-sampling modulated conv."""
    gold, x = _parity()
    gold = gold["modulated_conv"]
    for i, (kw, t, ref) in enumerate(zip(P.MODCONV_CASES, gold["templates"], gold["out"])):
        _, demod, up, down = P.modconv_args(kw)
        sd = R.seeded_state_dict(P.template_sd(t), P.MODCONV_SEED + i)
        got = R.modulated_conv2d(x["mc_x"], sd["weight"], sd["modulation.weight"], sd["modulation.bias"], x["mc_style"], demod,
                                 up, sd.get("blur.kernel"), down)
        assert ref.shape == got.shape and (ref - got).abs().max() < 1e-5, kw
