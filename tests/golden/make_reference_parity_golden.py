"""Generates tests/golden/reference_parity_golden.pt: outputs of the REAL reference modules (imported in place through
oracle/reference_import.py, where the reference is present) for the oracle-vs-reference parity tests
tests/test_oracle_{stylegan2,resize,texture_loss}.py::test_oracle_*_imported_reference*, which then run anywhere.

    python tests/golden/make_reference_parity_golden.py

Only outputs are stored.  Inputs come from inputs() and weights from oracle.stylegan2_ref.seeded_state_dict over the recorded
key->shape templates, both seeded; the tests regenerate them and check the stored input checksums first.
"""
import contextlib
import io
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import reference_import as ri  # noqa: E402
from oracle import stylegan2_ref as R  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_parity_golden.pt")
UPFIRDN_CASES = ((1, 1, (2, 2)), (2, 1, (2, 1)), (1, 2, (1, 1)), (1, 1, (-1, 2)), (2, 2, (3, 0)))
MODCONV_CASES = (dict(downsample=True), dict(upsample=True), dict(), dict(demodulate=False))  # the last one: 16 -> 3, 1x1 (ToRGB)
G_SEED, D_SEED, MODCONV_SEED = 5, 6, 20


def inputs():
    """Every input of the parity cases, uniform in [-1, 1) from one seeded generator."""
    g = torch.Generator().manual_seed(2024)
    shapes = {"cond": (2, 6, 64, 64), "z": (2, 512), "img": (4, 3, 64, 64), "d_cond": (4, 6, 64, 64), "fir_x": (2, 5, 9, 9),
              "mc_x": (2, 16, 8, 8), "mc_style": (2, 512), "resize_x": (2, 3, 13, 10), "r1_x": (3, 3, 8, 8), "r1_w": (3, 8, 8)}
    return {k: torch.rand(s, generator=g) * 2 - 1 for k, s in shapes.items()}


def checksums(x):
    return {k: v.double().sum().item() for k, v in x.items()}


def template(sd):
    return {"shapes": {k: tuple(v.shape) for k, v in sd.items()},
            "kernels": {k: v.clone() for k, v in sd.items() if k.endswith(".kernel")}}


def template_sd(t):
    """A state_dict of the recorded shapes (zeros) with the recorded FIR kernels: the input of seeded_state_dict."""
    sd = {k: torch.zeros(s) for k, s in t["shapes"].items()}
    sd.update(t["kernels"])
    return sd


def modconv_args(kw):
    """(constructor arguments, demodulate, upsample, downsample) of a MODCONV_CASES entry."""
    demod = kw.get("demodulate", True)
    ctor = (16, 24, 3, 512) if demod else (16, 3, 1, 512)
    return ctor, demod, kw.get("upsample", False), kw.get("downsample", False)


def stylegan2(x):
    """test_oracle_stylegan2.py::test_oracle_equals_imported_reference"""
    SG, D, L = ri.reference_modules()
    with contextlib.redirect_stdout(io.StringIO()):
        g = SG(embedding_vocab_size=20, rendered_flame_ascondition=True, normal_maps_as_cond=True)
        d = D(size=64, num_color_chnls=9)
    out = {"g_template": template(g.state_dict()), "d_template": template(d.state_dict())}
    g.load_state_dict(R.seeded_state_dict(g.state_dict(), G_SEED), strict=True)
    d.load_state_dict(R.seeded_state_dict(d.state_dict(), D_SEED), strict=True)
    k = L.make_kernel([1, 3, 3, 1])
    with torch.no_grad():
        out["g_out"] = [g(x["cond"], None, step=4, alpha=1, input_indices=idx)[0] for idx in (torch.tensor([1, 19]), x["z"])]
        out["d_scores"] = d(x["img"], condition=x["d_cond"])[0]
    out["fir_kernel"] = k
    out["fir_out"] = [L.upfirdn2d(x["fir_x"], k, up, down, pad) for up, down, pad in UPFIRDN_CASES]
    return out


def modulated_conv(x):
    """test_oracle_stylegan2.py::test_oracle_layer_variants_equal_imported_reference"""
    _, _, L = ri.reference_modules()
    templates, outs = [], []
    with torch.no_grad():
        for i, kw in enumerate(MODCONV_CASES):
            ctor, demod, up, down = modconv_args(kw)
            m = L.ModulatedConv2d(*ctor, demodulate=demod, upsample=up, downsample=down)
            templates.append(template(m.state_dict()))
            m.load_state_dict(R.seeded_state_dict(m.state_dict(), MODCONV_SEED + i), strict=True)
            outs.append(m(x["mc_x"], x["mc_style"]))
    return {"templates": templates, "out": outs}


def resize(x):
    """test_oracle_resize.py::test_oracle_equals_imported_reference"""
    f = ri.reference_fast_image_reshape()
    return {f"{mode}_{clamp}": f(x["resize_x"], 21, 6, non_diff_allowed=clamp, mode=mode)
            for mode in ("bicubic", "bilinear") for clamp in (False, True)}


def losses(x):
    """test_oracle_texture_loss.py::test_oracle_equals_imported_reference_losses (textures / face mask: texture_loss_golden.npz)"""
    import numpy as np
    L = ri.reference_losses()
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "texture_loss_golden.npz"))
    tex = torch.from_numpy(g["textures"])
    me = types.SimpleNamespace(face_region_only_mask=torch.from_numpy(g["face_big"]))
    r1_x = x["r1_x"].clone().requires_grad_(True)
    out = (r1_x * x["r1_w"]).sum((1, 2, 3)).pow(2)[:, None]
    return {"pair23_big": L.InterpolatedTextureLoss.pairwise_texture_loss(me, tex[2], tex[3]),
            "r1": L.grad_penalty_loss([r1_x], out, step=None).detach()}


def main():
    x = inputs()
    gold = {"input_checksums": checksums(x), "stylegan2": stylegan2(x), "modulated_conv": modulated_conv(x), "resize": resize(x),
            "losses": losses(x)}
    torch.save(gold, OUT)
    print("wrote", OUT, os.path.getsize(OUT) // 1024, "KiB")


if __name__ == "__main__":
    main()
