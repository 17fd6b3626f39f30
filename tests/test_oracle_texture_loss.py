"""CPU: the texture-interpolation loss oracle against values produced by the real reference methods."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import texture_loss_ref as R  # noqa: E402


def gold():
    return np.load(os.path.join(os.path.dirname(__file__), "golden", "texture_loss_golden.npz"))


@pytest.mark.parametrize("tag", ["same", "big"])
def test_oracle_reproduces_reference_values(tag):
    g = gold()
    tex, msk = torch.from_numpy(g["textures"]), torch.from_numpy(g["tx_masks"])
    face = torch.from_numpy(g[f"face_{tag}"])
    assert R.pairwise_texture_loss(face, tex[0], tex[1]).item() == pytest.approx(float(g[f"pair01_{tag}"]), rel=1e-6)
    loop = R.texture_pairs_loss(face, tex, msk, g[f"loop_pairs_{tag}"])
    assert loop.item() == pytest.approx(float(g[f"loop_{tag}"]), rel=1e-6)
    assert len(R.all_pairs(6)) == 10


def test_oracle_equals_imported_reference_losses():
    """R1 and the pairwise texture loss of the oracle vs values of the REAL loss_functions.losses
    (tests/golden/make_reference_parity_golden.py)."""
    from golden import make_reference_parity_golden as P
    from oracle import stylegan2_ref as S
    gold_all = torch.load(os.path.join(os.path.dirname(__file__), "golden", "reference_parity_golden.pt"), weights_only=True)
    ref = gold_all["losses"]
    xs = P.inputs()
    assert P.checksums(xs) == gold_all["input_checksums"]
    g = gold()
    tex = torch.from_numpy(g["textures"])
    assert torch.equal(ref["pair23_big"], R.pairwise_texture_loss(torch.from_numpy(g["face_big"]), tex[2], tex[3]))
    x = xs["r1_x"].clone().requires_grad_(True)
    out = (x * xs["r1_w"]).sum((1, 2, 3)).pow(2)[:, None]
    got = S.grad_penalty_loss([x], out)
    assert torch.allclose(ref["r1"], got, rtol=1e-6, atol=0)
