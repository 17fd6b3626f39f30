"""torch's single-tensor Adam restated in fp64 over the operands of gif_adam_ema_step_f32, and the per-element bounds the fused
kernel is held to.  Shared by test_gpu_linear_reduce_routes.test_flat_adam (chunk and alignment edges, where the tolerance was
measured: worst |got - ref| / R 1.5e-7, TOL 1e-6) and test_gpu_resume (per-parameter step counts)."""
import math

import numpy as np
import torch

TOL_ADAM = 1e-6
TINY = 1e-30


def f32(v):
    return float(np.float32(v))


def adam_ref(p, g, m, v, t, lr, b1, b2, eps, device_step):
    """torch's single-tensor Adam in fp64 over the kernel's operands: lr, betas and eps arrive as fp32; the bias corrections are
    formed in double from the Python betas (host) or from the fp32 betas (device step count: a loss-scaled step, or an optimiser
    whose parameters carry unequal counts)."""
    lrf, b1f, b2f, epsf = f32(lr), f32(b1), f32(b2), f32(eps)
    m2 = b1f * m + (1 - b1f) * g
    v2 = b2f * v + (1 - b2f) * g * g
    c1, c2 = (b1f, b2f) if device_step else (b1, b2)
    bc1, bc2 = 1 - c1 ** t, 1 - c2 ** t
    denom = v2.sqrt() / math.sqrt(bc2) + epsf
    upd = lrf / bc1 * m2 / denom
    return p - upd, m2, v2, upd


def adam_bounds(p0, g, m0, vr, upd):
    """R of |got - ref| <= TOL_ADAM * R for exp_avg, exp_avg_sq and the parameter (fp64 CPU tensors of one step's operands)."""
    return m0.abs() + g.abs(), vr.abs(), p0.abs() + 4 * upd.abs()


def check(got, ref, R, what, tol=TOL_ADAM):
    """|got - ref| <= tol * R + TINY element-wise; got: any tensor (moved to CPU fp64); ref, R: fp64 CPU.  Returns the worst ratio."""
    got = got.detach().double().cpu()
    assert got.shape == ref.shape == R.shape, (what, got.shape, ref.shape, R.shape)
    assert torch.isfinite(got).all(), f"{what}: {int((~torch.isfinite(got)).sum())} non-finite elements"
    err = (got - ref).abs()
    ratio = (err / (R + TINY)).max().item() if err.numel() else 0.0
    print(f"\n[adam ratio] {what}: {ratio:.3e}")
    bad = err > tol * R + TINY
    if bad.any():
        i = tuple(int(v) for v in bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements out of bound; first at {i}: got {got[i].item():.9e} "
                             f"ref {ref[i].item():.9e} R {R[i].item():.3e}; worst ratio {ratio:.3e} > {tol:.1e}")
    return ratio
