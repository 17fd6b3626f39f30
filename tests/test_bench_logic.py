"""bench.py host logic that needs no GPU: where the R1 iterations of a run fall (timed region / warm-up)."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


def _r1_steps(steps, warmup, r1_every):
    it = bench.r1_start_iteration(steps, warmup, r1_every)
    warm = [k for k in range(warmup) if r1_every and (it + k + 1) % r1_every == 0]
    timed = [k for k in range(steps) if r1_every and (it + warmup + k + 1) % r1_every == 0]
    return warm, timed


@pytest.mark.parametrize("steps,warmup,r1_every", [(20, 5, 16), (16, 2, 16), (32, 5, 16), (40, 5, 16), (20, 5, 4), (12, 3, 16), (20, 0, 16),
                                                   (5, 2, 16), (12, 3, 100000), (1, 0, 16), (16, 2, 0)])
def test_r1_share_of_the_timed_region(steps, warmup, r1_every):
    """The timed steps contain round(steps / r1_every) R1 iterations whatever the warm-up does (the reference runs R1 every 16th step)."""
    warm, timed = _r1_steps(steps, warmup, r1_every)
    assert len(timed) == (int(round(steps / r1_every)) if r1_every else 0)
    assert all(b - a == r1_every for a, b in zip(timed, timed[1:]))


@pytest.mark.parametrize("steps,warmup,r1_every", [(20, 5, 16), (16, 2, 16), (32, 5, 16), (40, 5, 16)])
def test_first_r1_iteration_is_a_warmup_step(steps, warmup, r1_every):
    """The driver's and the default command lines: the last warm-up step is an R1 iteration, so that the timed one is not the first of the
    process (buffer allocation, kernel loading)."""
    warm, timed = _r1_steps(steps, warmup, r1_every)
    assert warm == [warmup - 1] and timed and timed[0] == r1_every - 1


def test_flat_sample_is_fixed_and_complete_below_the_sample_size():
    """--dump-outputs: a small output is written whole, a large one as the same seeded positions in every run."""
    import numpy as np
    import torch
    small = [torch.arange(6.0).view(2, 3), torch.ones(4, dtype=torch.float64)]
    assert np.array_equal(bench.flat_sample(small, k=16), np.r_[np.arange(6.0), np.ones(4)].astype(np.float32))
    big = [torch.randn(300, generator=torch.Generator().manual_seed(1)), torch.randn(50, 7, generator=torch.Generator().manual_seed(2))]
    a, b = bench.flat_sample(big, k=64, seed=3), bench.flat_sample([t.clone() for t in big], k=64, seed=3)
    assert a.dtype == np.float32 and a.shape == (64,) and np.array_equal(a, b)
    whole = torch.cat([t.reshape(-1) for t in big]).numpy()
    assert np.isin(a, whole).all() and len(np.unique(a)) == 64, "distinct elements of the output"
    assert not np.array_equal(a, bench.flat_sample(big, k=64, seed=4))


def test_dump_outputs_writes_float_npy_files_under_the_cap(tmp_path):
    import numpy as np
    arrays = {"loss": np.asarray(0.25, np.float64), "w": np.arange(10, dtype=np.float32)}
    bench.dump_outputs(str(tmp_path / "out"), arrays)
    assert sorted(os.listdir(tmp_path / "out")) == ["loss.npy", "w.npy"]
    assert np.load(tmp_path / "out" / "loss.npy") == 0.25 and np.array_equal(np.load(tmp_path / "out" / "w.npy"), arrays["w"])
    with pytest.raises(TypeError):
        bench.dump_outputs(str(tmp_path / "bad"), {"idx": np.arange(3)})
    with pytest.raises(ValueError):
        bench.dump_outputs(str(tmp_path / "big"), arrays, cap=40)
    assert bench.DUMP_SAMPLE * 4 * 5 + 16 <= bench.DUMP_CAP_BYTES, "five sampled sets + two losses fit the cap"
