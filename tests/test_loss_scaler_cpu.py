"""train_step.DeviceLossScaler's policy on the CPU (no library needed: the flag-word calls are device-only), step by step against a
restatement of its docstring:

    an overflow halves the scale and resets the clean count; `growth_interval` consecutive clean steps double it; the result is clamped
    to [1, max_scale]; inv_scale is the reciprocal of the scale the gradients were produced with; skipped counts the overflows.

Every scale here is a power of two, so scale, 1 / scale and the counters are exact in fp32 and the comparison is equality.  An overflow
reaches update() through one of these channels: +inf, -inf or NaN in the bucket (first element, a middle one, the last gradient, the
last element of the buffer), or the scaler's saturation snapshot `sat` beside a finite bucket — parked in the bucket's flag slot by
end_backward(bucket), or read by update() directly when no bucket was given."""
import itertools
import math

import pytest
import torch

from gif_amd.train_step import DeviceLossScaler, FlatGradBucket

CPU = torch.device("cpu")
MAX_SCALE = 2.0 ** 20  # DeviceLossScaler's default


class Policy:
    """The docstring, restated."""

    def __init__(self, init_scale, growth_interval, max_scale=MAX_SCALE):
        self.scale, self.interval, self.max_scale = float(init_scale), growth_interval, float(max_scale)
        self.clean = self.skipped = 0
        self.inv_scale = 1.0 / self.scale

    def update(self, overflow):
        self.inv_scale = 1.0 / self.scale  # the scale this step's gradients carry
        if overflow:
            self.skipped, self.clean, new = self.skipped + 1, 0, self.scale / 2
        else:
            self.clean, new = self.clean + 1, self.scale
            if self.clean >= self.interval:
                self.clean, new = 0, self.scale * 2
        self.scale = min(max(new, 1.0), self.max_scale)
        return 1.0 if overflow else 0.0


def _bucket():
    params = [torch.nn.Parameter(torch.zeros(5)), torch.nn.Parameter(torch.zeros(3, 7)), torch.nn.Parameter(torch.zeros(70))]
    b = FlatGradBucket(params)
    last_grad = b.offsets[-1] + params[-1].numel() - 1
    assert b.flag_offset > last_grad and b.flat.numel() == b.flag_offset + b.ALIGN
    return b, {"first": 0, "middle": b.offsets[1] + 10, "last_grad": last_grad, "last": b.flat.numel() - 1}


CHANNELS = [(v, where) for v in (math.inf, -math.inf, math.nan) for where in ("first", "middle", "last_grad", "last")] + \
           [("sat", "slot"), ("sat", "direct")]


def _one_step(sc, bucket, spots, channel):
    """One optimiser step as GifTrainer runs it; channel None: a clean step."""
    bucket.zero()
    sc.begin_step()
    bucket.flat[:bucket.flag_offset].fill_(0.25)  # the backward pass: finite gradients
    with_bucket = True
    if channel is not None:
        v, where = channel
        if v == "sat":
            sc.sat.fill_(1.0)  # what gif_f16_overflow_or_into leaves behind when a store saturated
            with_bucket = where == "slot"
        else:
            bucket.flat[spots[where]] = v
    sc.end_backward(bucket if with_bucket else None)
    if channel is not None and channel[0] == "sat" and not with_bucket:
        assert torch.isfinite(bucket.flat).all()  # the flag alone carries this overflow
    sc.update(bucket.flat)


@pytest.mark.parametrize("growth_interval", [1, 2, 3, 5])
@pytest.mark.parametrize("init_scale", [1.0, 2.0, 2.0 ** 12, 2.0 ** 19, 2.0 ** 20])
def test_scaler_follows_its_policy_step_by_step(init_scale, growth_interval):
    g = torch.Generator().manual_seed(int(init_scale) * 7 + growth_interval)
    sc = DeviceLossScaler(CPU, init_scale=init_scale, growth_interval=growth_interval)
    ref = Policy(init_scale, growth_interval)
    assert sc.scale.item() == ref.scale and sc.inv_scale.item() == ref.inv_scale and sc.skipped.item() == 0
    bucket, spots = _bucket()
    channels = itertools.cycle(CHANNELS)
    # three regimes of the overflow rate: growth dominates (the clamp at max_scale), a mix, overflow dominates (the clamp at 1)
    seen = set()
    for rate, steps in ((0.02, 160), (0.5, 40), (0.9, 60)):
        for _ in range(steps):
            channel = next(channels) if torch.rand((), generator=g).item() < rate else None
            _one_step(sc, bucket, spots, channel)
            want = ref.update(channel is not None)
            got = (sc.found_inf.item(), sc.scale.item(), sc.inv_scale.item(), sc.skipped.item())
            assert got == (want, ref.scale, ref.inv_scale, float(ref.skipped)), (channel, got, vars(ref))
            seen.add(ref.scale)
    assert ref.skipped >= len(CHANNELS), "every channel signalled an overflow at least once"
    assert 1.0 in seen, "the run never sat on the lower clamp"
    assert MAX_SCALE in seen, "the run never sat on the upper clamp"


def test_a_run_of_clean_steps_shorter_than_the_interval_does_not_grow():
    sc = DeviceLossScaler(CPU, init_scale=64.0, growth_interval=3)
    bucket, spots = _bucket()
    scales = []
    for channel in (None, None, (math.inf, "first"), None, None, (math.nan, "last"), None, None, None, None):
        _one_step(sc, bucket, spots, channel)
        scales.append(sc.scale.item())
    # two clean steps, an overflow (the count starts again), two clean, an overflow, three clean: the only growth
    assert scales == [64.0, 64.0, 32.0, 32.0, 32.0, 16.0, 16.0, 16.0, 32.0, 32.0]
    assert sc.skipped.item() == 2.0


def test_max_scale_argument_and_an_init_scale_above_it():
    sc = DeviceLossScaler(CPU, init_scale=2.0 ** 30, growth_interval=1, max_scale=2.0 ** 8)
    bucket, spots = _bucket()
    _one_step(sc, bucket, spots, (math.inf, "middle"))
    assert sc.inv_scale.item() == 2.0 ** -30 and sc.scale.item() == 2.0 ** 8  # clamp(2^29, 1, 2^8)
    _one_step(sc, bucket, spots, None)
    assert sc.inv_scale.item() == 2.0 ** -8 and sc.scale.item() == 2.0 ** 8   # doubled, clamped again


def test_end_backward_writes_the_flag_slot_and_nothing_else():
    sc = DeviceLossScaler(CPU)
    bucket, _ = _bucket()
    pattern = torch.arange(1, bucket.flat.numel() + 1, dtype=torch.float32)
    for sat, want in ((1.0, math.inf), (0.0, 0.0), (3.0, math.inf)):
        bucket.flat.copy_(pattern)
        sc.begin_step()
        sc.sat.fill_(sat)
        sc.end_backward(bucket)
        assert bucket.flat[bucket.flag_offset].item() == want and bucket.flag_slot.item() == want
        keep = torch.ones(bucket.flat.numel(), dtype=torch.bool)
        keep[bucket.flag_offset] = False
        assert torch.equal(bucket.flat[keep], pattern[keep])
    sc.end_backward(None)  # no bucket: nothing to write
    assert bucket.flag_slot.item() == math.inf


def test_bucket_zero_clears_the_flag_slot():
    sc = DeviceLossScaler(CPU)
    bucket, _ = _bucket()
    sc.sat.fill_(1.0)
    sc.end_backward(bucket)
    assert bucket.flag_slot.item() == math.inf
    bucket.zero()
    assert bucket.flag_slot.item() == 0.0 and not bucket.flat.any()
    assert all(p.grad is None for p in bucket.params)


def test_a_second_update_does_not_see_the_previous_steps_snapshot():
    sc = DeviceLossScaler(CPU, init_scale=16.0, growth_interval=100)
    bucket, _ = _bucket()
    bucket.zero()
    sc.begin_step()
    sc.sat.fill_(1.0)
    sc.end_backward(bucket)
    sc.update(bucket.flat)
    assert (sc.found_inf.item(), sc.scale.item(), sc.skipped.item()) == (1.0, 8.0, 1.0)
    # the next step: begin_step() drops the snapshot, zero() the slot; update() without an end_backward() of its own finds nothing
    bucket.zero()
    sc.begin_step()
    assert sc.sat.item() == 0.0
    sc.update(bucket.flat)
    assert (sc.found_inf.item(), sc.scale.item(), sc.inv_scale.item(), sc.skipped.item()) == (0.0, 8.0, 1.0 / 8.0, 1.0)
