"""Reference for the f16x2 row arithmetic (gif_amd/csrc/h2_row.h), written from the description in gif_amd/csrc/common.h ("f16x2 (h2)")
with numpy float32 values; tests/test_h2_row_cpu.py compares the header's host build with it line by line.

A row of the GEMM carries a power-of-two exponent e: its values are multiplied by 2^e before they are split into f16 terms.
  * activations: a running exponent.  It starts at the largest one a float scale can hold (126).  When a 16-element K group brings a
    maximum m with m * 2^e above 65472 (just below the f16 overflow threshold), the row takes the exponent that puts m into
    [2^13, 2^14); the accumulators are multiplied by 2^(change).  Later values may grow 4x before that happens again.
  * weights: one exponent per packed row, the row maximum lands in [2^14, 2^15).
  * window: a row is `wide` when the smallest NON-ZERO group maximum lies more than 14 exponent steps below the row maximum
    (weights: a group more than 16 steps below the row maximum makes the row `narrow`); distances are those of the floats' exponent
    fields, all-zero groups do not count.
Exponents are clamped to [-126, 126]."""
import numpy as np

TARGET, TARGET_W = 13, 14
LIMIT = 65472.0
WINDOW, WINDOW_W = 14, 16


def f32(bits):
    return np.array([bits], dtype=np.uint32).view(np.float32)[0]


def bits_of(x):
    return int(np.array([x], dtype=np.float32).view(np.uint32)[0])


def field(x):
    """exponent field of a float32 value: 2^(field - 127) <= |x| < 2^(field - 126) for a normal x, 0 for zero and denormals"""
    return (bits_of(x) >> 23) & 0xFF


def exp_for(m, target):
    """e with m * 2^e in [2^target, 2^(target + 1)), from m's binade, clamped"""
    return int(max(-126, min(126, target - (field(m) - 127))))


def pow2(e):
    return np.float32(np.ldexp(np.float32(1.0), e))


def limit_for(e):
    with np.errstate(over="ignore"):
        return np.float32(np.ldexp(np.float64(LIMIT), -e))  # (beyond the float range: infinity, no value outgrows it)


class Row:
    def __init__(self):
        self.ex, self.dl = 126, 0
        self.max = np.float32(0.0)
        self.smallest = None  # smallest non-zero group maximum

    def observe(self, groups):
        """one decision over the maxima of one or more groups; True when the exponent changed"""
        for m in groups:
            self.max = max(self.max, m)
            if m > 0 and (self.smallest is None or m < self.smallest):
                self.smallest = m
        m = max(groups)
        self.dl = 0
        if m > limit_for(self.ex):
            new = exp_for(m, TARGET)
            self.dl, self.ex = new - self.ex, new
            return True
        return False

    def wide(self):
        return self.smallest is not None and field(self.max) - field(self.smallest) > WINDOW

    def text(self):
        gmin = 0xFFFFFFFF if self.smallest is None else bits_of(self.smallest) - 1  # (how the kernels keep it: bits - 1, "none" is the largest)
        return "ex=%d dl=%d sc=%08x lim=%08x max=%08x gmin=%08x wide=%d" % (
            self.ex, self.dl, bits_of(pow2(self.ex)), bits_of(limit_for(self.ex)), bits_of(self.max), gmin, int(self.wide()))


def weight_exp(rowmax):
    return exp_for(rowmax, TARGET_W)


def weight_narrow(rowmax, gm):
    return bool(gm > 0 and field(rowmax) - field(gm) > WINDOW_W)
