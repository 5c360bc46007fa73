"""Rows for the partition step's exchange (mxa_topk_grp.hpp grp_partition; the lane form
tools/topk_model.py partition_lanes), shared by test_exchange_model_cpu.py and
test_gpu_exchange.py.  Every row holds small integers, so it also fits the packed elements.

With torch's comparator (greater) the larger values go to the front: a left stop is a key
<= the pivot, a right stop a key >= the pivot, and equal keys are both.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(ROOT, "tools") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "tools"))

from topk_model import window_for  # noqa: E402

F32 = np.float32


def constant(n):
    """Every position is both kinds of stop: nsw = (l - f - 1) // 2 on every step, the
    largest there is."""
    return np.full(n, 3, F32)


def descending(n):
    """Strictly descending values, the comparator's order: nothing ever swaps."""
    return np.arange(n, 0, -1).astype(F32)


def ascending(n):
    return np.arange(1, n + 1).astype(F32)


def two_valued(n, shift=0):
    """The low half first, then the high half, rotated right by `shift` positions (each
    shift moves the first step's cut by one position)."""
    row = np.ones(n, F32)
    row[:n // 2] = 0
    return np.roll(row, shift)


def spike(n, pos):
    """One large value at `pos` among equal values."""
    row = np.full(n, 2, F32)
    row[pos] = 9
    return row


def random_rows(n, count=16):
    """Half of them over 2 values, half over 3."""
    rng = np.random.default_rng(97 * n + count)
    rows = rng.integers(0, 2, (count, n))
    rows[count // 2:] = rng.integers(0, 3, (count - count // 2, n))
    return rows.astype(F32)


def first_width(n):
    """The window width E of the first step of an n-key row (n <= 512)."""
    return window_for(n, 0, n)[0]


def named_rows(n):
    """[(name, row)] of every builder at length n; the two-valued row at every shift below
    the first step's window width."""
    out = [("constant", constant(n)), ("descending", descending(n)), ("ascending", ascending(n))]
    out += [(f"two_valued+{s}", two_valued(n, s)) for s in range(first_width(n))]
    out += [("spike@1", spike(n, 1)), (f"spike@{n - 1}", spike(n, n - 1))]
    out += [(f"random{r}", row) for r, row in enumerate(random_rows(n))]
    return out


def batch(n):
    return np.stack([row for _, row in named_rows(n)])


# the standalone op's cases: n = 33 .. 256 gives windows E = 4 .. 16 with and without
# padding and both NP of the packed form; k = 20 the tail hand-over, 40 the whole-prefix
# rank, 0.6 n the queued segments (n >= 128); n = 300, 512 the 64-bit elements with
# 16-bit slots
NS = (33, 64, 96, 128, 160, 197, 224, 256)
NK = [(n, k) for n in NS for k in sorted({min(20, n - 1), *((40,) if n >= 64 else ()), -(-6 * n // 10)})]
NK += [(n, k) for n in (300, 512) for k in (20, 180)]
# (B, H, N, T, D, k) of the fused calls
FUSED = [(1, 2, 224, 224, 64, 20), (1, 2, 256, 256, 72, 154)]
