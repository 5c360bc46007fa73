"""The lane form of the partition step (tools/topk_model.py partition_lanes: one slot index
space, one combined mask per lane -- what mxa_topk_grp.hpp grp_partition computes) against
the reference form Row.partition_pivot, and the whole top-k on it against libstdc++."""
import numpy as np
import pytest

import exchange_cases as XC
from oracle import mx_oracle as O
from topk_model import LANES, Row, keys_from_f32, partition_lanes, topk_model

WIDTHS = (2, 4, 6, 8, 10, 12, 14, 16, 24, 32)


def check_step(keys, f, l, E, b):
    """One step in both forms: arrays and cut equal, used slots exactly [0, 2 nsw)."""
    ref = Row(keys)
    cut_ref = ref.partition_pivot(f, l)
    k, i, cut, info = partition_lanes(keys, f, l, E, b)
    assert cut == cut_ref, (f, l, E, b)
    assert np.array_equal(k, ref.k) and np.array_equal(i, ref.i), (f, l, E, b)
    assert sorted(info["slots"]) == list(range(2 * info["nsw"])), (f, l, E, b)
    return cut, info


@pytest.mark.parametrize("E", WIDTHS)
def test_lane_form_equals_reference_form(E):
    """Whole rows (with and without window padding) and random sub-ranges at random even
    bases, every builder's row, every window width."""
    rng = np.random.default_rng(E)
    for n in (LANES * E, LANES * E - 3):
        for name, row in XC.named_rows(n):
            keys = keys_from_f32(row)
            check_step(keys, 0, n, E, 0)
            for _ in range(3):
                f = int(rng.integers(0, n - 4))
                l = int(rng.integers(f + 4, n + 1))
                b = int(rng.integers(0, f // 2 + 1)) * 2  # even, b <= f; l <= n <= b + 16 E
                check_step(keys, f, l, E, b)


@pytest.mark.parametrize("nd", [1, 2, 3, 5, 9, 1000])
def test_lane_form_random_alphabets(nd):
    rng = np.random.default_rng(nd)
    for E in WIDTHS:
        n = int(rng.integers(max(8, LANES * E // 2), LANES * E + 1))
        keys = keys_from_f32(rng.integers(0, nd, n).astype(np.float32))
        for _ in range(6):
            f = int(rng.integers(0, n - 4))
            l = int(rng.integers(f + 4, n + 1))
            b = int(rng.integers(0, f // 2 + 1)) * 2
            check_step(keys, f, l, E, b)


def test_pins_cut_offsets_and_largest_swap_count():
    """What the builders are for, at n = 224 (first window E = 14, base 0).  The shifted
    two-valued rows put the first step's cut at every in-lane offset 0 .. 13 (offset 0: a
    lane boundary); the constant row swaps (l - f - 1) // 2 pairs (at least the (n - 2) // 2
    asked of it; one more for odd n), the descending row none, with X = 0 in every lane."""
    n = 224
    assert XC.first_width(n) == 14
    offs = set()
    for s in range(14):
        cut, info = check_step(keys_from_f32(XC.two_valued(n, s)), 0, n, 14, 0)
        offs.add(cut % 14)
        assert info["nsw"] > 0
    assert offs == set(range(14))
    for m in (n, 197):
        _, info = check_step(keys_from_f32(XC.constant(m)), 0, m, 14, 0)
        assert info["nsw"] == (m - 1) // 2 >= (m - 2) // 2
    _, info = check_step(keys_from_f32(XC.descending(n)), 0, n, 14, 0)
    assert info["nsw"] == 0 and not any(info["X"])


@pytest.mark.parametrize("n,k", XC.NK)
def test_whole_topk_on_lane_form(n, k):
    """Every step of the whole top-k in the lane form, in the windows the kernel picks,
    against libstdc++: one row of each builder (the two-valued row at three shifts)."""
    E = XC.first_width(n)
    keep = {"constant", "descending", "ascending", "two_valued+0", "two_valued+1", f"two_valued+{E - 1}", "spike@1",
            f"spike@{n - 1}", "random0", "random7", "random8", "random15"}
    rows = np.stack([row for name, row in XC.named_rows(n) if name in keep])
    _, want = O.topk(rows, k)
    for r, w in zip(rows, want):
        got, _ = topk_model(r, k, lanes=True)
        assert np.array_equal(got, w), (n, k, r.tolist())
