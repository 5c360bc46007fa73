"""A row's first partition step (mxa_topk_grp.hpp grp_topk's first trip): f = 0, l = n, b = 0,
the window the whole allocated row.  The lane model (tools/topk_model.py partition_lanes) at
exactly those arguments against the reference form Row.partition_pivot, the median candidates
at positions 1, n >> 1 and n - 1, and the whole top-k whose first step it is against libstdc++.
(A form of grp_partition specialised on these constants was measured and not kept, DESIGN.md
section 4; these are the properties it relied on.)"""
import numpy as np
import pytest

import exchange_cases as XC
from oracle import mx_oracle as O
from topk_model import LANES, Row, grp_alloc, keys_from_f32, partition_lanes, topk_model, window_for

# around the tail's width 48, the window widths' edges (a multiple of 32, one more) and DeiT's 197
NS = (49, 50, 64, 65, 96, 127, 128, 129, 197, 224, 225, 256)


def first_E(n):
    """The first step's window width: the whole allocated row."""
    return grp_alloc(n) // LANES


@pytest.mark.parametrize("n", NS)
def test_first_width_is_the_allocated_row(n):
    """g.npa / 16 is what the walk up grp_try's chain picks for [0, n): the narrowest window
    that holds the range, at base 0."""
    assert window_for(n, 0, n) == (first_E(n), 0)
    assert LANES * (first_E(n) - 2) < n <= LANES * first_E(n)


@pytest.mark.parametrize("n", NS)
def test_first_step_lane_form(n):
    """Every builder's row: arrays and cut of the lane form at (0, n, E, 0) equal the reference
    form's, the slots used are exactly [0, 2 nsw)."""
    E = first_E(n)
    for name, row in XC.named_rows(n):
        keys = keys_from_f32(row)
        ref = Row(keys)
        cut_ref = ref.partition_pivot(0, n)
        k, i, cut, info = partition_lanes(keys, 0, n, E, 0)
        assert cut == cut_ref, (n, name)
        assert np.array_equal(k, ref.k) and np.array_equal(i, ref.i), (n, name)
        assert sorted(info["slots"]) == list(range(2 * info["nsw"])), (n, name)


@pytest.mark.parametrize("n", NS)
def test_first_step_median_candidates(n):
    """The pivot the step moves to position 0 is the median of positions 1, n >> 1, n - 1 (the
    first of equal candidates in __move_median_to_first's order), and old position 0 goes there."""
    rng = np.random.default_rng(n)
    for nd in (2, 3, 1000):
        keys = keys_from_f32(rng.integers(0, nd, n).astype(np.float32))
        r = Row(keys)
        r.median_to_first(0, n)
        cand = (1, n >> 1, n - 1)
        med = sorted(int(keys[c]) for c in cand)[1]
        assert int(r.k[0]) == med
        m = int(r.i[0])
        assert m in cand and int(r.i[m]) == 0
        assert all(int(r.i[z]) == z for z in range(1, n) if z != m)


@pytest.mark.parametrize("k", [20, 33])
@pytest.mark.parametrize("n", NS)
def test_whole_topk_after_first_step(n, k):
    """The whole top-k in the lane form against libstdc++ (k = 33: the tail's limit)."""
    E = first_E(n)
    keep = {"constant", "descending", "ascending", "two_valued+0", "two_valued+1", f"two_valued+{E - 1}", "spike@1",
            f"spike@{n - 1}", "random0", "random7", "random8", "random15"}
    rows = np.stack([row for name, row in XC.named_rows(n) if name in keep])
    _, want = O.topk(rows, k)
    for r, w in zip(rows, want):
        got, _ = topk_model(r, k, lanes=True)
        assert np.array_equal(got, w), (n, k, r.tolist())
