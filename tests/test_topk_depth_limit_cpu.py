"""CPU: which branch of the packed selection each depth-limit GPU case reaches.

The GPU tests of test_gpu_parity.py (test_topk_depth_limit_handovers*, test_fused_depth_limit_
handover) only test what they are named for if their rows exhaust introselect's depth limit
where intended.  oracle/topk_ref.cpp's probe restates libstdc++'s introselect loop (same
partition, same 2 lg(n) depth) and reports where the depth limit is reached and where the
range first fits the tail's 48-position prefix; these tests assert, as a condition, the branch
of every (n, k, variant) the GPU tests use (tests/topk_cases.py), that the packed path with
the one-lane tail takes the case at all (tail_width_for, every value's low mantissa byte
zero) and, for the fused op, that the oracle's approximate scores order the keys as the
adversary row does."""
import numpy as np
import pytest

import topk_cases as C
from oracle import mx_oracle as O


def _packs(row):
    return not (np.ascontiguousarray(row, np.float32).view(np.uint32) & 0xFF).any()


def test_default_adversary_row_unchanged_and_variants_differ():
    for n, k in ((197, 30), (120, 20), (64, 5)):
        lo, hi = O.antiqsort_row(n, k), O.antiqsort_row(n, k, high=True)
        assert np.array_equal(lo, O.antiqsort_row(n, k, high=False))
        assert (lo <= 0).all() and (hi >= 0).all() and len(np.unique(hi)) == n


@pytest.mark.parametrize("n,k,want", C.STANDALONE, ids=C.case_id)  # (DTYPE_CASE is one of them)
def test_standalone_case_branches(n, k, want):
    assert C.DTYPE_CASE in C.STANDALONE
    assert C.tail_width_for(n, k) == C.TAIL_PREF, "the one-lane tail does not take this case"
    hi, lo = O.antiqsort_row(n, k, high=True), O.antiqsort_row(n, k)
    got_hi, p_hi = C.branch_of(hi, k)
    got_lo, p_lo = C.branch_of(lo, k)
    print(f"n={n} k={k}: high -> {got_hi} {p_hi}; low -> {got_lo} {p_lo}")
    assert got_hi == want, p_hi
    assert got_lo == C.low_branch(n, k), p_lo
    if want == C.GROUP:
        assert p_hi["f"] == 0 and p_hi["l"] > C.TAIL_PREF and p_hi["hand"] is None
    else:
        assert p_hi["f"] == 0 and k <= p_hi["l"] <= C.TAIL_PREF and p_hi["hand"][0] <= C.TAIL_PREF
    batch = C.standalone_batch(n, k)
    assert batch.shape[0] > 64 and _packs(batch)
    assert np.array_equal(batch[0], hi) and np.array_equal(batch[1], lo)
    if n == C.DTYPE_CASE[0] and k == C.DTYPE_CASE[1]:  # the row's integers are exact in both 16-bit types
        import torch
        t = torch.from_numpy(batch)
        for dt in (torch.float16, torch.bfloat16):
            assert torch.equal(t.to(dt).to(torch.float32), t)


def test_probe_table():
    """The high-variant row reaches the depth limit for every small k (the table the GPU
    cases were chosen from), the existing low-variant row only for large k."""
    for n, l in ((100, 77), (120, 97), (128, 101), (197, 170), (256, 225)):
        for k in range(2, 34):
            if k * 64 <= n:
                continue
            b, p = C.branch_of(O.antiqsort_row(n, k, high=True), k)
            assert (b, p["f"], p["l"]) == (C.GROUP, 0, l), (n, k, p)
            assert C.branch_of(O.antiqsort_row(n, k), k)[0] == C.low_branch(n, k), (n, k)
    for n, l, hand, kmax in ((64, 41, (47, 3), 33), (48, 29, (48, 10), 29), (49, 30, (48, 9), 30), (40, 21, (40, 10), 21),
                             (33, 14, (33, 10), 14)):
        for k in range(2, 34):
            b, p = C.branch_of(O.antiqsort_row(n, k, high=True), k)
            if k <= kmax:
                assert (b, p["f"], p["l"], p["hand"]) == (C.TAIL, 0, l, hand), (n, k, p)
            else:
                assert b == C.NONE, (n, k, p)


def test_existing_depth_limit_pairs():
    """test_topk_depth_limit_fallbacks_and_partial_sort's pairs: which reach the depth limit
    (k * 64 <= n is partial_sort, no introselect at all)."""
    got = {(n, k): O.introselect_probe(O.antiqsort_row(n, k), k, 0)["depth_limit"]
           for n, k in [(197, 30), (197, 154), (256, 77), (256, 154), (512, 300), (120, 20)]}
    assert got == {(197, 30): True, (197, 154): True, (256, 77): True, (256, 154): True, (512, 300): True,
                   (120, 20): False}
    assert 4 * 64 <= 300


@pytest.mark.parametrize("T,k,mode,want", C.FUSED, ids=C.case_id)
def test_fused_case_scores_and_branches(T, k, mode, want):
    assert C.tail_width_for(T, k) == C.TAIL_PREF
    q, kk, v, rank, qrows = C.fused_inputs(T, k)
    aq, ak = O.approx_operands(q[0, 0], kk[0, 0], mode)
    pred = O.exact_matmul_f32(aq, np.swapaxes(ak, -1, -2))
    assert len(qrows) >= 3
    for r in qrows:
        row = pred[r]
        assert len(np.unique(row)) == T
        assert np.array_equal(np.argsort(np.argsort(row, kind="stable"), kind="stable"), rank)
        assert _packs(row), "the scores need their low mantissa byte: the row would leave the packed pass"
        got, p = C.branch_of(row, k)
        assert got == want, p
    print(f"T={T} k={k} {mode}: {want}")
