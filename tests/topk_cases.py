"""The depth-limit cases of the top-k tests, shared by the GPU tests (test_gpu_parity.py)
and the CPU test that pins which branch each case's rows reach (test_topk_depth_limit_cpu.py).

Branches of the packed selection (mxa_topk_grp.hpp grp_topk with TW > 0, mxa_tail.hpp):
  GROUP -- introselect's depth limit is reached in the group kernel with l > 48: heap_select
           there, then the "sort hand-over" of [0, k) to the one-lane tail (phase 1);
  TAIL  -- the range fits the tail's 48-position prefix first (phase-0 hand-over) and the
           depth limit is then reached inside the tail (its own heap_select);
  NONE  -- the depth limit is never reached with l - f > 3.
"""
import numpy as np

from oracle import mx_oracle as O

GROUP, TAIL, NONE = "group depth limit, l > 48", "phase-0 hand-over, then the tail's depth limit", "none"
TAIL_PREF = 48  # mxa_launch.hpp kTailPref


def case_id(x):
    """pytest id of a case's field: the branch as one word"""
    return {GROUP: "group", TAIL: "tail", NONE: "none"}.get(x, str(x))


def tail_width_for(n, k):
    """mxa_launch.hpp tail_width_for: the prefix the one-lane tail takes over, 0 = none."""
    if k <= 0 or k > 33 or k * 64 <= n:
        return 0
    return TAIL_PREF if k + 2 <= TAIL_PREF and k + (n + 31) // 32 <= TAIL_PREF else 0


# ---- the standalone op: (n, k, the branch of the high-variant row) --------------------
SORT_HANDOVER = [(n, k, GROUP) for n in (100, 128, 197, 256) for k in (2, 5, 9, 13, 17, 20, 21, 25, 29, 32, 33)
                 if k * 64 > n]
TAIL_DEPTH = [(64, 5, TAIL), (64, 17, TAIL), (64, 20, TAIL), (64, 33, TAIL), (48, 5, TAIL), (48, 21, TAIL),
              (48, 29, TAIL), (49, 20, TAIL), (40, 9, TAIL), (40, 21, TAIL), (33, 5, TAIL), (33, 13, TAIL)]
STANDALONE = SORT_HANDOVER + TAIL_DEPTH
DTYPE_CASE = (197, 21, GROUP)  # once more with float16 / bfloat16 inputs


def low_branch(n, k):
    """The branch of the existing (front-peeled) row antiqsort_row(n, k): two elements leave
    the front per step, so the depth 2 lg(n) runs out before f passes k - 1 only for
    k - 1 >= 2 * 2 lg(n); rows of n <= 48 are handed over at once."""
    if k - 1 < 4 * (int(n).bit_length() - 1):
        return NONE
    return TAIL if n <= TAIL_PREF else GROUP


def branch_of(row, k):
    """The branch the probe (libstdc++'s introselect loop) says `row` reaches."""
    p = O.introselect_probe(row, k, TAIL_PREF)
    if not p["depth_limit"]:
        return NONE, p
    return (TAIL if p["hand"] is not None else GROUP), p


def standalone_batch(n, k):
    """More than 64 rows (several tail waves; pending and non-pending rows share a wave): the
    high- and low-variant adversary rows scattered among small-alphabet random rows."""
    rng = np.random.default_rng(1000 * n + k)
    rows = rng.integers(0, 3, (70, n)).astype(np.float32)
    rows[40:] = rng.integers(-6, 7, (30, n)).astype(np.float32) * np.float32(0.25)
    hi, lo = O.antiqsort_row(n, k, high=True), O.antiqsort_row(n, k)
    for r in (0, 31, 63, 64, 69):
        rows[r] = hi
    for r in (1, 65):
        rows[r] = lo
    return rows


# ---- the fused op: the depth-limit row as approximate scores ---------------------------
FUSED = [(T, k, "ex_pred", GROUP) for T in (197, 120) for k in (5, 17, 20, 21, 33)]
FUSED += [(64, 20, "ex_pred", TAIL), (64, 33, "ex_pred", TAIL)]
FUSED += [(197, 21, "MXINT4", GROUP), (197, 21, "true_ex", GROUP)]
ADV_QUERY_ROWS = (0, 5, 31, 32, 63)  # clipped to N; the other query rows of head 0 are random


def fused_inputs(T, k):
    """q, k, v (1, 2, T, 64) and the adversary row's rank vector.  Head 0's key j holds +1 in
    p0[j] positions of MX block 0 and in p1[j] of block 1, -1 elsewhere, p0 = r % 33,
    p1 = r // 33 with r the dense rank of the high-variant row's value at j; an adversarial
    query is +1 in block 0 and +64 in block 1, so its score 2 (p0 + 64 p1) - const rises
    strictly with r.  Head 1 and the other query rows of head 0 are random."""
    row = O.antiqsort_row(T, k, high=True)
    rank = np.argsort(np.argsort(row, kind="stable"), kind="stable")
    assert len(np.unique(row)) == T
    rng = np.random.default_rng(7 * T + k)
    q = rng.standard_normal((1, 2, T, 64), dtype=np.float32)
    kk = rng.standard_normal((1, 2, T, 64), dtype=np.float32)
    v = rng.standard_normal((1, 2, T, 64), dtype=np.float32)
    p0, p1 = rank % 33, rank // 33
    pos = np.arange(32)
    kk[0, 0, :, :32] = np.where(pos[None, :] < p0[:, None], 1.0, -1.0)
    kk[0, 0, :, 32:] = np.where(pos[None, :] < p1[:, None], 1.0, -1.0)
    qrows = [r for r in ADV_QUERY_ROWS if r < T]
    q[0, 0, qrows, :32] = 1.0
    q[0, 0, qrows, 32:] = 64.0
    return q, kk, v, rank, qrows
