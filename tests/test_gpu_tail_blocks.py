"""The one-lane top-k tail's block stores (mxa_tail.hpp): a wave whose 64 rows are all the
tail's writes its index and prune-mask runs in 16-byte chunks; every other wave (a partial last
wave, a row finished in the selection kernel or left for the 64-bit pass, an output that is
only 8-byte aligned, the standalone values output) keeps one lane per row.  Every comparison is
bit-exact: idx and mask words against the oracle's libstdc++ top-k of the oracle's approximate
scores, as test_gpu_parity.py compares them; the call without an idx output (the 16-bit
workspace copy) through the attention output and the mask words.

What these tests cannot tell: which of the two store paths a wave took.  Both give the same
bytes, so the tests pin the results at the shapes where the paths change over (and that a
block store never reaches a row or a byte that is not the tail's); that the block path is
taken at all shows only in the kernel trace.  The records are read one
per lane in every wave (block record loads were measured and not kept)."""
import functools

import numpy as np
import pytest
import torch

import topk_cases as TC
from gpu_support import OUT_TOL, M, attn_entry, dev, host, out_rows_close, same, same_bits  # noqa: F401
from oracle import mx_oracle as O

pytestmark = pytest.mark.gpu

SHAPES = {"rows64": (1, 64), "rows70": (2, 35), "rows2x197": (2, 197)}  # (H, N): H * N rows of B = 1
SENTINEL = -0x0123456789ABCDEF


@functools.lru_cache(maxsize=None)
def _inputs(H, N, T):
    """q, k, v and the oracle's ex_pred scores (H * N, T), computed once; no test writes to them"""
    rng = np.random.default_rng(10000 * H + 100 * N + T)
    q = rng.standard_normal((1, H, N, 64), dtype=np.float32)
    kk = rng.standard_normal((1, H, T, 64), dtype=np.float32)
    v = rng.standard_normal((1, H, T, 64), dtype=np.float32)
    return q, kk, v, _pred(q, kk)


def _pred(q, kk):
    aq, ak = O.approx_operands(q, kk, "ex_pred")
    return O.exact_matmul_f32(aq, np.swapaxes(ak, -1, -2)).reshape(-1, kk.shape[2])


def _attention(M, q, kk, v, k, idx="new", mask=True):
    """mxa_attention (ex_pred) through the C ABI: idx "new" (a fresh int64 tensor), None (no idx
    output: the kept indices stay in the workspace's 16-bit copy) or a caller's int64 tensor
    of H * N * k elements, written in place.  Returns out, idx, mask words on the host."""
    take = (() if idx is None else ("idx",)) + (("mask",) if mask else ())
    r = attn_entry(M, "mxa_attention", dev(q), dev(kk), dev(v), 0.125, take=take, k_top=k, idx=None if isinstance(idx, str) else idx)
    rows = lambda name: host(r[name]).reshape(-1, r[name].shape[-1] if r[name].dim() > 1 else k) if name in r else None
    return host(r["out"]), rows("idx"), rows("mask")


def _mask_bits(M, words, T):
    return host(M.unpack_mask(torch.from_numpy(words), T))


def _check_all_outputs(M, q, kk, v, k, want, what):
    """idx requested or not, prune mask requested or not: idx and mask against `want`, the
    attention output of every variant bit-identical to the first's"""
    T = kk.shape[2]
    out0 = None
    for with_idx in (True, False):
        for with_mask in (True, False):
            w = f"{what} idx={with_idx} mask={with_mask}"
            out, idx, words = _attention(M, q, kk, v, k, idx="new" if with_idx else None, mask=with_mask)
            if with_idx:
                same(idx, want, w + " idx")
            if with_mask:
                same(_mask_bits(M, words, T), O.prune_mask(want, T), w + " mask")
            if out0 is None:
                out0 = out
            same_bits(out, out0, w + " out")
    return out0


@pytest.mark.parametrize("k", [2, 19, 20, 21, 33])
@pytest.mark.parametrize("T", [33, 197, 256])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_fused_blocks(M, shape, T, k):
    """One full block (64 rows), a full block and a 6-row partial wave (70), blocks that straddle
    a head boundary (2 x 197); odd k: a row's index run is no multiple of 16 bytes.  (k = 2 on
    rows of 197 and 256 keys is std::partial_sort and never reaches the tail: kept as the
    control that those rows are untouched.)"""
    H, N = SHAPES[shape]
    q, kk, v, pred = _inputs(H, N, T)
    _, want = O.topk(pred, k)
    out = _check_all_outputs(M, q, kk, v, k, want, f"{shape} T{T} k{k}")
    if k == 20:
        ro = O.attention(q, kk, v, 0.125, k_top=k, pred_mode="ex_pred")
        assert O.normwise_rel_err(out, ro["out"]) <= OUT_TOL
        out_rows_close(out, ro, v, f"{shape} T{T} k{k} out")


@pytest.mark.parametrize("r", [0, 31, 63])
def test_non_pending_row_in_full_block(M, r):
    """A query row whose scores do not pack (test_packed_pass_fallback_rows' construction) at row
    r of an otherwise full block: the block keeps the per-lane stores, the row's result comes
    from the 64-bit pass, its neighbours' from the tail.  A second full block behind it."""
    T, k = 197, 20
    rng = np.random.default_rng(300 + r)
    q = rng.standard_normal((1, 1, 128, 64), dtype=np.float32)
    kk = rng.standard_normal((1, 1, T, 64), dtype=np.float32)
    v = rng.standard_normal((1, 1, T, 64), dtype=np.float32)
    q[0, 0, r, 32:] *= np.float32(2.0 ** 20)
    _, want = O.topk(_pred(q, kk), k)
    _check_all_outputs(M, q, kk, v, k, want, f"non-pending row {r}")


@pytest.mark.parametrize("k", [20, 21])
def test_idx_view_8_byte_aligned(M, k):
    """An idx output one int64 into a larger buffer: the same results, and the elements before
    and after the view keep their sentinel."""
    H, N = SHAPES["rows70"]
    q, kk, v, pred = _inputs(H, N, 197)
    _, want = O.topk(pred, k)
    n = H * N * k
    buf = torch.full((n + 3,), SENTINEL, dtype=torch.int64, device="cuda")
    view = buf[1:1 + n]
    assert view.data_ptr() % 16 == 8
    out, idx, words = _attention(M, q, kk, v, k, idx=view)
    same(idx, want, "idx")
    same(_mask_bits(M, words, 197), O.prune_mask(want, 197), "mask")
    got = host(buf)
    assert got[0] == SENTINEL and (got[1 + n:] == SENTINEL).all()
    out_a, idx_a, _ = _attention(M, q, kk, v, k)
    same(idx_a, want, "aligned idx")
    same_bits(out, out_a, "out")


@pytest.mark.parametrize("rows", [64, 70])
def test_standalone_values_stay_per_lane(M, rows):
    """M.topk(packed=True) with its values output on a full block and a block plus six rows of
    n = 197, k = 20: indices, values and mask words bit-exact."""
    n, k = 197, 20
    rng = np.random.default_rng(rows)
    x = rng.integers(-6, 7, (rows, n)).astype(np.float32) * np.float32(0.25)
    for i in range(0, rows, 3):  # distinct values among the tie-heavy rows
        x[i] = rng.permutation(n).astype(np.float32) * np.float32(0.5) - np.float32(40.0)
    want_v, want = O.topk(x, k)
    vals, idx, words = M.topk(dev(x), k, return_mask=True)
    same(host(idx), want, "idx")
    same_bits(host(vals), want_v, "values")
    same(host(M.unpack_mask(words, n)), O.prune_mask(want, n), "mask")
    vals, idx = M.topk(dev(x), k)
    same(host(idx), want, "idx, no mask")
    same_bits(host(vals), want_v, "values, no mask")


def test_depth_limit_handover_in_full_block(M):
    """The antiqsort_row(197, 33, high=True) adversary as approximate scores (topk_cases
    fused_inputs): its query rows reach introselect's depth limit in the selection kernel and
    hand [0, k) over for the sort (phase 1), inside full blocks of pending rows: the phase-1
    rows' results leave through the block stores like their neighbours'."""
    T, k = 197, 33
    q, kk, v, rank, qrows = TC.fused_inputs(T, k)
    pred = _pred(q, kk)
    for r in qrows:
        same(np.argsort(np.argsort(pred[r], kind="stable"), kind="stable"), rank, "score order")
    _, want = O.topk(pred, k)
    _check_all_outputs(M, q, kk, v, k, want, "depth-limit hand-over")
