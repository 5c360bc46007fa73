"""The dense branch and k > 64 on rows of 513 .. 1,024 keys on the device (mx_topk_attention ->
mxa_attention_full -> finish_qk_long_kernel, behind select_long_kernel on the top-k path), at both
widths: out bit for bit on the exact-result cases; true / pred / idx / mask bit for bit and out by
the norm and by the row-wise bound of finish_qk_kernel's arithmetic (n_add = ntb, chain = 8 ntb + 2)
on the peaked random inputs whose eligible shares test_long_dense_cpu.py asserts; the edges of the
tiling (a 17th block of one key, the 256-key chunk boundary, ragged and full last blocks, partial
query tiles, one to four D blocks); special values and both branches of the exact epilogue; the
launch plan's grid.y split; and, for the calls the sibling entry points take too, every accepting
entry point's outputs against mxa_attention_full's and the op's, bit for bit.  The
references are computed once in long_dense_cases.py and shared with the CPU file."""
import numpy as np
import pytest
import torch

import attn4_cases as A
import exact_out_cases as EC
import long_dense_cases as LC
import topk_cases as TC
from gpu_support import ELEM, M, OUT_TOL, attn_entry, attn_run as run, check_attn as check_scores, check_exact_out  # noqa: F401
from gpu_support import check_siblings, dev, out_close, out_rows_close, r_kw, r_scale, rnd, same, same_bits
from oracle import mx_oracle as O

pytestmark = pytest.mark.gpu
F32 = np.float32


def oracle(q, k, v, scale, bits=8, **kw):
    if "flush_subnormals" in kw:
        kw["flush"] = kw.pop("flush_subnormals")
    return O.attention(q, k, v, scale, elem=ELEM[bits], **kw)


# ---- 1. the exact-result cases, bit for bit --------------------------------------------------------------
@pytest.mark.parametrize("c", LC.EXACT + LC.EXACT_BF16, ids=LC.case_id)
def test_exact_out(M, c):
    check_exact_out(M, c, EC.inputs(c), EC.reference(c), EC.SCALE, 8, LC.case_id(c))


@pytest.mark.parametrize("c", LC.EXACT4, ids=LC.case_id)
def test_exact_out4(M, c):
    check_exact_out(M, c, A.exact_inputs(c), A.exact_reference(c), EC.SCALE, 4, LC.case_id(c))


# ---- 2. against the oracle on the peaked random inputs ---------------------------------------------------
@pytest.mark.parametrize("c", LC.ROWS + LC.ROWS4, ids=LC.rcase_id)
def test_rows_vs_oracle(M, c):
    q, k, v, bias = LC.r_inputs(c)
    r = LC.r_reference(c)
    got = run(M, q, k, v, r_scale(c), c.bits, True, bias=bias, **r_kw(c))
    what = LC.rcase_id(c)
    check_scores(got, r, what)
    out_close(got["out"], r["out"], OUT_TOL, what + " out")
    out_rows_close(got["out"], r, v, what, LC.kernel_name(c.k), c.bits)  # finish_qk_kernel's n_add and chain


# ---- 3. the edges of the tiling ----------------------------------------------------------------------------
EDGES = [(513, 1, 8), (513, 33, 72), (768, 17, 32), (769, 33, 128), (1000, 17, 72), (1000, 1, 128), (1024, 33, 8),
         (1024, 17, 32)]


@pytest.mark.parametrize("T,N,D", EDGES)
def test_tiling_edges(M, T, N, D):
    q, k, v = rnd((1, 2, N, D), T + N), rnd((1, 2, T, D), T + N + 1), rnd((1, 2, T, D), T + N + 2)
    scale = float(D) ** -0.5
    what = f"T{T} N{N} D{D}"
    dense = run(M, q, k, v, scale, top_k=False)
    r = oracle(q, k, v, scale, top_k=False)
    check_scores(dense, r, what + " dense")
    out_close(dense["out"], r["out"], OUT_TOL, what + " dense out")
    for kt in (65, 512, T):
        got = run(M, q, k, v, scale, k_top=kt)
        r = oracle(q, k, v, scale, k_top=kt)
        check_scores(got, r, f"{what} k{kt}")
        out_close(got["out"], r["out"], OUT_TOL, f"{what} k{kt} out")
        if kt == T:  # the same kernel with every mask bit set
            same_bits(got["out"], dense["out"], what + " k = T against dense")


def test_k_equal_T_is_dense_at_width_4(M):
    T, N, D = 769, 17, 72
    q, k, v = rnd((1, 2, N, D), 4), rnd((1, 2, T, D), 5), rnd((1, 2, T, D), 6)
    dense, full = run(M, q, k, v, 0.125, 4, top_k=False), run(M, q, k, v, 0.125, 4, k_top=T)
    same_bits(full["out"], dense["out"], "k = T against dense")
    r = oracle(q, k, v, 0.125, 4, top_k=False)
    check_scores(dense, r, "w4 dense")
    out_close(dense["out"], r["out"], OUT_TOL, "w4 dense out")


# ---- 4. special values -------------------------------------------------------------------------------------
def _both(M, q, k, v, scale, what, kt=65, **kw):
    """the dense branch and k = kt against the oracle: true (pred, idx, mask) bit for bit, the NaN pattern
    of out and its finite elements by the norm"""
    okw = dict(kw)
    for sel in (dict(top_k=False), dict(k_top=kt)):
        got = run(M, q, k, v, scale, **sel, **kw)
        r = oracle(q, k, v, scale, **sel, **okw)
        check_scores(got, r, f"{what} {sel}")
        out_close(got["out"], r["out"], OUT_TOL, f"{what} {sel} out")
    return r


def test_nan_query_row_and_key(M):
    q, k, v = rnd((1, 2, 33, 64), 41), rnd((1, 2, 513, 64), 42), rnd((1, 2, 513, 64), 43)
    q[0, 0, 3, 5] = np.nan
    k[0, 1, 512, 40] = np.nan
    r = _both(M, q, k, v, 0.125, "NaN")
    assert np.isnan(r["out"][0, 0, 3]).all() and np.isfinite(r["out"][0, 0, 4]).all()


def test_masked_rows(M):
    """a bias row that is -inf throughout (a NaN output row) and one that leaves 20 finite keys, fewer
    than one block (k = 65 keeps 45 keys of score -inf beside them)"""
    q, k, v = rnd((1, 2, 33, 64), 44), rnd((1, 2, 513, 64), 45), rnd((1, 2, 513, 64), 46)
    bias = np.zeros((1, 1, 33, 513), F32)
    bias[0, 0, 2, :] = -np.inf
    bias[0, 0, 17, :] = -np.inf
    bias[0, 0, 17, 500:513] = 0.0
    bias[0, 0, 17, 7:14] = 0.0
    assert np.isfinite(bias[0, 0, 17]).sum() == 20
    r = _both(M, q, k, v, 0.125, "masked", bias=bias, approx=False)
    assert np.isnan(r["out"][0, :, 2]).all() and np.isfinite(r["out"][0, :, 17]).all()


@pytest.mark.parametrize("which", ["fast", "spread", "tiny", "huge"])
def test_exact_epilogue_branches(M, which):
    """both forms of the exact epilogue and fq_exact's fp64 sum (test_long_dense_cpu.py asserts from the
    oracle's block exponents which each input takes); "tiny" again with flush_subnormals"""
    q, k, v = LC.epilogue_inputs(which)
    _both(M, q, k, v, 0.125, which)
    if which == "tiny":
        _both(M, q, k, v, 0.125, which + " flush", flush_subnormals=True)


def test_flush_subnormals_and_bfloat(M):
    q, k, v = rnd((1, 2, 17, 72), 47), rnd((1, 2, 600, 72), 48), rnd((1, 2, 600, 72), 49)
    _both(M, q, k, v, 72.0 ** -0.5, "flush", flush_subnormals=True)
    _both(M, q, k, v, 72.0 ** -0.5, "bfloat16", bfloat=16)


# ---- 5. launch planning ------------------------------------------------------------------------------------
def _all_idx(q, k, kt):
    aq, ak = O.approx_operands(q, k, "ex_pred")
    return O.topk(O.exact_matmul_f32(aq, np.swapaxes(ak, -1, -2)), kt)[1]


def test_one_head_of_1024_rows(M):
    """one head: its 64 tiles split over grid.y"""
    N, D, kt = 1024, 72, 154
    q, k, v = rnd((1, 1, N, D), 50), rnd((1, 1, N, D), 51), rnd((1, 1, N, D), 52)
    scale = float(D) ** -0.5
    got = run(M, q, k, v, scale, scores=False, k_top=kt)
    r = O.attention(q, k, v, scale, k_top=kt)
    same(got["idx"], r["idx"], "idx")
    out_close(got["out"], r["out"], OUT_TOL, "out")
    dense = run(M, q, k, v, scale, scores=False, top_k=False)
    out_close(dense["out"], O.attention(q, k, v, scale, top_k=False)["out"], OUT_TOL, "dense out")


def test_64_heads_of_33_rows(M):
    B, H, N, T, D, kt = 4, 16, 33, 513, 32, 65
    q, k, v = rnd((B, H, N, D), 53), rnd((B, H, T, D), 54), rnd((B, H, T, D), 55)
    scale = float(D) ** -0.5
    got = run(M, q, k, v, scale, scores=False, k_top=kt)
    same(got["idx"], _all_idx(q, k, kt), "idx (every row)")
    r = O.attention(q[:1, :1], k[:1, :1], v[:1, :1], scale, k_top=kt)
    out_close(got["out"][:1, :1], r["out"], OUT_TOL, "out (head 0)")
    dense = run(M, q, k, v, scale, scores=False, top_k=False)
    for b, h in ((0, 0), (3, 15)):
        r = O.attention(q[b:b + 1, h:h + 1], k[b:b + 1, h:h + 1], v[b:b + 1, h:h + 1], scale, top_k=False)
        out_close(dense["out"][b:b + 1, h:h + 1], r["out"], OUT_TOL, f"dense out (head {b}, {h})")


# ---- 6. delegation -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,kw,widths", [(197, dict(k_top=20), (8, 4)), (256, dict(k_top=154), (8, 4)), (120, dict(top_k=False), (8, 4)),
                                         (300, dict(top_k=False), (8,)), (300, dict(k_top=100), (8,)), (600, dict(k_top=20), (8, 4)),
                                         (1000, dict(k_top=64), (8, 4)), (70, dict(k_top=20), (8, 4))])
def test_other_calls_are_byte_identical(M, T, kw, widths):
    """T <= 512, and k <= 64 on longer rows: every entry point that accepts the call, called directly,
    writes the bytes mxa_attention_full writes -- out, idx, true, pred and the mask words -- and so does
    M.mx_topk_attention; the same for the scores alone (mxa_approx_scores, _long, _bits and
    M.mx_approx_scores)"""
    q, k, v = (dev(rnd((1, 2, n, 64), 60 + j)) for j, n in enumerate((40, T, T)))
    check_siblings(M, q, k, v, 0.125, widths, **kw)


def test_depth_limit_adversary_above_k_64(M):
    """select_long_kernel behind the fused path at k = 129: head 0's adversarial query rows meet the
    row that exhausts introselect's depth limit (topk_cases.fused_inputs)"""
    T, kt = 1000, 129
    q, k, v, _, qrows = TC.fused_inputs(T, kt)
    got = run(M, q, k, v, 0.125, scores=False, k_top=kt)
    want = _all_idx(q, k, kt)
    same(got["idx"], want, "idx (every row)")
    same(got["mask"], O.prune_mask(want, T), "mask")
    rows = sorted(set(qrows[:8]) | set(range(8)))
    r = O.attention(q[:, :, rows], k, v, 0.125, k_top=kt)
    same(r["idx"], want[:, :, rows], "oracle idx")
    out_close(got["out"][:, :, rows], r["out"], OUT_TOL, "out (the adversarial rows and eight more)")


def test_without_idx_and_mask_out(M):
    """the caller takes neither idx nor mask: the 16-bit index copy and the workspace's mask words"""
    q, k, v = (dev(x) for x in (rnd((1, 2, 33, 72), 70), rnd((1, 2, 1000, 72), 71), rnd((1, 2, 1000, 72), 72)))
    scale = 72.0 ** -0.5
    want = M.mx_topk_attention(q, k, v, scale, k_top=129, return_mask=True)[0]
    got = attn_entry(M, "mxa_attention_full", q, k, v, scale, 8, take=(), k_top=129)
    assert set(got) == {"out"}
    assert torch.equal(got["out"], want)
