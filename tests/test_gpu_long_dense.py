"""The dense branch and k > 64 on rows of 513 .. 1,024 keys on the device (mx_topk_attention ->
mxa_attention_full -> finish_qk_long_kernel, behind select_long_kernel on the top-k path), at both
widths: out bit for bit on the exact-result cases; true / pred / idx / mask bit for bit and out by
the norm and by the row-wise bound of finish_qk_kernel's arithmetic (n_add = ntb, chain = 8 ntb + 2)
on the peaked random inputs whose eligible shares test_long_dense_cpu.py asserts; the edges of the
tiling (a 17th block of one key, the 256-key chunk boundary, ragged and full last blocks, partial
query tiles, one to four D blocks); special values and both branches of the exact epilogue; the
launch plan's grid.y split; and the delegation of every other call to the existing route.  The
references are computed once in long_dense_cases.py and shared with the CPU file."""
import numpy as np
import pytest
import torch

import attn4_cases as A
import exact_out_cases as EC
import long_dense_cases as LC
import topk_cases as TC
from gpu_support import M, OUT_TOL, dev, dev_opt, host, out_close, out_row_bound, same, same_bits  # noqa: F401
from gpu_support import ELIGIBLE_ELEMS, ELIGIBLE_ROWS
from oracle import mx_oracle as O

pytestmark = pytest.mark.gpu
F32 = np.float32


def run(M, q, k, v, scale, bits=8, scores=True, **kw):
    """the op -> dict of host arrays (out; idx, mask on the top-k path; true, pred with scores)"""
    topk = kw.get("top_k", True)
    kw = {a: (dev(x) if isinstance(x, np.ndarray) else x) for a, x in kw.items()}
    res = M.mx_topk_attention(dev(q), dev(k), dev(v), scale, return_scores=scores, return_mask=topk, elem_bits=bits, **kw)
    torch.cuda.synchronize()
    got = dict(out=host(res[0]))
    if topk:
        got.update(idx=host(res[1]), mask=host(M.unpack_mask(res[-1], k.shape[-2])))
    else:
        assert res[1] is None
    if scores:
        got.update(true=host(res[2]), pred=host(res[3]))
    return got


def oracle(q, k, v, scale, bits=8, **kw):
    if "flush_subnormals" in kw:
        kw["flush"] = kw.pop("flush_subnormals")
    return (A.attention4 if bits == 4 else O.attention)(q, k, v, scale, **kw)


def check_scores(got, r, what):
    """true, and on the top-k path pred (absent with approx off), idx and the mask: equal values, NaN
    against NaN (gpu_support.same, as test_gpu_long_rows.py compares them)"""
    if "true" in got:
        same(got["true"], r["true"], what + " true")
        if "pred" in r:
            same(got["pred"], r["pred"], what + " pred")
    if "idx" in r:
        same(got["idx"], r["idx"], what + " idx")
        same(got["mask"], O.prune_mask(r["idx"], r["true"].shape[-1]), what + " mask")
    else:
        assert "idx" not in got


def rows_close(got, r, v, what, k, bits=8):
    """gpu_support.out_rows_close with finish_qk_kernel's n_add and chain, at either width"""
    bound, fin, (se, sr), kernel, _ = (A.out_row_bound4 if bits == 4 else out_row_bound)(r, v, LC.kernel_name(k))
    assert se <= ELIGIBLE_ELEMS and sr <= ELIGIBLE_ROWS, f"{what}: eligible elements {se:.4%}, rows {sr:.2%}"
    ref = np.asarray(r["out"])
    same(np.isnan(got), np.isnan(ref), what + " NaN pattern")
    err = np.abs(got[fin].astype(np.float64) - ref[fin].astype(np.float64))
    b = bound[fin]
    ratio = np.where(err == 0, 0.0, err / np.where(b > 0, b, 1e-300))
    worst = float(ratio.max()) if ratio.size else 0.0
    print(f"rows_close {what}: {kernel} w{bits}, eligible elements {se:.4%} rows {sr:.2%}, worst |got - ref| / (A + F) {worst:.3f}")
    if worst > 1:
        i = np.unravel_index(np.argmax(ratio), ratio.shape)
        raise AssertionError(f"{what}: |got - ref| / (A + F) = {worst:.3f} at row {np.argwhere(fin)[i[0]].tolist()} "
                             f"column {i[1]}: got {got[fin][i]!r} want {ref[fin][i]!r} bound {b[i]:.3e}")


# ---- 1. the exact-result cases, bit for bit --------------------------------------------------------------
def _exact(M, c, bits):
    q, kk, v, bias = A.exact_inputs(c) if bits == 4 else EC.inputs(c)
    r = A.exact_reference(c) if bits == 4 else EC.reference(c)
    kw = dict(c.kw)
    kw.update(dict(k_top=c.k) if c.k else dict(top_k=False))
    for scores in (False, True):  # the plain and the EXTRA instantiations (a bias / bfloat: EXTRA both times)
        got = run(M, q, kk, v, EC.SCALE, bits, scores, bias=dev_opt(bias), **kw)
        w = f"{LC.case_id(c)} w{bits} scores={scores}"
        if c.k:
            same(got["idx"], r["idx"], w + " idx")
            same(got["mask"], O.prune_mask(r["idx"], c.T), w + " mask")
        if scores:
            same(got["true"], r["true"], w + " true")
        same_bits(got["out"], r["out"], w + " out")


@pytest.mark.parametrize("c", LC.EXACT + LC.EXACT_BF16, ids=LC.case_id)
def test_exact_out(M, c):
    _exact(M, c, 8)


@pytest.mark.parametrize("c", LC.EXACT4, ids=LC.case_id)
def test_exact_out4(M, c):
    _exact(M, c, 4)


# ---- 2. against the oracle on the peaked random inputs ---------------------------------------------------
@pytest.mark.parametrize("c", LC.ROWS + LC.ROWS4, ids=LC.rcase_id)
def test_rows_vs_oracle(M, c):
    q, k, v, bias = LC.r_inputs(c)
    r = LC.r_reference(c)
    got = run(M, q, k, v, LC.r_scale(c), c.bits, True, bias=dev_opt(bias), **LC.r_kw(c))
    what = LC.rcase_id(c)
    check_scores(got, r, what)
    out_close(got["out"], r["out"], OUT_TOL, what + " out")
    rows_close(got["out"], r, v, what, c.k, c.bits)


# ---- 3. the edges of the tiling ----------------------------------------------------------------------------
def rnd(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape, dtype=F32)


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
def _full(M, q, k, v, scale, bits, **kw):
    """mxa_attention_full called directly with every output -> (out, idx, true, pred, mask) tensors"""
    kt, topk = kw.get("k_top", 20), kw.get("top_k", True)
    p, dv, (B, H, Nq, T, D), _ = M.ops._attn_params(q, k, v, scale, kt, "ex_pred", topk, topk, None, False, 0, None)
    out = torch.empty((B, H, Nq, D), dtype=torch.float32, device=dv)
    M.ops._bind_out(p, out)
    idx = M.ops._new_idx(p, B, H, Nq, kt, topk, dv)
    mask = torch.empty((B, H, Nq, (T + 31) // 32), dtype=torch.int32, device=dv) if topk else None
    true_s = torch.empty((B, H, Nq, T), dtype=torch.float32, device=dv)
    pred_s = torch.full((B, H, Nq, T), float("nan"), dtype=torch.float32, device=dv)
    p.true_out, p.pred_out = true_s.data_ptr(), pred_s.data_ptr()
    if topk:
        p.mask_out = mask.data_ptr()
    lib = M._native.lib()
    M.ops._call_with_workspace(lib.mxa_attention_full_workspace_bytes, lib.mxa_attention_full, "mxa_attention_full", p, bits,
                               dev=dv)
    torch.cuda.synchronize()
    return out, idx, true_s, pred_s, mask


@pytest.mark.parametrize("T,kw,widths", [(197, dict(k_top=20), (8, 4)), (256, dict(k_top=154), (8, 4)), (120, dict(top_k=False), (8, 4)),
                                         (300, dict(top_k=False), (8,)), (300, dict(k_top=100), (8,)), (600, dict(k_top=20), (8, 4)),
                                         (1000, dict(k_top=64), (8, 4))])
def test_other_calls_are_byte_identical(M, T, kw, widths):
    """T <= 512, and k <= 64 on longer rows: the new entry point runs today's route"""
    q, k, v = (dev(rnd((1, 2, n, 64), 60 + j)) for j, n in enumerate((40, T, T)))
    for bits in widths:
        ref = M.mx_topk_attention(q, k, v, 0.125, return_scores=True, return_mask=kw.get("top_k", True), elem_bits=bits, **kw)
        got = _full(M, q, k, v, 0.125, bits, **kw)
        bits32 = lambda a: a.view(torch.int32) if a.dtype == torch.float32 else a
        for a, b, what in zip(got, tuple(ref) + (None,), ("out", "idx", "true", "pred", "mask")):
            if b is None:
                assert a is None or what == "mask" and not kw.get("top_k", True), what
            else:
                assert torch.equal(bits32(a), bits32(b)), (what, bits)


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
    lib = M._native.lib()
    p, d, _, keep = M.ops._attn_params(q, k, v, scale, 129, "ex_pred", True, True, None, False, 0, None)
    out = torch.full_like(want, float("nan"))
    M.ops._bind_out(p, out)
    assert not p.idx_out and not p.mask_out
    M.ops._call_with_workspace(lib.mxa_attention_full_workspace_bytes, lib.mxa_attention_full, "mxa_attention_full", p, 8, dev=d)
    torch.cuda.synchronize()
    assert torch.equal(out, want)
