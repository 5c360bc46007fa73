"""The fused op on rows of 513 .. 1,024 keys with k <= 64 (mx_topk_attention / mx_approx_scores on
select_long_kernel and finish16_kernel's long variant; mxa_attention_long called directly): true and approximate scores, kept indices and prune-mask
words bit-exact against the oracle (the reference itself for the fixture), the output within
OUT_TOL with an equal NaN pattern.  Shapes: N = 20 is one full 16-row tile and a partial one;
T = 513 / 1000 / 1024 one key past the short rows, a ragged last 32-block, the full mirror;
D = 32 / 72 / 128 one, three and four MX blocks; k = 7 / 16 / 20 / 64 both top-k branches
(k * 64 <= T is partial_sort) and every slot count of the finishing kernel."""
import numpy as np
import pytest
import torch

import topk_cases as TC
from gpu_support import OUT_TOL, M, attn_entry, attn_run as run, check_attn, dev, host, load, out_close  # noqa: F401
from gpu_support import out_rows_close, rnd, same
from oracle import mx_oracle as O

pytestmark = pytest.mark.gpu


def qkv(B, H, N, T, D, seed):
    return rnd((B, H, N, D), seed), rnd((B, H, T, D), seed + 1), rnd((B, H, T, D), seed + 2)


def check(got, ref, what, v=None):
    """ref: the oracle's (or the reference's) true, pred (absent with approx off), idx, out; v: of
    a float32 call with bfloat 0 / 32 and no flush checked against the oracle -- the row-wise
    bound beside the norm"""
    check_attn(got, ref, what)
    out_close(got["out"], ref["out"], OUT_TOL, what + " out")
    if v is not None:
        out_rows_close(got["out"], ref, v, what + " out")


# ---- 1. the reference's own arrays --------------------------------------------------------------
@pytest.mark.parametrize("mode", ["ex_pred", "MXINT4"])
def test_long_rows_vs_reference(M, mode):
    d = load("attn_long.npz")
    got = run(M, d["q"], d["k"], d["v"], float(d["scale"]), k_top=int(d["k_top"]), pred_mode=mode)
    check(got, dict(true=d["true"], pred=d[f"{mode}/pred"], idx=d[f"{mode}/idx"], out=d[f"{mode}/out"]), mode)


# ---- 2. ex_pred over the grid -------------------------------------------------------------------
@pytest.mark.parametrize("k", [7, 16, 20, 64])
@pytest.mark.parametrize("T", [513, 1000, 1024])
@pytest.mark.parametrize("D", [32, 72, 128])
def test_long_rows_expred_grid(M, D, T, k):
    q, kk, v = qkv(1, 2, 20, T, D, 1000 * D + T)
    scale = float(D) ** -0.5
    check(run(M, q, kk, v, scale, k_top=k), O.attention(q, kk, v, scale, k_top=k), f"D{D} T{T} k{k}", v)


# ---- 3. the other approximators, and the true scores ranked --------------------------------------
@pytest.mark.parametrize("D,T", [(72, 1000), (128, 1024)])
@pytest.mark.parametrize("mode", ["partial_Q", "partial_K", "MXINT4", "two_step_leading_ones", "true_ex", "true"])
def test_long_rows_modes(M, mode, D, T):
    q, kk, v = qkv(1, 2, 20, T, D, 77 * D + len(mode))
    q[0, 0, :, ::7] = 0.0  # zero elements (true_ex's zero indicators)
    kw = dict(approx=False) if mode == "true" else dict(pred_mode=mode)
    scale = float(D) ** -0.5
    check(run(M, q, kk, v, scale, k_top=20, **kw), O.attention(q, kk, v, scale, k_top=20, **kw), f"{mode} D{D} T{T}",
          v)


@pytest.mark.parametrize("D,T", [(72, 600), (64, 1024)])  # (the head dims the structured matrix exists for)
def test_long_rows_elsa(M, D, T):
    from mx_quantization_amd.funcs import _create_structured_orthogonal_matrix
    torch.manual_seed(D)
    proj = _create_structured_orthogonal_matrix(D).numpy()
    q, kk, v = qkv(1, 1, T, T, D, D + T)
    kk[0, 0, 5, :] = 0.0  # a zero key row: zero norm scales query row 5
    scale = float(D) ** -0.5
    got = run(M, q, kk, v, scale, k_top=20, pred_mode="ELSA", elsa_proj=proj)
    check(got, O.attention(q, kk, v, scale, k_top=20, pred_mode="ELSA", elsa_proj=proj), f"ELSA D{D} T{T}", v)


# ---- 4. special rows -----------------------------------------------------------------------------
@pytest.mark.parametrize("D", [64, 72])
def test_long_rows_special_rows(M, D):
    """test_expred_special_rows' set on rows of 600 keys, the special keys on both sides of key 512."""
    B, H, N, T = 2, 4, 96, 600
    q, kk, v = qkv(B, H, N, T, D, 5 + D)
    kk[0, 0, 7, :] = 0.0                        # zero key rows: exponent -126 blocks
    kk[0, 0, 577, :] = 0.0
    kk[0, 1, 11, 32:] *= np.float32(2.0 ** 40)  # exponent spread > 24 bits
    kk[0, 1, 530, 32:] *= np.float32(2.0 ** 40)
    q[0, 2, 3, 5] = np.nan                      # NaN row
    q[0, 2, 9, 40] = np.inf                     # Inf row
    kk[1, 0, 550, 3] = np.nan                   # NaN key
    q[1, 1, 17, :] *= np.float32(2.0 ** 100)    # true scores overflow for this row
    kk[1, 1, :, :] *= np.float32(2.0 ** 30)
    q[1, 2, :4, :] = 0.0                        # zero query rows: every pred ties across 600 keys
    # block exponents across the ex_pred key loop's fast range [-50, 61] (kExpFastLo / Hi)
    steps = (np.float32(2.0) ** np.arange(59, 64, dtype=np.float32).repeat(8))[:, None]
    kk[1, 3, :40, :] *= steps
    kk[1, 3, 520:560, :] *= steps
    q[1, 3, 40:80, :] *= (np.float32(2.0) ** -np.arange(49, 54, dtype=np.float32).repeat(8))[:, None]
    kk[1, 3, 100, 32:] *= np.float32(2.0 ** -60)
    kk[1, 3, 590, 32:] *= np.float32(2.0 ** -60)
    check(run(M, q, kk, v, 0.125, k_top=20), O.attention(q, kk, v, 0.125, k_top=20), f"special D{D}", v)


# ---- 5. bias -------------------------------------------------------------------------------------
@pytest.mark.parametrize("flush", [False, True])
@pytest.mark.parametrize("mode", ["ex_pred", "MXINT4"])
def test_long_rows_bias(M, mode, flush):
    B, H, N, T, D = 2, 2, 20, 1000, 72
    q, kk, v = qkv(B, H, N, T, D, 31)
    bias = np.zeros((B, 1, N, T), np.float32)
    bias[:, :, :, T // 2:] = -10000.0
    bias[1, 0, 2, :] = -np.inf  # every key masked: the row's softmax is NaN
    scale = float(D) ** -0.5
    got = run(M, q, kk, v, scale, k_top=20, pred_mode=mode, bias=bias, flush_subnormals=flush)
    check(got, O.attention(q, kk, v, scale, k_top=20, pred_mode=mode, bias=bias, flush=flush), f"bias {mode} flush={flush}",
          None if flush else v)


# ---- 6. the depth limit and ties ------------------------------------------------------------------
@pytest.mark.parametrize("T,k,mode", [(1024, 20, "ex_pred"), (1000, 33, "ex_pred"), (600, 5, "ex_pred"),
                                      (1024, 20, "MXINT4"), (1024, 20, "true_ex")])
def test_long_rows_depth_limit(M, T, k, mode):
    """topk_cases.fused_inputs: head 0's adversarial query rows meet the row that exhausts
    introselect's depth limit (ex_pred: test_long_rows_cpu pins the scores' order); the other
    rows are random, full of ties.  Every query row's pred, idx and mask."""
    q, kk, v, _, _ = TC.fused_inputs(T, k)
    check(run(M, q, kk, v, 0.125, k_top=k, pred_mode=mode), O.attention(q, kk, v, 0.125, k_top=k, pred_mode=mode),
          f"adversary T{T} k{k} {mode}", v)


# ---- 7. one full-size head group -------------------------------------------------------------------
def test_long_rows_full_size_heads(M):
    """PixArt 512x512 self-attention's rows, four heads: 64 tiles per head, the rows_per_wg
    chunking of both kernels.  Every row's idx against the oracle; out for head 0."""
    H, N, D, k = 4, 1024, 72, 20
    q, kk, v = qkv(1, H, N, N, D, 2024)
    scale = float(D) ** -0.5
    out, idx = M.mx_topk_attention(dev(q), dev(kk), dev(v), scale, k_top=k)
    torch.cuda.synchronize()
    aq, ak = O.approx_operands(q, kk, "ex_pred")
    _, want = O.topk(O.exact_matmul_f32(aq, np.swapaxes(ak, -1, -2)), k)
    same(host(idx), want, "idx (every row)")
    r = O.attention(q[:, :1], kk[:, :1], v[:, :1], scale, k_top=k)
    same(r["idx"], want[:, :1], "oracle idx")
    out_close(host(out)[:, :1], r["out"], OUT_TOL, "out (head 0)")


# ---- 8. bfloat16 elementwise rounding --------------------------------------------------------------
def test_long_rows_bfloat16(M):
    q, kk, v = qkv(1, 2, 20, 1000, 72, 16)
    scale = 72.0 ** -0.5
    check(run(M, q, kk, v, scale, k_top=20, bfloat=16), O.attention(q, kk, v, scale, k_top=20, bfloat=16), "bfloat16")


# ---- 9. the caller takes no idx and no mask: the 16-bit workspace copy -----------------------------
def test_long_rows_without_idx_out(M):
    q, kk, v = (dev(x) for x in qkv(1, 2, 20, 1000, 72, 9))
    scale = 72.0 ** -0.5
    want, _, mask = M.mx_topk_attention(q, kk, v, scale, k_top=20, return_mask=True)
    got = attn_entry(M, "mxa_attention_long", q, kk, v, scale, take=(), k_top=20)
    assert set(got) == {"out"}
    assert torch.equal(got["out"], want)


# ---- 10. the scores alone ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["ex_pred", "MXINT4", "true_ex"])
def test_long_rows_approx_scores(M, mode):
    q, kk, _ = qkv(1, 2, 20, 1000, 72, 40)
    aq, ak = O.approx_operands(q, kk, mode)
    same(host(M.mx_approx_scores(dev(q), dev(kk), mode)), O.exact_matmul_f32(aq, np.swapaxes(ak, -1, -2)), mode + " pred")
