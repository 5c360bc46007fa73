"""The fused op and topk on rows of 1,025 .. 4,096 keys (mxa_attention_xl: select_xl_kernel and
finish16_xl_kernel; mxa_topk_xl), k <= 64 and k * 64 <= T -- torch's partial_sort regime.
Kept indices, prune-mask words and scores bit for bit against the oracle, the output row by row
(out_rows_close) and within OUT_TOL.  B = 1, H = 2, N = 33: two 16-row tiles and a ragged row.
(T, k): 1025 / 16 the smallest accepted row; 1280 / 20 the k * 64 == T edge; 2085 / 20 a ragged
last 32-block, a ragged 64-key scan step and a three-block last chunk; 4096 / 20 and / 64 the
full four chunks and the full heap; 4095 / 1 a heap of one.  ex_pred's scores tie heavily, so
the ordinary cases exercise the tie order."""
import functools

import numpy as np
import pytest
import torch

from gpu_support import ELEM, OUT_TOL, M, attn_entry, attn_run, check_attn, dev, host, out_close  # noqa: F401
from gpu_support import out_rows_close, rnd, same, same_bits, to_bits
from oracle import mx_oracle as O

pytestmark = pytest.mark.gpu

TK = [(1025, 16), (1280, 20), (2085, 20), (4096, 20), (4096, 64), (4095, 1)]
N = 33


def mode_kw(mode):
    return dict(approx=False) if mode == "true" else dict(pred_mode=mode)


@functools.lru_cache(maxsize=None)
def case(T, k, D, mode, bits=8, biased=False, H=2, n=N):
    """inputs and the oracle's result, computed once"""
    seed = 7 * T + 131 * k + D
    q, kk, v = rnd((1, H, n, D), seed), rnd((1, H, T, D), seed + 1), rnd((1, H, T, D), seed + 2)
    bias = None
    if biased:  # PixArt's key mask: (B, 1, 1, T), 0 / -10000
        bias = np.zeros((1, 1, 1, T), np.float32)
        bias[..., T // 3:T // 2] = -10000.0
    scale = float(np.float32(D ** -0.5))
    ref = O.attention(q, kk, v, scale, k_top=k, bias=bias, elem=ELEM[bits], **mode_kw(mode))
    return q, kk, v, bias, scale, ref


def check_case(M, T, k, D, mode, bits=8, biased=False):
    q, kk, v, bias, scale, ref = case(T, k, D, mode, bits, biased)
    what = f"T{T} k{k} D{D} {mode} w{bits}" + (" bias" if biased else "")
    kw = dict(k_top=k, **mode_kw(mode), **(dict(bias=bias) if biased else {}))
    got = attn_run(M, q, kk, v, scale, bits, **kw)  # with the scores: the finishing kernel's EXTRA form
    check_attn(got, ref, what, same_bits)
    out_close(got["out"], ref["out"], OUT_TOL, what + " out")
    out_rows_close(got["out"], ref, v, what + " out", bits=bits)
    plain = attn_run(M, q, kk, v, scale, bits, scores=False, **kw)  # ... and without them (no bias: its plain form)
    same(plain["idx"], got["idx"], what + " idx without the scores")
    same_bits(plain["out"], got["out"], what + " out without the scores")


@pytest.mark.parametrize("mode", ["ex_pred", "MXINT4", "true"])
@pytest.mark.parametrize("D", [32, 72])
@pytest.mark.parametrize("T,k", TK)
def test_xl_rows(M, T, k, D, mode):
    check_case(M, T, k, D, mode)


@pytest.mark.parametrize("mode", ["ex_pred", "MXINT4"])
@pytest.mark.parametrize("T,k", [(1280, 20), (4096, 64)])
def test_xl_rows_mxint4_elements(M, T, k, mode):
    check_case(M, T, k, 72, mode, bits=4)


def test_xl_rows_mask_bias(M):
    check_case(M, 2085, 20, 72, "ex_pred", biased=True)


def test_v_nan_in_a_block_no_row_keeps(M):
    """the reference's dense 0 * NaN: one NaN element of V makes its block's scale NaN, and that
    poisons the element's output column in every row though no row keeps a key of the block"""
    T, k, D, c = 4096, 20, 72, 37
    q, kk, v, _, scale, ref = case(T, k, D, "ex_pred", H=1, n=4)
    free = np.setdiff1d(np.arange(T // 32), np.unique(ref["idx"] // 32))
    assert free.size, "a key block that no row keeps"
    vn = v.copy()
    vn[0, 0, 32 * free[free.size // 2] + 5, c] = np.nan
    got = attn_run(M, q, kk, v, scale, k_top=k, scores=False)["out"]
    gotn = attn_run(M, q, kk, vn, scale, k_top=k, scores=False)["out"]
    same(np.isnan(gotn), np.isnan(O.attention(q, kk, vn, scale, k_top=k)["out"]), "NaN pattern")
    assert np.isnan(gotn[..., c]).all() and not np.isnan(got).any()
    others = np.arange(D) != c
    same_bits(gotn[..., others], got[..., others], "the other columns")


# ---- topk: torch.topk on the CPU tensor is the specification ------------------------------------------
def topk_rows(n):
    g = np.random.default_rng(n)
    special = g.standard_normal(n).astype(np.float32)
    special[g.permutation(n)[:60]] = np.tile(np.array([np.nan, 0.0, -0.0, np.inf, -np.inf], np.float32), 12)
    up = np.arange(n, dtype=np.float32)
    rows = [g.standard_normal(n).astype(np.float32) for _ in range(4)]
    rows += [up, up[::-1], np.full(n, 1.5, np.float32), g.integers(0, 7, n).astype(np.float32), special]
    return torch.from_numpy(np.stack(rows))


NK = [(1025, 16), (1025, 1), (1280, 20), (1280, 1), (2085, 32), (2085, 1), (4096, 64), (4096, 1)]  # k: the largest allowed, and 1


@pytest.mark.parametrize("n,k,dt", [nk + (torch.float32,) for nk in NK] + [(2085, 32, torch.float16), (2085, 32, torch.bfloat16)],
                         ids=str)
def test_topk_xl(M, n, k, dt):
    x = topk_rows(n).to(dt)
    wv, wi = torch.topk(x, k, dim=-1)
    gv, gi, gm = M.topk(x.cuda(), k, return_mask=True)
    torch.cuda.synchronize()
    same(host(gi), wi.numpy(), f"n{n} k{k} idx")
    dts = {torch.float16: "f16", torch.bfloat16: "bf16"}.get(dt)
    same_bits(to_bits(gv), to_bits(wv), f"n{n} k{k} values", dt=dts, patterns=True)
    same(host(M.unpack_mask(gm, n)), O.prune_mask(wi.numpy(), n), f"n{n} k{k} mask")


# ---- siblings: mxa_attention_xl (the op) writes mxa_attention_full's bytes where both accept ----------
@pytest.mark.parametrize("T,kw", [(300, dict(k_top=20)), (1000, dict(k_top=20)), (600, dict(top_k=False))], ids=str)
def test_xl_writes_the_full_entry_points_bytes(M, T, kw):
    q, kk, v = dev(rnd((1, 2, N, 72), T)), dev(rnd((1, 2, T, 72), T + 1)), dev(rnd((1, 2, T, 72), T + 2))
    topk = kw.get("top_k", True)
    res = M.mx_topk_attention(q, kk, v, 0.125, return_scores=True, return_mask=topk, **kw)
    full = attn_entry(M, "mxa_attention_full", q, kk, v, 0.125, 8, **kw)
    op = dict(zip(("out", "idx", "true", "pred", "mask"), res))
    assert set(full) == {n for n, t in op.items() if t is not None}
    for name, t in full.items():
        assert torch.equal(t.view(torch.int32) if t.dtype == torch.float32 else t,
                           op[name].view(torch.int32) if t.dtype == torch.float32 else op[name]), name
