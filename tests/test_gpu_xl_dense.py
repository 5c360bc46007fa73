"""The dense branch on rows of 1,025 .. 4,096 keys on the device (mx_topk_attention -> mxa_attention_xl_full -> finish_qk_xl_kernel),
both widths.  N = 33: two 16-row tiles and a ragged one.  T: 1,025 a second chunk of one key; 2,085 a ragged last block and a two-block last
chunk; 3,840 / 4,096 PixArt-Sigma.  No row-wise bound (from the oracle alone 26 .. 100 % of such rows hold an eligible element): 1. and 3. instead."""
import numpy as np
import pytest

import attn4_cases as A
import exact_out_cases as EC
import long_dense_cases as LC
from gpu_support import ELEM, ENTRY_SIZES, M, OUT_TOL, _equal_bits, attn_entry, attn_run, check_attn, check_exact_out  # noqa: F401
from gpu_support import dev, out_close, rnd, same_bits
from oracle import mx_oracle as O
from test_xl_dense_cpu import EXACT4, EXACT8

pytestmark, F32, N = pytest.mark.gpu, np.float32, 33


def oracle(q, k, v, scale, bits=8, flush_subnormals=False, **kw):
    return O.attention(q, k, v, scale, top_k=False, elem=ELEM[bits], flush=flush_subnormals, **kw)


@pytest.mark.parametrize("c,bits", [(c, 8) for c in EXACT8] + [(c, 4) for c in EXACT4], ids=str)
def test_exact_out(M, c, bits):
    """1. out bit for bit (test_xl_dense_cpu.py asserts the cases' five conditions)"""
    inputs, r = (EC.inputs(c), EC.reference(c)) if bits == 8 else (A.exact_inputs(c), A.exact_reference(c))
    check_exact_out(M, c, inputs, r, EC.SCALE, bits, EC.case_id(c))


@pytest.mark.parametrize("T", [1025, 2085, 3840, 4096])
@pytest.mark.parametrize("D,bits", [(32, 8), (64, 8), (72, 8), (128, 8), (72, 4)])
def test_rows_vs_oracle(M, D, bits, T):
    """2. random inputs: true bit for bit, out by the norm; the plain instantiation's out equals the EXTRA one's"""
    q, k, v = rnd((1, 2, N, D), 7 * T + D), rnd((1, 2, T, D), 7 * T + D + 1), rnd((1, 2, T, D), 7 * T + D + 2)
    scale, what = float(F32(D ** -0.5)), f"T{T} D{D} w{bits}"
    r = oracle(q, k, v, scale, bits)
    got = attn_run(M, q, k, v, scale, bits, top_k=False)
    check_attn(got, r, what, same_bits)
    out_close(got["out"], r["out"], OUT_TOL, what + " out")
    same_bits(attn_run(M, q, k, v, scale, bits, scores=False, top_k=False)["out"], got["out"], what + " out without the scores")


@pytest.mark.parametrize("D", [72, 128])
def test_first_chunk_equals_the_long_kernel(M, D):
    """3. keys from 1,024 on masked to -inf (exp 0, zero P codes): finish_qk_long_kernel's sum chain and fmaf order give its bytes"""
    q, k, v = rnd((1, 2, N, D), 300 + D), rnd((1, 2, 2085, D), 301 + D), rnd((1, 2, 2085, D), 302 + D)
    bias = np.zeros((1, 1, 1, 2085), F32)
    bias[..., 1024:] = -np.inf
    for bits in (8, 4):
        a = attn_run(M, q, k, v, 0.125, bits, top_k=False, bias=bias)
        b = attn_run(M, q, k[:, :, :1024], v[:, :, :1024], 0.125, bits, top_k=False, bias=bias[..., :1024])
        same_bits(a["out"], b["out"], f"D{D} w{bits} out")
        same_bits(a["true"][..., :1024], b["true"], f"D{D} w{bits} true")


def special(which):  # 4. special values at T = 2,085, D = 64: (q, k, v, the op's keywords)
    if which in ("spread", "tiny", "tiny_flush"):  # both forms of the exact epilogue in every chunk (test_xl_dense_cpu.py)
        return (*LC.epilogue_inputs(which.split("_")[0], T=2085), dict(flush_subnormals=True) if "flush" in which else {})
    q, k, v = rnd((1, 2, N, 64), 41), rnd((1, 2, 2085, 64), 42), rnd((1, 2, 2085, 64), 43)
    if which == "nan":  # a NaN in one query row and in one key of the third chunk
        q[0, 0, 3, 5] = k[0, 1, 2060, 40] = np.nan
        return q, k, v, {}
    bias = np.zeros((1, 1, N, 2085), F32)  # "masked": a row that is -inf throughout; one with 20 finite keys, all in the last chunk
    bias[0, 0, (2, 17), :] = -np.inf
    bias[0, 0, 17, 2052:2072] = 0.0
    return q, k, v, dict(bias=bias)


@pytest.mark.parametrize("which", ["nan", "masked", "spread", "tiny", "tiny_flush"])
def test_special_values(M, which):
    q, k, v, kw = special(which)
    got, r = attn_run(M, q, k, v, 0.125, top_k=False, **kw), oracle(q, k, v, 0.125, **kw)
    check_attn(got, r, which)
    out_close(got["out"], r["out"], OUT_TOL, which + " out")
    assert which != "masked" or (np.isnan(r["out"][0, :, 2]).all() and np.isfinite(r["out"][0, :, 17]).all())


def test_one_head_of_4096_rows(M):
    """5. the launch plan: one head of 256 tiles, split over grid.y, several rounds per wave"""
    q, k, v = rnd((1, 1, 4096, 72), 50), rnd((1, 1, 4096, 72), 51), rnd((1, 1, 4096, 72), 52)
    got = attn_run(M, q, k, v, 0.125, scores=False, top_k=False)["out"]
    rows = list(range(48)) + list(range(4096 - 33, 4096))
    out_close(got[:, :, rows], oracle(q[:, :, rows], k, v, 0.125)["out"], OUT_TOL, "out (the first 48 and the last 33 rows)")


ENTRY_SIZES.setdefault("mxa_attention_xl", "mxa_attention_xl_workspace_bytes")  # (attn_entry's table of size functions)


@pytest.mark.parametrize("T,kw,name", [(600, dict(top_k=False), "mxa_attention_full"), (1000, dict(k_top=129), "mxa_attention_full"),
                                       (2085, dict(k_top=20), "mxa_attention_xl")], ids=str)
def test_writes_the_siblings_bytes(M, T, kw, name):
    """6. the op writes the bytes of the older entry points that take the call too"""
    q, kk, v = dev(rnd((1, 2, N, 72), T)), dev(rnd((1, 2, T, 72), T + 1)), dev(rnd((1, 2, T, 72), T + 2))
    res = M.mx_topk_attention(q, kk, v, 0.125, return_scores=True, return_mask=kw.get("top_k", True), **kw)  # (idx None on the dense branch)
    op = {n: t for n, t in zip(("out", "idx", "true", "pred", "mask"), res) if t is not None}
    _equal_bits(attn_entry(M, name, q, kk, v, 0.125, 8, **kw), op, name)
