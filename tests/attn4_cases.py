"""What the MXINT4 attention tests share (test_attn4_cpu.py, test_gpu_attn4.py): the exact-result
cases with a V that is its own MXINT4, and the GPU cases with their references (computed once,
left unchanged).  Nothing here touches the device.

The reference is the caller glue of the PixArt modules (MX_transformer_block.py:648-717,
:792-859) at a_elem_format = w_elem_format = "int4": matmul(q, k^T) and matmul(attn, v) quantize
their operands to MXINT4 and exponent_approximation builds every approximator from the MXINT4
MX_Q / MX_K: O.attention(elem="int4")."""
import collections
import functools

import numpy as np

import exact_out_cases as EC
import gpu_support as GS
from gpu_support import r_kw, r_scale, rnd  # noqa: F401
from oracle import mx_oracle as O

F32 = np.float32
MODES = ("ex_pred", "partial_Q", "partial_K", "MXINT4", "two_step_leading_ones", "true_ex")


def shares_within_caps(r, v):
    se, sr = GS.out_row_bound(r, v, bits=4)[2]
    return se <= GS.ELIGIBLE_ELEMS and sr <= GS.ELIGIBLE_ROWS, (se, sr)


def eligible_bf16(r, v, flush=False):
    """bfloat = 16: the P blocks whose MXINT4 codes or exponent may differ between two correct
    implementations.  P enters the output through its codes alone; the codes come from
    bf16(p), and two float32 softmaxes within tau of each other (gpu_support.out_row_bound's tau) round to
    different bfloat16 values only where p lies within tau of a bfloat16 rounding midpoint.
    Those elements are moved to their lower, then to their upper bfloat16 neighbour; a block whose
    codes or exponent change, or that holds two such elements, is eligible.  Returns the number of
    eligible blocks, the number of near-midpoint elements and the rows (..., N) with an eligible block."""
    k = r["idx"].shape[-1] if "idx" in r else 0
    T, D = r["attn"].shape[-1], v.shape[-1]
    _, chain = GS.n_add_and_chain(GS.finish_kernel_of(T, D, k), T, k)
    attn, true = r["attn"].astype(np.float64), r["true"].astype(np.float64)
    kept = O.prune_mask(r["idx"], T) if k else np.ones(attn.shape, bool)
    with np.errstate(invalid="ignore", over="ignore"):
        gap = np.where(kept, np.abs(true - np.max(np.where(kept, true, -np.inf), -1, keepdims=True)), 0.0)
        tau = (GS.TAU_C0 + (chain + GS.ref_chain(k or T)) / 2 + 2.0 * gap) * 2.0 ** -23
        bits = r["attn"].view(np.uint32)
        lo = (bits & np.uint32(0xFFFF0000)).view(F32).astype(np.float64)  # the bfloat16 value below p
        hi = ((bits & np.uint32(0xFFFF0000)) + np.uint32(0x10000)).view(F32).astype(np.float64)
        mid = (lo + hi) / 2
        near = kept & (attn > 0) & np.isfinite(attn) & (np.abs(attn - mid) <= tau * attn)
        a_lo = np.where(near, lo, O.quantize_bfloat(r["attn"], 16)).astype(F32)
        a_hi = np.where(near, hi, O.quantize_bfloat(r["attn"], 16)).astype(F32)
        _, c_lo, e_lo = O.quantize_mx(a_lo, "int4", 32, -1, flush=flush)
        _, c_hi, e_hi = O.quantize_mx(a_hi, "int4", 32, -1, flush=flush)
    changed = (c_lo != c_hi).any(-1) | (e_lo[..., 0] != e_hi[..., 0])
    crowded = O.to_blocks(near.astype(F32), -1, 32)[0].sum(-1) > 1
    return int((changed | crowded).sum()), int(near.sum()), (changed | crowded).any(-1)


# ---- exact-result cases at 4 bits (the construction of exact_out_cases.py) ----------------------
# q, k and the bias are exact_out_cases' (8.0 and 256 / width are MXINT4 values: code 4); V is
# integers |n| <= 7 times 2^e per (32-token block, column), so that V is its own MXINT4
_c = EC._c
EXACT = []
EXACT += [_c(EC.GATHER16, 1, 2, 20, T, D, k) for T in (70, 197) for D in (32, 72, 128) for k in (1, 20, 64)]
EXACT += [_c(EC.GATHER16, 1, 2, 20, T, D, k) for T, D, k in ((513, 32, 20), (513, 72, 64), (1000, 72, 20), (1000, 128, 64))]
EXACT += [_c(EC.MFMA, 1, 2, 70, 130, 64, 65), _c(EC.MFMA, 1, 2, 33, 256, 72, 154)]
EXACT += [_c(EC.DENSE_MFMA, 1, 2, 5, 20, 64, 0), _c(EC.DENSE_MFMA, 1, 2, 77, 120, 72, 0), _c(EC.DENSE_MFMA, 1, 2, 256, 256, 64, 0)]
EXACT += [_c(EC.GATHER16, 2, 2, 20, 197, 72, 20, True), _c(EC.GATHER16, 2, 2, 20, 1000, 72, 20, True),
          _c(EC.MFMA, 2, 2, 33, 256, 72, 65, True), _c(EC.DENSE_MFMA, 2, 2, 77, 120, 72, 0, True)]
EXACT += [_c(EC.GATHER16, 1, 2, 20, 197, 64, 20, approx=False), _c(EC.GATHER16, 1, 2, 20, 197, 64, 20, pred_mode="MXINT4")]
EXACT += [_c(EC.GATHER16, 1, 2, 20, 197, 64, 20, bfloat=16), _c(EC.MFMA, 1, 2, 77, 120, 72, 77, bfloat=16),
          _c(EC.GATHER16, 1, 2, 20, 513, 72, 20, bfloat=16)]


@functools.lru_cache(maxsize=None)
def exact_inputs(c):
    q, k, _, bias = EC.inputs(c)
    rng = np.random.default_rng([4, c.kind, c.N, c.T, c.D, c.k, int(c.bias)])
    n = rng.integers(-7, 8, (c.B, c.H, c.T, c.D)).astype(F32)
    e = rng.integers(0, 4, (c.B, c.H, (c.T + 31) // 32, c.D)).astype(F32)
    v = (n * np.exp2(np.repeat(e, 32, axis=2)[:, :, :c.T])).astype(F32)
    return q, k, v, bias


@functools.lru_cache(maxsize=None)
def exact_reference(c):
    q, k, v, bias = exact_inputs(c)
    return O.attention(q, k, v, EC.SCALE, bias=bias, elem="int4", **EC.oracle_kw(c))


# ---- the random GPU cases -----------------------------------------------------------------------
def pixart_bias(B, N, T, valid):
    """(1 - mask) * -10000 over the text tokens, (B, 1, 1, T)"""
    b = np.zeros((B, 1, 1, T), F32)
    b[..., valid:] = -10000.0
    return b


# k = 0: dense; mode None: approx=False; scores: the call also takes the true / approximate scores
RCase = collections.namedtuple("RCase", "N T D k mode scores bias flush bfloat seed")


def rcase_id(c):
    return (f"N{c.N}T{c.T}D{c.D}" + (f"k{c.k}" if c.k else "dense") + f"-{c.mode or 'trueK'}" +
            ("-scores" if c.scores else "") + ("-bias" if c.bias else "") + ("-flush" if c.flush else "") +
            (f"-bf{c.bfloat}" if c.bfloat != 32 else "") + f"-s{c.seed}")


def _r(N, T, D, k, mode="ex_pred", scores=False, bias=False, flush=False, bfloat=32, seed=0):
    return RCase(N, T, D, k, mode, scores, bias, flush, bfloat, seed)


def _grid():
    out, i = [], 0
    seven = MODES + (None,)
    for D in (32, 64, 72, 128):
        for N, T, bias in ((70, 70, False), (33, 197, False), (40, 120, True)):
            for k in (1, 7, 20, 64):
                # the modes thinned over the grid: each of the seven with every D, shape and k class
                out.append(_r(N, T, D, k, seven[i % 7], scores=(i // 7) % 2 == 0, bias=bias, flush=bias, seed=i))
                i += 1
    return out


GRID = _grid()
LONG = [_r(33, T, D, k, mode, scores=(j % 2 == 0), seed=100 + j)
        for j, (T, D, k, mode) in enumerate((T, D, k, m) for T in (513, 1000) for D in (32, 72) for k in (20, 64)
                                            for m in ("ex_pred", "MXINT4"))]
QK = [_r(70, 130, 64, 65, "ex_pred", True, seed=200), _r(70, 130, 72, 65, "true_ex", seed=201),
      _r(33, 256, 64, 154, "MXINT4", seed=202), _r(33, 256, 72, 154, "ex_pred", True, seed=203),
      _r(5, 20, 64, 0, seed=204), _r(5, 20, 72, 0, scores=True, seed=205), _r(77, 120, 64, 0, seed=206),
      _r(77, 120, 72, 0, scores=True, bias=True, flush=True, seed=207), _r(256, 256, 64, 0, seed=208),
      _r(256, 256, 72, 0, seed=209)]
# one random bfloat = 16 case whose eligible set is empty (asserted on the CPU): by the norm
BF16 = _r(40, 120, 72, 20, "ex_pred", True, bias=True, flush=True, bfloat=16, seed=300)
ROWS_CASES = GRID + LONG + QK


@functools.lru_cache(maxsize=None)
def r_inputs(c):
    """q, k, v as strided views of one packed (B, N, 3, H, D) qkv where N == T, bias or None"""
    B, H = 1, 2
    if c.N == c.T:
        qkv = rnd((B, c.N, 3, H, c.D), c.seed)
        q, k, v = (qkv[:, :, j].transpose(0, 2, 1, 3) for j in range(3))
    else:
        q, k, v = rnd((B, H, c.N, c.D), c.seed), rnd((B, H, c.T, c.D), c.seed + 1000), rnd((B, H, c.T, c.D), c.seed + 2000)
    bias = pixart_bias(B, c.N, c.T, c.T // 2) if c.bias else None
    return q, k, v, bias


@functools.lru_cache(maxsize=None)
def r_reference(c):
    q, k, v, bias = r_inputs(c)
    return O.attention(q, k, v, r_scale(c), bias=bias, flush=c.flush, bfloat=c.bfloat, elem="int4", **r_kw(c))


# ---- special blocks: NaN, +-Inf, all-zero and 2^+-100 blocks in Q, K and V ------------------------
SPECIAL_K, SPECIAL_SCALE = 7, 0.125


@functools.lru_cache(maxsize=None)
def special_inputs():
    q, k, v = rnd((1, 2, 40, 72), 400), rnd((1, 2, 70, 72), 401), rnd((1, 2, 70, 72), 402)
    q[0, 0, 3, 5], q[0, 1, 5, 40], k[0, 1, 6, 70] = np.nan, np.inf, -np.inf
    q[0, 0, 7, :] = 0.0
    q[0, 1, :, ::5] = 0.0  # zero elements, and the negative ones that round to the int4 code 0 elsewhere
    # (whole rows: a dot product whose blocks lie 2^100 apart leaves the range in which the oracle's
    # float64 sum of the approximate scores is exact)
    q[0, 0, 9, :] *= F32(2.0 ** 100)
    q[0, 0, 11, :] *= F32(2.0 ** -100)
    q[0, 0, 13, :] *= F32(2.0 ** -120)  # (head 0: true_ex maps the zero elements of head 1 to +1, 2^120 above)
    k[0, 0, 2, :] = 0.0
    k[0, 0, 4, :] *= F32(2.0 ** -100)
    k[0, 1, 8, :] *= F32(2.0 ** 90)
    v[0, 1, 33, 5] = np.nan  # (head 1: a NaN or Inf V block makes its output column NaN in every row)
    v[0, 1, 2, 7] = -np.inf
    v[0, 0, 32:64, 9] = 0.0
    v[0, 0, 0:32, 11] *= F32(2.0 ** 100)
    v[0, 1, 64:, 13] *= F32(2.0 ** -100)
    return q, k, v


@functools.lru_cache(maxsize=None)
def special_reference(mode):
    q, k, v = special_inputs()
    return O.attention(q, k, v, SPECIAL_SCALE, SPECIAL_K, mode, elem="int4")

