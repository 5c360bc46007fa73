"""Inputs and the oracle chain of the W4A4 fused-block tests (tests/test_proj4_cpu.py,
tests/test_gpu_proj4.py): M.mx_cross_attention / mx_qkv_attention / mx_topk_attention_proj with
elem_bits=4 -- the reference's PixArt configuration, w_elem_format = a_elem_format = "int4"
(workloads/PixArt/scripts/mx_inference.py:106-122).  Nothing here touches the device.

The reference is the oracle at elem="int4": O.mx_linear for every Linear, the modules' head
splits (cross_cases.heads_q / heads_kv, O.qkv_split), attn4_cases.attention4 for the core.  The
cross inputs are cross_cases.case's; the accumulation-path cases are cross_cases' constructions
restated against the one-digit gate (gate_cases at elem="int4": spreads <= 4)."""
import functools

import numpy as np

import attn4_cases as A4
import cross_cases as CC
import gate_cases as GC
from oracle import mx_oracle as O

F32 = np.float32
MODES = ("ex_pred", "MXINT4", "two_step_leading_ones")
# (B, N, T, C, C_kv, H), k_top -- beside cross_cases.SHAPES: a Q pass of 64 threads whose 32 * (C / 16) =
# 320 code loads exceed 4 per thread (the loads where they are used), while the KV pass preloads
SHAPES = dict(CC.SHAPES, d32w=((1, 40, 33, 160, 160, 5), 7))
# self-attention: (B, N, C, H), k_top (0: dense)
SELF_SHAPES = {
    "d48": ((2, 45, 96, 2), 20),
    "d32": ((2, 40, 64, 2), 7),
    "d72": ((1, 70, 144, 2), 20),
    "d64k65": ((1, 130, 128, 2), 65),   # finish_qk_kernel behind the fused projection
    "d72dense": ((1, 77, 144, 2), 0),
}


def case(name, nan_x=True):
    """cross_cases.case for its shapes; the same construction for the ones added here"""
    if name in CC.SHAPES:
        return CC.case(name, nan_x)
    return _case(name, nan_x)


@functools.lru_cache(maxsize=None)
def _case(name, nan_x):
    (B, N, T, C, Ckv, H), _ = SHAPES[name]
    rng = np.random.default_rng(B * 1000 + N * 7 + T)
    f = lambda *s, sc=1.0: (rng.standard_normal(s, dtype=F32) * F32(sc)).astype(F32)  # noqa: E731
    x, cond = f(B, N, C), f(B, T, Ckv)
    Wq, bq = f(C, C, sc=0.05), f(C, sc=0.1)
    Wkv, bkv = f(2 * C, Ckv, sc=0.05), f(2 * C, sc=0.1)
    Wo, bo = f(C, C, sc=0.05), f(C, sc=0.1)
    if nan_x:
        x[0, 3, 7] = np.nan
        Wq[5] = 0.0
    return x, cond, Wq, bq, Wkv, bkv, Wo, bo


def lin4(x, W, b=None, flush=False, bfloat=0):
    return O.mx_linear(x, W, b, elem="int4", flush=flush, bfloat=bfloat or 32)


@functools.lru_cache(maxsize=None)
def chain(name, mode="MXINT4", flush=False, bfloat=0, with_bias=True, top_k=True):
    """cross_cases.chain at int4: {q, kv, qh, kh, vh, bias, r}, computed once per parameter set"""
    (B, N, T, C, Ckv, H), k_top = SHAPES[name]
    x, cond, Wq, bq, Wkv, bkv, _, _ = case(name)
    q, kv = lin4(x, Wq, bq, flush, bfloat), lin4(cond, Wkv, bkv, flush, bfloat)
    qh = CC.heads_q(q, H)
    kh, vh = CC.heads_kv(kv, H)
    bias = CC.mask_bias(B, T) if with_bias else None
    r = A4.attention4(qh, kh, vh, (C // H) ** -0.5, k_top=k_top, pred_mode=mode, top_k=top_k, bias=bias, flush=flush,
                      bfloat=bfloat or 32)
    return dict(q=q, kv=kv, qh=qh, kh=kh, vh=vh, bias=bias, r=r)


@functools.lru_cache(maxsize=None)
def self_case(name):
    """x, Wqkv, bqkv, Wo, bo of a SELF_SHAPES entry (finite: a NaN token is a NaN key of every row)"""
    (B, N, C, H), _ = SELF_SHAPES[name]
    rng = np.random.default_rng(9000 + B * 100 + N * 7 + C)
    f = lambda *s, sc=1.0: (rng.standard_normal(s, dtype=F32) * F32(sc)).astype(F32)  # noqa: E731
    return f(B, N, C), f(3 * C, C, sc=0.05), f(3 * C, sc=0.1), f(C, C, sc=0.05), f(C, sc=0.1)


@functools.lru_cache(maxsize=None)
def self_chain(name, mode="ex_pred", flush=False, bfloat=0):
    (B, N, C, H), k = SELF_SHAPES[name]
    x, W, b, _, _ = self_case(name)
    qkv = lin4(x, W, b, flush, bfloat)
    qh, kh, vh = (np.ascontiguousarray(t) for t in O.qkv_split(qkv, H))
    kw = dict(k_top=k, pred_mode=mode) if k else dict(top_k=False)
    r = A4.attention4(qh, kh, vh, (C // H) ** -0.5, flush=flush, bfloat=bfloat or 32, **kw)
    return dict(qkv=qkv, qh=qh, kh=kh, vh=vh, r=r)


# ---------------------------------------------------------------- the accumulation paths at one digit
SPREAD_SHAPE = CC.SPREAD_SHAPE  # (2, 70, 70, 256, 256); H = 4 and 2
TILE_SHIFTS = {0: (0, 2, 4), 1: (12, 16, 20), 2: (5,)}  # a tile's largest row spread: 4 (the digit limit), 20, 5
Q_SHIFT, K_SHIFT = 10, 4  # head 0's q columns, one head's k columns (odd blocks)


def spread_tokens(rng, B, N, C):
    """cross_cases.spread_tokens with TILE_SHIFTS above"""
    x = GC.blocks_to_unit(rng.standard_normal((B, N, C), dtype=F32))
    odd = (np.arange(C) // 32) % 2 == 1
    for t in range(N):
        sh = TILE_SHIFTS[t // 32]
        x[:, t, odd] *= F32(2.0 ** sh[(t // 5) % len(sh)])
    return x


def _unit_weight(rng, out_f, in_f):
    return (GC.blocks_to_unit(rng.standard_normal((out_f, in_f), dtype=F32)) * F32(2.0 ** -5)).astype(F32)


@functools.lru_cache(maxsize=None)
def spread_case(H):
    """cross_cases.spread_case's construction against the one-digit gate: x, cond, Wq, bq, Wkv, bkv"""
    B, N, T, C, Ckv = SPREAD_SHAPE
    D = C // H
    rng = np.random.default_rng(131 + H)
    x, cond = spread_tokens(rng, B, N, C), spread_tokens(rng, B, T, Ckv)
    Wq, Wkv = _unit_weight(rng, C, C), _unit_weight(rng, 2 * C, Ckv)
    bq = (rng.standard_normal(C, dtype=F32) * F32(0.1)).astype(F32)
    bkv = (rng.standard_normal(2 * C, dtype=F32) * F32(0.1)).astype(F32)
    oddq, oddk = (np.arange(C) // 32) % 2 == 1, (np.arange(Ckv) // 32) % 2 == 1
    Wq[0:D][:, oddq] *= F32(2.0 ** Q_SHIFT)
    hk = min(1, H - 1)
    Wkv[hk * D: hk * D + D][:, oddk] *= F32(2.0 ** K_SHIFT)
    return x, cond, Wq, bq, Wkv, bkv


@functools.lru_cache(maxsize=None)
def spread_case_qkv(H):
    """the same for a (3C, C) qkv weight: head 0's q columns times 2^10, head 1's k columns times 2^4"""
    B, N, _, C, _ = SPREAD_SHAPE
    D = C // H
    rng = np.random.default_rng(231 + H)
    x = spread_tokens(rng, B, N, C)
    W = _unit_weight(rng, 3 * C, C)
    b = (rng.standard_normal(3 * C, dtype=F32) * F32(0.1)).astype(F32)
    odd = (np.arange(C) // 32) % 2 == 1
    W[0:D][:, odd] *= F32(2.0 ** Q_SHIFT)
    hk = min(1, H - 1)
    W[C + hk * D: C + hk * D + D][:, odd] *= F32(2.0 ** K_SHIFT)
    return x, W, b


def head_rows(W, H, parts, h):
    """the rows of head h's sub-matrices (groups s * H + h) of a (parts * H * D, C) weight"""
    D = W.shape[0] // (parts * H)
    return np.concatenate([W[(s * H + h) * D: (s * H + h + 1) * D] for s in range(parts)])


def spread_paths(tokens, W, H, parts):
    """cross_cases.spread_paths at width 4 (mxa_proj.hpp proj_block, MB 4): "digit" when the tile's
    largest row spread and the head's largest column spread are both <= 4, else "int32" when they
    sum to <= smax, else "fp64"; the gate quantity >= -126 everywhere, asserted."""
    B, N, C = tokens.shape
    smax = CC.proj_smax((C + 31) // 32)
    paths = {}
    for h in range(H):
        Wh = head_rows(W, H, parts, h)
        for b in range(B):
            q, smx, wsp = GC.gemm_gate(tokens[b], Wh, elem="int4")
            assert (q >= GC.GATE).all(), q
            for tb in range(len(smx)):
                dig = smx[tb] <= GC.DIGIT4_SPREAD and wsp <= GC.DIGIT4_SPREAD
                paths[b, tb, h] = "digit" if dig else "int32" if smx[tb] + wsp <= smax else "fp64"
    return paths


def normalise_weight_blocks(W, limit=GC.DIGIT4_SPREAD):
    """W with the blocks of any row whose MXINT4 exponents spread more than limit scaled up (by powers of
    two) to within limit of the row's largest: a random weight then has the digit operands"""
    e = GC.unit_exps(W, "int4")
    up = np.maximum(e.max(-1, keepdims=True) - limit - e, 0.0)
    return GC.scaled(W, up)


@functools.lru_cache(maxsize=None)
def subnormal_case(which):
    """cross_cases.subnormal_case's construction at width 4: which = "q" (H = 4; x and Wq times 2^-70, a
    bias of the results' magnitude) or "kv" (H = 2; cond and Wkv times 2^-70).  The first tile of the
    scaled source has row spreads <= 4; the weights' blocks are normalised to column spreads <= 4."""
    B, N, T, C, Ckv = SPREAD_SHAPE
    H = 4 if which == "q" else 2
    rng = np.random.default_rng(147 + H)
    x, cond = spread_tokens(rng, B, N, C), spread_tokens(rng, B, T, Ckv)
    Wq = normalise_weight_blocks((rng.standard_normal((C, C), dtype=F32) * F32(0.05)).astype(F32))
    Wkv = normalise_weight_blocks((rng.standard_normal((2 * C, Ckv), dtype=F32) * F32(0.05)).astype(F32))
    bq = bkv = None
    s = GC.pow2(-70)
    if which == "q":
        x, Wq = (x * s).astype(F32), (Wq * s).astype(F32)
        want = lin4(x, Wq)
        mag = np.abs(want[:, :32][want[:, :32] != 0]).astype(np.float64)
        bq = (rng.standard_normal(C) * np.exp2(np.floor(np.log2(np.median(mag))))).astype(F32)
    else:
        cond, Wkv = (cond * s).astype(F32), (Wkv * s).astype(F32)
    return H, x, cond, Wq, bq, Wkv, bkv


@functools.lru_cache(maxsize=None)
def nan_cond_case():
    """cross_cases.nan_cond_case's construction at width 4"""
    B, N, T, C, H = 3, 20, 40, 64, 2
    rng = np.random.default_rng(5)
    x, cond = rng.standard_normal((B, N, C), dtype=F32), rng.standard_normal((B, T, C), dtype=F32)
    Wq = (rng.standard_normal((C, C), dtype=F32) * F32(0.05)).astype(F32)
    Wkv = (rng.standard_normal((2 * C, C), dtype=F32) * F32(0.05)).astype(F32)
    cond[1, 9, 40] = np.nan
    q, kv = lin4(x, Wq), lin4(cond, Wkv)
    kh, vh = CC.heads_kv(kv, H)
    r = A4.attention4(CC.heads_q(q, H), kh, vh, (C // H) ** -0.5, k_top=7, pred_mode="MXINT4")
    return H, x, cond, Wq, Wkv, q, kv, vh, r
