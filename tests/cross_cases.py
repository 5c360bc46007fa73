"""Inputs and the oracle chain of the cross-attention tests (tests/test_cross_cpu.py,
tests/test_gpu_cross.py): M.mx_cross_attention is PixArt's MXCrossAttention.forward --
q = to_q(x), k = to_k(cond), v = to_v(cond) through mx.Linear, heads split as the module
splits them, then the masked top-k attention core.

Exponents, the gate and the block normalisation are those of tests/gate_cases.py.  The CPU
file proves with the oracle alone that each input sits in the regime its GPU test is
about (the NaN rows, the accumulation path of every (tile, head) of the spread case, the
subnormal gate); the GPU file repeats nothing of that and only compares."""
import functools

import numpy as np

import gate_cases as GC
from oracle import mx_oracle as O

# (B, N, T, C, C_kv, H), k_top -- the smallest shapes that reach each code path
SHAPES = {
    "d48": ((3, 45, 70, 96, 160, 2), 20),      # D = 48: two 32-column blocks, D % 32 != 0, ragged N and T, T > N
    "d32": ((2, 40, 20, 64, 64, 2), 7),        # D = 32: one wave per Q workgroup, T < 32, N > T
    "d72": ((2, 33, 77, 144, 96, 2), 20),      # D = 72: PixArt's head width, C no multiple of 64
    "pixart": ((1, 256, 120, 1152, 1152, 16), 20),  # the PixArt-alpha block width
}


def mask_bias(B, T):
    """PixArt's attention_mask bias (MX_pixart_transformer_2d.py:394-397): the second half of
    the text tokens masked, (B, 1, 1, T)."""
    return np.where(np.arange(T) < T // 2, 0.0, -10000.0).astype(np.float32)[None, None, None, :].repeat(B, 0)


def heads_q(q, H):
    """to_q's output (B, N, H*D) -> (B, H, N, D)"""
    B, N, HD = q.shape
    return np.ascontiguousarray(q.reshape(B, N, H, HD // H).transpose(0, 2, 1, 3))


def heads_kv(kv, H):
    """kv (B, T, 2*H*D) -> k, v (B, H, T, D): kv.reshape(B, T, 2, H, D)"""
    B, T, HD2 = kv.shape
    t = kv.reshape(B, T, 2, H, HD2 // (2 * H)).transpose(2, 0, 3, 1, 4)
    return np.ascontiguousarray(t[0]), np.ascontiguousarray(t[1])


@functools.lru_cache(maxsize=None)
def case(name, nan_x=True):
    """x, cond, Wq, bq, Wkv, bkv, Wo, bo of a SHAPES entry; nan_x: a NaN in x[0, 3, 7] and a
    zero row in Wq (the oracle then has exactly H NaN output rows, test_cross_cpu)."""
    (B, N, T, C, Ckv, H), _ = SHAPES[name]
    HD = C  # the module's inner_dim = query_dim
    rng = np.random.default_rng(B * 1000 + N * 7 + T)
    f = lambda *s, sc=1.0: (rng.standard_normal(s, dtype=np.float32) * np.float32(sc)).astype(np.float32)  # noqa: E731
    x, cond = f(B, N, C), f(B, T, Ckv)
    Wq, bq = f(HD, C, sc=0.05), f(HD, sc=0.1)
    Wkv, bkv = f(2 * HD, Ckv, sc=0.05), f(2 * HD, sc=0.1)
    Wo, bo = f(C, HD, sc=0.05), f(C, sc=0.1)
    if nan_x:
        x[0, 3, 7] = np.nan
        Wq[5] = 0.0
    return x, cond, Wq, bq, Wkv, bkv, Wo, bo


@functools.lru_cache(maxsize=None)
def chain(name, mode="MXINT4", flush=False, bfloat=0, with_bias=True, top_k=True, nan_x=True):
    """The oracle chain of a case: the two exact Linears, the module's head split, the
    attention core.  {q, kv, qh, kh, vh, bias, r}; computed once per parameter set and shared."""
    (B, N, T, C, Ckv, H), k_top = SHAPES[name]
    x, cond, Wq, bq, Wkv, bkv, _, _ = case(name, nan_x)
    bf = bfloat or 32
    q = O.mx_linear(x, Wq, bq, flush=flush, bfloat=bf)
    kv = O.mx_linear(cond, Wkv, bkv, flush=flush, bfloat=bf)
    qh = heads_q(q, H)
    kh, vh = heads_kv(kv, H)
    D = C // H
    bias = mask_bias(B, T) if with_bias else None
    r = O.attention(qh, kh, vh, D ** -0.5, k_top=k_top, pred_mode=mode, top_k=top_k, bias=bias, flush=flush, bfloat=bf)
    return dict(q=q, kv=kv, qh=qh, kh=kh, vh=vh, bias=bias, r=r)


# ---------------------------------------------------------------- the accumulation paths
SPREAD_SHAPE = (2, 70, 70, 256, 256)  # (B, N, T, C, C_kv); H = 4 and 2
TILE_SHIFTS = {0: (0, 3, 8), 1: (12, 16, 20), 2: (9,)}  # per 32-token tile: the shifts of its rows' odd blocks


def spread_tokens(rng, B, N, C):
    """(B, N, C) tokens with every 32-channel block normalised to one exponent, then the odd
    blocks of each row scaled by 2^s, s from the row's tile (TILE_SHIFTS, five rows per
    value): a tile's largest row spread is then exactly its largest shift -- 8 (the digit
    limit), 20 and 9."""
    x = GC.blocks_to_unit(rng.standard_normal((B, N, C), dtype=np.float32))
    odd = (np.arange(C) // 32) % 2 == 1
    for t in range(N):
        sh = TILE_SHIFTS[t // 32]
        x[:, t, odd] *= np.float32(2.0 ** sh[(t // 5) % len(sh)])
    return x


@functools.lru_cache(maxsize=None)
def spread_case(H):
    """test_qkv_projection_spread_paths for two token sources: x and cond from spread_tokens;
    both weights with every 32-block normalised (column spreads 0), then head 0's q columns
    times 2^10 and a head's k columns times 2^8 on the odd blocks (column spreads exactly 10
    and 8).  With smax = 9 (eight K-blocks) every (tile, head) has its path by construction:
    spread_paths() restates the kernel's decision and test_cross_cpu asserts all three occur
    in both passes."""
    B, N, T, C, Ckv = SPREAD_SHAPE
    D = C // H
    rng = np.random.default_rng(31 + H)
    x, cond = spread_tokens(rng, B, N, C), spread_tokens(rng, B, T, Ckv)
    Wq = (GC.blocks_to_unit(rng.standard_normal((C, C), dtype=np.float32)) * np.float32(2.0 ** -5)).astype(np.float32)
    Wkv = (GC.blocks_to_unit(rng.standard_normal((2 * C, Ckv), dtype=np.float32)) * np.float32(2.0 ** -5)).astype(np.float32)
    bq = (rng.standard_normal(C, dtype=np.float32) * np.float32(0.1)).astype(np.float32)
    bkv = (rng.standard_normal(2 * C, dtype=np.float32) * np.float32(0.1)).astype(np.float32)
    oddq, oddk = (np.arange(C) // 32) % 2 == 1, (np.arange(Ckv) // 32) % 2 == 1
    Wq[0:D][:, oddq] *= np.float32(2.0 ** 10)          # head 0's q columns
    hk = min(1, H - 1)
    Wkv[hk * D: hk * D + D][:, oddk] *= np.float32(2.0 ** 8)  # head hk's k columns
    return x, cond, Wq, bq, Wkv, bkv


def proj_smax(nbk):
    """mxa_gemm.hip gemm_smax: the largest row + column spread whose shifted int32 block sums
    cannot overflow, nbk * 32 * 127^2 * 2^smax < 2^31"""
    s = -1
    while nbk * 516128 * 2 ** (s + 1) < 2 ** 31:
        s += 1
    return s


def spread_paths(tokens, W, H, parts):
    """The projection kernel's accumulation path of every (image, tile, head) -- mxa_proj.hpp,
    one head per workgroup (a grid of B * 3 * H workgroups is less than one round of resident
    ones, so launch_proj's cost model takes one head per group): "digit" when the tile's
    largest row spread and the head's largest column spread are both <= 8, else "int32" when
    they sum to <= smax, else "fp64".  The gate quantity (tile min + head min, GC.gemm_gate)
    must be >= -126 everywhere for this to be the whole decision; asserted here."""
    B, N, C = tokens.shape
    D = W.shape[0] // (parts * H)
    smax = proj_smax((C + 31) // 32)
    paths = {}
    for h in range(H):
        Wh = np.concatenate([W[(s * H + h) * D: (s * H + h + 1) * D] for s in range(parts)])
        for b in range(B):
            q, smx, wsp = GC.gemm_gate(tokens[b], Wh)  # per 32-token tile
            assert (q >= GC.GATE).all(), q
            for tb in range(len(smx)):
                dig = smx[tb] <= GC.DIGIT_SPREAD and wsp <= GC.DIGIT_SPREAD
                paths[b, tb, h] = "digit" if dig else "int32" if smx[tb] + wsp <= smax else "fp64"
    return paths


# ---------------------------------------------------------------- the digit path's subnormal gate
@functools.lru_cache(maxsize=None)
def subnormal_case(which):
    """The "subnormal" regime of test_qkv_projection_digit_subnormal_gate on one of the two
    passes: which = "q" (H = 4; x and Wq times 2^-70, a bias of the results' magnitude) or "kv"
    (H = 2; cond and Wkv times 2^-70, no bias).  The first 32-token tile of the scaled source
    has row spreads <= 8 and the scaled weight column spreads <= 8: the digit operands, behind
    a gate that fires for every head (test_cross_cpu asserts both)."""
    B, N, T, C, Ckv = SPREAD_SHAPE
    H = 4 if which == "q" else 2
    rng = np.random.default_rng(47 + H)
    x, cond = spread_tokens(rng, B, N, C), spread_tokens(rng, B, T, Ckv)
    Wq = (rng.standard_normal((C, C), dtype=np.float32) * np.float32(0.05)).astype(np.float32)
    Wkv = (rng.standard_normal((2 * C, Ckv), dtype=np.float32) * np.float32(0.05)).astype(np.float32)
    bq = bkv = None
    s = GC.pow2(-70)
    if which == "q":
        x, Wq = (x * s).astype(np.float32), (Wq * s).astype(np.float32)
        want = O.mx_linear(x, Wq)
        mag = np.abs(want[:, :32][want[:, :32] != 0]).astype(np.float64)
        bq = (rng.standard_normal(C) * np.exp2(np.floor(np.log2(np.median(mag))))).astype(np.float32)
    else:
        cond, Wkv = (cond * s).astype(np.float32), (Wkv * s).astype(np.float32)
    return H, x, cond, Wq, bq, Wkv, bkv


# ---------------------------------------------------------------- a NaN among the key / value tokens
@functools.lru_cache(maxsize=None)
def nan_cond_case():
    """(3, 20, 40, 64, 64), H = 2, k = 7: a NaN in cond[1, 9, 40] -- key and value row 9 of image
    1 are NaN in every head."""
    B, N, T, C, H = 3, 20, 40, 64, 2
    rng = np.random.default_rng(5)
    x, cond = rng.standard_normal((B, N, C), dtype=np.float32), rng.standard_normal((B, T, C), dtype=np.float32)
    Wq = (rng.standard_normal((C, C), dtype=np.float32) * np.float32(0.05)).astype(np.float32)
    Wkv = (rng.standard_normal((2 * C, C), dtype=np.float32) * np.float32(0.05)).astype(np.float32)
    cond[1, 9, 40] = np.nan
    q, kv = O.mx_linear(x, Wq), O.mx_linear(cond, Wkv)
    kh, vh = heads_kv(kv, H)
    r = O.attention(heads_q(q, H), kh, vh, (C // H) ** -0.5, k_top=7, pred_mode="MXINT4")
    return H, x, cond, Wq, Wkv, q, kv, r
