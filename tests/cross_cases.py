"""Inputs and the oracle chain of the fused-block tests (tests/test_cross_cpu.py,
tests/test_proj4_cpu.py, tests/test_gpu_cross.py) at both widths: M.mx_cross_attention is PixArt's
MXCrossAttention.forward -- q = to_q(x), k = to_k(cond), v = to_v(cond) through mx.Linear,
heads split as the module splits them, then the masked top-k attention core; M.mx_qkv_attention
and mx_topk_attention_proj are the self-attention block's halves.  elem = "int4" is the
reference's PixArt configuration, w_elem_format = a_elem_format = "int4"
(workloads/PixArt/scripts/mx_inference.py:106-122).  Nothing here touches the device.

The reference is the oracle at `elem`: O.mx_linear for every Linear, the modules' head splits
(heads_q / heads_kv, O.qkv_split), O.attention for the core.  Exponents, the gate and the block
normalisation are those of tests/gate_cases.py.  The CPU file proves with the oracle alone that
each input sits in the regime its GPU test is about (the NaN rows, the accumulation path of
every (tile, head) of the spread case, the subnormal gate); the GPU file repeats nothing of that
and only compares."""
import collections
import functools

import numpy as np

import gate_cases as GC
from oracle import mx_oracle as O

F32 = np.float32
# (B, N, T, C, C_kv, H), k_top -- the smallest shapes that reach each code path
SHAPES = {
    "d48": ((3, 45, 70, 96, 160, 2), 20),      # D = 48: two 32-column blocks, D % 32 != 0, ragged N and T, T > N
    "d32": ((2, 40, 20, 64, 64, 2), 7),        # D = 32: one wave per Q workgroup, T < 32, N > T
    "d72": ((2, 33, 77, 144, 96, 2), 20),      # D = 72: PixArt's head width, C no multiple of 64
    "pixart": ((1, 256, 120, 1152, 1152, 16), 20),  # the PixArt-alpha block width
    # a Q pass of 64 threads whose 32 * (C / 16) = 320 code loads exceed 4 per thread (the loads where
    # they are used), while the KV pass preloads
    "d32w": ((1, 40, 33, 160, 160, 5), 7),
}
# self-attention: (B, N, C, H), k_top (0: dense)
SELF_SHAPES = {
    "d48": ((2, 45, 96, 2), 20),
    "d32": ((2, 40, 64, 2), 7),
    "d72": ((1, 70, 144, 2), 20),
    "d64k65": ((1, 130, 128, 2), 65),   # finish_qk_kernel behind the fused projection
    "d72dense": ((1, 77, 144, 2), 0),
}


def mask_bias(B, T):
    """PixArt's attention_mask bias (MX_pixart_transformer_2d.py:394-397): the second half of
    the text tokens masked, (B, 1, 1, T)."""
    return np.where(np.arange(T) < T // 2, 0.0, -10000.0).astype(F32)[None, None, None, :].repeat(B, 0)


def heads_q(q, H):
    """to_q's output (B, N, H*D) -> (B, H, N, D)"""
    B, N, HD = q.shape
    return np.ascontiguousarray(q.reshape(B, N, H, HD // H).transpose(0, 2, 1, 3))


def heads_kv(kv, H):
    """kv (B, T, 2*H*D) -> k, v (B, H, T, D): kv.reshape(B, T, 2, H, D)"""
    B, T, HD2 = kv.shape
    t = kv.reshape(B, T, 2, H, HD2 // (2 * H)).transpose(2, 0, 3, 1, 4)
    return np.ascontiguousarray(t[0]), np.ascontiguousarray(t[1])


def head_rows(W, H, parts, h):
    """the rows of head h's sub-matrices (groups s * H + h) of a (parts * H * D, C) weight"""
    D = W.shape[0] // (parts * H)
    return np.concatenate([W[(s * H + h) * D: (s * H + h + 1) * D] for s in range(parts)])


def _normal(rng):
    return lambda *s, sc=1.0: (rng.standard_normal(s, dtype=F32) * F32(sc)).astype(F32)


@functools.lru_cache(maxsize=None)
def case(name, nan_x=True):
    """x, cond, Wq, bq, Wkv, bkv, Wo, bo of a SHAPES entry (the module's inner_dim = query_dim = C);
    nan_x: a NaN in x[0, 3, 7] and a zero row in Wq (the oracle then has exactly H NaN output
    rows, test_cross_cpu)."""
    (B, N, T, C, Ckv, H), _ = SHAPES[name]
    f = _normal(np.random.default_rng(B * 1000 + N * 7 + T))
    x, cond = f(B, N, C), f(B, T, Ckv)
    Wq, bq = f(C, C, sc=0.05), f(C, sc=0.1)
    Wkv, bkv = f(2 * C, Ckv, sc=0.05), f(2 * C, sc=0.1)
    Wo, bo = f(C, C, sc=0.05), f(C, sc=0.1)
    if nan_x:
        x[0, 3, 7] = np.nan
        Wq[5] = 0.0
    return x, cond, Wq, bq, Wkv, bkv, Wo, bo


@functools.lru_cache(maxsize=None)
def chain(name, mode="MXINT4", flush=False, bfloat=0, with_bias=True, top_k=True, nan_x=True, elem="int8"):
    """The oracle chain of a case: the two exact Linears, the module's head split, the
    attention core.  {q, kv, qh, kh, vh, bias, r}; computed once per parameter set and shared."""
    (B, N, T, C, Ckv, H), k_top = SHAPES[name]
    x, cond, Wq, bq, Wkv, bkv, _, _ = case(name, nan_x)
    kw = dict(elem=elem, flush=flush, bfloat=bfloat or 32)
    q, kv = O.mx_linear(x, Wq, bq, **kw), O.mx_linear(cond, Wkv, bkv, **kw)
    qh = heads_q(q, H)
    kh, vh = heads_kv(kv, H)
    bias = mask_bias(B, T) if with_bias else None
    r = O.attention(qh, kh, vh, (C // H) ** -0.5, k_top=k_top, pred_mode=mode, top_k=top_k, bias=bias, **kw)
    return dict(q=q, kv=kv, qh=qh, kh=kh, vh=vh, bias=bias, r=r)


@functools.lru_cache(maxsize=None)
def self_case(name):
    """x, Wqkv, bqkv, Wo, bo of a SELF_SHAPES entry (finite: a NaN token is a NaN key of every row)"""
    (B, N, C, H), _ = SELF_SHAPES[name]
    f = _normal(np.random.default_rng(9000 + B * 100 + N * 7 + C))
    return f(B, N, C), f(3 * C, C, sc=0.05), f(3 * C, sc=0.1), f(C, C, sc=0.05), f(C, sc=0.1)


@functools.lru_cache(maxsize=None)
def self_chain(name, mode="ex_pred", flush=False, bfloat=0, elem="int8"):
    """{qkv, qh, kh, vh, r} of a self-attention case: the qkv Linear, O.qkv_split, the attention core"""
    (B, N, C, H), k = SELF_SHAPES[name]
    x, W, b, _, _ = self_case(name)
    kw = dict(elem=elem, flush=flush, bfloat=bfloat or 32)
    qkv = O.mx_linear(x, W, b, **kw)
    qh, kh, vh = (np.ascontiguousarray(t) for t in O.qkv_split(qkv, H))
    r = O.attention(qh, kh, vh, (C // H) ** -0.5, **(dict(k_top=k, pred_mode=mode) if k else dict(top_k=False)), **kw)
    return dict(qkv=qkv, qh=qh, kh=kh, vh=vh, r=r)


# ---------------------------------------------------------------- the accumulation paths
SPREAD_SHAPE = (2, 70, 70, 256, 256)  # (B, N, T, C, C_kv); H = 4 and 2
# Per width, against its digit limit (GC.SPREAD: 8 / 4).  tiles: per 32-token tile the shifts of its
# rows' odd blocks, so a tile's largest row spread is its largest shift -- the digit limit, 20, and one
# above the limit; q_shift / k_shift: head 0's q columns and one head's k columns (odd blocks); the
# generators' seeds (+ H) of spread_case, spread_case_qkv (no 8-bit test draws one) and subnormal_case
Spread = collections.namedtuple("Spread", "tiles q_shift k_shift seed seed_qkv seed_sub")
SPREAD = {
    "int8": Spread({0: (0, 3, 8), 1: (12, 16, 20), 2: (9,)}, 10, 8, 31, None, 47),
    "int4": Spread({0: (0, 2, 4), 1: (12, 16, 20), 2: (5,)}, 10, 4, 131, 231, 147),
}


def spread_tokens(rng, B, N, C, elem):
    """(B, N, C) tokens with every 32-channel block normalised to one exponent, then the odd
    blocks of each row scaled by 2^s, s from the row's tile (SPREAD[elem].tiles, five rows per
    value): a tile's largest row spread is then exactly its largest shift."""
    x = GC.blocks_to_unit(rng.standard_normal((B, N, C), dtype=F32))
    odd = (np.arange(C) // 32) % 2 == 1
    for t in range(N):
        sh = SPREAD[elem].tiles[t // 32]
        x[:, t, odd] *= F32(2.0 ** sh[(t // 5) % len(sh)])
    return x


def _unit_weight(rng, out_f, in_f):
    return (GC.blocks_to_unit(rng.standard_normal((out_f, in_f), dtype=F32)) * F32(2.0 ** -5)).astype(F32)


@functools.lru_cache(maxsize=None)
def spread_case(H, elem="int8"):
    """x, cond, Wq, bq, Wkv, bkv: x and cond from spread_tokens; both weights with every 32-block
    normalised (column spreads 0), then head 0's q columns times 2^q_shift and a head's k columns
    times 2^k_shift on the odd blocks (column spreads exactly those).  With smax = 9 (eight
    K-blocks) every (tile, head) has its path by construction: spread_paths() restates the
    kernel's decision and test_cross_cpu asserts all three occur in every pass."""
    B, N, T, C, Ckv = SPREAD_SHAPE
    D, sp = C // H, SPREAD[elem]
    rng = np.random.default_rng(sp.seed + H)
    x, cond = spread_tokens(rng, B, N, C, elem), spread_tokens(rng, B, T, Ckv, elem)
    Wq, Wkv = _unit_weight(rng, C, C), _unit_weight(rng, 2 * C, Ckv)
    bq, bkv = _normal(rng)(C, sc=0.1), _normal(rng)(2 * C, sc=0.1)
    oddq, oddk = (np.arange(C) // 32) % 2 == 1, (np.arange(Ckv) // 32) % 2 == 1
    Wq[0:D][:, oddq] *= F32(2.0 ** sp.q_shift)          # head 0's q columns
    hk = min(1, H - 1)
    Wkv[hk * D: hk * D + D][:, oddk] *= F32(2.0 ** sp.k_shift)  # head hk's k columns
    return x, cond, Wq, bq, Wkv, bkv


@functools.lru_cache(maxsize=None)
def spread_case_qkv(H, elem):
    """the same for a (3C, C) qkv weight: x, W, b; head 0's q columns and head hk's k columns scaled"""
    B, N, _, C, _ = SPREAD_SHAPE
    D, sp = C // H, SPREAD[elem]
    rng = np.random.default_rng(sp.seed_qkv + H)
    x = spread_tokens(rng, B, N, C, elem)
    W = _unit_weight(rng, 3 * C, C)
    b = _normal(rng)(3 * C, sc=0.1)
    odd = (np.arange(C) // 32) % 2 == 1
    W[0:D][:, odd] *= F32(2.0 ** sp.q_shift)
    hk = min(1, H - 1)
    W[C + hk * D: C + hk * D + D][:, odd] *= F32(2.0 ** sp.k_shift)
    return x, W, b


def proj_smax(nbk):
    """mxa_gemm.hip gemm_smax: the largest row + column spread whose shifted int32 block sums
    cannot overflow, nbk * 32 * 127^2 * 2^smax < 2^31"""
    s = -1
    while nbk * 516128 * 2 ** (s + 1) < 2 ** 31:
        s += 1
    return s


def spread_paths(tokens, W, H, parts, elem):
    """The projection kernel's accumulation path of every (image, tile, head) -- mxa_proj.hpp,
    one head per workgroup (a grid of B * 3 * H workgroups is less than one round of resident
    ones, so launch_proj's cost model takes one head per group): "digit" when the tile's
    largest row spread and the head's largest column spread are both within the width's digit
    limit, else "int32" when they sum to <= smax, else "fp64".  The gate quantity (tile min +
    head min, GC.gemm_gate) must be >= -126 everywhere for this to be the whole decision;
    asserted here."""
    B, N, C = tokens.shape
    smax, limit = proj_smax((C + 31) // 32), GC.SPREAD[elem]
    paths = {}
    for h in range(H):
        Wh = head_rows(W, H, parts, h)
        for b in range(B):
            q, smx, wsp = GC.gemm_gate(tokens[b], Wh, elem=elem)  # per 32-token tile
            assert (q >= GC.GATE).all(), q
            for tb in range(len(smx)):
                dig = smx[tb] <= limit and wsp <= limit
                paths[b, tb, h] = "digit" if dig else "int32" if smx[tb] + wsp <= smax else "fp64"
    return paths


# ---------------------------------------------------------------- the digit path's subnormal gate
def normalise_weight_blocks(W, elem):
    """W with the blocks of any row whose exponents spread more than the digit limit scaled up (by
    powers of two) to within the limit of the row's largest: a random weight then has the digit
    operands (at int8 these draws have them already and stay as they are)"""
    e = GC.unit_exps(W, elem)
    return GC.scaled(W, np.maximum(e.max(-1, keepdims=True) - GC.SPREAD[elem] - e, 0.0))


@functools.lru_cache(maxsize=None)
def subnormal_case(which, elem="int8"):
    """The "subnormal" regime of test_qkv_projection_digit_subnormal_gate on one of the two
    passes: which = "q" (H = 4; x and Wq times 2^-70, a bias of the results' magnitude) or "kv"
    (H = 2; cond and Wkv times 2^-70, no bias).  The first 32-token tile of the scaled source
    has row spreads within the digit limit and so have the weights' columns: the digit operands,
    behind a gate that fires for every head (test_cross_cpu asserts both)."""
    B, N, T, C, Ckv = SPREAD_SHAPE
    H = 4 if which == "q" else 2
    rng = np.random.default_rng(SPREAD[elem].seed_sub + H)
    x, cond = spread_tokens(rng, B, N, C, elem), spread_tokens(rng, B, T, Ckv, elem)
    Wq = normalise_weight_blocks(_normal(rng)(C, C, sc=0.05), elem)
    Wkv = normalise_weight_blocks(_normal(rng)(2 * C, Ckv, sc=0.05), elem)
    bq = bkv = None
    s = GC.pow2(-70)
    if which == "q":
        x, Wq = (x * s).astype(F32), (Wq * s).astype(F32)
        want = O.mx_linear(x, Wq, elem=elem)
        mag = np.abs(want[:, :32][want[:, :32] != 0]).astype(np.float64)
        bq = (rng.standard_normal(C) * np.exp2(np.floor(np.log2(np.median(mag))))).astype(F32)
    else:
        cond, Wkv = (cond * s).astype(F32), (Wkv * s).astype(F32)
    return H, x, cond, Wq, bq, Wkv, bkv


# ---------------------------------------------------------------- a NaN among the key / value tokens
@functools.lru_cache(maxsize=None)
def nan_cond_case(elem="int8"):
    """(3, 20, 40, 64, 64), H = 2, k = 7: a NaN in cond[1, 9, 40] -- key and value row 9 of image
    1 are NaN in every head.  H, x, cond, Wq, Wkv, q, kv, vh, r."""
    B, N, T, C, H = 3, 20, 40, 64, 2
    f = _normal(np.random.default_rng(5))
    x, cond, Wq, Wkv = f(B, N, C), f(B, T, C), f(C, C, sc=0.05), f(2 * C, C, sc=0.05)
    cond[1, 9, 40] = np.nan
    q, kv = O.mx_linear(x, Wq, elem=elem), O.mx_linear(cond, Wkv, elem=elem)
    kh, vh = heads_kv(kv, H)
    r = O.attention(heads_q(q, H), kh, vh, (C // H) ** -0.5, k_top=7, pred_mode="MXINT4", elem=elem)
    return H, x, cond, Wq, Wkv, q, kv, vh, r
