"""The CPU model of the digit kernels' gate (mxa_gemm.hpp mx_gemm_dig_kernel / mx_gemm_dig4_kernel,
mxa_mlp.hpp's fused fc1 kernels, mxa_proj.hpp qkv_proj_kernel) and the block construction of
the inputs built against it: the gates' quantities restated from the oracle's block exponents,
so that each test input provably sits in its regime.  The only statement of either; the
*_cases.py modules and the GPU tests build on it.

The device keeps a block's exponent as that of a code unit, e = es - 6 for MXINT8 (codes in
[-127, 127]) and es - 2 for MXINT4 (codes in [-7, 7]) (es: the oracle's shared exponent,
quantize_mx(...)[2]; value = code * 2^e).  Every block product is an integer times
2^(ex + ew), so a result is a multiple of 2^(min ex + min ew): normal (or zero) when that sum
is >= -126 -- the digit fast path's condition.  Below it the kernels sum the blocks in fp64
and round once to float32, subnormals included.

  the GEMM's digit kernels, per 32-row block:  min over its rows' blocks (NaN blocks and
      all-zero blocks left out) + min over every weight column's blocks    >= -126
  qkv_proj_kernel, per 32-token tile and head:  min over the tile's rows' blocks (NaN blocks
      left out) + min over the head's q, k, v weight columns' blocks       >= -126
and the digit operands exist when every row's and every weight column's spread (max - min)
is <= 8 for MXINT8 (kDigitSpread: two digits), <= 4 for MXINT4 (kDigit4Spread: 7 * 2^4 = 112
fits one signed int8 digit)."""
import warnings

import numpy as np

from oracle import mx_oracle as O

F32 = np.float32
GATE = -126          # the last value at which the gate does not fire
DIGIT_SPREAD = 8     # mxa_proj_args.hpp kDigitSpread
DIGIT4_SPREAD = 4    # mxa_proj_args.hpp kDigit4Spread
F32_MIN_NORMAL = np.float32(2.0 ** -126)
_UNIT = {"int8": 6.0, "int4": 2.0}                       # es - e per format
SPREAD = {"int8": DIGIT_SPREAD, "int4": DIGIT4_SPREAD}  # the digit operands' spread limit


def unit_exps(A, elem="int8", bfloat=32, flush=False):
    """(rows, nb) code-unit exponents of A's 32-blocks along its last axis as float64; NaN for
    a block that holds a NaN."""
    A = O.quantize_bfloat(np.asarray(A, F32), bfloat)
    return O.quantize_mx(A, elem, 32, -1, flush=flush)[2][..., 0].astype(np.float64) - _UNIT[elem]


def zero_blocks(A):
    A = np.asarray(A, F32)
    nb = (A.shape[-1] + 31) // 32
    P = np.zeros(A.shape[:-1] + (nb * 32,), F32)
    P[..., : A.shape[-1]] = A
    return (P.reshape(A.shape[:-1] + (nb, 32)) == 0).all(-1)


def row_stats(A, skip_zero_blocks, bfloat=32, elem="int8"):
    """per row: (min, spread) of the code-unit exponents (NaN: the row has no block left)"""
    e = unit_exps(A, elem, bfloat)
    if skip_zero_blocks:
        e = np.where(zero_blocks(A), np.nan, e)
    with warnings.catch_warnings():  # (a row of NaN / left-out blocks only: its min is NaN)
        warnings.simplefilter("ignore", RuntimeWarning)
        lo, hi = np.nanmin(e, -1), np.nanmax(e, -1)
    return lo, hi - lo


def gemm_gate(x, W, bfloat=32, elem="int8"):
    """The GEMM's digit kernels: (per 32-row block: rows' min + weight's min [NaN: no block
    left], per 32-row block the largest row spread, the largest weight column spread).  A row
    or column without a block left counts as spread 0 (so does a weight of such columns only,
    for which the MXINT8 tests' earlier copy gave NaN; no input has one)."""
    lo, sp = row_stats(x, True, bfloat, elem)
    wlo, wsp = row_stats(W, False, bfloat, elem)
    nrb = (x.shape[0] + 31) // 32
    with warnings.catch_warnings():  # (a row block, or a weight, of such rows only)
        warnings.simplefilter("ignore", RuntimeWarning)
        q = np.array([np.nanmin(lo[32 * r: 32 * r + 32]) for r in range(nrb)]) + np.nanmin(wlo)
    smx = np.array([np.nanmax(np.nan_to_num(sp[32 * r: 32 * r + 32])) for r in range(nrb)])
    return q, smx, np.nanmax(np.nan_to_num(wsp))


def on_digits(x, W, bfloat=32, elem="int8"):
    """per 32-row block: does the digit K loop take it?"""
    q, smx, wsp = gemm_gate(x, W, bfloat, elem)
    return (smx <= SPREAD[elem]) & (wsp <= SPREAD[elem]) & ~(q < GATE)


def assert_side(x, W, want, bfloat=32, what="", elem="int8"):
    """every row block on the wanted side ("digits" / "fp64"); returns (digit blocks, blocks)"""
    d = on_digits(x, W, bfloat, elem)
    assert (d.all() if want == "digits" else not d.any()), (what, want, gemm_gate(x, W, bfloat, elem))
    return int(d.sum()), d.size


def qkv_gate(x_tile, W, H):
    """qkv_proj_kernel on one 32-token tile (rows, C): (per head: tile min + the head's q, k, v
    columns' min, the tile's largest row spread, per head the largest column spread)."""
    lo, sp = row_stats(x_tile, False)
    wlo, wsp = row_stats(W, False)
    D = W.shape[0] // (3 * H)
    glo = wlo.reshape(3, H, D).min((0, 2))
    gsp = wsp.reshape(3, H, D).max((0, 2))
    return np.nanmin(lo) + glo, np.nanmax(np.nan_to_num(sp)), gsp


def pow2(e):
    return np.float32(2.0) ** np.float32(e)


# ---- block construction: every 32-block normalised to one binade, block b scaled by 2^(s_b) ----
def blocks_to_unit(a):
    """every 32-block along the last axis scaled by a power of two to max |.| in [1, 2): shared
    exponent 0 (a ragged last block by its valid columns)"""
    n = a.shape[-1]
    nb = (n + 31) // 32
    p = np.zeros(a.shape[:-1] + (nb * 32,), F32)
    p[..., :n] = a
    bm = np.abs(p.reshape(a.shape[:-1] + (nb, 32))).max(-1)
    return (a * np.repeat(np.exp2(-np.floor(np.log2(bm))).astype(F32), 32, axis=-1)[..., :n]).astype(F32)


def scaled(a, shifts):
    """block b of row r of a times 2^shifts[r, b]"""
    return (a * np.repeat(np.exp2(shifts.astype(np.float64)).astype(F32), 32, axis=-1)[..., : a.shape[-1]]).astype(F32)


def normalised_rows(rng, rows, inf, first_of_block_shift0=True):
    """test_mx_linear_digit_path_vs_oracle's rows: every 32-block normalised to max |x| in
    [1, 2), then scaled by 2^0 .. 2^8 (the row's whole spread); block 0 of the first row of
    every 32-row block keeps 2^0, so every row block has the same smallest exponent."""
    x = blocks_to_unit(rng.standard_normal((rows, inf), dtype=F32))
    sh = rng.integers(0, 9, size=(rows, (inf + 31) // 32))
    if first_of_block_shift0:
        sh[::32, 0] = 0
    return scaled(x, sh)


def k_edge_operands(rng, rows, outf, inf, wshift):
    """The K-edge tests' x (rows, inf) and W (outf, inf): every block normalised, x's blocks
    scaled by 2^0 .. 2^3 (each K-block contributes at its own scale), W's by 2^wshift."""
    nb = (inf + 31) // 32
    x = scaled(blocks_to_unit(rng.standard_normal((rows, inf), dtype=F32)), rng.integers(0, 4, size=(rows, nb)))
    W = scaled(blocks_to_unit(rng.standard_normal((outf, inf), dtype=F32)), np.full((outf, nb), wshift))
    return x, W
