"""CPU helpers for the tests of the digit kernels' subnormal gate (mxa_gemm.hpp
mx_gemm_dig_kernel, mxa_proj.hpp qkv_proj_kernel): the gates' quantities restated from the
oracle's block exponents, so that each test input provably sits in its regime.

The device keeps a block's exponent as that of a code unit, e = es - 6 for MXINT8 (es: the
oracle's shared exponent, quantize_mx(...)[2]; value = code * 2^e).  Every block product is
an integer times 2^(ex + ew), so a result is a multiple of 2^(min ex + min ew): normal (or
zero) when that sum is >= -126 -- the digit fast path's condition.  Below it the kernels sum
the blocks in fp64 and round once to float32, subnormals included.

  mx_gemm_dig_kernel, per 32-row block:  min over its rows' blocks (NaN blocks and all-zero
      blocks left out) + min over every weight column's blocks            >= -126
  qkv_proj_kernel, per 32-token tile and head:  min over the tile's rows' blocks (NaN blocks
      left out) + min over the head's q, k, v weight columns' blocks       >= -126
and the digit operands exist when every row's and every weight column's spread (max - min)
is <= 8 (kDigitSpread)."""
import warnings

import numpy as np

from oracle import mx_oracle as O

GATE = -126          # the last value at which the gate does not fire
DIGIT_SPREAD = 8     # mxa_proj_args.hpp kDigitSpread
F32_MIN_NORMAL = np.float32(2.0 ** -126)


def unit_exps(A):
    """(rows, nb) code-unit exponents of A's 32-blocks along its last axis as float64; NaN for
    a block that holds a NaN."""
    A = np.asarray(A, np.float32)
    return O.quantize_mx(A, "int8", 32, -1)[2][..., 0].astype(np.float64) - 6.0


def zero_blocks(A):
    A = np.asarray(A, np.float32)
    nb = (A.shape[-1] + 31) // 32
    P = np.zeros(A.shape[:-1] + (nb * 32,), np.float32)
    P[..., : A.shape[-1]] = A
    return (P.reshape(A.shape[:-1] + (nb, 32)) == 0).all(-1)


def row_stats(A, skip_zero_blocks):
    """per row: (min, spread) of the code-unit exponents (NaN: the row has no block left)"""
    e = unit_exps(A)
    if skip_zero_blocks:
        e = np.where(zero_blocks(A), np.nan, e)
    with warnings.catch_warnings():  # (a row of NaN / left-out blocks only: its min is NaN)
        warnings.simplefilter("ignore", RuntimeWarning)
        lo, hi = np.nanmin(e, -1), np.nanmax(e, -1)
    return lo, hi - lo


def gemm_gate(x, W):
    """mx_gemm_dig_kernel: (per 32-row block: rows' min + weight's min, the largest row spread
    per block, the largest weight column spread)."""
    lo, sp = row_stats(x, True)
    wlo, wsp = row_stats(W, False)
    nrb = (x.shape[0] + 31) // 32
    q = np.array([np.nanmin(lo[32 * r: 32 * r + 32]) for r in range(nrb)]) + np.nanmin(wlo)
    smx = np.array([np.nanmax(np.nan_to_num(sp[32 * r: 32 * r + 32])) for r in range(nrb)])
    return q, smx, np.nanmax(wsp)


def qkv_gate(x_tile, W, H):
    """qkv_proj_kernel on one 32-token tile (rows, C): (per head: tile min + the head's q, k, v
    columns' min, the tile's largest row spread, per head the largest column spread)."""
    lo, sp = row_stats(x_tile, False)
    wlo, wsp = row_stats(W, False)
    D = W.shape[0] // (3 * H)
    glo = wlo.reshape(3, H, D).min((0, 2))
    gsp = wsp.reshape(3, H, D).max((0, 2))
    return np.nanmin(lo) + glo, np.nanmax(np.nan_to_num(sp)), gsp


def normalised_rows(rng, rows, inf, first_of_block_shift0=True):
    """test_mx_linear_digit_path_vs_oracle's rows: every 32-block normalised to max |x| in
    [1, 2), then scaled by 2^0 .. 2^8 (the row's whole spread); block 0 of the first row of
    every 32-row block keeps 2^0, so every row block has the same smallest exponent."""
    x = rng.standard_normal((rows, inf), dtype=np.float32)
    nb = (inf + 31) // 32
    xp = np.zeros((rows, nb * 32), np.float32)
    xp[:, :inf] = x
    bm = np.abs(xp.reshape(rows, nb, 32)).max(-1)
    norm = np.repeat(np.exp2(-np.floor(np.log2(bm))).astype(np.float32), 32, axis=1)[:, :inf]
    sh = rng.integers(0, 9, size=(rows, nb))
    if first_of_block_shift0:
        sh[::32, 0] = 0
    xs = np.repeat(np.exp2(sh).astype(np.float32), 32, axis=1)[:, :inf]
    return (x * norm * xs).astype(np.float32)


def pow2(e):
    return np.float32(2.0) ** np.float32(e)
