"""What the tests of the score bias's layouts and of a caller's out buffer share
(test_bias_cases_cpu.py, test_gpu_bias_out.py): one smallest shape per finishing kernel
(include/mxa.h MXA_FIN_*) at each width, a real-valued bias whose storage the GPU file varies,
the value sets its broadcast layouts stand for, and the oracle's references (computed once, left
unchanged).  Nothing here touches the device.

Every kernel addresses the bias through four element strides (Rows2Args bs0 .. bs3) and the output
through three (os0 .. os2).  A 0 / -10000 mask of shape (B, 1, 1, T) leaves bs1 = bs2 = 0 and bs3 = 1
and never reorders a ranking; the bias here is standard_normal * 2 on all of (B, H, N, T), so a
dropped, swapped or ignored stride changes the kept indices of every row (test_bias_cases_cpu.py
asserts it from the oracle alone).  B >= 2 and H >= 2 everywhere, H = 3 where it is cheap: a b / h
mix-up cannot cancel."""
import collections
import functools

import numpy as np

import cross_cases as CC
import exact_out_cases as EC
import long_dense_cases as LC
from gpu_support import ELEM, out_row_bound, r_kw, r_scale  # noqa: F401
from oracle import mx_oracle as O

F32 = np.float32
# the row-wise bound's entry (gpu_support.n_add_and_chain) per finishing kind; the tiled long kernel keeps
# finish_qk_kernel's figures (long_dense_cases.kernel_name)
KERNEL = {EC.GATHER16: "fin16", EC.GATHER32: "fin32", EC.MFMA: "qk", EC.DENSE_MFMA: "dense_qk", EC.DENSE_ROWS: "dense_rows",
          LC.MFMA_LONG: "qk", LC.DENSE_MFMA_LONG: "dense_qk"}
# k = 0: dense; mode None: approx=False (top-k of the true scores); bits: the width; seed: the generator's
Case = collections.namedtuple("Case", "kind B H N T D k mode bits seed")


def _c(kind, B, H, N, T, D, k, mode="ex_pred", bits=8, seed=1):
    return Case(kind, B, H, N, T, D, k, mode, bits, seed)


def case_id(c):
    return (f"{KERNEL[c.kind]}{'_long' if c.T > 512 else ''}-B{c.B}H{c.H}N{c.N}T{c.T}D{c.D}" + (f"k{c.k}" if c.k else "dense") +
            (f"-{c.mode or 'trueK'}" if c.k else "") + (f"-w{c.bits}" if c.bits != 8 else ""))


G16 = _c(EC.GATHER16, 2, 3, 40, 77, 48, 20)
MFMA = _c(EC.MFMA, 2, 2, 40, 130, 64, 65)
G32 = _c(EC.GATHER32, 2, 2, 40, 300, 72, 129)
DENSE_MFMA = _c(EC.DENSE_MFMA, 2, 2, 40, 77, 48, 0)
DENSE_ROWS = _c(EC.DENSE_ROWS, 2, 2, 40, 300, 72, 0)
CASES = [G16, G16._replace(mode="MXINT4"), G16._replace(mode=None), MFMA, G32, DENSE_MFMA, DENSE_ROWS,
         _c(EC.GATHER16, 2, 2, 33, 600, 32, 20), _c(LC.MFMA_LONG, 2, 2, 33, 600, 32, 129),
         _c(LC.DENSE_MFMA_LONG, 2, 2, 33, 513, 32, 0)]
CASES += [G16._replace(bits=4), G16._replace(mode="MXINT4", bits=4), MFMA._replace(bits=4), DENSE_MFMA._replace(bits=4),
          _c(LC.DENSE_MFMA_LONG, 2, 2, 33, 513, 32, 0, bits=4)]
XDT_CASES = [G16, MFMA, G32, DENSE_MFMA, DENSE_ROWS]  # the kernels with a float16 / bfloat16 instantiation

# the value sets: "full" is the (B, H, N, T) values that layouts (a) .. (d) store four ways; the others are the
# broadcast layouts' -- (e) "hnt" (H, N, T), (f) "h1t" (1, H, 1, T), (g) "nt" (N, T), (h) "mask" -- cut from the
# same values, and the two the CPU file adds: "head0" (head 0's over the heads) and "none".  "hnt" is also batch
# 0's values over the batches.
VALUE_SETS = ("full", "hnt", "h1t", "nt", "mask")


@functools.lru_cache(maxsize=None)
def inputs(c):
    """q, k, v and the bias values (B, H, N, T) = standard_normal * 2, from default_rng(seed) in that order"""
    rng = np.random.default_rng([c.seed, c.N, c.T, c.D])
    q = rng.standard_normal((c.B, c.H, c.N, c.D), dtype=F32)
    k = rng.standard_normal((c.B, c.H, c.T, c.D), dtype=F32)
    v = rng.standard_normal((c.B, c.H, c.T, c.D), dtype=F32)
    bias = (rng.standard_normal((c.B, c.H, c.N, c.T), dtype=F32) * F32(2.0)).astype(F32)
    return q, k, v, bias


def mask_bias(B, N, T):
    """The masks the suite already passes, in one: (B, 1, N, T), 0 on the first T // 2 + 5 b keys of image b and
    -10000 behind them (PixArt's), and row 2 of the last image all -inf (exact_out_cases'): a NaN row in every kind"""
    m = np.zeros((B, 1, N, T), F32)
    for b in range(B):
        m[b, ..., T // 2 + 5 * b:] = -10000.0
    m[B - 1, 0, 2, :] = -np.inf
    return m


def bias_values(c, vs):
    """the array a value set passes as `bias` (it broadcasts to (B, H, N, T) the way the op does)"""
    V = inputs(c)[3]
    return {"full": V, "hnt": V[0], "h1t": V[:1, :, :1, :], "nt": V[0, 0], "head0": V[:, :1],
            "mask": mask_bias(c.B, c.N, c.T), "none": None}[vs]


@functools.lru_cache(maxsize=None)
def reference(c, vs="full"):
    q, k, v, _ = inputs(c)
    return O.attention(q, k, v, r_scale(c), bias=bias_values(c, vs), elem=ELEM[c.bits], **r_kw(c))


def shares(c, vs):
    """the eligible shares (elements, rows) of the row-wise bound, from the oracle alone"""
    return out_row_bound(reference(c, vs), inputs(c)[2], KERNEL[c.kind], c.bits)[2]


# ---- the fused blocks: the existing chains' projections, a real-valued bias ---------------------------
def fused_bias(B, H, N, T, vs, seed=3):
    V = (np.random.default_rng([seed, B, H, N, T]).standard_normal((B, H, N, T), dtype=F32) * F32(2.0)).astype(F32)
    return {"full": V, "hnt": V[0]}[vs]


@functools.lru_cache(maxsize=None)
def cross_reference(bits, vs):
    """mx_cross_attention on cross_cases "d48": the chain's qh, kh, vh (the oracle's Linears and the
    module's head split) through the oracle's attention at the width, with the bias of a value set.
    Returns (the chain, bias, r)."""
    (B, N, T, C, _, H), k_top = CC.SHAPES["d48"]
    ch = CC.chain("d48", "ex_pred", elem=ELEM[bits])
    bias = fused_bias(B, H, N, T, vs)
    return ch, bias, O.attention(ch["qh"], ch["kh"], ch["vh"], (C // H) ** -0.5, k_top=k_top, pred_mode="ex_pred", bias=bias,
                                 elem=ELEM[bits])


@functools.lru_cache(maxsize=None)
def self_reference(bits, vs):
    """mx_qkv_attention on cross_cases.SELF_SHAPES["d48"]: cross_cases.self_chain's projections at the width.
    Returns (qkv, (qh, kh, vh), bias, r)."""
    (B, N, C, H), k = CC.SELF_SHAPES["d48"]
    ch = CC.self_chain("d48", elem=ELEM[bits])
    heads = ch["qh"], ch["kh"], ch["vh"]
    bias = fused_bias(B, H, N, N, vs)
    return ch["qkv"], heads, bias, O.attention(*heads, (C // H) ** -0.5, k_top=k, pred_mode="ex_pred", bias=bias, elem=ELEM[bits])
