"""What the tests of the dense branch and k > 64 on rows of 513 .. 1,024 keys share
(test_long_dense_cpu.py, test_gpu_long_dense.py; mxa_attention_full, finish_qk_long_kernel): the
exact-result cases (the construction of exact_out_cases.py, at 4 bits attn4_cases.py's), the peaked
random inputs whose eligible shares of the row-wise bound the CPU file asserts from the oracle alone,
the inputs that steer the exact epilogue into each of its branches, and the references (computed
once, left unchanged).  Nothing here touches the device."""
import collections
import functools

import numpy as np

import attn4_cases as A
import exact_out_cases as EC
from gpu_support import ELEM, out_row_bound, r_kw, r_scale  # noqa: F401
from oracle import mx_oracle as O

F32 = np.float32
MFMA_LONG, DENSE_MFMA_LONG = 6, 7  # include/mxa.h MXA_FIN_*: mxa_attention_full alone reports them
_c = EC._c


def kind_of(T, k):
    """mxa_launch.hpp finish_choice(full = true) on rows over 512 keys; k = 0: dense"""
    assert T > 512
    return DENSE_MFMA_LONG if not k else (MFMA_LONG if k > 64 else EC.GATHER16)


def kernel_name(k):
    """gpu_support.n_add_and_chain's entry: the tiled kernel keeps finish_qk_kernel's n_add = ntb
    and chain = 8 ntb + 2"""
    return "qk" if k else "dense_qk"


def case_id(c):
    s = f"{'qk' if c.k else 'dense_qk'}_long-B{c.B}N{c.N}T{c.T}D{c.D}" + (f"k{c.k}" if c.k else "")
    return s + ("-bias" if c.bias else "") + "".join(f"-{a}={b}" for a, b in c.kw)


# ---- exact-result cases ---------------------------------------------------------------------------
# (the Case's kind is finish_qk_kernel's, MFMA / DENSE_MFMA: it names the arithmetic -- exact_out_cases.case_id
# and the inputs' seed read it; the kernel that runs a case is kind_of(T, k))
DENSE_SHAPES = ((40, 1000, 72), (33, 513, 32), (40, 1024, 128))
TOPK_SHAPES = ((40, 600, 64, 65), (40, 1000, 72, 129), (40, 1024, 128, 257))
EXACT = [_c(EC.DENSE_MFMA, 1, 2, N, T, D, 0) for N, T, D in DENSE_SHAPES]
EXACT += [_c(EC.MFMA, 1, 2, N, T, D, k) for N, T, D, k in TOPK_SHAPES]
EXACT += [_c(EC.DENSE_MFMA, 1, 2, 40, 1000, 72, 0, True), _c(EC.MFMA, 1, 2, 40, 1000, 72, 129, True)]
EXACT_BF16 = [_c(EC.MFMA, 1, 2, 40, 1000, 72, 129, bfloat=16)]
# at 4 bits: attn4_cases.exact_inputs / exact_reference (V integers |n| <= 7 times 2^e)
EXACT4 = [_c(EC.DENSE_MFMA, 1, 2, 40, 1000, 72, 0), _c(EC.DENSE_MFMA, 1, 2, 33, 513, 32, 0),
          _c(EC.MFMA, 1, 2, 40, 600, 64, 65), _c(EC.MFMA, 1, 2, 40, 1024, 128, 257),
          _c(EC.DENSE_MFMA, 1, 2, 40, 1000, 72, 0, True), _c(EC.MFMA, 1, 2, 40, 1000, 72, 129, True)]


# ---- peaked random inputs ---------------------------------------------------------------------------
# k = 0: dense; mode None: approx=False; qmul: the queries' multiplier (plain standard_normal rows of
# 1,000 keys exceed the row cap of the row-wise bound: test_long_dense_cpu.py); bits: the width
RCase = collections.namedtuple("RCase", "N T D k mode bias qmul bits")
QMUL = 8.0
# the generator's seed, chosen with QMUL from the oracle alone: the largest eligible shares over ROWS + ROWS4 are
# 0.27 % of the elements and 13.75 % of the rows (seed 7 leaves the dense 1,000-key rows at 20 %; the row share is a
# count over 80 rows and moves by several rows from seed to seed)
SEED = 15


def rcase_id(c):
    return (f"N{c.N}T{c.T}D{c.D}" + (f"k{c.k}" if c.k else "dense") + f"-{c.mode or 'trueK'}" + ("-bias" if c.bias else "") +
            f"-x{c.qmul:g}" + (f"-w{c.bits}" if c.bits != 8 else ""))


def _r(N, T, D, k, mode="ex_pred", bias=False, qmul=QMUL, bits=8):
    return RCase(N, T, D, k, mode, bias, qmul, bits)


ROWS = [_r(N, T, D, 0, bias=b) for N, T, D in ((40, 1000, 72), (33, 513, 32)) for b in (False, True)]
ROWS += [_r(40, 1000, 72, 129, m, b) for m in ("ex_pred", "MXINT4", "true_ex", None) for b in (False, True)]
ROWS += [_r(40, 600, 64, 65, "ex_pred"), _r(40, 600, 64, 65, "MXINT4", True),
         _r(40, 1024, 128, 257, "true_ex"), _r(40, 1024, 128, 257, None, True)]
ROWS4 = [_r(40, 1000, 72, 0, bits=4), _r(33, 513, 32, 0, bias=True, bits=4), _r(40, 1000, 72, 129, "ex_pred", bits=4),
         _r(40, 600, 64, 65, "MXINT4", True, bits=4)]


@functools.lru_cache(maxsize=None)
def r_inputs(c):
    """default_rng(SEED), q, k, v drawn in that order (B = 1, H = 2), the queries times qmul; the
    PixArt-style bias 0 / -10000 on the second half of the keys"""
    rng = np.random.default_rng(SEED)
    q = rng.standard_normal((1, 2, c.N, c.D), dtype=F32)
    k = rng.standard_normal((1, 2, c.T, c.D), dtype=F32)
    v = rng.standard_normal((1, 2, c.T, c.D), dtype=F32)
    q = (q * F32(c.qmul)).astype(F32)
    bias = A.pixart_bias(1, c.N, c.T, c.T // 2) if c.bias else None
    return q, k, v, bias


@functools.lru_cache(maxsize=None)
def r_reference(c):
    q, k, v, bias = r_inputs(c)
    return O.attention(q, k, v, r_scale(c), bias=bias, elem=ELEM[c.bits], **r_kw(c))


def r_shares(c):
    """the eligible shares (elements, rows) of the row-wise bound, from the oracle alone"""
    return out_row_bound(r_reference(c), r_inputs(c)[2], kernel_name(c.k), c.bits)[2]


# ---- the exact epilogue's branches -----------------------------------------------------------------
# finish_qk_long_kernel takes the shifted-int32 form for a (wave, 16-key tile) when the wave's largest
# query block-exponent spread plus the tile's largest key spread is <= 10 and the smallest query plus
# the smallest key exponent is >= -100; else fq_exact, whose int32 form needs a product's exponents
# within 10 and >= -100, else its fp64 sum.  D = 64 (two blocks); the multipliers act on the second.
def epilogue_inputs(which, N=33, T=513, D=64, seed=11):
    rng = np.random.default_rng(seed)
    q = rng.standard_normal((1, 2, N, D), dtype=F32)
    k = rng.standard_normal((1, 2, T, D), dtype=F32)
    v = rng.standard_normal((1, 2, T, D), dtype=F32)
    if which == "spread":  # some keys' blocks 2^14 apart: their tiles leave the fast form, fq_exact sums in fp64
        k[:, :, ::37, 32:] *= F32(2.0 ** 14)
    elif which == "tiny":  # everything near 2^-110: qmin + kmin < -100, the fp64 sum of subnormal scores
        q *= F32(2.0 ** -55)
        k *= F32(2.0 ** -55)
    elif which == "huge":  # scores of magnitude 2^40
        q *= F32(2.0 ** 20)
        k *= F32(2.0 ** 20)
    else:
        assert which == "fast"
    return q, k, v


def epilogue_branches(q, k):
    """per (query row, key) from the oracle's block exponents: (fast-eligible, needs fp64): the
    element-level conditions of the test the kernel makes per wave and tile"""
    eq = O.quantize_mx(q, "int8", 32, -1)[2][..., 0].astype(np.int64)  # (B, H, N, nb)
    ek = O.quantize_mx(k, "int8", 32, -1)[2][..., 0].astype(np.int64)
    e = eq[:, :, :, None, :] + ek[:, :, None, :, :]
    spread, emin = e.max(-1) - e.min(-1), e.min(-1) - 12  # (codes' unit: 2^(e - 6) each)
    qs, ks = eq.max(-1) - eq.min(-1), ek.max(-1) - ek.min(-1)
    fast = (qs[..., :, None] + ks[..., None, :] <= 10) & (emin >= -100)
    return fast, (spread > 10) | (emin < -100)
