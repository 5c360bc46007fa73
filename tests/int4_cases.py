"""The inputs of the MXINT4 Linear / MLP tests (include/mxa.h mxa_linear_weight_prep_bits;
mxa_gemm.hpp mx_gemm_dig4_kernel, mxa_mlp.hpp mx_mlp_fc1_4_kernel), shared by the GPU tests
(test_gpu_int4.py) and by the CPU test that proves with the oracle alone on which side of the
one-digit kernel's gate every row block of every case sits (test_int4_cpu.py).

Exponents and the gate are those of tests/gate_cases.py at elem="int4" (bound below under this
module's names): codes in [-7, 7], the code unit's exponent e = es - 2.  The one-digit kernel
takes a 32-row block when
    the largest spread (max - min of e, all-zero blocks left out) of its rows  <= 4,
    the largest spread of every weight column of the launch                   <= 4   and
    min e over the rows' blocks + min e over the weight's blocks              >= -126;
any other row block is summed block by block in fp64 in the same workgroup.  Beyond 144
K-blocks (K = 4,608), or for a weight without digits over the output columns (groups that are
neither out_features nor a multiple of 32 columns), the tile kernel runs."""
import functools

import numpy as np

import gate_cases as GC
from gate_cases import DIGIT4_SPREAD  # noqa: F401
from gpu_support import rnd, same_bits  # noqa: F401
from mlp_cases import case as mlp_case  # noqa: F401
from oracle import mx_oracle as O

F32 = np.float32
DIG4_NBK_MAX = 144  # mxa_gemm.hpp kGemmDig4NbkMax = mxa_mlp.hpp kMlp4NbkMax
SPECS = {  # the reference's workloads/PixArt/scripts/mx_inference.py:106-122
    'w_elem_format': 'int4', 'a_elem_format': 'int4', 'scale_bits': 8,
    'shared_exp_method': 'max', 'block_size': 32, 'bfloat': 16, 'fp': 0,
    'bfloat_subnorms': True, 'round': 'nearest', 'round_mx_output': 'nearest',
    'round_output': 'nearest', 'round_weight': 'nearest',
    'mx_flush_fp32_subnorms': False, 'custom_cuda': False, 'quantize_backprop': False,
}


def golden_linear(P, i):
    """(x, W, b) of case i of tests/golden/linear_int4.npz, regenerated from its seed"""
    rows, inf, outf = (int(v) for v in P[f"lin{i}/shape"])
    s = int(P[f"lin{i}/seed"])
    return rnd((rows, inf), s), rnd((outf, inf), s + 1, 0.15), rnd((outf,), s + 2, 0.5)


def golden_mlp(P):
    rows, inf, hid, outf = (int(v) for v in P["mlp/shape"])
    s = int(P["mlp/seed"])
    return (rnd((rows, inf), s), rnd((hid, inf), s + 1, 0.15), rnd((hid,), s + 2, 0.5), rnd((outf, hid), s + 3, 0.1),
            rnd((outf,), s + 4, 0.1))


def linear_case(rows, inf, outf, seed):
    """the issue's ordinary data: x ~ N(0, 1), W = 0.15 N(0, 1), b = 0.5 N(0, 1)"""
    return rnd((rows, inf), seed), rnd((outf, inf), seed + 1, 0.15), rnd((outf,), seed + 2, 0.5)


# ---- the gate: tests/gate_cases.py at elem="int4" ------------------------------------------------
unit_exps = functools.partial(GC.unit_exps, elem="int4")
zero_blocks = GC.zero_blocks
row_stats = functools.partial(GC.row_stats, elem="int4")
gate = functools.partial(GC.gemm_gate, elem="int4")
on_digits = functools.partial(GC.on_digits, elem="int4")
assert_side = functools.partial(GC.assert_side, elem="int4")
blocks_to_unit, scaled = GC.blocks_to_unit, GC.scaled  # the gate edges are built from these


EDGE_ROWS, EDGE_IN, EDGE_OUT = 70, 256, 64
EDGES = {  # name: (largest row spread, largest column spread, min ex + min ew, side)
    "row_spread_4": (4, 0, -40, "digits"),
    "row_spread_5": (5, 0, -40, "fp64"),
    "col_spread_4": (2, 4, -40, "digits"),
    "col_spread_5": (2, 5, -40, "fp64"),
    "gate_m126": (4, 4, -126, "digits"),
    "gate_m127": (4, 4, -127, "fp64"),
    "gate_m155": (4, 4, -155, "fp64"),
}


def edge(name):
    """(x, W): every row block of x has a row whose blocks are exactly `row spread` apart (and a
    row holding the smallest exponent), W a column exactly `column spread` apart; the smallest
    code-unit exponents of x and W share the wanted sum about evenly."""
    rsp, csp, q, _ = EDGES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    nb = EDGE_IN // 32
    sx = rng.integers(0, rsp + 1, size=(EDGE_ROWS, nb))
    sx[::32, 0], sx[::32, 1] = 0, rsp  # the first row of every row block: the whole spread
    sw = rng.integers(0, csp + 1, size=(EDGE_OUT, nb))
    sw[5, 2], sw[5, 6] = 0, csp
    bx = (q + 4) // 2  # shared exponents bx + (q + 4 - bx) = q + 4: code units q (each above -127)
    x = scaled(blocks_to_unit(rng.standard_normal((EDGE_ROWS, EDGE_IN), dtype=F32)), sx + bx)
    W = scaled(blocks_to_unit(rng.standard_normal((EDGE_OUT, EDGE_IN), dtype=F32)), sw + (q + 4 - bx))
    return x, W


def assert_edge(name, x, W):
    rsp, csp, q, side = EDGES[name]
    gq, smx, wsp = gate(x, W)
    assert (smx == rsp).all() and wsp == csp and (gq == q).all(), (name, gq, smx, wsp)
    return assert_side(x, W, side, what=name)


# ---- the largest accumulator ----------------------------------------------------------------
ACC_ROWS, ACC_IN, ACC_OUT = 33, 4608, 40


def accumulator(alternate):
    """Every code +-7 (values 1.75 * 2^s), every block but one per row of x and per row of W at
    shift 4, that one at shift 0: |c| = 143 * 32 * 112^2 + ... ~ 5.7e7 in the int32 accumulator.
    alternate: x's sign flips from K-block to K-block, so the running sum swings instead."""
    nb = ACC_IN // 32
    sx = np.full((ACC_ROWS, nb), 4)
    sx[np.arange(ACC_ROWS), np.arange(ACC_ROWS) % nb] = 0
    sw = np.full((ACC_OUT, nb), 4)
    sw[np.arange(ACC_OUT), (np.arange(ACC_OUT) + 50) % nb] = 0
    x = scaled(np.full((ACC_ROWS, ACC_IN), 1.75, F32), sx)
    W = scaled(np.full((ACC_OUT, ACC_IN), 1.75, F32), sw - 8)
    if alternate:
        x *= np.repeat(np.where(np.arange(nb) % 2 == 0, 1, -1).astype(F32), 32)[None, :]
    return x, W


def assert_accumulator(x, W, alternate):
    cx = O.quantize_mx(x, "int4", 32, -1)[1]
    cw = O.quantize_mx(W, "int4", 32, -1)[1]
    assert (np.abs(cx) == 7).all() and (np.abs(cw) == 7).all()
    q, smx, wsp = gate(x, W)
    assert (smx == 4).all() and wsp == 4
    ex, ew = unit_exps(x), unit_exps(W)
    dx = (cx.astype(np.int64) * np.exp2(ex - ex.min(-1, keepdims=True)).astype(np.int64)[..., None])
    dw = (cw.astype(np.int64) * np.exp2(ew - ew.min(-1, keepdims=True)).astype(np.int64)[..., None])
    assert np.abs(dx).max() == 112 and np.abs(dw).max() == 112  # one signed int8 digit each
    c = np.einsum("rbk,obk->ro", dx, dw)
    big = int(np.abs(c).max())
    assert big < 2 ** 31
    if not alternate:
        assert big > 5.6e7, big
    assert_side(x, W, "digits", what="accumulator")
    return big


# ---- the K edge -------------------------------------------------------------------------------
K_EDGE_ROWS, K_EDGE_OUT = 33, 40
K_EDGE_IN = (4608, 4640)  # 144 K-blocks: the one-digit kernel's last; 145: the tile kernel


def k_edge(inf):
    """every block of x and W normalised, x's blocks scaled by 2^0 .. 2^3 (each K-block at its own
    scale), W by 2^-6"""
    x, W = GC.k_edge_operands(np.random.default_rng(inf), K_EDGE_ROWS, K_EDGE_OUT, inf, -6)
    return x, W, rnd((K_EDGE_OUT,), inf + 1, 0.5)


def assert_k_edge(inf, x, W):
    assert (inf + 31) // 32 == {4608: DIG4_NBK_MAX, 4640: DIG4_NBK_MAX + 1}[inf]
    assert DIG4_NBK_MAX * 1024 + 400 + 4224 == 152080 <= 160 * 1024  # the MLP launch's LDS at 144 blocks
    return assert_side(x, W, "digits", what=f"K = {inf}")  # (the gate's side, were the kernel to take the K)


# ---- the MLP ----------------------------------------------------------------------------------
MLP_SHAPES = ((70, 96, 160, 40), (33, 100, 136, 96), (45, 64, 4608, 40), (45, 64, 4640, 40), (5, 32, 32, 7))
