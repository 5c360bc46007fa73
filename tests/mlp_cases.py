"""The inputs of the MLP tests that have to sit in a particular regime of mx_mlp_fc1_kernel's
epilogue quantizer (mxa_mlp.hpp MlpEpi -> xo_block), of the GELU (mxa_act.hpp) or of fc2's
digit kernel, shared by the GPU tests (test_gpu_mlp.py) and by the CPU test that proves with
the oracle alone that each input is where it is meant to be (test_mlp_cases_cpu.py).

Exponents, the gate and the block construction are those of tests/gate_cases.py at its
default elem="int8": the oracle's shared exponent es of a 32-block (quantize_mx(...)[2]), the
code unit's exponent es - 6, the digit kernel's gate on the sum of the rows' and the weight's
smallest code-unit exponents (>= -126: the digit fast path; below, or with a spread beyond
kDigitSpread = 8, the fp64 block sums).  same_bits is tests/gpu_support.py's.  The regimes of the
hidden matrix are asserted on pre = O.mx_linear(x, W1, b1) and on torch's CPU GELU of it:
they hold with a margin of many ulps, the device's own GELU may differ in the last bits."""
import math

import numpy as np
import torch

import gate_cases as GC
from gpu_support import same_bits
from oracle import mx_oracle as O

F32 = np.float32
ACTS = ("gelu", "gelu_tanh")
MLP_NBK_MAX = 72  # mxa_mlp.hpp kMlpNbkMax: the K-blocks the fused fc1 stages in LDS


def case(rows, inf, hid, outf, seed):
    """ordinary data: x ~ N(0, 1), pre of standard deviation about 0.15 sqrt(inf) (the MXINT4
    tests' too: int4_cases.mlp_case)"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((rows, inf), dtype=F32)
    W1 = (rng.standard_normal((hid, inf), dtype=F32) * F32(0.15)).astype(F32)
    b1 = (rng.standard_normal(hid, dtype=F32) * F32(0.5)).astype(F32)
    W2 = (rng.standard_normal((outf, hid), dtype=F32) * F32(0.1)).astype(F32)
    b2 = (rng.standard_normal(outf, dtype=F32) * F32(0.1)).astype(F32)
    return x, W1, b1, W2, b2


def _al(n):
    return (n + 255) // 256 * 256


def workspace_bytes(rows, inf, hid, fused):
    """mxa_mlp_workspace_bytes restated (tests/test_mlp_cpu.py mlp_workspace): the MX rows of x
    and of the hidden matrix; the fallback adds the fp32 hidden matrix."""
    mxr = lambda r, c: _al((r + 31) // 32 * 32 * ((c + 31) // 32) * 32) + _al(r * ((c + 31) // 32) * 2)  # noqa: E731
    return mxr(rows, inf) + mxr(rows, hid) + (0 if fused else _al(rows * hid * 4))


def gelu_cpu(pre, act):
    """torch's own CPU kernel on a float32 array"""
    t = torch.from_numpy(np.ascontiguousarray(pre, dtype=F32))
    return torch.nn.functional.gelu(t, approximate="tanh" if act == "gelu_tanh" else "none").numpy()


def shared_exps(A):
    """(rows, nb) the oracle's shared exponents es of A's 32-blocks (clamped to >= -127)"""
    return O.quantize_mx(np.asarray(A, F32), "int8", 32, -1)[2][..., 0]


# ---- the exact Linear: integer arithmetic instead of the oracle's float64 sums ------------
def _rne_f32(n, e):
    """n 2^e (Python int n) rounded once to float32, ties to even, subnormals included"""
    if n == 0:
        return F32(0.0)
    s, n = (-1.0, -n) if n < 0 else (1.0, n)
    lsb = max(n.bit_length() - 1 + e - 23, -149)
    sh = lsb - e
    if sh <= 0:
        q = n << -sh
    else:
        q, r, half = n >> sh, n & ((1 << sh) - 1), 1 << (sh - 1)
        if r > half or (r == half and q & 1):
            q += 1
    return F32(s * math.ldexp(float(q), lsb))  # (q <= 2^24: exact; beyond float32: inf)


def exact_mx_linear(x, W, bias=None, flush=False):
    """O.mx_linear(x, W, bias, flush=flush) for NaN-free float32 operands with every block sum
    taken exactly: codes times 2^exponent as Python ints, one rounding to float32, then the
    float32 bias add.  Where O.exact_matmul_f32's float64 accumulation is no longer provably
    exact (blocks more than 2^29 apart) this says which result is the right one."""
    _, cx, ex = O.quantize_mx(np.asarray(x, F32), "int8", 32, -1, flush=flush)
    _, cw, ew = O.quantize_mx(np.asarray(W, F32), "int8", 32, -1, flush=flush)
    P = np.einsum("rbk,obk->rob", cx.astype(np.int64), cw.astype(np.int64))  # |.| <= 32 127^2
    E = (ex[:, None, :, 0] + ew[None, :, :, 0]).astype(np.int64) - 12
    lo = int(E.min())
    S = (P.astype(object) * (2 ** (E - lo).astype(object))).sum(-1)
    out = np.array([[_rne_f32(int(v), lo) for v in row] for row in S], dtype=F32).reshape(S.shape)
    return out if bias is None else (out + np.asarray(bias, F32)).astype(F32)


# ---- 2. the K edge of the fused fc1 -------------------------------------------------------
K_EDGE_ROWS, K_EDGE_HID, K_EDGE_OUT = 33, 64, 40
K_EDGE_INF = (2304, 2290, 2336)  # 72 blocks; 72 blocks, 18 valid columns in the last; 73 blocks


def k_edge(inf):
    """test_mx_linear_long_k_tile_vs_oracle's operands: every block of x and W1 normalised, x's
    blocks then scaled by 2^0 .. 2^3 (each K-block contributes at its own scale); W1 by 2^-6 so
    that pre stays of order 1 and the GELU is not saturated."""
    x, W1 = GC.k_edge_operands(np.random.default_rng(inf), K_EDGE_ROWS, K_EDGE_HID, inf, -6)
    _, _, b1, W2, b2 = case(K_EDGE_ROWS, 32, K_EDGE_HID, K_EDGE_OUT, inf + 1)
    return x, W1, b1, W2, b2


def assert_k_edge(inf, x, W1):
    """the digit fast path at every row block, row spreads 3, column spreads 0; the block count
    on its side of kMlpNbkMax"""
    q, smx, wsp = GC.gemm_gate(x, W1)
    assert (q >= GC.GATE).all() and smx.max() == 3 and wsp == 0, (q, smx, wsp)
    nb = (inf + 31) // 32
    assert nb == {2304: MLP_NBK_MAX, 2290: MLP_NBK_MAX, 2336: MLP_NBK_MAX + 1}[inf]
    assert MLP_NBK_MAX * 2048 + 400 + 4224 == 152080 <= 160 * 1024  # the LDS the 72-block launch asks for
    return dict(gate=q.min(), row_spread=smx.max(), col_spread=wsp)


# ---- 4. hidden-value extremes through the epilogue quantizer --------------------------------
EXT_SHAPE = (70, 96, 224, 40)  # seven hidden blocks, three row blocks, the last partial
EXTREMES = ("spread", "zero_block", "tiny", "sub_gate")


def _blk(j):
    return slice(32 * j, 32 * j + 32)


def extremes(name):
    """(x, W1, b1, W2, b2) of the case `name` (assert_extremes says what each is)"""
    rows, inf, hid, outf = EXT_SHAPE
    x, W1, b1, W2, b2 = case(rows, inf, hid, outf, 224)
    if name in ("zero_block", "sub_gate"):
        b1[_blk(1)] = -30.0
        if name == "sub_gate":
            W2 = (W2 * F32(2.0 ** -122)).astype(F32)
            b2 = (b2 * F32(2.0 ** -122)).astype(F32)
    elif name == "spread":
        b1[_blk(1)] = -30.0
        b1[_blk(2)] = 4096.0
        b1[_blk(3)] = -5.2
        b1[128:144], b1[144:160] = 300.0, -30.0
        W1[_blk(5)] *= F32(2.0 ** -100)
        b1[_blk(5)] = 0.0
        # W2's columns of the small blocks scaled up, so that every block's codes are seen in y
        W2[:, _blk(3)] *= F32(2.0 ** 24)
        W2[:, _blk(5)] *= F32(2.0 ** 100)
    elif name == "tiny":
        # x's first block as the dictated GELU inputs have it (gelu_pinned): code 64 in column 0
        x[:, :32] = np.random.default_rng(5).uniform(-1.9, 1.9, (rows, 32)).astype(F32)
        x[:, 0], x[:, 1] = 1.0, 1.5
        # block 4: pre = +-m 2^-132, m in [64, 128): normal, and act = pre / 2 is subnormal
        m = (64 + (np.arange(32) * 37) % 64).astype(F32)
        m[0] = 127.0
        W1[_blk(4)] = 0.0
        W1[_blk(4), 0] = m * np.where(np.arange(32) % 3 == 0, -1, 1).astype(F32) * F32(2.0 ** -132)
        b1[_blk(4)] = 0.0
        W2[:, _blk(4)] *= F32(2.0 ** 125)  # so that the subnormal block is seen in y
        # block 5: act of about 2^-125: the quantizer's es < -121
        W1[_blk(5)] *= F32(2.0 ** -124)
        b1[_blk(5)] = 0.0
        W2[:, _blk(5)] *= F32(2.0 ** 118)
    else:
        raise ValueError(name)
    return x, W1, b1, W2, b2


def _seen_in_y(a, W2, b2, flush, blocks):
    """per block: the share of y's elements that change when the block of act is zeroed"""
    y = O.mx_linear(a, W2, b2, flush=flush)
    out = {}
    for j in blocks:
        a0 = a.copy()
        a0[:, _blk(j)] = 0.0
        out[j] = float((O.mx_linear(a0, W2, b2, flush=flush) != y).mean())
    return out


def assert_extremes(name, x, W1, b1, W2, b2, act, flush):
    """The regime of the case on the oracle's pre and torch's CPU GELU of it; returns the
    figures (DESIGN.md section 4 quotes them)."""
    rows, inf, hid, outf = EXT_SHAPE
    pre = O.mx_linear(x, W1, b1, flush=flush)
    a = gelu_cpu(pre, act)
    assert np.isfinite(pre).all() and np.isfinite(a).all()
    q1, smx1, wsp1 = GC.gemm_gate(x, W1)
    lo, sp = GC.row_stats(a, True)
    _, sp_all = GC.row_stats(a, False)
    zb = GC.zero_blocks(a)
    es = shared_exps(a)
    q2, smx2, wsp2 = GC.gemm_gate(a, W2)
    fig = dict(fc1_gate=q1.max(), fc1_row_spread=smx1.max(), fc1_col_spread=wsp1, hidden_spread_min=np.nanmin(sp),
               hidden_spread_max=np.nanmax(sp), fc2_gate=q2.max(), fc2_col_spread=wsp2)
    assert smx1.max() <= GC.DIGIT_SPREAD and wsp1 <= GC.DIGIT_SPREAD, fig
    if name != "tiny":  # fc1 on the digit fast path at every row block
        assert (q1 >= GC.GATE).all(), fig
    if name in ("spread", "zero_block", "sub_gate"):  # the GELU's own all-zero block, every row
        assert zb[:, 1].all() and np.signbit(a[:, _blk(1)]).all() and (pre[:, _blk(1)] < -10).all()
    if name == "spread":
        assert (a[:, _blk(2)] == pre[:, _blk(2)]).all() and (pre[:, _blk(2)] > 4000).all()  # large
        t = a[:, _blk(3)]  # exact zeros next to |act| of about 1e-7
        assert ((t == 0).any(-1) & (t != 0).any(-1)).sum() > rows // 2 and np.abs(t[t != 0]).min() < 1e-6
        assert (a[:, 128:144] > 280).all() and (a[:, 144:160] == 0).all()  # large next to zeros in one block
        t = a[:, _blk(5)]  # act = pre / 2 of about 2^-101
        assert (t == pre[:, _blk(5)] * F32(0.5)).all() and (es[:, 5] <= -97).all() and (es[:, 5] >= -106).all()
        # fc2's digit kernel sums every row block in fp64, on exponents the epilogue wrote
        assert (sp > GC.DIGIT_SPREAD).all(), fig
        fig["seen_in_y"] = _seen_in_y(a, W2, b2, flush, (0, 2, 3, 4, 5, 6))
        assert min(fig["seen_in_y"].values()) > 0.5, fig
    elif name in ("zero_block", "sub_gate"):
        # within the digit spread only because the zero block is left out of the row statistics
        assert (sp <= GC.DIGIT_SPREAD).all() and (sp_all > GC.DIGIT_SPREAD).all(), fig
        assert wsp2 <= GC.DIGIT_SPREAD, fig
        if name == "zero_block":
            assert (q2 >= GC.GATE).all(), fig  # fc2's fast path
        else:  # fc2's subnormal gate alone, and results on both sides of 2^-126
            assert (q2 < GC.GATE).all(), fig
            y = O.mx_linear(a, W2, b2, flush=flush)
            sub = (np.abs(y) < GC.F32_MIN_NORMAL) & (y != 0)
            assert sub.any() and not sub.all(), sub.sum()
            fig["y_subnormal"] = int(sub.sum())
    elif name == "tiny":
        assert (q1 < GC.GATE).all(), fig  # fc1's fp64 block sums at every row block
        p4, a4 = pre[:, _blk(4)], a[:, _blk(4)]
        assert (np.abs(p4) >= GC.F32_MIN_NORMAL).all()  # normal pre ...
        assert (a4 == p4 * F32(0.5)).all() and (np.abs(a4) < GC.F32_MIN_NORMAL).all()  # ... subnormal act
        assert (es[:, 4] == -127).all()  # the block's shared exponent: flushed with flush_subnormals
        # x's and W1's own blocks are normal: with flush_subnormals nothing of them is flushed
        assert (shared_exps(x) > -127).all() and (shared_exps(W1[_blk(4)])[:, 0] == -126).all()
        assert (np.abs(a[:, _blk(5)]).max(-1) < 2.0 ** -121).all() and (es[:, 5] < -121).all() and (es[:, 5] > -127).all()
        yf, yn = O.mx_linear(a, W2, b2, flush=True), O.mx_linear(a, W2, b2, flush=False)
        fig["y_flush_sensitive"] = int((yf != yn).sum())
        assert fig["y_flush_sensitive"] > 0
        fig["seen_in_y"] = _seen_in_y(a, W2, b2, False, (4, 5))
        assert min(fig["seen_in_y"].values()) > 0.5, fig
    return fig, pre, a


# ---- 5. the GELU where the formula pins it --------------------------------------------------
GELU_ROWS = 33
_MS = (64, 77, 101, 127)


def _targets(es_):
    t = [s * m * 2.0 ** (e - 6) for e in es_ for m in _MS for s in (1.0, -1.0)]
    return [v for v in t if (abs(v) >= 10 or abs(v) <= 2.0 ** -30) and abs(v) <= 2.0 ** 100]


def gelu_pinned(kind):
    """(x, W1, b1, target): O.mx_linear(x, W1, b1) == target in every row.
    x (33, 32) has 1.0 in column 0 (code 64 of a block of shared exponent 0); W1's row j is
    +-m 2^(e - 6) in column 0 (code m of a block of shared exponent e) and 0 elsewhere, so pre =
    64 m 2^(-6 + e - 6) exactly.  "fast": e >= -114, the digit fast path.  "slow": the smallest
    normal weights, zero rows whose b1 is the (subnormal, zero) target, and -0.0 -- reached as a
    sum of -2^-152 (x's second block holds 2^-26 next to 2^-20, the weight -2^-126) rounded to
    float32 with b1 = -0.0: fc1's fp64 block sums."""
    rng = np.random.default_rng(32)
    x = rng.uniform(-1.9, 1.9, (GELU_ROWS, 32)).astype(F32)
    x[:, 0], x[:, 1] = 1.0, 1.5
    if kind == "fast":
        t = _targets((3, 4, 5, 6, 7, 10, 20, 50, 64, 99, 100, -24, -30, -31, -40, -60, -100, -113, -114))
        t = np.array(t, np.float64)  # 128 of them
        W1 = np.zeros((t.size, 32), F32)
        W1[:, 0] = t.astype(F32)
        return x, W1, None, t.astype(F32)
    if kind != "slow":
        raise ValueError(kind)
    tw = np.array(_targets((-115, -120, -125, -126)), np.float64)  # normal weights below the gate
    sub = [2.0 ** e for e in (-127, -128, -130, -140, -148, -149)] + [3 * 2.0 ** -149, 5 * 2.0 ** -149, 127 * 2.0 ** -133,
                                                                          (2 ** 23 - 1) * 2.0 ** -149]
    tb = np.array([s * v for v in sub for s in (1.0, -1.0)] + [0.0, 0.0], np.float64)  # b1 on zero rows
    n = tw.size + tb.size + 2
    hid = (n + 15) // 16 * 16
    x2 = np.zeros((GELU_ROWS, 64), F32)
    x2[:, :32] = x
    x2[:, 32], x2[:, 33] = 2.0 ** -20, 2.0 ** -26
    W1 = np.zeros((hid, 64), F32)
    b1 = np.zeros(hid, F32)
    t = np.zeros(hid, F32)
    W1[:tw.size, 0] = tw.astype(F32)
    t[:tw.size] = tw.astype(F32)
    b1[tw.size:tw.size + tb.size] = tb.astype(F32)
    t[tw.size:tw.size + tb.size] = tb.astype(F32)
    for j, s in ((tw.size + tb.size, -1.0), (tw.size + tb.size + 1, 1.0)):  # -+2^-152 -> -+0.0
        W1[j, 33] = s * 2.0 ** -126
        b1[j] = t[j] = s * 0.0
    return x2, W1, b1, t


def gelu_closed_form(pre):
    """What mxa_act.hpp's operation order gives once erff / tanhf are exactly +-1 (|pre| >= 10)
    or 1 + (a value below 2^-25) is 1 (|pre| <= 2^-30): pre; -0.0; fl32(pre / 2), subnormal
    rounding and the sign of zero included.  NaN elsewhere (not pinned)."""
    pre = np.asarray(pre, F32)
    out = np.full(pre.shape, np.nan, F32)
    out[pre >= 10] = pre[pre >= 10]
    out[pre <= -10] = F32(-0.0)
    tiny = np.abs(pre) <= F32(2.0 ** -30)
    out[tiny] = (pre[tiny] * F32(0.5)).astype(F32)
    return out


def assert_gelu_pinned(kind, x, W1, b1, t):
    """pre is the target bit for bit on the oracle; the gate's side; every target in a pinned region"""
    same_bits(O.mx_linear(x, W1, b1), np.broadcast_to(t, (x.shape[0], t.size)), f"{kind}: dictated pre")
    q, smx, wsp = GC.gemm_gate(x, W1)
    if kind == "fast":
        assert smx.max() == 0 and wsp == 0 and (q >= GC.GATE).all(), (q, smx, wsp)
    else:
        assert (q < GC.GATE).all(), q
    assert not np.isnan(gelu_closed_form(t)).any()
    return dict(gate=q.max())
