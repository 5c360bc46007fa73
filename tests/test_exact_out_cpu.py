"""The conditions under which the attention output of tests/exact_out_cases.py is the only
float32 result a correct implementation can produce, proved per case with the oracle alone
(DESIGN.md section 2).  The GPU file (test_gpu_exact_out.py) parametrizes over the same list
objects and only compares bits."""
import ctypes

import numpy as np
import pytest

import exact_out_cases as EC
from gpu_support import same, same_bits
from oracle import mx_oracle as O

ALL = EC.CASES + [EC.CHUNK32]


def _ref(c):
    heads = (1, 1) if c is EC.CHUNK32 else None
    return EC.inputs(c, heads), EC.reference(c, heads)


def _bf(c):
    return dict(c.kw).get("bfloat", 32)


def _finite_rows(r):
    return ~np.isnan(r["attn"]).any(-1)


@pytest.mark.parametrize("c", ALL, ids=EC.case_id)
def test_score_gaps_are_zero_or_wide(c):
    """1. within every query row two true scores are equal or at least 150 apart: exp of the
    lower one is exactly 0 in float32, by np.exp and by exp2((v - mx) log2 e), subnormals flushed
    or not (e^-150 < 2^-216)"""
    _, r = _ref(c)
    t = np.sort(r["true"].astype(np.float64), axis=-1)
    fin = np.isfinite(t).all(-1)
    assert fin.sum() >= fin.size - (c.H if c.bias else 0) and fin.any()
    gap = np.diff(t[fin], axis=-1)
    assert ((gap == 0) | (gap >= 150)).all(), gap[(gap != 0) & (gap < 150)][:4]
    assert (gap >= 150).any(-1).all()  # (no row whose scores all tie)
    x = np.float32(-150.0)
    assert np.exp(x) == 0 and np.exp2(np.float32(x * np.float32(1.4426950408889634))) == 0


@pytest.mark.parametrize("c", ALL, ids=EC.case_id)
def test_v_is_its_own_mx_along_the_tokens(c):
    """2. MX(v, axis=-2) == v, and v holds integers"""
    (_, _, v, _), _ = _ref(c)
    same_bits(O.quantize_mx(O.quantize_bfloat(v, _bf(c)), "int8", 32, -2)[0], v, "MX(v)")
    assert (v == np.round(v)).all() and np.abs(v).max() <= 15 * 8


@pytest.mark.parametrize("c", ALL, ids=EC.case_id)
def test_out_is_the_exact_product(c):
    """3. out equals the float64 product of the quantized operands, that product is a float32,
    and the per-element sum of |Pq| |Vq| is below 2^24 granules (a row's granule: the code step
    2^(e - 6) of its lowest non-zero P block, V being integers): every partial sum in every
    order is an integer below 2^24 times the granule, so exact in float32"""
    (_, _, v, _), r = _ref(c)
    fin = _finite_rows(r)
    pq, _, pe = O.quantize_mx(O.quantize_bfloat(r["attn"], _bf(c)), "int8", 32, -1)
    vq = O.quantize_mx(O.quantize_bfloat(v, _bf(c)), "int8", 32, -2)[0]
    with np.errstate(invalid="ignore"):
        prod = np.matmul(pq.astype(np.float64), vq.astype(np.float64))
        S = np.matmul(np.abs(pq).astype(np.float64), np.abs(vq).astype(np.float64))
    assert (prod[fin] == prod[fin].astype(np.float32)).all()
    same_bits(r["out"][fin], O.quantize_bfloat(prod[fin].astype(np.float32), _bf(c)), "out vs the exact product")
    assert np.isnan(r["out"][~fin]).all()
    blk, _ = O.to_blocks(pq, -1, 32)
    e = np.where((blk != 0).any(-1), pe[..., 0], np.inf)  # the exponents of the non-zero blocks
    gran = np.exp2(e.min(-1) - 6)[fin]
    assert np.isfinite(gran).all()
    assert (pq[fin] / gran[:, None] == np.round(pq[fin] / gran[:, None])).all()
    worst = (S[fin] / gran[:, None]).max()
    print(f"{EC.case_id(c)}: sum |Pq||Vq| reaches 2^{np.log2(max(worst, 1)):.1f} granules")
    assert worst < 2 ** 24


@pytest.mark.parametrize("c", ALL, ids=EC.case_id)
def test_p_codes_survive_four_ulp(c):
    """4. every non-zero p moved by 4 ulp either way keeps the MX codes of P.  Rows whose m is a
    power of two are exempt: p = 1/m is exact there in any implementation, and below it lies
    the next binade."""
    _, r = _ref(c)
    m, _ = EC.tied(c, r)
    rows = (m > 0) & ((m & (m - 1)) != 0)
    assert rows.any() or c.k == 1
    a = r["attn"][rows]
    codes = O.quantize_mx(O.quantize_bfloat(a, _bf(c)), "int8", 32, -1)[1]
    for d in (-4, 4):
        b = a.copy().view(np.int32)
        b[a != 0] += d
        same(O.quantize_mx(O.quantize_bfloat(b.view(np.float32), _bf(c)), "int8", 32, -1)[1], codes, f"P codes at {d} ulp")


@pytest.mark.parametrize("c", ALL, ids=EC.case_id)
def test_tie_counts_vary(c):
    """5. rows with m < k (kept slots of zero weight, P blocks whose codes are all zero) and
    rows with m >= k; on the dense branch m takes several values; k = 1 has m = 1"""
    _, r = _ref(c)
    m_all, kept = EC.tied(c, r)
    m = m_all[m_all > 0]
    if c.k == 1:
        assert (m == 1).all()
    elif c.k:
        assert (m < kept).any() and (m >= kept).any(), np.unique(m)
        fin = _finite_rows(r)
        assert (np.take_along_axis(r["attn"], r["idx"], -1)[fin] == 0).any()  # a kept slot of zero weight
        if c.T >= 197:  # (a row of three key blocks can have a hot key in each)
            pq = O.quantize_mx(r["attn"], "int8", 32, -1)[0]
            idx_blocks = np.take_along_axis(O.to_blocks(pq, -1, 32)[0].any(-1), r["idx"] >> 5, -1)
            assert (~idx_blocks)[fin].any()  # a kept key in a P block whose codes are all zero
    else:
        assert len(np.unique(m)) >= 3, np.unique(m)
    if c.T > 512 and not c.bias:  # the rows won by a hot class: weights on both sides of key 512
        hot = (r["attn"] > 0) & ((m_all > 0) & (m_all < kept))[..., None]
        assert hot[..., :512].any() and hot[..., 512:].any()


@pytest.fixture(scope="module")
def nat():
    from mx_quantization_amd import _native
    return _native


@pytest.mark.parametrize("c", [c for c in ALL if c.T <= 512], ids=EC.case_id)
def test_cases_reach_their_kernel(nat, c):
    """the dispatch (mxa_attention_finish_kernel makes no GPU call): each case of at most 512
    keys names the finishing kernel it runs on; longer rows have the 16-row kernel's LONG
    variant alone (mxa_attention_long refuses k > 64)"""
    p = nat.AttnParams()
    p.q = p.k = p.v = p.out = 16  # non-null placeholders: nothing is launched
    p.B, p.H, p.N, p.T, p.D, p.k_top = c.B, c.H, c.N, c.T, c.D, c.k
    kw = dict(c.kw)
    p.pred_mode, p.top_k, p.approx, p.scale = nat.PRED_MODES[kw.get("pred_mode", "ex_pred")], int(c.k > 0), int(
        c.k > 0 and kw.get("approx", True)), EC.SCALE
    p.bfloat = kw.get("bfloat", 0)
    if c.bias:
        p.bias = 16
    assert nat.lib().mxa_attention_finish_kernel(ctypes.byref(p)) == c.kind


def test_long_cases_are_the_16_row_kernels():
    for c in ALL:
        if c.T > 512:
            assert c.kind == EC.GATHER16 and 0 < c.k <= 64 and c.T <= 1024
    c = EC.CHUNK32
    assert c.B * c.H * ((c.N + 31) // 32) >= 2048  # mxa_sel_long.hip: rows_per_wg = 32
