"""The conditions under which the attention output of tests/exact_out_cases.py is the only
float32 result a correct implementation can produce (exact_out_cases.CONDITIONS), proved per case
with the oracle alone.  The GPU file (test_gpu_exact_out.py) parametrizes over the same list
objects and only compares bits."""
import ctypes

import pytest

import exact_out_cases as EC

ALL = EC.CASES + [EC.CHUNK32]


def _ref(c):
    heads = (1, 1) if c is EC.CHUNK32 else None
    return EC.inputs(c, heads), EC.reference(c, heads)


@pytest.mark.parametrize("c", ALL, ids=EC.case_id)
def test_score_gaps_are_zero_or_wide(c):
    EC.score_gaps_are_zero_or_wide(c, *_ref(c), "int8")


@pytest.mark.parametrize("c", ALL, ids=EC.case_id)
def test_v_is_its_own_mx_along_the_tokens(c):
    EC.operands_are_their_own_mx(c, *_ref(c), "int8")


@pytest.mark.parametrize("c", ALL, ids=EC.case_id)
def test_out_is_the_exact_product(c):
    EC.out_is_the_exact_product(c, *_ref(c), "int8")


@pytest.mark.parametrize("c", ALL, ids=EC.case_id)
def test_p_codes_survive_four_ulp(c):
    EC.p_codes_survive_four_ulp(c, *_ref(c), "int8")


@pytest.mark.parametrize("c", ALL, ids=EC.case_id)
def test_tie_counts_vary(c):
    EC.tie_counts_vary(c, *_ref(c), "int8")


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
