"""The MXINT4 attention core (mxa_attention_bits and its siblings), the part that needs no GPU:
attention4 (tests/attn4_cases.py) against the reference's fixture at a_elem_format = "int4", the
new entry points' bindings and refusals (host logic that returns before any HIP call), the
conditions of the exact-result cases at this width, and the eligible-share caps of every case
test_gpu_attn4.py bounds row by row."""
import ctypes

import numpy as np
import pytest

import attn4_cases as A
import exact_out_cases as EC
from gpu_support import ELIGIBLE_ELEMS, ELIGIBLE_ROWS, OUT_TOL, host_params, load, same, same_bits
from oracle import mx_oracle as O

ARG, UNSUPPORTED, WORKSPACE = -1, -2, -4
NEW = ("mxa_attention_bits_workspace_bytes", "mxa_attention_bits", "mxa_approx_scores_bits", "mxa_approx_values_bits")


@pytest.fixture(scope="module")
def nat():
    from mx_quantization_amd import _native
    return _native


@pytest.fixture(scope="module")
def gold():
    return load("attn_int4.npz")


# ---- the restated glue against the reference --------------------------------------------------
def _check(r, g, tag, true_key):
    same_bits(r["true"], g[true_key], f"{tag} true")
    for kk in ("pred", "aq", "ak", "idx"):
        if f"{tag}/{kk}" in g:
            ref = g[f"{tag}/{kk}"]
            if kk == "idx":
                same(r[kk], ref.astype(np.int64), f"{tag} idx")
            else:
                same_bits(r[kk][..., :32, :] if kk in ("aq", "ak") else r[kk], ref, f"{tag} {kk}")
    err = O.normwise_rel_err(r["out"], g[f"{tag}/out"])
    print(f"{tag}: out normwise {err:.3e}")
    assert err <= OUT_TOL


@pytest.mark.parametrize("mode", A.MODES)
def test_attention4_vs_reference_self(gold, mode):
    q, k, v, sc = gold["self/q"], gold["self/k"], gold["self/v"], float(gold["self/scale"])
    _check(A.attention4(q, k, v, sc, 20, mode), gold, f"self/{mode}_k20", "self/true")


def test_attention4_vs_reference_true_topk_and_dense(gold):
    q, k, v, sc = gold["self/q"], gold["self/k"], gold["self/v"], float(gold["self/scale"])
    _check(A.attention4(q, k, v, sc, 30, approx=False), gold, "self/trueK_k30", "self/true")
    _check(A.attention4(q, k, v, sc, top_k=False), gold, "self/dense", "self/true")


@pytest.mark.parametrize("mode", ["ex_pred", "MXINT4"])
def test_attention4_vs_reference_cross(gold, mode):
    """the PixArt cross-attention slice: mask bias, flush, bfloat = 16"""
    q, k, v, sc = gold["cross/q"], gold["cross/k"], gold["cross/v"], float(gold["cross/scale"])
    bias = gold["cross/bias"][:, None]  # (B, 1, 1, T)
    kw = dict(bias=bias, flush=True, bfloat=16)
    _check(A.attention4(q, k, v, sc, 20, mode, **kw), gold, f"cross/{mode}_k20", "cross/true")
    if mode == "ex_pred":
        _check(A.attention4(q, k, v, sc, top_k=False, **kw), gold, "cross/dense", "cross/true")


def test_int4_operands_differ_from_int8_ones(gold):
    """what the drop-in got wrong at a_elem_format = "int4": the sign, EXION and true_ex operands
    of the MXINT4 tensor are not those of the MXINT8 one (an element that rounds to the int4
    code 0 has the sign "+")"""
    q, k = gold["self/q"], gold["self/k"]
    for mode in ("ex_pred", "two_step_leading_ones", "true_ex"):
        a8 = O.approx_operands(q, k, mode)[0]
        assert (a8[..., :32, :] != gold[f"self/{mode}_k20/aq"]).any(), mode


# ---- the ABI ----------------------------------------------------------------------------------
def test_exports_sigs_and_abi_version(nat):
    import subprocess
    from test_boundary_cpu import _ctype_of_decl, _header_params
    hdr = _header_params()
    syms = subprocess.run(["nm", "-D", "--defined-only", nat.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for fn in NEW:
        assert fn in hdr and fn in nat._SIGS and fn in nat.EXPORTS and f" T {fn}\n" in syms, fn
        norm = lambda t: ctypes.c_void_p if isinstance(t, type) and issubclass(t, ctypes._Pointer) else t
        assert [norm(t) for t in nat._SIGS[fn][1]] == [_ctype_of_decl(d) for d in hdr[fn]], fn
    assert nat.ABI_VERSION == 6 and nat.lib().mxa_abi_version() == 6


def test_bits_entry_points_refuse_before_any_launch(nat):
    lib = nat.lib()
    bits = lambda p, w=4: lib.mxa_attention_bits(ctypes.byref(p), w, None)
    ok = host_params(nat, 1, 1, 10, 70, 64, 5)
    ok.pred_out = 16
    for w in (3, 0, 16, -4):
        assert bits(ok, w) == ARG, w
        assert lib.mxa_approx_scores_bits(ctypes.byref(ok), w, None) == ARG, w
        assert lib.mxa_attention_bits_workspace_bytes(ctypes.byref(ok), w) == -1, w
        assert lib.mxa_approx_values_bits(16, 16, 4, 32, 32, 32, 0, 0, 0, 0, w, None) == ARG, w
    assert bits(ok) == WORKSPACE and lib.mxa_approx_scores_bits(ctypes.byref(ok), 4, None) == WORKSPACE
    assert bits(host_params(nat, 1, 1, 70, 70, 64, 5, "ELSA")) == UNSUPPORTED
    for field in ("dtype", "score_dtype"):
        p = host_params(nat, 1, 1, 10, 70, 64, 5)
        setattr(p, field, nat.DT_F16)
        assert bits(p) == UNSUPPORTED, field
    assert bits(host_params(nat, 1, 1, 10, 300, 64, 65)) == UNSUPPORTED            # finish_kernel
    assert bits(host_params(nat, 1, 1, 10, 300, 64, 0, top_k=0)) == UNSUPPORTED    # dense_rows_kernel
    assert bits(host_params(nat, 1, 1, 10, 1025, 64, 5)) == UNSUPPORTED            # T > 1,024
    p = host_params(nat, 1, 1, 10, 1025, 64, 5)
    p.pred_out = 16
    assert lib.mxa_approx_scores_bits(ctypes.byref(p), 4, None) == UNSUPPORTED
    # the scores alone have no finishing kernel: any T <= 1,024
    p = host_params(nat, 1, 1, 10, 300, 64, 0, top_k=0)
    p.pred_out = 16
    assert lib.mxa_approx_scores_bits(ctypes.byref(p), 4, None) == WORKSPACE
    # approx_values_bits validates like approx_values
    assert lib.mxa_approx_values_bits(None, 16, 4, 32, 32, 32, 0, 0, 0, 0, 4, None) == ARG
    assert lib.mxa_approx_values_bits(16, 16, 4, 32, 32, 32, 5, 0, 0, 0, 4, None) == ARG
    assert lib.mxa_approx_values_bits(16, 16, 0, 32, 32, 32, 0, 0, 0, 0, 4, None) == 0  # no rows: nothing to do


@pytest.mark.parametrize("mode", A.MODES)
def test_every_supported_combination_has_a_plan(nat, mode):
    """a null workspace is refused with MXA_ERR_WORKSPACE, after the LDS plans of the selection
    and finishing kernels (no GPU call): every supported combination fits"""
    lib = nat.lib()
    for D in (32, 64, 72, 128):
        for T in (70, 256, 513, 1024):
            ks = (5, 20, 64) + ((65, 0) if T <= 256 else ())
            for k in ks:
                p = host_params(nat, 2, 16, T, T, D, k, mode, top_k=int(k > 0))
                assert lib.mxa_attention_bits(ctypes.byref(p), 4, None) == WORKSPACE, (mode, D, T, k)
                p.approx = 0
                assert lib.mxa_attention_bits(ctypes.byref(p), 4, None) == WORKSPACE, (mode, D, T, k, "approx=0")
                p.bias, p.bfloat, p.flush_subnormals = 16, 16, 1
                assert lib.mxa_attention_bits(ctypes.byref(p), 4, None) == WORKSPACE, (mode, D, T, k, "extra")


def test_width_8_is_the_long_entry_point(nat):
    lib = nat.lib()
    cases = [host_params(nat, 2, 3, 70, 70, 64, 20), host_params(nat, 1, 1, 10, 600, 64, 5), host_params(nat, 1, 1, 10, 600, 64, 65),
             host_params(nat, 1, 1, 10, 1025, 64, 5), host_params(nat, 1, 2, 40, 300, 72, 0, top_k=0),
             host_params(nat, 1, 1, 70, 70, 64, 5, "ELSA"), host_params(nat, 1, 1, 10, 70, 200, 5)]
    f16 = host_params(nat, 1, 1, 10, 70, 64, 5)
    f16.dtype = nat.DT_F16
    for p in cases + [f16]:
        assert lib.mxa_attention_bits(ctypes.byref(p), 8, None) == lib.mxa_attention_long(ctypes.byref(p), None)
        p.pred_out = 16
        assert lib.mxa_approx_scores_bits(ctypes.byref(p), 8, None) == lib.mxa_approx_scores_long(ctypes.byref(p), None)
        for w in (8, 4):  # codes stay one byte each: one size
            assert lib.mxa_attention_bits_workspace_bytes(ctypes.byref(p), w) == lib.mxa_attention_long_workspace_bytes(
                ctypes.byref(p))
    assert lib.mxa_attention_bits_workspace_bytes(None, 4) == -1


def test_ops_refuse_other_widths():
    """elem_bits is checked before anything touches a device"""
    import torch
    import mx_quantization_amd as M
    x = torch.zeros(1, 1, 4, 32)
    for w in (3, 16, 0, "4"):
        with pytest.raises(ValueError):
            M.mx_topk_attention(x, x, x, 1.0, 2, elem_bits=w)
        with pytest.raises(ValueError):
            M.mx_approx_scores(x, x, elem_bits=w)
        with pytest.raises(ValueError):
            M.ops.approx_values(x, "sign", elem_bits=w)


# ---- the exact-result cases at 4 bits (the five conditions of test_exact_out_cpu.py) --------------
def _bf(c):
    return dict(c.kw).get("bfloat", 32)


def _finite_rows(r):
    return ~np.isnan(r["attn"]).any(-1)


@pytest.mark.parametrize("c", A.EXACT, ids=EC.case_id)
def test_exact4_operands_are_their_own_mxint4(c):
    """q and k are their own MXINT4 along D, v along the tokens (integers |n| <= 7 times 2^e)"""
    q, k, v, _ = A.exact_inputs(c)
    same_bits(O.quantize_mx(O.quantize_bfloat(q, _bf(c)), "int4", 32, -1)[0], q, "MX4(q)")
    same_bits(O.quantize_mx(O.quantize_bfloat(k, _bf(c)), "int4", 32, -1)[0], k, "MX4(k)")
    same_bits(O.quantize_mx(O.quantize_bfloat(v, _bf(c)), "int4", 32, -2)[0], v, "MX4(v)")
    assert (v == np.round(v)).all() and np.abs(v).max() <= 7 * 8


@pytest.mark.parametrize("c", A.EXACT, ids=EC.case_id)
def test_exact4_score_gaps_are_zero_or_wide(c):
    r = A.exact_reference(c)
    t = np.sort(r["true"].astype(np.float64), axis=-1)
    fin = np.isfinite(t).all(-1)
    assert fin.sum() >= fin.size - (c.H if c.bias else 0) and fin.any()
    gap = np.diff(t[fin], axis=-1)
    assert ((gap == 0) | (gap >= 150)).all(), gap[(gap != 0) & (gap < 150)][:4]
    assert (gap >= 150).any(-1).all()


@pytest.mark.parametrize("c", A.EXACT, ids=EC.case_id)
def test_exact4_out_is_the_exact_product(c):
    """out equals the float64 product of the MXINT4 operands, that product is a float32, and the
    per-element sum of |Pq| |Vq| is below 2^24 granules (the code step 2^(e - 2) of the row's
    lowest non-zero P block): every partial sum in every order is exact in float32"""
    (_, _, v, _), r = A.exact_inputs(c), A.exact_reference(c)
    fin = _finite_rows(r)
    pq, _, pe = O.quantize_mx(O.quantize_bfloat(r["attn"], _bf(c)), "int4", 32, -1)
    vq = O.quantize_mx(O.quantize_bfloat(v, _bf(c)), "int4", 32, -2)[0]
    with np.errstate(invalid="ignore"):
        prod = np.matmul(pq.astype(np.float64), vq.astype(np.float64))
        S = np.matmul(np.abs(pq).astype(np.float64), np.abs(vq).astype(np.float64))
    assert (prod[fin] == prod[fin].astype(np.float32)).all()
    same_bits(r["out"][fin], O.quantize_bfloat(prod[fin].astype(np.float32), _bf(c)), "out vs the exact product")
    assert np.isnan(r["out"][~fin]).all()
    blk, _ = O.to_blocks(pq, -1, 32)
    e = np.where((blk != 0).any(-1), pe[..., 0], np.inf)
    gran = np.exp2(e.min(-1) - 2)[fin]
    assert np.isfinite(gran).all()
    assert (pq[fin] / gran[:, None] == np.round(pq[fin] / gran[:, None])).all()
    assert (S[fin] / gran[:, None]).max() < 2 ** 24


@pytest.mark.parametrize("c", A.EXACT, ids=EC.case_id)
def test_exact4_p_codes_survive_four_ulp(c):
    """every non-zero p moved by 4 ulp either way keeps the MXINT4 codes of P: p = 1/m lies
    4 ulp inside a cell of the 4-bit grid, floor(p 2^(2 - e) + 1/2) with the clip at 7 (m = 65,
    129: y = 7.9 clips from either side).  Rows whose m is a power of two are exempt, as at 8 bits."""
    r = A.exact_reference(c)
    m, _ = EC.tied(c, r)
    rows = (m > 0) & ((m & (m - 1)) != 0)
    assert rows.any() or c.k == 1
    a = r["attn"][rows]
    codes = O.quantize_mx(O.quantize_bfloat(a, _bf(c)), "int4", 32, -1)[1]
    for d in (-4, 4):
        b = a.copy().view(np.int32)
        b[a != 0] += d
        same(O.quantize_mx(O.quantize_bfloat(b.view(np.float32), _bf(c)), "int4", 32, -1)[1], codes, f"P codes at {d} ulp")


@pytest.mark.parametrize("c", A.EXACT, ids=EC.case_id)
def test_exact4_tie_counts_vary(c):
    r = A.exact_reference(c)
    m_all, kept = EC.tied(c, r)
    m = m_all[m_all > 0]
    if c.k == 1:
        assert (m == 1).all()
    elif c.k:
        assert (m < kept).any() and (m >= kept).any(), np.unique(m)
        assert (np.take_along_axis(r["attn"], r["idx"], -1)[_finite_rows(r)] == 0).any()  # a kept slot of zero weight
    else:
        assert len(np.unique(m)) >= 3, np.unique(m)


def test_exact4_cases_cover_the_kernels():
    kinds = {(c.kind, c.T > 512) for c in A.EXACT}
    assert kinds == {(EC.GATHER16, False), (EC.GATHER16, True), (EC.MFMA, False), (EC.DENSE_MFMA, False)}
    for c in A.EXACT:  # what mxa_attention_bits supports at width 4
        assert c.T <= 1024 and (c.T <= 256 or 0 < c.k <= 64)


# ---- the random GPU cases: the eligible shares, from the oracle alone ---------------------------
@pytest.mark.parametrize("c", A.ROWS_CASES, ids=A.rcase_id)
def test_eligible_shares_within_caps(c):
    ok, (se, sr) = A.shares_within_caps(A.r_reference(c), A.r_inputs(c)[2])
    print(f"{A.rcase_id(c)}: eligible elements {se:.4%} rows {sr:.2%}")
    assert ok and se <= ELIGIBLE_ELEMS and sr <= ELIGIBLE_ROWS


@pytest.mark.parametrize("mode", ["ex_pred", "two_step_leading_ones", "MXINT4"])
def test_special_case_eligible_shares(mode):
    r = A.special_reference(mode)
    ok, shares = A.shares_within_caps(r, A.special_inputs()[2])
    fin = np.isfinite(r["out"]).all(-1)
    print(mode, shares, "finite rows", int(fin.sum()), "of", fin.size)
    assert ok and fin.any() and not fin.all()


@pytest.mark.parametrize("tag,k", [(f"self/{m}_k20", 20) for m in A.MODES] + [("self/trueK_k30", 30), ("self/dense", 0)])
def test_fixture_cases_eligible_shares(gold, tag, k):
    q, kk, v, sc = gold["self/q"], gold["self/k"], gold["self/v"], float(gold["self/scale"])
    mode = tag.split("/")[1].rsplit("_k", 1)[0]
    kw = dict(top_k=False) if not k else (dict(k_top=k, approx=False) if mode == "trueK" else dict(k_top=k, pred_mode=mode))
    assert A.shares_within_caps(A.attention4(q, kk, v, sc, **kw), v)[0]


def test_bf16_cases_have_no_eligible_block(gold):
    """the bfloat = 16 cases test_gpu_attn4.py checks by the norm: the random one has no P block
    whose codes could differ between two correct softmaxes (attn4_cases.eligible_bf16); the
    fixture's cross-attention slice is checked on the rows without one, nearly all of them"""
    c = A.BF16
    assert A.eligible_bf16(A.r_reference(c), A.r_inputs(c)[2], c.flush)[0] == 0
    q, k, v, sc = gold["cross/q"], gold["cross/k"], gold["cross/v"], float(gold["cross/scale"])
    for kw in (dict(k_top=20, pred_mode="ex_pred"), dict(k_top=20, pred_mode="MXINT4"), dict(top_k=False)):
        r = A.attention4(q, k, v, sc, bias=gold["cross/bias"][:, None], flush=True, bfloat=16, **kw)
        rows = A.eligible_bf16(r, v, True)[2]
        print(kw, "rows with an eligible block:", int(rows.sum()), "of", rows.size)
        assert rows.mean() <= 0.02, kw


def test_eligible_bf16_sees_a_midpoint():
    """a p one float32 ulp from a bfloat16 midpoint whose two neighbours code differently is found"""
    attn = np.zeros((1, 1, 1, 32), np.float32)
    attn[..., 0] = 0.5                                   # the block maximum: es = -1, step 2^-3
    attn[..., 1] = np.float32(0.1875 - 2.0 ** -11) + np.float32(2.0 ** -26)  # an ulp above the midpoint below 1.5 steps
    r = dict(attn=attn, true=np.zeros_like(attn), idx=np.arange(20)[None, None, None])
    n, near, rows = A.eligible_bf16(r, np.zeros((1, 1, 32, 64), np.float32))
    assert near == 1 and n == 1 and rows.all()
