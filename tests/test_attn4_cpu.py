"""The MXINT4 attention core (mxa_attention_bits and its siblings), the part that needs no GPU:
the oracle's attention at elem="int4" against the reference's fixture at a_elem_format = "int4", the
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
    _check(O.attention(q, k, v, sc, 20, mode, elem="int4"), gold, f"self/{mode}_k20", "self/true")


def test_attention4_vs_reference_true_topk_and_dense(gold):
    q, k, v, sc = gold["self/q"], gold["self/k"], gold["self/v"], float(gold["self/scale"])
    _check(O.attention(q, k, v, sc, 30, approx=False, elem="int4"), gold, "self/trueK_k30", "self/true")
    _check(O.attention(q, k, v, sc, top_k=False, elem="int4"), gold, "self/dense", "self/true")


@pytest.mark.parametrize("mode", ["ex_pred", "MXINT4"])
def test_attention4_vs_reference_cross(gold, mode):
    """the PixArt cross-attention slice: mask bias, flush, bfloat = 16"""
    q, k, v, sc = gold["cross/q"], gold["cross/k"], gold["cross/v"], float(gold["cross/scale"])
    bias = gold["cross/bias"][:, None]  # (B, 1, 1, T)
    kw = dict(bias=bias, flush=True, bfloat=16)
    _check(O.attention(q, k, v, sc, 20, mode, elem="int4", **kw), gold, f"cross/{mode}_k20", "cross/true")
    if mode == "ex_pred":
        _check(O.attention(q, k, v, sc, top_k=False, elem="int4", **kw), gold, "cross/dense", "cross/true")


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


# ---- the exact-result cases at 4 bits (exact_out_cases.CONDITIONS) --------------
def _exact4(c):
    return c, A.exact_inputs(c), A.exact_reference(c), "int4"


@pytest.mark.parametrize("c", A.EXACT, ids=EC.case_id)
def test_exact4_operands_are_their_own_mxint4(c):
    EC.operands_are_their_own_mx(*_exact4(c))


@pytest.mark.parametrize("c", A.EXACT, ids=EC.case_id)
def test_exact4_score_gaps_are_zero_or_wide(c):
    EC.score_gaps_are_zero_or_wide(*_exact4(c))


@pytest.mark.parametrize("c", A.EXACT, ids=EC.case_id)
def test_exact4_out_is_the_exact_product(c):
    EC.out_is_the_exact_product(*_exact4(c))


@pytest.mark.parametrize("c", A.EXACT, ids=EC.case_id)
def test_exact4_p_codes_survive_four_ulp(c):
    EC.p_codes_survive_four_ulp(*_exact4(c))


@pytest.mark.parametrize("c", A.EXACT, ids=EC.case_id)
def test_exact4_tie_counts_vary(c):
    EC.tie_counts_vary(*_exact4(c))


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
    assert A.shares_within_caps(O.attention(q, kk, v, sc, elem="int4", **kw), v)[0]


def test_bf16_cases_have_no_eligible_block(gold):
    """the bfloat = 16 cases test_gpu_attn4.py checks by the norm: the random one has no P block
    whose codes could differ between two correct softmaxes (attn4_cases.eligible_bf16); the
    fixture's cross-attention slice is checked on the rows without one, nearly all of them"""
    c = A.BF16
    assert A.eligible_bf16(A.r_reference(c), A.r_inputs(c)[2], c.flush)[0] == 0
    q, k, v, sc = gold["cross/q"], gold["cross/k"], gold["cross/v"], float(gold["cross/scale"])
    for kw in (dict(k_top=20, pred_mode="ex_pred"), dict(k_top=20, pred_mode="MXINT4"), dict(top_k=False)):
        r = O.attention(q, k, v, sc, bias=gold["cross/bias"][:, None], flush=True, bfloat=16, elem="int4", **kw)
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
