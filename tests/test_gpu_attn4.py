"""The MXINT4 attention core on the device (mx_topk_attention / mx_approx_scores / approx_values
with elem_bits=4: mxa_attention_bits and its siblings) against the reference's fixture at
a_elem_format = "int4" and against the oracle's attention at elem="int4": true and approximate
scores, kept indices and mask words bit for bit; out bit for bit on the exact-result cases, by
the row-wise bound at width 4 elsewhere, by the norm on the bfloat = 16 rows that
test_attn4_cpu.py shows to have no eligible P block.  The references are computed once in
attn4_cases.py and shared with the CPU file, which asserts the eligible-share caps from the oracle
alone."""
import collections

import numpy as np
import pytest
import torch

import attn4_cases as A
import exact_out_cases as EC
from gpu_support import M, OUT_TOL, attn_run, check_attn, check_exact_out, check_siblings, dev, host, load  # noqa: F401
from gpu_support import out_close, out_rows_close, r_kw, r_scale, rnd, same, same_bits
from oracle import mx_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold():
    return load("attn_int4.npz")


# what _run reads of an RCase, for the calls that are none: k = 0 dense; mode None: approx=False (r_kw)
Call = collections.namedtuple("Call", "k mode flush bfloat", defaults=(False, 32))


def _run(M, q, k, v, scale, c, bias=None, scores=True):
    """attn_run at elem_bits=4 for an RCase or a Call"""
    return attn_run(M, q, k, v, scale, 4, scores, bias=bias, flush_subnormals=c.flush, bfloat=0 if c.bfloat == 32 else c.bfloat,
                    **r_kw(c))


# ---- the reference's fixture --------------------------------------------------------------------
FIXTURE = [(f"{m}_k20", 20, m) for m in A.MODES] + [("trueK_k30", 30, None), ("dense", 0, "ex_pred")]


@pytest.mark.parametrize("tag,k,mode", FIXTURE, ids=[f[0] for f in FIXTURE])
def test_fixture_self(M, gold, tag, k, mode):
    q, kk, v, sc = gold["self/q"], gold["self/k"], gold["self/v"], float(gold["self/scale"])
    kw = dict(top_k=False) if not k else (dict(k_top=k, approx=False) if mode is None else dict(k_top=k, pred_mode=mode))
    r = O.attention(q, kk, v, sc, elem="int4", **kw)  # (test_attn4_cpu.py: equal to the fixture bit for bit)
    if k:
        same(r["idx"], gold[f"self/{tag}/idx"].astype(np.int64), "oracle idx vs fixture")
    got = _run(M, q, kk, v, sc, Call(k, mode))
    same_bits(got["true"], gold["self/true"], tag + " true vs fixture")
    if k and mode is not None:
        same_bits(got["pred"], gold[f"self/{tag}/pred"], tag + " pred vs fixture")
    check_attn(got, r, tag, same_bits)
    out_rows_close(got["out"], dict(r, out=gold[f"self/{tag}/out"]), v, tag, bits=4)


@pytest.mark.parametrize("tag,k,mode", [("ex_pred_k20", 20, "ex_pred"), ("MXINT4_k20", 20, "MXINT4"), ("dense", 0, "ex_pred")])
def test_fixture_cross_bf16(M, gold, tag, k, mode):
    """the PixArt cross slice: mask bias, flush, bfloat = 16; out by the norm on the rows without
    an eligible P block (attn4_cases.eligible_bf16; at most 2 % of the rows have one)"""
    q, kk, v, sc = gold["cross/q"], gold["cross/k"], gold["cross/v"], float(gold["cross/scale"])
    bias = gold["cross/bias"][:, None]
    kw = dict(k_top=k, pred_mode=mode) if k else dict(top_k=False)
    r = O.attention(q, kk, v, sc, bias=bias, flush=True, bfloat=16, elem="int4", **kw)
    rows = ~A.eligible_bf16(r, v, True)[2]
    got = _run(M, q, kk, v, sc, Call(k, mode, True, 16), bias)
    same_bits(got["true"], gold["cross/true"], tag + " true vs fixture")
    if k:
        same_bits(got["pred"], gold[f"cross/{tag}/pred"], tag + " pred vs fixture")
        same(got["idx"], gold[f"cross/{tag}/idx"].astype(np.int64), tag + " idx vs fixture")
    check_attn(got, r, tag, same_bits)
    out_close(got["out"][rows], gold[f"cross/{tag}/out"][rows], OUT_TOL, tag + " out")


# ---- the grid, the long rows and finish_qk_kernel against the oracle at int4 ---------------------------------
@pytest.mark.parametrize("c", A.ROWS_CASES, ids=A.rcase_id)
def test_rows_vs_attention4(M, c):
    q, k, v, bias = A.r_inputs(c)
    r = A.r_reference(c)
    tq, tk, tv = dev(q), dev(k), dev(v)
    if c.N == c.T:  # strided views of one packed qkv on the device
        qkv = torch.stack([tq.permute(0, 2, 1, 3), tk.permute(0, 2, 1, 3), tv.permute(0, 2, 1, 3)], 2).contiguous()
        tq, tk, tv = (qkv[:, :, j].permute(0, 2, 1, 3) for j in range(3))
        assert not tq.is_contiguous()
    got = _run(M, tq, tk, tv, r_scale(c), c, bias, c.scores)
    check_attn(got, r, A.rcase_id(c), same_bits)
    out_rows_close(got["out"], r, v, A.rcase_id(c), bits=4)


def test_random_bf16_case_by_the_norm(M):
    c = A.BF16
    q, k, v, bias = A.r_inputs(c)
    r = A.r_reference(c)
    got = _run(M, q, k, v, r_scale(c), c, bias, c.scores)
    check_attn(got, r, "bf16", same_bits)
    out_close(got["out"], r["out"], OUT_TOL, "bf16 out")


def test_approx_scores_bits(M, gold):
    q, kk = gold["self/q"], gold["self/k"]
    for mode in A.MODES:
        pred = M.mx_approx_scores(dev(q), dev(kk), mode, elem_bits=4)
        same_bits(host(pred), gold[f"self/{mode}_k20/pred"], mode)
    c = A.LONG[0]
    q, k, _, _ = A.r_inputs(c)
    same_bits(host(M.mx_approx_scores(dev(q), dev(k), c.mode, elem_bits=4)), A.r_reference(c)["pred"], "long rows")


# ---- exact-result cases: out, idx and mask bit for bit ------------------------------------------------
@pytest.mark.parametrize("c", A.EXACT, ids=EC.case_id)
def test_exact_out4(M, c):
    check_exact_out(M, c, A.exact_inputs(c), A.exact_reference(c), EC.SCALE, 4, EC.case_id(c))


# ---- special blocks ------------------------------------------------------------------------------
def test_special_blocks_operands(M):
    """approx_values(.., elem_bits=4) against ExponentApproximation(elem="int4") bit for bit, -0.0
    (a negative element that rounds to the code 0) included"""
    q, k, _ = A.special_inputs()
    ea = O.ExponentApproximation(q, k, 32, elem="int4")
    want = {"sign": ea.exponent_based_sign(), "mxint8": (ea.MX_Q, ea.MX_K), "mxint4": ea.MXINT4(),
            "exion": ea.two_step_leading_ones(), "true_ex": ea.exponent_based_sign_leading_ones()}
    assert (np.signbit(ea.MX_Q) & (ea.MX_Q == 0)).any()  # the fixture holds a -0.0
    for kind, (wq, wk) in want.items():
        same_bits(host(M.ops.approx_values(dev(q), kind, elem_bits=4)), wq, kind + " q")
        same_bits(host(M.ops.approx_values(dev(k), kind, elem_bits=4)), wk, kind + " k")
    # an unaligned view and a ragged row length take the one-lane-per-element kernel
    same_bits(host(M.ops.approx_values(dev(q)[..., 1:71], "exion", elem_bits=4)),
              O.ExponentApproximation(q[..., 1:71], k, 32, elem="int4").two_step_leading_ones()[0], "exion ragged")
    # flush and bfloat
    eb = O.ExponentApproximation(q, k, 32, elem="int4", flush=True, bfloat=16)
    same_bits(host(M.ops.approx_values(dev(q), "sign", flush=True, bfloat=16, elem_bits=4)), eb.exponent_based_sign()[0],
              "sign flush bf16")


@pytest.mark.parametrize("mode", ["ex_pred", "two_step_leading_ones", "MXINT4"])
def test_special_blocks_fused(M, mode):
    """(not true_ex: it maps an element that rounds to the code 0 to +1, 2^100 above the other
    elements of a 2^-100 row, so the float64 sum of such a score is exact in neither the oracle
    nor the device; its operands on these blocks are pinned by test_special_blocks_operands)"""
    q, k, v = A.special_inputs()
    r = A.special_reference(mode)
    got = _run(M, q, k, v, A.SPECIAL_SCALE, Call(A.SPECIAL_K, mode))
    check_attn(got, r, mode, same_bits)  # (idx: NaN scores rank first, in torch's order)
    out_rows_close(got["out"], r, v, mode, bits=4)  # the NaN pattern (a NaN V block poisons its column) and the finite rows


# ---- width 8 through the width-taking entry points ----------------------------------------------------
@pytest.mark.parametrize("T", [70, 600])
def test_width_8_is_byte_identical(M, T):
    """self-attention rows (N = T, two images) at width 8: mxa_attention_bits(p, 8), mxa_attention_full(p, 8),
    mxa_attention_long and (T <= 512) mxa_attention, called directly, and their score entry points"""
    q, k, v = (dev(rnd((2, 2, T, 64), 500 + j)) for j in range(3))
    check_siblings(M, q, k, v, 0.125, (8,), k_top=20)
    assert torch.equal(M.ops.approx_values(q, "sign", elem_bits=8), M.ops.approx_values(q, "sign"))


def test_library_refuses_at_width_4(M):
    q = dev(rnd((1, 2, 70, 64), 510))
    with pytest.raises(M._native.NativeError):
        M.mx_topk_attention(q.half(), q.half(), q.half(), 0.125, 20, elem_bits=4)
    with pytest.raises(M._native.NativeError):
        M.mx_topk_attention(q, q, q, 0.125, 20, autocast=torch.float16, elem_bits=4)
    with pytest.raises(M._native.NativeError):
        M.mx_topk_attention(q, q, q, 0.125, 20, pred_mode="ELSA", elsa_proj=torch.eye(64, device="cuda"), elem_bits=4)


# ---- the drop-in under an int4 spec --------------------------------------------------------------------
def test_dropin_int4_operands_and_matmul(M, gold):
    """exponent_approximation at a_elem_format = "int4": the six operand pairs equal the
    reference's bit for bit (from MXINT8 codes the sign, EXION and true_ex pairs differ);
    mx.matmul(q, k^T) at that spec is the fused call's true score before the scale"""
    M.install_dropin()
    import mx
    from funcs import exponent_approximation
    from mx.specs import apply_mx_specs
    specs = apply_mx_specs({"a_elem_format": "int4", "w_elem_format": "int4", "block_size": 32, "scale_bits": 8, "bfloat": 32})
    q, k, v = dev(gold["self/q"]), dev(gold["self/k"]), dev(gold["self/v"])
    for mode in A.MODES:
        obj = exponent_approximation(q, k, specs)
        fn = {"ex_pred": obj.exponent_based_sign, "true_ex": obj.exponent_based_sign_leading_ones}.get(mode, getattr(obj, mode, None))
        aq, ak = fn()
        same_bits(host(aq)[..., :32, :], gold[f"self/{mode}_k20/aq"], mode + " aq")
        same_bits(host(ak)[..., :32, :], gold[f"self/{mode}_k20/ak"], mode + " ak")
    s = mx.matmul(q, k.transpose(-2, -1), mx_specs=specs, mode_config="aa")
    sc = float(gold["self/scale"])
    true = M.mx_topk_attention(q, k, v, sc, 20, return_scores=True, elem_bits=4)[2]
    same_bits(host(s * sc), host(true), "mx.matmul * scale vs the fused call's true scores")
    same_bits(host(s * sc), gold["self/true"], "... vs the fixture")
