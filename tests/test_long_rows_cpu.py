"""Rows of 513 .. 1,024 keys (mxa_attention_long and its siblings), the part that needs no GPU:
the oracle against the reference's fixture, the entry points' refusals and LDS plans (host
logic that returns before any HIP call), the workspace size, and the conditions the GPU tests
of test_gpu_long_rows.py rely on."""
import ctypes

import numpy as np
import pytest

import topk_cases as TC
from gpu_support import OUT_TOL, host_params, load, same
from oracle import mx_oracle as O

MODES = ["ex_pred", "partial_Q", "partial_K", "MXINT4", "two_step_leading_ones", "true_ex", "ELSA"]
UNSUPPORTED, WORKSPACE = -2, -4


@pytest.fixture(scope="module")
def nat():
    from mx_quantization_amd import _native
    return _native


@pytest.mark.parametrize("mode", ["ex_pred", "MXINT4"])
def test_oracle_vs_reference_long_rows(mode):
    """The CPU oracle on the reference's 1,000-key rows: true, pred and idx bit-exact."""
    d = load("attn_long.npz")
    r = O.attention(d["q"], d["k"], d["v"], float(d["scale"]), k_top=int(d["k_top"]), pred_mode=mode)
    same(r["true"], d["true"], "true")
    same(r["pred"], d[f"{mode}/pred"], "pred")
    same(r["idx"], d[f"{mode}/idx"].astype(np.int64), "idx")
    assert O.normwise_rel_err(r["out"], d[f"{mode}/out"]) <= OUT_TOL


def test_long_entry_points_refuse_before_any_launch(nat):
    lib = nat.lib()
    long_ = lambda p: lib.mxa_attention_long(ctypes.byref(p), None)
    assert long_(host_params(nat, 1, 1, 10, 1025, 64, 5)) == UNSUPPORTED            # T > 1,024
    assert long_(host_params(nat, 1, 1, 10, 600, 64, 5, top_k=0)) == UNSUPPORTED    # the dense branch
    assert long_(host_params(nat, 1, 1, 10, 600, 64, 65)) == UNSUPPORTED            # k > 64
    for field in ("dtype", "score_dtype"):                                      # float16 tensors / autocast
        p = host_params(nat, 1, 1, 10, 600, 64, 5)
        setattr(p, field, nat.DT_F16)
        assert long_(p) == UNSUPPORTED, field
    p = host_params(nat, 1, 1, 10, 1025, 64, 5)
    p.pred_out = 16
    assert lib.mxa_approx_scores_long(ctypes.byref(p), None) == UNSUPPORTED
    # the short entry points keep their rule
    p = host_params(nat, 1, 1, 10, 600, 64, 5)
    p.pred_out = 16
    assert lib.mxa_attention(ctypes.byref(p), None) == UNSUPPORTED
    assert lib.mxa_approx_scores(ctypes.byref(p), None) == UNSUPPORTED
    assert lib.mxa_attention_path(ctypes.byref(p)) == UNSUPPORTED
    # ... and the long ones take the call as far as its (absent) workspace
    assert long_(p) == WORKSPACE
    assert lib.mxa_approx_scores_long(ctypes.byref(p), None) == WORKSPACE


@pytest.mark.parametrize("mode", MODES)
def test_every_supported_combination_has_a_plan(nat, mode):
    """The LDS plans of the selection and finishing kernels run before the workspace check and
    make no GPU call: a null workspace is refused with MXA_ERR_WORKSPACE, not
    MXA_ERR_UNSUPPORTED, so every combination fits the 160 KB."""
    lib = nat.lib()
    for D in (32, 64, 72, 128):
        for T in (513, 1000, 1024):
            for k in (5, 20, 64):
                p = host_params(nat, 2, 16, T, T, D, k, mode)
                assert lib.mxa_attention_long(ctypes.byref(p), None) == WORKSPACE, (mode, D, T, k)
                p.approx = 0  # top-k on the true scores
                assert lib.mxa_attention_long(ctypes.byref(p), None) == WORKSPACE, (mode, D, T, k, "approx=0")


def test_long_workspace_bytes(nat):
    lib = nat.lib()
    p = host_params(nat, 256, 12, 197, 197, 64, 20)
    assert lib.mxa_attention_long_workspace_bytes(ctypes.byref(p)) == lib.mxa_attention_workspace_bytes(ctypes.byref(p))
    # PixArt 512x512 self-attention, ex_pred.  Per head: Q, K codes + exponents (true and
    # approximate) + sign words (2 x 1024 x (96 + 6 + 6 + 12) B), V^T codes + exponents
    # (72 x 1024 + 32 x 72 x 2 B), the 16-bit kept indices (1024 x 20 x 2 B); no tail
    # records, flags or mask words (those belong to rows of <= 256 keys); 11 regions, each
    # rounded up to 256 B
    p = host_params(nat, 2, 16, 1024, 1024, 72, 20)
    per_head = 2 * 1024 * (96 + 6 + 6 + 12) + 72 * 1024 + 32 * 72 * 2 + 1024 * 20 * 2
    nbytes = lib.mxa_attention_long_workspace_bytes(ctypes.byref(p))
    assert 32 * per_head <= nbytes < 32 * per_head + 12 * 256
    assert lib.mxa_attention_long_workspace_bytes(None) == -1


# ---- what the GPU tests rely on ---------------------------------------------------------------
@pytest.mark.parametrize("n,k", [(513, 20), (1000, 20), (1024, 17), (1024, 33), (1000, 64)])
def test_adversary_rows_reach_the_depth_limit(n, k):
    assert k * 64 > n  # introselect, not partial_sort
    p = O.introselect_probe(O.antiqsort_row(n, k, high=True), k)
    assert p["depth_limit"] and p["l"] - p["f"] > 3, p


@pytest.mark.parametrize("T,k", [(1024, 20), (1000, 33), (600, 5)])
def test_fused_adversary_scores_follow_the_rank(T, k):
    """topk_cases.fused_inputs on long rows: rank // 33 <= 31 fits block 1's 32 positions, so an
    adversarial query's ex_pred scores rise strictly with the adversary row's rank."""
    q, kk, _, rank, qrows = TC.fused_inputs(T, k)
    assert rank.max() // 33 <= 31
    aq, ak = O.approx_operands(q[:, :1], kk[:, :1], "ex_pred")
    pred = O.exact_matmul_f32(aq, np.swapaxes(ak, -1, -2))
    for r in qrows:
        same(np.argsort(np.argsort(pred[0, 0, r], kind="stable"), kind="stable"), rank, "score order")


def test_random_expred_rows_are_full_of_ties():
    """standard_normal inputs: an ex_pred row of 1,000 keys holds hundreds of duplicated values,
    so the order test on random rows is a test of torch's tie order."""
    rng = np.random.default_rng(72 * 1000 + 1000)
    q = rng.standard_normal((1, 1, 20, 72), dtype=np.float32)
    kk = rng.standard_normal((1, 1, 1000, 72), dtype=np.float32)
    aq, ak = O.approx_operands(q, kk, "ex_pred")
    pred = O.exact_matmul_f32(aq, np.swapaxes(ak, -1, -2))[0, 0]
    dup = [1000 - len(np.unique(row)) for row in pred]
    assert min(dup) >= 300, dup
