"""The dense branch and k > 64 on rows of 513 .. 1,024 keys (mxa_attention_full and its siblings),
the part that needs no GPU: the exports, the refusals and LDS plans (host logic that returns
before any HIP call), the dispatch report, the workspace size, and the conditions the GPU tests of
test_gpu_long_dense.py rely on -- the exact-result cases' five conditions, the eligible shares of
the row-wise bound on the peaked random inputs, the exact epilogue's branch per special input."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import attn4_cases as A
import exact_out_cases as EC
import long_dense_cases as LC
from gpu_support import ELIGIBLE_ELEMS, ELIGIBLE_ROWS, host_params
from oracle import mx_oracle as O

MODES = ["ex_pred", "partial_Q", "partial_K", "MXINT4", "two_step_leading_ones", "true_ex", "ELSA"]
ARG, UNSUPPORTED, WORKSPACE = -1, -2, -4
NEW = ("mxa_attention_full_workspace_bytes", "mxa_attention_full", "mxa_attention_full_finish_kernel")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def nat():
    from mx_quantization_amd import _native
    return _native


def _full(nat, p, bits=8):
    return nat.lib().mxa_attention_full(ctypes.byref(p), bits, None)


# ---- exports and refusals ---------------------------------------------------------------------------
def test_exports_sigs_and_abi_version(nat):
    header = open(os.path.join(ROOT, "include", "mxa.h")).read()
    syms = subprocess.run(["nm", "-D", "--defined-only", nat.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert name + "(" in header and name in nat._SIGS and name in nat.EXPORTS
        assert f" T {name}\n" in syms, name
    assert "MX_transformer_block.py:704-705" in header and ":700-702" in header
    assert "#define MXA_FIN_MFMA_LONG 6" in header and "#define MXA_FIN_DENSE_MFMA_LONG 7" in header
    assert nat.ABI_VERSION == 6 and nat.lib().mxa_abi_version() == 6 and "#define MXA_ABI_VERSION 6 " in header
    assert set(nat.FIN_KERNELS_FULL) == {LC.MFMA_LONG, LC.DENSE_MFMA_LONG}


def test_full_entry_point_refuses_before_any_launch(nat):
    lib = nat.lib()
    for bits in (8, 4):
        assert _full(nat, host_params(nat, 1, 1, 10, 1025, 64, 5), bits) == UNSUPPORTED           # T > 1,024
        assert _full(nat, host_params(nat, 1, 1, 10, 1025, 64, 0, top_k=0), bits) == UNSUPPORTED
        for k, top_k in ((5, 1), (65, 1), (0, 0)):
            for field in ("dtype", "score_dtype"):                                          # float16 tensors / autocast
                p = host_params(nat, 1, 1, 10, 600, 64, k, top_k=top_k)
                setattr(p, field, nat.DT_F16)
                assert _full(nat, p, bits) == UNSUPPORTED, (bits, k, field)
    for k, top_k in ((5, 1), (65, 1)):                                                      # ELSA at width 4
        assert _full(nat, host_params(nat, 1, 1, 600, 600, 64, k, "ELSA", top_k), 4) == UNSUPPORTED
        assert _full(nat, host_params(nat, 1, 1, 600, 600, 64, k, "ELSA", top_k), 8) == WORKSPACE
    for bits in (0, 2, 16, -4):                                                             # other widths
        p = host_params(nat, 1, 1, 10, 600, 64, 65)
        assert _full(nat, p, bits) == ARG
        assert lib.mxa_attention_full_workspace_bytes(ctypes.byref(p), bits) == -1
        assert lib.mxa_attention_full_finish_kernel(ctypes.byref(p), bits) == ARG
    assert lib.mxa_attention_full_workspace_bytes(None, 8) == -1
    # what mxa_attention_bits refuses at T <= 512 stays refused: the 32-row and the dense row kernel at width 4
    assert _full(nat, host_params(nat, 1, 2, 100, 300, 64, 100), 4) == UNSUPPORTED
    assert _full(nat, host_params(nat, 1, 2, 100, 300, 64, 0, top_k=0), 4) == UNSUPPORTED
    assert _full(nat, host_params(nat, 1, 1, 10, 60, 160, 5), 8) == UNSUPPORTED                  # D > 128
    # mxa_attention_long still refuses the dense branch and k = 65 at T = 600; the new entry point takes
    # the same parameters as far as their (absent) workspace
    for k, top_k in ((5, 0), (65, 1)):
        p = host_params(nat, 1, 1, 10, 600, 64, k, top_k=top_k)
        assert lib.mxa_attention_long(ctypes.byref(p), None) == UNSUPPORTED
        assert lib.mxa_attention_bits(ctypes.byref(p), 8, None) == UNSUPPORTED
        assert lib.mxa_attention_bits(ctypes.byref(p), 4, None) == UNSUPPORTED
        assert _full(nat, p, 8) == WORKSPACE and _full(nat, p, 4) == WORKSPACE
    p = host_params(nat, 1, 1, 10, 600, 64, 601)                                                # k > T
    assert _full(nat, p, 8) == ARG


@pytest.mark.parametrize("mode", MODES)
def test_every_supported_combination_has_a_plan(nat, mode):
    """The LDS plans of the selection and finishing kernels run before the workspace check and make
    no GPU call: a null workspace is refused with MXA_ERR_WORKSPACE, never MXA_ERR_UNSUPPORTED."""
    for bits in (8,) if mode == "ELSA" else (8, 4):
        for D in (32, 64, 72, 128):
            for T in (513, 1000, 1024):
                for k in (0, 65, 154, 512, T):
                    p = host_params(nat, 2, 16, T, T, D, k, mode, top_k=int(k > 0))
                    assert _full(nat, p, bits) == WORKSPACE, (mode, bits, D, T, k)
                    p.approx = 0  # top-k on the true scores
                    assert _full(nat, p, bits) == WORKSPACE, (mode, bits, D, T, k, "approx=0")


def test_dispatch_report(nat):
    lib = nat.lib()
    fk = lambda p, bits=8: lib.mxa_attention_full_finish_kernel(ctypes.byref(p), bits)
    for bits in (8, 4):
        for T in (513, 1000, 1024):
            for k in (65, 154, T):
                assert fk(host_params(nat, 2, 16, T, T, 72, k), bits) == LC.MFMA_LONG == LC.kind_of(T, k)
            assert fk(host_params(nat, 2, 16, T, T, 72, 0, top_k=0), bits) == LC.DENSE_MFMA_LONG == LC.kind_of(T, 0)
            for k in (1, 20, 64):
                assert fk(host_params(nat, 2, 16, T, T, 72, k), bits) == EC.GATHER16 == LC.kind_of(T, k)
    # rows of at most 512 keys: what mxa_attention_finish_kernel reports
    for a, kw in (((256, 12, 197, 197, 64, 20), {}), ((64, 16, 256, 256, 72, 154), {}), ((1, 2, 100, 300, 64, 100), {}),
                  ((256, 12, 197, 197, 64, 20), dict(top_k=0)), ((1, 2, 100, 300, 64, 20), dict(top_k=0)),
                  ((1, 2, 100, 512, 64, 65), {}), ((1, 2, 100, 512, 64, 0), dict(top_k=0))):
        p = host_params(nat, *a, **kw)
        want = lib.mxa_attention_finish_kernel(ctypes.byref(p))
        assert want in (1, 2, 3, 4, 5) and fk(p) == want, (a, kw)
    for c in LC.EXACT + LC.EXACT_BF16 + LC.EXACT4:
        p = host_params(nat, c.B, c.H, c.N, c.T, c.D, c.k, top_k=int(c.k > 0))
        assert fk(p) == LC.kind_of(c.T, c.k) and fk(p, 4) == LC.kind_of(c.T, c.k), LC.case_id(c)


def test_workspace_bytes(nat):
    """equal to mxa_attention_bits_workspace_bytes on the shapes both accept; on the new top-k shapes the
    prune-mask words are added (whatever mask_out is), on the dense ones nothing"""
    lib = nat.lib()
    both = lambda p, bits: (lib.mxa_attention_full_workspace_bytes(ctypes.byref(p), bits),
                            lib.mxa_attention_bits_workspace_bytes(ctypes.byref(p), bits))
    for bits in (8, 4):
        for a, kw in (((256, 12, 197, 197, 64, 20), {}), ((64, 16, 256, 256, 72, 154), {}), ((2, 16, 1024, 1024, 72, 20), {}),
                      ((1, 2, 100, 300, 64, 100), {}), ((1, 2, 77, 120, 72, 0), dict(top_k=0)), ((2, 2, 33, 513, 32, 64), {})):
            f, b = both(host_params(nat, *a, **kw), bits)
            assert f == b > 0, (bits, a, kw)
        p = host_params(nat, 2, 16, 1024, 1024, 72, 154)
        f, b = both(p, bits)
        assert f == b + 32 * 1024 * 32 * 4  # (B H N) rows of ntb = 32 words, a multiple of 256 B
        p.mask_out = 16
        assert both(p, bits)[0] == f
        f, b = both(host_params(nat, 2, 16, 1024, 1024, 72, 0, top_k=0), bits)
        assert f == b


# ---- the exact-result cases: the five conditions (exact_out_cases.CONDITIONS) ---------------------------------
@pytest.mark.parametrize("c", LC.EXACT + LC.EXACT_BF16, ids=LC.case_id)
def test_exact_cases_meet_the_five_conditions(c):
    for condition in EC.CONDITIONS:
        condition(c, EC.inputs(c), EC.reference(c), "int8")


@pytest.mark.parametrize("c", LC.EXACT4, ids=LC.case_id)
def test_exact4_cases_meet_the_five_conditions(c):
    for condition in EC.CONDITIONS:
        condition(c, A.exact_inputs(c), A.exact_reference(c), "int4")


# ---- the peaked random inputs: the eligible shares, from the oracle alone ---------------------------------
@pytest.mark.parametrize("c", LC.ROWS + LC.ROWS4, ids=LC.rcase_id)
def test_eligible_shares_within_caps(c):
    se, sr = LC.r_shares(c)
    msg = (f"{LC.rcase_id(c)}: eligible elements {se:.4%} of the cap {ELIGIBLE_ELEMS:.2%}, "
           f"rows {sr:.2%} of the cap {ELIGIBLE_ROWS:.0%}")
    print(msg)
    assert se <= ELIGIBLE_ELEMS and sr <= ELIGIBLE_ROWS, msg


def test_plain_rows_exceed_the_row_cap():
    """why the queries are peaked: plain standard_normal dense rows of 1,000 keys have an eligible
    element in over half of the rows"""
    c = LC._r(40, 1000, 72, 0, qmul=1.0)
    se, sr = LC.r_shares(c)
    assert sr > ELIGIBLE_ROWS, (se, sr)


# ---- the exact epilogue's branches ---------------------------------------------------------------------------
def test_epilogue_inputs_take_their_branch():
    fast, f64 = LC.epilogue_branches(*LC.epilogue_inputs("fast")[:2])
    assert fast.all() and not f64.any()
    fast, f64 = LC.epilogue_branches(*LC.epilogue_inputs("huge")[:2])
    assert fast.all() and not f64.any()
    q, k, _ = LC.epilogue_inputs("huge")
    t = O.attention(q, k, k, 0.125, top_k=False)["true"]
    assert 2.0 ** 38 < np.abs(t).max() < 2.0 ** 48
    fast, f64 = LC.epilogue_branches(*LC.epilogue_inputs("spread")[:2])
    assert (~fast).any() and fast.any() and f64.any()
    assert (~fast).any(-2).sum() < fast.shape[-1] * fast.shape[1] // 8  # (a few keys per head: the other tiles stay fast)
    fast, f64 = LC.epilogue_branches(*LC.epilogue_inputs("tiny")[:2])
    assert not fast.any() and f64.all()
