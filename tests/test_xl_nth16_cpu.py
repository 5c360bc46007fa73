"""float16 / bfloat16 top-k with k_top > 64 on rows of 1,025 .. 4,096 keys (mxa_attention_nth_dt) without a GPU: the
exports and the host logic that answers before any HIP call -- mxa_attention_nth's answers on its calls and on every
float32 call, the finishing kernel of the 16-bit calls, and what is still refused."""
import ctypes
import subprocess

import pytest

from gpu_support import host_params
from test_long_dtype_cpu import F32_SETS
from test_xl_dense_cpu import answers
from test_xl_nth_cpu import NTH, params
from test_xl_rows_cpu import ROOT

ARG, UNSUPPORTED, WORKSPACE = -1, -2, -4  # include/mxa.h MXA_ERR_*
GATHER16_XL, MFMA_XL, GATHER_XL = 8, 10, 11  # ... MXA_FIN_*


@pytest.fixture(scope="module")
def nat():
    from mx_quantization_amd import _native
    return _native


def params16(nat, T, k, D, dt, autocast, mode="ex_pred"):
    """16-bit tensors, or float32 tensors under a 16-bit autocast"""
    p = params(nat, T, k, D, mode, None if autocast else dt)
    p.score_dtype = dt if autocast else 0
    return p


def test_exports(nat):
    header = open(ROOT + "/include/mxa.h").read()
    syms = subprocess.run(["nm", "-D", "--defined-only", nat.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in ("mxa_attention_nth_dt_workspace_bytes", "mxa_attention_nth_dt", "mxa_attention_nth_dt_finish_kernel"):
        assert name + "(" in header and name in nat._SIGS and f" T {name}\n" in syms, name
    assert f"#define MXA_FIN_GATHER_XL {GATHER_XL}\n" in header and set(nat.FIN_KERNELS_NTH_DT) == {GATHER_XL}


@pytest.mark.parametrize("a", F32_SETS, ids=str)
def test_answers_as_nth_on_its_calls(nat, a):
    for bits in (8, 4):
        for top_k in {a[6], 0}:
            p = host_params(nat, *a[:6], top_k=top_k)
            assert answers(nat, "mxa_attention_nth_dt", p, bits) == answers(nat, "mxa_attention_nth", p, bits), (bits, top_k)


@pytest.mark.parametrize("T,k", NTH, ids=str)
def test_float32_calls_keep_their_kernels(nat, T, k):
    for bits in (8, 4):
        for D in (32, 72, 128):
            p = params(nat, T, k, D)
            got = answers(nat, "mxa_attention_nth_dt", p, bits)
            assert got == answers(nat, "mxa_attention_nth", p, bits) and got[::2] == (WORKSPACE, GATHER16_XL if k <= 64 else MFMA_XL)
    for dt in (nat.DT_F16, nat.DT_BF16):  # ... and the 16-bit calls mxa_attention_nth serves (k_top <= 64)
        p = params(nat, T, min(k, 64), dt=dt)
        assert answers(nat, "mxa_attention_nth_dt", p, 8) == answers(nat, "mxa_attention_nth", p, 8)


@pytest.mark.parametrize("autocast", [False, True])
@pytest.mark.parametrize("T", [1025, 2085, 4096])
def test_16_bit_kernels(nat, T, autocast):
    lib = nat.lib()
    for dt in (nat.DT_F16, nat.DT_BF16):
        for D in (32, 72, 128):
            for k, kind in ((65, GATHER_XL), (154, GATHER_XL), (256, GATHER_XL), (257, MFMA_XL), (T, MFMA_XL)):
                p = params16(nat, T, k, D, dt, autocast)
                status, size, got = answers(nat, "mxa_attention_nth_dt", p, 8)
                assert (status, got) == (WORKSPACE, kind) and size > 0 and size % 256 == 0, (dt, D, k)
                assert lib.mxa_attention_nth(ctypes.byref(p), 8, None) == UNSUPPORTED
                assert lib.mxa_attention_nth_dt(ctypes.byref(p), 4, None) == UNSUPPORTED  # MXINT4 at 16 bits


def test_gather_reserves_no_mask_words(nat):
    lib, size = nat.lib(), {}
    for k in (256, 257):  # the masked kernel's call holds 66 rows of 66 mask words more than one index a row
        size[k] = lib.mxa_attention_nth_dt_workspace_bytes(ctypes.byref(params(nat, 2085, k, dt=nat.DT_BF16)), 8)
    assert size[257] - size[256] >= 66 * 66 * 4


def test_refusals(nat):
    lib = nat.lib()
    nth = lambda p, bits=8: lib.mxa_attention_nth_dt(ctypes.byref(p), bits, None)  # noqa: E731
    elsa = params(nat, 2048, 154, mode="ELSA", dt=nat.DT_BF16)
    elsa.N = 2048
    assert nth(elsa) == UNSUPPORTED
    elsa.dtype = nat.DT_F32
    assert nth(elsa) == UNSUPPORTED
    for k in (20, 154, 300):
        assert nth(params(nat, 4097, k, dt=nat.DT_F16)) == UNSUPPORTED
    assert nth(params(nat, 2085, 2086, dt=nat.DT_F16)) == ARG and nth(params(nat, 2085, 154, dt=nat.DT_F16), 3) == ARG
    assert lib.mxa_attention_nth_dt_workspace_bytes(None, 8) == -1
    scores = params(nat, 2085, 154, dt=nat.DT_BF16)  # no scores-only form on such rows
    scores.pred_out = 256
    assert lib.mxa_approx_scores_bits(ctypes.byref(scores), 8, None) == UNSUPPORTED
