"""Top-k outside std::partial_sort's regime on rows of 1,025 .. 4,096 keys (mxa_attention_nth, mxa_topk_xl_nth)
without a GPU: the exports and the host logic that answers before any HIP call -- what the new entry point
accepts, what it still refuses, that it answers as mxa_attention_dt on that one's calls, and which kernel finishes."""
import ctypes
import subprocess

import pytest

from gpu_support import host_params
from test_long_dtype_cpu import F32_SETS
from test_xl_dense_cpu import answers
from test_xl_rows_cpu import ROOT

ARG, UNSUPPORTED, WORKSPACE = -1, -2, -4  # include/mxa.h MXA_ERR_*
GATHER16_XL, MFMA_XL = 8, 10               # ... MXA_FIN_*
# (T, k) of test_gpu_xl_nth.py and the issue's calls: k_top = 20 below 1,280 keys, --k 30, 64 below 4,096, 154
NTH = [(1025, 17), (1279, 20), (1919, 30), (2085, 64), (4095, 64), (2085, 65), (2048, 154), (4096, 154), (4096, 614), (4096, 4096)]


@pytest.fixture(scope="module")
def nat():
    from mx_quantization_amd import _native
    return _native


def params(nat, T, k, D=72, mode="ex_pred", dt=None):
    p = host_params(nat, 1, 2, 33, T, D, k, mode)
    if dt:
        p.dtype = dt
    return p


def test_exports(nat):
    header = open(ROOT + "/include/mxa.h").read()
    syms = subprocess.run(["nm", "-D", "--defined-only", nat.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in ("mxa_attention_nth_workspace_bytes", "mxa_attention_nth", "mxa_attention_nth_finish_kernel", "mxa_topk_xl_nth"):
        assert name + "(" in header and name in nat._SIGS and f" T {name}\n" in syms, name
    assert f"#define MXA_FIN_MFMA_XL {MFMA_XL}\n" in header and set(nat.FIN_KERNELS_NTH) == {MFMA_XL}
    assert nat.ABI_VERSION == 6 and nat.lib().mxa_abi_version() == 6


@pytest.mark.parametrize("a", F32_SETS, ids=str)
def test_answers_as_dt_on_its_calls(nat, a):
    for bits in (8, 4):
        for top_k in {a[6], 0}:
            p = host_params(nat, *a[:6], top_k=top_k)
            assert answers(nat, "mxa_attention_nth", p, bits) == answers(nat, "mxa_attention_dt", p, bits), (bits, top_k)


@pytest.mark.parametrize("T,k", NTH, ids=str)
@pytest.mark.parametrize("mode", ["ex_pred", "MXINT4", "two_step_leading_ones", "true_ex", "true"])
def test_accepts_the_nth_element_regime(nat, T, k, mode):
    lib = nat.lib()
    for bits in (8, 4):
        for D in (32, 72, 128):  # nbd 1 (the staged key records), 3 and 4 (the tables in the workspace)
            p = params(nat, T, k, D, "ex_pred" if mode == "true" else mode)
            p.approx = int(mode != "true")
            status, size, kind = answers(nat, "mxa_attention_nth", p, bits)
            assert (status, kind) == (WORKSPACE, GATHER16_XL if k <= 64 else MFMA_XL) and size > 0 and size % 256 == 0
            for old in ("mxa_attention_dt", "mxa_attention_xl_full", "mxa_attention_xl", "mxa_attention_full"):
                assert getattr(lib, old)(ctypes.byref(p), bits, None) == UNSUPPORTED, old


def test_workspace_of_k_over_64_does_not_depend_on_mask_out(nat):
    lib, p = nat.lib(), params(nat, 2085, 154)
    size = lib.mxa_attention_nth_workspace_bytes(ctypes.byref(p), 8)
    small = lib.mxa_attention_nth_workspace_bytes(ctypes.byref(params(nat, 2085, 64)), 8)
    p.mask_out = 256
    assert lib.mxa_attention_nth_workspace_bytes(ctypes.byref(p), 8) == size
    # (the mask words' region is there, beside the longer index lists: 66 rows of 66 words and of 154 - 64 uint16)
    assert size - small >= 66 * 66 * 4 + 66 * 90 * 2


def test_16_bit_dtypes(nat):
    lib = nat.lib()
    nth = lambda p, bits=8: lib.mxa_attention_nth(ctypes.byref(p), bits, None)  # noqa: E731
    for dt in (nat.DT_F16, nat.DT_BF16):
        p = params(nat, 1279, 20, dt=dt)
        assert answers(nat, "mxa_attention_nth", p, 8)[::2] == (WORKSPACE, GATHER16_XL)
        assert nth(p, 4) == UNSUPPORTED                                # MXINT4 with 16-bit tensors
        assert nth(params(nat, 2085, 154, dt=dt)) == UNSUPPORTED       # k_top > 64 with 16-bit tensors ...
        ac = params(nat, 2085, 154)
        ac.score_dtype = dt
        assert nth(ac) == UNSUPPORTED                                  # ... or scores


def test_refusals(nat):
    lib = nat.lib()
    nth = lambda p, bits=8: lib.mxa_attention_nth(ctypes.byref(p), bits, None)  # noqa: E731
    elsa = params(nat, 2048, 154, mode="ELSA")
    elsa.N = 2048
    assert nth(elsa) == UNSUPPORTED
    assert nth(params(nat, 4097, 154)) == UNSUPPORTED and nth(params(nat, 4097, 20)) == UNSUPPORTED
    assert nth(params(nat, 2085, 2086)) == ARG and nth(params(nat, 2085, 0)) == ARG  # k_top outside 1 .. T
    assert nth(params(nat, 2085, 154), 3) == ARG and lib.mxa_attention_nth_workspace_bytes(None, 8) == -1
    scores = params(nat, 2085, 154)  # no scores-only form on such rows: that entry point stops at 1,024 keys
    scores.pred_out = 256
    assert lib.mxa_approx_scores_bits(ctypes.byref(scores), 8, None) == UNSUPPORTED


def test_topk_xl_nth_host_answers(nat):
    lib = nat.lib()
    topk = lambda n, k, vals=256, idx=256, rows=0, dt=nat.DT_F32: lib.mxa_topk_xl_nth(vals, rows, n, n, k, idx, None, None, dt, None)  # noqa: E731
    for n, k in NTH + [(1100, 20), (2048, 128), (2048, 0)]:  # (rows == 0: accepted, nothing launched)
        assert topk(n, k) == 0, (n, k)
    assert topk(4097, 20) == UNSUPPORTED and topk(4097, 128) == UNSUPPORTED
    assert topk(2048, 2049) == ARG and topk(2048, -1) == ARG and topk(2048, 128, vals=None) == ARG
    assert topk(2048, 128, idx=None) == ARG and topk(2048, 128, dt=7) == ARG
    # ... and mxa_topk_xl's / mxa_topk's own answers where those accept or refuse on their arguments
    for n, k in ((4096, 64), (1280, 20), (1024, 500), (300, 20)):
        assert topk(n, k) == lib.mxa_topk_xl(256, 0, n, n, k, 256, None, None, nat.DT_F32, None) == 0
