"""Rows of 4,097 .. 16,384 keys (mxa_attention_xxl, mxa_topk_xxl) without a GPU: the exports and the host logic
that answers before any HIP call -- the predecessors' answers up to 4,096 keys, the finishing kernel of the new
rows, every refusal of the out-of-scope list, and the older entry points' unchanged bound."""
import ctypes
import subprocess

import pytest

from gpu_support import host_params
from test_long_dtype_cpu import F32_SETS
from test_xl_dense_cpu import answers
from test_xl_nth_cpu import NTH, params
from test_xl_rows_cpu import MODES, ROOT

ARG, UNSUPPORTED, WORKSPACE = -1, -2, -4  # include/mxa.h MXA_ERR_*
GATHER16_XXL = 12                          # ... MXA_FIN_GATHER16_XXL
XXL = [(4097, 16), (4097, 64), (5000, 20), (9249, 20), (16384, 20), (16384, 64), (16383, 1)]  # test_gpu_xxl_rows.py's


@pytest.fixture(scope="module")
def nat():
    from mx_quantization_amd import _native
    return _native


def test_exports(nat):
    header = open(ROOT + "/include/mxa.h").read()
    syms = subprocess.run(["nm", "-D", "--defined-only", nat.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in ("mxa_attention_xxl_workspace_bytes", "mxa_attention_xxl", "mxa_attention_xxl_finish_kernel", "mxa_topk_xxl"):
        assert name + "(" in header and name in nat._SIGS and f" T {name}\n" in syms, name
    assert f"#define MXA_FIN_GATHER16_XXL {GATHER16_XXL}\n" in header and set(nat.FIN_KERNELS_XXL) == {GATHER16_XXL}
    assert nat.ABI_VERSION == 6 and nat.lib().mxa_abi_version() == 6


@pytest.mark.parametrize("a", F32_SETS, ids=str)
def test_answers_as_nth_dt_up_to_4096_keys(nat, a):
    for bits in (8, 4, 3):
        for top_k in {a[6], 0}:
            p = host_params(nat, *a[:6], top_k=top_k)
            assert answers(nat, "mxa_attention_xxl", p, bits) == answers(nat, "mxa_attention_nth_dt", p, bits), (bits, top_k)
    for T, k in NTH:  # ... outside partial_sort's regime, float32 and 16-bit
        for dt in (None, nat.DT_F16):
            p = params(nat, T, k, dt=dt)
            assert answers(nat, "mxa_attention_xxl", p, 8) == answers(nat, "mxa_attention_nth_dt", p, 8), (T, k, dt)


@pytest.mark.parametrize("T,k", XXL, ids=str)
def test_accepts_the_new_rows(nat, T, k):
    """a null workspace is refused only after the refusals and both kernels' LDS plans have passed"""
    lib = nat.lib()
    sizes = set()
    for bits in (8, 4):
        for D in (32, 72, 128):
            for mode in MODES:
                p = params(nat, T, k, D, mode)
                assert answers(nat, "mxa_attention_xxl", p, bits)[::2] == (WORKSPACE, GATHER16_XXL), (bits, D, mode)
                p.approx = 0  # top-k on the true scores
                assert lib.mxa_attention_xxl(ctypes.byref(p), bits, None) == WORKSPACE, (bits, D, mode, "approx=0")
        p = params(nat, T, k)
        sizes.add(lib.mxa_attention_xxl_workspace_bytes(ctypes.byref(p), bits))
        p.mask_out = 16  # the gather kernel reads the kept indices: no mask words held
        sizes.add(lib.mxa_attention_xxl_workspace_bytes(ctypes.byref(p), bits))
        for old in ("mxa_attention_nth_dt", "mxa_attention_nth", "mxa_attention_dt", "mxa_attention_xl"):  # the siblings keep their bound
            assert getattr(lib, old)(ctypes.byref(p), bits, None) == UNSUPPORTED, old
    (size,) = sizes
    # at least Q's and K's codes (D padded to 96) and V's transposed codes (T padded to 32-key blocks), two heads
    assert size >= 2 * ((33 + T) * 96 + 72 * ((T + 31) // 32 * 32)) and size % 256 == 0


def test_workspace_is_sized_in_64_bits(nat):
    p = host_params(nat, 32, 16, 16384, 16384, 72, 20)  # Q's and K's codes (D padded to 96) and V's: over 2^31 B
    assert nat.lib().mxa_attention_xxl_workspace_bytes(ctypes.byref(p), 8) > 32 * 16 * 16384 * (2 * 96 + 72) > 2 ** 31


def test_refusals(nat):
    lib = nat.lib()
    xxl = lambda p, bits=8: lib.mxa_attention_xxl(ctypes.byref(p), bits, None)  # noqa: E731
    for bits in (8, 4):
        for T, k in ((4097, 65), (4097, 0), (5000, 79), (16384, 65), (16384, 154), (16385, 20), (20000, 1)):
            want = ARG if k == 0 else UNSUPPORTED  # (k_top = 0 on the top-k branch is a bad argument at every length)
            assert xxl(params(nat, T, k), bits) == want, (T, k)
        assert xxl(host_params(nat, 1, 2, 33, 8192, 72, 0, top_k=0), bits) == UNSUPPORTED  # the dense branch
        for field in ("dtype", "score_dtype"):  # float16 / bfloat16 tensors, autocast scores
            for dt in (nat.DT_F16, nat.DT_BF16):
                p = params(nat, 8192, 20)
                setattr(p, field, dt)
                assert xxl(p, bits) == UNSUPPORTED, (field, dt)
        assert xxl(host_params(nat, 1, 2, 8192, 8192, 72, 20, "ELSA"), bits) == UNSUPPORTED
        p = params(nat, 8192, 20)
        p.pred_out = 16  # the scores alone
        assert lib.mxa_approx_scores_bits(ctypes.byref(p), bits, None) == UNSUPPORTED
        xq, pj, xc = nat.QkvParams(), nat.ProjParams(), nat.CrossParams()  # every fused projection
        xq.x = xq.wq = pj.wq = pj.y = xc.x = xc.cond = xc.wq_q = xc.wq_kv = 16
        xq.C = xq.x_row_stride = xc.C = xc.C_kv = xc.x_row_stride = xc.cond_row_stride = pj.out_features = pj.y_row_stride = 96
        p = host_params(nat, 1, 2, 8192, 8192, 72, 20)
        assert lib.mxa_qkv_attention_full(ctypes.byref(p), ctypes.byref(xq), bits, None) == UNSUPPORTED
        assert lib.mxa_attention_proj_full(ctypes.byref(p), None, ctypes.byref(pj), bits, None) == UNSUPPORTED
        assert lib.mxa_cross_attention_bits(ctypes.byref(p), ctypes.byref(xc), None, bits, None) == UNSUPPORTED
    assert xxl(params(nat, 8192, 20), 3) == ARG
    assert lib.mxa_attention_xxl_workspace_bytes(None, 8) == -1


def test_topk_xxl_statuses(nat):
    lib = nat.lib()
    call = lambda name, rows, n, k, dt=0: getattr(lib, name)(16, rows, n, n, k, 16, None, None, dt, None)  # noqa: E731
    xxl = lambda *a: call("mxa_topk_xxl", *a)  # noqa: E731
    assert xxl(1, 16385, 20) == UNSUPPORTED and xxl(1, 4097, 65) == UNSUPPORTED
    assert xxl(1, 5000, 79) == UNSUPPORTED and xxl(1, 8192, 0) == UNSUPPORTED
    assert xxl(1, 8192, 8193) == ARG and xxl(1, 8192, 20, 3) == ARG
    for n, k in XXL + [(4096, 64), (4096, 154), (1280, 20), (600, 5)]:  # no rows: accepted, nothing launched
        assert xxl(0, n, k) == 0
    for n, k in ((4096, 65), (2085, 0), (2085, 2086), (1100, 3)):  # up to 4,096 values: mxa_topk_xl_nth's answer
        assert xxl(0, n, k) == call("mxa_topk_xl_nth", 0, n, k)
    assert call("mxa_topk_xl_nth", 1, 4097, 20) == UNSUPPORTED and call("mxa_topk_xl", 1, 4097, 20) == UNSUPPORTED
