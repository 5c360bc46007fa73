"""Rows of 1,025 .. 4,096 keys (mxa_attention_xl, mxa_topk_xl), the part that needs no GPU: the
exports, and the host logic that answers before any HIP call -- the statuses (a null workspace
is refused with MXA_ERR_WORKSPACE only after the refusals and both kernels' LDS plans have
passed) and the workspace sizes."""
import ctypes
import os
import subprocess

import pytest

from gpu_support import host_params

ARG, UNSUPPORTED, WORKSPACE = -1, -2, -4
GATHER16_XL = 8  # include/mxa.h MXA_FIN_GATHER16_XL
NEW = ("mxa_attention_xl_workspace_bytes", "mxa_attention_xl", "mxa_attention_xl_finish_kernel", "mxa_topk_xl")
MODES = ["ex_pred", "partial_Q", "MXINT4", "two_step_leading_ones", "true_ex"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (B, H, N, T, D, k, top_k): rows of at most 1,024 keys, every finishing kernel of mxa_attention_full
SHORT = [(256, 12, 197, 197, 64, 20, 1), (64, 16, 256, 256, 72, 154, 1), (1, 2, 100, 300, 64, 20, 0), (2, 16, 1024, 1024, 72, 20, 1),
         (2, 16, 1024, 1024, 72, 154, 1), (1, 2, 40, 600, 64, 0, 0), (1, 2, 100, 300, 64, 100, 1), (1, 1, 10, 60, 160, 5, 1)]


@pytest.fixture(scope="module")
def nat():
    from mx_quantization_amd import _native
    return _native


def _xl(nat, p, bits=8):
    return nat.lib().mxa_attention_xl(ctypes.byref(p), bits, None)


def test_exports(nat):
    header = open(os.path.join(ROOT, "include", "mxa.h")).read()
    syms = subprocess.run(["nm", "-D", "--defined-only", nat.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NEW:
        assert name + "(" in header and name in nat._SIGS and f" T {name}\n" in syms, name
    assert f"#define MXA_FIN_GATHER16_XL {GATHER16_XL}\n" in header and set(nat.FIN_KERNELS_XL) == {GATHER16_XL}
    assert nat.ABI_VERSION == 6 and nat.lib().mxa_abi_version() == 6


@pytest.mark.parametrize("a", SHORT, ids=str)
def test_answers_as_full_up_to_1024_keys(nat, a):
    lib = nat.lib()
    for bits in (8, 4, 3):
        for mode in ("ex_pred", "ELSA"):
            p = host_params(nat, *a[:6], mode, top_k=a[6])
            r = ctypes.byref(p)
            assert _xl(nat, p, bits) == lib.mxa_attention_full(r, bits, None), (bits, mode)
            assert lib.mxa_attention_xl_workspace_bytes(r, bits) == lib.mxa_attention_full_workspace_bytes(r, bits)
            assert lib.mxa_attention_xl_finish_kernel(r, bits) == lib.mxa_attention_full_finish_kernel(r, bits)


@pytest.mark.parametrize("T,k", [(1025, 16), (1280, 20), (4096, 64), (4096, 1), (3840, 20)])
def test_accepts_the_partial_sort_regime(nat, T, k):
    lib = nat.lib()
    sizes = set()
    for bits in (8, 4):
        for D in (32, 72, 128):
            for mode in MODES:
                p = host_params(nat, 1, 16, T, T, D, k, mode)
                assert _xl(nat, p, bits) == WORKSPACE, (bits, D, mode)
                assert lib.mxa_attention_xl_finish_kernel(ctypes.byref(p), bits) == GATHER16_XL
                p.approx = 0  # top-k on the true scores
                assert _xl(nat, p, bits) == WORKSPACE, (bits, D, mode, "approx=0")
        p = host_params(nat, 1, 16, T, T, 72, k)
        sizes.add(lib.mxa_attention_xl_workspace_bytes(ctypes.byref(p), bits))
        p.mask_out = 16  # the gather kernel reads the kept indices: no mask words held, whatever mask_out is
        sizes.add(lib.mxa_attention_xl_workspace_bytes(ctypes.byref(p), bits))
        for old in (lib.mxa_attention_full, lib.mxa_attention_bits):  # the siblings keep their refusal
            assert old(ctypes.byref(p), bits, None) == UNSUPPORTED
        assert lib.mxa_attention_long(ctypes.byref(p), None) == UNSUPPORTED
    (size,) = sizes
    # at least Q's and K's codes (D padded to 96) and V's transposed codes (T padded to 32-key blocks)
    assert size >= 16 * (2 * T * 96 + 72 * ((T + 31) // 32 * 32)) and size % 256 == 0


def test_refusals(nat):
    lib = nat.lib()
    for bits in (8, 4):
        for T, k in ((1279, 20), (4096, 65), (4097, 20), (1025, 17), (2048, 33)):
            assert _xl(nat, host_params(nat, 1, 2, 33, T, 72, k), bits) == UNSUPPORTED, (T, k)
        assert _xl(nat, host_params(nat, 1, 2, 33, 2048, 72, 0, top_k=0), bits) == UNSUPPORTED  # the dense branch
        for field in ("dtype", "score_dtype"):  # float16 tensors / autocast
            p = host_params(nat, 1, 2, 33, 2048, 72, 20)
            setattr(p, field, nat.DT_F16)
            assert _xl(nat, p, bits) == UNSUPPORTED, field
        assert _xl(nat, host_params(nat, 1, 2, 2048, 2048, 72, 20, "ELSA"), bits) == UNSUPPORTED
        xq = nat.QkvParams()  # a fused projection: the *_full blocks stop at 1,024 keys
        xq.x = xq.wq = 16
        xq.C = xq.x_row_stride = 96
        p = host_params(nat, 1, 2, 2048, 2048, 72, 20)
        assert lib.mxa_qkv_attention_full(ctypes.byref(p), ctypes.byref(xq), bits, None) == UNSUPPORTED
    assert _xl(nat, host_params(nat, 1, 2, 33, 2048, 72, 0), 8) == ARG  # k_top = 0 on the top-k branch
    assert _xl(nat, host_params(nat, 1, 2, 33, 2048, 72, 20), 3) == ARG
    assert lib.mxa_attention_xl_workspace_bytes(None, 8) == -1


def test_topk_xl_statuses(nat):
    xl = lambda rows, n, k, dt=0: nat.lib().mxa_topk_xl(16, rows, n, n, k, 16, None, None, dt, None)
    assert xl(1, 4097, 20) == UNSUPPORTED and xl(1, 1279, 20) == UNSUPPORTED
    assert xl(1, 4096, 65) == UNSUPPORTED and xl(1, 2048, 0) == UNSUPPORTED
    assert xl(1, 2048, 2049) == ARG and xl(1, 2048, 20, 3) == ARG
    for n, k in ((1025, 16), (4096, 64), (600, 5)):  # no rows: accepted, nothing launched (n <= 1,024: mxa_topk's answer)
        assert xl(0, n, k) == 0
    assert nat.lib().mxa_topk(16, 1, 1025, 1025, 16, 16, None, None, 0, None) == UNSUPPORTED  # mxa_topk keeps its bound
