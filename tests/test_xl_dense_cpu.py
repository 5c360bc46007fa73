"""The dense branch on rows of 1,025 .. 4,096 keys (mxa_attention_xl_full) without a GPU: the exports, the host logic that answers before
any HIP call, and what test_gpu_xl_dense.py relies on -- the exact cases' five conditions, the exact epilogue's branch per special input."""
import ctypes
import subprocess

import pytest

import attn4_cases as A
import exact_out_cases as EC
import long_dense_cases as LC
from gpu_support import host_params
from test_xl_rows_cpu import ROOT, SHORT

UNSUPPORTED, WORKSPACE, DENSE_MFMA_XL = -2, -4, 9  # include/mxa.h MXA_ERR_*, MXA_FIN_DENSE_MFMA_XL
EXACT8 = [EC._c(EC.DENSE_MFMA, 1, 2, 33, T, D, 0) for T in (1025, 2085, 4096) for D in (32, 72, 128)]
EXACT8 += [EC._c(EC.DENSE_MFMA, 2, 2, 33, 2085, 72, 0, True), EC._c(EC.DENSE_MFMA, 1, 2, 33, 4096, 72, 0, bfloat=16)]
EXACT4 = [EC._c(EC.DENSE_MFMA, 1, 2, 33, T, 72, 0) for T in (2085, 4096)]


@pytest.fixture(scope="module")
def nat():
    from mx_quantization_amd import _native
    return _native


def answers(nat, name, p, bits):  # (status on a null workspace, workspace size, finishing kernel)
    lib, r = nat.lib(), ctypes.byref(p)
    return getattr(lib, name)(r, bits, None), getattr(lib, name + "_workspace_bytes")(r, bits), getattr(lib, name + "_finish_kernel")(r, bits)


def test_exports(nat):
    header = open(ROOT + "/include/mxa.h").read()
    syms = subprocess.run(["nm", "-D", "--defined-only", nat.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in ("mxa_attention_xl_full_workspace_bytes", "mxa_attention_xl_full", "mxa_attention_xl_full_finish_kernel"):
        assert name + "(" in header and name in nat._SIGS and f" T {name}\n" in syms, name
    assert f"#define MXA_FIN_DENSE_MFMA_XL {DENSE_MFMA_XL}\n" in header and set(nat.FIN_KERNELS_XL_FULL) == {DENSE_MFMA_XL}


@pytest.mark.parametrize("T", [1025, 3840, 4096])
def test_accepts_the_dense_branch(nat, T):
    for bits in (8, 4):
        for D in (32, 72, 128):
            p = host_params(nat, 1, 2, 33, T, D, 0, top_k=0)
            status, size, kind = answers(nat, "mxa_attention_xl_full", p, bits)
            assert (status, kind) == (WORKSPACE, DENSE_MFMA_XL) and size > 0 and size % 256 == 0, (bits, D)
            p.mask_out = 16  # no mask words are held for it, whatever mask_out is
            assert nat.lib().mxa_attention_xl_full_workspace_bytes(ctypes.byref(p), bits) == size
            for old in (nat.lib().mxa_attention_xl, nat.lib().mxa_attention_full, nat.lib().mxa_attention_bits):  # the siblings keep their refusal
                assert old(ctypes.byref(p), bits, None) == UNSUPPORTED, (bits, D)


@pytest.mark.parametrize("a", SHORT + [(1, 16, T, T, 72, k, 1) for T, k in ((1025, 16), (1280, 20), (4096, 64), (4096, 1), (3840, 20))], ids=str)
def test_answers_as_xl(nat, a):
    for bits in (8, 4):
        p = host_params(nat, *a[:6], top_k=a[6])
        assert answers(nat, "mxa_attention_xl_full", p, bits) == answers(nat, "mxa_attention_xl", p, bits), bits


def test_refusals(nat):
    f16 = host_params(nat, 1, 2, 33, 2048, 72, 0, top_k=0)
    f16.dtype = nat.DT_F16  # (the library reads the tensors' dtype from the parameters)
    for p in (host_params(nat, 1, 2, 33, 4097, 72, 0, top_k=0), host_params(nat, 1, 2, 33, 4097, 72, 20), f16,
              host_params(nat, 1, 2, 33, 2048, 72, 65), host_params(nat, 1, 2, 2048, 2048, 72, 0, "ELSA", top_k=0)):
        for bits in (8, 4):
            assert nat.lib().mxa_attention_xl_full(ctypes.byref(p), bits, None) == UNSUPPORTED, (p.T, p.k_top, bits)


@pytest.mark.parametrize("c,bits", [(c, 8) for c in EXACT8] + [(c, 4) for c in EXACT4], ids=str)
def test_exact_cases_meet_the_five_conditions(c, bits):
    inputs, r = (EC.inputs(c), EC.reference(c)) if bits == 8 else (A.exact_inputs(c), A.exact_reference(c))
    for condition in EC.CONDITIONS:
        condition(c, inputs, r, f"int{bits}")


def test_epilogue_inputs_take_their_branch_in_every_chunk():
    fast, f64 = LC.epilogue_branches(*LC.epilogue_inputs("spread", T=2085)[:2])
    for chunk in (slice(0, 1024), slice(1024, 2048), slice(2048, 2085)):
        assert (~fast[..., chunk]).any() and fast[..., chunk].any() and f64[..., chunk].any()
    fast, f64 = LC.epilogue_branches(*LC.epilogue_inputs("tiny", T=2085)[:2])
    assert not fast.any() and f64.all() and fast.shape[-1] == 2085
