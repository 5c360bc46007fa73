"""float16 / bfloat16 on rows of 513 .. 4,096 keys (mxa_attention_dt) without a GPU: the exports and the host logic
that answers before any HIP call -- what the new entry point accepts, that it answers as mxa_attention_xl_full on every
float32 call, and that every older entry point keeps its refusal."""
import ctypes
import subprocess

import pytest

import long_dtype_cases as LD
from gpu_support import host_params
from test_xl_dense_cpu import answers
from test_xl_rows_cpu import ROOT, SHORT

ARG, UNSUPPORTED, WORKSPACE = -1, -2, -4  # include/mxa.h MXA_ERR_*
F32_SETS = SHORT + [(1, 16, T, T, 72, k, 1) for T, k in ((1025, 16), (1280, 20), (4096, 64), (4096, 1), (3840, 20))]


@pytest.fixture(scope="module")
def nat():
    from mx_quantization_amd import _native
    return _native


def dt_params(nat, c, mode=None):
    p = host_params(nat, LD.B, LD.H, LD.N, c.T, c.D, c.k, mode or c.mode, top_k=int(c.k != 0))
    p.dtype = {"f32": nat.DT_F32, "f16": nat.DT_F16, "bf16": nat.DT_BF16}[c.dt]
    p.score_dtype = {None: 0, "f16": nat.DT_F16, "bf16": nat.DT_BF16}[c.ac]
    return p


def test_exports(nat):
    header = open(ROOT + "/include/mxa.h").read()
    syms = subprocess.run(["nm", "-D", "--defined-only", nat.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in ("mxa_attention_dt_workspace_bytes", "mxa_attention_dt", "mxa_attention_dt_finish_kernel"):
        assert name + "(" in header and name in nat._SIGS and f" T {name}\n" in syms, name
    assert nat.ABI_VERSION == 6 and nat.lib().mxa_abi_version() == 6


@pytest.mark.parametrize("a", F32_SETS, ids=str)
def test_answers_as_xl_full_in_float32(nat, a):
    for bits in (8, 4):
        for top_k in {a[6], 0}:  # (and the set's dense branch)
            p = host_params(nat, *a[:6], top_k=top_k)
            assert answers(nat, "mxa_attention_dt", p, bits) == answers(nat, "mxa_attention_xl_full", p, bits), (bits, top_k)


@pytest.mark.parametrize("c", LD.CASES, ids=LD.case_id)
def test_accepts_the_16_bit_cases(nat, c):
    p, lib = dt_params(nat, c), nat.lib()
    status, size, kind = answers(nat, "mxa_attention_dt", p, 8)
    assert (status, kind) == (WORKSPACE, c.fin) and size > 0 and size % 256 == 0
    f32 = host_params(nat, LD.B, LD.H, LD.N, c.T, c.D, c.k, c.mode, top_k=int(c.k != 0))
    assert size == lib.mxa_attention_xl_full_workspace_bytes(ctypes.byref(f32), 8)  # codes are a byte each at every dtype
    for old in (lib.mxa_attention_xl_full, lib.mxa_attention_xl, lib.mxa_attention_full, lib.mxa_attention_bits):
        assert old(ctypes.byref(p), 8, None) == UNSUPPORTED
    assert lib.mxa_attention_long(ctypes.byref(p), None) == UNSUPPORTED
    assert lib.mxa_attention_dt(ctypes.byref(p), 4, None) == UNSUPPORTED  # MXINT4 with 16-bit tensors or scores


def test_refusals(nat):
    lib, f16 = nat.lib(), LD.CASES[0]
    dt = lambda p, bits=8: lib.mxa_attention_dt(ctypes.byref(p), bits, None)  # noqa: E731
    assert dt(dt_params(nat, f16._replace(T=100)), 4) == UNSUPPORTED  # MXINT4 at any length
    assert dt(dt_params(nat, f16._replace(T=100)), 8) == WORKSPACE
    elsa = dt_params(nat, f16._replace(T=2048, dt="f32"), "ELSA")
    elsa.N = 2048
    assert dt(elsa) == UNSUPPORTED  # ELSA on rows over 1,024 keys
    for T, k in ((2048, 65), (1279, 20), (4097, 20), (4097, 0)):  # k > 64, k * 64 > T, rows over 4,096 keys
        for d in ("f32", "f16"):
            assert dt(dt_params(nat, f16._replace(T=T, k=k, dt=d))) == UNSUPPORTED, (T, k, d)
    for mode in ("two_step_leading_ones", "true_ex"):  # approximators that are not exact in 16 bits
        assert dt(dt_params(nat, f16, mode)) == UNSUPPORTED, mode
    assert dt(host_params(nat, 1, 2, 33, 2048, 72, 20), 3) == ARG and lib.mxa_attention_dt_workspace_bytes(None, 8) == -1
