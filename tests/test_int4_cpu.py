"""MXINT4 Linear / MLP without a GPU: the two width-taking exports, their argument refusals
(before any HIP call), the drop-in's routing as a function of the specs, the reference fixture
against the oracle, and -- for every input of tests/int4_cases.py -- the side of the one-digit
kernel's gate every row block sits on, from the oracle's block exponents alone."""
import os

import numpy as np
import pytest
import torch

import int4_cases as C
from gpu_support import G
from oracle import mx_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def P():
    return np.load(os.path.join(G, "linear_int4.npz"))


def test_exports_and_header_agree():
    import re
    from mx_quantization_amd import _native as N
    lib = N.lib()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mxa.h")).read(), flags=re.S)
    for fn, nargs in (("mxa_linear_weight_bytes_bits", 4), ("mxa_linear_weight_prep_bits", 9)):
        assert fn in N.EXPORTS and hasattr(lib, fn)
        assert len(N._SIGS[fn][1]) == nargs
        m = re.search(r"\b" + fn + r"\s*\(([^)]*)\)", hdr)
        assert m and len(m.group(1).split(",")) == nargs, fn
    assert lib.mxa_abi_version() == N.ABI_VERSION == 6


@pytest.mark.parametrize("out_f,in_f,gw", [(160, 96, 160), (1152, 4608, 1152), (3456, 1152, 72), (48, 100, 24)])
def test_weight_bytes(out_f, in_f, gw):
    """elem_bits 8 is mxa_linear_weight_bytes; the 4-bit buffer is smaller by one digit plane"""
    from mx_quantization_amd import _native as N
    lib = N.lib()
    b8, b4 = lib.mxa_linear_weight_bytes_bits(out_f, in_f, gw, 8), lib.mxa_linear_weight_bytes_bits(out_f, in_f, gw, 4)
    assert b8 == lib.mxa_linear_weight_bytes(out_f, in_f, gw) > 0
    pcols, cpad = out_f // gw * ((gw + 31) // 32) * 32, (in_f + 31) // 32 * 32
    al = lambda n: (n + 255) // 256 * 256  # noqa: E731
    assert b8 - b4 == al(2 * pcols * cpad) - al(pcols * cpad) > 0


def test_argument_refusals_without_gpu():
    """every refusal returns before any HIP call (this machine has no device to call)"""
    from mx_quantization_amd import _native as N
    lib = N.lib()
    for bits in (0, 2, 5, 6, 16, -4):
        assert lib.mxa_linear_weight_bytes_bits(64, 32, 64, bits) == -1
    assert lib.mxa_linear_weight_bytes_bits(64, 32, 48, 4) == -1  # group width does not divide
    assert lib.mxa_linear_weight_bytes_bits(0, 32, 1, 4) == -1
    w = torch.zeros(64, 32)
    buf = torch.zeros(lib.mxa_linear_weight_bytes_bits(64, 32, 64, 8) + 16, dtype=torch.uint8)
    p = (buf.data_ptr() + 15) // 16 * 16
    for bits in (0, 2, 5, 6, 16):
        assert lib.mxa_linear_weight_prep_bits(w.data_ptr(), 64, 32, 64, 0, 0, bits, p, None) == -1
    assert lib.mxa_linear_weight_prep_bits(None, 64, 32, 64, 0, 0, 4, p, None) == -1
    assert lib.mxa_linear_weight_prep_bits(w.data_ptr(), 64, 32, 64, 0, 0, 4, None, None) == -1
    assert lib.mxa_linear_weight_prep_bits(w.data_ptr(), 64, 32, 48, 0, 0, 4, p, None) == -1
    assert lib.mxa_linear_weight_prep_bits(w.data_ptr(), 64, 32, 64, 0, 9, 4, p, None) == -1  # bfloat 9
    assert lib.mxa_linear_weight_prep_bits(w.data_ptr(), 64, 32, 64, 0, 0, 4, p + 4, None) == -1  # misaligned


def test_python_refusals_without_gpu():
    import mx_quantization_amd as M
    with pytest.raises(ValueError):
        M.LinearWeightMX(torch.zeros(64, 32), 64, elem_bits=5)
    with pytest.raises(M.NativeError):  # (a valid width: the CPU tensor is what is refused)
        M.LinearWeightMX(torch.zeros(64, 32), 64, elem_bits=4)
    with pytest.raises(M.NativeError):
        M.mx_linear(torch.zeros(8, 32), torch.zeros(64, 32), elem_bits=4)
    with pytest.raises(M.NativeError):
        M.mx_mlp(torch.zeros(8, 32), torch.zeros(64, 32), None, torch.zeros(16, 64), None, elem_bits=4)


def test_dropin_routing_is_a_function_of_the_specs():
    """mx.Linear's prepared-weight route: both formats int8 or both int4, nearest roundings"""
    from mx_quantization_amd.mx.linear import fused_elem_bits
    from mx_quantization_amd.mx.specs import apply_mx_specs
    s = lambda **kw: apply_mx_specs(dict(C.SPECS, **kw))  # noqa: E731
    assert fused_elem_bits(s()) == 4
    assert fused_elem_bits(s(bfloat=32)) == 4
    assert fused_elem_bits(s(w_elem_format="int8", a_elem_format="int8")) == 8
    assert fused_elem_bits(s(w_elem_format="int8")) == 0  # W8A4
    assert fused_elem_bits(s(a_elem_format="int8")) == 0  # W4A8
    assert fused_elem_bits(s(round_output="floor")) == 0
    assert fused_elem_bits(s(round_weight="even")) == 0


def test_oracle_equals_the_reference_fixture(P):
    """the reference's mx.Linear under its PixArt int4 specs == O.mx_linear(elem="int4"), bit for bit"""
    for i in range(3):
        x, W, b = C.golden_linear(P, i)
        for bf in (16, 32):
            C.same_bits(O.mx_linear(x, W, b, elem="int4", bfloat=bf), P[f"lin{i}/y_bf{bf}"], f"lin{i} bfloat {bf}")
    x, W1, b1, W2, b2 = C.golden_mlp(P)
    for bf in (16, 32):
        C.same_bits(O.mx_linear(x, W1, b1, elem="int4", bfloat=bf), P[f"mlp/pre_bf{bf}"], f"mlp pre bfloat {bf}")
        C.same_bits(O.mx_linear(P[f"mlp/act_bf{bf}"], W2, b2, elem="int4", bfloat=bf), P[f"mlp/y_bf{bf}"],
                    f"mlp y bfloat {bf}")


# ---- the side of the gate, every row block of every case --------------------------------------
def test_plain_cases_sit_on_the_digit_path(P):
    for rows, inf, outf in ((33, 96, 40), (70, 256, 64)):
        x, W, _ = C.linear_case(rows, inf, outf, inf)
        for bf in (32, 16):
            C.assert_side(x, W, "digits", bf, what=(rows, inf, outf, bf))
    for i in range(3):
        x, W, _ = C.golden_linear(P, i)
        for bf in (32, 16):
            C.assert_side(x, W, "digits", bf, what=f"lin{i}")
    x, W1, _, _, _ = C.golden_mlp(P)
    C.assert_side(x, W1, "digits", what="mlp fc1")


@pytest.mark.parametrize("name", sorted(C.EDGES))
def test_gate_edges(name):
    x, W = C.edge(name)
    nd, n = C.assert_edge(name, x, W)
    assert n == 3 and nd == (3 if C.EDGES[name][3] == "digits" else 0)
    if name == "gate_m155":  # far below the gate the results themselves are subnormal
        y = O.mx_linear(x, W, None, elem="int4")
        assert ((np.abs(y) < np.float32(2.0 ** -126)) & (y != 0)).any()


@pytest.mark.parametrize("alternate", [False, True])
def test_accumulator_case(alternate):
    x, W = C.accumulator(alternate)
    big = C.assert_accumulator(x, W, alternate)
    print("largest |accumulator|", big)


@pytest.mark.parametrize("inf", C.K_EDGE_IN)
def test_k_edge_case(inf):
    x, W, _ = C.k_edge(inf)
    C.assert_k_edge(inf, x, W)


@pytest.mark.parametrize("rows,inf,hid,outf", C.MLP_SHAPES)
def test_mlp_cases_fc1_on_the_digit_path(rows, inf, hid, outf):
    x, W1, b1, W2, b2 = C.mlp_case(rows, inf, hid, outf, rows * 13 + hid)
    C.assert_side(x, W1, "digits", what="fc1")
